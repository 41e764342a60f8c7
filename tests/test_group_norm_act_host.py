"""pdr_group_norm_act / pdr_group_norm_act_grad without a GPU: the host-only plan and workspace size, the documented
order of the argument checks (nothing is launched, no pointer is looked at before its turn), the Python surface's
refusal of CPU tensors, the process-wide switch, the module path's unchanged bits and parameter names with the switch
off, and a check that the bounds of tests/group_norm_act_cases.py discriminate: the float64 reference rounded to fp32
passes them, five plausible wrong implementations do not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule, MyGroupNorm
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import Mlp_plus_t_emb, Swish, build_shared_mlp
from tests import group_norm_act_cases as GC

OK, EINVAL, EUNSUP = _lib.PDR_OK, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED


def test_plan_reports_family_partitions_and_channels_per_group():
    # small slabs: one partition of the smallest size; the family follows S % 4 and the alignment flag
    for C, S, G, fam, Cg in [(32, 1, 32, 0, 1), (35, 7, 32, 0, 1), (64, 12, 32, 1, 2), (67, 33, 32, 0, 2),
                             (131, 260, 32, 1, 4), (16, 20, 16, 1, 1), (10, 8, 4, 1, 2), (512, 512, 32, 1, 16)]:
        assert GC.plan(C, S, G, 1) == (OK, [fam, 1, 8192, Cg]), (C, S, G)
        assert GC.plan(C, S, G, 0) == (OK, [0, 1, 8192, Cg]), (C, S, G)
    # partitions from m = Cg S alone: E = max(8192, ceil(m / 32) rounded up to 1024), P = ceil(m / E) <= 32
    for C, S, G in [(32, 8192, 32), (32, 8193, 32), (32, 16385, 32), (64, 32768, 32), (128, 32768, 32),
                    (512, 16384, 32), (35, 999999, 32), (32, 1 << 24, 32)]:
        rc, (fam, P, E, Cg) = GC.plan(C, S, G, 1)
        m = Cg * S
        want_E = max(8192, -(-(-(-m // 32)) // 1024) * 1024)
        assert rc == OK and Cg == (C - C % G) // G and fam == int(S % 4 == 0)
        assert E == want_E and P == -(-m // E) and 1 <= P <= 32 and E % 1024 == 0 and (P - 1) * E < m <= P * E
        assert GC.plan(2 * C, S, 2 * G, 1)[1][1:] == [P, E, Cg]            # the same (Cg, S): the same cut
    assert GC.plan(32, 8192, 32)[1][1] == 1 and GC.plan(32, 8193, 32)[1][1] == 2
    assert GC.plan(128, 32768, 32)[1][1:3] == [16, 8192] and GC.plan(512, 32768, 32)[1][1:3] == [32, 16384]
    for bad in [(0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, -1), (-4, 4, 1), (4, -4, 1), (3, 4, 4)]:
        assert GC.plan(*bad)[0] == EINVAL, bad
    assert GC.plan(1 << 20, 1 << 20, 32)[0] == EUNSUP and GC.plan(32, 1 << 31, 32)[0] == EUNSUP
    assert _lib.load().pdr_group_norm_act_plan(32, 8, 32, 1, None) == EINVAL


def test_workspace_serves_the_forward_partials_and_the_backward_rows():
    for B, C, S, G in [(1, 32, 1, 32), (2, 35, 7, 32), (3, 64, 100000, 32), (32, 128, 32768, 32), (2, 16, 20, 16)]:
        P = GC.plan(C, S, G)[1][1]
        assert GC.workspace_bytes(B, C, S, G) == 16 * max(B * G * P, B * C), (B, C, S, G)
    for empty in [(0, 32, 8, 32), (2, 0, 8, 32), (2, 32, 0, 32), (2, 32, 8, 0), (2, 8, 8, 32), (-1, 32, 8, 32)]:
        assert GC.workspace_bytes(*empty) == 0, empty


def test_calls_validate_their_arguments_in_the_documented_order_without_a_gpu():
    lib = _lib.load()
    p = 0x1000                                         # never dereferenced: every call below returns before a launch

    def fwd(B, C, S, G, act=1, eps=1e-5, x=p, gamma=p, beta=p, y=p, mean=p, rstd=p, ws=p):
        return lib.pdr_group_norm_act(x, gamma, beta, B, C, S, G, eps, act, y, mean, rstd, ws, None)

    def bwd(B, C, S, G, act=1, x=p, gamma=p, beta=p, mean=p, rstd=p, gy=p, gx=p, gw=p, gb=p, ws=p):
        return lib.pdr_group_norm_act_grad(x, gamma, beta, mean, rstd, gy, B, C, S, G, act, gx, gw, gb, ws, None)

    for call in (fwd, bwd):
        # 1. a negative size, G <= 0 or an activation outside 0..2: before anything else
        assert call(-1, 32, 8, 32) == EINVAL and call(1, -32, 8, 32) == EINVAL and call(1, 32, -8, 32) == EINVAL
        assert call(1, 32, 8, 0) == EINVAL and call(1, 32, 8, -4) == EINVAL
        assert call(1, 32, 8, 32, act=3) == EINVAL and call(1, 32, 8, 32, act=-1) == EINVAL
        assert call(0, 32, 8, 32, act=3) == EINVAL and call(-1, 32, 8, 32, x=None) == EINVAL
        assert call(-1, 1 << 20, 1 << 20, 32) == EINVAL
        # 2. fewer channels than groups (nothing would be normalised), before the empty problem
        assert call(1, 31, 8, 32) == EINVAL and call(0, 31, 8, 32) == EINVAL and call(1, 3, 1 << 40, 4) == EINVAL
        # 3. an empty problem: OK, no pointer looked at
        for shape in ((0, 32, 8, 32), (1, 0, 8, 32), (1, 32, 0, 32), (0, 0, 0, 1)):
            assert call(*shape, x=None, ws=None, mean=None, rstd=None, gamma=None) == OK, shape
        # 4. 2^31 elements or more, before the pointers
        assert call(1 << 10, 1 << 11, 1 << 10, 32) == EUNSUP and call(1 << 10, 1 << 11, 1 << 10, 32, x=None) == EUNSUP
        assert call(1, 32, 1 << 31, 32) == EUNSUP and call((1 << 31) - 1, (1 << 31) - 1, (1 << 40), 32) == EUNSUP
        # 5. the pointers
        assert call(1, 32, 8, 32, x=None) == EINVAL and call(1, 32, 8, 32, ws=None) == EINVAL
        assert call(1, 32, 8, 32, gamma=None) == EINVAL and call(1, 32, 8, 32, beta=None) == EINVAL
    assert fwd(1, 32, 8, 32, eps=-1.0) == EINVAL and fwd(1, 32, 8, 32, eps=float("nan")) == EINVAL
    assert fwd(0, 32, 8, 32, eps=-1.0) == EINVAL and fwd(1, 32, 8, 32, y=None) == EINVAL
    assert fwd(0, 32, 8, 32, y=None) == OK
    assert bwd(1, 32, 8, 32, mean=None) == EINVAL and bwd(1, 32, 8, 32, rstd=None) == EINVAL
    assert bwd(1, 32, 8, 32, gy=None) == EINVAL and bwd(1, 32, 8, 32, gx=None, gw=None, gb=None) == EINVAL
    assert bwd(1, 32, 8, 32, gamma=None, beta=None) == EINVAL           # gradients of parameters that are not there
    assert bwd(1, 32, 8, 32, gamma=None, beta=None, gw=None) == EINVAL
    assert bwd(1, 1 << 11, 1 << 20, 32, gx=None, gw=None, gb=None) == EUNSUP
    assert bwd(1, 0, 8, 32, gy=None, gx=None, gw=None, gb=None) == OK
    assert lib.pdr_version() == 200


def test_cpu_tensors_are_refused():
    x, w, b = torch.randn(2, 35, 5, 3), torch.ones(32), torch.zeros(32)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.group_norm_act(x, w, b, 32, 1e-5, "relu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.group_norm_act_grad(x, w, b, torch.zeros(2, 32), torch.ones(2, 32), torch.randn(2, 35, 5, 3), 32, "relu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.group_norm_act(x, w, b, 32, act="swish")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.group_norm_act(x, None, None, 32)


def test_switch_defaults_to_off_and_round_trips():
    assert _ext.is_fused_group_norm() is False and pointnet2_ops.is_fused_group_norm() is False
    try:
        assert _ext.set_fused_group_norm(True) is False and _ext.is_fused_group_norm() is True
        assert pointnet2_ops.set_fused_group_norm(True) is True
        assert _ext.set_fused_group_norm(False) is True and _ext.is_fused_group_norm() is False
        for bad in (None, 1, "on"):
            with pytest.raises(TypeError):
                _ext.set_fused_group_norm(bad)
        assert _ext.is_fused_group_norm() is False
    finally:
        _ext.set_fused_group_norm(False)
    assert _ext.is_fused_attention_pool() is False                      # the other switch is its own
    assert _ext.group_norm_act_supported((32, 35, 1024, 32), 32) and _ext.group_norm_act_supported((2, 32), 32)
    assert not _ext.group_norm_act_supported((2, 31, 8), 32) and not _ext.group_norm_act_supported((1 << 11, 1 << 10, 1 << 10), 32)


# ---- the module path with the switch off (and, on CPU tensors, with it on) ----------------------------------------
def explicit_sequential(seq, x):
    """What the stack computed before NormActSequential: its children in order, MyGroupNorm and the activations
    written out."""
    for m in seq:
        if isinstance(m, MyGroupNorm):
            c, gn = m.num_channels, m.group_norm
            h = F.group_norm(x[:, :c], m.num_groups, gn.weight, gn.bias, gn.eps)
            x = h if x.shape[1] == c else torch.cat([h, x[:, c:]], dim=1)
        elif isinstance(m, torch.nn.ReLU):
            x = F.relu(x)
        elif isinstance(m, Swish):
            x = x * torch.sigmoid(x)
        else:
            assert isinstance(m, torch.nn.Conv2d)
            x = F.conv2d(x, m.weight, m.bias)
    return x


def both_switch_settings(fn):
    prev = _ext.set_fused_group_norm(False)
    try:
        off = fn()
        _ext.set_fused_group_norm(True)
        on = fn()
    finally:
        _ext.set_fused_group_norm(prev)
    return off, on


as_bits = lambda t: t.contiguous().view(torch.int32)


@pytest.mark.parametrize("bn_first", [False, True])
@pytest.mark.parametrize("activation", ["relu", "swish"])
def test_build_shared_mlp_gives_the_composition_s_bits_and_keys(bn_first, activation):
    torch.manual_seed(3)
    mlp = build_shared_mlp([35, 32, 64], bn=True, bn_first=bn_first, bias=bn_first, activation=activation)
    if bn_first:
        keys = ["0.group_norm.weight", "0.group_norm.bias", "2.weight", "2.bias", "3.group_norm.weight",
                "3.group_norm.bias", "5.weight", "5.bias"]
    else:
        keys = ["0.weight", "1.group_norm.weight", "1.group_norm.bias", "3.weight", "4.group_norm.weight",
                "4.group_norm.bias"]
    assert list(mlp.state_dict().keys()) == keys and isinstance(mlp, torch.nn.Sequential) and len(mlp) == 6
    x = torch.randn(2, 35, 5, 3)
    with torch.no_grad():
        want = explicit_sequential(mlp, x.clone())
        off, on = both_switch_settings(lambda: mlp(x.clone()))
    assert torch.equal(as_bits(off), as_bits(want)) and torch.equal(as_bits(on), as_bits(want))


def test_mlp_plus_t_emb_gives_the_composition_s_bits_and_keys():
    torch.manual_seed(4)
    mod = Mlp_plus_t_emb([35, 32, 32, 64], bn=True, res_connect=True, include_t=True, t_dim=16)
    assert list(mod.state_dict().keys()) == [
        "fc.weight", "fc.bias", "res_connect.weight", "first_mlp.0.weight", "first_mlp.1.group_norm.weight",
        "first_mlp.1.group_norm.bias", "second_mlp.0.weight", "second_mlp.1.group_norm.weight",
        "second_mlp.1.group_norm.bias", "rest_mlp.0.weight", "rest_mlp.1.group_norm.weight",
        "rest_mlp.1.group_norm.bias"]
    x, t = torch.randn(2, 35, 5, 3), torch.randn(2, 16)
    with torch.no_grad():
        h = explicit_sequential(mod.first_mlp, x.clone()) + mod.fc(t).unsqueeze(2).unsqueeze(3)
        h = explicit_sequential(mod.rest_mlp, explicit_sequential(mod.second_mlp, h))
        want = h + mod.res_connect(x)
        off, on = both_switch_settings(lambda: mod(x.clone(), t_emb=t))
    assert torch.equal(as_bits(off), as_bits(want)) and torch.equal(as_bits(on), as_bits(want))


def test_attention_module_gives_the_composition_s_bits_and_keys():
    torch.manual_seed(5)
    B, N, K = 2, 5, 3
    mod = AttentionModule(8, 35, 8, 35, 64)
    assert list(mod.state_dict().keys()) == [
        "feat_conv.weight", "feat_conv.bias", "grouped_feat_conv.weight", "grouped_feat_conv.bias",
        "weight_conv.1.group_norm.weight", "weight_conv.1.group_norm.bias", "weight_conv.2.weight", "weight_conv.2.bias",
        "weight_conv.4.group_norm.weight", "weight_conv.4.group_norm.bias", "weight_conv.5.weight", "weight_conv.5.bias",
        "feat_out_conv.0.weight", "feat_out_conv.0.bias", "feat_out_conv.1.group_norm.weight",
        "feat_out_conv.1.group_norm.bias"]
    feat, gf, gfo = torch.randn(B, 8, N), torch.randn(B, 35, N, K), torch.randn(B, 64, N, K)
    with torch.no_grad():
        q = mod.feat_conv(feat.unsqueeze(-1)).expand(-1, -1, -1, K)
        scores = explicit_sequential(mod.weight_conv, torch.cat([q, mod.grouped_feat_conv(gf)], dim=1))
        want = (explicit_sequential(mod.feat_out_conv, gfo.clone()) * F.softmax(scores, dim=-1)).sum(dim=-1)
        off, on = both_switch_settings(lambda: mod(feat, gf, gfo.clone(), 'all'))
    assert torch.equal(as_bits(off), as_bits(want)) and torch.equal(as_bits(on), as_bits(want))


# ---- the bounds discriminate ----------------------------------------------------------------------------------------
VARIANTS = ("unbiased_variance", "eps_left_out", "relu_mask_from_xh", "dgamma_misses_last_cloud", "fp32_single_pass")


def candidate(shape, x, gamma, beta, gy, act, variant):
    """The op by its defining formulas in float64 numpy, rounded to fp32 at the end, with one deliberate mistake."""
    B, C, S, G = shape
    Cg = (C - C % G) // G
    Cn, m = G * Cg, Cg * S
    xd, dy = x.astype(np.float64), gy.astype(np.float64)
    xs = xd[:, :Cn].reshape(B, G, m)
    with np.errstate(all="ignore"):
        if variant == "fp32_single_pass":
            x32 = xs.astype(np.float32)
            mean = x32.mean(-1, dtype=np.float32)
            var = ((x32 * x32).mean(-1, dtype=np.float32) - mean * mean).astype(np.float64)
            mean, var = mean.astype(np.float64), np.maximum(var, 0.0)
        else:
            mean = xs.mean(-1)
            var = ((xs - mean[..., None]) ** 2).sum(-1) / (m - 1 if variant == "unbiased_variance" else m)
        rstd = 1.0 / np.sqrt(var + (0.0 if variant == "eps_left_out" else GC.EPS))
        row = lambda a: np.repeat(a, Cg, axis=1)[:, :, None]
        g = np.ones(Cn) if gamma is None else gamma.astype(np.float64)
        b = np.zeros(Cn) if beta is None else beta.astype(np.float64)
        xh = (xd[:, :Cn] - row(mean)) * row(rstd)
        z = np.concatenate([xh * g[None, :, None] + b[None, :, None], xd[:, Cn:]], axis=1)
        s = 1.0 / (1.0 + np.exp(-z))
        if act == "relu":
            mask = z > 0
            if variant == "relu_mask_from_xh":
                mask = np.concatenate([xh > 0, xd[:, Cn:] > 0], axis=1)
            y, dz = np.where(z > 0, z, 0.0), dy * mask
        elif act == "swish":
            y, dz = z * s, dy * s * (1 + z * (1 - s))
        else:
            y, dz = z, dy
        r1, r2 = (dz[:, :Cn] * xh).sum(-1), dz[:, :Cn].sum(-1)
        c1 = row((g[None, :] * r1).reshape(B, G, Cg).sum(-1))
        c2 = row((g[None, :] * r2).reshape(B, G, Cg).sum(-1))
        gx = np.concatenate([row(rstd) * (g[None, :, None] * dz[:, :Cn] - (c2 + xh * c1) / m), dz[:, Cn:]], axis=1)
        gw = (r1[:-1] if variant == "dgamma_misses_last_cloud" else r1).sum(0)
        out = dict(y=y, mean=mean, rstd=rstd, gx=gx, gw=None if gamma is None else gw,
                   gb=None if gamma is None else r2.sum(0))
        return {k: None if a is None else a.astype(np.float32) for k, a in out.items()}


def test_the_bounds_pass_the_rounded_reference_and_fail_five_wrong_implementations():
    """The fp32-rounded float64 reference and the mistake-free candidate stay within every bound on every case; each
    mistake leaves them on at least one -- the fp32 single-pass moments on an "offset" case."""
    failed_by = {v: [] for v in VARIANTS}
    for shape in GC.FIXED_SHAPES:
        for pattern in GC.PATTERNS:
            for affine in (False, True):
                x, gamma, beta, gy = GC.make(shape, pattern, affine)
                for act in GC.ACTS:
                    ref = GC.reference(shape, x, gamma, beta, gy, act)
                    rounded = {k: None if ref[k] is None else ref[k].astype(np.float32) for k in GC.OUTPUTS}
                    case = (shape, pattern, affine, act)
                    assert max(GC.worst_ratio(rounded, ref).values()) <= 1.0, case
                    honest = GC.worst_ratio(candidate(shape, x, gamma, beta, gy, act, None), ref)
                    assert max(honest.values()) <= 1.0, (case, honest)
                    for v in VARIANTS:
                        worst = GC.worst_ratio(candidate(shape, x, gamma, beta, gy, act, v), ref)
                        if max(worst.values()) > 1.0:
                            failed_by[v].append(case)
    for v in VARIANTS:
        print(v, "leaves the bounds on", len(failed_by[v]), "cases")
        assert failed_by[v], v
    assert any(c[1] == "offset" for c in failed_by["fp32_single_pass"])
    assert all(c[3] == "relu" for c in failed_by["relu_mask_from_xh"])
    assert all(c[2] for c in failed_by["dgamma_misses_last_cloud"])
