"""pdr_relu_group_norm_conv_cf and its two gradient calls without a GPU: the host-only plan and workspace size, the
documented order of the argument checks (nothing is launched, no pointer is looked at before its turn), the
`relu_group_norm_conv_supported` predicate against the plan's PDR_EUNSUPPORTED, the switch, the module path on CPU
tensors with the switch on, and the emulation of tests/relu_group_norm_conv_cases.py inside the derived bounds against
the float64 composition on every case, pattern and affine setting -- the bounds and the emulation are checked here
before any GPU sees them."""
import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule
from tests import relu_group_norm_cases as RC
from tests import relu_group_norm_conv_cases as CC

OK, EINVAL, EUNSUP = _lib.PDR_OK, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED


def test_plan_reports_the_statistics_plan_the_tile_and_the_chain_length():
    for case in CC.cases():
        B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = CC.dims(case)
        for al in (1, 0):
            rc, p = CC.plan(C1, C2, N, K, G, Cout, al)
            rc0, p0 = RC.plan(C1, C2, N, K, G, al)
            assert rc == OK and rc0 == OK and [p["family"], p["P"], p["E"], p["Cg"]] == p0, case
            assert p["family"] == int(bool(al) and K % 4 == 0)
            assert p["tile"] > 0 and p["tile"] % 32 == 0 and p["rows"] in (32, 64, 128) and p["rows"] >= min(Cout, 128)
            # the chain length from S alone: a multiple of 32, R = ceil(S / L) ranges, at most 16
            assert p["L"] % 32 == 0 and p["R"] == -(-S // p["L"]) and 1 <= p["R"] <= 16
            if 2 * C <= 1024:
                assert CC.plan(C1, C2 + C, N, K, 2 * G, Cout + 7, al)[1]["L"] == p["L"]
    for S_big in (1 << 16, (1 << 20) + 4):
        p = CC.plan(0, 32, S_big // 4, 4, 32, 32)[1]
        assert p["R"] <= 16 and (p["R"] - 1) * p["L"] < S_big <= p["R"] * p["L"] and p["L"] % 32 == 0
    case = CC.plan_case()
    p = CC.plan(*case[1:])[1]
    assert p["R"] >= 2 and -(-case[3] * case[4] // p["tile"]) >= 3
    for bad in [(-1, 4, 4, 4, 1, 8), (0, 0, 4, 4, 1, 8), (4, 4, 0, 4, 1, 8), (4, 4, 4, 0, 1, 8), (4, 4, 4, 4, 0, 8),
                (4, 4, 4, 4, 1, 0), (4, 4, 4, 4, 1, -3), (1, 2, 4, 4, 4, 8)]:
        assert CC.plan(*bad)[0] == EINVAL, bad
    assert CC.plan(0, 1025, 4, 4, 32, 8)[0] == EUNSUP and CC.plan(0, 32, 4, 4, 32, 1025)[0] == EUNSUP
    assert CC.plan(0, 1024, 4, 4, 32, 1024)[0] == OK and CC.plan(256, 651, 512, 32, 32, 512)[0] == OK
    assert CC.plan(0, 32, 1 << 16, 1 << 15, 32, 8)[0] == EUNSUP and CC.plan(0, 32, 1 << 12, 1 << 10, 32, 1024)[0] == EUNSUP
    assert _lib.load().pdr_relu_group_norm_conv_cf_plan(0, 32, 8, 4, 32, 8, 1, None) == EINVAL


def test_workspace_serves_the_forward_partials_and_the_weight_gradient_partials():
    for case in CC.cases() + [(3, 32, 137, 2048, 32, 32, 169), (32, 256, 651, 512, 32, 32, 512)]:
        B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = CC.dims(case)
        p = CC.plan(C1, C2, N, K, G, Cout)[1]
        fwd = 16 * B * G * (p["P"] + 1)
        bwd = -(-4 * B * p["R"] * Cout * C // 8) * 8 + 8 * B * p["R"] * Cout
        assert CC.workspace_bytes(*case) == max(fwd, bwd), case
    for empty in [(0, 0, 32, 8, 4, 32, 8), (2, 0, 0, 8, 4, 32, 8), (2, 0, 32, 0, 4, 32, 8), (2, 0, 32, 8, 0, 32, 8),
                  (2, 0, 32, 8, 4, 0, 8), (2, 4, 4, 8, 4, 32, 8), (2, 0, 32, 8, 4, 32, 0), (2, 0, 1025, 8, 4, 32, 8),
                  (4096, 0, 32, 8, 4, 32, 8)]:
        assert CC.workspace_bytes(*empty) == 0, empty


def test_calls_validate_their_arguments_in_the_documented_order_without_a_gpu():
    lib = _lib.load()
    p = 0x1000                                         # never dereferenced: every call below returns before a launch

    def fwd(B, C1, C2, N, K, G, Cout=8, eps=1e-5, q=p, k=p, gamma=p, beta=p, W=p, cb=p, out=p, mean=p, rstd=p, ws=p):
        return lib.pdr_relu_group_norm_conv_cf(q, k, gamma, beta, W, cb, B, C1, C2, N, K, G, Cout, eps, out, mean, rstd,
                                               ws, None)

    def gwt(B, C1, C2, N, K, G, Cout=8, q=p, k=p, gamma=p, beta=p, mean=p, rstd=p, go=p, gW=p, gb=p, ws=p, **_):
        return lib.pdr_relu_group_norm_conv_cf_grad_weight(q, k, gamma, beta, mean, rstd, go, B, C1, C2, N, K, G, Cout,
                                                           gW, gb, ws, None)

    for call in (fwd, gwt):
        # 1. a negative size, C2 < 1, G < 1 or Cout < 1: before anything else
        for bad in [(-1, 8, 24, 8, 4, 32), (1, -8, 40, 8, 4, 32), (1, 8, 24, -8, 4, 32), (1, 8, 24, 8, -4, 32),
                    (1, 32, 0, 8, 4, 32), (1, 8, 24, 8, 4, 0), (1, 8, 24, 8, 4, 32, 0), (1, 8, 24, 8, 4, 32, -2),
                    (0, 8, 24, 8, 4, 32, 0)]:
            assert call(*bad) == EINVAL, bad
        assert call(1 << 10, 0, 1 << 11, 1 << 5, 1 << 5, 32, 0) == EINVAL          # Cout before the limits
        # 2. fewer channels than groups, before the empty problem
        assert call(1, 8, 23, 8, 4, 32) == EINVAL and call(0, 8, 23, 8, 4, 32) == EINVAL
        # 3. an empty problem: OK, no pointer looked at, whatever the widths
        for shape in ((0, 8, 24, 8, 4, 32), (1, 8, 24, 0, 4, 32), (1, 8, 24, 8, 0, 32), (0, 0, 2000, 0, 0, 1, 5000)):
            assert call(*shape, q=None, k=None, ws=None, mean=None, rstd=None, gamma=None, W=None, out=None) == OK, shape
        # 4. the limits, before the pointers
        assert call(1 << 10, 0, 1 << 11, 1 << 5, 1 << 5, 32, k=None) == EUNSUP
        assert call(1, 0, 1025, 8, 4, 32, k=None) == EUNSUP and call(1, 0, 32, 8, 4, 32, 1025, k=None) == EUNSUP
        assert call(4096, 0, 32, 1, 1, 32, k=None) == EUNSUP
        assert call(1, 0, 32, 1 << 12, 1 << 10, 32, 1024, k=None) == EUNSUP         # B Cout N K = 2^32
        assert call(4095, 0, 1024, 1, 1, 32, 1024, k=None) == EINVAL                # inside every limit: the pointers' turn
        # 5. the pointers
        assert call(1, 8, 24, 8, 4, 32, k=None) == EINVAL and call(1, 8, 24, 8, 4, 32, q=None) == EINVAL
        assert call(1, 8, 24, 8, 4, 32, ws=None) == EINVAL and call(1, 8, 24, 8, 4, 32, mean=None) == EINVAL
        assert call(1, 8, 24, 8, 4, 32, rstd=None) == EINVAL
        assert call(1, 8, 24, 8, 4, 32, gamma=None) == EINVAL and call(1, 8, 24, 8, 4, 32, beta=None) == EINVAL
    assert fwd(1, 8, 24, 8, 4, 32, eps=-1.0) == EINVAL and fwd(1, 8, 24, 8, 4, 32, eps=float("nan")) == EINVAL
    assert fwd(1, 8, 24, 8, 4, 32, W=None) == EINVAL and fwd(1, 8, 24, 8, 4, 32, out=None) == EINVAL
    assert gwt(1, 8, 24, 8, 4, 32, go=None) == EINVAL and gwt(1, 8, 24, 8, 4, 32, gW=None, gb=None) == EINVAL

    def gin(B, C, N, K, Cout, W=p, go=p, gx=p):
        return lib.pdr_relu_group_norm_conv_cf_grad_input(W, go, B, C, N, K, Cout, gx, None)

    for bad in [(-1, 8, 4, 4, 8), (1, 0, 4, 4, 8), (1, 8, -4, 4, 8), (1, 8, 4, -4, 8), (1, 8, 4, 4, 0), (0, 8, 4, 4, 0)]:
        assert gin(*bad) == EINVAL, bad
    assert gin(0, 8, 4, 4, 8, W=None, go=None, gx=None) == OK and gin(1, 8, 0, 4, 8, W=None) == OK
    assert gin(1, 1025, 4, 4, 8, W=None) == EUNSUP and gin(1, 8, 4, 4, 1025, W=None) == EUNSUP
    assert gin(4096, 8, 1, 1, 8, W=None) == EUNSUP and gin(1, 1024, 1 << 11, 1 << 10, 8, W=None) == EUNSUP
    assert gin(1, 8, 4, 4, 8, W=None) == EINVAL and gin(1, 8, 4, 4, 8, go=None) == EINVAL
    assert gin(1, 8, 4, 4, 8, gx=None) == EINVAL
    assert lib.pdr_version() == 200


def test_supported_predicate_agrees_with_the_plan():
    shapes = [(c[1], (c[0], c[2], c[3], c[4]), c[5], c[6]) for c in CC.cases()]
    shapes += [(128, (32, 41, 2048, 32), 32, 169), (256, (32, 651, 512, 32), 32, 512), (0, (1, 1025, 4, 4), 32, 8),
               (0, (1, 32, 4, 4), 32, 1025), (0, (1, 1024, 4, 4), 32, 1024), (8, (2, 23, 8, 4), 32, 8),
               (0, (1, 32, 1 << 12, 1 << 10), 32, 1024), (0, (1, 32, 1 << 16, 1 << 15), 32, 8), (0, (2, 32, 8, 4), 32, 0),
               (4, (1, 64, 8, 4), 32, 1)]
    for C1, ks, G, Cout in shapes:
        rc = CC.plan(C1, ks[1], ks[2], ks[3], G, Cout)[0]
        one = (1,) + tuple(ks[1:])
        assert _ext.relu_group_norm_conv_supported(C1, one, G, Cout) == (rc == OK), (C1, ks, G, Cout)
        if rc == OK and ks[0] * max(C1 + ks[1], Cout) * ks[2] * ks[3] < 2 ** 31:
            assert _ext.relu_group_norm_conv_supported(C1, ks, G, Cout)
            assert CC.workspace_bytes(ks[0], C1, ks[1], ks[2], ks[3], G, Cout) > 0
    assert not _ext.relu_group_norm_conv_supported(0, (4096, 32, 1, 1), 32, 8)
    assert CC.workspace_bytes(4096, 0, 32, 1, 1, 32, 8) == 0 and CC.workspace_bytes(4095, 0, 32, 1, 1, 32, 8) > 0
    assert not _ext.relu_group_norm_conv_supported(0, (2, 32, 8), 32, 8)


def test_cpu_tensors_are_refused():
    q, k, w, b = torch.randn(2, 8, 5), torch.randn(2, 27, 5, 3), torch.ones(32), torch.zeros(32)
    W, cb = torch.randn(16, 35), torch.zeros(16)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.relu_group_norm_conv(q, k, w, b, 32, 1e-5, W, cb)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.relu_group_norm_conv_grad_input(W, torch.randn(2, 16, 5, 3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.relu_group_norm_conv_grad_weight(q, k, w, b, torch.zeros(2, 32), torch.ones(2, 32), torch.randn(2, 16, 5, 3),
                                              32)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.relu_group_norm_conv(k, w, b, 32, 1e-5, W, cb, q=q)


def test_switch_defaults_to_off_round_trips_and_is_independent_of_the_other_six():
    others = (_ext.is_fused_attention_pool, _ext.is_fused_group_norm, _ext.is_fused_grouping, _ext.is_fused_knn_grouping,
              _ext.is_fused_score_norm, _ext.is_fused_injection)
    assert _ext.is_fused_score_conv() is False and pointnet2_ops.is_fused_score_conv() is False
    try:
        assert _ext.set_fused_score_conv(True) is False and _ext.is_fused_score_conv() is True
        assert [f() for f in others] == [False] * 6
        assert pointnet2_ops.set_fused_score_conv(True) is True
        assert _ext.set_fused_score_conv(False) is True and _ext.is_fused_score_conv() is False
        for bad in (None, 1, "on"):
            with pytest.raises(TypeError):
                _ext.set_fused_score_conv(bad)
        assert _ext.is_fused_score_conv() is False
        for setter in (_ext.set_fused_attention_pool, _ext.set_fused_group_norm, _ext.set_fused_grouping,
                       _ext.set_fused_knn_grouping, _ext.set_fused_score_norm, _ext.set_fused_injection):
            try:
                assert setter(True) is False and _ext.is_fused_score_conv() is False
            finally:
                setter(False)
    finally:
        _ext.set_fused_score_conv(False)


def graph_names(t):
    seen, names, todo = set(), [], [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return sorted(names)


@pytest.mark.parametrize("count", ["all", "tensor"])
def test_attention_module_on_cpu_tensors_takes_the_composition_with_the_switch_on(count):
    torch.manual_seed(5)
    B, N, K = 2, 5, 3
    mod = AttentionModule(8, 35, 8, 35, 64)
    keys = sorted(mod.state_dict())
    feat, gf, gfo = torch.randn(B, 8, N), torch.randn(B, 35, N, K), torch.randn(B, 64, N, K)
    cnt = 'all' if count == "all" else torch.randint(0, K + 1, (B, N), dtype=torch.int32)
    as_bits = lambda t: t.detach().contiguous().view(torch.int32)
    off = mod(feat, gf, gfo.clone(), cnt)
    scores_off = mod.score_head(feat, gf)
    prev = _ext.set_fused_score_conv(True)
    try:
        on = mod(feat, gf, gfo.clone(), cnt)
        scores_on = mod.score_head(feat, gf)
    finally:
        _ext.set_fused_score_conv(prev)
    assert torch.equal(as_bits(off), as_bits(on)) and torch.equal(as_bits(scores_off), as_bits(scores_on))
    assert graph_names(scores_on) == graph_names(scores_off) and graph_names(on) == graph_names(off)
    assert not any("ReluGroupNorm" in n for n in graph_names(on))
    assert sorted(mod.state_dict()) == keys and len(keys) == 16
    assert keys == sorted(
        ["feat_conv.weight", "feat_conv.bias", "grouped_feat_conv.weight", "grouped_feat_conv.bias"]
        + ["weight_conv.%d.%s" % (i, n) for i in (2, 5) for n in ("weight", "bias")]
        + ["weight_conv.%d.group_norm.%s" % (i, n) for i in (1, 4) for n in ("weight", "bias")]
        + ["feat_out_conv.0.weight", "feat_out_conv.0.bias", "feat_out_conv.1.group_norm.weight",
           "feat_out_conv.1.group_norm.bias"])


# ---- the emulation inside the bounds, against the float64 composition ------------------------------------------------------
@pytest.mark.parametrize("case", CC.cases(), ids=lambda c: "x".join(map(str, c)))
def test_emulation_meets_the_bounds_on_every_pattern(case):
    B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = CC.dims(case)
    L = CC.plan(C1, C2, N, K, G, Cout)[1]["L"]
    worst = dict(out=0.0, gW=0.0, gb=0.0)
    for pattern in CC.PATTERNS:
        for affine in (True, False):
            q, k, gamma, beta, W, cbias, go, gy = CC.make(case, pattern, affine)
            ref = RC.reference(case[:6], q, k, gamma, beta, gy)
            # the fp32 statistics a kernel would hand over: the float64 ones, rounded (inside RC's bounds by definition)
            mean, rstd = ref["mean"].astype(np.float32), ref["rstd"].astype(np.float32)
            xn = CC.xn_bits(case, q, k, gamma, beta, mean, rstd)
            assert RC.worst_ratio(dict(y=xn), ref)["y"] <= 1.0
            acc = CC.chain(W, xn)
            for cb in (cbias, None):
                out = acc if cb is None else (acc + cb[None, :, None, None]).astype(np.float32)
                r64 = CC.composition64(q, k, gamma, beta, W, cb, G)
                worst["out"] = max(worst["out"], CC.ratio(np.abs(out - r64["out"]), CC.out_bound(case, ref, W, r64["out"])))
            # the float64 sums of the SAME xn: an fp32 chain over ranges of L, folded in double, must sit inside the bound
            gw64, gwabs, gb64, gbabs = CC.grad_weight_reference(go, xn)
            gflat, xflat = go.reshape(B, Cout, S), xn.reshape(B, C, S)
            acc = np.zeros((Cout, C))
            for b in range(B):
                for lo in range(0, S, L):
                    acc += np.einsum("os,cs->oc", gflat[b, :, lo:lo + L], xflat[b, :, lo:lo + L], dtype=np.float32)
            worst["gW"] = max(worst["gW"], CC.ratio(np.abs(acc.astype(np.float32) - gw64), (L + 4) * CC.U * gwabs + CC.SUB))
            gbe = gflat.astype(np.float64).sum((0, 2)).astype(np.float32)
            worst["gb"] = max(worst["gb"], CC.ratio(np.abs(gbe - gb64), (CC.U + CC.V * (B * S + 2)) * gbabs + CC.SUB))
            # the input-gradient chain against its float64 product: C -> Cout in the bound's chain term
            gxn = CC.emulate_grad_input(W, go)
            g64 = np.einsum("oc,bonk->bcnk", W.astype(np.float64), go.astype(np.float64))
            gab = np.einsum("oc,bonk->bcnk", np.abs(W.astype(np.float64)), np.abs(go.astype(np.float64)))
            assert CC.ratio(np.abs(gxn - g64), (Cout + 2) * CC.U * gab + CC.SUB) <= 1.0
    print("worst ratios to the bounds", case, worst)
    assert worst["out"] <= 1.0 and worst["gW"] <= 1.0 and worst["gb"] <= 1.0, worst


def test_xn_bits_is_the_y_of_the_sibling_emulation_and_the_exact_fma_agrees_with_fma32():
    case = CC.FIXED_CASES[0]
    q, k, gamma, beta, W, cbias, go, gy = CC.make(case, "normal", True)
    emu = RC.emulate(case[:6], q, k, gamma, beta, gy, 1)
    xn = CC.xn_bits(case, q, k, gamma, beta, emu["mean"], emu["rstd"])
    assert np.array_equal(RC.bits(xn), RC.bits(emu["y"]))
    out = CC.emulate_forward(W, None, xn)
    X = xn.reshape(xn.shape[0], xn.shape[1], -1)
    for b, o, s in [(0, 0, 0), (1, 39, 27), (0, 17, 5)]:
        exact = CC.chain_exact(W[o], X[b, :, s])
        assert exact.view(np.uint32) == out.reshape(out.shape[0], out.shape[1], -1)[b, o, s].view(np.uint32)
    assert CC.same_bits_or_exact(out, out, W, xn) == 0
