"""pdr_group_norm_act / pdr_group_norm_act_grad on the GPU, through _ext.group_norm_act / group_norm_act_grad (thin
wrappers of the two C calls), pointnet2_utils.group_norm_act and the module path under set_fused_group_norm.

Reference and bounds: tests/group_norm_act_cases.py (the float64 composition on the CPU and bounds derived from the
kernels' stated operation chain; its module docstring justifies every term).  Every element of y, mean, rstd, grad_x,
grad_gamma and grad_beta is asserted within its own bound; nothing is excluded.

Module level there is no closed bound through convolutions and several norms, so the test measures the switch-off
path's error against the same module in float64 on the CPU and requires the switch-on error to be at most 4 x that,
with a floor of 8 u: two fp32 pipelines whose reductions run in different orders."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule, MyGroupNorm
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import Mlp_plus_t_emb, Swish, build_shared_mlp
from tests import group_norm_act_cases as GC

pytestmark = pytest.mark.gpu

bits = GC.bits
_IN, _REF = {}, {}


def inputs(shape, pattern, affine):
    key = (shape, pattern, affine)
    if key not in _IN:
        arrays = GC.make(shape, pattern, affine)
        for a in arrays:
            if a is not None:
                a.setflags(write=False)
        _IN[key] = arrays
    return _IN[key]


def reference(shape, pattern, affine, act):
    """Host inputs and the float64 reference of a case, computed once and left unchanged."""
    key = (shape, pattern, affine, act)
    if key not in _REF:
        _REF[key] = GC.reference(shape, *inputs(shape, pattern, affine), act)
    return inputs(shape, pattern, affine), _REF[key]


def dev(a, cuda, offset=False):
    """Device copy of a host array; offset=True: a contiguous view 4 bytes into its storage."""
    if a is None:
        return None
    t = torch.tensor(np.asarray(a))                    # a copy: the cached host arrays are read-only
    if not offset:
        return t.to(cuda)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def run(arrays, G, act, cuda, offset=False, need=(True, True, True)):
    """The six outputs of the two C calls as a dict of device tensors (a gradient not asked for: None)."""
    x, gamma, beta, gy = arrays
    xd, gd, bd, gyd = dev(x, cuda, offset), dev(gamma, cuda), dev(beta, cuda), dev(gy, cuda, offset)
    y, mean, rstd = _ext.group_norm_act(xd, gd, bd, G, GC.EPS, act)
    gx, gw, gb = _ext.group_norm_act_grad(xd, gd, bd, mean, rstd, gyd, G, act, *need)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, gx=gx, gw=gw, gb=gb)


def host(got):
    return {k: None if t is None else t.cpu().numpy() for k, t in got.items()}


def check(got, ref, label):
    worst = GC.worst_ratio(host(got), ref)
    print(label, " ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)


CASES = [(sh, p, a, act) for sh in GC.shapes() for p in GC.PATTERNS for a in (False, True) for act in GC.ACTS]
_id = lambda c: "%s-%s-%s-%s" % ("x".join(map(str, c[0])), c[1], "affine" if c[2] else "plain", c[3])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_six_outputs_within_the_derived_bounds(cuda, case):
    shape, pattern, affine, act = case
    B, C, S, G = shape
    arrays, ref = reference(*case)
    assert GC.plan(C, S, G, 1)[1][0] == int(S % 4 == 0)
    got = run(arrays, G, act, cuda)
    check(got, ref, _id(case))
    # pass-through channels: z = x and dx = dz.  Where the activation is exact (none, relu) y and grad_x are compared
    # by bits with act(x) and dy act'(x); Swish goes through v_exp_f32, which no host computes bit for bit: its
    # pass-through channels stand under the bounds above with b_z = 0.
    Cn = C - C % G
    if Cn < C and act != "swish":
        x, gy = arrays[0][:, Cn:], arrays[3][:, Cn:]
        keep = x > 0 if act == "relu" else np.ones_like(x, bool)
        zero = np.zeros_like(x)
        assert np.array_equal(bits(got["y"])[:, Cn:], bits(np.where(keep, x, zero)))
        assert np.array_equal(bits(got["gx"])[:, Cn:], bits(np.where(keep, gy, zero)))


SOME = [((2, 67, 33, 32), "normal", True, "relu"), ((2, 35, 7, 32), "offset", True, "swish"),
        ((2, 16, 20, 16), "normal", False, "none"), ((1, 131, 260, 32), "normal", True, "swish")]


@pytest.mark.parametrize("case", SOME + [(GC.shapes()[-1], "normal", True, "relu")], ids=_id)
def test_same_bits_run_after_run_and_with_a_subset_of_the_gradients(cuda, case):
    shape, pattern, affine, act = case
    arrays = inputs(shape, pattern, affine)
    first, second = run(arrays, shape[3], act, cuda), run(arrays, shape[3], act, cuda)
    for k in GC.OUTPUTS:
        assert (first[k] is None) == (second[k] is None)
        assert first[k] is None or np.array_equal(bits(first[k]), bits(second[k])), k
    only_x = run(arrays, shape[3], act, cuda, need=(True, False, False))
    assert only_x["gw"] is None and only_x["gb"] is None and np.array_equal(bits(only_x["gx"]), bits(first["gx"]))
    if affine:
        only_w = run(arrays, shape[3], act, cuda, need=(False, True, False))
        assert only_w["gx"] is None and only_w["gb"] is None and np.array_equal(bits(only_w["gw"]), bits(first["gw"]))


@pytest.mark.parametrize("case", SOME[:3], ids=_id)
def test_a_cloud_of_a_batch_has_the_bits_of_its_own_call(cuda, case):
    shape, pattern, affine, act = case
    assert shape[0] == 2
    x, gamma, beta, gy = inputs(shape, pattern, affine)
    batched = run((x, gamma, beta, gy), shape[3], act, cuda)
    for b in range(shape[0]):
        alone = run((x[b:b + 1], gamma, beta, gy[b:b + 1]), shape[3], act, cuda)
        for k in ("y", "mean", "rstd", "gx"):
            assert np.array_equal(bits(batched[k])[b:b + 1], bits(alone[k])), (k, b)


def test_current_stream_and_graph_capture_of_forward_and_backward(cuda):
    """Both calls launch on torch's current stream without a hidden synchronisation: captured on a side stream, the
    graph replays with changed inputs and gives the eager call's bits."""
    shape, act = (2, 67, 33, 32), "swish"
    first, second = inputs(shape, "normal", True), inputs(shape, "offset", True)
    xd, gd, bd, gyd = (dev(a, cuda) for a in first)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y, mean, rstd = _ext.group_norm_act(xd, gd, bd, 32, GC.EPS, act)      # warm the allocator outside the capture
        _ext.group_norm_act_grad(xd, gd, bd, mean, rstd, gyd, 32, act)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y, mean, rstd = _ext.group_norm_act(xd, gd, bd, 32, GC.EPS, act)
            gx, gw, gb = _ext.group_norm_act_grad(xd, gd, bd, mean, rstd, gyd, 32, act)
    torch.cuda.current_stream().wait_stream(side)
    for arrays in (first, second):
        for t, a in zip((xd, gd, bd, gyd), arrays):
            t.copy_(torch.tensor(np.asarray(a)))
        for t in (y, mean, rstd, gx, gw, gb):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(arrays, 32, act, cuda)
        for k, t in zip(GC.OUTPUTS, (y, mean, rstd, gx, gw, gb)):
            assert np.array_equal(bits(t), bits(eager[k])), k


@pytest.mark.parametrize("act", GC.ACTS)
def test_public_function_under_autograd(cuda, act):
    """pointnet2_utils.group_norm_act on a 4-d tensor: the C-level bits; a non-contiguous grad_out; needs_input_grad
    subsets; a view with a storage offset (the scalar family) under the same bounds."""
    shape = (2, 67, 33, 32)                                               # as (2, 67, 11, 3)
    (x, gamma, beta, gy), ref = reference(shape, "normal", True, act)
    want = run((x, gamma, beta, gy), 32, act, cuda)
    four = lambda t: t.view(2, 67, 11, 3)
    xd, gd, bd = four(dev(x, cuda)).requires_grad_(), dev(gamma, cuda).requires_grad_(), dev(beta, cuda).requires_grad_()
    y = pointnet2_utils.group_norm_act(xd, gd, bd, 32, GC.EPS, act)
    assert y.shape == xd.shape and all(t.data_ptr() != y.data_ptr() for t in y.grad_fn.saved_tensors)     # never y
    saved = sorted(tuple(t.shape) for t in y.grad_fn.saved_tensors)
    assert saved == sorted([(2, 67, 11, 3), (2, 32), (2, 32), (64,), (64,)])              # x, mean, rstd, weight, bias
    g_nc = four(dev(gy, cuda)).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)       # same values, other strides
    assert not g_nc.is_contiguous()
    gx, gw, gb = torch.autograd.grad(y, (xd, gd, bd), g_nc)
    for k, t in (("y", y), ("gx", gx), ("gw", gw), ("gb", gb)):
        assert np.array_equal(bits(t).reshape(-1), bits(want[k]).reshape(-1)), k
    # subsets of needs_input_grad
    x2, g2, b2 = four(dev(x, cuda)), dev(gamma, cuda).requires_grad_(), dev(beta, cuda)
    (gw2,) = torch.autograd.grad(pointnet2_utils.group_norm_act(x2, g2, b2, 32, GC.EPS, act), (g2,), four(dev(gy, cuda)))
    assert np.array_equal(bits(gw2), bits(want["gw"]))
    x3 = four(dev(x, cuda)).requires_grad_()
    (gx3,) = torch.autograd.grad(pointnet2_utils.group_norm_act(x3, dev(gamma, cuda), dev(beta, cuda), 32, GC.EPS, act),
                                 (x3,), four(dev(gy, cuda)))
    assert np.array_equal(bits(gx3).reshape(-1), bits(want["gx"]).reshape(-1))
    # without affine parameters
    (xp, _, _, gyp), refp = reference(shape, "normal", False, act)
    x4 = dev(xp, cuda).requires_grad_()
    y4 = pointnet2_utils.group_norm_act(x4, None, None, 32, GC.EPS, act)
    (gx4,) = torch.autograd.grad(y4, (x4,), dev(gyp, cuda))
    check(dict(y=y4.detach(), gx=gx4), refp, "autograd-plain-" + act)
    # a view with a storage offset: the scalar family, although S % 4 == 0 would allow the vector one
    shape_v = (1, 64, 12, 32)
    (xv, gav, bev, gyv), refv = reference(shape_v, "offset", True, act)
    assert GC.plan(64, 12, 32, 1)[1][0] == 1 and GC.plan(64, 12, 32, 0)[1][0] == 0
    x5, g5, b5 = dev(xv, cuda, offset=True).requires_grad_(), dev(gav, cuda).requires_grad_(), dev(bev, cuda).requires_grad_()
    y5 = pointnet2_utils.group_norm_act(x5, g5, b5, 32, GC.EPS, act)
    gx5, gw5, gb5 = torch.autograd.grad(y5, (x5, g5, b5), dev(gyv, cuda, offset=True))
    check(dict(y=y5.detach(), gx=gx5, gw=gw5, gb=gb5), refv, "autograd-offset-view-" + act)
    check(run((xv, gav, bev, gyv), 32, act, cuda, offset=True), refv, "c-offset-view-" + act)


# ---- the module path -------------------------------------------------------------------------------------------------
def explicit_sequential(seq, x):
    """What the stack computed before NormActSequential: its children in order, written out."""
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
            x = F.conv2d(x, m.weight, m.bias)
    return x


def evaluate(mod, inputs_, r, grads):
    """[out] + gradients of sum(out * r) w.r.t. every parameter and every floating input, float64 on the CPU."""
    inputs_ = [t.detach().clone().requires_grad_() if torch.is_tensor(t) and t.is_floating_point() else t
               for t in inputs_]
    out = mod(*inputs_)
    res = [out.detach().double().cpu()]
    if grads:
        wrt = list(mod.parameters()) + [t for t in inputs_ if torch.is_tensor(t) and t.requires_grad]
        res += [g.double().cpu() for g in torch.autograd.grad((out * r).sum(), wrt)]
    return res


def judge(label, names, want, off, on):
    """Errors as max |diff| / scale, scale = the tensor's largest float64 element -- or, for a gradient whose float64
    reference is below 1e-3 of the largest gradient element of the module (exactly zero in exact arithmetic, such as
    the time embedding's behind a one-channel-per-group norm: both errors are rounding noise), that largest element."""
    top = max([float(w.abs().max()) for w in want[1:]] or [0.0])
    failed = []
    for i, (name, w, a, b) in enumerate(zip(names, want, off, on)):
        scale = float(w.abs().max())
        if i > 0 and scale < 1e-3 * top:
            scale = top
        e_off, e_on = float((a - w).abs().max()) / scale, float((b - w).abs().max()) / scale
        print("%s %-32s scale %.3g  switch off %.3g  switch on %.3g" % (label, name, scale, e_off, e_on))
        if not e_on <= max(4.0 * e_off, 8.0 * GC.U):
            failed.append((name, e_off, e_on))
    assert not failed, (label, failed)


def on_and_off(fn):
    prev = _ext.set_fused_group_norm(False)
    try:
        off = fn()
        _ext.set_fused_group_norm(True)
        on = fn()
    finally:
        _ext.set_fused_group_norm(prev)
    return off, on


@pytest.mark.parametrize("activation", ["relu", "swish"])
def test_mlp_plus_t_emb_switch_on_against_switch_off_and_float64(cuda, activation):
    """Mlp_plus_t_emb([35, 32, 32, 64], bn, res_connect, include_t) on (2, 35, 5, 3): the forward for relu and swish,
    parameter and input gradients for swish (no mask can flip).

    Measured on an MI355X (switch off, switch on; the test prints every figure, DESIGN 7a.4 keeps them): out 3.1e-7,
    3.4e-7 with relu and 4.5e-7, 3.4e-7 with swish; the swish gradients 1.6e-8 .. 6.1e-7 and 1.6e-8 .. 9.2e-7, the
    switch-on error 0.65 x to 1.6 x the switch-off one."""
    torch.manual_seed(21)
    mod64 = Mlp_plus_t_emb([35, 32, 32, 64], bn=True, res_connect=True, include_t=True, activation=activation).double()
    gen = torch.Generator().manual_seed(22)
    x, t, r = torch.randn(2, 35, 5, 3, generator=gen), torch.randn(2, 128, generator=gen), torch.randn(2, 64, 5, 3, generator=gen)
    grads = activation == "swish"
    want = evaluate(mod64, [x.double(), t.double()], r.double(), grads)
    mod32 = copy.deepcopy(mod64).float().to(cuda)
    off, on = on_and_off(lambda: evaluate(mod32, [x.to(cuda), t.to(cuda)], r.to(cuda), grads))
    names = ["out"] + [n for n, _ in mod64.named_parameters()] + ["feature", "t_emb"]
    judge("mlp-" + activation, names, want, off, on)


def test_attention_module_switch_on_against_switch_off_and_float64(cuda):
    """AttentionModule(8, 35, 8, 35, 64) on matching shapes: its activations are ReLU, so the forward is judged."""
    torch.manual_seed(23)
    mod64 = AttentionModule(8, 35, 8, 35, 64).double()
    gen = torch.Generator().manual_seed(24)
    feat, gf, gfo = torch.randn(2, 8, 5, generator=gen), torch.randn(2, 35, 5, 3, generator=gen), torch.randn(2, 64, 5, 3, generator=gen)
    cnt = torch.randint(0, 4, (2, 5), generator=gen, dtype=torch.int32)
    want = evaluate(mod64, [feat.double(), gf.double(), gfo.double(), cnt], None, False)
    mod32 = copy.deepcopy(mod64).float().to(cuda)
    off, on = on_and_off(lambda: evaluate(mod32, [feat.to(cuda), gf.to(cuda), gfo.to(cuda), cnt.to(cuda)], None, False))
    judge("attention", ["out"], want, off, on)


def test_the_fused_modules_call_the_op_and_save_no_activation_output(cuda):
    """With the switch on a [conv, norm, act] stack runs one GroupNormAct per norm and no GroupNorm / ReLU node."""
    torch.manual_seed(25)
    mlp = build_shared_mlp([35, 32, 64], bn=True, activation="swish").to(cuda)
    x = torch.randn(2, 35, 5, 3, device=cuda)

    def node_names():
        out = mlp(x)                                       # kept alive: a custom Function's node lives with its output
        seen, todo, names = set(), [out.grad_fn], []
        while todo:
            n = todo.pop()
            if n is None or n in seen:
                continue
            seen.add(n)
            names.append(type(n).__name__)
            todo += [f for f, _ in n.next_functions]
        return names

    off, on = on_and_off(node_names)
    assert sum("GroupNormAct" in n for n in on) == 2 and not any("GroupNormAct" in n for n in off)
    assert not any("NativeGroupNorm" in n or "Sigmoid" in n or "Cat" in n for n in on)
    assert any("NativeGroupNorm" in n for n in off) and any("Sigmoid" in n for n in off)


def test_switch_off_gpu_modules_have_the_composition_s_bits_run_by_run(cuda):
    torch.manual_seed(26)
    as_bits = lambda t: t.contiguous().view(torch.int32)
    for bn_first in (False, True):
        for activation in ("relu", "swish"):
            mlp = build_shared_mlp([35, 32, 64], bn=True, bn_first=bn_first, bias=bn_first, activation=activation).to(cuda)
            x = torch.randn(2, 35, 5, 3, device=cuda)
            assert _ext.is_fused_group_norm() is False
            with torch.no_grad():
                want = explicit_sequential(mlp, x.clone())
                for _ in range(2):
                    assert torch.equal(as_bits(mlp(x.clone())), as_bits(want))
    mod = AttentionModule(8, 35, 8, 35, 64).to(cuda)
    feat, gf, gfo = torch.randn(2, 8, 5, device=cuda), torch.randn(2, 35, 5, 3, device=cuda), torch.randn(2, 64, 5, 3, device=cuda)
    with torch.no_grad():
        q = mod.feat_conv(feat.unsqueeze(-1)).expand(-1, -1, -1, 3)
        scores = explicit_sequential(mod.weight_conv, torch.cat([q, mod.grouped_feat_conv(gf)], dim=1))
        want = (explicit_sequential(mod.feat_out_conv, gfo.clone()) * F.softmax(scores, dim=-1)).sum(dim=-1)
        for _ in range(2):
            assert torch.equal(as_bits(mod(feat, gf, gfo.clone(), 'all')), as_bits(want))
