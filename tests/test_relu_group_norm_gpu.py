"""pdr_relu_group_norm_cf / pdr_relu_group_norm_cf_grad on the GPU, through _ext.relu_group_norm /
relu_group_norm_grad (thin wrappers of the two C calls), pointnet2_utils.relu_group_norm and AttentionModule under
set_fused_score_norm.

Reference and bounds: tests/relu_group_norm_cases.py (the float64 composition on the CPU and bounds derived from the
kernels' stated operation chain; its module docstring justifies every term).  Every element of y, mean, rstd, grad_q,
grad_k, grad_gamma and grad_beta is asserted within its own bound; nothing is excluded.  The gradients are also held,
bit for bit, against the module's operation-for-operation emulation fed the statistics the forward saved.

Module level there is no closed bound through convolutions and several norms, so those tests use the rule of
tests/test_group_norm_act_gpu.py: the switch-off path's error against the same module in float64 on the CPU is
measured, and the switch-on error must be at most 4 x that, with a floor of 8 u."""
import copy

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import PointnetSAModule
from tests import relu_group_norm_cases as RC

pytestmark = pytest.mark.gpu

bits = RC.bits
_IN, _REF = {}, {}


def inputs(case, pattern, affine):
    key = (case, pattern, affine)
    if key not in _IN:
        arrays = RC.make(case, pattern, affine)
        for a in arrays:
            if a is not None:
                a.setflags(write=False)
        _IN[key] = arrays
    return _IN[key]


def reference(case, pattern, affine):
    """Host inputs and the float64 reference of a case, computed once and left unchanged."""
    key = (case, pattern, affine)
    if key not in _REF:
        _REF[key] = RC.reference(case, *inputs(case, pattern, affine))
    return inputs(case, pattern, affine), _REF[key]


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


def run(arrays, G, cuda, offset=False, need=(True, True, True, True)):
    """The seven outputs of the two C calls as a dict of device tensors (a gradient not asked for: None)."""
    q, k, gamma, beta, gy = arrays
    qd, kd, gd, bd, gyd = dev(q, cuda), dev(k, cuda, offset), dev(gamma, cuda), dev(beta, cuda), dev(gy, cuda, offset)
    y, mean, rstd = _ext.relu_group_norm(qd, kd, gd, bd, G, RC.EPS)
    gq, gk, gw, gb = _ext.relu_group_norm_grad(qd, kd, gd, bd, mean, rstd, gyd, G, *need)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, gq=gq, gk=gk, gw=gw, gb=gb)


def host(got):
    return {name: None if t is None else t.cpu().numpy() for name, t in got.items()}


def check(got, ref, label):
    worst = RC.worst_ratio(host(got), ref)
    print(label, " ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)


def check_bits(got, case, arrays, vec, label):
    """Gradients (and y, mean) against the emulation fed the kernel's own saved statistics."""
    h = host(got)
    emu = RC.emulate(case, *arrays, vec, mean=h["mean"], rstd=h["rstd"])
    assert np.array_equal(bits(h["mean"]), bits(emu["mean"])), label
    for name in ("gq", "gk", "gw", "gb"):
        assert (h[name] is None) == (emu[name] is None), (label, name)
        if h[name] is not None:
            diff = int((bits(h[name]) != bits(emu[name])).sum())
            assert diff == 0, (label, name, diff)


CASES = [(c, p, a) for c in RC.cases() for p in RC.PATTERNS for a in (False, True)]
_id = lambda c: "%s-%s-%s" % ("x".join(map(str, c[0])), c[1], "affine" if c[2] else "plain")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_seven_outputs_within_the_derived_bounds_and_gradients_equal_the_emulation(cuda, case):
    shape, pattern, affine = case
    B, C1, C2, N, K, G, C, Cg, Cn, S = RC.dims(shape)
    arrays, ref = reference(*case)
    vec = RC.plan(C1, C2, N, K, G, 1)[1][0]
    assert vec == int(K % 4 == 0)
    got = run(arrays, G, cuda)
    check(got, ref, _id(case))
    check_bits(got, shape, arrays, vec, _id(case))
    q, k, gamma, beta, gy = arrays
    x = RC.virtual(q, k)
    # pass-through channels: y = relu(x) and dx = x > 0 ? dy : +0, by bits
    if Cn < C:
        keep, zero = x[:, Cn:] > 0, np.zeros_like(x[:, Cn:])
        assert np.array_equal(bits(got["y"])[:, Cn:], bits(np.where(keep, x[:, Cn:], zero)))
        lo = max(Cn, C1)
        assert np.array_equal(bits(got["gk"])[:, lo - C1:], bits(np.where(x[:, lo:] > 0, gy[:, lo:], zero[:, lo - Cn:])))
    if pattern == "nonpos":
        for g in RC.nonpos_groups(shape):
            assert not bits(got["mean"])[:, g].any()                       # mean +0, variance 0
            for c in range(g * Cg, (g + 1) * Cg):
                want = np.float32(0.0) if beta is None else beta[c]
                assert np.array_equal(bits(got["y"])[:, c], bits(np.full((B, N, K), want, np.float32)))
                assert not (bits(got["gq"])[:, c] if c < C1 else bits(got["gk"])[:, c - C1]).any()
    if pattern == "zero_gy":
        for name in ("gq", "gk", "gw", "gb"):
            assert got[name] is None or not host(got)[name].any(), name      # zero everywhere (a negative gamma: -0)


SOME = [((2, 33, 34, 7, 4, 32), "normal", True), ((2, 32, 35, 5, 3, 32), "offset", True),
        ((2, 16, 4, 10, 2, 4), "normal", False), ((2, 0, 64, 9, 5, 32), "normal", True)]


@pytest.mark.parametrize("case", SOME + [(RC.cases()[-1], "normal", True)], ids=_id)
def test_same_bits_run_after_run_and_with_each_gradient_asked_for_alone(cuda, case):
    shape, pattern, affine = case
    arrays, G = inputs(*case), shape[5]
    first, second = run(arrays, G, cuda), run(arrays, G, cuda)
    for name in RC.OUTPUTS:
        assert (first[name] is None) == (second[name] is None)
        assert first[name] is None or np.array_equal(bits(first[name]), bits(second[name])), name
    for i, name in enumerate(("gq", "gk", "gw", "gb")):
        if first[name] is None:
            continue
        need = tuple(j == i for j in range(4))
        alone = run(arrays, G, cuda, need=need)
        assert [n for n in ("gq", "gk", "gw", "gb") if alone[n] is not None] == [name]
        assert np.array_equal(bits(alone[name]), bits(first[name])), name


@pytest.mark.parametrize("case", SOME + [(RC.cases()[-1], "normal", True)], ids=_id)
def test_a_cloud_of_a_batch_has_the_bits_of_its_own_call(cuda, case):
    shape, pattern, affine = case
    assert shape[0] == 2
    q, k, gamma, beta, gy = inputs(*case)
    batched = run((q, k, gamma, beta, gy), shape[5], cuda)
    for b in range(2):
        alone = run((None if q is None else q[b:b + 1], k[b:b + 1], gamma, beta, gy[b:b + 1]), shape[5], cuda)
        for name in ("y", "mean", "rstd", "gq", "gk"):
            if batched[name] is not None:
                assert np.array_equal(bits(batched[name])[b:b + 1], bits(alone[name])), (name, b)


@pytest.mark.parametrize("case", [((1, 32, 137, 16, 8, 32), "normal", True), ((2, 33, 34, 7, 4, 32), "offset", True),
                                  ((1, 40, 24, 6, 8, 32), "nonpos", False)], ids=_id)
def test_a_view_four_bytes_into_its_storage_takes_the_scalar_family(cuda, case):
    shape, pattern, affine = case
    B, C1, C2, N, K, G = shape
    arrays, ref = reference(*case)
    assert RC.plan(C1, C2, N, K, G, 1)[1][0] == 1 and RC.plan(C1, C2, N, K, G, 0)[1][0] == 0
    got = run(arrays, G, cuda, offset=True)
    check(got, ref, "offset-view-" + _id(case))
    check_bits(got, shape, arrays, 0, "offset-view-" + _id(case))


def test_a_nan_in_q_or_k_reaches_y(cuda):
    shape = (2, 33, 34, 7, 4, 32)
    B, C1, C2, N, K, G, C, Cg, Cn, S = RC.dims(shape)
    q, k, gamma, beta, gy = (None if a is None else a.copy() for a in inputs(shape, "normal", True))
    q[0, 3, 2] = np.nan                                 # group 1 of cloud 0, a q-only group
    k[1, C2 - 1, 4, 1] = np.nan                         # the last channel of cloud 1: a pass-through one
    k[1, 5, 0, 0] = -np.nan                             # group (C1 + 5) / Cg of cloud 1
    y = host(run((q, k, gamma, beta, gy), G, cuda))["y"]
    assert np.isnan(y[0, 2:4]).all() and np.isnan(y[1, (C1 + 5) // Cg * Cg:(C1 + 5) // Cg * Cg + Cg]).all()
    assert np.isnan(y[1, C - 1, 4, 1]) and np.isnan(y[1, C - 1]).sum() == 1
    clean = np.ones(y.shape, bool)
    clean[0, 2:4] = False
    clean[1, (C1 + 5) // Cg * Cg:(C1 + 5) // Cg * Cg + Cg] = False
    clean[1, C - 1, 4, 1] = False
    assert np.isfinite(y[clean]).all()


def test_current_stream_and_graph_capture_of_forward_and_backward(cuda):
    """Both calls launch on torch's current stream without a hidden synchronisation: captured on a side stream (a
    linear sequence, no parallel branches), the graph replays with changed inputs and gives the eager call's bits."""
    shape = (2, 33, 34, 7, 4, 32)
    first, second = inputs(shape, "normal", True), inputs(shape, "offset", True)
    qd, kd, gd, bd, gyd = (dev(a, cuda) for a in first)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y, mean, rstd = _ext.relu_group_norm(qd, kd, gd, bd, 32, RC.EPS)      # warm the allocator outside the capture
        _ext.relu_group_norm_grad(qd, kd, gd, bd, mean, rstd, gyd, 32)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y, mean, rstd = _ext.relu_group_norm(qd, kd, gd, bd, 32, RC.EPS)
            gq, gk, gw, gb = _ext.relu_group_norm_grad(qd, kd, gd, bd, mean, rstd, gyd, 32)
    torch.cuda.current_stream().wait_stream(side)
    for arrays in (first, second):
        for t, a in zip((qd, kd, gd, bd, gyd), arrays):
            t.copy_(torch.tensor(np.asarray(a)))
        for t in (y, mean, rstd, gq, gk, gw, gb):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(arrays, 32, cuda)
        for name, t in zip(RC.OUTPUTS, (y, mean, rstd, gq, gk, gw, gb)):
            assert np.array_equal(bits(t), bits(eager[name])), name


def test_public_function_under_autograd(cuda):
    """pointnet2_utils.relu_group_norm: the C-level bits; what it saves; a non-contiguous grad_out; needs_input_grad
    subsets; q=None."""
    shape = (2, 33, 34, 7, 4, 32)
    B, C1, C2, N, K, G = shape
    (q, k, gamma, beta, gy), ref = reference(shape, "normal", True)
    want = run((q, k, gamma, beta, gy), G, cuda)
    leaf = lambda a: dev(a, cuda).requires_grad_()
    qd, kd, gd, bd = leaf(q), leaf(k), leaf(gamma), leaf(beta)
    y = pointnet2_utils.relu_group_norm(kd, gd, bd, G, RC.EPS, q=qd)
    assert tuple(y.shape) == (B, C1 + C2, N, K)
    saved = sorted(tuple(t.shape) for t in y.grad_fn.saved_tensors)
    assert saved == sorted([(B, C1, N), (B, C2, N, K), (B, G), (B, G), (64,), (64,)])   # q, k, mean, rstd, weight, bias
    assert all(t.data_ptr() != y.data_ptr() for t in y.grad_fn.saved_tensors)            # never y
    g_nc = dev(gy, cuda).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)             # same values, other strides
    assert not g_nc.is_contiguous()
    grads = torch.autograd.grad(y, (qd, kd, gd, bd), g_nc)
    for name, t in zip(("y", "gq", "gk", "gw", "gb"), (y,) + grads):
        assert np.array_equal(bits(t), bits(want[name])), name
    # subsets of needs_input_grad: q alone, the weight alone, k and the bias
    for wanted in (("gq",), ("gw",), ("gk", "gb")):
        ts = dict(gq=dev(q, cuda), gk=dev(k, cuda), gw=dev(gamma, cuda), gb=dev(beta, cuda))
        for name in wanted:
            ts[name].requires_grad_()
        out = pointnet2_utils.relu_group_norm(ts["gk"], ts["gw"], ts["gb"], G, RC.EPS, q=ts["gq"])
        got = torch.autograd.grad(out, [ts[name] for name in wanted], dev(gy, cuda))
        for name, t in zip(wanted, got):
            assert np.array_equal(bits(t), bits(want[name])), (wanted, name)
    # q=None, with and without parameters, under the bounds and with the C call's bits
    shape0 = (2, 0, 64, 9, 5, 32)
    for affine in (True, False):
        (_, k0, ga0, be0, gy0), ref0 = reference(shape0, "normal", affine)
        want0 = run((None, k0, ga0, be0, gy0), 32, cuda)
        k0d = leaf(k0)
        params = [leaf(ga0), leaf(be0)] if affine else [None, None]
        y0 = pointnet2_utils.relu_group_norm(k0d, params[0], params[1], 32, RC.EPS)
        g0 = torch.autograd.grad(y0, [k0d] + [p for p in params if p is not None], dev(gy0, cuda))
        got0 = dict(y=y0.detach(), gk=g0[0], gw=g0[1] if affine else None, gb=g0[2] if affine else None)
        check(got0, ref0, "autograd-no-q-%s" % ("affine" if affine else "plain"))
        for name, t in got0.items():
            assert t is None or np.array_equal(bits(t), bits(want0[name])), name


# ---- the module path -------------------------------------------------------------------------------------------------
def evaluate(mod, inputs_, r):
    """[out] + gradients of sum(out * r) w.r.t. every parameter and every floating input, as float64 CPU tensors (a
    module that returns (new_xyz, new_features) is judged on the features)."""
    inputs_ = [t.detach().clone().requires_grad_() if torch.is_tensor(t) and t.is_floating_point() else t
               for t in inputs_]
    out = mod(*inputs_)
    if isinstance(out, tuple):
        out = out[1]
    wrt = list(mod.parameters()) + [t for t in inputs_ if torch.is_tensor(t) and t.requires_grad]
    grads = torch.autograd.grad((out * r).sum(), wrt, allow_unused=True)
    return [out.detach().double().cpu()] + [torch.zeros_like(w).double().cpu() if g is None else g.double().cpu()
                                           for g, w in zip(grads, wrt)]


def judge(label, names, want, off, on):
    """The rule of tests/test_group_norm_act_gpu.py: errors as max |diff| / scale, scale = the tensor's largest
    reference element -- or, for a gradient whose reference is below 1e-3 of the module's largest gradient element,
    that largest element; the switch-on error is at most 4 x the switch-off error, with a floor of 8 u."""
    top = max([float(w.abs().max()) for w in want[1:]] or [0.0])
    failed = []
    for i, (name, w, a, b) in enumerate(zip(names, want, off, on)):
        scale = float(w.abs().max())
        if i > 0 and scale < 1e-3 * top:
            scale = top
        e_off, e_on = float((a - w).abs().max()) / scale, float((b - w).abs().max()) / scale
        print("%s %-34s scale %.3g  switch off %.3g  switch on %.3g  ratio %.3g"
              % (label, name, scale, e_off, e_on, e_on / e_off if e_off else float("inf")))
        if not e_on <= max(4.0 * e_off, 8.0 * RC.U):
            failed.append((name, e_off, e_on))
    assert not failed, (label, failed)


def on_and_off(fn):
    prev = _ext.set_fused_score_norm(False)
    try:
        off = fn()
        _ext.set_fused_score_norm(True)
        on = fn()
    finally:
        _ext.set_fused_score_norm(prev)
    return off, on


@pytest.mark.parametrize("count", ["tensor", "all"])
def test_attention_module_switch_on_against_switch_off_and_float64(cuda, count):
    """AttentionModule(8, 35, 8, 35, 64) at B = 2, N = 12, K = 8 against the same module in float64 on the CPU: the
    output and every parameter and input gradient under the 4 x rule.  (C1 = 32, C2 = 35: 67 channels, Cg = 2, 3
    pass-through channels; the second link has 64.)

    Measured on an MI355X (switch off, switch on; the test prints every figure, DESIGN 7a.7 keeps them): with a count
    tensor out 4.14e-7, 4.14e-7, gradients 1.7e-8 .. 7.1e-7 and 1.8e-8 .. 6.8e-7, the switch-on error 0.62 x to 1.65 x
    the switch-off one; with 'all' out 2.38e-7, 2.24e-7, ratios 0.75 x to 1.35 x."""
    torch.manual_seed(31)
    mod64 = AttentionModule(8, 35, 8, 35, 64).double()
    gen = torch.Generator().manual_seed(32)
    B, N, K = 2, 12, 8
    feat, gf = torch.randn(B, 8, N, generator=gen), torch.randn(B, 35, N, K, generator=gen)
    gfo, r = torch.randn(B, 64, N, K, generator=gen), torch.randn(B, 64, N, generator=gen)
    cnt = 'all' if count == "all" else torch.randint(0, K + 1, (B, N), generator=gen, dtype=torch.int32)
    want = evaluate(mod64, [feat.double(), gf.double(), gfo.double(), cnt], r.double())
    mod32 = copy.deepcopy(mod64).float().to(cuda)
    on_dev = lambda t: t.to(cuda) if torch.is_tensor(t) else t
    off, on = on_and_off(lambda: evaluate(mod32, [on_dev(t) for t in (feat, gf, gfo, cnt)], r.to(cuda)))
    names = ["out"] + [n for n, _ in mod64.named_parameters()] + ["feat", "grouped_feat", "grouped_feat_out"]
    assert len(names) == len(want) == len(on)
    judge("attention-" + count, names, want, off, on)


def node_names(out):
    seen, todo, names = set(), [out.grad_fn], []
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.append(type(n).__name__)
        todo += [f for f, _ in n.next_functions]
    return names


def test_the_score_head_s_graph_with_the_switch_on_and_off(cuda):
    """Switch on: two ReluGroupNorm nodes and no cat, expand or ReLU node under `scores`; switch off: today's graph."""
    torch.manual_seed(33)
    mod = AttentionModule(8, 35, 8, 35, 64).to(cuda)
    feat = torch.randn(2, 8, 12, device=cuda, requires_grad=True)
    gf = torch.randn(2, 35, 12, 8, device=cuda, requires_grad=True)

    def names():
        scores = mod.score_head(feat, gf)                  # kept alive: a custom Function's node lives with its output
        assert tuple(scores.shape) == (2, 64, 12, 8)
        return node_names(scores)

    off, on = on_and_off(names)
    assert sum("ReluGroupNorm" in n for n in on) == 2 and not any("ReluGroupNorm" in n for n in off)
    assert not any(("Cat" in n or "Expand" in n or "Relu" in n) and "ReluGroupNorm" not in n for n in on), on
    assert sum("ReluBackward" in n for n in off) == 2 and sum("NativeGroupNormBackward" in n for n in off) == 2
    assert any("ExpandBackward" in n for n in off) and sum("CatBackward" in n for n in off) == 2, off
    # an attention_bn=False head has no norm: the composition, whatever the switch says
    plain = AttentionModule(8, 35, 8, 35, 64, attention_bn=False).to(cuda)
    off, on = on_and_off(lambda: node_names(plain.score_head(feat, gf)))
    assert off == on and not any("ReluGroupNorm" in n for n in on)


def double_ops(mp):
    """Patch the module path for a float64 evaluation WITH gradients (as tests/test_query_group_gpu.py does): FPS and
    the ball query decide on the fp32 cast of their coordinates (the decisions of the fp32 run), gather and group are
    torch indexing in the input's dtype."""
    fps, ball = pointnet2_utils.furthest_point_sample, pointnet2_utils.ball_query
    f32 = lambda t: t.detach().float().contiguous()

    def gather(points, idx):                                 # (B, C, N), (B, m) -> (B, C, m)
        return points.gather(2, idx.long().unsqueeze(1).expand(-1, points.shape[1], -1))

    def group(points, idx):                                  # (B, C, N), (B, np, ns) -> (B, C, np, ns)
        return gather(points, idx.reshape(idx.shape[0], -1)).reshape(*points.shape[:2], *idx.shape[1:])
    mp.setattr(pointnet2_utils, "furthest_point_sample", lambda xyz, n: fps(f32(xyz), n))
    mp.setattr(pointnet2_utils, "ball_query", lambda r, ns, xyz, new_xyz: ball(r, ns, f32(xyz), f32(new_xyz)))
    mp.setattr(pointnet2_utils, "gather_operation", gather)
    mp.setattr(pointnet2_utils, "grouping_operation", group)


def test_sa_module_with_attention_switch_on_against_switch_off_and_float64(cuda, monkeypatch):
    """A PointnetSAModule with attention at npoint = 8, nsample = 4, N = 24 (Swish in its MLP, so the only ReLUs are
    the attention module's): new features and every parameter and input gradient, the switch on against off under
    the same 4 x rule, both against the module in float64 with the fp32 run's sampling and grouping decisions.

    Measured on an MI355X: new_features 3.25e-7 off, 3.86e-7 on; gradients 7.5e-9 .. 6.4e-7 and 5.2e-9 .. 6.0e-7, the
    switch-on error 0.70 x to 1.45 x the switch-off one."""
    torch.manual_seed(34)
    mod = PointnetSAModule([16, 32, 32], npoint=8, radius=0.6, nsample=4, include_abs_coordinate=True,
                           include_center_coordinate=True, activation='swish',
                           attention_setting=dict(use_attention_module=True, attention_bn=True,
                                                  transform_grouped_feat_out=True, last_activation=True)).to(cuda)
    gen = torch.Generator().manual_seed(35)
    xyz, feats = torch.rand(2, 24, 3, generator=gen).to(cuda), torch.randn(2, 16, 24, generator=gen).to(cuda)
    r = torch.randn(2, 32, 8, generator=gen).to(cuda)
    with monkeypatch.context() as mp:
        double_ops(mp)
        want = evaluate(copy.deepcopy(mod).double(), [xyz.double(), feats.double()], r.double())
    off, on = on_and_off(lambda: evaluate(mod, [xyz, feats], r))
    names = ["new_features"] + [n for n, _ in mod.named_parameters()] + ["xyz", "features"]
    assert len(names) == len(want) == len(on)
    judge("sa-module", names, want, off, on)
