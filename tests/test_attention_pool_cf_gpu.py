"""pdr_attention_pool_cf / pdr_attention_pool_cf_grad on the GPU, through _ext.attention_pool / attention_pool_grad
(thin wrappers of the two C calls), pointnet2_utils.attention_pool and AttentionModule.

Reference and bounds: tests/attention_pool_cf_cases.py (the float64 composition on the CPU and bounds derived from the
kernel's stated operation chain; its module docstring justifies every constant).  Every element of out, grad_values and
of grad_scores at valid slots is asserted within its own bound; grad_scores at masked slots is checked by bits.

Module level there is no closed bound through two convs and GroupNorms, so the test measures the COMPOSITION's error
against float64 per tensor, as max |diff| / rms(float64 tensor), and requires the fused path's error to be at most 4 x
that or 1e-6, whichever is larger: two fp32 chains of the same length that differ in rounding order only."""
import copy

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule
from tests import attention_pool_cf_cases as AC

pytestmark = pytest.mark.gpu

bits = AC.bits
_REF = {}


def reference(shape, mode, pattern):
    """Host inputs and the float64 reference of a case, computed once and left unchanged."""
    key = (shape, mode, pattern)
    if key not in _REF:
        s, v, cnt, g = AC.make(shape, mode, pattern)
        ref = AC.reference(s, v, cnt, g)
        for a in (s, v, g) + (() if cnt is None else (cnt,)):
            a.setflags(write=False)
        _REF[key] = (s, v, cnt, g, ref)
    return _REF[key]


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


def run(s, v, cnt, g, cuda, offset=False, need=(True, True)):
    """(out, grad_scores, grad_values) of the two C calls, device tensors (a gradient not asked for: None)."""
    sd, vd, cd, gd = dev(s, cuda, offset), dev(v, cuda, offset), dev(cnt, cuda), dev(g, cuda)
    out = _ext.attention_pool(sd, vd, cd)
    gs, gv = _ext.attention_pool_grad(sd, vd, cd, gd, need[0], need[1])
    torch.cuda.synchronize()
    return out, gs, gv


def check(got, ref, label):
    """Every element within its derived bound (printed first); masked grad_scores exactly +0.0f."""
    out, gs, gv = (t.cpu().numpy().astype(np.float64) for t in got)
    for name, have, want, bound, sel in (("out", out, ref["out"], ref["b_out"], None),
                                         ("grad_values", gv, ref["gv"], ref["b_gv"], None),
                                         ("grad_scores", gs, ref["gs"], ref["b_gs"], ~ref["masked"])):
        err = np.abs(have - want)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        if sel is not None:
            ratio = np.where(sel, ratio, 0.0)
        print("%s %s: max |err| %.3g, max err / bound %.3g" % (label, name, err.max(), ratio.max()))
        assert np.isfinite(have).all(), (label, name)
        assert ratio.max() <= 1.0, (label, name, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    assert not bits(got[1])[ref["masked"]].any(), (label, "grad_scores at masked slots is not +0.0f")


CASES = [(sh, m, p) for sh in AC.SHAPES for m in AC.COUNT_MODES for p in AC.PATTERNS]
_id = lambda c: "%s-%s-%s" % ("x".join(map(str, c[0])), c[1], c[2])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_and_backward_within_the_derived_bounds(cuda, case):
    shape, mode, pattern = case
    s, v, cnt, g, ref = reference(*case)
    rc, plan = AC.plan(shape[3], 1)
    assert rc == 0 and plan[0] == int(shape[3] % 4 == 0)
    got = run(s, v, cnt, g, cuda)
    check(got, ref, _id(case))
    if mode != "none":
        # other junk in the masked score slots: not a bit of any output changes
        s2 = AC.make(shape, mode, pattern, junk=1)[0]
        assert np.array_equal(s2[~ref["masked"]], s[~ref["masked"]])
        assert ref["masked"].sum() < 32 or not np.array_equal(s2, s)
        other = run(s2, v, cnt, g, cuda)
        for a, b in zip(got, other):
            assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("shape", [(2, 3, 9, 8), (2, 33, 65, 32), (1, 3, 11, 33)], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_run_after_run_and_with_one_gradient_only(cuda, shape):
    s, v, cnt, g, _ = reference(shape, "random", "normal")
    first = run(s, v, cnt, g, cuda)
    second = run(s, v, cnt, g, cuda)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b))
    _, gs_only, none_v = run(s, v, cnt, g, cuda, need=(True, False))
    _, none_s, gv_only = run(s, v, cnt, g, cuda, need=(False, True))
    assert none_v is None and none_s is None
    assert np.array_equal(bits(gs_only), bits(first[1])) and np.array_equal(bits(gv_only), bits(first[2]))


def test_more_rows_than_one_workgroup_or_grid_pass_by_a_non_multiple(cuda):
    """Rows derived from the plan: where the grid strides (plan[3] > 0) more rows than one grid pass, and otherwise more
    than three workgroups, in both cases by a non-multiple of the rows per workgroup."""
    for K in (4, 12, 16, 64, 5):
        rc, plan = AC.plan(K, 1)
        assert rc == 0
        rows_per_wg, per_pass = plan[2], plan[3]
        if per_pass > 0:
            # a pass covers every lane group once: rows of one pass are a multiple of rows_per_wg; reach just past one
            rows = per_pass * rows_per_wg * 2 + rows_per_wg + 1
        else:
            rows = 3 * rows_per_wg + 1
        assert rows * K < 1 << 22, "a grid pass too large for a quick test: shrink the grid or derive another shape"
        N = 7
        C = (rows + N - 1) // N
        shape = (1, C, N, K)
        assert C * N > 3 * rows_per_wg and (C * N) % rows_per_wg != 0
        s, v, cnt, g = AC.make(shape, "random", "normal")
        check(run(s, v, cnt, g, cuda), AC.reference(s, v, cnt, g), "rows-K%d" % K)


@pytest.mark.parametrize("shape", [(2, 3, 9, 8), (1, 4, 130, 16), (1, 3, 7, 12)], ids=lambda s: "x".join(map(str, s)))
def test_a_view_with_a_storage_offset_takes_the_scalar_family_and_agrees(cuda, shape):
    s, v, cnt, g, ref = reference(shape, "random", "spread")
    assert AC.plan(shape[3], 1)[1][0] == 1 and AC.plan(shape[3], 0)[1][0] == 0    # aligned: vector; this view: scalar
    check(run(s, v, cnt, g, cuda, offset=True), ref, "offset-" + "x".join(map(str, shape)))


@pytest.mark.parametrize("mode", ["random", "none"])
def test_public_function_under_autograd_has_the_c_level_bits(cuda, mode):
    shape = (2, 33, 65, 32)
    s, v, cnt, g, _ = reference(shape, mode, "normal")
    want = run(s, v, cnt, g, cuda)
    sd, vd = dev(s, cuda).requires_grad_(), dev(v, cuda).requires_grad_()
    count = 'all' if cnt is None else dev(cnt, cuda)
    out = pointnet2_utils.attention_pool(sd, vd, count)
    gs, gv = torch.autograd.grad(out, (sd, vd), dev(g, cuda))
    for a, b in zip((out, gs, gv), want):
        assert np.array_equal(bits(a), bits(b))
    # needs_input_grad: only the values require a gradient
    s2, v2 = dev(s, cuda), dev(v, cuda).requires_grad_()
    (gv2,) = torch.autograd.grad(pointnet2_utils.attention_pool(s2, v2, count), (v2,), dev(g, cuda))
    assert np.array_equal(bits(gv2), bits(want[2]))


def test_current_stream_and_graph_capture_of_forward_and_backward(cuda):
    """Forward and backward launch on torch's current stream without a hidden synchronisation or allocation of their
    own: captured on a side stream, the graph replays with changed inputs."""
    shape = (2, 5, 33, 16)
    first = AC.make(shape, "random", "normal")
    second = AC.make(shape, "random", "spread")
    sd, vd, cd, gd = (dev(a, cuda) for a in first)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _ext.attention_pool_grad(sd, vd, cd, gd)                 # warm the allocator outside the capture
        _ext.attention_pool(sd, vd, cd)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = _ext.attention_pool(sd, vd, cd)
            gs, gv = _ext.attention_pool_grad(sd, vd, cd, gd)
    torch.cuda.current_stream().wait_stream(side)
    for host in (first, second):
        for t, a in zip((sd, vd, cd, gd), host):
            t.copy_(torch.from_numpy(a))
        for t in (out, gs, gv):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(*host, cuda)
        for a, b in zip((out, gs, gv), eager):
            assert np.array_equal(bits(a), bits(b))


def test_attention_module_fused_against_composition_and_float64(cuda):
    """AttentionModule(8, 11, 8, 11, 32), B = 2, N = 20, K = 8, random counts in [0, K]: output and the gradient of a
    random linear functional w.r.t. every parameter and the three inputs, switch on and off on the GPU, against float64
    on the CPU from the same parameters.

    Measured (max |diff| / rms of the float64 tensor; composition, fused): out 9.4e-7, 9.4e-7; the parameters and inputs
    with a non-zero gradient 2.4e-7 .. 2.3e-6 for either path, the fused error between 0.6 x and 1.5 x the
    composition's.  Three gradients are zero in exact arithmetic -- weight_conv.4.group_norm.bias and weight_conv.5.bias
    (softmax is invariant to a shift of all valid slots of a row) and feat_out_conv.0.bias (a one-channel-per-group
    GroupNorm follows) -- so their float64 rms is 1e-16 .. 1e-15 and both ratios are rounding noise over rounding
    noise: 1.2e9 / 1.3e9, 1.0e9 / 1.8e9, 1.6e9 / 1.4e9."""
    torch.manual_seed(11)
    B, N, K = 2, 20, 8
    mod64 = AttentionModule(8, 11, 8, 11, 32).double()
    gen = torch.Generator().manual_seed(12)
    host = [torch.randn(B, 8, N, generator=gen), torch.randn(B, 11, N, K, generator=gen),
            torch.randn(B, 32, N, K, generator=gen)]
    cnt = torch.randint(0, K + 1, (B, N), generator=gen, dtype=torch.int32)
    R = torch.randn(B, 32, N, generator=gen)

    def evaluate(mod, inputs, count, r):
        inputs = [t.detach().clone().requires_grad_() for t in inputs]
        out = mod(*inputs, count)
        params = list(mod.parameters())
        grads = torch.autograd.grad((out * r).sum(), params + inputs)
        return [out.detach().double().cpu()] + [t.double().cpu() for t in grads]

    names = ["out"] + [n for n, _ in mod64.named_parameters()] + ["feat", "grouped_feat", "grouped_feat_out"]
    want = evaluate(mod64, [t.double() for t in host], cnt, R.double())
    mod32 = copy.deepcopy(mod64).float().to(cuda)
    prev = _ext.is_fused_attention_pool()
    try:
        _ext.set_fused_attention_pool(False)
        comp = evaluate(mod32, [t.to(cuda) for t in host], cnt.to(cuda), R.to(cuda))
        _ext.set_fused_attention_pool(True)
        fused = evaluate(mod32, [t.to(cuda) for t in host], cnt.to(cuda), R.to(cuda))
    finally:
        _ext.set_fused_attention_pool(prev)
    failed = []
    for name, w, c, f in zip(names, want, comp, fused):
        rms = float(w.pow(2).mean().sqrt())
        e_comp, e_fused = float((c - w).abs().max()) / rms, float((f - w).abs().max()) / rms
        print("%-28s rms %.3g  composition %.3g  fused %.3g" % (name, rms, e_comp, e_fused))
        if not e_fused <= max(4.0 * e_comp, 1e-6):
            failed.append((name, e_comp, e_fused))
    assert not failed, failed
