"""pdr_group_norm_act_add / pdr_group_norm_act_add_grad on the GPU, through _ext.group_norm_act_add /
group_norm_act_add_grad (thin wrappers of the two C calls), pointnet2_utils.group_norm_act_add and the module path under
set_fused_injection.

The op is pdr_group_norm_act followed by two fp32 additions, and its backward is pdr_group_norm_act_grad plus grad_e.
What the entries share is therefore tested by BITS against the existing entries on the same inputs (those stand under
the derived bounds of tests/test_group_norm_act_gpu.py); grad_e, the one new quantity, against its own bound and, bit
for bit, against an operation-for-operation emulation of the row order (tests/group_norm_act_add_cases.py).

Module level: the rule of DESIGN 7a.4 -- the switch-on error against the float64 module on the CPU is at most 4 x the
switch-off error, with a floor of 8 u -- on the output, every parameter gradient and every input gradient, for ReLU and
Swish.  ReLU seeds: a gradient is comparable only where no ReLU decision differs between the evaluations, so the seeds
45 ([35, 64, 64, 64]) and 54 ([64, 64, 64, 64]) are those of 40 .. 79 whose smallest |z| in front of a ReLU is largest,
measured on the CPU under float64_ops("oracle") at both dtypes: 1.8e-4 and 1.5e-4, with equal masks at both dtypes and
an fp32 error of z of 1.9e-6 and 2.2e-6."""
import copy

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import Mlp_plus_t_emb
from tests import group_norm_act_add_cases as AC
from tests import group_norm_act_cases as GC

pytestmark = pytest.mark.gpu

bits = GC.bits
_IN, _REF = {}, {}
PATTERN, AFFINE = "normal", True


def inputs(shape, which="both"):
    """Read-only host arrays (x, gamma, beta, gy, e, r) of a shape, computed once."""
    if shape not in _IN:
        arrays = GC.make(shape, PATTERN, AFFINE) + AC.terms(shape)
        for a in arrays:
            a.setflags(write=False)
        _IN[shape] = arrays
    x, gamma, beta, gy, e, r = _IN[shape]
    return x, gamma, beta, gy, (e if which in ("e", "both") else None), (r if which in ("r", "both") else None)


def reference(shape, act):
    if (shape, act) not in _REF:
        _REF[shape, act] = GC.reference(shape, *inputs(shape)[:4], act)
    return _REF[shape, act]


def dev(a, cuda, offset=False):
    """Device copy of a host array; offset=True: a contiguous view 4 bytes into its storage."""
    if a is None:
        return None
    t = torch.tensor(np.asarray(a))
    if not offset:
        return t.to(cuda)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


NAMES = ("y", "mean", "rstd", "gx", "gw", "gb", "ge")


def run(arrays, G, act, cuda, offset=False, need=(True, True, True, True), offset_r=None):
    """The seven outputs of the two new C calls as a dict of device tensors (a gradient not asked for: None)."""
    x, gamma, beta, gy, e, r = arrays
    xd, gd, bd, gyd = dev(x, cuda, offset), dev(gamma, cuda), dev(beta, cuda), dev(gy, cuda, offset)
    ed, rd = dev(e, cuda), dev(r, cuda, offset if offset_r is None else offset_r)
    y, mean, rstd = _ext.group_norm_act_add(xd, gd, bd, G, GC.EPS, act, ed, rd)
    gx, gw, gb, ge = _ext.group_norm_act_add_grad(xd, gd, bd, mean, rstd, gyd, G, act, *need)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, gx=gx, gw=gw, gb=gb, ge=ge)


def run_existing(arrays, G, act, cuda, offset=False):
    x, gamma, beta, gy = arrays[:4]
    xd, gd, bd, gyd = dev(x, cuda, offset), dev(gamma, cuda), dev(beta, cuda), dev(gy, cuda, offset)
    y, mean, rstd = _ext.group_norm_act(xd, gd, bd, G, GC.EPS, act)
    gx, gw, gb = _ext.group_norm_act_grad(xd, gd, bd, mean, rstd, gyd, G, act)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, gx=gx, gw=gw, gb=gb)


def composed(old, arrays, cuda):
    """(y_gna + e[:, :, None]) + r with torch's fp32 additions on the device."""
    y = old["y"]
    if arrays[4] is not None:
        y = y + dev(arrays[4], cuda)[:, :, None]
    if arrays[5] is not None:
        y = y + dev(arrays[5], cuda)
    return y


def check_grad_e(ge, gy, vec, label):
    got = ge.cpu().numpy()
    err = np.abs(got.astype(np.float64) - AC.row_sums_exact(gy)) / AC.grad_e_bound(gy)
    print(label, "grad_e worst error / bound %.3g" % err.max())
    assert not AC.outside(got, gy).any(), label                                  # pass-through rows included
    assert np.array_equal(bits(got), bits(AC.row_sums_emulated(gy, vec))), label


def against_the_existing_entry(shape, act, which, cuda, offset):
    B, C, S, G = shape
    arrays = inputs(shape, which)
    vec = 4 if GC.plan(C, S, G, 0 if offset else 1)[1][0] else 1
    assert vec == (1 if offset or S % 4 else 4)
    old, new = run_existing(arrays, G, act, cuda, offset), run(arrays, G, act, cuda, offset)
    for k in ("mean", "rstd", "gx", "gw", "gb"):
        assert torch.equal(old[k], new[k]) and np.array_equal(bits(old[k]), bits(new[k])), k
    assert torch.equal(new["y"], composed(old, arrays, cuda))
    check_grad_e(new["ge"], arrays[3], vec, "%s-%s-%s%s" % ("x".join(map(str, shape)), act, which,
                                                            "-offset" if offset else ""))


CASES = [(sh, act, w) for sh in AC.shapes() for act in GC.ACTS for w in AC.TERMS]
_id = lambda c: "%s-%s-%s" % ("x".join(map(str, c[0])), c[1], c[2])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_of_the_existing_entry_and_grad_e(cuda, case):
    """mean, rstd, grad_x, grad_gamma, grad_beta: the existing entries' bits; y: theirs followed by torch's two
    additions; grad_e: within u |sum| + S v sum|grad_y| of the exact row sum and bit-equal to the emulated order."""
    against_the_existing_entry(*case, cuda=cuda, offset=False)


@pytest.mark.parametrize("case", [c for c in CASES if c[0][2] % 4 == 0 and c[2] == "both"], ids=_id)
def test_scalar_family_through_a_view_four_bytes_into_its_storage(cuda, case):
    """The shapes the vector family would take, with x, grad_y and r offset: V = 1 in the emulation."""
    against_the_existing_entry(*case, cuda=cuda, offset=True)


@pytest.mark.parametrize("shape", AC.shapes(), ids=lambda s: "x".join(map(str, s)))
def test_without_terms_y_is_the_existing_entry_s(cuda, shape):
    for act in GC.ACTS:
        arrays = inputs(shape, "both")[:4] + (None, None)
        old, new = run_existing(arrays, shape[3], act, cuda), run(arrays, shape[3], act, cuda)
        for k in ("y", "mean", "rstd", "gx", "gw", "gb"):
            assert np.array_equal(bits(old[k]), bits(new[k])), (act, k)


@pytest.mark.parametrize("shape", AC.shapes()[:4], ids=lambda s: "x".join(map(str, s)))
def test_an_all_zero_grad_y_gives_exact_zeros(cuda, shape):
    x, gamma, beta, gy, e, r = inputs(shape)
    got = run((x, gamma, beta, np.zeros_like(gy), e, r), shape[3], "swish", cuda)
    assert not bits(got["ge"]).any()                                             # +0.0, bit for bit


SOME = [((2, 67, 33, 32), "relu"), ((2, 35, 7, 32), "swish"), ((2, 16, 20, 16), "none"), ((1, 131, 260, 32), "swish")]
_id2 = lambda c: "%s-%s" % ("x".join(map(str, c[0])), c[1])


@pytest.mark.parametrize("case", SOME + [(AC.shapes()[-1], "relu")], ids=_id2)
def test_same_bits_run_after_run_and_each_gradient_alone(cuda, case):
    shape, act = case
    arrays = inputs(shape)
    first, second = run(arrays, shape[3], act, cuda), run(arrays, shape[3], act, cuda)
    for k in NAMES:
        assert np.array_equal(bits(first[k]), bits(second[k])), k
    for i, k in enumerate(("gx", "gw", "gb", "ge")):
        need = tuple(j == i for j in range(4))
        alone = run(arrays, shape[3], act, cuda, need=need)
        assert [n for n in ("gx", "gw", "gb", "ge") if alone[n] is not None] == [k]
        assert np.array_equal(bits(alone[k]), bits(first[k])), k
    x, gamma, beta, gy, e, r = arrays
    xd, gyd = dev(x, cuda), dev(gy, cuda)
    with pytest.raises(RuntimeError, match="invalid argument"):                  # all four NULL
        _ext.group_norm_act_add_grad(xd, dev(gamma, cuda), dev(beta, cuda), first["mean"], first["rstd"], gyd, shape[3],
                                     act, False, False, False, False)


@pytest.mark.parametrize("case", SOME[:3], ids=_id2)
def test_a_cloud_of_a_batch_has_the_bits_of_its_own_call(cuda, case):
    shape, act = case
    assert shape[0] == 2
    x, gamma, beta, gy, e, r = inputs(shape)
    batched = run((x, gamma, beta, gy, e, r), shape[3], act, cuda)
    for b in range(shape[0]):
        alone = run((x[b:b + 1], gamma, beta, gy[b:b + 1], e[b:b + 1], r[b:b + 1]), shape[3], act, cuda)
        for k in ("y", "mean", "rstd", "gx", "ge"):
            assert np.array_equal(bits(batched[k])[b:b + 1], bits(alone[k])), (k, b)


def test_graph_capture_of_forward_and_backward(cuda):
    """Captured on a side stream, the graph replays with changed inputs and gives the eager call's bits."""
    shape, act = (2, 67, 33, 32), "swish"
    first = inputs(shape)
    second = tuple(np.ascontiguousarray(a[::-1]) if a.ndim == 1 else np.ascontiguousarray(a[:, ::-1]) for a in first)
    xd, gd, bd, gyd, ed, rd = (dev(a, cuda) for a in first)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y, mean, rstd = _ext.group_norm_act_add(xd, gd, bd, 32, GC.EPS, act, ed, rd)      # warm the allocator
        _ext.group_norm_act_add_grad(xd, gd, bd, mean, rstd, gyd, 32, act)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y, mean, rstd = _ext.group_norm_act_add(xd, gd, bd, 32, GC.EPS, act, ed, rd)
            gx, gw, gb, ge = _ext.group_norm_act_add_grad(xd, gd, bd, mean, rstd, gyd, 32, act)
    torch.cuda.current_stream().wait_stream(side)
    for arrays in (first, second):
        for t, a in zip((xd, gd, bd, gyd, ed, rd), arrays):
            t.copy_(torch.tensor(np.asarray(a)))
        for t in (y, mean, rstd, gx, gw, gb, ge):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(arrays, 32, act, cuda)
        for k, t in zip(NAMES, (y, mean, rstd, gx, gw, gb, ge)):
            assert np.array_equal(bits(t), bits(eager[k])), k


@pytest.mark.parametrize("shape", [(2, 35, 7, 32), (2, 16, 20, 16)], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_infinity_in_the_terms_propagate_as_torch_add_does(cuda, shape):
    x, gamma, beta, gy, e, r = inputs(shape)
    e, r = e.copy(), r.copy()
    e[0, 1], e[1, 2], e[0, 5] = np.nan, np.inf, -np.inf
    r[0, 3, 2], r[1, 0, 0], r[0, 5, 1] = np.nan, -np.inf, np.inf                  # (0, 5, 1): -inf + inf
    arrays = (x, gamma, beta, gy, e, r)
    old, new = run_existing(arrays, shape[3], "relu", cuda), run(arrays, shape[3], "relu", cuda)
    want = composed(old, arrays, cuda)
    assert torch.equal(torch.isnan(new["y"]), torch.isnan(want)) and bool(torch.isnan(want[0, 1]).all())
    assert bool(torch.isnan(want[0, 5, 1])) and int(torch.isnan(want).sum()) == shape[2] + 2
    assert torch.equal(torch.nan_to_num(new["y"], nan=7.0), torch.nan_to_num(want, nan=7.0))
    for k in ("gx", "gw", "gb"):                                                 # the backward reads neither term
        assert np.array_equal(bits(old[k]), bits(new[k])), k


@pytest.mark.parametrize("shape", [(1, 131, 260, 32), (2, 16, 20, 16), AC.shapes()[-1]],
                         ids=lambda s: "x".join(map(str, s)))
def test_a_misaligned_residual_takes_the_scalar_family(cuda, shape):
    """x and y aligned, r 4 bytes off: the vector family's 16-byte loads of r would be misaligned, so the call takes
    the scalar family; the two agree up to the summation order of the statistics.  Each is judged against the
    float64 reference under GC's bound of y carried through the two additions."""
    B, C, S, G = shape
    arrays = inputs(shape)
    for act in GC.ACTS:
        want, bound = AC.forward_reference(reference(shape, act), arrays[4], arrays[5])
        ref = reference(shape, act)
        for label, off_r in (("vector", False), ("scalar", True)):
            got = run(arrays, G, act, cuda, offset_r=off_r)
            y = got["y"].cpu().numpy().astype(np.float64)
            ratio = float((np.abs(y - want) / bound).max())
            stats = GC.worst_ratio(dict(mean=got["mean"].cpu().numpy(), rstd=got["rstd"].cpu().numpy()), ref)
            print("x".join(map(str, shape)), act, label, "y %.3g" % ratio, stats)
            assert ratio <= 1.0 and max(stats.values()) <= 1.0, (label, act, ratio, stats)


# ---- autograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", GC.ACTS)
def test_public_function_under_autograd(cuda, act):
    """pointnet2_utils.group_norm_act_add on a 4-d tensor: the C-level bits, grad_r = grad_y, nothing of the output's
    size saved but x, and subsets of needs_input_grad."""
    shape = (2, 67, 33, 32)                                                       # as (2, 67, 11, 3)
    arrays = inputs(shape)
    want = run(arrays, 32, act, cuda)
    four = lambda t: t.view(2, 67, 11, 3)
    leaf = lambda a, f=lambda t: t: f(dev(a, cuda)).requires_grad_()
    xd, gd, bd, ed, rd = leaf(arrays[0], four), leaf(arrays[1]), leaf(arrays[2]), leaf(arrays[4]), leaf(arrays[5], four)
    gyd = four(dev(arrays[3], cuda))
    y = pointnet2_utils.group_norm_act_add(xd, gd, bd, 32, GC.EPS, act, add=ed, residual=rd)
    assert type(y.grad_fn).__name__ == "GroupNormActAddBackward"
    saved = sorted(tuple(t.shape) for t in y.grad_fn.saved_tensors)
    assert saved == sorted([(2, 67, 11, 3), (2, 32), (2, 32), (64,), (64,)])     # x, mean, rstd, weight, bias
    assert [t.data_ptr() for t in y.grad_fn.saved_tensors if t.dim() == 4] == [xd.data_ptr()]
    gx, gw, gb, ge, gr = torch.autograd.grad(y, (xd, gd, bd, ed, rd), gyd)
    for k, t in (("y", y), ("gx", gx), ("gw", gw), ("gb", gb), ("ge", ge)):
        assert np.array_equal(bits(t).reshape(-1), bits(want[k]).reshape(-1)), k
    assert torch.equal(gr, gyd)
    # subsets: only e; only r (no kernel runs: a wrapper counts); e and the weight, without x
    for wrt, names in (((ed,), ("ge",)), ((ed, gd), ("ge", "gw")), ((xd, rd), ("gx", None))):
        y = pointnet2_utils.group_norm_act_add(xd, gd, bd, 32, GC.EPS, act, add=ed, residual=rd)
        for g, k in zip(torch.autograd.grad(y, wrt, gyd), names):
            assert torch.equal(g, gyd) if k is None else np.array_equal(bits(g).reshape(-1), bits(want[k]).reshape(-1))
    calls, real = [], _ext.group_norm_act_add_grad
    _ext.group_norm_act_add_grad = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        x2, r2 = four(dev(arrays[0], cuda)), leaf(arrays[5], four)
        y = pointnet2_utils.group_norm_act_add(x2, dev(arrays[1], cuda), dev(arrays[2], cuda), 32, GC.EPS, act,
                                               residual=r2)
        (g,) = torch.autograd.grad(y, (r2,), gyd)
    finally:
        _ext.group_norm_act_add_grad = real
    assert torch.equal(g, gyd) and not calls


def test_tensors_that_are_not_contiguous_are_copied(cuda):
    """x and the residual as channels-last views (what a 1x1 convolution returns for the transposed groups of an
    unfused group_knn), the embedding as a strided slice: the bits of the dense call."""
    shape, act = (2, 67, 33, 32), "relu"
    arrays = inputs(shape)
    want = run(arrays, 32, act, cuda)
    last = lambda a: dev(a, cuda).view(2, 67, 11, 3).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    xd, rd = last(arrays[0]).requires_grad_(), last(arrays[5]).requires_grad_()
    ed = torch.stack([dev(arrays[4], cuda)] * 2, dim=2)[:, :, 0].requires_grad_()
    assert not (xd.is_contiguous() or rd.is_contiguous() or ed.is_contiguous())
    gd, bd = dev(arrays[1], cuda), dev(arrays[2], cuda)
    y = pointnet2_utils.group_norm_act_add(xd, gd, bd, 32, GC.EPS, act, add=ed, residual=rd)
    gyd = dev(arrays[3], cuda).view(2, 67, 11, 3)
    gx, ge, gr = torch.autograd.grad(y, (xd, ed, rd), gyd)
    for k, t in (("y", y), ("gx", gx), ("ge", ge)):
        assert np.array_equal(bits(t.contiguous()).reshape(-1), bits(want[k]).reshape(-1)), k
    assert torch.equal(gr, gyd)


# ---- the module path --------------------------------------------------------------------------------------------------
SPECS = {"conv-residual": ([35, 64, 64, 64], 45), "identity-residual": ([64, 64, 64, 64], 54)}
SHAPE = (2, 12, 8)                                                                # B, N, K


def module_case(kind, activation):
    spec, seed = SPECS[kind]
    torch.manual_seed(seed)
    mod64 = Mlp_plus_t_emb(spec, bn=True, res_connect=True, include_t=True, include_condition=True,
                           include_second_condition=True, activation=activation).double()
    assert (mod64.res_connect is None) == (kind == "identity-residual")
    gen = torch.Generator().manual_seed(seed + 1)
    B, N, K = SHAPE
    args = [torch.randn(B, spec[0], N, K, generator=gen)] + [torch.randn(B, 128, generator=gen) for _ in range(3)]
    r = torch.randn(B, spec[-1], N, K, generator=gen)
    return mod64, args, r


def evaluate(mod, args, r):
    """[out] + gradients of sum(out * r) w.r.t. every parameter and every input, float64 on the CPU."""
    args = [t.detach().clone().requires_grad_() for t in args]
    out = mod(*args)
    wrt = list(mod.parameters()) + args
    return [out.detach().double().cpu()] + [g.double().cpu() for g in torch.autograd.grad((out * r).sum(), wrt)]


def judge(label, names, want, off, on):
    """The rule and the scale of tests/test_group_norm_act_gpu.py `judge`."""
    top = max(float(w.abs().max()) for w in want[1:])
    failed = []
    for i, (name, w, a, b) in enumerate(zip(names, want, off, on)):
        scale = float(w.abs().max())
        if i > 0 and scale < 1e-3 * top:
            scale = top
        e_off, e_on = float((a - w).abs().max()) / scale, float((b - w).abs().max()) / scale
        print("%s %-36s scale %.3g  switch off %.3g  switch on %.3g" % (label, name, scale, e_off, e_on))
        if not e_on <= max(4.0 * e_off, 8.0 * GC.U):
            failed.append((name, e_off, e_on))
    assert not failed, (label, failed)


def on_and_off(fn):
    prev = _ext.set_fused_injection(False)
    try:
        off = fn()
        _ext.set_fused_injection(True)
        on = fn()
    finally:
        _ext.set_fused_injection(prev)
    return off, on


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


@pytest.mark.parametrize("activation", ["relu", "swish"])
@pytest.mark.parametrize("kind", sorted(SPECS))
def test_mlp_plus_t_emb_switch_on_against_switch_off_and_float64(cuda, kind, activation):
    """Output, every parameter gradient and every input gradient (feature, t_emb, condition_emb,
    second_condition_emb).  64-wide layers: Cg = 2, so the norm behind an embedding leaves it a gradient.

    Measured on an MI355X (the test prints every figure, DESIGN 7a.9 keeps them): output 3.0e-7 to 4.1e-7 off and
    2.7e-7 to 4.1e-7 on; gradients 4.8e-8 to 9.9e-7 off and 2.4e-8 to 8.4e-7 on, the switch-on error 0.35 x to 1.43 x
    the switch-off one; t_emb 4.5e-7 to 9.9e-7 off, 3.1e-7 to 8.4e-7 on."""
    mod64, args, r = module_case(kind, activation)
    want = evaluate(mod64, [a.double() for a in args], r.double())
    mod32 = copy.deepcopy(mod64).float().to(cuda)
    off, on = on_and_off(lambda: evaluate(mod32, [a.to(cuda) for a in args], r.to(cuda)))
    names = ["out"] + [n for n, _ in mod64.named_parameters()] + ["feature", "t_emb", "condition_emb",
                                                                    "second_condition_emb"]
    assert len(names) == len(want)
    for n, w in zip(names, want):                            # the embeddings' paths carry a gradient: grad_e is judged
        assert float(w.abs().max()) > 0, n
    judge("%s-%s" % (kind, activation), names, want, off, on)


@pytest.mark.parametrize("kind", sorted(SPECS))
def test_one_node_per_stack_and_no_full_size_add(cuda, kind):
    mod64, args, _ = module_case(kind, "swish")
    mod = mod64.float().to(cuda)
    args = [a.to(cuda) for a in args]
    B, N, K = SHAPE

    def graph():
        out = mod(*args)                                     # kept alive: a custom Function's node lives with its output
        return out, node_names(out)

    (out_off, off), (out_on, on) = on_and_off(graph)
    assert sum(n == "GroupNormActAddBackward" for n in on) == 3 and "GroupNormActAddBackward" not in off
    # the Linear layers add their bias inside AddmmBackward; what is left of AddBackward0 with the switch off are the
    # three broadcast adds and the residual add, all of the output's size
    assert sum(n == "AddBackward0" for n in off) == 4 and not any(n.startswith("AddBackward") for n in on)
    assert not any("NativeGroupNorm" in n or "Sigmoid" in n for n in on)
    assert out_on.shape == out_off.shape == (B, 64, N, K)


def test_switch_off_bits_equal_the_parent_behaviour_run_by_run(cuda):
    """With the switch off the forward is the text it always was: first_mlp, + fc(t), second_mlp, + fc_condition(c),
    rest_mlp, + fc_second_condition(c2), + residual -- written out here -- and the same bits run after run."""
    as_bits = lambda t: t.contiguous().view(torch.int32)
    for kind in sorted(SPECS):
        for activation in ("relu", "swish"):
            mod64, args, _ = module_case(kind, activation)
            mod = mod64.float().to(cuda)
            x, t, c, c2 = (a.to(cuda) for a in args)
            assert _ext.is_fused_injection() is False
            with torch.no_grad():
                h = mod.first_mlp(x) + mod.fc(t).unsqueeze(2).unsqueeze(3)
                h = mod.second_mlp(h) + mod.fc_condition(c).unsqueeze(2).unsqueeze(3)
                h = mod.rest_mlp(h) + mod.fc_second_condition(c2).unsqueeze(2).unsqueeze(3)
                want = h + (x if mod.res_connect is None else mod.res_connect(x))
                for _ in range(2):
                    assert torch.equal(as_bits(mod(x, t, c, c2)), as_bits(want))


def test_a_stack_the_op_does_not_take_falls_to_the_composition_with_the_same_result(cuda):
    """bn_first and bn=False stacks do not end in [MyGroupNorm, act]: with the switch on they run `forward` and the
    two torch additions, the switch-off bits."""
    as_bits = lambda t: t.contiguous().view(torch.int32)
    gen = torch.Generator().manual_seed(61)
    x, t = torch.randn(2, 64, 5, 3, generator=gen).to(cuda), torch.randn(2, 128, generator=gen).to(cuda)
    for kw in (dict(bn=True, bn_first=True, bias=True), dict(bn=False)):
        torch.manual_seed(60)
        mod = Mlp_plus_t_emb([64, 64, 64], res_connect=True, include_t=True, **kw).to(cuda)
        with torch.no_grad():
            off, on = on_and_off(lambda: mod(x, t))
        assert torch.equal(as_bits(off), as_bits(on))
        _, names = on_and_off(lambda: node_names(mod(x, t)))
        assert "GroupNormActAddBackward" not in names
