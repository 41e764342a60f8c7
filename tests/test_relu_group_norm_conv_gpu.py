"""pdr_relu_group_norm_conv_cf / _grad_input / _grad_weight on the GPU, through _ext.relu_group_norm_conv* (thin wrappers
of the C calls), pointnet2_utils.relu_group_norm_conv and AttentionModule under set_fused_score_conv.

Bits: mean / rstd equal those of _ext.relu_group_norm; out and the input gradient equal the emulated fma chains of
tests/relu_group_norm_conv_cases.py (where the 80-bit emulation may have rounded twice, the Fraction-exact chain); the
final gradients equal _ext.relu_group_norm_grad fed the input-gradient buffer.  Bounds: out against the float64
composition, grad_W / grad_bias against float64 sums, as derived in the helper; every worst ratio is printed."""
import copy

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule
from tests import relu_group_norm_cases as RC
from tests import relu_group_norm_conv_cases as CC
from tests.test_relu_group_norm_gpu import dev, evaluate, judge, node_names

pytestmark = pytest.mark.gpu

bits = RC.bits
_IN, _REF = {}, {}


def inputs(case, pattern, affine):
    key = (case, pattern, affine)
    if key not in _IN:
        arrays = CC.make(case, pattern, affine)
        for a in arrays:
            if a is not None:
                a.setflags(write=False)
        _IN[key] = arrays
    return _IN[key]


def reference(case, pattern, affine):
    """RC's float64 reference of the normalised tensor (y, b_y) for a case, computed once and left unchanged."""
    key = (case, pattern, affine)
    if key not in _REF:
        q, k, gamma, beta, W, cbias, go, gy = inputs(*key)
        _REF[key] = RC.reference(case[:6], q, k, gamma, beta, gy)
    return _REF[key]


def run(arrays, G, cuda, offset=False, bias=True, need=(True, True, True, True, True, True), partials=False):
    """Everything the three C calls and the sibling backward give, as a dict of device tensors (not asked for: None)."""
    q, k, gamma, beta, W, cbias, go, _ = arrays
    qd, kd, gd, bd = dev(q, cuda), dev(k, cuda, offset), dev(gamma, cuda), dev(beta, cuda)
    Wd, cbd, god = dev(W, cuda), dev(cbias, cuda) if bias else None, dev(go, cuda, offset)
    out, mean, rstd = _ext.relu_group_norm_conv(qd, kd, gd, bd, G, RC.EPS, Wd, cbd)
    r = dict(out=out, mean=mean, rstd=rstd, gxn=None, gq=None, gk=None, gw=None, gb=None, gcw=None, gcb=None, parts=None)
    if need[4] or need[5]:
        got = _ext.relu_group_norm_conv_grad_weight(qd, kd, gd, bd, mean, rstd, god, G, need[4], need[5],
                                                    return_partials=partials)
        r["gcw"], r["gcb"] = got[0], got[1]
        if partials:
            r["parts"] = got[2].clone()
    if any(need[:4]):
        r["gxn"] = _ext.relu_group_norm_conv_grad_input(Wd, god)
        r["gq"], r["gk"], r["gw"], r["gb"] = _ext.relu_group_norm_grad(qd, kd, gd, bd, mean, rstd, r["gxn"], G, *need[:4])
    torch.cuda.synchronize()
    return r


def host(t):
    return None if t is None else t.detach().cpu().numpy()


CASES = [(c, p, a) for c in CC.cases() for p in CC.PATTERNS for a in (False, True)]
_id = lambda c: "%s-%s-%s" % ("x".join(map(str, c[0])), c[1], "affine" if c[2] else "plain")
GRADS = ("gq", "gk", "gw", "gb", "gcw", "gcb")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_of_the_chains_and_bounds_against_float64(cuda, case):
    shape, pattern, affine = case
    B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = CC.dims(shape)
    arrays = inputs(*case)
    q, k, gamma, beta, W, cbias, go, gy = arrays
    plan = CC.plan(C1, C2, N, K, G, Cout, 1)[1]
    assert plan["family"] == int(K % 4 == 0)
    got = run(arrays, G, cuda)
    # statistics: the sibling op's bits on the same inputs
    _, mean0, rstd0 = _ext.relu_group_norm(dev(q, cuda), dev(k, cuda), dev(gamma, cuda), dev(beta, cuda), G, RC.EPS)
    assert np.array_equal(bits(got["mean"]), bits(mean0)) and np.array_equal(bits(got["rstd"]), bits(rstd0))
    # the forward chain, given the op's statistics
    xn = CC.xn_bits(shape, q, k, gamma, beta, host(got["mean"]), host(got["rstd"]))
    emu = CC.emulate_forward(W, cbias, xn)
    n_exact = CC.same_bits_or_exact(host(got["out"]), emu, W, xn, cbias)
    # the input-gradient chain
    emu_g = CC.emulate_grad_input(W, go)
    n_exact += CC.same_bits_or_exact(host(got["gxn"]), emu_g, np.ascontiguousarray(W.T), go)
    # bounds
    ref = reference(*case)
    out64 = CC.composition64(q, k, gamma, beta, W, cbias, G)["out"]
    r_out = CC.ratio(np.abs(host(got["out"]) - out64), CC.out_bound(shape, ref, W, out64))
    gw64, gwabs, gb64, gbabs = CC.grad_weight_reference(go, xn)
    r_gw = CC.ratio(np.abs(host(got["gcw"]) - gw64), (plan["L"] + 4) * CC.U * gwabs + CC.SUB)
    r_gb = CC.ratio(np.abs(host(got["gcb"]) - gb64), (CC.U + CC.V * (B * S + 2)) * gbabs + CC.SUB)
    print("%s worst ratio to the bound: out %.3g grad_W %.3g grad_bias %.3g; exact-fma elements %d"
          % (_id(case), r_out, r_gw, r_gb, n_exact))
    assert r_out <= 1.0 and r_gw <= 1.0 and r_gb <= 1.0, (r_out, r_gw, r_gb)
    if pattern == "zero_gy":
        for name in GRADS + ("gxn",):
            assert got[name] is None or not host(got[name]).any(), name


SOME = [((2, 33, 34, 7, 4, 32, 40), "normal", True), ((2, 32, 35, 5, 3, 32, 33), "offset", True),
        ((2, 0, 32, 9, 5, 32, 32), "normal", False), (CC.plan_case(), "normal", True)]


@pytest.mark.parametrize("case", SOME, ids=_id)
def test_same_bits_run_after_run_and_with_each_gradient_asked_for_alone(cuda, case):
    shape, pattern, affine = case
    arrays, G = inputs(*case), shape[5]
    first, second = run(arrays, G, cuda), run(arrays, G, cuda)
    for name in ("out", "mean", "rstd", "gxn") + GRADS:
        assert (first[name] is None) == (second[name] is None)
        assert first[name] is None or np.array_equal(bits(first[name]), bits(second[name])), name
    for i, name in enumerate(GRADS):
        if first[name] is None:
            continue
        alone = run(arrays, G, cuda, need=tuple(j == i for j in range(6)))
        assert [n for n in GRADS if alone[n] is not None] == [name]
        assert np.array_equal(bits(alone[name]), bits(first[name])), name
    nobias = run(arrays, G, cuda, bias=False)
    xn = CC.xn_bits(shape, *arrays[:4], host(first["mean"]), host(first["rstd"]))     # bias NULL: the chain itself
    CC.same_bits_or_exact(host(nobias["out"]), CC.chain(arrays[4], xn), arrays[4], xn)


@pytest.mark.parametrize("case", SOME, ids=_id)
def test_a_cloud_of_a_batch_has_the_bits_of_its_own_call_and_the_fold_is_per_cloud_partials_in_order(cuda, case):
    shape, pattern, affine = case
    B = shape[0]
    q, k, gamma, beta, W, cbias, go, gy = inputs(*case)
    batched = run((q, k, gamma, beta, W, cbias, go, gy), shape[5], cuda, partials=True)
    parts = host(batched["parts"]).astype(np.float64)                      # (B, R, Cout, C)
    assert parts.shape[:2] == (B, CC.plan(*shape[1:])[1]["R"])
    fold = np.zeros(parts.shape[2:])
    for b in range(B):
        one = (None if q is None else q[b:b + 1], k[b:b + 1], gamma, beta, W, cbias, go[b:b + 1], None)
        alone = run(one, shape[5], cuda)
        for name in ("out", "mean", "rstd", "gxn", "gq", "gk"):
            if batched[name] is not None:
                assert np.array_equal(bits(batched[name])[b:b + 1], bits(alone[name])), (name, b)
        mine = np.zeros(parts.shape[2:])
        for r in range(parts.shape[1]):                                    # ascending (b, range), in double
            mine = mine + parts[b, r]
            fold = fold + parts[b, r]
        assert np.array_equal(bits(alone["gcw"]), bits(mine.astype(np.float32))), b
    assert np.array_equal(bits(batched["gcw"]), bits(fold.astype(np.float32)))


@pytest.mark.parametrize("case", [((2, 33, 34, 7, 4, 32, 40), "offset", True), ((1, 40, 24, 6, 8, 32, 96), "nonpos", False),
                                  (CC.plan_case(), "normal", True)], ids=_id)
def test_a_view_four_bytes_into_its_storage_takes_the_scalar_family_and_meets_the_same_bits(cuda, case):
    shape, pattern, affine = case
    B, C1, C2, N, K, G, Cout = shape
    assert CC.plan(C1, C2, N, K, G, Cout, 1)[1]["family"] == 1 and CC.plan(C1, C2, N, K, G, Cout, 0)[1]["family"] == 0
    arrays = inputs(*case)
    q, k, gamma, beta, W, cbias, go, gy = arrays
    got, vec = run(arrays, G, cuda, offset=True), run(arrays, G, cuda)
    # the statistics' summation order is the family's: the chains are judged given each run's own statistics
    xn = CC.xn_bits(shape, q, k, gamma, beta, host(got["mean"]), host(got["rstd"]))
    CC.same_bits_or_exact(host(got["out"]), CC.emulate_forward(W, cbias, xn), W, xn, cbias)
    assert np.array_equal(bits(got["gxn"]), bits(vec["gxn"]))              # no statistics in it: the same bits
    if np.array_equal(bits(got["mean"]), bits(vec["mean"])) and np.array_equal(bits(got["rstd"]), bits(vec["rstd"])):
        assert np.array_equal(bits(got["out"]), bits(vec["out"]))
    gw64, gwabs, gb64, gbabs = CC.grad_weight_reference(go, xn)
    L = CC.plan(C1, C2, N, K, G, Cout, 0)[1]["L"]
    assert CC.ratio(np.abs(host(got["gcw"]) - gw64), (L + 4) * CC.U * gwabs + CC.SUB) <= 1.0
    assert np.array_equal(bits(got["gcb"]), bits(vec["gcb"]))


def test_a_nan_in_k_reaches_the_outputs_the_composition_s_nan_reaches(cuda):
    shape = (2, 33, 34, 7, 4, 32, 40)
    B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = CC.dims(shape)
    q, k, gamma, beta, W, cbias, go, gy = (None if a is None else a.copy() for a in inputs(shape, "normal", True))
    k[1, C2 - 1, 4, 1] = np.nan                         # the last channel of cloud 1, a pass-through one: one position
    k[0, 5, 0, 0] = -np.nan                             # a normalised channel of cloud 0: its group, every position
    want = CC.composition64(q, k, gamma, beta, W, cbias, G)["out"]
    out = host(run((q, k, gamma, beta, W, cbias, go, gy), G, cuda)["out"])
    assert np.array_equal(np.isnan(out), np.isnan(want))
    assert np.isnan(out[0]).all() and np.isnan(out[1]).sum() == Cout and np.isnan(out[1, :, 4, 1]).all()


def test_current_stream_and_graph_capture_of_forward_and_backward(cuda):
    """Every call launches on torch's current stream without a hidden synchronisation: captured on a side stream (a
    linear sequence, no parallel branches), the graph replays with changed inputs and gives the eager call's bits."""
    shape = (2, 33, 34, 7, 4, 32, 40)
    first, second = inputs(shape, "normal", True), inputs(shape, "offset", True)
    qd, kd, gd, bd, Wd, cbd, god = (dev(a, cuda) for a in first[:7])

    def step():
        out, mean, rstd = _ext.relu_group_norm_conv(qd, kd, gd, bd, 32, RC.EPS, Wd, cbd)
        gcw, gcb = _ext.relu_group_norm_conv_grad_weight(qd, kd, gd, bd, mean, rstd, god, 32)
        gxn = _ext.relu_group_norm_conv_grad_input(Wd, god)
        gq, gk, gw, gb = _ext.relu_group_norm_grad(qd, kd, gd, bd, mean, rstd, gxn, 32)
        return dict(out=out, mean=mean, rstd=rstd, gxn=gxn, gq=gq, gk=gk, gw=gw, gb=gb, gcw=gcw, gcb=gcb)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                            # warm the allocator outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            held = step()
    torch.cuda.current_stream().wait_stream(side)
    for arrays in (first, second):
        for t, a in zip((qd, kd, gd, bd, Wd, cbd, god), arrays[:7]):
            t.copy_(torch.tensor(np.asarray(a)))
        for t in held.values():
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(arrays, 32, cuda)
        for name, t in held.items():
            assert np.array_equal(bits(t), bits(eager[name])), name


def test_public_function_under_autograd(cuda):
    """pointnet2_utils.relu_group_norm_conv: the C-level bits; what it saves; needs_input_grad subsets; a Conv2d-shaped
    weight; no conv bias; q=None."""
    shape = (2, 33, 34, 7, 4, 32, 40)
    B, C1, C2, N, K, G, Cout = shape
    arrays = inputs(shape, "normal", True)
    q, k, gamma, beta, W, cbias, go, gy = arrays
    want = run(arrays, G, cuda)
    leaf = lambda a: dev(a, cuda).requires_grad_()
    qd, kd, gd, bd, Wd, cbd = leaf(q), leaf(k), leaf(gamma), leaf(beta), leaf(W.reshape(Cout, C1 + C2, 1, 1)), leaf(cbias)
    out = pointnet2_utils.relu_group_norm_conv(kd, gd, bd, G, RC.EPS, Wd, cbd, q=qd)
    assert tuple(out.shape) == (B, Cout, N, K) and type(out.grad_fn).__name__ == "ReluGroupNormConvBackward"
    saved = sorted(tuple(t.shape) for t in out.grad_fn.saved_tensors)
    assert saved == sorted([(B, C1, N), (B, C2, N, K), (B, G), (B, G), (64,), (64,), (Cout, C1 + C2)])   # never xn
    grads = torch.autograd.grad(out, (qd, kd, gd, bd, Wd, cbd), dev(go, cuda))
    assert tuple(grads[4].shape) == (Cout, C1 + C2, 1, 1)
    for name, t in zip(("out",) + GRADS, (out,) + grads):
        assert np.array_equal(bits(t).ravel(), bits(want[name]).ravel()), name
    for wanted in (("gq",), ("gcw",), ("gk", "gb"), ("gcb", "gw")):
        ts = dict(gq=dev(q, cuda), gk=dev(k, cuda), gw=dev(gamma, cuda), gb=dev(beta, cuda), gcw=dev(W, cuda),
                  gcb=dev(cbias, cuda))
        for name in wanted:
            ts[name].requires_grad_()
        o = pointnet2_utils.relu_group_norm_conv(ts["gk"], ts["gw"], ts["gb"], G, RC.EPS, ts["gcw"], ts["gcb"], q=ts["gq"])
        got = torch.autograd.grad(o, [ts[name] for name in wanted], dev(go, cuda))
        for name, t in zip(wanted, got):
            assert np.array_equal(bits(t), bits(want[name])), (wanted, name)
    # q=None, no norm parameters, no conv bias
    shape0 = (2, 0, 32, 9, 5, 32, 32)
    a0 = inputs(shape0, "normal", False)
    want0 = run(a0, 32, cuda, bias=False)
    k0, W0 = leaf(a0[1]), leaf(a0[4])
    o0 = pointnet2_utils.relu_group_norm_conv(k0, None, None, 32, RC.EPS, W0, None)
    g0 = torch.autograd.grad(o0, (k0, W0), dev(a0[6], cuda))
    for name, t in zip(("out", "gk", "gcw"), (o0,) + g0):
        assert np.array_equal(bits(t), bits(want0[name])), name


# ---- the module path -------------------------------------------------------------------------------------------------
def with_switches(fn, conv, norm=False):
    prev_c, prev_n = _ext.set_fused_score_conv(conv), _ext.set_fused_score_norm(norm)
    try:
        return fn()
    finally:
        _ext.set_fused_score_conv(prev_c)
        _ext.set_fused_score_norm(prev_n)


@pytest.mark.parametrize("count", ["tensor", "all"])
def test_attention_module_switch_on_against_switch_off_and_float64(cuda, count):
    """AttentionModule(8, 35, 8, 35, 64) at B = 2, N = 12, K = 8 against the same module in float64 on the CPU, the seeds
    of tests/test_relu_group_norm_gpu.py: the output and every parameter and input gradient under its 4 x rule."""
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
    fn = lambda: evaluate(mod32, [on_dev(t) for t in (feat, gf, gfo, cnt)], r.to(cuda))
    off, on = with_switches(fn, False), with_switches(fn, True)
    names = ["out"] + [n for n, _ in mod64.named_parameters()] + ["feat", "grouped_feat", "grouped_feat_out"]
    assert len(names) == len(want) == len(on)
    judge("attention-conv-" + count, names, want, off, on)


def test_the_score_head_s_graph_with_the_switch_on_and_off(cuda):
    torch.manual_seed(33)
    mod = AttentionModule(8, 35, 8, 35, 64).to(cuda)
    keys = sorted(mod.state_dict())
    feat = torch.randn(2, 8, 12, device=cuda, requires_grad=True)
    gf = torch.randn(2, 35, 12, 8, device=cuda, requires_grad=True)

    def names():
        scores = mod.score_head(feat, gf)                  # kept alive: a custom Function's node lives with its output
        assert tuple(scores.shape) == (2, 64, 12, 8)
        return node_names(scores)

    off = with_switches(names, False)
    for norm in (False, True):
        on = with_switches(names, True, norm)
        assert sum(n == "ReluGroupNormConvBackward" for n in on) == 2, on
        assert not any(n == "ReluGroupNormBackward" for n in on), on
        # feat_conv and grouped_feat_conv remain: the two convolutions in front of the head, none behind a norm
        assert sum("ConvolutionBackward" in n for n in on) == 2 and sum("ConvolutionBackward" in n for n in off) == 4
        assert not any("Cat" in n or "Expand" in n or n.startswith("Relu") and "GroupNorm" not in n for n in on), on
    assert not any("ReluGroupNorm" in n for n in off)
    assert sum("ReluBackward" in n for n in off) == 2 and sum("NativeGroupNormBackward" in n for n in off) == 2
    assert any("ExpandBackward" in n for n in off) and sum("CatBackward" in n for n in off) == 2, off
    assert sorted(mod.state_dict()) == keys
    # an attention_bn=False head has no norm: the composition, whatever the switch says
    plain = AttentionModule(8, 35, 8, 35, 64, attention_bn=False).to(cuda)
    p_off = with_switches(lambda: node_names(plain.score_head(feat, gf)), False)
    p_on = with_switches(lambda: node_names(plain.score_head(feat, gf)), True)
    assert sorted(p_off) == sorted(p_on) and not any("ReluGroupNorm" in n for n in p_on)


def test_autograd_holds_neither_the_cat_nor_the_normalised_tensor(cuda):
    """(2, 32, 35, 64, 8), Cout = 64: the bytes alive between forward and backward grow by less than out + k + one
    (B, C, N, K) tensor with the op; the composition's growth is above that."""
    B, C1, C2, N, K, Cout, G = 2, 32, 35, 64, 8, 64, 32
    C = C1 + C2
    gen = torch.Generator().manual_seed(7)
    leaf = lambda *s: torch.randn(*s, generator=gen).to(cuda).requires_grad_()
    q, k, W, cb = leaf(B, C1, N), leaf(B, C2, N, K), leaf(Cout, C), leaf(Cout)
    gamma, beta = leaf(64), leaf(64)
    limit = 4 * (B * Cout * N * K + B * C2 * N * K + B * C * N * K)

    def grown(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(cuda)
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated(cuda) - before, out

    fused, out_f = grown(lambda: pointnet2_utils.relu_group_norm_conv(k, gamma, beta, G, RC.EPS, W, cb, q=q))

    def composed():
        x = torch.cat([q.unsqueeze(-1).expand(-1, -1, -1, K), k], dim=1)
        return torch.nn.functional.conv2d(RC.composition(None, x, gamma, beta, G, RC.EPS), W[:, :, None, None], cb)

    plain, out_p = grown(composed)
    print("bytes held between forward and backward: op %d, composition %d, limit %d" % (fused, plain, limit))
    assert fused < limit < plain
    assert float((out_f - out_p).detach().abs().max()) < 1e-4
