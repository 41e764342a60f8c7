"""Matrix-free EMD gradient (pdr_emd_cost_grad[_ragged] through pointnet2/emd.py) on the GPU.

Ground truth and bar.  The bar of the EMD gradient kernels is rtol 1e-3 / atol 1e-5 against the CPU oracle's
matchcost_grad on a given match (test_emd_vs_oracle, test_matchcost_and_its_gradients_on_a_given_padded_match).  The
truth here is O.matchcost_grad(g, a, b, match) with match = approxmatch_forward(a, b): the oracle applied to the matrix
the unchanged GPU forward writes from the very factors the matrix-free kernel reads.  The same bar is asserted against
the default path's gradients, matchcost_backward on that matrix.  The kernel evaluates every entry by
emd_match_kernel's expression, so what is left between the two is the order of one float32 sum per row; on the CPU the
oracle against a float64 closed sum and against a float32 sum in reversed order stays below 1 % of the bar at (17, 5),
(300, 1100), (1100, 300) and 1000^2.

Inputs are uniform in [-0.5, 0.5], grad_cost uniform in [0.5, 1.5].  Each case's truth is computed once and shared.

Dense shapes (n, m), B = 2 (B = 3 for the reference's 2-point known-answer pair):
  the issue's       (2, 2) known answer, (1, 1), (17, 5), (64, 64), (300, 1100), (1100, 300), (1025, 257), (2048, 2048)
  kernel boundaries emd_cost_grad_kernel gives one thread per own point in workgroups of 256 (4 waves of 64) and streams
                    the opposite cloud in LDS tiles of 256 points; both sides run it, so n and m each cross both:
                    (63, 65), (65, 63)        one wave partly filled / one lane into the second wave
                    (255, 257), (257, 255)    last lane of a workgroup and of a tile missing / one row into the second
                                              workgroup and one point into the second tile
                    (256, 512), (512, 256)    exactly one and exactly two workgroups / tiles
                    (513, 767)                a third workgroup of one row, a third tile one short of full
Lengths: the three cases of tests/test_ragged_emd_gpu.py (padded 300 x 1100 and 1100 x 300; lengths around 16, 256 and
1024, clamped, empty pairs), padding NaN in one variant and +-50 in the other.
"""
import numpy as np
import pytest
import torch

from oracle import pdr_oracle as O
from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2 import emd
from tests.test_ragged_emd_gpu import CASES, FILLS, dev, host, lengths_on, padded, pair_sizes, same_bits

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-3, 1e-5
KAT = (2, 2)
DENSE = [KAT, (1, 1), (17, 5), (64, 64), (300, 1100), (1100, 300), (1025, 257), (2048, 2048),
         (63, 65), (65, 63), (255, 257), (257, 255), (256, 512), (512, 256), (513, 767)]


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want)
    print("%s: max abs err %.3g, max err / (atol + rtol |want|) %.3g"
          % (what, err.max(initial=0), (err / (ATOL + RTOL * np.abs(want))).max(initial=0)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def clouds(n, m):
    if (n, m) == KAT:                                        # PytorchEMD/test_emd_loss.py:7-23
        a = np.array([[[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]]], dtype=np.float32).repeat(3, 0)
        b = np.array([[[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]]], dtype=np.float32).repeat(3, 0)
    else:
        rr = np.random.default_rng(7 * n + m)
        a = rr.uniform(-0.5, 0.5, (2, n, 3)).astype(np.float32)
        b = rr.uniform(-0.5, 0.5, (2, m, 3)).astype(np.float32)
    g = np.random.default_rng(n + m).uniform(0.5, 1.5, a.shape[0]).astype(np.float32)
    return a, b, g


@pytest.fixture(scope="module")
def dense_truth(cuda):
    """(n, m) -> clouds on the device, the oracle's gradients on the GPU forward's match and the default path's."""
    cache = {}

    def get(n, m):
        if (n, m) not in cache:
            a, b, g = clouds(n, m)
            at, bt, gt = dev(a, cuda), dev(b, cuda), dev(g, cuda)
            match = emd.approxmatch_forward(at, bt)
            o1, o2 = O.matchcost_grad(g, a, b, host(match))
            d1, d2 = emd.matchcost_backward(gt, at, bt, match)
            cache[(n, m)] = dict(a=at, b=bt, g=gt, o1=o1, o2=o2, d1=host(d1), d2=host(d2), np=(a, b, g))
        return cache[(n, m)]
    return get


@pytest.mark.parametrize("n,m", DENSE)
def test_dense_gradients_against_the_oracle_and_the_default_path(cuda, dense_truth, n, m):
    t = dense_truth(n, m)
    cost, ws = emd.emd_cost_fused(t["a"], t["b"], return_workspace=True)
    assert torch.equal(cost, emd.emd_cost_fused(t["a"], t["b"]))
    assert ws.dtype == torch.float32 and ws.numel() * 4 == _lib.load().pdr_emd_workspace_bytes(t["a"].shape[0], n, m)
    kept = ws.clone()
    g1, g2 = emd.emd_cost_backward(t["g"], t["a"], t["b"], ws)
    assert torch.equal(ws, kept), "the workspace is read only"
    assert g1.shape == t["a"].shape and g2.shape == t["b"].shape
    close(host(g1), t["o1"], "grad1 vs oracle")
    close(host(g2), t["o2"], "grad2 vs oracle")
    close(host(g1), t["d1"], "grad1 vs matchcost_backward")
    close(host(g2), t["d2"], "grad2 vs matchcost_backward")
    # grad1 is matchcost_grad1_kernel's operation sequence on the entries emd_match_kernel's expression gives: the
    # bits of the default path (grad2 sums in index order where matchcost_grad2_kernel sums by lanes: the bar above)
    assert same_bits(host(g1), t["d1"]), "grad1 differs from matchcost_backward on the forward's match"
    # the same input gives the same bits, from the same workspace and from a second forward
    r1, r2 = emd.emd_cost_backward(t["g"], t["a"], t["b"], ws)
    s1, s2 = emd.emd_cost_backward(t["g"], t["a"], t["b"], emd.emd_cost_fused(t["a"], t["b"], return_workspace=True)[1])
    assert torch.equal(r1, g1) and torch.equal(r2, g2) and torch.equal(s1, g1) and torch.equal(s2, g2)
    if (n, m) == KAT:   # match is the permutation [[0, 1], [1, 0]] to 1e-6: xyz1_k pairs with xyz2_(1-k)
        a, b, g = t["np"]
        close(host(g1), 2 * (a - b[:, ::-1]) * g[:, None, None], "grad1 vs the known answer")
        close(host(g2), 2 * (b - a[:, ::-1]) * g[:, None, None], "grad2 vs the known answer")


def test_the_workspace_of_approxmatch_serves_too(cuda, dense_truth):
    """The C ABI promises the factors after pdr_approxmatch as well: raw calls, one workspace, same gradients."""
    t = dense_truth(300, 1100)
    B, n, m = 2, 300, 1100
    lib = _lib.load()
    ws = torch.empty(lib.pdr_emd_workspace_bytes(B, n, m) // 4, dtype=torch.float32, device=cuda)
    match = torch.empty(B, m, n, dtype=torch.float32, device=cuda)
    g1, g2 = torch.empty_like(t["a"]), torch.empty_like(t["b"])
    s = torch.cuda.current_stream().cuda_stream
    assert lib.pdr_approxmatch(t["a"].data_ptr(), t["b"].data_ptr(), B, n, m, match.data_ptr(), ws.data_ptr(), s) == 0
    assert lib.pdr_emd_cost_grad(t["g"].data_ptr(), t["a"].data_ptr(), t["b"].data_ptr(), ws.data_ptr(), B, n, m,
                                 g1.data_ptr(), g2.data_ptr(), s) == 0
    w1, w2 = emd.emd_cost_backward(t["g"], t["a"], t["b"], emd.emd_cost_fused(t["a"], t["b"], return_workspace=True)[1])
    assert torch.equal(g1, w1) and torch.equal(g2, w2)


# ------------------------------------------------------------------ lengths
@pytest.fixture(scope="module")
def ragged_truth(cuda):
    """Per case: the valid points, grad_cost, and per pair the oracle's gradients on the match the GPU forward gives on
    the slices (None for an empty pair)."""
    out = {}
    for ci, name in enumerate(CASES):
        n, m, l1, l2 = CASES[name]
        rr = np.random.default_rng(300 + ci)
        x = rr.uniform(-0.5, 0.5, (len(l1), n, 3)).astype(np.float32)
        y = rr.uniform(-0.5, 0.5, (len(l1), m, 3)).astype(np.float32)
        g = rr.uniform(0.5, 1.5, len(l1)).astype(np.float32)
        pairs = []
        for b, (a, c) in enumerate(pair_sizes(name)):
            if a == 0:
                pairs.append(None)
                continue
            xs, ys = x[b:b + 1, :a], y[b:b + 1, :c]
            match = host(emd.approxmatch_forward(dev(xs, cuda), dev(ys, cuda)))
            pairs.append(O.matchcost_grad(g[b:b + 1], xs, ys, match))
        out[name] = dict(valid=(x, y), g=g, pairs=pairs)
    return out


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_with_lengths(cuda, ragged_truth, name, fill):
    """Valid rows within the bar of the oracle on the slices and of the default path with lengths; padded rows and
    empty pairs exactly 0 as bits, whatever the padding holds."""
    t = ragged_truth[name]
    x, y = padded(name, fill, t["valid"])
    xt, yt, gt = dev(x, cuda), dev(y, cuda), dev(t["g"], cuda)
    l1, l2 = lengths_on(name, cuda)
    cost, ws = emd.emd_cost_fused(xt, yt, l1, l2, return_workspace=True)
    assert torch.equal(cost, emd.emd_cost_fused(xt, yt, l1, l2))
    g1, g2 = (host(v) for v in emd.emd_cost_backward(gt, xt, yt, ws, l1, l2))
    d1, d2 = (host(v) for v in emd.matchcost_backward(gt, xt, yt, emd.approxmatch_forward(xt, yt, l1, l2), l1, l2))
    n, m = x.shape[1], y.shape[1]
    for b, ((a, c), p) in enumerate(zip(pair_sizes(name), t["pairs"])):
        assert same_bits(g1[b, a:], np.zeros((n - a, 3))) and same_bits(g2[b, c:], np.zeros((m - c, 3))), b
        if p is None:
            assert a == 0 and c == 0
            continue
        close(g1[b, :a], p[0][0], "pair %d (%d, %d) grad1 vs oracle" % (b, a, c))
        close(g2[b, :c], p[1][0], "pair %d (%d, %d) grad2 vs oracle" % (b, a, c))
        close(g1[b, :a], d1[b, :a], "pair %d grad1 vs matchcost_backward" % b)
        close(g2[b, :c], d2[b, :c], "pair %d grad2 vs matchcost_backward" % b)


@pytest.mark.parametrize("n,m", [(300, 1100), (1100, 300)])
def test_full_or_absent_lengths_equal_the_dense_call(cuda, dense_truth, n, m):
    t = dense_truth(n, m)
    B = t["a"].shape[0]
    f1 = torch.full((B,), n, dtype=torch.int64, device=cuda)
    f2 = torch.full((B,), m, dtype=torch.int64, device=cuda)
    cost, ws = emd.emd_cost_fused(t["a"], t["b"], return_workspace=True)
    d1, d2 = emd.emd_cost_backward(t["g"], t["a"], t["b"], ws)
    for la, lb in ((f1, f2), (f1, None), (None, f2), (None, None), (f1 + 5, f2 + 5), (f1.int(), f2.int())):
        c, w = emd.emd_cost_fused(t["a"], t["b"], la, lb, return_workspace=True)
        r1, r2 = emd.emd_cost_backward(t["g"], t["a"], t["b"], w, la, lb)
        assert torch.equal(c, cost) and torch.equal(r1, d1) and torch.equal(r2, d2)


# ------------------------------------------------------------------ autograd
def _leaves(t):
    return t["a"].clone().requires_grad_(True), t["b"].clone().requires_grad_(True)


@pytest.mark.parametrize("module", [False, True])
def test_autograd_matrix_free(cuda, dense_truth, module):
    """The cost is the one of the call without a gradient, bit for bit; the gradients are within the bar of the
    default differentiable path's (both pass grad_cost through undivided); two runs give the same bits."""
    t = dense_truth(300, 1100)
    fn = (lambda *a, **k: emd.EMD_distance()(*a, **k)) if module else emd.earth_mover_distance
    a, b = _leaves(t)
    cost = fn(a, b, matrix_free=True)
    assert cost.requires_grad and torch.equal(cost.detach(), emd.earth_mover_distance(a.detach(), b.detach()))
    (cost * t["g"]).sum().backward()
    a0, b0 = _leaves(t)
    (emd.earth_mover_distance(a0, b0) * t["g"]).sum().backward()
    close(host(a.grad), host(a0.grad), "xyz1.grad vs the default path")
    close(host(b.grad), host(b0.grad), "xyz2.grad vs the default path")
    close(host(a.grad), t["o1"], "xyz1.grad vs oracle")
    close(host(b.grad), t["o2"], "xyz2.grad vs oracle")
    a2, b2 = _leaves(t)
    (fn(a2, b2, matrix_free=True) * t["g"]).sum().backward()
    assert torch.equal(a2.grad, a.grad) and torch.equal(b2.grad, b.grad)
    # the transposed layout of the reference's signature, and a cloud that needs no gradient
    a3 = t["a"].transpose(1, 2).clone().requires_grad_(True)
    c3 = fn(a3, t["b"].transpose(1, 2), True, matrix_free=True)
    assert torch.equal(c3.detach(), cost.detach())
    (c3 * t["g"]).sum().backward()
    assert torch.equal(a3.grad.transpose(1, 2), a.grad)


@pytest.mark.parametrize("module", [False, True])
@pytest.mark.parametrize("name", ["grad2_grid", "swapped"])
def test_autograd_matrix_free_with_lengths(cuda, ragged_truth, name, module):
    t = ragged_truth[name]
    x, y = padded(name, "nan", t["valid"])
    l1, l2 = lengths_on(name, cuda)
    fn = (lambda *a, **k: emd.EMD_distance()(*a, **k)) if module else emd.earth_mover_distance
    xt, yt = dev(x, cuda).requires_grad_(True), dev(y, cuda).requires_grad_(True)
    cost = fn(xt, yt, lengths1=l1, lengths2=l2, matrix_free=True)
    assert cost.requires_grad
    assert torch.equal(cost.detach(), emd.earth_mover_distance(xt.detach(), yt.detach(), lengths1=l1, lengths2=l2))
    cost.sum().backward()
    x0, y0 = dev(x, cuda).requires_grad_(True), dev(y, cuda).requires_grad_(True)
    emd.earth_mover_distance(x0, y0, lengths1=l1, lengths2=l2).sum().backward()
    g1, g2, d1, d2 = (host(v.grad) for v in (xt, yt, x0, y0))
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    for b, (a, c) in enumerate(pair_sizes(name)):
        assert same_bits(g1[b, a:], np.zeros_like(g1[b, a:])) and same_bits(g2[b, c:], np.zeros_like(g2[b, c:])), b
        if a:
            assert g1[b, :a].any(-1).all() and g2[b, :c].any(-1).all(), "pair %d: a valid row without a gradient" % b
            close(g1[b, :a], d1[b, :a], "pair %d xyz1.grad vs the default path" % b)
            close(g2[b, :c], d2[b, :c], "pair %d xyz2.grad vs the default path" % b)


def test_the_saved_workspace_is_per_call(cuda, dense_truth):
    """Two forwards on different inputs, then the two backwards: each gives what it gives alone."""
    ta, tb = dense_truth(300, 1100), dense_truth(1100, 300)
    alone = []
    for t in (ta, tb):
        a, b = _leaves(t)
        (emd.earth_mover_distance(a, b, matrix_free=True) * t["g"]).sum().backward()
        alone.append((a.grad, b.grad))
    a1, b1 = _leaves(ta)
    a2, b2 = _leaves(tb)
    c1 = emd.earth_mover_distance(a1, b1, matrix_free=True)
    c2 = emd.earth_mover_distance(a2, b2, matrix_free=True)
    (c1 * ta["g"]).sum().backward()
    (c2 * tb["g"]).sum().backward()
    for got, want in zip((a1, b1, a2, b2), alone[0] + alone[1]):
        assert torch.equal(got.grad, want)


# ------------------------------------------------------------------ memory
def test_no_match_sized_tensor_is_allocated(cuda, dense_truth):
    """B = 2, 2048^2: the match would be 33.5 MB, the workspace is 0.38 MB.  Peak growth over forward + backward below
    an eighth of the matrix with matrix_free=True; at least the matrix on the default path (the test discriminates)."""
    t = dense_truth(2048, 2048)
    matrix = 4 * 2 * 2048 * 2048

    def growth(**kw):
        a, b = _leaves(t)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(cuda)
        before = torch.cuda.memory_allocated(cuda)
        emd.earth_mover_distance(a, b, **kw).sum().backward()
        torch.cuda.synchronize()
        assert a.grad is not None and b.grad is not None
        return torch.cuda.max_memory_allocated(cuda) - before

    free, default = growth(matrix_free=True), growth()
    print("peak growth: matrix_free %d B, default %d B, matrix %d B" % (free, default, matrix))
    assert free < matrix // 8
    assert default >= matrix


# ------------------------------------------------------------------ capture
def test_captured_forward_and_backward_follow_data_overwritten_before_replay(cuda, ragged_truth):
    """emd_cost_fused(return_workspace=True) + emd_cost_backward with lengths captured on a side stream after two
    warm-up calls; clouds, grad_cost and lengths are overwritten in place and the graph replayed: the result is the
    eager call's on the new data."""
    first, second = ragged_truth["grad2_grid"], ragged_truth["tile_edges"]
    x, y = padded("grad2_grid", "big", first["valid"])
    xt, yt, gt = dev(x, cuda), dev(y, cuda), dev(first["g"], cuda)
    t1, t2 = lengths_on("grad2_grid", cuda)

    def run():
        cost, ws = emd.emd_cost_fused(xt, yt, t1, t2, return_workspace=True)
        return (cost, *emd.emd_cost_backward(gt, xt, yt, ws, t1, t2))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
        run()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = run()
    torch.cuda.current_stream().wait_stream(s)
    for name, t, fill in (("grad2_grid", first, "big"), ("tile_edges", second, "nan")):
        nx, ny = padded(name, fill, t["valid"])
        xt.copy_(dev(nx, cuda)), yt.copy_(dev(ny, cuda)), gt.copy_(dev(t["g"], cuda))
        n1, n2 = lengths_on(name, cuda)
        t1.copy_(n1), t2.copy_(n2)
        g.replay()
        torch.cuda.synchronize()
        xe, ye, ge = dev(nx, cuda), dev(ny, cuda), dev(t["g"], cuda)
        cost, ws = emd.emd_cost_fused(xe, ye, n1, n2, return_workspace=True)
        want = (cost, *emd.emd_cost_backward(ge, xe, ye, ws, n1, n2))
        for got, w in zip(out, want):
            assert torch.equal(got, w) and bool(torch.isfinite(got).all())
    assert same_bits(host(out[1])[:2], np.zeros((2, 300, 3)))           # tile_edges: pairs 0 and 1 are empty
