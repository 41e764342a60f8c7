"""Length-aware kNN / Chamfer (pytorch3d lengths1 / lengths2) on the GPU: pdr_knn_points_ragged and
pdr_chamfer_nn_ragged through `_ext` and `chamfer_distance`.

Ground truth is the CPU oracle's knn on the SLICED clouds, cloud by cloud, placed into outputs pre-filled by the padding
rule; distances must be bit-equal and indices equal.  The padded rows of the searched cloud hold copies of that cloud's
valid query points, so a candidate taken from the padding shows up as distance 0 at an index >= the length; the padded
query rows hold finite garbage.

Which kernel a case runs (the dispatch of pdr_knn_points, a function of the PADDED n2 and K):
  K = 1 without nn      nn1_kernel (n2 = 130: one LDS tile, 1100: two); with nn: nn_search_kernel<1>
  K <= 8, 64 <= n2 <= 1024   knn_wave_kernel: n2 = 64 one chunk (a cloud shorter than 57 points leaves a lane group
                        empty: every slot becomes a rank-path candidate), 130 a partial third chunk, 1000 sixteen
                        chunks with a partial last one; n1 = 13200 makes a wave walk 16 queries
  K <= 8, n2 = 1100     nn_search_kernel<4 / 8>, two LDS tiles
  K = 16 / 32, n2 = 300 nn_search_kernel<16 / 32>
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pdr_oracle as O
from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import chamfer_distance
from point_diffusion_refinement_amd.pointnet2_ops import _ext

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def length_sets(n1, n2, K):
    """Two batches of B = 5 that together take lengths2 through {0, 1, K-1, K, 63, 64, 65, n2-1, n2} (beyond n2: the
    kernel's clamp) next to valid queries, and lengths1 through {0, 1, n1-1, n1}."""
    return [([n1, n1 - 1, n1, 1, n1], [0, 1, K - 1, K, 63]),
            ([n1, 1, n1 - 1, n1, 0], [64, 65, n2 - 1, n2, 63])]


def make_clouds(seed, n1, n2, l1, l2, both_ways=False):
    """x (B,n1,3), y (B,n2,3): y's padded rows are copies of the cloud's valid queries; x's padded rows are garbage, or
    (both_ways: x is searched too) copies of y's valid points."""
    rr = np.random.default_rng(seed)
    B = len(l1)
    x = rr.uniform(-1, 1, (B, n1, 3)).astype(np.float32)
    y = rr.uniform(-1, 1, (B, n2, 3)).astype(np.float32)
    for b in range(B):
        a, c = min(l1[b], n1), min(l2[b], n2)
        vx, vy = x[b, :a].copy(), y[b, :c].copy()
        if a > 0 and c < n2:
            y[b, c:] = vx[np.arange(n2 - c) % a]
        if both_ways and c > 0 and a < n1:
            x[b, a:] = vy[np.arange(n1 - a) % c]
        elif a < n1:
            x[b, a:] = rr.uniform(-50, 50, (n1 - a, 3)).astype(np.float32)
    return x, y


def sliced_knn(x, y, l1, l2, K):
    """The oracle on x[b, :l1[b]] / y[b, :l2[b]] in outputs pre-filled with the padding rule (0, -1)."""
    B, n1, n2 = x.shape[0], x.shape[1], y.shape[1]
    d = np.zeros((B, n1, K), np.float32)
    i = np.full((B, n1, K), -1, np.int64)
    for b in range(B):
        a, c = min(l1[b], n1), min(l2[b], n2)
        if a > 0:
            d[b, :a], i[b, :a] = (o[0] for o in O.knn(x[b:b + 1, :a], y[b:b + 1, :c], K))
    return d, i


def gathered(y, i):
    nn = np.take_along_axis(y[:, None], np.maximum(i, 0)[..., None], 2)
    nn[i < 0] = 0
    return nn


def check_knn(cuda, x, y, l1, l2, K):
    od, oi = sliced_knn(x, y, l1, l2, K)
    xt, yt = dev(x, cuda), dev(y, cuda)
    t1, t2 = dev(np.asarray(l1, np.int64), cuda), dev(np.asarray(l2, np.int64), cuda)
    for return_nn in (False, True):
        d, i, nn = _ext.knn_points(xt, yt, K, return_nn=return_nn, lengths1=t1, lengths2=t2)
        assert np.array_equal(host(i), oi), "indices, return_nn=%s" % return_nn
        assert np.array_equal(host(d).view(np.uint32), od.view(np.uint32)), "distances, return_nn=%s" % return_nn
        if return_nn:
            assert np.array_equal(host(nn), gathered(y, oi))


CASES = ([(K, n2, n1) for K in (1, 3, 8) for n2 in (130, 1100) for n1 in (1, 257)]
         + [(K, 300, n1) for K in (16, 32) for n1 in (1, 257)]
         + [(3, 64, 257), (8, 64, 257), (8, 1000, 257)])


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("K,n2,n1", CASES)
def test_knn_points_with_lengths_is_the_oracle_on_the_slices(cuda, K, n2, n1, which):
    l1, l2 = length_sets(n1, n2, K)[which]
    x, y = make_clouds(1000 * K + n2 + n1 + which, n1, n2, l1, l2)
    check_knn(cuda, x, y, l1, l2, K)


def test_knn_wave_kernel_walks_padded_queries_inside_a_wave(cuda):
    """13200 queries per cloud: the wave-per-query kernel gives every wave 16 consecutive queries, so the lengths cut
    through a wave's own range (valid queries first, padded ones after them)."""
    n1, n2, K = 13200, 130, 3
    l1, l2 = [n1, n1 - 1, 1, 0, 7777], [130, 65, 2, 129, 64]
    x, y = make_clouds(77, n1, n2, l1, l2)
    check_knn(cuda, x, y, l1, l2, K)


@pytest.mark.parametrize("n2,K", [(100, 8), (700, 5)])
def test_knn_with_lengths_through_exact_ties(cuda, n2, K):
    """The inputs of test_knn_wave_kernel_ties_and_partial_chunks (integer lattice, a cloud of identical points,
    duplicated points) with lengths2 cutting through the tied block: with `same`, every point of the cloud is tied
    (more than 64 candidates -> the exact extraction) and the padded rows are tied with them too."""
    rr = np.random.default_rng(900 + n2 + K)
    B = 5
    lattice = rr.integers(-3, 4, (B, n2, 3)).astype(np.float32)
    same = np.broadcast_to(np.array([0.25, -0.5, 0.125], np.float32), (B, n2, 3)).copy()
    dup = rr.uniform(-1, 1, (B, n2, 3)).astype(np.float32)
    dup[:, n2 // 2:] = dup[:, : n2 - n2 // 2]
    l1 = [100, 99, 41, 100, 0]
    l2 = [n2 - 1, 70, 65, K - 1, n2 // 2 + 3]
    for y in (lattice, same, dup):
        x = np.concatenate([y[:, :40], rr.integers(-3, 4, (B, 60, 3)).astype(np.float32)], 1)
        check_knn(cuda, x, y, l1, l2, K)


@pytest.mark.parametrize("K,n2", [(1, 130), (1, 1100), (3, 64), (8, 130), (8, 1000), (8, 1100), (16, 300), (32, 300)])
def test_full_or_absent_lengths_equal_the_dense_search(cuda, K, n2):
    B, n1 = 3, 257
    rr = np.random.default_rng(K + n2)
    x = dev(rr.uniform(-1, 1, (B, n1, 3)).astype(np.float32), cuda)
    y = dev(rr.uniform(-1, 1, (B, n2, 3)).astype(np.float32), cuda)
    f1 = torch.full((B,), n1, dtype=torch.int64, device=cuda)
    f2 = torch.full((B,), n2, dtype=torch.int64, device=cuda)
    for return_nn in (False, True):
        want = _ext.knn_points(x, y, K, return_nn=return_nn)
        for la, lb in ((f1, f2), (f1, None), (None, f2), (None, None), (f1 + 5, f2 + 5)):
            got = _ext.knn_points(x, y, K, return_nn=return_nn, lengths1=la, lengths2=lb)
            assert all(torch.equal(g, w) for g, w in zip(got[:2 + return_nn], want[:2 + return_nn]))
    if K == 1:
        want = _ext.chamfer_nn(x, y)
        for la, lb in ((f1, f2), (f1, None), (None, f2), (None, None)):
            assert all(torch.equal(g, w) for g, w in zip(_ext.chamfer_nn(x, y, la, lb), want))


def test_lengths_are_validated_like_the_other_arguments(cuda):
    x, y = torch.rand(2, 64, 3, device=cuda), torch.rand(2, 70, 3, device=cuda)
    ok = torch.full((2,), 64, dtype=torch.int64, device=cuda)
    for bad in (ok.int(), ok.cpu(), ok[:1], ok[:, None].expand(2, 2), torch.stack([ok, ok], 1)[:, 0]):
        with pytest.raises(RuntimeError):
            _ext.knn_points(x, y, 3, lengths1=bad)
        with pytest.raises(RuntimeError):
            _ext.knn_points(x, y, 3, lengths2=bad)
        with pytest.raises(RuntimeError):
            _ext.chamfer_nn(x, y, bad, None)
        with pytest.raises(RuntimeError):
            _ext.chamfer_nn(x, y, None, bad)


# ------------------------------------------------------------------ Chamfer
CH_N1, CH_N2 = 300, 1100
CH_L1 = [0, 1, 299, 300, 150]
CH_L2 = [1100, 0, 1099, 1, 1025]


@pytest.fixture(scope="module")
def chamfer_case():
    """One ragged batch shared (read-only) by the Chamfer tests: clouds, and the sliced oracle's K = 1 searches in both
    directions with (0, 0) where a query is padded or its opposite cloud is empty."""
    x, y = make_clouds(4242, CH_N1, CH_N2, CH_L1, CH_L2, both_ways=True)
    dxy, ixy = sliced_knn(x, y, CH_L1, CH_L2, 1)
    dyx, iyx = sliced_knn(y, x, CH_L2, CH_L1, 1)
    return x, y, dxy[..., 0], np.maximum(ixy[..., 0], 0), dyx[..., 0], np.maximum(iyx[..., 0], 0)


def lengths_on(cuda):
    return dev(np.asarray(CH_L1, np.int64), cuda), dev(np.asarray(CH_L2, np.int64), cuda)


def test_chamfer_nn_with_lengths(cuda, chamfer_case):
    x, y, dxy, ixy, dyx, iyx = chamfer_case
    xt, yt = dev(x, cuda), dev(y, cuda)
    t1, t2 = lengths_on(cuda)
    gdx, gix, gdy, giy = _ext.chamfer_nn(xt, yt, t1, t2)
    assert np.array_equal(host(gix), ixy) and np.array_equal(host(giy), iyx)
    assert np.array_equal(host(gdx).view(np.uint32), dxy.view(np.uint32))
    assert np.array_equal(host(gdy).view(np.uint32), dyx.view(np.uint32))
    for b in range(len(CH_L1)):
        a, c = CH_L1[b], CH_L2[b]
        assert not host(gdx)[b, a:].any() and not host(gix)[b, a:].any()          # padded entries: 0 / 0
        assert not host(gdy)[b, c:].any() and not host(giy)[b, c:].any()
        if a == 0:
            assert not host(gdy)[b].any() and not host(giy)[b].any()              # empty opposite cloud: 0 / 0
        if c == 0:
            assert not host(gdx)[b].any() and not host(gix)[b].any()
    d1, i1, _ = _ext.knn_points(xt, yt, 1, lengths1=t1, lengths2=t2)
    d2, i2, _ = _ext.knn_points(yt, xt, 1, lengths1=t2, lengths2=t1)
    assert torch.equal(gdx, d1[..., 0]) and torch.equal(gix, i1[..., 0].clamp(min=0))
    assert torch.equal(gdy, d2[..., 0]) and torch.equal(giy, i2[..., 0].clamp(min=0))


def _cosine_term(cuda, n_own, n_other, idx, lengths):
    """1 - |cos| between every point's normal and its neighbour's (the ORACLE's indices), 0 on padded points: float32
    with the module's torch op on the device, so only the summation order of the reductions is left to differ."""
    near = np.take_along_axis(n_other, idx[..., None], 1)
    t = host(1 - torch.abs(F.cosine_similarity(dev(n_own, cuda), dev(near, cuda), dim=2, eps=1e-6)))
    t[np.arange(t.shape[1])[None] >= np.asarray(lengths)[:, None]] = 0
    return t


@pytest.mark.parametrize("batch_reduction,point_reduction,weighted,normals",
                         [(None, None, False, False), (None, None, True, False), ("mean", "mean", False, False),
                          ("mean", "mean", True, True), ("sum", "sum", False, False)])
def test_chamfer_distance_with_lengths(cuda, chamfer_case, batch_reduction, point_reduction, weighted, normals):
    """chamfer_distance(x, y, x_lengths, y_lengths, ...) against the same reductions of the sliced oracle searches: the
    unreduced distance maps exactly, the reduced sums to rtol 1e-6 of their float64 value (torch owns the fp32
    summation order).  The cosine term (reduced only: the module adds an (N,P1) and an (N,P2) map) is held to the
    same rtol 1e-6: its per-point map is evaluated from the oracle's indices with the module's own torch op on the
    device (_cosine_term).  The reduced cases leave out the two clouds with an empty side ("mean" divides by the
    lengths)."""
    x, y, dxy, ixy, dyx, iyx = chamfer_case
    keep = slice(0, None) if point_reduction is None else slice(2, None)
    x, y, dxy, ixy, dyx, iyx = (a[keep] for a in (x, y, dxy, ixy, dyx, iyx))
    l1, l2 = np.asarray(CH_L1)[keep], np.asarray(CH_L2)[keep]
    N = len(l1)
    rr = np.random.default_rng(5)
    w = rr.uniform(0.5, 2, N).astype(np.float32) if weighted else None
    nx = rr.standard_normal(x.shape).astype(np.float32) if normals else None
    ny = rr.standard_normal(y.shape).astype(np.float32) if normals else None
    opt = lambda a: dev(a, cuda) if a is not None else None
    cx, cy, cn = chamfer_distance(dev(x, cuda), dev(y, cuda), dev(l1.astype(np.int64), cuda),
                                  dev(l2.astype(np.int64), cuda), opt(nx), opt(ny), opt(w),
                                  batch_reduction=batch_reduction, point_reduction=point_reduction)
    wx = w[:, None] if weighted else np.float32(1)
    ex, ey = dxy * wx, dyx * wx                                                # (one fp32 product, as the module)
    if normals:
        en_x, en_y = _cosine_term(cuda, nx, ny, ixy, l1) * wx, _cosine_term(cuda, ny, nx, iyx, l2) * wx
    else:
        assert cn is None
    if point_reduction is None:
        assert np.array_equal(host(cx), ex) and np.array_equal(host(cy), ey)
        return
    red = lambda m, l: m.astype(np.float64).sum(1) / (l if point_reduction == "mean" else 1)
    div = (w.astype(np.float64).sum() if weighted else N) if batch_reduction == "mean" else 1
    np.testing.assert_allclose(host(cx), red(ex, l1).sum() / div, rtol=1e-6)
    np.testing.assert_allclose(host(cy), red(ey, l2).sum() / div, rtol=1e-6)
    if normals:
        want = (red(en_x, l1).sum() + red(en_y, l2).sum()) / div
        np.testing.assert_allclose(host(cn), want, rtol=1e-6)


def test_chamfer_distance_gradient_with_lengths(cuda, chamfer_case):
    """Both clouds require a gradient: two length-aware differentiable K = 1 searches.  Against oracle.knn_grad on the
    slices with the tolerance of test_knn_grad_vs_oracle (float atomics: 1e-5 relative to the gradient scale); padded
    rows receive exactly zero."""
    x, y, dxy, ixy, dyx, iyx = chamfer_case
    rr = np.random.default_rng(7)
    g1 = rr.standard_normal(dxy.shape).astype(np.float32)
    g2 = rr.standard_normal(dyx.shape).astype(np.float32)
    xt = torch.tensor(x, device=cuda, requires_grad=True)
    yt = torch.tensor(y, device=cuda, requires_grad=True)
    t1, t2 = lengths_on(cuda)
    cx, cy, _ = chamfer_distance(xt, yt, t1, t2, batch_reduction=None, point_reduction=None)
    assert cx.requires_grad and cy.requires_grad
    assert np.array_equal(host(cx), dxy) and np.array_equal(host(cy), dyx)
    ((cx * dev(g1, cuda)).sum() + (cy * dev(g2, cuda)).sum()).backward()
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    for b in range(len(CH_L1)):
        a, c = CH_L1[b], CH_L2[b]
        if a == 0 or c == 0:
            continue
        xs, ys = x[b:b + 1, :a], y[b:b + 1, :c]
        ax, ay = O.knn_grad(xs, ys, ixy[b:b + 1, :a, None], g1[b:b + 1, :a, None])
        by, bx = O.knn_grad(ys, xs, iyx[b:b + 1, :c, None], g2[b:b + 1, :c, None])
        gx[b, :a], gy[b, :c] = ax[0] + bx[0], ay[0] + by[0]
    scale = max(1.0, float(np.abs(gy).max()))                                 # (as test_knn_grad_vs_oracle)
    np.testing.assert_allclose(host(xt.grad), gx, rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(host(yt.grad), gy, rtol=1e-5, atol=1e-5 * scale)
    for b in range(len(CH_L1)):
        assert not host(xt.grad)[b, CH_L1[b]:].any() and not host(yt.grad)[b, CH_L2[b]:].any()


# ------------------------------------------------------------------ capture
def test_captured_searches_follow_lengths_overwritten_before_replay(cuda):
    """One knn_points and one chamfer_nn call with lengths, captured on a single stream; the length tensors are then
    overwritten in place and the graph replayed: the outputs follow the NEW lengths, so the lengths are read on the
    device at run time and never by the host."""
    n1, n2, K = 257, 130, 3
    first = ([257, 100, 1, 0, 256], [130, 64, 2, 77, 0])
    second = ([5, 257, 200, 64, 0], [65, 129, 130, 1, 99])
    # padding built for the SECOND lengths: the replay is the call whose leaks must show
    x, y = make_clouds(31, n1, n2, *second)
    xt, yt = dev(x, cuda), dev(y, cuda)
    t1, t2 = dev(np.asarray(first[0], np.int64), cuda), dev(np.asarray(first[1], np.int64), cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _ext.knn_points(xt, yt, K, lengths1=t1, lengths2=t2)
        _ext.chamfer_nn(xt, yt, t1, t2)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d, i, _ = _ext.knn_points(xt, yt, K, lengths1=t1, lengths2=t2)
            cdx, cix, cdy, ciy = _ext.chamfer_nn(xt, yt, t1, t2)
    torch.cuda.current_stream().wait_stream(s)
    for l1, l2 in (first, second):
        t1.copy_(dev(np.asarray(l1, np.int64), cuda))
        t2.copy_(dev(np.asarray(l2, np.int64), cuda))
        g.replay()
        torch.cuda.synchronize()
        od, oi = sliced_knn(x, y, l1, l2, K)
        assert np.array_equal(host(i), oi) and np.array_equal(host(d).view(np.uint32), od.view(np.uint32))
        dxy, ixy = sliced_knn(x, y, l1, l2, 1)
        dyx, iyx = sliced_knn(y, x, l2, l1, 1)
        assert np.array_equal(host(cix), np.maximum(ixy[..., 0], 0)) and np.array_equal(host(cdx), dxy[..., 0])
        assert np.array_equal(host(ciy), np.maximum(iyx[..., 0], 0)) and np.array_equal(host(cdy), dyx[..., 0])
