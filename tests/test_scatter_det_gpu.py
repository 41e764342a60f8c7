"""Deterministic backward twins on the GPU: gather / group / three_interpolate grads and the kNN backward through
`_ext.*_grad_det`, compared BIT FOR BIT (uint32 views) with the CPU oracle, whose sequential loops fix the summation
order these kernels implement (sources in ascending position, fp32, from +0.0, products rounded before the add).

Index patterns: every index equal (one segment longer than several builder ranges: the wave-per-destination sum), a
permutation (every segment one source), destinations nobody names (+0.0, sign bit included), a real ball-query index
with empty balls.  Sizes: B in {1, 3}, C in {1, 9, 16} (slab remainder), N in {1, 63, 96, 3072} and 16384 (the scan's
widest), P odd, P = 0, P beyond 65536 (longer builder ranges), the full-size grouping shape."""
import numpy as np
import pytest
import torch

from oracle import pdr_oracle as O
from point_diffusion_refinement_amd.pointnet2_ops import _ext
from point_diffusion_refinement_amd.pointnet2_ops import pointnet2_utils as PU

gpu = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def values(rr, kind, shape):
    """'wide': +-10^U(-3, 3); 'normal': standard normal."""
    if kind == "wide":
        return (rr.choice([-1.0, 1.0], shape) * 10.0 ** rr.uniform(-3, 3, shape)).astype(np.float32)
    return rr.standard_normal(shape).astype(np.float32)


KINDS = ("wide", "normal")


def ball_index():
    """A real ball-query index with empty balls: B=2, N=96, np=64, ns=8, r=0.45, eight queries of each cloud shifted
    out of it (their rows are all 0, so point 0 collects 64 extra sources)."""
    rr = np.random.default_rng(77)
    p = rr.uniform(-1, 1, (2, 96, 3)).astype(np.float32)
    q = p[:, :64].copy()
    q[:, 5::8] += 10.0
    idx, cnt = O.ball_query(q, p, 0.45, 8)
    assert (cnt == 0).sum() == 16 and (idx[cnt == 0] == 0).all()
    return idx, p, q


def pattern(rr, name, B, P, N):
    """(B, P) destinations in [0, N)."""
    if name == "equal":
        return np.full((B, P), N // 2, np.int32)
    if name == "perm":
        assert P == N
        return np.stack([rr.permutation(N) for _ in range(B)]).astype(np.int32)
    if name == "sparse":                                    # only every fifth destination is ever named
        return (rr.integers(0, (N + 4) // 5, (B, P)) * 5).astype(np.int32)
    return rr.integers(0, N, (B, P)).astype(np.int32)


# ------------------------------------------------------------------------------------ the sanity check (no GPU needed)
def test_reversing_the_source_order_changes_the_bits():
    """A condition of the whole file, not a measurement: on the ball-query index, adding every destination's sources in
    DESCENDING position must change the bits of >= 20 % of the destination elements with more than one source --
    otherwise a bit comparison could not tell the fixed order from another one."""
    idx, _, _ = ball_index()
    B, N, P, C = 2, 96, 64 * 8, 5
    flat = idx.reshape(B, P)
    counts = np.stack([np.bincount(flat[b], minlength=N) for b in range(B)])
    assert counts.max() >= 64 and (counts == 0).any()
    multi = np.broadcast_to((counts >= 2)[:, None, :], (B, C, N))
    for kind in KINDS:
        g = values(np.random.default_rng(5), kind, (B, C, 64, 8))
        fwd = O.group_points_grad(g, idx, N)
        rev = O.gather_points_grad(g.reshape(B, C, P)[..., ::-1].copy(), flat[:, ::-1].copy(), N)
        np.testing.assert_allclose(rev, fwd, rtol=1e-4, atol=1e-4 * np.abs(g).max())     # the same gradient ...
        changed = (bits(fwd) != bits(rev))[multi].mean()
        print("reversed order changes %.1f %% of the multi-source elements (%s values)" % (100 * changed, kind))
        assert changed >= 0.20, (kind, changed)                                           # ... in other bits


# ------------------------------------------------------------------------------------------------ gather / group
# (B, C, N, units, pattern): gather has m = units, group np = units and ns = 3, interpolate n = units (P = 3 units)
ROW_CASES = [(1, 1, 1, 259, "equal"), (3, 9, 63, 337, "random"), (1, 16, 96, 833, "sparse"), (3, 9, 3072, 1667, "random"),
             (1, 16, 3072, 1667, "equal"), (3, 1, 96, 1667, "equal"), (1, 9, 3072, 1667, "sparse"),
             (3, 16, 63, 0, "random"), (1, 1, 3072, 0, "random")]


@gpu
@pytest.mark.parametrize("B,C,N,u,pat", ROW_CASES + [(3, 9, 63, 63, "perm"), (1, 16, 3072, 3072, "perm"),
                                                      (1, 1, 63, 70001, "random"), (1, 9, 16384, 4099, "random")])
def test_gather_grad_det_bits(cuda, B, C, N, u, pat):
    rr = np.random.default_rng(B + C + N + u)
    idx = pattern(rr, pat, B, u, N)
    for kind in KINDS:
        g = values(rr, kind, (B, C, u))
        got = _ext.gather_points_grad_det(dev(g, cuda), dev(idx, cuda), N)
        assert same_bits(got, O.gather_points_grad(g, idx, N)), kind
    if pat == "sparse":
        unnamed = np.setdiff1d(np.arange(N), idx.reshape(-1))
        assert unnamed.size and (bits(got.cpu().numpy())[:, :, unnamed] == 0).all()       # +0.0: sign bit clear


@gpu
@pytest.mark.parametrize("B,C,N,u,pat", ROW_CASES + [(3, 9, 63, 21, "perm"), (1, 16, 3072, 1024, "perm")])
def test_group_grad_det_bits(cuda, B, C, N, u, pat):
    rr = np.random.default_rng(2 * B + C + N + u)
    idx = pattern(rr, pat, B, u * 3, N).reshape(B, u, 3)
    for kind in KINDS:
        g = values(rr, kind, (B, C, u, 3))
        got = _ext.group_points_grad_det(dev(g, cuda), dev(idx, cuda), N)
        assert same_bits(got, O.group_points_grad(g, idx, N)), kind
    if pat == "sparse":
        unnamed = np.setdiff1d(np.arange(N), idx.reshape(-1))
        assert unnamed.size and (bits(got.cpu().numpy())[:, :, unnamed] == 0).all()


@gpu
@pytest.mark.parametrize("B,C,N,u,pat", ROW_CASES + [(3, 9, 63, 21, "perm"), (1, 16, 3072, 1024, "perm")])
def test_three_interpolate_grad_det_bits(cuda, B, C, N, u, pat):
    rr = np.random.default_rng(3 * B + C + N + u)
    idx = pattern(rr, pat, B, u * 3, N).reshape(B, u, 3)
    for kind in KINDS:
        g = values(rr, kind, (B, C, u))
        w = values(rr, kind, (B, u, 3)) if kind == "wide" else rr.random((B, u, 3)).astype(np.float32)
        got = _ext.three_interpolate_grad_det(dev(g, cuda), dev(idx, cuda), dev(w, cuda), N)
        assert same_bits(got, O.three_interpolate_grad(g, idx, w, N)), kind
    if pat == "sparse":
        unnamed = np.setdiff1d(np.arange(N), idx.reshape(-1))
        assert unnamed.size and (bits(got.cpu().numpy())[:, :, unnamed] == 0).all()


@gpu
def test_ball_query_index_with_empty_balls_all_ops(cuda):
    """The issue's input: B=2, C=5, N=96, np=64, ns=8, r=0.45 with empty balls, through all four ops."""
    idx, p, q = ball_index()
    B, C, N = 2, 5, 96
    rr = np.random.default_rng(9)
    for kind in KINDS:
        g = values(rr, kind, (B, C, 64, 8))
        assert same_bits(_ext.group_points_grad_det(dev(g, cuda), dev(idx, cuda), N), O.group_points_grad(g, idx, N))
        flat, gf = idx.reshape(B, 512), g.reshape(B, C, 512)
        assert same_bits(_ext.gather_points_grad_det(dev(gf, cuda), dev(flat, cuda), N), O.gather_points_grad(gf, flat, N))
        tri, gt, w = flat[:, :510].reshape(B, 170, 3).copy(), g.reshape(B, C, 512)[:, :, :170].copy(), values(rr, kind, (B, 170, 3))
        assert same_bits(_ext.three_interpolate_grad_det(dev(gt, cuda), dev(tri, cuda), dev(w, cuda), N),
                         O.three_interpolate_grad(gt, tri, w, N))
        for K in (1, 4):
            ki = flat.reshape(B, 512 // K, K).astype(np.int64)
            gd = values(rr, kind, (B, 512 // K, K))
            x = rr.standard_normal((B, 512 // K, 3)).astype(np.float32)
            gx, gy = _ext.knn_points_grad(dev(x, cuda), dev(p, cuda), dev(ki, cuda), dev(gd, cuda), deterministic=True)
            ox, oy = O.knn_grad(x, p, ki, gd)
            assert same_bits(gx, ox) and same_bits(gy, oy), (kind, K)


# ------------------------------------------------------------------------------------------------------------ kNN
@gpu
@pytest.mark.parametrize("B,n1,n2,K,pat", [(1, 259, 1, 1, "equal"), (3, 337, 63, 4, "random"), (1, 833, 96, 4, "sparse"),
                                           (3, 1667, 3072, 1, "random"), (1, 1667, 3072, 4, "equal"),
                                           (3, 63, 63, 1, "perm"), (1, 24, 96, 4, "perm"), (1, 768, 3072, 4, "perm"),
                                           (1, 4099, 16384, 1, "random"), (3, 0, 63, 4, "random"),
                                           (1, 17501, 96, 4, "random")])
def test_knn_grad_det_bits(cuda, B, n1, n2, K, pat):
    rr = np.random.default_rng(5 * B + n1 + n2 + K)
    idx = pattern(rr, pat, B, n1 * K, n2).reshape(B, n1, K).astype(np.int64)
    if pat in ("random", "sparse") and n1:
        idx[rr.random(idx.shape) < 0.1] = -1                                    # padding slots are skipped
    x = rr.standard_normal((B, n1, 3)).astype(np.float32)
    y = rr.standard_normal((B, n2, 3)).astype(np.float32)
    for kind in KINDS:
        gd = values(rr, kind, (B, n1, K))
        gx, gy = _ext.knn_points_grad(dev(x, cuda), dev(y, cuda), dev(idx, cuda), dev(gd, cuda), deterministic=True)
        ox, oy = O.knn_grad(x, y, idx, gd)
        assert same_bits(gx, ox), kind
        assert same_bits(gy, oy), kind
    if pat == "sparse":
        unnamed = np.setdiff1d(np.arange(n2), idx.reshape(-1))
        assert unnamed.size and (bits(gy.cpu().numpy())[:, unnamed] == 0).all()


@gpu
@pytest.mark.parametrize("K", [1, 4])
def test_knn_grad_det_on_the_ragged_forward(cuda, K):
    """The -1 slots of the length-aware forward (padded queries, clouds shorter than K) add nothing."""
    rr = np.random.default_rng(31 + K)
    B, n1, n2 = 3, 300, 96
    x = rr.standard_normal((B, n1, 3)).astype(np.float32)
    y = rr.standard_normal((B, n2, 3)).astype(np.float32)
    l1, l2 = torch.tensor([300, 123, 0], device=cuda), torch.tensor([96, 2, 50], device=cuda)
    _, idx, _ = _ext.knn_points(dev(x, cuda), dev(y, cuda), K, lengths1=l1, lengths2=l2)
    hidx = idx.cpu().numpy()
    assert (hidx < 0).any() and (hidx >= 0).any()
    for kind in KINDS:
        gd = values(rr, kind, (B, n1, K))
        gx, gy = _ext.knn_points_grad(dev(x, cuda), dev(y, cuda), idx, dev(gd, cuda), deterministic=True)
        ox, oy = O.knn_grad(x, y, hidx, gd)
        assert same_bits(gx, ox) and same_bits(gy, oy), kind
        assert (bits(gy.cpu().numpy())[1, 2:] == 0).all() and (bits(gx.cpu().numpy())[2] == 0).all()


# ------------------------------------------------------------------------------------------------------ full size
@gpu
def test_group_grad_det_full_size_with_empty_balls(cuda):
    """B=2, C=16, N=3072, np=2048, ns=32: the feature-transfer level, a tenth of the balls empty (point 0 collects
    their 32 slots each: one segment of several thousand sources among ordinary ones)."""
    rr = np.random.default_rng(41)
    B, C, N, npnt, ns = 2, 16, 3072, 2048, 32
    idx = rr.integers(0, N, (B, npnt, ns)).astype(np.int32)
    idx[rr.random((B, npnt)) < 0.1] = 0
    for kind in KINDS:
        g = values(rr, kind, (B, C, npnt, ns))
        got = _ext.group_points_grad_det(dev(g, cuda), dev(idx, cuda), N)
        assert same_bits(got, O.group_points_grad(g, idx, N)), kind


# ------------------------------------------------------------------------------------------------------ run to run
@gpu
def test_same_bits_run_to_run_and_from_a_captured_graph(cuda):
    idx, p, _ = ball_index()
    rr = np.random.default_rng(51)
    B, C, N = 2, 5, 96
    g = dev(values(rr, "wide", (B, C, 64, 8)), cuda)
    gi = dev(idx, cuda)
    tri, w = dev(idx.reshape(B, 512)[:, :510].reshape(B, 170, 3).copy(), cuda), dev(values(rr, "wide", (B, 170, 3)), cuda)
    gt = dev(values(rr, "wide", (B, C, 170)), cuda)
    ki, gd = dev(idx.reshape(B, 128, 4).astype(np.int64), cuda), dev(values(rr, "wide", (B, 128, 4)), cuda)
    x, y = dev(rr.standard_normal((B, 128, 3)).astype(np.float32), cuda), dev(p, cuda)

    def run():
        return (_ext.group_points_grad_det(g, gi, N), _ext.gather_points_grad_det(g.view(B, C, 512), gi.view(B, 512), N),
                _ext.three_interpolate_grad_det(gt, tri, w, N)) + _ext.knn_points_grad(x, y, ki, gd, deterministic=True)

    first = [t.cpu().numpy() for t in run()]
    second = [t.cpu().numpy() for t in run()]
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                               # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.cpu().numpy() for t in captured]
    for a, b_, c in zip(first, second, replayed):
        assert np.array_equal(bits(a), bits(b_)) and np.array_equal(bits(a), bits(c))


# ----------------------------------------------------------------------------------------- against the atomic twin
@gpu
def test_det_equals_the_atomic_twin_within_its_tolerances(cuda):
    """The two are the same gradient: tolerances and inputs of tests/test_ops_gpu.py (standard normal values, random
    indices; gather 1e-5, group and interpolate 1e-4, kNN 1e-5 of the gradient scale)."""
    rr = np.random.default_rng(61)
    for B, C, N, m in [(2, 3, 100, 37), (2, 35, 2048, 1024)]:
        idx, g = dev(rr.integers(0, N, (B, m)).astype(np.int32), cuda), dev(values(rr, "normal", (B, C, m)), cuda)
        np.testing.assert_allclose(_ext.gather_points_grad_det(g, idx, N).cpu().numpy(),
                                   _ext.gather_points_grad(g, idx, N).cpu().numpy(), rtol=1e-5, atol=1e-5)
    for B, C, N, npnt, ns in [(2, 4, 100, 37, 8), (3, 9, 16, 16, 32), (2, 32, 3072, 2048, 32)]:
        idx = dev(rr.integers(0, N, (B, npnt, ns)).astype(np.int32), cuda)
        g = dev(values(rr, "normal", (B, C, npnt, ns)), cuda)
        np.testing.assert_allclose(_ext.group_points_grad_det(g, idx, N).cpu().numpy(),
                                   _ext.group_points_grad(g, idx, N).cpu().numpy(), rtol=1e-4, atol=1e-4)
    for B, C, n, m in [(2, 19, 333, 1500), (2, 19, 2048, 1024)]:
        idx = dev(rr.integers(0, m, (B, n, 3)).astype(np.int32), cuda)
        g, w = dev(values(rr, "normal", (B, C, n)), cuda), dev(rr.random((B, n, 3)).astype(np.float32), cuda)
        np.testing.assert_allclose(_ext.three_interpolate_grad_det(g, idx, w, m).cpu().numpy(),
                                   _ext.three_interpolate_grad(g, idx, w, m).cpu().numpy(), rtol=1e-4, atol=1e-4)
    for B, n1, n2, K in [(2, 300, 257, 1), (2, 128, 64, 8)]:
        x, y = dev(values(rr, "normal", (B, n1, 3)), cuda), dev(values(rr, "normal", (B, n2, 3)), cuda)
        gd = dev(values(rr, "normal", (B, n1, K)), cuda)
        _, idx, _ = _ext.knn_points(x, y, K)
        dx, dy = _ext.knn_points_grad(x, y, idx, gd, deterministic=True)
        ax, ay = _ext.knn_points_grad(x, y, idx, gd, deterministic=False)
        scale = max(1.0, float(ay.abs().max()))
        assert torch.equal(dx, ax)                                               # grad_x: the same code, the same bits
        np.testing.assert_allclose(dy.cpu().numpy(), ay.cpu().numpy(), rtol=1e-5, atol=1e-5 * scale)


# ------------------------------------------------------------------------------------------------ through autograd
@pytest.fixture
def torch_deterministic():
    prev_switch, prev = _ext.set_deterministic(None), torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev)
    _ext.set_deterministic(prev_switch)


@gpu
def test_calc_cd_backward_is_bit_reproducible_under_the_torch_flag(cuda, torch_deterministic):
    from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import calc_cd
    rr = np.random.default_rng(71)
    out = rr.standard_normal((2, 700, 3)).astype(np.float32)
    gt = np.repeat(rr.standard_normal((2, 40, 3)), 10, axis=1).astype(np.float32)          # clusters: many queries share a target
    gt += rr.standard_normal(gt.shape).astype(np.float32) * 1e-3
    grads = []
    for _ in range(2):
        o, t = dev(out, cuda).requires_grad_(), dev(gt, cuda).requires_grad_()
        cd_p, cd_t = calc_cd(o, t)
        (cd_p.sum() + cd_t.sum()).backward()
        grads.append((o.grad.cpu().numpy(), t.grad.cpu().numpy()))
    assert np.array_equal(bits(grads[0][0]), bits(grads[1][0])) and np.array_equal(bits(grads[0][1]), bits(grads[1][1]))
    assert np.isfinite(grads[0][0]).all() and np.abs(grads[0][1]).max() > 0
    # its kNN part: knn_points' backward under the flag is the oracle's, bit for bit
    o, t = dev(out, cuda).requires_grad_(), dev(gt, cuda).requires_grad_()
    gd = values(rr, "wide", (2, 700, 1))
    d, idx, _ = _ext.knn_points(o, t, 1)
    (d * dev(gd, cuda)).sum().backward()
    ox, oy = O.knn_grad(out, gt, idx.cpu().numpy(), gd)
    assert same_bits(o.grad, ox) and same_bits(t.grad, oy)


@gpu
def test_query_and_group_backward_is_bit_reproducible_under_the_torch_flag(cuda, torch_deterministic):
    idx, p, q = ball_index()
    rr = np.random.default_rng(81)
    feats = values(rr, "normal", (2, 5, 96))
    wgt = values(rr, "wide", (2, 8, 64, 8))                                               # 5 feature + 3 xyz channels
    grouper = PU.QueryAndGroup(0.45, 8, use_xyz=True)
    grads = []
    for _ in range(2):
        f, xyz = dev(feats, cuda).requires_grad_(), dev(p, cuda).requires_grad_()
        (grouper(xyz, dev(q, cuda), f) * dev(wgt, cuda)).sum().backward()
        grads.append((f.grad.cpu().numpy(), xyz.grad.cpu().numpy()))
    assert np.array_equal(bits(grads[0][0]), bits(grads[1][0])) and np.array_equal(bits(grads[0][1]), bits(grads[1][1]))
    # its group part: the feature gradient is group_points_grad of the weights, the oracle's bits
    assert same_bits(grads[0][0], O.group_points_grad(wgt[:, :5], idx, 96))
    assert same_bits(np.ascontiguousarray(grads[0][1].transpose(0, 2, 1)), O.group_points_grad(wgt[:, 5:], idx, 96))
