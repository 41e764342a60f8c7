"""All-pairs Chamfer kernel (pdr_chamfer_pairwise through _ext.chamfer_pairwise) and the set-level metrics of
pointnet2/set_metrics.py on the GPU.

Shapes (S, R, n, m), the smallest at which the kernel's loops can go wrong: (1,1,1,1); (3,5,130,70) a partial query
block and one LDS tile; (2,3,1100,257) two LDS tiles, odd sizes; (5,4,64,2100) more candidates than queries, three
tiles, and in the other direction a second query pass (a pass is 2048 queries); (9,9,200,200) the self-matrix; and (260,253,3,2): 65780 pairs,
the only size at which the pair grid has a second, partial row.

Tolerances.  Against the library's own minima (float64 sums of pdr_chamfer_nn's float32 distances): rtol 2^-17 =
128 * 2^-24, atol 0 -- every addend is non-negative, so a summation order with at most k dependent fp32 additions is
within k * 2^-24 of the exact sum, and the kernel's chain is ceil(max(n, m) / 256) + 10 <= 74 (header of
csrc/chamfer_pairs.hip).  Against float64 from scratch: rtol 1e-5 >= (128 + 8) * 2^-24, the 8 for the fp32 rounding of
one distance.

Symmetric: the self-matrix path and the plain call on (x, x) share their summation order (one routine sums a direction
from the two clouds' valid rows alone), so the WHOLE matrix is asserted bit-equal, not only the upper triangle.
"""
import os

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2 import set_metrics as SM
from point_diffusion_refinement_amd.pointnet2.emd import earth_mover_distance
from point_diffusion_refinement_amd.pointnet2_ops import _ext

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (3, 5, 130, 70), (2, 3, 1100, 257), (5, 4, 64, 2100), (9, 9, 200, 200)]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_metrics.npz")


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clouds(shape):
    S, R, n, m = shape
    rr = np.random.default_rng(S * 1000003 + R * 10007 + n * 101 + m)
    return rr.uniform(-1, 1, (S, n, 3)).astype(np.float32), rr.uniform(-1, 1, (R, m, 3)).astype(np.float32)


def cd_float64(x, y):
    """from scratch: distances, minima, means and their sum in float64"""
    out = np.zeros((x.shape[0], y.shape[0]))
    for s, a in enumerate(x.astype(np.float64)):
        for r, b in enumerate(y.astype(np.float64)):
            d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
            out[s, r] = d.min(1).mean() + d.min(0).mean()
    return out


_cache = {}


def case(shape, cuda):
    """clouds, the kernel's matrix and the two expected matrices of a shape: computed once, shared, never modified"""
    if shape not in _cache:
        S, R, n, m = shape
        x, y = clouds(shape)
        xt, yt = dev(x, cuda), dev(y, cuda)
        cd = host(_ext.chamfer_pairwise(xt, yt))
        # the composed route: every pair spelled out, the library's own K = 1 minima, summed in float64
        si, ri = np.divmod(np.arange(S * R), R)
        dx, _, dy, _ = _ext.chamfer_nn(xt[dev(si, cuda)].contiguous(), yt[dev(ri, cuda)].contiguous())
        own = (host(dx).astype(np.float64).sum(1) / n + host(dy).astype(np.float64).sum(1) / m).reshape(S, R)
        _cache[shape] = dict(x=x, y=y, xt=xt, yt=yt, cd=cd, own=own, f64=cd_float64(x, y))
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_the_librarys_own_minima(cuda, shape):
    c = case(shape, cuda)
    assert c["cd"].shape == shape[:2] and c["cd"].dtype == np.float32
    print("max rel. deviation from the float64 sum of pdr_chamfer_nn minima:", np.max(np.abs(c["cd"] - c["own"]) / c["own"]))
    np.testing.assert_allclose(c["cd"], c["own"], rtol=2.0 ** -17, atol=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_float64_from_scratch(cuda, shape):
    c = case(shape, cuda)
    print("max rel. deviation from float64:", np.max(np.abs(c["cd"] - c["f64"]) / c["f64"]))
    np.testing.assert_allclose(c["cd"], c["f64"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_two_calls_give_the_same_bits(cuda, shape):
    c = case(shape, cuda)
    again = host(_ext.chamfer_pairwise(c["xt"], c["yt"]))
    assert np.array_equal(bits(again), bits(c["cd"]))


def test_second_grid_row(cuda):
    """65780 pairs of tiny clouds: the grid is 65536 wide with a second, partial row"""
    S, R, n, m = shape = (260, 253, 3, 2)
    x, y = clouds(shape)
    xt, yt = dev(x, cuda), dev(y, cuda)
    d = ((x.astype(np.float64)[:, None, :, None, :] - y.astype(np.float64)[None, :, None, :, :]) ** 2).sum(-1)
    want = d.min(3).mean(2) + d.min(2).mean(2)
    cd = host(_ext.chamfer_pairwise(xt, yt))
    np.testing.assert_allclose(cd, want, rtol=1e-5, atol=0)
    # and the self-matrix at that size
    full, sym = host(_ext.chamfer_pairwise(xt, xt)), host(_ext.chamfer_pairwise(xt, xt, symmetric=True))
    assert np.array_equal(bits(full), bits(sym)) and not np.any(np.diag(sym))


def test_symmetric_self_matrix(cuda):
    c = case((9, 9, 200, 200), cuda)
    xt = c["xt"]
    lens = dev(np.array([200, 199, 1, 0, 200, 150, 64, 200, 205], np.int64), cuda)
    for l in (None, lens):
        sym = host(_ext.chamfer_pairwise(xt, xt, l, l, symmetric=True))
        assert np.array_equal(bits(sym), bits(sym.T))
        assert np.array_equal(bits(np.diag(sym)), np.zeros(9, np.uint32))          # exactly +0
        full = host(_ext.chamfer_pairwise(xt, xt, l, l))
        assert np.array_equal(bits(sym), bits(full))                                # the whole matrix, see the header
        assert np.all(sym[~np.eye(9, dtype=bool)][None] >= 0)
        # pairwise_cd takes the self-matrix path by itself when it is handed one object twice
        assert np.array_equal(bits(host(SM.pairwise_cd(xt, xt, l, l))), bits(sym))
    empty = 3
    assert not np.any(sym[empty]) and not np.any(sym[:, empty])                     # an empty cloud: 0 with everyone
    assert np.all(sym[np.arange(9) != empty][:, np.arange(9) != empty][~np.eye(8, dtype=bool)] > 0)
    # the binding refuses a self-matrix of two sets
    with pytest.raises(RuntimeError, match="invalid argument"):
        _ext.chamfer_pairwise(xt, xt.clone(), symmetric=True)


def padded_case(shape, rnd):
    """Ragged clouds of a shape.  lengths_x[s] walks {0, 1, n-1, n, n+5} with s and the round, lengths_y likewise: over
    the 5 rounds every cloud takes every value.  The padded rows of every x cloud hold copies of valid y points and the
    other way round -- a candidate taken from the padding shows up as a minimum of 0 -- or, for every other cloud, NaN."""
    S, R, n, m = shape
    x, y = clouds(shape)
    lx = np.array([(0, 1, n - 1, n, n + 5)[(s + rnd) % 5] for s in range(S)], np.int64)
    ly = np.array([(0, 1, m - 1, m, m + 5)[(r + 2 * rnd + 1) % 5] for r in range(R)], np.int64)
    vx = np.concatenate([x[s, :min(lx[s], n)] for s in range(S)])
    vy = np.concatenate([y[r, :min(ly[r], m)] for r in range(R)])
    for arr, lens, other, size in ((x, lx, vy, n), (y, ly, vx, m)):
        for b in range(arr.shape[0]):
            a = int(min(lens[b], size))
            if a < size:
                if (b + rnd) % 2 or len(other) == 0:
                    arr[b, a:] = np.nan
                else:
                    arr[b, a:] = other[(np.arange(size - a) + 7 * b) % len(other)]
    return x, y, lx, ly


@pytest.mark.parametrize("shape", SHAPES[:4])
def test_lengths_give_the_dense_call_on_the_slices(cuda, shape):
    S, R, n, m = shape
    for rnd in range(5):
        x, y, lx, ly = padded_case(shape, rnd)
        xt, yt = dev(x, cuda), dev(y, cuda)
        got = host(_ext.chamfer_pairwise(xt, yt, dev(lx, cuda), dev(ly, cuda)))
        want = np.zeros((S, R), np.float32)                     # a pair with an empty side: 0
        for s in range(S):
            for r in range(R):
                a, c = int(min(lx[s], n)), int(min(ly[r], m))
                if a > 0 and c > 0:
                    want[s, r] = host(_ext.chamfer_pairwise(xt[s:s + 1, :a].contiguous(), yt[r:r + 1, :c].contiguous()))[0, 0]
        assert np.array_equal(bits(got), bits(want)), (shape, rnd, got, want)
        assert np.all(np.isfinite(got))
        assert np.all((got == 0) == ((np.minimum(lx, n)[:, None] == 0) | (np.minimum(ly, m)[None, :] == 0)))


@pytest.mark.parametrize("shape", SHAPES[1:4])
def test_full_or_absent_lengths_are_the_dense_call(cuda, shape):
    c = case(shape, cuda)
    S, R, n, m = shape
    fx, fy = dev(np.full(S, n, np.int64), cuda), dev(np.full(R, m + 3, np.int64), cuda)
    for lx, ly in ((fx, fy), (fx, None), (None, fy)):
        assert np.array_equal(bits(host(_ext.chamfer_pairwise(c["xt"], c["yt"], lx, ly))), bits(c["cd"]))
    assert np.array_equal(bits(host(SM.pairwise_cd(c["xt"], c["yt"]))), bits(c["cd"]))


def test_pairwise_emd_is_earth_mover_distance_on_the_explicit_pairs(cuda):
    S, R, n, m = shape = (3, 5, 130, 70)
    c = case(shape, cuda)
    xt, yt = c["xt"], c["yt"]
    si, ri = (dev(a, cuda) for a in np.divmod(np.arange(S * R), R))
    X, Y = xt[si].contiguous(), yt[ri].contiguous()
    want = host(earth_mover_distance(X, Y)).reshape(S, R)
    assert np.all(want > 0)
    for bs in (1, 3, 1000):
        assert np.array_equal(bits(host(SM.pairwise_emd(xt, yt, bs))), bits(want)), bs
    lx = dev(np.array([130, 1, 77], np.int64), cuda)
    ly = dev(np.array([70, 0, 35, 69, 75], np.int64), cuda)
    want = host(earth_mover_distance(X, Y, lengths1=lx[si], lengths2=ly[ri])).reshape(S, R)
    assert not np.any(want[:, 1]) and np.all(want[:, [0, 2, 3, 4]] > 0)
    for bs in (1, 3, 1000):
        assert np.array_equal(bits(host(SM.pairwise_emd(xt, yt, bs, lx, ly))), bits(want)), bs
    # one-sided lengths
    want = host(earth_mover_distance(X, Y, lengths2=ly[ri])).reshape(S, R)
    assert np.array_equal(bits(host(SM.pairwise_emd(xt, yt, 4, None, ly))), bits(want))


def fixture(cuda):
    with np.load(GOLD) as z:
        gold = {k: z[k] for k in z.files}
    return gold, dev(gold["sample_pcs"], cuda), dev(gold["ref_pcs"], cuda), int(gold["batch_size"])


def fixture_matrices(cuda):
    if "fixture" not in _cache:
        gold, smp, ref, bs = fixture(cuda)
        _cache["fixture"] = {tag: tuple(host(M) for M in SM.pairwise_emd_cd(a, b, bs))
                             for tag, (a, b) in (("rs", (ref, smp)), ("rr", (ref, ref)), ("ss", (smp, smp)))}
    return _cache["fixture"]


def test_pairwise_matrices_on_the_reference_fixture(cuda):
    """The three CD matrices against the reference's at rtol 1e-5, atol 0; the three EMD matrices, every entry, at the
    project's EMD bar of rtol 1e-4 (tests/test_fullsize_gpu.py) plus the UNDERFLOW term of fp32 arithmetic.

    Why an absolute term at all: the model of an fp32 operation is fl(a op b) = (a op b)(1 + d) + e with |d| <= 2^-24
    and, where the result is subnormal, |e| <= 2^-150.  A purely relative bound drops e, and the diagonals of the EMD
    self-matrices live where e is everything: the approximate EMD of a cloud with itself is a sum of products that
    underflow (diagonal entries between 0 and 7.3e-12, most of them subnormal; the first version of this test, with
    atol 0, failed on M_rr_emd[5,5] = 0.0 against the oracle's 4.2e-45 and M_ss_emd[4,4] = 0.0 against 7.0e-45, three
    and five steps of the format, and on nothing else).  The term, from the arithmetic and not from those figures: an
    entry is (1 / n) * sum over n * m pairs of d2 * match, match = a sum over 10 levels of a product of three factors;
    per pair at most 30 operations of match can underflow (30 * 2^-150), scaled by d2 <= 27 (coordinates within
    [-1.5, 1.5]^3), plus the product and its addition: < 2^9 * 2^-149 per pair and per evaluation, 2^10 * 2^-149 for
    the two evaluations compared, times n * m / n:
        atol = 2^10 * m * 2^-149 = 1.4e-40 at m = 96
    -- 32 orders of magnitude below the atol of 1e-8 that torch.allclose adds to the same bar in test_fullsize_gpu.py,
    and 39 below the smallest off-diagonal entry, so for every entry the metrics read the bound is the relative one."""
    gold = fixture(cuda)[0]
    got = fixture_matrices(cuda)
    atol_emd = 2.0 ** 10 * gold["ref_pcs"].shape[1] * 2.0 ** -149
    for tag in ("rs", "rr", "ss"):
        for kind, M, rtol, atol in (("cd", got[tag][0], 1e-5, 0.0), ("emd", got[tag][1], 1e-4, atol_emd)):
            want = gold["M_%s_%s" % (tag, kind)]
            off = np.ones(M.shape, bool) if tag == "rs" else ~np.eye(len(M), dtype=bool)
            print("M_%s_%s max rel. off the self-diagonal %.3g" % (tag, kind, np.max(np.abs(M - want)[off] / want[off])),
                  "" if tag == "rs" else "diagonal %s golden %s" % (np.diag(M), np.diag(want)))
            np.testing.assert_allclose(M, want, rtol=rtol, atol=atol, err_msg="M_%s_%s" % (tag, kind))
        if tag != "rs":
            assert not np.any(np.diag(got[tag][0])) and np.all(np.diag(got[tag][1]) >= 0)


def test_compute_all_metrics_on_the_reference_fixture(cuda):
    gold, smp, ref, bs = fixture(cuda)
    res = SM.compute_all_metrics(smp, ref, bs)
    want = {k[4:]: v for k, v in gold.items() if k.startswith("all/")}
    assert sorted(res) == sorted(want) and len(res) == 12
    for k, v in res.items():
        assert v.device.type == "cuda"
        print(k, host(v), want[k])
        if "cov" in k or "acc" in k:
            assert np.array_equal(host(v), want[k]), (k, host(v), want[k])
        else:
            np.testing.assert_allclose(host(v), want[k], rtol=1e-4, atol=0, err_msg=k)
