"""Direct parity tests of the assembly and activation kernels (csrc/fused_gather.hip, csrc/act_ops.hip):
pdr_group_build, pdr_knn_build, pdr_gather_rows, pdr_gather_rows2, pdr_pad_rows, pdr_apply_act, pdr_act_colmax.

Every kernel is called through the C ABI and compared with a plain numpy evaluation of its definition in
include/pdr_hip.h (never with its own Python wrapper).  Outputs are pre-filled with NaN and carry a guard row behind
the last row: everything the contract says is written must match, everything else must still be NaN.  Every index
handed to a kernel is in range and every kNN case has K <= n2."""
import ctypes

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2_ops import pointnet2_utils as PU

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 2                                                    # sentinel rows behind the last output row


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sentinel(rows, ld, cuda):
    return torch.full((rows + GUARD, ld), float("nan"), dtype=torch.float32, device=cuda)


def _assert_bits(got, want, what):
    """Bit equality of two float32 arrays, with the first difference in the message."""
    got = np.ascontiguousarray(got, dtype=F32)
    want = np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, len(bad), got.size, i, got[i], want[i]))


def _assert_untouched(a, what):
    assert np.isnan(a).all(), "%s: %d of %d sentinel elements were overwritten" % (what, int((~np.isnan(a)).sum()), a.size)


# ---------------------------------------------------------------------------------------------------------------------
# pdr_group_build
# ---------------------------------------------------------------------------------------------------------------------

def _group_build_ref(feats, xyz, new_xyz, idx, counts, patch_empty, with_abs, with_centre, ldo):
    """[feats[idx] | xyz[idx] - centre | (xyz[idx]) | (centre) | 0 ...]; an empty ball of patch_empty is its own centre
    with a zero feature.  float32 throughout: one subtraction, everything else a copy."""
    B, m, K = idx.shape
    bi = np.arange(B)[:, None, None]
    ab = xyz[bi, idx]                                                   # (B, m, K, 3)
    ctr = np.broadcast_to(new_xyz[:, :, None, :], ab.shape)
    f = feats[bi, idx] if feats is not None else np.zeros((B, m, K, 0), F32)
    if patch_empty:
        empty = (counts <= 0)[:, :, None, None]
        ab = np.where(empty, ctr, ab)
        f = np.where(empty, F32(0), f)
    parts = [f, ab - ctr] + ([ab] if with_abs else []) + ([ctr] if with_centre else [])
    G = np.concatenate(parts, axis=-1).reshape(B * m * K, -1).astype(F32)
    out = np.zeros((B * m * K, ldo), F32)
    out[:, :G.shape[1]] = G
    return out, G.shape[1]


class _GroupInputs:
    """Random clouds, in-range neighbour indices (rows 0 and n - 1 included) and ball counts with about a third of the
    balls empty; an empty ball keeps a random index, which the kernel must not use."""

    def __init__(self, cuda, B, n, m, K, Cs, seed):
        rng = np.random.default_rng(seed)
        self.B, self.n, self.m, self.K, self.Cs = B, n, m, K, Cs
        self.feats = rng.standard_normal((B, n, Cs)).astype(F32) if Cs else None
        self.xyz = rng.uniform(-1, 1, (B, n, 3)).astype(F32)
        self.new_xyz = rng.uniform(-1, 1, (B, m, 3)).astype(F32)
        self.idx = rng.integers(0, n, (B, m, K)).astype(np.int32)
        self.idx.reshape(-1)[0] = n - 1
        self.idx.reshape(-1)[-1] = 0
        self.counts = np.where(rng.random((B, m)) < 1 / 3, 0, rng.integers(1, K + 1, (B, m))).astype(np.int32)
        if B * m >= 3:
            self.counts.reshape(-1)[1] = 0
        self.d = {k: _dev(getattr(self, k), cuda) for k in ("xyz", "new_xyz", "idx", "counts")}
        self.d["feats"] = _dev(self.feats, cuda) if Cs else None
        self.cuda = cuda

    def run(self, mode, with_abs, with_centre, pad):
        """mode: 'patch' (patch_empty = 1), 'nopatch' (patch_empty = 0, counts given), 'nocounts' (counts NULL)."""
        B, n, m, K, Cs = self.B, self.n, self.m, self.K, self.Cs
        Cout = Cs + 3 + (3 if with_abs else 0) + (3 if with_centre else 0)
        ldo = Cout + pad
        rows = B * m * K
        out = _sentinel(rows, ldo, self.cuda)
        d = self.d
        rc = _lib.load().pdr_group_build(
            d["feats"].data_ptr() if Cs else None, Cs, d["xyz"].data_ptr(), d["new_xyz"].data_ptr(), d["idx"].data_ptr(),
            None if mode == "nocounts" else d["counts"].data_ptr(), B, n, m, K, int(mode == "patch"), int(with_abs),
            int(with_centre), out.data_ptr(), ldo, _stream())
        what = "group_build B=%d n=%d m=%d K=%d Cs=%d %s abs=%d centre=%d pad=%d" % (B, n, m, K, Cs, mode, with_abs,
                                                                                  with_centre, pad)
        assert rc == _lib.PDR_OK, what
        got = out.cpu().numpy()
        want, cout = _group_build_ref(self.feats, self.xyz, self.new_xyz, self.idx, self.counts, mode == "patch",
                                      with_abs, with_centre, ldo)
        assert cout == Cout
        _assert_bits(got[:rows], want, what)                  # features, geometry AND the zero padding columns
        _assert_untouched(got[rows:], what + " guard rows")
        return got[:rows]


_ALL_FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("B,n,m,K", [(1, 1, 1, 1), (3, 100, 37, 8), (2, 64, 16, 32)])
@pytest.mark.parametrize("Cs", [0, 7, 8, 39, 40, 131])
def test_group_build_equals_its_definition(cuda, Cs, B, n, m, K):
    """Lane widths 16 / 32 / 64 on both sides of their boundaries (row widths 16 | 17 and 48 | 49 with abs + centre),
    all four (abs, centre) combinations at Cs = 0 and 8, 0 / 1 / 3 / 8 padding columns, patched and unpatched empty
    balls and NULL counts, ragged position counts: bit-equal."""
    inp = _GroupInputs(cuda, B, n, m, K, Cs, seed=1000 * Cs + B * m * K)
    for with_abs, with_centre in (_ALL_FLAGS if Cs in (0, 8) else [(1, 1)]):
        for pad in (0, 1, 3, 8):
            for mode in ("patch", "nopatch", "nocounts"):
                inp.run(mode, with_abs, with_centre, pad)


def test_group_build_patches_exactly_the_empty_balls(cuda):
    """patch_empty = 1: zero feature, rel = 0, abs = centre in every slot of a ball with count 0; patch_empty = 0 with
    the same counts: no patch -- stated on the output itself, next to the reference comparison of run()."""
    inp = _GroupInputs(cuda, 3, 100, 37, 8, 8, seed=5)
    K, Cs = inp.K, inp.Cs
    empty = np.repeat(inp.counts.reshape(-1) <= 0, K)
    assert 0.2 < empty.mean() < 0.5
    ctr = np.repeat(inp.new_xyz.reshape(-1, 3), K, axis=0)
    got = inp.run("patch", 1, 1, 3)
    assert (got[empty, :Cs] == 0).all() and (got[empty, Cs:Cs + 3] == 0).all()
    assert np.array_equal(got[empty, Cs + 3:Cs + 6], ctr[empty]) and np.array_equal(got[:, Cs + 6:Cs + 9], ctr)
    raw = inp.run("nopatch", 1, 1, 3)
    assert np.array_equal(raw, inp.run("nocounts", 1, 1, 3))
    assert np.array_equal(raw[~empty], got[~empty]) and (raw[empty, :Cs] != 0).all()


@pytest.mark.parametrize("B,m,K,Cs,lanes", [(3, 6000, 32, 0, 16), (2, 2100, 32, 40, 64)])
def test_group_build_grid_stride_second_pass(cuda, B, m, K, Cs, lanes):
    """The launch is capped at 32768 workgroups of 256 / lanes positions: these are the smallest position counts at
    which the grid-stride loop of the 16- and of the 64-lane form iterates twice."""
    assert B * m * K > 32768 * (256 // lanes)
    inp = _GroupInputs(cuda, B, 257, m, K, Cs, seed=B + m)
    inp.run("patch", 1, 1, 3)


@pytest.mark.parametrize("with_abs,with_centre", _ALL_FLAGS)
def test_group_build_channel_order_is_query_and_group(cuda, with_abs, with_centre):
    """QueryAndGroup (pointnet2_utils.py) with subset=False on the same ball query, permuted to channel-last, is
    pdr_group_build bit for bit: [features | rel | (abs) | (centre)], empty balls patched."""
    B, n, m, K, Cs, r = 2, 100, 37, 8, 5, 0.35
    g = torch.Generator().manual_seed(11)
    xyz = (torch.rand(B, n, 3, generator=g) * 2 - 1).to(cuda)
    new_xyz = (torch.rand(B, m, 3, generator=g) * 2 - 1).to(cuda)
    feats = torch.randn(B, Cs, n, generator=g).to(cuda)                 # channel-first, as the module takes it
    qg = PU.QueryAndGroup(r, K, include_abs_coordinate=bool(with_abs), include_center_coordinate=bool(with_centre))
    want = qg(xyz, new_xyz, feats, subset=False).permute(0, 2, 3, 1).reshape(B * m * K, -1).cpu().numpy()
    idx, counts = PU.ball_query(r, K, xyz, new_xyz)
    nempty = int((counts <= 0).sum())
    assert 0 < nempty < B * m, "the radius should leave some balls empty and some not"
    Cout = Cs + 3 + 3 * with_abs + 3 * with_centre
    assert want.shape[1] == Cout
    out = _sentinel(B * m * K, Cout + 1, cuda)
    feats_cl = feats.transpose(1, 2).contiguous()
    idx, counts = idx.int().contiguous(), counts.int().contiguous()
    rc = _lib.load().pdr_group_build(feats_cl.data_ptr(), Cs, xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr(),
                                     counts.data_ptr(), B, n, m, K, 1, with_abs, with_centre, out.data_ptr(), Cout + 1,
                                     _stream())
    assert rc == _lib.PDR_OK
    got = out.cpu().numpy()
    _assert_bits(got[:B * m * K, :Cout], want, "group_build vs QueryAndGroup abs=%d centre=%d" % (with_abs, with_centre))
    assert (got[:B * m * K, Cout] == 0).all()
    _assert_untouched(got[B * m * K:], "guard rows")


# ---------------------------------------------------------------------------------------------------------------------
# pdr_knn_build
# ---------------------------------------------------------------------------------------------------------------------

def _knn_search(x, y, K):
    """Brute-force K nearest (float32 squared distances, ascending, lower index first): in-range int64 indices."""
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1, dtype=F32)
    idx = np.argsort(d, axis=2, kind="stable")[:, :, :K]
    return np.take_along_axis(d, idx, 2).astype(F32), idx.astype(np.int64)


def _knn_build_ref(feats, x, y, idx, d2, ldo):
    """[feats[idx] | d2 | w | y[idx] | y[idx] - x | x | 0 ...] in float32, the weight in the kernel's order: a
    sequential norm += 1 / (d2_k + 1e-8) over k, then (1 / (d2 + 1e-8)) / norm.  Also the float64 weights."""
    B, n1, K = idx.shape
    bi = np.arange(B)[:, None, None]
    ab = y[bi, idx]
    xq = np.broadcast_to(x[:, :, None, :], ab.shape)
    eps, one = F32(1e-8), F32(1)
    norm = np.zeros((B, n1), F32)
    for k in range(K):
        norm = norm + one / (d2[:, :, k] + eps)
    w = (one / (d2 + eps)) / norm[:, :, None]
    r64 = 1.0 / (d2.astype(np.float64) + np.float64(eps))
    w64 = r64 / r64.sum(2, keepdims=True)
    f = feats[bi, idx] if feats is not None else np.zeros((B, n1, K, 0), F32)
    G = np.concatenate([f, d2[..., None], w[..., None], ab, ab - xq, xq], axis=-1).reshape(B * n1 * K, -1).astype(F32)
    out = np.zeros((B * n1 * K, ldo), F32)
    out[:, :G.shape[1]] = G
    return out, w64.reshape(-1)


class _KnnInputs:
    def __init__(self, cuda, B, n1, n2, K, C, seed):
        assert K <= n2
        rng = np.random.default_rng(seed)
        self.B, self.n1, self.n2, self.K, self.C, self.cuda = B, n1, n2, K, C, cuda
        self.y = rng.uniform(-1, 1, (B, n2, 3)).astype(F32)
        self.x = rng.uniform(-1, 1, (B, n1, 3)).astype(F32)
        ncopy = min(n1, n2) // 3 + 1
        self.x[:, :ncopy] = self.y[:, :ncopy]                 # exact zero distances: the 1e-8 term carries the weight
        self.feats = rng.standard_normal((B, n2, C)).astype(F32) if C else None
        self.d2, self.idx = _knn_search(self.x, self.y, K)
        assert (self.d2[:, :ncopy, 0] == 0).all() and self.idx.min() >= 0 and self.idx.max() < n2
        self.d = {k: _dev(getattr(self, k), cuda) for k in ("x", "y", "idx", "d2")}
        self.d["feats"] = _dev(self.feats, cuda) if C else None

    def run(self, pad):
        B, n1, n2, K, C = self.B, self.n1, self.n2, self.K, self.C
        Cout, rows = C + 11, B * n1 * K
        ldo = Cout + pad
        out = _sentinel(rows, ldo, self.cuda)
        d = self.d
        rc = _lib.load().pdr_knn_build(d["feats"].data_ptr() if C else None, C, d["x"].data_ptr(), d["y"].data_ptr(),
                                       d["idx"].data_ptr(), d["d2"].data_ptr(), B, n1, n2, K, out.data_ptr(), ldo,
                                       _stream())
        what = "knn_build B=%d n1=%d n2=%d K=%d C=%d pad=%d" % (B, n1, n2, K, C, pad)
        assert rc == _lib.PDR_OK, what
        got = out.cpu().numpy()
        want, w64 = _knn_build_ref(self.feats, self.x, self.y, self.idx, self.d2, ldo)
        _assert_untouched(got[rows:], what + " guard rows")
        pad_cols = got[:rows, Cout:]
        assert not np.isnan(pad_cols).any(), ("%s: padding columns %s of the %d were left unwritten"
                                              % (what, sorted(set(np.argwhere(np.isnan(pad_cols))[:, 1])), pad))
        rel = np.abs(got[:rows, C + 1].astype(np.float64) - w64) / w64
        print("%s: weight vs float64 max rel %.3g (bound %.3g)" % (what, rel.max(), (K + 3) * 2.0 ** -24))
        assert rel.max() <= (K + 3) * 2.0 ** -24, what
        _assert_bits(got[:rows], want, what)                  # every column, the weight and the zero padding included


@pytest.mark.parametrize("K", [1, 3, 8, 32])
@pytest.mark.parametrize("C", [0, 5, 6, 37, 38, 128])
def test_knn_build_equals_its_definition(cuda, C, K):
    """Row widths 16 | 17 and 48 | 49 (the lane-width boundaries) and 11 / 139, K = 1 .. 32, exact zero distances,
    0 / 1 / 3 / 5 / 8 padding columns at every width (8 of them at C = 0 and C = 5 need more padding lanes than the
    16-lane form has behind its 11 geometry lanes).  Copies and the one subtraction are bit-equal; so is the weight
    column: the device's fp32 division is correctly rounded and the library is built without contraction, hence
    a float32 numpy evaluation in the kernel's order -- sequential norm over k, then (1 / (d2 + 1e-8)) / norm --
    reproduces its bits.  (The weaker statement |w - w64| <= (K + 3) 2^-24 w64, K additions and three roundings, is
    asserted as well.)"""
    inp = _KnnInputs(cuda, 2, 37, 45, K, C, seed=100 * C + K)
    for pad in (0, 1, 3, 5, 8):
        inp.run(pad)


def test_knn_build_grid_stride_second_pass(cuda):
    """More than 32768 x 16 positions in the 16-lane form (row width 16), with the widest padding."""
    inp = _KnnInputs(cuda, 3, 6000, 40, 32, 5, seed=77)
    assert inp.B * inp.n1 * inp.K > 32768 * 16
    inp.run(8)


@pytest.mark.parametrize("K", [3, 8])
def test_knn_build_channel_order_is_group_knn(cuda, K):
    """group_knn (pointnet2_utils.py) on the same clouds: features, d2 and the nine geometry columns bit-equal, the
    weights (torch sums the K reciprocals in its own order) within (K + 3) 2^-24 relative."""
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    B, n1, n2, C = 2, 37, 45, 6
    g = torch.Generator().manual_seed(13)
    y = (torch.rand(B, n2, 3, generator=g) * 2 - 1)
    x = (torch.rand(B, n1, 3, generator=g) * 2 - 1)
    x[:, :9] = y[:, :9]
    feats = torch.randn(B, n2, C, generator=g)
    x, y, feats = x.to(cuda), y.to(cuda), feats.to(cuda)
    want = PU.group_knn(x, y, feats, K).reshape(B * n1 * K, C + 11).cpu().numpy()
    d2, idx, _ = _ext.knn_points(x, y, K)
    d2, idx = d2.contiguous(), idx.long().contiguous()
    assert int(idx.min()) >= 0 and int(idx.max()) < n2
    rows = B * n1 * K
    out = _sentinel(rows, C + 11, cuda)
    rc = _lib.load().pdr_knn_build(feats.data_ptr(), C, x.data_ptr(), y.data_ptr(), idx.data_ptr(), d2.data_ptr(), B, n1,
                                   n2, K, out.data_ptr(), C + 11, _stream())
    assert rc == _lib.PDR_OK
    got = out.cpu().numpy()
    geo = [c for c in range(C + 11) if c != C + 1]
    _assert_bits(got[:rows][:, geo], want[:, geo], "knn_build vs group_knn K=%d" % K)
    w, ww = got[:rows, C + 1].astype(np.float64), want[:, C + 1].astype(np.float64)
    rel = np.abs(w - ww) / ww
    print("knn_build vs group_knn K=%d: weight max rel %.3g (bound %.3g)" % (K, rel.max(), (K + 3) * 2.0 ** -24))
    assert rel.max() <= (K + 3) * 2.0 ** -24
    _assert_untouched(got[rows:], "guard rows")


# ---------------------------------------------------------------------------------------------------------------------
# pdr_gather_rows / pdr_gather_rows2 / pdr_pad_rows
# ---------------------------------------------------------------------------------------------------------------------

def _row_indices(rng, B, n, m):
    idx = rng.integers(0, n, (B, m)).astype(np.int32)
    idx[:, 0], idx[:, -1] = 0, n - 1
    idx[:, 1:4] = idx[:, 4:5]                                  # repeats
    return idx


@pytest.mark.parametrize("C", [1, 3, 35, 128])
def test_gather_rows_equals_fancy_indexing(cuda, C):
    B, n, m = 3, 50, 37
    assert (B * m * C) % 256
    rng = np.random.default_rng(C)
    src = rng.standard_normal((B, n, C)).astype(F32)
    idx = _row_indices(rng, B, n, m)
    d_src, d_idx = _dev(src, cuda), _dev(idx, cuda)
    out = _sentinel(B * m, C, cuda)
    lib = _lib.load()
    assert lib.pdr_gather_rows(d_src.data_ptr(), d_idx.data_ptr(), B, n, C, m, out.data_ptr(), _stream()) == _lib.PDR_OK
    got = out.cpu().numpy()
    _assert_bits(got[:B * m], src[np.arange(B)[:, None], idx].reshape(B * m, C), "gather_rows C=%d" % C)
    _assert_untouched(got[B * m:], "gather_rows guard rows")
    out.fill_(float("nan"))
    assert lib.pdr_gather_rows(d_src.data_ptr(), d_idx.data_ptr(), B, n, C, 0, out.data_ptr(), _stream()) == _lib.PDR_OK
    _assert_untouched(out.cpu().numpy(), "gather_rows m=0")


@pytest.mark.parametrize("C0,C1", [(1, 3), (3, 128), (35, 1)])
def test_gather_rows2_equals_cat_then_fancy_indexing(cuda, C0, C1):
    B, n, m = 3, 50, 37
    C = C0 + C1
    assert (B * m * C) % 256
    rng = np.random.default_rng(10 * C0 + C1)
    a = rng.standard_normal((B, n, C0)).astype(F32)
    b = rng.standard_normal((B, n, C1)).astype(F32)
    idx = _row_indices(rng, B, n, m)
    d_a, d_b, d_idx = _dev(a, cuda), _dev(b, cuda), _dev(idx, cuda)
    out = _sentinel(B * m, C, cuda)
    lib = _lib.load()
    call = lambda mm: lib.pdr_gather_rows2(d_a.data_ptr(), C0, d_b.data_ptr(), C1, d_idx.data_ptr(), B, n, mm,
                                           out.data_ptr(), _stream())
    assert call(m) == _lib.PDR_OK
    got = out.cpu().numpy()
    want = np.concatenate([a, b], axis=2)[np.arange(B)[:, None], idx].reshape(B * m, C)
    _assert_bits(got[:B * m], want, "gather_rows2 C0=%d C1=%d" % (C0, C1))
    _assert_untouched(got[B * m:], "gather_rows2 guard rows")
    out.fill_(float("nan"))
    assert call(0) == _lib.PDR_OK
    _assert_untouched(out.cpu().numpy(), "gather_rows2 m=0")


@pytest.mark.parametrize("pad", [0, 1, 3, 13])
@pytest.mark.parametrize("C", [1, 3, 35, 128])
def test_pad_rows_equals_zero_padding(cuda, C, pad):
    rows, ldo = 111, C + pad
    rng = np.random.default_rng(C + pad)
    src = rng.standard_normal((rows, C)).astype(F32)
    d_src = _dev(src, cuda)
    out = _sentinel(rows, ldo, cuda)
    lib = _lib.load()
    assert lib.pdr_pad_rows(d_src.data_ptr(), rows, C, out.data_ptr(), ldo, _stream()) == _lib.PDR_OK
    got = out.cpu().numpy()
    _assert_bits(got[:rows], np.pad(src, ((0, 0), (0, pad))), "pad_rows C=%d pad=%d" % (C, pad))
    _assert_untouched(got[rows:], "pad_rows guard rows")
    out.fill_(float("nan"))
    assert lib.pdr_pad_rows(d_src.data_ptr(), 0, C, out.data_ptr(), ldo, _stream()) == _lib.PDR_OK
    _assert_untouched(out.cpu().numpy(), "pad_rows rows=0")


# ---------------------------------------------------------------------------------------------------------------------
# pdr_apply_act / pdr_act_colmax
# ---------------------------------------------------------------------------------------------------------------------

_SCALES = np.array([-1, -0.5, -0.25, 0.25, 0.5, 1, 2], F32)


def _dyadic(rng, shape):
    """multiples of 1/64 in [-8, 8]: with scales in {+-1/4, +-1/2, +-1, 2} every fp32 operation of the prologue is exact"""
    return (rng.integers(-512, 513, shape) / 64.0).astype(F32)


class _ActCase:
    """A pdr_layer_in_t over plain segments, with its float64 evaluation.

    segs: (C, column offset, ld, row_div) per segment; position p reads row p // row_div of the segment's table.  The
    tables, scale / shift (ld ss_ld, 0 = dense), add (ld add_ld) and the residual (column offset 2, ld C + 5) hold
    dyadic values (exact arithmetic) or normal random ones."""

    def __init__(self, cuda, B, rpb, segs, dyadic=True, ss_ld=0, add_ld=0, seed=0):
        rng = np.random.default_rng(seed)
        draw = (lambda s: _dyadic(rng, s)) if dyadic else (lambda s: rng.standard_normal(s).astype(F32))
        self.cuda, self.B, self.rpb, self.P, self.segs = cuda, B, rpb, B * rpb, segs
        self.C = C = sum(s[0] for s in segs)
        self.ss_ld, self.add_ld = ss_ld, add_ld or C
        P = self.P
        self.tables = [draw(((P + div - 1) // div, ld)) for (_, _, ld, div) in segs]
        self.x = np.concatenate([t[np.arange(P) // div, off:off + c] for t, (c, off, ld, div) in zip(self.tables, segs)],
                                axis=1)
        ssw = ss_ld or C
        self.scale = (rng.choice(_SCALES, (B, ssw)) if dyadic else rng.standard_normal((B, ssw))).astype(F32)
        self.shift, self.add = draw((B, ssw)), draw((B, self.add_ld))
        self.res = draw((P, C + 5))
        self.d = {"tables": [_dev(t, cuda) for t in self.tables]}
        for k in ("scale", "shift", "add", "res"):
            self.d[k] = _dev(getattr(self, k), cuda)

    def struct(self, pre, post, scale=True, shift=True, add=True, res=False):
        li = _lib.LayerIn()
        li.n_seg = len(self.segs)
        for i, (t, (c, off, ld, div)) in enumerate(zip(self.d["tables"], self.segs)):
            li.seg[i].ptr, li.seg[i].C, li.seg[i].ld, li.seg[i].row_div = t.data_ptr() + 4 * off, c, ld, div
        li.scale = self.d["scale"].data_ptr() if scale else None
        li.shift = self.d["shift"].data_ptr() if shift else None
        li.ss_ld = self.ss_ld
        if add:
            li.add, li.add_ld = self.d["add"].data_ptr(), self.add_ld
        if res:
            # the kernel reads rseg.ptr[row * ld + c] over all C columns: C and row_div of rseg are not consulted
            li.rseg.ptr, li.rseg.ld = self.d["res"].data_ptr() + 4 * 2, self.C + 5
            li.rseg.C, li.rseg.row_div = (1, 8) if res == "odd" else (self.C, 1)
        li.pre_relu, li.post_relu, li.rows_per_batch = int(pre), int(post), self.rpb
        return li

    def terms(self, pre, post, scale=True, shift=True, add=True, res=False):
        """float64: (post(pre(x) s + h) + add + residual, the magnitude sum |pre(x) s| + |h| + |add| + |res|)"""
        C = self.C
        b = np.arange(self.P) // self.rpb
        x = self.x.astype(np.float64)
        x = np.maximum(x, 0) if pre else x
        s = self.scale[b, :C].astype(np.float64) if scale else 1.0
        h = self.shift[b, :C].astype(np.float64) if shift else 0.0
        a = self.add[b, :C].astype(np.float64) if add else 0.0
        r = self.res[:, 2:2 + C].astype(np.float64) if res else 0.0
        v = x * s + h
        v = np.maximum(v, 0) if post else v
        return v + a + r, np.abs(x * s) + np.abs(h) + np.abs(a) + np.abs(r)

    def apply(self, ldo, **kw):
        P, C = self.P, self.C
        li = self.struct(**kw)
        out = _sentinel(P, ldo, self.cuda)
        rc = _lib.load().pdr_apply_act(ctypes.byref(li), P, C, out.data_ptr(), ldo, _stream())
        what = "apply_act B=%d rpb=%d segs=%s ss_ld=%d ldo=%d %s" % (self.B, self.rpb, self.segs, self.ss_ld, ldo, kw)
        assert rc == _lib.PDR_OK, what
        got = out.cpu().numpy()
        _assert_untouched(got[P:], what + " guard rows")
        _assert_untouched(got[:P, C:], what + " columns [C, ldo)")
        return got[:P, :C], what

    def colmax(self, **kw):
        B, C = self.B, self.C
        li = self.struct(**kw)
        out = _sentinel(B, C, self.cuda)
        rc = _lib.load().pdr_act_colmax(ctypes.byref(li), self.P, C, out.data_ptr(), _stream())
        what = "act_colmax B=%d rpb=%d segs=%s %s" % (B, self.rpb, self.segs, kw)
        assert rc == _lib.PDR_OK, what
        got = out.cpu().numpy()
        _assert_untouched(got[B:], what + " guard rows")
        return got[:B], what


_PRE_POST = [(0, 0), (0, 1), (1, 0), (1, 1)]
# (B, rows_per_batch, segments (C, column offset, ld, row_div), ss_ld, add_ld): 1, 2 and 4 segments at non-zero
# column offsets with ld > C, broadcast segments (row_div 8 / 32) next to plain ones, dense and strided scale / shift and
# add rows, B = 3 with rows_per_batch no multiple of 256 / C (workgroups straddle clouds), P C no multiple of 256
_APPLY_CASES = [
    (3, 37, [(7, 3, 12, 1)], 0, 0),
    (3, 40, [(5, 2, 9, 8), (30, 1, 33, 1)], 38, 41),
    (3, 96, [(3, 1, 4, 32), (64, 4, 70, 1), (1, 2, 3, 1), (13, 5, 20, 8)], 0, 90),
]


@pytest.mark.parametrize("case", range(len(_APPLY_CASES)))
def test_apply_act_is_exact_on_dyadic_operands(cuda, case):
    """x, shift, add, residual multiples of 1/64 in [-8, 8] and scale in {+-1/4, +-1/2, +-1, 2}: every fp32 operation of
    post(pre(x) s + h) + add + residual is exact, so the kernel must reproduce the float64 evaluation bit for bit --
    all four ReLU placements, add / residual present and absent, scale / shift NULL, ldo = C and ldo > C."""
    B, rpb, segs, ss_ld, add_ld = _APPLY_CASES[case]
    ac = _ActCase(cuda, B, rpb, segs, dyadic=True, ss_ld=ss_ld, add_ld=add_ld, seed=case)
    assert (ac.P * ac.C) % 256 and (rpb * ac.C) % 256          # a ragged last workgroup; workgroups straddle clouds
    variants = [dict(pre=p, post=q, add=a, res=r) for p, q in _PRE_POST for a in (True, False) for r in (True, False)]
    variants += [dict(pre=0, post=1, scale=False), dict(pre=1, post=0, shift=False),
                 dict(pre=0, post=0, scale=False, shift=False, add=False), dict(pre=0, post=1, res="odd")]
    for i, kw in enumerate(variants):
        got, what = ac.apply(ac.C + (3 if i % 4 else 0), **kw)
        want, _ = ac.terms(**kw)
        assert np.array_equal(want.astype(F32).astype(np.float64), want), "the dyadic case is not exact in fp32"
        _assert_bits(got, want.astype(F32), what)


def test_apply_act_general_values_within_three_roundings(cuda):
    """Normal random operands: |got - want64| <= 4 * 2^-24 * (|pre(x) s| + |h| + |add| + |res|) elementwise -- the fused
    multiply-add and the two additions round once each (3 * 2^-24 of the largest partial sum, which the magnitude sum
    bounds), with a margin of one."""
    B, rpb, segs, ss_ld, add_ld = _APPLY_CASES[1]
    ac = _ActCase(cuda, B, rpb, segs, dyadic=False, ss_ld=ss_ld, add_ld=add_ld, seed=9)
    for pre, post in _PRE_POST:
        kw = dict(pre=pre, post=post, add=True, res=True)
        got, what = ac.apply(ac.C + 3, **kw)
        want, mag = ac.terms(**kw)
        err = np.abs(got.astype(np.float64) - want)
        print("%s: max err / (2^-24 magnitude) = %.3f" % (what, float((err / (2.0 ** -24 * mag)).max())))
        assert (err <= 4 * 2.0 ** -24 * mag).all(), what


def _colmax_want(ac, **kw):
    want, _ = ac.terms(**kw)
    want = want.reshape(ac.B, ac.rpb, ac.C).max(axis=1)
    assert np.array_equal(want.astype(F32).astype(np.float64), want)
    return want.astype(F32)


@pytest.mark.parametrize("C", [3, 64, 65, 200])
@pytest.mark.parametrize("rpb", [1, 3, 5, 16, 17, 100, 1024])
def test_act_colmax_is_the_exact_column_maximum(cuda, rpb, C):
    """Dyadic operands (exact prologue), B = 3: the maximum over the rows of every cloud, bit-equal to float64 -- fewer
    rows than the kernel's 4 row slices x 4 loads, a clamped tail, many rows; one segment and two with a broadcast one
    (row_div 8); add present and absent; and columns that are negative in EVERY row (post_relu = 0, no add), whose
    maximum is that negative value and not 0."""
    B = 3
    one = _ActCase(cuda, B, rpb, [(C, 3, C + 5, 1)], ss_ld=C + 2, add_ld=C + 1, seed=rpb * 1000 + C)
    c0 = C // 3
    two = _ActCase(cuda, B, rpb, [(c0, 1, c0 + 2, 8), (C - c0, 2, C + 3, 1)], seed=rpb * 1000 + C + 1)
    for ac in (one, two):
        # |x s| <= 16: a shift of -20 makes the columns 0, C // 2 and C - 1 negative in every row
        neg = sorted({0, C // 2, C - 1})
        ac.shift[:, neg] = -20
        ac.d["shift"] = _dev(ac.shift, cuda)
        for pre, post in _PRE_POST:
            for add in (True, False):
                kw = dict(pre=pre, post=post, add=add)
                got, what = ac.colmax(**kw)
                want = _colmax_want(ac, **kw)
                _assert_bits(got, want, what)
                if not post and not add:
                    assert (got[:, neg] < 0).all(), what + ": an all-negative column must keep its negative maximum"
