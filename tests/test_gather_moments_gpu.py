"""pdr_gather_moments / _tiles / _tiles_twin (csrc/fused_gather.hip): the statistics-only pass of a virtual first conv
over the column windows [first C1 | . | key C2] of a [first | residual | key] output.  Reference: the EXISTING
pdr_gather_add / _tiles / _tiles_twin with Y = NULL on the same inputs -- bit-equal on the windows' columns -- and a
float64 numpy evaluation of the moments of U[a] + V[i] + d2 r1 + w r2 at the tolerance test_fused_gpu.py uses for
pdr_gather_add's moments (1e-4 (|m| + 1)).  Every case prefills `partial` with a finite sentinel and checks that the
residual window's entries (and every entry of a skipped tile) still hold it."""
import numpy as np
import pytest
import torch

from tests.golden.det_weights import fill_deterministic
from tests.golden.tiny_config import small_fused_config

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2 import fused_network as FN
from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Case:
    """Seeded inputs of one launch: tables U (B n_src + 1, ld), [V | V0] (B m, 2 ld), random indices in [0, n_src),
    the kNN scalars / rows or the ball counts (a third of them zero)."""

    def __init__(self, dev, B, n_src, m, K, cols, form, seed):
        self.B, self.n_src, self.m, self.K, self.form = B, n_src, m, K, form
        C1, Clast, C2 = cols
        self.cols, self.Cout, self.relu_col0 = cols, C1 + Clast + C2, C1 + Clast
        self.windows = (0, C1, C1 + Clast, C2)                      # win0_col0, win0_cols, win1_col0, win1_cols
        self.rpb = m * K
        self.tpb = (self.rpb + 127) // 128
        ld = self.ld = (self.Cout + 3) // 4 * 4
        g = torch.Generator(device=dev).manual_seed(seed)
        P = B * self.rpb
        self.U = torch.randn(B * n_src + 1, ld, device=dev, generator=g)
        self.V2 = torch.randn(B * m, 2 * ld, device=dev, generator=g)
        self.idx = torch.randint(0, n_src, (P,), device=dev, dtype=torch.int32, generator=g)
        knn = form == "knn"
        self.s1 = torch.rand(P, device=dev, generator=g) if knn else None
        self.s2 = torch.rand(P, device=dev, generator=g) if knn else None
        self.r1 = torch.randn(ld + 4, device=dev, generator=g) if knn else None
        self.r2 = torch.randn(ld + 4, device=dev, generator=g) if knn else None
        self.counts = None
        if not knn:
            self.counts = torch.randint(1, 5, (B * m,), device=dev, dtype=torch.int32, generator=g)
            self.counts[torch.arange(B * m, device=dev) % 3 == 1] = 0                       # a third: empty balls

    def head(self):
        """The arguments every entry point starts with, through Cout."""
        has_em = self.counts is not None
        return (self.U.data_ptr(), self.ld, self.n_src, self.V2.data_ptr(),
                self.V2.data_ptr() + 4 * self.ld if has_em else None, 2 * self.ld, self.idx.data_ptr(), _ptr(self.counts))

    def knn_args(self):
        return (_ptr(self.s1), _ptr(self.r1), _ptr(self.s2), _ptr(self.r2))

    def rows64(self, idx=None, K=None):
        """float64 numpy rows of the conv output (P, Cout): U[a] + V[i] + d2 r1 + w r2, empty ball -> V0[i]."""
        K = self.K if K is None else K
        idx = (self.idx if idx is None else idx).cpu().numpy().astype(np.int64).reshape(-1)
        P, C, ld = idx.shape[0], self.Cout, self.ld
        rpb = P // self.B
        b, q = np.arange(P) // rpb, np.arange(P) // K
        U, V2 = self.U.double().cpu().numpy(), self.V2.double().cpu().numpy()
        y = U[b * self.n_src + idx, :C] + V2[q, :C]
        if self.s1 is not None:
            y = y + self.s1.double().cpu().numpy()[:, None] * self.r1.double().cpu().numpy()[None, :C]
            y = y + self.s2.double().cpu().numpy()[:, None] * self.r2.double().cpu().numpy()[None, :C]
        if self.counts is not None:
            y = np.where((self.counts.cpu().numpy()[q] <= 0)[:, None], V2[q, ld:ld + C], y)
        return y

    def moments64(self):
        """float64 per-tile moments (B, tpb, Cout, 2), ReLU from relu_col0 on; a cloud's last tile may be ragged."""
        f = self.rows64()
        f[:, self.relu_col0:] = np.maximum(f[:, self.relu_col0:], 0)
        f = f.reshape(self.B, self.rpb, self.Cout)
        out = np.zeros((self.B, self.tpb, self.Cout, 2))
        for t in range(self.tpb):
            blk = f[:, t * 128:(t + 1) * 128]
            out[:, t, :, 0], out[:, t, :, 1] = blk.sum(1), (blk * blk).sum(1)
        return out

    def in_windows(self):
        w = np.zeros(self.Cout, dtype=bool)
        w[self.windows[0]:self.windows[0] + self.windows[1]] = True
        w[self.windows[2]:self.windows[2] + self.windows[3]] = True
        return w


def _check(got, ref, case, rows=None, want64=None):
    """got / ref: (B ptpb, Cout, 2) of the new / the existing entry point, both prefilled with the sentinel.  Window
    columns bit-equal on every row; every other column still the sentinel; rows (a bool mask over the partial rows
    that the launch writes; None: all) -- the others hold the sentinel in every column; want64: float64 moments of the
    written rows."""
    w = torch.from_numpy(case.in_windows()).to(got.device)
    assert torch.equal(got[:, w], ref[:, w]), "window moments differ from pdr_gather_add's"
    assert bool((got[:, ~w] == SENTINEL).all()), "an entry outside the windows was written"
    if rows is not None:
        assert bool((got[~rows] == SENTINEL).all()), "a partial row of a skipped tile was written"
        assert not bool((got[rows][:, w] == SENTINEL).any())
    else:
        assert not bool((got[:, w] == SENTINEL).any())
    if want64 is not None:
        g = got.double().cpu().numpy()[:, case.in_windows()]
        wm = want64[:, case.in_windows()]
        if rows is not None:
            g, wm = g[rows.cpu().numpy()], wm[rows.cpu().numpy()]
        err = np.abs(g - wm) - 1e-4 * (np.abs(wm) + 1)
        print("max |moment - float64| / (|m| + 1) = %.2e" % float((np.abs(g - wm) / (np.abs(wm) + 1)).max()))
        assert (err <= 0).all()


def _plain(case, st):
    lib = _lib.load()
    shape = (case.B * case.tpb, case.Cout, 2)
    ref = torch.full(shape, SENTINEL, device=case.U.device)
    got = torch.full(shape, SENTINEL, device=case.U.device)
    tail = (case.B, case.rpb, case.K, case.Cout)
    _lib.check(lib.pdr_gather_add(*case.head(), *case.knn_args(), *tail, None, case.ld, ref.data_ptr(), case.relu_col0,
                                  0, -1, st), "gather_add")
    _lib.check(lib.pdr_gather_moments(*case.head(), *case.knn_args(), *tail, got.data_ptr(), case.relu_col0,
                                      *case.windows, st), "gather_moments")
    torch.cuda.synchronize()
    return got, ref


@pytest.mark.parametrize("cols", [(8, 8, 7), (64, 32, 43), (128, 128, 171)], ids=["lpr16", "lpr64_one_pass", "two_passes"])
def test_knn_form_k8(cuda, cols):
    """B = 3, n_src = 37, m = 40, K = 8: 320 rows per cloud = two full tiles + a 64-row tile.  (8, 8, 7): 16 lanes per
    row; (64, 32, 43): 64 lanes, one column pass; (128, 128, 171): two column passes on grid.y."""
    case = _Case(cuda, 3, 37, 40, 8, cols, "knn", 100 + sum(cols))
    got, ref = _plain(case, torch.cuda.current_stream().cuda_stream)
    _check(got, ref, case, want64=case.moments64().reshape(-1, case.Cout, 2))


def test_knn_form_k6_not_a_power_of_two(cuda):
    case = _Case(cuda, 2, 37, 50, 6, (16, 16, 9), "knn", 7)
    got, ref = _plain(case, torch.cuda.current_stream().cuda_stream)
    _check(got, ref, case, want64=case.moments64().reshape(-1, case.Cout, 2))


def test_one_window_only(cuda):
    """No extra convs: [first 64 | residual 64], only [0, 64) is walked."""
    case = _Case(cuda, 3, 37, 40, 8, (64, 64, 0), "knn", 11)
    assert case.windows[3] == 0
    got, ref = _plain(case, torch.cuda.current_stream().cuda_stream)
    _check(got, ref, case, want64=case.moments64().reshape(-1, case.Cout, 2))


@pytest.fixture(scope="module")
def ball(cuda):
    """Ball form, K = 32: B = 2, n_src = 50, m = 12 -> 384 rows per cloud (three tiles), a third of the balls empty,
    columns (128, 128, 137); its float64 moments are computed once for the tests that share it."""
    case = _Case(cuda, 2, 50, 12, 32, (128, 128, 137), "ball", 32)
    assert int((case.counts == 0).sum()) == case.B * case.m // 3
    return case, case.moments64()


def test_ball_form_k32(cuda, ball):
    case, want = ball
    got, ref = _plain(case, torch.cuda.current_stream().cuda_stream)
    _check(got, ref, case, want64=want.reshape(-1, case.Cout, 2))


def _subset(case):
    """tile_valid that clears one tile per cloud (the second of the first cloud, the third of the other) and
    partial_tpb = 5 > the 3 tiles (+ 1 twin tile) per cloud -> (tile_valid, ptpb, written main partial rows)."""
    tv = torch.ones(case.B, case.tpb, dtype=torch.uint8, device=case.U.device)
    tv[0, 1], tv[1, 2] = 0, 0
    ptpb = 5
    rows = torch.zeros(case.B, ptpb, dtype=torch.bool, device=case.U.device)
    rows[:, :case.tpb] = tv.bool()
    return tv.reshape(-1).contiguous(), ptpb, rows


def test_ball_form_tile_subset(cuda, ball):
    case, want = ball
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    tv, ptpb, rows = _subset(case)
    shape = (case.B * ptpb, case.Cout, 2)
    ref, got = torch.full(shape, SENTINEL, device=cuda), torch.full(shape, SENTINEL, device=cuda)
    tail = (case.B, case.rpb, case.K, case.Cout)
    _lib.check(lib.pdr_gather_add_tiles(*case.head(), None, None, None, None, *tail, None, case.ld, ref.data_ptr(),
                                        case.relu_col0, 0, -1, tv.data_ptr(), ptpb, st), "gather_add_tiles")
    _lib.check(lib.pdr_gather_moments_tiles(*case.head(), None, None, None, None, *tail, got.data_ptr(), case.relu_col0,
                                            *case.windows, tv.data_ptr(), ptpb, st), "gather_moments_tiles")
    torch.cuda.synchronize()
    want5 = np.zeros((case.B, ptpb, case.Cout, 2))
    want5[:, :case.tpb] = want
    _check(got, ref, case, rows=rows.reshape(-1), want64=want5.reshape(-1, case.Cout, 2))


def test_twin_form(cuda, ball):
    """idx0 / wrow0 / wmul = K as SplitFirstConv passes them: Yd bit-equal to pdr_gather_add_tiles_twin's in every
    column, the main tiles' and the twin tile's moments bit-equal on the windows; the twin tile's moments are K x those
    of the per-query rows q >= wrow0[b] (float64)."""
    case, want = ball
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    tv, ptpb, rows = _subset(case)
    rows[:, case.tpb] = True                                          # the twin tile of every cloud (m = 12 queries)
    idx0 = case.idx.view(case.B, case.m, case.K)[:, :, 0].contiguous()
    wrow0 = torch.tensor([4, 9], dtype=torch.int32, device=cuda)
    shape = (case.B * ptpb, case.Cout, 2)
    ref, got = torch.full(shape, SENTINEL, device=cuda), torch.full(shape, SENTINEL, device=cuda)
    Yd_ref = torch.full((case.B * case.m, case.ld), SENTINEL, device=cuda)
    Yd = torch.full((case.B * case.m, case.ld), SENTINEL, device=cuda)
    tail = (case.B, case.rpb, case.K, case.Cout)
    _lib.check(lib.pdr_gather_add_tiles_twin(*case.head(), *tail, None, case.ld, ref.data_ptr(), case.relu_col0, 0, -1,
                                             tv.data_ptr(), ptpb, idx0.data_ptr(), Yd_ref.data_ptr(), case.ld,
                                             wrow0.data_ptr(), float(case.K), st), "gather_add_tiles_twin")
    _lib.check(lib.pdr_gather_moments_tiles_twin(*case.head(), *tail, got.data_ptr(), case.relu_col0, *case.windows,
                                                 tv.data_ptr(), ptpb, idx0.data_ptr(), Yd.data_ptr(), case.ld,
                                                 wrow0.data_ptr(), float(case.K), st), "gather_moments_tiles_twin")
    torch.cuda.synchronize()
    assert torch.equal(Yd, Yd_ref) and not bool((Yd[:, :case.Cout] == SENTINEL).any())
    # float64: main tiles as before; the twin tile = K x the moments of the per-query rows from wrow0[b] on
    yq = case.rows64(idx=idx0, K=1)
    np.testing.assert_allclose(Yd[:, :case.Cout].cpu().numpy(), yq, rtol=1e-6, atol=1e-6)
    yq[:, case.relu_col0:] = np.maximum(yq[:, case.relu_col0:], 0)
    yq = yq.reshape(case.B, case.m, case.Cout)
    want5 = np.zeros((case.B, ptpb, case.Cout, 2))
    want5[:, :case.tpb] = want
    for b in range(case.B):
        sel = yq[b, int(wrow0[b]):]
        want5[b, case.tpb, :, 0], want5[b, case.tpb, :, 1] = case.K * sel.sum(0), case.K * (sel * sel).sum(0)
    _check(got, ref, case, rows=rows.reshape(-1), want64=want5.reshape(-1, case.Cout, 2))


def test_argument_errors_launch_nothing():
    """Decided on the host: pointers are never dereferenced (no GPU needed for the codes themselves)."""
    lib = _lib.load()
    p, EINVAL, EUNSUP, OK = 0x1000, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED, _lib.PDR_OK

    def gm(win=(0, 64, 128, 43), partial=p, B=2, K=8, ldu=172, r1=p, U=p):
        return lib.pdr_gather_moments(U, ldu, 100, p, None, 172, p, None, p, r1, p, p, B, 256, K, 171, partial, 128,
                                      *win, None)
    assert gm(win=(0, 62, 130, 41)) == EUNSUP and gm(win=(2, 62, 128, 43)) == EUNSUP     # a start off a float4
    assert gm(win=(0, 64, 60, 43)) == EINVAL and gm(win=(128, 43, 0, 64)) == EINVAL       # overlapping, descending
    assert gm(win=(0, 64, 128, 44)) == EINVAL and gm(win=(0, 172, 0, 0)) == EINVAL        # past the last column
    assert gm(win=(-4, 64, 128, 43)) == EINVAL and gm(win=(0, 0, 128, 43)) == EINVAL and gm(win=(0, 64, 128, -1)) == EINVAL
    assert gm(partial=None) == EINVAL and gm(U=None) == EINVAL and gm(K=7) == EINVAL      # 256 rows, K = 7
    assert gm(ldu=170) == EINVAL and gm(r1=None) == EINVAL and gm(U=0x1004) == EINVAL
    assert gm(B=0) == OK and gm(win=(0, 64, 0, 0), B=0) == OK
    tiles = lambda tv=p, ptpb=2: lib.pdr_gather_moments_tiles(p, 172, 100, p, None, 172, p, None, None, None, None, None,
                                                              2, 256, 8, 171, p, 128, 0, 64, 128, 43, tv, ptpb, None)
    assert tiles(tv=None) == EINVAL and tiles(ptpb=1) == EINVAL
    tw = lambda **k: lib.pdr_gather_moments_tiles_twin(
        p, 172, 100, p, None, 172, p, None, 2, 256, 32, 171, k.get("partial", p), 128, *k.get("win", (0, 64, 128, 43)),
        k.get("tv", p), k.get("ptpb", 3), k.get("idx0", p), k.get("Yd", p), k.get("ldyd", 172), k.get("wrow0", p), 32.0,
        None)
    assert tw(tv=None) == EINVAL and tw(idx0=None) == EINVAL and tw(Yd=None) == EINVAL and tw(wrow0=None) == EINVAL
    assert tw(ptpb=2) == EINVAL and tw(ldyd=170) == EINVAL and tw(partial=None) == EINVAL
    assert tw(win=(0, 64, 126, 45)) == EUNSUP and tw(win=(0, 64, 32, 43)) == EINVAL


def test_small_network_is_bit_equal_with_and_without_moment_windows(cuda, monkeypatch):
    """The smallest fused forward of the suite (small_fused_config, B = 2, a cached call as test_fused_gpu.py's
    test_fused_network_small_config): MOMENT_WINDOWS on and off give torch.equal outputs, and `on` does go through the
    new entry points."""
    net = fill_deterministic(PointNet2CloudCondition(small_fused_config()), 21).eval().to(cuda)
    fused = FN.FusedCloudConditionNet(net)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 256, 3, generator=g).to(cuda)
    cond = torch.cat([torch.rand(2, 384, 3, generator=g) * 2 - 1, torch.ones(2, 384, 1)], 2).to(cuda)
    ts, label = torch.tensor([9.0, 4.0], device=cuda), torch.tensor([1, 7], device=cuda)
    lib = _lib.load()
    calls = {}
    for name in ("pdr_gather_moments", "pdr_gather_moments_tiles", "pdr_gather_moments_tiles_twin"):
        def counted(*a, _f=getattr(lib, name), _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    outs = {}
    with torch.no_grad():
        net.reset_cond_features()
        net(x, cond, ts=ts, label=label, use_retained_condition_feature=True)           # fills the cache
        fused.sync_condition()
        for on in (True, False):
            monkeypatch.setattr(FN, "MOMENT_WINDOWS", on)
            calls.clear()
            outs[on] = fused(x * 0.9, cond, ts=ts - 1, label=label, use_retained_condition_feature=True).clone()
            assert (sum(calls.values()) > 0) == on, calls
    assert torch.equal(outs[True], outs[False])
    assert bool(torch.isfinite(outs[True]).all())
