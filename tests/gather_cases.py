"""The dispatch table of the virtual first conv's gather kernel (csrc/fused_gather.hip: one body, gather_tile, behind
pdr_gather_add / _tiles / _tiles_twin and pdr_gather_moments / _tiles / _tiles_twin), the launches that walk it and the
inputs and float64 references those launches run on.  A plain module: tests/test_gather_dispatch_plan.py walks the list
through pdr_gather_plan on the host, tests/test_gather_dispatch_gpu.py runs every case.

A case is one launch.  Rows per cloud are two full 128-row tiles plus a ragged tail (344 = 32 / 32 / 24 / 0 rows in the
last tile's waves for K = 8, m = 43), B = 3 clouds of n_src = 37 source points unless the case is about something else.
Inputs are built so that the preconditions hold and are asserted, on the inputs and on the float64 reference (never on
kernel output): every cloud gathers source 0 and source n_src - 1, every wave with two queries holds an empty and a
non-empty ball, and both signs occur in every ReLU column of every tile:
    U[a, c] = (-1)^(a + c) (0.5 + |N(0, 1)|),   V, V0 ~ U(-0.25, 0.25),   s ~ U(0, 1),   r ~ 0.1 N(0, 1)
so the sign of a row is that of its source point's parity unless the ball is empty.

Bounds (u = 2^-24, float32 unit roundoff):
  Y, forms without s1 / s2: one float32 add -- bit-equal to numpy's float32 U + V, or to V0.
  Y, forms with s1 / s2: two FMAs and an add, <= 3 roundings: |Y - ref| <= 4 u (|U| + |V| + |s1 r1| + |s2 r2|).
  moments of a tile of n <= 128 rows (float32 sums in a fixed tree): |m1 - ref| <= (n + 4) u sum|y|,
  |m2 - ref| <= (n + 6) u sum y^2, both sums in float64 from the reference rows; twin tiles, one more rounding for
  wmul: (n + 5), (n + 7).
"""
import collections
import ctypes
import functools
import itertools
import os

import numpy as np

from point_diffusion_refinement_amd import _lib

U32 = 2.0 ** -24
SENTINEL = 12345.0
B, N_SRC = 3, 37
TM = 128

HAS_COUNTS, HAS_S1, HAS_S2, HAS_Y, HAS_PARTIAL, HAS_TILES, HAS_TWIN = 1, 2, 4, 8, 16, 32, 64
PLAN_FIELDS = ("lpr", "kpow2", "has_s", "has_em", "ywin", "stats", "shared", "shared_rows", "c0a", "na", "c0b", "nb",
               "w4", "passes", "grid_x", "grid_y", "n_main", "n_twin", "tpb", "twin_tpb", "ycol0", "y4", "tiles",
               "reserved")
Plan = collections.namedtuple("Plan", PLAN_FIELDS)

# entry point, B, n_src, m, K, Cout, form, out, relu_col0, windows (c0a, na, c0b, nb), tiles (None or "subset"),
# twin (None or (wrow0 per cloud, wmul)), same_clouds (every cloud a copy of the first)
Case = collections.namedtuple("Case", "entry B n_src m K Cout form out relu_col0 windows tiles twin same_clouds")

FORMS = ("ball_em", "ball", "knn", "knn_s1", "s_em")       # counts | - | s1 s2 | s1 | s1 s2 counts
OUTS = ("yp", "y", "p", "wp", "w")                          # Y + partial | Y | partial | Y window + partial | Y window
COUTS = {16: (7, 64), 32: (65, 128), 64: (129, 256, 257, 300)}
SHARED_ROWS = {16: 16, 32: 8, 64: 4}
M_OF_K = {1: 300, 2: 172, 4: 86, 8: 43, 16: 21, 32: 9, 3: 100, 6: 50, 64: 5}   # rows: 300 .. 344, a ragged third tile
K_DIV = (6, 64, 3)                                          # the division form: no power of two, or above 32


def lpr_of(Cout):
    return 16 if Cout <= 64 else 32 if Cout <= 128 else 64


def pad4(c):
    return (c + 3) // 4 * 4


def case_id(c):
    s = "%s-B%d-m%d-K%d-C%d-%s-%s-relu%d" % (c.entry, c.B, c.m, c.K, c.Cout, c.form, c.out, c.relu_col0)
    if c.entry.startswith("moments"):
        s += "-win%d_%d_%d_%d" % c.windows
    if c.twin:
        s += "-wrow" + "_".join(map(str, c.twin[0]))
    return s + ("-same" if c.same_clouds else "")


def _case(entry, K, Cout, form, out, relu_col0, m=None, Bc=B, n_src=N_SRC, windows=None, tiles=None, twin=None,
          same=False):
    return Case(entry, Bc, n_src, M_OF_K[K] if m is None else m, K, Cout, form, out, relu_col0,
                windows or (0, Cout, 0, 0), tiles, twin, same)


def relu_choices(Cout):
    """0 | inside a float4 piece | the first column of a second pass (where there is one) | >= Cout."""
    inside = 42 if Cout > 43 else 5
    return (0, inside, Cout + 3) + ((256,) if Cout > 256 else ())


def ywindow(c):
    """(ycol0, ycols, ldy) of the Y a case writes: the whole width, or a window with ycol0 > 0, ycols no multiple of 4
    and ldy beyond the padded window."""
    if "w" not in c.out:
        return 0, c.Cout, pad4(c.Cout)
    ycol0 = 4 if c.Cout < 16 else 8
    ycols = max(1, (c.Cout - ycol0) // 2)
    ycols -= ycols % 4 == 0
    return ycol0, ycols, pad4(ycols) + 4


# ------------------------------------------------------------------------------------------------- the list
def main_cases():
    """pdr_gather_add over lanes per row x {K at / above the shared threshold, below it, division form} x forms x
    outputs; the width, K and relu_col0 of a cell rotate through their lists."""
    cases, i = [], 0
    for lpr, kclass, form, out in itertools.product((16, 32, 64), ("shared", "row", "div"), FORMS, OUTS):
        thr = SHARED_ROWS[lpr]
        ks = {"shared": [k for k in (1, 2, 4, 8, 16, 32) if k >= thr], "row": [k for k in (1, 2, 4, 8, 16, 32) if k < thr],
              "div": list(K_DIV)}[kclass]
        # (thr first among the shared ones, thr / 2 last among the others: both sides of the threshold)
        K = ks[(i // 3) % len(ks)] if kclass != "row" else ks[::-1][(i // 3) % len(ks)]
        Cout = COUTS[lpr][i % len(COUTS[lpr])]
        rc = relu_choices(Cout)
        cases.append(_case("add", K, Cout, form, out, rc[(i // 2) % len(rc)]))
        i += 1
    return cases


def edge_cases():
    """Clouds shorter than a tile; the K = 1 Y-only launch of the network; the column passes walked inside the workgroup
    (more than 1024 tiles, more than 256 walked columns) with statistics, Y only and as a statistics-only pass, together
    with the same clouds on grid.y; relu_col0 on the first column of the second pass with both outputs."""
    tiny = [_case("add", 8, C, form, out, r, m=1) for C, form, out, r in
            [(64, "ball", "yp", 42), (128, "knn", "yp", 0), (257, "ball", "yp", 256), (300, "ball", "p", 42),
             (7, "ball", "y", 0)]]
    k1 = [_case("add", 1, C, "ball_em", "y", 0) for C in (64, 128, 300)]
    serial = []
    for Bc in (3, 1025):
        serial += [_case("add", 8, 260, "ball", "yp", 42, m=1, Bc=Bc, n_src=9, same=True),
                   _case("add", 8, 260, "ball", "y", 0, m=1, Bc=Bc, n_src=9, same=True),
                   _case("add", 2, 301, "knn", "p", 256, m=4, Bc=Bc, n_src=9, same=True),
                   _case("moments", 8, 301, "ball_em", "p", 256, m=2, Bc=Bc, n_src=9, same=True,
                         windows=(0, 254, 256, 45))]
    second = [_case("add", 8, C, form, out, 256) for C, form, out in
              [(257, "ball_em", "yp", ), (300, "knn", "yp"), (300, "ball", "p"), (257, "s_em", "p")]]
    return tiny + k1 + serial + second


MOMENT_WINDOWS = (
    # Cout, windows, relu_col0
    (63, (0, 16, 0, 0), 8),                  # one window
    (63, (0, 10, 32, 31), 32),               # first length no multiple of 4; win1 ends at Cout, Cout % 4 = 3
    (127, (32, 40, 0, 0), 42),               # one window, not from column 0
    (127, (0, 30, 64, 63), 64),
    (301, (0, 64, 0, 0), 0),
    (301, (0, 254, 256, 45), 256),           # 64 + 12 pieces: the windows lie in different passes
    (301, (0, 100, 200, 101), 150),          # one pass of 25 + 26 pieces; nothing before relu_col0 in window b
    (301, (0, 158, 164, 137), 166),          # 40 + 35 pieces: the first pass holds both windows, the second only b
)


def moment_cases():
    cases, i = [], 0
    ks = (8, 32, 1, 6, 64, 2, 16, 4, 3)
    for (Cout, win, relu), form in itertools.product(MOMENT_WINDOWS, FORMS):
        cases.append(_case("moments", ks[i % len(ks)], Cout, form, "p", relu, windows=win))
        i += 1
    return cases


def tile_cases():
    """Tile subsets: the first tile of cloud 0, the last (ragged) tile of cloud 1 and every tile of cloud 2 cleared,
    partial_tpb two rows larger than needed."""
    add = [_case("add_tiles", K, C, form, out, r, tiles="subset") for K, C, form, out, r in
           [(8, 64, "ball_em", "yp", 42), (6, 65, "knn", "yp", 0), (32, 300, "ball", "wp", 256), (1, 128, "s_em", "p", 42),
            (64, 257, "ball_em", "y", 0), (16, 7, "knn_s1", "yp", 5)]]
    mom = [_case("moments_tiles", K, C, form, "p", r, windows=w, tiles="subset") for K, C, form, r, w in
           [(8, 63, "ball_em", 32, (0, 10, 32, 31)), (6, 127, "knn", 64, (0, 30, 64, 63)),
            (32, 301, "ball", 256, (0, 254, 256, 45))]]
    return add + mom


def twin_cases():
    """Twin tiles behind a tile subset: every lanes-per-row, with and without counts, K = 32 / 8 / 6, m = 12 (one short
    twin tile) and m = 300 (three per cloud, the last of 44 rows); four clouds with wrow0 = 0, a tile boundary, inside
    a tile and m."""
    cases = []
    for (li, C), form, (ki, K), (mi, m) in itertools.product(enumerate((64, 128, 300)), ("ball_em", "ball"),
                                                            enumerate((32, 8, 6)), enumerate((12, 300))):
        wrow0 = (0, 5, 12, 7) if m == 12 else (0, 128, 200, 300)
        relu = relu_choices(C)[1 + (ki + mi) % 2 * (2 if C > 256 else 0)]
        kind = (ki + li + (form == "ball")) % 2 if mi else 2
        # a Y with partial beside the twin | no Y | the statistics-only pass over two windows
        if kind == 2:
            cases.append(_case("add_twin", K, C, form, "yp" if ki else "wp", relu, m=m, Bc=4, tiles="subset",
                               twin=(wrow0, float(K))))
        elif kind == 1:
            cases.append(_case("add_twin", K, C, form, "p", relu, m=m, Bc=4, tiles="subset", twin=(wrow0, float(K))))
        else:
            w = (0, C // 4 - 2, pad4(C // 2), C - pad4(C // 2))
            cases.append(_case("moments_twin", K, C, form, "p", w[2], m=m, Bc=4, tiles="subset", windows=w,
                               twin=(wrow0, float(K))))
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = main_cases() + edge_cases() + moment_cases() + tile_cases() + twin_cases()
    assert len(set(cases)) == len(cases)
    return tuple(cases)


def groups():
    """The cases in groups of a few dozen launches: one pytest item each."""
    out = collections.OrderedDict()
    for c in all_cases():
        if c.B > 1000:
            key = "serial"
        elif c.entry == "add" and c.tiles is None:
            key = "add-lpr%d-%s" % (lpr_of(c.Cout), c.form)
        else:
            key = "%s-lpr%d" % (c.entry, lpr_of(c.Cout))
        out.setdefault(key, []).append(c)
    return out


# ----------------------------------------------------------------------------------------------- the plan
def flags_of(c):
    f = 0
    if c.form in ("ball_em", "s_em"):
        f |= HAS_COUNTS
    if c.form in ("knn", "knn_s1", "s_em"):
        f |= HAS_S1
    if c.form in ("knn", "s_em"):
        f |= HAS_S2
    if c.out != "p":
        f |= HAS_Y
    if "p" in c.out:
        f |= HAS_PARTIAL
    if c.tiles:
        f |= HAS_TILES
    if c.twin:
        f |= HAS_TWIN
    return f


def tiles_per_cloud(c):
    return (c.m * c.K + TM - 1) // TM


def twin_tiles_per_cloud(c):
    return (c.m + TM - 1) // TM if c.twin else 0


def partial_tpb(c):
    """Rows of `partial` per cloud: the main tiles, the twin tiles behind them, and with a subset two rows to spare."""
    return tiles_per_cloud(c) + twin_tiles_per_cloud(c) + (2 if c.tiles else 0)


def plan_call(*args):
    """pdr_gather_plan(B, n_src, rows_per_batch, K, Cout, ldu, ldv, ldy, ycol0, ycols, win0_col0, win0_cols, win1_col0,
    win1_cols, partial_tpb, ldyd, flags) -> (rc, Plan)."""
    if not os.path.exists(_lib.LIB_PATH):      # the case lists are made at collection time, before any fixture runs
        import __graft_entry__
        __graft_entry__.build()
    out = (ctypes.c_int * 24)()
    rc = _lib.load().pdr_gather_plan(*args, out)
    return rc, Plan(*out)


def plan_args(c):
    ld = pad4(c.Cout)
    ycol0, ycols, ldy = ywindow(c)
    return (c.B, c.n_src, c.m * c.K, c.K, c.Cout, ld, 2 * ld, ldy, ycol0, ycols) + tuple(c.windows) + (
        partial_tpb(c) if c.tiles else 0, ld + 4 if c.twin else 0, flags_of(c))


def plan(c):
    return plan_call(*plan_args(c))


# ------------------------------------------------------------------------------------------------- inputs
def _seed(c):
    return [17, c.n_src, c.m, c.K, c.Cout, FORMS.index(c.form), len(c.entry), c.relu_col0]


def tile_valid(c):
    """(B, tpb) bytes: the first tile of cloud 0, the last tile of cloud 1 and every tile of cloud 2 cleared."""
    tv = np.ones((c.B, tiles_per_cloud(c)), dtype=np.uint8)
    tv[0, 0] = 0
    tv[1 % c.B, -1] = 0
    tv[2 % c.B, :] = 0
    return tv


@functools.lru_cache(maxsize=64)
def inputs(c):
    """The arrays of a launch, read-only: U (B n_src, ld), V2 = [V | V0] (B m, 2 ld), idx (B, m, K), counts (B, m) or
    None, s1 / s2 (B m K) and r1 / r2 (ld) or None."""
    r = np.random.default_rng(_seed(c))
    Bg = 1 if c.same_clouds else c.B                       # clouds generated; the others are copies
    ld = pad4(c.Cout)
    a, col = np.arange(c.n_src)[:, None], np.arange(ld)[None, :]
    sgn = (1 - 2 * ((a + col) % 2)).astype(np.float32)
    U = (sgn[None] * (0.5 + np.abs(r.standard_normal((Bg, c.n_src, ld))))).astype(np.float32)
    V2 = r.uniform(-0.25, 0.25, (Bg, c.m, 2 * ld)).astype(np.float32)
    idx = r.integers(0, c.n_src, (Bg, c.m, c.K)).astype(np.int32)
    counts = None
    if c.form in ("ball_em", "s_em"):
        q = np.arange(c.m)[None, :] + np.arange(Bg)[:, None]
        counts = np.where(q % 2 == 1, 0, r.integers(1, 5, (Bg, c.m))).astype(np.int32)
        if c.m == 1:
            counts[:] = 2                                   # a one-query cloud that is empty has no row to sign-check
    rpb = c.m * c.K
    for b in range(Bg):
        flat = idx[b].reshape(-1)
        for t in range(0, rpb, TM):                          # no tile of empty balls only: its rows would be one row
            if counts is not None and not (counts[b, t // c.K:(min(rpb, t + TM) - 1) // c.K + 1] > 0).any():
                counts[b, t // c.K] = 2
        even, odd = lambda: 2 * r.integers(0, (c.n_src + 1) // 2), lambda: 1 + 2 * r.integers(0, c.n_src // 2)
        liveq = np.ones(c.m, dtype=bool) if counts is None else counts[b] > 0
        live = np.repeat(liveq, c.K)
        if c.twin:                                           # the same among the first neighbours a twin tile counts
            for j in range(0, c.m, TM):
                qs = np.flatnonzero(liveq[j:j + TM]) + j
                qs = qs[qs >= c.twin[0][b]]
                if len(qs) >= 2:
                    idx[b, qs[0], 0], idx[b, qs[1], 0] = even(), odd()
        for t in range(0, rpb, TM):                          # a source of either parity (= sign) in every tile
            rows = t + np.flatnonzero(live[t:t + TM])
            rows = rows[rows % c.K != 0] if c.K > 1 else rows    # (not a first neighbour)
            if len(rows) >= 2:
                flat[rows[0]], flat[rows[1]] = even(), odd()
            if t == 0 and len(rows) >= 4:                    # both ends of the source range, in balls that are not empty
                flat[rows[2]], flat[rows[3]] = 0, c.n_src - 1
    has_s1, has_s2 = c.form in ("knn", "knn_s1", "s_em"), c.form in ("knn", "s_em")
    s1 = r.uniform(0, 1, (Bg, c.m * c.K)).astype(np.float32) if has_s1 else None
    s2 = r.uniform(0, 1, (Bg, c.m * c.K)).astype(np.float32) if has_s2 else None
    r1 = (0.1 * r.standard_normal(ld)).astype(np.float32) if has_s1 else None
    r2 = (0.1 * r.standard_normal(ld)).astype(np.float32) if has_s2 else None
    rep = lambda x: None if x is None else np.ascontiguousarray(np.repeat(x, c.B // Bg, axis=0))
    d = dict(U=rep(U), V2=rep(V2), idx=rep(idx), counts=rep(counts), s1=rep(s1), s2=rep(s2), r1=r1, r2=r2)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def _rows(c, d, idx, K):
    """Rows (B, m K, Cout) of a launch with these indices: float64 value, float32 value of the forms that are one add
    (None with s1 / s2) and the float64 bound of the others."""
    C, ld = c.Cout, pad4(c.Cout)
    q = np.arange(idx.shape[1] * K) // K
    b = np.arange(c.B)[:, None]
    flat = idx.reshape(c.B, -1)
    u32, v32 = d["U"][b, flat, :C], d["V2"][:, q, :C]
    v0 = d["V2"][:, q, ld:ld + C]
    y64 = u32.astype(np.float64) + v32
    mag = np.abs(u32).astype(np.float64) + np.abs(v32)
    y32 = None
    if d["s1"] is None:
        y32 = u32 + v32                                      # float32, one rounding
    for s, rr in ((d["s1"], d["r1"]), (d["s2"], d["r2"])):
        if s is not None:
            t = s.astype(np.float64)[:, :, None] * rr.astype(np.float64)[None, None, :C]
            y64, mag = y64 + t, mag + np.abs(t)
    bound = 4 * U32 * mag
    if d["counts"] is not None:
        em = (d["counts"][:, q] <= 0)[:, :, None]
        y64, bound = np.where(em, v0, y64), np.where(em, 0.0, bound)
        if y32 is not None:
            y32 = np.where(em, v0, y32)
    return y64, y32, bound


def _moments(f, n, extra=0, scale=1.0):
    """f: (rows, C) float64 summands -> (m1, m2, bound1, bound2), each (C,)."""
    a, s = np.abs(f).sum(0), (f * f).sum(0)
    return (scale * f.sum(0), scale * s, (n + 4 + extra) * U32 * abs(scale) * a, (n + 6 + extra) * U32 * abs(scale) * s)


def in_windows(c):
    w = np.zeros(c.Cout, dtype=bool)
    w[c.windows[0]:c.windows[0] + c.windows[1]] = True
    w[c.windows[2]:c.windows[2] + c.windows[3]] = True
    return w


Reference = collections.namedtuple(
    "Reference", "y64 y32 ybound row_written mom mom_bound mom_written yd32 tile_valid wrow0 ptpb")


@functools.lru_cache(maxsize=8)
def reference(c):
    """What the launch must leave behind, after the preconditions of the case.
    y64 / y32 / ybound (B rpb, Cout): the rows; row_written (B rpb) bool: rows of walked tiles;
    mom / mom_bound (B ptpb, Cout, 2) float64 and mom_written (B ptpb, Cout) bool: the entries of `partial` the launch
    writes (every other one keeps its sentinel); yd32 (B m, Cout): the twin's per-query rows or None."""
    d = inputs(c)
    rpb, tpb, ptpb = c.m * c.K, tiles_per_cloud(c), partial_tpb(c)
    y64, y32, yb = _rows(c, d, d["idx"], c.K)
    tv = tile_valid(c) if c.tiles else np.ones((c.B, tpb), dtype=np.uint8)
    roww = np.repeat(tv.astype(bool), TM, axis=1)[:, :rpb]
    mom = np.zeros((c.B * ptpb, c.Cout, 2))
    bound = np.zeros_like(mom)
    written = np.zeros((c.B * ptpb, c.Cout), dtype=bool)
    win = in_windows(c)
    relu = np.arange(c.Cout) >= c.relu_col0

    def signs_ok(f, what):
        cols = win & relu
        if cols.any():
            assert (f[:, cols] > 0).any(0).all() and (f[:, cols] < 0).any(0).all(), \
                "%s %s: a ReLU column of one sign" % (case_id(c), what)
    if "p" in c.out:
        for b in range(1 if c.same_clouds else c.B):         # (copies of a cloud: computed once)
            for t in range(tpb):
                if not tv[b, t]:
                    continue
                blk = y64[b, t * TM:(t + 1) * TM]
                signs_ok(blk, "cloud %d tile %d" % (b, t))
                m1, m2, b1, b2 = _moments(np.where(relu[None], np.maximum(blk, 0), blk), blk.shape[0])
                for bb in range(c.B) if c.same_clouds else (b,):
                    row = bb * ptpb + t
                    mom[row, :, 0], mom[row, :, 1], bound[row, :, 0], bound[row, :, 1] = m1, m2, b1, b2
                    written[row] = win
    yd32, wrow0 = None, None
    if c.twin:
        wrow0, wmul = np.asarray(c.twin[0], dtype=np.int32), c.twin[1]
        q64, yd32, _ = _rows(c, d, d["idx"][:, :, :1], 1)
        for b in range(c.B):
            for j in range(twin_tiles_per_cloud(c)):
                lo, hi = max(j * TM, int(wrow0[b])), min(c.m, (j + 1) * TM)
                blk = q64[b, lo:hi] if hi > lo else q64[b, :0]
                if blk.shape[0] >= 4:
                    signs_ok(blk, "cloud %d twin tile %d" % (b, j))
                row = b * ptpb + tpb + j
                m1, m2, b1, b2 = _moments(np.where(relu[None], np.maximum(blk, 0), blk), blk.shape[0], 1, wmul)
                mom[row, :, 0], mom[row, :, 1], bound[row, :, 0], bound[row, :, 1] = m1, m2, b1, b2
                written[row] = win
    check_inputs(c, d)
    P = c.B * rpb
    ref = Reference(y64.reshape(P, -1), None if y32 is None else y32.reshape(P, -1), yb.reshape(P, -1),
                    roww.reshape(P), mom, bound, written, None if yd32 is None else yd32.reshape(c.B * c.m, -1),
                    tv, wrow0, ptpb)
    for a in ref:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def wave_rows(c):
    """Rows of each wave of a cloud's LAST tile."""
    nvalid = c.m * c.K - (tiles_per_cloud(c) - 1) * TM
    return [max(0, min(32, nvalid - 32 * w)) for w in range(4)]


def check_inputs(c, d):
    """Preconditions that are facts of the inputs."""
    rpb = c.m * c.K
    for b in range(c.B if not c.same_clouds else 1):
        live = np.ones(c.m, dtype=bool) if d["counts"] is None else d["counts"][b] > 0
        used = d["idx"][b][live]
        if rpb >= 8:
            assert used.min() == 0 and used.max() == c.n_src - 1, "%s: cloud %d misses an end of the sources" % (
                case_id(c), b)
        if d["counts"] is not None and c.m > 1:
            em = np.repeat(d["counts"][b] <= 0, c.K)
            if c.K <= 16:       # a wave of 32 rows reaches two queries: it holds an empty and a non-empty one
                for r0 in range(0, rpb, 32):
                    if (r0 % TM) + 32 <= TM and min(rpb, r0 + 32) - r0 > c.K:
                        w = em[r0:r0 + 32]
                        assert w.any() and not w.all(), "%s: cloud %d rows %d..: one kind of ball" % (case_id(c), b, r0)
            else:               # K = 32 / 64: a wave is (part of) one query; a TILE with two queries holds both kinds
                for r0 in range(0, rpb, TM):
                    w = em[r0:r0 + TM]
                    assert w.shape[0] <= c.K or w.any() and not w.all(), "%s: cloud %d tile at row %d: one kind of ball" % (case_id(c), b, r0)
