"""pdr_gather_plan over the dispatch table of the virtual first conv's gather kernel (csrc/fused_gather.hip), host only:
nothing is launched, no device pointer exists.

Every cell of REQUIRED -- the 48 instantiations of gather_kernel, the 24 that enter the twin body, and what a launch
decides at run time (the row walk, statistics on or off, the ReLU or the plain loop, passes on grid.y or inside the
workgroup, windows, tile subsets, twin tiles, ragged and empty waves) -- must be reached by a case of
tests/gather_cases.py, which is what tests/test_gather_dispatch_gpu.py runs; the plan must refuse exactly what the calls
refuse; and every reference must meet the preconditions its case is for.
"""
import itertools

import numpy as np

from point_diffusion_refinement_amd import _lib
from tests import gather_cases as gc

TF = (0, 1)
REQUIRED = (
    [("kernel", lpr, kp, hs, he, yw) for lpr, kp, hs, he, yw in itertools.product((16, 32, 64), TF, TF, TF, TF)] +
    [("twin body", lpr, kp, he, yw) for lpr, kp, he, yw in itertools.product((16, 32, 64), TF, TF, TF)] +
    [("walk", lpr, w, st) for lpr in (16, 32, 64) for w in ("shared", "row", "division")
     for st in ("stats", "Y only")] +
    [("threshold", lpr, side) for lpr in (16, 32, 64) for side in ("K = rows", "K = rows / 2")] +
    [("K", k) for k in (1, 2, 4, 8, 16, 32, 64, "3 or 6")] +
    [("K", k, "not in a twin tile, per row") for k in (1, 2, 4)] +
    [("K no power of two", w) for w in ("Y", "counts", "lpr 32", "lpr 64")] +
    [("Y only", w) for w in ("K = 1", "column window", "serial passes")] +
    [("form", f, lpr) for f in gc.FORMS for lpr in (16, 32, 64)] +
    [("Cout", C) for C in (7, 64, 65, 128, 129, 256, 257, 300)] + [("Y", "Cout % 4 != 0")] +
    [("Y window", lpr, "ycol0 > 0, ycols % 4 != 0, ldy > padded") for lpr in (16, 32, 64)] +
    [("Y window", 64, "two passes")] +
    [("pass", loop, walk) for loop in ("relu", "plain", "relu from inside a piece") for walk in ("shared", "per row")] +
    [("relu_col0", w) for w in (0, "inside a float4 piece", "first column of the second pass", ">= Cout")] +
    [("passes", w) for w in ("one", "grid.y", "serial", "exactly 256 columns", "second pass of one piece")] +
    [("windows", w) for w in ("one", "two", "first length % 4 != 0", "in different passes", "both in one pass", "a pass holds both",
                              "win1 ends at Cout, Cout % 4 != 0")] +
    [("tiles", e) for e in ("add_tiles", "moments_tiles")] + [("tiles", "first / last ragged / whole cloud cleared"),
                                                              ("tiles", "partial_tpb larger than needed")] +
    [("twin", "K", k) for k in (32, 8, 6)] + [("twin", "m", 12), ("twin", "three tiles per cloud, the last ragged")] +
    [("twin", "wrow0", w) for w in ("0", "tile boundary", "inside a tile", "m")] +
    [("rows", w) for w in ("cloud shorter than a tile", "last wave % 32 != 0", "empty wave", "two full tiles + tail")])


def _report(title, reached, required):
    print("\n%s: %d cells reached" % (title, len(reached)))
    for cell in sorted(reached, key=str):
        print("  %-64s %3d cases  e.g. %s" % (cell, len(reached[cell]), reached[cell][0]))
    missing = [c for c in required if c not in reached]
    assert not missing, "%s: cells no case reaches: %s" % (title, missing)


def _pass_columns(p):
    """First columns of the float4 pieces of every column pass, as gather_tile walks the windows."""
    w4a = (p.na + 3) // 4
    cols = [p.c0a + 4 * q if q < w4a else p.c0b + 4 * (q - w4a) for q in range(p.w4)]
    return [cols[i:i + p.lpr] for i in range(0, p.w4, p.lpr)]


def _cells(c, p):
    lpr, rpb = p.lpr, c.m * c.K
    cells = [("kernel", lpr, p.kpow2, p.has_s, p.has_em, p.ywin), ("form", c.form, lpr)]
    walk = "shared" if p.shared else ("row" if p.kpow2 else "division")
    cells.append(("walk", lpr, walk, "stats" if p.stats else "Y only"))
    if c.K == p.shared_rows:
        assert p.shared
        cells.append(("threshold", lpr, "K = rows"))
    if 2 * c.K == p.shared_rows:
        assert not p.shared
        cells.append(("threshold", lpr, "K = rows / 2"))
    cells.append(("K", c.K if c.K not in (3, 6) else "3 or 6"))
    if c.K in (1, 2, 4) and not p.shared:
        cells.append(("K", c.K, "not in a twin tile, per row"))
    if not p.kpow2:
        cells += [("K no power of two", w) for w, on in (("Y", p.ywin), ("counts", p.has_em), ("lpr 32", lpr == 32),
                                                         ("lpr 64", lpr == 64)) if on]
    passes = _pass_columns(p)
    serial = p.passes > 1 and p.grid_y == 1
    if not p.stats:
        cells += [("Y only", w) for w, on in (("K = 1", c.K == 1), ("column window", "w" in c.out), ("serial passes", serial))
                  if on]
    if c.entry.startswith("add"):
        cells.append(("Cout", c.Cout))
    if p.ywin:
        ycol0, ycols, ldy = gc.ywindow(c)
        if c.Cout % 4:
            cells.append(("Y", "Cout % 4 != 0"))
        if ycol0 > 0 and ycols % 4 and ldy > p.y4:
            cells.append(("Y window", lpr, "ycol0 > 0, ycols % 4 != 0, ldy > padded"))
            if p.passes == 2:
                cells.append(("Y window", 64, "two passes"))
    if p.stats:
        for cols in passes:                   # the loop a pass takes: gather_tile's `relu` and its per-lane bounds
            relu = cols[-1] + 3 >= c.relu_col0
            split = any(col < c.relu_col0 < col + 4 for col in cols)
            loop = "relu from inside a piece" if split else ("relu" if relu else "plain")
            cells.append(("pass", loop, "shared" if p.shared else "per row"))
        walked = [col + j for cols in passes for col in cols for j in range(4)]
        if c.relu_col0 == 0:
            cells.append(("relu_col0", 0))
        elif c.relu_col0 >= c.Cout:
            cells.append(("relu_col0", ">= Cout"))
        elif c.relu_col0 % 4 and c.relu_col0 in walked:
            cells.append(("relu_col0", "inside a float4 piece"))
        if p.passes > 1 and c.relu_col0 == passes[1][0]:
            cells.append(("relu_col0", "first column of the second pass"))
    cells.append(("passes", "one" if p.passes == 1 else ("serial" if serial else "grid.y")))
    if p.w4 == 64 and lpr == 64:
        cells.append(("passes", "exactly 256 columns"))
    if p.w4 == 65:
        cells.append(("passes", "second pass of one piece"))
    if c.entry.startswith("moments"):
        cells.append(("windows", "two" if p.nb else "one"))
        if p.nb:
            w4a = (p.na + 3) // 4
            if p.na % 4:
                cells.append(("windows", "first length % 4 != 0"))
            cells.append(("windows", "in different passes" if w4a % lpr == 0 else
                          "both in one pass" if p.w4 <= lpr else "a pass holds both"))
            if p.c0b + p.nb == c.Cout and c.Cout % 4:
                cells.append(("windows", "win1 ends at Cout, Cout % 4 != 0"))
    if c.tiles and not c.twin:
        tv = gc.tile_valid(c)
        assert tv[0, 0] == 0 and tv[1, -1] == 0 and not tv[2].any() and tv[0, 1:].all() and rpb % gc.TM
        cells += [("tiles", c.entry), ("tiles", "first / last ragged / whole cloud cleared")]
        if gc.partial_tpb(c) > p.tpb:
            cells.append(("tiles", "partial_tpb larger than needed"))
    if c.twin:
        assert p.n_twin == c.B * p.twin_tpb and p.n_main == c.B * p.tpb and p.grid_x == p.n_main + p.n_twin
        cells += [("twin body", lpr, p.kpow2, p.has_em, p.ywin), ("twin", "K", c.K)]
        if c.m == 12:
            cells.append(("twin", "m", 12))
        if p.twin_tpb == 3 and c.m % gc.TM:
            cells.append(("twin", "three tiles per cloud, the last ragged"))
        for w in c.twin[0]:
            cells.append(("twin", "wrow0", "0" if w == 0 else "m" if w == c.m else
                          "tile boundary" if w % gc.TM == 0 else "inside a tile"))
    waves = gc.wave_rows(c)
    if rpb < gc.TM:
        cells.append(("rows", "cloud shorter than a tile"))
    if any(w % 32 for w in waves):
        cells.append(("rows", "last wave % 32 != 0"))
    if 0 in waves:
        cells.append(("rows", "empty wave"))
    if rpb > 2 * gc.TM and rpb % gc.TM:
        cells.append(("rows", "two full tiles + tail"))
    return cells


def test_cases_reach_every_cell_of_the_dispatch_table():
    reached = {}
    for c in gc.all_cases():
        rc, p = gc.plan(c)
        assert rc == _lib.PDR_OK, (gc.case_id(c), rc)
        # what the plan reports is what the case is about
        assert p.lpr == gc.lpr_of(c.Cout) and p.shared_rows == gc.SHARED_ROWS[p.lpr] and p.tpb == gc.tiles_per_cloud(c)
        assert p.stats == ("p" in c.out) and p.ywin == (c.out != "p") and p.tiles == bool(c.tiles)
        assert (p.c0a, p.na) == c.windows[:2] and p.nb == c.windows[3] and (not p.nb or p.c0b == c.windows[2])
        assert p.grid_y == (p.passes if p.grid_x <= 1024 and p.passes > 1 else 1)
        for cell in _cells(c, p):
            reached.setdefault(cell, []).append(gc.case_id(c))
    _report("gather", reached, REQUIRED)
    assert len(gc.all_cases()) <= 400, "a few hundred launches at most"
    # the example of the issue is what its comment says: 344 rows, waves of 32 / 32 / 24 / 0 in the last tile
    k8 = next(c for c in gc.all_cases() if c.K == 8 and c.m == 43)
    assert gc.wave_rows(k8) == [32, 32, 24, 0]


def _plan(B=3, n_src=37, rpb=344, K=8, Cout=171, ld=None, ldy=None, ycol0=0, ycols=-1, win=None, ptpb=0, ldyd=0,
          flags=gc.HAS_PARTIAL):
    ld = gc.pad4(Cout) if ld is None else ld
    return gc.plan_call(B, n_src, rpb, K, Cout, ld, ld, ld if ldy is None else ldy, ycol0, ycols,
                        *(win or (0, Cout, 0, 0)), ptpb, ldyd, flags)


def test_shared_walk_threshold_for_every_K():
    """For each lanes-per-row and K = 1 .. 64: KPOW2 is 'a power of two <= 32', and the one-V-row-per-query walk is
    taken from K = 16 / 8 / 4 on -- read from the constants the kernel reads."""
    for Cout, lpr in ((64, 16), (128, 32), (300, 64)):
        for K in range(1, 65):
            rc, p = _plan(rpb=3 * K, K=K, Cout=Cout)
            pow2 = K & (K - 1) == 0 and K <= 32
            assert rc == _lib.PDR_OK and p.lpr == lpr and p.kpow2 == pow2, (Cout, K, p)
            assert p.shared_rows == {16: 16, 32: 8, 64: 4}[lpr] and p.shared == (pow2 and K >= p.shared_rows), (Cout, K, p)


def test_lanes_per_row_boundaries_and_grid_y():
    for Cout in range(1, 700):
        rc, p = _plan(Cout=Cout)
        assert rc == _lib.PDR_OK and p.lpr == (16 if Cout <= 64 else 32 if Cout <= 128 else 64), (Cout, p)
        assert p.w4 == (Cout + 3) // 4 and p.passes == -(-p.w4 // p.lpr)
    for Cout, lpr in ((64, 16), (65, 32), (128, 32), (129, 64)):
        assert _plan(Cout=Cout)[1].lpr == lpr
    # grid.y == passes exactly when nblocks <= 1024 && passes > 1 (B tiles of one 8-row cloud; twin tiles count)
    for Bq, Cout, twin in itertools.product((1, 341, 512, 513, 1024, 1025, 3000), (256, 257, 513, 300), (False, True)):
        flags = gc.HAS_PARTIAL | ((gc.HAS_TILES | gc.HAS_TWIN) if twin else 0)
        rc, p = _plan(B=Bq, rpb=8, Cout=Cout, flags=flags, ptpb=2, ldyd=gc.pad4(Cout))
        nblocks = Bq * (2 if twin else 1)
        assert rc == _lib.PDR_OK and p.grid_x == nblocks and p.n_twin == (Bq if twin else 0), (Bq, Cout, twin, p)
        assert (p.grid_y == p.passes) == (nblocks <= 1024 and p.passes > 1) or p.passes == 1, (Bq, Cout, twin, p)
        assert p.grid_y == (p.passes if nblocks <= 1024 and p.passes > 1 else 1)
    # windows of a statistics-only pass: the passes are those of the walked pieces, the lanes per row those of Cout
    rc, p = _plan(Cout=301, win=(0, 254, 256, 45))
    assert (p.lpr, p.w4, p.passes, p.grid_y) == (64, 76, 2, 2) and (p.c0a, p.na, p.c0b, p.nb) == (0, 254, 256, 45)
    rc, p = _plan(Cout=301, win=(0, 64, 0, 0))
    assert (p.lpr, p.w4, p.passes, p.grid_y) == (64, 16, 1, 1) and (p.c0b, p.nb) == (64, 0)


def test_plan_refuses_what_the_calls_refuse():
    """The code table of test_gather_moments_gpu.py::test_argument_errors_launch_nothing, for every refusal that does
    not depend on a pointer's value: the same code from the plan and from the call (whose pointers are never read)."""
    lib = _lib.load()
    p, EINVAL, EUNSUP, OK = 0x1000, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED, _lib.PDR_OK
    S12 = gc.HAS_S1 | gc.HAS_S2

    def gm(win=(0, 64, 128, 43), partial=p, B=2, K=8, ldu=172):
        call = lib.pdr_gather_moments(p, ldu, 100, p, None, 172, p, None, p, p, p, p, B, 256, K, 171, partial, 128, *win,
                                      None)
        rc, _ = gc.plan_call(B, 100, 256, K, 171, ldu, 172, 0, 0, -1, *win, 0, 0, S12 | (gc.HAS_PARTIAL if partial else 0))
        return call, rc
    for kw, want in [(dict(win=(0, 62, 130, 41)), EUNSUP), (dict(win=(2, 62, 128, 43)), EUNSUP),
                     (dict(win=(0, 64, 60, 43)), EINVAL), (dict(win=(128, 43, 0, 64)), EINVAL),
                     (dict(win=(0, 64, 128, 44)), EINVAL), (dict(win=(0, 172, 0, 0)), EINVAL),
                     (dict(win=(-4, 64, 128, 43)), EINVAL), (dict(win=(0, 0, 128, 43)), EINVAL),
                     (dict(win=(0, 64, 128, -1)), EINVAL), (dict(partial=None), EINVAL), (dict(K=7), EINVAL),
                     (dict(K=0), EINVAL), (dict(ldu=170), EINVAL), (dict(B=-1), EINVAL), (dict(B=0), OK),
                     (dict(win=(0, 64, 0, 0), B=0), OK), (dict(win=(0, 64, 60, 43), B=0), EINVAL)]:
        assert gm(**kw) == (want, want), (kw, gm(**kw), want)

    def tiles(ptpb=2, B=2):
        call = lib.pdr_gather_moments_tiles(p, 172, 100, p, None, 172, p, None, None, None, None, None, B, 256, 8, 171, p,
                                            128, 0, 64, 128, 43, p, ptpb, None)
        rc, _ = gc.plan_call(B, 100, 256, 8, 171, 172, 172, 0, 0, -1, 0, 64, 128, 43, ptpb, 0,
                             gc.HAS_PARTIAL | gc.HAS_TILES)
        return call, rc
    assert tiles(ptpb=1) == (EINVAL, EINVAL) and tiles(ptpb=1, B=0) == (EINVAL, EINVAL) and tiles(B=0) == (OK, OK)

    def tw(win=(0, 64, 128, 43), partial=p, ptpb=3, ldyd=172, K=32, B=2, s=0):
        call = None
        if not s:
            call = lib.pdr_gather_moments_tiles_twin(p, 172, 100, p, None, 172, p, None, B, 256, K, 171, partial, 128,
                                                     *win, p, ptpb, p, p, ldyd, p, 32.0, None)
        rc, _ = gc.plan_call(B, 100, 256, K, 171, 172, 172, 0, 0, -1, *win, ptpb, ldyd,
                             s | gc.HAS_TILES | gc.HAS_TWIN | (gc.HAS_PARTIAL if partial else 0))
        return call, rc
    for kw, want in [(dict(ptpb=2), EINVAL), (dict(ldyd=170), EINVAL), (dict(partial=None), EINVAL),
                     (dict(win=(0, 64, 126, 45)), EUNSUP), (dict(win=(0, 64, 32, 43)), EINVAL), (dict(K=7), EINVAL),
                     (dict(K=7, B=0), EINVAL), (dict(ptpb=2, B=0), OK)]:
        assert tw(**kw) == (want, want), (kw, tw(**kw), want)
    assert tw(s=gc.HAS_S1)[1] == EINVAL                                # the twin form is the ball form
    # pdr_gather_add: the written window of Y.  (Accepted sizes with B > 0 go to the plan alone: the call would launch.)
    def add(ycol0=0, ycols=-1, ldy=172, Y=p, partial=p, call=True):
        rc, pl = gc.plan_call(2, 100, 256, 8, 171, 172, 172, ldy, ycol0, ycols, 0, 171, 0, 0, 0, 0,
                              (gc.HAS_Y if Y else 0) | (gc.HAS_PARTIAL if partial else 0))
        if not call:
            return rc, pl
        return lib.pdr_gather_add(p, 172, 100, p, None, 172, p, None, None, None, None, None, 2, 256, 8, 171, Y, ldy,
                                  partial, 128, ycol0, ycols, None), rc
    for kw in [dict(ycol0=2), dict(ycol0=-4), dict(ycol0=8, ycols=164), dict(ycols=0), dict(ldy=170),
               dict(ycol0=8, ycols=30, ldy=28), dict(Y=None, partial=None)]:
        assert add(**kw) == (EINVAL, EINVAL), (kw, add(**kw))
    for kw, y in [(dict(ycol0=8, ycols=30, ldy=32), (8, 32)), (dict(partial=None), (0, 172)), (dict(Y=None, ldy=0), (0, 0)),
                  (dict(ycol0=168), (168, 4))]:
        rc, pl = add(call=False, **kw)
        assert rc == OK and pl.lpr == 64 and (pl.ycol0, pl.y4) == y, (kw, pl)
    assert _plan(B=2, rpb=256, Cout=171, win=(0, 64, 128, 43))[0] == OK            # the base call of the tables above
    # an empty call launches nothing; no `out`, unknown flags
    rc, pl = _plan(B=0)
    assert rc == OK and not any(pl)
    assert lib.pdr_gather_plan(*([3, 37, 344, 8, 64, 64, 64, 64, 0, -1, 0, 64, 0, 0, 0, 0, 16]), None) == EINVAL
    assert gc.plan_call(3, 37, 344, 8, 64, 64, 64, 64, 0, -1, 0, 64, 0, 0, 0, 0, 128 | 16)[0] == EINVAL


def test_every_reference_meets_its_precondition():
    """Computing a reference asserts, on the inputs and the float64 rows: both ends of the source range are gathered,
    empty and non-empty balls share every wave that holds two queries, both signs occur in every ReLU column of every
    tile.  Here also: the ragged tail is ragged, and the empty balls really are V0 rows."""
    ragged = 0
    for c in gc.all_cases():
        ref, d = gc.reference(c), gc.inputs(c)
        rpb = c.m * c.K
        if c.m > 1 and not c.twin and not c.same_clouds:
            assert rpb > 2 * gc.TM and rpb % gc.TM, gc.case_id(c)
            ragged += any(w % 32 for w in gc.wave_rows(c)) and 0 in gc.wave_rows(c)
        if d["counts"] is not None:
            em = np.repeat(d["counts"].reshape(-1) <= 0, c.K)
            ld = gc.pad4(c.Cout)
            v0 = np.repeat(d["V2"].reshape(c.B * c.m, -1)[:, ld:ld + c.Cout], c.K, axis=0)
            assert np.array_equal(ref.y64[em], v0[em].astype(np.float64)) and em.any() and not em.all()
        assert np.isfinite(ref.y64).all() and np.isfinite(ref.mom).all()
    assert ragged >= 10
