"""pdr_fps_plan / pdr_knn_plan / pdr_ball_query_plan over the dispatch tables of the geometry kernels, host only
(nothing is launched, no device pointer exists).

Every cell listed below -- every instantiation of csrc/fps.hip, csrc/neighbors.hip (dense) and csrc/ball_query.hip, at
the sizes where it can go wrong -- must be reached by a case of tests/geometry_cases.py, which is what
tests/test_geometry_dispatch_gpu.py runs; and the plans must refuse exactly what the calls refuse.
"""
import ctypes

from point_diffusion_refinement_amd import _lib
from tests import geometry_cases as gc

# ---- FPS: the 22 instantiations, (family, T, PPT) -> (smallest, largest) admissible N over all option settings, from
# plan_fps (csrc/fps.hip).  slots = R Q with R = min(2^floor(log2 N), 512), Q = ceil(N / R); the wave kernel takes
# slots <= 128 / 256 / 512 / 1024 / 2048 / 4096, the lean kernel N <= 512 / 1024 / 2048 / 3072 / 4080 (above 128), the
# resident kernel N <= T PPT; the wave and lean kernels end at N = 4080 (N float4 + 256 B <= 64 KiB of LDS) and the
# stream kernel starts behind 12288 (3 N floats of LDS).
FPS_REQUIRED = {
    ("resident", 64, 1): (1, 64), ("resident", 64, 2): (65, 128), ("resident", 256, 1): (129, 256),
    ("resident", 256, 2): (257, 512), ("resident", 256, 4): (513, 1024), ("resident", 256, 8): (1025, 2048),
    ("resident", 256, 12): (2049, 3072), ("resident", 256, 16): (3073, 4096), ("resident", 1024, 8): (4097, 8192),
    ("resident", 1024, 12): (8193, 12288),
    ("wave", 64, 2): (1, 128), ("wave", 64, 4): (129, 256), ("wave", 256, 2): (257, 512), ("wave", 256, 4): (513, 1024),
    ("wave", 256, 8): (1025, 2048), ("wave", 256, 16): (2049, 4080),
    ("lean", 256, 2): (129, 512), ("lean", 256, 4): (513, 1024), ("lean", 256, 8): (1025, 2048),
    ("lean", 256, 12): (2049, 3072), ("lean", 256, 16): (3073, 4080),
    ("stream", 1024, 0): (12289, None),
}
FPS_NEED_PADDED = {c for c in FPS_REQUIRED if c[0] in ("wave", "lean")}     # also at an N with R Q > N

# ---- kNN (dense instantiations; the ragged ones share plan_knn)
KNN_REQUIRED = (
    [("thread", kmax, "Kout=KMAX") for kmax in (1, 4, 8, 16, 32)] +
    [("thread", kmax, "Kout<KMAX") for kmax in (4, 8, 16, 32)] +
    [("thread", "n2<K"), ("thread", "n2>1024")] +
    [("wave", nch, what) for nch in (1, 2, 4, 8, 16) for what in ("smallest n2", "largest n2", "odd K", "qpw>1")] +
    [("packed",), ("group", "wave")] + [("group", "thread", kg) for kg in (4, 8, 16)])
KNN_WAVE_N2 = {1: (64, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512), 16: (513, 1024)}

# ---- ball query: resident NCH at both edges of its range of n (NCH = 1: the table starts at n = 63), the streaming
# kernel, and queries-per-wave 2 and 16 with a partial last workgroup
BALL_EDGES = {1: (63, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512), 16: (513, 1024), 32: (1025, 2048),
              48: (2049, 3072), 64: (3073, 4096)}
BALL_REQUIRED = ([("resident", nch, n) for nch, edges in BALL_EDGES.items() for n in edges] +
                 [("stream",), ("qpw", 2), ("qpw", 16)])


def _report(title, reached, required):
    print("\n%s: %d cells reached" % (title, len(reached)))
    for cell in sorted(reached, key=str):
        print("  %-34s %3d cases  e.g. %s" % (cell, len(reached[cell]), reached[cell][0]))
    missing = [c for c in required if c not in reached]
    assert not missing, "%s: cells no case reaches: %s" % (title, missing)


def test_fps_plan_boundaries_are_the_stated_ones():
    """The table above is what the library does: over every N up to behind the stream threshold and every option set,
    each cell's smallest and largest N are the stated ones, and no other cell exists."""
    lo, hi = {}, {}
    for opts in gc.FPS_OPTION_SETS.values():
        with gc.options(opts):
            for N in range(1, 12400):
                rc, cell, slots = gc.fps_plan(N)
                assert rc == _lib.PDR_OK and slots >= N, (N, rc, cell, slots)
                lo[cell] = min(lo.get(cell, N), N)
                hi[cell] = max(hi.get(cell, N), N)
    assert set(lo) == set(FPS_REQUIRED)
    for cell, (a, b) in FPS_REQUIRED.items():
        assert lo[cell] == a and (b is None or hi[cell] == b), (cell, lo[cell], hi[cell])
    out = (ctypes.c_int * 4)()
    assert _lib.load().pdr_fps_plan(0, out) == _lib.PDR_EINVAL and _lib.load().pdr_fps_plan(5, None) == _lib.PDR_EINVAL


def test_fps_cases_reach_every_instantiation_at_its_edges():
    reached, padded, at = {}, set(), {}
    for opt, N in gc.fps_cases():
        with gc.options(gc.FPS_OPTION_SETS[opt]):
            rc, cell, slots = gc.fps_plan(N)
            # the plan and the workspace query agree on where the stream kernel (and its workspace) starts
            assert (_lib.load().pdr_fps_workspace_bytes(gc.B, N) > 0) == (cell[0] == "stream"), (opt, N, cell)
        reached.setdefault(cell, []).append("%s: N=%d m=%d" % (opt, N, gc.fps_m(N)))
        at.setdefault(cell, set()).add(N)
        if slots > N:
            padded.add(cell)
    _report("FPS", reached, FPS_REQUIRED)
    for cell, (a, b) in FPS_REQUIRED.items():
        assert a in at[cell] and (b is None or b in at[cell]), "%s is not run at both edges %s" % (cell, (a, b))
    assert not FPS_NEED_PADDED - padded, "never run with padded slots: %s" % sorted(FPS_NEED_PADDED - padded)


def _knn_cells(shape, cell, group):
    _, n1, n2, K, nn = shape
    family, param, qpw, _ = cell
    if group:
        return [("group", "wave")] if family == "wave" else [("group", "thread", param)]
    if family == "packed":
        return [("packed",)]
    if family == "thread":
        cells = [("thread", param, "Kout=KMAX" if K == param else "Kout<KMAX")]
        if n2 < K:
            cells.append(("thread", "n2<K"))
        if n2 > 1024:
            cells.append(("thread", "n2>1024"))
        return cells
    cells = []
    if n2 == KNN_WAVE_N2[param][0]:
        cells.append(("wave", param, "smallest n2"))
    if n2 == KNN_WAVE_N2[param][1]:
        cells.append(("wave", param, "largest n2"))
    if K % 2:
        cells.append(("wave", param, "odd K"))
    if qpw > 1:
        cells.append(("wave", param, "qpw>1"))
    return cells


def test_knn_cases_reach_every_instantiation_at_its_edges():
    reached = {}
    for opt, shape in gc.knn_cases():
        with gc.options(gc.KNN_OPTION_SETS[opt]):
            for group in (False, True) if gc.knn_group_applies(shape) else (False,):
                rc, cell = gc.knn_plan(shape, group)
                assert rc == _lib.PDR_OK, (opt, shape, group, rc)
                n2, K = shape[2], shape[3]
                if cell[0] == "wave":        # what the wave kernel relies on
                    assert 2 - group <= K <= 8 and K <= n2 and KNN_WAVE_N2[cell[1]][0] <= n2 <= KNN_WAVE_N2[cell[1]][1]
                    assert opt == "defaults"
                if cell[0] == "thread":
                    assert K <= cell[1]
                for c in _knn_cells(shape, cell, group):
                    reached.setdefault(c, []).append("%s: B=%d n1=%d n2=%d K=%d%s" % (
                        (opt,) + shape[:4] + (" group" if group else "" if shape[4] else " no nn",)))
    _report("kNN", reached, KNN_REQUIRED)
    # the qpw > 1 shapes are what their comment says: a partial and an empty wave in the last workgroup
    rc, cell = gc.knn_plan((64, 1000, 64, 8, True))
    assert cell == ("wave", 1, 16, 16) and 1000 - 15 * 64 == 2 * 16 + 8
    rc, cell = gc.knn_plan((8, 1030, 64, 8, True))
    assert cell == ("wave", 1, 2, 129) and 1030 - 128 * 8 == 3 * 2


def test_knn_plan_refuses_what_the_calls_refuse():
    lib = _lib.load()
    out = (ctypes.c_int * 4)()
    plan = lambda B, n1, n2, K, nn=0, group=0: lib.pdr_knn_plan(B, n1, n2, K, nn, group, out)
    points = lambda B, n1, n2, K: lib.pdr_knn_points(None, None, B, n1, n2, K, None, None, None, None)
    group = lambda B, n1, n2, K: lib.pdr_knn_group(None, None, B, n1, n2, K, None, None, None, None)
    EINVAL, EUNSUP, OK = _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED, _lib.PDR_OK
    # refusals that do not depend on a pointer: the same code from the plan and from the call (with null pointers)
    for args, want in [((2, 300, 64, 33), EUNSUP), ((2, 300, 64, 40), EUNSUP), ((2, 300, 64, 0), EINVAL),
                       ((-1, 300, 64, 8), EINVAL), ((2, -1, 64, 8), EINVAL), ((2, 300, -1, 8), EINVAL)]:
        assert plan(*args) == want == points(*args), args
    for args, want in [((2, 300, 64, 17), EUNSUP), ((2, 300, 100, 32), EUNSUP), ((2, 300, 7, 8), EINVAL),
                       ((2, 300, 16, 17), EINVAL), ((2, 300, 0, 1), EINVAL), ((2, 300, 64, 0), EINVAL),
                       ((-1, 300, 64, 8), EINVAL)]:
        assert plan(*args, group=1) == want == group(*args), args
    # accepted sizes: the plan says OK where the call gets as far as its pointer check (EINVAL for the null pointers)
    for args in [(2, 300, 64, 32), (2, 300, 0, 3), (2, 300, 3, 8)]:
        assert plan(*args) == OK and points(*args) == EINVAL, args
    for args in [(2, 300, 64, 16), (2, 300, 16, 16), (2, 300, 1, 1)]:
        assert plan(*args, group=1) == OK and group(*args) == EINVAL, args
    # empty calls launch nothing
    for args in [(0, 300, 64, 8), (2, 0, 64, 8)]:
        assert plan(*args) == OK and out[0] == -1 and points(*args) == OK
        assert plan(*args, group=1) == OK and out[0] == -1 and group(*args) == OK
    assert lib.pdr_knn_plan(2, 300, 64, 8, 0, 0, None) == EINVAL


def test_ball_query_cases_reach_every_instantiation_at_its_edges():
    lib = _lib.load()
    reached = {}
    for case in gc.ball_cases():
        Bq, m, n, ns, radius = case
        rc, (nch, resident, qpw, gx) = gc.ball_plan(case)
        assert rc == _lib.PDR_OK and radius < 2.0
        label = "B=%d m=%d n=%d nsample=%d r=%.3f" % case
        if resident:
            assert n <= 64 * nch and nch in gc.BALL_RESIDENT_NCH
            reached.setdefault(("resident", nch, n), []).append(label)
        else:
            assert n > 64 * gc.BALL_RESIDENT_NCH[-1]
            reached.setdefault(("stream",), []).append(label)
        if qpw > 1:
            assert m % (4 * qpw) and gx == -(-m // (4 * qpw))
            reached.setdefault(("qpw", qpw), []).append(label)
    _report("ball query", reached, BALL_REQUIRED)
    out = (ctypes.c_int * 4)()
    for args in [(-1, 64, 10), (2, 0, 10), (2, 64, -1)]:
        assert lib.pdr_ball_query_plan(*args, out) == _lib.PDR_EINVAL
        assert lib.pdr_ball_query(None, None, args[0], args[1], args[2], 0.5, 16, None, None, None) == _lib.PDR_EINVAL
    assert lib.pdr_ball_query_plan(2, 64, 0, out) == _lib.PDR_OK and list(out) == [0, 0, 0, 0]
    assert lib.pdr_ball_query_plan(2, 64, 10, None) == _lib.PDR_EINVAL


def test_every_reference_meets_its_precondition():
    """The inputs really contain what they are for (ties, excluded points, empty / partly filled / saturated balls):
    computing a reference asserts it, on the oracle's result.  Runs the oracle over every case, no GPU."""
    for N in gc.FPS_SIZES:
        for kind in gc.FPS_INPUTS:
            gc.fps_reference(N, kind)
    for shape in sorted({s[:4] + (True,) for _, s in gc.knn_cases()}):
        for kind in gc.KNN_INPUTS:
            gc.knn_reference(shape, kind)
    for case in gc.ball_cases():
        gc.ball_reference(case)
