"""The dispatch tables of the geometry kernels (csrc/fps.hip, csrc/neighbors.hip, csrc/ball_query.hip), the cases that
walk them and the inputs those cases run on.  A plain module: tests/test_geometry_dispatch_plan.py walks the tables
through pdr_fps_plan / pdr_knn_plan / pdr_ball_query_plan on the host, tests/test_geometry_dispatch_gpu.py runs every
case against oracle.pdr_oracle.

The contract of these kernels is bit-exact indices, so an input only tests something where the order of equal values or
a cap decides the answer.  Every reference below is therefore computed together with a PRECONDITION, asserted on the
oracle's result (never on the kernel's): a lattice cloud must really produce ties, a near-origin cloud must really
lose points to the |p|^2 <= 1e-3 exclusion, a ball query must really see empty, partly filled and saturated balls.
References are computed once per process, shared, and handed out read-only.
"""
import ctypes
import functools
import math
import os

import numpy as np

from oracle import pdr_oracle as O
from point_diffusion_refinement_amd import _lib
from tests.layer_cases import options  # noqa: F401  (set / restore process-wide options; re-exported for the tests)

B = 2


def _plan(fn, *args):
    """A host-only plan query of libpdr_hip.so: (return code, the four ints it reports)."""
    if not os.path.exists(_lib.LIB_PATH):      # the case lists are made at collection time, before any fixture runs
        import __graft_entry__
        __graft_entry__.build()
    out = (ctypes.c_int * 4)()
    rc = getattr(_lib.load(), fn)(*args, out)
    return rc, tuple(out)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _seed(name):
    """A stable integer per input kind (no hash(): it is salted per process)."""
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def lattice_side(n):
    """g = max(2, ceil((n / 2)^(1/3))): about two points per lattice site."""
    return max(2, math.ceil(round((n / 2.0) ** (1.0 / 3.0), 9)))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ====================================================================================================== FPS
FPS_FAMILIES = ("resident", "wave", "lean", "stream")
FPS_OPTION_SETS = {
    "defaults": {},
    "fps_wave=2": {"fps_wave": 2},
    "fps_wave=0": {"fps_wave": 0},
    "fps_wave=0,fps_lean=0": {"fps_wave": 0, "fps_lean": 0},
}
FPS_SIZES = (1, 2, 63, 64, 65, 100, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1024, 1025, 2048, 2049, 3072, 3073,
             4080, 4081, 4096, 4097, 8192, 8193, 12288, 12289)
FPS_INPUTS = ("uniform", "lattice", "near_origin")
FPS_TIE_MIN_N = 63          # below this a cloud is too small for a share of rounds / points to mean anything


def fps_m(N):
    """m = N runs the cloud to exhaustion (every later round is a tie at distance 0); above 1025 points m = 512."""
    return N if N <= 1025 else 512


def fps_plan(N):
    """(rc, (family name, T, PPT), slots) under the options in force."""
    rc, out = _plan("pdr_fps_plan", N)
    if rc != _lib.PDR_OK:
        return rc, None, None
    return rc, (FPS_FAMILIES[out[0]], out[1], out[2]), out[3]


def fps_cases():
    """(option set, N): every size under the defaults, and under each further option set where it selects another cell
    than under the sets before it."""
    cases, seen = [], {}
    for opt, opts in FPS_OPTION_SETS.items():
        with options(opts):
            for N in FPS_SIZES:
                rc, cell, _ = fps_plan(N)
                assert rc == _lib.PDR_OK, (opt, N, rc)
                if cell not in seen.setdefault(N, set()):
                    seen[N].add(cell)
                    cases.append((opt, N))
    return cases


def fps_input(N, kind):
    r = _rng(11, N, _seed(kind))
    if kind == "uniform":
        return r.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    if kind == "lattice":      # duplicates, exact ties, and the excluded origin
        return r.integers(0, lattice_side(N), (B, N, 3)).astype(np.float32)
    if kind == "near_origin":  # |p|^2 <= 1e-3 excludes a share of the points
        return r.uniform(-0.05, 0.05, (B, N, 3)).astype(np.float32)
    raise ValueError(kind)


def fps_tie_share(xyz, idx):
    """Share of the rounds whose maximum running distance is attained by more than one point, with the running
    distances recomputed in float64 along the picks `idx`; also checks that every pick attains that maximum (on integer
    coordinates float32 and float64 agree exactly, so this holds for the oracle on a lattice)."""
    ties = rounds = 0
    for b in range(xyz.shape[0]):
        p = xyz[b].astype(np.float64)
        excluded = (p * p).sum(1) <= 1e-3
        run = np.where(excluded, -1.0, 1e10)
        for j in range(1, idx.shape[1]):
            d = ((p - p[idx[b, j - 1]]) ** 2).sum(1)
            run = np.where(excluded, -1.0, np.minimum(run, d))
            mx = run.max()
            assert run[idx[b, j]] == mx, "cloud %d round %d: the pick does not attain the maximum" % (b, j)
            ties += int((run == mx).sum() > 1)
            rounds += 1
    return ties / max(rounds, 1)


@functools.lru_cache(maxsize=None)
def fps_reference(N, kind):
    """(xyz, the oracle's indices), read-only, after the input's precondition."""
    xyz = fps_input(N, kind)
    idx = O.furthest_point_sampling(xyz, fps_m(N))
    if N >= FPS_TIE_MIN_N and kind == "lattice":
        share = fps_tie_share(xyz, idx)
        assert share >= 0.5, "FPS lattice N=%d: only %.2f of the rounds are ties" % (N, share)
    if N >= FPS_TIE_MIN_N and kind == "near_origin":
        x = xyz.astype(np.float64)
        share = float(((x * x).sum(-1) <= 1e-3).mean())
        assert 0.05 <= share <= 0.5, "FPS near-origin N=%d: %.3f of the points excluded" % (N, share)
    return _frozen(xyz, idx)


# ====================================================================================================== kNN
KNN_FAMILIES = {0: "thread", 1: "wave", 2: "packed", -1: "none"}
KNN_OPTION_SETS = {"defaults": {}, "knn_wave=0": {"knn_wave": 0}}
KNN_KS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32)
KNN_N2 = (63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2500)
KNN_N1 = 300                 # a partial workgroup in every kernel
KNN_INPUTS = ("uniform", "lattice", "identical")
# qpw > 1 in the wave kernel needs B ceil(n1 / (4 qpw)) >= 1024: (B, n1, n2, K).  1000 = 15 * 64 + 40: at qpw = 16 the
# last workgroup has one partial and one empty wave; 1030 = 128 * 8 + 6: at qpw = 2 its last wave is empty
KNN_QPW_SHAPES = ([(64, 1000, n2, 8) for n2 in (64, 200)] +             # qpw 16: NCH 1, 4
                  [(8, 1030, n2, 8) for n2 in (64, 100, 300, 1000)])    # qpw 2: NCH 1, 2, 8, 16


def knn_shapes():
    """(B, n1, n2, K, return_nn): the K x n2 table (n2 = 1 and K - 1 give padding slots), K = 1 also without `nn`
    (the packed kernel), and the qpw > 1 shapes."""
    shapes = []
    for K in KNN_KS:
        for n2 in sorted(set((1, K - 1) + KNN_N2) - {0}):
            shapes.append((B, KNN_N1, n2, K, True))
            if K == 1:
                shapes.append((B, KNN_N1, n2, K, False))
    return shapes + [s + (True,) for s in KNN_QPW_SHAPES]


def knn_plan(shape, group=False):
    """(rc, cell) with cell = (family name, template parameter, qpw, workgroups per cloud)."""
    Bq, n1, n2, K, nn = shape
    rc, out = _plan("pdr_knn_plan", Bq, n1, n2, K, int(nn and not group), int(group))
    return rc, ((KNN_FAMILIES[out[0]],) + out[1:] if rc == _lib.PDR_OK else None)


def knn_group_applies(shape):
    return shape[4] and shape[3] <= min(shape[2], 16)


def knn_cases():
    """(option set, shape): every shape under the defaults, and with knn_wave = 0 where that changes the kernel of
    knn_points or of knn_group."""
    cases, first = [], {}
    for opt, opts in KNN_OPTION_SETS.items():
        with options(opts):
            for shape in knn_shapes():
                cell = (knn_plan(shape), knn_plan(shape, group=True) if knn_group_applies(shape) else None)
                if first.setdefault(shape, cell) != cell or opt == "defaults":
                    cases.append((opt, shape))
    return cases


def knn_input(shape, kind):
    Bq, n1, n2, K, _ = shape
    r = _rng(13, Bq, n1, n2, K, _seed(kind))
    x = r.uniform(-1, 1, (Bq, n1, 3)).astype(np.float32)
    if kind == "uniform":
        y = r.uniform(-1, 1, (Bq, n2, 3)).astype(np.float32)
    elif kind == "lattice":    # queries on the cloud's lattice: zero distances and ties at every rank
        g = lattice_side(n2)
        y = r.integers(0, g, (Bq, n2, 3)).astype(np.float32)
        x = r.integers(0, g, (Bq, n1, 3)).astype(np.float32)
    elif kind == "identical":  # every distance of a query is the same: the answer is the index order alone
        y = np.repeat(r.uniform(-1, 1, (Bq, 1, 3)), n2, axis=1).astype(np.float32)
    else:
        raise ValueError(kind)
    return x, y


@functools.lru_cache(maxsize=None)
def knn_reference(shape, kind):
    """(x, y, the oracle's squared distances, indices), read-only, after the input's precondition.  One reference
    serves knn_points with and without `nn` and knn_group."""
    Bq, n1, n2, K, _ = shape
    x, y = knn_input(shape[:4] + (True,), kind)
    d, i = O.knn(x, y, K)
    if kind == "lattice" and K < n2:
        d1, _ = O.knn(x, y, K + 1)
        assert np.array_equal(d1[..., :K], d)
        tie = float((d1[..., K - 1] == d1[..., K]).mean())
        zero = float((d[..., 0] == 0).mean())
        assert tie >= 0.5, "kNN lattice n2=%d K=%d: K-th = (K+1)-th distance for only %.2f of the queries" % (n2, K, tie)
        assert zero >= 0.5, "kNN lattice n2=%d K=%d: only %.2f of the queries have a zero distance" % (n2, K, zero)
    return _frozen(x, y, d, i)


# =============================================================================================== ball query
BALL_RESIDENT_NCH = (1, 2, 4, 8, 16, 32, 48, 64)
BALL_N = (63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097)
BALL_NS_AT_300 = (1, 2, 63, 64, 65, 128, 200)
BALL_M = 150
BALL_QPW_SHAPES = ((64, 1000, 100), (8, 1030, 3072))      # (B, m, n): qpw 16 and 2, m no multiple of 4 qpw


def ball_radius(n, ns, dense=False):
    return min(1.6, (6.0 * ns / n) ** (1.0 / 3.0)) if dense else min(1.2, (1.9 * ns / n) ** (1.0 / 3.0))


def ball_cases():
    """(B, m, n, nsample, radius)."""
    return ([(B, BALL_M, n, 16, ball_radius(n, 16)) for n in BALL_N] +
            [(B, BALL_M, 300, ns, ball_radius(300, ns, dense=True)) for ns in BALL_NS_AT_300] +
            [(Bq, m, n, 16, ball_radius(n, 16)) for Bq, m, n in BALL_QPW_SHAPES])


def ball_plan(case):
    """(rc, (NCH, resident, qpw, workgroups per cloud))."""
    return _plan("pdr_ball_query_plan", case[0], case[2], case[1])


def ball_input(case):
    """A uniform cloud on [-1, 1]^3; a third of the queries are copies of cloud points, a third uniform on [-1, 1]^3,
    a third uniform on [3, 4]^3 (empty balls: every radius here is below 2)."""
    Bq, m, n, ns, _ = case
    r = _rng(17, Bq, m, n, ns)
    xyz = r.uniform(-1, 1, (Bq, n, 3)).astype(np.float32)
    a = m // 3
    pick = r.integers(0, n, (Bq, a))
    q = np.concatenate([np.take_along_axis(xyz, pick[..., None], 1),
                        r.uniform(-1, 1, (Bq, a, 3)).astype(np.float32),
                        r.uniform(3, 4, (Bq, m - 2 * a, 3)).astype(np.float32)], 1)
    return np.ascontiguousarray(q), xyz


@functools.lru_cache(maxsize=None)
def ball_reference(case):
    """(queries, cloud, the oracle's indices, counts), read-only, after the preconditions."""
    q, xyz = ball_input(case)
    ns, radius = case[3], case[4]
    idx, cnt = O.ball_query(q, xyz, radius, ns)
    empty, full = float((cnt == 0).mean()), float((cnt == ns).mean())
    part = float(((cnt > 0) & (cnt < ns)).mean())
    assert empty >= 0.25, "ball query %r: %.2f empty balls" % (case, empty)
    assert full >= 0.05, "ball query %r: %.2f saturated balls" % (case, full)
    if ns >= 16:
        assert part >= 0.05, "ball query %r: %.2f partly filled balls" % (case, part)
    return _frozen(q, xyz, idx, cnt)
