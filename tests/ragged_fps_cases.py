"""The dispatch table of the length-aware FPS (csrc/fps_ragged.hip), the cases that walk it and the inputs they run on.
A plain module: tests/test_ragged_fps_host.py walks the table through pdr_fps_ragged_plan on the host,
tests/test_ragged_fps_gpu.py runs every case against oracle.pdr_oracle on each materialised slice.

A case is (N, mirror_axis, lengths, input kind, m): a padded batch of len(lengths) clouds of stride N whose padding rows
are NaN.  The walk has two levels, because the kernel chooses twice:
  * the HOST picks an instantiation (family, threads T, points per thread PPT) from V = N * (mirror ? 2 : 1);
    pdr_fps_ragged_plan reports it, and `instantiations` finds every one with the N range it serves;
  * inside a resident launch every WORKGROUP picks the round loop built for ceil(V_b / T) points per thread rounded up to
    one of LOOP_PPT.  The plan cannot report that (it never sees a length), so the steps are listed here.
As in tests/geometry_cases.py every reference comes with a precondition asserted on the oracle's result, and is computed
once per process and handed out read-only.
"""
import functools

import numpy as np

from oracle import pdr_oracle as O
from point_diffusion_refinement_amd import _lib
from tests.geometry_cases import FPS_INPUTS, FPS_TIE_MIN_N, _frozen, _plan, _rng, _seed, fps_tie_share, lattice_side

RAGGED_FAMILIES = ("resident", "stream")
RESIDENT_MAX_V = 12288
LOOP_PPT = (2, 4, 8, 12, 16)            # the round loops a resident workgroup chooses from (fps_ragged.hip)
OVER_ASK_MAX_N = 257


def ragged_plan(N, axis):
    """(rc, (family name, T, PPT), dynamic LDS bytes)."""
    rc, out = _plan("pdr_fps_ragged_plan", N, axis)
    if rc != _lib.PDR_OK:
        return rc, None, None
    return rc, (RAGGED_FAMILIES[out[0]], out[1], out[2]), out[3]


def virtual_size(N, axis):
    return N * (2 if axis >= 0 else 1)


@functools.lru_cache(maxsize=None)
def instantiations(mirror):
    """[(cell, smallest N, largest N)] for every resident instantiation the plan reports, in ascending N, found by
    asking the plan for every N up to the first one it hands to the stream kernel."""
    axis = 2 if mirror else -1
    found = []
    N = 1
    while True:
        rc, cell, _ = ragged_plan(N, axis)
        assert rc == _lib.PDR_OK, (N, axis, rc)
        if cell[0] == "stream":
            return tuple(found)
        if found and found[-1][0] == cell:
            found[-1][2] = N
        else:
            found.append([cell, N, N])
        N += 1
        assert N <= RESIDENT_MAX_V + 1, "the plan never reaches the stream kernel"


def default_lengths(N):
    return (N, N // 2 + 1, 1, 0)


def case_m(N, axis):
    return min(virtual_size(N, axis), 512)


def edge_sizes(mirror):
    """Every N at which a launch or a workgroup of a full cloud takes another path: 1, 2, the largest N of each
    instantiation and the next larger one, and the same for each round loop inside an instantiation."""
    f = 2 if mirror else 1
    sizes = {1, 2}
    for (_, T, PPT), lo, hi in instantiations(mirror):
        sizes |= {hi, hi + 1}
        for ppt in LOOP_PPT:
            n = T * ppt // f
            if ppt < PPT and lo <= n < hi:
                sizes |= {n, n + 1}
    return sorted(sizes)


# Round loops that no full cloud reaches -- the loops for 2 and 4 points per thread of the widest instantiation, whose
# own clouds start above them -- are reached by short clouds of a wide batch: lengths on both sides of each step.
def _short_cloud_cases():
    out = []
    for mirror, axis in ((False, -1), (True, 1)):
        (_, T, _), lo, hi = instantiations(mirror)[-1]
        f = 2 if mirror else 1
        N = lo + (hi - lo) // 8
        steps = [T * p // f for p in LOOP_PPT if T * p // f < lo]
        lengths = tuple(v for s in steps for v in (s, s + 1))
        out.append((N, axis, lengths, "lattice", 64))
    return out


@functools.lru_cache(maxsize=None)
def ragged_cases():
    cases = []
    for mirror in (False, True):
        inst_edges = {1, 2}
        for _, _, hi in instantiations(mirror):
            inst_edges |= {hi, hi + 1}
        for n_case, N in enumerate(edge_sizes(mirror)):
            axis = n_case % 3 if mirror else -1
            # every input kind at the instantiations' own edges, the tie-heavy lattice at the steps inside them
            kinds = FPS_INPUTS if N in inst_edges else ("lattice",)
            for kind in kinds:
                cases.append((N, axis, default_lengths(N), kind, case_m(N, axis)))
        for N in (2, 65, OVER_ASK_MAX_N):
            axis = 0 if mirror else -1
            cases.append((N, axis, default_lengths(N), "lattice", virtual_size(N, axis) + 5))
    cases += _short_cloud_cases()
    assert all(c[0] <= OVER_ASK_MAX_N for c in cases if c[4] > virtual_size(c[0], c[1]))
    return tuple(cases)


def case_id(case):
    N, axis, lengths, kind, m = case
    tail = "" if lengths == default_lengths(N) else "-L" + "_".join(map(str, lengths))
    return "N%d-ax%d-%s-m%d%s" % (N, axis, kind, m, tail)


def ragged_input(N, axis, lengths, kind):
    """(B,N,3) float32 with NaN in every padding row."""
    B, V = len(lengths), virtual_size(N, axis)
    r = _rng(29, N, axis + 1, B, _seed(kind))
    if kind == "uniform":
        xyz = r.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    elif kind == "lattice":      # duplicates, exact ties (more with a mirror: sites on the plane), the excluded origin
        xyz = r.integers(0, lattice_side(V), (B, N, 3)).astype(np.float32)
    elif kind == "near_origin":  # |p|^2 <= 1e-3 excludes a share of the points
        xyz = r.uniform(-0.05, 0.05, (B, N, 3)).astype(np.float32)
    else:
        raise ValueError(kind)
    for b, L in enumerate(lengths):
        xyz[b, L:] = np.nan
    return xyz


def virtual_cloud(cloud, L, axis):
    """(V_b,4) float32: the L originals with tag +1, then -- with a mirror -- their images with tag -1."""
    p = cloud[:L]
    rows = np.concatenate([p, np.ones((L, 1), np.float32)], 1)
    if axis < 0:
        return rows
    sign = np.ones(3, np.float32)
    sign[axis] = -1
    return np.concatenate([rows, np.concatenate([p * sign, -np.ones((L, 1), np.float32)], 1)], 0)


def slice_reference(cloud, L, axis, m):
    """(idx (m,) int32, rows (m,4) float32, the virtual cloud) of one cloud by the oracle; length 0: -1 / 0."""
    v = virtual_cloud(cloud, L, axis)
    if L == 0:
        return np.full(m, -1, np.int32), np.zeros((m, 4), np.float32), v
    idx = O.furthest_point_sampling(np.ascontiguousarray(v[None, :, :3]), m)[0].astype(np.int32)
    return idx, v[idx], v


@functools.lru_cache(maxsize=None)
def ragged_reference(case):
    """(xyz, the oracle's idx (B,m), the rows (B,m,4) gathered from the virtual clouds), read-only, after the input's
    preconditions (asserted per cloud, on the oracle's picks)."""
    N, axis, lengths, kind, m = case
    xyz = ragged_input(N, axis, lengths, kind)
    idx = np.empty((len(lengths), m), np.int32)
    rows = np.empty((len(lengths), m, 4), np.float32)
    for b, L in enumerate(lengths):
        idx[b], rows[b], v = slice_reference(xyz[b], L, axis, m)
        if len(v) < FPS_TIE_MIN_N:
            continue
        if kind == "lattice":
            share = fps_tie_share(v[None, :, :3], idx[b][None])
            assert share >= 0.5, "%s cloud %d: only %.2f of the rounds are ties" % (case_id(case), b, share)
        if kind == "near_origin":
            x = v[:, :3].astype(np.float64)
            share = float(((x * x).sum(-1) <= 1e-3).mean())
            assert 0.05 <= share <= 0.5, "%s cloud %d: %.3f of the points excluded" % (case_id(case), b, share)
    return _frozen(xyz, idx, rows)
