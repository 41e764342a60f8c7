"""Helper of test_jsd_host.py / test_jsd_gpu.py / golden/make_jsd_golden.py (not a test module): the numpy restatement
of the nearest-cell rule of pdr_occupancy_grid (include/pdr_hip.h) and the cloud makers the tests draw from.

The restatement builds its own grid tables, with the reference's arithmetic spelled out, and shares no code with
pointnet2/set_metrics.py:

    axis[i]  = float32(i * spacing - 0.5),  spacing = 1.0 / float(R - 1) in float64
    kept     = every cell, or those whose float32 numpy.linalg.norm is <= 0.5; compact index = rank in ascending
               (i R + j) R + k
    a point, widened to float64:
      per axis the first index of the smallest |axis[i] - p| (float64) -- lower index on a tie, clamped beyond the ends;
      that cell if it is kept (fast path), else the first kept cell of the smallest (dx dx + dy dy) + dz dz (float64).
    a point with a non-finite coordinate goes nowhere and is counted as skipped.
"""
import numpy as np


def tables(R, clip):
    """-> axis (R,) f32, cell_of (R,R,R) int64 (compact index or -1), kept_ijk (cells, 3) int64.  clip: False, True (the
    reference's sphere of radius 0.5) or a radius."""
    spacing = 1.0 / float(R - 1)
    axis = np.array([i * spacing - 0.5 for i in range(R)], dtype=np.float32)
    ijk = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1).reshape(-1, 3)
    keep = np.ones(R ** 3, dtype=bool)
    if clip:
        # float32 rows, as the reference's norm(grid, axis=1); `clip` may also be another radius than the reference's 0.5
        keep = np.linalg.norm(axis[ijk], axis=1) <= (0.5 if isinstance(clip, (bool, np.bool_)) else float(clip))
    cell_of = np.full(R ** 3, -1, dtype=np.int64)
    cell_of[keep] = np.arange(int(keep.sum()))
    return axis, cell_of.reshape(R, R, R), ijk[keep]


def nearest_cells(points, R, clip, return_gap=False):
    """points (n, 3) float32, all finite -> compact cell per point (n,) int64 and the mask of the slow-path points;
    with return_gap also, per point, second-smallest minus smallest float64 squared distance to a kept cell."""
    axis, cell_of, kept = tables(R, clip)
    a = axis.astype(np.float64)
    p = points.astype(np.float64)
    idx = [np.argmin(np.abs(a[None, :] - p[:, d, None]), axis=1) for d in range(3)]     # first minimum: lower index
    cell = cell_of[idx[0], idx[1], idx[2]]
    slow = cell < 0
    ka = a[kept]                                                  # (cells, 3) widened float32 coordinates
    gap = np.full(len(p), np.inf)
    todo = np.arange(len(p)) if return_gap else np.nonzero(slow)[0]
    for s in range(0, len(todo), 128):
        t = todo[s:s + 128]
        dx, dy, dz = (ka[None, :, d] - p[t, d, None] for d in range(3))
        d2 = dx * dx + dy * dy + dz * dz
        first = np.argmin(d2, axis=1)                             # first minimum: lowest compact index
        if return_gap and d2.shape[1] > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            gap[t] = two[:, 1] - two[:, 0]
        cell[t] = np.where(slow[t], first, cell[t])
    return (cell, slow, gap) if return_gap else (cell, slow)


def occupancy(clouds, R, clip, lengths=None):
    """clouds (S, n, 3) float32 -> dict(counters, bernoulli (cells,) int64, skipped, slow_share)"""
    cells = len(tables(R, clip)[2])
    counters, bernoulli = np.zeros(cells, dtype=np.int64), np.zeros(cells, dtype=np.int64)
    skipped = n_slow = n_points = 0
    for s, cloud in enumerate(clouds):
        if lengths is not None:
            cloud = cloud[:max(0, min(int(lengths[s]), len(cloud)))]
        finite = np.isfinite(cloud).all(axis=1)
        skipped += int((~finite).sum())
        cell, slow = nearest_cells(cloud[finite], R, clip)
        np.add.at(counters, cell, 1)
        bernoulli[np.unique(cell)] += 1
        n_slow += int(slow.sum())
        n_points += int(finite.sum())
    return {"counters": counters, "bernoulli": bernoulli, "skipped": skipped,
            "slow_share": n_slow / max(n_points, 1)}


# ---- cloud makers: (S, n, 3) float32 ---------------------------------------------------------------------------------

def ball(rng, S, n):
    """uniform in the interior of the ball of radius 0.5"""
    v = rng.normal(size=(S, n, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    return (v * 0.5 * rng.uniform(size=(S, n, 1)) ** (1.0 / 3.0)).astype(np.float32)


def cube(rng, S, n):
    return rng.uniform(-0.5, 0.5, size=(S, n, 3)).astype(np.float32)


def shell(rng, S, n):
    """on the sphere of radius 0.5: a surface normalised to the unit sphere"""
    v = rng.normal(size=(S, n, 3))
    return (v * 0.5 / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)


def wide(rng, S, n):
    """sticks out of the cube: exercises the clamping of the per-axis index"""
    return rng.uniform(-0.8, 0.8, size=(S, n, 3)).astype(np.float32)


MAKERS = {"ball": ball, "cube": cube, "shell": shell, "wide": wide}
