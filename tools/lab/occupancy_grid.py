"""Occupancy-grid kernel (set_metrics.OccupancyGrid -> pdr_occupancy_grid): time of one launch over a set, on clouds
that almost never and clouds that mostly take the slow path of the nearest-cell rule.

    python -m tools.lab.occupancy_grid [--sets 1000] [--points 2048] [--resolution 28] [--repeats 7] [--launches 50]
                                       [--out profiles/jsd_occupancy.json]

Two sets of `sets` clouds of `points` points: uniform in the interior of the ball of radius 0.5 (about 3 % of the points
find their separable cell clipped away) and on its surface (about 60 %).  A launch takes a fraction of a millisecond,
so a timed window is `launches` back-to-back launches into the same counters between two device events (the counters
are allocated and zeroed before the first event) and the time per launch is reported; two warm-up windows per set,
then `repeats` rounds alternating the two sets; the median of each is recorded with its spread.  The slow-path shares come from the numpy
restatement of the rule (tests/occupancy_cases.py) on the first 8 clouds of each set, and the first 8 clouds' counters
are compared with it before anything is timed.  There is nothing to compare the times against: the reference's loop
needs sklearn on the host and is not run here.
"""
import argparse
import json
import statistics

import numpy as np
import torch

from tests import occupancy_cases as OC


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1000)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50, help="launches per timed window")
    ap.add_argument("--out", default="profiles/jsd_occupancy.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU path"
    from point_diffusion_refinement_amd.pointnet2 import set_metrics as SM
    from point_diffusion_refinement_amd.pointnet2_ops import _ext

    rng = np.random.default_rng(0)
    axis, cell_of, cells = SM.grid_tables(a.resolution, True, "cuda")
    sets, share = {}, {}
    for kind in ("ball", "shell"):
        clouds = OC.MAKERS[kind](rng, a.sets, a.points)
        sets[kind] = torch.from_numpy(clouds).cuda()
        head = OC.occupancy(clouds[:8], a.resolution, True)
        share[kind] = head["slow_share"]
        got = _ext.occupancy_grid(sets[kind][:8].contiguous(), axis, cell_of, cells)
        assert np.array_equal(got[0].cpu().numpy(), head["counters"]) and int(got[2][0]) == 0, kind

    def timed(x):
        out = tuple(torch.zeros(k, dtype=torch.int32, device="cuda") for k in (cells, cells, 1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            _ext.occupancy_grid(x, axis, cell_of, cells, out=out)
        e1.record()
        torch.cuda.synchronize()
        assert int(out[0].sum()) == a.launches * x.shape[0] * x.shape[1]
        return e0.elapsed_time(e1) / a.launches

    ms = {k: [] for k in sets}
    for rnd in range(2 + a.repeats):
        for k, x in sets.items():
            t = timed(x)
            if rnd >= 2:
                ms[k].append(t)
    result = {"device": torch.cuda.get_device_name(0), "sets": a.sets, "points": a.points,
              "resolution": a.resolution, "cells": cells, "repeats": a.repeats, "launches_per_window": a.launches,
              "method": "device events around a window of back-to-back launches, time per launch; 2 warm-up windows, "
                        "median of alternating rounds"}
    for k in sets:
        med = statistics.median(ms[k])
        result[k] = {"ms": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
                     "us_per_cloud": round(1e3 * med / a.sets, 4), "slow_path_share": round(share[k], 4)}
    result["shell_over_ball"] = round(result["shell"]["ms"] / result["ball"]["ms"], 3)
    text = json.dumps(result, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
