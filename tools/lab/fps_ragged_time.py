"""mirror_and_concat, dense against the one-launch length-aware form, at the producer's size (B = 32, N = 2048 ->
2048 and 3072 points):

    python -m tools.lab.fps_ragged_time [--reps 60] [--out FILE.json]

  (a) dense      mirror_and_concat(partial): the (B,2N,4) concat, FPS to 2048 and to 3072, two transposed gathers
  (b) full       mirror_and_concat(partial, lengths = N everywhere): the concat and ONE 3072-round launch
  (c) half       the same with every length at N / 2: do short clouds pay for the padding?
  (b') / (c')    the FPS launch of (b) / (c) alone, without the torch code around it

Device events around one call, after a warm-up, the versions ALTERNATING inside one process; per version the median and
the spread (5th / 95th percentile, min) over the repetitions.  The outputs of (a) and (b) are compared bit for bit
before anything is timed.
"""
import argparse
import json

import numpy as np
import torch

from point_diffusion_refinement_amd.pointnet2.data_utils import mirror_partial
from point_diffusion_refinement_amd.pointnet2_ops import _ext

B, N, NUM_POINTS, AXIS = 32, 2048, (2048, 3072), 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("at least 50 repetitions per version")
    if not torch.cuda.is_available():
        raise SystemExit("fps_ragged_time needs a GPU: a CPU run measures nothing")

    g = torch.Generator().manual_seed(0)
    partial = (torch.rand(B, N, 3, generator=g) - 0.5).cuda()
    full = torch.full((B,), N, dtype=torch.int64, device="cuda")
    half = torch.full((B,), N // 2, dtype=torch.int64, device="cuda")
    m = max(NUM_POINTS)
    versions = {
        "a_dense": lambda: mirror_partial.mirror_and_concat(partial, AXIS, NUM_POINTS),
        "b_full": lambda: mirror_partial.mirror_and_concat(partial, AXIS, NUM_POINTS, lengths=full),
        "c_half": lambda: mirror_partial.mirror_and_concat(partial, AXIS, NUM_POINTS, lengths=half),
        "b_full_fps_only": lambda: _ext.furthest_point_sampling_ragged(partial, m, lengths=full, mirror_axis=AXIS,
                                                                       return_rows=True),
        "c_half_fps_only": lambda: _ext.furthest_point_sampling_ragged(partial, m, lengths=half, mirror_axis=AXIS,
                                                                       return_rows=True),
    }
    for d, r in zip(versions["a_dense"](), versions["b_full"]()):
        assert torch.equal(d.view(torch.int32), r.view(torch.int32)), "dense and length-aware outputs differ"
    for _ in range(args.warmup):
        for fn in versions.values():
            fn()
    torch.cuda.synchronize()

    times = {name: [] for name in versions}
    for _ in range(args.reps):
        for name, fn in versions.items():           # alternating: drift of the clocks hits every version alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)

    result = {"B": B, "N": N, "num_points": NUM_POINTS, "axis": AXIS, "reps": args.reps, "unit": "us", "versions": {}}
    print("%-18s %9s %9s %9s %9s" % ("version", "median", "p05", "p95", "min"))
    for name, t in times.items():
        t = np.asarray(t)
        row = {"median": float(np.median(t)), "p05": float(np.percentile(t, 5)), "p95": float(np.percentile(t, 95)),
               "min": float(t.min())}
        result["versions"][name] = row
        print("%-18s %9.1f %9.1f %9.1f %9.1f" % (name, row["median"], row["p05"], row["p95"], row["min"]))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
