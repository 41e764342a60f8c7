"""Forward plus backward of the Chamfer training loss: calc_cd_fused(...)[i].mean() (pdr_chamfer_loss /
pdr_chamfer_loss_grad) against calc_cd(...)[i].mean(), the composition it replaces, with the atomic and with the
deterministic backward kernels (pointnet2_ops.set_deterministic).  DESIGN section 7a.1, the protocol of 7a: device
events around one call (allocation included), 5 warm-up calls, 30 repetitions alternating between the variants,
medians, everything in one process.

    python tools/chamfer_loss_bench.py [--shapes 32x2048x2048,8x16384x16384] [--reps 30] [--warmup 5]
                                       [--only fused,parent_det] [--out profiles/chamfer_loss.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import calc_cd, calc_cd_fused  # noqa: E402
from point_diffusion_refinement_amd.pointnet2_ops import _ext  # noqa: E402

LOSSES = (("cd_t", 1), ("cd_p", 0))


def variants(out, gt, i):
    """name -> callable running one forward + backward; `out` requires a gradient (refined_X), gt does not (X)."""
    def fused():
        out.grad = None
        calc_cd_fused(out, gt)[i].mean().backward()

    def parent(deterministic):
        def run():
            out.grad = None
            prev = _ext.set_deterministic(deterministic)
            try:
                calc_cd(out, gt)[i].mean().backward()
            finally:
                _ext.set_deterministic(prev)
        return run
    return {"fused": fused, "parent_atomic": parent(False), "parent_det": parent(True)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="32x2048x2048,8x16384x16384")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variant names (default: all three)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chamfer_loss_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    lines = ["# %s, torch %s, reps %d, warm-up %d, ms per forward + backward (median [min .. max])"
             % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.warmup)]
    for shape in args.shapes.split(","):
        B, n1, n2 = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cpu").manual_seed(B * 1000003 + n1 * 101 + n2)
        gt = (torch.rand(B, n1, 3, generator=g) * 2 - 1).to(dev)
        out = (torch.rand(B, n2, 3, generator=g) * 2 - 1).to(dev).requires_grad_()
        for name, i in LOSSES:
            runs = variants(out, gt, i)
            if args.only:
                runs = {k: v for k, v in runs.items() if k in args.only.split(",")}
            grads = {}
            for k, fn in runs.items():
                for _ in range(args.warmup):
                    fn()
                grads[k] = out.grad.clone()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, fn in runs.items():                       # alternating
                    times[k].append(timed(fn))
            row = "%-16s %-5s" % (shape, name)
            for k in runs:
                t = times[k]
                row += "  %s %.3f [%.3f .. %.3f]" % (k, statistics.median(t), min(t), max(t))
            if "fused" in grads:
                for k in grads:
                    if k != "fused":
                        diff = (grads[k] - grads["fused"]).abs().max().item() / grads[k].abs().max().item()
                        row += "  max|grad - %s| / max|grad| %.2e" % (k, diff)
            print(row, flush=True)
            lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
