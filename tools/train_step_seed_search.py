"""The CPU figures behind the inputs of tests/test_train_step_f64_host.py / _gpu.py and of
tests/test_refine_step_f64_host.py / _gpu.py (section 7a.10), per input seed:

  * the smallest top-1 / top-2 gap of the two max-over-points reductions of the global PointNet in the float64 run
    (the decision that stays unpinned; a case's seed must keep it at 1e-4 or more),
  * on how many ReLU mask elements an fp32 and a float64 evaluation of one step disagree, and the worst gradient error
    of the fp32 step against float64 on its own masks (unpinned) and under the fp32 masks (pinned),
  * --stage refine: the same for the refinement step of a head variant and a Chamfer loss type (no regime: its inputs
    are tests/refine_step_cases.py `inputs`), with the figures of the Chamfer tape -- queries whose taped neighbour is
    not float64's own, the largest ratio to the honesty bound, delta, the smallest nearest-neighbour distance -- and
    the pinned errors of the parameter gradients / records / output / loss and of the displacement gradient.

Everything runs on the CPU through tests/float64_network.py (`float64_ops("oracle")`); no GPU is used.

    python tools/train_step_seed_search.py [--activation relu] [--regime noise] [--seeds 1 2 3 4 5 6 7] [--threads 0]
    python tools/train_step_seed_search.py --stage refine [--variant up4] [--loss cd_t] [--activation relu] ...
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def refine(args):
    from tests import refine_step_cases as RC
    for seed in args.seeds:
        r = RC.cpu_runs(args.variant, args.loss, args.activation, seed)
        e = RC.errors(r["r32"], r["pinned"])
        h = r["honesty"]
        print("refine %s %s %s seed %d: gaps %s; %d sites, %d elements, %d differ; Chamfer tape: %d terms, %d queries "
              "differ from float64's own search (%d from its tape), ratio %.2f, delta %.1e, nearest %.1e; pinned "
              "gradients / records / output / loss %.2e %.2e %.2e %.2e, displacement gradient %.2e" % (
                  (args.variant, args.loss, args.activation, seed, {k: "%.1e (%d dead)" % v for k, v in r["gaps"].items()},
                   len(r["tape32"]), r["tape32"].elements(), r["tape32"].differing(r["tape64"]), len(r["chamfer32"]),
                   h["differing"],
                   sum(int((a[k] != b[k]).sum()) for a, b in zip(r["chamfer32"].terms, r["chamfer64"].terms)
                       for k in ("idx_gt", "idx_out")), h["ratio"], h["delta"], h["nearest"])
                  + RC.summary(e) + (e["grad:displacement"],)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stage", default="ddpm", choices=("ddpm", "refine"))
    ap.add_argument("--activation", default="relu", choices=("relu", "swish"))
    ap.add_argument("--regime", default="noise", choices=("noise", "surface"))
    ap.add_argument("--variant", default="up4", choices=("plain", "up4", "up4c"), help="head variant (--stage refine)")
    ap.add_argument("--loss", default="cd_t", choices=("cd_t", "cd_p"), help="Chamfer loss type (--stage refine)")
    ap.add_argument("--seeds", type=int, nargs="+", default=list(range(1, 8)))
    ap.add_argument("--threads", type=int, default=0, help="torch.set_num_threads (0: leave it)")
    args = ap.parse_args()
    import torch
    from oracle import pdr_oracle
    from tests import float64_network as F64
    from tests import train_step_cases as TC
    pdr_oracle.build()
    if args.threads:
        torch.set_num_threads(args.threads)
    if args.stage == "refine":
        return refine(args)
    net = TC.network(args.activation)
    f64 = F64.float64_model(net)
    for seed in args.seeds:
        data = TC.inputs(args.regime, seed)
        with F64.float64_ops("oracle", dtype=torch.float32), F64.relu_tape("record") as tape32:
            r32 = TC.step(net, data)
        with F64.float64_ops("oracle"), F64.relu_tape("record") as tape64, F64.record_max_gaps(f64) as gaps:
            r64 = TC.step(f64, data)
        with F64.float64_ops("oracle"), F64.relu_tape("replay", tape32):
            pinned = TC.step(f64, data)
        print("%s %s seed %d: gaps %s; %d sites, %d elements, %d differ; gradients / records / output unpinned "
              "%.2e %.2e %.2e, pinned %.2e %.2e %.2e" % (
                  (args.activation, args.regime, seed,
                   {k: "%.1e (%d dead)" % v for k, v in gaps.items()}, len(tape32), tape32.elements(),
                   tape32.differing(tape64)) + TC.summary(TC.errors(r32, r64)) + TC.summary(TC.errors(r32, pinned))),
              flush=True)


if __name__ == "__main__":
    main()
