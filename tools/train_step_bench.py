"""Forward plus backward of the whole DDPM network on the module (trainable) path with an MSE loss on its output: all
five one-op switches off (set_fused_attention_pool, set_fused_group_norm, set_fused_grouping, set_fused_knn_grouping,
set_fused_score_norm) against all five on, against all five and set_fused_injection on (the setting "six", DESIGN
7a.9), and against those six and set_fused_score_conv on (the setting "seven").  DESIGN sections 7a.3 to
7a.7 each list this figure as not measured.

One child process per setting and round (--rounds > 1 alternates the settings: off, on, six, off, on, six, ..), each
under its own time limit; the first child that fails ends the run.  In a child:
PointNet2CloudCondition(ddpm_pointnet_config()) with seed 0, configs.synthetic_batch(B), a fixed random target; device
events around one forward + loss + backward (gradients cleared before, no optimiser step), warm-up steps, then
repetitions, the median; torch.cuda.max_memory_allocated over the timed steps.  Running out of device memory is a
RESULT ({"oom": true}), not an error.

    python tools/train_step_bench.py [--B 8] [--reps 10] [--warmup 3] [--limit 300] [--settings off,on,six] [--rounds 1]
                                     [--out profiles/train_step_injection.json]
    python tools/train_step_bench.py --settings off,six,seven --out profiles/train_step_score_conv.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWITCHES = ("set_fused_attention_pool", "set_fused_group_norm", "set_fused_grouping", "set_fused_knn_grouping",
            "set_fused_score_norm")
SETTINGS = {"off": (), "on": SWITCHES, "six": SWITCHES + ("set_fused_injection",),
            "seven": SWITCHES + ("set_fused_injection", "set_fused_score_conv")}


def measure(setting, B, reps, warmup):
    import torch
    from point_diffusion_refinement_amd import pointnet2_ops
    from point_diffusion_refinement_amd.pointnet2 import configs
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    if not torch.cuda.is_available():
        sys.exit("train_step_bench: no GPU (the module path has no CPU ops)")
    dev = torch.device("cuda:0")
    on = SETTINGS[setting]
    for name in SETTINGS["seven"]:
        getattr(pointnet2_ops, name)(name in on)
    torch.manual_seed(0)
    net = PointNet2CloudCondition(configs.ddpm_pointnet_config()).to(dev).train()
    x, cond, label = configs.synthetic_batch(B, device=dev)
    ts = torch.full((B,), 500.0, device=dev)
    row = {"setting": setting, "switches_on": [n[len("set_fused_"):] for n in on], "B": B, "oom": False}

    def step():
        net.zero_grad(set_to_none=True)
        net.reset_cond_features()
        out = net(x, cond, ts=ts, label=label)
        loss = torch.nn.functional.mse_loss(out, target)
        loss.backward()
        return loss

    try:
        with torch.no_grad():
            net.reset_cond_features()
            target = torch.randn_like(net(x, cond, ts=ts, label=label))
        for _ in range(warmup):
            loss = step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(reps):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = step()
            e.record()
            e.synchronize()
            times.append(a.elapsed_time(e))
        row.update(step_ms=statistics.median(times), step_ms_min=min(times), step_ms_max=max(times),
                   peak_bytes=torch.cuda.max_memory_allocated(), loss=float(loss))
    except torch.cuda.OutOfMemoryError:
        row.update(oom=True, peak_bytes=torch.cuda.max_memory_allocated())
    return row


def child(args_list, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("train_step_bench: %s ran into its time limit of %d s; stopping" % (what, limit))
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        sys.exit("train_step_bench: %s exited with %d; stopping" % (what, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one child process, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--settings", default="off,on,six", help="comma-separated: off | on (five switches) | six | seven")
    ap.add_argument("--rounds", type=int, default=1, help="processes per setting, the settings alternating")
    ap.add_argument("--one", default="", help="(child) measure one setting: off | on | six | seven")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(measure(args.one, args.B, args.reps, args.warmup)), flush=True)
        return
    settings = args.settings.split(",")
    if not settings or any(s not in SETTINGS for s in settings):
        ap.error("--settings takes a comma-separated list of %s" % ", ".join(SETTINGS))
    result = {"tool": "train_step_bench", "B": args.B, "reps": args.reps, "warmup": args.warmup,
              "rounds": args.rounds, "rows": []}
    for rnd in range(args.rounds):
        for setting in settings:
            row = child(["--one", setting, "--B", str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                        args.limit, "switches " + setting)
            row["round"] = rnd
            result["rows"].append(row)
            sys.stderr.write("round %d switches %-3s  %s\n" % (rnd, setting, "out of memory" if row["oom"] else
                             "%.1f ms  peak %.0f MiB" % (row["step_ms"], row["peak_bytes"] / 2 ** 20)))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
