"""Forward plus backward of the front of AttentionModule's score head with set_fused_score_norm on (the op
pointnet2_utils.relu_group_norm: pdr_relu_group_norm_cf / pdr_relu_group_norm_cf_grad) against the switch off (the
torch composition: expand, cat, in-place ReLU, MyGroupNorm), at the head shapes of the DDPM network with B = 32.
DESIGN section 7a.7.

The shapes come from pointnet2/configs.py: a probe process builds PointNet2CloudCondition(ddpm_pointnet_config()),
runs one forward of the module path at B = 2 with a hook on every AttentionModule, and records (C1, C2, the width
between weight_conv's two convs, N, K) -- every head the network runs, not a hand-kept list.  Each distinct head gives
two rows:
    "first":   q (B, C1, N) and k (B, C2, N, K) -> expand + cat + weight_conv[0] (ReLU) + weight_conv[1] (MyGroupNorm)
    "second":  h (B, inter, N, K)               -> weight_conv[3] (ReLU) + weight_conv[4] (MyGroupNorm)
The convolutions are not part of either row.  In the module the second link's input is a convolution's output, which
the in-place ReLU may overwrite; here it is a leaf, handed over through an identity Function that returns an alias of
it, so that the composition runs its in-place ReLU as in the module (the leaf's values are rectified by the first
call; neither variant's time depends on the values).

Protocol (that of tools/group_norm_act_bench.py): one child process per distinct head, each under its own time limit;
the first child that fails ends the run (nothing is tried again).  In a child: device events around one forward +
backward through autograd (allocation included), warm-up calls, then repetitions alternating between the variants,
medians; torch.cuda.max_memory_allocated of one forward + backward of each, taken after the warm-up with the inputs
already resident (`resident_bytes`).  Three variants: "op" (switch on), "composition" (switch off, the parent commit's
behaviour) and "composition_fused_gn" (switch off with set_fused_group_norm(True): the composition's best form).

    python tools/score_norm_bench.py [--B 32] [--reps 30] [--warmup 5] [--limit 120] [--out profiles/relu_group_norm.json]
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


def probe():
    """[{"C1", "C2", "inter", "G1", "G2", "N", "K", "heads"}]: the distinct score heads of one forward of the network."""
    import torch
    from point_diffusion_refinement_amd.pointnet2 import configs
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule, MyGroupNorm
    if not torch.cuda.is_available():
        sys.exit("score_norm_bench: no GPU (the module path has no CPU ops)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet2CloudCondition(configs.ddpm_pointnet_config()).to(dev)
    seen = {}

    def hook(m, args):
        wc = m.weight_conv
        if len(wc) != 6 or not isinstance(wc[1], MyGroupNorm):
            return
        gf = args[1]
        key = (m.feat_conv.out_channels, m.grouped_feat_conv.out_channels, wc[2].out_channels, wc[1].num_groups,
               wc[4].num_groups, int(gf.shape[2]), int(gf.shape[3]))
        seen[key] = seen.get(key, 0) + 1

    for m in net.modules():
        if isinstance(m, AttentionModule):
            m.register_forward_pre_hook(hook)
    B = 2
    x, cond, label = configs.synthetic_batch(B, device=dev)
    with torch.no_grad():
        net.reset_cond_features()
        net(x, cond, ts=torch.full((B,), 500.0, device=dev), label=label)
    torch.cuda.synchronize()
    names = ("C1", "C2", "inter", "G1", "G2", "N", "K")
    return [dict(zip(names, k), heads=n) for k, n in sorted(seen.items())]


def measure(link, C1, C2, G, N, K, B, reps, warmup):
    """One link of one head, in this process: the dict of the module docstring."""
    import torch
    from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
    from point_diffusion_refinement_amd.pointnet2_ops.attention import MyGroupNorm, NormActSequential
    if not torch.cuda.is_available():
        sys.exit("score_norm_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    C = C1 + C2
    g = torch.Generator(device=dev).manual_seed(C1 * 1000003 + C2 * 101 + N * 7 + K)
    q = torch.randn(B, C1, N, device=dev, generator=g).requires_grad_() if C1 else None
    k = torch.randn(B, C2, N, K, device=dev, generator=g).requires_grad_()
    stack = NormActSequential(torch.nn.ReLU(inplace=True), MyGroupNorm(G, C)).to(dev)     # weight_conv[0:2] / [3:5]
    gn = stack[1].group_norm
    with torch.no_grad():
        gn.weight.add_(0.1 * torch.randn(gn.weight.shape, device=dev, generator=g))
        gn.bias.add_(0.1 * torch.randn(gn.bias.shape, device=dev, generator=g))
    grad_out = torch.randn(B, C, N, K, device=dev, generator=g)
    leaves = [t for t in (q, k, gn.weight, gn.bias) if t is not None]

    class Alias(torch.autograd.Function):                    # a non-leaf that shares the leaf's storage
        @staticmethod
        def forward(ctx, t):
            return t.detach()

        @staticmethod
        def backward(ctx, grad):
            return grad

    def clear():
        for t in leaves:
            t.grad = None

    def op():
        clear()
        pointnet2_utils.relu_group_norm(k, gn.weight, gn.bias, G, gn.eps, q=q).backward(grad_out)

    def composition():                                       # AttentionModule.forward's lines, as at the parent commit
        clear()
        x = torch.cat([q.unsqueeze(-1).expand(-1, -1, -1, K), k], dim=1) if C1 else Alias.apply(k)
        stack(x).backward(grad_out)

    def composition_fused_gn():
        prev = _ext.set_fused_group_norm(True)
        try:
            composition()
        finally:
            _ext.set_fused_group_norm(prev)

    runs = {"op": op, "composition": composition, "composition_fused_gn": composition_fused_gn}

    def timed(fn):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e)

    grads, peak, diff = {}, {}, {}
    for name in ("composition", "composition_fused_gn", "op"):   # the op last: the second link's leaf is rectified by then
        for _ in range(warmup):
            runs[name]()
        grads[name] = [t.grad.clone() for t in leaves]
    for i, name in enumerate((["q"] if C1 else []) + ["k", "weight", "bias"]):   # same results before any timing
        a, b = grads["op"][i], grads["composition"][i]
        diff[name] = ((a - b).abs().max() / b.abs().max()).item()
    del grads, a, b
    clear()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()                 # the inputs, the parameters and grad_out
    for name, fn in runs.items():
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
        clear()
    times = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():                        # alternating
            times[name].append(timed(fn))
    row = {"link": link, "shape": [B, C, N, K], "C1": C1, "C2": C2, "G": G, "resident_bytes": resident,
           "output_bytes": B * C * N * K * 4}
    for name in runs:
        row[name + "_ms"] = statistics.median(times[name])
        row[name + "_ms_min"], row[name + "_ms_max"] = min(times[name]), max(times[name])
        row[name + "_peak_bytes"] = peak[name]
    for name, d in diff.items():
        row["max_grad_%s_diff_over_max" % name] = d
    return row


def child(args_list, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("score_norm_bench: %s ran into its time limit of %d s; stopping" % (what, limit))
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        sys.exit("score_norm_bench: %s exited with %d; stopping" % (what, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child process, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--probe", action="store_true", help="(child) print the network's score heads as JSON")
    ap.add_argument("--one", default="", help="(child) measure C1:C2:inter:G1:G2:N:K, e.g. 32:137:64:32:32:2048:32")
    ap.add_argument("--list", action="store_true", help="print the heads and exit")
    args = ap.parse_args()
    if args.probe:
        print(json.dumps(probe()), flush=True)
        return
    if args.one:
        C1, C2, inter, G1, G2, N, K = (int(v) for v in args.one.split(":"))
        print(json.dumps([measure("first", C1, C2, G1, N, K, args.B, args.reps, args.warmup),
                          measure("second", 0, inter, G2, N, K, args.B, args.reps, args.warmup)]), flush=True)
        return
    heads = child(["--probe"], args.limit, "the probe")
    if args.list:
        for h in heads:
            print("C1 %d  C2 %d  inter %d  N %d  K %d  %d heads" % (h["C1"], h["C2"], h["inter"], h["N"], h["K"], h["heads"]))
        return
    result = {"tool": "score_norm_bench", "B": args.B, "reps": args.reps, "warmup": args.warmup,
              "heads_per_forward": sum(h["heads"] for h in heads), "rows": []}
    for h in heads:                                          # a child per distinct head, its two links in turn
        one = ":".join(str(h[n]) for n in ("C1", "C2", "inter", "G1", "G2", "N", "K"))
        rows = child(["--one", one, "--B", str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                     args.limit, one)
        for row in rows:
            row["heads_in_network"] = h["heads"]
            result["rows"].append(row)
            sys.stderr.write("%-28s %-6s op %.3f ms  composition %.3f ms  with fused group norm %.3f ms\n"
                             % (one, row["link"], row["op_ms"], row["composition_ms"], row["composition_fused_gn_ms"]))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
