"""Forward plus backward of one [ReLU, MyGroupNorm, Conv2d 1x1] link of AttentionModule's score head by three routes, at
the head shapes of the DDPM network with B = 32.  DESIGN section 7a.11.
    "composition":  expand + cat + in-place ReLU + MyGroupNorm + Conv2d            (every switch off)
    "norm_op":      pointnet2_utils.relu_group_norm + Conv2d                       (set_fused_score_norm)
    "op":           pointnet2_utils.relu_group_norm_conv                           (set_fused_score_conv)

The shapes come from pointnet2/configs.py, as in tools/score_norm_bench.py: a probe process builds
PointNet2CloudCondition(ddpm_pointnet_config()), runs one forward of the module path at B = 2 with a hook on every
AttentionModule and records (C1, C2, the width between weight_conv's two convs, the head's output width, N, K).  Each
distinct head gives two rows:
    "first":   q (B, C1, N), k (B, C2, N, K) -> weight_conv[0:3]  (C1 + C2 -> inter)
    "second":  h (B, inter, N, K)            -> weight_conv[3:6]  (inter -> C_out)
In the module the second link's input is a convolution's output, which the in-place ReLU may overwrite; here it is a
leaf handed over through an identity Function that returns an alias of it (tools/score_norm_bench.py).

Protocol (that of tools/score_norm_bench.py): one child process per distinct head, each under its own time limit; the
first child that fails ends the run.  In a child: the three routes' outputs and gradients are compared BEFORE any timing
(an assertion: relative to the largest element, at most 1e-4); device events around one forward + backward through
autograd (allocation included), warm-up calls, then repetitions alternating between the routes: median, min, max;
torch.cuda.max_memory_allocated of one forward + backward of each, taken after the warm-up with the inputs already
resident (`resident_bytes`).  The sums over the network's heads (row x heads_in_network) are recorded too.

    python tools/score_conv_bench.py [--B 32] [--reps 20] [--warmup 3] [--limit 180] [--out profiles/relu_group_norm_conv.json]
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

ROUTES = ("composition", "norm_op", "op")
NAMES = ("C1", "C2", "inter", "Cout", "G1", "G2", "N", "K")


def probe():
    """[{C1, C2, inter, Cout, G1, G2, N, K, heads}]: the distinct score heads of one forward of the network."""
    import torch
    from point_diffusion_refinement_amd.pointnet2 import configs
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule, MyGroupNorm
    if not torch.cuda.is_available():
        sys.exit("score_conv_bench: no GPU (the module path has no CPU ops)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet2CloudCondition(configs.ddpm_pointnet_config()).to(dev)
    seen = {}

    def hook(m, args):
        wc = m.weight_conv
        if len(wc) != 6 or not isinstance(wc[1], MyGroupNorm):
            return
        gf = args[1]
        key = (m.feat_conv.out_channels, m.grouped_feat_conv.out_channels, wc[2].out_channels, wc[5].out_channels,
               wc[1].num_groups, wc[4].num_groups, int(gf.shape[2]), int(gf.shape[3]))
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
    return [dict(zip(NAMES, k), heads=n) for k, n in sorted(seen.items())]


def measure(link, C1, C2, G, Cout, N, K, B, reps, warmup):
    """One link of one head, in this process: the dict of the module docstring."""
    import torch
    from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
    from point_diffusion_refinement_amd.pointnet2_ops.attention import MyGroupNorm, NormActSequential
    if not torch.cuda.is_available():
        sys.exit("score_conv_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    C = C1 + C2
    if not _ext.relu_group_norm_conv_supported(C1, (B, C2, N, K), G, Cout):
        sys.exit("score_conv_bench: the op does not take %s" % ((B, C1, C2, N, K, G, Cout),))
    g = torch.Generator(device=dev).manual_seed(C1 * 1000003 + C2 * 101 + N * 7 + K)
    q = torch.randn(B, C1, N, device=dev, generator=g).requires_grad_() if C1 else None
    k = torch.randn(B, C2, N, K, device=dev, generator=g).requires_grad_()
    stack = NormActSequential(torch.nn.ReLU(inplace=True), MyGroupNorm(G, C),
                              torch.nn.Conv2d(C, Cout, kernel_size=1)).to(dev)             # weight_conv[0:3] / [3:6]
    gn, conv = stack[1].group_norm, stack[2]
    with torch.no_grad():
        gn.weight.add_(0.1 * torch.randn(gn.weight.shape, device=dev, generator=g))
        gn.bias.add_(0.1 * torch.randn(gn.bias.shape, device=dev, generator=g))
    grad_out = torch.randn(B, Cout, N, K, device=dev, generator=g)
    leaves = [t for t in (q, k, gn.weight, gn.bias, conv.weight, conv.bias) if t is not None]
    leaf_names = (["q"] if C1 else []) + ["k", "gamma", "beta", "conv_weight", "conv_bias"]

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

    def composition():                                       # AttentionModule.score_head's lines with every switch off
        clear()
        x = torch.cat([q.unsqueeze(-1).expand(-1, -1, -1, K), k], dim=1) if C1 else Alias.apply(k)
        out = stack(x)
        out.backward(grad_out)
        return out

    def norm_op():                                           # ... with set_fused_score_norm
        clear()
        out = conv(pointnet2_utils.relu_group_norm(k, gn.weight, gn.bias, G, gn.eps, q=q))
        out.backward(grad_out)
        return out

    def op():                                                # ... with set_fused_score_conv
        clear()
        out = pointnet2_utils.relu_group_norm_conv(k, gn.weight, gn.bias, G, gn.eps, conv.weight.view(Cout, C), conv.bias,
                                                   q=q)
        out.backward(grad_out)
        return out

    runs = {"composition": composition, "norm_op": norm_op, "op": op}

    def timed(fn):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e)

    results, peak, diff = {}, {}, {}
    for name in ROUTES:                                      # the ops last: the second link's leaf is rectified by then
        for _ in range(max(warmup, 1)):
            out = runs[name]()
        results[name] = [out.detach().clone()] + [t.grad.clone() for t in leaves]
        del out
    for other in ("composition", "norm_op"):                 # equal results before any timing
        for name, a, b in zip(["out"] + leaf_names, results["op"], results[other]):
            d = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
            diff["%s_vs_%s" % (name, other)] = d
            assert d <= 1e-4, (link, name, other, d)
    del results, a, b
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
    row = {"link": link, "shape": [B, C, N, K], "C1": C1, "C2": C2, "G": G, "Cout": Cout, "resident_bytes": resident,
           "normalised_bytes": B * C * N * K * 4, "output_bytes": B * Cout * N * K * 4}
    for name in runs:
        row[name + "_ms"] = statistics.median(times[name])
        row[name + "_ms_min"], row[name + "_ms_max"] = min(times[name]), max(times[name])
        row[name + "_peak_bytes"] = peak[name]
    row["max_diff_over_max"] = max(diff.values())
    return row


def child(args_list, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("score_conv_bench: %s ran into its time limit of %d s; stopping" % (what, limit))
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        sys.exit("score_conv_bench: %s exited with %d; stopping" % (what, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="time limit of one child process, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--probe", action="store_true", help="(child) print the network's score heads as JSON")
    ap.add_argument("--one", default="", help="(child) measure C1:C2:inter:Cout:G1:G2:N:K")
    ap.add_argument("--list", action="store_true", help="print the heads and exit")
    args = ap.parse_args()
    if args.probe:
        print(json.dumps(probe()), flush=True)
        return
    if args.one:
        C1, C2, inter, Cout, G1, G2, N, K = (int(v) for v in args.one.split(":"))
        print(json.dumps([measure("first", C1, C2, G1, inter, N, K, args.B, args.reps, args.warmup),
                          measure("second", 0, inter, G2, Cout, N, K, args.B, args.reps, args.warmup)]), flush=True)
        return
    heads = child(["--probe"], args.limit, "the probe")
    if args.list:
        for h in heads:
            print("  ".join("%s %d" % (n, h[n]) for n in NAMES) + "  %d heads" % h["heads"])
        return
    result = {"tool": "score_conv_bench", "B": args.B, "reps": args.reps, "warmup": args.warmup,
              "heads_per_forward": sum(h["heads"] for h in heads), "rows": []}
    for h in heads:                                          # a child per distinct head, its two links in turn
        one = ":".join(str(h[n]) for n in NAMES)
        rows = child(["--one", one, "--B", str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                     args.limit, one)
        for row in rows:
            row["heads_in_network"] = h["heads"]
            result["rows"].append(row)
            sys.stderr.write("%-34s %-6s composition %.3f ms  norm op + conv %.3f ms  op %.3f ms   peak MiB %.0f %.0f %.0f\n"
                             % ((one, row["link"]) + tuple(row[r + "_ms"] for r in ROUTES)
                                + tuple(row[r + "_peak_bytes"] / 2 ** 20 for r in ROUTES)))
    for r in ROUTES:
        result["sum_%s_ms" % r] = sum(row[r + "_ms"] * row["heads_in_network"] for row in result["rows"])
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
