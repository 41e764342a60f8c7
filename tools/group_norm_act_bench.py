"""Forward plus backward of MyGroupNorm + activation as one op (pointnet2_utils.group_norm_act: pdr_group_norm_act /
pdr_group_norm_act_grad) against the torch composition it replaces (nn.GroupNorm, the slice and cat when C % G != 0,
ReLU or x * sigmoid(x)), at the link shapes of the DDPM network with B = 32.  DESIGN section 7a.4.

The shapes come from pointnet2/configs.py: a probe process builds PointNet2CloudCondition(ddpm_pointnet_config()),
runs one forward of the module path at B = 2 with a hook on every MyGroupNorm, and records (C, trailing dimensions,
groups, the activation that follows it in its stack) -- every link the network runs, not a hand-kept list.  Distinct
(C, N, K, G) shapes are then measured at B = --B for ReLU and Swish, whichever the network itself uses there.

Protocol (that of tools/attention_pool_bench.py): one child process per distinct tensor shape, each under its own time limit;
the first child that fails ends the run (nothing is tried again).  In a child: device events around one forward +
backward through autograd (allocation included), warm-up calls, then repetitions alternating between the two variants,
medians; torch.cuda.max_memory_allocated of one forward + backward of each, taken after the warm-up with the inputs
already resident (`resident_bytes`).  `op_gbytes_per_s` is the bytes the op's five kernels must move -- forward 2 reads
and 1 write of the tensor, backward 4 reads and 1 write: 32 bytes per element -- over the op's time, which also holds
the allocations and autograd's bookkeeping.

    python tools/group_norm_act_bench.py [--B 32] [--reps 30] [--warmup 5] [--limit 120] [--out profiles/group_norm_act.json]
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
    """[{"C", "rest", "G", "act", "links"}]: the distinct MyGroupNorm inputs of one forward of the DDPM network."""
    import torch
    from point_diffusion_refinement_amd.pointnet2 import configs
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from point_diffusion_refinement_amd.pointnet2_ops.attention import MyGroupNorm, NormActSequential, fused_act_of
    if not torch.cuda.is_available():
        sys.exit("group_norm_act_bench: no GPU (the module path has no CPU ops)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet2CloudCondition(configs.ddpm_pointnet_config()).to(dev)
    act_after, seen = {}, {}
    for seq in net.modules():
        if isinstance(seq, NormActSequential):
            mods = list(seq)
            for i, m in enumerate(mods):
                if isinstance(m, MyGroupNorm):
                    act_after[id(m)] = (fused_act_of(mods[i + 1]) if i + 1 < len(mods) else None) or "none"

    def hook(m, args):
        x = args[0]
        key = (int(x.shape[1]), tuple(int(d) for d in x.shape[2:]), m.num_groups, act_after.get(id(m), "none"))
        seen[key] = seen.get(key, 0) + 1

    for m in net.modules():
        if isinstance(m, MyGroupNorm):
            m.register_forward_pre_hook(hook)
    B = 2
    x, cond, label = configs.synthetic_batch(B, device=dev)
    with torch.no_grad():
        net.reset_cond_features()
        net(x, cond, ts=torch.full((B,), 500.0, device=dev), label=label)
    torch.cuda.synchronize()
    return [{"C": k[0], "rest": list(k[1]), "G": k[2], "act": k[3], "links": n} for k, n in sorted(seen.items())]


def measure(C, rest, G, act, B, reps, warmup):
    """One shape, in this process: the dict of the module docstring."""
    import torch
    import torch.nn.functional as F
    from point_diffusion_refinement_amd.pointnet2_ops import pointnet2_utils
    if not torch.cuda.is_available():
        sys.exit("group_norm_act_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cn = C - C % G
    g = torch.Generator(device=dev).manual_seed(C * 1000003 + sum(rest) * 101 + G)
    x = torch.randn(B, C, *rest, device=dev, generator=g).requires_grad_()
    w = (1 + 0.1 * torch.randn(cn, device=dev, generator=g)).requires_grad_()
    b = (0.1 * torch.randn(cn, device=dev, generator=g)).requires_grad_()
    grad_out = torch.randn(B, C, *rest, device=dev, generator=g)
    leaves = (x, w, b)

    def clear():
        for t in leaves:
            t.grad = None

    def op():
        clear()
        pointnet2_utils.group_norm_act(x, w, b, G, 1e-5, act).backward(grad_out)

    def composition():                                       # MyGroupNorm.forward and the activation module, as today
        clear()
        h = F.group_norm(x[:, :cn], G, w, b, 1e-5)
        z = h if cn == C else torch.cat([h, x[:, cn:]], dim=1)
        y = F.relu(z) if act == "relu" else (z * torch.sigmoid(z) if act == "swish" else z)
        y.backward(grad_out)

    runs = {"op": op, "composition": composition}

    def timed(fn):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        return a.elapsed_time(e)

    grads, peak, diff = {}, {}, {}
    for k, fn in runs.items():
        for _ in range(warmup):
            fn()
        grads[k] = [t.grad.clone() for t in leaves]
    for i, name in enumerate(("x", "weight", "bias")):       # same results before any timing is compared
        p, q = grads["op"][i], grads["composition"][i]
        diff[name] = ((p - q).abs().max() / q.abs().max()).item()
    del grads, p, q
    clear()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()                 # the four inputs
    for k, fn in runs.items():
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated()
        clear()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():                           # alternating
            times[k].append(timed(fn))
    moved = x.numel() * 32
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"shape": [B, C] + list(rest), "G": G, "act": act, "op_ms": med["op"], "op_ms_min": min(times["op"]),
            "op_ms_max": max(times["op"]), "composition_ms": med["composition"],
            "composition_ms_min": min(times["composition"]), "composition_ms_max": max(times["composition"]),
            "op_bytes_moved": moved, "op_gbytes_per_s": moved / med["op"] / 1e6, "resident_bytes": resident,
            "op_peak_bytes": peak["op"], "composition_peak_bytes": peak["composition"],
            "max_grad_x_diff_over_max": diff["x"], "max_grad_weight_diff_over_max": diff["weight"],
            "max_grad_bias_diff_over_max": diff["bias"]}


def child(args_list, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("group_norm_act_bench: %s ran into its time limit of %d s; stopping" % (what, limit))
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        sys.exit("group_norm_act_bench: %s exited with %d; stopping" % (what, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child process, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--probe", action="store_true", help="(child) print the network's links as JSON")
    ap.add_argument("--one", default="", help="(child) measure C:rest:G:acts, e.g. 35:1024x32:32:relu,swish")
    ap.add_argument("--list", action="store_true", help="print the links and exit")
    args = ap.parse_args()
    if args.probe:
        print(json.dumps(probe()), flush=True)
        return
    if args.one:
        C, rest, G, acts = args.one.split(":")
        print(json.dumps([measure(int(C), [int(v) for v in rest.split("x")], int(G), act, args.B, args.reps, args.warmup)
                          for act in acts.split(",")]), flush=True)
        return
    links = child(["--probe"], args.limit, "the probe")
    if args.list:
        for l in links:
            print("%d x %s  G %d  %-5s  %d links" % (l["C"], "x".join(map(str, l["rest"])), l["G"], l["act"], l["links"]))
        return
    # the network's stacks use one activation; the op serves both, so every distinct tensor shape is timed for ReLU
    # and Swish (the links that run without an activation -- weight_conv's norms -- as 'none' too, where they occur)
    todo = {}
    for l in links:
        acts = todo.setdefault((l["C"], tuple(l["rest"]), l["G"]), {"relu": 0, "swish": 0})
        acts[l["act"]] = acts.get(l["act"], 0) + l["links"]
    result = {"tool": "group_norm_act_bench", "B": args.B, "reps": args.reps, "warmup": args.warmup,
              "links_per_forward": sum(l["links"] for l in links), "shapes": []}
    for (C, rest, G), acts in sorted(todo.items()):              # a child per tensor shape, its activations in turn
        one = "%d:%s:%d:%s" % (C, "x".join(map(str, rest)), G, ",".join(sorted(acts)))
        rows = child(["--one", one, "--B", str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                     args.limit, one)
        for row in rows:
            row["links_in_network"] = acts[row["act"]]
            result["shapes"].append(row)
            sys.stderr.write("%-24s %-5s op %.3f ms  composition %.3f ms\n"
                             % (one.rsplit(":", 1)[0], row["act"], row["op_ms"], row["composition_ms"]))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
