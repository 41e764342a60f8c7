"""Forward plus backward of group_knn(..., transpose=True) with its grouping head as one op
(pointnet2_utils.knn_and_group: pdr_knn_group_cf / pdr_knn_group_cf_grad, behind set_fused_knn_grouping) against the
torch composition it replaces (a transpose copy of the features, knn_gather, the weight arithmetic, the cat and two
transposes), at the shapes of the DDPM network with B = 32.  DESIGN section 7a.6.

The shapes come from pointnet2/configs.py: a probe process builds PointNet2CloudCondition(ddpm_pointnet_config()),
runs one forward of the module path at B = 2 with a hook on group_knn, and records (n1, n2, K, C, transpose) -- every
kNN grouping the network runs, not a hand-kept list.

Each distinct shape is measured at B = --B on two kinds of clouds in [-1, 1]^3: "noise" (standard normal coordinates
times 0.5, what q_sample gives late in the chain) and "surface" (points on a sphere of radius 0.5 with a little noise).
As in the network, the searched cloud y is a subset of the queries x when n2 < n1 (an upsampled level contains its
parents: the first neighbour of such a query is itself, d2 == 0), and an independent draw otherwise.  What is timed is
the whole of group_knn, its neighbour search included (pdr_knn_group with the switch on, knn_points with it off), so
the three variants differ in everything the switch changes: the module with set_fused_knn_grouping(True) against the
switch off in both backward modes (set_deterministic(False): atomics, set_deterministic(True): the order-fixed
knn_points backward; torch.gather's own backward stays what it is).  The composition returns a non-contiguous view
that its consumers (Conv2d, MyGroupNorm) copy; that copy is NOT in these figures.

Protocol (that of tools/query_group_bench.py): one child process per shape, each under its own time limit; the first
child that fails ends the run (nothing is tried again).  In a child: device events around one forward + backward
through autograd (allocation included), warm-up calls, then repetitions alternating between the three variants,
medians; torch.cuda.max_memory_allocated of one forward + backward of each, taken after the warm-up with the inputs
already resident (`resident_bytes`).  `op_gbytes_per_s` is 8 bytes per output element -- the forward's one store and
the backward's one load of the big tensor -- over the op's time, which also holds the search, allocations and
autograd's bookkeeping.  `forward_aligned_ms` / `forward_offset_ms` time the forward launch alone (no search) into a
preallocated buffer and into a view 4 bytes into it: the vector family against the scalar one where K % 4 == 0
(4 bytes per output element).

    python tools/knn_group_bench.py [--B 32] [--reps 30] [--warmup 5] [--limit 120] [--out profiles/knn_group_cf.json]
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

DATA = ("noise", "surface")


def probe():
    """[{"n1", "n2", "K", "C", "calls"}]: the distinct transpose=True kNN groupings of one forward."""
    import torch
    from point_diffusion_refinement_amd.pointnet2 import configs
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from point_diffusion_refinement_amd.pointnet2_ops import pointnet2_utils
    if not torch.cuda.is_available():
        sys.exit("knn_group_bench: no GPU (the module path has no CPU ops)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet2CloudCondition(configs.ddpm_pointnet_config()).to(dev)
    seen = {}
    inner = pointnet2_utils.group_knn

    def hook(x, y, features_at_y, K, transpose=False):
        if transpose:
            key = (int(x.shape[1]), int(y.shape[1]), int(K), int(features_at_y.shape[1]))
            seen[key] = seen.get(key, 0) + 1
        return inner(x, y, features_at_y, K, transpose=transpose)

    pointnet2_utils.group_knn = hook
    B = 2
    x, cond, label = configs.synthetic_batch(B, device=dev)
    with torch.no_grad():
        net.reset_cond_features()
        net(x, cond, ts=torch.full((B,), 500.0, device=dev), label=label)
    torch.cuda.synchronize()
    pointnet2_utils.group_knn = inner
    return [dict(zip(("n1", "n2", "K", "C"), k), calls=c) for k, c in sorted(seen.items())]


def clouds(kind, B, n, gen, dev):
    import torch
    p = torch.randn(B, n, 3, device=dev, generator=gen)
    if kind == "noise":
        return 0.5 * p
    return 0.5 * p / p.norm(dim=2, keepdim=True) + 0.01 * torch.randn(B, n, 3, device=dev, generator=gen)


def measure(s, kind, B, reps, warmup):
    """One shape on one kind of cloud, in this process: the dict of the module docstring."""
    import torch
    from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
    dev = torch.device("cuda:0")
    n1, n2, K, C = s["n1"], s["n2"], s["K"], s["C"]
    g = torch.Generator(device=dev).manual_seed(n1 * 1000003 + n2 * 10007 + K * 101 + C + DATA.index(kind))
    x = clouds(kind, B, n1, g, dev)
    if n2 < n1:
        pick = torch.stack([torch.randperm(n1, device=dev, generator=g)[:n2] for _ in range(B)])
        y = x.gather(1, pick.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    else:
        y = clouds(kind, B, n2, g, dev)
    feat = torch.randn(B, C, n2, device=dev, generator=g)
    leaves = [t.requires_grad_() for t in (x, y, feat)]
    grad_out = torch.randn(B, C + 11, n1, K, device=dev, generator=g)

    def clear():
        for t in leaves:
            t.grad = None

    def run(fused, det):
        def fn():
            clear()
            _ext.set_fused_knn_grouping(fused)
            _ext.set_deterministic(det)
            pointnet2_utils.group_knn(x, y, feat, K, transpose=True).backward(grad_out)
        return fn

    runs = {"op": run(True, False), "composition": run(False, False), "composition_det": run(False, True)}

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
        grads[k] = [None if t.grad is None else t.grad.clone() for t in leaves]
    for i, name in enumerate(("x", "y", "features")):            # the same results before any timing is compared
        p, q = grads["op"][i], grads["composition_det"][i]
        diff[name] = ((p - q).abs().max() / q.abs().max().clamp_min(1e-30)).item()
    del grads
    clear()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    for k, fn in runs.items():
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated()
        clear()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():                               # alternating
            times[k].append(timed(fn))
    _ext.set_deterministic(None)
    # the forward launch alone in both kernel families: the same call into an aligned buffer (K % 4 == 0: the vector
    # family) and into a view 4 bytes further (the scalar family), no search and no allocation in either
    xd, yd, fd = (t.detach() for t in leaves)
    d, idx, _ = _ext.knn_group(xd, yd, K)
    buf = torch.empty(grad_out.numel() + 4, device=dev)
    outs = {"aligned": buf[:grad_out.numel()].view(grad_out.shape), "offset": buf[1:grad_out.numel() + 1].view(grad_out.shape)}
    fwd = {k: (lambda o=o: _ext.knn_group_cf(xd, yd, fd, idx, d, out=o)) for k, o in outs.items()}
    fam = {k: [] for k in fwd}
    for fn in fwd.values():
        for _ in range(warmup):
            fn()
    for _ in range(reps):
        for k, fn in fwd.items():
            fam[k].append(timed(fn))
    moved = grad_out.numel() * 8
    row = {"shape": [B, C + 11, n1, K], "n2": n2, "C": C, "data": kind, "calls_in_network": s["calls"],
           "zero_distance_slots": float((d == 0).float().mean().item()), "resident_bytes": resident,
           "op_bytes_moved": moved}
    for k, v in times.items():
        row[k + "_ms"], row[k + "_ms_min"], row[k + "_ms_max"] = statistics.median(v), min(v), max(v)
        row[k + "_peak_bytes"] = peak[k]
    row["op_gbytes_per_s"] = moved / row["op_ms"] / 1e6
    row["forward_family"] = "vector" if K % 4 == 0 else "scalar"          # what the aligned call runs
    row["forward_aligned_ms"], row["forward_offset_ms"] = statistics.median(fam["aligned"]), statistics.median(fam["offset"])
    row["forward_aligned_gbytes_per_s"] = grad_out.numel() * 4 / row["forward_aligned_ms"] / 1e6
    row["forward_offset_gbytes_per_s"] = grad_out.numel() * 4 / row["forward_offset_ms"] / 1e6
    for name, v in diff.items():
        row["max_grad_%s_diff_over_max" % name] = v
    return row


def child(args_list, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("knn_group_bench: %s ran into its time limit of %d s; stopping" % (what, limit))
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        sys.exit("knn_group_bench: %s exited with %d; stopping" % (what, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child process, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--probe", action="store_true", help="(child) print the network's kNN groupings as JSON")
    ap.add_argument("--one", default="", help="(child) measure one grouping, given as the probe's JSON object")
    ap.add_argument("--list", action="store_true", help="print the groupings and exit")
    args = ap.parse_args()
    if args.probe:
        print(json.dumps(probe()), flush=True)
        return
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("knn_group_bench: no GPU (there is no CPU path to time)")
        s = json.loads(args.one)
        print(json.dumps([measure(s, kind, args.B, args.reps, args.warmup) for kind in DATA]), flush=True)
        return
    shapes = child(["--probe"], args.limit, "the probe")
    if args.list:
        for s in shapes:
            print(json.dumps(s))
        return
    result = {"tool": "knn_group_bench", "B": args.B, "reps": args.reps, "warmup": args.warmup,
              "groupings_per_forward": sum(s["calls"] for s in shapes), "shapes": []}
    for s in shapes:                                             # a child per shape, both kinds of cloud in turn
        what = "n1 %d n2 %d K %d C %d" % (s["n1"], s["n2"], s["K"], s["C"])
        rows = child(["--one", json.dumps(s), "--B", str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                     args.limit, what)
        for row in rows:
            result["shapes"].append(row)
            sys.stderr.write("%-32s %-7s op %.3f ms  composition %.3f ms  deterministic %.3f ms\n"
                             % (what, row["data"], row["op_ms"], row["composition_ms"], row["composition_det_ms"]))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
