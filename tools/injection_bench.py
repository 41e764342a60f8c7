"""Forward plus backward of the tail of an Mlp_plus_t_emb stack -- MyGroupNorm, ReLU / Swish, the broadcast add of an
embedding and, behind the last stack, the residual add -- as one op (pointnet2_utils.group_norm_act_add:
pdr_group_norm_act_add / pdr_group_norm_act_add_grad) against the two forms it replaces, at the tails of the DDPM
network with B = 32.  DESIGN section 7a.9.

    composition   nn.GroupNorm (slice and cat when C % G != 0), the activation, h + e[:, :, None, None], h + r
    fused_gn      pointnet2_utils.group_norm_act (what set_fused_group_norm(True) runs), then the same torch adds:
                  the fair baseline, the only difference to the op being the adds

The tails come from pointnet2/configs.py: a probe process builds PointNet2CloudCondition(ddpm_pointnet_config()), runs
one forward of the module path at B = 2 with a wrapper around NormActSequential.forward_add under
set_fused_injection(True), and records (C, trailing dimensions, groups, activation, embedding present, residual
present) of every call that carries a term -- and whether the stack ends in the pair the op absorbs.  `sites_per_forward`
is the number of such calls in one forward.

Protocol (that of tools/group_norm_act_bench.py): one child process per distinct tensor shape, each under its own time
limit; the first child that fails ends the run (nothing is tried again).  In a child: device events around one
forward + backward through autograd (allocation included), warm-up calls, then repetitions alternating between the
three variants, medians; torch.cuda.max_memory_allocated of one forward + backward of each.  `op_gbytes_per_s` is the
bytes the op's five kernels must move -- forward 2 reads and 1 write, one more read with a residual; backward 4 reads
and 1 write: 32 or 36 bytes per element -- over the op's time.

    python tools/injection_bench.py [--B 32] [--reps 30] [--warmup 5] [--limit 120] [--out profiles/group_norm_act_add.json]
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
    """[{"C", "rest", "G", "act", "e", "r", "absorbed", "sites"}]: the distinct tails of one forward of the network."""
    import torch
    from point_diffusion_refinement_amd import pointnet2_ops
    from point_diffusion_refinement_amd.pointnet2 import configs
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from point_diffusion_refinement_amd.pointnet2_ops.attention import MyGroupNorm, NormActSequential, fused_act_of
    if not torch.cuda.is_available():
        sys.exit("injection_bench: no GPU (the module path has no CPU ops)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet2CloudCondition(configs.ddpm_pointnet_config()).to(dev)
    seen, inner = {}, NormActSequential.forward_add

    def forward_add(self, x, add=None, residual=None):
        out = inner(self, x, add, residual)
        if add is not None or residual is not None:
            mods = list(self)
            pair = len(mods) >= 2 and isinstance(mods[-2], MyGroupNorm) and bool(fused_act_of(mods[-1]))
            key = (int(out.shape[1]), tuple(int(d) for d in out.shape[2:]), mods[-2].num_groups if pair else 0,
                   (fused_act_of(mods[-1]) if pair else "none"), add is not None, residual is not None,
                   type(out.grad_fn).__name__ == "GroupNormActAddBackward")
            seen[key] = seen.get(key, 0) + 1
        return out

    NormActSequential.forward_add = forward_add
    prev = pointnet2_ops.set_fused_injection(True)
    try:
        B = 2
        x, cond, label = configs.synthetic_batch(B, device=dev)
        net.reset_cond_features()
        net(x, cond, ts=torch.full((B,), 500.0, device=dev), label=label)       # with grad: the op leaves its node
        torch.cuda.synchronize()
    finally:
        pointnet2_ops.set_fused_injection(prev)
        NormActSequential.forward_add = inner
    return [{"C": k[0], "rest": list(k[1]), "G": k[2], "act": k[3], "e": k[4], "r": k[5], "absorbed": k[6], "sites": n}
            for k, n in sorted(seen.items())]


def measure(C, rest, G, act, has_e, has_r, B, reps, warmup):
    """One tail, in this process: the dict of the module docstring."""
    import torch
    import torch.nn.functional as F
    from point_diffusion_refinement_amd.pointnet2_ops import pointnet2_utils
    if not torch.cuda.is_available():
        sys.exit("injection_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cn = C - C % G
    g = torch.Generator(device=dev).manual_seed(C * 1000003 + sum(rest) * 101 + G)
    x = torch.randn(B, C, *rest, device=dev, generator=g).requires_grad_()
    w = (1 + 0.1 * torch.randn(cn, device=dev, generator=g)).requires_grad_()
    b = (0.1 * torch.randn(cn, device=dev, generator=g)).requires_grad_()
    e = torch.randn(B, C, device=dev, generator=g).requires_grad_() if has_e else None
    r = torch.randn(B, C, *rest, device=dev, generator=g).requires_grad_() if has_r else None
    grad_out = torch.randn(B, C, *rest, device=dev, generator=g)
    leaves = [t for t in (x, w, b, e, r) if t is not None]
    names = [n for n, t in zip(("x", "weight", "bias", "e", "r"), (x, w, b, e, r)) if t is not None]
    lift = (slice(None), slice(None)) + (None,) * len(rest)

    def clear():
        for t in leaves:
            t.grad = None

    def adds(y):
        if e is not None:
            y = y + e[lift]
        if r is not None:
            y = y + r
        return y

    def op():
        clear()
        pointnet2_utils.group_norm_act_add(x, w, b, G, 1e-5, act, add=e, residual=r).backward(grad_out)

    def fused_gn():
        clear()
        adds(pointnet2_utils.group_norm_act(x, w, b, G, 1e-5, act)).backward(grad_out)

    def composition():
        clear()
        h = F.group_norm(x[:, :cn], G, w, b, 1e-5)
        z = h if cn == C else torch.cat([h, x[:, cn:]], dim=1)
        y = F.relu(z) if act == "relu" else (z * torch.sigmoid(z) if act == "swish" else z)
        adds(y).backward(grad_out)

    runs = {"op": op, "fused_gn": fused_gn, "composition": composition}

    def timed(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z)

    grads, peak, diff = {}, {}, {}
    for k, fn in runs.items():
        for _ in range(warmup):
            fn()
        grads[k] = [t.grad.clone() for t in leaves]
    for i, name in enumerate(names):                         # same results before any timing is compared
        p, q = grads["op"][i], grads["composition"][i]
        diff[name] = ((p - q).abs().max() / q.abs().max()).item()
    del grads, p, q
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
        for k, fn in runs.items():                           # alternating
            times[k].append(timed(fn))
    moved = x.numel() * (36 if has_r else 32)
    row = {"shape": [B, C] + list(rest), "G": G, "act": act, "e": has_e, "r": has_r, "op_bytes_moved": moved,
           "resident_bytes": resident}
    for k, v in times.items():
        row.update({k + "_ms": statistics.median(v), k + "_ms_min": min(v), k + "_ms_max": max(v),
                    k + "_peak_bytes": peak[k]})
    row["op_gbytes_per_s"] = moved / row["op_ms"] / 1e6
    row.update({"max_grad_%s_diff_over_max" % n: d for n, d in diff.items()})
    return row


def child(args_list, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("injection_bench: %s ran into its time limit of %d s; stopping" % (what, limit))
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        sys.exit("injection_bench: %s exited with %d; stopping" % (what, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child process, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--probe", action="store_true", help="(child) print the network's tails as JSON")
    ap.add_argument("--one", default="", help="(child) measure C:rest:G:variants, a variant being act/e/r, "
                                              "e.g. 64:1024x32:32:swish/1/0,swish/1/1")
    ap.add_argument("--list", action="store_true", help="print the tails and exit")
    args = ap.parse_args()
    if args.probe:
        print(json.dumps(probe()), flush=True)
        return
    if args.one:
        C, rest, G, variants = args.one.split(":")
        rows = []
        for v in variants.split(","):
            act, has_e, has_r = v.split("/")
            rows.append(measure(int(C), [int(d) for d in rest.split("x")], int(G), act, has_e == "1", has_r == "1",
                                args.B, args.reps, args.warmup))
        print(json.dumps(rows), flush=True)
        return
    tails = child(["--probe"], args.limit, "the probe")
    if args.list:
        for t in tails:
            print("%d x %s  G %d  %-5s  e %d  r %d  absorbed %d  %d sites" % (
                t["C"], "x".join(map(str, t["rest"])), t["G"], t["act"], t["e"], t["r"], t["absorbed"], t["sites"]))
        return
    todo = {}
    for t in tails:
        if t["absorbed"]:
            key = "%s/%d/%d" % (t["act"], t["e"], t["r"])
            shape = todo.setdefault((t["C"], tuple(t["rest"]), t["G"]), {})
            shape[key] = shape.get(key, 0) + t["sites"]
    result = {"tool": "injection_bench", "B": args.B, "reps": args.reps, "warmup": args.warmup,
              "sites_per_forward": sum(t["sites"] for t in tails),
              "sites_on_the_composition": sum(t["sites"] for t in tails if not t["absorbed"]), "tails": []}
    for (C, rest, G), variants in sorted(todo.items()):          # a child per tensor shape, its variants in turn
        one = "%d:%s:%d:%s" % (C, "x".join(map(str, rest)), G, ",".join(sorted(variants)))
        rows = child(["--one", one, "--B", str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                     args.limit, one)
        for row in rows:
            row["sites_in_network"] = variants["%s/%d/%d" % (row["act"], row["e"], row["r"])]
            result["tails"].append(row)
            sys.stderr.write("%-22s %-5s e %d r %d  op %.3f ms  fused_gn %.3f ms  composition %.3f ms\n"
                             % (one.split(":", 3)[0] + ":" + one.split(":", 3)[1], row["act"], row["e"], row["r"],
                                row["op_ms"], row["fused_gn_ms"], row["composition_ms"]))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
