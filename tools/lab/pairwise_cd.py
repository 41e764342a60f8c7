"""All-pairs Chamfer matrix: the fused kernel (set_metrics.pairwise_cd -> pdr_chamfer_pairwise) against the composed
route on the kernels that were there before it -- per sample: expand to R copies, _ext.chamfer_nn, two means, one add
(what _pairwise_EMD_CD_ of the reference does with its own chamfer extension).

    python -m tools.lab.pairwise_cd [--sets 256] [--points 2048] [--repeats 5] [--out profiles/pairwise_cd.txt] [--lib PATH]

Times S = R = sets, n = m = points, and the self-matrix of one set (the composed route has no shortcut for it: it
evaluates both triangles, as the reference does for M_rr and M_ss).  Device events around whole calls, two warm-up
rounds, then `repeats` rounds alternating the two routes; the median round of each is reported with its spread, and
the ratio composed / fused.  The two results are compared first (rtol 1e-5: float32 means in another order).
"""
import argparse
import statistics

import torch

from point_diffusion_refinement_amd import _lib


def composed(x, y, ext):
    rows = []
    R = y.shape[0]
    for s in range(x.shape[0]):
        xs = x[s].view(1, -1, 3).expand(R, -1, -1).contiguous()
        dl, _, dr, _ = ext.chamfer_nn(xs, y)
        rows.append((dl.mean(dim=1) + dr.mean(dim=1)).view(1, -1))
    return torch.cat(rows, dim=0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/pairwise_cd.txt")
    ap.add_argument("--lib", default=None, help="another build of libpdr_hip.so (lab builds)")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = a.lib
    assert torch.cuda.is_available(), "timing needs the GPU: there is no CPU path"
    from point_diffusion_refinement_amd.pointnet2 import set_metrics as SM
    from point_diffusion_refinement_amd.pointnet2_ops import _ext

    g = torch.Generator().manual_seed(0)
    x = (torch.rand(a.sets, a.points, 3, generator=g) * 2 - 1).cuda()
    y = (torch.rand(a.sets, a.points, 3, generator=g) * 2 - 1).cuda()
    lines = ["pairwise Chamfer matrix, S = R = %d clouds of n = m = %d points, %s; ms per matrix, median of %d "
             "alternating rounds after 2 warm-up rounds (min .. max)"
             % (a.sets, a.points, torch.cuda.get_device_name(0), a.repeats)]
    for name, (p, q) in (("x vs y", (x, y)), ("self-matrix", (x, x))):
        routes = {"fused": lambda: SM.pairwise_cd(p, q), "composed": lambda: composed(p, q, _ext)}
        ms = {k: [] for k in routes}
        for rnd in range(2 + a.repeats):
            res = {}
            for k, fn in routes.items():
                t, res[k] = timed(fn)
                if rnd >= 2:
                    ms[k].append(t)
            torch.testing.assert_close(res["fused"], res["composed"], rtol=1e-5, atol=0)
        med = {k: statistics.median(v) for k, v in ms.items()}
        evals = 2.0 * a.sets * a.sets * a.points * a.points
        for k in routes:
            lines.append("  %-12s %-9s %9.2f  (%.2f .. %.2f)   %.2f T point pairs/s of the full matrix"
                         % (name, k, med[k], min(ms[k]), max(ms[k]), evals / med[k] / 1e9))
        lines.append("  %-12s composed / fused = %.2f" % (name, med["composed"] / med["fused"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
