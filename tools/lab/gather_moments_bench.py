"""The statistics-only pass of a virtual first conv at the shapes of a reverse step (B = 32): the whole-width
pdr_gather_add (Y = NULL) against pdr_gather_moments over the [first | . | key] windows, alone on the chip, with the
windows' moments compared bit for bit:  python -m tools.lab.gather_moments_bench [--lib path/to/lib.so] [--reps 50]"""
import argparse

import torch

from point_diffusion_refinement_amd import _lib

# (block, queries per cloud, K, (C1, Clast, C2), source points per cloud, kNN form)
SHAPES = [
    ("FP 2048", 2048, 8, (128, 128, 171), 1024, True), ("FP 1024", 1024, 8, (128, 128, 331), 256, True),
    ("FP 256", 256, 8, (256, 256, 331), 64, True), ("FP 64", 64, 8, (256, 256, 651), 16, True),
    ("ball 1024", 1024, 32, (128, 128, 137), 2048, False), ("ball 256", 256, 32, (128, 128, 137), 1024, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = args.lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, st = args.batch, torch.cuda.current_stream().cuda_stream
    for name, m, K, (C1, Cl, C2), n_src, knn in SHAPES:
        Cout, rpb = C1 + Cl + C2, m * K
        g = torch.Generator(device=dev).manual_seed(m + Cout)
        P, ld = B * rpb, (Cout + 31) // 32 * 32
        U = torch.randn(B * n_src + 1, ld, device=dev, generator=g)
        V2 = torch.randn(B * m, 2 * ld, device=dev, generator=g)
        idx = torch.randint(0, n_src, (P,), device=dev, dtype=torch.int32, generator=g)
        cnt = None if knn else torch.randint(0, 4, (B * m,), device=dev, dtype=torch.int32, generator=g)
        s1, s2 = (torch.rand(P, device=dev, generator=g) for _ in range(2)) if knn else (None, None)
        r1, r2 = (torch.randn(ld + 4, device=dev, generator=g) for _ in range(2)) if knn else (None, None)
        p = lambda t: t.data_ptr() if t is not None else None
        head = (U.data_ptr(), ld, n_src, V2.data_ptr(), None if knn else V2.data_ptr() + 4 * ld, 2 * ld, idx.data_ptr(),
                p(cnt), p(s1), p(r1), p(s2), p(r2), B, rpb, K, Cout)
        old = torch.zeros(B * (rpb // 128), Cout, 2, device=dev)
        new = torch.zeros_like(old)
        calls = {
            "whole": lambda: _lib.check(lib.pdr_gather_add(*head, None, ld, old.data_ptr(), C1 + Cl, 0, -1, st), "gather_add"),
            "windows": lambda: _lib.check(lib.pdr_gather_moments(*head, new.data_ptr(), C1 + Cl, 0, C1, C1 + Cl, C2, st),
                                          "gather_moments"),
        }
        us = {}
        for key, call in calls.items():
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us[key] = e0.elapsed_time(e1) / args.reps * 1e3
        w = torch.ones(Cout, dtype=torch.bool, device=dev)
        w[C1:C1 + Cl] = False
        same = bool(torch.equal(old[:, w], new[:, w])) and bool((new[:, ~w] == 0).all())
        print("%-9s rows=%7d K=%2d cols=%d+%d+%d: whole %6.1f us, windows %6.1f us (%+5.1f %%; residual share %4.1f %%) | %s"
              % (name, P, K, C1, Cl, C2, us["whole"], us["windows"], 100.0 * (us["windows"] / us["whole"] - 1.0),
                 100.0 * Cl / Cout, "windows bit-equal, residual untouched" if same else "DIFFERS"))


if __name__ == "__main__":
    main()
