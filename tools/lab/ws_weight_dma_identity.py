"""Bit-identity probe of the layer kernels between two BUILDS of libpdr_hip.so (a process loads one build):

    python -m tools.lab.ws_weight_dma_identity OUT.json            # digests of this build
    python -m tools.lab.ws_weight_dma_identity OUT.json REF.json   # ... compared with another build's

Runs the nine shapes / source forms of tools/lab/patches/r6_double_accumulator.patch's session (odd and even tiles per
workgroup, one and two column tiles, a partial single chunk, plain / residual / ball / kNN sources) plus the
residual-gathered forms, a narrow and a 64-column output and a paired launch, built by tests/layer_cases.py, and writes
the SHA-256 of every output and statistics array.  Exit status 1 when a digest differs from REF's.
"""
import ctypes
import hashlib
import json
import sys

import torch

from point_diffusion_refinement_amd import _lib
from tests import layer_cases as lc

CASES = [(8, 16384, 128, 128, "plain"), (9, 16384, 128, 128, "plain"), (4, 16384, 171, 256, "plain"),
         (8, 16384, 3, 128, "plain"), (8, 16384, 40, 128, "plain"), (8, 16384, 128, 128, "residual"),
         (8, 16384, 105, 128, "ball"), (8, 16384, 128, 128, "knn"), (9, 16384, 171, 128, "knn"),
         # beyond the nine: residual-gathered (ball / kNN form), narrow and 64-column tiles, a partial row tile
         (8, 16384, 171, 128, "ball_res"), (8, 16384, 171, 128, "knn_res"), (8, 16384, 41, 32, "plain"),
         (8, 8192, 73, 64, "ball"), (5, 1000, 171, 140, "residual"), (5, 1000 - 8, 73, 35, "knn")]


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for i, (B, rpb, Cin, Cout, form) in enumerate(CASES):
        c = lc.Case(B=B, rpb=rpb, segs=(Cin,), Cout=Cout, form=form, K=8, ss=True, post=True, relu_col0=Cout // 2,
                    seed=i, pair=(i == 11), tile_list=(i == 11), ptpb_extra=1 if i == 11 else -1)
        L = lc.build(c, dev)
        L.x64 = L.m64 = None
        Y = torch.full((c.P, c.ldy), float("nan"), device=dev)
        part = torch.full((c.B * L.ptpb, c.Cout, 2), float("nan"), device=dev)
        _lib.check(lib.pdr_fused_layer(ctypes.byref(L.li), c.P, c.Cin, L.ptr("Wt"), c.ldw, L.ptr("bias"), c.Cout,
                                       Y.data_ptr(), c.ldy, part.data_ptr(), c.relu_col0, st), "fused_layer")
        torch.cuda.synchronize()
        out[c.label()] = [digest(Y), digest(part)]
        if c.pair:
            L2 = lc.build(lc.pair_case(c), dev, weights=(L.keep["Wt"], L.keep.get("bias")))
            c2 = L2.case
            Ya, Yb = torch.full_like(Y, float("nan")), torch.full((c2.P, c2.ldy), float("nan"), device=dev)
            pa = torch.full_like(part, float("nan"))
            pb = torch.full((c2.B * L2.ptpb, c2.Cout, 2), float("nan"), device=dev)
            _lib.check(lib.pdr_fused_layer_pair(ctypes.byref(L.li), c.P, ctypes.byref(L2.li), c2.P, c.Cin, L.ptr("Wt"),
                                                c.ldw, L.ptr("bias"), c.Cout, Ya.data_ptr(), c.ldy, Yb.data_ptr(), c2.ldy,
                                                pa.data_ptr(), pb.data_ptr(), c.relu_col0, st), "fused_layer_pair")
            torch.cuda.synchronize()
            out[c.label() + " paired"] = [digest(Ya), digest(pa), digest(Yb), digest(pb)]
    json.dump(out, open(sys.argv[1], "w"), indent=1)
    if len(sys.argv) > 2:
        ref = json.load(open(sys.argv[2]))
        bad = [k for k in out if ref.get(k) != out[k]]
        print("%d cases, %d differ from %s%s" % (len(out), len(bad), sys.argv[2], ": " + "; ".join(bad) if bad else ""))
        return 1 if bad else 0
    print("%d cases written" % len(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
