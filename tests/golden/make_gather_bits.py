"""Recorded bits of the virtual first conv's gather pass (csrc/fused_gather.hip): pdr_gather_add* / pdr_gather_moments*.

    python -m tests.golden.make_gather_bits [--lib path/to/libpdr_hip.so] [--out tests/golden/gather_bits.npz]     (GPU)

tests/test_gather_bits_gpu.py rebuilds the same inputs, makes the same calls and asks for torch.equal against the file
this writes, so the file is the independent side of that comparison: record it from a library whose kernels are known
good, never from the change under test.  Inputs are drawn on the CPU with fixed seeds and moved to the device, so they
do not depend on the machine.  Moments are stored raw (float32, with the sentinel where the contract leaves an entry
unwritten), Y / Yd as the SHA-256 of their bytes (test_fused_gpu.py / test_gather_moments_gpu.py pin their values).

The recording run also asserts what DESIGN.md 4.11 states: on the windows' columns pdr_gather_moments* equals
pdr_gather_add* bit for bit (and Yd of the two twin entry points in every column)."""
import argparse
import hashlib
import os

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib

SENTINEL = 12345.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gather_bits.npz")
B = 2

# (id, form, K, queries per cloud, source points per cloud, (first, residual, key) columns, seed)
CASES = [
    ("knn_k8_lpr16", "knn", 8, 24, 37, (8, 8, 7), 1),              # 192 rows per cloud: a full tile + a 64-row tile
    ("knn_k8_lpr32", "knn", 8, 24, 37, (32, 32, 40), 2),
    ("knn_k8_lpr64", "knn", 8, 24, 37, (64, 32, 43), 3),           # 64 lanes per row, one column pass
    ("knn_k8_two_passes", "knn", 8, 24, 37, (128, 128, 171), 4),   # two column passes on grid.y
    ("knn_k6", "knn", 6, 32, 37, (16, 16, 9), 5),                  # K not a power of two
    ("ball_k32", "ball", 32, 12, 50, (128, 128, 137), 6),          # 384 rows: three tiles; shared query row
    ("ball_k4", "ball", 4, 64, 50, (64, 32, 43), 7),               # K < DEPTH x rows per instruction: a V row per row
]
TILES_CASE = "ball_k32"


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Case:
    """Inputs of one case: tables U (B n_src + 1, ld), [V | V0] (B m, 2 ld), indices in [0, n_src), the kNN scalars and
    rows or the ball counts (every third one 0)."""

    def __init__(self, dev, form, K, m, n_src, cols, seed):
        self.form, self.K, self.m, self.n_src, self.cols = form, K, m, n_src, cols
        C1, Clast, C2 = cols
        self.Cout, self.relu_col0 = C1 + Clast + C2, C1 + Clast
        self.res = (C1, Clast)                                      # the residual window (col0, cols)
        self.windows = (0, C1, C1 + Clast, C2)
        self.rpb = m * K
        self.tpb = (self.rpb + 127) // 128
        ld = self.ld = (self.Cout + 3) // 4 * 4
        g = torch.Generator().manual_seed(seed)                     # CPU: the same numbers on every machine
        P, knn = B * self.rpb, form == "knn"
        self.U = torch.randn(B * n_src + 1, ld, generator=g).to(dev)
        self.V2 = torch.randn(B * m, 2 * ld, generator=g).to(dev)
        self.idx = torch.randint(0, n_src, (P,), dtype=torch.int32, generator=g).to(dev)
        self.s1 = torch.rand(P, generator=g).to(dev) if knn else None
        self.s2 = torch.rand(P, generator=g).to(dev) if knn else None
        self.r1 = torch.randn(ld + 4, generator=g).to(dev) if knn else None
        self.r2 = torch.randn(ld + 4, generator=g).to(dev) if knn else None
        self.counts = None
        if not knn:
            counts = torch.randint(1, 5, (B * m,), dtype=torch.int32, generator=g)
            counts[torch.arange(B * m) % 3 == 1] = 0
            self.counts = counts.to(dev)
        self.dev = dev

    def tabs(self):
        em = self.counts is not None
        return (self.U.data_ptr(), self.ld, self.n_src, self.V2.data_ptr(), self.V2.data_ptr() + 4 * self.ld if em else None,
                2 * self.ld, self.idx.data_ptr(), _ptr(self.counts))

    def knn(self):
        return (_ptr(self.s1), _ptr(self.r1), _ptr(self.s2), _ptr(self.r2))

    def dims(self):
        return (B, self.rpb, self.K, self.Cout)

    def full(self, *shape):
        return torch.full(shape, SENTINEL, device=self.dev)

    def in_windows(self):
        w = torch.zeros(self.Cout, dtype=torch.bool, device=self.dev)
        w[self.windows[0]:self.windows[0] + self.windows[1]] = True
        w[self.windows[2]:self.windows[2] + self.windows[3]] = True
        return w


def make_case(dev, cid):
    spec = next(c for c in CASES if c[0] == cid)
    return Case(dev, *spec[1:])


def digest(t):
    return np.frombuffer(hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).digest(), dtype=np.uint8).copy()


def run_plain(lib, c, st):
    """The five calls recorded for every case -> {name: moments tensor | Y tensor}; every output prefilled with the
    sentinel.  The residual window's Y has 4 columns more than the window: they stay unwritten."""
    P, ld, rc0 = B * c.rpb, c.ld, c.relu_col0
    out = {}
    m = out["add_y_whole.moments"] = c.full(B * c.tpb, c.Cout, 2)
    y = out["add_y_whole.y"] = c.full(P, ld)
    _lib.check(lib.pdr_gather_add(*c.tabs(), *c.knn(), *c.dims(), y.data_ptr(), ld, m.data_ptr(), rc0, 0, -1, st), "gather_add")
    m = out["add_y_window.moments"] = c.full(B * c.tpb, c.Cout, 2)
    y = out["add_y_window.y"] = c.full(P, (c.res[1] + 3) // 4 * 4 + 4)
    _lib.check(lib.pdr_gather_add(*c.tabs(), *c.knn(), *c.dims(), y.data_ptr(), y.shape[1], m.data_ptr(), rc0, *c.res, st),
               "gather_add")
    m = out["add_no_y.moments"] = c.full(B * c.tpb, c.Cout, 2)
    _lib.check(lib.pdr_gather_add(*c.tabs(), *c.knn(), *c.dims(), None, ld, m.data_ptr(), rc0, 0, -1, st), "gather_add")
    y = out["add_no_partial.y"] = c.full(P, ld)
    _lib.check(lib.pdr_gather_add(*c.tabs(), *c.knn(), *c.dims(), y.data_ptr(), ld, None, rc0, 0, -1, st), "gather_add")
    m = out["moments.moments"] = c.full(B * c.tpb, c.Cout, 2)
    _lib.check(lib.pdr_gather_moments(*c.tabs(), *c.knn(), *c.dims(), m.data_ptr(), rc0, *c.windows, st), "gather_moments")
    torch.cuda.synchronize()
    return out


PTPB = 5


def tile_subset(c):
    """One tile cleared per cloud (the second of the first cloud, the third of the other) -> (tile_valid, the partial
    rows (B, PTPB) that the main tiles write)."""
    tv = torch.ones(B, c.tpb, dtype=torch.uint8, device=c.dev)
    tv[0, 1], tv[1, 2] = 0, 0
    rows = torch.zeros(B, PTPB, dtype=torch.bool, device=c.dev)
    rows[:, :c.tpb] = tv.bool()
    return tv.reshape(-1).contiguous(), rows


def run_tiles(lib, c, st):
    """_tiles and _tiles_twin of both families on the tile subset, partial_tpb = 5, idx0 = the first neighbours,
    wrow0 = [4, 9], wmul = K."""
    P, ld, rc0 = B * c.rpb, c.ld, c.relu_col0
    tv, _ = tile_subset(c)
    idx0 = c.idx.view(B, c.m, c.K)[:, :, 0].contiguous()
    wrow0 = torch.tensor([4, 9], dtype=torch.int32).to(c.dev)
    twin = (tv.data_ptr(), PTPB, idx0.data_ptr())
    none4 = (None, None, None, None)
    out = {}
    m = out["add_tiles.moments"] = c.full(B * PTPB, c.Cout, 2)
    y = out["add_tiles.y"] = c.full(P, ld)
    _lib.check(lib.pdr_gather_add_tiles(*c.tabs(), *none4, *c.dims(), y.data_ptr(), ld, m.data_ptr(), rc0, 0, -1,
                                        tv.data_ptr(), PTPB, st), "gather_add_tiles")
    m = out["add_tiles_twin.moments"] = c.full(B * PTPB, c.Cout, 2)
    y = out["add_tiles_twin.y"] = c.full(P, ld)
    yd = out["add_tiles_twin.yd"] = c.full(B * c.m, ld)
    _lib.check(lib.pdr_gather_add_tiles_twin(*c.tabs(), *c.dims(), y.data_ptr(), ld, m.data_ptr(), rc0, 0, -1, *twin,
                                             yd.data_ptr(), ld, wrow0.data_ptr(), float(c.K), st), "gather_add_tiles_twin")
    m = out["moments_tiles.moments"] = c.full(B * PTPB, c.Cout, 2)
    _lib.check(lib.pdr_gather_moments_tiles(*c.tabs(), *none4, *c.dims(), m.data_ptr(), rc0, *c.windows, tv.data_ptr(),
                                            PTPB, st), "gather_moments_tiles")
    m = out["moments_tiles_twin.moments"] = c.full(B * PTPB, c.Cout, 2)
    yd = out["moments_tiles_twin.yd"] = c.full(B * c.m, ld)
    _lib.check(lib.pdr_gather_moments_tiles_twin(*c.tabs(), *c.dims(), m.data_ptr(), rc0, *c.windows, *twin, yd.data_ptr(),
                                                 ld, wrow0.data_ptr(), float(c.K), st), "gather_moments_tiles_twin")
    torch.cuda.synchronize()
    return out


def check_unwritten(c, out):
    """What the contract leaves unwritten still holds the sentinel; what it writes does not (the inputs are random
    floats: none equals the sentinel).  Shared by the recording run and the test."""
    w = c.in_windows()
    wide = out["add_y_window.y"]
    assert bool((wide[:, (c.res[1] + 3) // 4 * 4:] == SENTINEL).all()), "columns behind the Y window were written"
    assert not bool((wide[:, :c.res[1]] == SENTINEL).any())
    for k in ("add_y_whole.y", "add_no_partial.y"):
        assert not bool((out[k][:, :c.Cout] == SENTINEL).any()), k
    for k in ("add_y_whole.moments", "add_y_window.moments", "add_no_y.moments"):
        assert not bool((out[k] == SENTINEL).any()), k
    assert bool((out["moments.moments"][:, ~w] == SENTINEL).all()), "a moment outside the windows was written"
    assert not bool((out["moments.moments"][:, w] == SENTINEL).any())
    if "add_tiles.moments" not in out:
        return
    _, rows = tile_subset(c)
    main, twin = rows.reshape(-1), rows.clone()
    twin[:, c.tpb] = True                                           # m <= 128 queries: one twin tile per cloud
    twin = twin.reshape(-1)
    for k, written, cols in (("add_tiles.moments", main, None), ("add_tiles_twin.moments", twin, None),
                             ("moments_tiles.moments", main, w), ("moments_tiles_twin.moments", twin, w)):
        assert bool((out[k][~written] == SENTINEL).all()), k + ": a partial row of a skipped tile was written"
        got = out[k][written]
        if cols is not None:
            assert bool((got[:, ~cols] == SENTINEL).all()), k + ": a moment outside the windows was written"
            got = got[:, cols]
        assert not bool((got == SENTINEL).any()), k
    tile_rows = rows[:, :c.tpb].repeat_interleave(128, 1)[:, :c.rpb].reshape(-1)       # rows of Y that a kept tile owns
    for k in ("add_tiles.y", "add_tiles_twin.y"):
        assert bool((out[k][~tile_rows] == SENTINEL).all()), k + ": a row of a skipped tile was written"
        assert not bool((out[k][tile_rows][:, :c.Cout] == SENTINEL).any()), k
    for k in ("add_tiles_twin.yd", "moments_tiles_twin.yd"):
        assert not bool((out[k][:, :c.Cout] == SENTINEL).any()), k


def check_claims(c, out):
    """DESIGN.md 4.11, asserted when recording: the moments do not depend on Y, and pdr_gather_moments* equals
    pdr_gather_add* on the windows' columns."""
    w = c.in_windows()
    ref = out["add_y_whole.moments"]
    assert torch.equal(out["add_y_window.moments"], ref) and torch.equal(out["add_no_y.moments"], ref)
    assert torch.equal(out["add_no_partial.y"], out["add_y_whole.y"])
    assert torch.equal(out["add_y_window.y"][:, :c.res[1]], out["add_y_whole.y"][:, c.res[0]:c.res[0] + c.res[1]])
    assert torch.equal(out["moments.moments"][:, w], ref[:, w]), "pdr_gather_moments differs from pdr_gather_add"
    if "add_tiles.moments" in out:
        assert torch.equal(out["moments_tiles.moments"][:, w], out["add_tiles.moments"][:, w])
        assert torch.equal(out["moments_tiles_twin.moments"][:, w], out["add_tiles_twin.moments"][:, w])
        assert torch.equal(out["moments_tiles_twin.yd"], out["add_tiles_twin.yd"])
        assert torch.equal(out["add_tiles_twin.y"], out["add_tiles.y"])


def run_case(lib, dev, cid, st):
    c = make_case(dev, cid)
    out = run_plain(lib, c, st)
    if cid == TILES_CASE:
        out.update(run_tiles(lib, c, st))
    return c, out


def to_record(out):
    """Moments raw, Y / Yd as digests."""
    return {k: (v.cpu().numpy() if k.endswith(".moments") else digest(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--lib", default=None, help="the library to record from (default: the package's own)")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = args.lib
    lib, dev = _lib.load(), torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rec = {}
    for spec in CASES:
        c, out = run_case(lib, dev, spec[0], st)
        check_unwritten(c, out)
        check_claims(c, out)
        for k, v in to_record(out).items():
            rec["%s/%s" % (spec[0], k)] = v
        print("%-18s %2d outputs, windows bit-equal to the whole width" % (spec[0], len(out)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (args.out, len(rec), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
