"""Cases of pdr_fused_layer_pool / pdr_fused_layer_pool_f16x3 across their dispatch table, and a float64 reference
written from include/pdr_hip.h and attention.py:83-96.  (A helper module like tests/layer_cases.py, not a conftest.)

A `PoolCase` is a plain-form `layer_cases.Case` (no statistics, no residual, no per-query output term: the score conv)
plus the pooled fields.  `build(case, dev)` makes device tensors and the pdr_layer_in_t; `build(case, None)` fills the
same struct with fake addresses for the host-only plan.  `expected(P)` is what `out` must hold after the call.

REFERENCE (float64, never the kernel): s = the scores and S = their magnitude sums of layer_cases.reference; counts are
clamped to at least 1 (an empty ball pools its slot 0); masked slots are exactly -1e9; p = softmax over the K slots of a
query; v = act(values * vscale[b] + vshift[b]); out[q] = sum_k p_k v_k.

BOUND, derived and not tuned.  For query q and column c, over the valid slots,
    E     = max_k ( e_k + 4 u (|s_k| + |max_k s|) )
    e_k   = 2 (Cin + 4) u S_k                                                 exact entry point
    e_k   = 2 (Cin + 4) u S_k + 2^-21 S_k + 2^-25 (|x_row|_1 + |w_col|_1)     split-f16 entry point
    bound = expm1(2 E) sum_k p_k |v_k - out|  +  2 (K + 8) u sum_k p_k (|values vscale| + |vshift|).
e_k is the worst-case error of an fp32 dot product of Cin + 4 terms (layer_cases.y_bound); the split form adds what its
operand contract in the header allows: each operand held to max(2^-23 |x|, 2^-25) and the dropped lo x lo product,
2^-22 relative -- together below 2^-21 S_k -- plus the absolute floors 2^-25 against the other operand's magnitudes.
4 u (|s| + |m|) covers the roundings of the log2(e) scaling, of the maximum subtraction and of the exponential's
argument.  If every score moves by at most E, every ratio of two softmax weights moves by a factor of at most e^{2E};
the weight changes sum to 0, so the weighted mean moves by at most expm1(2E) times the weighted mean absolute deviation
of v: the first term.  The second is the fp32 error of the K-term sums for numerator and denominator, the value FMA
and the division, (K + 8) roundings each way, on the magnitudes that enter them.  A patched row (pdr_layer_in_t.
patch_values) is one FMA and one maximum: 2 u (|patch vscale| + |vshift|).

INPUTS THAT MAKE FAULTS LOUD: value rows of masked slots hold +-1e6 (finite: 0 * NaN is NaN in the reference as well),
valid slots O(1); one family has |s| ~ 100 (a missing maximum subtraction overflows); vscale / vshift differ between
batch elements; source rows differ between every pair of positions; padding columns of `values`, of the patch rows and
of the sources are NaN; `out` is NaN-prefilled.
"""
import ctypes
import dataclasses

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib
from tests import layer_cases as lc

U = lc.U
options = lc.options
COUNT_MODES = ("none", "random", "zero", "full", "one")
TILE_COLS = {0: 32, 1: 64, 2: 96, 3: 160, 4: 128, 5: 128, 6: 128, 7: 32, 8: 64}   # tile_tn() over pdr::kTiles
OPTION_SETS = {k: lc.OPTION_SETS[k] for k in ("defaults", "narrow_kc32=0", "fused_ws=0", "fused_ws=0,narrow_kc32=0")}
# resident workgroups of a pooled wave-specialised launch (launch_fused_layer_ws): 768 for the narrow variant 7
RESIDENT = {7: 768}
# refusal mutations of a built pdr_layer_in_t
MUTATIONS = ("rseg", "oadd", "gathered", "row_div2", "nchunks", "no_n_tiles")


@dataclasses.dataclass
class PoolCase:
    B: int
    rpb: int
    segs: tuple
    D: int
    K: int = 8
    counts: str = "random"
    v_relu: bool = True
    vscale: bool = True
    vshift: bool = True
    ldv_extra: int = 0              # ldv = pad4(D) + ldv_extra
    ldo_extra: int = 0
    tile_list: bool = False         # a hand-built ascending subset of the 128-row tiles
    out_rows: bool = False          # a random permutation of the queries
    patch: bool = False             # patch_values / patch_w (K on the queries of unlisted tiles)
    split: bool = False             # pdr_fused_layer_pool_f16x3
    score_scale: float = 1.0
    pre: bool = False
    post: bool = False
    ss: bool = False
    ss_extra: int = 0
    add: bool = False
    bias: bool = True
    unaligned: bool = False
    mutate: str = ""                # one of MUTATIONS
    want_rc: int = _lib.PDR_OK      # what plan and launch must return
    seed: int = 0
    tag: str = ""

    @property
    def Cin(self):
        return sum(self.segs)

    @property
    def P(self):
        return self.B * self.rpb

    @property
    def nq(self):
        return self.P // self.K

    @property
    def ldv(self):
        return lc.pad4(self.D) + self.ldv_extra

    @property
    def ldo(self):
        return lc.pad4(self.D) + self.ldo_extra

    def layer_case(self):
        return lc.Case(B=self.B, rpb=self.rpb, segs=self.segs, Cout=self.D, form="plain", stats=False, pre=self.pre,
                       post=self.post, ss=self.ss, ss_extra=self.ss_extra, add=self.add, bias=self.bias,
                       unaligned=self.unaligned, seed=self.seed, tag=self.tag)

    def label(self):
        f = ["B%d" % self.B, "rpb%d" % self.rpb, "cin%s" % "+".join(map(str, self.segs)), "D%d" % self.D, "K%d" % self.K,
             "counts=" + self.counts, "ldv+%d" % self.ldv_extra, "ldo+%d" % self.ldo_extra]
        for k in ("v_relu", "vscale", "vshift", "tile_list", "out_rows", "patch", "split", "pre", "post", "ss", "add",
                  "bias", "unaligned"):
            if getattr(self, k):
                f.append(k)
        if self.score_scale != 1.0:
            f.append("s*%g" % self.score_scale)
        if self.mutate:
            f.append("mutate=" + self.mutate)
        return "-".join(f) + ("[%s]" % self.tag if self.tag else "")


def variant(rpb, D, opts):
    """pick_tile (csrc/fused_layer.hip), restated: the tile variant of rows_per_batch x D under an option set."""
    narrow = opts.get("narrow_kc32", 1)
    if narrow and rpb >= 128 and D <= 64:
        return 7 if D <= 32 else 8
    if rpb >= 256 and D <= 64:
        return 0 if D <= 32 else 1
    if rpb >= 128:
        return 2 if D <= 96 else 3 if 128 < D <= 160 else 4
    return 5 if rpb >= 64 else 6


def expected_plan(case, opts):
    """The 8 ints pdr_fused_layer_pool_plan must report for an accepted case, from the header's rules alone."""
    v = variant(case.rpb, case.D, opts)
    tm = lc.TILE_ROWS[v]
    ws = bool(opts.get("fused_ws", 1)) and case.rpb % tm == 0 and v not in (3, 6)
    return [int(ws), v, int(case.split), case.B * ((case.rpb + tm - 1) // tm), (case.D + TILE_COLS[v] - 1) // TILE_COLS[v],
            int(case.tile_list), int(case.out_rows), int(case.patch)]


class Pooled:
    """A built pooled case: the score layer (layer_cases.Layer) and the pooled tensors (or fake addresses)."""

    def __init__(self, case, L):
        self.case, self.L, self.dev = case, L, L.dev
        self.keep = {}
        self.nchunks = sum((C + 31) // 32 for C in case.segs)

    def ptr(self, name):
        t = self.keep.get(name)
        return None if t is None else t.data_ptr()

    def _weights(self):
        c = self.case
        if c.split:
            return self.ptr("Wp"), self.nchunks + (1 if c.mutate == "nchunks" else 0)
        return self.L.ptr("Wt"), lc.pad4(c.D)

    def new_out(self):
        return torch.full((self.case.nq, self.case.ldo), float("nan"), device=self.dev)

    def plan(self, out_addr=None):
        """(rc, plan[8]) of pdr_fused_layer_pool_plan."""
        c = self.case
        W, ldw = self._weights()
        plan = (ctypes.c_int * 8)(*([-7] * 8))
        rc = _lib.load().pdr_fused_layer_pool_plan(ctypes.byref(self.L.li), c.P, c.Cin, W, ldw, c.D, self.ptr("values"),
                                                   c.ldv, c.K, out_addr or self.ptr("out") or 1 << 20, c.ldo, int(c.split), plan)
        return rc, list(plan)

    def launch(self, out):
        c = self.case
        W, ldw = self._weights()
        fn = _lib.load().pdr_fused_layer_pool_f16x3 if c.split else _lib.load().pdr_fused_layer_pool
        rc = fn(ctypes.byref(self.L.li), c.P, c.Cin, W, ldw, self.L.ptr("bias"), c.D, self.ptr("values"), c.ldv,
                self.ptr("vscale"), self.ptr("vshift"), int(c.v_relu), self.ptr("counts"), c.K, out.data_ptr(), c.ldo,
                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def listed_tiles(case):
    """(B, tiles per cloud) of the hand-built tile subset: cloud 0 empty, cloud 1 full, cloud 2 its even tiles, ..."""
    tpb = (case.rpb + 127) // 128
    m = np.zeros((case.B, tpb), dtype=bool)
    for b in range(case.B):
        if b % 3 == 1:
            m[b] = True
        elif b % 3 == 2:
            m[b, ::2] = True
    return m


def build(case, dev):
    c = case
    L = lc.build(c.layer_case(), dev)
    P = Pooled(c, L)
    real = dev is not None
    li = L.li
    g = torch.Generator(device=dev).manual_seed(7919 * c.seed + 31 * c.rpb + c.D + 1000003 * c.K) if real else None
    nan = float("nan")

    def keep(name, t_or_bytes):
        P.keep[name] = t_or_bytes if real else lc._Fake(t_or_bytes)
        return P.keep[name]

    def randn(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    nq, K, D, B = c.nq, c.K, c.D, c.B
    qpb = c.rpb // K if c.rpb % K == 0 else 0
    if not real:
        for name, n in (("values", c.P * c.ldv), ("out", max(nq, 1) * c.ldo)):
            keep(name, 4 * n)
        if c.vscale:
            keep("vscale", 4 * B * D)
        if c.vshift:
            keep("vshift", 4 * B * D)
        if c.counts != "none":
            keep("counts", 4 * max(nq, 1))
        if c.split:
            keep("Wp", 2 * 2 * 128 * 32 * P.nchunks * ((D + 63) // 64))
    else:
        # NaN in the padding columns of the sources (the reference was taken from the first C columns)
        for si, C in enumerate(c.segs):
            L.keep["x%d" % si][:, C:] = nan
        if c.score_scale != 1.0:
            L.keep["Wt"].mul_(c.score_scale)
        if c.split:
            from point_diffusion_refinement_amd.pointnet2.fused_network import pack_f16x3
            v = variant(c.rpb, D, {})
            img, nch = pack_f16x3(L.keep["Wt"], D, c.segs, TN=64 if v == 8 else 128)
            assert nch == P.nchunks
            keep("Wp", img)
        # counts
        cnt = None
        if c.counts != "none":
            if c.counts == "random":
                cnt = torch.randint(0, K + 1, (nq,), device=dev, generator=g, dtype=torch.int32)
                if qpb:
                    cnt.view(B, qpb)[:, 0] = 0                  # every cloud has an empty ball and a full one
                    cnt.view(B, qpb)[:, -1] = K if qpb > 1 else 0
            else:
                cnt = torch.full((nq,), {"zero": 0, "full": K, "one": 1}[c.counts], device=dev, dtype=torch.int32)
            keep("counts", cnt)
        valid = torch.full((nq,), K, device=dev) if cnt is None else cnt.long().clamp(min=1)
        P.valid = valid
        # values: O(1) in the valid slots, +-1e6 in the masked ones, NaN in the padding columns
        V = torch.full((c.P, c.ldv), nan, device=dev)
        V[:, :D] = randn(c.P, D)
        if c.rpb % K == 0:
            slot = torch.arange(c.P, device=dev) % K
            masked = slot >= valid.repeat_interleave(K)
            big = torch.where(randn(c.P, D) > 0, 1e6, -1e6)
            V[:, :D] = torch.where(masked[:, None], big, V[:, :D])
        keep("values", V)
        if c.vscale:
            keep("vscale", torch.rand(B, D, device=dev, generator=g) * 3 - 1.5)
        if c.vshift:
            keep("vshift", randn(B, D))
    # subset / row map / patched rows
    if c.tile_list:
        lt = listed_tiles(c)
        sel = np.flatnonzero(lt.reshape(-1)).astype(np.int32)
        P.listed = lt
        if real:
            tl = torch.full((lt.size,), -1, device=dev, dtype=torch.int32)
            tl[:len(sel)] = torch.from_numpy(sel).to(dev)
            keep("tile_list", tl)
            keep("n_tiles", torch.tensor([len(sel)], device=dev, dtype=torch.int32))
        else:
            keep("tile_list", 4 * lt.size)
            keep("n_tiles", 4)
        li.tile_list = P.ptr("tile_list")
        li.n_tiles = None if c.mutate == "no_n_tiles" else P.ptr("n_tiles")
    if c.out_rows:
        keep("out_rows", torch.randperm(nq, device=dev, generator=g).int() if real else 4 * nq)
        li.out_rows = P.ptr("out_rows")
    if c.patch:
        pld = lc.pad4(D) + 4
        if real:
            pv = torch.full((nq, pld), nan, device=dev)
            pv[:, :D] = randn(nq, D)
            pw = torch.zeros(nq, device=dev)
            if c.tile_list and c.rpb % 128 == 0:
                unlisted = ~torch.from_numpy(listed_tiles(c)).to(dev).reshape(-1)
                pw = unlisted.repeat_interleave(128 // K).float() * K
            # the patch rows of the queries that are not patched are loud
            pv[:, :D] = torch.where((pw > 0)[:, None], pv[:, :D], torch.where(randn(nq, D) > 0, 1e6, -1e6))
            keep("patch_values", pv)
            keep("patch_w", pw)
        else:
            keep("patch_values", 4 * nq * pld)
            keep("patch_w", 4 * nq)
        li.patch_values, li.patch_w, li.patch_ld = P.ptr("patch_values"), P.ptr("patch_w"), pld
    # refusal mutations
    if c.mutate == "rseg":
        li.rseg.ptr, li.rseg.C, li.rseg.ld, li.rseg.row_div = L.ptr("x0"), c.Cin, lc.pad4(c.Cin), 1
    elif c.mutate == "oadd":
        li.oadd, li.oadd_ld, li.oadd_div = P.ptr("values"), c.ldv, K
    elif c.mutate == "gathered":
        li.seg[0].gV, li.seg[0].g_ldv, li.seg[0].g_nsrc = P.ptr("values"), c.ldv, 1
    elif c.mutate == "row_div2":
        li.seg[0].row_div = 2
    return P


def pool_reference(s, e, raw, cnt, vs, vh, v_relu, fault=None):
    """The pooling itself in float64: s, e (scores and their error allowance) and raw (value rows) are (nq, K, D), cnt
    (nq,) counts or None, vs / vh (nq, 1, D) the value scale and shift of every query's batch element.  Returns the
    pooled rows and their bound (module docstring)."""
    nq, K, D = s.shape
    dev = s.device
    cnt = torch.full((nq,), K, device=dev) if cnt is None else cnt.long()
    k = torch.arange(K, device=dev)
    ok_true = k[None] < cnt.clamp(min=1)[:, None]                                              # (nq, K)
    if fault != "no_clamp":
        cnt = cnt.clamp(min=1)
    ok = (k[None] <= cnt[:, None]) if fault == "mask_le" else (k[None] < cnt[:, None])
    p = torch.softmax(torch.where(ok[..., None], s, torch.full_like(s, -1e9)), 1)
    if fault == "next_query":
        raw = raw.roll(-1, 0)
    if fault == "reversed":
        raw = raw.flip(1)
    v = raw * vs + vh
    if v_relu and fault != "no_relu":
        v = v.relu()
    out = (p * v).sum(1)
    neg = torch.full_like(s, -float("inf"))
    m = torch.where(ok_true[..., None], s, neg).amax(1, keepdim=True)
    E = torch.where(ok_true[..., None], e + 4.0 * U * (s.abs() + m.abs()), neg).amax(1)
    bound = torch.expm1(2.0 * E) * (p * (v - out[:, None]).abs()).sum(1) + \
        2.0 * (K + 8) * U * (p * ((raw * vs).abs() + vh.abs())).sum(1)
    return out, bound


def reference(P, fault=None):
    """(out64, bound): (P / K, D) float64 pooled rows in QUERY order and their error bound (module docstring).
    `fault`: a planted fault of the reference itself, for the self-check of tests/test_pool_dispatch_plan.py."""
    c, L, dev = P.case, P.L, P.dev
    K, D, nq = c.K, c.D, c.nq
    s, S = lc.reference(L)
    e = 2.0 * (c.Cin + 4) * U * S
    if c.split:
        xn = L.x64.abs().sum(1, keepdim=True)
        wn = L.keep["Wt"][:, :D].double().abs().sum(0, keepdim=True)
        e = e + 2.0 ** -21 * S + 2.0 ** -25 * (xn + wn)
    b = torch.arange(nq, device=dev) // (c.rpb // K)
    if fault == "vscale_b0":
        b = torch.zeros_like(b)
    one = torch.ones(nq, 1, D, device=dev, dtype=torch.float64)
    vs = P.keep["vscale"].double()[b][:, None] if "vscale" in P.keep else one
    vh = P.keep["vshift"].double()[b][:, None] if "vshift" in P.keep else 0.0 * one
    return pool_reference(s.view(nq, K, D), e.view(nq, K, D), P.keep["values"][:, :D].double().view(nq, K, D),
                          P.keep.get("counts"), vs, vh, c.v_relu, fault)


def expected(P, fault=None):
    """(want, bound, written): rows of `out` (P / K, D) in float64 with their bounds, and the (P / K,) mask of the rows
    the call writes; every other row, and every column >= D, keeps what it held."""
    c, dev = P.case, P.dev
    K, D, nq = c.K, c.D, c.nq
    ref, bnd = reference(P, fault)
    listed_q = torch.ones(nq, dtype=torch.bool, device=dev)
    if c.tile_list:
        listed_q = torch.from_numpy(P.listed).to(dev).reshape(-1).repeat_interleave(128 // K)
    rows = P.keep["out_rows"].long() if c.out_rows and fault != "no_out_rows" else torch.arange(nq, device=dev)
    want = torch.full((nq, D), float("nan"), device=dev, dtype=torch.float64)
    bound = torch.zeros_like(want)
    written = torch.zeros(nq, dtype=torch.bool, device=dev)
    if c.patch:
        pw = P.keep["patch_w"] > 0
        if fault == "patch_listed":
            pw = torch.ones_like(pw)
        b = torch.arange(nq, device=dev) // (c.rpb // K)
        pv = P.keep["patch_values"][:, :D].double()
        vs = P.keep["vscale"].double()[b] if "vscale" in P.keep else torch.ones_like(pv)
        vh = P.keep["vshift"].double()[b] if "vshift" in P.keep else torch.zeros_like(pv)
        a = pv * vs + vh
        if c.v_relu:
            a = a.relu()
        want[rows[pw]] = a[pw]
        bound[rows[pw]] = (2.0 * U * ((pv * vs).abs() + vh.abs()))[pw]
        written[rows[pw]] = True
        if fault == "patch_listed":
            return want, bound, written
    want[rows[listed_q]] = ref[listed_q]
    bound[rows[listed_q]] = bnd[listed_q]
    written[rows[listed_q]] = True
    return want, bound, written


# planted faults of the reference and the cases that exercise them
FAULTS = {
    "mask_le": lambda c: c.counts in ("random", "zero", "one"),
    "no_clamp": lambda c: c.counts in ("random", "zero"),
    "no_relu": lambda c: c.v_relu,
    "vscale_b0": lambda c: c.vscale,
    "next_query": lambda c: True,
    "reversed": lambda c: True,
    "no_out_rows": lambda c: c.out_rows,
    "patch_listed": lambda c: c.patch,
}


# ---- generators --------------------------------------------------------------------------------------------------
SEG_SETS = [(64,), (33,), (100,), (259,), (16, 17), (33, 31, 36), (20, 12, 40, 8), (64, 64), (100, 33), (40,)]


def _features(i):
    """Deterministic mix of the optional features for the i-th case of a family."""
    return dict(counts=COUNT_MODES[i % 5], v_relu=i % 2 == 0, vscale=i % 3 != 1, vshift=i % 4 != 2, bias=i % 7 != 3,
                ldv_extra=(0, 4, 36)[i % 3], ldo_extra=(0, 4, 36)[(i // 2) % 3], pre=bool(i & 1), post=bool(i & 2),
                ss=bool((i + 1) & 2), ss_extra=(0, 0, 3)[i % 3], add=bool(i & 4), segs=SEG_SETS[i % len(SEG_SETS)],
                score_scale=100.0 if i % 4 == 1 else 1.0)


def _cell(rpb, D, i0, tag, Ks=(8, 16, 32), **kw):
    out = []
    for j, K in enumerate(Ks):
        i = i0 + j
        f = _features(i)
        f.update(kw)
        out.append(PoolCase(B=2 + i % 2, rpb=rpb, D=D, K=K, seed=i, tag=tag, **f))
    return out


# wave-specialised cells under the default options: (variant, Ds, rows per cloud of one tile and of three)
WS_DEFAULT = ((7, (8, 32), (128, 384)), (8, (33, 35, 64), (128, 384)), (2, (65, 96), (128, 384)),
              (4, (100, 128, 200, 256), (128, 384)), (5, (128,), (64,)))
WS_NARROW0 = ((0, (8, 32), (256, 768)), (1, (33, 64), (256, 768)))
# uniform-wave cells under every option set: (variant, D, rows per cloud)
UNIFORM_DEFAULT = ((3, 129, 128), (3, 160, 384), (6, 64, 32), (5, 100, 96), (7, 32, 160), (8, 64, 416), (4, 128, 160),
                   (4, 200, 416))
UNIFORM_NARROW0 = ((0, 32, 384),)
MANY_D = {0: 8, 1: 36, 2: 68, 4: 100, 5: 100, 7: 8, 8: 36}


def many_tiles(v, opt):
    """More row tiles than the persistent grid has workgroups (rows from layer_cases._many_tiles, cut to whole tiles):
    after its first tile a workgroup re-seeds the accumulators with the bias inside the pooled epilogue."""
    m = lc._many_tiles(v, "plain", opt, "ws")
    tm = lc.TILE_ROWS[v]
    tpb = 1 if v == 5 else m.rpb // tm
    tiles = RESIDENT.get(v, lc.RESIDENT["ws"]) + 7
    B = (tiles + tpb - 1) // tpb
    if B % 8 == 0:
        B += 1
    return PoolCase(B=B, rpb=tpb * tm, segs=(20,), D=MANY_D[v], K=(8, 16, 32)[v % 3], counts="random", ss=True, post=True,
                    seed=50 + v, tag="%s v%d many" % (opt, v))


def subset_cases(opt):
    """Tile subset, row map and patched rows on the 128-row wave-specialised variants (D a multiple of 4)."""
    out = []
    combos = ((True, False, False), (True, True, False), (True, False, True), (True, True, True), (False, True, False),
              (False, True, True), (False, False, True))
    shapes = ((7, 32), (8, 64), (2, 96), (4, 200), (4, 128))
    for i, (tl, orow, patch) in enumerate(combos):
        for j, (v, D) in enumerate(shapes):
            f = _features(3 * i + j)
            f.update(ldo_extra=(0, 4, 36)[(i + j) % 3])
            out.append(PoolCase(B=3, rpb=(384, 128, 256)[(i + j) % 3], D=D, K=(8, 16, 32)[(i + j) % 3], tile_list=tl,
                                out_rows=orow, patch=patch, seed=200 + 7 * i + j, tag="%s subset v%d" % (opt, v), **f))
    return out


def refusals(opt):
    """Calls both the plan and the launch must refuse, with the code."""
    EU, EI = _lib.PDR_EUNSUPPORTED, _lib.PDR_EINVAL
    base = dict(B=2, segs=(64,), tag=opt + " refused")
    out = []
    if opt == "defaults":
        out += [PoolCase(rpb=128, D=64, K=4, want_rc=EU, **base)]
        out += [PoolCase(rpb=128, D=64, mutate=m, want_rc=EU, **base) for m in ("rseg", "oadd", "gathered", "row_div2")]
        out += [PoolCase(rpb=48, D=64, K=8, want_rc=EI, **base), PoolCase(rpb=200, D=64, K=8, want_rc=EI, **base)]
        out += [PoolCase(rpb=128, D=64, unaligned=True, want_rc=EU, **base)]
        # a tile list, row map or patch where the uniform-wave kernel would run: a partial last tile, variant 3
        for kw in (dict(tile_list=True), dict(out_rows=True), dict(patch=True)):
            out += [PoolCase(rpb=160, D=64, want_rc=EU, **kw, **base), PoolCase(rpb=256, D=132, want_rc=EU, **kw, **base)]
        out += [PoolCase(rpb=64, D=128, tile_list=True, want_rc=EU, **base)]             # 64-row tiles
        out += [PoolCase(rpb=128, D=64, tile_list=True, mutate="no_n_tiles", want_rc=EU, **base)]
    if opt == "narrow_kc32=0":
        out += [PoolCase(rpb=256, D=64, tile_list=True, want_rc=EU, **base)]             # 256-row tiles
    if opt.startswith("fused_ws=0"):
        for kw in (dict(tile_list=True), dict(out_rows=True), dict(patch=True)):
            out += [PoolCase(rpb=256, D=64, want_rc=EU, **kw, **base)]
    if opt == "split":
        out += [PoolCase(rpb=128, D=96, split=True, want_rc=EU, **base), PoolCase(rpb=128, D=32, split=True, want_rc=EU, **base)]
        out += [PoolCase(rpb=128, D=129, split=True, want_rc=EU, **base), PoolCase(rpb=160, D=128, split=True, want_rc=EU, **base)]
        out += [PoolCase(rpb=128, D=128, split=True, mutate="nchunks", want_rc=EI, **base)]
    return out


def targeted(opt):
    """Targeted cases of option set `opt` (a key of OPTION_SETS, or "split": the f16x3 entry point, default options)."""
    cases, i = [], 0
    if opt == "split":
        for v, D, rpb in ((4, 128, 128), (4, 200, 384), (4, 100, 256), (5, 128, 64), (5, 68, 64), (8, 64, 128), (8, 36, 384)):
            for K in (8, 16, 32):
                f = _features(i)
                f.update(segs=((64,), (100,), (64, 33), (259,), (96, 64))[i % 5])
                cases.append(PoolCase(B=2 + i % 2, rpb=rpb, D=D, K=K, split=True, seed=300 + i, tag="split v%d" % v, **f))
                i += 1
        f = _features(1)
        f.update(segs=(64, 36))
        cases += [PoolCase(B=3, rpb=256, D=D, K=16, split=True, tile_list=True, out_rows=True, patch=True, seed=340 + D,
                           tag="split subset", **f) for D in (64, 128)]
        cases.append(dataclasses.replace(many_tiles(4, opt), split=True, segs=(64,)))
        return cases + refusals(opt)
    narrow0 = "narrow_kc32=0" in opt
    for v, Ds, rpbs in (WS_NARROW0 if narrow0 else WS_DEFAULT):
        for D in Ds:
            for rpb in rpbs:
                cases += _cell(rpb, D, i, "%s v%d" % (opt, v))
                i += 3
    for v, D, rpb in (UNIFORM_NARROW0 if narrow0 else UNIFORM_DEFAULT):
        cases += _cell(rpb, D, i, "%s uniform v%d" % (opt, v))
        i += 3
    if not opt.startswith("fused_ws=0"):
        cases += [many_tiles(v, opt) for v in ((0, 1) if narrow0 else (2, 4, 5, 7, 8))]
    if opt == "defaults":
        cases += subset_cases(opt)
        # whole groups of 8 clouds: the XCD-local tile order of ws_xcd_order = 2
        cases.append(PoolCase(B=8, rpb=384, segs=(33,), D=64, K=16, counts="random", ss=True, seed=77, tag="xcd order"))
    return cases + refusals(opt)


def required_cells(opt):
    """(wave-specialised?, variant, D, rows per cloud) of every cell of the table `targeted(opt)` must reach, plus
    ("many", variant) and ("subset", variant, tile_list, out_rows, patch)."""
    if opt == "split":
        return [(1, 4, 128, 128), (1, 4, 200, 384), (1, 5, 128, 64), (1, 8, 64, 128), ("many", 4),
                ("subset", 8, 1, 1, 1), ("subset", 4, 1, 1, 1)]
    narrow0 = "narrow_kc32=0" in opt
    ws_on = not opt.startswith("fused_ws=0")
    cells = []
    for v, Ds, rpbs in (WS_NARROW0 if narrow0 else WS_DEFAULT):
        cells += [(int(ws_on), v, D, rpb) for D in Ds for rpb in rpbs]
    cells += [(0, v, D, rpb) for v, D, rpb in (UNIFORM_NARROW0 if narrow0 else UNIFORM_DEFAULT)]
    if ws_on:
        cells += [("many", v) for v in ((0, 1) if narrow0 else (2, 4, 5, 7, 8))]
    if opt == "defaults":
        cells += [("subset", v, tl, orow, patch) for v in (2, 4, 7, 8)
                  for tl, orow, patch in ((1, 0, 0), (1, 1, 1), (0, 1, 0))]
    return cells


def cells_of(case, plan):
    """The cells of required_cells() an accepted case reaches, from the plan the library returned."""
    ws, v = plan[0], plan[1]
    out = [(ws, v, case.D, case.rpb)]
    resident = (RESIDENT.get(v, 512) + plan[4] - 1) // plan[4]
    if ws and plan[3] > resident and not plan[5]:
        out.append(("many", v))
    if plan[5] or plan[6] or plan[7]:
        out.append(("subset", v, plan[5], plan[6], plan[7]))
    return out


def random_cases(opt, n, seed=0):
    """A seeded stream of random accepted cases that mixes the features (every option set gets its own stream)."""
    rng = np.random.default_rng(seed * 7919 + sum(map(ord, opt)))
    split = opt == "split"
    opts = {} if split else OPTION_SETS[opt]
    out = []
    while len(out) < n:
        i = len(out)
        K = int(rng.choice([8, 16, 32]))
        rpb = int(rng.choice([64, 128, 256] if split else [32, 64, 96, 128, 160, 256, 384, 416, 512, 1024]))
        D = int(rng.choice([64, 100, 128, 200] if split else [3, 8, 32, 33, 35, 64, 65, 96, 100, 128, 129, 160, 200, 256]))
        v = variant(rpb, D, opts)
        if split and v not in (4, 5, 8):
            continue
        nseg = int(rng.integers(1, 5))
        segs = tuple(int(rng.choice([64, 100] if split else [3, 16, 17, 33, 64, 100])) for _ in range(nseg))
        if sum(segs) > 260:
            segs = segs[:2]
        ws = bool(opts.get("fused_ws", 1)) and rpb % lc.TILE_ROWS[v] == 0 and v not in (3, 6)
        sub = ws and lc.TILE_ROWS[v] == 128 and D % 4 == 0 and bool(rng.integers(0, 2))
        tl = sub and bool(rng.integers(0, 2))
        out.append(PoolCase(
            B=int(rng.choice([2, 3])), rpb=rpb, segs=segs, D=D, K=K, counts=str(rng.choice(COUNT_MODES)),
            v_relu=bool(rng.integers(0, 2)), vscale=bool(rng.integers(0, 3)), vshift=bool(rng.integers(0, 3)),
            ldv_extra=int(rng.choice([0, 4, 36])), ldo_extra=int(rng.choice([0, 4, 36])), tile_list=tl,
            out_rows=sub and bool(rng.integers(0, 2)), patch=sub and bool(rng.integers(0, 2)), split=split,
            score_scale=float(rng.choice([1.0, 1.0, 100.0, 0.01])), pre=bool(rng.integers(0, 2)),
            post=bool(rng.integers(0, 2)), ss=bool(rng.integers(0, 2)), ss_extra=int(rng.choice([0, 3])),
            add=bool(rng.integers(0, 2)), bias=bool(rng.integers(0, 4)), seed=20000 + i, tag="%s random %d" % (opt, i)))
    return out
