"""Cases of pdr_fused_layer across its dispatch table, and a float64 reference written from include/pdr_hip.h.

A `Case` describes one call: batch elements, rows per batch element, the input channel segments, Cout, the source
form and the optional features of pdr_layer_in_t.  `build(case, dev)` turns it into device tensors and a
`_lib.LayerIn`; `build(case, None)` fills the same struct with fake, correctly aligned addresses for the host-only
plan (nothing is allocated and nothing may be launched with it).  `reference(layer)` evaluates the documented
semantics in float64 on the device, with the magnitude sum S of every term that enters an output element, and
`reference_stats(layer, Y)` the per-tile moments of a given Y.  `targeted(opt_set)` and `random_cases(opt_set, n)`
are the generators.  (A helper module, not a conftest: the tests import it.)
"""
import contextlib
import ctypes
import dataclasses

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib

U = 2.0 ** -24                      # unit roundoff of fp32

# option sets the dispatch tests run under (process-wide pdr_set_option values)
OPTION_SETS = {
    "defaults": {},
    "narrow_kc32=0": {"narrow_kc32": 0},
    "fused_ws=0": {"fused_ws": 0},
    "fused_ws=0,narrow_kc32=0": {"fused_ws": 0, "narrow_kc32": 0},      # the uniform-wave 256-row tiles
    "deep_chunks=0": {"deep_chunks": 0},
    "deep_ks=0": {"deep_ks": 0},
    "ws_xcd_order=0": {"ws_xcd_order": 0},
    "ws_xcd_order=2": {"ws_xcd_order": 2},
    "ws_narrow3=0": {"ws_narrow3": 0},
}

# source forms: plain segments, plain residual, ball-gathered main source / residual, kNN-gathered main / residual
FORMS = ("plain", "residual", "ball", "ball_res", "knn", "knn_res")
GATHERED = ("ball", "ball_res", "knn", "knn_res")


@contextlib.contextmanager
def options(opts):
    """Set process-wide options for the duration of a block; the previous values come back in any case."""
    saved = {n: _lib.get_option(n) for n in _lib.option_names()}
    try:
        for n, v in opts.items():
            _lib.set_option(n, v)
        yield
    finally:
        for n, v in saved.items():
            _lib.set_option(n, v)


def pad4(n):
    return (n + 3) // 4 * 4


@dataclasses.dataclass
class Case:
    B: int
    rpb: int                        # rows per batch element
    segs: tuple                     # input channel widths, 1..4 segments
    Cout: int
    form: str = "plain"
    K: int = 8                      # gK of gathered forms (a power of two)
    div: tuple = ()                 # row_div per plain segment (default 1)
    ldy_extra: int = 0              # ldy = pad4(Cout) + ldy_extra
    unaligned: bool = False         # first segment with an odd leading dimension: scalar staging
    pre: bool = False
    post: bool = False
    ss: bool = False                # scale / shift rows
    ss_extra: int = 0               # ss_ld = Cin + ss_extra (0: ss_ld = 0, i.e. Cin)
    add: bool = False
    bias: bool = True
    oadd: bool = False
    odiv: int = 0                   # oadd_div (0: K)
    oadd_rows: bool = False
    relu_col0: int = 0
    stats: bool = True              # pass `partial`
    wrow0: bool = False
    wmul: float = 1.0
    ptpb_extra: int = -1            # partial_tpb = tiles per batch + extra (-1: partial_tpb = 0)
    tile_list: bool = False
    walk_reverse: int = 0
    empty: float = 0.3              # fraction of empty balls (ball forms)
    pair: bool = False              # run as the first problem of pdr_fused_layer_pair (second: pair_case())
    seed: int = 0
    tag: str = ""

    @property
    def Cin(self):
        return sum(self.segs)

    @property
    def P(self):
        return self.B * self.rpb

    @property
    def ldy(self):
        return pad4(self.Cout) + self.ldy_extra

    @property
    def ldw(self):
        return pad4(self.Cout)

    @property
    def oadd_div(self):
        return self.odiv or self.K

    def label(self):
        f = [self.form, "B%d" % self.B, "rpb%d" % self.rpb, "cin%s" % "+".join(map(str, self.segs)), "cout%d" % self.Cout]
        for k in ("unaligned", "pre", "post", "ss", "add", "oadd", "oadd_rows", "wrow0", "tile_list", "pair"):
            if getattr(self, k):
                f.append(k)
        if self.walk_reverse:
            f.append("rev")
        if not self.stats:
            f.append("nostats")
        if self.form in GATHERED or self.div:
            f.append("K%d" % self.K)
        f.append("rc%d" % self.relu_col0)
        return "-".join(f) + ("[%s]" % self.tag if self.tag else "")


def pair_case(c):
    """The second problem of a paired launch: plain source of the same width, weighted statistics, its own rows (on
    128-row tiles of the same variant when launched alone, as the network pairs them; the last one partial)."""
    return Case(B=c.B, rpb=168, segs=(c.Cin,), Cout=c.Cout, wrow0=True, wmul=float(c.K), relu_col0=c.relu_col0,
                ptpb_extra=1, seed=c.seed + 7)


class _Fake:
    """Stand-in for a device tensor in the host-only plan: an address, nothing behind it."""
    _next = 1 << 24

    def __init__(self, nbytes):
        self.addr = _Fake._next
        _Fake._next += (nbytes + 4095) // 4096 * 4096 + 4096

    def data_ptr(self):
        return self.addr


class Layer:
    """A built case: tensors (or fake addresses), the LayerIn, the weights and the output geometry."""

    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        self.keep = {}

    def ptr(self, name, off_floats=0):
        t = self.keep.get(name)
        return None if t is None else t.data_ptr() + 4 * off_floats

    @property
    def tm(self):
        return _lib.load().pdr_fused_layer_tile_rows(self.case.rpb, self.case.Cout)

    @property
    def tpb(self):
        return (self.case.rpb + self.tm - 1) // self.tm

    @property
    def ptpb(self):
        return self.tpb + self.case.ptpb_extra if self.case.ptpb_extra >= 0 else self.tpb

    def plan(self):
        """(rc, out[8]) of pdr_fused_layer_plan."""
        c = self.case
        out = (ctypes.c_int * 8)()
        rc = _lib.load().pdr_fused_layer_plan(ctypes.byref(self.li), c.P, c.Cin, self.ptr("Wt"), c.ldw, c.Cout,
                                              self.y_addr(), c.ldy, out)
        return rc, list(out)

    def y_addr(self):
        # the plan looks at Y's alignment only (thin kernel); a real launch passes its own tensor
        return self.keep["Y"].data_ptr() if "Y" in self.keep else 1 << 20


def build(case, dev, weights=None):
    """Device tensors (dev a torch.device) or fake addresses (dev None) for `case` and its LayerIn."""
    c = case
    L = Layer(c, dev)
    real = dev is not None
    g = torch.Generator(device=dev).manual_seed(1000003 * c.seed + 7919 * c.rpb + c.Cout) if real else None
    f32 = torch.float32

    def t(name, shape, kind="randn", lo=0, hi=1, dtype=f32):
        n = int(np.prod(shape))
        if not real:
            L.keep[name] = _Fake(4 * max(n, 1))
            return L.keep[name]
        if kind == "randn":
            x = torch.randn(*shape, device=dev, generator=g, dtype=dtype)
        elif kind == "rand":
            x = torch.rand(*shape, device=dev, generator=g, dtype=dtype) * (hi - lo) + lo
        else:
            x = torch.randint(lo, hi, shape, device=dev, generator=g, dtype=dtype)
        L.keep[name] = x
        return x

    P, B, rpb, K, Cin = c.P, c.B, c.rpb, c.K, c.Cin
    li = _lib.LayerIn()
    li.n_seg = len(c.segs)
    li.rows_per_batch = rpb
    nq = P // K if c.form in GATHERED else 0
    n_src = 3 * K + 5
    if c.form in GATHERED:
        t("gidx", (P,), "int", 0, n_src, torch.int32)
        li.gidx, li.gK = L.ptr("gidx"), K
        if c.form.startswith("ball"):
            cnt = t("gcnt", (nq,), "int", 1, K + 1, torch.int32)
            if real and c.empty > 0:
                cnt[torch.rand(nq, device=dev, generator=g) < c.empty] = 0
            li.gcnt = L.ptr("gcnt")
        else:
            t("gs1", (P,), "rand")
            t("gs2", (P,), "rand")
            li.gs1, li.gs2 = L.ptr("gs1"), L.ptr("gs2")

    def gathered_seg(s, prefix, C):
        """Fill pdr_seg_t s with a gathered table of C channels; returns (value, |terms|) in float64."""
        ld = pad4(C) + 4
        tab = t(prefix + "U", (B * n_src + 1, ld))
        if real:
            tab[-1].zero_()                                  # the table's all-zero row (g_zrow)
        s.ptr, s.C, s.ld, s.row_div = tab.data_ptr(), C, ld, 1
        s.g_nsrc, s.g_zrow = n_src, B * n_src
        if c.form.startswith("ball"):
            V2 = t(prefix + "V", (nq, 2 * ld))            # gV0 = the second half of every row: one allocation
            s.gV, s.gV0, s.g_ldv = V2.data_ptr(), V2.data_ptr() + 4 * ld, 2 * ld
        else:
            V = t(prefix + "V", (nq, ld))
            s.gV, s.g_ldv = V.data_ptr(), ld
            r1, r2 = t(prefix + "r1", (pad4(C),)), t(prefix + "r2", (pad4(C),))
            s.g_r1, s.g_r2 = r1.data_ptr(), r2.data_ptr()
        if not real:
            return None
        p = torch.arange(P, device=dev)
        b, q = p // rpb, p // K
        nb = tab[(b * n_src + L.keep["gidx"].long())][:, :C].double()
        if c.form.startswith("ball"):
            v = V2[q][:, :C].double()
            empty = (L.keep["gcnt"][q] <= 0)[:, None]
            v0 = V2[q][:, ld:ld + C].double()
            val = torch.where(empty, v0, nb + v)
            mag = torch.where(empty, v0.abs(), nb.abs() + v.abs())
        else:
            v = V[q][:, :C].double()
            t1 = L.keep["gs1"].double()[:, None] * r1[:C].double()[None]
            t2 = L.keep["gs2"].double()[:, None] * r2[:C].double()[None]
            val = nb + v + t1 + t2
            mag = nb.abs() + v.abs() + t1.abs() + t2.abs()
        return val, mag

    xs, ms = [], []
    for si, C in enumerate(c.segs):
        s = li.seg[si]
        if si == 0 and c.form in ("ball", "knn"):
            r = gathered_seg(s, "s0", C)
        else:
            d = c.div[si] if si < len(c.div) else 1
            ld = pad4(C) + (1 if (si == 0 and c.unaligned) else 4 * (si % 2))
            X = t("x%d" % si, (P // d, ld))
            s.ptr, s.C, s.ld, s.row_div = X.data_ptr(), C, ld, d
            r = None
            if real:
                v = X[:, :C].double().repeat_interleave(d, 0)
                r = (v, v.abs())
        if real:
            xs.append(r[0])
            ms.append(r[1])
    bidx = torch.arange(P, device=dev) // rpb if real else None
    if real:
        x, m = torch.cat(xs, 1), torch.cat(ms, 1)
    # prologue: x' = post(pre(x) * scale + shift) + add + residual
    li.pre_relu, li.post_relu = int(c.pre), int(c.post)
    if real and c.pre:
        x = x.relu()
    if c.ss:
        ssl = Cin + c.ss_extra if c.ss_extra else Cin
        li.ss_ld = Cin + c.ss_extra if c.ss_extra else 0
        sc, sh = t("scale", (B, ssl), "rand", -2, 2), t("shift", (B, ssl))
        li.scale, li.shift = sc.data_ptr(), sh.data_ptr()
        if real:
            a, s_ = sc[:, :Cin].double()[bidx], sh[:, :Cin].double()[bidx]
            x = x * a + s_
            m = m * a.abs() + s_.abs()
    if real and c.post:
        x = x.relu()
    if c.add:
        ald = Cin + 3
        ad = t("add", (B, ald))
        li.add, li.add_ld = ad.data_ptr(), ald
        if real:
            a = ad[:, :Cin].double()[bidx]
            x, m = x + a, m + a.abs()
    if c.form == "residual":
        R = t("res", (P, pad4(Cin) + 4 * (c.seed % 2)))
        li.rseg.ptr, li.rseg.C, li.rseg.ld, li.rseg.row_div = R.data_ptr(), Cin, R.shape[1] if real else pad4(Cin), 1
        if real:
            r = R[:, :Cin].double()
            x, m = x + r, m + r.abs()
    if c.form in ("ball_res", "knn_res"):
        r = gathered_seg(li.rseg, "r", Cin)
        if real:
            x, m = x + r[0], m + r[1]
    # weights, bias
    if weights is not None:
        L.keep["Wt"], L.keep["bias"] = weights
    else:
        Wt = t("Wt", (Cin, c.ldw))
        if real:
            Wt.mul_(1.0 / Cin ** 0.5)
        if c.bias:
            t("bias", (c.Cout,))
    # output-side per-query term
    if c.oadd:
        od = c.oadd_div
        nq_o = (P + od - 1) // od
        oa = t("oadd", (nq_o, c.ldw + 4))
        li.oadd, li.oadd_ld, li.oadd_div = oa.data_ptr(), c.ldw + 4, od
        if c.oadd_rows:
            perm = t("oadd_rows", (nq_o,), "int", 0, 1, torch.int32)
            if real:
                perm.copy_(torch.randperm(nq_o, device=dev, generator=g).int())
            li.oadd_rows = perm.data_ptr()
    if c.wrow0:
        w0 = t("wrow0", (B,), "int", 0, max(1, c.rpb), torch.int32)
        li.wrow0, li.wmul = w0.data_ptr(), c.wmul
    if c.ptpb_extra >= 0:
        li.partial_tpb = L.ptpb
    li.walk_reverse = c.walk_reverse
    if c.tile_list:
        ntile = B * L.tpb
        tl = t("tile_list", (ntile,), "int", 0, 1, torch.int32)
        nt = t("n_tiles", (1,), "int", 0, 1, torch.int32)
        if real:
            pick = torch.rand(ntile, device=dev, generator=g) < 0.5
            pick[0] = True
            sel = pick.nonzero()[:, 0].int()
            tl.fill_(-1)
            tl[:len(sel)] = sel
            nt.fill_(len(sel))
            L.picked = pick
        li.tile_list, li.n_tiles = tl.data_ptr(), nt.data_ptr()
    L.li = li
    if real:
        L.x64, L.m64 = x, m
    return L


def reference(L):
    """(Y64, S): float64 output of the documented semantics and the sum of |terms| of every element (P, Cout)."""
    c = L.case
    Wt = L.keep["Wt"][:, :c.Cout].double()
    y = L.x64 @ Wt
    S = L.m64 @ Wt.abs()
    if "bias" in L.keep:
        b = L.keep["bias"][:c.Cout].double()
        y, S = y + b, S + b.abs()
    if c.oadd:
        q = torch.arange(c.P, device=L.dev) // c.oadd_div
        if c.oadd_rows:
            q = L.keep["oadd_rows"].long()[q]
        o = L.keep["oadd"][q][:, :c.Cout].double()
        y, S = y + o, S + o.abs()
    return y, S


def y_bound(L, S):
    return 2.0 * (L.case.Cin + 4) * U * S


def reference_stats(L, Y):
    """float64 per-tile moments of the kernel's own Y (P, >= Cout) and their |.| sums: (B, tpb, Cout, 2) each."""
    c = L.case
    tm, tpb = L.tm, L.tpb
    y = Y[:, :c.Cout].double().view(c.B, c.rpb, c.Cout)
    col = torch.arange(c.Cout, device=L.dev)
    f = torch.where(col >= c.relu_col0, y.clamp_min(0), y)
    w = torch.ones(c.B, c.rpb, device=L.dev, dtype=torch.float64)
    if c.wrow0:
        r = torch.arange(c.rpb, device=L.dev)
        w = (r[None] >= L.keep["wrow0"].long()[:, None]).double() * c.wmul
    fw = f * w[..., None]
    pad = tpb * tm - c.rpb

    def tiles(v):
        v = torch.nn.functional.pad(v, (0, 0, 0, pad))
        return v.view(c.B, tpb, tm, c.Cout).sum(2)
    s1, s2 = tiles(fw), tiles(fw * f)
    a1, a2 = tiles(fw.abs()), tiles((fw * f).abs())
    return torch.stack([s1, s2], -1), torch.stack([a1, a2], -1)


# ---- generators --------------------------------------------------------------------------------------------------
# tile rows of each variant -- a copy of tile_tm() over pdr::kTiles (csrc/layer_tiles.h, the one table; Python cannot
# include it) -- and a Cout range that makes pick_tile (csrc/fused_layer.hip) select it
TILE_ROWS = {0: 256, 1: 256, 2: 128, 3: 128, 4: 128, 5: 64, 6: 32, 7: 128, 8: 128}
COUTS = {0: (3, 32), 1: (33, 64), 2: (65, 96), 3: (129, 160), 4: (97, 128, 161), 5: (3, 33, 129, 161),
         6: (3, 65, 161), 7: (3, 32), 8: (33, 64)}
# resident workgroups of the persistent grids: wave-specialised 512 / ncol, uniform-wave 1536 / ncol
RESIDENT = {"ws": 512, "uniform": 1536}
SEG_SETS = [(15,), (17,), (31, 2), (33,), (16, 16, 1), (41, 7, 9, 3), (64,), (12, 20)]


def _rpbs(v, gathered, K):
    """Row counts per batch element at the edges of variant v's tile: full tiles, partial last tiles (by 1 / TM-1 rows,
    by half a tile; whole queries for gathered sources), a single tile."""
    tm = TILE_ROWS[v]
    lo = {0: 256, 1: 256, 5: 64, 6: 1}.get(v, 128)     # smallest rpb that keeps the variant
    q = K if gathered else 1
    out = [("full", 2 * tm), ("single", tm), ("half", tm + tm // 2 if tm + tm // 2 >= lo else tm // 2)]
    if v == 5:
        out = [("full", 64), ("partial1", 64 + q), ("partialTm1", 128 - q), ("half", 96)]
    elif v == 6:
        out = [("full", 32), ("partial1", 32 + q), ("partialTm1", 64 - q), ("half", 48),
               ("tiny", q)]
    else:
        out += [("partial1", tm + q) if tm + q >= lo else ("partial1", 2 * tm + q),
                ("partialTm1", 2 * tm - q)]
    return [(n, r) for n, r in out if r % q == 0 and r >= 1]


def _features(i, Cout):
    """Deterministic mix of the optional features for the i-th case of a cell."""
    tn_edge = 32 if Cout > 32 else Cout
    rc = [0, min(16, Cout), tn_edge, Cout][i % 4]
    return dict(pre=bool(i & 1), post=bool(i & 2), ss=bool((i + 1) & 2), add=bool(i & 4), oadd=bool((i + 2) % 3 == 0),
                ldy_extra=(0, 4, 1, 8)[i % 4], ss_extra=(0, 0, 3)[i % 3], relu_col0=rc,
                ptpb_extra=(-1, 0, 2)[i % 3], bias=(i % 5) != 4)


def _cell_cases(v, form, opt, seed0):
    out = []
    gathered = form in GATHERED
    tm = TILE_ROWS[v]
    K = 4 if tm == 32 else (8 if tm <= 64 else 32 if form.startswith("ball") and seed0 % 2 else 8)
    for ci, Cout in enumerate(COUTS[v]):
        for i, (edge, rpb) in enumerate(_rpbs(v, gathered, K)):
            segs = SEG_SETS[(i + 3 * ci + seed0) % len(SEG_SETS)]
            if form in ("residual", "ball_res", "knn_res"):
                segs = (sum(segs),)
            B = (1, 5, 8, 16)[(i + ci) % 4]
            f = _features(i + ci + seed0, Cout)
            if gathered and f["oadd"]:
                f["odiv"] = 32 if rpb % 32 == 0 and tm % 32 == 0 else K
                f["oadd_rows"] = form in ("ball", "ball_res") and f["odiv"] >= 32
            out.append(Case(B=B, rpb=rpb, segs=segs, Cout=Cout, form=form, K=K, seed=seed0 + 31 * i + ci,
                            tag="%s v%d %s" % (opt, v, edge), **f))
    return out


def _many_tiles(v, form, opt, family):
    """More row tiles than the persistent grid holds resident workgroups: every workgroup walks several tiles."""
    tm = TILE_ROWS[v]
    Cout = COUTS[v][-1]
    ncol = 1
    if v in (4, 5, 6):
        ncol = (Cout + 127) // 128
    tiles = RESIDENT[family] // ncol + 7
    gathered = form in GATHERED
    K = 8
    rpb = {5: 96, 6: 48}.get(v, 3 * tm + (K if gathered else 5))
    tpb = (rpb + tm - 1) // tm
    B = (tiles + tpb - 1) // tpb
    if B % 8 == 0:
        B += 1                                    # not whole groups of 8 clouds (the XCD-local order's condition)
    return Case(B=B, rpb=rpb, segs=(20,), Cout=Cout, form=form, K=K, ss=True, post=True, oadd=v % 2 == 0,
                relu_col0=Cout // 2, seed=v * 11 + FORMS.index(form), tag="%s v%d many" % (opt, v))


WS_VARIANTS = (0, 1, 2, 4, 5, 7, 8)
UNIFORM_VARIANTS = tuple(range(9))
PAIR_VARIANTS = (2, 4, 7, 8)


def targeted(opt):
    """Targeted cases for option set `opt`: the dispatch cells it decides, at every edge."""
    cases = []
    if opt in ("defaults", "narrow_kc32=0"):
        vs = (0, 1) if opt == "narrow_kc32=0" else (2, 4, 5, 7, 8)
        for v in vs:
            for fi, form in enumerate(FORMS):
                cases += _cell_cases(v, form, opt, 17 * v + fi)
            cases.append(_many_tiles(v, "plain", opt, "ws"))
            cases.append(_many_tiles(v, "ball", opt, "ws"))
    if opt == "narrow_kc32=0":
        # variants 2 / 3 / 5 / 6 keep their shapes; 128..255 rows of <= 64 channels move to variant 2
        cases.append(Case(B=5, rpb=200, segs=(33,), Cout=40, ss=True, tag="narrow v2 from <=64"))
        cases += [advisor_case(cout) for cout in (32, 64)]
    if opt in ("fused_ws=0", "fused_ws=0,narrow_kc32=0"):
        for v in UNIFORM_VARIANTS if opt == "fused_ws=0" else (0, 1):
            for fi, form in enumerate(("plain", "residual", "ball")):
                cases += _cell_cases(v, form, opt, 13 * v + fi)
            cases.append(_many_tiles(v, "plain", opt, "uniform"))
    if opt == "fused_ws=0":
        # what the uniform kernels cannot carry: kNN-gathered sources and tile subsets (refused by plan and launch)
        cases.append(Case(B=2, rpb=256, segs=(33,), Cout=64, form="knn", tag="refused knn"))
        cases.append(Case(B=2, rpb=256, segs=(33,), Cout=64, tile_list=True, tag="refused tile_list"))
    if opt == "defaults":
        cases += _special_defaults()
    if opt in ("deep_chunks=0", "deep_ks=0"):
        cases += _deep_cases(opt)
    if opt in ("ws_xcd_order=0", "ws_xcd_order=2"):
        for fi, form in enumerate(FORMS):
            cases.append(Case(B=16, rpb=384, segs=(41,), Cout=64, form=form, ss=True, relu_col0=20, seed=fi,
                              tag=opt))
            cases.append(Case(B=5, rpb=1000 if form not in GATHERED else 1024 - 8, segs=(33,), Cout=128, form=form,
                              post=True, seed=fi + 9, tag=opt))
    if opt == "ws_narrow3=0":
        for fi, form in enumerate(FORMS):
            cases += _cell_cases(7, form, opt, 5 + fi)[:3]
        cases.append(_many_tiles(7, "plain", opt, "ws"))
    return cases


def advisor_case(Cout):
    """narrow_kc32=0, 384 rows per cloud (a 256-row tile + a half tile), ball-gathered source with gK = 32 and the
    per-query term through a permuting row map with oadd_div = 32: the half tile must add row oadd_rows[p / 32]."""
    return Case(B=3, rpb=384, segs=(24,), Cout=Cout, form="ball", K=32, oadd=True, odiv=32, oadd_rows=True,
                ss=True, post=True, relu_col0=Cout // 2, seed=384 + Cout, tag="advisor")


def _deep_cases(opt):
    c = []
    for tag, B, rpb, Cin, Cout in (("deep6", 16, 16, 130, 256), ("deep6", 4, 48, 200, 129),
                                   ("deep5", 16, 64, 96, 128), ("deep5", 8, 100, 129, 161),
                                   ("deep4", 8, 256, 80, 128), ("deep4", 4, 300, 160, 161)):
        for i, form in enumerate(("plain", "residual")):
            c.append(Case(B=B, rpb=rpb, segs=(Cin,) if form == "residual" else (Cin - 33, 33), Cout=Cout, form=form,
                          ss=True, post=bool(i), add=bool(i), oadd=not i, relu_col0=Cout // 3, seed=Cin + i,
                          tag="%s %s" % (opt, tag)))
    return c


def _special_defaults():
    c = _deep_cases("defaults")
    # thin kernel: <= 4 input channels, nothing applied on the way in, no statistics
    for i, (B, rpb, Cin, Cout, d) in enumerate(((2, 64, 3, 201, 1), (5, 1000, 3, 33, 1), (8, 16, 4, 129, 1),
                                                (1, 256, 3, 3, 8), (16, 2048, 3, 65, 1))):
        c.append(Case(B=B, rpb=rpb, segs=(Cin,), Cout=Cout, div=(d,), K=d, stats=False, ldy_extra=4 * (i % 2),
                      seed=i, tag="thin"))
    # scalar staging: an odd leading dimension on the first source
    for i, (B, rpb, segs, Cout) in enumerate(((3, 300, (17,), 33), (1, 128, (31, 2), 97), (5, 96, (45,), 129),
                                              (2, 40, (15,), 3), (8, 512, (40,), 64), (2, 256, (20,), 161))):
        c.append(Case(B=B, rpb=rpb, segs=segs, Cout=Cout, unaligned=True, form="residual" if i == 0 else "plain",
                      ss=True, pre=bool(i % 2), add=True, relu_col0=Cout // 2, seed=i, tag="scalar"))
    # walk_reverse and the tile subsets (128-row tiles) on the wave-specialised kernels
    for i, (form, Cout, rpb) in enumerate((("plain", 32, 2048 + 64), ("ball", 64, 1024 + 32), ("knn", 128, 512),
                                           ("residual", 96, 300), ("plain", 161, 256))):
        c.append(Case(B=5, rpb=rpb, segs=(33,), Cout=Cout, form=form, walk_reverse=1, ss=True, seed=i, tag="reverse"))
        if form in ("plain", "ball"):
            c.append(Case(B=5, rpb=rpb, segs=(33,), Cout=Cout, form=form, tile_list=True, ptpb_extra=2, ss=True,
                          oadd=True, relu_col0=16, seed=i, tag="tile_list"))
    # weighted statistics (per-query launches) and the row map on plain sources
    for i, (rpb, Cout) in enumerate(((256, 128), (16, 64), (2048, 32), (300, 161), (97, 33))):
        c.append(Case(B=3, rpb=rpb, segs=(40,), Cout=Cout, wrow0=True, wmul=32.0, ptpb_extra=1, oadd=True, K=1,
                      oadd_rows=True, relu_col0=Cout // 2, seed=i, tag="weighted"))
    # paired launches: a listed first problem (plain / ball-gathered) + a weighted second one
    for v, Cout in ((2, 96), (4, 128), (7, 32), (8, 64)):
        for form in ("plain", "ball"):
            c.append(Case(B=5, rpb=512 + 128 if form == "ball" else 512 + 100, segs=(40,), Cout=Cout, form=form, K=32,
                          tile_list=True, ptpb_extra=1, ss=True, relu_col0=Cout // 2, pair=True, seed=v,
                          tag="pair v%d" % v))
    return c


def random_cases(opt, n, seed=0):
    """A seeded stream of random cases that mixes the features (every option set gets its own stream)."""
    rng = np.random.default_rng(seed * 7919 + sum(map(ord, opt)))
    out = []
    for i in range(n):
        form = str(rng.choice(FORMS if not opt.startswith("fused_ws=0") else ("plain", "residual", "ball")))
        gathered = form in GATHERED
        K = int(rng.choice([4, 8, 16, 32]))
        rpb = int(rng.choice([1, 16, 33, 64, 96, 128, 129, 200, 256, 384, 1000, 2048, 3000]))
        if gathered or rng.integers(0, 2):
            rpb = max(K, (rpb + K - 1) // K * K)
        nseg = 1 if form in ("residual", "ball_res", "knn_res") else int(rng.integers(1, 5))
        segs = tuple(int(rng.choice([1, 3, 4, 15, 16, 17, 31, 33, 64, 100, 129])) for _ in range(nseg))
        Cout = int(rng.choice([3, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 200]))
        B = int(rng.choice([1, 2, 5, 8, 16]))
        while B * rpb * max(sum(segs), Cout) > (1 << 22):
            B = max(1, B // 2)
            if B == 1:
                break
        div = tuple(int(K if (rng.integers(0, 3) == 0 and rpb % K == 0 and K <= 32) else 1) for _ in segs)
        if gathered:
            div = (1,) + div[1:]
        odiv = int(rng.choice([1, 2, K, 32])) if rpb % 32 == 0 else 1
        has_oadd = bool(rng.integers(0, 2))
        f = dict(pre=bool(rng.integers(0, 2)), post=bool(rng.integers(0, 2)), ss=bool(rng.integers(0, 2)),
                 add=bool(rng.integers(0, 2)), oadd=has_oadd, odiv=odiv,
                 oadd_rows=has_oadd and bool(rng.integers(0, 2)), ldy_extra=int(rng.choice([0, 1, 4])),
                 relu_col0=int(rng.choice([0, 16, 32, 128, Cout])), ptpb_extra=int(rng.choice([-1, 0, 3])),
                 wrow0=bool(rng.integers(0, 4) == 0), wmul=float(rng.choice([1.0, 32.0])),
                 walk_reverse=int(rng.integers(0, 2)), unaligned=bool(rng.integers(0, 6) == 0) and not gathered,
                 bias=bool(rng.integers(0, 4)), stats=bool(rng.integers(0, 5)))
        out.append(Case(B=B, rpb=rpb, segs=segs, Cout=Cout, form=form, K=K, div=div, seed=10000 + i,
                        tag="%s random %d" % (opt, i), **f))
    return out


def corner_cases():
    """Malformed kNN marks, where the library's two readings of "kNN-form" differ (pdr::LayerSource, csrc/layer_tiles.h):
    the kernel form follows g_r1 alone, the plan's refusal and its out[3] follow g_r1 OR g_r2.  Plan-level only (fake
    addresses).  Each entry: (label, options, Layer, expected rc, expected (out[0], out[2], out[3]) or None) -- what
    the library returned before the dispatch had one source of truth, pinned so that it stays."""
    OK, EUNSUP = _lib.PDR_OK, _lib.PDR_EUNSUPPORTED
    row = 0x7000                                  # a fake (C,) row address

    def layer(form, **marks):
        L = build(Case(B=2, rpb=2048, segs=(64,), Cout=64, form=form, K=8), None)
        for k, v in marks.items():
            where, field = k.split("__")
            setattr(L.li.seg[0] if where == "seg" else L.li.rseg, field, v)
        return L

    out = []
    for ws in (1, 0):
        o = {} if ws else {"fused_ws": 0}
        t = "" if ws else " fused_ws=0"

        def add(label, L, rc_ws, cell):
            # without the wave-specialised kernels every marked call is refused
            out.append((label + t, o, L, rc_ws if ws else EUNSUP, cell if ws and rc_ws == OK else None))
        # g_r2 without g_r1: runs as the plain / ball form of the wave-specialised kernel; reported as kNN when gathered
        add("plain + seg g_r2", layer("plain", seg__g_r2=row), OK, (1, 0, 0))
        add("ball + seg g_r2", layer("ball", seg__g_r2=row), OK, (1, 0, 2))
        add("ball_res + rseg g_r2", layer("ball_res", rseg__g_r2=row), OK, (1, 1, 2))
        add("residual + seg g_r2", layer("residual", seg__g_r2=row), OK, (1, 1, 0))
        # g_r1 alone is a kNN form without its arrays: no instantiation
        add("plain + seg g_r1", layer("plain", seg__g_r1=row), EUNSUP, None)
        add("ball + seg g_r1", layer("ball", seg__g_r1=row), EUNSUP, None)
        add("ball_res + rseg g_r1", layer("ball_res", rseg__g_r1=row), EUNSUP, None)
        # a stale gathered residual descriptor (rseg.gV without rseg.ptr) still carries its marks
        add("plain + stale rseg gV g_r1", layer("plain", rseg__gV=row, rseg__g_r1=row), EUNSUP, None)
        add("plain + stale rseg gV g_r2", layer("plain", rseg__gV=row, rseg__g_r2=row), OK, (1, 0, 0))
    # an unmarked stale descriptor is ignored either way
    out.append(("plain + stale rseg gV fused_ws=0", {"fused_ws": 0}, layer("plain", rseg__gV=row), OK, (0, 0, 0)))
    return out


def cell_of(L, rc, out):
    """Dispatch cell a case reached (None when the plan refused it): ('ws' | 'uniform', variant, form), ('thin',),
    ('deep', 4 | 5 | 6), ('scalar',) -- plus ('pair', variant) for the first problem of a paired launch."""
    if rc != _lib.PDR_OK:
        return None
    c = L.case
    if out[6] and not c.stats and not c.tile_list:
        return ("thin",)
    if out[7]:
        return ("deep", out[1])
    if not out[4]:
        return ("scalar",)
    if c.pair:
        return ("pair", out[1]) if out[0] else None
    return ("ws" if out[0] else "uniform", out[1], c.form)
