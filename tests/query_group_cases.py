"""Cases, references and derived error bounds of pdr_query_group_cf / pdr_query_group_cf_grad.
(A helper module like tests/group_norm_act_cases.py, not a conftest and not a test file.)

FORWARD REFERENCE (never the kernel): `forward_reference`, the composition of QueryAndGroup.forward evaluated in numpy
fp32 -- gather, select, one subtraction, concatenate.  The kernel's output must be array_equal to it.

BACKWARD REFERENCE, PART ONE: `emulate_backward`, the chain stated in the header of csrc/query_group_cf.hip, run
sequentially with explicit fp32 adds in ascending order (numpy float32 arrays: every `+` and `-` below rounds once to
fp32).  The kernel's gradients must have its bits (`bits`: the uint32 view).  Inputs are finite and of normal range
(standard normal draws), so denormal handling cannot differ.

BACKWARD REFERENCE, PART TWO: `reference64`, float64 autograd of `composition` (the module's own torch expression,
have * a + none * c included) on the CPU, with per-element bounds derived from the chain.  u = 2^-24.
  A sequential fp32 sum of L addends x_1 .. x_L from +0 makes L - 1 rounding adds (0 + x_1 is exact); its error is at
  most g(L) sum|x_i| with g(L) = (L - 1) u / (1 - (L - 1) u), the first-order (L - 1) u sum|x_i| made rigorous.
  grad_features[b,c,j]: the addends are grad_out values, exact:            b = g(L) sum|g_f|
  grad_xyz[b,j,d]: the addends are a = fl(g_r + g_a), each off by u (|g_r| + |g_a|) when both slices exist (adding
    +0 is exact) and at most (1 + u)(|g_r| + |g_a|) large:                 b = sum e_a + g(L) (1 + u) sum(|g_r| + |g_a|)
  grad_new_xyz[b,q,d]: L = K addends t_k.  t0 = fl(g_c - g_r) is off by e_0 = u (|g_c| + |g_r|) when the centre slice
    exists (0 - g_r is exact).  Unpatched: t = t0, |t| <= M = (1 + u)(|g_c| + |g_r|), e_t = e_0.  Patched:
    t = fl(t0 + a): e_t = e_0 + e_a + u M, M = (1 + u)^2 (|g_c| + 2 |g_r| + |g_a|) (the exact value g_c + g_a is
    smaller; the bound follows the operations, not the result):            b = sum e_t + g(K) sum M
  Every bound is multiplied by 1 + 2^-24 for the float64 reference's own rounding ((L + 3) 2^-53 sum|.| against
  (L - 1) 2^-24 sum|.|).  Where no rounding happens (one source, no second slice) the bound is 0: the value is exact.
  Destinations no real slot names have L = 0 and bound 0 -- and must be +0.0f by bits, which part one checks.
`emulate_backward` itself must pass these bounds (tests/test_query_group_host.py checks it here, on the CPU).

INDEX PATTERNS are synthetic, never from a ball query, never outside [0, n): "ball" (c ascending indices, then the
first repeated; c from counts where given), "zero" (every slot names point 0), "random" (duplicates), "perm" (a
permutation, m K == n), "sparse" (only every third point is named: the others' gradient is exactly +0.0f).
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib

U = 2.0 ** -24
FLAGS = (0, 1, 3, 5, 7)            # features only | relative | + absolute | + centre | all: the five meaningful words
COUNTS = (None, "zero", "mixed", "positive")
PATTERNS = ("ball", "zero", "random", "sparse")

Case = namedtuple("Case", "B n m K C flags counts pattern offset")


def triples(flags):
    return 0 if not flags & 1 else 1 + bool(flags & 2) + bool(flags & 4)


def case_id(c):
    return "B%d-n%d-m%d-K%d-C%s-f%d-%s-%s%s" % (c.B, c.n, c.m, c.K, c.C, c.flags, c.counts or "nocounts", c.pattern,
                                                "-offset" if c.offset else "")


def _table():
    rows = []
    Bs, ns, ms, Cs = (1, 3), (1, 5, 70, 300), (1, 3, 17, 70), (None, 1, 7, 8, 9, 35)
    # (K, offset view): scalar by K, vector, vector, scalar by alignment, scalar by K, scalar by K, vector
    fams = ((3, False), (4, False), (32, False), (8, True), (33, False), (1, False), (64, False))
    # every (family, counts mode, flags) twice; the other dimensions cycle with strides that do not line up
    for i, (rep, flags, counts, (K, offset)) in enumerate((r, f, c, k) for r in range(2) for f in FLAGS for c in COUNTS
                                                          for k in fams):
        C = Cs[(i * 5 + i // 6) % 6]
        if flags == 0 and C is None:
            C = Cs[1 + i % 5]
        rows.append(Case(Bs[i % 2], ns[(i // 2 + i // 8) % 4], ms[(i // 3 + i // 12) % 4], K, C, flags, counts,
                         PATTERNS[(i + i // 4) % 4], offset))
    # m K above 256 and no multiple of it, in both families, every counts mode
    for j, counts in enumerate(COUNTS):
        rows.append(Case(3, 300, 17, 32, 35, 7, counts, PATTERNS[j], False))
        rows.append(Case(1, 70, 17, 33, 9, 3, counts, PATTERNS[3 - j], False))
    # a permutation: m K == n
    rows += [Case(3, 70, 70, 1, 8, 7, None, "perm", False), Case(1, 68, 17, 4, 7, 1, "mixed", "perm", False),
             Case(3, 300, 75, 4, None, 5, None, "perm", True)]
    # segment lengths around the builder's long-segment threshold (256): K = 1, every slot names point 0; a patched
    # variant whose slots contribute nothing, and a mixed one
    for m in (255, 256, 257):
        rows += [Case(1, 5, m, 1, 9, 3, None, "zero", False), Case(3, 5, m, 1, 1, 7, "positive", "zero", False),
                 Case(1, 5, m, 1, 9, 7, "zero", "zero", False), Case(3, 300, m, 1, 35, 1, "mixed", "zero", False)]
    # long segments in the vector family and next to short ones
    rows += [Case(3, 70, 70, 8, 35, 7, None, "zero", False), Case(1, 5, 70, 64, 7, 3, "mixed", "random", False)]
    return rows


CASES = _table()


def family(case):
    """1: the vector family runs (K % 4 == 0 and no offset view), 0: the scalar one."""
    return int(case.K % 4 == 0 and not case.offset)


def plan(n, m, K, C, flags, aligned16=1):
    """(rc, [family, grid.x, grid.y, feature slabs, output channels, E])."""
    out = (ctypes.c_int * 6)(-7, -7, -7, -7, -7, -7)
    rc = _lib.load().pdr_query_group_cf_plan(n, m, K, C, flags, aligned16, out)
    return rc, list(out)


def workspace_bytes(B, n, m, K):
    return _lib.load().pdr_query_group_cf_workspace_bytes(B, n, m, K)


Arrays = namedtuple("Arrays", "xyz new_xyz features idx counts grad_out")


def make(case):
    """Read-only fp32 / int32 host arrays of a case, seeded by the case."""
    B, n, m, K = case.B, case.n, case.m, case.K
    rng = np.random.default_rng([B, n, m, K, case.C or 0, case.flags, COUNTS.index(case.counts),
                                 (PATTERNS + ("perm",)).index(case.pattern), int(case.offset)])
    xyz = rng.standard_normal((B, n, 3)).astype(np.float32)
    new_xyz = rng.standard_normal((B, m, 3)).astype(np.float32)
    features = None if case.C is None else rng.standard_normal((B, case.C, n)).astype(np.float32)
    counts = None
    if case.counts == "zero":
        counts = np.zeros((B, m), np.int32)
    elif case.counts == "positive":
        counts = rng.integers(1, K + 1, (B, m)).astype(np.int32)
    elif case.counts == "mixed":
        counts = rng.integers(0, K + 1, (B, m)).astype(np.int32)
        counts[rng.random((B, m)) < 0.4] = 0
        counts.reshape(-1)[0] = 0                                   # at least one of each kind where m allows
        counts.reshape(-1)[-1] = max(1, int(counts.reshape(-1)[-1])) if B * m > 1 else 0
    if case.pattern == "zero":
        idx = np.zeros((B, m, K), np.int32)
    elif case.pattern == "random":
        idx = rng.integers(0, n, (B, m, K)).astype(np.int32)
    elif case.pattern == "sparse":
        idx = (3 * rng.integers(0, (n + 2) // 3, (B, m, K))).astype(np.int32)
    elif case.pattern == "perm":
        assert m * K == n
        idx = np.stack([rng.permutation(n) for _ in range(B)]).reshape(B, m, K).astype(np.int32)
    else:
        idx = np.zeros((B, m, K), np.int32)
        for b in range(B):
            for q in range(m):
                c = int(counts[b, q]) if counts is not None else int(rng.integers(1, K + 1))
                if c <= 0:
                    continue                                        # an empty ball: every slot names point 0
                hits = np.sort(rng.choice(n, c, replace=c > n))
                idx[b, q, :c] = hits
                idx[b, q, c:] = hits[0]
    assert idx.min() >= 0 and idx.max() < n
    ctot = (case.C or 0) + 3 * triples(case.flags)
    grad_out = rng.standard_normal((B, ctot, m, K)).astype(np.float32)
    out = Arrays(xyz, new_xyz, features, idx, counts, grad_out)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def _patched(A):
    B, m, K = A.idx.shape
    return np.zeros((B, m), bool) if A.counts is None else A.counts <= 0


def forward_reference(A, flags):
    """The composition in numpy fp32: gather, select, one subtraction; channels [features | relative | abs | centre]."""
    B, m, K = A.idx.shape
    ix = A.idx.astype(np.int64)
    pat = _patched(A)[:, None, :, None]                                         # (B, 1, m, 1)
    parts = []
    if A.features is not None:
        g = np.take_along_axis(A.features, ix.reshape(B, 1, m * K), axis=2).reshape(B, -1, m, K)
        parts.append(np.where(pat, np.float32(0.0), g))
    if flags & 1:
        centre = np.broadcast_to(A.new_xyz.transpose(0, 2, 1)[:, :, :, None], (B, 3, m, K))
        ab = np.take_along_axis(A.xyz.transpose(0, 2, 1), ix.reshape(B, 1, m * K), axis=2).reshape(B, 3, m, K)
        ab = np.where(pat, centre, ab)
        parts.append(ab - centre)
        if flags & 2:
            parts.append(ab)
        if flags & 4:
            parts.append(centre)
    out = np.concatenate(parts, axis=1).astype(np.float32)
    assert out.dtype == np.float32
    return out


def _slices(A, flags, channel_order_wrong=False):
    """(g_f (B,C,m,K) or None, g_r, g_a, g_c (B,3,m,K) or None) of grad_out."""
    C = 0 if A.features is None else A.features.shape[1]
    E = triples(flags)
    g = A.grad_out
    if channel_order_wrong and E and C:                     # a kernel that believes in [relative | features | ...]
        g = np.concatenate([g[:, 3:3 + C], g[:, :3], g[:, 3 + C:]], axis=1)
    gf = g[:, :C] if C else None
    gr = g[:, C:C + 3] if E else None
    ga = g[:, C + 3:C + 6] if E and flags & 2 else None
    gc = g[:, C + 3 * (E - 1):C + 3 * E] if E and flags & 4 else None
    return gf, gr, ga, gc


def _ordered_sum(values, idx, real, n, descending=False):
    """values (B, Cx, P) fp32, idx (B, P), real (B, P) bool -> (B, Cx, n): out[b, :, j] = the fp32 sum from +0.0f of
    values[b, :, p] over the real p with idx[b, p] == j, in ascending p.  Round r adds the r-th source of every
    destination at once: one explicit fp32 add per source, in order."""
    B, Cx, P = values.shape
    out = np.zeros((B, Cx, n), np.float32)
    for b in range(B):
        ps = np.nonzero(real[b])[0]
        if descending:
            ps = ps[::-1]
        ds = idx[b, ps].astype(np.int64)
        order = np.argsort(ds, kind="stable")
        ps, ds = ps[order], ds[order]
        first = np.searchsorted(ds, ds, side="left")
        rank = np.arange(ds.size) - first
        acc = out[b]
        for r in range(int(rank.max()) + 1 if ds.size else 0):
            sel = rank == r
            acc[:, ds[sel]] = acc[:, ds[sel]] + values[b][:, ps[sel]]          # float32 + float32: one rounding
    return out


VARIANTS = ("descending", "patched_included", "no_g_a", "centre_sign", "channel_order")


def emulate_backward(A, flags, variant=None):
    """Sequential fp32 emulation of the stated backward chain -> (grad_features or None, grad_xyz, grad_new_xyz).
    `variant`: one of VARIANTS, a plausible WRONG implementation (for the check that the references discriminate)."""
    assert variant is None or variant in VARIANTS
    B, m, K = A.idx.shape
    n = A.xyz.shape[1]
    P = m * K
    gf, gr, ga, gc = _slices(A, flags, variant == "channel_order")
    pat = _patched(A)
    real = np.broadcast_to(~pat[:, :, None], (B, m, K)).reshape(B, P)
    if variant == "patched_included":
        real = np.ones((B, P), bool)
    idx = A.idx.reshape(B, P)
    desc = variant == "descending"
    zero = np.zeros((B, 3, m, K), np.float32)
    grad_f = None if gf is None else _ordered_sum(np.ascontiguousarray(gf).reshape(B, -1, P), idx, real, n, desc)
    if gr is None:
        return grad_f, np.zeros((B, n, 3), np.float32), np.zeros((B, m, 3), np.float32)
    a = gr + (zero if ga is None or variant == "no_g_a" else ga)                # fl(g_r + g_a)
    grad_x = _ordered_sum(np.ascontiguousarray(a).reshape(B, 3, P), idx, real, n, desc).transpose(0, 2, 1)
    t = (zero if gc is None else gc) - gr                                        # fl(g_c - g_r)
    if variant == "centre_sign":
        t = gr - (zero if gc is None else gc)
    t = np.where(pat[:, None, :, None], t + a, t)                                # patched: fl(t + a)
    acc = np.zeros((B, 3, m), np.float32)
    for k in (range(K - 1, -1, -1) if desc else range(K)):
        acc = acc + t[..., k]
    assert a.dtype == t.dtype == acc.dtype == np.float32
    return grad_f, np.ascontiguousarray(grad_x), np.ascontiguousarray(acc.transpose(0, 2, 1))


def composition(xyz, new_xyz, features, idx, counts, flags):
    """QueryAndGroup.forward after the neighbour search, as the module writes it, in the dtype of its inputs."""
    B, m, K = idx.shape
    flat = idx.long().reshape(B, 1, m * K)
    group = lambda t: t.gather(2, flat.expand(-1, t.shape[1], -1)).reshape(B, t.shape[1], m, K)
    have = none = None
    if counts is not None:
        have = (counts > 0).to(xyz.dtype).unsqueeze(1).unsqueeze(-1)
        none = 1 - have
    parts = []
    if features is not None:
        grouped = group(features)
        if have is not None:
            grouped = have * grouped + none * torch.zeros(features.shape[1], dtype=xyz.dtype).view(1, -1, 1, 1)
        parts.append(grouped)
    if flags & 1:
        centre = new_xyz.transpose(1, 2).unsqueeze(-1)
        ab = group(xyz.transpose(1, 2).contiguous())
        if have is not None:
            ab = have * ab + none * centre
        parts.append(ab - centre)
        if flags & 2:
            parts.append(ab)
        if flags & 4:
            parts.append(centre.expand(-1, -1, -1, K))
    return torch.cat(parts, dim=1)


def _gamma(L):
    L = np.asarray(L, np.float64)
    k = np.maximum(L - 1, 0) * U
    return k / (1 - k)


def reference64(A, flags):
    """float64 autograd of `composition` on the CPU and the bounds of the module docstring: a dict of read-only
    float64 arrays gf (None without features), gx, gn and b_gf, b_gx, b_gn."""
    B, m, K = A.idx.shape
    n = A.xyz.shape[1]
    P = m * K
    leaf = lambda a: None if a is None else torch.tensor(a).double().requires_grad_()
    xyz, new_xyz, feat = leaf(A.xyz), leaf(A.new_xyz), leaf(A.features)
    cnt = None if A.counts is None else torch.tensor(A.counts)
    out = composition(xyz, new_xyz, feat, torch.tensor(A.idx), cnt, flags)
    wrt = [t for t in (feat, xyz, new_xyz) if t is not None]
    grads = list(torch.autograd.grad(out, wrt, torch.tensor(A.grad_out).double(), allow_unused=True))
    grads = [torch.zeros_like(w) if g is None else g for g, w in zip(grads, wrt)]
    gf = grads.pop(0).numpy() if feat is not None else None
    gx, gn = grads[0].numpy(), grads[1].numpy()

    absg = lambda s: np.zeros((B, 3, m, K)) if s is None else np.abs(s.astype(np.float64))
    f, r, a_, c = _slices(A, flags)
    pat = _patched(A)
    real = np.broadcast_to(~pat[:, :, None], (B, m, K)).reshape(B, P)
    idx = A.idx.reshape(B, P).astype(np.int64)

    def scatter(v):                                                              # (B, Cx, P) -> (B, Cx, n), real slots only
        o = np.zeros((B, v.shape[1], n))
        for b in range(B):
            np.add.at(o[b], (slice(None), idx[b][real[b]]), v[b][:, real[b]])
        return o
    L = scatter(np.ones((B, 1, P)))                                              # (B, 1, n) sources per destination
    slack = 1 + 2.0 ** -24
    b_gf = None if f is None else _gamma(L) * scatter(np.abs(f.astype(np.float64)).reshape(B, -1, P)) * slack
    mag_a = absg(r) + absg(a_)
    e_a = U * mag_a if (r is not None and a_ is not None) else np.zeros_like(mag_a)
    b_gx = (scatter(e_a.reshape(B, 3, P)) + _gamma(L) * (1 + U) * scatter(mag_a.reshape(B, 3, P))) * slack
    e_0 = U * (absg(c) + absg(r)) if (c is not None and r is not None) else np.zeros((B, 3, m, K))
    M_un, M_pa = (1 + U) * (absg(c) + absg(r)), (1 + U) ** 2 * (absg(c) + 2 * absg(r) + absg(a_))
    p4 = pat[:, None, :, None]
    e_t, M = np.where(p4, e_0 + e_a + U * M_pa, e_0), np.where(p4, M_pa, M_un)
    b_gn = (e_t.sum(-1) + _gamma(K) * M.sum(-1)) * slack                         # (B, 3, m)
    res = dict(gf=gf, gx=gx, gn=gn, b_gf=b_gf, b_gx=b_gx.transpose(0, 2, 1), b_gn=b_gn.transpose(0, 2, 1))
    for v in res.values():
        if v is not None:
            v.setflags(write=False)
    return res


OUTPUTS = ("gf", "gx", "gn")


def worst_ratio(got, ref):
    """{name: max |got - reference| / bound} over the gradients in `got` (a dict; None entries skipped); an error at a
    zero bound or a non-finite value gives inf."""
    out = {}
    for name in OUTPUTS:
        if got.get(name) is None or ref[name] is None:
            continue
        have = np.asarray(got[name], dtype=np.float64).reshape(ref[name].shape)
        err, bound = np.abs(have - ref[name]), ref["b_" + name]
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        ratio = np.where(np.isfinite(have), ratio, np.inf)
        out[name] = float(ratio.max()) if ratio.size else 0.0
    return out


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


_CACHE = {}


def references(case):
    """(arrays, forward reference, emulated gradients, float64 reference) of a case, computed once, read-only."""
    if case not in _CACHE:
        A = make(case)
        fwd = forward_reference(A, case.flags)
        emu = dict(zip(OUTPUTS, emulate_backward(A, case.flags)))
        for a in [fwd] + list(emu.values()):
            if a is not None:
                a.setflags(write=False)
        _CACHE[case] = (A, fwd, emu, reference64(A, case.flags))
    return _CACHE[case]
