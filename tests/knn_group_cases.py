"""Cases, references and derived error bounds of pdr_knn_group_cf / pdr_knn_group_cf_grad.
(A helper module like tests/query_group_cases.py, not a conftest and not a test file.)

FORWARD REFERENCE (never the kernel): `forward_reference`, numpy fp32 -- copies, one subtraction, and the weight chain
r_k = fl(1 / fl(d_k + 1e-8f)), S = r_0 + .. + r_{K-1} ascending from +0, w_k = fl(r_k / S).  The kernel's output must be
array_equal to it and have its bits.

BACKWARD REFERENCE, PART ONE: `emulate_backward`, the chain stated in the header of csrc/knn_group_cf.hip, run
sequentially with explicit fp32 operations in ascending order (numpy float32 arrays: every `+ - * /` rounds once to
fp32).  The kernel's gradients must have its bits.  Inputs are finite and of normal range.

BACKWARD REFERENCE, PART TWO: `reference64`, float64 autograd on the CPU of group_knn's torch expression (`composition`)
with d2 recomputed differentiably as |x - y[idx]|^2, with per-element bounds derived from the chain.  u = 2^-24.  Every
intermediate of the chain is followed as a pair (v, E): v its value in float64 arithmetic, E a bound on |fp32 - v|.
  inputs: x, y and grad_out are fp32 numbers, E = 0.  d: v = |x - y[idx]|^2 in float64, E = |dists - v| (`dists` is
    data handed to the op -- the fp32 distance of the search --, so its distance from v is known exactly).
    1e-8f: v = 1e-8, E = |float32(1e-8) - 1e-8|.
  fl(a +- b): (va +- vb, Ea + Eb), then the rounding.   fl(a b): (va vb, |va| Eb + |vb| Ea + Ea Eb), then the rounding.
  fl(a / b): q = va / vb, (q, (Ea + |q| Eb) / (|vb| - Eb)), then the rounding.   2 G is exact: (2 v, 2 E).
  the rounding of an operation with exact result v and accumulated bound E adds u (|v| + E).
  a sequential sum of L addends (v_i, E_i) from +0 makes L - 1 rounding adds (0 + x_1 is exact):
    (sum v_i, sum E_i + g(L) sum(|v_i| + E_i)),  g(L) = (L - 1) u / (1 - (L - 1) u).
  The chain: s = d + 1e-8, r = 1 / s, S = sum_k r, w = r / S, dot = sum_k fl(g_w w), h = fl(g_w - dot) / S,
  G = g_d - fl(fl(r r) h), e = x - y[idx], t = fl(2 G) e;  grad_x = sum_k fl(fl(g_c - g_r) + t);  grad_y[j] = the
  ordered sum over the slots naming j of fl(fl(g_a + g_r) - t);  grad_features[c,j] = the ordered sum of g_f (exact
  addends: b = g(L) sum|g_f|).  At a slot with d = 0 (a query that coincides with its neighbour) G is ill-conditioned
  -- r r is 1e16 -- but e is exactly 0 there with E = 0, so t = 0 with E = 0: the OUTPUTS are bounded, not G.
  Every bound is multiplied by 1 + 2^-24 for the float64 reference's own rounding.  Destinations no slot names have
  L = 0 and bound 0 -- and must be +0.0f by bits, which part one checks.
Because derived worst-case bounds can be loose, a NORM-WISE CAP stands beside them: for each gradient tensor of each
case, max|got - reference64| / max|reference64| <= CAP = 1e-5.  Its basis, numpy on the CPU: the stated chain for
grad_x measured 6.1e-8 to 6.4e-7 over B = 2, n1 70 / 300, n2 40 / 70 / 300, K 1 / 3 / 8 / 16, independent and
coincident draws and coordinates scaled by 0.05, while a dropped or mis-signed term is of order 1e-1;
tests/test_knn_group_cf_host.py establishes grad_y and grad_features on every row of the table (its printed worst
figures for the emulation: grad_features 2.7e-6 -- the 257-addend sums --, grad_x 2.8e-7, grad_y 1.6e-6) and on a
sample of rows drawn again with `make(case, scale=0.05)` (1.1e-6, 1.7e-6, 1.5e-6).
`emulate_backward` itself must pass the bounds and the cap (tests/test_knn_group_cf_host.py checks it, on the CPU).

INDEX PATTERNS: "knn" (a real top-K, K <= n2, of independently drawn standard-normal x and y, computed here in numpy;
dists the fp32 squared distance, ascending, ties by index), "coincident" (the same, but every second query is a row of
y: d2 == 0 exactly for its first neighbour -- the network's own situation, upsampled levels contain their parents),
"zero" (every slot names point 0) and "random" (duplicates; any K), the last two with dists computed from idx.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib
from tests.query_group_cases import U, _gamma, _ordered_sum, bits  # noqa: F401  (bits is re-exported)

GEO = 11
CAP = 1e-5
EPS32 = np.float32(1e-8)
PATTERNS = ("knn", "coincident", "zero", "random")

Case = namedtuple("Case", "B n1 n2 K C pattern offset")


def case_id(c):
    return "B%d-n1_%d-n2_%d-K%d-C%s-%s%s" % (c.B, c.n1, c.n2, c.K, c.C, c.pattern, "-offset" if c.offset else "")


def _table():
    rows = []
    Bs, n1s, n2s, Cs = (1, 3), (1, 3, 17, 70, 257), (1, 5, 70, 300), (None, 1, 7, 8, 9, 35)
    # (K, offset view): scalar by K, vector, vector, scalar by alignment, scalar by K, vector, scalar by alignment (twice)
    fams = ((3, False), (4, False), (8, False), (8, True), (1, False), (16, False), (16, True), (4, True))
    # every (family, pattern) four times; the other dimensions cycle with strides that do not line up
    for i, (rep, pattern, (K, offset)) in enumerate((r, p, k) for r in range(4) for p in PATTERNS for k in fams):
        j = (i // 2 + i // 7) % 4
        if pattern in ("knn", "coincident"):                 # a real top-K needs K <= n2
            while n2s[j] < K:
                j = (j + 1) % 4
        rows.append(Case(Bs[i % 2], n1s[(i // 3 + i // 11) % 5], n2s[j], K, Cs[(i * 5 + i // 6) % 6], pattern, offset))
    # n1 K above 256 and no multiple of it, in both families, every pattern
    for p in PATTERNS:
        rows.append(Case(3, 70, 300, 8, 35, p, False))
        rows.append(Case(1, 257, 70, 3, 9, p, False))
        rows.append(Case(1, 70, 70, 4, 7, p, True))
    # segment lengths around the builder's long-segment threshold (256): one point, one neighbour
    for n1 in (255, 256, 257):
        rows += [Case(1, n1, 1, 1, 9, "zero", False), Case(3, n1, 1, 1, None, "knn", False),
                 Case(1, n1, 1, 1, 35, "coincident", False)]
    # long segments in the vector family and next to short ones
    rows += [Case(3, 70, 5, 8, 35, "zero", False), Case(1, 257, 5, 4, 7, "random", False),
             Case(1, 257, 5, 4, 8, "knn", True)]
    # most points of y named by no slot: their gradient is exactly +0.0f
    rows += [Case(3, 3, 300, 1, 7, "knn", False), Case(1, 3, 300, 4, 9, "coincident", False),
             Case(3, 1, 300, 16, 35, "knn", False), Case(1, 17, 300, 3, None, "random", False),
             Case(3, 1, 70, 8, 1, "coincident", True)]
    return list(dict.fromkeys(rows))                         # a required row the cycle already produced stays once


CASES = _table()


def family(case):
    """1: the vector family runs (K % 4 == 0 and no offset view), 0: the scalar one."""
    return int(case.K % 4 == 0 and not case.offset)


def plan(n1, n2, K, C, aligned16=1):
    """(rc, [family, grid.x, grid.y, feature slabs, output channels])."""
    out = (ctypes.c_int * 5)(-7, -7, -7, -7, -7)
    rc = _lib.load().pdr_knn_group_cf_plan(n1, n2, K, C, aligned16, out)
    return rc, list(out)


def workspace_bytes(B, n1, n2, K):
    return _lib.load().pdr_knn_group_cf_workspace_bytes(B, n1, n2, K)


Arrays = namedtuple("Arrays", "x y features idx dists grad_out")


def sq_dist32(x, y_at):
    """fp32 squared distance of x (..., 3) and y_at (..., 3), each operation rounded: (dx dx + dy dy) + dz dz."""
    d = (x - y_at).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def gather_rows(y, idx):
    """y (B, n2, 3), idx (B, n1, K) -> (B, n1, K, 3)."""
    B, n1, K = idx.shape
    return np.take_along_axis(y, idx.reshape(B, n1 * K, 1).astype(np.int64), axis=1).reshape(B, n1, K, 3)


def make(case, scale=1.0):
    """Read-only fp32 / int32 host arrays of a case, seeded by the case."""
    B, n1, n2, K = case.B, case.n1, case.n2, case.K
    rng = np.random.default_rng([B, n1, n2, K, case.C or 0, PATTERNS.index(case.pattern), int(case.offset)])
    x = (scale * rng.standard_normal((B, n1, 3))).astype(np.float32)
    y = (scale * rng.standard_normal((B, n2, 3))).astype(np.float32)
    features = None if case.C is None else rng.standard_normal((B, case.C, n2)).astype(np.float32)
    if case.pattern == "coincident":
        x[:, ::2] = y[:, np.arange(0, n1, 2) % n2]
    if case.pattern in ("knn", "coincident"):
        assert K <= n2
        d_all = sq_dist32(x[:, :, None, :], y[:, None, :, :])                    # (B, n1, n2)
        idx = np.argsort(d_all, axis=2, kind="stable")[:, :, :K].astype(np.int32)
    elif case.pattern == "zero":
        idx = np.zeros((B, n1, K), np.int32)
    else:
        idx = rng.integers(0, n2, (B, n1, K)).astype(np.int32)
    dists = sq_dist32(x[:, :, None, :], gather_rows(y, idx)).astype(np.float32)
    if case.pattern == "coincident":
        assert not dists[:, ::2, 0].any()
    assert idx.min() >= 0 and idx.max() < n2 and dists.dtype == np.float32
    grad_out = rng.standard_normal((B, (case.C or 0) + GEO, n1, K)).astype(np.float32)
    out = Arrays(x, y, features, idx, dists, grad_out)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def weights32(dists, from_distance=False):
    """(r, S, w) of the stated chain in fp32; dists (B, n1, K)."""
    d = np.sqrt(dists) if from_distance else dists
    r = np.float32(1.0) / (d + EPS32)
    S = np.zeros(dists.shape[:2], np.float32)
    for k in range(dists.shape[2]):
        S = S + r[..., k]
    w = r / S[..., None]
    assert r.dtype == S.dtype == w.dtype == np.float32
    return r, S, w


def forward_reference(A, variant=None):
    """numpy fp32: channels [features | d2 | w | nn_abs | nn_rel | x], (B, C + 11, n1, K)."""
    B, n1, K = A.idx.shape
    parts = []
    if A.features is not None:
        ix = A.idx.astype(np.int64).reshape(B, 1, n1 * K)
        parts.append(np.take_along_axis(A.features, ix, axis=2).reshape(B, -1, n1, K))
    w = weights32(A.dists, variant == "w_from_distance")[2]
    ab = gather_rows(A.y, A.idx).transpose(0, 3, 1, 2)                           # (B, 3, n1, K)
    xr = np.broadcast_to(A.x.transpose(0, 2, 1)[:, :, :, None], (B, 3, n1, K))
    parts += [A.dists[:, None], w[:, None], ab, ab - xr, xr]
    out = np.concatenate(parts, axis=1)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def _slices(A):
    """(g_f (B,C,n1,K) or None, g_d, g_w (B,n1,K), g_a, g_r, g_c (B,3,n1,K)) of grad_out."""
    C = 0 if A.features is None else A.features.shape[1]
    g = A.grad_out
    return (g[:, :C] if C else None, g[:, C], g[:, C + 1], g[:, C + 2:C + 5], g[:, C + 5:C + 8], g[:, C + 8:C + 11])


VARIANTS = ("w_from_distance", "no_dot", "y_sign", "no_g_r_in_x", "descending", "no_weight_path")


def emulate_backward(A, variant=None):
    """Sequential fp32 emulation of the stated backward chain -> (grad_features or None, grad_x, grad_y).
    `variant`: one of VARIANTS, a plausible WRONG implementation (for the check that the references discriminate)."""
    assert variant is None or variant in VARIANTS
    B, n1, K = A.idx.shape
    n2 = A.y.shape[1]
    P = n1 * K
    gf, gd, gw, ga, gr, gc = _slices(A)
    desc = variant == "descending"
    ks = range(K - 1, -1, -1) if desc else range(K)
    r, S, w = weights32(A.dists, variant == "w_from_distance")
    dot = np.zeros((B, n1), np.float32)
    for k in ks:
        dot = dot + gw[..., k] * w[..., k]
    if variant == "no_dot":
        dot = np.zeros((B, n1), np.float32)
    h = (gw - dot[..., None]) / S[..., None]
    G = gd - (r * r) * h
    if variant == "no_weight_path":                          # the gradient through w forgotten: G = g_d
        G = gd + np.float32(0.0)
    e = (A.x[:, :, None, :] - gather_rows(A.y, A.idx)).transpose(0, 3, 1, 2)     # (B, 3, n1, K): fl(x - y[idx])
    t = (np.float32(2.0) * G)[:, None] * e
    vx = (gc - (np.zeros_like(gr) if variant == "no_g_r_in_x" else gr)) + t
    acc = np.zeros((B, 3, n1), np.float32)
    for k in ks:
        acc = acc + vx[..., k]
    vy = (ga + gr) + t if variant == "y_sign" else (ga + gr) - t
    assert h.dtype == G.dtype == e.dtype == t.dtype == vx.dtype == vy.dtype == acc.dtype == np.float32
    idx = A.idx.reshape(B, P)
    real = np.ones((B, P), bool)
    grad_f = None if gf is None else _ordered_sum(np.ascontiguousarray(gf).reshape(B, -1, P), idx, real, n2, desc)
    grad_y = _ordered_sum(np.ascontiguousarray(vy).reshape(B, 3, P), idx, real, n2, desc).transpose(0, 2, 1)
    return grad_f, np.ascontiguousarray(acc.transpose(0, 2, 1)), np.ascontiguousarray(grad_y)


def composition(x, y, features, idx, dists=None):
    """group_knn(..., transpose=True) after the search, as the function writes it, in the dtype of its inputs; d2 is
    |x - y[idx]|^2, differentiable (what knn_points' backward differentiates), unless `dists` is given."""
    B, n1, K = idx.shape
    flat = idx.long().reshape(B, n1 * K, 1)
    nn_abs = y.gather(1, flat.expand(-1, -1, 3)).reshape(B, n1, K, 3)
    x_rep = x.unsqueeze(2).repeat(1, 1, K, 1)
    nn_rel = nn_abs - x_rep
    d2 = ((x_rep - nn_abs) ** 2).sum(-1) if dists is None else dists
    d2 = d2.unsqueeze(3)
    recip = 1.0 / (d2 + 1e-8)
    weight = recip / torch.sum(recip, dim=2, keepdim=True)
    parts = [d2, weight, nn_abs, nn_rel, x_rep]
    if features is not None:
        feats_y = features.transpose(1, 2)
        parts.insert(0, feats_y.gather(1, flat.expand(-1, -1, feats_y.shape[2])).reshape(B, n1, K, -1))
    return torch.cat(parts, dim=3).transpose(2, 3).transpose(1, 2)


# ---- (value, bound) pairs of the module docstring ---------------------------------------------------------------------
def _rnd(v, e):
    return v, e + U * (np.abs(v) + e)


def _add(a, b):
    return _rnd(a[0] + b[0], a[1] + b[1])


def _sub(a, b):
    return _rnd(a[0] - b[0], a[1] + b[1])


def _mul(a, b):
    return _rnd(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])


def _div(a, b):
    q = a[0] / b[0]
    return _rnd(q, (a[1] + np.abs(q) * b[1]) / (np.abs(b[0]) - b[1]))


def _ksum(a):
    """sequential sum over the last axis (K addends)."""
    K = a[0].shape[-1]
    return a[0].sum(-1), a[1].sum(-1) + _gamma(K) * (np.abs(a[0]) + a[1]).sum(-1)


def reference64(A):
    """float64 autograd of `composition` on the CPU and the bounds of the module docstring: a dict of read-only
    float64 arrays gf (None without features), gx, gy and b_gf, b_gx, b_gy."""
    B, n1, K = A.idx.shape
    n2 = A.y.shape[1]
    P = n1 * K
    leaf = lambda a: None if a is None else torch.tensor(a).double().requires_grad_()
    x, y, feat = leaf(A.x), leaf(A.y), leaf(A.features)
    out = composition(x, y, feat, torch.tensor(A.idx))
    wrt = [t for t in (feat, x, y) if t is not None]
    grads = list(torch.autograd.grad(out, wrt, torch.tensor(A.grad_out).double(), allow_unused=True))
    grads = [torch.zeros_like(w) if g is None else g for g, w in zip(grads, wrt)]
    gf = grads.pop(0).numpy() if feat is not None else None
    gx, gy = grads[0].numpy(), grads[1].numpy()

    f64 = lambda a: (np.asarray(a, np.float64), 0.0)
    f, g_d, g_w, g_a, g_r, g_c = _slices(A)
    X, Yg = A.x.astype(np.float64)[:, :, None, :], gather_rows(A.y, A.idx).astype(np.float64)
    dv = ((X - Yg) ** 2).sum(-1)                                                  # (B, n1, K)
    d = (dv, np.abs(A.dists.astype(np.float64) - dv))
    r = _div((np.ones_like(dv), 0.0), _add(d, (np.float64(1e-8), abs(float(EPS32) - 1e-8))))
    S = _ksum(r)
    S = (S[0][..., None], S[1][..., None])
    w = _div(r, S)
    dot = _ksum(_mul(f64(g_w), w))
    h = _div(_sub(f64(g_w), (dot[0][..., None], dot[1][..., None])), S)
    G = _sub(f64(g_d), _mul(_mul(r, r), h))
    e = _rnd((X - Yg).transpose(0, 3, 1, 2), 0.0)                                 # (B, 3, n1, K)
    t = _mul((2 * G[0][:, None], 2 * G[1][:, None]), e)
    vx = _add(_sub(f64(g_c), f64(g_r)), t)
    b_gx = _ksum(vx)[1]                                                           # (B, 3, n1)
    vy = _sub(_add(f64(g_a), f64(g_r)), t)
    idx = A.idx.reshape(B, P).astype(np.int64)

    def scatter(v):                                                               # (B, Cx, P) -> (B, Cx, n2)
        o = np.zeros((B, v.shape[1], n2))
        for b in range(B):
            np.add.at(o[b], (slice(None), idx[b]), v[b])
        return o
    L = scatter(np.ones((B, 1, P)))                                               # (B, 1, n2) sources per destination
    slack = 1 + 2.0 ** -24
    b_gf = None if f is None else _gamma(L) * scatter(np.abs(f.astype(np.float64)).reshape(B, -1, P)) * slack
    b_gy = scatter(vy[1].reshape(B, 3, P)) + _gamma(L) * scatter((np.abs(vy[0]) + vy[1]).reshape(B, 3, P))
    res = dict(gf=gf, gx=gx, gy=gy, b_gf=b_gf, b_gx=b_gx.transpose(0, 2, 1) * slack, b_gy=b_gy.transpose(0, 2, 1) * slack)
    for k in res:
        if res[k] is not None:
            res[k] = np.ascontiguousarray(res[k])
            res[k].setflags(write=False)
    return res


OUTPUTS = ("gf", "gx", "gy")


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


def norm_error(got, ref):
    """{name: max |got - reference| / max |reference|}: what CAP bounds (a reference that is zero everywhere -- it
    never is in the table -- asks for an exact zero)."""
    out = {}
    for name in OUTPUTS:
        if got.get(name) is None or ref[name] is None:
            continue
        have = np.asarray(got[name], dtype=np.float64).reshape(ref[name].shape)
        err, top = float(np.abs(have - ref[name]).max()), float(np.abs(ref[name]).max())
        out[name] = err / top if top > 0 else (0.0 if err == 0 else float("inf"))
        if not np.isfinite(have).all():
            out[name] = float("inf")
    return out


_CACHE = {}


def references(case):
    """(arrays, forward reference, emulated gradients, float64 reference) of a case, computed once, read-only."""
    if case not in _CACHE:
        A = make(case)
        fwd = forward_reference(A)
        emu = dict(zip(OUTPUTS, emulate_backward(A)))
        for a in [fwd] + list(emu.values()):
            if a is not None:
                a.setflags(write=False)
        _CACHE[case] = (A, fwd, emu, reference64(A))
    return _CACHE[case]
