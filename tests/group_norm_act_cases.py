"""Cases, float64 reference and derived error bounds of pdr_group_norm_act / pdr_group_norm_act_grad.
(A helper module like tests/attention_pool_cf_cases.py, not a conftest.)

REFERENCE (never the kernel): `composition`, act(MyGroupNorm(x)) written out with torch.nn.functional.group_norm, the
slice and cat, relu and x * sigmoid(x), evaluated in float64 on the CPU from the fp32 inputs; gradients from float64
autograd of it.  F.group_norm is called as torch.group_norm, the operator behind it: F.group_norm's own size guard
refuses one value per channel, the (1, 32, 1) case here.  eps is EPS = float32(1e-5) on both sides (the C call takes
a float).

BOUNDS, derived from the operation chain in the header of csrc/group_norm_act.hip.  u = 2^-24 (fp32), v = 2^-53
(double).  For one slab of m elements: mean, var (biased), rstd = 1 / sqrt(var + eps), A1 = E|x|, A2 = E[x^2], all
float64; for one element xh = (x - mean) rstd, z = xh gamma + beta (gamma = 1, beta = 0 without affine parameters).

  mean:   b_mean = u |mean| + v (m + 1) A1
    a double sum of m terms in ANY order is within (m - 1) v sum|x|, the division adds v; the rounding to fp32 u |mean|.
  rstd:   rel = u + v (3 m + 4) A2 / (2 (var + eps)) + 4 v,      b_rstd = rstd rel
    var_d = s2 / m - mean_d^2:  (m + 1) v A2 for s2 / m,  2 |mean| m v A1 + v mean^2 for the square,  v max(..) for the
    difference; with |mean| A1 <= A2 and mean^2 <= A2 that is v (3 m + 4) A2 on var + eps, half of it (relative) on
    rstd; the clamp at 0 only moves var_d towards the truth.  4 v: the sum with eps, square root, division, slack.
    u: the rounding of rstd to fp32.
  xh:     b_xh = rstd b_mean (1 + 4 u) + |xh| (3 u + rel)
    d = fl(x - mean^) is off by b_mean + u |x - mean|, times rstd; the product with rstd^ adds (rel + u) |xh|; the
    third u and the factor 1 + 4 u are slack for the second-order terms.  The first term holds the
    u |mean| rstd of the fp32-rounded saved mean, the dominant term when |mean| >> std.
  z:      b_z = |gamma| b_xh (1 + u) + u |z|            one fused multiply-add.  Pass-through channel: z = x, b_z = 0.
  y:      none, relu: b_y = b_z (both 1-Lipschitz; the ReLU mask is decided, see below).
          swish:  b_y = 1.1 b_z + |y| ((1 - s) de + 4 u) + 2^-120,     de = expm1(2 u |z|) + 2 u,   s = sigmoid(z)
    |d/dz z s(z)| < 1.1.  t = fl(z fl(-log2 e)) moves the exponent by 2 u |z| (natural units), v_exp_f32 is good to
    1 ulp = 2 u: e is within de, relatively.  s = 1 / (1 + e) moves by e / (1 + e) = (1 - s) of that, plus u for the
    sum and u for the division; fl(z s) one more; the fourth u is slack.  2^-120 covers a flushed or overflowed e.
  dz:     none, relu: b_dz = 0 -- dz is dy or +0 exactly.
          swish:  es = (1 - s) de + 2 u   (relative error of s^),   a = s (1 + z (1 - s)) = act'(z),
                  b_dz = |dy| (0.5 b_z + s (|z| (s es + 2 u (1 - s)) + u |1 + z (1 - s)|) + (es + 2 u) |a| + u s)
                         + u |dz|
    |act''| <= 0.5 carries b_z.  q = fl(1 - s^) is off by s es + u (1 - s); p = fl(z q) by |z| times that plus
    u |z| (1 - s); w = fl(1 + p) by that plus u |1 + p|; fl(s^ w) by s times that plus (es + u) |a|; one more u |a| and
    u s of slack; the product with dy adds u |dz|.
  row and slab sums (products and sums in double: v terms only):
      e_r1[b, c] = sum_s (b_dz |xh| + |dz| b_xh + b_dz b_xh) + v (S + 2) sum_s |dz xh|
      e_r2[b, c] = sum_s b_dz + v (S + 2) sum_s |dz|
      e_c1 = sum_c |gamma| e_r1 + v (Cg + 2) sum_c |gamma r1|,     e_c2 likewise      (over the slab's Cg rows)
      e_k1 = e_c1 / m + (u + v) |c1 / m|,                          e_k2 likewise      (k = float(c / m))
  grad_gamma:  b = sum_b e_r1 (1 + u) + (u + v (B + 2)) sum_b |r1| + 2^-149;      grad_beta likewise with r2.
  grad_x (normalised channel), dx = rstd w, w = gamma dz - (xh k1 + k2):
      e_t  = |gamma| b_dz + u |gamma dz|                                    fl(gamma dz^)
      e_t2 = b_xh (|k1| + e_k1) + |xh| e_k1 + e_k2 + u (|xh k1 + k2| + the three terms before)     the fma
      e_w  = (e_t + e_t2) (1 + u) + u |w|                                   the difference
      b_dx = rstd e_w (1 + rel + 2 u) + |dx| (rel + 2 u) + 2^-149           the product with rstd^, one u of slack
  grad_x (pass-through channel): b_dx = b_dz.

RELU MASK SAFETY.  A gradient check means nothing where the sign of z is undecided, so `make` leaves no element with
|z64| < 1e-3 (and `reference` asserts b_z < |z64| there, so the kernel's z has the reference's sign): it moves such
an element's x away (pass-through: to +-2e-3; normalised: by 4e-3 / (rstd |gamma|) in the direction that grows |z|),
repeats, and asserts that none is left.  Where a slab has variance exactly 0 (the "constant" pattern, one-element slabs)
no x can move z = beta: there beta is kept at least 2e-3 from zero and the kernel's z is beta exactly (the fp32 mean
of m copies of x is x, so d = 0 and fma(0, gamma, beta) = beta), and WITHOUT affine parameters z is exactly +-0 on
both sides (asserted on the reference), which decides the mask too: off.  No element is excluded
from any comparison.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from point_diffusion_refinement_amd import _lib

U = 2.0 ** -24
V = 2.0 ** -53
SUB = 2.0 ** -149
EPS = float(np.float32(1e-5))
ACTS = ("none", "relu", "swish")
PATTERNS = ("normal", "offset", "constant")
MASK_GAP = 1e-3

# (B, C, S, G): one-element slabs (variance 0); 3 pass-through channels, scalar family; Cg = 2, vector family; both
# with more than one cloud and odd sizes; Cg = 4; the min(32, cin) groups with 2 pass-through channels.
FIXED_SHAPES = [(1, 32, 1, 32), (2, 35, 7, 32), (1, 64, 12, 32), (2, 67, 33, 32), (1, 131, 260, 32), (2, 16, 20, 16),
                (1, 10, 8, 4)]


def plan(C, S, G, aligned16=1):
    """(rc, [family, partitions per slab, elements per partition, Cg])."""
    out = (ctypes.c_long * 4)(-7, -7, -7, -7)
    rc = _lib.load().pdr_group_norm_act_plan(C, S, G, aligned16, out)
    return rc, list(out)


def workspace_bytes(B, C, S, G):
    return _lib.load().pdr_group_norm_act_workspace_bytes(B, C, S, G)


def partition_shapes():
    """C = G = 32 (Cg = 1, m = S) with S read from the plan: one element more than one partition and two partitions
    plus one (scalar family: S is odd), and the same with four more (vector family): the partial combine and the
    tails run."""
    rc, p = plan(32, 1, 32)
    assert rc == 0
    E = p[2]
    shapes = []
    for S, fam, parts in ((E + 1, 0, 2), (2 * E + 1, 0, 3), (E + 4, 1, 2), (2 * E + 4, 1, 3)):
        rc, q = plan(32, S, 32)
        assert rc == 0 and q == [fam, parts, E, 1], (S, q)
        shapes.append((1, 32, S, 32))
    return shapes


def shapes():
    return FIXED_SHAPES + partition_shapes()


def composition(x, weight, bias, G, eps, act):
    """act(MyGroupNorm(x)) of pointnet2_ops/attention.py:18-32 and the activation modules, in x's dtype."""
    C = x.shape[1]
    cn = C - C % G
    # torch.group_norm is what F.group_norm calls after its size guard, which refuses the one-value-per-channel case
    # (1, 32, 1) although the operator defines it (variance 0)
    h = torch.group_norm(x[:, :cn], G, weight, bias, eps, False)
    z = h if cn == C else torch.cat([h, x[:, cn:]], dim=1)
    if act == "relu":
        return F.relu(z)
    if act == "swish":
        return z * torch.sigmoid(z)
    return z


def _slab_view(a, B, G, Cg):
    """(B, C, S) -> (B, G, Cg * S) of the normalised channels."""
    return a[:, :G * Cg].reshape(B, G, -1)


def _z64(x, gamma, beta, G):
    """float64 z of the composition (B, C, S) and the per-slab rstd (B, G), straight from the definition."""
    B, C, S = x.shape
    Cg = (C - C % G) // G
    xs = _slab_view(x.astype(np.float64), B, G, Cg)
    mean = xs.mean(-1, keepdims=True)
    var = ((xs - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    xh = ((xs - mean) * rstd).reshape(B, G * Cg, S)
    g = np.ones(G * Cg) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(G * Cg) if beta is None else beta.astype(np.float64)
    z = np.concatenate([xh * g[None, :, None] + b[None, :, None], x[:, G * Cg:].astype(np.float64)], axis=1)
    return z, rstd[..., 0], var[..., 0]


def make(shape, pattern, affine):
    """fp32 host arrays (x (B, C, S), gamma, beta (Cn) or None, grad_y), seeded by shape / pattern / affine, after the
    mask-safety pass of the module docstring.  The same inputs serve all three activations."""
    B, C, S, G = shape
    Cg = (C - C % G) // G
    Cn = G * Cg
    rng = np.random.default_rng([B, C, S, G, PATTERNS.index(pattern), int(affine)])
    if pattern == "normal":
        x = rng.standard_normal((B, C, S)) * 2.0 + rng.standard_normal((B, C, 1))
    elif pattern == "offset":
        x = 100.0 + rng.standard_normal((B, C, S))
    else:
        x = rng.standard_normal((B, C, S))
        slab = np.round(rng.uniform(-8.0, 8.0, (B, G, 1)) * 4.0) / 4.0          # one repeated value per slab
        x[:, :Cn] = np.broadcast_to(slab, (B, G, Cg * S)).reshape(B, Cn, S)
    x = x.astype(np.float32)
    gamma = beta = None
    if affine:
        gamma = 1.0 + 0.5 * rng.standard_normal(Cn)
        gamma = np.where(np.abs(gamma) < 0.1, 0.1, gamma).astype(np.float32)
        beta = 0.5 * rng.standard_normal(Cn)
        beta = np.where(np.abs(beta) < 2e-3, 2e-3, beta).astype(np.float32)
    gy = rng.standard_normal((B, C, S)).astype(np.float32)
    for _ in range(20):
        z, rstd, var = _z64(x, gamma, beta, G)
        flat = np.repeat(var == 0.0, Cg, axis=1)[:, :, None]                     # (B, Cn, 1): slabs no x can move
        movable = np.concatenate([np.broadcast_to(~flat, (B, Cn, S)), np.ones((B, C - Cn, S), bool)], axis=1)
        bad = (np.abs(z) < MASK_GAP) & movable
        if not bad.any():
            break
        g = np.ones(Cn) if gamma is None else gamma.astype(np.float64)
        per_z = np.concatenate([np.repeat(rstd, Cg, axis=1)[:, :, None] * g[None, :, None] * np.ones((1, 1, S)),
                                np.ones((B, C - Cn, S))], axis=1)               # dz / dx, up to 1 - 1 / m
        sign = np.where(z >= 0, 1.0, -1.0)
        x = np.where(bad, x + sign * 4.0 * MASK_GAP / per_z, x).astype(np.float32)
    z, _, var = _z64(x, gamma, beta, G)
    flat = np.concatenate([np.broadcast_to(np.repeat(var == 0.0, Cg, axis=1)[:, :, None], (B, Cn, S)),
                           np.zeros((B, C - Cn, S), bool)], axis=1)
    undecided = np.abs(z) < MASK_GAP
    if affine:
        assert not undecided.any(), (shape, pattern, int(undecided.sum()))
    else:
        assert not (undecided & ~flat).any() and not z[flat].any(), (shape, pattern)
    return x, gamma, beta, gy


def reference(shape, x, gamma, beta, gy, act):
    """float64 composition and its autograd gradients on the CPU with the bounds of the module docstring: a dict of
    read-only float64 arrays y, mean, rstd, gx, gw, gb (gw / gb None without affine parameters) and b_<name> each."""
    B, C, S, G = shape
    Cg = (C - C % G) // G
    Cn = G * Cg
    m = Cg * S
    x64 = torch.tensor(x).double().requires_grad_()
    params = [] if gamma is None else [torch.tensor(gamma).double().requires_grad_(),
                                       torch.tensor(beta).double().requires_grad_()]
    y = composition(x64, params[0] if params else None, params[1] if params else None, G, EPS, act)
    grads = torch.autograd.grad(y, [x64] + params, torch.tensor(gy).double())
    y, gx = y.detach().numpy(), grads[0].numpy()
    gw, gb = (grads[1].numpy(), grads[2].numpy()) if params else (None, None)

    xd, dy = x.astype(np.float64), gy.astype(np.float64)
    xs = _slab_view(xd, B, G, Cg)
    mean = xs.mean(-1)
    var = ((xs - mean[..., None]) ** 2).mean(-1)
    rstd = 1.0 / np.sqrt(var + EPS)
    A1, A2 = np.abs(xs).mean(-1), (xs ** 2).mean(-1)
    b_mean = U * np.abs(mean) + V * (m + 1) * A1
    rel = U + V * (3 * m + 4) * A2 / (2 * (var + EPS)) + 4 * V
    b_rstd = rstd * rel
    row = lambda a: np.repeat(a, Cg, axis=1)[:, :, None]                        # (B, G) -> (B, Cn, 1)
    g = np.ones(Cn) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(Cn) if beta is None else beta.astype(np.float64)
    g3, b3 = g[None, :, None], b[None, :, None]
    xn, dyn = xd[:, :Cn], dy[:, :Cn]
    xh = (xn - row(mean)) * row(rstd)
    zn = xh * g3 + b3
    b_xh = row(rstd) * row(b_mean) * (1 + 4 * U) + np.abs(xh) * (3 * U + row(rel))
    b_zn = np.abs(g3) * b_xh * (1 + U) + U * np.abs(zn)
    z = np.concatenate([zn, xd[:, Cn:]], axis=1)
    b_z = np.concatenate([b_zn, np.zeros((B, C - Cn, S))], axis=1)
    flat = np.concatenate([np.broadcast_to(row(var == 0.0), (B, Cn, S)), np.zeros((B, C - Cn, S), bool)], axis=1)
    assert (b_z < np.abs(z))[~flat].all(), shape                                # the kernel's z has the reference's sign
    if act == "swish":
        s = 1.0 / (1.0 + np.exp(-z))
        de = np.expm1(2 * U * np.abs(z)) + 2 * U
        b_y = 1.1 * b_z + np.abs(z * s) * ((1 - s) * de + 4 * U) + 2.0 ** -120
        es = (1 - s) * de + 2 * U
        a = s * (1 + z * (1 - s))
        dz = dy * a
        b_dz = np.abs(dy) * (0.5 * b_z + s * (np.abs(z) * (s * es + 2 * U * (1 - s)) + U * np.abs(1 + z * (1 - s)))
                             + (es + 2 * U) * np.abs(a) + U * s) + U * np.abs(dz)
    else:
        b_y = b_z
        dz = dy * (z > 0) if act == "relu" else dy
        b_dz = np.zeros_like(dz)
    dzn, b_dzn = dz[:, :Cn], b_dz[:, :Cn]
    r1, r2 = (dzn * xh).sum(-1), dzn.sum(-1)                                    # (B, Cn)
    e_r1 = (b_dzn * np.abs(xh) + np.abs(dzn) * b_xh + b_dzn * b_xh).sum(-1) + V * (S + 2) * np.abs(dzn * xh).sum(-1)
    e_r2 = b_dzn.sum(-1) + V * (S + 2) * np.abs(dzn).sum(-1)
    b_gw = e_r1.sum(0) * (1 + U) + (U + V * (B + 2)) * np.abs(r1).sum(0) + SUB
    b_gb = e_r2.sum(0) * (1 + U) + (U + V * (B + 2)) * np.abs(r2).sum(0) + SUB
    slab = lambda a: a.reshape(B, G, Cg).sum(-1)                                # (B, Cn) -> (B, G)
    ag = np.abs(g)[None, :]
    c1, c2 = slab(g[None, :] * r1), slab(g[None, :] * r2)
    e_c1 = slab(ag * e_r1) + V * (Cg + 2) * slab(ag * np.abs(r1))
    e_c2 = slab(ag * e_r2) + V * (Cg + 2) * slab(ag * np.abs(r2))
    k1, k2 = row(c1 / m), row(c2 / m)
    e_k1, e_k2 = row(e_c1 / m) + (U + V) * np.abs(k1), row(e_c2 / m) + (U + V) * np.abs(k2)
    e_t = np.abs(g3) * b_dzn + U * np.abs(g3 * dzn)
    t2 = xh * k1 + k2
    e_t2 = b_xh * (np.abs(k1) + e_k1) + np.abs(xh) * e_k1 + e_k2
    e_t2 = e_t2 + U * (np.abs(t2) + e_t2)
    w = g3 * dzn - t2
    e_w = (e_t + e_t2) * (1 + U) + U * np.abs(w)
    dxn = row(rstd) * w
    b_dxn = row(rstd) * e_w * (1 + row(rel) + 2 * U) + np.abs(dxn) * (row(rel) + 2 * U) + SUB
    b_gx = np.concatenate([b_dxn, b_dz[:, Cn:]], axis=1)
    r = dict(y=y, mean=mean, rstd=rstd, gx=gx, gw=gw, gb=gb, b_y=b_y, b_mean=b_mean, b_rstd=b_rstd, b_gx=b_gx,
             b_gw=b_gw if params else None, b_gb=b_gb if params else None, z=z, dz=dz)
    for a in r.values():
        if a is not None:
            a.setflags(write=False)
    return r


OUTPUTS = ("y", "mean", "rstd", "gx", "gw", "gb")


def worst_ratio(got, ref):
    """{name: max |got - reference| / bound} over the six outputs (`got`: a dict of arrays, None entries skipped); a
    non-finite value or an error at a zero bound gives inf."""
    out = {}
    for name in OUTPUTS:
        if got.get(name) is None or ref[name] is None:
            continue
        have = np.asarray(got[name], dtype=np.float64).reshape(ref[name].shape)
        err, bound = np.abs(have - ref[name]), ref["b_" + name]
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        ratio = np.where(np.isfinite(have), ratio, np.inf)
        out[name] = float(ratio.max())
    return out


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)
