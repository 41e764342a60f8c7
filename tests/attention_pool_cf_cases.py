"""Cases, float64 reference and derived error bounds of pdr_attention_pool_cf / pdr_attention_pool_cf_grad.
(A helper module like tests/pool_cases.py, not a conftest.)

REFERENCE (never the kernel): the composition of pointnet2_ops/attention.py:71-77, written out in `composition`,
evaluated in float64 on the CPU from the fp32 inputs; gradients from float64 autograd of it.

BOUNDS, derived from the operation chain in the header of csrc/attention_pool_cf.hip, u = 2^-24.  For one row let V be
its valid slots (k < c_n), s_m = max_V s_k, p the float64 softmax weights, out = sum_k p_k v_k, D_k = v_k - out.

  E, the worst perturbation of an exponent argument, in natural-log units, over the valid slots:
      E = max_V [ 4 u (|s_k| + |s_m|) + 2 u ].
    The kernel forms fl(fl(s_k c) - fl(s_m c)) with c = fl(log2 e): one relative u for the constant, one for each of
    the two products and one for the difference, each on at most (|s_k| + |s_m|) log2 e; three roundings touch any one
    term, the fourth u is slack for the second-order terms (the 4 u (|s| + |m|) of tests/pool_cases.py).  v_exp_f32 is
    accurate to 1 ulp = 2^-23 relative = 2 u, and ln(1 + 2u) <= 2u moves it into the exponent: the + 2 u.
    A masked slot has weight exactly 0 on both sides (exp of about -1e9) and does not enter E.
  If every exponent moves by at most E, every RATIO of two weights moves by a factor within e^{+-2E}; so the
  normalised weights p^ the kernel's e_k define satisfy |p^_k - p_k| <= expm1(2E) p_k, and, the changes summing to
  zero, the exactly evaluated weighted mean moves by at most expm1(2E) sum_k p_k |D_k|.

  out:          B_out = expm1(2E) sum_k p_k |D_k|  +  (2K + 4) u e^{2E} sum_k p_k |v_k|  +  TINY sum_k |v_k|
    second term: l is K - 1 additions of positive terms (relative (K - 1) u whatever the order, sequential or tree),
    acc is K fused multiply-adds (K u on sum_k e_k |v_k|), the division one more: (2K) u in all, + 4 u of slack for
    the second-order terms, on sum_k p^_k |v_k| <= e^{2E} sum_k p_k |v_k|.
  grad_values:  B_gv[k] = |g| p_k ( expm1(2E) + (K + 4) u e^{2E} )  +  TINY |g| + 2^-149
    w_k = fl(e_k fl(1 / l^)): (K - 1) u for l^, u for the reciprocal, u for the product, u for fl(g w_k): (K + 2) u,
    + 2 u slack.
  grad_scores:  the kernel multiplies gv_k (within B_gv of g p_k) by fl(v_k - out^) (out^ within B_out of out):
      dD    = B_out + u (|D_k| + B_out)                 error of fl(v_k - out^) against D_k
      gv_hi = |g| p_k + B_gv[k]                         magnitude of the first factor
      B_gs[k] = gv_hi dD  +  B_gv[k] |D_k|  +  u gv_hi (|D_k| + dD)  +  TINY |g| (|D_k| + 1) + 2^-149
    (error of the second factor, of the first, and the rounding of the product.)  At masked slots grad_scores is
    exactly +0.0f: checked by bits, not by a bound.
  TINY = 2^-125: v_exp_f32 returns 0 instead of a subnormal, an absolute 2^-126 on a weight (l >= 1: the slot of the
  maximum contributes exactly 1), and a product that lands among the subnormals is rounded to within 2^-149.

INPUTS THAT MAKE FAULTS LOUD: in the ragged count modes the masked slots of `scores` hold +-1e6 (finite, and far above
every valid score: a kernel that looked at one would put all the weight there); a second draw of that junk must change
no bit of any output.  The "spread" scores reach +-60 (without the maximum subtraction exp overflows), the "equal" ones
make every weight 1 / c_n.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from point_diffusion_refinement_amd import _lib

U = 2.0 ** -24
TINY = 2.0 ** -125
SUB = 2.0 ** -149

# (B, C, N, K): one row; scalar family with rows a multiple of nothing; every lane count of the vector family
# (1 / 2 / 4 / 8 / 16), more than one workgroup, rows not a multiple of the rows per workgroup; idle lanes (K = 12, 40)
SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (1, 3, 11, 33), (2, 3, 9, 4), (2, 3, 9, 8), (1, 4, 130, 16), (2, 33, 65, 32),
          (1, 2, 5, 64), (1, 3, 7, 12), (1, 2, 9, 40)]
COUNT_MODES = ("none", "random", "zero", "one", "full")
PATTERNS = ("normal", "spread", "equal")


def plan(K, aligned16=1):
    """(rc, [family, lanes per row, rows per workgroup, rows per lane group per grid pass])."""
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = _lib.load().pdr_attention_pool_cf_plan(K, aligned16, out)
    return rc, list(out)


def make(shape, mode, pattern, junk=0):
    """fp32 host arrays (scores, values, counts or None, grad_out), seeded by shape / mode / pattern; `junk` selects the
    draw of the +-1e6 that fills the masked score slots and changes nothing else."""
    B, C, N, K = shape
    rng = np.random.default_rng([B, C, N, K, COUNT_MODES.index(mode), PATTERNS.index(pattern)])
    if pattern == "normal":
        s = rng.standard_normal(shape) * 4.0
    elif pattern == "spread":
        s = rng.uniform(-60.0, 60.0, shape)
    else:
        s = np.broadcast_to(rng.standard_normal((B, C, N, 1)) * 3.0, shape)
    s = np.ascontiguousarray(s, dtype=np.float32)
    v = rng.standard_normal(shape).astype(np.float32)
    g = rng.standard_normal((B, C, N)).astype(np.float32)
    if mode == "none":
        cnt = None
    elif mode == "random":
        cnt = rng.integers(-1, K + 3, (B, N)).astype(np.int32)          # [-1, K + 2]
    else:
        cnt = np.full((B, N), {"zero": 0, "one": 1, "full": K}[mode], dtype=np.int32)
    if cnt is not None:
        masked = np.arange(K)[None, None, None, :] >= np.clip(cnt, 1, K)[:, None, :, None]
        jr = np.random.default_rng([junk, B, C, N, K])
        s = np.where(masked, np.where(jr.random(shape) < 0.5, -1e6, 1e6), s).astype(np.float32)
    return s, v, cnt, g


def count_to_mask(count, K):
    ar = torch.arange(K, device=count.device, dtype=count.dtype)
    return ar.view(1, 1, K) < count.unsqueeze(-1)


def composition(scores, values, count):
    """attention.py:71-77 with the value conv taken as done, in the dtype of `scores`; count a tensor or None ('all')."""
    K = scores.shape[-1]
    if count is not None:
        mask = count_to_mask(torch.clamp(count, min=1), K).unsqueeze(1).to(scores.dtype)
        scores = scores * mask + (-1e9) * (1 - mask)
    weight = F.softmax(scores, dim=-1)
    return (values * weight).sum(dim=-1)


def reference(s, v, cnt, g):
    """float64 composition and its autograd gradients on the CPU, with the bounds of the module docstring.
    Returns a dict of read-only float64 arrays: out, gs, gv, b_out, b_gs, b_gv, and the bool array `masked`."""
    K = s.shape[-1]
    s64 = torch.from_numpy(s).double().requires_grad_()
    v64 = torch.from_numpy(v).double().requires_grad_()
    c = None if cnt is None else torch.from_numpy(cnt).long()
    out = composition(s64, v64, c)
    gs, gv = torch.autograd.grad(out, (s64, v64), torch.from_numpy(g).double())
    out, gs, gv = out.detach().numpy(), gs.numpy(), gv.numpy()
    cn = np.full((s.shape[0], s.shape[2]), K) if cnt is None else np.clip(cnt.astype(np.int64), 1, K)
    valid = np.arange(K)[None, None, None, :] < cn[:, None, :, None]
    valid = np.broadcast_to(valid, s.shape)
    sd, vd, gd = s.astype(np.float64), v.astype(np.float64), np.abs(g.astype(np.float64))[..., None]
    sm = np.where(valid, sd, -np.inf).max(-1, keepdims=True)
    E = np.where(valid, 4 * U * (np.abs(sd) + np.abs(sm)) + 2 * U, 0.0).max(-1, keepdims=True)
    p = np.where(valid, np.exp(np.where(valid, sd - sm, 0.0)), 0.0)
    p = p / p.sum(-1, keepdims=True)
    D = np.abs(vd - out[..., None])
    rel, grow = np.expm1(2 * E), np.exp(2 * E)
    b_out = (rel * (p * D).sum(-1, keepdims=True) + (2 * K + 4) * U * grow * (p * np.abs(vd)).sum(-1, keepdims=True)
             + TINY * np.abs(vd).sum(-1, keepdims=True))
    b_gv = gd * p * (rel + (K + 4) * U * grow) + TINY * gd + SUB
    dD = b_out + U * (D + b_out)
    gv_hi = gd * p + b_gv
    b_gs = gv_hi * dD + b_gv * D + U * gv_hi * (D + dD) + TINY * gd * (D + 1) + SUB
    r = dict(out=out, gs=gs, gv=gv, b_out=b_out[..., 0], b_gs=b_gs, b_gv=b_gv, masked=~valid)
    for a in r.values():
        a.setflags(write=False)
    return r


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)
