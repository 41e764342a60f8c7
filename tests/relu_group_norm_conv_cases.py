"""Cases, float64 reference, derived error bounds and an operation-for-operation emulation of
pdr_relu_group_norm_conv_cf / _grad_input / _grad_weight.  (A helper module like tests/relu_group_norm_cases.py, which it
builds on, not a conftest.)

REFERENCE (never the kernel): `composition64`, conv2d(MyGroupNorm(relu(cat([q expanded over K, k], 1)))) in float64 on
the CPU from the fp32 inputs, gradients from float64 autograd of it.

EMULATION.  xn = the normalised tensor with the kernel's bits given the op's fp32 mean / rstd (`xn_bits`: the chain
d = fl(u - mean), xh = fl(d rstd), fma(xh, gamma, beta) of RC.emulate, without RC.emulate's backward).  The two
bit-defined GEMMs are `chain`: acc = +0, then one vectorised RC.fma32 step per contraction index, ascending.

BOUNDS, u = 2^-24, v = 2^-53.
  out     |out - ref| <= sum_c |W| b_y[c] + (C + 2) u sum_c |W xn| + u |out|
            b_y: RC's bound on the normalised value; a chain of C fmas is within C u sum|terms| of the exact sum of its
            terms to first order, the + 2 is slack for the second order and the bias add, u |out| the last rounding.
  grad_W  against the float64 sum of grad_out xn_emulated (xn_emulated has the kernel's bits: only accumulation error is
            left): (L + 4) u sum |grad_out xn| + 2^-149 -- a chain of at most L fmas per partial, the partials added in
            double and rounded once.
  grad_b  (u + v (B N K + 2)) sum |grad_out| + 2^-149: a double sum in any order, rounded once.
"""
import ctypes
from fractions import Fraction

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib
from tests import relu_group_norm_cases as RC

U, V, SUB, EPS, PATTERNS = RC.U, RC.V, RC.SUB, RC.EPS, RC.PATTERNS
PLAN_KEYS = ("family", "P", "E", "Cg", "tile", "L", "R", "rows")

# (B, C1, C2, N, K, G, Cout): a group straddling q | k, 3 pass-through channels, vector family, Cout no multiple of 32,
# S = 28 below one tile; scalar family, odd S; no q, K = 1; Cg = 1, Cout = C; whole groups inside q; several c-chunks
# and more than one column block; the network's widest head at 16 positions.
FIXED_CASES = [(2, 33, 34, 7, 4, 32, 40), (2, 32, 35, 5, 3, 32, 33), (1, 0, 64, 12, 1, 32, 64), (2, 0, 32, 9, 5, 32, 32),
               (1, 40, 24, 6, 8, 32, 96), (1, 64, 331, 4, 8, 32, 160), (1, 256, 651, 2, 8, 32, 512)]


def plan(C1, C2, N, K, G, Cout, aligned16=1):
    """(rc, dict of PLAN_KEYS)."""
    out = (ctypes.c_long * 8)(*([-7] * 8))
    rc = _lib.load().pdr_relu_group_norm_conv_cf_plan(C1, C2, N, K, G, Cout, aligned16, out)
    return rc, dict(zip(PLAN_KEYS, (int(v) for v in out)))


def workspace_bytes(B, C1, C2, N, K, G, Cout):
    return _lib.load().pdr_relu_group_norm_conv_cf_workspace_bytes(B, C1, C2, N, K, G, Cout)


def plan_case():
    """B = 3, C1 = C2 = 32, Cout = 64, K = 32 and N read from the plan: one query more than a weight-gradient chain
    holds, so a cloud has two ranges (the second a tail of one query), at least three position tiles, the last one
    partial."""
    rc, p = plan(32, 32, 1, 32, 32, 64)
    assert rc == 0
    N = p["L"] // 32 + 1
    rc, p = plan(32, 32, N, 32, 32, 64)
    S = N * 32
    assert rc == 0 and p["R"] >= 2 and -(-S // p["tile"]) >= 3 and S % p["tile"] != 0 and S % p["L"] != 0, (N, p)
    return (3, 32, 32, N, 32, 32, 64)


def cases():
    return FIXED_CASES + [plan_case()]


def dims(case):
    B, C1, C2, N, K, G, Cout = case
    C = C1 + C2
    Cg = (C - C % G) // G
    return B, C1, C2, N, K, G, Cout, C, Cg, G * Cg, N * K


def make(case, pattern, affine):
    """fp32 host arrays (q, k, gamma, beta as RC.make, W (Cout, C), cbias (Cout), grad_out (B, Cout, N, K), grad_y of
    RC.make), seeded by case / pattern / affine."""
    B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = dims(case)
    q, k, gamma, beta, gy = RC.make(case[:6], pattern, affine)
    rng = np.random.default_rng([B, C1, C2, N, K, G, Cout, PATTERNS.index(pattern), int(affine)])
    W = (rng.standard_normal((Cout, C)) / np.sqrt(C)).astype(np.float32)
    cbias = (0.5 * rng.standard_normal(Cout)).astype(np.float32)
    go = rng.standard_normal((B, Cout, N, K)).astype(np.float32)
    if pattern == "zero_gy":
        go = np.zeros_like(go)
    return q, k, gamma, beta, W, cbias, go, gy


def xn_bits(case, q, k, gamma, beta, mean, rstd):
    """The normalised tensor (B, C, N, K) fp32 with the kernel's bits given fp32 mean / rstd (B, G): RC.emulate's y."""
    B, C1, C2, N, K, G, Cout, C, Cg, Cn, S = dims(case)
    f32 = np.float32
    u = RC.relu32(RC.virtual(q, k).astype(f32)).reshape(B, C, S)
    row = lambda a: np.repeat(np.asarray(a, f32), Cg, axis=1)[:, :, None]
    gm = np.ones(Cn, f32) if gamma is None else gamma
    bt = np.zeros(Cn, f32) if beta is None else beta
    d = (u[:, :Cn] - row(mean)).astype(f32)
    xh = (d * row(rstd)).astype(f32)
    y = np.concatenate([RC.fma32(xh, gm[None, :, None], bt[None, :, None]), u[:, Cn:]], axis=1)
    return y.reshape(B, C, N, K)


def chain(A, X):
    """A (M, Kd), X (B, Kd, ...) fp32 -> (B, M, ...): acc = +0; for kk ascending: acc = fma(A[m, kk], X[b, kk], acc)."""
    A, X = np.asarray(A, np.float32), np.asarray(X, np.float32)
    shape = X.shape
    X = X.reshape(shape[0], shape[1], -1)
    acc = np.zeros((shape[0], A.shape[0], X.shape[2]), np.float32)
    for kk in range(A.shape[1]):
        acc = RC.fma32(A[None, :, kk, None], X[:, None, kk, :], acc)
    return acc.reshape((shape[0], A.shape[0]) + shape[2:])


def emulate_forward(W, cbias, xn):
    acc = chain(W, xn)
    return acc if cbias is None else (acc + cbias[None, :, None, None]).astype(np.float32)


def emulate_grad_input(W, go):
    return chain(np.ascontiguousarray(W.T), go)


def fma32_exact(a, b, c):
    """One fp32 fused multiply-add through exact rationals (scalars): where RC.fma32's 80-bit sum double-rounds."""
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    lo = np.float32(float(r))                   # float(r) is correctly rounded to double: a candidate, then its neighbours
    best = None
    for cand in (np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - r)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return np.float32(best[1])


def chain_exact(A_row, X_col):
    """The chain of one output element with exact fmas: A_row (Kd), X_col (Kd)."""
    acc = np.float32(0.0)
    for a, x in zip(A_row, X_col):
        acc = fma32_exact(a, x, acc)
    return acc


def same_bits_or_exact(got, emu, A, X, bias=None):
    """got == emu bit for bit, or, on the differing elements (where the 80-bit fma32 may have rounded twice), got ==
    the chain with Fraction-exact fmas.  got / emu (B, M, ...), A (M, Kd), X (B, Kd, ...).  Returns the number of
    elements that needed the exact chain; raises AssertionError on a real difference."""
    gb, eb = RC.bits(got).reshape(emu.shape), RC.bits(emu)
    bad = np.argwhere(gb != eb)
    assert len(bad) <= 64, "%d of %d elements differ from the emulated chain" % (len(bad), gb.size)
    for idx in bad:
        b, m = idx[0], idx[1]
        rest = tuple(idx[2:])
        v = chain_exact(A[m], X[(b, slice(None)) + rest])
        if bias is not None:
            v = np.float32(v + bias[m])
        have = np.asarray(got).reshape(emu.shape)[tuple(idx)]
        assert np.float32(have).view(np.uint32) == v.view(np.uint32), (tuple(idx), have, v, emu[tuple(idx)])
    return len(bad)


def composition64(q, k, gamma, beta, W, cbias, G, go=None):
    """The float64 composition on the CPU.  -> dict out (B, Cout, N, K) and, with `go`, gq, gk, gw, gb, gcw, gcb
    (float64 numpy; None where the input is)."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a)).double().requires_grad_(go is not None)
    q64, k64, g64, b64, W64, c64 = t(q), t(k), t(gamma), t(beta), t(W), t(cbias)
    y = RC.composition(q64, k64, g64, b64, G, EPS)
    out = torch.nn.functional.conv2d(y, W64[:, :, None, None], c64)
    r = dict(out=out.detach().numpy(), gq=None, gk=None, gw=None, gb=None, gcw=None, gcb=None)
    if go is not None:
        named = [(n, v) for n, v in (("gq", q64), ("gk", k64), ("gw", g64), ("gb", b64), ("gcw", W64), ("gcb", c64))
                 if v is not None]
        grads = torch.autograd.grad(out, [v for _, v in named], torch.tensor(go).double())
        for (n, _), g in zip(named, grads):
            r[n] = g.numpy()
    return r


def out_bound(case, ref_rc, W, out64):
    """The bound on |out - out64| from RC.reference's y and b_y (float64 (B, C, N, K))."""
    C = W.shape[1]
    aw = np.abs(W.astype(np.float64))
    t1 = np.einsum("oc,bcnk->bonk", aw, ref_rc["b_y"])
    t2 = np.einsum("oc,bcnk->bonk", aw, np.abs(ref_rc["y"]))
    return t1 + (C + 2) * U * t2 + U * np.abs(out64)


def grad_weight_reference(go, xn):
    """(float64 sum of grad_out xn over (b, n, j), the sum of |grad_out xn|, sum grad_out, sum |grad_out|)."""
    g, x = go.astype(np.float64), xn.astype(np.float64)
    return (np.einsum("bonk,bcnk->oc", g, x), np.einsum("bonk,bcnk->oc", np.abs(g), np.abs(x)), g.sum((0, 2, 3)),
            np.abs(g).sum((0, 2, 3)))


def ratio(err, bound):
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(np.where(np.isfinite(err), r, np.inf))) if r.size else 0.0
