"""Cases, emulation and bounds of pdr_group_norm_act_add / pdr_group_norm_act_add_grad, on top of
tests/group_norm_act_cases.py (a helper module like it, not a conftest).

The op is pdr_group_norm_act followed by two fp32 additions, y = fl(fl(act(z) + e[b, c]) + r[b, c, s]); its backward
is pdr_group_norm_act_grad plus ONE new quantity,
    grad_e[b, c] = float(sum_s double(grad_y[b, c, s]))      the raw grad_y, on every row, pass-through rows too.
Everything the two entries share with the existing ones is tested by bit-equality against those (the GPU test); this
module holds what is new:

  inputs      `terms(shape)`: e (B, C) and r (B, C, S), seeded by the shape; x, gamma, beta, grad_y are GC.make's.
  emulation   `row_sums_emulated(gy, V)`: the row kernel's order, operation for operation in IEEE double -- thread t of
              256 adds the elements (256 i + t) V .. + V - 1 for i = 0, 1, .. to a +0.0 accumulator, the 64 lanes of a
              wave fold by a butterfly over lane distance 32, 16, .. 1 (lane 0 is read; every lane holds the same bits),
              the four waves add ascending, one rounding to fp32.  V = 4 in the vector family, 1 in the scalar one.
  reference   `row_sums_exact(gy)`: math.fsum, the correctly rounded double of the exact sum.
  bound       `grad_e_bound(gy)` = u |sum| + S v sum |grad_y|: a double sum of S terms in ANY order is within
              (S - 1) v sum|.| of the exact one, the rounding to fp32 adds u |sum| (u = 2^-24, v = 2^-53).
  forward     `forward_bound(ref, e, r)`: b_y of GC.reference carried through the two additions,
              b = b_y (1 + 2 u) + u |y + e| (1 + u) + u |(y + e) + r|, with y, e, r the float64 values.
  wrong variants, for the host test that shows the bound can tell them apart:
              `grad_e_before_activation`: the gradient of act(z + e) -- e injected in front of the activation;
              `grad_e_from_dz`: the row sum of dz = dy act'(z) instead of dy.
"""
import math

import numpy as np

from tests import group_norm_act_cases as GC

U, V = GC.U, GC.V
TERMS = ("e", "r", "both")


def shapes():
    """The four fixed shapes of the issue -- pass-through channels with an odd S (scalar family), the vector family,
    one and two clouds -- and one two-partition shape read from the plan (vector family, P = 2)."""
    fixed = [(2, 35, 7, 32), (2, 67, 33, 32), (1, 131, 260, 32), (2, 16, 20, 16)]
    assert all(s in GC.FIXED_SHAPES for s in fixed)
    two = GC.partition_shapes()[2]
    rc, p = GC.plan(two[1], two[2], two[3])
    assert rc == 0 and p[0] == 1 and p[1] == 2, p
    return fixed + [two]


def terms(shape, which="both"):
    """fp32 host arrays (e (B, C) or None, r (B, C, S) or None)."""
    B, C, S, G = shape
    rng = np.random.default_rng([B, C, S, G, 77])
    e = rng.standard_normal((B, C)).astype(np.float32)
    r = (2.0 * rng.standard_normal((B, C, S))).astype(np.float32)
    assert which in TERMS
    return (e if which in ("e", "both") else None), (r if which in ("r", "both") else None)


def row_sums_emulated(gy, vec):
    """gy (..., S) fp32 -> (...) fp32: the row kernel's sum of the raw grad_y, operation for operation.  Padding a row
    with +0.0 up to a whole number of passes changes no bit: an accumulator that starts at +0.0 is never -0.0."""
    gy = np.asarray(gy, dtype=np.float32)
    lead, S = gy.shape[:-1], gy.shape[-1]
    assert vec in (1, 4) and (vec == 1 or S % 4 == 0)
    passes = -(-S // (256 * vec))
    a = np.zeros((int(np.prod(lead, dtype=np.int64)), passes * 256 * vec), dtype=np.float64)
    a[:, :S] = gy.reshape(-1, S).astype(np.float64)
    a = a.reshape(-1, passes, 256, vec)
    acc = np.zeros((a.shape[0], 256), dtype=np.float64)
    for i in range(passes):
        for j in range(vec):
            acc = acc + a[:, i, :, j]
    waves = acc.reshape(-1, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, :, lane ^ off]
    w = waves[:, :, 0]
    total = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return total.astype(np.float32).reshape(lead)


def row_sums_exact(gy):
    """(..., S) -> (...) float64: the correctly rounded exact sum of every row."""
    gy = np.asarray(gy, dtype=np.float64)
    flat = gy.reshape(-1, gy.shape[-1])
    return np.array([math.fsum(row) for row in flat], dtype=np.float64).reshape(gy.shape[:-1])


def grad_e_bound(gy):
    gy = np.asarray(gy, dtype=np.float64)
    return U * np.abs(row_sums_exact(gy)) + gy.shape[-1] * V * np.abs(gy).sum(-1)


def outside(got, gy):
    """Boolean (...) array: rows of `got` that leave grad_e_bound around the exact row sum (or are not finite)."""
    got = np.asarray(got, dtype=np.float64)
    return ~(np.abs(got - row_sums_exact(gy)) <= grad_e_bound(gy))


def forward_reference(ref, e, r):
    """float64 (y + e[:, :, None]) + r of a GC.reference dict and the bound of the module docstring."""
    y, b = ref["y"], ref["b_y"] * (1 + 2 * U)
    if e is not None:
        y = y + e.astype(np.float64)[:, :, None]
        b = b + U * np.abs(y) * (1 + U)
    if r is not None:
        y = y + r.astype(np.float64)
        b = b + U * np.abs(y)
    return y, b


def _act_prime(z, act):
    if act == "relu":
        return (z > 0).astype(np.float64)
    if act == "swish":
        s = 1.0 / (1.0 + np.exp(-z))
        return s * (1 + z * (1 - s))
    return np.ones_like(z)


def grad_e_before_activation(ref, gy, e, act):
    """WRONG on purpose: grad_e of y = act(z + e) + r, float64."""
    return (gy.astype(np.float64) * _act_prime(ref["z"] + e.astype(np.float64)[:, :, None], act)).sum(-1)


def grad_e_from_dz(ref):
    """WRONG on purpose: the row sum of dz = dy act'(z) instead of the raw dy, float64."""
    return ref["dz"].sum(-1)
