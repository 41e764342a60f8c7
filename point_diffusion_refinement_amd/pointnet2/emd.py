"""Approximate earth mover's distance -- same surface as reference pointnet2/emd.py
(EarthMoverDistanceFunction :6-28, earth_mover_distance :31-56, EMD_distance :58-72),
running on libpdr_hip.so instead of the `emd_cuda` extension.

    cost = sum_{k,l} |xyz1_k - xyz2_l|^2 * match[l,k] / max(n, m)

When neither the match matrix nor a gradient is requested, the cost comes from the
fused pdr_emd_cost path that never materialises the (B,m,n) matrix (16.8 MB per
2048^2 pair in the reference, rewritten once per temperature level).

Padded batches: every function takes `lengths1` / `lengths2`, (B,) integer tensors; cloud b is then the pair
xyz1[b, :lengths1[b]], xyz2[b, :lengths2[b]] and gets exactly what the dense call gives on those slices (cost divided by
the pair's own max(n_b, m_b); match entries and gradient rows of the padding are 0; an empty pair costs 0).  The kernels
read the lengths on the device (pdr_*_ragged): no host sync, same launches, capturable.

Matrix-free gradient (`matrix_free=True`, opt-in): the default differentiable path materialises the (B,m,n) float32
match (537 MB at B = 32 and 2048^2) and autograd keeps it until backward, as the reference does.  With
matrix_free=True the forward is the fused cost (bit-equal to the call without a gradient) and the autograd node saves
only the clouds, the lengths and the call's workspace (10 * (n + m) factors per pair); backward is emd_cost_backward
(pdr_emd_cost_grad), which evaluates every match entry on the fly from those factors, by the expression
approxmatch_forward writes it with.  The gradients are those of the default path on its own match (grad1 bit for bit,
grad2 up to the order of one sum); the cost differs from the default path's in the last bits only (another reduction
order), which is why the default stays what it was.
"""
import torch
import torch.nn as nn

from .. import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(x, name):
    assert x.is_cuda, "Only support cuda currently."
    if x.dtype != torch.float32:
        raise RuntimeError("%s must be float32 (the double instantiation of the reference is not built)" % name)
    if x.dim() != 3 or x.shape[2] != 3:
        raise RuntimeError("%s must be (B, N, 3)" % name)


def _lengths(lengths, ref, name):
    """(B,) integer tensor -> int64 on `ref`'s device, contiguous (what the kernels read); None stays None = full."""
    if lengths is None:
        return None
    if not torch.is_tensor(lengths) or lengths.dim() != 1 or lengths.shape[0] != ref.shape[0]:
        raise RuntimeError("%s must be a tensor of shape (B,)" % name)
    if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
        raise RuntimeError("%s must be an integer tensor" % name)
    return lengths.to(device=ref.device, dtype=torch.int64).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def approxmatch_forward(xyz1, xyz2, lengths1=None, lengths2=None):
    """emd_cuda.approxmatch_forward: (B,n,3), (B,m,3) -> match (B,m,n); with lengths, match[b, l, k] = 0 for
    l >= lengths2[b] or k >= lengths1[b]."""
    _check(xyz1, "xyz1"), _check(xyz2, "xyz2")
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    lib = _lib.load()
    match = torch.empty((B, m, n), dtype=torch.float32, device=xyz1.device)
    temp = torch.empty((lib.pdr_emd_workspace_bytes(B, n, m) // 4,), dtype=torch.float32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        if lengths1 is None and lengths2 is None:
            _lib.check(lib.pdr_approxmatch(xyz1.data_ptr(), xyz2.data_ptr(), B, n, m, match.data_ptr(),
                                           temp.data_ptr(), _stream()), "approxmatch_forward")
        else:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            _lib.check(lib.pdr_approxmatch_ragged(xyz1.data_ptr(), xyz2.data_ptr(), _ptr(l1), _ptr(l2), B, n, m,
                                                  match.data_ptr(), temp.data_ptr(), _stream()), "approxmatch_forward")
    return match


def matchcost_forward(xyz1, xyz2, match, lengths1=None, lengths2=None):
    """emd_cuda.matchcost_forward: -> cost (B), not yet divided by max(n,m); with lengths, over the valid block of
    `match` only (its padding is never read)."""
    _check(xyz1, "xyz1"), _check(xyz2, "xyz2")
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    lib = _lib.load()
    cost = torch.empty((B,), dtype=torch.float32, device=xyz1.device)
    temp = torch.empty((lib.pdr_matchcost_workspace_bytes(B, n, m) // 4,), dtype=torch.float32, device=xyz1.device)
    match = match.contiguous()
    with torch.cuda.device(xyz1.device):
        if lengths1 is None and lengths2 is None:
            _lib.check(lib.pdr_matchcost(xyz1.data_ptr(), xyz2.data_ptr(), match.data_ptr(), B, n, m,
                                         cost.data_ptr(), temp.data_ptr(), _stream()), "matchcost_forward")
        else:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            _lib.check(lib.pdr_matchcost_ragged(xyz1.data_ptr(), xyz2.data_ptr(), _ptr(l1), _ptr(l2), match.data_ptr(),
                                                B, n, m, cost.data_ptr(), temp.data_ptr(), _stream()),
                       "matchcost_forward")
    return cost


def matchcost_backward(grad_cost, xyz1, xyz2, match, lengths1=None, lengths2=None):
    """emd_cuda.matchcost_backward: -> [grad1 (B,n,3), grad2 (B,m,3)]; with lengths, rows of the padding are 0."""
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    grad_cost = grad_cost.contiguous()
    with torch.cuda.device(xyz1.device):
        if lengths1 is None and lengths2 is None:
            _lib.check(_lib.load().pdr_matchcost_grad(grad_cost.data_ptr(), xyz1.data_ptr(),
                                                      xyz2.data_ptr(), match.data_ptr(), B, n, m, g1.data_ptr(),
                                                      g2.data_ptr(), _stream()), "matchcost_backward")
        else:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            _lib.check(_lib.load().pdr_matchcost_grad_ragged(grad_cost.data_ptr(), xyz1.data_ptr(), xyz2.data_ptr(),
                                                             _ptr(l1), _ptr(l2), match.data_ptr(), B, n, m,
                                                             g1.data_ptr(), g2.data_ptr(), _stream()),
                       "matchcost_backward")
    return [g1, g2]


def emd_cost_fused(xyz1, xyz2, lengths1=None, lengths2=None, return_workspace=False, workspace=None):
    """matchcost(approxmatch(xyz1, xyz2)) without the match matrix (no autograd).  return_workspace: -> (cost, temp),
    temp the call's workspace holding the per-level factors emd_cost_backward reads (layout private).  workspace: a
    float32 tensor of at least pdr_emd_workspace_bytes(B, n, m) bytes to use instead of allocating one (a caller that
    walks many batches, set_metrics.pairwise_emd, allocates it once)."""
    _check(xyz1, "xyz1"), _check(xyz2, "xyz2")
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    lib = _lib.load()
    cost = torch.empty((B,), dtype=torch.float32, device=xyz1.device)
    if workspace is None:
        temp = torch.empty((lib.pdr_emd_workspace_bytes(B, n, m) // 4,), dtype=torch.float32, device=xyz1.device)
    else:
        temp = workspace
        if (temp.dtype != torch.float32 or temp.device != xyz1.device or not temp.is_contiguous()
                or temp.numel() * 4 < lib.pdr_emd_workspace_bytes(B, n, m)):
            raise RuntimeError("workspace must be a contiguous float32 tensor on the clouds' device of at least "
                               "pdr_emd_workspace_bytes(B, n, m) bytes")
    with torch.cuda.device(xyz1.device):
        if lengths1 is None and lengths2 is None:
            _lib.check(lib.pdr_emd_cost(xyz1.data_ptr(), xyz2.data_ptr(), B, n, m, cost.data_ptr(), temp.data_ptr(),
                                        _stream()), "emd_cost")
        else:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            _lib.check(lib.pdr_emd_cost_ragged(xyz1.data_ptr(), xyz2.data_ptr(), _ptr(l1), _ptr(l2), B, n, m,
                                               cost.data_ptr(), temp.data_ptr(), _stream()), "emd_cost")
    return (cost, temp) if return_workspace else cost


def emd_cost_backward(grad_cost, xyz1, xyz2, workspace, lengths1=None, lengths2=None):
    """matchcost_backward on the match of approxmatch_forward(xyz1, xyz2) without that matrix: `workspace` is what
    emd_cost_fused(xyz1, xyz2, lengths1, lengths2, return_workspace=True) returned for the same clouds and lengths
    (read only).  -> [grad1 (B,n,3), grad2 (B,m,3)]; with lengths, rows of the padding are 0."""
    _check(xyz1, "xyz1"), _check(xyz2, "xyz2")
    xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    lib = _lib.load()
    if (workspace.dtype != torch.float32 or workspace.device != xyz1.device or not workspace.is_contiguous()
            or workspace.numel() * 4 < lib.pdr_emd_workspace_bytes(B, n, m)):
        raise RuntimeError("workspace is not the one emd_cost_fused(return_workspace=True) returns for these sizes")
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    grad_cost = grad_cost.contiguous()
    with torch.cuda.device(xyz1.device):
        if lengths1 is None and lengths2 is None:
            _lib.check(lib.pdr_emd_cost_grad(grad_cost.data_ptr(), xyz1.data_ptr(), xyz2.data_ptr(),
                                             workspace.data_ptr(), B, n, m, g1.data_ptr(), g2.data_ptr(), _stream()),
                       "emd_cost_backward")
        else:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            _lib.check(lib.pdr_emd_cost_grad_ragged(grad_cost.data_ptr(), xyz1.data_ptr(), xyz2.data_ptr(), _ptr(l1),
                                                    _ptr(l2), workspace.data_ptr(), B, n, m, g1.data_ptr(),
                                                    g2.data_ptr(), _stream()), "emd_cost_backward")
    return [g1, g2]


def _pair_denominator(xyz1, xyz2, lengths1, lengths2):
    """max(n_b, m_b) per pair as float32 on the device (lengths clamped like the kernels clamp them, None = full),
    at least 1 so that an empty pair, whose cost is 0, stays 0."""
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    full = lambda v: torch.full((B,), v, dtype=torch.int64, device=xyz1.device)
    l1 = full(n) if lengths1 is None else lengths1.clamp(0, n)
    l2 = full(m) if lengths2 is None else lengths2.clamp(0, m)
    return torch.maximum(l1, l2).clamp(min=1).to(torch.float32)


class EarthMoverDistanceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, return_match=False, lengths1=None, lengths2=None):
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        assert xyz1.is_cuda and xyz2.is_cuda, "Only support cuda currently."
        needs_grad = any(ctx.needs_input_grad[:2])
        ctx.ragged = lengths1 is not None or lengths2 is not None
        if ctx.ragged:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            # tensor / Python number (the dense line below) multiplies by the number's float32 reciprocal; the same two
            # roundings here, so a full pair gets the dense bits
            scale = torch.reciprocal(_pair_denominator(xyz1, xyz2, l1, l2))
            if not return_match and not needs_grad:
                return emd_cost_fused(xyz1, xyz2, l1, l2) * scale
            match = approxmatch_forward(xyz1, xyz2, l1, l2)
            cost = matchcost_forward(xyz1, xyz2, match, l1, l2) * scale
            ctx.lengths = (l1, l2)
            ctx.save_for_backward(xyz1, xyz2, match)
            return (cost, match) if return_match else cost
        denom = max(xyz1.shape[1], xyz2.shape[1])
        if not return_match and not needs_grad:
            return emd_cost_fused(xyz1, xyz2) / denom
        match = approxmatch_forward(xyz1, xyz2)
        cost = matchcost_forward(xyz1, xyz2, match) / denom
        ctx.save_for_backward(xyz1, xyz2, match)
        return (cost, match) if return_match else cost

    @staticmethod
    def backward(ctx, grad_cost, *unused):
        xyz1, xyz2, match = ctx.saved_tensors
        if ctx.ragged:
            g1, g2 = matchcost_backward(grad_cost.contiguous(), xyz1, xyz2, match, *ctx.lengths)
            return g1, g2, None, None, None
        g1, g2 = matchcost_backward(grad_cost.contiguous(), xyz1, xyz2, match)
        return g1, g2, None


class EarthMoverDistanceMatrixFreeFunction(torch.autograd.Function):
    """The fused cost with a gradient: saves the clouds, the lengths and the workspace, never a (B,m,n) tensor."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, lengths1=None, lengths2=None):
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        assert xyz1.is_cuda and xyz2.is_cuda, "Only support cuda currently."
        if lengths1 is None and lengths2 is None:
            l1 = l2 = None
            cost, temp = emd_cost_fused(xyz1, xyz2, return_workspace=True)
            cost = cost / max(xyz1.shape[1], xyz2.shape[1])
        else:
            l1, l2 = _lengths(lengths1, xyz1, "lengths1"), _lengths(lengths2, xyz2, "lengths2")
            cost, temp = emd_cost_fused(xyz1, xyz2, l1, l2, return_workspace=True)
            cost = cost * torch.reciprocal(_pair_denominator(xyz1, xyz2, l1, l2))
        ctx.lengths = (l1, l2)
        ctx.save_for_backward(xyz1, xyz2, temp)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        xyz1, xyz2, temp = ctx.saved_tensors
        g1, g2 = emd_cost_backward(grad_cost.contiguous(), xyz1, xyz2, temp, *ctx.lengths)
        return g1, g2, None, None


def _prep(xyz1, xyz2, transpose):
    if xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    if transpose:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    return xyz1, xyz2


def earth_mover_distance(xyz1, xyz2, transpose=False, return_match=False, lengths1=None, lengths2=None,
                         matrix_free=False):
    """xyz1 (b,n,3), xyz2 (b,m,3) [or (b,3,n) with transpose] -> cost (b) [, match (b,m,n)].
    lengths1 / lengths2 (b,) integer tensors: pair i is xyz1[i, :lengths1[i]], xyz2[i, :lengths2[i]].
    matrix_free: differentiable without the (b,m,n) match in forward or backward (module docstring); the cost is the
    one the call without a gradient returns.  There is no match to return: with return_match it raises ValueError."""
    if matrix_free and return_match:
        raise ValueError("matrix_free=True builds no match matrix: it cannot be combined with return_match=True")
    xyz1, xyz2 = _prep(xyz1, xyz2, transpose)
    if matrix_free:
        return EarthMoverDistanceMatrixFreeFunction.apply(xyz1, xyz2, lengths1, lengths2)
    if lengths1 is None and lengths2 is None:
        return EarthMoverDistanceFunction.apply(xyz1, xyz2, bool(return_match))
    return EarthMoverDistanceFunction.apply(xyz1, xyz2, bool(return_match), lengths1, lengths2)


class EMD_distance(nn.Module):
    def forward(self, xyz1, xyz2, transpose=False, return_match=False, lengths1=None, lengths2=None,
                matrix_free=False):
        return earth_mover_distance(xyz1, xyz2, transpose=transpose, return_match=return_match, lengths1=lengths1,
                                    lengths2=lengths2, matrix_free=matrix_free)
