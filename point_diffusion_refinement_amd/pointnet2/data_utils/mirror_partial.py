"""Mirror-and-concat preprocessing of partial clouds -- same surface as reference
pointnet2/data_utils/mirror_partial.py (mirror :5-9, down_sample_points :11-20, mirror_and_concat :22-38),
the producer of the (B, 3072, 4) condition clouds of the DDPM configs
(mvp_dataloader/generate_mirrored_partial.py:44).

A partial cloud is reflected about a coordinate plane, the copy is tagged with a 4th channel (-1; originals +1),
both are concatenated and farthest-point-sampled (on xyz only) down to the requested sizes.  FPS and the row
gather run on libpdr_hip.so; tensors stay on the input's device (the reference moves them with `.cuda()`).

Beyond the reference: every function takes `lengths` for PADDED batches of clouds with different point counts (sensor
crops, KITTI- or ScanNet-style partials); without it each runs exactly the dense code.
"""
import torch

from ...pointnet2_ops import _ext, pointnet2_utils


def mirror(partial, axis=1):
    """(B,N,3) -> copy with coordinate `axis` negated."""
    sign = torch.ones(partial.shape[-1], dtype=partial.dtype, device=partial.device)
    sign[axis] = -1
    return partial * sign


def tagged_concat(partial, axis, lengths):
    """(B,N,3) padded clouds, lengths (B,) -> (B,2N,4): cloud b's 2 L_b valid rows first -- its L_b originals (tag +1),
    then their mirror images (tag -1) --, every padding row 0.  Pure torch, any device; rows of `partial` at or beyond
    a length are never used for their value."""
    B, N, _ = partial.shape
    L = lengths.to(device=partial.device, dtype=torch.int64).clamp(0, N).view(B, 1)
    k = torch.arange(2 * N, device=partial.device).view(1, 2 * N)
    mirrored = (k >= L) & (k < 2 * L)
    valid = (k < 2 * L).unsqueeze(-1)
    src = torch.where(mirrored, k - L, k).clamp(max=N - 1)
    pts = partial.gather(1, src.unsqueeze(-1).expand(B, 2 * N, 3))
    pts = torch.where(mirrored.unsqueeze(-1), mirror(pts, axis), pts)
    one = torch.ones(B, 2 * N, 1, dtype=partial.dtype, device=partial.device)
    both = torch.cat([pts, torch.where(mirrored.unsqueeze(-1), -one, one)], 2)
    return torch.where(valid, both, torch.zeros_like(both)).contiguous()


def down_sample_points(xyz, npoints, lengths=None):
    """(B,N,4) -> (B,npoints,4): FPS on the first three channels, all channels of the picked rows.  With `lengths`
    ((B,) int64 on the device) only cloud b's first lengths[b] rows are sampled; a cloud of length 0 gives rows of 0."""
    if lengths is not None:
        idx = pointnet2_utils.furthest_point_sample_ragged(xyz[:, :, 0:3].contiguous(), npoints, lengths)
        picked = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), idx.clamp(min=0))
        picked = torch.where((idx >= 0).unsqueeze(1), picked, torch.zeros_like(picked))
        return picked.transpose(1, 2).contiguous()
    idx = pointnet2_utils.furthest_point_sample(xyz[:, :, 0:3].contiguous(), npoints)
    picked = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), idx)      # (B,4,npoints)
    return picked.transpose(1, 2).contiguous()


def mirror_and_concat(partial, axis=2, num_points=(2048, 3072), lengths=None):
    """(B,N,3) -> ((B,2N,4) tagged concat, then one (B,n,4) down-sampled cloud per entry of num_points).

    With `lengths` ((B,) int64 on the device; full lengths included) `partial` is a padded batch: the concat is
    `tagged_concat`, and the down-sampled clouds come from ONE length-aware FPS launch to max(num_points) that reads
    the mirrored half on the fly and writes the picked rows itself -- FPS is prefix-consistent, so the first n picks
    are the run to n.  Full lengths give the bits of the dense path."""
    if lengths is not None:
        axis = axis % 3
        both = tagged_concat(partial, axis, lengths)
        _, rows = _ext.furthest_point_sampling_ragged(partial.contiguous(), max(num_points), lengths=lengths,
                                                      mirror_axis=axis, return_rows=True)
        return (both,) + tuple(rows[:, :n].contiguous() for n in num_points)
    B, N, _ = partial.shape
    tag = torch.ones(B, N, 1, dtype=partial.dtype, device=partial.device)
    both = torch.cat([torch.cat([partial, tag], 2), torch.cat([mirror(partial, axis), -tag], 2)], 1).contiguous()
    return (both,) + tuple(down_sample_points(both, n) for n in num_points)
