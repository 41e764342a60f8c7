"""Chamfer distance / F-score -- same surface as reference pointnet2/chamfer_loss_new.py
(chamfer_distance :67-217, fscore :219-232, calc_cd :234-245, Chamfer_F1 :247-256).

The two nearest-neighbour searches (pytorch3d knn_points K=1 in the reference,
:149-150) run on libpdr_hip.so: ONE launch for both directions (pdr_chamfer_nn) on the
hot path = dense clouds of equal length per batch without gradient (what
completion_eval.py feeds); two differentiable knn_points calls when a gradient is
needed (train.py:518).  Ragged `x_lengths` / `y_lengths` take the same two routes: the
kernels read the per-cloud lengths on the device (pdr_chamfer_nn_ragged, one launch;
length-aware knn_points with a gradient), reference :121-128, 152-155 semantics: padded
points are not candidates and contribute 0.  pytorch3d `Pointclouds` objects are rejected.
All distances are SQUARED; cd_p takes the square root per point before the mean;
the F-score threshold is applied to squared distances.
fscore / calc_cd / Chamfer_F1 take the lengths too: precision, recall and the means are over each cloud's valid
points, and a cloud of length 0 yields 0 for every metric.
calc_cd_fused / ChamferLoss (not in the reference) are calc_cd's cd_p / cd_t as a training loss on kernels of their own
(pdr_chamfer_loss, pdr_chamfer_loss_grad): three launches for forward plus backward, bit-reproducible.
"""
from typing import Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..pointnet2_ops import _ext


def _validate_chamfer_reduction_inputs(batch_reduction: Union[str, None], point_reduction: Union[str, None]):
    if batch_reduction is not None and batch_reduction not in ["mean", "sum"]:
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction is not None and point_reduction not in ["mean", "sum"]:
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if point_reduction is None and batch_reduction is not None:
        raise ValueError('batch_reduction must be set to None if point_reduction is already None')


def _dense(points, lengths, normals, name):
    if not torch.is_tensor(points):
        raise ValueError("The input pointclouds should be torch.Tensor of shape (minibatch, num_points, 3) "
                         "(pytorch3d Pointclouds objects are not supported by this build).")
    if points.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    if lengths is not None:
        if lengths.ndim != 1 or lengths.shape[0] != points.shape[0]:
            raise ValueError("Expected lengths to be of shape (N,)")
    if normals is not None and normals.ndim != 3:
        raise ValueError("Expected normals to be of shape (N, P, 3")
    if lengths is None:
        lengths = torch.full((points.shape[0],), points.shape[1], dtype=torch.int64, device=points.device)
    return points, lengths, normals


def _nearest(a, b):
    d, i, _ = _ext.knn_points(a.contiguous(), b.contiguous(), 1)
    return d[..., 0], i[..., 0]


def _nearest_both(x, y):
    """(cham_x, idx_x, cham_y, idx_y) of dense clouds: one launch without autograd, two differentiable searches
    otherwise."""
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _nearest(x, y) + _nearest(y, x)
    return _ext.chamfer_nn(x.contiguous(), y.contiguous())


def _nearest_lengths(a, la, b, lb):
    """Differentiable search of a[n, :la[n]] in b[n, :lb[n]]: padded queries and queries of an empty cloud come back
    as (0, -1); index 0 instead keeps the normals gather in range (those entries are masked, or have no neighbour)."""
    d, i, _ = _ext.knn_points(a.contiguous(), b.contiguous(), 1, lengths1=la, lengths2=lb)
    return d[..., 0], i[..., 0].clamp(min=0)


def _nearest_both_ragged(x, x_lengths, y, y_lengths):
    """(cham_x, idx_x, cham_y, idx_y) of padded clouds, sample n being x[n, :x_lengths[n]] and y[n, :y_lengths[n]]:
    padded queries get distance 0 / index 0 (what the reference's masking leaves, :152-155).  The kernels read the
    lengths on the device: one launch without autograd, two differentiable searches otherwise."""
    if not x.is_cuda:
        return _nearest_per_sample(x, x_lengths, y, y_lengths) + _nearest_per_sample(y, y_lengths, x, x_lengths)
    lx = x_lengths.to(device=x.device, dtype=torch.int64).contiguous()
    ly = y_lengths.to(device=y.device, dtype=torch.int64).contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _nearest_lengths(x, lx, y, ly) + _nearest_lengths(y, ly, x, lx)
    return _ext.chamfer_nn(x.contiguous(), y.contiguous(), lx, ly)


def _nearest_per_sample(a, la, b, lb):
    """Tensors that are not on a GPU: `_ext` has no implementation for them, so this is reached only with a backend
    substituted for it that knows the dense signatures alone (tests/oracle_backend.py); one dense search per sample
    over the slices, same results."""
    d = a.new_zeros(a.shape[:2])
    i = torch.zeros(a.shape[:2], dtype=torch.int64, device=a.device)
    for n in range(a.shape[0]):
        na, nb = int(la[n]), int(lb[n])
        if na == 0 or nb == 0:
            continue
        dn, jn = _nearest(a[n:n + 1, :na], b[n:n + 1, :nb])
        d[n, :na], i[n, :na] = dn[0], jn[0]
    return d, i


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction: Union[str, None] = "mean", point_reduction: Union[str, None] = "mean"):
    """Returns (cham_x, cham_y, cham_normals): squared distance from every x point to its
    nearest y point and vice versa, reduced as requested; (N,P1)/(N,P2) when both reductions are None."""
    _validate_chamfer_reduction_inputs(batch_reduction, point_reduction)
    x, x_lengths, x_normals = _dense(x, x_lengths, x_normals, "x")
    y, y_lengths, y_normals = _dense(y, y_lengths, y_normals, "y")
    with_normals = x_normals is not None and y_normals is not None
    N, P1, D = x.shape
    if y.shape[0] != N or y.shape[2] != D:
        raise ValueError("y does not have the correct shape.")
    if weights is not None:
        if weights.size(0) != N:
            raise ValueError("weights must be of shape (N,).")
        if not (weights >= 0).all():
            raise ValueError("weights cannot be negative.")
        if weights.sum() == 0.0:
            z = (x.sum((1, 2)) * weights.view(N, 1).squeeze(1))
            if batch_reduction in ["mean", "sum"]:
                return z.sum() * 0.0, z.sum() * 0.0
            return z * 0.0, z * 0.0

    P2 = y.shape[1]
    ragged = bool((x_lengths != P1).any()) or bool((y_lengths != P2).any())
    if ragged:
        if bool((x_lengths > P1).any()) or bool((y_lengths > P2).any()):
            raise ValueError("lengths exceed the padded size")
        cham_x, idx_x, cham_y, idx_y = _nearest_both_ragged(x, x_lengths, y, y_lengths)
        x_mask = torch.arange(P1, device=x.device)[None] >= x_lengths[:, None]
        y_mask = torch.arange(P2, device=y.device)[None] >= y_lengths[:, None]
    else:
        cham_x, idx_x, cham_y, idx_y = _nearest_both(x, y)
    norm_x = norm_y = x.new_zeros(())
    if weights is not None:
        cham_x = cham_x * weights.view(N, 1)
        cham_y = cham_y * weights.view(N, 1)
    if with_normals:
        near_x = y_normals.gather(1, idx_x.unsqueeze(-1).expand(-1, -1, y_normals.shape[2]))
        near_y = x_normals.gather(1, idx_y.unsqueeze(-1).expand(-1, -1, x_normals.shape[2]))
        norm_x = 1 - torch.abs(F.cosine_similarity(x_normals, near_x, dim=2, eps=1e-6))
        norm_y = 1 - torch.abs(F.cosine_similarity(y_normals, near_y, dim=2, eps=1e-6))
        if ragged:
            norm_x = norm_x.masked_fill(x_mask, 0.0)
            norm_y = norm_y.masked_fill(y_mask, 0.0)
        if weights is not None:
            norm_x = norm_x * weights.view(N, 1)
            norm_y = norm_y * weights.view(N, 1)

    if point_reduction is not None:
        cham_x, cham_y = cham_x.sum(1), cham_y.sum(1)
        if with_normals:
            norm_x, norm_y = norm_x.sum(1), norm_y.sum(1)
        if point_reduction == "mean":
            cham_x, cham_y = cham_x / x_lengths, cham_y / y_lengths
            if with_normals:
                norm_x, norm_y = norm_x / x_lengths, norm_y / y_lengths
    if batch_reduction is not None:
        cham_x, cham_y = cham_x.sum(), cham_y.sum()
        if with_normals:
            norm_x, norm_y = norm_x.sum(), norm_y.sum()
        if batch_reduction == "mean":
            div = weights.sum() if weights is not None else N
            cham_x, cham_y = cham_x / div, cham_y / div
            if with_normals:
                norm_x, norm_y = norm_x / div, norm_y / div
    return cham_x, cham_y, (norm_x + norm_y if with_normals else None)


def _valid_mean(v, lengths):
    """Mean of every row of v (B,P) over its first lengths[b] entries (None: all P); 0 for a length of 0.  Entries
    beyond the length are not read into the sum, whatever they hold."""
    if lengths is None:
        return v.mean(1)
    lengths = lengths.to(v.device).clamp(0, v.shape[1])
    valid = torch.arange(v.shape[1], device=v.device)[None] < lengths[:, None]
    return torch.where(valid, v, torch.zeros_like(v)).sum(1) / lengths.clamp(min=1).to(v.dtype)


def fscore(dist1, dist2, threshold=0.0001, lengths1=None, lengths2=None):
    """F-score of two (B,P) SQUARED nearest-neighbour distance maps at `threshold` (also squared).
    lengths1 / lengths2 (B,): precision and recall over the first lengths[b] points of each map only (a padded point's
    distance of 0 is not a hit); a cloud of length 0 has precision / recall / F-score 0."""
    if lengths1 is None and lengths2 is None:
        p1 = torch.mean((dist1 < threshold).float(), dim=1)
        p2 = torch.mean((dist2 < threshold).float(), dim=1)
    else:
        p1 = _valid_mean((dist1 < threshold).float(), lengths1)
        p2 = _valid_mean((dist2 < threshold).float(), lengths2)
    f = 2 * p1 * p2 / (p1 + p2)
    f[torch.isnan(f)] = 0
    return f, p1, p2


def calc_cd(output, gt, calc_f1=False, f1_threshold=0.0001, output_lengths=None, gt_lengths=None):
    """cd_p = (mean sqrt d1 + mean sqrt d2)/2, cd_t = mean d1 + mean d2, with d1 = gt->output.
    output_lengths / gt_lengths (B,): sample b is output[b, :output_lengths[b]] against gt[b, :gt_lengths[b]]; the
    means are over the valid points, and a sample with an empty cloud gives 0 for every metric."""
    if output_lengths is not None or gt_lengths is not None:
        on = lambda l, ref: None if l is None else l.to(device=ref.device, dtype=torch.int64)
        output_lengths, gt_lengths = on(output_lengths, output), on(gt_lengths, gt)
        d1, d2, _ = chamfer_distance(gt, output, x_lengths=gt_lengths, y_lengths=output_lengths, batch_reduction=None,
                                     point_reduction=None)
        cd_p = (_valid_mean(torch.sqrt(d1), gt_lengths) + _valid_mean(torch.sqrt(d2), output_lengths)) / 2
        cd_t = _valid_mean(d1, gt_lengths) + _valid_mean(d2, output_lengths)
        if calc_f1:
            f1, _, _ = fscore(d1, d2, threshold=f1_threshold, lengths1=gt_lengths, lengths2=output_lengths)
            return cd_p, cd_t, f1
        return cd_p, cd_t
    d1, d2, _ = chamfer_distance(gt, output, batch_reduction=None, point_reduction=None)
    cd_p = (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2
    cd_t = d1.mean(1) + d2.mean(1)
    if calc_f1:
        f1, _, _ = fscore(d1, d2, threshold=f1_threshold)
        return cd_p, cd_t, f1
    return cd_p, cd_t


def calc_cd_fused(output, gt, output_lengths=None, gt_lengths=None):
    """(cd_p, cd_t), each (B,), with calc_cd's definitions and argument order (d1 = gt->output) as a TRAINING LOSS:
    differentiable w.r.t. both clouds, three launches for forward plus backward (pdr_chamfer_loss,
    pdr_chamfer_loss_grad) and bit-reproducible without any switch.  The means are over the valid points; a sample with
    an empty cloud gives 0.  Where calc_cd's cd_p has a NaN gradient -- a coincident pair -- this one's sqrt term is 0.
    train.py:518 becomes calc_cd_fused(X, refined_X)[loss_idx].mean()."""
    if not (torch.is_tensor(output) and torch.is_tensor(gt)) or output.ndim != 3 or gt.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, 3)")
    if output.shape[0] != gt.shape[0]:
        raise ValueError("output and gt must hold the same number of clouds")
    on = lambda l, ref: None if l is None else l.to(device=ref.device, dtype=torch.int64).contiguous()
    output_lengths, gt_lengths = on(output_lengths, output), on(gt_lengths, gt)
    sums = _ext.chamfer_loss_sums(gt.contiguous(), output.contiguous(), gt_lengths, output_lengths)
    count = lambda l, ref: float(ref.shape[1]) if l is None else l.clamp(0, ref.shape[1]).clamp(min=1).to(sums.dtype)
    n_gt, n_out = count(gt_lengths, gt), count(output_lengths, output)
    cd_p = (sums[:, 2] / n_gt + sums[:, 3] / n_out) / 2
    cd_t = sums[:, 0] / n_gt + sums[:, 1] / n_out
    return cd_p, cd_t


class ChamferLoss(nn.Module):
    """calc_cd_fused as a module: `loss_type` 'cd_t' | 'cd_p' picks the metric, `weights` (B,) scales each cloud's
    value, `reduction` 'mean' | 'sum' | None reduces over the batch ('mean' divides by the sum of the weights when
    they are given, as chamfer_distance does)."""

    def __init__(self, loss_type="cd_t", reduction="mean"):
        super().__init__()
        if loss_type not in ("cd_t", "cd_p"):
            raise ValueError('loss_type must be one of ["cd_t", "cd_p"]')
        if reduction is not None and reduction not in ("mean", "sum"):
            raise ValueError('reduction must be one of ["mean", "sum"] or None')
        self.loss_type, self.reduction = loss_type, reduction

    def forward(self, output, gt, output_lengths=None, gt_lengths=None, weights=None):
        if weights is not None:
            if weights.ndim != 1 or weights.size(0) != output.shape[0]:
                raise ValueError("weights must be of shape (N,).")
            if not (weights >= 0).all():
                raise ValueError("weights cannot be negative.")
        cd_p, cd_t = calc_cd_fused(output, gt, output_lengths, gt_lengths)
        loss = cd_t if self.loss_type == "cd_t" else cd_p
        if weights is not None:
            loss = loss * weights.to(loss)
        if self.reduction is None:
            return loss
        if self.reduction == "sum":
            return loss.sum()
        return loss.sum() / (weights.to(loss).sum() if weights is not None else loss.shape[0])


class Chamfer_F1(nn.Module):
    def __init__(self, f1_threshold=0.0001):
        super().__init__()
        self.f1_threshold = f1_threshold

    def forward(self, xyz1, xyz2, lengths1=None, lengths2=None):
        return calc_cd(xyz1, xyz2, calc_f1=True, f1_threshold=self.f1_threshold, output_lengths=lengths1,
                       gt_lengths=lengths2)
