"""Python surface of the point ops -- same names, signatures and return tuples as
the reference's pointnet2_ops/pointnet2_utils.py, running on libpdr_hip.so.

    furthest_point_sample, gather_operation, three_nn, three_interpolate,
    grouping_operation, ball_query           (pointnet2_utils.py:93,129,164,219,268,304)
    QueryAndGroup, GroupAll, group_knn       (:307,441,487)
    count_to_mask, average_feature           (:36,46)
    attention_pool                           (attention.py:71-77 as one op: masked softmax over K and the weighted
                                              sum of the values, with a one-launch backward that saves no weights)
    query_and_group, knn_and_group           (what QueryAndGroup / group_knn do after their neighbour search, each as
                                              one op with an order-fixed backward; behind set_fused_grouping /
                                              set_fused_knn_grouping, default off)

kNN comes from this package's own `_ext.knn_points` (the reference imports
pytorch3d.ops.knn, :7).  Autograd: FPS / ball_query / three_nn are
non-differentiable as in the reference; gather / group / three_interpolate have
backward kernels -- the atomic ones, or, under `_ext.set_deterministic` /
`torch.use_deterministic_algorithms(True)`, the order-fixed `*_grad_det` ones.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import _ext


def count_to_mask(count, K):
    """(B,npoint) counts -> bool mask (B,npoint,K): slot k valid iff k < count."""
    ar = torch.arange(K, device=count.device, dtype=count.dtype)
    return ar.view(1, 1, K) < count.unsqueeze(-1)


def average_feature(feature, count, K):
    """Masked mean over the neighbour axis. feature (B,C,npoint,K); count (B,npoint) or 'all'."""
    if isinstance(count, str) and count == 'all':
        return F.avg_pool2d(feature, kernel_size=[1, feature.size(3)]).squeeze(-1)
    count = torch.clamp(count, min=1)
    mask = count_to_mask(count, K).unsqueeze(1)
    return (feature * mask).sum(dim=-1) / count.unsqueeze(1)


class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        out = _ext.furthest_point_sampling(xyz, npoint)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ()


furthest_point_sample = FurthestPointSampling.apply


class FurthestPointSamplingRagged(Function):
    @staticmethod
    def forward(ctx, xyz, npoint, lengths):
        out = _ext.furthest_point_sampling_ragged(xyz, npoint, lengths=lengths)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ()


# (B,N,3) padded clouds, npoint, lengths (B,) int64 or None -> (B,npoint) i32: FPS of each cloud's first lengths[b]
# rows (pytorch3d's sample_farthest_points(lengths=...) with this library's tie order); a cloud of length 0 gets -1
furthest_point_sample_ragged = FurthestPointSamplingRagged.apply


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.n = features.size(2)
        return _ext.gather_points(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        grad = _ext.gather_points_grad_det if _ext.is_deterministic() else _ext.gather_points_grad
        return grad(grad_out.contiguous(), idx, ctx.n), None


gather_operation = GatherOperation.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        dist2, idx = _ext.three_nn(unknown, known)
        dist = torch.sqrt(dist2)  # reference returns the L2 distance, not its square (:152-153)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, grad_dist, grad_idx):
        return ()


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        ctx.save_for_backward(idx, weight)
        ctx.m = features.size(2)
        return _ext.three_interpolate(features, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        grad = _ext.three_interpolate_grad_det if _ext.is_deterministic() else _ext.three_interpolate_grad
        g = grad(grad_out.contiguous(), idx, weight, ctx.m)
        return g, torch.zeros_like(idx), torch.zeros_like(weight)


three_interpolate = ThreeInterpolate.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.n = features.size(2)
        return _ext.group_points(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        grad = _ext.group_points_grad_det if _ext.is_deterministic() else _ext.group_points_grad
        return grad(grad_out.contiguous(), idx, ctx.n), torch.zeros_like(idx)


grouping_operation = GroupingOperation.apply


class AttentionPool(Function):
    """scores, values (B,C,N,K) f32, count (B,N) i32 / None / 'all' -> (B,C,N): _ext.attention_pool; the backward
    recomputes the softmax from the saved inputs (no weight tensor is kept) and is order-fixed."""

    @staticmethod
    def forward(ctx, scores, values, count):
        if isinstance(count, torch.Tensor):
            ctx.save_for_backward(scores, values, count)
        else:
            ctx.save_for_backward(scores, values)
        return _ext.attention_pool(scores, values, count)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        scores, values = ctx.saved_tensors[:2]
        count = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        need_s, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_s or need_v):
            return None, None, None
        gs, gv = _ext.attention_pool_grad(scores, values, count, grad_out.contiguous().float(), need_s, need_v)
        return gs, gv, None                                     # count (integer) is not differentiable


attention_pool = AttentionPool.apply


class GroupNormAct(Function):
    """act(MyGroupNorm(x)): _ext.group_norm_act.  Saves x, weight, bias and the (B, G) mean / rstd -- never y; the
    backward recomputes the normalised values from them and is order-fixed."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, act):
        y, mean, rstd = _ext.group_norm_act(x, weight, bias, num_groups, eps, act)
        ctx.num_groups, ctx.act, ctx.affine = num_groups, act, weight is not None
        if ctx.affine:
            ctx.save_for_backward(x, mean, rstd, weight, bias)
        else:
            ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd = ctx.saved_tensors[:3]
        weight, bias = ctx.saved_tensors[3:] if ctx.affine else (None, None)
        need_x = ctx.needs_input_grad[0]
        need_w, need_b = (ctx.needs_input_grad[1], ctx.needs_input_grad[2]) if ctx.affine else (False, False)
        if not (need_x or need_w or need_b):
            return None, None, None, None, None, None
        gx, gw, gb = _ext.group_norm_act_grad(x, weight, bias, mean, rstd, grad_y.contiguous().float(), ctx.num_groups,
                                              ctx.act, need_x, need_w, need_b)
        return gx, gw, gb, None, None, None


def group_norm_act(x, weight, bias, num_groups, eps=1e-5, act='none'):
    """x (B, C, ...) f32 on the GPU, weight / bias (C - C % num_groups) or both None -> act(MyGroupNorm(x)) as one
    differentiable op (pdr_group_norm_act / pdr_group_norm_act_grad); act 'none' | 'relu' | 'swish'.  The trailing
    C % num_groups channels are not normalised, the activation applies to every channel (attention.py:18-32)."""
    return GroupNormAct.apply(x.contiguous(), weight, bias, num_groups, eps, act)


class GroupNormActAdd(Function):
    """(act(MyGroupNorm(x)) + add[:, :, None]) + residual: _ext.group_norm_act_add.  Saves what GroupNormAct saves --
    x, weight, bias and the (B, G) mean / rstd -- and nothing of the output's size: the backward needs neither add nor
    residual.  The residual's gradient is grad_y itself; add's is its row sum, from the row kernel of the backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, add, residual, num_groups, eps, act):
        y, mean, rstd = _ext.group_norm_act_add(x, weight, bias, num_groups, eps, act, add, residual)
        ctx.num_groups, ctx.act, ctx.affine = num_groups, act, weight is not None
        if ctx.affine:
            ctx.save_for_backward(x, mean, rstd, weight, bias)
        else:
            ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd = ctx.saved_tensors[:3]
        weight, bias = ctx.saved_tensors[3:] if ctx.affine else (None, None)
        need_x, need_e, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        need_w, need_b = (ctx.needs_input_grad[1], ctx.needs_input_grad[2]) if ctx.affine else (False, False)
        grad_y = grad_y.contiguous().float()
        gx = gw = gb = ge = None
        if need_x or need_w or need_b or need_e:
            gx, gw, gb, ge = _ext.group_norm_act_add_grad(x, weight, bias, mean, rstd, grad_y, ctx.num_groups, ctx.act,
                                                          need_x, need_w, need_b, need_e)
        return gx, gw, gb, ge, (grad_y if need_r else None), None, None, None


def group_norm_act_add(x, weight, bias, num_groups, eps=1e-5, act='none', add=None, residual=None):
    """group_norm_act with the two adds Mlp_plus_t_emb makes behind a stack folded in, as one differentiable op
    (pdr_group_norm_act_add / pdr_group_norm_act_add_grad): add (B, C) or None is broadcast over the trailing
    dimensions, residual (x's shape) or None is added after it -- (act(MyGroupNorm(x)) + add[:, :, None]) + residual,
    the composition's order and roundings."""
    return GroupNormActAdd.apply(x.contiguous(), weight, bias, None if add is None else add.contiguous(),
                                 None if residual is None else residual.contiguous(), num_groups, eps, act)


class ReluGroupNorm(Function):
    """MyGroupNorm(relu([q over K | k])): _ext.relu_group_norm.  Saves q, k, weight, bias and the (B, G) mean / rstd --
    neither the cat nor y; the backward recomputes the normalised values from them and is order-fixed."""

    @staticmethod
    def forward(ctx, q, k, weight, bias, num_groups, eps):
        y, mean, rstd = _ext.relu_group_norm(q, k, weight, bias, num_groups, eps)
        ctx.num_groups, ctx.has_q, ctx.affine = num_groups, q is not None, weight is not None
        ctx.save_for_backward(*[t for t in (k, mean, rstd, q, weight, bias) if t is not None])
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        saved = list(ctx.saved_tensors)
        k, mean, rstd = saved[:3]
        q = saved[3] if ctx.has_q else None
        weight, bias = saved[-2:] if ctx.affine else (None, None)
        need_q = ctx.has_q and ctx.needs_input_grad[0]
        need_k = ctx.needs_input_grad[1]
        need_w, need_b = (ctx.needs_input_grad[2], ctx.needs_input_grad[3]) if ctx.affine else (False, False)
        if not (need_q or need_k or need_w or need_b):
            return None, None, None, None, None, None
        gq, gk, gw, gb = _ext.relu_group_norm_grad(q, k, weight, bias, mean, rstd, grad_y.contiguous().float(),
                                                   ctx.num_groups, need_q, need_k, need_w, need_b)
        return gq, gk, gw, gb, None, None


def relu_group_norm(k, weight, bias, num_groups, eps=1e-5, q=None):
    """k (B, C2, N, K) f32 on the GPU, q (B, C1, N) or None, weight / bias (C - C % num_groups) or both None,
    C = C1 + C2 -> MyGroupNorm(relu(cat([q expanded over K, k], 1))) (B, C, N, K) as one differentiable op
    (pdr_relu_group_norm_cf / pdr_relu_group_norm_cf_grad): the ReLU-then-norm links of AttentionModule.weight_conv,
    the first one without its expand and cat.  The trailing C % num_groups channels are not normalised."""
    return ReluGroupNorm.apply(None if q is None else q.contiguous(), k.contiguous(), weight, bias, num_groups, eps)


class ReluGroupNormConv(Function):
    """conv1x1(MyGroupNorm(relu([q over K | k]))): _ext.relu_group_norm_conv.  Saves q, k, the (B, G) mean / rstd and
    the parameters -- not the cat and not the normalised tensor, which never exists.  Backward: the weight gradient
    (normalised values recomputed; first, so that its workspace and the buffer below are never alive together), the
    input-gradient GEMM into a (B, C, N, K) buffer, then _ext.relu_group_norm_grad on the buffer, which is released
    before the gradients are returned; the GEMM is skipped when none of q / k / weight / bias needs a gradient.  All
    of it order-fixed."""

    @staticmethod
    def forward(ctx, q, k, weight, bias, conv_weight, conv_bias, num_groups, eps):
        out, mean, rstd = _ext.relu_group_norm_conv(q, k, weight, bias, num_groups, eps, conv_weight, conv_bias)
        ctx.num_groups, ctx.has_q, ctx.affine, ctx.has_cb = num_groups, q is not None, weight is not None, \
            conv_bias is not None
        ctx.save_for_backward(*[t for t in (k, mean, rstd, conv_weight, q, weight, bias) if t is not None])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        k, mean, rstd, conv_weight = saved[:4]
        q = saved[4] if ctx.has_q else None
        weight, bias = saved[-2:] if ctx.affine else (None, None)
        need = ctx.needs_input_grad
        need_q = ctx.has_q and need[0]
        need_k = need[1]
        need_w, need_b = (need[2], need[3]) if ctx.affine else (False, False)
        need_cw, need_cb = need[4], ctx.has_cb and need[5]
        grad_out = grad_out.contiguous().float()
        gq = gk = gw = gb = gcw = gcb = None
        if need_cw or need_cb:
            gcw, gcb = _ext.relu_group_norm_conv_grad_weight(q, k, weight, bias, mean, rstd, grad_out, ctx.num_groups,
                                                             need_cw, need_cb)
        if need_q or need_k or need_w or need_b:
            gxn = _ext.relu_group_norm_conv_grad_input(conv_weight, grad_out)
            gq, gk, gw, gb = _ext.relu_group_norm_grad(q, k, weight, bias, mean, rstd, gxn, ctx.num_groups, need_q,
                                                       need_k, need_w, need_b)
            del gxn
        return gq, gk, gw, gb, gcw, gcb, None, None


def relu_group_norm_conv(k, weight, bias, num_groups, eps, conv_weight, conv_bias, q=None):
    """k (B, C2, N, K) f32 on the GPU, q (B, C1, N) or None, weight / bias (C - C % num_groups) or both None,
    conv_weight (Cout, C) or (Cout, C, 1, 1), conv_bias (Cout) or None, C = C1 + C2 ->
    conv1x1(MyGroupNorm(relu(cat([q expanded over K, k], 1)))) (B, Cout, N, K) as one differentiable op
    (pdr_relu_group_norm_conv_cf and its two gradient calls, then pdr_relu_group_norm_cf_grad): a whole
    [ReLU, MyGroupNorm, Conv2d] link of AttentionModule.weight_conv without the cat and without the normalised tensor."""
    conv_weight = conv_weight.reshape(conv_weight.shape[0], -1).contiguous()
    return ReluGroupNormConv.apply(None if q is None else q.contiguous(), k.contiguous(), weight, bias, conv_weight,
                                   conv_bias, num_groups, eps)


class QueryGroup(Function):
    """xyz (B,n,3), new_xyz (B,m,3), features (B,C,n) | None, idx (B,m,K) i32, counts (B,m) i32 | None, flags ->
    (B, C + 3E, m, K): _ext.query_group.  Saves idx and counts only -- every output value is a copy or one difference
    of the inputs, so the backward needs none of them; it is order-fixed whatever set_deterministic says."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, idx, counts, flags):
        if counts is not None:
            ctx.save_for_backward(idx, counts)
        else:
            ctx.save_for_backward(idx)
        ctx.n, ctx.flags = xyz.shape[1], flags
        ctx.C = 0 if features is None else features.shape[1]
        return _ext.query_group(xyz, new_xyz, features, idx, counts, flags)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        idx = ctx.saved_tensors[0]
        counts = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        need_x, need_n = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_f = ctx.needs_input_grad[2] and ctx.C > 0
        if not (need_x or need_n or need_f):
            return None, None, None, None, None, None
        gf, gx, gn = _ext.query_group_grad(idx, counts, grad_out.contiguous().float(), ctx.n, ctx.C, ctx.flags,
                                           need_f, need_x, need_n)
        return gx, gn, gf, None, None, None


def query_and_group(xyz, new_xyz, features, idx, counts=None, use_xyz=True, include_abs_coordinate=False,
                    include_center_coordinate=False):
    """The part of QueryAndGroup.forward after the neighbour search as one differentiable op (pdr_query_group_cf /
    pdr_query_group_cf_grad): fp32 GPU tensors xyz (B,n,3), new_xyz (B,m,3), features (B,C,n) or None, idx (B,m,K)
    int32, counts (B,m) int32 or None -> (B, C + 3E, m, K), channels [features | relative | absolute | centre].  A
    `counts` tensor asks for the module's patch of empty balls: a query with counts <= 0 gets itself as every
    neighbour and all-zero features.  Without use_xyz the two include_* flags are ignored, as in the module."""
    flags = _ext.query_group_flags(use_xyz, include_abs_coordinate, include_center_coordinate)
    return QueryGroup.apply(xyz.contiguous(), new_xyz.contiguous(), None if features is None else features.contiguous(),
                            idx.contiguous(), None if counts is None else counts.contiguous(), flags)


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        # NOTE the native op takes the queries first (bindings: ball_query(new_xyz, xyz, r, ns))
        idx, counts = _ext.ball_query(new_xyz, xyz, radius, nsample)
        ctx.mark_non_differentiable(idx, counts)
        return idx, counts

    @staticmethod
    def backward(ctx, *grads):
        return ()


ball_query = BallQuery.apply


def knn_gather(x, idx):
    """x (B,M,C), idx (B,N,K) int64 -> (B,N,K,C) = x[b, idx[b,n,k], :]."""
    B, M, C = x.shape
    _, N, K = idx.shape
    flat = idx.reshape(B, N * K, 1).expand(-1, -1, C)
    return x.gather(1, flat).view(B, N, K, C)


class QueryAndGroup(nn.Module):
    """Neighbourhood grouping around `new_xyz` (radius ball or K nearest).

    Output channels: [grouped features | relative xyz | (absolute xyz) | (centre xyz)].
    With subset=False a query without any neighbour is given itself as its only
    neighbour with an all-zero feature (reference :376-386, 404-410).
    """

    def __init__(self, radius, nsample, use_xyz=True, include_abs_coordinate=False,
                 include_center_coordinate=False, neighbor_def='radius'):
        super().__init__()
        if neighbor_def not in ('radius', 'nn'):
            raise AssertionError('neighbor_def must be radius or nn')
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz
        self.include_abs_coordinate = include_abs_coordinate
        self.include_center_coordinate = include_center_coordinate
        self.neighbor_def = neighbor_def
        self.neighbor_stats = None
        self.neighbor_num_quantile = None
        self.quantile = torch.linspace(0, 1, 11)

    def _neighbours(self, xyz, new_xyz):
        if self.neighbor_def == 'radius':
            return ball_query(self.radius, self.nsample, xyz, new_xyz)
        k = min(self.nsample, xyz.shape[1])
        _, idx, _ = _ext.knn_points(new_xyz, xyz, k)
        idx = idx.int()
        counts = torch.ones(idx.shape[0], idx.shape[1], device=new_xyz.device) * k
        return idx, counts

    def forward(self, xyz, new_xyz, features=None, subset=True, record_neighbor_stats=False,
                return_counts=False):
        idx, counts = self._neighbours(xyz, new_xyz)
        radius_mode = self.neighbor_def == 'radius'
        if self._takes_fused_op(xyz, new_xyz, features, idx):
            patch_empty = (not subset) and radius_mode
            new_features = query_and_group(xyz, new_xyz, features, idx, counts if patch_empty else None, self.use_xyz,
                                           self.include_abs_coordinate, self.include_center_coordinate)
            return self._finish(new_features, counts, radius_mode, record_neighbor_stats, return_counts)
        centre = new_xyz.transpose(1, 2).unsqueeze(-1)                     # (B,3,np,1)
        abs_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx)  # (B,3,np,K)
        patch_empty = (not subset) and radius_mode
        if patch_empty:
            have = (counts > 0).float().unsqueeze(1).unsqueeze(-1).detach()
            none = 1 - have
            abs_xyz = have * abs_xyz + none * centre
        parts = [abs_xyz - centre]
        if self.include_abs_coordinate:
            parts.append(abs_xyz)
        if self.include_center_coordinate:
            parts.append(centre.expand(-1, -1, -1, abs_xyz.shape[3]))
        grouped_xyz = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

        if features is not None:
            grouped = grouping_operation(features, idx)
            if patch_empty:
                zero = torch.zeros(features.shape[1], device=features.device).view(1, -1, 1, 1)
                grouped = have * grouped + none * zero
            new_features = torch.cat([grouped, grouped_xyz], dim=1) if self.use_xyz else grouped
        else:
            if not self.use_xyz:
                raise AssertionError("Cannot have not features and not use xyz as a feature!")
            new_features = grouped_xyz
        return self._finish(new_features, counts, radius_mode, record_neighbor_stats, return_counts)

    def _takes_fused_op(self, xyz, new_xyz, features, idx):
        """set_fused_grouping(True), fp32 GPU tensors and a size pdr_query_group_cf takes.  (The flag is read directly
        and before anything else: with the switch off this path calls nothing.)"""
        if not _ext._fused_grouping:
            return False
        floats = [xyz, new_xyz] + ([] if features is None else [features])
        if not all(t.is_cuda and t.dtype == torch.float32 for t in floats) or idx.dtype != torch.int32:
            return False
        if features is None and not self.use_xyz:
            return False                                     # the composition raises its own error
        flags = _ext.query_group_flags(self.use_xyz, self.include_abs_coordinate, self.include_center_coordinate)
        C = 0 if features is None else features.shape[1]
        return _ext.query_group_supported(xyz.shape[0], xyz.shape[1], idx.shape[1], idx.shape[2], C, flags)

    def _finish(self, new_features, counts, radius_mode, record_neighbor_stats, return_counts):
        if record_neighbor_stats:
            with torch.no_grad():
                c = counts.float()
                self.neighbor_stats = torch.stack([c.min(), c.mean(), c.max()])
                self.neighbor_num_quantile = torch.quantile(c, self.quantile.to(c.device)).long()

        if return_counts:
            return new_features, ('all' if not radius_mode else counts)
        return new_features


class GroupAll(nn.Module):
    """Single group holding the whole cloud: (B, C(+3), 1, N)."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        gxyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return gxyz
        gfeat = features.unsqueeze(2)
        return torch.cat([gfeat, gxyz], dim=1) if self.use_xyz else gfeat


class KnnGroup(Function):
    """x (B,n1,3), y (B,n2,3), features (B,C,n2) | None, idx (B,n1,K) i32, dists (B,n1,K) f32 -> (B, C + 11, n1, K):
    _ext.knn_group_cf.  Saves x, y, idx and dists only -- no float tensor of output size; the backward recomputes the
    weights from dists and is order-fixed whatever set_deterministic says."""

    @staticmethod
    def forward(ctx, x, y, features, idx, dists):
        ctx.save_for_backward(x, y, idx, dists)
        ctx.C = 0 if features is None else features.shape[1]
        return _ext.knn_group_cf(x, y, features, idx, dists)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, y, idx, dists = ctx.saved_tensors
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_f = ctx.needs_input_grad[2] and ctx.C > 0
        if not (need_x or need_y or need_f):
            return None, None, None, None, None
        gf, gx, gy = _ext.knn_group_cf_grad(x, y, idx, dists, grad_out.contiguous().float(), ctx.C, need_f, need_x, need_y)
        return gx, gy, gf, None, None


def knn_and_group(x, y, features, idx, dists):
    """The part of group_knn(..., transpose=True) after the neighbour search as one differentiable op
    (pdr_knn_group_cf / pdr_knn_group_cf_grad): fp32 GPU tensors x (B,n1,3), y (B,n2,3), features (B,C,n2) or None,
    idx (B,n1,K) int32 and dists (B,n1,K) as `_ext.knn_group` returns them (no padding slot) -> (B, C + 11, n1, K)
    contiguous, channels [features | d2 | w | nn_abs | nn_rel | x].  `dists` is taken as the squared distance
    |x - y[idx]|^2 that the search computed: its gradient flows to x and y inside the op, not to `dists`."""
    return KnnGroup.apply(x.contiguous(), y.contiguous(), None if features is None else features.contiguous(),
                          idx.contiguous(), dists.detach().contiguous())


def _group_knn_takes_fused_op(x, y, features_at_y, K, transpose):
    """set_fused_knn_grouping(True), transpose=True, fp32 GPU tensors, K <= min(n2, 16) (pdr_knn_group's contract: no
    padding slot) and a size pdr_knn_group_cf takes.  (The flag is read directly and before anything else: with the
    switch off this path calls nothing.)"""
    if not _ext._fused_knn_grouping:
        return False
    if not transpose or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
                                for t in (x, y, features_at_y)):
        return False
    if x.dim() != 3 or y.dim() != 3 or features_at_y.dim() != 3 or features_at_y.shape[2] != y.shape[1]:
        return False                                         # the composition raises its own error
    K = int(K)
    if K > min(y.shape[1], 16):
        return False
    return _ext.knn_group_cf_supported(x.shape[0], x.shape[1], y.shape[1], K, features_at_y.shape[1])


def group_knn(x, y, features_at_y, K, transpose=False):
    """K nearest neighbours of x (B,N1,3) in y (B,N2,3) with 11 geometric channels.

    Returns (B,N1,K,C+11) = [feats | d2 | normalised 1/(d2+1e-8) | nn_abs(3) | nn_rel(3) | x(3)],
    or its (B,C+11,N1,K) view when transpose=True (features_at_y then is (B,C,N2)).
    The inverse-distance weights use the SQUARED distances (reference :500-503).
    """
    if _group_knn_takes_fused_op(x, y, features_at_y, K, transpose):
        d2, idx, _ = _ext.knn_group(x.detach().contiguous(), y.detach().contiguous(), K)
        return knn_and_group(x, y, features_at_y, idx, d2)
    feats_y = features_at_y.transpose(1, 2).contiguous() if transpose else features_at_y
    d2, idx, nn_abs = _ext.knn_points(x, y, K, return_nn=True)
    # K > N2: knn_points pads missing neighbours with idx -1 (dist 0, nn 0).  pytorch3d zero-initialises idx, so
    # the reference's knn_gather reads row 0 there; clamp to reproduce that instead of an out-of-range gather.
    neigh = knn_gather(feats_y, idx.clamp(min=0))
    x_rep = x.unsqueeze(2).repeat(1, 1, K, 1)
    nn_rel = nn_abs - x_rep
    d2 = d2.unsqueeze(3)
    recip = 1.0 / (d2 + 1e-8)
    weight = recip / torch.sum(recip, dim=2, keepdim=True)
    out = torch.cat([neigh, d2, weight, nn_abs, nn_rel, x_rep], dim=3)
    if transpose:
        out = out.transpose(2, 3).transpose(1, 2)
    return out
