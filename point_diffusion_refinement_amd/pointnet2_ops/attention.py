"""Per-neighbourhood attention pooling (reference pointnet2_ops/attention.py:35-96).

`AttentionModule` replaces max-pooling over the K neighbours of every SA /
feature-transfer / kNN-FP block: scores = MLP([conv(query) | conv(key)]) masked by
the ball-query count, softmax over K, weighted sum of conv(value).  Parameter
names (feat_conv, grouped_feat_conv, weight_conv.{1,2,4,5}, feat_out_conv.{0,1})
match the reference so its checkpoints load key for key.  `GlobalAttentionModule`
(N x N, attention.py:98-154) is not enabled by any shipped config and is not built.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ext
from .pointnet2_utils import attention_pool, group_norm_act, group_norm_act_add, relu_group_norm, \
    relu_group_norm_conv


class MyGroupNorm(nn.Module):
    """GroupNorm over the first C - C % G channels; trailing channels (appended xyz
    coordinates) pass through un-normalised (attention.py:6-23)."""

    def __init__(self, num_groups, num_channels):
        super().__init__()
        self.num_groups = num_groups
        self.num_channels = num_channels - num_channels % num_groups
        self.group_norm = nn.GroupNorm(self.num_groups, self.num_channels)

    def forward(self, x):
        if self.fusable(x):
            return self.fused(x, 'none')
        c = self.num_channels
        if x.shape[1] == c:
            return self.group_norm(x)
        return torch.cat([self.group_norm(x[:, :c]), x[:, c:]], dim=1)

    def fusable(self, x):
        """The switch is on (`set_fused_group_norm`, default off) and x is an fp32 GPU tensor of a shape
        pdr_group_norm_act takes."""
        return _ext.is_fused_group_norm() and x.is_cuda and x.dtype == torch.float32 and \
            x.shape[1] - x.shape[1] % self.num_groups == self.num_channels and \
            _ext.group_norm_act_supported(x.shape, self.num_groups)

    def injectable(self, x, add, residual):
        """x, add (B, C) and residual (x's shape), the last two optional, are fp32 GPU tensors of a shape
        pdr_group_norm_act_add takes.  Reached only under `set_fused_injection(True)`; independent of
        `set_fused_group_norm`.  Like `fusable` it does not ask for dense strides: `group_norm_act_add` copies a tensor
        that is not contiguous (the transposed groups of an unfused group_knn are the one such case in the network)."""
        C = x.shape[1]
        for t, shape in ((x, x.shape), (add, (x.shape[0], C)), (residual, x.shape)):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.shape == shape):
                return False
        return C - C % self.num_groups == self.num_channels and _ext.group_norm_act_supported(x.shape, self.num_groups)

    def fused(self, x, act):
        """act(self(x)) as one op: two launches forward, three backward, only x and (B, G) statistics saved."""
        gn = self.group_norm
        return group_norm_act(x, gn.weight, gn.bias, self.num_groups, gn.eps, act)


def fused_act_of(module):
    """'relu' / 'swish' for an activation module group_norm_act can absorb, else None."""
    if isinstance(module, nn.ReLU):
        return 'relu'
    return getattr(module, 'fused_act', None)


class NormActSequential(nn.Sequential):
    """nn.Sequential (same children, same parameter names) whose forward, with `set_fused_group_norm(True)`, runs a
    MyGroupNorm and the activation module directly after it as one `group_norm_act` call.  With the switch off it
    calls its children in order, as nn.Sequential does."""

    def forward(self, x):
        if not _ext.is_fused_group_norm():
            return super().forward(x)
        return self._run(list(self), x)

    @staticmethod
    def _run(mods, x):
        """The modules `mods` in order, a fusable MyGroupNorm and the activation after it as one op."""
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, MyGroupNorm) and m.fusable(x):
                act = fused_act_of(mods[i + 1]) if i + 1 < len(mods) else None
                x = m.fused(x, act or 'none')
                i += 2 if act else 1
            else:
                x = m(x)
                i += 1
        return x

    def forward_add(self, x, add=None, residual=None):
        """(self(x) + add[:, :, None, ..]) + residual, add (B, C) and residual (self(x)'s shape) each optional: what
        Mlp_plus_t_emb computes behind a stack (`set_fused_injection`).  Where the stack ends in a MyGroupNorm and an
        activation `group_norm_act` can absorb, and the norm's input, add and residual are fp32 GPU tensors of a
        shape the kernels take, the children before that pair run as `forward` runs them and the pair and the adds
        are ONE `group_norm_act_add` op; otherwise `forward` and the two torch additions."""
        if add is None and residual is None:
            return self.forward(x)
        mods = list(self)
        n = len(mods) - 2
        if n >= 0 and isinstance(mods[n], MyGroupNorm) and fused_act_of(mods[n + 1]):
            h = self._run(mods[:n], x)                     # (fusable is False with set_fused_group_norm off)
            if mods[n].injectable(h, add, residual):
                gn = mods[n].group_norm
                return group_norm_act_add(h, gn.weight, gn.bias, mods[n].num_groups, gn.eps, fused_act_of(mods[n + 1]),
                                          add, residual)
            h = self._run(mods[n:], h)
        else:
            h = self.forward(x)
        if add is not None:
            h = h + add[(slice(None), slice(None)) + (None,) * (h.dim() - 2)]
        if residual is not None:
            h = h + residual
        return h


def count_to_mask(count, K):
    ar = torch.arange(K, device=count.device, dtype=count.dtype)
    return ar.view(1, 1, K) < count.unsqueeze(-1)


def _act_norm_conv(cin, cout, norm):
    layers = [nn.ReLU(inplace=True)]
    if norm:
        layers.append(MyGroupNorm(min(32, cin), cin))
    layers.append(nn.Conv2d(cin, cout, kernel_size=1))
    return layers


def _fusable(scores, values):
    """fp32 GPU tensors of a shape pdr_attention_pool_cf takes (K <= 64, fewer than 2^31 elements)."""
    return scores.is_cuda and values.is_cuda and scores.dtype == torch.float32 and values.dtype == torch.float32 and \
        _ext.attention_pool_supported(*scores.shape)


class AttentionModule(nn.Module):
    def __init__(self, C_in1, C_in2, C1, C2, C_out, attention_bn=True, transform_grouped_feat_out=True,
                 last_activation=True):
        super().__init__()
        C1, C2 = max(C1, 32), max(C2, 32)
        self.feat_conv = nn.Conv2d(C_in1, C1, kernel_size=1)
        self.grouped_feat_conv = nn.Conv2d(C_in2, C2, kernel_size=1)
        inter = min(C1 + C2, C_out)
        self.weight_conv = NormActSequential(*(_act_norm_conv(C1 + C2, inter, attention_bn) +
                                           _act_norm_conv(inter, C_out, attention_bn)))
        self.transform_grouped_feat_out = transform_grouped_feat_out
        if transform_grouped_feat_out:
            tail = [nn.Conv2d(C_out, C_out, kernel_size=1)]
            if last_activation:
                if attention_bn:
                    tail.append(MyGroupNorm(min(32, C_out), C_out))
                tail.append(nn.ReLU(inplace=True))
            self.feat_out_conv = NormActSequential(*tail)

    def score_head(self, feat, grouped_feat):
        """feat (B,C_in1,N), grouped_feat (B,C_in2,N,K) -> scores (B,C_out,N,K): weight_conv over
        [feat_conv(query) repeated over K | grouped_feat_conv(key)]."""
        K = grouped_feat.shape[-1]
        if _ext._fused_score_norm or _ext._fused_score_conv:   # read directly: with both off this path calls nothing
            scores = self._fused_score_head(feat, grouped_feat)
            if scores is not None:
                return scores
        q = self.feat_conv(feat.unsqueeze(-1)).expand(-1, -1, -1, K)
        k = self.grouped_feat_conv(grouped_feat)
        return self.weight_conv(torch.cat([q, k], dim=1))

    def _fused_score_head(self, feat, grouped_feat):
        """The score head without the expand and the cat, each [ReLU, MyGroupNorm] pair of weight_conv as one
        `relu_group_norm` op (set_fused_score_norm, default off); None where that does not apply: no norms
        (attention_bn=False), tensors that are not fp32 on the GPU, or a shape the kernels do not take.
        With set_fused_score_conv (default off) a whole [ReLU, MyGroupNorm, Conv2d] link whose shape
        `relu_group_norm_conv_supported` accepts is one `relu_group_norm_conv` op with the Conv2d's own weight and
        bias; a link it does not accept runs as above under set_fused_score_norm, else as the composition."""
        wc = self.weight_conv
        if len(wc) != 6 or not (isinstance(wc[1], MyGroupNorm) and isinstance(wc[4], MyGroupNorm)):
            return None
        if not (feat.is_cuda and grouped_feat.is_cuda and feat.dtype == torch.float32
                and grouped_feat.dtype == torch.float32 and feat.dim() == 3 and grouped_feat.dim() == 4):
            return None
        B, _, N, K = grouped_feat.shape
        C1, C2 = self.feat_conv.out_channels, self.grouped_feat_conv.out_channels
        if not (_ext.relu_group_norm_supported(C1, (B, C2, N, K), wc[1].num_groups)
                and _ext.relu_group_norm_supported(0, (B, wc[2].out_channels, N, K), wc[4].num_groups)):
            return None
        conv_on, norm_on = _ext._fused_score_conv, _ext._fused_score_norm
        as_conv = [conv_on and _ext.relu_group_norm_conv_supported(c1, (B, c2, N, K), wc[i].num_groups,
                                                                    wc[i + 1].out_channels)
                   for i, c1, c2 in ((1, C1, C2), (4, 0, wc[2].out_channels))]
        if not norm_on and not any(as_conv):
            return None
        q = self.feat_conv(feat.unsqueeze(-1)).squeeze(-1)
        h = self.grouped_feat_conv(grouped_feat)
        for i, fused in ((1, as_conv[0]), (4, as_conv[1])):
            gn, conv = wc[i].group_norm, wc[i + 1]
            if fused:
                h = relu_group_norm_conv(h, gn.weight, gn.bias, wc[i].num_groups, gn.eps,
                                         conv.weight.view(conv.out_channels, -1), conv.bias, q=q)
            elif norm_on:
                h = conv(relu_group_norm(h, gn.weight, gn.bias, wc[i].num_groups, gn.eps, q=q))
            else:                                         # the composition of this link
                if q is not None:
                    h = torch.cat([q.unsqueeze(-1).expand(-1, -1, -1, K), h], dim=1)
                h = conv(wc[i](wc[i - 1](h)))
            q = None
        return h

    def forward(self, feat, grouped_feat, grouped_feat_out, count):
        """feat (B,C_in1,N) query; grouped_feat (B,C_in2,N,K) key; grouped_feat_out (B,C_out,N,K)
        value; count (B,N) valid neighbours or 'all'.  Returns (B,C_out,N)."""
        K = grouped_feat.shape[-1]
        scores = self.score_head(feat, grouped_feat)
        if _ext.is_fused_attention_pool() and _fusable(scores, grouped_feat_out):
            # one launch forward, one backward, no saved softmax (pdr_attention_pool_cf); the switch is off by default
            if self.transform_grouped_feat_out:
                grouped_feat_out = self.feat_out_conv(grouped_feat_out)
            if not (isinstance(count, str) and count == 'all'):
                count = count.int().contiguous()
            return attention_pool(scores.contiguous(), grouped_feat_out.contiguous(), count)
        if not (isinstance(count, str) and count == 'all'):
            mask = count_to_mask(torch.clamp(count, min=1), K).unsqueeze(1).float()
            scores = scores * mask + (-1e9) * (1 - mask)
        weight = F.softmax(scores, dim=-1)
        if self.transform_grouped_feat_out:
            grouped_feat_out = self.feat_out_conv(grouped_feat_out)
        return (grouped_feat_out * weight).sum(dim=-1)
