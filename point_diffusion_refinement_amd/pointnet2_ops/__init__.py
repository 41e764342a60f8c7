"""Drop-in for the reference's `pointnet2_ops` package (pointnet2_ops/__init__.py:1-3).

`set_deterministic(True | False | None)` chooses the backward kernels of gather / group / three_interpolate /
knn_points: order-fixed, atomic, or (None, the default) whatever `torch.are_deterministic_algorithms_enabled()` says.
`set_fused_attention_pool(True | False)` (default False) makes `AttentionModule` pool with the one-launch
`pointnet2_utils.attention_pool` and its one-launch backward instead of the torch composition.
`set_fused_group_norm(True | False)` (default False) makes every `MyGroupNorm` of the module path, with the ReLU / Swish
that follows it, run as the one op `pointnet2_utils.group_norm_act` instead of nn.GroupNorm, cat and activation.
`set_fused_grouping(True | False)` (default False) makes `QueryAndGroup` hand everything after its neighbour search to
the one op `pointnet2_utils.query_and_group` instead of two grouping_operations, the empty-ball patch and the cats.
`set_fused_knn_grouping(True | False)` (default False) makes `group_knn(..., transpose=True)` hand everything after its
neighbour search to the one op `pointnet2_utils.knn_and_group` instead of knn_gather, the weight arithmetic, the cat
and two transposes.
`set_fused_score_norm(True | False)` (default False) makes `AttentionModule` run the front of its score head -- expand,
cat, then each [ReLU, MyGroupNorm] pair of `weight_conv` -- as the one op `pointnet2_utils.relu_group_norm`, which
never builds the cat.
`set_fused_injection(True | False)` (default False) makes `Mlp_plus_t_emb` fold the embedding it adds behind each of its
[conv, MyGroupNorm, act] stacks, and the residual behind the last one, into the stack's last norm and activation: the
one op `pointnet2_utils.group_norm_act_add` instead of the norm, the activation, the broadcast adds and the residual
add.
`set_fused_score_conv(True | False)` (default False) makes `AttentionModule` run each [ReLU, MyGroupNorm, Conv2d 1x1]
link of its score head as the one op `pointnet2_utils.relu_group_norm_conv`, whose fp32 MFMA GEMM normalises its
operand as it loads it: neither the cat nor the normalised tensor is built or saved."""
from . import pointnet2_modules, pointnet2_utils  # noqa: F401
from ._ext import (is_deterministic, is_fused_attention_pool, is_fused_group_norm, is_fused_grouping,  # noqa: F401
                   is_fused_injection, is_fused_knn_grouping, is_fused_score_conv, is_fused_score_norm,
                   set_deterministic, set_fused_attention_pool, set_fused_group_norm, set_fused_grouping,
                   set_fused_injection, set_fused_knn_grouping, set_fused_score_conv, set_fused_score_norm)
