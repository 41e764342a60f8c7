"""Stand-in for the reference's compiled module `pointnet2_ops._ext`.

Same nine callables with the same argument order and return types as the pybind
module defined in _ext-src/src/bindings.cpp:6-19, plus `knn_points` (the
pytorch3d.ops.knn entry the reference's Python layer calls).  Each function
validates like the reference's AT_ASSERT macros (_ext-src/include/utils.h:5-25:
contiguous, dtype, device) -- raising RuntimeError instead of aborting --,
allocates the outputs as torch tensors and forwards raw device pointers plus the
CURRENT stream to libpdr_hip.so.  CPU tensors are rejected exactly like the
reference ("CPU not supported", sampling.cpp:34): there is no CPU fallback.
"""
import ctypes

import torch

from .. import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t, name, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must be a %s tensor" % (name, "float" if dtype == torch.float32 else "int"))


def _req_xyz(t, name):
    """(B, N, 3) coordinate clouds: the kernels read three floats per point."""
    if t.dim() != 3 or t.shape[2] != 3:
        raise RuntimeError("%s must have shape (B, N, 3), got %s" % (name, tuple(t.shape)))


def _same_device(*ts):
    d = ts[0].device
    for t in ts[1:]:
        if t.device != d:
            raise RuntimeError("all tensors must live on the same device")


_deterministic = None      # set_deterministic: None = follow torch.are_deterministic_algorithms_enabled()


def set_deterministic(mode):
    """Choose the backward kernels of gather / group / three_interpolate / knn_points: True = the order-fixed
    `*_grad_det` calls (same input, same bits), False = the atomic ones, None (the default) = follow
    `torch.are_deterministic_algorithms_enabled()`.  Returns the previous setting.  In deterministic mode a size the
    deterministic kernels do not support raises; nothing falls back to atomics."""
    global _deterministic
    if mode is not None and not isinstance(mode, bool):
        raise TypeError("set_deterministic takes True, False or None, got %r" % (mode,))
    prev, _deterministic = _deterministic, mode
    return prev


def is_deterministic():
    """Whether the autograd Functions take the deterministic backward kernels right now."""
    if _deterministic is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    return _deterministic


_fused_attention_pool = False     # set_fused_attention_pool: AttentionModule pools with pdr_attention_pool_cf


def set_fused_attention_pool(mode):
    """Process-wide switch: True = `AttentionModule.forward` pools its fp32 GPU tensors with one `attention_pool` launch
    (and one backward launch) where the kernel supports the shape; False (the default) = the torch composition, as ever.
    Returns the previous setting."""
    global _fused_attention_pool
    if not isinstance(mode, bool):
        raise TypeError("set_fused_attention_pool takes True or False, got %r" % (mode,))
    prev, _fused_attention_pool = _fused_attention_pool, mode
    return prev


def is_fused_attention_pool():
    """Whether AttentionModule.forward takes the fused pooling kernel right now."""
    return _fused_attention_pool


_fused_group_norm = False         # set_fused_group_norm: MyGroupNorm (+ the activation after it) runs pdr_group_norm_act


def set_fused_group_norm(mode):
    """Process-wide switch: True = every `MyGroupNorm` of the module path, with the ReLU / Swish that directly follows
    it in the same `nn.Sequential`, runs as one `group_norm_act` op (and its backward) for fp32 GPU tensors of a shape
    the kernels support; False (the default) = `nn.GroupNorm`, the slice-and-cat and the activation modules, as ever.
    Returns the previous setting."""
    global _fused_group_norm
    if not isinstance(mode, bool):
        raise TypeError("set_fused_group_norm takes True or False, got %r" % (mode,))
    prev, _fused_group_norm = _fused_group_norm, mode
    return prev


def is_fused_group_norm():
    """Whether MyGroupNorm takes the fused kernels right now."""
    return _fused_group_norm


_fused_grouping = False           # set_fused_grouping: QueryAndGroup groups with pdr_query_group_cf


def set_fused_grouping(mode):
    """Process-wide switch: True = `QueryAndGroup.forward` hands everything after its neighbour search to the one op
    `pointnet2_utils.query_and_group` (one launch forward, an order-fixed backward) for fp32 GPU tensors of a size the
    kernels support; False (the default) = the torch composition of grouping_operation, select, subtract and cat, as
    ever.  Returns the previous setting."""
    global _fused_grouping
    if not isinstance(mode, bool):
        raise TypeError("set_fused_grouping takes True or False, got %r" % (mode,))
    prev, _fused_grouping = _fused_grouping, mode
    return prev


def is_fused_grouping():
    """Whether QueryAndGroup takes the fused grouping op right now."""
    return _fused_grouping


_fused_knn_grouping = False       # set_fused_knn_grouping: group_knn groups with pdr_knn_group_cf


def set_fused_knn_grouping(mode):
    """Process-wide switch: True = `group_knn(..., transpose=True)` searches with `knn_group` and hands everything after
    the search to the one op `pointnet2_utils.knn_and_group` (one launch forward, an order-fixed backward) for fp32 GPU
    tensors with K <= min(n2, 16) and a size the kernels support; False (the default) = the torch composition of
    knn_points, knn_gather, the weight arithmetic, cat and two transposes, as ever.  Returns the previous setting."""
    global _fused_knn_grouping
    if not isinstance(mode, bool):
        raise TypeError("set_fused_knn_grouping takes True or False, got %r" % (mode,))
    prev, _fused_knn_grouping = _fused_knn_grouping, mode
    return prev


def is_fused_knn_grouping():
    """Whether group_knn takes the fused grouping op right now."""
    return _fused_knn_grouping


_fused_score_norm = False         # set_fused_score_norm: AttentionModule's score head runs pdr_relu_group_norm_cf


def set_fused_score_norm(mode):
    """Process-wide switch: True = `AttentionModule.forward` skips the expand and the cat of its score head and runs each
    [ReLU, MyGroupNorm] pair of `weight_conv` as one `relu_group_norm` op (and its backward) for fp32 GPU tensors of a
    shape the kernels support; False (the default) = the torch composition, as ever.  Independent of the other
    switches.  Returns the previous setting."""
    global _fused_score_norm
    if not isinstance(mode, bool):
        raise TypeError("set_fused_score_norm takes True or False, got %r" % (mode,))
    prev, _fused_score_norm = _fused_score_norm, mode
    return prev


def is_fused_score_norm():
    """Whether AttentionModule's score head takes the fused ReLU + GroupNorm op right now."""
    return _fused_score_norm


_fused_score_conv = False         # set_fused_score_conv: the score head's links run pdr_relu_group_norm_conv_cf


def set_fused_score_conv(mode):
    """Process-wide switch: True = `AttentionModule.forward` skips the expand and the cat of its score head and runs each
    [ReLU, MyGroupNorm, Conv2d 1x1] link of `weight_conv` as one `relu_group_norm_conv` op (and its backward), which
    never builds the normalised tensor, for fp32 GPU tensors of a shape the kernels support; a link they do not take
    runs as it does under `set_fused_score_norm`.  False (the default) = as ever.  Independent of the other switches.
    Returns the previous setting."""
    global _fused_score_conv
    if not isinstance(mode, bool):
        raise TypeError("set_fused_score_conv takes True or False, got %r" % (mode,))
    prev, _fused_score_conv = _fused_score_conv, mode
    return prev


def is_fused_score_conv():
    """Whether AttentionModule's score head takes the fused ReLU + GroupNorm + conv op right now."""
    return _fused_score_conv


_fused_injection = False          # set_fused_injection: Mlp_plus_t_emb's adds run inside pdr_group_norm_act_add


def set_fused_injection(mode):
    """Process-wide switch: True = `Mlp_plus_t_emb.forward` hands the last [MyGroupNorm, ReLU / Swish] of each of its
    stacks, together with the embedding it injects behind that stack and (behind the last stack) the residual, to the
    one op `pointnet2_utils.group_norm_act_add` for fp32 GPU tensors of a shape the kernels support; False
    (the default) = the stack followed by the broadcast adds and the residual add, as ever.  Independent of the other
    switches.  Returns the previous setting."""
    global _fused_injection
    if not isinstance(mode, bool):
        raise TypeError("set_fused_injection takes True or False, got %r" % (mode,))
    prev, _fused_injection = _fused_injection, mode
    return prev


def is_fused_injection():
    """Whether Mlp_plus_t_emb folds its injections and residual into the GroupNorm + activation op right now."""
    return _fused_injection


def _scatter_workspace(B, P, N, device):
    """Scratch of one `*_grad_det` call (pdr_scatter_workspace_bytes), a torch allocation per call."""
    nbytes = _lib.load().pdr_scatter_workspace_bytes(int(B), int(P), int(N))
    return torch.empty((max(int(nbytes), 4),), dtype=torch.uint8, device=device)


def furthest_point_sampling(points, nsamples):
    """(B,N,3) f32 -> (B,nsamples) i32   [sampling.cpp:66-87]"""
    _req(points, "points", torch.float32)
    _req_xyz(points, "points")
    B, N, _ = points.shape
    lib = _lib.load()
    out = torch.empty((B, nsamples), dtype=torch.int32, device=points.device)
    ws = lib.pdr_fps_workspace_bytes(B, N)
    temp = torch.empty((ws // 4,), dtype=torch.float32, device=points.device) if ws else None
    with torch.cuda.device(points.device):
        _lib.check(lib.pdr_furthest_point_sampling(points.data_ptr(), B, N, int(nsamples),
                                                   temp.data_ptr() if temp is not None else None,
                                                   out.data_ptr(), _stream()), "furthest_point_sampling")
    return out


def furthest_point_sampling_ragged(points, nsamples, lengths=None, mirror_axis=None, return_rows=False):
    """Length-aware FPS of a padded batch, optionally of every cloud together with its mirror image, in one launch:
    (B,N,3) f32 [, lengths (B,) i64 on the device] -> idx (B,nsamples) i32 [, rows (B,nsamples,4) f32].

    Cloud b is the virtual cloud of its first lengths[b] rows, followed -- when `mirror_axis` is 0 / 1 / 2 -- by the
    same rows with that coordinate negated; `idx` indexes the virtual cloud and row j of `rows` is the picked point's
    (x, y, z, tag), tag -1 for a mirrored point.  Each row of `idx` is what `furthest_point_sampling` returns for the
    materialised virtual cloud; padding rows are never read, a cloud of length 0 gets idx -1 / rows 0
    (pdr_furthest_point_sampling_ragged of include/pdr_hip.h)."""
    if mirror_axis is not None and mirror_axis not in (0, 1, 2):
        raise ValueError("mirror_axis must be None, 0, 1 or 2, got %r" % (mirror_axis,))
    _req(points, "points", torch.float32)
    _req_xyz(points, "points")
    _req_lengths(lengths, "lengths", points)
    axis = -1 if mirror_axis is None else int(mirror_axis)
    B, N, _ = points.shape
    m = int(nsamples)
    lib = _lib.load()
    idx = torch.empty((B, m), dtype=torch.int32, device=points.device)
    rows = torch.empty((B, m, 4), dtype=torch.float32, device=points.device) if return_rows else None
    ws = lib.pdr_fps_ragged_workspace_bytes(B, N, axis)
    temp = torch.empty((ws // 4,), dtype=torch.float32, device=points.device) if ws else None
    with torch.cuda.device(points.device):
        _lib.check(lib.pdr_furthest_point_sampling_ragged(points.data_ptr(), _ptr(lengths), B, N, axis, m, _ptr(temp),
                                                          idx.data_ptr(), _ptr(rows), _stream()),
                   "furthest_point_sampling_ragged")
    return (idx, rows) if return_rows else idx


def gather_points(points, idx):
    """(B,C,N) f32, (B,m) i32 -> (B,C,m)   [sampling.cpp:15-38]"""
    _req(points, "points", torch.float32)
    _req(idx, "idx", torch.int32)
    _same_device(points, idx)
    B, C, N = points.shape
    m = idx.shape[1]
    out = torch.empty((B, C, m), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _lib.check(_lib.load().pdr_gather_points(points.data_ptr(), idx.data_ptr(), B, C, N, m,
                                                 out.data_ptr(), _stream()), "gather_points")
    return out


def gather_points_grad(grad_out, idx, n):
    """(B,C,m) f32, (B,m) i32, n -> (B,C,n)   [sampling.cpp:40-64]"""
    _req(grad_out, "grad_out", torch.float32)
    _req(idx, "idx", torch.int32)
    _same_device(grad_out, idx)
    B, C, m = grad_out.shape
    out = torch.empty((B, C, n), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_gather_points_grad(grad_out.data_ptr(), idx.data_ptr(), B, C, int(n), m,
                                                      out.data_ptr(), _stream()), "gather_points_grad")
    return out


def gather_points_grad_det(grad_out, idx, n):
    """gather_points_grad with a fixed summation order (pdr_gather_points_grad_det): sources added in ascending
    position from +0.0, the same bits run after run."""
    _req(grad_out, "grad_out", torch.float32)
    _req(idx, "idx", torch.int32)
    _same_device(grad_out, idx)
    B, C, m = grad_out.shape
    out = torch.empty((B, C, n), dtype=torch.float32, device=grad_out.device)
    ws = _scatter_workspace(B, m, n, grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_gather_points_grad_det(grad_out.data_ptr(), idx.data_ptr(), B, C, int(n), m,
                                                          out.data_ptr(), ws.data_ptr(), _stream()),
                   "gather_points_grad_det")
    return out


def ball_query(new_xyz, xyz, radius, nsample):
    """(B,m,3), (B,n,3), r, ns -> (idx (B,m,ns) i32, counts (B,m) i32)   [ball_query.cpp:10-38]"""
    _req(new_xyz, "new_xyz", torch.float32)
    _req(xyz, "xyz", torch.float32)
    _req_xyz(new_xyz, "new_xyz")
    _req_xyz(xyz, "xyz")
    _same_device(new_xyz, xyz)
    if new_xyz.shape[0] != xyz.shape[0]:
        raise RuntimeError("new_xyz and xyz must have the same batch size")
    B, m, _ = new_xyz.shape
    n = xyz.shape[1]
    idx = torch.empty((B, m, nsample), dtype=torch.int32, device=xyz.device)
    counts = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.check(_lib.load().pdr_ball_query(new_xyz.data_ptr(), xyz.data_ptr(), B, n, m, float(radius),
                                              int(nsample), idx.data_ptr(), counts.data_ptr(), _stream()),
                   "ball_query")
    return idx, counts


def group_points(points, idx):
    """(B,C,N) f32, (B,np,ns) i32 -> (B,C,np,ns)   [group_points.cpp:12-36]"""
    _req(points, "points", torch.float32)
    _req(idx, "idx", torch.int32)
    _same_device(points, idx)
    B, C, N = points.shape
    _, npnt, ns = idx.shape
    out = torch.empty((B, C, npnt, ns), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _lib.check(_lib.load().pdr_group_points(points.data_ptr(), idx.data_ptr(), B, C, N, npnt, ns,
                                                out.data_ptr(), _stream()), "group_points")
    return out


def group_points_grad(grad_out, idx, n):
    """(B,C,np,ns) f32, (B,np,ns) i32, n -> (B,C,n)   [group_points.cpp:38-64]"""
    _req(grad_out, "grad_out", torch.float32)
    _req(idx, "idx", torch.int32)
    _same_device(grad_out, idx)
    B, C, npnt, ns = grad_out.shape
    out = torch.empty((B, C, n), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_group_points_grad(grad_out.data_ptr(), idx.data_ptr(), B, C, int(n), npnt, ns,
                                                     out.data_ptr(), _stream()), "group_points_grad")
    return out


def group_points_grad_det(grad_out, idx, n):
    """group_points_grad with a fixed summation order (pdr_group_points_grad_det)."""
    _req(grad_out, "grad_out", torch.float32)
    _req(idx, "idx", torch.int32)
    _same_device(grad_out, idx)
    B, C, npnt, ns = grad_out.shape
    out = torch.empty((B, C, n), dtype=torch.float32, device=grad_out.device)
    ws = _scatter_workspace(B, npnt * ns, n, grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_group_points_grad_det(grad_out.data_ptr(), idx.data_ptr(), B, C, int(n), npnt, ns,
                                                         out.data_ptr(), ws.data_ptr(), _stream()),
                   "group_points_grad_det")
    return out


def three_nn(unknowns, knows):
    """(B,n,3), (B,m,3) -> [dist2 (B,n,3) f32 SQUARED, idx (B,n,3) i32]   [interpolate.cpp:14-40]"""
    _req(unknowns, "unknowns", torch.float32)
    _req(knows, "knows", torch.float32)
    _req_xyz(unknowns, "unknowns")
    _req_xyz(knows, "knows")
    _same_device(unknowns, knows)
    B, n, _ = unknowns.shape
    m = knows.shape[1]
    dist2 = torch.empty((B, n, 3), dtype=torch.float32, device=unknowns.device)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknowns.device)
    with torch.cuda.device(unknowns.device):
        _lib.check(_lib.load().pdr_three_nn(unknowns.data_ptr(), knows.data_ptr(), B, n, m, dist2.data_ptr(),
                                            idx.data_ptr(), _stream()), "three_nn")
    return [dist2, idx]


def three_interpolate(points, idx, weight):
    """(B,C,m) f32, (B,n,3) i32, (B,n,3) f32 -> (B,C,n)   [interpolate.cpp:42-70]"""
    _req(points, "points", torch.float32)
    _req(idx, "idx", torch.int32)
    _req(weight, "weight", torch.float32)
    _same_device(points, idx, weight)
    B, C, m = points.shape
    n = idx.shape[1]
    out = torch.empty((B, C, n), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _lib.check(_lib.load().pdr_three_interpolate(points.data_ptr(), idx.data_ptr(), weight.data_ptr(), B, C, m,
                                                     n, out.data_ptr(), _stream()), "three_interpolate")
    return out


def three_interpolate_grad(grad_out, idx, weight, m):
    """(B,C,n) f32, (B,n,3) i32, (B,n,3) f32, m -> (B,C,m)   [interpolate.cpp:72-100]"""
    _req(grad_out, "grad_out", torch.float32)
    _req(idx, "idx", torch.int32)
    _req(weight, "weight", torch.float32)
    _same_device(grad_out, idx, weight)
    B, C, n = grad_out.shape
    out = torch.empty((B, C, m), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_three_interpolate_grad(grad_out.data_ptr(), idx.data_ptr(), weight.data_ptr(), B,
                                                          C, n, int(m), out.data_ptr(), _stream()),
                   "three_interpolate_grad")
    return out


def three_interpolate_grad_det(grad_out, idx, weight, m):
    """three_interpolate_grad with a fixed summation order (pdr_three_interpolate_grad_det)."""
    _req(grad_out, "grad_out", torch.float32)
    _req(idx, "idx", torch.int32)
    _req(weight, "weight", torch.float32)
    _same_device(grad_out, idx, weight)
    B, C, n = grad_out.shape
    out = torch.empty((B, C, m), dtype=torch.float32, device=grad_out.device)
    ws = _scatter_workspace(B, 3 * n, m, grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_three_interpolate_grad_det(grad_out.data_ptr(), idx.data_ptr(), weight.data_ptr(),
                                                              B, C, n, int(m), out.data_ptr(), ws.data_ptr(),
                                                              _stream()), "three_interpolate_grad_det")
    return out


def knn_points_grad(p1, p2, idx, grad_dists, deterministic=False):
    """Backward of knn_points' squared distances: (B,n1,3), (B,n2,3), idx (B,n1,K) i64, grad_dists (B,n1,K)
    -> (grad_p1, grad_p2).  deterministic=True takes pdr_knn_points_grad_det, whose grad_p2 is summed in a fixed order
    (grad_p1 is order-fixed in both)."""
    _req(p1, "p1", torch.float32)
    _req(p2, "p2", torch.float32)
    _req(idx, "idx", torch.int64)
    _req(grad_dists, "grad_dists", torch.float32)
    _same_device(p1, p2, idx, grad_dists)
    B, n1, _ = p1.shape
    n2, K = p2.shape[1], idx.shape[2]
    g1 = torch.empty_like(p1)
    g2 = torch.empty_like(p2)
    lib = _lib.load()
    with torch.cuda.device(p1.device):
        if deterministic:
            ws = _scatter_workspace(B, n1 * K, n2, p1.device)
            _lib.check(lib.pdr_knn_points_grad_det(p1.data_ptr(), p2.data_ptr(), idx.data_ptr(), grad_dists.data_ptr(),
                                                   B, n1, n2, K, g1.data_ptr(), g2.data_ptr(), ws.data_ptr(),
                                                   _stream()), "knn_points_grad_det")
        else:
            _lib.check(lib.pdr_knn_points_grad(p1.data_ptr(), p2.data_ptr(), idx.data_ptr(), grad_dists.data_ptr(), B,
                                               n1, n2, K, g1.data_ptr(), g2.data_ptr(), _stream()), "knn_points_grad")
    return g1, g2


def _req_lengths(t, name, cloud):
    """pytorch3d per-cloud lengths: (B,) int64 on the clouds' device, or None (every cloud full).  The values stay on
    the device: the kernels read and clamp them, nothing here does."""
    if t is None:
        return
    _req(t, name, torch.int64)
    if t.dim() != 1 or t.shape[0] != cloud.shape[0]:
        raise RuntimeError("%s must have shape (B,) = (%d,), got %s" % (name, cloud.shape[0], tuple(t.shape)))
    _same_device(cloud, t)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _knn_forward(p1, p2, K, return_nn, lengths1=None, lengths2=None):
    B, n1, _ = p1.shape
    n2 = p2.shape[1]
    dists = torch.empty((B, n1, K), dtype=torch.float32, device=p1.device)
    idx = torch.empty((B, n1, K), dtype=torch.int64, device=p1.device)
    nn = torch.empty((B, n1, K, 3), dtype=torch.float32, device=p1.device) if return_nn else None
    with torch.cuda.device(p1.device):
        if lengths1 is None and lengths2 is None:
            rc = _lib.load().pdr_knn_points(p1.data_ptr(), p2.data_ptr(), B, n1, n2, int(K), dists.data_ptr(),
                                            idx.data_ptr(), _ptr(nn), _stream())
        else:
            rc = _lib.load().pdr_knn_points_ragged(p1.data_ptr(), p2.data_ptr(), _ptr(lengths1), _ptr(lengths2), B,
                                                   n1, n2, int(K), dists.data_ptr(), idx.data_ptr(), _ptr(nn),
                                                   _stream())
        _lib.check(rc, "knn_points")
    return dists, idx, nn


def chamfer_nn(x, y, x_lengths=None, y_lengths=None):
    """Both K = 1 searches of a Chamfer evaluation in one launch:
    (B,n1,3), (B,n2,3) -> (dist_xy (B,n1), idx_xy (B,n1) i64, dist_yx (B,n2), idx_yx (B,n2) i64); not differentiable
    (chamfer_distance uses knn_points when a gradient is needed).  With `x_lengths` / `y_lengths` ((B,) int64 on the
    clouds' device) cloud b is x[b, :x_lengths[b]] / y[b, :y_lengths[b]]; padded queries and queries of an empty
    opposite cloud get distance 0 and index 0."""
    _req(x, "x", torch.float32)
    _req(y, "y", torch.float32)
    _same_device(x, y)
    if x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
        raise RuntimeError("chamfer_nn: (B,n,3) clouds with equal batch size")
    _req_lengths(x_lengths, "x_lengths", x)
    _req_lengths(y_lengths, "y_lengths", y)
    B, n1, _ = x.shape
    n2 = y.shape[1]
    dx = torch.empty((B, n1), dtype=torch.float32, device=x.device)
    dy = torch.empty((B, n2), dtype=torch.float32, device=x.device)
    ix = torch.empty((B, n1), dtype=torch.int64, device=x.device)
    iy = torch.empty((B, n2), dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        if x_lengths is None and y_lengths is None:
            rc = _lib.load().pdr_chamfer_nn(x.data_ptr(), y.data_ptr(), B, n1, n2, dx.data_ptr(), ix.data_ptr(),
                                            dy.data_ptr(), iy.data_ptr(), _stream())
        else:
            rc = _lib.load().pdr_chamfer_nn_ragged(x.data_ptr(), y.data_ptr(), _ptr(x_lengths), _ptr(y_lengths), B,
                                                   n1, n2, dx.data_ptr(), ix.data_ptr(), dy.data_ptr(),
                                                   iy.data_ptr(), _stream())
        _lib.check(rc, "chamfer_nn")
    return dx, ix, dy, iy


def _chamfer_loss_forward(x, y, x_lengths, y_lengths, with_idx):
    B, n1, _ = x.shape
    n2 = y.shape[1]
    lib = _lib.load()
    sums = torch.empty((B, 4), dtype=torch.float32, device=x.device)
    ix = torch.empty((B, n1), dtype=torch.int32, device=x.device) if with_idx else None
    iy = torch.empty((B, n2), dtype=torch.int32, device=x.device) if with_idx else None
    nbytes = lib.pdr_chamfer_loss_workspace_bytes(B, n1, n2)     # block partials of this call, a torch allocation
    ws = torch.empty((max(int(nbytes), 4),), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pdr_chamfer_loss(x.data_ptr(), y.data_ptr(), _ptr(x_lengths), _ptr(y_lengths), B, n1, n2,
                                        sums.data_ptr(), _ptr(ix), _ptr(iy), ws.data_ptr(), _stream()), "chamfer_loss")
    return sums, ix, iy


class _ChamferLossSums(torch.autograd.Function):
    """pdr_chamfer_loss with its int32 indices saved for pdr_chamfer_loss_grad (one launch, order-fixed: the same bits
    whatever set_deterministic says)."""

    @staticmethod
    def forward(ctx, x, y, x_lengths, y_lengths):
        sums, ix, iy = _chamfer_loss_forward(x, y, x_lengths, y_lengths, True)
        ctx.save_for_backward(x, y, x_lengths, y_lengths, ix, iy)
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sums):
        x, y, x_lengths, y_lengths, ix, iy = ctx.saved_tensors
        B, n1, _ = x.shape
        gs = grad_sums.contiguous().float()
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().pdr_chamfer_loss_grad(x.data_ptr(), y.data_ptr(), _ptr(x_lengths), _ptr(y_lengths),
                                                         ix.data_ptr(), iy.data_ptr(), gs.data_ptr(), B, n1,
                                                         y.shape[1], gx.data_ptr(), gy.data_ptr(), _stream()),
                       "chamfer_loss_grad")
        return gx, gy, None, None


def chamfer_loss_sums(x, y, x_lengths=None, y_lengths=None):
    """The four sums a Chamfer loss is made of, differentiable w.r.t. both clouds (pdr_chamfer_loss /
    pdr_chamfer_loss_grad): (B,n1,3), (B,n2,3) -> sums (B,4) f32 =
    (sum_i d_xy, sum_j d_yx, sum_i sqrt d_xy, sum_j sqrt d_yx) with d_xy[i] = min_j |x_i - y_j|^2, over the valid
    points.  `x_lengths` / `y_lengths` ((B,) int64 on the clouds' device, None = full) as in chamfer_nn; a pair with an
    empty side gives four zeros.  Under torch.no_grad(), or when neither cloud requires a gradient, no index is
    computed.  Where the torch composition's gradient of sqrt is NaN -- a coincident pair, d = 0 -- this one's sqrt
    term is 0."""
    _req(x, "x", torch.float32)
    _req(y, "y", torch.float32)
    _same_device(x, y)
    _req_xyz(x, "x")
    _req_xyz(y, "y")
    if x.shape[0] != y.shape[0]:
        raise RuntimeError("chamfer_loss_sums: (B,n,3) clouds with equal batch size")
    _req_lengths(x_lengths, "x_lengths", x)
    _req_lengths(y_lengths, "y_lengths", y)
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _ChamferLossSums.apply(x, y, x_lengths, y_lengths)
    return _chamfer_loss_forward(x, y, x_lengths, y_lengths, False)[0]


def _req_pool(scores, values, count):
    """Shapes and dtypes of the attention pool's inputs; returns (B, C, N, K) and the count tensor or None ('all')."""
    _req(scores, "scores", torch.float32)
    _req(values, "values", torch.float32)
    _same_device(scores, values)
    if scores.dim() != 4 or values.shape != scores.shape:
        raise RuntimeError("attention_pool: scores and values must both be (B, C, N, K), got %s and %s"
                           % (tuple(scores.shape), tuple(values.shape)))
    B, C, N, K = scores.shape
    if count is None or (isinstance(count, str) and count == 'all'):
        return (B, C, N, K), None
    _req(count, "count", torch.int32)
    _same_device(scores, count)
    if tuple(count.shape) != (B, N):
        raise RuntimeError("count must have shape (B, N) = (%d, %d), got %s" % (B, N, tuple(count.shape)))
    return (B, C, N, K), count


def attention_pool_supported(B, C, N, K):
    """Whether pdr_attention_pool_cf takes a (B, C, N, K) problem (it refuses K > 64 and 2^31 elements or more)."""
    plan = (_lib._c.c_int * 4)()
    return _lib.load().pdr_attention_pool_cf_plan(int(K), 1, plan) == _lib.PDR_OK and B * C * N * K < 2 ** 31


def attention_pool(scores, values, count):
    """Masked softmax over the K neighbours and weighted sum of the values, in one launch (pdr_attention_pool_cf):
    scores, values (B,C,N,K) f32, count (B,N) i32 / None / 'all' -> (B,C,N).  Slots k >= clamp(count, 1, K) carry
    exactly -1e9 (attention.py:71-77)."""
    (B, C, N, K), cnt = _req_pool(scores, values, count)
    out = torch.empty((B, C, N), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().pdr_attention_pool_cf(scores.data_ptr(), values.data_ptr(), _ptr(cnt), B, C, N, K,
                                                     out.data_ptr(), _stream()), "attention_pool")
    return out


def attention_pool_grad(scores, values, count, grad_out, need_scores=True, need_values=True):
    """Backward of attention_pool in one launch (pdr_attention_pool_cf_grad): recomputes the weights from scores /
    values, nothing saved.  grad_out (B,C,N) f32 -> (grad_scores, grad_values), each (B,C,N,K) or None when not
    needed (at least one must be)."""
    (B, C, N, K), cnt = _req_pool(scores, values, count)
    _req(grad_out, "grad_out", torch.float32)
    _same_device(scores, grad_out)
    if tuple(grad_out.shape) != (B, C, N):
        raise RuntimeError("grad_out must have shape (B, C, N) = (%d, %d, %d), got %s" % (B, C, N, tuple(grad_out.shape)))
    gs = torch.empty_like(scores) if need_scores else None
    gv = torch.empty_like(values) if need_values else None
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().pdr_attention_pool_cf_grad(scores.data_ptr(), values.data_ptr(), _ptr(cnt),
                                                          grad_out.data_ptr(), B, C, N, K, _ptr(gs), _ptr(gv),
                                                          _stream()), "attention_pool_grad")
    return gs, gv


GROUP_NORM_ACTS = ("none", "relu", "swish")      # the `act` codes 0, 1, 2 of pdr_group_norm_act


def _req_group_norm(x, weight, bias, num_groups, act):
    """Shapes and dtypes of group_norm_act's inputs; returns (B, C, S, G, act code)."""
    _req(x, "x", torch.float32)
    if x.dim() < 2:
        raise RuntimeError("group_norm_act: x must be (B, C, ...), got %s" % (tuple(x.shape),))
    if act not in GROUP_NORM_ACTS:
        raise ValueError("group_norm_act: act must be one of %s, got %r" % (GROUP_NORM_ACTS, act))
    B, C, G = int(x.shape[0]), int(x.shape[1]), int(num_groups)
    S = 1
    for d in x.shape[2:]:
        S *= int(d)
    if (weight is None) != (bias is None):
        raise RuntimeError("group_norm_act: weight and bias must both be given or both be None")
    if weight is not None:
        cn = C - C % G if G > 0 else -1
        for t, name in ((weight, "weight"), (bias, "bias")):
            _req(t, name, torch.float32)
            _same_device(x, t)
            if tuple(t.shape) != (cn,):
                raise RuntimeError("%s must have shape (C - C %% G,) = (%d,), got %s" % (name, cn, tuple(t.shape)))
    return B, C, S, G, GROUP_NORM_ACTS.index(act)


def _group_norm_workspace(B, C, S, G, device):
    nbytes = _lib.load().pdr_group_norm_act_workspace_bytes(B, C, S, G)
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def group_norm_act_supported(shape, num_groups):
    """Whether pdr_group_norm_act takes an x of this shape (B, C, ...): at least `num_groups` channels, fewer than 2^31
    elements."""
    if len(shape) < 2:
        return False
    n = 1
    for d in shape:
        n *= int(d)
    return 0 < int(num_groups) <= int(shape[1]) and n < 2 ** 31


def group_norm_act(x, weight, bias, num_groups, eps=1e-5, act="none"):
    """act(MyGroupNorm(x)) in two launches (pdr_group_norm_act): x (B, C, ...) f32, weight / bias (C - C % G) f32 or
    both None -> (y like x, mean (B, G), rstd (B, G)).  Channels past C - C % G are not normalised; the activation
    ('none' | 'relu' | 'swish') applies to all."""
    B, C, S, G, code = _req_group_norm(x, weight, bias, num_groups, act)
    y = torch.empty_like(x)
    mean = torch.empty((B, max(G, 0)), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = _group_norm_workspace(B, C, S, G, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_group_norm_act(x.data_ptr(), _ptr(weight), _ptr(bias), B, C, S, G, float(eps), code,
                                                  y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(),
                                                  _stream()), "group_norm_act")
    return y, mean, rstd


def group_norm_act_grad(x, weight, bias, mean, rstd, grad_y, num_groups, act="none", need_x=True, need_weight=True,
                        need_bias=True):
    """Backward of group_norm_act in three launches (pdr_group_norm_act_grad): recomputes z from x and the saved (B, G)
    statistics.  -> (grad_x, grad_weight, grad_bias), None where not needed (at least one must be; without weight /
    bias the last two are always None)."""
    B, C, S, G, code = _req_group_norm(x, weight, bias, num_groups, act)
    _req(grad_y, "grad_y", torch.float32)
    if grad_y.shape != x.shape:
        raise RuntimeError("grad_y must have x's shape %s, got %s" % (tuple(x.shape), tuple(grad_y.shape)))
    for t, name in ((mean, "mean"), (rstd, "rstd")):
        _req(t, name, torch.float32)
        if tuple(t.shape) != (B, G):
            raise RuntimeError("%s must have shape (B, G) = (%d, %d), got %s" % (name, B, G, tuple(t.shape)))
    _same_device(x, grad_y, mean, rstd)
    gx = torch.empty_like(x) if need_x else None
    gw = torch.empty_like(weight) if need_weight and weight is not None else None
    gb = torch.empty_like(bias) if need_bias and bias is not None else None
    ws = _group_norm_workspace(B, C, S, G, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_group_norm_act_grad(x.data_ptr(), _ptr(weight), _ptr(bias), mean.data_ptr(),
                                                       rstd.data_ptr(), grad_y.data_ptr(), B, C, S, G, code, _ptr(gx),
                                                       _ptr(gw), _ptr(gb), ws.data_ptr(), _stream()),
                   "group_norm_act_grad")
    return gx, gw, gb


def _req_injection(x, B, C, add, residual):
    """Shapes and dtypes of group_norm_act_add's optional terms: add (B, C), residual of x's shape."""
    if add is not None:
        _req(add, "add", torch.float32)
        _same_device(x, add)
        if tuple(add.shape) != (B, C):
            raise RuntimeError("add must have shape (B, C) = (%d, %d), got %s" % (B, C, tuple(add.shape)))
    if residual is not None:
        _req(residual, "residual", torch.float32)
        _same_device(x, residual)
        if residual.shape != x.shape:
            raise RuntimeError("residual must have x's shape %s, got %s" % (tuple(x.shape), tuple(residual.shape)))


def group_norm_act_add(x, weight, bias, num_groups, eps=1e-5, act="none", add=None, residual=None):
    """(act(MyGroupNorm(x)) + add[:, :, None]) + residual in the two launches of group_norm_act
    (pdr_group_norm_act_add): x, weight, bias as there, add (B, C) f32 or None, residual like x or None ->
    (y like x, mean (B, G), rstd (B, G)).  mean and rstd have group_norm_act's bits, y those of its y followed by the
    two fp32 additions in that order; a term that is None is skipped."""
    B, C, S, G, code = _req_group_norm(x, weight, bias, num_groups, act)
    _req_injection(x, B, C, add, residual)
    y = torch.empty_like(x)
    mean = torch.empty((B, max(G, 0)), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = _group_norm_workspace(B, C, S, G, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_group_norm_act_add(x.data_ptr(), _ptr(weight), _ptr(bias), _ptr(add), _ptr(residual),
                                                      B, C, S, G, float(eps), code, y.data_ptr(), mean.data_ptr(),
                                                      rstd.data_ptr(), ws.data_ptr(), _stream()), "group_norm_act_add")
    return y, mean, rstd


def group_norm_act_add_grad(x, weight, bias, mean, rstd, grad_y, num_groups, act="none", need_x=True, need_weight=True,
                            need_bias=True, need_add=True):
    """Backward of group_norm_act_add in the three launches of group_norm_act_grad (pdr_group_norm_act_add_grad); it
    needs neither add nor residual.  -> (grad_x, grad_weight, grad_bias, grad_add (B, C)), None where not needed (at
    least one must be).  The first three have group_norm_act_grad's bits; grad_add is the row sum of grad_y, in double
    in the row kernel's order, rounded once.  The residual's gradient is grad_y itself."""
    B, C, S, G, code = _req_group_norm(x, weight, bias, num_groups, act)
    _req(grad_y, "grad_y", torch.float32)
    if grad_y.shape != x.shape:
        raise RuntimeError("grad_y must have x's shape %s, got %s" % (tuple(x.shape), tuple(grad_y.shape)))
    for t, name in ((mean, "mean"), (rstd, "rstd")):
        _req(t, name, torch.float32)
        if tuple(t.shape) != (B, G):
            raise RuntimeError("%s must have shape (B, G) = (%d, %d), got %s" % (name, B, G, tuple(t.shape)))
    _same_device(x, grad_y, mean, rstd)
    gx = torch.empty_like(x) if need_x else None
    gw = torch.empty_like(weight) if need_weight and weight is not None else None
    gb = torch.empty_like(bias) if need_bias and bias is not None else None
    ge = torch.empty((B, C), dtype=torch.float32, device=x.device) if need_add else None
    if B * C * S == 0 and ge is not None:                    # the empty problem launches nothing: a sum of nothing
        ge.zero_()
    ws = _group_norm_workspace(B, C, S, G, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_group_norm_act_add_grad(x.data_ptr(), _ptr(weight), _ptr(bias), mean.data_ptr(),
                                                           rstd.data_ptr(), grad_y.data_ptr(), B, C, S, G, code,
                                                           _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ge), ws.data_ptr(),
                                                           _stream()), "group_norm_act_add_grad")
    return gx, gw, gb, ge


def _req_relu_group_norm(q, k, weight, bias, num_groups):
    """Shapes and dtypes of relu_group_norm's inputs; returns (B, C1, C2, N, K, G)."""
    _req(k, "k", torch.float32)
    if k.dim() != 4:
        raise RuntimeError("relu_group_norm: k must be (B, C2, N, K), got %s" % (tuple(k.shape),))
    B, C2, N, K = (int(d) for d in k.shape)
    C1, G = 0, int(num_groups)
    if q is not None:
        _req(q, "q", torch.float32)
        _same_device(k, q)
        if q.dim() != 3 or int(q.shape[0]) != B or int(q.shape[2]) != N:
            raise RuntimeError("q must have shape (B, C1, N) = (%d, C1, %d), got %s" % (B, N, tuple(q.shape)))
        C1 = int(q.shape[1])
    if (weight is None) != (bias is None):
        raise RuntimeError("relu_group_norm: weight and bias must both be given or both be None")
    if weight is not None:
        C = C1 + C2
        cn = C - C % G if G > 0 else -1
        for t, name in ((weight, "weight"), (bias, "bias")):
            _req(t, name, torch.float32)
            _same_device(k, t)
            if tuple(t.shape) != (cn,):
                raise RuntimeError("%s must have shape (C - C %% G,) = (%d,), got %s" % (name, cn, tuple(t.shape)))
    return B, C1, C2, N, K, G


def _relu_group_norm_workspace(B, C1, C2, N, K, G, device):
    nbytes = _lib.load().pdr_relu_group_norm_cf_workspace_bytes(B, C1, C2, N, K, G)
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def relu_group_norm_supported(C1, k_shape, num_groups):
    """Whether pdr_relu_group_norm_cf takes q (B, C1, N) (C1 = 0: no q) with k of shape (B, C2, N, K): at least one k
    channel, at least `num_groups` channels in all, fewer than 2^31 output elements and fewer than 2^24 (b, c) rows."""
    if len(k_shape) != 4:
        return False
    B, C2, N, K = (int(d) for d in k_shape)
    C = int(C1) + C2
    return int(C1) >= 0 and C2 >= 1 and 0 < int(num_groups) <= C and B * C < 2 ** 24 and B * C * N * K < 2 ** 31


def relu_group_norm(q, k, weight, bias, num_groups, eps=1e-5):
    """MyGroupNorm(relu(cat([q broadcast over K, k], 1))) in two launches (pdr_relu_group_norm_cf) without the cat:
    q (B, C1, N) f32 or None, k (B, C2, N, K) f32, weight / bias (C - C % G) f32 or both None, C = C1 + C2
    -> (y (B, C, N, K), mean (B, G), rstd (B, G)).  Channels past C - C % G are not normalised (ReLU only)."""
    B, C1, C2, N, K, G = _req_relu_group_norm(q, k, weight, bias, num_groups)
    y = torch.empty((B, C1 + C2, N, K), dtype=torch.float32, device=k.device)
    mean = torch.empty((B, max(G, 0)), dtype=torch.float32, device=k.device)
    rstd = torch.empty_like(mean)
    ws = _relu_group_norm_workspace(B, C1, C2, N, K, G, k.device)
    with torch.cuda.device(k.device):
        _lib.check(_lib.load().pdr_relu_group_norm_cf(_ptr(q), k.data_ptr(), _ptr(weight), _ptr(bias), B, C1, C2, N, K,
                                                      G, float(eps), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                      ws.data_ptr(), _stream()), "relu_group_norm")
    return y, mean, rstd


def relu_group_norm_grad(q, k, weight, bias, mean, rstd, grad_y, num_groups, need_q=True, need_k=True,
                         need_weight=True, need_bias=True):
    """Backward of relu_group_norm in up to four launches (pdr_relu_group_norm_cf_grad): recomputes the normalised
    values from q, k and the saved (B, G) statistics.  -> (grad_q, grad_k, grad_weight, grad_bias), None where not
    needed (at least one must be; without q / weight / bias theirs are always None)."""
    B, C1, C2, N, K, G = _req_relu_group_norm(q, k, weight, bias, num_groups)
    _req(grad_y, "grad_y", torch.float32)
    if tuple(grad_y.shape) != (B, C1 + C2, N, K):
        raise RuntimeError("grad_y must have shape (B, C1 + C2, N, K) = %s, got %s"
                           % ((B, C1 + C2, N, K), tuple(grad_y.shape)))
    for t, name in ((mean, "mean"), (rstd, "rstd")):
        _req(t, name, torch.float32)
        if tuple(t.shape) != (B, G):
            raise RuntimeError("%s must have shape (B, G) = (%d, %d), got %s" % (name, B, G, tuple(t.shape)))
    _same_device(k, grad_y, mean, rstd)
    gq = torch.empty_like(q) if need_q and C1 > 0 else None
    gk = torch.empty_like(k) if need_k else None
    gw = torch.empty_like(weight) if need_weight and weight is not None else None
    gb = torch.empty_like(bias) if need_bias and bias is not None else None
    ws = _relu_group_norm_workspace(B, C1, C2, N, K, G, k.device)
    with torch.cuda.device(k.device):
        _lib.check(_lib.load().pdr_relu_group_norm_cf_grad(_ptr(q), k.data_ptr(), _ptr(weight), _ptr(bias),
                                                           mean.data_ptr(), rstd.data_ptr(), grad_y.data_ptr(), B, C1,
                                                           C2, N, K, G, _ptr(gq), _ptr(gk), _ptr(gw), _ptr(gb),
                                                           ws.data_ptr(), _stream()), "relu_group_norm_grad")
    return gq, gk, gw, gb


def _req_relu_group_norm_conv(q, k, weight, bias, num_groups, conv_weight, conv_bias):
    """Shapes and dtypes of relu_group_norm_conv's inputs; returns (B, C1, C2, N, K, G, Cout)."""
    B, C1, C2, N, K, G = _req_relu_group_norm(q, k, weight, bias, num_groups)
    _req(conv_weight, "conv_weight", torch.float32)
    _same_device(k, conv_weight)
    if conv_weight.dim() != 2 or int(conv_weight.shape[1]) != C1 + C2:
        raise RuntimeError("conv_weight must have shape (Cout, C1 + C2) = (Cout, %d), got %s"
                           % (C1 + C2, tuple(conv_weight.shape)))
    Cout = int(conv_weight.shape[0])
    if conv_bias is not None:
        _req(conv_bias, "conv_bias", torch.float32)
        _same_device(k, conv_bias)
        if tuple(conv_bias.shape) != (Cout,):
            raise RuntimeError("conv_bias must have shape (Cout,) = (%d,), got %s" % (Cout, tuple(conv_bias.shape)))
    return B, C1, C2, N, K, G, Cout


def _relu_group_norm_conv_workspace(B, C1, C2, N, K, G, Cout, device):
    nbytes = _lib.load().pdr_relu_group_norm_conv_cf_workspace_bytes(B, C1, C2, N, K, G, Cout)
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def relu_group_norm_conv_supported(C1, k_shape, num_groups, Cout):
    """Whether pdr_relu_group_norm_conv_cf and its two gradients take q (B, C1, N) (C1 = 0: no q), k of shape
    (B, C2, N, K) and a (Cout, C1 + C2) weight: what relu_group_norm_supported asks, at most 1024 channels on either
    side of the convolution, at most 4095 clouds and fewer than 2^31 output elements."""
    if not relu_group_norm_supported(C1, k_shape, num_groups):
        return False
    B, C2, N, K = (int(d) for d in k_shape)
    Cout = int(Cout)
    return 1 <= Cout <= 1024 and int(C1) + C2 <= 1024 and B <= 4095 and B * Cout * N * K < 2 ** 31


def relu_group_norm_conv(q, k, weight, bias, num_groups, eps, conv_weight, conv_bias):
    """conv1x1(MyGroupNorm(relu(cat([q broadcast over K, k], 1)))) in three launches (pdr_relu_group_norm_conv_cf)
    without the cat and without the normalised tensor: q, k, weight, bias as relu_group_norm, conv_weight (Cout, C)
    f32, conv_bias (Cout) f32 or None -> (out (B, Cout, N, K), mean (B, G), rstd (B, G))."""
    B, C1, C2, N, K, G, Cout = _req_relu_group_norm_conv(q, k, weight, bias, num_groups, conv_weight, conv_bias)
    out = torch.empty((B, Cout, N, K), dtype=torch.float32, device=k.device)
    mean = torch.empty((B, max(G, 0)), dtype=torch.float32, device=k.device)
    rstd = torch.empty_like(mean)
    ws = _relu_group_norm_conv_workspace(B, C1, C2, N, K, G, Cout, k.device)
    with torch.cuda.device(k.device):
        _lib.check(_lib.load().pdr_relu_group_norm_conv_cf(_ptr(q), k.data_ptr(), _ptr(weight), _ptr(bias),
                                                           conv_weight.data_ptr(), _ptr(conv_bias), B, C1, C2, N, K, G,
                                                           Cout, float(eps), out.data_ptr(), mean.data_ptr(),
                                                           rstd.data_ptr(), ws.data_ptr(), _stream()),
                   "relu_group_norm_conv")
    return out, mean, rstd


def relu_group_norm_conv_grad_input(conv_weight, grad_out):
    """grad_out (B, Cout, N, K) f32, conv_weight (Cout, C) f32 -> the gradient (B, C, N, K) of the normalised tensor
    (pdr_relu_group_norm_conv_cf_grad_input, one launch): what relu_group_norm_grad takes as grad_y."""
    _req(conv_weight, "conv_weight", torch.float32)
    _req(grad_out, "grad_out", torch.float32)
    _same_device(grad_out, conv_weight)
    if conv_weight.dim() != 2 or grad_out.dim() != 4 or int(grad_out.shape[1]) != int(conv_weight.shape[0]):
        raise RuntimeError("relu_group_norm_conv_grad_input: conv_weight (Cout, C) and grad_out (B, Cout, N, K), got "
                           "%s and %s" % (tuple(conv_weight.shape), tuple(grad_out.shape)))
    B, Cout, N, K = (int(d) for d in grad_out.shape)
    C = int(conv_weight.shape[1])
    gxn = torch.empty((B, C, N, K), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().pdr_relu_group_norm_conv_cf_grad_input(conv_weight.data_ptr(), grad_out.data_ptr(), B, C,
                                                                      N, K, Cout, gxn.data_ptr(), _stream()),
                   "relu_group_norm_conv_grad_input")
    return gxn


def relu_group_norm_conv_grad_weight(q, k, weight, bias, mean, rstd, grad_out, num_groups, need_weight=True,
                                     need_bias=True, return_partials=False):
    """Gradients of the convolution's weight (Cout, C) and bias (Cout) (pdr_relu_group_norm_conv_cf_grad_weight): the
    normalised values are recomputed from q, k and the saved (B, G) statistics.  -> (grad_conv_weight,
    grad_conv_bias), None where not needed (at least one must be).  return_partials=True appends the fp32 partials
    (B, R, Cout, C) the fold added up (a view of the call's workspace; None without the weight gradient)."""
    B, C1, C2, N, K, G = _req_relu_group_norm(q, k, weight, bias, num_groups)
    _req(grad_out, "grad_out", torch.float32)
    if grad_out.dim() != 4 or tuple(grad_out.shape[0:1] + grad_out.shape[2:]) != (B, N, K):
        raise RuntimeError("grad_out must have shape (B, Cout, N, K) = (%d, Cout, %d, %d), got %s"
                           % (B, N, K, tuple(grad_out.shape)))
    Cout = int(grad_out.shape[1])
    for t, name in ((mean, "mean"), (rstd, "rstd")):
        _req(t, name, torch.float32)
        if tuple(t.shape) != (B, G):
            raise RuntimeError("%s must have shape (B, G) = (%d, %d), got %s" % (name, B, G, tuple(t.shape)))
    _same_device(k, grad_out, mean, rstd)
    C = C1 + C2
    gw = torch.empty((Cout, C), dtype=torch.float32, device=k.device) if need_weight else None
    gb = torch.empty((Cout,), dtype=torch.float32, device=k.device) if need_bias else None
    if B * N * K == 0:                                        # the empty problem launches nothing: a sum of nothing
        for t in (gw, gb):
            if t is not None:
                t.zero_()
    ws = _relu_group_norm_conv_workspace(B, C1, C2, N, K, G, Cout, k.device)
    with torch.cuda.device(k.device):
        _lib.check(_lib.load().pdr_relu_group_norm_conv_cf_grad_weight(_ptr(q), k.data_ptr(), _ptr(weight), _ptr(bias),
                                                                       mean.data_ptr(), rstd.data_ptr(),
                                                                       grad_out.data_ptr(), B, C1, C2, N, K, G, Cout,
                                                                       _ptr(gw), _ptr(gb), ws.data_ptr(), _stream()),
                   "relu_group_norm_conv_grad_weight")
    if not return_partials:
        return gw, gb
    parts = None
    if gw is not None and B * N * K > 0:
        R = relu_group_norm_conv_plan(C1, C2, N, K, G, Cout)["R"]
        parts = ws.view(torch.float32)[:B * R * Cout * C].view(B, R, Cout, C)
    return gw, gb, parts


def relu_group_norm_conv_plan(C1, C2, N, K, num_groups, Cout, aligned16=True):
    """pdr_relu_group_norm_conv_cf_plan as a dict: family (0 scalar, 1 vector), P, E, Cg (the statistics plan), tile
    (positions per workgroup of the GEMMs), L (positions per weight-gradient chain), R (ranges per cloud), rows
    (output rows per workgroup of the forward GEMM)."""
    out = (ctypes.c_long * 8)()
    _lib.check(_lib.load().pdr_relu_group_norm_conv_cf_plan(int(C1), int(C2), int(N), int(K), int(num_groups), int(Cout),
                                                            int(bool(aligned16)), out), "relu_group_norm_conv_plan")
    return dict(zip(("family", "P", "E", "Cg", "tile", "L", "R", "rows"), (int(v) for v in out)))


QUERY_GROUP_USE_XYZ, QUERY_GROUP_ABS, QUERY_GROUP_CENTER = 1, 2, 4     # the `flags` bits of pdr_query_group_cf


def query_group_flags(use_xyz, include_abs_coordinate=False, include_center_coordinate=False):
    """The `flags` word of query_group from the three booleans of QueryAndGroup."""
    return ((QUERY_GROUP_USE_XYZ if use_xyz else 0) | (QUERY_GROUP_ABS if include_abs_coordinate else 0)
            | (QUERY_GROUP_CENTER if include_center_coordinate else 0))


def _query_group_triples(flags):
    if not flags & QUERY_GROUP_USE_XYZ:
        return 0
    return 1 + bool(flags & QUERY_GROUP_ABS) + bool(flags & QUERY_GROUP_CENTER)


def query_group_supported(B, n, m, K, C, flags):
    """Whether pdr_query_group_cf and its backward take these sizes (C: feature channels, 0 or None without features):
    a non-empty problem within the inverse-index builder's limits (n <= 16384, m K <= 2^22, B <= 65535) with fewer
    than 2^31 output elements and at least one output channel."""
    B, n, m, K, C, flags = int(B), int(n), int(m), int(K), int(C or 0), int(flags)
    ctot = C + 3 * _query_group_triples(flags)
    if min(B, n, m, K) <= 0 or C < 0 or not 0 <= flags <= 7 or ctot == 0:
        return False
    return n <= 16384 and m * K <= 2 ** 22 and B <= 65535 and B * ctot * m * K < 2 ** 31


def _req_query_group(idx, counts, B, m):
    _req(idx, "idx", torch.int32)
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != m:
        raise RuntimeError("idx must have shape (B, m, K) = (%d, %d, K), got %s" % (B, m, tuple(idx.shape)))
    if counts is not None:
        _req(counts, "counts", torch.int32)
        _same_device(idx, counts)
        if tuple(counts.shape) != (B, m):
            raise RuntimeError("counts must have shape (B, m) = (%d, %d), got %s" % (B, m, tuple(counts.shape)))


def query_group(xyz, new_xyz, features, idx, counts, flags, out=None):
    """The grouping head of QueryAndGroup in one launch (pdr_query_group_cf): xyz (B,n,3), new_xyz (B,m,3), features
    (B,C,n) or None, idx (B,m,K) i32, counts (B,m) i32 or None (given: queries with counts <= 0 are patched) ->
    (B, C + 3E, m, K) f32 with the channels [features | relative | absolute | centre] that `flags` enables.  `out`: a
    contiguous fp32 tensor of that shape to write into (nothing is allocated then)."""
    _req(xyz, "xyz", torch.float32)
    _req(new_xyz, "new_xyz", torch.float32)
    _req_xyz(xyz, "xyz")
    _req_xyz(new_xyz, "new_xyz")
    _same_device(xyz, new_xyz, idx)
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    if new_xyz.shape[0] != B:
        raise RuntimeError("xyz and new_xyz must have the same batch size")
    _req_query_group(idx, counts, B, m)
    C = 0
    if features is not None:
        _req(features, "features", torch.float32)
        _same_device(xyz, features)
        if features.dim() != 3 or features.shape[0] != B or features.shape[2] != n:
            raise RuntimeError("features must have shape (B, C, n) = (%d, C, %d), got %s" % (B, n, tuple(features.shape)))
        C = int(features.shape[1])
    K, flags = int(idx.shape[2]), int(flags)
    shape = (B, C + 3 * _query_group_triples(flags), m, K)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=xyz.device)
    else:
        _req(out, "out", torch.float32)
        _same_device(xyz, out)
        if tuple(out.shape) != shape:
            raise RuntimeError("out must have shape %s, got %s" % (shape, tuple(out.shape)))
    with torch.cuda.device(xyz.device):
        _lib.check(_lib.load().pdr_query_group_cf(xyz.data_ptr(), new_xyz.data_ptr(), _ptr(features), idx.data_ptr(),
                                                  _ptr(counts), B, n, m, K, C, flags, out.data_ptr(), _stream()),
                   "query_group")
    return out


def query_group_grad(idx, counts, grad_out, n, C, flags, need_features=True, need_xyz=True, need_new_xyz=True):
    """Backward of query_group with a fixed summation order (pdr_query_group_cf_grad): idx, counts, flags as in the
    forward, grad_out (B, C + 3E, m, K), n the cloud size, C the feature channels (0 without features) ->
    (grad_features (B,C,n), grad_xyz (B,n,3), grad_new_xyz (B,m,3)), None where not needed (at least one must be;
    grad_features is None when C == 0)."""
    _req(grad_out, "grad_out", torch.float32)
    if grad_out.dim() != 4:
        raise RuntimeError("grad_out must be (B, C + 3E, m, K), got %s" % (tuple(grad_out.shape),))
    B, ctot, m, K = (int(d) for d in grad_out.shape)
    _req_query_group(idx, counts, B, m)
    _same_device(grad_out, idx)
    n, C, flags = int(n), int(C), int(flags)
    if idx.shape[2] != K or ctot != C + 3 * _query_group_triples(flags):
        raise RuntimeError("grad_out %s does not match idx %s, C = %d and flags = %d"
                           % (tuple(grad_out.shape), tuple(idx.shape), C, flags))
    dev = grad_out.device
    gf = torch.empty((B, C, n), dtype=torch.float32, device=dev) if need_features and C > 0 else None
    gx = torch.empty((B, n, 3), dtype=torch.float32, device=dev) if need_xyz else None
    gn = torch.empty((B, m, 3), dtype=torch.float32, device=dev) if need_new_xyz else None
    if B * m * K == 0:                                       # the empty problem writes nothing: every gradient is +0
        for g in (gf, gx, gn):
            if g is not None:
                g.zero_()
    nbytes = _lib.load().pdr_query_group_cf_workspace_bytes(B, n, m, K)
    ws = torch.empty((max(int(nbytes), 4),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pdr_query_group_cf_grad(idx.data_ptr(), _ptr(counts), grad_out.data_ptr(), B, n, m, K, C,
                                                       flags, _ptr(gf), _ptr(gx), _ptr(gn), ws.data_ptr(), _stream()),
                   "query_group_grad")
    return gf, gx, gn


KNN_GROUP_GEO = 11                # d2 | w | nn_abs (3) | nn_rel (3) | x (3): the channels group_knn adds to the features


def knn_group_cf_supported(B, n1, n2, K, C):
    """Whether pdr_knn_group_cf and its backward take these sizes (C: feature channels, 0 or None without features):
    a non-empty problem within the inverse-index builder's limits (n2 <= 16384, n1 K <= 2^22, B <= 65535) with fewer
    than 2^31 output elements and at most 524272 feature channels (the slabs of 8 are one grid dimension)."""
    B, n1, n2, K, C = int(B), int(n1), int(n2), int(K), int(C or 0)
    if min(B, n1, n2, K) <= 0 or C < 0:
        return False
    return (n2 <= 16384 and n1 * K <= 2 ** 22 and B <= 65535 and B * (C + KNN_GROUP_GEO) * n1 * K < 2 ** 31
            and C <= 8 * 65534)


def _req_knn_group_cf(x, y, idx, dists):
    _req(x, "x", torch.float32)
    _req(y, "y", torch.float32)
    _req_xyz(x, "x")
    _req_xyz(y, "y")
    _req(idx, "idx", torch.int32)
    _req(dists, "dists", torch.float32)
    _same_device(x, y, idx, dists)
    B, n1, _ = x.shape
    if y.shape[0] != B:
        raise RuntimeError("x and y must have the same batch size")
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != n1:
        raise RuntimeError("idx must have shape (B, n1, K) = (%d, %d, K), got %s" % (B, n1, tuple(idx.shape)))
    if dists.shape != idx.shape:
        raise RuntimeError("dists must have idx's shape %s, got %s" % (tuple(idx.shape), tuple(dists.shape)))
    return int(B), int(n1), int(y.shape[1]), int(idx.shape[2])


def knn_group_cf(x, y, features, idx, dists, out=None):
    """The grouping head of group_knn(..., transpose=True) in one launch (pdr_knn_group_cf): x (B,n1,3), y (B,n2,3),
    features (B,C,n2) or None, idx (B,n1,K) i32 and dists (B,n1,K) f32 as `knn_group` returns them ->
    (B, C + 11, n1, K) f32 with the channels [features | d2 | w | nn_abs | nn_rel | x].  `out`: a contiguous fp32 tensor
    of that shape to write into (nothing is allocated then)."""
    B, n1, n2, K = _req_knn_group_cf(x, y, idx, dists)
    C = 0
    if features is not None:
        _req(features, "features", torch.float32)
        _same_device(x, features)
        if features.dim() != 3 or features.shape[0] != B or features.shape[2] != n2:
            raise RuntimeError("features must have shape (B, C, n2) = (%d, C, %d), got %s" % (B, n2, tuple(features.shape)))
        C = int(features.shape[1])
    shape = (B, C + KNN_GROUP_GEO, n1, K)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _req(out, "out", torch.float32)
        _same_device(x, out)
        if tuple(out.shape) != shape:
            raise RuntimeError("out must have shape %s, got %s" % (shape, tuple(out.shape)))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_knn_group_cf(x.data_ptr(), y.data_ptr(), _ptr(features), idx.data_ptr(),
                                                dists.data_ptr(), B, n1, n2, K, C, out.data_ptr(), _stream()),
                   "knn_group_cf")
    return out


def knn_group_cf_grad(x, y, idx, dists, grad_out, C, need_features=True, need_x=True, need_y=True):
    """Backward of knn_group_cf with a fixed summation order (pdr_knn_group_cf_grad): x, y, idx, dists as in the
    forward, grad_out (B, C + 11, n1, K), C the feature channels (0 without features) ->
    (grad_features (B,C,n2), grad_x (B,n1,3), grad_y (B,n2,3)), None where not needed (at least one must be;
    grad_features is None when C == 0)."""
    B, n1, n2, K = _req_knn_group_cf(x, y, idx, dists)
    _req(grad_out, "grad_out", torch.float32)
    _same_device(x, grad_out)
    C = int(C)
    if tuple(grad_out.shape) != (B, C + KNN_GROUP_GEO, n1, K):
        raise RuntimeError("grad_out must be (B, C + 11, n1, K) = %s, got %s"
                           % ((B, C + KNN_GROUP_GEO, n1, K), tuple(grad_out.shape)))
    dev = x.device
    gf = torch.empty((B, C, n2), dtype=torch.float32, device=dev) if need_features and C > 0 else None
    gx = torch.empty((B, n1, 3), dtype=torch.float32, device=dev) if need_x else None
    gy = torch.empty((B, n2, 3), dtype=torch.float32, device=dev) if need_y else None
    if B * n1 * K == 0:                                      # the empty problem writes nothing: every gradient is +0
        for g in (gf, gx, gy):
            if g is not None:
                g.zero_()
    ws = None                                                # the inverse index: grad_x alone builds none
    if gf is not None or gy is not None:
        nbytes = _lib.load().pdr_knn_group_cf_workspace_bytes(B, n1, n2, K)
        ws = torch.empty((max(int(nbytes), 4),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pdr_knn_group_cf_grad(x.data_ptr(), y.data_ptr(), idx.data_ptr(), dists.data_ptr(),
                                                     grad_out.data_ptr(), B, n1, n2, K, C, _ptr(gf), _ptr(gx), _ptr(gy),
                                                     _ptr(ws), _stream()), "knn_group_cf_grad")
    return gf, gx, gy


def chamfer_pairwise(x, y, x_lengths=None, y_lengths=None, symmetric=False):
    """All-pairs Chamfer distance between two sets of clouds in one launch (pdr_chamfer_pairwise):
    (S,n,3), (R,m,3) -> cd (S,R) f32, cd[s,r] = mean_i min_j |x_s,i - y_r,j|^2 + mean_j min_i (the same); not
    differentiable.  `x_lengths` (S,) / `y_lengths` (R,) int64 on the clouds' device: cloud s is x[s, :x_lengths[s]];
    a pair with an empty side gets 0.  symmetric=True is the self-matrix: `y` must be `x` and `y_lengths` `x_lengths`
    (same memory); only the pairs s <= r are evaluated and mirrored."""
    _req(x, "x", torch.float32)
    _req(y, "y", torch.float32)
    _same_device(x, y)
    _req_xyz(x, "x")
    _req_xyz(y, "y")
    _req_lengths(x_lengths, "x_lengths", x)
    _req_lengths(y_lengths, "y_lengths", y)
    S, n, _ = x.shape
    R, m, _ = y.shape
    cd = torch.empty((S, R), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_chamfer_pairwise(x.data_ptr(), y.data_ptr(), _ptr(x_lengths), _ptr(y_lengths), S, R,
                                                    n, m, 1 if symmetric else 0, cd.data_ptr(), _stream()),
                   "chamfer_pairwise")
    return cd


def occupancy_grid(clouds, axis, cell_of, cells, lengths=None, out=None):
    """Occupancy counters of a set of clouds on a voxel grid in one launch (pdr_occupancy_grid): clouds (S,n,3) f32,
    axis (R,) f32 and cell_of (R,R,R) i32 -- the grid tables of set_metrics.grid_tables, on the clouds' device --
    -> (counters (cells,) i32, bernoulli (cells,) i32, skipped (1,) i32).  The kernel ADDS: `out` is such a triple to
    accumulate into (nothing is allocated then); without it the three are allocated as zeros.  `lengths` (S,) int64:
    cloud s is clouds[s, :lengths[s]]."""
    _req(clouds, "clouds", torch.float32)
    _req_xyz(clouds, "clouds")
    _req(axis, "axis", torch.float32)
    _req(cell_of, "cell_of", torch.int32)
    _same_device(clouds, axis, cell_of)
    _req_lengths(lengths, "lengths", clouds)
    R, cells = int(axis.numel()), int(cells)
    if cell_of.numel() != R ** 3:
        raise RuntimeError("cell_of must hold R^3 = %d entries, got %d" % (R ** 3, cell_of.numel()))
    if out is None:
        counters, bernoulli, skipped = (torch.zeros((k,), dtype=torch.int32, device=clouds.device)
                                        for k in (max(cells, 0), max(cells, 0), 1))
    else:
        counters, bernoulli, skipped = out
        for t, name, k in ((counters, "counters", cells), (bernoulli, "bernoulli", cells), (skipped, "skipped", 1)):
            _req(t, name, torch.int32)
            if t.numel() != k:
                raise RuntimeError("%s must hold %d entries, got %d" % (name, k, t.numel()))
        _same_device(clouds, counters, bernoulli, skipped)
    S, n, _ = clouds.shape
    with torch.cuda.device(clouds.device):
        _lib.check(_lib.load().pdr_occupancy_grid(clouds.data_ptr(), _ptr(lengths), S, n, R, axis.data_ptr(),
                                                  cell_of.data_ptr(), cells, counters.data_ptr(),
                                                  bernoulli.data_ptr(), skipped.data_ptr(), _stream()),
                   "occupancy_grid")
    return counters, bernoulli, skipped


def knn_group(x, y, K):
    """knn_points for group_knn in the fused network: (dists (B,n1,K) f32, idx (B,n1,K) i32, weights (B,n1,K) f32)
    with weights = normalised 1 / (d2 + 1e-8) (pointnet2_utils.py:500-503)."""
    _req(x, "x", torch.float32)
    _req(y, "y", torch.float32)
    _same_device(x, y)
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
        raise RuntimeError("knn_group: x (B,n1,3) and y (B,n2,3) with equal batch size required, got %s and %s"
                           % (tuple(x.shape), tuple(y.shape)))
    B, n1, _ = x.shape
    n2 = y.shape[1]
    K = int(K)
    if K > min(n2, 16):
        # outside pdr_knn_group's contract (no padding slots, K <= 16): knn_points pads like pytorch3d (idx -1,
        # distance 0); weights as group_knn computes them from the squared distances
        d, i, _ = knn_points(x, y, K)
        w = 1.0 / (d + 1e-8)
        w = w / w.sum(dim=2, keepdim=True)
        return d, i.clamp(min=0).to(torch.int32), w
    d = torch.empty((B, n1, K), dtype=torch.float32, device=x.device)
    w = torch.empty((B, n1, K), dtype=torch.float32, device=x.device)
    i = torch.empty((B, n1, K), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pdr_knn_group(x.data_ptr(), y.data_ptr(), B, n1, n2, int(K), d.data_ptr(),
                                             i.data_ptr(), w.data_ptr(), _stream()), "knn_group")
    return d, i, w


class _KnnDists(torch.autograd.Function):
    """Differentiable squared distances of knn_points (pytorch3d `_knn_points` backward, norm 2).  With lengths the
    padded queries and slots carry idx -1, which pdr_knn_points_grad skips: padded rows get a zero gradient."""

    @staticmethod
    def forward(ctx, p1, p2, K, lengths1=None, lengths2=None):
        dists, idx, _ = _knn_forward(p1, p2, K, False, lengths1, lengths2)
        ctx.save_for_backward(p1, p2, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    def backward(ctx, grad_dists, _grad_idx):
        p1, p2, idx = ctx.saved_tensors
        g1, g2 = knn_points_grad(p1, p2, idx, grad_dists.contiguous().float(), deterministic=is_deterministic())
        return g1, g2, None, None, None


def knn_points(p1, p2, K, return_nn=False, lengths1=None, lengths2=None):
    """pytorch3d.ops.knn.knn_points on padded clouds:
    (B,n1,3), (B,n2,3) -> (dists (B,n1,K) f32 squared ascending, idx (B,n1,K) i64, nn (B,n1,K,3) | None).
    `lengths1` / `lengths2` ((B,) int64 on the clouds' device, None = full): cloud b searches p2[b, :lengths2[b]] for
    the queries p1[b, :lengths1[b]]; slots beyond lengths2[b] and every slot of a padded query are (0, -1, nn 0).
    With grad enabled and an input that requires it, `dists` (and `nn`, as a gather of p2) are differentiable."""
    _req(p1, "p1", torch.float32)
    _req(p2, "p2", torch.float32)
    _same_device(p1, p2)
    if p1.shape[2] != 3 or p2.shape[2] != 3:
        raise RuntimeError("knn_points: only D=3 is built")
    _req_lengths(lengths1, "lengths1", p1)
    _req_lengths(lengths2, "lengths2", p2)
    if torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad):
        dists, idx = _KnnDists.apply(p1, p2, int(K), lengths1, lengths2)
        nn = None
        if return_nn:
            B, n1, _ = p1.shape
            safe = idx.clamp(min=0).reshape(B, n1 * int(K), 1).expand(-1, -1, 3)
            nn = p2.gather(1, safe).reshape(B, n1, int(K), 3) * (idx >= 0).unsqueeze(-1)
        return dists, idx, nn
    return _knn_forward(p1, p2, K, return_nn, lengths1, lengths2)
