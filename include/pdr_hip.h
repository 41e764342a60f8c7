/*
 * pdr_hip.h -- C ABI of libpdr_hip.so (MI355X / gfx950 native ops of PDR's DDPM
 * reverse-sampling hot path).
 *
 * Drop-in boundary: every entry point below replaces one symbol the reference
 * binds through pybind (paths relative to the reference repository):
 *
 *   pointnet2_ops_lib/pointnet2_ops/_ext-src/src/bindings.cpp:6-19  (9 symbols)
 *   PytorchEMD/cuda/emd.cpp:23-27                                   (3 symbols)
 *   pytorch3d.ops.knn.knn_points (un-vendored dependency; call sites
 *       pointnet2_ops/pointnet2_utils.py:365,496-497 and
 *       pointnet2/chamfer_loss_new.py:149-150)
 *
 * Conventions (differences from the reference are deliberate and listed):
 *   - plain pointers to DEVICE memory + int sizes + a stream handle; no torch
 *     types.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     The reference's EMD launches on the default stream (emd_kernel.cu:191,277);
 *     here every op honours `stream`.
 *   - all tensors are dense, row-major ("contiguous"), fp32 / int32 unless a
 *     parameter says int64.
 *   - outputs are caller-allocated.  Unlike ball_query.cpp:21-27 they need NOT be
 *     zero-initialised: every output element is written by the kernel.
 *   - return value: PDR_OK (0) or a negative PDR_E* code.  Nothing prints or
 *     calls exit() (contrast cuda_utils.h:30-39).  No hidden allocation, no
 *     device synchronisation: calls are thread-safe and capturable into a
 *     hipGraph.  The library never reads the environment (ABI 0.2.0; rounds 1-5
 *     read ten PDR_* variables once per process).  The only process-wide state is
 *     the table of kernel-selection options of pdr_set_option below (which kernel
 *     family / tile shape / tile order runs an op; results are identical, for the
 *     layer kernels and the GroupNorm fold up to fp32 / fp64 summation order).
 *     tests/test_fused_gpu.py::test_ddpm_forward_with_every_non_default_variant runs
 *     the full DDPM forward under each of them.
 *   - validation covers pointers, sizes and alignment; VALUES are not inspected
 *     (an out-of-range index in a caller-provided idx array is undefined
 *     behaviour, as in the reference's kernels).
 *   - int32 indexing: B*C*N*nsample must stay below 2^31 (same as reference).
 */
#ifndef PDR_HIP_H
#define PDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDR_OK 0
#define PDR_EINVAL (-1)      /* null pointer / non-positive size / bad argument */
#define PDR_EUNSUPPORTED (-2) /* size outside what the kernels were built for */
#define PDR_ELAUNCH (-3)     /* hipGetLastError() != hipSuccess after launch  */

typedef void *pdr_stream_t; /* hipStream_t */

/* library version: major*10000 + minor*100 + patch.  A caller built against another minor version must not call the
 * entry points listed for it below (the Python binding refuses to load a library of another version).
 *   0.1.0 (100)  rounds 1-4.
 *   0.2.0 (200)  round 5 grew three signatures without a bump: pdr_reverse_step gained probe_acc / probe_out
 *                before `stream`, pdr_gn_fold gained nvalid_a / tpb_main_a / nvalid_b / tpb_main_b, pdr_layer_in_t gained
 *                wrow0 / wmul / patch_values / patch_ld / patch_w before `reserved_`; round 6: pdr_layer_in_t.oadd_rows, probe_out is a 4-slot ring
 *                (int[16]), pdr_set_option replaces the environment knobs, pdr_point_chain / pdr_point_chain_plan /
 *                pdr_fused_layer_pair are new; pdr_knn_points_ragged / pdr_chamfer_nn_ragged are new; pdr_approxmatch_ragged /
 *                pdr_emd_cost_ragged / pdr_matchcost_ragged / pdr_matchcost_grad_ragged are new; pdr_emd_cost_grad /
 *                pdr_emd_cost_grad_ragged are new; pdr_chamfer_pairwise is new; pdr_fps_plan / pdr_knn_plan /
 *                pdr_ball_query_plan (host-only dispatch queries) are new; pdr_gather_plan (the same for
 *                pdr_gather_add* / pdr_gather_moments*) is new; pdr_occupancy_grid is new; pdr_fused_layer_pool_plan (the same
 *                for the two pooled entry points) is new; pdr_scatter_workspace_bytes and the four deterministic backward
 *                twins pdr_*_grad_det are new; pdr_chamfer_loss_workspace_bytes / pdr_chamfer_loss / pdr_chamfer_loss_grad
 *                are new; pdr_fps_ragged_workspace_bytes / pdr_fps_ragged_plan / pdr_furthest_point_sampling_ragged are
 *                new; pdr_attention_pool_cf_plan / pdr_attention_pool_cf / pdr_attention_pool_cf_grad are new;
 *                pdr_group_norm_act_workspace_bytes / pdr_group_norm_act_plan / pdr_group_norm_act /
 *                pdr_group_norm_act_grad are new; pdr_query_group_cf_workspace_bytes / pdr_query_group_cf_plan /
 *                pdr_query_group_cf / pdr_query_group_cf_grad are new; pdr_knn_group_cf_workspace_bytes /
 *                pdr_knn_group_cf_plan / pdr_knn_group_cf / pdr_knn_group_cf_grad are new;
 *                pdr_relu_group_norm_cf_workspace_bytes / pdr_relu_group_norm_cf_plan / pdr_relu_group_norm_cf /
 *                pdr_relu_group_norm_cf_grad are new; pdr_group_norm_act_add / pdr_group_norm_act_add_grad are new;
 *                pdr_relu_group_norm_conv_cf_workspace_bytes / pdr_relu_group_norm_conv_cf_plan /
 *                pdr_relu_group_norm_conv_cf / pdr_relu_group_norm_conv_cf_grad_input /
 *                pdr_relu_group_norm_conv_cf_grad_weight are new. */
int pdr_version(void);
/* last hip error string seen by this thread after a PDR_ELAUNCH ("" if none) */
const char *pdr_last_error(void);
/* Kernel-selection options (process-wide, relaxed atomics; set them before capturing a hipGraph -- a captured launch
 * keeps the kernel it was captured with).  Unknown name / value out of range: PDR_EINVAL.
 *   name            default  values
 *   fused_ws           1     0: uniform-wave layer kernels instead of the wave-specialised ones
 *   narrow_kc32        1     0: 256-row tiles for outputs of <= 64 channels (see pdr_fused_layer_tile_rows)
 *   fps_wave           1     rank-ordered one-wave FPS kernel: 0 never, 1 up to 256 points, 2 up to 4096
 *   fps_lean           1     0: the round-1 resident FPS kernel instead of the instruction-lean one
 *   knn_wave           1     0: thread-per-query instead of wave-per-query kNN for K <= 8
 *   gn_fold_small      1     0: 1024-thread GroupNorm fold workgroups
 *   ws_narrow3         1     0: two instead of three co-resident workgroups per CU for the 128 x 32 tiles
 *   ws_xcd_order       1     tile order of the layer kernels: 0 plain, 1 XCD-local for the gathered ones, 2 for all
 *   deep_chunks        1     0: the tiny per-point layers of the deep levels on the ordinary tiles (pdr_fused_layer_plan)
 *   deep_ks            1     0: those layers without the K split among a workgroup's waves
 *   deep_jobs32      256     a layer on 32-row tiles is right-sized when it has at most this many 32 x 128 jobs
 *   deep_jobs64      512     ... on 64-row tiles: at most this many 64 x 64 jobs
 * pdr_option_name(i): name of option i (0 <= i < number of options), NULL beyond -- lets a binding enumerate them. */
int pdr_set_option(const char *name, int value);
int pdr_get_option(const char *name, int *value);
const char *pdr_option_name(int index);

/* include/cuda_utils.h:13-19 opt_n_threads(): min(2^floor(log2 x), 512).  The FPS
 * tie order depends on this value; exported so callers and
 * tests can reproduce it. */
int pdr_opt_n_threads(int work_size);

/* ---- furthest point sampling ------------------------------------------------
 * replaces furthest_point_sampling(points, nsamples)  (sampling.cpp:66-87,
 * kernel sampling_gpu.cu:69-173).
 *   xyz (B,N,3) f32  ->  idx (B,m) i32, idx[:,0] = 0.
 * `temp` is the reference's (B,N) f32 scratch (sampling.cpp:74-76); this
 * implementation keeps the running distances in registers and needs it only when
 * pdr_fps_workspace_bytes() > 0 (N beyond the register-resident limit); pass NULL
 * otherwise.  Index-exact w.r.t. the reference kernel's block-size-dependent tie
 * order and its |p|^2 <= 1e-3 exclusion. */
size_t pdr_fps_workspace_bytes(int B, int N);
int pdr_furthest_point_sampling(const float *xyz, int B, int N, int m,
                                float *temp, int *idx, pdr_stream_t stream);
/* Which kernel pdr_furthest_point_sampling runs for a cloud of N points under the current fps_wave / fps_lean options.
 * Host only (no HIP call, no device pointer); the launch reads the same decision, so the kernel that runs is the one
 * reported.  out = {family (0 resident, 1 wave, 2 lean, 3 stream), threads per cloud T, points per thread PPT (0: the
 * stream kernel strides), slots = R Q with R = pdr_opt_n_threads(N), Q = ceil(N / R)}.  N <= 0: PDR_EINVAL. */
int pdr_fps_plan(int N, int out[4]);

/* Furthest point sampling of a PADDED batch with per-cloud lengths, optionally of every cloud together with its mirror
 * image, in ONE launch that also writes the picked rows (the length-aware, mirroring form of the call above;
 * pytorch3d's sample_farthest_points(lengths=...) with the reference kernel's tie order).
 *   xyz (B,N,3) f32, lengths (B) i64 or NULL  ->  idx (B,m) i32, rows (B,m,4) f32 (may be NULL; 16-byte aligned)
 *   - lengths follows pdr_knn_points_ragged: an int64 array of B entries in DEVICE memory, read only by the kernel and
 *     clamped there to [0, N]; NULL = every cloud is full; N stays the row stride.  The host never reads it, so the call
 *     neither synchronises nor allocates, is one launch and is capturable: a replayed graph follows the lengths then in
 *     memory.
 *   - mirror_axis is -1 (no mirror) or 0 / 1 / 2.  Cloud b is a VIRTUAL cloud of V_b = L_b points, or 2 L_b with a
 *     mirror: virtual point k < L_b is xyz[b,k], virtual point k >= L_b is xyz[b,k-L_b] with the sign bit of coordinate
 *     mirror_axis flipped (what `partial * sign` gives, -0.0 included).  Nothing of size 2N is materialised.
 *   - idx holds the picks as virtual indices; row j of `rows` is the picked virtual point's (x, y, z, tag), tag = +1 for
 *     an original and -1 for a mirrored point (+1 without a mirror).
 *   - row b of idx is, index for index, what pdr_furthest_point_sampling returns for the materialised virtual cloud
 *     (1, V_b, 3) and the same m: the tie order (which does not depend on the length: for every N the reference's rank
 *     is the order of the key (bitrev9(k % 512), k / 512)), the |p|^2 <= 1e-3 exclusion, "all excluded -> 0", m > V_b
 *     (rounds after exhaustion are ties at the current maximum) and idx[b,0] = 0.
 *   - rows at or beyond a length are never read for their value (NaN included); a cloud of length 0 gets idx = -1 and
 *     rows = 0 in every slot; every output element is written exactly once; the same input gives the same bits, and no
 *     option of pdr_set_option changes which kernel runs.
 *   - two forms, chosen on the host from V = N * (mirror ? 2 : 1) and reported by pdr_fps_ragged_plan (host only; the
 *     launch reads the same decision): out = {family (0 resident, 1 stream), threads per cloud, points per thread (0:
 *     the stream kernel strides), dynamic LDS bytes}.  Resident (V <= 12288): no workspace, the cloud in LDS, running
 *     distances in registers, one workgroup per cloud; the reported points per thread are the launch's maximum -- every
 *     workgroup runs the loop built for ceil(V_b / threads) rounded up to 2, 4, 8, 12 or 16, so a short cloud does not
 *     pay for N.  Stream (above): running distances in `temp`, pdr_fps_ragged_workspace_bytes = B * V floats.
 *   - validation, on the host before any launch, in this order: B < 0, N <= 0, m < 0 or mirror_axis outside [-1, 2]:
 *     PDR_EINVAL; B == 0 or m == 0: PDR_OK, nothing launched, no pointer looked at; V > 2^20 or B * max(V, m) >= 2^31:
 *     PDR_EUNSUPPORTED; NULL xyz / idx, a NULL temp where the workspace size is positive, or a misaligned rows:
 *     PDR_EINVAL.  The workspace query returns 0 for B <= 0 and for sizes the call refuses. */
size_t pdr_fps_ragged_workspace_bytes(int B, int N, int mirror_axis);
int pdr_fps_ragged_plan(int N, int mirror_axis, int out[4]);
int pdr_furthest_point_sampling_ragged(const float *xyz, const int64_t *lengths, int B, int N, int mirror_axis, int m,
                                       float *temp, int *idx, float *rows, pdr_stream_t stream);

/* ---- gather -----------------------------------------------------------------
 * gather_points(points (B,C,N), idx (B,m)) -> out (B,C,m)   sampling.cpp:15-38
 * gather_points_grad(grad_out (B,C,m), idx, n) -> grad_points (B,C,N)  :40-64
 * (grad_points is fully written: zero-filled, then scatter-added) */
int pdr_gather_points(const float *points, const int *idx, int B, int C, int N,
                      int m, float *out, pdr_stream_t stream);
int pdr_gather_points_grad(const float *grad_out, const int *idx, int B, int C,
                           int N, int m, float *grad_points, pdr_stream_t stream);

/* ---- ball query -------------------------------------------------------------
 * ball_query(new_xyz (B,m,3), xyz (B,n,3), radius, nsample)
 *      -> idx (B,m,nsample) i32, counts (B,m) i32      ball_query.cpp:10-38,
 * kernel ball_query_gpu.cu:9-47.  NOTE argument order: queries first. */
int pdr_ball_query(const float *new_xyz, const float *xyz, int B, int n, int m,
                   float radius, int nsample, int *idx, int *counts,
                   pdr_stream_t stream);
/* Which instantiation pdr_ball_query runs for these sizes (host only, read by the launch itself):
 * out = {NCH (64-point cloud slots per lane), resident (1: n <= 64 NCH, the cloud lives in registers; 0: the streaming
 * kernel), queries per wave, workgroups per cloud}; all 0 for an empty call (B == 0 or m == 0), which launches nothing.
 * B < 0, n <= 0 or m < 0: PDR_EINVAL, as the call. */
int pdr_ball_query_plan(int B, int n, int m, int out[4]);

/* ---- grouping ---------------------------------------------------------------
 * group_points(points (B,C,N), idx (B,np,ns)) -> out (B,C,np,ns)
 *                                                 group_points.cpp:12-36
 * group_points_grad(grad_out (B,C,np,ns), idx, n) -> (B,C,N)   :38-64 */
int pdr_group_points(const float *points, const int *idx, int B, int C, int N,
                     int np, int ns, float *out, pdr_stream_t stream);
int pdr_group_points_grad(const float *grad_out, const int *idx, int B, int C,
                          int N, int np, int ns, float *grad_points,
                          pdr_stream_t stream);

/* ---- 3-NN interpolation -----------------------------------------------------
 * three_nn(unknown (B,n,3), known (B,m,3)) -> dist2 (B,n,3) f32 SQUARED,
 *                                             idx (B,n,3) i32  interpolate.cpp:14-40
 * three_interpolate(points (B,C,m), idx (B,n,3), weight (B,n,3)) -> (B,C,n)  :42-70
 * three_interpolate_grad(grad_out (B,C,n), idx, weight, m) -> (B,C,m)        :72-100 */
int pdr_three_nn(const float *unknown, const float *known, int B, int n, int m,
                 float *dist2, int *idx, pdr_stream_t stream);
int pdr_three_interpolate(const float *points, const int *idx,
                          const float *weight, int B, int C, int m, int n,
                          float *out, pdr_stream_t stream);
int pdr_three_interpolate_grad(const float *grad_out, const int *idx,
                               const float *weight, int B, int C, int n, int m,
                               float *grad_points, pdr_stream_t stream);

/* ---- K nearest neighbours (pytorch3d.ops.knn_points contract) ---------------
 *   x (B,n1,3), y (B,n2,3), 1 <= K <= 32
 *   -> dists (B,n1,K) f32 squared, ascending; idx (B,n1,K) i64;
 *      nn (B,n1,K,3) f32 = y[idx]  (may be NULL: return_nn=False)
 * equal distances: lower index first.  K > n2: trailing slots dist 0, idx -1,
 * nn 0 (pytorch3d pads the same way).
 * (pytorch3d is not vendored by the reference: this order is the builder's contract, not a pin.  Against a
 * restatement of pytorch3d's published MinK -- replace the current maximum on a strictly smaller key, stable bubble
 * sort; oracle/pdr_oracle.c pdr_oracle_knn_mink, tests/test_oracle.py -- distances are always identical and indices
 * are identical on tie-free input and for K = 1; among EXACTLY equal distances MinK returns slot order (replacement
 * history) instead of index order and may keep another of several points tied at the K-th distance.) */
int pdr_knn_points(const float *x, const float *y, int B, int n1, int n2, int K,
                   float *dists, int64_t *idx, float *nn, pdr_stream_t stream);
/* pdr_knn_points with pytorch3d's per-cloud lengths: cloud b searches y[b, :lengths2[b]] for the queries
 * x[b, :lengths1[b]]; n1 / n2 stay the padded sizes (row strides).  lengths1 / lengths2 are int64 arrays of B entries
 * in DEVICE memory, read by the kernels only and clamped there to [0, n1] / [0, n2]: the host never reads them, so the
 * call neither synchronises nor allocates and is capturable like the dense one (a replayed graph follows the lengths
 * then in memory).  NULL = every cloud is full.  Rows at or beyond a cloud's length are never candidates, whatever
 * they hold.  Every slot k >= lengths2[b] of a valid query and every slot of a padded query (p >= lengths1[b]) gets
 * dist 0, idx -1, nn 0 -- the dense rule for K > n2.  Distance arithmetic, scan order, the tie rule, validation,
 * return codes and the kernel choice (a function of n2 and K) are those of pdr_knn_points; with NULL or full lengths
 * the output is bit-identical to it. */
int pdr_knn_points_ragged(const float *x, const float *y, const int64_t *lengths1, const int64_t *lengths2,
                          int B, int n1, int n2, int K, float *dists, int64_t *idx, float *nn, pdr_stream_t stream);

/* Both nearest-neighbour searches of one Chamfer evaluation (chamfer_loss_new.py:149-150: knn_points(x, y, K=1)
 * and knn_points(y, x, K=1)) in ONE launch: dist_xy / idx_xy (B,n1) = squared distance and index of the nearest
 * y point of every x point, dist_yx / idx_yx (B,n2) the reverse; first minimum wins (in-tree cross-check
 * chamfer3D.cu:26-129).  Bit-identical to two pdr_knn_points(K = 1) calls. */
int pdr_chamfer_nn(const float *x, const float *y, int B, int n1, int n2, float *dist_xy,
                   int64_t *idx_xy, float *dist_yx, int64_t *idx_yx, pdr_stream_t stream);
/* pdr_chamfer_nn with per-cloud lengths (same rules as pdr_knn_points_ragged: device int64, clamped on the device,
 * NULL = full), still ONE launch for both directions: lengths1 bounds x as queries of dist_xy and as candidates of
 * dist_yx, lengths2 bounds y the other way round.  Padded queries, and valid queries whose opposite cloud is empty,
 * get dist 0 and idx 0 (NOT -1: chamfer_distance gathers normals with these indices and masks the padded entries).
 * With NULL or full lengths bit-identical to pdr_chamfer_nn. */
int pdr_chamfer_nn_ragged(const float *x, const float *y, const int64_t *lengths1, const int64_t *lengths2,
                          int B, int n1, int n2, float *dist_xy, int64_t *idx_xy, float *dist_yx, int64_t *idx_yx,
                          pdr_stream_t stream);
/* All-pairs Chamfer distance between two SETS of clouds (the Chamfer half of _pairwise_EMD_CD_,
 * pointnet2/models/pvd/metrics/evaluation_metrics.py:45-78, which expands one cloud R times, calls chamfer_distance and
 * reduces 2 (n + m) distances per pair with torch launches):  x (S,n,3), y (R,m,3)  ->  cd (S,R) f32, fully written,
 *     cd[s,r] = (1/n_s) sum_i min_j |x_s,i - y_r,j|^2  +  (1/m_r) sum_j min_i |x_s,i - y_r,j|^2
 * = calc_cd's cd_t = the reference's dl.mean(1) + dr.mean(1), one float per pair; nothing per point is stored and no
 * index is recovered.  ONE launch (a workgroup per pair), no workspace, no atomics, no allocation, no synchronisation:
 * capturable like every call here.
 *   - lengths_x / lengths_y follow the rules of pdr_knn_points_ragged: int64 arrays of S / R entries in DEVICE memory,
 *     read by the kernel only and clamped there to [0, n] / [0, m]; NULL = every cloud is full; n / m stay the row
 *     strides.  Rows at or beyond a cloud's length are never queries and never candidates, whatever they hold (NaN
 *     included).  A pair with an empty side gets cd = 0 (what calc_cd gives).  A pair's value depends on its two
 *     clouds' valid rows only: with NULL or full lengths the result is bit-identical to the call without lengths, and a
 *     ragged pair gets the bits of the dense call on the two slices.
 *   - the distance is the knn expression (fma(dz, dz, fma(dy, dy, dx * dx)) on the differences, never the expanded
 *     |x|^2 + |y|^2 - 2 x.y): every per-point minimum has the bits pdr_chamfer_nn returns for that pair.
 *   - the sums are deterministic: their order is fixed by the code (per thread in ascending query order, then a fixed
 *     tree), so the same input gives the same bits run after run.  The longest chain of dependent fp32 roundings is
 *     ceil(max(n, m) / 256) + 10 -- 74 for n, m <= 16384 --, and every addend is non-negative: cd is within
 *     74 * 2^-24 relative of the exact sum of the fp32 minima.
 *   - symmetric != 0 is the self-matrix: it requires x == y, lengths_x == lengths_y, S == R and n == m (PDR_EINVAL
 *     otherwise, checked before anything else but the signs of the sizes).  Only the pairs s <= r are evaluated and
 *     their owner writes cd[s,r] and cd[r,s]: roughly half the work.  The matrix is bitwise symmetric, equal bit for
 *     bit to the plain call on (x, x) (whose two triangles add the same two sums in opposite order), and its diagonal
 *     is exactly 0 for non-empty clouds of finite points (a point's distance to itself is exactly 0 here).
 *   - validation: a negative size: PDR_EINVAL; S == 0 or R == 0: PDR_OK, nothing done, no pointer looked at;
 *     n <= 0 or m <= 0 with S, R > 0: PDR_EINVAL (as pdr_chamfer_nn); NULL x / y / cd: PDR_EINVAL; more than 2^30
 *     pairs: PDR_EUNSUPPORTED.  cd and the clouds are indexed in size_t. */
int pdr_chamfer_pairwise(const float *x, const float *y, const int64_t *lengths_x, const int64_t *lengths_y,
                         int S, int R, int n, int m, int symmetric, float *cd, pdr_stream_t stream);
/* The Chamfer distance as a TRAINING LOSS (calc_cd(X, refined_X)[loss_idx].mean().backward(), pointnet2/train.py:518):
 * x (B,n1,3), y (B,n2,3)  ->  sums (B,4) f32, fully written,
 *     sums[b] = { sum_i d_xy[i], sum_j d_yx[j], sum_i sqrt(d_xy[i]), sum_j sqrt(d_yx[j]) },  d_xy[i] = min_j |x_i - y_j|^2
 * over the valid points of each cloud (d_yx the reverse): everything cd_t and cd_p are made of; the divisions by the
 * lengths, the / 2, weights and the batch reduction are the caller's, on (B,4).  idx_xy (B,n1) / idx_yx (B,n2) int32
 * receive the index where each minimum is attained -- what pdr_chamfer_loss_grad needs; both may be NULL for a
 * loss-only call (exactly one NULL: PDR_EINVAL).  TWO launches on `stream` (the search with per-workgroup partial sums
 * into the workspace, then a finishing launch), no atomics, no allocation, no synchronisation: capturable.
 *   - minima and indices are those of pdr_chamfer_nn / pdr_chamfer_nn_ragged, bit for bit: the knn expression
 *     fma(dz, dz, fma(dy, dy, dx * dx)) on the differences, strict <, first minimum wins.  A padded query and a query
 *     whose opposite cloud is empty get index -1 (and add nothing).
 *   - lengths1 / lengths2 follow pdr_knn_points_ragged: int64 arrays of B entries in DEVICE memory, read by the kernels
 *     only and clamped there to [0, n1] / [0, n2]; NULL = every cloud is full; n1 / n2 stay the row strides.  Rows at or
 *     beyond a length are never queries, never candidates and never read for their value (NaN included).  A pair with
 *     an empty side has all four sums +0.0f.
 *   - the sums are deterministic (no floating-point atomics): the order is fixed by the code and is a function of the
 *     two lengths only -- per thread in ascending query order, a fixed tree per 1024-query block, then the blocks in
 *     ascending order.  A ragged pair gets the bits of the dense call on the two slices; NULL or full lengths give the
 *     bits of the call without lengths; asking for the indices changes no bit of sums.  The longest chain of dependent
 *     fp32 roundings is 12 + ceil(max(n1, n2) / 1024) -- 28 for n <= 16384 -- and every addend is non-negative:
 *     sums[0:2] is within 28 * 2^-24 relative of the exact sum of the fp32 minima, sums[2:4] (one more rounding per
 *     addend, the sqrt) within 30 * 2^-24 of the exact sum of their square roots.
 *   - workspace: pdr_chamfer_loss_workspace_bytes(B, n1, n2) bytes of device memory, 4-byte aligned; positive for
 *     supported positive sizes, non-decreasing in each argument, 0 for B <= 0 and for sizes the call refuses.  Its
 *     contents are private and undefined afterwards; two calls in flight at once need a workspace each.
 *   - validation, decided on the host before any launch, in this order: a negative size: PDR_EINVAL; B == 0: PDR_OK,
 *     nothing launched, no pointer looked at; n1 <= 0 or n2 <= 0: PDR_EINVAL; sizes the kernels do not index --
 *     B > 65535, max(n1, n2) > 2^24 or B max(n1, n2) >= 2^31 --: PDR_EUNSUPPORTED; NULL x / y / sums, exactly one NULL
 *     index array, a NULL workspace or one that is not 4-byte aligned: PDR_EINVAL. */
size_t pdr_chamfer_loss_workspace_bytes(int B, int n1, int n2);
int pdr_chamfer_loss(const float *x, const float *y, const int64_t *lengths1, const int64_t *lengths2,
                     int B, int n1, int n2, float *sums, int *idx_xy, int *idx_yx, void *workspace,
                     pdr_stream_t stream);
/* Backward of pdr_chamfer_loss w.r.t. both clouds.  grad_sums (B,4) f32 = (g0, g1, g2, g3) = d(loss)/d(sums[b]); idx_xy /
 * idx_yx are the arrays the forward wrote; grad_x (B,n1,3) and grad_y (B,n2,3) are fully written.  The coefficient on
 * a squared distance is
 *     w_xy[i] = g0 + (g2 == 0 ? 0 : g2 * 0.5 / sqrt(d_xy[i])),     w_yx[j] = g1 + (g3 == 0 ? 0 : g3 * 0.5 / sqrt(d_yx[j]))
 * with d recomputed from x, y and the saved index by the knn expression (the bits the forward saw; no distance tensor
 * is saved), and
 *     grad_x[b,i] = fl(2 w_xy[i]) (x_i - y_idx_xy[i])  -  sum over j with idx_yx[j] == i, j ascending, of
 *                   fl(2 w_yx[j]) (y_j - x_i)
 * grad_y being the mirror image.  Every product is rounded before its add (no fused multiply-add); an element starts
 * from its query term (+0.0f when that index is -1) and the scattered terms are added after it in ascending source
 * order, so the same input gives the same bits.  ONE launch, no workspace, no atomics of any kind, no allocation, no
 * synchronisation: capturable.  Each output element is written exactly once.
 *   - zero coefficient: when g2 (g3) is exactly 0 the sqrt term is not evaluated; a cd_t-only loss never sees 0 * inf.
 *   - zero distance: when d == 0 the sqrt term contributes exactly 0.  A subgradient choice -- the direction x - y is 0
 *     there -- that DEPARTS from the torch composition sqrt(d).backward(), which gives inf * 0 = NaN for a coincident
 *     pair; mirrored condition clouds and x == y make coincident pairs real.
 *   - padded rows of either cloud and all rows of a pair with an empty side get +0.0f; a padded source is never added.
 *     An index outside [0, n) of the opposite cloud is skipped and reaches no memory.
 *   - how: an inverse scan.  One thread owns a destination point, the opposite direction's index array streams through
 *     LDS and the thread compares every entry with its own index: n1 n2 integer compares per cloud and direction.
 *   - validation: the forward's size checks and codes, then a NULL x / y / idx_xy / idx_yx / grad_sums / grad_x /
 *     grad_y: PDR_EINVAL. */
int pdr_chamfer_loss_grad(const float *x, const float *y, const int64_t *lengths1, const int64_t *lengths2,
                          const int *idx_xy, const int *idx_yx, const float *grad_sums, int B, int n1, int n2,
                          float *grad_x, float *grad_y, pdr_stream_t stream);
/* The pooling tail of AttentionModule.forward (pointnet2_ops/attention.py:71-77) for the TRAINABLE path, channel-first
 * and differentiable (pdr_attention_pool below is the channel-last, forward-only form of the fused sampler):
 *     scores, values (B,C,N,K) f32, dense, K innermost (what weight_conv / feat_out_conv write);
 *     counts (B,N) int32, shared by the C channels of a cloud, NULL = 'all'   ->   out (B,C,N) f32.
 * For row (b,c,n) let c_n = min(max(counts[b,n], 1), K) -- the reference's clamp(min=1); a count above K masks nothing.
 * Slot k < c_n carries s_k, slot k >= c_n carries exactly -1e9f (as the reference and pdr_attention_pool);
 * w = softmax over the K slots and out = sum_k w_k v_k.  ONE launch, no workspace, no atomics of any kind, no
 * allocation, no synchronisation: capturable.  Every output element is written exactly once; the same input gives the
 * same bits.
 *   - operation chain, one fp32 rounding per step (no fused multiply-add but the one written):
 *         t_k = k < c_n ? s_k : -1e9f,   a_k = fl(t_k * fl(log2 e)),   m = max_k a_k (exact),
 *         e_k = v_exp_f32(fl(a_k - m)),  l = sum_k e_k,  acc = sum_k fma(v_k, e_k, acc),  out = fl(acc / l).
 *     The sums run in ascending k from +0.0f in the scalar family; in the vector family per lane (4 consecutive slots,
 *     ascending) and then as a butterfly over the row's lanes (lane distance 1, 2, 4, 8).  The two families agree up to
 *     that order.
 *   - the score held by a masked slot is NOT inspected.  A deliberate departure from the torch composition, for a
 *     non-finite masked score only: there scores * mask gives inf * 0 = NaN.  Masked slots of `values` ARE multiplied
 *     by their weight (0 unless the valid scores are near -1e9), as in the reference: a non-finite masked value gives NaN.
 *   - two kernel families, chosen on the host and reported by pdr_attention_pool_cf_plan.  Vector: K % 4 == 0 and every
 *     non-NULL pointer of the call 16-byte aligned; a row belongs to L = ceil_pow2(K / 4) adjacent lanes, one float4
 *     each (a wave's load covers 64 / L consecutive rows), max / sum / dot folded across them with DPP; 256 / L rows per
 *     workgroup, the grid covers all rows.  Scalar: any other 1 <= K <= 64, or a misaligned pointer (a contiguous view
 *     with a storage offset); a thread per row, scalar loads.
 *   - validation, decided on the host before any launch, in this order: a negative size or K <= 0: PDR_EINVAL;
 *     B C N == 0: PDR_OK, nothing launched, no pointer looked at; K > 64 or B C N K >= 2^31: PDR_EUNSUPPORTED; a NULL
 *     scores / values / out: PDR_EINVAL.  Elements are indexed in size_t. */
int pdr_attention_pool_cf(const float *scores, const float *values, const int *counts,
                          int B, int C, int N, int K, float *out, pdr_stream_t stream);
/* Backward of pdr_attention_pool_cf w.r.t. scores and values.  grad_out (B,C,N); grad_scores / grad_values (B,C,N,K),
 * fully written; either may be NULL (autograd's needs_input_grad), both NULL: PDR_EINVAL.  The kernel recomputes m, l,
 * e_k and out from scores / values by the forward's operation chain (the forward's bits; no weight tensor and no `out`
 * is saved or passed), then, every product rounded before it is used,
 *     rl = fl(1 / l),   w_k = fl(e_k * rl),
 *     grad_values[k] = fl(g * w_k)
 *     grad_scores[k] = k < c_n ? fl(fl(g * w_k) * fl(v_k - out)) : +0.0f
 * ONE launch, no workspace, no atomics of any kind, no allocation, no synchronisation: capturable.  Every output
 * element is written exactly once; the same input gives the same bits, and asking for one gradient only changes no bit
 * of it.  Kernel families and alignment rule as the forward (all of scores, values, counts, grad_out and the non-NULL
 * gradients).  Validation: the forward's size checks and codes in the same order, then a NULL scores / values /
 * grad_out, or both gradients NULL: PDR_EINVAL. */
int pdr_attention_pool_cf_grad(const float *scores, const float *values, const int *counts,
                               const float *grad_out, int B, int C, int N, int K,
                               float *grad_scores, float *grad_values, pdr_stream_t stream);
/* Which kernel the two calls above run for K slots per row.  Host only (no HIP call, no device pointer); the launches
 * read the same decision.  aligned16 != 0: every non-NULL pointer of the call is 16-byte aligned.
 * out = {family (0 scalar, 1 vector), lanes per row L, rows per workgroup (256 / L), rows per lane group per grid pass
 * -- 0: the grid covers all rows, which it always does}.  K <= 0 or a NULL out: PDR_EINVAL; K > 64: PDR_EUNSUPPORTED. */
int pdr_attention_pool_cf_plan(int K, int aligned16, int out[4]);
/* MyGroupNorm followed by an activation (pointnet2_ops/attention.py:18-32, pointnet2_modules.py:37-53) for the TRAINABLE
 * path, as one differentiable op (the inference path folds GroupNorm into its consumer kernels: pdr_gn_fold):
 *     x (B,C,S) f32, dense, S = the product of all trailing dimensions;  gamma, beta (Cn) f32, both NULL = 1 and 0
 *     ->  y (B,C,S) f32,  mean, rstd (B,G) f32 (either may be NULL: a caller that needs no gradient).
 * Cn = C - C % G, Cg = Cn / G.  Group g of cloud b is the contiguous slab of m = Cg S floats at (b C + g Cg) S:
 *     mean, biased variance, rstd = 1 / sqrt(var + eps);  c < Cn: z = (x - mean) rstd gamma[c] + beta[c];
 *     c >= Cn (the appended xyz channels): z = x;   y = act(z) on every channel,
 *     act 0: none, 1: ReLU (z > 0 ? z : +0), 2: Swish (z sigmoid(z)).
 * TWO launches (statistics partials, then apply), no atomics of any kind, no allocation, no synchronisation:
 * capturable.  Every output element is written exactly once; the same input gives the same bits, and cloud b of a
 * batched call has the bits of the B = 1 call on that cloud.
 *   - operation chain (csrc/group_norm_act.hip states it in full): the moments s1 = sum x, s2 = sum x^2 accumulate in
 *     double; mean_d = s1 / m, var_d = max(s2 / m - mean_d^2, 0); mean = float(mean_d), rstd = float(1 / sqrt(var_d +
 *     eps)) are the values written AND applied; then, one fp32 rounding each, d = x - mean, xh = d rstd,
 *     z = fma(xh, gamma, beta); Swish: t = z fl(-log2 e), e = v_exp_f32(t), s = 1 / (1 + e), y = z s.
 *   - summation order: a function of (Cg, S) and the kernel family only.  A slab is cut into P <= 32 partitions of E
 *     elements (E a multiple of 1024, at least 8192, from m alone; pdr_group_norm_act_plan reports both); inside a
 *     partition thread t of 256 takes elements (256 i + t) V .. + V - 1, i ascending, then a lane butterfly, the four
 *     waves ascending, the P partials ascending.
 *   - two kernel families: vector (V = 4: S % 4 == 0 and x, y 16-byte aligned) and scalar (V = 1: anything else, such
 *     as a contiguous view with a storage offset).  They agree up to the summation order.
 *   - workspace: pdr_group_norm_act_workspace_bytes(B, C, S, G) bytes, 8-byte aligned, the caller's; it serves either
 *     call (forward: B G P pairs of doubles; backward: B C pairs).  Not read after the call returns its last kernel.
 *   - validation, decided on the host before any launch, in this order: B, C or S negative, G <= 0, act outside 0..2,
 *     eps negative or NaN: PDR_EINVAL; 0 < C < G (Cn == 0): PDR_EINVAL; B C S == 0: PDR_OK, nothing launched, no
 *     pointer looked at; B C S >= 2^31: PDR_EUNSUPPORTED; a NULL x / y / workspace, or exactly one of gamma / beta
 *     NULL: PDR_EINVAL. */
int pdr_group_norm_act(const float *x, const float *gamma, const float *beta, int B, int C, long S, int G,
                       float eps, int act, float *y, float *mean, float *rstd, void *workspace, pdr_stream_t stream);
/* Backward of pdr_group_norm_act.  mean, rstd: what the forward wrote; grad_y (B,C,S); grad_x (B,C,S), grad_gamma,
 * grad_beta (Cn), each fully written, each may be NULL (autograd's needs_input_grad), all three NULL: PDR_EINVAL;
 * gamma NULL with a non-NULL grad_gamma / grad_beta: PDR_EINVAL.  Nothing but x and the (B,G) statistics is saved: the
 * kernels recompute d, xh, z (and the sigmoid) from x, mean, rstd, gamma, beta by the forward's operation sequence --
 * the forward's bits, so the ReLU mask is the forward's -- then
 *     dz = dy act'(z)      (ReLU: z > 0 ? dy : +0;  Swish: dy (s (1 + z (1 - s))), every product rounded)
 *     r1[b,c] = sum_s dz xh,  r2[b,c] = sum_s dz            in double, to the workspace, order as a partition's
 *     c1 = sum_c gamma r1,  c2 = sum_c gamma r2             over the slab's Cg rows, ascending, in double
 *     dx = rstd (gamma dz - fma(xh, float(c1 / m), float(c2 / m)));   pass-through channel: dx = dz
 *     dgamma[c] = sum_b r1[b,c],  dbeta[c] = sum_b r2[b,c]  ascending b, in double, rounded once
 * THREE launches (row sums, dx, parameter sums; dx or the parameter sums are skipped when not asked for), no atomics,
 * no allocation, no synchronisation: capturable; the same input gives the same bits.  Kernel families as the forward
 * (x, grad_y and grad_x aligned).  Validation: the forward's size checks in the same order, then the pointers. */
int pdr_group_norm_act_grad(const float *x, const float *gamma, const float *beta, const float *mean,
                            const float *rstd, const float *grad_y, int B, int C, long S, int G, int act,
                            float *grad_x, float *grad_gamma, float *grad_beta, void *workspace, pdr_stream_t stream);
/* Bytes of workspace either call above needs; 0 for an empty or invalid problem.  Host only. */
size_t pdr_group_norm_act_workspace_bytes(int B, int C, long S, int G);
/* The decision the two calls above read.  Host only.  aligned16 != 0: the tensor pointers of the call are 16-byte
 * aligned.  out = {family (0 scalar, 1 vector), partitions per slab P, elements per partition E, Cg}.
 * C, S or G <= 0, C < G or a NULL out: PDR_EINVAL; C S >= 2^31: PDR_EUNSUPPORTED. */
int pdr_group_norm_act_plan(int C, long S, int G, int aligned16, long out[4]);
/* pdr_group_norm_act with what Mlp_plus_t_emb adds behind a [conv, MyGroupNorm, act] stack folded into the apply
 * kernel: an embedding add (B,C) f32 broadcast over S and a residual (B,C,S) f32 dense, each may be NULL,
 *     y = fl(fl(act(z) + add[b,c]) + residual[b,c,s])     the composition's order; a NULL term is skipped.
 * Everything else is pdr_group_norm_act's: the same two launches, statistics, operation chain, summation order,
 * workspace, properties and validation (the sizes first, in the same order, then the pointers; add and residual are
 * optional, so they add no failure).  mean and rstd have pdr_group_norm_act's bits, y has the bits of its y followed
 * by the two fp32 additions, and with add == residual == NULL the call launches that entry's kernels.  A NaN or an
 * infinity in add / residual propagates as an fp32 addition propagates it.  The vector family also needs residual
 * 16-byte aligned. */
int pdr_group_norm_act_add(const float *x, const float *gamma, const float *beta, const float *add,
                           const float *residual, int B, int C, long S, int G, float eps, int act, float *y,
                           float *mean, float *rstd, void *workspace, pdr_stream_t stream);
/* Backward of pdr_group_norm_act_add.  It reads neither add nor residual: d y / d act(z) = 1, so grad_x, grad_gamma and
 * grad_beta are pdr_group_norm_act_grad's on the same grad_y, bit for bit; the residual's gradient is grad_y itself
 * (no kernel; the caller returns it); and
 *     grad_add[b,c] = float(sum_s double(grad_y[b,c,s]))   (B,C) f32, the RAW grad_y, pass-through rows included,
 * summed in double in the row order (thread t of 256 takes elements (256 i + t) V .. + V - 1, i ascending, then the
 * lane butterfly, the four waves ascending), rounded once and written by the row kernel: the same THREE launches and
 * the same workspace as pdr_group_norm_act_grad.  Each of the four gradients may be NULL; all four NULL: PDR_EINVAL.
 * No atomics, no allocation, no synchronisation: capturable; the same input gives the same bits, and cloud b of a
 * batched call has the bits of the B = 1 call on that cloud (grad_gamma / grad_beta sum over b). */
int pdr_group_norm_act_add_grad(const float *x, const float *gamma, const float *beta, const float *mean,
                                const float *rstd, const float *grad_y, int B, int C, long S, int G, int act,
                                float *grad_x, float *grad_gamma, float *grad_beta, float *grad_add, void *workspace,
                                pdr_stream_t stream);
/* The front of AttentionModule's score head on the TRAINABLE path (pointnet2_ops/attention.py: expand, cat, then
 * weight_conv's ReLU and MyGroupNorm -- activation FIRST, then norm) as one differentiable op over a tensor that is
 * never built:
 *     k (B,C2,N,K) f32 dense, C2 >= 1;  q (B,C1,N) f32 dense, or NULL with C1 = 0;  gamma, beta (Cn) f32, both NULL = 1, 0
 *     ->  y (B,C,N,K) f32 contiguous, C = C1 + C2;  mean, rstd (B,G) f32 (either may be NULL).
 * The virtual input is x = cat([q[..., None] repeated K times, k], dim 1), S = N K.  u = relu(x) on ALL channels
 * (x > 0 ? x : +0; a NaN stays a NaN, as torch.relu leaves it); Cn = C - C % G, Cg = Cn / G; group g of cloud b is the
 * virtual channels [g Cg, (g + 1) Cg) -- inside q, inside k, or across the boundary --, m = Cg S values:
 *     mean, biased variance, rstd = 1 / sqrt(var + eps);  c < Cn: y = (u - mean) rstd gamma[c] + beta[c];  c >= Cn: y = u.
 * TWO launches (statistics partials, then apply), no atomics, no allocation, no synchronisation: capturable.  Every
 * output element is written exactly once; the same input gives the same bits, and cloud b of a batched call has the
 * bits of the B = 1 call on that cloud.
 *   - operation chain (csrc/relu_group_norm.hip states it in full): moments in double; a q value is read once and the
 *     double sums over the slab's q values are multiplied by double(K) (one rounding each); mean_d = S1 / m,
 *     var_d = max(S2 / m - mean_d^2, 0); mean = float(mean_d), rstd = float(1 / sqrt(var_d + eps)) are the values
 *     written AND applied; then, one fp32 rounding each, d = u - mean, xh = d rstd, y = fma(xh, gamma, beta).
 *   - summation order: a function of (C1, Cg, N, K) and the kernel family only.  The k values of a slab are cut into
 *     P <= 32 partitions of E elements (E a multiple of 1024, at least 8192, from m = Cg S alone;
 *     pdr_relu_group_norm_cf_plan reports both), the slab's q values are one more partition (V = 1); inside a partition
 *     thread t of 256 takes elements (256 i + t) V .. + V - 1, i ascending, then a lane butterfly, the four waves
 *     ascending; the q term first, then the P partials ascending.
 *   - two kernel families: vector (V = 4: K % 4 == 0 and k, y 16-byte aligned) and scalar (V = 1: anything else).
 *   - workspace: pdr_relu_group_norm_cf_workspace_bytes(B, C1, C2, N, K, G) bytes, 8-byte aligned, the caller's; it
 *     serves either call (forward: B G (P + 1) pairs of doubles; backward: B C pairs).
 *   - validation, on the host before any launch, in this order: B, C1, N or K negative, C2 < 1, G < 1, eps negative or
 *     NaN: PDR_EINVAL; C1 + C2 < G: PDR_EINVAL; B N K == 0: PDR_OK, nothing launched, no pointer looked at;
 *     B C N K >= 2^31 or B C >= 2^24 (a grid's x dimension; every y dimension is at most 65535 by construction):
 *     PDR_EUNSUPPORTED; a NULL k / y / workspace, C1 > 0 with a NULL q, or exactly one of gamma / beta NULL: PDR_EINVAL. */
int pdr_relu_group_norm_cf(const float *q, const float *k, const float *gamma, const float *beta, int B, int C1,
                           int C2, int N, int K, int G, float eps, float *y, float *mean, float *rstd,
                           void *workspace, pdr_stream_t stream);
/* Backward of pdr_relu_group_norm_cf.  mean, rstd: what the forward wrote; grad_y (B,C,N,K); grad_q (B,C1,N), grad_k
 * (B,C2,N,K), grad_gamma, grad_beta (Cn), each fully written, each may be NULL (not wanted); all four NULL, gamma NULL
 * with a non-NULL grad_gamma / grad_beta, or grad_q with C1 == 0: PDR_EINVAL.  The kernels recompute u, d, xh from q, k
 * and the saved statistics by the forward's sequence (the forward's bits), then
 *     r1[b,c] = sum_s grad_y xh,  r2[b,c] = sum_s grad_y       in double, to the workspace, order as a partition's
 *     c1 = sum_c gamma r1,  c2 = sum_c gamma r2                over the slab's Cg rows, ascending, in double
 *     du = rstd (gamma grad_y - fma(xh, float(c1 / m), float(c2 / m)));   pass-through channel: du = grad_y
 *     dx = x > 0 ? du : +0   (the mask is on the raw input);   grad_k = dx on the k channels
 *     grad_q[b,c,n] = x > 0 ? float(sum_j double(du[b,c,n,j])) : +0    a double sum over j = 0 .. K - 1, ascending from
 *                     +0, rounded once; the q part of dx is never stored
 *     dgamma[c] = sum_b r1[b,c],  dbeta[c] = sum_b r2[b,c]     ascending b, in double, rounded once
 * Up to FOUR launches (row sums, grad_k, grad_q, parameter sums; those not asked for are skipped), no atomics, no
 * allocation, no synchronisation: capturable; the same input gives the same bits.  Kernel families as the forward (k,
 * grad_y and grad_k aligned).  Validation: the forward's size checks in the same order, then the pointers. */
int pdr_relu_group_norm_cf_grad(const float *q, const float *k, const float *gamma, const float *beta,
                                const float *mean, const float *rstd, const float *grad_y, int B, int C1, int C2, int N,
                                int K, int G, float *grad_q, float *grad_k, float *grad_gamma, float *grad_beta,
                                void *workspace, pdr_stream_t stream);
/* Bytes of workspace either call above needs; 0 for an empty, invalid or unsupported problem.  Host only. */
size_t pdr_relu_group_norm_cf_workspace_bytes(int B, int C1, int C2, int N, int K, int G);
/* The decision the two calls above read.  Host only.  aligned16 != 0: the tensor pointers of the call are 16-byte
 * aligned.  out = {family (0 scalar, 1 vector), k partitions per slab P, elements per partition E, Cg}.
 * C1 < 0, C2, N, K or G < 1, C1 + C2 < G or a NULL out: PDR_EINVAL; C N K >= 2^31 or C >= 2^24: PDR_EUNSUPPORTED. */
int pdr_relu_group_norm_cf_plan(int C1, int C2, int N, int K, int G, int aligned16, long out[4]);
/* A whole link of AttentionModule's score head on the TRAINABLE path ([ReLU, MyGroupNorm, Conv2d 1x1] over the virtual
 * cat of pdr_relu_group_norm_cf) as one differentiable op whose fp32 MFMA GEMM normalises its operand as it loads it:
 * the normalised tensor (B,C,N,K) is never written, read back or saved.  q, k, gamma, beta, mean, rstd and every size
 * as pdr_relu_group_norm_cf; W (Cout,C) row-major f32 (the Conv2d weight viewed 2-D), bias (Cout) f32 or NULL
 *     ->  out (B,Cout,N,K) f32 dense;  mean, rstd (B,G) f32 with the bits pdr_relu_group_norm_cf writes (both required).
 * With xn[b,c,n,j] exactly the value pdr_relu_group_norm_cf writes to y (same statistics kernel, same element chain:
 * csrc/relu_group_norm.h), the GEMM is defined bit for bit:
 *     acc = +0;  for c = 0 .. C-1 ascending: acc = fma(W[o,c], xn[b,c,n,j], acc);  out = bias ? fl(acc + bias[o]) : acc
 * (v_mfma_f32_32x32x2_f32 with its k index walking c in order; the LDS chunks of 16 channels continue the chain).
 * THREE launches (statistics partials, mean / rstd, GEMM), no atomics, no allocation, no synchronisation: capturable;
 * the same input gives the same bits, and cloud b of a batched call has the bits of the B = 1 call on that cloud.
 *   - families: vector (K % 4 == 0 and k 16-byte aligned: 16-byte loads) and scalar; out is stored dword by dword.
 *   - workspace: pdr_relu_group_norm_conv_cf_workspace_bytes bytes, 8-byte aligned, the caller's; it serves the forward
 *     and pdr_relu_group_norm_conv_cf_grad_weight.
 *   - validation, on the host before any launch, in this order: B, C1, N or K negative, C2 < 1, G < 1, Cout < 1, eps
 *     negative or NaN: PDR_EINVAL; C1 + C2 < G: PDR_EINVAL; B N K == 0: PDR_OK, nothing launched, no pointer looked at;
 *     B C N K >= 2^31, B Cout N K >= 2^31, B C >= 2^24, C > 1024, Cout > 1024 or B > 4095: PDR_EUNSUPPORTED; a NULL
 *     k / W / out / mean / rstd / workspace, C1 > 0 with a NULL q, or exactly one of gamma / beta NULL: PDR_EINVAL. */
int pdr_relu_group_norm_conv_cf(const float *q, const float *k, const float *gamma, const float *beta, const float *W,
                                const float *bias, int B, int C1, int C2, int N, int K, int G, int Cout, float eps,
                                float *out, float *mean, float *rstd, void *workspace, pdr_stream_t stream);
/* Input gradient of the GEMM above, bit-defined the same way over the other index:
 *     acc = +0;  for o = 0 .. Cout-1 ascending: acc = fma(W[o,c], grad_out[b,o,n,j], acc);  grad_xn[b,c,n,j] = acc
 * grad_out (B,Cout,N,K) -> grad_xn (B,C,N,K), fully written: what pdr_relu_group_norm_cf_grad takes as grad_y.  ONE
 * launch, no prologue, no workspace.  Vector family: K % 4 == 0 and grad_out 16-byte aligned.  B, N or K negative, C
 * or Cout < 1: PDR_EINVAL; B N K == 0: PDR_OK; the limits above: PDR_EUNSUPPORTED; a NULL pointer: PDR_EINVAL. */
int pdr_relu_group_norm_conv_cf_grad_input(const float *W, const float *grad_out, int B, int C, int N, int K, int Cout,
                                           float *grad_xn, pdr_stream_t stream);
/* Weight and bias gradients: grad_W[o,c] = sum_{b,n,j} grad_out[b,o,n,j] xn[b,c,n,j] with xn recomputed from q, k and
 * the SAVED mean / rstd (the forward's bits), grad_bias[o] = sum grad_out.  Either may be NULL (not wanted); both NULL:
 * PDR_EINVAL.  Order-fixed, no atomics: the N K positions of a cloud are cut into R ranges of L positions (the plan
 * reports both; from N K alone); a workgroup accumulates one (cloud, range) of a tile of grad_W in one fp32 MFMA chain
 * from +0 and writes the partial to the workspace; the B R partials of an element are added in DOUBLE in ascending
 * (b, range) order and rounded once.  grad_bias: double sums of a (b, o, range) (thread t of 256 takes positions t,
 * t + 256, .., then the block sum of pdr_relu_group_norm_cf), then the same fold.  Up to FOUR launches; capturable.
 * Vector family: K % 4 == 0 and k, grad_out 16-byte aligned.  Validation as the forward (no eps), then the pointers. */
int pdr_relu_group_norm_conv_cf_grad_weight(const float *q, const float *k, const float *gamma, const float *beta,
                                            const float *mean, const float *rstd, const float *grad_out, int B, int C1,
                                            int C2, int N, int K, int G, int Cout, float *grad_W, float *grad_bias,
                                            void *workspace, pdr_stream_t stream);
/* Bytes of workspace the forward or the weight gradient needs (the larger: B G (P + 1) pairs of doubles; B R Cout C
 * floats + B R Cout doubles); 0 for an empty, invalid or unsupported problem.  Host only. */
size_t pdr_relu_group_norm_conv_cf_workspace_bytes(int B, int C1, int C2, int N, int K, int G, int Cout);
/* The decision the calls above read.  Host only.  out = {family (0 scalar, 1 vector), P, E, Cg (the statistics plan of
 * pdr_relu_group_norm_cf_plan), positions per workgroup of the GEMMs, positions per weight-gradient chain L, ranges
 * per cloud R, output rows per workgroup of the forward GEMM}.  Errors as pdr_relu_group_norm_cf_plan, and Cout < 1:
 * PDR_EINVAL; the forward's limits (with B = 1): PDR_EUNSUPPORTED. */
int pdr_relu_group_norm_conv_cf_plan(int C1, int C2, int N, int K, int G, int Cout, int aligned16, long out[8]);
/* Neighbourhood grouping of the TRAINABLE path: what QueryAndGroup.forward (pointnet2_ops/pointnet2_utils.py) does
 * after its neighbour search, channel-first, as one differentiable op (the inference path gathers channel-last in
 * pdr_group_build):
 *     xyz (B,n,3), new_xyz (B,m,3), features (B,C,n) or NULL, idx (B,m,K) int32, counts (B,m) int32 or NULL
 *     ->  out (B, Cu + 3E, m, K) f32, channels [features | relative | absolute | centre], Cu = C, or 0 when features
 *         is NULL (C is ignored then).
 * flags: bit 0 use_xyz (the relative channels xyz[idx] - new_xyz), bit 1 include_abs (xyz[idx]), bit 2 include_center
 * (new_xyz, repeated over K); bits 1 and 2 are ignored without bit 0, as in the module.  E = 0 .. 3 is the number of
 * coordinate triples the flags enable.  A non-NULL counts is the module's patch_empty: query q with counts[b,q] <= 0 is
 * PATCHED -- absolute = the centre, relative = centre - centre, features = +0.0f, and idx is not read for it.
 * ONE launch, no atomics, no allocation, no synchronisation: capturable.  Every output element is a bit-for-bit copy of
 * its source or, in the relative channels, the one rounded difference a - c (no fma).  The torch composition computes a
 * patched or passed value as 1 * a + 0 * c; this call SELECTS it: the two differ only for -0.0 and non-finite inputs.
 * An index outside [0, n) in a slot of an unpatched query is the caller's error, as for pdr_group_points.
 *   - two kernel families: vector (K % 4 == 0 and out 16-byte aligned: four k per thread, one 16-byte store per
 *     channel) and scalar (anything else); the same bits.  pdr_query_group_cf_plan reports the decision.
 *   - limits: n <= 16384, m K <= 2^22, B <= 65535, B m K < 2^31 (the inverse-index builder's, so that every forward
 *     has its backward) and B (Cu + 3E) m K < 2^31.
 *   - validation, decided on the host before any launch, in this order: B, m, K or C negative, n <= 0, flags outside
 *     0 .. 7, no channel at all (without use_xyz: Cu == 0): PDR_EINVAL; B, m or K zero: PDR_OK, nothing launched, no
 *     pointer looked at; the limits: PDR_EUNSUPPORTED; a NULL idx / out, or with use_xyz a NULL xyz / new_xyz:
 *     PDR_EINVAL. */
int pdr_query_group_cf(const float *xyz, const float *new_xyz, const float *features, const int *idx,
                       const int *counts, int B, int n, int m, int K, int C, int flags, float *out,
                       pdr_stream_t stream);
/* Backward of pdr_query_group_cf.  idx, counts, flags: the forward's; C: the feature channels of grad_out (0 when the
 * forward had no features); grad_out (B, C + 3E, m, K).  grad_features (B,C,n), grad_xyz (B,n,3), grad_new_xyz (B,m,3):
 * each fully written, each may be NULL (autograd's needs_input_grad; its launches are skipped), all three NULL:
 * PDR_EINVAL.  g_f, g_r, g_a, g_c are the slices of grad_out, a slice whose flag is off counts as +0; a slot p = (q, k)
 * is REAL when its query is not patched and 0 <= idx[b,p] < n (an index outside is skipped, as in the *_grad_det calls):
 *     a[d,p]               = fl(g_r[d,p] + g_a[d,p])     the absolute coordinate's gradient: xyz[idx]'s for a real slot,
 *                                                        the centre's for a slot of a patched query
 *     grad_features[b,c,j] = sum of g_f[b,c,p] over the real slots p with idx[b,p] == j, ascending p, fp32 from +0.0f
 *     grad_xyz[b,j,d]      = the same sum of a[d,p]
 *     grad_new_xyz[b,q,d]  = sum over k ascending, fp32 from +0.0f, of t_k = fl(g_c[k] - g_r[k]), and for a patched
 *                            query t_k = fl(fl(g_c[k] - g_r[k]) + a[k]);  without use_xyz both coordinate gradients
 *                            are +0.0f
 * Every output element is written exactly once, there are no float atomics, the same input gives the same bits, and a
 * cloud has the same bits alone and in a batch.  The inverse index of the *_grad_det calls (csrc/scatter_index.h) is
 * built once per call and serves grad_features and grad_xyz; grad_new_xyz is one more kernel.  No allocation, no
 * synchronisation: capturable.  workspace: pdr_query_group_cf_workspace_bytes(B, n, m, K) bytes, 4-byte aligned, the
 * caller's; needed when grad_features (C > 0) or, with use_xyz, grad_xyz is asked for.  Validation: the forward's size
 * checks in the same order (the empty problem leaves the gradient buffers alone), then the pointers. */
int pdr_query_group_cf_grad(const int *idx, const int *counts, const float *grad_out, int B, int n, int m, int K, int C,
                            int flags, float *grad_features, float *grad_xyz, float *grad_new_xyz, void *workspace,
                            pdr_stream_t stream);
/* Bytes of workspace pdr_query_group_cf_grad needs: pdr_scatter_workspace_bytes(B, m K, n) -- positive for positive
 * sizes within the limits, 0 for an empty, invalid or unsupported problem.  Host only. */
size_t pdr_query_group_cf_workspace_bytes(int B, int n, int m, int K);
/* The decision pdr_query_group_cf reads.  Host only.  C: the feature channels in use (0 without features);
 * aligned16 != 0: out is 16-byte aligned.  out = {family (0 scalar, 1 vector), grid.x (workgroups of 256 threads over
 * the m K positions, four per thread in the vector family), grid.y (channel slabs), feature slabs (8 channels each;
 * the coordinate channels are one more slab), output channels C + 3E, E}.  The size checks of the forward for one
 * cloud; m or K zero or a NULL out: PDR_EINVAL. */
int pdr_query_group_cf_plan(int n, int m, int K, int C, int flags, int aligned16, int out[6]);
/* Nearest-neighbour grouping of the TRAINABLE path: what group_knn(..., transpose=True)
 * (pointnet2_ops/pointnet2_utils.py) does after its neighbour search, channel-first, as one differentiable op (the
 * inference path gathers channel-last in pdr_knn_build):
 *     x (B,n1,3), y (B,n2,3), features (B,C,n2) or NULL, idx (B,n1,K) int32, dists (B,n1,K) f32
 *     ->  out (B, Cu + 11, n1, K) f32, channels [features | d2 | w | nn_abs (3) | nn_rel (3) | x (3)], Cu = C, or 0
 *         when features is NULL (C is ignored then).
 * idx and dists are what pdr_knn_group returned: no padding slot, 0 <= idx < n2; an index outside is the caller's
 * error, as for pdr_query_group_cf.  ONE launch, no atomics, no allocation, no synchronisation: capturable.  The
 * feature, d2, nn_abs and x channels are bit-for-bit copies of features[:, :, idx], dists, y[idx] and x[q];
 * nn_rel = fl(y[idx] - x[q]); w_k = fl(r_k / S) with r_k = fl(1.0f / fl(d_k + 1e-8f)) and S the fp32 sum of r_0 ..
 * r_{K-1} in ascending k from +0 (no fma anywhere) -- the bits of pdr_knn_group's weights.
 *   - two kernel families: vector (K % 4 == 0 and out 16-byte aligned: four k per thread, one 16-byte store per
 *     channel) and scalar (anything else); the same bits.  pdr_knn_group_cf_plan reports the decision.
 *   - limits: n2 <= 16384, n1 K <= 2^22, B <= 65535, B n1 K < 2^31 (the inverse-index builder's, so that every forward
 *     has its backward), B (Cu + 11) n1 K < 2^31 and Cu <= 524272 (the channel slabs are one grid dimension).
 *   - validation, decided on the host before any launch, in this order: B, n1, K or C negative, n2 <= 0: PDR_EINVAL;
 *     B, n1 or K zero: PDR_OK, nothing launched, no pointer looked at; the limits: PDR_EUNSUPPORTED; a NULL x, y, idx,
 *     dists or out: PDR_EINVAL. */
int pdr_knn_group_cf(const float *x, const float *y, const float *features, const int *idx, const float *dists, int B,
                     int n1, int n2, int K, int C, float *out, pdr_stream_t stream);
/* Backward of pdr_knn_group_cf.  x, y, idx, dists: the forward's; C: the feature channels of grad_out (0 when the
 * forward had no features); grad_out (B, C + 11, n1, K).  grad_features (B,C,n2), grad_x (B,n1,3), grad_y (B,n2,3):
 * each fully written, each may be NULL (autograd's needs_input_grad; its launches are skipped), all three NULL:
 * PDR_EINVAL.  g_f, g_d, g_w, g_a, g_r, g_c are the slices of grad_out; a slot p = (q, k) is REAL when
 * 0 <= idx[b,p] < n2 (an index outside is skipped, as in the *_grad_det calls; its e is +0).  With r_k, S, w_k as in the
 * forward, every operation rounded to fp32, no fma:
 *     dot = sum_k fl(g_w_k * w_k) ascending from +0;  h_k = fl(fl(g_w_k - dot) / S);
 *     G_k = fl(g_d_k - fl(fl(r_k * r_k) * h_k));  e = fl(x[q] - y[idx]);  t = fl(fl(2 G_k) * e)
 *     grad_x[b,q,d]        = sum over k ascending, fp32 from +0.0f, of fl(fl(g_c - g_r) + t)
 *     grad_features[b,c,j] = sum of g_f[b,c,p] over the real slots p with idx[b,p] == j, ascending p, fp32 from +0.0f
 *     grad_y[b,j,d]        = the same ordered sum of fl(fl(g_a + g_r) - t)
 * Every output element is written exactly once, there are no float atomics, the same input gives the same bits, and a
 * cloud has the same bits alone and in a batch.  The inverse index of the *_grad_det calls (csrc/scatter_index.h) is
 * built once per call and serves grad_features and grad_y; grad_x is one more kernel and needs no index.  No
 * allocation, no synchronisation: capturable.  workspace: pdr_knn_group_cf_workspace_bytes(B, n1, n2, K) bytes, 4-byte
 * aligned, the caller's; needed when grad_features (C > 0) or grad_y is asked for.  Validation: the forward's size
 * checks in the same order (the empty problem leaves the gradient buffers alone), then the pointers. */
int pdr_knn_group_cf_grad(const float *x, const float *y, const int *idx, const float *dists, const float *grad_out,
                          int B, int n1, int n2, int K, int C, float *grad_features, float *grad_x, float *grad_y,
                          void *workspace, pdr_stream_t stream);
/* Bytes of workspace pdr_knn_group_cf_grad needs: pdr_scatter_workspace_bytes(B, n1 K, n2) -- positive for positive
 * sizes within the limits, 0 for an empty, invalid or unsupported problem.  Host only. */
size_t pdr_knn_group_cf_workspace_bytes(int B, int n1, int n2, int K);
/* The decision pdr_knn_group_cf reads.  Host only.  C: the feature channels in use (0 without features);
 * aligned16 != 0: out is 16-byte aligned.  out = {family (0 scalar, 1 vector), grid.x (workgroups of 256 threads over
 * the n1 K positions, four per thread in the vector family), grid.y (channel slabs), feature slabs (8 channels each;
 * the 11 geometric channels are one more slab), output channels C + 11}.  The size checks of the forward for one
 * cloud; n1 or K zero or a NULL out: PDR_EINVAL. */
int pdr_knn_group_cf_plan(int n1, int n2, int K, int C, int aligned16, int out[5]);
/* Voxel-grid occupancy counters of a SET of clouds (the loop of entropy_of_occupancy_grid,
 * pointnet2/models/pvd/metrics/evaluation_metrics.py:198-237, which queries a KD-tree per cloud and counts in Python):
 *     clouds (S,n,3) f32  ->  counters[c] += points of all clouds whose nearest kept grid cell is c,
 *                             bernoulli[c] += clouds with at least one such point        (cells int32 each)
 * The call ADDS: the caller zero-initialises both arrays, so a set can be fed in chunks.  ONE launch (a workgroup per
 * cloud, its per-cell counts in LDS, then one integer atomic add per occupied cell and array), no workspace, no
 * allocation, no synchronisation, no floating-point atomics: the outputs are deterministic, and the call is capturable.
 *   - the grid is DATA built by the caller as the reference builds it (unit_cube_grid_point_cloud :163-181):
 *     axis[i] = (float)(i * spacing - 0.5), spacing = 1.0 / (R - 1) in double, R values; cell (i,j,k) has the linear
 *     index (i R + j) R + k and cell_of[linear] (R^3 int32) is its compact index in [0, cells) -- the kept cells
 *     numbered in ascending linear order -- or -1 for a cell that was clipped away.  All three in DEVICE memory.  An
 *     entry outside [0, cells) is treated as -1.
 *   - the nearest-cell rule.  The point is widened to double.  Per axis the index i with the smallest |axis[i] - p|
 *     (axis[i] widened, compared in double) is taken; the lower index wins a tie and a point beyond the ends clamps.
 *     If cell_of keeps that cell it is the answer; otherwise the answer is the kept cell with the smallest
 *     (dx dx + dy dy) + dz dz in double on the widened differences (no fused multiply-add).
 *     equal distances: the lowest compact index.  (sklearn's NearestNeighbors, which the reference queries, pins no
 *     order among EXACTLY tied cells: this order is the builder's contract, not a pin, as for pdr_knn_points.  On
 *     tie-free input -- the two nearest kept cells more than 1e-12 apart in squared distance -- the counters are
 *     identical to the reference's: tests/golden/make_jsd_golden.py asserts it.)
 *   - lengths follows pdr_chamfer_pairwise: int64 array of S entries in DEVICE memory, clamped on the device to [0, n],
 *     NULL = every cloud is full, n stays the row stride; rows at or beyond a length are never read for their value.
 *   - a point with a non-finite coordinate inside its length goes to no cell and adds 1 to skipped[0] (device int32,
 *     may be NULL); nothing is indexed with a value derived from it.  (So does every point when cell_of keeps no
 *     cell at all.)
 *   - validation, decided on the host before any launch: a negative size, n <= 0 with S > 0, cells <= 0 or a NULL
 *     clouds / axis / cell_of / counters / bernoulli: PDR_EINVAL; S == 0: PDR_OK, nothing launched, no pointer looked
 *     at; R outside [2, 32], cells > R^3 or S n >= 2^31: PDR_EUNSUPPORTED. */
int pdr_occupancy_grid(const float *clouds, const int64_t *lengths, int S, int n, int R,
                       const float *axis, const int32_t *cell_of, int cells,
                       int32_t *counters, int32_t *bernoulli, int32_t *skipped, pdr_stream_t stream);
/* pdr_knn_points for group_knn (pointnet2_utils.py:487-514) inside the fused network: same search, int32 indices
 * and the normalised interpolation weights w = (1/(d2+1e-8)) / sum_k (1/(d2_k+1e-8)) of :500-503 (SQUARED
 * distances, k ascending) in the same pass.  Requires K <= min(n2, 16). */
int pdr_knn_group(const float *x, const float *y, int B, int n1, int n2, int K, float *dists, int *idx,
                  float *weights, pdr_stream_t stream);
/* Which kernel pdr_knn_points / pdr_knn_points_ragged (group = 0; has_nn != 0: `nn` is asked for) or pdr_knn_group
 * (group = 1) runs for these sizes under the current knn_wave option.  Host only; the launches read the same decision.
 * out = {family (0 thread per query, 1 wave per query, 2 packed K = 1; -1: an empty call, nothing is launched), the
 * kernel's template parameter (thread: KMAX 1 / 4 / 8 / 16 / 32; wave: NCH 1 / 2 / 4 / 8 / 16 cloud slots per lane;
 * packed: query pairs per thread), queries per wave (0 outside the wave kernel), workgroups per cloud}.
 * Returns what the call itself returns before it looks at a pointer: PDR_EINVAL for a negative size or K <= 0 (group:
 * also n2 <= 0 or K > n2), PDR_EUNSUPPORTED for K > 32 (group: K > 16). */
int pdr_knn_plan(int B, int n1, int n2, int K, int has_nn, int group, int out[4]);

/* Backward of pdr_knn_points w.r.t. both clouds (pytorch3d knn_points backward, norm 2;
 * makes chamfer_loss_new.py:149-167 / calc_cd :234-245 differentiable as train.py:518 needs;
 * K = 1 cross-check: chamfer3D.cu:155-195):
 *   grad_x[p] = sum_k 2 g[p,k] (x[p] - y[idx[p,k]]),  grad_y[j] = -sum_{idx[p,k] = j} (same term).
 * idx < 0 (padding) is skipped.  grad_x (B,n1,3) is overwritten; grad_y (B,n2,3) is zeroed on the
 * stream and accumulated with float atomics (summation order not fixed; pdr_knn_points_grad_det below fixes it).
 * This skip is also what makes pdr_knn_points_ragged differentiable without a kernel of its own: its padded queries
 * and the slots beyond a cloud's length carry idx -1, so padded rows of either cloud receive exactly zero. */
int pdr_knn_points_grad(const float *x, const float *y, const int64_t *idx,
                        const float *grad_dists, int B, int n1, int n2, int K,
                        float *grad_x, float *grad_y, pdr_stream_t stream);

/* ---- deterministic backward twins -------------------------------------------
 * pdr_gather_points_grad, pdr_group_points_grad, pdr_three_interpolate_grad and the grad_y half of pdr_knn_points_grad
 * scatter with float atomics: the same gradient, but the order of the fp32 adds -- and with it the last bits -- changes
 * from run to run.  The _det calls below take the same arguments plus a workspace and compute the same sums in ONE
 * FIXED ORDER, so the same input gives the same bits; the atomic calls and their outputs are unchanged.
 *   - the summation order.  Every output element starts from +0.0f and its contributions are added one after the
 *     other in fp32, in ascending order of their SOURCE POSITION in the index array; every product is rounded before it
 *     is added (no fused multiply-add):
 *         gather / group   grad_points[b,c,d]  = sum over pos with idx[b,pos] == d, pos ascending, of grad_out[b,c,pos]
 *                          (pos = j for gather, j ns + k for group)
 *         interpolate      grad_points[b,c,d]  = sum over pos = 3 j + t with idx[b,j,t] == d, pos ascending, of
 *                          fl(grad_out[b,c,j] * weight[b,j,t])
 *         kNN grad_y       grad_y[b,d,c] = 0 - d_1 - d_2 - ... over pos = j K + t with idx[b,j,t] == d, pos ascending,
 *                          d_i = fl(fl(2 grad_dists[b,j,t]) * fl(x[b,j,c] - y[b,d,c])); idx < 0 is skipped
 *         kNN grad_x       as pdr_knn_points_grad (t ascending in registers: already order-fixed), the same bits
 *     This is the order of the sequential loops of oracle/pdr_oracle.c, whose results these calls reproduce bit for bit.
 *     A destination that no source names gets +0.0f.  Every output element is written exactly once.
 *   - how.  An inverse index (per destination, its source positions ascending) is built in the workspace by a stable
 *     counting sort -- integer atomics count, nothing floating-point is atomic --, then one thread per (destination,
 *     8-channel slab) adds its list; a list of 256 or more sources (a ball query without a hit names point 0 in every
 *     slot) is added by one wave, lane = channel, still one add after the other.  Five launches and one memset of a part
 *     of the workspace on `stream` (kNN: six launches), no allocation, no synchronisation: capturable.
 *   - P, the source positions per cloud, is m, np ns, 3 n and n1 K; N, the destinations, is N, N, m and n2.
 *     pdr_scatter_workspace_bytes(B, P, N) is the size of the workspace of such a call: positive for positive sizes,
 *     non-decreasing in each argument over the supported sizes, 0 for B <= 0 and for sizes the calls refuse.  Its contents are private and
 *     undefined afterwards; two calls in flight at once need a workspace each.
 *   - validation, decided on the host before any launch, in this order: the atomic twin's size checks and its empty
 *     cases with the twin's codes (B == 0: PDR_OK, nothing looked at); sizes these kernels do not index --
 *     N > 16384, P > 4194304, B > 65535 or B P >= 2^31 --: PDR_EUNSUPPORTED; then the twin's pointer checks, and with
 *     sources to add (P > 0; kNN: also n2 > 0) a NULL workspace, or one that is not 4-byte aligned: PDR_EINVAL.
 *     With P == 0 the output is zero-filled and the workspace is not looked at.
 *   - an index outside [0, N) is skipped (the kNN padding -1 by contract; any other such value is still an error of
 *     the caller, but it reaches no memory here). */
size_t pdr_scatter_workspace_bytes(int B, int P, int N);
int pdr_gather_points_grad_det(const float *grad_out, const int *idx, int B, int C, int N, int m,
                               float *grad_points, void *workspace, pdr_stream_t stream);
int pdr_group_points_grad_det(const float *grad_out, const int *idx, int B, int C, int N, int np, int ns,
                              float *grad_points, void *workspace, pdr_stream_t stream);
int pdr_three_interpolate_grad_det(const float *grad_out, const int *idx, const float *weight, int B, int C,
                                   int n, int m, float *grad_points, void *workspace, pdr_stream_t stream);
int pdr_knn_points_grad_det(const float *x, const float *y, const int64_t *idx, const float *grad_dists,
                            int B, int n1, int n2, int K, float *grad_x, float *grad_y, void *workspace,
                            pdr_stream_t stream);

/* ---- approximate EMD --------------------------------------------------------
 * approxmatch_forward(xyz1 (B,n,3), xyz2 (B,m,3)) -> match (B,m,n)
 *                                          emd_kernel.cu:29-161, host :174-196
 * matchcost_forward(xyz1, xyz2, match) -> cost (B)       :204-246, host :260-282
 * matchcost_backward(grad_cost (B), xyz1, xyz2, match) -> grad1 (B,n,3), grad2 (B,m,3)
 *                                                        :290-359, host :376-401
 * `temp` = device scratch of pdr_emd_workspace_bytes(B,n,m) bytes (the reference
 * allocates its own (B,2(n+m)) temp, :186).
 * pdr_emd_cost = matchcost(approxmatch()) without materialising the 4*B*n*m-byte
 * match matrix (what pointnet2/emd.py:12-16 needs when return_match=False and no
 * gradient is requested); cost is NOT yet divided by max(n,m).
 * pdr_approxmatch and pdr_emd_cost (and their _ragged forms) LEAVE in `temp` the per-level factors of the closed form
 *     match[b,l,k] = sum_level exp(level * |xyz1_k - xyz2_l|^2) * ratioL[level][k] * ratioR[level][l]
 * (10 * (n + m) floats per pair; the layout stays private).  This is a promise of the interface: pdr_emd_cost_grad
 * below reads them, so a caller that wants gradients keeps that workspace untouched until then. */
size_t pdr_emd_workspace_bytes(int B, int n, int m);       /* approxmatch, emd_cost */
size_t pdr_matchcost_workspace_bytes(int B, int n, int m); /* matchcost */
int pdr_approxmatch(const float *xyz1, const float *xyz2, int B, int n, int m,
                    float *match, float *temp, pdr_stream_t stream);
int pdr_matchcost(const float *xyz1, const float *xyz2, const float *match,
                  int B, int n, int m, float *cost, float *temp,
                  pdr_stream_t stream);
int pdr_matchcost_grad(const float *grad_cost, const float *xyz1,
                       const float *xyz2, const float *match, int B, int n,
                       int m, float *grad1, float *grad2, pdr_stream_t stream);
int pdr_emd_cost(const float *xyz1, const float *xyz2, int B, int n, int m,
                 float *cost, float *temp, pdr_stream_t stream);
/* Matrix-free matchcost_backward: the gradients of pdr_matchcost_grad on the match of pdr_approxmatch, without a
 * (B,m,n) matrix anywhere:
 *     grad1[b,k,:] = grad_cost[b] * sum_l 2 * match[b,l,k] * (xyz1[b,k] - xyz2[b,l])
 *     grad2[b,l,:] = grad_cost[b] * sum_k 2 * match[b,l,k] * (xyz2[b,l] - xyz1[b,k])
 * with match[b,l,k] evaluated on the fly from the factors in `temp`, by the expression pdr_approxmatch writes the
 * matrix with (same distance, same exp, levels summed in the same order): every pair contributes the value the matrix
 * would have held, and match is a constant of the differentiation, as in the reference (emd_kernel.cu:290-359).
 * `temp` is the workspace of pdr_emd_workspace_bytes(B,n,m) bytes that a preceding pdr_emd_cost[_ragged] or
 * pdr_approxmatch[_ragged] call on the SAME xyz1, xyz2, lengths, B, n and m left behind; it is only read, so one forward
 * serves any number of these calls.  Sums run sequentially over the opposite index and nothing is atomic: the same
 * input gives the same bits.  grad1 agrees bit for bit with pdr_matchcost_grad on that matrix; grad2 sums in index
 * order where pdr_matchcost_grad sums by lanes.  Two launches on `stream`, no allocation, no synchronisation
 * (capturable).  Validation and return codes are pdr_matchcost_grad's (B == 0: PDR_OK, nothing done). */
int pdr_emd_cost_grad(const float *grad_cost, const float *xyz1, const float *xyz2, const float *temp,
                      int B, int n, int m, float *grad1, float *grad2, pdr_stream_t stream);
/* The EMD calls with per-cloud lengths (the rules of pdr_knn_points_ragged: lengths1 / lengths2 are int64 arrays
 * of B entries in DEVICE memory, read by the kernels only and clamped there to [0, n] / [0, m]; the host never reads
 * them, so the calls neither synchronise nor allocate, stay capturable, and a replayed graph follows the lengths then
 * in memory; NULL = every cloud is full).  Cloud b is the pair xyz1[b, :n_b], xyz2[b, :m_b] with n_b = lengths1[b],
 * m_b = lengths2[b]; n / m stay the padded sizes: the row strides of xyz1, xyz2, match, the gradients and the
 * workspace, and the sizes pdr_emd_workspace_bytes / pdr_matchcost_workspace_bytes are asked with.  The reference has
 * no such call; the contract is that cloud b gets exactly what the dense call gives on the two slices:
 *   - the factors multiL / multiR (emd_kernel.cu:31-38) are per cloud, from (n_b, m_b) with the same integer division,
 *     computed on the device;
 *   - rows at or beyond a cloud's length are never candidates and never reach an output, whatever they hold (NaN
 *     included); the loops over the opposite cloud run to m_b / n_b, sequentially from index 0 in tiles of 1024, so
 *     the valid region is computed by the dense kernels' operation sequence (bit-identical to the dense call on the
 *     slices, cost included: the reductions over k do not depend on the padded n);
 *   - every output is fully written: match[b, l, k] = 0 for l >= m_b or k >= n_b (pdr_matchcost_ragged and
 *     pdr_matchcost_grad_ragged never READ those entries of a given match), gradient rows of padded points are
 *     exactly 0, cost[b] sums valid rows only;
 *   - a pair with n_b == 0 or m_b == 0 is empty: nothing is divided, cost 0, match rows 0, gradients 0.
 * Validation and return codes are the dense calls'; the launches are the dense calls' (same kernels' grids over the
 * padded sizes, same count); with NULL or full lengths the output is bit-identical to the dense call. */
int pdr_approxmatch_ragged(const float *xyz1, const float *xyz2, const int64_t *lengths1, const int64_t *lengths2,
                           int B, int n, int m, float *match, float *temp, pdr_stream_t stream);
int pdr_matchcost_ragged(const float *xyz1, const float *xyz2, const int64_t *lengths1, const int64_t *lengths2,
                         const float *match, int B, int n, int m, float *cost, float *temp, pdr_stream_t stream);
int pdr_matchcost_grad_ragged(const float *grad_cost, const float *xyz1, const float *xyz2, const int64_t *lengths1,
                              const int64_t *lengths2, const float *match, int B, int n, int m, float *grad1,
                              float *grad2, pdr_stream_t stream);
int pdr_emd_cost_ragged(const float *xyz1, const float *xyz2, const int64_t *lengths1, const int64_t *lengths2,
                        int B, int n, int m, float *cost, float *temp, pdr_stream_t stream);
/* pdr_emd_cost_grad under the same rules: rows at or beyond a cloud's length are never loaded (coordinates or
 * factors), never candidates, and get gradient exactly 0; an empty pair gets all-zero gradients; `temp` comes from a
 * preceding _ragged forward with the same lengths.  Two NULL length pointers: this IS pdr_emd_cost_grad. */
int pdr_emd_cost_grad_ragged(const float *grad_cost, const float *xyz1, const float *xyz2,
                             const int64_t *lengths1, const int64_t *lengths2, const float *temp,
                             int B, int n, int m, float *grad1, float *grad2, pdr_stream_t stream);

/* ==== fused channel-LAST layer kernels ========================================
 * These have no single pybind counterpart: each replaces a COMPOSITION of torch ops
 * the reference issues from Python on (B,C,npoint,K) tensors.  Activations here are
 * channel-last: X is (P positions, C channels), P = B*npoint*K.
 *
 * pdr_fused_layer   = [GroupNorm apply -> ReLU -> + embedding rows -> + residual ->
 *                      torch.cat of inputs] -> Conv2d 1x1 (+bias) -> moments of the output
 *                     (pointnet2_modules.py:42-67 build_shared_mlp, :69-174 Mlp_plus_t_emb,
 *                      attention.py:43-55 weight_conv / :60-66 feat_out_conv)
 * pdr_gn_reduce / pdr_gn_finalize = nn.GroupNorm statistics (MyGroupNorm,
 *                      pointnet2_modules.py:23-40) folded to per-(batch,channel) y = x*scale+shift
 * pdr_group_build   = QueryAndGroup.forward after ball_query (pointnet2_utils.py:368-414)
 * pdr_knn_build     = group_knn after knn_points (pointnet2_utils.py:497-510)
 * pdr_attention_pool= mask, softmax over K, weighted sum (attention.py:83-96)
 * pdr_gather_rows   = gather_operation on a channel-last matrix
 */
typedef struct {
  const float *ptr; /* (rows, C) with leading dimension ld */
  int C;
  int ld;
  int row_div;      /* source row = position / row_div (broadcast over K neighbours) */
  /* GATHERED source (gV != NULL): the value at position p of batch element b is
   *     ptr[(b * g_nsrc + gidx[p]) * ld + c]  +  gV[(p / gK) * g_ldv + c]
   * (neighbour row of a per-source-point table + query row), or gV0[(p / gK) * g_ldv + c] where
   * gcnt[p / gK] <= 0 (empty ball).  gidx / gcnt / gK live in pdr_layer_in_t.  This is the first
   * conv of a grouped block (see pdr_gather_add) consumed WITHOUT materialising its output. */
  const float *gV;
  const float *gV0;
  int g_ldv;
  int g_nsrc;
  /* Row index (relative to ptr, i.e. over all batch elements) of an ALL-ZERO row of the table, or -1.
   * With it (and gV0 - gV a small non-negative offset inside one allocation) empty balls are read as
   * "zero neighbour row + gV0 row" by plain address arithmetic; the wave-specialised kernel needs it
   * whenever gcnt is given. */
  int g_zrow;
  int g_reserved;
  /* kNN form of a gathered source (both non-NULL; group_knn's first conv, see pdr_gather_add): the value gets two
   * more per-position terms  + gs1[p] * g_r1[c] + gs2[p] * g_r2[c]  (gs1 = squared distance, gs2 = interpolation
   * weight of position p, in pdr_layer_in_t; g_r1 / g_r2 = the conv's rows of those two channels, offset to this
   * segment's first column, readable up to the segment's 4-padded width).  No empty balls in this form. */
  const float *g_r1;
  const float *g_r2;
} pdr_seg_t;

typedef struct {
  int n_seg;            /* 1..4 channel segments, concatenated in order */
  pdr_seg_t seg[4];
  const float *scale;   /* (B,Cin) or NULL(=1)  x' = post(pre(x)*scale + shift) + add + residual */
  const float *shift;   /* (B,Cin) or NULL(=0) */
  const float *add;     /* (B,Cin) rows of leading dimension add_ld, or NULL */
  pdr_seg_t rseg;       /* row-wise residual over all Cin channels (ptr NULL = none); may be gathered (ball or
                         * kNN form, sharing gidx / gcnt / gs1 / gs2 with the sources; the sources are plain then) */
  int add_ld;
  int pre_relu, post_relu;
  int rows_per_batch;   /* npoint*K: positions per batch element (one GroupNorm instance) */
  const int *gidx;      /* (P) neighbour index per position, shared by all gathered sources */
  const int *gcnt;      /* (P / gK) ball counts or NULL */
  int gK;               /* neighbours per query (power of two) */
  int ss_ld;            /* leading dimension of scale / shift rows (0 = Cin) */
  /* OUTPUT-side broadcast add: y[p, :] += oadd[(p / oadd_div) * oadd_ld + :] before the moments.
   * Used for the query half of the attention score conv: conv([q.expand(K) | k]) = conv_k(k) + Z[query] */
  const float *oadd;
  int oadd_ld;
  int oadd_div;         /* power of two */
  /* (round 6) NULL, or (P / oadd_div) ints: position p adds row oadd_rows[p / oadd_div] of `oadd` instead of row
   * p / oadd_div -- a block evaluated on SORTED queries reads the per-query term where the query conv wrote it, in the
   * original query order (no row gather of the query features in front of the query conv) */
  const int *oadd_rows;
  const float *gs1;     /* (P) per-position scalars of kNN-form gathered sources (see pdr_seg_t.g_r1), or NULL */
  const float *gs2;
  /* A SUBSET of the row tiles (NULL: all of them): the launch computes the row tiles tile_list[0 .. *n_tiles)
   * (row tile = b * tiles_per_batch + t, both in device memory: the subset is decided on the device, see
   * pdr_dedup_plan) and neither reads nor writes the rows of any other tile.  Wave-specialised tile shapes only
   * (PDR_EUNSUPPORTED otherwise). */
  const int *tile_list;
  const int *n_tiles;
  /* pooled launches (pdr_fused_layer_pool*): query q's pooled row is written to row out_rows[q] of `out` (NULL: row q)
   * -- a block evaluated on sorted queries (pdr_dedup_sort) writes its output in the original order.  Wave-specialised
   * tile shapes only. */
  const int *out_rows;
  int partial_tpb;      /* rows of `partial` per batch element (0 = tiles_per_batch): tile t of batch element b
                         * writes row b * partial_tpb + t */
  /* WEIGHTED statistics (per-query launches of a deduplicated block, round 5): NULL, or (B) ints -- only the rows
   * r >= wrow0[b] of batch element b (r = row within the batch element) count in `partial`, and the tile's moments
   * are multiplied by wmul (the K copies each such row stands for).  Y is written for every row. */
  float wmul;
  const int *wrow0;
  /* pooled launches (pdr_fused_layer_pool*): NULL, or the per-QUERY value rows (P / K, patch_ld) of a deduplicated
   * block -- before it walks its tiles the launch writes out[out_rows ? out_rows[q] : q, :] = act(patch_values[q, :] *
   * vscale + vshift) for every query q with patch_w[q] > 0 (= pdr_patch_rows, without its launch).  Wave-specialised
   * tile shapes only; D, patch_ld and ldo multiples of 4. */
  const float *patch_values;
  const float *patch_w;
  int patch_ld;
  /* (the former reserved_ field, 0 = as before) wave-specialised tile shapes without a tile_list: nonzero = the launch
   * walks its row tiles from the last to the first.  Which rows a tile holds, Y and `partial` do not change -- only the
   * order in time; a caller alternates it along a chain of layers whose activations exceed the memory-side cache. */
  int walk_reverse;
} pdr_layer_in_t;

/* rows per workgroup tile chosen for `rows_per_batch` and `Cout` (256/128/64/32); a batch element is cut
 * into ceil(rows_per_batch / tile) tiles, the last one possibly partial.  This is the row count behind each
 * row of the `partial` statistics of pdr_fused_layer. */
int pdr_fused_layer_tile_rows(int rows_per_batch, int Cout);
/* index of the kernel instantiation used for this shape: 0 256x32, 1 256x64 (16-channel chunks; with
 * PDR_NARROW_KC32=0 only), 2 128x96, 3 128x160, 4 128x128 (2-D grid), 5 64x128, 6 32x128, 7 128x32, 8 128x64
 * (32-channel chunks: the default for outputs of <= 64 channels) */
int pdr_fused_layer_variant(int rows_per_batch, int Cout);
/* The launch pdr_fused_layer would make for these arguments, without launching (profilers attribute a call
 * to its kernel symbol): out[0..6] (8 ints of space) = {wave-specialised kernel (csrc/fused_layer_ws.hip)?,
 * tile variant id, residual source?, gathered source (0 none, 1 ball form, 2 kNN form), float4 staging?,
 * split-f16 arithmetic?, thin kernel (<= 4 input channels, no prologue; used when `partial` is NULL)?}; out[7] = 128
 * when the launch is a RIGHT-SIZED TINY LAYER, else 0: a layer whose tiles number at most 256 (32-row tiles), 512 in
 * 64 x 64 tiles (64-row tiles, plain sources) or 128 (128-row tiles, plain sources) and has > 64 input channels runs on
 * the uniform-wave kernel with 128-channel chunks and 32 x 32 (the four waves of a workgroup each walk a quarter of
 * the input channels) / 64 x 32 (two ways) / 128 x 64 tiles (out[0] = 0 then) -- a launch of a few dozen workgroups is
 * bound by its serial chunk walk and its waves' MFMA chains, not by the matrix pipes.  The rows of `partial` per
 * batch element do not change (same row tiles).  PDR_DEEP_CHUNKS=0: never.
 * Same return codes as pdr_fused_layer.  Process-wide tuning knob read once: PDR_FUSED_WS=0 selects the uniform-wave kernels. */
int pdr_fused_layer_plan(const pdr_layer_in_t *in, long P, int Cin, const float *Wt, int ldw, int Cout,
                         const float *Y, int ldy, int *out);
/* Y (P,Cout; ld ldy) = prologue(X) . Wt + bias, Wt (Cin,Cout) row-major (the conv weight
 * transposed; 16-B aligned, leading dimension ldw >= Cout with ldw % 4 == 0), exact fp32 MFMA.
 * Sources whose pointers are 16-B aligned and whose leading dimensions are multiples of 4 floats
 * (rows padded to a multiple of 4 channels) are staged with 16-B loads; what the padding columns hold is never used
 * (they may be uninitialised, NaN included: channels beyond a segment's C enter the product as exact zeros).  partial: NULL or (B*tiles_per_batch, Cout, 2) floats receiving the
 * per-tile sum / sum of squares of y (columns >= relu_col0: of relu(y)). */
int pdr_fused_layer(const pdr_layer_in_t *in, long P, int Cin, const float *Wt, int ldw,
                    const float *bias, int Cout, float *Y, int ldy, float *partial,
                    int relu_col0, pdr_stream_t stream);
/* pdr_fused_layer over TWO row sets in ONE launch (round 6): (in, Y, partial) = a tile subset (in->tile_list) of 128-row
 * tiles with plain or ball-gathered sources and no residual; (in2, Y2, partial2) = plain sources, typically with weighted
 * statistics (wrow0 / wmul) and its rows of `partial` behind the first problem's (partial2 = their first row; one row per
 * 128 rows of a batch element, in2->partial_tpb rows per batch element).  Same weights, bias, Cout and relu_col0.  A
 * deduplicated block's per-neighbour launch and per-query launch of one layer become one link of its launch chain; the
 * values written are those of the two pdr_fused_layer calls.  PDR_EUNSUPPORTED: launch them one by one. */
int pdr_fused_layer_pair(const pdr_layer_in_t *in, long P, const pdr_layer_in_t *in2, long P2, int Cin, const float *Wt,
                         int ldw, const float *bias, int Cout, float *Y, int ldy, float *Y2, int ldy2, float *partial,
                         float *partial2, int relu_col0, pdr_stream_t stream);
/* pdr_fused_layer in SPLIT-f16 arithmetic (opt-in, never the default): x . w is evaluated as xh wh + xh wl + xl wh
 * with xh = f16(x), xl = f16(x - xh) (same for w) on v_mfma_f32_32x32x16_f16, fp32 accumulation: every operand is
 * held to max(2^-23 |x|, 2^-25) (two 11-bit halves; the MFMA honours the subnormal lo parts), the dropped xl wl term
 * is 2^-22 relative -- fp32-class products at 3/16 of the fp32 MFMA cycles, PROVIDED the operands are of ordinary
 * magnitude.  RANGE CONTRACT of the activations (after the prologue): the conversions run with MODE.FP16_OVFL = 1,
 * so an overflowing half saturates at +-65504 instead of becoming inf: |x| <= 131008 is represented as
 * hi = +-65504 + lo like any other value (relative error <= 2^-11 * 65504 / |x| above 65504, i.e. still 2^-12);
 * beyond 131008 both halves SATURATE and the product is silently that of the clamped operand -- finite, never NaN
 * (before round 4 |x| > 65504 produced inf - inf = NaN).  Weights outside the f16 range are refused when the
 * image is packed.  Inputs whose rms is below ~1e-3 lose relative accuracy to the 2^-25 absolute floor (the fused
 * network feeds these layers GroupNorm outputs, coordinates, embeddings and first-conv sums of O(1-100)).
 * `Wp`: the weights packed by the caller, 16-byte aligned: for every column block cb (128 columns; 64 for tile
 * variant 8) and every K-chunk c (the input segments in order, each cut into chunks of 32 channels, the
 * last one zero-padded) one block  [hi | lo] x [columns][32 k] halves (k contiguous, 64-byte rows) whose
 * 16-byte granule g of column n is stored at position g ^ ((n >> 2) & 3);  block index = cb * nchunks + c.
 * Available for the wave-specialised tile variants 4, 5 and 8 (pdr_fused_layer_variant); returns PDR_EUNSUPPORTED
 * otherwise -- callers then use pdr_fused_layer. */
int pdr_fused_layer_f16x3(const pdr_layer_in_t *in, long P, int Cin, const void *Wp, int nchunks,
                          const float *bias, int Cout, float *Y, int ldy, float *partial, int relu_col0,
                          pdr_stream_t stream);
/* pdr_fused_layer whose output (the attention scores, D channels) is consumed in the epilogue:
 * out[q,:] = sum_k softmax_k(mask(scores))[k,:] * act(values[q*K+k,:]*vscale + vshift); the (P x D)
 * score tensor is never written.  K in {8,16,32}; counts (P/K) or NULL = all neighbours valid.
 * = weight_conv's last Conv2d + mask + F.softmax + weighted sum (attention.py:83-96).
 * Plain (not gathered) sources without residual or per-query output term; rows_per_batch % 32 == 0.
 * Carried by the wave-specialised tiles when rows_per_batch is a multiple of the tile rows (every shape of the
 * shipped configs), by the uniform-wave kernel otherwise. */
int pdr_fused_layer_pool(const pdr_layer_in_t *in, long P, int Cin, const float *Wt, int ldw,
                         const float *bias, int D, const float *values, int ldv, const float *vscale,
                         const float *vshift, int v_relu, const int *counts, int K, float *out,
                         int ldo, pdr_stream_t stream);
/* the same with the score conv on split-f16 arithmetic: Wp / nchunks = the packed weight image of
 * pdr_fused_layer_f16x3; 128-column wave-specialised tiles only (PDR_EUNSUPPORTED otherwise) */
int pdr_fused_layer_pool_f16x3(const pdr_layer_in_t *in, long P, int Cin, const void *Wp, int nchunks,
                               const float *bias, int D, const float *values, int ldv,
                               const float *vscale, const float *vshift, int v_relu, const int *counts,
                               int K, float *out, int ldo, pdr_stream_t stream);
/* The launch a pooled entry point would make for these arguments, without launching (host only; nothing behind the
 * pointers is read): split = 0 asks for pdr_fused_layer_pool (W = Wt, ldw_or_nchunks = ldw), split != 0 for
 * pdr_fused_layer_pool_f16x3 (W = Wp, ldw_or_nchunks = nchunks).  Returns exactly the code that entry point returns for
 * the same `in`, P, Cin, weights, D, values, ldv, K, out and ldo (bias, vscale, vshift, v_relu, counts and the stream
 * decide nothing); PDR_EINVAL also when `plan` is NULL.  On PDR_OK plan[0..7] (8 ints) =
 *   {wave-specialised kernel (csrc/fused_layer_ws.hip; 0 = the uniform-wave kernel's pooled epilogue)?,
 *    tile variant id (pdr_fused_layer_variant(rows_per_batch, D)), split-f16 arithmetic?,
 *    row tiles of the launch = P / rows_per_batch * ceil(rows_per_batch / tile rows) (with a tile subset: the tiles the
 *    list is drawn from), column blocks = ceil(D / tile columns),
 *    tile subset (in->tile_list)?, row map (in->out_rows)?, patched rows (in->patch_values)?};
 * `plan` is not written otherwise.  The wave-specialised kernel is taken when PDR_FUSED_WS is not 0, rows_per_batch is a
 * multiple of the tile rows and the variant has one (not 3, not 6); the last three need it. */
int pdr_fused_layer_pool_plan(const pdr_layer_in_t *in, long P, int Cin, const void *W, int ldw_or_nchunks,
                              int D, const float *values, int ldv, int K, const float *out, int ldo,
                              int split, int *plan);
/* chan_stats[b, coff+c] (double sum, double sumsq) = mult * sum over tiles of batch b;
 * `partial` points at the first of C columns inside rows of ldp columns */
int pdr_gn_reduce(const float *partial, int ldp, int B, int tiles_per_batch, int C, double mult,
                  double *chan_stats, int Ctot, int coff, pdr_stream_t stream);
/* pdr_gn_reduce (x1 or x2 sources) + pdr_gn_finalize in one launch; part1 may be NULL.
 * nvalidX (NULL, or (B) ints) / tpb_mainX: source X was produced by a tile SUBSET (pdr_layer_in_t.tile_list on sorted
 * queries, pdr_dedup_prepare): of the first tpb_mainX partial rows of batch element b only the first nvalidX[b] were
 * written and only those are summed; rows >= tpb_mainX (the per-query rows' weighted moments) always count. */
int pdr_gn_fold(const float *part0, int ldp0, int tpb0, int C0, double mult0, const float *part1,
                int ldp1, int tpb1, int C1, double mult1, int B, int Cn, int G, double n, float eps,
                const float *gamma, const float *beta, float *scale, float *shift, const int *nvalid0,
                int tpb_main0, const int *nvalid1, int tpb_main1, pdr_stream_t stream);
/* out (P,C; ld ldo >= C) = prologue(X): materialise an activation descriptor,
 *     out[p, c] = post(pre(x[p, c]) * scale[b, c] + shift[b, c]) + add[b, c] + residual[p, c],  b = p / rows_per_batch,
 * the product and the shift as one fused multiply-add, then one fp32 addition per present term, in this order; columns
 * [C, ldo) of `out` are not touched.  Plain sources only (a gathered segment or residual: PDR_EUNSUPPORTED), row_div a
 * power of two, segment widths summing to C.  The RESIDUAL is read as rseg.ptr[p * rseg.ld + c] for every column c of
 * the C: only `ptr` and `ld` of rseg are consulted, its `C` and `row_div` are not (a residual is one row per position
 * over all channels; a column offset goes into ptr). */
int pdr_apply_act(const pdr_layer_in_t *in, long P, int C, float *out, int ldo,
                  pdr_stream_t stream);
/* out (B,C) = max over the rows of every batch element of prologue(X) (plain sources, no residual): the global
 * max-pooling of Pnet2Stage (pnet.py:27-40: F.max_pool2d over all points) on a lazily-activated layer output */
int pdr_act_colmax(const pdr_layer_in_t *in, long P, int C, float *out, pdr_stream_t stream);
/* GroupNorm(G groups over the first Cn of C channels; the rest pass through), n elements
 * per channel per batch element -> scale, shift (B,C) */
int pdr_gn_finalize(const double *chan_stats, int B, int C, int Cn, int G, double n, float eps,
                    const float *gamma, const float *beta, float *scale, float *shift,
                    pdr_stream_t stream);
/* out (B*m*K rows of leading dimension ldo >= Cs+3[+3][+3]) = [feats[idx] | rel | abs | centre];
 * feats (B,n,Cs) channel-last (NULL when Cs == 0); columns beyond the row width are zero-filled, at most 8 of them
 * (ldo - width > 8: PDR_EINVAL).  rel = xyz[b, idx] - new_xyz[b, j]; abs (with_abs) = xyz[b, idx]; centre
 * (with_centre) = new_xyz[b, j].  patch_empty (needs counts): a query with counts[b, j] <= 0 gets a zero feature,
 * rel = 0 and abs = its centre in all K slots (QueryAndGroup with subset=False); otherwise counts may be NULL and is
 * not read. */
int pdr_group_build(const float *feats, int Cs, const float *xyz, const float *new_xyz,
                    const int *idx, const int *counts, int B, int n, int m, int K,
                    int patch_empty, int with_abs, int with_centre, float *out, int ldo,
                    pdr_stream_t stream);
/* out (B*n1*K rows, ld ldo) = [feats_y[idx] | d2 | w | nn_abs | nn_rel | x]; idx int64 (B,n1,K), d2 (B,n1,K) the
 * squared distances of pdr_knn_points; feats_y (B,n2,C) channel-last (NULL when C == 0).
 *   w[p] = (1/(d2[p]+1e-8)) / norm,  norm = sum over k = 0..K-1, in this order, of 1/(d2[b,i,k]+1e-8)   (fp32)
 *   nn_abs = y[b, idx], nn_rel = nn_abs - x[b,i], x = x[b,i]; every other column is a copy.
 * C+11 <= ldo <= C+11+8 (PDR_EINVAL otherwise); the columns [C+11, ldo) of every row are zero-filled, for every C.
 * Every index must lie in [0, n2): the search must have been made with K <= n2 (pdr_knn_points pads K > n2 with
 * idx -1, which this call would read out of bounds -- values are not inspected). */
int pdr_knn_build(const float *feats_y, int C, const float *x, const float *y,
                  const long long *idx, const float *d2, int B, int n1, int n2, int K,
                  float *out, int ldo, pdr_stream_t stream);
/* out (B*npoint, D) = sum_k softmax_k(mask(scores)) * act(values*vscale+vshift);
 * scores/values (B*npoint*K, D) with leading dims lds/ldv; counts (B,npoint) or NULL = 'all' */
int pdr_attention_pool(const float *scores, int lds, const float *values, int ldv,
                       const float *vscale, const float *vshift, int v_relu, const int *counts,
                       int B, int npoint, int K, int D, float *out, pdr_stream_t stream);
/* First 1x1 conv of a grouped block without the grouped tensor (the conv is linear in the gathered
 * rows): Y[p,:] = U[b, idx[p], :] + V[p / K, :] (+ s1[p] r1[:] + s2[p] r2[:]); where counts[p / K] <= 0
 * (empty ball, subset=False) Y[p,:] = V0[p / K, :].  Replaces QueryAndGroup / group_knn + the first
 * Conv2d (pointnet2_utils.py:368-414, 497-510; pointnet2_modules.py:119-121).  Moments as in
 * pdr_fused_layer with 128-row tiles.  All leading dimensions multiples of 4 floats, all row pointers
 * 16-byte aligned.  Only the column window [ycol0, ycol0 + ycols) of the result is written, to columns
 * [0, ycols) of Y (ycol0 a multiple of 4; ycols = -1: through the last column); Y may be NULL (moments
 * only).  Consumers read the unwritten columns as a GATHERED source of pdr_fused_layer. */
int pdr_gather_add(const float *U, int ldu, int n_src, const float *V, const float *V0, int ldv,
                   const int *idx, const int *counts, const float *s1, const float *r1,
                   const float *s2, const float *r2, int B, int rows_per_batch, int K, int Cout,
                   float *Y, int ldy, float *partial, int relu_col0, int ycol0, int ycols,
                   pdr_stream_t stream);

/* ---- Neighbourhoods that are K copies of one row --------------------------------------
 * ball_query pads a neighbourhood with its first hit (ball_query_gpu.cu:29-44), so a query with at most one point
 * in its ball (an empty ball of a feature-transfer block is replaced by the query itself, pointnet2_utils.py:
 * 387-401) contributes K identical rows to every per-neighbour tensor of its block.  pdr_dedup_plan marks the
 * 128-row tiles all of whose queries are such copies; the block's per-neighbour launches skip them
 * (pdr_layer_in_t.tile_list, pdr_gather_add_tiles) and a per-QUERY chain of the same layers supplies their
 * GroupNorm moments (pdr_weighted_moments) and pooled rows (pdr_patch_rows).
 *
 * pdr_dedup_plan: idx (B,m,K) int32 / counts (B,m) of a ball query -> idx0 (B,m) first neighbours; row_w (B,m)
 * float = K for the queries of skipped tiles, else 0; tile_valid (B*m*K/128) bytes; tile_list (same length: the
 * valid row-tile numbers, ascending) and n_tiles (1).  K in {8,16,32}, m*K a multiple of 128. */
int pdr_dedup_plan(const int *idx, const int *counts, int B, int m, int K, int *idx0, float *row_w,
                   unsigned char *tile_valid, int *tile_list, int *n_tiles, pdr_stream_t stream);
/* pdr_dedup_sort + pdr_gather_rows of the ball query's index rows / counts / query coordinates into the sorted order +
 * pdr_dedup_plan on the sorted arrays, in ONE launch (round 5; same values): perm, inv, perm_rows (B,m) as
 * pdr_dedup_sort; idx_s (B,m,K), counts_s (B,m), xyz_s (B,m,3; xyz may be NULL) the inputs in that order; idx0, row_w,
 * tile_valid, tile_list, n_tiles as pdr_dedup_plan; nvalid (2 B ints): [b] = valid tiles of cloud b -- with sorted
 * queries its FIRST nvalid[b] tiles --, [B + b] = nvalid[b] * (128 / K) = the first query of its skipped tiles
 * (pdr_layer_in_t.wrow0 of the per-query launches, pdr_gn_fold's nvalid); probe_acc (NULL or 2 ints, accumulated with
 * atomics): [0] += sum_b nvalid[b], [1] += B m K / 128.  B <= 1024, m <= 4096 (PDR_EUNSUPPORTED beyond: the six
 * launches it replaces), idx / idx_s 16-byte aligned. */
int pdr_dedup_prepare(const int *idx, const int *counts, const float *xyz, int B, int m, int K, int *perm, int *inv,
                      int *perm_rows, int *idx_s, int *counts_s, float *xyz_s, int *idx0, float *row_w,
                      unsigned char *tile_valid, int *tile_list, int *n_tiles, int *nvalid, int *probe_acc,
                      pdr_stream_t stream);
/* the probe counters of pdr_dedup_prepare without the plan: probe_acc[0] += the tiles a plan of these ball counts
 * would walk, [1] += B m K / 128 (the step with every neighbourhood evaluated carries it, so that the sampler can
 * tell which of its two captured steps the next x_t wants: reverse_sampler.py) */
int pdr_dedup_probe(const int *counts, int B, int m, int K, int *probe_acc, pdr_stream_t stream);
/* Stable partition of every cloud's queries, those with more than one neighbour first: perm[b][j] = original index
 * of the query at sorted position j, inv = the inverse.  A block evaluated on its queries in that order (its per-query
 * inputs through pdr_gather_rows with perm, its output through pdr_gather_rows with inv) has its one-point
 * neighbourhoods in whole tiles.  perm_rows (NULL or (B,m)): b * m + perm[b][j], the same permutation as row numbers
 * of a (B*m)-row tensor (pdr_layer_in_t.out_rows, pdr_patch_rows). */
int pdr_dedup_sort(const int *counts, int B, int m, int *perm, int *inv, int *perm_rows, pdr_stream_t stream);
/* pdr_gather_add over the tiles with tile_valid[tile] != 0 only (the others are neither read nor written); tile t
 * of batch element b writes row b * partial_tpb + t of `partial`. */
int pdr_gather_add_tiles(const float *U, int ldu, int n_src, const float *V, const float *V0, int ldv,
                         const int *idx, const int *counts, const float *s1, const float *r1,
                         const float *s2, const float *r2, int B, int rows_per_batch, int K, int Cout,
                         float *Y, int ldy, float *partial, int relu_col0, int ycol0, int ycols,
                         const unsigned char *tile_valid, int partial_tpb, pdr_stream_t stream);
/* pdr_gather_add_tiles + the block's per-QUERY rows in the same launch (round 5: was a K = 1 pdr_gather_add on the
 * first neighbours + pdr_weighted_moments): Yd (B*m, ldyd) <- U[b, idx0[q]] + V[q] (empty ball: V0[q]), every column,
 * m = rows_per_batch / K; partial row b*partial_tpb + tiles_per_batch + j <- wmul x the moments of the rows
 * q >= wrow0[b] of the j-th group of 128 queries of cloud b.  Ball form (no s1 / s2);
 * partial_tpb >= tiles_per_batch + ceil(m / 128). */
int pdr_gather_add_tiles_twin(const float *U, int ldu, int n_src, const float *V, const float *V0, int ldv,
                              const int *idx, const int *counts, int B, int rows_per_batch, int K, int Cout, float *Y,
                              int ldy, float *partial, int relu_col0, int ycol0, int ycols,
                              const unsigned char *tile_valid, int partial_tpb, const int *idx0, float *Yd, int ldyd,
                              const int *wrow0, float wmul, pdr_stream_t stream);
/* The STATISTICS-ONLY pass of pdr_gather_add / _tiles / _tiles_twin (Y == NULL there) over one or two column windows
 * [win0_col0, win0_col0 + win0_cols) and [win1_col0, win1_col0 + win1_cols) (win1_cols = 0: one window): ascending,
 * disjoint, inside [0, Cout).  Only the windows' columns are gathered and reduced; their moments go to the same entries
 * of `partial` as pdr_gather_add's, with the same bits, and every other entry of `partial` is left unwritten (the
 * first conv of a grouped block is [first | residual | key]: no GroupNorm reads the residual window's moments).  The
 * twin form writes Yd whole, as pdr_gather_add_tiles_twin.  PDR_EUNSUPPORTED when a window does not start on a
 * multiple of 4 columns (use pdr_gather_add); PDR_EINVAL for windows that overlap, descend or leave [0, Cout), a NULL
 * partial, and whatever pdr_gather_add rejects. */
int pdr_gather_moments(const float *U, int ldu, int n_src, const float *V, const float *V0, int ldv,
                       const int *idx, const int *counts, const float *s1, const float *r1,
                       const float *s2, const float *r2, int B, int rows_per_batch, int K, int Cout,
                       float *partial, int relu_col0, int win0_col0, int win0_cols, int win1_col0, int win1_cols,
                       pdr_stream_t stream);
int pdr_gather_moments_tiles(const float *U, int ldu, int n_src, const float *V, const float *V0, int ldv,
                             const int *idx, const int *counts, const float *s1, const float *r1,
                             const float *s2, const float *r2, int B, int rows_per_batch, int K, int Cout,
                             float *partial, int relu_col0, int win0_col0, int win0_cols, int win1_col0,
                             int win1_cols, const unsigned char *tile_valid, int partial_tpb, pdr_stream_t stream);
int pdr_gather_moments_tiles_twin(const float *U, int ldu, int n_src, const float *V, const float *V0, int ldv,
                                  const int *idx, const int *counts, int B, int rows_per_batch, int K, int Cout,
                                  float *partial, int relu_col0, int win0_col0, int win0_cols, int win1_col0,
                                  int win1_cols, const unsigned char *tile_valid, int partial_tpb, const int *idx0,
                                  float *Yd, int ldyd, const int *wrow0, float wmul, pdr_stream_t stream);
/* Host-only (nothing is launched, no pointer exists): what pdr_gather_add* / pdr_gather_moments* launch for these sizes,
 * windows and pointers -- the decision of the ONE host function their launch path reads, with the same return code as
 * the call for every refusal that does not depend on a pointer's value.  flags: which optional pointers the call
 * carries; a pointer that goes with a flagged one (V0 with counts, r1 with s1, r2 with s2, Yd and wrow0 with idx0) and
 * every required pointer count as given and 16-byte aligned.  The windows of pdr_gather_add* are (0, Cout, 0, 0); ldy /
 * ycol0 / ycols are read with PDR_GATHER_HAS_Y only, partial_tpb with _TILES / _TWIN, ldyd with _TWIN.  out (24 ints;
 * all 0 for a refused or an empty (B = 0) call):
 *   [0]  lanes per row LPR: 16 (Cout <= 64) / 32 (Cout <= 128) / 64      [1]  KPOW2: K a power of two <= 32
 *   [2]  HAS_S: s1 or s2                [3]  HAS_EM: counts              [4]  YWIN: a Y is written
 *   [5]  statistics (partial != NULL)   [6]  the main tiles walk one V row per query: KPOW2 and K >= out[7]
 *   [7]  rows a wave walks per iteration with this LPR (16 / 8 / 4)
 *   [8]..[11]  the windows as walked: first column and length of the first, of the second (length 0: one window)
 *   [12] float4 pieces of the windows   [13] column passes = ceil([12] / LPR)
 *   [14] grid.x = [16] + [17]           [15] grid.y: [13] when the passes are dealt to workgroups ([14] <= 1024 and
 *        [13] > 1), else 1: every workgroup walks its tile's passes one after the other
 *   [16] main tiles = B [18]            [17] twin tiles = B [19]
 *   [18] 128-row tiles per cloud        [19] twin tiles per cloud = ceil(rows_per_batch / K / 128); 0: no twin form
 *   [20] [21] the written window of Y: first column, length padded to 4 (0: no Y)
 *   [22] a tile subset is walked        [23] 0 (reserved) */
#define PDR_GATHER_HAS_COUNTS 1u
#define PDR_GATHER_HAS_S1 2u
#define PDR_GATHER_HAS_S2 4u
#define PDR_GATHER_HAS_Y 8u
#define PDR_GATHER_HAS_PARTIAL 16u
#define PDR_GATHER_HAS_TILES 32u /* tile_valid */
#define PDR_GATHER_HAS_TWIN 64u  /* idx0 / Yd / wrow0: pdr_gather_*_tiles_twin */
int pdr_gather_plan(int B, int n_src, int rows_per_batch, int K, int Cout, int ldu, int ldv, int ldy, int ycol0,
                    int ycols, int win0_col0, int win0_cols, int win1_col0, int win1_cols, int partial_tpb, int ldyd,
                    unsigned flags, int out[24]);
/* Moments of a materialised (B*rpb, C) tensor with one weight per row, appended to the moments of a tile subset:
 * partial row b*ptpb + tpb_full + j  <-  sum_r w[r] f, sum_r w[r] f^2 over the rows r of 128-row tile j of batch
 * element b (f = y, columns >= relu_col0: max(y,0)); partial rows b*ptpb + t (t < tpb_full) of the tiles with
 * tile_valid[b*tpb_full + t] == 0  <-  0.  ptpb >= tpb_full + ceil(rpb/128). */
int pdr_weighted_moments(const float *Y, int ldy, int B, int rpb, int C, int relu_col0, const float *row_w,
                         float *partial, int ptpb, int tpb_full, const unsigned char *tile_valid,
                         pdr_stream_t stream);
/* out[r,:D] = act(V[q,:D] * vscale[b] + vshift[b]) for the rows q with row_w[q] > 0, r = out_rows[q] (NULL: q); other
 * rows untouched. */
int pdr_patch_rows(const float *V, int ldv, const float *vscale, const float *vshift, int v_relu,
                   const float *row_w, int B, int rpb, int D, float *out, int ldo, const int *out_rows,
                   pdr_stream_t stream);
/* out (B,m,C) = src (B,n,C)[idx (B,m)] */
int pdr_gather_rows(const float *src, const int *idx, int B, int n, int C, int m, float *out,
                    pdr_stream_t stream);


/* ---- reverse-step update ------------------------------------------------------
 * The elementwise tail of one reverse step in one launch, step index and constants on the device:
 *   mode 0 (util.py:246-250 `sampling`):       x <- (x - A[t] eps) / B[t] + C[t] z
 *                                              A = (1-alpha)/sqrt(1-alpha_bar), B = sqrt(alpha), C = sigma (C[0] = 0)
 *   mode 1 (util_fastdpmv2.py:186-204):        x <- x A[t] + (B[t] eps + C[t] z)
 * x, z (npoints,3) dense (z may be NULL = 0); eps rows `ld_eps` floats apart; t_dev: int64 step index in device
 * memory.  Same operations in the same order as the PyTorch expression (bit-identical). */
int pdr_reverse_update(float *x, const float *eps, int ld_eps, const float *z, const float *tab_a,
                       const float *tab_b, const float *tab_c, const long long *t_dev, long npoints,
                       int mode, pdr_stream_t stream);
/* pdr_reverse_update + the step bookkeeping around it in ONE launch (util.py:246-250 plus the loop header
 * `for t in range(T-1,-1,-1)` / `ts = t * ones(B)` of :232-236; util_fastdpmv2.py:186-204, 340-376):
 *   noise:  rng_state != NULL: z ~ N(0,1) drawn in the kernel (Philox4x32-10, key = rng_state[0], counter =
 *           (element quad, rng_state[1])), `z` ignored; else z as in pdr_reverse_update (NULL = 0);
 *   after the update the last workgroup (device ticket, `ticket` = one zero-initialised int, left zero) sets
 *   *t_dev -= 1, *ts_out = ts_table ? ts_table[t-1] : float(t-1) (skipped when ts_out == NULL or t-1 < 0) and
 *   rng_state[1] += 1.  Same arithmetic, operation order and rounding as pdr_reverse_update. */
int pdr_reverse_step(float *x, const float *eps, int ld_eps, const float *z, const float *tab_a,
                     const float *tab_b, const float *tab_c, long long *t_dev, const float *ts_table,
                     float *ts_out, unsigned long long *rng_state, int *ticket, long npoints, int mode,
                     int *probe_acc, int *probe_out, pdr_stream_t stream);
/* (probe_acc / probe_out, both NULL or both set: the same last workgroup copies the two probe counters of this step
 * (pdr_dedup_prepare / pdr_dedup_probe) into probe_out -- device-visible pinned host memory, int[16] = a ring of four
 * slots {tiles walked, tiles, step counter t, 1}, slot t & 3 (ABI 101; ABI 100 wrote int[2]) -- and zeroes probe_acc for
 * the next step.  The sampler reads the slot of ONE given step a step or two later to pick the captured step for the
 * next x_t; the tag tells it when that slot has been overwritten, so its choices do not depend on timing.) */
/* out (B, W; ld ldo) = row clamp(*t_dev, 0, T-1) of table (T, W; ld ldt), broadcast to B rows: one reverse step's
 * per-block step-embedding rows fc(t_emb) looked up in a table built once per schedule with pdr_embed_linear over all T
 * step values (the chain depends on t only; same bits as evaluating it per step).  W, ldt, ldo multiples of 4. */
int pdr_embed_select(const float *table, int ldt, int T, const long long *t_dev, int B, int W, float *out, int ldo,
                     pdr_stream_t stream);
/* ---- step embedding chain -------------------------------------------------------
 * out (B,N; ld ldo) = act(bias + in . W^T), W (N,K) row-major as nn.Linear stores it, act 0 = none, 1 = swish
 * (x sigmoid(x)).  in = x (B,K; ld ldx) when ts == NULL, else the sinusoidal step embedding of
 * pointnet2_ssg_sem.py:14-31 computed on the fly: in[b,k] = sin(ts[b] freq[k]) for k < half, cos(ts[b] freq[k-half])
 * after (K == 2 half; ts element stride ts_stride, 0 = one step value for the whole batch).  Replaces calc_t_emb,
 * fc_t1 / fc_t2 + swish (pointnet2_with_pcld_condition.py:183-184) and the per-block fc(t_emb) Linear layers
 * (pointnet2_modules.py:113-120) of one reverse step: three launches.  K % 8 == 0 and 16-byte aligned rows, else
 * PDR_EUNSUPPORTED. */
int pdr_embed_linear(const float *x, int ldx, const float *ts, int ts_stride, const float *freq, int half,
                     const float *W, const float *bias, int B, int K, int N, int act, float *out, int ldo,
                     pdr_stream_t stream);
/* ---- a chain of per-point layers of one block as ONE launch (the fused per-level block kernel, for the
 * per-point halves of the deep levels; csrc/point_chain.hip) -------------------------------------------------------------
 * Replaces, for rows-per-cloud n <= 256, the launch sequence conv -> GroupNorm fold -> conv -> fold -> activation that
 * evaluates Mlp_plus_t_emb (pointnet2_modules.py:69-174) on per-point rows -- PointnetKnnFPModule's mlp2 (:829-839) --
 * or the query conv + first score conv of AttentionModule (attention.py:70-82).
 *   layer l:  y = x_l . Wt + bias                      x_0 = [seg0 | seg1 | seg2] (rows b n + r of plain tensors),
 *             f = relu_pre ? max(y, 0) : y             x_l = the activated main columns of layer l - 1
 *             z = GroupNorm(groups, Cn)(f) (gamma != NULL; the first Cn channels are normalised over the n rows of the
 *                 cloud, the rest pass: MyGroupNorm, pointnet2_modules.py:23-40), relu_post, + add[b, :]
 *   layer 0 with `residual`: its columns [main_cols, Cout) (the residual conv sharing the input) stay raw and are added
 *   to the LAST layer's z (Cout - main_cols == the last layer's width); every other layer has main_cols == Cout.
 *   out (B n, ldo) = z of the last layer.
 * B clouds x G workgroups (G <= 8, B G <= 256: all resident): a workgroup owns ALL n rows of its cloud for a block of
 * output columns that is made of whole GroupNorm groups, so statistics, fold and activation are local to it; the
 * workgroups of a cloud exchange the activated blocks through `scratch` (write-through stores, one counter per cloud in
 * `sync`, one agent-scope acquire per layer boundary) -- no GroupNorm launch, no partial moments, no grid-wide barrier.
 * scratch: >= out[1] floats of pdr_point_chain_plan; sync: >= 2 B + 1 ints, ZEROED ONCE by the caller -- the launch leaves
 * them zero (sync[2 B] != 0 afterwards: a workgroup gave up waiting; never seen, kept so that a fault cannot hang the
 * device).  Supported: n in {16, 32, 64, 128, 256}, every width a multiple of 16 G with column blocks of whole groups,
 * 16-byte aligned pointers (segments, Wt, bias, add, out, and scratch when n_layers > 1), leading dimensions (seg.ld,
 * ldw, add_ld, ldo) multiples of 4; otherwise PDR_EUNSUPPORTED (the caller runs the layers one by one).  A leading
 * dimension below its width, widths that do not chain and NULL out / scratch / sync are PDR_EINVAL.  Exact fp32 MFMA (v_mfma_f32_16x16x4_f32); equals the layer-by-layer evaluation up to fp32 summation order. */
typedef struct {
  const float *ptr;     /* (B n, ld) */
  int C, ld;
} pdr_chain_seg_t;
typedef struct {
  const float *Wt;      /* (Cin, ldw) the conv weight transposed, as pdr_fused_layer */
  const float *bias;    /* (Cout) or NULL */
  int ldw, Cin, Cout, main_cols;
  const float *gamma;   /* (>= Cn) GroupNorm weight, NULL = no GroupNorm behind this layer */
  const float *beta;
  int groups, Cn;
  float eps;
  int relu_pre, relu_post;
  const float *add;     /* (B, add_ld) row added after the activation (fc(t_emb) / fc_condition rows), or NULL */
  int add_ld;
  int reserved_;
} pdr_chain_layer_t;
typedef struct {
  int n_layers, n_seg;
  pdr_chain_seg_t seg[3];
  pdr_chain_layer_t layer[4];
  int residual, ldo;
  float *out;
  float *scratch;
  int *sync;
} pdr_point_chain_t;
/* out[0] = G (workgroups per cloud), out[1] = floats of `scratch`, out[2] = ints of `sync`, out[3] = workgroups of the
 * launch; host logic only (scratch / sync may still be NULL).  Return codes as pdr_point_chain. */
int pdr_point_chain_plan(const pdr_point_chain_t *chain, int B, int n, long *out);
int pdr_point_chain(const pdr_point_chain_t *chain, int B, int n, pdr_stream_t stream);
/* out (B,m,C0+C1) = rows idx (B,m) of the channel-last concatenation [src0 (B,n,C0) | src1 (B,n,C1)] without
 * building it (the `torch.cat([mapped, features], 1)` + gather_operation of pointnet2_with_pcld_condition.py
 * :392-398 and pointnet2_modules.py:243-246 in one launch) */
int pdr_gather_rows2(const float *src0, int C0, const float *src1, int C1, const int *idx, int B, int n, int m,
                     float *out, pdr_stream_t stream);
/* out (rows, ldo) = [src (rows, C) | 0]: channel-last rows padded to a 16-byte multiple (the layer kernels stage
 * rows with 16-byte loads; replaces F.pad's fill + strided copy) */
int pdr_pad_rows(const float *src, long rows, int C, float *out, int ldo, pdr_stream_t stream);
/* measurement aid (no reference counterpart): one thread writes the 100 MHz wall clock to *slot on `stream`;
 * capturable, so a replayed step can carry its own time stamps (tools/lab/step_markers.py) */
int pdr_mark_time(unsigned long long *slot, pdr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDR_HIP_H */
