// chamfer_loss.hip -- the Chamfer distance as a TRAINING LOSS: pdr_chamfer_loss (forward) and pdr_chamfer_loss_grad.
//
// Replaces, for calc_cd(X, refined_X)[loss_idx].mean().backward() (reference pointnet2/train.py:518), the composition
// of two differentiable knn_points(K = 1) searches, (B,n) distance and int64 index tensors, sqrt / mean / sum torch
// launches and two scattered backward calls.  Per cloud pair the forward writes FOUR floats
//     sums[b] = { sum_i d_xy[i], sum_j d_yx[j], sum_i sqrt(d_xy[i]), sum_j sqrt(d_yx[j]) },
//     d_xy[i] = min_j |x_i - y_j|^2   (d_yx the reverse)
// over the valid points -- everything cd_t and cd_p are made of -- and, when a gradient will be asked for, the two
// int32 nearest-neighbour index arrays.  The backward takes d(loss)/d(sums) and writes grad_x and grad_y in ONE launch.
//
// FORWARD.  The search is the packed scan of nn1_scan.h, nn1_kernel's loop (neighbors.hip): a thread owns 2 QP queries as packed fp32 pairs, the candidate
// cloud streams through LDS in 1024-point float4 tiles every lane reads at the same address, the distance is PDR_ACC3
// on the differences, per 8-point chunk only a running minimum is kept and the ONE recorded chunk of a query is
// rescanned in ascending order with a strict `<`: every minimum and index has the bits pdr_chamfer_nn returns (a valid
// query without a finite distance counts 0 and gets index -1, as there).  A workgroup owns 512 QP consecutive queries
// of one (cloud, direction) and writes one (sum d, sum sqrt d) partial into the workspace; a finishing launch (one
// thread per output float) adds the partials.  Two launches, no atomics.
//
// SUMMATION ORDER (fixed by the code, a function of the two LENGTHS only).  Query q of a direction belongs to block
// q / (512 QP) and there to thread t = q % 256; a thread adds the minima of its 2 QP queries to one accumulator in
// ascending order, the 64 accumulators of a wave are summed by an xor butterfly (6 levels), the 4 wave sums as
// (w0 + w1) + (w2 + w3), and the finishing thread adds the block partials one after the other in ascending block order.
// Slots beyond a length add +0.0f, which is exact, so the padded sizes never show: a ragged pair gets the bits of the
// dense call on the two slices, and NULL or full lengths give the bits of the call without lengths.  LONGEST CHAIN of
// dependent fp32 roundings (QP = 2):
//     4 + 6 + 2 + ceil(max(n1, n2) / 1024)   =   28 for n <= 16384   (14 at 2048)
// plus the one rounding of sqrt per addend for sums[2:4].  Every addend is >= 0, so sums[0:2] is within 28 * 2^-24
// relative of the exact sum of the fp32 minima and sums[2:4] within 30 * 2^-24 of the exact sum of their square roots.
//
// BACKWARD.  With (g0, g1, g2, g3) = d(loss)/d(sums[b]) the coefficient on a squared distance is
//     w_xy[i] = g0 + (g2 == 0 ? 0 : g2 * 0.5 / sqrt(d_xy[i])),      w_yx[j] likewise with g1, g3,
// d being recomputed from x, y and the saved index with PDR_ACC3 (the bits the forward saw), and
//     grad_x[b,i] = fl(2 w_xy[i]) (x_i - y_idx_xy[i])  -  sum over j with idx_yx[j] == i, j ascending, of
//                   fl(2 w_yx[j]) (y_j - x_i)
// grad_y is the mirror image.  Every product is rounded before its add; the element starts from the query term (+0.0f
// when that index is outside the opposite cloud) and the scattered terms follow in ascending source order.
//   * g2 == 0 (g3 == 0): the sqrt term is not evaluated, so a cd_t-only loss never meets 0 * inf.
//   * d == 0: the sqrt term contributes exactly 0 -- a subgradient choice, the direction x - y is 0 there.  This
//     DEPARTS from the torch composition, whose sqrt backward gives inf * 0 = NaN for a coincident pair (mirrored
//     condition clouds and x == y make such pairs real).
// The scatter is an INVERSE SCAN: one thread owns a destination point, the opposite direction's index array streams
// through LDS in 1024-entry tiles (every lane reads the same int4: a broadcast), a thread compares the entries with
// its own index and, on a match -- n per cloud in all --, loads that source point and subtracts its term.  n1 n2
// integer compares per cloud and direction, no workspace, no atomics of any kind, each output element written once:
// the ascending order and the reproducible bits fall out of the loop.  Padded rows and rows of a pair with an empty
// side get +0.0f; an index outside [0, n) matches no destination and reaches no memory.
//
// GRID.  Forward: (ceil(max(n1, n2) / (512 QP)), B, 2 directions) workgroups of 256 threads; the compiler reports 72
// VGPRs with index recovery and 58 without, no scratch, 16,416 B of LDS.  Splitting a (cloud, direction) over
// workgroups is what the workspace and the finishing launch pay for: measured forward + backward through calc_cd_fused
// at (B, n1, n2) = (32, 2048, 2048) / (8, 16384, 16384), 0.306 / 1.504 ms against 0.383 / 14.6 ms with one workgroup
// per (cloud, direction) (-DPDR_CDL_ONE_WG=1) and 0.344 / 1.436 ms with QP = 1 (profiles/chamfer_loss.txt).
// Backward: (ceil(max(n1, n2) / 256), B, 2 sides) workgroups, 23 VGPRs, 4 KB of LDS.
//
// SIZES.  Refused with PDR_EUNSUPPORTED: B > 65535 (grid y), B max(n1, n2) >= 2^31 (int32 positions) and
// max(n1, n2) > 2^24 (keeps every query / candidate position and the block count of the finishing loop in int).
#include "nn1_scan.h"

namespace {

using pdr::cloud_len;
using pdr::kTile;              // candidate points per LDS tile (forward) and index entries per LDS tile (backward)
constexpr int kMaxN = 1 << 24;

#ifndef PDR_CDL_QP
#define PDR_CDL_QP 2           // query PAIRS per thread (lab builds: -DPDR_CDL_QP=1)
#endif
#ifndef PDR_CDL_ONE_WG
#define PDR_CDL_ONE_WG 0       // lab builds: 1 = one workgroup per (cloud, direction) walks all its query blocks
#endif

constexpr int kBlockQ = 256 * 2 * PDR_CDL_QP;   // queries per block = per partial sum

// partial sums: (B, 2 directions, nblk blocks, {sum d, sum sqrt d})
__device__ __forceinline__ size_t partial_at(int b, int dir, int nblk, int blk) {
  return ((static_cast<size_t>(b) * 2 + dir) * nblk + blk) * 2;
}

template <int QP, bool WITH_IDX>
__global__ __launch_bounds__(256) void chamfer_loss_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const int64_t* __restrict__ len_x,
                                                           const int64_t* __restrict__ len_y, int n1, int n2,
                                                           int* __restrict__ idx_xy, int* __restrict__ idx_yx,
                                                           float* __restrict__ partial, int nblk) {
  constexpr int NQ = 2 * QP;                       // queries per thread
  constexpr int QPB = 256 * NQ;
  __shared__ float4 tile[kTile];
  __shared__ float wsum[8];
  const int dir = blockIdx.z, b = blockIdx.y;
  const int nq = dir ? n2 : n1, nc = dir ? n1 : n2;
  const float* queries = (dir ? y : x) + static_cast<size_t>(b) * nq * 3;
  const float* c = (dir ? x : y) + static_cast<size_t>(b) * nc * 3;
  int* idx = dir ? idx_yx : idx_xy;
  const int nqe = cloud_len(dir ? len_y : len_x, b, nq);
  const int nce_all = cloud_len(dir ? len_x : len_y, b, nc);
  // the grid covers max(n1, n2); a block beyond this direction's padded size has nothing to write (uniform)
  for (int blk = blockIdx.x; blk * QPB < nq; blk += gridDim.x) {
    const int q0 = blk * QPB + threadIdx.x;        // thread t owns queries q0 + 256 i (coalesced loads / stores)
    const int nce = blk * QPB < nqe ? nce_all : 0; // a block of padded queries scans nothing
    // slots beyond the length shadow the last valid query (row 0 of an empty cloud; its value is never used)
    pdr::Nn1State<QP> st;
    pdr::nn1_load(st, queries, q0, nqe - 1);
    pdr::nn1_scan<QP, WITH_IDX>(st, c, nce, tile);
    float acc[2] = {0.0f, 0.0f};                                 // sum d, sum sqrt d
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const int j = q0 + 256 * s;
      // a valid query with a finite minimum; anything else adds +0.0f (exact).  Ascending query order.
      const bool valid = j < nqe && st.best[s >> 1][s & 1] < __builtin_inff();
      const float d = valid ? st.best[s >> 1][s & 1] : 0.0f;
      acc[0] += d;
      acc[1] += __builtin_sqrtf(d);
      if (WITH_IDX && j < nq)                                    // -1: padded query / empty opposite cloud
        idx[static_cast<size_t>(b) * nq + j] = valid ? pdr::nn1_recover(st, s, c, nce).i : -1;
    }
    pdr::block_sum_256(acc, wsum);
    if (threadIdx.x == 0) {
      float* out = partial + partial_at(b, dir, nblk, blk);
      out[0] = acc[0];
      out[1] = acc[1];
    }
  }
}

// one thread per output float: sums[b][k], k = direction + 2 * (sqrt ? 1 : 0); block partials added in ascending order
__global__ __launch_bounds__(256) void chamfer_loss_finish(const float* __restrict__ partial,
                                                           const int64_t* __restrict__ len_x,
                                                           const int64_t* __restrict__ len_y, int B, int n1, int n2,
                                                           int nblk, int block_q, float* __restrict__ sums) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= B * 4) return;
  const int b = o >> 2, dir = o & 1, comp = (o >> 1) & 1;
  const int lx = cloud_len(len_x, b, n1), ly = cloud_len(len_y, b, n2);
  const int nqe = dir ? ly : lx;
  const int nb = (lx > 0 && ly > 0) ? (nqe + block_q - 1) / block_q : 0;   // a pair with an empty side: +0.0f
  const float* p = partial + partial_at(b, dir, nblk, 0) + comp;
  float s = 0.0f;
  for (int k = 0; k < nb; ++k) s += p[2 * k];
  sums[o] = s;
}

// coefficient of a squared distance d: g_sq + g_sqrt * 0.5 / sqrt(d); the sqrt term is skipped for a zero coefficient
// and contributes 0 at d == 0.  Returned doubled (exact).
__device__ __forceinline__ float loss_coef2(float g_sq, float g_sqrt, float d) {
  float term = 0.0f;
  if (g_sqrt != 0.0f && d != 0.0f) term = (g_sqrt * 0.5f) / __builtin_sqrtf(d);
  return 2.0f * (g_sq + term);
}

__global__ __launch_bounds__(256) void chamfer_loss_grad_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ y,
                                                                const int64_t* __restrict__ len_x,
                                                                const int64_t* __restrict__ len_y,
                                                                const int* __restrict__ idx_xy,
                                                                const int* __restrict__ idx_yx,
                                                                const float* __restrict__ grad_sums, int n1, int n2,
                                                                float* __restrict__ grad_x,
                                                                float* __restrict__ grad_y) {
  __shared__ int4 itile[kTile / 4];
  // side 0 writes grad_x: destinations are x points, sources are y points (those whose idx_yx names the destination)
  const int side = blockIdx.z, b = blockIdx.y;
  const int nd = side ? n2 : n1, ns = side ? n1 : n2;
  if (static_cast<int>(blockIdx.x) * 256 >= nd) return;          // uniform: the grid covers max(n1, n2)
  const float* dst = (side ? y : x) + static_cast<size_t>(b) * nd * 3;
  const float* src = (side ? x : y) + static_cast<size_t>(b) * ns * 3;
  const int* idx_own = (side ? idx_yx : idx_xy) + static_cast<size_t>(b) * nd;   // destination -> its nearest source
  const int* idx_src = (side ? idx_xy : idx_yx) + static_cast<size_t>(b) * ns;   // source -> its nearest destination
  float* grad = (side ? grad_y : grad_x) + static_cast<size_t>(b) * nd * 3;
  const int lx = cloud_len(len_x, b, n1), ly = cloud_len(len_y, b, n2);
  const int nde = (lx > 0 && ly > 0) ? (side ? ly : lx) : 0;     // a pair with an empty side: every row +0.0f
  const int nse = side ? lx : ly;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < nde;
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  if (static_cast<int>(blockIdx.x) * 256 < nde) {                // uniform: a block of padded rows scans nothing
    const float* g = grad_sums + static_cast<size_t>(b) * 4;
    const float g_own = g[side], g_own_sqrt = g[2 + side];       // coefficients of this side's own queries
    const float g_src = g[1 - side], g_src_sqrt = g[3 - side];   // ... and of the opposite direction's
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
      px = dst[static_cast<size_t>(i) * 3 + 0];
      py = dst[static_cast<size_t>(i) * 3 + 1];
      pz = dst[static_cast<size_t>(i) * 3 + 2];
      const int j = idx_own[i];
      if (j >= 0 && j < nse) {                                   // query term; otherwise the element starts from +0.0f
        const float* s = src + static_cast<size_t>(j) * 3;
        const float dx = px - s[0], dy = py - s[1], dz = pz - s[2];
        const float w2 = loss_coef2(g_own, g_own_sqrt, PDR_ACC3(dx, dy, dz));
        gx = w2 * dx;
        gy = w2 * dy;
        gz = w2 * dz;
      }
    }
    const int me = live ? i : -2;                                // -2 matches no entry (padding entries are -1)
    for (int k0 = 0; k0 < nse; k0 += kTile) {
      const int kn = (nse - k0) < kTile ? (nse - k0) : kTile;
      const int kpad = (kn + 3) & ~3;
      __syncthreads();
      int* flat = reinterpret_cast<int*>(itile);
      for (int t = threadIdx.x; t < kpad; t += 256) flat[t] = t < kn ? idx_src[k0 + t] : -1;
      __syncthreads();
      for (int t0 = 0; t0 < kpad; t0 += 4) {
        const int4 e = itile[t0 >> 2];                           // every lane reads the same address: one broadcast
        if ((e.x == me) | (e.y == me) | (e.z == me) | (e.w == me)) {
          const int ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {                          // ascending source order
            if (ev[u] == me) {
              const float* s = src + static_cast<size_t>(k0 + t0 + u) * 3;
              const float dx = s[0] - px, dy = s[1] - py, dz = s[2] - pz;
              const float w2 = loss_coef2(g_src, g_src_sqrt, PDR_ACC3(dx, dy, dz));
              gx -= w2 * dx;
              gy -= w2 * dy;
              gz -= w2 * dz;
            }
          }
        }
      }
    }
  }
  if (i < nd) {
    grad[static_cast<size_t>(i) * 3 + 0] = live ? gx : 0.0f;
    grad[static_cast<size_t>(i) * 3 + 1] = live ? gy : 0.0f;
    grad[static_cast<size_t>(i) * 3 + 2] = live ? gz : 0.0f;
  }
}

// the size checks both calls share, in the order the header states them
int check_sizes(int B, int n1, int n2) {
  if (B < 0 || n1 < 0 || n2 < 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  if (n1 <= 0 || n2 <= 0) return PDR_EINVAL;
  const int nmax = n1 > n2 ? n1 : n2;
  if (B > 65535 || nmax > kMaxN || static_cast<long long>(B) * nmax >= (1ll << 31)) return PDR_EUNSUPPORTED;
  return PDR_OK;
}

int blocks_per_direction(int n1, int n2) { return ((n1 > n2 ? n1 : n2) + kBlockQ - 1) / kBlockQ; }

}  // namespace

extern "C" size_t pdr_chamfer_loss_workspace_bytes(int B, int n1, int n2) {
  if (B <= 0 || check_sizes(B, n1, n2) != PDR_OK) return 0;
  return static_cast<size_t>(B) * 2 * blocks_per_direction(n1, n2) * 2 * sizeof(float);
}

extern "C" int pdr_chamfer_loss(const float* x, const float* y, const int64_t* lengths1, const int64_t* lengths2, int B,
                                int n1, int n2, float* sums, int* idx_xy, int* idx_yx, void* workspace,
                                pdr_stream_t stream) {
  const int rc = check_sizes(B, n1, n2);
  if (rc != PDR_OK || B == 0) return rc;
  if (!x || !y || !sums) return PDR_EINVAL;
  if ((idx_xy == nullptr) != (idx_yx == nullptr)) return PDR_EINVAL;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3)) return PDR_EINVAL;
  float* partial = static_cast<float*>(workspace);
  const int nblk = blocks_per_direction(n1, n2);
  const dim3 grid(PDR_CDL_ONE_WG ? 1 : nblk, B, 2);
  hipStream_t s = pdr::as_stream(stream);
  if (idx_xy)
    hipLaunchKernelGGL((chamfer_loss_kernel<PDR_CDL_QP, true>), grid, dim3(256), 0, s, x, y, lengths1, lengths2, n1, n2,
                       idx_xy, idx_yx, partial, nblk);
  else
    hipLaunchKernelGGL((chamfer_loss_kernel<PDR_CDL_QP, false>), grid, dim3(256), 0, s, x, y, lengths1, lengths2, n1,
                       n2, idx_xy, idx_yx, partial, nblk);
  int lrc = pdr::check_launch();
  if (lrc != PDR_OK) return lrc;
  hipLaunchKernelGGL(chamfer_loss_finish, dim3(pdr::blocks_for(static_cast<long>(B) * 4)), dim3(256), 0, s, partial,
                     lengths1, lengths2, B, n1, n2, nblk, kBlockQ, sums);
  return pdr::check_launch();
}

extern "C" int pdr_chamfer_loss_grad(const float* x, const float* y, const int64_t* lengths1, const int64_t* lengths2,
                                     const int* idx_xy, const int* idx_yx, const float* grad_sums, int B, int n1,
                                     int n2, float* grad_x, float* grad_y, pdr_stream_t stream) {
  const int rc = check_sizes(B, n1, n2);
  if (rc != PDR_OK || B == 0) return rc;
  if (!x || !y || !idx_xy || !idx_yx || !grad_sums || !grad_x || !grad_y) return PDR_EINVAL;
  const int nmax = n1 > n2 ? n1 : n2;
  hipLaunchKernelGGL(chamfer_loss_grad_kernel, dim3((nmax + 255) / 256, B, 2), dim3(256), 0, pdr::as_stream(stream), x,
                     y, lengths1, lengths2, idx_xy, idx_yx, grad_sums, n1, n2, grad_x, grad_y);
  return pdr::check_launch();
}
