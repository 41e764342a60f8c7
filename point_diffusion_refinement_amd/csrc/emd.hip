// emd.hip -- approximate earth mover's distance (auction-style soft matching).
//
// Replaces approxmatch / matchcost / matchcostgrad{1,2} (reference
// PytorchEMD/cuda/emd_kernel.cu:29-161, 204-246, 290-359).  The reference runs
// 32 blocks x 512 threads (one block per cloud pair, all 10 temperature levels in
// one launch, __syncthreads between passes) and read-modify-writes the 4*n*m-byte
// match matrix once per level (~350 MB of HBM traffic per 2048^2 pair).
//
// MI355X design:
//  * every pass of every level is its own launch over grid (ceil(n/256), B), so a
//    batch of 32 pairs fills all 256 CUs instead of 32; the kernel boundary is the
//    inter-pass barrier.
//  * the per-level factors ratioL[level][k], ratioR[level][l] are KEPT
//    (10 x (n+m) floats per pair) -- match is the closed form
//        match[l,k] = sum_level exp(level*d2(k,l)) * ratioL[level][k] * ratioR[level][l]
//    so the materialising API writes the matrix exactly ONCE (level order and
//    operation order identical to the reference's `match += w`), and the cost-only
//    path (pdr_emd_cost) never touches a matrix at all: 49 KB of traffic per pair
//    instead of 350 MB.
//  * the gradient needs no matrix either (pdr_emd_cost_grad, emd_cost_grad_kernel): the factors are still in the
//    workspace when the forward returns, and each thread re-evaluates its row / column of match from them.
//  * the opposite cloud streams through LDS as float4 {x,y,z,weight}; all lanes
//    read the same address (broadcast).  Per-thread accumulation order over the
//    opposite cloud is sequential, as in the reference, so the only numeric
//    difference to the oracle is __expf (v_exp_f32) vs expf.
//
// Per-cloud lengths (pdr_*_ragged): every kernel is ONE body with a RAGGED switch; the dense entry points instantiate
// it off and pass no lengths, so they run the code they always ran.  Switched on, cloud b is the pair
// xyz1[b, :ne], xyz2[b, :me] (pair_len: read on the device, clamped, an empty side empties the pair); n and m stay the
// row strides and the grid sizes.  A thread whose own row is padding keeps walking the tile loops' barriers and does
// not write; a workgroup whose rows are ALL padding gets a loop bound of 0 (uniform over the workgroup).  The loops over
// the opposite cloud run to me / ne from index 0 in the same tiles, so the valid region is computed by the dense
// operation sequence on the slices, and nothing beyond a length is ever loaded -- points, workspace or match.
#include "pdr_common.h"

namespace {

constexpr int kLevels = 10;
constexpr int kTile = 1024;

__host__ __device__ inline float level_value(int li) {
  // emd_kernel.cu:49-53: level = -4^j for j = 7..-1, then 0 for j = -2
  const int j = 7 - li;
  if (j == -2) return 0.0f;
  float v = 1.0f;
  if (j >= 0) for (int t = 0; t < j; ++t) v *= 4.0f;
  else for (int t = 0; t < -j; ++t) v *= 0.25f;
  return -v;
}

// workspace layout per batch element (floats):
//   remainL[n] remainR[m] ratioL[kLevels][n] ratioR[kLevels][m] costpart[n]
__host__ __device__ inline size_t ws_floats(int n, int m) {
  return static_cast<size_t>(n) * (2 + kLevels) + static_cast<size_t>(m) * (1 + kLevels);
}
struct Ws {
  float *remainL, *remainR, *ratioL, *ratioR, *costpart;
};
__device__ inline Ws ws_of(float* temp, int b, int n, int m) {
  float* base = temp + static_cast<size_t>(b) * ws_floats(n, m);
  Ws w;
  w.remainL = base;
  w.remainR = base + n;
  w.ratioL = w.remainR + m;
  w.ratioR = w.ratioL + static_cast<size_t>(kLevels) * n;
  w.costpart = w.ratioR + static_cast<size_t>(kLevels) * m;
  return w;
}

// Valid sizes of pair b: (n, m) without RAGGED; else lengths1[b] / lengths2[b] clamped to [0, n] / [0, m] (NULL = full),
// and (0, 0) when either is 0 -- an empty pair has no candidates, no rows and nothing to divide.
struct PairLen {
  int n, m;
};
template <bool RAGGED>
__device__ __forceinline__ PairLen pair_len(const int64_t* __restrict__ len1,
                                            const int64_t* __restrict__ len2, int b, int n, int m) {
  PairLen p{n, m};
  if (RAGGED) {
    p.n = pdr::cloud_len(len1, b, n);
    p.m = pdr::cloud_len(len2, b, m);
    if (p.n == 0 || p.m == 0) p.n = p.m = 0;
  }
  return p;
}

// RAGGED: multiL / multiR are the pair's own (emd_kernel.cu:31-38 on (ne, me), same integer division)
template <bool RAGGED>
__global__ __launch_bounds__(256) void emd_init_kernel(float* temp, int n, int m, float multiL,
                                                       float multiR,
                                                       const int64_t* __restrict__ len1 = nullptr,
                                                       const int64_t* __restrict__ len2 = nullptr) {
  const Ws w = ws_of(temp, blockIdx.y, n, m);
  const PairLen len = pair_len<RAGGED>(len1, len2, blockIdx.y, n, m);
  const int ne = len.n, me = len.m;
  if (RAGGED && ne > 0) {   // (ne > 0 implies me > 0)
    if (ne >= me) { multiL = 1.0f; multiR = static_cast<float>(ne / me); }
    else          { multiL = static_cast<float>(me / ne); multiR = 1.0f; }
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < ne) {
    w.remainL[i] = multiL;
    w.costpart[i] = 0.0f;
  }
  if (i < me) w.remainR[i] = multiR;
}

// pass 1 (emd_kernel.cu:55-88): ratioL[k] = remainL[k] / (1e-9 + sum_l exp(level d) remainR[l])
template <bool RAGGED>
__global__ __launch_bounds__(256) void emd_pass1_kernel(const float* __restrict__ xyz1,
                                                        const float* __restrict__ xyz2,
                                                        float* temp, int n, int m, int li,
                                                        const int64_t* __restrict__ len1 = nullptr,
                                                        const int64_t* __restrict__ len2 = nullptr) {
  __shared__ float4 tile[kTile];
  const int b = blockIdx.y;
  const Ws w = ws_of(temp, b, n, m);
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int ne = len.n;
  const int me = RAGGED && static_cast<int>(blockIdx.x) * 256 >= ne ? 0 : len.m;
  const float level = level_value(li);
  const int k = blockIdx.x * 256 + threadIdx.x;
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  float x1 = 0, y1 = 0, z1 = 0;
  if (k < ne) { x1 = p1[k * 3]; y1 = p1[k * 3 + 1]; z1 = p1[k * 3 + 2]; }
  float suml = 1e-9f;
  for (int l0 = 0; l0 < me; l0 += kTile) {
    const int lend = (me - l0) < kTile ? (me - l0) : kTile;
    __syncthreads();
    for (int l = threadIdx.x; l < lend; l += 256)
      tile[l] = make_float4(p2[(l0 + l) * 3], p2[(l0 + l) * 3 + 1], p2[(l0 + l) * 3 + 2],
                            w.remainR[l0 + l]);
    __syncthreads();
    for (int l = 0; l < lend; ++l) {
      const float4 t = tile[l];
      const float dx = t.x - x1, dy = t.y - y1, dz = t.z - z1;
      const float d = level * PDR_SUM3(dx, dy, dz);
      suml = __builtin_fmaf(__expf(d), t.w, suml);   // single-use product: contracted (model N1)
    }
  }
  if (k < ne) w.ratioL[static_cast<size_t>(li) * n + k] = w.remainL[k] / suml;
}

// pass 2 (emd_kernel.cu:90-122)
template <bool RAGGED>
__global__ __launch_bounds__(256) void emd_pass2_kernel(const float* __restrict__ xyz1,
                                                        const float* __restrict__ xyz2,
                                                        float* temp, int n, int m, int li,
                                                        const int64_t* __restrict__ len1 = nullptr,
                                                        const int64_t* __restrict__ len2 = nullptr) {
  __shared__ float4 tile[kTile];
  const int b = blockIdx.y;
  const Ws w = ws_of(temp, b, n, m);
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int me = len.m;
  const int ne = RAGGED && static_cast<int>(blockIdx.x) * 256 >= me ? 0 : len.n;
  const float level = level_value(li);
  const float* ratioL = w.ratioL + static_cast<size_t>(li) * n;
  const int l = blockIdx.x * 256 + threadIdx.x;
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  float x2 = 0, y2 = 0, z2 = 0;
  if (l < me) { x2 = p2[l * 3]; y2 = p2[l * 3 + 1]; z2 = p2[l * 3 + 2]; }
  float sumr = 0;
  for (int k0 = 0; k0 < ne; k0 += kTile) {
    const int kend = (ne - k0) < kTile ? (ne - k0) : kTile;
    __syncthreads();
    for (int k = threadIdx.x; k < kend; k += 256)
      tile[k] = make_float4(p1[(k0 + k) * 3], p1[(k0 + k) * 3 + 1], p1[(k0 + k) * 3 + 2],
                            ratioL[k0 + k]);
    __syncthreads();
    for (int k = 0; k < kend; ++k) {
      const float4 t = tile[k];
      const float dx = x2 - t.x, dy = y2 - t.y, dz = z2 - t.z;
      sumr = __builtin_fmaf(__expf(level * PDR_SUM3(dx, dy, dz)), t.w, sumr);   // model N1
    }
  }
  if (l < me) {
    const float rr = w.remainR[l];
    sumr *= rr;
    const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
    w.ratioR[static_cast<size_t>(li) * m + l] = consumption * rr;
    w.remainR[l] = fmaxf(0.0f, rr - sumr);
  }
}

// pass 3 (emd_kernel.cu:124-157) without the match RMW; accumulates
// costpart[k] += sum_l d2 * w  (what matchcost :226-231 would add for this level)
template <bool RAGGED>
__global__ __launch_bounds__(256) void emd_pass3_kernel(const float* __restrict__ xyz1,
                                                        const float* __restrict__ xyz2,
                                                        float* temp, int n, int m, int li,
                                                        const int64_t* __restrict__ len1 = nullptr,
                                                        const int64_t* __restrict__ len2 = nullptr) {
  __shared__ float4 tile[kTile];
  const int b = blockIdx.y;
  const Ws w = ws_of(temp, b, n, m);
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int ne = len.n;
  const int me = RAGGED && static_cast<int>(blockIdx.x) * 256 >= ne ? 0 : len.m;
  const float level = level_value(li);
  const float* ratioR = w.ratioR + static_cast<size_t>(li) * m;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  float x1 = 0, y1 = 0, z1 = 0, rl = 0;
  if (k < ne) {
    x1 = p1[k * 3]; y1 = p1[k * 3 + 1]; z1 = p1[k * 3 + 2];
    rl = w.ratioL[static_cast<size_t>(li) * n + k];
  }
  float suml = 0, cost = 0;
  for (int l0 = 0; l0 < me; l0 += kTile) {
    const int lend = (me - l0) < kTile ? (me - l0) : kTile;
    __syncthreads();
    for (int l = threadIdx.x; l < lend; l += 256)
      tile[l] = make_float4(p2[(l0 + l) * 3], p2[(l0 + l) * 3 + 1], p2[(l0 + l) * 3 + 2],
                            ratioR[l0 + l]);
    __syncthreads();
    for (int l = 0; l < lend; ++l) {
      const float4 t = tile[l];
      const float dx = t.x - x1, dy = t.y - y1, dz = t.z - z1;
      const float d2 = PDR_SUM3(dx, dy, dz);
      const float wgt = __expf(level * d2) * rl * t.w;
      suml += wgt;
      cost = __builtin_fmaf(d2, wgt, cost);
    }
  }
  if (k < ne) {
    w.remainL[k] = fmaxf(0.0f, w.remainL[k] - suml);
    w.costpart[k] += cost;
  }
}

// match[b,l,k] = sum_level exp(level d2) * ratioL[level][k] * ratioR[level][l]
// thread <-> k (coalesced rows of match), block handles 16 rows l.
// RAGGED: the grid still covers the padded (m, n) matrix; entries with l >= me or k >= ne are written as 0.
template <bool RAGGED>
__global__ __launch_bounds__(256) void emd_match_kernel(const float* __restrict__ xyz1,
                                                        const float* __restrict__ xyz2,
                                                        float* temp, int n, int m,
                                                        float* __restrict__ match,
                                                        const int64_t* __restrict__ len1 = nullptr,
                                                        const int64_t* __restrict__ len2 = nullptr) {
  constexpr int ROWS = 16;
  __shared__ float4 rows[ROWS];
  __shared__ float rr[ROWS][kLevels];
  const int b = blockIdx.z;
  const Ws w = ws_of(temp, b, n, m);
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int ne = len.n, me = len.m;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int l0 = blockIdx.y * ROWS;
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  if (threadIdx.x < ROWS) {
    const int l = l0 + threadIdx.x;
    rows[threadIdx.x] = l < me ? make_float4(p2[l * 3], p2[l * 3 + 1], p2[l * 3 + 2], 0.0f)
                               : make_float4(0, 0, 0, 0);
  }
  if (threadIdx.x < ROWS * kLevels) {
    const int r = threadIdx.x / kLevels, li = threadIdx.x % kLevels;
    rr[r][li] = (l0 + r) < me ? w.ratioR[static_cast<size_t>(li) * m + l0 + r] : 0.0f;
  }
  __syncthreads();
  if (k >= n) return;
  float* mt = match + static_cast<size_t>(b) * n * m;
  if (RAGGED) {   // past the only barrier: rows of the padding, and this thread's whole column when it is padding
    for (int r = k < ne ? (me > l0 ? me - l0 : 0) : 0; r < ROWS && l0 + r < m; ++r)
      mt[static_cast<size_t>(l0 + r) * n + k] = 0.0f;
    if (k >= ne) return;
  }
  const float x1 = p1[k * 3], y1 = p1[k * 3 + 1], z1 = p1[k * 3 + 2];
  float rl[kLevels];
#pragma unroll
  for (int li = 0; li < kLevels; ++li) rl[li] = w.ratioL[static_cast<size_t>(li) * n + k];
  for (int r = 0; r < ROWS && l0 + r < me; ++r) {
    const float4 t = rows[r];
    const float dx = t.x - x1, dy = t.y - y1, dz = t.z - z1;
    const float d2 = PDR_SUM3(dx, dy, dz);
    float acc = 0.0f;
#pragma unroll
    for (int li = 0; li < kLevels; ++li)
      acc += __expf(level_value(li) * d2) * rl[li] * rr[r][li];
    mt[static_cast<size_t>(l0 + r) * n + k] = acc;
  }
}

// cost[b] = sum_k costpart[k]  (deterministic tree)
// RAGGED: over the ne valid rows; thread t adds rows t, t + 256, ... whatever the padded n is
template <bool RAGGED>
__global__ __launch_bounds__(256) void emd_cost_reduce_kernel(float* temp, int n, int m,
                                                              float* __restrict__ cost,
                                                              const int64_t* __restrict__ len1 = nullptr,
                                                              const int64_t* __restrict__ len2 = nullptr) {
  __shared__ float part[4];
  const int b = blockIdx.x;
  const Ws w = ws_of(temp, b, n, m);
  const int ne = pair_len<RAGGED>(len1, len2, b, n, m).n;
  float s = 0;
  for (int k = threadIdx.x; k < ne; k += 256) s += w.costpart[k];
  s = pdr::wave_sum_f32(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) cost[b] = (part[0] + part[1]) + (part[2] + part[3]);
}

// matchcost with a given match (emd_kernel.cu:204-246): block per (b, 256-wide k slab)
// RAGGED: a slab of padding writes the partial +0, which sum_partials_kernel adds without changing a bit
template <bool RAGGED>
__global__ __launch_bounds__(256) void matchcost_kernel(const float* __restrict__ xyz1,
                                                        const float* __restrict__ xyz2,
                                                        const float* __restrict__ match, int n,
                                                        int m, float* __restrict__ partial,
                                                        const int64_t* __restrict__ len1 = nullptr,
                                                        const int64_t* __restrict__ len2 = nullptr) {
  __shared__ float4 tile[kTile];
  __shared__ float part[4];
  const int b = blockIdx.y;
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int ne = len.n;
  const int me = RAGGED && static_cast<int>(blockIdx.x) * 256 >= ne ? 0 : len.m;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  const float* mt = match + static_cast<size_t>(b) * n * m;
  float x1 = 0, y1 = 0, z1 = 0;
  if (k < ne) { x1 = p1[k * 3]; y1 = p1[k * 3 + 1]; z1 = p1[k * 3 + 2]; }
  float subsum = 0;
  for (int l0 = 0; l0 < me; l0 += kTile) {
    const int lend = (me - l0) < kTile ? (me - l0) : kTile;
    __syncthreads();
    for (int l = threadIdx.x; l < lend; l += 256)
      tile[l] = make_float4(p2[(l0 + l) * 3], p2[(l0 + l) * 3 + 1], p2[(l0 + l) * 3 + 2], 0.0f);
    __syncthreads();
    if (k < ne) {
      for (int l = 0; l < lend; ++l) {
        const float4 t = tile[l];
        const float dx = t.x - x1, dy = t.y - y1, dz = t.z - z1;
        subsum = __builtin_fmaf(PDR_SUM3(dx, dy, dz), mt[static_cast<size_t>(l0 + l) * n + k],
                                subsum);
      }
    }
  }
  subsum = pdr::wave_sum_f32(subsum);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = subsum;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[static_cast<size_t>(b) * gridDim.x + blockIdx.x] =
        (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void sum_partials_kernel(const float* __restrict__ partial, int nblk,
                                    float* __restrict__ cost) {
  const int b = blockIdx.x;
  float s = 0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += partial[static_cast<size_t>(b) * nblk + i];
  s = pdr::wave_sum_f32(s);
  if (threadIdx.x == 0) cost[b] = s;
}

// matchcostgrad1 (emd_kernel.cu:337-359): thread per xyz1 point, loop over xyz2
// RAGGED: rows of the padding get exactly 0 (no barrier in this kernel: they leave at once)
template <bool RAGGED>
__global__ __launch_bounds__(256) void matchcost_grad1_kernel(
    const float* __restrict__ grad_cost, const float* __restrict__ xyz1,
    const float* __restrict__ xyz2, const float* __restrict__ match, int n, int m,
    float* __restrict__ grad1, const int64_t* __restrict__ len1 = nullptr,
    const int64_t* __restrict__ len2 = nullptr) {
  const int b = blockIdx.y;
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n) return;
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int me = len.m;
  if (RAGGED && l >= len.n) {
    float* z = grad1 + (static_cast<size_t>(b) * n + l) * 3;
    z[0] = 0.0f; z[1] = 0.0f; z[2] = 0.0f;
    return;
  }
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  const float* mt = match + static_cast<size_t>(b) * n * m;
  const float x1 = p1[l * 3], y1 = p1[l * 3 + 1], z1 = p1[l * 3 + 2];
  float dx = 0, dy = 0, dz = 0;
  for (int k = 0; k < me; ++k) {
    const float d = mt[static_cast<size_t>(k) * n + l] * 2;
    dx += (x1 - p2[k * 3 + 0]) * d;
    dy += (y1 - p2[k * 3 + 1]) * d;
    dz += (z1 - p2[k * 3 + 2]) * d;
  }
  const float g = grad_cost[b];
  float* o = grad1 + (static_cast<size_t>(b) * n + l) * 3;
  o[0] = dx * g; o[1] = dy * g; o[2] = dz * g;
}

// matchcostgrad2 (emd_kernel.cu:290-331): wave per xyz2 point, lanes stride over xyz1
template <bool RAGGED>
__global__ __launch_bounds__(256) void matchcost_grad2_kernel(
    const float* __restrict__ grad_cost, const float* __restrict__ xyz1,
    const float* __restrict__ xyz2, const float* __restrict__ match, int n, int m,
    float* __restrict__ grad2, const int64_t* __restrict__ len1 = nullptr,
    const int64_t* __restrict__ len2 = nullptr) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= m) return;
  const int lane = threadIdx.x & 63;
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int ne = len.n;
  if (RAGGED && k >= len.m) {   // (k is the wave's: the whole wave leaves)
    if (lane < 3) grad2[(static_cast<size_t>(b) * m + k) * 3 + lane] = 0.0f;
    return;
  }
  const float* p1 = xyz1 + static_cast<size_t>(b) * n * 3;
  const float* p2 = xyz2 + static_cast<size_t>(b) * m * 3;
  const float* mt = match + (static_cast<size_t>(b) * m + k) * n;
  const float x2 = p2[k * 3], y2 = p2[k * 3 + 1], z2 = p2[k * 3 + 2];
  float sx = 0, sy = 0, sz = 0;
  for (int j = lane; j < ne; j += 64) {
    const float d = mt[j] * 2;
    sx += (x2 - p1[j * 3 + 0]) * d;
    sy += (y2 - p1[j * 3 + 1]) * d;
    sz += (z2 - p1[j * 3 + 2]) * d;
  }
  sx = pdr::wave_sum_f32(sx);
  sy = pdr::wave_sum_f32(sy);
  sz = pdr::wave_sum_f32(sz);
  if (lane == 0) {
    const float g = grad_cost[b];
    float* o = grad2 + (static_cast<size_t>(b) * m + k) * 3;
    o[0] = sx * g; o[1] = sy * g; o[2] = sz * g;
  }
}

// Matrix-free matchcostgrad (pdr_emd_cost_grad): the two kernels above with match[l,k] evaluated on the fly from the
// factors run_levels left in the workspace, by emd_match_kernel's expression (dx = xyz2 - xyz1, PDR_SUM3, __expf,
// levels 0..9 in order, (exp * ratioL) * ratioR), so a pair contributes the value the matrix would have held.
// SIDE 0: thread <-> xyz1 point k, xyz2 streamed (grad1); SIDE 1: thread <-> xyz2 point l, xyz1 streamed (grad2).
// The own point's ten factors sit in registers; the opposite cloud streams through LDS in tiles of kGradTile points,
// 64 bytes each {x,y,z,-}{f0..f3}{f4..f7}{f8,f9,-,-}, all lanes on one address.  Accumulation over the opposite index
// is sequential from 0 and nothing is atomic: the result is a function of the input alone.  SIDE 0 is
// matchcost_grad1_kernel's operation sequence; SIDE 1 sums in index order where matchcost_grad2_kernel sums by lanes.
// RAGGED: as in the passes -- a padded own row walks the barriers and writes 0; a workgroup of padding loops 0 times;
// the tile is filled below the opposite length only, coordinates and factors alike.
constexpr int kGradTile = 256;
template <bool RAGGED, int SIDE>
__global__ __launch_bounds__(256) void emd_cost_grad_kernel(const float* __restrict__ grad_cost,
                                                            const float* __restrict__ xyz1,
                                                            const float* __restrict__ xyz2,
                                                            const float* __restrict__ temp, int n, int m,
                                                            float* __restrict__ grad,
                                                            const int64_t* __restrict__ len1 = nullptr,
                                                            const int64_t* __restrict__ len2 = nullptr) {
  __shared__ float4 tile[kGradTile][4];
  const int b = blockIdx.y;
  const Ws w = ws_of(const_cast<float*>(temp), b, n, m);   // (read only)
  const PairLen len = pair_len<RAGGED>(len1, len2, b, n, m);
  const int nown = SIDE == 0 ? n : m, nopp = SIDE == 0 ? m : n;   // padded sizes = row strides
  const int eown = SIDE == 0 ? len.n : len.m;
  const int eopp = RAGGED && static_cast<int>(blockIdx.x) * 256 >= eown ? 0 : (SIDE == 0 ? len.m : len.n);
  const float* pown = (SIDE == 0 ? xyz1 : xyz2) + static_cast<size_t>(b) * nown * 3;
  const float* popp = (SIDE == 0 ? xyz2 : xyz1) + static_cast<size_t>(b) * nopp * 3;
  const float* fown = SIDE == 0 ? w.ratioL : w.ratioR;
  const float* fopp = SIDE == 0 ? w.ratioR : w.ratioL;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < eown;
  float xo = 0, yo = 0, zo = 0, fo[kLevels];
#pragma unroll
  for (int li = 0; li < kLevels; ++li) fo[li] = 0.0f;
  if (valid) {
    xo = pown[i * 3]; yo = pown[i * 3 + 1]; zo = pown[i * 3 + 2];
#pragma unroll
    for (int li = 0; li < kLevels; ++li) fo[li] = fown[static_cast<size_t>(li) * nown + i];
  }
  float gx = 0, gy = 0, gz = 0;
  for (int j0 = 0; j0 < eopp; j0 += kGradTile) {
    const int jend = (eopp - j0) < kGradTile ? (eopp - j0) : kGradTile;
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < jend) {
      const int j = j0 + threadIdx.x;
      float f[kLevels];
#pragma unroll
      for (int li = 0; li < kLevels; ++li) f[li] = fopp[static_cast<size_t>(li) * nopp + j];
      tile[threadIdx.x][0] = make_float4(popp[j * 3], popp[j * 3 + 1], popp[j * 3 + 2], 0.0f);
      tile[threadIdx.x][1] = make_float4(f[0], f[1], f[2], f[3]);
      tile[threadIdx.x][2] = make_float4(f[4], f[5], f[6], f[7]);
      tile[threadIdx.x][3] = make_float4(f[8], f[9], 0.0f, 0.0f);
    }
    __syncthreads();
    if (valid) {
      for (int j = 0; j < jend; ++j) {
        const float4 t = tile[j][0], a = tile[j][1], c = tile[j][2], e = tile[j][3];
        const float ft[kLevels] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, e.x, e.y};
        // xyz2 - xyz1 on both sides, as emd_match_kernel forms it
        const float dx = SIDE == 0 ? t.x - xo : xo - t.x;
        const float dy = SIDE == 0 ? t.y - yo : yo - t.y;
        const float dz = SIDE == 0 ? t.z - zo : zo - t.z;
        const float d2 = PDR_SUM3(dx, dy, dz);
        float acc = 0.0f;
#pragma unroll
        for (int li = 0; li < kLevels; ++li) {
          const float rl = SIDE == 0 ? fo[li] : ft[li], rr = SIDE == 0 ? ft[li] : fo[li];
          acc += __expf(level_value(li) * d2) * rl * rr;
        }
        const float d = acc * 2;
        gx += (xo - t.x) * d;
        gy += (yo - t.y) * d;
        gz += (zo - t.z) * d;
      }
    }
  }
  if (i >= nown) return;
  float* o = grad + (static_cast<size_t>(b) * nown + i) * 3;
  if (valid) {
    const float g = grad_cost[b];
    o[0] = gx * g; o[1] = gy * g; o[2] = gz * g;
  } else if (RAGGED) {
    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
  }
}

// init + 10 levels of three passes: 31 launches over the padded sizes, with or without lengths
template <bool RAGGED>
int run_levels(const float* xyz1, const float* xyz2, const int64_t* len1, const int64_t* len2, int B,
               int n, int m, float* temp, hipStream_t s) {
  float multiL, multiR;  // emd_kernel.cu:31-38, integer division (RAGGED: redone per pair on the device)
  if (n >= m) { multiL = 1.0f; multiR = static_cast<float>(n / m); }
  else        { multiL = static_cast<float>(m / n); multiR = 1.0f; }
  const int nm = n > m ? n : m;
  hipLaunchKernelGGL(emd_init_kernel<RAGGED>, dim3((nm + 255) / 256, B), dim3(256), 0, s, temp, n, m,
                     multiL, multiR, len1, len2);
  const dim3 gn((n + 255) / 256, B), gm((m + 255) / 256, B);
  for (int li = 0; li < kLevels; ++li) {
    hipLaunchKernelGGL(emd_pass1_kernel<RAGGED>, gn, dim3(256), 0, s, xyz1, xyz2, temp, n, m, li, len1, len2);
    hipLaunchKernelGGL(emd_pass2_kernel<RAGGED>, gm, dim3(256), 0, s, xyz1, xyz2, temp, n, m, li, len1, len2);
    hipLaunchKernelGGL(emd_pass3_kernel<RAGGED>, gn, dim3(256), 0, s, xyz1, xyz2, temp, n, m, li, len1, len2);
  }
  return pdr::check_launch();
}

// The four entry points, dense (RAGGED = false, no lengths) and with lengths: one validation, one launch sequence.
template <bool RAGGED>
int approxmatch(const float* xyz1, const float* xyz2, const int64_t* len1, const int64_t* len2, int B,
                int n, int m, float* match, float* temp, pdr_stream_t stream) {
  if (B < 0 || n <= 0 || m <= 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  if (!xyz1 || !xyz2 || !match || !temp) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  int rc = run_levels<RAGGED>(xyz1, xyz2, len1, len2, B, n, m, temp, s);
  if (rc != PDR_OK) return rc;
  hipLaunchKernelGGL(emd_match_kernel<RAGGED>, dim3((n + 255) / 256, (m + 15) / 16, B), dim3(256), 0, s,
                     xyz1, xyz2, temp, n, m, match, len1, len2);
  return pdr::check_launch();
}

template <bool RAGGED>
int emd_cost(const float* xyz1, const float* xyz2, const int64_t* len1, const int64_t* len2, int B, int n,
             int m, float* cost, float* temp, pdr_stream_t stream) {
  if (B < 0 || n <= 0 || m <= 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  if (!xyz1 || !xyz2 || !cost || !temp) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  int rc = run_levels<RAGGED>(xyz1, xyz2, len1, len2, B, n, m, temp, s);
  if (rc != PDR_OK) return rc;
  hipLaunchKernelGGL(emd_cost_reduce_kernel<RAGGED>, dim3(B), dim3(256), 0, s, temp, n, m, cost, len1, len2);
  return pdr::check_launch();
}

template <bool RAGGED>
int matchcost(const float* xyz1, const float* xyz2, const int64_t* len1, const int64_t* len2,
              const float* match, int B, int n, int m, float* cost, float* temp, pdr_stream_t stream) {
  if (B < 0 || n <= 0 || m <= 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  if (!xyz1 || !xyz2 || !match || !cost || !temp) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  // slab partials (B, ceil(n/256)) in `temp`, then a fixed-order sum: deterministic
  const int nblk = (n + 255) / 256;
  hipLaunchKernelGGL(matchcost_kernel<RAGGED>, dim3(nblk, B), dim3(256), 0, s, xyz1, xyz2, match, n, m,
                     temp, len1, len2);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(B), dim3(64), 0, s, temp, nblk, cost);
  return pdr::check_launch();
}

template <bool RAGGED>
int matchcost_grad(const float* grad_cost, const float* xyz1, const float* xyz2, const int64_t* len1,
                   const int64_t* len2, const float* match, int B, int n, int m, float* grad1,
                   float* grad2, pdr_stream_t stream) {
  if (B < 0 || n <= 0 || m <= 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  if (!grad_cost || !xyz1 || !xyz2 || !match || !grad1 || !grad2) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  hipLaunchKernelGGL(matchcost_grad1_kernel<RAGGED>, dim3((n + 255) / 256, B), dim3(256), 0, s,
                     grad_cost, xyz1, xyz2, match, n, m, grad1, len1, len2);
  hipLaunchKernelGGL(matchcost_grad2_kernel<RAGGED>, dim3((m + 3) / 4, B), dim3(256), 0, s, grad_cost,
                     xyz1, xyz2, match, n, m, grad2, len1, len2);
  return pdr::check_launch();
}

// `temp` holds the factors of a preceding approxmatch / emd_cost on the same clouds, lengths and sizes; read only
template <bool RAGGED>
int emd_cost_grad(const float* grad_cost, const float* xyz1, const float* xyz2, const int64_t* len1,
                  const int64_t* len2, const float* temp, int B, int n, int m, float* grad1, float* grad2,
                  pdr_stream_t stream) {
  if (B < 0 || n <= 0 || m <= 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  if (!grad_cost || !xyz1 || !xyz2 || !temp || !grad1 || !grad2) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  hipLaunchKernelGGL((emd_cost_grad_kernel<RAGGED, 0>), dim3((n + 255) / 256, B), dim3(256), 0, s, grad_cost,
                     xyz1, xyz2, temp, n, m, grad1, len1, len2);
  hipLaunchKernelGGL((emd_cost_grad_kernel<RAGGED, 1>), dim3((m + 255) / 256, B), dim3(256), 0, s, grad_cost,
                     xyz1, xyz2, temp, n, m, grad2, len1, len2);
  return pdr::check_launch();
}

}  // namespace

extern "C" size_t pdr_emd_workspace_bytes(int B, int n, int m) {
  if (B <= 0 || n <= 0 || m <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(B) * ws_floats(n, m);
}

extern "C" size_t pdr_matchcost_workspace_bytes(int B, int n, int m) {
  if (B <= 0 || n <= 0 || m <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(B) * ((n + 255) / 256);
}

extern "C" int pdr_approxmatch(const float* xyz1, const float* xyz2, int B, int n, int m,
                               float* match, float* temp, pdr_stream_t stream) {
  return approxmatch<false>(xyz1, xyz2, nullptr, nullptr, B, n, m, match, temp, stream);
}

extern "C" int pdr_emd_cost(const float* xyz1, const float* xyz2, int B, int n, int m,
                            float* cost, float* temp, pdr_stream_t stream) {
  return emd_cost<false>(xyz1, xyz2, nullptr, nullptr, B, n, m, cost, temp, stream);
}

extern "C" int pdr_matchcost(const float* xyz1, const float* xyz2, const float* match, int B,
                             int n, int m, float* cost, float* temp, pdr_stream_t stream) {
  return matchcost<false>(xyz1, xyz2, nullptr, nullptr, match, B, n, m, cost, temp, stream);
}

extern "C" int pdr_matchcost_grad(const float* grad_cost, const float* xyz1, const float* xyz2,
                                  const float* match, int B, int n, int m, float* grad1,
                                  float* grad2, pdr_stream_t stream) {
  return matchcost_grad<false>(grad_cost, xyz1, xyz2, nullptr, nullptr, match, B, n, m, grad1, grad2,
                               stream);
}

// The same calls with per-cloud lengths (device int64, read by the kernels only; NULL = full; include/pdr_hip.h).
// Without any lengths each IS the dense call.
extern "C" int pdr_approxmatch_ragged(const float* xyz1, const float* xyz2, const int64_t* lengths1,
                                      const int64_t* lengths2, int B, int n, int m, float* match,
                                      float* temp, pdr_stream_t stream) {
  if (!lengths1 && !lengths2)
    return approxmatch<false>(xyz1, xyz2, nullptr, nullptr, B, n, m, match, temp, stream);
  return approxmatch<true>(xyz1, xyz2, lengths1, lengths2, B, n, m, match, temp, stream);
}

extern "C" int pdr_emd_cost_ragged(const float* xyz1, const float* xyz2, const int64_t* lengths1,
                                   const int64_t* lengths2, int B, int n, int m, float* cost,
                                   float* temp, pdr_stream_t stream) {
  if (!lengths1 && !lengths2)
    return emd_cost<false>(xyz1, xyz2, nullptr, nullptr, B, n, m, cost, temp, stream);
  return emd_cost<true>(xyz1, xyz2, lengths1, lengths2, B, n, m, cost, temp, stream);
}

extern "C" int pdr_matchcost_ragged(const float* xyz1, const float* xyz2, const int64_t* lengths1,
                                    const int64_t* lengths2, const float* match, int B, int n, int m,
                                    float* cost, float* temp, pdr_stream_t stream) {
  if (!lengths1 && !lengths2)
    return matchcost<false>(xyz1, xyz2, nullptr, nullptr, match, B, n, m, cost, temp, stream);
  return matchcost<true>(xyz1, xyz2, lengths1, lengths2, match, B, n, m, cost, temp, stream);
}

extern "C" int pdr_matchcost_grad_ragged(const float* grad_cost, const float* xyz1, const float* xyz2,
                                         const int64_t* lengths1, const int64_t* lengths2,
                                         const float* match, int B, int n, int m, float* grad1,
                                         float* grad2, pdr_stream_t stream) {
  if (!lengths1 && !lengths2)
    return matchcost_grad<false>(grad_cost, xyz1, xyz2, nullptr, nullptr, match, B, n, m, grad1, grad2,
                                 stream);
  return matchcost_grad<true>(grad_cost, xyz1, xyz2, lengths1, lengths2, match, B, n, m, grad1, grad2,
                              stream);
}

// Matrix-free gradients of the cost from the workspace a preceding pdr_emd_cost[_ragged] / pdr_approxmatch[_ragged]
// left behind (include/pdr_hip.h): no (B, m, n) matrix, two launches, capturable.
extern "C" int pdr_emd_cost_grad(const float* grad_cost, const float* xyz1, const float* xyz2,
                                 const float* temp, int B, int n, int m, float* grad1, float* grad2,
                                 pdr_stream_t stream) {
  return emd_cost_grad<false>(grad_cost, xyz1, xyz2, nullptr, nullptr, temp, B, n, m, grad1, grad2, stream);
}

extern "C" int pdr_emd_cost_grad_ragged(const float* grad_cost, const float* xyz1, const float* xyz2,
                                        const int64_t* lengths1, const int64_t* lengths2, const float* temp,
                                        int B, int n, int m, float* grad1, float* grad2, pdr_stream_t stream) {
  if (!lengths1 && !lengths2)
    return emd_cost_grad<false>(grad_cost, xyz1, xyz2, nullptr, nullptr, temp, B, n, m, grad1, grad2, stream);
  return emd_cost_grad<true>(grad_cost, xyz1, xyz2, lengths1, lengths2, temp, B, n, m, grad1, grad2, stream);
}
