// attention_pool_cf.hip -- the pooling tail of AttentionModule.forward (attention.py:71-77) for the TRAINABLE path:
// channel-first, differentiable, one launch forward (pdr_attention_pool_cf) and one backward (pdr_attention_pool_cf_grad).
//
// Replaces the torch chain  mask = count_to_mask(clamp(count, 1), K);  scores * mask + (-1e9) * (1 - mask);
// softmax(dim=-1);  (values * weight).sum(-1)  -- seven full-size (B, C, N, K) passes forward, a saved softmax output
// and as many launches again backward -- by one read of scores and values forward, and one read of both plus one write
// of both gradients backward.  pdr_attention_pool (fused_gather.hip) is the channel-last, forward-only form of the
// graph-captured sampler; this file is its transpose: K innermost, as Conv2d writes it.
//
// OPERATION CHAIN of row (b, c, n), c_n = min(max(counts[b, n], 1), K) (counts NULL: c_n = K); every step one fp32
// rounding, -ffp-contract=off, the only fused multiply-adds are the ones written here:
//     t_k = k < c_n ? s_k : -1e9f                       the score held by a masked slot is not inspected
//     a_k = fl(t_k * fl(log2 e))
//     m   = max_k a_k                                   exact
//     e_k = v_exp_f32(fl(a_k - m))                      in [0, 1], 1 at the maximum
//     l   = sum_k e_k            acc = sum_k fma(v_k, e_k, acc)          (orders below)
//     out = fl(acc / l)
// backward, after the SAME chain on the same inputs (so m, l and out have the forward's bits; nothing is saved):
//     rl  = fl(1 / l)            w_k = fl(e_k * rl)
//     grad_values[k] = fl(g * w_k)
//     grad_scores[k] = k < c_n ? fl(fl(g * w_k) * fl(v_k - out)) : +0.0f
// SUMMATION ORDER.  Scalar family: l and acc start from +0.0f and take the slots in ascending k.  Vector family: lane j
// of a row's L lanes holds slots 4j .. 4j+3, adds them in ascending k from +0.0f, and the L partial sums are folded by
// a butterfly over lane distance 1, 2, 4, 8 (DPP quad_perm, quad_perm, row_half_mirror, row_mirror: every lane of the
// group ends with the same bits).  Slots >= K of an idle lane carry a = -inf, e = 0, v = 0.  The two families agree up
// to that order; each gives the same bits for the same input.
//
// KERNEL SHAPE.  Memory-bound; rows are 16-256 bytes.  Vector family (K % 4 == 0, every pointer 16-byte aligned): a row
// belongs to L = ceil_pow2(K / 4) ADJACENT lanes, one float4 each, so a wave's load instruction covers 64 / L consecutive
// rows -- one contiguous KiB when K / 4 is a power of two -- instead of 64 different cache lines.  256 threads = 256 / L
// rows per workgroup; the grid covers all rows (at most 2^27 workgroups), no grid stride.  Scalar family (any other
// K <= 64, or a misaligned pointer): a thread per row, three passes over its K slots (maximum; sums; backward: the
// gradients) with scalar loads, passes two and three out of the cache.  No LDS, no workspace, no atomics.
// Bytes per row: forward 8 K + 4 (+ 4 for the count); backward 8 K + 4 read, 4 K written per requested gradient.
#include "pdr_common.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kMasked = -1e9f;
constexpr int kMaxK = 64;

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// Butterfly over the L adjacent lanes of a row (L a power of two <= 16, groups aligned to L: inside one DPP row).  After
// the two quad_perm steps a quad is uniform, so the mirrors (lane i <-> 7 - i, i <-> 15 - i) pair each quad with the
// right partner; a + b and b + a have the same bits, so the whole group ends uniform.
template <int L, bool MAX>
__device__ __forceinline__ float group_fold(float v) {
#define PDR_FOLD(ctrl) { const float o = dpp_f32<ctrl>(v); v = MAX ? fmaxf(v, o) : v + o; }
  if (L >= 2) PDR_FOLD(0xB1)     // quad_perm [1,0,3,2]
  if (L >= 4) PDR_FOLD(0x4E)     // quad_perm [2,3,0,1]
  if (L >= 8) PDR_FOLD(0x141)    // row_half_mirror
  if (L >= 16) PDR_FOLD(0x140)   // row_mirror
#undef PDR_FOLD
  return v;
}

// c_n of the row: counts[b N + n] with row = (b C + c) N + n, clamped to [1, K]
__device__ __forceinline__ int row_count(const int* __restrict__ counts, unsigned row, unsigned C, unsigned N, int K) {
  if (!counts) return K;
  const unsigned b = row / (C * N), n = row % N;
  const int c = counts[static_cast<size_t>(b) * N + n];
  return c < 1 ? 1 : (c > K ? K : c);
}

// GRAD false: out[row].  GRAD true: grad_scores / grad_values (either may be NULL) from grad_out[row].
template <int L, bool GRAD>
__global__ __launch_bounds__(256) void pool_cf_vec_kernel(const float* __restrict__ scores,
                                                          const float* __restrict__ values,
                                                          const int* __restrict__ counts,
                                                          const float* __restrict__ grad_out, unsigned C, unsigned N,
                                                          int K, unsigned rows, float* __restrict__ out,
                                                          float* __restrict__ grad_scores,
                                                          float* __restrict__ grad_values) {
  constexpr unsigned RPB = 256 / L;
  const int k0 = 4 * static_cast<int>(threadIdx.x % L);
  const unsigned row_raw = blockIdx.x * RPB + threadIdx.x / L;
  const bool live = row_raw < rows;
  const unsigned row = live ? row_raw : rows - 1;     // rows past the end shadow the last one: every lane folds
  const bool has = k0 < K;                            // K % 4 == 0: a lane holds four slots or none
  const int cn = row_count(counts, row, C, N, K);
  const size_t at = static_cast<size_t>(row) * K + k0;
  float4 s4 = make_float4(0, 0, 0, 0), v4 = make_float4(0, 0, 0, 0);
  if (has) {
    s4 = *reinterpret_cast<const float4*>(scores + at);
    v4 = *reinterpret_cast<const float4*>(values + at);
  }
  const float s[4] = {s4.x, s4.y, s4.z, s4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
  float a[4], m = -__builtin_inff();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + i;
    a[i] = k >= K ? -__builtin_inff() : (k < cn ? s[i] : kMasked) * kLog2e;
    m = fmaxf(m, a[i]);
  }
  m = group_fold<L, true>(m);
  float e[4], l = 0.0f, acc = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[i] = __builtin_amdgcn_exp2f(a[i] - m);
    l += e[i];
    acc = __builtin_fmaf(v[i], e[i], acc);
  }
  l = group_fold<L, false>(l);
  acc = group_fold<L, false>(acc);
  const float o = acc / l;
  if (!GRAD) {
    if (live && k0 == 0) out[row] = o;
    return;
  }
  const float g = grad_out[row];
  const float rl = 1.0f / l;
  float gv[4], gs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gv[i] = g * (e[i] * rl);
    gs[i] = k0 + i < cn ? gv[i] * (v[i] - o) : 0.0f;
  }
  if (live && has) {
    if (grad_values) *reinterpret_cast<float4*>(grad_values + at) = make_float4(gv[0], gv[1], gv[2], gv[3]);
    if (grad_scores) *reinterpret_cast<float4*>(grad_scores + at) = make_float4(gs[0], gs[1], gs[2], gs[3]);
  }
}

template <bool GRAD>
__global__ __launch_bounds__(256) void pool_cf_scalar_kernel(const float* __restrict__ scores,
                                                             const float* __restrict__ values,
                                                             const int* __restrict__ counts,
                                                             const float* __restrict__ grad_out, unsigned C, unsigned N,
                                                             int K, unsigned rows, float* __restrict__ out,
                                                             float* __restrict__ grad_scores,
                                                             float* __restrict__ grad_values) {
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= rows) return;
  const unsigned row = static_cast<unsigned>(t);
  const int cn = row_count(counts, row, C, N, K);
  const float* s = scores + static_cast<size_t>(row) * K;
  const float* v = values + static_cast<size_t>(row) * K;
  float m = -__builtin_inff();
  for (int k = 0; k < K; ++k) m = fmaxf(m, (k < cn ? s[k] : kMasked) * kLog2e);
  float l = 0.0f, acc = 0.0f;
  for (int k = 0; k < K; ++k) {
    const float e = __builtin_amdgcn_exp2f((k < cn ? s[k] : kMasked) * kLog2e - m);
    l += e;
    acc = __builtin_fmaf(v[k], e, acc);
  }
  const float o = acc / l;
  if (!GRAD) {
    out[row] = o;
    return;
  }
  const float g = grad_out[row];
  const float rl = 1.0f / l;
  float* gsr = grad_scores ? grad_scores + static_cast<size_t>(row) * K : nullptr;
  float* gvr = grad_values ? grad_values + static_cast<size_t>(row) * K : nullptr;
  for (int k = 0; k < K; ++k) {
    const float e = __builtin_amdgcn_exp2f((k < cn ? s[k] : kMasked) * kLog2e - m);
    const float gv = g * (e * rl);
    if (gvr) gvr[k] = gv;
    if (gsr) gsr[k] = k < cn ? gv * (v[k] - o) : 0.0f;
  }
}

struct Plan {
  int vec, L;
};

Plan plan_of(int K, bool aligned16) {
  if (!aligned16 || K % 4 != 0) return {0, 1};
  int L = 1;
  while (4 * L < K) L *= 2;
  return {1, L};
}

// the checks both calls share, in the order the header states them; *rows = B C N on PDR_OK with something to do
int check_sizes(int B, int C, int N, int K, unsigned* rows) {
  *rows = 0;
  if (B < 0 || C < 0 || N < 0 || K <= 0) return PDR_EINVAL;
  if (B == 0 || C == 0 || N == 0) return PDR_OK;
  if (K > kMaxK) return PDR_EUNSUPPORTED;
  constexpr long long lim = 1ll << 31;
  long long p = static_cast<long long>(B) * C;        // every factor >= 1: a product at or above 2^31 stays there
  if (p >= lim) return PDR_EUNSUPPORTED;
  p *= N;
  if (p >= lim) return PDR_EUNSUPPORTED;
  if (p * K >= lim) return PDR_EUNSUPPORTED;
  *rows = static_cast<unsigned>(p);
  return PDR_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // NULL counts as aligned

template <bool GRAD>
int launch(const float* scores, const float* values, const int* counts, const float* grad_out, int C, int N, int K,
           unsigned rows, float* out, float* grad_scores, float* grad_values, pdr_stream_t stream) {
  const bool al = aligned16(scores) && aligned16(values) && aligned16(counts) && aligned16(grad_out) && aligned16(out) &&
                  aligned16(grad_scores) && aligned16(grad_values);
  const Plan p = plan_of(K, al);
  hipStream_t st = pdr::as_stream(stream);
  const unsigned uC = static_cast<unsigned>(C), uN = static_cast<unsigned>(N);
#define PDR_LAUNCH_VEC(LL)                                                                                          \
  hipLaunchKernelGGL((pool_cf_vec_kernel<LL, GRAD>), dim3((rows + 256 / LL - 1) / (256 / LL)), dim3(256), 0, st, scores, \
                     values, counts, grad_out, uC, uN, K, rows, out, grad_scores, grad_values)
  if (!p.vec)
    hipLaunchKernelGGL((pool_cf_scalar_kernel<GRAD>), dim3(pdr::blocks_for(static_cast<long>(rows))), dim3(256), 0, st,
                       scores, values, counts, grad_out, uC, uN, K, rows, out, grad_scores, grad_values);
  else if (p.L == 1) PDR_LAUNCH_VEC(1);
  else if (p.L == 2) PDR_LAUNCH_VEC(2);
  else if (p.L == 4) PDR_LAUNCH_VEC(4);
  else if (p.L == 8) PDR_LAUNCH_VEC(8);
  else PDR_LAUNCH_VEC(16);
#undef PDR_LAUNCH_VEC
  return pdr::check_launch();
}

}  // namespace

extern "C" int pdr_attention_pool_cf_plan(int K, int aligned16, int out[4]) {
  if (K <= 0 || !out) return PDR_EINVAL;
  if (K > kMaxK) return PDR_EUNSUPPORTED;
  const Plan p = plan_of(K, aligned16 != 0);
  out[0] = p.vec;
  out[1] = p.L;
  out[2] = 256 / p.L;
  out[3] = 0;                                         // the grid covers all rows
  return PDR_OK;
}

extern "C" int pdr_attention_pool_cf(const float* scores, const float* values, const int* counts, int B, int C, int N,
                                     int K, float* out, pdr_stream_t stream) {
  unsigned rows;
  const int rc = check_sizes(B, C, N, K, &rows);
  if (rc != PDR_OK || rows == 0) return rc;
  if (!scores || !values || !out) return PDR_EINVAL;
  return launch<false>(scores, values, counts, nullptr, C, N, K, rows, out, nullptr, nullptr, stream);
}

extern "C" int pdr_attention_pool_cf_grad(const float* scores, const float* values, const int* counts,
                                          const float* grad_out, int B, int C, int N, int K, float* grad_scores,
                                          float* grad_values, pdr_stream_t stream) {
  unsigned rows;
  const int rc = check_sizes(B, C, N, K, &rows);
  if (rc != PDR_OK || rows == 0) return rc;
  if (!scores || !values || !grad_out || (!grad_scores && !grad_values)) return PDR_EINVAL;
  return launch<true>(scores, values, counts, grad_out, C, N, K, rows, nullptr, grad_scores, grad_values, stream);
}
