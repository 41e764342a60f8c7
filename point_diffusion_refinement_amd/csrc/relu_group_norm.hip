// relu_group_norm.hip -- the front of AttentionModule's score head on the TRAINABLE path (pointnet2_ops/attention.py:
// expand, cat, then weight_conv's ReLU and MyGroupNorm) as one differentiable op over a tensor that is never built:
// pdr_relu_group_norm_cf (two launches) and pdr_relu_group_norm_cf_grad (up to four).  group_norm_act.hip is the
// norm-then-activation link; this file is activation-then-norm over two sources and stands on its own.
//
// k (B, C2, N, K) fp32 dense, q (B, C1, N) fp32 dense or NULL with C1 = 0.  C = C1 + C2, S = N K.  The VIRTUAL tensor
//   x[b, c, n, j] = c < C1 ? q[b, c, n] : k[b, c - C1, n, j]
// is only ever read through its sources.  Cn = C - C % G, Cg = Cn / G; group g of cloud b is the virtual channels
// [g Cg, (g + 1) Cg), m = Cg S values; it may lie in q, in k, or straddle the boundary.  Channels c >= Cn pass through.
//
// OPERATION CHAIN, -ffp-contract=off, the only fused multiply-adds are the ones written here.
//   u = x > 0 ? x : (x == x ? +0.0f : x)         ReLU on EVERY channel; a NaN stays a NaN (as torch.relu leaves it)
//   statistics of a slab (doubles; every u and u^2 is exact in double):
//     k rows:  s1 = sum u,  s2 = sum fma(u, u, s2)                          over the slab's k values (order below)
//     q rows:  t1 = sum u,  t2 = sum fma(u, u, t2)  over the slab's q values, each read ONCE, then
//              t1 = fl(double(K) t1),  t2 = fl(double(K) t2)                one double rounding each: the weight K
//     S1 = t1 + (k partials in ascending order),  S2 likewise
//     mean_d = S1 / m,  var_d = max(S2 / m - mean_d mean_d, 0)
//     mean = float(mean_d),  rstd = float(1 / sqrt(var_d + double(eps)))    the fp32 values written to mean / rstd
//   element of a normalised channel c (one fp32 rounding each; gamma / beta NULL: 1 and 0 in the same chain):
//     d = fl(u - mean),  xh = fl(d rstd),  y = fma(xh, gamma[c], beta[c]);      pass-through channel: y = u
//   backward recomputes u, d, xh by the SAME sequence from q, k and the SAVED fp32 mean / rstd: the forward's bits.
//     row sums (doubles, products exact):  r1[b, c] = sum_s dy xh,   r2[b, c] = sum_s dy      (q rows: xh of n = s / K)
//     slab sums (doubles, ascending c):    c1 = sum_c gamma[c] r1[b, c],   c2 = sum_c gamma[c] r2[b, c]
//     k1 = float(c1 / m),  k2 = float(c2 / m)
//     du = fl(rstd fl(fl(gamma[c] dy) - fma(xh, k1, k2)))                  pass-through channel: du = dy
//     dx = x > 0 ? du : +0.0f                                              the mask is on the raw input: exact
//     grad_k = dx on the k channels
//     grad_q[b, c, n] = x > 0 ? float(sum_j double(du[b, c, n, j])) : +0.0f    a DOUBLE sum over j = 0 .. K - 1 in
//                       ascending order from +0, rounded to fp32 once; the q part of dx is never stored
//     dgamma[c] = float(sum_b r1[b, c]),  dbeta[c] = float(sum_b r2[b, c])  (doubles, ascending b)
// SUMMATION ORDER, a function of (C1, Cg, N, K) and the kernel family only -- never of B, the grid or timing; no atomics.
//   The k values of a slab (its k rows are contiguous in k) are cut into partitions of E elements, E from m = Cg S alone
//   (plan_of: a multiple of 1024, at least 8192, P = ceil(m / E) <= 32; a slab with fewer k rows leaves its last
//   partitions empty: they add +0).  Thread t of a partition's 256 takes the elements (256 i + t) V .. + V - 1 for
//   i = 0, 1, .. ascending (V = 4 vector family, 1 scalar family); the 64 lanes of a wave are folded by a butterfly
//   over lane distance 32, 16, .. 1, the 4 waves added in ascending order, the partials in ascending order after the
//   q term.  The q values of a slab (contiguous in q) are one partition of their own with V = 1 in both families.  A row
//   sum of the backward is the same with the row's S virtual elements as one partition.
//
// KERNEL SHAPE.  Memory-bound.  Forward: rgn_stats_kernel on a grid (B G, 1 + P) -- workgroup y = 0 sums the slab's q
// values, y = 1 .. P the k partitions, one (s1, s2) pair each -- and rgn_apply_kernel, grid (B C rows, chunks of a row),
// which combines its slab's 1 + P pairs, reads k a second time (a q row reads N floats for S outputs) and writes y; the
// workgroup of a group's first row and first chunk stores mean and rstd.  Backward: rgn_rows_kernel, a workgroup per
// normalised (b, c) row, writes (r1, r2); rgn_dk_kernel on the k rows' apply grid writes grad_k; rgn_dq_kernel, a
// thread per (b, c, n), reads its K values of grad_y and writes one grad_q; rgn_dparam_kernel, a thread per channel.
// Passes over the big tensor: forward k twice + y once; backward grad_y twice, k twice, grad_k once.  16-byte accesses
// when K % 4 == 0 and k / y (forward) or k / grad_y / grad_k (backward) are 16-byte aligned (a float4 then lies inside
// one query's K values); anything else takes the scalar family, the same kernels with 4-byte accesses.
// VALIDATION ORDER (both calls, on the host, before any launch):
//   1. B, C1, N or K negative, C2 < 1, G < 1 (forward: eps negative or NaN): PDR_EINVAL
//   2. C1 + C2 < G (nothing would be normalised): PDR_EINVAL
//   3. B N K == 0: PDR_OK, nothing launched, no pointer looked at
//   4. B C N K >= 2^31, or B C >= 2^24 (a grid's x dimension times 256 threads must stay below 2^32): PDR_EUNSUPPORTED.
//      Every y dimension is at most 65535 by construction (P <= 32; chunk grids are clamped and stride).
//   5. NULL k, C1 > 0 with q NULL, NULL y / workspace (backward: mean / rstd / grad_y), exactly one of gamma / beta
//      NULL: PDR_EINVAL; backward also: gamma NULL with grad_gamma / grad_beta, grad_q with C1 == 0, or all four
//      gradients NULL: PDR_EINVAL
// SHARED CODE: the partition plan, block_sum2, rgn_stats_kernel, the fold of a slab's partials, Row and the element chain
// (relu_of, xh_of, y_of), row_of and the size checks live in relu_group_norm.h; relu_group_norm_conv.hip uses the same.
// NOT MEASURED: see DESIGN 7a.7.
#include "pdr_common.h"
#include "relu_group_norm.h"

namespace {

constexpr long kRowChunk = 4096;     // elements of a row a workgroup of the apply / dk kernels is sized for
constexpr unsigned kMaxGridY = 65535;

// the V raw values of the row at element i (V == 4: K % 4 == 0, so the four share one query of a q row)
template <int V>
__device__ __forceinline__ void load_x(Pack<V>& p, const Row& r, long i, unsigned K) {
  if (r.is_q) {
    const float v = r.src[static_cast<unsigned>(i) / K];
#pragma unroll
    for (int j = 0; j < V; ++j) p.v[j] = v;
  } else {
    p.load(r.src + i);
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void rgn_apply_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta,
                                                        const double* __restrict__ part, int C1, int C2, int N, int K,
                                                        int G, int Cg, int Cn, int P1, float eps,
                                                        float* __restrict__ y, float* __restrict__ mean_out,
                                                        float* __restrict__ rstd_out) {
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const size_t row = blockIdx.x;                       // b C + c
  const size_t b = row / C;
  const int c = static_cast<int>(row % C);
  Row r;
  r.src = src_of(q, k, b, c, C1, C2, N, S);
  r.is_q = c < C1;
  r.norm = c < Cn;
  r.mean = 0.0f, r.rstd = 1.0f, r.gamma = 1.0f, r.beta = 0.0f;
  if (r.norm) {
    const int g = c / Cg;
    const size_t slab = b * G + g;
    slab_mean_rstd(part + slab * P1 * 2, P1, static_cast<double>(Cg) * static_cast<double>(S), eps, &r.mean, &r.rstd);
    if (gamma) r.gamma = gamma[c], r.beta = beta[c];
    if (blockIdx.y == 0 && threadIdx.x == 0 && c == g * Cg) {
      if (mean_out) mean_out[slab] = r.mean;
      if (rstd_out) rstd_out[slab] = r.rstd;
    }
  }
  float* yr = y + row * static_cast<size_t>(S);
  const long step = static_cast<long>(gridDim.y) * 256 * V;
  for (long i = (static_cast<long>(blockIdx.y) * 256 + threadIdx.x) * V; i < S; i += step) {
    Pack<V> p;
    load_x<V>(p, r, i, static_cast<unsigned>(K));
#pragma unroll
    for (int j = 0; j < V; ++j) p.v[j] = y_of(r, relu_of(p.v[j]));
    p.store(yr + i);
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------
// k1, k2 of the slab of normalised channel c from its Cg rows of (r1, r2)
__device__ __forceinline__ void slab_terms(const double* __restrict__ rows, const float* __restrict__ gamma, size_t b,
                                           int c, int C, int Cg, long S, float* k1, float* k2) {
  const int c0 = c / Cg * Cg;
  const double* o = rows + (b * C + c0) * 2;
  double c1 = 0.0, c2 = 0.0;
  for (int j = 0; j < Cg; ++j) {
    const double gm = gamma ? static_cast<double>(gamma[c0 + j]) : 1.0;
    c1 = __builtin_fma(gm, o[2 * j], c1);
    c2 = __builtin_fma(gm, o[2 * j + 1], c2);
  }
  const double m = static_cast<double>(Cg) * static_cast<double>(S);
  *k1 = static_cast<float>(c1 / m);
  *k2 = static_cast<float>(c2 / m);
}

__device__ __forceinline__ float du_of(const Row& r, float u, float dy, float k1, float k2) {
  return r.norm ? r.rstd * (r.gamma * dy - __builtin_fmaf(xh_of(r, u), k1, k2)) : dy;
}

template <int V>
__global__ __launch_bounds__(256) void rgn_rows_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ dy, int C1, int C2, int N, int K,
                                                       int G, int Cg, int Cn, double* __restrict__ rows) {
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const size_t row = blockIdx.x;
  const int c = static_cast<int>(row % C);
  if (c >= Cn) return;                                 // the whole workgroup: a pass-through row has no sums
  const size_t b = row / C;
  const Row r = row_of(src_of(q, k, b, c, C1, C2, N, S), c < C1, gamma, beta, mean, rstd, b, c, G, Cg, Cn);
  const float* gr = dy + row * static_cast<size_t>(S);
  double r1 = 0.0, r2 = 0.0;
#pragma unroll 2
  for (long i = static_cast<long>(threadIdx.x) * V; i < S; i += 256 * V) {
    Pack<V> p, g;
    load_x<V>(p, r, i, static_cast<unsigned>(K));
    g.load(gr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double d = static_cast<double>(g.v[j]);
      r1 = __builtin_fma(d, static_cast<double>(xh_of(r, relu_of(p.v[j]))), r1);
      r2 += d;
    }
  }
  block_sum2(r1, r2);
  if (threadIdx.x == 0) {
    rows[row * 2] = r1;
    rows[row * 2 + 1] = r2;
  }
}

template <int V>
__global__ __launch_bounds__(256) void rgn_dk_kernel(const float* __restrict__ k, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dy,
                                                     const double* __restrict__ rows, int C1, int C2, int N, int K,
                                                     int G, int Cg, int Cn, float* __restrict__ dk) {
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const size_t krow = blockIdx.x;                      // b C2 + (c - C1)
  const size_t b = krow / C2;
  const int c = C1 + static_cast<int>(krow % C2);
  const Row r = row_of(k + krow * static_cast<size_t>(S), false, gamma, beta, mean, rstd, b, c, G, Cg, Cn);
  float k1 = 0.0f, k2 = 0.0f;
  if (r.norm) slab_terms(rows, gamma, b, c, C, Cg, S, &k1, &k2);
  const float* gr = dy + (b * C + c) * static_cast<size_t>(S);
  float* dr = dk + krow * static_cast<size_t>(S);
  const long step = static_cast<long>(gridDim.y) * 256 * V;
  for (long i = (static_cast<long>(blockIdx.y) * 256 + threadIdx.x) * V; i < S; i += step) {
    Pack<V> p, g;
    p.load(r.src + i);
    g.load(gr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float du = du_of(r, relu_of(p.v[j]), g.v[j], k1, k2);
      p.v[j] = p.v[j] > 0.0f ? du : 0.0f;
    }
    p.store(dr + i);
  }
}

template <int V>
__global__ __launch_bounds__(256) void rgn_dq_kernel(const float* __restrict__ q, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dy,
                                                     const double* __restrict__ rows, int C1, int C2, int N, int K,
                                                     int G, int Cg, int Cn, float* __restrict__ dq) {
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const size_t qrow = blockIdx.x;                      // b C1 + c
  const size_t b = qrow / C1;
  const int c = static_cast<int>(qrow % C1);
  const Row r = row_of(q + qrow * static_cast<size_t>(N), true, gamma, beta, mean, rstd, b, c, G, Cg, Cn);
  float k1 = 0.0f, k2 = 0.0f;
  if (r.norm) slab_terms(rows, gamma, b, c, C, Cg, S, &k1, &k2);
  const float* gr = dy + (b * C + c) * static_cast<size_t>(S);
  float* dr = dq + qrow * static_cast<size_t>(N);
  const int step = static_cast<int>(gridDim.y) * 256;
  for (int n = static_cast<int>(blockIdx.y) * 256 + threadIdx.x; n < N; n += step) {
    const float x = r.src[n];
    const float u = relu_of(x);
    const float* g0 = gr + static_cast<size_t>(n) * K;
    double acc = 0.0;
    for (int j = 0; j < K; j += V) {
      Pack<V> g;
      g.load(g0 + j);
#pragma unroll
      for (int t = 0; t < V; ++t) acc += static_cast<double>(du_of(r, u, g.v[t], k1, k2));
    }
    dr[n] = x > 0.0f ? static_cast<float>(acc) : 0.0f;
  }
}

__global__ __launch_bounds__(256) void rgn_dparam_kernel(const double* __restrict__ rows, int B, int C, int Cn,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Cn) return;
  double a1 = 0.0, a2 = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* o = rows + (static_cast<size_t>(b) * C + c) * 2;
    a1 += o[0];
    a2 += o[1];
  }
  if (dgamma) dgamma[c] = static_cast<float>(a1);
  if (dbeta) dbeta[c] = static_cast<float>(a2);
}

// ---- host ----------------------------------------------------------------------------------------------------------
unsigned chunks_of(long n, long per) {
  const long c = (n + per - 1) / per;
  return static_cast<unsigned>(c > kMaxGridY ? kMaxGridY : c);
}

}  // namespace

extern "C" size_t pdr_relu_group_norm_cf_workspace_bytes(int B, int C1, int C2, int N, int K, int G) {
  long long n;
  if (check_sizes(B, C1, C2, N, K, G, 0.0f, &n) != PDR_OK || n == 0) return 0;
  const int C = C1 + C2;
  const Plan p = plan_of(C, static_cast<long>(N) * K, K, G, true);
  const size_t fwd = static_cast<size_t>(B) * G * (p.P + 1), bwd = static_cast<size_t>(B) * C;
  return (fwd > bwd ? fwd : bwd) * 2 * sizeof(double);
}

extern "C" int pdr_relu_group_norm_cf_plan(int C1, int C2, int N, int K, int G, int aligned16, long out[4]) {
  if (C1 < 0 || C2 < 1 || N < 1 || K < 1 || G < 1 || !out) return PDR_EINVAL;
  long long n;
  const int rc = check_sizes(1, C1, C2, N, K, G, 0.0f, &n);
  if (rc != PDR_OK) return rc;
  const Plan p = plan_of(C1 + C2, static_cast<long>(N) * K, K, G, aligned16 != 0);
  out[0] = p.vec;
  out[1] = p.P;
  out[2] = p.E;
  out[3] = p.Cg;
  return PDR_OK;
}

extern "C" int pdr_relu_group_norm_cf(const float* q, const float* k, const float* gamma, const float* beta, int B,
                                      int C1, int C2, int N, int K, int G, float eps, float* y, float* mean,
                                      float* rstd, void* workspace, pdr_stream_t stream) {
  long long n;
  const int rc = check_sizes(B, C1, C2, N, K, G, eps, &n);
  if (rc != PDR_OK || n == 0) return rc;
  if (!k || (C1 > 0 && !q) || !y || !workspace || (gamma == nullptr) != (beta == nullptr)) return PDR_EINVAL;
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const Plan p = plan_of(C, S, K, G, aligned16(k) && aligned16(y));
  const int Cn = p.Cg * G, P1 = static_cast<int>(p.P) + 1;
  double* part = static_cast<double*>(workspace);
  hipStream_t st = pdr::as_stream(stream);
  const dim3 gs(static_cast<unsigned>(B) * G, static_cast<unsigned>(P1));
  const dim3 ga(static_cast<unsigned>(B) * C, chunks_of(S, kRowChunk));
  if (p.vec) {
    hipLaunchKernelGGL(rgn_stats_kernel<4>, gs, dim3(256), 0, st, q, k, C1, C2, N, K, G, p.Cg, p.E, part);
    hipLaunchKernelGGL(rgn_apply_kernel<4>, ga, dim3(256), 0, st, q, k, gamma, beta, part, C1, C2, N, K, G, p.Cg, Cn,
                       P1, eps, y, mean, rstd);
  } else {
    hipLaunchKernelGGL(rgn_stats_kernel<1>, gs, dim3(256), 0, st, q, k, C1, C2, N, K, G, p.Cg, p.E, part);
    hipLaunchKernelGGL(rgn_apply_kernel<1>, ga, dim3(256), 0, st, q, k, gamma, beta, part, C1, C2, N, K, G, p.Cg, Cn,
                       P1, eps, y, mean, rstd);
  }
  return pdr::check_launch();
}

extern "C" int pdr_relu_group_norm_cf_grad(const float* q, const float* k, const float* gamma, const float* beta,
                                           const float* mean, const float* rstd, const float* grad_y, int B, int C1,
                                           int C2, int N, int K, int G, float* grad_q, float* grad_k,
                                           float* grad_gamma, float* grad_beta, void* workspace,
                                           pdr_stream_t stream) {
  long long n;
  const int rc = check_sizes(B, C1, C2, N, K, G, 0.0f, &n);
  if (rc != PDR_OK || n == 0) return rc;
  if (!k || (C1 > 0 && !q) || !mean || !rstd || !grad_y || !workspace || (gamma == nullptr) != (beta == nullptr))
    return PDR_EINVAL;
  if (!gamma && (grad_gamma || grad_beta)) return PDR_EINVAL;
  if (grad_q && C1 == 0) return PDR_EINVAL;
  if (!grad_q && !grad_k && !grad_gamma && !grad_beta) return PDR_EINVAL;
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const Plan p = plan_of(C, S, K, G, aligned16(k) && aligned16(grad_y) && aligned16(grad_k));
  const int Cn = p.Cg * G;
  double* rows = static_cast<double*>(workspace);
  hipStream_t st = pdr::as_stream(stream);
  const dim3 gr(static_cast<unsigned>(B) * C);
  const dim3 gk(static_cast<unsigned>(B) * C2, chunks_of(S, kRowChunk));
  const dim3 gq(static_cast<unsigned>(B) * C1, chunks_of(N, 256));
#define PDR_RGN_BACKWARD(V)                                                                                          \
  hipLaunchKernelGGL(rgn_rows_kernel<V>, gr, dim3(256), 0, st, q, k, gamma, beta, mean, rstd, grad_y, C1, C2, N, K, G, \
                     p.Cg, Cn, rows);                                                                                \
  if (grad_k)                                                                                                        \
    hipLaunchKernelGGL(rgn_dk_kernel<V>, gk, dim3(256), 0, st, k, gamma, beta, mean, rstd, grad_y, rows, C1, C2, N, K, \
                       G, p.Cg, Cn, grad_k);                                                                         \
  if (grad_q)                                                                                                        \
    hipLaunchKernelGGL(rgn_dq_kernel<V>, gq, dim3(256), 0, st, q, gamma, beta, mean, rstd, grad_y, rows, C1, C2, N, K, \
                       G, p.Cg, Cn, grad_q)
  if (p.vec) {
    PDR_RGN_BACKWARD(4);
  } else {
    PDR_RGN_BACKWARD(1);
  }
#undef PDR_RGN_BACKWARD
  if (grad_gamma || grad_beta)
    hipLaunchKernelGGL(rgn_dparam_kernel, dim3((Cn + 255) / 256), dim3(256), 0, st, rows, B, C, Cn, grad_gamma,
                       grad_beta);
  return pdr::check_launch();
}
