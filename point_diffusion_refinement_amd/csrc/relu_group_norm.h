// relu_group_norm.h -- the statistics pass and the element chain of MyGroupNorm(relu([q over K | k])), shared by
// relu_group_norm.hip (which writes the normalised tensor) and relu_group_norm_conv.hip (whose GEMM normalises its
// operand as it loads it): ONE definition of the partition plan, the block sum, the statistics kernel, the fold of a
// slab's partials and the chain u -> d -> xh -> y, so that both files agree bit for bit.  The operation chain, the
// summation order and the validation order are stated in the header of relu_group_norm.hip.
#pragma once
#include "pdr_common.h"

namespace {

constexpr long kPartMin = 8192;      // smallest partition of a slab, elements
constexpr long kPartMax = 32;        // most k partitions of a slab

struct Plan {
  int vec;      // 1: float4 accesses
  long P, E;    // k partitions per slab, elements per partition
  int Cg;
};

Plan plan_of(int C, long S, int K, int G, bool aligned16) {
  Plan p;
  p.Cg = (C - C % G) / G;
  p.vec = aligned16 && K % 4 == 0;
  const long m = p.Cg * S;
  long E = (m + kPartMax - 1) / kPartMax;
  E = (E + 1023) / 1024 * 1024;
  p.E = E < kPartMin ? kPartMin : E;
  p.P = m > 0 ? (m + p.E - 1) / p.E : 1;
  return p;
}

// (a, b) summed over the workgroup's 256 threads in the fixed order of the header; every thread gets the result
__device__ __forceinline__ void block_sum2(double& a, double& b) {
  __shared__ double lds[8];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  const int w = threadIdx.x >> 6;
  if (pdr::lane_id() == 0) {
    lds[2 * w] = a;
    lds[2 * w + 1] = b;
  }
  __syncthreads();
  a = ((lds[0] + lds[2]) + lds[4]) + lds[6];
  b = ((lds[1] + lds[3]) + lds[5]) + lds[7];
}

template <int V>
struct Pack;
template <>
struct Pack<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <>
struct Pack<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// torch.relu: a NaN is kept, everything else that is not positive becomes +0
__device__ __forceinline__ float relu_of(float x) { return x > 0.0f ? x : (x == x ? 0.0f : x); }

// a virtual (b, c) row: where its values come from and what turns u into y
struct Row {
  const float* src;   // q row (N floats) or k row (S floats)
  bool is_q, norm;
  float mean, rstd, gamma, beta;
};

__device__ __forceinline__ const float* src_of(const float* __restrict__ q, const float* __restrict__ k, size_t b, int c,
                                               int C1, int C2, int N, long S) {
  return c < C1 ? q + (b * C1 + c) * static_cast<size_t>(N) : k + (b * C2 + (c - C1)) * static_cast<size_t>(S);
}

__device__ __forceinline__ float xh_of(const Row& r, float u) {
  const float d = u - r.mean;
  return d * r.rstd;
}

__device__ __forceinline__ float y_of(const Row& r, float u) {
  return r.norm ? __builtin_fmaf(xh_of(r, u), r.gamma, r.beta) : u;
}

// mean and rstd of a slab from its 1 + P pairs of partials: the q term, then the k partials, ascending
__device__ __forceinline__ void slab_mean_rstd(const double* __restrict__ o, int P1, double m, float eps, float* mean_f,
                                               float* rstd_f) {
  double s1 = 0.0, s2 = 0.0;
  for (int p = 0; p < P1; ++p) {
    s1 += o[2 * p];
    s2 += o[2 * p + 1];
  }
  const double mean = s1 / m;
  double var = s2 / m - mean * mean;
  if (var < 0.0) var = 0.0;
  *mean_f = static_cast<float>(mean);
  *rstd_f = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
}

// the row of virtual channel c of cloud b from SAVED fp32 statistics
__device__ __forceinline__ Row row_of(const float* src, bool is_q, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                      const float* __restrict__ rstd, size_t b, int c, int G, int Cg, int Cn) {
  Row r;
  r.src = src;
  r.is_q = is_q;
  r.norm = c < Cn;
  r.mean = 0.0f, r.rstd = 1.0f, r.gamma = 1.0f, r.beta = 0.0f;
  if (r.norm) {
    const size_t slab = b * G + c / Cg;
    r.mean = mean[slab];
    r.rstd = rstd[slab];
    if (gamma) r.gamma = gamma[c], r.beta = beta[c];
  }
  return r;
}

template <int V>
__global__ __launch_bounds__(256) void rgn_stats_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                        int C1, int C2, int N, int K, int G, int Cg, long E,
                                                        double* __restrict__ part) {
  const size_t slab = blockIdx.x;                      // b G + g
  const size_t b = slab / G;
  const int c0 = static_cast<int>(slab % G) * Cg, c1 = c0 + Cg;
  double s1 = 0.0, s2 = 0.0;
  if (blockIdx.y == 0) {                               // the slab's q values, each once, weighted by K at the end
    const int cq = c1 < C1 ? c1 : C1;
    if (c0 < cq) {
      const float* base = q + (b * C1 + c0) * static_cast<size_t>(N);
      const long len = static_cast<long>(cq - c0) * N;
      for (long i = threadIdx.x; i < len; i += 256) {
        const double d = static_cast<double>(relu_of(base[i]));
        s1 += d;
        s2 = __builtin_fma(d, d, s2);
      }
    }
    block_sum2(s1, s2);
    s1 = static_cast<double>(K) * s1;
    s2 = static_cast<double>(K) * s2;
  } else {                                             // partition y - 1 of the slab's k values
    const int k0 = (c0 > C1 ? c0 : C1) - C1, k1 = c1 - C1;
    if (k0 < k1) {
      const long S = static_cast<long>(N) * K;
      const float* base = k + (b * C2 + k0) * static_cast<size_t>(S);
      const long mk = static_cast<long>(k1 - k0) * S;
      const long lo = static_cast<long>(blockIdx.y - 1) * E;
      const long hi = lo + E < mk ? lo + E : mk;       // V == 4: mk, E and lo are multiples of 4
#pragma unroll 4
      for (long i = lo + static_cast<long>(threadIdx.x) * V; i < hi; i += 256 * V) {
        Pack<V> p;
        p.load(base + i);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const double d = static_cast<double>(relu_of(p.v[j]));
          s1 += d;
          s2 = __builtin_fma(d, d, s2);
        }
      }
    }
    block_sum2(s1, s2);
  }
  if (threadIdx.x == 0) {
    double* o = part + (slab * gridDim.y + blockIdx.y) * 2;
    o[0] = s1;
    o[1] = s2;
  }
}

// steps 1-4 of the validation order; *n = B C N K on PDR_OK (0: nothing to do)
int check_sizes(int B, int C1, int C2, int N, int K, int G, float eps, long long* n) {
  *n = 0;
  if (B < 0 || C1 < 0 || N < 0 || K < 0 || C2 < 1 || G < 1 || !(eps >= 0.0f)) return PDR_EINVAL;
  const long long C = static_cast<long long>(C1) + C2;
  if (C < G) return PDR_EINVAL;
  if (B == 0 || N == 0 || K == 0) return PDR_OK;
  constexpr long long lim = 1ll << 31;
  const long long rows = B * C;                        // both below 2^32: no overflow
  if (rows >= (1ll << 24)) return PDR_EUNSUPPORTED;
  const long long S = static_cast<long long>(N) * K;   // below 2^62
  if (S >= lim || rows * S >= lim) return PDR_EUNSUPPORTED;
  *n = rows * S;
  return PDR_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // NULL counts as aligned

}  // namespace
