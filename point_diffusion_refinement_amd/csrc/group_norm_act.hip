// group_norm_act.hip -- the link that follows almost every 1x1 convolution of the TRAINABLE path, MyGroupNorm then
// ReLU / Swish (pointnet2_ops/attention.py:18-32, pointnet2_modules.py:37-53), as one differentiable op:
// pdr_group_norm_act (two launches) and pdr_group_norm_act_grad (three launches).  The inference path folds GroupNorm
// into its consumer kernels (gn_stats.hip, gn_fold.h); this file is for the module path, which had no kernel for it.
//
// x (B, C, S) fp32 dense, S = the product of all trailing dimensions.  Cn = C - C % G, Cg = Cn / G.  Group g of cloud b
// is the contiguous slab of m = Cg S floats at (b C + g Cg) S.  Channels c >= Cn pass through: z = x.
//
// OPERATION CHAIN, -ffp-contract=off, the only fused multiply-adds are the ones written here.
//   statistics of a slab (doubles; every x and x^2 is exact in double):
//     s1 = sum x,  s2 = sum fma(x, x, s2)                                   (order below)
//     mean_d = s1 / m,  var_d = max(s2 / m - mean_d mean_d, 0)
//     mean = float(mean_d),  rstd = float(1 / sqrt(var_d + double(eps)))   the fp32 values written to mean / rstd
//   element of a normalised channel c (every step one fp32 rounding; gamma / beta NULL: 1 and 0 in the same chain):
//     d = fl(x - mean),  xh = fl(d rstd),  z = fma(xh, gamma[c], beta[c])
//   activation:  0: y = z.   1: y = z > 0 ? z : +0.0f.
//     2: t = fl(z fl(-log2 e)),  e = v_exp_f32(t),  s = fl(1 / fl(1 + e)),  y = fl(z s)
//   backward recomputes d, xh, z (and s) by the SAME sequence from x and the SAVED fp32 mean / rstd: the forward's
//   bits, so the ReLU mask z > 0 is the forward's.  Then
//     dz = 0: dy   1: z > 0 ? dy : +0.0f   2: fl(dy fl(s fl(1 + fl(z fl(1 - s)))))
//     row sums (doubles, products exact):  r1[b, c] = sum_s dz xh,   r2[b, c] = sum_s dz
//     slab sums (doubles, ascending c):    c1 = sum_c gamma[c] r1[b, c],   c2 = sum_c gamma[c] r2[b, c]
//     k1 = float(c1 / m),  k2 = float(c2 / m)
//     dx = fl(rstd fl(fl(gamma[c] dz) - fma(xh, k1, k2)))                  pass-through channel: dx = dz
//     dgamma[c] = float(sum_b r1[b, c]),  dbeta[c] = float(sum_b r2[b, c])  (doubles, ascending b)
// SUMMATION ORDER, a function of (Cg, S) and the kernel family only -- never of B, the grid or timing; no atomics.
//   A slab is cut into P partitions of E elements (plan_of: E a multiple of 1024, at least 8192, P <= 32, from m
//   alone).  Thread t of a partition's 256 takes the elements (256 i + t) V .. + V - 1 of the partition for
//   i = 0, 1, .. in ascending order (V = 4 vector family, 1 scalar family); the 64 lanes of a wave are folded by a
//   butterfly over lane distance 32, 16, .. 1 (a + b = b + a: every lane ends with the same bits), the 4 waves are
//   added in ascending order, and the P partials in ascending order.  A row sum of the backward is the same with the
//   row's S elements as one partition.
//
// KERNEL SHAPE.  Memory-bound; a slab is contiguous.  Forward: gn_stats_kernel on a grid (B G, P) reads x once with
// 16-byte loads and writes one (s1, s2) pair per workgroup; gn_apply_kernel, grid (B C rows, chunks of a row), reads x
// a second time (out of L2 / Infinity Cache where the tensor fits) and writes y; every workgroup combines its slab's
// P <= 32 partials itself, and the workgroup of a group's first row and first chunk stores mean and rstd.  Backward:
// gn_rows_kernel, a workgroup per (b, c) row, writes (r1, r2); gn_dx_kernel, the apply kernel's grid, combines its
// slab's Cg rows and writes dx; gn_dparam_kernel, a thread per channel, adds the rows over b.  Bytes: forward 2 reads
// + 1 write of the tensor, backward 4 reads (x and dy twice) + 1 write.  S % 4 != 0 or a pointer of x / y / grad_y /
// grad_x that is not 16-byte aligned takes the scalar family: the same kernels with 4-byte accesses.
// NOT MEASURED: a single launch with one workgroup per slab, and other values of P / E.
//
// INJECTION AND RESIDUAL (pdr_group_norm_act_add / pdr_group_norm_act_add_grad): what Mlp_plus_t_emb adds
// behind a [conv, MyGroupNorm, act] stack, e (B, C) broadcast over S and r (B, C, S), each optional, in the order of
// the composition h + e[:, :, None] then + r:
//     y = fl(fl(act(z) + e[b, c]) + r[b, c, s])        an absent term is skipped, not added as zero
//   Forward: gn_stats_kernel as above; the apply kernel's ADD variant loads e[b C + c] once per workgroup (a uniform
//   address: a scalar) and r with the family's pack width (the vector family also needs r 16-byte aligned).  Without
//   e and r the entry launches the kernels of pdr_group_norm_act: the same bits.  Bytes: one more read with r.
//   Backward: d y / d act(z) = 1, so grad_x, grad_gamma, grad_beta are the chain above on the same grad_y, bit for bit,
//   and need neither e nor r; grad_r is grad_y itself (no kernel: the caller returns it);
//     grad_e[b, c] = float(sum_s double(grad_y[b, c, s]))    the RAW grad_y, not dz, pass-through rows too
//   summed by the row kernel's GE variant in the row order above (thread stride, butterfly, four waves ascending), in
//   double, rounded once, written by thread 0 of the row's workgroup: no launch and no workspace more.
#include "pdr_common.h"

namespace {

constexpr float kNegLog2e = -1.44269504088896340736f;
constexpr long kPartMin = 8192;      // smallest partition of a slab, elements
constexpr long kPartMax = 32;        // most partitions of a slab
constexpr long kRowChunk = 4096;     // elements of a row a workgroup of the apply / dx kernels is sized for
constexpr unsigned kMaxGridY = 65535;

struct Plan {
  int vec;      // 1: float4 accesses
  long P, E;    // partitions per slab, elements per partition
  int Cg;
};

Plan plan_of(int C, long S, int G, bool aligned16) {
  Plan p;
  p.Cg = (C - C % G) / G;
  p.vec = aligned16 && S % 4 == 0;
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

// the same for three sums (the row kernel with grad_e): the order of each is block_sum2's
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c) {
  __shared__ double lds[12];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  const int w = threadIdx.x >> 6;
  if (pdr::lane_id() == 0) {
    lds[3 * w] = a;
    lds[3 * w + 1] = b;
    lds[3 * w + 2] = c;
  }
  __syncthreads();
  a = ((lds[0] + lds[3]) + lds[6]) + lds[9];
  b = ((lds[1] + lds[4]) + lds[7]) + lds[10];
  c = ((lds[2] + lds[5]) + lds[8]) + lds[11];
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

// what a (b, c) row needs to turn x into z
struct Row {
  bool norm;
  float mean, rstd, gamma, beta;
};

__device__ __forceinline__ float z_of(const Row& r, float x, float* xh) {
  if (!r.norm) {
    *xh = 0.0f;
    return x;
  }
  const float d = x - r.mean;
  *xh = d * r.rstd;
  return __builtin_fmaf(*xh, r.gamma, r.beta);
}

__device__ __forceinline__ float sigmoid_of(float z) {
  const float e = __builtin_amdgcn_exp2f(z * kNegLog2e);
  return 1.0f / (1.0f + e);
}

template <int ACT>
__device__ __forceinline__ float act_of(float z) {
  if (ACT == 1) return z > 0.0f ? z : 0.0f;
  if (ACT == 2) return z * sigmoid_of(z);
  return z;
}

template <int ACT>
__device__ __forceinline__ float dz_of(float z, float dy) {
  if (ACT == 1) return z > 0.0f ? dy : 0.0f;
  if (ACT == 2) {
    const float s = sigmoid_of(z);
    return dy * (s * (1.0f + z * (1.0f - s)));
  }
  return dy;
}

// ---- forward -------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, int C, long S, int G, int Cg,
                                                       long m, long E, double* __restrict__ part) {
  const size_t slab = blockIdx.x;                      // b G + g
  const size_t b = slab / G, g = slab % G;
  const float* base = x + (b * C + g * Cg) * static_cast<size_t>(S);
  const long lo = static_cast<long>(blockIdx.y) * E;
  const long hi = lo + E < m ? lo + E : m;             // V == 4: m, E and lo are multiples of 4
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (long i = lo + static_cast<long>(threadIdx.x) * V; i < hi; i += 256 * V) {
    Pack<V> p;
    p.load(base + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double d = static_cast<double>(p.v[j]);
      s1 += d;
      s2 = __builtin_fma(d, d, s2);
    }
  }
  block_sum2(s1, s2);
  if (threadIdx.x == 0) {
    double* q = part + (slab * gridDim.y + blockIdx.y) * 2;
    q[0] = s1;
    q[1] = s2;
  }
}

// ADD: y = fl(fl(act(z) + e[row]) + res[row, s]), e / res each may be NULL (not both: the host launches ADD = false)
template <int V, int ACT, bool ADD>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta,
                                                       const double* __restrict__ part, int C, long S, int G, int Cg,
                                                       int Cn, int P, float eps, const float* __restrict__ e,
                                                       const float* __restrict__ res, float* __restrict__ y,
                                                       float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const size_t row = blockIdx.x;                       // b C + c
  const size_t b = row / C;
  const int c = static_cast<int>(row % C);
  Row r;
  r.norm = c < Cn;
  r.mean = 0.0f, r.rstd = 1.0f, r.gamma = 1.0f, r.beta = 0.0f;
  if (r.norm) {
    const int g = c / Cg;
    const size_t slab = b * G + g;
    const double* q = part + slab * P * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < P; ++p) {
      s1 += q[2 * p];
      s2 += q[2 * p + 1];
    }
    const double m = static_cast<double>(Cg) * static_cast<double>(S);
    const double mean = s1 / m;
    double var = s2 / m - mean * mean;
    if (var < 0.0) var = 0.0;
    r.mean = static_cast<float>(mean);
    r.rstd = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
    if (gamma) r.gamma = gamma[c], r.beta = beta[c];
    if (blockIdx.y == 0 && threadIdx.x == 0 && c == g * Cg) {
      if (mean_out) mean_out[slab] = r.mean;
      if (rstd_out) rstd_out[slab] = r.rstd;
    }
  }
  const float* xr = x + row * static_cast<size_t>(S);
  float* yr = y + row * static_cast<size_t>(S);
  const long step = static_cast<long>(gridDim.y) * 256 * V;
  if (ADD) {
    const bool has_e = e != nullptr;                   // uniform over the grid
    const float ev = has_e ? e[row] : 0.0f;            // one value per workgroup
    const float* rr = res ? res + row * static_cast<size_t>(S) : nullptr;
    for (long i = (static_cast<long>(blockIdx.y) * 256 + threadIdx.x) * V; i < S; i += step) {
      Pack<V> p, q;
      p.load(xr + i);
      if (rr) q.load(rr + i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float xh;
        float a = act_of<ACT>(z_of(r, p.v[j], &xh));
        if (has_e) a = a + ev;
        if (rr) a = a + q.v[j];
        p.v[j] = a;
      }
      p.store(yr + i);
    }
    return;
  }
  for (long i = (static_cast<long>(blockIdx.y) * 256 + threadIdx.x) * V; i < S; i += step) {
    Pack<V> p;
    p.load(xr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float xh;
      p.v[j] = act_of<ACT>(z_of(r, p.v[j], &xh));
    }
    p.store(yr + i);
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Row row_of(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ mean, const float* __restrict__ rstd, size_t b, int c,
                                      int G, int Cg, int Cn) {
  Row r;
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

// GE: also ge[row] = float(sum_s double(dy)), the raw dy in the order of r2, on EVERY row (pass-through rows read dy
// alone and write no row sums)
template <int V, int ACT, bool GE>
__global__ __launch_bounds__(256) void gn_rows_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ dy,
                                                      int C, long S, int G, int Cg, int Cn,
                                                      double* __restrict__ rows, float* __restrict__ ge) {
  const size_t row = blockIdx.x;
  const int c = static_cast<int>(row % C);
  const float* gr = dy + row * static_cast<size_t>(S);
  if (c >= Cn) {                                       // the whole workgroup: a pass-through row has no row sums
    if (GE) {
      double r3 = 0.0, none = 0.0;
#pragma unroll 2
      for (long i = static_cast<long>(threadIdx.x) * V; i < S; i += 256 * V) {
        Pack<V> q;
        q.load(gr + i);
#pragma unroll
        for (int j = 0; j < V; ++j) r3 += static_cast<double>(q.v[j]);
      }
      block_sum2(r3, none);
      if (threadIdx.x == 0) ge[row] = static_cast<float>(r3);
    }
    return;
  }
  const Row r = row_of(gamma, beta, mean, rstd, row / C, c, G, Cg, Cn);
  const float* xr = x + row * static_cast<size_t>(S);
  double r1 = 0.0, r2 = 0.0, r3 = 0.0;
#pragma unroll 2
  for (long i = static_cast<long>(threadIdx.x) * V; i < S; i += 256 * V) {
    Pack<V> p, q;
    p.load(xr + i);
    q.load(gr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float xh;
      const float z = z_of(r, p.v[j], &xh);
      const double dz = static_cast<double>(dz_of<ACT>(z, q.v[j]));
      r1 = __builtin_fma(dz, static_cast<double>(xh), r1);
      r2 += dz;
      if (GE) r3 += static_cast<double>(q.v[j]);
    }
  }
  if (GE)
    block_sum3(r1, r2, r3);
  else
    block_sum2(r1, r2);
  if (threadIdx.x == 0) {
    rows[row * 2] = r1;
    rows[row * 2 + 1] = r2;
    if (GE) ge[row] = static_cast<float>(r3);
  }
}

template <int V, int ACT>
__global__ __launch_bounds__(256) void gn_dx_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, const float* __restrict__ dy,
                                                    const double* __restrict__ rows, int C, long S, int G, int Cg,
                                                    int Cn, float* __restrict__ dx) {
  const size_t row = blockIdx.x;
  const size_t b = row / C;
  const int c = static_cast<int>(row % C);
  const Row r = row_of(gamma, beta, mean, rstd, b, c, G, Cg, Cn);
  float k1 = 0.0f, k2 = 0.0f;
  if (r.norm) {
    const int c0 = c / Cg * Cg;
    const double* q = rows + (b * C + c0) * 2;
    double c1 = 0.0, c2 = 0.0;
    for (int j = 0; j < Cg; ++j) {
      const double gm = gamma ? static_cast<double>(gamma[c0 + j]) : 1.0;
      c1 = __builtin_fma(gm, q[2 * j], c1);
      c2 = __builtin_fma(gm, q[2 * j + 1], c2);
    }
    const double m = static_cast<double>(Cg) * static_cast<double>(S);
    k1 = static_cast<float>(c1 / m);
    k2 = static_cast<float>(c2 / m);
  }
  const float* xr = x + row * static_cast<size_t>(S);
  const float* gr = dy + row * static_cast<size_t>(S);
  float* dr = dx + row * static_cast<size_t>(S);
  const long step = static_cast<long>(gridDim.y) * 256 * V;
  for (long i = (static_cast<long>(blockIdx.y) * 256 + threadIdx.x) * V; i < S; i += step) {
    Pack<V> p, q;
    p.load(xr + i);
    q.load(gr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float xh;
      const float z = z_of(r, p.v[j], &xh);
      const float dz = dz_of<ACT>(z, q.v[j]);
      p.v[j] = r.norm ? r.rstd * (r.gamma * dz - __builtin_fmaf(xh, k1, k2)) : dz;
    }
    p.store(dr + i);
  }
}

__global__ __launch_bounds__(256) void gn_dparam_kernel(const double* __restrict__ rows, int B, int C, int Cn,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Cn) return;
  double a1 = 0.0, a2 = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* q = rows + (static_cast<size_t>(b) * C + c) * 2;
    a1 += q[0];
    a2 += q[1];
  }
  if (dgamma) dgamma[c] = static_cast<float>(a1);
  if (dbeta) dbeta[c] = static_cast<float>(a2);
}

// ---- host ----------------------------------------------------------------------------------------------------------
// the checks all calls share, in the order the header states them; *n = B C S on PDR_OK (0: nothing to do)
int check_sizes(int B, int C, long S, int G, int act, float eps, long long* n) {
  *n = 0;
  if (B < 0 || C < 0 || S < 0 || G <= 0 || act < 0 || act > 2 || !(eps >= 0.0f)) return PDR_EINVAL;
  if (C > 0 && C < G) return PDR_EINVAL;               // Cn == 0: nothing would be normalised
  if (B == 0 || C == 0 || S == 0) return PDR_OK;
  constexpr long long lim = 1ll << 31;
  if (S >= lim) return PDR_EUNSUPPORTED;
  long long p = static_cast<long long>(B) * C;         // every factor >= 1: a product at or above 2^31 stays there
  if (p >= lim) return PDR_EUNSUPPORTED;
  p *= S;
  if (p >= lim) return PDR_EUNSUPPORTED;
  *n = p;
  return PDR_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // NULL counts as aligned

unsigned chunks_of(long S) {
  const long n = (S + kRowChunk - 1) / kRowChunk;
  return static_cast<unsigned>(n > kMaxGridY ? kMaxGridY : n);
}

#define PDR_GN_BY_ACT(V, CALL)   \
  if (act == 0) CALL(V, 0);      \
  else if (act == 1) CALL(V, 1); \
  else CALL(V, 2)
#define PDR_GN_BY_FAMILY(CALL)  \
  if (p.vec) {                  \
    PDR_GN_BY_ACT(4, CALL);     \
  } else {                      \
    PDR_GN_BY_ACT(1, CALL);     \
  }

// both forward entries: add == residual == NULL launches the kernels pdr_group_norm_act always launched
int forward(const float* x, const float* gamma, const float* beta, const float* add, const float* residual, int B,
            int C, long S, int G, float eps, int act, float* y, float* mean, float* rstd, void* workspace,
            pdr_stream_t stream) {
  long long n;
  const int rc = check_sizes(B, C, S, G, act, eps, &n);
  if (rc != PDR_OK || n == 0) return rc;
  if (!x || !y || !workspace || (gamma == nullptr) != (beta == nullptr)) return PDR_EINVAL;
  const Plan p = plan_of(C, S, G, aligned16(x) && aligned16(y) && aligned16(residual));
  const int Cn = p.Cg * G, P = static_cast<int>(p.P);
  const long m = p.Cg * S;
  double* part = static_cast<double*>(workspace);
  hipStream_t st = pdr::as_stream(stream);
  const dim3 gs(static_cast<unsigned>(B) * G, static_cast<unsigned>(P)), ga(static_cast<unsigned>(B) * C, chunks_of(S));
  if (p.vec)
    hipLaunchKernelGGL(gn_stats_kernel<4>, gs, dim3(256), 0, st, x, C, S, G, p.Cg, m, p.E, part);
  else
    hipLaunchKernelGGL(gn_stats_kernel<1>, gs, dim3(256), 0, st, x, C, S, G, p.Cg, m, p.E, part);
#define PDR_GN_APPLY(V, A)                                                                                         \
  hipLaunchKernelGGL((gn_apply_kernel<V, A, false>), ga, dim3(256), 0, st, x, gamma, beta, part, C, S, G, p.Cg, Cn, P, \
                     eps, add, residual, y, mean, rstd)
#define PDR_GN_APPLY_ADD(V, A)                                                                                    \
  hipLaunchKernelGGL((gn_apply_kernel<V, A, true>), ga, dim3(256), 0, st, x, gamma, beta, part, C, S, G, p.Cg, Cn, P, \
                     eps, add, residual, y, mean, rstd)
  if (add || residual) {
    PDR_GN_BY_FAMILY(PDR_GN_APPLY_ADD)
  } else {
    PDR_GN_BY_FAMILY(PDR_GN_APPLY)
  }
#undef PDR_GN_APPLY
#undef PDR_GN_APPLY_ADD
  return pdr::check_launch();
}

// both backward entries: grad_add == NULL launches the kernels pdr_group_norm_act_grad always launched
int backward(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
             const float* grad_y, int B, int C, long S, int G, int act, float* grad_x, float* grad_gamma,
             float* grad_beta, float* grad_add, void* workspace, pdr_stream_t stream) {
  long long n;
  const int rc = check_sizes(B, C, S, G, act, 0.0f, &n);
  if (rc != PDR_OK || n == 0) return rc;
  if (!x || !mean || !rstd || !grad_y || !workspace || (gamma == nullptr) != (beta == nullptr)) return PDR_EINVAL;
  if (!gamma && (grad_gamma || grad_beta)) return PDR_EINVAL;
  if (!grad_x && !grad_gamma && !grad_beta && !grad_add) return PDR_EINVAL;
  const Plan p = plan_of(C, S, G, aligned16(x) && aligned16(grad_y) && aligned16(grad_x));
  const int Cn = p.Cg * G;
  double* rows = static_cast<double*>(workspace);
  hipStream_t st = pdr::as_stream(stream);
  const dim3 gr(static_cast<unsigned>(B) * C), ga(static_cast<unsigned>(B) * C, chunks_of(S));
#define PDR_GN_ROWS(V, A)                                                                                          \
  hipLaunchKernelGGL((gn_rows_kernel<V, A, false>), gr, dim3(256), 0, st, x, gamma, beta, mean, rstd, grad_y, C, S, G, \
                     p.Cg, Cn, rows, grad_add)
#define PDR_GN_ROWS_GE(V, A)                                                                                      \
  hipLaunchKernelGGL((gn_rows_kernel<V, A, true>), gr, dim3(256), 0, st, x, gamma, beta, mean, rstd, grad_y, C, S, G, \
                     p.Cg, Cn, rows, grad_add)
  if (grad_add) {
    PDR_GN_BY_FAMILY(PDR_GN_ROWS_GE)
  } else {
    PDR_GN_BY_FAMILY(PDR_GN_ROWS)
  }
#undef PDR_GN_ROWS
#undef PDR_GN_ROWS_GE
  if (grad_x) {
#define PDR_GN_DX(V, A)                                                                                              \
  hipLaunchKernelGGL((gn_dx_kernel<V, A>), ga, dim3(256), 0, st, x, gamma, beta, mean, rstd, grad_y, rows, C, S, G, \
                     p.Cg, Cn, grad_x)
    PDR_GN_BY_FAMILY(PDR_GN_DX)
#undef PDR_GN_DX
  }
  if (grad_gamma || grad_beta)
    hipLaunchKernelGGL(gn_dparam_kernel, dim3((Cn + 255) / 256), dim3(256), 0, st, rows, B, C, Cn, grad_gamma,
                       grad_beta);
  return pdr::check_launch();
}

}  // namespace

extern "C" size_t pdr_group_norm_act_workspace_bytes(int B, int C, long S, int G) {
  if (B <= 0 || C <= 0 || S <= 0 || G <= 0 || C < G) return 0;
  const Plan p = plan_of(C, S, G, true);
  const size_t fwd = static_cast<size_t>(B) * G * p.P, bwd = static_cast<size_t>(B) * C;
  return (fwd > bwd ? fwd : bwd) * 2 * sizeof(double);
}

extern "C" int pdr_group_norm_act_plan(int C, long S, int G, int aligned16, long out[4]) {
  if (C <= 0 || S <= 0 || G <= 0 || C < G || !out) return PDR_EINVAL;
  if (S >= (1ll << 31) || static_cast<long long>(C) * S >= (1ll << 31)) return PDR_EUNSUPPORTED;
  const Plan p = plan_of(C, S, G, aligned16 != 0);
  out[0] = p.vec;
  out[1] = p.P;
  out[2] = p.E;
  out[3] = p.Cg;
  return PDR_OK;
}

extern "C" int pdr_group_norm_act(const float* x, const float* gamma, const float* beta, int B, int C, long S, int G,
                                  float eps, int act, float* y, float* mean, float* rstd, void* workspace,
                                  pdr_stream_t stream) {
  return forward(x, gamma, beta, nullptr, nullptr, B, C, S, G, eps, act, y, mean, rstd, workspace, stream);
}

extern "C" int pdr_group_norm_act_add(const float* x, const float* gamma, const float* beta, const float* add,
                                      const float* residual, int B, int C, long S, int G, float eps, int act, float* y,
                                      float* mean, float* rstd, void* workspace, pdr_stream_t stream) {
  return forward(x, gamma, beta, add, residual, B, C, S, G, eps, act, y, mean, rstd, workspace, stream);
}

extern "C" int pdr_group_norm_act_grad(const float* x, const float* gamma, const float* beta, const float* mean,
                                       const float* rstd, const float* grad_y, int B, int C, long S, int G, int act,
                                       float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                                       pdr_stream_t stream) {
  return backward(x, gamma, beta, mean, rstd, grad_y, B, C, S, G, act, grad_x, grad_gamma, grad_beta, nullptr,
                  workspace, stream);
}

extern "C" int pdr_group_norm_act_add_grad(const float* x, const float* gamma, const float* beta, const float* mean,
                                           const float* rstd, const float* grad_y, int B, int C, long S, int G,
                                           int act, float* grad_x, float* grad_gamma, float* grad_beta,
                                           float* grad_add, void* workspace, pdr_stream_t stream) {
  return backward(x, gamma, beta, mean, rstd, grad_y, B, C, S, G, act, grad_x, grad_gamma, grad_beta, grad_add,
                  workspace, stream);
}
