// relu_group_norm_conv.hip -- a whole link of AttentionModule's score head on the TRAINABLE path
// (pointnet2_ops/attention.py::_act_norm_conv: [ReLU, MyGroupNorm, Conv2d 1x1] over cat([q over K, k], 1)) as one
// differentiable op whose GEMM normalises its operand as it loads it: the normalised tensor (B, C, N, K), the largest
// of the block, is never written, never read back and never saved.  The fp32 GEMM family of the trainable path:
//   pdr_relu_group_norm_conv_cf              out = W xn + bias                 (forward, three launches)
//   pdr_relu_group_norm_conv_cf_grad_input   gxn = W^T grad_out                (one launch, no prologue)
//   pdr_relu_group_norm_conv_cf_grad_weight  grad_W = grad_out xn^T, grad_bias (up to four launches)
// q, k, gamma, beta, C = C1 + C2, S = N K, Cn, Cg and the virtual tensor x are those of relu_group_norm.hip; the
// statistics kernel, the fold of a slab's partials and the element chain are the SAME code (relu_group_norm.h), so
//   xn[b, c, n, j] = exactly the value pdr_relu_group_norm_cf writes to y, and mean / rstd have its bits.
// W (Cout, C) row-major (the Conv2d weight viewed 2-D), bias (Cout) or NULL, out (B, Cout, N, K) dense.
//
// OPERATION CHAIN, -ffp-contract=off.
//   forward     acc = +0;  for c = 0 .. C - 1 ascending: acc = fma(W[o, c], xn[b, c, n, j], acc);
//               out[b, o, n, j] = bias ? fl(acc + bias[o]) : acc
//   grad_input  acc = +0;  for o = 0 .. Cout - 1 ascending: acc = fma(W[o, c], grad_out[b, o, n, j], acc);
//               gxn[b, c, n, j] = acc                  (what pdr_relu_group_norm_cf_grad takes as grad_y)
//   Both are what v_mfma_f32_32x32x2_f32 computes when its k index walks the contraction in order: a k-ordered fmaf
//   chain, one rounding per product (fused_layer.hip relies on the same).  The contraction goes through LDS in chunks of
//   16 that CONTINUE the accumulators: the chain is never split.  An odd contraction length is filled by one product
//   (-0) x (+0) = -0, and acc + (-0) = acc for every acc, NaN and -0 included.
//   grad_weight xn is recomputed from q, k and the SAVED mean / rstd (the forward's bits).  The S positions of a cloud
//               are cut into R = ceil(S / L) ranges of L positions (L from S alone: a multiple of 32, at least 1024,
//               R <= 16; the plan reports it).  A workgroup owns one (cloud, range) and a tile of grad_W; it
//               accumulates grad_out[b, o, s] xn[b, c, s] over its range in one MFMA chain (ascending s, from +0) and
//               writes the fp32 partial to the workspace.  The fold adds the B R partials of an element in DOUBLE in
//               ascending (b, range) order and rounds once.
//               grad_bias[o]: the positions of a (b, o, range) are summed in double (thread t of 256 takes positions
//               t, t + 256, .. ascending, then block_sum2), the B R partials in double in ascending (b, range) order,
//               rounded once.
//   The order is a function of (C1, C2, N, K, Cout) and the kernel family only; no atomics.
//
// KERNEL SHAPE.  rgc_gemm_kernel: a workgroup (4 waves) takes one cloud, 128 positions and TM in {32, 64, 128} output
// rows (the plan reports TM; wave tiles 1x1, 2x1, 2x2 MFMA tiles of 32 x 32).  Positions are the MFMA's column index:
// stores of a register are 128 contiguous bytes.  Per chunk of 16 contraction indices the raw operand (16-byte loads
// in the vector family; a q row reads one float per query) is fetched into registers while the previous chunk's MFMAs
// run, taken through the Row chain on its way into LDS (k-major: Xs[c][s], Ws[c][o]), and read back one dword per
// lane and MFMA (ds_read_b32 is serviced per half-wave: a k-major row of 32 consecutive dwords has no conflict).
// The per-channel (mean, rstd, gamma, beta) of the cloud sit in LDS (16 KiB at C = 1024).  Output rows beyond one TM
// are further workgroups (grid y) that read the operand again -- through L2; see DESIGN 7a.11 "left open".
// rgc_wgrad_kernel: tiles of 64 x 64 or 128 x 128 (Cout x C), chunks of 32 positions, both operands transposed on the
// way into LDS (row stride TO + 1: conflict-free both ways).
// Two families as relu_group_norm.hip: vector (K % 4 == 0 and the big input tensors 16-byte aligned) and scalar.
//
// VALIDATION ORDER (on the host, before any launch), relu_group_norm.hip's with the extensions:
//   1. B, C1, N or K negative, C2 < 1, G < 1, Cout < 1 (forward: eps negative or NaN): PDR_EINVAL
//   2. C1 + C2 < G: PDR_EINVAL
//   3. B N K == 0: PDR_OK, nothing launched, no pointer looked at
//   4. B C N K >= 2^31, B Cout N K >= 2^31, B C >= 2^24, C > 1024, Cout > 1024 or B > 4095: PDR_EUNSUPPORTED
//   5. pointers: NULL k / W / out / mean / rstd / workspace, C1 > 0 with q NULL, exactly one of gamma / beta NULL
//      (grad_weight: NULL grad_out, or grad_W and grad_bias both NULL): PDR_EINVAL
// grad_input takes (C, Cout) only: B, N, K negative or C, Cout < 1: PDR_EINVAL; empty: PDR_OK; the limits of 4;
// NULL W / grad_out / grad_xn: PDR_EINVAL.
#include "pdr_common.h"
#include "relu_group_norm.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKC = 16;            // contraction indices per LDS chunk of the GEMM
constexpr int kTS = 128;           // positions per workgroup of the GEMM
constexpr int kKS = 32;            // positions per LDS chunk of the weight gradient
constexpr long kChainMin = 1024;   // shortest weight-gradient chain, positions
constexpr long kRangesMax = 16;    // most ranges per cloud
constexpr int kMaxC = 1024, kMaxCout = 1024, kMaxB = 4095;

struct ConvPlan {
  Plan st;       // the statistics plan
  int TM;        // output rows per workgroup of the forward GEMM
  long L, R;     // positions per weight-gradient chain, ranges per cloud
  int TW;        // weight-gradient tile (Cout and C)
};

int tile_rows(int M) { return M <= 32 ? 32 : (M <= 64 ? 64 : 128); }

ConvPlan conv_plan_of(int C, long S, int K, int G, int Cout, bool aligned) {
  ConvPlan p;
  p.st = plan_of(C, S, K, G, aligned);
  p.TM = tile_rows(Cout);
  long L = (S + kRangesMax - 1) / kRangesMax;
  L = (L + 31) / 32 * 32;
  p.L = L < kChainMin ? kChainMin : L;
  p.R = S > 0 ? (S + p.L - 1) / p.L : 1;
  p.TW = (C > 64 && Cout > 64) ? 128 : 64;
  return p;
}

// where the virtual normalised operand comes from
struct XnSrc {
  const float* q;
  const float* k;
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* rstd;
  int C1, C2, N, K, G, Cg, Cn;
};

// (mean, rstd, gamma, beta) of channels [c0, c0 + n) of cloud b to LDS; a pass-through channel is (0, 1, 1, 0)
__device__ __forceinline__ void stage_rows(float4* rp, const XnSrc& x, size_t b, int c0, int n) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const int c = c0 + i;
    const Row r = row_of(nullptr, false, x.gamma, x.beta, x.mean, x.rstd, b, c, x.G, x.Cg, c < x.C1 + x.C2 ? x.Cn : 0);
    rp[i] = make_float4(r.mean, r.rstd, r.gamma, r.beta);
  }
}

__device__ __forceinline__ float xn_of(const float4 p, bool norm, float raw) {
  Row r;
  r.src = nullptr, r.is_q = false, r.norm = norm;
  r.mean = p.x, r.rstd = p.y, r.gamma = p.z, r.beta = p.w;
  return y_of(r, relu_of(raw));
}

// ---- out[b, m, s] = sum_kk A[m, kk] X[b, kk, s] (+ bias[m]), the contraction ascending ----------------------------------
// MODE 0: forward.  A = W (M = Cout, Kd = C, kk contiguous), X = xn through the Row chain.
// MODE 1: input gradient.  A = W^T (M = C, Kd = Cout, m contiguous), X = grad_out as it is.
template <int V, int MODE, int WM, int RT, int CT>
__global__ __launch_bounds__(256) void rgc_gemm_kernel(const float* __restrict__ A, int M, int Kd, XnSrc xs,
                                                       const float* __restrict__ X, const float* __restrict__ bias,
                                                       long S, float* __restrict__ out) {
  constexpr int WSN = 4 / WM;                 // waves along the positions
  constexpr int TM = WM * RT * 32;
  static_assert(WSN * CT * 32 == kTS, "position tile");
  constexpr int WPT = TM * kKC / 256;         // weight values per thread and chunk
  constexpr int XPT = kKC * kTS / 256;        // operand values per thread and chunk
  __shared__ float Ws[kKC][TM + 1];
  __shared__ __attribute__((aligned(16))) float Xs[kKC][kTS];
  __shared__ float4 rp[MODE == 0 ? kMaxC : 1];

  const int t = threadIdx.x;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int il = lane & 31, hi = lane >> 5;
  const int wm = wave % WM, wsn = wave / WM;
  const long s0 = static_cast<long>(blockIdx.x) * kTS;
  const int m0 = blockIdx.y * TM;
  const size_t b = blockIdx.z;
  const long ld_a = MODE == 0 ? Kd : M;       // row length of W as stored

  if constexpr (MODE == 0) stage_rows(rp, xs, b, 0, Kd);

  float xr[XPT], wr[WPT];
  // the raw values of chunk c0 into registers
  auto fetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < XPT / V; ++i) {
      const int e = t + 256 * i;
      const int cl = e / (kTS / V), sl = (e % (kTS / V)) * V;
      const int c = c0 + cl;
      const long s = s0 + sl;
      Pack<V> p;
#pragma unroll
      for (int j = 0; j < V; ++j) p.v[j] = 0.0f;
      if (c < Kd && s < S) {                  // V == 4: S is a multiple of 4, the four are inside or outside together
        if (MODE == 0) {
          if (c < xs.C1) {
            const float v = xs.q[(b * xs.C1 + c) * static_cast<size_t>(xs.N) + static_cast<unsigned>(s) / static_cast<unsigned>(xs.K)];
#pragma unroll
            for (int j = 0; j < V; ++j) p.v[j] = v;
          } else {
            p.load(xs.k + (b * xs.C2 + (c - xs.C1)) * static_cast<size_t>(S) + s);
          }
        } else {
          p.load(X + (b * Kd + c) * static_cast<size_t>(S) + s);
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) xr[V * i + j] = p.v[j];
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int e = t + 256 * i;
      const int kl = MODE == 0 ? e % kKC : e / TM, ml = MODE == 0 ? e / kKC : e % TM;
      const int m = m0 + ml, kk = c0 + kl;
      const bool ok = m < M && kk < Kd;
      const long at = MODE == 0 ? static_cast<long>(m) * ld_a + kk : static_cast<long>(kk) * ld_a + m;
      wr[i] = ok ? A[ok ? at : 0] : -0.0f;    // the fill: (-0) x (+0) = -0 leaves every accumulator as it is
    }
  };
  // registers to LDS, the operand through the Row chain
  auto commit = [&](int c0) {
#pragma unroll
    for (int i = 0; i < XPT / V; ++i) {
      const int e = t + 256 * i;
      const int cl = e / (kTS / V), sl = (e % (kTS / V)) * V;
      const int c = c0 + cl;
      const bool ok = c < Kd && s0 + sl < S;
      Pack<V> p;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float v = xr[V * i + j];
        if (MODE == 0) v = xn_of(rp[ok ? c : 0], c < xs.Cn, v);
        p.v[j] = ok ? v : 0.0f;
      }
      p.store(&Xs[cl][sl]);
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int e = t + 256 * i;
      const int kl = MODE == 0 ? e % kKC : e / TM, ml = MODE == 0 ? e / kKC : e % TM;
      Ws[kl][ml] = wr[i];
    }
  };

  f32x16 acc[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  fetch(0);
  for (int c0 = 0; c0 < Kd; c0 += kKC) {
    __syncthreads();                          // the previous chunk's MFMAs have read LDS (first trip: rp is staged)
    commit(c0);
    __syncthreads();
    if (c0 + kKC < Kd) fetch(c0 + kKC);       // in flight during the MFMAs below
    const int left = Kd - c0;
    const int ksteps = ((left < kKC ? left : kKC) + 1) >> 1;
    for (int kk = 0; kk < ksteps; ++kk) {
      float a[RT], x[CT];
#pragma unroll
      for (int i = 0; i < RT; ++i) a[i] = Ws[2 * kk + hi][(wm * RT + i) * 32 + il];
#pragma unroll
      for (int j = 0; j < CT; ++j) x[j] = Xs[2 * kk + hi][(wsn * CT + j) * 32 + il];
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], x[j], acc[i][j], 0, 0, 0);
    }
  }

  // C / D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const long s = s0 + (wsn * CT + j) * 32 + il;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wm * RT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (m < M && s < S) {
          const float v = acc[i][j][r];
          out[(b * M + m) * static_cast<size_t>(S) + s] = bias ? v + bias[m] : v;
        }
      }
    }
}

// mean / rstd (B, G) from the statistics partials: the arithmetic of rgn_apply_kernel, once per slab
__global__ __launch_bounds__(256) void rgc_mean_rstd_kernel(const double* __restrict__ part, int slabs, int P1, double m,
                                                            float eps, float* __restrict__ mean,
                                                            float* __restrict__ rstd) {
  const int slab = blockIdx.x * 256 + threadIdx.x;
  if (slab >= slabs) return;
  float mu, rs;
  slab_mean_rstd(part + static_cast<size_t>(slab) * P1 * 2, P1, m, eps, &mu, &rs);
  mean[slab] = mu;
  rstd[slab] = rs;
}

// ---- weight gradient: part[b R + r][o][c] = sum over the range's positions of grad_out[b, o, s] xn[b, c, s] ----------------
template <int V, int RT, int CT>
__global__ __launch_bounds__(256) void rgc_wgrad_kernel(XnSrc xs, const float* __restrict__ go, int Cout, long S, long L,
                                                        int R, float* __restrict__ part) {
  constexpr int TO = 2 * RT * 32, TC = 2 * CT * 32;
  constexpr int GPT = TO * kKS / 256, XPT = TC * kKS / 256;
  __shared__ float Gs[kKS][TO + 1];
  __shared__ float Xs[kKS][TC + 1];
  __shared__ float4 rp[TC];

  const int t = threadIdx.x;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int il = lane & 31, hi = lane >> 5;
  const int wo = wave & 1, wc = wave >> 1;
  const int C = xs.C1 + xs.C2;
  const int c0 = blockIdx.x * TC, o0 = blockIdx.y * TO;
  const size_t b = blockIdx.z / R;
  const long rg = blockIdx.z % R;
  const long p_lo = rg * L, p_hi = p_lo + L < S ? p_lo + L : S;

  stage_rows(rp, xs, b, c0, TC);

  float gr[GPT], xr[XPT];
  auto fetch = [&](long p0) {
#pragma unroll
    for (int i = 0; i < GPT / V; ++i) {
      const int e = t + 256 * i;
      const int sl = (e % (kKS / V)) * V, ol = e / (kKS / V);
      const int o = o0 + ol;
      const long s = p0 + sl;
      Pack<V> p;
#pragma unroll
      for (int j = 0; j < V; ++j) p.v[j] = 0.0f;
      if (o < Cout && s < p_hi) p.load(go + (b * Cout + o) * static_cast<size_t>(S) + s);
#pragma unroll
      for (int j = 0; j < V; ++j) gr[V * i + j] = p.v[j];
    }
#pragma unroll
    for (int i = 0; i < XPT / V; ++i) {
      const int e = t + 256 * i;
      const int sl = (e % (kKS / V)) * V, cl = e / (kKS / V);
      const int c = c0 + cl;
      const long s = p0 + sl;
      Pack<V> p;
#pragma unroll
      for (int j = 0; j < V; ++j) p.v[j] = 0.0f;
      if (c < C && s < p_hi) {
        if (c < xs.C1) {
          const float v = xs.q[(b * xs.C1 + c) * static_cast<size_t>(xs.N) + static_cast<unsigned>(s) / static_cast<unsigned>(xs.K)];
#pragma unroll
          for (int j = 0; j < V; ++j) p.v[j] = v;
        } else {
          p.load(xs.k + (b * xs.C2 + (c - xs.C1)) * static_cast<size_t>(S) + s);
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) xr[V * i + j] = p.v[j];
    }
  };
  auto commit = [&](long p0) {
#pragma unroll
    for (int i = 0; i < GPT / V; ++i) {
      const int e = t + 256 * i;
      const int sl = (e % (kKS / V)) * V, ol = e / (kKS / V);
#pragma unroll
      for (int j = 0; j < V; ++j) Gs[sl + j][ol] = gr[V * i + j];     // a value outside the problem was fetched as 0
    }
#pragma unroll
    for (int i = 0; i < XPT / V; ++i) {
      const int e = t + 256 * i;
      const int sl = (e % (kKS / V)) * V, cl = e / (kKS / V);
      const int c = c0 + cl;
      const bool ok = c < C && p0 + sl < p_hi;
#pragma unroll
      for (int j = 0; j < V; ++j) Xs[sl + j][cl] = ok ? xn_of(rp[cl], c < xs.Cn, xr[V * i + j]) : 0.0f;
    }
  };

  f32x16 acc[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  fetch(p_lo);
  for (long p0 = p_lo; p0 < p_hi; p0 += kKS) {
    __syncthreads();
    commit(p0);
    __syncthreads();
    if (p0 + kKS < p_hi) fetch(p0 + kKS);
    const long left = p_hi - p0;
    const int ksteps = static_cast<int>(((left < kKS ? left : kKS) + 1) >> 1);
    for (int kk = 0; kk < ksteps; ++kk) {
      float a[RT], x[CT];
#pragma unroll
      for (int i = 0; i < RT; ++i) a[i] = Gs[2 * kk + hi][(wo * RT + i) * 32 + il];
#pragma unroll
      for (int j = 0; j < CT; ++j) x[j] = Xs[2 * kk + hi][(wc * CT + j) * 32 + il];
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], x[j], acc[i][j], 0, 0, 0);
    }
  }

  float* dst = part + static_cast<size_t>(blockIdx.z) * Cout * C;
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int c = c0 + (wc * CT + j) * 32 + il;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + (wo * RT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (o < Cout && c < C) dst[static_cast<size_t>(o) * C + c] = acc[i][j][r];
      }
    }
}

// bpart[b R + r][o] = the double sum of grad_out[b, o, range r]
__global__ __launch_bounds__(256) void rgc_bias_part_kernel(const float* __restrict__ go, int Cout, long S, long L, int R,
                                                            double* __restrict__ bpart) {
  const size_t row = blockIdx.x;              // b Cout + o
  const size_t b = row / Cout;
  const int o = static_cast<int>(row % Cout);
  const long p_lo = static_cast<long>(blockIdx.y) * L, p_hi = p_lo + L < S ? p_lo + L : S;
  const float* g = go + row * static_cast<size_t>(S);
  double a = 0.0, unused = 0.0;
  for (long s = p_lo + threadIdx.x; s < p_hi; s += 256) a += static_cast<double>(g[s]);
  block_sum2(a, unused);
  if (threadIdx.x == 0) bpart[(b * R + blockIdx.y) * Cout + o] = a;
}

// out[i] = float(sum over the BR partials of element i, ascending, in double)
template <typename T>
__global__ __launch_bounds__(256) void rgc_fold_kernel(const T* __restrict__ part, int BR, long n,
                                                       float* __restrict__ out) {
  const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int r = 0; r < BR; ++r) a += static_cast<double>(part[static_cast<size_t>(r) * n + i]);
  out[i] = static_cast<float>(a);
}

// ---- host ----------------------------------------------------------------------------------------------------------
// steps 1-4 of the header's validation order; *n = B C N K on PDR_OK (0: nothing to do)
int conv_check_sizes(int B, int C1, int C2, int N, int K, int G, int Cout, float eps, long long* n) {
  const int rc = check_sizes(B, C1, C2, N, K, G, eps, n);
  if (rc == PDR_EINVAL) return rc;
  if (Cout < 1) {
    *n = 0;
    return PDR_EINVAL;
  }
  if (rc != PDR_OK || *n == 0) return rc;
  const long long C = static_cast<long long>(C1) + C2;
  if (static_cast<long long>(B) * Cout * N * K >= (1ll << 31) || C > kMaxC || Cout > kMaxCout || B > kMaxB) {
    *n = 0;
    return PDR_EUNSUPPORTED;
  }
  return PDR_OK;
}

size_t wgrad_part_bytes(int B, long R, int C, int Cout) {
  const size_t n = static_cast<size_t>(B) * R * Cout * C * sizeof(float);
  return (n + 7) / 8 * 8;
}

template <int V, int MODE>
void launch_gemm(int TM, dim3 grid, hipStream_t st, const float* A, int M, int Kd, const XnSrc& xs, const float* X,
                 const float* bias, long S, float* out) {
  if (TM == 32)
    hipLaunchKernelGGL((rgc_gemm_kernel<V, MODE, 1, 1, 1>), grid, dim3(256), 0, st, A, M, Kd, xs, X, bias, S, out);
  else if (TM == 64)
    hipLaunchKernelGGL((rgc_gemm_kernel<V, MODE, 1, 2, 1>), grid, dim3(256), 0, st, A, M, Kd, xs, X, bias, S, out);
  else
    hipLaunchKernelGGL((rgc_gemm_kernel<V, MODE, 2, 2, 2>), grid, dim3(256), 0, st, A, M, Kd, xs, X, bias, S, out);
}

}  // namespace

extern "C" size_t pdr_relu_group_norm_conv_cf_workspace_bytes(int B, int C1, int C2, int N, int K, int G, int Cout) {
  long long n;
  if (conv_check_sizes(B, C1, C2, N, K, G, Cout, 0.0f, &n) != PDR_OK || n == 0) return 0;
  const int C = C1 + C2;
  const ConvPlan p = conv_plan_of(C, static_cast<long>(N) * K, K, G, Cout, true);
  const size_t fwd = static_cast<size_t>(B) * G * (p.st.P + 1) * 2 * sizeof(double);
  const size_t bwd = wgrad_part_bytes(B, p.R, C, Cout) + static_cast<size_t>(B) * p.R * Cout * sizeof(double);
  return fwd > bwd ? fwd : bwd;
}

extern "C" int pdr_relu_group_norm_conv_cf_plan(int C1, int C2, int N, int K, int G, int Cout, int aligned16,
                                                long out[8]) {
  if (C1 < 0 || C2 < 1 || N < 1 || K < 1 || G < 1 || Cout < 1 || !out) return PDR_EINVAL;
  long long n;
  const int rc = conv_check_sizes(1, C1, C2, N, K, G, Cout, 0.0f, &n);
  if (rc != PDR_OK) return rc;
  const ConvPlan p = conv_plan_of(C1 + C2, static_cast<long>(N) * K, K, G, Cout, aligned16 != 0);
  out[0] = p.st.vec;
  out[1] = p.st.P;
  out[2] = p.st.E;
  out[3] = p.st.Cg;
  out[4] = kTS;
  out[5] = p.L;
  out[6] = p.R;
  out[7] = p.TM;
  return PDR_OK;
}

extern "C" int pdr_relu_group_norm_conv_cf(const float* q, const float* k, const float* gamma, const float* beta,
                                           const float* W, const float* bias, int B, int C1, int C2, int N, int K,
                                           int G, int Cout, float eps, float* out, float* mean, float* rstd,
                                           void* workspace, pdr_stream_t stream) {
  long long n;
  const int rc = conv_check_sizes(B, C1, C2, N, K, G, Cout, eps, &n);
  if (rc != PDR_OK || n == 0) return rc;
  if (!k || (C1 > 0 && !q) || !W || !out || !mean || !rstd || !workspace || (gamma == nullptr) != (beta == nullptr))
    return PDR_EINVAL;
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const ConvPlan p = conv_plan_of(C, S, K, G, Cout, aligned16(k));
  const int Cn = p.st.Cg * G, P1 = static_cast<int>(p.st.P) + 1;
  double* part = static_cast<double*>(workspace);
  hipStream_t st = pdr::as_stream(stream);
  const dim3 gs(static_cast<unsigned>(B) * G, static_cast<unsigned>(P1));
  if (p.st.vec)
    hipLaunchKernelGGL(rgn_stats_kernel<4>, gs, dim3(256), 0, st, q, k, C1, C2, N, K, G, p.st.Cg, p.st.E, part);
  else
    hipLaunchKernelGGL(rgn_stats_kernel<1>, gs, dim3(256), 0, st, q, k, C1, C2, N, K, G, p.st.Cg, p.st.E, part);
  hipLaunchKernelGGL(rgc_mean_rstd_kernel, dim3(pdr::blocks_for(static_cast<long>(B) * G)), dim3(256), 0, st, part,
                     B * G, P1, static_cast<double>(p.st.Cg) * static_cast<double>(S), eps, mean, rstd);
  const XnSrc xs = {q, k, gamma, beta, mean, rstd, C1, C2, N, K, G, p.st.Cg, Cn};
  const dim3 grid(static_cast<unsigned>((S + kTS - 1) / kTS), static_cast<unsigned>((Cout + p.TM - 1) / p.TM),
                  static_cast<unsigned>(B));
  if (p.st.vec)
    launch_gemm<4, 0>(p.TM, grid, st, W, Cout, C, xs, nullptr, bias, S, out);
  else
    launch_gemm<1, 0>(p.TM, grid, st, W, Cout, C, xs, nullptr, bias, S, out);
  return pdr::check_launch();
}

extern "C" int pdr_relu_group_norm_conv_cf_grad_input(const float* W, const float* grad_out, int B, int C, int N, int K,
                                                      int Cout, float* grad_xn, pdr_stream_t stream) {
  if (B < 0 || N < 0 || K < 0 || C < 1 || Cout < 1) return PDR_EINVAL;
  if (B == 0 || N == 0 || K == 0) return PDR_OK;
  const long long S = static_cast<long long>(N) * K, lim = 1ll << 31;
  if (C > kMaxC || Cout > kMaxCout || B > kMaxB || S >= lim || B * S * C >= lim || B * S * Cout >= lim)
    return PDR_EUNSUPPORTED;
  if (!W || !grad_out || !grad_xn) return PDR_EINVAL;
  const bool vec = K % 4 == 0 && aligned16(grad_out);
  const int TM = tile_rows(C);
  const XnSrc xs = {};
  const dim3 grid(static_cast<unsigned>((S + kTS - 1) / kTS), static_cast<unsigned>((C + TM - 1) / TM),
                  static_cast<unsigned>(B));
  hipStream_t st = pdr::as_stream(stream);
  if (vec)
    launch_gemm<4, 1>(TM, grid, st, W, C, Cout, xs, grad_out, nullptr, static_cast<long>(S), grad_xn);
  else
    launch_gemm<1, 1>(TM, grid, st, W, C, Cout, xs, grad_out, nullptr, static_cast<long>(S), grad_xn);
  return pdr::check_launch();
}

extern "C" int pdr_relu_group_norm_conv_cf_grad_weight(const float* q, const float* k, const float* gamma,
                                                       const float* beta, const float* mean, const float* rstd,
                                                       const float* grad_out, int B, int C1, int C2, int N, int K,
                                                       int G, int Cout, float* grad_W, float* grad_bias,
                                                       void* workspace, pdr_stream_t stream) {
  long long n;
  const int rc = conv_check_sizes(B, C1, C2, N, K, G, Cout, 0.0f, &n);
  if (rc != PDR_OK || n == 0) return rc;
  if (!k || (C1 > 0 && !q) || !mean || !rstd || !grad_out || !workspace || (gamma == nullptr) != (beta == nullptr))
    return PDR_EINVAL;
  if (!grad_W && !grad_bias) return PDR_EINVAL;
  const int C = C1 + C2;
  const long S = static_cast<long>(N) * K;
  const ConvPlan p = conv_plan_of(C, S, K, G, Cout, aligned16(k) && aligned16(grad_out));
  const int Cn = p.st.Cg * G, R = static_cast<int>(p.R), BR = B * R;
  float* part = static_cast<float*>(workspace);
  double* bpart = reinterpret_cast<double*>(static_cast<char*>(workspace) + wgrad_part_bytes(B, p.R, C, Cout));
  hipStream_t st = pdr::as_stream(stream);
  if (grad_W) {
    const XnSrc xs = {q, k, gamma, beta, mean, rstd, C1, C2, N, K, G, p.st.Cg, Cn};
    const dim3 grid(static_cast<unsigned>((C + p.TW - 1) / p.TW), static_cast<unsigned>((Cout + p.TW - 1) / p.TW),
                    static_cast<unsigned>(BR));
    if (p.st.vec) {
      if (p.TW == 128)
        hipLaunchKernelGGL((rgc_wgrad_kernel<4, 2, 2>), grid, dim3(256), 0, st, xs, grad_out, Cout, S, p.L, R, part);
      else
        hipLaunchKernelGGL((rgc_wgrad_kernel<4, 1, 1>), grid, dim3(256), 0, st, xs, grad_out, Cout, S, p.L, R, part);
    } else {
      if (p.TW == 128)
        hipLaunchKernelGGL((rgc_wgrad_kernel<1, 2, 2>), grid, dim3(256), 0, st, xs, grad_out, Cout, S, p.L, R, part);
      else
        hipLaunchKernelGGL((rgc_wgrad_kernel<1, 1, 1>), grid, dim3(256), 0, st, xs, grad_out, Cout, S, p.L, R, part);
    }
    const long nw = static_cast<long>(Cout) * C;
    hipLaunchKernelGGL(rgc_fold_kernel<float>, dim3(pdr::blocks_for(nw)), dim3(256), 0, st, part, BR, nw, grad_W);
  }
  if (grad_bias) {
    hipLaunchKernelGGL(rgc_bias_part_kernel, dim3(static_cast<unsigned>(B) * Cout, static_cast<unsigned>(R)), dim3(256),
                       0, st, grad_out, Cout, S, p.L, R, bpart);
    hipLaunchKernelGGL(rgc_fold_kernel<double>, dim3(pdr::blocks_for(Cout)), dim3(256), 0, st, bpart, BR,
                       static_cast<long>(Cout), grad_bias);
  }
  return pdr::check_launch();
}
