// fused_gather.hip -- channel-last neighbourhood assembly and attention pooling.
//
// group_build : QueryAndGroup.forward (reference pointnet2_utils.py:332-438) in one pass:
//               G[b,j,k,:] = [ feats[b, idx[b,j,k], :] | rel xyz | abs xyz | centre xyz ]
//               with the subset=False patch (no neighbour -> the query itself, zero feature).
//               The reference runs group_points twice + 3 elementwise passes + 2 torch.cat over
//               the K-times expanded tensor.
// knn_build   : group_knn (pointnet2_utils.py:487-514):
//               G[b,i,k,:] = [ feats_y[b, idx, :] | d2 | w | nn_abs | nn_rel | x ],
//               w = (1/(d2+1e-8)) / sum_k (1/(d2_k+1e-8))   (SQUARED distances, as the reference).
// attention_pool : tail of AttentionModule.forward (attention.py:83-96): count mask (-1e9),
//               softmax over the K neighbours, value = relu(GN(conv(h))) folded as scale/shift,
//               weighted sum -> (B*npoint, D).
// All tensors channel-LAST: a position's channels are contiguous, so neighbour feature rows are
// read as whole contiguous segments and every store is coalesced.
#include <type_traits>

#include "pdr_common.h"

namespace {

// LPP lanes per position p = (b, j, k) (16 / 32 / 64 by row width); the lanes of a group stride over
// the output channels, so the neighbour's feature row is read as one contiguous segment and the
// output row is written contiguously; index / count are loaded once per group.
template <int LPP>
__global__ __launch_bounds__(256) void group_build_kernel(
    const float* __restrict__ feats, int Cs, int n, const float* __restrict__ xyz,
    const float* __restrict__ new_xyz, const int* __restrict__ idx, const int* __restrict__ counts,
    int m, int K, int patch_empty, int with_abs, int with_centre, long npos, int Cout, int ldo,
    float* __restrict__ out) {
  constexpr int GPB = 256 / LPP;           // position groups per workgroup
  const int lane = threadIdx.x % LPP;
  const long g0 = static_cast<long>(blockIdx.x) * GPB + threadIdx.x / LPP;
  const long ngroups = static_cast<long>(gridDim.x) * GPB;
  for (long p = g0; p < npos; p += ngroups) {
    const long bj = p / K;                 // b * m + j
    const int b = static_cast<int>(bj / m);
    const int a = idx[p];
    const bool empty = patch_empty && counts[bj] <= 0;
    const float* frow = feats + (static_cast<long>(b) * n + a) * Cs;
    float* orow = out + p * ldo;
    for (int c = lane; c < Cs; c += LPP) orow[c] = empty ? 0.0f : frow[c];
    for (int c = Cout + lane; c < ldo; c += LPP) orow[c] = 0.0f;   // padding columns, whatever LPP and ldo - Cout
    if (lane < Cout - Cs) {
      const int g = lane;                  // 0..2 rel, 3..5 abs|centre, 6..8 centre
      const int d = g % 3;
      const float ctr = new_xyz[bj * 3 + d];
      const float ab = empty ? ctr : xyz[(static_cast<long>(b) * n + a) * 3 + d];
      const int kind = g / 3;
      float v;
      if (kind == 0) v = ab - ctr;
      else if (kind == 1) v = with_abs ? ab : ctr;
      else v = ctr;
      orow[Cs + g] = v;
    }
  }
}

template <int LPP>
__global__ __launch_bounds__(256) void knn_build_kernel(
    const float* __restrict__ feats_y, int C, int n2, const float* __restrict__ x,
    const float* __restrict__ y, const long long* __restrict__ idx, const float* __restrict__ d2,
    int n1, int K, long npos, int Cout, int ldo, float* __restrict__ out) {
  constexpr int GPB = 256 / LPP;
  const int lane = threadIdx.x % LPP;
  const long g0 = static_cast<long>(blockIdx.x) * GPB + threadIdx.x / LPP;
  const long ngroups = static_cast<long>(gridDim.x) * GPB;
  for (long p = g0; p < npos; p += ngroups) {
    const long bi = p / K;                 // (b, i)
    const int b = static_cast<int>(bi / n1);
    const long a = idx[p];
    const float* frow = feats_y + (static_cast<long>(b) * n2 + a) * C;
    float* orow = out + p * ldo;
    for (int c = lane; c < C; c += LPP) orow[c] = frow[c];
    for (int c = Cout + lane; c < ldo; c += LPP) orow[c] = 0.0f;   // padding columns, whatever LPP and ldo - Cout
    if (lane < 11) {
      float v;
      if (lane == 0) {
        v = d2[p];
      } else if (lane == 1) {
        float norm = 0.0f;
        for (int k = 0; k < K; ++k) norm += 1.0f / (d2[bi * K + k] + 1e-8f);
        v = (1.0f / (d2[p] + 1e-8f)) / norm;
      } else {
        const int g = lane - 2;            // 0..2 nn_abs, 3..5 nn_rel, 6..8 x
        const int d = g % 3;
        const float xq = x[bi * 3 + d];
        const float ab = y[(static_cast<long>(b) * n2 + a) * 3 + d];
        v = g < 3 ? ab : (g < 6 ? ab - xq : xq);
      }
      orow[C + lane] = v;
    }
  }
}

// One lane per (query row, 4 channels): scores and values are streamed ONCE as float4 with an
// online softmax (running max m, normaliser l, accumulator rescaled by exp(m_old - m_new)); the
// result equals softmax-then-sum up to fp32 rounding.
__global__ __launch_bounds__(256) void attention_pool_kernel(
    const float* __restrict__ scores, int lds, const float* __restrict__ values, int ldv,
    const float* __restrict__ vscale, const float* __restrict__ vshift, int v_relu,
    const int* __restrict__ counts, int K, int D, int npoint, long rows, float* __restrict__ out) {
  const int D4 = D >> 2;
  const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= rows * D4) return;
  const long row = t / D4;
  const int d = static_cast<int>(t - row * D4) * 4;
  const int b = static_cast<int>(row / npoint);
  int cnt = K;
  if (counts) {
    cnt = counts[row];
    cnt = cnt < 1 ? 1 : cnt;             // attention.py:85 clamp(min=1)
  }
  float4 sc = make_float4(1, 1, 1, 1), sh = make_float4(0, 0, 0, 0);
  if (vscale) sc = *reinterpret_cast<const float4*>(vscale + static_cast<long>(b) * D + d);
  if (vshift) sh = *reinterpret_cast<const float4*>(vshift + static_cast<long>(b) * D + d);
  const float lo = v_relu ? 0.0f : -__builtin_inff();
  const float* s = scores + row * K * lds + d;
  const float* v = values + row * K * ldv + d;
  float m[4], l[4], acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { m[j] = -__builtin_inff(); l[j] = 0.0f; acc[j] = 0.0f; }
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    float4 sk = *reinterpret_cast<const float4*>(s + static_cast<long>(k) * lds);
    const float4 vk = *reinterpret_cast<const float4*>(v + static_cast<long>(k) * ldv);
    if (k >= cnt) sk = make_float4(-1e9f, -1e9f, -1e9f, -1e9f);   // masked slots: exactly -1e9
    const float se[4] = {sk.x, sk.y, sk.z, sk.w};
    const float ve[4] = {vk.x, vk.y, vk.z, vk.w};
    const float sce[4] = {sc.x, sc.y, sc.z, sc.w}, she[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // softmax in the base-2 domain: exp(s - m) = exp2((s - m) log2 e) with the hardware v_exp_f32
      // (two instructions per exponential instead of the ~10 of expf: the kernel was VALU-, not
      // HBM-limited).  Arguments are <= 0, results in (0, 1]; the rounding of s * log2(e) perturbs
      // the weights by <= |s - m| * 2^-23 relative.
      const float s2 = se[j] * 1.44269504088896340736f;
      const float mn = fmaxf(m[j], s2);
      const float corr = __builtin_amdgcn_exp2f(m[j] - mn);   // exp2(-inf) = 0 on the first slot
      const float w = __builtin_amdgcn_exp2f(s2 - mn);
      const float val = fmaxf(__builtin_fmaf(ve[j], sce[j], she[j]), lo);
      l[j] = __builtin_fmaf(l[j], corr, w);
      acc[j] = __builtin_fmaf(acc[j], corr, val * w);
      m[j] = mn;
    }
  }
  *reinterpret_cast<float4*>(out + row * D + d) =
      make_float4(acc[0] / l[0], acc[1] / l[1], acc[2] / l[2], acc[3] / l[3]);
}

// Wave-per-query form for K * D / 4 <= 64 * NL float4 per query with D / 4 a power of two <= 64: a
// query's K x D block of scores (and of values) is CONTIGUOUS, so the wave reads it with NL fully
// coalesced 1-KiB loads each (lane -> (k = e / D4, c4 = e % D4), e = i * 64 + lane) instead of 8
// separate 128-byte pieces per instruction.  All scores sit in registers: exact two-pass softmax
// (max, then exp2 / sums), folded across the lanes that share a channel group with xor shuffles.
template <int NL>
__global__ __launch_bounds__(256) void attention_pool_wave_kernel(
    const float* __restrict__ scores, const float* __restrict__ values, const float* __restrict__ vscale,
    const float* __restrict__ vshift, int v_relu, const int* __restrict__ counts, int K, int D, int npoint,
    long rows, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int D4 = D >> 2;
  const int sh = __builtin_ctz(D4);
  const int c4 = lane & (D4 - 1);
  const int k0 = lane >> sh;                 // first neighbour of this lane
  const int kstep = 64 >> sh;                // neighbours covered per load
  const float lo = v_relu ? 0.0f : -__builtin_inff();
  const long nwaves = static_cast<long>(gridDim.x) * 4;
  for (long row = static_cast<long>(blockIdx.x) * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const int b = static_cast<int>(row / npoint);
    int cnt = K;
    if (counts) {
      cnt = counts[row];
      cnt = cnt < 1 ? 1 : cnt;               // attention.py:85 clamp(min=1)
    }
    const float4* s4 = reinterpret_cast<const float4*>(scores + row * K * D) + lane;
    const float4* v4 = reinterpret_cast<const float4*>(values + row * K * D) + lane;
    float4 sv[NL], vv[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const bool ok = k0 + i * kstep < K;
      sv[i] = ok ? s4[i * 64] : make_float4(0, 0, 0, 0);
      vv[i] = ok ? v4[i * 64] : make_float4(0, 0, 0, 0);
    }
    float4 sc = make_float4(1, 1, 1, 1), shv = make_float4(0, 0, 0, 0);
    if (vscale) sc = *reinterpret_cast<const float4*>(vscale + static_cast<long>(b) * D + 4 * c4);
    if (vshift) shv = *reinterpret_cast<const float4*>(vshift + static_cast<long>(b) * D + 4 * c4);
    float m[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    float se[NL][4];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int k = k0 + i * kstep;
      const float e[4] = {sv[i].x, sv[i].y, sv[i].z, sv[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // slots beyond K do not exist (-inf: weight 0); masked slots are exactly -1e9 as in the reference
        se[i][j] = k >= K ? -__builtin_inff() : (k >= cnt ? -1e9f : e[j]) * 1.44269504088896340736f;
        m[j] = fmaxf(m[j], se[i][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      for (int off = D4; off < 64; off <<= 1) m[j] = fmaxf(m[j], __shfl_xor(m[j], off, 64));
    float l[4] = {0, 0, 0, 0}, acc[4] = {0, 0, 0, 0};
    const float sce[4] = {sc.x, sc.y, sc.z, sc.w}, she[4] = {shv.x, shv.y, shv.z, shv.w};
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const float ve[4] = {vv[i].x, vv[i].y, vv[i].z, vv[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float w = __builtin_amdgcn_exp2f(se[i][j] - m[j]);
        const float val = fmaxf(__builtin_fmaf(ve[j], sce[j], she[j]), lo);
        l[j] += w;
        acc[j] = __builtin_fmaf(val, w, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      for (int off = D4; off < 64; off <<= 1) {
        l[j] += __shfl_xor(l[j], off, 64);
        acc[j] += __shfl_xor(acc[j], off, 64);
      }
    if (lane < D4)
      *reinterpret_cast<float4*>(out + row * D + 4 * c4) =
          make_float4(acc[0] / l[0], acc[1] / l[1], acc[2] / l[2], acc[3] / l[3]);
  }
}

// rows of a channel-last matrix: out[b, j, :] = src[b, idx[b,j], :]
__global__ __launch_bounds__(256) void gather_rows_cl_kernel(const float* __restrict__ src, int n,
                                                             int C, const int* __restrict__ idx,
                                                             int m, long total,
                                                             float* __restrict__ out) {
  const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const long bj = e / C;
  const int c = static_cast<int>(e - bj * C);
  const int b = static_cast<int>(bj / m);
  out[e] = src[(static_cast<long>(b) * n + idx[bj]) * C + c];
}

// out[b, j, :] = [src0[b, idx[b,j], :] | src1[b, idx[b,j], :]]: gather of the rows of a concatenation that is never
// materialised (torch.cat + gather_rows as one launch)
__global__ __launch_bounds__(256) void gather_rows2_cl_kernel(const float* __restrict__ src0, int C0,
                                                              const float* __restrict__ src1, int C1, int n,
                                                              const int* __restrict__ idx, int m, long total,
                                                              float* __restrict__ out) {
  const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const int C = C0 + C1;
  const long bj = e / C;
  const int c = static_cast<int>(e - bj * C);
  const int b = static_cast<int>(bj / m);
  const long row = static_cast<long>(b) * n + idx[bj];
  out[e] = c < C0 ? src0[row * C0 + c] : src1[row * C1 + (c - C0)];
}

// rows of C floats -> rows of ldo >= C floats, zero-filled behind column C (F.pad as ONE launch: torch pads with a
// fill plus a strided copy)
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ src, int C, int ldo, long total,
                                                       float* __restrict__ out) {
  const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const long r = e / ldo;
  const int c = static_cast<int>(e - r * ldo);
  out[e] = c < C ? src[r * C + c] : 0.0f;
}

}  // namespace

extern "C" int pdr_group_build(const float* feats, int Cs, const float* xyz, const float* new_xyz,
                               const int* idx, const int* counts, int B, int n, int m, int K,
                               int patch_empty, int with_abs, int with_centre, float* out, int ldo,
                               pdr_stream_t stream) {
  if (B < 0 || n <= 0 || m < 0 || K <= 0 || Cs < 0) return PDR_EINVAL;
  if (B == 0 || m == 0) return PDR_OK;
  if (!xyz || !new_xyz || !idx || !out || (Cs > 0 && !feats) || (patch_empty && !counts))
    return PDR_EINVAL;
  const int Cout = Cs + 3 + (with_abs ? 3 : 0) + (with_centre ? 3 : 0);
  if (ldo < Cout || ldo - Cout > 8) return PDR_EINVAL;
  const long npos = static_cast<long>(B) * m * K;
  // channel order after the features: rel | (abs) | (centre); the kernel's `kind` 1 slot is abs
  // when with_abs else centre
  hipStream_t s = pdr::as_stream(stream);
#define PDR_GB(LPP)                                                                                 \
  do {                                                                                              \
    const long nblk = (npos + 256 / LPP - 1) / (256 / LPP);                                         \
    hipLaunchKernelGGL(group_build_kernel<LPP>, dim3(static_cast<unsigned>(nblk < 32768 ? nblk : 32768)), \
                       dim3(256), 0, s, feats, Cs, n, xyz, new_xyz, idx, counts, m, K, patch_empty, \
                       with_abs, with_centre, npos, Cout, ldo, out);                                \
  } while (0)
  if (Cout <= 16) PDR_GB(16);
  else if (Cout <= 48) PDR_GB(32);
  else PDR_GB(64);
#undef PDR_GB
  return pdr::check_launch();
}

extern "C" int pdr_knn_build(const float* feats_y, int C, const float* x, const float* y,
                             const long long* idx, const float* d2, int B, int n1, int n2, int K,
                             float* out, int ldo, pdr_stream_t stream) {
  if (B < 0 || n1 < 0 || n2 <= 0 || K <= 0 || C < 0) return PDR_EINVAL;
  if (B == 0 || n1 == 0) return PDR_OK;
  if (!x || !y || !idx || !d2 || !out || (C > 0 && !feats_y)) return PDR_EINVAL;
  const int Cout = C + 11;
  if (ldo < Cout || ldo - Cout > 8) return PDR_EINVAL;
  const long npos = static_cast<long>(B) * n1 * K;
  hipStream_t s = pdr::as_stream(stream);
#define PDR_KB(LPP)                                                                                 \
  do {                                                                                              \
    const long nblk = (npos + 256 / LPP - 1) / (256 / LPP);                                         \
    hipLaunchKernelGGL(knn_build_kernel<LPP>, dim3(static_cast<unsigned>(nblk < 32768 ? nblk : 32768)), \
                       dim3(256), 0, s, feats_y, C, n2, x, y, idx, d2, n1, K, npos, Cout, ldo, out); \
  } while (0)
  if (Cout <= 16) PDR_KB(16);
  else if (Cout <= 48) PDR_KB(32);
  else PDR_KB(64);
#undef PDR_KB
  return pdr::check_launch();
}

extern "C" int pdr_attention_pool(const float* scores, int lds, const float* values, int ldv,
                                  const float* vscale, const float* vshift, int v_relu,
                                  const int* counts, int B, int npoint, int K, int D, float* out,
                                  pdr_stream_t stream) {
  if (B < 0 || npoint < 0 || K <= 0 || D <= 0) return PDR_EINVAL;
  if (B == 0 || npoint == 0) return PDR_OK;
  if (!scores || !values || !out) return PDR_EINVAL;
  const long rows = static_cast<long>(B) * npoint;
  if (D % 4 || lds % 4 || ldv % 4) return PDR_EUNSUPPORTED;
  {
    // wave-per-query form: dense rows (ld == D), D / 4 a power of two <= 64, <= 8 loads per lane
    const int D4 = D / 4;
    const long per_query = static_cast<long>(K) * D4;
    const int kstep = D4 <= 64 ? 64 / (D4 ? D4 : 1) : 0;
    if (lds == D && ldv == D && D4 <= 64 && (D4 & (D4 - 1)) == 0 && per_query <= 512 && kstep > 0) {
      const int nl = static_cast<int>((K + kstep - 1) / kstep);
      long blocks = (rows + 3) / 4;
      if (blocks > 256L * 16) blocks = 256L * 16;
      const dim3 grid(static_cast<unsigned>(blocks));
      hipStream_t st = pdr::as_stream(stream);
#define PDR_AP(NL)                                                                                      \
  hipLaunchKernelGGL(attention_pool_wave_kernel<NL>, grid, dim3(256), 0, st, scores, values, vscale,    \
                     vshift, v_relu, counts, K, D, npoint, rows, out)
      if (nl <= 1) PDR_AP(1);
      else if (nl <= 2) PDR_AP(2);
      else if (nl <= 4) PDR_AP(4);
      else PDR_AP(8);
#undef PDR_AP
      return pdr::check_launch();
    }
  }
  hipLaunchKernelGGL(attention_pool_kernel, dim3(pdr::blocks_for(rows * (D / 4))), dim3(256), 0,
                     pdr::as_stream(stream), scores, lds, values, ldv, vscale, vshift, v_relu, counts, K,
                     D, npoint, rows, out);
  return pdr::check_launch();
}

extern "C" int pdr_gather_rows2(const float* src0, int C0, const float* src1, int C1, const int* idx, int B, int n,
                                int m, float* out, pdr_stream_t stream) {
  if (B < 0 || n <= 0 || C0 <= 0 || C1 <= 0 || m < 0) return PDR_EINVAL;
  if (B == 0 || m == 0) return PDR_OK;
  if (!src0 || !src1 || !idx || !out) return PDR_EINVAL;
  const long total = static_cast<long>(B) * m * (C0 + C1);
  hipLaunchKernelGGL(gather_rows2_cl_kernel, dim3(pdr::blocks_for(total)), dim3(256), 0, pdr::as_stream(stream), src0,
                     C0, src1, C1, n, idx, m, total, out);
  return pdr::check_launch();
}

extern "C" int pdr_pad_rows(const float* src, long rows, int C, float* out, int ldo, pdr_stream_t stream) {
  if (rows < 0 || C <= 0 || ldo < C) return PDR_EINVAL;
  if (rows == 0) return PDR_OK;
  if (!src || !out) return PDR_EINVAL;
  const long total = rows * ldo;
  hipLaunchKernelGGL(pad_rows_kernel, dim3(pdr::blocks_for(total)), dim3(256), 0, pdr::as_stream(stream), src, C, ldo,
                     total, out);
  return pdr::check_launch();
}

extern "C" int pdr_gather_rows(const float* src, const int* idx, int B, int n, int C, int m,
                               float* out, pdr_stream_t stream) {
  if (B < 0 || n <= 0 || C <= 0 || m < 0) return PDR_EINVAL;
  if (B == 0 || m == 0) return PDR_OK;
  if (!src || !idx || !out) return PDR_EINVAL;
  const long total = static_cast<long>(B) * m * C;
  hipLaunchKernelGGL(gather_rows_cl_kernel, dim3(pdr::blocks_for(total)), dim3(256), 0,
                     pdr::as_stream(stream), src, n, C, idx, m, total, out);
  return pdr::check_launch();
}

// ---------------------------------------------------------------------------------------------
// gather_add / gather_moments: first 1x1 conv of a grouped block WITHOUT the grouped tensor.
//
// The grouped input of QueryAndGroup / group_knn is a gather of per-point rows plus per-query
// terms, and the conv is linear, so for position p = (b, j, k) with neighbour a = idx[p]:
//     conv([feat[a] | xyz[a]-c_j | xyz[a] | c_j]) = U[b,a,:] + V[b,j,:]
//         U = [feat | xyz] . [W_f ; W_rel + W_abs]   (one row per SOURCE point,  n  rows)
//         V = c . (W_ctr - W_rel) + bias             (one row per QUERY,         m  rows)
//     kNN: conv([feat[a] | d2 | w | y[a] | y[a]-x_i | x_i]) = U[b,a,:] + V[b,i,:] + d2 r1 + w r2
// U and V are small GEMMs over n and m rows (fused_layer); this kernel produces the (m K)-row
// output with one gather + add per element and the GroupNorm moments of the result.  It removes
// 2 P Cin Cout flops (37 % of a reverse step's GEMM work) and the P x Cin grouped tensor.
// Empty balls (subset=False): the reference substitutes the query itself with a zero feature:
// Y = V0[b,j,:] = c . (W_abs + W_ctr) + bias.
//
// One workgroup = 128 positions; each wave owns 32 CONSECUTIVE positions whose neighbour indices /
// empty flags / per-position scalars are fetched with one coalesced load and then broadcast from
// registers.  A row is covered by LPR lanes x float4 (LPR = 16 / 32 / 64 by output width), so a wave
// instruction moves 64 / LPR rows and narrow outputs keep every lane busy.  Every U / V / Y access is a
// contiguous row segment.
//
// ONE body serves every entry point.  It walks one or two column WINDOWS of the output: pdr_gather_add* the single
// window [0, Cout); pdr_gather_moments* -- the statistics-only pass of a virtual first conv -- the windows whose moments
// a GroupNorm reads, [first C1 | . | key C2] of [first C1 | residual Clast | key C2]: the residual window enters its
// consumer as a plain row-wise add, nobody reads its moments, so no lane gathers or reduces it.  The float4 pieces of the
// windows form ONE index space (piece q < w4a: window a, else window b), so a column pass has no idle range of lanes in
// its middle; the moments go to the columns' ORIGINAL places in `partial`, every other entry stays unwritten.
//
// A column's moments do not depend on the windows: LPR comes from the Cout thresholds (host) whatever is walked, so a
// column's rows are dealt to the same (wave, row sub-group), accumulated in the same order and folded through the same
// shuffle / LDS tree; only WHICH lane of a sub-group holds a column differs, which no sum depends on.
//
// The kernel is VALU-issue bound (PMC: 35 VALU instructions per 16-byte gather in its first form, waves issue-stalled
// 47 % of their cycles), so the per-row work is kept minimal: the query row V[i] is loaded once per iteration of rows
// that belong to one query (3 of 4 loads of the K = 8 form with 64 lanes per row, 31 of 32 of the K = 32 ball form), else
// its address is an add + shift when K is a power of two that divides the wave's 32 rows (every shipped config; the
// general form is a 64-bit division per row group); a row's index / kNN scalars are scalar registers where a wave
// instruction covers one row; the kNN terms and the empty-ball select exist only in the instantiations that have their
// inputs; the ReLU of the statistics is one v_max against a per-lane bound and runs only in a column pass that reaches
// relu_col0; addresses are 32-bit offsets.  Adds / FMAs are written as float pairs (v_pk_add_f32 / v_pk_fma_f32).
//
// YWIN instantiations (pdr_gather_add* with a Y) also WRITE the columns [yw.c0, yw.c1) of the walked rows, at column
// c - yw.c0 of Y, and allow partial == NULL (Y only: no accumulation, no fold, no barrier).  The flag is compile-time:
// the statistics-only instantiations are on the step's critical path and carry no pointer, branch or register for it.
//
// TWIN tiles (blockIdx.x >= tw.n_main; pdr_gather_*_tiles_twin): the same sum over the block's per-QUERY rows --
// neighbour = the query's first one (tw.idx0), K = 1 -- written whole to tw.Y (EVERY column: the per-query chain reads
// its residual columns), with the GroupNorm moments of the rows q >= wrow0[b] (the queries of the cloud's skipped tiles)
// times tw.wmul, on the windows' columns, in partial row b partial_tpb + tiles_per_batch + tile: what a separate K = 1
// launch + pdr_weighted_moments produced, in the launch that walks the tile subset.
typedef float pdr_f2 __attribute__((ext_vector_type(2)));

// How a wave walks its 32 rows with LPR lanes per row -- read by gather_tile AND by plan_gather, so that the plan's
// `shared` threshold cannot drift from the kernel's.  rpi: rows per wave instruction.  depth: row groups in flight per
// iteration -- the kernel is bound by the latency of its L2 gathers, so every wave keeps `depth` independent 16-byte U
// loads outstanding (4 measured against 2; the order of a column's sum does not depend on it; 8 for LPR 64 measured
// 0-10 % slower than 4: DESIGN.md 4.11).  shared_rows = depth x rpi rows per iteration: a power-of-two K >= that many
// rows takes the one-V-row-per-query walk (16 / 8 / 4 for LPR 16 / 32 / 64).
struct GatherWalk {
  int rpi, depth, shared_rows;
};
constexpr GatherWalk gather_walk(int lpr) {
  const int rpi = 64 / lpr;
  const int depth = 32 / rpi < 4 ? 32 / rpi : 4;
  return {rpi, depth, depth * rpi};
}

template <bool YWIN>
struct YWindow {};
template <>
struct YWindow<true> {
  float* Y;            // (B rows_per_batch, ld): columns [c0, c1) of the output, from column 0 on
  int ld, c0, c1;
};

template <bool YWIN>
YWindow<YWIN> y_window(float* Y, int ld, int c0, int c1) {
  if constexpr (YWIN) return {Y, ld, c0, c1};
  else return {};
}

template <int LPR, bool KPOW2, bool HAS_S, bool HAS_EM, bool TWIN, bool YWIN>
__device__ __forceinline__ void gather_tile(
    const float* __restrict__ U, int ldu, int n_src, const float* __restrict__ V, const float* __restrict__ V0, int ldv,
    const int* __restrict__ idx, const int* __restrict__ counts, const float* __restrict__ s1,
    const float* __restrict__ r1, const float* __restrict__ s2, const float* __restrict__ r2, int rows_per_batch_,
    int K_, int Cout, float* __restrict__ partial, int relu_col0, const pdr::MomentWindows& mw,
    const unsigned char* __restrict__ tile_valid, int partial_tpb, const pdr::GatherTwin& tw, const YWindow<YWIN>& yw,
    float (*red)[4 * LPR][2]) {
  static_assert(!(TWIN && YWIN), "a twin tile writes tw.Y whole, never a window");
  constexpr int TM = 128;
  constexpr int RPI = gather_walk(LPR).rpi;       // rows per wave instruction
  constexpr int DEPTH = gather_walk(LPR).depth;   // row groups in flight per iteration (gather_walk)
  constexpr int CW = 4 * LPR;              // columns covered per pass
  const int rows_per_batch = TWIN ? rows_per_batch_ / K_ : rows_per_batch_;
  const int K = TWIN ? 1 : K_;
  const int* __restrict__ idx_e = TWIN ? tw.idx0 : idx;
  // (the wave number as a scalar: what depends on it alone -- nrows, the loop over the rows -- stays in scalar registers)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane / LPR, cl = lane % LPR;
  // a per-row value held by lane `row` of the wave: with one row per wave instruction the row is uniform and the value
  // a scalar (v_readlane: no LDS round trip, and the row's address arithmetic leaves the vector ALU)
  auto row_value = [](int val, int row) {
    if constexpr (RPI == 1) return __builtin_amdgcn_readlane(val, __builtin_amdgcn_readfirstlane(row));
    else return __shfl(val, row, 64);
  };
  const int tpb = (rows_per_batch + TM - 1) / TM;
  const int n_main = tw.n_main > 0 ? tw.n_main : static_cast<int>(gridDim.x);
  const int bid = TWIN ? static_cast<int>(blockIdx.x) - n_main : pdr::xcd_contiguous(blockIdx.x, n_main);
  const int b = bid / tpb, tb = bid - b * tpb;
  // a tile subset (pdr_dedup_plan): the other tiles are neither read nor written
  if (!TWIN && tile_valid && !tile_valid[bid]) return;   // uniform
  const int tpb_main = (rows_per_batch_ + TM - 1) / TM;
  // the tile's partial row (twin tiles behind the cloud's main tiles)
  const long prow = static_cast<long>(b) * (partial_tpb > 0 ? partial_tpb : tpb) + (TWIN ? tpb_main : 0) + tb;
  const long row0 = static_cast<long>(b) * rows_per_batch + static_cast<long>(tb) * TM;
  const int nvalid = min(TM, rows_per_batch - tb * TM);
  // statistics: rows >= wlo of the tile count (twin: the queries behind the cloud's valid tiles)
  const int wlo = TWIN ? min(max(tw.wrow0[b] - tb * TM, 0), TM) : 0;   // uniform
  const float* Ub = U + static_cast<long>(b) * n_src * ldu;
  const int wr0 = wave * 32;
  const int myr = min(wr0 + (lane & 31), nvalid - 1);
  const long myp = row0 + myr;
  const int my_idx = idx_e[myp];
  const int my_empty = (HAS_EM && counts[myp / K] <= 0) ? 1 : 0;
  const float my_s1 = (HAS_S && s1) ? s1[myp] : 0.0f;
  const float my_s2 = (HAS_S && s2) ? s2[myp] : 0.0f;
  const int nrows = max(0, min(32, nvalid - wr0));   // uniform
  const int ksh = KPOW2 ? __builtin_ctz(K) : -1;          // KPOW2: K a power of two <= 32
  const long qbase = (row0 + wr0) / K;                     // exact when ksh >= 0 (row0 + wr0 is a multiple of K)
  const float* Vq = V + qbase * ldv;
  const long v0d = HAS_EM ? V0 - V : 0;                    // elements from V to V0 (same address space)
  // the walked columns as float4 pieces: [0, w4a) of window a, [w4a, w4) of window b (TWIN: every column)
  const int wa0 = TWIN ? 0 : mw.c0a, wb0 = TWIN ? 0 : mw.c0b;
  const int w4a = TWIN ? (Cout + 3) >> 2 : (mw.na + 3) >> 2;
  const int w4 = w4a + (TWIN ? 0 : (mw.nb + 3) >> 2);
  const int ea = mw.c0a + mw.na, eb = mw.c0b + mw.nb;     // window ends
  // (grid.y > 1, round 6: the column passes of a tile dealt to grid.y workgroups -- a launch of a few hundred tiles with
  // a wide output (the first conv of the 16- / 64-point levels: 128-512 tiles x 1,100 columns) was a serial walk of five
  // passes per wave on a half-empty chip)
  for (int p0 = static_cast<int>(blockIdx.y) * LPR; p0 < w4; p0 += LPR * static_cast<int>(gridDim.y)) {
    const int q = p0 + cl;
    const bool cok = q < w4;   // row widths are padded to a multiple of 4 in ldu / ldv / ldy
    const int c = cok ? (q >= w4a ? wb0 + 4 * (q - w4a) : wa0 + 4 * q) : 0;
    float4 q1 = make_float4(0, 0, 0, 0), q2 = make_float4(0, 0, 0, 0);
    if (HAS_S && cok && r1) q1 = *reinterpret_cast<const float4*>(r1 + c);
    if (HAS_S && cok && r2) q2 = *reinterpret_cast<const float4*>(r2 + c);
    // columns ascend with the piece number: the pass reaches relu_col0 iff its last piece does (uniform)
    const int ql = min(p0 + LPR, w4) - 1;
    const bool relu = (ql >= w4a ? wb0 + 4 * (ql - w4a) : wa0 + 4 * ql) + 3 >= relu_col0;
    float lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) lo[j] = (c + j >= relu_col0) ? 0.0f : -__builtin_inff();
    bool ywin = false;
    if constexpr (YWIN) ywin = c >= yw.c0 && c < yw.c1;
    pdr_f2 a1l = {0, 0}, a1h = {0, 0}, a2l = {0, 0}, a2h = {0, 0};
    // One query row for a whole iteration when its DEPTH x RPI rows cannot straddle two queries (K a power of two >=
    // that many rows; a wave's rows start on a multiple of K and nrows is one): V is loaded when r enters a new query
    // and the empty-ball select is a scalar branch.  Else (K = 1 twin tiles, small or odd K) a V row per row.  SHARED,
    // RELU and STATS (false: Y only) are compile-time so that each form is a loop of its own (uniform choice).
    auto walk_rows = [&](auto shared_tag, auto relu_tag, auto stats_tag) {
      constexpr bool SHARED = decltype(shared_tag)::value, RELU = decltype(relu_tag)::value;
      constexpr bool STATS = decltype(stats_tag)::value;
      float4 vq = make_float4(0, 0, 0, 0);
      int emq = 0;
      for (int r = 0; r < nrows; r += DEPTH * RPI) {
        float4 u[DEPTH], v[DEPTH];
        float t1[DEPTH], t2[DEPTH];
        int em[DEPTH], rr[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
          rr[k] = r + k * RPI + sub;                               // this lane's row (per sub-group)
          const int rc = min(rr[k], nrows - 1);
          const int a = row_value(my_idx, rc);
          if (HAS_S) {
            t1[k] = __int_as_float(row_value(__float_as_int(my_s1), rc));
            t2[k] = __int_as_float(row_value(__float_as_int(my_s2), rc));
          }
          u[k] = *reinterpret_cast<const float4*>(Ub + static_cast<unsigned>(a * ldu + c));
          if (!SHARED) {
            em[k] = HAS_EM ? row_value(my_empty, rc) : 0;
            const float* vp;
            if constexpr (KPOW2) vp = Vq + static_cast<unsigned>((rc >> ksh) * ldv + c);
            else vp = V + ((row0 + wr0 + rc) / K) * ldv + c;
            v[k] = *reinterpret_cast<const float4*>(vp + (em[k] ? v0d : 0));
          }
        }
        // (behind the U loads: the first one of an iteration waits for nothing that is still in flight)
        if constexpr (SHARED) if ((r & (K - 1)) == 0) {
          emq = HAS_EM ? row_value(my_empty, r) : 0;
          vq = *reinterpret_cast<const float4*>(Vq + static_cast<unsigned>((r >> ksh) * ldv + c) + (emq ? v0d : 0));
        }
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
          if (rr[k] < nrows && cok) {
            const float4 vv = SHARED ? vq : v[k];
            pdr_f2 yl = {vv.x, vv.y}, yh = {vv.z, vv.w};
            if (!HAS_EM || !(SHARED ? emq : em[k])) {
              yl = pdr_f2{u[k].x, u[k].y} + yl;
              yh = pdr_f2{u[k].z, u[k].w} + yh;
              if (HAS_S) {
                const pdr_f2 s1v = {t1[k], t1[k]}, s2v = {t2[k], t2[k]};
                yl = __builtin_elementwise_fma(s1v, pdr_f2{q1.x, q1.y}, yl);
                yh = __builtin_elementwise_fma(s1v, pdr_f2{q1.z, q1.w}, yh);
                yl = __builtin_elementwise_fma(s2v, pdr_f2{q2.x, q2.y}, yl);
                yh = __builtin_elementwise_fma(s2v, pdr_f2{q2.z, q2.w}, yh);
              }
            }
            if (TWIN)
              *reinterpret_cast<float4*>(tw.Y + (row0 + wr0 + rr[k]) * tw.ldy + c) = make_float4(yl.x, yl.y, yh.x, yh.y);
            if constexpr (YWIN) {
              if (ywin)
                *reinterpret_cast<float4*>(yw.Y + (row0 + wr0 + rr[k]) * yw.ld + (c - yw.c0)) =
                    make_float4(yl.x, yl.y, yh.x, yh.y);
            }
            if (STATS && (!TWIN || wr0 + rr[k] >= wlo)) {
              if (RELU) {
                const float e[4] = {yl.x, yl.y, yh.x, yh.y};
                float f[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  asm("v_max_f32 %0, %1, %2" : "=v"(f[j]) : "v"(e[j]), "v"(lo[j]));   // max(y, 0) or y (bound -inf)
                yl = pdr_f2{f[0], f[1]};
                yh = pdr_f2{f[2], f[3]};
              }
              a1l += yl;
              a1h += yh;
              a2l = __builtin_elementwise_fma(yl, yl, a2l);
              a2h = __builtin_elementwise_fma(yh, yh, a2h);
            }
          }
        }
      }
    };
    bool shared = false;                                           // uniform
    if constexpr (KPOW2 && !TWIN) shared = K >= gather_walk(LPR).shared_rows;
    if constexpr (YWIN) {
      if (!partial) {              // Y only: nothing is accumulated, folded or waited for (uniform: no barrier is missed)
        if (!shared) walk_rows(std::false_type{}, std::false_type{}, std::false_type{});
        if constexpr (KPOW2) if (shared) walk_rows(std::true_type{}, std::false_type{}, std::false_type{});
        continue;
      }
    }
    if constexpr (KPOW2 && !TWIN) {
      if (shared) {
        if (relu) walk_rows(std::true_type{}, std::true_type{}, std::true_type{});
        else walk_rows(std::true_type{}, std::false_type{}, std::true_type{});
      }
    }
    if (!shared) {
      if (relu) walk_rows(std::false_type{}, std::true_type{}, std::true_type{});
      else walk_rows(std::false_type{}, std::false_type{}, std::true_type{});
    }
    // fold the RPI row sub-groups (lanes with equal `cl`), then the 4 waves through LDS
    float a1[4] = {a1l.x, a1l.y, a1h.x, a1h.y}, a2[4] = {a2l.x, a2l.y, a2h.x, a2h.y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int off = LPR; off < 64; off <<= 1) {
        a1[j] += __shfl_xor(a1[j], off, 64);
        a2[j] += __shfl_xor(a2[j], off, 64);
      }
    }
    if (sub == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        red[wave][4 * cl + j][0] = a1[j];
        red[wave][4 * cl + j][1] = a2[j];
      }
    }
    __syncthreads();
    const int t = static_cast<int>(threadIdx.x);
    const int qq = p0 + (t >> 2);
    if (t < CW && qq < w4) {
      const int col = (qq >= w4a ? wb0 + 4 * (qq - w4a) : wa0 + 4 * qq) + (t & 3);
      // a window's last piece may reach past its end; a twin tile walked the columns between the windows too
      const bool keep = TWIN ? ((col >= mw.c0a && col < ea) || (col >= mw.c0b && col < eb)) : col < (qq >= w4a ? eb : ea);
      if (keep) {
        const float m1 = (red[0][t][0] + red[1][t][0]) + (red[2][t][0] + red[3][t][0]);
        const float m2 = (red[0][t][1] + red[1][t][1]) + (red[2][t][1] + red[3][t][1]);
        float* o = partial + (prow * Cout + col) * 2;
        o[0] = TWIN ? m1 * tw.wmul : m1;
        o[1] = TWIN ? m2 * tw.wmul : m2;
      }
    }
    __syncthreads();
  }
}

template <int LPR, bool KPOW2, bool HAS_S, bool HAS_EM, bool YWIN>
__global__ __launch_bounds__(256) void gather_kernel(
    const float* __restrict__ U, int ldu, int n_src, const float* __restrict__ V, const float* __restrict__ V0, int ldv,
    const int* __restrict__ idx, const int* __restrict__ counts, const float* __restrict__ s1,
    const float* __restrict__ r1, const float* __restrict__ s2, const float* __restrict__ r2, int rows_per_batch, int K,
    int Cout, float* __restrict__ partial, int relu_col0, pdr::MomentWindows mw,
    const unsigned char* __restrict__ tile_valid, int partial_tpb, pdr::GatherTwin tw, YWindow<YWIN> yw) {
  __shared__ float red[4][4 * LPR][2];
  if constexpr (!HAS_S) {                  // (twin tiles exist in the ball form only)
    if (tw.n_main > 0 && static_cast<int>(blockIdx.x) >= tw.n_main) {   // uniform
      gather_tile<LPR, KPOW2, false, HAS_EM, true, false>(U, ldu, n_src, V, V0, ldv, idx, counts, s1, r1, s2, r2,
                                                          rows_per_batch, K, Cout, partial, relu_col0, mw, tile_valid,
                                                          partial_tpb, tw, YWindow<false>{}, red);
      return;
    }
  }
  gather_tile<LPR, KPOW2, HAS_S, HAS_EM, false, YWIN>(U, ldu, n_src, V, V0, ldv, idx, counts, s1, r1, s2, r2, rows_per_batch,
                                                      K, Cout, partial, relu_col0, mw, tile_valid, partial_tpb, tw, yw, red);
}

// ---- the dispatch decision: ONE host function, read by gather_launch below and by pdr_gather_plan ---------------------
// What plan_gather reads of a call: its sizes, its windows and WHICH pointers are there (and whether they are 16-byte
// aligned) -- never what a pointer points to.
struct GatherCall {
  int B, n_src, rows_per_batch, K, Cout, ldu, ldv, ldy, ycol0, ycols;
  int win0_col0, win0_cols, win1_col0, win1_cols, partial_tpb, ldyd;
  bool required;                 // U, V and idx
  bool counts, V0, s1, r1, s2, r2, Y, partial, tile_valid;
  bool idx0, Yd, wrow0;          // the twin form's pointers
  bool aligned, Yd_aligned;      // U, V, V0, Y, r1, r2 (those present) / Yd
};

struct GatherPlan {
  int lpr;                       // lanes per row: 16 / 32 / 64; 0: an empty call (B = 0), nothing is launched
  bool kpow2, has_s, has_em, ywin;   // the instantiation gather_kernel<LPR, KPOW2, HAS_S, HAS_EM, YWIN>
  bool stats;                    // partial != NULL (false: the Y-only walk, no fold, no barrier)
  bool shared;                   // the main tiles walk one V row per query (kpow2 and K >= shared_rows)
  int shared_rows;               // gather_walk(lpr).shared_rows
  pdr::MomentWindows mw;         // the windows as walked
  int w4, passes;                // float4 pieces of the windows; column passes of lpr pieces
  int grid_x, grid_y;            // grid.y = passes when they are dealt to workgroups, else 1 (walked in the workgroup)
  int n_main, tpb;               // main tiles (B tpb) and per cloud
  int n_twin, twin_tpb;          // twin tiles (grid_x - n_main) and per cloud; 0 without the twin form
  int ycol0, y4;                 // the written window [ycol0, ycol0 + y4) (padded to float4); y4 = 0 without a Y
  bool tiles;                    // a tile subset is walked
};

// Every return code of pdr_gather_add* / pdr_gather_moments* that is decided behind their NULL checks of tile_valid /
// idx0, in the order the calls have always decided them.  The windows of pdr_gather_add* are the whole width
// (0, Cout, 0, 0).
static int plan_gather(const GatherCall& a, GatherPlan* p) {
  *p = GatherPlan{};
  if (!a.required || (!a.Y && !a.partial) || a.B < 0 || a.rows_per_batch <= 0 || a.K <= 0 || a.Cout <= 0 || a.n_src <= 0)
    return PDR_EINVAL;
  const int tpb = (a.rows_per_batch + 127) / 128;
  // (the entry points with a tile subset refuse these whatever B is: the twin form rows that are no whole queries, the
  // plain subset form a partial stride below the tiles of a cloud -- the twin form's stride is checked below)
  if (a.idx0 && (!a.tile_valid || a.rows_per_batch % a.K != 0)) return PDR_EINVAL;
  if (a.tile_valid && !a.idx0 && a.partial_tpb < tpb) return PDR_EINVAL;
  // windows: inside [0, Cout), ascending, disjoint
  if (a.win0_col0 < 0 || a.win0_cols <= 0 || a.win0_cols > a.Cout - a.win0_col0) return PDR_EINVAL;
  if (a.win1_cols < 0 ||
      (a.win1_cols > 0 && (a.win1_col0 < a.win0_col0 + a.win0_cols || a.win1_cols > a.Cout - a.win1_col0)))
    return PDR_EINVAL;
  if (a.B == 0) return PDR_OK;
  if (a.rows_per_batch % a.K != 0 || (a.counts && !a.V0) || (a.s1 && !a.r1) || (a.s2 && !a.r2)) return PDR_EINVAL;
  const int c4 = (a.Cout + 3) & ~3;
  const int ycols = a.ycols < 0 ? a.Cout - a.ycol0 : a.ycols;   // -1: every column from ycol0 on
  // the written window [ycol0, ycol0 + ycols) starts on a float4 boundary; Y holds it from column 0
  if (a.Y && (a.ycol0 < 0 || a.ycol0 % 4 || ycols <= 0 || a.ycol0 + ycols > a.Cout)) return PDR_EINVAL;
  const int y4 = (ycols + 3) & ~3;
  if (a.ldu % 4 || a.ldv % 4 || a.ldu < c4 || a.ldv < c4 || (a.Y && (a.ldy % 4 || a.ldy < y4))) return PDR_EINVAL;
  // rows are moved as float4: every base pointer (possibly offset to a column sub-range) 16-B aligned
  if (!a.aligned) return PDR_EINVAL;
  const bool has_s = a.s1 || a.s2;
  long nblocks = static_cast<long>(a.B) * tpb;
  p->n_main = static_cast<int>(nblocks);
  if (a.idx0) {
    // twin blocks: the per-query rows (rows_per_batch / K per cloud) behind the main tiles
    const int mq = a.rows_per_batch / a.K;
    if (!a.Yd || !a.wrow0 || !a.partial || has_s || a.ldyd % 4 || a.ldyd < c4 || !a.Yd_aligned ||
        a.partial_tpb < tpb + (mq + 127) / 128)
      return PDR_EINVAL;
    p->twin_tpb = (mq + 127) / 128;
    nblocks += static_cast<long>(a.B) * p->twin_tpb;
  }
  if (nblocks >= (1L << 31)) return PDR_EINVAL;
  // rows move as float4 pieces: a window starts on one (the caller keeps the whole width for the others)
  if (a.win0_col0 % 4 || (a.win1_cols > 0 && a.win1_col0 % 4)) return PDR_EUNSUPPORTED;
  p->mw = pdr::MomentWindows{a.win0_col0, a.win0_cols, a.win1_cols > 0 ? a.win1_col0 : a.win0_col0 + a.win0_cols,
                             a.win1_cols > 0 ? a.win1_cols : 0};
  // lanes per row from the FULL width, whatever is walked: what keeps the order of every column's sum
  p->lpr = a.Cout <= 64 ? 16 : (a.Cout <= 128 ? 32 : 64);
  p->kpow2 = (a.K & (a.K - 1)) == 0 && a.K <= 32;
  p->has_s = has_s, p->has_em = a.counts, p->ywin = a.Y, p->stats = a.partial, p->tiles = a.tile_valid;
  p->shared_rows = p->lpr == 16 ? gather_walk(16).shared_rows
                                : (p->lpr == 32 ? gather_walk(32).shared_rows : gather_walk(64).shared_rows);
  p->shared = p->kpow2 && a.K >= p->shared_rows;
  // column passes per workgroup: all of them, unless the launch has fewer tiles than the chip holds workgroups
  p->w4 = (p->mw.na + 3) / 4 + (p->mw.nb + 3) / 4;
  p->passes = (p->w4 + p->lpr - 1) / p->lpr;
  p->grid_x = static_cast<int>(nblocks);
  p->grid_y = (nblocks <= 1024 && p->passes > 1) ? p->passes : 1;
  p->tpb = tpb;
  p->n_twin = p->grid_x - p->n_main;
  p->ycol0 = a.Y ? a.ycol0 : 0;
  p->y4 = a.Y ? y4 : 0;
  return PDR_OK;
}

// The one launch path of pdr_gather_add* / pdr_gather_moments*: it launches what plan_gather names.
// Y (B*rows_per_batch, columns [ycol0, ycol0 + ycols) of Cout; ld ldy) = U[b, idx[p]] + V[p / K] (+ s1[p] r1 + s2[p] r2),
// empty balls -> V0; NULL: statistics only.  U (B, n_src, ldu), V / V0 (B*rows_per_batch/K, ldv); all leading dimensions
// multiples of 4, 16-B aligned.  partial: NULL (with a Y) or (B * ceil(rows_per_batch / 128), Cout, 2) moments as in
// pdr_fused_layer, written on the columns of the windows [win0_col0, + win0_cols) and, with win1_cols > 0,
// [win1_col0, + win1_cols): pdr_gather_add* passes the whole width.  Every return code is decided before the launch.
static int gather_launch(const float* U, int ldu, int n_src, const float* V, const float* V0, int ldv, const int* idx,
                         const int* counts, const float* s1, const float* r1, const float* s2, const float* r2, int B,
                         int rows_per_batch, int K, int Cout, float* Y, int ldy, float* partial, int relu_col0, int ycol0,
                         int ycols, int win0_col0, int win0_cols, int win1_col0, int win1_cols,
                         const unsigned char* tile_valid, int partial_tpb, pdr_stream_t stream,
                         const int* idx0 = nullptr, float* Yd = nullptr, int ldyd = 0, const int* wrow0 = nullptr,
                         float wmul = 1.0f) {
  auto al = [](const void* q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; };
  GatherCall a{};
  a.B = B, a.n_src = n_src, a.rows_per_batch = rows_per_batch, a.K = K, a.Cout = Cout, a.ldu = ldu, a.ldv = ldv;
  a.ldy = ldy, a.ycol0 = ycol0, a.ycols = ycols, a.win0_col0 = win0_col0, a.win0_cols = win0_cols;
  a.win1_col0 = win1_col0, a.win1_cols = win1_cols, a.partial_tpb = partial_tpb, a.ldyd = ldyd;
  a.required = U && V && idx;
  a.counts = counts, a.V0 = V0, a.s1 = s1, a.r1 = r1, a.s2 = s2, a.r2 = r2, a.Y = Y, a.partial = partial;
  a.tile_valid = tile_valid, a.idx0 = idx0, a.Yd = Yd, a.wrow0 = wrow0;
  a.aligned = al(U) && al(V) && al(V0) && al(Y) && al(r1) && al(r2);   // (a NULL pointer counts as aligned)
  a.Yd_aligned = al(Yd);
  GatherPlan p;
  const int rc = plan_gather(a, &p);
  if (rc != PDR_OK || p.lpr == 0) return rc;
  const pdr::GatherTwin tw{idx0, Yd, wrow0, ldyd, p.n_twin > 0 ? p.n_main : 0, wmul};
  const pdr::MomentWindows mw = p.mw;
  const dim3 grid(static_cast<unsigned>(p.grid_x), static_cast<unsigned>(p.grid_y));
  hipStream_t st = pdr::as_stream(stream);
#define PDR_G_Y(LPR, KP, HS, HE, YW)                                                                                  \
  hipLaunchKernelGGL((gather_kernel<LPR, KP, HS, HE, YW>), grid, dim3(256), 0, st, U, ldu, n_src, V, V0, ldv, idx,    \
                     counts, s1, r1, s2, r2, rows_per_batch, K, Cout, partial, relu_col0, mw, tile_valid, partial_tpb, \
                     tw, y_window<YW>(Y, ldy, p.ycol0, p.ycol0 + p.y4))
#define PDR_G_E(LPR, KP, HS, HE)              \
  do {                                        \
    if (p.ywin) PDR_G_Y(LPR, KP, HS, HE, true);    \
    else PDR_G_Y(LPR, KP, HS, HE, false);     \
  } while (0)
#define PDR_G_K(LPR, KP, HS)                  \
  do {                                        \
    if (p.has_em) PDR_G_E(LPR, KP, HS, true);   \
    else PDR_G_E(LPR, KP, HS, false);         \
  } while (0)
#define PDR_G(LPR)                                        \
  do {                                                    \
    if (p.kpow2 && p.has_s) PDR_G_K(LPR, true, true);     \
    else if (p.kpow2) PDR_G_K(LPR, true, false);          \
    else if (p.has_s) PDR_G_K(LPR, false, true);          \
    else PDR_G_K(LPR, false, false);                      \
  } while (0)
  if (p.lpr == 16) PDR_G(16);
  else if (p.lpr == 32) PDR_G(32);
  else PDR_G(64);
#undef PDR_G
#undef PDR_G_K
#undef PDR_G_E
#undef PDR_G_Y
  return pdr::check_launch();
}

// Host only: what a call with these sizes, windows and pointers would launch.  flags: PDR_GATHER_HAS_* of pdr_hip.h; a
// pointer that goes with a flagged one (V0 with counts, r1 / r2 with s1 / s2, Yd and wrow0 with idx0) and every
// required pointer count as given and aligned.
extern "C" int pdr_gather_plan(int B, int n_src, int rows_per_batch, int K, int Cout, int ldu, int ldv, int ldy,
                               int ycol0, int ycols, int win0_col0, int win0_cols, int win1_col0, int win1_cols,
                               int partial_tpb, int ldyd, unsigned flags, int out[24]) {
  if (!out || (flags & ~0x7fu)) return PDR_EINVAL;
  GatherCall a{};
  a.B = B, a.n_src = n_src, a.rows_per_batch = rows_per_batch, a.K = K, a.Cout = Cout, a.ldu = ldu, a.ldv = ldv;
  a.ldy = ldy, a.ycol0 = ycol0, a.ycols = ycols, a.win0_col0 = win0_col0, a.win0_cols = win0_cols;
  a.win1_col0 = win1_col0, a.win1_cols = win1_cols, a.partial_tpb = partial_tpb, a.ldyd = ldyd;
  a.required = a.aligned = a.Yd_aligned = true;
  a.counts = a.V0 = flags & PDR_GATHER_HAS_COUNTS;
  a.s1 = a.r1 = flags & PDR_GATHER_HAS_S1;
  a.s2 = a.r2 = flags & PDR_GATHER_HAS_S2;
  a.Y = flags & PDR_GATHER_HAS_Y, a.partial = flags & PDR_GATHER_HAS_PARTIAL;
  a.tile_valid = flags & PDR_GATHER_HAS_TILES;
  a.idx0 = a.Yd = a.wrow0 = flags & PDR_GATHER_HAS_TWIN;
  GatherPlan p;
  const int rc = plan_gather(a, &p);
  const int v[24] = {p.lpr, p.kpow2, p.has_s, p.has_em, p.ywin, p.stats, p.shared, p.shared_rows, p.mw.c0a, p.mw.na,
                     p.mw.c0b, p.mw.nb, p.w4, p.passes, p.grid_x, p.grid_y, p.n_main, p.n_twin, p.tpb, p.twin_tpb,
                     p.ycol0, p.y4, p.tiles, 0};
  for (int i = 0; i < 24; ++i) out[i] = rc == PDR_OK ? v[i] : 0;
  return rc;
}

extern "C" int pdr_gather_moments(const float* U, int ldu, int n_src, const float* V, const float* V0, int ldv,
                                  const int* idx, const int* counts, const float* s1, const float* r1, const float* s2,
                                  const float* r2, int B, int rows_per_batch, int K, int Cout, float* partial,
                                  int relu_col0, int win0_col0, int win0_cols, int win1_col0, int win1_cols,
                                  pdr_stream_t stream) {
  return gather_launch(U, ldu, n_src, V, V0, ldv, idx, counts, s1, r1, s2, r2, B, rows_per_batch, K, Cout, nullptr, 0,
                       partial, relu_col0, 0, -1, win0_col0, win0_cols, win1_col0, win1_cols, nullptr, 0, stream);
}

extern "C" int pdr_gather_moments_tiles(const float* U, int ldu, int n_src, const float* V, const float* V0, int ldv,
                                        const int* idx, const int* counts, const float* s1, const float* r1,
                                        const float* s2, const float* r2, int B, int rows_per_batch, int K, int Cout,
                                        float* partial, int relu_col0, int win0_col0, int win0_cols, int win1_col0,
                                        int win1_cols, const unsigned char* tile_valid, int partial_tpb,
                                        pdr_stream_t stream) {
  if (!tile_valid) return PDR_EINVAL;
  return gather_launch(U, ldu, n_src, V, V0, ldv, idx, counts, s1, r1, s2, r2, B, rows_per_batch, K, Cout, nullptr, 0,
                       partial, relu_col0, 0, -1, win0_col0, win0_cols, win1_col0, win1_cols, tile_valid, partial_tpb,
                       stream);
}

extern "C" int pdr_gather_moments_tiles_twin(const float* U, int ldu, int n_src, const float* V, const float* V0,
                                             int ldv, const int* idx, const int* counts, int B, int rows_per_batch,
                                             int K, int Cout, float* partial, int relu_col0, int win0_col0,
                                             int win0_cols, int win1_col0, int win1_cols,
                                             const unsigned char* tile_valid, int partial_tpb, const int* idx0,
                                             float* Yd, int ldyd, const int* wrow0, float wmul, pdr_stream_t stream) {
  if (!tile_valid || !idx0) return PDR_EINVAL;
  return gather_launch(U, ldu, n_src, V, V0, ldv, idx, counts, nullptr, nullptr, nullptr, nullptr, B, rows_per_batch, K,
                       Cout, nullptr, 0, partial, relu_col0, 0, -1, win0_col0, win0_cols, win1_col0, win1_cols, tile_valid,
                       partial_tpb, stream, idx0, Yd, ldyd, wrow0, wmul);
}

extern "C" int pdr_gather_add(const float* U, int ldu, int n_src, const float* V, const float* V0,
                              int ldv, const int* idx, const int* counts, const float* s1,
                              const float* r1, const float* s2, const float* r2, int B,
                              int rows_per_batch, int K, int Cout, float* Y, int ldy, float* partial,
                              int relu_col0, int ycol0, int ycols, pdr_stream_t stream) {
  return gather_launch(U, ldu, n_src, V, V0, ldv, idx, counts, s1, r1, s2, r2, B, rows_per_batch, K, Cout, Y, ldy, partial,
                       relu_col0, ycol0, ycols, 0, Cout, 0, 0, nullptr, 0, stream);
}

// pdr_gather_add over a SUBSET of its 128-row tiles: tile_valid (B * ceil(rows_per_batch / 128)) bytes from
// pdr_dedup_plan, tiles with a zero byte are neither read nor written; tile t of batch element b writes row
// b * partial_tpb + t of `partial` (partial_tpb >= tiles per batch element).
extern "C" int pdr_gather_add_tiles(const float* U, int ldu, int n_src, const float* V, const float* V0,
                                    int ldv, const int* idx, const int* counts, const float* s1,
                                    const float* r1, const float* s2, const float* r2, int B,
                                    int rows_per_batch, int K, int Cout, float* Y, int ldy, float* partial,
                                    int relu_col0, int ycol0, int ycols, const unsigned char* tile_valid,
                                    int partial_tpb, pdr_stream_t stream) {
  if (!tile_valid) return PDR_EINVAL;
  return gather_launch(U, ldu, n_src, V, V0, ldv, idx, counts, s1, r1, s2, r2, B, rows_per_batch, K, Cout, Y, ldy, partial,
                       relu_col0, ycol0, ycols, 0, Cout, 0, 0, tile_valid, partial_tpb, stream);
}

// pdr_gather_add_tiles + the block's per-QUERY rows in the same launch (round 5: was a second, K = 1 pdr_gather_add on
// the first neighbours followed by pdr_weighted_moments): Yd (B m, ldyd) <- U[b, idx0[q]] + V[q] (empty ball: V0[q]),
// every column; partial row b partial_tpb + tpb + j <- wmul x the moments of the rows q >= wrow0[b] of the cloud's
// j-th group of 128 queries (m = rows_per_batch / K queries per cloud).  Ball form only (no s1 / s2).
extern "C" int pdr_gather_add_tiles_twin(const float* U, int ldu, int n_src, const float* V, const float* V0,
                                         int ldv, const int* idx, const int* counts, int B, int rows_per_batch, int K,
                                         int Cout, float* Y, int ldy, float* partial, int relu_col0, int ycol0,
                                         int ycols, const unsigned char* tile_valid, int partial_tpb, const int* idx0,
                                         float* Yd, int ldyd, const int* wrow0, float wmul, pdr_stream_t stream) {
  if (!tile_valid || !idx0) return PDR_EINVAL;
  return gather_launch(U, ldu, n_src, V, V0, ldv, idx, counts, nullptr, nullptr, nullptr, nullptr, B, rows_per_batch, K,
                       Cout, Y, ldy, partial, relu_col0, ycol0, ycols, 0, Cout, 0, 0, tile_valid, partial_tpb, stream, idx0,
                       Yd, ldyd, wrow0, wmul);
}
