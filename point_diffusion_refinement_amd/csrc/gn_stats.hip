// gn_stats.hip -- GroupNorm statistics: from the layer kernels' per-(tile, channel) partial sums to the per-(batch,
// channel) affine form y = x * scale + shift that the NEXT layer's prologue applies.
//
// A layer kernel (fused_layer.hip, fused_layer_ws.hip) leaves one row of (sum f(y), sum f(y)^2) per row tile in `partial`.
// pdr_gn_fold reduces up to two such sources over the tiles of a batch element in double, in a fixed order (no atomics),
// and folds the groups in the same launch; pdr_gn_reduce + pdr_gn_finalize are the same computation as two launches
// through a (B, C) table of double moments.  The group fold itself is pdr::gn_scale_shift (gn_fold.h).
#include "gn_fold.h"

namespace {

// chan_stats[b, coff + c] (double2) = mult * sum over the tiles of batch b of partial[tile, c].
// 1024 threads = 32 channels x 32 tile-slices: the per-(b,c) sum over up to 512 tiles is split
// over 32 lanes' worth of independent loads and folded through LDS in a fixed order.
__global__ __launch_bounds__(1024) void gn_reduce_kernel(const float* __restrict__ partial, int ldp,
                                                         int tiles_per_batch, int C, double mult,
                                                         double* __restrict__ chan_stats, int Ctot,
                                                         int coff) {
  __shared__ double red[32][32][2];
  const int b = blockIdx.y;
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float* p = partial + (static_cast<long>(b) * tiles_per_batch * ldp + c) * 2;
    for (int t = sl; t < tiles_per_batch; t += 32) {
      const float2 v = *reinterpret_cast<const float2*>(p + static_cast<long>(t) * ldp * 2);
      s1 += v.x;
      s2 += v.y;
    }
  }
  red[sl][cl][0] = s1;
  red[sl][cl][1] = s2;
  __syncthreads();
  if (sl == 0 && c < C) {
    double a1 = 0.0, a2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      a1 += red[k][cl][0];
      a2 += red[k][cl][1];
    }
    double* o = chan_stats + (static_cast<long>(b) * Ctot + coff + c) * 2;
    o[0] = a1 * mult;
    o[1] = a2 * mult;
  }
}

// gn_reduce + gn_finalize for up to two partial sources in ONE launch: block b reduces the tile
// partials of batch element b into LDS (double), then folds GroupNorm to scale / shift.
struct FoldPart {
  const float* partial;   // first of `C` columns inside rows of `ldp` columns
  int ldp, tiles_per_batch, C;
  double mult;
  // a tile SUBSET produced these rows (round 5): of the first tpb_main rows of batch element b only the first
  // nvalid[b] were written (sorted queries: a cloud's valid tiles are its first ones) -- the others are skipped, not
  // read as zeros (nobody zeroes them any more); rows >= tpb_main (the per-query rows' moments) always count
  const int* nvalid;
  int tpb_main;
};

__global__ __launch_bounds__(1024) void gn_fold_wide_kernel(FoldPart p0, FoldPart p1, int C, int Cn, int G,
                                                       double n, float eps,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta,
                                                       float* __restrict__ scale,
                                                       float* __restrict__ shift) {
  extern __shared__ __attribute__((aligned(16))) double cs[];   // [C][2]
  __shared__ double red[32][32][2];
  const int b = blockIdx.x;
  double* redf = &red[0][0][0];   // [1024][2]
  int coff = 0;
  for (int part = 0; part < 2; ++part) {
    const FoldPart p = part == 0 ? p0 : p1;
    if (!p.partial) continue;
    // W channels x (1024 / W) tile slices per pass: ONE pass (two barriers) for C <= 1024 instead of
    // one per 32 channels -- the kernel is barrier / latency bound, not bandwidth bound
    int W = 32;
    while (W < p.C && W < 1024) W <<= 1;
    const int nsl = 1024 / W;
    const int cl = threadIdx.x & (W - 1), sl = threadIdx.x / W;
    for (int c0 = 0; c0 < p.C; c0 += W) {
      const int c = c0 + cl;
      double s1 = 0.0, s2 = 0.0;
      if (c < p.C) {
        const float* q = p.partial + (static_cast<long>(b) * p.tiles_per_batch * p.ldp + c) * 2;
        const int nv = p.nvalid ? p.nvalid[b] : p.tpb_main;
        for (int t = sl; t < p.tiles_per_batch; t += nsl * 8) {
          float2 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int tt = t + nsl * u;
            v[u] = (tt < p.tiles_per_batch && !(tt >= nv && tt < p.tpb_main))
                       ? *reinterpret_cast<const float2*>(q + static_cast<long>(tt) * p.ldp * 2)
                       : make_float2(0.0f, 0.0f);
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            s1 += v[u].x;
            s2 += v[u].y;
          }
        }
      }
      redf[threadIdx.x * 2 + 0] = s1;
      redf[threadIdx.x * 2 + 1] = s2;
      __syncthreads();
      if (sl == 0 && c < p.C) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < nsl; ++k) {
          a1 += redf[(k * W + cl) * 2 + 0];
          a2 += redf[(k * W + cl) * 2 + 1];
        }
        cs[(coff + c) * 2 + 0] = a1 * p.mult;
        cs[(coff + c) * 2 + 1] = a2 * p.mult;
      }
      __syncthreads();
    }
    coff += p.C;
  }
  for (int c = threadIdx.x; c < C; c += 1024) {
    float sc = 1.0f, sh = 0.0f;
    if (c < Cn) {
      const int cpg = Cn / G;
      const int g0 = (c / cpg) * cpg;
      double s1 = 0.0, s2 = 0.0;
      for (int j = 0; j < cpg; ++j) {
        s1 += cs[(g0 + j) * 2 + 0];
        s2 += cs[(g0 + j) * 2 + 1];
      }
      const pdr::GnAffine a = pdr::gn_scale_shift(s1, s2, n * cpg, eps, gamma, beta, c);
      sc = a.scale;
      sh = a.shift;
    }
    scale[static_cast<long>(b) * C + c] = sc;
    shift[static_cast<long>(b) * C + c] = sh;
  }
}

// The fold that runs in the step (cpg = Cn / G <= 32): one 256-thread workgroup per (batch element, window of
// whole groups covering <= 32 channels).  A launch is B x ceil(Cn / window) small workgroups of four waves with
// 2.5 KB of LDS and < 40 VGPRs, so that it is admitted beside resident layer workgroups of the other stream
// instead of waiting for a CU to drain (the 1024-thread / 16 KB + 16 C form above could not co-reside with two
// persistent 512-thread layer workgroups; rocprofv3: 23.5 us per fold inside the two-stream step vs 7 us alone).
// Lanes 0-31 / 32-63 of a wave read the same 32 channels (256 contiguous bytes of a tile's partial row) of two
// different tile slices; 8 slices per workgroup, four loads in flight per thread; double sums, fixed order.
// U = partial rows in flight per thread and trip: 4 for up to 128 tiles per batch element (one or two trips), 16 above --
// the level-0 layers have 256 / 512 tiles per batch element, i.e. 32 / 64 rows per thread, and every trip is a dependent
// round trip to rows another kernel has just written (~1 us): 16 trips -> 4 (round 4; tools/lab/gn_fold_bench.py).
template <int U>
__global__ __launch_bounds__(256) void gn_fold_kernel(FoldPart p0, FoldPart p1, int C, int Cn, int G, int CW,
                                                      double n, float eps,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta,
                                                      float* __restrict__ scale,
                                                      float* __restrict__ shift) {
  __shared__ double red[4][32][2];
  __shared__ double cs[32][2];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * CW;
  if (c0 >= Cn) {   // the trailing workgroup: channels outside the normalised range pass through
    for (int c = Cn + threadIdx.x; c < C; c += 256) {
      scale[static_cast<long>(b) * C + c] = 1.0f;
      shift[static_cast<long>(b) * C + c] = 0.0f;
    }
    return;
  }
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, wave = threadIdx.x >> 6;
  const int c = c0 + cl;
  const bool valid = cl < CW && c < Cn;
  double s1 = 0.0, s2 = 0.0, mult = 1.0;
  if (valid) {
    const bool first = c < p0.C;
    const FoldPart p = first ? p0 : p1;
    const int col = first ? c : c - p0.C;
    mult = p.mult;
    const long stride = static_cast<long>(p.ldp) * 2;
    const float* q = p.partial + (static_cast<long>(b) * p.tiles_per_batch * p.ldp + col) * 2;
    // (loaded beside the partial rows, consumed behind them: no extra dependent round trip)
    const int nv = p.nvalid ? p.nvalid[b] : p.tpb_main;
    const int tpb_main = p.tpb_main;
    for (int t = sl; t < p.tiles_per_batch; t += 8 * U) {
      // U loads in flight: unconditional, from a clamped tile (t itself is valid), zeroed afterwards -- a load
      // under `tt < tiles` compiles to a branch with its own vmcnt(0), i.e. U dependent round trips per trip
      float2 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int tt = t + 8 * u;
        v[u] = *reinterpret_cast<const float2*>(q + (tt < p.tiles_per_batch ? tt : t) * stride);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int tt = t + 8 * u;
        const bool ok = tt < p.tiles_per_batch && !(tt >= nv && tt < tpb_main);   // (skipped tiles hold garbage)
        s1 += ok ? v[u].x : 0.0f;
        s2 += ok ? v[u].y : 0.0f;
      }
    }
  }
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if ((threadIdx.x & 63) < 32) {
    red[wave][cl][0] = s1;
    red[wave][cl][1] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    cs[cl][0] = (red[0][cl][0] + red[1][cl][0] + red[2][cl][0] + red[3][cl][0]) * mult;
    cs[cl][1] = (red[0][cl][1] + red[1][cl][1] + red[2][cl][1] + red[3][cl][1]) * mult;
  }
  __syncthreads();
  if (threadIdx.x < 32 && valid) {
    const int cpg = Cn / G;
    const int g0 = (cl / cpg) * cpg;
    double g1 = 0.0, g2 = 0.0;
    for (int j = 0; j < cpg; ++j) {
      g1 += cs[g0 + j][0];
      g2 += cs[g0 + j][1];
    }
    const pdr::GnAffine a = pdr::gn_scale_shift(g1, g2, n * cpg, eps, gamma, beta, c);
    scale[static_cast<long>(b) * C + c] = a.scale;
    shift[static_cast<long>(b) * C + c] = a.shift;
  }
}

// GroupNorm(G groups over the first Cn of C channels, eps) folded to y = x*scale + shift;
// channels >= Cn pass through (MyGroupNorm).  n = elements per channel per batch.
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ chan_stats, int C,
                                                          int Cn, int G, double n, float eps,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          float* __restrict__ scale,
                                                          float* __restrict__ shift) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float sc = 1.0f, sh = 0.0f;
  if (c < Cn) {
    const int cpg = Cn / G;
    const int g0 = (c / cpg) * cpg;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < cpg; ++j) {
      s1 += chan_stats[(static_cast<long>(b) * C + g0 + j) * 2 + 0];
      s2 += chan_stats[(static_cast<long>(b) * C + g0 + j) * 2 + 1];
    }
    const pdr::GnAffine a = pdr::gn_scale_shift(s1, s2, n * cpg, eps, gamma, beta, c);
      sc = a.scale;
      sh = a.shift;
  }
  scale[static_cast<long>(b) * C + c] = sc;
  shift[static_cast<long>(b) * C + c] = sh;
}

}  // namespace

extern "C" int pdr_gn_reduce(const float* partial, int ldp, int B, int tiles_per_batch, int C,
                             double mult, double* chan_stats, int Ctot, int coff,
                             pdr_stream_t stream) {
  if (!partial || !chan_stats || B <= 0 || tiles_per_batch <= 0 || C <= 0 || coff < 0 ||
      coff + C > Ctot || ldp < C)
    return PDR_EINVAL;
  hipLaunchKernelGGL(gn_reduce_kernel, dim3((C + 31) / 32, B), dim3(1024), 0, pdr::as_stream(stream),
                     partial, ldp, tiles_per_batch, C, mult, chan_stats, Ctot, coff);
  return pdr::check_launch();
}

// One-launch GroupNorm fold: up to two partial sources (second may be NULL) covering C = C0 + C1
// channels in order; see pdr_gn_reduce / pdr_gn_finalize for the semantics.
extern "C" int pdr_gn_fold(const float* part0, int ldp0, int tpb0, int C0, double mult0,
                           const float* part1, int ldp1, int tpb1, int C1, double mult1, int B, int Cn,
                           int G, double n, float eps, const float* gamma, const float* beta,
                           float* scale, float* shift, const int* nvalid0, int tpb_main0, const int* nvalid1,
                           int tpb_main1, pdr_stream_t stream) {
  if (!part0 || C0 <= 0 || tpb0 <= 0 || ldp0 < C0 || B <= 0 || G <= 0 || !scale || !shift)
    return PDR_EINVAL;
  if (part1 && (C1 <= 0 || tpb1 <= 0 || ldp1 < C1)) return PDR_EINVAL;
  if ((nvalid0 && (tpb_main0 <= 0 || tpb_main0 > tpb0)) || (nvalid1 && (!part1 || tpb_main1 <= 0 || tpb_main1 > tpb1)))
    return PDR_EINVAL;
  const int C = C0 + (part1 ? C1 : 0);
  if (Cn < 0 || Cn > C || (Cn > 0 && (Cn % G != 0 || !gamma || !beta))) return PDR_EINVAL;
  // (without a subset: nv = tpb_main = 0 -- the range [nv, tpb_main) of skipped rows is empty)
  FoldPart p0{part0, ldp0, tpb0, C0, mult0, nvalid0, nvalid0 ? tpb_main0 : 0};
  FoldPart p1{part1, ldp1, tpb1, part1 ? C1 : 0, mult1, nvalid1, nvalid1 ? tpb_main1 : 0};
  const bool small_form = pdr::option(pdr::OPT_GN_FOLD_SMALL) != 0;
  const int cpg = Cn > 0 ? Cn / G : 1;
  if (small_form && cpg <= 32) {
    // windows of whole groups covering <= 32 channels; one more workgroup row for pass-through channels
    const int CW = (32 / cpg) * cpg;
    const int nw = (Cn + CW - 1) / CW + (C > Cn ? 1 : 0);
    // (same sums in the same order for either U: slices of 8 tiles, rows ascending within a slice)
    if (tpb0 > 128 || (part1 && tpb1 > 128))
      hipLaunchKernelGGL(gn_fold_kernel<16>, dim3(nw, B), dim3(256), 0, pdr::as_stream(stream), p0, p1, C, Cn, G,
                         CW, n, eps, gamma, beta, scale, shift);
    else
      hipLaunchKernelGGL(gn_fold_kernel<4>, dim3(nw, B), dim3(256), 0, pdr::as_stream(stream), p0, p1, C, Cn, G,
                         CW, n, eps, gamma, beta, scale, shift);
    return pdr::check_launch();
  }
  if (static_cast<size_t>(C) * 16 > 48 * 1024) return PDR_EUNSUPPORTED;
  hipLaunchKernelGGL(gn_fold_wide_kernel, dim3(B), dim3(1024), static_cast<size_t>(C) * 16,
                     pdr::as_stream(stream), p0, p1, C, Cn, G, n, eps, gamma, beta, scale, shift);
  return pdr::check_launch();
}

extern "C" int pdr_gn_finalize(const double* chan_stats, int B, int C, int Cn, int G, double n,
                               float eps, const float* gamma, const float* beta, float* scale,
                               float* shift, pdr_stream_t stream) {
  if (!chan_stats || !scale || !shift || B <= 0 || C <= 0 || Cn < 0 || Cn > C || G <= 0 ||
      (Cn > 0 && (Cn % G != 0 || !gamma || !beta)))
    return PDR_EINVAL;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((C + 255) / 256, B), dim3(256), 0,
                     pdr::as_stream(stream), chan_stats, C, Cn, G, n, eps, gamma, beta, scale, shift);
  return pdr::check_launch();
}
