// fps_round.h -- the index-exact round of furthest point sampling, written once for the kernels of fps.hip and
// fps_ragged.hip (device only).  A round is: read the last pick -> packed distance / min update of the points a thread
// holds -> in-lane arg-max (the kernels' own: it depends on the slot layout) -> wave arg-max -> cross-wave exchange.
//
// Two kinds of pieces.  A __forceinline__ function is optimised on its own BEFORE it is inlined, and for the pieces
// that unroll loops over a thread's registers that changed the kernels' code (other instruction order and register
// allocation, up to 6 % per call): those -- FPS_INITIAL_DISTANCE, FPS_PACKED_UPDATE, FPS_LOAD_SORTED_SLOTS -- are
// macros, like PDR_SUM3 of pdr_common.h, and expand in the kernel exactly as if written there.  The wave arg-max, the
// exchange and the stream form are functions: the kernels compile to the same instructions with them.
#pragma once
#include "pdr_common.h"

// Running distance a point of squared norm mag = PDR_SUM3(x, y, z) starts with: -1 = never selectable, never updated
// upward (excluded points, and the `padding` slots beyond the cloud).
// reference: `if (mag <= 1e-3) continue;` -- float promoted to double
#define FPS_INITIAL_DISTANCE(mag, padding) (((padding) || static_cast<double>(mag) <= 1e-3) ? -1.0f : 1e10f)

// tmp[g] = min(tmp[g], |p[g] - c|^2) for G pairs of points (arrays of fps::f2) on PACKED fp32: two points per v_pk_*
// instruction, each half IEEE-exact, the PDR_SUM3 expression tree -> the bits of the scalar form.  Written stage by
// stage over groups of GS pairs so that consecutive instructions are independent: one wave per SIMD has nothing else
// to hide the VALU latency of a dependent chain behind.  GS bounds the temporaries alive at once (4 f2 per pair of a
// group).  The optional trailing statement runs for every pair right after its minimum, with `pair` (its index) and
// `r` (the new tmp[pair]) in scope: the in-lane scan of a kernel that fuses it with the update.
#define FPS_PACKED_UPDATE(G_, GS_, px, py, pz, tmp, cx, cy, cz, ...)                                             \
  {                                                                                                              \
    constexpr int fpu_G = (G_), fpu_GS = (GS_);                                                                  \
    _Pragma("unroll") for (int fpu_g0 = 0; fpu_g0 < fpu_G; fpu_g0 += fpu_GS) {                                   \
      fps::f2 fpu_dx[fpu_GS], fpu_dy[fpu_GS], fpu_dz[fpu_GS], fpu_d[fpu_GS];                                     \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)                                                         \
        if (fpu_g0 + g < fpu_G) fpu_dy[g] = py[fpu_g0 + g] - (cy);                                               \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)                                                         \
        if (fpu_g0 + g < fpu_G) fpu_dx[g] = px[fpu_g0 + g] - (cx);                                               \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)   /* PDR_SUM3: fma(c, c, fma(a, a, b * b)) */           \
        if (fpu_g0 + g < fpu_G) fpu_d[g] = fpu_dy[g] * fpu_dy[g];                                                \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)                                                         \
        if (fpu_g0 + g < fpu_G) fpu_dz[g] = pz[fpu_g0 + g] - (cz);                                               \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)                                                         \
        if (fpu_g0 + g < fpu_G) fpu_d[g] = __builtin_elementwise_fma(fpu_dx[g], fpu_dx[g], fpu_d[g]);            \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)                                                         \
        if (fpu_g0 + g < fpu_G) fpu_d[g] = __builtin_elementwise_fma(fpu_dz[g], fpu_dz[g], fpu_d[g]);            \
      _Pragma("unroll") for (int g = 0; g < fpu_GS; ++g)                                                         \
        if (fpu_g0 + g < fpu_G) {                                                                                \
          /* v_min_f32 directly (fminf / elementwise_min first canonicalise both operands: +1 VALU per point) */ \
          const int pair = fpu_g0 + g;                                                                           \
          fps::f2 r;                                                                                             \
          asm("v_min_f32 %0, %1, %2" : "=v"(r[0]) : "v"(fpu_d[g][0]), "v"(tmp[pair][0]));                        \
          asm("v_min_f32 %0, %1, %2" : "=v"(r[1]) : "v"(fpu_d[g][1]), "v"(tmp[pair][1]));                        \
          tmp[pair] = r;                                                                                         \
          __VA_ARGS__                                                                                            \
        }                                                                                                        \
    }                                                                                                            \
  }

// Thread `tid` of T_ takes the points k = tid + i T_ of p_[N_][3] into its arrays px, py, pz (float[PPT_]) with their
// initial running distance tmp and the tie key
//     low = (0xFFFF - tierank) << 16 | k   (larger = preferred; padding: 0),
// tierank = bitrev(k % R_) * Q_ + k / R_, sorted by descending `low` (= ascending tie rank) so that "first strictly
// greater wins" inside the thread is the reference's order.
#define FPS_LOAD_SORTED_SLOTS(T_, PPT_, p_, N_, R_, Rbits_, Q_, tid_, px, py, pz, tmp, low)                \
  {                                                                                                        \
    _Pragma("unroll") for (int i = 0; i < (PPT_); ++i) {                                                   \
      const int k = (tid_) + i * (T_);                                                                     \
      if (k < (N_)) {                                                                                      \
        px[i] = (p_)[k * 3 + 0];                                                                           \
        py[i] = (p_)[k * 3 + 1];                                                                           \
        pz[i] = (p_)[k * 3 + 2];                                                                           \
        const float mag = PDR_SUM3(px[i], py[i], pz[i]);                                                   \
        tmp[i] = FPS_INITIAL_DISTANCE(mag, false);                                                         \
        const unsigned rank = pdr::bitrev(static_cast<unsigned>(k % (R_)), (Rbits_)) * (Q_) + k / (R_);    \
        low[i] = ((0xFFFFu - rank) << 16) | static_cast<unsigned>(k);                                      \
      } else {                                                                                             \
        px[i] = py[i] = pz[i] = 0.0f;                                                                      \
        tmp[i] = -1.0f; /* padding */                                                                      \
        low[i] = 0u;                                                                                       \
      }                                                                                                    \
    }                                                                                                      \
    _Pragma("unroll") for (int a = 0; a < (PPT_) - 1; ++a) {                                               \
      _Pragma("unroll") for (int c = 0; c < (PPT_) - 1 - a; ++c) {                                         \
        if (low[c] < low[c + 1]) {                                                                         \
          float t;                                                                                         \
          unsigned u;                                                                                      \
          t = px[c]; px[c] = px[c + 1]; px[c + 1] = t;                                                     \
          t = py[c]; py[c] = py[c + 1]; py[c + 1] = t;                                                     \
          t = pz[c]; pz[c] = pz[c + 1]; pz[c + 1] = t;                                                     \
          t = tmp[c]; tmp[c] = tmp[c + 1]; tmp[c + 1] = t;                                                 \
          u = low[c]; low[c] = low[c + 1]; low[c + 1] = u;                                                 \
        }                                                                                                  \
      }                                                                                                    \
    }                                                                                                      \
  }

namespace fps {

typedef float f2 __attribute__((ext_vector_type(2)));

struct Point {
  float x, y, z, tag;   // tag: +1 an original, -1 a mirrored point (fps_ragged.hip); unused by the dense kernels
};

// Wave-wide maximum of non-negative keys with the DPP shift as an operand modifier of the v_max_u32 itself (one
// instruction per step; pdr::wave_max_u32 of pdr_common.h is the builtin form: a v_mov_dpp and a select per step).
// Lanes without a DPP source are disabled for that step and keep their own value; lane 63 ends with the maximum.
// (two wait states between a VALU write of a register and a DPP read of it: the assembler does not insert them)
__device__ __forceinline__ unsigned wave_max_u32_asm(unsigned v) {
  asm volatile(
      "s_nop 1\n\t"
      "v_max_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(v));
  return __builtin_amdgcn_readlane(v, 63);
}

// Wave arg-max as two 32-bit reductions instead of one on a 64-bit key: the value (best >= 0 -> monotone uint bits; "no
// candidate" (-1) -> 0), then `key` (larger = preferred) among the lanes that hold the winning value.  A candidate at
// distance +0.0 has value bits 0 like "no candidate", but keeps its key.  Returns (value bits, winning key), uniform in
// the wave; key 0 = no candidate at all.
__device__ __forceinline__ unsigned long long wave_argmax(float best, unsigned key) {
  const unsigned vb = best < 0.0f ? 0u : __float_as_uint(best);
  const unsigned vmax = wave_max_u32_asm(vb);
  const unsigned cand = (vb == vmax && !(best < 0.0f)) ? key : 0u;
  return pdr::u64_from(vmax, wave_max_u32_asm(cand));
}

// Cross-wave maximum with ONE barrier: every wave publishes its key in `s` (W u64 slots), all read the W entries
// back.  The caller alternates between two such rows by the parity of the round, so a wave may publish round j + 1
// while another still reads round j.
template <int W>
__device__ __forceinline__ unsigned long long exchange_max(unsigned long long* s, unsigned long long key) {
  if constexpr (W > 1) {
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = key;
    __syncthreads();
    key = s[0];
#pragma unroll
    for (int w = 1; w < W; ++w) {
      const unsigned long long o = s[w];
      key = o > key ? o : key;
    }
  }
  return key;
}

// Streaming form for clouds too large to stay in registers: all m rounds of one cloud of V points by a workgroup of
// kStreamThreads threads -- running distances in tp[V] (global memory), points re-read from `src` every round
// (src.point(k) returns a Point), two-stage (value, rank) arg-max.  The rank is the lexicographic key
// (bitrev9(k & 511), k >> 9), which for every V >= 512 is the order of the reference's
// bitrev(k % R) * ceil(V / R) + k / R (R = 512), with k below it: 9 + 23 + 32 bits hold every int k and need no
// inverse.  A thread walks k = tid + kStreamThreads i: k & 511 is the same for all of its points and k >> 9 grows with
// i, so it meets them in ascending rank and "first strictly greater wins" needs no rank inside the scan.  rows (may be
// NULL) receives the picked points.  Not on the hot path; kept simple.
constexpr int kStreamThreads = 1024;
static_assert(kStreamThreads % 512 == 0, "a thread's points must share k & 511: the in-lane scan relies on it");

template <class Source>
__device__ __forceinline__ void stream_rounds(const Source& src, int V, int m, float* __restrict__ tp,
                                              int* __restrict__ out, float4* __restrict__ rows) {
  constexpr int kWaves = kStreamThreads / 64;
  __shared__ float sval[kWaves];
  __shared__ unsigned long long srank[kWaves];
  __shared__ int sold;
  const int tid = threadIdx.x;
  for (int k = tid; k < V; k += kStreamThreads) {
    const Point v = src.point(k);
    const float mag = PDR_SUM3(v.x, v.y, v.z);
    tp[k] = FPS_INITIAL_DISTANCE(mag, false);
  }
  if (tid == 0) out[0] = 0;
  __syncthreads();
  int old = 0;
  for (int j = 1; j < m; ++j) {
    const Point c = src.point(old);
    if (tid == 0 && rows) rows[j - 1] = make_float4(c.x, c.y, c.z, c.tag);
    float best = -1.0f;
    unsigned bestk = 0u;
    for (int k = tid; k < V; k += kStreamThreads) {
      const Point v = src.point(k);
      const float dx = v.x - c.x, dy = v.y - c.y, dz = v.z - c.z;
      const float d2 = fminf(PDR_SUM3(dx, dy, dz), tp[k]);
      tp[k] = d2;
      const bool better = d2 > best;
      best = better ? d2 : best;
      bestk = better ? static_cast<unsigned>(k) : bestk;
    }
    // smaller = preferred; low 32 bits = k
    unsigned long long bestrank =
        best < 0.0f ? ~0ull : pdr::u64_from((__brev(bestk & 511u) >> 23 << 23) | (bestk >> 9), bestk);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const unsigned long long orank = __shfl_xor(bestrank, off, 64);
      const bool better = ov > best || (ov == best && orank < bestrank);
      best = better ? ov : best;
      bestrank = better ? orank : bestrank;
    }
    if ((tid & 63) == 0) {
      sval[tid >> 6] = best;
      srank[tid >> 6] = bestrank;
    }
    __syncthreads();
    if (tid == 0) {
      float bv = sval[0];
      unsigned long long br = srank[0];
      for (int w = 1; w < kWaves; ++w) {
        const bool better = sval[w] > bv || (sval[w] == bv && srank[w] < br);
        bv = better ? sval[w] : bv;
        br = better ? srank[w] : br;
      }
      sold = bv < 0.0f ? 0 : static_cast<int>(br & 0xFFFFFFFFull);   // no candidate at all: index 0, as the reference
      out[j] = sold;
    }
    __syncthreads();
    old = sold;
  }
  if (tid == 0 && rows) {
    const Point c = src.point(old);
    rows[m - 1] = make_float4(c.x, c.y, c.z, c.tag);
  }
}

}  // namespace fps
