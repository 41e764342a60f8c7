// fps.hip -- furthest point sampling for gfx950.
//
// Replaces furthest_point_sampling_kernel (reference sampling_gpu.cu:69-173).
// The reference runs one 512-thread block per cloud, re-reads/re-writes the
// (B,N) `temp` array from global memory every round and pays ~10 __syncthreads
// per round for its shared-memory tree.  Here a cloud is owned by one workgroup
// of T threads whose points AND running min-distances live in VGPRs for the
// whole kernel; a round is
//     LDS broadcast of the last pick -> PPT fused distance/min/arg-max updates
//     -> one DPP wave arg-max (no LDS) -> W-entry LDS exchange, ONE barrier.
// Index-exactness: the reference's winner is the maximum value with ties broken
// by (bit-reversed reference thread id, then lowest k) -- the shared-memory tree
// keeps the LEFT slot on ties, so bit 0 of tid is the most significant tie bit.
// That total order is folded into a 64-bit key so the result is independent of
// this kernel's own thread geometry:
//     key = float_bits(d2) << 32 | (0xFFFF - tierank) << 16 | k
// with tierank = bitrev(k % R) * ceil(N/R) + k / R and R = opt_n_threads(N)
// (cuda_utils.h:13-19).  Each thread pre-sorts its points by tierank so the
// in-register scan needs only the reference's strict '>'.
//
// The pieces of a round that do not depend on a kernel's slot layout (exclusion rule, packed distance update, DPP wave
// arg-max, cross-wave exchange, the sorted load, the stream form) are in fps_round.h, shared with fps_ragged.hip.
#include "fps_round.h"

#include <cstdlib>

namespace {

using fps::f2;

constexpr int kMaxResidentN = 16384;  // 16-bit k / tierank fields

template <int T, int PPT>
__global__ __launch_bounds__(T) void fps_resident_kernel(
    const float* __restrict__ xyz, int N, int m, int R, int Rbits, int Q,
    int* __restrict__ idxs) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int W = T / 64;
  float* sx = smem;
  float* sy = smem + N;
  float* sz = smem + 2 * N;
  // exchange slots: 2 parities x W waves (u64), 16-B aligned behind the cloud
  unsigned long long* slots =
      reinterpret_cast<unsigned long long*>(smem + ((3 * N + 3) & ~3));

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* p = xyz + static_cast<size_t>(b) * N * 3;
  int* out = idxs + static_cast<size_t>(b) * m;

  for (int i = tid; i < N; i += T) {
    sx[i] = p[i * 3 + 0];
    sy[i] = p[i * 3 + 1];
    sz[i] = p[i * 3 + 2];
  }

  float px[PPT], py[PPT], pz[PPT], tmp[PPT];
  unsigned low[PPT];  // (0xFFFF - tierank) << 16 | k ; larger = preferred
  FPS_LOAD_SORTED_SLOTS(T, PPT, p, N, R, Rbits, Q, tid, px, py, pz, tmp, low)

  if (tid == 0) out[0] = 0;
  __syncthreads();

  int old = 0;
  for (int j = 1; j < m; ++j) {
    const float x1 = sx[old], y1 = sy[old], z1 = sz[old];
    float best = -1.0f;
    unsigned bestlow = 0u;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const float dx = px[i] - x1, dy = py[i] - y1, dz = pz[i] - z1;
      const float d = PDR_SUM3(dx, dy, dz);
      const float d2 = fminf(d, tmp[i]);
      tmp[i] = d2;
      const bool gt = d2 > best;
      best = gt ? d2 : best;
      bestlow = gt ? low[i] : bestlow;
    }
    // best >= 0 -> monotone uint bits; "no candidate" (-1) -> key 0
    unsigned long long key =
        best < 0.0f ? 0ull : pdr::u64_from(__float_as_uint(best), bestlow);
    key = pdr::wave_max_u64(key);
    key = fps::exchange_max<W>(slots + (j & 1) * W, key);
    old = static_cast<int>(key & 0xFFFFull);
    if (tid == 0) out[j] = old;
  }
}

// One WAVE per cloud (N <= 64 * PPT <= 2048): no workgroup barrier and no LDS exchange in the round.
//   * lane l, slot i owns the point of tie rank r = 64 i + l (k = (r % Q) R + bitrev(r / Q)): inside a lane the
//     slots are already in the reference's tie order, so "first strictly greater wins" needs no sorting;
//   * the distance update runs on PACKED fp32 (FPS_PACKED_UPDATE);
//   * the wave arg-max is two 32-bit DPP reductions (value, then rank|index among the lanes holding the value)
//     instead of one on a 64-bit key; the winner's coordinates come back from LDS by index (one ds_read_b128).
// A round is ~7 VALU slots per point + ~150 cycles: 2048 -> 1024 in ~0.26 ms (the 4-wave form needs 0.49 ms
// because every round ends in a barrier + LDS exchange); the deeper levels of the chain shrink likewise.

// (da, la) <- (db > da) ? (db, lb) : (da, la)
__device__ __forceinline__ void fps_combine(float& da, unsigned& la, float db, unsigned lb) {
  asm volatile(
      "v_cmp_gt_f32 vcc, %2, %0\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32 %0, %0, %2, vcc\n\t"
      "v_cndmask_b32 %1, %1, %3, vcc"
      : "+v"(da), "+v"(la)
      : "v"(db), "v"(lb)
      : "vcc");
}
// two independent combines, interleaved so that neither mask is read in the two issue slots after its write
__device__ __forceinline__ void fps_combine2(float& da, unsigned& la, float db, unsigned lb, float& dc,
                                             unsigned& lc, float dd, unsigned ld) {
  unsigned long long m;
  asm volatile(
      "v_cmp_gt_f32 vcc, %5, %0\n\t"
      "v_cmp_gt_f32 %4, %7, %2\n\t"
      "s_nop 0\n\t"
      "v_cndmask_b32 %0, %0, %5, vcc\n\t"
      "v_cndmask_b32 %1, %1, %6, vcc\n\t"
      "v_cndmask_b32 %2, %2, %7, %4\n\t"
      "v_cndmask_b32 %3, %3, %8, %4"
      : "+v"(da), "+v"(la), "+v"(dc), "+v"(lc), "=&s"(m)
      : "v"(db), "v"(lb), "v"(dd), "v"(ld)
      : "vcc");
}

// first tree level on two slot pairs (2H, 2H+1) and (2H+2, 2H+3): the slot numbers are immediates
template <int H>
__device__ __forceinline__ void fps_first2(const f2& a, const f2& b, float& bd0, unsigned& bs0, float& bd1,
                                           unsigned& bs1) {
  unsigned long long m;
  asm volatile(
      "v_cmp_gt_f32 vcc, %6, %5\n\t"
      "v_cmp_gt_f32 %4, %8, %7\n\t"
      "s_nop 0\n\t"
      "v_cndmask_b32 %0, %5, %6, vcc\n\t"
      "v_cndmask_b32 %1, %9, %10, vcc\n\t"
      "v_cndmask_b32 %2, %7, %8, %4\n\t"
      "v_cndmask_b32 %3, %11, %12, %4"
      : "=&v"(bd0), "=&v"(bs0), "=&v"(bd1), "=&v"(bs1), "=&s"(m)
      : "v"(a[0]), "v"(a[1]), "v"(b[0]), "v"(b[1]), "n"(2 * H), "n"(2 * H + 1), "n"(2 * H + 2), "n"(2 * H + 3)
      : "vcc");
}
template <int H>
__device__ __forceinline__ void fps_first1(const f2& a, float& bd0, unsigned& bs0) {
  asm volatile(
      "v_cmp_gt_f32 vcc, %3, %2\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32 %0, %2, %3, vcc\n\t"
      "v_cndmask_b32 %1, %4, %5, vcc"
      : "=&v"(bd0), "=&v"(bs0)
      : "v"(a[0]), "v"(a[1]), "n"(2 * H), "n"(2 * H + 1)
      : "vcc");
}
template <int H, int NH>
__device__ __forceinline__ void fps_level0(const f2 (&tmp)[NH], float (&bd)[NH], unsigned (&bs)[NH]) {
  if constexpr (H + 1 < NH) {
    fps_first2<H>(tmp[H], tmp[H + 1], bd[H], bs[H], bd[H + 1], bs[H + 1]);
    fps_level0<H + 2, NH>(tmp, bd, bs);
  } else if constexpr (H < NH) {
    fps_first1<H>(tmp[H], bd[H], bs[H]);
  }
}

template <int T, int PPT>
__global__ __launch_bounds__(T) void fps_wave_kernel(const float* __restrict__ xyz, int N, int m, int R,
                                                     int Rbits, int Q, int* __restrict__ idxs) {
  static_assert(PPT % 2 == 0, "points are processed in pairs");
  constexpr int W = T / 64;
  extern __shared__ __attribute__((aligned(16))) float4 cloud4[];
  __shared__ unsigned long long slots[2][W > 1 ? W : 1];   // per-wave (value, rank) of a round, two parities
  const int b = blockIdx.x;
  const int lane = threadIdx.x;                        // thread index in the workgroup (slot stride = T)
  const float* p = xyz + static_cast<size_t>(b) * N * 3;
  int* out = idxs + static_cast<size_t>(b) * m;
  for (int i = lane; i < N; i += T) cloud4[i] = make_float4(p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2], 0.0f);

  // slot i of thread l holds the point of tie rank r = T i + l; only coordinates and running distances stay in
  // registers -- the slot number is an immediate in the arg-max tree and the point index is recovered from the
  // winning rank with scalar arithmetic once per round
  f2 px[PPT / 2], py[PPT / 2], pz[PPT / 2], tmp[PPT / 2];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int r = i * T + lane;
    const int hi = r / Q, lo = r - hi * Q;
    const int k = lo * R + static_cast<int>(pdr::bitrev(static_cast<unsigned>(hi), Rbits));
    const bool valid = hi < R && k < N;
    const int kk = valid ? k : 0;
    const float x = p[kk * 3 + 0], y = p[kk * 3 + 1], z = p[kk * 3 + 2];
    const float mag = PDR_SUM3(x, y, z);
    px[i >> 1][i & 1] = valid ? x : 0.0f;
    py[i >> 1][i & 1] = valid ? y : 0.0f;
    pz[i >> 1][i & 1] = valid ? z : 0.0f;
    tmp[i >> 1][i & 1] = FPS_INITIAL_DISTANCE(mag, !valid);   // padding: never selectable, never updated upward
  }
  if (lane == 0) out[0] = 0;
  __syncthreads();

  int old = 0;
  for (int j = 1; j < m; ++j) {
    const float4 c = cloud4[old];
    // ---- phase 1: all distance updates (the results ARE the new running minima), in groups of at most 8 pairs
    FPS_PACKED_UPDATE(PPT / 2, (PPT / 2 < 8 ? PPT / 2 : 8), px, py, pz, tmp, c.x, c.y, c.z)
    // ---- phase 2: this lane's arg-max as a TREE over its slots: combine(a, b) with a before b in slot order lets b
    // win only if STRICTLY greater = "first maximum in slot order", what the sequential strict-'>' scan returns.
    // The combines are spelled in assembly, two per block (one mask in VCC, one in an SGPR pair, each consumed >= 2
    // issue slots after it is written): the compiler's own rendering of the select pairs (v_max + v_cmp_eq to
    // re-derive the winner, an s_nop behind every v_cmp) needed ~900 instructions per round.
    float bd[PPT / 2];
    unsigned bs[PPT / 2];                              // winning slot of the sub-tree
    fps_level0<0, PPT / 2>(tmp, bd, bs);
#pragma unroll
    for (int st = 1; st < PPT / 2; st <<= 1) {
#pragma unroll
      for (int i = 0; i + st < PPT / 2; i += 4 * st) {
        if (i + 3 * st < PPT / 2) fps_combine2(bd[i], bs[i], bd[i + st], bs[i + st], bd[i + 2 * st], bs[i + 2 * st],
                                               bd[i + 3 * st], bs[i + 3 * st]);
        else fps_combine(bd[i], bs[i], bd[i + st], bs[i + st]);
      }
    }
    const float best = bd[0];
    // fps::wave_argmax with the builtin reduction of pdr_common.h: value first, then the tie rank among the lanes that
    // hold the winning value: smaller rank preferred -> reduce 0xFFFF - r with max
    const unsigned vb = best < 0.0f ? 0u : __float_as_uint(best);
    const unsigned vmax = pdr::wave_max_u32(vb);
    const unsigned rk = 0xFFFFu - (bs[0] * static_cast<unsigned>(T) + static_cast<unsigned>(lane));
    const unsigned cand = (vb == vmax && best >= 0.0f) ? rk : 0u;
    unsigned win = pdr::wave_max_u32(cand);            // uniform in the wave
    // one barrier per round: every wave publishes (value, rank); all read the W entries back
    win = static_cast<unsigned>(fps::exchange_max<W>(slots[j & 1], pdr::u64_from(vmax, win)) & 0xFFFFFFFFull);
    // rank -> point index with scalar arithmetic (win == 0: no candidate at all -> index 0, as the reference)
    const int rw = 0xFFFF - static_cast<int>(win);
    const int hw = rw / Q, lw = rw - hw * Q;
    old = win == 0u ? 0 : lw * R + static_cast<int>(pdr::bitrev(static_cast<unsigned>(hw), Rbits));
    if (lane == 0) out[j] = old;
  }
}

// ---- the resident kernel, instruction-lean (round 5) ------------------------------------------------------------
// With one wave per SIMD a round is bound by the NUMBER of VALU instructions it issues, not by their latency alone:
// the disassembly of fps_resident_kernel<256, 8> holds ~155 per round (72 for the eight distance updates incl. a
// canonicalising v_max in front of every v_min, 24 for the in-lane arg-max, 47 for the 64-bit DPP arg-max -- two
// v_mov_dpp, a 64-bit compare and two selects per step --, a dozen for the exchange) against 1,150 cycles measured.
// fps_wave_kernel above trimmed the updates but pays an integer division per round to turn its tie rank back into a
// point index, and ended up with as many instructions (532 vs 490 us).  This form keeps the resident kernel's
// (distance bits, tie key | index) key -- no division -- and removes the rest:
//   * the cloud lives in LDS as float4: one ds_read_b128 for the last pick instead of an address computation and
//     three ds_read_b32;
//   * distance updates on packed fp32 (FPS_PACKED_UPDATE: two points per v_pk_add / v_pk_mul / v_pk_fma, v_min_f32
//     spelled directly): 32 instructions for eight points instead of 72;
//   * the wave arg-max as two 32-bit reductions whose DPP shift is an operand modifier of the v_max_u32 itself
//     (fps::wave_argmax): 12 + 6 instructions instead of 47.
// Same picks as fps_resident_kernel for every input (tests/test_ops_gpu.py::test_fps_index_exact runs both:
// option fps_lean = 0 selects the old kernel).
template <int T, int PPT>
__global__ __launch_bounds__(T) void fps_lean_kernel(const float* __restrict__ xyz, int N, int m, int R, int Rbits,
                                                     int Q, int* __restrict__ idxs) {
  static_assert(PPT % 2 == 0, "points are updated in pairs");
  constexpr int W = T / 64;
  extern __shared__ __attribute__((aligned(16))) float4 lean_cloud[];
  __shared__ unsigned long long slots[2][W > 1 ? W : 1];   // per-wave key of a round, two parities
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* p = xyz + static_cast<size_t>(b) * N * 3;
  int* out = idxs + static_cast<size_t>(b) * m;
  for (int i = tid; i < N; i += T) lean_cloud[i] = make_float4(p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2], 0.0f);

  float sx[PPT], sy[PPT], sz[PPT], st[PPT];
  unsigned low[PPT];  // (0xFFFF - tierank) << 16 | k ; larger = preferred
  FPS_LOAD_SORTED_SLOTS(T, PPT, p, N, R, Rbits, Q, tid, sx, sy, sz, st, low)
  f2 px[PPT / 2], py[PPT / 2], pz[PPT / 2], tmp[PPT / 2];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    px[i >> 1][i & 1] = sx[i];
    py[i >> 1][i & 1] = sy[i];
    pz[i >> 1][i & 1] = sz[i];
    tmp[i >> 1][i & 1] = st[i];
  }
  if (tid == 0) out[0] = 0;
  __syncthreads();

  int old = 0;
  for (int j = 1; j < m; ++j) {
    const float4 c = lean_cloud[old];
    float best = -1.0f;
    unsigned bestlow = 0u;
    // all pairs at once; the in-lane scan takes each pair as its minimum is ready
    FPS_PACKED_UPDATE(PPT / 2, PPT / 2, px, py, pz, tmp, c.x, c.y, c.z,
      _Pragma("unroll") for (int e = 0; e < 2; ++e) {
        const bool gt = r[e] > best;
        best = gt ? r[e] : best;
        bestlow = gt ? low[2 * pair + e] : bestlow;
      })
    unsigned long long key = fps::wave_argmax(best, bestlow);
    key = fps::exchange_max<W>(slots[j & 1], key);
    old = static_cast<int>(key & 0xFFFFull);
    if (tid == 0) out[j] = old;
  }
}

// Streaming fallback for N > kMaxResidentN: same ordering rule, running distances
// in the caller's (B,N) temp (reference sampling.cpp:74-76); fps::stream_rounds on
// the points as they lie in memory.  Not on the BASELINE hot path; kept simple.
struct DenseSource {
  const float* __restrict__ p;
  __device__ __forceinline__ fps::Point point(int k) const { return {p[k * 3], p[k * 3 + 1], p[k * 3 + 2], 1.0f}; }
};

__global__ __launch_bounds__(fps::kStreamThreads) void fps_stream_kernel(const float* __restrict__ xyz, int N, int m,
                                                          float* __restrict__ temp, int* __restrict__ idxs) {
  const int b = blockIdx.x;
  fps::stream_rounds(DenseSource{xyz + static_cast<size_t>(b) * N * 3}, N, m, temp + static_cast<size_t>(b) * N,
                     idxs + static_cast<size_t>(b) * m, nullptr);
}

}  // namespace

extern "C" int pdr_opt_n_threads(int work_size) {
  // cuda_utils.h:13-19, evaluated in double exactly like the reference host code
  if (work_size <= 0) return 1;
  const int pow_2 = static_cast<int>(log(static_cast<double>(work_size)) / log(2.0));
  int t = 1 << pow_2;
  if (t > 512) t = 512;
  if (t < 1) t = 1;
  return t;
}

extern "C" size_t pdr_fps_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0) return 0;
  // 3N floats of LDS must fit next to the exchange slots (160 KiB per workgroup)
  return (N <= 12288) ? 0 : static_cast<size_t>(B) * N * sizeof(float);
}

namespace {

// ---- the dispatch decision: ONE table of cells and ONE host function, read by the launch below and by pdr_fps_plan --
enum FpsFamily { kFpsResident = 0, kFpsWave = 1, kFpsLean = 2, kFpsStream = 3 };

// Every instantiation, once: X(family, kernel, T, PPT).  A cell carries T * PPT slots; inside a family the cells are in
// ascending size and plan_fps takes the first one that is large enough (wave: for the R Q rank slots, lean and
// resident: for the N points).  The launch switch is generated from the same list, so the plan cannot name a cell
// without a launch.
//
// Measured on MI355X, B = 32 (tools/lab/fps_time.py), us per call:
//                      2048->1024  1024->256  256->64  3072->1024
//   4 waves, barrier        490        105       25        566      (fps_resident_kernel, default above 256 slots)
//   1 wave, 32 slots/lane   696        121       20         --      (one wave issues <= 1 instruction / ~4-5 cycles)
//   4 waves, rank-ordered   532        127       20        665      (fewer VALU slots, but the round is a LATENCY
//                                                                    chain: LDS read -> update -> tree -> 2 DPP
//                                                                    reductions -> exchange -> index recovery)
// so the rank-ordered variant (fps_wave_kernel) is used where it wins (<= 256 slots: no barrier at all).
//   wave: rank-ordered slots + packed distances + tree arg-max: ONE wave while a lane holds <= 4 slots (no barrier at
//     all), four waves (one per SIMD: a single wave issues at most one instruction every ~4-5 cycles, measured 680 ns
//     per round with 32 slots per lane) above that;
//   lean: the instruction-lean resident kernel, an even number of points per thread;
//   resident: the round-1 kernel (512 / 1024 threads per cloud -- fewer points per thread against a wider exchange --,
//     round 5, us per call at B = 32: 2048->1024 492 / 525 / 885, 1024->256 105 / 124 / 215 for 256 / 512 / 1024
//     threads: not taken).
#define PDR_FPS_CELLS(X)                                                                                      \
  X(kFpsWave, fps_wave_kernel, 64, 2)        X(kFpsWave, fps_wave_kernel, 64, 4)                                \
  X(kFpsWave, fps_wave_kernel, 256, 2)       X(kFpsWave, fps_wave_kernel, 256, 4)                               \
  X(kFpsWave, fps_wave_kernel, 256, 8)       X(kFpsWave, fps_wave_kernel, 256, 16)                              \
  X(kFpsLean, fps_lean_kernel, 256, 2)       X(kFpsLean, fps_lean_kernel, 256, 4)                               \
  X(kFpsLean, fps_lean_kernel, 256, 8)       X(kFpsLean, fps_lean_kernel, 256, 12)                              \
  X(kFpsLean, fps_lean_kernel, 256, 16)                                                                         \
  X(kFpsResident, fps_resident_kernel, 64, 1)    X(kFpsResident, fps_resident_kernel, 64, 2)                    \
  X(kFpsResident, fps_resident_kernel, 256, 1)   X(kFpsResident, fps_resident_kernel, 256, 2)                   \
  X(kFpsResident, fps_resident_kernel, 256, 4)   X(kFpsResident, fps_resident_kernel, 256, 8)                   \
  X(kFpsResident, fps_resident_kernel, 256, 12)  X(kFpsResident, fps_resident_kernel, 256, 16)                  \
  X(kFpsResident, fps_resident_kernel, 1024, 8)  X(kFpsResident, fps_resident_kernel, 1024, 12)

struct FpsCell {
  int family, T, PPT;
};
#define PDR_FPS_CELL_ROW(FAMILY, KERNEL, T_, PPT_) {FAMILY, T_, PPT_},
constexpr FpsCell kFpsCells[] = {PDR_FPS_CELLS(PDR_FPS_CELL_ROW)};
#undef PDR_FPS_CELL_ROW

struct FpsPlan {
  int family, T, PPT;     // kernel family and its template parameters (stream: 1024 threads, PPT 0 = strided)
  int R, Rbits, Q;        // the reference's thread geometry: R = opt_n_threads(N), Q = ceil(N / R); tie rank < R Q
};

// Option fps_wave: 0 = never, 1 = where it wins (<= 256 slots), 2 = for every size up to 4096 slots (A/B and test
// runs).  Option fps_lean = 0: the round-1 resident kernel instead of the lean one.
int plan_fps(int N, FpsPlan* p) {
  if (N <= 0) return PDR_EINVAL;
  p->R = pdr_opt_n_threads(N);
  p->Rbits = 0;
  while ((1 << p->Rbits) < p->R) ++p->Rbits;
  p->Q = (N + p->R - 1) / p->R;
  if (pdr_fps_workspace_bytes(1, N) > 0) {
    p->family = kFpsStream, p->T = fps::kStreamThreads, p->PPT = 0;
    return PDR_OK;
  }
  const long slots = static_cast<long>(p->R) * p->Q;
  const int wave_mode = pdr::option(pdr::OPT_FPS_WAVE);
  const bool use_wave = wave_mode == 2 || (wave_mode == 1 && slots <= 256);
  // the wave and lean kernels keep the cloud in N * 16 bytes of dynamic LDS next to their static exchange slots: stay
  // inside the 64 KiB a launch gets without raising hipFuncAttributeMaxDynamicSharedMemorySize, else the resident kernel
  const bool fits64k = static_cast<size_t>(N) * sizeof(float4) + 256 <= 64 * 1024;
  static_assert(kMaxResidentN >= 12288, "resident path must cover the LDS-resident range");
  int family = kFpsResident;
  long size = N;
  if (use_wave && fits64k && slots <= 4096) family = kFpsWave, size = slots;
  else if (pdr::option(pdr::OPT_FPS_LEAN) != 0 && N > 128 && fits64k) family = kFpsLean;
  for (const FpsCell& c : kFpsCells)
    if (c.family == family && size <= static_cast<long>(c.T) * c.PPT) {
      p->family = c.family, p->T = c.T, p->PPT = c.PPT;
      return PDR_OK;
    }
  return PDR_EUNSUPPORTED;
}

// One launch for the three resident families: they share the argument list and differ in the kernel and its dynamic LDS.
using FpsKernel = void (*)(const float*, int, int, int, int, int, int*);
int launch_fps(FpsKernel kernel, const FpsPlan& p, const float* xyz, int B, int N, int m, int* idx, hipStream_t s) {
  // wave, lean: the cloud as float4 (static exchange slots); resident: 3 N floats and the exchange slots behind them
  const size_t lds = p.family != kFpsResident
                         ? static_cast<size_t>(N) * sizeof(float4)
                         : static_cast<size_t>((3 * N + 3) & ~3) * sizeof(float) +
                               2 * (p.T / 64) * sizeof(unsigned long long);
  // the attribute is per DEVICE: set it on every large launch (cheap host call, no global state), checked
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          160 * 1024) != hipSuccess)
    return PDR_ELAUNCH;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(p.T), lds, s, xyz, N, m, p.R, p.Rbits, p.Q, idx);
  return pdr::check_launch();
}

}  // namespace

// Which kernel pdr_furthest_point_sampling runs for a cloud of N points under the current fps_wave / fps_lean options
// (host only): out = {family (0 resident, 1 wave, 2 lean, 3 stream), T, PPT, slots = R Q}.
extern "C" int pdr_fps_plan(int N, int out[4]) {
  if (!out) return PDR_EINVAL;
  FpsPlan p;
  const int rc = plan_fps(N, &p);
  if (rc != PDR_OK) return rc;
  out[0] = p.family, out[1] = p.T, out[2] = p.PPT, out[3] = p.R * p.Q;
  return PDR_OK;
}

extern "C" int pdr_furthest_point_sampling(const float* xyz, int B, int N, int m,
                                           float* temp, int* idx, pdr_stream_t stream) {
  if (B < 0 || N <= 0 || m < 0) return PDR_EINVAL;
  if (B == 0 || m == 0) return PDR_OK;
  if (!xyz || !idx) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  FpsPlan p;
  const int rc = plan_fps(N, &p);
  if (rc != PDR_OK) return rc;
  if (p.family == kFpsStream) {
    if (!temp) return PDR_EINVAL;
    hipLaunchKernelGGL(fps_stream_kernel, dim3(B), dim3(fps::kStreamThreads), 0, s, xyz, N, m, temp, idx);
    return pdr::check_launch();
  }
#define PDR_FPS_RUN(FAMILY, KERNEL, T_, PPT_)                  \
  if (p.family == (FAMILY) && p.T == (T_) && p.PPT == (PPT_)) \
    return launch_fps(&KERNEL<T_, PPT_>, p, xyz, B, N, m, idx, s);
  PDR_FPS_CELLS(PDR_FPS_RUN)
#undef PDR_FPS_RUN
  return PDR_EUNSUPPORTED;
}
