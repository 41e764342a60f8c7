// nn1_scan.h -- the packed K = 1 nearest-neighbour scan of a 256-thread workgroup.
// The definition behind chamfer_loss_kernel (chamfer_loss.hip) and direction_sum (chamfer_pairs.hip), whose per-point
// minima and indices must have the bits of pdr_chamfer_nn (include/pdr_hip.h).  nn1_kernel (neighbors.hip:
// pdr_chamfer_nn, the K = 1 route of pdr_knn_points, and their ragged forms) takes kTile, kChunk and f32x2 from here
// but spells the same scan out in its own body, for the launch time measured there: keep the two equal.
//
// chamfer_loss_new.py:149-167 asks knn_points(K=1) twice (x -> y and y -> x); 8.39 M pair evaluations per
// 2048^2 cloud pair, so the search is bound by VALU ISSUE SLOTS per pair, not by memory.  The generic kernel of
// neighbors.hip spends ~9 slots per pair (6 distance + compare + 2 selects) plus one LDS read.  Here:
//   * a thread owns 2 QP queries held as QP float PAIRS: the distance expression runs on packed fp32
//     (v_pk_add / v_pk_mul / v_pk_fma: two queries per instruction, each lane IEEE-exact, same ACC3 expression
//     tree as the generic kernel -> bit-identical distances);
//   * the candidate cloud streams through LDS in kTile-point float4 tiles every lane reads at the SAME address: every
//     LDS point (one ds_read, broadcast) serves all 2 QP queries;
//   * no per-pair index bookkeeping: per chunk of kChunk points only the running minimum (v_min / v_min3) is kept,
//     and once per chunk `chunk_min < best` (STRICT) records the chunk; when the scan is over the ONE recorded
//     chunk of each query is rescanned in ascending order with strict `<`, which returns the first (lowest-index)
//     point attaining the minimum = "first minimum wins" (chamfer3D.cu:26-129, pdr_hip.h knn contract).
// ~4 issue slots per pair; 3.5 without TRACK, where no chunk is recorded and the minimum goes straight into `best`
// (gfx950 has no packed fp32 minimum: the compiler folds two candidates into one v_min3_f32 per query).  The minima of
// the two forms are the minimum of the same set of non-NaN, non-negative values: the same bits.
#pragma once
#include "pdr_common.h"

namespace pdr {

constexpr int kTile = 1024;    // candidate points per LDS tile
constexpr int kChunk = 8;      // candidates per unrolled step; tiles are padded to a multiple with +inf points

typedef float f32x2 __attribute__((ext_vector_type(2)));

// The 2 QP queries of a thread: slot s is half s & 1 of pair s >> 1.
template <int QP>
struct Nn1State {
  f32x2 x[QP], y[QP], z[QP];
  f32x2 best[QP];      // running minimum; +inf: no candidate with a non-NaN distance
  int chunk[2 * QP];   // TRACK: first point of the earliest chunk holding `best`
};

// Slot s takes row q0 + 256 s of q (coalesced over the workgroup when q0 = first row + threadIdx.x); slots past row
// `last` shadow row max(last, 0), whose results the caller drops.
template <int QP>
__device__ __forceinline__ void nn1_load(Nn1State<QP>& st, const float* q, int q0, int last) {
#pragma unroll
  for (int p = 0; p < QP; ++p) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* r = q + static_cast<size_t>(max(min(q0 + 256 * (2 * p + h), last), 0)) * 3;
      st.x[p][h] = r[0];
      st.y[p][h] = r[1];
      st.z[p][h] = r[2];
    }
  }
}

// best (and with TRACK chunk) of every slot over the candidates c[0 .. nc); nc = 0 scans nothing.  Called by all 256
// threads with the same c, nc and tile (kTile float4 of LDS).
template <int QP, bool TRACK>
__device__ __forceinline__ void nn1_scan(Nn1State<QP>& st, const float* c, int nc,
                                         float4* __restrict__ tile) {
  static_assert(kTile % kChunk == 0, "a padded tile fits the LDS array");
#pragma unroll
  for (int p = 0; p < QP; ++p) {
    st.best[p] = f32x2{__builtin_inff(), __builtin_inff()};
    st.chunk[2 * p] = st.chunk[2 * p + 1] = 0;
  }
  for (int k0 = 0; k0 < nc; k0 += kTile) {
    const int kn = (nc - k0) < kTile ? (nc - k0) : kTile;
    const int kpad = (kn + kChunk - 1) / kChunk * kChunk;
    __syncthreads();
    for (int t = threadIdx.x; t < kpad; t += 256) {
      const float* s = c + static_cast<size_t>(k0 + min(t, kn - 1)) * 3;
      // slots beyond the cloud: +inf coordinates -> distance +inf, never below any minimum
      tile[t] = t < kn ? make_float4(s[0], s[1], s[2], 0.0f)
                       : make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.0f);
    }
    __syncthreads();
    for (int t0 = 0; t0 < kpad; t0 += kChunk) {
      f32x2 cm[QP];
#pragma unroll
      for (int p = 0; p < QP; ++p) cm[p] = TRACK ? f32x2{__builtin_inff(), __builtin_inff()} : st.best[p];
#pragma unroll
      for (int u = 0; u < kChunk; ++u) {
        const float4 pt = tile[t0 + u];
#pragma unroll
        for (int p = 0; p < QP; ++p) {
          const f32x2 dx = st.x[p] - pt.x, dy = st.y[p] - pt.y, dz = st.z[p] - pt.z;
          f32x2 d = dx * dx;                                   // PDR_ACC3 on both halves of the pair
          d = __builtin_elementwise_fma(dy, dy, d);
          d = __builtin_elementwise_fma(dz, dz, d);
          cm[p] = __builtin_elementwise_min(cm[p], d);
        }
      }
#pragma unroll
      for (int p = 0; p < QP; ++p) {
        if constexpr (!TRACK) {
          st.best[p] = cm[p];
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bool up = cm[p][h] < st.best[p][h];          // strict: the EARLIEST chunk holding the minimum
            st.best[p][h] = up ? cm[p][h] : st.best[p][h];
            st.chunk[2 * p + h] = up ? k0 + t0 : st.chunk[2 * p + h];
          }
        }
      }
    }
  }
}

struct Nn1Hit {
  float d;   // the minimum; +inf with i = -1
  int i;     // the first candidate attaining it; -1: no candidate (nc = 0, or no non-NaN distance)
};

// Index recovery for slot s after a TRACK scan over c[0 .. nc): the recorded chunk is rescanned from global memory
// (kChunk points, ascending, strict <).
template <int QP>
__device__ __forceinline__ Nn1Hit nn1_recover(const Nn1State<QP>& st, int s, const float* c, int nc) {
  const float x0 = st.x[s >> 1][s & 1], y0 = st.y[s >> 1][s & 1], z0 = st.z[s >> 1][s & 1];
  const float* chunk = c + static_cast<size_t>(st.chunk[s]) * 3;
  Nn1Hit hit{__builtin_inff(), -1};
  for (int u = 0; u < kChunk; ++u) {
    const int k = st.chunk[s] + u;
    if (k < nc) {
      const float* r = chunk + 3 * u;
      const float dx = x0 - r[0], dy = y0 - r[1], dz = z0 - r[2];
      const float d = PDR_ACC3(dx, dy, dz);
      if (d < hit.d) {
        hit.d = d;
        hit.i = k;
      }
    }
  }
  return hit;
}

// N sums over the 256 threads of a workgroup at once, returned in every thread; wsum: 4 N floats of LDS.  The order is
// part of what the callers document: the 64 values of a wave by an xor butterfly (6 levels), the 4 wave sums as
// (w0 + w1) + (w2 + w3).
template <int N>
__device__ __forceinline__ void block_sum_256(float (&v)[N], float* __restrict__ wsum) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum_f32(v[i]);
  __syncthreads();                                               // wsum of the previous sum has been read
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) wsum[4 * i + (threadIdx.x >> 6)] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (wsum[4 * i] + wsum[4 * i + 1]) + (wsum[4 * i + 2] + wsum[4 * i + 3]);
}

}  // namespace pdr
