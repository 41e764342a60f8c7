// occupancy.hip -- voxel-grid occupancy counters of a SET of clouds: pdr_occupancy_grid.
//
// Replaces the loop of entropy_of_occupancy_grid (reference pointnet2/models/pvd/metrics/evaluation_metrics.py:198-237):
// per cloud a KD-tree query of every point against the centres of an R^3 grid in [-0.5, 0.5]^3 (for the JSD: the 10 144
// of 28^3 centres inside the unit sphere), then two Python loops that add 1 per point to `grid_counters` and 1 per
// cloud and distinct cell to `grid_bernoulli_rvars`.  Here a workgroup owns a cloud: its per-cell point counts live in
// LDS, and when every point is binned each OCCUPIED cell issues one integer atomic add of its count into `counters` and
// one +1 into `bernoulli`.  Integer atomics only: the outputs do not depend on the order of arrival.
//
// THE NEAREST-CELL RULE (include/pdr_hip.h states it for callers).  The host passes the grid as data, built exactly as
// the reference builds it: axis[i] = float32(i * spacing - 0.5) and cell_of[(i R + j) R + k] = compact index of a kept
// cell or -1.  A point is widened to float64 and
//   1. per axis takes the index whose WIDENED float32 coordinate is nearest, |axis[i] - p| compared in float64 over the
//      R table values in ascending order with a strict <: the lower index wins a tie and points beyond the ends clamp.
//      The squared distance is a sum over the axes, so (i, j, k) is the nearest cell of the full grid;
//   2. if cell_of says that cell is kept, it is the answer (fast path);
//   3. else the answer is the kept cell of smallest float64 squared distance d = (dx dx + dy dy) + dz dz on the widened
//      differences (-ffp-contract=off: three products, two additions), the lowest index among equals.
// Step 3 is not rare (3 % of the points of a cloud uniform in the ball, 47 % in the cube, 60 % on the r = 0.5 shell).
// Its points are queued and the waves of the workgroup take them in turn, a wave per point.
//
// STEP 3 IS A PRUNED SEARCH WITH THE ARGMIN OF THE FULL SCAN.  A wave scans a BOX of cells [ilo, ihi] x [jlo, jhi] x
// [klo, khi], 64 cells at a time in ascending linear index (per lane a strict <), then a 6-level xor butterfly keeps
// the smaller (distance, linear index) pair; whether a cell is kept is one bit of an R^3-bit map in LDS.
//   a. boxes of half-width r = 1, 2, 3, 4, 6, 9, ... around the separable cell (clamped to the grid) until one holds a
//      kept cell; D = the smallest d in that box.
//   b. every cell with d <= D lies in the box F = { i : fl(dx dx) <= D } x { j : ... } x { k : ... }: floating-point
//      addition of non-negative terms is monotone, fl(a + b) >= a, so d >= fl(dx dx), fl(dy dy), fl(dz dz) for the very
//      values the scan computes.  The cell found in (a) is in F.  If F lies inside the box already scanned, every cell
//      outside that box has d > D and the pair found is the full scan's; otherwise F is scanned and its pair is.
// Both are the minimum of (d, linear index) over all kept cells, and the kept cells are numbered in ascending linear
// index, so "lowest linear index" is "lowest compact index".  A table that keeps no cell at all ends (a) with the box
// that covers the grid: the point goes to no cell and is counted in `skipped`.
//
// LDS (dynamic, one carve, every offset a multiple of 16; 12 560 B + 4 B per cell):
//     axd    32 doubles        the axis table, widened (8-byte stride: the 32 values cover the 64 banks once)
//     queue  1024 ints        points of the current pass whose separable cell is clipped
//     qcell  1024 ints        their separable cell, i << 10 | j << 5 | k
//     ctrl   4 ints           queue length, skipped points
//     kept   1024 words       bit L: cell_of[L] is a compact index in [0, cells)
//     counts cells ints       the cloud's points per cell
// 28^3 clipped: 53 136 B, two workgroups per CU by their 32 waves; 32^3 unclipped: 143 632 B, one.
// WORKGROUP: 1024 threads = 16 waves; a pass bins 1024 points (one per thread, coalesced 12-byte rows), then its 16
// waves drain the queue.  No value derived from a non-finite coordinate is ever used as an index: such a point is
// counted in `skipped` before step 1.
#include "pdr_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kHeadBytes = 32 * 8 + kThreads * 4 + kThreads * 4 + 16 + 1024 * 4;   // axd, queue, qcell, ctrl, kept
constexpr int kNone = 0x7fffffff;

// step 1 for one axis; p is finite.  All lanes read the same LDS address (broadcast).
__device__ __forceinline__ int nearest_axis(const double* __restrict__ axd, int R, double p) {
  int best = 0;
  double bd = __builtin_fabs(axd[0] - p);
  for (int i = 1; i < R; ++i) {
    const double d = __builtin_fabs(axd[i] - p);
    if (d < bd) {
      bd = d;
      best = i;
    }
  }
  return best;
}

struct Box {
  int lo[3], hi[3];
};

__device__ __forceinline__ bool inside(const Box& a, const Box& b) {   // a within b
  return a.lo[0] >= b.lo[0] && a.hi[0] <= b.hi[0] && a.lo[1] >= b.lo[1] && a.hi[1] <= b.hi[1] &&
         a.lo[2] >= b.lo[2] && a.hi[2] <= b.hi[2];
}

// The smallest (d, linear index) over the kept cells of a box, by one wave; uniform result, bL = kNone if none is kept.
__device__ __forceinline__ void scan_box(const unsigned* __restrict__ kept, const double* __restrict__ axd, int R,
                                         const Box& box, double px, double py, double pz, double& bd, int& bL) {
  const int wj = box.hi[1] - box.lo[1] + 1, wk = box.hi[2] - box.lo[2] + 1;
  const int wjk = wj * wk, W = (box.hi[0] - box.lo[0] + 1) * wjk;
  bd = __builtin_inf();
  bL = kNone;
  for (int t = pdr::lane_id(); t < W; t += 64) {                  // ascending t = ascending linear index per lane
    const int a = t / wjk, rem = t - a * wjk, b = rem / wk, c = rem - b * wk;
    const int i = box.lo[0] + a, j = box.lo[1] + b, k = box.lo[2] + c;
    const int L = (i * R + j) * R + k;
    if ((kept[L >> 5] >> (L & 31)) & 1u) {
      const double dx = axd[i] - px, dy = axd[j] - py, dz = axd[k] - pz;
      const double d = dx * dx + dy * dy + dz * dz;
      if (d < bd) {
        bd = d;
        bL = L;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double od = __shfl_xor(bd, off, 64);
    const int oL = __shfl_xor(bL, off, 64);
    if (od < bd || (od == bd && oL < bL)) {
      bd = od;
      bL = oL;
    }
  }
}

// { i : fl((axd[i] - p)^2) <= D } as an index range; not empty when D is the distance of a cell.  One wave.
__device__ __forceinline__ void axis_range(const double* __restrict__ axd, int R, double p, double D, int& lo, int& hi) {
  const int l = pdr::lane_id();
  const double dx = axd[l & 31] - p;
  const unsigned long long m = __ballot(l < R && dx * dx <= D);
  lo = m ? __builtin_ctzll(m) : 0;
  hi = m ? 63 - __builtin_clzll(m) : R - 1;
}

__global__ __launch_bounds__(kThreads) void occupancy_kernel(const float* __restrict__ clouds,
                                                             const int64_t* __restrict__ lengths, int n, int R,
                                                             const float* __restrict__ axis,
                                                             const int32_t* __restrict__ cell_of, int cells,
                                                             int32_t* __restrict__ counters,
                                                             int32_t* __restrict__ bernoulli,
                                                             int32_t* __restrict__ skipped) {
  extern __shared__ __attribute__((aligned(16))) unsigned char occ_smem[];
  double* axd = reinterpret_cast<double*>(occ_smem);
  int* queue = reinterpret_cast<int*>(occ_smem + 32 * 8);
  int* qcell = queue + kThreads;
  int* ctrl = qcell + kThreads;
  unsigned* kept = reinterpret_cast<unsigned*>(ctrl + 4);
  int* counts = reinterpret_cast<int*>(kept + 1024);

  const int s = blockIdx.x;
  const int len = pdr::cloud_len(lengths, s, n);
  if (len == 0) return;                                          // uniform: an empty cloud touches nothing
  const float* cloud = clouds + static_cast<size_t>(s) * n * 3;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R3 = R * R * R;

  if (tid < 32) axd[tid] = static_cast<double>(axis[tid < R ? tid : R - 1]);
  if (tid < 4) ctrl[tid] = 0;
  for (int c = tid; c < cells; c += kThreads) counts[c] = 0;
  // the kept-cell bit map: a wave covers 64 consecutive linear indices per step, lane 0 stores their two words
  for (int L0 = wave * 64; L0 < R3; L0 += kThreads) {
    const int L = L0 + lane;
    const bool k = L < R3 && static_cast<unsigned>(cell_of[L < R3 ? L : 0]) < static_cast<unsigned>(cells);
    const unsigned long long m = __ballot(k);
    if (lane == 0) {
      kept[L0 >> 5] = static_cast<unsigned>(m);
      kept[(L0 >> 5) + 1] = static_cast<unsigned>(m >> 32);
    }
  }
  __syncthreads();

  int my_skipped = 0;
  for (int p0 = 0; p0 < len; p0 += kThreads) {
    const int pi = p0 + tid;
    if (pi < len) {
      const float* row = cloud + static_cast<size_t>(pi) * 3;
      const float x = row[0], y = row[1], z = row[2];
      if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) {
        const int i = nearest_axis(axd, R, static_cast<double>(x));
        const int j = nearest_axis(axd, R, static_cast<double>(y));
        const int k = nearest_axis(axd, R, static_cast<double>(z));
        const int L = (i * R + j) * R + k;
        if ((kept[L >> 5] >> (L & 31)) & 1u) {
          atomicAdd(&counts[cell_of[L]], 1);
        } else {
          const int q = atomicAdd(&ctrl[0], 1);                  // at most one entry per thread and pass
          queue[q] = pi;
          qcell[q] = i << 10 | j << 5 | k;
        }
      } else {
        ++my_skipped;
      }
    }
    __syncthreads();
    const int qn = ctrl[0];
    for (int q = wave; q < qn; q += kWaves) {
      const float* pt = cloud + static_cast<size_t>(queue[q]) * 3;   // wave-uniform
      const double px = static_cast<double>(pt[0]), py = static_cast<double>(pt[1]), pz = static_cast<double>(pt[2]);
      const int c0[3] = {qcell[q] >> 10, (qcell[q] >> 5) & 31, qcell[q] & 31};
      Box box;
      double bd;
      int bL;
      for (int r = 1;; r += r < 2 ? 1 : r >> 1) {                 // (a): 1, 2, 3, 4, 6, 9, 13, 19, 28, 42
        bool whole = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          box.lo[a] = c0[a] - r > 0 ? c0[a] - r : 0;
          box.hi[a] = c0[a] + r < R - 1 ? c0[a] + r : R - 1;
          whole = whole && box.lo[a] == 0 && box.hi[a] == R - 1;
        }
        scan_box(kept, axd, R, box, px, py, pz, bd, bL);
        if (bL != kNone || whole) break;
      }
      if (bL != kNone) {                                           // (b)
        Box f;
        axis_range(axd, R, px, bd, f.lo[0], f.hi[0]);
        axis_range(axd, R, py, bd, f.lo[1], f.hi[1]);
        axis_range(axd, R, pz, bd, f.lo[2], f.hi[2]);
        if (!inside(f, box)) scan_box(kept, axd, R, f, px, py, pz, bd, bL);
      }
      if (lane == 0) {
        if (bL != kNone)
          atomicAdd(&counts[cell_of[bL]], 1);
        else
          atomicAdd(&ctrl[1], 1);                                // a table without one kept cell: the point goes nowhere
      }
    }
    __syncthreads();                                             // the queue has been read
    if (tid == 0) ctrl[0] = 0;
    __syncthreads();
  }

  if (my_skipped) atomicAdd(&ctrl[1], my_skipped);
  __syncthreads();
  for (int c = tid; c < cells; c += kThreads) {
    const int v = counts[c];
    if (v > 0) {
      atomicAdd(&counters[c], v);
      atomicAdd(&bernoulli[c], 1);
    }
  }
  if (tid == 0 && skipped && ctrl[1] > 0) atomicAdd(skipped, ctrl[1]);
}

}  // namespace

extern "C" int pdr_occupancy_grid(const float* clouds, const int64_t* lengths, int S, int n, int R, const float* axis,
                                  const int32_t* cell_of, int cells, int32_t* counters, int32_t* bernoulli,
                                  int32_t* skipped, pdr_stream_t stream) {
  if (S < 0 || n < 0 || R < 0 || cells < 0) return PDR_EINVAL;
  if (S == 0) return PDR_OK;
  if (n <= 0 || cells <= 0) return PDR_EINVAL;
  if (!clouds || !axis || !cell_of || !counters || !bernoulli) return PDR_EINVAL;
  if (R < 2 || R > 32 || cells > R * R * R) return PDR_EUNSUPPORTED;
  if (static_cast<long long>(S) * n >= (1ll << 31)) return PDR_EUNSUPPORTED;
  const size_t lds = (kHeadBytes + static_cast<size_t>(cells) * 4 + 15) / 16 * 16;      // <= 143 632
  // the attribute is per DEVICE: set it on every large launch (cheap host call, no global state), checked
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&occupancy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          160 * 1024) != hipSuccess)
    return PDR_ELAUNCH;
  hipLaunchKernelGGL(occupancy_kernel, dim3(static_cast<unsigned>(S)), dim3(kThreads), lds, pdr::as_stream(stream),
                     clouds, lengths, n, R, axis, cell_of, cells, counters, bernoulli, skipped);
  return pdr::check_launch();
}
