// scatter_index.h -- the inverse index that turns a scatter-add into an order-fixed gather, and the two ordered sums
// over it.  Shared by scatter_det.hip (the four *_grad_det calls), query_group_cf.hip (pdr_query_group_cf_grad) and
// knn_group_cf.hip (pdr_knn_group_cf_grad); everything here has internal linkage, each file gets its own copy of the
// kernels.
//
// An INVERSE INDEX lists, for every destination, its source positions in ascending order, and one thread (or, for a
// very long list, one lane of a wave) adds them in exactly that order in fp32 from +0.0f -- the order of the CPU
// oracle's sequential loops.  Every output element is written exactly once.
//
// Builder (stable counting sort, per cloud; P source positions, N destinations, W <= 64 position ranges of R each).
// The destination of a position comes from a functor `dest(i, N)` -> [0, N) or -1, i = b P + pos: a position with -1
// is in no list (kNN padding, an index outside [0, N), a slot of a patched query):
//   1. rank   : wave w walks its range [w R, (w + 1) R) in ascending 64-position steps.  In a step, equal destinations
//               are ranked by lane with a ballot loop; the first lane of each group adds the group's size to
//               cnt[w][d] with an INTEGER atomic (only wave w ever touches row w, one step after the other, so the
//               value it gets back is the number of earlier positions of its range with that destination).
//               rank[pos] = positions before pos in range w with the same destination.
//   2. scan   : one workgroup per cloud turns cnt[.][d] into its exclusive prefix over w, scans the totals into
//               start[0 .. N] and lists the destinations with >= kLong sources in ascending order.
//   3. place  : order[start[d] + cnt[w][d] + rank[pos]] = pos, one thread per position -- every slot is a function of
//               the index array alone, so nothing depends on execution order.
// Sum (the addend comes from an argument struct A: a.term(b, c, d, pos), a.out_at(b, c, d), a.C channels, a.P, a.N):
//   4. short  : one thread per (destination, 8-channel slab) as in gather_rows_kernel (coalesced stores), segments
//               shorter than kLong.
//   5. long   : one wave per (listed destination, 64 channels), lane = channel: the adds of a segment stay serial and
//               in order, 64 channels advance per instruction (the empty-ball case: every slot of a ball query without
//               a hit names point 0).  The list is read 64 entries per coalesced load and handed on by readlane.
#pragma once
#include "pdr_common.h"

namespace {
namespace scatter_index {

constexpr int kSlab = 8;          // channels per thread of the short sum (group_gather.hip's slab)
constexpr int kLong = 256;        // segments of at least this many sources go to the wave-per-destination kernel
constexpr int kMaxRanges = 64;    // W: position ranges (= rows of the count matrix) per cloud
constexpr int kMinSteps = 16;     // a range is at least 16 steps of 64 positions
constexpr int kScanThreads = 1024;
constexpr int kScanPer = 16;      // destinations per scan thread
constexpr int kMaxN = kScanThreads * kScanPer;   // 16384
constexpr int kMaxP = 1 << 22;

// positions per range: a multiple of 64, at least 1024, and such that ceil(P / R) <= kMaxRanges
inline int range_len(int P) {
  const int steps = (P + 64 * kMaxRanges - 1) / (64 * kMaxRanges);
  return 64 * (steps < kMinSteps ? kMinSteps : steps);
}
inline int ranges_for(int P) { return (P + range_len(P) - 1) / range_len(P); }
// rows of the count matrix the workspace holds: never fewer than ranges_for(P), and non-decreasing in P
inline int ranges_cap(int P) {
  const int w = (P + 64 * kMinSteps - 1) / (64 * kMinSteps);
  return w < kMaxRanges ? w : kMaxRanges;
}

// Workspace layout (int32 each; B clouds): cnt (B, Wcap, N) | nlong (B) | start (B, N + 1) | order (B, P) | rank (B, P)
// | longlist (B, P / kLong).  cnt and nlong lead so that one memset clears both.
struct Workspace {
  int *cnt, *nlong, *start, *order, *rank, *longlist;
  int Wcap, max_long;
  size_t zero_bytes, bytes;
};

inline Workspace carve(void* base, int B, int P, int N) {
  Workspace w;
  w.Wcap = ranges_cap(P);
  w.max_long = P / kLong;
  const size_t nb = static_cast<size_t>(B);
  const size_t o_nlong = nb * w.Wcap * N, o_start = o_nlong + nb, o_order = o_start + nb * (static_cast<size_t>(N) + 1),
               o_rank = o_order + nb * P, o_long = o_rank + nb * P, o_end = o_long + nb * w.max_long;
  w.zero_bytes = o_start * sizeof(int);
  w.bytes = o_end * sizeof(int);
  int* p = static_cast<int*>(base);
  w.cnt = p;
  if (p) w.nlong = p + o_nlong, w.start = p + o_start, w.order = p + o_order, w.rank = p + o_rank, w.longlist = p + o_long;
  else w.nlong = w.start = w.order = w.rank = w.longlist = nullptr;
  return w;
}

// sizes the kernels cannot index (decided before any pointer is looked at)
inline bool unsupported(long B, long P, long N) {
  return N > kMaxN || P > kMaxP || B > 65535 || B * P >= (1L << 31);
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// destination of a source position, or -1 for "no destination": the kNN padding slots, and any value outside [0, N)
// (never dereferenced, so a bad index cannot reach memory through these kernels)
__device__ __forceinline__ int dest_of(const int* idx, size_t i, int N) {
  const int d = idx[i];
  return (d >= 0 && d < N) ? d : -1;
}
__device__ __forceinline__ int dest_of(const int64_t* idx, size_t i, int N) {
  const int64_t d = idx[i];
  return (d >= 0 && d < N) ? static_cast<int>(d) : -1;
}

// the plain destination functor: position i of the flat (B, P) index array
template <typename IdxT>
struct IndexDest {
  const IdxT* idx;
  __device__ __forceinline__ int operator()(size_t i, int N) const { return dest_of(idx, i, N); }
};

// ---- 1. rank ---------------------------------------------------------------------------------------------------------
template <typename Dest>
__global__ __launch_bounds__(256) void rank_kernel(Dest dest, int P, int N, int R, int W, int Wcap,
                                                   int* __restrict__ cnt, int* __restrict__ rank) {
  const int b = blockIdx.y;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= W) return;                                     // whole waves leave together
  const int lane = pdr::lane_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  int* row = cnt + (static_cast<size_t>(b) * Wcap + w) * N;
  const int p0 = w * R;
  const int p1 = (p0 + R < P) ? p0 + R : P;
  for (int base = p0; base < p1; base += 64) {
    const int pos = base + lane;
    const int d = pos < p1 ? dest(static_cast<size_t>(b) * P + pos, N) : -1;
    // groups of equal destinations among the 64 lanes: rank inside the group, its size and its first lane
    unsigned long long todo = __ballot(d >= 0);
    int r = 0, size = 0, first = lane;
    while (todo) {
      const int lead = __ffsll(static_cast<long long>(todo)) - 1;
      const int dl = __shfl(d, lead, 64);
      const unsigned long long m = __ballot(d == dl);     // dl >= 0: only valid lanes match
      if (d == dl) {
        r = __popcll(m & below);
        size = __popcll(m);
        first = lead;
      }
      todo &= ~m;
    }
    int before = 0;
    if (d >= 0 && first == lane) before = atomicAdd(row + d, size);
    before = __shfl(before, first, 64);
    if (d >= 0) rank[static_cast<size_t>(b) * P + pos] = before + r;
  }
}

// ---- 2. scan ---------------------------------------------------------------------------------------------------------
// One workgroup per cloud; thread t owns the destinations [t E, (t + 1) E), E = ceil(N / 1024) <= 16.
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int N, int W, int Wcap, int max_long,
                                                            int* __restrict__ cnt, int* __restrict__ start,
                                                            int* __restrict__ nlong, int* __restrict__ longlist) {
  __shared__ unsigned long long sh[kScanThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const int E = (N + kScanThreads - 1) / kScanThreads;
  int* c = cnt + static_cast<size_t>(b) * Wcap * N;
  int tot[kScanPer];
  unsigned long long mine = 0;                            // (long segments << 32) | sources, of this thread's range
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    tot[k] = 0;
    const int d = t * E + k;
    if (k < E && d < N) {
      int run = 0;
      for (int w = 0; w < W; ++w) {
        const int v = c[static_cast<size_t>(w) * N + d];
        c[static_cast<size_t>(w) * N + d] = run;
        run += v;
      }
      tot[k] = run;
      mine += static_cast<unsigned long long>(run) + (run >= kLong ? (1ull << 32) : 0ull);
    }
  }
  // inclusive Hillis-Steele scan of the 1024 packed pairs (both halves stay far below 2^32: no carry between them)
  sh[t] = mine;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const unsigned long long add = t >= off ? sh[t - off] : 0ull;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const unsigned long long excl = sh[t] - mine;
  int s = static_cast<int>(excl & 0xffffffffull);
  int l = static_cast<int>(excl >> 32);
  int* st = start + static_cast<size_t>(b) * (static_cast<size_t>(N) + 1);
  int* ll = longlist + static_cast<size_t>(b) * max_long;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int d = t * E + k;
    if (k < E && d < N) {
      st[d] = s;
      s += tot[k];
      if (tot[k] >= kLong) ll[l++] = d;                   // l < max_long: every listed segment holds >= kLong of P sources
    }
  }
  if (t == kScanThreads - 1) {
    const unsigned long long all = sh[t];
    st[N] = static_cast<int>(all & 0xffffffffull);
    nlong[b] = static_cast<int>(all >> 32);
  }
}

// ---- 3. place --------------------------------------------------------------------------------------------------------
template <typename Dest>
__global__ __launch_bounds__(256) void place_kernel(Dest dest, int P, int N, int R, int Wcap,
                                                    const int* __restrict__ cnt, const int* __restrict__ start,
                                                    const int* __restrict__ rank, int* __restrict__ order) {
  const int b = blockIdx.y;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= P) return;
  const int d = dest(static_cast<size_t>(b) * P + pos, N);
  if (d < 0) return;
  const int w = pos / R;
  const int slot = start[static_cast<size_t>(b) * (static_cast<size_t>(N) + 1) + d] +
                   cnt[(static_cast<size_t>(b) * Wcap + w) * N + d] + rank[static_cast<size_t>(b) * P + pos];
  order[static_cast<size_t>(b) * P + slot] = pos;         // slot < start[N] <= P
}

// ---- 4. short segments: one thread per (destination, channel slab) ---------------------------------------------------
template <typename A>
__global__ __launch_bounds__(256) void sum_short_kernel(A a, const int* __restrict__ start,
                                                        const int* __restrict__ order) {
  const int b = blockIdx.z;
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= a.N) return;
  const int c0 = blockIdx.y * kSlab;
  const int cn = (a.C - c0) < kSlab ? (a.C - c0) : kSlab;
  const int* st = start + static_cast<size_t>(b) * (static_cast<size_t>(a.N) + 1);
  const int s0 = st[d], s1 = st[d + 1];
  if (s1 - s0 >= kLong) return;                           // sum_long_kernel writes this destination
  const int* ord = order + static_cast<size_t>(b) * a.P;
  float acc[kSlab];
#pragma unroll
  for (int c = 0; c < kSlab; ++c) acc[c] = 0.0f;
  for (int s = s0; s < s1; s += 2) {                      // two sources in flight; the adds stay in order
    const bool two = s + 1 < s1;
    const int pa = ord[s], pb = two ? ord[s + 1] : pa;
    float va[kSlab], vb[kSlab];
#pragma unroll
    for (int c = 0; c < kSlab; ++c) {
      va[c] = c < cn ? a.term(b, c0 + c, d, pa) : 0.0f;
      vb[c] = (two && c < cn) ? a.term(b, c0 + c, d, pb) : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < kSlab; ++c) {
      acc[c] += va[c];
      if (two) acc[c] += vb[c];
    }
  }
#pragma unroll
  for (int c = 0; c < kSlab; ++c)
    if (c < cn) a.out[a.out_at(b, c0 + c, d)] = acc[c];
}

// ---- 5. long segments: one wave per (listed destination, 64 channels), lane = channel --------------------------------
template <typename A>
__global__ __launch_bounds__(64) void sum_long_kernel(A a, int max_long, const int* __restrict__ start,
                                                      const int* __restrict__ order, const int* __restrict__ nlong,
                                                      const int* __restrict__ longlist) {
  const int b = blockIdx.z;
  if (static_cast<int>(blockIdx.x) >= nlong[b]) return;
  const int d = longlist[static_cast<size_t>(b) * max_long + blockIdx.x];
  const int lane = threadIdx.x;
  const bool live = blockIdx.y * 64 + lane < a.C;
  const int c = live ? blockIdx.y * 64 + lane : 0;        // lanes beyond C stay in the wave (they hand on list entries)
  const int* st = start + static_cast<size_t>(b) * (static_cast<size_t>(a.N) + 1);
  const int s0 = st[d], s1 = st[d + 1];
  const int* ord = order + static_cast<size_t>(b) * a.P;
  float acc = 0.0f;
  for (int s = s0; s < s1; s += 64) {
    // 64 list entries with one coalesced load, then handed to the whole wave one after the other
    const int left = s1 - s;
    const int mine = lane < left ? ord[s + lane] : 0;
    if (left >= 64) {
#pragma unroll
      for (int u0 = 0; u0 < 64; u0 += 16) {               // sixteen loads in flight, sixteen adds in order
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = a.term(b, c, d, __builtin_amdgcn_readlane(mine, u0 + u));
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
      }
    } else {
      for (int u = 0; u < left; ++u) acc += a.term(b, c, d, __shfl(mine, u, 64));
    }
  }
  if (live) a.out[a.out_at(b, c, d)] = acc;
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the builder on `s`: P > 0, sizes supported, the workspace non-NULL and 4-byte aligned (the caller checked)
template <typename Dest>
bool build(Dest dest, int B, int P, int N, const Workspace& ws, hipStream_t s) {
  const int R = range_len(P), W = ranges_for(P);
  if (hipMemsetAsync(ws.cnt, 0, ws.zero_bytes, s) != hipSuccess) return false;
  hipLaunchKernelGGL((rank_kernel<Dest>), dim3((W + 3) / 4, B), dim3(256), 0, s, dest, P, N, R, W, ws.Wcap, ws.cnt,
                     ws.rank);
  hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(kScanThreads), 0, s, N, W, ws.Wcap, ws.max_long, ws.cnt, ws.start,
                     ws.nlong, ws.longlist);
  hipLaunchKernelGGL((place_kernel<Dest>), dim3((P + 255) / 256, B), dim3(256), 0, s, dest, P, N, R, ws.Wcap, ws.cnt,
                     ws.start, ws.rank, ws.order);
  return true;
}

// both sums of one output over a built index; a.C > 0
template <typename A>
void sums(const A& a, int B, const Workspace& ws, hipStream_t s) {
  hipLaunchKernelGGL((sum_short_kernel<A>), dim3((a.N + 255) / 256, (a.C + kSlab - 1) / kSlab, B), dim3(256), 0, s, a,
                     ws.start, ws.order);
  if (ws.max_long > 0)
    hipLaunchKernelGGL((sum_long_kernel<A>), dim3(ws.max_long, (a.C + 63) / 64, B), dim3(64), 0, s, a, ws.max_long,
                       ws.start, ws.order, ws.nlong, ws.longlist);
}

}  // namespace scatter_index
}  // namespace
