// scatter_det.hip -- deterministic twins of the four scatter-add backward calls (gather / group / three_interpolate
// grads and the grad_y half of the kNN backward).
//
// The atomic twins (group_gather.hip, neighbors.hip) add every contribution where it lands; the order of the float
// adds is whatever the hardware makes of it.  Here the scatter is turned into a gather: an INVERSE INDEX lists, for
// every destination, its source positions in ascending order, and one thread (or, for a very long list, one lane of a
// wave) adds them in exactly that order in fp32 from +0.0f -- the order of the CPU oracle's sequential loops, so the
// result is the oracle's bit for bit and the same run after run.  Every output element is written exactly once.
//
// Builder (stable counting sort, per cloud; P source positions, N destinations, W <= 64 position ranges of R each):
//   1. rank   : wave w walks its range [w R, (w + 1) R) in ascending 64-position steps.  In a step, equal destinations
//               are ranked by lane with a ballot loop; the first lane of each group adds the group's size to
//               cnt[w][d] with an INTEGER atomic (only wave w ever touches row w, one step after the other, so the
//               value it gets back is the number of earlier positions of its range with that destination).
//               rank[pos] = positions before pos in range w with the same destination.
//   2. scan   : one workgroup per cloud turns cnt[.][d] into its exclusive prefix over w, scans the totals into
//               start[0 .. N] and lists the destinations with >= kLong sources in ascending order.
//   3. place  : order[start[d] + cnt[w][d] + rank[pos]] = pos, one thread per position -- every slot is a function of
//               the index array alone, so nothing depends on execution order.
// Sum:
//   4. short  : one thread per (destination, 8-channel slab) as in gather_rows_kernel (coalesced stores), segments
//               shorter than kLong.
//   5. long   : one wave per (listed destination, 64 channels), lane = channel: the adds of a segment stay serial and
//               in order, 64 channels advance per instruction (the empty-ball case: every slot of a ball query without
//               a hit names point 0).  The list is read 64 entries per coalesced load and handed on by readlane.
#include "pdr_common.h"

namespace {

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

// ---- 1. rank ---------------------------------------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(256) void rank_kernel(const IdxT* __restrict__ idx, int P, int N, int R, int W, int Wcap,
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
    const int d = pos < p1 ? dest_of(idx, static_cast<size_t>(b) * P + pos, N) : -1;
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
template <typename IdxT>
__global__ __launch_bounds__(256) void place_kernel(const IdxT* __restrict__ idx, int P, int N, int R, int Wcap,
                                                    const int* __restrict__ cnt, const int* __restrict__ start,
                                                    const int* __restrict__ rank, int* __restrict__ order) {
  const int b = blockIdx.y;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= P) return;
  const int d = dest_of(idx, static_cast<size_t>(b) * P + pos, N);
  if (d < 0) return;
  const int w = pos / R;
  const int slot = start[static_cast<size_t>(b) * (static_cast<size_t>(N) + 1) + d] +
                   cnt[(static_cast<size_t>(b) * Wcap + w) * N + d] + rank[static_cast<size_t>(b) * P + pos];
  order[static_cast<size_t>(b) * P + slot] = pos;         // slot < start[N] <= P
}

// ---- the addends -----------------------------------------------------------------------------------------------------
enum Op { kRows, kInterp, kKnn };

struct SumArgs {
  const float* go;   // rows / interp: grad_out (B, C, P) / (B, C, P / 3); kNN: grad_dists (B, P)
  const float* w;    // interp: weight (B, P)
  const float* x;    // kNN: queries (B, n1, 3)
  const float* y;    // kNN: cloud (B, N, 3)
  float* out;        // rows / interp: (B, C, N); kNN: (B, N, 3)
  int C, P, N, K, n1;
};

// the term that source position `pos` adds to channel c of destination d (products rounded before the add:
// the library is built with -ffp-contract=off)
template <int OP>
__device__ __forceinline__ float term(const SumArgs& a, int b, int c, int d, int pos) {
  if (OP == kRows) return a.go[(static_cast<size_t>(b) * a.C + c) * a.P + pos];
  if (OP == kInterp)
    return a.go[(static_cast<size_t>(b) * a.C + c) * (a.P / 3) + pos / 3] * a.w[static_cast<size_t>(b) * a.P + pos];
  const int j = pos / a.K;
  const float g = 2.0f * a.go[static_cast<size_t>(b) * a.P + pos];
  const float diff = a.x[(static_cast<size_t>(b) * a.n1 + j) * 3 + c] - a.y[(static_cast<size_t>(b) * a.N + d) * 3 + c];
  return -(g * diff);                                     // acc -= t and acc += -t are the same rounding
}

template <int OP>
__device__ __forceinline__ size_t out_index(const SumArgs& a, int b, int c, int d) {
  return OP == kKnn ? (static_cast<size_t>(b) * a.N + d) * 3 + c : (static_cast<size_t>(b) * a.C + c) * a.N + d;
}

// ---- 4. short segments: one thread per (destination, channel slab) ---------------------------------------------------
template <int OP>
__global__ __launch_bounds__(256) void sum_short_kernel(SumArgs a, const int* __restrict__ start,
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
      va[c] = c < cn ? term<OP>(a, b, c0 + c, d, pa) : 0.0f;
      vb[c] = (two && c < cn) ? term<OP>(a, b, c0 + c, d, pb) : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < kSlab; ++c) {
      acc[c] += va[c];
      if (two) acc[c] += vb[c];
    }
  }
#pragma unroll
  for (int c = 0; c < kSlab; ++c)
    if (c < cn) a.out[out_index<OP>(a, b, c0 + c, d)] = acc[c];
}

// ---- 5. long segments: one wave per (listed destination, 64 channels), lane = channel --------------------------------
template <int OP>
__global__ __launch_bounds__(64) void sum_long_kernel(SumArgs a, int max_long, const int* __restrict__ start,
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
        for (int u = 0; u < 16; ++u) v[u] = term<OP>(a, b, c, d, __builtin_amdgcn_readlane(mine, u0 + u));
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
      }
    } else {
      for (int u = 0; u < left; ++u) acc += term<OP>(a, b, c, d, __shfl(mine, u, 64));
    }
  }
  if (live) a.out[out_index<OP>(a, b, c, d)] = acc;
}

// grad_x of the kNN backward: knn_grad_kernel of neighbors.hip without its grad_y half (one thread per query, its K
// terms in registers, k ascending -- already order-fixed, the same bits)
__global__ __launch_bounds__(256) void knn_grad_x_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const int64_t* __restrict__ idx,
                                                         const float* __restrict__ gd, int n1, int n2, int K,
                                                         float* __restrict__ gx) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n1) return;
  const float* q = x + (static_cast<size_t>(b) * n1 + j) * 3;
  const float* p = y + static_cast<size_t>(b) * n2 * 3;
  const float qx = q[0], qy = q[1], qz = q[2];
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  for (int t = 0; t < K; ++t) {
    const int64_t k = idx[(static_cast<size_t>(b) * n1 + j) * K + t];
    if (k < 0 || k >= n2) continue;
    const float g = 2.0f * gd[(static_cast<size_t>(b) * n1 + j) * K + t];
    ax += g * (qx - p[k * 3 + 0]);
    ay += g * (qy - p[k * 3 + 1]);
    az += g * (qz - p[k * 3 + 2]);
  }
  float* o = gx + (static_cast<size_t>(b) * n1 + j) * 3;
  o[0] = ax;
  o[1] = ay;
  o[2] = az;
}

// sizes the kernels cannot index (decided before any pointer is looked at)
inline bool unsupported(long B, long P, long N) {
  return N > kMaxN || P > kMaxP || B > 65535 || B * P >= (1L << 31);
}

// builder + both sums on `s`; P > 0, sizes supported, pointers checked by the caller
template <int OP, typename IdxT>
int scatter_det(const IdxT* idx, int B, const SumArgs& a, void* workspace, hipStream_t s) {
  const int P = a.P, N = a.N;
  const Workspace ws = carve(workspace, B, P, N);
  const int R = range_len(P), W = ranges_for(P);
  if (hipMemsetAsync(workspace, 0, ws.zero_bytes, s) != hipSuccess) return pdr::check_launch();
  hipLaunchKernelGGL((rank_kernel<IdxT>), dim3((W + 3) / 4, B), dim3(256), 0, s, idx, P, N, R, W, ws.Wcap, ws.cnt,
                     ws.rank);
  hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(kScanThreads), 0, s, N, W, ws.Wcap, ws.max_long, ws.cnt, ws.start,
                     ws.nlong, ws.longlist);
  hipLaunchKernelGGL((place_kernel<IdxT>), dim3((P + 255) / 256, B), dim3(256), 0, s, idx, P, N, R, ws.Wcap, ws.cnt,
                     ws.start, ws.rank, ws.order);
  hipLaunchKernelGGL((sum_short_kernel<OP>), dim3((N + 255) / 256, (a.C + kSlab - 1) / kSlab, B), dim3(256), 0, s, a,
                     ws.start, ws.order);
  if (ws.max_long > 0)
    hipLaunchKernelGGL((sum_long_kernel<OP>), dim3(ws.max_long, (a.C + 63) / 64, B), dim3(64), 0, s, a, ws.max_long,
                       ws.start, ws.order, ws.nlong, ws.longlist);
  return pdr::check_launch();
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

int rows_det(const float* grad_out, const int* idx, int B, int C, int N, int P, float* grad_points, void* workspace,
             hipStream_t s) {
  if (unsupported(B, P, N)) return PDR_EUNSUPPORTED;
  if (!grad_points || (P > 0 && (!grad_out || !idx || !workspace || misaligned(workspace)))) return PDR_EINVAL;
  if (P == 0) {                                           // nothing to add: every element is +0.0
    if (hipMemsetAsync(grad_points, 0, sizeof(float) * static_cast<size_t>(B) * C * N, s) != hipSuccess)
      return pdr::check_launch();
    return PDR_OK;
  }
  SumArgs a = {};
  a.go = grad_out, a.out = grad_points, a.C = C, a.P = P, a.N = N;
  return scatter_det<kRows>(idx, B, a, workspace, s);
}

}  // namespace

extern "C" size_t pdr_scatter_workspace_bytes(int B, int P, int N) {
  if (B <= 0 || P < 0 || N <= 0 || unsupported(B, P, N)) return 0;
  return carve(nullptr, B, P, N).bytes;
}

extern "C" int pdr_gather_points_grad_det(const float* grad_out, const int* idx, int B, int C, int N, int m,
                                          float* grad_points, void* workspace, pdr_stream_t stream) {
  if (B < 0 || C < 0 || N <= 0 || m < 0) return PDR_EINVAL;
  if (B == 0 || C == 0) return PDR_OK;
  return rows_det(grad_out, idx, B, C, N, m, grad_points, workspace, pdr::as_stream(stream));
}

extern "C" int pdr_group_points_grad_det(const float* grad_out, const int* idx, int B, int C, int N, int np, int ns,
                                         float* grad_points, void* workspace, pdr_stream_t stream) {
  if (B < 0 || C < 0 || N <= 0 || np < 0 || ns < 0) return PDR_EINVAL;
  if (B == 0 || C == 0) return PDR_OK;
  const long P = static_cast<long>(np) * ns;
  if (P > kMaxP) return PDR_EUNSUPPORTED;
  return rows_det(grad_out, idx, B, C, N, static_cast<int>(P), grad_points, workspace, pdr::as_stream(stream));
}

extern "C" int pdr_three_interpolate_grad_det(const float* grad_out, const int* idx, const float* weight, int B, int C,
                                              int n, int m, float* grad_points, void* workspace,
                                              pdr_stream_t stream) {
  if (B < 0 || C < 0 || m <= 0 || n < 0) return PDR_EINVAL;
  if (B == 0 || C == 0) return PDR_OK;
  const long P = 3L * n;
  if (unsupported(B, P, m)) return PDR_EUNSUPPORTED;
  if (!grad_points || (n > 0 && (!grad_out || !idx || !weight || !workspace || misaligned(workspace))))
    return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  if (n == 0) {
    if (hipMemsetAsync(grad_points, 0, sizeof(float) * static_cast<size_t>(B) * C * m, s) != hipSuccess)
      return pdr::check_launch();
    return PDR_OK;
  }
  SumArgs a = {};
  a.go = grad_out, a.w = weight, a.out = grad_points, a.C = C, a.P = static_cast<int>(P), a.N = m;
  return scatter_det<kInterp>(idx, B, a, workspace, s);
}

extern "C" int pdr_knn_points_grad_det(const float* x, const float* y, const int64_t* idx, const float* grad_dists,
                                       int B, int n1, int n2, int K, float* grad_x, float* grad_y, void* workspace,
                                       pdr_stream_t stream) {
  if (B < 0 || n1 < 0 || n2 < 0 || K <= 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  const long P = static_cast<long>(n1) * K;
  if (unsupported(B, P, n2)) return PDR_EUNSUPPORTED;
  hipStream_t s = pdr::as_stream(stream);
  if (n2 > 0 && !grad_y) return PDR_EINVAL;
  if (n1 == 0) {
    if (n2 > 0 && hipMemsetAsync(grad_y, 0, sizeof(float) * static_cast<size_t>(B) * n2 * 3, s) != hipSuccess)
      return PDR_ELAUNCH;
    return PDR_OK;
  }
  if (!x || !idx || !grad_dists || !grad_x || (n2 > 0 && (!y || !workspace || misaligned(workspace))))
    return PDR_EINVAL;
  hipLaunchKernelGGL(knn_grad_x_kernel, dim3((n1 + 255) / 256, B), dim3(256), 0, s, x, y, idx, grad_dists, n1, n2, K,
                     grad_x);
  if (n2 == 0) return pdr::check_launch();
  SumArgs a = {};
  a.go = grad_dists, a.x = x, a.y = y, a.out = grad_y, a.C = 3, a.P = static_cast<int>(P), a.N = n2, a.K = K, a.n1 = n1;
  return scatter_det<kKnn>(idx, B, a, workspace, s);
}
