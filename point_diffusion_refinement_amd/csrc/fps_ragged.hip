// fps_ragged.hip -- furthest point sampling of a padded batch with per-cloud lengths, optionally of the cloud AND its
// mirror image, writing the picked rows itself (pdr_furthest_point_sampling_ragged of include/pdr_hip.h).
//
// Cloud b is a VIRTUAL cloud of V_b = L_b (no mirror) or 2 L_b points: virtual point k < L_b is xyz[b,k], virtual point
// k >= L_b is xyz[b,k-L_b] with the sign bit of one coordinate flipped.  Nothing of size 2N exists: a thread builds its
// virtual points in registers once, and the last pick is read back from the L_b originals in LDS.
//
// Tie order.  pdr_furthest_point_sampling (fps.hip) ranks point k of an N-point cloud by
//     bitrev(k % R) * ceil(N / R) + k / R,   R = opt_n_threads(N),
// which for EVERY N is the order of the lexicographic key (bitrev9(k % 512), k / 512): one key serves every length of a
// batch, and no per-cloud thread geometry is needed.  Here  rank = bitrev9(k & 511) << QB | k >> 9  with QB bits for
// k >> 9 (5 in the resident kernels: k < 16384; 23 in the stream form, fps::stream_rounds, shared with fps.hip).
//
// Resident form (V <= 12288): fps_lean_kernel's round from the same pieces of fps_round.h -- LDS read of the last pick,
// FPS_PACKED_UPDATE, in-lane arg-max, fps::wave_argmax, fps::exchange_max (one barrier) -- with two changes:
//   * thread t owns the points k = t + i T.  With T a divisor or a multiple of 512 the tie order of a thread's own
//     points is a COMPILE-TIME permutation of i (slot_point below), so the slots are laid out in that order, need no
//     sorting and no per-slot key register: the in-lane scan tracks the winning i as an immediate and the key of the
//     one winner is computed after the scan;
//   * a launch is instantiated for the batch's stride (T threads, at most PPT points per thread), but every workgroup
//     runs the round loop built for ITS cloud: ceil(V_b / T) points per thread rounded up to 2, 4, 8, 12 or 16.  A cloud
//     much shorter than N does not pay for N.
#include "fps_round.h"

namespace {

using fps::f2;
using VPoint = fps::Point;

constexpr int kResidentMaxV = 12288;      // 3 floats per ORIGINAL point in LDS next to the exchange slots (160 KiB)
constexpr long kMaxV = 1l << 20;          // the ABI's bound on a virtual cloud (PDR_EUNSUPPORTED above it)

constexpr int brev_const(int v, int bits) {
  int r = 0;
  for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1) << (bits - 1 - i);
  return r;
}
// The i (point k = tid + i T) held by slot s of a thread with PPT points, slots in ascending tie rank.
//   T >= 512 (a multiple of 512): k & 511 is the same for all of a thread's points and k >> 9 grows with i.
//   T < 512 (G = 512 / T): k & 511 = tid + (i % G) T -> bitrev9 = bitrev9(tid) + bitrev_G(i % G), and k >> 9 = i / G.
template <int T, int PPT>
constexpr int slot_point(int s) {
  if (T >= 512) return s;
  constexpr int G = T >= 512 ? 1 : 512 / T;
  int gb = 0;
  while ((1 << gb) < G) ++gb;
  int n = 0;
  for (int r = 0; r < G; ++r)
    for (int i = brev_const(r, gb); i < PPT; i += G) {
      if (n == s) return i;
      ++n;
    }
  return 0;
}
template <int T, int PPT, int S>
struct SlotPoint {
  static constexpr int value = slot_point<T, PPT>(S);
};

__device__ __forceinline__ float flip_if(float v, bool flip) {
  return __uint_as_float(__float_as_uint(v) ^ (flip ? 0x80000000u : 0u));
}

// virtual point `k` of a cloud whose L originals are at sx / sy / sz[i * STRIDE] (k < V is the caller's business):
// STRIDE 1 for the planes in LDS, 3 for the rows in global memory
template <int STRIDE = 1>
__device__ __forceinline__ VPoint virtual_point(const float* sx, const float* sy, const float* sz, int k, int L,
                                                int axis) {
  const bool mir = k >= L;
  const int src = mir ? k - L : k;
  VPoint v;
  v.x = flip_if(sx[src * STRIDE], mir && axis == 0);
  v.y = flip_if(sy[src * STRIDE], mir && axis == 1);
  v.z = flip_if(sz[src * STRIDE], mir && axis == 2);
  v.tag = mir ? -1.0f : 1.0f;
  return v;
}

template <int T, int PPT, int S>
__device__ __forceinline__ void scan_slots(const f2 (&tmp)[PPT / 2], float& best, unsigned& besti) {
  if constexpr (S < PPT) {
    const float v = tmp[S >> 1][S & 1];
    const bool gt = v > best;
    best = gt ? v : best;
    besti = gt ? static_cast<unsigned>(SlotPoint<T, PPT, S>::value) : besti;
    scan_slots<T, PPT, S + 1>(tmp, best, besti);
  }
}
template <int T, int PPT, int S>
__device__ __forceinline__ void load_slots(f2 (&px)[PPT / 2], f2 (&py)[PPT / 2], f2 (&pz)[PPT / 2],
                                           f2 (&tmp)[PPT / 2], const float* sx, const float* sy, const float* sz,
                                           int tid, int L, int V, int axis) {
  if constexpr (S < PPT) {
    const int k = tid + SlotPoint<T, PPT, S>::value * T;
    const bool valid = k < V;
    const VPoint v = virtual_point(sx, sy, sz, valid ? k : 0, L, axis);
    const float mag = PDR_SUM3(v.x, v.y, v.z);
    px[S >> 1][S & 1] = valid ? v.x : 0.0f;
    py[S >> 1][S & 1] = valid ? v.y : 0.0f;
    pz[S >> 1][S & 1] = valid ? v.z : 0.0f;
    tmp[S >> 1][S & 1] = FPS_INITIAL_DISTANCE(mag, !valid);   // beyond the cloud: as an excluded point
    load_slots<T, PPT, S + 1>(px, py, pz, tmp, sx, sy, sz, tid, L, V, axis);
  }
}

// all m rounds of one cloud with PPT points per thread (V <= T PPT)
template <int T, int PPT>
__device__ __forceinline__ void ragged_rounds(const float* sx, const float* sy, const float* sz,
                                              unsigned long long* slots, int L, int V, int axis, int m,
                                              int* __restrict__ out, float4* __restrict__ rows) {
  static_assert(PPT % 2 == 0, "points are updated in pairs");
  constexpr int W = T / 64;
  constexpr int G = PPT / 2;
  const int tid = threadIdx.x;
  f2 px[G], py[G], pz[G], tmp[G];
  load_slots<T, PPT, 0>(px, py, pz, tmp, sx, sy, sz, tid, L, V, axis);

  int old = 0;
  if (tid == 0) out[0] = 0;
  for (int j = 1; j < m; ++j) {
    const VPoint c = virtual_point(sx, sy, sz, old, L, axis);
    if (tid == 0 && rows) rows[j - 1] = make_float4(c.x, c.y, c.z, c.tag);
    // distance updates in groups of at most 4 pairs (a workgroup of 1024 threads has 128 VGPRs per lane: the
    // temporaries of all pairs at once do not fit)
    FPS_PACKED_UPDATE(G, (G < 4 ? G : 4), px, py, pz, tmp, c.x, c.y, c.z)
    // first strictly greater in slot order = in tie order
    float best = -1.0f;
    unsigned besti = 0u;
    scan_slots<T, PPT, 0>(tmp, best, besti);
    const unsigned k = static_cast<unsigned>(tid) + besti * T;
    const unsigned rank = (__brev(k & 511u) >> 23 << 5) | (k >> 9);
    const unsigned low = ((0xFFFFu - rank) << 16) | k;         // larger = preferred
    unsigned long long key = fps::wave_argmax(best, low);
    key = fps::exchange_max<W>(slots + (j & 1) * W, key);
    old = static_cast<int>(key & 0xFFFFull);                   // no candidate at all: key 0 -> index 0, as the reference
    if (tid == 0) out[j] = old;
  }
  if (tid == 0 && rows) {
    const VPoint c = virtual_point(sx, sy, sz, old, L, axis);
    rows[m - 1] = make_float4(c.x, c.y, c.z, c.tag);
  }
}

// a cloud of length 0: idx = -1, rows = 0 in every slot
__device__ __forceinline__ void write_empty(int* __restrict__ out, float4* __restrict__ rows, int m, int tid, int T) {
  for (int j = tid; j < m; j += T) {
    out[j] = -1;
    if (rows) rows[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

template <int T, int PPT>
__global__ __launch_bounds__(T) void fps_ragged_resident_kernel(const float* __restrict__ xyz,
                                                                const int64_t* __restrict__ lengths, int N, int axis,
                                                                int m, int* __restrict__ idxs,
                                                                float4* __restrict__ rows4) {
  extern __shared__ __attribute__((aligned(16))) float fpr_smem[];
  float* sx = fpr_smem;
  float* sy = fpr_smem + N;
  float* sz = fpr_smem + 2 * N;
  // exchange slots: 2 parities x W waves (u64), 16-B aligned behind the cloud
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(fpr_smem + ((3 * N + 3) & ~3));
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = pdr::cloud_len(lengths, b, N);
  const int V = axis >= 0 ? 2 * L : L;
  int* out = idxs + static_cast<size_t>(b) * m;
  float4* rows = rows4 ? rows4 + static_cast<size_t>(b) * m : nullptr;
  if (L == 0) {
    write_empty(out, rows, m, tid, T);
    return;
  }
  const float* p = xyz + static_cast<size_t>(b) * N * 3;
  for (int i = tid; i < L; i += T) {
    sx[i] = p[i * 3 + 0];
    sy[i] = p[i * 3 + 1];
    sz[i] = p[i * 3 + 2];
  }
  __syncthreads();
  const int need = (V + T - 1) / T;                            // uniform in the workgroup; <= PPT by the host's plan
  if (need <= 2) {
    ragged_rounds<T, 2>(sx, sy, sz, slots, L, V, axis, m, out, rows);
    return;
  }
  if constexpr (PPT >= 4)
    if (need <= 4) {
      ragged_rounds<T, 4>(sx, sy, sz, slots, L, V, axis, m, out, rows);
      return;
    }
  if constexpr (PPT >= 8)
    if (need <= 8) {
      ragged_rounds<T, 8>(sx, sy, sz, slots, L, V, axis, m, out, rows);
      return;
    }
  if constexpr (PPT >= 12)
    if (need <= 12) {
      ragged_rounds<T, 12>(sx, sy, sz, slots, L, V, axis, m, out, rows);
      return;
    }
  if constexpr (PPT >= 16) ragged_rounds<T, 16>(sx, sy, sz, slots, L, V, axis, m, out, rows);
}

// Streaming form for V > kResidentMaxV: fps::stream_rounds on the virtual cloud built from the rows in global memory,
// running distances in the caller's temp (row stride = the batch's V).  Kept simple.
struct VirtualSource {
  const float* __restrict__ p;
  int L, axis;
  __device__ __forceinline__ VPoint point(int k) const { return virtual_point<3>(p, p + 1, p + 2, k, L, axis); }
};

__global__ __launch_bounds__(fps::kStreamThreads) void fps_ragged_stream_kernel(const float* __restrict__ xyz,
                                                                 const int64_t* __restrict__ lengths, int N, int axis,
                                                                 int m, float* __restrict__ temp,
                                                                 int* __restrict__ idxs, float4* __restrict__ rows4) {
  const int b = blockIdx.x;
  const int L = pdr::cloud_len(lengths, b, N);
  int* out = idxs + static_cast<size_t>(b) * m;
  float4* rows = rows4 ? rows4 + static_cast<size_t>(b) * m : nullptr;
  if (L == 0) {
    write_empty(out, rows, m, threadIdx.x, fps::kStreamThreads);
    return;
  }
  fps::stream_rounds(VirtualSource{xyz + static_cast<size_t>(b) * N * 3, L, axis}, axis >= 0 ? 2 * L : L, m,
                     temp + static_cast<size_t>(b) * N * (axis >= 0 ? 2 : 1), out, rows);
}

// ---- the dispatch decision: ONE host function, read by the launch and by pdr_fps_ragged_plan -------------------------
enum { kRaggedResident = 0, kRaggedStream = 1 };

struct RaggedPlan {
  int family, T, PPT;
  size_t lds;
};

// every resident instantiation, once: X(T, PPT), V <= T PPT, ascending.  plan_ragged takes the first cell that is large
// enough and the launch switch is generated from the same list.
#define PDR_FPS_RAGGED_CELLS(X) X(64, 2) X(256, 16) X(1024, 12)
#define PDR_FPS_RAGGED_ROW(T_, PPT_) {T_, PPT_},
constexpr int kRaggedCells[][2] = {PDR_FPS_RAGGED_CELLS(PDR_FPS_RAGGED_ROW)};
#undef PDR_FPS_RAGGED_ROW

bool plan_ragged(int N, int mirror_axis, RaggedPlan* p) {
  if (N <= 0 || mirror_axis < -1 || mirror_axis > 2) return false;
  const long V = static_cast<long>(N) * (mirror_axis >= 0 ? 2 : 1);
  if (V > kMaxV) return false;
  if (V > kResidentMaxV) {
    p->family = kRaggedStream, p->T = fps::kStreamThreads, p->PPT = 0, p->lds = 0;
    return true;
  }
  for (const auto& c : kRaggedCells)
    if (V <= static_cast<long>(c[0]) * c[1]) {
      p->family = kRaggedResident, p->T = c[0], p->PPT = c[1];
      p->lds = static_cast<size_t>((3 * N + 3) & ~3) * sizeof(float) + 2 * (c[0] / 64) * sizeof(unsigned long long);
      return true;
    }
  return false;
}

template <int T, int PPT>
int launch_ragged(const RaggedPlan& p, const float* xyz, const int64_t* lengths, int B, int N, int axis, int m, int* idx,
                  float* rows, hipStream_t s) {
  // the attribute is per DEVICE: set it on every large launch (cheap host call, no global state), checked
  if (p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_ragged_resident_kernel<T, PPT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return PDR_ELAUNCH;
  hipLaunchKernelGGL((fps_ragged_resident_kernel<T, PPT>), dim3(B), dim3(T), p.lds, s, xyz, lengths, N, axis, m, idx,
                     reinterpret_cast<float4*>(rows));
  return pdr::check_launch();
}

// sizes the call refuses with PDR_EUNSUPPORTED
bool ragged_too_large(int B, int N, int mirror_axis, int m) {
  const long V = static_cast<long>(N) * (mirror_axis >= 0 ? 2 : 1);
  return V > kMaxV || static_cast<long>(B) * (V > m ? V : m) >= (1l << 31);
}

}  // namespace

extern "C" size_t pdr_fps_ragged_workspace_bytes(int B, int N, int mirror_axis) {
  RaggedPlan p;
  if (B <= 0 || !plan_ragged(N, mirror_axis, &p) || ragged_too_large(B, N, mirror_axis, 0)) return 0;
  if (p.family != kRaggedStream) return 0;
  return static_cast<size_t>(B) * N * (mirror_axis >= 0 ? 2 : 1) * sizeof(float);
}

extern "C" int pdr_fps_ragged_plan(int N, int mirror_axis, int out[4]) {
  if (!out || N <= 0 || mirror_axis < -1 || mirror_axis > 2) return PDR_EINVAL;
  RaggedPlan p;
  if (!plan_ragged(N, mirror_axis, &p)) return PDR_EUNSUPPORTED;
  out[0] = p.family, out[1] = p.T, out[2] = p.PPT, out[3] = static_cast<int>(p.lds);
  return PDR_OK;
}

extern "C" int pdr_furthest_point_sampling_ragged(const float* xyz, const int64_t* lengths, int B, int N,
                                                  int mirror_axis, int m, float* temp, int* idx, float* rows,
                                                  pdr_stream_t stream) {
  if (B < 0 || N <= 0 || m < 0 || mirror_axis < -1 || mirror_axis > 2) return PDR_EINVAL;
  if (B == 0 || m == 0) return PDR_OK;
  RaggedPlan p;
  if (ragged_too_large(B, N, mirror_axis, m) || !plan_ragged(N, mirror_axis, &p)) return PDR_EUNSUPPORTED;
  if (!xyz || !idx || (p.family == kRaggedStream && !temp)) return PDR_EINVAL;
  if (rows && (reinterpret_cast<uintptr_t>(rows) & 15)) return PDR_EINVAL;   // rows are stored as float4
  hipStream_t s = pdr::as_stream(stream);
  if (p.family == kRaggedStream) {
    hipLaunchKernelGGL(fps_ragged_stream_kernel, dim3(B), dim3(fps::kStreamThreads), 0, s, xyz, lengths, N, mirror_axis, m, temp, idx,
                       reinterpret_cast<float4*>(rows));
    return pdr::check_launch();
  }
#define PDR_FPS_RAGGED_RUN(T_, PPT_)    \
  if (p.T == (T_) && p.PPT == (PPT_)) \
    return launch_ragged<T_, PPT_>(p, xyz, lengths, B, N, mirror_axis, m, idx, rows, s);
  PDR_FPS_RAGGED_CELLS(PDR_FPS_RAGGED_RUN)
#undef PDR_FPS_RAGGED_RUN
  return PDR_EUNSUPPORTED;
}
