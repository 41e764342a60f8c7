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
// k >> 9 (5 in the resident kernels: k < 16384; 11 in the stream kernel: k < 2^20).
//
// Resident form (V <= 12288): fps_lean_kernel's round -- LDS read of the last pick, packed-fp32 distance updates (each
// half IEEE-exact, the PDR_SUM3 tree), in-lane arg-max, two 32-bit DPP reductions (value, then key), one barrier -- with
// two changes:
//   * thread t owns the points k = t + i T.  With T a divisor or a multiple of 512 the tie order of a thread's own
//     points is a COMPILE-TIME permutation of i (slot_point below), so the slots are laid out in that order, need no
//     sorting and no per-slot key register: the in-lane scan tracks the winning i as an immediate and the key of the
//     one winner is computed after the scan;
//   * a launch is instantiated for the batch's stride (T threads, at most PPT points per thread), but every workgroup
//     runs the round loop built for ITS cloud: ceil(V_b / T) points per thread rounded up to 2, 4, 8, 12 or 16.  A cloud
//     much shorter than N does not pay for N.
#include "pdr_common.h"

namespace {

constexpr int kResidentMaxV = 12288;      // 3 floats per ORIGINAL point in LDS next to the exchange slots (160 KiB)
constexpr long kMaxV = 1l << 20;          // stream kernel: 9 + 11 rank bits, k in 20 bits

typedef float fpr_f2 __attribute__((ext_vector_type(2)));

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

// wave-wide maximum of non-negative keys: the DPP shift is an operand modifier of the v_max_u32 itself (lanes without a
// source keep their own value; lane 63 ends with the maximum).  Two wait states between a VALU write of a register and
// a DPP read of it: the assembler does not insert them.  (fps.hip keeps the same reduction private to its file.)
__device__ __forceinline__ unsigned fpr_wave_max_u32(unsigned v) {
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

__device__ __forceinline__ float flip_if(float v, bool flip) {
  return __uint_as_float(__float_as_uint(v) ^ (flip ? 0x80000000u : 0u));
}

// virtual point `k` of a cloud whose L originals are in LDS (k < V is the caller's business)
struct VPoint {
  float x, y, z, tag;
};
__device__ __forceinline__ VPoint virtual_point(const float* sx, const float* sy, const float* sz, int k, int L,
                                                int axis) {
  const bool mir = k >= L;
  const int src = mir ? k - L : k;
  VPoint v;
  v.x = flip_if(sx[src], mir && axis == 0);
  v.y = flip_if(sy[src], mir && axis == 1);
  v.z = flip_if(sz[src], mir && axis == 2);
  v.tag = mir ? -1.0f : 1.0f;
  return v;
}

template <int T, int PPT, int S>
__device__ __forceinline__ void scan_slots(const fpr_f2 (&tmp)[PPT / 2], float& best, unsigned& besti) {
  if constexpr (S < PPT) {
    const float v = tmp[S >> 1][S & 1];
    const bool gt = v > best;
    best = gt ? v : best;
    besti = gt ? static_cast<unsigned>(SlotPoint<T, PPT, S>::value) : besti;
    scan_slots<T, PPT, S + 1>(tmp, best, besti);
  }
}
template <int T, int PPT, int S>
__device__ __forceinline__ void load_slots(fpr_f2 (&px)[PPT / 2], fpr_f2 (&py)[PPT / 2], fpr_f2 (&pz)[PPT / 2],
                                           fpr_f2 (&tmp)[PPT / 2], const float* sx, const float* sy, const float* sz,
                                           int tid, int L, int V, int axis) {
  if constexpr (S < PPT) {
    const int k = tid + SlotPoint<T, PPT, S>::value * T;
    const bool valid = k < V;
    const VPoint v = virtual_point(sx, sy, sz, valid ? k : 0, L, axis);
    const float mag = PDR_SUM3(v.x, v.y, v.z);
    px[S >> 1][S & 1] = valid ? v.x : 0.0f;
    py[S >> 1][S & 1] = valid ? v.y : 0.0f;
    pz[S >> 1][S & 1] = valid ? v.z : 0.0f;
    // reference: `if (mag <= 1e-3) continue;` -- float promoted to double.  Beyond the cloud: never selectable, never
    // updated upward
    tmp[S >> 1][S & 1] = (!valid || static_cast<double>(mag) <= 1e-3) ? -1.0f : 1e10f;
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
  fpr_f2 px[G], py[G], pz[G], tmp[G];
  load_slots<T, PPT, 0>(px, py, pz, tmp, sx, sy, sz, tid, L, V, axis);

  int old = 0;
  if (tid == 0) out[0] = 0;
  for (int j = 1; j < m; ++j) {
    const VPoint c = virtual_point(sx, sy, sz, old, L, axis);
    if (tid == 0 && rows) rows[j - 1] = make_float4(c.x, c.y, c.z, c.tag);
    // distance updates in groups of at most 4 pairs, written stage by stage so that consecutive instructions are
    // independent (a workgroup of 1024 threads has 128 VGPRs per lane: the temporaries of all pairs at once do not fit)
    constexpr int GS = G < 4 ? G : 4;
#pragma unroll
    for (int g0 = 0; g0 < G; g0 += GS) {
      fpr_f2 dx[GS], dy[GS], dz[GS], d[GS];
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) dy[g] = py[g0 + g] - c.y;
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) dx[g] = px[g0 + g] - c.x;
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) d[g] = dy[g] * dy[g];                  // PDR_SUM3: fma(c, c, fma(a, a, b * b))
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) dz[g] = pz[g0 + g] - c.z;
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) d[g] = __builtin_elementwise_fma(dx[g], dx[g], d[g]);
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) d[g] = __builtin_elementwise_fma(dz[g], dz[g], d[g]);
#pragma unroll
      for (int g = 0; g < GS; ++g)
        if (g0 + g < G) {
          // v_min_f32 directly (fminf first canonicalises both operands: +1 VALU per point)
          fpr_f2 r;
          asm("v_min_f32 %0, %1, %2" : "=v"(r[0]) : "v"(d[g][0]), "v"(tmp[g0 + g][0]));
          asm("v_min_f32 %0, %1, %2" : "=v"(r[1]) : "v"(d[g][1]), "v"(tmp[g0 + g][1]));
          tmp[g0 + g] = r;
        }
    }
    // first strictly greater in slot order = in tie order
    float best = -1.0f;
    unsigned besti = 0u;
    scan_slots<T, PPT, 0>(tmp, best, besti);
    const unsigned k = static_cast<unsigned>(tid) + besti * T;
    const unsigned rank = (__brev(k & 511u) >> 23 << 5) | (k >> 9);
    const unsigned low = ((0xFFFFu - rank) << 16) | k;         // larger = preferred
    // best >= 0 -> monotone uint bits; "no candidate" (-1) -> 0
    const unsigned vb = best < 0.0f ? 0u : __float_as_uint(best);
    const unsigned vmax = fpr_wave_max_u32(vb);                // uniform
    // (a candidate at distance +0.0 has value bits 0 like "no candidate", but keeps its key)
    const unsigned cand = (vb == vmax && !(best < 0.0f)) ? low : 0u;
    const unsigned wlow = fpr_wave_max_u32(cand);
    unsigned long long key = pdr::u64_from(vmax, wlow);
    if constexpr (W > 1) {
      unsigned long long* sl = slots + (j & 1) * W;
      if ((tid & 63) == 0) sl[tid >> 6] = key;
      __syncthreads();
      unsigned long long r = sl[0];
#pragma unroll
      for (int w = 1; w < W; ++w) {
        const unsigned long long o = sl[w];
        r = o > r ? o : r;
      }
      key = r;
    }
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

// Streaming form for V > kResidentMaxV: fps_stream_kernel of fps.hip on the virtual cloud -- running distances in the
// caller's temp (row stride = the batch's V), points re-read from global memory every round, two-stage (value, rank)
// arg-max.  Kept simple.
__device__ __forceinline__ VPoint virtual_point_global(const float* __restrict__ p, int k, int L, int axis) {
  const bool mir = k >= L;
  const int src = mir ? k - L : k;
  VPoint v;
  v.x = flip_if(p[src * 3 + 0], mir && axis == 0);
  v.y = flip_if(p[src * 3 + 1], mir && axis == 1);
  v.z = flip_if(p[src * 3 + 2], mir && axis == 2);
  v.tag = mir ? -1.0f : 1.0f;
  return v;
}

__global__ __launch_bounds__(1024) void fps_ragged_stream_kernel(const float* __restrict__ xyz,
                                                                 const int64_t* __restrict__ lengths, int N, int axis,
                                                                 int m, float* __restrict__ temp,
                                                                 int* __restrict__ idxs, float4* __restrict__ rows4) {
  __shared__ float sval[16];
  __shared__ unsigned srank[16];
  __shared__ int sold;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = pdr::cloud_len(lengths, b, N);
  const int V = axis >= 0 ? 2 * L : L;
  int* out = idxs + static_cast<size_t>(b) * m;
  float4* rows = rows4 ? rows4 + static_cast<size_t>(b) * m : nullptr;
  if (L == 0) {
    write_empty(out, rows, m, tid, 1024);
    return;
  }
  const float* p = xyz + static_cast<size_t>(b) * N * 3;
  float* tp = temp + static_cast<size_t>(b) * N * (axis >= 0 ? 2 : 1);
  for (int k = tid; k < V; k += 1024) {
    const VPoint v = virtual_point_global(p, k, L, axis);
    const float mag = PDR_SUM3(v.x, v.y, v.z);
    tp[k] = (static_cast<double>(mag) <= 1e-3) ? -1.0f : 1e10f;
  }
  if (tid == 0) out[0] = 0;
  __syncthreads();
  int old = 0;
  for (int j = 1; j < m; ++j) {
    const VPoint c = virtual_point_global(p, old, L, axis);
    if (tid == 0 && rows) rows[j - 1] = make_float4(c.x, c.y, c.z, c.tag);
    float best = -1.0f;
    unsigned bestrank = ~0u;                                   // bitrev9(k & 511) << 11 | k >> 9; smaller = preferred
    for (int k = tid; k < V; k += 1024) {
      const VPoint v = virtual_point_global(p, k, L, axis);
      const float dx = v.x - c.x, dy = v.y - c.y, dz = v.z - c.z;
      const float d2 = fminf(PDR_SUM3(dx, dy, dz), tp[k]);
      tp[k] = d2;
      const unsigned rank = (__brev(static_cast<unsigned>(k) & 511u) >> 23 << 11) | (static_cast<unsigned>(k) >> 9);
      const bool better = d2 > best || (d2 == best && d2 >= 0.0f && rank < bestrank);
      best = better ? d2 : best;
      bestrank = better ? rank : bestrank;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const unsigned orank = __shfl_xor(bestrank, off, 64);
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
      unsigned br = srank[0];
      for (int w = 1; w < 16; ++w) {
        const bool better = sval[w] > bv || (sval[w] == bv && srank[w] < br);
        bv = better ? sval[w] : bv;
        br = better ? srank[w] : br;
      }
      // rank -> k: the low 11 bits are k >> 9, the 9 above them bitrev9(k & 511)
      const unsigned k = ((br & 2047u) << 9) | (__brev(br >> 11) >> 23);
      sold = bv < 0.0f ? 0 : static_cast<int>(k);
      out[j] = sold;
    }
    __syncthreads();
    old = sold;
  }
  if (tid == 0 && rows) {
    const VPoint c = virtual_point_global(p, old, L, axis);
    rows[m - 1] = make_float4(c.x, c.y, c.z, c.tag);
  }
}

// ---- the dispatch decision: ONE host function, read by the launch and by pdr_fps_ragged_plan -------------------------
enum { kRaggedResident = 0, kRaggedStream = 1 };

struct RaggedPlan {
  int family, T, PPT;
  size_t lds;
};

constexpr int kRaggedResidentTable[][2] = {{64, 2}, {256, 16}, {1024, 12}};   // {T, PPT}: V <= T PPT

bool plan_ragged(int N, int mirror_axis, RaggedPlan* p) {
  if (N <= 0 || mirror_axis < -1 || mirror_axis > 2) return false;
  const long V = static_cast<long>(N) * (mirror_axis >= 0 ? 2 : 1);
  if (V > kMaxV) return false;
  if (V > kResidentMaxV) {
    p->family = kRaggedStream, p->T = 1024, p->PPT = 0, p->lds = 0;
    return true;
  }
  for (const auto& c : kRaggedResidentTable)
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
    hipLaunchKernelGGL(fps_ragged_stream_kernel, dim3(B), dim3(1024), 0, s, xyz, lengths, N, mirror_axis, m, temp, idx,
                       reinterpret_cast<float4*>(rows));
    return pdr::check_launch();
  }
  // every instantiation of kRaggedResidentTable, keyed by what the plan reports
#define PDR_FPS_RAGGED_RUN(T_, PPT_)    \
  if (p.T == (T_) && p.PPT == (PPT_)) \
  return launch_ragged<T_, PPT_>(p, xyz, lengths, B, N, mirror_axis, m, idx, rows, s)
  PDR_FPS_RAGGED_RUN(64, 2);
  PDR_FPS_RAGGED_RUN(256, 16);
  PDR_FPS_RAGGED_RUN(1024, 12);
#undef PDR_FPS_RAGGED_RUN
  return PDR_EUNSUPPORTED;
}
