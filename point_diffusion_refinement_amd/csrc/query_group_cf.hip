// query_group_cf.hip -- the part of QueryAndGroup.forward after the neighbour search (pointnet2_utils.py) for the
// TRAINABLE path, channel-first as Conv2d reads it, as one op with its backward: pdr_query_group_cf /
// pdr_query_group_cf_grad.  (The inference path has had the same gather, channel-last and forward only, in
// fused_gather.hip.)
//
//   xyz (B,n,3), new_xyz (B,m,3), features (B,C,n) | NULL, idx (B,m,K) i32, counts (B,m) i32 | NULL
//   -> out (B, Cu + 3E, m, K),  channels [features (Cu) | relative (3) | absolute (3) | centre (3)],
//   Cu = C with features, 0 without; E = the coordinate triples `flags` enables (bit 0 use_xyz: relative; bit 1
//   include_abs and bit 2 include_center count only with bit 0, as in the module).  P = m K positions per cloud.
//
// A non-NULL `counts` is the module's patch_empty: query q with counts[b,q] <= 0 is PATCHED -- its absolute
// coordinates are the centre's, its relative ones centre - centre, its feature channels +0.0f, and idx is not read
// for it in either direction.
//
// FORWARD, one launch.  Every output element is a bit-for-bit copy of its source, or, for the relative channels, the one
// rounded difference a - c (no fma: -ffp-contract=off).  The composition computes a patched or passed value as
// 1 * a + 0 * c; here it is SELECTED.  The two differ only for -0.0 and non-finite inputs.
//   Mapping (gather_rows_kernel of group_gather.hip): one thread per output position (q, k), consecutive lanes at
//   consecutive addresses, grid = (positions / 256, channel slabs, B).  A slab is 8 feature channels, or -- the last
//   slab when E > 0 -- all 3E coordinate channels, read from the 12-byte rows of xyz and new_xyz; the index and the
//   patched flag are loaded once per thread and reused over the slab.  Two families: vector (K % 4 == 0 and `out`
//   16-byte aligned: a thread takes four consecutive k of one query and stores 16 bytes per channel) and scalar
//   (anything else, such as a view 4 bytes into its storage).  pdr_query_group_cf_plan reports the decision.
//
// BACKWARD.  g_f, g_r, g_a, g_c: the slices of grad_out; a slice whose flag is off counts as +0.  A slot p = (q, k) is
// REAL when its query is not patched and 0 <= idx[b,p] < n (an index outside is skipped: dest_of of scatter_index.h).
//   a[d,p]             = fl(g_r[d,p] + g_a[d,p])                  gradient of the slot's absolute coordinate: it belongs
//                                                                 to xyz[idx] for a real slot, to the centre for a
//                                                                 patched one
//   grad_features[b,c,j] = sum of g_f[b,c,p] over the real slots p with idx[b,p] == j, ascending p, fp32 from +0.0f
//   grad_xyz[b,j,d]      = the same sum of a[d,p]
//   grad_new_xyz[b,q,d]  = sum over k = 0 .. K-1, ascending, fp32 from +0.0f, of t_k:
//                          t_k = fl(g_c[k] - g_r[k]) for a slot of an unpatched query,
//                          t_k = fl(fl(g_c[k] - g_r[k]) + a[k]) for a patched one
//   Without use_xyz both coordinate gradients are +0.0f everywhere.
// Every output element is written exactly once; no float atomics; the same input gives the same bits, and a cloud has
// the same bits alone and in a batch (nothing crosses clouds).  Launches: the inverse index of scatter_index.h (memset,
// rank, scan, place), built ONCE per call with patched slots left out, then the short and long ordered sums for
// grad_features (C channels, batch stride (C + 3E) P in grad_out) and again for grad_xyz (the three virtual channels
// a), and one kernel for grad_new_xyz (a thread per output element, its K terms serial).  A NULL gradient pointer skips
// that output and its launches; only grad_new_xyz asked for builds no index.
//
// Limits: the builder's (n <= 16384, m K <= 2^22, B <= 65535, B m K < 2^31) and B (C + 3E) m K < 2^31.
// Validation, on the host before any launch, in this order (both calls):
//   1. B, m, K or C negative, n <= 0, flags outside 0 .. 7, no channel at all (without use_xyz: C == 0, or in the
//      forward a NULL `features` -- C counts as 0 then, here and below; only its NULL-ness is looked at): PDR_EINVAL
//   2. B, m or K zero: PDR_OK, nothing launched, no pointer looked at (there is no output element to write; the
//      backward leaves its gradient buffers alone)
//   3. the limits above: PDR_EUNSUPPORTED
//   4. the pointers: PDR_EINVAL.  Forward: idx, out; xyz and new_xyz with use_xyz.  Backward: idx, grad_out; all
//      three gradient pointers NULL; the workspace (NULL or not 4-byte aligned) when grad_features (C > 0) or, with
//      use_xyz, grad_xyz is asked for.
#include "scatter_index.h"

namespace {

namespace si = scatter_index;

constexpr int kSlab = 8;          // feature channels per thread (group_gather.hip's slab)
constexpr unsigned kUseXyz = 1u, kAbs = 2u, kCentre = 4u;

inline int triples(unsigned flags) {
  if (!(flags & kUseXyz)) return 0;
  return 1 + ((flags & kAbs) ? 1 : 0) + ((flags & kCentre) ? 1 : 0);
}

struct FwdArgs {
  const float *xyz, *new_xyz, *feat;
  const int *idx, *counts;
  float* out;
  int n, m, K, C, Ctot, P, fslabs;   // C: feature channels in use; fslabs = ceil(C / 8)
  unsigned flags;
};

template <int V>
__device__ __forceinline__ void store(float* dst, const float (&v)[V]) {
  if (V == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u) dst[u] = v[u];
  }
}

// V = 4: K % 4 == 0, so the four positions of a thread belong to one query, P % 4 == 0, and every channel row of `out`
// starts 16-byte aligned when `out` does
template <int V>
__global__ __launch_bounds__(256) void query_group_kernel(FwdArgs a) {
  const int b = blockIdx.z;
  const int pos = (blockIdx.x * 256 + threadIdx.x) * V;
  if (pos >= a.P) return;
  const int q = pos / a.K;
  const bool patched = a.counts != nullptr && a.counts[static_cast<size_t>(b) * a.m + q] <= 0;
  int src[V];
#pragma unroll
  for (int u = 0; u < V; ++u) src[u] = patched ? 0 : a.idx[static_cast<size_t>(b) * a.P + pos + u];
  float* dst = a.out + static_cast<size_t>(b) * a.Ctot * a.P + pos;
  const int slab = blockIdx.y;
  if (slab < a.fslabs) {
    const int c0 = slab * kSlab;
    const int cn = (a.C - c0) < kSlab ? (a.C - c0) : kSlab;
    const float* f = a.feat + (static_cast<size_t>(b) * a.C + c0) * a.n;
    float v[kSlab][V];
#pragma unroll
    for (int c = 0; c < kSlab; ++c)
#pragma unroll
      for (int u = 0; u < V; ++u) v[c][u] = (c < cn && !patched) ? f[static_cast<size_t>(c) * a.n + src[u]] : 0.0f;
#pragma unroll
    for (int c = 0; c < kSlab; ++c)
      if (c < cn) store<V>(dst + static_cast<size_t>(c0 + c) * a.P, v[c]);
    return;
  }
  // the coordinate slab: relative | absolute | centre
  const float* ctr = a.new_xyz + (static_cast<size_t>(b) * a.m + q) * 3;
  const float* cloud = a.xyz + static_cast<size_t>(b) * a.n * 3;
  dst += static_cast<size_t>(a.C) * a.P;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float c = ctr[d];
    float ab[V], rel[V], cc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      ab[u] = patched ? c : cloud[static_cast<size_t>(src[u]) * 3 + d];
      rel[u] = ab[u] - c;
      cc[u] = c;
    }
    float* o = dst + static_cast<size_t>(d) * a.P;
    store<V>(o, rel);
    o += static_cast<size_t>(3) * a.P;
    if (a.flags & kAbs) {
      store<V>(o, ab);
      o += static_cast<size_t>(3) * a.P;
    }
    if (a.flags & kCentre) store<V>(o, cc);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// destination of position i = b P + pos of the flat index: none for a slot of a patched query (idx is not read)
struct RealSlot {
  const int* idx;
  const int* counts;
  int K;
  __device__ __forceinline__ int operator()(size_t i, int N) const {
    if (counts != nullptr && counts[i / K] <= 0) return -1;      // i / K = b m + q
    return si::dest_of(idx, i, N);
  }
};

// grad_features: the first C of grad_out's Ctot channels
struct FeatureSum {
  const float* go;
  float* out;
  int C, Ctot, P, N;
  __device__ __forceinline__ float term(int b, int c, int, int pos) const {
    return go[(static_cast<size_t>(b) * Ctot + c) * P + pos];
  }
  __device__ __forceinline__ size_t out_at(int b, int c, int d) const { return (static_cast<size_t>(b) * C + c) * N + d; }
};

// grad_xyz: the three virtual channels a = fl(g_r + g_a); c_abs < 0: no absolute slice, g_a = +0
struct XyzSum {
  const float* go;
  float* out;
  int C, Ctot, P, N, c_rel, c_abs;   // C == 3
  __device__ __forceinline__ float term(int b, int c, int, int pos) const {
    const float gr = go[(static_cast<size_t>(b) * Ctot + c_rel + c) * P + pos];
    const float ga = c_abs >= 0 ? go[(static_cast<size_t>(b) * Ctot + c_abs + c) * P + pos] : 0.0f;
    return gr + ga;
  }
  __device__ __forceinline__ size_t out_at(int b, int c, int d) const { return (static_cast<size_t>(b) * N + d) * 3 + c; }
};

// grad_new_xyz: one thread per output element (b, q, d) -- consecutive lanes store consecutive floats; the K terms of
// a thread are K consecutive floats of up to three channel rows
__global__ __launch_bounds__(256) void centre_grad_kernel(const float* __restrict__ go, const int* __restrict__ counts,
                                                          int m, int K, int Ctot, int c_rel, int c_abs, int c_ctr,
                                                          float* __restrict__ out) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= m * 3) return;
  const int q = t / 3, d = t - q * 3;
  const bool patched = counts != nullptr && counts[static_cast<size_t>(b) * m + q] <= 0;
  const size_t P = static_cast<size_t>(m) * K;
  const float* base = go + static_cast<size_t>(b) * Ctot * P + static_cast<size_t>(q) * K;
  const float* gr = base + static_cast<size_t>(c_rel + d) * P;
  const float* ga = c_abs >= 0 ? base + static_cast<size_t>(c_abs + d) * P : nullptr;
  const float* gc = c_ctr >= 0 ? base + static_cast<size_t>(c_ctr + d) * P : nullptr;
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) {
    const float r = gr[k];
    float tk = (gc ? gc[k] : 0.0f) - r;
    if (patched) tk = tk + (r + (ga ? ga[k] : 0.0f));
    acc += tk;
  }
  out[(static_cast<size_t>(b) * m + q) * 3 + d] = acc;
}

// steps 1 to 3 of the validation both calls share; *done: the call is over with the returned code
int check_sizes(int B, int n, int m, int K, int C, int flags, bool* done) {
  *done = true;
  if (B < 0 || m < 0 || K < 0 || C < 0 || n <= 0 || flags < 0 || flags > 7) return PDR_EINVAL;
  if (C == 0 && !(flags & 1)) return PDR_EINVAL;
  if (B == 0 || m == 0 || K == 0) return PDR_OK;
  const long P = static_cast<long>(m) * K;
  if (P > si::kMaxP || si::unsupported(B, P, n)) return PDR_EUNSUPPORTED;
  if (static_cast<long>(B) * (C + 3 * triples(flags)) >= ((1L << 31) + P - 1) / P) return PDR_EUNSUPPORTED;
  *done = false;
  return PDR_OK;
}

inline bool vector_family(int K, int aligned16) { return K % 4 == 0 && aligned16 != 0; }

}  // namespace

extern "C" size_t pdr_query_group_cf_workspace_bytes(int B, int n, int m, int K) {
  if (B <= 0 || n <= 0 || m <= 0 || K <= 0) return 0;
  const long P = static_cast<long>(m) * K;
  if (P > si::kMaxP || si::unsupported(B, P, n)) return 0;
  return si::carve(nullptr, B, static_cast<int>(P), n).bytes;
}

extern "C" int pdr_query_group_cf_plan(int n, int m, int K, int C, int flags, int aligned16, int out[6]) {
  if (!out) return PDR_EINVAL;
  bool done;
  const int rc = check_sizes(1, n, m, K, C, flags, &done);
  if (rc != PDR_OK) return rc;
  if (m == 0 || K == 0) return PDR_EINVAL;                  // nothing runs: there is no decision to report
  const int V = vector_family(K, aligned16) ? 4 : 1;
  const int E = triples(static_cast<unsigned>(flags));
  const int P = m * K;
  out[0] = V == 4;
  out[1] = (P / V + 255) / 256;
  out[2] = (C + kSlab - 1) / kSlab + (E > 0 ? 1 : 0);
  out[3] = (C + kSlab - 1) / kSlab;
  out[4] = C + 3 * E;
  out[5] = E;
  return PDR_OK;
}

extern "C" int pdr_query_group_cf(const float* xyz, const float* new_xyz, const float* features, const int* idx,
                                  const int* counts, int B, int n, int m, int K, int C, int flags, float* out,
                                  pdr_stream_t stream) {
  const int Cu = features ? C : 0;                          // NULL-ness only; nothing is dereferenced on the host
  bool done;
  const int rc = check_sizes(B, n, m, K, C < 0 ? C : Cu, flags, &done);
  if (done) return rc;
  const unsigned fl = static_cast<unsigned>(flags);
  const int E = triples(fl);
  if (!idx || !out || (E > 0 && (!xyz || !new_xyz))) return PDR_EINVAL;
  FwdArgs a;
  a.xyz = xyz, a.new_xyz = new_xyz, a.feat = features, a.idx = idx, a.counts = counts, a.out = out;
  a.n = n, a.m = m, a.K = K, a.C = Cu, a.Ctot = Cu + 3 * E, a.P = m * K, a.fslabs = (Cu + kSlab - 1) / kSlab;
  a.flags = fl;
  const bool vec = vector_family(K, (reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  const int slabs = a.fslabs + (E > 0 ? 1 : 0);
  const dim3 grid((a.P / (vec ? 4 : 1) + 255) / 256, slabs, B);
  hipStream_t s = pdr::as_stream(stream);
  if (vec) hipLaunchKernelGGL(query_group_kernel<4>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(query_group_kernel<1>, grid, dim3(256), 0, s, a);
  return pdr::check_launch();
}

extern "C" int pdr_query_group_cf_grad(const int* idx, const int* counts, const float* grad_out, int B, int n, int m,
                                       int K, int C, int flags, float* grad_features, float* grad_xyz,
                                       float* grad_new_xyz, void* workspace, pdr_stream_t stream) {
  bool done;
  int rc = check_sizes(B, n, m, K, C, flags, &done);
  if (done) return rc;
  const unsigned fl = static_cast<unsigned>(flags);
  const int E = triples(fl);
  const bool want_f = grad_features != nullptr && C > 0, want_x = grad_xyz != nullptr && E > 0;
  if (!idx || !grad_out || (!grad_features && !grad_xyz && !grad_new_xyz)) return PDR_EINVAL;
  if ((want_f || want_x) && (!workspace || si::misaligned(workspace))) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  const int P = m * K, Ctot = C + 3 * E;
  const int c_rel = C, c_abs = (fl & kAbs) && E > 0 ? C + 3 : -1;
  const int c_ctr = (fl & kCentre) && E > 0 ? C + 3 * (E - 1) : -1;
  if (E == 0) {                                             // no coordinate channel: both coordinate gradients are +0
    if (grad_xyz && hipMemsetAsync(grad_xyz, 0, sizeof(float) * static_cast<size_t>(B) * n * 3, s) != hipSuccess)
      return pdr::check_launch();
    if (grad_new_xyz && hipMemsetAsync(grad_new_xyz, 0, sizeof(float) * static_cast<size_t>(B) * m * 3, s) != hipSuccess)
      return pdr::check_launch();
  }
  if (want_f || want_x) {
    const si::Workspace ws = si::carve(workspace, B, P, n);
    if (!si::build(RealSlot{idx, counts, K}, B, P, n, ws, s)) return pdr::check_launch();
    if (want_f) si::sums(FeatureSum{grad_out, grad_features, C, Ctot, P, n}, B, ws, s);
    if (want_x) si::sums(XyzSum{grad_out, grad_xyz, 3, Ctot, P, n, c_rel, c_abs}, B, ws, s);
  }
  if (grad_new_xyz && E > 0)
    hipLaunchKernelGGL(centre_grad_kernel, dim3((m * 3 + 255) / 256, B), dim3(256), 0, s, grad_out, counts, m, K, Ctot,
                       c_rel, c_abs, c_ctr, grad_new_xyz);
  return pdr::check_launch();
}
