// knn_group_cf.hip -- the part of group_knn(..., transpose=True) after the neighbour search (pointnet2_utils.py) for the
// TRAINABLE path, channel-first as Conv2d reads it, as one op with its backward: pdr_knn_group_cf /
// pdr_knn_group_cf_grad.  (The inference path has had the same gather, channel-last and forward only, in
// fused_gather.hip.)  The conventions are those of query_group_cf.hip.
//
//   x (B,n1,3), y (B,n2,3), features (B,C,n2) | NULL, idx (B,n1,K) i32, dists (B,n1,K) f32
//   -> out (B, Cu + 11, n1, K),  channels [features (Cu) | d2 | w | nn_abs (3) | nn_rel (3) | x (3)],
//   Cu = C with features, 0 without.  P = n1 K positions per cloud; q = the query of a position, k its slot.
// idx and dists are what the library's own search returned (pdr_knn_group): no padding slot, 0 <= idx < n2.  The
// forward TRUSTS idx, as pdr_query_group_cf does; dists is data (it is copied and fed to the weight chain, never used
// as an address).
//
// FORWARD, one launch.  -ffp-contract=off: every product and quotient below is rounded before it is used.
//   features, d2, nn_abs, x  bit-for-bit copies of features[:, :, idx], dists, y[idx], x[q]
//   nn_rel[d]                fl(y[idx,d] - x[q,d])
//   w_k                      fl(r_k / S),  r_k = fl(1.0f / fl(d_k + 1e-8f)),  S = the fp32 sum of r_0 .. r_{K-1} in
//                            ascending k from +0 -- the chain of pdr_knn_group and pdr_knn_build: the bits of
//                            pdr_knn_group's `weights`
//   Mapping (query_group_kernel): one thread per output position (q, k), consecutive lanes at consecutive addresses,
//   grid = (positions / 256, channel slabs, B).  A slab is 8 feature channels, or -- the last slab -- the 11 geometric
//   channels; its thread reads the K distances of its query to form S (K serial loads of one cached row).  The index is
//   loaded once per thread and reused over the slab.  Two families: vector (K % 4 == 0 and `out` 16-byte aligned: a
//   thread takes four consecutive k of one query and stores 16 bytes per channel) and scalar (anything else, such as a
//   view 4 bytes into its storage).  pdr_knn_group_cf_plan reports the decision.
//
// BACKWARD.  g_f, g_d, g_w, g_a, g_r, g_c: the slices of grad_out in channel order.  A slot p = (q, k) is REAL when
// 0 <= idx[b,p] < n2 (an index outside is skipped: dest_of of scatter_index.h; it is in no list and y is not read for
// it -- its e below is +0).  Per query, with r_k, S and w_k recomputed from dists exactly as in the forward:
//   dot      = sum over k ascending, fp32 from +0, of fl(g_w_k * w_k)
//   h_k      = fl(fl(g_w_k - dot) / S)
//   G_k      = fl(g_d_k - fl(fl(r_k * r_k) * h_k))            the whole gradient of the slot's squared distance
//   e_{k,d}  = fl(x[q,d] - y[idx,d])
//   t_{k,d}  = fl(fl(2 G_k) * e_{k,d})                          pytorch3d's kNN backward, as in knn_grad_x_kernel
//   grad_x[b,q,d]        = sum over k ascending, fp32 from +0.0f, of fl(fl(g_c - g_r) + t)
//   grad_features[b,c,j] = sum of g_f[b,c,p] over the real slots p with idx[b,p] == j, ascending p, fp32 from +0.0f
//   grad_y[b,j,d]        = the same ordered sum of fl(fl(g_a + g_r) - t)
// Every output element is written exactly once (a destination no slot names gets +0.0f); no float atomics; the same
// input gives the same bits, and a cloud has the same bits alone and in a batch (nothing crosses clouds), whatever
// set_deterministic says.  Launches: the inverse index of scatter_index.h (memset, rank, scan, place), built ONCE per
// call, then the short and long ordered sums for grad_features (the first C of C + 11 channels of grad_out) and again
// for grad_y (three virtual channels; the addend recomputes its query's S and dot, 2 K cached loads), and one kernel
// for grad_x (a thread per query, its K terms serial).  A NULL gradient pointer skips that output and its launches;
// only grad_x asked for builds no index.
//
// Limits: the builder's (n2 <= 16384, n1 K <= 2^22, B <= 65535, B n1 K < 2^31), B (C + 11) n1 K < 2^31, and
// C <= 524272 (the channel slabs are grid.y: ceil(C / 8) + 1 <= 65535).
// Validation, on the host before any launch, in this order (both calls):
//   1. B, n1, K or C negative, n2 <= 0 (the plan, which reports a decision, also refuses K <= 0 and n1 <= 0): PDR_EINVAL
//   2. B, n1 or K zero: PDR_OK, nothing launched, no pointer looked at (there is no output element to write; the
//      backward leaves its gradient buffers alone)
//   3. the limits above: PDR_EUNSUPPORTED
//   4. the pointers: PDR_EINVAL.  Forward: x, y, idx, dists, out (a NULL `features` is the call without features: C
//      counts as 0 then, here and above; only its NULL-ness is looked at).  Backward: x, y, idx, dists, grad_out; all
//      three gradient pointers NULL; the workspace (NULL or not 4-byte aligned) when grad_features (C > 0) or grad_y
//      is asked for.
#include "scatter_index.h"

namespace {

namespace si = scatter_index;

constexpr int kSlab = 8;          // feature channels per thread (group_gather.hip's slab)
constexpr int kGeo = 11;          // d2 | w | nn_abs (3) | nn_rel (3) | x (3)
constexpr float kEps = 1e-8f;
constexpr int kMaxC = kSlab * 65534;   // feature slabs plus the geometric one are grid.y <= 65535

struct FwdArgs {
  const float *x, *y, *feat, *dists;
  const int* idx;
  float* out;
  int n1, n2, K, C, Ctot, P, fslabs;   // C: feature channels in use; fslabs = ceil(C / 8)
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

__device__ __forceinline__ float recip_of(float d) { return 1.0f / (d + kEps); }

// S of a query: the K distances of row `dq`, ascending k from +0
__device__ __forceinline__ float norm_of(const float* __restrict__ dq, int K) {
  float S = 0.0f;
  for (int k = 0; k < K; ++k) S += recip_of(dq[k]);
  return S;
}

// V = 4: K % 4 == 0, so the four positions of a thread belong to one query, P % 4 == 0, and every channel row of `out`
// starts 16-byte aligned when `out` does
template <int V>
__global__ __launch_bounds__(256) void knn_group_kernel(FwdArgs a) {
  const int b = blockIdx.z;
  const int pos = (blockIdx.x * 256 + threadIdx.x) * V;
  if (pos >= a.P) return;
  const int q = pos / a.K;
  int src[V];
#pragma unroll
  for (int u = 0; u < V; ++u) src[u] = a.idx[static_cast<size_t>(b) * a.P + pos + u];
  float* dst = a.out + static_cast<size_t>(b) * a.Ctot * a.P + pos;
  const int slab = blockIdx.y;
  if (slab < a.fslabs) {
    const int c0 = slab * kSlab;
    const int cn = (a.C - c0) < kSlab ? (a.C - c0) : kSlab;
    const float* f = a.feat + (static_cast<size_t>(b) * a.C + c0) * a.n2;
    float v[kSlab][V];
#pragma unroll
    for (int c = 0; c < kSlab; ++c)
#pragma unroll
      for (int u = 0; u < V; ++u) v[c][u] = c < cn ? f[static_cast<size_t>(c) * a.n2 + src[u]] : 0.0f;
#pragma unroll
    for (int c = 0; c < kSlab; ++c)
      if (c < cn) store<V>(dst + static_cast<size_t>(c0 + c) * a.P, v[c]);
    return;
  }
  // the geometric slab: d2 | w | nn_abs | nn_rel | x
  dst += static_cast<size_t>(a.C) * a.P;
  const float* dq = a.dists + static_cast<size_t>(b) * a.P + static_cast<size_t>(q) * a.K;
  const float S = norm_of(dq, a.K);
  const int k0 = pos - q * a.K;
  float d2[V], w[V];
#pragma unroll
  for (int u = 0; u < V; ++u) {
    d2[u] = dq[k0 + u];
    w[u] = recip_of(d2[u]) / S;
  }
  store<V>(dst, d2);
  store<V>(dst + a.P, w);
  const float* xq = a.x + (static_cast<size_t>(b) * a.n1 + q) * 3;
  const float* cloud = a.y + static_cast<size_t>(b) * a.n2 * 3;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float c = xq[d];
    float ab[V], rel[V], cc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      ab[u] = cloud[static_cast<size_t>(src[u]) * 3 + d];
      rel[u] = ab[u] - c;
      cc[u] = c;
    }
    store<V>(dst + static_cast<size_t>(2 + d) * a.P, ab);
    store<V>(dst + static_cast<size_t>(5 + d) * a.P, rel);
    store<V>(dst + static_cast<size_t>(8 + d) * a.P, cc);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// G of slot k of the query whose rows are dq (distances), gd and gw (the d2 and w slices of grad_out), all K long
struct SlotGrad {
  float S, dot;
  __device__ __forceinline__ void prepare(const float* __restrict__ dq, const float* __restrict__ gw, int K) {
    S = norm_of(dq, K);
    dot = 0.0f;
    for (int k = 0; k < K; ++k) dot += gw[k] * (recip_of(dq[k]) / S);
  }
  // fl(2 G_k)
  __device__ __forceinline__ float twice(float d, float gd, float gw) const {
    const float r = recip_of(d);
    const float h = (gw - dot) / S;
    const float G = gd - (r * r) * h;
    return 2.0f * G;
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

// grad_y: the three virtual channels fl(fl(g_a + g_r) - t); j is the slot's destination, idx[b,pos], inside [0, n2)
struct YSum {
  const float *go, *x, *y, *dists;
  float* out;
  int C, Ctot, P, N, n1, K, c_geo;   // C == 3; c_geo: the d2 channel of grad_out
  __device__ __forceinline__ float term(int b, int c, int j, int pos) const {
    const int q = pos / K;
    const float* base = go + (static_cast<size_t>(b) * Ctot + c_geo) * P;
    const size_t row = static_cast<size_t>(q) * K;
    const float* dq = dists + static_cast<size_t>(b) * P + row;
    SlotGrad s;
    s.prepare(dq, base + P + row, K);
    const int k = pos - q * K;
    const float g2 = s.twice(dq[k], base[pos], base[static_cast<size_t>(P) + pos]);
    const float e = x[(static_cast<size_t>(b) * n1 + q) * 3 + c] - y[(static_cast<size_t>(b) * N + j) * 3 + c];
    const float t = g2 * e;
    const float ga = base[static_cast<size_t>(2 + c) * P + pos], gr = base[static_cast<size_t>(5 + c) * P + pos];
    return (ga + gr) - t;
  }
  __device__ __forceinline__ size_t out_at(int b, int c, int d) const { return (static_cast<size_t>(b) * N + d) * 3 + c; }
};

// grad_x: one thread per query (b, q); its K terms serial, the three coordinates side by side
__global__ __launch_bounds__(256) void query_grad_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const int* __restrict__ idx, const float* __restrict__ dists,
                                                         const float* __restrict__ go, int n1, int n2, int K, int Ctot,
                                                         int c_geo, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n1) return;
  const size_t P = static_cast<size_t>(n1) * K, row = static_cast<size_t>(q) * K;
  const float* base = go + (static_cast<size_t>(b) * Ctot + c_geo) * P + row;
  const float* dq = dists + static_cast<size_t>(b) * P + row;
  const int* iq = idx + static_cast<size_t>(b) * P + row;
  const float* gd = base;
  const float* gw = base + P;
  SlotGrad s;
  s.prepare(dq, gw, K);
  const float* xq = x + (static_cast<size_t>(b) * n1 + q) * 3;
  const float* cloud = y + static_cast<size_t>(b) * n2 * 3;
  const float xv[3] = {xq[0], xq[1], xq[2]};
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int k = 0; k < K; ++k) {
    const float g2 = s.twice(dq[k], gd[k], gw[k]);
    const int j = iq[k];
    const bool real = j >= 0 && j < n2;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float e = real ? xv[d] - cloud[static_cast<size_t>(j) * 3 + d] : 0.0f;
      const float t = g2 * e;
      const float gr = base[static_cast<size_t>(5 + d) * P + k], gc = base[static_cast<size_t>(8 + d) * P + k];
      acc[d] += (gc - gr) + t;
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) out[(static_cast<size_t>(b) * n1 + q) * 3 + d] = acc[d];
}

// steps 1 to 3 of the validation both calls share; *done: the call is over with the returned code
int check_sizes(int B, int n1, int n2, int K, int C, bool* done) {
  *done = true;
  if (B < 0 || n1 < 0 || K < 0 || C < 0 || n2 <= 0) return PDR_EINVAL;
  if (B == 0 || n1 == 0 || K == 0) return PDR_OK;
  const long P = static_cast<long>(n1) * K;
  if (P > si::kMaxP || si::unsupported(B, P, n2)) return PDR_EUNSUPPORTED;
  if (static_cast<long>(B) * (static_cast<long>(C) + kGeo) >= ((1L << 31) + P - 1) / P) return PDR_EUNSUPPORTED;
  if (C > kMaxC) return PDR_EUNSUPPORTED;
  *done = false;
  return PDR_OK;
}

inline bool vector_family(int K, int aligned16) { return K % 4 == 0 && aligned16 != 0; }

}  // namespace

extern "C" size_t pdr_knn_group_cf_workspace_bytes(int B, int n1, int n2, int K) {
  if (B <= 0 || n1 <= 0 || n2 <= 0 || K <= 0) return 0;
  const long P = static_cast<long>(n1) * K;
  if (P > si::kMaxP || si::unsupported(B, P, n2)) return 0;
  return si::carve(nullptr, B, static_cast<int>(P), n2).bytes;
}

extern "C" int pdr_knn_group_cf_plan(int n1, int n2, int K, int C, int aligned16, int out[5]) {
  if (!out) return PDR_EINVAL;
  bool done;
  const int rc = check_sizes(1, n1, n2, K, C, &done);
  if (rc != PDR_OK) return rc;
  if (n1 == 0 || K == 0) return PDR_EINVAL;                 // nothing runs: there is no decision to report
  const int V = vector_family(K, aligned16) ? 4 : 1;
  const int P = n1 * K;
  out[0] = V == 4;
  out[1] = (P / V + 255) / 256;
  out[2] = (C + kSlab - 1) / kSlab + 1;
  out[3] = (C + kSlab - 1) / kSlab;
  out[4] = C + kGeo;
  return PDR_OK;
}

extern "C" int pdr_knn_group_cf(const float* x, const float* y, const float* features, const int* idx,
                                const float* dists, int B, int n1, int n2, int K, int C, float* out,
                                pdr_stream_t stream) {
  const int Cu = features ? C : 0;                          // NULL-ness only; nothing is dereferenced on the host
  bool done;
  const int rc = check_sizes(B, n1, n2, K, C < 0 ? C : Cu, &done);
  if (done) return rc;
  if (!x || !y || !idx || !dists || !out) return PDR_EINVAL;
  FwdArgs a;
  a.x = x, a.y = y, a.feat = features, a.dists = dists, a.idx = idx, a.out = out;
  a.n1 = n1, a.n2 = n2, a.K = K, a.C = Cu, a.Ctot = Cu + kGeo, a.P = n1 * K, a.fslabs = (Cu + kSlab - 1) / kSlab;
  const bool vec = vector_family(K, (reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  const dim3 grid((a.P / (vec ? 4 : 1) + 255) / 256, a.fslabs + 1, B);
  hipStream_t s = pdr::as_stream(stream);
  if (vec) hipLaunchKernelGGL(knn_group_kernel<4>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(knn_group_kernel<1>, grid, dim3(256), 0, s, a);
  return pdr::check_launch();
}

extern "C" int pdr_knn_group_cf_grad(const float* x, const float* y, const int* idx, const float* dists,
                                     const float* grad_out, int B, int n1, int n2, int K, int C, float* grad_features,
                                     float* grad_x, float* grad_y, void* workspace, pdr_stream_t stream) {
  bool done;
  const int rc = check_sizes(B, n1, n2, K, C, &done);
  if (done) return rc;
  const bool want_f = grad_features != nullptr && C > 0, want_y = grad_y != nullptr;
  if (!x || !y || !idx || !dists || !grad_out || (!grad_features && !grad_x && !grad_y)) return PDR_EINVAL;
  if ((want_f || want_y) && (!workspace || si::misaligned(workspace))) return PDR_EINVAL;
  hipStream_t s = pdr::as_stream(stream);
  const int P = n1 * K, Ctot = C + kGeo;
  if (want_f || want_y) {
    const si::Workspace ws = si::carve(workspace, B, P, n2);
    if (!si::build(si::IndexDest<int>{idx}, B, P, n2, ws, s)) return pdr::check_launch();
    if (want_f) si::sums(FeatureSum{grad_out, grad_features, C, Ctot, P, n2}, B, ws, s);
    if (want_y) si::sums(YSum{grad_out, x, y, dists, grad_y, 3, Ctot, P, n2, n1, K, C}, B, ws, s);
  }
  if (grad_x)
    hipLaunchKernelGGL(query_grad_kernel, dim3((n1 + 255) / 256, B), dim3(256), 0, s, x, y, idx, dists, grad_out, n1, n2,
                       K, Ctot, C, grad_x);
  return pdr::check_launch();
}
