// scatter_det.hip -- deterministic twins of the four scatter-add backward calls (gather / group / three_interpolate
// grads and the grad_y half of the kNN backward).
//
// The atomic twins (group_gather.hip, neighbors.hip) add every contribution where it lands; the order of the float
// adds is whatever the hardware makes of it.  Here the scatter is turned into a gather: an INVERSE INDEX lists, for
// every destination, its source positions in ascending order, and one thread (or, for a very long list, one lane of a
// wave) adds them in exactly that order in fp32 from +0.0f -- the order of the CPU oracle's sequential loops, so the
// result is the oracle's bit for bit and the same run after run.  Every output element is written exactly once.
//
// The inverse-index builder (rank, scan, place) and the short and long ordered sums live in scatter_index.h, which
// states them; this file holds the four addends and the entry points.
#include "scatter_index.h"

namespace {

using namespace scatter_index;

// ---- the addends -----------------------------------------------------------------------------------------------------
enum Op { kRows, kInterp, kKnn };

template <int OP>
struct SumArgs {
  const float* go;   // rows / interp: grad_out (B, C, P) / (B, C, P / 3); kNN: grad_dists (B, P)
  const float* w;    // interp: weight (B, P)
  const float* x;    // kNN: queries (B, n1, 3)
  const float* y;    // kNN: cloud (B, N, 3)
  float* out;        // rows / interp: (B, C, N); kNN: (B, N, 3)
  int C, P, N, K, n1;

  // the term that source position `pos` adds to channel c of destination d (products rounded before the add:
  // the library is built with -ffp-contract=off)
  __device__ __forceinline__ float term(int b, int c, int d, int pos) const {
    if (OP == kRows) return go[(static_cast<size_t>(b) * C + c) * P + pos];
    if (OP == kInterp)
      return go[(static_cast<size_t>(b) * C + c) * (P / 3) + pos / 3] * w[static_cast<size_t>(b) * P + pos];
    const int j = pos / K;
    const float g = 2.0f * go[static_cast<size_t>(b) * P + pos];
    const float diff = x[(static_cast<size_t>(b) * n1 + j) * 3 + c] - y[(static_cast<size_t>(b) * N + d) * 3 + c];
    return -(g * diff);                                   // acc -= t and acc += -t are the same rounding
  }
  __device__ __forceinline__ size_t out_at(int b, int c, int d) const {
    return OP == kKnn ? (static_cast<size_t>(b) * N + d) * 3 + c : (static_cast<size_t>(b) * C + c) * N + d;
  }
};

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

// builder + both sums on `s`; P > 0, sizes supported, pointers checked by the caller
template <int OP, typename IdxT>
int scatter_det(const IdxT* idx, int B, const SumArgs<OP>& a, void* workspace, hipStream_t s) {
  const Workspace ws = carve(workspace, B, a.P, a.N);
  if (!build(IndexDest<IdxT>{idx}, B, a.P, a.N, ws, s)) return pdr::check_launch();
  sums(a, B, ws, s);
  return pdr::check_launch();
}

int rows_det(const float* grad_out, const int* idx, int B, int C, int N, int P, float* grad_points, void* workspace,
             hipStream_t s) {
  if (unsupported(B, P, N)) return PDR_EUNSUPPORTED;
  if (!grad_points || (P > 0 && (!grad_out || !idx || !workspace || misaligned(workspace)))) return PDR_EINVAL;
  if (P == 0) {                                           // nothing to add: every element is +0.0
    if (hipMemsetAsync(grad_points, 0, sizeof(float) * static_cast<size_t>(B) * C * N, s) != hipSuccess)
      return pdr::check_launch();
    return PDR_OK;
  }
  SumArgs<kRows> a = {};
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
  SumArgs<kInterp> a = {};
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
  SumArgs<kKnn> a = {};
  a.go = grad_dists, a.x = x, a.y = y, a.out = grad_y, a.C = 3, a.P = static_cast<int>(P), a.N = n2, a.K = K, a.n1 = n1;
  return scatter_det<kKnn>(idx, B, a, workspace, s);
}
