// chamfer_pairs.hip -- all-pairs Chamfer distance between two SETS of clouds: pdr_chamfer_pairwise.
//
// Replaces the Chamfer half of _pairwise_EMD_CD_ (reference pointnet2/models/pvd/metrics/evaluation_metrics.py:45-78):
// that loop expands one cloud R times, calls chamfer_distance on the batch, receives 2 (n + m) distances and int64
// indices per cloud pair (49 KB per 2048^2 pair) and reduces them to ONE float per pair with torch launches.  Here a
// workgroup owns a pair (s, r): nothing per point is stored, no index is recovered, one float is written.
//
//   cd[s,r] = (1/n_s) sum_i min_j |x_s,i - y_r,j|^2  +  (1/m_r) sum_j min_i |x_s,i - y_r,j|^2
//
// Both terms are ONE routine, direction_sum(queries, candidates), on the packed scan of nn1_scan.h without its chunk
// recording (no index is asked for): the queries of a direction live in registers as
// packed fp32 PAIRS (two queries per v_pk_add / v_pk_mul / v_pk_fma, each half IEEE-exact), the candidate cloud streams
// through LDS in 1024-point float4 tiles every lane reads at the same address (one broadcast read per point), and per
// (query, candidate) only the distance and a share of a minimum are issued (gfx950 has no packed fp32 minimum: the
// compiler folds two candidates into one v_min3_f32 per query): 3.5 VALU issue slots per point pair, which is what
// bounds the kernel -- a 2048^2 pair reads 48 KB and evaluates 8.4 M distances.  The distance is PDR_ACC3 on
// the differences, the expression tree of nn1_kernel (neighbors.hip), so every per-point minimum has the bits
// pdr_chamfer_nn returns; what is new is only the sum.
//
// SUMMATION ORDER (fixed by the code, no atomics: the same input gives the same bits).  Thread t of the 256 owns the
// queries t, t + 256, t + 512, ... of a direction and adds their minima to one accumulator in ascending order:
// ceil(n_q / 256) sequential additions (the first one to 0.0f is exact).  The 64 accumulators of a wave are summed by
// an xor butterfly (6 levels), the 4 wave sums as (w0 + w1) + (w2 + w3) (2 levels), then one division by the length and
// one addition of the two directions.  LONGEST CHAIN of dependent fp32 roundings:
//     ceil(max(n, m) / 256) + 6 + 2 + 1 + 1   =   74 for n, m <= 16384   (18 at 2048)
// which is what the test tolerance of 128 * 2^-24 rests on (every addend is >= 0).
// The order depends on the LENGTHS of the two clouds only, never on the padded sizes n / m, the position of the pair
// in the matrix or `symmetric`: a ragged pair gets the bits of the dense call on the two slices, and the symmetric path
// gets the bits of the plain call on (x, x) -- cd[s,r] = A/n_s + B/n_r and cd[r,s] = B/n_r + A/n_s there, the same two
// direction sums added in the other order, and fp32 addition commutes.
//
// GRID: one 256-thread workgroup per pair, pair = s * R + r in a 2-D grid (x up to 65536 wide).  The compiler reports
// 86 VGPRs, no scratch, 16,400 B of LDS: 5 waves per SIMD = 5 workgroups per CU, so S * R of a few hundred already puts
// a workgroup on every CU and 1280 pairs fill every slot; a pair is never split over workgroups because its sum would
// need a workspace or atomics.  symmetric: the workgroups of s > r exit at once, the owner of s <= r writes cd[s,r] and
// cd[r,s].  A thread holds 8 queries per pass (PDR_CDP_QP = 4 pairs): one broadcast LDS read serves 8 distances;
// measured at 256 x 256 clouds of 2048 points 55.3 ms against 59.0 ms with 4 queries (profiles/pairwise_cd.txt).
#include "nn1_scan.h"

namespace {

using pdr::kTile;

#ifndef PDR_CDP_QP
#define PDR_CDP_QP 4           // query PAIRS per thread and pass (lab builds: -DPDR_CDP_QP=2)
#endif

// sum over the queries q[0 .. nq) of min over the candidates c[0 .. nc) of the squared distance; nq, nc >= 1.
// Returned in every thread.  Rows at or beyond nq / nc are never loaded.
template <int QP>
__device__ __forceinline__ float direction_sum(const float* __restrict__ q, int nq, const float* __restrict__ c,
                                               int nc, float4* __restrict__ tile, float* __restrict__ wsum) {
  constexpr int NQ = 2 * QP;
  float acc[1] = {0.0f};
  for (int pass = 0; pass < nq; pass += 256 * NQ) {
    // thread t owns queries q0 + 256 i (coalesced loads); slots beyond nq shadow the last query and are not summed
    const int q0 = pass + threadIdx.x;
    pdr::Nn1State<QP> st;
    pdr::nn1_load(st, q, q0, nq - 1);
    pdr::nn1_scan<QP, false>(st, c, nc, tile);
#pragma unroll
    for (int s = 0; s < NQ; ++s)
      acc[0] += q0 + 256 * s < nq ? st.best[s >> 1][s & 1] : 0.0f;   // ascending query order; + 0.0f is exact
  }
  pdr::block_sum_256(acc, wsum);
  return acc[0];
}

template <int QP>
__global__ __launch_bounds__(256) void chamfer_pairs_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const int64_t* __restrict__ len_x,
                                                            const int64_t* __restrict__ len_y, int S, int R, int n,
                                                            int m, int symmetric, float* __restrict__ cd) {
  __shared__ float4 tile[kTile];
  __shared__ float wsum[4];
  const long long pair = static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x;
  if (pair >= static_cast<long long>(S) * R) return;            // uniform: the last grid row may be partial
  const int s = static_cast<int>(pair / R), r = static_cast<int>(pair % R);
  if (symmetric && s > r) return;                                // written by the owner of (r, s)
  const int ns = pdr::cloud_len(len_x, s, n), mr = pdr::cloud_len(len_y, r, m);
  float v = 0.0f;                                                // a pair with an empty side: calc_cd's 0
  if (ns > 0 && mr > 0) {
    const float* xs = x + static_cast<size_t>(s) * n * 3;
    const float* yr = y + static_cast<size_t>(r) * m * 3;
    const float a = direction_sum<QP>(xs, ns, yr, mr, tile, wsum);
    const float b = direction_sum<QP>(yr, mr, xs, ns, tile, wsum);
    v = a / static_cast<float>(ns) + b / static_cast<float>(mr);
  }
  if (threadIdx.x == 0) {
    cd[static_cast<size_t>(s) * R + r] = v;
    if (symmetric) cd[static_cast<size_t>(r) * R + s] = v;       // S == R; on the diagonal the same element twice
  }
}

}  // namespace

extern "C" int pdr_chamfer_pairwise(const float* x, const float* y, const int64_t* lengths_x, const int64_t* lengths_y,
                                    int S, int R, int n, int m, int symmetric, float* cd, pdr_stream_t stream) {
  if (S < 0 || R < 0 || n < 0 || m < 0) return PDR_EINVAL;
  if (symmetric && (x != y || lengths_x != lengths_y || S != R || n != m)) return PDR_EINVAL;
  if (S == 0 || R == 0) return PDR_OK;
  if (n <= 0 || m <= 0) return PDR_EINVAL;
  if (!x || !y || !cd) return PDR_EINVAL;
  const long long pairs = static_cast<long long>(S) * R;
  if (pairs > (1ll << 30)) return PDR_EUNSUPPORTED;
  const unsigned gx = pairs < 65536 ? static_cast<unsigned>(pairs) : 65536u;
  const unsigned gy = static_cast<unsigned>((pairs + gx - 1) / gx);   // <= 16384
  hipLaunchKernelGGL((chamfer_pairs_kernel<PDR_CDP_QP>), dim3(gx, gy), dim3(256), 0, pdr::as_stream(stream), x, y,
                     lengths_x, lengths_y, S, R, n, m, symmetric ? 1 : 0, cd);
  return pdr::check_launch();
}
