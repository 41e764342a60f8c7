// dedup.hip -- neighbourhoods that are K copies of one row: the plan that finds them, and the
// moments and pooled rows that the per-query side chain supplies in their place.
//
// ball_query pads a neighbourhood with its first hit; a query with at most ONE neighbour in its ball (count <= 1; an
// empty ball of a feature-transfer block is replaced by the query itself) therefore contributes K identical rows to
// every per-neighbour tensor of its block: the convs repeat one row K times, the attention pooling returns that row's
// value (one unmasked slot), the GroupNorm moments count it K times.  On x_t of a reverse process (noise for most of
// the trajectory) that is the rule, not the exception.  pdr_dedup_plan marks the 128-row tiles (128 / K queries)
// ALL of whose queries are such copies; the block's per-neighbour launches skip them (pdr_layer_in_t.tile_list,
// pdr_gather_add_tiles) and a K times smaller per-QUERY chain of the same layers supplies their moments
// (pdr_weighted_moments) and their pooled rows (pdr_patch_rows).  Same values as the full evaluation up to fp32
// summation order of the moments.
#include "pdr_common.h"

// (1) per tile, in parallel: the valid flag, its queries' weights and first neighbours
__global__ __launch_bounds__(256) void dedup_flags_kernel(const int* __restrict__ idx, const int* __restrict__ counts,
                                                          int K, long nq, int qpt, int* __restrict__ idx0,
                                                          float* __restrict__ row_w,
                                                          unsigned char* __restrict__ tile_valid) {
  const long q = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;   // 256 / qpt whole tiles per workgroup
  if (q >= nq) return;
  const int cnt = counts[q];
  idx0[q] = idx[q * K];
  // a tile's qpt (2 .. 16, a power of two) queries sit in consecutive lanes of one wave
  int v = cnt > 1 ? 1 : 0;
  for (int off = 1; off < qpt; off <<= 1) v |= __shfl_xor(v, off, 64);   // (every lane takes part in every exchange)
  const bool valid = v != 0;
  row_w[q] = valid ? 0.0f : static_cast<float>(K);
  if ((q & (qpt - 1)) == 0) tile_valid[q / qpt] = valid ? 1 : 0;
}

// (2) ONE workgroup: ordered compaction of the valid tile numbers (ballot prefix per wave, wave totals through LDS,
// chunks of 1024 tiles in ascending order)
__global__ __launch_bounds__(1024) void dedup_compact_kernel(const unsigned char* __restrict__ tile_valid, int ntiles,
                                                            int* __restrict__ tile_list, int* __restrict__ n_tiles) {
  __shared__ int wtot[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int i0 = 0; i0 < ntiles; i0 += 1024) {
    const int i = i0 + tid;
    const bool valid = i < ntiles && tile_valid[i] != 0;
    const unsigned long long bal = __ballot(valid);
    const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < 16; ++w) {
      woff += w < wave ? wtot[w] : 0;
      tot += wtot[w];
    }
    const int base = base_s;
    if (valid) tile_list[base + woff + before] = i;
    __syncthreads();
    if (tid == 0) base_s = base + tot;
    __syncthreads();
  }
  if (tid == 0) *n_tiles = base_s;
}

// Stable partition of a cloud's queries: those with more than one neighbour first (in their original order), the
// one-point ones behind them.  perm[b][j] = original index of the query at sorted position j, inv = its inverse.
// One workgroup per cloud; chunks of 1024 queries, two passes (real neighbourhoods, then the rest).
__global__ __launch_bounds__(1024) void dedup_sort_kernel(const int* __restrict__ counts, int m,
                                                         int* __restrict__ perm, int* __restrict__ inv,
                                                         int* __restrict__ perm_rows) {
  __shared__ int wtot[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* cb = counts + static_cast<long>(blockIdx.x) * m;
  int* pb = perm + static_cast<long>(blockIdx.x) * m;
  int* ib = inv + static_cast<long>(blockIdx.x) * m;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int i0 = 0; i0 < m; i0 += 1024) {
      const int i = i0 + tid;
      const bool take = i < m && ((cb[i] > 1) == (pass == 0));
      const unsigned long long bal = __ballot(take);
      const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wtot[wave] = __builtin_popcountll(bal);
      __syncthreads();
      int woff = 0, tot = 0;
      for (int w = 0; w < 16; ++w) {
        woff += w < wave ? wtot[w] : 0;
        tot += wtot[w];
      }
      const int base = base_s;
      if (take) {
        const int j = base + woff + before;
        pb[j] = i;
        ib[i] = j;
        if (perm_rows) perm_rows[static_cast<long>(blockIdx.x) * m + j] = static_cast<int>(blockIdx.x) * m + i;
      }
      __syncthreads();
      if (tid == 0) base_s = base + tot;
      __syncthreads();
    }
  }
}

// counts (B, m) -> perm, inv (B, m) int32: see dedup_sort_kernel.  A block evaluated on its queries in `perm` order
// (pdr_gather_rows of its per-query inputs) has its one-point neighbourhoods in whole tiles; pdr_gather_rows with
// `inv` puts its output back.
extern "C" int pdr_dedup_sort(const int* counts, int B, int m, int* perm, int* inv, int* perm_rows,
                              pdr_stream_t stream) {
  if (!counts || !perm || !inv || B < 0 || m <= 0 || static_cast<long>(B) * m >= (1L << 31)) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  hipLaunchKernelGGL(dedup_sort_kernel, dim3(B), dim3(1024), 0, pdr::as_stream(stream), counts, m, perm, inv, perm_rows);
  return pdr::check_launch();
}

// idx (B, m, K) int32 / counts (B, m) of a ball query ->
//   idx0 (B, m): the first neighbour of every query;  row_w (B, m) float: K for the queries of skipped tiles, else 0;
//   tile_valid (B * m K / 128) bytes, tile_list (same length, the valid tile numbers in ascending order), n_tiles (1).
// A tile = 128 rows = 128 / K queries is VALID (computed by the per-neighbour launches) when any of its queries has
// more than one neighbour.  K in {8, 16, 32}, m K a multiple of 128.
extern "C" int pdr_dedup_plan(const int* idx, const int* counts, int B, int m, int K, int* idx0, float* row_w,
                              unsigned char* tile_valid, int* tile_list, int* n_tiles, pdr_stream_t stream) {
  if (!idx || !counts || !idx0 || !row_w || !tile_valid || !tile_list || !n_tiles || B < 0 || m <= 0) return PDR_EINVAL;
  if (!(K == 8 || K == 16 || K == 32) || (static_cast<long>(m) * K) % 128 != 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  const int qpt = 128 / K;
  const long ntiles = static_cast<long>(B) * m / qpt;
  if (ntiles >= (1L << 30)) return PDR_EINVAL;
  const long nq = static_cast<long>(B) * m;
  hipLaunchKernelGGL(dedup_flags_kernel, dim3(pdr::blocks_for(nq)), dim3(256), 0, pdr::as_stream(stream), idx, counts, K,
                     nq, qpt, idx0, row_w, tile_valid);
  hipLaunchKernelGGL(dedup_compact_kernel, dim3(1), dim3(1024), 0, pdr::as_stream(stream), tile_valid,
                     static_cast<int>(ntiles), tile_list, n_tiles);
  return pdr::check_launch();
}

// ---- sort + gathers + plan in ONE launch (round 5) ------------------------------------------------------------------
// pdr_dedup_sort, the three pdr_gather_rows of the sorted index rows / counts / query coordinates and the two kernels
// of pdr_dedup_plan were six dependent launches behind every ball query of the x_t branch -- at the head of a step they
// sit between the first ball query and the first block (0.13 -> 0.38 ms in profiles/r4_timeline_markers.json).  With
// the queries SORTED a cloud's valid tiles are simply its first nv = ceil(real / (128 / K)) tiles, so the whole plan is
// a count + a stable partition per cloud: one 1024-thread workgroup per cloud does all of it.
//   (1) real neighbourhoods (count > 1) of clouds 0 .. b -> this cloud's nv and the offset of its tiles in the list
//       (every workgroup recounts its predecessors: B m int loads, L2 hits -- no inter-workgroup communication);
//   (2) the stable partition of pdr_dedup_sort (perm / inv / perm_rows);
//   (3) rows gathered into that order: index rows (K ints = 16-byte pieces), counts, coordinates, first neighbours,
//       weights (K behind the cloud's valid tiles, else 0);
//   (4) tile flags, the ascending tile list, per-cloud [nv | first weighted query], the probe counters.
constexpr int kMaxPrepareClouds = 1024;
constexpr int kMaxPrepareQueries = 4096;   // a cloud's permutation lives in LDS (16 KB)

__global__ __launch_bounds__(1024) void dedup_prepare_kernel(
    const int* __restrict__ idx, const int* __restrict__ counts, const float* __restrict__ xyz, int m, int K, int nB,
    int* __restrict__ perm, int* __restrict__ inv, int* __restrict__ perm_rows, int* __restrict__ idx_s,
    int* __restrict__ counts_s, float* __restrict__ xyz_s, int* __restrict__ idx0, float* __restrict__ row_w,
    unsigned char* __restrict__ tile_valid, int* __restrict__ tile_list, int* __restrict__ n_tiles,
    int* __restrict__ nvalid, int* __restrict__ probe_acc) {
  __shared__ int nreal_s[kMaxPrepareClouds];
  __shared__ int perm_s[kMaxPrepareQueries];
  __shared__ int wtot[16];
  __shared__ int base_s, prefix_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int qpt = 128 / K, tpb = m / qpt;
  if (tid == 0) base_s = 0;
  // (1) one WAVE per cloud 0 .. b (waves take clouds wave, wave + 16, ...): every lane's loads of a cloud are
  // independent and issued together -- a 16-byte load per 4 counts where the rows allow it
  const bool vec = (m & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 15) == 0;   // uniform
  for (int bb = wave; bb <= b; bb += 16) {
    const int* cb = counts + static_cast<long>(bb) * m;
    int c = 0;
    if (vec) {
      const int4* c4 = reinterpret_cast<const int4*>(cb);
      const int n4 = m >> 2;
      for (int i0 = 0; i0 < n4; i0 += 64 * 8) {
        int4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 64 * u + lane;
          v[u] = c4[i < n4 ? i : 0];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool ok = i0 + 64 * u + lane < n4;
          c += ok ? (v[u].x > 1) + (v[u].y > 1) + (v[u].z > 1) + (v[u].w > 1) : 0;
        }
      }
    } else {
      for (int i = lane; i < m; i += 64) c += cb[i] > 1 ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) nreal_s[bb] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int p = 0;
    for (int bb = 0; bb < b; ++bb) p += (nreal_s[bb] + qpt - 1) / qpt;
    prefix_s = p;
  }
  const int nv = (nreal_s[b] + qpt - 1) / qpt;       // valid tiles of this cloud: its first nv
  const int q0 = nv * qpt;                            // first query of the skipped tiles
  // (2) stable partition: real neighbourhoods first
  const int* cb = counts + static_cast<long>(b) * m;
  int* pb = perm + static_cast<long>(b) * m;
  int* ib = inv + static_cast<long>(b) * m;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i0 = 0; i0 < m; i0 += 1024) {
      const int i = i0 + tid;
      const bool take = i < m && ((cb[i] > 1) == (pass == 0));
      const unsigned long long bal = __ballot(take);
      const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wtot[wave] = __builtin_popcountll(bal);
      __syncthreads();
      int woff = 0, tot = 0;
      for (int w = 0; w < 16; ++w) {
        woff += w < wave ? wtot[w] : 0;
        tot += wtot[w];
      }
      const int base = base_s;
      if (take) {
        const int j = base + woff + before;
        perm_s[j] = i;
        pb[j] = i;
        ib[i] = j;
        if (perm_rows) perm_rows[static_cast<long>(b) * m + j] = b * m + i;
      }
      __syncthreads();
      if (tid == 0) base_s = base + tot;
      __syncthreads();
    }
  }
  // (3) per-query rows in sorted order (the permutation comes from LDS: no global round trip in front of every row)
  for (int j = tid; j < m; j += 1024) {
    const int src = perm_s[j];
    const long qs = static_cast<long>(b) * m + src, qd = static_cast<long>(b) * m + j;
    counts_s[qd] = cb[src];
    idx0[qd] = idx[qs * K];
    row_w[qd] = j >= q0 ? static_cast<float>(K) : 0.0f;
    if (xyz) {
      const float x = xyz[qs * 3 + 0], y = xyz[qs * 3 + 1], z = xyz[qs * 3 + 2];
      xyz_s[qd * 3 + 0] = x;
      xyz_s[qd * 3 + 1] = y;
      xyz_s[qd * 3 + 2] = z;
    }
  }
  // index rows as 16-byte pieces, four in flight per thread
  const int k4 = K / 4, ksh4 = __builtin_ctz(k4);     // (K in {8, 16, 32}: 2, 4 or 8 pieces per row)
  const int npiece = m * k4;
  const int4* src4 = reinterpret_cast<const int4*>(idx + static_cast<long>(b) * m * K);
  int4* dst4 = reinterpret_cast<int4*>(idx_s + static_cast<long>(b) * m * K);
  for (int e0 = 0; e0 < npiece; e0 += 4096) {
    int4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = min(e0 + 1024 * u + tid, npiece - 1);
      v[u] = src4[(perm_s[e >> ksh4] << ksh4) + (e & (k4 - 1))];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + 1024 * u + tid;
      if (e < npiece) dst4[e] = v[u];
    }
  }
  // (4) tiles
  const int prefix = prefix_s;
  for (int t = tid; t < tpb; t += 1024) {
    tile_valid[static_cast<long>(b) * tpb + t] = t < nv ? 1 : 0;
    if (t < nv) tile_list[prefix + t] = b * tpb + t;
  }
  if (tid == 0) {
    nvalid[b] = nv;
    nvalid[nB + b] = q0;
    if (b == nB - 1) *n_tiles = prefix + nv;
    if (probe_acc) {
      atomicAdd(&probe_acc[0], nv);
      atomicAdd(&probe_acc[1], tpb);
    }
  }
}

// The same count without the plan (the step with every neighbourhood evaluated carries it so that the sampler can tell
// when the deduplicated step would be the faster one again): probe_acc[0] += tiles a plan would walk, [1] += tiles.
__global__ __launch_bounds__(256) void dedup_probe_kernel(const int* __restrict__ counts, int m, int K,
                                                          int* __restrict__ probe_acc) {
  __shared__ int tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  const int* cb = counts + static_cast<long>(blockIdx.x) * m;
  int c = 0;
  for (int i = threadIdx.x; i < m; i += 256) c += cb[i] > 1 ? 1 : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&tot, c);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int qpt = 128 / K;
    atomicAdd(&probe_acc[0], (tot + qpt - 1) / qpt);
    atomicAdd(&probe_acc[1], m / qpt);
  }
}

// idx (B, m, K) int32 / counts (B, m) of a ball query, xyz (B, m, 3) query coordinates (may be NULL) -> everything a
// grouped block needs to evaluate its one-point neighbourhoods once, in ONE launch (= pdr_dedup_sort + pdr_gather_rows
// of idx / counts / xyz + pdr_dedup_plan on the sorted arrays, same values):
//   perm, inv, perm_rows (B, m): the stable partition (real neighbourhoods first) as in pdr_dedup_sort;
//   idx_s (B, m, K), counts_s (B, m), xyz_s (B, m, 3): the inputs in that order;
//   idx0, row_w (B, m), tile_valid (B m K / 128), tile_list, n_tiles: as pdr_dedup_plan on the sorted arrays;
//   nvalid (2 B ints): [b] = valid tiles of cloud b (its FIRST nv tiles), [B + b] = nv * (128 / K) = the first query of
//   its skipped tiles (pdr_layer_in_t.wrow0 of the per-query launches);
//   probe_acc (NULL or 2 ints): [0] += sum_b nv, [1] += B m K / 128.
extern "C" int pdr_dedup_prepare(const int* idx, const int* counts, const float* xyz, int B, int m, int K, int* perm,
                                 int* inv, int* perm_rows, int* idx_s, int* counts_s, float* xyz_s, int* idx0,
                                 float* row_w, unsigned char* tile_valid, int* tile_list, int* n_tiles, int* nvalid,
                                 int* probe_acc, pdr_stream_t stream) {
  if (!idx || !counts || !perm || !inv || !idx_s || !counts_s || (xyz && !xyz_s) || !idx0 || !row_w || !tile_valid ||
      !tile_list || !n_tiles || !nvalid || B < 0 || m <= 0)
    return PDR_EINVAL;
  if (!(K == 8 || K == 16 || K == 32) || (static_cast<long>(m) * K) % 128 != 0) return PDR_EINVAL;
  if (static_cast<long>(B) * m * K >= (1L << 31)) return PDR_EINVAL;
  if (B > kMaxPrepareClouds || m > kMaxPrepareQueries) return PDR_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(idx_s)) % 16 != 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  hipLaunchKernelGGL(dedup_prepare_kernel, dim3(B), dim3(1024), 0, pdr::as_stream(stream), idx, counts, xyz, m, K, B,
                     perm, inv, perm_rows, idx_s, counts_s, xyz_s, idx0, row_w, tile_valid, tile_list, n_tiles, nvalid,
                     probe_acc);
  return pdr::check_launch();
}

extern "C" int pdr_dedup_probe(const int* counts, int B, int m, int K, int* probe_acc, pdr_stream_t stream) {
  if (!counts || !probe_acc || B < 0 || m <= 0) return PDR_EINVAL;
  if (!(K == 8 || K == 16 || K == 32) || (static_cast<long>(m) * K) % 128 != 0) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  hipLaunchKernelGGL(dedup_probe_kernel, dim3(B), dim3(256), 0, pdr::as_stream(stream), counts, m, K, probe_acc);
  return pdr::check_launch();
}

// Per-tile GroupNorm moments of a materialised (B rpb, C) tensor with one WEIGHT per row, written behind the
// moments of a tile subset: block (j, cy) handles rows [128 j, 128 j + 128) of batch element b = j / tpbd and 64
// columns; the trailing blocks zero the partial rows of the tiles the subset skipped.
__global__ __launch_bounds__(256) void weighted_moments_kernel(const float* __restrict__ Y, int ldy, int C, int rpb,
                                                               int tpbd, int nB, int relu_col0,
                                                               const float* __restrict__ row_w,
                                                               float* __restrict__ partial, int ptpb, int tpb_full,
                                                               const unsigned char* __restrict__ tile_valid) {
  const int nmom = nB * tpbd;
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  if (static_cast<int>(blockIdx.x) >= nmom) {
    // zero the rows of skipped tiles: 16 tiles per block, this block's 64 columns
    const int t0 = (static_cast<int>(blockIdx.x) - nmom) * 16;
    for (int k = sl; k < 16; k += 4) {
      const int t = t0 + k;
      if (t < nB * tpb_full && !tile_valid[t] && c < C) {
        const int b = t / tpb_full, tb = t - b * tpb_full;
        float* o = partial + ((static_cast<long>(b) * ptpb + tb) * C + c) * 2;
        o[0] = 0.0f;
        o[1] = 0.0f;
      }
    }
    return;
  }
  __shared__ float red[4][64][2];
  const int b = blockIdx.x / tpbd, j = blockIdx.x - b * tpbd;
  const int r0 = j * 128 + sl * 32, r1 = min(r0 + 32, rpb);
  float s1 = 0.0f, s2 = 0.0f;
  if (c < C) {
    const float lo = c >= relu_col0 ? 0.0f : -__builtin_inff();
    const float* yp = Y + (static_cast<long>(b) * rpb) * ldy + c;
    const float* wp = row_w + static_cast<long>(b) * rpb;
    // a launch of a few microseconds: every load of a thread in flight at once (a row loop of dependent-looking loads
    // took 12 us), and no row of Y is read for a slice whose weights are all zero (sorted queries: the rule)
    float w[32];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      w[k] = r0 + k < r1 ? wp[min(r0 + k, rpb - 1)] : 0.0f;
      any = any || w[k] > 0.0f;
    }
    if (any) {
#pragma unroll
      for (int k0 = 0; k0 < 32; k0 += 16) {
        float y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = yp[static_cast<long>(min(r0 + k0 + k, rpb - 1)) * ldy];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const float f = fmaxf(y[k], lo);
          s1 = __builtin_fmaf(w[k0 + k], f, s1);
          s2 = __builtin_fmaf(w[k0 + k] * f, f, s2);
        }
      }
    }
  }
  red[sl][cl][0] = s1;
  red[sl][cl][1] = s2;
  __syncthreads();
  if (sl == 0 && c < C) {
    float* o = partial + ((static_cast<long>(b) * ptpb + tpb_full + j) * C + c) * 2;
    o[0] = (red[0][cl][0] + red[1][cl][0]) + (red[2][cl][0] + red[3][cl][0]);
    o[1] = (red[0][cl][1] + red[1][cl][1]) + (red[2][cl][1] + red[3][cl][1]);
  }
}

// partial (B * ptpb, C, 2): rows [b ptpb + tpb_full + j] (j < ceil(rpb / 128)) <- sum_r w[r] f, sum_r w[r] f^2 over the
// rows of tile j of Y (B rpb, C; ld ldy), f = y (columns >= relu_col0: max(y, 0)); rows [b ptpb + t] of the tiles
// t < tpb_full with tile_valid[b tpb_full + t] == 0 <- 0.  ptpb >= tpb_full + ceil(rpb / 128).
extern "C" int pdr_weighted_moments(const float* Y, int ldy, int B, int rpb, int C, int relu_col0, const float* row_w,
                                    float* partial, int ptpb, int tpb_full, const unsigned char* tile_valid,
                                    pdr_stream_t stream) {
  if (!Y || !row_w || !partial || !tile_valid || B < 0 || rpb <= 0 || C <= 0 || ldy < C || tpb_full <= 0) return PDR_EINVAL;
  const int tpbd = (rpb + 127) / 128;
  if (ptpb < tpb_full + tpbd) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  const long nz = (static_cast<long>(B) * tpb_full + 15) / 16;
  const dim3 grid(static_cast<unsigned>(static_cast<long>(B) * tpbd + nz), static_cast<unsigned>((C + 63) / 64));
  hipLaunchKernelGGL(weighted_moments_kernel, grid, dim3(256), 0, pdr::as_stream(stream), Y, ldy, C, rpb, tpbd, B,
                     relu_col0, row_w, partial, ptpb, tpb_full, tile_valid);
  return pdr::check_launch();
}

// out[q, :D] = act(V[q, :D] * vscale[b] + vshift[b]) for the rows q with row_w[q] > 0 (the pooled output of a query
// whose neighbourhood is K copies of one row is that row's activated value); other rows untouched.
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ V, int ldv,
                                                         const float* __restrict__ vscale,
                                                         const float* __restrict__ vshift, int v_relu,
                                                         const float* __restrict__ row_w, int rpb, int D, long total,
                                                         float* __restrict__ out, int ldo,
                                                         const int* __restrict__ out_rows) {
  const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const long q = e / D;
  const int d = static_cast<int>(e - q * D);
  if (!(row_w[q] > 0.0f)) return;
  const long b = q / rpb;
  float v = V[q * ldv + d];
  const float s = vscale ? vscale[b * D + d] : 1.0f;
  const float h = vshift ? vshift[b * D + d] : 0.0f;
  v = __builtin_fmaf(v, s, h);
  if (v_relu) v = fmaxf(v, 0.0f);
  out[(out_rows ? static_cast<long>(out_rows[q]) : q) * ldo + d] = v;
}

extern "C" int pdr_patch_rows(const float* V, int ldv, const float* vscale, const float* vshift, int v_relu,
                              const float* row_w, int B, int rpb, int D, float* out, int ldo, const int* out_rows,
                              pdr_stream_t stream) {
  if (!V || !row_w || !out || B < 0 || rpb <= 0 || D <= 0 || ldv < D || ldo < D) return PDR_EINVAL;
  if (B == 0) return PDR_OK;
  const long total = static_cast<long>(B) * rpb * D;
  hipLaunchKernelGGL(patch_rows_kernel, dim3(pdr::blocks_for(total)), dim3(256), 0, pdr::as_stream(stream), V, ldv, vscale,
                     vshift, v_relu, row_w, rpb, D, total, out, ldo, out_rows);
  return pdr::check_launch();
}
