// act_ops.hip -- a layer's lazily-activated output, consumed WITHOUT a GEMM: the layer kernels leave y pre-GroupNorm and
// the next layer's A-loader applies the prologue (fused_layer.hip); where the consumer is not a layer kernel the same
// prologue is applied here -- materialised (pdr_apply_act) or reduced to a per-cloud column maximum (pdr_act_colmax).
#include "pdr_common.h"

namespace {

// resolved source of ONE input channel (a thread's column is fixed)
struct ColSrc {
  const float* ptr;  // segment base + channel offset
  int ld;
  int shift;         // log2(row_div): neighbour-broadcast divisors are powers of two here
};

__device__ __forceinline__ ColSrc resolve_col(const pdr_layer_in_t& in, int c) {
  ColSrc r;
  r.ptr = in.seg[0].ptr;
  r.ld = in.seg[0].ld;
  r.shift = 0;
  int c0 = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < in.n_seg) {
      const int cs = in.seg[s].C;
      if (c >= c0 && c < c0 + cs) {
        r.ptr = in.seg[s].ptr + (c - c0);
        r.ld = in.seg[s].ld;
        r.shift = __builtin_ctz(in.seg[s].row_div);
      }
      c0 += cs;
    }
  }
  return r;
}

__device__ __forceinline__ float load_col(const ColSrc& s, long row) {
  return s.ptr[(row >> s.shift) * s.ld];
}

// The activation of one value: ReLU placement (conv -> GN -> ReLU of the MLPs, ReLU -> GN -> conv of the attention score
// net) around the folded GroupNorm s, h.  The `if` form, not the GEMM prologues' fmaxf(x, lo) with lo = -inf: the two
// treat a NaN input differently.  The embedding add stays with the callers: apply_act_kernel skips an absent add,
// act_colmax_kernel adds 0, and x + 0 is not x for x = -0.
__device__ __forceinline__ float activate(const pdr_layer_in_t& in, float x, float s, float h) {
  if (in.pre_relu) x = fmaxf(x, 0.0f);
  x = __builtin_fmaf(x, s, h);
  if (in.post_relu) x = fmaxf(x, 0.0f);
  return x;
}

// out (P, C; ld ldo) = prologue(X): materialise an activation (needed where the next consumer
// gathers whole feature rows, e.g. group_build / gather_rows).  The residual is one row per position over all C
// channels: rseg.ptr[row * rseg.ld + c] -- rseg.C and rseg.row_div are not consulted.  Columns [C, ldo) are left alone.
__global__ __launch_bounds__(256) void apply_act_kernel(pdr_layer_in_t in, long P, int C,
                                                        float* __restrict__ out, int ldo) {
  const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= P * C) return;
  const long row = e / C;
  const int c = static_cast<int>(e - row * C);
  const int b = static_cast<int>(row / in.rows_per_batch);
  float v = load_col(resolve_col(in, c), row);
  const int ss_ld = in.ss_ld > 0 ? in.ss_ld : C;
  const float s = in.scale ? in.scale[static_cast<long>(b) * ss_ld + c] : 1.0f;
  const float h = in.shift ? in.shift[static_cast<long>(b) * ss_ld + c] : 0.0f;
  v = activate(in, v, s, h);
  if (in.add) v += in.add[static_cast<long>(b) * in.add_ld + c];
  if (in.rseg.ptr) v += in.rseg.ptr[row * in.rseg.ld + c];
  out[row * ldo + c] = v;
}

// out (B, C) = max over the rows of every batch element of prologue(X): the global max-pooling of Pnet2Stage
// (pnet.py:27-40 of the reference: F.max_pool2d over all points) applied to a layer's lazily-activated output, without
// materialising the activation.  256 threads = 64 channels x 4 row slices; a wave reads 256-byte row pieces.
__global__ __launch_bounds__(256) void act_colmax_kernel(pdr_layer_in_t in, int C, float* __restrict__ out) {
  __shared__ float red[4][64];
  const int b = blockIdx.y;
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int rpb = in.rows_per_batch;
  float m = -__builtin_inff();
  if (c < C) {
    const ColSrc src = resolve_col(in, c);
    const int ss_ld = in.ss_ld > 0 ? in.ss_ld : C;
    const float s = in.scale ? in.scale[static_cast<long>(b) * ss_ld + c] : 1.0f;
    const float h = in.shift ? in.shift[static_cast<long>(b) * ss_ld + c] : 0.0f;
    const float a = in.add ? in.add[static_cast<long>(b) * in.add_ld + c] : 0.0f;
    const long row0 = static_cast<long>(b) * rpb;
    for (int r = sl; r < rpb; r += 16) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + 4 * u;
        v[u] = load_col(src, row0 + (rr < rpb ? rr : r));       // (clamped: unconditional loads, all in flight)
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) m = fmaxf(m, activate(in, v[u], s, h) + a);
    }
  }
  red[sl][cl] = m;
  __syncthreads();
  if (sl == 0 && c < C)
    out[static_cast<long>(b) * C + c] = fmaxf(fmaxf(red[0][cl], red[1][cl]), fmaxf(red[2][cl], red[3][cl]));
}

}  // namespace

extern "C" int pdr_apply_act(const pdr_layer_in_t* in, long P, int C, float* out, int ldo,
                             pdr_stream_t stream) {
  if (!in || !out || P < 0 || C <= 0 || in->n_seg < 1 || in->n_seg > 4 || in->rows_per_batch <= 0)
    return PDR_EINVAL;
  if (in->rseg.gV) return PDR_EUNSUPPORTED;   // gathered sources: pdr_fused_layer only
  if (P == 0) return PDR_OK;
  int ctot = 0;
  for (int s = 0; s < in->n_seg; ++s) {
    if (in->seg[s].row_div < 1 || (in->seg[s].row_div & (in->seg[s].row_div - 1))) return PDR_EUNSUPPORTED;
    if (in->seg[s].gV) return PDR_EUNSUPPORTED;
    ctot += in->seg[s].C;
  }
  if (ctot != C) return PDR_EINVAL;
  hipLaunchKernelGGL(apply_act_kernel, dim3(static_cast<unsigned>((P * C + 255) / 256)), dim3(256), 0,
                     pdr::as_stream(stream), *in, P, C, out, ldo);
  return pdr::check_launch();
}

extern "C" int pdr_act_colmax(const pdr_layer_in_t* in, long P, int C, float* out, pdr_stream_t stream) {
  if (!in || !out || P < 0 || C <= 0 || in->n_seg < 1 || in->n_seg > 4 || in->rows_per_batch <= 0 ||
      P % in->rows_per_batch != 0)
    return PDR_EINVAL;
  if (in->rseg.ptr || in->oadd) return PDR_EUNSUPPORTED;   // plain prologue only
  if (P == 0) return PDR_OK;
  int ctot = 0;
  for (int s = 0; s < in->n_seg; ++s) {
    if (!in->seg[s].ptr || in->seg[s].row_div < 1 || (in->seg[s].row_div & (in->seg[s].row_div - 1)))
      return PDR_EUNSUPPORTED;
    if (in->seg[s].gV) return PDR_EUNSUPPORTED;
    ctot += in->seg[s].C;
  }
  if (ctot != C) return PDR_EINVAL;
  const dim3 grid(static_cast<unsigned>((C + 63) / 64), static_cast<unsigned>(P / in->rows_per_batch));
  hipLaunchKernelGGL(act_colmax_kernel, grid, dim3(256), 0, pdr::as_stream(stream), *in, C, out);
  return pdr::check_launch();
}
