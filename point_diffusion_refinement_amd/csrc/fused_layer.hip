// fused_layer.hip -- one pass per shared-MLP layer of PDR's grouped point MLPs.
//
// The reference evaluates every `Conv2d 1x1 -> GroupNorm -> ReLU (+ t / condition
// embedding) (+ residual)` stage of Mlp_plus_t_emb / AttentionModule
// (pointnet2_modules.py:69-174, attention.py:35-96) as 4-8 separate full passes
// over a materialised (B, C, npoint, K) tensor (conv, GN moments, GN apply, ReLU,
// broadcast adds, torch.cat of the inputs).  On MI355X those passes are pure HBM
// traffic: the first profile of a reverse step spent 70 % of its time in
// cat / elementwise / moments kernels and 14 TFLOP/s in the convolutions.
//
// Here a layer is ONE kernel over channel-LAST activations X (P positions x Cin):
//
//   A-loader : x' = post( pre(x) * scale[b,c] + shift[b,c] ) + add[b,c] + R[p,c]
//              - x is the concatenation of up to 4 channel segments, each with its own
//                pointer / leading dimension / neighbour-broadcast divisor, so the
//                torch.cat([q.expand(K), k]) and cat([feat, skip, xyz]) tensors of the
//                reference are never built;
//              - scale/shift = the PRODUCER layer's GroupNorm folded to per-(batch,
//                channel) affine form, pre/post = ReLU placement (conv->GN->ReLU of the
//                MLPs vs ReLU->GN->conv of the attention score net), add = fc(t_emb) /
//                fc_condition / fc_second_condition rows, R = the residual branch.
//   GEMM     : Y = x' . Wt (+ bias) with v_mfma_f32_32x32x2_f32 -- exact fp32 (bitwise
//              an fmaf chain), 4 waves x (32 rows x up to 128 columns), A and W staged
//              k-major through LDS so every ds_read_b32 is conflict-free.
//   epilogue : per-(tile, channel) partial sums of f(y), f(y)^2 (f = identity or ReLU)
//              for the NEXT GroupNorm -- reduced and folded deterministically by pdr_gn_fold
//              (gn_stats.hip), no atomics.
//
// Roofline: at the dominant shapes (P = 2.1 M positions, C = 32-96) the layer moves
// 4 (Cin + Cout) bytes per position for 2 Cin Cout flops: 5-20 flop/B, i.e. HBM-bound
// (machine balance ~25 flop/B at the 157 TF fp32-MFMA peak).
#include "layer_tiles.h"

#include <cstdlib>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// Block tile TM x TN = (WR*RT*32) x (WC*CT*32); wave (wr, wc) owns RT x CT MFMA tiles of 32x32.
// grid.x strides over the row tiles (cut per batch element), grid.y = column blocks.
// K is walked segment by segment in chunks of KC channels, so within a chunk the source
// pointer / leading dimension / broadcast shift are wave-uniform (scalar registers) and every A
// load is `scalar base + 32-bit lane offset`.
// Pipeline per chunk: global -> registers (prologue applied) is issued BEFORE the MFMAs of the
// previous chunk, registers -> LDS after them: the loads overlap the matrix pipe.
using pdr::PoolArgs;   // POOL epilogue (pdr_common.h)

// KS (round 5): the four waves split the K walk KS ways -- wave (wr, wc, kq) multiplies the k-pairs kq, kq + KS, ... of
// every chunk into its own accumulators, the partial products are summed through LDS before the epilogue (in the
// fixed order kq = 0, 1, ...).  For the tiny layers of plan_layer: their time is the length of a wave's MFMA chain.
template <int RT, int CT, int WR, int WC, int KC, bool RADD, bool VEC, bool GATH, bool POOL = false, int KS = 1>
__global__ __launch_bounds__(256, 2) void fused_layer_kernel(
    pdr_layer_in_t in, int Cin, const float* __restrict__ Wt, int ldw,
    const float* __restrict__ bias, int Cout, float* __restrict__ Y, int ldy,
    float* __restrict__ partial, int relu_col0, int n_row_tiles, PoolArgs pool = PoolArgs()) {
  static_assert(WR * WC * KS == 4, "4 waves per workgroup");
  static_assert(KS == 1 || !POOL, "pooled epilogue: no K split");
  constexpr int TM = WR * RT * 32, TN = WC * CT * 32;
  // scalar A path: thread -> (column ac, rows ar0 + RSTEP i)
  constexpr int APT = TM * KC / 256;
  constexpr int RSTEP = 256 / KC;
  // vector A path (VEC: every segment 16-B aligned, ld % 4 == 0): thread -> (float4 column vc4,
  // rows vr0 + VSTEP i): 4x fewer load instructions and address computations
  constexpr int C4 = KC / 4;
  constexpr int VSTEP = 256 / C4;
  constexpr int APT4 = TM / VSTEP;
  // W chunk (always float4; Wt is packed with ldw % 4 == 0): element e4 = tid + 256 i
  constexpr int TN4 = TN / 4;
  constexpr int WPT4 = (KC * TN4 + 255) / 256;
  __shared__ float As[KC][TM + 1];
  __shared__ __attribute__((aligned(16))) float Bs[KC][TN + 4];
  __shared__ float red[WR][TN][2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave % WR, wc = KS == 1 ? wave / WR : (wave / WR) % WC, kq = KS == 1 ? 0 : wave / (WR * WC);
  const int il = lane & 31, hi = lane >> 5;
  const int rpb = in.rows_per_batch;
  const int tpb = (rpb + TM - 1) / TM;
  const int n0 = blockIdx.y * TN;
  const float lo_pre = in.pre_relu ? 0.0f : -__builtin_inff();
  const float lo_post = in.post_relu ? 0.0f : -__builtin_inff();
  const bool single_chunk = in.n_seg == 1 && Cin <= KC;   // W staged once per workgroup
  bool w_loaded = false;

  float bias_r[CT];   // this lane's bias per column tile (the column block is fixed per workgroup)
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int col = n0 + (wc * CT + j) * 32 + il;
    bias_r[j] = (bias && col < Cout) ? bias[col] : 0.0f;
  }
  // registers of the chunk in flight
  float ra[VEC ? 1 : APT], rr[(RADD && !VEC) ? APT : 1];
  float4 rv[VEC ? APT4 : 1], rrv[(RADD && VEC) ? APT4 : 1];
  // gathered sources (GATH): second operand (query row) of the chunk / residual in flight, and this
  // thread's per-tile neighbour indices / empty-ball flags (its rows are the same for every chunk)
  float4 rv2[GATH ? APT4 : 1], rrv2[(GATH && RADD) ? APT4 : 1];
  int tidx[GATH ? APT4 : 1], tem[GATH ? APT4 : 1];
  bool f_g = false;            // chunk in flight comes from a gathered segment
  const int gshift = GATH ? __builtin_ctz(in.gK) : 0;
  float4 rwv[WPT4];
  float ps[VEC ? 4 : 1], ph[VEC ? 4 : 1], pa[VEC ? 4 : 1];   // per-channel prologue parameters
  float pok[(VEC && RADD) ? 4 : 1];                           // 1 / 0: channel inside the segment
  float f_s = 1.0f, f_h = 0.0f, f_a = 0.0f;
  bool f_cok = false;
  int f_kmax = 0;
  int f_okm = 0;               // VEC: bit j = channel j of this thread's float4 lies inside the segment

  for (int tile = blockIdx.x; tile < n_row_tiles; tile += gridDim.x) {
    const int b = tile / tpb, tb = tile - b * tpb;
    const long row0 = static_cast<long>(b) * rpb + static_cast<long>(tb) * TM;
    const int nvalid = min(TM, rpb - tb * TM);
    const int ss_ld = in.ss_ld > 0 ? in.ss_ld : Cin;
    const float* sc_b = in.scale ? in.scale + static_cast<long>(b) * ss_ld : nullptr;
    const float* sh_b = in.shift ? in.shift + static_cast<long>(b) * ss_ld : nullptr;
    const float* ad_b = in.add ? in.add + static_cast<long>(b) * in.add_ld : nullptr;
    const float* rd_b = in.rseg.ptr ? in.rseg.ptr + row0 * in.rseg.ld : nullptr;   // plain residual
    if constexpr (GATH) {
#pragma unroll
      for (int i = 0; i < APT4; ++i) {
        const int r = min(tid / C4 + VSTEP * i, nvalid - 1);
        tidx[i] = in.gidx[row0 + r];
        tem[i] = (in.gcnt && in.gcnt[(row0 + r) >> gshift] <= 0) ? 1 : 0;
      }
    }

    // fetch(): ONLY address arithmetic + loads -- nothing consumes a loaded value, so no
    // s_waitcnt is emitted and the loads stay in flight across the MFMA loop that follows.
    // commit(): prologue math on the arrived values + LDS stores.
    // (sg, ks, cbase): segment, channel offset inside it, global channel index of its first channel
    auto fetch = [&](int sg, int ks, int cbase) {
      // `opaque`: re-materialise the per-thread indices on every call.  Without it LLVM hoists the
      // loop-invariant row / address values out of the chunk loop and keeps them alive across the
      // MFMA loop (>100 VGPRs, occupancy 1).
      int t = tid;
      asm volatile("" : "+v"(t));
      const pdr_seg_t seg = in.seg[sg];
      const int shift = __builtin_ctz(seg.row_div);
      const float* abase = seg.ptr + (row0 >> shift) * seg.ld;      // uniform; row0 % row_div == 0
      f_kmax = min(KC, seg.C - ks);                                  // valid channels in this chunk
      if constexpr (VEC) {
        const int vc4 = t % C4, vr0 = t / C4;
        const int cl = ks + 4 * vc4;                                 // first channel of this float4
        const int clc = min(cl, ((seg.C + 3) & ~3) - 4);             // keep the 16-B load in the row
        f_cok = cl == clc;                                           // else: all 4 lanes are padding
        f_okm = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = f_cok && (clc + j) < seg.C;
          f_okm |= ok ? 1 << j : 0;
          const int cg = cbase + min(clc + j, seg.C - 1);
          // channels beyond the segment are forced to 0 (scale = shift = add = 0)
          ps[j] = ok ? (sc_b ? sc_b[cg] : 1.0f) : 0.0f;
          ph[j] = (ok && sh_b) ? sh_b[cg] : 0.0f;
          pa[j] = (ok && ad_b) ? ad_b[cg] : 0.0f;
          if constexpr (RADD) pok[j] = ok ? 1.0f : 0.0f;
        }
        f_g = GATH && seg.gV != nullptr;                             // uniform
        if (GATH && f_g) {
          const float* ub = seg.ptr + static_cast<long>(b) * seg.g_nsrc * seg.ld + clc;
#pragma unroll
          for (int i = 0; i < APT4; ++i) {
            const int r = min(vr0 + VSTEP * i, nvalid - 1);
            const long q = (row0 + r) >> gshift;
            rv[i] = *reinterpret_cast<const float4*>(ub + static_cast<long>(tidx[i]) * seg.ld);
            rv2[i] = *reinterpret_cast<const float4*>((tem[i] ? seg.gV0 : seg.gV) + q * seg.g_ldv + clc);
          }
        } else {
#pragma unroll
          for (int i = 0; i < APT4; ++i) {
            // rows beyond nvalid re-read the tile's last row; masked in the epilogue
            const int r = min(vr0 + VSTEP * i, nvalid - 1);
            rv[i] = *reinterpret_cast<const float4*>(abase + (r >> shift) * seg.ld + clc);
          }
        }
        if constexpr (RADD) {
          if (GATH && in.rseg.gV != nullptr) {
            const float* ub = in.rseg.ptr + static_cast<long>(b) * in.rseg.g_nsrc * in.rseg.ld + cbase + clc;
#pragma unroll
            for (int i = 0; i < APT4; ++i) {
              const int r = min(vr0 + VSTEP * i, nvalid - 1);
              const long q = (row0 + r) >> gshift;
              rrv[i] = *reinterpret_cast<const float4*>(ub + static_cast<long>(tidx[i]) * in.rseg.ld);
              rrv2[i] = *reinterpret_cast<const float4*>((tem[i] ? in.rseg.gV0 : in.rseg.gV) +
                                                         q * in.rseg.g_ldv + cbase + clc);
            }
          } else {
#pragma unroll
            for (int i = 0; i < APT4; ++i) {
              const int r = min(vr0 + VSTEP * i, nvalid - 1);
              rrv[i] = *reinterpret_cast<const float4*>(rd_b + r * in.rseg.ld + cbase + clc);
            }
          }
        }
      } else {
        const int ac = t % KC, ar0 = t / KC;
        const int cl = ks + ac;                                      // channel inside the segment
        f_cok = cl < seg.C;
        const int cc = f_cok ? cl : seg.C - 1;
        const int cg = cbase + cc;                                   // global input channel
        f_s = sc_b ? sc_b[cg] : 1.0f;
        f_h = sh_b ? sh_b[cg] : 0.0f;
        f_a = ad_b ? ad_b[cg] : 0.0f;
#pragma unroll
        for (int i = 0; i < APT; ++i) {
          const int r = min(ar0 + RSTEP * i, nvalid - 1);
          ra[i] = abase[(r >> shift) * seg.ld + cc];
        }
        if constexpr (RADD) {
#pragma unroll
          for (int i = 0; i < APT; ++i) {
            const int r = min(ar0 + RSTEP * i, nvalid - 1);
            rr[i] = rd_b[r * in.rseg.ld + cg];
          }
        }
      }
      if (!(single_chunk && w_loaded)) {
        const float* wbase = Wt + static_cast<long>(cbase + ks) * ldw + n0;
        const int nmax = ldw - n0 - 4;                               // last in-row float4 offset
#pragma unroll
        for (int i = 0; i < WPT4; ++i) {
          const int e = t + 256 * i;
          const int k = e / TN4, n4 = e - k * TN4;
          rwv[i] = *reinterpret_cast<const float4*>(wbase + min(k, f_kmax - 1) * ldw + min(4 * n4, nmax));
        }
      }
    };
    auto commit = [&]() {
      int t = tid;
      asm volatile("" : "+v"(t));
      if constexpr (VEC) {
        const int vc4 = t % C4, vr0 = t / C4;
#pragma unroll
        for (int i = 0; i < APT4; ++i) {
          float x[4] = {rv[i].x, rv[i].y, rv[i].z, rv[i].w};
          if constexpr (GATH) {
            if (f_g) {   // neighbour row + query row; empty ball: the query row alone (V0)
              const float v2[4] = {rv2[i].x, rv2[i].y, rv2[i].z, rv2[i].w};
#pragma unroll
              for (int j = 0; j < 4; ++j) x[j] = tem[i] ? v2[j] : x[j] + v2[j];
            }
          }
          float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if constexpr (RADD) {
            q[0] = rrv[i].x; q[1] = rrv[i].y; q[2] = rrv[i].z; q[3] = rrv[i].w;
            if constexpr (GATH) {
              if (in.rseg.gV != nullptr) {
                const float v2[4] = {rrv2[i].x, rrv2[i].y, rrv2[i].z, rrv2[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = tem[i] ? v2[j] : q[j] + v2[j];
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v = fmaxf(x[j], lo_pre);
            v = __builtin_fmaf(v, ps[j], ph[j]);
            v = fmaxf(v, lo_post) + pa[j];
            if constexpr (RADD) v = __builtin_fmaf(q[j], pok[j], v);
            // a padding column may hold anything (NaN x 0 is NaN): the channels beyond the segment are exactly 0
            As[4 * vc4 + j][vr0 + VSTEP * i] = (f_okm >> j & 1) ? v : 0.0f;
          }
        }
      } else {
        const int ac = t % KC, ar0 = t / KC;
        const float s = f_cok ? f_s : 0.0f, h = f_cok ? f_h : 0.0f, a = f_cok ? f_a : 0.0f;
        const float rok = f_cok ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < APT; ++i) {
          float v = fmaxf(ra[i], lo_pre);
          v = __builtin_fmaf(v, s, h);
          v = fmaxf(v, lo_post) + a;
          if constexpr (RADD) v = __builtin_fmaf(rr[i], rok, v);
          As[ac][ar0 + RSTEP * i] = v;
        }
      }
      if (!(single_chunk && w_loaded)) {
#pragma unroll
        for (int i = 0; i < WPT4; ++i) {
          const int e = t + 256 * i;
          const int k = e / TN4, n4 = e - k * TN4;
          const bool kok = k < f_kmax;
          float4 w = rwv[i];
          w.x = (kok && n0 + 4 * n4 + 0 < Cout) ? w.x : 0.0f;
          w.y = (kok && n0 + 4 * n4 + 1 < Cout) ? w.y : 0.0f;
          w.z = (kok && n0 + 4 * n4 + 2 < Cout) ? w.z : 0.0f;
          w.w = (kok && n0 + 4 * n4 + 3 < Cout) ? w.w : 0.0f;
          if (e < KC * TN4) *reinterpret_cast<float4*>(&Bs[k][4 * n4]) = w;
        }
        w_loaded = true;
      }
    };

    f32x16 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    int sg = 0, ks = 0, cbase = 0;
    fetch(0, 0, 0);
    while (true) {
      __syncthreads();                 // previous chunk's MFMAs (and epilogue reads of `red`) done
      commit();
      __syncthreads();
      const int segC = in.seg[sg].C;
      const int ksteps = (min(KC, segC - ks) + 1) >> 1;
      ks += KC;
      if (ks >= segC) {
        cbase += segC;
        ks = 0;
        ++sg;
      }
      const bool more = sg < in.n_seg;
      if (more) fetch(sg, ks, cbase);  // in flight during the MFMAs below
      for (int kk = (KS == 1 ? 0 : kq); kk < ksteps; kk += KS) {
        float a[RT], w[CT];
#pragma unroll
        for (int i = 0; i < RT; ++i) a[i] = As[2 * kk + hi][(wr * RT + i) * 32 + il];
#pragma unroll
        for (int j = 0; j < CT; ++j) w[j] = Bs[2 * kk + hi][(wc * CT + j) * 32 + il];
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = 0; j < CT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], w[j], acc[i][j], 0, 0, 0);
      }
      if (!more) break;
    }

    if constexpr (KS > 1) {
      // sum the KS partial products of every MFMA tile: waves kq > 0 park their accumulators in the (now idle) W stage,
      // waves kq = 0 add them in the order kq = 1, 2, ...; only those run the epilogue below
      static_assert(sizeof(float) * (KS - 1) * WR * WC * RT * CT * 16 * 64 <= sizeof(Bs), "K-split scratch");
      float* scr = &Bs[0][0];
      __syncthreads();                 // every wave has read its last operands
      if (kq > 0) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              scr[((((kq - 1) * WR * WC + wc * WR + wr) * RT * CT + i * CT + j) * 16 + r) * 64 + lane] = acc[i][j][r];
      }
      __syncthreads();
      if (kq == 0) {
#pragma unroll
        for (int q = 1; q < KS; ++q)
#pragma unroll
          for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < CT; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r)
                acc[i][j][r] += scr[((((q - 1) * WR * WC + wc * WR + wr) * RT * CT + i * CT + j) * 16 + r) * 64 + lane];
      }
    }
    [[maybe_unused]] const bool epi_wave = kq == 0;      // uniform per wave
    // ---- epilogue: C/D layout col = lane&31, row = (reg&3) + 8 (reg>>2) + 4 (lane>>5).
    // Full row tiles (the common case) store through ONE predicated region per 32-column tile:
    // per-element conditions would put every store in its own basic block, each opened by an
    // s_waitcnt vmcnt(0) that drains the previous store (stores count in vmcnt on gfx950).
    int il_e = il;
    asm volatile("" : "+v"(il_e));
    // weighted statistics (in.wrow0, see pdr_layer_in_t): rows below wrow0[b] do not count, the rest x wmul
    const int wlo = in.wrow0 ? min(max(in.wrow0[b] - tb * TM, 0), TM) : 0;   // uniform
    const bool rows_full = nvalid == TM && wlo == 0;   // uniform
    if constexpr (POOL) {
      // a 32-row MFMA tile holds 32 / K whole queries (K in {8, 16, 32}); for a fixed column a
      // query's K rows sit in registers {r : (r >> 2) / (K / 8) == g} of both lane halves
      const int K = pool.K;
      const int gsz = K >> 3;                 // 8-row register groups per query
      const int ksh = __builtin_ctz(K);
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int col = n0 + (wc * CT + j) * 32 + il_e;
        const bool colok = col < Cout;
        const int cc = colok ? col : 0;
        const float bv = bias_r[j];
        const float vs = pool.vscale ? pool.vscale[static_cast<long>(b) * Cout + cc] : 1.0f;
        const float vh = pool.vshift ? pool.vshift[static_cast<long>(b) * Cout + cc] : 0.0f;
        const float lo = pool.v_relu ? 0.0f : -__builtin_inff();
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const int rbase = (wr * RT + i) * 32;
          if (rbase >= nvalid) continue;        // uniform (tiles end on query boundaries)
          float val[16], sc[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rl = rbase + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const long p = row0 + rl;
            int cnt = K;
            if (pool.counts) {
              cnt = pool.counts[p >> ksh];
              cnt = cnt < 1 ? 1 : cnt;
            }
            const int kk = rl & (K - 1);
            sc[r] = kk < cnt ? acc[i][j][r] + bv : -1e9f;
            val[r] = fmaxf(__builtin_fmaf(pool.values[p * pool.ldv + cc], vs, vh), lo);
          }
          for (int g = 0; g < 4; g += gsz) {      // uniform trip count
            float m = -__builtin_inff();
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if ((r >> 2) >= g && (r >> 2) < g + gsz) m = fmaxf(m, sc[r]);
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float l = 0.0f, a = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if ((r >> 2) >= g && (r >> 2) < g + gsz) {
                const float w = expf(sc[r] - m);
                l += w;
                a = __builtin_fmaf(val[r], w, a);
              }
            l += __shfl_xor(l, 32, 64);
            a += __shfl_xor(a, 32, 64);
            if (hi == 0 && colok) {
              const long q = (row0 + rbase + 8 * g) >> ksh;
              pool.out[q * pool.ldo + col] = a / l;
            }
          }
        }
      }
      continue;   // next row tile
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      if constexpr (KS > 1) {
        if (!epi_wave) break;           // (K split: the other waves hold partial products only)
      }
      const int cl = (wc * CT + j) * 32 + il_e;
      const int col = n0 + cl;
      const bool colok = col < Cout;
      const float bv = bias_r[j];
      const bool relu_stat = col >= relu_col0;
      float s1 = 0.0f, s2 = 0.0f;
      float* ybase = Y + row0 * ldy + col;
      if (colok && in.oadd) {
        // per-query term of a split conv (one row of `oadd` per oadd_div positions)
        const int osh = __builtin_ctz(in.oadd_div);
        const float* ob = in.oadd + col;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rl = min((wr * RT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, nvalid - 1);
            const long oq = (row0 + rl) >> osh;
            acc[i][j][r] += ob[(in.oadd_rows ? static_cast<long>(in.oadd_rows[oq]) : oq) * in.oadd_ld];
          }
        }
      }
      if (colok) {
        if (rows_full) {
#pragma unroll
          for (int i = 0; i < RT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = (wr * RT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
              const float y = acc[i][j][r] + bv;
              ybase[rl * ldy] = y;
              const float f = relu_stat ? fmaxf(y, 0.0f) : y;
              s1 += f;
              s2 = __builtin_fmaf(f, f, s2);
            }
          }
        } else {
#pragma unroll
          for (int i = 0; i < RT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = (wr * RT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
              const float y = acc[i][j][r] + bv;
              if (rl < nvalid) {
                ybase[rl * ldy] = y;
                if (rl >= wlo) {
                  const float f = relu_stat ? fmaxf(y, 0.0f) : y;
                  s1 += f;
                  s2 = __builtin_fmaf(f, f, s2);
                }
              }
            }
          }
        }
      }
      if (partial) {
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (in.wrow0) {
          s1 *= in.wmul;
          s2 *= in.wmul;
        }
        if (hi == 0) {
          red[wr][cl][0] = s1;
          red[wr][cl][1] = s2;
        }
      }
    }
    if (partial) {
      __syncthreads();
      if (tid < TN && n0 + tid < Cout) {
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int w = 0; w < WR; ++w) {
          s1 += red[w][tid][0];
          s2 += red[w][tid][1];
        }
        // (row b partial_tpb + tb of `partial`, as the wave-specialised kernels: partial_tpb = 0 -> tiles per batch)
        const long prow = static_cast<long>(b) * (in.partial_tpb > 0 ? in.partial_tpb : tpb) + tb;
        float* o = partial + (prow * Cout + n0 + tid) * 2;
        o[0] = s1;
        o[1] = s2;
      }
    }
  }
}

// Layers with <= 4 input channels and no prologue -- the per-query / per-source coordinate tables of the split
// first convs, xyz . W (+ bias): three fmas per output and a pure write stream, not a job for 32 x 32 MFMA tiles
// (30 launches per step).  A thread owns 4 consecutive output columns of one row; accumulation order = the tile
// kernels' (bias first, then the channels in MFMA order), so the results are the same bits.
__global__ __launch_bounds__(256) void fused_layer_thin_kernel(const float* __restrict__ X, int ldx, int shift,
                                                               int Cin, const float* __restrict__ Wt, int ldw,
                                                               const float* __restrict__ bias, int Cout,
                                                               float* __restrict__ Y, int ldy, long P, int qshift) {
  // 256 threads = (256 >> qshift) rows x (1 << qshift) column quads; a thread keeps its quad's weights in registers
  // and walks kThinIters rows; a wave stores whole contiguous row pieces
  constexpr int kThinIters = 8;
  const int ql = 1 << qshift;
  const int cq = threadIdx.x & (ql - 1), rl = threadIdx.x >> qshift;
  const int c0 = 4 * (static_cast<int>(blockIdx.y) * ql + cq);
  if (c0 >= Cout) return;                             // (columns up to the 4-padded width are written)
  const int rpp = 256 >> qshift;
  float4 w[4];
  float b4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    w[k] = k < Cin ? *reinterpret_cast<const float4*>(Wt + static_cast<long>(k) * ldw + c0) : make_float4(0, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) b4[j] = (bias && c0 + j < Cout) ? bias[c0 + j] : 0.0f;
  const long r0 = static_cast<long>(blockIdx.x) * (rpp * kThinIters) + rl;
  // all eight row loads in flight before the first store (a load inside `if (row < P)` waits for itself AND -- stores
  // count in vmcnt on gfx9 -- for the previous trip's store: eight dependent round trips per workgroup)
  float4 xr[kThinIters];
#pragma unroll
  for (int it = 0; it < kThinIters; ++it) {
    const long row = r0 + static_cast<long>(it) * rpp;
    xr[it] = *reinterpret_cast<const float4*>(X + ((row < P ? row : P - 1) >> shift) * ldx);
  }
#pragma unroll
  for (int it = 0; it < kThinIters; ++it) {
    const long row = r0 + static_cast<long>(it) * rpp;
    if (row < P) {
      const float4 x = xr[it];
      const float xs[4] = {x.x, x.y, x.z, x.w};
      float acc[4] = {b4[0], b4[1], b4[2], b4[3]};
      // channel order 0, 2, 1, 3: the tile kernels' first MFMA of a channel quad multiplies the pair (0, 2), the
      // second (1, 3)
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = ((o & 1) << 1) | (o >> 1);
        if (k < Cin) {
          acc[0] = __builtin_fmaf(xs[k], w[k].x, acc[0]);
          acc[1] = __builtin_fmaf(xs[k], w[k].y, acc[1]);
          acc[2] = __builtin_fmaf(xs[k], w[k].z, acc[2]);
          acc[3] = __builtin_fmaf(xs[k], w[k].w, acc[3]);
        }
      }
      *reinterpret_cast<float4*>(Y + row * ldy + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
  }
}

using pdr::LayerSource;
using pdr::Tile;

// Tile selection: the id of a variant of pdr::kTiles (layer_tiles.h; its height and width are tile_tm / tile_tn
// there).  "Tall" shapes stack all four waves along the rows and give every wave the full output width (one column
// block => the input is read exactly once): used whenever Cout <= 160.  Wide outputs use 128 x 128 tiles (2 x 2
// waves) over a 2-D grid.
// narrow outputs: 128-row tiles staged in 32-channel chunks (ids 7, 8) instead of 256-row tiles in 16-channel
// chunks (ids 0, 1): a row of <= 32 channels is then fetched as ONE whole 128-byte line (the half-line fetches of
// the 16-channel chunks were re-read from HBM).  Option narrow_kc32 = 0: the 256-row tiles.
inline bool narrow_kc32() { return pdr::option(pdr::OPT_NARROW_KC32) != 0; }
inline int pick_tile(int rows_per_batch, int Cout) {
  if (narrow_kc32() && rows_per_batch >= 128 && Cout <= 32) return 7;
  if (narrow_kc32() && rows_per_batch >= 128 && Cout <= 64) return 8;
  if (rows_per_batch >= 256 && Cout <= 32) return 0;
  if (rows_per_batch >= 256 && Cout <= 64) return 1;
  if (rows_per_batch >= 128 && Cout <= 96) return 2;
  if (rows_per_batch >= 128 && Cout > 128 && Cout <= 160) return 3;
  // (64-row tiles for the deep levels, whose 128 x 128 tiling has fewer jobs than the 512 resident workgroups -- B = 32:
  // 16 k rows x 128 columns = 128 jobs -- measured 8.72-8.77 vs 8.75-8.77 ms per step in round 4: no gain, not taken)
  if (rows_per_batch >= 128) return 4;
  if (rows_per_batch >= 64) return 5;
  return 6;
}
}  // namespace

extern "C" int pdr_fused_layer_tile_rows(int rows_per_batch, int Cout) {
  if (rows_per_batch <= 0 || Cout <= 0) return 0;
  return pdr::tile_tm(pick_tile(rows_per_batch, Cout));
}

// which kernel instantiation pdr_fused_layer() launches (0..8: the index into pdr::kTiles, see pick_tile); lets
// profilers and bench.py attribute a launch to its kernel symbol
extern "C" int pdr_fused_layer_variant(int rows_per_batch, int Cout) {
  if (rows_per_batch <= 0 || Cout <= 0) return -1;
  return pick_tile(rows_per_batch, Cout);
}

// The dispatch decision of pdr_fused_layer: plan_layer() is the only place that decides or refuses; pdr_fused_layer
// launches what it names, pdr_fused_layer_plan reports it (profilers / bench.py attribute a call to the kernel
// symbol it launches without duplicating these rules), the pair and f16x3 entry points build on its `ws`.
namespace {
enum class Family {
  Thin,         // fused_layer_thin_kernel
  DeepSplitK,   // right-sized tiny layer, the waves split the K walk (`deep` = 6: 32 x 32 / 4 ways, 5: 64 x 32 / 2 ways)
  Deep,         // right-sized tiny layer (`deep` = 6: 32 x 128, 5: 64 x 64, 4: 128 x 64; 128-channel chunks)
  Ws,           // fused_layer_ws_kernel of the tile variant
  Uniform       // fused_layer_kernel of the tile variant
};

struct LayerPlan {
  Family family;
  int id, tm;     // tile variant (pdr::kTiles) and its rows
  LayerSource src;
  bool vec;       // float4 staging
  bool ws;        // the wave-specialised kernel of `id` carries this input (whatever `family` pdr_fused_layer takes)
  bool thin;      // the thin kernel could run this call (it does when there is no `partial` and no tile subset)
  long ntiles;
  int ncol;       // column blocks of the tile variant
  // right-sized launch of a tiny layer: 0 = none, else the tile variant whose launch it replaces (4, 5, 6); their
  // shapes are outside pdr::kTiles and named where pdr_fused_layer launches them
  int deep;
  int deep_tn;    // column-block width of the Deep / DeepSplitK launch (0: none)
};

bool deep_chunks() { return pdr::option(pdr::OPT_DEEP_CHUNKS) != 0; }

bool use_ws_kernels() { return pdr::option(pdr::OPT_FUSED_WS) != 0; }

// has_partial: the call collects statistics (the thin kernel has none).  Y may be null (pooled / planning callers).
int plan_layer(const pdr_layer_in_t* in, long P, int Cin, const float* Wt, int ldw, int Cout, const float* Y,
               int ldy, bool has_partial, LayerPlan* pl) {
  if (!in || !Wt || P < 0 || Cin <= 0 || Cout <= 0 || in->n_seg < 1 || in->n_seg > 4 || ldw < Cout ||
      (Y && ldy < Cout))
    return PDR_EINVAL;
  // the weight matrix is staged with 16-B loads: packed with a 4-float-aligned leading dimension
  if (ldw % 4 != 0 || reinterpret_cast<uintptr_t>(Wt) % 16 != 0) return PDR_EINVAL;
  int ctot = 0;
  for (int s = 0; s < in->n_seg; ++s) {
    if (!in->seg[s].ptr || in->seg[s].C <= 0 || in->seg[s].row_div < 1) return PDR_EINVAL;
    if (in->seg[s].row_div & (in->seg[s].row_div - 1)) return PDR_EUNSUPPORTED;  // power of two only
    ctot += in->seg[s].C;
  }
  if (ctot != Cin || in->rows_per_batch <= 0 || P % in->rows_per_batch != 0) return PDR_EINVAL;
  if (in->oadd && (in->oadd_div < 1 || (in->oadd_div & (in->oadd_div - 1)) || in->oadd_ld < Cout))
    return PDR_EINVAL;
  if (in->ss_ld != 0 && in->ss_ld < Cin) return PDR_EINVAL;
  const int id = pick_tile(in->rows_per_batch, Cout), tm = pdr::tile_tm(id);
  for (int sg = 0; sg < in->n_seg; ++sg) {
    // every tile must start on a multiple of the broadcast divisor
    const int d = in->seg[sg].row_div;
    if (in->rows_per_batch % d != 0 || (in->rows_per_batch > tm && tm % d != 0)) return PDR_EUNSUPPORTED;
  }
  const long nb = P / in->rows_per_batch;
  // rows of `partial` per batch element: at least its tiles (a smaller stride would fold tiles of two batch elements
  // into one row); weighted statistics come with a weight
  if (in->partial_tpb > 0 && in->partial_tpb < (in->rows_per_batch + tm - 1) / tm) return PDR_EINVAL;
  pl->id = id;
  pl->tm = tm;
  pl->ntiles = nb * ((in->rows_per_batch + tm - 1) / tm);
  pl->ncol = (Cout + pdr::tile_tn(id) - 1) / pdr::tile_tn(id);
  const LayerSource src = pdr::layer_source(*in);
  const bool gath = src.gath, radd = src.radd;
  // vector (float4) A staging needs every source 16-B aligned with a leading dimension that is a
  // multiple of 4 floats and rows padded to a multiple of 4 channels
  auto aligned = [](const float* p, int ld, int C) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0 && ld >= ((C + 3) & ~3);
  };
  bool vec = true;
  for (int sg = 0; sg < in->n_seg; ++sg) {
    const pdr_seg_t& g = in->seg[sg];
    vec = vec && aligned(g.ptr, g.ld, g.C);
    if (g.gV) {
      vec = vec && aligned(g.gV, g.g_ldv, g.C) && (!g.gV0 || aligned(g.gV0, g.g_ldv, g.C));
      if (g.row_div != 1 || g.g_nsrc <= 0) return PDR_EINVAL;
    }
  }
  if (radd) {
    vec = vec && in->n_seg == 1 && aligned(in->rseg.ptr, in->rseg.ld, Cin);
    if (in->rseg.gV)
      vec = vec && aligned(in->rseg.gV, in->rseg.g_ldv, Cin) &&
            (!in->rseg.gV0 || aligned(in->rseg.gV0, in->rseg.g_ldv, Cin));
  }
  if (gath) {
    // gathered sources exist only in the vector path; one shared index array, K a power of two that
    // divides the row tile so that a tile starts on a query boundary
    if (!vec || !in->gidx || in->gK <= 0 || (in->gK & (in->gK - 1)) || in->rows_per_batch % in->gK != 0 ||
        tm % in->gK != 0)
      return PDR_EUNSUPPORTED;
    for (int sg = 0; sg < in->n_seg; ++sg)
      if (in->seg[sg].gV && in->gcnt && !in->seg[sg].gV0) return PDR_EINVAL;
  }
  pl->src = src;
  pl->vec = vec;
  // steady-state layers (float4-staged sources): wave-specialised kernel where an instantiation exists
  pl->ws = use_ws_kernels() && vec && pdr::fused_layer_ws_supported(id, src, *in, Cin);
  // TINY layers (round 5; option deep_chunks = 0: never).  The per-point layers of the deep levels are launches of a few
  // dozen workgroups, each a serial walk over the input channels: their time is (chunks) x (load latency) + (MFMAs per
  // wave) x 64 cycles on a chip that is half to seven eighths empty.  Where every workgroup of the launch is resident
  // at once they run on the uniform-wave kernel with 128-channel chunks (a quarter of the round trips) and, for the
  // 64- / 128-row tiles, half-width tiles (twice the workgroups, half the MFMAs per wave):
  //   32-row tiles (batch elements of < 64 rows: 16 points per cloud), <= 256 jobs          -> 32 x 128, 128-channel chunks
  //   64-row tiles (64 .. 127 rows: 64 points), plain sources, <= 512 jobs of 64 x 64       -> 64 x 64,  128-channel chunks
  //   128-row tiles (128 .. 511 rows at B = 32: 256 points), plain sources, <= 128 jobs     -> 128 x 64, 128-channel chunks
  // (128 for the last: beyond that every CU already holds a workgroup and the matrix pipes are what the launch waits
  // for -- bound at 256 / 512: step 5.85 / 6.06 ms against 5.79 at 128.)  Measured alone on the
  // chip, B = 32: 16 rows 512 -> 512 35.8 -> 27.6 us, 64 rows 256 -> 256 16.6 -> 14.0, 256 rows 128 -> 128 16.2 -> 12.5,
  // 256 -> 256 26.7 -> 22.0, 512 rows 128 -> 128 17.2 -> 13.6; step 6.03 -> 5.87 ms (profiles/r5_tiny_layers_ab.txt).
  pl->deep = 0;
  if (deep_chunks() && Cin > 64 && !in->tile_list) {
    if (id == 6 && pl->ntiles * pl->ncol <= pdr::option(pdr::OPT_DEEP_JOBS32)) pl->deep = 6;
    else if (id == 5 && vec && !gath && pl->ntiles * ((Cout + 63) / 64) <= pdr::option(pdr::OPT_DEEP_JOBS64)) pl->deep = 5;
    else if (id == 4 && vec && !gath && pl->ntiles * pl->ncol <= 128) pl->deep = 4;
  }
  // ... and, for plain sources, the waves of the first two split the K walk (fused_layer_kernel's KS): 4 ways on
  // 32 x 32 tiles for the 32-row family (16 rows per cloud: a wave's chain of Cin / 2 MFMAs was most of the launch),
  // 2 ways on 64 x 32 tiles for the 64-row family; not for the 128-row family (128 x 32 tiles, measured: 256 rows
  // 256 -> 256 22.0 -> 54.3 us -- four times the workgroups re-reading the same 128 input rows).  Option deep_ks = 0:
  // no split (A/B).
  const bool split_k = (pl->deep == 6 || pl->deep == 5) && pdr::option(pdr::OPT_DEEP_KS) != 0 && vec && !gath;
  pl->deep_tn = !pl->deep ? 0 : split_k ? 32 : pl->deep == 6 ? 128 : 64;
  // <= 4 input channels, nothing to apply on the way in, 16-byte rows on both sides: the thin kernel (it collects no
  // statistics: taken only without `partial`)
  pl->thin = vec && Cin <= 4 && in->n_seg == 1 && !gath && !radd && !in->scale && !in->shift && !in->add &&
             !in->pre_relu && !in->post_relu && !in->oadd && Y && ldy % 4 == 0 &&
             reinterpret_cast<uintptr_t>(Y) % 16 == 0 && ldw >= ((Cout + 3) & ~3) && ldy >= ((Cout + 3) & ~3) &&
             P < (1L << 31);
  // what only the wave-specialised kernels carry: kNN-form gathered sources (the caller materialises instead) and a
  // tile subset (128-row tiles)
  if (src.knn_marked && !pl->ws) return PDR_EUNSUPPORTED;
  if (in->tile_list && (!in->n_tiles || !pl->ws || tm != 128)) return PDR_EUNSUPPORTED;
  pl->family = pl->thin && !has_partial && !in->tile_list ? Family::Thin
               : split_k                                   ? Family::DeepSplitK
               : pl->deep                                  ? Family::Deep
               : pl->ws                                    ? Family::Ws
                                                           : Family::Uniform;
  return PDR_OK;
}

// everything of a uniform-wave launch but the grid and the template arguments
struct LayerArgs {
  hipStream_t s; const pdr_layer_in_t& in; int Cin; const float* Wt; int ldw; const float* bias; int Cout;
  float* Y; int ldy; float* partial; int relu_col0, n_row_tiles; PoolArgs pool;
};

template <class T, bool RADD, bool VEC, bool GATH, bool POOL = false, int KS = 1>
void launch_k(dim3 grid, const LayerArgs& a) {
  hipLaunchKernelGGL((fused_layer_kernel<T::RT, T::CT, T::WR, T::WC, T::KC, RADD, VEC, GATH, POOL, KS>), grid,
                     dim3(256), 0, a.s, a.in, a.Cin, a.Wt, a.ldw, a.bias, a.Cout, a.Y, a.ldy, a.partial, a.relu_col0,
                     a.n_row_tiles, a.pool);
}

// residual x (gathered / float4-staged / scalar-staged sources)
template <class T>
void launch_form(dim3 grid, const LayerArgs& a, const LayerPlan& pl) {
  if (pl.src.radd) {
    if (pl.src.gath) launch_k<T, true, true, true>(grid, a);
    else if (pl.vec) launch_k<T, true, true, false>(grid, a);
    else launch_k<T, true, false, false>(grid, a);
  } else {
    if (pl.src.gath) launch_k<T, false, true, true>(grid, a);
    else if (pl.vec) launch_k<T, false, true, false>(grid, a);
    else launch_k<T, false, false, false>(grid, a);
  }
}

// float4-staged plain sources (the right-sized tiny layers), the K walk split KS ways
template <class T, int KS = 1>
void launch_plain(dim3 grid, const LayerArgs& a, bool radd) {
  if (radd) launch_k<T, true, true, false, false, KS>(grid, a);
  else launch_k<T, false, true, false, false, KS>(grid, a);
}

// grid of the uniform-wave kernel: enough workgroups to fill 256 CUs a few times over; the rest is covered by the
// grid stride
dim3 uniform_grid(long ntiles, int ncol) {
  const long cap = (256L * 6 + ncol - 1) / ncol;
  return dim3(static_cast<unsigned>(ntiles > cap ? cap : ntiles), static_cast<unsigned>(ncol));
}
}  // namespace

// out[0..6] = {wave-specialised kernel?, tile variant id, residual source?, gathered source (0 no / 1 ball / 2 kNN),
// float4 staging?, split-f16 arithmetic?, thin kernel when called without `partial`?} of the launch
// pdr_fused_layer would make for these arguments: the plan of a call WITH `partial`, and whether the thin kernel
// would replace it without.
extern "C" int pdr_fused_layer_plan(const pdr_layer_in_t* in, long P, int Cin, const float* Wt, int ldw, int Cout,
                                    const float* Y, int ldy, int* out) {
  if (!out) return PDR_EINVAL;
  LayerPlan pl;
  const int rc = plan_layer(in, P, Cin, Wt, ldw, Cout, Y, ldy, true, &pl);
  if (rc != PDR_OK) return rc;
  out[0] = pl.family == Family::Ws;
  out[1] = pl.id;
  out[2] = pl.src.radd;
  out[3] = pl.src.gath ? (pl.src.knn_marked ? 2 : 1) : 0;
  out[4] = pl.vec;
  out[5] = 0;
  out[6] = pl.thin;
  out[7] = pl.deep ? 128 : 0;   // channels per chunk of a right-sized tiny launch (plan_layer), else 0
  return PDR_OK;
}

// Y (P, Cout; leading dim ldy) = prologue(X) . Wt + bias.  partial: NULL or
// (B * tiles_per_batch, Cout, 2) floats receiving per-tile sum / sum of squares of y
// (columns >= relu_col0: of relu(y)).
extern "C" int pdr_fused_layer(const pdr_layer_in_t* in, long P, int Cin, const float* Wt, int ldw,
                               const float* bias, int Cout, float* Y, int ldy, float* partial,
                               int relu_col0, pdr_stream_t stream) {
  if (!Y) return PDR_EINVAL;
  LayerPlan pl;
  const int prc = plan_layer(in, P, Cin, Wt, ldw, Cout, Y, ldy, partial != nullptr, &pl);
  if (prc != PDR_OK) return prc;
  if (P == 0) return PDR_OK;
  hipStream_t s = pdr::as_stream(stream);
  const int nt = static_cast<int>(pl.ntiles);
  const LayerArgs a{s, *in, Cin, Wt, ldw, bias, Cout, Y, ldy, partial, relu_col0, nt, PoolArgs()};
  // the right-sized launches: one workgroup per job
  auto deep_grid = [&] {
    return dim3(static_cast<unsigned>(pl.ntiles), static_cast<unsigned>((Cout + pl.deep_tn - 1) / pl.deep_tn));
  };
  switch (pl.family) {
    case Family::Thin: {
      const int c4n = (Cout + 3) / 4;
      int qshift = 3;                                    // 8 .. 64 column quads per row of threads
      while (qshift < 6 && (1 << qshift) < c4n) ++qshift;
      const int ql = 1 << qshift, rows_per_block = (256 >> qshift) * 8;
      const dim3 tgrid(static_cast<unsigned>((P + rows_per_block - 1) / rows_per_block),
                       static_cast<unsigned>((c4n + ql - 1) / ql));
      hipLaunchKernelGGL(fused_layer_thin_kernel, tgrid, dim3(256), 0, s, in->seg[0].ptr, in->seg[0].ld,
                         __builtin_ctz(in->seg[0].row_div), Cin, Wt, ldw, bias, Cout, Y, ldy, P, qshift);
      break;
    }
    case Family::DeepSplitK:
      if (pl.deep == 6) launch_plain<Tile<1, 1, 1, 1, 128>, 4>(deep_grid(), a, pl.src.radd);   // 32 x 32, 4 ways
      else launch_plain<Tile<1, 1, 2, 1, 128>, 2>(deep_grid(), a, pl.src.radd);                // 64 x 32, 2 ways
      break;
    case Family::Deep:
      if (pl.deep == 6) launch_form<Tile<1, 1, 1, 4, 128>>(uniform_grid(pl.ntiles, pl.ncol), a, pl);   // 32 x 128
      else if (pl.deep == 5) launch_plain<Tile<1, 1, 2, 2, 128>>(deep_grid(), a, pl.src.radd);           // 64 x 64
      else launch_plain<Tile<2, 1, 2, 2, 128>>(deep_grid(), a, pl.src.radd);                             // 128 x 64
      break;
    case Family::Ws:
      pdr::launch_fused_layer_ws(pl.id, pl.src, *in, Cin, Wt, ldw, bias, Cout, Y, ldy, partial, relu_col0, nt, pl.ncol,
                                 s);
      break;
    case Family::Uniform:
      pdr::with_tile(pl.id, [&](auto t) { launch_form<decltype(t)>(uniform_grid(pl.ntiles, pl.ncol), a, pl); });
      break;
  }
  return pdr::check_launch();
}

// The same layer over TWO row sets in ONE launch (round 6): `in` / Y / partial = the tile subset of a deduplicated block's
// per-neighbour rows (pdr_layer_in_t.tile_list; plain or ball-gathered sources, no residual), `in2` / Y2 / partial2 = its
// per-QUERY rows (plain sources, weighted statistics).  Replaces two dependent launches of a block's launch chain by
// one; the results are those of the two pdr_fused_layer calls, bit for bit (same tiles, same kernels' arithmetic).
// PDR_EUNSUPPORTED when the pair has no wave-specialised 128-row instantiation: the caller launches them one by one.
extern "C" int pdr_fused_layer_pair(const pdr_layer_in_t* in, long P, const pdr_layer_in_t* in2, long P2, int Cin,
                                    const float* Wt, int ldw, const float* bias, int Cout, float* Y, int ldy,
                                    float* Y2, int ldy2, float* partial, float* partial2, int relu_col0,
                                    pdr_stream_t stream) {
  if (!Y || !Y2 || !in || !in2) return PDR_EINVAL;
  LayerPlan pl, pl2;
  int rc = plan_layer(in, P, Cin, Wt, ldw, Cout, Y, ldy, partial != nullptr, &pl);
  if (rc != PDR_OK) return rc;
  rc = plan_layer(in2, P2, Cin, Wt, ldw, Cout, Y2, ldy2, partial2 != nullptr, &pl2);
  if (rc != PDR_OK) return rc;
  if (P == 0 || P2 == 0) return PDR_EUNSUPPORTED;
  if ((partial == nullptr) != (partial2 == nullptr)) return PDR_EINVAL;
  // the first problem decides the tile shape: a listed launch of 128-row tiles; the second runs on the same tiles
  // (its batch elements may be shorter than a tile: partial tiles, one row of `partial2` per 128 rows)
  if (!in->tile_list || !pl.ws || !pdr::tile_has_pair(pl.id) || !pl.vec || !pl2.vec || pl.src.radd || pl2.src.radd ||
      pl2.src.gath || pl.src.knn_marked || in2->tile_list)
    return PDR_EUNSUPPORTED;
  const int tpb2 = (in2->rows_per_batch + pl.tm - 1) / pl.tm;
  if (in2->partial_tpb > 0 && in2->partial_tpb < tpb2) return PDR_EINVAL;
  for (int sg = 0; sg < in2->n_seg; ++sg)
    if (in2->seg[sg].row_div != 1) return PDR_EUNSUPPORTED;
  // the second problem on the FIRST's tile variant (pl2 is its plan on a variant of its own), without an index array
  if (in2->gidx || !pdr::fused_layer_ws_supported(pl.id, pl2.src, *in2, Cin)) return PDR_EUNSUPPORTED;
  pdr::WsTwin tw;
  tw.in[1] = *in2;
  tw.Y[1] = Y2;
  tw.partial[1] = partial2;
  tw.ldy[1] = ldy2;
  tw.n_row_tiles[1] = static_cast<int>((P2 / in2->rows_per_batch) * tpb2);
  tw.gx = 0;
  pdr::launch_fused_layer_ws_pair(pl.id, pl.src.gath, *in, Cin, Wt, ldw, bias, Cout, Y, ldy, partial, relu_col0,
                                  static_cast<int>(pl.ntiles), pl.ncol, tw, pdr::as_stream(stream));
  return pdr::check_launch();
}

// pdr_fused_layer with SPLIT-f16 arithmetic (opt-in): both GEMM operands are split into f16 hi + lo parts and the
// product is accumulated as xh wh + xh wl + xl wh on v_mfma_f32_32x32x16_f16 with fp32 accumulation (~22 mantissa
// bits kept).  Wp = weight image of pdr-side packing (see include/pdr_hip.h), nchunks = K-chunks per column block.
// Only the wave-specialised tile variants of pdr::tile_has_split carry this mode: PDR_EUNSUPPORTED otherwise (callers
// fall back to the exact fp32 entry point).
extern "C" int pdr_fused_layer_f16x3(const pdr_layer_in_t* in, long P, int Cin, const void* Wp, int nchunks,
                                     const float* bias, int Cout, float* Y, int ldy, float* partial,
                                     int relu_col0, pdr_stream_t stream) {
  if (!Y || !Wp || nchunks <= 0 || reinterpret_cast<uintptr_t>(Wp) % 16 != 0) return PDR_EINVAL;
  LayerPlan pl;
  // (the fp32 weight arguments of the plan are placeholders: alignment-clean dummies)
  const int prc = plan_layer(in, P, Cin, reinterpret_cast<const float*>(Wp), (Cout + 3) & ~3, Cout, Y, ldy,
                             partial != nullptr, &pl);
  if (prc != PDR_OK) return prc;
  if (P == 0) return PDR_OK;
  if (!pl.ws || !pdr::tile_has_split(pl.id)) return PDR_EUNSUPPORTED;
  int nch = 0;
  for (int s = 0; s < in->n_seg; ++s) nch += (in->seg[s].C + 31) / 32;
  if (nch != nchunks) return PDR_EINVAL;   // the image was packed for another segment structure
  pdr::launch_fused_layer_ws(pl.id, pl.src, *in, Cin, reinterpret_cast<const float*>(Wp), nchunks, bias, Cout, Y, ldy,
                             partial, relu_col0, static_cast<int>(pl.ntiles), pl.ncol, pdr::as_stream(stream), true);
  return pdr::check_launch();
}

// scores = prologue(X) . Wt + bias are consumed by the POOL epilogue:
//   out[q, :] = sum_k softmax_k(mask(scores))[k, :] * act(values[q K + k, :] * vscale + vshift)
// K in {8, 16, 32}; Cout = D (channels of scores, values and out).
namespace {
// pooled launch that also writes the pooled rows of the skipped tiles' queries (pdr_layer_in_t.patch_values): the
// kernel reads patch_values / writes `out` in 16-byte pieces of 4 channels and reads patch_w[q] for every query
bool pool_patch_args_ok(const pdr_layer_in_t& in, int D, const float* out, int ldo) {
  if (!in.patch_values) return true;
  return in.patch_w != nullptr && in.patch_ld >= D && D % 4 == 0 && in.patch_ld % 4 == 0 && ldo % 4 == 0 &&
         reinterpret_cast<uintptr_t>(in.patch_values) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
}

// What the two pooled entry points share: validation of everything but the weights (`weights_ok`: the caller's own
// check of its weight arguments, part of the first PDR_EINVAL), the tile and the grid arithmetic.  nch = 32-channel
// chunks of the segments (the packed weight image's structure).
struct PoolPlan {
  int id, tm, ncol, nch;
  long ntiles;
  bool vec;   // float4 staging possible (every pooled kernel needs it; refused after the EINVAL checks)
};
int plan_pool(const pdr_layer_in_t* in, long P, int Cin, bool weights_ok, int D, const float* values, int ldv, int K,
              const float* out, int ldo, PoolPlan* pp) {
  if (!in || !weights_ok || !values || !out || P <= 0 || Cin <= 0 || D <= 0 || in->n_seg < 1 || in->n_seg > 4 ||
      ldv < D || ldo < D)
    return PDR_EINVAL;
  if (!pool_patch_args_ok(*in, D, out, ldo)) return PDR_EINVAL;
  if (!(K == 8 || K == 16 || K == 32)) return PDR_EUNSUPPORTED;
  if (in->rseg.ptr || in->oadd) return PDR_EUNSUPPORTED;
  int ctot = 0;
  pp->nch = 0;
  pp->vec = true;
  for (int s = 0; s < in->n_seg; ++s) {
    const pdr_seg_t& g = in->seg[s];
    if (!g.ptr || g.C <= 0 || g.row_div != 1 || g.gV) return PDR_EUNSUPPORTED;
    pp->vec = pp->vec && reinterpret_cast<uintptr_t>(g.ptr) % 16 == 0 && g.ld % 4 == 0 && g.ld >= ((g.C + 3) & ~3);
    ctot += g.C;
    pp->nch += (g.C + 31) / 32;
  }
  if (ctot != Cin || in->rows_per_batch <= 0 || P % in->rows_per_batch != 0 || in->rows_per_batch % 32 != 0)
    return PDR_EINVAL;
  pp->id = pick_tile(in->rows_per_batch, D);
  pp->tm = pdr::tile_tm(pp->id);
  pp->ntiles = P / in->rows_per_batch * ((in->rows_per_batch + pp->tm - 1) / pp->tm);
  pp->ncol = (D + pdr::tile_tn(pp->id) - 1) / pdr::tile_tn(pp->id);
  return PDR_OK;
}

// The dispatch decision of the two pooled entry points: decide_pool() is the only place that decides or refuses;
// pdr_fused_layer_pool / pdr_fused_layer_pool_f16x3 launch what it names, pdr_fused_layer_pool_plan reports it.
// W / ldw_or_nchunks: Wt and ldw of the exact entry point, Wp and nchunks of the split one.
struct PoolDecision {
  PoolPlan pp;
  bool ws;            // fused_layer_ws_kernel (else fused_layer_kernel<.., POOL = true>)
  LayerSource src;
};
int decide_pool(const pdr_layer_in_t* in, long P, int Cin, const void* W, int ldw_or_nchunks, int D,
                const float* values, int ldv, int K, const float* out, int ldo, bool split, PoolDecision* d) {
  const bool w16 = W && reinterpret_cast<uintptr_t>(W) % 16 == 0;
  const bool weights_ok = split ? w16 && ldw_or_nchunks > 0 : w16 && ldw_or_nchunks >= D && ldw_or_nchunks % 4 == 0;
  PoolPlan& pp = d->pp;
  const int rc = plan_pool(in, P, Cin, weights_ok, D, values, ldv, K, out, ldo, &pp);
  if (rc != PDR_OK) return rc;
  if (split) {
    if (pp.nch != ldw_or_nchunks) return PDR_EINVAL;   // the image was packed for another segment structure
    if (!pp.vec || !use_ws_kernels()) return PDR_EUNSUPPORTED;
    if (!pdr::tile_has_split(pp.id) || in->rows_per_batch % pp.tm != 0) return PDR_EUNSUPPORTED;
  } else if (!pp.vec) {
    return PDR_EUNSUPPORTED;
  }
  if (in->tile_list && (!in->n_tiles || pp.tm != 128)) return PDR_EUNSUPPORTED;
  d->src = pdr::layer_source(*in);
  // wave-specialised kernels carry the pooled epilogue for the tile shapes whose rows tile whole queries
  d->ws = use_ws_kernels() && in->rows_per_batch % pp.tm == 0 && pdr::fused_layer_ws_supported(pp.id, d->src, *in, Cin);
  if (split && !d->ws) return PDR_EUNSUPPORTED;
  // tile subsets / row maps / patched rows: wave-specialised kernels only
  if (!d->ws && (in->tile_list || in->out_rows || in->patch_values)) return PDR_EUNSUPPORTED;
  return PDR_OK;
}
}  // namespace

// plan[0..7] = {wave-specialised kernel?, tile variant id, split-f16 arithmetic?, row tiles, column blocks, tile
// subset?, row map?, patched rows?} of the launch the matching pooled entry point would make, and its return code.
extern "C" int pdr_fused_layer_pool_plan(const pdr_layer_in_t* in, long P, int Cin, const void* W, int ldw_or_nchunks,
                                         int D, const float* values, int ldv, int K, const float* out, int ldo,
                                         int split, int* plan) {
  if (!plan) return PDR_EINVAL;
  PoolDecision d;
  const int rc = decide_pool(in, P, Cin, W, ldw_or_nchunks, D, values, ldv, K, out, ldo, split != 0, &d);
  if (rc != PDR_OK) return rc;
  plan[0] = d.ws;
  plan[1] = d.pp.id;
  plan[2] = split != 0;
  plan[3] = static_cast<int>(d.pp.ntiles);
  plan[4] = d.pp.ncol;
  plan[5] = in->tile_list != nullptr;
  plan[6] = in->out_rows != nullptr;
  plan[7] = in->patch_values != nullptr;
  return PDR_OK;
}

// pdr_fused_layer_pool with the score conv on split-f16 arithmetic (packed weight image as pdr_fused_layer_f16x3);
// the wave-specialised tiles of pdr::tile_has_split only: PDR_EUNSUPPORTED otherwise (the caller uses the exact entry
// point).
extern "C" int pdr_fused_layer_pool_f16x3(const pdr_layer_in_t* in, long P, int Cin, const void* Wp, int nchunks,
                                          const float* bias, int D, const float* values, int ldv,
                                          const float* vscale, const float* vshift, int v_relu,
                                          const int* counts, int K, float* out, int ldo, pdr_stream_t stream) {
  PoolDecision d;
  const int rc = decide_pool(in, P, Cin, Wp, nchunks, D, values, ldv, K, out, ldo, true, &d);
  if (rc != PDR_OK) return rc;
  const PoolArgs pa{values, vscale, vshift, counts, out, ldv, ldo, K, v_relu};
  pdr::launch_fused_layer_ws(d.pp.id, d.src, *in, Cin, reinterpret_cast<const float*>(Wp), nchunks, bias, D, nullptr, 0,
                             nullptr, D, static_cast<int>(d.pp.ntiles), d.pp.ncol, pdr::as_stream(stream), true, &pa);
  return pdr::check_launch();
}

extern "C" int pdr_fused_layer_pool(const pdr_layer_in_t* in, long P, int Cin, const float* Wt, int ldw,
                                    const float* bias, int D, const float* values, int ldv,
                                    const float* vscale, const float* vshift, int v_relu,
                                    const int* counts, int K, float* out, int ldo,
                                    pdr_stream_t stream) {
  PoolDecision d;
  const int rc = decide_pool(in, P, Cin, Wt, ldw, D, values, ldv, K, out, ldo, false, &d);
  if (rc != PDR_OK) return rc;
  const PoolPlan& pp = d.pp;
  hipStream_t s = pdr::as_stream(stream);
  const PoolArgs pa{values, vscale, vshift, counts, out, ldv, ldo, K, v_relu};
  const int nt = static_cast<int>(pp.ntiles);
  if (d.ws) {
    pdr::launch_fused_layer_ws(pp.id, d.src, *in, Cin, Wt, ldw, bias, D, nullptr, 0, nullptr, D, nt, pp.ncol, s, false,
                               &pa);
    return pdr::check_launch();
  }
  const LayerArgs a{s, *in, Cin, Wt, ldw, bias, D, nullptr, 0, nullptr, D, nt, pa};
  pdr::with_tile(pp.id, [&](auto t) { launch_k<decltype(t), false, true, false, true>(uniform_grid(pp.ntiles, pp.ncol), a); });
  return pdr::check_launch();
}
