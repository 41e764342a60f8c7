// layer_tiles.h -- the tile variants of the layer kernels (fused_layer.hip, fused_layer_ws.hip): THE table, what is
// derived from it, and the host-side interface between the two translation units.
//
// A variant is <RT, CT, WR, WC, KC>: wave (wr, wc) of WR x WC consumer waves owns RT x CT MFMA tiles of 32 x 32, the K
// walk is staged in chunks of KC channels; the workgroup tile is TM x TN = (WR RT 32) x (WC CT 32).  pick_tile()
// (fused_layer.hip) chooses the id; everything else about a variant is read here.  Adding or changing a variant is an
// edit of kTiles (and of the predicates below when it has no wave-specialised / split-f16 form).  tools/ and tests/
// keep Python copies of the row counts (they cannot include this file): tools/kernel_roofline.py:_VARIANT,
// tools/lab/ws_trace.py, tests/layer_cases.py:TILE_ROWS.
#pragma once
#include "pdr_common.h"

namespace pdr {

struct TileShape {
  int rt, ct, wr, wc, kc;
  constexpr int tm() const { return wr * rt * 32; }
  constexpr int tn() const { return wc * ct * 32; }
};

constexpr TileShape kTiles[] = {
    {2, 1, 4, 1, 16},   // 0: 256 x 32   narrow outputs, 16-channel chunks (option narrow_kc32 = 0)
    {2, 2, 4, 1, 16},   // 1: 256 x 64
    {1, 3, 4, 1, 32},   // 2: 128 x 96
    {1, 5, 4, 1, 32},   // 3: 128 x 160  80 accumulators: over the 128-register budget of the wave-specialised kernel
    {2, 2, 2, 2, 32},   // 4: 128 x 128  2 x 2 waves, 2-D grid
    {1, 2, 2, 2, 32},   // 5: 64 x 128
    {1, 1, 1, 4, 32},   // 6: 32 x 128
    {1, 1, 4, 1, 32},   // 7: 128 x 32   narrow outputs, whole 128-byte lines per row (the default)
    {1, 2, 4, 1, 32},   // 8: 128 x 64
};
constexpr int kNumTiles = static_cast<int>(sizeof(kTiles) / sizeof(kTiles[0]));

constexpr int tile_tm(int id) { return kTiles[id].tm(); }
constexpr int tile_tn(int id) { return kTiles[id].tn(); }
// fused_layer_ws_kernel is instantiated for every variant but the 128 x 160 and the 32-row one
constexpr bool tile_has_ws(int id) { return id != 3 && id != 6; }
// ... with split-f16 arithmetic for the 128-column variants of 2 x 2 waves and the 64-column one
constexpr bool tile_has_split(int id) { return id == 4 || id == 5 || id == 8; }
// ... as a paired launch (pdr::WsTwin) for its 128-row variants: 2, 4, 7, 8
constexpr bool tile_has_pair(int id) { return tile_has_ws(id) && tile_tm(id) == 128; }

// compile-time form of a shape: what the launch sites hand to the kernel templates.  ID = -1: a shape outside the
// table (the right-sized tiny-layer launches of plan_layer).
template <int RT_, int CT_, int WR_, int WC_, int KC_, int ID_ = -1>
struct Tile {
  static constexpr int RT = RT_, CT = CT_, WR = WR_, WC = WC_, KC = KC_, id = ID_;
};
template <int ID>
using TableTile = Tile<kTiles[ID].rt, kTiles[ID].ct, kTiles[ID].wr, kTiles[ID].wc, kTiles[ID].kc, ID>;

// runtime id -> f(TableTile<id>{}); ids come from pick_tile()
template <class F>
inline void with_tile(int id, F&& f) {
  static_assert(kNumTiles == 9, "one case per variant");
  switch (id) {
    case 0: f(TableTile<0>{}); break;
    case 1: f(TableTile<1>{}); break;
    case 2: f(TableTile<2>{}); break;
    case 3: f(TableTile<3>{}); break;
    case 4: f(TableTile<4>{}); break;
    case 5: f(TableTile<5>{}); break;
    case 6: f(TableTile<6>{}); break;
    case 7: f(TableTile<7>{}); break;
    case 8: f(TableTile<8>{}); break;
    default: break;
  }
}

// What the sources of a call are, read off pdr_layer_in_t in ONE place.
//   knn / knn_res  decide the kernel form (GATH = 2 of fused_layer_ws_kernel) and what fused_layer_ws_supported asks
//                  of the kNN arrays: a main segment / the gathered residual carries g_r1.
//   knn_marked     the wider mark plan_layer refuses and reports by: g_r1 OR g_r2 on any main segment or on a gathered
//                  residual.  The two differ on malformed input only (g_r2 without g_r1): such a call runs the ball /
//                  plain form of the wave-specialised kernel, is refused where that kernel is not taken, and
//                  pdr_fused_layer_plan reports it as kNN-form when gathered (pinned by tests/layer_cases.py).
struct LayerSource {
  bool radd, gath, knn, knn_res, knn_marked;
};
inline LayerSource layer_source(const pdr_layer_in_t& in) {
  LayerSource s{in.rseg.ptr != nullptr, false, false, in.rseg.gV && in.rseg.g_r1,
                in.rseg.gV && (in.rseg.g_r1 || in.rseg.g_r2)};
  s.gath = s.radd && in.rseg.gV;
  for (int sg = 0; sg < in.n_seg; ++sg) {
    const pdr_seg_t& g = in.seg[sg];
    s.gath = s.gath || g.gV;
    s.knn = s.knn || g.g_r1;
    s.knn_marked = s.knn_marked || g.g_r1 || g.g_r2;
  }
  return s;
}

// fused_layer_ws.hip.  Whether the wave-specialised kernel of tile variant `id` carries this input (false for the
// variants without an instantiation).  The two launchers below size the persistent grid and launch; the CALLER has
// asked fused_layer_ws_supported (plan_layer, or the pooled entry points themselves) and, for `split` (f16x3
// arithmetic: Wt = packed weight image, ldw = chunks per column block), tile_has_split(id).
bool fused_layer_ws_supported(int id, const LayerSource& src, const pdr_layer_in_t& in, int Cin);
void launch_fused_layer_ws(int id, const LayerSource& src, const pdr_layer_in_t& in, int Cin, const float* Wt, int ldw,
                           const float* bias, int Cout, float* Y, int ldy, float* partial, int relu_col0,
                           int n_row_tiles, int ncol, hipStream_t s, bool split = false,
                           const PoolArgs* pool = nullptr);
// one launch for (in, Y, partial) and (twin.in[1], twin.Y[1], twin.partial[1]): plain or ball-gathered sources without
// a residual in the first problem, plain sources in the second; tile_has_pair(id)
void launch_fused_layer_ws_pair(int id, bool gath, const pdr_layer_in_t& in, int Cin, const float* Wt, int ldw,
                                const float* bias, int Cout, float* Y, int ldy, float* partial, int relu_col0,
                                int n_row_tiles, int ncol, WsTwin twin, hipStream_t s);

}  // namespace pdr
