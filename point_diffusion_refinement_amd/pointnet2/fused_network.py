"""Fused, channel-last execution of the cached-condition reverse step.

`FusedCloudConditionNet(net)` wraps a `PointNet2CloudCondition` (same parameters, no
copies except transposed / concatenated GEMM operands) and evaluates
    eps = net(x_t, condition, ts, label, use_retained_condition_feature=True)
for every step AFTER the first of a batch, i.e. with the condition branch retained,
through the fused kernels of libpdr_hip.so:

    ball_query / knn_points / FPS       (index-exact native ops)
    pdr_group_build / pdr_knn_build     QueryAndGroup / group_knn, channel-last, one pass
    pdr_fused_layer                     [GN-apply, ReLU, +embedding, +residual, concat] -> 1x1 conv
                                        (fp32 MFMA) -> bias -> GroupNorm moments, one pass per layer
    pdr_gn_reduce / pdr_gn_finalize     GroupNorm statistics -> per-(batch, channel) scale/shift
    pdr_attention_pool                  count mask, softmax over K, weighted sum

Per block (SA / feature-transfer / kNN-FP) the first GEMM computes the three 1x1 convs that
read the grouped tensor -- first_mlp conv, res_connect conv, attention key conv -- in one pass.
Supported family = every shipped config: bn (GroupNorm) on, bn_first off, ReLU, attention
pooling, kNN feature propagation without grouper, radius neighbourhoods, local + global
condition features.  Anything else raises NotImplementedError at construction.

The arithmetic is the reference's layer by layer (same GroupNorm definition, same injection
points); only the summation order inside GEMMs / moments differs, as it does between any two
BLAS back ends.

What is NOT evaluated layer by layer the reference's way, with the same results: the first conv of a
grouped block is split into per-point tables (SplitFirstConv), and a neighbourhood that ball_query filled with
`nsample` copies of one point is evaluated once (Dedup / SortedQueries: the per-neighbour launches walk only the
128-row tiles that hold a real neighbourhood, a per-query chain of the same layers stands in for the rest).
"""
import contextlib
import ctypes
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..pointnet2_ops import _ext
from ..pointnet2_ops.attention import MyGroupNorm
from .models.pointnet2_ssg_sem import calc_t_emb


# ---- evaluation variants --------------------------------------------------------------------------------------
# Module constants, not environment knobs (round 4: the seventeen PDR_* reads are gone; the variants that lost their
# A/B -- step embeddings ahead of the geometry fork, query-independent block halves on a third stream, row bounds on
# the two-stream fork -- are deleted, DESIGN.md section 4.4 keeps their measurements).  What is left are the
# reference-shaped / unfused forms of each fusion: tests monkeypatch them as cross-checks of the default, and
# tests/test_fused_gpu.py::test_ddpm_forward_with_every_non_default_variant runs the full DDPM forward with each.
# For same-box A/B runs the lab scripts set PDR_FUSED_OPTS="NAME=value,..." (parsed once, below).
#
# First conv of every grouped block through per-point U / V tables + pdr_gather_add instead of a GEMM over the
# materialised grouped tensor (see SplitFirstConv).  False = reference-shaped evaluation.
USE_SPLIT_FIRST = True
# Attention score conv over [q.expand(K) | k]: evaluate the query half once per query (see FusedAttention)
SPLIT_QUERY_CONV = True
# Last attention score conv + mask + softmax + weighted sum in one kernel (scores never written): the pooled
# epilogue of the wave-specialised layer kernel reduces the accumulators in place and reads the value rows in
# accumulator layout.  MI355X, B = 32, same box: 9.64 / 9.74 ms per step fused vs 10.30 / 10.28 separate.
FUSE_SCORE_POOL = True
# First call of a batch: run the condition branch through the fused blocks too (False: layer-by-layer torch path;
# the cross-check of test_fused_first_call_runs_the_condition_branch).
FUSE_CONDITION_BRANCH = True
# The first conv's (P x Cout) output is not written: its consumers (second MLP conv, attention key) gather
# U[idx] + V in the producer waves of the wave-specialised layer kernel (12.28 vs 12.58 ms per step materialised) ...
USE_VIRTUAL_FIRST = True
# ... also for the kNN (feature-propagation) blocks: consumers add d2 r1 + w r2 in their producer waves (GATH = 2)
USE_VIRTUAL_KNN = True
# The residual conv's columns of a virtual first conv are not written either: the layer that adds the residual
# gathers U_res[idx] + V_res (RADD + GATH instantiations), for residual windows of up to GATHER_RES channels
# (9.35 ms gathering only the 32-channel residuals, 9.24 up to 64, 9.20 all of them); kNN blocks: GATHER_RES_KNN.
GATHER_RES = 4096
GATHER_RES_KNN = True
# (Geometry: one event per level instead of one after the whole chain, -1.8 % step time at B = 32 in round 3; the
# one-event form is gone since round 5 -- its variant run found the unordered cross-stream read documented at xyz4().)
# Step-embedding chain as three pdr_embed_linear launches instead of ~12 torch / hipBLASLt ones (False: torch chain)
NATIVE_EMBED = True
# ... and, inside a sampler's loop, not even those: the chain depends on t only, so the samplers evaluate it for all T
# step values of their schedule once (FusedCloudConditionNet.build_step_table) and a step looks its row up
# (pdr_embed_select, one launch).  Round 3 measured this bit-identical and dropped it because the chain was hidden
# behind the first ball query; with one-point neighbourhoods evaluated once it ended at 0.28 ms of a 6.4-ms step
# (profiles/r4_timeline_markers.json).
STEP_TABLE = True
# The global PointNet of a new batch (models/pnet.py) through the fused layer kernels (False: the torch module ->
# MIOpen convolutions, what rounds 1-3 did)
FUSE_GLOBAL_PNET = True
# Neighbourhoods that are K copies of one row (ball_query pads with the first hit; a query with <= 1 point in its ball,
# the rule on x_t for most of a reverse process) are evaluated ONCE: the per-neighbour launches of a grouped block walk
# only the 128-row tiles that contain a real neighbourhood (pdr_dedup_plan), a per-QUERY chain of the same layers
# supplies the moments (x K) and the pooled rows of the others.  DESIGN.md section 4.7.  Blocks with fewer queries per
# cloud than DEDUP_MIN_QUERIES run whole (same box: 512 -> 7.35 ms, 256 -> 6.98, 64 -> 6.84 / 6.88; later, with the
# decoder halves hoisted, 64 -> 6.43 / 6.44, 16 -> 6.30: even the 16-query blocks, whose launches do next to nothing).
DEDUP = True
DEDUP_MIN_QUERIES = 16
# ... on the block's queries SORTED per cloud, real neighbourhoods first: a tile is walked when ANY of its 4 queries has a
# real neighbourhood, so unsorted 14 % such queries keep 45 % of the tiles; sorted, 14 %.  The block's per-query inputs
# (index rows, counts, coordinates, query features) are gathered in that order, its pooled rows are written back to
# their original places.  (Round 4 kept the unsorted form as a variant; round 5 builds on the sorted structure -- a
# cloud's valid tiles are its FIRST ones, the per-query rows that count are its LAST ones -- and dropped it.)
#
# Round 5: the launches the deduplicated step had added, taken out again (each with its round-4 form as a cross-check):
# sort + three row gathers + two plan kernels behind every ball query as ONE launch (pdr_dedup_prepare) ...
FUSED_PLAN = True
# ... the moments of the per-query rows computed by the per-query launches themselves (pdr_layer_in_t.wrow0 / wmul,
# pdr_gather_add_tiles_twin) and a fold that skips a cloud's invalid tile range (pdr_gn_fold nvalid) instead of a
# pdr_weighted_moments launch + zero fills behind every layer; the K = 1 first-neighbour gather_add rides in the
# launch that walks the tile subset ...
TWIN_STATS = True
# ... and the pooled rows of the skipped tiles' queries written by the pooled launch (pdr_layer_in_t.patch_values)
# instead of a pdr_patch_rows launch behind it.
FUSED_PATCH = True
# The statistics-only pass of a virtual first conv (pdr_gather_add with Y = NULL) walks only the column windows whose
# moments a GroupNorm reads (pdr_gather_moments*): the first conv's own columns and the attention's key columns, not the
# residual conv's window between them (22-33 % of the columns).  Same bits in the windows; False: the whole-width pass.
MOMENT_WINDOWS = True
# The query-independent half of the DECODER's feature-transfer blocks (first-conv statistics, shared MLP, value conv: it
# needs coordinates, the static condition features and the step embeddings only) on the geometry stream once that
# stream is done with the geometry (1.4 ms into the step), beside the encoder; the decoder then only runs the query /
# score / pooling half.  (Round 3 measured such a hoist slower at 11.7 ms per step, every kernel filling the chip; with
# one-point neighbourhoods evaluated once the launches are small.)
# (The same half of the ENCODER's blocks of levels >= 1 on a fourth stream, each as soon as its level's geometry exists:
# 7.07 vs 6.46 ms -- it runs beside the sampling chain and the SA blocks that everything else waits for.  Removed.)
AHEAD_DECODER_MAPS = True
# ... the level-0 one of them on the MAIN stream, right behind the first feature-transfer block: in a sampling loop the
# main stream then sits idle until the level-0 sampling is done (0.32 -> 0.57 ms: tools/lab/step_markers.py,
# MARK_BACK_TO_BACK), and that half needs level-0 coordinates only.  Same box: 6.04 / 6.02 vs 6.09 / 6.10 ms per step.
HOIST_LEVEL0_ON_MAIN = True
# Round 6: the same half of the ENCODER's feature-transfer blocks of levels >= 1 on the GEOMETRY stream, each right behind
# its level's neighbourhoods -- that stream spends most of the first millisecond waiting for the sampling chain, and the
# half needs that level's coordinates only; the block on the main stream is then its query / score / pooling half.
# (Round 4 tried this on a stream of its own, a FIFTH one, and lost 0.6 ms: the step's four streams are the device's four
# hardware queues -- tools/lab/two_batches.py: more queues, or two graphs in flight, serialise --, a fifth shares one.)
AHEAD_ENCODER_MAPS = True
# ... also in the step that evaluates every neighbourhood: 8.27 / 8.28 vs 8.31 / 8.31 ms per step, same box (unlike the
# sampling chain's own stream and the level-0 decoder half on the main stream, which pay only in the deduplicated form)
AHEAD_ENCODER_MAPS_WHOLE = True
# ... and the first SA block's per-source table (the source half of its split first conv: level-0 rows, ready when the
# first feature-transfer block is) in the main stream's idle window behind that block, ahead of the wait for the level-0
# sampling -- one 40-us launch less between the end of the sampling chain and the first SA block's output.
SA0_TABLE_AHEAD = True
# The per-source table U = [mapped | features | xyz] . W of the other SA blocks and of every feature-propagation block reads
# the output of the feature-transfer block in front of it (`mapped`) -- but only in its first 32-128 input channels; the
# rest (the level's own features and coordinates, 2/3 to 9/10 of the K walk) is ready BEFORE that feature-transfer block
# runs its query half, during which the blocks' second stream has nothing to do.  The table is therefore built in two
# launches: U_early = [features | xyz] . W[Cm:] on the second stream beside the feature-transfer block, then
# U = mapped . W[:Cm] + U_early (an output-side add of the layer kernel) on the critical path -- 40-65-us launches become
# 15-25-us ones.  Same products, another summation order (1e-6).  MEASURED AND LEFT OFF: 5.69 / 5.70 vs 5.61 / 5.64 ms per
# step (whole evaluation 8.63 / 8.66 vs 8.53 / 8.53), same box -- the fork / join of the second stream and the second
# launch cost more than the shorter K walk returns (a dependent launch costs what it costs, whatever its K).
SPLIT_SOURCE_TABLES = False
# Round 6: a block evaluated on SORTED queries no longer gathers its query features into that order in front of the
# query conv (one launch on the chain of every feature-transfer / SA block): the query conv and the query half of the
# first score conv run in the ORIGINAL query order and the per-neighbour launch reads the per-query term through the
# sorted -> original row map (pdr_layer_in_t.oadd_rows).
QUERIES_IN_PLACE = True
# Round 6: the attention's query conv of an SA / feature-propagation block (it reads the block's query features only) on the
# blocks' second stream at the head of the block, beside the per-source table and the first conv's statistics pass on the
# main stream -- it was the first link of the main stream's chain behind them.
QUERY_CONV_AHEAD = True
# (Tried: the per-query chain of a stage on a companion stream beside the stage's per-neighbour launch, both feeding the
# stage's fold.  From the block halves' auxiliary stream -- a fork of a forked stream -- hipStreamEndCapture segfaults
# (ROCm 7.2); from the main stream only it is slower, 6.90 / 6.93 vs 6.85 ms: the fork / join costs more than the
# 5-us launches it hides.  Removed.)


# Round 6: the per-point chains of the deep levels -- a feature-propagation block's second MLP on <= 256
# points per cloud -- as ONE launch (pdr_point_chain: a cluster of workgroups per cloud, column blocks of whole GroupNorm
# groups, so conv -> GroupNorm -> ReLU -> + embedding -> conv -> ... -> + residual needs no fold launch and no partial
# moments; csrc/point_chain.hip).  False: the layer-by-layer launches (the cross-check of
# tests/test_fused_gpu.py::test_point_chain_*).
POINT_CHAINS = True
# Round 6: a deduplicated block's per-neighbour launch (tile subset) and per-query launch of one layer as ONE launch
# (pdr_fused_layer_pair: the second problem's workgroups ride behind the first's) -- a block's launch chain loses a link
# per layer (plain / ball-gathered sources without a residual: the shared MLP's convs and the key half of the first
# score conv; the value conv, which adds a gathered residual, stays two launches).  False: one launch each.
PAIRED_LAUNCHES = True
# True: a layer launch walks its row tiles in the direction OPPOSITE to the launch that wrote its main source
# (pdr_layer_in_t.walk_reverse).  The activations of the 262,144- / 524,288-row levels (134 / 268 MB per layer) do not
# survive a launch in the 256-MB memory-side cache when the reader starts where the writer started; read from the end
# the writer's tail is still there: tools/lab/half_batch.py --zigzag, four plain 128 -> 128 layers + folds alone on the
# chip, 830 -> 734 us at 524,288 rows, 439 -> 398 at 262,144, same bits.  In the STEP it buys nothing (5.497 vs 5.492 ms,
# four alternating rounds of 100 steps; whole evaluation 8.50 vs 8.52): the wide launches of a feature-propagation block
# mostly read GATHERED tables, and between a producer and its consumer the block's other half streams 268 MB through
# the cache on the second stream (on one stream: 5.59-5.64 with and without).  Off; kept as a variant of the tests.
ZIGZAG_WALK = False


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Time stamps inside a step (tools/lab/step_markers.py sets MARKS = {"buf": uint64 device tensor, "names": []}):
# mark(name) launches pdr_mark_time on the CURRENT stream; capturable, so the stamps of an untraced graph replay
# can be read back afterwards.  None = no launches (the default).
MARKS = None


def mark(name, detail=False):
    if MARKS is None or (detail and not MARKS.get("detail")):
        return
    i = len(MARKS["names"])
    if i >= MARKS["buf"].numel():
        return
    MARKS["names"].append(name)
    _lib.check(_lib.load().pdr_mark_time(MARKS["buf"].data_ptr() + 8 * i, _stream()), "mark_time")


def _ptr(t, offset=0):
    return t.data_ptr() + 4 * offset


# The gathered form of a source segment: row p reads U[gidx[p]] + V[p / gK] (V0 for an empty ball; kNN form:
# + gs1[p] r1 + gs2[p] r2).  V / V0 / r1 / r2 are (tensor, offset in floats) pairs.
Gather = namedtuple("Gather", "V V0 ldv nsrc zrow r1 r2", defaults=(-1, None, None))


class Seg(namedtuple("Seg", "t off C ld div gather", defaults=(1, None))):
    """One source segment of an Act: columns [off, off + C) of the (rows, ld) tensor `t`; row p reads row p / div;
    `gather`: `t` is a per-source-point table read through the Act's neighbour index (a Gather)."""
    __slots__ = ()

    @property
    def gathered(self):
        return self.gather is not None

    @staticmethod
    def of(s):
        """A Seg from what call sites may hand over: a Seg, or its fields as a plain tuple (gather part as a dict)."""
        s = s if isinstance(s, Seg) else Seg(*s)
        return s._replace(gather=Gather(**s.gather)) if isinstance(s.gather, dict) else s

    def fill(self, cseg):
        """-> pdr_seg_t."""
        cseg.ptr, cseg.C, cseg.ld, cseg.row_div = _ptr(self.t, self.off), self.C, self.ld, self.div
        g = self.gather
        if g is not None:
            cseg.gV = _ptr(*g.V)
            cseg.gV0 = _ptr(*g.V0) if g.V0 is not None else None
            cseg.g_ldv, cseg.g_nsrc, cseg.g_zrow = g.ldv, g.nsrc, g.zrow
            if g.r1 is not None:                            # kNN form: + s1[p] r1[c] + s2[p] r2[c]
                cseg.g_r1, cseg.g_r2 = _ptr(*g.r1), _ptr(*g.r2)


class Act:
    """A lazily-evaluated activation: channel segments (`segs`, a list of Seg; `radd`, one Seg covering all channels
    that is added row-wise) + the prologue the consumer applies.  Segments may be given as Seg or as plain tuples
    (tensor, offset_floats, C, ld[, row_div[, gather as Gather or dict]]); they are Seg from here on."""

    def __init__(self, segs, P, B, rows_per_batch, scale=None, shift=None, add=None, add_ld=0, radd=None,
                 pre_relu=False, post_relu=False):
        self.segs = [Seg.of(s) for s in segs]
        self.P, self.B, self.rpb = P, B, rows_per_batch
        self.scale, self.shift, self.add, self.add_ld = scale, shift, add, add_ld
        self.radd = None if radd is None else Seg.of(radd)
        self.pre_relu, self.post_relu = pre_relu, post_relu
        self.C = sum(s.C for s in self.segs)
        self.gidx = self.gcnt = None   # shared neighbour index / ball counts of gathered segments
        self.gK = 0
        self.gs1 = self.gs2 = None     # kNN form: per-position distance / weight of gathered segments
        self.first = None              # the FirstOut the gathered segments come from (fallback: materialise)
        self.ss_ld = 0                 # leading dimension of scale / shift (0 = C)
        self.oadd = None               # (tensor (rows, ld), div): output-side per-query add
        self.oadd_rows = None          # int32 (P / div): row of `oadd` each query reads (None: its own)
        self.dd = None                 # Dedup plan of the block: the launch walks its tile subset
        self.twin = None               # the same activation over the block's per-QUERY rows (first neighbour only)
        self.wrow0, self.wmul = None, 0.0   # a twin's weighted statistics: rows >= wrow0[b] count, x wmul
        self.patch = None              # pooled launch: (per-query value rows, row weights) of the skipped tiles

    def walk(self):
        """Direction of a launch over this activation: opposite to the producer of its widest materialised segment
        (ZIGZAG_WALK); forward when that producer is unknown (a table, an input) or the launch walks a tile list."""
        if not ZIGZAG_WALK or self.dd is not None:
            return 0
        best = None
        for sg in self.segs + ([self.radd] if self.radd is not None else []):
            if not sg.gathered and sg.div == 1 and (best is None or sg.C > best.C):
                best = sg
        if best is None:
            return 0
        return 1 - _WALK.get(best.t.data_ptr(), 1)

    _SHARED = ("scale", "shift", "add", "add_ld", "pre_relu", "post_relu", "ss_ld")

    def __setattr__(self, k, v):
        object.__setattr__(self, k, v)
        tw = self.__dict__.get("twin")
        if tw is not None and k in Act._SHARED:            # the prologue is the same for both row sets
            object.__setattr__(tw, k, v)

    def struct(self, partial_tpb=0, weighted=True):
        """-> pdr_layer_in_t.  partial_tpb: rows per cloud of the statistics tensor the launch writes (0: the tile
        subset's own count, or one row per tile); weighted=False: a twin's launch without its weighted statistics."""
        li = _lib.LayerIn()
        li.n_seg = len(self.segs)
        for i, seg in enumerate(self.segs):
            seg.fill(li.seg[i])
        li.scale = self.scale.data_ptr() if self.scale is not None else None
        li.shift = self.shift.data_ptr() if self.shift is not None else None
        li.add = self.add.data_ptr() if self.add is not None else None
        li.add_ld = self.add_ld if self.add is not None else 0
        if self.radd is not None:
            self.radd.fill(li.rseg)
        li.pre_relu, li.post_relu, li.rows_per_batch = int(self.pre_relu), int(self.post_relu), self.rpb
        li.ss_ld = self.ss_ld
        if self.oadd is not None:
            li.oadd, li.oadd_ld, li.oadd_div = self.oadd[0].data_ptr(), self.oadd[0].shape[1], self.oadd[1]
            if self.oadd_rows is not None:
                li.oadd_rows = self.oadd_rows.data_ptr()
        if self.gidx is not None:
            li.gidx = self.gidx.data_ptr()
            li.gcnt = self.gcnt.data_ptr() if self.gcnt is not None else None
            li.gK = self.gK
            if self.gs1 is not None:
                li.gs1, li.gs2 = self.gs1.data_ptr(), self.gs2.data_ptr()
        li.partial_tpb = partial_tpb
        if self.dd is not None:
            li.tile_list, li.n_tiles = self.dd.tile_list.data_ptr(), self.dd.n_tiles.data_ptr()
            li.partial_tpb = partial_tpb or self.dd.ptpb
        if weighted and self.wrow0 is not None:
            li.wrow0, li.wmul = self.wrow0.data_ptr(), self.wmul
        if self.patch is not None:
            Vd, w = self.patch
            li.patch_values, li.patch_ld, li.patch_w = Vd.data_ptr(), Vd.shape[1], w.data_ptr()
        li.walk_reverse = self.walk()
        return li


# One-point neighbourhoods are evaluated once only while BOTH hold: the module constant above (tests / lab A-B) and the
# switch of the network whose forward is in flight (FusedCloudConditionNet.dedup: the sampler captures the step both
# ways and picks per step, reverse_sampler.py).
_NET_DEDUP = [True]
# probe counters of the forward in flight (int32[2] device tensor or None): [0] += tiles a plan walks, [1] += tiles
_PROBE = [None]


def _dedup_on():
    return DEDUP and _NET_DEDUP[0]


def _probe_ptr():
    return _PROBE[0].data_ptr() if _PROBE[0] is not None else None


class Dedup:
    """Plan of one grouped block's per-neighbour launches on its SORTED queries: which 128-row tiles hold a real
    neighbourhood (a cloud's first nvalid[b]), the weights / first neighbours of the per-query chain that stands in for
    the others (a cloud's queries from wrow0[b] on)."""

    def __init__(self, idx, counts, B, m, K, prepared=None):
        dev = idx.device
        self.B, self.m, self.K = B, m, K
        self.tpb, self.tpbd = m * K // 128, (m + 127) // 128
        self.ptpb = self.tpb + self.tpbd                       # partial rows per cloud: [tiles | per-query tiles]
        nt = B * self.tpb
        self.idx0 = torch.empty((B, m), dtype=torch.int32, device=dev)
        self.row_w = torch.empty((B * m,), dtype=torch.float32, device=dev)
        self.tile_valid = torch.empty((nt,), dtype=torch.uint8, device=dev)
        self.tile_list = torch.empty((nt,), dtype=torch.int32, device=dev)
        self.n_tiles = torch.empty((1,), dtype=torch.int32, device=dev)
        self.nvalid = None                                     # (2, B) int32: [valid tiles | first weighted query]
        if prepared is not None:
            prepared(self)                                     # pdr_dedup_prepare fills everything (SortedQueries)
            return
        _lib.check(_lib.load().pdr_dedup_plan(idx.data_ptr(), counts.data_ptr(), B, m, K, self.idx0.data_ptr(),
                                              self.row_w.data_ptr(), self.tile_valid.data_ptr(),
                                              self.tile_list.data_ptr(), self.n_tiles.data_ptr(), _stream()),
                   "dedup_plan")
        # (the round-4 form, a cross-check variant: what pdr_dedup_prepare also returns, in a few torch launches)
        nv = self.tile_valid.view(B, self.tpb).sum(1, dtype=torch.int32)
        self.nvalid = torch.stack([nv, nv * (128 // K)]).contiguous()
        if _PROBE[0] is not None:
            _PROBE[0][0:1] += self.n_tiles
            _PROBE[0][1:2] += nt

    @property
    def wrow0(self):
        return self.nvalid[1]

    def moments(self, Yd, C, relu_col0, partial):
        """Weighted moments of the per-query rows behind the tile subset's, zeros for the skipped tiles (the round-4
        form: TWIN_STATS = False)."""
        _lib.check(_lib.load().pdr_weighted_moments(Yd.data_ptr(), Yd.shape[1], self.B, self.m, C, relu_col0,
                                                    self.row_w.data_ptr(), partial.data_ptr(), self.ptpb, self.tpb,
                                                    self.tile_valid.data_ptr(), _stream()), "weighted_moments")


class SortedQueries:
    """A grouped block's queries in the order it evaluates them: the stable partition of the ball counts (real
    neighbourhoods first), its inverse, the ball query's outputs / the query coordinates gathered into that order, and
    the Dedup plan of the sorted arrays (`plan`).  One pdr_dedup_prepare launch (FUSED_PLAN; six launches before)."""

    def __init__(self, idx, counts, new_xyz):
        B, m, K = idx.shape
        dev = idx.device
        lib = _lib.load()
        self.perm = torch.empty((B, m), dtype=torch.int32, device=dev)
        self.inv = torch.empty((B, m), dtype=torch.int32, device=dev)
        self.perm_rows = torch.empty((B, m), dtype=torch.int32, device=dev)     # b m + perm: rows of a (B m)-row tensor
        self.plan = None
        if FUSED_PLAN and K in (8, 16, 32) and (m * K) % 128 == 0 and B <= 1024 and m <= 4096:
            new_xyz = new_xyz.contiguous()
            self.idx = torch.empty_like(idx)
            self.counts = torch.empty_like(counts)
            self.xyz = torch.empty_like(new_xyz)
            nvalid = torch.empty((2, B), dtype=torch.int32, device=dev)

            def prepared(dd):
                _lib.check(lib.pdr_dedup_prepare(
                    idx.data_ptr(), counts.data_ptr(), new_xyz.data_ptr(), B, m, K, self.perm.data_ptr(),
                    self.inv.data_ptr(), self.perm_rows.data_ptr(), self.idx.data_ptr(), self.counts.data_ptr(),
                    self.xyz.data_ptr(), dd.idx0.data_ptr(), dd.row_w.data_ptr(), dd.tile_valid.data_ptr(),
                    dd.tile_list.data_ptr(), dd.n_tiles.data_ptr(), nvalid.data_ptr(), _probe_ptr(), _stream()),
                    "dedup_prepare")
                dd.nvalid = nvalid
            self.plan = Dedup(self.idx, self.counts, B, m, K, prepared=prepared)
            return
        _lib.check(lib.pdr_dedup_sort(counts.data_ptr(), B, m, self.perm.data_ptr(), self.inv.data_ptr(),
                                      self.perm_rows.data_ptr(), _stream()), "dedup_sort")
        # (rows of 32-bit words moved as they are: the row gather does no arithmetic)
        self.idx = gather_rows(idx.view(torch.float32), self.perm).view(torch.int32)
        self.counts = gather_rows(counts.view(B, m, 1).view(torch.float32), self.perm).view(torch.int32).view(B, m)
        self.xyz = gather_rows(new_xyz.contiguous(), self.perm)
        if K in (8, 16, 32) and (m * K) % 128 == 0:
            self.plan = Dedup(self.idx, self.counts, B, m, K)


# Columns [col0, col0 + C) of a set of statistics, counted `mult` times: what Norm.fold and FoldReq.second take
# (Stats.window makes one; a plain tuple of the same fields is accepted).
Window = namedtuple("Window", "partial col0 C tpb mult sub", defaults=(1.0, None))


class Stats(namedtuple("Stats", "partial tpb sub", defaults=(None,))):
    """The GroupNorm moments a launch wrote: `partial` (B tpb, C, 2) -- None when none were asked for --, its rows per
    cloud `tpb`, and, when a tile subset produced them, `sub` = (valid tiles per cloud, main tiles per cloud), the
    subset arguments of pdr_gn_fold."""
    __slots__ = ()

    def window(self, col0, C, mult=1.0):
        return Window(self.partial, col0, C, self.tpb, mult, self.sub)


class LayerOut:
    """What run_layer returns: `Y`, its `stats` (a Stats), `folded` = (scale, shift) when a fold was requested with the
    layer, and what a DEDUPLICATED layer adds: `twin` (the output of its per-query rows) and `dd` (the block's Dedup
    plan).  Iterating gives (Y, partial, tiles_per_batch), the spelling of the kernel tests."""
    __slots__ = ("Y", "stats", "folded", "twin", "dd")

    def __init__(self, Y, stats, folded=None, twin=None, dd=None):
        self.Y, self.stats, self.folded, self.twin, self.dd = Y, stats, folded, twin, dd

    def __iter__(self):
        return iter((self.Y, self.stats.partial, self.stats.tpb))


# What one half of a block hands to the other:
# FusedAttention.values: the value conv's output, its folded GroupNorm, the per-query value rows of a deduplicated block
Values = namedtuple("Values", "V scale shift twin")
# EmbeddingBank.get: the (B, C) block of one registered Linear = columns [off, off + C) of `t` (leading dimension ld)
Injected = namedtuple("Injected", "t off ld")
# per-query first-conv tables [V | V0] made ahead of a block, and the query order they were made for (a SortedQueries;
# None: the original order)
QueryTables = namedtuple("QueryTables", "V2 order", defaults=(None,))
# a grouped block behind its first conv (FusedGroupedBlock._head): sizes, the ball counts and the first conv in the
# block's query order `sq` (a SortedQueries or None); rows: the row map of query features left in their original order.
# query / q_ahead belong to the OTHER half -- the query features in the block's order and their query conv made ahead --
# and are here only because the two-stream form issues both ahead of the first conv (the head is given the queries then)
Head = namedtuple("Head", "B m K counts first folded sq rows query q_ahead", defaults=(None,) * 5)
# FusedGroupedBlock.prepare: the head, the value half (a thunk) and the event behind both when another stream ran them
Prepared = namedtuple("Prepared", "head values event", defaults=(None,))


def _ready(x):
    """The thunk form of a value that exists already (see _on_aux for one that another stream is still making)."""
    return lambda: x


def act_from(lo, C, P, B, rpb, **kw):
    """Act over the first C columns of a LayerOut, with its per-query twin when the layer ran deduplicated."""
    a = Act([Seg(lo.Y, 0, C, lo.Y.shape[1])], P, B, rpb, **kw)
    if lo.dd is not None:
        a.dd = lo.dd
        a.twin = _twin_act([Seg(lo.twin, 0, C, lo.twin.shape[1])], lo.dd, B, **kw)
    return a


def _twin_act(segs, dd, B, **kw):
    """Act over a deduplicated block's per-QUERY rows; with TWIN_STATS its launch weights its own statistics."""
    tw = Act(segs, dd.B * dd.m, B, dd.m, **kw)
    if TWIN_STATS:
        tw.wrow0, tw.wmul = dd.wrow0, float(dd.K)
    return tw


class FirstOut:
    """Output of a block's first conv and its statistics (`stats`, a Stats): a materialised (P, ld) tensor, or VIRTUAL =
    per-source-point table U (with one all-zero row appended), per-query table V2 = [V | V0] and the neighbour index,
    read by consumers as a gathered source (seg() gives the Seg of a column window either way).  In virtual form the
    residual columns [res_col0, res_col0 + res.shape... ) may still be materialised (`Yres`): they are consumed as a
    row-wise residual, which stays a plain read."""

    def __init__(self, Y=None, stats=None, U=None, V2=None, ld=0, has_v0=False, idx=None, counts=None, K=0, nsrc=0,
                 zrow=-1, Yres=None, res_col0=0, res_cols=0, s1=None, s2=None, r1=None, r2=None, materialise=None):
        self.Y, self.stats, self.U, self.V2, self.ld, self.has_v0 = Y, stats, U, V2, ld, has_v0
        self.idx, self.counts, self.K, self.nsrc, self.zrow = idx, counts, K, nsrc, zrow
        self.Yres, self.res_col0, self.res_cols = Yres, res_col0, res_cols
        self.s1, self.s2, self.r1, self.r2 = s1, s2, r1, r2          # kNN form (r1 / r2: padded conv rows)
        self.materialise = materialise                                # (col0, C) -> (P, pad4(C)) tensor
        self.dd, self.deg = None, None      # Dedup plan + the first conv of the per-query rows (B m, ld), materialised

    @property
    def virtual(self):
        return self.Y is None

    def seg(self, col0, C):
        if not self.virtual:
            return Seg(self.Y, col0, C, self.Y.shape[1])
        if self.Yres is not None and col0 >= self.res_col0 and col0 + C <= self.res_col0 + self.res_cols:
            return Seg(self.Yres, col0 - self.res_col0, C, self.Yres.shape[1])
        kNN = self.s1 is not None
        g = Gather(V=(self.V2, col0), V0=(self.V2, self.ld + col0) if self.has_v0 else None, ldv=self.V2.shape[1],
                   nsrc=self.nsrc, zrow=self.zrow, r1=(self.r1, col0) if kNN else None,
                   r2=(self.r2, col0) if kNN else None)
        return Seg(self.U, col0, C, self.U.shape[1], 1, g)

    def attach(self, act):
        if self.virtual:
            act.gidx, act.gcnt, act.gK = self.idx, self.counts, self.K
            act.gs1, act.gs2, act.first = self.s1, self.s2, self
        if self.dd is not None:
            dd, Yd = self.dd, self.deg
            if act.twin is None:
                # the activation reads this first conv: its twin reads the same columns of the per-query rows
                if len(act.segs) != 1 or not act.segs[0].gathered:
                    raise NotImplementedError("deduplicated block: one gathered source per layer")
                sg = act.segs[0]
                tw = _twin_act([Seg(Yd, sg.off, sg.C, Yd.shape[1])], dd, act.B)
                for k in Act._SHARED:
                    object.__setattr__(tw, k, getattr(act, k))
                act.dd, act.twin = dd, tw
            if act.radd is not None and act.radd.gathered:      # gathered residual window
                act.twin.radd = Seg(Yd, act.radd.off, act.radd.C, Yd.shape[1])
        return act


def _pad4(c):
    return (c + 3) // 4 * 4


# xyz4's cache entry: the source tensor, its padded copy, the stream that made the copy and an event behind it
Padded = namedtuple("Padded", "src padded stream event")
_XYZ4 = {}
# Per-forward registry of what the geometry prepass made for a neighbour-index tensor (keyed by the tensor's id; the
# entry, a Geom, holds the tensor, so the id cannot be reused within the forward).
# Cleared with _XYZ4 at the start of a forward.  (Rounds 4-5 hung these on the index tensors as attributes.)
_GEOM = {}
# per forward: data_ptr of a layer output -> the direction (0 forward / 1 reversed) its producer walked (ZIGZAG_WALK)
_WALK = {}


def _new_forward():
    _XYZ4.clear()
    _GEOM.clear()
    _WALK.clear()


class Geom:
    """_GEOM's entry for the index tensor `tensor`: `sorted`, its SortedQueries once made; `probed`: its probe ran."""
    __slots__ = ("tensor", "sorted", "probed")

    def __init__(self, tensor):
        self.tensor, self.sorted, self.probed = tensor, None, False


def _geom(idx, create=False):
    e = _GEOM.get(id(idx))
    if e is None and create:
        e = _GEOM[id(idx)] = Geom(idx)
    return e


def xyz4(t):
    """(B, n, C) channel-last rows padded to a multiple of 4 floats (cached per forward): as a C-wide segment
    with a 16-byte-aligned leading dimension they qualify for the float4-staged kernels; ld = 3 (coordinates)
    or 35 would force the scalar-load path.  Returns the padded tensor (last dim = ld).
    The cache is shared by the streams of a forward: an entry remembers the stream that produced it and an event
    behind the pad launch, and a hit from ANOTHER stream waits for that event first (round 4 ordered such pairs by hand,
    producing the copy before a fork or on the consumer's stream; the one pair nobody had ordered -- the first
    feature-transfer block's in-block tables on the main stream against its decoder twin's on the geometry stream,
    LEVEL_EVENTS = False -- read the copy before it was written: tests/test_fused_gpu.py, variant test, mixed input)."""
    if t.shape[-1] % 4 == 0:
        return t
    key = (t.data_ptr(), tuple(t.shape))
    hit = _XYZ4.get(key)
    if hit is None:
        # the entry holds the SOURCE too: while it lives, the allocator cannot hand the source's address to
        # another same-shape tensor, so a key can never alias a different tensor within one forward
        C = t.shape[-1]
        stream = ev = None
        if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous():
            padded = torch.empty(t.shape[:-1] + (_pad4(C),), dtype=torch.float32, device=t.device)
            _lib.check(_lib.load().pdr_pad_rows(t.data_ptr(), t.numel() // C, C, padded.data_ptr(), _pad4(C),
                                                _stream()), "pad_rows")
        else:
            padded = torch.nn.functional.pad(t, (0, -C % 4)).contiguous()
        if t.is_cuda:
            cur = torch.cuda.current_stream(t.device)
            stream, ev = cur.cuda_stream, torch.cuda.Event()
            ev.record(cur)
        hit = _XYZ4[key] = Padded(t, padded, stream, ev)
    elif hit.event is not None:
        cur = torch.cuda.current_stream(t.device)
        if cur.cuda_stream != hit.stream:
            cur.wait_event(hit.event)
    return hit.padded


def plain(t2d, B, rows_per_batch, row_div=1, C=None):
    """Act over a (rows, ld) tensor whose first C columns are the channels (ld may be padded)."""
    rows, ld = t2d.shape
    C = ld if C is None else C
    return Act([Seg(t2d, 0, C, ld, row_div)], rows * row_div, B, rows_per_batch)


class Conv:
    """A 1x1 conv (or several sharing the input, concatenated along the outputs) as Wt (Cin, Cout)."""

    def __init__(self, convs):
        convs = [c for c in convs if c is not None]
        ws = [c.weight.detach().reshape(c.weight.shape[0], -1) for c in convs]
        wt = torch.cat(ws, 0).t().contiguous()
        self.Cin, self.Cout = wt.shape
        dev = wt.device
        # leading dimension padded to a multiple of 4 floats: the kernel stages W with 16-B loads
        self.ldw = _pad4(self.Cout)
        self.Wt = torch.zeros((self.Cin, self.ldw), dtype=torch.float32, device=dev)
        self.Wt[:, :self.Cout] = wt
        self.bias = torch.cat([c.bias.detach() if c.bias is not None else torch.zeros(w.shape[0], device=dev)
                               for c, w in zip(convs, ws)]).contiguous()
        self.widths = [w.shape[0] for w in ws]
        self.f16x3 = {}           # split-f16 weight images: source segment widths + (column-block width,) -> (image, chunks)
        self.pair_ok = {}         # (rows per cloud, queries per cloud) -> False once pdr_fused_layer_pair declined the shape

    def f16x3_image(self, seg_widths, TN):
        """(image, chunks) of pack_f16x3 for sources of these widths and TN-column blocks, packed once."""
        key = tuple(seg_widths) + (TN,)
        if key not in self.f16x3:
            self.f16x3[key] = pack_f16x3(self.Wt, self.Cout, key[:-1], TN)
        return self.f16x3[key]


# Every grouped block evaluates its two independent halves -- shared MLP + value conv | query conv + score convs --
# on two streams between the first GEMM and the pooling (parallel branches of the captured hipGraph).
# `_PAR["stream"]` is set by the network around its forward.  Measured on MI355X (B = 32, same box, ms per step):
# off 11.08 / 11.14, only the blocks of <= 65,536 positions 11.05 / 11.03, all blocks 10.89 / 10.88 (B = 8: 5.61 ->
# 5.30 with the deep levels alone): the small launches of one half fill the gaps and tails of the other, also at
# level 0 -- so every block forks (the row bounds of rounds 2-3 are gone).
# Per-query first-conv tables ([V | V0]: coordinates x static weights; one thin launch per block) are evaluated on the
# geometry stream as soon as a level's coordinates exist, ahead of that level's event, instead of at the head of
# their block on the main stream (8.615 / 8.601 / 8.623 vs 8.642 / 8.660 / 8.675 ms inside the blocks).
SIDE_TABLES = True
# The sampling chain (FPS + gather per level) on a stream of its own instead of in front of each level's groupings on the
# geometry stream: same box, 60 back-to-back replays, 6.07 / 6.13 vs 6.16 / 6.16 ms per step.
# (ISSUE ORDER, measured with it: a LONE replay of the step shows the main stream's first kernel 0.29 ms into the step --
# the graph's nodes reach the hardware queues one after the other in creation order, the geometry stream's ~50 first --
# and interleaving the launches by need (sampling 0, first neighbourhoods, first block, level-l groupings just ahead of
# the blocks that wait for them, the hoisted decoder halves last) moved the first block from 0.43 to 0.26 ms and the
# end of the step from 6.28 to 6.18 ms in that picture.  In a sampling LOOP the host submits step i + 1 while step i
# runs, the head is not waiting for its own submission, and the interleaved order was SLOWER: 6.44 / 6.46 vs 6.07 / 6.13
# ms per step (with the sampling chain on the geometry stream 6.81 / 6.83 vs 6.16).  Geometry first, as in round 4.)
FPS_STREAM = True
# (The feature-propagation blocks' two halves on ONE stream -- VERDICT r4 item 3: their kernels fill the chip, the dominant
# one takes 182 us inside the two-stream step against 145 us alone --: 6.07 / 6.06 vs 6.05 / 6.08 ms per step, same box:
# what one kernel loses beside its neighbour the neighbour gains.  Not a switch.)
_PAR = {"stream": None}


def _on_aux(fn):
    """fn() on the blocks' second stream, behind everything the current stream has issued; returns a thunk that makes
    the current stream wait for it and yields fn's result (None when there is no second stream)."""
    aux = _PAR["stream"]
    if aux is None:
        return None
    main = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(main)
    aux.wait_event(ev)
    with torch.cuda.stream(aux):
        result = fn()
        done = torch.cuda.Event()
        done.record(aux)

    def join():
        main.wait_event(done)
        return result
    return join


@contextlib.contextmanager
def _single_stream():
    """The blocks inside run both halves on the current stream (a half hoisted onto a stream that is busy anyway)."""
    saved, _PAR["stream"] = _PAR["stream"], None
    try:
        yield
    finally:
        _PAR["stream"] = saved


# Arithmetic of the wide GEMMs of the forward in flight: "f32" (exact fp32 MFMA, default) or "split_f16"
# (opt-in; FusedCloudConditionNet(precision=...) sets it around its forward).  See pack_f16x3 / run_layer.
_PRECISION = ["f32"]
# tile variants that have a split-f16 instantiation: 4 / 5 (128-column blocks), 8 (64-column blocks)
SPLIT_VARIANTS = (4, 5, 8)
# layers with fewer input channels stay exact (HBM-bound: nothing to gain).  Same box, split step: 128 -> 7.33 ms, 64 ->
# 7.16, 32 -> 7.16 (the 64-channel layers of the 64-column tiles are the ones that matter)
SPLIT_MIN_CIN = 64


def _apply_lab_opts():
    """PDR_FUSED_OPTS="NAME=value,NAME=value": lab override of the module constants above for same-box A/B runs
    (tools/lab/ab_env.sh); values are parsed with the type of the constant they replace."""
    spec = __import__("os").environ.get("PDR_FUSED_OPTS", "")
    for item in filter(None, (t.strip() for t in spec.split(","))):
        name, _, val = item.partition("=")
        cur = globals().get(name)
        if name.startswith("_") or not isinstance(cur, (bool, int)):
            raise ValueError("PDR_FUSED_OPTS: unknown option %r" % name)
        globals()[name] = (val.lower() in ("1", "true", "on")) if isinstance(cur, bool) else int(val)


_apply_lab_opts()


def pack_f16x3(Wt, Cout, seg_widths, TN=128):
    """Weight image of pdr_fused_layer_f16x3 (layout contract in include/pdr_hip.h): Wt (Cin, >= Cout) fp32 ->
    int16 tensor [column block][chunk][hi | lo][TN cols][32 k], k-granules XOR-swizzled; TN = column-block width of the
    tile variant that will run the layer (128, or 64 for variant 8); returns (image, chunks)."""
    KC = 32
    W = Wt[:, :Cout].float()
    half = torch.float16
    hi = W.to(half)                                             # round to nearest even, as v_cvt_pk_f16_f32
    # (packed once per layer, before any graph capture: the check may synchronise)
    if not bool(torch.isfinite(hi).all()):
        raise ValueError("split-f16 arithmetic: a weight is not finite or exceeds the f16 range (65504); use "
                         "precision='f32' for this network")
    lo = (W - hi.float()).to(half)                              # (subnormal halves kept, as the kernel's operands)
    chunks, k = [], 0
    for C in seg_widths:
        for ks in range(0, C, KC):
            chunks.append((k + ks, min(KC, C - ks)))
        k += C
    assert k == W.shape[0]
    ncb = (Cout + TN - 1) // TN
    img = torch.zeros((ncb, len(chunks), 2, TN, KC), dtype=half, device=Wt.device)
    for cb in range(ncb):
        n0 = cb * TN
        nn_ = min(TN, Cout - n0)
        for ci, (k0, km) in enumerate(chunks):
            img[cb, ci, 0, :nn_, :km] = hi[k0:k0 + km, n0:n0 + nn_].t()
            img[cb, ci, 1, :nn_, :km] = lo[k0:k0 + km, n0:n0 + nn_].t()
    # granule g (8 k = 16 bytes) of column n is stored at position g ^ ((n >> 2) & 3)  (XOR: an involution)
    img = img.view(ncb, len(chunks), 2, TN, 4, 8)
    n = torch.arange(TN, device=Wt.device)
    pos = torch.arange(4, device=Wt.device)[None, :] ^ ((n >> 2) & 3)[:, None]          # [n][p] -> source granule
    img = img.gather(4, pos[None, None, None, :, :, None].expand_as(img)).contiguous()
    return img.view(torch.int16).reshape(-1), len(chunks)


def _launch_split(lib, act, conv, li, y_ptr, ldy, partial_ptr, relu_col0, tiny_exact=True):
    """Try the f16x3 entry point; False when this layer is not carried by it (caller uses the exact kernel).
    tiny_exact=False: also for the tiny layers that run_layer leaves to the exact kernel (kernel tests)."""
    if _PRECISION[0] != "split_f16" or conv.Cin < SPLIT_MIN_CIN:
        return False
    if torch.is_tensor(partial_ptr):                    # (callers may hand over the statistics tensor itself)
        partial_ptr = partial_ptr.data_ptr()
    variant = lib.pdr_fused_layer_variant(act.rpb, conv.Cout)
    if variant not in SPLIT_VARIANTS:
        return False
    # (a tiny layer -- a few dozen workgroups, bound by its serial chunk walk, not by the matrix pipes -- is faster on
    # the exact right-sized launch than on the split tiles: pdr_fused_layer_plan out[7])
    plan = (ctypes.c_int * 8)()
    if lib.pdr_fused_layer_plan(ctypes.byref(li), act.P, conv.Cin, conv.Wt.data_ptr(), conv.ldw, conv.Cout, y_ptr, ldy,
                                plan) == _lib.PDR_OK and plan[7] and tiny_exact:
        return False
    img, nch = conv.f16x3_image([sg.C for sg in act.segs], 64 if variant == 8 else 128)
    rc = lib.pdr_fused_layer_f16x3(ctypes.byref(li), act.P, conv.Cin, img.data_ptr(), nch, conv.bias.data_ptr(),
                                    conv.Cout, y_ptr, ldy, partial_ptr, relu_col0, _stream())
    if rc == _lib.PDR_EUNSUPPORTED:
        return False
    _lib.check(rc, "fused_layer_f16x3")
    return True


_run_layer_split = _launch_split          # (the name the kernel tests and tools/lab/split_half.py call it by)


def _ldy(Cout):
    # rows of wide, odd-width outputs (105, 140, 297 ... = [first | res | key] GEMMs) start on
    # 128-byte boundaries: pad the leading dimension, consumers address columns through `ld`
    # (narrow outputs: a multiple of 4 floats, so that consumers can stage them with 16-B loads)
    return _pad4(Cout) if (Cout <= 64 or Cout % 32 == 0) else (Cout + 31) // 32 * 32


class FoldReq:
    """The GroupNorm fold that follows a layer, requested together with the layer: channels = columns
    [col0, col0 + C0) of that layer's output (+ the columns of `second`, a Window of another launch's statistics).
    (Round 3 carried such folds inside the producing launch -- per-batch-element device tickets, the completing
    workgroup folds -- and measured it slower at every size; the request object stayed because it keeps
    the producer and its GroupNorm in one place.)"""

    def __init__(self, norm, C0, n, col0=0, mult0=1.0, second=None):
        self.norm, self.C0, self.n, self.col0, self.mult0, self.second = norm, C0, n, col0, mult0, second

    @property
    def C(self):
        return self.C0 + (self.second.C if self.second else 0)

    def launch(self, stats, B):
        """pdr_gn_fold over this request's window of `stats` (the producing layer's Stats) -> (scale, shift)."""
        parts = [stats.window(self.col0, self.C0, self.mult0)] + ([self.second] if self.second else [])
        return self.norm.fold(parts, B, self.C, self.n)


def _stats_rows(lib, act, conv, stats):
    """Where the statistics of a layer over `act` go -> (rows of `partial` per cloud, twin_stats).  Plain: one row per
    tile.  Deduplicated (act.dd): the tile subset's rows, then the per-query rows' -- twin_stats: written by the
    per-query launch itself (pdr_layer_in_t.wrow0 / wmul), one per tile of that launch, whatever tile height it
    picks; else pdr_weighted_moments' groups of 128 rows.  (The paired launch has a layout of its own: _launch_pair.)"""
    tm = lib.pdr_fused_layer_tile_rows(act.rpb, conv.Cout)
    tpb = (act.rpb + tm - 1) // tm
    dd = act.dd
    if dd is None:
        return tpb, False
    assert tm == 128 and tpb == dd.tpb, (tm, tpb, dd.tpb)
    twin_stats = act.twin is not None and stats and TWIN_STATS and act.twin.wrow0 is not None
    tmd = lib.pdr_fused_layer_tile_rows(dd.m, conv.Cout)
    return dd.tpb + ((dd.m + tmd - 1) // tmd if twin_stats else dd.tpbd), twin_stats


def _launch_pair(lib, act, conv, Y, y_ptr, ldy, stats, rc0):
    """Both row sets of a deduplicated layer in ONE launch (128-row tiles for the per-query rows too: their statistics
    rows follow the tile subset's) -> LayerOut, or None when the layer runs as two launches."""
    dd, tw = act.dd, act.twin
    if not PAIRED_LAUNCHES or _PRECISION[0] != "f32" or act.radd is not None or \
            not conv.pair_ok.get((act.rpb, dd.m), True):
        return None
    tpb_p = dd.tpb + (dd.m + 127) // 128
    part_p = torch.empty((act.B * tpb_p, conv.Cout, 2), dtype=torch.float32, device=Y.device) if stats else None
    Yd = torch.empty((tw.P, ldy), dtype=torch.float32, device=Y.device)
    li, li2 = act.struct(tpb_p if stats else 0), tw.struct(tpb_p if stats else 0)
    # only where the per-query launch runs on the wave-specialised 128-row tiles anyway (the 1024- / 2048-query
    # levels): the deep levels' per-query rows have launches of their own size that beat riding on
    # 128-row tiles by more than the launch they would save (measured: all levels paired 5.78 vs 5.75 ms unpaired)
    plan = (ctypes.c_int * 8)()
    rc = lib.pdr_fused_layer_plan(ctypes.byref(li2), tw.P, conv.Cin, conv.Wt.data_ptr(), conv.ldw, conv.Cout,
                                  Yd.data_ptr(), ldy, plan)
    if rc == _lib.PDR_OK and plan[0] == 1 and plan[7] == 0 and plan[1] in (2, 4, 7, 8):
        rc = lib.pdr_fused_layer_pair(ctypes.byref(li), act.P, ctypes.byref(li2), tw.P, conv.Cin, conv.Wt.data_ptr(),
                                      conv.ldw, conv.bias.data_ptr(), conv.Cout, y_ptr, ldy, Yd.data_ptr(), ldy,
                                      part_p.data_ptr() if stats else None,
                                      _ptr(part_p, dd.tpb * conv.Cout * 2) if stats else None, rc0, _stream())
        if rc == _lib.PDR_OK:
            return LayerOut(Y, Stats(part_p, tpb_p, (dd.nvalid[0], dd.tpb) if stats else None), twin=Yd, dd=dd)
        if rc != _lib.PDR_EUNSUPPORTED:
            _lib.check(rc, "fused_layer_pair")
    conv.pair_ok[(act.rpb, dd.m)] = False                   # (not asked again for this shape)
    return None


def _launch_exact(lib, act, conv, li, y_ptr, ldy, partial_ptr, rc0):
    """pdr_fused_layer; returns the pdr_layer_in_t that was launched: `li`, or that of the plain sources a kNN-form
    gathered source was materialised into."""
    def launch():
        return lib.pdr_fused_layer(ctypes.byref(li), act.P, conv.Cin, conv.Wt.data_ptr(), conv.ldw,
                                   conv.bias.data_ptr(), conv.Cout, y_ptr, ldy, partial_ptr, rc0, _stream())
    rc = launch()
    if rc == _lib.PDR_EUNSUPPORTED and act.gs1 is not None and act.first is not None:
        # a kNN-form gathered source reached a tile shape without a wave-specialised kernel: materialise the
        # columns it reads (one pdr_gather_add window per segment) and run the layer on plain sources
        def dense(sg):
            return Seg(act.first.materialise(sg.off, sg.C), 0, sg.C, _pad4(sg.C)) if sg.gathered else sg
        plain_act = Act([dense(sg) for sg in act.segs], act.P, act.B, act.rpb, scale=act.scale, shift=act.shift,
                        add=act.add, add_ld=act.add_ld, radd=None if act.radd is None else dense(act.radd),
                        pre_relu=act.pre_relu, post_relu=act.post_relu)
        plain_act.ss_ld, plain_act.oadd = act.ss_ld, act.oadd
        li = plain_act.struct()
        rc = launch()
    _lib.check(rc, "fused_layer")
    return li


def _launch(lib, act, conv, Y, y_ptr, ldy, partial_ptr, rc0, partial_tpb=0, weighted=True):
    """One layer launch over `act` into Y: on split-f16 arithmetic where the forward in flight asks for it and a tile
    variant carries the layer, else the exact kernel; its walk direction is recorded for its consumers."""
    li = act.struct(partial_tpb, weighted)
    if not _launch_split(lib, act, conv, li, y_ptr, ldy, partial_ptr, rc0):
        li = _launch_exact(lib, act, conv, li, y_ptr, ldy, partial_ptr, rc0)
    _WALK[Y.data_ptr()] = li.walk_reverse


def _launch_twin(lib, act, conv, ldy, rc0, stats, twin_stats, partial, tpb):
    """The same layer over the per-query rows of a deduplicated block (first neighbour of every query): its rows stand
    for the K copies in the skipped tiles -- moments weighted by K there, 0 elsewhere.  -> (Yd, Stats.sub)."""
    dd, tw = act.dd, act.twin
    Yd = torch.empty((tw.P, ldy), dtype=torch.float32, device=conv.Wt.device)
    if twin_stats:
        # ... computed by that launch itself (pdr_layer_in_t.wrow0 / wmul) into the rows behind the tile subset's;
        # the fold skips the rows of the tiles the subset skipped (Stats.sub)
        _launch(lib, tw, conv, Yd, Yd.data_ptr(), ldy, _ptr(partial, dd.tpb * conv.Cout * 2), rc0, partial_tpb=tpb)
        return Yd, (dd.nvalid[0], dd.tpb)
    _launch(lib, tw, conv, Yd, Yd.data_ptr(), ldy, None, rc0, weighted=False)
    if stats:
        dd.moments(Yd, conv.Cout, rc0, partial)
    return Yd, None


def run_layer(act, conv, stats=False, relu_col0=None, extra_rows=0, out=None, fold=None, stats_into=None):
    """Y (P, Cout) = prologue(act) . Wt + bias -> LayerOut (Y, stats = Stats(partial or None, rows per cloud, subset)).
    extra_rows: zero rows appended to Y (the zero row of a gathered table); out = (tensor, col0): write into
    columns [col0, col0 + ldy') of an existing (P, ld) tensor instead of allocating.
    fold: a FoldReq -- the GroupNorm fold (pdr_gn_fold) of this layer's statistics is launched right behind it,
    LayerOut.folded = (scale, shift).
    stats_into = (partial, first row, rows per cloud): the statistics go to rows [b rows_per_cloud + first row + tile] of
    an existing partial tensor.
    A deduplicated activation (act.dd, act.twin) runs over its tile subset and over its per-query rows, as one paired
    launch or two (LayerOut.twin, LayerOut.dd); where the statistics rows of both go: _stats_rows."""
    lib = _lib.load()
    assert act.C == conv.Cin, (act.C, conv.Cin)
    assert act.dd is None or (out is None and not extra_rows)
    ldy = _ldy(conv.Cout)
    if out is not None:
        Y, ycol0 = out
        y_ptr, ldy = _ptr(Y, ycol0), Y.shape[1]
    else:
        Y = torch.empty((act.P + extra_rows, ldy), dtype=torch.float32, device=conv.Wt.device)
        if extra_rows:
            Y[act.P:].zero_()
        y_ptr = Y.data_ptr()
    stats = stats or fold is not None
    rc0 = conv.Cout if relu_col0 is None else relu_col0
    tpb, twin_stats = _stats_rows(lib, act, conv, stats)
    dd = act.dd if act.twin is not None else None
    lo = None
    if dd is not None and (twin_stats or not stats) and stats_into is None:
        lo = _launch_pair(lib, act, conv, Y, y_ptr, ldy, stats, rc0)
    if lo is None:
        partial, row0, ptpb = None, 0, 0
        if stats_into is not None:
            partial, row0, ptpb = stats_into
        elif stats:
            partial = torch.empty((act.B * tpb, conv.Cout, 2), dtype=torch.float32, device=Y.device)
            ptpb = tpb if act.dd is not None else 0
        _launch(lib, act, conv, Y, y_ptr, ldy, None if partial is None else _ptr(partial, row0 * conv.Cout * 2), rc0,
                partial_tpb=ptpb)
        Yd, sub = _launch_twin(lib, act, conv, ldy, rc0, stats, twin_stats, partial, tpb) if dd is not None else \
            (None, None)
        lo = LayerOut(Y, Stats(partial, tpb, sub), twin=Yd, dd=dd)
    if fold is not None:
        lo.folded = fold.launch(lo.stats, act.B)
    return lo


def materialize(act):
    # (a deduplicated activation holds uninitialised rows in its skipped tiles: only the layer kernels, which walk the
    # tile subset, may read it)
    assert act.dd is None, "materialize() of a deduplicated block's activation"
    lib = _lib.load()
    out = torch.empty((act.P, act.C), dtype=torch.float32, device=act.segs[0].t.device)
    li = act.struct()
    _lib.check(lib.pdr_apply_act(ctypes.byref(li), act.P, act.C, out.data_ptr(), act.C, _stream()), "apply_act")
    return out


class Norm:
    """MyGroupNorm / nn.GroupNorm parameters."""

    def __init__(self, mod):
        gn = mod.group_norm if isinstance(mod, MyGroupNorm) else mod
        self.G, self.Cn, self.eps = gn.num_groups, gn.num_channels, gn.eps
        self.gamma, self.beta = gn.weight.detach().contiguous(), gn.bias.detach().contiguous()

    def fold(self, parts, B, C, n):
        """parts: one or two Window (Stats.window; or their fields as plain tuples) covering C channels in order.
        Returns (scale, shift) of shape (B, C): GroupNorm folded to y = x * scale + shift."""
        lib = _lib.load()
        dev = self.gamma.device
        parts = [Window(*p) for p in parts]
        assert 1 <= len(parts) <= 2 and sum(p.C for p in parts) == C
        scale = torch.empty((B, C), dtype=torch.float32, device=dev)
        shift = torch.empty((B, C), dtype=torch.float32, device=dev)

        def window(w):
            return (_ptr(w.partial, 2 * w.col0), w.partial.shape[1], w.tpb, w.C, float(w.mult)) if w is not None else \
                (None, 0, 0, 0, 1.0)

        def sub(w):
            # statistics of a tile SUBSET (Stats.sub): (valid tiles per cloud, main tiles)
            return (w.sub[0].data_ptr(), w.sub[1]) if w is not None and w.sub is not None else (None, 0)
        a, b = parts[0], (parts[1] if len(parts) == 2 else None)
        _lib.check(lib.pdr_gn_fold(*window(a), *window(b), B, self.Cn, self.G, float(n), float(self.eps),
                                   self.gamma.data_ptr(), self.beta.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                   *sub(a), *sub(b), _stream()), "gn_fold")
        return scale, shift


def _split_shared_mlp(seq):
    """[(conv, Norm)] of a build_shared_mlp Sequential laid out conv -> GroupNorm -> ReLU (bn_first=False)."""
    mods = list(seq)
    if len(mods) % 3 != 0:
        raise NotImplementedError("fused path expects conv -> GroupNorm -> ReLU stages")
    layers = []
    for i in range(0, len(mods), 3):
        conv, norm, act = mods[i:i + 3]
        if not (isinstance(conv, nn.Conv2d) and isinstance(norm, MyGroupNorm) and isinstance(act, nn.ReLU)):
            raise NotImplementedError("fused path expects conv -> GroupNorm -> ReLU stages")
        layers.append((conv, Norm(norm)))
    return layers


class EmbeddingBank:
    """All fc / fc_condition / fc_second_condition Linear layers of the network evaluated as THREE
    GEMMs per step (one per embedding kind) instead of ~30 tiny ones."""

    def __init__(self):
        self.groups = {"t": [], "c": [], "c2": []}
        self.out = {}

    def register(self, kind, lin):
        self.groups[kind].append(lin)
        return (kind, len(self.groups[kind]) - 1)

    def pack(self):
        self.W, self.b, self.offs = {}, {}, {}
        for k, mods in self.groups.items():
            if mods:
                self.W[k] = torch.cat([m.weight.detach() for m in mods], 0).contiguous()
                self.b[k] = torch.cat([m.bias.detach() for m in mods], 0).contiguous()
                o, offs = 0, []
                for m in mods:
                    offs.append((o, m.weight.shape[0]))
                    o += m.weight.shape[0]
                self.offs[k] = offs

    def evaluate_kind(self, kind, src, static=False):
        """One embedding kind.  static=True: the result is written IN PLACE into the buffer of the previous call
        (same shape), so that a captured hipGraph -- which does not contain this GEMM -- keeps reading a valid
        address whose contents follow the batch.  On the GPU the GEMM is pdr_embed_linear (round 4: the condition /
        class embedding rows of a new batch ran through F.linear -> hipBLASLt, 2 x 820 us for B = 32 rows)."""
        if kind not in self.W:
            return
        W, b = self.W[kind], self.b[kind]
        old = self.out.get(kind)
        reuse = static and old is not None and old.shape == (src.shape[0], W.shape[0]) and old.device == src.device
        if NATIVE_EMBED and src.is_cuda and src.dtype == torch.float32 and src.dim() == 2 and W.shape[1] % 8 == 0:
            x = src if (src.is_contiguous() and src.data_ptr() % 16 == 0 and src.shape[1] % 4 == 0) else \
                src.contiguous().clone()
            out = old if reuse else torch.empty((x.shape[0], W.shape[0]), dtype=torch.float32, device=x.device)
            rc = _lib.load().pdr_embed_linear(x.data_ptr(), x.shape[1], None, 0, None, 0, W.data_ptr(), b.data_ptr(),
                                              x.shape[0], x.shape[1], W.shape[0], 0, out.data_ptr(), out.shape[1],
                                              _stream())
            if rc != _lib.PDR_EUNSUPPORTED:
                _lib.check(rc, "embed_linear")
                self.out[kind] = out
                return
        val = F.linear(src, W, b)
        if reuse:
            old.copy_(val)
        else:
            self.out[kind] = val

    def get(self, handle):
        """Injected (tensor, offset, ld) of the (B, C) block of `handle`."""
        if handle is None:
            return None
        k, i = handle
        o, n = self.offs[k][i]
        return Injected(self.out[k], o, self.out[k].shape[1])


class FusedMlp:
    """Mlp_plus_t_emb (+ optional extra 1x1 convs sharing its input) on Act descriptors."""

    def __init__(self, mlp, bank, extra_convs=(), cond_kind="c"):
        """cond_kind: which embedding the call site feeds to `fc_condition` ("c" = global feature;
        "c2" = class embedding, as PointnetKnnFPModule does for its mlp1)."""
        if mlp.first_conv_bool:
            raise NotImplementedError("first_conv (bn_first) networks use the unfused path")
        stages = _split_shared_mlp(mlp.first_mlp) + _split_shared_mlp(mlp.second_mlp)
        if mlp.rest_mlp is not None:
            stages += _split_shared_mlp(mlp.rest_mlp)
        self.norms = [n for _, n in stages]
        self.res_identity = mlp.res_connect_bool and mlp.res_connect is None
        res_conv = mlp.res_connect if (mlp.res_connect_bool and mlp.res_connect is not None) else None
        self.has_res = mlp.res_connect_bool
        first = [stages[0][0]] + ([res_conv] if res_conv is not None else []) + list(extra_convs)
        self.first = Conv(first)
        self.rest = [Conv([c]) for c, _ in stages[1:]]
        self.C1 = stages[0][0].weight.shape[0]
        self.Clast = stages[-1][0].weight.shape[0]
        self.res_col0 = self.C1 if res_conv is not None else None
        self.extra_col0 = self.C1 + (self.Clast if res_conv is not None else 0)
        # embedding injected AFTER stage i's ReLU: t after 0, condition after 1, second condition after last
        self.inject = {}
        if mlp.include_t:
            self.inject[0] = bank.register("t", mlp.fc)
        if mlp.include_condition:
            self.inject[1] = bank.register(cond_kind, mlp.fc_condition)
        if mlp.include_second_condition:
            last = len(stages) - 1
            assert last not in self.inject
            self.inject[last] = bank.register("c2", mlp.fc_second_condition)
        self._chain_sync = {}     # chain(): (B, device) -> the cluster counters of pdr_point_chain

    def __call__(self, x, bank, relu_stats_extra=True):
        """x: Act over the grouped input.  Returns (h Act [final activation incl. residual], first) where the FirstOut
        `first` holds the [first conv | res conv | extra convs] columns and their statistics."""
        relu0 = self.extra_col0 if relu_stats_extra else None
        lo = run_layer(x, self.first, relu_col0=relu0, fold=self.first_fold(x.rpb))
        first = FirstOut(Y=lo.Y, stats=lo.stats)
        return self.after_first(first, x.P, x.B, x.rpb, bank, x, folded=_ready(lo.folded))

    def chain(self, x, bank):
        """The whole MLP on per-point rows as ONE pdr_point_chain launch -> (P, Clast) tensor, or None when the shapes
        are outside that kernel (the caller then runs __call__ + materialize).  x: Act over plain row-major segments."""
        if not POINT_CHAINS or x.dd is not None or x.scale is not None or x.add is not None or x.radd is not None or \
                x.pre_relu or x.post_relu or x.oadd is not None or not 1 <= len(x.segs) <= 3 or \
                (self.has_res and self.res_col0 is None) or self.extra_col0 != self.first.Cout or \
                _PRECISION[0] != "f32" or len(self.norms) > 4:
            return None
        if any(sg.gathered or sg.div != 1 for sg in x.segs):
            return None
        lib = _lib.load()
        B, n = x.B, x.rpb
        ch = _lib.PointChain()
        ch.n_layers, ch.n_seg = len(self.norms), len(x.segs)
        for i, sg in enumerate(x.segs):
            ch.seg[i].ptr, ch.seg[i].C, ch.seg[i].ld = _ptr(sg.t, sg.off), sg.C, sg.ld
        convs = [self.first] + self.rest
        keep = []
        for i, (conv, norm) in enumerate(zip(convs, self.norms)):
            L = ch.layer[i]
            L.Wt, L.bias, L.ldw, L.Cin, L.Cout = conv.Wt.data_ptr(), conv.bias.data_ptr(), conv.ldw, conv.Cin, conv.Cout
            L.main_cols = self.C1 if i == 0 else conv.Cout
            L.gamma, L.beta, L.groups, L.Cn, L.eps = norm.gamma.data_ptr(), norm.beta.data_ptr(), norm.G, norm.Cn, norm.eps
            L.relu_pre, L.relu_post = 0, 1
            inj = bank.get(self.inject.get(i))
            if inj is not None:
                if inj.off % 4 != 0:
                    return None
                L.add, L.add_ld = _ptr(inj.t, inj.off), inj.ld
                keep.append(inj.t)
        ch.residual = 1 if self.res_col0 is not None else 0
        plan = (ctypes.c_long * 4)()
        if lib.pdr_point_chain_plan(ctypes.byref(ch), B, n, plan) != _lib.PDR_OK:
            return None
        dev = self.first.Wt.device
        out = torch.empty((B * n, self.Clast), dtype=torch.float32, device=dev)
        scratch = torch.empty((max(int(plan[1]), 4),), dtype=torch.float32, device=dev)
        # the cluster counters: zeroed once, left zero by every launch (one buffer per batch size of this block)
        sync = self._chain_sync.get((B, dev))
        if sync is None:
            sync = self._chain_sync[(B, dev)] = torch.zeros((int(plan[2]),), dtype=torch.int32, device=dev)
        ch.out, ch.ldo, ch.scratch, ch.sync = out.data_ptr(), out.shape[1], scratch.data_ptr(), sync.data_ptr()
        rc = lib.pdr_point_chain(ctypes.byref(ch), B, n, _stream())
        if rc == _lib.PDR_EUNSUPPORTED:
            return None
        _lib.check(rc, "point_chain")
        return out

    def first_fold(self, rpb):
        """Fold request of the GroupNorm behind the first conv (for whoever launches that conv)."""
        return FoldReq(self.norms[0], self.C1, rpb)

    def first_conv_args(self, rpb):
        """What a SplitFirstConv that stands for this MLP's first conv is called with: the residual conv's column
        window, the first GroupNorm's fold request and the column windows whose moments are read at all -- [0, C1) by
        first_fold / after_first, [extra_col0, Cout) as the `second` window of the attention's n1_fold
        (FusedAttention.__call__: key_col0 = extra_col0, C2 = the key conv's width).  The residual window between them
        enters the MLP as a row-wise add (cur.radd): no GroupNorm reads its moments."""
        windows = [(0, self.C1)]
        if self.first.Cout > self.extra_col0:
            windows.append((self.extra_col0, self.first.Cout - self.extra_col0))
        return dict(res=(self.res_col0, self.Clast) if self.res_col0 is not None else None, fold=self.first_fold(rpb),
                    windows=tuple(windows))

    def after_first(self, first, P, B, rpb, bank, x=None, folded=None):
        """Everything behind the first conv, given its output and statistics (`first`, a FirstOut) and, when whoever
        launched the first conv made or requested it, the fold of the first GroupNorm (`folded`: a thunk yielding
        (scale, shift), called here, on the stream that runs the rest of the MLP).  Returns (h, first)."""
        stats = first.stats
        cur = first.attach(Act([first.seg(0, self.C1)], P, B, rpb))
        folded = folded() if folded is not None else None
        for i, norm in enumerate(self.norms):
            C = cur.C
            scale, shift = folded if folded is not None else norm.fold([stats.window(0, C)], B, C, rpb)
            cur.scale, cur.shift, cur.post_relu = scale, shift, True
            inj = bank.get(self.inject.get(i))
            if inj is not None:
                cur.add, cur.add_ld = inj.t[:, inj.off:], inj.ld
            if i < len(self.rest):
                lo = run_layer(cur, self.rest[i], fold=FoldReq(self.norms[i + 1], self.rest[i].Cout, rpb))
                stats, folded = lo.stats, lo.folded
                cur = act_from(lo, self.rest[i].Cout, P, B, rpb)
        if self.has_res:
            if self.res_col0 is not None:
                cur.radd = first.seg(self.res_col0, self.Clast)
                first.attach(cur)
            else:
                if x is None or len(x.segs) != 1 or x.scale is not None or x.pre_relu or x.post_relu or \
                        x.add is not None:
                    raise NotImplementedError("identity residual over a composite input")
                cur.radd = x.segs[0]
        return cur, first


class FusedAttention:
    """AttentionModule on Act descriptors; the key conv is computed by the caller's first GEMM."""

    def __init__(self, att):
        if not att.transform_grouped_feat_out:
            raise NotImplementedError("attention without feat_out_conv")
        self.key_conv = att.grouped_feat_conv      # handed to FusedMlp(extra_convs=...)
        self.q = Conv([att.feat_conv])
        wc = list(att.weight_conv)
        if len(wc) != 6:
            raise NotImplementedError("attention score net without GroupNorm (attention_bn=False)")
        self.n1, self.w1, self.n2, self.w2 = Norm(wc[1]), Conv([wc[2]]), Norm(wc[4]), Conv([wc[5]])
        # conv([q.expand(K) | k]) = conv_k(k) + conv_q(q): the query half is evaluated once per QUERY
        # (K times fewer flops) and enters the per-position GEMM as an output-side broadcast add
        c1 = att.feat_conv.weight.shape[0]
        zero_b = torch.zeros_like(self.w1.bias)
        self.w1_q = _RawConv(self.w1.Wt[:c1], self.w1.bias, self.w1.Cout)
        self.w1_k = _RawConv(self.w1.Wt[c1:], zero_b, self.w1.Cout)
        fo = list(att.feat_out_conv)
        self.v = Conv([fo[0]])
        self.v_norm = Norm(fo[1]) if len(fo) > 1 and isinstance(fo[1], MyGroupNorm) else None
        self.v_relu = isinstance(fo[-1], nn.ReLU)
        self.C1, self.C2 = self.q.Cout, att.grouped_feat_conv.weight.shape[0]
        self.D = self.w2.Cout

    def values(self, h, B, npoint, K):
        """Value half (independent of the query features): value conv + its GroupNorm fold -> Values (V, scale, shift,
        twin); twin: the per-query value rows of a deduplicated block.  (Not the LayerOut: its statistics are done
        with.)"""
        lo = run_layer(h, self.v, fold=FoldReq(self.v_norm, self.D, npoint * K) if self.v_norm is not None else None)
        return Values(lo.Y, *(lo.folded or (None, None)), lo.twin)

    def query_conv(self, query, B, npoint):
        """The query conv and its statistics (the first launch of __call__), for callers that issue it ahead."""
        return run_layer(plain(query, B, npoint), self.q, stats=True, relu_col0=0)

    def __call__(self, query, first, key_col0, counts, B, npoint, K, values, sorted_q=None, query_rows=None,
                 q_ahead=None):
        """query: (B*npoint, Cq) tensor; key = columns [key_col0, key_col0 + C2) of the block's first conv `first` (a
        FirstOut: output + statistics);
        values: a thunk yielding the Values of self.values(h, ...), called where the pooling needs them: it launches
        the value half there, or joins the stream that runs it (_on_aux), or hands over what exists (_ready).
        q_ahead: a thunk of the same kinds yielding the LayerOut of query_conv when that conv was launched ahead.
        query_rows: int32 (B*npoint) -- `query` is in another row order than the block's positions (QUERIES_IN_PLACE:
        the original order of a block evaluated on sorted queries): position p's query is row query_rows[p / K]."""
        lib = _lib.load()
        P = B * npoint * K
        # GroupNorm over [q.expand(K) | key]: the q half's moments count K times, the key half's come from the first
        # conv's launch -- both folded at the end of the q conv's launch
        Ct = self.C1 + self.C2
        n1_fold = FoldReq(self.n1, self.C1, npoint * K, mult0=float(K),
                          second=first.stats.window(key_col0, self.C2))
        if q_ahead is not None:                      # the query conv was launched ahead (query_conv): join, then fold
            ql = q_ahead()
            s, t = n1_fold.launch(ql.stats, B)
        else:
            ql = run_layer(plain(query, B, npoint), self.q, relu_col0=0, fold=n1_fold)
            s, t = ql.folded
        q = ql.Y
        if SPLIT_QUERY_CONV and (K & (K - 1)) == 0:
            zq = Act([Seg(q, 0, self.C1, q.shape[1])], B * npoint, B, npoint, scale=s, shift=t, pre_relu=True)
            zq.ss_ld = Ct
            Z = run_layer(zq, self.w1_q).Y
            a = first.attach(Act([first.seg(key_col0, self.C2)], P, B, npoint * K, scale=s[:, self.C1:],
                                 shift=t[:, self.C1:], pre_relu=True))
            a.ss_ld = Ct
            a.oadd = (Z, K)
            if a.twin is not None:
                a.twin.oadd = (Z, 1)                 # per-query rows: one row per query of Z
            if query_rows is not None:               # Z is in the ORIGINAL query order: read through the row map
                a.oadd_rows = query_rows
                if a.twin is not None:
                    a.twin.oadd_rows = query_rows
            lo1 = run_layer(a, self.w1_k, relu_col0=0, fold=FoldReq(self.n2, self.w1.Cout, npoint * K))
        else:
            a = first.attach(Act([Seg(q, 0, self.C1, q.shape[1], K), first.seg(key_col0, self.C2)], P, B,
                                 npoint * K, scale=s, shift=t, pre_relu=True))
            lo1 = run_layer(a, self.w1, relu_col0=0, fold=FoldReq(self.n2, self.w1.Cout, npoint * K))
        S1, (s, t) = lo1.Y, lo1.folded
        mark("  blk:main_scores_ready", True)
        score_in = Act([Seg(S1, 0, self.w1.Cout, S1.shape[1])], P, B, npoint * K, scale=s, shift=t, pre_relu=True)
        dd = lo1.dd
        score_in.dd = dd                             # the pooled launch walks the block's tile subset
        # a block evaluated on sorted queries (SortedQueries): the pooled launch and the patch write every query's row
        # at its ORIGINAL place (out_rows); the unfused fallback below pools in sorted order and gathers back
        fused_pool = FUSE_SCORE_POOL and K in (8, 16, 32) and (npoint * K) % 32 == 0 and self.D % 4 == 0
        out_rows = sorted_q.perm_rows if (sorted_q is not None and dd is not None and fused_pool) else None
        V, vs, vt, Vtwin = values()                  # (the value half ran on another stream: this joins it)
        mark("  blk:joined", True)
        out = torch.empty((B * npoint, self.D), dtype=torch.float32, device=V.device)
        cptr = counts.data_ptr() if counts is not None else None
        vsp, vtp = (vs.data_ptr(), vt.data_ptr()) if vs is not None else (None, None)

        # queries of the skipped tiles: one unmasked neighbour, i.e. the pooled row is its activated value row --
        # written by the pooled launch itself (FUSED_PATCH; a pdr_patch_rows launch behind it before)
        patched = dd is not None and FUSED_PATCH and fused_pool and V.shape[1] % 4 == 0
        if patched:
            score_in.patch = (Vtwin, dd.row_w)

        def patch():
            if dd is not None and not patched:
                Vd = Vtwin
                _lib.check(lib.pdr_patch_rows(Vd.data_ptr(), Vd.shape[1], vsp, vtp, int(self.v_relu),
                                              dd.row_w.data_ptr(), B, npoint, self.D, out.data_ptr(), self.D,
                                              out_rows.data_ptr() if out_rows is not None else None, _stream()),
                           "patch_rows")
            if sorted_q is not None and out_rows is None:
                # sorted queries whose rows were not placed by a row map (whole evaluation, unfused pooling)
                return gather_rows(out.view(B, npoint, -1), sorted_q.inv).view(B * npoint, -1)
            return out
        if fused_pool:
            # last score conv + mask + softmax over K + weighted sum in ONE kernel: scores stay in the
            # MFMA accumulators
            li = score_in.struct()
            if out_rows is not None:
                li.out_rows = out_rows.data_ptr()     # sorted queries: pooled rows go back to their original places
            variant = lib.pdr_fused_layer_variant(npoint * K, self.D) \
                if _PRECISION[0] == "split_f16" and self.w2.Cin >= SPLIT_MIN_CIN else None
            if variant in SPLIT_VARIANTS:
                # score conv on split-f16 arithmetic too (128-column tiles; else the exact kernel below)
                img, nch = self.w2.f16x3_image([self.w2.Cin], 64 if variant == 8 else 128)
                rc = lib.pdr_fused_layer_pool_f16x3(ctypes.byref(li), P, self.w2.Cin, img.data_ptr(), nch,
                                                     self.w2.bias.data_ptr(), self.D, V.data_ptr(), V.shape[1], vsp, vtp,
                                                     int(self.v_relu), cptr, K, out.data_ptr(), self.D, _stream())
                if rc != _lib.PDR_EUNSUPPORTED:
                    _lib.check(rc, "fused_layer_pool_f16x3")
                    return patch()
            _lib.check(lib.pdr_fused_layer_pool(ctypes.byref(li), P, self.w2.Cin, self.w2.Wt.data_ptr(), self.w2.ldw,
                                                self.w2.bias.data_ptr(), self.D, V.data_ptr(), V.shape[1], vsp, vtp,
                                                int(self.v_relu), cptr, K, out.data_ptr(), self.D, _stream()),
                       "fused_layer_pool")
            return patch()
        scores = run_layer(score_in, self.w2).Y
        _lib.check(lib.pdr_attention_pool(scores.data_ptr(), scores.shape[1], V.data_ptr(), V.shape[1], vsp, vtp,
                                          int(self.v_relu), cptr, B, npoint, K, self.D, out.data_ptr(), _stream()),
                   "attention_pool")
        return patch()


class _RawConv:
    """Conv-like view over explicit (Wt, bias) tensors."""

    def __init__(self, Wt, bias, Cout):
        self.Wt, self.bias = Wt.contiguous(), bias.contiguous()
        self.Cin, self.ldw, self.Cout = Wt.shape[0], Wt.shape[1], Cout
        self.f16x3, self.pair_ok = {}, {}            # (as Conv's)

    f16x3_image = Conv.f16x3_image


class SplitFirstConv:
    """First 1x1 conv of a grouped block evaluated WITHOUT the grouped (P x Cin) tensor.

    The grouped input is a gather of per-point rows plus per-query terms and the conv is linear:
        ball:  conv([feat[a] | xyz[a]-c | xyz[a] | c])            = U[a] + V[j]
               U = [feat | xyz].[W_f ; W_rel+W_abs]  (n rows),  V = c.(W_ctr-W_rel) + bias  (m rows),
               empty ball (subset=False: neighbour := the query, zero feature): V0 = c.(W_abs+W_ctr) + bias
        kNN:   conv([feat[a] | d2 | w | y[a] | y[a]-x | x])        = U[a] + V[i] + d2 r1 + w r2
               U = [feat | y].[W_f ; W_abs+W_rel],  V = x.(W_x-W_rel) + bias,  r1 / r2 = the d2 / weight rows
    U and V are two small GEMMs over the n source / m query rows; pdr_gather_add then writes the
    (m K)-row result and its GroupNorm moments in one pass.  Saves 2 P Cin Cout flops and the grouped
    tensor; the result differs from the direct conv only by fp32 summation order."""

    def __init__(self, first, Cs, kind, with_abs=True, with_centre=True):
        Wt, bias, Cout, dev = first.Wt, first.bias, first.Cout, first.Wt.device
        self.Cout, self.ld = Cout, first.ldw
        self._tables = {}
        self._halves = {}                                  # _table_halves: Cm -> (late, early)
        zero3 = torch.zeros((3, first.ldw), device=dev)
        zb = torch.zeros_like(bias)
        pad_bias = torch.zeros(first.ldw, device=dev)
        pad_bias[:Cout] = bias
        W_f = Wt[:Cs]
        if kind == 'ball':
            W_rel = Wt[Cs:Cs + 3]
            o = Cs + 3
            W_abs = Wt[o:o + 3] if with_abs else zero3
            o += 3 if with_abs else 0
            W_ctr = Wt[o:o + 3] if with_centre else zero3
            self.U = _RawConv(torch.cat([W_f, W_rel + W_abs], 0), zb, Cout)
            self.V = _RawConv(W_ctr - W_rel, bias, Cout)
            self.V0 = _RawConv(W_abs + W_ctr, bias, Cout)
            # [V | V0] as ONE rank-3 product (one thin launch per block instead of two): columns [0, Cout) and
            # [ld, ld + Cout) of a 2 ld wide table, the padding columns have zero weights
            ld = _ldy(Cout)
            wcat = torch.zeros((3, 2 * ld), device=dev)
            bcat = torch.zeros(2 * ld, device=dev)
            wcat[:, :first.ldw], wcat[:, ld:ld + first.ldw] = self.V.Wt, self.V0.Wt
            bcat[:Cout], bcat[ld:ld + Cout] = bias, bias
            self.VV0 = _RawConv(wcat, bcat, 2 * ld)
            self.r1 = self.r2 = None
        else:
            # (4 floats of slack: consumers read these rows in 16-byte pieces up to a segment's 4-padded width)
            pad = torch.zeros(4, device=dev)
            self.r1, self.r2 = torch.cat([Wt[Cs], pad]).contiguous(), torch.cat([Wt[Cs + 1], pad]).contiguous()
            W_abs, W_rel, W_x = Wt[Cs + 2:Cs + 5], Wt[Cs + 5:Cs + 8], Wt[Cs + 8:Cs + 11]
            self.U = _RawConv(torch.cat([W_f, W_abs + W_rel], 0), zb, Cout)
            self.V = _RawConv(W_x - W_rel, bias, Cout)
            self.V0 = None

    def source_table(self, src_feats_cl, src_xyz):
        """U (B*n + 1, ld): the per-source-point half of the conv; its last row is all zero (read for empty
        balls).  Depends on the SOURCE cloud only, so callers whose source is static across reverse steps (the
        feature-transfer blocks read the retained condition features) compute it once per batch."""
        B, n, Cs = src_feats_cl.shape
        u_in = Act(feature_segments(src_feats_cl) + [Seg(xyz4(src_xyz), 0, 3, 4)], B * n, B, n)
        # the table lives in a buffer owned by this block (one per shape), zeroed ONCE: the GEMM rewrites rows
        # [0, B n) every call and nothing ever writes the trailing zero row, so no fill launch per step
        key = (B * n + 1, _ldy(self.U.Cout))
        buf = self._tables.get(key)
        if buf is None:
            buf = self._tables[key] = torch.zeros(key, dtype=torch.float32, device=src_xyz.device)
        run_layer(u_in, self.U, out=(buf, 0))
        return buf

    def _table_halves(self, Cm):
        """(late, early) convs of the per-source table split behind its first Cm input channels."""
        if Cm not in self._halves:
            zb = torch.zeros_like(self.U.bias)
            self._halves[Cm] = (_RawConv(self.U.Wt[:Cm], self.U.bias, self.U.Cout),
                                _RawConv(self.U.Wt[Cm:], zb, self.U.Cout))
        return self._halves[Cm]

    def source_table_early(self, Cm, early_feats_cl, src_xyz):
        """U_early (B n, ld) = [early features | xyz] . W[Cm:]: the part of source_table() that does not read the first
        Cm channels of the source features (SPLIT_SOURCE_TABLES)."""
        B, n, _ = early_feats_cl.shape
        u_in = Act(feature_segments(early_feats_cl) + [Seg(xyz4(src_xyz), 0, 3, 4)], B * n, B, n)
        return run_layer(u_in, self._table_halves(Cm)[1]).Y

    def source_table_late(self, late_feats_cl, part):
        """U = late features . W[:Cm] + U_early, into the block's table buffer (see source_table)."""
        B, n, Cm = late_feats_cl.shape
        key = (B * n + 1, _ldy(self.U.Cout))
        buf = self._tables.get(key)
        if buf is None:
            buf = self._tables[key] = torch.zeros(key, dtype=torch.float32, device=part.device)
        a = Act(feature_segments(late_feats_cl), B * n, B, n)
        a.oadd = (part, 1)
        run_layer(a, self._table_halves(Cm)[0], out=(buf, 0))
        return buf

    def query_tables(self, query_xyz, has_v0):
        """[V | V0] (B*m, ld or 2 ld): the per-QUERY half of the conv (coordinates and static weights only)."""
        B, m, _ = query_xyz.shape
        ld = _ldy(self.U.Cout)
        q_in = plain(xyz4(query_xyz).reshape(B * m, 4), B, m, C=3)
        V2 = torch.empty((B * m, 2 * ld if has_v0 else ld), dtype=torch.float32, device=query_xyz.device)
        if has_v0:
            run_layer(q_in, self.VV0, out=(V2, 0))
        else:
            run_layer(q_in, self.V, out=(V2, 0))
        return V2

    def __call__(self, src_feats_cl, src_xyz, query_xyz, idx32, counts, K, relu_col0, s1=None, s2=None,
                 virtual=False, res=None, U=None, V2=None, fold=None, dd=None, windows=None):
        """-> (first, folded).  first = a FirstOut with this conv's statistics: over the (B*m*K, ld) output, or with
        virtual=True in the form that consumers read as a gathered source (only the GroupNorm moments are computed
        here).  fold: FoldReq of the GroupNorm behind this conv; folded = a thunk launching that fold -> (scale, shift),
        None without request.
        windows: one or two (col0, cols) -- the only columns whose moments anyone reads (FusedMlp.first_conv_args).  A
        statistics-only pass (virtual, nothing written) then leaves the other columns of `partial` UNWRITTEN
        (MOMENT_WINDOWS).  Every reader of a virtual first conv's statistics stays inside the windows: Stats.window is
        called by FoldReq.launch (first_fold: [0, C1)), FusedMlp.after_first ([0, C1)) and FusedAttention.__call__
        (the key window [extra_col0, Cout)); Dedup.moments (TWIN_STATS = False) WRITES rows of `partial`, all columns,
        and reads none; _stats_rows / _launch_pair lay out the statistics of the layer launches BEHIND the first conv,
        not these; tools/kernel_roofline.py counts bytes from the arguments and does not read `partial`."""
        lib = _lib.load()
        B, n, Cs = src_feats_cl.shape
        m = query_xyz.shape[1]
        if U is None:
            U = self.source_table(src_feats_cl, src_xyz)
        ld = U.shape[1]
        has_v0 = counts is not None
        if V2 is None:
            V2 = self.query_tables(query_xyz, has_v0)
        assert V2.shape == (B * m, 2 * ld if has_v0 else ld)
        ldv = V2.shape[1]
        rpb = m * K
        tpb = (rpb + 127) // 128
        virtual = virtual and (s1 is None) == (s2 is None) and (K & (K - 1)) == 0 and 128 % K == 0 and \
            not (s1 is not None and has_v0)
        # deduplicated evaluation (dd, a Dedup plan): the virtual ball form with a gathered (or no) residual only
        if dd is not None and not (virtual and s1 is None and (res is None or res[1] <= GATHER_RES)):
            dd = None
        Y = None if virtual else torch.empty((B * rpb, ld), dtype=torch.float32, device=U.device)
        ptpb = dd.ptpb if dd is not None else tpb
        partial = torch.empty((B * ptpb, self.Cout, 2), dtype=torch.float32, device=U.device)
        cptr = counts.data_ptr() if has_v0 else None

        # the argument groups every gather entry point shares: the tables, the kNN terms, the shape
        tabs = (U.data_ptr(), ld, n, V2.data_ptr(), _ptr(V2, ld) if has_v0 else None, ldv)
        knn = (s1.data_ptr() if s1 is not None else None, self.r1.data_ptr() if s1 is not None else None,
               s2.data_ptr() if s2 is not None else None, self.r2.data_ptr() if s2 is not None else None)
        dims = (B, rpb, K, self.Cout)

        def gather(y, ldy, ycol0, ycols):
            """One pass over the block's rows: the moments of `windows` alone when nothing is written (MOMENT_WINDOWS),
            else -- or where the windows are not carried -- of the whole width, with the window [ycol0, + ycols) of the
            output written to y.  -> Yd, the first conv of every query's FIRST neighbour (B m rows: the per-query
            chain's input), of a deduplicated block; else None."""
            forms = [("gather_add", (y, ldy, partial.data_ptr(), relu_col0, ycol0, ycols))]
            if y is None and MOMENT_WINDOWS and windows:
                w0, w1 = windows[0], (windows[1] if len(windows) > 1 else (0, 0))
                forms.insert(0, ("gather_moments", (partial.data_ptr(), relu_col0, w0[0], w0[1], w1[0], w1[1])))
            Yd = torch.empty((B * m, ld), dtype=torch.float32, device=U.device) if dd is not None else None
            for name, out in forms:
                head = (*tabs, idx32.data_ptr(), cptr)
                if dd is None:
                    rc = getattr(lib, "pdr_" + name)(*head, *knn, *dims, *out, _stream())
                elif TWIN_STATS:
                    # Yd is written, with its weighted moments, by extra workgroups of the launch that walks the tile subset
                    name += "_tiles_twin"
                    rc = getattr(lib, "pdr_" + name)(*head, *dims, *out, dd.tile_valid.data_ptr(), ptpb, dd.idx0.data_ptr(),
                                                     Yd.data_ptr(), ld, dd.wrow0.data_ptr(), float(K), _stream())
                else:
                    name += "_tiles"
                    rc = getattr(lib, "pdr_" + name)(*head, *knn, *dims, *out, dd.tile_valid.data_ptr(), ptpb, _stream())
                if rc != _lib.PDR_EUNSUPPORTED:             # (windows off a float4 are not carried: the whole width)
                    break
            _lib.check(rc, name)
            if dd is not None and TWIN_STATS:
                sub[0] = (dd.nvalid[0], dd.tpb)
            elif dd is not None:
                _lib.check(lib.pdr_gather_add(*tabs, dd.idx0.data_ptr(), cptr, None, None, None, None, B, m, 1, self.Cout,
                                              Yd.data_ptr(), ld, None, relu_col0, 0, -1, _stream()), "gather_add")
                dd.moments(Yd, self.Cout, relu_col0, partial)
            return Yd

        # (a thunk: the fold is launched by whoever consumes it, i.e. on the stream that runs the rest of the MLP)
        sub = [None]                                   # set by gather: the statistics of a tile subset
        folded = (lambda: fold.launch(Stats(partial, ptpb, sub[0]), B)) if fold is not None else None

        if not virtual:
            gather(Y.data_ptr(), ld, 0, -1)
            return FirstOut(Y=Y, stats=Stats(partial, tpb)), folded
        # virtual: GroupNorm moments of every column, but only the residual columns (a row-wise add in their
        # consumer, which stays a plain read) are written -- one pass
        Yres = None
        if res is not None and res[1] <= GATHER_RES and (s1 is None or GATHER_RES_KNN):
            res = None                        # consumers gather the residual window like any other
            Yd = gather(None, ld, 0, -1)
        elif res is not None and res[0] % 4 == 0:
            Yres = torch.empty((B * rpb, _pad4(res[1])), dtype=torch.float32, device=U.device)
            Yd = gather(Yres.data_ptr(), Yres.shape[1], res[0], res[1])
        else:
            res = None
            Yd = gather(None, ld, 0, -1)
        def materialise(col0, C):
            """Columns [col0, col0 + C) of the conv output as a tensor (fallback of consumers that cannot gather)."""
            assert col0 % 4 == 0
            Yc = torch.empty((B * rpb, _pad4(C)), dtype=torch.float32, device=U.device)
            _lib.check(lib.pdr_gather_add(*tabs, idx32.data_ptr(), cptr, *knn, *dims, Yc.data_ptr(), Yc.shape[1], None,
                                          relu_col0, col0, C, _stream()), "gather_add")
            return Yc

        first = FirstOut(stats=Stats(partial, ptpb, sub[0]), U=U, V2=V2, ld=ld, has_v0=has_v0, idx=idx32,
                         counts=counts if has_v0 else None, K=K, nsrc=n, zrow=B * n, Yres=Yres,
                         res_col0=res[0] if res else 0, res_cols=res[1] if res else 0, s1=s1, s2=s2,
                         r1=self.r1 if s1 is not None else None, r2=self.r2 if s1 is not None else None,
                         materialise=materialise)
        if dd is not None:
            first.dd, first.deg = dd, Yd
        return first, folded


def group_build(feats_cl, xyz, new_xyz, idx, counts, patch_empty, with_abs, with_centre):
    B, n, Cs = feats_cl.shape
    _, m, K = idx.shape
    Cout = Cs + 3 + (3 if with_abs else 0) + (3 if with_centre else 0)
    out = torch.empty((B * m * K, _pad4(Cout)), dtype=torch.float32, device=feats_cl.device)
    _lib.check(_lib.load().pdr_group_build(feats_cl.data_ptr(), Cs, xyz.data_ptr(), new_xyz.data_ptr(),
                                           idx.data_ptr(), counts.data_ptr(), B, n, m, K, int(patch_empty),
                                           int(with_abs), int(with_centre), out.data_ptr(), out.shape[1],
                                           _stream()), "group_build")
    return out, Cout


class Cat:
    """[a | b] along the channel axis of two (B, n, C) channel-last tensors, NOT materialised: the layer kernels
    read a concatenation as separate input segments and pdr_gather_rows2 gathers its rows directly, so the
    `torch.cat` launches of the reference composition (8 per step) disappear.  dense() builds it where a consumer
    needs one tensor."""

    def __init__(self, a, b):
        assert a.shape[:2] == b.shape[:2]
        self.parts = (a, b)
        self.shape = (a.shape[0], a.shape[1], a.shape[2] + b.shape[2])
        self.device = a.device
        self._dense = None

    def dense(self):
        if self._dense is None:
            self._dense = torch.cat(self.parts, dim=2)
        return self._dense


def feature_segments(feats_cl):
    """Input segments of a (B, n, C) feature tensor or a Cat of two."""
    parts = feats_cl.parts if isinstance(feats_cl, Cat) else (feats_cl,)
    return [Seg(xyz4(t), 0, t.shape[2], _pad4(t.shape[2])) for t in parts]


def gather_rows(src_cl, idx):
    if isinstance(src_cl, Cat):
        a, b = src_cl.parts
        B, n, C = src_cl.shape
        m = idx.shape[1]
        out = torch.empty((B, m, C), dtype=torch.float32, device=a.device)
        _lib.check(_lib.load().pdr_gather_rows2(a.data_ptr(), a.shape[2], b.data_ptr(), b.shape[2], idx.data_ptr(), B, n,
                                                m, out.data_ptr(), _stream()), "gather_rows2")
        return out
    B, n, C = src_cl.shape
    m = idx.shape[1]
    out = torch.empty((B, m, C), dtype=torch.float32, device=src_cl.device)
    _lib.check(_lib.load().pdr_gather_rows(src_cl.data_ptr(), idx.data_ptr(), B, n, C, m, out.data_ptr(),
                                           _stream()), "gather_rows")
    return out


class FusedGroupedBlock:
    """ball-query grouping -> Mlp_plus_t_emb -> attention pooling (SA body and feature transfer)."""

    def __init__(self, grouper, mlp, att, bank):
        if grouper.neighbor_def != 'radius' or not grouper.use_xyz:
            raise NotImplementedError("fused path: radius neighbourhoods with xyz channels")
        self.radius, self.nsample = grouper.radius, grouper.nsample
        self.with_abs, self.with_centre = grouper.include_abs_coordinate, grouper.include_center_coordinate
        self.att = FusedAttention(att)
        self.mlp = FusedMlp(mlp, bank, extra_convs=[self.att.key_conv])
        self.split = None   # built lazily (needs the source feature width)
        self.static_U = None
        self.dedup = False  # evaluate one-point neighbourhoods once (set for the x_t branch, see Dedup)
        self._t128 = {}     # _tiles_128: rows per cloud -> bool

    _WS_ON = []

    @staticmethod
    def _ws_kernels_on():
        """Tile subsets are walked by the wave-specialised layer kernels only (PDR_FUSED_WS=0 turns them off)."""
        if not FusedGroupedBlock._WS_ON:
            li = _lib.LayerIn()
            li.n_seg = 1
            li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = 0x1000, 64, 64, 1     # (never dereferenced)
            li.rows_per_batch = 8192
            plan = (ctypes.c_int * 8)()
            rc = _lib.load().pdr_fused_layer_plan(ctypes.byref(li), 8192, 64, 0x1000, 64, 64, 0x1000, 64, plan)
            FusedGroupedBlock._WS_ON.append(rc == 0 and plan[0] == 1)
        return FusedGroupedBlock._WS_ON[0]

    def _tiles_128(self, rpb):
        """Every per-neighbour layer of this block runs on 128-row tiles (the granularity of a plan)."""
        if rpb not in self._t128:
            tr = _lib.load().pdr_fused_layer_tile_rows
            couts = [c.Cout for c in self.mlp.rest] + [self.att.v.Cout, self.att.w1.Cout, self.att.w2.Cout]
            self._t128[rpb] = all(tr(rpb, c) == 128 for c in couts)
        return self._t128[rpb]

    def _plan(self, idx, counts, B, m, K, sq=None):
        """The Dedup plan of this block's (sorted) neighbourhoods -- `idx` = the sorted index rows of `sq`, the
        SortedQueries plan_ahead made on the geometry stream (shared by the encoder / decoder feature-transfer blocks
        of a level) --, or None when the block runs whole."""
        if not self._eligible(idx, m, K):
            return None
        # (only ever the plan of SORTED queries: the weighted statistics and the fold's skipped range rely on a cloud's
        # valid tiles being its first ones -- an index tensor that did not pass plan_ahead runs whole)
        return sq.plan if (sq is not None and sq.idx is idx) else None

    def _shape_ok(self, idx, m, K):
        """This block COULD evaluate its one-point neighbourhoods once (whatever the switches say)."""
        return (self.dedup and USE_SPLIT_FIRST and USE_VIRTUAL_FIRST and SPLIT_QUERY_CONV and
                K in (8, 16, 32) and m >= DEDUP_MIN_QUERIES and (m * K) % 128 == 0 and idx.dtype == torch.int32 and
                self._ws_kernels_on() and self._tiles_128(m * K))

    def _eligible(self, idx, m, K):
        return _dedup_on() and self._shape_ok(idx, m, K)

    def _sorted(self, idx):
        """The SortedQueries made for this index tensor, when this block evaluates its queries in that order."""
        e = _geom(idx)
        return e.sorted if (e is not None and _dedup_on() and self.dedup) else None

    def plan_ahead(self, neigh, new_xyz):
        """On the CURRENT stream (the one that produced `neigh`), ahead of the block: the query order and the plan --
        or, in a forward that evaluates every neighbourhood, only the probe count of what a plan would walk."""
        idx, counts = neigh
        B, m, K = idx.shape
        e = _geom(idx, create=True)
        if self._eligible(idx, m, K):
            if e.sorted is None:
                e.sorted = SortedQueries(idx, counts, new_xyz)      # (with the plan of the sorted arrays)
        elif _PROBE[0] is not None and self._shape_ok(idx, m, K) and not e.probed:
            _lib.check(_lib.load().pdr_dedup_probe(counts.data_ptr(), B, m, K, _probe_ptr(), _stream()), "dedup_probe")
            e.probed = True
        return neigh

    def side_tables(self, neigh, new_xyz, has_v0):
        """Per-query tables of the first conv, for the query order the block will use -> QueryTables."""
        sq = self._sorted(neigh[0])
        return QueryTables(self.split.query_tables(sq.xyz if sq is not None else new_xyz, has_v0=has_v0), sq)

    def _make_split(self, Cs):
        if self.split is None:
            self.split = SplitFirstConv(self.mlp.first, Cs, 'ball', self.with_abs, self.with_centre)
        return self.split

    @staticmethod
    def _in_place(K):
        """Sorted queries: the query features stay in their original order (the split query conv reads them there)."""
        return QUERIES_IN_PLACE and SPLIT_QUERY_CONV and K in (32, 64)     # (one query per 32-row block: oadd_rows)

    def prepare_static_source(self, src_xyz, src_feats_cl):
        """The source cloud of this block does not change between reverse steps (retained condition features):
        evaluate its per-source table once per batch, in place when a captured graph already reads the buffer."""
        if not USE_SPLIT_FIRST:
            return
        U = self._make_split(src_feats_cl.shape[2]).source_table(src_feats_cl, src_xyz)
        if self.static_U is U:
            pass                      # the block's own table buffer (rewritten in place by source_table)
        elif self.static_U is not None and self.static_U.shape == U.shape:
            self.static_U.copy_(U)
        else:
            self.static_U = U

    def neighbours(self, src_xyz, new_xyz):
        return _ext.ball_query(new_xyz, src_xyz, self.radius, self.nsample)

    @staticmethod
    def _ordered(query_feats_cl, sq, rows):
        """The query features as the attention reads them: gathered into the block's sorted order unless it reads them
        through the row map `rows`."""
        return gather_rows(query_feats_cl, sq.perm) if (sq is not None and rows is None) else query_feats_cl

    def _head(self, src_xyz, src_feats_cl, new_xyz, subset, neigh, tables, U=None, query=None, q_ahead=None):
        """The block up to and including its first conv (USE_SPLIT_FIRST) -> Head: the neighbours, the switch to the
        sorted query order, the per-query tables `tables` (a QueryTables) if they were made for that order -- else the
        first conv evaluates them --, the first conv's statistics pass.  query: the block's query features, when the
        caller has them already: put into the block's order here, ahead of the first conv, and their query conv goes
        ahead on the second stream unless `q_ahead` (made on the ORIGINAL query order) still serves."""
        B, m, _ = new_xyz.shape
        K = self.nsample
        idx, counts = neigh if neigh is not None else self.neighbours(src_xyz, new_xyz)
        sq, rows = self._sorted(idx), None
        if sq is not None:                     # the block's queries in sorted order (the pooling puts the output back)
            idx, counts, new_xyz = sq.idx, sq.counts, sq.xyz
            rows = sq.perm_rows if self._in_place(K) else None
        if query is not None:
            query = self._ordered(query, sq, rows)
            if q_ahead is not None and not (sq is None or rows is not None):
                q_ahead = None                 # (made on the original order, but this block gathered its queries)
            if q_ahead is None and QUERY_CONV_AHEAD and SPLIT_QUERY_CONV:
                qf = query.reshape(B * m, -1)
                q_ahead = _on_aux(lambda: self.att.query_conv(qf, B, m))
        first, folded = self._make_split(src_feats_cl.shape[2])(
            src_feats_cl, src_xyz, new_xyz, idx, None if subset else counts, K, self.mlp.extra_col0,
            virtual=USE_VIRTUAL_FIRST, U=U if U is not None else self.static_U,
            V2=tables.V2 if (tables is not None and tables.order is sq) else None,
            dd=self._plan(idx, counts, B, m, K, sq), **self.mlp.first_conv_args(m * K))
        return Head(B, m, K, counts, first, folded, sq, rows, query, q_ahead)

    def _values(self, hd, bank):
        """The half that does not involve the query features, behind the head: shared MLP + value half -> Values."""
        h, _ = self.mlp.after_first(hd.first, hd.B * hd.m * hd.K, hd.B, hd.m * hd.K, bank, folded=hd.folded)
        return self.att.values(h, hd.B, hd.m, hd.K)

    def _pool(self, hd, query_feats_cl, values, q_ahead=None):
        """The query / score / pooling half -> (B, m, D), rows in the original query order (see FusedAttention)."""
        out = self.att(query_feats_cl.reshape(hd.B * hd.m, -1), hd.first, self.mlp.extra_col0, hd.counts, hd.B, hd.m,
                       hd.K, values, sorted_q=hd.sq, query_rows=hd.rows, q_ahead=q_ahead)
        return out.view(hd.B, hd.m, -1)

    def prepare(self, src_xyz, src_feats_cl, new_xyz, bank, subset, neigh=None, V2=None):
        """Everything that does not involve the QUERY features: grouping, the shared MLP and the value half of the
        attention -> Prepared.  For the feature-transfer blocks this depends on coordinates and static tables only, so
        it can run ahead of the feature path on another stream."""
        if USE_SPLIT_FIRST:
            hd = self._head(src_xyz, src_feats_cl, new_xyz, subset, neigh, V2)
            return Prepared(hd, _ready(self._values(hd, bank)))
        B, m, _ = new_xyz.shape
        idx, counts = neigh if neigh is not None else self.neighbours(src_xyz, new_xyz)
        K = self.nsample
        dense_feats = src_feats_cl.dense() if isinstance(src_feats_cl, Cat) else src_feats_cl
        G, Cg = group_build(dense_feats, src_xyz, new_xyz, idx, counts, not subset, self.with_abs, self.with_centre)
        h, first = self.mlp(plain(G, B, m * K, C=Cg), bank)
        return Prepared(Head(B, m, K, counts, first), _ready(self.att.values(h, B, m, K)))

    def finish(self, prep, query_feats_cl):
        hd = prep.head
        return self._pool(hd, self._ordered(query_feats_cl, hd.sq, hd.rows), prep.values)

    def __call__(self, src_xyz, src_feats_cl, new_xyz, query_feats_cl, bank, subset, neigh=None, V2=None, U=None,
                 q_ahead=None):
        """V2: the QueryTables made ahead for this block, if any.  U: the per-source table of the first conv
        (SplitFirstConv.source_table) when the caller made it ahead of time -- it needs the source cloud only, not the
        queries.  q_ahead: a thunk yielding the attention's query conv when the caller launched it ahead
        (FusedAttention.query_conv on the ORIGINAL query order: QUERIES_IN_PLACE)."""
        if not (USE_SPLIT_FIRST and _PAR["stream"] is not None):
            return self.finish(self.prepare(src_xyz, src_feats_cl, new_xyz, bank, subset, neigh, V2=V2),
                               query_feats_cl)
        # first conv here, then [MLP + value conv] on the auxiliary stream beside [query / score convs]
        hd = self._head(src_xyz, src_feats_cl, new_xyz, subset, neigh, V2, U, query_feats_cl, q_ahead)
        mark("  blk:first_conv_stats_done", True)

        def value_half():
            mark("  blk:aux_begin", True)
            r = self._values(hd, bank)
            mark("  blk:aux_values_done", True)
            return r
        out = self._pool(hd, hd.query, _on_aux(value_half), hd.q_ahead)
        mark("  blk:pool_done", True)
        return out


class FusedKnnFP:
    def __init__(self, fp, bank):
        if fp.include_grouper or not fp.use_attention_module:
            raise NotImplementedError("fused path: kNN-FP with attention and without grouper")
        self.K = fp.K
        self.att = FusedAttention(fp.attention_module)
        # mlp1's fc_condition is fed the SECOND condition (class) embedding (pointnet2_modules.py:791-793)
        self.mlp1 = FusedMlp(fp.mlp1, bank, extra_convs=[self.att.key_conv], cond_kind="c2")
        self.mlp2 = FusedMlp(fp.mlp2, bank)
        self.split = None

    def _make_split(self, C):
        if self.split is None:
            self.split = SplitFirstConv(self.mlp1.first, C, 'knn')
        return self.split

    def __call__(self, unknown, known, unknown_feats_cl, known_feats_cl, bank, knn=None, V2=None, U=None):
        lib = _lib.load()
        B, n, _ = unknown.shape
        n2, C = known.shape[1], known_feats_cl.shape[2]
        K = self.K
        # squared distances, int32 neighbour indices and group_knn's normalised 1/(d2+1e-8) weights from ONE
        # native call (normally issued by the geometry prepass on the side stream)
        d2, idx, wgt = knn if knn is not None else _ext.knn_group(unknown, known, K)
        q_ahead = None
        if USE_SPLIT_FIRST and QUERY_CONV_AHEAD and SPLIT_QUERY_CONV:
            qf = unknown_feats_cl.reshape(B * n, -1)
            q_ahead = _on_aux(lambda: self.att.query_conv(qf, B, n))
        if USE_SPLIT_FIRST:
            first, folded = self._make_split(C)(
                known_feats_cl, known, unknown, idx, None, K, self.mlp1.extra_col0, s1=d2, s2=wgt,
                V2=V2.V2 if V2 is not None else None, U=U, virtual=USE_VIRTUAL_FIRST and USE_VIRTUAL_KNN,
                **self.mlp1.first_conv_args(n * K))

            def mlp():
                return self.mlp1.after_first(first, B * n * K, B, n * K, bank, folded=folded)[0]
            if _PAR["stream"] is not None:
                values = _on_aux(lambda: self.att.values(mlp(), B, n, K))
            else:
                h = mlp()
                values = lambda: self.att.values(h, B, n, K)        # (one stream: launched where the pooling needs it)
        else:
            G = torch.empty((B * n * K, _pad4(C + 11)), dtype=torch.float32, device=unknown.device)
            idx64 = idx.long()
            known_dense = known_feats_cl.dense() if isinstance(known_feats_cl, Cat) else known_feats_cl
            _lib.check(lib.pdr_knn_build(known_dense.data_ptr(), C, unknown.data_ptr(), known.data_ptr(),
                                         idx64.data_ptr(), d2.data_ptr(), B, n, n2, K, G.data_ptr(), G.shape[1],
                                         _stream()), "knn_build")
            h, first = self.mlp1(plain(G, B, n * K, C=C + 11), bank)
            values = lambda: self.att.values(h, B, n, K)
        interp = self.att(unknown_feats_cl.reshape(B * n, -1), first, self.mlp1.extra_col0, None, B, n, K, values,
                          q_ahead=q_ahead)
        Cs = unknown_feats_cl.shape[2]
        x2 = Act([Seg(interp, 0, self.att.D, interp.shape[1]), Seg(xyz4(unknown_feats_cl), 0, Cs, _pad4(Cs)),
                  Seg(xyz4(unknown), 0, 3, 4)], B * n, B, n)
        out = self.mlp2.chain(x2, bank)                # one launch for the <= 256-point levels (POINT_CHAINS)
        if out is None:
            h2, _ = self.mlp2(x2, bank, relu_stats_extra=False)
            out = materialize(h2)
        return out.view(B, n, -1)


def act_colmax(act):
    """(B, C) = max over every batch element's rows of the lazily-activated `act` (pdr_act_colmax)."""
    assert act.dd is None, "act_colmax() of a deduplicated block's activation"
    out = torch.empty((act.B, act.C), dtype=torch.float32, device=act.segs[0].t.device)
    li = act.struct()
    _lib.check(_lib.load().pdr_act_colmax(ctypes.byref(li), act.P, act.C, out.data_ptr(), _stream()), "act_colmax")
    return out


class FusedPnet2Stage:
    """Pnet2Stage (models/pnet.py; reference pnet.py:7-40) -- the global PointNet that summarises the condition cloud
    once per batch -- on the fused layer kernels: per-point MLP (conv -> GroupNorm -> ReLU, twice), max over the
    points, [feature | global].expand -> MLP -> max.  Round 3 ran it through torch Conv2d -> MIOpen (naive_conv /
    miopen rows in the first-step profile).  The concatenation with the broadcast global vector is never built: the
    second stage reads the first stage's output twice -- once with its GroupNorm folded in, once with scale 0 -- and
    the global vector enters as the per-batch `add` row of the second read."""

    def __init__(self, pnet):
        def stages(mlp):
            if mlp.first_conv_bool or mlp.include_t or mlp.include_condition or mlp.include_second_condition or \
                    mlp.res_connect_bool or mlp.rest_mlp is not None:
                raise NotImplementedError("fused Pnet2Stage: plain two-layer MLPs")
            out = []
            for seq in (mlp.first_mlp, mlp.second_mlp):
                mods = list(seq)
                if not isinstance(mods[0], nn.Conv2d):
                    raise NotImplementedError("fused Pnet2Stage: conv -> GroupNorm -> ReLU stages")
                if len(mods) == 1:
                    out.append((Conv([mods[0]]), None))                     # remove_last_activation: conv only
                elif len(mods) == 3 and isinstance(mods[1], MyGroupNorm) and isinstance(mods[2], nn.ReLU):
                    out.append((Conv([mods[0]]), Norm(mods[1])))
                else:
                    raise NotImplementedError("fused Pnet2Stage: conv -> GroupNorm -> ReLU stages")
            return out
        self.s1, self.s2 = stages(pnet.mlp1), stages(pnet.mlp2)
        if self.s1[0][1] is None or self.s2[0][1] is None:
            raise NotImplementedError("fused Pnet2Stage: the first layer of a stage is normalised")

    @staticmethod
    def _mlp(x, stages, B, n):
        """x: Act -> Act of the stage's output (its last GroupNorm + ReLU folded in lazily, if it has one)."""
        (c1, n1), (c2, n2) = stages
        lo = run_layer(x, c1, fold=FoldReq(n1, c1.Cout, n))
        a1 = act_from(lo, c1.Cout, B * n, B, n, scale=lo.folded[0], shift=lo.folded[1], post_relu=True)
        if n2 is None:
            return act_from(run_layer(a1, c2), c2.Cout, B * n, B, n)
        lo = run_layer(a1, c2, fold=FoldReq(n2, c2.Cout, n))
        return act_from(lo, c2.Cout, B * n, B, n, scale=lo.folded[0], shift=lo.folded[1], post_relu=True)

    def __call__(self, g_in):
        """g_in (B, n, Cin) channel-last -> (B, C_out) global feature."""
        B, n, _ = g_in.shape
        x = Act(feature_segments(g_in), B * n, B, n)
        f = self._mlp(x, self.s1, B, n)
        g = act_colmax(f)                                                   # (B, C1)
        C1 = f.C
        Y, ld = f.segs[0].t, f.segs[0].ld
        dev = g.device
        one = torch.ones((B, C1), device=dev) if f.scale is None else f.scale
        zero = torch.zeros((B, C1), device=dev)
        # [f | g.expand(n)]: the second half = rows of ZEROS + the `add` row g.  The zeros are a small buffer read as a
        # neighbour-broadcast segment (one row per d positions, d = the largest power of two dividing both the cloud and
        # the tile height); round 4 read Y a second time at scale 0, which turned an inf in Y into NaN where the
        # reference's concatenation holds a finite g -- kept only for clouds no power of two > 1 divides
        tm = _lib.load().pdr_fused_layer_tile_rows(n, self.s2[0][0].Cout)
        d = 1
        while d * 2 <= tm and n % (d * 2) == 0 and tm % (d * 2) == 0:
            d *= 2
        if d > 1 and C1 % 4 == 0:
            second, s_second = Seg(torch.zeros((B * n // d, C1), device=dev), 0, C1, C1, d), one
        else:
            second, s_second = Seg(Y, 0, C1, ld), zero
        both = Act([Seg(Y, 0, C1, ld), second], B * n, B, n,
                   scale=torch.cat([one, s_second], 1).contiguous(),
                   shift=torch.cat([zero if f.shift is None else f.shift, zero], 1).contiguous(),
                   add=torch.cat([zero, g], 1).contiguous(), add_ld=2 * C1, post_relu=f.post_relu)
        return act_colmax(self._mlp(both, self.s2, B, n))


class FusedCloudConditionNet:
    """Cached-condition forward of PointNet2CloudCondition through the fused kernels."""

    def __init__(self, net, precision="f32"):
        """precision: "f32" (default; every GEMM on the exact fp32 MFMA) or "split_f16" (opt-in: GEMMs with
        Cin >= 64 split both operands into f16 hi + lo parts and run 3 f16 MFMAs with fp32 accumulation: fp32-class
        products -- eps within 1.2e-5 of the exact network -- for operands of ordinary magnitude, see
        include/pdr_hip.h pdr_fused_layer_f16x3)."""
        hp = net.hparams
        if precision == "split_bf16":
            # the name of rounds 1-2; the halves are f16 since round 3 (same call sites, different range contract:
            # include/pdr_hip.h pdr_fused_layer_f16x3) -- accepted with a warning instead of breaking callers
            import warnings
            warnings.warn("precision='split_bf16' is a deprecated alias of 'split_f16' (f16 hi + lo halves; see the "
                          "range contract in include/pdr_hip.h)", DeprecationWarning, stacklevel=2)
            precision = "split_f16"
        if precision not in ("f32", "split_f16"):
            raise ValueError("precision must be 'f32' or 'split_f16'")
        self.precision = precision
        if net.scale_factor != 1:
            raise NotImplementedError("fused path: scale_factor == 1 (coordinates are not rescaled here)")
        if not (net.include_local_feature and net.include_global_feature and hp['include_class_condition']
                and net.attach_position_to_input_feature and net.bn and not hp['bn_first']
                and net.network_activation == 'relu'):
            raise NotImplementedError("configuration outside the fused family (see module docstring)")
        self.net = net
        self.bank = EmbeddingBank()
        b = self.bank
        self.enc_map = [FusedGroupedBlock(m.mapper, m.mlp, m.attention_module, b) for m in net.encoder_feature_map]
        self.dec_map = [FusedGroupedBlock(m.mapper, m.mlp, m.attention_module, b) for m in net.decoder_feature_map]
        self.sa = []
        for sa in net.SA_modules:
            if len(sa.groupers) != 1 or not sa.use_attention_module:
                raise NotImplementedError("fused path: single-scale SA with attention")
            blk = FusedGroupedBlock(sa.groupers[0], sa.mlps[0], sa.attention_modules[0], b)
            blk.npoint = sa.npoint
            self.sa.append(blk)
        self.fp = [FusedKnnFP(fp, b) for fp in net.FP_modules]
        # the blocks of the x_t branch see noise-like clouds for most of a reverse process: their one-point
        # neighbourhoods are evaluated once (Dedup); the condition branch (a surface, once per batch) runs whole
        for blk in self.enc_map + self.dec_map + self.sa:
            blk.dedup = True
        # condition branch (evaluated once per batch): same block types, no embeddings (include_t / condition False)
        self.cond_sa = []
        for sa in net.SA_modules_condition:
            if len(sa.groupers) != 1 or not sa.use_attention_module:
                raise NotImplementedError("fused path: single-scale SA with attention")
            blk = FusedGroupedBlock(sa.groupers[0], sa.mlps[0], sa.attention_modules[0], b)
            blk.npoint = sa.npoint
            self.cond_sa.append(blk)
        self.cond_fp = [FusedKnnFP(fp, b) for fp in net.FP_modules_condition]
        head = list(net.fc_lyaer)
        if not (len(head) == 4 and isinstance(head[1], nn.GroupNorm) and isinstance(head[2], nn.ReLU)):
            raise NotImplementedError("fused path: Conv1d -> GroupNorm -> ReLU -> Conv1d head")
        self.head1, self.head_norm, self.head2 = Conv([head[0]]), Norm(head[1]), Conv([head[3]])
        b.pack()
        try:
            self.global_pnet = FusedPnet2Stage(net.global_pnet)
        except NotImplementedError:
            self.global_pnet = None              # (outside the fused family: the torch module computes it)
        self.enc_cl = self.dec_cl = None
        self._synced = False
        self._streams = {"side": None, "fps": None, "aux": None}     # created on first use (_stream_named)
        self.return_strided_eps = False
        self.two_streams = True       # the two halves of every block on two streams (False: profiling tools that want
        self._label_key = None        # every kernel alone on the chip)
        # One-point neighbourhoods evaluated once (DEDUP) in THIS network's forwards.  The samplers capture the step both
        # ways and switch per step (reverse_sampler.py); the refinement forward, whose input is a finished surface, turns
        # it off (generation.refine_completion).
        self.dedup = True
        # probe: int32[2] device counters a forward adds to -- [0] tiles the deduplicated step walks / would walk, [1]
        # tiles of its deduplicable blocks (pdr_dedup_prepare / pdr_dedup_probe); None = no probe launches
        self.probe = None
        # (table (T, W) of every block's fc(t_emb) rows for all step values of a schedule, int64 device step counter):
        # set by a sampler (build_step_table); the step's embedding chain is then ONE row lookup (pdr_embed_select)
        self.step_table = None

    def _stream_named(self, name):
        """The geometry ("side"), sampling ("fps") or block-halves ("aux") stream of this network."""
        if self._streams[name] is None:
            self._streams[name] = torch.cuda.Stream(device=next(self.net.parameters()).device)
        return self._streams[name]

    def sync_condition(self):
        """Channel-last copies of the retained condition features.  Called once per batch, after the
        first (unfused) step has filled the network's cache; buffers are reused in place so that a
        captured hipGraph keeps reading valid addresses."""
        net = self.net

        def convert(dst, src):
            if dst is not None and len(dst) == len(src) and all(d.shape == (f.shape[0], f.shape[2], f.shape[1])
                                                                for d, f in zip(dst, src)):
                for d, f in zip(dst, src):
                    d.copy_(f.transpose(1, 2))
                return dst
            return [f.transpose(1, 2).contiguous() for f in src]

        self.enc_cl = convert(self.enc_cl, net.encoder_cond_features)
        self.dec_cl = convert(self.dec_cl, net.decoder_cond_features)
        saved_precision = _PRECISION[0]
        _PRECISION[0] = self.precision
        # the feature-transfer blocks read these static clouds as their SOURCE: the per-source half of their
        # first conv (SplitFirstConv.source_table) is evaluated here, once per batch, not once per step
        with torch.no_grad():
            _new_forward()
            for i, blk in enumerate(self.enc_map):
                blk.prepare_static_source(net.l_uvw[i], self.enc_cl[i])
            for i, blk in enumerate(self.dec_map):
                blk.prepare_static_source(net.l_uvw[i], self.dec_cl[i])
            _XYZ4.clear()
            # fc_condition(global feature) of every block: one GEMM per BATCH (static buffer, see _embeddings)
            self.bank.evaluate_kind("c", net.global_feature, static=True)
        _PRECISION[0] = saved_precision
        self._synced = True

    def _condition_branch(self, condition):
        """Condition branch of a new batch (pointnet2_with_pcld_condition.py:360-369, 383-414 of the reference:
        global PointNet, SA_modules_condition, FP_modules_condition) through the fused blocks; fills the
        network's retained features in the REFERENCE layout, exactly what the layer-by-layer path retains."""
        net, bank = self.net, self.bank
        uvw = condition[:, :, 0:3].contiguous()
        cond0 = torch.cat([condition[:, :, 3:], uvw / net.scale_factor], dim=2).contiguous() \
            if condition.shape[2] > 3 else (uvw / net.scale_factor)
        raw = net.partial_in_fea_dim - 3 if net.attach_position_to_input_feature else net.partial_in_fea_dim
        g_in = torch.cat([uvw, condition[:, :, 3:3 + raw]], dim=2) if raw > 0 else uvw
        if self.global_pnet is not None and FUSE_GLOBAL_PNET:
            net.global_feature = self.global_pnet(g_in.contiguous())
        else:
            net.global_feature = net.global_pnet(g_in.transpose(1, 2)).detach().clone()
        l_uvw, l_cond = [uvw], [cond0]
        for i, sa in enumerate(self.cond_sa):
            sel = _ext.furthest_point_sampling(l_uvw[i], sa.npoint)
            l_uvw.append(gather_rows(l_uvw[i], sel))
            centre = gather_rows(l_cond[i], sel)
            l_cond.append(sa(l_uvw[i], l_cond[i], l_uvw[i + 1], centre, bank, subset=True))
        net.l_uvw = l_uvw
        net.encoder_cond_features = [f.transpose(1, 2).contiguous() for f in l_cond]
        for i in range(-1, -(len(self.cond_fp) + 1), -1):
            l_cond[i - 1] = self.cond_fp[i](l_uvw[i - 1], l_uvw[i], l_cond[i - 1], l_cond[i], bank)
        net.decoder_cond_features = [f.transpose(1, 2).contiguous() for f in l_cond]
        self._synced = False

    @torch.no_grad()
    def forward(self, pointcloud, condition, ts=None, label=None, use_retained_condition_feature=False):
        """Same signature and default as PointNet2CloudCondition.forward (:276): without retention the condition
        branch is evaluated for this call only (the refinement stage); samplers pass True."""
        net, hp, bank = self.net, self.net.hparams, self.bank
        fresh = not use_retained_condition_feature or net.encoder_cond_features is None or \
            net.decoder_cond_features is None or net.global_feature is None
        if fresh:
            if not FUSE_CONDITION_BRANCH:
                # first step of a batch (condition branch not retained yet): reference-layout path.  This call does
                # not pass through _embeddings, so the class-embedding rows of the blocks are refreshed HERE: a
                # captured step (which contains no class-embedding GEMM) of a later batch would otherwise keep
                # reading the rows of the batch the graph was captured on
                out = net(pointcloud, condition, ts=ts, label=label,
                          use_retained_condition_feature=use_retained_condition_feature)
                if use_retained_condition_feature and label is not None:
                    self._refresh_class_embedding(label)
                return out
        saved = _PRECISION[0], _NET_DEDUP[0], _PROBE[0]
        _PRECISION[0], _NET_DEDUP[0], _PROBE[0] = self.precision, bool(self.dedup), self.probe
        saved_par = _PAR["stream"]
        _PAR["stream"] = self._stream_named("aux") if self.two_streams else None
        try:
            if fresh:
                _new_forward()
                self._condition_branch(condition)
            return self._forward_cached(pointcloud, condition, ts, label)
        finally:
            _PRECISION[0], _NET_DEDUP[0], _PROBE[0] = saved
            _PAR["stream"] = saved_par
            if not use_retained_condition_feature:
                self.reset_cond_features()

    def _embeddings(self, ts, label):
        """Step / condition / class embeddings of every block (EmbeddingBank).  Only the step embedding changes
        from step to step: the condition (global feature) GEMM is refreshed by sync_condition once per batch, the
        class-embedding GEMM when the label tensor changed (identity + version), both IN PLACE."""
        net, hp, bank = self.net, self.net.hparams, self.bank
        if ts is not None and hp['include_t']:
            if STEP_TABLE and self.step_table is not None and self._embed_select(ts.shape[0]):
                pass
            elif not (NATIVE_EMBED and ts.is_cuda and "t" in bank.W and self._embed_linear_chain(ts)):
                t_emb = net.activation(net.fc_t1(calc_t_emb(ts, hp['t_dim'])))
                t_emb = net.activation(net.fc_t2(t_emb))
                bank.evaluate_kind("t", t_emb)
        if self._label_key is None or self._label_key[0] is not label or self._label_key[1] != label._version \
                or "c2" not in bank.out:
            self._refresh_class_embedding(label)
        if "c" not in bank.out:
            bank.evaluate_kind("c", net.global_feature, static=True)

    def _refresh_class_embedding(self, label):
        """fc_second_condition(class_emb(label)) of every block, IN PLACE (a captured graph keeps its address);
        remembered by label identity + version."""
        with torch.no_grad():
            self.bank.evaluate_kind("c2", self.net.class_emb(label), static=True)
        # (the key holds the tensor itself: while it is referenced here its address cannot be recycled)
        self._label_key = (label, label._version)

    def build_step_table(self, ts_values):
        """Every block's fc(t_emb) rows for ALL the step values of a schedule ((T,) float32 tensor: entry i = the
        network time input while a sampler's device step counter reads i), through the same three pdr_embed_linear
        launches as a step's chain with T rows instead of B -- the chain depends on t only, a row's arithmetic does not
        depend on the rows beside it, so a looked-up row holds the bits the per-step chain would produce.  None when
        the shapes are outside the kernels' contract."""
        bank = self.bank
        if not (STEP_TABLE and NATIVE_EMBED and self.net.hparams['include_t'] and "t" in bank.W and ts_values.is_cuda):
            return None
        saved = bank.out.get("t")
        ok = self._embed_linear_chain(ts_values.float().contiguous())
        table = bank.out.get("t") if ok else None
        if saved is not None:
            bank.out["t"] = saved
        elif "t" in bank.out:
            del bank.out["t"]
        if table is None or table.shape[1] % 4 != 0:
            return None
        return table

    def _embed_select(self, B):
        """bank.out["t"] (B, W) <- row `step counter` of the step table (pdr_embed_select): the whole embedding chain
        of a step as one lookup launch."""
        table, t_dev = self.step_table
        out = torch.empty((B, table.shape[1]), dtype=torch.float32, device=table.device)
        rc = _lib.load().pdr_embed_select(table.data_ptr(), table.shape[1], table.shape[0], t_dev.data_ptr(), B,
                                          table.shape[1], out.data_ptr(), out.shape[1], _stream())
        if rc == _lib.PDR_EUNSUPPORTED:
            return False
        _lib.check(rc, "embed_select")
        self.bank.out["t"] = out
        return True

    def _embed_linear_chain(self, ts):
        """calc_t_emb -> fc_t1 -> swish -> fc_t2 -> swish -> every block's fc (pointnet2_with_pcld_condition.py
        :183-184, pointnet2_modules.py:113-120) through pdr_embed_linear; False when the shapes are outside the
        kernel's contract (caller runs the torch chain)."""
        net, bank, lib = self.net, self.bank, _lib.load()
        t_dim = net.hparams['t_dim']
        if t_dim % 8 != 0 or ts.dim() != 1:
            return False
        if ts.dtype != torch.float32:
            ts = ts.float()
        from .models.pointnet2_ssg_sem import _frequencies
        B, half = ts.shape[0], t_dim // 2
        freq = _frequencies(half, ts.device)
        dev = ts.device
        h1 = torch.empty((B, 4 * t_dim), dtype=torch.float32, device=dev)
        h2 = torch.empty((B, 4 * t_dim), dtype=torch.float32, device=dev)
        Wb, bb = bank.W["t"], bank.b["t"]
        out = torch.empty((B, Wb.shape[0]), dtype=torch.float32, device=dev)
        w1, w2 = net.fc_t1.weight, net.fc_t2.weight
        st = _stream()
        rc = lib.pdr_embed_linear(None, 0, ts.data_ptr(), ts.stride(0), freq.data_ptr(), half, w1.data_ptr(),
                                  net.fc_t1.bias.data_ptr(), B, t_dim, 4 * t_dim, 1, h1.data_ptr(), h1.shape[1], st)
        if rc == _lib.PDR_EUNSUPPORTED:
            return False
        _lib.check(rc, "embed_linear")
        _lib.check(lib.pdr_embed_linear(h1.data_ptr(), h1.shape[1], None, 0, None, 0, w2.data_ptr(),
                                        net.fc_t2.bias.data_ptr(), B, 4 * t_dim, 4 * t_dim, 1, h2.data_ptr(),
                                        h2.shape[1], st), "embed_linear")
        _lib.check(lib.pdr_embed_linear(h2.data_ptr(), h2.shape[1], None, 0, None, 0, Wb.data_ptr(), bb.data_ptr(), B,
                                        4 * t_dim, Wb.shape[0], 0, out.data_ptr(), out.shape[1], st), "embed_linear")
        bank.out["t"] = out
        return True

    def _forward_cached(self, pointcloud, condition, ts, label):
        net, hp, bank = self.net, self.net.hparams, self.bank
        B, N, _ = pointcloud.shape
        _new_forward()
        mark("step:begin")
        xyz = pointcloud[:, :, 0:3].contiguous()
        # scale_factor == 1 (checked at construction): xyz / 1 is xyz, bit for bit -- no division kernel, and the
        # 16-byte padded copy of the coordinates serves as the level-0 feature rows too
        feat0 = torch.cat([pointcloud[:, :, 3:], xyz], dim=2).contiguous() if pointcloud.shape[2] > 3 else xyz
        if not self._synced:
            self.sync_condition()
        enc_cl, dec_cl = self.enc_cl, self.dec_cl
        l_uvw = net.l_uvw

        # ---- geometry on two side streams ------------------------------------------------------------------------
        # The sampling chain (FPS + gather per level: a pure dependency chain on 32 of 256 CUs, 0.63 ms end to end), every
        # ball query with its plan, and every kNN search depend on coordinates only.  They run beside the GEMMs of the
        # blocks on streams of their own: `fps` carries the sampling chain from the step's first microsecond, `side` the
        # groupings, each waiting only for ITS level's sampling (one event per level, both ways).  All of it -- and the
        # hoisted decoder halves -- is issued ahead of the first block (FPS_STREAM above: the measured alternatives).
        # The encoder and decoder feature-transfer modules of one level query the SAME clouds with the same radius /
        # nsample (shipped configs): that ball query is computed once and shared.
        main = torch.cuda.current_stream()
        side = self._stream_named("side")
        # (both placements pay only while the blocks' launches are small -- one-point neighbourhoods evaluated once; with
        # every neighbourhood evaluated the main stream has no idle window and the sampling chain competes with full
        # kernels: same box, whole form, 9.33 / 9.34 ms per step with both, 8.78 without the level-0 hoist on the main
        # stream, 8.70 / 8.72 without either)
        fps_on = FPS_STREAM and _dedup_on()
        hoist0_main = HOIST_LEVEL0_ON_MAIN and _dedup_on()
        fps_s = self._stream_named("fps") if fps_on else side
        xyz4(xyz)                                   # (read by all three streams: produced ahead of the fork)
        side.wait_stream(main)
        fps_s.wait_stream(main)
        nlev = len(self.sa)
        l_xyz, sels, fm_neigh, sa_neigh, knn, tables = [xyz], [], {}, [None] * nlev, {}, {}
        ev_fps, ev_sa, ev_fm = [None] * nlev, [None] * nlev, {}
        side_tables_on = SIDE_TABLES and USE_SPLIT_FIRST

        def fm_key(i, blk):
            return (i % (nlev + 1), blk.radius, blk.nsample)

        def event(stream):
            ev = torch.cuda.Event()
            ev.record(stream)
            return ev

        def sample_level(i):
            """fps stream: level i -> i + 1 (FPS + row gather), its event."""
            with torch.cuda.stream(fps_s):
                sel = _ext.furthest_point_sampling(l_xyz[i], self.sa[i].npoint)
                sels.append(sel)
                l_xyz.append(gather_rows(l_xyz[i], sel))
                ev_fps[i] = event(fps_s)

        def transfer_level(lv, tables_for):
            """side stream: neighbourhoods + plan (+ per-query tables) of the feature-transfer blocks of level lv."""
            with torch.cuda.stream(side):
                for blk in ([self.enc_map[lv]] if lv < nlev else []) + [self.dec_map[lv]]:
                    if fm_key(lv, blk) not in fm_neigh:
                        fm_neigh[fm_key(lv, blk)] = blk.plan_ahead(blk.neighbours(l_uvw[lv], l_xyz[lv]), l_xyz[lv])
                    if side_tables_on and blk.split is not None and blk in tables_for:
                        tables[id(blk)] = blk.side_tables(fm_neigh[fm_key(lv, blk)], l_xyz[lv], True)
                ev_fm[lv] = event(side)

        def group_level(i):
            """side stream: SA block i's neighbourhoods + plan + tables (needs level i + 1 of the sampling chain)."""
            sa = self.sa[i]
            if not fps_on:
                sample_level(i)                 # (one geometry stream: the sampling right in front of its consumers)
            with torch.cuda.stream(side):
                if fps_on:
                    side.wait_event(ev_fps[i])
                sa_neigh[i] = sa.plan_ahead(sa.neighbours(l_xyz[i], l_xyz[i + 1]), l_xyz[i + 1])
                xyz4(l_xyz[i + 1])              # padded coordinates of the new level: produced before its event
                if side_tables_on and sa.split is not None:
                    tables[id(sa)] = sa.side_tables(sa_neigh[i], l_xyz[i + 1], False)
                ev_sa[i] = event(side)

        with torch.cuda.stream(fps_s):
            mark("fps:begin")
        if fps_on:
            sample_level(0)
        transfer_level(0, (self.enc_map[0], self.dec_map[0]) if hoist0_main else (self.enc_map[0],))
        with torch.cuda.stream(side):
            mark("side:first_ball_query_done")
        if fps_on:
            for i in range(1, nlev):
                sample_level(i)

        # ---- step embeddings (one row lookup inside a sampler's loop, else the three-launch chain)
        mark("main:before_embeddings", detail=True)
        self._embeddings(ts, label)
        mark("main:embeddings_done")
        ev_emb = event(main)

        def transfer(blk, l, cl, query, V2=None, q_ahead=None):
            prep = prepared.get(id(blk))
            if prep is not None:
                if prep.event is not None:
                    main.wait_event(prep.event)
                return blk.finish(prep, query)
            return blk(l_uvw[l], cl[l], l_xyz[l], query, bank, subset=False, neigh=fm_neigh[fm_key(l, blk)], V2=V2,
                       q_ahead=q_ahead)

        prepared = {}
        hoist = AHEAD_DECODER_MAPS and USE_SPLIT_FIRST and self.two_streams
        hoisted = [False]
        hoist_enc = AHEAD_ENCODER_MAPS and hoist and (_dedup_on() or AHEAD_ENCODER_MAPS_WHOLE)

        def hoist_map(blk, cl, l):
            """side stream: the query-independent half of a feature-transfer block of level l (first-conv statistics,
            shared MLP, value conv: coordinates, static condition features `cl` and embeddings only).  The decoder's
            blocks once the geometry is done; the encoder's right behind level l's neighbourhoods (see FPS_STREAM on
            when hoists pay)."""
            if tables.get(id(blk)) is None:
                # (no per-query tables made on the geometry stream: the block runs whole on the main stream)
                return
            with torch.cuda.stream(side):
                if not hoisted[0]:
                    side.wait_event(ev_emb)                 # the blocks' MLPs add the step / condition embeddings
                    hoisted[0] = True
                with _single_stream():
                    prep = blk.prepare(l_uvw[l], cl[l], l_xyz[l], bank, subset=False, neigh=fm_neigh[fm_key(l, blk)],
                                       V2=tables[id(blk)])
                prepared[id(blk)] = prep._replace(event=event(side))

        def geometry_tail():
            """side stream, behind the last level's groupings: the remaining per-query tables and the kNN searches (first
            used by the decoder)."""
            with torch.cuda.stream(side):
                mark("side:encoder_geometry_done")
                if side_tables_on:
                    if self.dec_map[0].split is not None and id(self.dec_map[0]) not in tables:
                        tables[id(self.dec_map[0])] = self.dec_map[0].side_tables(fm_neigh[fm_key(0, self.dec_map[0])],
                                                                                  l_xyz[0], True)
                    for i in range(-1, -(len(self.fp) + 1), -1):
                        fp = self.fp[i]
                        if fp.split is not None:
                            tables[id(fp)] = QueryTables(fp.split.query_tables(l_xyz[i - 1], has_v0=False))
                for i in range(-1, -(len(self.fp) + 1), -1):
                    knn[i] = _ext.knn_group(l_xyz[i - 1], l_xyz[i], self.fp[i].K)
                mark("side:knn_done")
                return event(side)

        # every remaining geometry launch and every hoisted half ahead of the first block (see FPS_STREAM above for why
        # not interleaved with the blocks)
        for k in range(nlev):
            group_level(k)
            lv = k + 1
            transfer_level(lv, (self.enc_map[lv],) if lv < nlev else (self.dec_map[lv],))
            if lv < nlev and hoist_enc:
                hoist_map(self.enc_map[lv], enc_cl, lv)
        if side_tables_on:
            # the decoder's transfer blocks of the inner levels share the encoder's neighbourhoods: their tables
            with torch.cuda.stream(side):
                for l in range(1, nlev):
                    blk = self.dec_map[l]
                    if blk.split is not None and id(blk) not in tables:
                        tables[id(blk)] = blk.side_tables(fm_neigh[fm_key(l, blk)], l_xyz[l], True)
        ev_knn = geometry_tail()
        if hoist:
            for l in range(nlev, 0 if hoist0_main else -1, -1):   # in the order the decoder will ask for them
                hoist_map(self.dec_map[l], dec_cl, l)

        def table_early(split, Cm, early_feats, src_xyz):
            """second stream, beside the feature-transfer block that is about to run on the main stream: the part of a
            block's per-source table that does not need that block's output (SPLIT_SOURCE_TABLES) -> (part, event)."""
            aux = _PAR["stream"]
            if not (SPLIT_SOURCE_TABLES and USE_SPLIT_FIRST and aux is not None) or early_feats.shape[2] % 4 != 0:
                return None
            aux.wait_event(event(main))
            with torch.cuda.stream(aux):
                part = split.source_table_early(Cm, early_feats, src_xyz)
                return part, event(aux)

        def table_late(split, pending, late_feats):
            if pending is None:
                return None
            main.wait_event(pending[1])
            return split.source_table_late(late_feats, pending[0])

        # ---- feature path ------------------------------------------------------------------------
        # (the first block's query conv reads x_t only: issued before the wait for the first neighbourhoods)
        q0 = None
        if QUERY_CONV_AHEAD and SPLIT_QUERY_CONV and QUERIES_IN_PLACE and USE_SPLIT_FIRST and _PAR["stream"] is not None:
            q0 = _ready(self.enc_map[0].att.query_conv(feat0.reshape(B * N, -1), B, N))
        main.wait_event(ev_fm[0])
        mark("main:after_wait_first_ball_query")
        l_feat = [feat0]
        for i, sa in enumerate(self.sa):
            if i > 0:
                main.wait_event(ev_fm[i])
            Cm = self.enc_map[i].att.D                    # width of the feature-transfer block's output
            pend = table_early(sa._make_split(Cm + l_feat[i].shape[2]), Cm, l_feat[i], l_xyz[i]) if i > 0 else None
            mapped = transfer(self.enc_map[i], i, enc_cl, l_feat[i], V2=tables.get(id(self.enc_map[i])),
                              q_ahead=q0 if i == 0 else None)
            mark("main:enc_map%d_done" % i)
            if i == 0 and hoist0_main and hoist and tables.get(id(self.dec_map[0])) is not None:
                with _single_stream():
                    prepared[id(self.dec_map[0])] = self.dec_map[0].prepare(
                        l_uvw[0], dec_cl[0], l_xyz[0], bank, subset=False, neigh=fm_neigh[fm_key(0, self.dec_map[0])],
                        V2=tables.get(id(self.dec_map[0])))
            sa_in = Cat(mapped, l_feat[i]) if USE_SPLIT_FIRST else torch.cat([mapped, l_feat[i]], dim=2)
            U_ahead = table_late(sa.split, pend, mapped)
            if i == 0 and SA0_TABLE_AHEAD and USE_SPLIT_FIRST and hoist0_main and _PAR["stream"] is not None:
                U_ahead = sa._make_split(sa_in.shape[2]).source_table(sa_in, l_xyz[i])
            main.wait_event(ev_sa[i])
            mark("main:after_wait_sa%d_geometry" % i)
            centre = gather_rows(sa_in, sels[i])
            l_feat.append(sa(l_xyz[i], sa_in, l_xyz[i + 1], centre, bank, subset=True, neigh=sa_neigh[i],
                             V2=tables.get(id(sa)), U=U_ahead))
            mark("main:sa%d_done" % i)
        main.wait_event(ev_knn)
        for i in range(-1, -(len(self.fp) + 1), -1):
            Cm = self.dec_map[i].att.D
            pend = table_early(self.fp[i]._make_split(Cm + l_feat[i].shape[2]), Cm, l_feat[i], l_xyz[i]) \
                if USE_SPLIT_FIRST else None
            mapped = transfer(self.dec_map[i], i % (nlev + 1), dec_cl, l_feat[i], V2=tables.get(id(self.dec_map[i])))
            fp_in = Cat(mapped, l_feat[i]) if USE_SPLIT_FIRST else torch.cat([mapped, l_feat[i]], dim=2)
            mark("main:dec_map%d_done" % (i % (nlev + 1)))
            l_feat[i - 1] = self.fp[i](l_xyz[i - 1], l_xyz[i], l_feat[i - 1], fp_in, bank, knn=knn[i],
                                       V2=tables.get(id(self.fp[i])), U=table_late(self.fp[i].split, pend, mapped))
            mark("main:fp%d_done" % (i % (nlev + 1)))
        mapped = transfer(self.dec_map[0], 0, dec_cl, l_feat[0], V2=tables.get(id(self.dec_map[0])))
        Cm, Cf = mapped.shape[2], l_feat[0].shape[2]
        head_in = Act([Seg(mapped, 0, Cm, Cm), Seg(l_feat[0], 0, Cf, Cf), Seg(xyz4(xyz), 0, 3, 4)], B * N, B, N)
        lo = run_layer(head_in, self.head1, fold=FoldReq(self.head_norm, self.head1.Cout, N))
        out = run_layer(act_from(lo, self.head1.Cout, B * N, B, N, scale=lo.folded[0], shift=lo.folded[1],
                                 post_relu=True), self.head2).Y
        mark("main:head_done")
        eps = out.view(B, N, out.shape[1])[:, :, :self.head2.Cout]
        # (B, N, Cout) view over the layer's 4-float rows; samplers consume it in place (pdr_reverse_update reads a
        # leading dimension), everybody else gets the dense tensor the module returns
        return eps if self.return_strided_eps else eps.contiguous()

    __call__ = forward

    # the sampler talks to the wrapped network for cache management
    def reset_cond_features(self):
        self.net.reset_cond_features()
        self._synced = False
        self._label_key = None          # a new batch: the class embedding rows are refreshed on first use

    def parameters(self):
        return self.net.parameters()
