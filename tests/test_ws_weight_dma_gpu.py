"""The wave-specialised layer kernel's weight transport (csrc/fused_layer_ws.hip: W chunks go global -> LDS by DMA,
retired by a counted wait ahead of a raw barrier) at the smallest shapes at which it can go wrong.

Every case is a call of the public entry points judged as tests/test_layer_dispatch_gpu.py and
tests/test_pool_dispatch_gpu.py judge theirs: every element against a float64 torch evaluation within the worst-case
fp32 bound of tests/layer_cases.py (the derived pooled / split bound of tests/pool_cases.py), the statistics rows
against the kernel's own output, NaN-prefilled memory the call must not write, and a second launch of the same problem
into fresh outputs giving the same bytes.

Shapes: B = 2 clouds of 128 rows (one tile), 200 (a partial row tile: the general fetch path) and 384 (three tiles per
cloud: a persistent workgroup that owns more than one tile crosses tile boundaries with both stage parities -- the
chunk counts below are odd and even); Cin 32 (one full chunk), 41, 73, 171 (partial last chunks: the weight rows of
the chunk's tail are clamped on the SOURCE address; 2 to 6 chunks), 64 (two full chunks) and 41 + 32 (the first
segment ends in a partial chunk); Cout 32, 35, 64 (the 128 x 32 and 128 x 64 tiles: 2 and 4 DMA pieces per wave; 35:
the column clamp and `ldw` padding), 128, 140, 256 (128 x 128 tiles, grid.y > 1 at 256; 140 takes the 128 x 160 tile,
which has no wave-specialised form and runs the uniform-wave kernel: the table offers nothing else there).
"""
import ctypes

import pytest
import torch

from point_diffusion_refinement_amd import _lib
from tests import layer_cases as lc
from tests import pool_cases as pc
from tests import test_layer_dispatch_gpu as layer_run
from tests import test_pool_dispatch_gpu as pool_run

pytestmark = pytest.mark.gpu

RPBS = (128, 200, 384)
SEGS = ((32,), (41,), (64,), (73,), (171,), (41, 32))
COUTS = (32, 35, 64, 128, 140, 256)
# (variant, more than two chunks per tile) the wave-specialised kernel must have been reached on by the cases of a form:
# the 128 x 32, 128 x 64 and 128 x 128 tiles, each with a stage that is written a second time within one tile
WS_CELLS = {(v, deep) for v in (7, 8, 4) for deep in (False, True)}
# With default options the few-tile 128 x 128 launches of more than 64 input channels run the right-sized tiny-layer
# launch of the uniform-wave kernel (plan_layer, option deep_chunks); the option is off here so that these small shapes
# reach the kernel under test, as they do in the network at its row counts.
OPTS = {"deep_chunks": 0}


def _chunks(case):
    return sum((C + 31) // 32 for C in case.segs)


def _cases(form, pair=False):
    out = []
    for ri, rpb in enumerate(RPBS):
        for si, segs in enumerate(SEGS):
            for ci, Cout in enumerate(COUTS):
                i = ri + 3 * si + 5 * ci
                s = (sum(segs),) if form in ("residual", "ball_res", "knn_res") else segs
                # prologue features in turn; the per-query output term and weighted statistics are not the transport's
                out.append(lc.Case(B=2, rpb=rpb, segs=s, Cout=Cout, form=form, K=8, pre=bool(i & 1), post=bool(i & 2),
                                   ss=bool((i + 1) & 2), add=bool(i & 4), relu_col0=(0, min(16, Cout), Cout)[i % 3],
                                   ldy_extra=(0, 4)[i % 2], pair=pair, tile_list=pair, ptpb_extra=1 if pair else -1,
                                   seed=i, tag="w-dma"))
    return out


def _run_layer_cases(cases, dev):
    failures, cells = [], set()
    with lc.options(OPTS):
        for case in cases:
            try:
                L = lc.build(case, dev)
                rc, plan = L.plan()
                cell = lc.cell_of(L, rc, plan)
                if cell and cell[0] == "ws":
                    cells.add((cell[1], _chunks(case) > 2))
                layer_run._run_case(case, dev, "defaults")
            except (AssertionError, pytest.fail.Exception) as e:     # every case reports; the test fails at the end
                failures.append(str(e).splitlines()[0])
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))
    return cells


@pytest.mark.timeout(120)
@pytest.mark.parametrize("form", lc.FORMS)
def test_every_source_form(cuda, form):
    """plain, residual, ball-gathered, residual-gathered (ball / kNN) and kNN-gathered sources over rows x Cin x Cout."""
    cells = _run_layer_cases(_cases(form), cuda)
    assert WS_CELLS <= cells, "%s: wave-specialised variants reached: %s" % (form, sorted(cells))


def _launch_pair(L, L2):
    c, c2 = L.case, L2.case
    Ya, pa = layer_run._buffers(L)
    Yb, pb = layer_run._buffers(L2)
    rc = _lib.load().pdr_fused_layer_pair(ctypes.byref(L.li), c.P, ctypes.byref(L2.li), c2.P, c.Cin, L.ptr("Wt"),
                                          c.ldw, L.ptr("bias"), c.Cout, Ya.data_ptr(), c.ldy, Yb.data_ptr(), c2.ldy,
                                          pa.data_ptr(), pb.data_ptr(), c.relu_col0,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, Ya, pa, Yb, pb


@pytest.mark.timeout(120)
@pytest.mark.parametrize("form", ["plain", "ball"])
def test_paired_launch(cuda, form):
    """pdr_fused_layer_pair (a listed first problem, as the entry point asks; Cout 140 has no paired variant): BOTH
    problems of the one launch against float64, and two launches for the bytes.  (Not against the two single launches:
    alone, the second problem's few rows may run another kernel, with another summation order.)"""
    cases = [c for c in _cases(form, pair=True) if (c.rpb != 200 or form == "plain") and c.Cout != 140]
    failures, cells = [], set()
    with lc.options(OPTS):
        for case in cases:
            try:
                L = lc.build(case, cuda)
                L2 = lc.build(lc.pair_case(case), cuda, weights=(L.keep["Wt"], L.keep.get("bias")))
                rc_plan, plan = L.plan()
                cell = lc.cell_of(L, rc_plan, plan)
                assert cell and cell[0] == "pair", case.label() + ": no paired variant"
                cells.add((cell[1], _chunks(case) > 2))
                rc, Ya, pa, Yb, pb = _launch_pair(L, L2)
                layer_run._check(L, _lib.PDR_OK, rc, Ya, pa)
                layer_run._check(L2, _lib.PDR_OK, rc, Yb, pb)
                rc, Yc, pc_, Yd, pd = _launch_pair(L, L2)
                assert rc == _lib.PDR_OK and all(layer_run._same(a, b)
                                                 for a, b in ((Ya, Yc), (pa, pc_), (Yb, Yd), (pb, pd))), \
                    case.label() + ": two paired launches differ"
            except (AssertionError, pytest.fail.Exception) as e:
                failures.append(str(e).splitlines()[0])
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))
    assert WS_CELLS <= cells, "%s pair: variants reached: %s" % (form, sorted(cells))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("split", [False, True])
def test_pooled_epilogue_and_split_f16(cuda, split):
    """The pooled launch (K = 8) and, where the variant exists (64- and 128-column tiles), its split-f16 form: the
    packed weight image is copied linearly, [hi | lo] x columns x 64 bytes per chunk."""
    failures, worst, ws = [], {}, 0
    cases = []
    for rpb in (128, 384):                               # (pooled launches take whole row tiles only)
        for si, segs in enumerate(SEGS):
            for D in COUTS:
                if split and D in (32, 140):               # (128 x 32 and 128 x 160 tiles: no split-f16 form)
                    continue
                cases.append(pc.PoolCase(B=2, rpb=rpb, segs=segs, D=D, K=8, split=split, ss=bool(si & 1),
                                         post=bool(si & 2), seed=si + D, tag="w-dma"))
    for case in cases:
        try:
            P = pc.build(case, cuda)
            out = P.new_out()
            rc, plan = P.plan(out.data_ptr())
            ws += int(rc == _lib.PDR_OK and bool(plan[0]))
            pool_run._run_case(case, cuda, worst)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(str(e).splitlines()[0])
    for key, ratio in sorted(worst.items()):
        print("\nworst error / bound of %s on the %s kernel: %.4f" % (key[0], key[1], ratio))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))
    assert ws >= len(cases) // 2, "%d of %d cases on the wave-specialised kernel" % (ws, len(cases))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("form", lc.FORMS)
def test_split_f16_layer(cuda, form):
    """pdr_fused_layer_f16x3 (the packed weight image is copied linearly into LDS) on the variants that carry it -- the
    128 x 64 and 128 x 128 tiles -- against float64 at the bar of tests/test_fused_gpu.py::
    test_split_f16_layer_vs_float64: 2e-6 of the sum of magnitudes entering the element, + 1; statistics rows against
    the kernel's own output as in the exact kernel; two launches for the bytes."""
    from point_diffusion_refinement_amd.pointnet2.fused_network import pack_f16x3
    lib, failures, n = _lib.load(), [], 0
    for case in _cases(form):
        if case.Cout in (32, 140):
            continue
        L = lc.build(case, cuda)
        c = case
        variant = lib.pdr_fused_layer_variant(c.rpb, c.Cout)
        img, nch = pack_f16x3(L.keep["Wt"], c.Cout, c.segs, 64 if variant == 8 else 128)
        outs = []
        for _ in range(2):
            Y, part = layer_run._buffers(L)
            rc = lib.pdr_fused_layer_f16x3(ctypes.byref(L.li), c.P, c.Cin, img.data_ptr(), nch, L.ptr("bias"), c.Cout,
                                           Y.data_ptr(), c.ldy, part.data_ptr(), c.relu_col0,
                                           torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            outs.append((rc, Y, part))
        (rc, Y, part), what = outs[0], c.label()
        if rc == _lib.PDR_EUNSUPPORTED:                  # (a form the split variants do not carry at this shape)
            continue
        try:
            assert rc == _lib.PDR_OK and outs[1][0] == rc, "%s: rc %d" % (what, rc)
            n += 1
            y64, S = lc.reference(L)
            err = float(((Y[:, :c.Cout].double() - y64).abs() / (S + 1.0)).max())
            assert err < 2e-6, "%s: error %.3g of the magnitude sum" % (what, err)
            ref, mag = lc.reference_stats(L, Y)
            got = part.view(c.B, L.ptpb, c.Cout, 2)[:, :L.tpb]
            assert bool(((got.double() - ref).abs() <= 2.0 * L.tm * lc.U * mag).all()), what + ": statistics rows"
            assert layer_run._same(Y, outs[1][1]) and layer_run._same(part, outs[1][2]), what + ": two launches differ"
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), n, "\n".join(failures[:40]))
    assert n >= 3 * len(SEGS) * 4 // 2, "%d cases ran" % n
