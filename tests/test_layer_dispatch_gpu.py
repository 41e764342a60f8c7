"""pdr_fused_layer across its dispatch table on the GPU, against a float64 evaluation of include/pdr_hip.h.

For every case of tests/layer_cases.py under every option set: the launch returns what the plan returned (a refused
call writes nothing); every computed element of Y is within the worst-case fp32 bound 2 n u S of the float64 value
(n = Cin + 4, S = the sum of |terms| entering the element), so one wrong row, column, chunk or per-query term fails;
every written row of `partial` holds the moments of the kernel's own Y within 2 TM u sum|f|, row by row; everything
the call must not write keeps its NaN bits; and the launches the header promises to be byte-identical are.
"""
import ctypes

import pytest
import torch

from point_diffusion_refinement_amd import _lib
from tests import layer_cases as lc

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _buffers(L):
    c = L.case
    Y = torch.full((c.P, c.ldy), float("nan"), device=L.dev)
    part = torch.full((c.B * L.ptpb, c.Cout, 2), float("nan"), device=L.dev) if c.stats else None
    return Y, part


def _launch(L):
    c = L.case
    Y, part = _buffers(L)
    rc = _lib.load().pdr_fused_layer(ctypes.byref(L.li), c.P, c.Cin, L.ptr("Wt"), c.ldw, L.ptr("bias"), c.Cout,
                                     Y.data_ptr(), c.ldy, None if part is None else part.data_ptr(), c.relu_col0,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, Y, part


def _plan(L, Y):
    L.keep["Y"] = Y
    try:
        return L.plan()
    finally:
        del L.keep["Y"]


def _computed_rows(L):
    """(B, tpb) mask of the tiles the launch computes and (P,) mask of their rows."""
    c = L.case
    tiles = L.picked.view(c.B, L.tpb) if c.tile_list else torch.ones(c.B, L.tpb, dtype=torch.bool, device=L.dev)
    rows = tiles.repeat_interleave(L.tm, 1)[:, :c.rpb].reshape(c.P)
    return tiles, rows


def _check(L, rc_plan, rc, Y, part):
    c, what = L.case, L.case.label()
    assert rc == rc_plan, "%s: launch rc %d, plan rc %d" % (what, rc, rc_plan)
    if rc != _lib.PDR_OK:
        assert bool((_bits(Y) == NAN_BITS).all()), what + ": a refused call wrote Y"
        assert part is None or bool((_bits(part) == NAN_BITS).all()), what + ": a refused call wrote `partial`"
        return
    tiles, rows = _computed_rows(L)
    y = Y[:, :c.Cout]
    y64, S = lc.reference(L)
    err = (y.double() - y64).abs()
    bound = lc.y_bound(L, S)
    bad = ~(err <= bound) & rows[:, None]
    if bool(bad.any()):
        r, col = [int(v) for v in bad.nonzero()[0]]
        pytest.fail("%s: %d elements outside the bound; first at row %d (b %d, r %d) col %d: Y %r, float64 %r, "
                    "bound %.3g" % (what, int(bad.sum()), r, r // c.rpb, r % c.rpb, col, float(y[r, col]),
                                    float(y64[r, col]), float(bound[r, col])))
    # rows of tiles outside the list, padding columns beyond the 4-padded width: untouched
    assert bool((_bits(Y[~rows]) == NAN_BITS).all()), what + ": rows of unlisted tiles written"
    if c.ldy > lc.pad4(c.Cout):
        assert bool((_bits(Y[:, lc.pad4(c.Cout):]) == NAN_BITS).all()), what + ": padding columns written"
    if c.ldy % 4 or c.ldy < lc.pad4(c.Cout):
        assert bool((_bits(Y[:, c.Cout:]) == NAN_BITS).all()), what + ": columns beyond Cout written"
    if part is None:
        return
    ref, mag = lc.reference_stats(L, Y)
    pv = part.view(c.B, L.ptpb, c.Cout, 2)
    got = pv[:, :L.tpb]
    sbad = ~((got.double() - ref).abs() <= 2.0 * L.tm * lc.U * mag) & tiles[:, :, None, None]
    if bool(sbad.any()):
        b, t, col, k = [int(v) for v in sbad.nonzero()[0]]
        pytest.fail("%s: statistics row b %d tile %d col %d %s: %r vs float64 %r" % (
            what, b, t, col, ("sum", "sumsq")[k], float(got[b, t, col, k]), float(ref[b, t, col, k])))
    untouched = torch.ones(c.B, L.ptpb, dtype=torch.bool, device=L.dev)
    untouched[:, :L.tpb] = ~tiles
    assert bool((_bits(pv[untouched]) == NAN_BITS).all()), what + ": `partial` rows outside the written ones changed"


def _rerun_same(L, Y, part, what):
    rc, Y2, part2 = _launch(L)
    assert rc == _lib.PDR_OK
    assert _same(Y, Y2) and (part is None or _same(part, part2)), "%s: %s" % (L.case.label(), what)


def _run_case(case, dev, opt):
    L = lc.build(case, dev)
    Y0, _ = _buffers(L)
    rc_plan, out = _plan(L, Y0)
    rc, Y, part = _launch(L)
    _check(L, rc_plan, rc, Y, part)
    if rc != _lib.PDR_OK:
        return
    _rerun_same(L, Y, part, "two launches of the same case differ")
    if case.walk_reverse:
        L.li.walk_reverse = 0
        _rerun_same(L, Y, part, "walk_reverse 0 / 1 differ")
        L.li.walk_reverse = case.walk_reverse
    if opt.startswith("ws_xcd_order"):
        with lc.options({"ws_xcd_order": 1}):
            _rerun_same(L, Y, part, "ws_xcd_order %s / 1 differ" % opt[-1])
    if case.oadd and case.oadd_rows:
        # the same oadd gathered into order beforehand: the same bytes where the same kernel runs
        og = L.keep["oadd"][L.keep["oadd_rows"].long()].contiguous()
        L.keep["oadd_g"] = og
        L.li.oadd, L.li.oadd_rows = og.data_ptr(), None
        if _plan(L, Y0) == (rc_plan, out):
            _rerun_same(L, Y, part, "oadd_rows vs pre-gathered oadd differ")
    if case.pair:
        _run_pair(L, Y, part, dev)


def _run_pair(L, Y, part, dev):
    """pdr_fused_layer_pair against its two single launches: the same bytes in both outputs and both statistics."""
    L2 = lc.build(lc.pair_case(L.case), dev, weights=(L.keep["Wt"], L.keep.get("bias")))
    rc2, Y2, part2 = _launch(L2)
    Y20, _ = _buffers(L2)
    rcp, _ = _plan(L2, Y20)
    _check(L2, rcp, rc2, Y2, part2)
    c, c2 = L.case, L2.case
    Ya, pa = _buffers(L)
    Yb, pb = _buffers(L2)
    rc = _lib.load().pdr_fused_layer_pair(ctypes.byref(L.li), c.P, ctypes.byref(L2.li), c2.P, c.Cin, L.ptr("Wt"),
                                          c.ldw, L.ptr("bias"), c.Cout, Ya.data_ptr(), c.ldy, Yb.data_ptr(), c2.ldy,
                                          pa.data_ptr(), pb.data_ptr(), c.relu_col0,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.PDR_OK, c.label()
    assert _same(Ya, Y) and _same(pa, part), c.label() + ": paired launch, first problem"
    assert _same(Yb, Y2) and _same(pb, part2), c.label() + ": paired launch, second problem"


@pytest.mark.timeout(240)
@pytest.mark.parametrize("opt", list(lc.OPTION_SETS))
def test_layer_dispatch_table(cuda, opt):
    failures, cases = [], lc.targeted(opt) + lc.random_cases(opt, 30)
    with lc.options(lc.OPTION_SETS[opt]):
        for case in cases:
            try:
                _run_case(case, cuda, opt)
            except (AssertionError, pytest.fail.Exception) as e:     # every case reports; the test fails at the end
                failures.append(str(e).splitlines()[0])
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))


@pytest.mark.timeout(60)
@pytest.mark.parametrize("Cout", [32, 64])
def test_advisor_case_partial_tile_reads_the_mapped_query_row(cuda, Cout):
    """narrow_kc32 = 0, 384 rows per cloud (tile variant 0 / 1: a 256-row tile and a half tile), ball-gathered source
    with gK = 32, per-query term with oadd_div = 32 through a permuting oadd_rows: the half tile must add row
    oadd_rows[p / 32] of oadd, not row p / 32."""
    with lc.options({"narrow_kc32": 0}):
        _run_case(lc.advisor_case(Cout), cuda, "narrow_kc32=0")
