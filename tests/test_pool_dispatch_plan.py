"""pdr_fused_layer_pool_plan over the pooled dispatch table, host only, and the float64 reference of
tests/pool_cases.py checked against itself with planted faults (CPU tensors; nothing is launched).

Under each option set every cell of the table -- kernel form x tile variant x D x rows per cloud, the persistent-grid
cells and the tile subset / row map / patched rows cells -- must be reached with PDR_OK by a targeted case, judged on
the 8 ints the plan returns against the same tuple computed here from rows_per_batch, D, the options and the
features: a case that quietly runs on another kernel fails.  The refusals return the codes the header gives them.
"""
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from tests import pool_cases as pc

OPTS = list(pc.OPTION_SETS) + ["split"]


def _options(opt):
    return pc.options({} if opt == "split" else pc.OPTION_SETS[opt])


@pytest.mark.parametrize("opt", OPTS)
def test_plan_reaches_every_pooled_cell_and_refuses_what_the_launch_refuses(opt):
    opts = {} if opt == "split" else pc.OPTION_SETS[opt]
    reached = {}
    with _options(opt):
        targeted = pc.targeted(opt)
        for case in targeted + pc.random_cases(opt, 40):
            P = pc.build(case, None)
            rc, plan = P.plan()
            assert rc == case.want_rc, (case.label(), rc, plan)
            if rc != _lib.PDR_OK:
                assert plan == [-7] * 8, (case.label(), "a refusal wrote the plan")
                continue
            assert plan == pc.expected_plan(case, opts), (case.label(), plan, pc.expected_plan(case, opts))
            assert plan[1] == _lib.load().pdr_fused_layer_variant(case.rpb, case.D)
            if case in targeted:
                for cell in pc.cells_of(case, plan):
                    reached.setdefault(cell, []).append(case.label())
        refused = [c for c in targeted if c.want_rc != _lib.PDR_OK]
    assert refused, "no refusal under " + opt
    missing = [c for c in pc.required_cells(opt) if c not in reached]
    print("\n%s: %d targeted cases, %d cells reached, %d refusals" % (opt, len(targeted), len(reached), len(refused)))
    assert not missing, "%s: pooled dispatch cells no targeted case reaches: %s" % (opt, missing)


def test_every_k_and_feature_is_mixed_into_the_cells():
    """K in {8, 16, 32} in every (form, variant, D, rows) cell; every counts mode, v_relu 0 / 1, NULL vscale / vshift /
    bias, the three paddings of ldv and ldo, a D that is no multiple of 4, the prologue's parts and 1..4 segments with a
    partial 32-channel chunk appear among the accepted targeted cases of the default options."""
    cases = [c for c in pc.targeted("defaults") if c.want_rc == _lib.PDR_OK]
    by_cell = {}
    for c in cases:
        if not (c.tile_list or c.out_rows or c.patch) and "many" not in c.tag and "xcd" not in c.tag:
            by_cell.setdefault((c.D, c.rpb), set()).add(c.K)
    assert all(ks == {8, 16, 32} for ks in by_cell.values()), by_cell
    assert {c.counts for c in cases} == set(pc.COUNT_MODES)
    for field in ("v_relu", "vscale", "vshift", "bias", "pre", "post", "ss", "add"):
        assert {getattr(c, field) for c in cases} == {False, True}, field
    assert {c.ldv_extra for c in cases} == {0, 4, 36} == {c.ldo_extra for c in cases}
    assert any(c.D % 4 for c in cases) and any(c.ss and c.ss_extra for c in cases)
    assert {len(c.segs) for c in cases} == {1, 2, 3, 4}
    assert {33, 100, 259} <= {w for c in cases for w in c.segs}
    assert any(c.score_scale == 100.0 for c in cases)


def test_plan_argument_errors():
    import ctypes
    lib = _lib.load()
    P = pc.build(pc.PoolCase(B=2, rpb=128, segs=(64,), D=64), None)
    c = P.case
    args = [ctypes.byref(P.L.li), c.P, c.Cin, P.L.ptr("Wt"), 64, 64, P.ptr("values"), c.ldv, c.K, P.ptr("out"), c.ldo, 0]
    plan = (ctypes.c_int * 8)()
    assert lib.pdr_fused_layer_pool_plan(*args, plan) == _lib.PDR_OK and list(plan)[:5] == [1, 8, 0, 2, 1]
    assert lib.pdr_fused_layer_pool_plan(*args, None) == _lib.PDR_EINVAL
    for i, bad in ((0, None), (3, None), (3, P.L.ptr("Wt") + 4), (4, 62), (6, None), (7, 60), (9, None), (10, 60), (1, 0)):
        a = list(args)
        a[i] = bad
        assert lib.pdr_fused_layer_pool_plan(*a, plan) == _lib.PDR_EINVAL, (i, bad)


def _differs(a, b, bound):
    """Some element that both write differs by more than 10 x the bound, or the written rows differ."""
    wa, ba, ma = a
    wb, _, mb = b
    both = ma & mb
    far = (wa[both] - wb[both]).abs() > 10.0 * bound[both]
    return bool(far.any()) or not torch.equal(ma, mb)


@pytest.mark.parametrize("opt", OPTS)
def test_planted_faults_leave_the_bound_by_more_than_ten_times(opt):
    """Each planted fault of the reference differs from the true reference by more than 10 x the bound on at least one
    element in EVERY accepted targeted case that exercises the feature (so a kernel with that fault fails that case), and
    the true reference is finite wherever a row is written."""
    dev = torch.device("cpu")
    counted = dict.fromkeys(pc.FAULTS, 0)
    for case in pc.targeted(opt):
        if case.want_rc != _lib.PDR_OK or case.P > 20000:        # (the persistent-grid cases: the same code at B ~ 500)
            continue
        P = pc.build(case, dev)
        true = pc.expected(P)
        want, bound, written = true
        assert bool(torch.isfinite(want[written]).all()) and bool(torch.isfinite(bound[written]).all()), case.label()
        assert bool(written.any()), case.label()
        for fault, exercised in pc.FAULTS.items():
            if not exercised(case):
                continue
            assert _differs(pc.expected(P, fault), true, bound), "%s: fault %s stays within 10 x the bound" % (
                case.label(), fault)
            counted[fault] += 1
    need = set(pc.FAULTS) - ({"no_out_rows", "patch_listed"} if opt not in ("defaults", "split") else set())
    assert all(counted[f] > 0 for f in need), counted
