"""pdr_point_chain_plan over the point chain's dispatch table, host only, and the float64 reference of
tests/chain_cases.py checked against itself with planted faults (CPU tensors; nothing is launched).

Every reachable (rows per cloud, cluster size G, column tiles per wave CT, placement) cell must be reached with PDR_OK
by a targeted case, judged on the four longs the plan returns against the same numbers computed in chain_cases from
the header's rules: a case that quietly runs on another cluster size fails.  The refusals return the codes the header
gives them, from the plan and from the launch entry (which refuses on the host, before any launch).
"""
import ctypes

import pytest

from point_diffusion_refinement_amd import _lib
from tests import chain_cases as cc

OK, EI, EU = cc.OK, cc.EI, cc.EU


def test_plan_reaches_every_cell_and_refuses_what_the_header_refuses():
    targeted = cc.targeted()
    reached, refused = {}, {}
    for case in targeted + cc.random_cases(200):
        assert cc.want_rc_of(case) == case.want_rc, (case.label(), "the restated rules give", cc.want_rc_of(case))
        rc, plan = cc.build(case, None).plan()
        assert rc == case.want_rc, (case.label(), rc, plan)
        assert plan == cc.expected_plan(case), (case.label(), plan, cc.expected_plan(case))
        if case not in targeted:
            continue
        if rc == OK:
            assert case.B * plan[0] <= 256, case.label()
            reached.setdefault(cc.cell_of(case, plan[0]), []).append(case.label())
        elif case.tag.startswith("refused: "):
            refused[case.tag[len("refused: "):]] = rc
    missing = [c for c in cc.required_cells() if c not in reached]
    print("\n%d targeted cases, %d of %d cells reached, %d refusal lines hit" % (
        len(targeted), len(set(reached) & set(cc.required_cells())), len(cc.required_cells()), len(refused)))
    assert not missing, "dispatch cells no targeted case reaches: %s" % missing
    assert len(cc.required_cells()) == 72
    # at least one refusal from each line of the header's lists, with that line's code
    assert refused == {name: rc for name, (rc, _) in cc.DEFECTS.items()}
    eu = {k for k, v in refused.items() if v == EU}
    assert {"n=8", "n=48", "n=512", "B=257", "width 40", "wm+wres>128", "group straddles", "seg.ld%4", "ldw%4",
            "unaligned seg.ptr", "unaligned Wt", "unaligned bias", "unaligned add", "unaligned scratch"} <= eu
    assert {"n_layers=0", "n_layers=5", "n_seg=0", "n_seg=4", "B<0", "n<=0", "Cin mismatch", "main_cols!=Cout",
            "residual width", "gamma without beta", "Cn%groups", "Cn>main_cols", "add_ld<main_cols", "ldo<cols",
            "ldw<Cout", "seg.ld<roundup4(C)"} == set(refused) - eu


def test_random_cases_cover_accepted_and_refused():
    cases = cc.random_cases(200)
    assert cases == cc.random_cases(200)                                  # a seeded stream
    by_rc = {rc: sum(c.want_rc == rc for c in cases) for rc in (OK, EI, EU)}
    assert all(v >= 20 for v in by_rc.values()), by_rc
    assert all(c.B * c.n <= 8192 and c.B * cc.plan_G(c) <= 256 for c in cases if c.want_rc == OK)
    assert {c.n for c in cases if c.want_rc == OK} == set(cc.NS)


def test_every_feature_is_mixed_into_the_cells():
    """Layer and segment counts, partial chunks, paddings, residual blocks wider and narrower than layer 0's main
    block, changing widths, NULL gamma / bias / add, pass-through tails, the group sizes and the four ReLU pairs appear
    among the accepted targeted cases; the residency steps are planned and B = 64 / 256 launch."""
    cases = [c for c in cc.targeted() if c.want_rc == OK]
    assert {len(c.layers) for c in cases} == {1, 2, 3, 4}
    assert {len(c.segs) for c in cases} == {1, 2, 3}
    assert {3, 35, 40, 64, 259} <= {w for c in cases for w in c.segs}
    for field in ("seg_ld_extra", "ldw_extra", "ldo_extra", "add_ld_extra"):
        assert {getattr(c, field) > 0 for c in cases} == {False, True}, field
    assert any(c.add_ld_extra > 0 and any(s.has_add for s in c.layers) for c in cases)
    assert {c.residual for c in cases} == {False, True}
    assert any(c.residual and c.cols > c.layers[0].Cout for c in cases), "residual block wider than the main block"
    assert any(c.residual and c.cols < c.layers[0].Cout for c in cases), "residual block narrower than the main block"
    assert any(len({s.Cout for s in c.layers}) == 3 for c in cases), "widths that change along the chain"
    many = [c for c in cases if len(c.layers) >= 3]
    assert any(not c.layers[0].has_gn for c in many) and any(not c.layers[-1].has_gn for c in many)
    assert any(not s.has_gn for c in many for s in c.layers[1:-1])
    for field in ("has_gn", "has_bias", "has_add"):
        assert {getattr(s, field) for c in cases for s in c.layers} == {False, True}, field
    gn = [(c, s) for c in cases for s in c.layers if s.has_gn]
    assert any(s.Cn < s.Cout for _, s in gn), "a pass-through tail"
    assert {1, 8, 32} <= {s.groups for _, s in gn}
    assert any(s.Cn == s.groups for _, s in gn), "cpg = 1"
    assert any(cc.plan_G(c) < cc.plan_G(c, use_groups=False) for c in cases), "a cpg that forces a smaller cluster"
    assert {(s.relu_pre, s.relu_post) for _, s in gn} == {(False, False), (False, True), (True, False), (True, True)}
    # every n carries several layer counts, residual on and off, and a partial chunk
    for n in cc.NS:
        at = [c for c in cases if c.n == n]
        assert len({len(c.layers) for c in at}) >= 3 and {c.residual for c in at} == {False, True}, n
        assert any(C % 4 for c in at for C in c.segs) and any(not s.has_gn for c in at for s in c.layers), n
    res = {c.B: c for c in cases if c.tag == "residency"}
    assert sorted(res) == [32, 33, 64, 65, 128, 129, 256]
    assert [cc.plan_G(res[B]) for B in sorted(res)] == [4, 4, 4, 2, 2, 1, 1]
    assert sorted(B for B, c in res.items() if not c.plan_only) == [64, 256]
    net = [c for c in cases if c.tag == "network"]
    assert sorted((c.B, c.n, cc.plan_G(c)) for c in net) == [(32, 64, 8), (32, 256, 8), (40, 64, 4), (40, 256, 4)]


def test_argument_errors_through_both_entry_points():
    """Every refusal line through pdr_point_chain_plan and pdr_point_chain (refusing cases only: the launch entry
    returns on the host, nothing launches); NULL out / scratch / sync are argument errors of the launch entry."""
    lib = _lib.load()
    plan = (ctypes.c_long * 4)()
    assert cc.build(cc.BASE, None).plan()[0] == OK
    for name, (want, fn) in cc.DEFECTS.items():
        case = fn(cc.BASE)
        assert cc.want_rc_of(case) == want == cc.launch_rc_of(case) != OK, name
        P = cc.build(case, None)
        assert P.plan()[0] == want, name
        assert P.launch() == want, name
    for name, fn in cc.LAUNCH_DEFECTS.items():
        case = fn(cc.BASE)
        P = cc.build(case, None)
        assert P.plan()[0] == OK and cc.launch_rc_of(case) == EI, name
        assert P.launch() == EI, name
    one = cc.LAUNCH_DEFECTS["NULL out"](cc.ChainCase(B=2, n=64, segs=(64,), layers=(cc.L(64),)))
    assert cc.build(one, None).launch() == EI
    P = cc.build(cc.BASE, None)
    assert lib.pdr_point_chain_plan(None, 2, 64, plan) == EI and lib.pdr_point_chain(None, 2, 64, None) == EI
    assert lib.pdr_point_chain_plan(ctypes.byref(P.ch), 2, 64, None) == EI
    # an unaligned scratch is no obstacle to a single layer, which never reads it
    single = cc.ChainCase(B=2, n=64, segs=(64,), layers=(cc.L(64),), mutate="unaligned_scratch")
    assert cc.build(single, None).plan()[0] == OK


@pytest.fixture(scope="module")
def accepted():
    return [c for c in cc.targeted() if c.want_rc == OK and not c.plan_only]


def test_no_targeted_case_needs_a_bar_above_2e_5(accepted):
    """A case whose float32 evaluation is further than 5e-6 from float64 is ill-conditioned and is redrawn, not
    tolerated: the bar max(5e-6, 4 e32) stays at or below 2e-5 for every launched targeted case."""
    worst = max((cc.reference_and_bar(c)[2], c.label()) for c in accepted)
    print("\nlargest e32 of %d targeted cases: %.3g (%s)" % (len(accepted), worst[0], worst[1]))
    assert worst[0] <= 5e-6, worst


def test_planted_faults_leave_the_bar_by_more_than_ten_times(accepted):
    """Each planted fault of the reference moves the float64 result by more than 10 x the case's bar in EVERY accepted
    targeted case that exercises it (so a kernel with that fault fails that case)."""
    counted = dict.fromkeys(cc.FAULTS, 0)
    for case in accepted:
        want, bar, _ = cc.reference_and_bar(case)
        assert bool(want.isfinite().all()), case.label()
        for fault, exercised in cc.FAULTS.items():
            if not exercised(case):
                continue
            moved = cc.rel(cc.faulted(case, fault), want)
            assert moved > 10.0 * bar, "%s: fault %s moves the reference by %.3g, the bar is %.3g" % (
                case.label(), fault, moved, bar)
            counted[fault] += 1
    print("\ncases per planted fault: %s" % counted)
    assert all(v >= 5 for v in counted.values()), counted
