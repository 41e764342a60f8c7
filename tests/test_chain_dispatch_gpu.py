"""pdr_point_chain across its dispatch table on the GPU, against the float64 reference and the measured bar of
tests/chain_cases.py.

For every case: `out` is NaN-prefilled with guard rows behind B n and guard columns in [cols, ldo); `scratch` is
NaN-prefilled before each launch, so a read before the producer's store shows as NaN; the first launch is within
max(5e-6, 4 e32) of float64 (e32: the same chain in float32 torch on the CPU), the second gives the same bytes; the
guards keep their NaN bits; `sync` is all zero afterwards, sync[2 B] included.

Safety, kept in this file's code: one chain launch in flight at a time (a synchronize follows every launch); every
launched case satisfies B G <= 256 (all workgroups resident); chain_cases.build makes device tensors for accepted,
aligned cases only; a non-zero sync[2 B] -- a workgroup gave up waiting -- fails the test at once through
`WorkgroupGaveUp`, which no collect-and-go-on handler catches, and nothing further is launched.
"""
import pytest
import torch

from tests import chain_cases as cc

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
_GAVE_UP = []                       # labels of the launches after which sync[2 B] was set: nothing launches after one


class WorkgroupGaveUp(Exception):
    """sync[2 B] != 0 after a launch: to be explained from the kernel's code, not retried."""


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(P):
    """One launch, alone on the device, and the state of the counters after it."""
    c = P.case
    assert cc.want_rc_of(c) == cc.OK and c.B * cc.plan_G(c) <= 256
    if _GAVE_UP:
        raise WorkgroupGaveUp("not launched: a workgroup gave up waiting in %s" % _GAVE_UP[0])
    torch.cuda.synchronize()
    rc = P.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == cc.OK, "%s: launch rc %d" % (c.label(), rc)
    sync = P.sync.tolist()
    if sync[2 * c.B] != 0:
        _GAVE_UP.append(c.label())
        raise WorkgroupGaveUp(c.label())
    assert sync == [0] * len(sync), c.label() + ": cluster counters not restored"


def _run_case(case, dev, launches=2):
    """-> (cell, error / bar, e32) of an accepted case."""
    what = case.label()
    P = cc.build(case, dev)
    rc, plan = P.plan()
    assert rc == cc.OK and plan == cc.expected_plan(case), "%s: plan rc %d %s" % (what, rc, plan)
    want, bar, e32 = cc.reference_and_bar(case)
    rows, cols = case.B * case.n, case.cols
    first = None
    for k in range(launches):
        P.out.fill_(float("nan"))
        P.scratch.fill_(float("nan"))
        _launch(P)
        assert bool((_bits(P.out[rows:]) == NAN_BITS).all()), what + ": rows behind B n written"
        assert bool((_bits(P.out[:, cols:]) == NAN_BITS).all()), what + ": columns in [cols, ldo) written"
        if k == 0:
            first = P.out[:rows, :cols].clone()
            got = first.double().cpu()
            assert bool(got.isfinite().all()), "%s: %d non-finite outputs" % (what, int((~got.isfinite()).sum()))
            err = cc.rel(got, want)
            assert err < bar, "%s: error %.3g, bar %.3g (e32 %.3g)" % (what, err, bar, e32)
        else:
            assert torch.equal(_bits(first), _bits(P.out[:rows, :cols])), what + ": two launches differ"
    return cc.cell_of(case, plan[0]), err / bar, e32


def _run_all(cases, dev, launches, what):
    failures, cells, worst, e32max = [], set(), 0.0, 0.0
    for case in cases:
        try:
            cell, ratio, e32 = _run_case(case, dev, launches)
        except (AssertionError, pytest.fail.Exception) as e:         # every case reports; the test fails at the end
            failures.append(str(e).splitlines()[0])                  # (WorkgroupGaveUp is not caught: stop at once)
            continue
        cells.add(cell)
        worst, e32max = max(worst, ratio), max(e32max, e32)
    print("\n%s: %d cases, worst error / bar %.4f, largest e32 %.3g" % (what, len(cases), worst, e32max))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))
    return cells


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", cc.NS)
def test_chain_dispatch_table(cuda, n):
    """All accepted targeted cases of n rows per cloud; the (n, G, CT, place) cells they reach cover the table."""
    cases = [c for c in cc.targeted() if c.want_rc == cc.OK and not c.plan_only and c.n == n]
    cells = _run_all(cases, cuda, 2, "n = %d" % n)
    need = {c for c in cc.required_cells() if c[0] == n}
    print("n = %d: cells reached %s" % (n, sorted(cells & need)))
    assert need <= cells, "n = %d: cells not reached: %s" % (n, sorted(need - cells))


@pytest.mark.timeout(120)
def test_chain_random_cases(cuda):
    """The accepted cases of the 200 random ones (at most 256 workgroups and 8192 rows each), one launch each."""
    cases = [c for c in cc.random_cases(200) if c.want_rc == cc.OK]
    assert len(cases) >= 50
    _run_all(cases, cuda, 1, "random")


HANDOFF = [
    cc.ChainCase(B=5, n=64, segs=(40, 3), layers=(cc.L(128), cc.L(128)), seed=901, tag="hand-off"),
    cc.ChainCase(B=3, n=256, segs=(128,), layers=(cc.L(128), cc.L(128)), residual=True, seed=902, tag="hand-off"),
    cc.ChainCase(B=33, n=64, segs=(256, 256, 3), layers=(cc.L(256), cc.L(256)), residual=True, seed=903, tag="hand-off"),
]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", HANDOFF, ids=lambda c: "B%d-n%d" % (c.B, c.n))
def test_chain_hand_off_under_changing_inputs(cuda, case):
    """The cross-XCD hand-off (place = 0: a cloud's cluster is spread over the XCDs) with consumers whose caches hold
    the PREVIOUS launch's scratch: 40 launches reuse one scratch without prefill, every segment gets another of 8
    inputs before each launch (new values into the same device tensors), every output is compared with the float64
    result of ITS input.  A stale block is off by O(1)."""
    assert case.B % 8 != 0 and cc.want_rc_of(case) == cc.OK
    T = cc.tensors(case)
    inputs = [T[0]] + [cc.alt_segments(case, k) for k in range(7)]
    wants = [cc.evaluate(case, (sg, T[1]))[0] for sg in inputs]
    e32 = max(cc.rel(cc.evaluate(case, (sg, T[1]), torch.float32)[0].double(), w) for sg, w in zip(inputs, wants))
    bar = max(5e-6, 4.0 * e32)
    P = cc.build(case, cuda)
    assert P.plan()[1] == cc.expected_plan(case) and P.plan()[1][0] * case.B <= 256
    staged = [[sg.to(cuda) for sg in inp] for inp in inputs]
    rows, cols = case.B * case.n, case.cols
    worst = 0.0
    for it in range(40):
        k = (3 * it) % 8 if it % 2 else it % 8                      # not a fixed cycle of neighbours
        P.set_segments(staged[k])
        _launch(P)
        err = cc.rel(P.out[:rows, :cols].double().cpu(), wants[k])
        worst = max(worst, err)
        assert err < bar, "launch %d (input %d): error %.3g, bar %.3g" % (it, k, err, bar)
    print("\nhand-off %s: cell %s, worst error / bar %.4f over 40 launches (e32 %.3g)" % (
        case.label(), cc.cell_of(case, cc.plan_G(case)), worst / bar, e32))
