"""pdr_fused_layer_pool / pdr_fused_layer_pool_f16x3 across their dispatch table on the GPU, against the float64
reference and the derived bound of tests/pool_cases.py; pdr_attention_pool against the same reference.

For every case: the launch returns what pdr_fused_layer_pool_plan returned (a refused call writes nothing); every
expected element of `out` is within the bound; everything else -- rows of unlisted, unpatched queries, columns >= D up
to ldo -- keeps its NaN bits; a second launch gives the same bytes; ws_xcd_order 0 and 2 give the bytes of 1.
"""
import ctypes

import pytest
import torch

from point_diffusion_refinement_amd import _lib
from tests import pool_cases as pc

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_case(case, dev, worst):
    what = case.label()
    P = pc.build(case, dev)
    out = P.new_out()
    rc_plan, plan = P.plan(out.data_ptr())
    rc = P.launch(out)
    assert rc_plan == case.want_rc, "%s: plan rc %d, expected %d" % (what, rc_plan, case.want_rc)
    assert rc == rc_plan, "%s: launch rc %d, plan rc %d" % (what, rc, rc_plan)
    if rc != _lib.PDR_OK:
        assert bool((_bits(out) == NAN_BITS).all()), what + ": a refused call wrote `out`"
        return
    D = case.D
    want, bound, written = pc.expected(P)
    got = out[:, :D].double()
    err = (got - want).abs()
    bad = ~(err <= bound) & written[:, None]
    if bool(bad.any()):
        r, col = [int(v) for v in bad.nonzero()[0]]
        q = int((P.keep["out_rows"] == r).nonzero()[0]) if case.out_rows else r
        pytest.fail("%s: %d elements outside the bound; first at row %d (query %d, cloud %d) col %d: got %r, float64 %r, "
                    "bound %.3g" % (what, int(bad.sum()), r, q, q // (case.rpb // case.K), col, float(got[r, col]),
                                    float(want[r, col]), float(bound[r, col])))
    assert bool((_bits(out[~written]) == NAN_BITS).all()), what + ": rows of unlisted, unpatched queries written"
    assert bool((_bits(out[:, D:]) == NAN_BITS).all()), what + ": columns >= D written"
    ratio = float((err[written] / bound[written].clamp_min(1e-300)).max())
    key = ("split" if case.split else "exact", "ws" if plan[0] else "uniform")
    worst[key] = max(worst.get(key, 0.0), ratio)
    out2 = P.new_out()
    assert P.launch(out2) == _lib.PDR_OK and torch.equal(_bits(out), _bits(out2)), what + ": two launches differ"
    if plan[0]:
        for order in (0, 2):
            with pc.options({"ws_xcd_order": order}):
                out3 = P.new_out()
                assert P.launch(out3) == _lib.PDR_OK and torch.equal(_bits(out), _bits(out3)), \
                    "%s: ws_xcd_order %d / 1 differ" % (what, order)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("opt", list(pc.OPTION_SETS) + ["split"])
def test_pool_dispatch_table(cuda, opt):
    failures, worst = [], {}
    cases = pc.targeted(opt) + pc.random_cases(opt, 20)
    with pc.options({} if opt == "split" else pc.OPTION_SETS[opt]):
        for case in cases:
            try:
                _run_case(case, cuda, worst)
            except (AssertionError, pytest.fail.Exception) as e:     # every case reports; the test fails at the end
                failures.append(str(e).splitlines()[0])
    for key, ratio in sorted(worst.items()):
        print("\n%s: worst error / bound of %s on the %s kernel: %.4f" % (opt, key[0], key[1], ratio))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))


# (B, npoint, K, D, v_relu, vscale / vshift, counts mode): the branches test_attention_pool_matches_masked_softmax
# leaves out -- two loads per lane (NL = 2), the grid cap of the wave-per-query kernel (> 16384 queries), D / 4 not a
# power of two (the generic kernel), v_relu = 0, NULL vscale / vshift, all-zero counts
ATTENTION_CASES = [(2, 40, 16, 32, True, True, "random"), (2, 8200, 8, 8, True, True, "random"),
                   (3, 33, 8, 24, True, True, "random"), (2, 17, 32, 40, False, True, "random"),
                   (2, 64, 16, 32, False, False, "zero"), (2, 20, 8, 24, True, False, "zero"),
                   (2, 50, 32, 64, False, True, "none")]


@pytest.mark.timeout(60)
@pytest.mark.parametrize("B,npoint,K,D,v_relu,affine,counts", ATTENTION_CASES)
def test_attention_pool_within_the_derived_bound(cuda, B, npoint, K, D, v_relu, affine, counts):
    """pdr_attention_pool against pool_cases.pool_reference with the scores given (e_k = 0): every element within
    expm1(2E) sum_k p_k |v_k - out| + 2 (K + 8) u sum_k p_k (|values vscale| + |vshift|), E = max_k 4u (|s_k| + |max s|)."""
    dev = cuda
    g = torch.Generator(device=dev).manual_seed(1000 * B + 10 * npoint + K + D)
    nq = B * npoint
    scores = torch.randn(nq * K, D, device=dev, generator=g) * 3
    valid = torch.full((nq,), K, device=dev)
    cnt = None
    if counts != "none":
        cnt = torch.randint(0, K + 1, (nq,), device=dev, generator=g, dtype=torch.int32)
        cnt[0], cnt[-1] = 0, K
        if counts == "zero":
            cnt.zero_()
        valid = cnt.long().clamp(min=1)
    values = torch.randn(nq * K, D, device=dev, generator=g)
    masked = (torch.arange(nq * K, device=dev) % K) >= valid.repeat_interleave(K)
    values = torch.where(masked[:, None], torch.where(values > 0, 1e6, -1e6), values)       # masked slots are loud
    vs = torch.rand(B, D, device=dev, generator=g) * 3 - 1.5 if affine else None
    vh = torch.randn(B, D, device=dev, generator=g) if affine else None
    out = torch.full((nq, D), float("nan"), device=dev)
    rc = _lib.load().pdr_attention_pool(scores.data_ptr(), D, values.data_ptr(), D, vs.data_ptr() if affine else None,
                                        vh.data_ptr() if affine else None, int(v_relu),
                                        None if cnt is None else cnt.data_ptr(), B, npoint, K, D, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.PDR_OK
    b = torch.arange(nq, device=dev) // npoint
    one = torch.ones(nq, 1, D, device=dev, dtype=torch.float64)
    s = scores.double().view(nq, K, D)
    want, bound = pc.pool_reference(s, torch.zeros_like(s), values.double().view(nq, K, D), cnt,
                                    vs.double()[b][:, None] if affine else one,
                                    vh.double()[b][:, None] if affine else 0.0 * one, v_relu)
    err = (out.double() - want).abs()
    print("\nworst error / bound: %.4f" % float((err / bound.clamp_min(1e-300)).max()))
    bad = ~(err <= bound)
    if bool(bad.any()):
        q, col = [int(v) for v in bad.nonzero()[0]]
        pytest.fail("%d elements outside the bound; first at query %d col %d: got %r, float64 %r, bound %.3g" % (
            int(bad.sum()), q, col, float(out[q, col]), float(want[q, col]), float(bound[q, col])))
