"""One whole training step of the REFINEMENT stage with the six one-op switches and the fused Chamfer loss, against
float64 with every decision pinned -- the method of tests/test_train_step_f64_gpu.py and
tests/test_train_step_injection_gpu.py (whose `switches`, `injection_calls`, `_stacks`, `_sites` and `_same_indices` are
used as they are), on the six cases of tests/refine_step_cases.py (the reference itself is checked by
tests/test_refine_step_f64_host.py).

Per case (head plain / up4 / up4c, loss cd_t / cd_p, relu / swish; B = 2, N = 128, N_gt = 200) and per setting -- `off`
(no switch, calc_cd), `six` (all six switches, calc_cd), `off+fused_loss`, `six+fused_loss` (the same with calc_cd_fused)
-- one fp32 step (forward with ts = None, refine_loss, backward; set_deterministic(True)) records its ReLU tape, its
Chamfer tape (the two index tensors `_ext.chamfer_nn` returns for each Chamfer term, on the step's own refined clouds)
and its index log; the float64 model under `float64_ops("hip")` replays both tapes (settings with equal tapes share one
reference), logs equal index tensors and never searches.  e(S, t) is the error of S at each of the 817 parameter
gradients, at each of the 26 block records, at the gradient w.r.t. the network output, at the output and at the loss.

  1. coverage     with the six on, every fused entry's forward and backward run once per site of this module tree --
                  group_norm_act_add at every stack of an Mlp_plus_t_emb that carries a class embedding or a residual
                  (none carries a step embedding here), group_norm_act at the norms left over -- and no site is on the
                  composition; with all off no fused entry runs; with fused_loss `_ext.chamfer_loss_sums` and its
                  backward run once per Chamfer term and neither `_ext.chamfer_nn` nor `knn_points_grad` runs, without
                  it the K = 1 searches and two `knn_points_grad` calls per term do
  2. the rule     e(S, t) <= 4 max(e(off, t), median of e(off, .) over the gradients of t's block) for every parameter
                  gradient, every block record and grad:displacement; the output and the loss stand alone, the loss
                  with the floor RC.LOSS_FLOOR under its e(off)                                    
  3. the cap      e(off, t) <= 4 E_CPU_REFINE of the case: guards the reference and both tapes, not the ops
  4. fused loss   given the SAME fp32 displacement, loss and displacement gradient of calc_cd_fused (and of calc_cd)
                  against the float64 taped-index evaluation of that refined cloud, within the bounds derived from the
                  header of tests/test_chamfer_loss_gpu.py (below)
  5. determinism  two six+fused_loss steps are bit-equal in loss, output and every gradient
  6. tape honesty `F64.chamfer_tape_honesty` on every run; no coincident pair
  7. the judge    the three faults of RC.FAULTS seeded in Python in the six+fused_loss run each fail 2. at
                  grad:displacement

THE BOUNDS OF 4.  The op's contract (csrc/chamfer_loss.hip, tests/test_chamfer_loss_gpu.py): an element of the gradient
w.r.t. a cloud, with float64 terms t_m, k of them scattered, is within (k + 16) 2^-24 sum |t_m|; sums[:, 0:2] within 28
and sums[:, 2:4] within 30 roundings of 2^-24 relative to the float64 sums of the fp32 minima.  Here the op sits behind
point_upsample and in front of two means:
  * an element of the displacement gradient is c sum_p g_p over the P <= f + 2 refined points p it moves (f grid points,
    the centre among the outputs, the centre of the intermediate term), each g_p within (k_p + 16) 2^-24 mag_p of its
    float64 value.  The sum adds P - 1 roundings and the constant factors (output_scale_factor, 1 / sqrt(f), the
    intermediate weight, 1 / 2) at most 3, each relative to |g_p| <= mag_p; the upstream gradient of a sum is
    (1 / B)(1 / n) [/ 2] evaluated in fp32, 3 roundings common to every term of a direction.  So
        |error| <= 2^-24 |c| sum_p (k_p + 16 + GRAD_EXTRA) mag_p,   GRAD_EXTRA = (f + 1) + 3 + 3
  * the loss is a positive combination of the four sums.  Against float64 distances (not the fp32 minima) an addend
    also carries the rounding of its fp32 distance, 5 roundings (half of them behind the root, plus the root: 3.5);
    the division by n, the add of the directions, the batch mean and the weighted add of the two terms are 4 more:
        |loss - loss64| <= (28 + 5 + 4) 2^-24 loss64 for cd_t, (30 + 4 + 4) 2^-24 loss64 for cd_p

THE SCALE OF A SMALL GRADIENT.  e(t) divides by the tensor's largest float64 element, or by the network's largest
gradient element where the tensor is below 1e-3 of it.  `off` and S have references of their own, so a tensor next to
that threshold can fall on either side of it: FP_modules.1.mlp2.fc_condition.weight of plain-cd_p-relu has its largest
element at 0.997e-3 of the top in the `off` reference and at 1.055e-3 in the `six` one; its largest error is 2.13e-8
off and 1.87e-8 six, yet e(off) = 1.49e-6 and e(six) = 1.28e-3, 215 times the bound (one tensor of up4-cd_t-relu
likewise, 297 times; a forward / backward mask check of both norm ops found nothing).  Which gradients take the
network's largest element as scale is therefore decided once per case, on the `off` run's reference, and every setting
of the case is measured that way (`TC.errors(.., top_scaled_names)`); FACTOR is unchanged.

MEASURED on an MI355X (DESIGN 7a.10 has the tables; the tests print every figure): 25 / 50 / 17 / 8 / 66 sites of the
five ops and 37 stacks on group_norm_act_add in every case, none on the composition; the largest e / bound with six on,
with either loss, 0.51 (plain-cd_p-relu), 0.63 (plain-cd_t-swish), 0.56 (up4-cd_t-relu), 0.82 (up4-cd_t-swish), 0.90
(up4c-cd_p-swish), 0.57 (up4c-cd_t-relu); e(off) within 1.6 E_CPU_REFINE; bounds of 4. used to 0.14 (gradient) and 0.03
(loss); one query of up4c-cd_t-relu with a taped neighbour other than float64's, below 1e-3 of the honesty bound; the
seeded faults at 4.3e4, 1.3e5 and 104 times the bound of grad:displacement.
"""
import collections
import contextlib

import pytest
import torch

from tests import float64_network as F64
from tests import refine_step_cases as RC
from tests import test_train_step_f64_gpu as S1
from tests import test_train_step_injection_gpu as INJ

from point_diffusion_refinement_amd.pointnet2_ops import _ext

pytestmark = pytest.mark.gpu

SETTINGS = {"off": ((), False), "six": (INJ.ALL, False), "off+fused_loss": ((), True), "six+fused_loss": (INJ.ALL, True)}
U = 2.0 ** -24
LOSS_CHAIN = {"cd_t": 28 + 5 + 4, "cd_p": 30 + 4 + 4}
_STATE = {}


@contextlib.contextmanager
def loss_calls():
    """Counters around the `_ext` entries a Chamfer loss can reach: the one-launch search, the backward of the K = 1
    kNN, the fused sums and their backward.  Enter it INSIDE chamfer_tape("record"), whose own search is then not
    counted."""
    counts = collections.Counter()
    names = ("chamfer_nn", "knn_points_grad", "chamfer_loss_sums")
    saved = {k: getattr(_ext, k) for k in names}
    backward = _ext._ChamferLossSums.backward

    def counted(name, fn):
        def wrapped(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapped
    for k, fn in saved.items():
        setattr(_ext, k, counted(k, fn))
    _ext._ChamferLossSums.backward = staticmethod(counted("chamfer_loss_sums_backward", backward))
    try:
        yield counts
    finally:
        _ext._ChamferLossSums.backward = staticmethod(backward)
        for k, fn in saved.items():
            setattr(_ext, k, fn)


def _case(case, device):
    if case not in _STATE:
        variant, loss_type, activation, seed = RC.CASES[case]
        net = RC.network(variant, activation).to(device)
        data = tuple(t if t is None else t.to(device) for t in RC.inputs(seed))
        _STATE[case] = dict(net=net, f64=F64.float64_model(net), refs=[], runs={}, data=data, variant=variant,
                            loss_type=loss_type, activation=activation)
    return _STATE[case]


def _fp32_step(c, setting, fault=None):
    """-> dict of one fp32 step under `setting`: result, both tapes, index log, the three call records."""
    on, fused = SETTINGS[setting]
    with INJ.switches(on), F64.log_indices() as log, F64.count_ext_calls(c["net"]) as calls, \
            F64.relu_tape("record") as tape, INJ.injection_calls(c["net"]) as inj, \
            F64.chamfer_tape("record", nn=_ext.chamfer_nn) as ct, loss_calls() as loss:
        result = RC.step(c["net"], c["data"], c["variant"], c["loss_type"], fused=fused, cd=ct.cd, fault=fault)
    torch.cuda.synchronize()
    return dict(result=result, tape=tape, chamfer=ct.tape, log=log, calls=calls, inj=inj, loss=loss, fused=fused)


def _reference(c, tape, chamfer):
    """The float64 step under both tapes -> (step result, index log, its output cloud per Chamfer term); one evaluation
    per distinct pair of tapes."""
    for t, ct, ref in c["refs"]:
        if t.shapes() == tape.shapes() and t.differing(tape) == 0 and ct.same_decisions(chamfer):
            return ref
    with F64.float64_ops("hip"), F64.log_indices() as log, F64.relu_tape("replay", tape), \
            F64.chamfer_tape("replay", chamfer) as replay:
        ref = RC.step(c["f64"], c["data"], c["variant"], c["loss_type"], cd=replay.cd)
    c["refs"].append((tape, chamfer, (ref, log, replay.outputs)))
    return c["refs"][-1][2]


def _judged(c, run):
    """Errors and tape honesty of a step against its reference; the index logs must agree -- the network's, and the
    K = 1 searches of a composition loss (two per term, behind the network's) with the Chamfer tape."""
    ref, ref_log, outputs64 = _reference(c, run["tape"], run["chamfer"])
    if "top_scaled" not in c:                     # the off run of the case comes first (`_run`) and decides the scales
        c["top_scaled"] = RC.top_scaled(ref)
    searches = 0 if run["fused"] else 2 * len(run["chamfer"])
    log = run["log"]
    S1._same_indices(log[:len(log) - searches], ref_log)
    for n, (name, idx) in enumerate(log[len(log) - searches:]):
        term = run["chamfer"].terms[n // 2]
        assert name == "knn_points" and torch.equal(idx[..., 0], term["idx_out" if n % 2 else "idx_gt"]), (n, name)
    run["e"] = RC.errors(run["result"], ref, c["top_scaled"])
    run["top"] = max(float(g.abs().max()) for g in ref["grads"].values() if g is not None)
    run["near"] = sorted((float(g.abs().max()) / run["top"], n) for n, g in ref["grads"].items()
                         if g is not None and 0.5e-3 <= float(g.abs().max()) / run["top"] <= 2e-3)
    run["honesty"] = F64.chamfer_tape_honesty(run["chamfer"], outputs64)
    return run


def _run(c, setting):
    if setting != "off":
        _run(c, "off")
    if setting not in c["runs"]:
        c["runs"][setting] = _judged(c, _fp32_step(c, setting))
    return c["runs"][setting]


def _report(case, name, e, e_off):
    failed, worst = RC.judge(e, e_off)
    print("%-18s %-16s gradients %.2e  records %.2e  output %.2e  loss %.2e  grad:displacement %.2e   worst e / bound "
          "%.2f at %s" % ((case, name) + RC.summary(e) + (e["grad:displacement"],) + worst))
    return failed


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_every_switch_reaches_every_site_and_the_loss_takes_its_route(cuda, case):
    c = _case(case, cuda)
    sites = S1._sites(c["net"])
    stacks = {block: INJ._stacks(mod) for block, mod in F64.module_names(c["net"]).items()}
    assert all(sum(per_block.values()) > 0 for per_block in sites.values()) and sum(stacks.values()) > 0
    assert sum(stacks.values()) == INJ._stacks(c["net"])                      # every such stack lies in a recorded block
    relu = c["activation"] == "relu"
    terms = RC.terms(c["variant"])
    off = _run(c, "off")
    for setting, (on, fused) in SETTINGS.items():
        run = _run(c, setting)
        calls, inj, loss = run["calls"], run["inj"], run["loss"]
        fallen = []
        for s in F64.SWITCHES:
            fwd, bwd = F64.FUSED_ENTRIES[s]
            total = 0
            for block, n in sites[s].items():
                extra = 0
                if s == "group_norm":
                    # the score head's norms run inside relu_group_norm, a stack with a term inside group_norm_act_add;
                    # behind a ReLU the tape's wrapper of that entry asks group_norm_act for the site's mask
                    n -= sites["score_norm"][block] + stacks[block]
                    extra = stacks[block] if relu else 0
                want = n if on else 0
                total += want
                if calls.count(fwd, block) != want + (extra if on else 0):
                    fallen.append((block, s, "%d of %d sites took _ext.%s; the rest were refused by %s or by the dtype / "
                                   "device test before it" % (calls.count(fwd, block) - (extra if on else 0), want, fwd,
                                                              S1.PREDICATES[s])))
            if on:
                assert calls.count(fwd, None) == 0, (setting, fwd)           # every call belongs to a recorded block
                assert 1 <= calls.count(bwd) <= total, (setting, s, calls.count(bwd), total)
                if s == "group_norm":
                    assert calls.count(bwd) == total, (setting, calls.count(bwd), total)      # (a norm has parameters)
                else:
                    assert calls.count(bwd) == calls.differentiable(fwd), (setting, s, calls.count(bwd))
            else:
                assert calls.count(fwd) == calls.count(bwd) == 0, (setting, s)
        want = sum(stacks.values()) if on else 0
        assert inj.stacks == want and len(inj.backward) == want, (setting, inj.stacks, len(inj.backward), want)
        assert len(inj.forward) == want, "%s: stacks on the composition: %d" % (setting, want - len(inj.forward))
        assert all(block is not None for block, _ in inj.forward + inj.backward)
        assert not fallen, "%s: sites on the composition although their switch is on: %s" % (setting, fallen)
        assert run["tape"].shapes() == off["tape"].shapes()                   # the same ReLU sites, fused or not
        assert len(run["chamfer"]) == terms
        if fused:
            want_loss = {"chamfer_loss_sums": terms, "chamfer_loss_sums_backward": terms}
        else:
            want_loss = {"knn_points_grad": 2 * terms}
        print("%-18s %-16s %s group_norm_act_add %d / %d of %d stacks; loss %s" % (
            case, setting, {e: calls.count(e) for pair in F64.FUSED_ENTRIES.values() for e in pair}, len(inj.forward),
            len(inj.backward), sum(stacks.values()), dict(loss)))
        assert dict(loss) == want_loss, (setting, dict(loss), want_loss)


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_switch_on_error_within_four_times_switch_off(cuda, case):
    c = _case(case, cuda)
    off = _run(c, "off")
    failures = {}
    for setting in SETTINGS:
        run = _run(c, setting)
        failed = _report(case, setting, run["e"], off["e"])
        print("    mask elements differing from the off run: %d of %d; Chamfer decisions equal to the off run's: %s; "
              "references held %d" % (run["tape"].differing(off["tape"]), run["tape"].elements(),
                                      run["chamfer"].same_decisions(off["chamfer"]), len(c["refs"])))
        for t in ("grad:displacement", "loss", "out"):
            print("    %-18s off %.2e  %s %.2e" % (t, off["e"][t], setting, run["e"][t]))
        print("    %d gradients scaled by the network's largest element (%.3e in this run's reference); largest "
              "element / that, of the gradients within a factor 2 of the 1e-3 threshold: %s" % (
                  len(c["top_scaled"]), run["top"], ["%.2e %s%s" % (r, n, " (top-scaled)" if n in c["top_scaled"] else "")
                                                     for r, n in run["near"]]))
        if failed:
            failures[setting] = failed
    assert not failures, "(tensor, block, e, bound) above the rule, per setting: %s" % failures


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_composition_error_within_four_times_the_cpu_baseline(cuda, case):
    got = RC.summary(_run(_case(case, cuda), "off")["e"])
    print("%-18s off: gradients %.2e  records %.2e  output %.2e  loss %.2e   E_cpu %s" % (
        (case,) + got + (RC.E_CPU_REFINE[case],)))
    for measured, baseline in zip(got, RC.E_CPU_REFINE[case]):
        assert measured <= RC.FACTOR * baseline, (got, RC.E_CPU_REFINE[case])


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_fused_loss_and_composition_on_the_same_refined_cloud(cuda, case):
    """The displacement of the off run as a leaf, so that both losses see the same fp32 refined cloud -- a non-leaf
    view chain whose centre feeds two terms -- and the float64 evaluation of THAT cloud with the taped indices."""
    c = _case(case, cuda)
    variant, loss_type = c["variant"], c["loss_type"]
    f = RC.VARIANTS[variant][0]
    generated, _, gt = c["data"][:3]
    held = {}
    for fused in (True, False):
        leaf = _run(c, "off")["result"]["out"].to(device=cuda, dtype=torch.float32).requires_grad_()
        with INJ.switches(()), F64.chamfer_tape("record", nn=_ext.chamfer_nn) as ct:
            loss = RC.refine_loss(leaf, generated, gt, variant, loss_type, fused, cd=ct.cd)
            loss.backward()
        want, mag, scattered = RC.displacement_gradient(variant, loss_type, ct.tape)
        loss64 = sum(F64.taped_cd(t["out"], t["gt"], t["idx_gt"], t["idx_out"])[1 if loss_type == "cd_t" else 0].mean()
                     * (RC.INTERMEDIATE_WEIGHT if n else 1.0) for n, t in enumerate(ct.tape.terms))
        got = leaf.grad.double().cpu()
        assert bool(torch.isfinite(got).all()) and got.shape == want.shape
        bound = U * ((16 + (f + 1) + 3 + 3) * mag + scattered)
        ratio = float(((got - want).abs() / bound).max())
        loss_ratio = abs(float(loss.detach()) - float(loss64)) / (LOSS_CHAIN[loss_type] * U * float(loss64))
        print("%-18s %-13s displacement gradient: worst error / bound %.3f (largest weighted count of scattered terms %d); loss "
              "%.9g, float64 %.9g, error / bound %.3f" % (case, "calc_cd_fused" if fused else "calc_cd", ratio,
                                                          int((scattered / mag).max()), float(loss.detach()), float(loss64),
                                                          loss_ratio))
        held[fused] = (ratio, loss_ratio, ct.tape)
    assert held[True][2].same_decisions(held[False][2])
    assert held[True][0] <= 1.0 and held[True][1] <= 1.0, held[True][:2]
    assert held[False][0] <= 1.0 and held[False][1] <= 1.0, held[False][:2]


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_two_six_on_fused_loss_steps_are_bit_equal(cuda, case):
    c = _case(case, cuda)
    first, second = _run(c, "six+fused_loss")["result"], _fp32_step(c, "six+fused_loss")["result"]
    names = [k for k in ("loss", "out", "out_grad") if not torch.equal(first[k], second[k])]
    names += ["grad:" + n for n, g in first["grads"].items() if g is not None and not torch.equal(g, second["grads"][n])]
    names += ["record:" + n for n, r in first["records"].items() if not torch.equal(r, second["records"][n])]
    assert not names, "two six+fused_loss steps differ at %d tensors %s" % (len(names), names[:8])


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_the_chamfer_tape_is_honest_on_every_run(cuda, case):
    c = _case(case, cuda)
    for setting in SETTINGS:
        h = _run(c, setting)["honesty"]
        print("%-18s %-16s queries whose taped neighbour is not float64's own: %d, largest ratio to the bound %.3f; "
              "delta %.2e, smallest nearest-neighbour distance %.2e" % (case, setting, h["differing"], h["ratio"],
                                                                        h["delta"], h["nearest"]))
        assert h["nearest"] >= RC.NEAREST_BOUND and h["ratio"] <= 1.0, (setting, h)


def test_the_judge_catches_three_seeded_faults(cuda):
    """The faults of RC.FAULTS, in Python, in the loss of the six+fused_loss run of FAULT_CASE; no kernel changes.  None
    of them changes the forward of the network, so both tapes and the reference are the unseeded run's."""
    case = RC.FAULT_CASE
    c = _case(case, cuda)
    e_off = _run(c, "off")["e"]
    base = _run(c, "six+fused_loss")
    assert not RC.judge(base["e"], e_off)[0]                                 # (the unseeded run passes)
    for fault in RC.FAULTS:
        run = _judged(c, _fp32_step(c, "six+fused_loss", fault=fault))
        assert run["tape"].differing(base["tape"]) == 0 and run["chamfer"].same_decisions(base["chamfer"])
        failed = _report(case, "fault " + fault[:10], run["e"], e_off)
        bound = RC.FACTOR * e_off["grad:displacement"]
        print("    %-17s %d tensors above the rule; grad:displacement e %.2e, %.3g times its bound; loss e %.2e" % (
            fault, len(failed), run["e"]["grad:displacement"], run["e"]["grad:displacement"] / bound, run["e"]["loss"]))
        assert "grad:displacement" in {t for t, _, _, _ in failed}, (fault, failed[:5])
