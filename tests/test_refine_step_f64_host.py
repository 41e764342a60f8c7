"""The reference of tests/test_refine_step_f64_gpu.py, checked on the CPU: one refinement step (forward without step
embedding, point_upsample, Chamfer loss with its intermediate term, backward) of the tiny network in float64 under the
ReLU decisions AND the nearest-neighbour assignment of the fp32 run it is compared with (tests/float64_network.py
`relu_tape`, `chamfer_tape`; tests/refine_step_cases.py) -- the pattern of tests/test_train_step_f64_host.py.

Both evaluations run on the CPU through `float64_ops("oracle")`: the fp32 module with calc_cd (the composition: neither
a fused op nor calc_cd_fused has a CPU form) and its double copy, whose loss gathers by the taped indices and calls no
search.  What is asserted, per case of `RC.CASES`:
  * `loss.backward()` of the float64 model reaches every parameter the step uses (all but fc_t1 / fc_t2);
  * the max-over-points of the global PointNet, which nothing pins, is at least 1e-4 from a tie in the float64 run;
  * no coincident pair: the smallest float64 nearest-neighbour distance is at least 1e-6 in both directions;
  * the Chamfer tape is honest (`F64.chamfer_tape_honesty`: a taped index differs from float64's own argmin only within
    what the output error can move the two distances);
  * the pinned error of the fp32 CPU composition is the E_CPU_REFINE that refine_step_cases.py records (within
    [E / 8, E]; the loss value, one fp32 number, only below E);
  * the taped float64 loss differentiated by autograd equals the Chamfer gradient written out term by term
    (`RC.displacement_gradient`) to 1e-12 of the sum of |terms| per element, for cd_t and cd_p and all three heads;
  * replaying the float64 run's own two tapes changes nothing;
  * three faults seeded in Python in the fp32 loss each leave the rule at grad:displacement.
"""
import pytest
import torch

from tests import float64_network as F64
from tests import refine_step_cases as RC
from tests import train_step_cases as TC

_CACHE = {}


def _runs(case):
    if case not in _CACHE:
        _CACHE[case] = RC.cpu_runs(*RC.CASES[case])
    return _CACHE[case]


def test_the_cases_are_the_six_of_the_design():
    assert sorted((v, l, a) for v, l, a, _ in RC.CASES.values()) == sorted([
        ("up4", "cd_t", "relu"), ("up4c", "cd_p", "swish"), ("plain", "cd_p", "relu"), ("up4", "cd_t", "swish"),
        ("plain", "cd_t", "swish"), ("up4c", "cd_t", "relu")])
    assert all(1 <= seed <= 20 for _, _, _, seed in RC.CASES.values())
    assert RC.N_GT != RC.N and RC.N_GT % RC.N != 0 and RC.VARIANTS[RC.CASES[RC.FAULT_CASE][0]][0] > 1


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_float64_backward_reaches_every_used_parameter(case):
    r = _runs(case)
    variant = RC.CASES[case][0]
    f, centre_out = RC.VARIANTS[variant]
    out_dim = 3 if f == 1 else 3 * (f if centre_out else f + 1)
    for run in (r["r64"], r["pinned"], r["r32"]):
        missing = [n for n, g in run["grads"].items() if g is None]
        assert missing == ["fc_t1.weight", "fc_t1.bias", "fc_t2.weight", "fc_t2.bias"], missing
        assert all(bool(torch.isfinite(g).all()) for g in run["grads"].values() if g is not None)
        assert run["out"].shape == run["out_grad"].shape == (RC.B, RC.N, out_dim)
        assert bool(torch.isfinite(run["out_grad"]).all()) and float(run["out_grad"].abs().max()) > 0
        assert float(run["loss"]) > 0
    assert len(r["chamfer32"]) == RC.terms(variant)
    n_out = {"plain": RC.N, "up4": 4 * RC.N, "up4c": 4 * RC.N}[variant]
    assert r["chamfer32"].terms[0]["idx_gt"].shape == (RC.B, RC.N_GT)
    assert r["chamfer32"].terms[0]["idx_out"].shape == (RC.B, n_out)
    assert r["chamfer32"].terms[-1]["idx_out"].shape == (RC.B, n_out if f == 1 else RC.N)


def test_the_uncovered_chamfer_entries_still_raise():
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    with F64.float64_ops("oracle"):
        for name in ("chamfer_nn", "chamfer_loss_sums", "knn_points_grad"):
            with pytest.raises(AssertionError, match=name):
                getattr(_ext, name)()


def test_a_chamfer_tape_that_does_not_fit_is_an_error_that_names_the_term():
    g = torch.Generator().manual_seed(0)
    out, gt = torch.randn(2, 7, 3, generator=g), torch.randn(2, 5, 3, generator=g)
    with pytest.raises(ValueError):
        with F64.chamfer_tape("record"):
            pass
    with pytest.raises(ValueError):
        with F64.chamfer_tape("replay"):
            pass
    seen = []
    with F64.chamfer_tape("record", nn=F64.oracle_chamfer_nn) as rec:
        assert rec.cd(lambda o, t: seen.append((o, t)) or "value")(out, gt) == "value"
    assert len(rec.tape) == 1 and seen[0][0] is out and rec.tape.terms[0]["idx_gt"].dtype == torch.int64
    # the recorded indices are the float64 argmin of these well-separated clouds, and the replay is calc_cd's formula
    pair = ((gt.double().unsqueeze(2) - out.double().unsqueeze(1)) ** 2).sum(-1)
    assert torch.equal(rec.tape.terms[0]["idx_gt"], pair.argmin(2)) and torch.equal(rec.tape.terms[0]["idx_out"], pair.argmin(1))
    with F64.chamfer_tape("replay", rec.tape) as rep:
        cd_p, cd_t = rep.cd()(out.double(), gt.double())
    d1, d2 = pair.min(2).values, pair.min(1).values
    assert torch.allclose(cd_t, d1.mean(1) + d2.mean(1), rtol=1e-14, atol=0)
    assert torch.allclose(cd_p, (d1.sqrt().mean(1) + d2.sqrt().mean(1)) / 2, rtol=1e-14, atol=0)
    with pytest.raises(AssertionError, match="term 0 was recorded"):
        with F64.chamfer_tape("replay", rec.tape) as rep:
            rep.cd()(out[:, :-1].double(), gt.double())
    with pytest.raises(AssertionError, match="Chamfer term 1, the tape holds 1"):
        with F64.chamfer_tape("replay", rec.tape) as rep:
            rep.cd()(out.double(), gt.double())
            rep.cd()(out.double(), gt.double())
    with pytest.raises(AssertionError, match="ended at term 0 of 1"):
        with F64.chamfer_tape("replay", rec.tape):
            pass


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_fp32_and_float64_record_the_same_sites(case):
    r = _runs(case)
    t32, t64 = r["tape32"], r["tape64"]
    assert len(t32) == len(t64) > 0 and t32.shapes() == t64.shapes() and set(t32.kinds) == {"relu"}
    differ = sum(int((a[k] != b[k]).sum()) for a, b in zip(r["chamfer32"].terms, r["chamfer64"].terms)
                 for k in ("idx_gt", "idx_out"))
    print(case, "ReLU sites", len(t32), "elements", t32.elements(), "differing", t32.differing(t64),
          "; Chamfer terms", len(r["chamfer32"]), "indices differing from the float64 run's own tape", differ)
    assert len(r["chamfer32"]) == len(r["chamfer64"])


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_max_over_points_is_far_from_a_tie(case):
    gaps = _runs(case)["gaps"]
    print(case, "seed", RC.CASES[case][3], gaps)
    assert set(gaps) == {"global_pnet.mlp1", "global_pnet.mlp2"}
    for name, (gap, dead) in gaps.items():
        assert gap >= RC.GAP_BOUND, (name, gap, dead)


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_no_coincident_pair_and_the_chamfer_tape_is_honest(case):
    h = _runs(case)["honesty"]
    print("%-18s queries whose taped neighbour is not float64's own: %d, largest ratio to the bound %.3f; delta %.2e, "
          "smallest nearest-neighbour distance %.2e" % (case, h["differing"], h["ratio"], h["delta"], h["nearest"]))
    assert h["nearest"] >= RC.NEAREST_BOUND, h
    assert h["ratio"] <= 1.0, h


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_cpu_baseline(case):
    r = _runs(case)
    e = RC.errors(r["r32"], r["pinned"])
    by_block = {}
    for t, v in e.items():
        if t.startswith("grad:"):
            by_block[TC.block(t)] = max(by_block.get(TC.block(t), 0.0), v)
    for b in sorted(by_block):
        print("%-18s %-26s worst gradient %.2e  record %.2e" % (case, b, by_block[b], e.get("record:" + b, float("nan"))))
    got = RC.summary(e)
    print("%-18s E_cpu measured (%d threads): gradients %.2e  records %.2e  output %.2e  loss %.2e   displacement "
          "gradient %.2e" % ((case, torch.get_num_threads()) + got + (e["grad:displacement"],)))
    assert sum(t.startswith("record:") for t in e) == 26 and sum(t.startswith("grad:") for t in e) == 817 + 1
    for measured, recorded in zip(got[:3], RC.E_CPU_REFINE[case]):
        assert recorded / 8 <= measured <= recorded, (got, RC.E_CPU_REFINE[case])
    assert got[3] <= RC.E_CPU_REFINE[case][3] >= RC.LOSS_FLOOR          # one fp32 number: a single draw, no lower limit
    assert min(e.values()) >= 0.0 and e["out"] > 0.0               # (two precisions, not one run against itself)


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_autograd_of_the_taped_loss_is_the_chamfer_gradient_term_by_term(case):
    """float64 against float64: `pinned["out_grad"]` went through torch autograd -- gathers, point_upsample's view /
    reshape / cat, the means; `RC.displacement_gradient` writes the same gradient out per term from the indices."""
    r = _runs(case)
    variant, loss_type = RC.CASES[case][:2]
    want, mag, _ = RC.displacement_gradient(variant, loss_type, r["chamfer32"], clouds=r["outputs64"])
    got = r["pinned"]["out_grad"]
    ratio = float(((got - want).abs() / mag.clamp(min=1e-300)).max())
    print("%-18s autograd against term-by-term: largest |difference| / sum |terms| %.2e" % (case, ratio))
    assert got.shape == want.shape and float(mag.min()) > 0
    assert bool(((got - want).abs() <= 1e-12 * mag).all()), ratio


def test_replaying_a_runs_own_tapes_changes_nothing():
    case = RC.FAULT_CASE
    r = _runs(case)
    variant, loss_type = RC.CASES[case][:2]
    with F64.float64_ops("oracle"), F64.relu_tape("replay", r["tape64"]), \
            F64.chamfer_tape("replay", r["chamfer64"]) as replay:
        again = RC.step(r["f64"], r["data"], variant, loss_type, cd=replay.cd)
    e = RC.errors(again, r["r64"])
    print(case, "own tapes replayed: largest e %.2e" % max(e.values()))
    assert max(e.values()) <= 1e-12 and torch.equal(again["out"], r["r64"]["out"])
    assert F64.chamfer_tape_honesty(r["chamfer64"], replay.outputs)["ratio"] <= 1.0


def test_the_judge_catches_three_seeded_faults():
    """The fp32 CPU step of FAULT_CASE with a fault in its loss, judged as a switch set is judged on the GPU, the
    unseeded fp32 CPU step being the baseline.  No fault changes the network's forward, so the run's tapes stay the
    unseeded run's and so does the reference."""
    case = RC.FAULT_CASE
    r = _runs(case)
    variant, loss_type = RC.CASES[case][:2]
    e_off = RC.errors(r["r32"], r["pinned"])
    assert not RC.judge(e_off, e_off)[0]
    for fault in RC.FAULTS:
        with F64.float64_ops("oracle", dtype=torch.float32), F64.relu_tape("record") as tape, \
                F64.chamfer_tape("record", nn=F64.oracle_chamfer_nn) as ct:
            got = RC.step(r["net"], r["data"], variant, loss_type, cd=ct.cd, fault=fault)
        assert tape.differing(r["tape32"]) == 0 and ct.tape.same_decisions(r["chamfer32"])
        e = RC.errors(got, r["pinned"])
        failed, worst = RC.judge(e, e_off)
        named = {t for t, _, _, _ in failed}
        print("%-18s fault %-17s %d tensors above the rule, worst e / bound %.3g at %s; grad:displacement e %.2e, "
              "%.3g times its bound; loss e %.2e" % (case, fault, len(failed), worst[0], worst[1], e["grad:displacement"],
                                                    e["grad:displacement"] / (TC.FACTOR * e_off["grad:displacement"]),
                                                    e["loss"]))
        assert "grad:displacement" in named, (fault, failed[:5])
