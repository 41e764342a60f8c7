"""The reference of tests/test_train_step_f64_gpu.py, checked on the CPU: one training step (forward, MSE loss, backward)
of the tiny network in float64 with the ReLU decisions of the fp32 run it is compared with (tests/float64_network.py
`relu_tape`, tests/train_step_cases.py).

Both evaluations here run on the CPU through `float64_ops("oracle")`: the fp32 module (the composition: no fused op has a
CPU form) and its double copy, same index tensors, same scatter-add backward stand-ins.  What is asserted:
  * `loss.backward()` of the float64 model runs and reaches every parameter;
  * a replayed tape changes nothing when it is the run's own (torch.equal), in both precisions;
  * the fp32 and the float64 run record the same ReLU sites in the same order;
  * the max-over-points of the global PointNet, which nothing pins, is at least 1e-4 from a tie in the float64 run;
  * the pinned error of the fp32 CPU composition is the E_cpu that train_step_cases.py records;
  * where fp32 and float64 disagree on mask elements, the unpinned error is at least 20 times the pinned one.

The seed of the last check: a search over the input seeds 1 .. 7 of (relu, noise) with this file's evaluation
(fp32 against float64, mask elements that differ / worst gradient error unpinned / pinned) gave
    1: 0   3: 0   4: 0   5: 0        no mask differs: 4.7e-5 .. 1.1e-4 either way
    2: 8 elements, 2.1e-2 / 2.8e-4     6: 2, 2.4e-2 / 5.7e-5     7: 9, 1.2e-2 / 4.2e-4
so FLIP_SEED = 2.  Which elements differ depends on the last bit of the host's fp32 convolutions (1 thread: 3 of them
at seed 9 of relu-surface, 8 threads: 9), so the test also covers a host on which seed 2 keeps its masks: it then inverts
one recorded element by hand (the unit of the last ReLU with the largest output) and asserts the same factor.
"""
import pytest
import torch

from tests import float64_network as F64
from tests import train_step_cases as TC

FLIP_SEED = 2
_CACHE = {}


def _runs(activation, regime, seed):
    """-> fp32 CPU step (tape recorded), float64 step on its own decisions (tape recorded), float64 step under the fp32
    tape, the float64 run's max-over-points gaps; computed once."""
    key = (activation, regime, seed)
    if key not in _CACHE:
        net = TC.network(activation)
        f64 = F64.float64_model(net)
        data = TC.inputs(regime, seed)
        with F64.float64_ops("oracle", dtype=torch.float32), F64.relu_tape("record") as tape32:
            r32 = TC.step(net, data)
        with F64.float64_ops("oracle"), F64.relu_tape("record") as tape64, F64.record_max_gaps(f64) as gaps:
            r64 = TC.step(f64, data)
        with F64.float64_ops("oracle"), F64.relu_tape("replay", tape32):
            pinned = TC.step(f64, data)
        _CACHE[key] = dict(net=net, f64=f64, data=data, r32=r32, r64=r64, pinned=pinned, tape32=tape32, tape64=tape64,
                           gaps=gaps)
    return _CACHE[key]


def _same(a, b):
    return torch.equal(a["out"], b["out"]) and a["grads"].keys() == b["grads"].keys() and \
        all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"]) and \
        all(torch.equal(a["records"][n], b["records"][n]) for n in a["records"])


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_float64_backward_reaches_every_parameter(case):
    r = _runs(*TC.CASES[case])
    for run in (r["r64"], r["pinned"], r["r32"]):
        missing = [n for n, g in run["grads"].items() if g is None]
        assert len(run["grads"]) == 837 and not missing, missing
        assert all(bool(torch.isfinite(g).all()) for g in run["grads"].values())
    assert any(float(g.abs().max()) > 0 for g in r["r64"]["grads"].values())


def test_the_uncovered_backward_entries_still_raise():
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    with F64.float64_ops("oracle"):
        for name in ("knn_points_grad", "attention_pool_grad", "group_norm_act_grad", "query_group_grad",
                     "knn_group_cf_grad", "relu_group_norm_grad"):
            with pytest.raises(AssertionError, match=name):
                getattr(_ext, name)()
        for name in F64.SWITCHES:
            assert getattr(_ext, "is_fused_" + name)() is False          # the switches still answer
    assert _ext.gather_points_grad.__module__ == _ext.__name__           # restored


def test_backward_stand_ins_are_the_adjoints_of_the_forward_ones():
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    g = torch.Generator().manual_seed(0)
    pts = torch.randn(2, 5, 16, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, 16, (2, 7, 3), generator=g, dtype=torch.int32)
    w = torch.rand(2, 7, 3, generator=g, dtype=torch.float64)
    with F64.float64_ops("oracle"):
        for suffix in ("", "_det"):
            for fwd, name, args, extra in ((_ext.gather_points, "gather_points_grad", (idx[:, :, 0].contiguous(),), ()),
                                           (_ext.group_points, "group_points_grad", (idx,), ()),
                                           (_ext.three_interpolate, "three_interpolate_grad", (idx, w), (w,))):
                out = fwd(pts, *args)
                go = torch.randn(out.shape, generator=g, dtype=torch.float64)
                (want,) = torch.autograd.grad(out, pts, go)
                got = getattr(_ext, name + suffix)(go, args[0], *extra, 16)
                assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=0, atol=1e-14), name + suffix
                assert getattr(_ext, name + suffix)(go.float(), args[0], *extra, 16).dtype == torch.float32


def test_replaying_a_runs_own_tape_changes_nothing():
    r = _runs(*TC.CASES["relu-noise"])
    for model, dtype, tape, taped in ((r["net"], torch.float32, r["tape32"], r["r32"]),
                                      (r["f64"], torch.float64, r["tape64"], r["r64"])):
        with F64.float64_ops("oracle", dtype=dtype):
            plain = TC.step(model, r["data"])
            with F64.relu_tape("replay", tape):
                replayed = TC.step(model, r["data"])
        assert _same(plain, taped) and _same(plain, replayed), dtype


def test_a_tape_that_does_not_fit_is_an_error_that_names_the_site():
    r = _runs(*TC.CASES["relu-noise"])
    tape = r["tape32"]
    short = F64.ReluTape(tape.masks[:-1], tape.kinds[:-1])
    with pytest.raises(AssertionError, match="ReLU call %d, the tape holds %d" % (len(short), len(short))):
        with F64.float64_ops("oracle"), F64.relu_tape("replay", short):
            TC.step(r["f64"], r["data"])
    wrong = F64.ReluTape(tape.masks[:7] + [tape.masks[7][:, :-1]] + tape.masks[8:], tape.kinds)
    with pytest.raises(AssertionError, match="site 7 "):
        with F64.float64_ops("oracle"), F64.relu_tape("replay", wrong):
            TC.step(r["f64"], r["data"])
    with pytest.raises(AssertionError, match="ended at site 1 of %d" % len(tape)):
        with F64.relu_tape("replay", tape):
            torch.nn.ReLU()(torch.zeros(tape.masks[0].shape))
    assert torch.nn.ReLU.forward(torch.nn.ReLU(), torch.tensor([-1.0, 2.0])).tolist() == [0.0, 2.0]     # restored


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_fp32_and_float64_record_the_same_sites(case):
    r = _runs(*TC.CASES[case])
    t32, t64 = r["tape32"], r["tape64"]
    assert len(t32) == len(t64) > 0 and t32.shapes() == t64.shapes() and set(t32.kinds) == {"relu"}
    print(case, "sites", len(t32), "elements", t32.elements(), "differing", t32.differing(t64))
    assert len(t32) == (154 if case.startswith("relu") else 79)


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_max_over_points_is_far_from_a_tie(case):
    gaps = _runs(*TC.CASES[case])["gaps"]
    print(case, gaps)
    assert set(gaps) == {"global_pnet.mlp1", "global_pnet.mlp2"}
    for name, (gap, dead) in gaps.items():
        assert gap >= TC.GAP_BOUND, (name, gap, dead)


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_cpu_baseline(case):
    r = _runs(*TC.CASES[case])
    e = TC.errors(r["r32"], r["pinned"])
    by_block = {}
    for t, v in e.items():
        if t.startswith("grad:"):
            by_block[TC.block(t)] = max(by_block.get(TC.block(t), 0.0), v)
    for b in sorted(by_block):
        print("%-14s %-26s worst gradient %.2e  record %.2e" % (case, b, by_block[b], e.get("record:" + b, float("nan"))))
    got = TC.summary(e)
    print("%-14s E_cpu measured: gradients %.2e  records %.2e  output %.2e" % ((case,) + got))
    assert len(by_block) == 30 and sum(t.startswith("record:") for t in e) == 26
    for measured, recorded in zip(got, TC.E_CPU[case]):
        assert recorded / 8 <= measured <= recorded, (got, TC.E_CPU[case])
    assert min(e.values()) >= 0.0 and e["out"] > 0.0               # (two precisions, not one run against itself)


def test_unpinned_masks_cost_twenty_times_the_rounding_error():
    r = _runs("relu", "noise", FLIP_SEED)
    differing = r["tape32"].differing(r["tape64"])
    pinned = TC.summary(TC.errors(r["r32"], r["pinned"]))[0]
    if differing:
        unpinned = TC.summary(TC.errors(r["r32"], r["r64"]))[0]
    else:                                   # this host's fp32 run kept float64's masks: invert one by hand
        site = len(r["tape32"]) - 1
        hooked = []
        h = r["f64"].fc_lyaer[-2].register_forward_hook(lambda m, a, out: hooked.append(out.detach()))
        with F64.float64_ops("oracle"), F64.relu_tape("replay", r["tape32"]):
            TC.step(r["f64"], r["data"])
        h.remove()
        index = tuple(int(i) for i in torch.unravel_index(hooked[0].argmax(), hooked[0].shape))
        with F64.float64_ops("oracle"), F64.relu_tape("replay", r["tape32"].flipped(site, index)):
            unpinned = TC.summary(TC.errors(r["r32"], TC.step(r["f64"], r["data"])))[0]
    print("seed %d: %d mask elements differ; worst gradient error unpinned %.2e, pinned %.2e"
          % (FLIP_SEED, differing, unpinned, pinned))
    assert unpinned >= 20 * pinned, (differing, unpinned, pinned)
