"""One whole training step of the trainable path with set_fused_injection, alone and together with the five other one-op
switches, against float64 with every decision pinned -- the method of tests/test_train_step_f64_gpu.py
(tests/train_step_cases.py, tests/float64_network.py), on the same three cases.

Per case and per switch set S -- all off, injection alone, all six on -- one fp32 step (forward, MSE loss, backward;
set_deterministic(True)) records its ReLU tape and its index tensors; the float64 model under `float64_ops("hip")`
replays that tape and must log equal index tensors.  e(S, t) is the error of S at the output, at every parameter
gradient and at every block record; the all-off run of THIS file is the baseline of `TC.judge`.

THE RELU TAPE does not know `_ext.group_norm_act_add`.  Inside its context the entry is wrapped here: a call with
act == "relu" also calls the tape's patched `_ext.group_norm_act` on the same x, which appends the site's mask.  That
mask is exact: the two entries share z bit for bit (tests/test_group_norm_act_add_gpu.py asserts mean, rstd and y so).

  1. coverage     forward and backward calls of the new entry = the stacks of the module tree's Mlp_plus_t_emb that
                  carry an embedding or a residual; no such stack takes the composition; with the switch off the entry
                  never runs; the tape has the all-off run's sites
  2. the rule     e(S, t) <= 4 max(e(off, t), median of e(off, .) over the gradients of t's block)      
  3. determinism  two six-on steps are bit-equal
  4. the judge    grad_e of one call scaled by 1 + 1e-3 fails 2. in that call's block

MEASURED on an MI355X (the tests print every figure): 45 stacks, 45 forward and 45 backward calls in every
case and both sets; the largest e / bound over all tensors 0.69 / 0.40 / 0.82 with injection alone and 0.63 / 0.80 /
0.54 with all six on (relu-noise, relu-surface, swish-noise); the seeded fault, in FP_modules.0, at 24 times its bound.
"""
import contextlib

import pytest
import torch

from tests import float64_network as F64
from tests import train_step_cases as TC

from point_diffusion_refinement_amd.pointnet2_ops import _ext
from point_diffusion_refinement_amd.pointnet2_ops.attention import NormActSequential
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import Mlp_plus_t_emb

pytestmark = pytest.mark.gpu

ALL = F64.SWITCHES + ("injection",)
SETS = {"off": (), "injection": ("injection",), "six": ALL}
_STATE = {}


@contextlib.contextmanager
def switches(on):
    """As tests/test_train_step_f64_gpu.py `switches`, with the sixth switch."""
    prev = {}
    library = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    try:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        prev["deterministic"] = _ext.set_deterministic(True)
        for name in ALL:
            prev[name] = getattr(_ext, "set_fused_" + name)(name in on)
        yield
    finally:
        for name, value in prev.items():
            getattr(_ext, "set_deterministic" if name == "deterministic" else "set_fused_" + name)(value)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = library


class Calls:
    """forward / backward: one (block, largest |grad_e| or None) per call of the new entry, in call order;
    `stacks`: forward_add calls that carried a term; `scale`: {backward call number: factor on its grad_e}."""

    def __init__(self):
        self.forward, self.backward, self.stacks, self.scale = [], [], 0, {}


@contextlib.contextmanager
def injection_calls(net):
    """Counters around `_ext.group_norm_act_add` / `_grad` and `NormActSequential.forward_add`, the tape's mask for the
    ReLU inside the op, and fault seeding.  Enter it INSIDE relu_tape("record")."""
    calls, stack, owner = Calls(), [], {}
    fwd, bwd, forward_add = _ext.group_norm_act_add, _ext.group_norm_act_add_grad, NormActSequential.forward_add

    def group_norm_act_add(x, weight, bias, num_groups, eps=1e-5, act="none", add=None, residual=None):
        if act == "relu":
            _ext.group_norm_act(x, weight, bias, num_groups, eps, act)         # the tape's: appends z > 0 of this site
        owner[x.data_ptr()] = stack[-1] if stack else None
        calls.forward.append((owner[x.data_ptr()], None))
        return fwd(x, weight, bias, num_groups, eps, act, add, residual)

    def group_norm_act_add_grad(x, *a, **k):
        out = bwd(x, *a, **k)
        n, ge = len(calls.backward), out[3]
        calls.backward.append((owner.get(x.data_ptr()), None if ge is None else float(ge.abs().max())))
        if n in calls.scale:
            out = out[:3] + (ge * calls.scale[n],)
        return out

    def counted_forward_add(self, x, add=None, residual=None):
        calls.stacks += add is not None or residual is not None
        return forward_add(self, x, add, residual)

    def leave(m, args, out):                                 # (returns None: a hook's return value replaces the output)
        stack.pop()

    handles = []
    for name, mod in F64.module_names(net).items():
        handles.append(mod.register_forward_pre_hook(lambda m, args, name=name: stack.append(name)))
        handles.append(mod.register_forward_hook(leave))
    _ext.group_norm_act_add, _ext.group_norm_act_add_grad = group_norm_act_add, group_norm_act_add_grad
    NormActSequential.forward_add = counted_forward_add
    try:
        yield calls
    finally:
        _ext.group_norm_act_add, _ext.group_norm_act_add_grad = fwd, bwd
        NormActSequential.forward_add = forward_add
        for h in handles:
            h.remove()


def _case(case, device):
    if case not in _STATE:
        activation, regime, seed = TC.CASES[case]
        net = TC.network(activation).to(device)
        _STATE[case] = dict(net=net, f64=F64.float64_model(net), refs=[], runs={},
                            data=tuple(t.to(device) for t in TC.inputs(regime, seed)))
    return _STATE[case]


def _fp32_step(c, on, scale=None):
    """-> (step result, tape, index log, Calls) of one fp32 step under the switch set `on`."""
    with switches(on), F64.log_indices() as log, F64.relu_tape("record") as tape, injection_calls(c["net"]) as calls:
        calls.scale.update(scale or {})
        result = TC.step(c["net"], c["data"])
    torch.cuda.synchronize()
    return result, tape, log, calls


def _reference(c, tape):
    """The float64 step under `tape` -> (step result, index log); one evaluation per distinct tape."""
    for t, ref in c["refs"]:
        if t.shapes() == tape.shapes() and t.differing(tape) == 0:
            return ref
    with F64.float64_ops("hip"), F64.log_indices() as log, F64.relu_tape("replay", tape):
        ref = TC.step(c["f64"], c["data"]), log
    c["refs"].append((tape, ref))
    return ref


def _same_indices(log_a, log_b):
    assert len(log_a) == len(log_b) > 0, (len(log_a), len(log_b))
    for i, ((na, a), (nb, b)) in enumerate(zip(log_a, log_b)):
        assert na == nb and a.shape == b.shape and bool((a.long() == b.long()).all()), (i, na, nb)


def _errors(c, result, tape, log):
    ref, ref_log = _reference(c, tape)
    _same_indices(log, ref_log)
    return TC.errors(result, ref)


def _run(c, name):
    if name not in c["runs"]:
        result, tape, log, calls = _fp32_step(c, SETS[name])
        c["runs"][name] = dict(result=result, tape=tape, calls=calls, e=_errors(c, result, tape, log))
    return c["runs"][name]


def _stacks(net):
    """Stacks of the module tree's Mlp_plus_t_emb that an embedding or the residual follows."""
    n = 0
    for m in net.modules():
        if isinstance(m, Mlp_plus_t_emb):
            last_is_second = m.rest_mlp is None
            n += bool(m.include_t)
            n += bool(m.include_condition or (last_is_second and m.res_connect_bool))
            if not last_is_second:
                n += bool(m.include_second_condition or m.res_connect_bool)
    return n


def _report(case, name, e, e_off):
    failed, worst = TC.judge(e, e_off)
    print("%-13s %-10s gradients %.2e  records %.2e  output %.2e   worst e / bound %.2f at %s"
          % ((case, name) + TC.summary(e) + worst))
    return failed


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_the_switch_reaches_every_stack_and_none_takes_the_composition(cuda, case):
    c = _case(case, cuda)
    want = _stacks(c["net"])
    assert want > 0
    off = _run(c, "off")
    assert not off["calls"].forward and not off["calls"].backward and off["calls"].stacks == 0
    for name in ("injection", "six"):
        run = _run(c, name)
        calls = run["calls"]
        print("%-13s %-10s stacks %d  forward_add with a term %d  forward calls %d  backward calls %d"
              % (case, name, want, calls.stacks, len(calls.forward), len(calls.backward)))
        assert calls.stacks == want                                      # every such stack goes through forward_add
        assert len(calls.forward) == want, "stacks on the composition: %d" % (want - len(calls.forward))
        assert len(calls.backward) == want
        assert all(block is not None for block, _ in calls.forward + calls.backward)
        assert run["tape"].shapes() == off["tape"].shapes()              # the same ReLU sites, fused or not


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_switch_on_error_within_four_times_switch_off(cuda, case):
    c = _case(case, cuda)
    e_off = _run(c, "off")["e"]
    failures = {}
    for name in SETS:
        run = _run(c, name)
        failed = _report(case, name, run["e"], e_off)
        print("    mask elements differing from the all-off run: %d of %d" % (
            run["tape"].differing(_run(c, "off")["tape"]), run["tape"].elements()))
        if failed:
            failures[name] = failed
    assert not failures, "(tensor, block, e, bound) above the rule, per switch set: %s" % failures


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_two_six_on_steps_are_bit_equal(cuda, case):
    c = _case(case, cuda)
    first, second = _run(c, "six")["result"], _fp32_step(c, SETS["six"])[0]
    names = [] if torch.equal(first["out"], second["out"]) else ["out"]
    names += ["grad:" + n for n, g in first["grads"].items() if not torch.equal(g, second["grads"][n])]
    names += ["record:" + n for n, r in first["records"].items() if not torch.equal(r, second["records"][n])]
    assert not names, "two six-on steps differ at %d tensors %s" % (len(names), names[:8])


def test_the_judge_catches_a_scaled_grad_e(cuda):
    """grad_e of ONE backward call of the six-on run of (relu, surface) times 1 + 1e-3, in Python: the call with the
    largest |grad_e| -- one whose embedding has a gradient that is not rounding noise (behind a one-channel-per-group
    norm it would be)."""
    c = _case("relu-surface", cuda)
    e_off = _run(c, "off")["e"]
    base = _run(c, "six")
    assert not TC.judge(base["e"], e_off)[0]                             # (the unseeded run passes)
    sizes = [(size or 0.0) for _, size in base["calls"].backward]
    n = max(range(len(sizes)), key=sizes.__getitem__)
    block = base["calls"].backward[n][0]
    assert sizes[n] > 0 and block is not None
    result, tape, log, calls = _fp32_step(c, SETS["six"], scale={n: 1 + 1e-3})
    assert calls.backward[n][0] == block
    failed = _report("relu-surface", "fault", _errors(c, result, tape, log), e_off)
    print("    backward call %d of %d in %s, |grad_e| %.3g: %s" % (n, len(sizes), block, sizes[n], failed[:4]))
    assert block in {b for _, b, _, _ in failed}, (block, failed[:5])
