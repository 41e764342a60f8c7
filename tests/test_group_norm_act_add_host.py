"""What can be said about pdr_group_norm_act_add without a GPU: the switch, the emulation of grad_e against its bound
(tests/group_norm_act_add_cases.py), that the bound tells two wrong formulas apart, and that the module path with the
switch off still runs inside `float64_ops`, which turns every public `_ext` function it does not know into a raiser."""
import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import Mlp_plus_t_emb
from tests import float64_network as F64
from tests import group_norm_act_add_cases as AC
from tests import group_norm_act_cases as GC

CASES = [(sh, p) for sh in AC.shapes() for p in ("normal", "offset")]
_id = lambda c: "%s-%s" % ("x".join(map(str, c[0])), c[1])


def test_switch_is_off_by_default_checks_its_argument_and_returns_the_previous_value():
    assert _ext._fused_injection is False and pointnet2_ops.is_fused_injection() is False
    for bad in (1, 0, None, "on"):
        with pytest.raises(TypeError):
            pointnet2_ops.set_fused_injection(bad)
    assert pointnet2_ops.is_fused_injection() is False
    try:
        assert pointnet2_ops.set_fused_injection(True) is False
        assert pointnet2_ops.is_fused_injection() is True and _ext._fused_injection is True
        assert pointnet2_ops.set_fused_injection(True) is True
        assert pointnet2_ops.set_fused_injection(False) is True
    finally:
        _ext.set_fused_injection(False)
    # independent of the other five
    for name in F64.SWITCHES:
        assert getattr(_ext, "is_fused_" + name)() is False


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_emulated_grad_e_stays_inside_its_bound(case):
    shape, pattern = case
    gy = GC.make(shape, pattern, True)[3]
    for vec in (1, 4) if shape[2] % 4 == 0 else (1,):
        got = AC.row_sums_emulated(gy, vec)
        assert got.dtype == np.float32 and got.shape == gy.shape[:2]
        err = np.abs(got.astype(np.float64) - AC.row_sums_exact(gy)) / AC.grad_e_bound(gy)
        print(_id(case), "V", vec, "worst error / bound %.3g" % err.max())
        assert not AC.outside(got, gy).any()
    assert not AC.row_sums_emulated(np.zeros_like(gy), 1).view(np.uint32).any()          # +0.0, bit for bit


def test_the_two_families_of_the_emulation_differ_only_in_order():
    gy = GC.make((1, 131, 260, 32), "normal", True)[3]
    a, b = AC.row_sums_emulated(gy, 1), AC.row_sums_emulated(gy, 4)
    assert not AC.outside(a, gy).any() and not AC.outside(b, gy).any()
    assert np.abs(a.astype(np.float64) - b).max() <= 2 * AC.grad_e_bound(gy).max()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_two_wrong_formulas_leave_the_bound_on_most_rows(case):
    """e injected in front of the activation (ReLU and Swish), and grad_e summed from dz instead of grad_y (ReLU)."""
    shape, pattern = case
    x, gamma, beta, gy = GC.make(shape, pattern, True)
    e, _ = AC.terms(shape)
    rows = shape[0] * shape[1]
    for act in ("relu", "swish"):
        ref = GC.reference(shape, x, gamma, beta, gy, act)
        bad = int(AC.outside(AC.grad_e_before_activation(ref, gy, e, act), gy).sum())
        print(_id(case), act, "e before the activation: %d of %d rows outside" % (bad, rows))
        assert bad > rows / 2
    ref = GC.reference(shape, x, gamma, beta, gy, "relu")
    bad = int(AC.outside(AC.grad_e_from_dz(ref), gy).sum())
    print(_id(case), "relu grad_e from dz: %d of %d rows outside" % (bad, rows))
    assert bad > rows / 2


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_mlp_plus_t_emb_runs_inside_float64_ops_with_the_switch_off(dtype):
    """`float64_ops` replaces every public function of `_ext` outside its pass-through list with a raiser -- the new
    switch's setter and getter among them.  The module path reads the variable, so it never meets one."""
    torch.manual_seed(31)
    mod = Mlp_plus_t_emb([35, 64, 64, 64], bn=True, res_connect=True, include_t=True, include_condition=True,
                         include_second_condition=True).to(dtype)
    gen = torch.Generator().manual_seed(32)
    args = [torch.randn(2, 35, 4, 3, generator=gen).to(dtype)] + [torch.randn(2, 128, generator=gen).to(dtype)
                                                                  for _ in range(3)]
    assert _ext._fused_injection is False
    want = mod(*args)
    with F64.float64_ops("oracle", dtype=dtype):
        with pytest.raises(AssertionError):
            _ext.is_fused_injection()                                  # the trap: a raiser stands here now
        got = mod(*args)
        got.sum().backward()
    assert torch.equal(got, want) and mod.fc.weight.grad is not None
    assert _ext.is_fused_injection() is False                          # restored
