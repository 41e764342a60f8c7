"""pdr_attention_pool_cf / pdr_attention_pool_cf_grad without a GPU: the host-only plan, the documented order of the
argument checks (nothing is launched, no pointer is looked at before its turn), the Python surface's refusal of CPU
tensors, the process-wide switch, and AttentionModule's unchanged bits with the switch off."""
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.attention import AttentionModule
from tests import attention_pool_cf_cases as AC

OK, EINVAL, EUNSUP = _lib.PDR_OK, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED


def test_plan_reports_family_and_lanes_per_row():
    for K, L in [(4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (12, 4), (20, 8), (40, 16)]:
        assert AC.plan(K, 1) == (OK, [1, L, 256 // L, 0]), K
    for K in (1, 3, 33, 63):
        assert AC.plan(K, 1) == (OK, [0, 1, 256, 0]), K
    for K in range(1, 65):
        assert AC.plan(K, 0) == (OK, [0, 1, 256, 0]), K
        rc, p = AC.plan(K, 1)
        assert rc == OK and p[0] == int(K % 4 == 0) and p[1] * p[2] == 256 and 4 * p[1] >= K * p[0]
        assert p[1] == 1 or 2 * p[1] < K                       # the smallest power of two that holds K / 4 float4
    for K in (0, -1, -64):
        assert AC.plan(K, 1)[0] == EINVAL
    assert AC.plan(65, 1)[0] == EUNSUP and AC.plan(65, 0)[0] == EUNSUP and AC.plan(1 << 20, 1)[0] == EUNSUP
    assert _lib.load().pdr_attention_pool_cf_plan(8, 1, None) == EINVAL


def test_calls_validate_their_arguments_in_the_documented_order_without_a_gpu():
    lib = _lib.load()
    p = 0x1000                                         # never dereferenced: every call below returns before a launch
    fwd = lambda B, C, N, K, s=p, v=p, o=p, cnt=p: lib.pdr_attention_pool_cf(s, v, cnt, B, C, N, K, o, None)
    bwd = lambda B, C, N, K, s=p, v=p, g=p, gs=p, gv=p, cnt=p: lib.pdr_attention_pool_cf_grad(s, v, cnt, g, B, C, N, K, gs,
                                                                                             gv, None)
    for call in (fwd, bwd):
        # 1. a negative size or K <= 0, before anything else (NULL pointers, K beyond 64 elsewhere in the call)
        assert call(-1, 2, 3, 8) == EINVAL and call(1, -2, 3, 8) == EINVAL and call(1, 2, -3, 8) == EINVAL
        assert call(1, 2, 3, 0) == EINVAL and call(1, 2, 3, -8) == EINVAL
        assert call(-1, 2, 3, 65) == EINVAL and call(0, 2, 3, 0) == EINVAL and call(-1, 2, 3, 8, s=None) == EINVAL
        # 2. an empty problem: OK, no pointer looked at -- K > 64 is not looked at either
        for shape in ((0, 2, 3, 8), (1, 0, 3, 8), (1, 2, 0, 8), (0, 0, 0, 65)):
            assert call(*shape, s=None, v=None, cnt=None) == OK, shape
        # 3. sizes the kernels do not take, before the pointers
        assert call(1, 2, 3, 65) == EUNSUP and call(1, 2, 3, 65, s=None) == EUNSUP
        assert call(4096, 512, 1024, 1) == EUNSUP and call(4096, 512, 1024, 1, v=None) == EUNSUP      # 2^31 elements
        assert call(1 << 16, 1 << 16, 1 << 16, 64) == EUNSUP and call((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 1) == EUNSUP
        assert call(1 << 20, 1, 32, 64) == EUNSUP                                                     # 2^31 with K
        # 4. NULL pointers
        assert call(1, 2, 3, 8, s=None) == EINVAL and call(1, 2, 3, 8, v=None) == EINVAL
    assert fwd(1, 2, 3, 8, o=None) == EINVAL
    assert fwd(0, 2, 3, 8, o=None) == OK
    assert bwd(1, 2, 3, 8, g=None) == EINVAL
    assert bwd(1, 2, 3, 8, gs=None, gv=None) == EINVAL
    assert bwd(1, 2, 3, 65, gs=None, gv=None) == EUNSUP and bwd(1, 0, 3, 8, g=None, gs=None, gv=None) == OK


def test_cpu_tensors_are_refused():
    s, v = torch.randn(1, 2, 3, 4), torch.randn(1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.attention_pool(s, v, None)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.attention_pool_grad(s, v, 'all', torch.randn(1, 2, 3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.attention_pool(s, v, torch.ones(1, 3, dtype=torch.int32))


def test_switch_defaults_to_off_and_round_trips():
    assert _ext.is_fused_attention_pool() is False and pointnet2_ops.is_fused_attention_pool() is False
    try:
        assert _ext.set_fused_attention_pool(True) is False and _ext.is_fused_attention_pool() is True
        assert pointnet2_ops.set_fused_attention_pool(True) is True
        assert _ext.set_fused_attention_pool(False) is True and _ext.is_fused_attention_pool() is False
        for bad in (None, 1, "on"):
            with pytest.raises(TypeError):
                _ext.set_fused_attention_pool(bad)
        assert _ext.is_fused_attention_pool() is False
    finally:
        _ext.set_fused_attention_pool(False)
    assert _ext.attention_pool_supported(32, 64, 512, 64) and not _ext.attention_pool_supported(1, 2, 3, 65)
    assert not _ext.attention_pool_supported(4096, 512, 1024, 1)


@pytest.mark.parametrize("count", ["tensor", "all"])
def test_module_on_cpu_tensors_gives_the_composition_s_bits(count):
    """With the switch off -- and, CPU tensors never being fused, with it on -- AttentionModule.forward is the
    composition of attention.py:71-77, written out here, bit for bit."""
    torch.manual_seed(5)
    B, N, K = 2, 20, 8
    mod = AttentionModule(8, 11, 8, 11, 32)
    feat, gf, gfo = torch.randn(B, 8, N), torch.randn(B, 11, N, K), torch.randn(B, 32, N, K)
    cnt = 'all' if count == "all" else torch.randint(0, K + 1, (B, N), dtype=torch.int32)
    with torch.no_grad():
        q = mod.feat_conv(feat.unsqueeze(-1)).expand(-1, -1, -1, K)
        scores = mod.weight_conv(torch.cat([q, mod.grouped_feat_conv(gf)], dim=1))
        want = AC.composition(scores, mod.feat_out_conv(gfo.clone()), None if count == "all" else cnt)
        got_off = mod(feat, gf, gfo.clone(), cnt)
        prev = _ext.set_fused_attention_pool(True)
        try:
            got_on = mod(feat, gf, gfo.clone(), cnt)
        finally:
            _ext.set_fused_attention_pool(prev)
    assert want.shape == (B, 32, N)
    as_bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(as_bits(got_off), as_bits(want)) and torch.equal(as_bits(got_on), as_bits(want))
