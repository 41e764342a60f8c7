"""pdr_query_group_cf / pdr_query_group_cf_grad without a GPU: the host-only plan and workspace size, the documented
order of the argument checks (nothing is launched, no pointer is looked at before its turn), the Python surface's
refusal of CPU tensors and wrong dtypes, the process-wide switch, QueryAndGroup's untouched composition with the switch
off, and a check that the references of tests/query_group_cases.py discriminate: the sequential fp32 emulation of the
stated chain passes the float64 bounds on every row of the table, five plausible wrong implementations are rejected."""
import collections

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from tests import query_group_cases as QC

OK, EINVAL, EUNSUP = _lib.PDR_OK, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED


def test_the_table_covers_what_it_promises():
    cases = QC.CASES
    assert len(set(cases)) == len(cases) >= 300
    seen = lambda f: collections.Counter(getattr(c, f) for c in cases)
    for field, values in (("B", (1, 3)), ("n", (1, 5, 70, 300)), ("m", (1, 3, 17, 70)), ("K", (1, 3, 4, 8, 32, 33, 64)),
                          ("C", (None, 1, 7, 8, 9, 35)), ("flags", QC.FLAGS), ("counts", QC.COUNTS),
                          ("pattern", QC.PATTERNS + ("perm",)), ("offset", (False, True))):
        assert all(seen(field)[v] >= 2 for v in values), (field, seen(field))
    # every pair (family -- vector, scalar by K, scalar by alignment -- x counts mode x flags)
    fam = lambda c: "offset" if c.offset else ("vector" if c.K % 4 == 0 else "scalar")
    pairs = collections.Counter((fam(c), c.counts, c.flags) for c in cases)
    assert len(pairs) == 3 * 4 * 5 and min(pairs.values()) >= 2
    assert any(c.m * c.K > 256 and (c.m * c.K) % 256 for c in cases if QC.family(c) == 1)
    assert any(c.m * c.K > 256 and (c.m * c.K) % 256 for c in cases if QC.family(c) == 0)
    for m in (255, 256, 257):                                # around the builder's long-segment threshold
        assert any(c.m == m and c.K == 1 and c.pattern == "zero" and c.counts is None for c in cases)
        assert any(c.m == m and c.K == 1 and c.pattern == "zero" and c.counts == "zero" for c in cases)
    for c in cases:                                          # flags 0 needs features; no index leaves the cloud
        assert c.C is not None or c.flags & 1


def test_plan_reports_the_family_and_its_grid():
    for c in QC.CASES:
        C, E = c.C or 0, QC.triples(c.flags)
        P, fslabs = c.m * c.K, -(-C // 8)
        for aligned in (1, 0):
            vec = int(c.K % 4 == 0 and aligned == 1)
            want = [vec, -(-(P // 4 if vec else P) // 256), fslabs + (E > 0), fslabs, C + 3 * E, E]
            assert QC.plan(c.n, c.m, c.K, C, c.flags, aligned) == (OK, want), (c, aligned)
    assert QC.plan(300, 17, 32, 35, 7)[1] == [1, 1, 6, 5, 44, 3] and QC.plan(300, 17, 32, 35, 7, 0)[1][:2] == [0, 3]
    assert QC.plan(300, 17, 32, 35, 6)[1][4:] == [35, 0]     # include_* without use_xyz: ignored
    for bad in [(0, 4, 4, 8, 1), (-1, 4, 4, 8, 1), (8, -1, 4, 8, 1), (8, 4, -4, 8, 1), (8, 4, 4, -8, 1), (8, 4, 4, 8, 8),
                (8, 4, 4, 8, -1), (8, 4, 4, 0, 0), (8, 4, 4, 0, 6), (8, 0, 4, 8, 1), (8, 4, 0, 8, 1)]:
        assert QC.plan(*bad)[0] == EINVAL, bad
    assert QC.plan(16385, 4, 4, 8, 1)[0] == EUNSUP and QC.plan(8, 1 << 12, (1 << 10) + 1, 8, 1)[0] == EUNSUP
    assert QC.plan(8, 1 << 12, 1 << 10, 502, 7)[0] == OK and QC.plan(8, 1 << 12, 1 << 10, 503, 7)[0] == EUNSUP and \
 QC.plan(8, 1 << 12, 1 << 10, 512, 1)[0] == EUNSUP
    assert _lib.load().pdr_query_group_cf_plan(8, 4, 4, 8, 1, 1, None) == EINVAL


def test_workspace_is_the_inverse_index_of_m_k_positions_over_n_destinations():
    ws = _lib.load().pdr_scatter_workspace_bytes
    for B, n, m, K in [(1, 1, 1, 1), (3, 300, 17, 32), (2, 5, 257, 1), (32, 1024, 1024, 32), (32, 2048, 2048, 32),
                       (1, 16384, 1 << 12, 1 << 10)]:
        got = QC.workspace_bytes(B, n, m, K)
        assert got == ws(B, m * K, n) and got > 0 and got % 4 == 0, (B, n, m, K)
        # cnt (B, Wcap, n) | nlong (B) | start (B, n + 1) | order (B, P) | rank (B, P) | longlist (B, P / 256), int32
        P = m * K
        wcap = min(64, -(-P // 1024))
        assert got == 4 * B * (wcap * n + 1 + n + 1 + 2 * P + P // 256)
    for none in [(0, 8, 4, 4), (2, 0, 4, 4), (2, 8, 0, 4), (2, 8, 4, 0), (-1, 8, 4, 4), (2, 16385, 4, 4),
                 (2, 8, 1 << 12, (1 << 10) + 1), (65536, 8, 4, 4)]:
        assert QC.workspace_bytes(*none) == 0, none


def test_calls_validate_their_arguments_in_the_documented_order_without_a_gpu():
    lib = _lib.load()
    p = 0x1000                                         # never dereferenced: every call below returns before a launch

    def fwd(B, n, m, K, C, flags, xyz=p, new_xyz=p, feat=p, idx=p, counts=p, out=p, **ignored):
        return lib.pdr_query_group_cf(xyz, new_xyz, feat, idx, counts, B, n, m, K, C, flags, out, None)

    def bwd(B, n, m, K, C, flags, idx=p, counts=p, go=p, gf=p, gx=p, gn=p, ws=p, **ignored):
        return lib.pdr_query_group_cf_grad(idx, counts, go, B, n, m, K, C, flags, gf, gx, gn, ws, None)

    for call in (fwd, bwd):
        # 1. a negative size, no point, a flag word outside 0 .. 7, no channel at all: before anything else
        for bad in [(-1, 8, 4, 4, 8, 1), (1, -8, 4, 4, 8, 1), (1, 0, 4, 4, 8, 1), (1, 8, -4, 4, 8, 1), (1, 8, 4, -4, 8, 1),
                    (1, 8, 4, 4, -8, 1), (1, 8, 4, 4, 8, 8), (1, 8, 4, 4, 8, -1), (1, 8, 4, 4, 0, 0), (1, 8, 4, 4, 0, 6),
                    (0, 8, 4, 4, 8, 9), (0, 0, 4, 4, 8, 1), (0, 8, 4, 4, 0, 4), (-1, 16385, 4, 4, 8, 1)]:
            assert call(*bad) == EINVAL and call(*bad, idx=None) == EINVAL, bad
        # 2. the empty problem: OK, no pointer looked at
        for empty in [(0, 8, 4, 4, 8, 1), (1, 8, 0, 4, 8, 1), (1, 8, 4, 0, 8, 1), (0, 16385, 0, 0, 8, 7),
                      (0, 8, 1 << 20, 1 << 20, 0, 1)]:
            assert call(*empty, xyz=None, new_xyz=None, idx=None, out=None, go=None, gf=None, gx=None, gn=None,
                        ws=None, counts=None) == OK, empty
        # 3. the unsupported sizes, before the pointers
        for big in [(1, 16385, 4, 4, 8, 1), (1, 8, 1 << 12, (1 << 10) + 1, 8, 1), (65536, 8, 4, 4, 8, 1),
                    (512, 8, 1 << 12, 1 << 10, 0, 1), (1, 8, 1 << 12, 1 << 10, 512, 1), (1, 8, 1 << 12, 1 << 10, 503, 7)]:
            assert call(*big) == EUNSUP and call(*big, idx=None, out=None, go=None, gf=None, gx=None, gn=None) == EUNSUP, big
        assert call(1, 8, 1 << 12, 1 << 10, 502, 7, idx=None) == EINVAL         # 511 channels: inside the limit
        # 4. the pointers
        assert call(1, 8, 4, 4, 8, 1, idx=None) == EINVAL
    assert fwd(1, 8, 4, 4, 8, 1, out=None) == EINVAL and fwd(1, 8, 4, 4, 8, 1, xyz=None) == EINVAL
    assert fwd(1, 8, 4, 4, 8, 7, new_xyz=None) == EINVAL
    assert fwd(1, 8, 4, 4, 8, 0, feat=None) == EINVAL and fwd(0, 8, 4, 4, 8, 0, feat=None) == EINVAL   # no channel: step 1
    assert fwd(0, 8, 4, 4, 8, 1, feat=None, out=None) == OK
    assert fwd(1, 8, 1 << 12, 1 << 10, 512, 1, feat=None, idx=None) == EINVAL   # C is ignored without features
    assert bwd(1, 8, 4, 4, 8, 1, go=None) == EINVAL and bwd(1, 8, 4, 4, 8, 1, gf=None, gx=None, gn=None) == EINVAL
    assert bwd(1, 8, 4, 4, 8, 1, ws=None) == EINVAL and bwd(1, 8, 4, 4, 8, 1, ws=p + 2) == EINVAL
    assert bwd(1, 8, 4, 4, 8, 0, gf=None, ws=None, go=None) == EINVAL
    assert bwd(1, 8, 4, 0, 8, 1, gf=None, gx=None, gn=None) == OK
    assert lib.pdr_version() == 200


def test_cpu_tensors_and_wrong_dtypes_are_refused():
    xyz, new_xyz, feat = torch.randn(2, 5, 3), torch.randn(2, 3, 3), torch.randn(2, 7, 5)
    idx, cnt, go = torch.zeros(2, 3, 4, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32), torch.randn(2, 10, 3, 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.query_group(xyz, new_xyz, feat, idx, cnt, 1)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.query_group_grad(idx, cnt, go, 5, 7, 1)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.query_and_group(xyz, new_xyz, feat, idx, cnt, True, False, False)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.query_and_group(xyz, new_xyz, None, idx)
    with pytest.raises(TypeError):
        _ext.query_group(xyz.numpy(), new_xyz, feat, idx, cnt, 1)
    # dtype and shape checks sit behind the device check on a CPU tensor; what can be told without a GPU is that the
    # wrappers go through _req (RuntimeError, never a crash) for every tensor argument
    for bad in (dict(xyz=xyz.double()), dict(idx=idx.long()), dict(counts=cnt.float()), dict(features=feat.half())):
        args = dict(xyz=xyz, new_xyz=new_xyz, features=feat, idx=idx, counts=cnt)
        args.update(bad)
        with pytest.raises(RuntimeError):
            _ext.query_group(args["xyz"], args["new_xyz"], args["features"], args["idx"], args["counts"], 1)
    assert _ext.query_group_flags(True, True, True) == 7 and _ext.query_group_flags(False, True, True) == 6
    assert _ext.query_group_flags(True, False, True) == 5 and _ext.query_group_flags(True) == 1


def test_switch_defaults_to_off_is_type_checked_and_returns_the_previous_value():
    assert _ext.is_fused_grouping() is False and pointnet2_ops.is_fused_grouping() is False
    try:
        assert _ext.set_fused_grouping(True) is False and _ext.is_fused_grouping() is True
        assert pointnet2_ops.set_fused_grouping(True) is True
        assert _ext.set_fused_grouping(False) is True and _ext.is_fused_grouping() is False
        for bad in (None, 1, 0, "on"):
            with pytest.raises(TypeError):
                _ext.set_fused_grouping(bad)
        assert _ext.is_fused_grouping() is False
    finally:
        _ext.set_fused_grouping(False)
    assert _ext.is_fused_group_norm() is False and _ext.is_fused_attention_pool() is False   # the others are their own
    sup = _ext.query_group_supported
    assert sup(32, 1024, 1024, 32, 32, 1) and sup(32, 2048, 2048, 32, 128, 7) and sup(1, 1, 1, 1, None, 1)
    assert not sup(1, 8, 4, 4, None, 0) and not sup(1, 8, 4, 4, 0, 6) and not sup(0, 8, 4, 4, 8, 1)
    assert not sup(1, 16385, 4, 4, 8, 1) and not sup(1, 8, 1 << 12, (1 << 10) + 1, 8, 1) and not sup(1, 8, 4, 4, 8, 8)
    assert sup(1, 8, 1 << 12, 1 << 10, 502, 7) and not sup(1, 8, 1 << 12, 1 << 10, 503, 7)
    for B, n, m, K, C, flags in [(1, 8, 1 << 12, 1 << 10, 502, 7), (1, 8, 1 << 12, 1 << 10, 503, 7), (3, 300, 17, 32, 35, 7),
                                 (65536, 8, 4, 4, 8, 1), (1, 16385, 4, 4, 8, 1)]:      # the predicate is the C check
        rc = _lib.load().pdr_query_group_cf_grad(None, None, None, B, n, m, K, C, flags, None, None, None, None, None)
        assert sup(B, n, m, K, C, flags) == (rc != EUNSUP)


def test_switch_off_runs_exactly_the_composition(monkeypatch):
    """With the switch off QueryAndGroup never reaches the op (it is patched to raise), whatever the tensors are; with
    it on, CPU tensors still take the composition."""
    def boom(*a, **k):
        raise AssertionError("query_and_group reached with the switch off")
    monkeypatch.setattr(pointnet2_utils, "query_and_group", boom)
    grouper = pointnet2_utils.QueryAndGroup(0.5, 4, True, True, True)
    xyz, new_xyz, feat = torch.randn(2, 9, 3), torch.randn(2, 3, 3), torch.randn(2, 7, 9)
    idx = torch.zeros(2, 3, 4, dtype=torch.int32)
    assert _ext.is_fused_grouping() is False
    assert grouper._takes_fused_op(xyz, new_xyz, feat, idx) is False
    try:
        _ext.set_fused_grouping(True)
        assert grouper._takes_fused_op(xyz, new_xyz, feat, idx) is False         # CPU tensors
    finally:
        _ext.set_fused_grouping(False)
    try:
        from tests.oracle_backend import oracle_ops
    except (ImportError, OSError):
        return                                               # no CPU oracle here: the branch condition above stands
    torch.manual_seed(7)
    new_xyz = torch.cat([xyz[:, :2], xyz[:, :1] + 50.0], dim=1)                  # the last ball is empty
    for settings in (False, True):
        prev = _ext.set_fused_grouping(settings)
        try:
            with oracle_ops():
                for subset in (True, False):
                    out, cnt = grouper(xyz, new_xyz, feat, subset=subset, return_counts=True)
                    assert out.shape == (2, 7 + 9, 3, 4) and int(cnt[0, 2]) == 0
                    A = QC.Arrays(xyz.numpy(), new_xyz.numpy(), feat.numpy(), _ext.ball_query(new_xyz, xyz, 0.5, 4)[0].numpy(),
                                  None if subset else cnt.numpy(), None)
                    want = QC.forward_reference(A, 7)
                    # 1 * a + 0 * c of the composition against the reference's select: the same values
                    assert np.array_equal(out.numpy(), want)
        finally:
            _ext.set_fused_grouping(prev)


DISCRIMINATING = [QC.Case(3, 70, 17, 32, 7, 7, "mixed", "random", False), QC.Case(1, 5, 70, 64, 7, 3, "mixed", "random", False),
                  QC.Case(3, 300, 17, 32, 35, 7, "mixed", "random", False)]


def accepted(got, case):
    """What tests/test_query_group_gpu.py asks of the kernel's gradients: the emulation's bits and the float64 bounds."""
    _, _, emu, ref = QC.references(case)
    same = all(np.array_equal(QC.bits(got[k]), QC.bits(emu[k])) for k in QC.OUTPUTS if emu[k] is not None)
    return same and max(QC.worst_ratio(got, ref).values()) <= 1.0


def test_the_emulation_passes_the_float64_bounds_on_every_row():
    worst = collections.defaultdict(float)
    for case in QC.CASES:
        A, fwd, emu, ref = QC.references(case)
        ratios = QC.worst_ratio(emu, ref)
        assert max(ratios.values()) <= 1.0, (case, ratios)
        for k, v in ratios.items():
            worst[k] = max(worst[k], v)
        C, Ctot = case.C or 0, (case.C or 0) + 3 * QC.triples(case.flags)
        assert fwd.shape == (case.B, Ctot, case.m, case.K) and fwd.dtype == np.float32
        assert (emu["gf"] is None) == (case.C is None)
        # a destination no real slot names: exactly +0.0f
        real = np.broadcast_to(((A.counts > 0) if A.counts is not None else np.ones((case.B, case.m), bool))[:, :, None],
                               A.idx.shape)
        for b in range(case.B):
            unused = np.setdiff1d(np.arange(case.n), A.idx[b][real[b]])
            assert not QC.bits(emu["gx"][b, unused]).any()
            if emu["gf"] is not None:
                assert not QC.bits(emu["gf"][b][:, unused]).any()
    print("emulation over bound:", dict(worst))
    assert any(c.pattern == "sparse" and c.n >= 5 for c in QC.CASES)


@pytest.mark.parametrize("variant", QC.VARIANTS)
def test_a_plausible_wrong_implementation_is_rejected(variant):
    for case in DISCRIMINATING:
        A, fwd, emu, ref = QC.references(case)
        assert accepted(emu, case)
        wrong = dict(zip(QC.OUTPUTS, QC.emulate_backward(A, case.flags, variant)))
        assert not accepted(wrong, case), (variant, case)
    if variant == "channel_order":                           # the forward reference tells the two layouts apart too
        A, fwd, _, _ = QC.references(DISCRIMINATING[0])
        C = A.features.shape[1]
        swapped = np.concatenate([fwd[:, C:C + 3], fwd[:, :C], fwd[:, C + 3:]], axis=1)
        assert not np.array_equal(swapped, fwd)
