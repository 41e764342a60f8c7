"""pdr_knn_group_cf / pdr_knn_group_cf_grad without a GPU: the host-only plan and workspace size, the documented order
of the argument checks (nothing is launched, no pointer is looked at before its turn), the Python surface's refusal of
CPU tensors and wrong dtypes, the process-wide switch, group_knn's untouched composition with the switch off, and a
check that the references of tests/knn_group_cases.py discriminate: the sequential fp32 emulation of the stated chain
passes the per-element float64 bounds and the norm-wise cap on every row of the table, six plausible wrong
implementations are rejected."""
import collections

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from tests import knn_group_cases as KC
from tests.oracle_backend import oracle_ops

OK, EINVAL, EUNSUP = _lib.PDR_OK, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED


def test_the_table_covers_what_it_promises():
    cases = KC.CASES
    assert len(set(cases)) == len(cases) >= 150
    seen = lambda f: collections.Counter(getattr(c, f) for c in cases)
    for field, values in (("B", (1, 3)), ("n1", (1, 3, 17, 70, 257)), ("n2", (1, 5, 70, 300)), ("K", (1, 3, 4, 8, 16)),
                          ("C", (None, 1, 7, 8, 9, 35)), ("pattern", KC.PATTERNS), ("offset", (False, True))):
        assert all(seen(field)[v] >= 2 for v in values), (field, seen(field))
    # every pair (family -- vector, scalar by K, scalar by alignment -- x pattern)
    fam = lambda c: "offset" if c.offset else ("vector" if c.K % 4 == 0 else "scalar")
    pairs = collections.Counter((fam(c), c.pattern) for c in cases)
    assert len(pairs) == 3 * 4 and min(pairs.values()) >= 2, pairs
    assert all(c.K % 4 == 0 for c in cases if c.offset)      # the offset rows are scalar by alignment alone
    assert all(KC.family(c) == (fam(c) == "vector") for c in cases)
    for f in (0, 1):                                         # more than one block, the last one partly filled
        assert any(c.n1 * c.K > 256 and (c.n1 * c.K) % 256 for c in cases if KC.family(c) == f)
    for n1 in (255, 256, 257):                               # around the builder's long-segment threshold
        assert any(c.n1 == n1 and c.n2 == 1 and c.K == 1 for c in cases)
    for c in cases:
        assert c.pattern in ("zero", "random") or c.K <= c.n2
    # rows where most points of y are named by no slot
    sparse = [c for c in cases if c.n2 == 300 and c.n1 * c.K <= 51]
    assert len(sparse) >= 4 and {KC.family(c) for c in sparse} == {0, 1}
    for c in sparse:
        A = KC.references(c)[0]
        assert all(np.unique(A.idx[b]).size <= c.n2 // 4 for b in range(c.B))
    # the coincident rows have exact zero distances, the others none
    for c in cases[::7]:
        A = KC.references(c)[0]
        if c.pattern == "coincident":
            assert (A.dists[:, ::2, 0] == 0).all()
        assert A.idx.dtype == np.int32 and A.dists.dtype == np.float32 and (A.dists >= 0).all()


def test_plan_reports_the_family_and_its_grid():
    for c in KC.CASES:
        C = c.C or 0
        P, fslabs = c.n1 * c.K, -(-C // 8)
        for aligned in (1, 0):
            vec = int(c.K % 4 == 0 and aligned == 1)
            want = [vec, -(-(P // 4 if vec else P) // 256), fslabs + 1, fslabs, C + 11]
            assert KC.plan(c.n1, c.n2, c.K, C, aligned) == (OK, want), (c, aligned)
    assert KC.plan(70, 300, 8, 35)[1] == [1, 1, 6, 5, 46] and KC.plan(70, 300, 8, 35, 0)[1][:2] == [0, 3]
    assert KC.plan(2048, 1024, 8, 160)[1] == [1, 16, 21, 20, 171]
    for bad in [(4, 0, 4, 8), (4, -1, 4, 8), (-1, 8, 4, 8), (4, 8, -4, 8), (4, 8, 4, -8), (0, 8, 4, 8), (4, 8, 0, 8)]:
        assert KC.plan(*bad)[0] == EINVAL, bad
    assert KC.plan(4, 16385, 4, 8)[0] == EUNSUP and KC.plan(1 << 12, 8, (1 << 10) + 1, 8)[0] == EUNSUP
    assert KC.plan(1 << 12, 8, 1 << 10, 500)[0] == OK and KC.plan(1 << 12, 8, 1 << 10, 501)[0] == EUNSUP
    # the channel slabs are grid.y: 65534 feature slabs and the geometric one
    assert KC.plan(1, 1, 1, 8 * 65534)[1] == [0, 1, 65535, 65534, 8 * 65534 + 11] and KC.plan(1, 1, 1, 8 * 65534 + 1)[0] == EUNSUP
    assert _lib.load().pdr_knn_group_cf_plan(4, 8, 4, 8, 1, None) == EINVAL


def test_workspace_is_the_inverse_index_of_n1_k_positions_over_n2_destinations():
    ws = _lib.load().pdr_scatter_workspace_bytes
    for B, n1, n2, K in [(1, 1, 1, 1), (3, 70, 300, 8), (2, 257, 1, 1), (32, 64, 16, 8), (32, 2048, 1024, 8),
                         (1, 1 << 12, 16384, 1 << 10)]:
        got = KC.workspace_bytes(B, n1, n2, K)
        assert got == ws(B, n1 * K, n2) and got > 0 and got % 4 == 0, (B, n1, n2, K)
    for none in [(0, 4, 8, 4), (2, 4, 0, 4), (2, 0, 8, 4), (2, 4, 8, 0), (-1, 4, 8, 4), (2, 4, 16385, 4),
                 (2, 1 << 12, 8, (1 << 10) + 1), (65536, 4, 8, 4)]:
        assert KC.workspace_bytes(*none) == 0, none


def test_calls_validate_their_arguments_in_the_documented_order_without_a_gpu():
    lib = _lib.load()
    p = 0x1000                                         # never dereferenced: every call below returns before a launch

    def fwd(B, n1, n2, K, C, x=p, y=p, feat=p, idx=p, dists=p, out=p, **ignored):
        return lib.pdr_knn_group_cf(x, y, feat, idx, dists, B, n1, n2, K, C, out, None)

    def bwd(B, n1, n2, K, C, x=p, y=p, idx=p, dists=p, go=p, gf=p, gx=p, gy=p, ws=p, **ignored):
        return lib.pdr_knn_group_cf_grad(x, y, idx, dists, go, B, n1, n2, K, C, gf, gx, gy, ws, None)

    for call in (fwd, bwd):
        # 1. a negative size, no point to search in: before anything else
        for bad in [(-1, 4, 8, 4, 8), (1, -4, 8, 4, 8), (1, 4, -8, 4, 8), (1, 4, 0, 4, 8), (1, 4, 8, -4, 8),
                    (1, 4, 8, 4, -8), (0, 4, 0, 4, 8), (0, 0, -1, 0, 8), (-1, 4, 16385, 4, 8)]:
            assert call(*bad) == EINVAL and call(*bad, idx=None) == EINVAL, bad
        # 2. the empty problem: OK, no pointer looked at
        for empty in [(0, 4, 8, 4, 8), (1, 0, 8, 4, 8), (1, 4, 8, 0, 8), (0, 0, 16385, 0, 8), (0, 1 << 20, 8, 1 << 20, 0)]:
            assert call(*empty, x=None, y=None, idx=None, dists=None, out=None, go=None, gf=None, gx=None, gy=None,
                        ws=None) == OK, empty
        # 3. the unsupported sizes, before the pointers
        for big in [(1, 4, 16385, 4, 8), (1, 1 << 12, 8, (1 << 10) + 1, 8), (65536, 4, 8, 4, 8),
                    (512, 1 << 12, 8, 1 << 10, 0), (1, 1 << 12, 8, 1 << 10, 501), (1, 1, 1, 1, 8 * 65534 + 1)]:
            assert call(*big) == EUNSUP, big
            assert call(*big, x=None, idx=None, dists=None, out=None, go=None, gf=None, gx=None, gy=None) == EUNSUP, big
        assert call(1, 1 << 12, 8, 1 << 10, 500, idx=None) == EINVAL             # 511 channels: inside the limit
        assert call(1, 1, 1, 1, 8 * 65534, idx=None) == EINVAL                   # 65535 slabs: inside the limit
        # 4. the pointers
        for name in ("x", "y", "idx", "dists"):
            assert call(1, 4, 8, 4, 8, **{name: None}) == EINVAL, name
    assert fwd(1, 4, 8, 4, 8, out=None) == EINVAL
    assert fwd(0, 4, 8, 4, 8, feat=None, out=None) == OK
    assert fwd(1, 1 << 12, 8, 1 << 10, 501, feat=None, idx=None) == EINVAL       # C is ignored without features
    assert fwd(1, 4, 8, 4, -8, feat=None) == EINVAL                              # but a negative C is step 1
    assert bwd(1, 4, 8, 4, 8, go=None) == EINVAL and bwd(1, 4, 8, 4, 8, gf=None, gx=None, gy=None) == EINVAL
    assert bwd(1, 4, 8, 4, 8, ws=None) == EINVAL and bwd(1, 4, 8, 4, 8, ws=p + 2) == EINVAL
    assert bwd(1, 4, 8, 4, 0, gx=None, gy=None, ws=None, go=None) == EINVAL
    assert bwd(1, 4, 8, 0, 8, gf=None, gx=None, gy=None) == OK
    assert lib.pdr_version() == 200


def test_cpu_tensors_and_wrong_dtypes_are_refused():
    x, y, feat = torch.randn(2, 3, 3), torch.randn(2, 5, 3), torch.randn(2, 7, 5)
    idx, d, go = torch.zeros(2, 3, 4, dtype=torch.int32), torch.rand(2, 3, 4), torch.randn(2, 18, 3, 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.knn_group_cf(x, y, feat, idx, d)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.knn_group_cf_grad(x, y, idx, d, go, 7)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.knn_and_group(x, y, feat, idx, d)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.knn_and_group(x, y, None, idx, d)
    with pytest.raises(TypeError):
        _ext.knn_group_cf(x.numpy(), y, feat, idx, d)
    # dtype and shape checks sit behind the device check on a CPU tensor; what can be told without a GPU is that the
    # wrappers go through _req (RuntimeError, never a crash) for every tensor argument
    for bad in (dict(x=x.double()), dict(idx=idx.long()), dict(dists=d.double()), dict(features=feat.half())):
        args = dict(x=x, y=y, features=feat, idx=idx, dists=d)
        args.update(bad)
        with pytest.raises(RuntimeError):
            _ext.knn_group_cf(args["x"], args["y"], args["features"], args["idx"], args["dists"])


def test_switch_defaults_to_off_is_type_checked_and_returns_the_previous_value():
    assert _ext.is_fused_knn_grouping() is False and pointnet2_ops.is_fused_knn_grouping() is False
    try:
        assert _ext.set_fused_knn_grouping(True) is False and _ext.is_fused_knn_grouping() is True
        assert pointnet2_ops.set_fused_knn_grouping(True) is True
        assert _ext.is_fused_grouping() is False             # the others are their own
        assert _ext.set_fused_knn_grouping(False) is True and _ext.is_fused_knn_grouping() is False
        for bad in (None, 1, 0, "on"):
            with pytest.raises(TypeError):
                _ext.set_fused_knn_grouping(bad)
        assert _ext.is_fused_knn_grouping() is False
    finally:
        _ext.set_fused_knn_grouping(False)
    assert _ext.is_fused_group_norm() is False and _ext.is_fused_attention_pool() is False
    sup = _ext.knn_group_cf_supported
    assert sup(32, 64, 16, 8, 640) and sup(32, 2048, 1024, 8, 160) and sup(1, 1, 1, 1, None)
    assert not sup(0, 4, 8, 4, 8) and not sup(1, 4, 0, 4, 8) and not sup(1, 4, 8, 0, 8) and not sup(1, 4, 8, 4, -1)
    assert not sup(1, 4, 16385, 4, 8) and not sup(1, 1 << 12, 8, (1 << 10) + 1, 8) and not sup(65536, 4, 8, 4, 8)
    assert sup(1, 1 << 12, 8, 1 << 10, 500) and not sup(1, 1 << 12, 8, 1 << 10, 501)
    assert sup(1, 1, 1, 1, 8 * 65534) and not sup(1, 1, 1, 1, 8 * 65534 + 1)
    for B, n1, n2, K, C in [(1, 1 << 12, 8, 1 << 10, 500), (1, 1 << 12, 8, 1 << 10, 501), (3, 70, 300, 8, 35),
                            (65536, 4, 8, 4, 8), (1, 4, 16385, 4, 8), (1, 1, 1, 1, 8 * 65534),
                            (1, 1, 1, 1, 8 * 65534 + 1)]:                              # the predicate is the C check
        rc = _lib.load().pdr_knn_group_cf_grad(None, None, None, None, None, B, n1, n2, K, C, None, None, None, None, None)
        assert sup(B, n1, n2, K, C) == (rc != EUNSUP)


def test_switch_off_runs_exactly_the_composition(monkeypatch):
    """With the switch off group_knn reaches none of the new functions (they are patched to raise), whatever the
    tensors are; with it on, CPU tensors, transpose=False and K > n2 still take the composition."""
    def boom(*a, **k):
        raise AssertionError("a function of the fused kNN grouping was reached")
    monkeypatch.setattr(pointnet2_utils, "knn_and_group", boom)
    monkeypatch.setattr(pointnet2_utils.KnnGroup, "forward", staticmethod(boom))
    for name in ("knn_group_cf", "knn_group_cf_grad", "knn_group_cf_supported", "knn_group"):
        monkeypatch.setattr(_ext, name, boom)
    x, y, feat = torch.randn(2, 6, 3), torch.randn(2, 9, 3), torch.randn(2, 7, 9)
    assert _ext.is_fused_knn_grouping() is False
    with oracle_ops():
        out = pointnet2_utils.group_knn(x, y, feat, 4, transpose=True)
        flat = pointnet2_utils.group_knn(x, y, feat.transpose(1, 2).contiguous(), 4)
    assert out.shape == (2, 7 + 11, 6, 4) and not out.is_contiguous()
    assert torch.equal(flat.transpose(2, 3).transpose(1, 2), out)
    idx = torch.topk(((x[:, :, None] - y[:, None]) ** 2).sum(-1), 4, dim=2, largest=False).indices
    A = KC.Arrays(x.numpy(), y.numpy(), feat.numpy(), idx.int().numpy(), out[:, 7].numpy(), None)
    want = KC.forward_reference(A)
    keep = [c for c in range(18) if c != 8]                  # the composition's w is torch's sum, not the stated chain
    assert np.array_equal(out.numpy()[:, keep], want[:, keep])
    assert np.allclose(out.numpy()[:, 8], want[:, 8], rtol=(4 + 3) * 2.0 ** -24, atol=0)
    # with the switch on: the predicate itself (restored) sends these to the composition without touching the op
    monkeypatch.undo()
    for name in ("knn_group_cf", "knn_group_cf_grad", "knn_group"):
        monkeypatch.setattr(_ext, name, boom)
    monkeypatch.setattr(pointnet2_utils, "knn_and_group", boom)
    takes = pointnet2_utils._group_knn_takes_fused_op
    assert takes(x, y, feat, 4, True) is False               # the switch is off
    try:
        _ext.set_fused_knn_grouping(True)
        assert takes(x, y, feat, 4, True) is False           # CPU tensors
        assert takes(x.double(), y.double(), feat.double(), 4, True) is False
        with oracle_ops():
            assert pointnet2_utils.group_knn(x, y, feat, 4, transpose=True).shape == (2, 18, 6, 4)
    finally:
        _ext.set_fused_knn_grouping(False)


DISCRIMINATING = [KC.Case(3, 70, 300, 8, 35, "knn", False), KC.Case(3, 70, 300, 8, 35, "coincident", False),
                  KC.Case(1, 257, 70, 3, 9, "random", False)]


def accepted(got, case):
    """What tests/test_knn_group_cf_gpu.py asks of the kernel's gradients: the emulation's bits, the per-element
    float64 bounds and the norm-wise cap."""
    _, _, emu, ref = KC.references(case)
    same = all(np.array_equal(KC.bits(got[k]), KC.bits(emu[k])) for k in KC.OUTPUTS if emu[k] is not None)
    return same and max(KC.worst_ratio(got, ref).values()) <= 1.0 and max(KC.norm_error(got, ref).values()) <= KC.CAP


def test_the_emulation_passes_the_float64_bounds_and_the_cap_on_every_row():
    worst, worst_norm = collections.defaultdict(float), collections.defaultdict(float)
    for case in KC.CASES:
        A, fwd, emu, ref = KC.references(case)
        ratios, norms = KC.worst_ratio(emu, ref), KC.norm_error(emu, ref)
        assert max(ratios.values()) <= 1.0, (case, ratios)
        assert max(norms.values()) <= KC.CAP, (case, norms)
        for k in ratios:
            worst[k], worst_norm[k] = max(worst[k], ratios[k]), max(worst_norm[k], norms[k])
        assert fwd.shape == (case.B, (case.C or 0) + 11, case.n1, case.K) and fwd.dtype == np.float32
        assert (emu["gf"] is None) == (case.C is None)
        assert set(ratios) == set(norms) == {k for k in KC.OUTPUTS if emu[k] is not None}
        # a point of y no slot names: exactly +0.0f
        for b in range(case.B):
            unused = np.setdiff1d(np.arange(case.n2), A.idx[b])
            assert not KC.bits(emu["gy"][b, unused]).any()
            if emu["gf"] is not None:
                assert not KC.bits(emu["gf"][b][:, unused]).any()
    print("emulation over bound:", dict(worst), "over the largest reference value:", dict(worst_norm))


SCALED = [c for c in KC.CASES if c.n1 >= 17 and c.n2 >= 5][::6]


def test_the_emulation_passes_bounds_and_cap_with_coordinates_scaled_by_a_twentieth():
    """Part of the cap's stated basis: x and y times 0.05, so squared distances are 400 times smaller and the weights'
    reciprocals that much larger."""
    assert len(SCALED) >= 12 and {c.pattern for c in SCALED} == set(KC.PATTERNS)
    worst = collections.defaultdict(float)
    for case in SCALED:
        A = KC.make(case, scale=0.05)
        assert np.abs(A.x).max() < 0.3 and A.dists.max() < 0.3
        emu, ref = dict(zip(KC.OUTPUTS, KC.emulate_backward(A))), KC.reference64(A)
        ratios, norms = KC.worst_ratio(emu, ref), KC.norm_error(emu, ref)
        assert max(ratios.values()) <= 1.0, (case, ratios)
        assert max(norms.values()) <= KC.CAP, (case, norms)
        for k in norms:
            worst[k] = max(worst[k], norms[k])
    print("scaled by 0.05, emulation over the largest reference value:", dict(worst))


def test_the_forward_reference_is_the_weight_of_the_torch_expression():
    """The numpy chain against group_knn's torch expression in float64 fed the same fp32 distances: (K + 3) 2^-24
    relative (K - 1 adds, three more roundings), the bound tests/test_assembly_gpu.py uses for this weight."""
    for case in KC.CASES[::5]:
        A, fwd, _, _ = KC.references(case)
        C = case.C or 0
        leaf = lambda a: None if a is None else torch.tensor(a).double()
        want = KC.composition(leaf(A.x), leaf(A.y), leaf(A.features), torch.tensor(A.idx), leaf(A.dists)).numpy()
        copies = [c for c in range(C + 11) if c != C + 1 and not C + 5 <= c < C + 8]
        assert np.array_equal(fwd[:, copies], want[:, copies])
        rel_want = want[:, C + 5:C + 8]                      # nn_rel: one rounded subtraction
        assert (np.abs(fwd[:, C + 5:C + 8] - rel_want) <= 2.0 ** -24 * np.abs(rel_want)).all()
        rel = np.abs(fwd[:, C + 1] - want[:, C + 1]) / want[:, C + 1]
        assert rel.max() <= (case.K + 3) * 2.0 ** -24, (case, rel.max())


@pytest.mark.parametrize("variant", KC.VARIANTS)
def test_a_plausible_wrong_implementation_is_rejected(variant):
    for case in DISCRIMINATING:
        A, fwd, emu, ref = KC.references(case)
        assert accepted(emu, case)
        wrong = dict(zip(KC.OUTPUTS, KC.emulate_backward(A, variant)))
        assert not accepted(wrong, case), (variant, case)
        if variant != "descending":                          # a wrong formula is far outside the cap, not only off by bits
            assert max(KC.norm_error(wrong, ref).values()) > 1e3 * KC.CAP, (variant, case)
            assert max(KC.worst_ratio(wrong, ref).values()) > 1e3, (variant, case)
    if variant == "w_from_distance":                         # the forward reference tells the two weights apart too
        A, fwd, _, _ = KC.references(DISCRIMINATING[0])
        assert not np.array_equal(KC.forward_reference(A, variant), fwd)
