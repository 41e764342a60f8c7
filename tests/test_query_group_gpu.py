"""pdr_query_group_cf / pdr_query_group_cf_grad on the GPU, through _ext.query_group / query_group_grad (thin wrappers
of the two C calls), pointnet2_utils.query_and_group and QueryAndGroup under set_fused_grouping.

References and bounds: tests/query_group_cases.py.  Every row of its table: the forward is array_equal with the numpy
fp32 composition; the three gradients have the bits of the sequential fp32 emulation of the stated chain and lie within
the per-element bounds around the float64 autograd of the composition; nothing is excluded.

Module level the switch changes no forward bit (asserted), so what separates switch on from switch off is the order of
the backward's sums.  The two tiny modules are held against their float64 evaluation (`double_ops`: a double copy whose
index ops see the fp32 coordinates and whose gathers are differentiable torch indexing, the idea of
tests/float64_network.py with gradients) with the attention-pool and GroupNorm switches on in both runs and the
grouping switch on / off: the switch-on error may exceed the switch-off error by no more than a factor of 2."""
import copy

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from point_diffusion_refinement_amd.pointnet2_ops.pointnet2_modules import FeatureMapModule, PointnetSAModule
from tests import query_group_cases as QC

pytestmark = pytest.mark.gpu

bits = QC.bits


def dev(a, cuda, offset=False):
    """Device copy of a host array; offset=True: a contiguous view 4 bytes into its storage."""
    if a is None:
        return None
    t = torch.tensor(np.asarray(a))                    # a copy: the cached host arrays are read-only
    if not offset:
        return t.to(cuda)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def forward(A, case, cuda):
    out = None
    if case.offset:
        out = dev(np.zeros(A.grad_out.shape, np.float32), cuda, offset=True)
    got = _ext.query_group(dev(A.xyz, cuda), dev(A.new_xyz, cuda), dev(A.features, cuda), dev(A.idx, cuda),
                           dev(A.counts, cuda), case.flags, out=out)
    assert (got.data_ptr() % 16 == 0) == (not case.offset)
    return got


def backward(A, case, cuda, need=(True, True, True)):
    """{gf, gx, gn} of one pdr_query_group_cf_grad call as host arrays (a gradient not asked for: None)."""
    got = _ext.query_group_grad(dev(A.idx, cuda), dev(A.counts, cuda), dev(A.grad_out, cuda, case.offset),
                                case.n, case.C or 0, case.flags, *need)
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu().numpy() for k, t in zip(QC.OUTPUTS, got)}


@pytest.mark.parametrize("case", QC.CASES, ids=QC.case_id)
def test_forward_bits_backward_bits_and_float64_bounds(cuda, case):
    A, fwd, emu, ref = QC.references(case)
    assert QC.plan(case.n, case.m, case.K, case.C or 0, case.flags, int(not case.offset))[1][0] == QC.family(case)
    out = forward(A, case, cuda).cpu().numpy()
    assert out.shape == fwd.shape and np.array_equal(out, fwd)
    assert np.array_equal(bits(out), bits(fwd))              # finite inputs: the copies keep even the sign of zero
    got = backward(A, case, cuda)
    worst = QC.worst_ratio(got, ref)
    print(QC.case_id(case), " ".join("%s %.3g" % kv for kv in worst.items()))
    for k in QC.OUTPUTS:
        assert (got[k] is None) == (emu[k] is None), k
        assert got[k] is None or np.array_equal(bits(got[k]), bits(emu[k])), k
    assert max(worst.values()) <= 1.0, worst
    # each gradient alone: the other two pointers are NULL
    for i, k in enumerate(QC.OUTPUTS):
        if emu[k] is None:
            continue
        alone = backward(A, case, cuda, need=tuple(j == i for j in range(3)))
        assert all((alone[o] is None) == (o != k) for o in QC.OUTPUTS)
        assert np.array_equal(bits(alone[k]), bits(emu[k])), k


BATCHED = [c for c in QC.CASES if c.B == 3][::4]


@pytest.mark.parametrize("case", BATCHED, ids=QC.case_id)
def test_same_bits_run_after_run_and_for_a_cloud_alone(cuda, case):
    A = QC.references(case)[0]
    first, second = backward(A, case, cuda), backward(A, case, cuda)
    for k in QC.OUTPUTS:
        assert first[k] is None or np.array_equal(bits(first[k]), bits(second[k])), k
    one = lambda a: None if a is None else np.ascontiguousarray(a[1:2])
    A1 = QC.Arrays(*(one(a) for a in A))
    c1 = case._replace(B=1)
    assert np.array_equal(bits(forward(A1, c1, cuda)), bits(forward(A, case, cuda))[1:2])
    alone = backward(A1, c1, cuda)
    for k in QC.OUTPUTS:
        assert first[k] is None or np.array_equal(bits(alone[k]), bits(first[k][1:2])), k


def test_wrong_dtypes_and_shapes_are_refused(cuda):
    A = QC.references(QC.Case(3, 70, 17, 32, 7, 7, "mixed", "random", False))[0]
    ok = dict(xyz=dev(A.xyz, cuda), new_xyz=dev(A.new_xyz, cuda), features=dev(A.features, cuda), idx=dev(A.idx, cuda),
              counts=dev(A.counts, cuda))
    for bad in (dict(xyz=ok["xyz"].double()), dict(idx=ok["idx"].long()), dict(counts=ok["counts"].float()),
                dict(features=ok["features"].half()), dict(features=ok["features"][:, :, :5].contiguous()),
                dict(counts=ok["counts"][:, :3].contiguous()), dict(new_xyz=ok["new_xyz"][:2].contiguous()),
                dict(xyz=ok["xyz"].transpose(1, 2))):
        args = dict(ok)
        args.update(bad)
        with pytest.raises(RuntimeError):
            _ext.query_group(args["xyz"], args["new_xyz"], args["features"], args["idx"], args["counts"], 7)
    go = dev(A.grad_out, cuda)
    with pytest.raises(RuntimeError):
        _ext.query_group_grad(ok["idx"], ok["counts"], go, 70, 7, 3)            # flags do not match the channels
    with pytest.raises(RuntimeError):
        _ext.query_group_grad(ok["idx"], ok["counts"], go, 70, 7, 7, False, False, False)
    with pytest.raises(RuntimeError):
        _ext.query_group(ok["xyz"], ok["new_xyz"], None, ok["idx"], None, 0)    # no channel at all


def test_the_function_saves_indices_only_and_honours_needs_input_grad(cuda):
    case = QC.Case(3, 70, 17, 32, 7, 7, "mixed", "random", False)
    A, fwd, emu, _ = QC.references(case)
    leaf = lambda a, g: dev(a, cuda).requires_grad_(g)
    for needs in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        xyz, new_xyz, feat = leaf(A.xyz, needs[0]), leaf(A.new_xyz, needs[1]), leaf(A.features, needs[2])
        out = pointnet2_utils.query_and_group(xyz, new_xyz, feat, dev(A.idx, cuda), dev(A.counts, cuda), True, True, True)
        assert np.array_equal(bits(out), bits(fwd))
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 2 and all(not t.is_floating_point() for t in saved)
        go = dev(A.grad_out, cuda)
        out.backward(go.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))   # a non-contiguous grad_out
        for t, k, need in ((xyz, "gx", needs[0]), (new_xyz, "gn", needs[1]), (feat, "gf", needs[2])):
            assert (t.grad is not None) == need
            assert not need or np.array_equal(bits(t.grad), bits(emu[k])), k
    out = pointnet2_utils.query_and_group(dev(A.xyz, cuda), dev(A.new_xyz, cuda), None, dev(A.idx, cuda))
    assert out.shape == (3, 3, 17, 32) and out.grad_fn is None


# ---- QueryAndGroup under the switch ----------------------------------------------------------------------------------
def both(fn):
    prev = _ext.set_fused_grouping(False)
    try:
        off = fn()
        _ext.set_fused_grouping(True)
        on = fn()
    finally:
        _ext.set_fused_grouping(prev)
    return off, on


def module_clouds(cuda, n=300, m=70):
    gen = torch.Generator().manual_seed(31)
    xyz = torch.rand(2, n, 3, generator=gen)
    new_xyz = xyz[:, torch.randperm(n, generator=gen)[:m]] + 0.02 * torch.randn(2, m, 3, generator=gen)
    new_xyz[:, ::9] += 50.0                                  # a few queries far outside the cloud: their balls are empty
    feat = torch.randn(2, 35, n, generator=gen)
    return xyz.to(cuda), new_xyz.contiguous().to(cuda), feat.to(cuda)


def run_grouper(grouper, xyz, new_xyz, feat, subset, seed):
    xyz, new_xyz, feat = (t.detach().clone().requires_grad_() for t in (xyz, new_xyz, feat))
    out, count = grouper(xyz, new_xyz, feat, subset=subset, return_counts=True, record_neighbor_stats=True)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)
    wrt = (feat, xyz, new_xyz)
    grads = torch.autograd.grad(out, wrt, go, allow_unused=True)             # without use_xyz the composition has no path
    grads = [torch.zeros_like(w) if g is None else g for g, w in zip(grads, wrt)]
    return out.detach(), count, go, dict(zip(QC.OUTPUTS, (g.cpu().numpy() for g in grads))), grouper.neighbor_stats.clone()


def judge_grouper(grouper, clouds, subset, patch, flags, seed):
    xyz, new_xyz, feat = clouds
    off, on = both(lambda: run_grouper(grouper, xyz, new_xyz, feat, subset, seed))
    assert np.array_equal(bits(on[0]), bits(off[0]))
    assert (on[1] == off[1]) if isinstance(on[1], str) else torch.equal(on[1], off[1])
    assert torch.equal(on[4], off[4])
    idx, counts = grouper._neighbours(xyz, new_xyz)
    A = QC.Arrays(xyz.cpu().numpy(), new_xyz.cpu().numpy(), feat.cpu().numpy(), idx.cpu().numpy(),
                  counts.cpu().numpy() if patch else None, on[2].cpu().numpy())
    assert np.array_equal(bits(on[0]), bits(QC.forward_reference(A, flags)))
    ref = QC.reference64(A, flags)
    emu = dict(zip(QC.OUTPUTS, QC.emulate_backward(A, flags)))
    worst_on, worst_off = QC.worst_ratio(on[3], ref), QC.worst_ratio(off[3], ref)
    print("switch on", worst_on, "switch off", worst_off)
    assert max(worst_on.values()) <= 1.0 and max(worst_off.values()) <= 1.0
    for k in QC.OUTPUTS:
        assert np.array_equal(bits(on[3][k]), bits(emu[k])), k
        assert (np.abs(on[3][k].astype(np.float64) - off[3][k]) <= 2 * ref["b_" + k]).all(), k
    return counts


@pytest.mark.parametrize("subset", [True, False])
def test_query_and_group_radius_mode_switch_on_against_switch_off(cuda, subset):
    clouds = module_clouds(cuda)
    grouper = pointnet2_utils.QueryAndGroup(0.2, 32, True, True, True)
    counts = judge_grouper(grouper, clouds, subset, patch=not subset, flags=7, seed=32)
    assert int((counts == 0).sum()) >= 8 and int((counts > 0).sum()) > 100
    plain = pointnet2_utils.QueryAndGroup(0.2, 32, use_xyz=False)
    judge_grouper(plain, clouds, subset, patch=not subset, flags=0, seed=33)


@pytest.mark.parametrize("n_cloud", [300, 20])
def test_query_and_group_nn_mode_switch_on_against_switch_off(cuda, n_cloud):
    """n_cloud = 20: nsample = 32 > n, the group holds K = 20 neighbours."""
    xyz, new_xyz, feat = module_clouds(cuda)
    clouds = (xyz[:, :n_cloud].contiguous(), new_xyz, feat[:, :, :n_cloud].contiguous())
    grouper = pointnet2_utils.QueryAndGroup(None, 32, True, True, False, neighbor_def='nn')
    off, on = both(lambda: run_grouper(grouper, *clouds, False, 34))
    assert on[0].shape == (2, 35 + 6, 70, min(32, n_cloud)) and on[1] == off[1] == 'all'
    judge_grouper(grouper, clouds, False, patch=False, flags=3, seed=34)


def test_the_switch_picks_the_op_and_leaves_other_tensors_to_the_composition(cuda, monkeypatch):
    xyz, new_xyz, feat = module_clouds(cuda)
    grouper = pointnet2_utils.QueryAndGroup(0.2, 32, True, True, True)
    names = lambda: type(grouper(xyz, new_xyz, feat.clone().requires_grad_(), subset=False).grad_fn).__name__
    off, on = both(names)
    assert "QueryGroup" in on and "QueryGroup" not in off
    prev = _ext.set_fused_grouping(True)
    try:
        with monkeypatch.context() as mp:                    # double tensors (the float64 evaluation below): not the op's
            double_ops(mp)
            out = grouper(xyz.double(), new_xyz.double(), feat.double().requires_grad_(), subset=False)
        assert out.dtype == torch.float64 and "QueryGroup" not in type(out.grad_fn).__name__
    finally:
        _ext.set_fused_grouping(prev)


# ---- two tiny modules against their float64 evaluation ----------------------------------------------------------------
ATTENTION = dict(use_attention_module=True, attention_bn=True, transform_grouped_feat_out=True, last_activation=True)


def evaluate(mod, inputs_, r, pick):
    """[out] + gradients of sum(out * r) w.r.t. every parameter and every floating input, as float64 CPU tensors."""
    inputs_ = [t.detach().clone().requires_grad_() for t in inputs_]
    out = pick(mod(*inputs_))
    wrt = list(mod.parameters()) + inputs_
    grads = torch.autograd.grad((out * r.to(out.dtype)).sum(), wrt, allow_unused=True)
    return [out.detach().double().cpu()] + [torch.zeros_like(w).double().cpu() if g is None else g.double().cpu()
                                           for g, w in zip(grads, wrt)]


def double_ops(mp):
    """Patch the module path for a float64 evaluation WITH gradients: FPS and the ball query decide on the fp32 cast of
    their coordinates (the decisions of the fp32 run), gather and group are torch indexing in the input's dtype."""
    fps, ball = pointnet2_utils.furthest_point_sample, pointnet2_utils.ball_query
    f32 = lambda t: t.detach().float().contiguous()

    def gather(points, idx):                                 # (B, C, N), (B, m) -> (B, C, m)
        return points.gather(2, idx.long().unsqueeze(1).expand(-1, points.shape[1], -1))

    def group(points, idx):                                  # (B, C, N), (B, np, ns) -> (B, C, np, ns)
        return gather(points, idx.reshape(idx.shape[0], -1)).reshape(*points.shape[:2], *idx.shape[1:])
    mp.setattr(pointnet2_utils, "furthest_point_sample", lambda xyz, n: fps(f32(xyz), n))
    mp.setattr(pointnet2_utils, "ball_query", lambda r, ns, xyz, new_xyz: ball(r, ns, f32(xyz), f32(new_xyz)))
    mp.setattr(pointnet2_utils, "gather_operation", gather)
    mp.setattr(pointnet2_utils, "grouping_operation", group)


def against_float64(label, mod, inputs_, pick, cuda, monkeypatch):
    mod = mod.to(cuda)
    inputs_ = [t.to(cuda) for t in inputs_]
    with torch.no_grad():
        shape = pick(mod(*inputs_)).shape
    r = torch.randn(shape, generator=torch.Generator().manual_seed(41)).to(cuda)
    with monkeypatch.context() as mp:
        double_ops(mp)
        want = evaluate(copy.deepcopy(mod).double(), [t.double() for t in inputs_], r.double(), pick)
    saved = _ext.set_fused_attention_pool(True), _ext.set_fused_group_norm(True)
    try:
        off, on = both(lambda: evaluate(mod, inputs_, r, pick))
    finally:
        _ext.set_fused_attention_pool(saved[0])
        _ext.set_fused_group_norm(saved[1])
    names = ["out"] + [n for n, _ in mod.named_parameters()] + ["input%d" % i for i in range(len(inputs_))]
    top = max(float(w.abs().max()) for w in want[1:])
    failed, worst = [], (0.0, 0.0)
    for i, (name, w, a, b) in enumerate(zip(names, want, off, on)):
        scale = float(w.abs().max())
        if i > 0 and scale < 1e-3 * top:                     # zero in exact arithmetic: judge against the largest gradient
            scale = top
        e_off, e_on = float((a - w).abs().max()) / scale, float((b - w).abs().max()) / scale
        print("%s %-40s scale %.3g  switch off %.3g  switch on %.3g" % (label, name, scale, e_off, e_on))
        worst = (max(worst[0], e_off), max(worst[1], e_on))
        if not e_on <= 2.0 * e_off:
            failed.append((name, e_off, e_on))
    print("%s worst: switch off %.3g  switch on %.3g" % (label, *worst))
    assert torch.equal(off[0], on[0])                        # the op changes no forward bit
    assert not failed, (label, failed)


def test_feature_map_module_all_three_switches_on_against_float64(cuda, monkeypatch):
    torch.manual_seed(42)
    mod = FeatureMapModule([8, 32, 32], 0.3, 8, activation='swish', attention_setting=ATTENTION, query_feature_dim=16)
    gen = torch.Generator().manual_seed(43)
    xyz = torch.rand(2, 40, 3, generator=gen)
    new_xyz = (xyz[:, :24] + 0.05 * torch.randn(2, 24, 3, generator=gen)).contiguous()
    new_xyz[:, ::7] += 50.0                                  # empty balls: subset=False patches them
    feat, query = torch.randn(2, 8, 40, generator=gen), torch.randn(2, 16, 24, generator=gen)

    class Wrapped(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, xyz_, feat_, new_, q_):
            return self.inner(xyz_, feat_, new_, features_at_new_xyz=q_)
    against_float64("feature-map", Wrapped(mod), [xyz, feat, new_xyz, query], lambda o: o, cuda, monkeypatch)


def test_pointnet_sa_module_all_three_switches_on_against_float64(cuda, monkeypatch):
    torch.manual_seed(44)
    mod = PointnetSAModule([8, 32, 32], npoint=16, radius=0.4, nsample=8, include_abs_coordinate=True,
                           include_center_coordinate=True, activation='swish', attention_setting=ATTENTION)
    gen = torch.Generator().manual_seed(45)
    xyz, feat = torch.rand(2, 40, 3, generator=gen), torch.randn(2, 8, 40, generator=gen)
    against_float64("sa-module", mod, [xyz, feat], lambda o: o[1], cuda, monkeypatch)
