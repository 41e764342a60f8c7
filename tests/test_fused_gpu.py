"""The fused channel-last execution (libpdr_hip.so fused_layer / group_build / attention_pool ...)
must reproduce the layer-by-layer PyTorch execution of the same network -- which itself is pinned
to the reference's Python by tests/test_reference_golden.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests.chain_cases import chain_case as _chain_case, launch_chain as _launch_chain
from tests.golden.det_weights import fill_deterministic
from tests.golden.tiny_config import small_fused_config

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2 import fused_network as FN
from point_diffusion_refinement_amd.pointnet2 import util
from point_diffusion_refinement_amd.pointnet2.configs import ddpm_pointnet_config, synthetic_batch
from point_diffusion_refinement_amd.pointnet2.models.pointnet2_with_pcld_condition import PointNet2CloudCondition
from point_diffusion_refinement_amd.pointnet2.reverse_sampler import GraphedReverseSampler

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(((a - b).abs() / (b.abs() + 1.0)).max())


def _conv(W, bias):
    m = torch.nn.Conv2d(W.shape[1], W.shape[0], 1).to(W.device)
    m.weight.data = W.reshape(W.shape[0], W.shape[1], 1, 1).clone()
    m.bias.data = bias.clone()
    return FN.Conv([m])


@pytest.mark.parametrize("P,Cin,Cout,rpb", [(256, 13, 96, 128), (512, 79, 35, 64), (1024, 331, 331, 256),
                                            (96, 3, 32, 32), (4096, 64, 32, 4096), (2048, 163, 3, 1024),
                                            (64, 35, 44, 16), (600, 20, 70, 200),
                                            # many row tiles per (persistent) workgroup
                                            (1 << 18, 41, 32, 8192), (1 << 18, 64, 64, 1 << 16),
                                            (1 << 17, 128, 128, 4096)])
def test_fused_layer_matches_torch(cuda, P, Cin, Cout, rpb):
    g = torch.Generator().manual_seed(P + Cin)
    B = P // rpb
    c1 = Cin // 2 if Cin > 4 else Cin
    K = 4
    q = torch.randn(P // K, c1, generator=g).to(cuda)                     # broadcast segment (row_div = K)
    k = torch.randn(P, Cin - c1 + 5, generator=g).to(cuda)               # strided segment (ld > C), unaligned
    scale, shift, add = (torch.randn(B, Cin, generator=g).to(cuda) for _ in range(3))
    radd = torch.randn(P, Cin + 2, generator=g).to(cuda)
    W = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(cuda)
    bias = torch.randn(Cout, generator=g).to(cuda)
    segs = [(q, 0, c1, c1, K)] + ([(k, 3, Cin - c1, Cin - c1 + 5, 1)] if Cin > c1 else [])
    for pre, post in ((False, True), (True, False)):
        act = FN.Act(segs, P, B, rpb, scale=scale, shift=shift, add=add, add_ld=Cin, radd=(radd, 1, Cin, Cin + 2, 1),
                     pre_relu=pre, post_relu=post)
        conv = _conv(W, bias)
        Y, part, tpb = FN.run_layer(act, conv, stats=True, relu_col0=Cout // 2)
        x = torch.cat([q.repeat_interleave(K, 0)] + ([k[:, 3:3 + Cin - c1]] if Cin > c1 else []), 1)
        bidx = torch.arange(P, device=cuda) // rpb
        if pre:
            x = x.relu()
        x = x * scale[bidx] + shift[bidx]
        if post:
            x = x.relu()
        x = x + add[bidx] + radd[:, 1:1 + Cin]
        ref = (x.double() @ W.t().double() + bias.double())
        assert _rel(Y[:, :Cout].double(), ref) < 2e-5
        np.testing.assert_allclose(FN.materialize(act).cpu().numpy(), x.cpu().numpy(), rtol=1e-6, atol=1e-6)
        f = ref.clone()
        f[:, Cout // 2:] = f[:, Cout // 2:].relu()
        s1 = f.view(B, rpb, Cout).sum(1)
        s2 = (f * f).view(B, rpb, Cout).sum(1)
        got = part.view(B, tpb, Cout, 2).double().sum(1)
        assert _rel(got[..., 0], s1) < 1e-4 and _rel(got[..., 1], s2) < 1e-4


@pytest.mark.parametrize("B,K,N,act", [(32, 128, 512, 1), (5, 512, 4104, 0), (40, 32, 128, 1), (1, 64, 33, 0)])
def test_embed_linear_matches_torch(cuda, B, K, N, act):
    """pdr_embed_linear (csrc/embed.hip): Linear (+ swish) over B rows, plain input and the sinusoidal-step prologue,
    against float64 torch; reference: pointnet2_ssg_sem.py:14-31, pointnet2_with_pcld_condition.py:183-184."""
    from point_diffusion_refinement_amd.pointnet2.models.pointnet2_ssg_sem import _frequencies, calc_t_emb, swish
    lib = _lib.load()
    g = torch.Generator().manual_seed(B + K + N)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    bias = torch.randn(N, generator=g).to(cuda)
    x = torch.randn(B, K, generator=g).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty((B, N), device=cuda)
    _lib.check(lib.pdr_embed_linear(x.data_ptr(), K, None, 0, None, 0, W.data_ptr(), bias.data_ptr(), B, K, N, act,
                                    out.data_ptr(), N, st), "embed_linear")
    want = torch.nn.functional.linear(x.double(), W.double(), bias.double())
    want = swish(want) if act else want
    np.testing.assert_allclose(out.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-6)
    # sinusoidal prologue: step values as large as T - 1 = 999 and fractional FastDPM times; a (1,) tensor expanded
    # to the batch (stride 0) as the samplers pass it
    half = K // 2
    freq = _frequencies(half, cuda)
    for ts in (torch.linspace(0.0, 999.0, B).to(cuda), torch.tensor([417.25], device=cuda).expand(B)):
        _lib.check(lib.pdr_embed_linear(None, 0, ts.data_ptr(), ts.stride(0), freq.data_ptr(), half, W.data_ptr(),
                                        bias.data_ptr(), B, K, N, act, out.data_ptr(), N, st), "embed_linear")
        emb = calc_t_emb(ts.contiguous(), K)                           # f32 sin / cos of the f32 product, as the reference
        want = torch.nn.functional.linear(emb.double(), W.double(), bias.double())
        want = swish(want) if act else want
        np.testing.assert_allclose(out.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=5e-6)
    assert lib.pdr_embed_linear(x.data_ptr(), K, None, 0, None, 0, W.data_ptr(), bias.data_ptr(), B, K - 4, N, 0,
                                out.data_ptr(), N, st) in (_lib.PDR_EUNSUPPORTED, _lib.PDR_EINVAL)


def test_native_step_embedding_chain_equals_the_torch_chain(cuda, monkeypatch):
    """FusedCloudConditionNet._embeddings: three pdr_embed_linear launches == calc_t_emb / fc_t1 / fc_t2 / bank GEMM."""
    net, fused = _pair(small_fused_config(), 21, cuda)
    ts = torch.tensor([13.0, 977.0], device=cuda)
    label = torch.tensor([1, 7], device=cuda)
    net.global_feature = torch.zeros((2, 128), device=cuda)
    with torch.no_grad():
        monkeypatch.setattr(FN, "NATIVE_EMBED", False)
        fused._embeddings(ts, label)
        want = fused.bank.out["t"].clone()
        monkeypatch.setattr(FN, "NATIVE_EMBED", True)
        fused._embeddings(ts, label)
        got = fused.bank.out["t"]
    assert got.data_ptr() != want.data_ptr()
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-6)
    net.global_feature = None


def test_groupnorm_fold_matches_torch_groupnorm(cuda):
    g = torch.Generator().manual_seed(3)
    B, rpb, C = 3, 256, 79                                               # MyGroupNorm(32, 79): 64 normalised + 15 pass-through
    x = (torch.randn(B * rpb, C, generator=g) * 2 + 0.7).to(cuda)
    from point_diffusion_refinement_amd.pointnet2_ops.attention import MyGroupNorm
    gn = fill_deterministic(MyGroupNorm(32, C), 9).to(cuda)
    ident = _conv(torch.eye(C, device=cuda), torch.zeros(C, device=cuda))
    Y, part, tpb = FN.run_layer(FN.plain(x, B, rpb), ident, stats=True)
    scale, shift = FN.Norm(gn).fold([(part, 0, C, tpb, 1.0)], B, C, rpb)
    got = FN.materialize(FN.Act([(Y, 0, C, Y.shape[1], 1)], B * rpb, B, rpb, scale=scale, shift=shift))
    want = gn(x.view(B, rpb, C).permute(0, 2, 1).unsqueeze(-1)).squeeze(-1).permute(0, 2, 1).reshape(B * rpb, C)
    np.testing.assert_allclose(got.cpu().numpy(), want.detach().cpu().numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("remove_last", [False, True])
def test_fused_global_pointnet_matches_the_torch_module(cuda, remove_last):
    """VERDICT r3 missing 5: the global PointNet of a new batch (models/pnet.py; reference pnet.py:27-40) on the fused
    layer kernels + pdr_act_colmax instead of torch Conv2d -> MIOpen, incl. the variant without the stages' last
    GroupNorm / ReLU; and the condition / class embedding GEMMs of EmbeddingBank on pdr_embed_linear."""
    from point_diffusion_refinement_amd.pointnet2.models.pnet import Pnet2Stage
    torch.manual_seed(4)
    pnet = fill_deterministic(Pnet2Stage([4, 128, 256], [512, 1024], bn=True, remove_last_activation=remove_last),
                              17).eval().to(cuda)
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(3, 3072, 4, generator=g) * 2 - 1).to(cuda)
    with torch.no_grad():
        want = pnet(x.transpose(1, 2))
        got = FN.FusedPnet2Stage(pnet)(x.contiguous())
    assert got.shape == want.shape == (3, 1024)
    from tests import parity
    parity.check("fused_global_pointnet:%s" % ("conv_last" if remove_last else "gn_relu_last"), "hip", got, want, 1e-4)
    # pdr_act_colmax alone: max over rows of relu(x s + t) + a
    y = torch.randn(2 * 500, 70, generator=g).to(cuda)
    sc, sh, ad = (torch.randn(2, 70, generator=g).to(cuda) for _ in range(3))
    act = FN.Act([(y, 0, 70, 70, 1)], 1000, 2, 500, scale=sc, shift=sh, add=ad, add_ld=70, post_relu=True)
    ref = ((y.view(2, 500, 70) * sc[:, None] + sh[:, None]).relu() + ad[:, None]).amax(1)
    assert torch.equal(FN.act_colmax(act), ref) or float((FN.act_colmax(act) - ref).abs().max()) < 1e-6
    # embedding rows of a new batch through pdr_embed_linear == F.linear
    bank = FN.EmbeddingBank()
    lin = [torch.nn.Linear(1024, 96).to(cuda), torch.nn.Linear(1024, 40).to(cuda)]
    for m in lin:
        bank.register("c", m)
    bank.pack()
    src = torch.randn(5, 1024, generator=g).to(cuda)
    with torch.no_grad():
        bank.evaluate_kind("c", src, static=True)
        first = bank.out["c"]
        ref = torch.cat([m(src) for m in lin], 1)
        np.testing.assert_allclose(first.cpu().numpy(), ref.cpu().numpy(), rtol=2e-5, atol=2e-5)
        bank.evaluate_kind("c", src * 0.5, static=True)                   # in place: same buffer, new contents
        assert bank.out["c"].data_ptr() == first.data_ptr()
        np.testing.assert_allclose(bank.out["c"].cpu().numpy(), torch.cat([m(src * 0.5) for m in lin], 1).cpu().numpy(),
                                   rtol=2e-5, atol=2e-5)


def _pair(cfg, seed, device):
    net = fill_deterministic(PointNet2CloudCondition(cfg), seed).eval().to(device)
    return net, FN.FusedCloudConditionNet(net)


def _cached_eps(net, fused, x, cond, ts, label):
    with torch.no_grad():
        net.reset_cond_features()
        net(x, cond, ts=ts, label=label, use_retained_condition_feature=True)       # fills the cache
        x2 = x * 0.9
        ref = net(x2, cond, ts=ts - 1, label=label, use_retained_condition_feature=True)
        fused.sync_condition()
        got = fused(x2, cond, ts=ts - 1, label=label, use_retained_condition_feature=True)
    return got, ref


@pytest.mark.parametrize("split_first", ["virtual", "materialised", False])
def test_fused_network_small_config(cuda, split_first, monkeypatch):
    """split_first=True: first conv of each grouped block via per-point U/V tables + gather_add;
    False: GEMM over the materialised grouped tensor (group_build / knn_build).  Both must match torch."""
    monkeypatch.setattr(FN, "USE_SPLIT_FIRST", bool(split_first))
    monkeypatch.setattr(FN, "USE_VIRTUAL_FIRST", split_first == "virtual")
    net, fused = _pair(small_fused_config(), 21, cuda)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 256, 3, generator=g).to(cuda)
    cond = torch.cat([torch.rand(2, 384, 3, generator=g) * 2 - 1, torch.ones(2, 384, 1)], 2).to(cuda)
    ts, label = torch.tensor([9.0, 4.0], device=cuda), torch.tensor([1, 7], device=cuda)
    got, ref = _cached_eps(net, fused, x, cond, ts, label)
    err = ((got - ref).abs() / (ref.abs() + 1.0))
    assert err.max() < 1e-2 and (err < 1e-3).float().mean() > 0.99, (err.max(), (err < 1e-3).float().mean())


def test_optional_fusions_match(cuda, monkeypatch):
    """The optional paths (virtual first conv of the ball and of the kNN blocks, score+pool epilogue) stay
    numerically equivalent, on and off."""
    net, fused = _pair(small_fused_config(), 22, cuda)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 256, 3, generator=g).to(cuda)
    cond = torch.cat([torch.rand(2, 384, 3, generator=g) * 2 - 1, torch.ones(2, 384, 1)], 2).to(cuda)
    ts, label = torch.tensor([9.0, 4.0], device=cuda), torch.tensor([1, 7], device=cuda)
    base, _ = _cached_eps(net, fused, x, cond, ts, label)
    for flag, values in (("FUSE_SCORE_POOL", (True, False)), ("USE_VIRTUAL_FIRST", (True, False)),
                         ("USE_VIRTUAL_KNN", (True, False)), ("GATHER_RES", (0, 32, 4096)),
                         ("GATHER_RES_KNN", (True, False))):
        default = getattr(FN, flag)
        for value in values:
            monkeypatch.setattr(FN, flag, value)
            got, _ = _cached_eps(net, fused, x, cond, ts, label)
            assert ((got - base).abs() / (base.abs() + 1.0)).max() < 1e-3, (flag, value)
        monkeypatch.setattr(FN, flag, default)


def test_fused_network_ddpm_config_and_graphed_sampler(cuda):
    torch.manual_seed(0)
    net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)            # default (random) init
    fused = FN.FusedCloudConditionNet(net)
    x, cond, label = synthetic_batch(2, seed=3, device=cuda)
    ts = torch.tensor([500.0, 20.0], device=cuda)
    got, ref = _cached_eps(net, fused, x, cond, ts, label)
    err = ((got - ref).abs() / (ref.abs() + 1.0))
    assert err.max() < 1e-2 and (err < 1e-3).float().mean() > 0.99, (err.max(), (err < 1e-3).float().mean())

    # reverse sampler: fused + hipGraph replay vs the reference-style eager loop, same CPU noise stream
    dh = util.calc_diffusion_hyperparams(6, 1e-4, 0.02)
    util.set_device(cuda)
    util.set_noise_source('cpu')
    torch.manual_seed(77)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        want = util.sampling(net, (2, 2048, 3), dh, label=label, verbose=False, condition=cond)
    util.set_device(None)
    outs = {}
    for use_graph in (False, True):
        sampler = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=use_graph)
        torch.manual_seed(77)
        outs[use_graph] = sampler.sample((2, 2048, 3), cond, label)
    # graph replay == eager launch of the same kernels
    assert ((outs[True] - outs[False]).abs() / (outs[False].abs() + 1.0)).max() < 1e-5
    # vs the layer-by-layer loop: ~1e-6 per step, except that a near-tie in a discrete decision (FPS pick, ball
    # membership, ReLU / mask boundary) may flip in ONE cloud and move its trajectory by ~1e-2:
    # every cloud agrees in the bulk, at most one of the two carries such a flip
    per_cloud = ((outs[True] - want).abs() / (want.abs() + 1.0)).flatten(1)
    assert (per_cloud.median(1).values < 1e-4).all(), per_cloud.median(1).values
    assert int((per_cloud.max(1).values < 1e-3).sum()) >= 1 and float(per_cloud.max()) < 0.5, per_cloud.max(1).values
    # a second batch through the SAME captured graph (retained features are re-pointed in place)
    x2, cond2, label2 = synthetic_batch(2, seed=4, device=cuda)
    torch.manual_seed(78)
    a = sampler.sample((2, 2048, 3), cond2, label2)
    torch.manual_seed(78)
    b = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=False).sample((2, 2048, 3), cond2, label2)
    assert ((a - b).abs() / (b.abs() + 1.0)).max() < 1e-5         # same kernels, same inputs


def test_xcd_local_tile_order_is_bit_identical(cuda, tmp_path):
    """Option ws_xcd_order (set through the child's binding -> two subprocesses): the XCD-local cloud-major tile order of the layer
    kernels changes WHICH workgroup computes a tile, never the tile: one uncached + three cached reverse steps of the
    DDPM config at B = 8 give identical bytes under the plain order and under the XCD-local order for every layer."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for order in ("0", "2"):
        path = str(tmp_path / ("x%s.pt" % order))
        env = dict(os.environ, PDR_OPTIONS="ws_xcd_order=" + order, ORDER_CHECK_B="8")
        subprocess.check_call([sys.executable, "-m", "tools.lab.order_check", path], cwd=root, env=env,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        outs.append(torch.load(path))
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


# (name, environment, must be bit-identical to the default run)
_VARIANTS = [
    # kernel-selection options of libpdr_hip.so (pdr_set_option, include/pdr_hip.h; the child's binding applies
    # PDR_OPTIONS at load -- the library itself never reads the environment)
    ("ws_off", {"PDR_OPTIONS": "fused_ws=0"}, False), ("narrow_kc16", {"PDR_OPTIONS": "narrow_kc32=0"}, False),
    ("fps_wave0", {"PDR_OPTIONS": "fps_wave=0"}, True), ("fps_wave2", {"PDR_OPTIONS": "fps_wave=2"}, True),
    ("fps_resident", {"PDR_OPTIONS": "fps_lean=0"}, True),
    ("knn_thread", {"PDR_OPTIONS": "knn_wave=0"}, True), ("narrow_2wg", {"PDR_OPTIONS": "ws_narrow3=0"}, True),
    ("fold_1024_threads", {"PDR_OPTIONS": "gn_fold_small=0"}, False),
    ("xcd_plain", {"PDR_OPTIONS": "ws_xcd_order=0"}, True), ("xcd_all", {"PDR_OPTIONS": "ws_xcd_order=2"}, True),
    ("tiny_layers_on_ordinary_tiles", {"PDR_OPTIONS": "deep_chunks=0"}, False),
    ("tiny_layers_without_k_split", {"PDR_OPTIONS": "deep_ks=0"}, False),
    # evaluation variants of fused_network.py (module constants; PDR_FUSED_OPTS is the lab override)
    ("no_score_pool", {"PDR_FUSED_OPTS": "FUSE_SCORE_POOL=0"}, False),
    ("materialised_first", {"PDR_FUSED_OPTS": "USE_VIRTUAL_FIRST=0"}, False),
    ("materialised_knn", {"PDR_FUSED_OPTS": "USE_VIRTUAL_KNN=0"}, False),
    ("residual_written", {"PDR_FUSED_OPTS": "GATHER_RES=0"}, False),
    ("residual_32", {"PDR_FUSED_OPTS": "GATHER_RES=32"}, False),
    ("residual_knn_written", {"PDR_FUSED_OPTS": "GATHER_RES_KNN=0"}, False),
    ("tables_in_blocks", {"PDR_FUSED_OPTS": "SIDE_TABLES=0"}, True),
    ("sampling_on_the_geometry_stream", {"PDR_FUSED_OPTS": "FPS_STREAM=0"}, True),
    ("torch_embedding_chain", {"PDR_FUSED_OPTS": "NATIVE_EMBED=0"}, False),
    ("query_conv_unsplit", {"PDR_FUSED_OPTS": "SPLIT_QUERY_CONV=0"}, False),
    ("grouped_first_conv", {"PDR_FUSED_OPTS": "USE_SPLIT_FIRST=0"}, False),
    ("layerwise_condition_branch", {"PDR_FUSED_OPTS": "FUSE_CONDITION_BRANCH=0"}, False),
    ("torch_global_pointnet", {"PDR_FUSED_OPTS": "FUSE_GLOBAL_PNET=0"}, False),
    ("whole_neighbourhoods", {"PDR_FUSED_OPTS": "DEDUP=0"}, False),
    # the round-4 forms of the launches round 5 fused (cross-checks of the default)
    ("plan_in_six_launches", {"PDR_FUSED_OPTS": "FUSED_PLAN=0"}, True),
    ("weighted_moments_launches", {"PDR_FUSED_OPTS": "TWIN_STATS=0"}, False),
    ("patch_rows_launch", {"PDR_FUSED_OPTS": "FUSED_PATCH=0"}, True),
    ("dedup_from_256_queries", {"PDR_FUSED_OPTS": "DEDUP_MIN_QUERIES=256"}, False),
    ("decoder_maps_in_place", {"PDR_FUSED_OPTS": "AHEAD_DECODER_MAPS=0"}, False),
    ("level0_decoder_map_on_the_geometry_stream", {"PDR_FUSED_OPTS": "HOIST_LEVEL0_ON_MAIN=0"}, False),
    # round 6: the paired launches as two launches each (same tiles, same arithmetic), the point chains layer by layer
    ("one_launch_per_row_set", {"PDR_FUSED_OPTS": "PAIRED_LAUNCHES=0"}, True),    # (same tiles, same kernels' arithmetic)
    ("point_chains_layer_by_layer", {"PDR_FUSED_OPTS": "POINT_CHAINS=0"}, False),
    ("encoder_maps_in_place", {"PDR_FUSED_OPTS": "AHEAD_ENCODER_MAPS=0"}, False),
    ("first_sa_table_in_the_block", {"PDR_FUSED_OPTS": "SA0_TABLE_AHEAD=0"}, True),
    ("source_tables_in_two_launches", {"PDR_FUSED_OPTS": "SPLIT_SOURCE_TABLES=1"}, False),
    ("query_features_gathered_into_sorted_order", {"PDR_FUSED_OPTS": "QUERIES_IN_PLACE=0"}, False),
    ("query_conv_in_its_place", {"PDR_FUSED_OPTS": "QUERY_CONV_AHEAD=0"}, True),
    # every launch walking its tiles against its producer's direction (pdr_layer_in_t.walk_reverse): order in time only
    ("tiles_walked_against_the_producer", {"PDR_FUSED_OPTS": "ZIGZAG_WALK=1"}, True),
]


def test_ddpm_forward_with_every_non_default_variant(cuda, tmp_path):
    """every surviving kernel-selection knob and evaluation variant, at its non-default values, on
    the FULL DDPM architecture (one first + one cached forward, B = 2, fixed inputs => identical geometry): scheduling
    variants give identical bytes, arithmetic variants stay within north_star's 1e-4 of the default evaluation."""
    import os
    import subprocess
    import sys
    from tests import parity
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jobs = [("default", {}, True)] + _VARIANTS
    procs = []
    results = {}

    def reap(limit):
        while len(procs) > limit:
            name, p, path = procs.pop(0)
            _, err = p.communicate()
            assert p.returncode == 0, (name, err.decode()[-2000:])
            results[name] = torch.load(path)
    for name, env, _ in jobs:
        path = str(tmp_path / (name + ".pt"))
        e = dict(os.environ, **env)
        procs.append((name, subprocess.Popen([sys.executable, "-m", "tools.variant_check", path], cwd=root, env=e,
                                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE), path))
        reap(7)                                            # at most 8 children at a time
    reap(0)
    base = results["default"]
    assert all(bool(torch.isfinite(v).all()) for v in base.values())
    for name, _, identical in _VARIANTS:
        for call in ("first", "cached", "mixed"):
            got, want = results[name][call], base[call]
            if identical:
                assert torch.equal(got, want), (name, call, float((got - want).abs().max()))
            else:
                parity.check("variant:%s:%s" % (name, call), "hip", got, want, 1e-4)


def test_graphed_sampler_options_t_slices_and_precomputed_xt(cuda):
    """GraphedReverseSampler.sample(return_multiple_t_slices=, use_a_precomputed_XT=) (util.py:217-222, 246-248): the
    slice steps run eagerly through PyTorch ops, every other step as a graph replay; against the layer-by-layer
    reference-style loop `util.sampling` on the same CPU noise stream."""
    import contextlib, io
    net, fused = _pair(small_fused_config(), 29, cuda)
    dh = util.calc_diffusion_hyperparams(9, 1e-4, 0.02)
    g = torch.Generator().manual_seed(12)
    cond = torch.cat([torch.rand(2, 256, 3, generator=g) * 2 - 1, torch.ones(2, 256, 1)], 2).to(cuda)
    label = torch.tensor([4, 9], device=cuda)
    XT = torch.randn(2, 128, 3, generator=g).to(cuda)
    kw = dict(return_multiple_t_slices=True, t_slices=[5, 1], use_a_precomputed_XT=True, step=7, XT=XT)
    util.set_device(cuda)
    util.set_noise_source('cpu')
    try:
        torch.manual_seed(41)
        with contextlib.redirect_stdout(io.StringIO()):
            want, want_slices = util.sampling(net, (2, 128, 3), dh, label=label, verbose=False, condition=cond, **kw)
    finally:
        util.set_device(None)
    for use_graph in (True, False):
        torch.manual_seed(41)
        got, slices = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=use_graph).sample((2, 128, 3), cond, label, **kw)
        assert sorted(slices) == [1, 5] == sorted(want_slices)
        for a, b in [(got, want)] + [(slices[t], want_slices[t]) for t in (1, 5)]:
            assert ((a - b).abs() / (b.abs() + 1.0)).max() < 2e-4, use_graph


@pytest.mark.parametrize("fuse_branch", [False, True])
def test_second_batch_with_other_labels_through_the_captured_graph(cuda, fuse_branch, monkeypatch):
    """The class-embedding rows of the blocks live in a static buffer that a captured step only READS: a second batch
    with DIFFERENT labels must refresh them before its replays -- also when the first step of a batch takes the
    layer-by-layer path (FUSE_CONDITION_BRANCH = False) and never reaches the embedding bank."""
    monkeypatch.setattr(FN, "FUSE_CONDITION_BRANCH", fuse_branch)
    net, fused = _pair(small_fused_config(), 23, cuda)
    dh = util.calc_diffusion_hyperparams(5, 1e-4, 0.02)
    g = torch.Generator().manual_seed(11)
    cond = torch.cat([torch.rand(2, 256, 3, generator=g) * 2 - 1, torch.ones(2, 256, 1)], 2).to(cuda)
    graphed = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=True)
    outs = []
    for labels in ([1, 5], [9, 2]):
        label = torch.tensor(labels, device=cuda)
        torch.manual_seed(31)
        a = graphed.sample((2, 128, 3), cond, label)
        torch.manual_seed(31)
        b = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=False).sample((2, 128, 3), cond, label)
        assert ((a - b).abs() / (b.abs() + 1.0)).max() < 1e-5, labels          # same kernels, same inputs
        outs.append(a)
    assert (outs[0] - outs[1]).abs().max() > 1e-4                              # the label does matter


@pytest.mark.parametrize("P,Cin,Cout,rpb", [(512, 13, 96, 256), (1024, 331, 587, 512), (256, 64, 32, 256),
                                            (2048, 171, 140, 1024), (128, 41, 105, 128)])
def test_fused_layer_vector_staging(cuda, P, Cin, Cout, rpb):
    """16-B aligned, 4-float-padded sources take the float4 staging path; same answer as torch."""
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    B = P // rpb
    ld = (Cin + 3) // 4 * 4
    x = torch.zeros(P, ld, device=cuda)
    x[:, :Cin] = torch.randn(P, Cin, generator=g).to(cuda)
    x[:, Cin:] = float("nan")                                              # padding must never leak in
    scale, shift, add = (torch.randn(B, Cin, generator=g).to(cuda) for _ in range(3))
    radd = torch.zeros(P, ld, device=cuda)
    radd[:, :Cin] = torch.randn(P, Cin, generator=g).to(cuda)
    W = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(cuda)
    bias = torch.randn(Cout, generator=g).to(cuda)
    conv = _conv(W, bias)
    bidx = torch.arange(P, device=cuda) // rpb
    for use_radd in (False, True):
        act = FN.Act([(x, 0, Cin, ld, 1)], P, B, rpb, scale=scale, shift=shift, add=add, add_ld=Cin,
                     radd=(radd, 0, Cin, ld, 1) if use_radd else None, post_relu=True)
        Y, part, tpb = FN.run_layer(act, conv, stats=True)
        ref = (x[:, :Cin] * scale[bidx] + shift[bidx]).relu() + add[bidx]
        if use_radd:
            ref = ref + radd[:, :Cin]
        ref = ref.double() @ W.t().double() + bias.double()
        assert torch.isfinite(Y[:, :Cout]).all()
        assert _rel(Y[:, :Cout].double(), ref) < 2e-5
        got = part.view(B, tpb, Cout, 2).double().sum(1)
        assert _rel(got[..., 0], ref.view(B, rpb, Cout).sum(1)) < 1e-4


@pytest.mark.parametrize("method,schedule,kappa", [("var", "quadratic", 0.5), ("step", "linear", 0.0)])
def test_graphed_fast_sampler_matches_fastdpm_reference_loop(cuda, method, schedule, kappa):
    """Config-5 sampler: graph-captured FastDPM loop (fractional time steps, DDIM-style update) == the
    reference-style eager loop of util_fastdpmv2 on the same CPU noise stream."""
    import contextlib, io
    from point_diffusion_refinement_amd.pointnet2 import util_fastdpmv2 as F
    from point_diffusion_refinement_amd.pointnet2.configs import DIFFUSION_CONFIG
    from point_diffusion_refinement_amd.pointnet2.reverse_sampler import GraphedFastSampler
    net, fused = _pair(small_fused_config(), 23, cuda)
    dh = util.calc_diffusion_hyperparams(**DIFFUSION_CONFIG)
    g = torch.Generator().manual_seed(8)
    cond = torch.cat([torch.rand(2, 384, 3, generator=g) * 2 - 1, torch.ones(2, 384, 1)], 2).to(cuda)
    label = torch.tensor([3, 11], device=cuda)
    util.set_device(cuda)
    util.set_noise_source('cpu')
    try:
        torch.manual_seed(99)
        with contextlib.redirect_stdout(io.StringIO()):
            want = F.fast_sampling_function_v2(net, (2, 256, 3), dh, DIFFUSION_CONFIG, length=8,
                                               sampling_method=method, schedule=schedule, kappa=kappa, label=label,
                                               verbose=False, condition=cond)
    finally:
        util.set_device(None)
    for use_graph in (False, True):
        sampler = GraphedFastSampler(fused, dh, DIFFUSION_CONFIG, length=8, sampling_method=method,
                                     schedule=schedule, kappa=kappa, noise='cpu', use_graph=use_graph)
        torch.manual_seed(99)
        got = sampler.sample((2, 256, 3), cond, label)
        rel = ((got - want).abs() / (want.abs() + 1.0))
        assert rel.max() < 1e-3 and (rel < 1e-4).float().mean() > 0.99, (use_graph, rel.max())


def _random_layer_case(seed, cuda):
    """One random pdr_fused_layer problem + its float64 reference (aligned segments => the wave-specialised
    kernel; `gath` adds a gathered first-conv source: ball form with empty balls on even seeds, kNN form --
    two more per-position terms s1[p] r1[c] + s2[p] r2[c] -- on odd seeds)."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    rpb = int(rng.choice([16, 32, 96, 128, 160, 256, 384, 1000, 2048, 1 << 16]))   # last: many tiles per workgroup
    B = int(rng.integers(1, 4))
    K = int(rng.choice([8, 16, 32]))
    if rpb % K:
        rpb = (rpb // K + 1) * K
    P = B * rpb
    gath = bool(rng.integers(0, 2)) and 128 % K == 0
    nseg = int(rng.integers(1, 4))
    widths = [int(rng.choice([3, 4, 17, 32, 41, 64, 100, 128, 200])) for _ in range(nseg)]
    Cin = sum(widths)
    Cout = int(rng.choice([3, 32, 35, 64, 96, 105, 128, 140, 200, 256, 427]))
    segs, cols = [], []
    idx = cnt = knn = dense = None
    for si, C in enumerate(widths):
        ld = (C + 3) // 4 * 4 + 4 * int(rng.integers(0, 2))
        if gath and si == 0:
            n_src = int(rng.integers(K, 3 * K))
            U = torch.randn(B * n_src + 1, ld, generator=g)
            U[-1] = 0
            V2 = torch.randn(P // K, 2 * ld, generator=g)
            idx = torch.randint(0, n_src, (P,), generator=g, dtype=torch.int32)
            cnt = torch.randint(0, 3, (P // K,), generator=g, dtype=torch.int32)       # 1/3 empty balls
            bsel = torch.arange(P) // rpb
            rows = U[bsel * n_src + idx.long()][:, :C] + V2[torch.arange(P) // K][:, :C]
            if seed % 2:                                                              # kNN form
                cnt = None
                s1, s2 = torch.rand(P, generator=g), torch.rand(P, generator=g)
                r1, r2 = torch.randn(ld + 4, generator=g), torch.randn(ld + 4, generator=g)
                rows = rows + s1[:, None] * r1[None, :C] + s2[:, None] * r2[None, :C]
                knn = (s1.to(cuda), s2.to(cuda), r1.to(cuda), r2.to(cuda))
                gd = {"V": (V2.to(cuda), 0), "V0": None, "ldv": 2 * ld, "nsrc": n_src, "zrow": B * n_src,
                      "r1": (knn[2], 0), "r2": (knn[3], 0)}
                dense = torch.zeros(P, (C + 3) // 4 * 4)
                dense[:, :C] = rows
                cols.append(rows)
            else:
                empty = (cnt[torch.arange(P) // K] <= 0).unsqueeze(1)
                cols.append(torch.where(empty, V2[torch.arange(P) // K][:, ld:ld + C], rows))
                gd = {"V": (V2.to(cuda), 0), "V0": (V2.to(cuda), ld), "ldv": 2 * ld, "nsrc": n_src,
                      "zrow": B * n_src}
            segs.append((U.to(cuda), 0, C, ld, 1, gd))
        else:
            div = K if rng.integers(0, 3) == 0 else 1         # neighbour-broadcast segment (also next to a gathered one)
            t = torch.randn(P // div, ld, generator=g)
            cols.append(t[:, :C].repeat_interleave(div, 0))
            segs.append((t.to(cuda), 0, C, ld, div))
    x = torch.cat(cols, 1).double()
    has_ss, has_add = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    has_radd = bool(rng.integers(0, 2)) and nseg == 1 and not gath
    has_oadd = bool(rng.integers(0, 2))
    pre, post = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    scale = torch.randn(B, Cin, generator=g) if has_ss else None
    shift = torch.randn(B, Cin, generator=g) if has_ss else None
    add = torch.randn(B, Cin, generator=g) if has_add else None
    bidx = torch.arange(P) // rpb
    if pre:
        x = x.relu()
    if has_ss:
        x = x * scale[bidx].double() + shift[bidx].double()
    if post:
        x = x.relu()
    if has_add:
        x = x + add[bidx].double()
    radd = None
    if has_radd:
        rt = torch.randn(P, (Cin + 3) // 4 * 4, generator=g)
        x = x + rt[:, :Cin].double()
        radd = (rt.to(cuda), 0, Cin, rt.shape[1], 1)
    W = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    bias = torch.randn(Cout, generator=g)
    ref = x @ W.t().double() + bias.double()
    act = FN.Act(segs, P, B, rpb, scale=None if scale is None else scale.to(cuda),
                 shift=None if shift is None else shift.to(cuda), add=None if add is None else add.to(cuda),
                 add_ld=Cin, radd=radd, pre_relu=pre, post_relu=post)
    if gath:
        act.gidx, act.gcnt, act.gK = idx.to(cuda), None if cnt is None else cnt.to(cuda), K
        if knn is not None:
            act.gs1, act.gs2 = knn[0], knn[1]
            # what SplitFirstConv hands consumers without a kNN-gathering kernel (run_layer's fallback)
            act.first = type("First", (), {"materialise": staticmethod(lambda col0, C: dense.to(cuda))})
    if has_oadd:
        od = torch.randn(P // K, (Cout + 3) // 4 * 4, generator=g)
        ref = ref + od[:, :Cout].repeat_interleave(K, 0).double()
        act.oadd = (od.to(cuda), K)
    return act, _conv(W.to(cuda), bias.to(cuda)), ref, (B, rpb, Cout)


@pytest.mark.parametrize("P,rpb,Cin,Cout,div", [(2048, 64, 3, 201, 1), (65536, 2048, 3, 427, 1), (512, 16, 3, 1097, 1),
                                               (8192, 256, 4, 32, 1), (4096, 1024, 3, 3, 1), (4096, 128, 3, 105, 8)])
def test_thin_layer_kernel(cuda, P, rpb, Cin, Cout, div):
    """<= 4 input channels, no prologue, no statistics (the coordinate tables of the split first convs): the thin
    kernel must give the SAME BITS as the wave-specialised MFMA tile kernel (selected by asking for statistics) and
    match float64."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(P + Cout)
    x = torch.randn(P // div, 4, generator=g)
    W = torch.randn(Cout, Cin, generator=g)
    bias = torch.randn(Cout, generator=g)
    conv = _conv(W.to(cuda), bias.to(cuda))
    B = P // rpb
    act = FN.Act([(x.to(cuda), 0, Cin, 4, div)], P, B, rpb)
    plan = (ctypes.c_int * 8)()
    li = act.struct()
    Y0 = torch.empty(4, device=cuda)
    assert lib.pdr_fused_layer_plan(ctypes.byref(li), P, Cin, conv.Wt.data_ptr(), conv.ldw, Cout, Y0.data_ptr(),
                                    FN._ldy(Cout), plan) == 0
    assert plan[6] == 1
    thin, _, _ = FN.run_layer(act, conv, stats=False)
    tile, part, _ = FN.run_layer(act, conv, stats=True)
    torch.cuda.synchronize()
    if plan[0]:            # wave-specialised tile kernel: bias first, channels in MFMA order -- the same fma chain
        assert torch.equal(thin[:, :Cout], tile[:, :Cout])
    else:                  # uniform-wave kernel (32-row tiles): bias added last
        assert _rel(thin[:, :Cout].double().cpu(), tile[:, :Cout].double().cpu()) < 1e-6
    ref = x[:, :Cin].double().repeat_interleave(div, 0) @ W.t().double() + bias.double()
    assert _rel(thin[:, :Cout].double().cpu(), ref) < 1e-5


def _narrow_case(seed, cuda, B, rpb, Cin, Cout, kind, K=32):
    """One narrow single-source layer on 128-row tiles (tile variants 7 / 8) + float64 reference.  kind: 'plain', 'radd' (residual source) or 'gath' (ball-form gathered source, 1/3 empty balls)."""
    g = torch.Generator().manual_seed(seed)
    P = B * rpb
    ld = (Cin + 3) // 4 * 4 + 4 * (seed % 2)
    bidx = torch.arange(P) // rpb
    act_kw, gidx = {}, None
    if kind == "gath":
        n_src = 3 * K
        U = torch.randn(B * n_src + 1, ld, generator=g)
        U[-1] = 0
        V2 = torch.randn(P // K, 2 * ld, generator=g)
        idx = torch.randint(0, n_src, (P,), generator=g, dtype=torch.int32)
        cnt = torch.randint(0, 3, (P // K,), generator=g, dtype=torch.int32)
        q = torch.arange(P) // K
        rows = U[bidx * n_src + idx.long()][:, :Cin] + V2[q][:, :Cin]
        x = torch.where((cnt[q] <= 0).unsqueeze(1), V2[q][:, ld:ld + Cin], rows).double()
        V2c = V2.to(cuda)
        seg = (U.to(cuda), 0, Cin, ld, 1, {"V": (V2c, 0), "V0": (V2c, ld), "ldv": 2 * ld, "nsrc": n_src,
                                            "zrow": B * n_src})
        gidx = (idx.to(cuda), cnt.to(cuda))
    elif kind == "knn":          # kNN-form gathered source: U[idx] + V + s1 r1 + s2 r2, no empty balls
        n_src = 3 * K
        U = torch.randn(B * n_src + 1, ld, generator=g)
        V2 = torch.randn(P // K, ld, generator=g)
        idx = torch.randint(0, n_src, (P,), generator=g, dtype=torch.int32)
        s1, s2 = torch.rand(P, generator=g), torch.rand(P, generator=g)
        r1, r2 = torch.randn(ld + 4, generator=g), torch.randn(ld + 4, generator=g)
        q = torch.arange(P) // K
        rows = U[bidx * n_src + idx.long()][:, :Cin] + V2[q][:, :Cin]
        rows = rows + s1[:, None] * r1[None, :Cin] + s2[:, None] * r2[None, :Cin]
        x = rows.double()
        main_knn = (s1.to(cuda), s2.to(cuda), r1.to(cuda), r2.to(cuda))
        seg = (U.to(cuda), 0, Cin, ld, 1, {"V": (V2.to(cuda), 0), "V0": None, "ldv": ld, "nsrc": n_src,
                                            "zrow": B * n_src, "r1": (main_knn[2], 0), "r2": (main_knn[3], 0)})
        gidx = (idx.to(cuda), None)
    else:
        t = torch.randn(P, ld, generator=g)
        x = t[:, :Cin].double()
        seg = (t.to(cuda), 0, Cin, ld, 1)
    pre, post = bool(seed & 1), bool(seed & 2)
    has_ss, has_add, has_oadd = bool(seed & 4) or kind in ("radd", "rgath", "rknn"), bool(seed & 8), bool(seed & 16)
    scale = torch.randn(B, Cin, generator=g) if has_ss else None
    shift = torch.randn(B, Cin, generator=g) if has_ss else None
    add = torch.randn(B, Cin, generator=g) if has_add else None
    if pre:
        x = x.relu()
    if has_ss:
        x = x * scale[bidx].double() + shift[bidx].double()
    if post:
        x = x.relu()
    if has_add:
        x = x + add[bidx].double()
    radd = None
    if kind == "radd":
        rt = torch.randn(P, (Cin + 3) // 4 * 4, generator=g)
        x = x + rt[:, :Cin].double()
        radd = (rt.to(cuda), 0, Cin, rt.shape[1], 1)
    if kind == "rgath":          # residual = a gathered first-conv window (ball form, 1/3 empty balls)
        n_src, ldr = 3 * K, (Cin + 3) // 4 * 4 + 4
        U = torch.randn(B * n_src + 1, ldr, generator=g)
        U[-1] = 0
        V2 = torch.randn(P // K, 2 * ldr, generator=g)
        idx = torch.randint(0, n_src, (P,), generator=g, dtype=torch.int32)
        cnt = torch.randint(0, 3, (P // K,), generator=g, dtype=torch.int32)
        q = torch.arange(P) // K
        rows = U[bidx * n_src + idx.long()][:, :Cin] + V2[q][:, :Cin]
        x = x + torch.where((cnt[q] <= 0).unsqueeze(1), V2[q][:, ldr:ldr + Cin], rows).double()
        V2c = V2.to(cuda)
        radd = (U.to(cuda), 0, Cin, ldr, 1, {"V": (V2c, 0), "V0": (V2c, ldr), "ldv": 2 * ldr, "nsrc": n_src,
                                              "zrow": B * n_src})
        gidx = (idx.to(cuda), cnt.to(cuda))
    knn = None
    if kind == "rknn":           # residual = a gathered first-conv window, kNN form (+ s1 r1 + s2 r2, no empty balls)
        n_src, ldr = 3 * K, (Cin + 3) // 4 * 4 + 4
        U = torch.randn(B * n_src + 1, ldr, generator=g)
        V2 = torch.randn(P // K, ldr, generator=g)
        idx = torch.randint(0, n_src, (P,), generator=g, dtype=torch.int32)
        s1, s2 = torch.rand(P, generator=g), torch.rand(P, generator=g)
        r1, r2 = torch.randn(ldr + 4, generator=g), torch.randn(ldr + 4, generator=g)
        q = torch.arange(P) // K
        rows = U[bidx * n_src + idx.long()][:, :Cin] + V2[q][:, :Cin]
        rows = rows + s1[:, None] * r1[None, :Cin] + s2[:, None] * r2[None, :Cin]
        x = x + rows.double()
        knn = (s1.to(cuda), s2.to(cuda), r1.to(cuda), r2.to(cuda))
        radd = (U.to(cuda), 0, Cin, ldr, 1, {"V": (V2.to(cuda), 0), "V0": None, "ldv": ldr, "nsrc": n_src,
                                              "zrow": B * n_src, "r1": (knn[2], 0), "r2": (knn[3], 0)})
        gidx = (idx.to(cuda), None)
        dense = torch.zeros(P, (Cin + 3) // 4 * 4)
        dense[:, :Cin] = rows
    W = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    bias = torch.randn(Cout, generator=g)
    ref = x @ W.t().double() + bias.double()
    act = FN.Act([seg], P, B, rpb, scale=None if scale is None else scale.to(cuda),
                 shift=None if shift is None else shift.to(cuda), add=None if add is None else add.to(cuda),
                 add_ld=Cin, radd=radd, pre_relu=pre, post_relu=post)
    if gidx is not None:
        act.gidx, act.gcnt, act.gK = gidx[0], gidx[1], K
    if kind == "knn":
        act.gs1, act.gs2 = main_knn[0], main_knn[1]
    if knn is not None:
        act.gs1, act.gs2 = knn[0], knn[1]
        # what SplitFirstConv hands consumers without a kNN-gathering kernel (run_layer's fallback)
        act.first = type("First", (), {"materialise": staticmethod(lambda col0, C: dense.to(cuda))})
    if has_oadd:
        od = torch.randn(P // K, (Cout + 3) // 4 * 4, generator=g)
        ref = ref + od[:, :Cout].repeat_interleave(K, 0).double()
        act.oadd = (od.to(cuda), K)
    return act, _conv(W.to(cuda), bias.to(cuda)), ref


@pytest.mark.parametrize("kind", ["plain", "radd", "gath", "rgath", "rknn"])
def test_narrow_layers_on_128_row_tiles(cuda, kind):
    """Tile variants 7 / 8 (128 rows, 32-channel chunks: the level-0 / level-1 narrow layers): channel counts that
    end inside a chunk, all prologue / epilogue options, more tiles than resident workgroups (persistent loop) with
    an odd number of tiles per cloud, one-tile clouds."""
    lib = _lib.load()
    shapes = [(3, 128, 32, 32), (2, 256, 17, 32), (2, 384, 41, 32), (1, 1024, 44, 64), (2, 128, 64, 64),
              (3, 2048, 33, 64), (2, 4096, 48, 32), (5, 128 * 1365, 32, 32), (3, 128 * 1501, 64, 64)]
    for n, (B, rpb, Cin, Cout) in enumerate(shapes):
        for seed in ((n, n + 13, n + 31) if rpb < 100000 else (n + 7,)):
            act, conv, ref = _narrow_case(seed, cuda, B, rpb, Cin, Cout, kind)
            plan = (ctypes.c_int * 8)()
            li = act.struct()
            Y0 = torch.empty(1, device=cuda)
            assert lib.pdr_fused_layer_plan(ctypes.byref(li), act.P, Cin, conv.Wt.data_ptr(), conv.ldw, Cout,
                                            Y0.data_ptr(), (Cout + 3) // 4 * 4, plan) == 0
            assert plan[0] == 1 and plan[1] == (7 if Cout <= 32 else 8), (kind, B, rpb, Cin, Cout, list(plan[:6]))
            rc0 = (0, Cout // 2 + 1, Cout)[seed % 3]
            Y, part, tpb = FN.run_layer(act, conv, stats=True, relu_col0=rc0)
            torch.cuda.synchronize()
            assert tpb == rpb // 128
            got = Y[:, :Cout].double().cpu()
            assert torch.isfinite(got).all()
            assert _rel(got, ref) < 5e-5, (kind, B, rpb, Cin, Cout, seed, _rel(got, ref))
            f = ref.clone()
            f[:, rc0:] = f[:, rc0:].relu()
            s1 = f.view(B, rpb, Cout).sum(1)
            s2 = (f * f).view(B, rpb, Cout).sum(1)
            st = part.view(B, tpb, Cout, 2).double().sum(1).cpu()
            assert _rel(st[..., 0], s1) < 2e-4 and _rel(st[..., 1], s2) < 2e-4, (kind, B, rpb, Cin, Cout, seed)


# (B = 8 / 16 / 24: whole groups of 8 clouds take the XCD-local tile order of the gathered kernels; 10: the plain one)
@pytest.mark.parametrize("B,rpb,Cin,Cout", [(2, 256, 128, 128), (3, 64, 256, 256), (2, 1024, 100, 140), (2, 384, 64, 96),
                                            (8, 256, 128, 128), (16, 128, 64, 96), (24, 512, 128, 128), (10, 256, 128, 128)])
@pytest.mark.parametrize("kind", ["rgath", "rknn"])
def test_gathered_residual_on_wide_tiles(cuda, B, rpb, Cin, Cout, kind):
    """A gathered residual (the residual conv of a virtual first conv) through the 128- / 64-row wide tiles and
    through a shape without a wave-specialised instantiation (128 x 160: uniform-wave kernel)."""
    for seed in (3, 12, 21):
        act, conv, ref = _narrow_case(seed, cuda, B, rpb, Cin, Cout, kind)
        Y, part, tpb = FN.run_layer(act, conv, stats=True, relu_col0=Cout)
        torch.cuda.synchronize()
        got = Y[:, :Cout].double().cpu()
        assert _rel(got, ref) < 5e-5, (B, rpb, Cin, Cout, seed, _rel(got, ref))
        st = part.view(B, tpb, Cout, 2).double().sum(1).cpu()
        assert _rel(st[..., 0], ref.view(B, rpb, Cout).sum(1)) < 2e-4


# (B = 8 / 16: the XCD-local tile order; 10: the plain one; 16384 rows per cloud at B = 8: eight tiles per persistent
# workgroup, the launch shape of the dominant kernel of the step)
@pytest.mark.parametrize("B,rpb,Cin,Cout,K", [(2, 256, 128, 128, 8), (8, 16384, 128, 128, 8), (10, 128 * 33, 96, 128, 8),
                                              (16, 128 * 9, 160, 256, 16), (3, 192, 100, 96, 8), (2, 1024, 75, 64, 8)])
def test_knn_gathered_source_on_wide_and_narrow_tiles(cuda, B, rpb, Cin, Cout, K):
    """The kNN-form gathered first conv as the MAIN source (U[idx] + V + d2 r1 + w r2: the second convs of the
    feature-propagation blocks, `fused_layer_ws_kernel<..., GATH = 2>` -- the dominant kernel of the step) against the
    float64 layer, output and per-tile moments; whole and partial row tiles, channel counts that end inside a chunk."""
    lib = _lib.load()
    for seed in (5, 6):
        act, conv, ref = _narrow_case(seed, cuda, B, rpb, Cin, Cout, "knn", K=K)
        plan = (ctypes.c_int * 8)()
        li = act.struct()
        Y0 = torch.empty(1, device=cuda)
        assert lib.pdr_fused_layer_plan(ctypes.byref(li), act.P, Cin, conv.Wt.data_ptr(), conv.ldw, Cout,
                                        Y0.data_ptr(), (Cout + 3) // 4 * 4, plan) == 0
        assert plan[0] == 1 and plan[3] == 2, list(plan[:6])      # wave-specialised, kNN-form gathered source
        Y, part, tpb = FN.run_layer(act, conv, stats=True, relu_col0=Cout // 2)
        torch.cuda.synchronize()
        got = Y[:, :Cout].double().cpu()
        assert torch.isfinite(got).all() and _rel(got, ref) < 5e-5, (B, rpb, Cin, Cout, seed, _rel(got, ref))
        f = ref.clone()
        f[:, Cout // 2:] = f[:, Cout // 2:].relu()
        st = part.view(B, tpb, Cout, 2).double().sum(1).cpu()
        assert _rel(st[..., 0], f.view(B, rpb, Cout).sum(1)) < 2e-4
        assert _rel(st[..., 1], (f * f).view(B, rpb, Cout).sum(1)) < 2e-4


@pytest.mark.parametrize("B,rpb,Cin,Cout,deep", [
    (32, 16, 512, 512, True), (4, 16, 320, 300, True), (32, 16, 643, 1163, False),      # 32-row tiles: <= 256 jobs
    (32, 64, 256, 256, True), (8, 64, 200, 70, True), (32, 64, 515, 512, True), (32, 64, 323, 1097, False),
    (32, 256, 128, 128, True), (2, 384, 331, 200, True), (32, 256, 387, 512, False), (32, 512, 128, 128, True),
    (32, 256, 64, 128, False)])
@pytest.mark.parametrize("kind", ["plain", "radd"])
def test_right_sized_tiny_layers(cuda, B, rpb, Cin, Cout, deep, kind):
    """The per-point layers of the deep levels (a few dozen workgroups per launch) run on the uniform-wave kernel with
    128-channel chunks and half-width tiles where every workgroup of the launch is resident at once
    (pdr_fused_layer_plan out[7]); the shapes of the DDPM step at B = 32, shapes on both sides of the job bounds, channel
    counts that end inside a chunk, every prologue option, against the float64 layer (output and per-tile moments)."""
    lib = _lib.load()
    for seed in (4, 11):
        act, conv, ref = _narrow_case(seed, cuda, B, rpb, Cin, Cout, kind, K=16)
        plan = (ctypes.c_int * 8)()
        li = act.struct()
        Y0 = torch.empty(1, device=cuda)
        assert lib.pdr_fused_layer_plan(ctypes.byref(li), act.P, Cin, conv.Wt.data_ptr(), conv.ldw, Cout,
                                        Y0.data_ptr(), (Cout + 3) // 4 * 4, plan) == 0
        assert (plan[7] == 128) == deep and (not deep or plan[0] == 0 or plan[1] == 6), (list(plan), deep)
        rc0 = (0, Cout // 2 + 1, Cout)[seed % 3]
        Y, part, tpb = FN.run_layer(act, conv, stats=True, relu_col0=rc0)
        torch.cuda.synchronize()
        got = Y[:, :Cout].double().cpu()
        assert torch.isfinite(got).all() and _rel(got, ref) < 5e-5, (kind, B, rpb, Cin, Cout, seed, _rel(got, ref))
        f = ref.clone()
        f[:, rc0:] = f[:, rc0:].relu()
        st = part.view(B, tpb, Cout, 2).double().sum(1).cpu()
        assert _rel(st[..., 0], f.view(B, rpb, Cout).sum(1)) < 2e-4, (kind, B, rpb, Cin, Cout, seed)
        assert _rel(st[..., 1], (f * f).view(B, rpb, Cout).sum(1)) < 2e-4, (kind, B, rpb, Cin, Cout, seed)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ws", ["1", "0"])
def test_fused_layer_random_sweep(cuda, ws, monkeypatch):
    """60 random layer problems through both kernel families (option fused_ws is applied by the child binding, so the
    uniform-wave family is exercised in a child process)."""
    if ws == "0":
        import subprocess, sys, os
        env = dict(os.environ, PDR_OPTIONS="fused_ws=0", PDR_SWEEP_CHILD="1")
        r = subprocess.run([sys.executable, "-m", "pytest", __file__, "-q", "-x", "-m", "gpu", "-k",
                            "random_sweep and 1"], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    relu_cols = [0, 17, 10 ** 6]
    for seed in range(60):
        act, conv, ref, (B, rpb, Cout) = _random_layer_case(seed, cuda)
        rc0 = relu_cols[seed % 3]
        Y, part, tpb = FN.run_layer(act, conv, stats=True, relu_col0=min(rc0, Cout))
        torch.cuda.synchronize()
        got = Y[:, :Cout].double().cpu()
        assert torch.isfinite(got).all(), seed
        assert _rel(got, ref) < 5e-5, (seed, _rel(got, ref))
        f = ref.clone()
        f[:, min(rc0, Cout):] = f[:, min(rc0, Cout):].relu()
        s1 = f.view(B, rpb, Cout).sum(1)
        s2 = (f * f).view(B, rpb, Cout).sum(1)
        st = part.view(B, tpb, Cout, 2).double().sum(1).cpu()
        assert _rel(st[..., 0], s1) < 2e-4 and _rel(st[..., 1], s2) < 2e-4, seed


@pytest.mark.parametrize("cfg_name", ["small", "ddpm"])
def test_fused_first_call_runs_the_condition_branch(cuda, cfg_name):
    """First call of a batch (condition branch + global PointNet, pointnet2_with_pcld_condition.py:360-414 of the
    reference) through the fused blocks == layer-by-layer path: output AND the retained features."""
    if cfg_name == "small":
        net, fused = _pair(small_fused_config(), 25, cuda)
        g = torch.Generator().manual_seed(9)
        x = torch.randn(2, 256, 3, generator=g).to(cuda)
        cond = torch.cat([torch.rand(2, 384, 3, generator=g) * 2 - 1, torch.ones(2, 384, 1)], 2).to(cuda)
        ts, label = torch.tensor([7.0, 3.0], device=cuda), torch.tensor([2, 9], device=cuda)
    else:
        torch.manual_seed(1)
        net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)
        fused = FN.FusedCloudConditionNet(net)
        x, cond, label = synthetic_batch(2, seed=5, device=cuda)
        ts = torch.tensor([999.0, 40.0], device=cuda)

    def close(a, b, what):
        err = ((a - b).abs() / (b.abs() + 1.0))
        assert err.max() < 1e-2 and (err < 1e-3).float().mean() > 0.99, (what, float(err.max()))

    with torch.no_grad():
        net.reset_cond_features()
        ref = net(x, cond, ts=ts, label=label, use_retained_condition_feature=True)
        ref_cache = ([net.global_feature.clone()] + [f.clone() for f in net.encoder_cond_features] +
                     [f.clone() for f in net.decoder_cond_features])
        fused.reset_cond_features()
        assert net.encoder_cond_features is None
        got = fused(x, cond, ts=ts, label=label, use_retained_condition_feature=True)
        got_cache = [net.global_feature] + list(net.encoder_cond_features) + list(net.decoder_cond_features)
        close(got, ref, "eps")
        assert len(got_cache) == len(ref_cache)
        for i, (a, b) in enumerate(zip(got_cache, ref_cache)):
            assert a.shape == b.shape
            close(a, b, "cache %d" % i)
        # a cached step on top of the fused-filled cache
        got2 = fused(x * 0.9, cond, ts=ts - 1, label=label, use_retained_condition_feature=True)
        ref2 = net(x * 0.9, cond, ts=ts - 1, label=label, use_retained_condition_feature=True)
        close(got2, ref2, "cached eps")
        # not retained (the refinement stage calls the network this way): same output, nothing kept
        fused.reset_cond_features()
        got3 = fused(x, cond, ts=ts, label=label, use_retained_condition_feature=False)
        close(got3, ref, "unretained eps")
        assert net.encoder_cond_features is None and net.global_feature is None


@pytest.mark.parametrize("B,npoint,K,D,ld,use_counts", [(2, 64, 32, 32, 32, True), (3, 100, 8, 64, 72, False),
                                                        (1, 16, 16, 128, 128, True), (2, 2048, 32, 32, 32, True),
                                                        (2, 50, 8, 256, 256, False), (2, 33, 32, 64, 64, True),
                                                        (1, 7, 8, 8, 8, True), (1, 9, 32, 512, 512, True)])
def test_attention_pool_matches_masked_softmax(cuda, B, npoint, K, D, ld, use_counts):
    """pdr_attention_pool == count mask (-1e9), softmax over the K neighbours, weighted sum of
    relu(values * scale + shift)  (attention.py:83-96), against float64 torch."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * 1000 + npoint + K)
    P = B * npoint * K
    scores = (torch.randn(P, ld, generator=g) * 3).to(cuda)
    values = torch.randn(P, ld, generator=g).to(cuda)
    vs, vh = torch.randn(B, D, generator=g).to(cuda), torch.randn(B, D, generator=g).to(cuda)
    counts = torch.randint(0, K + 1, (B, npoint), generator=g, dtype=torch.int32).to(cuda) if use_counts else None
    out = torch.empty(B * npoint, D, device=cuda)
    _lib.check(lib.pdr_attention_pool(scores.data_ptr(), ld, values.data_ptr(), ld, vs.data_ptr(), vh.data_ptr(), 1,
                                      counts.data_ptr() if use_counts else None, B, npoint, K, D, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "attention_pool")
    s = scores[:, :D].double().view(B, npoint, K, D)
    v = values[:, :D].double().view(B, npoint, K, D)
    v = (v * vs.double().view(B, 1, 1, D) + vh.double().view(B, 1, 1, D)).relu()
    if use_counts:
        c = counts.clamp(min=1).view(B, npoint, 1, 1)
        mask = torch.arange(K, device=cuda).view(1, 1, K, 1) >= c
        s = torch.where(mask, torch.full_like(s, -1e9), s)
    want = (torch.softmax(s, dim=2) * v).sum(2).view(B * npoint, D)
    assert _rel(out.double(), want) < 2e-6


# ------------------------------------------------------------------ split-f16 (opt-in) arithmetic
@pytest.mark.parametrize("P,Cin,Cout,rpb,segs", [(1024, 128, 128, 256, (128,)), (2048, 331, 331, 1024, (171, 160)),
                                                 (512, 512, 512, 64, (512,)), (4096, 203, 128, 4096, (200, 3)),
                                                 (1 << 16, 256, 256, 8192, (128, 128)),
                                                 (4096, 256, 64, 1024, (256,)), (2048, 140, 64, 256, (128, 12))])
def test_split_f16_layer_vs_float64(cuda, P, Cin, Cout, rpb, segs, monkeypatch):
    """pdr_fused_layer_f16x3 (x . w = xh wh + xh wl + xl wh on f16 MFMA, fp32 accumulate; both operands held as two
    11-bit halves): every element within 2e-6 of the float64 result RELATIVE TO THE ROW's |x| . |w| scale -- the bar of
    the exact fp32 kernel (measured: 2.6e-7 vs 3.7e-7 exact) -- incl. multi-segment inputs, a partial last chunk, the
    prologue and a residual; statistics as in the exact kernel.  The last two shapes run on the 64-column tile
    variant (64-column weight image)."""
    g = torch.Generator().manual_seed(Cin * 3 + Cout)
    B = P // rpb
    xs, off = [], 0
    for C in segs:
        ld = (C + 3) // 4 * 4
        t = torch.full((P, ld), float("nan"))
        t[:, :C] = torch.randn(P, C, generator=g)
        xs.append((t.to(cuda), C, ld))
    scale, shift, add = (torch.randn(B, Cin, generator=g).to(cuda) for _ in range(3))
    W = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(cuda)
    bias = torch.randn(Cout, generator=g).to(cuda)
    conv = _conv(W, bias)
    bidx = torch.arange(P, device=cuda) // rpb
    x = torch.cat([t[:, :C] for t, C, _ in xs], 1)
    act = FN.Act([(t, 0, C, ld, 1) for t, C, ld in xs], P, B, rpb, scale=scale, shift=shift, add=add, add_ld=Cin,
                 post_relu=True)
    xin = (x * scale[bidx] + shift[bidx]).relu() + add[bidx]
    ref = xin.double() @ W.t().double() + bias.double()
    bound = (xin.abs().double() @ W.t().abs().double()) + 1.0
    monkeypatch.setattr(FN, "_PRECISION", ["split_f16"])
    lib = _lib.load()
    Y = torch.empty((P, FN._ldy(Cout)), device=cuda)
    tm = lib.pdr_fused_layer_tile_rows(rpb, Cout)
    tpb = (rpb + tm - 1) // tm
    part = torch.empty((B * tpb, Cout, 2), device=cuda)
    assert FN._run_layer_split(lib, act, conv, act.struct(), Y.data_ptr(), Y.shape[1], part, Cout,
                               tiny_exact=False), "split path not taken"
    err = ((Y[:, :Cout].double() - ref).abs() / bound)
    assert float(err.max()) < 2e-6, float(err.max())
    got = part.view(B, tpb, Cout, 2).double().sum(1)
    # (sums over rpb rows cancel: judge them against the sum of magnitudes)
    scale_sum = ref.abs().view(B, rpb, Cout).sum(1) + 1.0
    assert float(((got[..., 0] - ref.view(B, rpb, Cout).sum(1)).abs() / scale_sum).max()) < 1e-5
    assert float(((got[..., 1] - (ref * ref).view(B, rpb, Cout).sum(1)).abs() /
                  ((ref * ref).view(B, rpb, Cout).sum(1) + 1.0)).max()) < 1e-5
    # the mode really changes the arithmetic: not the bytes of the exact kernel, which meets the same bar
    monkeypatch.setattr(FN, "_PRECISION", ["f32"])
    Ye, _, _ = FN.run_layer(act, conv, stats=True)
    exact = ((Ye[:, :Cout].double() - ref).abs() / bound)
    assert float(exact.max()) < 2e-6 and not torch.equal(Ye[:, :Cout], Y[:, :Cout])


@pytest.mark.parametrize("magnitude,bar", [(1.0, 1e-6), (1e-2, 4e-6), (1e-4, 4e-4)])
def test_split_f16_representation_floor(cuda, magnitude, bar, monkeypatch):
    """The documented contract of the f16 hi + lo representation (include/pdr_hip.h): an operand is held to
    max(2^-23 |x|, 2^-25).  Inputs of rms 1 and 1e-2 (lo parts subnormal halves, which the MFMA honours) stay at the
    fp32 class (measured 2.6e-7 / 9.3e-7); at rms 1e-4 the absolute floor shows (1.0e-4) -- the reason the mode is
    opt-in and fed GroupNorm outputs, coordinates and embeddings only."""
    P, Cin, Cout, rpb = 1 << 14, 256, 256, 4096
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(P, Cin, generator=g) * magnitude).to(cuda)
    W = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(cuda)
    conv = _conv(W, torch.zeros(Cout, device=cuda))
    act = FN.Act([(x, 0, Cin, Cin, 1)], P, P // rpb, rpb)
    ref = x.double() @ W.t().double()
    bound = x.abs().double() @ W.t().abs().double()
    monkeypatch.setattr(FN, "_PRECISION", ["split_f16"])
    lib = _lib.load()
    Y = torch.empty((P, FN._ldy(Cout)), device=cuda)
    tm = lib.pdr_fused_layer_tile_rows(rpb, Cout)
    part = torch.empty(((P // rpb) * ((rpb + tm - 1) // tm), Cout, 2), device=cuda)
    assert FN._run_layer_split(lib, act, conv, act.struct(), Y.data_ptr(), Y.shape[1], part, Cout,
                               tiny_exact=False), "split path not taken"
    err = float(((Y[:, :Cout].double() - ref).abs() / bound).max())
    assert err < bar, err


def test_split_f16_large_activations_saturate_instead_of_nan(cuda, monkeypatch):
    """ADVICE r3 / include/pdr_hip.h range contract: activations beyond the f16 range.  65504 < |x| <= 131008 is
    carried by hi = +-65504 plus lo (MODE.FP16_OVFL clamps the conversions) at 2^-12 relative or better; beyond that the
    operand saturates -- the output is FINITE and equals the product of the clamped operand; never NaN / inf (which is
    what hi = inf, lo = x - inf = -inf produced before)."""
    P, Cin, Cout, rpb = 1 << 12, 128, 128, 1024
    g = torch.Generator().manual_seed(6)
    x = torch.randn(P, Cin, generator=g)
    x[::7, ::5] *= 4.0e4                                   # many values in (65504, 131008]
    x[3::64, 1::9] = 9.0e4 * torch.sign(x[3::64, 1::9])
    inside = x.clamp(-1.3e5, 1.3e5)
    assert float(inside.abs().max()) <= 131008 and int((inside.abs() > 65504).sum()) > 100
    W = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(cuda)
    conv = _conv(W, torch.zeros(Cout, device=cuda))
    monkeypatch.setattr(FN, "_PRECISION", ["split_f16"])
    lib = _lib.load()

    def run(xin):
        xin = xin.to(cuda)
        act = FN.Act([(xin, 0, Cin, Cin, 1)], P, P // rpb, rpb)
        Y = torch.empty((P, FN._ldy(Cout)), device=cuda)
        tm = lib.pdr_fused_layer_tile_rows(rpb, Cout)
        part = torch.empty(((P // rpb) * ((rpb + tm - 1) // tm), Cout, 2), device=cuda)
        assert FN._run_layer_split(lib, act, conv, act.struct(), Y.data_ptr(), Y.shape[1], part, Cout,
                                   tiny_exact=False), "split path not taken"
        return Y[:, :Cout].double().cpu(), xin.double().cpu()
    Y, xd = run(inside)
    assert bool(torch.isfinite(Y).all())
    ref = xd @ W.t().double().cpu()
    bound = xd.abs() @ W.t().abs().double().cpu()
    assert float(((Y - ref).abs() / bound).max()) < 2.0 ** -11       # worst operand: 2^-12 relative
    beyond = inside.clone()
    beyond[5::128, 2::11] = 1.0e6                                     # far outside: saturates at 131008
    Y2, xd2 = run(beyond)
    assert bool(torch.isfinite(Y2).all()), "saturation must not produce inf / NaN"
    ref2 = xd2.clamp(-131008.0, 131008.0) @ W.t().double().cpu()
    assert float(((Y2 - ref2).abs() / (xd2.clamp(-131008.0, 131008.0).abs() @ W.t().abs().double().cpu())).max()) \
        < 2.0 ** -11


def test_split_f16_network_and_sampler(cuda):
    """Opt-in precision='split_f16' on the shipped DDPM architecture: eps vs the exact fused network and vs the
    layer-by-layer network at north_star's 1e-4 (|d| / max(|want|, rms); measured 1.2e-5 max, 1.2e-6 median -- the
    exact fused network sits at 6.7e-6 / 6.8e-7 from the layer-by-layer one), and the graph-captured sampler vs the
    reference-style loop under the same thresholds as the exact mode
    (test_fused_network_ddpm_config_and_graphed_sampler)."""
    from tests import parity
    torch.manual_seed(0)
    net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)
    exact = FN.FusedCloudConditionNet(net)
    split = FN.FusedCloudConditionNet(net, precision="split_f16")
    x, cond, label = synthetic_batch(2, seed=3, device=cuda)
    ts = torch.tensor([500.0, 20.0], device=cuda)
    a, ref = _cached_eps(net, exact, x, cond, ts, label)
    b, _ = _cached_eps(net, split, x, cond, ts, label)
    parity.check("split_f16:eps_vs_exact_fused", "hip", b, a, 1e-4)
    parity.check("split_f16:eps_vs_layer_by_layer", "hip", b, ref, 1e-4)
    assert float((a - b).abs().max()) > 0.0                               # the split kernels really ran
    dh = util.calc_diffusion_hyperparams(6, 1e-4, 0.02)
    util.set_device(cuda)
    util.set_noise_source('cpu')
    torch.manual_seed(77)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        want = util.sampling(net, (2, 2048, 3), dh, label=label, verbose=False, condition=cond)
    util.set_device(None)
    torch.manual_seed(77)
    got = GraphedReverseSampler(split, dh, noise='cpu', use_graph=True).sample((2, 2048, 3), cond, label)
    per_cloud = ((got - want).abs() / (want.abs() + 1.0)).flatten(1)
    # measured medians 6.5e-7 / 4.9e-6 (the second cloud carries a flipped near-tie, as clouds of the exact mode do)
    assert (per_cloud.median(1).values < 1e-4).all(), per_cloud.median(1).values
    assert int((per_cloud.max(1).values < 1e-3).sum()) >= 1 and float(per_cloud.max()) < 0.5, per_cloud.max(1).values


@pytest.mark.parametrize("case", ["ball_empty_all", "ball_window", "ball_no_counts", "knn", "ragged_tile"])
def test_gather_add_matches_torch(cuda, case):
    """pdr_gather_add alone (the network tests only see it through whole blocks): Y = U[idx] + V (V0 for empty balls,
    + d2 r1 + w r2 for the kNN form) bit for bit against torch, the per-tile GroupNorm moments (ReLU from relu_col0 on)
    against float64; written column windows; a last tile of a cloud that is not full."""
    import ctypes
    from tools.lab.gather_add_bench import reference
    rpb, K, Cout, n_src, has_em, has_s, relu_col0, win = {
        "ball_empty_all": (1024, 32, 96, 300, True, False, 64, None),
        "ball_window": (512, 32, 72, 128, True, False, 40, (8, 24)),
        "ball_no_counts": (1024, 16, 160, 257, False, False, 0, None),
        "knn": (640, 8, 44, 64, False, True, 44, None),
        "ragged_tile": (1024 + 64, 32, 64, 99, True, False, 32, None),
    }[case]
    lib = _lib.load()
    B, dev = 3, cuda
    g = torch.Generator(device=dev).manual_seed(len(case))
    P, ld = B * rpb, (Cout + 3) // 4 * 4
    U = torch.randn(B * n_src + 1, ld, device=dev, generator=g)
    V2 = torch.randn(P // K, 2 * ld, device=dev, generator=g)
    idx = torch.randint(0, n_src, (P,), device=dev, dtype=torch.int32, generator=g)
    cnt = torch.randint(0, 3, (P // K,), device=dev, dtype=torch.int32, generator=g) if has_em else None
    s1 = torch.rand(P, device=dev, generator=g) if has_s else None
    s2 = torch.rand(P, device=dev, generator=g) if has_s else None
    r1 = torch.randn(ld + 4, device=dev, generator=g) if has_s else None
    r2 = torch.randn(ld + 4, device=dev, generator=g) if has_s else None
    tpb = (rpb + 127) // 128
    partial = torch.full((B * tpb, Cout, 2), float("nan"), device=dev)
    y0, yc = win if win else (0, -1)
    Y = torch.full((P, (yc + 3) // 4 * 4 if win else ld), float("nan"), device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.pdr_gather_add(U.data_ptr(), ld, n_src, V2.data_ptr(), V2.data_ptr() + 4 * ld if has_em else None,
                                  2 * ld, idx.data_ptr(), p(cnt), p(s1), p(r1), p(s2), p(r2), B, rpb, K, Cout,
                                  Y.data_ptr(), Y.shape[1], partial.data_ptr(), relu_col0, y0, yc,
                                  torch.cuda.current_stream().cuda_stream), "gather_add")
    torch.cuda.synchronize()
    # the tool's reference assumes whole tiles: evaluate it on rows padded per cloud to whole tiles for the moments
    want, _ = reference(U, V2, ld, idx, cnt, s1, r1, s2, r2, B, rpb, K, Cout, n_src, relu_col0)
    w = want[:, y0:y0 + (yc if win else Cout)]
    if has_s:       # torch's addcmul need not contract like the kernel's fma: one rounding per term
        assert ((Y[:, :w.shape[1]] - w).abs() <= 2e-6 * (w.abs() + 1)).all()
    else:
        assert torch.equal(Y[:, :w.shape[1]], w)
    f = want.double()
    f[:, relu_col0:] = f[:, relu_col0:].clamp_min(0)
    f = f.view(B, rpb, Cout)
    for t in range(tpb):
        blk = f[:, t * 128:(t + 1) * 128]
        wm = torch.stack([blk.sum(1), (blk * blk).sum(1)], -1)
        got = partial.view(B, tpb, Cout, 2)[:, t].double()
        assert ((got - wm).abs() <= 1e-4 * (wm.abs() + 1)).all(), (case, t)


def _ball_like_neighbourhoods(B, m, K, n_src, dev, seed, frac_many=0.1, small=3):
    """idx / counts as ball_query leaves them: slots >= count repeat the first hit; counts 0 .. small-1 and a few 7."""
    g = torch.Generator(device=dev).manual_seed(seed)
    counts = torch.randint(0, small, (B, m), device=dev, dtype=torch.int32, generator=g)
    counts[torch.rand(B, m, device=dev, generator=g) < frac_many] = 7
    first = torch.randint(0, n_src, (B, m, 1), device=dev, dtype=torch.int32, generator=g)
    rest = torch.randint(0, n_src, (B, m, K), device=dev, dtype=torch.int32, generator=g)
    slot = torch.arange(K, device=dev)[None, None, :]
    idx = torch.where(slot < counts[:, :, None], rest, first.expand(B, m, K)).contiguous()
    idx[:, :, 0] = first[:, :, 0]
    return idx, counts


@pytest.mark.parametrize("K", [32, 8])
def test_dedup_plan_tiles_and_weighted_moments_equal_the_whole_first_conv(cuda, K):
    """pdr_dedup_plan (valid tiles = any query with more than one neighbour, ascending list, first neighbours, weights)
    and the three launches that replace a whole pdr_gather_add -- pdr_gather_add_tiles over the valid tiles, the
    per-query pdr_gather_add (K = 1), pdr_weighted_moments -- give the same per-cloud GroupNorm moments; valid tiles'
    partial rows are bit-equal, skipped tiles' rows zero."""
    lib, dev = _lib.load(), cuda
    B, m, Cout, n_src, relu_col0 = 3, 1024, 96, 700, 64
    ld, qpt = Cout, 128 // K
    g = torch.Generator(device=dev).manual_seed(K)
    U = torch.randn(B * n_src + 1, ld, device=dev, generator=g)
    V2 = torch.randn(B * m, 2 * ld, device=dev, generator=g)
    # (a tile of 128 / K queries is skipped when ALL of them have <= 1 neighbour)
    idx, counts = _ball_like_neighbourhoods(B, m, K, n_src, dev, 10 + K, *((0.1, 3) if K == 32 else (0.05, 2)))
    st = torch.cuda.current_stream().cuda_stream
    tpb, tpbd = m * K // 128, (m + 127) // 128
    ptpb = tpb + tpbd
    full = torch.empty(B * tpb, Cout, 2, device=dev)
    tabs = (U.data_ptr(), ld, n_src, V2.data_ptr(), V2.data_ptr() + 4 * ld, 2 * ld)
    _lib.check(lib.pdr_gather_add(*tabs, idx.data_ptr(), counts.data_ptr(), None, None, None, None, B, m * K, K, Cout,
                                  None, ld, full.data_ptr(), relu_col0, 0, -1, st), "gather_add")
    idx0 = torch.empty(B, m, dtype=torch.int32, device=dev)
    row_w = torch.empty(B * m, device=dev)
    tv = torch.empty(B * tpb, dtype=torch.uint8, device=dev)
    tl = torch.full((B * tpb,), -1, dtype=torch.int32, device=dev)
    nt = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.pdr_dedup_plan(idx.data_ptr(), counts.data_ptr(), B, m, K, idx0.data_ptr(), row_w.data_ptr(),
                                  tv.data_ptr(), tl.data_ptr(), nt.data_ptr(), st), "dedup_plan")
    want_valid = (counts.view(-1, qpt) > 1).any(1)
    assert 0 < int(nt) < B * tpb and int(nt) == int(want_valid.sum())
    assert torch.equal(tl[:int(nt)].long(), want_valid.nonzero()[:, 0]) and torch.equal(tv.bool(), want_valid)
    assert torch.equal(idx0, idx[:, :, 0])
    assert torch.equal(row_w.view(-1, qpt), (~want_valid)[:, None].float().expand(-1, qpt) * K)
    part = torch.full((B * ptpb, Cout, 2), float("nan"), device=dev)
    _lib.check(lib.pdr_gather_add_tiles(*tabs, idx.data_ptr(), counts.data_ptr(), None, None, None, None, B, m * K, K,
                                        Cout, None, ld, part.data_ptr(), relu_col0, 0, -1, tv.data_ptr(), ptpb, st),
               "gather_add_tiles")
    Yd = torch.empty(B * m, ld, device=dev)
    _lib.check(lib.pdr_gather_add(*tabs, idx0.data_ptr(), counts.data_ptr(), None, None, None, None, B, m, 1, Cout,
                                  Yd.data_ptr(), ld, None, relu_col0, 0, -1, st), "gather_add")
    _lib.check(lib.pdr_weighted_moments(Yd.data_ptr(), ld, B, m, Cout, relu_col0, row_w.data_ptr(), part.data_ptr(),
                                        ptpb, tpb, tv.data_ptr(), st), "weighted_moments")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(part).any())
    pv = part.view(B, ptpb, Cout, 2)[:, :tpb].reshape(B * tpb, Cout, 2)
    assert torch.equal(pv[want_valid], full[want_valid]) and bool((pv[~want_valid] == 0).all())
    a, b = full.view(B, tpb, Cout, 2).double().sum(1), part.view(B, ptpb, Cout, 2).double().sum(1)
    assert float(((a - b).abs() / (a.abs() + 1)).max()) < 1e-4
    # pooled rows of the skipped tiles' queries: the activated value row; the others untouched
    D = 32
    V = torch.randn(B * m, D, device=dev, generator=g)
    vs, vt = torch.rand(B, D, device=dev, generator=g) + 0.5, torch.randn(B, D, device=dev, generator=g)
    out = torch.full((B * m, D), 7.0, device=dev)
    _lib.check(lib.pdr_patch_rows(V.data_ptr(), D, vs.data_ptr(), vt.data_ptr(), 1, row_w.data_ptr(), B, m, D,
                                  out.data_ptr(), D, None, st), "patch_rows")
    act = torch.relu(torch.addcmul(vt.repeat_interleave(m, 0), V, vs.repeat_interleave(m, 0)))
    want = torch.where((row_w > 0)[:, None], act, torch.full_like(out, 7.0))
    assert ((out - want).abs() <= 1e-6 * (want.abs() + 1)).all()
    # queries sorted per cloud, real neighbourhoods first, stable; inverse and row numbers; patched rows through a map
    perm = torch.empty(B, m, dtype=torch.int32, device=dev)
    inv, rows = torch.empty_like(perm), torch.empty_like(perm)
    _lib.check(lib.pdr_dedup_sort(counts.data_ptr(), B, m, perm.data_ptr(), inv.data_ptr(), rows.data_ptr(), st),
               "dedup_sort")
    real = counts > 1
    for b in range(B):
        wantp = torch.cat([real[b].nonzero()[:, 0], (~real[b]).nonzero()[:, 0]]).int()
        assert torch.equal(perm[b], wantp) and torch.equal(inv[b][perm[b].long()], torch.arange(m, device=dev).int())
    assert torch.equal(rows, perm + (torch.arange(B, device=dev) * m).int()[:, None])
    out2 = torch.full((B * m, D), 7.0, device=dev)
    _lib.check(lib.pdr_patch_rows(V.data_ptr(), D, vs.data_ptr(), vt.data_ptr(), 1, row_w.data_ptr(), B, m, D,
                                  out2.data_ptr(), D, rows.data_ptr(), st), "patch_rows")
    want2 = torch.full_like(out2, 7.0)
    sel = row_w > 0
    want2[rows.view(-1)[sel].long()] = act[sel]
    assert ((out2 - want2).abs() <= 1e-6 * (want2.abs() + 1)).all()


@pytest.mark.parametrize("shape", [(4096, 32, 32, 0), (4096, 64, 128, 0), (2048, 128, 128, 32), (4096, 41, 32, 32)])
def test_layer_tile_subset_matches_the_whole_layer_on_its_tiles(cuda, shape):
    """pdr_layer_in_t.tile_list: the listed 128-row tiles get bit-identical rows of Y and of the moments (written to
    row b * partial_tpb + t), every other row of both buffers is left untouched; plain and ball-gathered sources."""
    rpb, Cin, Cout, gath = shape
    lib, dev = _lib.load(), cuda
    B = 5
    g = torch.Generator(device=dev).manual_seed(rpb + Cin)
    P, ldx, ldw = B * rpb, (Cin + 3) // 4 * 4, (Cout + 3) // 4 * 4
    Wt = torch.randn(Cin, ldw, device=dev, generator=g) * 0.1
    bias = torch.randn(Cout, device=dev, generator=g)
    scale, shift = torch.rand(B, Cin, device=dev, generator=g) + 0.5, torch.randn(B, Cin, device=dev, generator=g)
    li = _lib.LayerIn()
    li.n_seg = 1
    keep = []
    if gath:
        K, n_src = gath, 300
        U = torch.randn(B * n_src + 1, ldx, device=dev, generator=g)
        U[-1].zero_()
        V2 = torch.randn(P // K, 2 * ldx, device=dev, generator=g)
        idx = torch.randint(0, n_src, (P,), device=dev, dtype=torch.int32, generator=g)
        cnt = torch.randint(0, 3, (P // K,), device=dev, dtype=torch.int32, generator=g)
        li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = U.data_ptr(), Cin, ldx, 1
        li.seg[0].gV, li.seg[0].gV0 = V2.data_ptr(), V2.data_ptr() + 4 * ldx
        li.seg[0].g_ldv, li.seg[0].g_nsrc, li.seg[0].g_zrow = 2 * ldx, n_src, B * n_src
        li.gidx, li.gcnt, li.gK = idx.data_ptr(), cnt.data_ptr(), K
        keep += [U, V2, idx, cnt]
    else:
        X = torch.randn(P, ldx, device=dev, generator=g)
        li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = X.data_ptr(), Cin, ldx, 1
        keep.append(X)
    li.scale, li.shift, li.pre_relu, li.post_relu, li.rows_per_batch = scale.data_ptr(), shift.data_ptr(), 0, 1, rpb
    assert lib.pdr_fused_layer_tile_rows(rpb, Cout) == 128
    tpb = rpb // 128
    st = torch.cuda.current_stream().cuda_stream

    def run(y, part):
        _lib.check(lib.pdr_fused_layer(ctypes.byref(li), P, Cin, Wt.data_ptr(), ldw, bias.data_ptr(), Cout,
                                       y.data_ptr(), ldw, part.data_ptr(), Cout // 2, st), "fused_layer")
        torch.cuda.synchronize()
    Y0, p0 = torch.empty(P, ldw, device=dev), torch.empty(B * tpb, Cout, 2, device=dev)
    run(Y0, p0)
    ntile = B * tpb
    pick = (torch.rand(ntile, device=dev, generator=g) < 0.3)
    pick[0], pick[-1] = True, False
    tl = torch.full((ntile,), -1, dtype=torch.int32, device=dev)
    sel = pick.nonzero()[:, 0].int()
    tl[:len(sel)] = sel
    nt = torch.tensor([len(sel)], dtype=torch.int32, device=dev)
    ptpb = tpb + 3
    li.tile_list, li.n_tiles, li.partial_tpb = tl.data_ptr(), nt.data_ptr(), ptpb
    Y1, p1 = torch.full((P, ldw), -5.0, device=dev), torch.full((B * ptpb, Cout, 2), -5.0, device=dev)
    run(Y1, p1)
    rows = pick.repeat_interleave(128)
    assert torch.equal(Y1[rows][:, :Cout], Y0[rows][:, :Cout]) and bool((Y1[~rows] == -5.0).all())
    pv = p1.view(B, ptpb, Cout, 2)
    assert torch.equal(pv[:, :tpb].reshape(ntile, Cout, 2)[pick], p0[pick])
    assert bool((pv[:, :tpb].reshape(ntile, Cout, 2)[~pick] == -5.0).all()) and bool((pv[:, tpb:] == -5.0).all())
    # an empty list is a launch that does nothing
    nt.zero_()
    Y2 = torch.full((P, ldw), -5.0, device=dev)
    run(Y2, p1)
    assert bool((Y2 == -5.0).all())


@pytest.mark.parametrize("cloud", ["noise", "mixed", "surface"])
def test_one_point_neighbourhoods_evaluated_once_match_the_whole_evaluation(cuda, cloud, monkeypatch):
    """DEDUP on vs off on the DDPM configuration: eps of a cached step agrees to fp32 summation order on a noise-like
    x_t (most tiles skipped), on x_t = q_sample(torus, t = 75) -- a MIXED plan: 30-90 % of the tiles walked, every block
    with walked and skipped tiles side by side -- and on the finished surface (t = 0: nearly every tile walked, the
    per-query chain idle); all three agree with the layer-by-layer network."""
    from tests import parity
    from point_diffusion_refinement_amd.pointnet2.configs import DIFFUSION_CONFIG, q_sample, synthetic_surface_batch
    torch.manual_seed(0)
    net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)
    fused = FN.FusedCloudConditionNet(net)
    x, cond, label = synthetic_batch(2, seed=5, device=cuda)
    ts = torch.tensor([300.0, 40.0], device=cuda)
    if cloud != "noise":
        t = 75 if cloud == "mixed" else 0
        x0, cond, label = synthetic_surface_batch(2, seed=5, device=cuda)
        # (_cached_eps evaluates the step on 0.9 x)
        x = q_sample(x0, t, util.calc_diffusion_hyperparams(**DIFFUSION_CONFIG), seed=5) / 0.9
        ts = torch.full((2,), float(t + 1), device=cuda)
    plans = []
    init = FN.Dedup.__init__

    def rec(self, *a, **k):
        init(self, *a, **k)
        plans.append(self)
    monkeypatch.setattr(FN.Dedup, "__init__", rec)
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(FN, "DEDUP", on)
        outs[on], ref = _cached_eps(net, fused, x, cond, ts, label)
    torch.cuda.synchronize()
    walked = sum(int(p.n_tiles) for p in plans) / float(sum(p.B * p.tpb for p in plans))
    assert plans and {"noise": walked < 0.3, "mixed": 0.3 < walked < 0.9, "surface": walked > 0.9}[cloud], walked
    parity.check("dedup:%s:on_vs_off" % cloud, "hip", outs[True], outs[False], 2e-5)
    err = ((outs[True] - ref).abs() / (ref.abs() + 1.0))
    assert err.max() < 1e-2 and (err < 1e-3).float().mean() > 0.99, (err.max(), (err < 1e-3).float().mean())


def _surface_sampler_inputs(cuda, B):
    from point_diffusion_refinement_amd.pointnet2.configs import DIFFUSION_CONFIG, synthetic_surface_batch
    torch.manual_seed(0)
    net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)
    fused = FN.FusedCloudConditionNet(net)
    x0, cond, label = synthetic_surface_batch(B, seed=3, device=cuda)
    return net, fused, util.calc_diffusion_hyperparams(**DIFFUSION_CONFIG), x0, cond, label


def test_adaptive_sampler_picks_the_form_of_each_step_from_the_probe(cuda):
    """GraphedReverseSampler(neighbourhoods='adaptive') on the DDPM configuration: restarted on a finished surface
    (use_a_precomputed_XT, step = 6: full balls) it replays the step with every neighbourhood evaluated, from noise the
    deduplicated one; the published walked share matches the plans'; and whichever form a step takes, the samples equal
    those of the two fixed forms to fp32 summation order (same CPU noise stream): after two steps to 2e-6 everywhere;
    after six a 1e-8 difference may have met a near-tie of a sampling / ball decision in one form and not in the other
    (it does with the round-5 tiny-layer kernels on this seed: tools/lab/forms_check.py -- 245 of 12288 coordinates
    above 1e-4, max 6.5e-4, while the whole form against itself under PDR_DEEP_CHUNKS=0 stays at 1.4e-7), so the six-step
    clouds are held to the bound a flipped cloud is held to everywhere in this suite."""
    net, fused, dh, x0, cond, label = _surface_sampler_inputs(cuda, 2)
    for steps in (2, 6):
        outs, counts = {}, {}
        for mode in ("adaptive", "once", "whole"):
            s = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=True, neighbourhoods=mode)
            torch.manual_seed(7)
            outs[mode] = s.sample((2, 2048, 3), cond, label, use_a_precomputed_XT=True, step=steps, XT=x0)
            counts[mode] = dict(s.mode_counts)
            if mode == "adaptive" and steps == 6:
                assert s.walked_share is not None and s.walked_share > 0.8, s.walked_share
        assert counts["once"]["whole"] == 0 and counts["whole"]["once"] == 0, counts
        if steps == 6:
            assert counts["adaptive"]["whole"] >= 4, counts
        for mode in ("once", "whole"):
            e = (outs["adaptive"] - outs[mode]).abs() / (outs[mode].abs() + 1.0)
            if steps == 2:
                assert float(e.max()) < 2e-6, (mode, float(e.max()))
            else:
                assert float(e.max()) < 1e-2 and float((e < 2e-4).float().mean()) > 0.95, (mode, float(e.max()))
    # from noise: the deduplicated form, chosen from the first step's probe
    s = GraphedReverseSampler(fused, util.calc_diffusion_hyperparams(5, 1e-4, 0.02), noise='cpu', use_graph=True)
    torch.manual_seed(7)
    out = s.sample((2, 2048, 3), cond, label)
    assert s.mode_counts["whole"] == 0 and s.mode_counts["once"] == 4 and s.walked_share < 0.3, (s.mode_counts, s.walked_share)
    assert bool(torch.isfinite(out).all())


@pytest.mark.timeout(600)
def test_captured_steps_replayed_on_changing_inputs_match_eager_whole_evaluations(cuda):
    """Soak: ONE sampler, its two captured steps, 200 replays; before every replay x_t is overwritten
    with the next point of a trajectory's marginal (q_sample of a torus at t = 199 ... 0: noise -> mixed -> surface, so
    the tile lists, the per-query chains and the adaptive switch all change under the same graphs) and the step counter
    set to t; after every 20th replay eps-equivalent state -- the updated x -- is compared with an EAGER step of a
    sampler that evaluates every neighbourhood (no graph, no tile subset), from the same x_t, same noise."""
    from point_diffusion_refinement_amd.pointnet2.configs import q_sample
    net, fused, dh, x0, cond, label = _surface_sampler_inputs(cuda, 2)
    s = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=True)
    import copy
    # (its own copy of the module: a network's retained condition features belong to one sampler at a time)
    ref = GraphedReverseSampler(FN.FusedCloudConditionNet(copy.deepcopy(net)), dh, noise='cpu', use_graph=False,
                                neighbourhoods='whole')
    torch.manual_seed(1)
    s.begin((2, 2048, 3), cond, label, x_T=q_sample(x0, 200, dh, seed=3), start_step=200)
    ref.begin((2, 2048, 3), cond, label, x_T=q_sample(x0, 200, dh, seed=3), start_step=200)
    worst, modes = 0.0, []
    for t in range(199, -1, -1):
        xt = q_sample(x0, t, dh, seed=3)
        for smp in (s,) + ((ref,) if t % 20 == 0 else ()):
            smp._x.copy_(xt)
            smp._t.fill_(t)
            smp._ts.fill_(float(t))
            smp.remaining = t + 1
        torch.manual_seed(1000 + t)
        s.advance(1)
        modes.append(s._mode)
        if t % 20 == 0:
            torch.manual_seed(1000 + t)
            ref.advance(1)
            torch.cuda.synchronize()
            worst = max(worst, _rel(s._x, ref._x))
            assert _rel(s._x, ref._x) < 5e-5, (t, modes[-1], _rel(s._x, ref._x))
    assert "once" in modes and "whole" in modes and modes[0] == "once" and modes[-1] == "whole", (modes[0], modes[-1])
    assert set(s._graphs) == {"once", "whole"}


# ---- round 5: the launches of the deduplicated step, fused ------------------------------------------------------------
@pytest.mark.parametrize("B,m,K", [(3, 1024, 32), (5, 256, 8), (2, 2048, 16), (33, 64, 32), (2, 16, 32)])
def test_dedup_prepare_equals_sort_gathers_and_plan(cuda, B, m, K):
    """pdr_dedup_prepare = pdr_dedup_sort + the row gathers of idx / counts / xyz + pdr_dedup_plan on the sorted arrays,
    bit for bit, in one launch; nvalid = [valid tiles | first weighted query] per cloud; the probe counters accumulate
    (pdr_dedup_probe adds the same two numbers without a plan)."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    n_src = 500
    idx, counts = _ball_like_neighbourhoods(B, m, K, n_src, dev, 3 * m + K, 0.2, 3)
    if B > 2:
        counts[1].clamp_(max=1)                      # a cloud without any real neighbourhood ...
        counts[2].fill_(5)                           # ... and one with nothing else
    xyz = torch.randn(B, m, 3, device=dev)
    qpt, tpb = 128 // K, m * K // 128
    i32 = dict(dtype=torch.int32, device=dev)
    # round-4 pipeline
    perm, inv, rows = (torch.empty(B, m, **i32) for _ in range(3))
    _lib.check(lib.pdr_dedup_sort(counts.data_ptr(), B, m, perm.data_ptr(), inv.data_ptr(), rows.data_ptr(), st), "sort")
    pl = perm.long()
    idx_s = torch.gather(idx, 1, pl[:, :, None].expand(-1, -1, K)).contiguous()
    cnt_s = torch.gather(counts, 1, pl).contiguous()
    xyz_s = torch.gather(xyz, 1, pl[:, :, None].expand(-1, -1, 3)).contiguous()
    idx0, row_w = torch.empty(B, m, **i32), torch.empty(B * m, device=dev)
    tv, tl, nt = torch.empty(B * tpb, dtype=torch.uint8, device=dev), torch.full((B * tpb,), -1, **i32), torch.empty(1, **i32)
    _lib.check(lib.pdr_dedup_plan(idx_s.data_ptr(), cnt_s.data_ptr(), B, m, K, idx0.data_ptr(), row_w.data_ptr(),
                                  tv.data_ptr(), tl.data_ptr(), nt.data_ptr(), st), "plan")
    # one launch
    perm2, inv2, rows2, idx02 = (torch.full((B, m), -7, **i32) for _ in range(4))
    idx_s2, cnt_s2, xyz_s2 = torch.full_like(idx, -7), torch.full_like(counts, -7), torch.full_like(xyz, -7.0)
    row_w2 = torch.full((B * m,), -7.0, device=dev)
    tv2, tl2, nt2 = torch.full((B * tpb,), 9, dtype=torch.uint8, device=dev), torch.full((B * tpb,), -1, **i32), torch.zeros(1, **i32)
    nvalid = torch.full((2, B), -7, **i32)
    acc = torch.tensor([5, 11], **i32)
    _lib.check(lib.pdr_dedup_prepare(idx.data_ptr(), counts.data_ptr(), xyz.data_ptr(), B, m, K, perm2.data_ptr(),
                                     inv2.data_ptr(), rows2.data_ptr(), idx_s2.data_ptr(), cnt_s2.data_ptr(),
                                     xyz_s2.data_ptr(), idx02.data_ptr(), row_w2.data_ptr(), tv2.data_ptr(),
                                     tl2.data_ptr(), nt2.data_ptr(), nvalid.data_ptr(), acc.data_ptr(), st), "prepare")
    torch.cuda.synchronize()
    n = int(nt)
    for name, a, b in (("perm", perm, perm2), ("inv", inv, inv2), ("rows", rows, rows2), ("idx", idx_s, idx_s2),
                       ("counts", cnt_s, cnt_s2), ("xyz", xyz_s, xyz_s2), ("idx0", idx0, idx02), ("row_w", row_w, row_w2),
                       ("tile_valid", tv, tv2), ("n_tiles", nt, nt2), ("tile_list", tl[:n], tl2[:n])):
        assert torch.equal(a, b), name
    assert bool((tl2[n:] == -1).all())
    nv = tv.view(B, tpb).sum(1).int()
    assert torch.equal(nvalid[0], nv) and torch.equal(nvalid[1], nv * qpt)
    # sorted queries: a cloud's valid tiles are its first ones
    assert torch.equal(tv.view(B, tpb).bool(), torch.arange(tpb, device=dev)[None, :] < nv[:, None])
    assert acc.tolist() == [5 + n, 11 + B * tpb]
    _lib.check(lib.pdr_dedup_probe(counts.data_ptr(), B, m, K, acc.data_ptr(), st), "probe")
    assert acc.tolist() == [5 + 2 * n, 11 + 2 * B * tpb]


def test_gather_add_tiles_twin_equals_the_three_launches(cuda):
    """pdr_gather_add_tiles_twin: the main tiles as pdr_gather_add_tiles (same bits), the per-query rows as the K = 1
    pdr_gather_add on the first neighbours (same bits), their weighted moments as pdr_weighted_moments (fp32 summation
    order), in one launch -- on sorted queries, with and without empty balls and a written column window."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    B, m, K, Cout, n_src, relu_col0 = 3, 1024, 32, 96, 700, 64
    ld = Cout
    g = torch.Generator(device=dev).manual_seed(3)
    U = torch.randn(B * n_src + 1, ld, device=dev, generator=g)
    V2 = torch.randn(B * m, 2 * ld, device=dev, generator=g)
    idx_u, counts_u = _ball_like_neighbourhoods(B, m, K, n_src, dev, 77, 0.15, 3)
    fm = FN.SortedQueries(idx_u, counts_u, torch.randn(B, m, 3, device=dev))
    dd, idx, counts = fm.plan, fm.idx, fm.counts
    assert dd is not None and 0 < int(dd.n_tiles) < B * dd.tpb
    tpb, ptpb = dd.tpb, dd.ptpb
    for has_counts, (ycol0, ycols) in ((True, (0, -1)), (False, (32, 32))):
        cptr = counts.data_ptr() if has_counts else None
        tabs = (U.data_ptr(), ld, n_src, V2.data_ptr(), V2.data_ptr() + 4 * ld if has_counts else None, 2 * ld)
        ncol = Cout if ycols < 0 else ycols
        Ya, Yb = (torch.full((B * m * K, ncol), -3.0, device=dev) for _ in range(2))
        pa, pb = (torch.full((B * ptpb, Cout, 2), float("nan"), device=dev) for _ in range(2))
        _lib.check(lib.pdr_gather_add_tiles(*tabs, idx.data_ptr(), cptr, None, None, None, None, B, m * K, K, Cout,
                                            Ya.data_ptr(), ncol, pa.data_ptr(), relu_col0, ycol0, ycols,
                                            dd.tile_valid.data_ptr(), ptpb, st), "tiles")
        Yda = torch.empty(B * m, ld, device=dev)
        _lib.check(lib.pdr_gather_add(*tabs, dd.idx0.data_ptr(), cptr, None, None, None, None, B, m, 1, Cout,
                                      Yda.data_ptr(), ld, None, relu_col0, 0, -1, st), "gather_add")
        _lib.check(lib.pdr_weighted_moments(Yda.data_ptr(), ld, B, m, Cout, relu_col0, dd.row_w.data_ptr(), pa.data_ptr(),
                                            ptpb, tpb, dd.tile_valid.data_ptr(), st), "weighted_moments")
        Ydb = torch.full((B * m, ld), -3.0, device=dev)
        _lib.check(lib.pdr_gather_add_tiles_twin(*tabs, idx.data_ptr(), cptr, B, m * K, K, Cout, Yb.data_ptr(), ncol,
                                                 pb.data_ptr(), relu_col0, ycol0, ycols, dd.tile_valid.data_ptr(), ptpb,
                                                 dd.idx0.data_ptr(), Ydb.data_ptr(), ld, dd.wrow0.data_ptr(), float(K), st),
                   "twin")
        torch.cuda.synchronize()
        assert torch.equal(Ya, Yb) and torch.equal(Yda, Ydb)
        va, vb = pa.view(B, ptpb, Cout, 2), pb.view(B, ptpb, Cout, 2)
        valid = dd.tile_valid.view(B, tpb).bool()
        assert torch.equal(va[:, :tpb][valid], vb[:, :tpb][valid])
        assert bool(torch.isnan(vb[:, :tpb][~valid]).all())             # skipped tiles: not written (nobody zeroes them)
        ta, tb = va[:, tpb:].double(), vb[:, tpb:].double()
        assert not bool(torch.isnan(tb).any())
        # (two fp32 summation orders of up to 128 weighted rows; judged against the size of the sums' terms: the second
        # moment bounds both -- |sum w f| <= sum w f^2 + sum w)
        scale = ta[..., 1:2].abs() + 32.0 * 128
        assert float(((ta - tb).abs() / scale).max()) < 2e-6


@pytest.mark.parametrize("rpb,Cin,Cout", [(2048, 32, 32), (1024, 64, 128), (256, 128, 128), (64, 256, 128), (16, 512, 512),
                                          (1024, 41, 64)])
def test_layer_weighted_statistics(cuda, rpb, Cin, Cout):
    """pdr_layer_in_t.wrow0 / wmul: Y as without them (same bits); partial rows = wmul x the moments of the rows
    r >= wrow0[b] -- wave-specialised tiles (128 / 64 rows) and the uniform kernel (32-row tiles), thresholds at 0, inside a
    tile, on a tile boundary and past the end."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    B = 4
    g = torch.Generator(device=dev).manual_seed(rpb + Cout)
    P, ldx, ldw = B * rpb, (Cin + 3) // 4 * 4, (Cout + 3) // 4 * 4
    X = torch.randn(P, ldx, device=dev, generator=g)
    Wt = torch.randn(Cin, ldw, device=dev, generator=g) * 0.1
    bias = torch.randn(Cout, device=dev, generator=g)
    scale, shift = torch.rand(B, Cin, device=dev, generator=g) + 0.5, torch.randn(B, Cin, device=dev, generator=g)
    li = _lib.LayerIn()
    li.n_seg = 1
    li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = X.data_ptr(), Cin, ldx, 1
    li.scale, li.shift, li.pre_relu, li.post_relu, li.rows_per_batch = scale.data_ptr(), shift.data_ptr(), 0, 1, rpb
    tm = lib.pdr_fused_layer_tile_rows(rpb, Cout)
    tpb = (rpb + tm - 1) // tm
    relu_col0 = Cout // 2
    Y0 = torch.empty(P, ldw, device=dev)
    _lib.check(lib.pdr_fused_layer(ctypes.byref(li), P, Cin, Wt.data_ptr(), ldw, bias.data_ptr(), Cout, Y0.data_ptr(),
                                   ldw, None, relu_col0, st), "plain")
    thr = torch.tensor([0, min(rpb, 5), min(rpb, tm) if tpb > 1 else rpb // 2, rpb + 3], dtype=torch.int32, device=dev)
    ptpb, off = tpb + 7, 5                                   # rows of another launch in front, as in a deduplicated layer
    part = torch.full((B * ptpb, Cout, 2), float("nan"), device=dev)
    li.wrow0, li.wmul, li.partial_tpb = thr.data_ptr(), 32.0, ptpb
    Y1 = torch.empty(P, ldw, device=dev)
    _lib.check(lib.pdr_fused_layer(ctypes.byref(li), P, Cin, Wt.data_ptr(), ldw, bias.data_ptr(), Cout, Y1.data_ptr(),
                                   ldw, part.data_ptr() + 4 * off * Cout * 2, relu_col0, st), "weighted")
    torch.cuda.synchronize()
    assert torch.equal(Y0[:, :Cout], Y1[:, :Cout])
    f = Y0[:, :Cout].double().view(B, rpb, Cout).clone()
    f[:, :, relu_col0:].clamp_(min=0)
    w = (torch.arange(rpb, device=dev)[None, :] >= thr[:, None].long()).double()[:, :, None] * 32.0
    pv = part.view(B, ptpb, Cout, 2)
    assert bool(torch.isnan(pv[:, :off]).all()) and bool(torch.isnan(pv[:, off + tpb:]).all())
    for t in range(tpb):
        rows = slice(t * tm, min((t + 1) * tm, rpb))
        want = torch.stack([(w[:, rows] * f[:, rows]).sum(1), (w[:, rows] * f[:, rows] ** 2).sum(1)], -1)
        got = pv[:, off + t].double()
        assert float(((got - want).abs() / (want.abs() + 1.0)).max()) < 2e-5, t


def test_gn_fold_skips_the_invalid_tile_range(cuda):
    """pdr_gn_fold(nvalid, tpb_main): rows [nvalid[b], tpb_main) of batch element b are not read -- NaN there, same
    scale / shift (bits) as the fold over the same rows with zeros in their place; both partial sources, both the
    small and the 16-row form."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(9)
    for B, tpb_main, extra, C0, C1, G in ((3, 40, 3, 64, 0, 32), (2, 512, 16, 32, 0, 32), (3, 24, 2, 32, 96, 32)):
        tpb = tpb_main + extra
        C = C0 + C1
        nv = torch.randint(0, tpb_main + 1, (B,), generator=g, device=dev).int()
        nv[0] = 0
        nv[-1] = tpb_main
        skip = (torch.arange(tpb, device=dev)[None, :] >= nv[:, None]) & (torch.arange(tpb, device=dev)[None, :] < tpb_main)
        parts = []
        for Cp in (C0, C1):
            if Cp:
                p = torch.rand(B, tpb, Cp, 2, device=dev, generator=g) + 0.5
                parts.append(p)
        gamma, beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g)
        outs = []
        for fill, use_nv in ((0.0, False), (float("nan"), True)):
            ps = []
            for p in parts:
                q = p.clone()
                q[skip] = fill
                ps.append(q.view(B * tpb, -1, 2).contiguous())
            scale, shift = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
            second = (ps[1].data_ptr(), C1, tpb, C1, 4.0) if C1 else (None, 0, 0, 0, 1.0)
            nva = (nv.data_ptr(), tpb_main) if use_nv else (None, 0)
            _lib.check(lib.pdr_gn_fold(ps[0].data_ptr(), C0, tpb, C0, 1.0, *second, B, C, G, 1000.0, 1e-5,
                                       gamma.data_ptr(), beta.data_ptr(), scale.data_ptr(), shift.data_ptr(), *nva,
                                       *(nva if C1 else (None, 0)), st), "gn_fold")
            outs.append((scale, shift))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert bool(torch.isfinite(outs[1][0]).all())


# every route from tile moments to a folded GroupNorm: (tiles per batch element of the parts, widths of the parts,
# Cn, G, options, entry points).  B = 3; C = 79 > Cn leaves pass-through channels behind the normalised range.
_FOLD_ROUTES = {
    "small_u4": ((2,), (79,), 64, 32, {}, "fold"),
    "small_u16": ((130,), (79,), 64, 32, {}, "fold"),            # > 128 tiles: 16 rows in flight per thread
    "two_parts": ((5, 3), (48, 31), 64, 32, {}, "fold"),         # the normalised range spans both sources
    "wide_cpg48": ((5,), (111,), 96, 2, {}, "fold"),             # 48 channels per group: no 32-channel window
    "wide_option": ((5,), (79,), 64, 32, {"gn_fold_small": 0}, "fold"),
    "reduce_finalize": ((5,), (79,), 64, 32, {}, "reduce"),
}


@pytest.mark.parametrize("route", sorted(_FOLD_ROUTES))
def test_gn_fold_routes_agree_with_a_float64_fold(cuda, route):
    """Every route from per-tile moments to (scale, shift) -- pdr_gn_fold in its small form with 4 and with 16 rows in
    flight, with two sources, in its wide form (chosen by the group width and by option gn_fold_small = 0), and
    pdr_gn_reduce + pdr_gn_finalize -- against a float64 fold of the same synthetic `partial` rows.

    Tolerance, from the arithmetic: the routes differ from the reference only in the order of their double sums over
    float inputs (about 2^-53 per term), which can flip one float rounding and no more.  scale = float(rstd) * gamma is
    one rounding of rstd and one float product: at most 2 float ulp.  shift = fma(-scale, float(mean), beta) adds the
    rounding of mean and of the fma: |d shift| <= 2^-22 (|scale mean| + |beta|).  Channels >= Cn are exactly (1, 0)."""
    from tests.layer_cases import options
    tpbs, widths, Cn, G, opts, entry = _FOLD_ROUTES[route]
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    B, C, eps = 3, sum(widths), 1e-5
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, route)))
    parts, mults = [], (1.0, 4.0)
    for tpb, Cp in zip(tpbs, widths):   # (sum x, sum x^2) of 128 values per tile and channel
        parts.append(torch.stack([torch.randn(B * tpb, Cp, device=dev, generator=g) * 8.0,
                                  (torch.rand(B * tpb, Cp, device=dev, generator=g) + 0.5) * 128.0], -1).contiguous())
    n = float(tpbs[0] * 128)
    gamma, beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g)
    scale, shift = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
    with options(opts):
        if entry == "fold":
            second = (None, 0, 0, 0, 1.0)
            if len(parts) > 1:
                second = (parts[1].data_ptr(), widths[1], tpbs[1], widths[1], mults[1])
            _lib.check(lib.pdr_gn_fold(parts[0].data_ptr(), widths[0], tpbs[0], widths[0], mults[0], *second, B, Cn, G, n,
                                       eps, gamma.data_ptr(), beta.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, 0,
                                       None, 0, st), "gn_fold")
        else:
            stats = torch.empty(B, C, 2, device=dev, dtype=torch.float64)
            _lib.check(lib.pdr_gn_reduce(parts[0].data_ptr(), C, B, tpbs[0], C, mults[0], stats.data_ptr(), C, 0, st),
                       "gn_reduce")
            _lib.check(lib.pdr_gn_finalize(stats.data_ptr(), B, C, Cn, G, n, eps, gamma.data_ptr(), beta.data_ptr(),
                                           scale.data_ptr(), shift.data_ptr(), st), "gn_finalize")
    torch.cuda.synchronize()
    got_sc, got_sh = scale.cpu().numpy(), shift.cpu().numpy()

    mom = np.concatenate([p.cpu().numpy().astype(np.float64).reshape(B, tpb, Cp, 2).sum(1) * m
                          for p, tpb, Cp, m in zip(parts, tpbs, widths, mults)], 1)          # (B, C, 2)
    cpg = Cn // G
    grp = mom[:, :Cn].reshape(B, G, cpg, 2).sum(2) / (n * cpg)                              # (B, G, 2)
    mean = np.repeat(grp[..., 0], cpg, 1)
    var = np.repeat(np.maximum(grp[..., 1] - grp[..., 0] ** 2, 0.0), cpg, 1)
    ga, be = gamma.cpu().numpy().astype(np.float64)[:Cn], beta.cpu().numpy().astype(np.float64)[:Cn]
    want_sc = ga / np.sqrt(var + float(np.float32(eps)))
    want_sh = be - want_sc * mean
    ulp = np.spacing(np.abs(want_sc).astype(np.float32)).astype(np.float64)
    err_sc = np.abs(got_sc[:, :Cn] - want_sc) / ulp
    err_sh = np.abs(got_sh[:, :Cn] - want_sh) / (2.0 ** -22 * (np.abs(want_sc * mean) + np.abs(be)))
    print("%s: scale error %.3f ulp (bound 2), shift error %.3f of its bound" % (route, err_sc.max(), err_sh.max()))
    assert err_sc.max() <= 2.0 and err_sh.max() <= 1.0
    assert np.all(got_sc[:, Cn:] == 1.0) and np.all(got_sh[:, Cn:] == 0.0)
    assert C > Cn and var.min() > 0.1   # pass-through channels exist; no group sits on the variance clamp


@pytest.mark.parametrize("D,K", [(32, 32), (64, 32), (128, 8)])
def test_pooled_launch_patches_the_skipped_queries(cuda, D, K):
    """pdr_layer_in_t.patch_values / patch_w on a pooled launch over a tile subset with a row map = the same launch
    without them followed by pdr_patch_rows: identical output rows."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    B, m, Cin = 3, 512, 64
    rpb = m * K
    P = B * rpb
    g = torch.Generator(device=dev).manual_seed(D + K)
    idx_u, counts_u = _ball_like_neighbourhoods(B, m, K, 300, dev, D, 0.2, 3)
    fm = FN.SortedQueries(idx_u, counts_u, torch.randn(B, m, 3, device=dev))
    dd, counts = fm.plan, fm.counts
    X = torch.randn(P, Cin, device=dev, generator=g)
    Wt = torch.randn(Cin, D, device=dev, generator=g) * 0.2
    bias = torch.randn(D, device=dev, generator=g)
    V = torch.randn(P, D, device=dev, generator=g)
    Vd = torch.randn(B * m, D, device=dev, generator=g)
    vs, vt = torch.rand(B, D, device=dev, generator=g) + 0.5, torch.randn(B, D, device=dev, generator=g)
    li = _lib.LayerIn()
    li.n_seg = 1
    li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = X.data_ptr(), Cin, Cin, 1
    li.rows_per_batch = rpb
    li.tile_list, li.n_tiles, li.out_rows = dd.tile_list.data_ptr(), dd.n_tiles.data_ptr(), fm.perm_rows.data_ptr()

    def pool(out):
        _lib.check(lib.pdr_fused_layer_pool(ctypes.byref(li), P, Cin, Wt.data_ptr(), D, bias.data_ptr(), D, V.data_ptr(),
                                            D, vs.data_ptr(), vt.data_ptr(), 1, counts.data_ptr(), K, out.data_ptr(), D,
                                            st), "pool")
    a = torch.full((B * m, D), -9.0, device=dev)
    pool(a)
    _lib.check(lib.pdr_patch_rows(Vd.data_ptr(), D, vs.data_ptr(), vt.data_ptr(), 1, dd.row_w.data_ptr(), B, m, D,
                                  a.data_ptr(), D, fm.perm_rows.data_ptr(), st), "patch_rows")
    b = torch.full((B * m, D), -9.0, device=dev)
    li.patch_values, li.patch_ld, li.patch_w = Vd.data_ptr(), D, dd.row_w.data_ptr()
    pool(b)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not bool((b == -9.0).any())


def test_embed_select_and_step_table(cuda):
    """The step-embedding table of a schedule holds, row by row, the bits the three-launch chain produces for that step;
    pdr_embed_select broadcasts the row of the device step counter (clamped) to the batch; a forward with the table
    equals a forward with the chain bit for bit."""
    net, fused = _pair(small_fused_config(), 31, cuda)
    T, B = 37, 3
    ts_all = torch.arange(T, dtype=torch.float32, device=cuda) * 1.5
    table = fused.build_step_table(ts_all)
    assert table is not None and table.shape[0] == T
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    t_dev = torch.zeros(1, dtype=torch.int64, device=cuda)
    for t in (0, 5, 36, 50, -2):
        t_dev.fill_(t)
        tc = min(max(t, 0), T - 1)
        assert fused._embed_linear_chain(ts_all[tc:tc + 1].expand(B))
        want = fused.bank.out["t"].clone()
        out = torch.full((B, table.shape[1]), -1.0, device=cuda)
        _lib.check(lib.pdr_embed_select(table.data_ptr(), table.shape[1], T, t_dev.data_ptr(), B, table.shape[1],
                                        out.data_ptr(), out.shape[1], st), "embed_select")
        assert torch.equal(out, want), t
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 256, 3, generator=g).to(cuda)
    cond = torch.cat([torch.rand(2, 384, 3, generator=g) * 2 - 1, torch.ones(2, 384, 1)], 2).to(cuda)
    label = torch.tensor([1, 7], device=cuda)
    t_dev.fill_(9)
    ts = ts_all[9:10].expand(2)
    with torch.no_grad():
        a = fused(x, cond, ts=ts, label=label, use_retained_condition_feature=True)
        a = fused(x * 0.9, cond, ts=ts, label=label, use_retained_condition_feature=True).clone()
        fused.step_table = (table, t_dev)
        b = fused(x * 0.9, cond, ts=ts, label=label, use_retained_condition_feature=True).clone()
        fused.step_table = None
    assert torch.equal(a, b)


# ---- round 6: a chain of per-point layers as ONE launch (pdr_point_chain) ------------------------------
# (the case builder, the float64 reference and the launch helper live in tests/chain_cases.py, which also walks the
# kernel's whole dispatch table: tests/test_chain_dispatch_plan.py, tests/test_chain_dispatch_gpu.py)
@pytest.mark.parametrize("B,n,seg_widths,widths,residual,relu_pre", [
    (32, 64, (256, 256, 3), (256, 256), True, False),      # the 64-point level's second MLP (fp4: 515 -> 256 -> 256)
    (32, 256, (128, 256, 3), (256, 256), True, False),     # the 256-point level's (fp3: 387 -> 256 -> 256)
    (2, 16, (64,), (128, 128, 128), False, False),         # three layers, no residual, 16 rows per cloud
    (3, 32, (32, 35), (80, 48), True, False),              # no multiple of 8 clouds, an odd segment, pass-through tails
    (8, 32, (96,), (64, 128), False, True),                # ReLU -> GroupNorm order (attention score nets), 32 rows
    (5, 64, (40, 3), (256,), False, False),                # one layer: no hand-off at all
])
def test_point_chain_matches_float64_layer_by_layer(cuda, B, n, seg_widths, widths, residual, relu_pre):
    """pdr_point_chain (one launch: column blocks of whole GroupNorm groups per workgroup, activated blocks exchanged
    inside the launch) against the float64 evaluation of the same chain layer by layer; three launches in a row give
    identical bytes and leave the cluster counters zero."""
    segs, layers, want = _chain_case(1000 + n + B, B, n, seg_widths, widths, residual, relu_pre, cuda)
    rc, got, plan = _launch_chain(segs, seg_widths, layers, B, n, residual, relu_pre, cuda)
    assert rc == _lib.PDR_OK and plan[0] >= 1 and plan[3] == B * plan[0], (rc, plan)
    assert bool(torch.isfinite(got).all())
    assert _rel(got.double().cpu(), want) < 5e-6, _rel(got.double().cpu(), want)


def test_point_chain_refuses_what_it_cannot_run(cuda):
    """Shapes outside the kernel: PDR_EUNSUPPORTED from the plan (the caller runs the layers one by one); argument
    errors: PDR_EINVAL."""
    segs, layers, _ = _chain_case(1, 2, 512, (64,), (64, 64), False, False, cuda)
    assert _launch_chain(segs, (64,), layers, 2, 512, False, False, cuda)[0] == _lib.PDR_EUNSUPPORTED      # rows
    segs, layers, _ = _chain_case(2, 2, 64, (64,), (96, 96), False, False, cuda)
    assert _launch_chain(segs, (64,), layers, 2, 64, False, False, cuda)[0] == _lib.PDR_OK                 # G = 2: 48 cols
    segs, layers, _ = _chain_case(3, 2, 64, (64,), (40, 40), False, False, cuda)
    layers[0]["cn"] = layers[1]["cn"] = 32
    assert _launch_chain(segs, (64,), layers, 2, 64, False, False, cuda)[0] == _lib.PDR_EUNSUPPORTED      # 40 columns
    lib = _lib.load()
    ch = _lib.PointChain()
    assert lib.pdr_point_chain(ctypes.byref(ch), 2, 64, None) == _lib.PDR_EINVAL


def test_point_chain_under_uneven_load_and_warm_caches(cuda):
    """The in-launch hand-off under the conditions the guide says hide a missing release / acquire: other kernels
    running on a second stream (uneven load: late workgroups, busy memory queues) and consumers whose caches are WARM
    with the previous launch's scratch (every launch reuses it).  200 launches with inputs changing every launch,
    every output compared with the float64 result of ITS input."""
    B, n, seg_widths, widths = 32, 64, (256, 256, 3), (256, 256)
    lib = _lib.load()
    segs, layers, want = _chain_case(77, B, n, seg_widths, widths, True, False, cuda)
    keep = [s.to(cuda) for s in segs]
    ch = _lib.PointChain()
    ch.n_layers, ch.n_seg, ch.residual = 2, 3, 1
    for i, (t, c) in enumerate(zip(keep, seg_widths)):
        ch.seg[i].ptr, ch.seg[i].C, ch.seg[i].ld = t.data_ptr(), c, t.shape[1]
    dvs = []
    for i, Ld in enumerate(layers):
        L = ch.layer[i]
        dv = {k: (v.to(cuda).contiguous() if torch.is_tensor(v) else v) for k, v in Ld.items()}
        dvs.append(dv)
        L.Wt, L.bias, L.ldw, L.Cin, L.Cout, L.main_cols = dv["W"].data_ptr(), dv["bias"].data_ptr(), dv["cout"], \
            dv["W"].shape[0], dv["cout"], dv["c"]
        L.gamma, L.beta, L.groups, L.Cn, L.eps, L.relu_post = dv["gamma"].data_ptr(), dv["beta"].data_ptr(), 32, dv["cn"], 1e-5, 1
        L.add, L.add_ld = dv["add"].data_ptr(), dv["add"].shape[1]
    plan = (ctypes.c_long * 4)()
    assert lib.pdr_point_chain_plan(ctypes.byref(ch), B, n, plan) == _lib.PDR_OK
    out = torch.empty((B * n, 256), device=cuda)
    scratch = torch.empty(int(plan[1]), device=cuda)
    sync = torch.zeros(int(plan[2]), dtype=torch.int32, device=cuda)
    ch.out, ch.ldo, ch.scratch, ch.sync = out.data_ptr(), 256, scratch.data_ptr(), sync.data_ptr()
    # the chain is affine in nothing useful, so the reference is recomputed per scale on the CPU for a few scales only
    scales = [1.0, -0.5, 2.0, 0.25]
    base = [s.clone() for s in keep]
    wants = []
    for sc in scales:
        sg = [(b.cpu() * sc) for b in base]
        x = torch.cat([s[:, :c] for s, c in zip(sg, seg_widths)], 1).double()
        h, res = x, None
        for i, Ld in enumerate(layers):
            y = h @ Ld["W"].double() + Ld["bias"].double()
            if i == 0:
                res, y = y[:, Ld["c"]:], y[:, :Ld["c"]]
            fn = y.view(B, n, -1).transpose(1, 2)
            z = torch.nn.functional.group_norm(fn, 32, Ld["gamma"].double(), Ld["beta"].double(), 1e-5).transpose(1, 2) \
                .reshape(B * n, -1).relu() + Ld["add"][:, :Ld["c"]].double().repeat_interleave(n, 0)
            h = z
        wants.append((h + res).float())
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=cuda)
    worst = 0.0
    for it in range(200):
        sc = scales[it % len(scales)]
        for k, b in zip(keep, base):
            torch.mul(b, sc, out=k)
        with torch.cuda.stream(side):
            for _ in range(2):
                big = (big @ big).clamp_(-1, 1)            # chip-filling kernels beside the chain launch
        _lib.check(lib.pdr_point_chain(ctypes.byref(ch), B, n, torch.cuda.current_stream().cuda_stream), "point_chain")
        got = out.clone()
        torch.cuda.synchronize()
        assert sync.tolist() == [0] * sync.numel(), it
        e = _rel(got.double().cpu(), wants[it % len(scales)].double())
        worst = max(worst, e)
        assert e < 2e-5, (it, e)          # (a stale block would be off by O(1); small inputs round at 5e-6)


@pytest.mark.parametrize("B", [2, 33])
def test_fp_block_second_mlp_as_one_launch_equals_the_layer_launches(cuda, monkeypatch, B):
    """The feature-propagation blocks of the 64- / 256-point levels evaluate their second MLP (conv -> GroupNorm -> ReLU ->
    + t embedding -> conv -> GroupNorm -> ReLU -> + condition embedding -> + residual conv) as ONE pdr_point_chain launch
    (fused_network.POINT_CHAINS); eps of the full DDPM network with and without it agree to fp32 summation order, and the
    chain really ran (two launches per cached forward: n = 64 and n = 256).  B = 2: clusters of 8 workgroups; B = 33:
    B G <= 256 leaves clusters of 4 with column blocks of 64 + 64 (four column tiles per wave), no multiple of 8 clouds."""
    torch.manual_seed(0)
    net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)
    fused = FN.FusedCloudConditionNet(net)
    x, cond, label = synthetic_batch(B, seed=5, device=cuda)
    ts = torch.tensor([300.0, 20.0], device=cuda).repeat((B + 1) // 2)[:B].contiguous()
    lib = _lib.load()
    calls = []
    real = lib.pdr_point_chain

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def pdr_point_chain(self, *a):
            calls.append(a[2])
            return real(*a)
    with torch.no_grad():
        fused(x, cond, ts=ts, label=label, use_retained_condition_feature=True)
        monkeypatch.setattr(_lib, "_lib", Spy())
        on = fused(x * 0.9, cond, ts=ts - 1, label=label, use_retained_condition_feature=True).clone()
        monkeypatch.setattr(_lib, "_lib", lib)
        monkeypatch.setattr(FN, "POINT_CHAINS", False)
        off = fused(x * 0.9, cond, ts=ts - 1, label=label, use_retained_condition_feature=True).clone()
    assert sorted(calls) == [64, 256], calls
    assert _rel(on, off) < 2e-6, _rel(on, off)


def test_graphed_samplers_without_a_step_table(cuda, monkeypatch):
    """when the network cannot build the step-embedding table (NATIVE_EMBED off, a t_dim or bank width outside
    pdr_embed_linear's contract) a sampler's native step must fall back to the per-step embedding chain -- round 5 handed
    the network a (None, counter) pair and crashed.  Both samplers, graph replay, against the same loops with the table."""
    from point_diffusion_refinement_amd.pointnet2.configs import DIFFUSION_CONFIG
    from point_diffusion_refinement_amd.pointnet2.reverse_sampler import GraphedFastSampler
    torch.manual_seed(0)
    net = PointNet2CloudCondition(ddpm_pointnet_config()).eval().to(cuda)
    fused = FN.FusedCloudConditionNet(net)
    x, cond, label = synthetic_batch(2, seed=9, device=cuda)
    dh = util.calc_diffusion_hyperparams(**DIFFUSION_CONFIG)

    def run(make):
        outs = []
        for native in (True, False):
            monkeypatch.setattr(FN, "NATIVE_EMBED", native)
            s = make()
            torch.manual_seed(3)
            s.begin((2, 2048, 3), cond, label, x_T=x, start_step=4)
            assert (s._table() is None) == (not native)
            outs.append(s.finish())
        return outs
    a, b = run(lambda: GraphedReverseSampler(fused, dh, noise='cpu', use_graph=True, neighbourhoods='once'))
    assert bool(torch.isfinite(b).all()) and _rel(b, a) < 1e-4, _rel(b, a)
    a, b = run(lambda: GraphedFastSampler(fused, dh, DIFFUSION_CONFIG, length=5, sampling_method='var',
                                          schedule='quadratic', kappa=0.5, noise='cpu', use_graph=True,
                                          neighbourhoods='once'))
    assert bool(torch.isfinite(b).all()) and _rel(b, a) < 1e-4, _rel(b, a)


def test_adaptive_sampler_is_reproducible_from_a_seed(cuda):
    """the per-step choice of the captured form reads the probe of ONE given step (a ring slot tagged with
    the step counter), not whatever the device has published last: two runs from one seed replay the same forms and
    give identical bytes, also when the switch flips on the way (a restart on a surface)."""
    net, fused, dh, x0, cond, label = _surface_sampler_inputs(cuda, 2)
    outs, forms = [], []
    for _ in range(2):
        s = GraphedReverseSampler(fused, dh, noise='cpu', use_graph=True, neighbourhoods='adaptive')
        torch.manual_seed(11)
        outs.append(s.sample((2, 2048, 3), cond, label, use_a_precomputed_XT=True, step=8, XT=x0))
        forms.append(dict(s.mode_counts))
    assert forms[0] == forms[1], forms
    assert torch.equal(outs[0], outs[1])


# ---- round 6: the first step of a batch and the refinement forward as graphs ---------------------------------------------
@pytest.mark.parametrize("mode,noise", [("once", "cpu"), ("adaptive", "device"), ("whole", "cpu")])
def test_first_step_as_a_graph_equals_the_eager_first_step(cuda, monkeypatch, mode, noise):
    """reverse_sampler.FIRST_STEP_GRAPH: from the second batch of a shape on, the uncached first step (condition branch +
    step) is a graph replay writing the retained features where the cached step's graphs read them.  Three batches with
    different conditions / labels / x_T, a few steps each: the same bytes as the sampler with the eager first step."""
    from point_diffusion_refinement_amd.pointnet2 import reverse_sampler as RS
    net, fused = _pair(small_fused_config(), 31, cuda)
    dh = util.calc_diffusion_hyperparams(12, 1e-4, 0.02)
    g = torch.Generator().manual_seed(5)
    batches = []
    for _ in range(3):
        cond = torch.cat([torch.rand(2, 256, 3, generator=g) * 2 - 1, torch.ones(2, 256, 1)], 2).to(cuda)
        batches.append((cond, torch.randint(0, 16, (2,), generator=g).to(cuda), torch.randn(2, 128, 3, generator=g).to(cuda)))
    outs = {}
    for first_graph in (True, False):
        monkeypatch.setattr(RS, "FIRST_STEP_GRAPH", first_graph)
        s = GraphedReverseSampler(fused, dh, noise=noise, use_graph=True, neighbourhoods=mode)
        res = []
        for i, (cond, label, xT) in enumerate(batches):
            torch.manual_seed(100 + i)
            s.begin((2, 128, 3), cond, label, x_T=xT)
            res.append(s._x.clone())                       # after the first step
            s.advance(4)
            res.append(s._x.clone())
        assert (s._first is not None) == first_graph
        outs[first_graph] = res
    for a, b in zip(outs[True], outs[False]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_graphed_refiner_equals_refine_completion(cuda):
    """generation.GraphedRefiner: the refinement forward + upsampling as one graph replay per batch == the eager
    refine_completion on every batch (the first is the eager warm-up itself)."""
    from point_diffusion_refinement_amd.pointnet2 import generation as G
    cfg = small_fused_config(include_t=False)
    cfg["point_upsample_factor"] = 4
    net, fused = _pair(cfg, 43, cuda)
    refiner = G.GraphedRefiner(fused, 0.001, 4)
    g = torch.Generator().manual_seed(9)
    for i in range(3):
        cond = torch.cat([torch.rand(2, 256, 3, generator=g) * 2 - 1, torch.ones(2, 256, 1)], 2).to(cuda)
        label = torch.randint(0, 16, (2,), generator=g).to(cuda)
        coarse = (torch.rand(2, 128, 3, generator=g) * 2 - 1).to(cuda)
        with torch.no_grad():
            got = refiner(coarse, cond, label)
            want = G.refine_completion(fused, coarse, cond, label, 0.001, 4)
        assert got.shape == (2, 4 * 128, 3) and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), (i, float((got - want).abs().max()))


# ---- round 6: row tiles walked from the last to the first ---------------------------------------------------------------
@pytest.mark.parametrize("B,rpb,Cin,Cout,form", [(16, 2048, 128, 128, "plain"), (8, 1024, 171, 128, "plain"),
                                                 (16, 4096, 32, 32, "plain"), (3, 1000, 64, 64, "plain"),
                                                 (16, 2048, 128, 128, "residual"), (8, 2048, 41, 32, "ball"),
                                                 (8, 2048, 105, 128, "knn")])
def test_layer_walked_backwards_writes_the_same_bytes(cuda, B, rpb, Cin, Cout, form):
    """pdr_layer_in_t.walk_reverse changes the ORDER IN TIME of a launch's row tiles, nothing else: outputs and per-tile
    statistics of the forward and the reversed walk are the same bytes -- whole groups of 8 clouds (the XCD-local tile
    order) and not, a ragged last tile, plain / residual / ball- and kNN-gathered sources."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(B + rpb + Cin)
    P, ldx, ldw = B * rpb, (Cin + 3) // 4 * 4, (Cout + 3) // 4 * 4
    X = torch.randn(P, ldx, device=dev, generator=g)
    R = torch.randn(P, ldx, device=dev, generator=g)
    Wt = torch.randn(Cin, ldw, device=dev, generator=g) * 0.1
    bias = torch.randn(Cout, device=dev, generator=g)
    scale = torch.rand(B, Cin, device=dev, generator=g) + 0.5
    shift = torch.randn(B, Cin, device=dev, generator=g)
    K, n_src = 8, 512
    U = torch.randn(B * n_src + 1, ldx, device=dev, generator=g)
    V2 = torch.randn(P // K, 2 * ldx, device=dev, generator=g)
    idx = torch.randint(0, n_src, (P,), device=dev, dtype=torch.int32, generator=g)
    cnt = torch.randint(1, K + 1, (P // K,), device=dev, dtype=torch.int32, generator=g)
    s1, s2 = torch.rand(P, device=dev, generator=g), torch.rand(P, device=dev, generator=g)
    r1, r2 = torch.randn(ldx + 4, device=dev, generator=g), torch.randn(ldx + 4, device=dev, generator=g)

    def run(reverse):
        li = _lib.LayerIn()
        li.n_seg = 1
        li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = X.data_ptr(), Cin, ldx, 1
        li.scale, li.shift, li.post_relu, li.rows_per_batch = scale.data_ptr(), shift.data_ptr(), 1, rpb
        if form == "residual":
            li.rseg.ptr, li.rseg.C, li.rseg.ld, li.rseg.row_div = R.data_ptr(), Cin, ldx, 1
        if form in ("ball", "knn"):
            li.seg[0].ptr = U.data_ptr()
            li.seg[0].gV, li.seg[0].gV0 = V2.data_ptr(), V2.data_ptr() + 4 * ldx
            li.seg[0].g_ldv, li.seg[0].g_nsrc, li.seg[0].g_zrow = 2 * ldx, n_src, B * n_src
            li.gidx, li.gcnt, li.gK = idx.data_ptr(), cnt.data_ptr(), K
            if form == "knn":
                li.gcnt, li.seg[0].gV0 = None, None
                li.gs1, li.gs2 = s1.data_ptr(), s2.data_ptr()
                li.seg[0].g_r1, li.seg[0].g_r2 = r1.data_ptr(), r2.data_ptr()
        li.walk_reverse = int(reverse)
        tm = lib.pdr_fused_layer_tile_rows(rpb, Cout)
        tpb = (rpb + tm - 1) // tm
        Y = torch.full((P, ldw), float("nan"), device=dev)
        part = torch.full((B * tpb, Cout, 2), float("nan"), device=dev)
        _lib.check(lib.pdr_fused_layer(ctypes.byref(li), P, Cin, Wt.data_ptr(), ldw, bias.data_ptr(), Cout, Y.data_ptr(),
                                       ldw, part.data_ptr(), Cout, st), "layer")
        torch.cuda.synchronize()
        return Y[:, :Cout].clone(), part.clone()
    y0, p0 = run(False)
    y1, p1 = run(True)
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(p0).all())
    assert torch.equal(y0, y1) and torch.equal(p0, p1)
    if form == "plain":
        x = torch.relu(X[:, :Cin].double().view(B, rpb, Cin) * scale.double()[:, None] + shift.double()[:, None])
        want = x.view(P, Cin) @ Wt[:, :Cout].double() + bias.double()
        assert _rel(y1.double(), want) < 2e-5


# ---- round 6: row map of the per-query term, paired launches ---------------------------------------------------------
@pytest.mark.parametrize("rpb,Cin,Cout,K,weighted", [(2048, 32, 32, 32, False), (1024, 64, 128, 32, False),
                                                     (256, 128, 128, 1, True), (64, 256, 128, 1, True),
                                                     (16, 128, 64, 1, True), (2048, 41, 64, 1, True)])
def test_layer_per_query_term_through_a_row_map(cuda, rpb, Cin, Cout, K, weighted):
    """pdr_layer_in_t.oadd_rows: position p adds row oadd_rows[p / div] of `oadd` -- the same bits as adding row p / div
    of the rows gathered into that order; 32 positions per query (the per-neighbour launches of a sorted block) and one
    position per query with weighted statistics (its per-query launches), both kernel families."""
    lib, dev = _lib.load(), cuda
    st = torch.cuda.current_stream().cuda_stream
    B = 3
    g = torch.Generator(device=dev).manual_seed(rpb + Cout + K)
    P, ldx, ldw = B * rpb, (Cin + 3) // 4 * 4, (Cout + 3) // 4 * 4
    X = torch.randn(P, ldx, device=dev, generator=g)
    Wt = torch.randn(Cin, ldw, device=dev, generator=g) * 0.1
    bias = torch.randn(Cout, device=dev, generator=g)
    nq = P // K
    Z = torch.randn(nq, ldw, device=dev, generator=g)
    perm = torch.cat([b * (nq // B) + torch.randperm(nq // B, device=dev, generator=g) for b in range(B)]).int()
    Zg = Z[perm.long()].contiguous()
    thr = torch.tensor([0, rpb // 3, rpb], dtype=torch.int32, device=dev)

    def run(oadd, rows):
        li = _lib.LayerIn()
        li.n_seg = 1
        li.seg[0].ptr, li.seg[0].C, li.seg[0].ld, li.seg[0].row_div = X.data_ptr(), Cin, ldx, 1
        li.rows_per_batch = rpb
        li.oadd, li.oadd_ld, li.oadd_div = oadd.data_ptr(), ldw, K
        if rows is not None:
            li.oadd_rows = rows.data_ptr()
        tm = lib.pdr_fused_layer_tile_rows(rpb, Cout)
        tpb = (rpb + tm - 1) // tm
        if weighted:
            li.wrow0, li.wmul = thr.data_ptr(), float(32)
        Y = torch.empty(P, ldw, device=dev)
        part = torch.empty(B * tpb, Cout, 2, device=dev)
        _lib.check(lib.pdr_fused_layer(ctypes.byref(li), P, Cin, Wt.data_ptr(), ldw, bias.data_ptr(), Cout, Y.data_ptr(),
                                       ldw, part.data_ptr(), Cout // 2, st), "layer")
        torch.cuda.synchronize()
        return Y[:, :Cout].clone(), part.clone()
    y0, p0 = run(Zg, None)
    y1, p1 = run(Z, perm)
    assert torch.equal(y0, y1) and torch.equal(p0, p1)
    want = X[:, :Cin].double() @ Wt[:, :Cout].double() + bias.double() + Zg[:, :Cout].double().repeat_interleave(K, 0)
    assert _rel(y1.double(), want) < 2e-5
