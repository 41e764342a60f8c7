"""The JSD of pointnet2/set_metrics.py without a GPU: the grid construction, the entropies and the two JSD formulas on
CPU tensors against tests/golden/jsd.npz (written by the reference's evaluation_metrics.py through
tests/golden/make_jsd_golden.py), the argument validation of pdr_occupancy_grid, which is decided on the host before
any launch, and OccupancyGrid's arithmetic and collective on counters that need no kernel.

TOLERANCE of the entropies and the JSD, 1e-10 absolute: float64, at most 10 144 non-negative terms, entropies at most
log2(10144) = 13.3; any summation order stays below 10144 * 2^-53 * 13.3 * 4 = 6e-11.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from point_diffusion_refinement_amd.pointnet2 import set_metrics as SM
from tests import occupancy_cases as OC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jsd.npz")
TOL = 1e-10
SETTINGS = ((28, True), (5, True), (28, False))


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_fixture_is_what_the_generator_promises(gold):
    assert gold["sample_pcs"].shape == (5, 200, 3) and gold["ref_pcs"].shape == (6, 200, 3)
    assert gold["sample_pcs"].dtype == np.float32 and gold["ref_pcs"].dtype == np.float32
    assert float(gold["jsd_self"]) == 0.0 and 0.0 < float(gold["jsd"]) <= 1.0
    for name in ("sample", "ref"):
        assert 0.2 <= float(gold["occ/%s/R28_clip1/slow_share" % name]) <= 0.8
        for R, clip in SETTINGS:
            counters = gold["occ/%s/R%d_clip%d/counters" % (name, R, int(clip))]
            assert counters.shape == (int(gold["cells/R%d_clip%d" % (R, int(clip))]),)
            assert counters.sum() == gold[name + "_pcs"].shape[0] * 200
    assert os.path.getsize(GOLD) < 1024 * 1024


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("R", [4, 5, 28])
def test_unit_cube_grid_is_bit_equal_to_the_reference(gold, R, clip):
    grid, spacing = SM.unit_cube_grid_point_cloud(R, clip)
    want = gold["grid/R%d_clip%d" % (R, int(clip))]
    assert spacing == 1.0 / float(R - 1)
    assert grid.dtype == np.float32 and grid.shape == ((len(want), 3) if clip else (R, R, R, 3))
    assert np.array_equal(grid.reshape(-1, 3).view(np.uint32), want.view(np.uint32))
    assert len(want) == ({28: 10144, 5: 33, 4: 8}[R] if clip else R ** 3)
    # the tables the kernel reads describe the same grid, and so do the restatement's
    axis, cell_of, cells = SM.grid_tables(R, clip, "cpu")
    assert cells == len(want) and axis.dtype == torch.float32 and cell_of.dtype == torch.int32
    full = SM.unit_cube_grid_point_cloud(R, False)[0].reshape(-1, 3)
    flat = cell_of.reshape(-1).numpy()
    assert np.array_equal(flat[flat >= 0], np.arange(cells)) and np.array_equal(full[flat >= 0], want)
    assert np.array_equal(axis.numpy(), full.reshape(R, R, R, 3)[0, 0, :, 2])
    o_axis, o_cell_of, o_kept = OC.tables(R, clip)
    assert np.array_equal(o_axis, axis.numpy()) and np.array_equal(o_cell_of, cell_of.numpy())
    assert np.array_equal(o_axis[o_kept], want)


def test_jsd_from_the_golden_counters_on_cpu_tensors(gold):
    for R, clip in SETTINGS:
        tag = "R%d_clip%d" % (R, int(clip))
        P = torch.from_numpy(gold["occ/sample/%s/counters" % tag])
        Q = torch.from_numpy(gold["occ/ref/%s/counters" % tag])
        got = SM.jensen_shannon_divergence(P, Q)
        assert got.dtype == torch.float64 and got.dim() == 0
        if (R, clip) == (28, True):
            assert abs(float(got) - float(gold["jsd"])) <= TOL
        assert abs(float(SM._jsdiv(P, Q)) - float(got)) <= 1e-4          # the reference's own agreement bound
        assert abs(float(SM.jensen_shannon_divergence(P, P))) <= TOL
    P, Q = torch.from_numpy(gold["hand/P"]), torch.from_numpy(gold["hand/Q"])
    assert abs(float(SM.jensen_shannon_divergence(P, Q)) - float(gold["hand/jsd"])) <= TOL
    assert abs(float(SM._jsdiv(P, Q)) - float(gold["hand/jsdiv"])) <= TOL
    assert abs(float(SM._jsdiv(P, Q)) - float(gold["hand/jsd"])) <= 1e-4
    assert SM._jsdiv(P, Q).dtype == torch.float64 and SM._jsdiv(P, Q).dim() == 0


def test_entropy_from_the_restated_bernoulli_counts_matches_the_reference(gold):
    """The reference returns the entropy but not the per-cloud counts behind it; the generator asserted that the
    restatement's counts reproduce it, so they stand in here."""
    for name in ("sample", "ref"):
        pcs = gold[name + "_pcs"]
        for R, clip in SETTINGS:
            tag = "R%d_clip%d" % (R, int(clip))
            occ = OC.occupancy(pcs, R, clip)
            assert np.array_equal(occ["counters"], gold["occ/%s/%s/counters" % (name, tag)].astype(np.int64))
            grid = SM.OccupancyGrid.from_counters(torch.from_numpy(occ["counters"]), torch.from_numpy(occ["bernoulli"]),
                                                  len(pcs), resolution=R, in_sphere=clip)
            ent = grid.entropy()
            assert ent.dtype == torch.float64 and ent.dim() == 0
            assert abs(float(ent) - float(gold["occ/%s/%s/entropy" % (name, tag)])) <= TOL


def test_the_two_value_errors():
    P = torch.tensor([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="Negative values."):
        SM.jensen_shannon_divergence(torch.tensor([1.0, -2.0, 3.0]), P)
    with pytest.raises(ValueError, match="Negative values."):
        SM.jensen_shannon_divergence(P, torch.tensor([1.0, 2.0, -3.0]))
    with pytest.raises(ValueError, match="Non equal size."):
        SM.jensen_shannon_divergence(P, torch.tensor([1.0, 2.0]))


def test_occupancy_grid_validates_its_arguments_without_a_gpu():
    """pdr_occupancy_grid: argument errors are return codes decided on the host (nothing is launched; the pointers below
    are never dereferenced); an empty set is a no-op that looks at no pointer."""
    from point_diffusion_refinement_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUP, OK = _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED, _lib.PDR_OK

    def call(clouds=0x1000, lengths=None, S=3, n=64, R=28, axis=0x2000, cell_of=0x3000, cells=10144, counters=0x4000,
             bernoulli=0x5000, skipped=0x6000):
        return lib.pdr_occupancy_grid(clouds, lengths, S, n, R, axis, cell_of, cells, counters, bernoulli, skipped, None)
    # negative sizes, even for an empty set
    assert call(S=-1) == EINVAL and call(n=-1) == EINVAL and call(R=-1) == EINVAL and call(cells=-1) == EINVAL
    assert call(S=0, n=-1) == EINVAL
    # an empty set: nothing to do, whatever the pointers and the grid
    assert call(S=0) == OK and call(S=0, n=0) == OK
    assert call(S=0, clouds=None, axis=None, cell_of=None, counters=None, bernoulli=None, skipped=None) == OK
    # clouds without points, a grid without cells
    assert call(n=0) == EINVAL and call(cells=0) == EINVAL
    # missing tensors; lengths and skipped may be absent
    for name in ("clouds", "axis", "cell_of", "counters", "bernoulli"):
        assert call(**{name: None}) == EINVAL, name
    # sizes outside what the kernel was built for
    assert call(R=1, cells=1) == EUNSUP and call(R=0, cells=1) == EUNSUP and call(R=33) == EUNSUP
    assert call(R=28, cells=28 ** 3 + 1) == EUNSUP and call(R=2, cells=9) == EUNSUP
    assert call(S=1 << 20, n=1 << 11) == EUNSUP and call(S=1 << 11, n=1 << 20) == EUNSUP       # S n = 2^31
    # one point fewer is supported: the call goes on to look at its pointers
    assert call(S=1, n=(1 << 31) - 1, clouds=None) == EINVAL


def test_occupancy_grid_rejects_cpu_tensors():
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    x = torch.rand(2, 16, 3)
    axis, cell_of, cells = SM.grid_tables(4, True, "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.occupancy_grid(x, axis, cell_of, cells)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        SM.entropy_of_occupancy_grid(x, 4, True)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        SM.jsd_between_point_cloud_sets(x, x)


def test_from_counters_and_merge(gold):
    cs = torch.from_numpy(gold["occ/sample/R28_clip1/counters"]).to(torch.int64)
    cr = torch.from_numpy(gold["occ/ref/R28_clip1/counters"]).to(torch.int64)
    a = SM.OccupancyGrid.from_counters(cs, (cs > 0).to(torch.int64), 5, skipped=1)
    b = SM.OccupancyGrid.from_counters(cr, (cr > 0).to(torch.int64) * 2, 6)
    assert a.counters.dtype == torch.int64 and a.n_clouds.dim() == 0 and int(a.skipped) == 1
    assert abs(float(a.jsd(b)) - float(gold["jsd"])) <= TOL and float(a.jsd(a)) == 0.0
    a.merge(b)
    assert torch.equal(a.counters, cs + cr) and torch.equal(a.bernoulli, (cs > 0).long() + 2 * (cr > 0).long())
    assert int(a.n_clouds) == 11 and int(a.skipped) == 1
    assert torch.equal(cs, torch.from_numpy(gold["occ/sample/R28_clip1/counters"]).long())    # the inputs were copied
    with pytest.raises(ValueError):
        a.merge(SM.OccupancyGrid.from_counters(cs[:33], cs[:33], 5, resolution=5))
    # entropy by hand: 4 cells, 4 clouds, a cell in every, in half, in one and in no cloud
    g = SM.OccupancyGrid.from_counters(torch.tensor([9, 5, 1, 0]), torch.tensor([4, 2, 1, 0]), 4, resolution=4)
    h = lambda p: -(p * np.log(p) + (1 - p) * np.log(1 - p))
    assert abs(float(g.entropy()) - (0.0 + h(0.5) + h(0.25) + 0.0) / 4) <= 1e-15


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        with np.load(GOLD) as z:
            mine = torch.from_numpy(z["occ/%s/R28_clip1/counters" % ("sample", "ref")[rank]]).long()
            ref = torch.from_numpy(z["occ/ref/R28_clip1/counters"]).long()
        grid = SM.OccupancyGrid.from_counters(mine, (mine > 0).long(), 5 + rank, skipped=rank).all_reduce()
        against = SM.OccupancyGrid.from_counters(ref, ref, 6)     # not reduced: the same on both ranks
        out[rank] = (grid.counters.numpy(), grid.bernoulli.numpy(), int(grid.n_clouds), int(grid.skipped),
                     float(grid.jsd(against)), float(grid.entropy()), float(grid.jsd(grid)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_all_reduce_sums_the_grids(gold):
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    cs, cr = (gold["occ/%s/R28_clip1/counters" % k].astype(np.int64) for k in ("sample", "ref"))
    for r in range(2):
        counters, bernoulli, n_clouds, skipped = out[r][:4]
        assert np.array_equal(counters, cs + cr) and np.array_equal(bernoulli, (cs > 0) * 1 + (cr > 0) * 1)
        assert n_clouds == 11 and skipped == 1
    assert out[0][4:] == out[1][4:]                                 # jsd and entropy: the same bits on both ranks
    want = SM.jensen_shannon_divergence(torch.from_numpy(cs + cr), torch.from_numpy(cr))
    assert abs(out[0][4] - float(want)) <= TOL and out[0][4] > 0.0 and out[0][6] == 0.0
