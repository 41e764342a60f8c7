"""Length-aware FPS (csrc/fps_ragged.hip) on the GPU: every case of tests/ragged_fps_cases.py against the oracle on each
materialised slice and against the dense kernel, the stream form, prefix consistency, the one-launch
mirror_and_concat against today's dense producer, graph replay with changed lengths, and repeatability."""
import functools

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2.data_utils import mirror_partial
from point_diffusion_refinement_amd.pointnet2_ops import _ext, pointnet2_utils
from tests import ragged_fps_cases as C

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run(xyz, m, lengths, axis, cuda, rows=True):
    """One kernel call on host arrays -> host arrays; lengths None = the NULL pointer."""
    x = torch.tensor(xyz).to(cuda)                             # a copy: the references are read-only
    ln = None if lengths is None else torch.tensor(list(lengths), dtype=torch.int64, device=cuda)
    out = _ext.furthest_point_sampling_ragged(x, m, lengths=ln, mirror_axis=None if axis < 0 else axis,
                                              return_rows=rows)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) if rows else out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case_outputs(case, cuda):
    N, axis, lengths, kind, m = case
    return run(C.ragged_reference(case)[0], m, lengths, axis, cuda)


def check_against(case, idx, rows, want_idx, want_rows):
    for b in range(len(case[2])):
        assert np.array_equal(idx[b], want_idx[b]), "%s cloud %d (length %d): first difference at pick %d" % (
            C.case_id(case), b, case[2][b], int(np.flatnonzero(idx[b] != want_idx[b])[0]))
    assert np.array_equal(bits(rows), bits(want_rows)), C.case_id(case)


@pytest.mark.parametrize("case", C.ragged_cases(), ids=C.case_id)
def test_every_case_against_the_oracle_per_slice(case, cuda):
    _, want_idx, want_rows = C.ragged_reference(case)
    idx, rows = case_outputs(case, cuda)
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape and rows.shape == want_rows.shape
    check_against(case, idx, rows, want_idx, want_rows)
    for b, L in enumerate(case[2]):
        if L == 0:
            assert (idx[b] == -1).all() and (bits(rows[b]) == 0).all()
        else:
            assert idx[b, 0] == 0


@pytest.mark.parametrize("case", C.ragged_cases(), ids=C.case_id)
def test_every_case_against_the_dense_kernel_per_slice(case, cuda):
    N, axis, lengths, kind, m = case
    xyz = C.ragged_reference(case)[0]
    idx, rows = case_outputs(case, cuda)
    for b, L in enumerate(lengths):
        if L == 0:
            continue
        v = C.virtual_cloud(xyz[b], L, axis)
        dense = _ext.furthest_point_sampling(torch.from_numpy(np.ascontiguousarray(v[None, :, :3])).to(cuda), m)
        dense = dense.cpu().numpy()[0]
        assert np.array_equal(idx[b], dense), (C.case_id(case), b)
        assert np.array_equal(bits(rows[b]), bits(v[dense])), (C.case_id(case), b)


@pytest.mark.parametrize("N,axis", [(1, -1), (129, -1), (1000, 1), (2048, 2), (4097, -1), (12289, -1), (6145, 0)])
def test_null_and_full_lengths_give_the_same_bits(N, axis, cuda):
    B, m = 3, min(C.virtual_size(N, axis), 200)
    xyz = C.ragged_input(N, axis, (N,) * B, "lattice")
    a = run(xyz, m, None, axis, cuda)
    b = run(xyz, m, (N,) * B, axis, cuda)
    c = run(xyz, m, (N + 7,) * B, axis, cuda)                  # clamped to N on the device
    for x, y, z in zip(a, b, c):
        assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z))


@pytest.mark.parametrize("kind", ["uniform", "lattice"])
@pytest.mark.parametrize("N,axis", [(12289, -1), (6145, 2)])
def test_stream_form(N, axis, kind, cuda):
    assert C.ragged_plan(N, axis)[1][0] == "stream"
    lengths, m = (N, 5000), 64
    xyz = C.ragged_input(N, axis, lengths, kind)
    idx, rows = run(xyz, m, lengths, axis, cuda)
    for b, L in enumerate(lengths):
        want_idx, want_rows, _ = C.slice_reference(xyz[b], L, axis, m)
        assert np.array_equal(idx[b], want_idx), (b, L)
        assert np.array_equal(bits(rows[b]), bits(want_rows)), (b, L)


def test_prefix_consistency(cuda):
    N, axis, lengths = 1000, 1, C.default_lengths(1000)
    xyz = C.ragged_input(N, axis, lengths, "lattice")
    short = run(xyz, 300, lengths, axis, cuda)
    long = run(xyz, 700, lengths, axis, cuda)
    assert np.array_equal(short[0], long[0][:, :300])
    assert np.array_equal(bits(short[1]), bits(long[1][:, :300]))


@pytest.mark.parametrize("kind", ["uniform", "lattice"])
def test_mirror_and_concat_with_full_lengths_is_the_dense_producer(kind, cuda):
    B, N = 2, 2048
    partial = torch.from_numpy(C.ragged_input(N, 2, (N,) * B, kind)).to(cuda)
    full = torch.full((B,), N, dtype=torch.int64, device=cuda)
    dense = mirror_partial.mirror_and_concat(partial)
    ragged = mirror_partial.mirror_and_concat(partial, lengths=full)
    assert len(dense) == len(ragged) == 3
    for d, r, n in zip(dense, ragged, (2 * N, 2048, 3072)):
        assert r.shape == d.shape == (B, n, 4) and r.is_contiguous()
        assert torch.equal(d.view(torch.int32), r.view(torch.int32))


def test_mirror_and_concat_with_ragged_lengths_against_the_oracle(cuda):
    B, N, axis, lengths, num_points = 3, 2048, 2, (2048, 1400, 700), (2048, 3072)
    xyz = C.ragged_input(N, axis, lengths, "lattice")
    ln = torch.tensor(lengths, dtype=torch.int64, device=cuda)
    both, small, large = mirror_partial.mirror_and_concat(torch.from_numpy(xyz).to(cuda), axis=axis,
                                                          num_points=num_points, lengths=ln)
    assert both.shape == (B, 2 * N, 4) and small.shape == (B, 2048, 4) and large.shape == (B, 3072, 4)
    for b, L in enumerate(lengths):                            # the last cloud has 1400 < 2048 virtual points: over-asked
        _, want_rows, v = C.slice_reference(xyz[b], L, axis, max(num_points))
        assert np.array_equal(bits(large[b].cpu().numpy()), bits(want_rows)), b
        assert np.array_equal(bits(small[b].cpu().numpy()), bits(want_rows[:2048])), b
        got = both[b].cpu().numpy()
        assert np.array_equal(bits(got[:2 * L]), bits(v)) and (bits(got[2 * L:]) == 0).all(), b


def test_down_sample_points_and_the_autograd_wrapper_with_lengths(cuda):
    N, lengths, m = 300, (300, 151, 1, 0), 64
    xyz = C.ragged_input(N, -1, lengths, "uniform")
    ln = torch.tensor(lengths, dtype=torch.int64, device=cuda)
    x = torch.from_numpy(xyz).to(cuda).requires_grad_(True)
    idx = pointnet2_utils.furthest_point_sample_ragged(x, m, ln)
    assert not idx.requires_grad
    cloud4 = torch.cat([torch.from_numpy(xyz).to(cuda), torch.full((4, N, 1), 7.0, device=cuda)], 2)
    picked = mirror_partial.down_sample_points(cloud4, m, lengths=ln).cpu().numpy()
    for b, L in enumerate(lengths):
        want_idx, want_rows, _ = C.slice_reference(xyz[b], L, -1, m)
        assert np.array_equal(idx[b].cpu().numpy(), want_idx), b
        want = np.concatenate([want_rows[:, :3], np.full((m, 1), 7.0 if L else 0.0, np.float32)], 1)
        assert np.array_equal(bits(picked[b]), bits(want)), b


# a resident launch, one above the 64 KiB of LDS a launch gets without asking for more, and the stream form
@pytest.mark.parametrize("N,axis", [(600, 0), (7000, -1), (13000, -1)])
def test_graph_replay_follows_the_lengths_in_memory(N, axis, cuda):
    m, mirror = 128, None if axis < 0 else axis
    first, second = (N, N // 2 + 1, 1, 0), (77, 0, N, N // 2 + 2)
    xyz = C.ragged_input(N, axis, (N,) * 4, "lattice")        # no padding: both sets of lengths read real points
    x = torch.from_numpy(xyz).to(cuda)
    ln = torch.tensor(first, dtype=torch.int64, device=cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _ext.furthest_point_sampling_ragged(x, m, lengths=ln, mirror_axis=mirror, return_rows=True)   # warm the allocator
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            idx, rows = _ext.furthest_point_sampling_ragged(x, m, lengths=ln, mirror_axis=mirror, return_rows=True)
    torch.cuda.current_stream().wait_stream(side)
    for lengths in (first, second):
        ln.copy_(torch.tensor(lengths, dtype=torch.int64))     # overwritten in place
        idx.fill_(-7)
        rows.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(xyz, m, lengths, axis, cuda)
        assert np.array_equal(idx.cpu().numpy(), eager[0]) and np.array_equal(bits(rows.cpu().numpy()), bits(eager[1]))
        for b, L in enumerate(lengths):
            want_idx, want_rows, _ = C.slice_reference(xyz[b], L, axis, m)
            assert np.array_equal(eager[0][b], want_idx) and np.array_equal(bits(eager[1][b]), bits(want_rows)), b


@pytest.mark.parametrize("N,axis", [(100, 2), (3000, -1), (5000, 1), (13000, -1)])
def test_two_eager_calls_give_identical_bits(N, axis, cuda):
    lengths = C.default_lengths(N)
    xyz = C.ragged_input(N, axis, lengths, "lattice")
    a = run(xyz, 96, lengths, axis, cuda)
    b = run(xyz, 96, lengths, axis, cuda)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
