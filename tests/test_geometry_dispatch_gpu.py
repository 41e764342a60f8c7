"""FPS, kNN and ball query across their dispatch tables on the GPU, bit for bit against oracle.pdr_oracle.

One test per case of tests/geometry_cases.py: it sets the case's options, asks the plan which kernel the call takes (the
cell is part of every failure message), runs the op on each input of the case and compares with the oracle: indices,
squared distances and counts with np.array_equal, the gathered neighbours with the gather of the oracle's indices,
knn_group's weights at the rtol of test_ops_gpu.py::test_knn_group_indices_and_weights.  Under non-default options the
result is also torch.equal to the default-option result of the same call.  tests/test_geometry_dispatch_plan.py proves,
without a GPU, that these cases reach every instantiation at its edges.
"""
import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2_ops import _ext
from tests import geometry_cases as gc

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)          # (a copy: the references are read-only)


def _host(t):
    return t.cpu().numpy()


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    at = tuple(int(v) for v in bad[0])
    return "%d of %d differ; first at %r: kernel %r, oracle %r" % (len(bad), want.size, at, got[at], want[at])


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (
        what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), "%s: %s" % (what, _first_diff(got, want))


# ------------------------------------------------------------------------------------------------------ FPS
@pytest.mark.parametrize("opt,N", gc.fps_cases(), ids=lambda v: str(v))
def test_fps_dispatch_cell(cuda, opt, N):
    m = gc.fps_m(N)
    for kind in gc.FPS_INPUTS:
        xyz, want = gc.fps_reference(N, kind)
        x = _dev(xyz, cuda)
        with gc.options(gc.FPS_OPTION_SETS[opt]):
            rc, cell, slots = gc.fps_plan(N)
            assert rc == _lib.PDR_OK
            got = _ext.furthest_point_sampling(x, m)
        what = "FPS %s N=%d m=%d %s [%s %s, %d slots]" % (opt, N, m, kind, cell[0], cell[1:], slots)
        _same(_host(got), want, what)
        if gc.FPS_OPTION_SETS[opt]:
            assert torch.equal(got, _ext.furthest_point_sampling(x, m)), what + ": differs from the default kernel"


# ------------------------------------------------------------------------------------------------------ kNN
def _knn_points(x, y, K, nn):
    d, i, g = _ext.knn_points(x, y, K, return_nn=nn)
    return (d, i, g) if nn else (d, i)


def _knn_case_id(v):
    return "B%d-n1_%d-n2_%d-K%d-%s" % (v[:4] + ("nn" if v[4] else "no_nn",)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("opt,shape", gc.knn_cases(), ids=_knn_case_id)
def test_knn_dispatch_cell(cuda, opt, shape):
    Bq, n1, n2, K, nn = shape
    for kind in gc.KNN_INPUTS:
        xq, yc, want_d, want_i = gc.knn_reference(shape[:4] + (True,), kind)
        x, y = _dev(xq, cuda), _dev(yc, cuda)
        with gc.options(gc.KNN_OPTION_SETS[opt]):
            rc, cell = gc.knn_plan(shape)
            assert rc == _lib.PDR_OK
            got = _knn_points(x, y, K, nn)
            grp = None
            if gc.knn_group_applies(shape):
                rcg, gcell = gc.knn_plan(shape, group=True)
                assert rcg == _lib.PDR_OK
                grp = _ext.knn_group(x, y, K)
        what = "kNN %s B=%d n1=%d n2=%d K=%d %s %s" % (opt, Bq, n1, n2, K, kind, cell)
        _same(_host(got[1]), want_i, what + " indices")
        _same(_host(got[0]), want_d, what + " distances")
        if nn:
            # y[idx], zeros in the padding slots (idx -1)
            gathered = np.take_along_axis(yc[:, None], np.maximum(want_i, 0)[..., None], 2) * (want_i >= 0)[..., None]
            _same(_host(got[2]), gathered.astype(np.float32), what + " gathered neighbours")
        if grp is not None:
            gwhat = "knn_group %s B=%d n1=%d n2=%d K=%d %s %s" % (opt, Bq, n1, n2, K, kind, gcell)
            assert grp[1].dtype == torch.int32
            _same(_host(grp[1]), want_i.astype(np.int32), gwhat + " indices")
            _same(_host(grp[0]), want_d, gwhat + " distances")
            recip = 1.0 / (want_d.astype(np.float64) + 1e-8)
            np.testing.assert_allclose(_host(grp[2]), recip / recip.sum(-1, keepdims=True), rtol=2e-6, err_msg=gwhat)
        if gc.KNN_OPTION_SETS[opt]:
            for a, b in zip(got, _knn_points(x, y, K, nn)):
                assert torch.equal(a, b), what + ": differs from the default kernel"
            if grp is not None:
                for a, b in zip(grp, _ext.knn_group(x, y, K)):
                    assert torch.equal(a, b), gwhat + ": differs from the default kernel"


# ----------------------------------------------------------------------------------------------- ball query
@pytest.mark.parametrize("case", gc.ball_cases(), ids=lambda c: "B%d-m%d-n%d-ns%d" % c[:4])
def test_ball_query_dispatch_cell(cuda, case):
    Bq, m, n, ns, radius = case
    q, xyz, want_i, want_c = gc.ball_reference(case)
    rc, (nch, resident, qpw, gx) = gc.ball_plan(case)
    assert rc == _lib.PDR_OK
    idx, cnt = _ext.ball_query(_dev(q, cuda), _dev(xyz, cuda), radius, ns)
    what = "ball query B=%d m=%d n=%d nsample=%d r=%.4f [NCH %d, %s, qpw %d]" % (
        Bq, m, n, ns, radius, nch, "resident" if resident else "stream", qpw)
    _same(_host(cnt), want_c, what + " counts")
    _same(_host(idx), want_i, what + " indices")
