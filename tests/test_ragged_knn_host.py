"""pdr_knn_points_ragged / pdr_chamfer_nn_ragged without a GPU: the symbols are exported and bound, and their argument
validation is the dense entries' (decided on the host before anything is launched; the lengths are never read there,
so NULL lengths pass it like any device pointer)."""
import ctypes
import os

from point_diffusion_refinement_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                          # (never dereferenced: every call below returns before a launch)
EINVAL, EUNSUP, OK = _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED, _lib.PDR_OK


def test_ragged_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(os.path.join(ROOT, "point_diffusion_refinement_amd", "libpdr_hip.so"))
    for name in ("pdr_knn_points_ragged", "pdr_chamfer_nn_ragged"):
        assert hasattr(raw, name), "libpdr_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert len(lib.pdr_knn_points_ragged.argtypes) == len(lib.pdr_knn_points.argtypes) + 2
    assert len(lib.pdr_chamfer_nn_ragged.argtypes) == len(lib.pdr_chamfer_nn.argtypes) + 2
    assert lib.pdr_version() == 200


def test_knn_points_ragged_validates_like_the_dense_entry():
    lib = _lib.load()

    def both(x=P, y=P, B=2, n1=64, n2=64, K=8, d=P, i=P, nn=P):
        """return code with device lengths, with NULL lengths, and of the dense entry: all three agree"""
        rc = [lib.pdr_knn_points_ragged(x, y, l1, l2, B, n1, n2, K, d, i, nn, None)
              for l1, l2 in ((P, P), (None, None), (P, None), (None, P))]
        rc.append(lib.pdr_knn_points(x, y, B, n1, n2, K, d, i, nn, None))
        assert len(set(rc)) == 1, rc
        return rc[0]

    assert both(x=None) == EINVAL and both(y=None) == EINVAL                  # cloud pointers
    assert both(d=None) == EINVAL and both(i=None) == EINVAL                  # output pointers
    assert both(B=-1) == EINVAL and both(n1=-1) == EINVAL and both(n2=-1) == EINVAL and both(K=0) == EINVAL
    assert both(K=33) == EUNSUP and both(K=33, x=None) == EUNSUP
    assert both(B=0) == OK and both(B=0, x=None, d=None) == OK                # empty batch: a no-op
    assert both(n1=0) == OK                                                   # no queries: nothing to write


def test_chamfer_nn_ragged_validates_like_the_dense_entry():
    lib = _lib.load()

    def both(x=P, y=P, B=2, n1=64, n2=64, dx=P, ix=P, dy=P, iy=P):
        rc = [lib.pdr_chamfer_nn_ragged(x, y, l1, l2, B, n1, n2, dx, ix, dy, iy, None)
              for l1, l2 in ((P, P), (None, None), (P, None), (None, P))]
        rc.append(lib.pdr_chamfer_nn(x, y, B, n1, n2, dx, ix, dy, iy, None))
        assert len(set(rc)) == 1, rc
        return rc[0]

    for name in ("x", "y", "dx", "ix", "dy", "iy"):
        assert both(**{name: None}) == EINVAL, name
    assert both(B=-1) == EINVAL and both(n1=0) == EINVAL and both(n2=0) == EINVAL
    assert both(B=0) == OK and both(B=0, x=None) == OK
