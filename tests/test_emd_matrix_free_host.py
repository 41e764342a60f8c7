"""Matrix-free EMD gradient entry points without a GPU.

pdr_emd_cost_grad / pdr_emd_cost_grad_ragged: declared in include/pdr_hip.h, exported by libpdr_hip.so, bound in
_lib.SIGNATURES (the ragged arity is the dense arity + 2), named in the 0.2.0 history comment with pdr_version() still
200, and validated on the host like pdr_matchcost_grad, before anything is launched (the pointer 0x1000 is never
dereferenced; the lengths are never read there, so NULL lengths pass like any device pointer).
earth_mover_distance(matrix_free=True, return_match=True) is refused before the device is touched: CPU tensors reach the
ValueError, not the "Only support cuda" assertion."""
import ctypes
import os
import re

import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2 import emd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000
EINVAL, OK = _lib.PDR_EINVAL, _lib.PDR_OK
DENSE, RAGGED = "pdr_emd_cost_grad", "pdr_emd_cost_grad_ragged"


def _header():
    return open(os.path.join(ROOT, "include", "pdr_hip.h")).read()


def _declared_arity():
    """name -> number of parameters of every function include/pdr_hip.h declares"""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: len(args.split(",")) for name, args in re.findall(r"\b(pdr_[a-z0-9_]+)\s*\(([^)]*)\)", text)}


def test_symbols_are_declared_exported_and_bound():
    declared = _declared_arity()
    raw = ctypes.CDLL(os.path.join(ROOT, "point_diffusion_refinement_amd", "libpdr_hip.so"))
    lib = _lib.load()
    for name in (DENSE, RAGGED):
        assert name in declared, "include/pdr_hip.h does not declare %s" % name
        assert hasattr(raw, name), "libpdr_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        assert len(getattr(lib, name).argtypes) == declared[name]
    assert declared[DENSE] == 10 and declared[RAGGED] == declared[DENSE] + 2
    assert len(getattr(lib, RAGGED).argtypes) == len(getattr(lib, DENSE).argtypes) + 2
    # the shape of pdr_matchcost_grad: `temp` stands where `match` stood
    assert _lib.SIGNATURES[DENSE] == _lib.SIGNATURES["pdr_matchcost_grad"]
    assert _lib.SIGNATURES[RAGGED] == _lib.SIGNATURES["pdr_matchcost_grad_ragged"]


def test_version_stays_200_and_the_history_names_both_entries():
    assert _lib.load().pdr_version() == 200 == _lib.ABI_VERSION
    history = _header().split("int pdr_version(void);")[0]
    assert re.search(r"\bpdr_emd_cost_grad\b", history) and re.search(r"\bpdr_emd_cost_grad_ragged\b", history)


def _both(g=P, x=P, y=P, temp=P, B=2, n=64, m=70, g1=P, g2=P):
    """return code with device lengths, NULL lengths, one of each, and of the dense entry: all agree"""
    lib = _lib.load()
    rc = [lib.pdr_emd_cost_grad_ragged(g, x, y, l1, l2, temp, B, n, m, g1, g2, None)
          for l1, l2 in ((P, P), (None, None), (P, None), (None, P))]
    rc.append(lib.pdr_emd_cost_grad(g, x, y, temp, B, n, m, g1, g2, None))
    assert len(set(rc)) == 1, rc
    return rc[0]


@pytest.mark.parametrize("name", ["g", "x", "y", "temp", "g1", "g2"])
def test_a_null_pointer_is_einval(name):
    assert _both(**{name: None}) == EINVAL


def test_sizes_are_validated_and_an_empty_batch_is_a_no_op():
    assert _both(B=-1) == EINVAL
    assert _both(n=0) == EINVAL and _both(n=-3) == EINVAL
    assert _both(m=0) == EINVAL and _both(m=-1) == EINVAL
    assert _both(B=0) == OK
    assert _both(B=0, g=None, x=None, y=None, temp=None, g1=None, g2=None) == OK
    assert _both(B=0, n=0) == EINVAL and _both(B=0, m=0) == EINVAL      # sizes are checked first


def test_matrix_free_with_return_match_is_refused_before_the_device():
    x, y = torch.zeros(2, 8, 3), torch.zeros(2, 9, 3)                    # CPU tensors: any device work would assert
    with pytest.raises(ValueError, match="matrix_free"):
        emd.earth_mover_distance(x, y, matrix_free=True, return_match=True)
    with pytest.raises(ValueError, match="matrix_free"):
        emd.EMD_distance()(x, y, return_match=True, matrix_free=True)
    with pytest.raises(ValueError, match="matrix_free"):
        emd.earth_mover_distance(x, y, False, True, None, None, True)   # positional, after the reference's four
