"""pdr_chamfer_loss / pdr_chamfer_loss_grad / pdr_chamfer_loss_workspace_bytes: what is decided on the host (no GPU):
the symbols, every validation rule of include/pdr_hip.h, the workspace query and the argument checks of the Python
surface."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pdr_chamfer_loss_workspace_bytes", "pdr_chamfer_loss", "pdr_chamfer_loss_grad")


def test_symbols_are_declared_exported_and_bound():
    from point_diffusion_refinement_amd import _lib
    text = open(os.path.join(ROOT, "include", "pdr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "point_diffusion_refinement_amd", "libpdr_hip.so"))
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), "%s is not declared in pdr_hip.h" % s
        assert hasattr(lib, s), "libpdr_hip.so does not export %s" % s
        assert s in _lib.SIGNATURES
    assert _lib.SIGNATURES["pdr_chamfer_loss_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES["pdr_chamfer_loss"][1]) == 12 and len(_lib.SIGNATURES["pdr_chamfer_loss_grad"][1]) == 13
    assert _lib.load().pdr_version() == 200                       # additive: no version bump


def test_entry_points_validate_their_arguments_without_a_gpu():
    """Every code is decided before a launch: fake non-NULL pointers are never dereferenced."""
    from point_diffusion_refinement_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUP, OK = _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED, _lib.PDR_OK
    X, Y, L1, L2, S, IX, IY, WS, GS, GX, GY = (0x1000 * k for k in range(1, 12))

    def fwd(x=X, y=Y, l1=None, l2=None, B=2, n1=8, n2=8, sums=S, ix=IX, iy=IY, ws=WS):
        return lib.pdr_chamfer_loss(x, y, l1, l2, B, n1, n2, sums, ix, iy, ws, None)

    def bwd(x=X, y=Y, l1=None, l2=None, ix=IX, iy=IY, gs=GS, B=2, n1=8, n2=8, gx=GX, gy=GY):
        return lib.pdr_chamfer_loss_grad(x, y, l1, l2, ix, iy, gs, B, n1, n2, gx, gy, None)

    for call in (fwd, bwd):
        # sizes: negative, non-positive clouds with B > 0, the empty batch
        assert call(B=-1) == EINVAL and call(n1=-1) == EINVAL and call(n2=-1) == EINVAL
        assert call(n1=0) == EINVAL and call(n2=0) == EINVAL
        assert call(B=0) == OK and call(B=0, n1=0, n2=0) == OK
        assert call(B=0, x=None, y=None) == OK                    # no pointer is looked at
        assert call(B=0, n1=-1) == EINVAL                         # a negative size is refused first
        # sizes the kernels do not index
        assert call(B=65536) == EUNSUP
        assert call(B=2, n1=1 << 30) == EUNSUP and call(B=2, n2=1 << 30) == EUNSUP     # B n >= 2^31
        assert call(B=1, n1=(1 << 24) + 1) == EUNSUP and call(B=1, n2=(1 << 24) + 1) == EUNSUP
        assert call(B=256, n1=1 << 23) == EUNSUP                  # 2^31 exactly
        # ... decided before the pointers
        assert call(B=65536, x=None) == EUNSUP
        assert call(x=None) == EINVAL and call(y=None) == EINVAL
    # forward pointers
    assert fwd(sums=None) == EINVAL
    assert fwd(ix=None) == EINVAL and fwd(iy=None) == EINVAL      # exactly one index array
    assert fwd(ws=None) == EINVAL and fwd(ix=None, iy=None, ws=None) == EINVAL
    assert fwd(ws=WS + 2) == EINVAL and fwd(ws=WS + 1) == EINVAL  # misaligned
    # backward pointers
    for name in ("ix", "iy", "gs", "gx", "gy"):
        assert bwd(**{name: None}) == EINVAL, name


def test_workspace_query():
    from point_diffusion_refinement_amd import _lib
    q = _lib.load().pdr_chamfer_loss_workspace_bytes
    for B in (0, -1, -70000):
        assert q(B, 2048, 2048) == 0
    for args in ((2, 0, 8), (2, 8, 0), (2, -1, 8), (2, 8, -1), (65536, 8, 8), (2, 1 << 30, 8), (1, 8, (1 << 24) + 1),
                 (256, 1 << 23, 8)):
        assert q(*args) == 0, args
    assert q(1, 1, 1) > 0 and q(32, 2048, 2048) > 0
    ns = (1, 2, 7, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4100, 8192, 16383, 16384)
    Bs = (1, 2, 3, 5, 8, 31, 32, 33, 64)
    for n_other in (1, 1024, 16384):
        for B in Bs:
            prev1 = prev2 = 0
            for n in ns:
                a, b = q(B, n, n_other), q(B, n_other, n)
                assert a >= prev1 and b >= prev2 and a > 0 and b > 0
                prev1, prev2 = a, b
    for n1 in (1, 2049, 16384):
        for n2 in (1, 1025, 16384):
            prev = 0
            for B in range(1, 65):
                assert q(B, n1, n2) >= prev
                prev = q(B, n1, n2)


def test_cpu_tensors_are_rejected():
    import torch
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import calc_cd_fused
    x = torch.rand(2, 16, 3)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.chamfer_loss_sums(x, x)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.chamfer_loss_sums(x.requires_grad_(), x)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        calc_cd_fused(x, x)


def test_chamfer_loss_module_rejects_bad_arguments():
    import torch
    from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import ChamferLoss
    for kw in ({"loss_type": "cd"}, {"loss_type": None}, {"reduction": "max"}, {"reduction": "none"}):
        with pytest.raises(ValueError):
            ChamferLoss(**kw)
    for kw in ({}, {"loss_type": "cd_p", "reduction": None}, {"loss_type": "cd_t", "reduction": "sum"}):
        ChamferLoss(**kw)
    x = torch.rand(2, 16, 3)
    with pytest.raises(ValueError, match="negative"):
        ChamferLoss()(x, x, weights=torch.tensor([1.0, -0.5]))
    with pytest.raises(ValueError, match=r"shape \(N,\)"):
        ChamferLoss()(x, x, weights=torch.ones(3))
