"""Deterministic backward twins (pdr_*_grad_det), host side: the ABI, the workspace query, the argument-error matrix
(decided before any launch: fake pointers, as tests/test_abi.py does it) and the Python switch.  No GPU."""
import re
import os

import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd import pointnet2_ops
from point_diffusion_refinement_amd.pointnet2_ops import _ext
from point_diffusion_refinement_amd.pointnet2_ops import pointnet2_utils as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pdr_scatter_workspace_bytes", "pdr_gather_points_grad_det", "pdr_group_points_grad_det",
       "pdr_three_interpolate_grad_det", "pdr_knn_points_grad_det"]
P_, OK, EINVAL, EUNSUP = 0x1000, _lib.PDR_OK, _lib.PDR_EINVAL, _lib.PDR_EUNSUPPORTED
MAX_N, MAX_P = 16384, 4194304


def test_the_five_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # a _det call takes its twin's arguments plus the workspace, in front of the stream
    for twin in ("pdr_gather_points_grad", "pdr_group_points_grad", "pdr_three_interpolate_grad", "pdr_knn_points_grad"):
        res, args = _lib.SIGNATURES[twin]
        assert _lib.SIGNATURES[twin + "_det"] == (res, args[:-1] + [_lib._P, args[-1]])
    assert "ascending order of their SOURCE POSITION" in header          # the order is stated in words


def test_workspace_bytes():
    ws = _lib.load().pdr_scatter_workspace_bytes
    assert ws(0, 1000, 100) == 0 and ws(-1, 1000, 100) == 0
    sizes_B, sizes_P, sizes_N = [1, 2, 3, 32], [0, 1, 63, 64, 1000, 1024, 1025, 65536, 65537, 70000, 196608, 524288], \
        [1, 63, 96, 3072, 16384]
    for B in sizes_B:
        for N in sizes_N:
            prev = 0
            for P in sizes_P:
                got = ws(B, P, N)
                assert got > 0 and got % 4 == 0 and got >= prev, (B, P, N, got, prev)
                assert got >= 4 * B * (N + 1 + P)                        # start and order are in there
                prev = got
    for P in sizes_P:
        for N in sizes_N:
            assert ws(1, P, N) <= ws(2, P, N) <= ws(3, P, N) <= ws(32, P, N)
        for B in sizes_B:
            col = [ws(B, P, N) for N in sizes_N]
            assert col == sorted(col)
    # the shipped shapes and the 16 384-point Chamfer are supported and modest
    assert 0 < ws(32, 2048 * 32, 3072) < 64 << 20
    assert 0 < ws(32, 16384, 16384) < 512 << 20
    assert ws(1, 524288, 16384) > 0 and ws(4095, 524288, 16384) > 0
    assert ws(1, 1000, MAX_N + 1) == 0 and ws(1, MAX_P + 1, 100) == 0 and ws(4096, 524288, 100) == 0   # refused sizes


def _twin_and_det(name):
    lib = _lib.load()
    return getattr(lib, name), getattr(lib, name + "_det")


def _same(name, argsets):
    """Every argument set: the _det call (workspace given) returns what the atomic twin returns."""
    twin, det = _twin_and_det(name)
    for args, want in argsets:
        assert twin(*args, None) == want, (name, args)
        assert det(*args, P_, None) == want, (name, args)


def test_gather_grad_det_argument_errors():
    _same("pdr_gather_points_grad", [
        ((P_, P_, -1, 4, 10, 5, P_), EINVAL), ((P_, P_, 2, -1, 10, 5, P_), EINVAL), ((P_, P_, 2, 4, 0, 5, P_), EINVAL),
        ((P_, P_, 2, 4, 10, -1, P_), EINVAL),
        ((None, None, 0, 4, 10, 5, None), OK), ((None, None, 2, 0, 10, 5, None), OK),       # nothing looked at
        ((P_, P_, 2, 4, 10, 5, None), EINVAL), ((None, P_, 2, 4, 10, 5, P_), EINVAL), ((P_, None, 2, 4, 10, 5, P_), EINVAL),
        ((None, None, 2, 4, 10, 0, None), EINVAL),
    ])
    _, det = _twin_and_det("pdr_gather_points_grad")
    assert det(P_, P_, 2, 4, 10, 5, P_, None, None) == EINVAL                               # work to do, no workspace
    assert det(P_, P_, 2, 4, 10, 5, P_, 0x1002, None) == EINVAL                             # int32 arrays live in it
    assert det(P_, P_, 0, 4, 10, 5, P_, None, None) == OK and det(P_, P_, 2, 0, 10, 5, P_, None, None) == OK
    assert det(P_, P_, 2, 4, MAX_N + 1, 5, P_, P_, None) == EUNSUP
    assert det(P_, P_, 2, 4, 10, MAX_P + 1, P_, P_, None) == EUNSUP
    assert det(P_, P_, 4096, 4, 10, 524288, P_, P_, None) == EUNSUP                         # B P = 2^31
    assert det(P_, P_, 65536, 4, 10, 5, P_, P_, None) == EUNSUP
    assert det(None, None, 2, 4, MAX_N + 1, 5, None, None, None) == EUNSUP                  # sizes before pointers


def test_group_grad_det_argument_errors():
    _same("pdr_group_points_grad", [
        ((P_, P_, -1, 4, 10, 5, 3, P_), EINVAL), ((P_, P_, 2, -1, 10, 5, 3, P_), EINVAL),
        ((P_, P_, 2, 4, 0, 5, 3, P_), EINVAL), ((P_, P_, 2, 4, 10, -1, 3, P_), EINVAL), ((P_, P_, 2, 4, 10, 5, -1, P_), EINVAL),
        ((None, None, 0, 4, 10, 5, 3, None), OK), ((None, None, 2, 0, 10, 5, 3, None), OK),
        ((P_, P_, 2, 4, 10, 5, 3, None), EINVAL), ((None, P_, 2, 4, 10, 5, 3, P_), EINVAL),
        ((P_, None, 2, 4, 10, 5, 3, P_), EINVAL), ((None, None, 2, 4, 10, 0, 3, None), EINVAL),
    ])
    _, det = _twin_and_det("pdr_group_points_grad")
    assert det(P_, P_, 2, 4, 10, 5, 3, P_, None, None) == EINVAL
    assert det(P_, P_, 2, 4, 10, 5, 3, P_, 0x1001, None) == EINVAL
    assert det(P_, P_, 0, 4, 10, 5, 3, P_, None, None) == OK
    assert det(P_, P_, 2, 4, MAX_N + 1, 5, 3, P_, P_, None) == EUNSUP
    assert det(P_, P_, 2, 4, 10, 2049, 2048, P_, P_, None) == EUNSUP                        # np ns > the P limit
    assert det(P_, P_, 2, 4, 10, 65536, 65536, P_, P_, None) == EUNSUP                      # np ns does not fit an int
    assert det(P_, P_, 4096, 4, 10, 16384, 32, P_, P_, None) == EUNSUP


def test_three_interpolate_grad_det_argument_errors():
    _same("pdr_three_interpolate_grad", [
        ((P_, P_, P_, -1, 4, 7, 10, P_), EINVAL), ((P_, P_, P_, 2, -1, 7, 10, P_), EINVAL),
        ((P_, P_, P_, 2, 4, -1, 10, P_), EINVAL), ((P_, P_, P_, 2, 4, 7, 0, P_), EINVAL),
        ((None, None, None, 0, 4, 7, 10, None), OK), ((None, None, None, 2, 0, 7, 10, None), OK),
        ((P_, P_, P_, 2, 4, 7, 10, None), EINVAL), ((None, P_, P_, 2, 4, 7, 10, P_), EINVAL),
        ((P_, None, P_, 2, 4, 7, 10, P_), EINVAL), ((P_, P_, None, 2, 4, 7, 10, P_), EINVAL),
        ((None, None, None, 2, 4, 0, 10, None), EINVAL),
    ])
    _, det = _twin_and_det("pdr_three_interpolate_grad")
    assert det(P_, P_, P_, 2, 4, 7, 10, P_, None, None) == EINVAL
    assert det(P_, P_, P_, 2, 4, 7, 10, P_, 0x1003, None) == EINVAL
    assert det(P_, P_, P_, 0, 4, 7, 10, P_, None, None) == OK
    assert det(P_, P_, P_, 2, 4, 7, MAX_N + 1, P_, P_, None) == EUNSUP
    assert det(P_, P_, P_, 2, 4, MAX_P // 3 + 1, 10, P_, P_, None) == EUNSUP                # 3 n > the P limit
    assert det(P_, P_, P_, 2048, 4, 349526, 10, P_, P_, None) == EUNSUP                     # B 3 n >= 2^31


def test_knn_grad_det_argument_errors():
    _same("pdr_knn_points_grad", [
        ((P_, P_, P_, P_, -1, 8, 9, 2, P_, P_), EINVAL), ((P_, P_, P_, P_, 2, -1, 9, 2, P_, P_), EINVAL),
        ((P_, P_, P_, P_, 2, 8, -1, 2, P_, P_), EINVAL), ((P_, P_, P_, P_, 2, 8, 9, 0, P_, P_), EINVAL),
        ((None, None, None, None, 0, 8, 9, 2, None, None), OK),
        ((P_, P_, P_, P_, 2, 8, 9, 2, P_, None), EINVAL),
        ((None, None, None, None, 2, 0, 9, 2, None, None), EINVAL),                        # n1 == 0 still writes grad_y
        ((None, None, None, None, 2, 0, 0, 2, None, None), OK),
    ])
    _, det = _twin_and_det("pdr_knn_points_grad")
    # the twin's remaining pointer checks come after it has queued the memset of grad_y, so only the _det call (which
    # decides everything before it touches the stream) is asked with fake pointers: the same code for each
    for hole in range(5):
        args = [P_, P_, P_, P_, 2, 8, 9, 2, P_, P_]
        args[hole if hole < 4 else 8] = None                                                # x, y, idx, grad_dists, grad_x
        assert det(*args, P_, None) == EINVAL, hole
    assert det(P_, P_, P_, P_, 2, 8, 9, 2, P_, P_, None, None) == EINVAL
    assert det(P_, P_, P_, P_, 2, 8, 9, 2, P_, P_, 0x1002, None) == EINVAL
    assert det(P_, P_, P_, P_, 0, 8, 9, 2, P_, P_, None, None) == OK
    assert det(P_, P_, P_, P_, 2, 8, MAX_N + 1, 2, P_, P_, P_, None) == EUNSUP
    assert det(P_, P_, P_, P_, 2, MAX_P // 2 + 1, 9, 2, P_, P_, P_, None) == EUNSUP         # n1 K > the P limit
    assert det(P_, P_, P_, P_, 2, 1 << 30, 9, 32, P_, P_, P_, None) == EUNSUP               # n1 K does not fit an int
    assert det(P_, P_, P_, P_, 8192, 16384, 9, 16, P_, P_, P_, None) == EUNSUP              # B n1 K = 2^31


# ---------------------------------------------------------------------------------------------------- the switch
@pytest.fixture
def restore_modes():
    prev_switch, prev_torch = _ext.set_deterministic(None), torch.are_deterministic_algorithms_enabled()
    yield
    _ext.set_deterministic(prev_switch)
    torch.use_deterministic_algorithms(prev_torch)


def test_switch_follows_torch_unless_set(restore_modes):
    assert pointnet2_ops.set_deterministic is _ext.set_deterministic
    torch.use_deterministic_algorithms(False)
    assert pointnet2_ops.is_deterministic() is False
    torch.use_deterministic_algorithms(True)
    assert pointnet2_ops.is_deterministic() is True
    assert pointnet2_ops.set_deterministic(False) is None and pointnet2_ops.is_deterministic() is False
    torch.use_deterministic_algorithms(False)
    assert pointnet2_ops.set_deterministic(True) is False and pointnet2_ops.is_deterministic() is True
    assert pointnet2_ops.set_deterministic(None) is True and pointnet2_ops.is_deterministic() is False
    with pytest.raises(TypeError):
        pointnet2_ops.set_deterministic(1)


class _Recorder:
    """Stand-in for the native calls of `_ext` the three autograd Functions go through: CPU tensors in, zeros out,
    every call recorded by name with its arguments."""

    NAMES = {"gather_points": lambda f, idx: f.new_zeros(f.shape[0], f.shape[1], idx.shape[1]),
             "group_points": lambda f, idx: f.new_zeros(f.shape[0], f.shape[1], idx.shape[1], idx.shape[2]),
             "three_interpolate": lambda f, idx, w: f.new_zeros(f.shape[0], f.shape[1], idx.shape[1])}
    GRADS = ["gather_points_grad", "group_points_grad", "three_interpolate_grad"]

    def __init__(self, monkeypatch):
        self.calls = []
        for name, fn in self.NAMES.items():
            monkeypatch.setattr(_ext, name, fn)
        for name in self.GRADS + [g + "_det" for g in self.GRADS]:
            monkeypatch.setattr(_ext, name, self._grad(name))

    def _grad(self, name):
        def call(*args):
            self.calls.append((name, args))
            g, n = args[0], args[-1]
            return g.new_zeros(g.shape[0], g.shape[1], n)
        return call


def _run_three_backwards():
    f = torch.rand(2, 5, 11, requires_grad=True)
    idx = torch.zeros(2, 7, dtype=torch.int32)
    PU.gather_operation(f, idx).sum().backward()
    gidx = torch.zeros(2, 4, 3, dtype=torch.int32)
    PU.grouping_operation(f, gidx).sum().backward()
    tidx, w = torch.zeros(2, 9, 3, dtype=torch.int32), torch.rand(2, 9, 3)
    PU.three_interpolate(f, tidx, w).sum().backward()
    return idx, gidx, tidx, w


def test_autograd_functions_call_the_old_names_with_the_switch_off(monkeypatch, restore_modes):
    rec = _Recorder(monkeypatch)
    for off in (lambda: _ext.set_deterministic(False),
                lambda: (_ext.set_deterministic(None), torch.use_deterministic_algorithms(False))):
        off()
        del rec.calls[:]
        idx, gidx, tidx, w = _run_three_backwards()
        assert [c[0] for c in rec.calls] == _Recorder.GRADS
        (_, ga), (_, gr), (_, ti) = rec.calls
        # today's arguments: (grad_out, idx, n) / (grad_out, idx, n) / (grad_out, idx, weight, m)
        same = lambda a, b: a.data_ptr() == b.data_ptr() and a.shape == b.shape
        assert len(ga) == 3 and ga[0].shape == (2, 5, 7) and same(ga[1], idx) and ga[2] == 11
        assert len(gr) == 3 and gr[0].shape == (2, 5, 4, 3) and same(gr[1], gidx) and gr[2] == 11
        assert len(ti) == 4 and ti[0].shape == (2, 5, 9) and same(ti[1], tidx) and same(ti[2], w) and ti[3] == 11
        assert all(a[0].is_contiguous() for a in (ga, gr, ti))


def test_autograd_functions_call_the_det_names_with_the_switch_on(monkeypatch, restore_modes):
    rec = _Recorder(monkeypatch)
    for on in (lambda: _ext.set_deterministic(True),
               lambda: (_ext.set_deterministic(None), torch.use_deterministic_algorithms(True))):
        on()
        del rec.calls[:]
        _run_three_backwards()
        assert [c[0] for c in rec.calls] == [g + "_det" for g in _Recorder.GRADS]
        assert [len(c[1]) for c in rec.calls] == [3, 3, 4]


def test_knn_backward_consults_the_switch(monkeypatch, restore_modes):
    seen = []

    def fake_grad(p1, p2, idx, g, deterministic=False):
        seen.append(deterministic)
        return torch.zeros_like(p1), torch.zeros_like(p2)

    def fake_forward(p1, p2, K, return_nn, lengths1=None, lengths2=None):
        B, n1, _ = p1.shape
        return p1.new_zeros(B, n1, K), torch.zeros(B, n1, K, dtype=torch.int64), None
    monkeypatch.setattr(_ext, "knn_points_grad", fake_grad)
    monkeypatch.setattr(_ext, "_knn_forward", fake_forward)
    for mode in (False, True, None):
        _ext.set_deterministic(mode)
        torch.use_deterministic_algorithms(False)
        x, y = torch.rand(1, 4, 3, requires_grad=True), torch.rand(1, 5, 3, requires_grad=True)
        d, _ = _ext._KnnDists.apply(x, y, 2)
        d.sum().backward()
    assert seen == [False, True, False]


def test_deterministic_mode_never_falls_back(monkeypatch, restore_modes):
    """An unsupported size raises in deterministic mode: the atomic call is not tried."""
    def boom(*a):
        raise RuntimeError("group_points_grad_det failed: unsupported size")
    called = []
    monkeypatch.setattr(_ext, "group_points", _Recorder.NAMES["group_points"])
    monkeypatch.setattr(_ext, "group_points_grad_det", boom)
    monkeypatch.setattr(_ext, "group_points_grad", lambda *a: called.append(a))
    _ext.set_deterministic(True)
    f = torch.rand(1, 2, 6, requires_grad=True)
    with pytest.raises(RuntimeError, match="unsupported size"):
        PU.grouping_operation(f, torch.zeros(1, 2, 2, dtype=torch.int32)).sum().backward()
    assert not called
    assert _lib._ERR[_lib.PDR_EUNSUPPORTED] == "unsupported size"
