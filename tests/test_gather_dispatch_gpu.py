"""The virtual first conv's gather kernel (csrc/fused_gather.hip) across its dispatch table on the GPU.

One test per group of cases of tests/gather_cases.py; every case is one launch, compared with the float64 numpy reference
at the bounds derived in gather_cases.py (Y of the forms without s1 / s2: bit for bit), with every buffer prefilled with
a sentinel that the entries the launch does not own must still hold.  Each test prints the largest error / bound ratio
it saw.  Beside the reference, the bit-equalities the kernel's comments claim: a column's moments are the same with and
without a Y, from pdr_gather_add (the whole width) and pdr_gather_moments (windows), from passes on grid.y and passes
walked in the workgroup, from a tile subset and the full launch; the twin tiles are a K = 1 pdr_gather_add on the first
neighbours.  tests/test_gather_dispatch_plan.py proves, without a GPU, that the cases reach every cell of the table.
"""
import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd import _lib
from tests import gather_cases as gc

pytestmark = pytest.mark.gpu

S = gc.SENTINEL
GUARD = 3                        # rows behind the last row of Y / Yd; `partial` gets one guard row


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)          # (a copy: the inputs are read-only)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _tensors(c, cuda):
    return {k: _dev(v, cuda) for k, v in gc.inputs(c).items()}


def _run(c, T, cuda):
    """The launch of case c on the device inputs T -> (Y, partial, Yd), each None or prefilled with the sentinel."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    ld, rpb = gc.pad4(c.Cout), c.m * c.K
    ycol0, ycols, ldy = gc.ywindow(c)
    ptpb = gc.partial_tpb(c)
    Y = torch.full((c.B * rpb + GUARD, ldy), S, device=cuda) if c.out != "p" else None
    partial = torch.full((c.B * ptpb + 1, c.Cout, 2), S, device=cuda) if "p" in c.out else None
    has_em = T["counts"] is not None
    head = (T["U"].data_ptr(), ld, c.n_src, T["V2"].data_ptr(), T["V2"].data_ptr() + 4 * ld if has_em else None, 2 * ld,
            T["idx"].data_ptr(), _ptr(T["counts"]))
    knn = (_ptr(T["s1"]), _ptr(T["r1"]), _ptr(T["s2"]), _ptr(T["r2"]))
    size = (c.B, rpb, c.K, c.Cout)
    yargs = (_ptr(Y), ldy, _ptr(partial), c.relu_col0, ycol0, -1 if "w" not in c.out else ycols)
    margs = (_ptr(partial), c.relu_col0) + tuple(c.windows)
    keep = []
    tiles, twin, Yd = (), (), None
    if c.tiles:
        tv = _dev(gc.tile_valid(c).reshape(-1), cuda)
        keep.append(tv)
        tiles = (tv.data_ptr(), ptpb)
    if c.twin:
        idx0 = T["idx"].view(c.B, c.m, c.K)[:, :, 0].contiguous()
        wrow0 = torch.tensor(c.twin[0], dtype=torch.int32, device=cuda)
        Yd = torch.full((c.B * c.m + GUARD, ld + 4), S, device=cuda)
        keep += [idx0, wrow0]
        twin = (idx0.data_ptr(), Yd.data_ptr(), ld + 4, wrow0.data_ptr(), float(c.twin[1]))
    if c.entry == "add":
        rc = lib.pdr_gather_add(*head, *knn, *size, *yargs, st)
    elif c.entry == "add_tiles":
        rc = lib.pdr_gather_add_tiles(*head, *knn, *size, *yargs, *tiles, st)
    elif c.entry == "add_twin":
        rc = lib.pdr_gather_add_tiles_twin(*head, *size, *yargs, *tiles, *twin, st)
    elif c.entry == "moments":
        rc = lib.pdr_gather_moments(*head, *knn, *size, *margs, st)
    elif c.entry == "moments_tiles":
        rc = lib.pdr_gather_moments_tiles(*head, *knn, *size, *margs, *tiles, st)
    elif c.entry == "moments_twin":
        rc = lib.pdr_gather_moments_tiles_twin(*head, *size, *margs, *tiles, *twin, st)
    else:
        raise ValueError(c.entry)
    _lib.check(rc, gc.case_id(c))
    torch.cuda.synchronize()
    return Y, partial, Yd


def _ratio(err, bound, what):
    """max err / bound; where the bound is 0 the error must be 0."""
    assert (err[bound == 0] == 0).all(), what + ": differs where the reference is exact"
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _check(c, ref, Y, partial, Yd):
    """-> the largest error / bound ratios (Y, m1, m2); asserts the bounds and the untouched memory."""
    what = gc.case_id(c)
    P, ratios = c.B * c.m * c.K, [0.0, 0.0, 0.0]
    if Y is not None:
        ycol0, ycols, _ = gc.ywindow(c)
        y4 = gc.pad4(ycols)
        Yh = Y.cpu().numpy()
        assert (Yh[P:] == S).all(), what + ": a guard row behind Y was written"
        assert (Yh[:, y4:] == S).all(), what + ": a column of Y behind the padded window was written"
        assert (Yh[:P][~ref.row_written] == S).all(), what + ": a row of a cleared tile was written"
        got = Yh[:P, :ycols][ref.row_written]
        assert not (got == S).any(), what + ": an entry of Y was not written"
        if ref.y32 is not None:
            want = ref.y32[ref.row_written, ycol0:ycol0 + ycols]
            bad = np.argwhere(got != want)
            assert not len(bad), "%s: Y is not the float32 sum: %d entries, first %r: %r vs %r" % (
                what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        else:
            err = np.abs(got.astype(np.float64) - ref.y64[ref.row_written, ycol0:ycol0 + ycols])
            ratios[0] = _ratio(err, ref.ybound[ref.row_written, ycol0:ycol0 + ycols], what + " Y")
            assert ratios[0] <= 1.0, "%s: |Y - ref| is %.3f of its bound" % (what, ratios[0])
    if partial is not None:
        ph = partial.cpu().numpy().astype(np.float64)
        assert (ph[-1] == S).all(), what + ": the guard row behind partial was written"
        ph = ph[:-1]
        assert (ph[~ref.mom_written] == S).all(), what + ": an entry of partial outside the windows / tiles was written"
        assert not (ph[ref.mom_written] == S).any(), what + ": an entry of partial was not written"
        err = np.abs(ph - ref.mom)[ref.mom_written]
        bound = ref.mom_bound[ref.mom_written]
        for k in (0, 1):
            ratios[1 + k] = _ratio(err[:, k], bound[:, k], "%s m%d" % (what, k + 1))
            assert ratios[1 + k] <= 1.0, "%s: |m%d - ref| is %.3f of its bound" % (what, k + 1, ratios[1 + k])
    if Yd is not None:
        Q, c4 = c.B * c.m, gc.pad4(c.Cout)
        Ydh = Yd.cpu().numpy()
        assert (Ydh[Q:] == S).all() and (Ydh[:, c4:] == S).all(), what + ": the twin wrote rows / columns of nothing"
        assert np.array_equal(Ydh[:Q, :c.Cout], ref.yd32), what + ": the twin's rows are not the float32 sum"
    return ratios


def _win(c, cuda):
    return torch.from_numpy(gc.in_windows(c)).to(cuda)


def _twin_as_k1(c, T, cuda, partial, Yd):
    """tw.Y and the twin moments, bit for bit: a K = 1 pdr_gather_add on idx0 gives the rows; the same launch with the
    queries q < wrow0[b] turned into empty balls whose V0 row is zero adds +0 where the twin adds nothing, so its tile
    moments times wmul (one float32 multiply) are the twin's."""
    what = gc.case_id(c)
    ld, Q = gc.pad4(c.Cout), c.B * c.m
    T1 = dict(T, idx=T["idx"].view(c.B, c.m, c.K)[:, :, 0].contiguous())
    c1 = c._replace(entry="add", K=1, out="yp", windows=(0, c.Cout, 0, 0), tiles=None, twin=None)
    Y1, _, _ = _run(c1, T1, cuda)
    assert torch.equal(Yd[:Q, :c.Cout], Y1[:Q, :c.Cout]), what + ": tw.Y differs from the K = 1 pdr_gather_add"
    q = torch.arange(c.m, device=cuda)[None, :]
    skipped = (q < torch.tensor(c.twin[0], device=cuda)[:, None]).reshape(-1)
    counts = T["counts"].reshape(-1).clone() if T["counts"] is not None else torch.ones(Q, dtype=torch.int32, device=cuda)
    counts[skipped] = 0
    V2 = T["V2"].reshape(Q, 2 * ld).clone()
    V2[skipped, ld:] = 0.0
    T2 = dict(T1, counts=counts, V2=V2)
    _, p1, _ = _run(c1._replace(out="p", form="ball_em"), T2, cuda)
    tpb, ttpb, ptpb = gc.tiles_per_cloud(c), gc.twin_tiles_per_cloud(c), gc.partial_tpb(c)
    got = partial[:-1].view(c.B, ptpb, c.Cout, 2)[:, tpb:tpb + ttpb]
    want = p1[:-1].view(c.B, ttpb, c.Cout, 2) * torch.tensor(c.twin[1], dtype=torch.float32, device=cuda)
    w = _win(c, cuda)
    assert torch.equal(got[:, :, w], want[:, :, w]), what + ": twin moments differ from the K = 1 launch's times wmul"


def _bit_equalities(c, T, cuda, Y, partial, Yd):
    what = gc.case_id(c)
    w = _win(c, cuda)
    if c.entry.startswith("add") and Y is not None and partial is not None:
        _, p2, _ = _run(c._replace(out="p"), T, cuda)
        assert torch.equal(partial, p2), what + ": the moments differ without a Y"
    if c.entry.startswith("moments"):
        _, p2, yd2 = _run(c._replace(entry=c.entry.replace("moments", "add"), windows=(0, c.Cout, 0, 0)), T, cuda)
        assert torch.equal(partial[:, w], p2[:, w]), what + ": window moments differ from pdr_gather_add's"
        if Yd is not None:
            assert torch.equal(Yd, yd2), what + ": tw.Y differs from pdr_gather_add_tiles_twin's"
    if c.tiles and not c.twin:
        full = c._replace(entry=c.entry.replace("_tiles", ""), tiles=None)
        Yf, pf, _ = _run(full, T, cuda)
        tv = torch.from_numpy(gc.tile_valid(c).astype(bool)).to(cuda)
        tpb, ptpb = gc.tiles_per_cloud(c), gc.partial_tpb(c)
        if partial is not None:
            sub = partial[:-1].view(c.B, ptpb, c.Cout, 2)[:, :tpb][tv]
            assert torch.equal(sub[:, w], pf[:-1].view(c.B, tpb, c.Cout, 2)[tv][:, w]), what + ": subset != full launch"
        if Y is not None:
            rows = torch.from_numpy(gc.reference(c).row_written).to(cuda)
            P = rows.shape[0]
            assert torch.equal(Y[:P][rows], Yf[:P][rows]), what + ": Y of the subset != Y of the full launch"
    if c.twin:
        _twin_as_k1(c, T, cuda, partial, Yd)


GROUPS = gc.groups()


@pytest.mark.parametrize("group", [g for g in GROUPS if g != "serial"])
def test_gather_dispatch_group(cuda, group):
    worst = [0.0, 0.0, 0.0]
    for c in GROUPS[group]:
        rc, plan = gc.plan(c)
        assert rc == _lib.PDR_OK, gc.case_id(c)
        T = _tensors(c, cuda)
        Y, partial, Yd = _run(c, T, cuda)
        r = _check(c, gc.reference(c), Y, partial, Yd)
        worst = [max(a, b) for a, b in zip(worst, r)]
        _bit_equalities(c, T, cuda, Y, partial, Yd)
    print("\ngather %s: %d launches, max error / bound: Y %.3f  m1 %.3f  m2 %.3f" % ((group, len(GROUPS[group])) + tuple(worst)))


def test_serial_passes_are_the_grid_y_passes(cuda):
    """More than 1024 tiles: a workgroup walks its tile's column passes one after the other (LDS reused between
    passes, two barriers per pass).  The same 8-row cloud 1025 times against the reference, every copy equal to the
    first, and the first bit-equal to the launch of three copies, whose passes go to grid.y."""
    worst = [0.0, 0.0, 0.0]
    serial = [c for c in GROUPS["serial"]]
    assert serial
    for c in serial:
        small = c._replace(B=3)
        assert small in gc.all_cases()
        (rc, ps), (rc3, p3) = gc.plan(c), gc.plan(small)
        assert rc == rc3 == _lib.PDR_OK and ps.passes == p3.passes == 2 and ps.grid_y == 1 and p3.grid_y == 2
        outs = {}
        for cc in (c, small):
            T = _tensors(cc, cuda)
            outs[cc.B] = _run(cc, T, cuda)
            r = _check(cc, gc.reference(cc), *outs[cc.B])
            worst = [max(a, b) for a, b in zip(worst, r)]
            if cc.entry == "moments":
                _bit_equalities(cc, T, cuda, *outs[cc.B])
        rpb, tpb = c.m * c.K, gc.tiles_per_cloud(c)
        (Ys, parts, _), (Y3, part3, _) = outs[c.B], outs[3]
        if Ys is not None:
            per = Ys[:c.B * rpb].view(c.B, rpb, -1)
            assert torch.equal(per, per[:1].expand_as(per)) and torch.equal(per[:3], Y3[:3 * rpb].view(3, rpb, -1))
        if parts is not None:
            per = parts[:-1].view(c.B, tpb, c.Cout, 2)
            assert torch.equal(per, per[:1].expand_as(per)), gc.case_id(c) + ": copies of a cloud differ"
            assert torch.equal(per[:3], part3[:-1].view(3, tpb, c.Cout, 2)), gc.case_id(c) + ": serial != grid.y"
    print("\ngather serial: %d launches, max error / bound: Y %.3f  m1 %.3f  m2 %.3f" % ((2 * len(serial),) + tuple(worst)))
