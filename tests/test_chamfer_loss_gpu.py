"""The fused Chamfer loss on the GPU: pdr_chamfer_loss / pdr_chamfer_loss_grad through _ext.chamfer_loss_sums,
calc_cd_fused and ChamferLoss.

References: minima and indices are _ext.chamfer_nn's (existing code, so exact ties cannot split the reference from the
kernel); the sums are float64 sums of those fp32 minima; the gradient is float64 on the CPU from the fp32 inputs and
chamfer_nn's indices, term by term, cross-checked against torch autograd of the same fixed-index expression.

Tolerances.  The header of csrc/chamfer_loss.hip states a chain of 12 + ceil(n / 1024) <= 28 dependent fp32 roundings
for n <= 16384 over non-negative addends: sums[:, 0:2] within 28 * 2^-24 relative, sums[:, 2:4] within 30 * 2^-24 (one
sqrt rounding per addend at up to 1 ulp on top).  A gradient element with float64 terms t_m, k of them scattered, is
within (k + 16) * 2^-24 * sum |t_m|: one rounding for the difference, one for the product, about 8 for the sqrt
coefficient (5 from the fp32 distance, halved by the root, plus sqrt, divide, multiply and add), k for the adds, and a
slack of about 1.3 x."""
import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2_ops import _ext
from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import ChamferLoss, calc_cd, calc_cd_fused

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SUM_CHAIN, SQRT_CHAIN = 28, 30
SHAPES = [(2, 1, 1), (3, 5, 1030), (2, 1025, 7), (2, 2051, 2048), (1, 4100, 4100)]
CASES = ([("uniform", s) for s in SHAPES]
         + [("lattice", s) for s in ((3, 5, 1030), (2, 1025, 7), (2, 2051, 2048))]
         + [("same_y", s) for s in ((3, 5, 1030), (2, 2051, 2048))]
         + [("equal", s) for s in ((2, 1, 1), (1, 4100, 4100))])
GRAD_SUMS = ("random", "squared_only", "sqrt_only")
_ids = lambda c: "%s-%dx%dx%d" % ((c[0],) + c[1])


def make(kind, shape):
    """fp32 host clouds (B,n1,3), (B,n2,3), seeded per kind and shape."""
    B, n1, n2 = shape
    rng = np.random.default_rng([B, n1, n2, len(kind)])
    if kind == "lattice":                                        # a 5^3 lattice: exact distance ties and duplicates
        x = rng.integers(0, 5, (B, n1, 3)).astype(np.float32) * 0.25
        y = rng.integers(0, 5, (B, n2, 3)).astype(np.float32) * 0.25 + np.float32(0.125)
        return x, y
    x = rng.uniform(-1, 1, (B, n1, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (B, n2, 3)).astype(np.float32)
    if kind == "same_y":                                         # one destination with n1 sources
        y[:] = y[:, :1]
    if kind == "equal":
        assert n1 == n2
        y = x.copy()
    return x, y


def grad_sums_of(pattern, B, seed=0):
    """(B,4) fp32: random magnitudes, ONE sign per cloud (both signs occur).  The bound's "one rounding for the add" of
    g0 + g2 * 0.5 / sqrt(d) holds when the two do not cancel; with opposite signs the contract's own fp32 evaluation
    order loses the cancelled bits (a numpy emulation of it misses the bound by the same factor)."""
    rng = np.random.default_rng(1000 + seed)
    sign = np.where(np.arange(B) % 2, -1.0, 1.0).astype(np.float32)[:, None]
    g = rng.uniform(0.25, 2.0, (B, 4)).astype(np.float32) * sign
    if pattern == "squared_only":
        g[:, 2:] = 0.0
        g[:, 1] = g[:, 0]
    if pattern == "sqrt_only":
        g[:, :2] = 0.0
        g[:, 3] = g[:, 2]
    return g


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def dev(a, cuda, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(cuda)


def eff(lengths, n):
    return None if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, n)


def run_loss(x, y, lx, ly, gs):
    """Forward with indices and backward through the public Function: (sums, grad_x, grad_y), device tensors."""
    xr, yr = x.detach().clone().requires_grad_(), y.detach().clone().requires_grad_()
    sums = _ext.chamfer_loss_sums(xr, yr, lx, ly)
    gx, gy = torch.autograd.grad(sums, (xr, yr), gs)
    return sums.detach(), gx, gy


_CACHE = {}


def reference(kind, shape, cuda):
    """Device inputs, chamfer_nn's minima / indices and the kernel's sums / indices of a dense case, computed once."""
    key = (kind, shape)
    if key not in _CACHE:
        xh, yh = make(kind, shape)
        x, y = dev(xh, cuda), dev(yh, cuda)
        dxy, ixy, dyx, iyx = (t.cpu().numpy() for t in _ext.chamfer_nn(x, y))
        sums, ix, iy = _ext._chamfer_loss_forward(x, y, None, None, True)
        for a in (xh, yh, dxy, ixy, dyx, iyx):
            a.setflags(write=False)
        _CACHE[key] = dict(xh=xh, yh=yh, x=x, y=y, dxy=dxy, ixy=ixy, dyx=dyx, iyx=iyx, sums=sums.cpu().numpy(),
                           ix=ix.cpu().numpy(), iy=iy.cpu().numpy())
    return _CACHE[key]


def check_sums(sums, dxy, dyx, valid_x=None, valid_y=None):
    """sums (4,) fp32 against the float64 sums of chamfer_nn's fp32 minima over the valid queries."""
    dxy = dxy.astype(np.float64) if valid_x is None else dxy[valid_x].astype(np.float64)
    dyx = dyx.astype(np.float64) if valid_y is None else dyx[valid_y].astype(np.float64)
    want = [dxy.sum(), dyx.sum(), np.sqrt(dxy).sum(), np.sqrt(dyx).sum()]
    for k, chain in enumerate((SUM_CHAIN, SUM_CHAIN, SQRT_CHAIN, SQRT_CHAIN)):
        err = abs(float(sums[k]) - want[k])
        print("sums[%d] = %.9g want %.9g rel %.3g (bound %.3g)" % (k, sums[k], want[k], err / max(want[k], 1e-300),
                                                                  chain * U))
        assert err <= chain * U * want[k], (k, float(sums[k]), want[k])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_indices_minima_and_sums_are_chamfer_nn_s(cuda, case):
    r = reference(*case, cuda)
    assert r["ix"].dtype == np.int32 and r["iy"].dtype == np.int32
    assert np.array_equal(r["ix"], r["ixy"]) and np.array_equal(r["iy"], r["iyx"])
    for b in range(case[1][0]):
        check_sums(r["sums"][b], r["dxy"][b], r["dyx"][b])
    # a loss-only call (no index asked for, as under no_grad) gives the same bits
    with torch.no_grad():
        plain = _ext.chamfer_loss_sums(r["x"].clone().requires_grad_(), r["y"])
    assert not plain.requires_grad and np.array_equal(bits(plain), bits(r["sums"]))


def reference_grad(xh, yh, ixy, iyx, gs):
    """float64 gradient of sum_b g0 S d_xy + g1 S d_yx + g2 S sqrt d_xy + g3 S sqrt d_yx with FIXED indices (-1: no
    term), the sqrt term dropped where d == 0; per element also sum |terms| and the number of scattered sources."""
    x, y, g = xh.astype(np.float64), yh.astype(np.float64), gs.astype(np.float64)
    B = x.shape[0]
    out = []
    for q, c, iq, ic, gq, gq_s, gc, gc_s in ((x, y, ixy, iyx, g[:, 0], g[:, 2], g[:, 1], g[:, 3]),
                                             (y, x, iyx, ixy, g[:, 1], g[:, 3], g[:, 0], g[:, 2])):
        want, mag, cnt = np.zeros_like(q), np.zeros_like(q), np.zeros(q.shape[:2], np.int64)

        def coef(diff, g_sq, g_sqrt):
            d = (diff * diff).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(d > 0, 0.5 / np.sqrt(d), 0.0)
            return 2.0 * (g_sq + g_sqrt * s)                     # s is finite: a zero coefficient gives a zero term
        for b in range(B):
            v = np.nonzero(iq[b] >= 0)[0]                        # own queries
            diff = q[b, v] - c[b, iq[b, v]]
            t = coef(diff, gq[b], gq_s[b])[:, None] * diff
            want[b, v] += t
            mag[b, v] += np.abs(t)
            s = np.nonzero(ic[b] >= 0)[0]                        # sources of the opposite direction
            dest = ic[b, s]
            diff = c[b, s] - q[b, dest]
            t = coef(diff, gc[b], gc_s[b])[:, None] * diff
            np.subtract.at(want[b], dest, t)
            np.add.at(mag[b], dest, np.abs(t))
            np.add.at(cnt[b], dest, 1)
        out.append((want, mag, cnt))
    return out


def autograd_grad(xh, yh, ixy, iyx, gs):
    """The same expression differentiated by torch autograd in float64 on the CPU."""
    x = torch.tensor(xh, dtype=torch.float64, requires_grad=True)
    y = torch.tensor(yh, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(gs, dtype=torch.float64)
    loss = x.sum() * 0 + y.sum() * 0
    for b in range(x.shape[0]):
        for q, c, idx, k in ((x, y, ixy, 0), (y, x, iyx, 1)):
            v = torch.tensor(np.nonzero(idx[b] >= 0)[0])
            d = ((q[b, v] - c[b, torch.tensor(idx[b])[v].long()]) ** 2).sum(-1)
            loss = loss + g[b, k] * d.sum() + g[b, 2 + k] * torch.sqrt(d[d > 0]).sum()
    loss.backward()
    return x.grad.numpy(), y.grad.numpy()


def check_grad(got_x, got_y, xh, yh, ixy, iyx, gs):
    ref = reference_grad(xh, yh, ixy, iyx, gs)
    auto = autograd_grad(xh, yh, ixy, iyx, gs)
    for name, got, (want, mag, cnt), a in zip("xy", (got_x, got_y), ref, auto):
        assert np.all(np.abs(a - want) <= 1e-12 * mag + 1e-300), "reference and autograd disagree on grad_" + name
        got = got.astype(np.float64)
        assert np.all(np.isfinite(got))
        bound = (cnt[..., None] + 16) * U * mag
        err = np.abs(got - want)
        worst = np.max(err / np.maximum(bound, 1e-300))
        print("grad_%s: worst error / bound %.3f, most sources %d" % (name, worst, cnt.max()))
        assert np.all(err <= bound), "grad_%s: %d of %d elements beyond (k + 16) 2^-24 sum |t|" % (
            name, int((err > bound).sum()), err.size)


@pytest.mark.parametrize("pattern", GRAD_SUMS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_gradients_match_float64_with_chamfer_nn_indices(cuda, case, pattern):
    r = reference(*case, cuda)
    gs = grad_sums_of(pattern, case[1][0])
    sums, gx, gy = run_loss(r["x"], r["y"], None, None, dev(gs, cuda))
    assert np.array_equal(bits(sums), bits(r["sums"]))
    check_grad(gx.cpu().numpy(), gy.cpu().numpy(), r["xh"], r["yh"], r["ixy"], r["iyx"], gs)


RAGGED_SHAPES = [(5, 5, 1030), (5, 1025, 7), (5, 2051, 2048)]


def ragged_lengths(n1, n2, which):
    if which == "edges":                                         # {0, 1, full, n + 5, -3} mixed
        return [0, 1, n1, n1 + 5, -3], [1, n2 + 5, n2, -3, n2]
    return [n1 // 2 + 1, 1, n1, min(3, n1), n1 - 1], [n2 - 1, n2 // 3 + 1, min(2, n2), n2, 1]


@pytest.mark.parametrize("which", ("edges", "inner"))
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_loss_values_match_calc_cd(cuda, shape, which):
    """calc_cd_fused against calc_cd (parent code), dense and ragged, rtol 1e-5."""
    xh, yh = make("uniform", shape)
    out, gt = dev(xh, cuda), dev(yh, cuda)
    cases = [(None, None)]
    lo, lg = ragged_lengths(shape[1], shape[2], which)
    cases.append((torch.tensor(np.clip(lo, 0, shape[1])), torch.tensor(np.clip(lg, 0, shape[2]))))   # calc_cd's range
    cases.append((None, cases[1][1]))
    for lo, lg in cases:
        want_p, want_t = calc_cd(out, gt, output_lengths=lo, gt_lengths=lg)
        got_p, got_t = calc_cd_fused(out, gt, output_lengths=lo, gt_lengths=lg)
        assert got_p.shape == got_t.shape == (shape[0],)
        for got, want in ((got_p, want_p), (got_t, want_t)):
            got, want = got.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
            print("calc_cd_fused %s want %s" % (got, want))
            assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want))


def test_loss_values_match_calc_cd_on_the_dense_cases(cuda):
    for case in CASES:
        r = reference(*case, cuda)
        want_p, want_t = calc_cd(r["x"], r["y"])
        got_p, got_t = calc_cd_fused(r["x"], r["y"])
        for got, want in ((got_p, want_p), (got_t, want_t)):
            got, want = got.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), case


def test_coincident_points_give_a_zero_sqrt_term_not_nan(cuda):
    # x == y: every pair coincides; with a non-zero sqrt coefficient every gradient is finite and exactly 0
    for case in (("equal", (2, 1, 1)), ("equal", (1, 4100, 4100))):
        r = reference(*case, cuda)
        for pattern in GRAD_SUMS:
            _, gx, gy = run_loss(r["x"], r["y"], None, None, dev(grad_sums_of(pattern, case[1][0]), cuda))
            for g in (gx, gy):
                g = g.cpu().numpy()
                assert np.all(np.isfinite(g)) and np.all(g == 0.0), (case, pattern)
    # the torch composition is NaN there: what the contract departs from
    xr = reference("equal", (2, 1, 1), cuda)["x"].clone().requires_grad_()
    calc_cd(xr, xr.detach().clone())[0].sum().backward()
    assert torch.isnan(xr.grad).any()
    # one planted coincident pair in a random cloud: its sqrt term is 0, everything else as in the gradient test
    xh, yh = make("uniform", (2, 1025, 1030))
    yh[0, 3] = xh[0, 5]
    yh[1, 1029] = xh[1, 1024]
    x, y = dev(xh, cuda), dev(yh, cuda)
    dxy, ixy, dyx, iyx = (t.cpu().numpy() for t in _ext.chamfer_nn(x, y))
    assert dxy[0, 5] == 0 and ixy[0, 5] == 3 and dyx[1, 1029] == 0 and iyx[1, 1029] == 1024
    for pattern in GRAD_SUMS:
        gs = grad_sums_of(pattern, 2, seed=7)
        _, gx, gy = run_loss(x, y, None, None, dev(gs, cuda))
        check_grad(gx.cpu().numpy(), gy.cpu().numpy(), xh, yh, ixy, iyx, gs)


@pytest.mark.parametrize("which", ("edges", "inner"))
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_ragged_pairs_get_the_bits_of_the_dense_call_on_the_slices(cuda, shape, which):
    B, n1, n2 = shape
    xh, yh = make("uniform", shape)
    l1, l2 = ragged_lengths(n1, n2, which)
    e1, e2 = eff(l1, n1), eff(l2, n2)
    for b in range(B):                                           # NaN in every padded row
        xh[b, e1[b]:] = np.nan
        yh[b, e2[b]:] = np.nan
    x, y = dev(xh, cuda), dev(yh, cuda)
    lx, ly = dev(l1, cuda, torch.int64), dev(l2, cuda, torch.int64)
    gs = dev(grad_sums_of("random", B, seed=3), cuda)
    sums, gx, gy = run_loss(x, y, lx, ly, gs)
    _, ix, iy = _ext._chamfer_loss_forward(x, y, lx, ly, True)
    dxy, ixy, dyx, iyx = (t.cpu().numpy() for t in _ext.chamfer_nn(x, y, lx, ly))
    sums, gx, gy, ix, iy = (t.cpu().numpy() for t in (sums, gx, gy, ix, iy))
    for b in range(B):
        a, c = int(e1[b]), int(e2[b])
        vx = np.arange(n1) < (a if c > 0 else 0)
        vy = np.arange(n2) < (c if a > 0 else 0)
        # indices: chamfer_nn's on the valid queries, -1 where it pads
        assert np.array_equal(ix[b][vx], ixy[b][vx]) and np.all(ix[b][~vx] == -1)
        assert np.array_equal(iy[b][vy], iyx[b][vy]) and np.all(iy[b][~vy] == -1)
        check_sums(sums[b], dxy[b], dyx[b], vx, vy)
        # padded rows and rows of a pair with an empty side: +0.0f
        assert not bits(gx[b][~vx]).any() and not bits(gy[b][~vy]).any()
        if a == 0 or c == 0:
            assert not bits(sums[b]).any()
            continue
        ds, dgx, dgy = run_loss(x[b:b + 1, :a].contiguous(), y[b:b + 1, :c].contiguous(), None, None, gs[b:b + 1])
        assert np.array_equal(bits(ds)[0], bits(sums[b]))
        assert np.array_equal(bits(dgx)[0], bits(gx[b, :a])) and np.array_equal(bits(dgy)[0], bits(gy[b, :c]))
    # full lengths are the call without lengths
    xh, yh = make("uniform", shape)
    x, y = dev(xh, cuda), dev(yh, cuda)
    full = run_loss(x, y, dev([n1] * B, cuda, torch.int64), dev([n2] * B, cuda, torch.int64), gs)
    one_sided = run_loss(x, y, None, dev([n2 + 5] * B, cuda, torch.int64), gs)
    none = run_loss(x, y, None, None, gs)
    for f, o, n in zip(full, one_sided, none):
        assert np.array_equal(bits(f), bits(n)) and np.array_equal(bits(o), bits(n))


def test_three_runs_give_the_same_bits(cuda):
    for case in (("same_y", (2, 2051, 2048)), ("uniform", (2, 2051, 2048))):
        r = reference(*case, cuda)
        gs = dev(grad_sums_of("random", 2), cuda)
        runs = [[bits(t) for t in run_loss(r["x"], r["y"], None, None, gs)] for _ in range(3)]
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert np.array_equal(a, b), case


def test_forward_and_backward_replay_from_a_graph(cuda):
    """Captured once on a side stream; replayed after the inputs AND the device lengths were overwritten in place."""
    B, n1, n2 = 3, 1100, 1030
    xh, yh = make("uniform", (B, n1, n2))
    x, y = dev(xh, cuda).requires_grad_(), dev(yh, cuda).requires_grad_()
    lx, ly = dev([n1, 700, 3], cuda, torch.int64), dev([n2, 1, 1030], cuda, torch.int64)
    gs = dev(grad_sums_of("random", B), cuda)

    def run():
        sums = _ext.chamfer_loss_sums(x, y, lx, ly)
        return (sums,) + torch.autograd.grad(sums, (x, y), gs)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                    # warm the allocator on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    x2h, y2h = make("uniform", (B, n1, n2 + 1))
    with torch.no_grad():
        x.copy_(dev(x2h, cuda))
        y.copy_(dev(y2h[:, :n2], cuda))
        lx.copy_(dev([5, n1 + 9, 1100], cuda, torch.int64))
        ly.copy_(dev([n2, 1000, 0], cuda, torch.int64))
        gs.copy_(dev(grad_sums_of("random", B, seed=5), cuda))
    for t in captured:
        t.detach().fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [bits(t) for t in captured]
    eager = [bits(t) for t in run()]
    for a, b in zip(replayed, eager):
        assert np.array_equal(a, b)
    assert not bits(captured[0][2]).any()                        # the pair whose y side became empty


def test_module_reductions_weights_and_single_backward(cuda):
    xh, yh = make("uniform", (3, 300, 257))
    out, gt = dev(xh, cuda).requires_grad_(), dev(yh, cuda)
    lo, lg = dev([300, 17, 0], cuda, torch.int64), dev([257, 257, 40], cuda, torch.int64)
    w = dev(np.array([0.5, 2.0, 1.25], np.float32), cuda)
    for lengths in ((None, None), (lo, lg)):
        cd_p, cd_t = (t.detach() for t in calc_cd_fused(out, gt, *lengths))
        for loss_type, v in (("cd_t", cd_t), ("cd_p", cd_p)):
            for weights in (None, w):
                vw = v if weights is None else v * weights
                want = {None: vw, "sum": vw.sum(), "mean": vw.sum() / (3 if weights is None else weights.sum())}
                for reduction, expect in want.items():
                    got = ChamferLoss(loss_type, reduction)(out, gt, *lengths, weights=weights)
                    assert got.requires_grad and got.shape == expect.shape
                    assert torch.allclose(got.detach(), expect, rtol=1e-6, atol=0), (loss_type, reduction)
    with pytest.raises(ValueError, match="negative"):
        ChamferLoss()(out, gt, weights=-w)
    # the gradient reaches `output` and the graph is used up by one backward
    loss = ChamferLoss("cd_p", "mean")(out, gt, lo, lg, weights=w)
    loss.backward()
    assert out.grad is not None and torch.isfinite(out.grad).all() and not bits(out.grad[2]).any()
    with pytest.raises(RuntimeError):
        loss.backward()
    # the training line
    out.grad = None
    calc_cd_fused(out, gt)[1].mean().backward()
    assert torch.isfinite(out.grad).all() and out.grad.abs().sum() > 0
