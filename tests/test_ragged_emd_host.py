"""Length-aware EMD entry points and ragged F-score / Chamfer metrics without a GPU.

pdr_approxmatch_ragged / pdr_emd_cost_ragged / pdr_matchcost_ragged / pdr_matchcost_grad_ragged: declared, exported and
bound with the dense entries' arguments plus the two length pointers, and validated like the dense entries (on the
host, before anything is launched; the lengths are never read there, so NULL lengths pass like any device pointer).

fscore / calc_cd with lengths run on CPU tensors over the oracle (tests/oracle_backend.py): a padded batch gives what
the dense functions give sample by sample on the slices, padded points do not count, an empty cloud gives zeros, and
absent lengths give today's expressions bit for bit."""
import ctypes
import os
import re

import numpy as np
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2.chamfer_loss_new import Chamfer_F1, calc_cd, chamfer_distance, fscore
from tests.oracle_backend import oracle_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000                                          # (never dereferenced: every call below returns before a launch)
EINVAL, OK = _lib.PDR_EINVAL, _lib.PDR_OK
PAIRS = {"pdr_approxmatch_ragged": "pdr_approxmatch", "pdr_emd_cost_ragged": "pdr_emd_cost",
         "pdr_matchcost_ragged": "pdr_matchcost", "pdr_matchcost_grad_ragged": "pdr_matchcost_grad"}


def _declared_arity():
    """name -> number of parameters of every function include/pdr_hip.h declares"""
    text = open(os.path.join(ROOT, "include", "pdr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: len(args.split(",")) for name, args in re.findall(r"\b(pdr_[a-z0-9_]+)\s*\(([^)]*)\)", text)}


def test_ragged_emd_symbols_are_declared_exported_and_bound():
    declared = _declared_arity()
    raw = ctypes.CDLL(os.path.join(ROOT, "point_diffusion_refinement_amd", "libpdr_hip.so"))
    lib = _lib.load()
    for name, dense in PAIRS.items():
        assert name in declared, "include/pdr_hip.h does not declare %s" % name
        assert hasattr(raw, name), "libpdr_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        assert len(getattr(lib, name).argtypes) == declared[name] == declared[dense] + 2
        assert len(getattr(lib, name).argtypes) == len(getattr(lib, dense).argtypes) + 2
    assert lib.pdr_version() == 200
    history = open(os.path.join(ROOT, "include", "pdr_hip.h")).read().split("int pdr_version(void);")[0]
    assert all(name in history for name in PAIRS), "the 0.2.0 history line names the new entries"


def _agree(ragged, dense):
    """return code with device lengths, NULL lengths, one of each, and of the dense entry: all agree"""
    rc = [ragged(l1, l2) for l1, l2 in ((P, P), (None, None), (P, None), (None, P))] + [dense()]
    assert len(set(rc)) == 1, rc
    return rc[0]


def test_approxmatch_and_emd_cost_ragged_validate_like_the_dense_entries():
    lib = _lib.load()
    for rname, dname in (("pdr_approxmatch_ragged", "pdr_approxmatch"), ("pdr_emd_cost_ragged", "pdr_emd_cost")):
        rf, df = getattr(lib, rname), getattr(lib, dname)

        def both(x=P, y=P, B=2, n=64, m=70, out=P, temp=P):
            return _agree(lambda l1, l2: rf(x, y, l1, l2, B, n, m, out, temp, None),
                          lambda: df(x, y, B, n, m, out, temp, None))

        for name in ("x", "y", "out", "temp"):
            assert both(**{name: None}) == EINVAL, (rname, name)
        assert both(B=-1) == EINVAL and both(n=0) == EINVAL and both(m=0) == EINVAL and both(n=-3) == EINVAL
        assert both(B=0) == OK and both(B=0, x=None, out=None) == OK          # empty batch: a no-op
        assert both(B=0, n=0) == EINVAL                                        # sizes are checked first


def test_matchcost_ragged_validates_like_the_dense_entry():
    lib = _lib.load()

    def both(x=P, y=P, match=P, B=2, n=64, m=70, cost=P, temp=P):
        return _agree(lambda l1, l2: lib.pdr_matchcost_ragged(x, y, l1, l2, match, B, n, m, cost, temp, None),
                      lambda: lib.pdr_matchcost(x, y, match, B, n, m, cost, temp, None))

    for name in ("x", "y", "match", "cost", "temp"):
        assert both(**{name: None}) == EINVAL, name
    assert both(B=-1) == EINVAL and both(n=0) == EINVAL and both(m=-1) == EINVAL
    assert both(B=0) == OK and both(B=0, match=None) == OK


def test_matchcost_grad_ragged_validates_like_the_dense_entry():
    lib = _lib.load()

    def both(g=P, x=P, y=P, match=P, B=2, n=64, m=70, g1=P, g2=P):
        return _agree(lambda l1, l2: lib.pdr_matchcost_grad_ragged(g, x, y, l1, l2, match, B, n, m, g1, g2, None),
                      lambda: lib.pdr_matchcost_grad(g, x, y, match, B, n, m, g1, g2, None))

    for name in ("g", "x", "y", "match", "g1", "g2"):
        assert both(**{name: None}) == EINVAL, name
    assert both(B=-1) == EINVAL and both(n=0) == EINVAL and both(m=0) == EINVAL
    assert both(B=0) == OK and both(B=0, g=None, g2=None) == OK


# ------------------------------------------------------------------ F-score / Chamfer metrics on a padded batch
def test_fscore_counts_valid_points_only():
    """Hand-made distance maps: a padded entry is 0 (what chamfer_distance leaves there) and would be a hit."""
    thr = 0.5
    d1 = torch.tensor([[0.1, 0.9, 0.2, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.9, 0.9, 0.1, 0.1, 0.7]])
    d2 = torch.tensor([[0.9, 0.1, 0.0, 0.0], [0.1, 0.1, 0.0, 0.0], [0.1, 0.9, 0.9, 0.9]])
    l1, l2 = torch.tensor([3, 0, 5]), torch.tensor([2, 2, 4])
    f, p1, p2 = fscore(d1, d2, thr, lengths1=l1, lengths2=l2)
    want1 = np.array([2 / 3, 0.0, 2 / 5], np.float32)                  # without lengths: 4/5, 1, 2/5
    want2 = np.array([1 / 2, 1.0, 1 / 4], np.float32)                  #                  3/4, 1, 1/4
    np.testing.assert_allclose(p1.numpy(), want1, rtol=1e-6)
    np.testing.assert_allclose(p2.numpy(), want2, rtol=1e-6)
    wantf = np.where(want1 + want2 > 0, 2 * want1 * want2 / np.maximum(want1 + want2, 1e-30), 0)
    np.testing.assert_allclose(f.numpy(), wantf, rtol=1e-6)
    assert f[1] == 0 and p1[1] == 0                                    # the empty cloud: 0, not NaN
    # one-sided lengths: the other map is averaged over its whole width
    _, q1, q2 = fscore(d1, d2, thr, lengths1=l1)
    assert torch.equal(q1, p1) and torch.equal(q2, (d2 < thr).float().mean(1))
    # garbage beyond the length is not read into the result
    d1n = d1.clone()
    d1n[0, 3:], d1n[1, :] = float("nan"), float("nan")
    fn, _, _ = fscore(d1n, d2, thr, lengths1=l1, lengths2=l2)
    assert torch.equal(fn, f)


def _padded_batch():
    rr = np.random.default_rng(11)
    out = torch.from_numpy(rr.uniform(-0.5, 0.5, (3, 48, 3)).astype(np.float32))
    gt = torch.from_numpy(rr.uniform(-0.5, 0.5, (3, 60, 3)).astype(np.float32))
    lo, lg = [48, 20, 33], [60, 0, 41]
    for b in range(3):
        out[b, lo[b]:] = 50.0                                           # padding: far away, would change every metric
        gt[b, lg[b]:] = -50.0
    return out, gt, lo, lg


def test_calc_cd_with_lengths_is_the_dense_calc_cd_on_the_slices():
    out, gt, lo, lg = _padded_batch()
    thr = 0.01
    with oracle_ops():
        cd_p, cd_t, f1 = calc_cd(out, gt, calc_f1=True, f1_threshold=thr, output_lengths=torch.tensor(lo),
                                 gt_lengths=torch.tensor(lg))
        m_p, m_t, m_f = Chamfer_F1(f1_threshold=thr)(out, gt, torch.tensor(lo), torch.tensor(lg))
        two = calc_cd(out, gt, output_lengths=torch.tensor(lo), gt_lengths=torch.tensor(lg))
        want = np.zeros((3, 3), np.float32)
        for b in range(3):
            if lo[b] and lg[b]:
                want[b] = [float(v) for v in calc_cd(out[b:b + 1, :lo[b]], gt[b:b + 1, :lg[b]], calc_f1=True,
                                                     f1_threshold=thr)]
        # gt alone padded (what evaluate_batch passes): the generated cloud counts in full
        g_p, g_t, g_f = calc_cd(out[:, :20].contiguous(), gt, calc_f1=True, f1_threshold=thr,
                                gt_lengths=torch.tensor(lg))
        want_g = np.zeros((3, 3), np.float32)
        for b in (0, 2):
            want_g[b] = [float(v) for v in calc_cd(out[b:b + 1, :20], gt[b:b + 1, :lg[b]], calc_f1=True,
                                                   f1_threshold=thr)]
    assert 0 < want[0, 2] < 1 and 0 < want[2, 2] < 1, "the threshold separates nothing: %r" % want[:, 2]
    got = torch.stack([cd_p, cd_t, f1], 1).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert not got[1].any()                                             # the sample with an empty cloud: zeros
    assert torch.equal(m_p, cd_p) and torch.equal(m_t, cd_t) and torch.equal(m_f, f1)
    assert torch.equal(two[0], cd_p) and torch.equal(two[1], cd_t) and len(two) == 2
    np.testing.assert_allclose(torch.stack([g_p, g_t, g_f], 1).numpy(), want_g, rtol=1e-6)


def test_absent_lengths_give_todays_expressions_exactly():
    out, gt, _, _ = _padded_batch()
    thr = 0.01
    with oracle_ops():
        d1, d2, _ = chamfer_distance(gt, out, batch_reduction=None, point_reduction=None)
        cd_p, cd_t, f1 = calc_cd(out, gt, calc_f1=True, f1_threshold=thr, output_lengths=None, gt_lengths=None)
        m = Chamfer_F1(f1_threshold=thr)(out, gt, lengths1=None, lengths2=None)
    assert torch.equal(cd_p, (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2)
    assert torch.equal(cd_t, d1.mean(1) + d2.mean(1))
    p1, p2 = (d1 < thr).float().mean(1), (d2 < thr).float().mean(1)
    f, q1, q2 = fscore(d1, d2, thr, lengths1=None, lengths2=None)
    want_f = 2 * p1 * p2 / (p1 + p2)
    want_f[torch.isnan(want_f)] = 0                                     # (sample 1: the padding is far away, no hit)
    assert torch.equal(q1, p1) and torch.equal(q2, p2) and torch.equal(f, want_f)
    assert torch.equal(f1, f) and all(torch.equal(a, b) for a, b in zip(m, (cd_p, cd_t, f1)))
