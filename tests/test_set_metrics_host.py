"""Set-level metrics without a GPU: lgan_mmd_cov / knn / metrics_from_matrices of pointnet2/set_metrics.py on the
matrices of tests/golden/set_metrics.npz (written by the reference's evaluation_metrics.py through
tests/golden/make_set_metrics_golden.py) against the outputs recorded there, a hand-made case with a known answer, and
the argument validation of pdr_chamfer_pairwise, which is decided on the host before any launch.

Counts, coverage and the accuracies are ratios of small integers computed by the same torch expressions on the same
float32 matrices: they must be EXACT.  The means (lgan_mmd, lgan_mmd_smp) are float32 sums of 6 / 7 terms: rtol 1e-6.
"""
import os

import numpy as np
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2 import set_metrics as SM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_metrics.npz")
EXACT = ("tp", "fp", "fn", "tn", "precision", "recall", "acc_t", "acc_f", "acc", "lgan_cov")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def mats(gold, kind):
    return [torch.from_numpy(gold["M_%s_%s" % (t, kind)]) for t in ("rr", "rs", "ss")]


def check(result, gold, prefix):
    want = {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}
    assert want and sorted(result) == sorted(want)
    for k, v in result.items():
        got = v.detach().cpu().numpy()
        if k.split("-")[0] in EXACT or k.split("-")[-1] in EXACT:
            assert np.array_equal(got, want[k]), (prefix, k, got, want[k])
        else:
            np.testing.assert_allclose(got, want[k], rtol=1e-6, atol=0, err_msg=prefix + k)


def test_fixture_is_what_the_generator_promises(gold):
    assert gold["sample_pcs"].shape == (6, 96, 3) and gold["ref_pcs"].shape == (7, 96, 3)
    assert gold["M_rs_cd"].shape == (7, 6) and gold["M_rr_emd"].shape == (7, 7) and gold["M_ss_cd"].shape == (6, 6)
    assert float(gold["min_gap"]) >= 1e-3
    assert os.path.getsize(GOLD) < 100 * 1024


@pytest.mark.parametrize("kind", ["cd", "emd"])
def test_lgan_mmd_cov_matches_the_reference(gold, kind):
    M_rs = torch.from_numpy(gold["M_rs_" + kind])
    check(SM.lgan_mmd_cov(M_rs.t()), gold, "lgan_%s/" % kind)


@pytest.mark.parametrize("sqrt", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind", ["cd", "emd"])
def test_knn_matches_the_reference(gold, kind, k, sqrt):
    check(SM.knn(*mats(gold, kind), k, sqrt=sqrt), gold, "knn_%s_k%d_sqrt%d/" % (kind, k, int(sqrt)))


def test_metrics_from_matrices_matches_compute_all_metrics_of_the_reference(gold):
    res = SM.metrics_from_matrices(*[torch.from_numpy(gold["M_%s_%s" % (t, kind)]) for kind in ("cd", "emd")
                                     for t in ("rs", "rr", "ss")])
    keys = ["%s-%s" % (k, t) for t in ("CD", "EMD") for k in ("lgan_mmd", "lgan_cov", "lgan_mmd_smp")]
    keys += ["1-NN-%s-%s" % (t, k) for t in ("CD", "EMD") for k in ("acc_t", "acc_f", "acc")]
    assert sorted(res) == sorted(keys)
    check(res, gold, "all/")


def test_hand_made_two_plus_two_case():
    """Sets x = {x0, x1}, y = {y0, y1} on a line at 0, 1 | 10, 12 -- except that y1 sits at 1.5: distances
         x0-x1 1      y0-y1 8.5     x0-y0 10   x0-y1 1.5   x1-y0 9   x1-y1 0.5
    Nearest other element: x0 -> x1 (x), x1 -> y1 (y), y0 -> y1 (y), y1 -> x1 (x).  With x labelled 1:
    pred = [1, 0, 0, 1], label = [1, 1, 0, 0]: tp 1, fn 1, tn 1, fp 1 -> every accuracy 0.5.
    lgan_mmd_cov of Mxy (samples x, references y): nearest reference of x0 is y1 (1.5), of x1 is y1 (0.5) -> one of two
    references covered: cov 0.5, mmd_smp = 1.0; nearest sample of y0 is x1 (9), of y1 is x1 (0.5): mmd = 4.75."""
    Mxx = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
    Myy = torch.tensor([[0.0, 8.5], [8.5, 0.0]])
    Mxy = torch.tensor([[10.0, 1.5], [9.0, 0.5]])
    s = SM.knn(Mxx, Mxy, Myy, 1)
    assert [float(s[k]) for k in ("tp", "fp", "fn", "tn")] == [1.0, 1.0, 1.0, 1.0]
    assert float(s["acc"]) == 0.5
    for k in ("precision", "recall", "acc_t", "acc_f"):
        assert float(s[k]) == pytest.approx(0.5, rel=1e-6)
    # square roots keep the order: same decisions
    assert float(SM.knn(Mxx, Mxy, Myy, 1, sqrt=True)["acc"]) == 0.5
    r = SM.lgan_mmd_cov(Mxy)
    assert float(r["lgan_cov"]) == 0.5 and float(r["lgan_mmd_smp"]) == 1.0 and float(r["lgan_mmd"]) == 4.75
    # and a separable case: every element's nearest other element is of its own set
    far = torch.full((2, 2), 100.0)
    s = SM.knn(Mxx, far, Myy, 1)
    assert float(s["acc"]) == 1.0 and float(s["tp"]) == 2.0 and float(s["tn"]) == 2.0


def test_pairwise_cd_rejects_cpu_tensors():
    x = torch.rand(2, 16, 3)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        SM.pairwise_cd(x, x)
    from point_diffusion_refinement_amd.pointnet2_ops import _ext
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.chamfer_pairwise(x, x)


def test_chamfer_pairwise_validates_its_arguments_without_a_gpu():
    """pdr_chamfer_pairwise: argument errors are return codes decided on the host (nothing is launched; the pointers
    below are never dereferenced); an empty set on either side is a no-op that looks at no pointer."""
    from point_diffusion_refinement_amd import _lib
    lib = _lib.load()
    p, q, l, k = 0x1000, 0x2000, 0x3000, 0x4000
    EINVAL, OK = _lib.PDR_EINVAL, _lib.PDR_OK

    def call(x=p, y=q, lx=None, ly=None, S=3, R=5, n=64, m=32, symmetric=0, cd=0x5000):
        return lib.pdr_chamfer_pairwise(x, y, lx, ly, S, R, n, m, symmetric, cd, None)
    # negative sizes
    assert call(S=-1) == EINVAL and call(R=-1) == EINVAL and call(n=-1) == EINVAL and call(m=-1) == EINVAL
    assert call(S=0, n=-1) == EINVAL                       # ... even for an empty set
    # an empty set: nothing to do, whatever the pointers
    assert call(S=0) == OK and call(R=0) == OK and call(S=0, R=0, x=None, y=None, cd=None) == OK
    assert call(S=0, n=0, m=0) == OK
    # clouds without points next to non-empty sets
    assert call(n=0) == EINVAL and call(m=0) == EINVAL
    # missing tensors
    assert call(x=None) == EINVAL and call(y=None) == EINVAL and call(cd=None) == EINVAL
    # the self-matrix needs ONE set: same clouds, same lengths, same sizes
    sym = dict(x=p, y=p, lx=l, ly=l, S=4, R=4, n=64, m=64, symmetric=1)
    assert call(**dict(sym, y=q)) == EINVAL
    assert call(**dict(sym, ly=k)) == EINVAL and call(**dict(sym, ly=None)) == EINVAL
    assert call(**dict(sym, R=5)) == EINVAL and call(**dict(sym, m=32)) == EINVAL
    assert call(**dict(sym, S=0, R=5)) == EINVAL           # checked before the empty-set shortcut
    assert call(**dict(sym, S=0, R=0)) == OK and call(**dict(sym, lx=None, ly=None, S=0, R=0)) == OK
    assert call(**dict(sym, n=0, m=0)) == EINVAL and call(**dict(sym, cd=None)) == EINVAL
    # more pairs than a launch is given
    assert call(S=1 << 16, R=(1 << 14) + 1) == _lib.PDR_EUNSUPPORTED
