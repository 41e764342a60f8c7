"""Generate tests/golden/set_metrics.npz from the REFERENCE's own set-level metrics (run in the build container only:
`python tests/golden/make_set_metrics_golden.py`).

The reference's pointnet2/models/pvd/metrics/evaluation_metrics.py is imported through tests/golden/ref_import.py
(unchanged: `.cuda()` is the identity there) with its three native / third-party dependencies replaced by stand-ins
backed by the CPU oracle:

    metrics.PyTorchEMD.emd                               -> oracle approxmatch / matchcost, cost / n as PyTorchEMD/emd.py:45
    metrics.ChamferDistancePytorch.chamfer3D.dist_chamfer_3D, .fscore -> oracle knn (K = 1), both directions
    tqdm                                                 -> the bare iterator

and its _pairwise_EMD_CD_, lgan_mmd_cov, knn and compute_all_metrics are run on 6 sample and 7 reference clouds of 96
points.  Every cloud has the same size, so the reference's `/ n` and this library's `/ max(n, m)` agree.

The discrete results (coverage, the 1-NN accuracies) are decided by argmins over the matrices.  They are comparable
between this fp32 oracle and a GPU kernel with another summation order only if no argmin is a near-tie, so the
generator ASSERTS that, for CD and for EMD, in every row and column of M_rs and in every column of the joint
(S + R)^2 1-NN matrix the smallest and the second-smallest entry are at least MIN_GAP apart (relative).  A draw that
fails is discarded and the next seed is tried (seed 0 has an EMD near-tie of 8.6e-4 in the 1-NN matrix, seed 1 a CD
near-tie of 7.6e-4 in M_rs; seed 2 is clean: smallest gap 1.0e-2); the seed used is stored in the file.  The gap is
not negotiable.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]

import ref_import as R  # noqa: E402

SEED = 0
N_SAMPLE, N_REF, N_POINTS = 6, 7, 96
BATCH_SIZE = 4          # the reference's ref batch: 7 references go as 4 + 3
MIN_GAP = 1e-3
O = R.O


def clouds(seed=SEED):
    """uniform in [-1, 1]^3 times a per-cloud, per-axis factor from [0.5, 1.5]; samples first, then references"""
    rng = np.random.default_rng(seed)
    out = []
    for count in (N_SAMPLE, N_REF):
        pts = rng.uniform(-1.0, 1.0, size=(count, N_POINTS, 3))
        out.append((pts * rng.uniform(0.5, 1.5, size=(count, 1, 3))).astype(np.float32))
    return out


def install_metric_standins():
    R.install()

    def earth_mover_distance(xyz1, xyz2, transpose=True):
        if transpose:
            xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
        a, b = R._np(xyz1), R._np(xyz2)
        return R._t(O.matchcost(a, b, O.approxmatch(a, b))) / a.shape[1]

    class chamfer_3DDist:
        def __call__(self, a, b):
            d1, i1, d2, i2 = O.chamfer(R._np(a), R._np(b))
            return R._t(d1), R._t(d2), R._t(i1.astype(np.int32)), R._t(i2.astype(np.int32))

    def fscore(dist1, dist2, threshold=0.001):
        raise NotImplementedError("the set-level metrics do not use the F-score")

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    module("metrics.PyTorchEMD")
    module("metrics.PyTorchEMD.emd", earth_mover_distance=earth_mover_distance)
    module("metrics.ChamferDistancePytorch")
    module("metrics.ChamferDistancePytorch.chamfer3D")
    module("metrics.ChamferDistancePytorch.chamfer3D.dist_chamfer_3D", chamfer_3DDist=chamfer_3DDist)
    module("metrics.ChamferDistancePytorch.fscore", fscore=fscore)
    module("tqdm", tqdm=lambda it, *a, **k: it)
    sys.path.insert(0, os.path.join(R.REF, "pointnet2", "models", "pvd"))
    import metrics.evaluation_metrics as EM
    return EM


def min_gap(M, dims):
    """smallest relative distance between the least and the second-least entry along each of `dims`"""
    M = np.asarray(M, dtype=np.float64)
    gap = np.inf
    for d in dims:
        two = np.sort(M, axis=d).take([0, 1], axis=d)
        a, b = two.take(0, axis=d), two.take(1, axis=d)
        gap = min(gap, float(((b - a) / b).min()))
    return gap


def joint(M_rr, M_rs, M_ss):
    J = np.block([[M_rr, M_rs], [M_rs.T, M_ss]]).astype(np.float64)
    np.fill_diagonal(J, np.inf)
    return J


def matrices(EM, smp, ref):
    """the three CD and the three EMD matrices of compute_all_metrics, and their smallest argmin gap"""
    ts, tr = torch.from_numpy(smp), torch.from_numpy(ref)
    M = {}
    for tag, (a, b) in (("rs", (tr, ts)), ("rr", (tr, tr)), ("ss", (ts, ts))):
        cd, emd = EM._pairwise_EMD_CD_(a, b, BATCH_SIZE)
        M[tag + "_cd"], M[tag + "_emd"] = cd.numpy(), emd.numpy()
    gap = np.inf
    for kind in ("cd", "emd"):
        g_rs = min_gap(M["rs_" + kind], (0, 1))
        g_nn = min_gap(joint(M["rr_" + kind], M["rs_" + kind], M["ss_" + kind]), (0,))
        print("  %s: minimum argmin gap %.3e in M_rs, %.3e in the 1-NN matrix" % (kind.upper(), g_rs, g_nn))
        gap = min(gap, g_rs, g_nn)
    return M, gap


def main():
    EM = install_metric_standins()
    # the seed is the only thing that moves when a draw has a near-tie; MIN_GAP stays
    for seed in range(SEED, SEED + 16):
        print("seed %d" % seed)
        smp, ref = clouds(seed)
        M, gap = matrices(EM, smp, ref)
        if gap >= MIN_GAP:
            break
        print("  near-tie (gap %.3e < %.0e): next seed" % (gap, MIN_GAP))
    assert gap >= MIN_GAP, "no seed in [%d, %d) is free of near-ties" % (SEED, SEED + 16)
    ts, tr = torch.from_numpy(smp), torch.from_numpy(ref)
    out = {"sample_pcs": smp, "ref_pcs": ref, "batch_size": np.int64(BATCH_SIZE), "seed": np.int64(seed),
           "min_gap": np.float64(gap)}
    for kind in ("cd", "emd"):
        for tag in ("rs", "rr", "ss"):
            out["M_%s_%s" % (tag, kind)] = M["%s_%s" % (tag, kind)]
        for k, v in EM.lgan_mmd_cov(torch.from_numpy(M["rs_" + kind]).t()).items():
            out["lgan_%s/%s" % (kind, k)] = v.numpy()
        for k in (1, 3):
            for sqrt in (False, True):
                res = EM.knn(*(torch.from_numpy(M[t + "_" + kind]) for t in ("rr", "rs", "ss")), k, sqrt=sqrt)
                for name, v in res.items():
                    out["knn_%s_k%d_sqrt%d/%s" % (kind, k, int(sqrt), name)] = v.numpy()
    for k, v in EM.compute_all_metrics(ts, tr, BATCH_SIZE).items():
        out["all/" + k] = v.numpy()
    path = os.path.join(HERE, "set_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote set_metrics.npz (%.1f KB, %d arrays)" % (os.path.getsize(path) / 1024, len(out)))


if __name__ == "__main__":
    main()
