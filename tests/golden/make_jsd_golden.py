"""Generate tests/golden/jsd.npz from the REFERENCE's own JSD functions (run in the build container only:
`python tests/golden/make_jsd_golden.py`).

The reference's pointnet2/models/pvd/metrics/evaluation_metrics.py is imported as make_set_metrics_golden.py imports it
(its install_metric_standins).  The module's `from sklearn.neighbors import NearestNeighbors` is commented out, so its
entropy_of_occupancy_grid cannot run as shipped; the name is put back into the module from sklearn, which is what the
function was written against (latent_3d_points).  Recorded:

    grid/R{4,5,28}_clip{0,1}      unit_cube_grid_point_cloud's grid, flattened to (cells, 3), and cells/...
    sample_pcs (5, 200, 3), ref_pcs (6, 200, 3)    float32 clouds: cube, shell, ball and wide ones mixed
    occ/{sample,ref}/R28_clip1 | R5_clip1 | R28_clip0 / {entropy, counters}    entropy_of_occupancy_grid
    jsd, jsd_self                 jsd_between_point_cloud_sets(sample, ref) and (sample, sample), which is exactly 0
    hand/{P, Q, jsd, jsdiv}       jensen_shannon_divergence and _jsdiv on two hand-made count vectors

The generator ASSERTS, and moves on to the next seed otherwise, never relaxing any of it:
  - for every point and every grid setting above, the smallest and the second-smallest float64 squared distance to a
    kept cell differ by more than MIN_GAP = 1e-12 (sklearn pins no order among tied cells; the kernel's is "lowest
    index"): the counters are then comparable EXACTLY;
  - the counters of the numpy restatement of the kernel's rule (tests/occupancy_cases.py) equal the reference's, and
    the entropy recomputed from the restatement's per-cloud counts equals the reference's to 1e-12;
  - the share of the points of the clipped R = 28 fixture that take the slow path lies in [0.2, 0.8]: both paths run.

The archive is written with fixed member timestamps, so a rerun gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE, os.path.join(ROOT, "tests")]

import make_set_metrics_golden as MS  # noqa: E402
import occupancy_cases as OC  # noqa: E402

SEED = 0
N_POINTS = 200
SAMPLE_KINDS = ("cube", "shell", "ball", "wide", "shell")
REF_KINDS = ("shell", "cube", "ball", "wide", "cube", "shell")
SETTINGS = ((28, True), (5, True), (28, False))
MIN_GAP = 1e-12


def clouds(seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([OC.MAKERS[k](rng, 1, N_POINTS) for k in kinds]) for kinds in (SAMPLE_KINDS, REF_KINDS)]


def scipy_entropy_of(bernoulli, n):
    from scipy.stats import entropy
    return sum(entropy([g / n, 1.0 - g / n]) for g in bernoulli if g > 0) / len(bernoulli)


def try_seed(EM, seed):
    """-> the arrays to record, or a string saying which assertion the draw fails"""
    smp, ref = clouds(seed)
    out = {"sample_pcs": smp, "ref_pcs": ref, "seed": np.int64(seed)}
    for R, clip in SETTINGS:
        tag = "R%d_clip%d" % (R, int(clip))
        for name, pcs in (("sample", smp), ("ref", ref)):
            gap = min(float(OC.nearest_cells(c, R, clip, return_gap=True)[2].min()) for c in pcs)
            if not gap > MIN_GAP:
                return "%s %s: two cells within %.3e of a point" % (name, tag, gap)
            ent, counters = EM.entropy_of_occupancy_grid(pcs, R, clip)
            mine = OC.occupancy(pcs, R, clip)
            if not np.array_equal(mine["counters"], counters.astype(np.int64)):
                return "%s %s: the restatement's counters differ from the reference's" % (name, tag)
            if abs(scipy_entropy_of(mine["bernoulli"], float(len(pcs))) - ent) > 1e-12:
                return "%s %s: the restatement's entropy differs from the reference's" % (name, tag)
            if (R, clip) == (28, True) and not 0.2 <= mine["slow_share"] <= 0.8:
                return "%s %s: slow-path share %.3f" % (name, tag, mine["slow_share"])
            out["occ/%s/%s/entropy" % (name, tag)] = np.float64(ent)
            out["occ/%s/%s/counters" % (name, tag)] = counters
            out["occ/%s/%s/slow_share" % (name, tag)] = np.float64(mine["slow_share"])
    out["jsd"] = np.float64(EM.jsd_between_point_cloud_sets(smp, ref))
    out["jsd_self"] = np.float64(EM.jsd_between_point_cloud_sets(smp, smp))
    assert out["jsd_self"] == 0.0
    return out


def write_npz(path, arrays):
    """numpy's .npz layout with a fixed timestamp per member (numpy.savez stamps the current time)"""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    EM = MS.install_metric_standins()
    from sklearn.neighbors import NearestNeighbors
    EM.NearestNeighbors = NearestNeighbors
    for seed in range(SEED, SEED + 16):
        out = try_seed(EM, seed)
        if not isinstance(out, str):
            break
        print("seed %d: %s: next seed" % (seed, out))
    assert not isinstance(out, str), "no seed in [%d, %d) passes the assertions" % (SEED, SEED + 16)
    print("seed %d" % seed)
    for R in (4, 5, 28):
        for clip in (False, True):
            grid = EM.unit_cube_grid_point_cloud(R, clip)[0].reshape(-1, 3)
            out["grid/R%d_clip%d" % (R, int(clip))] = grid
            out["cells/R%d_clip%d" % (R, int(clip))] = np.int64(len(grid))
    P = np.array([4.0, 0.0, 1.0, 7.0, 0.0, 3.0, 2.0, 0.0])
    Q = np.array([1.0, 2.0, 0.0, 5.0, 0.0, 3.0, 6.0, 1.0])
    out.update({"hand/P": P, "hand/Q": Q, "hand/jsd": np.float64(EM.jensen_shannon_divergence(P, Q)),
                "hand/jsdiv": np.float64(EM._jsdiv(P, Q))})
    path = os.path.join(HERE, "jsd.npz")
    write_npz(path, out)
    print("wrote jsd.npz (%.1f KB, %d arrays); jsd %.6f, slow-path share at R = 28 clipped %.3f / %.3f"
          % (os.path.getsize(path) / 1024, len(out), out["jsd"], out["occ/sample/R28_clip1/slow_share"],
             out["occ/ref/R28_clip1/slow_share"]))


if __name__ == "__main__":
    main()
