"""Set-level evaluation metrics: all-pairs distance matrices between two SETS of clouds, and MMD / coverage / 1-NN
accuracy on top of them -- the surface of the reference's pointnet2/models/pvd/metrics/evaluation_metrics.py
(_pairwise_EMD_CD_ :45-78, knn :82-111, lgan_mmd_cov :114-126, compute_all_metrics :129-157), the module
completion_eval.py:30 puts on its import path.  Names and result keys are the reference's.

The Chamfer matrix is one launch of pdr_chamfer_pairwise (csrc/chamfer_pairs.hip): a workgroup per pair of clouds, one
float per pair, nothing per point stored.  The reference expands one cloud R times per sample, receives distances and
indices per point and reduces them with torch launches.  The EMD matrix has no kernel of its own: every pair is an
independent auction that pdr_emd_cost already runs without the match matrix, so the row-major list of pairs goes
through it in chunks of `batch_size` pairs with one workspace.

Unlike the reference the matrices stay on the device they were computed on, and clouds may be padded (`x_lengths` /
`y_lengths`, the rules of chamfer_distance / earth_mover_distance).

The JSD of that module (unit_cube_grid_point_cloud :163-181, jsd_between_point_cloud_sets :184-195,
entropy_of_occupancy_grid :198-237, jensen_shannon_divergence :240-259, _jsdiv :262-278) is here too.  Its occupancy
grid -- every point of every cloud to its nearest cell of a 28^3 grid clipped to the unit sphere, which the reference
does with a KD-tree query and two Python loops per cloud -- is one launch of pdr_occupancy_grid (csrc/occupancy.hip): a
workgroup per cloud, counts in LDS, integer atomics into the two counter arrays.  The grid is passed to the kernel as
the tables the reference's own numpy arithmetic gives (`grid_tables`), and the nearest-cell rule, tie order included,
is the one include/pdr_hip.h states.  The entropies over the <= 32 768 counters are float64 torch on the counters'
device.  The counters are additive over clouds: OccupancyGrid accumulates them over chunks of a set and over ranks
(one all_reduce(SUM) per tensor), which makes the JSD the one set-level metric that shards without a gather.
"""
import math

import numpy as np
import torch

from .. import _lib
from ..pointnet2_ops import _ext
from . import emd as _emd


def _clouds(t, name):
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3:
        raise RuntimeError("%s must be a (clouds, points, 3) tensor" % name)
    return t.to(torch.float32).contiguous()


def pairwise_cd(x, y, x_lengths=None, y_lengths=None):
    """x (S,n,3), y (R,m,3) -> (S,R) float32 on the clouds' device:
        cd[s,r] = mean_i min_j |x_s,i - y_r,j|^2 + mean_j min_i |x_s,i - y_r,j|^2
    (calc_cd's cd_t; the reference's dl.mean(1) + dr.mean(1)).  x_lengths (S,) / y_lengths (R,): integer tensors, cloud
    s is x[s, :x_lengths[s]]; a pair with an empty side gets 0.  When `y is x` and the lengths are the same object this
    is the self-matrix: only the pairs s <= r are evaluated and mirrored (the same bits as the full evaluation)."""
    symmetric = y is x and y_lengths is x_lengths
    xc = _clouds(x, "x")
    lx = _emd._lengths(x_lengths, xc, "x_lengths")
    if symmetric:
        return _ext.chamfer_pairwise(xc, xc, lx, lx, symmetric=True)
    yc = _clouds(y, "y")
    return _ext.chamfer_pairwise(xc, yc, lx, _emd._lengths(y_lengths, yc, "y_lengths"))


def pairwise_emd(x, y, batch_size, x_lengths=None, y_lengths=None):
    """x (S,n,3), y (R,m,3) -> (S,R) float32: emd[s,r] = earth_mover_distance(x_s, y_r), the approximate EMD divided by
    max(n_s, m_r).  The S * R pairs are walked in row-major order, at most `batch_size` of them per call of the fused
    cost (pdr_emd_cost, pdr_emd_cost_ragged with lengths); the workspace is allocated once, for `batch_size` pairs.  A
    pair's value depends on neither `batch_size` nor its place in a call."""
    batch_size = int(batch_size)
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    xc, yc = _clouds(x, "x"), _clouds(y, "y")
    if xc.device != yc.device:
        raise RuntimeError("all tensors must live on the same device")
    (S, n, _), (R, m, _) = xc.shape, yc.shape
    lx, ly = _emd._lengths(x_lengths, xc, "x_lengths"), _emd._lengths(y_lengths, yc, "y_lengths")
    ragged = lx is not None or ly is not None
    out = torch.empty((S * R,), dtype=torch.float32, device=xc.device)
    chunk = min(batch_size, S * R)
    if chunk == 0:
        return out.view(S, R)
    ws = torch.empty((_lib.load().pdr_emd_workspace_bytes(chunk, n, m) // 4,), dtype=torch.float32, device=xc.device)
    for p0 in range(0, S * R, chunk):
        pair = torch.arange(p0, min(p0 + chunk, S * R), device=xc.device)
        si, ri = torch.div(pair, R, rounding_mode="floor"), pair % R
        a, b = xc[si], yc[ri]
        if ragged:
            la = None if lx is None else lx[si]
            lb = None if ly is None else ly[ri]
            cost = _emd.emd_cost_fused(a, b, la, lb, workspace=ws)
            # earth_mover_distance's scaling, operation for operation (emd.py: reciprocal of max(n_b, m_b), then a product)
            out[p0:p0 + pair.numel()] = cost * torch.reciprocal(_emd._pair_denominator(a, b, la, lb))
        else:
            out[p0:p0 + pair.numel()] = _emd.emd_cost_fused(a, b, workspace=ws) / max(n, m)
    return out.view(S, R)


def pairwise_emd_cd(sample_pcs, ref_pcs, batch_size):
    """_pairwise_EMD_CD_: -> (all_cd, all_emd), both (N_sample, N_ref), in the reference's return order."""
    return pairwise_cd(sample_pcs, ref_pcs), pairwise_emd(sample_pcs, ref_pcs, batch_size)


def lgan_mmd_cov(all_dist):
    """all_dist (N_sample, N_ref) -> {'lgan_mmd': mean over references of the distance to their nearest sample,
    'lgan_cov': share of the references that are some sample's nearest reference, 'lgan_mmd_smp': mean over samples of
    the distance to their nearest reference}, 0-d tensors like all_dist."""
    n_ref = all_dist.size(1)
    smp_min, smp_arg = all_dist.min(dim=1)
    ref_min = all_dist.min(dim=0).values
    covered = smp_arg.unique().numel()
    return {
        "lgan_mmd": ref_min.mean(),
        "lgan_cov": torch.tensor(float(covered) / float(n_ref)).to(all_dist),
        "lgan_mmd_smp": smp_min.mean(),
    }


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """k-NN two-sample test on the joint (n0 + n1)^2 distance matrix [[Mxx, Mxy], [Mxy^T, Myy]], set x labelled 1: a
    column's element is predicted 1 when at least k / 2 of its k nearest OTHER elements (infinite diagonal) are of set
    x.  -> tp, fp, fn, tn, precision, recall, acc_t, acc_f (denominators + 1e-10) and acc, 0-d tensors like Mxx."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.t(), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    blocked = M + torch.diag(torch.full((n0 + n1,), float("inf")).to(Mxx))
    idx = blocked.topk(k, 0, False).indices
    count = torch.zeros(n0 + n1).to(Mxx)
    for i in range(k):
        count = count + label[idx[i]]
    pred = (count >= float(k) / 2).to(Mxx)
    tp, fp = (pred * label).sum(), (pred * (1 - label)).sum()
    fn, tn = ((1 - pred) * label).sum(), ((1 - pred) * (1 - label)).sum()
    return {
        "tp": tp, "fp": fp, "fn": fn, "tn": tn,
        "precision": tp / (tp + fp + 1e-10),
        "recall": tp / (tp + fn + 1e-10),
        "acc_t": tp / (tp + fn + 1e-10),
        "acc_f": tn / (tn + fp + 1e-10),
        "acc": (label == pred).float().mean(),
    }


def metrics_from_matrices(M_rs_cd, M_rr_cd, M_ss_cd, M_rs_emd, M_rr_emd, M_ss_emd):
    """The dictionary of compute_all_metrics from its six matrices (rs = pairwise(ref, sample), (N_ref, N_sample)):
    lgan_mmd / lgan_cov / lgan_mmd_smp of M_rs^T and the three accuracies of the 1-NN test on (M_rr, M_rs, M_ss),
    each with the suffix / infix CD and EMD."""
    results = {}
    for tag, M_rs in (("CD", M_rs_cd), ("EMD", M_rs_emd)):
        results.update({"%s-%s" % (k, tag): v for k, v in lgan_mmd_cov(M_rs.t()).items()})
    for tag, (M_rr, M_rs, M_ss) in (("CD", (M_rr_cd, M_rs_cd, M_ss_cd)), ("EMD", (M_rr_emd, M_rs_emd, M_ss_emd))):
        one_nn = knn(M_rr, M_rs, M_ss, 1, sqrt=False)
        results.update({"1-NN-%s-%s" % (tag, k): v for k, v in one_nn.items() if "acc" in k})
    return results


def compute_all_metrics(sample_pcs, ref_pcs, batch_size):
    """sample_pcs (N_sample, n, 3), ref_pcs (N_ref, m, 3) on the GPU -> {'lgan_mmd-CD', 'lgan_cov-CD',
    'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc' and the same with EMD}.  Three Chamfer launches
    (the two self-matrices evaluate half their pairs) and the three EMD matrices in chunks of `batch_size` pairs."""
    M_rs_cd, M_rs_emd = pairwise_emd_cd(ref_pcs, sample_pcs, batch_size)
    M_rr_cd, M_rr_emd = pairwise_emd_cd(ref_pcs, ref_pcs, batch_size)
    M_ss_cd, M_ss_emd = pairwise_emd_cd(sample_pcs, sample_pcs, batch_size)
    return metrics_from_matrices(M_rs_cd, M_rr_cd, M_ss_cd, M_rs_emd, M_rr_emd, M_ss_emd)


# ---- JSD between two sets of clouds (voxel-grid occupancy) -----------------------------------------------------------

def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """Centres of the cells of a resolution^3 grid in the unit cube -> (grid, spacing), bit-equal to the reference's:
    grid[i,j,k] = float32((i, j, k) * spacing - 0.5) with spacing = 1.0 / (resolution - 1) in float64, shape
    (R, R, R, 3); with clip_sphere the (kept, 3) cells whose float32 norm is <= 0.5, in ascending (i R + j) R + k."""
    resolution = int(resolution)
    spacing = 1.0 / float(resolution - 1)
    axis = (np.arange(resolution) * spacing - 0.5).astype(np.float32)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1)
    if clip_sphere:
        grid = grid.reshape(-1, 3)
        grid = grid[np.linalg.norm(grid, axis=1) <= 0.5]
    return grid, spacing


_TABLES = {}


def grid_tables(resolution, in_sphere, device):
    """The grid as pdr_occupancy_grid reads it -> (axis (R,) f32, cell_of (R,R,R) i32, cells) on `device`: the axis
    coordinates of unit_cube_grid_point_cloud and, per cell, its index among the kept cells or -1.  Built once per
    (resolution, in_sphere, device)."""
    key = (int(resolution), bool(in_sphere), torch.device(device))
    if key not in _TABLES:
        R = key[0]
        grid, _ = unit_cube_grid_point_cloud(R, False)
        keep = np.ones(R ** 3, dtype=bool)
        if key[1]:
            keep = np.linalg.norm(grid.reshape(-1, 3), axis=1) <= 0.5
        cell_of = np.full(R ** 3, -1, dtype=np.int32)
        cell_of[keep] = np.arange(int(keep.sum()), dtype=np.int32)
        _TABLES[key] = (torch.from_numpy(np.ascontiguousarray(grid[0, 0, :, 2])).to(key[2]),
                        torch.from_numpy(cell_of.reshape(R, R, R)).to(key[2]), int(keep.sum()))
    return _TABLES[key]


def _bernoulli_entropy(bernoulli, n_clouds):
    """mean over the cells of the entropy (natural logarithm) of [g / n, 1 - g / n]; cells with g = 0 add nothing"""
    p = bernoulli.to(torch.float64) / n_clouds
    return (torch.special.entr(p) + torch.special.entr(1.0 - p)).sum() / bernoulli.numel()


def _entropy2(p):
    """scipy.stats.entropy(p, base=2) of a non-negative float64 vector: normalised, 0 log 0 = 0"""
    return torch.special.entr(p / p.sum()).sum() / math.log(2.0)


def jensen_shannon_divergence(P, Q):
    """Two non-negative count vectors of equal size, tensors on any device -> 0-d float64 tensor
    H((P_ + Q_) / 2) - (H(P_) + H(Q_)) / 2 of the normalised vectors, entropies to base 2."""
    P, Q = torch.as_tensor(P).to(torch.float64), torch.as_tensor(Q).to(torch.float64)
    if bool((P < 0).any()) or bool((Q < 0).any()):
        raise ValueError('Negative values.')
    if P.shape[0] != Q.shape[0]:
        raise ValueError('Non equal size.')
    P_, Q_ = P / P.sum(), Q / Q.sum()
    return _entropy2((P_ + Q_) / 2.0) - (_entropy2(P_) + _entropy2(Q_)) / 2.0


def _jsdiv(P, Q):
    """The reference's second way to the same number: the mean of the two Kullback-Leibler divergences (base 2) from
    the mid-point distribution, each over the entries where both operands are positive."""
    P, Q = torch.as_tensor(P).to(torch.float64), torch.as_tensor(Q).to(torch.float64)

    def kldiv(a, b):
        both = (a > 0) & (b > 0)
        one = torch.ones_like(a)
        return torch.where(both, a * torch.log2(torch.where(both, a, one) / torch.where(both, b, one)),
                           torch.zeros_like(a)).sum()

    P_, Q_ = P / P.sum(), Q / Q.sum()
    M = 0.5 * (P_ + Q_)
    return 0.5 * (kldiv(P_, M) + kldiv(Q_, M))


class OccupancyGrid:
    """Occupancy counters of a set of clouds, fed in chunks: `counters` (points per cell), `bernoulli` (clouds per
    cell), `n_clouds` and `skipped` (non-finite points, which go to no cell), int64 tensors on `device`.  Everything is
    a sum over clouds, so two grids of the same shape merge by addition and a set spread over ranks needs one
    all_reduce(SUM) per tensor."""

    def __init__(self, resolution=28, in_sphere=True, device=None):
        self.resolution, self.in_sphere = int(resolution), bool(in_sphere)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not 2 <= self.resolution <= 32:
            raise ValueError("grid resolution %d outside [2, 32]" % self.resolution)
        cells = grid_tables(self.resolution, self.in_sphere, "cpu")[2]
        if cells == 0:
            raise ValueError("the %d^3 grid clipped to the unit sphere keeps no cell" % self.resolution)
        self.counters = torch.zeros((cells,), dtype=torch.int64, device=self.device)
        self.bernoulli = torch.zeros((cells,), dtype=torch.int64, device=self.device)
        self.n_clouds = torch.zeros((), dtype=torch.int64, device=self.device)
        self.skipped = torch.zeros((), dtype=torch.int64, device=self.device)

    @classmethod
    def from_counters(cls, counters, bernoulli, n_clouds, skipped=0, resolution=28, in_sphere=True):
        """A grid from existing counter tensors on any device (the CPU included): the arithmetic and the collective
        need no kernel."""
        self = cls.__new__(cls)
        self.resolution, self.in_sphere, self.device = int(resolution), bool(in_sphere), counters.device
        if counters.dim() != 1 or bernoulli.shape != counters.shape:
            raise ValueError("counters and bernoulli must be vectors of one size")
        self.counters, self.bernoulli = counters.to(torch.int64).clone(), bernoulli.to(torch.int64).clone()
        self.n_clouds = torch.as_tensor(n_clouds, device=self.device).to(torch.int64).reshape(()).clone()
        self.skipped = torch.as_tensor(skipped, device=self.device).to(torch.int64).reshape(()).clone()
        return self

    def add(self, clouds, lengths=None):
        """clouds (S, n, 3) on this grid's device (and `lengths` (S,), the rule of pairwise_cd): one launch, added in"""
        c = _clouds(clouds, "clouds")
        axis, cell_of, cells = grid_tables(self.resolution, self.in_sphere, self.device)
        cnt, ber, skp = _ext.occupancy_grid(c, axis, cell_of, cells, _emd._lengths(lengths, c, "lengths"))
        self.counters += cnt
        self.bernoulli += ber
        self.skipped += skp[0]
        self.n_clouds += c.shape[0]
        return self

    def _same_grid(self, other):
        if (self.resolution, self.in_sphere) != (other.resolution, other.in_sphere) \
                or self.counters.shape != other.counters.shape:
            raise ValueError("the two occupancy grids differ in resolution or clipping")

    def merge(self, other):
        self._same_grid(other)
        for name in ("counters", "bernoulli", "n_clouds", "skipped"):
            getattr(self, name).add_(getattr(other, name).to(self.device))
        return self

    def all_reduce(self, group=None):
        """Sum over the ranks of `group`: afterwards every rank holds the whole set's grid."""
        import torch.distributed as dist
        for name in ("counters", "bernoulli", "n_clouds", "skipped"):
            dist.all_reduce(getattr(self, name), op=dist.ReduceOp.SUM, group=group)
        return self

    def entropy(self):
        """entropy_of_occupancy_grid's first result: 0-d float64 tensor"""
        return _bernoulli_entropy(self.bernoulli, self.n_clouds)

    def jsd(self, other):
        self._same_grid(other)
        return jensen_shannon_divergence(self.counters, other.counters.to(self.counters.device))


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, lengths=None):
    """pclouds (S, n, 3) on the GPU -> (entropy, counters): the mean over the grid's cells of the entropy of the
    Bernoulli variable "some point of a cloud falls into the cell" (0-d float64 tensor) and the points per cell
    ((cells,) float64 tensor), both on the clouds' device; no host synchronisation.  S counts every cloud, empty ones
    (`lengths`) included, as len(pclouds) does in the reference."""
    grid = OccupancyGrid(grid_resolution, in_sphere, device=pclouds.device).add(pclouds, lengths)
    return grid.entropy(), grid.counters.to(torch.float64)


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28, sample_lengths=None, ref_lengths=None):
    """JSD between the occupancy distributions of two sets of clouds on the resolution^3 grid clipped to the unit
    sphere -> Python float (one synchronisation, at the end).  numpy arrays are copied to the current device; tensors
    must be on a GPU.  ValueError when a point inside its length is not finite."""
    grids = []
    for pcs, lengths in ((sample_pcs, sample_lengths), (ref_pcs, ref_lengths)):
        if isinstance(pcs, np.ndarray):
            pcs = torch.from_numpy(np.ascontiguousarray(pcs, dtype=np.float32)).cuda()
        grids.append(OccupancyGrid(resolution, True, device=pcs.device).add(pcs, lengths))
    value, skipped = grids[0].jsd(grids[1]), grids[0].skipped + grids[1].skipped.to(grids[0].device)
    if int(skipped) != 0:
        raise ValueError("%d points with a non-finite coordinate" % int(skipped))
    return float(value)
