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
`y_lengths`, the rules of chamfer_distance / earth_mover_distance).  The JSD of that module (voxel-grid occupancy in
numpy) is not provided.
"""
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
