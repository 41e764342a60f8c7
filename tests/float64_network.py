"""TEST INFRASTRUCTURE: a float64 evaluation of PointNet2CloudCondition with the fp32 paths' geometry, and recorders
that pair every block of the torch module with the fused block built from it.

Every discrete decision of the network (FPS picks, ball membership and counts, kNN sets) depends on coordinates only,
and the coordinates of every level are gathers of the fp32 inputs.  A `.double()` copy of the module whose index ops
see the fp32 cast of their coordinate arguments therefore takes exactly the decisions the fp32 paths take; everything
that moves features runs in float64.  The rest of the graph (convs, GroupNorm, ReLU, masked softmax, max-pool) is
continuous, so what separates an fp32 evaluation from this one is rounding -- known per block.

    float64_ops(index_ops)   context: `pointnet2_ops._ext` swapped for the above ("oracle" = CPU oracle indices,
                             "hip" = the real `_ext` index kernels), step embedding pinned to its f32 specification
    float64_model(net)       deep copy in double, eval mode
    record_modules(net)      forward hooks -> per call {module name: (B, n, C) tensor} (+ "eps")
    record_fused(fused)      the same for FusedCloudConditionNet, keyed by the name of the module a block was built from
    log_indices()            the integer outputs of the index ops that are installed when it is entered

A whole training step (forward, loss, backward) is evaluated the same way.  `float64_ops` also covers the backward
entries the autograd Functions of pointnet2_utils.py call, so `loss.backward()` runs through the swap.  Two kinds of
decision are left once the geometry is shared, and a gradient is only comparable when they are shared too:

    relu_tape("record")        the ReLU masks of a forward, one per site in call order -- the fused entries that hold a
    relu_tape("replay", tape)  ReLU record the same sites as the composition -- and their replay in another
                               evaluation (the float64 model under the masks of the fp32 run it is the reference of)
    chamfer_tape("record", nn=..)   the nearest-neighbour assignment of every Chamfer term of a loss (the stage-two
    chamfer_tape("replay", tape)    step: it depends on the network's output) and its replay by gathers in float64;
                               chamfer_tape_honesty: a taped index differs from float64's own argmin only where the
                               output error can move the two distances past each other
    record_max_gaps(net)       the two max-over-points of the global PointNet are NOT pinned; this measures how far
                               each of them is from a tie, so a test can assert that no evaluation can pick another point
    coordinate_leaf(net, x)    a leaf in place of the level-0 coordinates (forward() cuts the graph at its input)
    count_ext_calls(net)       counters, block attribution and result editing for the ten fused `_ext` entries
    block_of(parameter name)   the top-level block a parameter belongs to
"""
import contextlib
import copy
import inspect

import numpy as np
import torch

from point_diffusion_refinement_amd.pointnet2 import fused_network as FN
from point_diffusion_refinement_amd.pointnet2.models import pointnet2_with_pcld_condition as _model
from point_diffusion_refinement_amd.pointnet2_ops import _ext

INDEX_OPS = ("furthest_point_sampling", "ball_query", "knn_points", "three_nn")
# switches and shape predicates of `_ext` that launch nothing: left in place
_PASS_THROUGH = {"set_deterministic", "is_deterministic", "set_fused_attention_pool", "is_fused_attention_pool",
                 "set_fused_group_norm", "is_fused_group_norm", "attention_pool_supported", "group_norm_act_supported",
                 "set_fused_grouping", "is_fused_grouping", "set_fused_knn_grouping", "is_fused_knn_grouping",
                 "set_fused_score_norm", "is_fused_score_norm"}
# the five one-op switches of the module path, and the `_ext` entries (forward, backward) each of them reaches
SWITCHES = ("attention_pool", "group_norm", "grouping", "knn_grouping", "score_norm")
FUSED_ENTRIES = {"attention_pool": ("attention_pool", "attention_pool_grad"),
                 "group_norm": ("group_norm_act", "group_norm_act_grad"),
                 "grouping": ("query_group", "query_group_grad"),
                 "knn_grouping": ("knn_group_cf", "knn_group_cf_grad"),
                 "score_norm": ("relu_group_norm", "relu_group_norm_grad")}
# the children of PointNet2CloudCondition whose outputs are recorded, and the fused network's lists built from them
BLOCK_LISTS = (("SA_modules", "sa"), ("FP_modules", "fp"), ("encoder_feature_map", "enc_map"),
               ("decoder_feature_map", "dec_map"), ("SA_modules_condition", "cond_sa"),
               ("FP_modules_condition", "cond_fp"))
CONDITION_PREFIXES = ("SA_modules_condition", "FP_modules_condition", "global_pnet")


# ------------------------------------------------------------------------------------------------ index backends
def _xyz32(t):
    return t.detach().to(torch.float32).contiguous()


def _oracle_index_ops():
    from oracle import pdr_oracle as O

    def n(t):
        return _xyz32(t).cpu().numpy()

    def back(a, like):
        return torch.from_numpy(np.ascontiguousarray(a)).to(like.device)

    return {"fps": lambda xyz, m: back(O.furthest_point_sampling(n(xyz), m), xyz),
            "ball": lambda q, xyz, r, ns: tuple(back(a, xyz) for a in O.ball_query(n(q), n(xyz), r, ns)),
            "knn": lambda p1, p2, K: back(O.knn(n(p1), n(p2), K)[1], p1),
            "three_nn": lambda u, k: back(O.three_nn(n(u), n(k))[1], u)}


def _hip_index_ops():
    fps, ball, knn, three = (getattr(_ext, k) for k in INDEX_OPS)      # the real kernels, captured before the swap
    return {"fps": lambda xyz, m: fps(_xyz32(xyz), m),
            "ball": lambda q, xyz, r, ns: ball(_xyz32(q), _xyz32(xyz), r, ns),
            "knn": lambda p1, p2, K: knn(_xyz32(p1), _xyz32(p2), K)[1],
            "three_nn": lambda u, k: three(_xyz32(u), _xyz32(k))[1]}


# ------------------------------------------------------------------------------------------------ data-moving ops
def _rows(points, idx):
    """points (B, n, D), idx (B, ...) integer, -1 = padding -> (rows (B, ..., D) in points' dtype, valid mask)."""
    B, _, D = points.shape
    valid = idx >= 0
    flat = idx.clamp(min=0).long().reshape(B, -1, 1).expand(-1, -1, D)
    return points.gather(1, flat).reshape(*idx.shape, D), valid


def _sq_dists(queries, points, idx):
    """Squared distances query -> chosen points, in the dtype of the inputs; 0 in padding slots."""
    nn, valid = _rows(points, idx)
    d = ((queries.unsqueeze(2) - nn) ** 2).sum(-1)
    return d * valid.to(d.dtype), nn * valid.unsqueeze(-1).to(nn.dtype)


def _gather_points(points, idx):
    """(B, C, N), (B, m) -> (B, C, m)"""
    return points.gather(2, idx.long().unsqueeze(1).expand(-1, points.shape[1], -1))


def _group_points(points, idx):
    """(B, C, N), (B, np, ns) -> (B, C, np, ns)"""
    B, C, _ = points.shape
    return _gather_points(points, idx.reshape(B, -1)).reshape(B, C, *idx.shape[1:])


def _three_interpolate(points, idx, weight):
    """(B, C, m), (B, n, 3), (B, n, 3) -> (B, C, n)"""
    return (_group_points(points, idx) * weight.to(points.dtype).unsqueeze(1)).sum(-1)


def _scatter_points_grad(grad_out, idx, n):
    """Backward of _gather_points / _group_points: (B, C, m) or (B, C, np, ns), idx (B, m) or (B, np, ns), n ->
    (B, C, n) in grad_out's dtype.  Indices are taken as the forward takes them (`idx.long()`, no padding slot: ball
    query pads with a real index, and a negative one raises here as it does there)."""
    B, C = grad_out.shape[:2]
    flat = idx.reshape(B, 1, -1).long().expand(-1, C, -1)
    return grad_out.new_zeros(B, C, int(n)).scatter_add_(2, flat, grad_out.reshape(B, C, -1))


def _three_interpolate_grad(grad_out, idx, weight, m):
    """Backward of _three_interpolate w.r.t. points: (B, C, n), (B, n, 3), (B, n, 3), m -> (B, C, m)."""
    return _scatter_points_grad(grad_out.unsqueeze(-1) * weight.to(grad_out.dtype).unsqueeze(1), idx, m)


def _table(index):
    def furthest_point_sampling(points, nsamples):
        return index["fps"](points, int(nsamples)).to(torch.int32)

    def ball_query(new_xyz, xyz, radius, nsample):
        idx, counts = index["ball"](new_xyz, xyz, radius, nsample)
        return idx.to(torch.int32), counts.to(torch.int32)

    def knn_points(p1, p2, K, return_nn=False, lengths1=None, lengths2=None):
        if lengths1 is not None or lengths2 is not None:
            raise NotImplementedError("float64_ops: knn_points with lengths is not on the module path")
        idx = index["knn"](p1, p2, int(K)).to(torch.int64)
        d, nn = _sq_dists(p1, p2, idx)
        return d, idx, (nn if return_nn else None)

    def three_nn(unknowns, knows):
        idx = index["three_nn"](unknowns, knows).to(torch.int32)
        return [_sq_dists(unknowns, knows, idx)[0], idx]

    table = {"furthest_point_sampling": furthest_point_sampling, "ball_query": ball_query, "knn_points": knn_points,
             "three_nn": three_nn, "gather_points": _gather_points, "group_points": _group_points,
             "three_interpolate": _three_interpolate}
    for suffix in ("", "_det"):                      # one scatter-add each: a fixed order has nothing to add in double
        table["gather_points_grad" + suffix] = _scatter_points_grad
        table["group_points_grad" + suffix] = _scatter_points_grad
        table["three_interpolate_grad" + suffix] = _three_interpolate_grad
    return table


def _uncovered(name):
    def raiser(*a, **k):
        raise AssertionError("float64_ops: the module path reached _ext.%s, which the float64 swap does not cover "
                             "(it would run an fp32 kernel)" % name)
    return raiser


@contextlib.contextmanager
def float64_ops(index_ops, f32_step_embedding=True, dtype=torch.float64):
    """Swap `pointnet2_ops._ext` for the float64 evaluation: index ops by `index_ops` ("oracle" | "hip") on the fp32
    cast of their coordinates, data-moving ops and their backward entries (gather / group / three_interpolate `_grad`
    and `_grad_det`, one scatter-add each) as torch indexing in their input's dtype, returned distances recomputed
    in the input dtype from the chosen indices; every other kernel entry of `_ext` raises.

    dtype: what the step embedding is cast to, i.e. the dtype of the model that runs inside.  The stand-ins follow
    their inputs, so `dtype=torch.float32` carries the fp32 module through the same table: the composition on the CPU.

    f32_step_embedding: `calc_t_emb` evaluates ts * freq in f32 and takes sin / cos of that f32 product; the fused
    pdr_embed_linear reproduces this on purpose, so it is the specification: the float64 model takes the f32 result cast
    to double (False: the double product -- only to show what the patch is worth)."""
    if index_ops not in ("oracle", "hip"):
        raise ValueError("index_ops must be 'oracle' or 'hip'")
    table = _table(_oracle_index_ops() if index_ops == "oracle" else _hip_index_ops())
    saved = {}
    for name, fn in list(vars(_ext).items()):
        if name in table:
            saved[name] = fn
            setattr(_ext, name, table[name])
        elif inspect.isfunction(fn) and fn.__module__ == _ext.__name__ and not name.startswith("_") \
                and name not in _PASS_THROUGH:
            saved[name] = fn
            setattr(_ext, name, _uncovered(name))
    assert set(table) <= set(saved), sorted(set(table) - set(saved))
    calc = _model.calc_t_emb
    if f32_step_embedding:
        _model.calc_t_emb = lambda ts, dim: calc(ts.to(torch.float32), dim).to(dtype)
    else:
        _model.calc_t_emb = lambda ts, dim: calc(ts.to(torch.float64), dim).to(dtype)
    try:
        yield
    finally:
        _model.calc_t_emb = calc
        for name, fn in saved.items():
            setattr(_ext, name, fn)


@contextlib.contextmanager
def log_indices():
    """Record the integer outputs of the index ops installed right now (enter it INSIDE oracle_ops / float64_ops, or
    alone around the real kernels) -> list of (op name, tensor on the CPU), in call order.  `_ext.knn_group`, the
    search `group_knn` takes instead of `knn_points` under set_fused_knn_grouping, is logged under the name
    "knn_points": the same decision at the same place in the call order (int32 there, int64 here)."""
    log = []
    saved = {k: getattr(_ext, k) for k in INDEX_OPS + ("knn_group",)}

    def wrap(name, fn):
        def logged(*a, **k):
            out = fn(*a, **k)
            for t in (out if isinstance(out, (tuple, list)) else (out,)):
                if torch.is_tensor(t) and not t.is_floating_point():
                    log.append((name, t.detach().cpu().clone()))
            return out
        return logged
    for name, fn in saved.items():
        setattr(_ext, name, wrap("knn_points" if name == "knn_group" else name, fn))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(_ext, name, fn)


def float64_model(net):
    """A deep copy of a PointNet2CloudCondition in double, eval mode, nothing retained."""
    m = copy.deepcopy(net)
    m.reset_cond_features()
    return m.double().eval()


# ------------------------------------------------------------------------------------------------ ReLU decisions
class ReluTape:
    """`masks`: one bool tensor (x > 0) per ReLU site of a forward, in call order; `kinds`: what recorded each
    ("relu" = an nn.ReLU module, "group_norm_act" / "relu_group_norm" = the fused entry that holds the ReLU)."""

    def __init__(self, masks=(), kinds=()):
        self.masks, self.kinds = list(masks), list(kinds)

    def __len__(self):
        return len(self.masks)

    def shapes(self):
        return [tuple(m.shape) for m in self.masks]

    def elements(self):
        return sum(m.numel() for m in self.masks)

    def differing(self, other):
        """Number of mask elements on which two tapes of the same sites disagree."""
        assert self.shapes() == other.shapes()
        return sum(int((a != b.to(a.device)).sum()) for a, b in zip(self.masks, other.masks))

    def flipped(self, site, index):
        """A copy with one element of one site inverted (`index`: a tuple into that site's mask)."""
        masks = list(self.masks)
        masks[site] = masks[site].clone()
        masks[site][index] = ~masks[site][index]
        return ReluTape(masks, self.kinds)


@contextlib.contextmanager
def relu_tape(mode, tape=None):
    """Pin the ReLU decisions of a forward, as the index ops pin the geometric ones.  A mask that differs between two
    evaluations is a decision, not rounding: the float64 gradient then belongs to another piecewise-linear function.

    mode "record": every nn.ReLU call (the in-place modules too, evaluated out of place) appends `x > 0` to a new tape
    and returns `x * mask`; the two fused `_ext` entries that contain a ReLU append the mask of the same virtual site:
    `group_norm_act(act="relu")` that of its output, `relu_group_norm(q, k)` that of cat([q over K, k], 1) -- the tensor
    the composition rectifies at weight_conv[0] / weight_conv[3].  A fused run and the composition therefore record
    the same sites in the same order.  Yields the tape.
    mode "replay": every nn.ReLU call consumes the next mask of `tape` (same shape, or an AssertionError that names
    the site) and returns `x * mask`; leaving the context with masks left over is an error too.  Swish, the masked
    softmax and the integer clamp of counts hold no such decision."""
    if mode not in ("record", "replay") or (mode == "replay") != (tape is not None):
        raise ValueError("relu_tape('record') or relu_tape('replay', tape)")
    relu_forward = torch.nn.ReLU.forward
    fused = {"group_norm_act": _ext.group_norm_act, "relu_group_norm": _ext.relu_group_norm}
    pos = [0]
    if mode == "record":
        tape = ReluTape()

        def forward(self, x):
            mask = x > 0
            tape.masks.append(mask)
            tape.kinds.append("relu")
            return x * mask.to(x.dtype)

        def group_norm_act(x, weight, bias, num_groups, eps=1e-5, act="none"):
            out = fused["group_norm_act"](x, weight, bias, num_groups, eps, act)
            if act == "relu":
                tape.masks.append(out[0] > 0)
                tape.kinds.append("group_norm_act")
            return out

        def relu_group_norm(q, k, *a, **kw):
            mask = k > 0
            if q is not None:
                mask = torch.cat([(q > 0).unsqueeze(-1).expand(-1, -1, -1, k.shape[3]), mask], 1)
            tape.masks.append(mask)
            tape.kinds.append("relu_group_norm")
            return fused["relu_group_norm"](q, k, *a, **kw)

        _ext.group_norm_act, _ext.relu_group_norm = group_norm_act, relu_group_norm
    else:
        def forward(self, x):
            site = pos[0]
            assert site < len(tape), "relu_tape: ReLU call %d, the tape holds %d sites" % (site, len(tape))
            mask = tape.masks[site]
            assert mask.shape == x.shape, "relu_tape: site %d (%s) was recorded with shape %s, replayed on %s" % (
                site, tape.kinds[site], tuple(mask.shape), tuple(x.shape))
            pos[0] += 1
            return x * mask.to(device=x.device, dtype=x.dtype)
    torch.nn.ReLU.forward = forward
    try:
        yield tape
        if mode == "replay":
            assert pos[0] == len(tape), "relu_tape: the replay ended at site %d of %d" % (pos[0], len(tape))
    finally:
        torch.nn.ReLU.forward = relu_forward
        _ext.group_norm_act, _ext.relu_group_norm = fused["group_norm_act"], fused["relu_group_norm"]


# ------------------------------------------------------------------------------------------------ Chamfer decisions
class ChamferTape:
    """`terms`: one dict per Chamfer term of a loss, in call order -- "idx_gt" (B, n_gt) / "idx_out" (B, n_out) int64:
    the nearest neighbour of every gt point in the output cloud and of every output point in gt, as the recording run's
    K = 1 search chose them; "out" (B, n_out, 3) / "gt" (B, n_gt, 3): the clouds that search saw, in double."""

    def __init__(self, terms=()):
        self.terms = list(terms)

    def __len__(self):
        return len(self.terms)

    def same_decisions(self, other):
        return len(self) == len(other) and all(torch.equal(a[k], b[k]) for a, b in zip(self.terms, other.terms)
                                               for k in ("idx_gt", "idx_out"))


def taped_sq_dists(output, gt, idx_gt, idx_out):
    """(d_gt (B, n_gt), d_out (B, n_out)): |gt_i - output_idx_gt(i)|^2 and |output_j - gt_idx_out(j)|^2 in the dtype of
    the clouds, by torch indexing alone -- differentiable in both clouds, no search."""
    def direction(queries, points, idx):
        rows = points.gather(1, idx.to(points.device).unsqueeze(-1).expand(-1, -1, 3))
        return ((queries - rows) ** 2).sum(-1)
    return direction(gt, output, idx_gt), direction(output, gt, idx_out)


def taped_cd(output, gt, idx_gt, idx_out):
    """calc_cd's (cd_p, cd_t), each (B,), from `taped_sq_dists`."""
    d1, d2 = taped_sq_dists(output, gt, idx_gt, idx_out)
    return (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2, d1.mean(1) + d2.mean(1)


@contextlib.contextmanager
def chamfer_tape(mode, tape=None, nn=None):
    """Pin the nearest-neighbour assignment of a Chamfer loss: the one decision that depends on the network's output,
    so the one the shared geometry and the ReLU tape leave open.  Yields an object whose `.cd(fn)` is the
    `(output, gt) -> (cd_p, cd_t)` a loss calls once per term.

    mode "record": `.cd(fn)` runs `nn(gt, output)` -- the K = 1 search in both directions, `_ext.chamfer_nn`'s
    signature and return order -- on the detached clouds, appends its two index tensors (and the clouds) to a new
    tape, then returns `fn(output, gt)`: calc_cd, calc_cd_fused (which returns no index: the extra search finds the
    same ones, its minima are chamfer_nn's bit for bit) or anything with their signature.  `.tape` is the tape.
    mode "replay": `.cd()` consumes the next term of `tape` and evaluates it by `taped_cd` on the clouds it is given
    (same shapes, or an AssertionError that names the term) -- no search, no `_ext` entry; `.outputs` collects the
    output clouds it saw (detached, on the CPU).  Leaving the context with terms left over is an error."""
    if mode not in ("record", "replay") or (mode == "replay") != (tape is not None) or (mode == "record") != (nn is not None):
        raise ValueError("chamfer_tape('record', nn=search) or chamfer_tape('replay', tape)")

    class Handle:
        pass
    h = Handle()
    if mode == "record":
        h.tape = ChamferTape()

        def cd(fn):
            def recorded(output, gt):
                o, g = output.detach().contiguous(), gt.detach().contiguous()
                _, idx_gt, _, idx_out = nn(g, o)
                h.tape.terms.append({"idx_gt": idx_gt.detach().long().cpu(), "idx_out": idx_out.detach().long().cpu(),
                                     "out": o.double().cpu(), "gt": g.double().cpu()})
                return fn(output, gt)
            return recorded
        h.cd = cd
        yield h
    else:
        h.tape, h.outputs = tape, []

        def cd(fn=None):
            def replayed(output, gt):
                n = len(h.outputs)
                assert n < len(tape), "chamfer_tape: Chamfer term %d, the tape holds %d" % (n, len(tape))
                term = tape.terms[n]
                assert output.shape == term["out"].shape and gt.shape == term["gt"].shape, \
                    "chamfer_tape: term %d was recorded on %s / %s, replayed on %s / %s" % (
                        n, tuple(term["out"].shape), tuple(term["gt"].shape), tuple(output.shape), tuple(gt.shape))
                h.outputs.append(output.detach().double().cpu())
                return taped_cd(output, gt, term["idx_gt"], term["idx_out"])
            return replayed
        h.cd = cd
        yield h
        assert len(h.outputs) == len(tape), "chamfer_tape: the replay ended at term %d of %d" % (len(h.outputs), len(tape))


def oracle_chamfer_nn(x, y):
    """`_ext.chamfer_nn`'s signature and return order on the CPU oracle (its K = 1 kNN, both directions, on the fp32
    cast of the clouds): the search a `chamfer_tape("record")` takes where no GPU is."""
    from oracle import pdr_oracle as O
    a, b = _xyz32(x).cpu().numpy(), _xyz32(y).cpu().numpy()
    out = []
    for p, q in ((a, b), (b, a)):
        d, i = O.knn(p, q, 1)
        out += [torch.from_numpy(np.ascontiguousarray(d[..., 0])), torch.from_numpy(np.ascontiguousarray(i[..., 0])).long()]
    return tuple(out)


def chamfer_tape_honesty(tape, outputs64):
    """The honesty condition of a replayed Chamfer tape.  `outputs64`: the float64 output cloud of every term (the
    replay's `.outputs`).  A taped index j may differ from float64's own argmin j* only where the recording run could
    not tell them apart.  With delta = the largest Euclidean distance between an output point of the recording run and
    the same point in float64, moving one endpoint of a pair by at most delta changes its squared distance d by at most
    2 sqrt(d) delta + delta^2; the recording run ranked j no worse than j*, and both distances move; its own fp32
    evaluation of the distance it ranked is within 16 * 2^-24 relative.  So, in float64 on the float64 clouds,
        d(j) - d(j*) <= 2 (2 sqrt(d(j)) delta + delta^2) + 16 * 2^-24 * d(j)
    for every query with j != j*, in both directions.
    -> {"differing": queries with j != j*, "ratio": the largest (d(j) - d(j*)) / bound over them (0.0 if none),
        "delta": the largest delta over the terms, "nearest": the smallest float64 nearest-neighbour DISTANCE (not
        squared) over all terms and both directions}"""
    assert len(tape) == len(outputs64) > 0
    differing, ratio, delta_max, nearest = 0, 0.0, 0.0, float("inf")
    for term, out in zip(tape.terms, outputs64):
        gt = term["gt"]
        delta = float((out - term["out"]).norm(dim=-1).max())
        delta_max = max(delta_max, delta)
        pair = ((gt.unsqueeze(2) - out.unsqueeze(1)) ** 2).sum(-1)          # (B, n_gt, n_out), float64, term by term
        for d_all, idx in ((pair, term["idx_gt"]), (pair.transpose(1, 2), term["idx_out"])):
            best = d_all.min(-1).values
            taped = d_all.gather(2, idx.unsqueeze(-1))[..., 0]
            nearest = min(nearest, float(best.min().sqrt()))
            other = taped > best                                            # (an exact float64 tie is the same minimum)
            bound = 2 * (2 * taped.sqrt() * delta + delta ** 2) + 16 * 2.0 ** -24 * taped
            differing += int(other.sum())
            if bool(other.any()):
                ratio = max(ratio, float(((taped - best) / bound)[other].max()))
    return {"differing": differing, "ratio": ratio, "delta": delta_max, "nearest": nearest}


@contextlib.contextmanager
def coordinate_leaf(net, x):
    """A gradient w.r.t. the coordinates of x_t.  `PointNet2CloudCondition.forward` splits its input under
    `torch.no_grad()` (as the reference does), so `x.requires_grad_()` reaches no op and `x.grad` stays None.  Here one
    leaf with x's values stands in for the level-0 coordinates wherever a recorded block receives them (the first
    encoder / last decoder feature map as queries, SA_modules.0 as the cloud, FP_modules.0 as the unknowns); the deeper
    levels are gathers of it.  That gradient runs through the coordinate paths of the grouping ops: relative and centre
    channels, kNN distances, weights.  The copy of the coordinates in the input features stays a constant, in every
    evaluation alike.  x: (B, N, 3) in the dtype the network sees.  Yields the leaf."""
    leaf = x.detach().clone().requires_grad_()

    def swap(t):
        same = torch.is_tensor(t) and t.shape == leaf.shape and t.dtype == leaf.dtype and not t.requires_grad
        return leaf if same and torch.equal(t, leaf.detach()) else t

    def hook(module, args, kwargs):
        return tuple(swap(t) for t in args), {k: swap(v) for k, v in kwargs.items()}
    handles = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in module_names(net).values()]
    try:
        yield leaf
    finally:
        for h in handles:
            h.remove()


@contextlib.contextmanager
def record_max_gaps(net):
    """The two max-over-points reductions of the global PointNet (models/pnet.py) are argmax decisions that nothing
    pins.  Forward hooks on `global_pnet.mlp1` / `.mlp2` -> {name: (smallest gap, dead columns)} per forward: the gap
    between the largest and the second-largest value of a reduced column over the tensor's largest magnitude, the
    minimum over the columns; a column whose largest value is exactly 0 behind a ReLU (every point rectified away, all
    of them tied at 0) is counted as dead and left out: its mask is pinned, so every evaluation has the same zeros there
    and whichever point the max picks passes a gradient that the mask then removes."""
    gaps = {}

    def hook(name):
        def record(m, args, out):
            t = out.detach()
            top = t.topk(2, dim=2).values                                   # (B, C, 2, 1)
            dead = (top[:, :, 0] == 0) & (top[:, :, 1] == 0)
            gap = ((top[:, :, 0] - top[:, :, 1]) / t.abs().max()).masked_fill(dead, float("inf"))
            gaps[name] = (float(gap.min()), int(dead.sum()))
        return record
    handles = [getattr(net.global_pnet, k).register_forward_hook(hook("global_pnet." + k)) for k in ("mlp1", "mlp2")]
    try:
        yield gaps
    finally:
        for h in handles:
            h.remove()


# ------------------------------------------------------------------------------------------------ fused-entry calls
# position of the saved tensor that ties a backward call to its forward call: (forward entry, arg) / (backward, arg)
_CALL_KEYS = {"attention_pool": 0, "attention_pool_grad": 0, "group_norm_act": 0, "group_norm_act_grad": 0,
              "relu_group_norm": 1, "relu_group_norm_grad": 1, "query_group": 3, "query_group_grad": 0,
              "knn_group_cf": 3, "knn_group_cf_grad": 2}


class ExtCalls:
    """`log`: (entry, block, differentiable) per call of a fused `_ext` entry, in call order -- block = the recorded
    child of the network the call belongs to, differentiable = a floating input required a gradient (forward entries).
    `edit[entry] = fn(n, block, out) -> out` rewrites the n-th result of an entry (fault seeding, in Python)."""

    def __init__(self):
        self.log, self.edit = [], {}

    def count(self, entry, block="*"):
        """Calls of `entry`, in all blocks or in one (None: outside every recorded block)."""
        return sum(1 for e, b, _ in self.log if e == entry and (block == "*" or b == block))

    def differentiable(self, entry):
        return sum(1 for e, _, d in self.log if e == entry and d)


@contextlib.contextmanager
def count_ext_calls(net):
    """Wrap the ten fused entries of `_ext` (FUSED_ENTRIES) with counters for one network -> ExtCalls.  A forward call
    is attributed to the recorded block whose forward is running, a backward call to the block of the forward call
    that saved the same tensor."""
    calls, stack, owner = ExtCalls(), [], {}
    saved = {e: getattr(_ext, e) for pair in FUSED_ENTRIES.values() for e in pair}

    def wrap(entry, fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            key = a[_CALL_KEYS[entry]].data_ptr()
            if entry.endswith("_grad"):
                block, diff = owner.get(key), False
            else:
                block = owner[key] = stack[-1] if stack else None
                diff = any(torch.is_tensor(t) and t.is_floating_point() and t.requires_grad for t in a)
            n = calls.count(entry)
            calls.log.append((entry, block, diff))
            return calls.edit[entry](n, block, out) if entry in calls.edit else out
        return wrapped
    def leave(m, args, out):
        stack.pop()
    handles = []
    for name, mod in module_names(net).items():
        handles.append(mod.register_forward_pre_hook(lambda m, args, name=name: stack.append(name)))
        handles.append(mod.register_forward_hook(leave))
    for entry, fn in saved.items():
        setattr(_ext, entry, wrap(entry, fn))
    try:
        yield calls
    finally:
        for entry, fn in saved.items():
            setattr(_ext, entry, fn)
        for h in handles:
            h.remove()


def block_of(name):
    """Top-level block of a parameter name: 'SA_modules.0.mlps.0.fc.weight' -> 'SA_modules.0', 'fc_t1.weight' ->
    'fc_t1', 'fc_lyaer.3.bias' -> 'fc_lyaer': the recorded blocks of `module_names`, and the network's other children."""
    parts = name.split(".")
    return ".".join(parts[:2]) if parts[0] in {attr for attr, _ in BLOCK_LISTS} else parts[0]


# ------------------------------------------------------------------------------------------------ recorders
def module_names(net):
    """name -> child module, for every recorded child of a PointNet2CloudCondition."""
    out = {}
    for attr, _ in BLOCK_LISTS:
        for i, m in enumerate(getattr(net, attr)):
            out["%s.%d" % (attr, i)] = m
    if getattr(net, "global_pnet", None) is not None:
        out["global_pnet"] = net.global_pnet
    return out


def _channel_last(t):
    """(B, C, n) -> (B, n, C); the global feature (B, C) -> (B, 1, C)."""
    t = t.detach()
    return (t.unsqueeze(1) if t.dim() == 2 else t.transpose(1, 2)).contiguous().clone()


class Recorder:
    """`calls`: one {name: (B, n, C) tensor} per forward of the recorded network, in call order; `eps` under "eps"."""

    def __init__(self):
        self.calls = []

    def begin(self):
        self.calls.append({})

    def put(self, name, t):
        self.calls[-1][name] = t


@contextlib.contextmanager
def record_modules(net):
    """Forward hooks on SA / FP / feature-map modules of both branches and on the global PointNet."""
    rec = Recorder()
    handles = [net.register_forward_pre_hook(lambda m, args: rec.begin()),
               net.register_forward_hook(lambda m, args, out: rec.put("eps", out.detach().clone()))]
    for name, mod in module_names(net).items():
        def hook(m, args, out, name=name):
            rec.put(name, _channel_last(out[1] if isinstance(out, tuple) else out))     # SA: (new_xyz, features)
        handles.append(mod.register_forward_hook(hook))
    try:
        yield rec
    finally:
        for h in handles:
            h.remove()


def fused_names(fused):
    """id(block instance) -> name of the torch module it was built from."""
    out = {}
    for attr, fattr in BLOCK_LISTS:
        blocks = getattr(fused, fattr)
        assert len(blocks) == len(getattr(fused.net, attr)), (attr, fattr)
        for i, blk in enumerate(blocks):
            out[id(blk)] = "%s.%d" % (attr, i)
    if fused.global_pnet is not None:
        out[id(fused.global_pnet)] = "global_pnet"
    return out


@contextlib.contextmanager
def record_fused(fused):
    """Class-level wrappers (restored on exit) around FusedGroupedBlock.__call__ / .finish, FusedKnnFP.__call__ and
    FusedPnet2Stage.__call__: the output of every block of `fused` is cloned where it is returned, on the stream
    current there (the buffers are reused).  A hoisted block returns through `finish`, a whole one through `__call__`
    (which may itself go through `finish`): one record per block and forward, the outermost.  `rec.dedup` holds, per
    forward, the names of the blocks whose per-neighbour launches walked a Dedup plan."""
    rec = Recorder()
    rec.dedup = []
    names = fused_names(fused)
    depth = [0]

    def wrap(fn):
        def wrapped(self, *a, **k):
            name = names.get(id(self))
            if name is None or not rec.calls:
                return fn(self, *a, **k)
            depth[0] += 1
            try:
                out = fn(self, *a, **k)
            finally:
                depth[0] -= 1
            if depth[0] == 0:
                assert name not in rec.calls[-1], "block %s returned twice in one forward" % name
                t = out.detach()
                rec.put(name, (t.unsqueeze(1) if t.dim() == 2 else t).clone())
            return out
        return wrapped

    def wrap_plan(fn):
        def wrapped(self, *a, **k):
            plan = fn(self, *a, **k)
            if plan is not None and id(self) in names and rec.dedup:
                rec.dedup[-1].add(names[id(self)])
            return plan
        return wrapped

    def wrap_net(fn):
        def wrapped(self, *a, **k):
            if self is not fused:
                return fn(self, *a, **k)
            rec.begin()
            rec.dedup.append(set())
            out = fn(self, *a, **k)
            rec.put("eps", out.detach().clone())
            return out
        return wrapped

    patches = [(FN.FusedGroupedBlock, "__call__", wrap), (FN.FusedGroupedBlock, "finish", wrap),
               (FN.FusedGroupedBlock, "_plan", wrap_plan), (FN.FusedKnnFP, "__call__", wrap),
               (FN.FusedPnet2Stage, "__call__", wrap), (FN.FusedCloudConditionNet, "__call__", wrap_net),
               (FN.FusedCloudConditionNet, "forward", wrap_net)]
    saved = [(cls, attr, cls.__dict__[attr]) for cls, attr, _ in patches]
    for cls, attr, w in patches:
        setattr(cls, attr, w(cls.__dict__[attr]))
    try:
        yield rec
    finally:
        for cls, attr, fn in saved:
            setattr(cls, attr, fn)


def is_condition_block(name):
    return name.startswith(CONDITION_PREFIXES)
