"""ctypes binding of libpdr_hip.so (the C ABI declared in include/pdr_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is
absent, importing an op raises.  Only device pointers, sizes and the current HIP
stream cross this boundary -- PyTorch is used for memory and streams, nothing else.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpdr_hip.so")

PDR_OK, PDR_EINVAL, PDR_EUNSUPPORTED, PDR_ELAUNCH = 0, -1, -2, -3
_ERR = {PDR_EINVAL: "invalid argument", PDR_EUNSUPPORTED: "unsupported size", PDR_ELAUNCH: "kernel launch failed"}

_c = ctypes
_P, _I, _F, _Z = _c.c_void_p, _c.c_int, _c.c_float, _c.c_size_t

# name -> (restype, argtypes); mirrors include/pdr_hip.h one to one
SIGNATURES = {
    "pdr_version": (_I, []),
    "pdr_last_error": (_c.c_char_p, []),
    "pdr_set_option": (_I, [_c.c_char_p, _I]),
    "pdr_get_option": (_I, [_c.c_char_p, _P]),
    "pdr_option_name": (_c.c_char_p, [_I]),
    "pdr_opt_n_threads": (_I, [_I]),
    "pdr_fps_workspace_bytes": (_Z, [_I, _I]),
    "pdr_furthest_point_sampling": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "pdr_fps_plan": (_I, [_I, _P]),
    "pdr_fps_ragged_workspace_bytes": (_Z, [_I, _I, _I]),
    "pdr_fps_ragged_plan": (_I, [_I, _I, _P]),
    "pdr_furthest_point_sampling_ragged": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "pdr_gather_points": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_gather_points_grad": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_ball_query": (_I, [_P, _P, _I, _I, _I, _F, _I, _P, _P, _P]),
    "pdr_ball_query_plan": (_I, [_I, _I, _I, _P]),
    "pdr_group_points": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "pdr_group_points_grad": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "pdr_three_nn": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_three_interpolate": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_three_interpolate_grad": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_knn_points": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "pdr_knn_points_ragged": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "pdr_chamfer_nn": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pdr_chamfer_nn_ragged": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pdr_chamfer_pairwise": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "pdr_chamfer_loss_workspace_bytes": (_Z, [_I, _I, _I]),
    "pdr_chamfer_loss": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pdr_chamfer_loss_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_attention_pool_cf_plan": (_I, [_I, _I, _P]),
    "pdr_attention_pool_cf": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_attention_pool_cf_grad": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pdr_group_norm_act_workspace_bytes": (_Z, [_I, _I, _c.c_long, _I]),
    "pdr_group_norm_act_plan": (_I, [_I, _c.c_long, _I, _I, _P]),
    "pdr_group_norm_act": (_I, [_P, _P, _P, _I, _I, _c.c_long, _I, _F, _I, _P, _P, _P, _P, _P]),
    "pdr_group_norm_act_grad": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _c.c_long, _I, _I, _P, _P, _P, _P, _P]),
    "pdr_group_norm_act_add": (_I, [_P, _P, _P, _P, _P, _I, _I, _c.c_long, _I, _F, _I, _P, _P, _P, _P, _P]),
    "pdr_group_norm_act_add_grad": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _c.c_long, _I, _I, _P, _P, _P, _P, _P, _P]),
    "pdr_relu_group_norm_cf_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "pdr_relu_group_norm_cf_plan": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "pdr_relu_group_norm_cf": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "pdr_relu_group_norm_cf_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "pdr_relu_group_norm_conv_cf_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I]),
    "pdr_relu_group_norm_conv_cf_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "pdr_relu_group_norm_conv_cf": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "pdr_relu_group_norm_conv_cf_grad_input": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "pdr_relu_group_norm_conv_cf_grad_weight": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P,
                                                     _P]),
    "pdr_query_group_cf_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "pdr_query_group_cf_plan": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "pdr_query_group_cf": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "pdr_query_group_cf_grad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pdr_knn_group_cf_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "pdr_knn_group_cf_plan": (_I, [_I, _I, _I, _I, _I, _P]),
    "pdr_knn_group_cf": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "pdr_knn_group_cf_grad": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pdr_occupancy_grid": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
    "pdr_knn_group": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "pdr_knn_plan": (_I, [_I, _I, _I, _I, _I, _I, _P]),
    "pdr_knn_points_grad": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pdr_scatter_workspace_bytes": (_Z, [_I, _I, _I]),
    "pdr_gather_points_grad_det": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pdr_group_points_grad_det": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "pdr_three_interpolate_grad_det": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pdr_knn_points_grad_det": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "pdr_emd_workspace_bytes": (_Z, [_I, _I, _I]),
    "pdr_matchcost_workspace_bytes": (_Z, [_I, _I, _I]),
    "pdr_approxmatch": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_matchcost": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_matchcost_grad": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_emd_cost": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_approxmatch_ragged": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_matchcost_ragged": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_matchcost_grad_ragged": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_emd_cost_ragged": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_emd_cost_grad": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_emd_cost_grad_ragged": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "pdr_fused_layer_tile_rows": (_I, [_I, _I]),
    "pdr_fused_layer_variant": (_I, [_I, _I]),
    "pdr_fused_layer_plan": (_I, [_P, _c.c_long, _I, _P, _I, _I, _P, _I, _P]),
    "pdr_fused_layer": (_I, [_P, _c.c_long, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P]),
    "pdr_fused_layer_pair": (_I, [_P, _c.c_long, _P, _c.c_long, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _P]),
    "pdr_fused_layer_f16x3": (_I, [_P, _c.c_long, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P]),
    "pdr_fused_layer_pool": (_I, [_P, _c.c_long, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P]),
    "pdr_fused_layer_pool_f16x3": (_I, [_P, _c.c_long, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P]),
    "pdr_fused_layer_pool_plan": (_I, [_P, _c.c_long, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _P]),
    "pdr_gn_reduce": (_I, [_P, _I, _I, _I, _I, _c.c_double, _P, _I, _I, _P]),
    "pdr_apply_act": (_I, [_P, _c.c_long, _I, _P, _I, _P]),
    "pdr_act_colmax": (_I, [_P, _c.c_long, _I, _P, _P]),
    "pdr_gn_fold": (_I, [_P, _I, _I, _I, _c.c_double, _P, _I, _I, _I, _c.c_double, _I, _I, _I, _c.c_double, _F,
                         _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    "pdr_gn_finalize": (_I, [_P, _I, _I, _I, _I, _c.c_double, _F, _P, _P, _P, _P, _P]),
    "pdr_group_build": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "pdr_knn_build": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "pdr_attention_pool": (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_gather_rows": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "pdr_reverse_update": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _c.c_long, _I, _P]),
    "pdr_reverse_step": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _c.c_long, _I, _P, _P, _P]),
    "pdr_embed_select": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _P]),
    "pdr_dedup_prepare": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pdr_dedup_probe": (_I, [_P, _I, _I, _I, _P, _P]),
    "pdr_gather_add_tiles_twin": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _P, _I,
                                       _P, _P, _I, _P, _F, _P]),
    "pdr_gather_rows2": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _P, _P]),
    "pdr_pad_rows": (_I, [_P, _c.c_long, _I, _P, _I, _P]),
    "pdr_mark_time": (_I, [_P, _P]),
    "pdr_embed_linear": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "pdr_gather_add": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _P]),
    "pdr_gather_add_tiles": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I,
                                  _P, _I, _P]),
    "pdr_gather_moments": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "pdr_gather_moments_tiles": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I,
                                      _I, _P, _I, _P]),
    "pdr_gather_moments_tiles_twin": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _P,
                                           _I, _P, _P, _I, _P, _F, _P]),
    "pdr_gather_plan": (_I, [_I] * 16 + [_c.c_uint, _P]),
    "pdr_dedup_plan": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "pdr_dedup_sort": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "pdr_weighted_moments": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    "pdr_patch_rows": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P]),
    "pdr_point_chain_plan": (_I, [_P, _I, _I, _P]),
    "pdr_point_chain": (_I, [_P, _I, _I, _P]),
}


class Seg(_c.Structure):
    _fields_ = [("ptr", _P), ("C", _I), ("ld", _I), ("row_div", _I), ("gV", _P), ("gV0", _P), ("g_ldv", _I),
                ("g_nsrc", _I), ("g_zrow", _I), ("g_reserved", _I), ("g_r1", _P), ("g_r2", _P)]


class LayerIn(_c.Structure):
    """pdr_layer_in_t of include/pdr_hip.h."""
    _fields_ = [("n_seg", _I), ("seg", Seg * 4), ("scale", _P), ("shift", _P), ("add", _P), ("rseg", Seg),
                ("add_ld", _I), ("pre_relu", _I), ("post_relu", _I), ("rows_per_batch", _I), ("gidx", _P),
                ("gcnt", _P), ("gK", _I), ("ss_ld", _I), ("oadd", _P), ("oadd_ld", _I), ("oadd_div", _I), ("oadd_rows", _P),
                ("gs1", _P), ("gs2", _P), ("tile_list", _P), ("n_tiles", _P), ("out_rows", _P), ("partial_tpb", _I),
                ("wmul", _F), ("wrow0", _P), ("patch_values", _P), ("patch_w", _P), ("patch_ld", _I),
                ("walk_reverse", _I)]
class ChainSeg(_c.Structure):
    _fields_ = [("ptr", _P), ("C", _I), ("ld", _I)]


class ChainLayer(_c.Structure):
    _fields_ = [("Wt", _P), ("bias", _P), ("ldw", _I), ("Cin", _I), ("Cout", _I), ("main_cols", _I), ("gamma", _P),
                ("beta", _P), ("groups", _I), ("Cn", _I), ("eps", _F), ("relu_pre", _I), ("relu_post", _I), ("add", _P),
                ("add_ld", _I), ("reserved_", _I)]


class PointChain(_c.Structure):
    """pdr_point_chain_t of include/pdr_hip.h."""
    _fields_ = [("n_layers", _I), ("n_seg", _I), ("seg", ChainSeg * 3), ("layer", ChainLayer * 4), ("residual", _I),
                ("ldo", _I), ("out", _P), ("scratch", _P), ("sync", _P)]


_lib = None
ABI_VERSION = 200          # pdr_version() this binding was written against (include/pdr_hip.h version history)


def load():
    """Load libpdr_hip.so; raise (never fall back) when it is missing or of another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "point_diffusion_refinement_amd: %s not found. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C %s/csrc`. "
                "There is no CPU fallback." % (LIB_PATH, _HERE))
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError = ABI mismatch, fail loudly
            fn.restype, fn.argtypes = res, args
        if lib.pdr_version() != ABI_VERSION:
            raise ImportError("point_diffusion_refinement_amd: %s is ABI %d, this binding needs %d -- rebuild it "
                              "(`make -C %s/csrc`)" % (LIB_PATH, lib.pdr_version(), ABI_VERSION, _HERE))
        _lib = lib
        _apply_env_options()
    return _lib


def set_option(name, value):
    """pdr_set_option: process-wide kernel-selection option (names / values: include/pdr_hip.h)."""
    check(load().pdr_set_option(name.encode(), int(value)), "set_option(%s=%r)" % (name, value))


def get_option(name):
    v = _c.c_int(0)
    check(load().pdr_get_option(name.encode(), _c.byref(v)), "get_option(%s)" % name)
    return v.value


def option_names():
    lib, out, i = load(), [], 0
    while True:
        n = lib.pdr_option_name(i)
        if n is None:
            return out
        out.append(n.decode())
        i += 1


def _apply_env_options():
    """The library itself never reads the environment (ABI 0.2.0).  For lab A/B runs and the variant tests, which
    start a child process per setting, THIS binding maps PDR_OPTIONS="name=value,..." -- and the PDR_<NAME>=v variables
    rounds 1-5 documented -- onto pdr_set_option once, at load."""
    for item in filter(None, (t.strip() for t in os.environ.get("PDR_OPTIONS", "").split(","))):
        name, _, val = item.partition("=")
        set_option(name.strip(), int(val))
    for name in option_names():
        val = os.environ.get("PDR_" + name.upper())
        if val is not None and val.strip().lstrip("-").isdigit():
            set_option(name, int(val))


def check(rc, what):
    if rc != PDR_OK:
        detail = ""
        if rc == PDR_ELAUNCH:
            detail = ": " + (load().pdr_last_error() or b"").decode()
        raise RuntimeError("%s failed: %s%s" % (what, _ERR.get(rc, "code %d" % rc), detail))
