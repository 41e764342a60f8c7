"""Host side of the layer launches (no GPU, no library): Act.struct() fills pdr_layer_in_t (include/pdr_hip.h) as its
inputs say, whether the segments are given as plain tuples / dicts or as Seg / Gather records."""
import ctypes

import pytest
import torch

from point_diffusion_refinement_amd import _lib
from point_diffusion_refinement_amd.pointnet2 import fused_network as FN


def _read(st):
    """ctypes structure -> nested dict of plain values (pointers: int or None)."""
    out = {}
    for name, _ in st._fields_:
        v = getattr(st, name)
        if isinstance(v, ctypes.Structure):
            v = _read(v)
        elif isinstance(v, ctypes.Array):
            v = [_read(e) for e in v]
        out[name] = v
    return out


def _ptr(t, off=0):
    return t.data_ptr() + 4 * off


def _cseg(ptr=None, C=0, ld=0, row_div=0, gV=None, gV0=None, g_ldv=0, g_nsrc=0, g_zrow=0, g_r1=None, g_r2=None):
    return dict(ptr=ptr, C=C, ld=ld, row_div=row_div, gV=gV, gV0=gV0, g_ldv=g_ldv, g_nsrc=g_nsrc, g_zrow=g_zrow,
                g_reserved=0, g_r1=g_r1, g_r2=g_r2)


def _layer_in(segs, rows_per_batch, **fields):
    """A zero-initialised pdr_layer_in_t with the given segments and fields, as a dict."""
    want = {name: (None if typ is _lib._P else 0) for name, typ in _lib.LayerIn._fields_}
    want.update(n_seg=len(segs), seg=segs + [_cseg()] * (4 - len(segs)), rseg=_cseg(), rows_per_batch=rows_per_batch)
    assert set(fields) <= set(want), set(fields) - set(want)
    want.update(fields)
    return want


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def _i(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def _forms(seg):
    """A segment given as (tensor, offset, C, ld, div[, gather dict]) in its two spellings: as it is, and as records."""
    rec = FN.Seg(*seg[:5], FN.Gather(**seg[5])) if len(seg) > 5 else FN.Seg(*seg)
    return seg, rec


@pytest.mark.parametrize("form", [0, 1], ids=["tuples", "records"])
def test_act_struct_fills_every_field_from_its_inputs(form):
    B, m, K = 2, 128, 16
    rpb, P = m * K, B * m * K
    # ---- one plain segment at a column offset + the whole prologue
    x, sc, sh, ad = _f(P, 40), _f(B, 64), _f(B, 64), _f(B, 48)
    a = FN.Act([_forms((x, 4, 33, 40, 1))[form]], P, B, rpb, scale=sc, shift=sh, add=ad, add_ld=48, pre_relu=True,
               post_relu=True)
    a.ss_ld = 64
    assert a.C == 33
    assert _read(a.struct()) == _layer_in([_cseg(_ptr(x, 4), 33, 40, 1)], rpb, scale=_ptr(sc), shift=_ptr(sh),
                                          add=_ptr(ad), add_ld=48, pre_relu=1, post_relu=1, ss_ld=64)
    # (add_ld belongs to `add`: without the rows it stays 0)
    assert _read(FN.Act([(x, 0, 40, 40, 1)], P, B, rpb, add_ld=48).struct()) == \
        _layer_in([_cseg(_ptr(x), 40, 40, 1)], rpb)
    # ---- two segments, the first broadcast over the K neighbours; output-side add through a row map
    q, k, Z, rows = _f(B * m, 32), _f(P, 36), _f(B * m, 64), _i(B * m)
    a = FN.Act([_forms((q, 0, 32, 32, K))[form], _forms((k, 1, 35, 36, 1))[form]], P, B, rpb)
    a.oadd, a.oadd_rows = (Z, K), rows
    assert a.C == 67
    assert _read(a.struct()) == _layer_in([_cseg(_ptr(q), 32, 32, K), _cseg(_ptr(k, 1), 35, 36, 1)], rpb,
                                          oadd=_ptr(Z), oadd_ld=64, oadd_div=K, oadd_rows=_ptr(rows))
    # ---- ball-gathered segment, with and without the empty-ball table V0 (and the default of zrow)
    n_src, ld = 50, 72
    U, V2, idx, cnt = _f(B * n_src + 1, ld), _f(B * m, 2 * ld), _i(P), _i(B * m)
    g = {"V": (V2, 8), "V0": (V2, ld + 8), "ldv": 2 * ld, "nsrc": n_src, "zrow": B * n_src}
    a = FN.Act([_forms((U, 8, 64, ld, 1, g))[form]], P, B, rpb)
    a.gidx, a.gcnt, a.gK = idx, cnt, K
    assert _read(a.struct()) == _layer_in(
        [_cseg(_ptr(U, 8), 64, ld, 1, gV=_ptr(V2, 8), gV0=_ptr(V2, ld + 8), g_ldv=2 * ld, g_nsrc=n_src,
               g_zrow=B * n_src)], rpb, gidx=_ptr(idx), gcnt=_ptr(cnt), gK=K)
    g = {"V": (V2, 0), "V0": None, "ldv": 2 * ld, "nsrc": n_src}
    a = FN.Act([_forms((U, 0, 64, ld, 1, g))[form]], P, B, rpb)
    a.gidx, a.gK = idx, K
    assert _read(a.struct()) == _layer_in(
        [_cseg(_ptr(U), 64, ld, 1, gV=_ptr(V2), g_ldv=2 * ld, g_nsrc=n_src, g_zrow=-1)], rpb, gidx=_ptr(idx), gK=K)
    # ---- kNN-gathered segment (+ gs1 r1 + gs2 r2) with a gathered residual window of the same first conv
    r1, r2, s1, s2 = _f(ld + 4), _f(ld + 4), _f(P), _f(P)
    g = {"V": (V2, 0), "V0": None, "ldv": 2 * ld, "nsrc": n_src, "zrow": B * n_src, "r1": (r1, 0), "r2": (r2, 0)}
    gr = dict(g, V=(V2, 32), r1=(r1, 32), r2=(r2, 32))
    a = FN.Act([_forms((U, 0, 32, ld, 1, g))[form]], P, B, rpb, radd=_forms((U, 32, 32, ld, 1, gr))[form])
    a.gidx, a.gK, a.gs1, a.gs2 = idx, K, s1, s2
    knn = dict(g_ldv=2 * ld, g_nsrc=n_src, g_zrow=B * n_src)
    assert _read(a.struct()) == _layer_in(
        [_cseg(_ptr(U), 32, ld, 1, gV=_ptr(V2), g_r1=_ptr(r1), g_r2=_ptr(r2), **knn)], rpb,
        rseg=_cseg(_ptr(U, 32), 32, ld, 1, gV=_ptr(V2, 32), g_r1=_ptr(r1, 32), g_r2=_ptr(r2, 32), **knn),
        gidx=_ptr(idx), gK=K, gs1=_ptr(s1), gs2=_ptr(s2))
    # ---- a tile list: its own rows of `partial` per cloud unless the launch names another count; pooled patch
    nvalid = _i(2, B)

    def prepared(dd):
        dd.nvalid = nvalid
    dd = FN.Dedup(idx.view(B, m, K), cnt.view(B, m), B, m, K, prepared=prepared)
    assert (dd.tpb, dd.tpbd, dd.ptpb) == (m * K // 128, 1, m * K // 128 + 1)
    S, Vd = _f(P, 64), _f(B * m, 32)
    a = FN.Act([_forms((S, 0, 64, 64, 1))[form]], P, B, rpb)
    a.dd, a.patch = dd, (Vd, dd.row_w)
    tiles = dict(tile_list=_ptr(dd.tile_list), n_tiles=_ptr(dd.n_tiles), patch_values=_ptr(Vd), patch_ld=32,
                 patch_w=_ptr(dd.row_w))
    assert _read(a.struct()) == _layer_in([_cseg(_ptr(S), 64, 64, 1)], rpb, partial_tpb=dd.ptpb, **tiles)
    assert _read(a.struct(partial_tpb=19)) == _layer_in([_cseg(_ptr(S), 64, 64, 1)], rpb, partial_tpb=19, **tiles)
    # ---- its twin over the per-query rows: weighted statistics (rows >= wrow0[b], x K) into rows of the same tensor
    Sd = _f(B * m, 64)
    tw = FN._twin_act([_forms((Sd, 0, 64, 64, 1))[form]], dd, B)
    assert (tw.P, tw.rpb) == (B * m, m)
    assert _read(tw.struct(partial_tpb=19)) == _layer_in([_cseg(_ptr(Sd), 64, 64, 1)], m, partial_tpb=19,
                                                         wrow0=_ptr(nvalid, B), wmul=float(K))
    assert _read(tw.struct()) == _layer_in([_cseg(_ptr(Sd), 64, 64, 1)], m, wrow0=_ptr(nvalid, B), wmul=float(K))
    assert _read(tw.struct(weighted=False)) == _layer_in([_cseg(_ptr(Sd), 64, 64, 1)], m)
