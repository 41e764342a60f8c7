"""Host side of the hand-overs between the halves of a block (no GPU, no library): field order and tuple compatibility of
the records of fused_network, the thunk form of a value made ahead, and the one-stream context of a hoisted half."""
import pytest
import torch

from point_diffusion_refinement_amd.pointnet2 import fused_network as FN


def test_injected_unpacks_and_indexes_as_tensor_offset_ld():
    bank = FN.EmbeddingBank()
    handles = [bank.register("t", torch.nn.Linear(8, c)) for c in (4, 12)]
    bank.pack()
    bank.out["t"] = torch.zeros(2, 16)
    assert bank.get(None) is None
    inj = bank.get(handles[1])
    assert isinstance(inj, tuple) and FN.Injected._fields == ("t", "off", "ld")
    t, off, ld = inj
    assert t is bank.out["t"] and (off, ld) == (4, 16)
    assert (inj[0], inj[1], inj[2]) == (inj.t, inj.off, inj.ld) and inj[0] is t and inj[1:] == (4, 16)
    assert tuple(bank.get(handles[0]))[1:] == (0, 16)


def test_records_keep_their_field_order():
    assert FN.Values._fields == ("V", "scale", "shift", "twin")
    V, scale, shift, twin = FN.Values(1, 2, 3, 4)
    assert (V, scale, shift, twin) == (1, 2, 3, 4)
    assert FN.QueryTables._fields == ("V2", "order")
    assert FN.QueryTables("tables") == ("tables", None)            # made for the original query order
    assert FN.Prepared._fields == ("head", "values", "event")
    prep = FN.Prepared("head", "values")
    assert prep.event is None and prep._replace(event="ev") == ("head", "values", "ev")
    assert FN.Head._fields == ("B", "m", "K", "counts", "first", "folded", "sq", "rows", "query", "q_ahead")
    assert FN.Head(2, 16, 8, "counts", "first")[5:] == (None,) * 5
    assert FN.Padded._fields == ("src", "padded", "stream", "event")
    idx = torch.zeros(1, dtype=torch.int32)
    e = FN.Geom(idx)
    assert e.tensor is idx and e.sorted is None and e.probed is False


def test_ready_is_the_thunk_of_an_existing_value():
    x = object()
    assert FN._ready(x)() is x
    assert FN._ready(None)() is None


def test_single_stream_restores_the_second_stream_when_its_body_raises():
    marker = object()
    saved, FN._PAR["stream"] = FN._PAR["stream"], marker
    try:
        with FN._single_stream():
            assert FN._PAR["stream"] is None
        assert FN._PAR["stream"] is marker
        with pytest.raises(RuntimeError):
            with FN._single_stream():
                assert FN._PAR["stream"] is None
                raise RuntimeError("body")
        assert FN._PAR["stream"] is marker
    finally:
        FN._PAR["stream"] = saved

