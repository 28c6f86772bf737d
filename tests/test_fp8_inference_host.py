"""CPU-only: the host side of exact inference over an fp8 table read in place (f3o) -- the refusals of
spp_graph_agg_forward_fp8, spp_graph_agg_parts_forward_fp8 and spp_fp8_rows_f32 (status -1, a message that starts with
the entry's own name; made before anything is enqueued, so fake pointers do and no GPU is needed), the type checks of
inference.Fp8Table, the entries that refuse an Fp8Table with a reason, and the pinned refusals of a bare Fp8Features,
which stay as they were."""
import ctypes

import pytest
import torch

_FAKE = 0x10000                                               # 16-byte aligned, never dereferenced
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)
AGG_ENTRIES = ["spp_graph_agg_forward_fp8", "spp_graph_agg_parts_forward_fp8"]


@pytest.fixture
def no_device(monkeypatch):
    """any step towards the device fails the test: the refusals must come first"""
    from salient_plusplus_amd import _native as nat

    def touched(*_a, **_k):
        raise AssertionError("a device call was made before the arguments were refused")
    monkeypatch.setattr(nat, "require_device", touched)


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def _call(nat, L, entry, scale=_FAKE, ws=_FAKE, nbytes=None, **over):
    """a call of ``entry`` that passes every check -- ten rows of F = 32 e4m3 columns, the slab of the first four
    targets, with parts the rows [0, 4) and [4, 10) -- altered by ``over``"""
    parts = "parts" in entry
    kw = dict(epilogue=nat.SPP_AGG_MEAN, x_elem=nat.SPP_ELEM_FP8_E4M3, out_elem=nat.SPP_ELEM_F32, rowptr_dev=_FAKE,
              col_dev=_FAKE, x_stride_elems=32, F=32, target_row0=0, target_ids_dev=None, num_targets=4, out_dev=_FAKE,
              out_stride_elems=0)
    kw.update(dict(num_parts=2) if parts else dict(x_dev=_FAKE, x_rows=10))
    bases = over.pop("bases", (_FAKE, 2 * _FAKE))
    kw.update(over)
    d = (nat.GraphAggPartsDesc if parts else nat.GraphAggDesc)(**kw)
    if parts:
        for i, v in enumerate((0, 4, 10)):
            d.part_offsets[i] = v
        for i, v in enumerate(bases):
            d.x_parts_dev[i] = v or None
    if nbytes is None:
        nbytes = 16 + 8 * max(int(d.num_targets), 0)
    return getattr(L, entry)(ctypes.byref(d), ctypes.c_void_p(scale), ctypes.c_void_p(ws), nbytes, None)


# (class, changes of the call, the word of the class)
AGG_REFUSALS = [
    ("fp32 rows", dict(x_elem=0), b"x_elem 0"),
    ("fp16 rows", dict(x_elem=1), b"x_elem 1"),
    ("bf16 rows", dict(x_elem=2), b"x_elem 2"),
    ("unknown x element code", dict(x_elem=9), b"x_elem 9"),
    ("NULL exponents", dict(scale=None), b"scale_log2_dev"),
    ("misaligned exponents", dict(scale=_FAKE + 2), b"scale_log2_dev"),
    ("F no multiple of 16", dict(F=24), b"multiple of 16"),
    ("fp8 output", dict(out_elem=3), b"out_elem 3"),
    ("fp16 output", dict(out_elem=1), b"element code"),
    ("a row stride that is no multiple of 4 bytes", dict(x_stride_elems=34), b"multiple of 4"),
    ("x stride too small", dict(x_stride_elems=16), b"smaller than the row"),
    ("unknown epilogue", dict(epilogue=2), b"epilogue"),
    ("slab and list both", dict(target_ids_dev=_FAKE), b"not both"),
    ("slab leaves the graph", dict(target_row0=8, num_targets=4), b"leaves the graph's 10 rows"),
    ("missing workspace", dict(ws=None, nbytes=0), b"workspace"),
    ("NULL out", dict(out_dev=None), b"NULL buffer"),
    ("misaligned out", dict(out_dev=_FAKE + 4), b"aligned to 4 elements"),
]
WHOLE_REFUSALS = [("NULL table", dict(x_dev=None), b"NULL buffer"),
                  ("a base that is no multiple of 4 bytes", dict(x_dev=_FAKE + 2), b"multiple of 4")]
PARTS_REFUSALS = [("too many parts", dict(num_parts=17), b"num_parts 17"),
                  ("NULL base of a non-empty part", dict(bases=(_FAKE, 0)), b"part 1"),
                  ("a part's base that is no multiple of 4 bytes", dict(bases=(_FAKE, 2 * _FAKE + 1)), b"multiple of 4")]
CASES = ([(e, *r) for e in AGG_ENTRIES for r in AGG_REFUSALS] + [(AGG_ENTRIES[0], *r) for r in WHOLE_REFUSALS]
         + [(AGG_ENTRIES[1], *r) for r in PARTS_REFUSALS])


@pytest.mark.parametrize("entry,what,over,word", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_fp8_aggregation_entries_refuse_by_status_and_name(entry, what, over, word):
    nat, L = _lib()
    assert _call(nat, L, entry, **over) == SPP_ERR_INVALID, what
    msg = L.spp_last_error()
    assert msg.startswith(entry.encode() + b":") and word in msg, (what, msg)


@pytest.mark.parametrize("entry", AGG_ENTRIES)
def test_empty_fp8_calls_return_ok_and_null_descriptors_do_not(entry):
    nat, L = _lib()
    for over in (dict(num_targets=0), dict(F=0), dict(num_targets=0, rowptr_dev=None, col_dev=None, out_dev=None)):
        assert _call(nat, L, entry, **over) == SPP_OK, (over, L.spp_last_error())
    assert getattr(L, entry)(None, ctypes.c_void_p(_FAKE), ctypes.c_void_p(_FAKE), 48, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()


def test_the_entries_without_fp8_keep_refusing_e4m3_rows():
    nat, L = _lib()
    for entry in ("spp_graph_agg_forward", "spp_graph_agg_parts_forward"):
        parts = "parts" in entry
        kw = dict(epilogue=nat.SPP_AGG_MEAN, x_elem=nat.SPP_ELEM_FP8_E4M3, out_elem=nat.SPP_ELEM_F32, rowptr_dev=_FAKE,
                  col_dev=_FAKE, x_stride_elems=32, F=32, target_row0=0, num_targets=4, out_dev=_FAKE)
        kw.update(dict(num_parts=1) if parts else dict(x_dev=_FAKE, x_rows=10))
        d = (nat.GraphAggPartsDesc if parts else nat.GraphAggDesc)(**kw)
        if parts:
            d.part_offsets[1], d.x_parts_dev[0] = 10, _FAKE
        assert getattr(L, entry)(ctypes.byref(d), ctypes.c_void_p(_FAKE), 48, None) == SPP_ERR_INVALID
        msg = L.spp_last_error()
        assert msg.startswith(entry.encode() + b":") and b"fp8 rows are not read or written here" in msg \
            and b"dequantise the table first" in msg, msg


ROWS_REFUSALS = [  # (q, src_rows, F, scale, row0, ids, n, dst), the word of the refusal
    ((_FAKE, 10, 24, _FAKE, 0, None, 4, _FAKE), b"multiple of 16"),
    ((_FAKE, 10, 32, _FAKE, 0, _FAKE, 4, _FAKE), b"not both"),
    ((_FAKE, 10, 32, _FAKE, -1, None, 4, _FAKE), b"one of them"),
    ((_FAKE, 10, 32, _FAKE, 8, None, 4, _FAKE), b"leaves the table's 10 rows"),
    ((_FAKE, 10, 32, _FAKE, 0, None, -4, _FAKE), b"negative size"),
    ((_FAKE, 10, -32, _FAKE, 0, None, 4, _FAKE), b"negative size"),
    ((None, 10, 32, _FAKE, 0, None, 4, _FAKE), b"NULL buffer"),
    ((_FAKE, 10, 32, None, 0, None, 4, _FAKE), b"NULL buffer"),
    ((_FAKE, 10, 32, _FAKE, 0, None, 4, None), b"NULL buffer"),
    ((_FAKE, 0, 32, _FAKE, -1, _FAKE, 4, _FAKE), b"empty table"),
    ((_FAKE + 8, 10, 32, _FAKE, 0, None, 4, _FAKE), b"aligned"),
    ((_FAKE, 10, 32, _FAKE + 1, 0, None, 4, _FAKE), b"aligned"),
    ((_FAKE, 10, 32, _FAKE, 0, None, 4, _FAKE + 4), b"aligned"),
]


@pytest.mark.parametrize("args,word", ROWS_REFUSALS, ids=[f"{i}-{c[1].decode()}" for i, c in enumerate(ROWS_REFUSALS)])
def test_fp8_rows_f32_refuses_by_status_and_name(args, word):
    _nat, L = _lib()
    assert L.spp_fp8_rows_f32(*args, None) == SPP_ERR_INVALID
    msg = L.spp_last_error()
    assert msg.startswith(b"spp_fp8_rows_f32:") and word in msg, msg


def test_fp8_rows_f32_empty_calls_return_ok():
    _nat, L = _lib()
    for args in ((_FAKE, 10, 32, _FAKE, 0, None, 0, _FAKE), (_FAKE, 10, 0, _FAKE, 0, None, 4, _FAKE),
                 (None, 10, 32, None, 10, None, 0, None), (None, 0, 32, None, -1, _FAKE, 0, None)):
        assert L.spp_fp8_rows_f32(*args, None) == SPP_OK, (args, L.spp_last_error())


def _tiny():
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import Fp8Table
    x8 = fp8.quantize_e4m3(torch.arange(48, dtype=torch.float32).view(3, 16))
    return x8, Fp8Table(x8), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])


def test_fp8table_type_checks():
    from salient_plusplus_amd.inference import Fp8Table
    x8, t, _rowptr, _col = _tiny()
    for bad in (torch.zeros((3, 16)), x8.q, None, t):
        with pytest.raises(TypeError, match="wraps an Fp8Features"):
            Fp8Table(bad)
    assert t.features is x8 and t.q is x8.q and t.scale_log2 is x8.scale_log2
    assert tuple(t.shape) == (3, 16) and t.size(0) == 3 and t.size(1) == 16 and t.dim() == 2
    assert t.device == x8.q.device and not t.is_cuda and t.dtype == torch.float8_e4m3fn and not t.requires_grad
    rows = t[torch.tensor([2, 2, 0, 1])]
    assert tuple(rows.shape) == (4, 16) and rows.features is x8
    for bad in (slice(0, 2), 1, torch.tensor([0], dtype=torch.int32), torch.tensor([[0]])):
        with pytest.raises(TypeError, match="1-D int64"):
            t[bad]
    with pytest.raises(TypeError, match="1-D int64"):
        rows[torch.tensor([0])]


def test_entries_that_read_the_table_in_place_take_whole_tables_only(no_device):
    from salient_plusplus_amd.inference import evaluate, field_inference, graph_aggregate, graph_aggregate_parts, \
        layerwise_inference
    from salient_plusplus_amd.models import SAGE
    x8, t, rowptr, col = _tiny()
    rows = t[torch.tensor([0, 1, 2])]
    sage = SAGE(16, 4, 2, 2)
    with pytest.raises(TypeError, match="whole Fp8Table"):
        graph_aggregate(rows, rowptr, col, row0=0, num_targets=3)
    with pytest.raises(TypeError, match="whole Fp8Table"):
        layerwise_inference(sage, rows, rowptr, col)
    with pytest.raises(TypeError, match="whole Fp8Table"):
        evaluate(sage, rows, rowptr, col)
    with pytest.raises(TypeError, match="whole Fp8Table"):
        field_inference(sage, rows, rowptr, col, torch.tensor([0]))
    with pytest.raises(TypeError, match="EVERY part is a whole Fp8Table"):
        graph_aggregate_parts([t, torch.zeros((0, 16))], [0, 3, 3], rowptr, col, row0=0, num_targets=3)
    with pytest.raises(TypeError, match="EVERY part is a whole Fp8Table"):
        graph_aggregate_parts([rows], [0, 3], rowptr, col, row0=0, num_targets=3)
    # the argument checks behind the table are the same ones, and come before the device
    with pytest.raises(ValueError, match="one row per node"):
        graph_aggregate(t, rowptr[:-1], col, row0=0, num_targets=1)
    with pytest.raises(ValueError, match="out_dtype"):
        graph_aggregate(t, rowptr, col, row0=0, num_targets=3, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="part 0 has 3 rows, part_offsets gives it 2"):
        graph_aggregate_parts([t, None], [0, 2, 2], rowptr, col, row0=0, num_targets=2)
    with pytest.raises(ValueError, match="act_dtype"):
        layerwise_inference(sage, t, rowptr, col, act_dtype=torch.float16)


def test_entries_that_do_not_read_an_fp8_table_refuse_fp8table_with_a_reason(no_device):
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GAT, SAGE
    _x8, t, rowptr, col = _tiny()
    a = torch.zeros((3, 1))
    peers = inf.LocalPeers(1)
    part = dict(part_offsets=[0, 3], rank=0, peers=peers)
    for call in (lambda: inf.partitioned_inference(SAGE(16, 4, 2, 2), t, rowptr, col, **part),
                 lambda: inf.partitioned_evaluate(SAGE(16, 4, 2, 2), t, rowptr, col, **part),
                 lambda: inf.partitioned_layerwise_inference(SAGE(16, 4, 2, 2), t, rowptr, col, **part),
                 lambda: inf.partitioned_inference(GAT(16, 4, 2, 2), t, rowptr, col, **part)):
        with pytest.raises(TypeError, match="x_local is an Fp8Table.*peers.share"):
            call()
    with pytest.raises(TypeError, match="x is an Fp8Table.*read in place only as.*projected rows"):
        inf.graph_gat_aggregate(t, a, a, rowptr, col, heads=1, row0=0, num_targets=3)
    with pytest.raises(TypeError, match="part 0 is an Fp8Table.*projected rows"):
        inf.graph_gat_aggregate_parts([t], [a.repeat(1, 2)], [0, 3], rowptr, col, heads=1, row0=0, num_targets=3)
    z = torch.zeros((3, 16))
    with pytest.raises(TypeError, match="z is an Fp8Table"):
        inf.resinc_epilogue(t, torch.ones(16), torch.zeros(16), negative_slope=0.01)
    with pytest.raises(TypeError, match="residual is an Fp8Table.*activations"):
        inf.resinc_epilogue(z, torch.ones(16), torch.zeros(16), negative_slope=0.01, residual=t, row0=0)
    with pytest.raises(TypeError, match="z is an Fp8Table"):
        inf.classify_rows(t)


def test_a_bare_fp8features_keeps_raising_the_pinned_messages(no_device):
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GIN, SAGE
    x8, _t, rowptr, col = _tiny()
    sage = SAGE(16, 4, 2, 2)
    part = dict(part_offsets=[0, 3], rank=0, peers=inf.LocalPeers(1))
    calls = [lambda: inf.graph_aggregate(x8, rowptr, col, row0=0, num_targets=1),
             lambda: inf.graph_aggregate_parts([x8], [0, 3], rowptr, col, row0=0, num_targets=1),
             lambda: inf.layerwise_inference(sage, x8, rowptr, col),
             lambda: sage.inference(x8, rowptr, col),
             lambda: GIN(16, 4, 2, 2).inference(x8, rowptr, col),
             lambda: inf.evaluate(sage, x8, rowptr, col),
             lambda: inf.field_inference(sage, x8, rowptr, col, torch.tensor([0])),
             lambda: inf.field_evaluate(sage, x8, rowptr, col, nodes=torch.tensor([0])),
             lambda: inf.partitioned_inference(sage, x8, rowptr, col, **part),
             lambda: inf.graph_gat_aggregate(x8, torch.zeros((3, 1)), torch.zeros((3, 1)), rowptr, col, heads=1, row0=0,
                                             num_targets=1),
             lambda: inf.resinc_epilogue(x8, torch.ones(16), torch.zeros(16), negative_slope=0.01)]
    for call in calls:
        with pytest.raises(TypeError, match=r"an fp8 feature table \(Fp8Features\) is not supported as inference input; "
                                            r"pass x.dequantize\(torch.float16\)") as e:
            call()
        assert str(e.value).endswith("Fp8Table(x) where the table is read in place")
