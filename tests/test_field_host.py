"""CPU-only: the host side of the receptive field (f3n) -- the ctypes layout of spp_field_desc against the header, the
exported entries, every refusal of spp_field_mark and spp_field_rows (status -1, a message that starts with the entry's own
name; made before anything is enqueued, so fake pointers do and no GPU is needed), the empty calls, and the argument
validation of ReceptiveFields, receptive_field, field_inference and field_evaluate before any device call."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FAKE = 0x10000                                               # 16-byte aligned, never dereferenced
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)
ENTRIES = ["spp_field_mark", "spp_field_rows"]


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


def test_field_desc_layout_matches_header():
    """sizeof and every field offset of spp_field_desc, in the header's order, cross-checked with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.FieldDesc._fields_]
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = header[header.index("typedef struct spp_field_desc {"):header.index("} spp_field_desc;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == names
    offs = ", ".join(f"offsetof(spp_field_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_field_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [getattr(nat.FieldDesc, n).offset for n in names]
    assert got == [ctypes.sizeof(nat.FieldDesc)] + offsets and offsets == sorted(offsets)


def test_library_exports_the_entries_and_keeps_its_abi_version():
    nat, L = _lib()
    for name in ENTRIES:
        assert hasattr(L, name) and nat.SIGNATURES[name][1][0]._type_ is nat.FieldDesc
    assert L.spp_abi_version() == 6
    # the cut is exported as the other families export theirs, and the workspace is graph_rows' list: 16 + 8 a row
    assert L.spp_field_chunk() >= 32
    assert [L.spp_field_workspace_bytes(n) for n in (-3, 0, 1, 1000)] == [16, 16, 24, 8016]
    from salient_plusplus_amd.inference import field_chunk, field_workspace_bytes
    assert field_chunk() == L.spp_field_chunk() and field_workspace_bytes(7) == 72


def _desc(nat, entry, **over):
    """a descriptor that passes every check of ``entry``: four ids over a graph of ten nodes; ``over`` alters it"""
    kw = dict(rowptr_dev=_FAKE, col_dev=_FAKE, num_nodes=10, ids_dev=_FAKE, num_ids=4, slot_dev=_FAKE)
    kw.update(dict(flag_dev=_FAKE) if entry == "spp_field_mark" else dict(frowptr_dev=_FAKE, fcol_dev=_FAKE, fcol_len=12))
    kw.update(over)
    return nat.FieldDesc(**kw)


def _call(nat, L, entry, over, ws=_FAKE, nbytes=None):
    d = _desc(nat, entry, **over)
    if nbytes is None:
        nbytes = 16 + 8 * max(int(d.num_ids), 0)              # spp_field_workspace_bytes(num_ids)
    return getattr(L, entry)(ctypes.byref(d), ctypes.c_void_p(ws), nbytes, None)


# (class, descriptor changes, workspace changes, the word of the class)
SHARED_REFUSALS = [
    ("negative num_nodes", dict(num_nodes=-1), {}, b"negative size"),
    ("negative num_ids", dict(num_ids=-1), {}, b"negative size"),
    ("negative fcol_len", dict(fcol_len=-1), {}, b"negative size"),
    ("missing workspace", {}, dict(ws=None, nbytes=0), b"workspace"),
    ("short workspace", {}, dict(nbytes=16 + 8 * 3), b"workspace"),
    ("misaligned workspace", {}, dict(ws=_FAKE + 8), b"workspace"),
    ("NULL rowptr", dict(rowptr_dev=None), {}, b"NULL buffer"),
    ("NULL col", dict(col_dev=None), {}, b"NULL buffer"),
    ("NULL ids", dict(ids_dev=None), {}, b"NULL buffer"),
    ("NULL slot", dict(slot_dev=None), {}, b"NULL buffer"),
    ("empty graph", dict(num_nodes=0), {}, b"empty graph"),
]
OWN_REFUSALS = {
    "spp_field_mark": [("NULL flag", dict(flag_dev=None), {}, b"flag_dev")],
    "spp_field_rows": [("NULL frowptr", dict(frowptr_dev=None), {}, b"frowptr_dev"),
                       ("NULL fcol", dict(fcol_dev=None), {}, b"fcol_dev")],
}
CASES = [(e, *r) for e in ENTRIES for r in SHARED_REFUSALS + OWN_REFUSALS[e]]


@pytest.mark.parametrize("entry,what,over,call,word", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_both_entries_refuse_every_class_by_their_own_name(entry, what, over, call, word):
    nat, L = _lib()
    assert _call(nat, L, entry, over, **call) == SPP_ERR_INVALID, what
    msg = L.spp_last_error()
    assert msg.startswith(entry.encode() + b":") and word in msg, (what, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_descriptor_is_refused(entry):
    nat, L = _lib()
    assert getattr(L, entry)(None, ctypes.c_void_p(_FAKE), 64, None) == SPP_ERR_INVALID
    assert L.spp_last_error().startswith(entry.encode() + b": NULL descriptor")


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_calls_return_ok_before_any_buffer_is_looked_at(entry):
    nat, L = _lib()
    nothing = dict(rowptr_dev=None, col_dev=None, ids_dev=None, slot_dev=None, flag_dev=None, frowptr_dev=None,
                   fcol_dev=None, fcol_len=0)
    for over in (dict(num_ids=0), dict(num_ids=0, num_nodes=0), dict(num_ids=0, **nothing)):
        assert _call(nat, L, entry, over) == SPP_OK, (over, L.spp_last_error())
    if entry == "spp_field_rows":                             # rows without entries need no fcol
        assert _call(nat, L, entry, dict(fcol_dev=None, fcol_len=0, num_ids=0)) == SPP_OK


# ---- the Python layer: everything is refused before the device is required ------------------------------------------
def _graph(N=6):
    rowptr = torch.arange(0, 2 * N + 1, 2, dtype=torch.int64)
    col = torch.arange(2 * N, dtype=torch.int64) % N
    return rowptr, col


def _sage(layers=2):
    from salient_plusplus_amd.models import SAGE
    return SAGE(4, 8, 3, layers)


BAD_NODES = [
    (TypeError, [0, 1]),
    (ValueError, torch.tensor([0, 1], dtype=torch.int32)),
    (ValueError, torch.tensor([[0, 1]], dtype=torch.int64)),
    (ValueError, torch.tensor([0, 6], dtype=torch.int64)),
    (ValueError, torch.tensor([-1, 2], dtype=torch.int64)),
]


@pytest.mark.parametrize("exc,nodes", BAD_NODES, ids=["list", "int32", "2-D", "above", "below"])
def test_bad_nodes_are_refused_by_name_before_the_device(no_device, exc, nodes):
    from salient_plusplus_amd import inference as inf
    rowptr, col = _graph()
    x = torch.zeros((6, 4), dtype=torch.float16)
    with pytest.raises(exc, match=r"^receptive_field: nodes"):
        inf.receptive_field(rowptr, col, nodes, 1)
    with pytest.raises(exc, match=r"^field_inference: nodes"):
        inf.field_inference(_sage(), x, rowptr, col, nodes)
    with pytest.raises(exc, match=r"^field_evaluate: (nodes|splits)"):
        inf.field_evaluate(_sage(), x, rowptr, col, nodes=nodes)
    # ReceptiveFields.field: the object exists only on a device, but its checks are the same function
    with pytest.raises(exc, match=r"^ReceptiveFields.field: nodes"):
        inf._check_nodes("ReceptiveFields.field", nodes, 6)


def test_bad_hops_graphs_and_runs_are_refused_before_the_device(no_device):
    from salient_plusplus_amd import inference as inf
    rowptr, col = _graph()
    nodes = torch.tensor([0, 3], dtype=torch.int64)
    x = torch.zeros((6, 4), dtype=torch.float16)
    with pytest.raises(ValueError, match=r"^receptive_field: hops must not be negative"):
        inf.receptive_field(rowptr, col, nodes, -1)
    for hops in (1.0, "2", None, True):
        with pytest.raises(TypeError, match=r"^receptive_field: hops must be an int"):
            inf.receptive_field(rowptr, col, nodes, hops)
    with pytest.raises(ValueError, match=r"^receptive_field: rowptr must be a contiguous 1-D int64"):
        inf.receptive_field(rowptr.to(torch.int32), col, nodes, 1)
    with pytest.raises(ValueError, match=r"^ReceptiveFields: col must be a contiguous 1-D int64"):
        inf.ReceptiveFields(rowptr, col.view(-1, 2))
    # a field of the wrong depth for the model: the plan checks hops against the layers
    f = inf.Field(nodes, [2, 2], torch.arange(2), torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="3 conv layers is scored over a field of 2 hops, got one of 1"):
        inf._field_plan(f, 3)
    m = _sage()
    with pytest.raises(ValueError, match=r"^field_inference: x has 6 rows, the graph 5 nodes"):
        inf.field_inference(m, x, rowptr[:-1], col, nodes)
    with pytest.raises(ValueError, match=r"^field_inference: act_dtype"):
        inf.field_inference(m, x, rowptr, col, nodes, act_dtype=torch.float16)
    with pytest.raises(ValueError, match=r"^field_inference: rows_per_slab must be positive"):
        inf.field_inference(m, x, rowptr, col, nodes, rows_per_slab=0)
    with pytest.raises(TypeError, match=r"^field_inference: fields must be a ReceptiveFields"):
        inf.field_inference(m, x, rowptr, col, nodes, fields=object())
    with pytest.raises(ValueError, match=r"^field_evaluate: give nodes or splits"):
        inf.field_evaluate(m, x, rowptr, col)
    with pytest.raises(ValueError, match=r"^field_evaluate: give either nodes or splits, not both"):
        inf.field_evaluate(m, x, rowptr, col, nodes=nodes, splits={"a": nodes})
    with pytest.raises(ValueError, match=r"^field_evaluate: y must be a contiguous int64 tensor of shape \[6\]"):
        inf.field_evaluate(m, x, rowptr, col, torch.zeros(5, dtype=torch.int64), nodes=nodes)


def test_fp8_partitioned_and_resinception_inputs_are_refused_with_a_reason(no_device):
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd import fp8 as fp8_mod
    from salient_plusplus_amd.models import SAGEResInception
    rowptr, col = _graph()
    nodes = torch.tensor([0, 3], dtype=torch.int64)
    x = torch.zeros((6, 4), dtype=torch.float16)
    fp8 = fp8_mod.quantize_e4m3(torch.zeros((6, 16)))
    for fn, kw in ((inf.field_inference, dict(nodes=nodes)), (inf.field_evaluate, dict(nodes=nodes))):
        name = fn.__name__
        with pytest.raises(TypeError, match=rf"^{name}: an fp8 feature table"):
            fn(_sage(), fp8, rowptr, col, **kw)
        with pytest.raises(NotImplementedError, match=rf"^{name}: a row-partitioned table is not scored over a receptive "
                                                      "field"):
            fn(_sage(), [x[:3], x[3:]], rowptr, col, **kw)
        with pytest.raises(NotImplementedError, match=rf"^{name}: SAGEResInception is not scored over a receptive field"):
            fn(SAGEResInception(4, 8, 3, 2), x, rowptr, col, **kw)
        with pytest.raises(NotImplementedError, match=rf"^{name}: implemented for SAGE, GIN and GAT"):
            fn(torch.nn.Linear(4, 3), x, rowptr, col, **kw)


def test_valid_arguments_reach_the_device_and_no_further():
    """with every argument in order the first thing asked for is the device: without one that is the error"""
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import inference as inf
    rowptr, col = _graph()
    nodes = torch.tensor([0, 3], dtype=torch.int64)
    m = _sage()
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        with pytest.raises(nat.SppError):
            inf.field_inference(m, torch.zeros((6, 4), dtype=torch.float16), rowptr, col, nodes)
        with pytest.raises(nat.SppError):
            inf.receptive_field(rowptr, col, nodes, 2)
    assert m.training                                         # a refused call leaves the mode alone
