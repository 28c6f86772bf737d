"""CPU-only: the host side of GAT attention and of GAT / SAGEResInception inference over a row-partitioned table -- the
ctypes layout of spp_graph_gat_parts_desc against the header, every refusal of spp_graph_gat_parts_forward by message
(the entry validates before it touches a device; the refusals it inherits show that it runs through
spp_graph_gat_forward's checks), the Python checks of inference.graph_gat_aggregate_parts and of
inference.partitioned_inference, made before the device and before ``peers`` is touched."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FAKE = 0x10000
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)


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


def test_graph_gat_parts_desc_layout_matches_header():
    """sizeof and every field offset, cross-checked by compiling the header with gcc; the older descriptors and the ABI
    version are as they were"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.GraphGatPartsDesc._fields_]
    offs = ", ".join(f"offsetof(spp_graph_gat_parts_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_graph_gat_parts_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(nat.GraphGatPartsDesc)] + [getattr(nat.GraphGatPartsDesc, n).offset for n in names]
    _nat, L = _lib()
    assert hasattr(L, "spp_graph_gat_parts_forward") and "spp_graph_gat_parts_forward" in nat.SIGNATURES
    assert L.spp_abi_version() == 6


def _desc(nat, offsets=(0, 4, 10), h=(_FAKE, 2 * _FAKE), a=(3 * _FAKE, 4 * _FAKE), **over):
    """a descriptor that passes every check (two parts, ten rows, F = 8 in two heads); no pointer is dereferenced by a
    refusal, and nothing is enqueued"""
    kw = dict(x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, heads=2, relu=0, num_parts=len(offsets) - 1,
              rowptr_dev=_FAKE, col_dev=_FAKE, x_stride_elems=8, a_stride_elems=0, F=8, target_row0=0,
              target_ids_dev=None, num_targets=4, out_dev=_FAKE, out_stride_elems=0, negative_slope=0.2)
    kw.update(over)
    d = nat.GraphGatPartsDesc(**kw)
    for i, v in enumerate(offsets):
        d.part_offsets[i] = v
    for i, (hv, av) in enumerate(zip(h, a)):
        d.h_parts_dev[i], d.a_parts_dev[i] = hv or None, av or None
    return d


OWN_REFUSALS = [
    ("no parts", dict(num_parts=0), b"num_parts 0"),
    ("too many parts", dict(num_parts=17), b"num_parts 17"),
    ("offsets do not start at 0", dict(offsets=(1, 4, 10)), b"part_offsets[0]"),
    ("offsets decrease", dict(offsets=(0, 5, 4)), b"part_offsets decrease"),
    ("NULL h base of a non-empty part", dict(h=(_FAKE, 0)), b"h_parts_dev"),
    ("NULL logits base of a non-empty part", dict(a=(0, 4 * _FAKE)), b"a_parts_dev"),
    ("logits stride below 2 * heads", dict(a_stride_elems=3), b"a_stride_elems"),
    ("negative logits stride", dict(a_stride_elems=-4), b"a_stride_elems"),
]
# one refusal of spp_graph_gat_forward per class: the new entry runs through the same validated path
INHERITED_REFUSALS = [
    ("fp8 rows", dict(x_elem="FP8_E4M3"), {}, b"fp8"),
    ("fp16 output", dict(out_elem="F16"), {}, b"out_elem"),
    ("heads does not divide F", dict(heads=3), {}, b"heads"),
    ("small workspace", {}, dict(bytes=8), b"workspace"),
    ("misaligned workspace", {}, dict(ws=_FAKE + 8), b"workspace"),
    ("both target forms", dict(target_ids_dev=_FAKE), {}, b"not both"),
    ("neither target form", dict(target_row0=-1), {}, b"one of them"),
    ("slab outside the graph", dict(target_row0=8, num_targets=4), {}, b"leaves the graph's 10 rows"),
    ("row stride smaller than the row", dict(x_stride_elems=7), {}, b"x_stride_elems"),
    ("output stride smaller than the row", dict(out_stride_elems=4), {}, b"out_stride_elems"),
    ("misaligned output base (vector form)", dict(out_dev=_FAKE + 4), {}, b"out_dev"),
]


def _refused(nat, L, over, call, word, what):
    over = {k: getattr(nat, "SPP_ELEM_" + v) if isinstance(v, str) else v for k, v in over.items()}
    d = _desc(nat, **over)
    ws = call.get("ws", _FAKE)
    nbytes = call.get("bytes", int(L.spp_graph_gat_workspace_bytes(max(d.num_targets, 0))))
    assert L.spp_graph_gat_parts_forward(ctypes.byref(d), ctypes.c_void_p(ws), nbytes, None) == SPP_ERR_INVALID, what
    msg = L.spp_last_error()
    assert msg.startswith(b"spp_graph_gat_parts_forward") and word in msg, (what, msg)


@pytest.mark.parametrize("what,over,word", OWN_REFUSALS, ids=[r[0] for r in OWN_REFUSALS])
def test_entry_refuses_a_bad_parts_form_before_anything_is_enqueued(what, over, word):
    nat, L = _lib()
    _refused(nat, L, over, {}, word, what)


@pytest.mark.parametrize("what,over,call,word", INHERITED_REFUSALS, ids=[r[0] for r in INHERITED_REFUSALS])
def test_entry_refuses_what_the_whole_matrix_entry_refuses(what, over, call, word):
    nat, L = _lib()
    _refused(nat, L, over, call, word, what)


def test_entry_refuses_a_null_descriptor_and_accepts_empty_calls():
    nat, L = _lib()
    assert L.spp_graph_gat_parts_forward(None, ctypes.c_void_p(_FAKE), 1 << 20, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    # T == 0 or F == 0: nothing to do, SPP_OK without touching a device or a buffer; an empty part may have NULL bases
    for over in (dict(num_targets=0), dict(F=0, x_stride_elems=0),
                 dict(num_targets=0, offsets=(0, 0, 10, 10), h=(0, _FAKE, 0), a=(0, _FAKE, 0)),
                 dict(num_targets=0, a_stride_elems=4), dict(num_targets=0, a_stride_elems=32)):
        d = _desc(nat, **over)
        assert L.spp_graph_gat_parts_forward(ctypes.byref(d), ctypes.c_void_p(_FAKE), 1 << 10, None) == SPP_OK, over


def _tiny(F=8, heads=2):
    h = torch.zeros((4, F), dtype=torch.float16)
    a = torch.zeros((4, 2 * heads))
    return [h[:2], h[2:]], [a[:2], a[2:]], [0, 2, 4], torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, 1, 2, 3])


def test_graph_gat_aggregate_parts_validates_its_arguments(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import P2PPeers, RowRefs, TableRows
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts as gap
    hp, ap, off, rowptr, col = _tiny()
    slab = dict(heads=2, row0=0, num_targets=4)
    with pytest.raises(ValueError, match="part_offsets must hold"):
        gap(hp, ap, [0], rowptr, col, **slab)
    with pytest.raises(ValueError, match="start at 0 and never decrease"):
        gap(hp, ap, [0, 3, 2], rowptr, col, **slab)
    with pytest.raises(ValueError, match="3 parts for 2 ranges"):                      # part count against offsets
        gap(hp + [None], ap, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="3 parts for 2 ranges"):
        gap(hp, ap + [None], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="part 1 has 2 rows"):
        gap(hp, ap, [0, 2, 5], rowptr, col, **slab)
    with pytest.raises(ValueError, match="part 1 holds the rows .* and is None"):      # a None part that holds rows
        gap([hp[0], None], ap, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="logits part 0 holds the rows .* and is None"):
        gap(hp, [None, ap[1]], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one dtype and one row width"):               # mixed dtypes
        gap([hp[0], hp[1].float()], ap, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one dtype and one row width"):               # mixed widths
        gap([hp[0], hp[1][:, :4]], ap, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one row stride"):                            # mixed strides
        gap([hp[0], torch.zeros((2, 16), dtype=torch.float16)[:, :8]], ap, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one row stride"):
        gap(hp, [ap[0], torch.zeros((2, 8))[:, :4]], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match=r"fp32 matrix \[rows, 2 \* heads = 4\]"):     # logits of the wrong type or width
        gap(hp, [t.half() for t in ap], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match=r"fp32 matrix \[rows, 2 \* heads = 4\]"):
        gap(hp, [t[:, :2] for t in ap], off, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="logits part 1 requires grad"):
        gap(hp, [ap[0], ap[1].clone().requires_grad_()], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="heads"):
        gap(hp, ap, off, rowptr, col, heads=3, row0=0, num_targets=4)
    with pytest.raises(ValueError, match="heads"):
        gap(hp, ap, off, rowptr, col, heads=0, row0=0, num_targets=4)
    with pytest.raises(TypeError, match="fp8"):
        gap([hp[0], fp8.quantize_e4m3(torch.zeros((2, 16)))], ap, off, rowptr, col, **slab)
    with pytest.raises(TypeError, match="TableRows"):
        gap([hp[0], TableRows(hp[1], torch.tensor([0]))], ap, off, rowptr, col, **slab)
    with pytest.raises(TypeError, match="RowRefs"):
        gap([hp[0], RowRefs(torch.zeros(2, dtype=torch.int64), None, 8, torch.float16, None, ())], ap, off, rowptr, col,
            **slab)
    with pytest.raises(ValueError, match="2-D"):
        gap([hp[0], hp[1].double()], ap, off, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="requires grad"):
        gap([hp[0], hp[1].clone().requires_grad_()], ap, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one row per node"):
        gap(hp, ap, off, rowptr[:-1], col, **slab)
    with pytest.raises(ValueError, match="int64"):
        gap(hp, ap, off, rowptr, col.int(), **slab)
    with pytest.raises(ValueError, match="not both"):
        gap(hp, ap, off, rowptr, col, target_ids=torch.tensor([0]), **slab)
    with pytest.raises(ValueError, match="either as a slab"):
        gap(hp, ap, off, rowptr, col, heads=2)
    with pytest.raises(ValueError, match="both row0 and num_targets"):
        gap(hp, ap, off, rowptr, col, heads=2, row0=0)
    with pytest.raises(ValueError, match="leaves the graph"):
        gap(hp, ap, off, rowptr, col, heads=2, row0=3, num_targets=2)
    with pytest.raises(ValueError, match="target_ids"):
        gap(hp, ap, off, rowptr, col, heads=2, target_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="out_dtype"):
        gap(hp, ap, off, rowptr, col, out_dtype=torch.float16, **slab)
    with pytest.raises(ValueError, match="out must be"):
        gap(hp, ap, off, rowptr, col, out=torch.zeros((4, 9)), **slab)
    # the P2PPeers forms: addresses only, so h's element type and width come from the caller; logits are fp32 [., 2H]
    peers, apeers = P2PPeers([0x1000, 0x2000], 16), P2PPeers([0x3000, 0x4000], 16)
    with pytest.raises(ValueError, match="needs dtype="):
        gap(peers, apeers, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="peer tables for 3 parts"):
        gap(peers, apeers, [0, 2, 4, 4], rowptr, col, dtype=torch.float16, F=8, **slab)
    with pytest.raises(ValueError, match="logits part 1 holds the rows .* has no address"):
        gap(peers, P2PPeers([0x3000, 0], 16), off, rowptr, col, dtype=torch.float16, F=8, **slab)
    with pytest.raises(ValueError, match="no multiple of the element size"):
        gap(peers, P2PPeers([0x3000, 0x4000], 18), off, rowptr, col, dtype=torch.float16, F=8, **slab)
    with pytest.raises(ValueError, match="smaller than 2 \\* heads"):
        gap(peers, P2PPeers([0x3000, 0x4000], 8), off, rowptr, col, dtype=torch.float16, F=8, **slab)
    with pytest.raises(ValueError, match="describe a P2PPeers source"):
        gap(hp, ap, off, rowptr, col, dtype=torch.float16, **slab)


def test_valid_arguments_need_the_device():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts as gap
    hp, ap, off, rowptr, col = _tiny()
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        with pytest.raises(nat.SppError):
            gap(hp, ap, off, rowptr, col, heads=2, row0=0, num_targets=4)
    else:                                                     # host tensors are refused where the device is there
        with pytest.raises(ValueError, match="one CUDA device"):
            gap(hp, ap, off, rowptr, col, heads=2, row0=0, num_targets=4)


class _NoPeers:
    def share(self, t):
        raise AssertionError("refused calls publish nothing")

    barrier = close = bind = abort = share


def test_partitioned_inference_refuses_before_the_device_and_before_peers(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import partitioned_inference as pinf
    from salient_plusplus_amd.models import GAT, GATConv, MLP, SAGE, SAGEResInception
    x = torch.zeros((4, 8), dtype=torch.float16)[2:]
    off, rowptr, col = [0, 2, 4], torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, 1, 2, 3])
    kw = dict(part_offsets=off, rank=1, peers=_NoPeers())
    with pytest.raises(NotImplementedError, match="SAGE, GIN, GAT and SAGEResInception, not Linear"):
        pinf(torch.nn.Linear(8, 2), x, rowptr, col, **kw)
    biased = GAT(8, 4, 2, 2)
    biased.convs[0] = GATConv(8, 4, bias=True)
    with pytest.raises(NotImplementedError, match="bias=False"):
        pinf(biased, x, rowptr, col, **kw)
    concat = GAT(8, 4, 2, 2, heads=2)
    concat.convs[-1] = GATConv(4, 2, heads=2, concat=True, bias=False)
    with pytest.raises(NotImplementedError, match="concat=False on the last layer"):
        pinf(concat, x, rowptr, col, **kw)
    three = SAGEResInception(8, 4, 2, 2)
    three.mlp = MLP(8 + 4 * 2, 4, 2, num_layers=3, end_up_with_fc=True)
    with pytest.raises(NotImplementedError, match="exactly two Linears"):
        pinf(three, x, rowptr, col, **kw)
    for model in (GAT(8, 4, 2, 2), GAT(8, 4, 2, 3, heads=2), SAGEResInception(8, 4, 2, 2), SAGE(8, 4, 2, 2)):
        for bad in ([1], [4], [2, 3, 0]):                    # global ids of another rank's range, or outside the graph
            with pytest.raises(ValueError, match=r"outside rank 1's range \[2, 4\)"):
                pinf(model, x, rowptr, col, nodes=torch.tensor(bad), **kw)
        with pytest.raises(ValueError, match="nodes must be"):
            pinf(model, x, rowptr, col, nodes=torch.tensor([0.5]), **kw)
        with pytest.raises(ValueError, match="act_dtype"):
            pinf(model, x, rowptr, col, act_dtype=torch.float16, **kw)
        with pytest.raises(ValueError, match="rows_per_slab"):
            pinf(model, x, rowptr, col, rows_per_slab=0, **kw)
        with pytest.raises(TypeError, match="peers must provide"):
            pinf(model, x, rowptr, col, **{**kw, "peers": type("P", (), {"share": print, "close": print})()})
        with pytest.raises(TypeError, match="fp8 feature table"):
            pinf(model, fp8.quantize_e4m3(torch.zeros((2, 16))), rowptr, col, **kw)
        with pytest.raises(ValueError, match="rank 2 outside"):
            pinf(model, x, rowptr, col, **{**kw, "rank": 2})
        with pytest.raises(ValueError, match="x_local has 2 rows"):
            pinf(model, x, rowptr, col, **{**kw, "part_offsets": [0, 1, 4]})
        with pytest.raises(ValueError, match="one row per node"):
            pinf(model, x, rowptr[:-1], col, **kw)
        assert model.training                                 # a refused call leaves the mode alone


def test_the_older_entry_is_the_common_one_under_its_own_name(no_device):
    """GAT and SAGEResInception pass the older entry's model filter too: every later check answers, in
    ``partitioned_inference``'s words behind the older entry's name, and a valid call goes on to the device"""
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import partitioned_inference as pinf
    from salient_plusplus_amd.inference import partitioned_layerwise_inference as pli
    from salient_plusplus_amd.models import GAT, GATConv, SAGE, SAGEResInception
    x = torch.zeros((4, 8), dtype=torch.float16)[2:]
    kw = dict(part_offsets=[0, 2, 4], rank=1, peers=_NoPeers())
    rowptr, col = torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, 1, 2, 3])
    old, new = "partitioned_layerwise_inference: ", "partitioned_inference: "
    for model in (GAT(8, 4, 2, 2), GAT(8, 4, 2, 2, heads=4), SAGEResInception(8, 4, 2, 2), SAGE(8, 4, 2, 2)):
        with pytest.raises(TypeError, match=f"^{old}an fp8 feature table"):      # the check behind the model filter
            pli(model, fp8.quantize_e4m3(torch.zeros((2, 16))), rowptr, col, **kw)
        for bad in (dict(rank=2), dict(part_offsets=[0, 1, 4]), dict(act_dtype=torch.float16), dict(rows_per_slab=0),
                    dict(nodes=torch.tensor([0.5])), dict(nodes=torch.tensor([1])), dict(peers=object())):
            with pytest.raises((TypeError, ValueError), match=f"^{old}") as got:
                pli(model, x, rowptr, col, **{**kw, **bad})
            with pytest.raises(type(got.value), match=f"^{new}") as want:
                pinf(model, x, rowptr, col, **{**kw, **bad})
            assert str(got.value)[len(old):] == str(want.value)[len(new):]
        with pytest.raises(AssertionError, match="before the arguments were refused"):   # valid: it reaches the device
            pli(model, x, rowptr, col, **kw)
        assert model.training
    biased = GAT(8, 4, 2, 2)
    biased.convs[0] = GATConv(8, 4, bias=True)
    with pytest.raises(NotImplementedError, match=f"^{old}GAT layers need bias=False"):
        pli(biased, x, rowptr, col, **kw)
    with pytest.raises(NotImplementedError, match=f"^{old}implemented for SAGE, GIN, GAT and SAGEResInception, not Linear$"):
        pli(torch.nn.Linear(8, 2), x, rowptr, col, **kw)
