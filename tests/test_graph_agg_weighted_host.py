"""CPU-only: the weighted member of the resident-graph aggregation family and GCN inference (spp.h f3s) without a device
-- the two descriptors against the header, every refusal spp_graph_agg_weighted_forward and spp_gcn_dinv make before a
launch, the argument checks of inference.graph_weighted_aggregate, gcn_dinv and of the drivers' edge_weight, and what
stays refused: GCN over parts and fields, GCN.inference."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SPP_OK, SPP_ERR_INVALID = 0, -1
_FAKE = 0x7F0000001000                                   # never dereferenced: every refusal comes before a launch


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


@pytest.fixture
def no_device(monkeypatch):
    """any step towards the device fails the test: the refusals must come first"""
    from salient_plusplus_amd import _native as nat

    def touched(*_a, **_k):
        raise AssertionError("a device call was made before the arguments were refused")
    monkeypatch.setattr(nat, "require_device", touched)


@pytest.mark.parametrize("struct,cname", [("GraphAggWeightedDesc", "spp_graph_agg_weighted_desc"),
                                          ("GcnDinvDesc", "spp_gcn_dinv_desc")])
def test_descriptor_layout_matches_header(tmp_path, struct, cname):
    """sizeof and every field offset, in the header's order, cross-checked by compiling the header with gcc"""
    nat, _ = _lib()
    cls = getattr(nat, struct)
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = header[header.index("typedef struct %s {" % cname):header.index("} %s;" % cname)]
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body))
    assert names == [f[0] for f in cls._fields_]
    offs = ", ".join(f"offsetof({cname}, {n})" for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spp.h"\n'
                   "int main(void) { size_t v[] = { sizeof(%s), %s };\n"
                   "  for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf(\"%%zu\\n\", v[i]);\n  return 0; }\n"
                   % (cname, offs))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in names]


def test_library_exports_the_entries_and_the_abi_version_stays():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    for name in ("spp_graph_agg_weighted_forward", "spp_gcn_dinv"):
        assert hasattr(L, name) and name in nat.SIGNATURES and f" {name}(" in header, name
    assert "#define SPP_ABI_VERSION 6" in header
    assert "graph_agg_weighted.hip" in __import__("salient_plusplus_amd.build", fromlist=["SOURCES"]).SOURCES


def _desc(nat, **over):
    kw = dict(x_elem=nat.SPP_ELEM_F16, out_elem=nat.SPP_ELEM_F32, fill=1, rowptr_dev=_FAKE, col_dev=_FAKE, x_dev=_FAKE,
              x_stride_elems=8, x_rows=100, F=8, target_row0=10, target_ids_dev=None, num_targets=5, out_dev=_FAKE,
              out_stride_elems=0, w_dev=_FAKE, dinv_dev=None, self_w_dev=_FAKE)
    kw.update(over)
    return nat.GraphAggWeightedDesc(**kw)


def test_weighted_forward_refusals_come_before_any_launch():
    nat, L = _lib()
    who = b"spp_graph_agg_weighted_forward"
    need = L.spp_graph_agg_workspace_bytes(5)

    def call(over):
        over = dict(over)
        ws, nbytes = over.pop("ws", _FAKE), over.pop("nbytes", need)
        return L.spp_graph_agg_weighted_forward(ctypes.byref(_desc(nat, **over)), ws, nbytes, None)

    cases = {
        # what spp_graph_agg_forward refuses
        "both target forms": (dict(target_ids_dev=_FAKE), b"not both"),
        "no target form": (dict(target_row0=-1), b"one of them"),
        "slab outside the graph": (dict(target_row0=98), b"leaves the graph"),
        "negative T": (dict(num_targets=-1), b"negative"),
        "negative F": (dict(F=-8), b"negative"),
        "unknown x code": (dict(x_elem=7), b"element code"),
        "fp16 output": (dict(out_elem=nat.SPP_ELEM_F16), b"element code"),
        "fp8 rows": (dict(x_elem=nat.SPP_ELEM_FP8_E4M3), b"fp8"),
        "fp8 output": (dict(out_elem=nat.SPP_ELEM_FP8_E4M3), b"fp8"),
        "output stride": (dict(out_stride_elems=7), b"output stride"),
        "row stride": (dict(x_stride_elems=7), b"row stride"),
        "NULL rowptr": (dict(rowptr_dev=None), b"NULL"),
        "NULL col": (dict(col_dev=None), b"NULL"),
        "NULL x": (dict(x_dev=None), b"NULL"),
        "NULL out": (dict(out_dev=None), b"NULL"),
        "misaligned output of the vector form": (dict(out_dev=_FAKE + 4), b"vector form"),
        "no workspace": (dict(ws=None), b"workspace"),
        "small workspace": (dict(nbytes=need - 1), b"workspace"),
        "misaligned workspace": (dict(ws=_FAKE + 8, nbytes=1 << 20), b"workspace"),
        # its own
        "dinv with self_w": (dict(dinv_dev=_FAKE), b"dinv_dev and self_w_dev together"),
        "fill 3": (dict(dinv_dev=_FAKE, self_w_dev=None, fill=3), b"fill"),
        "negative fill": (dict(dinv_dev=_FAKE, self_w_dev=None, fill=-1), b"fill"),
        "misaligned w": (dict(w_dev=_FAKE + 2), b"misaligned"),
        "misaligned dinv": (dict(dinv_dev=_FAKE + 1, self_w_dev=None), b"misaligned"),
        "misaligned self_w": (dict(self_w_dev=_FAKE + 3), b"misaligned"),
    }
    for what, (over, text) in cases.items():
        assert call(over) == SPP_ERR_INVALID, what
        msg = L.spp_last_error()
        assert who in msg and text in msg, (what, msg)
    assert L.spp_graph_agg_weighted_forward(None, _FAKE, need, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    # nothing to do: SPP_OK without a launch; fill is not read without dinv_dev
    for over in (dict(num_targets=0), dict(F=0, x_stride_elems=0), dict(num_targets=0, fill=9, w_dev=None, self_w_dev=None)):
        assert call(over) == SPP_OK, over
    # the descriptor's own refusals come even when there is nothing to do
    assert call(dict(num_targets=0, dinv_dev=_FAKE)) == SPP_ERR_INVALID
    assert call(dict(num_targets=0, dinv_dev=_FAKE, self_w_dev=None, fill=3)) == SPP_ERR_INVALID


def test_gcn_dinv_refusals_come_before_any_launch():
    nat, L = _lib()

    def call(**over):
        kw = dict(fill=1, rowptr_dev=_FAKE, num_nodes=5, w_dev=_FAKE, dinv_dev=_FAKE)
        kw.update(over)
        return L.spp_gcn_dinv(ctypes.byref(nat.GcnDinvDesc(**kw)), None)

    cases = {
        "fill 3": (dict(fill=3), b"fill"),
        "negative fill": (dict(fill=-1), b"fill"),
        "negative N": (dict(num_nodes=-1), b"num_nodes"),
        "N out of range": (dict(num_nodes=1 << 60), b"num_nodes"),
        "NULL rowptr": (dict(rowptr_dev=None), b"NULL"),
        "NULL dinv": (dict(dinv_dev=None), b"NULL"),
        "misaligned w": (dict(w_dev=_FAKE + 2), b"misaligned"),
        "misaligned dinv": (dict(dinv_dev=_FAKE + 1), b"misaligned"),
    }
    for what, (over, text) in cases.items():
        assert call(**over) == SPP_ERR_INVALID, what
        msg = L.spp_last_error()
        assert b"spp_gcn_dinv" in msg and text in msg, (what, msg)
    assert L.spp_gcn_dinv(None, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    assert call(num_nodes=0, rowptr_dev=None, dinv_dev=None) == SPP_OK


def _graph():
    """6 nodes, 9 entries"""
    return torch.tensor([0, 2, 3, 3, 6, 8, 9]), torch.tensor([1, 2, 0, 0, 4, 5, 3, 3, 1])


def test_graph_weighted_aggregate_validates_its_arguments(no_device):
    from salient_plusplus_amd import fp8 as fp8_mod
    from salient_plusplus_amd import inference as inf
    rowptr, col = _graph()
    x = torch.zeros((6, 4), dtype=torch.float16)
    w, v = torch.ones(9), torch.ones(6)
    what = "^graph_weighted_aggregate: "
    slab = dict(row0=0, num_targets=6)
    fn = inf.graph_weighted_aggregate
    for name, good, n in (("weight", w, 9), ("dinv", v, 6), ("self_weight", v, 6)):
        for bad in (good.double(), good.half(), torch.ones(n + 1), torch.ones((n, 1)), torch.ones(2 * n)[::2], list(range(n))):
            with pytest.raises(ValueError, match=rf"{what}{name} must be a contiguous fp32 tensor of shape \[{n}\]"):
                fn(x, rowptr, col, **{name: bad}, **slab)
        with pytest.raises(RuntimeError, match=rf"{what}{name} requires grad"):
            fn(x, rowptr, col, **{name: good.clone().requires_grad_()}, **slab)
    with pytest.raises(ValueError, match=what + "give dinv or self_weight, not both"):
        fn(x, rowptr, col, dinv=v, self_weight=v, **slab)
    for fill in (3, -1, 1.0, True, None):
        with pytest.raises(ValueError, match=what + "fill must be 0"):
            fn(x, rowptr, col, dinv=v, fill=fill, **slab)
    quant = fp8_mod.quantize_e4m3(torch.zeros((6, 16)))
    with pytest.raises(TypeError, match=what + "an fp8 feature table"):
        fn(quant, rowptr, col, weight=w, **slab)
    with pytest.raises(TypeError, match=what + "x is an Fp8Table.*fp8 tables.*take no edge weights"):
        fn(inf.Fp8Table(quant), rowptr, col, weight=w, **slab)
    with pytest.raises(NotImplementedError, match=what + "x is row-partitioned.*a row-partitioned x"):
        fn([x[:3], x[3:]], rowptr, col, weight=w, **slab)
    with pytest.raises(RuntimeError, match=what + "x requires grad"):
        fn(x.float().requires_grad_(), rowptr, col, **slab)
    with pytest.raises(ValueError, match=what + "x must be a 2-D"):
        fn(x.double(), rowptr, col, **slab)
    with pytest.raises(ValueError, match=what + "x has 6 rows"):
        fn(x, rowptr[:5], col, **slab)
    with pytest.raises(ValueError, match=what + "out_dtype"):
        fn(x, rowptr, col, out_dtype=torch.float16, **slab)
    with pytest.raises(ValueError, match=what + "give the targets either"):
        fn(x, rowptr, col)
    with pytest.raises(ValueError, match=what + "give the targets either.*not both"):
        fn(x, rowptr, col, target_ids=torch.tensor([0]), **slab)
    with pytest.raises(ValueError, match=what + "the slab"):
        fn(x, rowptr, col, row0=4, num_targets=3)
    with pytest.raises(ValueError, match=what + "out must be"):
        fn(x, rowptr, col, out=torch.zeros((6, 5)), **slab)
    with pytest.raises(AssertionError, match="before the arguments were refused"):       # valid: it reaches the device
        fn(x, rowptr, col, weight=w, dinv=v, fill=2, **slab)


def test_gcn_dinv_validates_its_arguments(no_device):
    from salient_plusplus_amd.inference import gcn_dinv
    rowptr, _col = _graph()
    w = torch.ones(9)
    with pytest.raises(ValueError, match="^gcn_dinv: rowptr"):
        gcn_dinv(rowptr.int())
    with pytest.raises(ValueError, match="^gcn_dinv: rowptr"):
        gcn_dinv(rowptr.view(1, -1))
    for bad in (w.double(), w.view(3, 3), torch.ones(18)[::2], [1.0] * 9):
        with pytest.raises(ValueError, match="^gcn_dinv: edge_weight"):
            gcn_dinv(rowptr, bad)
    with pytest.raises(RuntimeError, match="^gcn_dinv: edge_weight requires grad"):
        gcn_dinv(rowptr, w.clone().requires_grad_())
    with pytest.raises(AssertionError, match="before the arguments were refused"):
        gcn_dinv(rowptr, w, improved=True)


def _gcn(normalize=False):
    from salient_plusplus_amd.models import GCN
    return GCN(4, 8, 3, 2, normalize=normalize)


def test_the_resident_drivers_check_gcn_and_edge_weight_before_the_device(no_device):
    from salient_plusplus_amd import fp8 as fp8_mod
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GAT, GIN, SAGE, SAGEResInception
    rowptr, col = _graph()
    x = torch.zeros((6, 4), dtype=torch.float16)
    w = torch.ones(9)
    for fn in (inf.layerwise_inference, inf.evaluate):
        name = fn.__name__
        for other in (SAGE(4, 8, 3, 2), GIN(4, 8, 3, 2), GAT(4, 8, 3, 2), SAGEResInception(4, 8, 3, 2)):
            with pytest.raises(ValueError, match=rf"^{name}: edge_weight is GCN's.*{type(other).__name__}"):
                fn(other, x, rowptr, col, edge_weight=w)
        with pytest.raises(NotImplementedError, match=rf"^{name}: implemented for"):
            fn(torch.nn.Linear(4, 3), x, rowptr, col, edge_weight=w)
        for normalize in (False, True):
            m = _gcn(normalize)
            for bad in (w.double(), torch.ones(8), torch.ones((9, 1)), torch.ones(18)[::2]):
                with pytest.raises(ValueError, match=rf"^{name}: edge_weight must be a contiguous fp32 tensor of shape \[9\]"):
                    fn(m, x, rowptr, col, edge_weight=bad)
            with pytest.raises(RuntimeError, match=rf"^{name}: edge_weight requires grad"):
                fn(m, x, rowptr, col, edge_weight=w.clone().requires_grad_())
            quant = fp8_mod.quantize_e4m3(torch.zeros((6, 16)))
            with pytest.raises(TypeError, match=rf"^{name}: an fp8 feature table"):
                fn(m, quant, rowptr, col)
            with pytest.raises(TypeError, match=rf"^{name}: x is an Fp8Table.*GCN.*take no edge weights"):
                fn(m, inf.Fp8Table(quant), rowptr, col)
            with pytest.raises(NotImplementedError, match=rf"^{name}: GCN over a row-partitioned x"):
                fn(m, [x[:3], x[3:]], rowptr, col)
            with pytest.raises(ValueError, match=rf"^{name}: x has 6 rows"):
                fn(m, x, rowptr[:5], col)
            with pytest.raises(ValueError, match=rf"^{name}: act_dtype"):
                fn(m, x, rowptr, col, act_dtype=torch.float16)
            with pytest.raises(AssertionError, match="before the arguments were refused"):   # valid: it reaches the device
                fn(m, x, rowptr, col, edge_weight=w)
            with pytest.raises(AssertionError, match="before the arguments were refused"):
                fn(m, x, rowptr, col)
            assert m.training                                # a refused call leaves the mode alone


class _NoPeers:
    """peers that must never be reached: a refused call publishes nothing and waits for nobody"""

    def share(self, _t):
        raise AssertionError("share() was called by a refused call")

    barrier = close = share


def test_parts_and_fields_still_refuse_gcn_with_their_messages(no_device):
    from salient_plusplus_amd import inference as inf
    rowptr, col = _graph()
    x = torch.zeros((6, 4), dtype=torch.float16)
    nodes = torch.tensor([0, 3], dtype=torch.int64)
    m = _gcn()
    for fn in (inf.field_inference, inf.field_evaluate):
        with pytest.raises(NotImplementedError, match=rf"^{fn.__name__}: implemented for SAGE, GIN and GAT, not GCN$"):
            fn(m, x, rowptr, col, nodes=nodes)
        with pytest.raises(TypeError, match="edge_weight"):  # no weights in the field entries
            fn(m, x, rowptr, col, nodes=nodes, edge_weight=torch.ones(9))
    kw = dict(part_offsets=[0, 3, 6], rank=0, peers=_NoPeers())
    for fn in (inf.partitioned_inference, inf.partitioned_evaluate, inf.partitioned_layerwise_inference):
        with pytest.raises(NotImplementedError,
                           match=rf"^{fn.__name__}: implemented for SAGE, GIN, GAT and SAGEResInception, not GCN$"):
            fn(m, x[:3], rowptr, col, **kw)
        with pytest.raises(TypeError, match="edge_weight"):
            fn(m, x[:3], rowptr, col, edge_weight=torch.ones(9), **kw)


def test_gcn_inference_method_is_the_driver():
    from inference_method import assert_method_is_the_function
    rowptr, col = _graph()
    x = torch.zeros((6, 4), dtype=torch.float16)
    for normalize in (False, True):
        assert_method_is_the_function(_gcn(normalize), x, rowptr, col)
        assert_method_is_the_function(_gcn(normalize), x, rowptr, col, edge_weight=torch.ones(9))
    for bad in (torch.ones(8), torch.ones(9).double()):      # the method hands edge_weight on: the function's refusal
        with pytest.raises(ValueError, match=r"^layerwise_inference: edge_weight must be a contiguous fp32 tensor of "
                                             r"shape \[9\]"):
            _gcn().inference(x, rowptr, col, edge_weight=bad)


def test_no_device_means_an_error_not_a_fallback():
    """with every argument in order the first thing asked for is the device: without one that is the error"""
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import inference as inf
    rowptr, col = _graph()
    x = torch.zeros((6, 4), dtype=torch.float16)
    m = _gcn(True)
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        with pytest.raises(nat.SppError):
            inf.graph_weighted_aggregate(x, rowptr, col, row0=0, num_targets=6)
        with pytest.raises(nat.SppError):
            inf.gcn_dinv(rowptr)
        with pytest.raises(nat.SppError):
            inf.layerwise_inference(m, x, rowptr, col)
    assert m.training
