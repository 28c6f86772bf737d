"""CPU-only: the host side of exact layer-wise GAT inference -- the ctypes layout of spp_graph_gat_desc against the
header, the three exported entries, every refusal of spp_graph_gat_forward (made before anything is enqueued, so no GPU
is needed), and the argument validation of inference.graph_gat_aggregate and layerwise_inference(GAT(...), ...) before
any device call."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(F=4, heads=2):
    x = torch.zeros((3, F))
    a = torch.zeros((3, heads))
    return x, a, a.clone(), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])


@pytest.fixture
def no_device(monkeypatch):
    """any step towards the device fails the test: the refusals must come first"""
    from salient_plusplus_amd import _native as nat

    def touched(*_a, **_k):
        raise AssertionError("a device call was made before the arguments were refused")
    monkeypatch.setattr(nat, "require_device", touched)


def test_graph_gat_desc_layout_matches_header():
    """sizeof and every field offset of spp_graph_gat_desc, cross-checked by compiling the header with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.GraphGatDesc._fields_]
    offs = ", ".join(f"offsetof(spp_graph_gat_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_graph_gat_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(nat.GraphGatDesc)] + [getattr(nat.GraphGatDesc, n).offset for n in names]


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def test_library_exports_the_graph_attention():
    from salient_plusplus_amd.inference import graph_gat_chunk, graph_gat_workspace_bytes
    nat, L = _lib()
    for name in ("spp_graph_gat_forward", "spp_graph_gat_chunk", "spp_graph_gat_workspace_bytes"):
        assert hasattr(L, name) and name in nat.SIGNATURES
    assert L.spp_abi_version() == 6
    assert graph_gat_chunk() >= 32
    sizes = [graph_gat_workspace_bytes(T) for T in (0, 1, 2, 7, 1000, 1 << 20, 1 << 33)]
    assert sizes == sorted(sizes) and sizes[0] >= 16
    assert all(b >= 8 * T for b, T in zip(sizes, (0, 1, 2, 7, 1000, 1 << 20, 1 << 33)))


# a descriptor that passes every check; the pointers are never dereferenced by a refusal (nothing is enqueued)
_FAKE = 0x10000
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)


def _desc(nat, **over):
    kw = dict(x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, heads=2, relu=0, rowptr_dev=_FAKE, col_dev=_FAKE,
              x_dev=_FAKE, x_stride_elems=8, x_rows=10, F=8, a_src_dev=_FAKE, a_dst_dev=_FAKE, target_row0=0,
              target_ids_dev=None, num_targets=4, out_dev=_FAKE, out_stride_elems=0, negative_slope=0.2)
    kw.update(over)
    return nat.GraphGatDesc(**kw)


REFUSALS = [
    ("both target forms", dict(target_ids_dev=_FAKE), {}, b"not both"),
    ("neither target form", dict(target_row0=-1), {}, b"target_row0"),
    ("slab outside the graph", dict(target_row0=8, num_targets=4), {}, b"target_row0"),
    ("heads < 1", dict(heads=0), {}, b"heads"),
    ("heads does not divide F", dict(heads=3), {}, b"heads"),
    ("unknown x_elem", dict(x_elem=77), {}, b"x_elem"),
    ("fp16 output", dict(out_elem="F16"), {}, b"out_elem"),
    ("fp8 rows", dict(x_elem="FP8_E4M3"), {}, b"fp8"),
    ("fp8 output", dict(out_elem="FP8_E4M3"), {}, b"fp8"),
    ("misaligned output base (vector form)", dict(out_dev=_FAKE + 4), {}, b"out_dev"),
    ("misaligned output stride (vector form)", dict(out_stride_elems=10), {}, b"out_dev"),
    ("missing workspace", {}, dict(ws=None), b"workspace"),
    ("misaligned workspace", {}, dict(ws=_FAKE + 8), b"workspace"),
    ("small workspace", {}, dict(bytes=8), b"workspace"),
    ("row stride smaller than the row", dict(x_stride_elems=7), {}, b"x_stride_elems"),
    ("output stride smaller than the row", dict(out_stride_elems=4), {}, b"out_stride_elems"),
]


@pytest.mark.parametrize("what,over,call,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses_before_anything_is_enqueued(what, over, call, word):
    nat, L = _lib()
    over = {k: getattr(nat, "SPP_ELEM_" + v) if isinstance(v, str) else v for k, v in over.items()}
    d = _desc(nat, **over)
    ws = call.get("ws", _FAKE)
    nbytes = call.get("bytes", int(L.spp_graph_gat_workspace_bytes(d.num_targets)))
    assert L.spp_graph_gat_forward(ctypes.byref(d), ctypes.c_void_p(ws), nbytes, None) == SPP_ERR_INVALID, what
    assert word in L.spp_last_error(), (what, L.spp_last_error())


def test_entry_refuses_a_null_descriptor_and_accepts_empty_calls():
    nat, L = _lib()
    assert L.spp_graph_gat_forward(None, ctypes.c_void_p(_FAKE), 1 << 20, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    # T == 0 or F == 0: nothing to do, SPP_OK without touching a device or a buffer
    for over in (dict(num_targets=0), dict(F=0, x_stride_elems=0)):
        d = _desc(nat, **over)
        assert L.spp_graph_gat_forward(ctypes.byref(d), ctypes.c_void_p(_FAKE), 1 << 10, None) == SPP_OK, over


def test_graph_gat_aggregate_validates_its_arguments(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from salient_plusplus_amd.inference import graph_gat_aggregate as gat
    x, a_src, a_dst, rowptr, col = _tiny()
    slab = dict(heads=2, row0=0, num_targets=3)
    with pytest.raises(ValueError, match="not both"):
        gat(x, a_src, a_dst, rowptr, col, target_ids=torch.tensor([0]), **slab)
    with pytest.raises(ValueError, match="either as a slab"):
        gat(x, a_src, a_dst, rowptr, col, heads=2)
    with pytest.raises(ValueError, match="both row0 and num_targets"):
        gat(x, a_src, a_dst, rowptr, col, heads=2, row0=0)
    with pytest.raises(ValueError, match="leaves the graph"):
        gat(x, a_src, a_dst, rowptr, col, heads=2, row0=2, num_targets=2)
    with pytest.raises(ValueError, match="target_ids"):
        gat(x, a_src, a_dst, rowptr, col, heads=2, target_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="a_src"):                       # the wrong shape: one head's logits for two
        gat(x, a_src[:, :1].contiguous(), a_dst, rowptr, col, **slab)
    with pytest.raises(ValueError, match="a_dst"):                       # the wrong dtype
        gat(x, a_src, a_dst.double(), rowptr, col, **slab)
    with pytest.raises(ValueError, match="a_src"):                       # not contiguous
        gat(x, torch.zeros((3, 4))[:, ::2], a_dst, rowptr, col, **slab)
    with pytest.raises(ValueError, match="heads"):
        gat(x, torch.zeros((3, 3)), torch.zeros((3, 3)), rowptr, col, heads=3, row0=0, num_targets=3)
    with pytest.raises(ValueError, match="heads"):
        gat(x, a_src, a_dst, rowptr, col, heads=0, row0=0, num_targets=3)
    with pytest.raises(ValueError, match="out_dtype"):
        gat(x, a_src, a_dst, rowptr, col, out_dtype=torch.float16, **slab)
    with pytest.raises(ValueError, match="one row per node"):
        gat(x, a_src, a_dst, rowptr[:-1], col, **slab)
    with pytest.raises(ValueError, match="2-D"):
        gat(x.double(), a_src, a_dst, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="requires grad"):
        gat(x.clone().requires_grad_(), a_src, a_dst, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="a_src requires grad"):
        gat(x, a_src.clone().requires_grad_(), a_dst, rowptr, col, **slab)
    with pytest.raises(TypeError, match="fp8"):
        gat(fp8.quantize_e4m3(torch.zeros((3, 16))), a_src, a_dst, rowptr, col, **slab)
    with pytest.raises(TypeError, match="TableRows"):
        gat(TableRows(x, torch.tensor([0])), a_src, a_dst, rowptr, col, **slab)
    with pytest.raises(TypeError, match="RowRefs"):
        gat(RowRefs(torch.zeros(3, dtype=torch.int64), None, 4, torch.float16, None, ()), a_src, a_dst, rowptr, col,
            **slab)


def test_layerwise_inference_of_gat_validates_before_the_device(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import GAT, GATConv
    x, _a, _b, rowptr, col = _tiny()
    for heads in (1, 2):
        model = GAT(4, 4, 2, 2, heads=heads)
        with pytest.raises(TypeError, match="fp8 feature table"):
            layerwise_inference(model, fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col)
        with pytest.raises(TypeError, match="TableRows"):
            layerwise_inference(model, TableRows(x, torch.tensor([0])), rowptr, col)
        with pytest.raises(TypeError, match="RowRefs"):
            layerwise_inference(model, RowRefs(torch.zeros(3, dtype=torch.int64), None, 4, torch.float16, None, ()),
                                rowptr, col)
        with pytest.raises(RuntimeError, match="requires grad"):
            layerwise_inference(model, x.clone().requires_grad_(), rowptr, col)
        with pytest.raises(ValueError, match="one row per node"):
            layerwise_inference(model, x, rowptr[:-1], col)
        with pytest.raises(ValueError, match="act_dtype"):
            layerwise_inference(model, x, rowptr, col, act_dtype=torch.float16)
        with pytest.raises(ValueError, match="rows_per_slab"):
            layerwise_inference(model, x, rowptr, col, rows_per_slab=0)
        with pytest.raises(ValueError, match="nodes"):
            layerwise_inference(model, x, rowptr, col, nodes=torch.tensor([0.5]))
        with pytest.raises(ValueError, match="nodes"):
            layerwise_inference(model, x, rowptr, col, nodes=torch.tensor([[0]]))
        assert model.training                                 # a refused call leaves the mode alone
    biased = GAT(4, 4, 2, 2)
    biased.convs[0] = GATConv(4, 4, bias=True)
    with pytest.raises(NotImplementedError, match="bias=False"):
        layerwise_inference(biased, x, rowptr, col)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: implemented for SAGE, GIN, GAT, SAGEResInception, GCN and GATv2, not Linear$"):
        layerwise_inference(torch.nn.Linear(4, 2), x, rowptr, col)


def test_valid_gat_arguments_need_the_device_and_the_method_is_the_function():
    from inference_method import assert_method_is_the_function
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import GAT, GATConv
    x, _a, _b, rowptr, col = _tiny()
    for heads in (1, 2, 4):
        assert_method_is_the_function(GAT(4, 4, 2, 2, heads=heads), x, rowptr, col)
    biased = GAT(4, 4, 2, 2)
    biased.convs[0] = GATConv(4, 4, bias=True)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: GAT layers need bias=False"):
        biased.inference(x, rowptr, col)
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        from salient_plusplus_amd import _native as nat
        model = GAT(4, 4, 2, 2, heads=2)
        with pytest.raises(nat.SppError):
            layerwise_inference(model, x, rowptr, col)
        assert model.training
