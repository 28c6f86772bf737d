"""CPU-only: the host side of exact layer-wise SAGEResInception inference -- the ctypes layout of
spp_resinc_epilogue_desc against the header, the exported entry, every refusal of spp_resinc_epilogue (made before
anything is enqueued, so no GPU is needed), the argument validation of inference.resinc_epilogue before any device call,
and what the model's own inference() still says."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """any step towards the device fails the test: the refusals must come first"""
    from salient_plusplus_amd import _native as nat

    def touched(*_a, **_k):
        raise AssertionError("a device call was made before the arguments were refused")
    monkeypatch.setattr(nat, "require_device", touched)


def test_resinc_epilogue_desc_layout_matches_header():
    """sizeof and every field offset of spp_resinc_epilogue_desc, in the header's order, cross-checked with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.ResincEpilogueDesc._fields_]
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = header[header.index("typedef struct spp_resinc_epilogue_desc {"):header.index("} spp_resinc_epilogue_desc;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == names
    offs = ", ".join(f"offsetof(spp_resinc_epilogue_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_resinc_epilogue_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [getattr(nat.ResincEpilogueDesc, n).offset for n in names]
    assert got == [ctypes.sizeof(nat.ResincEpilogueDesc)] + offsets and offsets == sorted(offsets)


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def test_library_exports_the_epilogue_and_keeps_its_abi_version():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    assert "spp_status spp_resinc_epilogue(const spp_resinc_epilogue_desc* desc, void* stream);" in header
    assert hasattr(L, "spp_resinc_epilogue") and "spp_resinc_epilogue" in nat.SIGNATURES
    assert nat.SIGNATURES["spp_resinc_epilogue"][1][0]._type_ is nat.ResincEpilogueDesc
    assert L.spp_abi_version() == 6 and "#define SPP_ABI_VERSION 6" in header


# a descriptor that passes every check; the pointers are never dereferenced by a refusal (nothing is enqueued)
_FAKE = 0x10000
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)


def _desc(nat, **over):
    kw = dict(z_elem=nat.SPP_ELEM_F32, r_elem=nat.SPP_ELEM_F16, out_elem=nat.SPP_ELEM_BF16, negative_slope=0.01,
              z_dev=_FAKE, z_stride_elems=8, a_dev=_FAKE, b_dev=_FAKE, r_dev=_FAKE, r_stride_elems=8, r_rows=10,
              r_row0=0, r_ids_dev=None, n=4, C=8, out_dev=_FAKE, out_stride_elems=0)
    kw.update(over)
    return nat.ResincEpilogueDesc(**kw)


REFUSALS = [
    ("null z", dict(z_dev=None), b"NULL buffer"),
    ("null out", dict(out_dev=None), b"NULL buffer"),
    ("null a", dict(a_dev=None), b"NULL buffer"),
    ("null b", dict(b_dev=None), b"NULL buffer"),
    ("unknown z_elem", dict(z_elem=77), b"element code"),
    ("fp16 z", dict(z_elem="F16"), b"element code"),
    ("unknown r_elem", dict(r_elem=-3), b"element code"),
    ("fp8 residual", dict(r_elem="FP8_E4M3"), b"element code"),
    ("unknown out_elem", dict(out_elem=5), b"element code"),
    ("fp16 out", dict(out_elem="F16"), b"element code"),
    ("C == 0", dict(C=0), b"C = 0"),
    ("negative C", dict(C=-8), b"C = -8"),
    ("negative n", dict(n=-1), b"negative n"),
    ("negative z stride", dict(z_stride_elems=-8), b"negative row stride"),
    ("negative r stride", dict(r_stride_elems=-8), b"negative row stride"),
    ("negative out stride", dict(out_stride_elems=-8), b"negative row stride"),
    ("z stride smaller than the row", dict(z_stride_elems=7), b"smaller than the row"),
    ("out stride smaller than the row", dict(out_stride_elems=4), b"smaller than the row"),
    ("both slab and list", dict(r_ids_dev=_FAKE), b"not both"),
    ("both slab and list, no residual", dict(r_dev=None, r_ids_dev=_FAKE), b"not both"),
    ("a residual with neither", dict(r_row0=-1), b"needs its rows"),
    ("negative r_rows", dict(r_rows=-1), b"r_rows"),
    ("a residual of no rows", dict(r_rows=0), b"without rows"),
]


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses_before_anything_is_enqueued(what, over, word):
    nat, L = _lib()
    over = {k: getattr(nat, "SPP_ELEM_" + v) if isinstance(v, str) else v for k, v in over.items()}
    d = _desc(nat, **over)
    assert L.spp_resinc_epilogue(ctypes.byref(d), None) == SPP_ERR_INVALID, what
    assert word in L.spp_last_error(), (what, L.spp_last_error())


def test_entry_refuses_a_null_descriptor_and_accepts_an_empty_call():
    nat, L = _lib()
    assert L.spp_resinc_epilogue(None, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    # n == 0: nothing to do, SPP_OK without touching a device or a buffer -- with a slab, a list, or no residual
    for over in (dict(n=0), dict(n=0, r_row0=-1, r_ids_dev=_FAKE), dict(n=0, r_dev=None), dict(n=0, r_rows=0)):
        assert L.spp_resinc_epilogue(ctypes.byref(_desc(nat, **over)), None) == SPP_OK, over


def test_wrapper_validates_before_any_device_call(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from salient_plusplus_amd.inference import resinc_epilogue
    z, a, b = torch.zeros((3, 4)), torch.ones(4), torch.zeros(4)
    r = torch.zeros((5, 4), dtype=torch.float16)
    kw = dict(negative_slope=0.01)
    with pytest.raises(TypeError, match="resinc_epilogue.*TableRows"):
        resinc_epilogue(TableRows(z, torch.tensor([0])), a, b, **kw)
    with pytest.raises(TypeError, match="resinc_epilogue.*TableRows"):
        resinc_epilogue(z, a, b, residual=TableRows(z, torch.tensor([0])), row0=0, **kw)
    with pytest.raises(TypeError, match="resinc_epilogue.*RowRefs"):
        resinc_epilogue(z, a, b, residual=RowRefs(torch.zeros(3, dtype=torch.int64), None, 4, torch.float16, None, ()),
                        row0=0, **kw)
    with pytest.raises(TypeError, match="resinc_epilogue.*fp8"):
        resinc_epilogue(fp8.quantize_e4m3(torch.zeros((3, 16))), a, b, **kw)
    with pytest.raises(TypeError, match="resinc_epilogue.*fp8"):
        resinc_epilogue(torch.zeros((3, 16)), torch.ones(16), torch.ones(16),
                        residual=fp8.quantize_e4m3(torch.zeros((3, 16))), row0=0, **kw)
    with pytest.raises(TypeError, match="resinc_epilogue: z must be a torch.Tensor"):
        resinc_epilogue([[0.0]], a, b, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: z must be fp32 or bf16"):
        resinc_epilogue(z.half(), a, b, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: z must be a 2-D"):
        resinc_epilogue(z[0], a, b, **kw)
    with pytest.raises(RuntimeError, match="resinc_epilogue: z requires grad"):
        resinc_epilogue(z.clone().requires_grad_(), a, b, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: scale"):
        resinc_epilogue(z, a.double(), b, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: shift"):
        resinc_epilogue(z, a, torch.zeros(5), **kw)
    with pytest.raises(RuntimeError, match="resinc_epilogue: scale requires grad"):
        resinc_epilogue(z, a.clone().requires_grad_(), b, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue.*there is no residual"):
        resinc_epilogue(z, a, b, row0=0, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue.*either as a slab"):
        resinc_epilogue(z, a, b, residual=r, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue.*not both"):
        resinc_epilogue(z, a, b, residual=r, row0=0, row_ids=torch.tensor([0, 1, 2]), **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: row0"):
        resinc_epilogue(z, a, b, residual=r, row0=-1, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: row_ids"):
        resinc_epilogue(z, a, b, residual=r, row_ids=torch.tensor([0, 1]), **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: row_ids"):
        resinc_epilogue(z, a, b, residual=r, row_ids=torch.tensor([0, 1, 2], dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: residual must have"):
        resinc_epilogue(z, a, b, residual=torch.zeros((5, 3)), row0=0, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: out_dtype"):
        resinc_epilogue(z, a, b, out_dtype=torch.float16, **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: out must be"):
        resinc_epilogue(z, a, b, out=torch.zeros((3, 5)), **kw)
    with pytest.raises(ValueError, match="resinc_epilogue: out is"):
        resinc_epilogue(z, a, b, out=torch.zeros((3, 4)), out_dtype=torch.bfloat16, **kw)
    with pytest.raises(TypeError):                            # negative_slope is a required keyword
        resinc_epilogue(z, a, b)


def test_wrapper_needs_the_device_for_valid_arguments():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.inference import resinc_epilogue
    # no CPU fallback: without a device valid arguments fail at the device check, with one host tensors are refused
    refusal = (ValueError, "one CUDA device") if torch.cuda.is_available() else (nat.SppError, None)
    with pytest.raises(refusal[0], match=refusal[1]):
        resinc_epilogue(torch.zeros((3, 4)), torch.ones(4), torch.zeros(4), negative_slope=0.01)


def test_model_inference_is_the_driver():
    from inference_method import assert_method_is_the_function
    from salient_plusplus_amd.models import MLP, SAGEResInception
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = SAGEResInception(4, 4, 2, 2)
    assert_method_is_the_function(model, x, rowptr, col)
    model.mlp = MLP(4 + 4 * 2, 4, 2, num_layers=3, end_up_with_fc=True)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: SAGEResInception's head must be exactly two "
                                                  "Linears"):
        model.inference(x, rowptr, col)


def test_driver_refusals_for_sageresinception(no_device):
    """the refusals every model shares come before the device for SAGEResInception too; so does the head's check"""
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import MLP, SAGEResInception
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = SAGEResInception(4, 4, 2, 2)
    with pytest.raises(TypeError, match="fp8 feature table"):
        layerwise_inference(model, fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col)
    with pytest.raises(TypeError, match="TableRows"):
        layerwise_inference(model, TableRows(x, torch.tensor([0])), rowptr, col)
    with pytest.raises(TypeError, match="RowRefs"):
        layerwise_inference(model, RowRefs(torch.zeros(3, dtype=torch.int64), None, 4, torch.float16, None, ()), rowptr, col)
    with pytest.raises(ValueError, match="act_dtype"):
        layerwise_inference(model, x, rowptr, col, act_dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: implemented for SAGE, GIN, GAT, SAGEResInception, GCN and GATv2, not Linear$"):
        layerwise_inference(torch.nn.Linear(4, 2), x, rowptr, col)
    model.mlp = MLP(4 + 4 * 2, 4, 2, num_layers=2, bn=True, end_up_with_fc=False, act="LeakyReLU")
    with pytest.raises(NotImplementedError, match="exactly two Linears"):
        layerwise_inference(model, x, rowptr, col)
    model.mlp = MLP(4 + 4 * 2, 4, 2, num_layers=3, end_up_with_fc=True)
    with pytest.raises(NotImplementedError, match="exactly two Linears"):
        layerwise_inference(model, x, rowptr, col)
    assert model.training
