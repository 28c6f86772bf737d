"""CPU-only: the host side of exact whole-graph evaluation -- the ctypes layout of spp_classify_desc against the header,
the exported entry, every refusal of spp_classify_rows (made before anything is enqueued, so no GPU is needed), and the
argument validation of inference.classify_rows, evaluate and partitioned_evaluate before any device call."""
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


def test_classify_desc_layout_matches_header():
    """sizeof and every field offset of spp_classify_desc, in the header's order, cross-checked with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.ClassifyDesc._fields_]
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = header[header.index("typedef struct spp_classify_desc {"):header.index("} spp_classify_desc;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == names
    offs = ", ".join(f"offsetof(spp_classify_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_classify_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    offsets = [getattr(nat.ClassifyDesc, n).offset for n in names]
    assert got == [ctypes.sizeof(nat.ClassifyDesc)] + offsets and offsets == sorted(offsets)


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def test_library_exports_the_entry_and_keeps_its_abi_version():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    assert "spp_status spp_classify_rows(const spp_classify_desc* desc, void* stream);" in header
    assert hasattr(L, "spp_classify_rows") and "spp_classify_rows" in nat.SIGNATURES
    assert nat.SIGNATURES["spp_classify_rows"][1][0]._type_ is nat.ClassifyDesc
    assert L.spp_abi_version() == 6 and "#define SPP_ABI_VERSION 6" in header


# a descriptor that passes every check; the pointers are never dereferenced by a refusal (nothing is enqueued)
_FAKE = 0x10000
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)


def _desc(nat, **over):
    kw = dict(z_elem=nat.SPP_ELEM_BF16, z_dev=_FAKE, z_stride_elems=48, n=4, C=47, y_dev=_FAKE, y_rows=10, y_row0=0,
              row_ids_dev=None, pred_dev=_FAKE, nll_dev=_FAKE)
    kw.update(over)
    return nat.ClassifyDesc(**kw)


REFUSALS = [
    ("null z", dict(z_dev=None), b"NULL buffer"),
    ("no output", dict(pred_dev=None, nll_dev=None), b"nothing to write"),
    ("unknown z_elem", dict(z_elem=77), b"element code"),
    ("fp16 z", dict(z_elem="F16"), b"element code"),
    ("fp8 z", dict(z_elem="FP8_E4M3"), b"element code"),
    ("C == 0", dict(C=0, z_stride_elems=0), b"C = 0"),
    ("negative C", dict(C=-8), b"C = -8"),
    ("C == 2^31", dict(C=1 << 31, z_stride_elems=0), b"C = 2147483648"),
    ("negative n", dict(n=-1), b"negative n"),
    ("negative stride", dict(z_stride_elems=-48), b"negative row stride"),
    ("stride smaller than the row", dict(z_stride_elems=46), b"smaller than the row"),
    ("both slab and list", dict(row_ids_dev=_FAKE), b"not both"),
    ("both slab and list, no labels", dict(y_dev=None, row_ids_dev=_FAKE), b"not both"),
    ("labels with neither", dict(y_row0=-1), b"need their rows"),
    ("negative y_rows", dict(y_rows=-1), b"y_rows"),
]


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses_before_anything_is_enqueued(what, over, word):
    nat, L = _lib()
    over = {k: getattr(nat, "SPP_ELEM_" + v) if isinstance(v, str) else v for k, v in over.items()}
    d = _desc(nat, **over)
    assert L.spp_classify_rows(ctypes.byref(d), None) == SPP_ERR_INVALID, what
    assert word in L.spp_last_error(), (what, L.spp_last_error())


def test_entry_refuses_a_null_descriptor_and_accepts_an_empty_call():
    nat, L = _lib()
    assert L.spp_classify_rows(None, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    # n == 0: nothing to do, SPP_OK without touching a device or a buffer -- with a slab, a list, or no labels
    for over in (dict(n=0), dict(n=0, y_row0=-1, row_ids_dev=_FAKE), dict(n=0, y_dev=None), dict(n=0, y_rows=0),
                 dict(n=0, pred_dev=None), dict(n=0, nll_dev=None)):
        assert L.spp_classify_rows(ctypes.byref(_desc(nat, **over)), None) == SPP_OK, over


def test_classify_rows_validates_before_any_device_call(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import TableRows
    from salient_plusplus_amd.inference import classify_rows
    z, y = torch.zeros((3, 5)), torch.zeros(9, dtype=torch.int64)
    with pytest.raises(TypeError, match="classify_rows.*TableRows"):
        classify_rows(TableRows(z, torch.tensor([0])))
    with pytest.raises(TypeError, match="classify_rows.*fp8"):
        classify_rows(fp8.quantize_e4m3(torch.zeros((3, 16))))
    with pytest.raises(TypeError, match="classify_rows: z must be a torch.Tensor"):
        classify_rows([[0.0]])
    with pytest.raises(ValueError, match="classify_rows: z must be fp32 or bf16"):
        classify_rows(z.half())
    with pytest.raises(ValueError, match="classify_rows: z must be a 2-D"):
        classify_rows(z.double())
    with pytest.raises(ValueError, match="classify_rows: z must be a 2-D"):
        classify_rows(z[0])
    with pytest.raises(ValueError, match="classify_rows: z must be a 2-D.*unit column stride"):
        classify_rows(torch.zeros((3, 10))[:, ::2])
    with pytest.raises(ValueError, match="classify_rows: z needs at least one column"):
        classify_rows(torch.zeros((3, 0)))
    with pytest.raises(RuntimeError, match="classify_rows: z requires grad"):
        classify_rows(z.clone().requires_grad_())
    with pytest.raises(TypeError, match="classify_rows: y must be a torch.Tensor"):
        classify_rows(z, [0, 1, 2], row0=0)
    with pytest.raises(ValueError, match="classify_rows: y must be a contiguous 1-D int64"):
        classify_rows(z, y.int(), row0=0)
    with pytest.raises(ValueError, match="classify_rows: y must be a contiguous 1-D int64"):
        classify_rows(z, y.view(9, 1), row0=0)
    with pytest.raises(ValueError, match="classify_rows: y must be a contiguous 1-D int64"):
        classify_rows(z, y[::2], row0=0)
    with pytest.raises(ValueError, match="classify_rows.*there is no y"):
        classify_rows(z, row0=0)
    with pytest.raises(ValueError, match="classify_rows.*there is no y"):
        classify_rows(z, row_ids=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="classify_rows: nll needs the labels y"):
        classify_rows(z, nll=torch.zeros(3))
    with pytest.raises(ValueError, match="classify_rows.*either as a slab"):
        classify_rows(z, y)
    with pytest.raises(ValueError, match="classify_rows.*row0.*row_ids.*not both"):
        classify_rows(z, y, row0=0, row_ids=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="classify_rows: row0"):
        classify_rows(z, y, row0=-1)
    with pytest.raises(ValueError, match="classify_rows: row_ids"):
        classify_rows(z, y, row_ids=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="classify_rows: row_ids"):
        classify_rows(z, y, row_ids=torch.tensor([0, 1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="classify_rows: pred must be"):
        classify_rows(z, pred=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="classify_rows: pred must be"):
        classify_rows(z, pred=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="classify_rows: pred must be"):
        classify_rows(z, pred=torch.zeros(6, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="classify_rows: nll must be"):
        classify_rows(z, y, row0=0, nll=torch.zeros(2))
    with pytest.raises(ValueError, match="classify_rows: nll must be"):
        classify_rows(z, y, row0=0, nll=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="classify_rows: nll must be"):
        classify_rows(z, y, row0=0, nll=torch.zeros((3, 1)))
    with pytest.raises(AssertionError, match="before the arguments were refused"):      # valid: it reaches the device
        classify_rows(z, y, row0=0)


def test_classify_rows_needs_the_device_for_valid_arguments():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.inference import classify_rows
    # no CPU fallback: without a device valid arguments fail at the device check, with one host tensors are refused
    refusal = (ValueError, "one CUDA device") if torch.cuda.is_available() else (nat.SppError, None)
    with pytest.raises(refusal[0], match=refusal[1]):
        classify_rows(torch.zeros((3, 4)))


def _graph():
    return torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])


def test_evaluate_validates_before_any_device_call(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import evaluate
    from salient_plusplus_amd.models import SAGE
    x, rowptr, col = _graph()
    y = torch.zeros(3, dtype=torch.int64)
    model = SAGE(4, 4, 2, 2)
    with pytest.raises(NotImplementedError, match="evaluate: implemented for"):
        evaluate(torch.nn.Linear(4, 2), x, rowptr, col)
    with pytest.raises(TypeError, match="evaluate.*fp8 feature table"):
        evaluate(model, fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col)
    with pytest.raises(ValueError, match="evaluate: x must be a 2-D"):
        evaluate(model, x.double(), rowptr, col)
    with pytest.raises(ValueError, match="evaluate: rowptr"):
        evaluate(model, x, rowptr.int(), col)
    with pytest.raises(ValueError, match="evaluate: x has 3 rows"):
        evaluate(model, x, rowptr[:3], col)
    with pytest.raises(ValueError, match="evaluate: act_dtype"):
        evaluate(model, x, rowptr, col, act_dtype=torch.float16)
    with pytest.raises(ValueError, match="evaluate: rows_per_slab"):
        evaluate(model, x, rowptr, col, rows_per_slab=0)
    with pytest.raises(ValueError, match="evaluate: nodes must be"):
        evaluate(model, x, rowptr, col, nodes=torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(TypeError, match="evaluate: y must be a torch.Tensor"):
        evaluate(model, x, rowptr, col, [0, 1, 1])
    with pytest.raises(ValueError, match="evaluate: y must be"):
        evaluate(model, x, rowptr, col, y.int())
    with pytest.raises(ValueError, match="evaluate: y must be"):
        evaluate(model, x, rowptr, col, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="evaluate: y must be"):
        evaluate(model, x, rowptr, col, y.view(3, 1))
    ids = torch.tensor([0, 2])
    with pytest.raises(ValueError, match="evaluate.*nodes or splits, not both"):
        evaluate(model, x, rowptr, col, y, nodes=ids, splits={"valid": ids})
    with pytest.raises(TypeError, match="evaluate: splits must be"):
        evaluate(model, x, rowptr, col, y, splits=[ids])
    with pytest.raises(TypeError, match="evaluate: splits must be"):
        evaluate(model, x, rowptr, col, y, splits={})
    with pytest.raises(ValueError, match="evaluate: splits\\['test'\\]"):
        evaluate(model, x, rowptr, col, y, splits={"valid": ids, "test": ids.int()})
    with pytest.raises(ValueError, match="evaluate: splits\\['valid'\\]"):
        evaluate(model, x, rowptr, col, y, splits={"valid": ids.view(1, 2)})
    with pytest.raises(AssertionError, match="before the arguments were refused"):      # valid: it reaches the device
        evaluate(model, x, rowptr, col, y, splits={"valid": ids})
    assert model.training


class _NoPeers:
    """peers that must never be reached: a refused call publishes nothing and waits for nobody"""

    def share(self, _t):
        raise AssertionError("share() was called by a refused call")

    barrier = close = share


def test_partitioned_evaluate_validates_before_peers_and_device(no_device):
    from salient_plusplus_amd.inference import partitioned_evaluate
    from salient_plusplus_amd.models import GAT, SAGE
    x, rowptr, col = _graph()
    model = SAGE(4, 4, 2, 2)
    kw = dict(part_offsets=[0, 2, 3], rank=0, peers=_NoPeers())
    y = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="partitioned_evaluate: implemented for"):
        partitioned_evaluate(torch.nn.Linear(4, 2), x[:2], rowptr, col, y, **kw)
    with pytest.raises(ValueError, match="partitioned_evaluate: x_local must be a 2-D"):
        partitioned_evaluate(model, x[:2].double(), rowptr, col, y, **kw)
    with pytest.raises(ValueError, match="partitioned_evaluate: x_local has 3 rows"):
        partitioned_evaluate(model, x, rowptr, col, y, **kw)
    with pytest.raises(ValueError, match="partitioned_evaluate: rank 2"):
        partitioned_evaluate(model, x[:2], rowptr, col, y, **dict(kw, rank=2))
    with pytest.raises(ValueError, match="partitioned_evaluate: act_dtype"):
        partitioned_evaluate(model, x[:2], rowptr, col, y, act_dtype=torch.float16, **kw)
    with pytest.raises(ValueError, match="partitioned_evaluate: nodes outside rank 0"):
        partitioned_evaluate(model, x[:2], rowptr, col, y, nodes=torch.tensor([2]), **kw)
    with pytest.raises(TypeError, match="partitioned_evaluate: y_local must be a torch.Tensor"):
        partitioned_evaluate(model, x[:2], rowptr, col, [0, 1], **kw)
    with pytest.raises(ValueError, match="partitioned_evaluate: y_local must be"):
        partitioned_evaluate(model, x[:2], rowptr, col, y.int(), **kw)
    with pytest.raises(ValueError, match="partitioned_evaluate: y_local must be"):
        partitioned_evaluate(model, x[:2], rowptr, col, torch.zeros(3, dtype=torch.int64), **kw)
    with pytest.raises(TypeError, match="partitioned_evaluate: peers must provide"):
        partitioned_evaluate(model, x[:2], rowptr, col, y, **dict(kw, peers=object()))
    with pytest.raises(AssertionError, match="before the arguments were refused"):      # valid: it reaches the device
        partitioned_evaluate(GAT(4, 4, 2, 2, heads=1), x[:2], rowptr, col, y, **kw)
    assert model.training
