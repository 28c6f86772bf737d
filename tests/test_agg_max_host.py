"""CPU-only: max aggregation (SAGEConv(aggr="max")) without a device -- the descriptors of spp_agg_max_forward /
spp_agg_max_backward against the header, every refusal the two entries make before a launch, the Python argument checks,
the state dict of SAGE(aggr="max"), the default model's fast path, the plain-torch restatement _max_reference against
a literal loop, and the refusals of the partitioned entries."""
import ctypes
import math
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


@pytest.mark.parametrize("struct,cname", [("AggMaxFwdDesc", "spp_agg_max_fwd_desc"), ("AggMaxBwdDesc", "spp_agg_max_bwd_desc")])
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


def test_library_exports_the_entries():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    for name in ("spp_agg_max_forward", "spp_agg_max_backward"):
        assert hasattr(L, name) and name in nat.SIGNATURES and f"spp_status {name}(" in header
    assert (nat.SPP_AGG_MAX, nat.SPP_AGG_MAX_OPERAND) == (4, 5)
    assert "SPP_AGG_MAX = 4, SPP_AGG_MAX_OPERAND = 5" in header


def _fwd(nat, **over):
    kw = dict(source=nat.SPP_AGG_DENSE, x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, concat_target=0,
              rowptr_dev=_FAKE, col_dev=_FAKE, num_targets=5, x_dev=_FAKE, x_stride_elems=8, x_rows=0, n_id_dev=None,
              scale_log2_dev=None, F=8, out_dev=_FAKE, out_stride_elems=0, arg_dev=_FAKE)
    kw.update(over)
    return nat.AggMaxFwdDesc(**kw)


def _bwd(nat, **over):
    kw = dict(grad_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, concat_target=0, arg_dev=_FAKE, num_targets=5,
              num_sources=9, grad_out_dev=_FAKE, grad_out_stride_elems=0, F=8, grad_x_dev=_FAKE, workspace_dev=None,
              workspace_bytes=0)
    kw.update(over)
    return nat.AggMaxBwdDesc(**kw)


def test_forward_refusals_come_before_any_launch():
    nat, L = _lib()
    fp8 = dict(x_elem=nat.SPP_ELEM_FP8_E4M3, scale_log2_dev=_FAKE)
    cases = {
        "unknown source": (dict(source=3), b"source"),
        "negative source": (dict(source=-1), b"source"),
        "unknown x code": (dict(x_elem=7), b"element code"),
        "fp16 output": (dict(out_elem=nat.SPP_ELEM_F16), b"element code"),
        "fp8 output": (dict(out_elem=nat.SPP_ELEM_FP8_E4M3), b"element code"),
        "fp8 rows to an fp16 output": (dict(fp8, out_elem=nat.SPP_ELEM_F16), b"element code"),
        "fp8 rows without exponents": (dict(fp8, scale_log2_dev=None), b"exponents"),
        "fp8 row references": (dict(fp8, source=nat.SPP_AGG_ROWS, n_id_dev=_FAKE), b"fp8"),
        "fp8 rows, F % 4": (dict(fp8, F=6, x_stride_elems=6), b"fp8"),
        "negative T": (dict(num_targets=-1), b"negative"),
        "negative F": (dict(F=-8), b"negative"),
        "T * F out of range": (dict(num_targets=1 << 60), b"out of range"),
        "row stride": (dict(x_stride_elems=7), b"row stride"),
        "output stride": (dict(out_stride_elems=7), b"output stride"),
        "operand output stride": (dict(concat_target=1, out_stride_elems=8), b"output stride"),
        "negative output stride": (dict(out_stride_elems=-1), b"output stride"),
        "NULL rowptr": (dict(rowptr_dev=None), b"NULL"),
        "NULL col": (dict(col_dev=None), b"NULL"),
        "NULL x": (dict(x_dev=None), b"NULL"),
        "NULL out": (dict(out_dev=None), b"NULL"),
        "table without ids": (dict(source=nat.SPP_AGG_TABLE, x_rows=10), b"NULL"),
        "empty table": (dict(source=nat.SPP_AGG_TABLE, n_id_dev=_FAKE, x_rows=0), b"empty table"),
        "row references without addresses": (dict(source=nat.SPP_AGG_ROWS), b"NULL"),
        "misaligned out": (dict(out_dev=_FAKE + 2), b"misaligned"),
        "misaligned arg": (dict(arg_dev=_FAKE + 2), b"misaligned"),
        "misaligned x": (dict(x_dev=_FAKE + 1, x_elem=nat.SPP_ELEM_BF16), b"misaligned"),
    }
    for what, (over, text) in cases.items():
        assert L.spp_agg_max_forward(ctypes.byref(_fwd(nat, **over)), None) == SPP_ERR_INVALID, what
        msg = L.spp_last_error()
        assert b"spp_agg_max_forward" in msg and text in msg, (what, msg)
    assert L.spp_agg_max_forward(None, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    # nothing to do: SPP_OK without a launch (and without a look at the pointers)
    for over in (dict(num_targets=0), dict(F=0, x_stride_elems=0), dict(num_targets=0, rowptr_dev=None, out_dev=None)):
        assert L.spp_agg_max_forward(ctypes.byref(_fwd(nat, **over)), None) == SPP_OK, over


def test_backward_refusals_come_before_any_launch():
    nat, L = _lib()
    cases = {
        "fp16 gradient": (dict(grad_elem=nat.SPP_ELEM_F16), b"element code"),
        "fp8 output": (dict(out_elem=nat.SPP_ELEM_FP8_E4M3), b"element code"),
        "unknown code": (dict(out_elem=9), b"element code"),
        "negative T": (dict(num_targets=-1), b"bad sizes"),
        "S < T": (dict(num_sources=4), b"bad sizes"),
        "negative F": (dict(F=-1), b"bad sizes"),
        "S beyond int32": (dict(num_sources=1 << 31), b"2^31"),
        "S * F out of range": (dict(num_sources=(1 << 31) - 1, F=1 << 40), b"out of range"),
        "gradient stride": (dict(grad_out_stride_elems=7), b"gradient stride"),
        "operand gradient stride": (dict(concat_target=1, grad_out_stride_elems=8), b"gradient stride"),
        "NULL grad_x": (dict(grad_x_dev=None), b"NULL"),
        "NULL grad_out": (dict(grad_out_dev=None), b"NULL"),
        "NULL arg": (dict(arg_dev=None), b"NULL"),
        "misaligned grad_x": (dict(grad_x_dev=_FAKE + 2), b"misaligned"),
        "misaligned arg": (dict(arg_dev=_FAKE + 1), b"misaligned"),
        "bf16 without a workspace": (dict(out_elem=nat.SPP_ELEM_BF16), b"workspace"),
        "bf16, small workspace": (dict(out_elem=nat.SPP_ELEM_BF16, workspace_dev=_FAKE, workspace_bytes=4 * 9 * 8 - 1),
                                  b"workspace"),
        "bf16, misaligned workspace": (dict(out_elem=nat.SPP_ELEM_BF16, workspace_dev=_FAKE + 8, workspace_bytes=1 << 20),
                                       b"workspace"),
    }
    for what, (over, text) in cases.items():
        assert L.spp_agg_max_backward(ctypes.byref(_bwd(nat, **over)), None) == SPP_ERR_INVALID, what
        msg = L.spp_last_error()
        assert b"spp_agg_max_backward" in msg and text in msg, (what, msg)
    assert L.spp_agg_max_backward(None, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    for over in (dict(num_targets=0, num_sources=0), dict(F=0)):
        assert L.spp_agg_max_backward(ctypes.byref(_bwd(nat, **over)), None) == SPP_OK, over


def test_the_older_entries_still_refuse_the_max_codes():
    """spp_agg_forward / spp_agg_backward accept what they accepted; the parts entry refuses the maximum"""
    nat, L = _lib()
    for code in (nat.SPP_AGG_MAX, nat.SPP_AGG_MAX_OPERAND):
        assert L.spp_agg_forward(ctypes.byref(nat.AggFwdDesc(epilogue=code)), None) == SPP_ERR_INVALID
        assert b"epilogue" in L.spp_last_error()
        assert L.spp_agg_backward(ctypes.byref(nat.AggBwdDesc(epilogue=code)), None, 0, None) == SPP_ERR_INVALID
        d = nat.GraphAggPartsDesc(epilogue=code, x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, num_parts=1)
        d.part_offsets[1] = 4
        d.x_parts_dev[0] = _FAKE
        assert L.spp_graph_agg_parts_forward(ctypes.byref(d), None, 0, None) == SPP_ERR_INVALID
        assert b"epilogue" in L.spp_last_error()


def test_python_argument_checks():
    from salient_plusplus_amd.fast_sampler import TableRows
    from salient_plusplus_amd.fast_trainer.samplers import Adj__from_fast_sampler
    from salient_plusplus_amd.inference import graph_aggregate
    from salient_plusplus_amd.models import SAGE, SAGEConv, max_aggregate
    for bad in ("sum", "MAX", None, 1):
        with pytest.raises(ValueError, match="aggr must be 'mean' or 'max'"):
            SAGE(8, 8, 3, 2, aggr=bad)
        with pytest.raises(ValueError, match="aggr must be 'mean' or 'max'"):
            SAGEConv(8, 8, aggr=bad)
    with pytest.raises(TypeError):
        SAGE(8, 8, 3, 2, "max")                              # keyword only
    rowptr, col = torch.tensor([0, 1, 2]), torch.tensor([0, 1])
    x = torch.zeros((3, 4))
    with pytest.raises(ValueError, match="max_aggregate: x must be a 2-D fp32 / fp16 / bf16"):
        max_aggregate(x.double(), rowptr, col, 2)
    with pytest.raises(ValueError, match="max_aggregate: x must be a 2-D"):
        max_aggregate(x.long(), rowptr, col, 2)
    with pytest.raises(ValueError, match="max_aggregate: x must be a 2-D"):
        max_aggregate(x[0], rowptr, col, 2)
    with pytest.raises(TypeError, match="max_aggregate: x must be a tensor"):
        max_aggregate([[0.0]], rowptr, col, 2)
    # rows read in place are their own targets
    adj = Adj__from_fast_sampler((rowptr, col, torch.empty(0, dtype=torch.int64), (2, 3)))
    with pytest.raises(RuntimeError, match="first rows of x"):
        SAGEConv(4, 4, aggr="max")((TableRows(x, torch.arange(3)), x[:2]), adj.adj_t)
    # the resident entry takes the table itself, not a TableRows
    with pytest.raises(TypeError, match="TableRows"):
        graph_aggregate(TableRows(x, torch.arange(3)), rowptr, col, row0=0, num_targets=2, epilogue="max")
    with pytest.raises(ValueError, match="epilogue"):
        graph_aggregate(x, torch.tensor([0, 1, 2, 2]), col, row0=0, num_targets=2, epilogue="max_act")


def test_state_dict_is_the_mean_models_and_the_default_keeps_its_fast_path(monkeypatch):
    from salient_plusplus_amd import models
    torch.manual_seed(0)
    a = models.SAGE(128, 256, 47, 3, aggr="max")
    torch.manual_seed(0)
    b = models.SAGE(128, 256, 47, 3, aggr="mean")
    c = models.SAGE(128, 256, 47, 3)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == list(c.state_dict())
    assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]) for k in sa)
    b.load_state_dict(sa)
    assert a.aggr == "max" and b.aggr == c.aggr == "mean" and all(conv.aggr == "max" for conv in a.convs)
    # the default model still hands its batch to _SageStack; the max model never does
    seen = []

    class Taken(Exception):
        pass

    def apply(*args):
        seen.append(args)
        raise Taken

    monkeypatch.setattr(models._SageStack, "usable", staticmethod(lambda model, x, adjs: True))
    monkeypatch.setattr(models._SageStack, "apply", staticmethod(apply))

    class X:                                                 # (a stand-in for a CUDA matrix: only is_cuda is asked)
        is_cuda = True
    with pytest.raises(Taken):
        c(X(), [])
    assert len(seen) == 1
    assert a(torch.zeros((2, 47)), []).shape == (2, 47) and len(seen) == 1      # (no layers run: log_softmax only)


def _loop_reference(x, rowptr, col, T):
    """the contract, literally: from the first entry on, a later value replaces the best only if !(v <= best) and the
    best is not a NaN"""
    F = len(x[0])
    out = [[0.0] * F for _ in range(T)]
    arg = [[-1] * F for _ in range(T)]
    for t in range(T):
        for c in range(F):
            for k in range(rowptr[t], rowptr[t + 1]):
                v = x[col[k]][c]
                if k == rowptr[t] or (not (v <= out[t][c]) and out[t][c] == out[t][c]):
                    out[t][c], arg[t][c] = v, col[k]
    return out, arg


def test_max_reference_against_a_literal_loop():
    from salient_plusplus_amd.models import _max_reference
    nan, inf = float("nan"), float("inf")
    x = [[1.0, -2.0, 0.0, -inf],          # 0
         [3.0, -1.0, -0.0, -inf],         # 1
         [3.0, -5.0, 0.0, 2.0],           # 2
         [nan, -1.0, -0.0, nan],          # 3
         [7.0, -3.0, -0.0, 9.0],          # 4
         [-4.0, -4.0, -4.0, -4.0],        # 5
         [2.0, nan, 0.0, -inf]]           # 6
    rows = [[],                           # an empty row
            [5],                          # one entry
            [1, 2, 1, 0],                 # a duplicate edge and a tie (3.0 twice: the first stays), -0.0 before +0.0
            [5, 1, 0],                    # all negative in column 1; -inf in column 3
            [2, 3, 4],                    # a NaN before a larger value: the NaN stays
            [4, 3, 6, 2],                 # a NaN after a larger value: the NaN wins
            [0, 1, 6]]                    # only -inf in column 3; +0.0 before -0.0
    rowptr, col = [0], []
    for r in rows:
        col += r
        rowptr.append(len(col))
    want_out, want_arg = _loop_reference(x, rowptr, col, len(rows))
    out, arg = _max_reference(torch.tensor(x), torch.tensor(rowptr), torch.tensor(col), len(rows))
    assert out.dtype == torch.float32 and arg.dtype == torch.int32
    assert arg.tolist() == want_arg
    got = out.tolist()
    for t in range(len(rows)):
        for c in range(4):
            g, w = got[t][c], want_out[t][c]
            assert (math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1, g) == math.copysign(1, w)), (t, c, g, w)
    # the cases, spelled out
    assert got[0] == [0.0] * 4 and want_arg[0] == [-1] * 4
    assert got[1] == [-4.0] * 4 and want_arg[1] == [5] * 4
    assert want_arg[2][0] == 1 and math.copysign(1, got[2][2]) == -1 and want_arg[2][2] == 1
    assert got[3][1] == -1.0 and want_arg[3][1] == 1 and got[3][3] == -4.0 and want_arg[3][3] == 5
    assert math.isnan(got[4][0]) and want_arg[4][0] == 3 and math.isnan(got[5][0]) and want_arg[5][0] == 3
    assert math.isnan(got[5][3]) and want_arg[5][3] == 3
    assert got[6][3] == -inf and want_arg[6][3] == 0 and math.copysign(1, got[6][2]) == 1
    # fp16 and bf16 rows are read exactly
    for dt in (torch.float16, torch.bfloat16):
        o2, a2 = _max_reference(torch.tensor(x).to(dt), torch.tensor(rowptr), torch.tensor(col), len(rows))
        assert torch.equal(a2, arg) and torch.equal(o2.view(torch.int32)[~out.isnan()], out.view(torch.int32)[~out.isnan()])


def test_partitioned_entries_refuse_the_max_model():
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import SAGE
    model = SAGE(8, 8, 3, 2, aggr="max")
    x = torch.zeros((4, 8))
    rowptr, col = torch.tensor([0, 1, 2, 2, 2]), torch.tensor([1, 0])
    kw = dict(part_offsets=[0, 4], rank=0, peers=None)
    for entry in (inf.partitioned_inference, inf.partitioned_layerwise_inference, inf.partitioned_evaluate):
        with pytest.raises(NotImplementedError, match="aggr='max'.*not built over a row-partitioned table"):
            entry(model, x, rowptr, col, **kw)
    for epilogue in ("max", "max_operand"):
        with pytest.raises(NotImplementedError, match="not built over a row-partitioned table"):
            inf.graph_aggregate_parts([x], [0, 4], rowptr, col, row0=0, num_targets=4, epilogue=epilogue)
