"""CPU-only: the host side of exact layer-wise inference -- argument validation of inference.graph_aggregate and
layerwise_inference (before any device call), every model's ``.inference`` being that function, the resident-graph
accessor's refusals, and the ctypes layout of spp_graph_agg_desc against the header."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny():
    x = torch.zeros((3, 4))
    return x, torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])


def test_graph_agg_desc_layout_matches_header():
    """sizeof and every field offset of spp_graph_agg_desc, cross-checked by compiling the header with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.GraphAggDesc._fields_]
    offs = ", ".join(f"offsetof(spp_graph_agg_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_graph_agg_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(nat.GraphAggDesc)] + [getattr(nat.GraphAggDesc, n).offset for n in names]


def test_library_exports_the_graph_aggregation():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    from salient_plusplus_amd.inference import graph_agg_chunk, graph_agg_workspace_bytes
    build.build()
    L = nat.load()
    for name in ("spp_graph_agg_forward", "spp_graph_agg_chunk", "spp_graph_agg_workspace_bytes"):
        assert hasattr(L, name) and name in nat.SIGNATURES
    assert graph_agg_chunk() >= 32
    assert graph_agg_workspace_bytes(0) >= 16 and graph_agg_workspace_bytes(1000) >= 8 * 1000
    assert L.spp_abi_version() == 6
    # the entry validates before it touches a device: a refusal needs no GPU
    d = nat.GraphAggDesc(epilogue=nat.SPP_AGG_OPERAND_ACT)
    assert L.spp_graph_agg_forward(ctypes.byref(d), None, 0, None) == -1
    assert b"epilogue" in L.spp_last_error()


def test_graph_aggregate_validates_its_arguments():
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from salient_plusplus_amd.inference import graph_aggregate
    x, rowptr, col = _tiny()
    with pytest.raises(ValueError, match="not both"):
        graph_aggregate(x, rowptr, col, row0=0, num_targets=3, target_ids=torch.tensor([0]))
    with pytest.raises(ValueError, match="either as a slab"):
        graph_aggregate(x, rowptr, col)
    with pytest.raises(ValueError, match="both row0 and num_targets"):
        graph_aggregate(x, rowptr, col, row0=0)
    with pytest.raises(ValueError, match="leaves the graph"):
        graph_aggregate(x, rowptr, col, row0=2, num_targets=2)
    with pytest.raises(ValueError, match="epilogue"):
        graph_aggregate(x, rowptr, col, row0=0, num_targets=3, epilogue="operand_act")
    with pytest.raises(ValueError, match="out_dtype"):
        graph_aggregate(x, rowptr, col, row0=0, num_targets=3, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="target_ids"):
        graph_aggregate(x, rowptr, col, target_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="one row per node"):
        graph_aggregate(x, rowptr[:-1], col, row0=0, num_targets=1)
    with pytest.raises(ValueError, match="int64"):
        graph_aggregate(x, rowptr.int(), col, row0=0, num_targets=1)
    with pytest.raises(ValueError, match="2-D"):
        graph_aggregate(x.double(), rowptr, col, row0=0, num_targets=1)
    with pytest.raises(RuntimeError, match="requires grad"):
        graph_aggregate(x.clone().requires_grad_(), rowptr, col, row0=0, num_targets=1)
    with pytest.raises(TypeError, match="fp8"):
        graph_aggregate(fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col, row0=0, num_targets=1)
    with pytest.raises(TypeError, match="TableRows"):
        graph_aggregate(TableRows(x, torch.tensor([0])), rowptr, col, row0=0, num_targets=1)
    with pytest.raises(TypeError, match="RowRefs"):
        graph_aggregate(RowRefs(torch.zeros(3, dtype=torch.int64), None, 4, torch.float16, None, ()), rowptr, col,
                        row0=0, num_targets=1)


def test_layerwise_inference_validates_and_models_refuse_with_a_reason():
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import GAT, GIN, SAGE, SAGEResInception
    x, rowptr, col = _tiny()
    sage = SAGE(4, 4, 2, 2)
    from inference_method import assert_method_is_the_function
    for model in (GAT(4, 4, 2, 2), GAT(4, 4, 2, 2, heads=2), SAGEResInception(4, 4, 2, 2), sage, GIN(4, 4, 2, 2)):
        assert_method_is_the_function(model, x, rowptr, col)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: implemented for SAGE, GIN, GAT, SAGEResInception, GCN and GATv2, not Linear$"):
        layerwise_inference(torch.nn.Linear(4, 2), x, rowptr, col)
    with pytest.raises(TypeError, match="fp8 feature table"):
        sage.inference(fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col)
    with pytest.raises(ValueError, match="act_dtype"):
        sage.inference(x, rowptr, col, act_dtype=torch.float16)
    with pytest.raises(ValueError, match="rows_per_slab"):
        GIN(4, 4, 2, 2).inference(x, rowptr, col, rows_per_slab=0)
    with pytest.raises(ValueError, match="nodes"):
        sage.inference(x, rowptr, col, nodes=torch.tensor([0.5]))
    assert sage.training                                      # a refused call leaves the mode alone
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        from salient_plusplus_amd import _native as nat
        with pytest.raises(nat.SppError):
            sage.inference(x, rowptr, col)
        assert sage.training


def test_resident_graph_refuses_what_inference_cannot_read():
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd import fp8
    cfg = fs.Config()
    cfg.rowptr, cfg.col, cfg.x_cpu = torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros((1, 16))
    cfg.distributed = True
    with pytest.raises(RuntimeError, match="distributed"):
        fs.resident_graph(cfg)
    cfg.distributed = False
    cfg.x_cpu = fp8.quantize_e4m3(torch.zeros((1, 16)))
    with pytest.raises(RuntimeError, match="fp8"):
        fs.resident_graph(cfg)
    cfg.x_cpu = None
    with pytest.raises(RuntimeError, match="no feature table"):
        fs.resident_graph(cfg)
