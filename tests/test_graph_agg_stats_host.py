"""CPU-only (spp.h f4e): spp_graph_agg_stats_desc against the header, graph_stats_aggregate's argument checks, and PNA's
admission to the resident entries with every refusal that names it, in the wording the entries already had."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RP, CL = torch.tensor([0, 2, 2, 5, 5, 5]), torch.tensor([4, 1, 0, 3, 3])


def test_descriptor_size_matches_the_header(tmp_path):
    from salient_plusplus_amd import _native as nat, build
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "spp.h"\nint main(void) { printf("%zu\\n", '
                   "sizeof(spp_graph_agg_stats_desc)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")])
    assert int(subprocess.check_output([str(tmp_path / "t")])) == ctypes.sizeof(nat.GraphAggStatsDesc)
    flags = build.SOURCE_FLAGS
    assert "graph_agg_stats.hip" in build.SOURCES and flags["graph_agg_stats.hip"] == flags["aggregate_stats.hip"]


@pytest.mark.parametrize("F,kw,text", [
    (8, dict(scalers=("attenuation", "identity")), "scalers"), (8, dict(scalers=()), "scalers"),
    (8, dict(delta=0.0), "delta"), (8, dict(delta=float("inf")), "delta"),
    (8, dict(row0=0, num_targets=5, target_ids=torch.tensor([1])), "not both"), (6, dict(row0=0, num_targets=5), "F % 4"),
], ids=["scaler_order", "no_scaler", "delta_0", "delta_inf", "both_target_forms", "F_6"])
def test_graph_stats_aggregate_checks_its_arguments(F, kw, text):
    from salient_plusplus_amd.inference import graph_stats_aggregate
    with pytest.raises(ValueError, match=text):
        graph_stats_aggregate(torch.zeros((5, F)), RP, CL, **kw)


def test_pna_is_admitted_by_the_resident_entries_only():
    from salient_plusplus_amd import inference as I
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fp8 import Fp8Features
    model = models.PNA(8, 16, 4, 2, delta=1.2)
    assert not hasattr(model, "inference")
    x = torch.zeros((5, 8))
    with pytest.raises(NotImplementedError, match="implemented for SAGE, GIN, GAT, SAGEResInception, GCN and GATv2, not Linear"):
        I.layerwise_inference(torch.nn.Linear(2, 2), x, RP, CL)
    with pytest.raises(NotImplementedError, match="implemented for SAGE, GIN and GAT, not PNA"):
        I.field_inference(model, x, RP, CL, torch.tensor([1]))
    with pytest.raises(NotImplementedError, match="implemented for SAGE, GIN, GAT and SAGEResInception, not PNA"):
        I.partitioned_inference(model, x, RP, CL, part_offsets=[0, 5], rank=0, peers=None)
    table = I.Fp8Table(Fp8Features(torch.zeros((5, 16), dtype=torch.float8_e4m3fn), torch.zeros(16, dtype=torch.int8)))
    with pytest.raises(TypeError, match="PNA: a PNA model is scored over one resident"):
        I.layerwise_inference(model, table, RP, CL)
    with pytest.raises(ValueError, match="edge_weight is GCN's"):
        I.evaluate(model, x, RP, CL, edge_weight=torch.ones(5))
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        I.layerwise_inference(models.PNA(6, 16, 4, 2, delta=1.2), x, RP, CL)
