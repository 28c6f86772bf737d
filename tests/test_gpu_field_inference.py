"""-m gpu: inference.field_inference / field_evaluate against the existing whole-graph path on the same arguments --
layerwise_inference(..., nodes=nodes) and evaluate(..., nodes= / splits=) -- BIT FOR BIT, no tolerance: the field entries
run the same kernels and the same fixed GEMM tiles over the nodes within L - 1 hops of ``nodes`` only, and a row's bits
depend on its own row alone.  The graph is test_gpu_field's (a hub of 3 000 entries, a node without edges, a self-loop,
repeated entries, two disconnected components); the scored nodes are its 300 random ones (unsorted, with duplicates, in
both components) plus the hub, the node without edges and the self-loop."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_field import HUB, LONE, LOOP, N, NA, graph, node_sets  # noqa: E402

pytestmark = pytest.mark.gpu

HID, CLASSES = 16, 5
KINDS = ["sage", "gin", "gat1", "gat2"]
DTYPES = [torch.float32, torch.bfloat16]
_ID = dict(ids=lambda v: str(v).split(".")[-1])


@functools.lru_cache(maxsize=None)
def _x(F):
    g = torch.Generator().manual_seed(40 + F)
    return torch.randn((N, F), generator=g).to(torch.float16).cuda()


@functools.lru_cache(maxsize=None)
def _nodes():
    return torch.from_numpy(np.concatenate([node_sets()["random300"], [HUB, LONE, LOOP, HUB]])).cuda()


@functools.lru_cache(maxsize=None)
def _labels():
    """one label per node: a fifth of them -1 (unlabelled), some outside [0, classes)"""
    g = torch.Generator().manual_seed(9)
    y = torch.randint(0, CLASSES, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.2] = -1
    y[torch.rand(N, generator=g) < 0.05] = CLASSES + 2
    return y.cuda()


@functools.lru_cache(maxsize=None)
def _model(kind, F, L):
    """L conv layers.  The constructors of SAGE and GAT build at least two, so a one-layer model is their first layer
    made the last: in -> classes, and for two heads the mean of the heads (concat=False)"""
    from salient_plusplus_amd.models import GAT, GATConv, GIN, SAGE, SAGEConv, SAGEResInception
    torch.manual_seed(3)
    heads = 2 if kind == "gat2" else 1
    if kind == "gin":
        m = GIN(F, HID, CLASSES, L)
    elif kind == "sageri":
        m = SAGEResInception(F, HID, CLASSES, L)
    elif kind == "sage":
        m = SAGE(F, HID, CLASSES, max(L, 2))
        if L == 1:
            m.convs = torch.nn.ModuleList([SAGEConv(F, CLASSES, bias=False)])
    else:
        m = GAT(F, HID, CLASSES, max(L, 2), heads=heads)
        if L == 1:
            m.convs = torch.nn.ModuleList([GATConv(F, CLASSES, heads=heads, concat=heads == 1, bias=False)])
    m.num_layers = L
    assert len(m.convs) == L
    g = torch.Generator().manual_seed(8)
    for mod in m.modules():                                    # non-trivial running statistics and affine terms
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.5)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.0 + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _fields():
    from salient_plusplus_amd.inference import ReceptiveFields
    return ReceptiveFields(*graph())


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("rows_per_slab", [64, 1 << 20])
@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("F", [8, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_field_inference_is_layerwise_inference_bit_for_bit(kind, F, L, act_dtype, rows_per_slab):
    from salient_plusplus_amd.inference import field_inference, layerwise_inference
    rowptr, col = graph()
    model, x, nodes = _model(kind, F, L), _x(F), _nodes()
    kw = dict(rows_per_slab=rows_per_slab, act_dtype=act_dtype)
    want = layerwise_inference(model, x, rowptr, col, nodes=nodes, **kw)
    # a reused ReceptiveFields for one slab size, a temporary one for the other
    got = field_inference(model, x, rowptr, col, nodes, fields=_fields() if rows_per_slab == 64 else None, **kw)
    assert got.dtype == torch.float32 and got.shape == (nodes.numel(), CLASSES) and got.is_cuda
    assert bool(torch.isfinite(want).all())
    assert torch.equal(_bits(got), _bits(want))
    assert not model.training


@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("kind", KINDS)
def test_field_evaluate_is_evaluate(kind, act_dtype):
    from salient_plusplus_amd.inference import Evaluation, evaluate, field_evaluate
    rowptr, col = graph()
    model, x, nodes, y = _model(kind, 8, 3), _x(8), _nodes(), _labels()
    picked = y[nodes]
    assert bool((picked == -1).any()) and bool((picked >= CLASSES).any())           # both kinds of "no label" are scored
    splits = {"valid": nodes[:120], "test": nodes[100:]}                            # (two lists that share nodes)
    for kw in (dict(nodes=nodes), dict(splits=splits)):
        want = evaluate(model, x, rowptr, col, y, rows_per_slab=500, act_dtype=act_dtype, **kw)
        got = field_evaluate(model, x, rowptr, col, y, rows_per_slab=500, act_dtype=act_dtype, fields=_fields(), **kw)
        assert isinstance(got, Evaluation)
        assert torch.equal(got.pred, want.pred) and torch.equal(_bits(got.nll), _bits(want.nll))
        assert (got.labelled, got.correct) == (want.labelled, want.correct) and 0 < got.labelled < got.pred.numel()
        assert got.loss == want.loss and got.splits == want.splits
        assert set(got.splits) == (set(splits) if "splits" in kw else set())
    # without labels: predictions only
    want = evaluate(model, x, rowptr, col, nodes=nodes, act_dtype=act_dtype)
    got = field_evaluate(model, x, rowptr, col, nodes=nodes, act_dtype=act_dtype)
    assert got.nll is None and got.labelled is None and torch.equal(got.pred, want.pred)


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_field_is_read(kind):
    """every scored node lies in component A; the rows of x in component B are NaN: the result is what it was, finite,
    and no node of B is in the field"""
    from salient_plusplus_amd.inference import field_inference, receptive_field
    rowptr, col = graph()
    model, x = _model(kind, 8, 3), _x(8)
    nodes = _nodes()
    nodes = nodes[nodes < NA]
    assert nodes.numel() > 250
    want = field_inference(model, x, rowptr, col, nodes)
    poisoned = x.clone()
    poisoned[NA:] = float("nan")
    got = field_inference(model, poisoned, rowptr, col, nodes)
    assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want))
    f = receptive_field(rowptr, col, nodes, 2)
    assert int(f.ids.max()) < NA and f.sizes[2] < NA         # (GAT projects the whole table first: the NaN rows of x
                                                             #  become NaN rows of h, which no row of A reads)


@pytest.mark.parametrize("kind", KINDS)
def test_no_nodes_give_an_empty_result(kind):
    from salient_plusplus_amd.inference import field_evaluate, field_inference
    rowptr, col = graph()
    model, x = _model(kind, 8, 2), _x(8)
    none = torch.empty(0, dtype=torch.int64)
    out = field_inference(model, x, rowptr, col, none)
    assert out.shape == (0, CLASSES) and out.dtype == torch.float32 and out.device == x.device
    ev = field_evaluate(model, x, rowptr, col, _labels(), nodes=none.cuda())
    assert ev.pred.shape == (0,) and ev.nll.shape == (0,) and ev.labelled == 0 and ev.correct == 0 and ev.loss != ev.loss


def test_a_field_made_for_another_graph_is_refused():
    from salient_plusplus_amd.inference import ReceptiveFields, field_inference
    rowptr, col = graph()
    other = ReceptiveFields(rowptr.clone(), col.clone())
    with pytest.raises(ValueError, match="field_inference: fields was made for another graph"):
        field_inference(_model("sage", 8, 2), _x(8), rowptr, col, _nodes(), fields=other)


def test_sage_res_inception_is_refused_with_the_reason():
    from salient_plusplus_amd.inference import field_evaluate, field_inference
    rowptr, col = graph()
    model = _model("sageri", 8, 2)
    for fn, kw in ((field_inference, dict(nodes=_nodes())), (field_evaluate, dict(nodes=_nodes()))):
        with pytest.raises(NotImplementedError, match="head accumulates a block of every layer"):
            fn(model, _x(8), rowptr, col, **kw)
