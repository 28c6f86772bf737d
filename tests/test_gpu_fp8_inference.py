"""-m gpu: the resident drivers over an fp8 table read in place (inference.Fp8Table, f3o) against the same call on the
table dequantised to fp32 -- ``torch.equal``, no tolerance: layer 0's aggregation (spp_graph_agg_forward_fp8) and the
GEMM tiles of the table's own rows (spp_fp8_rows_f32) yield exactly v = float32(q) * 2^scale_log2, and everything behind
them is the fp32-table code path.  SAGE, GIN, GAT (heads 1 and 4) and SAGEResInception, fp32 and bf16 activations, all
nodes and ``nodes=``, ``evaluate`` with splits, and the field entries (SAGE, GIN, GAT)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, FIN, HID, CLASSES, LAYERS = 1500, 32, 16, 7, 3
SLAB = 401                                                     # below N: four slabs, the last one partial
KINDS = ["sage", "gin", "gat1", "gat4", "sageri"]
DTYPES = [torch.float32, torch.bfloat16]
_ID = dict(ids=lambda v: str(v).split(".")[-1])


@functools.lru_cache(maxsize=None)
def _data():
    """(Fp8Table on the GPU, its fp32 dequantisation computed on the CPU and copied, rowptr, col, y): degrees 0..12 and
    one hub row of 3 * 64 + 5 entries (longer than the aggregation chunk); columns of very different magnitudes, so
    that the exponents differ"""
    from salient_plusplus_amd.fp8 import quantize_e4m3
    from salient_plusplus_amd.inference import Fp8Table, graph_agg_chunk
    g = torch.Generator().manual_seed(23)
    deg = torch.randint(0, 13, (N,), generator=g)
    deg[700] = 3 * graph_agg_chunk() + 5
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    x = torch.randn((N, FIN), generator=g) * torch.logspace(-3, 2, FIN)
    x8 = quantize_e4m3(x)
    assert x8.scale_log2.unique().numel() > 8
    y = torch.randint(0, CLASSES, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.2] = -1
    return Fp8Table(x8.to("cuda")), x8.dequantize(torch.float32).cuda(), rowptr.cuda(), col.cuda(), y.cuda()


@functools.lru_cache(maxsize=None)
def _model(kind):
    from salient_plusplus_amd.models import GAT, GIN, SAGE, SAGEResInception
    torch.manual_seed(5)
    m = {"sage": lambda: SAGE(FIN, HID, CLASSES, LAYERS), "gin": lambda: GIN(FIN, HID, CLASSES, LAYERS),
         "gat1": lambda: GAT(FIN, HID, CLASSES, LAYERS, heads=1), "gat4": lambda: GAT(FIN, HID, CLASSES, LAYERS, heads=4),
         "sageri": lambda: SAGEResInception(FIN, HID, CLASSES, LAYERS)}[kind]()
    g = torch.Generator().manual_seed(9)
    for mod in m.modules():                                    # non-trivial running statistics and affine terms
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.5)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.0 + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _nodes():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, N, (90,), generator=g)
    ids[0], ids[1], ids[2] = 700, N - 1, 700                  # the hub, twice, and the last node
    return ids.cuda()


@functools.lru_cache(maxsize=None)
def _reference(kind, act_dtype):
    """layerwise_inference over the fp32 dequantisation, all nodes and ``nodes=``: computed once, never written"""
    from salient_plusplus_amd.inference import layerwise_inference
    _x8, v, rowptr, col, _y = _data()
    kw = dict(rows_per_slab=SLAB, act_dtype=act_dtype)
    full = layerwise_inference(_model(kind), v, rowptr, col, **kw)
    some = layerwise_inference(_model(kind), v, rowptr, col, nodes=_nodes(), **kw)
    assert bool(torch.isfinite(full).all()) and full.shape == (N, CLASSES)
    return full, some


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("kind", KINDS)
def test_layerwise_inference_from_the_fp8_table_equals_the_fp32_dequantisation(kind, act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference
    x8, _v, rowptr, col, _y = _data()
    full, some = _reference(kind, act_dtype)
    kw = dict(rows_per_slab=SLAB, act_dtype=act_dtype)
    assert _same_bits(layerwise_inference(_model(kind), x8, rowptr, col, **kw), full)
    assert _same_bits(layerwise_inference(_model(kind), x8, rowptr, col, nodes=_nodes(), **kw), some)
    assert _same_bits(some, full[_nodes()])
    if kind in ("sage", "gin"):                                # the models' own method is the same entry
        assert _same_bits(_model(kind).inference(x8, rowptr, col, **kw), full)


@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_from_the_fp8_table_equals_the_fp32_dequantisation(kind, act_dtype):
    from salient_plusplus_amd.inference import evaluate
    x8, v, rowptr, col, y = _data()
    splits = {"valid": _nodes()[:40], "test": _nodes()[40:]}
    for extra in (dict(), dict(splits=splits)):
        kw = dict(rows_per_slab=SLAB, act_dtype=act_dtype, **extra)
        got, want = evaluate(_model(kind), x8, rowptr, col, y, **kw), evaluate(_model(kind), v, rowptr, col, y, **kw)
        assert torch.equal(got.pred, want.pred) and _same_bits(got.nll, want.nll)
        assert (got.labelled, got.correct, got.loss) == (want.labelled, want.correct, want.loss) and want.labelled > 0
        assert got.splits == want.splits and (not extra or set(got.splits) == {"valid", "test"})
        assert got.accuracy == want.accuracy


@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "sageri"])
def test_field_entries_from_the_fp8_table_equal_layerwise_inference(kind, act_dtype):
    from salient_plusplus_amd.inference import evaluate, field_evaluate, field_inference
    x8, v, rowptr, col, y = _data()
    ids = _nodes()[:12]
    kw = dict(rows_per_slab=SLAB, act_dtype=act_dtype)
    assert _same_bits(field_inference(_model(kind), x8, rowptr, col, ids, **kw), _reference(kind, act_dtype)[0][ids])
    got = field_evaluate(_model(kind), x8, rowptr, col, y, nodes=ids, **kw)
    want = evaluate(_model(kind), v, rowptr, col, y, nodes=ids, **kw)
    assert torch.equal(got.pred, want.pred) and _same_bits(got.nll, want.nll)
    assert (got.labelled, got.correct, got.loss) == (want.labelled, want.correct, want.loss)


def test_sageresinception_stays_excluded_from_the_field_entries():
    from salient_plusplus_amd.inference import field_inference
    x8, _v, rowptr, col, _y = _data()
    with pytest.raises(NotImplementedError, match="SAGEResInception"):
        field_inference(_model("sageri"), x8, rowptr, col, _nodes()[:4])
