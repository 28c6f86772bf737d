"""-m gpu: the maximum in exact inference -- graph_aggregate(epilogue="max" / "max_operand") against the training
kernel on the same rows (bit for bit, hubs above the chunk included: a maximum rounds nothing), layerwise_inference of
SAGE(aggr="max") against the model's own forward over full hops (the mean test's tolerance,
test_gpu_layerwise_inference.py:61-68), and the entries that must agree with each other bit for bit."""
import functools

import pytest
import torch

from test_gpu_evaluate import FIN, HID, N, _graph, _labels

pytestmark = pytest.mark.gpu

CLASSES = 7
HUBS = [7, 899, 900, N - 1]                              # degrees 65, 137, 64 and 448 around the chunk of 64
_ID = dict(ids=lambda v: str(v).split(".")[-1])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _table(kind):
    """the graph's features as fp32 / fp16 / bf16 rows, or as an Fp8Table with the fp32 matrix it stands for"""
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import Fp8Table
    x, _rowptr, _col = _graph()
    if kind == "fp8":
        q = fp8.quantize_e4m3(x)
        return Fp8Table(q), q
    return (x.to(kind),) * 2


def _nodes():
    g = torch.Generator().manual_seed(4)
    return torch.cat([torch.randint(0, N, (300,), generator=g), torch.tensor(HUBS + [0, 7, 7, N - 1])]).cuda()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], **_ID)
@pytest.mark.parametrize("kind", [torch.float32, torch.float16, torch.bfloat16, "fp8"], **_ID)
def test_graph_aggregate_max_equals_the_training_kernel(kind, out_dtype):
    from salient_plusplus_amd.inference import graph_agg_chunk, graph_aggregate
    from salient_plusplus_amd.models import _agg_max_forward
    _x, rowptr, col = _graph()
    deg = rowptr[1:] - rowptr[:-1]
    assert graph_agg_chunk() == 64 and int((deg > 64).sum()) == 3 and int((deg == 0).sum()) > 0
    x, rows = _table(kind)
    ids = _nodes()
    for epilogue, concat in (("max", False), ("max_operand", True)):
        want, _ = _agg_max_forward(rowptr, col, N, rows, out_dtype, concat, False)       # the graph as one full hop
        whole = graph_aggregate(x, rowptr, col, row0=0, num_targets=N, epilogue=epilogue, out_dtype=out_dtype)
        assert _same(whole, want)
        assert bool((whole[deg == 0][:, :FIN] == 0).all())                               # empty rows
        slabs = [graph_aggregate(x, rowptr, col, row0=s, num_targets=min(700, N - s), epilogue=epilogue, out_dtype=out_dtype)
                 for s in range(0, N, 700)]
        assert _same(torch.cat(slabs), want)
        assert _same(graph_aggregate(x, rowptr, col, target_ids=ids, epilogue=epilogue, out_dtype=out_dtype), want[ids])


def test_graph_aggregate_max_scalar_form_and_special_values():
    """F = 6 (one column per lane), with a NaN, -inf and signed zeros among a hub's entries"""
    from salient_plusplus_amd.inference import graph_aggregate
    from salient_plusplus_amd.models import _agg_max_forward
    _x, rowptr, col = _graph()
    x = torch.randint(-3, 4, (N, 6), generator=torch.Generator().manual_seed(1)).float()
    x[5, :2], x[6], x[8, 4], x[9, 4] = float("nan"), float("-inf"), -0.0, 0.0
    x = x.cuda()
    for epilogue, concat in (("max", False), ("max_operand", True)):
        want, _ = _agg_max_forward(rowptr, col, N, x, torch.float32, concat, False)
        assert _same(graph_aggregate(x, rowptr, col, row0=0, num_targets=N, epilogue=epilogue), want)
    assert bool(want.isnan().any())


def _model():
    from salient_plusplus_amd.models import SAGE
    torch.manual_seed(31)
    return SAGE(FIN, HID, CLASSES, 3, aggr="max").cuda().eval()


def _forward_over_full_hops(model, x, rowptr, col, act_dtype):
    from salient_plusplus_amd.fast_trainer.samplers import Adj__from_fast_sampler
    e_id = torch.empty(0, dtype=torch.int64, device=x.device)
    adjs = [Adj__from_fast_sampler((rowptr, col, e_id, (N, N))) for _ in range(3)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=act_dtype == torch.bfloat16):
        return model(x, adjs).float()


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], **_ID)
def test_layerwise_inference_matches_the_forward_over_full_hops(act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    model = _model()
    want = _forward_over_full_hops(model, x, rowptr, col, act_dtype)
    got = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)
    assert got.dtype == torch.float32 and got.shape == (N, CLASSES) and bool(torch.isfinite(got).all())
    if act_dtype == torch.bfloat16:                      # test_gpu_layerwise_inference.py:63-66
        rel = float((got - want).norm() / want.norm())
        print(f"max layerwise bf16: relative error {rel:.3e}")
        assert rel < 1e-2, rel
    else:                                                # test_gpu_layerwise_inference.py:67-68
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    # a different model from the mean's: the aggr reached the kernels
    from salient_plusplus_amd.models import SAGE
    mean = SAGE(FIN, HID, CLASSES, 3).cuda().eval()
    mean.load_state_dict(model.state_dict())
    assert not torch.allclose(layerwise_inference(mean, x, rowptr, col, act_dtype=act_dtype), got, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], **_ID)
@pytest.mark.parametrize("kind", [torch.float16, "fp8"], **_ID)
def test_entries_agree_bit_for_bit(kind, act_dtype):
    from salient_plusplus_amd.inference import evaluate, field_evaluate, field_inference, layerwise_inference
    _x, rowptr, col = _graph()
    x, rows = _table(kind)
    model, y, ids = _model(), _labels(CLASSES), _nodes()
    kw = dict(act_dtype=act_dtype)
    lp = layerwise_inference(model, x, rowptr, col, **kw)
    assert torch.equal(layerwise_inference(model, x, rowptr, col, **kw), lp)               # repeated calls
    assert torch.equal(model.inference(x, rowptr, col, **kw), lp)
    if kind == "fp8":                                    # the bits of the same call on the dequantised table
        assert torch.equal(layerwise_inference(model, rows.dequantize(torch.float32), rowptr, col, **kw), lp)
    for rows_per_slab in (700, 64):
        assert torch.equal(layerwise_inference(model, x, rowptr, col, rows_per_slab=rows_per_slab, **kw), lp)
    assert torch.equal(layerwise_inference(model, x, rowptr, col, nodes=ids, **kw), lp[ids])
    assert torch.equal(layerwise_inference(model, x, rowptr, col, nodes=ids, rows_per_slab=97, **kw), lp[ids])
    assert torch.equal(field_inference(model, x, rowptr, col, ids, **kw), lp[ids])
    assert torch.equal(field_inference(model, x, rowptr, col, ids, rows_per_slab=97, **kw), lp[ids])
    ev = evaluate(model, x, rowptr, col, y, **kw)
    assert torch.equal(lp.gather(1, ev.pred.view(-1, 1)).squeeze(1), lp.max(1).values)
    for got in (evaluate(model, x, rowptr, col, y, rows_per_slab=700, **kw),):
        assert torch.equal(got.pred, ev.pred) and _same(got.nll, ev.nll)
    for got in (evaluate(model, x, rowptr, col, y, nodes=ids, **kw), field_evaluate(model, x, rowptr, col, y, nodes=ids, **kw)):
        assert torch.equal(got.pred, ev.pred[ids]) and _same(got.nll, ev.nll[ids])
        assert got.correct == int(((got.pred == y[ids]) & (y[ids] >= 0)).sum())
