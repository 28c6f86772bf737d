"""-m gpu: spp_graph_agg_stats_forward (csrc/graph_agg_stats.hip, spp.h f4e) through inference.graph_stats_aggregate, and
layerwise_inference / evaluate of a PNA model on top of it, on test_gpu_evaluate's 3 000-node graph: degrees 0..12 with
empty rows and hubs of 65, 137, 64 and 448 entries around the chunk of 64.

The values and bounds are test_gpu_agg_stats.expected's (its docstring derives them), in float64 with each row's d and K
over this graph as one hop: (d + 2) u (|K| + A) for the mean and its var -> std formula; min and max exact (with add: the
fp32 rounding of the float64 sum); 4u relative on top for the non-identity scalers.  They cover the chunked order of a long
row as they stand: every chunk is shifted by the ROW's K, so the addends are the row's own, and none passes through more
than d additions.  The 1000 + noise column runs on the same bounds: with unshifted sums, or a wrong chunk combine, its
variance is off by about u 10^6 d at the hubs.  The printed lines are a record, no bound's input."""
import copy
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_f64 as A  # noqa: E402
import test_gpu_agg_stats as S  # noqa: E402
from test_gpu_evaluate import FIN, HID, N, _graph  # noqa: E402

pytestmark = pytest.mark.gpu
_bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@functools.lru_cache(maxsize=None)
def hop():
    """the graph as one full hop on the CPU; three rows above the chunk and an empty one, from the degrees set in _graph()"""
    _, rowptr, col = _graph()
    h = A.Hop(rowptr.cpu(), col.cpu(), N, N)
    assert int((h.deg > 64).sum()) == 3 and int((h.deg == 0).sum()) >= 1
    return h


@functools.lru_cache(maxsize=None)
def rows(F, dtype=torch.float32):
    """(x [N, F] in dtype, add [N, F] fp32), on the CPU"""
    g = torch.Generator().manual_seed(F)
    x = torch.randn((N, F), generator=g)
    x[:, 3::4] = (2 * x[:, 3::4]).round() / 2
    x[:, 1] = 0.75
    x[:, 2] = 1000 + 1e-2 * x[:, 2]
    return x.to(dtype), torch.randn((N, F), generator=g)


@pytest.mark.parametrize("scalers", S.SCALERS, ids=["identity", "three_scalers"])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda v: str(v).split(".")[-1])
@pytest.mark.parametrize("F", [4, 128, 260])
def test_kernel_pair_against_float64(F, dtype, with_add, scalers, monkeypatch):
    from salient_plusplus_amd.inference import graph_stats_aggregate
    h = hop()
    monkeypatch.setattr(S, "hop", hop)                   # expected()'s formulas over THIS graph
    x, add = rows(F, dtype)[0], rows(F, dtype)[1] if with_add else None
    ref, bound, *_ = S.expected(x, add, torch.zeros((N, len(scalers) * 4 * F)), scalers)
    out = graph_stats_aggregate(x.cuda(), h.rowptr.cuda(), h.col.cuda(), add=add.cuda() if with_add else None,
                                scalers=scalers, delta=S.DELTA, eps=S.EPS, row0=0, num_targets=N)
    bad = []
    for i, name in enumerate(f"{s}.{a}" for s in scalers for a in ("mean", "min", "max", "std")):
        cols = slice(i * F, (i + 1) * F)                                   # identity.min / identity.max: bound 0, bit-exact
        ratio, where = A.worst(out[:, cols], ref[:, cols], bound[:, cols], h)
        print(f"GRAPH_STATS_RATIO {name}: {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append(f"{name}: err/bound {ratio:.3f} at {where}")
    assert not bool(out[(h.deg == 0).cuda()].any()), "the empty rows"
    assert not bad, bad


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=lambda v: str(v).split(".")[-1])
def test_one_result_per_row(out_dtype):
    from salient_plusplus_amd import models
    from salient_plusplus_amd.inference import graph_stats_aggregate
    h, F = hop(), 128
    x, add = (t.cuda() for t in rows(F))
    rp, cl = h.rowptr.cuda(), h.col.cuda()
    call = functools.partial(graph_stats_aggregate, x, rp, cl, scalers=S.SCALERS[1], delta=S.DELTA, eps=S.EPS, out_dtype=out_dtype)
    whole = call(add=add, row0=0, num_targets=N)
    assert torch.equal(_bits(whole), _bits(call(add=add, row0=0, num_targets=N))), "two runs, two results"
    slabs = torch.cat([call(add=add[s:s + 700], row0=s, num_targets=min(700, N - s)) for s in range(0, N, 700)])
    assert torch.equal(_bits(whole), _bits(slabs)), "the slabs of 700 rows"
    ids = torch.cat([torch.randint(0, N, (500,), generator=torch.Generator().manual_seed(3)),
                     torch.tensor([7, 899, 900, N - 1, 7, N - 1])]).cuda()
    assert torch.equal(_bits(whole[ids]), _bits(call(add=add[ids].contiguous(), target_ids=ids))), "target_ids"
    if out_dtype == torch.float32:                       # the min and max blocks: the training kernel's bits, any row length
        hopwise = models.stats_aggregate(x, rp, cl, N, add=add, scalers=S.SCALERS[1], delta=S.DELTA, eps=S.EPS)
        blocks = lambda t: t.view(N, 3, 4, F)[:, :, 1:3].contiguous()
        assert torch.equal(_bits(blocks(whole)), _bits(blocks(hopwise)))
        short = (h.deg <= 64).cuda()                     # (a record for DESIGN, not a condition: the epilogue's contraction)
        print("GRAPH_STATS_BITS rows d <= 64 are the training kernel's bits:", torch.equal(_bits(whole[short]), _bits(hopwise[short])))


def full_hops(model, x):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    _, rowptr, col = _graph()
    with torch.no_grad():
        return model(x, [(SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N)), None, (N, N))] * 3)


@functools.lru_cache(maxsize=None)
def pna():
    """(model, ids, float64 forward over three full hops [N, 7], whole-graph fp32 log-probabilities)"""
    from salient_plusplus_amd import models
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    torch.manual_seed(31)
    model = models.PNA(FIN, HID, 7, 3, delta=models.pna_delta(rowptr.cpu()))
    g = torch.Generator().manual_seed(8)
    for bn in model.bns:                                 # non-trivial running statistics, as test_gpu_evaluate._model
        bn.running_mean.copy_(torch.randn(HID, generator=g) * 0.5), bn.running_var.copy_(torch.rand(HID, generator=g) * 2.0 + 0.5)
        bn.weight.data.copy_(torch.rand(HID, generator=g) + 0.5), bn.bias.data.copy_(torch.randn(HID, generator=g) * 0.1)
    model = model.cuda().eval()
    ids = torch.cat([torch.randint(0, N, (300,), generator=g), torch.tensor([7, 899, 900, N - 1, 7])]).cuda()
    return model, ids, full_hops(copy.deepcopy(model).double(), x.double()), layerwise_inference(model, x, rowptr, col)


def test_pna_layerwise_against_float64(monkeypatch):
    """fp32: max|. - ref| / max|ref| to the float64 forward is at most 4x that of the fp32 forward on the plain-torch path
    (test_pna_step_against_float64's rule); bf16: below 1e-2 in relative norm (test_gpu_layerwise_inference.py's figure)"""
    from salient_plusplus_amd import models
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    model, _, ref, lp = pna()
    with monkeypatch.context() as mp:
        mp.setattr(models, "_stats_kernels_read", lambda *a: False)
        torch_path = full_hops(model, x.float())
    dist = lambda t: float((t.double() - ref).abs().max() / ref.abs().max())
    print(f"PNA_INFERENCE fp32: plain-torch forward {dist(torch_path):.3e} layerwise {dist(lp):.3e}")
    assert lp.shape == (N, 7) and lp.dtype == torch.float32 and dist(lp) <= 4 * dist(torch_path)
    lp16 = layerwise_inference(model, x, rowptr, col, act_dtype=torch.bfloat16)
    rel = float((lp16.double() - ref).norm() / ref.norm())
    print(f"PNA_INFERENCE bf16: relative error {rel:.3e}")
    assert rel < 1e-2


def test_pna_rows_do_not_depend_on_the_call():
    from salient_plusplus_amd.inference import evaluate, layerwise_inference
    x, rowptr, col = _graph()
    model, ids, _, lp = pna()
    y = torch.randint(0, 7, (N,), generator=torch.Generator().manual_seed(5)).cuda()
    ev = evaluate(model, x, rowptr, col, y)
    assert torch.equal(lp.gather(1, ev.pred.view(-1, 1)).squeeze(1), lp.max(1).values)
    for slab in (700, 64):
        assert torch.equal(_bits(lp), _bits(layerwise_inference(model, x, rowptr, col, rows_per_slab=slab))), slab
        other = evaluate(model, x, rowptr, col, y, rows_per_slab=slab)
        assert torch.equal(ev.pred, other.pred) and torch.equal(_bits(ev.nll), _bits(other.nll)), slab
    assert torch.equal(_bits(lp[ids]), _bits(layerwise_inference(model, x, rowptr, col, nodes=ids)))
    some = evaluate(model, x, rowptr, col, y, nodes=ids)
    assert torch.equal(ev.pred[ids], some.pred) and torch.equal(_bits(ev.nll[ids]), _bits(some.nll))
