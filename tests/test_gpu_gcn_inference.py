"""-m gpu: exact layer-wise GCN through inference.layerwise_inference and inference.evaluate (spp.h f3s), on a graph with
every row shape of the weighted kernel pair: the bits do not depend on rows_per_slab or on nodes=, evaluate returns the
argmax, the NLL and the split counts of those log-probabilities, the accuracy against a float64 dense restatement is
measured next to the training forward's over the whole graph as each hop, and bf16 activations stay inside a bound
propagated through the layers in float64."""
import functools
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FIN, HID, CLASSES, LAYERS = 24, 32, 5, 3
CASES = [(False, False), (False, True), (True, False), (True, True)]         # (normalize, with edge_weight)
_IDS = [f"{'norm' if n else 'plain'}-{'weights' if w else 'ones'}" for n, w in CASES]


@functools.lru_cache(maxsize=None)
def _graph():
    """~400 nodes: degrees 0, 1, 2, C-1, C, C+1, 2C, 3C+5, a hub of 20C+3, self-loops and repeated neighbours side by
    side; (x fp16, rowptr, col, edge weights) on the CPU"""
    from salient_plusplus_amd.inference import graph_agg_chunk
    Cc = graph_agg_chunk()
    g = torch.Generator().manual_seed(23)
    N = 401
    deg = torch.randint(3, 16, (N,), generator=g)
    special = {0: 0, 5: 1, 9: 2, 17: Cc - 1, 33: Cc, 64: Cc + 1, 130: 2 * Cc, 131: 3 * Cc + 5, 200: 20 * Cc + 3, 259: 0,
               260: Cc + 1, N - 1: 2 * Cc + 1}
    for k, v in special.items():
        deg[k] = v
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    for t in (5, 9, 17, 64, 131, 200, 300):
        col[rowptr[t]] = t
    for t in (9, 33, 130, 200, 301):
        col[rowptr[t + 1] - 1] = col[rowptr[t + 1] - 2]
    x = (torch.randn((N, FIN), generator=g) * 0.5).to(torch.float16)
    w = torch.rand(col.numel(), generator=g) * 0.5 + 0.05
    return x, rowptr, col, w


@functools.lru_cache(maxsize=None)
def _dev():
    return tuple(t.cuda() for t in _graph())


@functools.lru_cache(maxsize=None)
def _model(normalize):
    from salient_plusplus_amd.models import GCN
    torch.manual_seed(41)
    m = GCN(FIN, HID, CLASSES, LAYERS, normalize=normalize)
    g = torch.Generator().manual_seed(8)
    for bn in m.bns:                                           # non-trivial running statistics and affine terms
        bn.running_mean.copy_(torch.randn(HID, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(HID, generator=g) * 2.0 + 0.5)
        bn.weight.data.copy_(torch.rand(HID, generator=g) + 0.5)
        bn.bias.data.copy_(torch.randn(HID, generator=g) * 0.1)
    return m.cuda().eval()


def _labels():
    g = torch.Generator().manual_seed(3)
    N = _graph()[0].size(0)
    y = torch.randint(0, CLASSES, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.2] = -1
    return y.cuda()


def _run(normalize, weighted, **kw):
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col, w = _dev()
    return layerwise_inference(_model(normalize), x, rowptr, col, edge_weight=w if weighted else None, **kw)


@functools.lru_cache(maxsize=None)
def _full(normalize, weighted, act_dtype=torch.float32):
    return _run(normalize, weighted, act_dtype=act_dtype)


@functools.lru_cache(maxsize=None)
def _dense64(normalize, weighted):
    """the propagation matrix in float64 on the CPU: A's values (ones without weights), or PyG's gcn_norm of the whole
    graph with fill 1 -- D^-1/2 (A + I) D^-1/2, deg = the row sum of A + I"""
    _x, rowptr, col, w = _graph()
    N = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
    vals = w.double() if weighted else torch.ones(col.numel(), dtype=torch.float64)
    A = torch.zeros((N, N), dtype=torch.float64).index_put_((rows, col), vals, accumulate=True)
    if not normalize:
        return A
    A = A + torch.eye(N, dtype=torch.float64)
    dinv = A.sum(1).pow(-0.5)
    dinv[dinv == float("inf")] = 0
    return dinv.unsqueeze(1) * A * dinv.unsqueeze(0)


def _bn_affine(bn):
    s = bn.weight.double().cpu() / (bn.running_var.double().cpu() + bn.eps).sqrt()
    return s, bn.bias.double().cpu() - bn.running_mean.double().cpu() * s


@torch.no_grad()
def _reference64(normalize, weighted, eps=None):
    """the model in float64 on the CPU, as tests/test_agg_weighted_host.py restates GCN.forward: (log-probabilities, and
    with ``eps`` a bound on the error of log-probabilities computed with one rounding of relative size ``eps`` at each of
    a layer's steps)"""
    x = _graph()[0]
    M = _dense64(normalize, weighted)
    model = _model(normalize)
    h = x.double()
    E = torch.zeros_like(h)                                    # elementwise bound on the error of h
    for i, conv in enumerate(model.convs):
        W = conv.lin.weight.double().cpu()
        a = M @ h
        if eps is not None:                                    # the aggregate: the error coming in, and its own rounding
            Ea = M.abs() @ E
            Ea = Ea + eps * (M.abs() @ h.abs() + Ea)
        z = a @ W.t()
        if eps is not None:                                    # the product: rounded weights, then the rounded result
            Ez = Ea @ W.abs().t()
            Ez = Ez + (2 * eps + eps * eps) * ((a.abs() + Ea) @ W.abs().t())
        if i == LAYERS - 1:
            lp = torch.log_softmax(z, dim=-1)
            # log_softmax moves by at most twice the largest change of a row's logits
            return (lp, 2 * Ez.max(1, keepdim=True).values.expand_as(lp)) if eps is not None else lp
        s, t = _bn_affine(model.bns[i])
        h = z * s + t
        if eps is not None:                                    # BatchNorm's affine map, rounded; relu is 1-Lipschitz
            E = Ez * s.abs()
            E = E + eps * (z.abs() * s.abs() + t.abs() + E)
        h = h.relu()


@pytest.mark.parametrize("normalize,weighted", CASES, ids=_IDS)
def test_bits_do_not_depend_on_the_slab_or_on_nodes(normalize, weighted):
    full = _full(normalize, weighted)
    N = _graph()[0].size(0)
    assert full.shape == (N, CLASSES) and full.dtype == torch.float32 and bool(torch.isfinite(full).all())
    assert bool(((full.exp().sum(1) - 1).abs() < 1e-4).all())
    for rows in (130, 7):
        assert torch.equal(_run(normalize, weighted, rows_per_slab=rows), full), rows
    g = torch.Generator().manual_seed(5)
    nodes = torch.cat([torch.randperm(N, generator=g)[:150], torch.tensor([200, 200, 0, 131, 259])])
    for rows in (1 << 20, 7):
        assert torch.equal(_run(normalize, weighted, nodes=nodes.cuda(), rows_per_slab=rows), full[nodes.cuda()]), rows
    model = _model(normalize)
    model.train()
    try:                                                       # the training flag is restored
        assert torch.equal(_run(normalize, weighted), full) and model.training
    finally:
        model.eval()
    assert torch.equal(_run(normalize, weighted), full) and not model.training


@pytest.mark.parametrize("normalize,weighted", CASES, ids=_IDS)
def test_evaluate_is_the_argmax_and_nll_of_those_log_probabilities(normalize, weighted):
    from salient_plusplus_amd.inference import evaluate
    x, rowptr, col, w = _dev()
    ew = w if weighted else None
    model, y = _model(normalize), _labels()
    lp = _full(normalize, weighted)
    N = lp.size(0)
    ev = evaluate(model, x, rowptr, col, y, edge_weight=ew)
    assert ev.pred.shape == (N,) and ev.nll.shape == (N,) and ev.nll.dtype == torch.float32
    assert torch.equal(lp.gather(1, ev.pred.view(-1, 1)).squeeze(1), lp.max(1).values)
    lab = y >= 0
    lpy = lp.double().gather(1, y.clamp(min=0).view(-1, 1)).squeeze(1)
    gap = lp.double().max(1).values - lpy
    # classify_rows' bound and fp32 log_softmax's, the same expression (tests/test_gpu_evaluate.py)
    bound = 2 * (CLASSES + 8) * 2.0 ** -24 * (1.0 + gap + math.log(CLASSES))
    err = (ev.nll.double() + lpy).abs()
    print(f"normalize={normalize} weights={weighted}: max |nll + lp[y]| / bound = {(err / bound)[lab].max().item():.3f}")
    assert bool((err[lab] <= bound[lab]).all()) and bool((ev.nll[~lab] == 0).all())
    assert ev.labelled == int(lab.sum()) and ev.correct == int(((ev.pred == y) & lab).sum())
    assert abs(ev.loss - ev.nll[lab].double().mean().item()) <= 1e-13 * abs(ev.loss)
    g = torch.Generator().manual_seed(6)
    perm = torch.randperm(N, generator=g).cuda()
    splits = {"valid": perm[:90], "test": torch.cat([perm[90:200], perm[:3]])}
    got = evaluate(model, x, rowptr, col, y, splits=splits, rows_per_slab=7, edge_weight=ew)
    ids = torch.cat(list(splits.values()))
    assert torch.equal(got.pred, ev.pred[ids]) and torch.equal(got.nll.view(torch.int32), ev.nll[ids].view(torch.int32))
    for name, sel in splits.items():
        rec, l = got.splits[name], lab[sel]
        assert rec["labelled"] == int(l.sum()) and rec["correct"] == int(((ev.pred[sel] == y[sel]) & l).sum())
        want = ev.nll[sel][l].double().mean().item()
        assert abs(rec["loss"] - want) <= 1e-13 * abs(want)
    assert got.labelled == sum(r["labelled"] for r in got.splits.values())
    assert not model.training


@pytest.mark.parametrize("normalize,weighted", CASES, ids=_IDS)
def test_accuracy_next_to_the_training_forward(normalize, weighted):
    """e_inf, the largest error of layerwise_inference against the float64 dense restatement, is held against e_fwd, the
    largest error of the existing training forward run with the whole graph as each of its hops: e_inf <= 4 * e_fwd +
    2^-20.  The factor covers the other summation order on long rows and the fixed GEMM tiles; neither changes the
    operation count."""
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    x, rowptr, col, w = _dev()
    N = x.size(0)
    want = _reference64(normalize, weighted)
    model = _model(normalize)
    adj_t = SparseTensor(rowptr=rowptr, row=None, col=col, value=w if weighted else None, sparse_sizes=(N, N),
                         is_sorted=True, trust_data=True)
    with torch.no_grad():
        fwd = model.eval()(x, [(adj_t, None, (N, N))] * LAYERS)
    e_fwd = float((fwd.double().cpu() - want).abs().max())
    e_inf = float((_full(normalize, weighted).double().cpu() - want).abs().max())
    print(f"normalize={normalize} weights={weighted}: e_inf = {e_inf:.3e}, e_fwd = {e_fwd:.3e}, "
          f"ratio = {e_inf / max(e_fwd, 1e-300):.3f}")
    assert e_inf <= 4 * e_fwd + 2.0 ** -20


@pytest.mark.parametrize("normalize,weighted", CASES, ids=_IDS)
def test_bf16_activations_stay_inside_the_propagated_bound(normalize, weighted):
    """act_dtype=bf16 rounds, per layer, the aggregate, the weights, the product and BatchNorm's output to bf16, whose
    unit roundoff is 2^-8 (8 significand bits, round to nearest even).  The bound charges each of those steps
    eps = 2^-8 + 2^-16 -- the second term for the fp32 sums inside the step -- RELATIVE TO THE STEP'S MAGNITUDE SUM
    (|M| (|h| + E) for the aggregate, (|a| + E_a) |W|^T for the product, weights and result: a rounding is relative to
    the computed result, which the magnitude sum dominates), carries the incoming error through |M|, |W| and BatchNorm's
    scale, and ends in log_softmax, which moves by at most twice the largest change of a row's logits:
    _reference64(eps), float64 on the CPU.  The fp32 result's own error gets the same treatment with eps = 2^-16 (fp32
    chains of at most a few hundred roundings of 2^-24 each), so |bf16 - fp32| <= B(2^-8 + 2^-16) + B(2^-16), row by
    row."""
    lp16 = _full(normalize, weighted, torch.bfloat16)
    lp32 = _full(normalize, weighted)
    assert lp16.dtype == torch.float32 and lp16.shape == lp32.shape and bool(torch.isfinite(lp16).all())
    _lp, b16 = _reference64(normalize, weighted, eps=2.0 ** -8 + 2.0 ** -16)
    _lp, b32 = _reference64(normalize, weighted, eps=2.0 ** -16)
    err = (lp16.double() - lp32.double()).abs().cpu()
    bound = b16 + b32
    print(f"normalize={normalize} weights={weighted}: max |bf16 - fp32| = {float(err.max()):.3e}, "
          f"max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    for rows in (130, 7):                                      # and the bf16 bits do not depend on the slab either
        assert torch.equal(_run(normalize, weighted, act_dtype=torch.bfloat16, rows_per_slab=rows), lp16)


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("normalize,weighted", CASES, ids=_IDS)
def test_the_model_method_is_the_function(normalize, weighted, act_dtype):
    """``GCN.inference`` is ``layerwise_inference``: the same bits, ``edge_weight`` handed on, for every node and ``nodes=``"""
    from inference_method import assert_method_equals_function
    x, rowptr, col, w = _dev()
    N = x.size(0)
    g = torch.Generator().manual_seed(5)
    nodes = torch.cat([torch.randperm(N, generator=g)[:150], torch.tensor([200, 200, 0, 131, 259])]).cuda()
    kw = dict(edge_weight=w) if weighted else {}
    sub = assert_method_equals_function(_model(normalize), x, rowptr, col, nodes, act_dtype, **kw)
    assert sub.shape == (nodes.numel(), CLASSES) and torch.equal(sub, _full(normalize, weighted, act_dtype)[nodes])
