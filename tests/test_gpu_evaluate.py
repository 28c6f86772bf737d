"""-m gpu: inference.evaluate / partitioned_evaluate against inference.layerwise_inference on the same arguments.

evaluate makes layerwise_inference's pass and ends it in classify_rows, so with lp = layerwise_inference(...):
  * lp[i, pred[i]] == lp[i].max() on EVERY row, exactly: log_softmax is monotone in the logit, so the argmax of the
    logits attains the maximum log-probability;
  * |nll[i] + lp[i, y[i]]| <= 2 * (C + 8) * 2^-24 * (1 + (lp[i].max() - lp[i, y[i]]) + log C): the first half is
    classify_rows' own bound, the second fp32 log_softmax's rounding, which is the same arithmetic
    (fp32 differences, exponentials, a sum of C terms, a logarithm) in another order, so the same expression bounds it;
    z_y - m is read off lp, where it is lp[i, y] - lp[i].max() up to one rounding;
  * the counts and the loss are those computed from pred, nll and y.
A node's pred and nll are the same bits whatever rows_per_slab is, whether nodes= selected it, and whether the table
is resident or partitioned (LocalPeers, ranks as threads, P in {2, 3}).  No [rows, classes] matrix: at N = 2^19 and 172
classes the peak of evaluate stays below the size of that matrix."""
import functools
import math
import os
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, FIN, HID = 3000, 16, 32
KINDS = ["sage", "gin", "gat1", "gat4", "sageri"]
DTYPES = [torch.float32, torch.bfloat16]
OFFSETS = {2: [0, 1700, N], 3: [0, 900, 901, N]}               # (P = 3: rank 1 owns ONE node)
_ID = dict(ids=lambda v: str(v).split(".")[-1])


@functools.lru_cache(maxsize=None)
def _graph():
    """3 000 nodes, degrees 0..12 (231 empty rows or so) and four hubs above the aggregation chunk of 64"""
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 13, (N,), generator=g)
    deg[7], deg[899], deg[900], deg[N - 1] = 65, 2 * 64 + 9, 64, 7 * 64
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    x = torch.randn((N, FIN), generator=g).to(torch.float16)
    return x.cuda(), rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _labels(classes):
    """one label per node, 20 % of them -1 (unlabelled)"""
    g = torch.Generator().manual_seed(classes)
    y = torch.randint(0, classes, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.2] = -1
    return y.cuda()


@functools.lru_cache(maxsize=None)
def _model(kind, classes):
    from salient_plusplus_amd.models import GAT, GIN, SAGE, SAGEResInception
    torch.manual_seed(31)
    m = {"sage": lambda: SAGE(FIN, HID, classes, 3), "gin": lambda: GIN(FIN, HID, classes, 2),
         "gat1": lambda: GAT(FIN, HID, classes, 2, heads=1), "gat4": lambda: GAT(FIN, HID, classes, 2, heads=4),
         "sageri": lambda: SAGEResInception(FIN, HID, classes, 2)}[kind]()
    g = torch.Generator().manual_seed(8)
    for mod in m.modules():                                    # non-trivial running statistics and affine terms
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.5)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.0 + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _full(kind, classes, act_dtype):
    """(evaluate, layerwise_inference) over the whole graph, once per model, width and activation type"""
    from salient_plusplus_amd.inference import evaluate, layerwise_inference
    x, rowptr, col = _graph()
    model = _model(kind, classes)
    ev = evaluate(model, x, rowptr, col, _labels(classes), act_dtype=act_dtype)
    return ev, layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a.pred, b.pred) and torch.equal(_bits(a.nll), _bits(b.nll))


@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("classes", [7, 47])
@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_against_the_log_probabilities(kind, classes, act_dtype):
    from salient_plusplus_amd.inference import Evaluation
    ev, lp = _full(kind, classes, act_dtype)
    y = _labels(classes)
    assert isinstance(ev, Evaluation) and ev.pred.shape == (N,) and ev.pred.dtype == torch.int64
    assert ev.nll.shape == (N,) and ev.nll.dtype == torch.float32 and lp.shape == (N, classes)
    # the argmax of the logits attains the maximum log-probability: every row, exactly
    assert torch.equal(lp.gather(1, ev.pred.view(-1, 1)).squeeze(1), lp.max(1).values)
    lab = y >= 0
    lpy = lp.double().gather(1, y.clamp(min=0).view(-1, 1)).squeeze(1)
    gap = lp.double().max(1).values - lpy
    bound = 2 * (classes + 8) * 2.0 ** -24 * (1.0 + gap + math.log(classes))
    err = (ev.nll.double() + lpy).abs()
    print(f"{kind} C={classes} {act_dtype}: max |nll + lp[y]| / bound = {(err / bound)[lab].max().item():.3f}")
    assert bool((err[lab] <= bound[lab]).all())
    assert bool((ev.nll[~lab] == 0).all())
    # the counts and the loss, from pred, nll and y
    assert isinstance(ev.labelled, int) and isinstance(ev.correct, int) and isinstance(ev.loss, float)
    assert ev.labelled == int(lab.sum()) and ev.correct == int(((ev.pred == y) & lab).sum())
    want = ev.nll[lab].double().mean().item()
    assert abs(ev.loss - want) <= 1e-13 * abs(want)            # (float64 sums of 3 000 terms in two orders)
    assert ev.accuracy == ev.correct / ev.labelled and ev.splits == {}


@pytest.mark.parametrize("act_dtype", DTYPES, **_ID)
@pytest.mark.parametrize("classes", [7, 47])
@pytest.mark.parametrize("kind", KINDS)
def test_slab_size_and_nodes_change_no_bit(kind, classes, act_dtype):
    from salient_plusplus_amd.inference import evaluate
    x, rowptr, col = _graph()
    model, y = _model(kind, classes), _labels(classes)
    ev, _lp = _full(kind, classes, act_dtype)
    for rows_per_slab in (700, 1):
        got = evaluate(model, x, rowptr, col, y, rows_per_slab=rows_per_slab, act_dtype=act_dtype)
        assert _same(got, ev), (kind, rows_per_slab)
        assert (got.labelled, got.correct, got.loss) == (ev.labelled, ev.correct, ev.loss)
    g = torch.Generator().manual_seed(2)
    nodes = torch.cat([torch.randint(0, N, (400,), generator=g), torch.tensor([N - 1, 0, 7, 7, N - 1, 899])])
    for rows_per_slab in (1 << 20, 97):
        got = evaluate(model, x, rowptr, col, y, nodes=nodes, rows_per_slab=rows_per_slab, act_dtype=act_dtype)
        ids = nodes.cuda()
        assert torch.equal(got.pred, ev.pred[ids]) and torch.equal(_bits(got.nll), _bits(ev.nll[ids]))
        lab = y[ids] >= 0
        assert got.labelled == int(lab.sum()) and got.correct == int(((got.pred == y[ids]) & lab).sum())
    only = evaluate(model, x, rowptr, col, nodes=nodes, act_dtype=act_dtype)        # no labels: pred alone
    assert torch.equal(only.pred, ev.pred[nodes.cuda()])
    assert only.nll is None and only.labelled is None and only.correct is None and only.loss is None


@pytest.mark.parametrize("kind", KINDS)
def test_splits_equal_separate_calls(kind):
    from salient_plusplus_amd.inference import evaluate
    x, rowptr, col = _graph()
    classes = 47
    model, y = _model(kind, classes), _labels(classes)
    g = torch.Generator().manual_seed(4)
    perm = torch.randperm(N, generator=g)
    splits = {"valid": perm[:300], "test": perm[300:1000].cuda(), "none": perm[:0]}
    splits["valid"] = splits["valid"].cuda()
    splits["none"] = splits["none"].cuda()
    ev = evaluate(model, x, rowptr, col, y, splits=splits, rows_per_slab=256)
    cat = evaluate(model, x, rowptr, col, y, nodes=torch.cat(list(splits.values())), rows_per_slab=256)
    assert _same(ev, cat) and (ev.labelled, ev.correct, ev.loss) == (cat.labelled, cat.correct, cat.loss)
    assert list(ev.splits) == ["valid", "test", "none"]
    for name in ("valid", "test"):
        one = evaluate(model, x, rowptr, col, y, nodes=splits[name], rows_per_slab=256)
        rec = ev.splits[name]
        assert (rec["labelled"], rec["correct"]) == (one.labelled, one.correct) and rec["labelled"] > 0
        assert abs(rec["loss"] - one.loss) <= 1e-13 * abs(one.loss)
    assert ev.splits["none"]["labelled"] == 0 and math.isnan(ev.splits["none"]["loss"])
    assert ev.labelled == ev.splits["valid"]["labelled"] + ev.splits["test"]["labelled"]


def _partition(x, lo, hi):
    """rows [lo, hi) of x as a rank holds them: an allocation of its own, rows padded by the resident tables' rule"""
    from salient_plusplus_amd import fast_sampler as fs
    se = fs._row_stride_elems(x.size(1), x.element_size())
    part = torch.empty((hi - lo, se), dtype=x.dtype, device=x.device)[:, :x.size(1)]
    part.copy_(x[lo:hi])
    return part


def _run_threads(P, fn):
    """fn(rank) on P threads; the first exception of any rank is raised here"""
    errors, out = [], [None] * P

    def run(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            import traceback
            errors.append(f"rank {r}: {e}\n{traceback.format_exc()}")

    ts = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), "rank(s) hung"
    assert not errors, "\n".join(errors)
    return out


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind", ["sage", "gin", "gat4", "sageri"])
def test_ranks_as_threads_equal_the_resident_evaluation(kind, P):
    from salient_plusplus_amd.inference import LocalPeers, partitioned_evaluate
    x, rowptr, col = _graph()
    classes, act_dtype = 7, torch.float32
    model, y = _model(kind, classes), _labels(classes)
    ev, _lp = _full(kind, classes, act_dtype)
    off = OFFSETS[P]
    parts = [_partition(x, off[r], off[r + 1]) for r in range(P)]
    labels = [y[off[r]:off[r + 1]].contiguous() for r in range(P)]
    peers = LocalPeers(P, timeout=60.0)
    got = _run_threads(P, lambda r: partitioned_evaluate(model, parts[r], rowptr, col, labels[r], part_offsets=off, rank=r,
                                                         peers=peers, rows_per_slab=500, act_dtype=act_dtype))
    assert torch.equal(torch.cat([g.pred for g in got]), ev.pred)
    assert torch.equal(_bits(torch.cat([g.nll for g in got])), _bits(ev.nll))
    assert sum(g.labelled for g in got) == ev.labelled and sum(g.correct for g in got) == ev.correct
    total = sum(g.loss * g.labelled for g in got if g.labelled) / ev.labelled
    assert abs(total - ev.loss) <= 1e-12 * abs(ev.loss)
    # nodes= inside every rank's range, global ids, unsorted with duplicates
    peers = LocalPeers(P, timeout=60.0)

    def nodes_of(r):
        g = torch.Generator().manual_seed(40 + r)
        lo, hi = off[r], off[r + 1]
        return torch.cat([torch.randint(lo, hi, (min(50, hi - lo),), generator=g), torch.tensor([hi - 1, lo, hi - 1])])

    got = _run_threads(P, lambda r: partitioned_evaluate(model, parts[r], rowptr, col, labels[r], part_offsets=off, rank=r,
                                                         peers=peers, nodes=nodes_of(r), act_dtype=act_dtype))
    for r in range(P):
        ids = nodes_of(r).cuda()
        assert torch.equal(got[r].pred, ev.pred[ids]) and torch.equal(_bits(got[r].nll), _bits(ev.nll[ids]))
        lab = y[ids] >= 0
        assert got[r].labelled == int(lab.sum()) and got[r].correct == int(((got[r].pred == y[ids]) & lab).sum())


def test_no_rows_by_classes_matrix_is_held():
    """N = 2^19 nodes and 172 classes: the [N, 172] fp32 matrix (eight GEMM tiles of logits) is 361 MB, and evaluate's
    peak above what is allocated before the call stays below it; layerwise_inference, which returns it, goes above"""
    from salient_plusplus_amd.inference import evaluate, layerwise_inference
    from salient_plusplus_amd.models import SAGE
    n, classes = 1 << 19, 172
    g = torch.Generator().manual_seed(6)
    deg = torch.randint(0, 9, (n,), generator=g)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=g).cuda()
    rowptr = rowptr.cuda()
    x = torch.randn((n, FIN), generator=g).cuda()
    y = torch.randint(0, classes, (n,), generator=g).cuda()
    torch.manual_seed(1)
    model = SAGE(FIN, HID, classes, 2).cuda()
    matrix = n * classes * 4

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    ev, used = peak(lambda: evaluate(model, x, rowptr, col, y, rows_per_slab=1 << 16))
    print(f"evaluate: peak {used / 1e6:.1f} MB above the baseline; the matrix is {matrix / 1e6:.1f} MB")
    assert used < matrix
    lp, used_lp = peak(lambda: layerwise_inference(model, x, rowptr, col, rows_per_slab=1 << 16))
    print(f"layerwise_inference: peak {used_lp / 1e6:.1f} MB above the baseline")
    assert used_lp > matrix
    assert torch.equal(lp.gather(1, ev.pred.view(-1, 1)).squeeze(1), lp.max(1).values)
    assert ev.labelled == n and ev.correct == int((ev.pred == y).sum())
    assert model.training                                       # the mode the model came in


def test_the_training_flag_is_restored():
    from salient_plusplus_amd.inference import evaluate
    x, rowptr, col = _graph()
    for kind in KINDS:
        model = _model(kind, 7)
        for mode in (True, False):
            model.train(mode)
            evaluate(model, x, rowptr, col, _labels(7), nodes=torch.tensor([3, 1]))
            assert model.training == mode
        assert all(p.grad is None for p in model.parameters())
