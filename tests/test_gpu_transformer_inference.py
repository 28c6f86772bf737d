"""inference.layerwise_inference / transformer_inference / evaluate over a GraphTransformer model (the driver
``_attn_layers`` with ``_transformer_layer`` on spp_graph_transformer_forward): against the model restated in float64
and against the model's own device forward over L identical full hops, bit for bit against itself (slab sizes,
``nodes=``), ``evaluate``'s predictions and losses against the log-probabilities, and the peak memory against the
recipe's arithmetic.

The accuracy check has no free constant.  fp32: the distance to float64, max|a - ref| / max|ref|, may be at most 4x the
distance of the model's OWN forward (k_transformer_fwd over full hops, one whole GEMM a layer) on the same inputs -- the
project's margin in tests/test_gpu_gatv2_inference.py, for its reason: two fp32 evaluations of one formula in different
orders.  bf16 activations: the relative norm ||a - ref|| / ||ref||, at most 4x that of the own forward under bf16
autocast.  Every ratio is printed (DESIGN section 7 f3z records them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, FIN, HIDDEN, LAYERS = 400, 16, 32, 3
HUB = 17
EMPTY = (3, 250, N - 1)
CASES = [(H, classes, beta, True) for H in (1, 4) for classes in (5, 47) for beta in (False, True)] + [(4, 5, False, False)]


def _name(d):
    return str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _graph():
    """400 nodes of 0..10 entries, one hub row of 2 C_g + 9 (three chunks) with diagonal and repeated entries, three
    rows without entries"""
    from salient_plusplus_amd.inference import graph_transformer_chunk
    Cg = graph_transformer_chunk()
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 11, (N,), generator=g)
    deg[HUB] = 2 * Cg + 9
    deg[list(EMPTY)] = 0
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    b = int(rowptr[HUB])
    col[b + 1], col[b + Cg], col[b + 2 * Cg + 8], col[b + 5] = HUB, HUB, HUB, col[b + 4]
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _features():
    return torch.randn((N, FIN), generator=torch.Generator().manual_seed(6)).cuda()


def _model(H, classes, beta, root=True):
    from salient_plusplus_amd.models import GraphTransformer, TransformerConv
    torch.manual_seed(40 + 10 * H + classes + int(beta))
    model = GraphTransformer(FIN, HIDDEN, classes, LAYERS, heads=H, beta=beta)
    if not root:                                              # the same model rebuilt with root_weight=False
        dims = [FIN] + [HIDDEN] * (LAYERS - 1)
        for i in range(LAYERS):
            last = i == LAYERS - 1
            model.convs[i] = TransformerConv(dims[i], classes if last else HIDDEN // H, heads=H, concat=not last,
                                             root_weight=False)
    return model.cuda()


def _forward_over_full_hops(model, x, rowptr, col, act_dtype):
    """the model's own forward in eval mode: the graph as LAYERS identical full hops"""
    from salient_plusplus_amd.fast_trainer.samplers import Adj__from_fast_sampler
    e_id = torch.empty(0, dtype=torch.int64, device=x.device)
    adjs = [Adj__from_fast_sampler((rowptr, col, e_id, (N, N))) for _ in range(LAYERS)]
    was = model.training
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=act_dtype == torch.bfloat16):
        out = model(x, adjs)
    model.train(was)
    return out.float()


def _model_f64(model, x, rowptr, col):
    """the whole model restated in float64 on the CPU: the three projections with their biases, the formula
    (``_transformer_reference`` on float64 rows), the heads concatenated or averaged, the root term added or gated, ReLU
    between layers, log_softmax"""
    from salient_plusplus_amd.models import _transformer_reference
    rowptr, col, cur = rowptr.cpu(), col.cpu(), x.double().cpu()
    lin = lambda m, t: t @ m.weight.detach().double().cpu().t() + (m.bias.detach().double().cpu() if m.bias is not None else 0)
    for i, conv in enumerate(model.convs):
        H, Cc = conv.heads, conv.out_channels
        q, k, v = (lin(m, cur).view(N, H, Cc) for m in (conv.lin_query, conv.lin_key, conv.lin_value))
        out = _transformer_reference(q, k, v, rowptr, col, 1.0 / float(Cc) ** 0.5)
        out = out.reshape(N, H * Cc) if conv.concat else out.mean(1)
        if conv.lin_skip is not None:
            x_r = lin(conv.lin_skip, cur)
            if conv.lin_beta is not None:
                b = torch.sigmoid(lin(conv.lin_beta, torch.cat([out, x_r, out - x_r], -1)))
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        cur = torch.relu(out) if i < LAYERS - 1 else out
    return torch.log_softmax(cur, dim=-1)


def _distance(a, ref, act_dtype):
    a = a.double().cpu()
    if act_dtype == torch.bfloat16:
        return float((a - ref).norm() / ref.norm())
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("H,classes,beta,root", CASES)
def test_layerwise_inference_against_float64_and_the_own_forward(H, classes, beta, root, act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, beta, root).train()
    got = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)
    assert got.shape == (N, classes) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert model.training and all(p.grad is None for p in model.parameters()) and not got.requires_grad
    assert float((got.exp().sum(dim=1) - 1.0).abs().max()) < 1e-5
    ref = _model_f64(model, x, rowptr, col)
    d_own = _distance(_forward_over_full_hops(model, x, rowptr, col, act_dtype), ref, act_dtype)
    d_got = _distance(got, ref, act_dtype)
    print(f"TRANSFORMER_INFERENCE heads={H} classes={classes} beta={beta} root_weight={root} {_name(act_dtype)}: own forward "
          f"{d_own:.3e} layerwise_inference {d_got:.3e} ratio {d_got / d_own if d_own else float('inf'):.2f}")
    assert d_got <= 4 * d_own, (d_got, d_own)
    model.eval()
    assert torch.equal(layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype), got) and not model.training


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("H,classes,beta,root", [(4, 5, False, True), (1, 47, True, True), (4, 47, True, True),
                                                 (1, 5, False, True), (4, 5, False, False)])
def test_slab_size_nodes_and_the_entry_change_no_bit(H, classes, beta, root, act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference, transformer_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, beta, root).train()
    got = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, HUB, HUB, 0, 3, HUB])])
    for rows in (64, 1 << 20):
        assert torch.equal(layerwise_inference(model, x, rowptr, col, rows_per_slab=rows, act_dtype=act_dtype), got), rows
        sub = layerwise_inference(model, x, rowptr, col, nodes=nodes, rows_per_slab=rows, act_dtype=act_dtype)
        assert sub.shape == (nodes.numel(), classes) and torch.equal(sub, got[nodes.cuda()])
        assert torch.equal(transformer_inference(model, x, rowptr, col, nodes=nodes, rows_per_slab=rows,
                                                 act_dtype=act_dtype), sub)
    assert torch.equal(transformer_inference(model, x, rowptr, col, act_dtype=act_dtype), got) and model.training
    with pytest.raises(ValueError, match="outside the graph"):
        layerwise_inference(model, x, rowptr, col, nodes=torch.tensor([0, N]))


@pytest.mark.parametrize("H,classes,beta", [(4, 5, False), (1, 47, True)])
def test_evaluate_is_the_argmax_and_the_nll_of_the_log_probabilities(H, classes, beta):
    from salient_plusplus_amd.inference import evaluate, layerwise_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, beta).train()
    y = torch.randint(0, classes, (N,), generator=torch.Generator().manual_seed(3)).cuda()
    y[5], y[HUB + 1] = -1, -1
    logp = layerwise_inference(model, x, rowptr, col)
    ev = evaluate(model, x, rowptr, col, y, rows_per_slab=64)
    assert model.training
    labelled = y >= 0
    assert torch.equal(logp.gather(1, ev.pred[:, None]).squeeze(1), logp.max(1).values)      # pred attains the maximum
    want_nll = torch.where(labelled, -logp.gather(1, y.clamp(min=0)[:, None]).squeeze(1), torch.zeros(N, device="cuda"))
    torch.testing.assert_close(ev.nll, want_nll, rtol=1e-5, atol=1e-6)
    assert ev.labelled == int(labelled.sum()) and ev.correct == int((labelled & (ev.pred == y)).sum())
    nodes = torch.tensor([HUB, 0, HUB, 399, 3])
    sub = evaluate(model, x, rowptr, col, y, nodes=nodes)
    assert torch.equal(sub.pred, ev.pred[nodes.cuda()]) and torch.equal(sub.nll, ev.nll[nodes.cuda()])


def test_live_activation_matrices_are_what_the_docstring_counts():
    """``_transformer_layer`` states its memory as arithmetic: FIVE [N, hidden] matrices live at the end of a projection
    (cur, q, [k | v] worth two, skip), four while attending (the skip IS the next matrix).  Four layers at 393 216 nodes
    (six whole GEMM tiles) and hidden 256 in fp32: a matrix is M = 402.7 MB.  On top the projection holds one GEMM
    product at a time, the widest [65 536, 512] of [k | v]: 134 MB = 0.33 M; features, graph and the GEMM library's
    workspace are in the baseline.  So the peak is 5.33 M, one matrix more would be 6.33 M, and the bound live + 0.5 --
    the allowance of tests/test_gpu_gatv2_inference.py -- separates them."""
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import GraphTransformer
    n, hidden = 6 * 65536, 256
    g = torch.Generator().manual_seed(5)
    rowptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int64)
    col = torch.randint(0, n, (3 * n,), generator=g)
    x = torch.randn((n, 16), generator=g).cuda()
    rowptr, col = rowptr.cuda(), col.cuda()
    torch.manual_seed(2)
    model = GraphTransformer(16, hidden, 8, 4, heads=4).cuda()
    layerwise_inference(model, x[:64], rowptr[:65].clone(), col[:192] % 64)      # (warm the GEMM library's workspaces)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = layerwise_inference(model, x, rowptr, col)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    M = n * hidden * 4
    print(f"TRANSFORMER_MEMORY: peak {peak / M:.2f} matrices of {M / 1e6:.1f} MB (counted live: 5)")
    assert out.shape == (n, 8)
    assert peak <= (5 + 0.5) * M, peak / M


def test_shapes_the_kernels_do_not_take_are_refused_with_the_arithmetic():
    from salient_plusplus_amd.inference import evaluate, layerwise_inference, transformer_inference
    from salient_plusplus_amd.models import GraphTransformer
    rowptr, col = _graph()
    x = _features()
    for entry in (layerwise_inference, transformer_inference, evaluate):
        with pytest.raises(NotImplementedError, match=r"heads = 3"):
            entry(GraphTransformer(FIN, 36, 5, 2, heads=3).cuda(), x, rowptr, col)
        with pytest.raises(NotImplementedError, match=r"8 \* 256 = 2048"):
            entry(GraphTransformer(FIN, 32, 172, 2, heads=8).cuda(), x, rowptr, col)
    assert not hasattr(GraphTransformer, "inference")
