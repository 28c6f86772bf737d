"""inference.gatv2_inference / evaluate over a GATv2 model (the driver ``_attn_layers`` with ``_gatv2_layer`` on spp_graph_gatv2_forward):
against the model restated in float64 and against the model's own device forward over L identical full hops, bit for
bit against itself (slab sizes, ``nodes=``), and ``evaluate``'s predictions and losses against the log-probabilities.

The accuracy check has no free constant.  fp32: the distance to float64, max|a - ref| / max|ref|, may be at most 4x the
distance of the model's OWN forward (k_gatv2_fwd over full hops, one whole GEMM a layer) on the same inputs -- f3v's
margin, for f3v's reason: two fp32 evaluations of one formula in different orders.  bf16 activations: the relative norm
||a - ref|| / ||ref|| (the form the GAT inference test uses), at most 4x that of the own forward under bf16 autocast.
Every ratio is printed (DESIGN section 7 f3w records them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, FIN, HIDDEN, LAYERS = 400, 16, 32, 3
HUB = 17
CASES = [(H, classes, share) for H in (1, 4) for classes in (8, 5) for share in (False, True)]


def _name(d):
    return str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _graph():
    """400 nodes of 0..10 entries, one hub row of 2 C_g + 9 (three chunks) with diagonal entries, a node of degree 0"""
    from salient_plusplus_amd.inference import graph_gatv2_chunk
    Cg = graph_gatv2_chunk()
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 11, (N,), generator=g)
    deg[HUB], deg[3] = 2 * Cg + 9, 0
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    b = int(rowptr[HUB])
    col[b + 1], col[b + Cg], col[b + 2 * Cg + 8] = HUB, HUB, HUB
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _features():
    return torch.randn((N, FIN), generator=torch.Generator().manual_seed(6)).cuda()


def _model(H, classes, share):
    from salient_plusplus_amd.models import GATv2
    torch.manual_seed(40 + 10 * H + classes + int(share))
    return GATv2(FIN, HIDDEN, classes, LAYERS, heads=H, share_weights=share).cuda()


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
    """the whole model restated in float64 on the CPU: both projections, the formula (``_gatv2_reference`` on float64
    rows), ReLU between layers, the mean of the last layer's heads, log_softmax"""
    from salient_plusplus_amd.models import _gatv2_reference
    rowptr, col, cur = rowptr.cpu(), col.cpu(), x.double().cpu()
    for i, conv in enumerate(model.convs):
        H, Cc = conv.heads, conv.out_channels
        x_l = (cur @ conv.lin_l.weight.detach().double().cpu().t()).view(N, H, Cc)
        x_r = (cur @ conv.lin_r.weight.detach().double().cpu().t()).view(N, H, Cc)
        out = _gatv2_reference(x_l, x_r, conv.att.detach().double().cpu().view(H, Cc), rowptr, col, conv.negative_slope)
        cur = torch.relu(out.reshape(N, H * Cc)) if i < LAYERS - 1 else out.mean(1)
    return torch.log_softmax(cur, dim=-1)


def _distance(a, ref, act_dtype):
    a = a.double().cpu()
    if act_dtype == torch.bfloat16:
        return float((a - ref).norm() / ref.norm())
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("H,classes,share", CASES)
def test_gatv2_inference_against_float64_and_the_own_forward(H, classes, share, act_dtype):
    from salient_plusplus_amd.inference import gatv2_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, share).train()
    got = gatv2_inference(model, x, rowptr, col, act_dtype=act_dtype)
    assert got.shape == (N, classes) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert model.training and all(p.grad is None for p in model.parameters()) and not got.requires_grad
    assert float((got.exp().sum(dim=1) - 1.0).abs().max()) < 1e-5
    ref = _model_f64(model, x, rowptr, col)
    d_own = _distance(_forward_over_full_hops(model, x, rowptr, col, act_dtype), ref, act_dtype)
    d_got = _distance(got, ref, act_dtype)
    print(f"GATV2_INFERENCE heads={H} classes={classes} share={share} {_name(act_dtype)}: own forward {d_own:.3e} "
          f"gatv2_inference {d_got:.3e} ratio {d_got / d_own if d_own else float('inf'):.2f}")
    assert d_got <= 4 * d_own, (d_got, d_own)
    model.eval()
    assert torch.equal(gatv2_inference(model, x, rowptr, col, act_dtype=act_dtype), got) and not model.training


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("H,classes,share", [(4, 5, False), (1, 8, True), (4, 8, True), (1, 5, False)])
def test_slab_size_and_nodes_change_no_bit(H, classes, share, act_dtype):
    from salient_plusplus_amd.inference import gatv2_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, share)
    got = gatv2_inference(model, x, rowptr, col, act_dtype=act_dtype)
    for rows in (64, 1000, 1 << 20):
        assert torch.equal(gatv2_inference(model, x, rowptr, col, rows_per_slab=rows, act_dtype=act_dtype), got), rows
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, HUB, HUB, 0, 3, HUB])])
    for rows in (64, 1 << 20):
        sub = gatv2_inference(model, x, rowptr, col, nodes=nodes, rows_per_slab=rows, act_dtype=act_dtype)
        assert sub.shape == (nodes.numel(), classes) and torch.equal(sub, got[nodes.cuda()])
    with pytest.raises(ValueError, match="outside the graph"):
        gatv2_inference(model, x, rowptr, col, nodes=torch.tensor([0, N]))


@pytest.mark.parametrize("H,classes,share", [(4, 5, False), (1, 8, True)])
def test_evaluate_is_the_argmax_and_the_nll_of_the_log_probabilities(H, classes, share):
    from salient_plusplus_amd.inference import evaluate, gatv2_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, share).train()
    y = torch.randint(0, classes, (N,), generator=torch.Generator().manual_seed(3)).cuda()
    y[5], y[HUB + 1] = -1, -1
    logp = gatv2_inference(model, x, rowptr, col)
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


@pytest.mark.parametrize("share", [False, True], ids=["two_projections", "share_weights"])
def test_live_activation_matrices_are_what_the_docstring_counts(share):
    """``_gatv2_layer`` states its memory as arithmetic: three [N, hidden] matrices live at the worst moment (cur, x_l,
    x_r while projecting; x_l, x_r, nxt while attending), two with share_weights -- the previous layer's matrix must be
    gone once the projections are complete.  Four layers at 400 000 nodes and hidden 256 in fp32: a matrix is
    M = 409.6 MB.  On top the projection holds two GEMM tiles of 65 536 rows (the zero-padded last tile and a product,
    67 MB each: 0.33 M together); features, graph and the GEMM library's workspace are in the baseline.  So the peak is
    3.33 M (2.33 M), and one matrix more would be 4 M (3 M): the bound live + 0.5 separates them."""
    from salient_plusplus_amd.inference import gatv2_inference
    from salient_plusplus_amd.models import GATv2
    n, hidden = 400_000, 256
    g = torch.Generator().manual_seed(5)
    rowptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int64)
    col = torch.randint(0, n, (3 * n,), generator=g)
    x = torch.randn((n, 16), generator=g).cuda()
    rowptr, col = rowptr.cuda(), col.cuda()
    torch.manual_seed(2)
    model = GATv2(16, hidden, 8, 4, heads=4, share_weights=share).cuda()
    gatv2_inference(model, x[:64], rowptr[:65].clone(), col[:192] % 64)          # (warm the GEMM library's workspaces)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = gatv2_inference(model, x, rowptr, col)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    M = n * hidden * 4
    live = 2 if share else 3
    print(f"GATV2_MEMORY share={share}: peak {peak / M:.2f} matrices of {M / 1e6:.1f} MB (counted live: {live})")
    assert out.shape == (n, 8)
    assert peak <= (live + 0.5) * M, (peak / M, live)


def test_shapes_the_kernels_do_not_take_are_refused_with_the_arithmetic():
    from salient_plusplus_amd.inference import evaluate, gatv2_inference
    from salient_plusplus_amd.models import GATv2
    rowptr, col = _graph()
    x = _features()
    for entry in (gatv2_inference, evaluate):
        with pytest.raises(NotImplementedError, match=r"heads = 3"):
            entry(GATv2(FIN, 36, 5, 2, heads=3).cuda(), x, rowptr, col)
        with pytest.raises(NotImplementedError, match=r"8 \* 256 = 2048"):
            entry(GATv2(FIN, 32, 172, 2, heads=8).cuda(), x, rowptr, col)
    with pytest.raises(NotImplementedError, match=r"^layerwise_inference: layer 0 has heads = 3"):
        GATv2(FIN, 36, 5, 2, heads=3).cuda().inference(x, rowptr, col)


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("H,classes,share", [(4, 5, False), (4, 8, True), (1, 5, False)])
def test_the_method_and_both_entries_return_the_same_bits(H, classes, share, act_dtype):
    """``layerwise_inference`` takes the model, ``gatv2_inference`` is that call and ``GATv2.inference`` is too"""
    from inference_method import assert_method_equals_function
    from salient_plusplus_amd.inference import gatv2_inference, layerwise_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(H, classes, share).train()
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, HUB, HUB, 0, 3, HUB])])
    sub = assert_method_equals_function(model, x, rowptr, col, nodes, act_dtype)
    assert sub.shape == (nodes.numel(), classes)
    for kw in (dict(), dict(nodes=nodes), dict(rows_per_slab=64), dict(nodes=nodes, rows_per_slab=64)):
        assert torch.equal(layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype, **kw),
                           gatv2_inference(model, x, rowptr, col, act_dtype=act_dtype, **kw)), sorted(kw)
    assert model.training
