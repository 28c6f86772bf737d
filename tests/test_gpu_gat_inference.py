"""spp_graph_gat_forward (inference.graph_gat_aggregate) and layerwise_inference over GAT: the long-row softmax of exact
layer-wise inference, against a float64 restatement of GATConv's formula, against itself bit for bit (slabs, lists,
repeated calls), with ids that leave the graph, with offsets past 2^32 bytes, and as a whole model against the model's
own forward over L identical full hops.

Tolerance of the kernel tests, fp32 output: the project's forward tolerance for the GAT kernels (test_gpu_gat_heads.py,
FWD: rtol 2e-4, atol 2e-5) with the atol scaled by max(1, max|h|).  The output is a convex combination of rows of h;
with |e| <= 8 a weight carries about 1e-6 relative error from __expf, and the accumulation of a 9 C_g row at most
(C_g + 9 + 2) * 2^-24, together under 1e-5 * max|h|.  A bf16 output adds one rounding: 2^-8 relative.

GAT(32, 16, 5, L) cannot be built with heads=3 (the model wants hidden % heads == 0), so that case has hidden 18: six
columns a head, the scalar form with a head count that is no power of two."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 600
FWD = dict(rtol=2e-4, atol=2e-5)
HEADS_WIDTHS = [(1, 16), (1, 5), (4, 64), (3, 20), (2, 47)]
H_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
OUT_DTYPES = [torch.float32, torch.bfloat16]
SLOPE = 0.2
EMPTY_CHUNK_ROW, DEG0 = 200, 5


def _name(d):
    return str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _graph():
    """600 nodes, degrees 0..12; rows of exactly C_g, C_g + 1, 3 C_g + 7 and 9 C_g raw entries; diagonal and duplicate
    entries in short and long rows; a long row whose second chunk is nothing but its own id; a node of degree 0"""
    from salient_plusplus_amd.inference import graph_gat_chunk
    Cg = graph_gat_chunk()
    g = torch.Generator().manual_seed(5)
    deg = torch.randint(0, 13, (N,), generator=g)
    deg[DEG0], deg[20] = 0, 6
    deg[10], deg[11], deg[300], deg[N - 1], deg[EMPTY_CHUNK_ROW] = Cg, Cg + 1, 3 * Cg + 7, 9 * Cg, 2 * Cg + 5
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    b = rowptr[20]
    col[b + 1], col[b + 3] = 20, col[b + 2]                   # a short row: a diagonal entry and a duplicate
    b = rowptr[10]
    col[b], col[b + Cg - 1] = 10, 10                          # exactly C_g raw entries, diagonal at both ends
    b = rowptr[300]
    col[b + 2], col[b + Cg + 6], col[b + Cg + 8] = 300, 300, col[b + Cg + 7]
    b = rowptr[N - 1]
    col[b + 3], col[b + 5 * Cg], col[b + 9 * Cg - 1] = N - 1, N - 1, col[b + 9 * Cg - 2]
    b = rowptr[EMPTY_CHUNK_ROW]
    col[b + Cg:b + 2 * Cg] = EMPTY_CHUNK_ROW                  # chunk 1 is empty once the diagonal is dropped
    return rowptr.cuda(), col.cuda()


PLANTED = [DEG0, 10, 11, 20, 300, N - 1, EMPTY_CHUNK_ROW]


@functools.lru_cache(maxsize=None)
def _inputs(H, Cw, h_dtype):
    g = torch.Generator().manual_seed(100 * H + Cw)
    h = torch.randn((N, H * Cw), generator=g).to(h_dtype).cuda()
    a_src = (torch.rand((N, H), generator=g) * 8 - 4).cuda()
    a_dst = (torch.rand((N, H), generator=g) * 8 - 4).cuda()
    return h, a_src, a_dst


def _gat_f64(h, a_src, a_dst, rowptr, col, H, slope):
    """the formula in plain torch on float64 copies: row t of col without its entries j == t, one self loop,
    e = leaky_relu(a_src[j] + a_dst[t]), softmax over the row, the weighted sum of the rows of h; [n, H * C]"""
    n = h.size(0)
    h64 = h.double().view(n, H, -1)
    col = torch.where((col >= 0) & (col < n), col, torch.zeros_like(col))       # an entry outside the graph is node 0
    nodes = torch.arange(n, device=h.device)
    dst = torch.repeat_interleave(nodes, rowptr[1:] - rowptr[:-1])
    keep = col != dst
    src, dst = torch.cat([col[keep], nodes]), torch.cat([dst[keep], nodes])
    e = torch.nn.functional.leaky_relu(a_src.double()[src] + a_dst.double()[dst], slope)
    emax = torch.full((n, H), float("-inf"), dtype=torch.float64, device=h.device)
    emax = emax.scatter_reduce(0, dst[:, None].expand(-1, H), e, "amax")
    w = torch.exp(e - emax[dst])
    den = torch.zeros((n, H), dtype=torch.float64, device=h.device).index_add_(0, dst, w)
    out = torch.zeros_like(h64).index_add_(0, dst, (w / den[dst])[:, :, None] * h64[src])
    return out.reshape(n, -1)


@functools.lru_cache(maxsize=None)
def _reference(H, Cw, h_dtype):
    rowptr, col = _graph()
    return _gat_f64(*_inputs(H, Cw, h_dtype), rowptr, col, H, SLOPE)


def _whole(H, Cw, h_dtype, **kw):
    from salient_plusplus_amd.inference import graph_gat_aggregate
    return graph_gat_aggregate(*_inputs(H, Cw, h_dtype), *_graph(), heads=H, negative_slope=SLOPE, row0=0, num_targets=N,
                               **kw)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=_name)
@pytest.mark.parametrize("h_dtype", H_DTYPES, ids=_name)
@pytest.mark.parametrize("H,Cw", HEADS_WIDTHS)
def test_kernel_matches_the_float64_formula(H, Cw, h_dtype, out_dtype, relu):
    h = _inputs(H, Cw, h_dtype)[0]
    want = _reference(H, Cw, h_dtype)
    want = torch.relu(want) if relu else want
    got = _whole(H, Cw, h_dtype, relu=relu, out_dtype=out_dtype)
    assert got.dtype == out_dtype and got.shape == (N, H * Cw)
    scale = max(1.0, float(h.abs().max()))
    rtol = FWD["rtol"] + (2.0 ** -8 if out_dtype == torch.bfloat16 else 0.0)
    err = (got.double() - want).abs()
    print(f"H={H} C={Cw} h={_name(h_dtype)} out={_name(out_dtype)} relu={relu}: max abs error {float(err.max()):.3e}, "
          f"max error / (atol + rtol |want|) {float((err / (FWD['atol'] * scale + rtol * want.abs())).max()):.3e}")
    torch.testing.assert_close(got.double(), want, rtol=rtol, atol=FWD["atol"] * scale)
    assert torch.equal(got[DEG0].double(), (torch.relu(h[DEG0]) if relu else h[DEG0]).to(out_dtype).double())


@pytest.mark.parametrize("H,Cw,h_dtype", [(4, 64, torch.bfloat16), (2, 47, torch.float32), (1, 16, torch.float16)])
def test_a_rows_bits_depend_on_the_row_alone(H, Cw, h_dtype):
    from salient_plusplus_amd.inference import graph_gat_aggregate, graph_gat_workspace_bytes
    h, a_src, a_dst = _inputs(H, Cw, h_dtype)
    rowptr, col = _graph()
    call = functools.partial(graph_gat_aggregate, h, a_src, a_dst, rowptr, col, heads=H, negative_slope=SLOPE, relu=True)
    whole = call(row0=0, num_targets=N)
    for rows in (64, 1000):
        parts = [call(row0=s, num_targets=min(rows, N - s)) for s in range(0, N, rows)]
        assert torch.equal(torch.cat(parts), whole), rows
    g = torch.Generator().manual_seed(2)
    ids = torch.cat([torch.randperm(N, generator=g)[:90], torch.tensor(PLANTED + [300, N - 1, 300])])
    ids = ids[torch.randperm(ids.numel(), generator=g)].cuda()
    assert torch.equal(call(target_ids=ids), whole[ids])
    ws = torch.empty(graph_gat_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    first = call(row0=0, num_targets=N, workspace=ws)
    second = call(row0=0, num_targets=N, workspace=ws)
    assert torch.equal(first, second) and torch.equal(first, whole)
    assert torch.equal(call(target_ids=ids, workspace=ws), whole[ids])


@pytest.mark.parametrize("H,Cw", [(4, 64), (2, 47)])
def test_ids_that_leave_the_graph(H, Cw):
    from salient_plusplus_amd.inference import graph_gat_aggregate
    h, a_src, a_dst = _inputs(H, Cw, torch.float32)
    rowptr, col = _graph()
    bad = col.clone()
    for t, k, j in ((20, 0, N), (30, 0, -3), (300, 5, N + 5), (300, 100, 1 << 40), (N - 1, 7 * 64 + 1, -1), (0, 0, N)):
        if int(rowptr[t + 1] - rowptr[t]) > k:
            bad[rowptr[t] + k] = j
    as_node0 = torch.where((bad >= 0) & (bad < N), bad, torch.zeros_like(bad))
    call = functools.partial(graph_gat_aggregate, h, a_src, a_dst, rowptr, heads=H, negative_slope=SLOPE)
    got = call(bad, row0=0, num_targets=N)
    assert torch.equal(got, call(as_node0, row0=0, num_targets=N))
    torch.testing.assert_close(got.double(), _gat_f64(h, a_src, a_dst, rowptr, bad, H, SLOPE), rtol=FWD["rtol"],
                               atol=FWD["atol"] * max(1.0, float(h.abs().max())))
    ids = torch.tensor([3, N, 300, -1, N + 100, N - 1, 1 << 40, DEG0], device="cuda")
    inside = (ids >= 0) & (ids < N)
    out = call(bad, target_ids=ids)
    assert torch.equal(out[~inside], torch.zeros_like(out[~inside]))
    assert torch.equal(out[inside], got[ids[inside]])


def test_offsets_beyond_32_bits():
    """h as a strided fp16 view: 16 columns at a row stride of 32 768 elements over 70 000 rows (4.6 GB, of which only
    the last thousand rows are written or read), against the same rows as a small dense matrix"""
    from salient_plusplus_amd.inference import graph_gat_aggregate, graph_gat_chunk
    Cg, n, rows, stride, H = graph_gat_chunk(), 1000, 70_000, 32_768, 2
    g = torch.Generator().manual_seed(9)
    deg = torch.randint(0, 13, (n,), generator=g)
    deg[7], deg[n - 1] = 3 * Cg + 7, Cg + 1
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=g)
    col[rowptr[7] + 3] = 7
    small = torch.randn((n, 16), generator=g).to(torch.float16).cuda()
    a_src, a_dst = ((torch.rand((n, H), generator=g) * 8 - 4).cuda() for _ in range(2))
    rowptr, col = rowptr.cuda(), col.cuda()
    want = graph_gat_aggregate(small, a_src, a_dst, rowptr, col, heads=H, row0=0, num_targets=n)

    first = rows - n
    big = torch.empty(rows * stride, dtype=torch.float16, device="cuda").as_strided((rows, 16), (stride, 1))
    big[first:] = small
    big_src, big_dst = (torch.zeros((rows, H), device="cuda") for _ in range(2))
    big_src[first:], big_dst[first:] = a_src, a_dst
    big_rowptr = torch.cat([torch.zeros(first, dtype=torch.int64, device="cuda"), rowptr])
    big_col = col + first
    got = graph_gat_aggregate(big, big_src, big_dst, big_rowptr, big_col, heads=H, row0=first, num_targets=n)
    assert torch.equal(got, want)
    ids = torch.tensor([rows - 1, first + 7, first, first + 7], device="cuda")
    assert torch.equal(graph_gat_aggregate(big, big_src, big_dst, big_rowptr, big_col, heads=H, target_ids=ids),
                       want[ids - first])


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
FIN, CLASSES = 32, 5
MODEL_CASES = [(1, 2, 16), (1, 3, 16), (4, 2, 16), (3, 2, 18)]       # heads, layers, hidden (18: see the module docstring)


@functools.lru_cache(maxsize=None)
def _features():
    return torch.randn((N, FIN), generator=torch.Generator().manual_seed(6)).to(torch.float16).cuda()


def _model(heads, layers, hidden):
    from salient_plusplus_amd.models import GAT
    torch.manual_seed(40 + 10 * heads + layers)
    return GAT(FIN, hidden, CLASSES, layers, heads=heads).cuda()


def _forward_over_full_hops(model, x, rowptr, col, layers, act_dtype):
    """the model's existing forward in eval mode: the graph as `layers` identical full hops"""
    from salient_plusplus_amd.fast_trainer.samplers import Adj__from_fast_sampler
    e_id = torch.empty(0, dtype=torch.int64, device=x.device)
    adjs = [Adj__from_fast_sampler((rowptr, col, e_id, (N, N))) for _ in range(layers)]
    was = model.training
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=act_dtype == torch.bfloat16):
        out = model(x, adjs)
    model.train(was)
    return out.float()


def _model_f64(model, x, rowptr, col):
    """the whole model restated in float64: project, logits, the formula, ReLU between layers, the mean of the last
    layer's heads, log_softmax"""
    cur = x.double()
    for i, conv in enumerate(model.convs):
        H, Cw = conv.heads, conv.out_channels
        h = cur @ conv.lin_src.weight.detach().double().t()
        a_src = (h.view(N, H, Cw) * conv.att_src.detach().double().view(1, H, Cw)).sum(-1)
        a_dst = (h.view(N, H, Cw) * conv.att_dst.detach().double().view(1, H, Cw)).sum(-1)
        out = _gat_f64(h, a_src, a_dst, rowptr, col, H, conv.negative_slope)
        cur = torch.relu(out) if i < len(model.convs) - 1 else out.view(N, H, Cw).mean(1)
    return torch.log_softmax(cur, dim=-1)


def _assert_matches(act_dtype, got, want, what):
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all()), what
    if act_dtype == torch.bfloat16:
        rel = float((got.double() - want.double()).norm() / want.double().norm())
        print(f"{what}: relative error {rel:.3e}")
        assert rel < 1e-2, (what, rel)
    else:
        print(f"{what}: max abs error {float((got.double() - want.double()).abs().max()):.3e}")
        torch.testing.assert_close(got.double(), want.double(), msg=lambda m: f"{what}: {m}", **FWD)


@pytest.mark.parametrize("act_dtype", OUT_DTYPES, ids=_name)
@pytest.mark.parametrize("heads,layers,hidden", MODEL_CASES)
def test_gat_inference_matches_the_forward_over_full_hops(heads, layers, hidden, act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference
    rowptr, col = _graph()
    x = _features()
    model = _model(heads, layers, hidden).train()
    what = f"GAT heads={heads} x{layers} {_name(act_dtype)}"
    got = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)
    assert got.shape == (N, CLASSES)
    _assert_matches(act_dtype, got, _forward_over_full_hops(model, x, rowptr, col, layers, act_dtype), what + " vs forward")
    _assert_matches(act_dtype, got, _model_f64(model, x, rowptr, col), what + " vs float64")
    assert model.training and all(p.grad is None for p in model.parameters()) and not got.requires_grad
    assert float((got.exp().sum(dim=1) - 1.0).abs().max()) < 1e-5
    model.eval()
    assert torch.equal(layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype), got) and not model.training
    # nodes=: exactly the rows of the full result (an unsorted list with duplicates)
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, 300, 300, 0, 11, EMPTY_CHUNK_ROW, DEG0])])
    sub = layerwise_inference(model, x, rowptr, col, nodes=nodes, act_dtype=act_dtype)
    assert sub.shape == (nodes.numel(), CLASSES) and torch.equal(sub, got[nodes.cuda()])
    # the slab size changes no bit
    for rows in (64, 1000, 1 << 20):
        assert torch.equal(layerwise_inference(model, x, rowptr, col, rows_per_slab=rows, act_dtype=act_dtype), got), rows
    with pytest.raises(ValueError, match="outside the graph"):
        layerwise_inference(model, x, rowptr, col, nodes=torch.tensor([0, N]))


@pytest.mark.parametrize("act_dtype", OUT_DTYPES, ids=_name)
@pytest.mark.parametrize("heads,layers,hidden", [(1, 3, 16), (4, 2, 16)])
def test_the_model_method_is_the_function(heads, layers, hidden, act_dtype):
    from inference_method import assert_method_equals_function
    rowptr, col = _graph()
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, 300, 300, 0, 11, EMPTY_CHUNK_ROW, DEG0])])
    model = _model(heads, layers, hidden).train()
    sub = assert_method_equals_function(model, _features(), rowptr, col, nodes, act_dtype)
    assert sub.shape == (nodes.numel(), CLASSES)


def test_gat_inference_through_the_sampler_resident_graph():
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import GAT
    from salient_plusplus_amd.synthetic import make_workload
    wl = make_workload("S-tiny", device=torch.device("cuda", 0))
    cfg = FastSamplerConfig(
        x_cpu=wl.x.cpu(), x_gpu=torch.empty(0), y=wl.y.cpu().unsqueeze(-1), rowptr=wl.rowptr.cpu(), col=wl.col.cpu(),
        idx=wl.train_idx.cpu(), batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False, pin_memory=False,
        distributed=False, partition_book=None, cache=fs.Cache(), force_exact_num_batches=False, exact_num_batches=0,
        count_remote_frequency=False, use_cache=False)
    sampler = FastSampler(2, 4, cfg)
    torch.manual_seed(3)
    model = GAT(32, 64, 47, 3).cuda()
    out = layerwise_inference(model, *sampler.resident_graph())
    assert out.shape == (20_000, 47) and bool(torch.isfinite(out).all())
    assert float((out.exp().sum(dim=1) - 1.0).abs().max()) < 1e-5
