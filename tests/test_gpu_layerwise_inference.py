"""inference.layerwise_inference (SAGE.inference, GIN.inference): exact full-graph inference against the model's own,
tested forward over the same graph handed in as L identical full hops (T = S = N), with the tolerances the model tests
use against plain torch (test_gpu_model_step.py: SAGE fp32 rtol 1e-4 / atol 1e-5; test_gpu_gin_sage_ri.py: GIN fp32
1e-4 of the output's scale; test_gpu_amp_models.py: bf16 outputs within 1e-2 in relative norm)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, FIN, HID, CLASSES = 600, 32, 16, 5
CASES = [("sage", 2), ("sage", 3), ("gin", 2)]
ACT_DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _graph():
    """600 nodes, degrees 0..12 and three hubs above C; fp16 features; everything on the GPU"""
    from salient_plusplus_amd.inference import graph_agg_chunk
    Cc = graph_agg_chunk()
    g = torch.Generator().manual_seed(5)
    deg = torch.randint(0, 13, (N,), generator=g)
    deg[11], deg[300], deg[N - 1] = Cc + 1, 3 * Cc + 7, 9 * Cc
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    x = torch.randn((N, FIN), generator=g).to(torch.float16)
    return x.cuda(), rowptr.cuda(), col.cuda()


def _model(kind, layers):
    from salient_plusplus_amd.models import GIN, SAGE
    torch.manual_seed(20 + layers)
    if kind == "sage":
        return SAGE(FIN, HID, CLASSES, layers).cuda()
    m = GIN(FIN, HID, CLASSES, layers).cuda()
    g = torch.Generator().manual_seed(8)
    for mod in m.modules():                                    # non-trivial running statistics and affine terms
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.5)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.0 + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m


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


def _assert_matches(kind, act_dtype, got, want, what):
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all()), what
    if act_dtype == torch.bfloat16:
        rel = float((got - want).norm() / want.norm())
        print(f"{what}: relative error {rel:.3e}")
        assert rel < 1e-2, (what, rel)
    elif kind == "sage":
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5, msg=lambda m: f"{what}: {m}")
    else:
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * float(want.abs().max()) + 1e-8,
                                   msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("act_dtype", ACT_DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("kind,layers", CASES)
def test_inference_matches_the_forward_over_full_hops(kind, layers, act_dtype):
    """items 7, 8, 9 and the state half of 10"""
    from salient_plusplus_amd.inference import graph_aggregate, layerwise_inference
    x, rowptr, col = _graph()
    model = _model(kind, layers).train()
    want = _forward_over_full_hops(model, x, rowptr, col, layers, act_dtype)
    got = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)
    assert got.shape == (N, CLASSES)
    _assert_matches(kind, act_dtype, got, want, f"{kind} x{layers} {act_dtype}")
    assert model.training and all(p.grad is None for p in model.parameters()) and not got.requires_grad
    model.eval()
    assert torch.equal(model.inference(x, rowptr, col, act_dtype=act_dtype), got) and not model.training
    # nodes=: exactly the rows of the full result (an unsorted list with duplicates)
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, 300, 300, 0, 11])])
    sub = model.inference(x, rowptr, col, nodes=nodes, act_dtype=act_dtype)
    assert sub.shape == (nodes.numel(), CLASSES)
    assert torch.equal(sub, got[nodes.cuda()])
    # the slab size changes nothing the GEMMs read
    for rows in (64, 1000, 1 << 20):
        _assert_matches(kind, act_dtype, layerwise_inference(model, x, rowptr, col, rows_per_slab=rows, act_dtype=act_dtype),
                        want, f"{kind} x{layers} {act_dtype} slabs of {rows}")
    epilogue, scale = ("operand", 0.0) if kind == "sage" else ("sum", 1.0)
    whole = graph_aggregate(x, rowptr, col, row0=0, num_targets=N, epilogue=epilogue, self_scale=scale, out_dtype=act_dtype)
    for rows in (64, 1000):
        parts = [graph_aggregate(x, rowptr, col, row0=s, num_targets=min(rows, N - s), epilogue=epilogue, self_scale=scale,
                                 out_dtype=act_dtype) for s in range(0, N, rows)]
        assert torch.equal(torch.cat(parts), whole)


def test_every_models_method_is_the_function_and_inputs_it_does_not_read():
    """the refusals of item 10; GAT's and SAGEResInception's methods are ``layerwise_inference`` as SAGE's is"""
    from inference_method import assert_method_equals_function
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import TableRows
    from salient_plusplus_amd.models import GAT, SAGE, SAGEResInception
    x, rowptr, col = _graph()
    nodes = torch.tensor([N - 1, 300, 300, 0, 11, 7])
    torch.manual_seed(9)
    for other in (GAT(FIN, HID, CLASSES, 2).cuda(), SAGEResInception(FIN, HID, CLASSES, 2).cuda()):
        assert assert_method_equals_function(other, x, rowptr, col, nodes, torch.float32).shape == (6, CLASSES)
    model = SAGE(FIN, HID, CLASSES, 2).cuda()
    with pytest.raises(TypeError, match="fp8"):
        model.inference(fp8.quantize_e4m3(x), rowptr, col)
    with pytest.raises(TypeError, match="TableRows"):
        model.inference(TableRows(x, torch.arange(4).cuda()), rowptr, col)
    with pytest.raises(ValueError, match="outside the graph"):
        model.inference(x, rowptr, col, nodes=torch.tensor([0, N]))
    assert model.training


def test_inference_through_the_sampler_resident_graph():
    """item 11: a FastSampler over S-tiny hands out the resident (x, rowptr, col) its sessions read"""
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.models import SAGE
    from salient_plusplus_amd.synthetic import make_workload
    wl = make_workload("S-tiny", device=torch.device("cuda", 0))
    cfg = FastSamplerConfig(
        x_cpu=wl.x.cpu(), x_gpu=torch.empty(0), y=wl.y.cpu().unsqueeze(-1), rowptr=wl.rowptr.cpu(), col=wl.col.cpu(),
        idx=wl.train_idx.cpu(), batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False, pin_memory=False,
        distributed=False, partition_book=None, cache=fs.Cache(), force_exact_num_batches=False, exact_num_batches=0,
        count_remote_frequency=False, use_cache=False)
    sampler = FastSampler(2, 4, cfg)
    x, rowptr, col = sampler.resident_graph()
    assert x.is_cuda and rowptr.is_cuda and col.is_cuda and x.shape == (20_000, 32) and rowptr.numel() == 20_001
    session = iter(sampler).session                            # a session of the sampler holds the very same tensors
    sx, srp, scol = session.resident_graph()
    assert sx.data_ptr() == x.data_ptr() and srp.data_ptr() == rowptr.data_ptr() and scol.data_ptr() == col.data_ptr()
    torch.manual_seed(3)
    model = SAGE(32, 64, 47, 3).cuda()
    out = model.inference(*sampler.resident_graph())
    assert out.shape == (20_000, 47) and bool(torch.isfinite(out).all())
    assert float((out.exp().sum(dim=1) - 1.0).abs().max()) < 1e-5
    cfg_dist = FastSamplerConfig(**{**cfg.__dict__, "distributed": True, "partition_book": fs.RangePartitionBook(
        0, 2, torch.tensor([0, 10_000, 20_000]))})
    with pytest.raises(RuntimeError, match="distributed"):
        FastSampler(2, 4, cfg_dist).resident_graph()
