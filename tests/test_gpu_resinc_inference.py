"""inference.layerwise_inference for SAGEResInception: exact full-graph inference against the model's own, tested
forward over the same graph handed in as L identical full hops (T = S = N), with the tolerances the model tests use
(test_gpu_gin_sage_ri.py: fp32 rtol 1e-4, atol 1e-4 of the output's scale; test_gpu_amp_models.py: bf16 outputs within
1e-2 in relative norm, the reference under torch.autocast), and the bit-identity properties of the layer-wise driver:
``nodes=`` returns exactly the rows of the full result, the slab size changes no bit, a second call returns the same."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, FIN, HID, CLASSES = 600, 32, 16, 5
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


def _model(layers):
    from salient_plusplus_amd.models import SAGEResInception
    torch.manual_seed(40 + layers)
    m = SAGEResInception(FIN, HID, CLASSES, layers).cuda()
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


def _assert_matches(act_dtype, got, want, what):
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all()), what
    if act_dtype == torch.bfloat16:
        rel = float((got - want).norm() / want.norm())
        print(f"{what}: relative error {rel:.3e} (bound 1e-2)")
        assert rel < 1e-2, (what, rel)
    else:
        print(f"{what}: largest absolute error {float((got - want).abs().max()):.3e}, scale {float(want.abs().max()):.3e}")
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * float(want.abs().max()) + 1e-8,
                                   msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("act_dtype", ACT_DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("layers", [2, 3])
def test_inference_matches_the_forward_over_full_hops(layers, act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    model = _model(layers).train()
    want = _forward_over_full_hops(model, x, rowptr, col, layers, act_dtype)
    got = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype)
    assert got.shape == (N, CLASSES)
    _assert_matches(act_dtype, got, want, f"sageresinception x{layers} {act_dtype}")
    # the training flag is restored, nothing recorded a gradient
    assert model.training and all(p.grad is None for p in model.parameters()) and not got.requires_grad
    model.eval()
    assert torch.equal(layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype), got) and not model.training
    # nodes=: exactly the rows of the full result (an unsorted list with duplicates and the hubs)
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, 300, 300, 0, 11])])
    sub = layerwise_inference(model, x, rowptr, col, nodes=nodes, act_dtype=act_dtype)
    assert sub.shape == (nodes.numel(), CLASSES)
    assert torch.equal(sub, got[nodes.cuda()])
    # the slab size changes no bit, with and without nodes=
    for rows in (64, 1000, 1 << 20):
        assert torch.equal(layerwise_inference(model, x, rowptr, col, rows_per_slab=rows, act_dtype=act_dtype), got), rows
    assert torch.equal(layerwise_inference(model, x, rowptr, col, nodes=nodes, rows_per_slab=32, act_dtype=act_dtype), sub)
    empty = layerwise_inference(model, x, rowptr, col, nodes=torch.empty(0, dtype=torch.int64), act_dtype=act_dtype)
    assert empty.shape == (0, CLASSES) and empty.dtype == torch.float32


@pytest.mark.parametrize("act_dtype", ACT_DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_the_model_method_is_the_function(act_dtype):
    from inference_method import assert_method_equals_function
    x, rowptr, col = _graph()
    g = torch.Generator().manual_seed(1)
    nodes = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([N - 1, 300, 300, 0, 11])])
    for model in (_model(3).train(), _model(2).eval()):
        assert assert_method_equals_function(model, x, rowptr, col, nodes, act_dtype).shape == (nodes.numel(), CLASSES)


def test_a_head_that_is_not_two_linears_is_refused_by_the_function_and_the_method():
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import MLP
    x, rowptr, col = _graph()
    model = _model(2)
    model.mlp = MLP(FIN + HID * 2, 2 * CLASSES, CLASSES, num_layers=2, bn=True, act="LeakyReLU").cuda()
    with pytest.raises(NotImplementedError, match="exactly two Linears"):
        layerwise_inference(model, x, rowptr, col)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: SAGEResInception's head must be exactly two "
                                                  "Linears"):
        model.inference(x, rowptr, col)
    with pytest.raises(ValueError, match="outside the graph"):
        layerwise_inference(_model(2), x, rowptr, col, nodes=torch.tensor([0, N]))


def test_inference_through_the_sampler_resident_graph():
    """a FastSampler over S-tiny hands out the resident (x, rowptr, col) its sessions read"""
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import SAGEResInception
    from salient_plusplus_amd.synthetic import make_workload
    wl = make_workload("S-tiny", device=torch.device("cuda", 0))
    cfg = FastSamplerConfig(
        x_cpu=wl.x.cpu(), x_gpu=torch.empty(0), y=wl.y.cpu().unsqueeze(-1), rowptr=wl.rowptr.cpu(), col=wl.col.cpu(),
        idx=wl.train_idx.cpu(), batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False, pin_memory=False,
        distributed=False, partition_book=None, cache=fs.Cache(), force_exact_num_batches=False, exact_num_batches=0,
        count_remote_frequency=False, use_cache=False)
    sampler = FastSampler(2, 4, cfg)
    x, rowptr, col = sampler.resident_graph()
    assert x.is_cuda and x.shape == (20_000, 32) and rowptr.numel() == 20_001
    torch.manual_seed(3)
    model = SAGEResInception(32, 64, 47, 3).cuda()
    out = layerwise_inference(model, x, rowptr, col)
    assert out.shape == (20_000, 47) and bool(torch.isfinite(out).all())
    assert float((out.exp().sum(dim=1) - 1.0).abs().max()) < 1e-5
    nodes = torch.tensor([19_999, 7, 7, 0, 12_345])
    assert torch.equal(layerwise_inference(model, x, rowptr, col, nodes=nodes), out[nodes.cuda()])
