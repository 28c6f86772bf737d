"""-m gpu: models.GCN on the HIP kernels against the same modules run on the plain-torch restatements
(models._weighted_reference, models._gcn_norm_reference), on one three-hop MFG sampled from the synthetic generator's
smallest workload (S-tiny).

The tolerance is not fixed in advance: both paths evaluate the same formula in fp32 with different summation trees, so
the restatement's own error against its float64 run on this batch is the yardstick.  For the logits and for every
parameter gradient, the HIP model's error against the float64 run must be within 2 x the fp32 restatement's + 1e-6.
The error of a tensor is its relative Frobenius error, ||a - ref64|| / ||ref64|| (the measure of test_gpu_amp_models.py):
it averages over the tensor's elements, where the largest single deviation of two equally accurate fp32 evaluations
is an extreme value whose ratio is noisy for a 64-element gradient.  Both figures, and the largest absolute
deviations, are printed."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HID, CLASSES = 64, 47


@functools.lru_cache(maxsize=None)
def _batch():
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.fast_trainer.transferers import DevicePrefetcher
    from salient_plusplus_amd.synthetic import make_workload
    dev = torch.device("cuda", 0)
    wl = make_workload("S-tiny", seed=1234, device=dev)
    cfg = FastSamplerConfig(
        x_cpu=wl.x, x_gpu=torch.empty(0), y=wl.y.unsqueeze(-1), rowptr=wl.rowptr, col=wl.col, idx=wl.train_idx[:wl.batch_size],
        batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False, pin_memory=False, distributed=False,
        partition_book=None, cache=fs.Cache(), force_exact_num_batches=True, exact_num_batches=1,
        count_remote_frequency=False, use_cache=False)
    batch = next(iter(DevicePrefetcher([dev], iter(FastSampler(2, 4, cfg)))))[0]
    torch.cuda.synchronize()
    assert len(batch.adjs) == 3
    return batch.x, batch.adjs, batch.y.reshape(-1)


def _model(normalize, fused_norm, train=False):
    from salient_plusplus_amd.models import GCN
    x, _adjs, _y = _batch()
    torch.manual_seed(0)
    m = GCN(x.size(1), HID, CLASSES, 3, normalize=normalize, fused_norm=fused_norm).cuda()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                    # statistics and an affine map that do something in eval mode
        for bn in m.bns:
            bn.running_mean.copy_(torch.randn(HID, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(HID, generator=g) + 0.5)
            bn.weight.copy_(torch.rand(HID, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(HID, generator=g) * 0.1)
    return m.train() if train else m.eval()


def _restated(model, x, adjs):
    """model's forward with the kernels replaced by the plain-torch restatements, in the dtype of its parameters"""
    from salient_plusplus_amd.models import _gcn_norm_reference, _weighted_reference
    dt = model.convs[0].lin.weight.dtype
    x = x.to(dt)
    for i, (adj_t, _e, size) in enumerate(adjs):
        rowptr, col, value = adj_t.csr()
        T = int(size[1])
        w, sw = torch.ones(col.numel(), dtype=dt, device=col.device) if value is None else value.to(dt), None
        if model.normalize:
            w, sw = _gcn_norm_reference(rowptr, col, T, None if value is None else w, dtype=dt)
        x = F.linear(_weighted_reference(x, rowptr, col, w, T, sw), model.convs[i].lin.weight)
        if i != model.num_layers - 1:
            x = F.dropout(F.relu(model.bns[i](x)), p=0.5, training=model.training)
    return torch.log_softmax(x, dim=-1)


def _step(model, forward, x, adjs, y):
    model.zero_grad(set_to_none=True)
    out = forward(x, adjs)
    loss = F.nll_loss(out, y)
    loss.backward()
    return out.detach(), loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("fused_norm", [False, True], ids=["torch_tail", "fused_norm"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
def test_eval_step_matches_the_restatement_within_its_own_error(normalize, fused_norm):
    x, adjs, y = _batch()
    hip = _model(normalize, fused_norm)
    ref64 = copy.deepcopy(hip).double()
    out_h, loss_h, g_h = _step(hip, hip, x, adjs, y)
    out_r, _loss_r, g_r = _step(hip, lambda a, b: _restated(hip, a, b), x, adjs, y)
    out_d, _loss_d, g_d = _step(ref64, lambda a, b: _restated(ref64, a, b), x, adjs, y)
    assert out_h.shape == (int(adjs[-1].size[1]), CLASSES) and out_h.dtype == torch.float32 and bool(torch.isfinite(loss_h))
    used = [f"convs.{i}.lin.weight" for i in range(3)] + [f"bns.{i}.{n}" for i in range(2) for n in ("weight", "bias")]
    assert sorted(g_h) == sorted(g_r) == sorted(g_d) == sorted(used)         # (the last BatchNorm is unused)
    pairs = [("logits", out_h, out_r, out_d)] + [(n, g_h[n], g_r[n], g_d[n]) for n in used]
    worse = {}
    for name, h, r, d in pairs:
        assert h.shape == d.shape and h.dtype == torch.float32
        scale = float(d.norm().clamp(min=1e-300))
        e_ref, e_hip = float((r.double() - d).norm()) / scale, float((h.double() - d).norm()) / scale
        print(f"\nGCN_ERR normalize={normalize} fused_norm={fused_norm} {name}: restatement {e_ref:.3e} hip {e_hip:.3e}"
              f" (max abs {float((r.double() - d).abs().max()):.3e} / {float((h.double() - d).abs().max()):.3e})")
        if not e_hip <= 2 * e_ref + 1e-6:
            worse[name] = (e_hip, e_ref)
    assert not worse, worse


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
def test_training_step_runs_with_both_tails(normalize):
    """dropout makes the two tails' outputs differ (torch's generator against the library's): finite loss and the
    gradients' shapes only"""
    x, adjs, y = _batch()
    outs = []
    for fused_norm in (False, True):
        m = _model(normalize, fused_norm, train=True)
        torch.manual_seed(5)
        out, loss, grads = _step(m, m, x, adjs, y)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(out).all())
        assert {n: g.shape for n, g in grads.items()} == {n: p.shape for n, p in m.named_parameters() if not n.startswith("bns.2.")}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert int(m.bns[0].num_batches_tracked) == 1 and int(m.bns[2].num_batches_tracked) == 0
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])                 # (dropout was on)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_first_layer_over_rows_read_in_place_equals_the_materialised_run(amp):
    from salient_plusplus_amd.fast_sampler import TableRows
    x, adjs, _y = _batch()
    g = torch.Generator().manual_seed(6)
    table = torch.randn((900, x.size(1)), generator=g).half().cuda()
    n_id = torch.randint(0, 900, (x.size(0),), generator=g).cuda()
    for normalize in (False, True):
        m = _model(normalize, False)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            a, b = m(TableRows(table, n_id), adjs), m(table[n_id], adjs)
        assert a.shape == (int(adjs[-1].size[1]), CLASSES) and torch.equal(a, b)
