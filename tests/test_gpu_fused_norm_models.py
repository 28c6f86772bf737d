"""GPU: GIN and SAGEResInception with fused_norm=True (models.batch_norm_act on csrc/bn_act.hip) against the same model
with the flag off, loaded from the same state dict, on small delivered batches.  Tolerances are those of
test_gpu_gin_sage_ri.py (its _close: relative to the largest magnitude): eval and train output 1e-4, loss 1e-5, every
parameter gradient 1e-3, running buffers 1e-4, num_batches_tracked equal; the bf16-autocast step is held to
test_gpu_amp_models.py's output tolerance against the fp32 step."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

KINDS = ["gin", "sageresinception"]
AMP_OUT_TOL = 1e-2                                             # test_gpu_amp_models.py: OUT_TOL, relative Frobenius


def _model(kind, Fin, C, fused, dropout=0.0, hid=32):
    from salient_plusplus_amd.models import get_model_type
    return get_model_type(kind)(Fin, hid, C, 3, dropout=dropout, fused_norm=fused).cuda()


def _pair(kind, Fin, C, dropout=0.0):
    torch.manual_seed(3)
    plain = _model(kind, Fin, C, False, dropout)
    fused = _model(kind, Fin, C, True, dropout)
    # BatchNorm away from its initial state: an affine map and statistics worth normalising by
    with torch.no_grad():
        for m in plain.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.5, 0.5), m.running_var.uniform_(0.5, 2.0)
        if kind == "sageresinception":
            torch.nn.init.normal_(plain.res_linears[0].weight, std=0.5)      # a residual that matters
    fused.load_state_dict(plain.state_dict())
    return plain, fused


def _calls(monkeypatch):
    """counts the launches of the fused entries: the flagged model must run them, the other must not"""
    from salient_plusplus_amd import models as M
    seen = []
    real = M._BatchNormAct.apply
    monkeypatch.setattr(M._BatchNormAct, "apply", staticmethod(lambda *a: seen.append(a[0].dtype) or real(*a)))
    return seen


@pytest.mark.parametrize("kind", KINDS)
def test_flagged_models_match_the_unflagged_ones(kind, monkeypatch):
    from test_gpu_gin_sage_ri import _batches, _close, _step
    batches, C = _batches(100, n_batches=2)
    plain, fused = _pair(kind, 100, C)
    seen = _calls(monkeypatch)
    for b in batches:
        T0, end = int(b.adjs[0].size[1]), int(b.adjs[-1].size[1])
        assert end < T0                                      # the concatenated rows are the ones after the residual add
        plain.eval(), fused.eval()
        with torch.no_grad():
            want = plain(b.x, b.adjs)
            assert not seen
            _close(fused(b.x, b.adjs), want, 1e-4, "eval output")
            assert len(seen) == 3
        plain.train(), fused.train()
        seen.clear()
        op, lp, gp = _step(plain, b.x, b.adjs, b.y)
        assert not seen
        of, lf, gf = _step(fused, b.x, b.adjs, b.y)
        assert len(seen) == 3 and all(d == torch.float32 for d in seen)
        seen.clear()
        _close(of, op, 1e-4, "train output")
        _close(lf, lp, 1e-5, "loss")
        assert gf.keys() == gp.keys()
        for n in gp:
            _close(gf[n], gp[n], 1e-3, n)
        bf, bp = dict(fused.named_buffers()), dict(plain.named_buffers())
        assert bf.keys() == bp.keys()
        for n in bp:
            if "running" in n:
                _close(bf[n], bp[n], 1e-4, n)
            else:
                assert torch.equal(bf[n].cpu(), bp[n].cpu()), n


@pytest.mark.parametrize("kind", KINDS)
def test_default_dropouts_are_repeatable_and_training_lowers_the_loss(kind):
    from test_gpu_gin_sage_ri import _batches
    batches, C = _batches(100, n_batches=1, seed=2)
    b = batches[0]
    y = b.y.reshape(-1)

    def run(steps):
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        from salient_plusplus_amd.models import get_model_type
        model = get_model_type(kind)(100, 32, C, 3, fused_norm=True).cuda().train()      # the default dropouts
        assert model.dropout > 0
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        losses, out = [], None
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            out = model(b.x, b.adjs)
            loss = F.nll_loss(out, y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return out.detach(), losses, [p.detach().clone() for p in model.parameters()]

    # a run's first step is a function of the seed alone: the same masks, the same bits.  (Later steps pass through the
    # aggregation backward's fp32 atomics on small hops, whose order is not fixed; the tail's own backward is held to
    # bit-identity in test_gpu_bn_act.py.)
    out_a, loss_a, _ = run(1)
    out_b, loss_b, _ = run(1)
    assert torch.equal(out_a, out_b) and loss_a == loss_b
    _, losses, _ = run(10)
    assert losses[0] == loss_a[0]
    assert all(map(lambda v: v == v, losses)) and losses[-1] < losses[0], losses


@pytest.mark.parametrize("kind", KINDS)
def test_one_step_under_bf16_autocast(kind, monkeypatch):
    from test_gpu_gin_sage_ri import _batches
    batches, C = _batches(128, n_batches=1, seed=4)
    b = batches[0]
    _, fused = _pair(kind, 128, C)
    fused.train()
    state = {k: v.clone() for k, v in fused.state_dict().items()}
    seen = _calls(monkeypatch)

    def step(amp):
        fused.load_state_dict(state)
        fused.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = fused(b.x, b.adjs)
            loss = F.nll_loss(out, b.y.reshape(-1))
        loss.backward()
        return out.detach(), {n: p.grad for n, p in fused.named_parameters()}

    out32, g32 = step(False)
    seen.clear()
    out16, g16 = step(True)
    assert len(seen) == 3 and all(d == torch.bfloat16 for d in seen)      # z arrives as bf16 from the Linear
    assert out16.dtype == torch.float32 and bool(torch.isfinite(out16).all())
    rel = float((out16 - out32).norm() / out32.norm())
    print(f"\nFUSED_NORM_AMP {kind}: output rel err {rel:.3e}")
    assert rel < AMP_OUT_TOL
    assert all(g16[n] is not None and g16[n].dtype == torch.float32 and bool(torch.isfinite(g16[n]).all()) for n in g32)
