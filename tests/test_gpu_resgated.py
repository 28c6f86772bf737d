"""GPU: the ResGated kernel pair (csrc/resgated.hip, spp.h f4g) against tests/resgated_f64.py.  Margin (f3p's rule): twice the
error of _resgated_reference in fp32 on the device against the same float64 values, plus one fp32 ulp of the largest value."""
import copy
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resgated_f64 as G  # noqa: E402
from salient_plusplus_amd import _native as nat  # noqa: E402
from salient_plusplus_amd import models  # noqa: E402
from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor  # noqa: E402

pytestmark = pytest.mark.gpu


def _kernels(k, q, v, g, rowptr, col):
    (T, D), S, L = k.shape, q.size(0), nat.load()
    out, gk, gq, gv = (torch.full((n, D), float("nan"), device="cuda") for n in (T, T, S, S))   # every element must be written
    ws = torch.empty(L.spp_resgated_workspace_bytes(T, S, col.numel()), dtype=torch.uint8, device="cuda")
    d = models._resgated_desc(k, q, v, rowptr, col, out_dev=out, grad_out_dev=g, grad_k_dev=gk, grad_q_dev=gq, grad_v_dev=gv,
                              workspace_dev=ws)
    d.workspace_bytes = ws.numel()
    nat.check(L.spp_resgated_forward(C.byref(d), models._stream()))
    nat.check(L.spp_resgated_backward(C.byref(d), models._stream()))
    return out, gk, gq, gv


@pytest.mark.parametrize("regime", G.REGIMES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hop", [h for h in G.HOPS if h != "T0"])
@pytest.mark.parametrize("D", [4, 12, 256, 260, 1024])
def test_both_entries_against_float64_and_their_bits(D, hop, dtype, regime):
    rowptr, col, S = G.hop(hop)
    k, q, v, g = G.inputs(regime, rowptr.numel() - 1, S, D, dtype)
    want = [w.cuda() for w in G.restate(k, q, v, g, rowptr, col)]  # float64, once; then the fp32 reference on the device, once
    k, q, v, g, rowptr, col = (t.cuda() for t in (k, q, v, g, rowptr, col))
    k32, q32, v32 = (t.float().requires_grad_() for t in (k, q, v))
    (out := models._resgated_reference(k32, q32, v32, rowptr, col)).backward(g)
    ref, T, qv = (out.detach(), k32.grad, q32.grad, v32.grad), k.size(0), torch.cat([q, v], 1)
    for halves in (False, True):                                # q and v separate, and the halves of one [S, 2 D] matrix
        qq, vv = (qv[:, :D], qv[:, D:]) if halves else (q, v)
        got = _kernels(k, qq, vv, g, rowptr, col)
        for name, a, r, w in zip(("out", "grad_k", "grad_q", "grad_v"), got, ref, want):
            top = float(w.abs().max())
            err, ref_err = float((a.double() - w).abs().max()), float((r.double() - w).abs().max())
            margin = 2 * ref_err + (2.0 ** (math.floor(math.log2(top)) - 23) if top > 0 else 0.0)
            print(f"RESGATED_ERR D={D} {hop} {dtype} {regime} halves={halves} {name}: err {err:.3e} margin {margin:.3e} reference {ref_err:.3e}")
            assert err <= margin, (name, err, margin)
        assert all(torch.equal(a, b) for a, b in zip(got, _kernels(k, qq, vv, g, rowptr, col)))   # two runs: the same bits
    if (h := T // 2):                                           # the first half of the targets alone: the same rows
        part = _kernels(k[:h], q, v, g[:h], rowptr[:h + 1], col[:int(rowptr[h])])
        assert torch.equal(part[0], got[0][:h]) and torch.equal(part[1], got[1][:h])


def test_no_targets():
    rowptr, col, S = (t.cuda() if torch.is_tensor(t) else t for t in G.hop("T0"))
    k, q, v = (torch.zeros((n, 8), device="cuda", requires_grad=True) for n in (0, S, S))
    (out := models._ResGatedLayer.apply(k, q, v, rowptr, col)).sum().backward()
    assert out.shape == (0, 8) and not q.grad.any() and not v.grad.any() and q.grad.shape == (S, 8)


def _step(model, x, y, hops, dev, dtype, amp=False):
    adjs = [(SparseTensor(rowptr=rp.to(dev), col=cl.to(dev), sparse_sizes=(rp.numel() - 1, S)), None, (S, rp.numel() - 1))
            for rp, cl, S in hops]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        (loss := torch.nn.functional.nll_loss(model(x.to(dev, dtype), adjs), y.to(dev))).backward()
    return [loss.detach().double().cpu()] + [p.grad.double().cpu() for p in model.parameters()]


@pytest.mark.parametrize("amp", [False, True])
def test_model_step_against_float64_and_its_bits(amp, monkeypatch):
    """loss and every parameter gradient: the kernel path within 4x the reference path's distance (same device) to float64"""
    gen, hops = torch.Generator().manual_seed(3), []
    for S, T in ((150, 60), (60, 25), (25, 9)):                 # outermost hop first
        deg = torch.randint(0, 6, (T,), generator=gen)
        hops.append((torch.cat([deg.new_zeros(1), deg.cumsum(0)]), torch.randint(0, S, (int(deg.sum()),), generator=gen), S))
    x, y = torch.randn((150, 100), generator=gen), torch.randint(0, 7, (9,), generator=gen)
    torch.manual_seed(1)
    model = models.ResGated(100, 32, 7, 3, dropout=0.0).train()
    ref = _step(copy.deepcopy(model).double(), x, y, hops, "cpu", torch.float64)
    with monkeypatch.context() as mp:
        mp.setattr(models, "_resgated_kernels_read", lambda *a: False)
        dev = _step(copy.deepcopy(model).cuda(), x, y, hops, "cuda", torch.float32, amp)
    gpu, twice = (_step(copy.deepcopy(model).cuda(), x, y, hops, "cuda", torch.float32, amp) for _ in range(2))
    assert all(torch.equal(a, b) for a, b in zip(gpu, twice))
    for n, r, a, b in zip(["loss"] + [n for n, _ in model.named_parameters()], ref, dev, gpu):
        scale = float(r.abs().max())
        d_ref, d_ker = float((a - r).abs().max()) / scale, float((b - r).abs().max()) / scale
        assert d_ker <= 4 * d_ref, (n, d_ref, d_ker)


@pytest.mark.parametrize("dev,D", [("cpu", 8), ("cuda", 6)])
def test_fallbacks_return_the_references_bits(dev, D, monkeypatch):
    seen, ref = [], models._resgated_reference
    monkeypatch.setattr(models, "_resgated_reference", lambda *a: seen.append(ref(*a)) or seen[-1])
    monkeypatch.setattr(models._ResGatedLayer, "apply", None)   # the kernels' node is not reached
    rowptr, col, S = (t.to(dev) if torch.is_tensor(t) else t for t in G.hop("planted"))
    conv, x = models.ResGatedGraphConv(10, D).to(dev), torch.randn(S, 10, device=dev)
    out = conv((x, x[:5]), SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(5, S)))
    assert len(seen) == 1 and torch.equal(out, seen[0] + conv.lin_skip(x[:5]) + conv.bias)
    k, q = torch.zeros(5, 8, device="cuda"), torch.zeros(S, 16, device="cuda")
    assert models._resgated_kernels_read(k, q[:, :8], q[:, 8:]) and not models._resgated_kernels_read(k, q[:, ::2], q[:, 8:])
