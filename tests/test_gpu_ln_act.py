"""GPU: the f4f kernels (csrc/ln_act.hip; spp.h, spp_ln_act_forward / _backward) against a float64 restatement of their
contract, plain torch on the CPU, on the same fp32 / bf16 inputs.  The margin is bn_act's, measured and not chosen: torch's
own fp32 GPU path (F.layer_norm, the activation, the same mask, autograd) is compared with the same float64 values; the
kernels may be off by at most TWICE torch's error plus one fp32 ulp of the largest expected magnitude (bf16 output: plus half
a bf16 ulp of the value).  Both errors are printed (LN_ACT_ERR).  Inputs are nudged on the CPU until no float64
pre-activation lies within 1e-4 of zero (far above u's fp32 error): every activation's sign is decided."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = float(np.float32(1e-5))                                 # the descriptor's eps is an fp32
ACTS, SLOPE = ("none", "relu", "leaky_relu"), 0.01
R, SEED = 64, 0x1234567                                       # R: SPP_LN_ACT_SLAB_ROWS (_kernels asserts it)
_P = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None  # noqa: E731


def _kernels(z, gamma, beta, g, *, act, p, training, r=None, y_dtype=F32):
    """both entries as they stand: (y, mean, rstd, dz, dgamma, dbeta)"""
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    assert int(L.spp_ln_act_slab_rows()) == R
    n, Cd = z.shape
    el = {F32: 0, BF16: 2}
    nan = lambda shape, dt=F32: torch.full(shape, float("nan"), dtype=dt, device="cuda")
    y, mean, rstd, dz, dgamma, dbeta = nan((n, Cd), y_dtype), nan((n,)), nan((n,)), nan((n, Cd), z.dtype), nan((Cd,)), nan((Cd,))
    ws = torch.empty(int(L.spp_ln_act_workspace_bytes(n, Cd)), dtype=torch.uint8, device="cuda")
    d = nat.LnActDesc(z_elem=el[z.dtype], r_elem=el[r.dtype] if r is not None else 0, y_elem=el[y_dtype], g_elem=el[g.dtype],
                      act=ACTS.index(act), training=int(training), negative_slope=SLOPE, p=p, eps=EPS, seed=SEED, n=n, C=Cd,
                      z_dev=_P(z), gamma_dev=_P(gamma), beta_dev=_P(beta), r_dev=_P(r), y_dev=_P(y), mean_dev=_P(mean),
                      rstd_dev=_P(rstd), g_dev=_P(g), dz_dev=_P(dz), dgamma_dev=_P(dgamma), dbeta_dev=_P(dbeta),
                      workspace_dev=_P(ws), workspace_bytes=ws.numel())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nat.check(L.spp_ln_act_forward(C.byref(d), st))
    nat.check(L.spp_ln_act_backward(C.byref(d), st))
    return y, mean, rstd, dz, dgamma, dbeta


def _public(z, gamma, beta, g, *, act, p, training, r=None, y_dtype=F32, amp=False, monkeypatch=None):
    """the same six through models.layer_norm_act and autograd (mean, rstd: None), the seed planted; r goes in as fp32"""
    from salient_plusplus_amd import models
    monkeypatch.setattr(models, "_draw_seed", lambda: SEED)
    ln = torch.nn.LayerNorm(z.size(1), eps=EPS).cuda()
    ln.weight.data.copy_(gamma), ln.bias.data.copy_(beta)
    zk, rk = z.requires_grad_(True), (r.float().requires_grad_(True) if r is not None else None)
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        y = models.layer_norm_act(zk, ln, act=act, negative_slope=SLOPE, p=p, training=training, residual=rk)
    assert type(y.grad_fn).__name__ == "_LayerNormActBackward" and y.dtype == y_dtype
    (y * g).sum().backward()
    assert rk is None or torch.equal(rk.grad, g.float())      # the residual's gradient is g itself
    return y.detach(), None, None, zk.grad, ln.weight.grad, ln.bias.grad


def _keep(n, Cd, p):
    """act_keep.hip.h: e is kept iff the low (e even) or high half of mix64(SEED + (e >> 1) * GOLD) < (1 - p) * 2^32"""
    e = np.arange(n * Cd, dtype=np.uint64)
    x = np.uint64(SEED) + (e >> np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    half = np.where(e & np.uint64(1), x >> np.uint64(32), x & np.uint64(0xFFFFFFFF))
    return torch.from_numpy(half < np.uint64(int((1.0 - p) * 4294967296.0))).reshape(n, Cd)


def _restate(z, gamma, beta, g, r, act, keep, dt, dev):
    """the contract in plain torch at (dt, dev): (y, mean, rstd, dz, dgamma, dbeta); keep = mask * 1 / (1 - p)"""
    zz, ga, be = (t.to(dev, dt).requires_grad_(True) for t in (z, gamma, beta))
    h = F.layer_norm(zz, (z.size(1),), ga, be, EPS)
    h = F.relu(h) if act == "relu" else F.leaky_relu(h, SLOPE) if act == "leaky_relu" else h
    y = h * keep.to(dev, dt)
    (y * g.to(dev, dt)).sum().backward()
    if dt == F32:                                             # torch's own fp32 statistics
        mean, rstd = (t.reshape(-1) for t in torch.native_layer_norm(zz.detach(), (z.size(1),), ga.detach(), be.detach(), EPS)[1:])
    else:
        mean, rstd = zz.detach().mean(1), 1.0 / torch.sqrt(zz.detach().var(1, unbiased=False) + EPS)
    return (y.detach() + r.to(dev, dt) if r is not None else y.detach()), mean, rstd, zz.grad, ga.grad, be.grad


def _bounded(tag, got, torchs, want64, names=("y", "mean", "rstd", "dz", "dgamma", "dbeta")):
    """|got - want| <= 2 |torch - want| + ulp32(max |want|) [+ half a bf16 ulp of want]; prints both errors"""
    for name, a, t, e in zip(names, got, torchs, want64):
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), (tag, name)
        ek, et = ((x.double().cpu() - e).abs() for x in (a, t))
        top = float(e.abs().max())
        floor = 2.0 ** (math.frexp(top)[1] - 24) if top else 0.0
        half = torch.ldexp(torch.ones_like(e), torch.frexp(e)[1] - 9) * (e != 0) if a.dtype == BF16 else 0.0
        print(f"LN_ACT_ERR {tag} {name}: kernel {float(ek.max()):.3e} torch {float(et.max()):.3e} "
              f"ratio {float(ek.max()) / float(et.max()) if float(et.max()) else float('inf'):.2f} ulp {floor:.3e}")
        assert bool((ek <= 2 * float(et.max()) + floor + half).all()), (tag, name, float(ek.max()), float(et.max()), floor)


def _case(tag, n, Cd, seed, *, act, p, with_r, training, zdt=F32, ydt=F32, rows=None, run=_kernels, **kw):
    """seeded inputs with no float64 pre-activation within 1e-4 of zero (given `rows` are only checked); `run` against
    float64 under the margin, twice with identical bits, and rows [:m] alone with the bits of the whole; returns run's six"""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn((n, Cd), generator=gen) * 2.0 + 1.5 if rows is None else rows
    gamma, beta = torch.rand(Cd, generator=gen) + 0.5, torch.randn(Cd, generator=gen) * 0.5
    for _ in range(3):
        z = z.to(zdt).float()
        tie = F.layer_norm(z.double(), (Cd,), gamma.double(), beta.double(), EPS).abs() < 1e-4
        if rows is not None or not bool(tie.any()):
            break
        assert int(tie.sum()) < 0.01 * n * Cd
        z = z + tie * 0.0625
    assert not bool((tie & (z.var(1, keepdim=True) > 0)).any()), "an undecided sign"   # (a constant row: u = beta)
    g, r = (torch.randn((n, Cd), generator=gen).to(zdt).float() for _ in range(2))     # representable in every type used
    r = r if with_r else None
    keep = _keep(n, Cd, p) / (1.0 - p) if training and p > 0 else torch.ones((n, Cd))
    want, tor = (_restate(z, gamma, beta, g, r, act, keep, dt, dev) for dt, dev in ((F64, "cpu"), (F32, "cuda")))
    m = (n + 1) // 2
    part = lambda t, k: t[:k].cuda().to(zdt).contiguous() if t is not None else None
    go = lambda k: run(part(z, k), gamma.cuda(), beta.cuda(), part(g, k), act=act, p=p, training=training, r=part(r, k), y_dtype=ydt, **kw)
    got, again, few = go(n), go(n), go(m)
    _bounded(tag, got, tor, want)
    assert all(a is None or torch.equal(a, b) for a, b in zip(got, again))
    assert all(a is None or torch.equal(a[:m], b) for a, b in zip(got[:3], few[:3]))
    return got


# (act, p, residual, training, z / g / r type, y type)
CONFIGS = [("relu", 0.5, False, True, F32, F32), ("leaky_relu", 0.0, True, True, F32, BF16), ("none", 0.5, True, True, BF16, F32),
           ("relu", 0.5, False, False, F32, F32), ("leaky_relu", 0.5, True, True, BF16, BF16)]


@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
@pytest.mark.parametrize("Cd", [4, 12, 256, 260, 1024])
def test_entries_against_float64_twice_and_by_rows(Cd, cfg):
    act, p, with_r, training, zdt, ydt = CONFIGS[cfg]
    gpb = 256 // min(64, 1 << (Cd // 4 - 1).bit_length())     # rows per forward workgroup
    for n in sorted({1, 2, gpb - 1, gpb + 1, R - 1, R + 1, 2 * R + 3}):
        _case(f"[{n}x{Cd} cfg{cfg}]", n, Cd, 1000 * n + Cd + cfg, act=act, p=p, with_r=with_r, training=training, zdt=zdt, ydt=ydt)


@pytest.mark.parametrize("Cd", [12, 256, 1024])
def test_hard_rows(Cd):
    """a constant row, a row of mean 1e4 and unit spread (an E[z^2] - mean^2 variance fails it), values near 1e-20"""
    gen = torch.Generator().manual_seed(Cd + 1)                # (seeds whose float64 reference has no undecided sign: _case checks)
    rows = torch.stack([torch.full((Cd,), 3.7), torch.randn(Cd, generator=gen) + 1e4,
                        (torch.randn(Cd, generator=gen) * 0.5 + 1.0) * 1e-20])
    got = _case(f"[hard x{Cd}]", 3, Cd, Cd + 1, act="leaky_relu", p=0.0, with_r=False, training=True, rows=rows)
    assert float(got[2][0]) == pytest.approx(1.0 / math.sqrt(EPS), rel=1e-6)


@pytest.mark.parametrize("amp,p,with_r,zdt", [(False, 0.0, False, F32), (True, 0.0, False, F32), (False, 0.5, True, BF16)])
def test_public_path_fallbacks_and_the_empty_matrix(amp, p, with_r, zdt, monkeypatch):
    from salient_plusplus_amd.models import layer_norm_act    # (the third case: bf16 z, fp32 residual, dropout)
    _case(f"[public amp={amp} p={p}]", R + 1, 256, 17, act="relu", p=p, with_r=with_r, training=True, zdt=zdt, run=_public,
          amp=amp, monkeypatch=monkeypatch)
    # C = 6, a non-contiguous z and no rows: the torch composition's bits, forward and backward, with no kernel call refused
    z = torch.randn((R + 1, 256), device="cuda")
    for zz, node in ((z[:, :6].contiguous(), False), (z[:, ::2], False), (z[:0], True)):
        lm, grads = torch.nn.LayerNorm(zz.size(1)).cuda(), []
        for fn in (lambda t: layer_norm_act(t, lm, act="relu", p=0.0, training=True), lambda t: F.relu(lm(t))):
            t = zz.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=BF16, enabled=amp):
                out = fn(t)
            out.sum().backward()
            grads.append((out.detach(), t.grad))
        assert all(torch.equal(a, b) for a, b in zip(*grads))
        assert node == (type(layer_norm_act(zz.detach().requires_grad_(True), lm).grad_fn).__name__ == "_LayerNormActBackward")


def test_model_step_repeats_and_eval_matches_the_modules():
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    from salient_plusplus_amd.models import GATv2
    adjs = []
    for S, T in ((12, 8), (8, 4), (4, 2)):                    # rows of 1, 2, 3, 1, ... entries (the scaffold tests' batch)
        rows = [[(t + 5 * j) % S for j in range(1 + t % 3)] for t in range(T)]
        rowptr, col = torch.tensor([0] + [len(r) for r in rows]).cumsum(0), torch.tensor([c for r in rows for c in r])
        adjs.append((SparseTensor(rowptr=rowptr.cuda(), col=col.cuda(), sparse_sizes=(T, S)), None, (S, T)))
    x, labels = torch.randn((12, 100), generator=torch.Generator().manual_seed(1)).cuda(), torch.tensor([3, 5]).cuda()
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        model = GATv2(100, 32, 7, 3, heads=4, norm="layer").cuda().train()
        loss = F.nll_loss(model(x, adjs), labels)
        loss.backward()
        grads = {k: v.grad.clone() for k, v in model.named_parameters()}
        assert math.isfinite(float(loss.detach())) and all(bool(torch.isfinite(v).all()) and bool(v.abs().sum() > 0)
                                                           for k, v in grads.items() if k.startswith("norms."))
        torch.optim.SGD(model.parameters(), lr=0.1).step()
        runs.append([loss.detach()] + list(grads.values()) + [v.detach() for v in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    model.eval()                                              # eval: torch.nn.LayerNorm + F.relu spelled out, fp32 and float64
    with torch.no_grad():
        outs = []
        for dt in (F32, F64):
            h = x
            for i, (adj_t, _e, (S, T)) in enumerate(adjs):
                h = model.convs[i]((h, h[:T]), adj_t)
                if i < 2:
                    h = F.relu(F.layer_norm(h.to(dt), (32,), model.norms[i].weight.to(dt), model.norms[i].bias.to(dt), EPS)).float()
            outs.append(torch.log_softmax(h.to(dt), dim=-1))
        _bounded("[model eval]", (model(x, adjs),), (outs[0],), (outs[1].cpu(),), ("log_softmax",))
