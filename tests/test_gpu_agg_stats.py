"""-m gpu: the one-pass mean / min / max / std kernels (csrc/aggregate_stats.hip, spp.h f4b) against
models._stats_reference in float64 on the CPU, element by element, on one planted hop; then stats_aggregate's dispatch,
PNAConv and a 2-layer PNA step.  Each test prints the largest err / bound per quantity (AGG_STATS_RATIO lines: a record,
DESIGN section 7 f4b keeps the figures seen on an MI355X, not an input to the bounds).

The hop (T 300, S 400): row 0 empty, row 1 of one entry, row 2 = [5, 9, 5, 3] with x[5, 0] the row's minimum (a repeated
source: exactly one of its two entries may be credited), row 3 of 131 entries (an odd tail behind the pairs), row 4 of
ties, then 295 rows of 0..6 random entries (F = 4 puts 256 targets in a workgroup: two workgroups).  Columns: 1 is constant
(var = 0 exactly), 2 is 1000 + 1e-2 noise, every c % 4 == 3 holds multiples of 0.5 (ties), the rest are N(0, 1).

The bounds, u = 2^-24, per (t, c) with d entries, K the first entry's value, w_k = v_k - K, A = sum|w| / d, Q = sum w^2 / d,
m1 = mean - K; every bound is multiplied by G2 = 1 + 2^-10 for second-order terms:
  mean_b   (d + 2) u (|K| + A): the issue's sequential-sum bound (d roundings of w and of the chain, the division, K + m1).
  min, max no arithmetic: exact, and so are kmin / kmax.  With add: ONE rounding of min + add, exact in float64, so the
           reference rounded to fp32 is the value: bound 0.
  var      s2 / d carries (d + 2) u Q (each w^2 2u, the fmaf chain, the division), m1^2 carries 2 |m1| (d + 1) u A + u m1^2,
           the subtraction u Q, var + eps u (var + eps) and eps itself, an fp32 number, u eps.
  std      sqrt(a) - sqrt(a - e) = e / (sqrt(a) + sqrt(a - e)) <= e / (2 sqrt(eps)) with a = var + eps, plus 2u for sqrtf.
  scalers  identity is exact; the others carry 4u (logf 1 ulp = 2u, its division, the product) on top of the block's bound.
  G_a      = sum_s scale_s g: n_s terms, (4 + n_s) u M_a, M_a the sum of absolute values.
  grad_add G_mean + G_min + G_max: (6 + n_s) u (M_mean + M_min + M_max).
  grad_x   a sum of cnt_j terms G_mean / d + cs (v - mean_b) + [kmin] G_min + [kmax] G_max by atomics in any order, cs =
           G_std / (d std).  Per term: (6 + n_s) u M_mean / d; cs within ((7 + n_s) u + b_std / std) of itself; v - mean_b
           within u |mean| + (d + 1) u A + u |v - mean| (mean_b's own rounding of K + m1 plus the chain's: tighter than the
           issue's bound above, which it never exceeds); (4 + n_s) u on the credited G_min / G_max; 3u of the term for its
           three additions; then (cnt_j - 1) u of the terms' absolute sum for the atomics.
  bf16 out one rounding of a value within bound of ref: agg_f64.rounded.
The 1000 + noise column runs on these bounds like every other: with unshifted sums its var would be off by u 10^6 d."""
import copy
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_f64 as A  # noqa: E402
import gatv2_f64  # noqa: E402

pytestmark = pytest.mark.gpu
U, G2, F64 = A.U, A.G2, A.F64
SCALERS = [("identity",), ("identity", "amplification", "attenuation")]
DELTA, EPS = 1.25, 1e-5                                   # (delta: exact in fp32)


@functools.lru_cache(maxsize=None)
def hop():
    g = torch.Generator().manual_seed(7)
    rows = [[], [7], [5, 9, 5, 3], [(11 * i + 3) % 400 for i in range(131)], [2, 6, 2, 6, 8]]
    rows += [torch.randint(0, 400, (int(n),), generator=g).tolist() for n in torch.randint(0, 7, (295,), generator=g)]
    return A._from_rows(rows, len(rows), 400)


@functools.lru_cache(maxsize=None)
def inputs(F, dtype, n_s):
    """(x [S, F] in dtype, add [T, F], g [T, n_s * 4F]), fp32 on the CPU"""
    g = torch.Generator().manual_seed(F)
    x = torch.randn((400, F), generator=g)
    x[:, 3::4] = (2 * x[:, 3::4]).round() / 2
    x[:, 1] = 0.75
    x[:, 2] = 1000 + 1e-2 * x[:, 2]
    x[5, 0] = -7.0
    return x.to(dtype), torch.randn((hop().T, F), generator=g), torch.randn((hop().T, n_s * 4 * F), generator=g)


def expected(x, add, g, scalers):
    """float64 values and bounds: (out, b_out, kmin, kmax, grad_x, b_gx, grad_add, b_ga)"""
    from salient_plusplus_amd.models import _stats_reference
    h, F, ns = hop(), x.size(1), len(scalers)
    T, r = h.T, h.row
    xd = x.double().requires_grad_()
    ad = add.double().requires_grad_() if add is not None else None
    ref, kmin, kmax = _stats_reference(xd, h.rowptr, h.col, T, add=ad, scalers=scalers, delta=DELTA, eps=EPS, with_pos=True)
    ref.backward(g.double())
    ref, xv = ref.detach(), x.double()
    d = h.deg.double().unsqueeze(1)
    dc, has, xs = d.clamp(min=1), d > 0, xv[h.col]
    tsum = lambda v: torch.zeros((T, F), dtype=F64).index_add(0, r, v)
    K = torch.where(has, xv[h.col[h.rowptr[:-1].clamp(max=h.E - 1)]], 0.0)
    w = (xs - K[r]).abs()
    Aabs, Q, mean = tsum(w) / dc, tsum(w * w) / dc, tsum(xs) / dc
    m1 = mean - K
    var = tsum((xs - mean[r]) ** 2) / dc
    std = (var + EPS).sqrt()
    dvar = U * ((d + 2) * Q + 2 * (d + 1) * Aabs * m1.abs() + m1 * m1 + Q + var + 2 * EPS)
    b_std = dvar / ((var + EPS).sqrt() + (var + EPS - dvar).clamp(min=0).sqrt()) + 2 * U * std
    blocks = ref[:, :4 * F].view(T, 4, F)                                   # the identity scaler's: the values themselves
    moved = U * blocks.abs() if add is not None else torch.zeros_like(blocks)
    b_blocks = torch.stack([(d + 2) * U * (K.abs() + Aabs) + moved[:, 0], 0 * moved[:, 1], 0 * moved[:, 2], b_std], 1)
    blocks = torch.where(b_blocks == 0, blocks.float().double(), blocks)   # min + add: the fp32 rounding of an exact sum
    logd = torch.log(dc + 1)
    scale = {"identity": torch.ones_like(logd), "amplification": logd / DELTA, "attenuation": DELTA / logd}
    sc = torch.stack([scale[s] for s in scalers], 1)                        # [T, ns, 1]
    rel = torch.tensor([0.0 if s == "identity" else 4 * U for s in scalers], dtype=F64).view(1, ns, 1, 1)
    out = sc.unsqueeze(2) * blocks.unsqueeze(1) * has.view(T, 1, 1, 1)
    b_out = G2 * (sc.unsqueeze(2) * b_blocks.unsqueeze(1) + rel * out.abs()) * has.view(T, 1, 1, 1)
    M = (sc.unsqueeze(2) * g.double().view(T, ns, 4, F).abs()).sum(1) * has.view(T, 1, 1)      # [T, 4, F]: mean min max std
    b_ga = G2 * U * (6 + ns) * (M[:, 0] + M[:, 1] + M[:, 2])
    k = torch.arange(h.E).unsqueeze(1)
    hitn, hitx = (k == kmin[r]).double(), (k == kmax[r]).double()
    dv, cs = (xs - mean[r]).abs(), (M[:, 3] / (dc * std))[r]
    dmean = U * mean.abs() + (d + 1) * U * Aabs
    credited = hitn * M[r, 1] + hitx * M[r, 2]
    Mterm = (M[:, 0] / dc)[r] + cs * dv + credited
    dterm = ((6 + ns) * U * (M[:, 0] / dc)[r] + ((7 + ns) * U + (b_std / std)[r]) * cs * dv + cs * (dmean[r] + U * dv)
             + (4 + ns) * U * credited + 3 * U * Mterm)
    ssum = lambda v: torch.zeros((h.S, F), dtype=F64).index_add(0, h.col, v)
    b_gx = G2 * (ssum(dterm) + (h.indeg.double().unsqueeze(1) - 1).clamp(min=0) * U * ssum(Mterm))
    return (out.reshape(T, -1), b_out.reshape(T, -1), kmin, kmax, xd.grad, b_gx, ad.grad if ad is not None else None, b_ga)


def within(bad, what, got, ref, bound):
    ratio, where = A.worst(got, ref, bound, hop())
    print(f"AGG_STATS_RATIO {what}: {ratio:.3f}")
    if not ratio <= 1.0:
        bad.append(f"{what}: err/bound {ratio:.3f} at {where}")


@pytest.mark.parametrize("scalers", SCALERS, ids=["identity", "three_scalers"])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda v: str(v).split(".")[-1])
@pytest.mark.parametrize("F", [4, 128, 260])
def test_kernel_pair_against_float64(F, dtype, with_add, scalers):
    from salient_plusplus_amd import models as M
    h, ns = hop(), len(scalers)
    x, add, g = inputs(F, dtype, ns)
    add = add if with_add else None
    out_r, b_out, kmin, kmax, gx_r, b_gx, ga_r, b_ga = expected(x, add, g, scalers)
    dev = lambda t: t.cuda() if t is not None else None
    xd, rp, cl, args = dev(x), dev(h.rowptr), dev(h.col), (h.T, M._scaler_mask("test", scalers), DELTA, EPS)
    new = lambda *shape, dt=torch.float32: torch.full(shape, -77, dtype=dt, device="cuda")
    out, stats, pos = new(h.T, ns * 4 * F), new(h.T, 2 * F), new(h.T, 2 * F, dt=torch.int32)
    runs = []
    for _ in range(2):
        M._agg_stats_call("spp_agg_stats_forward", xd, rp, cl, *args, out_elem=M._ELEM[out.dtype], add_dev=dev(add),
                          out_dev=out, out_stride_elems=0, stats_dev=stats, pos_dev=pos)
        runs.append((out.clone(), stats.clone(), pos.clone()))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs)), "two runs, two results"
    gx, ga = torch.zeros((h.S, F), device="cuda"), new(h.T, F) if with_add else None
    M._agg_stats_call("spp_agg_stats_backward", xd, rp, cl, *args, grad_elem=M._ELEM[g.dtype], stats_dev=stats, pos_dev=pos,
                      grad_out_dev=dev(g), grad_out_stride_elems=0, grad_x_dev=gx, grad_add_dev=ga)
    torch.cuda.synchronize()
    bad = []
    if not (torch.equal(pos[:, :F].cpu().long(), kmin) and torch.equal(pos[:, F:].cpu().long(), kmax)):
        bad.append("kmin / kmax differ from the first occurrence")
    names = [f"{s}.{a}" for s in scalers for a in ("mean", "min", "max", "std")]
    for i, name in enumerate(names):                                       # identity.min / identity.max: bound 0, bit-exact
        cols = slice(i * F, (i + 1) * F)
        within(bad, "out " + name.split(".")[1] + ("" if name.startswith("identity") else " (scaled)"),
               out[:, cols], out_r[:, cols], b_out[:, cols])
    within(bad, "grad_x", gx, gx_r, b_gx)
    if with_add:
        within(bad, "grad_add", ga, ga_r, b_ga)
    assert bool((out[0] == 0).all()) and bool((pos[0] == -1).all()), "the empty row"
    assert not bad, bad


def test_bf16_output_under_autocast_and_degenerate_hops():
    from salient_plusplus_amd.models import stats_aggregate
    h = hop()
    x, add, g = inputs(128, torch.bfloat16, 3)
    out_r, b_out, *_ = expected(x, add, g, SCALERS[1])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = stats_aggregate(x.cuda(), h.rowptr.cuda(), h.col.cuda(), h.T, add=add.cuda(), scalers=SCALERS[1], delta=DELTA)
    assert out.dtype == torch.bfloat16
    bad = []
    within(bad, "out bf16", out, *A.rounded(out_r, b_out, torch.bfloat16))
    assert not bad, bad
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    for T, rowptr in ((0, torch.zeros(1, dtype=torch.int64)), (3, torch.zeros(4, dtype=torch.int64))):     # T == 0, E == 0
        xs = torch.randn((5, 8), device="cuda", requires_grad=True)
        ad = torch.randn((T, 8), device="cuda", requires_grad=True)
        out = stats_aggregate(xs, rowptr.cuda(), none, T, add=ad, scalers=SCALERS[1], delta=DELTA)
        out.sum().backward()
        assert out.shape == (T, 96) and not out.any() and not xs.grad.any() and not ad.grad.any()


def test_dispatch_between_the_kernels_and_the_reference(monkeypatch):
    from salient_plusplus_amd import models
    h, calls = hop(), []
    real = models._stats_reference
    monkeypatch.setattr(models, "_stats_reference", lambda *a, **k: calls.append(a[0].shape) or real(*a, **k))
    x = inputs(128, torch.float32, 1)[0]
    models.stats_aggregate(x, h.rowptr, h.col, h.T)                                  # CPU tensors
    models.stats_aggregate(x[:, :6].cuda(), h.rowptr.cuda(), h.col.cuda(), h.T)      # F % 4 != 0
    models.stats_aggregate(x.cuda()[:, 1:5], h.rowptr.cuda(), h.col.cuda(), h.T)     # rows not aligned to 4 elements
    assert len(calls) == 3
    models.stats_aggregate(x.cuda(), h.rowptr.cuda(), h.col.cuda(), h.T)
    assert len(calls) == 3


@pytest.mark.parametrize("what", ["layer", "model"])
def test_pna_step_against_float64(what, monkeypatch):
    """A PNAConv layer on the outer of two hops of a sampled batch (loss: the sum of squares), or a 2-layer PNA at hidden
    32 (nll, the dropout mask between the layers fixed): loss and every parameter gradient of the kernel path and of the
    same model on the SAME device sent to _stats_reference, against the model in float64 on the CPU.  Per tensor the
    distance is max|a - ref| / max|ref|; the kernel path may be up to 4x the reference path's (online sums and atomics
    against two-pass torch): test_gatv2_model_step_against_float64's margin.  The figures seen: DESIGN section 7 f4b."""
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor

    def fixed_dropout(x, p=0.5, training=True):
        mask = (torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(x.numel())) > p).to(x.dtype) / (1.0 - p)
        return torch.relu(x) * mask.to(x.device)

    monkeypatch.setattr(models, "relu_dropout", fixed_dropout)
    x, y, hops = gatv2_f64.sampled_batch(classes=8)
    hops = hops[1:]
    x = x[:hops[0][3]].contiguous()
    delta = models.pna_delta(hops[0][0])
    torch.manual_seed(1)
    model = (models.PNA(16, 32, 8, 2, delta=delta) if what == "model" else models.PNAConv(16, 32, delta=delta)).train()

    def step(m, dev, dtype):
        adjs = [(SparseTensor(rowptr=rp.to(dev), col=cl.to(dev), sparse_sizes=(T, S)), None, (S, T)) for rp, cl, T, S in hops]
        m.zero_grad()
        if what == "model":
            loss = torch.nn.functional.nll_loss(m(x.to(dev, dtype), adjs), y.to(dev))
        else:
            loss = m(x.to(dev, dtype), adjs[0][0], adjs[0][2]).square().sum()
        loss.backward()
        return [loss.detach().double().cpu()] + [p.grad.double().cpu() for p in m.parameters()]

    ref = step(copy.deepcopy(model).double(), "cpu", torch.float64)
    with monkeypatch.context() as mp:
        mp.setattr(models, "_stats_kernels_read", lambda *a: False)
        dev = step(copy.deepcopy(model).cuda(), "cuda", torch.float32)
    seen = []
    real = models._StatsAggregate.apply
    monkeypatch.setattr(models._StatsAggregate, "apply", staticmethod(lambda *a: seen.append(1) or real(*a)))
    gpu = step(copy.deepcopy(model).cuda(), "cuda", torch.float32)
    assert len(seen) == (2 if what == "model" else 1)
    bad = []
    for n, r, a, b in zip(["loss"] + [n for n, _ in model.named_parameters()], ref, dev, gpu):
        scale = float(r.abs().max())
        d_ref, d_ker = float((a - r).abs().max()) / scale, float((b - r).abs().max()) / scale
        print(f"PNA_STEP {what} {n}: reference path {d_ref:.3e} kernel path {d_ker:.3e}")
        if not d_ker <= 4 * d_ref:
            bad.append((n, d_ref, d_ker))
    assert not bad, bad
