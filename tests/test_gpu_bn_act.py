"""GPU: the f3p kernels (csrc/bn_act.hip; include/spp.h, spp_bn_act_forward / spp_bn_act_backward) against a float64
restatement of their contract, plain torch on the CPU, on the same fp32 input.

The margin of every comparison is measured, not chosen: torch's own fp32 path on the GPU (F.batch_norm, the activation,
the mask, autograd) is compared with the same float64 values, and the kernels may be off by at most TWICE torch's error
plus one fp32 ulp of the largest expected magnitude (two equally valid fp32 summation orders; the ulp covers the cases
where torch happens to be exact).  Every test prints both errors (BN_ACT_ERR lines).

Measured on an MI355X (890 comparisons): all within the margin; ratios kernel / torch 0.00-4.1, above 2 only where
torch's error is below one ulp of the largest value.

Shapes straddle the slab height R = SPP_BN_ACT_SLAB_ROWS and take C on both sides of the vector form (C % 4), of one
wave's 64 pieces (260) and of one lane per row (1, 3, 4)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = 1e-5
ACTS = {"none": 0, "relu": 1, "leaky_relu": 2}
SLOPE = 0.01


def _nat():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


def _R():
    return int(_nat()[1].spp_bn_act_slab_rows())


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _elem(t):
    return {F32: 0, BF16: 2}[t.dtype]


def _ws(n, Cd):
    nbytes = int(_nat()[1].spp_bn_act_workspace_bytes(n, Cd))
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def _forward(z, gamma, beta, *, act="none", slope=SLOPE, p=0.0, training=True, seed=0, momentum=0.1, rm=None, rv=None,
             nbt=None, r=None, y_dtype=None):
    """spp_bn_act_forward as it stands: (y, mean, invstd); rm / rv are updated in place"""
    nat, L = _nat()
    n, Cd = z.shape
    y = torch.full((n, Cd), float("nan"), dtype=y_dtype or z.dtype, device="cuda")
    mean = torch.full((Cd,), float("nan"), device="cuda")
    invstd = torch.full((Cd,), float("nan"), device="cuda")
    ws, nbytes = _ws(n, Cd)
    d = nat.BnActDesc(z_elem=_elem(z), r_elem=_elem(r) if r is not None else 0, y_elem=_elem(y), act=ACTS[act],
                      training=int(training), negative_slope=slope, p=p, eps=EPS,
                      momentum=-1.0 if momentum is None else momentum, seed=seed, n=n, C=Cd, z_dev=_P(z),
                      gamma_dev=_P(gamma), beta_dev=_P(beta), running_mean_dev=_P(rm), running_var_dev=_P(rv),
                      num_batches_tracked_dev=_P(nbt), r_dev=_P(r), y_dev=_P(y), mean_dev=_P(mean), invstd_dev=_P(invstd),
                      workspace_dev=_P(ws), workspace_bytes=nbytes)
    nat.check(L.spp_bn_act_forward(C.byref(d), _st()))
    return y, mean, invstd


def _backward(g, z, gamma, beta, mean, invstd, *, act="none", slope=SLOPE, p=0.0, training=True, seed=0):
    nat, L = _nat()
    n, Cd = z.shape
    dz = torch.full((n, Cd), float("nan"), dtype=z.dtype, device="cuda")
    dgamma = torch.full((Cd,), float("nan"), device="cuda")
    dbeta = torch.full((Cd,), float("nan"), device="cuda")
    ws, nbytes = _ws(n, Cd)
    d = nat.BnActDesc(z_elem=_elem(z), g_elem=_elem(g), act=ACTS[act], training=int(training), negative_slope=slope, p=p,
                      eps=EPS, seed=seed, n=n, C=Cd, z_dev=_P(z), gamma_dev=_P(gamma), beta_dev=_P(beta),
                      mean_dev=_P(mean), invstd_dev=_P(invstd), g_dev=_P(g), dz_dev=_P(dz), dgamma_dev=_P(dgamma),
                      dbeta_dev=_P(dbeta), workspace_dev=_P(ws), workspace_bytes=nbytes)
    nat.check(L.spp_bn_act_backward(C.byref(d), _st()))
    return dz, dgamma, dbeta


def _ulp(x):
    """one fp32 ulp at magnitude x"""
    return 0.0 if x == 0 else 2.0 ** (math.frexp(x)[1] - 1 - 23)


def _err(got, want64):
    return float((got.detach().double().cpu() - want64).abs().max()) if want64.numel() else 0.0


def _bounded(what, tag, got, torchs, want64):
    """the rule of this file: |got - want| <= 2 |torch - want| + ulp(max |want|); prints both errors"""
    ek, et = _err(got, want64), _err(torchs, want64)
    floor = _ulp(float(want64.abs().max())) if want64.numel() else 0.0
    print(f"BN_ACT_ERR {tag} {what}: kernel {ek:.3e} torch {et:.3e} ratio {ek / et if et else float('inf'):.2f} "
          f"ulp {floor:.3e}")
    assert ek <= 2 * et + floor, (tag, what, ek, et, floor)


def _act64(u, act, slope=SLOPE):
    return u if act == "none" else F.relu(u) if act == "relu" else F.leaky_relu(u, slope)


def _data(n, Cd, seed, loc=1.5, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn((n, Cd), generator=g) * scale + loc).float()
    gamma = torch.rand(Cd, generator=g) + 0.5
    beta = torch.randn(Cd, generator=g) * 0.5
    return z, gamma, beta


# ------------------------------------------------------------------------------------------ statistics, p = 0 output
def _shapes():
    R = SLAB
    return [(n, c) for n in (2, 3, 63, 65, R - 1, R, R + 1, 2 * R + 1) for c in (1, 3, 4, 47, 256, 260)]


# the header's constant, read without a device: the parametrisation needs it at collection time
SLAB = int(open(os.path.join(ROOT, "include", "spp.h")).read().split("#define SPP_BN_ACT_SLAB_ROWS ")[1].split()[0])
CASES = [(n, c, 1.5, 2.0) for n, c in _shapes()] + [(40000, 256, 1.5, 2.0), (4097, 8, 1e3, 0.1)]


@pytest.mark.parametrize("n,Cd,loc,scale", CASES, ids=[f"{n}x{c}" + ("-cancel" if loc > 100 else "") for n, c, loc, scale in CASES])
def test_statistics_output_and_buffers_against_float64(n, Cd, loc, scale):
    assert _R() == SLAB
    z, gamma, beta = _data(n, Cd, n * 1000 + Cd, loc, scale)
    tag = f"[{n}x{Cd}]"
    z64, g64, b64 = z.double(), gamma.double(), beta.double()
    mean64, var64 = z64.mean(0), z64.var(0, unbiased=False)
    invstd64 = 1.0 / torch.sqrt(var64 + EPS)
    unb64 = var64 * n / (n - 1)
    zc, gc, bc = z.cuda(), gamma.cuda(), beta.cuda()
    # torch's own fp32 statistics
    _, t_mean, t_invstd = torch.native_batch_norm(zc, gc, bc, None, None, True, 0.0, EPS)
    for act in ("relu", "leaky_relu"):
        want = _act64((z64 - mean64) * invstd64 * g64 + b64, act)
        y, mean, invstd = _forward(zc, gc, bc, act=act)
        ty = _act64(F.batch_norm(zc, None, None, gc, bc, True, 0.0, EPS), act)
        _bounded(f"y {act}", tag, y, ty, want)
    _bounded("mean", tag, mean, t_mean, mean64)
    _bounded("invstd", tag, invstd, t_invstd, invstd64)
    # var itself, through the unbiased running variance at momentum 1 from zeroed buffers
    rm, rv = torch.zeros(Cd, device="cuda"), torch.zeros(Cd, device="cuda")
    trm, trv = torch.zeros(Cd, device="cuda"), torch.zeros(Cd, device="cuda")
    _forward(zc, gc, bc, momentum=1.0, rm=rm, rv=rv)
    F.batch_norm(zc, trm, trv, gc, bc, True, 1.0, EPS)
    _bounded("var", tag, rv.double() * (n - 1) / n, trv.double() * (n - 1) / n, var64)
    # the buffers, momentum 0.1 and the cumulative average (third batch: factor 1/3)
    g = torch.Generator().manual_seed(5)
    rm0, rv0 = torch.randn(Cd, generator=g), torch.rand(Cd, generator=g) + 0.5
    for momentum, f in ((0.1, 0.1), (None, 1.0 / 3.0)):
        rm, rv, trm, trv = rm0.cuda(), rv0.cuda(), rm0.cuda(), rv0.cuda()
        nbt = torch.tensor(3, dtype=torch.int64, device="cuda")
        _forward(zc, gc, bc, momentum=momentum, rm=rm, rv=rv, nbt=nbt)
        F.batch_norm(zc, trm, trv, gc, bc, True, f, EPS)
        assert int(nbt) == 3                                  # read, never written: the caller counts
        _bounded(f"running_mean m={momentum}", tag, rm, trm, (1 - f) * rm0.double() + f * mean64)
        _bounded(f"running_var m={momentum}", tag, rv, trv, (1 - f) * rv0.double() + f * unb64)


def test_sum_of_squares_statistics_fail_the_cancellation_case():
    """what the case above is for: var = E[z^2] - E[z]^2 in fp32 misses it by orders of magnitude"""
    z, _, _ = _data(4097, 8, 4097008, 1e3, 0.1)
    var64 = z.double().var(0, unbiased=False)
    zc = z.cuda()
    naive = (zc * zc).mean(0) - zc.mean(0) ** 2
    t_var = zc.var(0, unbiased=False)
    assert _err(naive, var64) > 100 * (2 * _err(t_var, var64) + _ulp(float(var64.max())))


@pytest.mark.parametrize("momentum", [0.1, None])
def test_module_buffers_and_num_batches_tracked(momentum):
    """through models.batch_norm_act: num_batches_tracked exact, the buffers as torch.nn.BatchNorm1d leaves them"""
    from salient_plusplus_amd.models import batch_norm_act
    n, Cd = 2 * SLAB + 1, 47
    bn = torch.nn.BatchNorm1d(Cd, momentum=momentum).cuda()
    ref = torch.nn.BatchNorm1d(Cd, momentum=momentum).cuda()
    bn64 = torch.nn.BatchNorm1d(Cd, momentum=momentum).double()
    for step in range(3):
        z = _data(n, Cd, step)[0]
        batch_norm_act(z.cuda(), bn, act="relu")
        ref(z.cuda())
        bn64(z.double())
        assert int(bn.num_batches_tracked) == step + 1 == int(ref.num_batches_tracked)
        assert bn.num_batches_tracked.dtype == torch.int64
    _bounded(f"module running_mean m={momentum}", "[3 steps]", bn.running_mean, ref.running_mean, bn64.running_mean)
    _bounded(f"module running_var m={momentum}", "[3 steps]", bn.running_var, ref.running_var, bn64.running_var)
    bn.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    batch_norm_act(z.cuda(), bn, act="relu")
    assert int(bn.num_batches_tracked) == 3 and torch.equal(before[0], bn.running_mean) and torch.equal(before[1], bn.running_var)


@pytest.mark.parametrize("n,Cd", [(3, 4), (65, 47), (SLAB + 1, 260), (1000, 256)])
def test_eval_forward_uses_the_running_statistics(n, Cd):
    z, gamma, beta = _data(n, Cd, 77 + n)
    g = torch.Generator().manual_seed(6)
    rm0, rv0 = torch.randn(Cd, generator=g) + 1.5, torch.rand(Cd, generator=g) * 4 + 0.5
    rm, rv = rm0.cuda(), rv0.cuda()
    y, mean, invstd = _forward(z.cuda(), gamma.cuda(), beta.cuda(), act="leaky_relu", training=False, p=0.5, seed=9, rm=rm, rv=rv)
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and torch.equal(mean.cpu(), rm0)
    inv64 = 1.0 / torch.sqrt(rv0.double() + EPS)
    want = _act64((z.double() - rm0.double()) * inv64 * gamma.double() + beta.double(), "leaky_relu")
    ty = F.leaky_relu(F.batch_norm(z.cuda(), rm, rv, gamma.cuda(), beta.cuda(), False, 0.0, EPS), SLOPE)
    _bounded("eval y", f"[{n}x{Cd}]", y, ty, want)            # no dropout in eval: p and the seed are not read
    assert _err(invstd, inv64) <= _ulp(float(inv64.max()))


# ------------------------------------------------------------------------------------------ dropout
def _relu_dropout_keep(total, p, seed):
    nat, L = _nat()
    ones = torch.ones(total, device="cuda")
    out = torch.empty_like(ones)
    nat.check(L.spp_relu_dropout_forward(_P(ones), total, p, 1, seed, _P(out), _st()))
    return out != 0


def _mask(zc, p, seed):
    """the keep pattern of the forward at (seed, p): act none, gamma = 0, beta = 1 gives y = keep / (1 - p)"""
    Cd = zc.size(1)
    y, _, _ = _forward(zc, torch.zeros(Cd, device="cuda"), torch.ones(Cd, device="cuda"), act="none", p=p, seed=seed)
    scale = torch.tensor(1.0 / (1.0 - p)).float().item()
    assert bool(((y == 0) | (y == scale)).all())
    return y != 0


@pytest.mark.parametrize("n,Cd", [(2, 4), (65, 47), (SLAB + 1, 260), (63, 3), (1000, 256), (3, 1), (7, 3)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_pattern_is_the_relu_dropout_generators(n, Cd, p):
    z, gamma, beta = _data(n, Cd, 3)
    seed = 0x9E3779B97F4A7C15 ^ (n * Cd)
    zc = z.cuda()
    mask = _mask(zc, p, seed)
    # the elements spp_relu_dropout_forward keeps of n * C positive values (any n * C: its tail rule included)
    assert torch.equal(mask.reshape(-1), _relu_dropout_keep(n * Cd, p, seed))
    # and a real forward drops exactly those: y == 0 off the mask, the p = 0 output times 1 / (1 - p) on it
    y, _, _ = _forward(zc, gamma.cuda(), beta.cuda(), act="none", p=p, seed=seed)
    y0, _, _ = _forward(zc, gamma.cuda(), beta.cuda(), act="none", p=0.0, seed=seed)
    scale = torch.tensor(1.0 / (1.0 - p)).float().cuda()
    assert torch.equal(y, torch.where(mask, y0 * scale, torch.zeros_like(y0)))
    assert not torch.equal(mask, _mask(zc, p, seed + 1)) or n * Cd < 8


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction_is_binomial(p):
    n, Cd = 40000, 256
    zc = torch.zeros((n, Cd), device="cuda")
    kept = int(_mask(zc, p, 12345).sum())
    N = n * Cd
    sigma = math.sqrt(N * p * (1 - p))
    print(f"BN_ACT_KEEP p={p}: kept {kept} of {N}, expected {N * (1 - p):.0f}, {abs(kept - N * (1 - p)) / sigma:.2f} sigma")
    assert abs(kept - N * (1 - p)) <= 5 * sigma
    # p = 0 keeps everything, without the generator
    y, _, _ = _forward(zc[:1000], torch.zeros(Cd, device="cuda"), torch.ones(Cd, device="cuda"), p=0.0, seed=1)
    assert bool((y == 1).all())


# ------------------------------------------------------------------------------------------ backward
def _beta_without_ties(xh64, gamma64, gen):
    """beta per column such that no u = gamma * xh + beta lies within 1e-3 of 0: -beta / gamma sits in the middle of
    the widest gap between neighbouring xh of the column's central 80 %"""
    n, Cd = xh64.shape
    s, _ = torch.sort(xh64, dim=0)
    lo, hi = max(0, n // 10), max(2, n - n // 10)
    gaps = s[lo + 1:hi] - s[lo:hi - 1]
    if gaps.numel() == 0:
        return torch.full((Cd,), 3.0, dtype=F64) * gamma64.abs() + 1.0       # every u > 0
    k = gaps.argmax(0)
    mid = (s[lo:hi - 1].gather(0, k[None]) + s[lo + 1:hi].gather(0, k[None]))[0] / 2
    return -gamma64 * mid


BWD_SHAPES = [(65, 47), (2 * SLAB + 1, 260), (1000, 256), (3, 4)]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("with_r", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("act", ["relu", "leaky_relu", "none"])
def test_backward_against_float64_autograd(act, p, with_r, training):
    from salient_plusplus_amd.models import batch_norm_act
    for n, Cd in BWD_SHAPES:
        tag = f"[{n}x{Cd} {act} p={p} {'res' if with_r else 'nores'} {'train' if training else 'eval'}]"
        gen = torch.Generator().manual_seed(n + Cd)
        z, gamma, _ = _data(n, Cd, n + 7 * Cd)
        rm0, rv0 = torch.randn(Cd, generator=gen) * 0.3 + 1.5, torch.rand(Cd, generator=gen) * 4 + 1.0
        z64 = z.double()
        if training:
            mean64, var64 = z64.mean(0), z64.var(0, unbiased=False)
        else:
            mean64, var64 = rm0.double(), rv0.double()
        xh64 = (z64 - mean64) / torch.sqrt(var64 + EPS)
        beta = _beta_without_ties(xh64, gamma.double(), gen).float()
        u64 = xh64 * gamma.double() + beta.double()
        assert float(u64.abs().min()) > 1e-3, tag              # no sign ties: act' is unambiguous
        r = torch.randn((n, Cd), generator=gen) if with_r else None
        w = torch.randn((n, Cd), generator=gen)
        # the kernels, through the autograd node
        bn = torch.nn.BatchNorm1d(Cd, eps=EPS).cuda()
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
        zk = z.cuda().requires_grad_(True)
        rk = r.cuda().requires_grad_(True) if with_r else None
        torch.manual_seed(n)
        y = batch_norm_act(zk, bn, act=act, negative_slope=SLOPE, p=p, training=training, residual=rk)
        assert y.grad_fn is not None and type(y.grad_fn).__name__ == "_BatchNormActBackward"
        (y * w.cuda()).sum().backward()
        # the mask of that forward: the same seed drawn again, gamma = 0, beta = 1
        if training and p > 0:
            ones = torch.nn.BatchNorm1d(Cd, eps=EPS).cuda()
            with torch.no_grad():
                ones.weight.zero_(), ones.bias.fill_(1.0)
            torch.manual_seed(n)
            mask = (batch_norm_act(z.cuda(), ones, act="none", p=p, training=True) != 0).cpu()
            keep = 1.0 / (1.0 - p)
        else:
            mask, keep = torch.ones((n, Cd), dtype=torch.bool), 1.0

        def restate(dt, dev):
            zz = z.to(dev, dt).requires_grad_(True)
            gg, bb = gamma.to(dev, dt).requires_grad_(True), beta.to(dev, dt).requires_grad_(True)
            rr = r.to(dev, dt).requires_grad_(True) if with_r else None
            h = F.batch_norm(zz, rm0.to(dev, dt), rv0.to(dev, dt), gg, bb, training, 0.1, EPS)
            out = _act64(h, act) * mask.to(dev, dt) * keep
            out = out + rr if with_r else out
            (out * w.to(dev, dt)).sum().backward()
            return out.detach(), zz.grad, gg.grad, bb.grad, rr.grad if with_r else None

        want, tor = restate(F64, "cpu"), restate(F32, "cuda")
        got = (y.detach(), zk.grad, bn.weight.grad, bn.bias.grad, rk.grad if with_r else None)
        for name, a, t, e in zip(("y", "dz", "dgamma", "dbeta", "dr"), got, tor, want):
            if e is not None:
                _bounded(name, tag, a, t, e)
        if with_r:
            assert torch.equal(rk.grad, w.cuda())             # the residual's gradient is g itself


# ------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("n,Cd", [(65, 47), (2 * SLAB + 1, 260), (1000, 256)])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bf16_is_exact_upcast_and_one_rounding(n, Cd, training):
    z, gamma, beta = _data(n, Cd, 31 + n)
    g = torch.Generator().manual_seed(8)
    zb = z.cuda().to(BF16)
    rb = torch.randn((n, Cd), generator=g).cuda().to(BF16)
    gb = torch.randn((n, Cd), generator=g).cuda().to(BF16)
    gc, bc = gamma.cuda(), beta.cuda()
    rm0, rv0 = torch.randn(Cd, generator=g).cuda(), (torch.rand(Cd, generator=g) + 0.5).cuda()
    kw = dict(act="leaky_relu", p=0.1, seed=77, training=training)
    outs = {}
    for name, zz, rr, ydt in (("f32", zb.float(), rb.float(), F32), ("bf16->f32", zb, rb, F32), ("bf16->bf16", zb, rb, BF16),
                              ("mixed", zb, rb.float(), F32), ("f32->bf16", zb.float(), rb.float(), BF16)):
        rm, rv = rm0.clone(), rv0.clone()
        outs[name] = _forward(zz, gc, bc, rm=rm, rv=rv, r=rr, y_dtype=ydt, **kw) + (rm, rv)
    ref = outs["f32"]
    for name, o in outs.items():
        assert all(torch.equal(a, b) for a, b in zip(o[1:], ref[1:])), name     # mean, invstd, buffers: the same bits
        assert torch.equal(o[0], ref[0] if o[0].dtype == F32 else ref[0].to(BF16)), name
    _, mean, invstd = ref[:3]
    dref = _backward(gb.float(), zb.float(), gc, bc, mean, invstd, **kw)
    for zz, gg in ((zb, gb), (zb, gb.float()), (zb.float(), gb)):
        dz, dgamma, dbeta = _backward(gg, zz, gc, bc, mean, invstd, **kw)
        assert dz.dtype == zz.dtype and torch.equal(dz, dref[0].to(zz.dtype))
        assert torch.equal(dgamma, dref[1]) and torch.equal(dbeta, dref[2])


def test_unaligned_bases_take_the_scalar_form_with_the_same_bits():
    """C % 4 == 0 but a base off the 16-byte grid: the one-column form, workgroup-uniformly, the same result"""
    n, Cd = SLAB + 3, 8
    z, gamma, beta = _data(n, Cd, 1)
    buf = torch.zeros(n * Cd + 1, device="cuda")
    buf[1:] = z.cuda().reshape(-1)
    zu = buf[1:].view(n, Cd)
    assert zu.data_ptr() % 16 == 4
    kw = dict(act="relu", p=0.5, seed=5)
    a = _forward(z.cuda(), gamma.cuda(), beta.cuda(), **kw)
    b = _forward(zu, gamma.cuda(), beta.cuda(), **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    g = torch.randn((n, Cd), device="cuda")
    da = _backward(g, z.cuda(), gamma.cuda(), beta.cuda(), a[1], a[2], **kw)
    db = _backward(g, zu, gamma.cuda(), beta.cuda(), a[1], a[2], **kw)
    assert all(torch.equal(x, y) for x, y in zip(da, db))


# ------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("n,Cd", [(2 * SLAB + 1, 47), (40000, 256)])
def test_two_runs_are_bit_identical(n, Cd):
    z, gamma, beta = _data(n, Cd, 2)
    zc, gc, bc = z.cuda(), gamma.cuda(), beta.cuda()
    g = torch.randn((n, Cd), device="cuda")
    kw = dict(act="leaky_relu", p=0.1, seed=3)
    runs = []
    for _ in range(2):
        y, mean, invstd = _forward(zc, gc, bc, **kw)
        runs.append((y, mean, invstd) + _backward(g, zc, gc, bc, mean, invstd, **kw))
        torch.empty(1 << 20, device="cuda").normal_()          # other work in between
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(bool(torch.isfinite(a).all()) for a in runs[0])
