"""-m gpu: the GATv2 kernels (csrc/gatv2.hip: spp_gatv2_forward, spp_gatv2_backward) against the float64 restatement and
the per-element bounds of tests/gatv2_f64.py, element by element, on gat_f64's planted hop and the logit regimes of
gatv2_f64.inputs; then GATv2Conv and a 2-layer GATv2 on the device.  Each test prints the largest err / bound per output
quantity (GATV2_F64_RATIO lines): a record, not an input to the bounds.

Seen on an MI355X: the docstring of test_zz_largest_ratios_seen."""
import collections
import copy
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gatv2_f64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
WIDTHS = [(1, 4), (1, 64), (4, 16), (8, 8), (8, 128)]       # (H, C) the entries accept; (8, 128): D = 1024
REFUSED = [(2, 12), (4, 260)]                               # C / 4 not a power of two; that and D > 1024
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SEEN = collections.defaultdict(float)


def _call(name, desc):
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.models import _stream
    return getattr(nat.load(), name)(C.byref(desc), _stream())


class Run:
    """both entries on one hop; x_l [S, H, C] and x_r [T, H, C] on the device (x_r may be a view of x_l)"""

    def __init__(self, hop, x_l, x_r, att, slope):
        self.hop, self.slope = hop, slope
        self.H, self.C = att.shape
        self.x_l, self.x_r = x_l.view(hop.S, self.H * self.C), x_r.view(hop.T, self.H * self.C)
        self.att = att.cuda()
        self.rowptr, self.col = hop.rowptr.cuda(), hop.col.cuda()

    def _f(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device="cuda")

    def _desc(self, out, rmax, rsum, **grads):
        from salient_plusplus_amd.models import _gatv2_desc
        return _gatv2_desc(self.x_l, self.x_r, self.att, self.rowptr, self.col, self.slope, out, rmax, rsum, **grads)

    def forward(self):
        T, H, Cc = self.hop.T, self.H, self.C
        out, rmax, rsum = self._f(T, H, Cc), self._f(T, H), self._f(T, H)
        assert _call("spp_gatv2_forward", self._desc(out, rmax, rsum)) == 0
        return out, rmax, rsum

    def backward(self, out, rmax, rsum, g, want_gxl=True):
        T, S, H, Cc = self.hop.T, self.hop.S, self.H, self.C
        gxl = self._f(S, H, Cc, zero=True) if want_gxl else None
        gxr = torch.full((T, H, Cc), float("nan"), device="cuda")
        gatt = torch.full((H, Cc), float("nan"), device="cuda")
        d = self._desc(out, rmax, rsum, grad_out_dev=g, grad_x_l_dev=gxl, grad_x_r_dev=gxr, grad_att_dev=gatt)
        assert _call("spp_gatv2_backward", d) == 0
        return gxl, gxr, gatt


class Checks:
    def __init__(self, hop):
        self.hop, self.tag, self.bad, self.top = hop, "", [], collections.defaultdict(float)

    def within(self, what, got, ref, bound):
        assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
        ratio, where = G.worst(got, ref, bound, self.hop)
        self.top[what] = max(self.top[what], ratio)
        SEEN[what] = max(SEEN[what], ratio)
        if not ratio <= 1.0:
            self.bad.append(f"{what} [{self.tag}] err/bound {ratio:.3f} at {where}")

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what} [{self.tag}] is not exact")

    def done(self):
        print("\nGATV2_F64_RATIO " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.top.items())))
        assert not self.bad, "\n".join(self.bad)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def pipeline(c, hop, name, H, Cc, dtype, alias, slope):
    c.tag = f"{name} slope {slope:.3g} {'aliased' if alias else 'distinct'}"
    x_l, x_r, att, g = G.inputs(name, hop, H, Cc, dtype)
    xl_d = x_l.cuda()
    if alias:                                                   # share_weights: x_r IS x_l[:T]
        x_r, xr_d = x_l[:hop.T], xl_d[:hop.T]
    else:
        xr_d = x_r.cuda()
    r = Run(hop, xl_d, xr_d, att, slope)
    out, rmax, rsum = r.forward()
    out2, rmax2, rsum2 = r.forward()
    c.exact("two forward runs", _same(out, out2) and _same(rmax, rmax2) and _same(rsum, rsum2))
    bw = G.backward(hop, x_l, x_r, att, g, slope)
    fw = bw.fw
    c.within("out", out, fw.out, fw.b_out)
    c.within("row_sum", rsum, fw.row_sum, fw.bs)
    c.within("row_max", rmax, fw.row_max, fw.bm)
    lone = hop.kept == 0                                        # alpha = 1: x_l[i] exactly
    c.exact("out of a target with no kept entry", torch.equal(out.cpu()[lone], x_l.float()[:hop.T][lone]))
    unnamed = hop.named == 0
    for want_gxl in (True, False):
        gxl, gxr, gatt = r.backward(out, rmax, rsum, g.cuda(), want_gxl)
        form = "" if want_gxl else "/no grad_xl"
        c.within("grad_xr" + form, gxr, bw.gxr, bw.b_gxr)
        c.within("grad_att" + form, gatt, bw.gatt, bw.b_gatt)
        if want_gxl:
            c.within("grad_xl", gxl, bw.gxl, bw.b_gxl)
            c.exact("grad_xl of unnamed sources", bool((gxl.cpu()[unnamed] == 0).all()))
    for t in (out, rsum, gxr, gatt):
        c.exact("finite", bool(torch.isfinite(t).all()))


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "aliased"])
@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("H,Cc", WIDTHS)
def test_both_entries_within_their_bounds_on_the_planted_hop(H, Cc, dtype, alias):
    """every regime at the slope the models use (float32(0.2)); three of them again at 0.25; the square hop at the
    narrowest and the widest instance"""
    hop = G.planted_hop(70, 70 if (H, Cc) in ((1, 4), (8, 128)) else 200)
    c = Checks(hop)
    for name in G.REGIMES:
        pipeline(c, hop, name, H, Cc, dtype, alias, G.SLOPES[0])
    for name in ("model", "zero", "wide"):
        pipeline(c, hop, name, H, Cc, dtype, alias, G.SLOPES[1])
    c.done()


@pytest.mark.parametrize("H,Cc", [(1, 64), (4, 16), (2, 256)])
def test_the_other_hop_and_a_head_of_several_steps(H, Cc):
    """the square hop where the first test takes (70, 200) and the other way round; (2, 256): a head of four backward
    steps, and two forward chunks per lane"""
    hop = G.planted_hop(70, 70 if Cc != 256 else 200)
    c = Checks(hop)
    for name in ("model", "ascending", "zero"):
        pipeline(c, hop, name, H, Cc, torch.float32, False, G.SLOPES[0])
    c.done()


@pytest.mark.parametrize("H,Cc", [(1, 4), (4, 16), (8, 128)])
def test_smallest_hops(H, Cc):
    none = torch.zeros(0, dtype=torch.int64)
    big = G.planted_hop(70, 200)
    # T = 0: nothing is written, grad_att is zeroed
    hop = G.Hop(torch.zeros(1, dtype=torch.int64), none, 0, 3)
    x_l, x_r, att, g = G.inputs("model", hop, H, Cc, torch.float32)
    r = Run(hop, x_l.cuda(), x_r.cuda(), att, G.SLOPES[0])
    out, rmax, rsum = r.forward()
    gxl, gxr, gatt = r.backward(out, rmax, rsum, g.cuda())
    assert out.shape == (0, H, Cc) and bool((gxl == 0).all()) and bool((gatt == 0).all())
    # T = 1 with a row of 130 entries
    one, _perm = big.one_row(69)
    c = Checks(one)
    pipeline(c, one, "model", H, Cc, torch.float32, False, G.SLOPES[0])
    pipeline(c, one, "zero", H, Cc, torch.bfloat16, True, G.SLOPES[0])
    # E = 0 with T = 70: every target is alone with its self loop
    hop = G.Hop(torch.zeros(71, dtype=torch.int64), none, 70, 200)
    pipeline(c, hop, "model", H, Cc, torch.float32, False, G.SLOPES[0])
    x_l, x_r, att, g = G.inputs("model", hop, H, Cc, torch.float32)
    out, rmax, rsum = Run(hop, x_l.cuda(), x_r.cuda(), att, G.SLOPES[0]).forward()
    assert torch.equal(out.cpu(), x_l[:70]) and bool((rsum == 1).all())
    c.done()


def _adj(hop):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    return SparseTensor(rowptr=hop.rowptr.cuda(), col=hop.col.cuda(), sparse_sizes=(hop.T, hop.S))


def _count(monkeypatch):
    from salient_plusplus_amd import models
    calls = []
    orig = models._GATv2Layer.apply
    monkeypatch.setattr(models._GATv2Layer, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    return calls


def _layer(monkeypatch, hop, H, Cc, concat, bias, share, amp, kernels):
    """GATv2Conv on the device against the float64 layer evaluated on the rows the layer itself projected (captured
    from lin_l / lin_r: fp32, or bf16 under autocast -- converted exactly, so the kernel-level bounds hold unchanged)"""
    from salient_plusplus_amd.models import GATv2Conv
    calls = _count(monkeypatch)
    torch.manual_seed(H * 100 + Cc)
    T, S, K = hop.T, hop.S, 12
    conv = GATv2Conv(K, Cc, heads=H, concat=concat, bias=bias, share_weights=share).cuda()
    if bias:
        torch.nn.init.normal_(conv.bias)
        torch.nn.init.normal_(conv.lin_l.bias)
    x = torch.randn(S, K).cuda()
    kept = {}

    def keep(key):
        return lambda m, i, o: (o.retain_grad(), kept.__setitem__(key, o))[0]

    hooks = [conv.lin_l.register_forward_hook(keep("x_l"))]
    if not share:
        hooks.append(conv.lin_r.register_forward_hook(keep("x_r")))
    g = torch.randn(T, H * Cc if concat else Cc)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = conv((x, x[:T]), _adj(hop))
    for h in hooks:
        h.remove()
    out.backward(g.cuda())
    assert len(calls) == (1 if kernels else 0) and out.dtype == torch.float32
    x_l = kept["x_l"].detach().cpu().view(S, H, Cc)
    assert x_l.dtype == (torch.bfloat16 if amp else torch.float32)
    x_r = x_l[:T] if share else kept["x_r"].detach().cpu().view(T, H, Cc)
    att = conv.att.detach().cpu().view(H, Cc)
    g_out = g.view(T, H, Cc) if concat else (g / H).unsqueeze(1).expand(T, H, Cc)      # (g / H: exact, H a power of two)
    bw = G.backward(hop, x_l, x_r, att, g_out, conv.negative_slope)
    ref, b_out, cast = G.layer_bounds(bw, concat, conv.bias.detach().cpu() if bias else None, x_l.dtype)
    c = Checks(hop)
    c.tag = f"H {H} C {Cc} concat {concat} bias {bias} share {share} amp {amp}"
    c.within("layer out", out.detach(), ref, b_out)
    c.within("layer grad_att", conv.att.grad.view(H, Cc), bw.gatt, bw.b_gatt)
    gl = kept["x_l"].grad.view(S, H, Cc)
    if share:                                                   # autograd sums grad_xl and grad_xr through the view
        pad = torch.zeros_like(bw.gxl)
        pad[:T] = bw.gxr
        bpad = torch.zeros_like(bw.b_gxl)
        bpad[:T] = bw.b_gxr
        ref_l = bw.gxl + pad
        b_l = G.G2 * (bw.b_gxl + bpad + cast * (bw.gxl.abs() + pad.abs()) + max(cast, G.U) * ref_l.abs())
        c.within("layer grad_xl + grad_xr", gl, ref_l, b_l)
    else:
        c.within("layer grad_xl", gl, bw.gxl, G.G2 * (bw.b_gxl + cast * bw.gxl.abs()))
        c.within("layer grad_xr", kept["x_r"].grad.view(T, H, Cc), bw.gxr, G.G2 * (bw.b_gxr + cast * bw.gxr.abs()))
    assert x.grad is None and conv.lin_l.weight.grad is not None and bool(torch.isfinite(conv.lin_l.weight.grad).all())
    c.done()


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast_bf16"])
@pytest.mark.parametrize("share", [False, True], ids=["two_maps", "share_weights"])
@pytest.mark.parametrize("concat,bias", [(True, True), (False, False), (False, True)])
def test_gatv2conv_on_the_kernels(concat, bias, share, amp, monkeypatch):
    _layer(monkeypatch, G.planted_hop(70, 200), 4, 16, concat, bias, share, amp, kernels=True)


@pytest.mark.parametrize("H,Cc", REFUSED)
def test_refused_widths_take_the_reference_path(H, Cc, monkeypatch):
    """spp.h f3v: C / 4 not a power of two and D > 1024 are refused by the entries; GATv2Conv still answers"""
    hop = G.planted_hop(70, 200)
    x_l, x_r, att, _g = G.inputs("model", hop, H, Cc, torch.float32)
    r = Run(hop, x_l.cuda(), x_r.cuda(), att, G.SLOPES[0])
    from salient_plusplus_amd import _native as nat
    out, rmax, rsum = r._f(hop.T, H, Cc), r._f(hop.T, H), r._f(hop.T, H)
    assert _call("spp_gatv2_forward", r._desc(out, rmax, rsum)) == -1
    assert "power of two" in nat.load().spp_last_error().decode()   # checked before D (D > 1024 alone: the host test)
    assert _call("spp_gatv2_backward", r._desc(out, rmax, rsum, grad_out_dev=out, grad_x_r_dev=out, grad_att_dev=out)) == -1
    _layer(monkeypatch, hop, H, Cc, True, True, False, False, kernels=False)


def test_gatv2_model_step_against_float64(monkeypatch):
    """A 2-layer GATv2(heads=4), one training step (nll loss, backward) on the two inner hops of a three-hop sampled
    batch, with the dropout mask between the layers fixed: loss and every parameter gradient of the kernel path, and of
    the fp32 reference path, against the same model in float64 (on the CPU).  Per tensor the distance is
    max|a - ref| / max|ref|; the kernel path may be up to 4x the reference path's (online against two-pass softmax,
    atomics).

    The reference path is the same model on the SAME device with GATv2Conv sent to _gatv2_reference, so that the two
    fp32 runs differ in the message passing alone.  The first version of this test ran it on the CPU and failed on the
    loss (1.503e-08 against 7.948e-08, ratio 5.29): measured over four batches, the reference path on the device gives
    the kernel path's loss bit for bit (2.52275467 both, the CPU 2.52275491; float64 2.52275487), so that difference was
    the device's GEMM / log_softmax against the CPU's, one ulp of one scalar, and none of it the kernels'.  The CPU
    run's distances are still printed.

    Measured on an MI355X (reference path on the device / kernel path / ratio; CPU reference path in brackets):
        loss                  7.948e-08  7.948e-08  1.00   (1.503e-08)
        convs.0.att           2.006e-07  2.085e-07  1.04   (2.268e-07)
        convs.0.lin_l.weight  3.130e-07  2.479e-07  0.79   (2.282e-07)
        convs.0.lin_r.weight  1.857e-07  3.472e-07  1.87   (2.801e-07)
        convs.1.att           2.277e-07  2.456e-07  1.08   (2.882e-07)
        convs.1.lin_l.weight  1.188e-07  1.632e-07  1.37   (1.240e-07)
        convs.1.lin_r.weight  2.467e-07  3.946e-07  1.60   (1.778e-07)
    (With __expf in the kernels, as the GAT kernels have it, the kernel path's convs.0.att / lin_r.weight /
    convs.1.lin_r.weight stood at 8.555e-07 / 1.275e-06 / 5.896e-07, up to 6.9x these reference figures: the kernels
    take expf for that reason.)"""
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    calls = _count(monkeypatch)

    def fixed_dropout(x, p=0.5, training=True):
        gen = torch.Generator().manual_seed(x.numel())
        mask = (torch.rand(tuple(x.shape), generator=gen) > p).to(x.dtype) / (1.0 - p)
        return torch.relu(x) * mask.to(x.device)

    monkeypatch.setattr(models, "relu_dropout", fixed_dropout)
    x, y, hops = G.sampled_batch(classes=8)
    hops = hops[1:]
    x = x[:hops[0][3]].contiguous()
    torch.manual_seed(1)
    model = models.GATv2(16, 32, 8, 2, heads=4).train()

    def step(m, dev, dtype):
        adjs = [(SparseTensor(rowptr=rp.to(dev), col=cl.to(dev), sparse_sizes=(T, S)), None, (S, T)) for rp, cl, T, S in hops]
        m.zero_grad()
        loss = torch.nn.functional.nll_loss(m(x.to(dev, dtype), adjs), y.to(dev))
        loss.backward()
        return [loss.detach().double().cpu()] + [p.grad.double().cpu() for p in m.parameters()]

    ref = step(copy.deepcopy(model).double(), "cpu", torch.float64)
    cpu = step(copy.deepcopy(model), "cpu", torch.float32)
    with monkeypatch.context() as mp:                           # the reference path on the device
        mp.setattr(models, "_gatv2_kernels_read", lambda *a: False)
        dev = step(copy.deepcopy(model).cuda(), "cuda", torch.float32)
    assert not calls
    gpu = step(copy.deepcopy(model).cuda(), "cuda", torch.float32)
    assert len(calls) == 2
    names = ["loss"] + [n for n, _ in model.named_parameters()]
    bad = []
    for n, r, a, b, c in zip(names, ref, dev, gpu, cpu):
        scale = float(r.abs().max())
        d_ref, d_ker = float((a - r).abs().max()) / scale, float((b - r).abs().max()) / scale
        print(f"GATV2_MODEL {n}: reference path {d_ref:.3e} kernel path {d_ker:.3e} ratio {d_ker / d_ref if d_ref else float('inf'):.2f}"
              f" (reference path on the CPU {float((c - r).abs().max()) / scale:.3e})")
        if not d_ker <= 4 * d_ref:
            bad.append((n, d_ref, d_ker))
    assert not bad, bad


def test_zz_largest_ratios_seen():
    """prints the largest err / bound per output quantity over the tests of this module that ran before it.

    Seen on an MI355X (a record, not an input to the bounds): out 0.20, row_max 0.35, row_sum 0.17, grad_xl 0.13 (0.27
    with __expf), grad_xr 0.07, grad_att 0.005, with and without grad_xl alike; at layer level out 0.21, grad_att 0.001,
    and under bf16 autocast grad_xl 0.99, grad_xr 0.95, their sum through the share_weights view 0.85 -- there the bound
    is almost entirely the cast back to bf16 (2^-8 |value|), which a round-to-nearest cast meets nearly in full."""
    print("\nGATV2_F64_LARGEST " + " ".join(f"{k}={v:.3f}" for k, v in sorted(SEEN.items())))
