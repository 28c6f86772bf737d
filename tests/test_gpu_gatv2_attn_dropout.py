"""-m gpu: attention dropout of the GATv2 kernels (spp.h f3x; csrc/gatv2.hip k_gatv2_fwd / k_gatv2_bwd with kDrop, through
spp_gatv2_forward_drop / spp_gatv2_backward_drop) against the float64 restatement and the per-element bounds of
tests/gatv2_drop_f64.py with the numpy mask of models._attn_keep_reference, on gat_f64's planted hop (T = 70, S = 200),
T = 1 with 130 entries, E = 0 and T = 0.  (H, C) covers the six forward <NQ, CPH> families and the backward's SPH = 1,
2, 4, 8, 16; rows fp32 and bf16 (fp16 on (4, 16)), p in {0.5, 0.6}, x_r distinct and aliased, the regimes model / wide /
zero.  Then GATv2Conv(dropout=0.6) in training on the device.

Largest err / bound seen on an MI355X: the docstring of test_zz_largest_ratios_seen."""
import collections
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gatv2_drop_f64 as GD  # noqa: E402
import gatv2_f64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, C) and the forward's <NQ, CPH> (gatv2_core.hip.h shape_of): (1,4) (4,16) (8,8) -> <1,1>; (2,256) -> <2,1>;
# (8,128) -> <4,1>; (1,512) -> <2,2>; (2,512) -> <4,2>; (1,1024) -> <4,4>.  The backward's SPH = max(1, C / 64):
# 1 (C <= 64), 2 (128), 4 (256), 8 (512), 16 (1024)
WIDTHS = [(1, 4), (4, 16), (8, 8), (2, 256), (8, 128), (1, 512), (2, 512), (1, 1024)]
DTYPES = [torch.float32, torch.bfloat16]
PS = [0.5, 0.6]
NAMES = ["model", "wide", "zero"]
SLOPE = G.SLOPES[0]
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SEEN = collections.defaultdict(float)


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat.load()


def _st():
    from salient_plusplus_amd.models import _stream
    return _stream()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Run:
    """both entries on one hop; drop = None: the entries without dropout, else (p, training, seed) through the _drop
    entries.  x_l [S, H, C] and x_r [T, H, C] on the device (x_r may be a view of x_l)"""

    def __init__(self, hop, x_l, x_r, att, slope):
        self.hop, self.slope = hop, slope
        self.H, self.C = att.shape
        self.x_l, self.x_r = x_l.view(hop.S, self.H * self.C), x_r.view(hop.T, self.H * self.C)
        self.att = att.cuda()
        self.rowptr, self.col = hop.rowptr.cuda(), hop.col.cuda()

    def _f(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device="cuda")

    def _call(self, name, d, drop):
        L = _lib()
        if drop is None:
            rc = getattr(L, name)(C.byref(d), _st())
        else:
            rc = getattr(L, name + "_drop")(C.byref(d), _st(), float(drop[0]), int(drop[1]), int(drop[2]))
        assert rc == 0, (name, drop, L.spp_last_error())

    def _desc(self, out, rmax, rsum, **grads):
        from salient_plusplus_amd.models import _gatv2_desc
        return _gatv2_desc(self.x_l, self.x_r, self.att, self.rowptr, self.col, self.slope, out, rmax, rsum, **grads)

    def forward(self, drop=None):
        T, H, Cc = self.hop.T, self.H, self.C
        out, rmax, rsum = self._f(T, H, Cc), self._f(T, H), self._f(T, H)
        self._call("spp_gatv2_forward", self._desc(out, rmax, rsum), drop)
        return out, rmax, rsum

    def backward(self, out, rmax, rsum, g, drop=None):
        T, S, H, Cc = self.hop.T, self.hop.S, self.H, self.C
        gxl = self._f(S, H, Cc, zero=True)
        gxr = torch.full((T, H, Cc), float("nan"), device="cuda")
        gatt = torch.full((H, Cc), float("nan"), device="cuda")
        d = self._desc(out, rmax, rsum, grad_out_dev=g, grad_x_l_dev=gxl, grad_x_r_dev=gxr, grad_att_dev=gatt)
        self._call("spp_gatv2_backward", d, drop)
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
        return ratio

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what} [{self.tag}] is not exact")

    def done(self):
        print("\nGATV2_DROP_RATIO " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.top.items())))
        assert not self.bad, "\n".join(self.bad)


@functools.lru_cache(maxsize=None)
def seed_for(H, p):
    """the first seed whose mask drops, for some head, the self loop of a target of the planted hop that keeps no CSR
    entry (so that out is exactly 0 there): found with the numpy restatement alone.  -> (seed, [(t, h), ...])"""
    hop = G.planted_hop(70, 200)
    for seed in range(1, 4000):
        _, ke = GD.mask(hop, H, p, seed)
        alive = torch.zeros((hop.T, H), dtype=torch.float64).index_add_(0, hop.r, ke)
        dead = alive == 0
        if bool(dead[hop.kept == 0].any()):
            return seed, [tuple(v) for v in torch.nonzero(dead).tolist()]
    raise AssertionError("no seed found")


def _device_rows(hop, name, H, Cc, dtype, alias):
    x_l, x_r, att, g = G.inputs(name, hop, H, Cc, dtype)
    xl_d = x_l.cuda()
    if alias:                                                   # share_weights: x_r IS x_l[:T]
        x_r, xr_d = x_l[:hop.T], xl_d[:hop.T]
    else:
        xr_d = x_r.cuda()
    return x_l, x_r, att, g, Run(hop, xl_d, xr_d, att, SLOPE)


def pipeline(c, hop, name, H, Cc, dtype, alias, p, seed, dead=()):
    c.tag = f"{name} p {p} seed {seed} {'aliased' if alias else 'distinct'}"
    x_l, x_r, att, g, r = _device_rows(hop, name, H, Cc, dtype, alias)
    drop = (p, 1, seed)
    _, ke = GD.mask(hop, H, p, seed)
    full = G.forward(hop, x_l, x_r, att, SLOPE)
    bw = GD.backward_drop(hop, x_l, x_r, att, g, SLOPE, ke, p, fw=full)
    # forward: the softmax statistics are those of the p = 0 call, bit for bit; two runs agree bit for bit
    out0, rmax0, rsum0 = r.forward()
    out, rmax, rsum = r.forward(drop)
    out2, rmax2, rsum2 = r.forward(drop)
    c.exact("two forward runs", _same(out, out2) and _same(rmax, rmax2) and _same(rsum, rsum2))
    c.exact("row_max is the p = 0 call's", _same(rmax, rmax0))
    c.exact("row_sum is the p = 0 call's", _same(rsum, rsum0))
    c.within("out", out, bw.fw.out, bw.fw.b_out)
    c.within("row_sum", rsum, bw.fw.row_sum, bw.fw.bs)
    c.within("row_max", rmax, bw.fw.row_max, bw.fw.bm)
    oc = out.cpu()
    for t, h in dead:
        c.exact(f"out of the dead pair ({t}, {h})", bool((oc[t, h] == 0).all()))
    if hop.T and name == "model":
        c.exact("out differs from p = 0", not torch.equal(out, out0))
    gxl, gxr, gatt = r.backward(out, rmax, rsum, g.cuda(), drop)
    c.within("grad_xl", gxl, bw.gxl, bw.b_gxl)
    c.within("grad_xr", gxr, bw.gxr, bw.b_gxr)
    c.within("grad_att", gatt, bw.gatt, bw.b_gatt)
    c.exact("grad_xl of unnamed sources", bool((gxl.cpu()[hop.named == 0] == 0).all()))
    for t in (out, rsum, gxl, gxr, gatt):
        c.exact("finite", bool(torch.isfinite(t).all()))
    return r, bw, (out, rmax, rsum), g


def _cases():
    out = [(H, Cc, dt) for (H, Cc) in WIDTHS for dt in DTYPES]
    return out + [(4, 16, torch.float16)]


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "aliased"])
@pytest.mark.parametrize("H,Cc,dtype", _cases(), **_ID)
def test_both_drop_entries_within_their_bounds_on_the_planted_hop(H, Cc, dtype, alias):
    hop = G.planted_hop(70, 200)
    c = Checks(hop)
    for p in PS:
        seed, dead = seed_for(H, p)
        for name in NAMES:
            pipeline(c, hop, name, H, Cc, dtype, alias, p, seed, dead)
    c.done()


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("H,Cc", WIDTHS)
def test_p_0_and_eval_mode_through_the_drop_entries_equal_the_entries_without(H, Cc, dtype):
    """out and grad_x_r involve no atomics: bit for bit"""
    hop = G.planted_hop(70, 200)
    _x_l, _x_r, _att, g, r = _device_rows(hop, "model", H, Cc, dtype, False)
    g = g.cuda()
    out, rmax, rsum = r.forward()
    _, gxr, _ = r.backward(out, rmax, rsum, g)
    for drop in ((0.6, 0, 11), (0.0, 1, 11), (0.0, 0, 0)):
        out2, rmax2, rsum2 = r.forward(drop)
        assert _same(out2, out) and _same(rmax2, rmax) and _same(rsum2, rsum), drop
        _, gxr2, _ = r.backward(out, rmax, rsum, g, drop)
        assert _same(gxr2, gxr), drop


@pytest.mark.parametrize("H,Cc", [(1, 4), (4, 16), (8, 128)])
def test_smallest_hops(H, Cc):
    none = torch.zeros(0, dtype=torch.int64)
    big = G.planted_hop(70, 200)
    # T = 0: nothing is written, grad_att is zeroed
    hop = G.Hop(torch.zeros(1, dtype=torch.int64), none, 0, 3)
    x_l, x_r, att, g = G.inputs("model", hop, H, Cc, torch.float32)
    r = Run(hop, x_l.cuda(), x_r.cuda(), att, SLOPE)
    out, rmax, rsum = r.forward((0.6, 1, 3))
    gxl, gxr, gatt = r.backward(out, rmax, rsum, g.cuda(), (0.6, 1, 3))
    assert out.shape == (0, H, Cc) and bool((gxl == 0).all()) and bool((gatt == 0).all())
    # T = 1 with a row of 130 entries
    one, _perm = big.one_row(69)
    c = Checks(one)
    pipeline(c, one, "model", H, Cc, torch.float32, False, 0.6, 3)
    pipeline(c, one, "zero", H, Cc, torch.bfloat16, True, 0.5, 4)
    # E = 0 with T = 70: every target is alone with its self loop, kept (x_l[i] * scale) or dropped (0)
    hop = G.Hop(torch.zeros(71, dtype=torch.int64), none, 70, 200)
    _r, _bw, (out, _rmax, rsum), _g = pipeline(c, hop, "model", H, Cc, torch.float32, False, 0.6, 5)
    keep = GD.mask(hop, H, 0.6, 5)[0]
    assert 0 < int(keep.sum()) < keep.size
    oc = out.cpu()
    assert bool((oc[torch.from_numpy(keep) == 0] == 0).all()) and bool((rsum == 1).all())
    c.done()


def test_a_backward_with_another_seed_misses_grad_x_r():
    hop = G.planted_hop(70, 200)
    c = Checks(hop)
    seed, _ = seed_for(4, 0.6)
    r, bw, (out, rmax, rsum), g = pipeline(c, hop, "model", 4, 16, torch.float32, False, 0.6, seed)
    c.done()
    _, gxr, _ = r.backward(out, rmax, rsum, g.cuda(), (0.6, 1, seed + 1))
    ratio, _ = G.worst(gxr, bw.gxr, bw.b_gxr)
    assert ratio > 1.0, ("a backward with another seed passed grad_x_r's bound", ratio)


def test_the_mask_is_attn_keeps_and_zeroing_its_entries_in_the_p_0_restatement_gives_out():
    from salient_plusplus_amd.models import _attn_keep_reference, _p
    hop = G.planted_hop(70, 200)
    H, Cc, p, seed = 4, 16, 0.6, 0x9E3779B97F4A7C15
    n = (hop.E + hop.T) * H
    keep = torch.full((n + 3,), 7, dtype=torch.uint8, device="cuda")
    assert _lib().spp_gat_mh_attn_keep(hop.E, hop.T, H, p, seed, _p(keep), _st()) == 0
    got = keep.cpu().numpy()
    assert np.array_equal(got[:n].reshape(-1, H), _attn_keep_reference(hop.E, hop.T, H, p, seed)) and (got[n:] == 7).all()
    # the float64 p = 0 restatement with exactly those entries zeroed, written out here
    x_l, x_r, att, g, r = _device_rows(hop, "model", H, Cc, torch.float32, False)
    fw = G.forward(hop, x_l, x_r, att, SLOPE)
    ke = GD.entry_keep(hop, got[:n].reshape(-1, H))
    alpha = fw.alpha * ke * GD.scale_of(p)
    want = torch.zeros((hop.T, H, Cc), dtype=torch.float64).index_add_(0, hop.r, alpha.unsqueeze(2) * x_l.double()[hop.s])
    out, _rmax, _rsum = r.forward((p, 1, seed))
    c = Checks(hop)
    c.within("out/device mask", out, want, GD.forward_drop(hop, x_l, x_r, att, SLOPE, ke, p, fw=fw).b_out)
    c.done()


# ------------------------------------------------------------------------------------------------ the layer
def _adj(hop):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    return SparseTensor(rowptr=hop.rowptr.cuda(), col=hop.col.cuda(), sparse_sizes=(hop.T, hop.S))


def _refuse_reference(monkeypatch):
    from salient_plusplus_amd import models

    def boom(*a, **k):
        raise AssertionError("_gatv2_reference was called")
    monkeypatch.setattr(models, "_gatv2_reference", boom)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast_bf16"])
@pytest.mark.parametrize("share", [False, True], ids=["two_maps", "share_weights"])
def test_gatv2conv_training_with_dropout_runs_the_kernels(share, amp, monkeypatch):
    """GATv2Conv(16, 16, heads=4, dropout=0.6).train() against the float64 layer with the mask of the (patched) seed, on
    the rows the layer itself projected (test_gpu_gatv2._layer's comparison)"""
    from salient_plusplus_amd import models
    seed, p, H, Cc = 0xC0FFEE1234567, 0.6, 4, 16
    monkeypatch.setattr(models, "_attn_seed", lambda: seed)
    _refuse_reference(monkeypatch)
    hop = G.planted_hop(70, 200)
    T, S, K = hop.T, hop.S, 16
    torch.manual_seed(3)
    conv = models.GATv2Conv(K, Cc, heads=H, dropout=p, share_weights=share).cuda().train()
    torch.nn.init.normal_(conv.bias)
    x = torch.randn(S, K).cuda()
    kept = {}

    def keep(key):
        return lambda m, i, o: (o.retain_grad(), kept.__setitem__(key, o))[0]

    hooks = [conv.lin_l.register_forward_hook(keep("x_l"))]
    if not share:
        hooks.append(conv.lin_r.register_forward_hook(keep("x_r")))
    g = torch.randn(T, H * Cc)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = conv((x, x[:T]), _adj(hop))
    for h in hooks:
        h.remove()
    out.backward(g.cuda())
    assert out.dtype == torch.float32
    x_l = kept["x_l"].detach().cpu().view(S, H, Cc)
    assert x_l.dtype == (torch.bfloat16 if amp else torch.float32)
    x_r = x_l[:T] if share else kept["x_r"].detach().cpu().view(T, H, Cc)
    att = conv.att.detach().cpu().view(H, Cc)
    _, ke = GD.mask(hop, H, p, seed)
    bw = GD.backward_drop(hop, x_l, x_r, att, g.view(T, H, Cc), conv.negative_slope, ke, p)
    ref, b_out, cast = G.layer_bounds(bw, True, conv.bias.detach().cpu(), x_l.dtype)
    c = Checks(hop)
    c.tag = f"share {share} amp {amp}"
    c.within("layer out", out.detach(), ref, b_out)
    c.within("layer grad_att", conv.att.grad.view(H, Cc), bw.gatt, bw.b_gatt)
    gl = kept["x_l"].grad.view(S, H, Cc)
    if share:                                                   # autograd sums grad_xl and grad_xr through the view
        pad, bpad = torch.zeros_like(bw.gxl), torch.zeros_like(bw.b_gxl)
        pad[:T], bpad[:T] = bw.gxr, bw.b_gxr
        ref_l = bw.gxl + pad
        b_l = G.G2 * (bw.b_gxl + bpad + cast * (bw.gxl.abs() + pad.abs()) + max(cast, G.U) * ref_l.abs())
        c.within("layer grad_xl + grad_xr", gl, ref_l, b_l)
    else:
        c.within("layer grad_xl", gl, bw.gxl, G.G2 * (bw.b_gxl + cast * bw.gxl.abs()))
        c.within("layer grad_xr", kept["x_r"].grad.view(T, H, Cc), bw.gxr, G.G2 * (bw.b_gxr + cast * bw.gxr.abs()))
    assert bool(torch.isfinite(conv.lin_l.weight.grad).all())
    c.done()


def test_gatv2conv_training_is_repeatable_under_manual_seed(monkeypatch):
    from salient_plusplus_amd import models
    _refuse_reference(monkeypatch)
    hop = G.planted_hop(70, 200)
    torch.manual_seed(5)
    conv = models.GATv2Conv(16, 16, heads=4, dropout=0.6).cuda().train()
    x = torch.randn(hop.S, 16).cuda()
    outs = []
    for seed in (9, 9, 10):
        torch.manual_seed(seed)
        outs.append(conv((x, x[:hop.T]), _adj(hop)).detach())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    with torch.no_grad():                                       # eval: the p = 0 module's bits
        plain = models.GATv2Conv(16, 16, heads=4).cuda().eval()
        plain.load_state_dict(conv.state_dict())
        assert torch.equal(conv.eval()((x, x[:hop.T]), _adj(hop)), plain((x, x[:hop.T]), _adj(hop)))


def test_refused_widths_and_cpu_tensors_still_take_the_reference_path(monkeypatch):
    from salient_plusplus_amd import models
    calls = []
    orig = models._gatv2_reference
    monkeypatch.setattr(models, "_gatv2_reference", lambda *a: (calls.append(a[-1]), orig(*a))[1])
    kernel = []
    orig_k = models._GATv2Layer.apply
    monkeypatch.setattr(models._GATv2Layer, "apply", lambda *a: (kernel.append(1), orig_k(*a))[1])
    hop = G.planted_hop(70, 200)
    torch.manual_seed(6)
    wide = models.GATv2Conv(16, 12, heads=2, dropout=0.6).cuda().train()      # C = 12: C / 4 not a power of two
    x = torch.randn(hop.S, 16).cuda()
    out = wide((x, x[:hop.T]), _adj(hop))
    assert calls == [0.6] and not kernel and bool(torch.isfinite(out).all())
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    cpu = models.GATv2Conv(16, 16, heads=4, dropout=0.6).train()
    adj = SparseTensor(rowptr=hop.rowptr, col=hop.col, sparse_sizes=(hop.T, hop.S))
    out = cpu((x.cpu(), x.cpu()[:hop.T]), adj)
    assert calls == [0.6, 0.6] and not kernel and bool(torch.isfinite(out).all())


def test_zz_largest_ratios_seen():
    """prints the largest err / bound per output quantity over the tests of this module that ran before it.

    Seen on an MI355X (a record, not an input to the bounds): out 0.06, row_max 0.22, row_sum 0.06, grad_xl 0.07,
    grad_xr 0.02, grad_att 0.004; out against the p = 0 restatement with spp_gat_mh_attn_keep's bytes zeroed 0.03; at
    layer level out 0.60, grad_att 0.001, and under bf16 autocast grad_xl 0.98, grad_xr 0.93, their sum through the
    share_weights view 0.92 -- there the bound is almost entirely the cast back to bf16 (2^-8 |value|)."""
    print("\nGATV2_DROP_LARGEST " + " ".join(f"{k}={v:.3f}" for k, v in sorted(SEEN.items())))
