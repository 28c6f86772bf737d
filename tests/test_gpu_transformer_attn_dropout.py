"""-m gpu: attention dropout inside the TransformerConv kernels (spp.h f4a: spp_transformer_forward_drop /
spp_transformer_backward_drop, csrc/transformer_conv.hip with kDrop) against the float64 restatement and the per-element
bounds of tests/transformer_drop_f64.py with the numpy mask of models._attn_keep_reference, on gat_f64's planted hops
(T = 70, S = 200 and the square one) in the logit regimes of transformer_f64.inputs; the bit facts the header states;
then TransformerConv(dropout=p) and GraphTransformer(attn_dropout=p) on the device.  Each test prints the largest
err / bound per output quantity (TRANSFORMER_DROP_RATIO lines): a record, not an input to the bounds."""
import collections
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transformer_drop_f64 as XD  # noqa: E402
import transformer_f64 as X  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, C): all six forward (NQ, CPH) families -- (1, 1): (1,4), (4,16), (8,8); (2, 1): (2,256); (4, 1): (8,128);
# (2, 2): (1,512); (4, 2): (2,512); (4, 4): (1,1024) -- and the backward's steps per head SPH = 1 .. 16
ISSUE_WIDTHS = [(1, 4), (4, 16), (8, 8), (2, 256), (8, 128), (1, 512), (2, 512), (1, 1024)]
# + one width for each of the backward's (NS, SPH) instantiations the list above leaves out, so that all fourteen run
# with the mask: (4,32) -> (2, 1); (1,128) -> (2, 2); (8,32) and (4,64) -> (4, 1), the flagship's; (2,128) -> (4, 2);
# (1,256) -> (4, 4); (8,64) -> (8, 1); (4,128) -> (8, 2); (4,256) -> (16, 4).  From NS = 4 on the backward draws through
# bwd_keep<true> (one hash per wavefront); (8,32) is its only case where the two heads that share a hash sit in the
# same step of a lane, so that the hash's half differs between lanes 0-31 and 32-63.
WIDTHS = ISSUE_WIDTHS + [(4, 32), (1, 128), (8, 32), (4, 64), (2, 128), (1, 256), (8, 64), (4, 128), (4, 256)]
CASES = [(H, Cc, dt) for H, Cc in WIDTHS for dt in (torch.float32, torch.bfloat16)] + [(4, 16, torch.float16)]
PS = (0.5, 0.6)
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SEEN = collections.defaultdict(float)


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat.load()


def _st():
    from salient_plusplus_amd.models import _stream
    return _stream()


@functools.lru_cache(maxsize=None)
def _ent(S):
    return X.entries_of(X.planted_hop(70, S))


@functools.lru_cache(maxsize=None)
def seed_for(ent, H, p):
    """the first seed whose mask drops every entry of some (target, head) of the hop: the case is then in every run, by
    construction"""
    for seed in range(1, 400):
        keep, ke = XD.mask(ent, H, p, seed)
        if bool(XD.all_dropped(ent, ke).any()):
            return seed
    raise AssertionError("no seed drops a whole (target, head)")


@functools.lru_cache(maxsize=None)
def _reference(ent, name, H, Cc, dtype):
    """the inputs of a regime and the float64 p = 0 forward: computed once, shared by the runs that differ in p, seed or
    the layout of k and v, and left unchanged"""
    q, k, v, g = X.inputs(name, ent, H, Cc, dtype)
    return q, k, v, g, X.forward(ent, q, k, v, X.scale32(Cc))


class Run:
    """both entries on one hop; q [T, D], k and v [S, D] on the device (k and v may be the halves of one matrix).
    drop: None for the entries without dropout, else (p, training, seed) for the _drop entries"""

    def __init__(self, ent, q, k, v, H, scale):
        self.ent, self.H, self.scale = ent, H, scale
        self.D = q.size(1)
        self.q, self.k, self.v = q, k, v
        self.rowptr, self.col = ent.rowptr.cuda(), ent.col.cuda()

    def _desc(self, out, rmax, rsum, **grads):
        from salient_plusplus_amd.models import _transformer_desc
        return _transformer_desc(self.q, self.k, self.v, self.H, self.rowptr, self.col, self.scale, out, rmax, rsum, **grads)

    @staticmethod
    def _call(name, d, drop):
        if drop is None:
            return getattr(_lib(), name)(C.byref(d), _st())
        return getattr(_lib(), name + "_drop")(C.byref(d), _st(), *drop)

    def forward(self, drop):
        T, H, Cc = self.ent.T, self.H, self.D // self.H
        out, rmax, rsum = (torch.full(s, float("nan"), device="cuda") for s in ((T, H, Cc), (T, H), (T, H)))
        assert self._call("spp_transformer_forward", self._desc(out, rmax, rsum), drop) == 0
        return out, rmax, rsum

    def backward(self, out, rmax, rsum, g, drop, want_k=True, want_v=True):
        T, S, H, Cc = self.ent.T, self.ent.S, self.H, self.D // self.H
        gk = torch.zeros((S, H, Cc), device="cuda") if want_k else None
        gv = torch.zeros((S, H, Cc), device="cuda") if want_v else None
        gq = torch.full((T, H, Cc), float("nan"), device="cuda")
        d = self._desc(out, rmax, rsum, grad_out_dev=g, grad_q_dev=gq, grad_k_dev=gk, grad_v_dev=gv)
        assert self._call("spp_transformer_backward", d, drop) == 0
        return gq, gk, gv


def on_device(ent, q, k, v, H, scale, fused):
    """fused: k and v as the halves of one [S, 2 D] matrix (row stride 2 D); else three matrices of their own"""
    S, T = ent.S, ent.T
    D = q[0].numel() if T else k[0].numel()
    if fused:
        kv = torch.cat([k.reshape(S, D), v.reshape(S, D)], 1).cuda()
        kd, vd = kv[:, :D], kv[:, D:]
    else:
        kd, vd = k.reshape(S, D).cuda(), v.reshape(S, D).cuda()
    return Run(ent, q.reshape(T, D).cuda(), kd, vd, H, scale)


class Checks:
    def __init__(self):
        self.tag, self.bad, self.top = "", [], collections.defaultdict(float)

    def within(self, what, got, ref, bound):
        assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
        ratio, where = X.worst(got, ref, bound)
        self.top[what] = max(self.top[what], ratio)
        SEEN[what] = max(SEEN[what], ratio)
        if not ratio <= 1.0:
            self.bad.append(f"{what} [{self.tag}] err/bound {ratio:.3f} at {where}")

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what} [{self.tag}] is not exact")

    def done(self):
        print("\nTRANSFORMER_DROP_RATIO " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.top.items())))
        assert not self.bad, "\n".join(self.bad)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def pipeline(c, ent, name, H, Cc, dtype, fused, p, seed, wants=((True, True),)):
    c.tag = (f"{name} H {H} C {Cc} {str(dtype).split('.')[-1]} {'k|v one matrix' if fused else 'k, v apart'} p {p} "
             f"seed {seed} T {ent.T} S {ent.S}")
    scale = X.scale32(Cc)
    q, k, v, g, fw0 = _reference(ent, name, H, Cc, dtype)
    _, ke = XD.mask(ent, H, p, seed)
    bw = XD.backward_drop(ent, q, k, v, g, scale, ke, p, fw=fw0)
    fw = bw.fw
    r = on_device(ent, q, k, v, H, scale, fused)
    drop = (p, 1, seed)
    out, rmax, rsum = r.forward(drop)
    out2, rmax2, rsum2 = r.forward(drop)
    c.exact("two forward runs with one seed", _same(out, out2) and _same(rmax, rmax2) and _same(rsum, rsum2))
    _o, rmax0, rsum0 = r.forward(None)
    c.exact("row_max / row_sum are spp_transformer_forward's bits", _same(rmax, rmax0) and _same(rsum, rsum0))
    c.within("out", out, fw.out, fw.b_out)
    c.within("row_sum", rsum, fw.row_sum, fw.bs)
    c.within("row_max", rmax, fw.row_max, fw.bm)
    empty, dropped = ent.n == 0, XD.all_dropped(ent, ke)
    oc = out.cpu()
    c.exact("out of a row without entries is 0", bool((oc[empty] == 0).all()))
    c.exact("out of a (target, head) with every entry dropped is 0", bool((oc[dropped] == 0).all()))
    unnamed = ent.named == 0
    for want_k, want_v in wants:
        gq, gk, gv = r.backward(out, rmax, rsum, g.cuda(), drop, want_k, want_v)
        form = "" if want_k and want_v else f"/{'k' if want_k else ''}{'v' if want_v else ''} only"
        c.within("grad_q" + form, gq, bw.gq, bw.b_gq)
        c.exact("grad_q of a row without entries is 0", bool((gq.cpu()[empty] == 0).all()))
        if want_k:
            c.within("grad_k" + form, gk, bw.gk, bw.b_gk)
            c.exact("grad_k of unnamed sources", bool((gk.cpu()[unnamed] == 0).all()))
        if want_v:
            c.within("grad_v" + form, gv, bw.gv, bw.b_gv)
            c.exact("grad_v of unnamed sources", bool((gv.cpu()[unnamed] == 0).all()))
        for t in (out, rmax, rsum, gq, gk, gv):
            c.exact("finite", t is None or bool(torch.isfinite(t).all()))
    return r, bw, (out, rmax, rsum), g


@pytest.mark.parametrize("H,Cc,dtype", CASES, **_ID)
def test_both_drop_entries_within_their_bounds_on_the_planted_hops(H, Cc, dtype):
    """all six regimes on planted_hop(70, 200) and on the square (70, 70), k and v apart and as the halves of one matrix
    in every one of them; p alternates between 0.5 and 0.6 from regime to regime and starts differently on the two
    hops, so every regime meets both p and both hops meet both.  That is a deliberate reduction: the full
    regime x p x hop product is NOT run (each (hop, regime) pair meets one p), to keep a case at a fraction of a second;
    the bounds and the properties checked are the same for every run.  The hops hold empty rows and one-entry rows, and
    the seeds are chosen so that some (target, head) loses every entry (asserted)."""
    c = Checks()
    for S, first in ((200, 0), (70, 1)):
        ent = _ent(S)
        assert bool((ent.n == 0).any()) and bool((ent.n == 1).any())
        for i, name in enumerate(X.REGIMES):
            p = PS[(i + first) % 2]
            seed = seed_for(ent, H, p)
            assert bool(XD.all_dropped(ent, XD.mask(ent, H, p, seed)[1]).any())
            for fused in (False, True):
                pipeline(c, ent, name, H, Cc, dtype, fused, p, seed)
    c.done()


def test_the_four_null_combinations_of_grad_k_and_grad_v():
    c = Checks()
    ent = _ent(200)
    pipeline(c, ent, "model", 4, 16, torch.float32, False, 0.6, seed_for(ent, 4, 0.6),
             wants=((True, True), (False, True), (True, False), (False, False)))
    c.done()


@pytest.mark.parametrize("H,Cc,dtype", [(4, 16, torch.float32), (8, 128, torch.bfloat16), (1, 1024, torch.float32)], **_ID)
def test_p_0_and_eval_mode_through_the_drop_entries_equal_the_entries_without(H, Cc, dtype):
    """training = 0 or p = 0 launch the kernels without dropout: the bits of out, row_max, row_sum and grad_q (grad_k
    and grad_v are sums of atomics, whose order is not fixed in either entry: they are inside the p = 0 bounds)"""
    ent = _ent(200)
    q, k, v, g, fw0 = _reference(ent, "model", H, Cc, dtype)
    bw = X.backward(ent, q, k, v, g, X.scale32(Cc), fw=fw0)
    r = on_device(ent, q, k, v, H, X.scale32(Cc), True)
    base = r.forward(None)
    gq0, _gk0, _gv0 = r.backward(*base, g.cuda(), None)
    c = Checks()
    for drop in ((0.0, 1, 7), (0.6, 0, 7), (0.0, 0, 7)):
        c.tag = f"drop {drop}"
        got = r.forward(drop)
        c.exact("forward", all(_same(a, b) for a, b in zip(got, base)))
        gq, gk, gv = r.backward(*got, g.cuda(), drop)
        c.exact("grad_q", _same(gq, gq0))
        c.within("grad_k", gk, bw.gk, bw.b_gk)
        c.within("grad_v", gv, bw.gv, bw.b_gv)
    c.done()


@pytest.mark.parametrize("H,Cc", [(1, 4), (4, 16), (8, 128)])
def test_smallest_hops(H, Cc):
    none = torch.zeros(0, dtype=torch.int64)
    big = _ent(200)
    scale = X.scale32(Cc)
    drop = (0.6, 1, 11)
    # T = 0: nothing is written, the caller's zeroed grad_k / grad_v stay zero
    ent = X.Entries(torch.zeros(1, dtype=torch.int64), none, 0, 3)
    q, k, v, g = X.inputs("model", ent, H, Cc, torch.float32)
    r = on_device(ent, q, k, v, H, scale, False)
    out, rmax, rsum = r.forward(drop)
    gq, gk, gv = r.backward(out, rmax, rsum, g.cuda(), drop)
    assert out.shape == (0, H, Cc) and gq.shape == (0, H, Cc)
    assert bool((gk == 0).all()) and bool((gv == 0).all())
    # T = 1 with one row of 130 entries
    c = Checks()
    one = X.one_row(big, 69)
    assert int(one.n[0]) == 130
    pipeline(c, one, "model", H, Cc, torch.float32, False, 0.5, 3)
    pipeline(c, one, "ascending", H, Cc, torch.bfloat16, True, 0.6, 4)
    # E = 0 with T = 70: every row is empty
    ent = X.Entries(torch.zeros(71, dtype=torch.int64), none, 70, 200)
    q, k, v, g = X.inputs("model", ent, H, Cc, torch.float32)
    r = on_device(ent, q, k, v, H, scale, True)
    out, rmax, rsum = r.forward(drop)
    gq, gk, gv = r.backward(out, rmax, rsum, g.cuda(), drop)
    for t in (out, rmax, rsum, gq, gk, gv):
        assert bool((t == 0).all()) and not bool(torch.isnan(t).any())
    c.done()


def test_a_backward_with_another_seed_misses_grad_q():
    ent = _ent(200)
    c = Checks()
    seed = seed_for(ent, 4, 0.6)
    r, bw, (out, rmax, rsum), g = pipeline(c, ent, "model", 4, 16, torch.float32, False, 0.6, seed)
    c.done()
    gq, _gk, _gv = r.backward(out, rmax, rsum, g.cuda(), (0.6, 1, seed + 1))
    ratio, _ = X.worst(gq, bw.gq, bw.b_gq)
    assert ratio > 1.0, ("a backward with another seed passed grad_q's bound", ratio)


def test_the_mask_is_attn_keeps_and_zeroing_its_entries_in_the_p_0_restatement_gives_out():
    from salient_plusplus_amd.models import _attn_keep_reference, _p
    ent = _ent(200)
    H, Cc, p, seed = 4, 16, 0.6, 0x9E3779B97F4A7C15
    n = (ent.E + ent.T) * H
    keep = torch.full((n + 3,), 7, dtype=torch.uint8, device="cuda")
    assert _lib().spp_gat_mh_attn_keep(ent.E, ent.T, H, p, seed, _p(keep), _st()) == 0
    got = keep.cpu().numpy()
    first = got[:ent.E * H].reshape(ent.E, H)                   # the bytes these entries apply: no self-loop draws
    assert np.array_equal(first, _attn_keep_reference(ent.E, 0, H, p, seed)) and (got[n:] == 7).all()
    # the float64 p = 0 restatement with exactly those entries zeroed, written out here
    q, k, v, _g, fw = _reference(ent, "model", H, Cc, torch.float32)
    ke = XD.entry_keep(ent, first, H)
    alpha = fw.alpha * ke * XD.scale_of(p)
    want = torch.zeros((ent.T, H, Cc), dtype=torch.float64).index_add_(0, ent.row, alpha.unsqueeze(2) * v.double()[ent.col])
    r = on_device(ent, q, k, v, H, X.scale32(Cc), False)
    out, _rmax, _rsum = r.forward((p, 1, seed))
    c = Checks()
    c.within("out/device mask", out, want, XD.forward_drop(ent, q, k, v, X.scale32(Cc), ke, p, fw=fw).b_out)
    c.done()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], **_ID)
@pytest.mark.parametrize("H,Cc", WIDTHS)     # (1, 512), (2, 512): heads of two chunks; (1, 1024): four; every backward (NS, SPH)
def test_one_entry_rows_at_logits_of_tens_are_exact_under_the_mask(H, Cc, dtype):
    """test_gpu_transformer's rows of ONE entry each (distinct sources, logits of tens), now with the mask at p = 0.5,
    where the drop scale is exactly 2.  The weight of the only entry is 1 to the bit in both kernels (one summation tree),
    so a kept (row, head) has out = 2 v[j], grad_v[j] = 2 g_i and grad_q = grad_k = 0 exactly (go = g . 2 v = 2 gh, every
    step a scaling by 2), and a dropped one has out, grad_q, grad_k and grad_v[j] exactly 0."""
    T, S, p, seed = 70, 200, 0.5, 21
    col = torch.randperm(S, generator=torch.Generator().manual_seed(3))[:T]
    ent = X.Entries(torch.arange(T + 1), col, T, S)
    q, k, v, g = X.inputs("model", ent, H, Cc, dtype)
    q, k = q * 8, k * 8                                          # exact; logits 16 N(0, 1)
    keep = torch.from_numpy(XD.mask(ent, H, p, seed)[0]).bool()  # [T, H]: entry t is row t's
    assert bool(keep.any()) and bool((~keep).any())
    r = on_device(ent, q, k, v, H, X.scale32(Cc), False)
    drop = (p, 1, seed)
    out, rmax, rsum = r.forward(drop)
    assert float(rmax.abs().max()) > 20 and bool((rsum == 1).all())
    want_out = torch.where(keep.unsqueeze(2), 2 * v.float()[col], torch.zeros(()))
    assert torch.equal(out.cpu(), want_out)
    gq, gk, gv = r.backward(out, rmax, rsum, g.cuda(), drop)
    want = torch.zeros((S, H, Cc))
    want[col] = torch.where(keep.unsqueeze(2), 2 * g, torch.zeros(()))
    assert torch.equal(gv.cpu(), want), float((gv.cpu() - want).abs().max())
    assert bool((gq == 0).all()) and bool((gk == 0).all())


# ------------------------------------------------------------------------------------------------ the layer
def _adj(ent, dev="cuda"):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    return SparseTensor(rowptr=ent.rowptr.to(dev), col=ent.col.to(dev), sparse_sizes=(ent.T, ent.S))


def _refuse_reference(monkeypatch):
    from salient_plusplus_amd import models

    def boom(*a, **k):
        raise AssertionError("_transformer_reference was called")
    monkeypatch.setattr(models, "_transformer_reference", boom)


@pytest.mark.parametrize("amp,beta", [(False, False), (True, False), (False, True)],
                         ids=["fp32", "autocast_bf16", "fp32_beta"])
def test_transformerconv_training_with_dropout_runs_the_kernels(amp, beta, monkeypatch):
    """TransformerConv(16, 16, heads=4, dropout=0.6).train() against the float64 layer with the mask of the (patched)
    seed, on the rows the layer itself projected (test_gpu_transformer._layer's comparison); the reference path raises"""
    from salient_plusplus_amd import models
    seed, p, H, Cc = 0xC0FFEE1234567, 0.6, 4, 16
    monkeypatch.setattr(models, "_attn_seed", lambda: seed)
    _refuse_reference(monkeypatch)
    calls = []
    orig = models._TransformerLayer.apply

    def apply(*a):
        out = orig(*a)
        out.retain_grad()
        calls.append((a, out))
        return out

    monkeypatch.setattr(models._TransformerLayer, "apply", apply)
    ent = _ent(200)
    T, S, K = ent.T, ent.S, 16
    torch.manual_seed(3)
    conv = models.TransformerConv(K, Cc, heads=H, dropout=p, beta=beta).cuda().train()
    x = torch.randn(S, K).cuda()
    kept = {}

    def keep(key):
        return lambda m, i, o: (o.retain_grad(), kept.__setitem__(key, o))[0]

    mods = {"q": conv.lin_query, "k": conv.lin_key, "v": conv.lin_value, "skip": conv.lin_skip, "gate": conv.lin_beta}
    hooks = [m.register_forward_hook(keep(n)) for n, m in mods.items() if m is not None]
    g = torch.randn(T, H * Cc)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = conv((x, x[:T]), _adj(ent))
    for h in hooks:
        h.remove()
    out.backward(g.cuda())
    assert len(calls) == 1 and len(calls[0][0]) == 8 and calls[0][0][7] == p and out.dtype == torch.float32
    rows = torch.bfloat16 if amp else torch.float32
    q = kept["q"].detach().cpu().view(T, H, Cc)
    k, v = (kept[n].detach().cpu().view(S, H, Cc) for n in ("k", "v"))
    assert q.dtype == k.dtype == v.dtype == rows
    g_att = calls[0][1].grad.detach().cpu().view(T, H, Cc) if beta else g.view(T, H, Cc)
    _, ke = XD.mask(ent, H, p, seed)
    bw = XD.backward_drop(ent, q, k, v, g_att, X.scale32(Cc), ke, p)
    ref, b, cast = X.layer_bounds(bw, True, rows)
    x_r = kept["skip"].detach().double().cpu()
    if beta:        # test_gpu_transformer._layer's gate: sigmoid within 8 u of its value, two products and a sum
        cb = 8 * X.U
        gate = torch.sigmoid(kept["gate"].detach().double().cpu())
        fin = gate * x_r + (1 - gate) * ref
        b = X.G2 * (cb * gate * x_r.abs() + cb * (gate * x_r).abs() + (cb * gate + cb * (1 - gate)) * ref.abs()
                    + (1 - gate) * b + 3 * X.U * ((gate * x_r).abs() + ((1 - gate) * ref).abs()))
        ref = fin
    else:
        ref = ref + x_r
        b = X.G2 * (b + X.U * ref.abs())
    c = Checks()
    c.tag = f"amp {amp} beta {beta}"
    c.within("layer out", out.detach(), ref, b)
    for n, val, bound in (("q", bw.gq, bw.b_gq), ("k", bw.gk, bw.b_gk), ("v", bw.gv, bw.b_gv)):
        c.within("layer grad_" + n, kept[n].grad.view(val.shape), val, X.G2 * (bound + cast * val.abs()))
    for lin in (conv.lin_query, conv.lin_key, conv.lin_value):
        assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all())
    c.done()


def test_transformerconv_training_is_repeatable_under_manual_seed(monkeypatch):
    from salient_plusplus_amd import models
    _refuse_reference(monkeypatch)
    ent = _ent(200)
    torch.manual_seed(5)
    conv = models.TransformerConv(16, 16, heads=4, dropout=0.6).cuda().train()
    x = torch.randn(ent.S, 16).cuda()
    outs = []
    for seed in (9, 9, None):
        if seed is not None:
            torch.manual_seed(seed)
        outs.append(conv((x, x[:ent.T]), _adj(ent)).detach())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    with torch.no_grad():                                       # eval: the p = 0 module's bits
        plain = models.TransformerConv(16, 16, heads=4).cuda().eval()
        plain.load_state_dict(conv.state_dict())
        assert torch.equal(conv.eval()((x, x[:ent.T]), _adj(ent)), plain((x, x[:ent.T]), _adj(ent)))


def test_refused_widths_cpu_tensors_and_other_head_counts_still_take_the_reference_path(monkeypatch):
    from salient_plusplus_amd import models
    calls, kernel = [], []
    orig, orig_k = models._transformer_reference, models._TransformerLayer.apply
    monkeypatch.setattr(models, "_transformer_reference", lambda *a: (calls.append(a[-1]), orig(*a))[1])
    monkeypatch.setattr(models._TransformerLayer, "apply", lambda *a: (kernel.append(1), orig_k(*a))[1])
    ent = _ent(200)
    torch.manual_seed(6)
    x = torch.randn(ent.S, 16).cuda()
    wide = models.TransformerConv(16, 12, heads=2, dropout=0.6).cuda().train()           # C = 12: C / 4 not a power of two
    three = models.TransformerConv(16, 16, heads=3, dropout=0.6, edge_dim=None).cuda().train()
    for i, conv in enumerate((wide, three)):
        torch.manual_seed(8)
        a = conv((x, x[:ent.T]), _adj(ent))
        torch.manual_seed(8)
        b = conv((x, x[:ent.T]), _adj(ent))
        c = conv((x, x[:ent.T]), _adj(ent))
        assert calls == [0.6] * (3 * i + 3) and not kernel and bool(torch.isfinite(a).all())
        # torch's generator decides the mask (the reference's index_add_ is atomics on the device: close, not equal)
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5) and not torch.allclose(a, c, rtol=1e-4, atol=1e-5)
    cpu = models.TransformerConv(16, 16, heads=4, dropout=0.6).train()
    out = cpu((x.cpu(), x.cpu()[:ent.T]), _adj(ent, "cpu"))
    assert calls == [0.6] * 7 and not kernel and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ the model
def test_graph_transformer_with_attn_dropout_trains_on_the_kernels_and_scores_without_it(monkeypatch):
    from gatv2_f64 import sampled_batch
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    from salient_plusplus_amd.inference import layerwise_inference
    _refuse_reference(monkeypatch)
    x, y, hops = sampled_batch(seeds=16, classes=8)            # 8 classes: the last layer is on the kernels too
    adjs = [(SparseTensor(rowptr=rp.cuda(), col=cl.cuda(), sparse_sizes=(T, S)), None, (S, T)) for rp, cl, T, S in hops]
    torch.manual_seed(2)
    model = models.GraphTransformer(16, 32, 8, len(hops), heads=4, attn_dropout=0.6).cuda().train()
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loss = torch.nn.functional.nll_loss(model(x.cuda(), adjs), y.cuda())
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    plain = models.GraphTransformer(16, 32, 8, len(hops), heads=4, attn_dropout=0.0).cuda().eval()
    plain.load_state_dict(model.state_dict())                    # no parameter or buffer of the dropout's
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(x.cuda(), adjs), plain(x.cuda(), adjs))
    N = 300
    gen = torch.Generator().manual_seed(4)
    deg = torch.randint(0, 9, (N,), generator=gen)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=gen)
    feats = torch.randn((N, 16), generator=gen).cuda()
    got = layerwise_inference(model.train(), feats, rowptr.cuda(), col.cuda())
    assert torch.equal(got, layerwise_inference(plain, feats, rowptr.cuda(), col.cuda()))


def test_zz_largest_ratios_seen():
    """prints the largest err / bound per output quantity over the tests of this module that ran before it (a record,
    not an input to the bounds; DESIGN section 7 f4a keeps the figures seen on an MI355X)"""
    print("\nTRANSFORMER_DROP_LARGEST " + " ".join(f"{k}={v:.3f}" for k, v in sorted(SEEN.items())))
