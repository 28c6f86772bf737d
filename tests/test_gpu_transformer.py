"""-m gpu: the TransformerConv kernels (csrc/transformer_conv.hip: spp_transformer_forward, spp_transformer_backward)
against the float64 restatement and the per-element bounds of tests/transformer_f64.py, element by element, on
gat_f64's planted hop (every CSR entry, diagonals kept, no self loops, empty rows) and the logit regimes of
transformer_f64.inputs; then TransformerConv and a 2-layer GraphTransformer on the device.  Each test prints the largest
err / bound per output quantity (TRANSFORMER_F64_RATIO lines): a record, not an input to the bounds.

Seen on an MI355X: the docstring of test_zz_largest_ratios_seen."""
import collections
import copy
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transformer_f64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
# (H, C) the entries accept: fewer than 64 lanes per row, one, two and four chunks per head, D = 1024
WIDTHS = [(1, 4), (1, 64), (4, 16), (8, 8), (8, 128), (2, 256)]
REFUSED = [(2, 12), (4, 260)]                               # C / 4 not a power of two; that and D > 1024
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SEEN = collections.defaultdict(float)


def _call(name, desc):
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.models import _stream
    return getattr(nat.load(), name)(C.byref(desc), _stream())


@functools.lru_cache(maxsize=None)
def _ent(S):
    return G.entries_of(G.planted_hop(70, S))


@functools.lru_cache(maxsize=None)
def _reference(ent, name, H, Cc, dtype):
    """the inputs of a regime and their float64 values and bounds: computed once, shared by the runs that differ in the
    layout of k and v only, and left unchanged"""
    q, k, v, g = G.inputs(name, ent, H, Cc, dtype)
    return q, k, v, g, G.backward(ent, q, k, v, g, G.scale32(Cc))


class Run:
    """both entries on one hop; q [T, D], k and v [S, D] on the device (k and v may be the halves of one matrix)"""

    def __init__(self, ent, q, k, v, H, scale):
        self.ent, self.H, self.scale = ent, H, scale
        self.D = q.size(1)
        self.q, self.k, self.v = q, k, v
        self.rowptr, self.col = ent.rowptr.cuda(), ent.col.cuda()

    def _f(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device="cuda")

    def _desc(self, out, rmax, rsum, **grads):
        from salient_plusplus_amd.models import _transformer_desc
        return _transformer_desc(self.q, self.k, self.v, self.H, self.rowptr, self.col, self.scale, out, rmax, rsum, **grads)

    def forward(self):
        T, H, Cc = self.ent.T, self.H, self.D // self.H
        out, rmax, rsum = (torch.full(s, float("nan"), device="cuda") for s in ((T, H, Cc), (T, H), (T, H)))
        assert _call("spp_transformer_forward", self._desc(out, rmax, rsum)) == 0
        return out, rmax, rsum

    def backward(self, out, rmax, rsum, g, want_k=True, want_v=True):
        T, S, H, Cc = self.ent.T, self.ent.S, self.H, self.D // self.H
        gk = self._f(S, H, Cc, zero=True) if want_k else None
        gv = self._f(S, H, Cc, zero=True) if want_v else None
        gq = torch.full((T, H, Cc), float("nan"), device="cuda")
        d = self._desc(out, rmax, rsum, grad_out_dev=g, grad_q_dev=gq, grad_k_dev=gk, grad_v_dev=gv)
        assert _call("spp_transformer_backward", d) == 0
        return gq, gk, gv


def on_device(ent, q, k, v, H, scale, fused):
    """fused: k and v as the halves of one [S, 2 D] matrix (row stride 2 D); else three matrices of their own"""
    S, T = ent.S, ent.T
    D = k[0].numel()
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
        ratio, where = G.worst(got, ref, bound)
        self.top[what] = max(self.top[what], ratio)
        SEEN[what] = max(SEEN[what], ratio)
        if not ratio <= 1.0:
            self.bad.append(f"{what} [{self.tag}] err/bound {ratio:.3f} at {where}")

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what} [{self.tag}] is not exact")

    def done(self):
        print("\nTRANSFORMER_F64_RATIO " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.top.items())))
        assert not self.bad, "\n".join(self.bad)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def pipeline(c, ent, name, H, Cc, dtype, fused, wants=((True, True), (False, True), (True, False), (False, False))):
    c.tag = f"{name} H {H} C {Cc} {str(dtype).split('.')[-1]} {'k|v one matrix' if fused else 'k, v apart'}"
    scale = G.scale32(Cc)
    q, k, v, g, bw = _reference(ent, name, H, Cc, dtype)
    r = on_device(ent, q, k, v, H, scale, fused)
    out, rmax, rsum = r.forward()
    out2, rmax2, rsum2 = r.forward()
    c.exact("two forward runs", _same(out, out2) and _same(rmax, rmax2) and _same(rsum, rsum2))
    fw = bw.fw
    c.within("out", out, fw.out, fw.b_out)
    c.within("row_sum", rsum, fw.row_sum, fw.bs)
    c.within("row_max", rmax, fw.row_max, fw.bm)
    empty = ent.n == 0
    for what, t in (("out", out), ("row_sum", rsum), ("row_max", rmax)):
        c.exact(what + " of a row without entries is 0", bool((t.cpu()[empty] == 0).all()))
    if name == "zero":                                          # q = 0: the plain mean of v over the row
        c.within("out against the mean of v", out, G.mean_of_v(ent, v), fw.b_out)
    unnamed = ent.named == 0
    for want_k, want_v in wants:
        gq, gk, gv = r.backward(out, rmax, rsum, g.cuda(), want_k, want_v)
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


@pytest.mark.parametrize("fused", [False, True], ids=["apart", "one_matrix"])
@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("H,Cc", WIDTHS)
def test_both_entries_within_their_bounds_on_the_planted_hops(H, Cc, dtype, fused):
    """every regime on planted_hop(70, 200) and on the square (70, 70); all four NULL combinations of grad_k / grad_v on
    the first, both wanted on the second"""
    c = Checks()
    for name in G.REGIMES:
        pipeline(c, _ent(200), name, H, Cc, dtype, fused)
        pipeline(c, _ent(70), name, H, Cc, dtype, fused, wants=((True, True),))
    c.done()


@pytest.mark.parametrize("H,Cc", [(1, 4), (4, 16), (8, 128)])
def test_smallest_hops(H, Cc):
    none = torch.zeros(0, dtype=torch.int64)
    big = _ent(200)
    scale = G.scale32(Cc)
    # T = 0: nothing is written, the caller's zeroed grad_k / grad_v stay zero
    ent = G.Entries(torch.zeros(1, dtype=torch.int64), none, 0, 3)
    q, k, v, g = G.inputs("model", ent, H, Cc, torch.float32)
    r = on_device(ent, q, k, v, H, scale, False)
    out, rmax, rsum = r.forward()
    gq, gk, gv = r.backward(out, rmax, rsum, g.cuda())
    assert out.shape == (0, H, Cc) and gq.shape == (0, H, Cc)
    assert bool((gk == 0).all()) and bool((gv == 0).all())
    # T = 1 with one row of 130 entries
    c = Checks()
    one = G.one_row(big, 69)
    assert int(one.n[0]) == 130
    pipeline(c, one, "model", H, Cc, torch.float32, False)
    pipeline(c, one, "ascending", H, Cc, torch.bfloat16, True)
    # E = 0 with T = 70: every row is empty
    ent = G.Entries(torch.zeros(71, dtype=torch.int64), none, 70, 200)
    pipeline(c, ent, "model", H, Cc, torch.float32, False)
    q, k, v, g = G.inputs("model", ent, H, Cc, torch.float32)
    r = on_device(ent, q, k, v, H, scale, True)
    out, rmax, rsum = r.forward()
    gq, gk, gv = r.backward(out, rmax, rsum, g.cuda())
    for t in (out, rmax, rsum, gq, gk, gv):
        assert bool((t == 0).all()) and not bool(torch.isnan(t).any())
    c.done()


def test_the_forward_repeats_its_bits():
    ent = _ent(200)
    q, k, v, _g = G.inputs("model", ent, 4, 16, torch.bfloat16)
    r = on_device(ent, q, k, v, 4, G.scale32(16), True)
    a, b = r.forward(), r.forward()
    assert all(_same(x, y) for x, y in zip(a, b))
    r2 = on_device(ent, q, k, v, 4, G.scale32(16), False)       # the layout of k and v changes no bit either
    assert all(_same(x, y) for x, y in zip(a, r2.forward()))


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("H,Cc", WIDTHS + [(1, 512), (2, 512), (1, 1024)])     # + heads of two and four forward chunks
def test_the_backward_recomputes_the_forwards_logit_bit_for_bit(H, Cc, dtype):
    """Rows of ONE entry each, distinct sources, logits of tens.  The forward's weight is exactly 1 (out = v[j],
    row_sum = 1, row_max = the logit).  The backward's alpha = expf(e' - row_max) / row_sum is 1 only if its recomputed
    e' is row_max bit for bit -- one summation tree in both kernels (csrc/transformer_conv.hip) -- and then
    grad_v[j] = g_i and grad_q = grad_k = 0 exactly.  With another order e' - row_max is a few ulps of sum|q k|, which
    at these logits is 1e-6 and more: the model-level distance of DESIGN section 7 f3y."""
    T, S = 70, 200
    col = torch.randperm(S, generator=torch.Generator().manual_seed(3))[:T]
    ent = G.Entries(torch.arange(T + 1), col, T, S)
    q, k, v, g = G.inputs("model", ent, H, Cc, dtype)
    q, k = q * 8, k * 8                                          # exact; logits 16 N(0, 1)
    r = on_device(ent, q, k, v, H, G.scale32(Cc), False)
    out, rmax, rsum = r.forward()
    assert float(rmax.abs().max()) > 20
    assert torch.equal(out.cpu(), v.float()[col]) and bool((rsum == 1).all())
    gq, gk, gv = r.backward(out, rmax, rsum, g.cuda())
    want = torch.zeros((S, H, Cc))
    want[col] = g
    assert torch.equal(gv.cpu(), want), float((gv.cpu() - want).abs().max())
    assert bool((gq == 0).all()) and bool((gk == 0).all())


# ------------------------------------------------------------------------------------------------ the layer
def _adj(ent):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    return SparseTensor(rowptr=ent.rowptr.cuda(), col=ent.col.cuda(), sparse_sizes=(ent.T, ent.S))


def _count(monkeypatch):
    """counts _TransformerLayer.apply calls and keeps each result with its gradient retained"""
    from salient_plusplus_amd import models
    calls = []
    orig = models._TransformerLayer.apply

    def apply(*a):
        out = orig(*a)
        if out.requires_grad:
            out.retain_grad()
        calls.append(out)
        return out

    monkeypatch.setattr(models._TransformerLayer, "apply", apply)
    return calls


def _layer(monkeypatch, ent, H, Cc, concat, bias, beta, root_weight, amp, kernels):
    """TransformerConv on the device against the float64 layer evaluated on the rows the layer itself projected
    (captured from lin_query / lin_key / lin_value, and lin_skip / lin_beta for the skip and the gate: fp32, or bf16
    under autocast -- converted exactly, so the kernel-level bounds hold unchanged).  The gradient that reaches the
    attention's output is read off the node itself when the gate stands between it and the loss."""
    from salient_plusplus_amd.models import TransformerConv
    calls = _count(monkeypatch)
    torch.manual_seed(H * 100 + Cc)
    T, S, K = ent.T, ent.S, 12
    conv = TransformerConv(K, Cc, heads=H, concat=concat, bias=bias, beta=beta, root_weight=root_weight).cuda()
    x = torch.randn(S, K).cuda()
    kept = {}

    def keep(key):
        return lambda m, i, o: (o.retain_grad(), kept.__setitem__(key, o))[0]

    mods = {"q": conv.lin_query, "k": conv.lin_key, "v": conv.lin_value, "skip": conv.lin_skip, "gate": conv.lin_beta}
    hooks = [m.register_forward_hook(keep(n)) for n, m in mods.items() if m is not None]
    width = H * Cc if concat else Cc
    g = torch.randn(T, width)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = conv((x, x[:T]), _adj(ent))
    for h in hooks:
        h.remove()
    out.backward(g.cuda())
    assert len(calls) == (1 if kernels else 0) and out.dtype == torch.float32
    rows = torch.bfloat16 if amp else torch.float32
    q = kept["q"].detach().cpu().view(T, H, Cc)
    k, v = (kept[n].detach().cpu().view(S, H, Cc) for n in ("k", "v"))
    assert q.dtype == k.dtype == v.dtype == rows
    if beta:                                                    # the gate stands between the attention and the loss
        assert kernels
        g_att = calls[0].grad.detach().cpu().view(T, H, Cc)
    else:                                                       # (g / H: exact, H a power of two)
        g_att = g.view(T, H, Cc) if concat else (g / H).unsqueeze(1).expand(T, H, Cc)
    bw = G.backward(ent, q, k, v, g_att, G.scale32(Cc))
    ref, b, cast = G.layer_bounds(bw, concat, rows)
    if root_weight:
        x_r = kept["skip"].detach().double().cpu()
        if beta:
            # b = sigmoid(z) on the captured z, within cb b (fp32: a few ulps, 8 u; bf16: computed in fp32 and rounded
            # once, with the bf16 product b x_r and the bf16 1 - b: 2^-8 covers each); then two products and a sum
            cb = 2.0 ** -8 if amp else 8 * G.U
            gate = torch.sigmoid(kept["gate"].detach().double().cpu())
            fin = gate * x_r + (1 - gate) * ref
            b = G.G2 * (cb * gate * x_r.abs() + cb * (gate * x_r).abs() + (cb * gate + cb * (1 - gate)) * ref.abs()
                        + (1 - gate) * b + 3 * G.U * ((gate * x_r).abs() + ((1 - gate) * ref).abs()))
            ref = fin
        else:
            ref = ref + x_r
            b = G.G2 * (b + G.U * ref.abs())
    c = Checks()
    c.tag = f"H {H} C {Cc} concat {concat} bias {bias} beta {beta} root_weight {root_weight} amp {amp}"
    c.within("layer out", out.detach(), ref, b)
    for n, val, bound in (("q", bw.gq, bw.b_gq), ("k", bw.gk, bw.b_gk), ("v", bw.gv, bw.b_gv)):
        c.within("layer grad_" + n, kept[n].grad.view(val.shape), val, G.G2 * (bound + cast * val.abs()))
    assert x.grad is None
    for lin in (conv.lin_query, conv.lin_key, conv.lin_value):
        assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all())
    c.done()


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast_bf16"])
@pytest.mark.parametrize("concat,bias,beta,root_weight", [(True, True, False, True), (False, False, False, True),
                                                          (True, True, True, True), (False, True, True, True),
                                                          (True, False, False, False), (False, True, False, False)])
def test_transformerconv_on_the_kernels(concat, bias, beta, root_weight, amp, monkeypatch):
    _layer(monkeypatch, _ent(200), 4, 16, concat, bias, beta, root_weight, amp, kernels=True)


@pytest.mark.parametrize("H,Cc", REFUSED)
def test_refused_widths_take_the_reference_path(H, Cc, monkeypatch):
    """spp.h f3y: C / 4 not a power of two and D > 1024 are refused by the entries; TransformerConv still answers"""
    from salient_plusplus_amd import _native as nat
    ent = _ent(200)
    q, k, v, _g = G.inputs("model", ent, H, Cc, torch.float32)
    r = on_device(ent, q, k, v, H, G.scale32(Cc), False)
    out, rmax, rsum = r._f(ent.T, H, Cc), r._f(ent.T, H), r._f(ent.T, H)
    assert _call("spp_transformer_forward", r._desc(out, rmax, rsum)) == -1
    msg = nat.load().spp_last_error().decode()
    assert "spp_transformer_forward" in msg and "power of two" in msg   # checked before D (D > 1024 alone: the host test)
    assert _call("spp_transformer_backward", r._desc(out, rmax, rsum, grad_out_dev=out, grad_q_dev=out)) == -1
    assert "spp_transformer_backward" in nat.load().spp_last_error().decode()
    _layer(monkeypatch, ent, H, Cc, True, True, False, True, False, kernels=False)


# ------------------------------------------------------------------------------------------------ the model
def test_graph_transformer_model_step_against_float64(monkeypatch):
    """A 2-layer GraphTransformer(16, 32, 8, 2, heads=4), one training step (nll loss, backward) on the two inner hops
    of a three-hop sampled batch (gatv2_f64.sampled_batch(classes=8)), with the dropout mask between the layers fixed:
    loss and every parameter gradient of the kernel path, and of the fp32 reference path on the SAME device (the layer
    sent to _transformer_reference, so that the two fp32 runs differ in the message passing alone), against the same
    model in float64 on the CPU.  Per tensor the distance is max|a - ref| / max|ref|; the kernel path may be up to 4x
    the reference path's (online against two-pass softmax, atomics): the margin of
    test_gatv2_model_step_against_float64.

    lin_key.bias is judged differently, because its exact gradient is ZERO (adding a constant to every key shifts all
    logits of a row alike: sum_j ge_ij = 0), so max|ref| is float64 rounding (1e-17) and the quotient of the two paths'
    distances is the quotient of two fp32 noises: the reference path ALONE read 3.2e+08 to 1.4e+09 on it from run to
    run (its index_add atomics), a spread of 4.5x.  That gradient is the column sum of the S rows of grad_k, S fp32
    numbers each known to u = 2^-24 of its size at best, so a value below (S + 1) u sum_j |grad_k[j, c]| (float64 run)
    is zero as far as fp32 can tell; the tensor passes inside the 4x margin OR under that floor, element by element.

    Measured on an MI355X (reference path on the device / kernel path / ratio):
        loss                      5.265e-08  1.663e-08  0.32
        convs.0.lin_key.weight    4.579e-07  4.368e-07  0.95
        convs.0.lin_key.bias      7.158e+08  1.670e+09  2.33   (exact gradient 0: see above)
        convs.0.lin_query.weight  2.649e-07  2.454e-07  0.93
        convs.0.lin_query.bias    2.819e-07  3.205e-07  1.14
        convs.0.lin_value.weight  2.384e-07  2.774e-07  1.16
        convs.0.lin_value.bias    1.480e-07  2.087e-07  1.41
        convs.0.lin_skip.weight   1.664e-07  2.136e-07  1.28
        convs.0.lin_skip.bias     1.014e-07  1.414e-07  1.39
        convs.1.lin_key.weight    9.856e-08  2.049e-07  2.08
        convs.1.lin_key.bias      9.171e+08  2.369e+09  2.58   (exact gradient 0)
        convs.1.lin_query.weight  1.766e-07  2.617e-07  1.48
        convs.1.lin_query.bias    1.740e-07  4.325e-07  2.49
        convs.1.lin_value.weight  4.604e-07  2.217e-07  0.48
        convs.1.lin_value.bias    1.762e-07  1.513e-07  0.86
        convs.1.lin_skip.weight   1.936e-07  1.565e-07  0.81
        convs.1.lin_skip.bias     1.125e-07  8.445e-08  0.75
    (With the backward recomputing its logits in another summation order than the forward, the last layer -- logits up
    to 18, rows dominated by one entry -- stood at 4.4 to 7.4 on lin_key / lin_query and up to 5.6 on lin_value: the
    kernels share one summation tree for that reason)"""
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    from gatv2_f64 import sampled_batch
    calls = _count(monkeypatch)

    def fixed_dropout(x, p=0.5, training=True):
        gen = torch.Generator().manual_seed(x.numel())
        mask = (torch.rand(tuple(x.shape), generator=gen) > p).to(x.dtype) / (1.0 - p)
        return torch.relu(x) * mask.to(x.device)

    monkeypatch.setattr(models, "relu_dropout", fixed_dropout)
    x, y, hops = sampled_batch(classes=8)
    hops = hops[1:]
    x = x[:hops[0][3]].contiguous()
    torch.manual_seed(1)
    model = models.GraphTransformer(16, 32, 8, 2, heads=4).train()

    def step(m, dev, dtype, keys=None):
        adjs = [(SparseTensor(rowptr=rp.to(dev), col=cl.to(dev), sparse_sizes=(T, S)), None, (S, T)) for rp, cl, T, S in hops]
        m.zero_grad()
        hooks = [c.lin_key.register_forward_hook(lambda mod, i, o: (o.retain_grad(), keys.append(o))[0]) for c in m.convs] \
            if keys is not None else []
        loss = torch.nn.functional.nll_loss(m(x.to(dev, dtype), adjs), y.to(dev))
        loss.backward()
        for h in hooks:
            h.remove()
        return [loss.detach().double().cpu()] + [p.grad.double().cpu() for p in m.parameters()]

    keys = []
    ref = step(copy.deepcopy(model).double(), "cpu", torch.float64, keys)
    # what fp32 cannot tell from zero in a column sum of the S rows of grad_k (the docstring)
    floor = {f"convs.{i}.lin_key.bias": (kk.size(0) + 1) * G.U * kk.grad.abs().sum(0) for i, kk in enumerate(keys)}
    with monkeypatch.context() as mp:                           # the reference path on the device
        mp.setattr(models, "_transformer_kernels_read", lambda *a: False)
        dev = step(copy.deepcopy(model).cuda(), "cuda", torch.float32)
    assert not calls
    gpu = step(copy.deepcopy(model).cuda(), "cuda", torch.float32)
    assert len(calls) == 2
    names = ["loss"] + [n for n, _ in model.named_parameters()]
    bad = []
    for n, r, a, b in zip(names, ref, dev, gpu):
        scale = float(r.abs().max())
        d_ref, d_ker = float((a - r).abs().max()) / scale, float((b - r).abs().max()) / scale
        print(f"TRANSFORMER_MODEL {n}: reference path {d_ref:.3e} kernel path {d_ker:.3e} "
              f"ratio {d_ker / d_ref if d_ref else float('inf'):.2f}")
        zero = n in floor and bool(((b - r).abs() <= floor[n]).all())
        if n in floor:
            print(f"TRANSFORMER_MODEL {n}: max|ref| {scale:.3e}; kernel path's largest |value| / floor "
                  f"{float(((b - r).abs() / floor[n]).max()):.3f}, reference path's {float(((a - r).abs() / floor[n]).max()):.3f}")
        if not (d_ker <= 4 * d_ref or zero):
            bad.append((n, d_ref, d_ker))
    assert not bad, bad


def test_zz_largest_ratios_seen():
    """prints the largest err / bound per output quantity over the tests of this module that ran before it (a record,
    not an input to the bounds; DESIGN section 7 f3y keeps the figures seen on an MI355X)"""
    print("\nTRANSFORMER_F64_LARGEST " + " ".join(f"{k}={v:.3f}" for k, v in sorted(SEEN.items())))
