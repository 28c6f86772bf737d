"""CPU: the float64 restatement of the edge-weighted aggregation in tests/agg_w_f64.py checked on its own.  Its closed-form
gradients against torch.autograd of models._weighted_reference in float64; its bounds against an fp32 emulation of the
kernels' order of operations -- the forward's and backward's fmaf chains, the weight gradient's lane partition, butterfly
and rounds in both forms, gcn_norm's chain -- which stays within every bound at every width, hop and type
tests/test_gpu_agg_w_f64.py uses and within HALF of it on the fp32 results of chains of 32 values or more (the _margin
rule of tests/test_agg_f64_host.py, whose module docstring says why the half is asked there and only there); planted
faults, each of which must exceed a bound somewhere; and the properties the weights are documented to have."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_f64 as A  # noqa: E402
import agg_w_f64 as W  # noqa: E402
from test_agg_f64_host import LONG, _fma, _margin, _ratio, _segments  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL_WIDTHS = A.WIDTHS + [1024]
WGRAD_WIDTHS = ALL_WIDTHS + [300, 1028]                    # 300 and 1028: the second round, scalar and vector form
GCN_HOPS = ["planted", "square", "tall", "E0", "T1", "T1S1"]


def _hops_for(F):
    return ["square"] if F in (300, 1024, 1028) else A.hops_for(F)


def _grad(hop, F, dtype):
    return A.values(hop.T, F, dtype, seed=9)


# ------------------------------------------------------------------------------------------------ fp32 emulation
def _chain(key, n, take, F, first=None, partial_bf16=False, cnt_less=None):
    """fmaf chains: acc[r] = fmaf(w, v, acc[r]) over the entries of key value r in ascending entry id; take(ids) ->
    (w [m], v [m, F]).  first [n, F]: the accumulators' start.  partial_bf16: the accumulator through bf16 once, before a
    chain's last entry.  cnt_less [n]: entries dropped from the end of each chain"""
    seg, cnt = _segments(key, n)
    if cnt_less is not None:
        cnt = cnt - cnt_less
    acc = torch.zeros((n, F), dtype=F32) if first is None else first.clone()
    for k in range(seg.size(1) if key.numel() else 0):
        live = torch.nonzero(cnt > k).flatten()
        if partial_bf16:
            last = live[cnt[live] == k + 1]
            acc[last] = acc[last].bfloat16().float()
        w, v = take(seg[live, k])
        acc[live] = _fma(w.unsqueeze(1), v, acc[live])
    return acc


def emu_forward(c, x, self_w, out_dtype=F32, fault=None):
    """k_agg_w_fwd: a row's entries in CSR order, one fmaf each onto 0, the self term last"""
    hop, xf = c.hop, x.float()
    less = hop.deg % 2 if fault == "drop_tail" else None
    acc = _chain(hop.row, hop.T, lambda ids: (c.w[ids], xf[hop.col[ids]]), xf.size(1), partial_bf16=fault == "bf16_partial",
                 cnt_less=less)
    if self_w and fault != "no_self":
        acc = _fma(c.sw.unsqueeze(1), xf[:hop.T], acc)
    return acc.to(out_dtype)


def _second_of_pairs(hop):
    """[E] the entry whose weight a wrong tedge reads: the entry before it where that is the same (t, s) pair, else itself"""
    ids = torch.arange(hop.E)
    if hop.E > 1:
        same = (hop.row[1:] == hop.row[:-1]) & (hop.col[1:] == hop.col[:-1])
        ids[1:] = torch.where(same, ids[:-1], ids[1:])
    return ids


def emu_backward(c, g, self_w, out_dtype=F32, fault=None):
    """k_agg_w_bwd over the ordered transposed hop: a source's entries in ascending CSR position, one fmaf each onto 0
    with the weight tedge names, the self term last and for s < T only"""
    hop, gf = c.hop, g.float()
    T, S, F = hop.T, hop.S, gf.size(1)
    wid = _second_of_pairs(hop) if fault == "wrong_tedge" else torch.arange(hop.E)
    less = hop.indeg % 2 if fault == "drop_tail" else None
    acc = _chain(hop.col, S, lambda ids: (c.w[wid[ids]], gf[hop.row[ids]]), F, partial_bf16=fault == "bf16_partial",
                 cnt_less=less)
    if self_w and fault != "no_self":
        acc[:T] = _fma(c.sw.unsqueeze(1), gf, acc[:T])
        if fault == "self_beyond_T":                           # s >= T reads self_w and g past their ends: here, row s - T
            n = min(S - T, T)
            acc[T:T + n] = _fma(c.sw[:n].unsqueeze(1), gf[:n], acc[T:T + n])
    return acc.to(out_dtype)


def emu_wgrad(c, x, g, vec, fault=None):
    """k_agg_w_wgrad: (grad_w [E], grad_self_w [T]).  Column r * 4 step + i * step + l * width + j belongs to round r,
    column step i, lane l, place j of its piece: a lane fmafs its columns of a round in that order onto 0 (a column past F
    is skipped: an fmaf of zeros here), group_sum's butterfly adds lane l ^ m for m = lpr / 2 .. 1, lane 0's sum is
    stored in round 0 and added to the stored value in every later round"""
    hop, sh = c.hop, W.wgrad_shape(x.size(1), vec)
    F = x.size(1)
    pad = sh.rounds * W.WGRAD_STEPS * sh.step - F

    def lanes(v):                                              # [N, F] -> [N, rounds, steps, lpr, width]
        v = torch.nn.functional.pad(v.float(), (0, pad))
        return v.view(v.size(0), sh.rounds, W.WGRAD_STEPS, sh.lpr, sh.width)

    def dots(gv, xv):
        gl, xl = lanes(gv), lanes(xv)
        if fault == "drop_step":                               # lane 0 leaves out its last column step of round 0
            last = min(W.WGRAD_STEPS, -(-F // sh.step)) - 1
            gl = gl.clone()
            gl[:, 0, last, 0, :] = 0
        s = torch.zeros(gl.shape[:2] + (sh.lpr,), dtype=F32)
        for i in range(W.WGRAD_STEPS):
            for j in range(sh.width):
                s = _fma(gl[:, :, i, :, j], xl[:, :, i, :, j], s)
        m = sh.lpr >> 1
        while m:
            s = s + s[..., torch.arange(sh.lpr) ^ m]
            m >>= 1
        out = s[:, 0, 0]
        for r in range(1, sh.rounds):
            out = s[:, r, 0] if fault == "overwrite" else out + s[:, r, 0]
        return out

    return dots(g[hop.row], x[hop.col]), dots(g, x[:hop.T])


def emu_gcn(hop, w, fill, fault=None):
    """k_gcn_dinv / k_gcn_coef: the row sum a sequential fp32 chain from 0 (the count itself without weights), fill + s,
    sqrtf, one division, inf -> 0; coef = (dinv_t w) dinv_s, self_coef = (dinv_t fill) dinv_t"""
    T = hop.T
    if w is None:
        s = hop.deg.float()
    else:
        seg, cnt = _segments(hop.row, T)
        s = torch.zeros(T, dtype=F32)
        for k in range(seg.size(1) if hop.E else 0):
            live = torch.nonzero(cnt > k).flatten()
            s[live] = s[live] + w[seg[live, k]]
    fl = torch.tensor(float(fill), dtype=F32)
    d = 1.0 / torch.sqrt(fl + s)
    dinv = torch.where(torch.isinf(d), torch.zeros_like(d), d)
    foreign = 1.0 / torch.sqrt(fl) if fill and fault != "no_fill_foreign" else torch.zeros((), dtype=F32)
    at = hop.col.clamp(max=max(T - 1, 0))
    ds = torch.where(hop.col < T, dinv[at], foreign) if T else foreign.expand(hop.E)
    if fault == "dinv_of_row":
        ds = dinv[hop.row]
    wk = torch.ones(hop.E, dtype=F32) if w is None else w
    return dinv[hop.row] * wk * ds, dinv * fl * dinv


# ------------------------------------------------------------------------------------------------ honest emulations
@pytest.mark.parametrize("F", ALL_WIDTHS)
def test_honest_forward_and_backward_emulations_stay_within_half_of_every_bound(F):
    """every hop, row / gradient type and output type of the GPU file at this width, with and without self_w"""
    top = 0.0
    for name in A.hops_for(F):
        c = W.case(name)
        hop = c.hop
        is_t = (torch.arange(hop.S) < hop.T).long()
        for self_w in (False, True):
            for xdt in (F32, F16, BF16):
                x = A.values(hop.S, F, xdt)
                top = max(top, _margin(emu_forward(c, x, self_w), hop.deg + int(self_w),
                                        lambda odt: W.forward(c, x, self_w, odt)))
            for gdt in (F32, BF16):
                g = _grad(hop, F, gdt)
                top = max(top, _margin(emu_backward(c, g, self_w), hop.indeg + is_t * int(self_w),
                                        lambda odt: W.backward(c, g, self_w, odt), (F32, BF16, F16)))
    print(f"\nAGG_W_F64_HOST forward / backward F {F}: largest err / bound of the long chains {top:.3f}")


@pytest.mark.parametrize("F", WGRAD_WIDTHS)
def test_honest_wgrad_emulation_stays_within_half_of_every_bound(F):
    """both forms where F % 4 == 0 (a misaligned source takes the scalar form); a dot product of 32 columns or more is a
    chain of 32 values or more"""
    top = 0.0
    for name in _hops_for(F):
        c = W.case(name)
        hop = c.hop
        for vec in (False, True) if F % 4 == 0 else (False,):
            for xdt in (F32, F16, BF16):
                for gdt in (F32, BF16):
                    x, g = A.values(hop.S, F, xdt), _grad(hop, F, gdt)
                    gw, gs = emu_wgrad(c, x, g, vec)
                    rw, bw, rs, bs = W.wgrad(c, x, g, vec)
                    for got, ref, b in ((gw, rw, bw), (gs, rs, bs)):
                        top = max(top, _margin(got, torch.full((got.numel(),), F), lambda odt: (ref, b), (F32,)))
    print(f"\nAGG_W_F64_HOST wgrad F {F}: largest err / bound {top:.3f}")


@pytest.mark.parametrize("fill", W.FILLS)
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_honest_gcn_norm_emulation_stays_within_half_of_every_bound(weighted, fill):
    top = 0.0
    for name in GCN_HOPS:
        hop = A.hop_of(name)
        w = W.gcn_weights(name) if weighted else None
        coef, self_coef = emu_gcn(hop, w, fill)
        rc, bc, rs, bs = W.gcn_norm(hop, w, fill)
        top = max(top, _margin(coef, hop.deg[hop.row], lambda odt: (rc, bc), (F32,)),
                  _margin(self_coef, hop.deg, lambda odt: (rs, bs), (F32,)))
        assert bool((bc >= 0).all()) and bool(torch.isfinite(bc).all()) and bool(torch.isfinite(rc).all())
        if fill == 0:                                          # D = 0: exact zeros wherever the target is touched
            dead = torch.zeros(hop.S, dtype=torch.bool)
            dead[:hop.T] = (hop.deg == 0) if w is None else torch.zeros(hop.T).index_add_(0, hop.row, w) == 0
            dead[hop.T:] = True
            touched = dead[hop.row] | dead[hop.col]
            assert bool((rc[touched] == 0).all()) and bool((bc[touched] == 0).all()) and bool((coef[touched] == 0).all())
            assert bool((rs == 0).all()) and bool((self_coef == 0).all())
    print(f"\nAGG_W_F64_HOST gcn_norm fill {fill}: largest err / bound of the long rows {top:.3f}")


def test_the_wgrad_counts_are_the_ones_the_derivation_names():
    assert W.wgrad_shape(1028, True).c == 16 + 6 + 1 and W.wgrad_shape(1028, True).rounds == 2
    assert W.wgrad_shape(300, False).c == 4 + 6 + 1 and W.wgrad_shape(300, False).rounds == 2
    assert W.wgrad_shape(1024, True).c == 16 + 6 and W.wgrad_shape(1024, False).c == 4 + 6 + 3
    assert W.wgrad_shape(1, False).c == 1 and W.wgrad_shape(2, False).c == 2 and W.wgrad_shape(4, True).c == 4
    assert W.wgrad_shape(260, True).lpr == 64 and W.wgrad_shape(260, True).m == 8          # 65 pieces: two column steps
    assert all(W.wgrad_shape(F, v).c < F + 1 for F in WGRAD_WIDTHS for v in (False, F % 4 == 0) if F > 1)


# ------------------------------------------------------------------------------------------------ planted faults
FWD_BWD_FAULTS = ["wrong_tedge", "drop_tail", "no_self", "self_beyond_T", "bf16_partial"]


# every hop that has what the fault needs: the square hop has no source beyond T
FWD_BWD_CASES = [(f, h) for f in FWD_BWD_FAULTS for h in A.HOPS if (f, h) != ("self_beyond_T", "square")]


@pytest.mark.parametrize("fault,name", FWD_BWD_CASES)
def test_a_planted_forward_or_backward_fault_exceeds_a_bound(fault, name):
    """in every kernel the fault can live in; fp32 rows, gradients and results, but for the accumulator rounded to bf16,
    which is judged against the bf16 result's bound"""
    c = W.case(name)
    hop, F = c.hop, 8
    odt = BF16 if fault == "bf16_partial" else F32
    x, g = A.values(hop.S, F, odt), _grad(hop, F, odt)
    each = []
    if fault in ("drop_tail", "no_self", "bf16_partial"):
        assert _ratio(emu_forward(c, x, True, odt), *W.forward(c, x, True, odt))[0] <= 1.0
        each.append(_ratio(emu_forward(c, x, True, odt, fault), *W.forward(c, x, True, odt))[0])
    assert _ratio(emu_backward(c, g, True, odt), *W.backward(c, g, True, odt))[0] <= 1.0
    each.append(_ratio(emu_backward(c, g, True, odt, fault), *W.backward(c, g, True, odt))[0])
    assert min(each) > 1.0, (fault, each)


@pytest.mark.parametrize("F,vec", [(300, False), (1028, True), (1028, False)])
@pytest.mark.parametrize("fault", ["drop_step", "overwrite"])
def test_a_planted_wgrad_fault_exceeds_a_bound(fault, F, vec):
    c = W.case("square")
    x, g = A.values(c.hop.S, F, F32), _grad(c.hop, F, F32)
    rw, bw, rs, bs = W.wgrad(c, x, g, vec)
    gw, gs = emu_wgrad(c, x, g, vec, fault)
    assert _ratio(gw, rw, bw)[0] > 1.0 and _ratio(gs, rs, bs)[0] > 1.0
    gw, gs = emu_wgrad(c, x, g, vec)
    assert _ratio(gw, rw, bw)[0] <= 0.5 and _ratio(gs, rs, bs)[0] <= 0.5


@pytest.mark.parametrize("fault,name", [(f, h) for f in ("dinv_of_row", "no_fill_foreign") for h in A.HOPS
                                        if (f, h) != ("no_fill_foreign", "square")])
def test_a_planted_gcn_norm_fault_exceeds_a_bound(fault, name):
    """no_fill_foreign needs a source that is no target (not the square hop) and a fill"""
    hop = A.hop_of(name)
    for w in (None, W.gcn_weights(name)):
        for fill in (1, 2):
            rc, bc, _rs, _bs = W.gcn_norm(hop, w, fill)
            assert _ratio(emu_gcn(hop, w, fill)[0], rc, bc)[0] <= 1.0
            assert _ratio(emu_gcn(hop, w, fill, fault)[0], rc, bc)[0] > 1.0, (fill, w is None)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("name", A.HOPS + A.DEGENERATE)
@pytest.mark.parametrize("self_w", [False, True], ids=["plain", "self_w"])
def test_closed_forms_agree_with_autograd_of_the_weighted_reference(self_w, name):
    from salient_plusplus_amd.models import _weighted_reference
    c = W.case(name)
    hop, F = c.hop, 5
    x, g = A.values(hop.S, F, F32), _grad(hop, F, F32)
    xq, wq, sq = (v.double().requires_grad_(True) for v in (x, c.w, c.sw))
    out = _weighted_reference(xq, hop.rowptr, hop.col, wq, hop.T, sq if self_w else None)
    (out * g.double()).sum().backward()

    def agree(ref, b, want):
        want = torch.where(b == 0, want.float().double(), want)                        # (a single rounding: as fp32)
        torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-14)
        assert bool((b >= 0).all()) and bool(torch.isfinite(b).all())

    agree(*W.forward(c, x, self_w), out.detach())
    agree(*W.backward(c, g, self_w), xq.grad)
    for vec in (False,):
        rw, bw, rs, bs = W.wgrad(c, x, g, vec)
        agree(rw, bw, wq.grad if wq.grad is not None else torch.zeros(hop.E, dtype=A.F64))
        if self_w:
            agree(rs, bs, sq.grad)


def test_gcn_norm_agrees_with_the_float64_reference():
    from salient_plusplus_amd.models import _gcn_norm_reference
    for name in GCN_HOPS:
        hop = A.hop_of(name)
        for w in (None, W.gcn_weights(name)):
            for fill, kw in ((0, dict(add_self_loops=False)), (1, dict()), (2, dict(improved=True))):
                want_c, want_s = _gcn_norm_reference(hop.rowptr, hop.col, hop.T, None if w is None else w.double(),
                                                     dtype=torch.float64, **kw)
                rc, _bc, rs, _bs = W.gcn_norm(hop, w, fill)
                torch.testing.assert_close(rc, want_c, rtol=1e-13, atol=0)
                torch.testing.assert_close(rs, want_s, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ the hops and weights
@pytest.mark.parametrize("name", A.HOPS)
def test_the_weights_have_their_documented_properties(name):
    c = W.case(name)
    hop = c.hop
    assert bool((c.w < 0).any()) and bool((c.w > 0).any()) and int((c.w == 0).sum()) >= hop.E // 12
    assert bool((c.sw == 0).any()) and bool((c.sw != 0).any())
    key = hop.row * hop.S + hop.col                            # entries of one (t, s) pair carry different weights
    order = torch.sort(key, stable=True).indices
    rep = key[order][1:] == key[order][:-1]
    assert int(rep.sum()) > 0
    pairs = torch.stack([key[order].double(), c.w[order].double()], 1)
    assert torch.unique(pairs, dim=0).size(0) == hop.E
    adjacent = _second_of_pairs(hop) != torch.arange(hop.E)    # ... the adjacent ones the wrong-tedge fault uses too
    assert int(adjacent.sum()) > 0 and bool((c.w[_second_of_pairs(hop)][adjacent] != c.w[adjacent]).all())
    t = W.zero_row(name)                                       # a zero-sum row for the fill-0 case
    gw = W.gcn_weights(name)
    assert t is not None and int(hop.deg[t]) == 3 and float(gw[hop.row == t].sum()) == 0.0
    assert bool((gw >= 0).all()) and bool((gw[hop.row != t] > 0).any())
    if name == "tall":
        assert all(int(hop.indeg[s]) > 600 for s in hop.hubs) and -(-hop.T // 256) == 3
        assert any(int(hop.indeg[s]) % 2 == 1 for s in hop.hubs)
    assert bool((hop.deg >= LONG).any()) or name == "tall"
    assert bool((hop.indeg >= LONG).any())
