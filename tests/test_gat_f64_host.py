"""CPU: the float64 GAT restatement of tests/gat_f64.py checked on its own.  Its closed-form gradients against
torch.autograd of an independent float64 formula; its bounds against an fp32 emulation of the kernels' order of operations
(an honest one stays within HALF of every bound; each planted fault exceeds a bound somewhere); and the properties the
planted hop is documented to have."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_f64 as G  # noqa: E402

F32 = torch.float32
WIDTHS = [4, 8, 12, 64, 260, 1024]                         # the widths of tests/test_gpu_gat_f64.py
OLD_WIDTHS = [1, 3, 47, 64, 130]                           # ... and of the older full-width kernels (H = 1)


def shape_of(K):
    return (70, 70) if K == 1024 else (70, 200)


def model_logits(x, V, T):
    """the "model" regime on the CPU: x . V in fp32"""
    return x.float() @ V[0].t(), x.float()[:T] @ V[1].t()


def logits_of(name, hop, x, V):
    H = V.size(1)
    return model_logits(x, V, hop.T) if name == "model" else G.regime(name, hop, H)


# ------------------------------------------------------------------------------------------------ fp32 emulation
def _lrelu32(raw, slope, fault):
    return raw if fault == "slope1" else torch.where(raw > 0, raw, raw * torch.tensor(slope, dtype=F32))


def emu_forward(hop, x, a_src, a_dst, slope, fault=None):
    """k_gat_mh_agg_fwd / k_gat_fwd: online softmax over a row in the kernel's order, every row at once"""
    x, a_src, a_dst = x.float(), a_src.float(), a_dst.float()
    T, H, K = hop.T, a_src.size(1), x.size(1)
    seq = hop.seq.clone()
    if fault == "drop_last_of_65":
        seq[hop.kept == 65, 65] = -1
    if fault == "swap_heads":
        a_dst = a_dst[:, [h ^ 1 for h in range(H)]]
    xn = x.clone()
    if fault == "column":
        xn[:, K - 1] = x[:, K - 2]
    mm = _lrelu32(a_src[:T] + a_dst, slope, fault)
    ss = torch.ones((T, H), dtype=F32)
    acc = x[:T].unsqueeze(1).repeat(1, H, 1)
    for p in range(1, seq.size(1)):
        on = (seq[:, p] >= 0).unsqueeze(1)
        j = hop.s[seq[:, p].clamp(min=0)]
        sc = _lrelu32(a_src[j] + a_dst, slope, fault)
        new = on & (sc > mm)
        r = torch.where(new, torch.exp(mm - sc), torch.ones((), dtype=F32))
        acc = acc * r.unsqueeze(2)
        if fault != "no_rescale":
            ss = ss * r
        mm = torch.where(new, sc, mm)
        w = torch.where(on, torch.exp(sc - mm), torch.zeros((), dtype=F32))
        ss = ss + w
        acc = acc + w.unsqueeze(2) * xn[j].unsqueeze(1)
    return acc * (1.0 / ss).unsqueeze(2), mm, ss


def emu_backward(hop, x, a_src, a_dst, slope, z, m, ssum, g, fault=None):
    """k_gat_mh_agg_bwd / k_gat_bwd: (grad_x atomic form, grad_a_src, grad_a_dst, alpha per softmax entry)"""
    x, a_src, a_dst, g = x.float(), a_src.float(), a_dst.float(), g.float()
    T, S, H, K = hop.T, hop.S, a_src.size(1), x.size(1)
    inv_s = 1.0 / ssum
    go = (g * z).sum(2)
    gad, gas = torch.zeros((T, H), dtype=F32), torch.zeros((S, H), dtype=F32)
    gx, alpha = torch.zeros((S, K), dtype=F32), torch.zeros((hop.r.numel(), H), dtype=F32)
    sl = torch.tensor(slope, dtype=F32)
    for p in range(hop.seq.size(1)):
        idx = hop.seq[:, p]
        on = idx >= 0
        j = hop.s[idx.clamp(min=0)]
        raw = a_src[j] + a_dst
        a = torch.exp(_lrelu32(raw, slope, None) - m) * inv_s
        gh = (g * x[j].unsqueeze(1)).sum(2)
        ge = a * (gh - go) * torch.where(raw > 0, torch.ones((), dtype=F32), sl)
        ge = torch.where(on.unsqueeze(1), ge, torch.zeros((), dtype=F32))
        if not (fault == "no_self_in_gad" and p == 0):
            gad = gad + ge
        gas.index_add_(0, j[on], ge[on])
        part = torch.zeros((T, K), dtype=F32)
        for h in range(H):
            part = part + a[:, h].unsqueeze(1) * g[:, h]
        gx.index_add_(0, j[on], part[on])
        alpha[idx[on]] = a[on]
    return gx, gas, gad, alpha


def emu_gather(hop, g, alpha_e, alpha_self, gas, gad, V):
    """k_gat_mh_gx_gather: one accumulator per source, every term added on its own"""
    g, V = g.float(), V.float()
    T, S, H = hop.T, hop.S, g.size(1)
    acc = torch.zeros((S, g.size(2)), dtype=F32)
    for h in range(H):
        acc = acc + gas[:, h].unsqueeze(1) * V[0, h]
    for h in range(H):
        acc[:T] = acc[:T] + gad[:, h].unsqueeze(1) * V[1, h]
        acc[:T] = acc[:T] + alpha_self[:, h].unsqueeze(1) * g[:, h]
    for k in range(hop.E):
        t, s = int(hop.row[k]), int(hop.col[k])
        for h in range(H):
            acc[s] = acc[s] + alpha_e[k, h] * g[t, h]
    return acc


def emu_all(hop, x, V, a_src, a_dst, g, slope, fault=None):
    """every kernel output of one training step's GAT aggregation, each stage fed the previous stage's fp32 output"""
    H = a_src.size(1)
    z, m, ssum = emu_forward(hop, x, a_src, a_dst, slope, fault)
    gx, gas, gad, alpha = emu_backward(hop, x, a_src, a_dst, slope, z, m, ssum, g, fault)
    alpha_e = torch.zeros((hop.E, H), dtype=F32)
    alpha_e[hop.eid] = alpha[:hop.nk]
    out = dict(z=z, row_max=m, row_sum=ssum, gx=gx, gas=gas, gad=gad, alpha_e=alpha_e, alpha_self=alpha[hop.nk:])
    if V is not None:
        out["gx_gather"] = emu_gather(hop, g, alpha_e, out["alpha_self"], gas, gad, V)
    return out


def ratios(hop, x, V, a_src, a_dst, g, slope, got):
    """err / bound per output quantity (the largest over its elements)"""
    bw = G.backward(hop, x, a_src, a_dst, g, slope, V)
    fw = bw.fw
    pairs = dict(z=(fw.z, fw.bz), row_sum=(fw.row_sum, fw.bs), gx=(bw.gx, bw.b_gx), gas=(bw.gas, bw.b_gas),
                 gad=(bw.gad, bw.b_gad), alpha_e=(bw.alpha_e, bw.b_alpha_e), alpha_self=(bw.alpha_self, bw.b_alpha_self))
    if V is not None:
        pairs["gx_gather"] = (bw.gx_gather, bw.b_gx_gather)
    out = {k: G.worst(got[k], ref, b, hop) for k, (ref, b) in pairs.items()}
    exact = torch.equal(got["row_max"], G.row_max32(hop, a_src, a_dst, slope))
    out["row_max"] = (0.0 if exact else float("inf"), "row_max is compared bit for bit")
    return out


# ------------------------------------------------------------------------------------------------ gradients
def _plain_formula(hop, x, a_src, a_dst, slope):
    """row by row, nothing shared with gat_f64.forward"""
    rows = []
    for t in range(hop.T):
        c = hop.col[int(hop.rowptr[t]):int(hop.rowptr[t + 1])]
        idx = torch.cat([c[c != t], torch.tensor([t])])
        e = torch.nn.functional.leaky_relu(a_src[idx] + a_dst[t], slope)           # [n, H]
        rows.append(torch.einsum("nh,nk->hk", torch.softmax(e, 0), x[idx]))
    return torch.stack(rows)


@pytest.mark.parametrize("S", [200, 70])
@pytest.mark.parametrize("H", [1, 2, 4])
def test_closed_form_gradients_are_autograds(H, S):
    hop = G.planted_hop(70, S)
    K = 12
    x, V, g = (t.double() for t in G.values(S, 70, K, H, F32))
    V = 3 * V                                               # logits of both signs, well apart
    close = functools.partial(torch.testing.assert_close, rtol=1e-10, atol=1e-13)
    for slope in G.SLOPES:
        # the aggregation alone: the atomic form's gradients
        xl, asl = x.clone().requires_grad_(True), (x @ V[0].t()).requires_grad_(True)
        adl = (x[:70] @ V[1].t()).requires_grad_(True)
        zf = _plain_formula(hop, xl, asl, adl, slope)
        zf.backward(g)
        bw = G.backward(hop, x, asl.detach(), adl.detach(), g, slope, V)
        close(bw.fw.z, zf.detach())
        close(bw.gas, asl.grad)
        close(bw.gad, adl.grad)
        close(bw.gx, xl.grad)
        assert abs(float(bw.alpha_e.sum() + bw.alpha_self.sum()) - 70 * H) < 1e-9
        # the whole layer: the gather form's grad_x and grad_V
        xl, Vl = x.clone().requires_grad_(True), V.clone().requires_grad_(True)
        _plain_formula(hop, xl, xl @ Vl[0].t(), xl[:70] @ Vl[1].t(), slope).backward(g)
        close(bw.gx_gather, xl.grad)
        close(G.logits_backward(x, bw.gas, bw.gad, 70)[0], Vl.grad)


# ------------------------------------------------------------------------------------------------ bounds
def _case(K, H, name, dtype=F32):
    T, S = shape_of(K) if K in WIDTHS else (70, 200)
    hop = G.planted_hop(T, S)
    x, V, g = G.values(S, T, K, H, dtype)
    a_src, a_dst = logits_of(name, hop, x, V)
    return hop, x, V, a_src, a_dst, g


def _honest(K, H, name, slope, gather=True, dtype=F32):
    hop, x, V, a_src, a_dst, g = _case(K, H, name, dtype)
    V = V if gather else None
    got = emu_all(hop, x, V, a_src, a_dst, g, slope)
    res = ratios(hop, x, V, a_src, a_dst, g, slope, got)
    bad = {k: v for k, v in res.items() if not v[0] <= 0.5}
    assert not bad, (K, H, name, slope, bad)
    assert all(torch.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("name", ["model"] + G.REGIMES)
@pytest.mark.parametrize("K", WIDTHS)
def test_an_honest_fp32_run_stays_within_half_of_every_bound(K, name):
    _honest(K, 2, name, G.SLOPES[0], gather=K <= 64)
    if K == 8:
        for H in (1, 4, 8):
            _honest(K, H, name, G.SLOPES[1], dtype=torch.bfloat16 if H == 4 else torch.float16)


@pytest.mark.parametrize("name", ["model"] + G.REGIMES)
def test_an_honest_fp32_run_of_the_full_width_kernels_stays_within_half_of_every_bound(name):
    for F in OLD_WIDTHS:
        _honest(F, 1, name, G.SLOPES[F % 2], gather=False)


def test_an_honest_fp32_run_of_the_logits_and_their_gradient_stays_within_half_of_every_bound():
    for K in WIDTHS:
        T, S = shape_of(K)
        x, V, g = G.values(S, T, K, 2, F32)
        lg = G.logits(x, V, T)
        a_src, a_dst = model_logits(x, V, T)
        assert G.worst(a_src, lg.a_src, lg.b_src)[0] <= 0.5 and G.worst(a_dst, lg.a_dst, lg.b_dst)[0] <= 0.5
        gas, gad = torch.randn((S, 2), generator=torch.Generator().manual_seed(K)), g[:, :, 0].contiguous()
        gv, b = G.logits_backward(x, gas, gad, T)
        got = torch.stack([gas.t() @ x, gad.t() @ x[:T]])
        assert G.worst(got, gv, b)[0] <= 0.5


FAULTS = ["drop_last_of_65", "keep_diag", "no_rescale", "slope1", "swap_heads", "column", "no_self_in_gad"]


@pytest.mark.parametrize("fault", FAULTS)
def test_a_planted_fault_exceeds_a_bound(fault):
    K, H = 8, 2
    for name in ("model", "equal", "ascending", "mixed"):
        hop, x, V, a_src, a_dst, g = _case(K, H, name)
        slope = G.SLOPES[0]
        run_on = G.Hop(hop.rowptr, hop.col, hop.T, hop.S, keep_diag=True) if fault == "keep_diag" else hop
        got = emu_all(run_on, x, None, a_src, a_dst, g, slope, fault)
        res = ratios(hop, x, None, a_src, a_dst, g, slope, got)
        over = {k: v[0] for k, v in res.items() if v[0] > 1.0}
        if over:
            return
    pytest.fail(f"{fault}: inside every bound in every regime tried")


@pytest.mark.parametrize("fault,name,outputs", [
    ("drop_last_of_65", "equal", ["z", "row_sum"]), ("keep_diag", "model", ["z", "row_sum"]),
    ("no_rescale", "ascending", ["row_sum", "z"]), ("slope1", "mixed", ["z", "row_max"]),
    ("swap_heads", "model", ["z"]), ("column", "model", ["z"]), ("no_self_in_gad", "model", ["gad"]),
])
def test_a_planted_fault_shows_where_it_should(fault, name, outputs):
    K, H = 8, 2
    hop, x, V, a_src, a_dst, g = _case(K, H, name)
    run_on = G.Hop(hop.rowptr, hop.col, hop.T, hop.S, keep_diag=True) if fault == "keep_diag" else hop
    got = emu_all(run_on, x, None, a_src, a_dst, g, G.SLOPES[0], fault)
    res = ratios(hop, x, None, a_src, a_dst, g, G.SLOPES[0], got)
    assert any(res[k][0] > 1.0 for k in outputs), {k: res[k] for k in outputs}


# ------------------------------------------------------------------------------------------------ the planted hop
@pytest.mark.parametrize("S", [200, 70])
def test_the_planted_hop_has_its_stated_properties(S):
    T = 70
    hop = G.planted_hop(T, S)
    cnt = (hop.rowptr[1:] - hop.rowptr[:-1]).tolist()
    kept = hop.kept.tolist()
    assert kept[:13] == G.COUNTS and set(kept) == set(G.COUNTS) and kept[69] == 130
    rows = [hop.col[int(hop.rowptr[t]):int(hop.rowptr[t + 1])].tolist() for t in range(T)]
    assert cnt[13] == 3 and rows[13] == [13, 13, 13] and kept[13] == 0                   # diagonal entries only
    assert cnt[0] == 0 and cnt[26] == 0 and cnt[65] == 0                                 # empty rows
    for t, pos, k in ((5, 0, 5), (18, 5, 5), (31, 2, 5), (11, 0, 65), (24, 65, 65), (37, 33, 65)):
        assert kept[t] == k and cnt[t] == k + 1 and rows[t][pos] == t, t                 # first, last, mid-round
    assert 33 % 4 != 0 and 33 % 4 != 3 and 2 % 4 == 2
    for t in range(T):
        mine = [j for j in rows[t] if j != t]
        if len(mine) >= 2:
            assert mine[1] == mine[0], t                                                 # the first source twice
        if len(mine) >= 3:
            assert G.HUB_LO in mine and hop.hub_hi in mine, t                            # both hubs
        if len(mine) == 1:
            assert mine == [hop.hub_hi]
    assert G.HUB_LO < T and (hop.hub_hi >= T or S == T) and kept[G.HUB_LO] == 0
    assert bool((hop.listed[S - 10:] == 0).all()) and int(hop.col.max()) == S - 11
    sink = G.sinks(hop)
    assert bool(((hop.s[:hop.nk] > hop.r[:hop.nk]) | sink[hop.s[:hop.nk]]).all())        # what lets a self loop be extreme
    # wavefront sharing at 8 targets a wavefront: 130 beside an empty row, and in the last wavefront with t = 70, 71 absent
    assert kept[25] == 130 and cnt[26] == 0 and 25 // 8 == 26 // 8
    assert kept[64] == 130 and cnt[65] == 0 and kept[69] == 130 and 69 // 8 == 64 // 8 == (T + 1) // 8 and T % 8 == 6
    # the entry list and the kernels' order
    assert hop.nk == sum(kept) and hop.seq.shape == (T, 131) and bool((hop.seq[:, 0] == hop.nk + torch.arange(T)).all())
    assert sorted(hop.seq[hop.seq >= 0].tolist()) == list(range(hop.nk + T))
    one, perm = hop.one_row(37)
    assert one.T == 1 and int(one.kept[0]) == 65 and int(one.listed.sum()) == 66 and perm[0] == 37 and perm[37] == 0


@pytest.mark.parametrize("S", [200, 70])
@pytest.mark.parametrize("H", [1, 8])
def test_the_logit_regimes_are_what_they_are_called(H, S):
    hop = G.planted_hop(70, S)
    T, nk = hop.T, hop.nk
    full = hop.n >= 2

    def per_row(name, slope=G.SLOPES[0]):
        a_src, a_dst = G.regime(name, hop, H)
        raw = (a_src[hop.s] + a_dst[hop.r]).double()
        assert bool((raw != 0).all()) and float(raw.abs().max()) < 128
        assert bool(((a_src.double() / G.Q) % 2 == 0).all()) and bool(((a_dst.double() / G.Q) % 2 == 1).all())
        e = torch.cat([G.lrelu(raw, slope), torch.full((1, H), float("nan"), dtype=torch.float64)])[hop.seq]
        return raw, e, G.forward(hop, torch.zeros((S, 4)), a_src, a_dst, slope)

    on = (hop.seq[:, 1:] >= 0).unsqueeze(2)
    _, e, fw = per_row("ascending")
    assert bool(((e[:, 1:] >= e[:, :-1]) | ~on).all()) and bool((fw.R[full] >= 1).all())
    short = hop.n <= 4                                     # a rescale at every edge but the repeated first source's
    assert bool((fw.R[short] == (hop.n - 1 - (hop.n >= 3).long())[short].unsqueeze(1)).all())
    assert S == T or int(fw.R.max()) >= 64                 # (longer rows draw their sources with repeats)
    _, e, fw = per_row("descending")
    assert bool(((e[:, 1:] <= e[:, :-1]) | ~on).all()) and bool((fw.R == 0).all())       # never
    _, e, fw = per_row("equal")
    assert bool(((e[:, 1:] == e[:, :1]) | ~on).all()) and bool((fw.R == 0).all())
    for name, sign in (("selfmax", 1.0), ("selfmin", -1.0)):
        _, e, fw = per_row(name)
        assert bool(((sign * (e[:, :1] - e[:, 1:]) > 0) | ~on).all())
    assert bool((fw.R[full] >= 1).all())                                                 # selfmin: the first edge rescales
    raw, _, _ = per_row("mixed")
    pos = torch.zeros((T, H)).index_add_(0, hop.r, (raw > 0).float())
    assert bool(((pos >= 1) & (pos < hop.n.unsqueeze(1)))[full].all())
    _, _, fw = per_row("wide")
    assert float(fw.d.max()) > 104 and float(torch.exp(-fw.d).min()) < 2.0 ** -149       # below the smallest subnormal
    assert bool((fw.d.max() <= 120))
