"""CPU: the float64 restatement of the mean / operand / sum aggregation in tests/agg_f64.py checked on its own.  Its
closed-form gradients against torch.autograd of an independent float64 formula; its bounds against an fp32 (and
bf16-rounding) emulation of the kernels' order of operations -- an honest one stays within HALF of every bound at every
width and element type tests/test_gpu_agg_f64.py uses, each planted fault exceeds a bound somewhere -- and the
properties the planted hops are documented to have.

Where the half is asked (_margin).  A bound that counts one or two roundings is attained by honest arithmetic: one
rounding to nearest reaches u of the value (1 + 2^-8 rounds to 1 in bf16), a row of two or three entries reaches nearly
all of its 1 or 2 u.  No emulation stays within half of such a bound, and doubling it would hide the faults it is
there for (a second rounding to bf16, a reciprocal of the wrong row).  A bound of c roundings is only reached when all c
err the same way, so the half is asked where c >= 32 -- the fp32 result of a row (a source) of 32 or more entries: the rows of 63 to 130,
the hubs' segments, the tall hop's planted segments of 63 to 65 -- at every
width and input type -- and every element, short chains and bf16 / fp16 results included, is held to its whole
bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_f64 as A  # noqa: E402
import gat_f64 as G  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL_WIDTHS = A.WIDTHS + [1024]
_ID = dict(ids=lambda v: str(v).split(".")[-1])


# ------------------------------------------------------------------------------------------------ fp32 emulation
def _fma(a, b, c):
    """fmaf: the product is exact in float64; (the float64 sum's own rounding is 2^-29 of fp32's)"""
    return (a.double() * b.double() + c.double()).float()


def _inv32(hop, plus=0):
    return 1.0 / (hop.deg + plus).clamp(min=1).float()


def _segments(key, n, order=None):
    """[n, L] entry ids per key value, -1 padded, in `order` (a permutation of the entries; default: ascending id)"""
    E = key.numel()
    order = torch.arange(E) if order is None else order
    idx = order[torch.sort(key[order], stable=True).indices]
    cnt = torch.bincount(key, minlength=n)
    seg = torch.full((n, max(int(cnt.max()) if n and E else 0, 1)), -1, dtype=torch.int64)
    start = torch.cumsum(cnt, 0) - cnt
    k = key[idx]
    seg[k, torch.arange(E) - start[k]] = idx
    return seg, cnt


def _out(acc, dtype):
    return acc if dtype == F32 else acc.to(dtype)


def emu_forward(hop, x, epilogue, scale=0.0, out_dtype=F32, inv=None, keep=None, fault=None):
    """k_agg_fwd: a row's entries in CSR order into a zero accumulator (the pairs of the vector form are added one after
    the other: the same chain), fmaf(s, x_t, acc) for the sum, acc * inv for the mean; every row at once.
    keep [E] bool: the entries a faulty kernel still reads; inv: the reciprocal it uses"""
    xf = x.float()
    T, F = hop.T, xf.size(1)
    if fault == "column":
        xf = xf.clone()
        xf[:, F - 1] = xf[:, F - 2]
    ids = torch.arange(hop.E) if keep is None else torch.nonzero(keep).flatten()
    seg, cnt = _segments(hop.row[ids], T)
    acc = torch.zeros((T, F), dtype=F32)
    for k in range(seg.size(1) if ids.numel() else 0):
        live = torch.nonzero(cnt > k).flatten()
        if fault == "bf16_partial":                           # the accumulator through bf16 before a row's last entry
            last = live[cnt[live] == k + 1]
            acc[last] = acc[last].bfloat16().float()
        acc[live] += xf[hop.col[ids[seg[live, k]]]]
    if epilogue == A.SUM:
        if A.fl32(scale) != 0:
            acc = _fma(torch.tensor(A.fl32(scale), dtype=F32), xf[:T], acc)
    else:
        acc = acc * (_inv32(hop) if inv is None else inv).unsqueeze(1)
        if epilogue == A.OPERAND:
            acc = torch.cat([acc, xf[:T]], 1)
    return _out(acc, out_dtype)


def _finish(acc, epilogue, mask, act_scale, out_dtype):
    if epilogue == A.OPERAND_ACT:
        acc = torch.where(mask, acc * torch.tensor(A.fl32(act_scale), dtype=F32), torch.zeros((), dtype=F32))
    return _out(acc, out_dtype)


def emu_gather(hop, g, epilogue, scale=0.0, mask=None, act_scale=2.0, out_dtype=F32, contract=False, inv=None,
               keep=None, fault=None, fault_at=None):
    """k_agg_bwd_gather over the ordered transposed hop: a source's entries in ascending CSR position, two at a time
    (acc += g0 w0 + g1 w1) plus an odd tail; the operand's target term first, the sum's fmaf(s, g_j, acc) last.
    contract: the compiler fused each product into the addition after it"""
    gf = g.float()
    T, S = hop.T, hop.S
    summ = epilogue == A.SUM
    F = gf.size(1) if summ else gf.size(1) // 2
    if fault == "column":
        gf = gf.clone()
        gf[:, F - 1] = gf[:, F - 2]
    ids = torch.arange(hop.E) if keep is None else torch.nonzero(keep).flatten()
    seg, cnt = _segments(hop.col[ids], S)
    if fault == "drop_tail":
        assert int(cnt[fault_at]) % 2 == 1
        cnt = cnt.clone()
        cnt[fault_at] -= 1
    inv = _inv32(hop) if inv is None else inv
    if fault == "inv_of_source":
        inv_s = torch.cat([inv, torch.ones(S - T, dtype=F32)])
    acc = torch.zeros((S, F), dtype=F32)
    if not summ and fault != "no_self":
        acc[:T] = gf[:, F:]

    def term(rows, k):
        """(g row [:, :F], weight [:, 1]) of the k-th entry of the sources `rows`"""
        t = hop.row[ids[seg[rows, k]]]
        w = torch.ones(rows.numel(), dtype=F32) if summ else inv_s[rows] if fault == "inv_of_source" else inv[t]
        return gf[t, :F], w.unsqueeze(1)

    for k in range(0, seg.size(1) if ids.numel() else 0, 2):
        two, one = torch.nonzero(cnt > k + 1).flatten(), torch.nonzero(cnt == k + 1).flatten()
        if fault == "bf16_partial":                           # the accumulator through bf16 before the last addition
            last = torch.cat([two[cnt[two] == k + 2], one])
            acc[last] = acc[last].bfloat16().float()
        if two.numel():
            (v0, w0), (v1, w1) = term(two, k), term(two, k + 1)
            acc[two] += _fma(v1, w1, v0 * w0) if contract else v0 * w0 + v1 * w1
        if one.numel():
            v0, w0 = term(one, k)
            acc[one] = _fma(v0, w0, acc[one]) if contract else acc[one] + v0 * w0
    if summ and A.fl32(scale) != 0 and fault != "no_self":
        acc[:T] = _fma(torch.tensor(A.fl32(scale), dtype=F32), gf, acc[:T])
    return _finish(acc, epilogue, mask, act_scale, out_dtype)


def emu_scatter(hop, g, epilogue, scale=0.0, mask=None, act_scale=2.0, out_dtype=F32, order_seed=0, inv=None, keep=None,
                fault=None):
    """k_grad_init / k_sum_grad_init / a zero fill, then k_agg_bwd_scatter's atomics -- each entry's fl(g w) added to its
    source's row in a seeded random order -- then the activation's backward and / or the rounding pass"""
    gf = g.float()
    T, S = hop.T, hop.S
    summ = epilogue == A.SUM
    F = gf.size(1) if summ or epilogue == A.MEAN else gf.size(1) // 2
    if fault == "column":
        gf = gf.clone()
        gf[:, F - 1] = gf[:, F - 2]
    ids = torch.arange(hop.E) if keep is None else torch.nonzero(keep).flatten()
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(order_seed))
    seg, cnt = _segments(hop.col[ids], S, perm)
    acc = torch.zeros((S, F), dtype=F32)
    if fault != "no_self":
        if summ:
            acc[:T] = torch.tensor(A.fl32(scale), dtype=F32) * gf
        elif epilogue != A.MEAN:
            acc[:T] = gf[:, F:]
    t = hop.row[ids]
    terms = gf[t, :F] if summ else gf[t, :F] * (_inv32(hop) if inv is None else inv)[t].unsqueeze(1)
    for k in range(seg.size(1) if ids.numel() else 0):
        live = torch.nonzero(cnt > k).flatten()
        acc[live] += terms[seg[live, k]]
    return _finish(acc, epilogue, mask, act_scale, out_dtype)


# ------------------------------------------------------------------------------------------------ the cases
FWD_EPILOGUES = [(A.MEAN, 0.0), (A.OPERAND, 0.0), (A.SUM, 0.0), (A.SUM, A.SCALE)]
BWD_FORMS = [(A.MEAN, "scatter"), (A.OPERAND, "scatter"), (A.OPERAND, "gather"), (A.OPERAND_ACT, "scatter"),
             (A.OPERAND_ACT, "gather"), (A.SUM, "scatter"), (A.SUM, "gather")]
# the operand's gradient has the vector form only
BWD_CASES = [(F, e, f) for F in ALL_WIDTHS for e, f in BWD_FORMS if e in (A.MEAN, A.SUM) or F % 4 == 0]


def _grad(hop, F, epilogue, dtype):
    return A.values(hop.T, F if epilogue in (A.MEAN, A.SUM) else 2 * F, dtype, seed=9)


LONG = 32


def _margin(acc, length, make, odts=(F32, BF16)):
    """acc: the emulation's fp32 result; length: the entries behind each of its rows; make(odt) -> (ref, bound).  The
    rows of LONG entries or more within half of the fp32 bound, every element within the whole bound, also once rounded
    to each other output type (see the module docstring); the long rows' ratio"""
    ref, b = make(F32)
    r, where = _ratio(acc, ref, b)
    assert r <= 1.0, (r, where)
    long = length >= LONG
    r, where = _ratio(acc[long], ref[long], b[long])
    assert r <= 0.5, (r, where)
    for odt in odts:
        if odt != F32:
            ro, where = _ratio(acc.to(odt), *make(odt))
            assert ro <= 1.0, (odt, ro, where)
    return r


def _ratio(got, ref, b, hop=None):
    return A.worst(got, ref, b, hop if hop is not None and got.size(0) == hop.T else None)


@pytest.mark.parametrize("F", ALL_WIDTHS)
def test_honest_forward_emulation_stays_within_half_of_every_bound(F):
    """every hop, epilogue, x and output type of the GPU file at this width"""
    top = 0.0
    for name in A.hops_for(F):
        hop = A.hop_of(name)
        for xdt in (F32, F16, BF16):
            x = A.values(hop.S, F, xdt)
            for epilogue, scale in FWD_EPILOGUES:
                acc = emu_forward(hop, x, epilogue, scale)
                top = max(top, _margin(acc, hop.deg, lambda odt: A.forward(hop, x, epilogue, scale, odt)))
    print(f"\nAGG_F64_HOST forward F {F}: largest err / bound {top:.3f}")


@pytest.mark.parametrize("F,epilogue,form", BWD_CASES)
def test_honest_backward_emulation_stays_within_half_of_every_bound(F, epilogue, form):
    """every hop, gradient and grad_x type of the GPU file at this width: the gather with and without contraction, the
    scatter in three random orders (one on the hops whose longest chain is short)"""
    top = 0.0
    for name in A.hops_for(F):
        hop = A.hop_of(name)
        mask = A.keep_mask(hop.S, F)
        for gdt in (F32, BF16):
            g = _grad(hop, F, epilogue, gdt)
            kw = dict(scale=A.SCALE, act_scale=2.0)
            if form == "gather":
                runs = [emu_gather(hop, g, epilogue, mask=mask, contract=c, **kw) for c in (False, True)]
            else:
                runs = [emu_scatter(hop, g, epilogue, mask=mask, order_seed=i, **kw)
                        for i in range(3 if name in A.HOPS and F <= 260 else 1)]
            for acc in runs:
                top = max(top, _margin(acc, hop.indeg,
                                        lambda odt: A.backward(hop, g, epilogue, form, A.SCALE, mask, 2.0, odt)))
    print(f"\nAGG_F64_HOST {epilogue} {form} F {F}: largest err / bound {top:.3f}")


def test_honest_emulation_of_the_wrappers_extra_roundings():
    """the fp16 cast of a gradient, the non-vector operand's scatter-plus-add, an act_scale that is no power of two"""
    hop = A.hop_of("planted")
    g = _grad(hop, 6, A.OPERAND, F32)
    for odt in (F32, BF16):
        got = emu_scatter(hop, g[:, :6], A.MEAN, out_dtype=odt)
        got[:hop.T] += g[:, 6:].to(odt)
        ref, b = A.operand_fallback(hop, g, odt)
        assert _ratio(got, ref, b)[0] <= 1.0, odt
        long = hop.indeg >= LONG
        assert odt != F32 or _ratio(got[long], ref[long], b[long])[0] <= 0.5
    g = _grad(hop, 12, A.SUM, F32)
    _margin(emu_gather(hop, g, A.SUM, A.SCALE), hop.indeg,
            lambda odt: A.rounded(*A.backward(hop, g, A.SUM, "gather", A.SCALE), odt), (F32, F16))
    ref, b = A.rounded(*A.backward(hop, g, A.SUM, "gather", A.SCALE), F16)
    assert bool((b[hop.indeg == 0][hop.T:] == 0).all())
    mask, sc = A.keep_mask(hop.S, 12), A.fl32(1 / (1 - 0.3))
    g = _grad(hop, 12, A.OPERAND_ACT, F32)
    ref, b = A.backward(hop, g, A.OPERAND_ACT, "gather", keep=mask, act_scale=sc)
    _margin(emu_gather(hop, g, A.OPERAND_ACT, mask=mask, act_scale=sc), hop.indeg, lambda odt: (ref, b), (F32,))


# ------------------------------------------------------------------------------------------------ planted faults
def _row_of(hop, n):
    return int(torch.nonzero(hop.deg == n).flatten()[0])


def _first_of_pairs(hop):
    """keep [E]: one entry of every (t, s) pair"""
    key = hop.row * hop.S + hop.col
    keep = torch.ones(hop.E, dtype=torch.bool)
    order = torch.sort(key, stable=True).indices              # (equal pairs need not be adjacent)
    keep[order[1:]] = key[order[1:]] != key[order[:-1]]
    return keep


def _odd_hub(hop):
    odd = [s for s in hop.hubs if int(hop.indeg[s]) % 2 == 1]
    assert odd, "a hub of odd in-degree"
    return odd[0]


FAULTS = ["drop_last_of_65", "drop_tail_of_hub", "dedup_pairs", "inv_deg_plus_1", "no_self", "column", "inv_of_source"]
# every hop that has what the fault needs: the tall hop has no row of 65, the (70, 200) hop's hubs have even in-degrees
FAULT_CASES = [(f, h) for f in FAULTS for h in A.HOPS
               if (f, h) not in (("drop_last_of_65", "tall"), ("drop_tail_of_hub", "planted"))]


@pytest.mark.parametrize("fault,hop_name", FAULT_CASES)
def test_a_planted_fault_exceeds_a_bound(fault, hop_name):
    """fp32 output and fp32 gradient, so the bf16 term hides nothing.  Each fault is emulated in every kernel it can
    live in and must exceed that kernel's bound somewhere, on every hop that has what the fault needs"""
    hop = A.hop_of(hop_name)
    F = 8
    x = A.values(hop.S, F, F32)
    g1, g2 = _grad(hop, F, A.SUM, F32), _grad(hop, F, A.OPERAND, F32)
    fw = {e: A.forward(hop, x, e, s) for e, s in ((A.MEAN, 0.0), (A.SUM, A.SCALE))}
    bw = {(e, f): A.backward(hop, g1 if e in (A.SUM, A.MEAN) else g2, e, f, A.SCALE)
          for e, f in ((A.MEAN, "scatter"), (A.OPERAND, "scatter"), (A.OPERAND, "gather"), (A.SUM, "scatter"),
                       (A.SUM, "gather"))}
    each = []                                                  # every entry must exceed its bound on its own

    def fwd(epilogue, scale, **kw):
        each.append(_ratio(emu_forward(hop, x, epilogue, scale, **kw), *fw[epilogue])[0])

    def gat(epilogue, **kw):
        for c in (False, True):
            each.append(_ratio(emu_gather(hop, g1 if epilogue == A.SUM else g2, epilogue, A.SCALE, contract=c, **kw),
                               *bw[(epilogue, "gather")])[0])

    def sca(epilogue, **kw):
        gg = g1 if epilogue in (A.SUM, A.MEAN) else g2
        each.append(_ratio(emu_scatter(hop, gg, epilogue, A.SCALE, **kw), *bw[(epilogue, "scatter")])[0])

    if fault == "drop_last_of_65":
        keep = torch.ones(hop.E, dtype=torch.bool)
        keep[int(hop.rowptr[_row_of(hop, 65) + 1]) - 1] = False
        fwd(A.MEAN, 0.0, keep=keep), fwd(A.SUM, A.SCALE, keep=keep)
        sca(A.MEAN, keep=keep), sca(A.SUM, keep=keep), gat(A.OPERAND, keep=keep)
    elif fault == "drop_tail_of_hub":
        s = _odd_hub(hop)
        gat(A.OPERAND, fault="drop_tail", fault_at=s), gat(A.SUM, fault="drop_tail", fault_at=s)
    elif fault == "dedup_pairs":
        keep = _first_of_pairs(hop)
        assert int(keep.sum()) < hop.E
        gat(A.OPERAND, keep=keep), gat(A.SUM, keep=keep), sca(A.OPERAND, keep=keep), fwd(A.MEAN, 0.0, keep=keep)
    elif fault == "inv_deg_plus_1":
        inv = _inv32(hop, 1)
        fwd(A.MEAN, 0.0, inv=inv), gat(A.OPERAND, inv=inv), sca(A.OPERAND, inv=inv), sca(A.MEAN, inv=inv)
    elif fault == "no_self":
        gat(A.OPERAND, fault=fault), gat(A.SUM, fault=fault), sca(A.OPERAND, fault=fault), sca(A.SUM, fault=fault)
    elif fault == "column":
        fwd(A.MEAN, 0.0, fault=fault), fwd(A.SUM, A.SCALE, fault=fault)
        gat(A.OPERAND, fault=fault), gat(A.SUM, fault=fault), sca(A.MEAN, fault=fault), sca(A.SUM, fault=fault)
    else:
        gat(A.OPERAND, fault=fault)
    assert each and min(each) > 1.0, (fault, each)
    _margin(emu_forward(hop, x, A.MEAN), hop.deg, lambda odt: fw[A.MEAN], (F32,))
    _margin(emu_gather(hop, g2, A.OPERAND, A.SCALE), hop.indeg, lambda odt: bw[(A.OPERAND, "gather")], (F32,))


@pytest.mark.parametrize("hop_name", A.HOPS)
def test_a_partial_sum_rounded_to_bf16_exceeds_the_bf16_bounds(hop_name):
    """the bf16-output case: the accumulator rounded to bf16 once, before a row's (a source's) last term"""
    hop = A.hop_of(hop_name)
    F = 8
    x, g = A.values(hop.S, F, BF16), _grad(hop, F, A.OPERAND, BF16)
    for epilogue in (A.MEAN, A.SUM):
        ref, b = A.forward(hop, x, epilogue, 0.0, BF16)
        assert _ratio(emu_forward(hop, x, epilogue, out_dtype=BF16), ref, b)[0] <= 1.0
        assert _ratio(emu_forward(hop, x, epilogue, out_dtype=BF16, fault="bf16_partial"), ref, b)[0] > 1.0
    ref, b = A.backward(hop, g, A.OPERAND, "gather", out_dtype=BF16)
    for c in (False, True):
        assert _ratio(emu_gather(hop, g, A.OPERAND, out_dtype=BF16, contract=c), ref, b)[0] <= 1.0
        assert _ratio(emu_gather(hop, g, A.OPERAND, out_dtype=BF16, contract=c, fault="bf16_partial"), ref, b)[0] > 1.0


# ------------------------------------------------------------------------------------------------ closed forms
def _formula(hop, x, epilogue, scale):
    """an independent float64 statement: one index_add over the entries"""
    s = torch.zeros((hop.T, x.size(1)), dtype=A.F64).index_add(0, hop.row, x[hop.col])
    if epilogue == A.SUM:
        return A.fl32(scale) * x[:hop.T] + s
    mean = s / hop.deg.clamp(min=1).double().unsqueeze(1)
    return mean if epilogue == A.MEAN else torch.cat([mean, x[:hop.T]], 1)


@pytest.mark.parametrize("hop_name", A.HOPS + A.DEGENERATE)
@pytest.mark.parametrize("epilogue", [A.MEAN, A.OPERAND, A.OPERAND_ACT, A.SUM])
def test_closed_forms_agree_with_autograd_of_an_independent_formula(epilogue, hop_name):
    hop = A.hop_of(hop_name)
    F = 5
    mask, sc = A.keep_mask(hop.S, F), A.fl32(1 / (1 - 0.3))
    z = A.values(hop.S, F, F32).double().requires_grad_(True)
    x = z * mask.double() * sc if epilogue == A.OPERAND_ACT else z
    kind = A.OPERAND if epilogue == A.OPERAND_ACT else epilogue
    out = _formula(hop, x, kind, A.SCALE)
    g = _grad(hop, F, epilogue, F32)
    (out * g.double()).sum().backward()
    if epilogue != A.OPERAND_ACT:
        ref, b = A.forward(hop, A.values(hop.S, F, F32), kind, A.SCALE)
        want = torch.where(b == 0, out.detach().float().double(), out.detach())     # (a single rounding: as fp32)
        torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-14)
    for form in ("scatter", "gather") if epilogue != A.MEAN else ("scatter",):
        ref, b = A.backward(hop, g, epilogue, form, A.SCALE, mask, sc)
        want = torch.where(b == 0, z.grad.float().double(), z.grad)
        torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-14)
        assert bool((b >= 0).all()) and bool(torch.isfinite(b).all())


# ------------------------------------------------------------------------------------------------ the hops
@pytest.mark.parametrize("name", ["planted", "square"])
def test_the_planted_hops_have_their_documented_properties(name):
    hop = A.hop_of(name)
    T, S = hop.T, hop.S
    assert (T, S) == ((70, 200) if name == "planted" else (70, 70))
    assert set(G.COUNTS) <= set(hop.deg.tolist())              # out-degrees 0, 1, ..., 9, 63, 64, 65, 130
    deg = hop.deg.tolist()
    assert any(deg[t] == 0 and max(deg[t - 1], deg[t + 1]) >= 65 for t in range(1, T - 1))      # empty next to long
    pairs = hop.row * S + hop.col
    assert pairs.unique().numel() < hop.E                      # rows repeat a source
    assert bool((hop.col < T).any()) and bool((hop.col == hop.row).any())                       # target and self edges
    lo, hi = hop.hubs
    assert lo < T and (hi >= T or S == T) and lo != hi
    others = hop.indeg.clone()
    others[list(hop.hubs)] = 0
    assert min(int(hop.indeg[lo]), int(hop.indeg[hi])) >= 50                                    # two hub sources
    assert S == T or int(others.max()) < 40                    # (the square hop's few sources are all named often)
    assert int(hop.deg[lo]) == 0                               # a hub target whose own row is empty
    assert bool((hop.indeg[S - 10:] == 0).all())               # the last 10 sources are named by nobody
    assert bool((hop.indeg[:T] == 0).any())                    # ... and so is a target: exactly its own term


def test_the_tall_hop_has_its_documented_properties():
    hop = A.hop_of("tall")
    T, S = hop.T, hop.S
    assert (T, S) == (600, 900) and -(-T // 256) == 3          # three workgroups of k_tr_count / k_tr_fill
    assert set(hop.deg.tolist()) == set(range(10)) and bool((hop.deg[::7] == 0).all())
    lo, hi = hop.hubs
    assert lo < T <= hi and int(hop.deg[lo]) == 0
    for s in hop.hubs:
        assert 600 <= int(hop.indeg[s]) <= 2000
        per_row = torch.bincount(hop.row[hop.col == s], minlength=T)
        assert int((per_row >= 1).sum()) > T // 2 and int((per_row >= 2).sum()) > 50           # most rows; some twice
    assert any(int(hop.indeg[s]) % 2 == 1 for s in hop.hubs)   # an odd tail on a hub's segment
    for s, k in A.TALL_PLANTED.items():
        assert int(hop.indeg[s]) == k
        if k >= 63:                                            # a segment filled from all three workgroups
            assert set((hop.row[hop.col == s] // 256).tolist()) == {0, 1, 2}
    assert {1, 3, 63, 65} & set(A.TALL_PLANTED.values()) and {2, 64} & set(A.TALL_PLANTED.values())
    others = hop.indeg.clone()
    others[list(hop.hubs) + list(A.TALL_PLANTED)] = 0
    assert int(others.max()) == 1
    assert bool((hop.indeg[S - 10:] == 0).all()) and bool((hop.indeg[:T] == 0).any())
    pairs = hop.row * S + hop.col
    assert pairs.unique().numel() < hop.E


def test_the_degenerate_and_switch_hops():
    shapes = {n: (A.hop_of(n).T, A.hop_of(n).S, A.hop_of(n).E) for n in A.DEGENERATE}
    assert shapes == {"T0": (0, 5, 0), "E0": (3, 5, 0), "T1": (1, 5, 3), "T1S1": (1, 1, 3)}
    for E in (4095, 4097):
        hop = A.switch_hop(E)
        assert hop.E == E and (E * 1024 >= 1 << 22) == (E > 4096)
        assert int(hop.indeg[5]) > 1000 and bool((hop.indeg[hop.S - 10:] == 0).all())
    hop = A.hop_of("planted")
    t = _row_of(hop, 130)
    one, perm = hop.one_row(t)
    assert one.T == 1 and one.E == 130 and torch.equal(perm[one.col], hop.col[hop.rowptr[t]:hop.rowptr[t + 1]])
    cut = hop.one_source(hop.hubs[0])
    assert cut.E == int(hop.indeg[hop.hubs[0]]) and torch.equal(cut.row, hop.row[hop.col == hop.hubs[0]])
