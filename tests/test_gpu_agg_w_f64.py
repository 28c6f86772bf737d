"""-m gpu: the edge-weighted aggregation kernels (csrc/aggregate_weighted.hip, csrc/transpose_hop.hip.h with edge ids)
through weighted_aggregate, gcn_norm and the raw entry spp_agg_weighted_backward, against the float64 restatement and
the per-element bounds of tests/agg_w_f64.py, on the planted hops of tests/agg_f64.py: hub sources, repeated (target,
source) pairs that carry different weights, rows of 63 to 130, empty rows, sources nobody names, a tall hop of three
k_tr_count / k_tr_fill workgroups, and T = 0, E = 0, T = 1, S = T = 1.

Every element of every output is compared: the share of elements or cases left out is 0.  An element whose bound is 0
-- an empty row, a row or segment of one value (the single rounding of w x), a source nobody names, a dot product of one
column, a coefficient that touches a target of degree 0 -- must be exactly its reference.  The forward and the weights'
gradient go through weighted_aggregate and autograd; the input's gradient fills the descriptor here, because grad_x and
the workspace start as NaN and the gradient is a slice of a buffer 4 columns wider with NaN in the spare columns.
Nothing is sampled.

Each test prints AGG_W_F64_RATIO <quantity> <largest err / bound>: a record, never an input to the bounds.  The values
seen on an MI355X are in the docstring of test_zz_largest_ratios_seen."""
import collections
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_f64 as A  # noqa: E402
import agg_w_f64 as W  # noqa: E402
from test_gpu_agg_f64 import _P, _csr, _nat, _same, _source, _st  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAN = float("nan")
ALL_WIDTHS = A.WIDTHS + [1024]
WGRAD_WIDTHS = ALL_WIDTHS + [300, 1028]                    # the second register round, scalar and vector form
SOURCES = ["dense", "slice", "one_in", "table", "refs"]
GCN_HOPS = ["planted", "square", "tall", "E0", "T1", "T1S1"]
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SEEN = collections.defaultdict(float)                      # quantity -> largest err / bound over the session


class Checks:
    """collects (quantity, err / bound, where); done() prints the record and names every quantity over its bound"""

    def __init__(self):
        self.tag, self.bad, self.top = "", [], collections.defaultdict(float)

    def within(self, what, got, ref, bound):
        assert tuple(got.shape) == tuple(ref.shape), (what, self.tag, got.shape, ref.shape)
        ratio, where = A.worst(got, ref, bound)
        self.top[what] = max(self.top[what], ratio)
        SEEN[what] = max(SEEN[what], ratio)
        if not ratio <= 1.0:
            self.bad.append(f"{what} [{self.tag}] err/bound {ratio:.3f} at {where}")

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what} [{self.tag}] does not hold")

    def done(self):
        for k, v in sorted(self.top.items()):
            print(f"\nAGG_W_F64_RATIO {k} {v:.3f}", end="")
        print()
        assert not self.bad, "\n".join(self.bad[:20])


def _hops_for(F):
    return ["square"] if F in (300, 1024, 1028) else A.hops_for(F)


@functools.lru_cache(maxsize=None)
def _weights(name):
    """(w, self_w) of the hop `name` on the GPU"""
    c = W.case(name)
    return c.w.cuda(), c.sw.cuda()


def _agg(hop, src, w, sw, amp=False):
    from salient_plusplus_amd.models import weighted_aggregate
    rowptr, col = _csr(hop)
    hop = A.hop_of(hop) if isinstance(hop, str) else hop
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        return weighted_aggregate(src, rowptr, col, w, hop.T, sw)


# ------------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=192)
def _fwd_ref(name, F, xdt, self_w, odt):
    c = W.case(name)
    return W.forward(c, A.values(c.hop.S, F, xdt), self_w, odt)


@pytest.mark.parametrize("F,kind", [(F, k) for F in ALL_WIDTHS for k in SOURCES])
def test_forward_within_its_bound_and_identical_twice(F, kind):
    """one_in forces the scalar form at F % 4 == 0; slice and table keep NaN next to every row"""
    c = Checks()
    for name in A.hops_for(F):
        hop = A.hop_of(name)
        w, sw = _weights(name)
        for xdt in (F32, F16, BF16):
            src = _source(kind, A.values(hop.S, F, xdt))
            for self_w in (False, True):
                long = hop.deg + int(self_w) >= 32
                for odt in (F32, BF16):
                    c.tag = f"{name} {kind} x {xdt} out {odt} self_w {self_w}"
                    out, again = (_agg(name, src, w, sw if self_w else None, odt == BF16) for _ in range(2))
                    assert out.dtype == odt
                    ref, b = _fwd_ref(name, F, xdt, self_w, odt)
                    c.within("forward", out, ref, b)
                    if odt == F32:                             # (a record of the chains alone: no bf16 rounding on top)
                        c.within("forward/fp32-rows>=32", out[long], ref[long], b[long])
                    c.exact("bound 0 on the rows of no or one value",
                            bool((b[hop.deg + int(self_w) <= 1] == 0).all()))
                    c.exact("forward twice", _same(out, again))
    c.done()


@pytest.mark.parametrize("F", [8, 65, 260])
def test_a_row_of_130_gives_the_same_bits_alone(F):
    """rows 12 and 25 (130 entries, next to a short and to an empty row) against the hop of that row alone, its weights
    and its self weight cut the same way"""
    hop = A.hop_of("planted")
    w, sw = _weights("planted")
    for xdt in (F32, F16):
        x = A.values(hop.S, F, xdt)
        for self_w in (False, True):
            full = _agg("planted", x.cuda(), w, sw if self_w else None)
            for t in (12, 25):
                assert int(hop.deg[t]) == 130
                one, perm = hop.one_row(t)
                w1 = w[int(hop.rowptr[t]):int(hop.rowptr[t + 1])].contiguous()
                alone = _agg(one, x[perm].cuda(), w1, sw[t:t + 1].contiguous() if self_w else None)
                assert _same(alone, full[t:t + 1].contiguous()), (xdt, self_w, t)


# ------------------------------------------------------------------------------------------------ backward
def _grad_buf(hop, F, gdt):
    """the gradient [T, F] as a slice of a buffer 4 columns wider with NaN in the spare columns; (cpu values, slice)"""
    g = A.values(hop.T, F, gdt, seed=9)
    buf = torch.full((hop.T, F + 4), NAN, dtype=gdt, device="cuda")
    buf[:, :F] = g.cuda()
    return g, buf[:, :F]


def _backward(hop, gs, w, sw, F, odt, fill=NAN):
    """spp_agg_weighted_backward with grad_x pre-filled with NaN and the workspace with `fill` (a float, or a byte)"""
    nat, L = _nat()
    rowptr, col = _csr(hop)
    T, S, E = hop.T, hop.S, hop.E
    assert gs.shape == (T, F) and w.shape == (E,) and (sw is None or sw.shape == (T,)) and w.dtype == F32
    assert rowptr.numel() == T + 1 and col.numel() == E and (E == 0 or (0 <= int(hop.col.min()) and int(hop.col.max()) < S))
    grad_x = torch.full((S, F), NAN, dtype=odt, device="cuda")
    nbytes = int(L.spp_agg_weighted_backward_workspace_bytes(T, S, E))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = (torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda") if isinstance(fill, int)
          else torch.full((nbytes // 4,), fill, dtype=F32, device="cuda"))
    ELEM = {F32: nat.SPP_ELEM_F32, BF16: nat.SPP_ELEM_BF16}
    d = nat.AggWeightedBwdDesc(grad_elem=ELEM[gs.dtype], out_elem=ELEM[odt], rowptr_dev=_P(rowptr), col_dev=_P(col),
                               num_targets=T, num_sources=S, num_edges=E, grad_out_dev=_P(gs),
                               grad_out_stride_elems=gs.stride(0), F=F, w_dev=_P(w), self_w_dev=_P(sw),
                               grad_x_dev=_P(grad_x))
    nat.check(L.spp_agg_weighted_backward(C.byref(d), _P(ws), nbytes, _st()))
    return grad_x


@pytest.mark.parametrize("self_w", [False, True], ids=["plain", "self_w"])
@pytest.mark.parametrize("F", ALL_WIDTHS)
def test_backward_within_its_bound(F, self_w):
    """all four (gradient, grad_x) pairs of fp32 / bf16 on every hop; a source nobody names is exactly 0, and for s < T
    with self_w exactly the single rounding of self_w_s g_s: those elements' bound is 0"""
    c = Checks()
    for name in A.hops_for(F):
        cs = W.case(name)
        hop = cs.hop
        w, sw = _weights(name)
        n = hop.indeg + (torch.arange(hop.S) < hop.T).long() * int(self_w)
        long = n >= 32
        for gdt in (F32, BF16):
            g, gs = _grad_buf(hop, F, gdt)
            for odt in (F32, BF16):
                c.tag = f"{name} g {gdt} grad_x {odt}"
                gx = _backward(hop, gs, w, sw if self_w else None, F, odt)
                ref, b = W.backward(cs, g, self_w, odt)
                c.within("grad_x", gx, ref, b)
                if odt == F32:
                    c.within("grad_x/fp32-segments>=32", gx[long], ref[long], b[long])
                c.exact("bound 0 on the sources of no or one value", bool((b[n <= 1] == 0).all()))
                c.exact("exactly 0 where nobody names the source", bool((gx[(n == 0).cuda()] == 0).all()))
                c.exact("the spare columns stay NaN", bool(torch.isnan(gs._base[:, F:]).all()))
    c.done()


@pytest.mark.parametrize("self_w", [False, True], ids=["plain", "self_w"])
@pytest.mark.parametrize("F", [8, 130, 260])
def test_backward_over_the_tall_hop_is_identical_twice_over_any_workspace_and_cut_down_to_a_hub(F, self_w):
    """k_tr_fill / k_tr_order with edge ids across three workgroups: hub segments of 885 and 828 entries filled by three
    workgroups' atomics, which k_tr_order must put into one order, with the weight of each entry.  Twice over a NaN
    workspace, once over a workspace of 0xA5 bytes; then a hub's row of grad_x against the hop cut down to the entries
    naming it, the weights cut the same way: the same targets and weights in the same order"""
    hop = A.hop_of("tall")
    w, sw = _weights("tall")
    sw = sw if self_w else None
    for gdt, odt in ((F32, F32), (BF16, BF16)):
        _g, gs = _grad_buf(hop, F, gdt)
        one, two = (_backward(hop, gs, w, sw, F, odt) for _ in range(2))
        three = _backward(hop, gs, w, sw, F, odt, fill=0xA5)
        assert not bool(torch.isnan(one).any())
        assert _same(one, two) and _same(one, three), (gdt, odt)
        for s in hop.hubs:
            assert int(hop.indeg[s]) > 600
            cut = _backward(hop.one_source(s), gs, w[(hop.col == s).cuda()].contiguous(), sw, F, odt)
            assert _same(cut[s], one[s]), (gdt, odt, s)


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrads(name, src, g, self_w, amp):
    """(grad_weight, grad_self_weight) through torch.autograd on weighted_aggregate"""
    w, sw = _weights(name)
    wq = w.clone().requires_grad_(True)
    sq = sw.clone().requires_grad_(True) if self_w else None
    out = _agg(name, src, wq, sq, amp)
    assert out.dtype == g.dtype
    out.backward(g)
    return wq.grad, (sq.grad if self_w else None)


@pytest.mark.parametrize("F", WGRAD_WIDTHS)
def test_wgrad_within_its_bound_identical_twice_and_over_every_source(F):
    """dense, TableRows and RowRefs read the same rows in the same form: the same bits.  one_in (a misaligned base: the
    scalar form at every width) is held to the scalar form's bound"""
    c = Checks()
    for name in _hops_for(F):
        cs = W.case(name)
        hop = cs.hop
        for xdt in (F32, F16, BF16):
            x = A.values(hop.S, F, xdt)
            srcs = {k: _source(k, x) for k in ("dense", "table", "refs", "one_in")}
            for amp in (False, True):
                g = A.values(hop.T, F, BF16 if amp else F32, seed=9)
                gd = g.cuda()
                for self_w in (False, True):
                    c.tag = f"{name} x {xdt} amp {amp} self_w {self_w}"
                    got = {k: _wgrads(name, s, gd, self_w, amp) for k, s in srcs.items()}
                    again = _wgrads(name, srcs["dense"], gd, self_w, amp)
                    for k, (gw, gsw) in got.items():
                        rw, bw, rs, bs = W.wgrad(cs, x, g, F % 4 == 0 and k != "one_in")
                        assert gw.dtype == F32 and gw.shape == (hop.E,)
                        c.within("grad_w", gw, rw, bw)
                        if self_w:
                            assert gsw.dtype == F32
                            c.within("grad_self_w", gsw, rs, bs)
                        if F >= 32:
                            c.within("grad_w/columns>=32", gw, rw, bw)
                    for k in ("table", "refs"):
                        c.exact(f"{k} as dense", _same(got[k][0], got["dense"][0]) and
                                (not self_w or _same(got[k][1], got["dense"][1])))
                    c.exact("wgrad twice", _same(again[0], got["dense"][0]) and
                            (not self_w or _same(again[1], got["dense"][1])))
    c.done()


# ------------------------------------------------------------------------------------------------ gcn_norm
@pytest.mark.parametrize("fill", W.FILLS)
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_gcn_norm_within_its_bound_and_identical_twice(weighted, fill):
    """rows of 130 (one thread walks them), three workgroups of targets, a row whose weights are all 0 and targets without
    entries: under fill 0 every coefficient touching them is exactly 0 (their bound is 0)"""
    from salient_plusplus_amd.models import gcn_norm
    kw = {0: dict(add_self_loops=False), 1: dict(), 2: dict(improved=True)}[fill]
    c = Checks()
    for name in GCN_HOPS:
        hop = A.hop_of(name)
        rowptr, col = _csr(name)
        w = W.gcn_weights(name) if weighted else None
        wd = w.cuda() if weighted else None
        c.tag = f"{name} fill {fill} weighted {weighted}"
        (coef, self_coef), (c2, s2) = (gcn_norm(rowptr, col, hop.T, wd, **kw) for _ in range(2))
        assert coef.dtype == self_coef.dtype == F32
        rc, bc, rs, bs = W.gcn_norm(hop, w, fill)
        c.within("gcn_norm/coef", coef, rc, bc)
        c.within("gcn_norm/self_coef", self_coef, rs, bs)
        long = hop.deg[hop.row] >= 32
        c.within("gcn_norm/coef/rows>=32", coef[long.cuda()], rc[long], bc[long])
        c.exact("gcn_norm twice", _same(coef, c2) and _same(self_coef, s2))
        if fill == 0:
            D = torch.zeros(hop.T, dtype=A.F64).index_add_(0, hop.row, w.double() if weighted else torch.ones(hop.E, dtype=A.F64))
            dead = torch.cat([D == 0, torch.ones(hop.S - hop.T, dtype=torch.bool)])
            touched = dead[hop.row] | dead[hop.col]
            t = W.zero_row(name)
            c.exact("a zero-sum row", not weighted or t is None or (int(hop.deg[t]) > 0 and bool(dead[t])))
            c.exact("exact zeros where D = 0", bool((bc[touched] == 0).all()) and bool((coef.cpu()[touched] == 0).all())
                    and bool((self_coef == 0).all()))
            c.exact("and only there", hop.E == 0 or weighted or bool((coef.cpu()[~touched] > 0).all()))
    c.done()


# ------------------------------------------------------------------------------------------------ autograd wrapper
WRAPPED = [("planted", 8, F16, False), ("planted", 6, BF16, False), ("planted", 8, F32, True), ("tall", 12, F32, True),
           ("T1", 8, F32, False), ("T1S1", 8, F32, False), ("T0", 8, F32, False), ("E0", 8, F32, False)]


@pytest.mark.parametrize("name,F,xdt,amp", WRAPPED, **_ID)
def test_autograd_wrapper_within_the_same_bounds(name, F, xdt, amp):
    """weighted_aggregate through .backward() with x, weight and self_weight requiring grad: an fp16 input (its gradient
    is cast by the wrapper), a bf16 input at a scalar width, bf16 autocast, T = 1 (the stride-0 spelling gs = 0) and
    the empty hops"""
    cs = W.case(name)
    hop = cs.hop
    x = A.values(hop.S, F, xdt)
    odt = BF16 if amp else F32
    c = Checks()
    c.tag = f"{name} F {F} x {xdt} amp {amp}"
    w, sw = _weights(name)
    xq, wq, sq = x.cuda().requires_grad_(True), w.clone().requires_grad_(True), sw.clone().requires_grad_(True)
    out = _agg(name, xq, wq, sq, amp)
    assert out.dtype == odt and out.shape == (hop.T, F)
    c.within("wrapper/forward", out.detach(), *W.forward(cs, x, True, odt))
    g = A.values(hop.T, F, odt, seed=9)
    out.backward(g.cuda())
    gdt = xdt if xdt in (F32, BF16) else F32                   # grad_x's type before the wrapper's cast
    ref, b = W.backward(cs, g, True, gdt)
    if xdt != gdt:
        ref, b = A.rounded(ref, b, xdt)
    assert xq.grad.dtype == xdt and xq.grad.shape == (hop.S, F)
    c.within("wrapper/grad_x", xq.grad, ref, b)
    rw, bw, rs, bs = W.wgrad(cs, x, g, F % 4 == 0)
    assert wq.grad.shape == (hop.E,) and sq.grad.shape == (hop.T,)
    c.within("wrapper/grad_w", wq.grad, rw, bw)
    c.within("wrapper/grad_self_w", sq.grad, rs, bs)
    c.done()


def test_zz_largest_ratios_seen():
    """asserts every err / bound recorded by the tests of this module that ran before it is <= 1, and prints them.

    Seen on an MI355X (a record, not an input to the bounds).  Every element: forward 0.996, grad_x 0.996, grad_w 0.892,
    grad_self_w 0.881, gcn_norm coef 0.500 and self_coef 0.557; the wrapper: forward 0.979, grad_x 0.981, grad_w 0.541,
    grad_self_w 0.330.  The first two sit next to 1 because a bound of ONE rounding has no slack -- a bf16 result, a
    row of two values -- not because a chain ran out of room.  Where the chain is all of the bound: the fp32 results of
    rows of 32 values or more 0.078, of segments of 32 or more 0.086 (the host emulation: 0.086); dot products of 32
    columns or more 0.204 (the emulation: 0.204); gcn_norm's coefficients on rows of 32 or more 0.397 (the emulation:
    0.397).  This file and test_gpu_agg_weighted.py together: 206 tests in 7.8 s; the slowest test of this file 0.44 s
    (the first forward case, which loads the library), every other one 0.3 s or less."""
    print("\nAGG_W_F64_LARGEST " + " ".join(f"{k}={v:.3f}" for k, v in sorted(SEEN.items())))
    assert all(v <= 1.0 for v in SEEN.values()), {k: v for k, v in SEEN.items() if not v <= 1.0}
