"""Float64 restatement of the edge-weighted aggregation kernels (csrc/aggregate_weighted.hip: k_agg_w_fwd, k_agg_w_bwd,
k_agg_w_wgrad, k_gcn_dinv / k_gcn_coef; csrc/transpose_hop.hip.h with edge ids: the transposed hop the backward walks)
with a per-element rounding bound next to every value, and the weights the tests put on the planted hops of
tests/agg_f64.py.  A helper: no tests in here.  Everything is on the CPU, vectorised, in float64; the fp32 / fp16 / bf16
rows and gradients and the fp32 weights convert to float64 exactly, and so does a product of two of them (24 + 24 bits).

The formulas.  Entry k of row t names source col k and carries w_k; targets are the first T sources.
  forward   out[t]        = sum_{k in row t} w_k x[col k]  (+ self_w_t x[t])
  backward  grad_x[s]     = sum_{k = (t, s)} w_k g[t]      (+ self_w_s g[s] for s < T)
  wgrad     grad_w[k]     = <g[t], x[col k]>,   grad_self_w[t] = <g[t], x[t]>
  gcn_norm  D_t = fill + sum_{k in row t} w_k,  dinv_t = D_t^-1/2 (0 where D_t = 0);  a source that is no target has
            D = fill;  coef[k] = dinv_t w_k dinv_{col k},  self_coef[t] = fill dinv_t^2

The bounds.  u = 2^-24.  M is always the reference expression with every term replaced by its absolute value.  The build
passes no fast-math flag, so nothing is re-associated and an fmaf is one rounding.
  forward / backward: every value is ONE fmaf onto the accumulator -- the row's entries in CSR order, a source's
            entries in ascending CSR position (the order k_tr_order leaves), the self term last; the pairs of the
            loops are two fmafs one after the other, the same chain.  Unlike the mean's first addition, the first fmaf
            rounds too (fl(w x + 0): the product has 48 bits), so n values are n roundings, each relative u of a partial
            sum that M bounds: n u M, with n = the row's length (the source's in-degree) + [the self term].  A zero
            weight still counts as a value (its fmaf rounds nothing): the bound is an upper bound.
            n = 0: exactly 0.  n = 1: the value is the single rounding of w x, an exact float64 product rounded to fp32
            here: bound 0.
  wgrad:    the call takes the vector form (pieces of 4 columns) when F % 4 == 0 and rows and gradient are aligned to 4
            elements with strides that are multiples of 4, else the scalar form (pieces of 1).  lpr = 2^lanes_log2(pieces)
            lanes share a row: the first power of two that covers the pieces, 64 at most.  A round is kWgradSteps = 4
            column steps of lpr pieces.  In a round a lane fmafs its columns in column order onto 0 (m values, m
            roundings, m <= 4 * the piece's width), group_sum adds log2(lpr) times (a fixed butterfly; a lane without
            columns adds an exact 0, which the count ignores: an upper bound), and every round after the first is one
            more addition onto the stored value.  A term of round 0 or 1 meets every later round's addition, so the
            longest path has c = m + log2(lpr) + (rounds - 1) roundings, m = min(4, ceil(F / (lpr * width))) * width:
            c u M.  F = 1028 in the vector form: 16 + 6 + 1 = 23; F = 300 in the scalar form: 4 + 6 + 1 = 11; F = 1: c = 1,
            the single rounding of g x: bound 0.
  gcn_norm: weights are non-negative, so every partial sum of a row is at most D_t and the bound is relative.  The row
            sum is a sequential chain from 0 (the first addition is exact): d - 1 roundings, and fill + s is one more
            when fill != 0; without weights s = (float) d and fill + s are exact.  a_t counts them: D is within a_t u.
            sqrtf and the division are correctly rounded: the build passes neither a fast-math flag nor
            -fno-hip-fp32-correctly-rounded-divide-sqrt, and clang's HIP default (-fhip-fp32-correctly-rounded-divide-sqrt,
            the clang command line reference) makes fp32 / and sqrt in device code correctly rounded -- what
            agg_f64.py assumes of the division.  So dinv_t is within delta_t = (a_t / 2 + 2) u: half the radicand's
            error, the root's rounding, the quotient's.  A source that is no target reads the host's 1.0f / sqrtf(fill):
            exact for fill = 1, 2 u for fill = 2, an exact 0 for fill = 0.
            coef = fl(fl(dinv_t w) dinv_s): delta_t + delta_s + 2 u (+ 1 u without weights: dinv_t * 1.f is exact).
            self_coef = fl(fl(dinv_t fill) dinv_t): fill is 1 or 2, the first product exact: 2 delta_t + u.
            D_t = 0 (fill 0 and an empty or all-zero row): sqrtf(0) = 0, 1 / 0 = inf, dinv = 0 exactly: every coef that
            touches t, as row or as source, and self_coef[t] are exactly 0; so is every coef of a zero weight.
  a bf16 / fp16 result: agg_f64.rounded (one rounding to nearest of a value within its bound).
  Second order: the longest chain here has 885 values (the tall hop's hub): 885 u = 5.3e-5, below 2^-11, so products of
            two first-order terms are below 2^-11 of the bound: every bound is multiplied by G2 = 1 + 2^-10.
None of these constants comes from GPU output."""
import functools
import types

import torch

import agg_f64 as A
import gat_f64 as G

U, G2, F64 = G.U, G.G2, G.F64
WGRAD_STEPS = 4                                            # kWgradSteps
FILLS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def weights(name):
    """(w [E], self_w [T]) in fp32 for the hop `name`: seeded normal draws, negative and positive; every seventh w is
    exactly 0 -- but never two entries of one (t, s) pair, so the entries of a repeated pair always carry DIFFERENT
    weights (a second zero keeps its draw); self_w[1], [12], [23], ... are exactly 0"""
    hop = A.hop_of(name)
    g = torch.Generator().manual_seed(4242 + 1000 * hop.T + hop.S)
    w = torch.randn(hop.E, generator=g)
    zero = torch.arange(hop.E) % 7 == 0
    key, seen = (hop.row * hop.S + hop.col).tolist(), set()
    for k in torch.nonzero(zero).flatten().tolist():
        zero[k] = key[k] not in seen
        seen.add(key[k])
    w[zero] = 0.0
    sw = torch.randn(hop.T, generator=g)
    sw[1::11] = 0.0
    return w, sw


def zero_row(name):
    """the target whose weights gcn_weights makes all zero (its first row of 3 entries), or None (T <= 1, no such row)"""
    hop = A.hop_of(name)
    rows = torch.nonzero(hop.deg == 3).flatten()
    return int(rows[0]) if hop.T > 1 and rows.numel() else None


@functools.lru_cache(maxsize=None)
def gcn_weights(name):
    """|w| of weights(name) -- non-negative, zeros included -- with the whole of zero_row(name) set to 0: under fill 0
    that row's D is 0 although the row has entries"""
    hop = A.hop_of(name)
    w = weights(name)[0].abs()
    t = zero_row(name)
    if t is not None:
        w[int(hop.rowptr[t]):int(hop.rowptr[t + 1])] = 0.0
    return w


class Case:
    """a hop with its weights: W [T, S] float64 the weights summed per (target, source), Wa the same of |w|"""

    def __init__(self, hop, w, sw):
        self.hop, self.w, self.sw = hop, w, sw
        assert w.shape == (hop.E,) and sw.shape == (hop.T,) and w.dtype == sw.dtype == torch.float32

    def _dense(self, v):
        return torch.zeros((self.hop.T, self.hop.S), dtype=F64).index_put_((self.hop.row, self.hop.col), v, accumulate=True)

    @functools.cached_property
    def W(self):
        return self._dense(self.w.double())

    @functools.cached_property
    def Wa(self):
        return self._dense(self.w.double().abs())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(A.hop_of(name), *weights(name))


def _chain(ref, M, n, out_dtype):
    """(ref, bound) of n [rows, 1] fmafs onto a zero accumulator, stored as out_dtype"""
    b = G2 * U * n * M
    single = (n == 1).expand_as(ref)
    ref = torch.where(single, ref.float().double(), ref)
    b = torch.where(single, torch.zeros_like(b), b)
    return A.rounded(ref, b, out_dtype)


def forward(c, x, self_w, out_dtype=torch.float32):
    """(ref, bound) [T, F] of k_agg_w_fwd; self_w: whether c.sw is passed"""
    xd, T = x.double(), c.hop.T
    ref, M = c.W @ xd, c.Wa @ xd.abs()
    n = c.hop.deg.double().unsqueeze(1)
    if self_w:
        own = c.sw.double().unsqueeze(1) * xd[:T]
        ref, M, n = ref + own, M + own.abs(), n + 1
    return _chain(ref, M, n, out_dtype)


def backward(c, g, self_w, out_dtype=torch.float32):
    """(ref, bound) [S, F] of k_agg_w_bwd; g [T, F]"""
    gd, T = g.double(), c.hop.T
    ref, M = c.W.t() @ gd, c.Wa.t() @ gd.abs()
    n = c.hop.indeg.double().unsqueeze(1)
    if self_w:
        own = c.sw.double().unsqueeze(1) * gd
        ref[:T] += own
        M[:T] += own.abs()
        n = n + (torch.arange(c.hop.S) < T).double().unsqueeze(1)
    return _chain(ref, M, n, out_dtype)


def wgrad_shape(F, vec):
    """the lane partition of k_agg_w_wgrad: width (columns a piece), lpr, log2 lpr, step (columns a column step), rounds,
    m (the most columns a lane holds in a round), c (the roundings on the longest path)"""
    assert F >= 1 and (not vec or F % 4 == 0)
    width = 4 if vec else 1
    pieces = F // width
    log2 = 0
    while (1 << log2) < pieces and log2 < 6:               # lanes_log2 (csrc/elem_io.hip.h)
        log2 += 1
    lpr = 1 << log2
    step = lpr * width
    rounds = -(-F // (step * WGRAD_STEPS))
    m = min(WGRAD_STEPS, -(-F // step)) * width
    return types.SimpleNamespace(width=width, lpr=lpr, log2=log2, step=step, rounds=rounds, m=m,
                                 c=m + log2 + rounds - 1)


def wgrad(c, x, g, vec):
    """(grad_w [E], bound, grad_self_w [T], bound) of k_agg_w_wgrad in the form the call takes (vec: the vector form)"""
    xd, gd, hop = x.double(), g.double(), c.hop
    cnt = wgrad_shape(xd.size(1), vec).c

    def dots(a, b):
        ref, M = (a * b).sum(1), (a * b).abs().sum(1)
        if cnt == 1:
            return ref.float().double(), torch.zeros_like(M)
        return ref, G2 * U * cnt * M

    return dots(gd[hop.row], xd[hop.col]) + dots(gd, xd[:hop.T])


def gcn_norm(hop, w, fill):
    """(coef [E], bound, self_coef [T], bound) of spp_gcn_norm; w [E] fp32, non-negative, or None (ones); fill 0, 1, 2"""
    assert fill in FILLS and (w is None or bool((w >= 0).all()))
    T, weighted = hop.T, w is not None
    wd = w.double() if weighted else torch.ones(hop.E, dtype=F64)
    D = fill + torch.zeros(T, dtype=F64).index_add_(0, hop.row, wd)
    dinv = torch.where(D > 0, D.clamp(min=1e-300).pow(-0.5), torch.zeros_like(D))
    a = torch.clamp(hop.deg.double() - 1, min=0) + (1.0 if fill else 0.0) if weighted else torch.zeros(T, dtype=F64)
    delta = (a / 2 + 2) * U
    is_t = hop.col < T
    at = hop.col.clamp(max=max(T - 1, 0))
    foreign, foreign_delta = (fill ** -0.5 if fill else 0.0), (2 * U if fill == 2 else 0.0)
    if T:
        ds = torch.where(is_t, dinv[at], torch.full_like(wd, foreign))
        dls = torch.where(is_t, delta[at], torch.full_like(wd, foreign_delta))
    else:
        ds, dls = torch.full_like(wd, foreign), torch.full_like(wd, foreign_delta)
    coef = dinv[hop.row] * wd * ds
    b_coef = G2 * (delta[hop.row] + dls + (2 if weighted else 1) * U) * coef.abs()
    self_coef = fill * dinv * dinv
    return coef, b_coef, self_coef, G2 * (2 * delta + U) * self_coef
