"""Float64 restatement of the mean / operand / sum aggregation kernels (csrc/aggregate.hip: k_agg_fwd,
k_agg_bwd_scatter, k_agg_bwd_gather, k_grad_init, k_sum_grad_init, k_relu_dropout_bwd_pre; csrc/transpose_hop.hip.h: the
transposed hop the gather walks) with a per-element rounding bound next to every value, and the planted hops the tests
run them on.  A helper: no tests in here.  Everything is on the CPU, vectorised, in float64; the fp32 / fp16 / bf16
inputs convert to float64 exactly.

The formulas.  n_t = deg t, inv_t = 1 / max(n_t, 1), cnt_s = the entries naming s (repeats counted), A[t, s] = the number
of entries (t, s); targets are the first T sources.
  forward   mean[t]    = inv_t sum_{e in row t} x[col e]                 operand[t] = [mean[t] | x[t]]
            sum[t]     = s x[t] + sum_{e in row t} x[col e]              (s is the fp32 number the kernel receives)
  backward  mean:        grad_x[j] = sum_{e: col e = j} g[row e] inv_{row e}
            operand:     grad_x[j] = (j < T ? g[j, F:2F] : 0) + the mean's, of g[:, :F]
            operand_act: the operand's, times keep[j, c] scale -- keep is the ReLU / dropout mask, an INPUT here
            sum:         grad_x[j] = (j < T ? s g[j] : 0) + sum_{e: col e = j} g[row e]

The bounds.  u = 2^-24.  M is always the reference expression with every term replaced by its absolute value.  A chain
of fp32 additions that joins m values, in ANY order (CSR order, pairs, atomics), is within (m - 1) u M of their exact
sum to first order: each value passes through at most m - 1 roundings, each relative u of a partial sum that M bounds.
An addition onto an exact 0 (a zeroed accumulator, a grad_x row that starts from 0) does not round, so a chain that starts
from zero counts one value less.  The build passes no fast-math flag: fp32 division is correctly rounded and sums are not
re-associated; products may be contracted into the addition that follows (fewer roundings, never more).
  inv:      fl(1 / n) is within u of inv_t, and exact when n is a power of two; a product by it rounds once more, unless n
            is a power of two.  r_t = 0 for n_t a power of two (or 0), else 2: the relative roundings of one value
            x inv_t or g inv_t (2 u, not 3: the reciprocal's and the product's).
  mean:     (max(n - 1, 0) + r_t) u M inv_t: the row's chain from a zero accumulator, then the product.  n = 1, 2, 4, ...
            leave the chain alone; n = 0 and n = 1 must be exact.
  operand:  the x_target half is a copy: bound 0.
  sum:      (max(n - 1, 0) + [s != 0]) u M: the chain, then ONE rounding for fmaf(s, x_t, acc).  n = 0: the value is the
            single rounding of s x_t (an exact product in float64 rounded to fp32 here): bound 0.
  scatter backward (atomics, any order; k_agg_bwd_scatter rounds g w once, w = fl(inv_t), then adds):
            sum_e r u |g| inv + adds u M.  adds = cnt_s - 1 for a row that starts from zero (the plain mean; j >= T), cnt_s
            for a target row of the operand (it starts from g[j, F:2F]).  The sum: the init pass rounds s g once, then
            cnt_s additions: (cnt_s + 1) u M for a target with s != 0 and cnt_s > 0, else (cnt_s - 1) u M.
  gather backward (k_agg_bwd_gather: ascending CSR position, acc += g0 w0 + g1 w1 per pair, odd tail, the operand's
            target term first, the sum's fmaf(s, g_j, acc) last): the same value count as the scatter -- cnt_s + 1 values
            for a target row, cnt_s otherwise, joined by pair and accumulator additions -- so adds is the same; each
            g inv is r u whether or not the compiler contracts the product; the sum's self term is one rounding less
            than the scatter's ((cnt_s - 1) + [j < T and s != 0]).
  exact 0s: a source nobody names has M = 0: it must be exactly 0, and for j < T exactly g[j, F:2F] (operand) or the
            single rounding of s g[j] (sum).  Masked elements of operand_act are exactly 0.
  operand_act: the kept elements are multiplied by scale = fl(1 / (1 - p)): exact when it is a power of two (p = 0.5),
            else one more u |ref|.
  a bf16 result (stored by the kernel, or by the rounding pass after a bf16 scatter): + 2^-8 (|ref| + bound), ONE rounding
            to nearest of a value within bound of ref: bf16 holds 8 significant bits, so half a unit in the last place is
            2^-8 of the value at worst (1 + 2^-8 rounds to 1); 2^-9 is exceeded by a single honest rounding.
            An fp16 gradient (the Python wrapper's .to(float16) of an fp32
            grad_x): + 2^-11 (|ref| + bound) + 2^-25 (fp16's subnormal spacing).  Where the bound before that rounding is
            0 the reference itself is rounded to the result's type and the bound stays 0.
  the wrapper's fallback for an operand of a non-vector width (models._MeanAggregate: the plain mean's scatter, then
            grad_x[:T] += g[:, F:].to(grad_x's type)): the mean's bound, its rounding to grad_x's type, the cast's rounding
            of g where the types differ, then one more rounding of that type for the addition (none where the mean's
            part is an exact 0).
  Second order: every relative first-order term above is below 2^-11 (2000 u = 1.2e-4 for the longest chain here), so
            products of two of them are below 2^-11 of the bound: every bound is multiplied by G2 = 1 + 2^-10; the
            rounding to bf16 / fp16 is applied to |ref| + bound, so its product with the rest is counted, not dropped.
None of these constants comes from GPU output."""
import functools

import numpy as np
import torch

import gat_f64 as G

U, G2, F64 = G.U, G.G2, G.F64
worst = G.worst
EPS = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MEAN, OPERAND, OPERAND_ACT, SUM = "mean", "operand", "operand_act", "sum"
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 12, 47, 64, 65, 130, 256, 260]        # + 1024 on the square hop only
VEC_WIDTHS = [w for w in WIDTHS if w % 4 == 0]
SCALE = 1.5
HOPS = ["planted", "square", "tall"]
DEGENERATE = ["T0", "E0", "T1", "T1S1"]


class Hop:
    """a CSR hop: row [E] the target of every entry, deg [T], indeg [S] (entries naming s), A [T, S] float64 counts"""

    def __init__(self, rowptr, col, T, S, hubs=()):
        self.rowptr, self.col, self.T, self.S, self.E, self.hubs = rowptr, col, T, S, int(col.numel()), tuple(hubs)
        assert rowptr.numel() == T + 1 and int(rowptr[-1]) == self.E
        self.deg = rowptr[1:] - rowptr[:-1]
        self.row = torch.repeat_interleave(torch.arange(T), self.deg)
        self.indeg = torch.bincount(col, minlength=S)
        self.n = self.deg                                      # (what gat_f64.worst names a row's length by)

    @functools.cached_property
    def A(self):
        one = torch.ones(self.E, dtype=F64)
        return torch.zeros((self.T, self.S), dtype=F64).index_put_((self.row, self.col), one, accumulate=True)

    def one_row(self, t):
        """row t alone as a T = 1 hop: target 0 is source t, so ids 0 and t trade places; (hop, perm): x1 = x[perm]"""
        b, e = int(self.rowptr[t]), int(self.rowptr[t + 1])
        col = self.col[b:e].clone()
        swap = col.clone()
        swap[col == t], swap[col == 0] = 0, t
        perm = torch.arange(self.S)
        perm[0], perm[t] = t, 0
        return Hop(torch.tensor([0, e - b]), swap, 1, self.S), perm

    def one_source(self, s):
        """the hop cut down to the entries naming s: every row keeps its place, the rows' lengths change"""
        keep = self.col == s
        deg = torch.bincount(self.row[keep], minlength=self.T)
        rowptr = torch.zeros(self.T + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(deg, 0)
        return Hop(rowptr, self.col[keep].clone(), self.T, self.S)


def _from_rows(rows, T, S, hubs=()):
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows], dtype=torch.int64), 0)
    return Hop(rowptr, torch.tensor([j for r in rows for j in r], dtype=torch.int64), T, S, hubs)


TALL_PLANTED = {21: 65, 701: 64, 702: 63, 703: 1, 704: 2, 28: 3}     # source -> in-degree (21 and 28 are targets)


@functools.lru_cache(maxsize=None)
def tall_hop():
    """(T, S) = (600, 900): three workgroups of k_tr_count / k_tr_fill.  Every seventh row is empty, the others have
    1 + t % 9 entries (so 0..9).  A row of d entries is [lo], [hi] (d = 1, by t's parity), [lo, hi], [lo, hi, lo],
    [lo, hi, lo, hi], or [lo, hi, d - 4 others, lo, hi]: the hubs lo = 14 (a target whose own row is empty) and hi = 700
    are named by most rows and twice by the rows of 3 or 4 and more, which brings their in-degrees above 600.  The others
    are a seeded shuffle of a pool that gives the sources of TALL_PLANTED exactly the in-degrees 65, 64, 63, 1, 2, 3 (their
    entries spread over all three workgroups; some rows name one of them twice) and names every further source at most
    once; the last 10 sources are named by nobody."""
    T, S, lo, hi = 600, 900, 14, 700
    degs = [0 if t % 7 == 0 else 1 + t % 9 for t in range(T)]
    n_other = sum(max(d - 4, 0) for d in degs)
    pool = [s for s, k in TALL_PLANTED.items() for _ in range(k)]
    cand = [j for j in range(S - 10) if j not in (lo, hi) and j not in TALL_PLANTED]
    pool += [cand[(37 * i) % len(cand)] for i in range(n_other - len(pool))]
    assert len(pool) == n_other and n_other - sum(TALL_PLANTED.values()) <= len(cand)
    perm = torch.randperm(n_other, generator=torch.Generator().manual_seed(600900)).tolist()
    pool = [pool[i] for i in perm]
    rows, at = [], 0
    for t, d in enumerate(degs):
        if d == 0:
            row = []
        elif d == 1:
            row = [lo if t % 2 else hi]
        elif d <= 4:
            row = [lo, hi, lo, hi][:d]
        else:
            row = [lo, hi] + pool[at:at + d - 4] + [lo, hi]
            at += d - 4
        rows.append(row)
    assert at == n_other
    return _from_rows(rows, T, S, (lo, hi))


@functools.lru_cache(maxsize=None)
def switch_hop(E):
    """(T, S) = (64, 100) with exactly E entries, for the wrappers' E * F >= 2^22 gather switch at F = 1024: rows of
    E // 64 or one more entries; every fourth entry of a row names the hub 5 (a target), the others walk the sources
    below 90 with a stride of 13 (repeats within a row); the last 10 sources are named by nobody"""
    T, S = 64, 100
    rows = [[5 if k % 4 == 0 else (7 * t + 13 * k) % (S - 10) for k in range(E // T + (1 if t < E % T else 0))]
            for t in range(T)]
    return _from_rows(rows, T, S, (5,))


@functools.lru_cache(maxsize=None)
def hop_of(name):
    if name in ("planted", "square"):
        h = G.planted_hop(70, 200 if name == "planted" else 70)
        return Hop(h.rowptr, h.col, h.T, h.S, (G.HUB_LO, h.hub_hi))
    if name == "tall":
        return tall_hop()
    none = torch.zeros(0, dtype=torch.int64)
    if name == "T0":
        return Hop(torch.zeros(1, dtype=torch.int64), none, 0, 5)
    if name == "E0":
        return Hop(torch.zeros(4, dtype=torch.int64), none, 3, 5)
    if name == "T1":
        return _from_rows([[0, 3, 3]], 1, 5)
    if name == "T1S1":
        return _from_rows([[0, 0, 0]], 1, 1)
    raise ValueError(name)


def hops_for(F, degenerate=True):
    """the hops a width runs on: every one, but 1024 on the square hop only"""
    return ["square"] if F == 1024 else HOPS + (DEGENERATE if degenerate else [])


@functools.lru_cache(maxsize=None)
def values(S, F, dtype, seed=0):
    """x [S, F] in dtype (also: a gradient [T, W] or a pre-activation z)"""
    g = torch.Generator().manual_seed(seed + 1000 * F + S)
    return (0.5 * torch.randn((S, F), generator=g)).to(dtype)


def keep_mask(S, F, seed=0):
    """a stand-in for the ReLU / dropout mask on the CPU: about a quarter kept (the GPU tests take the kernel's own)"""
    return torch.rand((S, F), generator=torch.Generator().manual_seed(77 + seed + F)) < 0.25


def fl32(v):
    return float(np.float32(v))


def _pow2(n):
    """n [.., 1] float64 counts: 0, 1, 2, 4, ... (1 / n and a product by it are exact)"""
    k = n.long()
    return (k & (k - 1)) == 0


def rounded(ref, b, dtype):
    """(ref, bound) after one rounding to dtype of a value within b of ref; where b == 0 the reference is rounded itself"""
    if dtype == torch.float32:
        return ref, b
    mag = ref.abs() + b
    extra = EPS[dtype] * mag
    if dtype == torch.float16:
        extra = extra + torch.where(mag > 0, 2.0 ** -25, 0.0)
    exact = b == 0
    return torch.where(exact, ref.float().to(dtype).double(), ref), torch.where(exact, torch.zeros_like(b), b + extra)


def forward(hop, x, epilogue, scale=0.0, out_dtype=torch.float32):
    """(ref, bound) [T, F or 2F] of k_agg_fwd"""
    xd = x.double()
    T = hop.T
    n = hop.deg.double().unsqueeze(1)
    s, M = hop.A @ xd, hop.A @ xd.abs()
    chain = torch.clamp(n - 1, min=0)
    if epilogue in (MEAN, OPERAND):
        inv = 1.0 / torch.clamp(n, min=1)
        ref = s * inv
        b = G2 * U * (chain + torch.where(_pow2(n), 0.0, 2.0)) * M * inv
        if epilogue == OPERAND:
            ref, b = torch.cat([ref, xd[:T]], 1), torch.cat([b, torch.zeros_like(b)], 1)
    elif epilogue == SUM:
        sc = fl32(scale)
        own = sc * xd[:T]
        ref, M = own + s, M + own.abs()
        b = G2 * U * (chain + (1.0 if sc != 0 else 0.0)) * M
        single = (n == 0).expand_as(ref)
        ref = torch.where(single, own.float().double(), ref)
        b = torch.where(single, torch.zeros_like(b), b)
    else:
        raise ValueError(epilogue)
    return rounded(ref, b, out_dtype)


def backward(hop, g, epilogue, form, scale=0.0, keep=None, act_scale=2.0, out_dtype=torch.float32):
    """(ref, bound) [S, F] of spp_agg_backward; g [T, F] (mean, sum) or [T, 2F]; form "scatter" / "gather";
    keep [S, F] bool and act_scale (the fp32 number fl(1 / (1 - p))) for operand_act"""
    gd = g.double()
    T, S = hop.T, hop.S
    At = hop.A.t()
    n = hop.deg.double().unsqueeze(1)
    cnt = hop.indeg.double().unsqueeze(1)
    is_t = (torch.arange(S) < T).unsqueeze(1)
    if epilogue == SUM:
        F = gd.size(1)
        sc = fl32(scale)
        own = torch.zeros((S, F), dtype=F64)
        own[:T] = sc * gd
        has = is_t & (sc != 0)
        ref, M = own + At @ gd, own.abs() + At @ gd.abs()
        c = torch.clamp(cnt - 1, min=0) + has.double()
        if form == "scatter":
            c = c + (has & (cnt > 0)).double()
        b = G2 * U * c * M
        single = (has & (cnt == 0)).expand_as(ref)
        ref = torch.where(single, own.float().double(), ref)
        b = torch.where(single, torch.zeros_like(b), b)
        return rounded(ref, b, out_dtype)
    operand = epilogue in (OPERAND, OPERAND_ACT)
    F = gd.size(1) // 2 if operand else gd.size(1)
    inv = 1.0 / torch.clamp(n, min=1)
    gm = gd[:, :F]
    own = torch.zeros((S, F), dtype=F64)
    if operand:
        own[:T] = gd[:, F:]
    ref, M = own + At @ (gm * inv), own.abs() + At @ (gm.abs() * inv)
    R = At @ (gm.abs() * inv * torch.where(_pow2(n), 0.0, 2.0))
    adds = torch.clamp(cnt - 1 + (is_t.double() if operand else 0.0), min=0)
    b = G2 * U * (R + adds * M)
    if epilogue == OPERAND_ACT:
        sc = fl32(act_scale)
        exact = float(np.log2(sc)).is_integer()
        b = torch.where(keep, b * sc + (0.0 if exact else G2 * U * (ref * sc).abs()), torch.zeros_like(b))
        ref = torch.where(keep, ref * sc, torch.zeros_like(ref))
    return rounded(ref, b, out_dtype)


def operand_fallback(hop, g, out_dtype):
    """(ref, bound) of models._MeanAggregate's backward at a non-vector width: the plain mean's scatter of g[:, :F] in
    out_dtype, then grad_x[:T] += g[:, F:] in out_dtype"""
    F = g.size(1) // 2
    ref, b = backward(hop, g[:, :F], MEAN, "scatter", out_dtype=out_dtype)
    ref, b = ref.clone(), b.clone()
    own = g.double()[:, F:]
    named = (hop.indeg[:hop.T] > 0).unsqueeze(1)
    ref[:hop.T] += own
    eps = EPS[out_dtype] if out_dtype != torch.float32 else U
    cast = EPS[out_dtype] * own.abs() if g.dtype != out_dtype else 0.0       # g[:, F:].to(out_dtype) rounds first
    b[:hop.T] = torch.where(named, b[:hop.T] + cast + G2 * eps * (ref[:hop.T].abs() + b[:hop.T] + cast), b[:hop.T])
    if out_dtype != torch.float32:                              # g[:, F:].to(out_dtype) of an unnamed target's row
        ref[:hop.T] = torch.where(named, ref[:hop.T], ref[:hop.T].float().to(out_dtype).double())
    return ref, b
