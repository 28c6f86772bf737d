"""Float64 restatement of the TransformerConv kernels (csrc/transformer_conv.hip: k_transformer_fwd, k_transformer_bwd;
spp.h f3y) with a per-element first-order rounding bound next to every value, and the inputs the tests run them on.  A
helper: no tests in here.  Everything is on the CPU, vectorised, in float64; fp32 / fp16 / bf16 inputs convert to
float64 exactly.  The planted hop and the constants are tests/gat_f64.py's; the ENTRY LIST is this file's own
(Entries): every CSR entry of the hop's raw (rowptr, col), diagonal entries kept, repeats kept, NO self loops -- not
Hop.r / Hop.s, which drop diagonals and append self loops.  n_i = rowptr[i + 1] - rowptr[i], and n_i = 0 is a real case.

The formulas (q [T, H, C], k [S, H, C], v [S, H, C], g [T, H, C]; entry (i, j) of row i; scale the fp32 number the
kernel receives, scale32(C) = float(float32(1 / sqrt(C)))):
  forward   e_ij = scale sum_c q[i,h,c] k[j,h,c],  m_i = max_j e_ij,  w_ij = exp(e_ij - m_i),  s_i = sum_j w_ij,
            alpha = w / s,  out[i,h,:] = sum_j alpha_ij v[j,h,:];      n_i = 0: out = 0, m_i = 0, s_i = 0
  backward  go_i = g_i . out_i,  gv_ij = g_i . v[j],  ge_ij = alpha_ij (gv_ij - go_i),  ges = ge scale,
            grad_v[j,h,c] = sum_i alpha_ij g[i,h,c],   grad_k[j,h,c] = sum_i ges_ij q[i,h,c],
            grad_q[i,h,c] = sum_j ges_ij k[j,h,c]      (n_i = 0: 0)

The bounds, built as gat_f64.py and gatv2_f64.py build theirs.  u = U = 2^-24; a sum of n fp32 terms, each a rounded
product, added in ANY order is within n u sum|term| of the exact sum to first order; M is the reference expression over
absolute values.
  logit:    a C-term dot product (each term one product and at most C - 1 additions: C u sum_c |q k|) and ONE product by
            scale (u |e|):  b_e = (C + 1) u scale sum_c |q k|.  row_max is the maximum of such numbers: within
            bm_i = max_j b_e_ij.
  weight:   the online softmax holds w_ij as a product of at most R_i + 1 factors exp(.) whose arguments add up to the
            COMPUTED e_ij - m_i.  R_i counts the rises of the running maximum AFTER the row's first entry, in CSR order
            (the first entry meets the empty state: its rescale multiplies zeros by expf(-inf) = 0 and its weight is
            expf(0) = 1, both exact); a dot product's rounding is not monotone, so a position counts as a rise whenever
            its exact logit comes within 2 bm_i of the running maximum of the exact logits.
            delta_ij = (R_i + 1) EXP0 + (EXP0 / 8 + u) d_ij + u R_i + b_e_ij + bm_i,   d_ij = m_i - e_ij
            (EXP0 = 1e-6 is gat_f64's figure for __expf at |arg| <= 8, scaled linearly beyond; expf is no worse);
            bw_ij = w_ij delta_ij + (R_i + 2) FLUSH   (FLUSH = 2^-126 per operation that can underflow).
  out:      sum_j |v[j]| bw_ij / s_i + M_out (sum_j bw_ij / s_i + (2 n_i + 4) u);      row_sum: sum_j bw_ij + n_i u s_i.
            A row without entries has bound 0 everywhere: its values are exact zeros.
  alpha in the backward (e recomputed in another summation order, which b_e covers; the forward's fp32 row_max and
            row_sum read):  dalpha_ij = b_e_ij + bm_i + u d_ij + EXP0 max(1, d_ij / 8) + b_s_i / s_i + 3 u;
            b_alpha = alpha dalpha + 2 FLUSH.
  go:       (C + 1) u sum_c |g out| + sum_c |g| b_out;      gv: (C + 1) u sum_c |g v|.
  ges:      scale (alpha (b_gv + b_go) + (b_alpha + 4 u alpha)(|gv| + |go|)) + FLUSH   (a subtraction, three products).
  grad_q:   sum_j b_ges |k| + (n_i + 2) u sum_j |ges k|            (one product per term, a chain of n_i).
  grad_k:   sum_i b_ges |q| + (cnt_j + 2) u sum_i |ges q|          (cnt_j entries name j: cnt_j atomics in any order).
  grad_v:   sum_i b_alpha |g| + (cnt_j + 2) u sum_i alpha |g|.
  Second order: G2 = 1 + 2^-10 on every bound built from more than one rounding, as in gat_f64.py.
  Layer level (layer_bounds): the mean over H heads adds (H + 1) u mean|out|; a gradient cast back to bf16 rows adds
  2^-8 |value| (fp16: 2^-11).
None of these constants comes from GPU output."""
import types

import numpy as np
import torch

from gat_f64 import COUNTS, EXP0, FLUSH, G2, U, HUB_LO, planted_hop, worst  # noqa: F401

F64 = torch.float64
REGIMES = ["model", "equal", "ascending", "descending", "wide", "zero"]


def scale32(C):
    """1 / sqrt(C) as the layer passes it: rounded to fp32"""
    return float(np.float32(1.0 / float(C) ** 0.5))


class Entries:
    """every CSR entry of a hop's raw (rowptr, col): row[k], col[k] in CSR order, n [T] the row lengths, named [S] the
    entries naming a source, seq [T, L] the entry ids of a row in CSR order, -1 padded"""

    def __init__(self, rowptr, col, T, S):
        self.rowptr, self.col, self.T, self.S, self.E = rowptr, col, T, S, int(col.numel())
        self.n = rowptr[1:] - rowptr[:-1]
        self.row = torch.repeat_interleave(torch.arange(T), self.n)
        self.named = torch.bincount(col, minlength=S)
        L = max(int(self.n.max()) if T else 1, 1)
        self.seq = torch.full((T, L), -1, dtype=torch.int64)
        if self.E:
            self.seq[self.row, torch.arange(self.E) - rowptr[:-1][self.row]] = torch.arange(self.E)
        self.hub_hi = None


def entries_of(hop):
    ent = Entries(hop.rowptr, hop.col, hop.T, hop.S)
    ent.hub_hi = getattr(hop, "hub_hi", None)
    return ent


def one_row(ent, t):
    """row t alone as a T = 1 hop over the same sources (target 0's q is the caller's to choose)"""
    b, e = int(ent.rowptr[t]), int(ent.rowptr[t + 1])
    return Entries(torch.tensor([0, e - b]), ent.col[b:e].clone(), 1, ent.S)


def _planted_logits(name, ent, H):
    """the per-(source, head) logit targets L [S, H] of a planted regime, in float64"""
    S = ent.S
    s = torch.arange(S, dtype=torch.int64).unsqueeze(1)
    h = torch.arange(H, dtype=torch.int64).unsqueeze(0)
    hub_hi = ent.hub_hi if ent.hub_hi is not None else S - 1
    if name in ("ascending", "descending"):        # along every row of the planted hop (its rows ascend by id, hubs last)
        key = s.clone()
        key[HUB_LO % S], key[hub_hi] = S, S + 1
        a = ((key - S // 2) * (1 + h)).double() / 64
        return a if name == "ascending" else -a
    if name == "equal":                            # one logit per head: bit-equal in every row
        return (((-1) ** h) * (2 + h)).double().expand(S, H).clone()
    if name == "wide":                             # a spread of 120 and more in a row: weights underflow to 0
        a = (-20 * 1024 + 2 * ((7919 * s + 131 * h) % 61440)).double() / 1024
        a[HUB_LO % S], a[hub_hi] = -20.0, 100.0
        return a
    raise ValueError(name)


def inputs(name, ent, H, C, dtype, seed=0):
    """(q [T, H, C], k [S, H, C], v [S, H, C] in dtype, g [T, H, C] in fp32) for a logit regime.
    "model": random rows.  The planted ones: q is 1 in the even columns and 0 in the odd ones; k carries the
    per-(source, head) value L * rs * 2 / C in its even columns, rs the power of two with sqrt(C) <= rs < 2 sqrt(C), so
    q . k = L * rs exactly (C / 2 equal terms, every partial sum a small multiple of one number) and the logit is
    fl(scale * L rs), between L and 1.42 L, the same bits for equal L; k's odd columns and all of v are random.
    "zero": q = 0, so every logit is 0 and out is the plain mean of v over the row."""
    S, T = ent.S, ent.T
    gen = torch.Generator().manual_seed(seed + 1000 * C + H)
    q = 0.5 * torch.randn((T, H, C), generator=gen)
    k = 0.5 * torch.randn((S, H, C), generator=gen)
    v = 0.5 * torch.randn((S, H, C), generator=gen)
    g = torch.randn((T, H, C), generator=gen)
    if name == "zero":
        q = torch.zeros((T, H, C))
    elif name != "model":
        rs = 1.0
        while rs * rs < C:
            rs *= 2.0
        q = torch.zeros((T, H, C))
        q[:, :, 0::2] = 1.0
        k[:, :, 0::2] = (_planted_logits(name, ent, H) * rs * 2.0 / C).float().unsqueeze(2)
    return q.to(dtype), k.to(dtype), v.to(dtype), g


def _rows(n, idx, v):
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=F64).index_add_(0, idx, v)


def forward(ent, q, k, v, scale):
    q, k, v = q.double(), k.double(), v.double()
    T, H, C = q.shape
    r, s = ent.row, ent.col
    prod = q[r] * k[s]                                                      # [E, H, C]
    e = scale * prod.sum(2)
    b_e = G2 * (C + 1) * U * scale * prod.abs().sum(2)
    idx = r.unsqueeze(1).expand(-1, H)
    m = torch.full((T, H), -float("inf"), dtype=F64).scatter_reduce(0, idx, e, "amax")
    bm = torch.zeros((T, H), dtype=F64).scatter_reduce(0, idx, b_e, "amax")
    d = m[r] - e
    w = torch.exp(-d)
    ssum = _rows(T, r, w)
    alpha = w / ssum[r]
    ep = torch.cat([e, torch.full((1, H), -float("inf"), dtype=F64)])[ent.seq]       # [T, L, H]
    on = (ent.seq[:, 1:] >= 0).unsqueeze(2)
    R = (on & (ep[:, 1:] > torch.cummax(ep, 1).values[:, :-1] - 2 * bm.unsqueeze(1))).sum(1).double()
    n = ent.n.double().unsqueeze(1)
    delta = (R[r] + 1) * EXP0 + (EXP0 / 8 + U) * d + U * R[r] + b_e + bm[r]
    bw = w * delta + (R[r] + 2) * FLUSH
    a3, b3 = alpha.unsqueeze(2), (bw / ssum[r]).unsqueeze(2)
    out = _rows(T, r, a3 * v[s])
    M = _rows(T, r, a3 * v[s].abs())
    has = (n > 0).double()
    rel = _rows(T, r, bw / ssum[r]) + (2 * n + 4) * U * has
    b_out = G2 * (_rows(T, r, b3 * v[s].abs()) + M * rel.unsqueeze(2))
    bs = G2 * (_rows(T, r, bw) + n * U * ssum)
    m = torch.where(n > 0, m, torch.zeros_like(m))                           # a row without entries: row_max = 0
    return types.SimpleNamespace(out=out, b_out=b_out, row_max=m, bm=bm, row_sum=ssum, bs=bs, alpha=alpha, e=e, b_e=b_e,
                                 d=d, R=R)


def backward(ent, q, k, v, g, scale, fw=None):
    """closed-form gradients of sum(out * g) and their bounds"""
    fw = fw or forward(ent, q, k, v, scale)
    q, k, v, g = q.double(), k.double(), v.double(), g.double()
    (T, H, C), S = q.shape, k.size(0)
    r, s = ent.row, ent.col
    ga, alpha = g.abs(), fw.alpha
    go = (g * fw.out).sum(2)
    b_go = (C + 1) * U * (ga * fw.out.abs()).sum(2) + (ga * fw.b_out).sum(2)
    gv = (g[r] * v[s]).sum(2)
    b_gv = (C + 1) * U * (ga[r] * v[s].abs()).sum(2)
    d_alpha = (fw.b_e + fw.bm[r] + U * fw.d + EXP0 * torch.clamp(fw.d / 8, min=1.0) + fw.bs[r] / fw.row_sum[r] + 3 * U)
    b_alpha = G2 * alpha * d_alpha + 2 * FLUSH
    ges = alpha * (gv - go[r]) * scale
    b_ges = G2 * scale * (alpha * (b_gv + b_go[r]) + (b_alpha + 4 * U * alpha) * (gv.abs() + go[r].abs())) + FLUSH
    n = ent.n.double().view(T, 1, 1)
    named = ent.named.double().view(S, 1, 1)
    g3, b3, a3 = ges.unsqueeze(2), b_ges.unsqueeze(2), alpha.unsqueeze(2)
    out = types.SimpleNamespace(fw=fw, ges=ges, b_ges=b_ges, b_alpha=b_alpha)
    out.gq = _rows(T, r, g3 * k[s])
    out.b_gq = G2 * (_rows(T, r, b3 * k[s].abs()) + (n + 2) * U * _rows(T, r, (g3 * k[s]).abs()))
    out.gk = _rows(S, s, g3 * q[r])
    out.b_gk = G2 * (_rows(S, s, b3 * q[r].abs()) + (named + 2) * U * _rows(S, s, (g3 * q[r]).abs()))
    out.gv = _rows(S, s, a3 * g[r])
    out.b_gv = G2 * (_rows(S, s, b_alpha.unsqueeze(2) * ga[r]) + (named + 2) * U * _rows(S, s, a3 * ga[r]))
    return out


def mean_of_v(ent, v):
    """the plain mean of v over each row's entries (zeros for a row without entries): what q = 0 must give"""
    v = v.double()
    n = ent.n.double().clamp(min=1).view(-1, 1, 1)
    return _rows(ent.T, ent.row, v[ent.col]) / n


def layer_bounds(bw, concat, rows_dtype):
    """the attention's output as TransformerConv shapes it before the skip, from backward()'s kernel-level values:
    (out, b_out, cast) -- out [T, H * C] or the mean over heads [T, C]; cast: the relative half ulp a gradient cast back
    to the rows' dtype adds (0 for fp32 rows)"""
    fw = bw.fw
    T, H, C = fw.out.shape
    if concat:
        out, b = fw.out.reshape(T, H * C), fw.b_out.reshape(T, H * C)
    else:
        out, b = fw.out.mean(1), fw.b_out.mean(1) + (H + 1) * U * fw.out.abs().mean(1)
    cast = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[rows_dtype]
    return out, G2 * b, cast
