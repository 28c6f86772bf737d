"""Float64 restatement of spp_graph_gatv2_forward (csrc/graph_gatv2.hip; spp.h f3w) over a whole graph, with a
per-element first-order rounding bound next to every value, and the planted graph the tests run it on.  A helper: no
tests in here.  Everything is on the CPU in float64; fp32 / bf16 inputs convert to float64 exactly.

The formula, per target t and head h (x_l, x_r [N, H, C] by global id, att [H, C]): the entries are row t's CSR entries
without the diagonal ones plus one self loop;  pre_jc = x_l[j,h,c] + x_r[t,h,c],  lr = pre > 0 ? pre : pre * slope,
e_j = sum_c att[h,c] lr_jc,  alpha = softmax_j(e),  out[t,h,:] = sum_j alpha_j x_l[j,h,:].  ``plain_rows`` states it row
by row in a Python loop; ``reference`` states it once more over the entry list of gat_f64.Hop and adds the bounds.
Neither knows of chunks: a chunk only enters the BOUND, as a count of roundings.

The bounds are tests/gatv2_f64.py's (u = U = 2^-24, EXP0, FLUSH, G2 from there; none of them from GPU output), with
what a long row adds.  C_g = the kernel's chunk; a row of L raw entries has k = max(1, ceil(L / C_g)) chunks and
M = k - 1 merges; an entry at raw position p sits in chunk p // C_g, the self loop in chunk 0.
  logit   b_e = (C + 2) u sum_c |att lr|, bm = max_j b_e: as gatv2_f64.forward (C is the kernel's C: a zero-padded
          channel adds an exact +0).
  weight  inside its chunk the online softmax holds w_j as a product of at most R + 1 factors exp(.), R the rises of
          the running maximum IN THAT CHUNK in the kernel's order (chunk 0: self loop, then CSR; any other chunk: its kept
          entries in CSR order, where the first one meets the empty state: its rescale multiplies zeros by exp(-inf) = 0
          and its own factor is exp(0) = 1, both exact, so it counts as the chunk's start and not as a rise).  A position
          counts as a rise whenever its exact logit comes within 2 bm of the running maximum of the exact logits, as
          in gatv2_f64.  Every merge the entry's state goes through multiplies it by ONE more factor exp(.) (f1 or
          f2) in TWO rounded operations (the product acc * f1 and the fma; for the merged side the fma alone): at most
          M merges, so M more factors and 2 M more roundings.  All factors' arguments have one sign and add up to the
          computed e_j - m, so the argument terms stay as they are:
            delta_j = (R + 1 + M) EXP0 + (EXP0 / 8 + u) d_j + u (R + 2 M) + b_e_j + bm,   d_j = m - e_j
            bw_j = w_j delta_j + (R + 2 + 2 M) FLUSH.
          (expf is at least as accurate as the __expf EXP0 was taken for.)
  out     sum_j |x_l[j]| bw_j / s + M_out (sum_j bw_j / s + (2 n + 4 + 2 M) u): the chains of numerator and denominator
          are n products and additions each plus one addition per merge; reciprocal and final product as gatv2_f64.
  G2 = 1 + 2^-10 on the whole, as there.  A bf16 OUTPUT adds one rounding of the computed value: the caller widens the
  bound b to b + 2^-8 (|ref| + b)."""
import functools
import types

import torch

from gat_f64 import EXP0, FLUSH, G2, U, Hop

F64 = torch.float64
N = 700
ISOLATED = N - 1                                           # no entries, named by nobody
ONLY_SELF = 11                                             # a short row of nothing but its own id
EMPTY_CHUNK_ROW = 9                                        # a long row whose second chunk is only its own id


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


@functools.lru_cache(maxsize=None)
def planted_graph(Cg):
    """About 700 nodes.  Rows 0..8 have 0, 1, 63, 64, 65, C_g, C_g + 1, 3 C_g + 7 and 9 C_g raw entries; row 9 has
    2 C_g + 5 with its second chunk nothing but 9; row 10 is short with diagonal entries first, mid and last and a
    duplicate; row 11 is [11, 11, 11]; row 12 has C_g + 1 entries whose last -- all of chunk 1 -- is 12; rows 7 and 8
    carry diagonal entries at chunk edges and duplicates; every other row has 0..12 random entries; node N - 1 is
    isolated.  Returns a gat_f64.Hop with T = S = N (plus hub_hi for gat_f64.regime, raw [N] and planted: the rows
    above)."""
    g = torch.Generator().manual_seed(7)
    lengths = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: Cg, 6: Cg + 1, 7: 3 * Cg + 7, 8: 9 * Cg, 9: 2 * Cg + 5, 10: 7, 11: 3,
               12: Cg + 1, ISOLATED: 0}
    rows = []
    for t in range(N):
        k = lengths.get(t, int(torch.randint(0, 13, (1,), generator=g)))
        rows.append(torch.randint(0, N - 1, (k,), generator=g).tolist())
    rows[7][2], rows[7][Cg - 1], rows[7][Cg], rows[7][Cg + 8] = 7, 7, 7, rows[7][Cg + 7]
    rows[8][3], rows[8][5 * Cg], rows[8][9 * Cg - 1], rows[8][40] = 8, 8, rows[8][9 * Cg - 2], rows[8][39]
    rows[9][Cg:2 * Cg] = [9] * Cg
    rows[10][0], rows[10][3], rows[10][6], rows[10][5] = 10, 10, 10, rows[10][4]
    rows[11] = [11, 11, 11]
    rows[12][Cg] = 12
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    hop = Hop(rowptr, torch.tensor([j for r in rows for j in r], dtype=torch.int64), N, N)
    hop.hub_hi = 52
    hop.raw = rowptr[1:] - rowptr[:-1]
    hop.planted = sorted(lengths)
    return hop


def plain_rows(rowptr, col, x_l, x_r, att, slope):
    """the formula row by row, [N, H, C] float64; nothing shared with ``reference``"""
    x_l, x_r, att = x_l.double(), x_r.double(), att.double()
    out = torch.empty_like(x_l)
    for t in range(x_l.size(0)):
        js = [j for j in col[int(rowptr[t]):int(rowptr[t + 1])].tolist() if j != t] + [t]
        v = x_l[js]                                                         # [n, H, C]
        pre = v + x_r[t]
        e = (att * torch.where(pre > 0, pre, pre * slope)).sum(2)
        out[t] = (torch.softmax(e, 0).unsqueeze(2) * v).sum(0)
    return out


def _rows(n, idx, v):
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=F64).index_add_(0, idx, v)


def reference(hop, x_l, x_r, att, slope, Cg):
    """out [N, H, C] and its bound b_out, both float64, for x_l, x_r [N, H, C] and att [H, C]"""
    x_l, x_r, att = x_l.double(), x_r.double(), att.double()
    T, (H, C), r, s, nk = hop.T, att.shape, hop.r, hop.s, hop.nk
    pre = x_l[s] + x_r[r]
    lr = lrelu(pre, slope)
    e = (att * lr).sum(2)                                                   # [entries, H]
    b_e = G2 * (C + 2) * U * (att.abs() * lr.abs()).sum(2)
    idx = r.unsqueeze(1).expand(-1, H)
    m = torch.full((T, H), -float("inf"), dtype=F64).scatter_reduce(0, idx, e, "amax")
    bm = torch.zeros((T, H), dtype=F64).scatter_reduce(0, idx, b_e, "amax")
    d = m[r] - e
    w = torch.exp(-d)
    ssum = _rows(T, r, w)
    alpha = w / ssum[r]
    # the chunk of every entry and the rises of the running maximum inside it, in the kernel's order
    chunk = torch.cat([(hop.eid - hop.rowptr[hop.row[hop.eid]]) // Cg, torch.zeros(T, dtype=torch.int64)])
    kmax = int(chunk.max()) + 1 if chunk.numel() else 1
    seg = r * kmax + chunk                                                  # (row, chunk), one id per segment
    order = torch.cat([torch.arange(nk) + 1, torch.zeros(T, dtype=torch.int64)])   # in a segment: self loop, then CSR
    perm = torch.argsort(seg * (nk + 2) + order)
    sseg = seg[perm]
    first = torch.ones_like(sseg, dtype=torch.bool)
    first[1:] = sseg[1:] != sseg[:-1]
    start = torch.nonzero(first).flatten()
    segno = torch.cumsum(first.long(), 0) - 1
    posn = torch.arange(sseg.numel()) - start[segno]
    L = int(posn.max()) + 1
    ep = torch.full((start.numel(), L, H), -float("inf"), dtype=F64)
    ep[segno, posn] = e[perm]
    bm_seg = bm[r[perm][start]].unsqueeze(1)                                # [segments, 1, H]
    on = torch.zeros((start.numel(), L), dtype=torch.bool)
    on[segno, posn] = True
    rise = on[:, 1:].unsqueeze(2) & (ep[:, 1:] > torch.cummax(ep, 1).values[:, :-1] - 2 * bm_seg)
    R_seg = rise.sum(1).double()                                            # [segments, H]
    R = torch.empty((nk + T, H), dtype=F64)
    R[perm] = R_seg[segno]
    M = (torch.clamp((hop.raw + Cg - 1) // Cg, min=1) - 1).double()        # merges of a row
    Mr = M[r].unsqueeze(1)
    n = hop.n.double().unsqueeze(1)
    delta = (R + 1 + Mr) * EXP0 + (EXP0 / 8 + U) * d + U * (R + 2 * Mr) + b_e + bm[r]
    bw = w * delta + (R + 2 + 2 * Mr) * FLUSH
    a3, b3 = alpha.unsqueeze(2), (bw / ssum[r]).unsqueeze(2)
    out = _rows(T, r, a3 * x_l[s])
    Mo = _rows(T, r, a3 * x_l[s].abs())
    rel = _rows(T, r, bw / ssum[r]) + (2 * n + 4 + 2 * M.unsqueeze(1)) * U
    b_out = G2 * (_rows(T, r, b3 * x_l[s].abs()) + Mo * rel.unsqueeze(2))
    return types.SimpleNamespace(out=out, b_out=b_out, R=R, M=M, e=e, row_max=m)


def widen_bf16(ref, bound):
    """the bound of a bf16 output: one more rounding, 2^-8 relative, of the computed value"""
    return bound + 2.0 ** -8 * (ref.abs() + bound)


# ---- a correct fp32 chunked computation in torch, and three ways to get it wrong (the host test's) --------------------
def chunked_fp32(rowptr, col, x_l, x_r, att, slope, Cg, fault=None):
    """the contract of spp.h f3w in fp32 torch ops, row by row: per chunk a two-pass softmax state (m, s, acc), chunk 0
    with the self loop, the states merged in chunk order.  ``fault``: "no_rescale" merges s and acc without f1 / f2,
    "self_everywhere" puts the self loop into every chunk, "keep_diag" does not skip diagonal entries."""
    x_l, x_r, att = x_l.float(), x_r.float(), att.float()
    sl = torch.tensor(slope, dtype=torch.float32)
    out = torch.empty_like(x_l)
    for t in range(x_l.size(0)):
        raw = col[int(rowptr[t]):int(rowptr[t + 1])].tolist()
        state = None
        for c in range(max(1, -(-len(raw) // Cg))):
            js = [j for j in raw[c * Cg:(c + 1) * Cg] if j != t or fault == "keep_diag"]
            if c == 0 or fault == "self_everywhere":
                js = [t] + js
            if not js:
                continue                                                    # an empty chunk merges as nothing
            v = x_l[js]
            pre = v + x_r[t]
            e = (att * torch.where(pre > 0, pre, pre * sl)).sum(2)          # [n, H]
            mc = e.max(0).values
            wc = torch.exp(e - mc)
            sc, ac = wc.sum(0), (wc.unsqueeze(2) * v).sum(0)
            if state is None:
                state = (mc, sc, ac)
                continue
            m0, s0, a0 = state
            mm = torch.maximum(m0, mc)
            f1, f2 = torch.exp(m0 - mm), torch.exp(mc - mm)
            if fault == "no_rescale":
                f1, f2 = torch.ones_like(f1), torch.ones_like(f2)
            state = (mm, s0 * f1 + sc * f2, a0 * f1.unsqueeze(1) + ac * f2.unsqueeze(1))
        out[t] = state[2] / state[1].unsqueeze(1)
    return out
