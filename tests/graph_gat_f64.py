"""Float64 restatement of spp_graph_gat_forward (csrc/graph_gat.hip: k_graph_gat_rows, k_graph_gat_long; spp.h f3h) over
a whole graph, with a per-element first-order rounding bound next to every value, the planted graph and the logit regimes
the tests run it on, and the contract once more in fp32 torch ops with five ways to get it wrong.  A helper: no tests in
here.  Everything is on the CPU; fp32 / fp16 / bf16 rows of h convert to float64 exactly.

The formula, per target t and head k (h [N, H, C], a_src and a_dst [N, H] by global id): the entries are row t's CSR
entries without the diagonal ones plus one self loop;  raw_j = a_src[j,k] + a_dst[t,k],  e_j = raw > 0 ? raw : raw * slope,
alpha = softmax_j(e),  out[t,k,:] = sum_j alpha_j h[j,k,:].  ``plain_rows`` states it row by row in a Python loop;
``reference`` states it once more over the entry list of gat_f64.Hop and adds the bounds.  Neither knows of chunks: a
chunk only enters the BOUND, as a count of roundings.

The bound, from the kernel's contract (the header comment of graph_gat.hip; spp.h, spp_graph_gat_forward).  u = U = 2^-24,
EXP0, FLUSH and G2 are gat_f64's; none of them comes from GPU output, and every other factor below is a count of
operations.  C_g = spp_graph_gat_chunk(); a row of L raw entries has k = max(1, ceil(L / C_g)) chunks and M = k - 1
merges; an entry at raw position p sits in chunk p // C_g, the self loop in chunk 0.
  logit   gat_f64.forward's term: the kernel has fl(fl(a_src + a_dst) * slope), one addition and one product, within
          b_e_j = 2 u |raw_j| of e_j.  Both operations are redone in fp32 on the CPU: where BOTH are exact for an entry
          (the planted regimes at slope 0.25, and wherever raw > 0 there), b_e_j = 0.  bm = max_j b_e_j over the row
          bounds the error of the row's computed maximum, |raw of the row's maximum| included.
  weight  inside its chunk the online softmax (State::take) holds w_j as a product of at most R + 1 factors __expf(.),
          R the rises of the running maximum IN THAT CHUNK in the kernel's order (chunk 0: self loop, then CSR; any other
          chunk: its kept entries in CSR order, where the first one meets the empty state: its rescale multiplies zeros by
          __expf(-inf) = 0 and its own factor is __expf(0) = 1, both exact, so it is the chunk's start and no rise).  R is
          counted from the exact logits: the computed logit is a monotone function of the exact raw (fl of a sum, fl of a
          product by a positive number), so a computed rise is an exact one.  Every merge (State::merge) the entry's
          state goes through multiplies it by ONE more factor (f1 or f2) in TWO rounded operations (the product
          acc * f1 and the fma; for the merged side the fma alone).  The state of chunk 0 goes through all M merges of
          the row; the state of chunk c >= 1 is merged in at merge c and is part of the running state from then on:
          M_j = M - c + 1 merges (counted per entry, so that an entry of the LAST chunk carries one merge and not M: a
          row whose weight sits there gets a bound that a wrong merge cannot hide in).  So M_j more factors and at most
          2 M_j more roundings.  All factors' arguments have one sign and add up to the computed m - e_j, so the
          argument terms stay gat_f64's:
            delta_j = (R + 1 + M_j) EXP0 + (EXP0 / 8 + u) d_j + u (R + 2 M_j) + b_e_j + bm,   d_j = m - e_j
            bw_j = w_j delta_j + (R + 2 + 2 M_j) FLUSH.
  out     sum_j |h_j| bw_j / s + M_out (sum_j bw_j / s + (2 n_c + 1) u),  M_out = sum_j alpha_j |h_j|: the weights' own
          errors in numerator and denominator (the rescales' and the merges' roundings are in delta_j already); the
          chains, which the contract cuts at the chunks: a chunk's acc takes its n' entries in n' fmas and its s in n'
          additions, so a term meets at most n_c = the row's largest count of entries in one chunk (the self loop
          counted in chunk 0) roundings in each, whatever the row's length: n_c u and n_c u; then what Piece::over
          performs (elem_io.hip.h): ONE fp32 division acc / s per column, which the build leaves correctly rounded
          (u; the device code holds the v_div_scale / v_div_fmas / v_div_fixup sequence) -- no reciprocal and no
          final product, so gat_f64's 2 u + u for those becomes u.
  n = 1   a row that keeps no entry is the self loop's state (m, 1, h_t) untouched: every merge is with an empty state
          (f1 = __expf(0) = 1, f2 = __expf(-inf) = 0, fma(0, 0, x) = x) and the division is by 1.  Nothing rounds: the
          bound of such a row is FLUSH alone.
  G2 = 1 + 2^-10 on the whole, as in gat_f64.  A bf16 OUTPUT adds one rounding of the computed value: the caller widens
  the bound b to b + 2^-8 (|ref| + b) (``widen_bf16``).  relu=True: the same bound against relu(ref), since
  |relu a - relu b| <= |a - b|."""
import functools
import types

import torch

import gat_f64
from gat_f64 import EXP0, FLUSH, G2, Q, U, Hop
from graph_gatv2_f64 import widen_bf16  # noqa: F401  (the bf16 output's bound: one more rounding)

F64 = torch.float64
N = 700
ISOLATED = N - 1                                           # no entries, named by nobody
EMPTY_CHUNK_ROW = 9                                        # a long row whose second chunk is only its own id
ONLY_SELF = 11                                             # a short row of nothing but its own id
DROPPED_TAIL_ROW = 12                                      # C_g + 1 entries, the last one -- all of chunk 1 -- itself
DEEP_ROW = 13                                              # 33 C_g + 1 raw entries
FIRST_TOP = 61                                             # position 1 of every row of three or more chunks
LAST_TOP = 60                                              # the last entry of every long row whose last chunk keeps one
REGIMES = gat_f64.REGIMES + ["model", "last_chunk_max", "dead_chunk"]
FAULTS = ["no_rescale", "self_everywhere", "keep_diag", "head0_everywhere", "merge_skips_last"]


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


@functools.lru_cache(maxsize=None)
def planted_graph(Cg):
    """About 700 nodes.  Rows 0..8 have 0, 1, 63, 64, 65, C_g, C_g + 1, 3 C_g + 7 and 9 C_g raw entries; row 9 has
    2 C_g + 5 with its second chunk nothing but 9; row 10 is short with diagonal entries first, mid and last and a
    duplicate; row 11 is [11, 11, 11]; row 12 has C_g + 1 entries whose last -- all of chunk 1 -- is 12; row 13 has
    33 C_g + 1: chunk c < 33 draws from the id band [14 + 20 c, 34 + 20 c) (so that logits rising with the id make EVERY
    merge rescale), with diagonal entries on both sides of the edge between chunks 15 and 16 and a duplicate; rows 7 and
    8 carry diagonal entries at chunk edges and duplicates; every other row has 0..12 random entries; node N - 1 is
    isolated.  FIRST_TOP is entry 1 of every row of three or more chunks and LAST_TOP the last entry of every long row
    but row 12, and neither occurs anywhere else in a long row (the regimes of this file hang on them).  Returns a
    gat_f64.Hop with T = S = N (plus hub_hi for gat_f64.regime, raw [N], chunk [nk]: the chunk of every kept entry, and
    planted: the rows above)."""
    g = torch.Generator().manual_seed(11)
    lengths = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: Cg, 6: Cg + 1, 7: 3 * Cg + 7, 8: 9 * Cg, 9: 2 * Cg + 5, 10: 7, 11: 3,
               12: Cg + 1, DEEP_ROW: 33 * Cg + 1, ISOLATED: 0}
    rows = []
    for t in range(N):
        k = lengths.get(t, int(torch.randint(0, 13, (1,), generator=g)))
        rows.append(torch.randint(0, N - 1, (k,), generator=g).tolist())
    rows[DEEP_ROW] = [14 + 20 * (p // Cg) + int(v) for p, v in
                      enumerate(torch.randint(0, 20, (33 * Cg + 1,), generator=g).tolist())]
    for t, row in enumerate(rows):
        if len(row) > Cg:
            row[:] = [62 if j in (FIRST_TOP, LAST_TOP) else j for j in row]
            if len(row) > 2 * Cg:
                row[1] = FIRST_TOP
            row[-1] = LAST_TOP
    rows[7][2], rows[7][Cg - 1], rows[7][Cg], rows[7][Cg + 8] = 7, 7, 7, rows[7][Cg + 7]
    rows[8][3], rows[8][5 * Cg], rows[8][9 * Cg - 2], rows[8][40] = 8, 8, rows[8][9 * Cg - 3], rows[8][39]
    rows[9][Cg:2 * Cg] = [9] * Cg
    rows[10][0], rows[10][3], rows[10][6], rows[10][5] = 10, 10, 10, rows[10][4]
    rows[11] = [11, 11, 11]
    rows[12][Cg] = 12
    rows[DEEP_ROW][16 * Cg - 1], rows[DEEP_ROW][16 * Cg], rows[DEEP_ROW][100] = DEEP_ROW, DEEP_ROW, rows[DEEP_ROW][99]
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    hop = Hop(rowptr, torch.tensor([j for r in rows for j in r], dtype=torch.int64), N, N)
    hop.hub_hi = 52
    hop.raw = rowptr[1:] - rowptr[:-1]
    hop.chunk = (hop.eid - rowptr[hop.row[hop.eid]]) // Cg
    hop.planted = sorted(lengths)
    return hop


def _chunks(hop, Cg):
    """per softmax entry (kept CSR entries, then the self loops) its chunk; per row its chunk count"""
    return torch.cat([hop.chunk, torch.zeros(hop.T, dtype=torch.int64)]), torch.clamp((hop.raw + Cg - 1) // Cg, min=1)


def _row_max(hop, v, on):
    """[T, H]: the maximum of v [entries, H] over the entries of a row selected by on [entries]; -inf where none"""
    H = v.size(1)
    v = torch.where(on.unsqueeze(1), v, torch.full_like(v, -float("inf")))
    return torch.full((hop.T, H), -float("inf"), dtype=F64).scatter_reduce(0, hop.r.unsqueeze(1).expand(-1, H), v, "amax")


def regime(name, hop, H, Cg):
    """(a_src, a_dst) [N, H] in fp32.  gat_f64.REGIMES: gat_f64.regime's.  The two of this file are built the same way
    (a_src even and a_dst odd multiples of Q = 2^-10, |a_src| + |a_dst| < 128, so raw is exact in fp32 and never 0), with
    every raw POSITIVE, so that no slope moves a gap, and differ by head.  Their properties are asserted here, over the
    exact logits, for every head and both slopes of gat_f64.SLOPES:
      last_chunk_max  a_src rises with the id (deep row: every chunk's maximum exceeds the one before, every merge
                      rescales) and LAST_TOP lies 33 or more above all: in every row that keeps an entry beyond chunk 0
                      (every row longer than C_g but DROPPED_TAIL_ROW, whose chunk 1 keeps nothing), the maximum sits in
                      the last chunk that keeps an entry, and every earlier chunk's maximum is at least 30 below it.
      dead_chunk      the sources kept in chunk 1 of a row of three or more chunks lie in [0.5, 2.5), FIRST_TOP (in chunk
                      0 of every such row) at 116 or more, everybody else in [30, 110): those entries lie more than 110
                      below the row's maximum and more than 104 > 149 ln 2 below chunk 0's, so f2 of their merge is 0."""
    if name in gat_f64.REGIMES:
        return gat_f64.regime(name, hop, H)
    T = hop.T
    s = torch.arange(T, dtype=torch.int64).unsqueeze(1)
    h = torch.arange(H, dtype=torch.int64).unsqueeze(0)
    chunk, nchunks = _chunks(hop, Cg)
    a_dst = (2 * ((7 * s + 3 * h) % 32) - 31).double() * Q
    if name == "last_chunk_max":
        a = 1024 + s * (8 + 2 * h)
        a[LAST_TOP] = 50 * 1024 + 2048 * h[0]
    elif name == "dead_chunk":
        dead = (nchunks[hop.r] >= 3) & (chunk == 1)
        a = 30 * 1024 + 2 * ((7919 * s + 131 * h) % 40960)
        low = torch.unique(hop.s[dead])
        a[low] = (512 + 2 * ((37 * s + 11 * h) % 1024))[low]
        a[FIRST_TOP] = 116 * 1024 + 512 * h[0]
    else:
        raise ValueError(name)
    a_src, a_dst = (a.double() * Q).float(), a_dst.float()
    assert bool((a_src.double() == a.double() * Q).all()) and float(a_src.abs().max()) + float(a_dst.abs().max()) < 128
    raw = a_src[hop.s] + a_dst[hop.r]
    assert bool((raw.double() == a_src[hop.s].double() + a_dst[hop.r].double()).all()) and bool((raw > 0).all())
    for slope in gat_f64.SLOPES:
        e = lrelu(raw.double(), slope)
        if name == "last_chunk_max":
            last = torch.zeros(T, dtype=torch.int64).scatter_reduce(0, hop.r, chunk, "amax")
            rows = last >= 1
            assert sorted(torch.nonzero(hop.raw > Cg).flatten().tolist()) == \
                sorted(torch.nonzero(rows).flatten().tolist() + [DROPPED_TAIL_ROW])
            gap = _row_max(hop, e, chunk == last[hop.r]) - _row_max(hop, e, chunk < last[hop.r])
            assert float(gap[rows].min()) >= 30 and float(gap[rows].max()) < 80, (name, slope, gap[rows].min())
        else:
            rows = torch.zeros(T, dtype=torch.bool)
            rows[hop.r[dead]] = True
            assert bool(rows[[7, 8, DEEP_ROW]].all()) and bool((nchunks[rows] >= 3).all())
            below = _row_max(hop, e, torch.ones_like(dead))[hop.r[dead]] - e[dead]
            first = (_row_max(hop, e, chunk == 0) - _row_max(hop, e, dead))[rows]
            assert float(below.min()) > 110 and float(first.min()) > 104, (name, slope, below.min(), first.min())
    return a_src, a_dst


@functools.lru_cache(maxsize=None)
def values(H, C):
    """h [N, H, C] in fp32, multiples of 2^-6 below 4 in size: the SAME numbers in fp32, fp16 and bf16, so one reference
    serves all three row types; att [2, H, C] in fp32 for the "model" regime"""
    g = torch.Generator().manual_seed(1000 * C + H)
    h = torch.clamp(torch.round(32 * torch.randn((N, H, C), generator=g)) / 64, -3.5, 3.5)
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(h.to(dt).float(), h)
    return h, 2 * torch.randn((2, H, C), generator=g) / C ** 0.5


@functools.lru_cache(maxsize=None)
def inputs(name, H, C, Cg):
    """(h [N, H, C], a_src, a_dst [N, H]), all fp32.  "model": the logits are a random projection of h, computed in fp32
    -- not exact, so the 2 u |raw| term of the bound is live"""
    h, att = values(H, C)
    if name == "model":
        return h, (h * att[0]).sum(2), (h * att[1]).sum(2)
    return (h,) + regime(name, planted_graph(Cg), H, Cg)


def plain_rows(rowptr, col, h, a_src, a_dst, slope):
    """the formula row by row, [N, H, C] float64; nothing shared with ``reference``"""
    h, a_src, a_dst = h.double(), a_src.double(), a_dst.double()
    out = torch.empty_like(h)
    for t in range(h.size(0)):
        js = [j for j in col[int(rowptr[t]):int(rowptr[t + 1])].tolist() if j != t] + [t]
        raw = a_src[js] + a_dst[t]
        e = torch.where(raw > 0, raw, raw * slope)
        out[t] = (torch.softmax(e, 0).unsqueeze(2) * h[js]).sum(0)
    return out


def _rows(n, idx, v):
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=F64).index_add_(0, idx, v)


def reference(hop, h, a_src, a_dst, slope, Cg):
    """out [N, H, C] and its bound b_out, both float64, for h [N, H, C] and the fp32 logit halves a_src, a_dst [N, H]"""
    a32s, a32d = a_src.float(), a_dst.float()
    h, a_src, a_dst = h.double(), a_src.double(), a_dst.double()
    T, H, r, s, nk = hop.T, a_src.size(1), hop.r, hop.s, hop.nk
    raw = a_src[s] + a_dst[r]
    e = lrelu(raw, slope)                                                   # [entries, H]
    raw32 = a32s[s] + a32d[r]                                               # the kernel's two operations, in fp32
    e32 = torch.where(raw32 > 0, raw32, raw32 * torch.tensor(slope, dtype=torch.float32))
    exact = (raw32.double() == raw) & (e32.double() == e)
    b_e = torch.where(exact, torch.zeros_like(raw), 2 * U * raw.abs())
    idx = r.unsqueeze(1).expand(-1, H)
    m = torch.full((T, H), -float("inf"), dtype=F64).scatter_reduce(0, idx, e, "amax")
    bm = torch.zeros((T, H), dtype=F64).scatter_reduce(0, idx, b_e, "amax")
    d = m[r] - e
    w = torch.exp(-d)
    ssum = _rows(T, r, w)
    alpha = w / ssum[r]
    # the chunk of every entry and the rises of the running maximum inside it, in the kernel's order
    chunk, nchunks = _chunks(hop, Cg)
    kmax = int(chunk.max()) + 1
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
    R_seg = (ep[:, 1:] > torch.cummax(ep, 1).values[:, :-1]).sum(1).double()       # [segments, H]
    R = torch.empty((nk + T, H), dtype=F64)
    R[perm] = R_seg[segno]
    M = (nchunks - 1).double()                                              # merges of a row
    Mj = torch.where(chunk == 0, M[r], M[r] - chunk + 1).unsqueeze(1)       # ... and those an entry's state goes through
    nc = torch.zeros(T, dtype=torch.int64).scatter_reduce(0, r[perm][start], torch.bincount(segno), "amax")
    nc = nc.double().unsqueeze(1)                                           # the longest chain of a row: entries in a chunk
    delta = (R + 1 + Mj) * EXP0 + (EXP0 / 8 + U) * d + U * (R + 2 * Mj) + b_e + bm[r]
    bw = w * delta + (R + 2 + 2 * Mj) * FLUSH
    a3, b3 = alpha.unsqueeze(2), (bw / ssum[r]).unsqueeze(2)
    out = _rows(T, r, a3 * h[s])
    Mo = _rows(T, r, a3 * h[s].abs())
    rel = _rows(T, r, bw / ssum[r]) + (2 * nc + 1) * U
    b_out = G2 * (_rows(T, r, b3 * h[s].abs()) + Mo * rel.unsqueeze(2))
    b_out[hop.n == 1] = FLUSH                                               # the self loop's state untouched: exact
    return types.SimpleNamespace(out=out, b_out=b_out, R=R, M=M, e=e, row_max=m)


worst = gat_f64.worst


# ---- the contract in fp32 torch ops, and five ways to get it wrong (the host test's) ---------------------------------
def chunked_fp32(rowptr, col, h, a_src, a_dst, slope, Cg, fault=None):
    """the contract of spp.h f3h in fp32 torch ops, row by row: per chunk a two-pass softmax state (m, s, acc), chunk 0
    with the self loop, the states merged in chunk order.  ``fault``: "no_rescale" merges s and acc without f1 / f2,
    "self_everywhere" puts the self loop into every chunk, "keep_diag" does not skip diagonal entries,
    "head0_everywhere" gives every column head 0's logits, "merge_skips_last" never merges the last chunk of a row of
    three or more chunks."""
    assert fault is None or fault in FAULTS
    h, a_src, a_dst = h.float(), a_src.float(), a_dst.float()
    if fault == "head0_everywhere":
        a_src, a_dst = a_src[:, :1].expand_as(a_src), a_dst[:, :1].expand_as(a_dst)
    sl = torch.tensor(slope, dtype=torch.float32)
    out = torch.empty_like(h)
    for t in range(h.size(0)):
        raw = col[int(rowptr[t]):int(rowptr[t + 1])].tolist()
        chunks = max(1, -(-len(raw) // Cg))
        state = None
        for c in range(chunks):
            if fault == "merge_skips_last" and chunks >= 3 and c == chunks - 1:
                continue
            js = [j for j in raw[c * Cg:(c + 1) * Cg] if j != t or fault == "keep_diag"]
            if c == 0 or fault == "self_everywhere":
                js = [t] + js
            if not js:
                continue                                                    # an empty chunk merges as nothing
            v = h[js]
            pre = a_src[js] + a_dst[t]
            e = torch.where(pre > 0, pre, pre * sl)                         # [n, H]
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
