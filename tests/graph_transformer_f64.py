"""Float64 restatement of spp_graph_transformer_forward (csrc/graph_transformer.hip; spp.h f3z) over a whole graph, with a
per-element first-order rounding bound next to every value, the planted graph the tests run it on, and an fp32 CPU
emulation of the chunked softmax that can be told to go wrong.  A helper: no tests in here.  Everything is on the CPU;
fp32 / fp16 / bf16 inputs convert to float64 exactly.

The formula, per target t and head h (q, k, v [N, H, C] by global id, scale the fp32 number the kernel receives):
  e_j = scale sum_c q[t,h,c] k[j,h,c] over EVERY CSR entry j of row t (no self loop, diagonal kept, repeats counted; a
  ``col`` entry outside [0, N) is node 0),  alpha = softmax_j(e),  r = sum_j alpha_j v[j,h,:]  (0 for an empty row),
  then r + skip[t] if a skip is given, max(., 0) with relu.
``plain_rows`` states it row by row with torch.softmax; ``reference`` states it once more over the entry list
(transformer_f64.Entries) and adds the bounds.  Neither knows of chunks: a chunk only enters the BOUND, as a count of
roundings.

The bounds are tests/transformer_f64.py's forward bounds (u = U = 2^-24, EXP0, FLUSH, G2 from gat_f64; none of them from
GPU output) with what a long row adds, derived as tests/graph_gatv2_f64.py derives its own.  C_g = the kernel's chunk; a
row of n entries has max(1, ceil(n / C_g)) chunks and M = chunks - 1 merges; the entry at position p sits in chunk
p // C_g, and EVERY chunk starts from the empty state.
  logit   the C-term tree (C u sum_c |q k|) and ONE product by scale:  b_e = (C + 1) u scale sum_c |q k|,
          bm = max_j b_e over the row.
  weight  inside its chunk the online softmax holds w_j as a product of at most R + 1 factors exp(.), R the rises of
          the running maximum IN THAT CHUNK after the chunk's first entry (which meets the empty state: its rescale
          multiplies zeros by expf(-inf) = 0 and its own factor is expf(0) = 1, both exact).  A position counts as a
          rise whenever its exact logit comes within 2 bm of the running maximum of the exact logits.  Every merge
          the entry's state goes through multiplies it by ONE more factor exp(.) (f1 or f2) in at most TWO rounded
          operations (the product acc * f1 and the fma): at most M merges.  All factors' arguments have one sign and
          add up to the computed e_j - m:
            delta_j = (R + 1 + M) EXP0 + (EXP0 / 8 + u) d_j + u (R + 2 M) + b_e_j + bm,   d_j = m - e_j
            bw_j = w_j delta_j + (R + 2 + 2 M) FLUSH.
  result  sum_j |v[j]| bw_j / s + M_out (sum_j bw_j / s + (2 n + 4 + 2 M) u): chains of n products and additions for
          numerator and denominator plus one addition per merge, the reciprocal and the final product.  A row without
          entries is exact zeros: bound 0.
  skip    ONE rounded addition of an exact fp32 value: b' = b + u (|r + skip| + b).  The ReLU is exact and 1-Lipschitz:
          the bound stays.
  G2 = 1 + 2^-10 on the whole.  A bf16 OUTPUT adds one rounding of the computed value: ``widen_bf16``,
  b + 2^-8 (|ref| + b)."""
import functools
import types

import torch

import transformer_f64 as tf
from gat_f64 import EXP0, FLUSH, G2, U

F64 = torch.float64
N = 700
ISOLATED = N - 1          # no entries, named by nobody
EMPTY, ONE, ONLY_SELF, REPEATS, EXACT, PLUS_ONE, DOUBLED, CHUNK, HUB, MID, BAD_COL = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
OUTSIDE = N + 3           # the col entry that leaves the graph (row BAD_COL, position 1): node 0
REGIMES = tf.REGIMES + ["rising", "falling"]


def hub_length(D, Cg):
    """more than 2 * (256 / lpr) * C_g entries, lpr = min(64, D / 4) lanes a row: the long kernel's workgroup runs
    256 / lpr chunks a round, so the hub takes more than two rounds and the LDS double buffer is written a third time"""
    lpr = 1
    while lpr < min(64, D // 4):
        lpr *= 2
    return 2 * (256 // lpr) * Cg + Cg + 5


@functools.lru_cache(maxsize=None)
def planted_graph(Cg, hub):
    """About 700 nodes (ids drawn from [0, N - 1): nobody names ISOLATED).  EMPTY and ISOLATED have no entries, ONE has
    one, ONLY_SELF is [2], REPEATS has a repeated entry and a diagonal one, EXACT has C_g entries and PLUS_ONE
    C_g + 1, CHUNK is a row of C_g entries and DOUBLED that very row written twice, HUB has ``hub`` entries and MID
    3 C_g + 7, both SORTED by id (so a logit that grows with the source's id rises from chunk to chunk), BAD_COL is a
    short row whose second entry is OUTSIDE the graph; every other row has 0..12 random entries.  Returns
    transformer_f64.Entries over ``col`` with OUTSIDE read as node 0 (T = S = N) with col_raw (what the kernel gets),
    raw [N] and planted (the rows above)."""
    g = torch.Generator().manual_seed(17)
    lengths = {EMPTY: 0, ONE: 1, ONLY_SELF: 1, REPEATS: 5, EXACT: Cg, PLUS_ONE: Cg + 1, DOUBLED: 2 * Cg, CHUNK: Cg,
               HUB: hub, MID: 3 * Cg + 7, BAD_COL: 6, ISOLATED: 0}
    rows = []
    for t in range(N):
        n = lengths.get(t, int(torch.randint(0, 13, (1,), generator=g)))
        rows.append(torch.randint(0, N - 1, (n,), generator=g).tolist())
    rows[ONLY_SELF] = [ONLY_SELF]
    rows[REPEATS][1], rows[REPEATS][3] = rows[REPEATS][0], REPEATS
    rows[DOUBLED] = rows[CHUNK] + rows[CHUNK]
    rows[HUB], rows[MID] = sorted(rows[HUB]), sorted(rows[MID])
    rows[BAD_COL][1] = OUTSIDE
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    col_raw = torch.tensor([j for r in rows for j in r], dtype=torch.int64)
    ent = tf.Entries(rowptr, torch.where((col_raw >= 0) & (col_raw < N), col_raw, torch.zeros_like(col_raw)), N, N)
    ent.hub_hi = HUB
    ent.col_raw, ent.raw, ent.planted = col_raw, ent.n, sorted(lengths)
    return ent


def inputs(name, ent, H, C, dtype, seed=0):
    """(q, k, v, skip [N, H, C] in dtype).  The six regimes of transformer_f64.inputs, and two more built the same way
    (q = 1 in the even columns, k's even columns carry L * rs * 2 / C so that the logit is fl(scale * L rs)):
    "rising", L = (id - N / 2) / 8, and "falling", its negative -- over the id-sorted rows HUB and MID the logits then
    rise (fall) by 8 or more from one chunk to the next, so early (late) chunks end up rescaled to almost nothing."""
    base = name if name in tf.REGIMES else "equal"
    q, k, v, _g = tf.inputs(base, ent, H, C, torch.float32, seed)
    if name not in tf.REGIMES:
        rs = 1.0
        while rs * rs < C:
            rs *= 2.0
        L = (torch.arange(N, dtype=F64) - N // 2).unsqueeze(1).expand(N, H) / 8
        L = L if name == "rising" else -L
        k[:, :, 0::2] = (L * rs * 2.0 / C).float().unsqueeze(2)
    gen = torch.Generator().manual_seed(seed + 77 * C + H)
    skip = 0.5 * torch.randn((N, H, C), generator=gen)
    return q.to(dtype), k.to(dtype), v.to(dtype), skip.to(dtype)


def plain_rows(rowptr, col, q, k, v, scale, rows=None):
    """the formula row by row with torch.softmax, [len(rows), H, C] float64; nothing shared with ``reference``"""
    q, k, v = q.double(), k.double(), v.double()
    rows = range(q.size(0)) if rows is None else rows
    out = torch.zeros((len(rows),) + tuple(q.shape[1:]), dtype=F64)
    for i, t in enumerate(rows):
        js = [j if 0 <= j < q.size(0) else 0 for j in col[int(rowptr[t]):int(rowptr[t + 1])].tolist()]
        if js:
            e = scale * (q[t] * k[js]).sum(2)                               # [n, H]
            out[i] = (torch.softmax(e, 0).unsqueeze(2) * v[js]).sum(0)
    return out


def _rows(n, idx, v):
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=F64).index_add_(0, idx, v)


def reference(ent, q, k, v, scale, Cg, skip=None, relu=False):
    """out [N, H, C] and its bound b_out, both float64, for q, k, v (and skip) [N, H, C]"""
    q, k, v = q.double(), k.double(), v.double()
    T, H, C = q.shape
    r, s = ent.row, ent.col
    prod = q[r] * k[s]
    e = scale * prod.sum(2)                                                 # [E, H]
    b_e = G2 * (C + 1) * U * scale * prod.abs().sum(2)
    idx = r.unsqueeze(1).expand(-1, H)
    m = torch.full((T, H), -float("inf"), dtype=F64).scatter_reduce(0, idx, e, "amax")
    bm = torch.zeros((T, H), dtype=F64).scatter_reduce(0, idx, b_e, "amax")
    d = m[r] - e
    w = torch.exp(-d)
    ssum = _rows(T, r, w)
    alpha = w / ssum[r]
    # the chunk of every entry and the rises of the running maximum inside it (CSR order is (row, chunk, position) order)
    pos = torch.arange(ent.E) - ent.rowptr[:-1][r]
    chunk, posn = pos // Cg, pos % Cg
    first = posn == 0
    segno = torch.cumsum(first.long(), 0) - 1
    nseg = int(segno[-1]) + 1 if ent.E else 0
    ep = torch.full((nseg, Cg, H), -float("inf"), dtype=F64)
    ep[segno, posn] = e
    on = torch.zeros((nseg, Cg), dtype=torch.bool)
    on[segno, posn] = True
    bm_seg = bm[r[first]].unsqueeze(1)                                      # [segments, 1, H]
    rise = on[:, 1:].unsqueeze(2) & (ep[:, 1:] > torch.cummax(ep, 1).values[:, :-1] - 2 * bm_seg)
    R = rise.sum(1).double()[segno]                                         # [E, H]
    n = ent.n.double().unsqueeze(1)                                         # [T, 1]
    M = (torch.clamp((ent.n + Cg - 1) // Cg, min=1) - 1).double().unsqueeze(1)
    Mr = M[r]
    delta = (R + 1 + Mr) * EXP0 + (EXP0 / 8 + U) * d + U * (R + 2 * Mr) + b_e + bm[r]
    bw = w * delta + (R + 2 + 2 * Mr) * FLUSH
    a3, b3 = alpha.unsqueeze(2), (bw / ssum[r]).unsqueeze(2)
    out = _rows(T, r, a3 * v[s])
    Mo = _rows(T, r, a3 * v[s].abs())
    rel = _rows(T, r, bw / ssum[r]) + (2 * n + 4 + 2 * M) * U * (n > 0).double()
    b_out = _rows(T, r, b3 * v[s].abs()) + Mo * rel.unsqueeze(2)
    if skip is not None:
        out = out + skip.double()
        b_out = b_out + U * (out.abs() + b_out)
    if relu:
        out = torch.clamp(out, min=0)
    return types.SimpleNamespace(out=out, b_out=G2 * b_out, R=R, M=M.squeeze(1), e=e, chunk=chunk)


def widen_bf16(ref, bound):
    """the bound of a bf16 output: one more rounding, 2^-8 relative, of the computed value"""
    return bound + 2.0 ** -8 * (ref.abs() + bound)


# ---- a correct fp32 chunked computation in torch, and three ways to get it wrong (the host test's) --------------------
def chunked_fp32(rowptr, col, q, k, v, scale, Cg, skip=None, relu=False, fault=None, rows=None):
    """the contract of spp.h f3z in fp32 torch ops, row by row: per chunk of C_g entries a two-pass softmax state
    (m, s, acc) from nothing, the states merged in chunk order into chunk 0's, zeros for an empty row, then the skip and
    the ReLU.  ``fault``: "merge_order" hands the merge its two states the wrong way round (f1 scales the incoming state
    and f2 the running one), "dropped_chunk" never merges a row's last chunk, "no_rescale" merges without f1 / f2."""
    q, k, v = q.float(), k.float(), v.float()
    sc32 = torch.tensor(scale, dtype=torch.float32)
    rows = range(q.size(0)) if rows is None else rows
    out = torch.zeros((len(rows),) + tuple(q.shape[1:]), dtype=torch.float32)
    for i, t in enumerate(rows):
        raw = [j if 0 <= j < q.size(0) else 0 for j in col[int(rowptr[t]):int(rowptr[t + 1])].tolist()]
        chunks = -(-len(raw) // Cg)
        state = None
        for c in range(chunks):
            if fault == "dropped_chunk" and chunks > 1 and c == chunks - 1:
                continue
            js = raw[c * Cg:(c + 1) * Cg]
            e = (q[t] * k[js]).sum(2) * sc32                                # [n, H]
            mc = e.max(0).values
            wc = torch.exp(e - mc)
            s_c, a_c = wc.sum(0), (wc.unsqueeze(2) * v[js]).sum(0)
            if state is None:
                state = (mc, s_c, a_c)
                continue
            m0, s0, a0 = state
            mm = torch.maximum(m0, mc)
            f1, f2 = torch.exp(m0 - mm), torch.exp(mc - mm)
            if fault == "no_rescale":
                f1, f2 = torch.ones_like(f1), torch.ones_like(f2)
            if fault == "merge_order":
                f1, f2 = f2, f1
            state = (mm, s0 * f1 + s_c * f2, a0 * f1.unsqueeze(1) + a_c * f2.unsqueeze(1))
        if state is not None:
            out[i] = state[2] / state[1].unsqueeze(1)
        if skip is not None:
            out[i] = out[i] + skip[t].float()
    return torch.clamp(out, min=0) if relu else out
