"""Float64 restatement of the GAT training kernels (csrc/gat.hip: k_gat_mh_rowdot, k_gat_mh_agg_fwd,
k_gat_mh_agg_bwd, k_gat_mh_gx_gather, k_gat_mh_colsum, k_gat_fwd, k_gat_bwd) with a per-element rounding bound next to
every value, and the planted hop and logit regimes the tests run them on.  A helper: no tests in here.  Everything is on
the CPU, vectorised, in float64; the fp32 / fp16 / bf16 inputs convert to float64 exactly.

The formulas (H heads, the header comments of gat.hip).  Row i's softmax entries are its CSR entries without the
diagonal ones (col == i) plus one self loop; n_i counts them.
  logits    a_src = x Vsrc^T [S, H],  a_dst = x[:T] Vdst^T [T, H]
  forward   raw_ij = a_src[j] + a_dst[i],  e_ij = raw > 0 ? raw : raw * slope,  m_i = max_j e_ij,  w_ij = exp(e_ij - m_i),
            s_i = sum_j w_ij,  alpha_ij = w_ij / s_i,  z[i,h,:] = sum_j alpha_ij x_j      (row_max = m, row_sum = s)
  backward  go_i = g_i . z_i,  gh_ij = g_i . x_j,  ge_ij = alpha_ij (gh_ij - go_i) (raw_ij > 0 ? 1 : slope),
            grad_a_dst[i] = sum_j ge_ij,  grad_a_src[j] = sum_i ge_ij,
            alpha_e = alpha per CSR entry (0 for a dropped diagonal entry),  alpha_self = alpha of the self loop,
            grad_x (atomic form)[s,:] = sum_i sum_h alpha_is g[i,h,:],
            grad_x (gather form) = that + grad_a_src Vsrc, and for s < T + grad_a_dst Vdst
  logits backward   grad_V = grad_a^T x
The slope is the fp32 number the kernel receives: SLOPES[0] = float(float32(0.2)), not 0.2; SLOPES[1] = 0.25 is exact.

The bounds.  u = 2^-24.  A sum of n fp32 terms, each a rounded product, added in ANY order (a lane's chain, a butterfly,
atomics) is within n u sum|term| of the exact sum to first order (each term meets its product's rounding and at most
n - 1 additions), so a K-term dot product has c = K + 1 whatever its lane count and butterfly depth, and a row's chain has
c = n_i + 1.  M is always the reference expression with every term replaced by its absolute value.
  EXP0 = 1e-6: the relative accuracy of __expf at |arg| <= 8, the figure tests/test_gpu_gat_inference.py works with;
      scaled linearly, eps_exp(d) = EXP0 max(1, d / 8) <= EXP0 + (EXP0 / 8) d  for  d = |arg|.
  The logit of an entry as the kernel has it: fl(fl(a_src + a_dst) * slope) is within 2 u |raw| of e (one addition, one
      product; both exact in the planted regimes at slope 0.25).  row_max is the maximum of such fp32 numbers, so it is
      compared bit for bit with the same two fp32 operations done on the CPU (row_max32).
  A weight of the forward.  The online softmax holds w_ij as a product of at most R_i + 1 factors exp(.), R_i the number of
      times the running maximum rises along the row in the kernel's order (self loop first, then the CSR order; counted
      here from the exact logits, an upper bound since rounding is monotone); their arguments have one sign and add up to
      d_ij = m_i - e_ij.  Each factor: its subtraction u |arg|, eps_exp(|arg|); each rescale one more product u.  So
      delta_ij = (R_i + 1) EXP0 + (EXP0 / 8 + u) d_ij + u R_i + 2 u (|raw_ij| + |raw of the row's maximum|).
  Anything below 2^-126 (FLUSH) may be flushed to zero or rounded as a subnormal: an absolute 2^-126 per operation that can
      underflow (the R_i + 1 exponentials and rescales of a weight plus one; exp and the product by 1 / s in the backward).
  z:        sum_j |x_j| bw_ij / s_i + M_z (sum_j bw_ij / s_i + (2 n_i + 4) u),   bw_ij = w_ij delta_ij + (R_i + 2) FLUSH:
            the weights' own errors in the numerator and in the denominator, the chain of n_i products and additions in
            both ((n_i + 1) u and n_i u), the reciprocal (2 u) and the final product (u).
  row_sum:  sum_j bw_ij + n_i u s_i.
  alpha in the backward: one exponential, then the product by 1 / row_sum:
            dalpha_ij = 2 u (|raw_ij| + |raw of the maximum|) + u d_ij + eps_exp(d_ij) + bound_s_i / s_i + 3 u
            (the kernel reads the forward's fp32 row_sum: its bound is propagated; reciprocal 2 u, product u);
            bound_alpha = alpha dalpha + 2 FLUSH.
  go:       (K + 1) u sum_c |g z| + sum_c |g| bound_z   (the kernel reads the forward's fp32 z);   gh: (K + 1) u sum_c |g x|.
  ge:       lrelu' (alpha (bound_gh + bound_go) + (bound_alpha + 3 u alpha)(|gh| + |go|)) + FLUSH  (a subtraction, two
            products).
  grad_a_dst: sum_j bound_ge + n_i u sum_j |ge|.      grad_a_src: the same over the entries naming s (atomics: any order).
  grad_x, atomic form: sum |g| bound_alpha + (H + cnt_s + 1) u sum alpha |g|: H products summed per entry, cnt_s atomics.
  grad_x, gather form: its accumulator takes L_s = H (entries naming s, dropped ones included (their weight is an exact
            0) + 1 + 2 [s < T]) products one after the other: (L_s + 1) u M, plus the bounds of what it reads:
            sum |g| bound_alpha + bound_gas |Vsrc| + bound_gad |Vdst|.  gather_from_parts() is the same kernel judged
            alone, from the fp32 alpha_e / alpha_self / grad_a it actually read: (L_s + 1) u M only.
  logits:   (K + 1) u sum_c |x v|.      grad_V: (rows + 1) u sum_j |grad_a x|, rows = S (src), T (dst).
  Second order: every relative first-order term above is below 2^-11 at these shapes ((R + 1) EXP0 <= 1.31e-4,
      (K + 1) u <= 6.2e-5, eps_exp(104) = 1.3e-5), so products of two of them are below 2^-11 of the bound:
      every bound built from more than one rounding is multiplied by G2 = 1 + 2^-10.
None of these constants comes from GPU output."""
import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
EXP0 = 1e-6
FLUSH = 2.0 ** -126
G2 = 1.0 + 2.0 ** -10
SLOPES = (float(np.float32(0.2)), 0.25)
COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130]
HUB_LO = 26                                                # a target (s < T) whose own row is empty
Q = 2.0 ** -10
REGIMES = ["ascending", "descending", "equal", "selfmax", "selfmin", "mixed", "wide"]      # + "model" (the caller's x.V)
F64 = torch.float64


class Hop:
    """A CSR hop and the softmax entry list of the formulas: entry k of (r, s) is the k-th kept CSR entry (CSR id eid[k]),
    followed by the T self loops.  seq [T, L]: the entries of a row in the kernels' order (self loop, then CSR order),
    -1 padded.  keep_diag=True restates the hop WITHOUT dropping diagonal entries (a planted fault of the host test)."""

    def __init__(self, rowptr, col, T, S, keep_diag=False):
        self.rowptr, self.col, self.T, self.S, self.E = rowptr, col, T, S, int(col.numel())
        ar = torch.arange(T)
        self.row = torch.repeat_interleave(ar, rowptr[1:] - rowptr[:-1])
        self.keep = torch.ones_like(self.col, dtype=torch.bool) if keep_diag else self.col != self.row
        self.eid = torch.nonzero(self.keep).flatten()
        self.nk = nk = int(self.eid.numel())
        self.r = torch.cat([self.row[self.keep], ar])
        self.s = torch.cat([self.col[self.keep], ar])
        self.kept = torch.bincount(self.row[self.keep], minlength=T)
        self.n = self.kept + 1
        self.named = torch.bincount(self.s, minlength=S)             # softmax entries naming s (self loop included)
        self.listed = torch.bincount(col, minlength=S)               # CSR entries naming s (dropped ones included)
        L = int(self.n.max()) if T else 1
        self.seq = torch.full((T, L), -1, dtype=torch.int64)
        if T:
            self.seq[:, 0] = nk + ar
            start = torch.cumsum(self.kept, 0) - self.kept
            rk = self.row[self.keep]
            self.seq[rk, 1 + torch.arange(nk) - start[rk]] = torch.arange(nk)

    def one_row(self, t):
        """row t alone as a T = 1 hop: target 0 is source t, so ids 0 and t trade places"""
        b, e = int(self.rowptr[t]), int(self.rowptr[t + 1])
        col = self.col[b:e].clone()
        swap = col.clone()
        swap[col == t], swap[col == 0] = 0, t
        perm = torch.arange(self.S)
        perm[0], perm[t] = t, 0
        return Hop(torch.tensor([0, e - b]), swap, 1, self.S), perm


@functools.lru_cache(maxsize=None)
def planted_hop(T=70, S=200):
    """The planted hop, (70, 200) or the square (70, 70).
    kept-entry counts cycle through COUNTS (t = 69 has 130: at 8 targets a wavefront it shares the last wavefront with
    two groups past T; t = 25 and 64 have 130 next to the empty rows 26 and 65; t = 12 has 130 next to t = 13, which is
    made of diagonal entries only);  diagonal entries first / last / mid-round in the rows of 5 (t = 5, 18, 31) and of 65
    (t = 11, 24, 37);  a row of k >= 4 is [f, f, others ascending by id, HUB_LO, hub_hi] (k = 1: [hub_hi], 2: [HUB_LO] * 2,
    3: [HUB_LO, HUB_LO, hub_hi]): it repeats its first source, and every row of 3 or more names both hubs, HUB_LO = 26 < T
    and hub_hi (S - 11 >= T; in the square hop 52);  the hubs' own rows are empty;  every other source a row t names has
    an id above t (so the self loop can be a row's strict maximum or minimum for all rows at once), drawn with repeats
    from (t, S - 10), the hubs when that is empty;  the last 10 sources are named by nobody."""
    assert T == 70 and S in (70, 200)
    hub_hi = S - 11 if S > T else 52
    g = torch.Generator().manual_seed(T * 1000 + S)
    counts = [COUNTS[t % len(COUNTS)] for t in range(T)]
    counts[69] = 130
    diag = {5: [0], 18: [5], 31: [2], 11: [0], 24: [65], 37: [33], 13: [0, 0, 0]}     # positions in the finished row
    rows = []
    for t, k in enumerate(counts):
        cand = torch.tensor([j for j in range(t + 1, S - 10) if j not in (HUB_LO, hub_hi)], dtype=torch.int64)
        if k == 0:
            row = []
        elif k == 1:
            row = [hub_hi]
        elif k <= 3:
            row = [HUB_LO, HUB_LO] + [hub_hi] * (k - 2)
        elif cand.numel() == 0:
            row = [HUB_LO] * (k - 1) + [hub_hi]
        else:
            others = sorted(cand[torch.randint(0, cand.numel(), (k - 3,), generator=g)].tolist())
            row = [others[0]] + others + [HUB_LO, hub_hi]
        assert len(row) == k
        for p in diag.get(t, []):
            row.insert(p, t)
        rows.append(row)
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    hop = Hop(rowptr, torch.tensor([j for r in rows for j in r], dtype=torch.int64), T, S)
    hop.hub_hi, hop.counts = hub_hi, counts
    return hop


def sinks(hop):
    """sources that head no kept entry: the non-targets and the targets whose rows keep nothing"""
    out = torch.ones(hop.S, dtype=torch.bool)
    out[:hop.T] = hop.kept == 0
    return out


def regime(name, hop, H):
    """(a_src [S, H], a_dst [T, H]) in fp32: a_src even and a_dst odd multiples of Q = 2^-10 below 128, so raw = a_src +
    a_dst is exact in fp32 and never 0."""
    S, T = hop.S, hop.T
    s = torch.arange(S, dtype=torch.int64).unsqueeze(1)
    h = torch.arange(H, dtype=torch.int64).unsqueeze(0)
    a_dst = (2 * ((7 * torch.arange(T).unsqueeze(1) + 3 * h) % 32) - 31).double() * Q
    sink = sinks(hop).unsqueeze(1)
    if name in ("ascending", "descending"):                # along every row; the self loop is the row's minimum / maximum
        key = s.clone()
        key[HUB_LO], key[hop.hub_hi] = S, S + 1
        a = ((key - S // 2) * (24 + 8 * h)).double()
        a = a if name == "ascending" else -a
    elif name == "equal":                                  # one logit per head, the self loop's included
        a = (((-1) ** h) * 8 * (64 + 2 * h)).double().expand(S, H)
    elif name in ("selfmax", "selfmin"):                   # strictly; the others in no order
        a = torch.where(sink, -(1024 + 2 * ((37 * s + 11 * h) % 1024)), 1024 + 32 * (T - s) + 0 * h).double()
        a = a if name == "selfmax" else -a
    elif name == "mixed":                                  # both LeakyReLU branches in every row of n >= 2
        sign = torch.where((s + h) % 2 == 0, 1, -1)
        kept = torch.cat([hop.kept, torch.zeros(S - T, dtype=torch.int64)]).unsqueeze(1)
        sign = torch.where(kept == 1, -1, torch.where(kept == 2, 1, sign))
        sign[HUB_LO], sign[hop.hub_hi] = -1, 1
        a = (sign * (256 + 2 * ((29 * s + 5 * h) % 512))).double()
    elif name == "wide":                                   # raw spread up to 120 in a row: weights underflow to 0
        a = (-20 * 1024 + 2 * ((7919 * s + 131 * h) % 61440)).double()
        a[HUB_LO], a[hop.hub_hi] = -20 * 1024, 100 * 1024
    else:
        raise ValueError(name)
    a_src = (a * Q).float()
    a_dst = a_dst.float()
    assert bool((a_src.double() == a * Q).all()) and float(a_src.abs().max()) + float(a_dst.abs().max()) < 128
    raw = a_src[hop.s] + a_dst[hop.r]
    assert bool((raw.double() == a_src[hop.s].double() + a_dst[hop.r].double()).all()) and bool((raw != 0).all())
    return a_src, a_dst


@functools.lru_cache(maxsize=None)
def values(S, T, K, H, dtype, seed=0):
    """x [S, K] in dtype, V [2, H, K] and g [T, H, K] in fp32"""
    g = torch.Generator().manual_seed(seed + 1000 * K + H)
    x = (0.5 * torch.randn((S, K), generator=g)).to(dtype)
    V = torch.randn((2, H, K), generator=g) / K ** 0.5
    return x, V, torch.randn((T, H, K), generator=g)


def lrelu(raw, slope):
    return torch.where(raw > 0, raw, raw * slope)


def row_max32(hop, a_src, a_dst, slope):
    """row_max as the kernel has it: the maximum of fl(fl(a_src + a_dst) * slope), in fp32"""
    raw = a_src.float()[hop.s] + a_dst.float()[hop.r]
    e = torch.where(raw > 0, raw, raw * torch.tensor(slope, dtype=torch.float32))
    H = a_src.size(1)
    return torch.full((hop.T, H), -float("inf")).scatter_reduce(0, hop.r.unsqueeze(1).expand(-1, H), e, "amax")


def _dense(hop, v):
    """[H, T, S]: the entries' values v [N, H] summed per (target, source)"""
    return torch.zeros((hop.T, hop.S, v.size(1)), dtype=F64).index_put_((hop.r, hop.s), v, accumulate=True).permute(2, 0, 1)


def _over_sources(A, x):
    """[T, H, K] = sum_s A[h, t, s] x[s, :]"""
    H, T, S = A.shape
    return (A.reshape(H * T, S) @ x).view(H, T, -1).permute(1, 0, 2)


def _over_targets(A, g):
    """[S, K] = sum_h sum_t A[h, t, s] g[t, h, :]"""
    return torch.bmm(A.transpose(1, 2), g.permute(1, 0, 2)).sum(0)


def _pair_dots(g, x):
    """[T, S, H] = g[t, h, :] . x[s, :]"""
    T, H, K = g.shape
    return (g.reshape(T * H, K) @ x.t()).view(T, H, -1).permute(0, 2, 1)


def _rows(n, idx, v):
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=F64).index_add_(0, idx, v)


def logits(x, V, T):
    """a_src, a_dst and their bounds"""
    x, V = x.double(), V.double()
    c = (x.size(1) + 1) * U
    return types.SimpleNamespace(a_src=x @ V[0].t(), b_src=c * (x.abs() @ V[0].abs().t()),
                                 a_dst=x[:T] @ V[1].t(), b_dst=c * (x[:T].abs() @ V[1].abs().t()))


def logits_backward(x, gas, gad, T):
    """grad_V [2, H, K] and its bound, from the grad_a the kernel is given"""
    x, gas, gad = x.double(), gas.double(), gad.double()
    gv = torch.stack([gas.t() @ x, gad.t() @ x[:T]])
    b = torch.stack([(x.size(0) + 1) * U * (gas.abs().t() @ x.abs()), (T + 1) * U * (gad.abs().t() @ x[:T].abs())])
    return gv, b


def forward(hop, x, a_src, a_dst, slope):
    x, a_src, a_dst = x.double(), a_src.double(), a_dst.double()
    T, H, r, s = hop.T, a_src.size(1), hop.r, hop.s
    raw = a_src[s] + a_dst[r]
    e = lrelu(raw, slope)
    m = torch.full((T, H), -float("inf"), dtype=F64).scatter_reduce(0, r.unsqueeze(1).expand(-1, H), e, "amax")
    d = m[r] - e
    w = torch.exp(-d)
    ssum = _rows(T, r, w)
    alpha = w / ssum[r]
    ep = torch.cat([e, torch.full((1, H), -float("inf"), dtype=F64)])[hop.seq]       # [T, L, H]
    R = (ep[:, 1:] > torch.cummax(ep, 1).values[:, :-1]).sum(1).double()             # rises of the running maximum
    rawm = torch.where(m > 0, m, m / slope).abs()
    n = hop.n.double().unsqueeze(1)
    delta = (R[r] + 1) * EXP0 + (EXP0 / 8 + U) * d + U * R[r] + 2 * U * (raw.abs() + rawm[r])
    bw = w * delta + (R[r] + 2) * FLUSH
    A, B = _dense(hop, alpha), _dense(hop, bw / ssum[r])
    z = _over_sources(A, x)
    Mz = _over_sources(A, x.abs())
    rel = _rows(T, r, bw / ssum[r]) + (2 * n + 4) * U
    bz = G2 * (_over_sources(B, x.abs()) + Mz * rel.unsqueeze(2))
    bs = G2 * (_rows(T, r, bw) + n * U * ssum)
    return types.SimpleNamespace(z=z, bz=bz, row_max=m, row_sum=ssum, bs=bs, alpha=alpha, raw=raw, e=e, d=d, R=R,
                                 rawm=rawm, A=A, Mz=Mz)


def backward(hop, x, a_src, a_dst, g, slope, V=None, fw=None):
    """closed-form gradients of sum(z * g) and their bounds; V [2, H, K]: the gather form's grad_x too"""
    fw = fw or forward(hop, x, a_src, a_dst, slope)
    x, g = x.double(), g.double()
    T, S, H, K, r, s, nk = hop.T, hop.S, g.size(1), x.size(1), hop.r, hop.s, hop.nk
    xa, ga = x.abs(), g.abs()
    alpha, raw = fw.alpha, fw.raw
    go, b_go = (g * fw.z).sum(2), (K + 1) * U * (ga * fw.z.abs()).sum(2) + (ga * fw.bz).sum(2)
    gh = _pair_dots(g, x)[r, s]
    gha = _pair_dots(ga, xa)[r, s]
    b_gh = (K + 1) * U * gha
    dl = torch.where(raw > 0, 1.0, slope).double()
    d_alpha = (2 * U * (raw.abs() + fw.rawm[r]) + U * fw.d + EXP0 * torch.clamp(fw.d / 8, min=1.0)
               + fw.bs[r] / fw.row_sum[r] + 3 * U)
    b_alpha = G2 * alpha * d_alpha + 2 * FLUSH
    ge = alpha * (gh - go[r]) * dl
    spread = gh.abs() + go[r].abs()
    b_ge = G2 * dl * (alpha * (b_gh + b_go[r]) + (b_alpha + 3 * U * alpha) * spread) + FLUSH
    n = hop.n.double().unsqueeze(1)
    named = hop.named.double().unsqueeze(1)
    out = types.SimpleNamespace(fw=fw, ge=ge)
    out.gad, out.b_gad = _rows(T, r, ge), _rows(T, r, b_ge) + n * U * _rows(T, r, ge.abs())
    out.gas, out.b_gas = _rows(S, s, ge), _rows(S, s, b_ge) + named * U * _rows(S, s, ge.abs())
    out.alpha_e, out.b_alpha_e = torch.zeros((hop.E, H), dtype=F64), torch.zeros((hop.E, H), dtype=F64)
    out.alpha_e[hop.eid], out.b_alpha_e[hop.eid] = alpha[:nk], b_alpha[:nk]
    out.alpha_self, out.b_alpha_self = alpha[nk:], b_alpha[nk:]
    A, Bm = fw.A, _dense(hop, b_alpha)
    out.gx = _over_targets(A, g)
    gxm = _over_targets(A, ga)
    b_read = _over_targets(Bm, ga)
    out.b_gx = G2 * (b_read + (H + named + 1) * U * gxm)
    if V is not None:
        V = V.double()
        is_t = (torch.arange(S) < T).double().unsqueeze(1)
        chain = H * (hop.listed.double().unsqueeze(1) + 1 + 2 * is_t)
        out.gx_gather, mag = out.gx + out.gas @ V[0], gxm + out.gas.abs() @ V[0].abs()
        b_read = b_read + out.b_gas @ V[0].abs()
        out.gx_gather[:T] += out.gad @ V[1]
        mag[:T] += out.gad.abs() @ V[1].abs()
        b_read[:T] += out.b_gad @ V[1].abs()
        out.b_gx_gather = G2 * (b_read + (chain + 1) * U * mag)
    return out


def gather_from_parts(hop, g, alpha_e, alpha_self, gas, gad, V):
    """k_gat_mh_gx_gather alone: grad_x and its bound from the fp32 values it read"""
    g, V, gas, gad = g.double(), V.double(), gas.double(), gad.double()
    T, S, H = hop.T, hop.S, g.size(1)
    A = torch.zeros((T, S, H), dtype=F64).index_put_((hop.row, hop.col), alpha_e.double(), accumulate=True)
    ar = torch.arange(T)
    A[ar, ar] += alpha_self.double()
    A = A.permute(2, 0, 1)
    gx, mag = _over_targets(A, g), _over_targets(A.abs(), g.abs())
    gx, mag = gx + gas @ V[0], mag + gas.abs() @ V[0].abs()
    gx[:T] += gad @ V[1]
    mag[:T] += gad.abs() @ V[1].abs()
    is_t = (torch.arange(S) < T).double().unsqueeze(1)
    chain = H * (hop.listed.double().unsqueeze(1) + 1 + 2 * is_t)
    return gx, G2 * (chain + 1) * U * mag + FLUSH


def worst(got, ref, bound, hop=None):
    """(largest err / bound, a description of the element): every element compared; an element whose bound is 0 must be
    exact"""
    err = (got.detach().double().cpu() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    if ratio.numel() == 0:
        return 0.0, "empty"
    k = int(ratio.argmax())
    idx = tuple(int(v) for v in np.unravel_index(k, tuple(ratio.shape)))
    where = f"index {idx} (row, head, column as the output has them)"
    if hop is not None and idx and ratio.size(0) == hop.T:
        where += f", row length {int(hop.n[idx[0]])}"
    return float(ratio.flatten()[k]), f"{where}: err {float(err.flatten()[k]):.3e} bound {float(bound.expand_as(err).flatten()[k]):.3e}"
