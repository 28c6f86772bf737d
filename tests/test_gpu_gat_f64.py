"""-m gpu: the GAT training kernels (csrc/gat.hip: spp_gat_mh_logits, _aggregate_forward, _aggregate_backward in its
atomic and vector forms, _aggregate_backward_gather, _logits_backward; spp_gat_forward / spp_gat_backward) against the
float64 restatement and the per-element bounds of tests/gat_f64.py, on its planted hop and logit regimes.

Each stage is given the previous GPU stage's fp32 output and the reference is computed from the same values.  Every
element of every output is compared (an element whose bound is 0 -- a dropped diagonal entry's weight, the gradient row
of a source nobody names -- must be exactly 0).  Each test prints, per output quantity, the largest err / bound it saw
(GAT_F64_RATIO lines): a record, not an input to the bounds.

Largest err / bound seen on an MI355X: the docstring of test_zz_largest_ratios_seen.
test_gather_grad_x_is_identical_wherever_its_grad_a_src_is found the one fault: the transposed hop's order."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_f64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

ELEM = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
HEADS = [1, 2, 4, 8]
WIDTHS = [4, 8, 12, 64, 260, 1024]                         # 1024 on the square hop only
NAMES = ["model"] + G.REGIMES
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SEEN = collections.defaultdict(float)                      # quantity -> largest err / bound over the session


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat.load()


def _p(t):
    from salient_plusplus_amd.models import _p as p_
    return p_(t)


def _st():
    from salient_plusplus_amd.models import _stream
    return _stream()


def _al16(n):
    return (n + 15) // 16 * 16


class Run:
    """the spp_gat_mh_* entries on one hop, as test_gpu_gat_heads._Run calls them, with the slope as a parameter and
    the gather form's workspace read back; every output is a fresh fp32 tensor"""

    def __init__(self, x, hop, H, V, slope):
        self.x, self.hop, self.H, self.V, self.slope = x, hop, H, V.cuda(), slope
        self.rowptr, self.col = hop.rowptr.cuda(), hop.col.cuda()
        self.T, self.E = hop.T, hop.E
        self.S, self.K = x.shape
        self.elem = ELEM[x.dtype]
        self.xs = x.stride(0) if self.S > 1 else self.K

    def _f(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device="cuda")

    def _call(self, name, *args):
        rc = getattr(_lib(), name)(*args)
        assert rc == 0, (name, rc)

    def logits(self):
        a_src, a_dst = self._f(self.S, self.H), self._f(self.T, self.H)
        self._call("spp_gat_mh_logits", _p(self.x), self.elem, self.xs, self.S, self.T, self.K, self.H, _p(self.V[0]),
                   _p(self.V[1]), _p(a_src), _p(a_dst), _st())
        return a_src, a_dst

    def forward(self, a_src, a_dst):
        z, rmax, rsum = self._f(self.T, self.H, self.K), self._f(self.T, self.H), self._f(self.T, self.H)
        self._call("spp_gat_mh_aggregate_forward", _p(self.rowptr), _p(self.col), self.T, _p(self.x), self.elem,
                   self.xs, self.K, self.H, _p(a_src), _p(a_dst), self.slope, _p(z), _p(rmax), _p(rsum), _st())
        return z, rmax, rsum

    def backward_atomic(self, a_src, a_dst, z, rmax, rsum, g, want_gx=True):
        g_x = self._f(self.S, self.K, zero=True) if want_gx else None
        g_as, g_ad = self._f(self.S, self.H, zero=True), self._f(self.T, self.H)
        self._call("spp_gat_mh_aggregate_backward", _p(self.rowptr), _p(self.col), self.T, _p(self.x), self.elem,
                   self.xs, self.K, self.H, _p(a_src), _p(a_dst), self.slope, _p(z), _p(rmax), _p(rsum), _p(g), _p(g_x),
                   _p(g_as), _p(g_ad), _st())
        return g_x, g_as, g_ad

    def backward_gather(self, a_src, a_dst, z, rmax, rsum, g):
        """(grad_x, grad_a_src, grad_a_dst, alpha_e [E, H], alpha_self [T, H]); the workspace starts as NaN"""
        L = _lib()
        g_x = self._f(self.S, self.K)
        g_as, g_ad = self._f(self.S, self.H, zero=True), self._f(self.T, self.H)
        nbytes = int(L.spp_gat_mh_aggregate_backward_gather_workspace_bytes(self.T, self.S, self.E, self.H))
        assert nbytes >= 0 and nbytes % 4 == 0
        ws = torch.full((max(nbytes // 4, 4),), float("nan"), dtype=torch.float32, device="cuda")
        self._call("spp_gat_mh_aggregate_backward_gather", _p(self.rowptr), _p(self.col), self.T, self.S, self.E,
                   _p(self.x), self.elem, self.xs, self.K, self.H, _p(a_src), _p(a_dst), self.slope, _p(z), _p(rmax),
                   _p(rsum), _p(g), _p(self.V[0]), _p(self.V[1]), _p(g_x), _p(g_as), _p(g_ad), _p(ws), nbytes, _st())
        # alpha_e [E, H] | alpha_self [T, H], each 16-byte aligned (gat_aggregate_backward_gather)
        n_e, off = self.E * self.H, _al16(4 * self.H * self.E) // 4
        alpha_e = ws[:n_e].view(self.E, self.H).clone()
        alpha_self = ws[off:off + self.T * self.H].view(self.T, self.H).clone()
        return g_x, g_as, g_ad, alpha_e, alpha_self

    def logits_backward(self, g_as, g_ad):
        g_V = self._f(2, self.H, self.K)
        self._call("spp_gat_mh_logits_backward", _p(self.x), self.elem, self.xs, self.S, self.T, self.K, self.H,
                   _p(g_as), _p(g_ad), _p(g_V[0]), _p(g_V[1]), _st())
        return g_V


def shape_of(K):
    return (70, 70) if K == 1024 else (70, 200)


def on_gpu(x, strided):
    """x on the GPU; strided: as a column slice of a wider matrix (row stride K + 8, 4 columns in)"""
    if not strided:
        return x.cuda()
    wide = torch.zeros((x.size(0), x.size(1) + 8), dtype=x.dtype, device="cuda")
    wide[:, 4:4 + x.size(1)] = x
    out = wide[:, 4:4 + x.size(1)]
    assert out.stride(0) != x.size(1) or x.size(0) == 1
    return out


class Checks:
    """collects (quantity, err / bound, where); fail() at the end names every quantity over its bound"""

    def __init__(self, hop, tag):
        self.hop, self.tag, self.bad, self.top = hop, tag, [], collections.defaultdict(float)

    def within(self, what, got, ref, bound):
        assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
        ratio, where = G.worst(got, ref, bound, self.hop)
        self.top[what] = max(self.top[what], ratio)
        SEEN[what] = max(SEEN[what], ratio)
        if not ratio <= 1.0:
            self.bad.append(f"{what} [{self.tag}] err/bound {ratio:.3f} at {where}")

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what} [{self.tag}] is not exact")

    def done(self):
        print("\nGAT_F64_RATIO " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.top.items())))
        assert not self.bad, "\n".join(self.bad)


def pipeline(c, hop, x_cpu, V, g_cpu, name, slope, strided):
    """every entry once on (hop, x, regime `name`), each stage judged from the fp32 values it was given"""
    T, S, H = hop.T, hop.S, V.size(1)
    c.tag = f"{name} slope {slope:.3g} {'strided' if strided else 'dense'}"
    r = Run(on_gpu(x_cpu, strided), hop, H, V, slope)
    g = g_cpu.cuda()
    a_src, a_dst = r.logits()
    lg = G.logits(x_cpu, V, T)
    c.within("a_src", a_src, lg.a_src, lg.b_src)
    c.within("a_dst", a_dst, lg.a_dst, lg.b_dst)
    if name != "model":
        a_src, a_dst = (t.cuda() for t in G.regime(name, hop, H))
    as_c, ad_c = a_src.cpu(), a_dst.cpu()
    # forward
    z, rmax, rsum = r.forward(a_src, a_dst)
    bw = G.backward(hop, x_cpu, as_c, ad_c, g_cpu, slope, V)
    fw = bw.fw
    c.within("z", z, fw.z, fw.bz)
    c.within("row_sum", rsum, fw.row_sum, fw.bs)
    c.exact("row_max", torch.equal(rmax.cpu(), G.row_max32(hop, as_c, ad_c, slope)))
    # backward, atomic form, with and without grad_x (the vector form)
    unnamed = torch.nonzero(hop.named == 0).flatten()
    assert bool((unnamed >= T).all()) and (unnamed.numel() >= 10 or S == T or not hasattr(hop, "hub_hi"))
    for want_gx in (True, False):
        gx, gas, gad = r.backward_atomic(a_src, a_dst, z, rmax, rsum, g, want_gx)
        form = "atomic" if want_gx else "vector"
        c.within(f"grad_a_src/{form}", gas, bw.gas, bw.b_gas)
        c.within(f"grad_a_dst/{form}", gad, bw.gad, bw.b_gad)
        if want_gx:
            c.within("grad_x/atomic", gx, bw.gx, bw.b_gx)
            c.exact("grad_x/atomic of unnamed sources", bool((gx.cpu()[unnamed] == 0).all()))
            gas_a, gad_a = gas, gad
    # backward, gather form, and what it left in the workspace
    gx, gas, gad, alpha_e, alpha_self = r.backward_gather(a_src, a_dst, z, rmax, rsum, g)
    c.within("grad_a_src/gather", gas, bw.gas, bw.b_gas)
    c.within("grad_a_dst/gather", gad, bw.gad, bw.b_gad)
    c.within("grad_x/gather", gx, bw.gx_gather, bw.b_gx_gather)
    c.exact("grad_x/gather of unnamed sources", bool((gx.cpu()[unnamed] == 0).all()))
    ref, bound = G.gather_from_parts(hop, g_cpu, alpha_e.cpu(), alpha_self.cpu(), gas.cpu(), gad.cpu(), V)
    c.within("grad_x/gather from its inputs", gx, ref, bound)
    c.within("alpha_e", alpha_e, bw.alpha_e, bw.b_alpha_e)
    c.within("alpha_self", alpha_self, bw.alpha_self, bw.b_alpha_self)
    c.exact("alpha_e of dropped diagonal entries", bool((alpha_e.cpu()[~hop.keep] == 0).all()))
    one = alpha_self.double().cpu() + torch.zeros((T, H), dtype=torch.float64).index_add_(0, hop.row, alpha_e.double().cpu())
    b_one = bw.b_alpha_self + torch.zeros((T, H), dtype=torch.float64).index_add_(0, hop.row, bw.b_alpha_e)
    c.within("alpha sums to 1", one, torch.ones_like(one), b_one)
    # logits backward, from the atomic form's fp32 gradients
    gv = r.logits_backward(gas_a, gad_a)
    ref, bound = G.logits_backward(x_cpu, gas_a.cpu(), gad_a.cpu(), T)
    c.within("grad_V", gv, ref, bound)
    for t in (z, rsum, gx, gas, gad, gv):
        c.exact("finite", bool(torch.isfinite(t).all()))
    return dict(a_src=a_src, a_dst=a_dst, z=z, rmax=rmax, rsum=rsum, gad=gad, gas=gas, gx=gx, alpha_e=alpha_e,
                alpha_self=alpha_self)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("K", WIDTHS)
@pytest.mark.parametrize("H", HEADS)
def test_every_entry_within_its_bound_on_the_planted_hop(H, K, dtype):
    """all regimes at the slope the models use (float32(0.2)); two of them again at 0.25, where LeakyReLU is exact"""
    T, S = shape_of(K)
    hop = G.planted_hop(T, S)
    x, V, g = G.values(S, T, K, H, dtype)
    c = Checks(hop, "")
    for i, name in enumerate(NAMES):
        pipeline(c, hop, x, V, g, name, G.SLOPES[0], strided=i % 2 == 1)
    for i, name in enumerate(("mixed", "model")):
        pipeline(c, hop, x, V, g, name, G.SLOPES[1], strided=i % 2 == 0)
    c.done()


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("H", HEADS)
def test_logits_and_their_gradient_past_one_colsum_workgroup_and_at_one_row(H, dtype):
    """S = 1030 is a second k_gat_mh_colsum workgroup of 6 rows: with targets among them (T = 1027) and without (T = 5)"""
    c = Checks(None, "")
    for S, T, K in ((1030, 1027, 8), (1030, 5, 8), (1, 1, 8), (1, 1, 260)):
        c.tag = f"S {S} T {T} K {K}"
        x, V, _ = G.values(S, T, K, H, dtype, seed=3)
        gen = torch.Generator().manual_seed(S + T)
        gas, gad = torch.randn((S, H), generator=gen), torch.randn((T, H), generator=gen)
        hop = G.Hop(torch.zeros(T + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), T, S)
        for strided in (False, True):
            r = Run(on_gpu(x, strided), hop, H, V, G.SLOPES[0])
            a_src, a_dst = r.logits()
            lg = G.logits(x, V, T)
            c.within("a_src", a_src, lg.a_src, lg.b_src)
            c.within("a_dst", a_dst, lg.a_dst, lg.b_dst)
            gv = r.logits_backward(gas.cuda(), gad.cuda())
            ref, bound = G.logits_backward(x, gas, gad, T)
            c.within("grad_V", gv, ref, bound)
    c.done()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


TWICE = [(8, 2, torch.float16), (12, 1, torch.float32), (64, 8, torch.bfloat16), (260, 4, torch.float32)]


def _twice(K, H, dtype, name):
    T, S = shape_of(K)
    hop = G.planted_hop(T, S)
    x, V, g = G.values(S, T, K, H, dtype)
    c = Checks(hop, "")
    one = pipeline(c, hop, x, V, g, name, G.SLOPES[0], strided=True)
    two = pipeline(c, hop, x, V, g, name, G.SLOPES[0], strided=True)
    c.done()
    return hop, one, two


@pytest.mark.parametrize("K,H,dtype", TWICE, **_ID)
def test_what_is_written_without_atomics_is_identical_run_to_run(K, H, dtype):
    for name in ("model", "wide"):
        _hop, one, two = _twice(K, H, dtype, name)
        for k in ("a_src", "a_dst", "z", "rmax", "rsum", "gad", "alpha_e", "alpha_self"):
            assert _same(one[k], two[k]), (name, k)


@pytest.mark.parametrize("K,H,dtype", TWICE, **_ID)
def test_gather_grad_x_is_identical_wherever_its_grad_a_src_is(K, H, dtype):
    """The gather form's grad_x row s is written without atomics from grad_a_src[s], alpha and grad_z, so two runs
    whose grad_a_src[s] agree must agree on it bit for bit.

    The regression test of the transposed hop's order (transpose_hop.hip.h).  k_tr_fill places entry (t, s) at
    start[s] + atomicAdd(&cursor[s], 1): within a wavefront that order is fixed, but T = 70 is two wavefronts, and which
    of them reaches a shared source's cursor first changes from run to run.  Before k_tr_order put every segment into
    ascending CSR position, 2 to 7 of the planted hop's 200 rows (sources named 9 to 19 times) differed between two
    runs in three of these four cases although their grad_a_src rows were equal; the values were within their bounds.
    (The hops of tests/test_gpu_gat_heads.py that assert this property have T = 37: one wavefront.)"""
    for name in ("model", "wide"):
        hop, one, two = _twice(K, H, dtype, name)
        same = (one["gas"] == two["gas"]).all(1)
        differ = same & (one["gx"] != two["gx"]).any(1)
        print(f"\nGAT_F64_GATHER_ROWS {name}: {int(same.sum())} rows with equal grad_a_src, {int(differ.sum())} of them "
              f"differ; their sources are named {hop.listed[differ.cpu()].tolist()} times")
        assert bool(same.any()) and _same(one["gx"][same], two["gx"][same]), name


PLANTED_ROWS = list(range(13)) + [13, 18, 24, 25, 31, 37, 64, 69]


@pytest.mark.parametrize("K", [8, 64, 260])
def test_a_rows_result_does_not_depend_on_its_wavefront_neighbours(K):
    """row t of the full call against a hop of that row alone (T = 1; target 0 is source t, so sources 0 and t trade
    places): the forward and grad_a_dst bit for bit, in the vector and in the atomic form"""
    T, S, H = 70, 200, 2
    hop = G.planted_hop(T, S)
    x, V, g = G.values(S, T, K, H, torch.float16)
    for name in ("model", "mixed"):
        r = Run(x.cuda(), hop, H, V, G.SLOPES[0])
        a_src, a_dst = r.logits() if name == "model" else (t.cuda() for t in G.regime(name, hop, H))
        z, rmax, rsum = r.forward(a_src, a_dst)
        gads = [r.backward_atomic(a_src, a_dst, z, rmax, rsum, g.cuda(), want_gx)[2] for want_gx in (True, False)]
        for t in PLANTED_ROWS:
            one, perm = hop.one_row(t)
            r1 = Run(x[perm].cuda(), one, H, V, G.SLOPES[0])
            as1, ad1 = a_src[perm.cuda()].contiguous(), a_dst[t:t + 1].contiguous()
            z1, m1, s1 = r1.forward(as1, ad1)
            assert _same(z1, z[t:t + 1]) and _same(m1, rmax[t:t + 1]) and _same(s1, rsum[t:t + 1]), (name, t)
            for want_gx, full in zip((True, False), gads):
                gad1 = r1.backward_atomic(as1, ad1, z1, m1, s1, g[t:t + 1].cuda(), want_gx)[2]
                assert _same(gad1, full[t:t + 1]), (name, t, want_gx)


def test_smallest_shapes():
    K, H = 8, 2
    x, V, g = G.values(3, 2, K, H, torch.float32, seed=5)
    none = torch.zeros(0, dtype=torch.int64)
    # T = 0: nothing to write; the gather form's grad_x is all rank-1 terms of a zero grad_a_src
    hop = G.Hop(torch.zeros(1, dtype=torch.int64), none, 0, 3)
    r = Run(x.cuda(), hop, H, V, G.SLOPES[0])
    a_src, a_dst = r.logits()
    z, rmax, rsum = r.forward(a_src, a_dst)
    assert z.shape == (0, H, K)
    gx, gas, _gad, _ae, _as = r.backward_gather(a_src, a_dst, z, rmax, rsum, torch.zeros((0, H, K)).cuda())
    assert bool((gx == 0).all()) and bool((gas == 0).all())
    gx, gas, _ = r.backward_atomic(a_src, a_dst, z, rmax, rsum, torch.zeros((0, H, K)).cuda())
    assert bool((gx == 0).all()) and bool((gas == 0).all())
    # T = 1 with an empty row, T = S = 1, and E = 0 with two targets in the gather form
    for T, S in ((1, 3), (1, 1), (2, 3)):
        hop = G.Hop(torch.zeros(T + 1, dtype=torch.int64), none, T, S)
        c = Checks(hop, "")
        out = pipeline(c, hop, x[:S], V, g[:T], "model", G.SLOPES[0], strided=False)
        c.done()
        assert torch.equal(out["z"], x[:T].cuda().unsqueeze(1).expand(T, H, K))              # z = x_t
        assert bool((out["rsum"] == 1).all()) and bool((out["alpha_self"] == 1).all())
        raw = out["a_src"][:T] + out["a_dst"]
        assert torch.equal(out["rmax"], torch.where(raw > 0, raw, raw * torch.tensor(G.SLOPES[0], device="cuda")))


@pytest.mark.parametrize("F", [1, 3, 47, 64, 130])
def test_the_full_width_kernels_within_the_same_bounds(F):
    """spp_gat_forward / spp_gat_backward through models._GatAggregate: the H = 1 references and bounds"""
    from salient_plusplus_amd.models import _GatAggregate
    T, S = 70, 200
    hop = G.planted_hop(T, S)
    h, V, g = G.values(S, T, F, 1, torch.float32)
    rowptr, col = hop.rowptr.cuda(), hop.col.cuda()
    c = Checks(hop, "")
    for i, name in enumerate(NAMES):
        slope = G.SLOPES[i % 2]
        c.tag = f"{name} slope {slope:.3g}"
        if name == "model":
            a_src, a_dst = h @ V[0].t(), h[:T] @ V[1].t()
        else:
            a_src, a_dst = G.regime(name, hop, 1)
        hq = h.cuda().requires_grad_(True)
        asq, adq = a_src[:, 0].cuda().requires_grad_(True), a_dst[:, 0].cuda().requires_grad_(True)
        out = _GatAggregate.apply(hq, asq, adq, rowptr, col, slope)
        out.backward(g[:, 0].cuda())
        bw = G.backward(hop, h, a_src, a_dst, g, slope)
        c.within("full-width z", out.detach().unsqueeze(1), bw.fw.z, bw.fw.bz)
        c.within("full-width grad_a_src", asq.grad.unsqueeze(1), bw.gas, bw.b_gas)
        c.within("full-width grad_a_dst", adq.grad.unsqueeze(1), bw.gad, bw.b_gad)
        c.within("full-width grad_h", hq.grad, bw.gx, bw.b_gx)
        unnamed = hop.named == 0
        c.exact("full-width grad_h of unnamed sources", bool((hq.grad.cpu()[unnamed] == 0).all()))
    c.done()


def test_zz_largest_ratios_seen():
    """prints the largest err / bound per output quantity over the tests of this module that ran before it.

    Seen on an MI355X (a record, not an input to the bounds): a_src 0.44, a_dst 0.47, z 0.37, row_sum 0.20, row_max exact,
    grad_a_src 0.18 (all three forms), grad_a_dst 0.04 / 0.03 / 0.03 (atomic / vector / gather), grad_x atomic 0.31,
    grad_x gather 0.27 (0.67 from the fp32 values the kernel read: there the bound is the accumulator's chain alone),
    alpha_e 0.45, alpha_self 0.31, alpha's sum 0.17, grad_V 0.50; the full-width kernels: z 0.07, grad_h 0.31,
    grad_a_src 0.16, grad_a_dst 0.02.  None is near 1; the largest are plain dot products and chains (a_src, grad_V,
    the gather accumulator), where c u M has no slack but the sign pattern of the roundings."""
    print("\nGAT_F64_LARGEST " + " ".join(f"{k}={v:.3f}" for k, v in sorted(SEEN.items())))
