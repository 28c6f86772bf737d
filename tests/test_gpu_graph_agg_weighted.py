"""spp_graph_agg_weighted_forward and spp_gcn_dinv (csrc/graph_agg_weighted.hip, spp.h f3s) through
inference.graph_weighted_aggregate and inference.gcn_dinv: the summation contract pinned bit for bit where it can be (rows
of at most C entries against spp_agg_weighted_forward, long rows with power-of-two weights against an fp32 restatement of
the contract on the CPU), bounded against float64 for general weights, the in-kernel gcn_norm coefficients against
spp_gcn_norm's, and the independence of a row's result from the launch."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FS = [1, 3, 4, 100, 128, 256]
XDTYPES = [torch.float32, torch.float16, torch.bfloat16]
OUT_DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -24
_name = lambda d: str(d).split(".")[-1]


def _chunk():
    from salient_plusplus_amd.inference import graph_agg_chunk
    return graph_agg_chunk()


@functools.lru_cache(maxsize=None)
def _graph():
    """~400 nodes: degrees 0, 1, 2, C-1, C, C+1, 2C, 3C+5, a hub of 20C+3, self-loops, repeated neighbours side by side
    and ordinary rows of 3..15 entries; (rowptr, col) on the CPU"""
    Cc = _chunk()
    assert Cc >= 32
    g = torch.Generator().manual_seed(11)
    N = 401
    deg = torch.randint(3, 16, (N,), generator=g)
    special = {0: 0, 5: 1, 9: 2, 17: Cc - 1, 33: Cc, 64: Cc + 1, 130: 2 * Cc, 131: 3 * Cc + 5, 200: 20 * Cc + 3, 259: 0,
               260: Cc + 1, N - 1: 2 * Cc + 1}
    for k, v in special.items():
        deg[k] = v
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    for t in (5, 9, 17, 64, 131, 200, 300):                    # self-loops
        col[rowptr[t]] = t
    for t in (9, 33, 130, 200, 301):                           # repeated neighbours, side by side
        col[rowptr[t + 1] - 1] = col[rowptr[t + 1] - 2]
    col[rowptr[200] + 7] = 0                                   # the hub reads a zero-degree node (dinv 0 with fill 0)
    return rowptr, col


@functools.lru_cache(maxsize=None)
def _dev_graph():
    rowptr, col = _graph()
    return rowptr.cuda(), col.cuda()


def _sizes():
    rowptr, col = _graph()
    return rowptr.numel() - 1, col.numel()


def _deg():
    rowptr, _ = _graph()
    return rowptr[1:] - rowptr[:-1]


@functools.lru_cache(maxsize=None)
def _x(F_, dtype):
    N, _E = _sizes()
    x = torch.randn((N, F_), generator=torch.Generator().manual_seed(100 + F_)) * 2.0
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def _weights(kind):
    """(weight [E], self_weight [N]) fp32 on the CPU: "randn", "pow2" (+-2^e, e in [-3, 3]) or "positive" (0.25 .. 2.25,
    edge weights a gcn_norm accepts)"""
    N, E = _sizes()
    g = torch.Generator().manual_seed({"randn": 1, "pow2": 2, "positive": 3}[kind])
    if kind == "randn":
        return torch.randn(E, generator=g), torch.randn(N, generator=g)
    if kind == "positive":
        return torch.rand(E, generator=g) * 2 + 0.25, None
    def draw(n):
        sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
        return sign * torch.exp2(torch.randint(-3, 4, (n,), generator=g).float())
    return draw(E), draw(N)


def _wagg(x, **kw):
    from salient_plusplus_amd.inference import graph_weighted_aggregate
    rowptr, col = _dev_graph()
    if not any(k in kw for k in ("row0", "target_ids")):
        kw.update(row0=0, num_targets=x.size(0))
    return graph_weighted_aggregate(x, rowptr, col, **kw)


def _cuda(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("xdtype", XDTYPES, ids=_name)
@pytest.mark.parametrize("F_", FS)
def test_short_rows_are_the_hop_kernels_bits(F_, xdtype):
    """item 1: with randn weights and a randn self_weight, rows of d <= C equal spp_agg_weighted_forward
    (models.weighted_aggregate) over the whole graph as one hop (T = S = N) bit for bit; the bf16 output equals the fp32
    output rounded once, on every row"""
    from salient_plusplus_amd.models import weighted_aggregate
    rowptr, col = _dev_graph()
    N, _E = _sizes()
    short = (_deg() <= _chunk()).cuda()
    assert int(short.sum()) >= 390 and int((~short).sum()) >= 6
    x = _x(F_, xdtype).cuda()
    w, sw = (t.cuda() for t in _weights("randn"))
    hop = weighted_aggregate(x, rowptr, col, w, N, sw)
    assert hop.dtype == torch.float32
    got = _wagg(x, weight=w, self_weight=sw)
    assert got.dtype == torch.float32 and got.shape == (N, F_)
    assert torch.equal(got[short], hop[short])
    got16 = _wagg(x, weight=w, self_weight=sw, out_dtype=torch.bfloat16)
    assert got16.dtype == torch.bfloat16
    assert torch.equal(got16, got.to(torch.bfloat16))
    hop_plain = weighted_aggregate(x, rowptr, col, w, N)               # and without a self term
    assert torch.equal(_wagg(x, weight=w)[short], hop_plain[short])


def _contract32(x, rowptr, col, w, sw, t, Cc):
    """the contract in plain fp32 on the CPU: chunks of C from zero in CSR order, chunk sums added in chunk order, the
    self term last"""
    xf = x.float()
    b, e = int(rowptr[t]), int(rowptr[t + 1])
    total = torch.zeros(x.size(1), dtype=torch.float32)
    for cb in range(b, e, Cc):
        acc = torch.zeros(x.size(1), dtype=torch.float32)
        for k in range(cb, min(e, cb + Cc)):
            acc = acc + w[k] * xf[int(col[k])]
        total = total + acc
    if sw is not None:
        total = total + sw[t] * xf[t]
    return total


@pytest.mark.parametrize("xdtype", XDTYPES, ids=_name)
@pytest.mark.parametrize("F_", FS)
def test_long_rows_are_the_contract_bit_for_bit(F_, xdtype):
    """item 2: the weights are signed powers of two, +-2^e with e in [-3, 3], so every product w * x is exact in fp32 and
    fmaf(w, x, acc) IS the plain fp32 acc + w * x.  The CPU restatement in plain fp32 torch -- chunks of C from zero,
    chunk sums added in chunk order, the self term (a power of two as well) last -- is therefore the contract exactly,
    and every long row must equal it under torch.equal (the bf16 output: that, rounded once)"""
    rowptr_c, col_c = _graph()
    Cc = _chunk()
    long_rows = torch.nonzero(_deg() > Cc).flatten().tolist()
    assert len(long_rows) >= 6
    xc = _x(F_, xdtype)
    w, sw = _weights("pow2")
    want = torch.stack([_contract32(xc, rowptr_c, col_c, w, sw, t, Cc) for t in long_rows])
    want_plain = torch.stack([_contract32(xc, rowptr_c, col_c, w, None, t, Cc) for t in long_rows])
    x = xc.cuda()
    got = _wagg(x, weight=w.cuda(), self_weight=sw.cuda())
    assert torch.equal(got[long_rows].cpu(), want)
    assert torch.equal(_wagg(x, weight=w.cuda())[long_rows].cpu(), want_plain)
    got16 = _wagg(x, weight=w.cuda(), self_weight=sw.cuda(), out_dtype=torch.bfloat16)
    assert torch.equal(got16[long_rows].cpu(), want.to(torch.bfloat16))
    ids = torch.tensor(long_rows[::-1], dtype=torch.int64).cuda()    # the same rows named by a list
    assert torch.equal(_wagg(x, weight=w.cuda(), self_weight=sw.cuda(), target_ids=ids).cpu(), want.flip(0))


@pytest.mark.parametrize("xdtype", XDTYPES, ids=_name)
@pytest.mark.parametrize("F_", FS)
def test_general_weights_hold_the_bound_against_float64(F_, xdtype):
    """item 3: |err| <= (C + ceil(d / C) + 3) * 2^-24 * sum |c_k x_k| (the self term in the sum) against float64 over the
    fp32 weights as exact numbers -- one rounding per fmaf of a chunk, the additions across chunks, the self term -- and
    2^-8 |result| more for a bf16 output; every row, short and long"""
    rowptr_c, col_c = _graph()
    N, _E = _sizes()
    Cc, deg = _chunk(), _deg()
    xc = _x(F_, xdtype)
    w, sw = _weights("randn")
    rows = torch.repeat_interleave(torch.arange(N), deg)
    prod = w.double().unsqueeze(1) * xc.double()[col_c]
    self_term = sw.double().unsqueeze(1) * xc.double()
    want = torch.zeros((N, F_), dtype=torch.float64).index_add_(0, rows, prod) + self_term
    mag = torch.zeros((N, F_), dtype=torch.float64).index_add_(0, rows, prod.abs()) + self_term.abs()
    n = (Cc + torch.ceil(deg.double() / Cc) + 3).unsqueeze(1)
    for odt in OUT_DTYPES:
        got = _wagg(xc.cuda(), weight=w.cuda(), self_weight=sw.cuda(), out_dtype=odt)
        bound = n * U * mag
        if odt == torch.bfloat16:
            bound = bound + 2.0 ** -8 * want.abs()
        err = (got.double().cpu() - want).abs()
        print(f"F={F_} {xdtype} -> {odt}: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("fill", [0, 1, 2])
def test_in_kernel_coefficients_are_gcn_norms_bits(fill, weighted):
    """item 4: graph_weighted_aggregate(dinv=gcn_dinv(...), fill=...) equals graph_weighted_aggregate(weight=coef,
    self_weight=self_coef) with models.gcn_norm's coefficients of the whole graph, on every row, short and long: this pins
    spp_gcn_dinv to spp_gcn_norm's dinv and the in-kernel expressions to k_gcn_coef.  Nodes 0 and 259 have no entries:
    with fill = 0 their dinv is 0, and the hub reads node 0"""
    from salient_plusplus_amd.inference import gcn_dinv
    from salient_plusplus_amd.models import gcn_norm
    rowptr, col = _dev_graph()
    N, _E = _sizes()
    w = _cuda(_weights("positive")[0]) if weighted else None
    kw = dict(add_self_loops=fill > 0, improved=fill == 2)
    dinv = gcn_dinv(rowptr, w, **kw)
    assert dinv.dtype == torch.float32 and dinv.shape == (N,) and bool(torch.isfinite(dinv).all())
    zero_deg = (_deg() == 0).cuda()
    assert bool(((dinv[zero_deg] == 0) if fill == 0 else ((dinv[zero_deg] - fill ** -0.5).abs() < 1e-6)).all())
    coef, self_coef = gcn_norm(rowptr, col, N, w, **kw)
    for F_, xdtype in ((3, torch.float32), (128, torch.float16), (100, torch.bfloat16)):
        x = _x(F_, xdtype).cuda()
        for odt in OUT_DTYPES:
            got = _wagg(x, weight=w, dinv=dinv, fill=fill, out_dtype=odt)
            want = _wagg(x, weight=coef, self_weight=self_coef, out_dtype=odt)
            assert torch.equal(got, want), (F_, xdtype, odt)
            assert bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("xdtype", XDTYPES, ids=_name)
@pytest.mark.parametrize("F_", FS)
def test_no_weights_is_the_plain_sum(F_, xdtype):
    """item 5: weight=None without dinv is graph_aggregate(epilogue="sum", self_scale=0) on every row: a weight of 1 makes
    the fmaf a plain addition, in the same order"""
    from salient_plusplus_amd.inference import graph_aggregate
    rowptr, col = _dev_graph()
    N, _E = _sizes()
    x = _x(F_, xdtype).cuda()
    for odt in OUT_DTYPES:
        want = graph_aggregate(x, rowptr, col, row0=0, num_targets=N, epilogue="sum", self_scale=0.0, out_dtype=odt)
        assert torch.equal(_wagg(x, out_dtype=odt), want)


@pytest.mark.parametrize("mode", ["explicit", "dinv"])
@pytest.mark.parametrize("F_,xdtype", [(3, torch.float32), (128, torch.float16), (100, torch.bfloat16)])
def test_a_rows_result_does_not_depend_on_the_launch(F_, xdtype, mode):
    """item 6: one slab, slabs of 1 / 7 / 130 rows (row0 != 0), a shuffled id list with duplicates and a second run give
    equal bits; ids outside the graph give zero rows; a strided view of a wider table reads the right columns"""
    from salient_plusplus_amd.inference import gcn_dinv, graph_agg_workspace_bytes
    rowptr, col = _dev_graph()
    N, _E = _sizes()
    x = _x(F_, xdtype).cuda()
    if mode == "explicit":
        w, sw = (t.cuda() for t in _weights("randn"))
        kw = dict(weight=w, self_weight=sw)
    else:
        w = _weights("positive")[0].cuda()
        kw = dict(weight=w, dinv=gcn_dinv(rowptr, w), fill=1)
    full = _wagg(x, **kw)
    assert torch.equal(_wagg(x, **kw), full)                                # a second run
    ws = torch.empty(graph_agg_workspace_bytes(130), dtype=torch.uint8, device="cuda")
    for rows in (1, 7, 130):
        out = torch.full_like(full, float("nan"))
        for s in range(0, N, rows):
            n = min(rows, N - s)
            _wagg(x, row0=s, num_targets=n, out=out[s:s + n], workspace=ws, **kw)
        assert torch.equal(out, full), rows
    g = torch.Generator().manual_seed(5)
    ids = torch.cat([torch.randperm(N, generator=g), torch.tensor([200, 200, 0, 131, 64])])
    assert torch.equal(_wagg(x, target_ids=ids.cuda(), **kw), full[ids.cuda()])
    outside = torch.tensor([200, -1, N, 3, 1 << 40, -(1 << 40), 131], dtype=torch.int64)
    got = _wagg(x, target_ids=outside.cuda(), **kw)
    inside = ((outside >= 0) & (outside < N)).cuda()
    assert torch.equal(got[inside], full[outside.cuda()[inside]])
    assert bool((got[~inside] == 0).all())
    for first in (4, 1):                                                    # 4: rows stay vector-aligned; 1: they do not
        wide = torch.randn((N, F_ + 12), generator=torch.Generator().manual_seed(9)).to(xdtype).cuda()
        wide[:, first:first + F_] = x
        assert torch.equal(_wagg(wide[:, first:first + F_], **kw), full), first


def test_the_wrapper_is_forward_only():
    """item 7: an x or a weight that requires grad is refused, as graph_aggregate refuses it"""
    x = _x(4, torch.float32).cuda()
    w, sw = (t.cuda() for t in _weights("randn"))
    with pytest.raises(RuntimeError, match="x requires grad"):
        _wagg(x.clone().requires_grad_(), weight=w)
    with pytest.raises(RuntimeError, match="weight requires grad"):
        _wagg(x, weight=w.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="self_weight requires grad"):
        _wagg(x, weight=w, self_weight=sw.clone().requires_grad_())
    out = _wagg(x, weight=w, self_weight=sw)
    assert not out.requires_grad and out.grad_fn is None
    assert math.isfinite(float(out.abs().sum()))
