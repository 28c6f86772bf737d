"""-m gpu: the edge-weighted aggregation kernels (csrc/aggregate_weighted.hip: spp_agg_weighted_forward / _backward /
_wgrad, spp_gcn_norm) against float64 restatements computed on the CPU.

Bounds (u = 2^-24; the inputs -- fp32 / fp16 / bf16 rows, fp32 weights and gradients -- are exact in float64):
  forward, per element:  (d + 2) u (|self_w x_t| + sum_k |w_k x_k|), d the row's length: the standard bound of a chain of
      d + 1 fmafs; a bf16 output adds 2^-8 |ref|.
  grad_x, per element:   the same form with the source's in-degree in place of d; a bf16 gradient adds 2^-8 |ref|, an
      fp16 one (rounded from fp32 by torch) 2^-10 |ref|: twice the format's half-ulp, as the bf16 term is, plus 2^-25,
      half the spacing of fp16's subnormals.
  grad_weight, grad_self_weight:  (F + 1) u sum_c |g x|.
  gcn_norm, relative:    (d_max + 8) u: the row sum, sqrtf, the division and the two products."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEGS = [3, 0, 1, 2, 4, 65, 7]                            # the pair loop and its tail, an empty row, a long row
WIDTHS = [1, 3, 4, 64, 132, 256]                         # scalar form; vector form, a partial last lane step included
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
_ID = dict(ids=lambda v: str(v).split(".")[-1])
SHAPES = [(20, 200), (70, 70)]                           # (T, S): T < S and T == S


@functools.lru_cache(maxsize=None)
def hop(T=20, S=200):
    """(rowptr, col, weight, self_weight) on the CPU.  Degrees cycle through DEGS; every row of two or more entries names
    its first source twice; the last 10 sources (and, for T < S, others) are named by nobody; weights are negative,
    zero and positive."""
    g = torch.Generator().manual_seed(T * 1000 + S)
    deg = torch.tensor([DEGS[t % len(DEGS)] for t in range(T)])
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    col = torch.randint(0, S - 10, (E,), generator=g)
    for t in range(T):
        if deg[t] >= 2:
            col[int(rowptr[t]) + 1] = col[int(rowptr[t])]
    w = torch.randn(E, generator=g)
    w[::7] = 0.0
    sw = torch.randn(T, generator=g)
    sw[1] = 0.0
    return rowptr, col, w, sw


@functools.lru_cache(maxsize=None)
def values(F, rows, dtype, seed=1):
    return torch.randn((rows, F), generator=torch.Generator().manual_seed(seed + F)).to(dtype)


def dense(rowptr, col, w, T, S):
    """(A, |A|) in float64: A[t, s] = the sum of row t's weights on source s"""
    row = torch.repeat_interleave(torch.arange(T), rowptr[1:] - rowptr[:-1])
    A = torch.zeros((T, S), dtype=torch.float64).index_put_((row, col), w.double(), accumulate=True)
    Aa = torch.zeros((T, S), dtype=torch.float64).index_put_((row, col), w.double().abs(), accumulate=True)
    return A, Aa


def expected(rows, T, S, self_w):
    """(ref, bound) of the forward over the float64 rows `rows` [S, F]"""
    rowptr, col, w, sw = hop(T, S)
    A, Aa = dense(rowptr, col, w, T, S)
    ref, mag = A @ rows, Aa @ rows.abs()
    if self_w:
        ref = ref + sw.double().unsqueeze(1) * rows[:T]
        mag = mag + (sw.double().unsqueeze(1) * rows[:T]).abs()
    d = (rowptr[1:] - rowptr[:-1]).double().unsqueeze(1)
    return ref, (d + 2) * U * mag


def within(got, ref, bound, extra=0.0, floor=0.0):
    err = (got.double().cpu() - ref).abs()
    lim = bound + extra * ref.abs() + floor
    assert bool((err <= lim).all()), f"max excess {float((err - lim).max()):.3e} (max err {float(err.max()):.3e})"


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def run(x, T, S, self_w, amp=False, graph=None):
    from salient_plusplus_amd.models import weighted_aggregate
    rowptr, col, w, sw = graph or hop(T, S)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        return weighted_aggregate(x, rowptr.cuda(), col.cuda(), w.cuda(), T, sw.cuda() if self_w else None)


def strided(x, pad):
    """x's values in a matrix whose row stride is x.size(1) + pad"""
    out = torch.zeros((x.size(0), x.size(1) + pad), dtype=x.dtype, device="cuda")
    out[:, :x.size(1)] = x
    return out[:, :x.size(1)]


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("F", WIDTHS)
def test_forward_dense(F, dtype):
    for T, S in SHAPES:
        x = values(F, S, dtype)
        for self_w in (False, True):
            ref, bound = expected(x.double(), T, S, self_w)
            for pad in (4, 3):                               # F % 4 == 0: the vector form, then the scalar form
                xs = strided(x, pad)
                assert xs.stride(0) != F
                out = run(xs, T, S, self_w)
                assert out.dtype == torch.float32 and out.shape == (T, F)
                within(out, ref, bound)
                assert same(out, run(xs, T, S, self_w))                          # run to run
                ob = run(xs, T, S, self_w, amp=True)
                assert ob.dtype == torch.bfloat16
                within(ob, ref, bound, 2.0 ** -8)
                assert same(ob, out.to(torch.bfloat16))                          # the fp32 result rounded once
            if not self_w:
                assert bool((out[1] == 0).all())                                 # an empty row


@pytest.mark.parametrize("F,dtype", [(3, torch.float16), (4, torch.float32), (132, torch.bfloat16), (256, torch.float16)])
def test_forward_table_rows_and_row_refs(F, dtype):
    """TableRows (an id outside the table reads row 0) and RowRefs give the result over the materialised rows"""
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    T, S = SHAPES[0]
    g = torch.Generator().manual_seed(9)
    table = values(F, 500, dtype, seed=4)
    n_id = torch.randint(0, 500, (S,), generator=g)
    n_id[3], n_id[50], n_id[150], n_id[0] = -1, 500, 1 << 40, 7
    rows = table[torch.where((n_id >= 0) & (n_id < 500), n_id, 0)]
    padded = strided(table.cuda(), 12)
    mat = rows.cuda()
    addr = mat.data_ptr() + torch.arange(S, dtype=torch.int64) * (F * mat.element_size())
    refs = RowRefs(addr.cuda(), None, F, dtype, None, (mat,))
    for self_w in (False, True):
        ref, bound = expected(rows.double(), T, S, self_w)
        want = run(mat, T, S, self_w)
        within(want, ref, bound)
        for src in (TableRows(padded, n_id.cuda()), refs):
            out = run(src, T, S, self_w)
            within(out, ref, bound)
            assert same(out, want)                           # the same rows in the same order
            ob = run(src, T, S, self_w, amp=True)
            assert same(ob, want.to(torch.bfloat16))


@pytest.mark.parametrize("F", [3, 64, 132])
def test_a_rows_result_does_not_depend_on_the_call(F):
    """bit-identical whether the call holds all T rows or that row alone"""
    T, S = SHAPES[0]
    rowptr, col, w, sw = hop(T, S)
    for pad in (4, 3):
        x = strided(values(F, S, torch.float32), pad)
        full = run(x, T, S, False)
        for t in range(len(DEGS)):
            b, e = int(rowptr[t]), int(rowptr[t + 1])
            one = (torch.tensor([0, e - b]), col[b:e].clone(), w[b:e].clone(), None)
            if e == b:
                continue                                     # (an empty hop: test_smallest_shapes)
            assert same(run(x, 1, S, False, graph=one), full[t:t + 1]), t
        # with the self term: target 0 alone
        b, e = int(rowptr[0]), int(rowptr[1])
        one = (torch.tensor([0, e - b]), col[b:e].clone(), w[b:e].clone(), sw[:1].clone())
        assert same(run(x, 1, S, True, graph=one), run(x, T, S, True)[:1])


def _grads(x, T, S, self_w, g, amp=False):
    """(grad_x or None, grad_weight, grad_self_weight or None) through torch.autograd on weighted_aggregate"""
    from salient_plusplus_amd.models import weighted_aggregate
    rowptr, col, w, sw = hop(T, S)
    if isinstance(x, torch.Tensor):
        x = x.detach().requires_grad_(True)
    wq = w.cuda().requires_grad_(True)
    sq = sw.cuda().requires_grad_(True) if self_w else None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = weighted_aggregate(x, rowptr.cuda(), col.cuda(), wq, T, sq)
    out.backward(g.to(out.dtype))
    return (x.grad if isinstance(x, torch.Tensor) else None), wq.grad, (sq.grad if self_w else None)


def _expected_grads(rows, T, S, self_w, g):
    """float64 references and bounds: rows [S, F] and g [T, F] in float64"""
    rowptr, col, w, sw = hop(T, S)
    A, Aa = dense(rowptr, col, w, T, S)
    F = rows.size(1)
    gx, mag = A.t() @ g, Aa.t() @ g.abs()
    if self_w:
        gx[:T] += sw.double().unsqueeze(1) * g
        mag[:T] += (sw.double().unsqueeze(1) * g).abs()
    indeg = torch.bincount(col, minlength=S).double().unsqueeze(1)
    row = torch.repeat_interleave(torch.arange(T), rowptr[1:] - rowptr[:-1])
    prod = g[row] * rows[col]
    own = g * rows[:T]
    named = torch.zeros(S, dtype=torch.bool)
    named[col] = True
    if self_w:
        named[:T] = True
    return (gx, (indeg + 2) * U * mag, prod.sum(1), (F + 1) * U * prod.abs().sum(1), own.sum(1),
            (F + 1) * U * own.abs().sum(1), named)


# 300 (row stride 303: one column per lane, five column steps) and 1028 (four columns per lane, five steps) take the
# weight gradient's second round of registers
@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("F", WIDTHS + [300, 1028])
def test_backward(F, dtype):
    for T, S in SHAPES:
        x = values(F, S, dtype)
        g = torch.randn((T, F), generator=torch.Generator().manual_seed(F))
        for self_w in (False, True):
            want_gx, b_gx, want_gw, b_gw, want_gs, b_gs, named = _expected_grads(x.double(), T, S, self_w, g.double())
            for pad in (4, 3):
                xs = strided(x, pad)
                gx, gw, gs = _grads(xs, T, S, self_w, g.cuda())
                assert gx.dtype == dtype and gx.shape == (S, F) and gw.dtype == torch.float32 and gw.shape == want_gw.shape
                within(gx, want_gx, b_gx, {torch.float32: 0.0, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -8}[dtype],
                       floor=2.0 ** -25 if dtype == torch.float16 else 0.0)
                assert bool((~named).any()) or (self_w and T == S)
                assert bool((gx.cpu()[~named] == 0).all())                       # rows nobody names: exactly 0
                within(gw, want_gw, b_gw)
                if self_w:
                    assert gs.dtype == torch.float32
                    within(gs, want_gs, b_gs)
                gx2, gw2, gs2 = _grads(xs, T, S, self_w, g.cuda())
                assert same(gw, gw2) and (not self_w or same(gs, gs2))                  # run to run


def test_backward_under_bf16_autocast_and_only_the_gradients_asked_for():
    from salient_plusplus_amd.models import weighted_aggregate
    T, S = SHAPES[0]
    F = 64
    rowptr, col, w, sw = hop(T, S)
    x = values(F, S, torch.bfloat16).cuda()
    g = torch.randn((T, F), generator=torch.Generator().manual_seed(0)).bfloat16()
    want_gx, b_gx, want_gw, b_gw, want_gs, b_gs, _named = _expected_grads(x.double().cpu(), T, S, True, g.double())
    gx, gw, gs = _grads(x, T, S, True, g.cuda(), amp=True)
    assert gx.dtype == torch.bfloat16 and gw.dtype == gs.dtype == torch.float32
    within(gx, want_gx, b_gx, 2.0 ** -8)
    within(gw, want_gw, b_gw)
    within(gs, want_gs, b_gs)
    # nothing requires grad: no node; only x: no weight gradient; only self_weight: the others get None
    args = (rowptr.cuda(), col.cuda())
    assert not weighted_aggregate(x, *args, w.cuda(), T, sw.cuda()).requires_grad
    xq = x.float().requires_grad_(True)
    wq, sq = w.cuda(), sw.cuda().requires_grad_(True)
    weighted_aggregate(xq.detach(), *args, wq, T, sq).backward(g.float().cuda())
    assert xq.grad is None and wq.grad is None
    within(sq.grad, want_gs, b_gs)
    weighted_aggregate(xq, *args, wq, T, sw.cuda()).backward(g.float().cuda())
    within(xq.grad, want_gx, b_gx)


def test_weight_gradient_over_rows_read_in_place():
    """a TableRows / RowRefs source gets no gradient; the weights' gradient reads it in place"""
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    T, S = SHAPES[0]
    for F, dtype in ((3, torch.float16), (132, torch.bfloat16)):
        table = values(F, 300, dtype, seed=8)
        n_id = torch.randint(0, 300, (S,), generator=torch.Generator().manual_seed(F))
        n_id[5] = 300                                        # reads row 0
        rows = table[torch.where(n_id < 300, n_id, 0)]
        g = torch.randn((T, F), generator=torch.Generator().manual_seed(F))
        _gx, _bx, want_gw, b_gw, want_gs, b_gs, _n = _expected_grads(rows.double(), T, S, True, g.double())
        mat = rows.cuda()
        addr = mat.data_ptr() + torch.arange(S, dtype=torch.int64) * (F * mat.element_size())
        _none, dense_gw, dense_gs = _grads(mat, T, S, True, g.cuda())
        for src in (TableRows(strided(table.cuda(), 8), n_id.cuda()), RowRefs(addr.cuda(), None, F, dtype, None, (mat,))):
            none, gw, gs = _grads(src, T, S, True, g.cuda())
            assert none is None
            within(gw, want_gw, b_gw)
            within(gs, want_gs, b_gs)
            assert same(gw, dense_gw) and same(gs, dense_gs)


@pytest.mark.parametrize("kw", [dict(), dict(improved=True), dict(add_self_loops=False)],
                         ids=["default", "improved", "no_self_loops"])
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_gcn_norm(kw, weighted):
    from salient_plusplus_amd.models import _gcn_norm_reference, gcn_norm
    for T, S in SHAPES:
        rowptr, col, w, _sw = hop(T, S)
        w = w.abs() if weighted else None                    # non-negative, zeros included
        coef, self_coef = gcn_norm(rowptr.cuda(), col.cuda(), T, w.cuda() if weighted else None, **kw)
        assert coef.dtype == self_coef.dtype == torch.float32 and coef.shape == (col.numel(),) and self_coef.shape == (T,)
        want_c, want_s = _gcn_norm_reference(rowptr, col, T, w.double() if weighted else None, dtype=torch.float64, **kw)
        tol = (max(DEGS) + 8) * U
        for got, want in ((coef, want_c), (self_coef, want_s)):
            err = (got.double().cpu() - want).abs()
            assert bool((err <= tol * want.abs()).all()), float((err / want.abs().clamp(min=1e-300)).max())
        if not kw.get("add_self_loops", True):
            assert bool((coef.cpu()[col >= T] == 0).all()) and bool((self_coef == 0).all())
            assert bool((coef.cpu()[(col < T) & (col % len(DEGS) != 1)] > 0).any())
        c2, s2 = gcn_norm(rowptr.cuda(), col.cuda(), T, w.cuda() if weighted else None, **kw)
        assert same(c2, coef) and same(s2, self_coef)


def test_smallest_shapes():
    from salient_plusplus_amd.models import gcn_norm, weighted_aggregate
    x = torch.tensor([[1.0], [9.0], [4.0]]).cuda().requires_grad_(True)          # T = 1, F = 1
    rowptr, col = torch.tensor([0, 3]).cuda(), torch.tensor([2, 0, 2]).cuda()
    w = torch.tensor([0.5, -2.0, 1.0]).cuda().requires_grad_(True)
    sw = torch.tensor([3.0]).cuda().requires_grad_(True)
    out = weighted_aggregate(x, rowptr, col, w, 1, sw)
    assert out.tolist() == [[0.5 * 4 - 2.0 + 4.0 + 3.0]]
    out.backward(torch.tensor([[2.0]]).cuda())
    assert x.grad.tolist() == [[-4.0 + 6.0], [0.0], [3.0]]
    assert w.grad.tolist() == [8.0, 2.0, 8.0] and sw.grad.tolist() == [2.0]
    x.grad = None
    # an empty hop (no entries) and no targets at all
    for T, rp in ((2, [0, 0, 0]), (0, [0])):
        rp = torch.tensor(rp).cuda()
        none = torch.zeros(0, dtype=torch.int64).cuda()
        w0 = torch.zeros(0).cuda().requires_grad_(True)
        z = weighted_aggregate(x, rp, none, w0, T)
        assert z.shape == (T, 1) and bool((z == 0).all())
        z.sum().backward()
        assert x.grad.tolist() == [[0.0], [0.0], [0.0]] and w0.grad.shape == (0,)
        x.grad = None
        coef, self_coef = gcn_norm(rp, none, T)
        assert coef.shape == (0,) and self_coef.tolist() == [1.0] * T


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
def test_get_model_type_gcn_builds_a_model_that_takes_a_training_step(normalize):
    """the name resolves to ``models.GCN``; the class it returns trains on a two-hop MFG of this file's hops (outermost
    first: 70 sources -> 70 targets -> 20 targets) with their weights' magnitudes as ``adj_t``'s values"""
    import torch.nn.functional as F
    from salient_plusplus_amd.fast_trainer.monkeypatch import Adj, SparseTensor
    from salient_plusplus_amd.models import GCN, get_model_type
    cls = get_model_type("gcn")
    assert cls is GCN and get_model_type("GCN") is GCN
    adjs = []
    for T, S in ((70, 70), (20, 70)):
        rowptr, col, w, _sw = hop(T, S)
        m = SparseTensor(rowptr=rowptr.cuda(), row=None, col=col.cuda(), value=w.abs().cuda(), sparse_sizes=(T, S),
                         is_sorted=True, trust_data=True)
        adjs.append(Adj(m, None, (S, T)))
    torch.manual_seed(3)
    model = cls(64, 32, 5, 2, normalize=normalize).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    x = values(64, 70, torch.float16).cuda()
    y = torch.randint(0, 5, (20,), generator=torch.Generator().manual_seed(2)).cuda()
    before = [p.detach().clone() for p in model.parameters()]
    out = model(x, adjs)
    assert out.shape == (20, 5) and out.dtype == torch.float32
    loss = F.nll_loss(out, y)
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss))
    for i, conv in enumerate(model.convs):
        g = conv.lin.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, i
    moved = [not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters())]
    assert any(moved) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert int(model.bns[0].num_batches_tracked) == 1
