"""-m gpu: the max aggregation kernels (csrc/aggregate_max.hip: spp_agg_max_forward / spp_agg_max_backward) against the
plain-torch restatement models._max_reference computed on the CPU.  A maximum rounds nothing, so every comparison is
torch.equal on bit patterns: out, arg, and (integer-valued gradients, exact fp32 sums in any order) grad_x."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

T, S = 67, 200
DEGS = [0, 1, 2, 3, 8, 9, 64, 65, 130]                   # both tails of the two-in-flight loop, short and long rows
WIDTHS = [1, 6, 100, 128, 260]                           # scalar form, vector form, more than one column step a lane
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAN_ROW, NINF_ROW, NZERO_ROW, PZERO_ROW = 10, 11, 12, 13
_ID = dict(ids=lambda v: str(v).split(".")[-1])


@functools.lru_cache(maxsize=None)
def hop(targets=T, sources=S, seed=3):
    """(rowptr, col) on the CPU: the degrees cycle through DEGS; duplicate edges, self-references and rows that hold
    only the planted special rows (only -inf; -0.0 before +0.0; +0.0 before -0.0; a NaN before and after larger values)"""
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor([DEGS[t % len(DEGS)] for t in range(targets)])
    rowptr = torch.zeros(targets + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, sources, (int(rowptr[-1]),), generator=g)
    for t in range(targets):
        b, d = int(rowptr[t]), int(deg[t])
        if d >= 2 and t % 2 == 0:
            col[b + 1] = col[b]                          # a duplicate edge
        if d >= 3 and t < sources:
            col[b + 2] = t                               # a self-reference
    if targets >= 13 and sources > PZERO_ROW:
        col[int(rowptr[1])] = NINF_ROW                                           # deg 1: only -inf
        col[int(rowptr[2]):int(rowptr[2]) + 2] = torch.tensor([NZERO_ROW, PZERO_ROW])    # -0.0 then +0.0
        col[int(rowptr[3]):int(rowptr[3]) + 3] = torch.tensor([PZERO_ROW, NZERO_ROW, NZERO_ROW])
        col[int(rowptr[4]):int(rowptr[4]) + 3] = torch.tensor([20, NAN_ROW, 21])         # a NaN between other values
        col[int(rowptr[10]):int(rowptr[10]) + 1] = NINF_ROW                      # deg 1 again
        col[int(rowptr[12]) + 5] = NAN_ROW                                       # deg 3 ... 8: a NaN late in the row
    return rowptr, col


@functools.lru_cache(maxsize=None)
def values(F, rows=S, seed=1, special=True):
    """fp32 [rows, F] on the CPU: small integers in [-3, 3] (ties are frequent; exact in fp16, bf16 and e4m3), with the
    special rows planted"""
    x = torch.randint(-3, 4, (rows, F), generator=torch.Generator().manual_seed(seed + F)).float()
    if special:
        x[NAN_ROW, ::2] = float("nan")
        x[NINF_ROW] = float("-inf")
        x[NZERO_ROW] = -0.0
        x[PZERO_ROW] = 0.0
        x[20] = 3.0                                      # (a maximum in front of the NaN)
    return x


@functools.lru_cache(maxsize=None)
def expected(F, dtype=torch.float32):
    """(out, arg) of _max_reference on the CPU over the values as `dtype` holds them: the same numbers for every dtype,
    but a NaN's payload is whatever the conversion to fp16 / bf16 left, and the maximum carries it"""
    rowptr, col = hop()
    from salient_plusplus_amd.models import _max_reference
    return _max_reference(values(F).to(dtype), rowptr, col, T)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def same_rounded(a, b):
    """same() for a bf16 OUTPUT against torch's own rounding of the fp32 one: every bit, except that where both hold a
    NaN its payload is not compared (the hardware convert keeps the payload's top bits, torch's cast writes 0x7fc0)"""
    a, b = a.cpu(), b.cpu()
    return torch.equal(a.isnan(), b.isnan()) and same(a.nan_to_num(7.0), b.nan_to_num(7.0))


def run(x, concat=False, want_arg=True, out_dtype=torch.float32, graph=None):
    from salient_plusplus_amd.models import _agg_max_forward
    rowptr, col = graph or hop()
    return _agg_max_forward(rowptr.cuda(), col.cuda(), rowptr.numel() - 1, x, out_dtype, concat, want_arg)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("F", WIDTHS)
def test_forward_dense(F, dtype):
    want, want_arg = expected(F, dtype)
    assert same(want_arg, expected(F)[1]) and torch.equal(want.nan_to_num(7.0), expected(F)[0].nan_to_num(7.0))
    x = values(F).to(dtype).cuda()
    out, arg = run(x)
    assert same(out, want) and same(arg, want_arg)
    # the special rows came out as the contract says
    assert bool((out[0] == 0).all()) and bool((arg[0] == -1).all())              # an empty row
    assert bool((out[1] == float("-inf")).all()) and bool((arg[1] == NINF_ROW).all())
    assert bool((bits(out[2]) == bits(torch.tensor([-0.0]))[0].item()).all()) and bool((arg[2] == NZERO_ROW).all())
    assert bool((bits(out[3]) == 0).all()) and bool((arg[3] == PZERO_ROW).all())
    assert bool(out[4, ::2].isnan().all()) and bool((arg[4, ::2] == NAN_ROW).all()) and bool((arg[4, 1::2] == 20).all())
    # no argmax: the same output; a bf16 output: the fp32 one rounded once; the operand: [max | x_target]
    out2, none = run(x, want_arg=False)
    assert none is None and same(out2, out)
    ob, ab = run(x, out_dtype=torch.bfloat16)
    assert same_rounded(ob, out.to(torch.bfloat16)) and same(ab, arg)
    for odt in (torch.float32, torch.bfloat16):
        oc, ac = run(x, concat=True, out_dtype=odt)
        assert oc.shape == (T, 2 * F) and same(ac, arg)
        assert same_rounded(oc[:, :F], out.to(odt)) and same_rounded(oc[:, F:], x[:T].float().to(odt))
        if odt == torch.float32:
            assert same(oc[:, :F], out) and same(oc[:, F:], x[:T].float())


@pytest.mark.parametrize("F,dtype", [(6, torch.float16), (100, torch.float16), (128, torch.bfloat16), (260, torch.float32)])
def test_forward_table_rows_and_row_refs(F, dtype):
    """TableRows (an id outside the table reads row 0) and RowRefs give the result over the materialised rows"""
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from salient_plusplus_amd.models import _max_reference
    rowptr, col = hop()
    g = torch.Generator().manual_seed(9)
    table = values(F, rows=500, seed=4, special=False).clone()
    table[7] = float("nan")
    n_id = torch.randint(0, 500, (S,), generator=g)
    n_id[3], n_id[50], n_id[199], n_id[20] = -1, 500, 1 << 40, 7
    table = table.to(dtype)                                  # (what the kernel reads, a NaN's payload included)
    rows = table[torch.where((n_id >= 0) & (n_id < 500), n_id, 0)].float()
    want, want_arg = _max_reference(rows, rowptr, col, T)
    padded = torch.zeros((500, F + 12), dtype=dtype).cuda()                      # rows of a padded resident table
    padded[:, :F] = table
    for concat in (False, True):
        out, arg = run(TableRows(padded[:, :F], n_id.cuda()), concat=concat)
        assert same(out[:, :F], want) and same(arg, want_arg)
        if concat:
            assert same(out[:, F:], rows[:T])
    mat = rows.to(dtype).cuda()
    addr = mat.data_ptr() + torch.arange(S, dtype=torch.int64) * (F * mat.element_size())
    refs = RowRefs(addr.cuda(), None, F, dtype, None, (mat,))
    for concat in (False, True):
        out, arg = run(refs, concat=concat)
        assert same(out[:, :F], want) and same(arg, want_arg)
        if concat:
            assert same(out[:, F:], rows[:T])


@pytest.mark.parametrize("F", [16, 128])
def test_forward_fp8_table_equals_the_run_on_its_dequantised_copy(F):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import TableRows
    g = torch.Generator().manual_seed(2)
    x = (values(F, special=False) * torch.rand((1, F), generator=g) * 40).cuda()          # columns of different scales
    q = fp8.quantize_e4m3(x)
    v = q.dequantize(torch.float32)
    assert not torch.equal(v, x) or F == 0                    # (really quantised)
    n_id = torch.randint(0, S, (S,), generator=g).cuda()
    n_id[5] = S + 3                                           # reads row 0
    for concat in (False, True):
        for odt in (torch.float32, torch.bfloat16):
            out, arg = run(q, concat=concat, out_dtype=odt)
            want, want_arg = run(v, concat=concat, out_dtype=odt)
            assert same(out, want) and same(arg, want_arg)
            out, arg = run(TableRows(q, n_id), concat=concat, out_dtype=odt)
            want, want_arg = run(TableRows(v, n_id), concat=concat, out_dtype=odt)
            assert same(out, want) and same(arg, want_arg)


def _grad_expected(arg, g, F, sources, concat):
    """index_add of g at the kernel's own arg (+ the target half), on the CPU in fp32: integer values, exact sums"""
    arg, g = arg.cpu().long(), g.cpu().float()
    want = torch.zeros((sources, F))
    cols = torch.arange(F).expand_as(arg)
    on = arg >= 0
    want.index_put_((arg[on], cols[on]), g[:, :F][on], accumulate=True)
    if concat:
        want[:arg.size(0)] += g[:, F:]
    return want


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("concat", [False, True], ids=["max", "operand"])
@pytest.mark.parametrize("F", WIDTHS)
def test_backward(F, concat, amp):
    from salient_plusplus_amd.models import _MaxAggregate
    rowptr, col = hop()
    dt = torch.bfloat16 if amp else torch.float32
    x = values(F, special=False).to(dt).cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = _MaxAggregate.apply(x, rowptr.cuda(), col.cuda(), T, concat)
    assert out.dtype == dt and out.shape == (T, 2 * F if concat else F)
    g = torch.randint(-8, 9, tuple(out.shape), generator=torch.Generator().manual_seed(F)).to(dt).cuda()
    out.backward(g)
    _, arg = run(x.detach())
    want = _grad_expected(arg, g, F, S, concat)
    assert x.grad.dtype == dt and same(x.grad, want.to(dt))
    named = torch.zeros(S, dtype=torch.bool)
    named[arg.cpu().long()[arg.cpu() >= 0]] = True
    if concat:
        named[:T] = True
    assert bool((~named).any()) and bool((x.grad[(~named).cuda()] == 0).all())


def test_backward_of_fp16_rows_and_no_gradient_into_tables():
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import TableRows
    from salient_plusplus_amd.models import max_aggregate
    rowptr, col = hop()
    F = 16
    x = values(F, special=False).half().cuda().requires_grad_(True)
    out = max_aggregate(x, rowptr.cuda(), col.cuda(), T)
    g = torch.randint(-8, 9, (T, F), generator=torch.Generator().manual_seed(0)).float().cuda()
    out.backward(g)
    _, arg = run(x.detach())
    assert x.grad.dtype == torch.float16 and same(x.grad, _grad_expected(arg, g, F, S, False).half())
    table = values(F, special=False).cuda().requires_grad_(True)
    o = max_aggregate(TableRows(table, torch.arange(S).cuda()), rowptr.cuda(), col.cuda(), T)
    assert not o.requires_grad                               # as the mean: a table source has no input gradient
    assert not max_aggregate(fp8.quantize_e4m3(table.detach()), rowptr.cuda(), col.cuda(), T).requires_grad


def test_smallest_shapes():
    from salient_plusplus_amd.models import _MaxAggregate, max_aggregate
    one = (torch.tensor([0, 3]), torch.tensor([2, 0, 2]))
    x = torch.tensor([[1.0], [9.0], [4.0]]).cuda().requires_grad_(True)        # T = 1, F = 1
    out = max_aggregate(x, one[0].cuda(), one[1].cuda(), 1)
    assert out.tolist() == [[4.0]]
    out.backward(torch.tensor([[5.0]]).cuda())
    assert x.grad.tolist() == [[0.0], [0.0], [5.0]]
    x.grad = None
    oc = _MaxAggregate.apply(x, one[0].cuda(), one[1].cuda(), 1, True)
    assert oc.tolist() == [[4.0, 1.0]]
    oc.backward(torch.tensor([[5.0, -2.0]]).cuda())
    assert x.grad.tolist() == [[-2.0], [0.0], [5.0]]
    x.grad = None
    none = (torch.zeros(1, dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int64).cuda())     # T = 0
    for concat in (False, True):
        z = _MaxAggregate.apply(x, none[0], none[1], 0, concat)
        assert z.shape == (0, 2 if concat else 1)
        z.sum().backward()
        assert x.grad.tolist() == [[0.0], [0.0], [0.0]]
        x.grad = None
