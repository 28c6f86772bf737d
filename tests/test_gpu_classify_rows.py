"""-m gpu: inference.classify_rows (spp_classify_rows) against torch on the same logits.

pred must equal torch.argmax(z.float(), -1) on every row (ties, NaNs, infinities included).  nll is compared with
F.cross_entropy(z.double(), y, reduction="none") under the bound DESIGN.md 7 f3m derives from the fp32 arithmetic,

    |nll - ref| <= (C + 8) * 2^-24 * (1 + |z_y - m| + log C),

and a row's two results must be the same bits wherever the row stands in the call, however it is loaded, and from run to
run.  One set of logits and one reference per (C, dtype, magnitude), shared by every n, layout and addressing form."""
import ctypes
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# a lane group of one lane (C <= 4 fp32 / 8 bf16), rows that are no multiple of the 16-byte piece, exactly one round
# (64, 65: 16 / 17 pieces of fp32), one over 64 lanes' worth (fp32: 349 > 256), several rounds (1000)
CS = [1, 2, 3, 5, 40, 47, 64, 65, 172, 349, 1000]
NS = [0, 1, 63, 64, 65, 1000]
DTYPES = [torch.float32, torch.bfloat16]
NMAX = 1000
_ID = dict(ids=lambda v: str(v).split(".")[-1])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _bound(z, y):
    """(C + 8) * 2^-24 * (1 + |z_y - m| + log C) per row, from the logits as the kernel reads them"""
    zf = z.double()
    zy = zf.gather(1, y.view(-1, 1)).squeeze(1)
    Cn = z.size(1)
    return (Cn + 8) * 2.0 ** -24 * (1.0 + (zy - zf.max(1).values).abs() + math.log(Cn))


@functools.lru_cache(maxsize=None)
def _case(Cn, dtype, scale):
    """NMAX rows of logits of magnitude up to ``scale``, labels, and torch's results on them"""
    g = torch.Generator().manual_seed(Cn * 7 + (dtype == torch.bfloat16))
    z = ((torch.rand((NMAX, Cn), generator=g) * 2 - 1) * scale).to(dtype).cuda()
    y = torch.randint(0, Cn, (NMAX,), generator=g).cuda()
    pred = torch.argmax(z.float(), -1)
    nll = F.cross_entropy(z.double(), y, reduction="none")
    return z, y, pred, nll, _bound(z, y)


def _layouts(z):
    """contiguous, a strided view (the rows start 3 elements into rows of another width: for most C one element per
    load) and a padded stride (a multiple of 8 elements: the widest loads C itself admits)"""
    n, Cn = z.shape
    view = torch.zeros((n, Cn + 7), dtype=z.dtype, device=z.device)[:, 3:3 + Cn]
    view.copy_(z)
    padded = torch.zeros((n, (Cn + 7) // 8 * 8 + 8), dtype=z.dtype, device=z.device)[:, :Cn]
    padded.copy_(z)
    return dict(contiguous=z.contiguous(), view=view, padded=padded)


def _check_nll(nll, ref, bound, what):
    err = (nll.double() - ref).abs()
    worst = (err / bound).max().item() if err.numel() else 0.0
    print(f"{what}: max |nll - ref| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("Cn", CS)
def test_random_logits_every_n_layout_and_addressing(Cn, dtype):
    from salient_plusplus_amd.inference import classify_rows
    for scale in (50.0, 1e-3):
        z, y, pred_ref, nll_ref, bound = _case(Cn, dtype, scale)
        g = torch.Generator().manual_seed(3)
        table = torch.randint(0, Cn, (1500,), generator=g).cuda()            # labels addressed by a list
        ids = torch.randint(0, 1500, (NMAX,), generator=g).cuda()            # shuffled, with duplicates
        ids[1::7] = ids[0::7][:ids[1::7].numel()]
        nll_ids_ref = F.cross_entropy(z.double(), table[ids], reduction="none")
        bound_ids = _bound(z, table[ids])
        for n in NS:
            for name, zl in _layouts(z[:n]).items():
                what = f"C={Cn} {dtype} scale={scale} n={n} {name}"
                pred, nll = classify_rows(zl, y, row0=0)
                assert pred.dtype == torch.int64 and nll.dtype == torch.float32 and pred.shape == nll.shape == (n,)
                assert torch.equal(pred, pred_ref[:n]), what
                _check_nll(nll, nll_ref[:n], bound[:n], what)
                pred2, nll2 = classify_rows(zl, table, row_ids=ids[:n].contiguous())
                assert torch.equal(pred2, pred_ref[:n]), what
                _check_nll(nll2, nll_ids_ref[:n], bound_ids[:n], what + " row_ids")
                only, none = classify_rows(zl)                               # pred only
                assert none is None and torch.equal(only, pred_ref[:n]), what
                if n:                                                       # nll only: the entry itself
                    assert torch.equal(_bits(_nll_only(zl, y)), _bits(nll)), what
                # caller-provided outputs, slices of longer vectors; a slab that starts inside y
                P, L = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda"), torch.full((n + 2,), -7.0, device="cuda")
                y_off = torch.cat([y.new_zeros(5), y])
                got = classify_rows(zl, y_off, row0=5, pred=P[1:n + 1], nll=L[1:n + 1])
                assert got[0].shape == got[1].shape == (n,)
                if n:                                                       # (an empty slice has no address)
                    assert got[0].data_ptr() == P[1:].data_ptr() and got[1].data_ptr() == L[1:].data_ptr()
                assert torch.equal(P[1:n + 1], pred) and torch.equal(_bits(L[1:n + 1]), _bits(nll)), what
                assert P[0] == -7 and P[n + 1] == -7 and L[0] == -7 and L[n + 1] == -7, what


def _nll_only(z, y):
    """spp_classify_rows with pred_dev NULL (the Python wrapper always returns pred)"""
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.models import _ELEM, _stream
    n, Cn = z.shape
    nll = torch.empty(n, dtype=torch.float32, device=z.device)
    d = nat.ClassifyDesc(z_elem=_ELEM[z.dtype], z_dev=z.data_ptr(), z_stride_elems=z.stride(0) if n > 1 else Cn, n=n,
                         C=Cn, y_dev=y.data_ptr(), y_rows=y.numel(), y_row0=0, row_ids_dev=None, pred_dev=None,
                         nll_dev=nll.data_ptr())
    nat.check(nat.load().spp_classify_rows(ctypes.byref(d), _stream()))
    return nll


def _tie_rows(Cn, dtype):
    """rows whose maximum (64.0, above every other logit) stands at two to four positions: neighbours inside one piece,
    the two sides of a piece boundary, one lane's pieces of different rounds, the row's ends, and random sets"""
    g = torch.Generator().manual_seed(Cn)
    W = 4 if dtype == torch.float32 else 8
    sets = [[0, Cn - 1], [Cn - 2, Cn - 1], [0, 1], [W - 1, W], [1, W + 1, 2 * W + 1], [0, 64 * W], [5, 64 * W + 5, 128 * W + 5],
            [W, 16 * W, 32 * W, 48 * W], [Cn // 2, Cn // 2 + 1, Cn - 1], [3, 64 * W - 1, 64 * W]]
    sets = [sorted({p for p in s if 0 <= p < Cn}) for s in sets]
    for k in (2, 3, 4) * 20:
        sets.append(sorted(set(torch.randint(0, Cn, (k,), generator=g).tolist())))
    sets = [s for s in sets if len(s) >= 2]
    z = (torch.rand((len(sets), Cn), generator=g) * 100 - 50).to(dtype)
    for r, s in enumerate(sets):
        z[r, s] = 64.0
    return z.cuda(), torch.tensor([s[0] for s in sets]).cuda()


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("Cn", [c for c in CS if c > 1])
def test_ties_take_the_smallest_index(Cn, dtype):
    from salient_plusplus_amd.inference import classify_rows
    z, first = _tie_rows(Cn, dtype)
    assert torch.equal(torch.argmax(z.float(), -1), first)
    for name, zl in _layouts(z).items():
        assert torch.equal(classify_rows(zl)[0], first), (Cn, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("Cn", CS)
def test_nan_inf_and_equal_rows_follow_torch(Cn, dtype):
    from salient_plusplus_amd.inference import classify_rows
    g = torch.Generator().manual_seed(100 + Cn)
    inf, nan = float("inf"), float("nan")
    rows = []
    for fill in (0.0, -0.0, 1.5, -inf, inf, nan):                            # all-equal rows: index 0
        rows.append(torch.full((Cn,), fill))
    zero = torch.zeros(Cn)
    zero[::2] = -0.0                                                         # -0.0 == 0.0: still index 0
    rows.append(zero)
    for special, k in [(nan, 1), (nan, 3), (inf, 1), (inf, 3), (-inf, 2)]:
        for _ in range(12):
            r = torch.rand(Cn, generator=g) * 100 - 50
            r[torch.randint(0, Cn, (k,), generator=g)] = special
            rows.append(r)
    for _ in range(12):                                                      # an inf BEFORE a NaN: the NaN wins
        r = torch.rand(Cn, generator=g) * 100 - 50
        pos = torch.randint(0, Cn, (4,), generator=g)
        r[pos[:2]], r[pos[2:]] = inf, nan
        rows.append(r)
    z = torch.stack(rows).to(dtype).cuda()
    want = torch.argmax(z.float(), -1)
    nanrow = torch.isnan(z.float()).any(1)
    firstnan = torch.isnan(z.float()).int().argmax(1)
    assert torch.equal(want[nanrow], firstnan[nanrow])                       # (what the contract says torch does)
    for name, zl in _layouts(z).items():
        assert torch.equal(classify_rows(zl)[0], want), (Cn, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("Cn", [1, 5, 47, 172, 349])
def test_rows_without_a_label_give_exactly_zero_and_leave_their_neighbours(Cn, dtype):
    from salient_plusplus_amd.inference import classify_rows
    z, y, pred_ref, _nll_ref, _b = _case(Cn, dtype, 50.0)
    n = 333
    z = z[:n]
    _pred, full = classify_rows(z, y, row0=0)
    bad = torch.arange(n, device="cuda") % 5 == 2
    for none in (-1, Cn, Cn + 12345, -(1 << 40)):                            # labels outside [0, C)
        yb = y.clone()
        yb[:n][bad] = none
        pred, nll = classify_rows(z, yb, row0=0)
        assert torch.equal(pred, pred_ref[:n])
        assert torch.equal(_bits(nll[bad]), torch.zeros_like(nll[bad]).view(torch.int32))
        assert torch.equal(_bits(nll[~bad]), _bits(full[~bad]))
    for none in (-1, NMAX, NMAX + 7, 1 << 40):                               # row ids outside [0, y_rows)
        ids = torch.arange(n, device="cuda")
        ids[bad] = none
        pred, nll = classify_rows(z, y, row_ids=ids)
        assert torch.equal(pred, pred_ref[:n])
        assert torch.equal(_bits(nll[bad]), torch.zeros_like(nll[bad]).view(torch.int32))
        assert torch.equal(_bits(nll[~bad]), _bits(full[~bad]))
    # a slab that runs past the end of y: the rows beyond it have no label
    pred, nll = classify_rows(z, y[:100].contiguous(), row0=0)
    assert bool((nll[100:] == 0).all()) and torch.equal(_bits(nll[:100]), _bits(full[:100]))


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("Cn", CS)
def test_a_row_gives_the_same_bits_wherever_it_stands(Cn, dtype):
    """257 rows alone, embedded at offset 1 and at offset 64 of a larger call, through the strided view, in reversed
    order, and a second time: pred and nll bit for bit"""
    from salient_plusplus_amd.inference import classify_rows
    zs, ys, _p, _n, _b = _case(Cn, dtype, 50.0)
    n = 257
    z, y = zs[:n].contiguous(), ys[:n].contiguous()
    pred, nll = classify_rows(z, y, row0=0)
    again = classify_rows(z, y, row0=0)
    assert torch.equal(again[0], pred) and torch.equal(_bits(again[1]), _bits(nll))
    for off in (1, 64):
        big = torch.cat([zs[500:500 + off], z, zs[900:905]]).contiguous()
        ids = torch.cat([torch.full((off,), -1), torch.arange(n), torch.full((5,), -1)]).cuda()
        p2, l2 = classify_rows(big, y, row_ids=ids)
        assert torch.equal(p2[off:off + n], pred) and torch.equal(_bits(l2[off:off + n]), _bits(nll)), (Cn, dtype, off)
    for name, zl in _layouts(z).items():
        p2, l2 = classify_rows(zl, y, row0=0)
        assert torch.equal(p2, pred) and torch.equal(_bits(l2), _bits(nll)), (Cn, dtype, name)
    p2, l2 = classify_rows(z.flip(0).contiguous(), y.flip(0).contiguous(), row0=0)
    assert torch.equal(p2.flip(0), pred) and torch.equal(_bits(l2.flip(0).contiguous()), _bits(nll)), (Cn, dtype, "reversed")
    p2, l2 = classify_rows(z.flip(0).contiguous(), y, row_ids=torch.arange(n - 1, -1, -1).cuda())
    assert torch.equal(p2.flip(0), pred) and torch.equal(_bits(l2.flip(0).contiguous()), _bits(nll)), (Cn, dtype, "list")
