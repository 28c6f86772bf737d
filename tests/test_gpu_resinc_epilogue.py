"""spp_resinc_epilogue through inference.resinc_epilogue against its arithmetic contract restated in float64 on the same
inputs (include/spp.h, f3i):

    y = a * z + b;   y = y >= 0 ? y : slope * y;   out = y + r[row(i)]        (a row index outside r: a row of zeros)

Bound per element.  The kernel rounds three or four times in fp32: once in the fma a * z + b, once in slope * y, once in
y + r (the fourth unit of the bound covers an fma result whose sign differs from the exact one's, which then takes the
other branch of the slope).  Every rounding is relative 2^-24 of a quantity no larger than |a z| + |b| + |r|, so

    fp32 output:  |got - want| <= 4 * 2^-24 * (|a z| + |b| + |r|)
    bf16 output:  that bound plus one bf16 rounding of the computed value, 2^-8 * (|want| + that bound)

n in {0, 1, 63, 257} x C in {1, 5, 16, 43, 256} (the scalar and the vector form at W = 4 and W = 8, tail lanes, tiles
that end inside a workgroup), dense / padded / odd row strides, slab and list addressing, both slopes."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

NS, CS = (0, 1, 63, 257), (1, 5, 16, 43, 256)
Z_DTYPES = (torch.float32, torch.bfloat16)
R_DTYPES = (torch.float32, torch.float16, torch.bfloat16, None)
OUT_DTYPES = (torch.float32, torch.bfloat16)
SENTINEL = -77.0


def _name(d):
    return "none" if d is None else str(d).split(".")[-1]


def _matrix(rows, C, stride, dtype, g):
    """[rows, C] as a view of a [rows, stride] allocation"""
    full = torch.randn((rows, stride), generator=g).to(dtype).cuda()
    return full, full[:, :C]


def _reference(z, a, b, slope, r, rows):
    """(want, bound32), float64: the contract on the same inputs; ``rows`` int64 [n] or None"""
    slope = float(torch.tensor(slope, dtype=torch.float32))            # the entry takes the slope as an fp32 value
    az = a.double() * z.double()
    y = az + b.double()
    y = torch.where(y >= 0, y, slope * y)
    mag = az.abs() + b.double().abs()
    if r is not None:
        inside = (rows >= 0) & (rows < r.size(0))
        rr = r.double()[rows.clamp(0, r.size(0) - 1)]
        y = torch.where(inside[:, None], y + rr, torch.zeros_like(y))
        mag = mag + rr.abs()
    return y, 4 * 2.0 ** -24 * mag


def _check(got, want, bound32, what):
    tol = bound32 if got.dtype == torch.float32 else bound32 + 2.0 ** -8 * (want.abs() + bound32)
    err = (got.double() - want).abs()
    assert bool(torch.isfinite(got).all()), what
    over = err > tol
    assert not bool(over.any()), (what, float(err[over].max()), float(tol[over].min()))
    return float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=_name)
@pytest.mark.parametrize("r_dtype", R_DTYPES, ids=_name)
@pytest.mark.parametrize("z_dtype", Z_DTYPES, ids=_name)
def test_epilogue_matches_the_contract_in_float64(z_dtype, r_dtype, out_dtype):
    from salient_plusplus_amd.inference import resinc_epilogue
    g = torch.Generator().manual_seed(31)
    worst, launches = 0.0, 0
    addressing = ("slab3", "slab8", "list") if r_dtype is not None else ("none",)
    slopes = itertools.cycle((0.01, 0.2))
    for n, C, strides, addr in itertools.product(NS, CS, ("dense", "padded", "odd"), addressing):
        stride = {"dense": C, "padded": C + 8, "odd": C + 3}[strides]
        slope = next(slopes)
        what = f"n={n} C={C} {strides} {addr} slope={slope} z={_name(z_dtype)} r={_name(r_dtype)} out={_name(out_dtype)}"
        _zf, z = _matrix(n, C, stride, z_dtype, g)
        a = (torch.rand(C, generator=g) + 0.5).cuda() * (torch.randint(0, 2, (C,), generator=g).cuda() * 2 - 1)
        b = (torch.randn(C, generator=g) * 0.5).cuda()
        out_full = torch.full((n + 4, stride), SENTINEL, dtype=out_dtype).cuda()
        out = out_full[2:2 + n, :C]                                    # a slab of a larger matrix
        kw, r, rows = {}, None, None
        if r_dtype is not None:
            R = n + 5
            _rf, r = _matrix(R, C, stride, r_dtype, g)
            if addr == "list":
                rows = torch.randint(0, R, (n,), generator=g)          # unsorted, with duplicates
                if n >= 4:
                    rows[1], rows[2], rows[3] = -1, R, rows[0]
                if n >= 63:
                    rows[n - 1], rows[n - 2] = -(1 << 40), 1 << 40
                rows = rows.cuda()
                kw = dict(residual=r, row_ids=rows)
            else:
                row0 = int(addr[4:])                                   # slab8: the last rows leave the residual
                rows = torch.arange(row0, row0 + n).cuda()
                kw = dict(residual=r, row0=row0)
        ret = resinc_epilogue(z, a, b, negative_slope=slope, out=out, **kw)
        launches += 1
        assert ret is out
        want, bound32 = _reference(z, a, b, slope, r, rows)
        worst = max(worst, _check(out, want, bound32, what))
        if r is not None and n:
            outside = (rows < 0) | (rows >= r.size(0))
            assert bool((out[outside] == 0).all()), what              # zero rows, exactly
            assert addr == "slab3" or n < 4 or bool(outside.any()), what
        # the rows around the slab and the padding behind its columns are untouched
        assert bool((out_full[:2] == SENTINEL).all()) and bool((out_full[2 + n:] == SENTINEL).all()), what
        assert bool((out_full[:, C:] == SENTINEL).all()), what
    print(f"z={_name(z_dtype)} r={_name(r_dtype)} out={_name(out_dtype)}: {launches} calls, worst error "
          f"{worst:.3f} of the bound")
    assert worst <= 1.0


def test_allocated_output_and_dtypes():
    """without ``out`` the result is a fresh dense matrix of ``out_dtype`` (fp32 by default), equal to the in-place form"""
    from salient_plusplus_amd.inference import resinc_epilogue
    g = torch.Generator().manual_seed(3)
    z = torch.randn((70, 24), generator=g).cuda()
    a, b = torch.rand(24, generator=g).cuda() + 0.5, torch.randn(24, generator=g).cuda()
    r = torch.randn((90, 24), generator=g).to(torch.float16).cuda()
    for dt in (None, torch.float32, torch.bfloat16):
        got = resinc_epilogue(z, a, b, negative_slope=0.2, residual=r, row0=20, out_dtype=dt)
        assert got.dtype == (dt or torch.float32) and got.shape == (70, 24) and got.is_contiguous()
        into = torch.empty_like(got)
        resinc_epilogue(z, a, b, negative_slope=0.2, residual=r, row0=20, out=into)
        assert torch.equal(got, into)
        assert not got.requires_grad
    empty = resinc_epilogue(z[:0], a, b, negative_slope=0.2, residual=r, row0=0, out_dtype=torch.bfloat16)
    assert empty.shape == (0, 24) and empty.dtype == torch.bfloat16


def test_bf16_output_is_the_fp32_output_rounded_once():
    from salient_plusplus_amd.inference import resinc_epilogue
    g = torch.Generator().manual_seed(4)
    for C in (43, 256):
        z = torch.randn((257, C), generator=g).cuda()
        a, b = torch.rand(C, generator=g).cuda() + 0.5, torch.randn(C, generator=g).cuda()
        r = torch.randn((300, C), generator=g).to(torch.bfloat16).cuda()
        ids = torch.randint(0, 300, (257,), generator=g).cuda()
        f32 = resinc_epilogue(z, a, b, negative_slope=0.01, residual=r, row_ids=ids)
        b16 = resinc_epilogue(z, a, b, negative_slope=0.01, residual=r, row_ids=ids, out_dtype=torch.bfloat16)
        assert torch.equal(b16, f32.to(torch.bfloat16))
        # and the same rows by slab as by the list that names them
        slab = resinc_epilogue(z, a, b, negative_slope=0.01, residual=r, row0=17)
        listed = resinc_epilogue(z, a, b, negative_slope=0.01, residual=r, row_ids=torch.arange(17, 17 + 257).cuda())
        assert torch.equal(slab, listed)


def test_offsets_are_64_bit():
    """a bf16 residual of [2^23 + 8, 256] (4.3 GB) addressed at its last 8 rows: element offsets from 2^31 on"""
    from salient_plusplus_amd.inference import resinc_epilogue
    R, C, n = (1 << 23) + 8, 256, 8
    g = torch.Generator().manual_seed(9)
    r = torch.empty((R, C), dtype=torch.bfloat16, device="cuda")
    tail = torch.randn((n, C), generator=g).to(torch.bfloat16).cuda()
    r[:n] = 0
    r[R - n:] = tail
    z = torch.randn((n, C), generator=g).cuda()
    a, b = torch.rand(C, generator=g).cuda() + 0.5, torch.randn(C, generator=g).cuda()
    order = torch.tensor([5, 0, 7, 7, 2, 1, 6, 3])
    for kw, rows in ((dict(row0=R - n), torch.arange(n)), (dict(row_ids=(R - n + order).cuda()), order)):
        for out_dtype in OUT_DTYPES:
            got = resinc_epilogue(z, a, b, negative_slope=0.01, residual=r, out_dtype=out_dtype, **kw)
            want, bound32 = _reference(z, a, b, 0.01, tail, rows.cuda())
            frac = _check(got, want, bound32, f"64-bit {list(kw)} {_name(out_dtype)}")
            print(f"64-bit offsets, {list(kw)[0]}, out {_name(out_dtype)}: worst error {frac:.3f} of the bound")
    del r
