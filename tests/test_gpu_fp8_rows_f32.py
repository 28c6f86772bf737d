"""spp_fp8_rows_f32 (csrc/gather_fp8.hip, f3o): rows of an fp8 table as dense fp32, exactly
``Fp8Features.dequantize(torch.float32)`` computed on the CPU -- as a slab and by an id list, for empty, tiny, odd and
multi-workgroup row counts, every non-NaN code and exponents from -64 to 63; an id outside the table reads row 0 and
raises the gather's asynchronous error; a refusal is a status and leaves the destination alone."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FS = [16, 48, 128, 272]
NS = [0, 1, 63, 1000]
ROWS = 1100
EXPONENTS = [-64, 0, 9, 63, -7, 20, -33, 1]
SPP_AERR_GATHER_INDEX = 1


@functools.lru_cache(maxsize=None)
def _table(F_):
    """(the table on the GPU, its fp32 dequantisation on the CPU): all 254 non-NaN codes, exponents cycling"""
    from salient_plusplus_amd.fp8 import Fp8Features
    g = torch.Generator().manual_seed(900 + F_)
    valid = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    codes = valid[torch.randint(0, 254, (ROWS, F_), generator=g)]
    codes.view(-1)[:254] = valid
    e = torch.tensor([EXPONENTS[c % len(EXPONENTS)] for c in range(F_)], dtype=torch.int8)
    x8 = Fp8Features(codes.view(torch.float8_e4m3fn), e)
    return x8.to("cuda"), x8.dequantize(torch.float32)


def _rows(x8, n, row0=-1, ids=None, dst=None):
    from salient_plusplus_amd import _native as nat
    dst = torch.full((n, x8.size(1)), -3.5, device="cuda") if dst is None else dst
    rc = nat.load().spp_fp8_rows_f32(x8.q.data_ptr(), x8.size(0), x8.size(1), x8.scale_log2.data_ptr(), row0,
                                     ids.data_ptr() if ids is not None else None, n, dst.data_ptr() if n else None, None)
    return rc, dst


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("F_", FS)
def test_slab_and_list_equal_the_cpu_dequantisation(F_, n):
    from salient_plusplus_amd import _native as nat
    x8, v = _table(F_)
    L = nat.load()
    L.spp_async_errors(0, 1)
    for row0 in (0, ROWS - n, 37 if n <= 63 else 100):
        rc, got = _rows(x8, n, row0=row0)
        assert rc == 0, L.spp_last_error()
        assert _same_bits(got.cpu(), v[row0:row0 + n]), (F_, n, row0)
    ids = torch.randint(0, ROWS, (n,), generator=torch.Generator().manual_seed(n))
    if n > 2:
        ids[1] = ids[0]                                        # duplicates, any order
        ids[2] = ROWS - 1
    dev_ids = ids.cuda() if n else torch.zeros(1, dtype=torch.int64, device="cuda")   # (an empty tensor has no address)
    rc, got = _rows(x8, n, ids=dev_ids)
    assert rc == 0, L.spp_last_error()
    assert _same_bits(got.cpu(), v[ids]), (F_, n)
    torch.cuda.synchronize()
    assert L.spp_async_errors(0, 1) == 0


@pytest.mark.parametrize("F_", [16, 272])
def test_an_id_outside_the_table_reads_row_0_and_is_reported(F_):
    from salient_plusplus_amd import _native as nat
    x8, v = _table(F_)
    L = nat.load()
    L.spp_async_errors(0, 1)
    ids = torch.tensor([5, -1, ROWS, 7, 1 << 40, ROWS - 1], dtype=torch.int64)
    rc, got = _rows(x8, ids.numel(), ids=ids.cuda())
    assert rc == 0, L.spp_last_error()
    inside = (ids >= 0) & (ids < ROWS)
    assert _same_bits(got.cpu(), v[torch.where(inside, ids, torch.zeros_like(ids))])
    torch.cuda.synchronize()
    assert L.spp_async_errors(0, 1) & SPP_AERR_GATHER_INDEX
    assert L.spp_async_errors(0, 1) == 0


def test_refusals_are_a_status_and_leave_the_destination_untouched():
    from salient_plusplus_amd import _native as nat
    x8, _v = _table(16)
    L = nat.load()
    dst = torch.full((8, 16), -3.5, device="cuda")
    q, sc, ids = x8.q.data_ptr(), x8.scale_log2.data_ptr(), torch.zeros(8, dtype=torch.int64, device="cuda").data_ptr()
    # (q, src_rows, F, scale, row0, ids, n, dst), the word of the refusal
    cases = [((q, ROWS, 24, sc, 0, None, 8, dst.data_ptr()), b"multiple of 16"),
             ((q, ROWS, 16, sc, 0, ids, 8, dst.data_ptr()), b"not both"),
             ((q, ROWS, 16, sc, -1, None, 8, dst.data_ptr()), b"one of them"),
             ((q, ROWS, 16, sc, ROWS - 7, None, 8, dst.data_ptr()), b"leaves the table"),
             ((q, ROWS, 16, sc, 0, None, -1, dst.data_ptr()), b"negative size"),
             ((None, ROWS, 16, sc, 0, None, 8, dst.data_ptr()), b"NULL buffer"),
             ((q, ROWS, 16, None, 0, None, 8, dst.data_ptr()), b"NULL buffer"),
             ((q, ROWS, 16, sc, 0, None, 8, None), b"NULL buffer"),
             ((q, 0, 16, sc, -1, ids, 8, dst.data_ptr()), b"empty table"),
             ((q + 4, ROWS, 16, sc, 0, None, 8, dst.data_ptr()), b"aligned"),
             ((q, ROWS, 16, sc + 2, 0, None, 8, dst.data_ptr()), b"aligned"),
             ((q, ROWS, 16, sc, 0, None, 8, dst.data_ptr() + 4), b"aligned")]
    for args, word in cases:
        assert L.spp_fp8_rows_f32(*args, None) == -1, word
        msg = L.spp_last_error()
        assert msg.startswith(b"spp_fp8_rows_f32:") and word in msg, msg
    torch.cuda.synchronize()
    assert bool((dst == -3.5).all())
