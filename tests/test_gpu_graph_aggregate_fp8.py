"""spp_graph_agg_forward_fp8 / spp_graph_agg_parts_forward_fp8 (csrc/graph_aggregate.hip, f3o) through
inference.graph_aggregate and graph_aggregate_parts over an ``Fp8Table``: the contract of include/spp.h pinned bit for bit
-- the fp8 entry returns the bits of the existing entry over the same table dequantised to fp32 on the CPU, for every
epilogue, output type and target form, with ids outside the graph, for every non-NaN e4m3 code and exponents from -64 to
63; the parts entry returns the bits of the resident one; the slab size changes nothing; a refusal is a status and leaves
the output alone."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FS = [16, 48, 128, 272]            # 272 = 17 pieces of 16: 68 dwords a row, more than a wavefront -> the second column pass
OUT_DTYPES = [torch.float32, torch.bfloat16]
EPILOGUES = [("mean", 0.0), ("operand", 0.0), ("sum", 1.5)]
EXPONENTS = [-64, 0, 9, 63, -7, 20, -33, 1]
N = 300
HUB = 200


def _chunk():
    from salient_plusplus_amd.inference import graph_agg_chunk
    return graph_agg_chunk()


@functools.lru_cache(maxsize=None)
def _graph():
    """300 nodes with the degrees 0, 1, 3, 4, 5, 64, 65, 129 and one row of 64 * 64 + 1 entries (at F = 16, four lanes a
    row, the long kernel's 64 lane groups need two rounds for its 65 chunks); ordinary rows of 2..12 entries; a few col
    entries outside the graph (they read row 0)"""
    assert _chunk() == 64                                      # the degrees below are written for C = 64
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(2, 13, (N,), generator=g)
    for k, v in {0: 0, 3: 1, 7: 3, 8: 4, 9: 5, 20: 64, 21: 65, 50: 129, HUB: 64 * 64 + 1, N - 1: 65}.items():
        deg[k] = v
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    for t, v in ((7, N), (21, -1), (50, N + 1000), (HUB, 1 << 40), (33, -(1 << 35))):
        col[rowptr[t] + 1] = v
    return rowptr, col


@functools.lru_cache(maxsize=None)
def _dev_graph():
    rowptr, col = _graph()
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _table(F_):
    """(Fp8Features on the CPU, its fp32 dequantisation on the GPU): codes drawn over all 254 non-NaN e4m3 codes -- both
    zeros, the subnormals, +-448 -- and every one of them present; exponents per column cycling through EXPONENTS"""
    from salient_plusplus_amd.fp8 import Fp8Features
    g = torch.Generator().manual_seed(500 + F_)
    valid = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    assert valid.numel() == 254
    codes = valid[torch.randint(0, 254, (N, F_), generator=g)]
    codes.view(-1)[:254] = valid                               # every code at least once (rows 0.. of the table)
    codes[HUB - 1].view(-1)[:16] = valid[torch.tensor([0, 127, 1, 128, 126, 253, 7, 8] * 2)]   # +-0, subnormals, +-448
    e = torch.tensor([EXPONENTS[c % len(EXPONENTS)] for c in range(F_)], dtype=torch.int8)
    x8 = Fp8Features(codes.view(torch.float8_e4m3fn), e)
    v = x8.dequantize(torch.float32)                            # on the CPU: the reference's input
    assert bool(torch.isfinite(v).all())
    return x8, v.cuda()


@functools.lru_cache(maxsize=None)
def _dev_table(F_):
    from salient_plusplus_amd.inference import Fp8Table
    return Fp8Table(_table(F_)[0].to("cuda"))


def _targets():
    ids = torch.tensor([HUB, 0, 3, 7, 8, 9, 20, 21, 50, N - 1, -1, N, HUB, 1 << 33, 33, 21], dtype=torch.int64)
    return [dict(row0=0, num_targets=N), dict(row0=19, num_targets=33), dict(target_ids=ids.cuda())]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(got, want) and torch.equal(_bits(got), _bits(want)), what


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("F_", FS)
def test_fp8_entry_returns_the_bits_of_the_fp32_dequantisation(F_, out_dtype):
    from salient_plusplus_amd.inference import graph_aggregate
    rowptr, col = _dev_graph()
    x8, v = _dev_table(F_), _table(F_)[1]
    for epilogue, scale in EPILOGUES:
        for tgt in _targets():
            kw = dict(epilogue=epilogue, self_scale=scale, out_dtype=out_dtype, **tgt)
            got, want = graph_aggregate(x8, rowptr, col, **kw), graph_aggregate(v, rowptr, col, **kw)
            _assert_same_bits(got, want, (F_, out_dtype, epilogue, sorted(tgt)))
            assert bool(torch.isfinite(want.float()).all())
    ids = _targets()[2]["target_ids"]
    outside = ((ids < 0) | (ids >= N)).nonzero().flatten()
    assert outside.numel() == 3 and not bool(got[outside].float().abs().sum())       # a target outside: a row of zeros


@pytest.mark.parametrize("n_parts", [1, 3, 16])
@pytest.mark.parametrize("F_", FS)
def test_parts_entry_returns_the_bits_of_the_resident_entry(F_, n_parts):
    from salient_plusplus_amd.inference import Fp8Table, graph_aggregate, graph_aggregate_parts
    rowptr, col = _dev_graph()
    x8 = _table(F_)[0]
    cuts = {1: [0, N], 3: [0, 120, 120, N], 16: [0, 1, 2, 40, 40] + [60 + 20 * k for k in range(11)] + [N]}[n_parts]
    assert len(cuts) == n_parts + 1 and (n_parts == 1 or any(a == b for a, b in zip(cuts, cuts[1:])))     # one part is empty
    parts = [Fp8Table(x8.rows(slice(a, b)).to("cuda")) if b > a or a == 40 else None for a, b in zip(cuts, cuts[1:])]
    for out_dtype in OUT_DTYPES:
        for epilogue, scale in EPILOGUES:
            for tgt in _targets():
                kw = dict(epilogue=epilogue, self_scale=scale, out_dtype=out_dtype, **tgt)
                got = graph_aggregate_parts(parts, cuts, rowptr, col, **kw)
                _assert_same_bits(got, graph_aggregate(_dev_table(F_), rowptr, col, **kw), (F_, n_parts, epilogue, sorted(tgt)))


@pytest.mark.parametrize("F_", [16, 272])
def test_result_does_not_depend_on_the_slab_size(F_):
    from salient_plusplus_amd.inference import graph_aggregate
    rowptr, col = _dev_graph()
    x8 = _dev_table(F_)
    for epilogue, scale in EPILOGUES:
        whole = graph_aggregate(x8, rowptr, col, row0=0, num_targets=N, epilogue=epilogue, self_scale=scale)
        slabs = [graph_aggregate(x8, rowptr, col, row0=s, num_targets=min(7, N - s), epilogue=epilogue, self_scale=scale)
                 for s in range(0, N, 7)]
        _assert_same_bits(torch.cat(slabs), whole, (F_, epilogue))


def _desc(nat, parts, x8, out, **over):
    rowptr, col = _dev_graph()
    F_ = x8.size(1)
    kw = dict(epilogue=nat.SPP_AGG_MEAN, x_elem=nat.SPP_ELEM_FP8_E4M3, out_elem=nat.SPP_ELEM_F32, rowptr_dev=rowptr.data_ptr(),
              col_dev=col.data_ptr(), x_stride_elems=F_, F=F_, target_row0=0, target_ids_dev=None, num_targets=N,
              out_dev=out.data_ptr(), out_stride_elems=0)
    kw.update(dict(num_parts=1) if parts else dict(x_dev=x8.q.data_ptr(), x_rows=N))
    kw.update(over)
    d = (nat.GraphAggPartsDesc if parts else nat.GraphAggDesc)(**kw)
    if parts:
        d.part_offsets[0], d.part_offsets[1], d.x_parts_dev[0] = 0, N, x8.q.data_ptr()
    return d


@pytest.mark.parametrize("entry", ["spp_graph_agg_forward_fp8", "spp_graph_agg_parts_forward_fp8"])
def test_refusals_are_a_status_and_leave_the_output_untouched(entry):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    x8 = _dev_table(16)
    out = torch.full((N, 16), 7.25, device="cuda")
    ws = torch.empty(16 + 8 * N, dtype=torch.uint8, device="cuda")
    scale = x8.scale_log2.data_ptr()
    cases = [("another x_elem", dict(x_elem=nat.SPP_ELEM_F32), scale, b"x_elem 0"),
             ("fp16 as x_elem", dict(x_elem=nat.SPP_ELEM_F16), scale, b"x_elem 1"),
             ("NULL exponents", {}, None, b"scale_log2_dev"),
             ("misaligned exponents", {}, scale + 1, b"scale_log2_dev"),
             ("F no multiple of 16", dict(F=8), scale, b"multiple of 16"),
             ("fp8 as out_elem", dict(out_elem=nat.SPP_ELEM_FP8_E4M3), scale, b"out_elem 3"),
             ("a row stride that is no multiple of 4 bytes", dict(x_stride_elems=18), scale, b"multiple of 4")]
    for what, over, sc, word in cases:
        d = _desc(nat, "parts" in entry, x8, out, **over)
        rc = getattr(L, entry)(C.byref(d), C.c_void_p(sc), C.c_void_p(ws.data_ptr()), ws.numel(), None)
        assert rc == -1, what
        msg = L.spp_last_error()
        assert msg.startswith(entry.encode() + b":") and word in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    d = _desc(nat, "parts" in entry, x8, out)                  # and the descriptor the cases were made from is accepted
    assert getattr(L, entry)(C.byref(d), C.c_void_p(scale), C.c_void_p(ws.data_ptr()), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.25).all())
