"""The GATv2 and TransformerConv training pairs (csrc/gatv2.hip, csrc/transformer_conv.hip: the eight entries
spp_{gatv2,transformer}_{forward,backward}[_drop]) against the bits of the commit BEFORE their shared pieces moved into
csrc/attn_train.hip.h: SHA-256 digests of the output bytes, recorded there on an MI355X and compared here with equality.
tests/golden/attention_train_bits.json holds one record per case and output array -- the digest and the array's first
eight values as hex, which say what moved when a digest does.

The digests are never made from the code under test.  To record them, check out the commit whose bits are the contract,
copy this file there unchanged and run it with SPP_RECORD_ATTENTION_TRAIN_BITS=<file to write>; recording refuses a
digest that is the one of an all-zero array of the same size, which would pin nothing.

Everything the kernels read is integer arithmetic: a multiplicative hash of (row, column) reduced to 16 bits and divided
by a power of two, exact in fp32 -- the same bytes on any machine and any torch, no random generator.  bf16 rows are
those values rounded to nearest even, so the fp32 and the bf16 cases read different numbers.

Shapes: every case of with_bwd_shape (which covers every case of with_fwd_shape), then (2, 8) -- D = 16, several targets
per wavefront -- and (8, 32) -- NS = 4 with two heads per hash word, the edge of the backward's once-per-wavefront hash.
Two hops of T = 5 targets over S = 40 sources.  Hop A is ragged: an empty row, a row holding its own diagonal entry, a
row with a repeated entry and a row of 9 entries (no multiple of 2 or 4: the clamped tail of a round).  In hop B every
`col` value is distinct and at least T, so every address of grad_x_l / grad_k / grad_v receives exactly one atomic add
onto zero and its bits are fixed; on hop A only the arrays without atomics are compared.  grad_att is compared where the
backward runs as one workgroup (T <= 256 / min(64, D): D <= 32 here); elsewhere the float64-bounded tests cover it.
Every case runs without dropout and with it (p = 0.5, a fixed seed, training = 1), on fp32 and on bf16 rows."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_train_bits.json")
RECORD = os.environ.get("SPP_RECORD_ATTENTION_TRAIN_BITS")

T, S = 5, 40
P, SEED = 0.5, 0x5EEDF4A7C15
SHAPES = [(1, 4), (2, 64), (1, 128), (4, 64), (2, 128), (1, 256), (8, 64),         # with_bwd_shape, case by case
          (4, 128), (2, 256), (1, 512), (8, 128), (4, 256), (2, 512), (1, 1024),
          (2, 8), (8, 32)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
HOPS = {
    "A": [[], [1, 7, 12], [9, 9, 11, 9], [5, 6, 13, 20, 21, 22, 30, 31, 39], [0, 3]],
    "B": [[17, 5, 33], [8], [6, 39, 21, 10, 27, 14, 35, 9, 30], [12, 24, 7, 19], [38, 11]],
}


def _hash8(rows, cols, salt):
    """[rows, cols] int64 in [0, 256): a multiplicative hash of (row, column); every intermediate stays below 2^40"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    v = (r * 73856093 + c * 19349663 + salt * 83492791) & 0xFFFFFF
    v = ((v ^ (v >> 11)) * 40503) & 0xFFFFFF
    v = ((v ^ (v >> 9)) * 48271) & 0xFFFFFF
    return (v >> 13) & 0xFF


def _matrix(salt, rows, cols, lo, div):
    """(hash + lo) / div with a 16-bit hash in units of 1 / 256: at most 17 significant bits, exact in fp32"""
    h = _hash8(rows, cols, salt) * 256 + _hash8(rows, cols, salt + 500)
    return (h + lo * 256).to(torch.float32) / (div * 256)


def _hop(name):
    rows = HOPS[name]
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    return rowptr.cuda(), torch.tensor([j for r in rows for j in r], dtype=torch.int64).cuda()


def _records(arrays):
    got = {}
    for name, a in arrays.items():
        raw = a.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
        got[name] = {"sha256": hashlib.sha256(raw).hexdigest(), "first8": raw[:32].hex()}
        if RECORD:
            assert got[name]["sha256"] != hashlib.sha256(bytes(len(raw))).hexdigest(), f"{name}: all zeros pin nothing"
    return got


def _call(name, desc, drop):
    import salient_plusplus_amd._native as nat
    args = (C.byref(desc), C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())))
    nat.check(getattr(nat.load(), name + "_drop")(*args, P, 1, SEED) if drop else getattr(nat.load(), name)(*args))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _variants():
    for hop in sorted(HOPS):
        for rn, rdt in DTYPES.items():
            for drop in (False, True):
                yield f"hop={hop},rows={rn},drop={int(drop)}", hop, rdt, drop


def _outputs(H, Cc):
    f32 = dict(dtype=torch.float32, device="cuda")
    D = H * Cc
    return D, torch.empty((T, D), **f32), torch.empty((T, H), **f32), torch.empty((T, H), **f32), \
        _matrix(8, T, D, -128, 64).cuda()


def _gatv2_cases(H, Cc):
    import salient_plusplus_amd._native as nat
    for key, hop, rdt, drop in _variants():
        D, out, rmax, rsum, g = _outputs(H, Cc)
        rowptr, col = _hop(hop)
        x_l = _matrix(1, S, D, -64, 64).to(rdt).cuda()           # the messages: [-1, 3)
        x_r = _matrix(2, T, D, -128, 64).to(rdt).cuda()
        att = _matrix(3, H, Cc, -128, 16 * Cc).cuda()
        g_xl, g_xr, g_att = torch.zeros((S, D), device="cuda"), torch.empty((T, D), device="cuda"), \
            torch.empty((H, Cc), device="cuda")
        d = nat.Gatv2Desc(heads=H, x_elem=nat.SPP_ELEM_F32 if rdt == torch.float32 else nat.SPP_ELEM_BF16,
                          negative_slope=0.2, rowptr_dev=_ptr(rowptr), col_dev=_ptr(col), num_targets=T, num_sources=S,
                          C=Cc, x_l_dev=_ptr(x_l), x_l_stride_elems=D, x_r_dev=_ptr(x_r), x_r_stride_elems=D,
                          att_dev=_ptr(att), out_dev=_ptr(out), row_max_dev=_ptr(rmax), row_sum_dev=_ptr(rsum),
                          grad_out_dev=_ptr(g), grad_x_l_dev=_ptr(g_xl), grad_x_r_dev=_ptr(g_xr),
                          grad_att_dev=_ptr(g_att))
        _call("spp_gatv2_forward", d, drop)
        _call("spp_gatv2_backward", d, drop)
        torch.cuda.synchronize()
        arrays = {"out": out, "row_max": rmax, "row_sum": rsum, "grad_x_r": g_xr}
        if hop == "B":
            arrays["grad_x_l"] = g_xl
        if T <= 256 // min(64, D):                                # the backward is one workgroup
            arrays["grad_att"] = g_att
        yield key, _records(arrays)


def _transformer_cases(H, Cc):
    import salient_plusplus_amd._native as nat
    for key, hop, rdt, drop in _variants():
        D, out, rmax, rsum, g = _outputs(H, Cc)
        rowptr, col = _hop(hop)
        q = _matrix(4, T, D, -128, 64).to(rdt).cuda()
        k, v = _matrix(5, S, D, -128, 64).to(rdt).cuda(), _matrix(6, S, D, -64, 64).to(rdt).cuda()
        g_q = torch.empty((T, D), device="cuda")
        g_k, g_v = torch.zeros((S, D), device="cuda"), torch.zeros((S, D), device="cuda")
        d = nat.TransformerDesc(heads=H, x_elem=nat.SPP_ELEM_F32 if rdt == torch.float32 else nat.SPP_ELEM_BF16,
                                scale=2.0 ** -(Cc.bit_length() // 2),     # a power of two near 1 / sqrt(C)
                                rowptr_dev=_ptr(rowptr), col_dev=_ptr(col), num_targets=T, num_sources=S, C=Cc,
                                q_dev=_ptr(q), q_stride_elems=D, k_dev=_ptr(k), k_stride_elems=D, v_dev=_ptr(v),
                                v_stride_elems=D, out_dev=_ptr(out), row_max_dev=_ptr(rmax), row_sum_dev=_ptr(rsum),
                                grad_out_dev=_ptr(g), grad_q_dev=_ptr(g_q), grad_k_dev=_ptr(g_k), grad_v_dev=_ptr(g_v))
        _call("spp_transformer_forward", d, drop)
        _call("spp_transformer_backward", d, drop)
        torch.cuda.synchronize()
        arrays = {"out": out, "row_max": rmax, "row_sum": rsum, "grad_q": g_q}
        if hop == "B":
            arrays["grad_k"], arrays["grad_v"] = g_k, g_v
        yield key, _records(arrays)


FAMILIES = {"gatv2": _gatv2_cases, "transformer": _transformer_cases}


def _dump(book, f):
    """the fixture's layout: one line per family and shape"""
    fams = (f'"{fam}": {{\n' + ",\n".join(f'"{sh}": ' + json.dumps(book[fam][sh], sort_keys=True, separators=(",", ":"))
                                           for sh in sorted(book[fam])) + "\n}" for fam in sorted(book))
    f.write("{\n" + ",\n".join(fams) + "\n}\n")


def test_the_hops_are_the_ones_the_digests_were_recorded_on():
    a, b = HOPS["A"], HOPS["B"]
    assert len(a) == len(b) == T
    assert a[0] == [] and 1 in a[1] and len(set(a[2])) < len(a[2]) and len(a[3]) == 9
    flat = [j for r in b for j in r]
    assert len(set(flat)) == len(flat) and all(T <= j < S for j in flat) and any(len(r) == 9 for r in b)
    assert all(0 <= j < S for r in a for j in r)
    for t in (_matrix(1, S, 1024, -64, 64), _matrix(5, S, 1024, -128, 64)):
        assert not torch.equal(t.bfloat16().float(), t) and t.unique().numel() > 20000


@pytest.mark.parametrize("H,Cc", SHAPES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_bits_are_the_parents(family, H, Cc):
    shape = f"H{H}_C{Cc}"
    got = dict(FAMILIES[family](H, Cc))
    if RECORD:
        book = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        book.setdefault(family, {})[shape] = got
        with open(RECORD, "w") as f:
            _dump(book, f)
        pytest.skip(f"recorded {len(got)} cases, compared nothing")
    want = json.load(open(FIXTURE))[family][shape]
    assert sorted(got) == sorted(want)
    assert all(sorted(got[key]) == sorted(want[key]) for key in got)
    moved = [f"{key}: {name} (first eight: {rec['first8']}, recorded {want[key][name]['first8']})"
             for key in sorted(got) for name, rec in got[key].items() if rec["sha256"] != want[key][name]["sha256"]]
    assert not moved, f"{len(moved)} digests moved: {moved[:8]}"
