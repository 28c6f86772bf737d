"""graph_gatv2_aggregate and graph_transformer_aggregate (csrc/graph_gatv2.hip, csrc/graph_transformer.hip: each a rows
kernel and a long-row kernel, the same pair but for four places) against the bits of the commit that added this test,
before anything is done to fold the two pairs into one: SHA-256 digests of the output bytes, recorded
there on an MI355X and compared here with equality.  tests/golden/graph_attention_bits.json holds one digest per case
and row class (empty, short, exactly one chunk, long), so a failure names what moved.

The digests are never made from the code under test.  To record them, check out the commit whose bits are the contract,
copy this file there unchanged and run it with SPP_RECORD_ATTENTION_BITS=<file to write>; recording refuses a digest
that is the one of an all-zero output of the same size (other than the empty rows'), which would pin nothing.

Everything the kernels read is integer arithmetic: a multiplicative hash of (row, column) reduced to 16 bits and divided
by a power of two, exact in fp32 -- the same bytes on any machine and any torch, no random generator.  bf16 rows are
those values rounded to nearest even, so the fp32 and the bf16 cases read different numbers.

The graph (40 nodes) has a row without entries, a row of diagonal entries only, rows of exactly C_g = 64 and of 65
entries, a row of repeats, one `col` id outside the graph, and a hub of 64 * 256 + 1 entries: at the narrowest shape
(one lane a row, 256 lane groups a workgroup) the shortest row whose long kernel runs a second round and so parks its
states in an LDS buffer that was used before; every wider shape runs many rounds on it.  One (H, C) per (NQ, CPH)
dispatch case, crossed with fp32 / bf16 rows and outputs, a slab and a shuffled id list (one duplicate, one id outside
the graph), relu on and off, and per family x_r apart / x_r is x_l, or no skip / a skip / a skip that is the output."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_attention_bits.json")
RECORD = os.environ.get("SPP_RECORD_ATTENTION_BITS")

N = 40
CG = 64
HUB_LEN = CG * 256 + 1
EMPTY, DIAG, ONE_CHUNK, JUST_OVER, REPEATS, OUTSIDE_COL, HUB, ONE_CHUNK_2 = range(8)
# <NQ, CPH> = <1,1> (1 lane a row), <1,1> (8 lanes), <2,1>, <2,2>, <4,1>, <4,2>, <4,4>
SHAPES = [(1, 4), (4, 8), (2, 256), (1, 512), (4, 256), (2, 512), (1, 1024)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CLASSES = ("empty", "short", "one_chunk", "long")


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


def _graph():
    """rowptr, col (with the entry outside the graph) and the entry count of every row"""
    rows = []
    for t in range(N):
        n = 1 + (t * 5) % 23
        if t == EMPTY:
            n = 0
        elif t in (ONE_CHUNK, ONE_CHUNK_2):
            n = CG
        elif t == JUST_OVER:
            n = CG + 1
        elif t == HUB:
            n = HUB_LEN
        row = (_hash8(1, n, 1000 + t)[0] % N).tolist() if n else []
        if t == DIAG:
            row = [DIAG, DIAG]
        elif t == REPEATS:
            row = [9, 9, 11, 9, 11, 11, 9]
        elif t == OUTSIDE_COL:
            row[2] = N + 3
        rows.append(row)
    assert len(rows[OUTSIDE_COL]) > 2 and DIAG not in (0, N + 3)
    deg = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.tensor([j for r in rows for j in r], dtype=torch.int64)
    return rowptr, col, deg


def _id_list():
    """every node, JUST_OVER a second time and one id outside the graph, in an order fixed by the hash"""
    ids = list(range(N)) + [JUST_OVER, N + 2]
    key = _hash8(1, len(ids), 77)[0].tolist()
    return [ids[p] for p in sorted(range(len(ids)), key=lambda p: (key[p], p))]


def _classes(targets, deg):
    """row class -> the output rows of it, in output order"""
    where = {c: [] for c in CLASSES}
    for i, t in enumerate(targets):
        n = int(deg[t]) if 0 <= t < N else 0          # a target outside the graph has no row: zeros
        where["empty" if n == 0 else "short" if n < CG else "one_chunk" if n == CG else "long"].append(i)
    assert all(where.values())
    return where


def _digests(out, where):
    host = out.cpu()
    got = {}
    for c, idx in where.items():
        raw = host[torch.tensor(idx)].contiguous().view(torch.uint8).numpy().tobytes()
        got[c] = hashlib.sha256(raw).hexdigest()
        if RECORD and c != "empty":
            assert got[c] != hashlib.sha256(bytes(len(raw))).hexdigest(), f"{c}: an all-zero output pins nothing"
    return got


def _crossed():
    """(key, rows dtype, out dtype, by ids, relu) of every case but the family's own variants"""
    for rn, rdt in DTYPES.items():
        for on, odt in DTYPES.items():
            for by_ids in (False, True):
                for relu in (False, True):
                    yield f"rows={rn},out={on},{'ids' if by_ids else 'slab'},relu={int(relu)}", rdt, odt, by_ids, relu


def _gatv2_cases(H, Cc):
    from salient_plusplus_amd.inference import graph_gatv2_aggregate
    D = H * Cc
    rowptr, col, deg = _graph()
    rowptr, col = rowptr.cuda(), col.cuda()
    ids = _id_list()
    x_l = _matrix(1, N, D, -64, 64)                    # the messages: [-1, 3), so a row of many entries is not all <= 0
    x_r = _matrix(2, N, D, -128, 64)
    att = (_matrix(3, H, Cc, -128, 16 * Cc)).cuda()
    for key, rdt, odt, by_ids, relu in _crossed():
        targets = ids if by_ids else list(range(N))
        kw = dict(target_ids=torch.tensor(ids).cuda()) if by_ids else dict(row0=0, num_targets=N)
        l, r = x_l.to(rdt).cuda(), x_r.to(rdt).cuda()
        for variant, xr in (("x_r", r), ("x_r_is_x_l", l)):
            out = graph_gatv2_aggregate(l, xr, att, rowptr, col, relu=relu, out_dtype=odt, **kw)
            yield f"{key},{variant}", _digests(out, _classes(targets, deg))


def _transformer_cases(H, Cc):
    from salient_plusplus_amd.inference import graph_transformer_aggregate
    D = H * Cc
    rowptr, col, deg = _graph()
    rowptr, col = rowptr.cuda(), col.cuda()
    ids = _id_list()
    scale = 2.0 ** -(Cc.bit_length() // 2)             # a power of two near 1 / sqrt(C)
    q, k = _matrix(4, N, D, -128, 64), _matrix(5, N, D, -128, 64)
    v, skip = _matrix(6, N, D, -64, 64), _matrix(7, N, D, -128, 64)
    for key, rdt, odt, by_ids, relu in _crossed():
        targets = ids if by_ids else list(range(N))
        kw = dict(target_ids=torch.tensor(ids).cuda()) if by_ids else dict(row0=0, num_targets=N)
        dq, dk, dv, ds = (t.to(rdt).cuda() for t in (q, k, v, skip))
        call = lambda **more: graph_transformer_aggregate(dq, dk, dv, rowptr, col, heads=H, scale=scale, relu=relu,
                                                          out_dtype=odt, **kw, **more)
        where = _classes(targets, deg)
        yield f"{key},no_skip", _digests(call(), where)
        yield f"{key},skip", _digests(call(skip=ds), where)
        if not by_ids and rdt == odt:                  # output row i IS skip row t: a slab over the one matrix
            buf = ds.clone()
            yield f"{key},skip_is_out", _digests(call(skip=buf, out=buf), where)


FAMILIES = {"gatv2": _gatv2_cases, "transformer": _transformer_cases}


def test_the_graph_is_the_one_the_digests_were_recorded_on():
    rowptr, col, deg = _graph()
    assert int(deg[EMPTY]) == 0 and int(deg[ONE_CHUNK]) == CG and int(deg[JUST_OVER]) == CG + 1
    assert int(deg[HUB]) == HUB_LEN and int(((col < 0) | (col >= N)).sum()) == 1
    assert col[rowptr[DIAG]:rowptr[DIAG + 1]].tolist() == [DIAG, DIAG]
    from salient_plusplus_amd.inference import graph_gatv2_chunk, graph_transformer_chunk
    assert graph_gatv2_chunk() == CG and graph_transformer_chunk() == CG
    ids = _id_list()
    assert ids != sorted(ids) and ids.count(JUST_OVER) == 2 and N + 2 in ids
    for t in (_matrix(1, N, 1024, -64, 64), _matrix(2, N, 1024, -128, 64)):
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
            json.dump(book, f, indent=0, sort_keys=True)
        pytest.skip(f"recorded {len(got)} cases, compared nothing")
    want = json.load(open(FIXTURE))[family][shape]
    assert sorted(got) == sorted(want)
    moved = [f"{key}: {c}" for key in sorted(got) for c in CLASSES if got[key][c] != want[key][c]]
    assert not moved, f"{len(moved)} of {len(got) * len(CLASSES)} digests moved: {moved[:12]}"
