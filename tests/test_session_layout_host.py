"""Host: fast_sampler._layout -- where a delivery writes a group of batches and what the consumer reads them through --
driven on CPU tensors with hand-made batch descriptors.  Checked: every pointer the native side gets is the address of
the view the consumer gets (None exactly for an empty one), the views tile the int64 arena in the documented order, every
batch's feature rows and received rows start on a 16-byte boundary, `flat` is the concatenation of the ownership buckets
and the rounded arenas sit on _coarse's grid."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salient_plusplus_amd import _native as nat  # noqa: E402
from salient_plusplus_amd import fast_sampler as fs  # noqa: E402

CPU = torch.device("cpu")
E_ID = torch.empty(0, dtype=torch.int64)


def _descs(n, H, P, rank, rng, all_local=False):
    """n hand-made spp_batch_desc: batch 1 (when there is one) has no node at all, every batch has a hop without edges,
    the buckets of a partitioned batch add up to its nodes with bucket (rank + 1) % P and -- every other batch -- the
    cache bucket empty; `all_local`: no node is owned by a peer"""
    descs = (nat.BatchDesc * n)()
    start = 0
    for i in range(n):
        d = descs[i]
        c = d.counts
        bs = int(rng.integers(1, 40))
        U = 0 if i == 1 else int(rng.integers(200, 900))
        c.num_nodes, c.num_seeds, c.num_hops = U, bs, H
        for h in range(H):
            T = 0 if U == 0 else int(rng.integers(1, max(2, U // (h + 1))))
            c.T[h], c.S[h] = T, min(U, T + int(rng.integers(0, 50)))
            c.E[h] = 0 if (U == 0 or h == i % H) else int(rng.integers(1, 4 * T + 2))
        if P:
            cached = 0 if i % 2 else U // 5
            rest = U - cached
            owners = [rank] if all_local else [m for m in range(P) if m != (rank + 1) % P]
            cuts = sorted(int(v) for v in rng.integers(0, rest + 1, size=len(owners) - 1))
            sizes = np.diff([0] + cuts + [rest])
            for m in range(P + 1):
                c.part_counts[m] = 0
            for m, s in zip(owners, sizes):
                c.part_counts[m] = int(s)
            c.part_counts[P] = cached
            assert sum(int(c.part_counts[m]) for m in range(P + 1)) == U
        d.batch_index, d.start, d.stop, d.slot = i, start, start + bs, i
        start += bs
    return descs


def _addr(p):
    """a c_void_p field or array element as an int (None / 0: the null pointer)"""
    return int(p or 0)


def _check_ptr(p, view, what):
    if view is None or view.numel() == 0:
        assert _addr(p) == 0, f"{what}: a pointer for an empty segment"
    else:
        assert _addr(p) == view.data_ptr(), f"{what}: the native side and the consumer disagree"


SCENARIOS = {
    # single-GPU sessions: feature rows of 8, 16, 200 and 256 bytes
    "rows8": dict(want_x=True, want_y=True, F=4, x_dtype=torch.float16),
    "rows16": dict(want_x=True, want_y=True, F=8, x_dtype=torch.float16),
    "rows200": dict(want_x=True, want_y=True, F=100, x_dtype=torch.float16),
    "rows256": dict(want_x=True, want_y=True, F=64, x_dtype=torch.float32),
    "fp8_table": dict(want_n_id=True, want_x8=True, want_y=True, F=32, x_dtype=torch.float16),
    "table_rows": dict(want_n_id=True, want_y=True),
    "no_features": dict(),
    # partitioned sessions
    "buckets_p2": dict(want_n_id=True, want_parts=True, P=2, rank=0, want_y=True),
    "buckets_p8": dict(want_n_id=True, want_parts=True, P=8, rank=5),
    "native_full_p2": dict(want_n_id=True, want_parts=True, P=2, rank=1, want_x=True, want_y=True, F=100,
                           x_dtype=torch.float16),
    "native_compact_p8": dict(want_n_id=True, P=8, rank=3, want_x=True, want_y=True, F=4, x_dtype=torch.float16),
    "refs_p2": dict(want_n_id=True, refs=True, want_parts=True, P=2, rank=1, want_y=True, F=100, x_dtype=torch.float16),
    "refs_compact_p8": dict(want_n_id=True, refs=True, P=8, rank=0, want_y=True, F=4, x_dtype=torch.float16),
    "refs_nothing_received": dict(want_n_id=True, refs=True, P=2, rank=0, want_y=True, F=100, x_dtype=torch.float16,
                                  all_local=True),
    "refs_p2p": dict(want_n_id=True, refs=True, P=2, rank=0, p2p=True, want_y=True, F=100, x_dtype=torch.float16),
}


@pytest.mark.parametrize("coarse", [True, False])
@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_layout(name, H, n, coarse):
    kw = dict(SCENARIOS[name])
    all_local = kw.pop("all_local", False)
    P, rank = kw.get("P", 0), kw.get("rank", 0)
    want_n_id, refs, want_parts = kw.get("want_n_id", False), kw.get("refs", False), kw.get("want_parts", False)
    want_x, want_x8, want_y = kw.get("want_x", False), kw.get("want_x8", False), kw.get("want_y", False)
    F, x_dtype = kw.get("F", 0), kw.get("x_dtype")
    if want_y:
        kw.update(y_width=1, y_dtype=torch.int64)
    descs = _descs(n, H, P, rank, np.random.default_rng(1000 * H + n), all_local)
    outs, records, arenas = fs._layout(descs, n, device=CPU, e_id=E_ID, coarse=coarse, **kw)
    assert len(outs) == n and len(records) == n

    # ---- the arenas, in the documented order: int64, x, y, received rows
    arenas = list(arenas)
    ids = arenas.pop(0)
    xa = arenas.pop(0) if (want_x or want_x8) else None
    ya = arenas.pop(0) if want_y else None
    received = [0 if kw.get("p2p") else int(d.counts.num_nodes) - int(d.counts.part_counts[rank]) - int(d.counts.part_counts[P])
                for d in descs] if refs else []
    xra = arenas.pop(0) if sum(received) else None
    assert not arenas
    assert ids.dtype == torch.int64 and ids.dim() == 1 and ids.device == CPU
    ids.copy_(torch.arange(ids.numel()))                # distinct values: equal contents mean equal places

    # ---- int64 arena: the views tile it batch after batch, and each pointer is its view's address
    off = 0

    def take(view, length, p, what, native=True):
        nonlocal off
        assert view.dtype == torch.int64 and tuple(view.shape) == (length,), what
        assert view.storage_offset() == off, f"{what}: not where the documented order puts it"
        assert view.untyped_storage().data_ptr() == ids.untyped_storage().data_ptr(), what
        if native:                                      # (the buckets reach the native side as one pointer: parts)
            _check_ptr(p, view, what)
        off += length

    for i, (r, o) in enumerate(zip(records, outs)):
        d, c, m = descs[i], descs[i].counts, o.mfg
        U = int(c.num_nodes)
        assert r.U == U and r.idx_range == (int(d.start), int(d.stop))
        if want_n_id:
            take(r.n_id, U, m.n_id, f"batch {i} n_id")
        else:
            assert r.n_id is None and _addr(m.n_id) == 0
        if refs:
            take(r.row_addr, U, m.row_addr, f"batch {i} row_addr")
        else:
            assert r.row_addr is None and _addr(m.row_addr) == 0
        assert len(r.adjs) == H
        for h, (rp, cl, e_id, ts) in enumerate(r.adjs):
            take(rp, int(c.T[h]) + 1, m.rowptr[h], f"batch {i} rowptr[{h}]")
            take(cl, int(c.E[h]), m.col[h], f"batch {i} col[{h}]")
            assert e_id is E_ID and ts == (int(c.T[h]), int(c.S[h]))
        for h in range(H, nat.SPP_MAX_HOPS):
            assert _addr(m.rowptr[h]) == 0 and _addr(m.col[h]) == 0
        if want_parts:
            pc = [int(c.part_counts[k]) for k in range(P + 1)]
            assert r.pc == pc and len(r.nids) == P
            flat_at = off
            for k in range(P):
                take(r.nids[k], pc[k], None, f"batch {i} bucket {k}", native=False)
            assert r.flat.storage_offset() == flat_at and r.flat.numel() == sum(pc[:P])
            assert torch.equal(r.flat, torch.cat(r.nids))          # exactly the concatenation of the P buckets
            _check_ptr(m.parts, r.flat, f"batch {i} parts")
            take(r.cached, pc[P], m.cached, f"batch {i} cached")
            take(r.perm, U, m.perm, f"batch {i} perm")
        else:
            assert r.nids is None and r.flat is None and r.cached is None and r.perm is None and r.pc is None
            assert _addr(m.parts) == 0 and _addr(m.cached) == 0 and _addr(m.perm) == 0
    assert ids.numel() == (fs._coarse(off) if coarse else off)
    if coarse and off > 2048:
        assert ids.numel() <= 1.03 * off

    # ---- feature rows and received rows: one view per batch, in order, disjoint, each on a 16-byte boundary
    def rows_arena(arena, views, lengths, ptrs, what):
        assert arena.dtype == x_dtype and arena.dim() == 2 and arena.size(1) == F and arena.is_contiguous()
        assert arena.data_ptr() % 16 == 0
        row_b = F * x_dtype.itemsize
        end = 0
        for i, (v, length) in enumerate(zip(views, lengths)):
            assert tuple(v.shape) == (length, F) and v.dtype == x_dtype and v.is_contiguous(), f"{what} {i}"
            assert v.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()
            first = v.storage_offset() // F
            assert v.storage_offset() % F == 0 and first >= end, f"{what} {i}: overlaps the batch before it"
            assert (first * row_b) % 16 == 0, f"{what} {i}: starts off a 16-byte boundary"
            assert first - end < 16 // math.gcd(row_b, 16), f"{what} {i}: more padding than the alignment needs"
            end = first + length
            if ptrs is not None:
                _check_ptr(ptrs[i], v, f"{what} {i}")
        assert end <= arena.size(0)
        pad = 16 // math.gcd(row_b, 16)
        total = sum(length + (-length) % pad for length in lengths)
        assert arena.size(0) == (fs._coarse(total) if coarse else total)
        if coarse and total > 2048:
            assert arena.size(0) <= 1.03 * total

    Us = [int(d.counts.num_nodes) for d in descs]
    if want_x or want_x8:
        # (the rows of an fp8 table are written by the dequantising gather: the native side gets no x pointer)
        rows_arena(xa, [r.x for r in records], Us, [o.x_out for o in outs] if want_x else None, "x")
        if want_x8:
            assert all(_addr(o.x_out) == 0 for o in outs)
    else:
        assert all(r.x is None and _addr(o.x_out) == 0 for r, o in zip(records, outs))
    if xra is not None:
        got = [(r.x_remote, k, o.mfg.x_remote) for r, k, o in zip(records, received, outs) if k]
        rows_arena(xra, [g[0] for g in got], [g[1] for g in got], [g[2] for g in got], "received rows")
    for r, k, o in zip(records, received or [0] * n, outs):
        if not k:                                       # nothing received for this batch: no view and no pointer
            assert r.x_remote is None and _addr(o.mfg.x_remote) == 0

    # ---- labels: exactly the seeds' rows, never rounded
    if want_y:
        bss = [int(d.stop) - int(d.start) for d in descs]
        assert tuple(ya.shape) == (sum(bss), 1) and ya.dtype == torch.int64
        at = 0
        for i, (r, o) in enumerate(zip(records, outs)):
            assert tuple(r.y.shape) == (bss[i], 1) and r.y.storage_offset() == at
            _check_ptr(o.y_out, r.y, f"batch {i} y")
            at += bss[i]
    else:
        assert all(r.y is None and _addr(o.y_out) == 0 for r, o in zip(records, outs))


def test_coarse_grid():
    """32 sizes per octave, never below the request, exact up to 64 elements"""
    for v in list(range(0, 200)) + [2047, 2048, 2049, 4095, 123457, (1 << 31) + 5]:
        c = fs._coarse(v)
        assert c >= max(v, 1)
        if v <= 64:
            assert c == max(v, 1)
        else:
            g = 1 << (v.bit_length() - 6)
            assert c % g == 0 and c - v < g
