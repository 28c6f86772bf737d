"""GPU: fp8 (e4m3) feature tables on the partitioned path -- every rank holds its partition (and its VIP cache) as
Fp8Features, the native exchange (session.hip) moves the e4m3 bytes, and the dequantising assembly of the delivery
launch (sampler.hip, k_deliver<16, false, true> / k_deliver_group<16, false, true>) writes fp16 rows.  Ranks are
threads on the in-process transport, as in test_gpu_native_exchange.py.

The table is a seeded normal [3000, F] quantised ONCE; ranks take full.rows(...).  Expected features are
full.rows(n_id).dequantize(fp16) with the oracle's n_id, compared as uint16 bit patterns: fp16(float32(q) * 2^e) is
one well-defined number (the product is exact, the rounding to fp16 happens once), so there is no tolerance."""
import dataclasses
import functools
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SIZES = [15, 10, 5]
N_CACHED = 250


@functools.lru_cache(maxsize=None)
def _graph():
    g = np.load(os.path.join(ROOT, "tests", "golden", "graph_a.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def _table(F):
    """(Fp8Features of the whole table, its fp16 dequantisation as a numpy array): quantised once per width"""
    from salient_plusplus_amd.fp8 import quantize_e4m3
    n = _graph()["rowptr"].shape[0] - 1
    x = np.random.default_rng(7).standard_normal((n, F)).astype(np.float16)
    full = quantize_e4m3(torch.from_numpy(x))
    return full, full.dequantize(torch.float16).numpy()


def _offsets(P, degenerate=False):
    n = _graph()["rowptr"].shape[0] - 1
    if degenerate:
        return [0, n, n]
    return {2: [0, 1400, n], 3: [0, 900, 2100, n]}[P]


def _rank_idx(rank, P):
    idx = _graph()["idx"]
    return idx[(len(idx) * rank) // P:(len(idx) * (rank + 1)) // P]


def _cached_vertices(rank, offsets):
    n = _graph()["rowptr"].shape[0] - 1
    lo, hi = int(offsets[rank]), int(offsets[rank + 1])
    remote = np.setdiff1d(np.arange(n), np.arange(lo, hi))
    return np.sort(np.random.default_rng(100 + rank).choice(remote, size=N_CACHED, replace=False)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _oracle(rank, P, nb, bs):
    """the oracle's batches of one rank's epoch, computed once and shared by the tests (and both epochs)"""
    from oracle import oracle as orc
    g, idx = _graph(), _rank_idx(rank, P)
    ranges = orc.batch_ranges(len(idx), bs, False, True, nb)
    return [(int(a), int(b), orc.sample_batch(g["rowptr"], g["col"], idx, int(a), int(b), SIZES)) for a, b in ranges]


def _rank_cfg(rank, P, offsets, use_cache, nb, bs, F, fs, fp16=False, bump_scale=None):
    """fp8: x_gpu = this rank's rows of the quantised table, x_cpu empty.  fp16: the same VALUES as an fp16 table (the
    comparison of case 4).  bump_scale: (rank, column) whose exponent is one higher than everybody else's."""
    from salient_plusplus_amd.fast_trainer.samplers import FastSamplerConfig
    from salient_plusplus_amd.fp8 import Fp8Features
    T = torch.from_numpy
    g = _graph()
    full, deq = _table(F)
    lo, hi = int(offsets[rank]), int(offsets[rank + 1])
    cache = fs.Cache()
    if use_cache:
        cv = _cached_vertices(rank, offsets)
        cache = fs.Cache(rank, P, T(cv), T(deq[cv].copy()) if fp16 else full.rows(T(cv)))
    if fp16:
        x_gpu, x_cpu = torch.empty(0), T(deq[lo:hi].copy())
    else:
        x_gpu, x_cpu = full.rows(slice(lo, hi)), torch.empty(0)
        if bump_scale is not None and bump_scale[0] == rank:
            e = x_gpu.scale_log2.clone()
            e[bump_scale[1]] += 1
            x_gpu = Fp8Features(x_gpu.q, e)
    return FastSamplerConfig(
        x_cpu=x_cpu, x_gpu=x_gpu, y=T(g["y"]).unsqueeze(-1), rowptr=T(g["rowptr"]), col=T(g["col"]), idx=T(_rank_idx(rank, P)),
        batch_size=bs, sizes=SIZES, skip_nonfull_batch=False, pin_memory=False, distributed=True,
        partition_book=fs.RangePartitionBook(rank, P, T(np.asarray(offsets, dtype=np.int64))), cache=cache,
        force_exact_num_batches=True, exact_num_batches=nb, count_remote_frequency=False, use_cache=use_cache)


def _check_batch(batch, want, deq, F):
    start, stop, m = want
    g = _graph()
    assert batch.x.is_cuda and batch.x.dtype == torch.float16 and tuple(batch.x.shape) == (m.n_id.shape[0], F)
    np.testing.assert_array_equal(batch.x.cpu().numpy().view(np.uint16), deq[m.n_id].view(np.uint16))
    np.testing.assert_array_equal(batch.y.cpu().numpy().reshape(-1), g["y"][m.n_id[:stop - start]])
    for adj, hop in zip(batch.adjs, m.hops):
        rp, cl, _ = adj.adj_t.csr()
        np.testing.assert_array_equal(rp.cpu().numpy(), hop.rowptr)
        np.testing.assert_array_equal(cl.cpu().numpy(), hop.col)


def _run_rank(rank, P, comms, offsets, use_cache, nb, bs, slots, F, epochs, fp16, errors, stats):
    it = None
    from salient_plusplus_amd import fast_sampler as fs
    try:
        from salient_plusplus_amd.fast_trainer.samplers import FastSampler
        from salient_plusplus_amd.fast_trainer.transferers import DeviceDistributedPrefetcher
        torch.cuda.set_device(0)
        fs.set_native_comm(comms[rank])
        cfg = _rank_cfg(rank, P, offsets, use_cache, nb, bs, F, fs, fp16=fp16)
        want = _oracle(rank, P, nb, bs)
        deq = _table(F)[1]
        dev = torch.device("cuda", 0)
        for epoch in range(epochs):     # the second epoch reuses the pooled sampler and grown buffers
            it = iter(FastSampler(2, slots, cfg))
            assert it.session.native_exchange
            pre = DeviceDistributedPrefetcher([dev], it, True)
            got = 0
            held = []
            for (batch,) in pre:
                held.append(batch)
                got += 1
                if got == 2:
                    pre.quiesce()       # every rank at the same batch: all in-flight exchanges complete
                if epoch == 0:          # epoch 1 compares after the epoch: no host sync between batches
                    _check_batch(held.pop(), want[got - 1], deq, F)
            for k, batch in enumerate(held):
                _check_batch(batch, want[k], deq, F)
            assert got == nb
            stats[rank] = pre.NUMBER_OF_SENT_BYTES
            it.session.close()
    except BaseException as e:  # noqa: BLE001
        import traceback
        errors.append(f"rank {rank}: {e}\n{traceback.format_exc()}")
        if it is not None:
            it.session.close()
        comms[rank].close()     # wakes the peers out of the rendezvous
    finally:
        fs.set_native_comm(None)


def _run(P, offsets, use_cache, nb, bs, slots, F, epochs=2, fp16=False, target=_run_rank, extra=()):
    from salient_plusplus_amd import fast_sampler as fs
    for r in range(P):                  # the shared references, once, before the ranks start
        _oracle(r, P, nb, bs)
    _table(F)
    comms = fs.NativeComm.local(P)
    errors, stats = [], {}
    ts = [threading.Thread(target=target, args=(r, P, comms, offsets, use_cache, nb, bs, slots, F, epochs, fp16, errors, stats)
                           + tuple(extra)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(180)
    hung = [t for t in ts if t.is_alive()]
    for c in comms:
        c.close()
    assert not hung, "rank thread hung"
    return errors, stats


# (P, degenerate book, cache, F, nb, bs, slots)
ONE_PIECE = (2, False, False, 16, 3, 32, 6)         # one 16-byte piece per row (one lane per row), one group
THREE_PIECES = (2, False, True, 48, 7, 16, 4)       # three pieces on four lanes (a lane past the last piece), several groups,
#                                                     ragged last group, all three sources (own partition / cache / received)
WORKLOAD = (3, False, True, 128, 5, 24, 16)         # the workload's width: eight pieces on eight lanes, the unconditional body
ALL_REMOTE = (2, True, False, 32, 4, 16, 8)         # book [0, n, n]: every row of rank 1 is received, rank 0 only serves


@pytest.mark.parametrize("case,issue", [(ONE_PIECE, "consumer"), (THREE_PIECES, "consumer"), (THREE_PIECES, "thread"),
                                        (WORKLOAD, "consumer"), (ALL_REMOTE, "consumer")])
def test_fp8_partitions_over_the_native_exchange(case, issue, monkeypatch):
    P, degenerate, use_cache, F, nb, bs, slots = case
    monkeypatch.setenv("SPP_EXCHANGE_ISSUE", issue)
    errors, stats = _run(P, _offsets(P, degenerate), use_cache, nb, bs, slots, F)
    assert not errors, "\n".join(errors)
    assert all(stats[r] > 0 for r in range(P))      # counts / ids / rows really travelled


def test_fp8_partitions_with_group_delivery(monkeypatch):
    """one delivery launch per GROUP (k_deliver_group's fp8 instantiation), output arenas of 2F-byte rows"""
    monkeypatch.setenv("SPP_GROUP_DELIVERY", "1")
    P, degenerate, use_cache, F, nb, bs, slots = THREE_PIECES
    errors, _stats = _run(P, _offsets(P, degenerate), use_cache, nb, bs, slots, F)
    assert not errors, "\n".join(errors)


def test_rows_wider_than_64_pieces():
    """F = 1040: 65 pieces on 64 lanes -- the beyond-64-pieces loop with its per-piece scales"""
    errors, _stats = _run(2, _offsets(2), False, 2, 8, 4, 1040)
    assert not errors, "\n".join(errors)


def test_fp8_halves_the_row_bytes_on_the_wire():
    """NUMBER_OF_SENT_BYTES (transferers.py: the Session's sent bytes = rows served * row_bytes + ids requested * 4 +
    counts) of the same epoch with the dequantised fp16 table and with the fp8 table: ids and counts are the same, a
    served row is 2F bytes against F -- the difference is exactly (rows this rank served) * F."""
    P, degenerate, use_cache, F, nb, bs, slots = THREE_PIECES
    offsets = _offsets(P, degenerate)
    e16, s16 = _run(P, offsets, use_cache, nb, bs, slots, F, epochs=1, fp16=True)
    assert not e16, "\n".join(e16)
    e8, s8 = _run(P, offsets, use_cache, nb, bs, slots, F, epochs=1)
    assert not e8, "\n".join(e8)
    for r in range(P):
        lo, hi = offsets[r], offsets[r + 1]
        served = 0                                   # rows the peers ask rank r for: theirs to need, r's to own, not cached
        for m in range(P):
            if m == r:
                continue
            cv = _cached_vertices(m, offsets)
            for _a, _b, mfg in _oracle(m, P, nb, bs):
                ids = mfg.n_id[(mfg.n_id >= lo) & (mfg.n_id < hi)]
                served += int((~np.isin(ids, cv)).sum())
        assert served > 0
        print(f"rank {r}: fp16 {s16[r]} B, fp8 {s8[r]} B, rows served {served}")
        assert s8[r] < s16[r]
        assert s16[r] - s8[r] == served * F


def _run_rank_mismatch(rank, P, comms, offsets, use_cache, nb, bs, slots, F, epochs, fp16, errors, stats, bump):
    from salient_plusplus_amd import fast_sampler as fs
    it = None
    try:
        from salient_plusplus_amd.fast_trainer.samplers import FastSampler
        torch.cuda.set_device(0)
        fs.set_native_comm(comms[rank])
        cfg = _rank_cfg(rank, P, offsets, use_cache, nb, bs, F, fs, bump_scale=bump)
        try:
            it = iter(FastSampler(2, slots, cfg))
            stats[rank] = "created"
            stats[rank] = "delivered" if next(it, None) is not None else "created"
        except RuntimeError as e:
            stats[rank] = str(e)
    except BaseException as e:  # noqa: BLE001
        import traceback
        errors.append(f"rank {rank}: {e}\n{traceback.format_exc()}")
    finally:
        # (the communicators are closed by the main thread after the join: a rank that left early would turn its
        # peer's refusal into "a peer rank left")
        if it is not None:
            it.session.close()
        fs.set_native_comm(None)


def test_ranks_with_different_scales_are_refused_at_creation():
    """rank 1's exponent of one column is one higher: a row it serves would be dequantised wrongly by rank 0 with no
    other symptom.  The creation-time rendezvous compares the scales' tags: creation fails on BOTH ranks, naming the
    scales; no batch is delivered and nobody waits for anybody."""
    P, degenerate, use_cache, F, nb, bs, slots = ONE_PIECE
    errors, stats = _run(P, _offsets(P, degenerate), use_cache, nb, bs, slots, F, target=_run_rank_mismatch, extra=((1, 5),))
    assert not errors, "\n".join(errors)
    for r in range(P):
        assert stats[r] not in ("created", "delivered") and "scales" in stats[r], stats[r]
    from salient_plusplus_amd import fast_sampler as fs
    torch.cuda.synchronize()
    assert fs.async_errors() == 0


def test_cache_with_other_scales_is_refused_before_any_device_call():
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fp8 import Fp8Features
    P, degenerate, _use_cache, F, nb, bs, _slots = THREE_PIECES
    offsets = _offsets(P, degenerate)
    full = _table(F)[0]
    cv = torch.from_numpy(_cached_vertices(0, offsets))
    e = full.scale_log2.clone()
    e[2] += 1
    cfg = _rank_cfg(0, P, offsets, True, nb, bs, F, fs)
    with pytest.raises(RuntimeError, match="scales"):
        dataclasses.replace(cfg, cache=fs.Cache(0, P, cv, Fp8Features(full.rows(cv).q, e)))
