"""GPU: batch-at-a-time delivery (SPP_GROUP_FETCH=0: spp_session_next / spp_session_export per batch) of DISTRIBUTED
sessions -- without a native communicator (the record carries the ownership buckets for the torch-collective exchange)
and with the native exchange between two in-process ranks.  Every record must be, field by field, the record the
default mode (the group fetched as a whole) hands out for the same batch, and every batch must match the oracle.
Graph, configurations and in-process ranks are those of test_gpu_native_exchange."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_gpu_native_exchange import SIZES, _check_batch, _graph, _rank_cfg  # noqa: E402

pytestmark = pytest.mark.gpu

OFFSETS = [0, 1400]             # two partitions: [0, 1400) and [1400, n)


def _host(t):
    return None if t is None else t.cpu().numpy().copy()


def _host_record(b, kept):
    """every field of a Session's distributed record as host data (features as their 16-bit patterns)"""
    return {
        "x": None if b.x is None else _host(b.x).view(np.uint16),
        "partition_nids": [_host(t) for t in b.partition_nids],
        "partition_nids_flat": _host(getattr(b, "partition_nids_flat", None)),
        "cached_nids": _host(b.cached_nids),
        "perm_partition_to_mfg": _host(b.perm_partition_to_mfg),
        "partition_counts": getattr(b, "partition_counts", None),
        "sliced_cpu_features": (tuple(b.sliced_cpu_features.shape), b.sliced_cpu_features.dtype,
                                b.sliced_cpu_features.device.type),
        "sliced_cpu_labels": _host(b.sliced_cpu_labels),
        "adjs": [(_host(rp), _host(cl), tuple(e.shape), (int(ts[0]), int(ts[1]))) for rp, cl, e, ts in b.adjs],
        "idx_range": (int(b.idx_range[0]), int(b.idx_range[1])),
        "n_id": _host(b.n_id),
        "kept": None if kept is None else (_host(kept[0]).view(np.uint16), _host(kept[1])),
        "devices": sorted({t.device.type for t in [b.cached_nids, b.perm_partition_to_mfg, b.n_id, *b.partition_nids]
                           if t is not None}),
    }


def _same(a, b, what):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert a is not None and b is not None, what
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} / {b.dtype}{b.shape}"
        np.testing.assert_array_equal(a, b, err_msg=what)
    elif isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        assert len(a) == len(b), what
        for k, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{what}[{k}]")
    else:
        assert a == b, f"{what}: {a!r} / {b!r}"


def _same_records(batch_mode, default_mode, compact, who):
    assert len(batch_mode) == len(default_mode), who
    for k, (a, b) in enumerate(zip(batch_mode, default_mode)):
        assert a.keys() == b.keys()
        for name in a:
            # a compact native record has no use for the bucket sizes: they are compared wherever both modes carry them
            if name == "partition_counts" and compact and (a[name] is None or b[name] is None):
                continue
            _same(a[name], b[name], f"{who} batch {k} {name}")


def _drain(sess, compact, check=None):
    sess.compact_native_records = compact
    out = []
    while True:
        b = sess.blocking_get_batch_distributed()
        if b is None:
            break
        kept = sess.take_native_features(b.idx_range) if sess.native_exchange else None
        if check is not None:
            check(b, len(out))
        out.append(_host_record(b, kept))
    return out


# ---- (a) no native communicator: the record of the torch-collective exchange ----
def _bucket_session_records(g, rank, use_cache, nb, bs, slots):
    from salient_plusplus_amd import fast_sampler as fs
    n = g["rowptr"].shape[0] - 1
    cfg, _idx = _rank_cfg(g, rank, 2, OFFSETS + [n], use_cache, nb, bs, fs)
    sess = fs.Session(2, slots, cfg.to_fast_sampler())
    try:
        assert not sess.native_exchange
        return _drain(sess, False), cfg
    finally:
        sess.close()


@pytest.mark.parametrize("rank,use_cache,nb,bs,slots", [(0, False, 3, 32, 6), (1, True, 7, 16, 4)])
def test_batch_fetch_non_native_distributed_records(rank, use_cache, nb, bs, slots, monkeypatch):
    from oracle import oracle as orc
    from salient_plusplus_amd import fast_sampler as fs
    fs.set_native_comm(None)
    g = _graph()
    monkeypatch.delenv("SPP_GROUP_FETCH", raising=False)
    monkeypatch.delenv("SPP_GROUP_DELIVERY", raising=False)
    want, _ = _bucket_session_records(g, rank, use_cache, nb, bs, slots)
    monkeypatch.setenv("SPP_GROUP_FETCH", "0")
    got, cfg = _bucket_session_records(g, rank, use_cache, nb, bs, slots)
    assert len(got) == nb
    _same_records(got, want, False, f"rank {rank}")
    # and the record itself: P buckets with the counted sizes, cat(buckets ++ cache vertices)[perm] == the oracle's n_id
    idx = cfg.idx.numpy()
    ranges = orc.batch_ranges(len(idx), bs, False, True, nb)
    cv = cfg.cache.cached_vertices.numpy()
    for k, r in enumerate(got):
        m = orc.sample_batch(g["rowptr"], g["col"], idx, int(ranges[k][0]), int(ranges[k][1]), SIZES)
        assert r["x"] is None and r["devices"] == ["cuda"]
        assert [len(t) for t in r["partition_nids"]] + [len(r["cached_nids"])] == list(r["partition_counts"])
        np.testing.assert_array_equal(np.concatenate(r["partition_nids"]), r["partition_nids_flat"])
        ids = np.concatenate(r["partition_nids"] + ([cv[r["cached_nids"]]] if use_cache else []))
        np.testing.assert_array_equal(ids[r["perm_partition_to_mfg"]], m.n_id)
        np.testing.assert_array_equal(r["n_id"], m.n_id)
        np.testing.assert_array_equal(r["sliced_cpu_labels"].reshape(-1), g["y"][m.n_id[:r["idx_range"][1] - r["idx_range"][0]]])
        for (rp, cl, e_shape, ts), hop in zip(r["adjs"], m.hops):
            np.testing.assert_array_equal(rp, hop.rowptr)
            np.testing.assert_array_equal(cl, hop.col)
            assert e_shape == (0,) and ts[0] == len(hop.rowptr) - 1


# ---- (b) the native exchange between two in-process ranks ----
def _native_rank(rank, P, comms, g, offsets, use_cache, nb, bs, slots, compact, errors, out):
    sess = None
    try:
        from oracle import oracle as orc
        from salient_plusplus_amd import fast_sampler as fs
        from salient_plusplus_amd.fast_trainer.samplers import PreparedBatch
        torch.cuda.set_device(0)
        fs.set_native_comm(comms[rank])
        cfg, idx = _rank_cfg(g, rank, P, offsets, use_cache, nb, bs, fs)
        ranges = orc.batch_ranges(len(idx), bs, False, True, nb)
        sess = fs.Session(2, slots, cfg.to_fast_sampler())
        assert sess.native_exchange

        def check(b, k):
            _check_batch(PreparedBatch.from_fast_sampler((b.x, b.sliced_cpu_labels, b.adjs, b.idx_range)), k, ranges, g, idx,
                         g["x"], orc)
        out[rank] = _drain(sess, compact, check)
        assert len(out[rank]) == nb
        sess.close()
    except BaseException as e:  # noqa: BLE001
        import traceback
        errors.append(f"rank {rank}: {e}\n{traceback.format_exc()}")
        if sess is not None:
            sess.close()
        comms[rank].close()     # wakes the peer out of the rendezvous
    finally:
        from salient_plusplus_amd import fast_sampler as fs
        fs.set_native_comm(None)


def _two_ranks(g, use_cache, nb, bs, slots, compact):
    from salient_plusplus_amd import fast_sampler as fs
    P = 2
    offsets = OFFSETS + [g["rowptr"].shape[0] - 1]
    comms = fs.NativeComm.local(P)
    errors, out = [], {}
    ts = [threading.Thread(target=_native_rank, args=(r, P, comms, g, offsets, use_cache, nb, bs, slots, compact, errors, out))
          for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    hung = [t for t in ts if t.is_alive()]
    for c in comms:
        c.close()
    assert not errors, "\n".join(errors)
    assert not hung, "rank thread hung"
    return out


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("P,use_cache,nb,bs,slots", [
    (2, False, 3, 32, 6),       # one group holds all batches
    (2, True, 7, 16, 4),        # several groups, ragged last group, VIP cache
])
def test_batch_fetch_native_exchange_in_process_ranks(P, use_cache, nb, bs, slots, compact, monkeypatch):
    monkeypatch.setenv("SPP_EXCHANGE_ISSUE", "consumer")
    monkeypatch.delenv("SPP_GROUP_DELIVERY", raising=False)
    g = _graph()
    monkeypatch.delenv("SPP_GROUP_FETCH", raising=False)
    want = _two_ranks(g, use_cache, nb, bs, slots, compact)
    monkeypatch.setenv("SPP_GROUP_FETCH", "0")
    got = _two_ranks(g, use_cache, nb, bs, slots, compact)
    for r in range(P):
        _same_records(got[r], want[r], compact, f"rank {r}")
        for rec in got[r]:
            assert rec["x"] is not None
            if compact:          # only what this repository's iterator reads; nothing kept for a reference-shaped consumer
                assert rec["partition_nids"] == [] and rec["partition_nids_flat"] is None and rec["kept"] is None
                assert len(rec["cached_nids"]) == 0 and len(rec["perm_partition_to_mfg"]) == 0
            else:
                assert len(rec["partition_nids"]) == P and rec["kept"] is not None
                np.testing.assert_array_equal(rec["kept"][0], rec["x"])
                np.testing.assert_array_equal(rec["kept"][1], rec["n_id"])
