"""Host side of fp8 feature tables on the partitioned path (no GPU): shared per-column exponents
(fp8.column_scales / quantize_e4m3(x, scale_log2=...)), the configuration a rank hands over
(x_gpu=Fp8Features, optional Fp8Features VIP cache), the refusals of everything the native exchange does not
serve -- all raised at construction, before any device call -- and the appended spp_exchange_cfg fields."""
import ctypes
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
from salient_plusplus_amd import fp8  # noqa: E402
from salient_plusplus_amd.fast_trainer import vip_cache  # noqa: E402
from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig  # noqa: E402
from salient_plusplus_amd.fp8 import Fp8Features, column_scales, quantize_e4m3  # noqa: E402

N = 3000


def _table(F):
    return torch.from_numpy(np.random.default_rng(7).standard_normal((N, F)).astype(np.float16))


def _codes(f):
    return f.q.view(torch.uint8)


@pytest.mark.parametrize("F", [16, 48])
def test_slice_quantised_against_the_table_scales_equals_rows_of_the_table(F):
    x = _table(F)
    x[:, 3] *= 300.0                      # columns of different magnitude: exponents differ
    x[:, 5] *= 2.0 ** -9
    x[:, 7] = 0                           # an all-zero column: exponent 0
    full = quantize_e4m3(x)
    e = column_scales(x)
    assert e.dtype == torch.int8 and e.shape == (F,) and torch.equal(e, full.scale_log2)
    assert len(set(e.tolist())) >= 3 and int(e[7]) == 0
    for a, b in ((0, 1400), (1400, N), (900, 2100), (17, 18), (5, 5)):
        part = quantize_e4m3(x[a:b], scale_log2=e)
        assert torch.equal(part.scale_log2, e)
        assert torch.equal(_codes(part), _codes(full.rows(slice(a, b))))
    # a slice alone would choose other exponents somewhere: the given ones really are used
    alone = quantize_e4m3(x[:40])
    assert not torch.equal(alone.scale_log2, e)
    assert torch.equal(_codes(quantize_e4m3(x[:40], scale_log2=e)), _codes(full.rows(slice(0, 40))))
    # int32 exponents (what an all-reduce works on) are accepted
    assert torch.equal(_codes(quantize_e4m3(x[:40], scale_log2=e.to(torch.int32))), _codes(full.rows(slice(0, 40))))
    # the element-wise maximum of the parts' exponents is the table's (the documented all-reduce recipe)
    parts = torch.stack([column_scales(x[a:b]) for a, b in ((0, 1400), (1400, N))])
    assert torch.equal(parts.amax(0)[e != 0], e[e != 0])


def test_given_scales_overflow_and_range_are_rejected():
    x = _table(16)
    e = column_scales(x)
    too_small = e.clone()
    too_small[4] -= 1                     # the column's maximum now lands above 448
    with pytest.raises(ValueError, match="overflow"):
        quantize_e4m3(x, scale_log2=too_small)
    quantize_e4m3(x, scale_log2=e + 1)    # larger exponents only lose precision
    for bad in (torch.full((16,), 64, dtype=torch.int8), torch.full((16,), -65, dtype=torch.int8),
                torch.full((16,), 200, dtype=torch.int32)):
        with pytest.raises(ValueError, match="scale_log2"):
            quantize_e4m3(x, scale_log2=bad)
    with pytest.raises(ValueError):
        quantize_e4m3(x, scale_log2=e[:8])                          # one exponent per column
    with pytest.raises(ValueError):
        quantize_e4m3(x, scale_log2=e.to(torch.float32))            # integers
    bad = x.clone()
    bad[3, 3] = float("nan")
    with pytest.raises(ValueError):
        quantize_e4m3(bad, scale_log2=e)
    with pytest.raises(ValueError):
        column_scales(bad)


def _cfg(part, P=2, rank=0, **kw):
    offs = torch.tensor([0, 1400, N] if P == 2 else [0, N])
    base = dict(x_cpu=torch.empty(0), x_gpu=part, y=torch.zeros(N, 1, dtype=torch.int64),
                rowptr=torch.zeros(N + 1, dtype=torch.int64), col=torch.zeros(0, dtype=torch.int64), idx=torch.arange(8),
                batch_size=2, sizes=[2], skip_nonfull_batch=False, pin_memory=False, distributed=True,
                partition_book=fs.RangePartitionBook(rank, P, offs), cache=fs.Cache(), force_exact_num_batches=True,
                exact_num_batches=4, count_remote_frequency=False, use_cache=False)
    base.update(kw)
    return FastSamplerConfig(**base)


def test_partitioned_configuration_constructs_and_keeps_the_fp8_tables():
    full = quantize_e4m3(_table(48))
    part = full.rows(slice(0, 1400))
    cfg = _cfg(part)
    native = cfg.to_fast_sampler()
    assert native.x_gpu is part and isinstance(native.x_gpu, Fp8Features) and native.distributed
    FastSampler(1, 2, cfg)
    cv = torch.tensor([1500, 1700, 2999])
    cache = fs.Cache(0, 2, cv, full.rows(cv))
    cfg = _cfg(part, cache=cache, use_cache=True)
    native = cfg.to_fast_sampler()
    assert isinstance(native.x_gpu, Fp8Features) and isinstance(native.cache.cached_features, Fp8Features)
    assert native.use_cache and fs.fp8_session_check(cfg) is False      # True is the single-GPU x_cpu table
    FastSampler(1, 2, cfg)


def test_cache_with_other_scales_or_width_is_refused():
    x = _table(48)
    full = quantize_e4m3(x)
    part = full.rows(slice(0, 1400))
    cv = torch.tensor([1500, 1700, 2999])
    e = full.scale_log2.clone()
    e[11] += 1
    with pytest.raises(RuntimeError, match="scales"):
        _cfg(part, cache=fs.Cache(0, 2, cv, quantize_e4m3(x[cv], scale_log2=e)), use_cache=True)
    with pytest.raises(RuntimeError, match="width"):
        _cfg(part, cache=fs.Cache(0, 2, cv, quantize_e4m3(_table(16)).rows(cv)), use_cache=True)
    with pytest.raises(RuntimeError, match="cache"):                     # fp16 rows in the cache of an fp8 partition
        _cfg(part, cache=fs.Cache(0, 2, cv, x[cv]), use_cache=True)
    # the native-shaped Config meets the same check in the Session, before any device call
    native = _cfg(part).to_fast_sampler()
    native.cache, native.use_cache = fs.Cache(0, 2, cv, quantize_e4m3(x[cv], scale_log2=e)), True
    with pytest.raises(RuntimeError, match="scales"):
        fs.Session(1, 2, native)


def test_modes_the_native_exchange_does_not_serve_are_refused(monkeypatch):
    for k in ("SPP_DIST_TRANSPORT", "SPP_ROW_REFS", "SPP_TABLE_FEATURES"):
        monkeypatch.delenv(k, raising=False)
    part = quantize_e4m3(_table(16)).rows(slice(0, 1400))
    cfg = _cfg(part)
    native = cfg.to_fast_sampler()
    fs.set_native_comm(None)
    # no native communicator (no process group, nothing pinned): today's fallback is the torch-collective prefetcher
    with pytest.raises(RuntimeError, match="torch-collective"):
        fs.Session(1, 2, native)
    # a pinned communicator of another shape than the partition book
    fs.set_native_comm(fs.NativeComm(None, 0, 3))
    try:
        with pytest.raises(RuntimeError, match="no native communicator"):
            fs.Session(1, 2, native)
    finally:
        fs.set_native_comm(None)
    monkeypatch.setenv("SPP_DIST_TRANSPORT", "torch")
    with pytest.raises(RuntimeError, match="SPP_DIST_TRANSPORT=torch"):
        fs.Session(1, 2, native)
    monkeypatch.setenv("SPP_DIST_TRANSPORT", "p2p")
    with pytest.raises(RuntimeError, match="(?i)p2p"):
        fs.Session(1, 2, native)
    monkeypatch.delenv("SPP_DIST_TRANSPORT")
    with pytest.raises(RuntimeError, match="row_refs"):
        FastSampler(1, 2, cfg, row_refs=True)
    with pytest.raises(RuntimeError, match="table_features"):
        FastSampler(1, 2, cfg, table_features=True)
    monkeypatch.setenv("SPP_ROW_REFS", "1")
    with pytest.raises(RuntimeError, match="row_refs"):
        fs.Session(1, 2, native)
    monkeypatch.delenv("SPP_ROW_REFS")
    monkeypatch.setenv("SPP_TABLE_FEATURES", "1")
    with pytest.raises(RuntimeError, match="table_features"):
        fs.Session(1, 2, native)
    monkeypatch.delenv("SPP_TABLE_FEATURES")
    # x_gpu next to host rows, or without distributed=True: the spelling is wrong
    with pytest.raises(RuntimeError, match="x_cpu"):
        _cfg(part, x_cpu=torch.zeros(4, 16, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="x_cpu"):
        _cfg(part, distributed=False, partition_book=None)
    # ... and the single-GPU spelling on a distributed session names the one to use
    with pytest.raises(RuntimeError, match="distributed.*x_gpu"):
        _cfg(torch.empty(0), x_cpu=part)
    # the cache-row fetch moves typed torch tensors: an fp8 partition is refused with a message
    with pytest.raises(RuntimeError, match="fp8 partition"):
        vip_cache.fetch_cache_rows(fs.RangePartitionBook(0, 2, torch.tensor([0, 1400, N])), torch.tensor([1500]), part)


def test_exchange_cfg_grew_and_a_zero_tail_is_not_fp8():
    fields = [n for n, _t in nat.ExchangeCfg._fields_]
    assert fields[-3:] == ["x_elem", "scale_log2_dev", "scales_tag"]
    before = ctypes.sizeof(type("Old", (ctypes.Structure,), {"_fields_": nat.ExchangeCfg._fields_[:-3]}))
    # (x_elem takes the padding behind issue_on_consumer; the pointer and the tag are new bytes)
    assert ctypes.sizeof(nat.ExchangeCfg) == before + 16
    assert nat.ExchangeCfg.x_elem.offset == nat.ExchangeCfg.issue_on_consumer.offset + 4 == before - 4
    assert nat.ExchangeCfg.scale_log2_dev.offset == before and nat.ExchangeCfg.scales_tag.offset == before + 8
    xc = nat.ExchangeCfg()                                              # ctypes zero-fills
    assert xc.x_elem == 0 != nat.SPP_ELEM_FP8_E4M3 and not xc.scale_log2_dev and xc.scales_tag == 0
    assert xc.x_elem in (nat.SPP_ELEM_F32, nat.SPP_ELEM_F16, nat.SPP_ELEM_BF16)     # "bytes, as today"
    # the tag: FNV-1a 64 of the exponent bytes, never the "not fp8" value
    e = torch.tensor([0, -1, 5, 63, -64] + [0] * 11, dtype=torch.int8)
    h = 0xcbf29ce484222325
    for b in e.numpy().tobytes():
        h = ((h ^ b) * 0x100000001b3) % (1 << 64)
    assert fs.fp8_scales_tag(e) == h != 0
    e2 = e.clone()
    e2[9] += 1
    assert fs.fp8_scales_tag(e2) != fs.fp8_scales_tag(e)
