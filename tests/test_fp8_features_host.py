"""CPU-only: the fp8 (e4m3, per-column power-of-two scale) feature table of salient_plusplus_amd.fp8 -- the definitions the
GPU kernels are tested against (tests/test_gpu_fp8_features.py) and the construction-time scope checks of the façade."""
import os

import pytest
import torch

from salient_plusplus_amd import fast_sampler as fs
from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
from salient_plusplus_amd.fp8 import Fp8Features, load, quantize_e4m3, save

FP8 = torch.float8_e4m3fn


def _codes(q):
    return q.view(torch.uint8)


def _table(n=300, F=32, seed=0, dtype=torch.float16):
    """random rows with the adversarial columns: all zero, one huge value, tiny values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F, generator=g) * torch.logspace(-3, 3, F)
    x[:, 3] = 0.0
    x[:, 5] = torch.randn(n, generator=g) * 1e-2
    x[n // 2, 5] = 60000.0
    x[:, 7] = torch.randn(n, generator=g) * 6e-8
    return x.to(dtype)


def test_all_256_codes_dequantize_as_torch_does():
    codes = torch.arange(256, dtype=torch.uint8).reshape(16, 16)
    f = Fp8Features(codes.view(FP8), torch.zeros(16, dtype=torch.int8))
    want = codes.view(FP8).to(torch.float32)
    got = f.dequantize(torch.float32)
    assert got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32)[~want.isnan()], want.view(torch.int32)[~want.isnan()])
    assert torch.equal(got.isnan(), want.isnan()) and int(want.isnan().sum()) == 2          # 0x7F and 0xFF only
    # with a scale: exactly float32(code) * 2^e
    for e in (-64, -7, 5, 63):
        fe = Fp8Features(codes.view(FP8), torch.full((16,), e, dtype=torch.int8))
        w = torch.ldexp(want.double(), torch.tensor(e)).float()                                # exact in fp64, exact in fp32
        ok = ~want.isnan()
        assert torch.equal(fe.dequantize(torch.float32)[ok], w[ok])
    # the fp16 value is v rounded once
    assert torch.equal(f.dequantize()[~want.isnan()], want.to(torch.float16)[~want.isnan()])


def test_quantiser_never_emits_a_nan_code():
    # every finite fp16 value, each in a column of its own kind of company
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    allh = bits.view(torch.float16)
    allh = allh[torch.isfinite(allh)]
    allh = torch.cat([allh, allh.new_zeros((-allh.numel()) % 16)]).reshape(-1, 16)
    for x in (allh, allh.t().contiguous()[:, :allh.size(0) // 16 * 16], _table(), _table(dtype=torch.float32),
              _table(dtype=torch.bfloat16)):
        c = _codes(quantize_e4m3(x).q)
        assert not bool(((c & 0x7F) == 0x7F).any())
    # what the clamp is for: torch's cast does not saturate
    assert torch.tensor([500.0]).to(FP8).view(torch.uint8).item() & 0x7F == 0x7F


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quantiser_bounds(dtype, seed):
    x = _table(seed=seed, dtype=dtype)
    f = quantize_e4m3(x)
    e = f.scale_log2.to(torch.int32)
    assert f.q.dtype == FP8 and f.scale_log2.dtype == torch.int8 and f.shape == x.shape
    assert int(e.abs().max()) <= 64 and int(e[3]) == 0
    v = f.dequantize(torch.float32).double()
    assert not bool(v.isnan().any())
    qs = f.q.to(torch.float32).double()                       # q = v * 2^-e
    assert float(qs.abs().max()) <= 448.0
    # Error bound per element, |v - x| <= max(2^-4 |x|, 2^(e-10)):
    #  * x / 2^e lies in [-448, 448] (the scale rule) and is rounded to the nearest e4m3 value.  A NORMAL e4m3 value in
    #    [2^k, 2^(k+1)) has 3 mantissa bits, so neighbours are 2^(k-3) apart and the rounding error is at most half of
    #    that, 2^(k-4) <= 2^-4 |x / 2^e|; multiplied by 2^e: 2^-4 |x|.
    #  * below the smallest normal (2^-6) the e4m3 values are the multiples of 2^-9 (subnormals), so the error is at most
    #    2^-10; multiplied by 2^e: 2^(e-10).
    xd = x.double()
    bound = torch.maximum(xd.abs() / 16, torch.ldexp(torch.ones_like(xd), (e - 10).expand_as(xd)))
    err = (v - xd).abs()
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max())}"
    # the scale is the SMALLEST admissible exponent: half of it would overflow 448 (unless clamped at -64 / all zero)
    m = xd.abs().amax(0)
    tight = (m > torch.ldexp(torch.full_like(m, 448.0), e - 1)) | (e == -64) | (m == 0)
    assert bool(tight.all())


def test_quantiser_is_idempotent_on_its_own_output():
    """quantize(dequantize(f)) reproduces the VALUES always, and (q, scale_log2) whenever f is in the quantiser's canonical
    form.  The scale rule makes a column's largest |q| land in (224, 448]; a maximum that ROUNDS DOWN to exactly 224
    (x / 2^e in (224, 232]) is the one exception: its value 224 * 2^e is re-encoded as 448 * 2^(e-1) -- the same numbers
    with every code doubled, which the rule ceil(log2(max / 448)) demands.  Both statements are asserted."""
    for seed in range(4):
        f = quantize_e4m3(_table(seed=seed))
        v = f.dequantize(torch.float32)
        g = quantize_e4m3(v)
        assert torch.equal(g.dequantize(torch.float32), v)
        qmax = f.q.to(torch.float32).abs().amax(0)
        canon = ((qmax > 224) | (f.scale_log2 == -64)) & (qmax > 0)
        assert int(canon.sum()) >= f.shape[1] - 4
        assert torch.equal(g.scale_log2[canon], f.scale_log2[canon])
        assert torch.equal(_codes(g.q)[:, canon], _codes(f.q)[:, canon])
    # the exception, made on purpose: max 225 -> code for 224, scale 0; re-quantised: 448 at scale -1
    x = torch.zeros(4, 16)
    x[0, :] = 225.0
    x[1, :] = 3.0
    f = quantize_e4m3(x)
    assert int(f.scale_log2[0]) == 0 and float(f.dequantize(torch.float32)[0, 0]) == 224.0
    g = quantize_e4m3(f.dequantize(torch.float32))
    assert int(g.scale_log2[0]) == -1 and torch.equal(g.dequantize(torch.float32), f.dequantize(torch.float32))
    assert torch.equal(quantize_e4m3(g.dequantize(torch.float32)).q.view(torch.uint8), g.q.view(torch.uint8))


def test_quantiser_rejects_bad_input(tmp_path):
    with pytest.raises(ValueError):
        quantize_e4m3(torch.zeros(4, 100, dtype=torch.float16))            # F % 16 != 0
    with pytest.raises(ValueError):
        Fp8Features(torch.zeros(4, 24, dtype=torch.uint8).view(FP8), torch.zeros(24, dtype=torch.int8))
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = torch.ones(4, 16)
        x[2, 3] = bad
        with pytest.raises(ValueError):
            quantize_e4m3(x)
    with pytest.raises(ValueError):
        Fp8Features(torch.zeros(4, 16, dtype=torch.uint8).view(FP8), torch.full((16,), 64, dtype=torch.int8))
    with pytest.raises(ValueError):
        Fp8Features(torch.zeros(4, 16, dtype=torch.uint8).view(FP8), torch.zeros(8, dtype=torch.int8))


def test_save_load_round_trip_and_accessors(tmp_path):
    f = quantize_e4m3(_table())
    p = os.path.join(tmp_path, "t.fp8")
    save(f, p)
    g = load(p)
    assert torch.equal(_codes(g.q), _codes(f.q)) and torch.equal(g.scale_log2, f.scale_log2)
    f.save(p)
    g = Fp8Features.load(p)
    assert torch.equal(_codes(g.q), _codes(f.q))
    assert f.dim() == 2 and f.size() == f.shape == torch.Size((300, 32)) and f.size(1) == 32 and f.numel() == 300 * 32
    assert f.device == torch.device("cpu") and not f.is_cuda and f.dtype == FP8
    h = f.to("cpu")
    assert torch.equal(_codes(h.q), _codes(f.q))
    r = f.rows(torch.tensor([5, 1, 5]))
    assert torch.equal(r.dequantize(torch.float32), f.dequantize(torch.float32)[[5, 1, 5]])
    assert f.q.stride() == (32, 1)
    with pytest.raises(ValueError):
        torch.save({"q": 1}, p)
        load(p)


def _cfg(x, **kw):
    n = x.size(0)
    base = dict(x_cpu=x, x_gpu=torch.empty(0), y=torch.zeros(n, 1, dtype=torch.int64), rowptr=torch.zeros(n + 1, dtype=torch.int64),
                col=torch.zeros(0, dtype=torch.int64), idx=torch.arange(4), batch_size=2, sizes=[2], skip_nonfull_batch=False,
                pin_memory=False, distributed=False, partition_book=None, cache=fs.Cache(), force_exact_num_batches=False,
                exact_num_batches=0, count_remote_frequency=False, use_cache=False)
    base.update(kw)
    return FastSamplerConfig(**base)


def test_fp8_table_outside_its_scope_is_refused_at_construction(monkeypatch):
    f = quantize_e4m3(_table(n=16))
    cfg = _cfg(f)                                              # in scope: constructs, converts, counts
    assert cfg.get_num_batches() == 2 and isinstance(cfg.to_fast_sampler().x_cpu, Fp8Features)
    FastSampler(1, 2, cfg)
    with pytest.raises(RuntimeError, match="distributed"):
        _cfg(f, distributed=True, partition_book=fs.RangePartitionBook(0, 1, torch.tensor([0, 16])))
    with pytest.raises(RuntimeError, match="cache"):
        _cfg(f, use_cache=True)
    with pytest.raises(RuntimeError, match="cache"):
        _cfg(f, cache=fs.Cache(0, 1, torch.tensor([1, 2]), torch.zeros(2, 32, dtype=torch.float16)))
    with pytest.raises(RuntimeError, match="row_refs"):
        FastSampler(1, 2, cfg, row_refs=True)
    with pytest.raises(RuntimeError, match="x_cpu"):
        _cfg(torch.zeros(16, 32, dtype=torch.float16), x_gpu=f)
    # the native-shaped Config is checked by the Session before any device call
    native = fs.Config()
    native.x_cpu, native.distributed = f, True
    with pytest.raises(RuntimeError, match="distributed"):
        fs.Session(1, 1, native)
    # the P2P transport is a mode of the distributed path only, so there is no P2P-specific refusal: asking for it
    # meets the refusal of distributed=True
    monkeypatch.setenv("SPP_DIST_TRANSPORT", "p2p")
    with pytest.raises(RuntimeError, match="distributed"):
        fs.Session(1, 1, native)
