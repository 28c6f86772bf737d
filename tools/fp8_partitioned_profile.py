"""fp16 versus fp8 (e4m3, per-column scale) PARTITION on a world-size-1 RCCL communicator, S-papers batch shape: the
partitioned delivery pipeline (sampling chain, count all-gather, fused assembly) with every row in the own partition --
it prices the dequantising assembly (k_deliver<16, false, true>) against the fp16 assembly (k_deliver<16>); with one
rank nothing travels, so this says nothing about the exchange.  fp16 and fp8 alternate in one process, three rounds
after warm-up; wall-clock around a whole epoch of 64 batches, device-synchronised.  Kernel times come from a separate run
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fp8_partitioned_profile.py
usage: fp8_partitioned_profile.py [workload=S-papers] [batches=64]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from salient_plusplus_amd import _native as nat  # noqa: E402
from salient_plusplus_amd import fast_sampler as fs  # noqa: E402
from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig  # noqa: E402
from salient_plusplus_amd.fast_trainer.transferers import DeviceDistributedPrefetcher  # noqa: E402
from salient_plusplus_amd.fp8 import quantize_e4m3  # noqa: E402
from salient_plusplus_amd.synthetic import make_workload  # noqa: E402

argv = sys.argv[1:]
name = argv[0] if len(argv) > 0 else "S-papers"
nb = int(argv[1]) if len(argv) > 1 else 64
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
wl = make_workload(name, seed=1234, device=dev)
N, F = wl.x.size(0), wl.x.size(1)
q = quantize_e4m3(wl.x)
tables = {"fp16": q.dequantize(torch.float16), "fp8": q}          # the same values behind both
print(f"FP8_PART_PROFILE workload {name}: {N} rows x {F}, {nb} batches of {wl.batch_size}", flush=True)

L = nat.load()
token = (C.c_uint8 * nat.SPP_COMM_ID_BYTES)()
nat.check(L.spp_comm_unique_id(token))
h = C.c_void_p()
nat.check(L.spp_comm_create(token, 0, 1, 0, C.byref(h)))
fs.set_native_comm(fs.NativeComm(h, 0, 1))
book = fs.RangePartitionBook(0, 1, torch.tensor([0, N]))


def config(table):
    return FastSamplerConfig(
        x_cpu=torch.empty(0), x_gpu=table, y=wl.y.unsqueeze(-1), rowptr=wl.rowptr, col=wl.col,
        idx=wl.train_idx[:nb * wl.batch_size], batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False,
        pin_memory=False, distributed=True, partition_book=book, cache=fs.Cache(), force_exact_num_batches=True,
        exact_num_batches=nb, count_remote_frequency=False, use_cache=False)


def epoch(kind, check=False):
    it = iter(FastSampler(2, 64, config(tables[kind])))
    assert it.session.native_exchange
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = rows = 0
    last = None
    for (b,) in DeviceDistributedPrefetcher([dev], it, True):
        n += 1
        rows += b.x.size(0)
        last = b
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert n == nb and last.x.dtype == torch.float16
    return dt / n * 1e6, rows / n, last


outs = {}
for kind in ("fp16", "fp8"):                       # warm-up (pooled sampler, arenas) and a value check
    _t, _r, outs[kind] = epoch(kind)
assert torch.equal(outs["fp16"].x.view(torch.int16), outs["fp8"].x.view(torch.int16)), "fp8 delivery differs from fp16"
res = {"fp16": [], "fp8": []}
for _round in range(3):
    for kind in ("fp16", "fp8"):
        t, r, _b = epoch(kind)
        res[kind].append(t)
print(f"FP8_PART_PROFILE partitioned pipeline, world 1, {r:.0f} rows / batch (us / batch): "
      + "; ".join(f"{k} " + " ".join(f"{v:.1f}" for v in res[k]) for k in res), flush=True)
fs.set_native_comm(None)
