"""fp16 versus fp8 (e4m3, per-column scale) feature table on the resident S-papers batch shape of model_step_profile.py:
the lone row delivery x = table[n_id] (plain gather against the dequantising gather), a whole delivery pipeline epoch,
and the SAGE and GIN optimisation step with table_features=True (first layer reads the table in place).  fp16 and fp8
alternate in one process, three rounds after warm-up; wall-clock around stream-synchronised loops.  Kernel times come from
a separate run under the profiler:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fp8_feature_profile.py
usage: fp8_feature_profile.py [workload=S-papers] [reps=50] [steps=20]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from salient_plusplus_amd import fast_sampler as fs  # noqa: E402
from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig  # noqa: E402
from salient_plusplus_amd.fast_trainer.transferers import DevicePrefetcher  # noqa: E402
from salient_plusplus_amd.fp8 import quantize_e4m3  # noqa: E402
from salient_plusplus_amd.models import get_model_type  # noqa: E402
from salient_plusplus_amd.synthetic import make_workload  # noqa: E402

argv = sys.argv[1:]
name = argv[0] if len(argv) > 0 else "S-papers"
reps = int(argv[1]) if len(argv) > 1 else 50
steps = int(argv[2]) if len(argv) > 2 else 20
dev = torch.device("cuda", 0)
wl = make_workload(name, seed=1234, device=dev)
F = wl.x.size(1)
tables = {"fp16": wl.x, "fp8": quantize_e4m3(wl.x)}
print(f"FP8_PROFILE workload {name}: {wl.x.size(0)} rows x {F}; table fp16 {wl.x.numel() * 2 / 2**30:.2f} GiB, "
      f"fp8 {wl.x.numel() / 2**30:.2f} GiB", flush=True)


def config(table, n_batches):
    return FastSamplerConfig(
        x_cpu=table, x_gpu=torch.empty(0), y=wl.y.unsqueeze(-1), rowptr=wl.rowptr, col=wl.col,
        idx=wl.train_idx[:n_batches * wl.batch_size], batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False,
        pin_memory=False, distributed=False, partition_book=None, cache=fs.Cache(), force_exact_num_batches=True,
        exact_num_batches=n_batches, count_remote_frequency=False, use_cache=False)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


# the resident batch (model_step_profile.py's), as TableRows over either table: same n_id, same hops
rows = {}
for kind, table in tables.items():
    it = DevicePrefetcher([dev], iter(FastSampler(2, 8, config(table, 8), table_features=True)))
    rows[kind] = next(it)[0]
    del it
torch.cuda.synchronize()
assert torch.equal(rows["fp16"].x.n_id, rows["fp8"].x.n_id)
U = rows["fp16"].x.n_id.numel()
print(f"FP8_PROFILE resident batch: {U} rows, {[int(a.adj_t.nnz()) for a in rows['fp16'].adjs]} edges", flush=True)


def epoch(table):
    n = 0
    for (_b,) in DevicePrefetcher([dev], iter(FastSampler(2, 64, config(table, 64)))):
        n += 1
    assert n == 64


models, opts = {}, {}
for arch in ("sage", "gin"):
    torch.manual_seed(0)
    models[arch] = get_model_type(arch)(F, 256, 47, 3).to(dev)
    opts[arch] = torch.optim.Adam(models[arch].parameters(), lr=1e-3, fused=True)


def step(arch, batch):
    def fn():
        opts[arch].zero_grad(set_to_none=True)
        loss = torch.nn.functional.nll_loss(models[arch](batch.x, batch.adjs), batch.y.reshape(-1))
        loss.backward()
        opts[arch].step()
    return fn


legs = [("lone delivery x = table[n_id] (us)", lambda k: timed(rows[k].x.materialize, reps) * 1e6),
        ("pipeline, 64 batches (us / batch)", lambda k: timed(lambda: epoch(tables[k]), 1) / 64 * 1e6),
        ("SAGE step, table_features (us)", lambda k: timed(step("sage", rows[k]), steps) * 1e6),
        ("GIN step, table_features (us)", lambda k: timed(step("gin", rows[k]), steps) * 1e6)]
for title, leg in legs:
    for kind in ("fp16", "fp8"):                   # warm-up
        leg(kind)
    res = {"fp16": [], "fp8": []}
    for _round in range(3):
        for kind in ("fp16", "fp8"):
            res[kind].append(leg(kind))
    print(f"FP8_PROFILE {title}: " + "; ".join(f"{k} " + " ".join(f"{v:.1f}" for v in res[k]) for k in res), flush=True)
