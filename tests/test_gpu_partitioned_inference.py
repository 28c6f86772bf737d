"""-m gpu: inference.partitioned_layerwise_inference against inference.layerwise_inference over the concatenated table:
every rank's result is the rows [off[r], off[r + 1]) of the unpartitioned one, bit for bit (the aggregation is
bit-identical by contract and the GEMMs run over tiles of one fixed shape, so a node's result depends on its own operand
row alone).  Ranks as threads of one process with LocalPeers (P in {2, 3}), through FastSampler.resident_partition(), and
as two processes on the one GPU with gloo and IpcPeers (HIP IPC mappings, as tests/test_gpu_row_refs_p2p.py)."""
import functools
import os
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, FIN, HID, CLASSES = 2003, 24, 32, 7
OFFSETS = {2: [0, 1100, N], 3: [0, 700, 701, N]}               # (P = 3: rank 1 owns ONE node)


def _graph_host():
    """2 003 nodes, degrees 0..12 and three hubs above C = 64 (one of them 9 C); fp16 features"""
    g = torch.Generator().manual_seed(5)
    deg = torch.randint(0, 13, (N,), generator=g)
    deg[11], deg[700], deg[N - 1] = 65, 3 * 64 + 7, 9 * 64
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    x = torch.randn((N, FIN), generator=g).to(torch.float16)
    return x, rowptr, col


@functools.lru_cache(maxsize=None)
def _graph():
    return tuple(t.cuda() for t in _graph_host())


def _model(kind):
    from salient_plusplus_amd.models import GIN, SAGE
    torch.manual_seed(23)
    if kind == "sage":
        return SAGE(FIN, HID, CLASSES, 3)
    m = GIN(FIN, HID, CLASSES, 2)
    g = torch.Generator().manual_seed(8)
    for mod in m.modules():                                    # non-trivial running statistics and affine terms
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.5)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.0 + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m


@functools.lru_cache(maxsize=None)
def _reference(kind, act_dtype):
    """the unpartitioned result, computed once per model and activation type"""
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    return layerwise_inference(_model(kind).cuda().eval(), x, rowptr, col, act_dtype=act_dtype)


def _partition(x, lo, hi):
    """rows [lo, hi) of x as a rank holds them: an allocation of its own, rows padded by the resident tables' rule (which
    is what gives a ONE-row partition the stride of its peers)"""
    from salient_plusplus_amd import fast_sampler as fs
    se = fs._row_stride_elems(x.size(1), x.element_size())
    part = torch.empty((hi - lo, se), dtype=x.dtype, device=x.device)[:, :x.size(1)]
    part.copy_(x[lo:hi])
    return part


def _nodes_of(off, r):
    """global ids of rank r's range: unsorted, with duplicates, its first and last node among them"""
    lo, hi = off[r], off[r + 1]
    g = torch.Generator().manual_seed(40 + r)
    pick = torch.randint(lo, hi, (min(50, hi - lo),), generator=g)
    return torch.cat([pick, torch.tensor([hi - 1, lo, hi - 1])])


def _run_threads(P, fn):
    """fn(rank) on P threads; the first exception of any rank is raised here"""
    errors, out = [], [None] * P

    def run(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            import traceback
            errors.append(f"rank {r}: {e}\n{traceback.format_exc()}")

    ts = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), "rank(s) hung"
    assert not errors, "\n".join(errors)
    return out


@pytest.mark.parametrize("rows_per_slab", [1 << 20, 97])
@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("kind,P", [("sage", 2), ("sage", 3), ("gin", 3), ("gin", 2)])
def test_ranks_as_threads_equal_the_unpartitioned_rows(kind, P, act_dtype, rows_per_slab):
    from salient_plusplus_amd.inference import LocalPeers, partitioned_layerwise_inference
    x, rowptr, col = _graph()
    want = _reference(kind, act_dtype)
    off = OFFSETS[P]
    model = _model(kind).cuda().eval()                         # one model, read by every rank
    parts = [_partition(x, off[r], off[r + 1]) for r in range(P)]
    for with_nodes in (False, True):
        peers = LocalPeers(P, timeout=60.0)

        def rank(r):
            nodes = _nodes_of(off, r) if with_nodes else None
            return partitioned_layerwise_inference(model, parts[r], rowptr, col, part_offsets=off, rank=r, peers=peers,
                                                   nodes=nodes, rows_per_slab=rows_per_slab, act_dtype=act_dtype)

        got = _run_threads(P, rank)
        for r in range(P):
            rows = want[_nodes_of(off, r).cuda()] if with_nodes else want[off[r]:off[r + 1]]
            assert got[r].dtype == torch.float32 and got[r].shape == rows.shape
            assert torch.equal(got[r].view(torch.int32), rows.view(torch.int32)), (kind, P, r, with_nodes)
    assert not model.training and all(p.grad is None for p in model.parameters())


def test_through_the_sampler_resident_partition():
    """two distributed FastSamplerConfigs (x_gpu + x_cpu halves of each partition) hand out the arguments of the call"""
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.inference import LocalPeers, partitioned_layerwise_inference
    xh, rowptr_h, col_h = _graph_host()
    off = OFFSETS[2]
    want = _reference("sage", torch.float32)
    model = _model("sage").cuda().eval()
    samplers = []
    for r in range(2):
        lo, hi = off[r], off[r + 1]
        cut = lo + (hi - lo) // 3
        cfg = FastSamplerConfig(
            x_cpu=xh[cut:hi].clone(), x_gpu=xh[lo:cut].clone().cuda(), y=torch.zeros((N, 1), dtype=torch.int64),
            rowptr=rowptr_h, col=col_h, idx=torch.arange(lo, hi), batch_size=64, sizes=[5, 5], skip_nonfull_batch=False,
            pin_memory=False, distributed=True, partition_book=fs.RangePartitionBook(r, 2, torch.tensor(off)),
            cache=fs.Cache(), force_exact_num_batches=False, exact_num_batches=0, count_remote_frequency=False,
            use_cache=False)
        samplers.append(FastSampler(2, 4, cfg))
    peers = LocalPeers(2, timeout=60.0)

    def rank(r):
        x_local, rowptr, col, offsets, rk = samplers[r].resident_partition()
        assert rk == r and offsets.tolist() == off and x_local.is_cuda and x_local.shape == (off[r + 1] - off[r], FIN)
        assert rowptr.is_cuda and col.is_cuda
        return partitioned_layerwise_inference(model, x_local, rowptr, col, part_offsets=offsets, rank=rk, peers=peers)

    got = _run_threads(2, rank)
    for r in range(2):
        assert torch.equal(got[r].view(torch.int32), want[off[r]:off[r + 1]].view(torch.int32))
    with pytest.raises(RuntimeError, match="distributed"):
        samplers[0].resident_graph()
    fs.clear_resident_cache()


# ---- two PROCESSES on one GPU: the ranks' partitions and activations reach each other through HIP IPC ---------------
def _ipc_worker(rank, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=2)
        from salient_plusplus_amd.inference import IpcPeers, layerwise_inference, partitioned_layerwise_inference
        x, rowptr, col = _graph()
        off = OFFSETS[2]
        x_local = _partition(x, off[rank], off[rank + 1])
        for kind in ("sage", "gin"):                           # (a failure raises: nothing more is started after it)
            model = _model(kind).cuda().eval()
            want = layerwise_inference(model, x, rowptr, col, act_dtype=torch.bfloat16)
            got = partitioned_layerwise_inference(model, x_local, rowptr, col, part_offsets=off, rank=rank,
                                                  peers=IpcPeers(timeout=60.0), rows_per_slab=500,
                                                  act_dtype=torch.bfloat16)
            assert torch.equal(got.view(torch.int32), want[off[rank]:off[rank + 1]].view(torch.int32)), \
                f"{kind}: rank {rank} differs"
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(f"rank {rank}: {e}\n{traceback.format_exc()}")
        raise


def test_two_processes_through_hip_ipc():
    """SAGE, then GIN, in the same two children (each under a join timeout; a failure is a non-zero exit)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_ipc_worker, args=(r, 29790, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()
    msgs = []
    while not q.empty():
        msgs.append(q.get())
    assert not alive, "rank(s) hung"
    assert all(p.exitcode == 0 for p in procs), "\n".join(msgs)
