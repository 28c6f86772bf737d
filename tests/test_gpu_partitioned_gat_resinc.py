"""-m gpu: inference.partitioned_inference for GAT and SAGEResInception against inference.layerwise_inference over the
concatenated table: every rank's result is the rows [off[r], off[r + 1]) (or its ``nodes``) of the unpartitioned one, bit
for bit -- the attention and the aggregation are bit-identical by contract and the GEMMs run over tiles of one fixed
shape.  Ranks as threads of one process with LocalPeers (P in {2, 3}; rank 1 of 3 owns ONE node), a rank that fails, and
two processes on the one GPU with gloo and IpcPeers (the published views of the wider h buffer pass through HIP IPC)."""
import functools
import os
import sys
import threading
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, FIN, HID, CLASSES = 2003, 24, 32, 7
OFFSETS = {2: [0, 1100, N], 3: [0, 700, 701, N]}               # (P = 3: rank 1 owns ONE node)


def _graph_host():
    """2 003 nodes, degrees 0..12 and three hubs above C_g = 64 (one of them 9 C_g); fp16 features"""
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
    from salient_plusplus_amd.models import GAT, GIN, SAGE, SAGEResInception
    torch.manual_seed(31)
    if kind in ("sage", "gin"):
        return (SAGE if kind == "sage" else GIN)(FIN, HID, CLASSES, 3)
    name, *rest = kind.split("-")
    layers = int(rest[-1][1:])
    if name == "gat":                                          # (h2: the last layer's h, 2 * 7 wide, is narrower than
        return GAT(FIN, HID, CLASSES, layers, heads=int(rest[0][1:]))   # the published buffer; its logits are not)
    m = SAGEResInception(FIN, HID, CLASSES, layers)
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


def _run_threads(P, fn, join=120):
    """fn(rank) on P threads; returns (results, errors by rank)"""
    errors, out = {}, [None] * P

    def run(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errors[r] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(join)
    assert not any(t.is_alive() for t in ts), "rank(s) hung"
    return out, errors


@pytest.mark.parametrize("rows_per_slab", [1 << 20, 97])
@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("kind,P", [("gat-h1-l2", 3), ("gat-h1-l3", 2), ("gat-h2-l2", 2), ("gat-h2-l3", 3),
                                    ("resinc-l2", 3), ("resinc-l3", 2), ("resinc-l3", 3)])
def test_ranks_as_threads_equal_the_unpartitioned_rows(kind, P, act_dtype, rows_per_slab):
    from salient_plusplus_amd.inference import LocalPeers, partitioned_inference
    x, rowptr, col = _graph()
    want = _reference(kind, act_dtype)
    off = OFFSETS[P]
    model = _model(kind).cuda().eval()                         # one model, read by every rank
    parts = [_partition(x, off[r], off[r + 1]) for r in range(P)]
    for with_nodes in (False, True):
        peers = LocalPeers(P, timeout=60.0)

        def rank(r):
            nodes = _nodes_of(off, r) if with_nodes else None
            return partitioned_inference(model, parts[r], rowptr, col, part_offsets=off, rank=r, peers=peers,
                                         nodes=nodes, rows_per_slab=rows_per_slab, act_dtype=act_dtype)

        got, errors = _run_threads(P, rank)
        assert not errors, errors
        for r in range(P):
            rows = want[_nodes_of(off, r).cuda()] if with_nodes else want[off[r]:off[r + 1]]
            assert got[r].dtype == torch.float32 and got[r].shape == rows.shape
            assert torch.equal(got[r].view(torch.int32), rows.view(torch.int32)), (kind, P, r, with_nodes)
    assert not model.training and all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("kind", ["gat-h2-l2", "resinc-l2"])
def test_one_rank_owning_everything_and_the_model_left_in_its_mode(kind):
    """P = 1 (nothing to read from a peer) on a model in training mode: the same bits, and the mode is restored"""
    from salient_plusplus_amd.inference import LocalPeers, partitioned_inference
    x, rowptr, col = _graph()
    model = _model(kind).cuda().train()
    got = partitioned_inference(model, _partition(x, 0, N), rowptr, col, part_offsets=[0, N], rank=0,
                                peers=LocalPeers(1, timeout=5.0), act_dtype=torch.bfloat16)
    assert torch.equal(got.view(torch.int32), _reference(kind, torch.bfloat16).view(torch.int32))
    assert model.training and all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("kind", ["sage", "gin", "gat-h1-l2", "gat-h2-l3", "resinc-l2"])
def test_the_common_entry_is_the_older_entry(kind):
    """``partitioned_layerwise_inference`` is ``partitioned_inference`` for every model the two admit"""
    from salient_plusplus_amd.inference import LocalPeers, partitioned_inference, partitioned_layerwise_inference
    x, rowptr, col = _graph()
    off = OFFSETS[3]
    model = _model(kind).cuda().eval()
    parts = [_partition(x, off[r], off[r + 1]) for r in range(3)]
    results = []
    for entry in (partitioned_inference, partitioned_layerwise_inference):
        peers = LocalPeers(3, timeout=60.0)
        got, errors = _run_threads(3, lambda r: entry(model, parts[r], rowptr, col, part_offsets=off, rank=r,
                                                      peers=peers, act_dtype=torch.bfloat16))
        assert not errors, errors
        results.append(got)
    for r, (a, b) in enumerate(zip(*results)):
        assert a.shape == (off[r + 1] - off[r], CLASSES) and torch.equal(a.view(torch.int32), b.view(torch.int32)), r
    assert not model.training


class _FailingShare:
    """LocalPeers whose ``share`` raises on rank 1: a Python exception, not a device fault"""

    def __init__(self, inner):
        self.inner, self._tls = inner, threading.local()

    def bind(self, rank):
        self._tls.rank = rank
        self.inner.bind(rank)

    def share(self, tensor):
        if self._tls.rank == 1:
            raise KeyError("rank 1 cannot publish")
        return self.inner.share(tensor)

    def barrier(self):
        self.inner.barrier()

    def abort(self):
        self.inner.abort()

    def close(self):
        self.inner.close()


@pytest.mark.parametrize("kind", ["gat-h2-l2", "resinc-l2"])
def test_a_failing_rank_makes_the_other_raise_instead_of_hanging(kind):
    from salient_plusplus_amd.inference import LocalPeers, partitioned_inference
    x, rowptr, col = _graph()
    off = OFFSETS[2]
    model = _model(kind).cuda().eval()
    parts = [_partition(x, off[r], off[r + 1]) for r in range(2)]
    peers = _FailingShare(LocalPeers(2, timeout=5.0))
    t0 = time.monotonic()
    _got, errors = _run_threads(2, lambda r: partitioned_inference(model, parts[r], rowptr, col, part_offsets=off, rank=r,
                                                                   peers=peers), join=30)
    assert time.monotonic() - t0 < 20
    assert isinstance(errors.get(1), KeyError)
    assert isinstance(errors.get(0), RuntimeError) and "another rank failed" in str(errors[0])
    assert not model.training


# ---- two PROCESSES on one GPU: h, the logits and the activations reach each other through HIP IPC -------------------
def _ipc_worker(rank, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=2)
        from salient_plusplus_amd.inference import IpcPeers, layerwise_inference, partitioned_inference
        x, rowptr, col = _graph()
        off = OFFSETS[2]
        x_local = _partition(x, off[rank], off[rank + 1])
        model = _model("gat-h2-l3").cuda().eval()
        want = layerwise_inference(model, x, rowptr, col, act_dtype=torch.bfloat16)
        got = partitioned_inference(model, x_local, rowptr, col, part_offsets=off, rank=rank,
                                    peers=IpcPeers(timeout=60.0), rows_per_slab=500, act_dtype=torch.bfloat16)
        assert torch.equal(got.view(torch.int32), want[off[rank]:off[rank + 1]].view(torch.int32)), \
            f"rank {rank} differs"
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(f"rank {rank}: {e}\n{traceback.format_exc()}")
        raise


def test_two_processes_through_hip_ipc():
    """GAT with two heads in bf16 at P = 2, in two fresh children (each under a join timeout; a failure is a non-zero
    exit)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_ipc_worker, args=(r, 29794, q)) for r in range(2)]
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
