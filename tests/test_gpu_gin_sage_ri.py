"""GPU: GINConv's sum aggregation (csrc/aggregate.hip k_csr_sum_*) against an fp32 index_add_ restatement, and the
GIN / SAGEResInception models (driver/models.py:95-283) against torch-only restatements of the reference modules
loaded from the same state dict.  Tolerances of the kernels as in test_gpu_model_step.py: forward 1e-5 (fp32 sums in
another order), backward 1e-4 (atomics / another order)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SIZES = [15, 10, 5]


# ---------------------------------------------------------------------------------------------- restatements
def _ref_sum(x, rowptr, col, T, s):
    cnt = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(T, device=x.device), cnt)
    xf = x if x.dtype == torch.float64 else x.float()
    return torch.zeros((T, x.size(1)), dtype=xf.dtype, device=x.device).index_add_(0, row, xf[col]) + s * xf[:T]


def _seq_sum(x, rowptr, col, T, s):
    """the kernels' exact arithmetic for an s with s * x exact in fp32 (then fmaf(s, x_t, acc) is one add of that
    product): each row's entries summed in fp32 in CSR order, one at a time, then s * x_t added"""
    deg = rowptr[1:] - rowptr[:-1]
    xf = x.float()
    acc = torch.zeros((T, x.size(1)), dtype=torch.float32, device=x.device)
    for k in range(int(deg.max()) if T else 0):
        on = k < deg
        acc = acc + torch.where(on.unsqueeze(-1), xf[col[torch.where(on, rowptr[:-1] + k, 0)]], 0.0)
    return acc + xf[:T] * s if s else acc


def _ref_mean(x, rowptr, col, T):
    cnt = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(T, device=x.device), cnt)
    out = torch.zeros((T, x.size(1)), dtype=torch.float32, device=x.device).index_add_(0, row, x.float()[col])
    return out / cnt.clamp(min=1).unsqueeze(-1).float()


class RefGINConv(torch.nn.Module):
    """PyG GINConv(nn, eps=0, train_eps=False): nn(sum_j x_j + (1 + eps) x_target)"""

    def __init__(self, nn):
        super().__init__()
        self.nn = nn
        self.register_buffer("eps", torch.zeros(1))

    def forward(self, x_pair, adj_t):
        x, x_t = x_pair
        rowptr, col, _ = adj_t.csr()
        return self.nn(_ref_sum(x, rowptr, col, x_t.size(0), 0.0) + (1 + self.eps) * x_t)


class RefGIN(torch.nn.Module):
    def __init__(self, i, h, o, L, p):
        super().__init__()
        mk = lambda d: torch.nn.Sequential(torch.nn.Linear(d, h), torch.nn.BatchNorm1d(h), torch.nn.ReLU(),  # noqa: E731
                                           torch.nn.Linear(h, h), torch.nn.ReLU())
        self.convs = torch.nn.ModuleList([RefGINConv(mk(i if k == 0 else h)) for k in range(L)])
        self.lin1, self.lin2, self.p = torch.nn.Linear(h, h), torch.nn.Linear(h, o), p

    def forward(self, x, adjs):
        x = x.to(torch.float)
        for k, (adj_t, _, size) in enumerate(adjs):
            x = self.convs[k]((x, x[:size[1]]), adj_t)
        x = F.dropout(self.lin1(x).relu(), p=self.p, training=self.training)
        return torch.log_softmax(self.lin2(x), dim=-1)


class RefSAGEConv(torch.nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.lin_l = torch.nn.Linear(i, o, bias=False)
        self.lin_r = torch.nn.Linear(i, o, bias=False)

    def forward(self, x_pair, adj_t):
        x, x_t = x_pair
        rowptr, col, _ = adj_t.csr()
        return self.lin_l(_ref_mean(x, rowptr, col, x_t.size(0))) + self.lin_r(x_t)


class RefMLP(torch.nn.Module):
    def __init__(self, i, h, o):
        super().__init__()
        self.module_list = torch.nn.Sequential(torch.nn.Linear(i, h), torch.nn.Linear(h, o))

    def forward(self, x):
        return self.module_list(x)


class RefSAGERI(torch.nn.Module):
    """driver/models.py:128-192 as written, the in-place residual add through the collected view included"""

    def __init__(self, i, h, o, L, p):
        super().__init__()
        self.convs = torch.nn.ModuleList([RefSAGEConv(i if k == 0 else h, h) for k in range(L)])
        self.bns = torch.nn.ModuleList([torch.nn.BatchNorm1d(h) for _ in range(L)])
        self.res_linears = torch.nn.ModuleList([torch.nn.Linear(i, h)] + [torch.nn.Identity() for _ in range(L - 1)])
        self.mlp = RefMLP(i + h * L, 2 * o, o)
        self.p = p

    def forward(self, _x, adjs):
        p, tr = self.p, self.training
        _x = _x.to(torch.float)
        collect = []
        end_size = adjs[-1][-1][1]
        x = F.dropout(_x, p=p, training=tr)
        collect.append(x[:end_size])
        for k, (adj_t, _, size) in enumerate(adjs):
            x_target = x[:size[1]]
            x = self.convs[k]((F.dropout(x, p=p, training=tr), F.dropout(x_target, p=p, training=tr)), adj_t)
            x = self.bns[k](x)
            x = F.leaky_relu(x)
            x = F.dropout(x, p=p, training=tr)
            collect.append(x[:end_size])
            x += self.res_linears[k](x_target)
        return torch.log_softmax(self.mlp(torch.cat(collect, -1)), dim=-1)


# ---------------------------------------------------------------------------------------------- helpers
def _hop(T, S, maxdeg, seed, hub=0, dup=False):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, maxdeg + 1, (T,), generator=g)
    deg[::7] = 0                                             # empty rows
    if hub and T > 1:
        deg[1] = hub                                         # one hub row
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    col = torch.randint(0, S, (E,), generator=g)
    if dup and E > 4:
        col[1::3] = col[0:E - 1:3][:col[1::3].numel()]       # repeated columns within rows
        col[2::5] = torch.randint(0, max(T, 1), (col[2::5].numel(),), generator=g)   # self / target edges
    return rowptr.cuda(), col.cuda()


def _close(a, b, rtol, what=""):
    """relative to the reference's scale (gradients of a deep stack span magnitudes); the 1e-8 floor covers gradients
    that are zero up to rounding (the bias of a Linear in front of a training-mode BatchNorm)"""
    atol = rtol * float(b.abs().max()) + 1e-8 if b.numel() else 0.0
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def _check_sum(got, x, rowptr, col, T, s, rel=1e-5):
    """against fp64, within rel x the sum of the magnitudes of the row's terms (the error of an fp32 sum in any order
    grows with the row's length: one hub row of 4500 terms differs by ~1e-4 between two orders)"""
    want = _ref_sum(x.double(), rowptr, col, T, s)
    bound = _ref_sum(x.double().abs(), rowptr, col, T, abs(s))
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = (got.double() - want).abs()
    assert bool((err <= rel * bound + 1e-6).all()), float((err - rel * bound).max())


def _batches(F_, n_batches=3, seed=0, **kw):
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.fast_trainer.transferers import DevicePrefetcher
    g = np.load(os.path.join(ROOT, "tests", "golden", "graph_a.npz"))
    T_ = torch.from_numpy
    n = g["rowptr"].shape[0] - 1
    x = T_((np.random.default_rng(seed).standard_normal((n, F_))).astype(np.float16))
    cfg = FastSamplerConfig(
        x_cpu=x, x_gpu=torch.empty(0), y=T_(g["y"]).unsqueeze(-1), rowptr=T_(g["rowptr"]), col=T_(g["col"]),
        idx=T_(g["idx"]), batch_size=64, sizes=SIZES, skip_nonfull_batch=False, pin_memory=False, distributed=False,
        partition_book=None, cache=fs.Cache(), force_exact_num_batches=True, exact_num_batches=n_batches,
        count_remote_frequency=False, use_cache=False)
    dev = torch.device("cuda", 0)
    out = [b for (b,) in DevicePrefetcher([dev], iter(FastSampler(2, 4, cfg, **kw)))]
    torch.cuda.synchronize()
    return out, int(g["y"].max()) + 1


def _step(model, x, adjs, y):
    model.zero_grad(set_to_none=True)
    out = model(x, adjs)
    loss = F.nll_loss(out, y.reshape(-1))
    loss.backward()
    return out.detach(), loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("eps", [0.0, 0.5])
@pytest.mark.parametrize("F_,dtype", [(3, torch.float16), (47, torch.float32), (100, torch.float16),
                                      (128, torch.float16), (256, torch.float32), (1024, torch.float32)])
def test_sum_aggregate_forward_backward(F_, dtype, eps):
    from salient_plusplus_amd.models import sum_aggregate
    T, S = 2000, 6000
    rowptr, col = _hop(T, S, 20, F_, dup=True)
    x = torch.randn((S, F_), generator=torch.Generator().manual_seed(1)).to(dtype).cuda()
    s = 1.0 + eps
    got = sum_aggregate(x, rowptr, col, T, s)
    torch.testing.assert_close(got, _ref_sum(x, rowptr, col, T, s), rtol=1e-5, atol=1e-5)
    if dtype == torch.float16 or s == 1.0:                   # s * x exact in fp32
        assert torch.equal(got, _seq_sum(x, rowptr, col, T, s))
    xg = x.clone().requires_grad_(True)
    xr = x.float().clone().requires_grad_(True)
    w = torch.randn((T, F_), device="cuda")
    (sum_aggregate(xg, rowptr, col, T, s) * w).sum().backward()
    (_ref_sum(xr, rowptr, col, T, s) * w).sum().backward()
    assert xg.grad.dtype == dtype
    torch.testing.assert_close(xg.grad.float(), xr.grad.to(dtype).float() if dtype == torch.float16 else xr.grad,
                               rtol=1e-3 if dtype == torch.float16 else 1e-4, atol=1e-3 if dtype == torch.float16 else 1e-5)


@pytest.mark.parametrize("F_,dtype", [(100, torch.float16), (47, torch.float32), (128, torch.float32)])
def test_sum_aggregate_strided_rows_hub_and_edge_cases(F_, dtype):
    from salient_plusplus_amd.models import sum_aggregate
    T, S = 700, 5000
    rowptr, col = _hop(T, S, 9, 3, hub=4500, dup=True)
    assert int(rowptr[2] - rowptr[1]) >= 4096
    buf = torch.randn((S, F_ + 28), device="cuda").to(dtype)
    x = buf[:, :F_]                                          # padded rows, as the resident table
    for s in (1.0, 1.5):
        _check_sum(sum_aggregate(x, rowptr, col, T, s), x, rowptr, col, T, s)
    # T = 0
    assert sum_aggregate(x, rowptr[:1], col[:0], 0, 1.0).shape == (0, F_)
    # E = 0: out = s * x[:T]
    empty = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    torch.testing.assert_close(sum_aggregate(x, empty, col[:0], T, 1.5), 1.5 * x[:T].float(), rtol=1e-6, atol=0)
    xg = x.float().clone().requires_grad_(True)
    g = torch.randn((T, F_), device="cuda")
    (sum_aggregate(xg, empty, col[:0], T, 1.5) * g).sum().backward()
    want = torch.zeros((S, F_), device="cuda")
    want[:T] = 1.5 * g
    torch.testing.assert_close(xg.grad, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("F_", [4, 47, 128, 256])
def test_sum_backward_gather_and_atomic_forms_on_both_sides_of_the_threshold(F_):
    import ctypes as C
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import models as M
    L = nat.load()
    p = lambda t: C.c_void_p(t.data_ptr())                                                     # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for T, S, maxdeg in ((300, 900, 8), (30000, 90000, 12)):          # E x F below and (for F >= 47) above 1 << 22
        rowptr, col = _hop(T, S, maxdeg, F_ + T, hub=4200, dup=True)
        E = col.numel()
        g = torch.randn((T, F_), device="cuda")
        for s in (1.0, 1.5):
            x = torch.randn((S, F_), device="cuda")
            xr = x.clone().requires_grad_(True)
            (_ref_sum(xr, rowptr, col, T, s) * g).sum().backward()
            ga = torch.full((S, F_), float("nan"), device="cuda")
            gb = torch.full((S, F_), float("nan"), device="cuda")
            nat.check(L.spp_csr_sum_backward(p(rowptr), p(col), T, S, p(g), F_, F_, s, p(ga), st))
            nbytes = int(L.spp_sage_operand_backward_workspace_bytes(T, S, E))
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            nat.check(L.spp_csr_sum_backward_gather(p(rowptr), p(col), T, S, E, p(g), F_, F_, s, p(gb), p(ws), nbytes, st))
            torch.testing.assert_close(ga, xr.grad, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(gb, xr.grad, rtol=1e-4, atol=1e-5)
            # and through autograd, whichever form the size picks
            xg = x.clone().requires_grad_(True)
            (M.sum_aggregate(xg, rowptr, col, T, s) * g).sum().backward()
            torch.testing.assert_close(xg.grad, xr.grad, rtol=1e-4, atol=1e-5)
        if F_ >= 47:
            assert (E * F_ >= M._SUM_GATHER_MIN_WORK) == (T == 30000)


def test_sum_forward_table_and_rows_equal_the_materialised_sum():
    import ctypes as C
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    p = lambda t: C.c_void_p(t.data_ptr())                                                     # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for F_, dtype in ((128, torch.float16), (100, torch.float32), (7, torch.float16), (47, torch.float32)):
        table = torch.randn((4000, F_ + 4), device="cuda").to(dtype)[:, :F_]
        n_id = torch.randperm(4000, device="cuda")[:1500]
        T = 400
        rowptr, col = _hop(T, 1500, 15, F_, dup=True)
        xm = table[n_id].contiguous()
        outs = [torch.full((T, F_), float("nan"), device="cuda") for _ in range(3)]
        half = int(dtype == torch.float16)
        nat.check(L.spp_csr_sum_forward(p(rowptr), p(col), T, p(xm), half, F_, F_, 1.5, p(outs[0]), F_, st))
        nat.check(L.spp_csr_sum_forward_table(p(rowptr), p(col), T, p(table), half, table.stride(0), 4000, p(n_id), F_,
                                              1.5, p(outs[1]), F_, st))
        addr = table.data_ptr() + n_id.to(torch.int64) * table.stride(0) * table.element_size()
        nat.check(L.spp_csr_sum_forward_rows(p(rowptr), p(col), T, p(addr), half, F_, 1.5, p(outs[2]), F_, st))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])      # same rows, same order
        torch.testing.assert_close(outs[0], _ref_sum(xm, rowptr, col, T, 1.5), rtol=1e-5, atol=1e-5)
        if not half:                                         # s * x exact in fp32: s = 2 for fp32 rows
            nat.check(L.spp_csr_sum_forward(p(rowptr), p(col), T, p(xm), half, F_, F_, 2.0, p(outs[0]), F_, st))
        assert torch.equal(outs[0], _seq_sum(xm, rowptr, col, T, 1.5 if half else 2.0))


def test_sum_entries_refuse_bad_arguments():
    import ctypes as C
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    rowptr, col = _hop(10, 20, 3, 0)
    g = torch.randn((10, 8), device="cuda")
    gx = torch.empty((20, 8), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                                     # noqa: E731
    with pytest.raises(nat.SppError, match="bad sizes"):
        nat.check(L.spp_csr_sum_backward(p(rowptr), p(col), 10, 5, p(g), 8, 8, 1.0, p(gx), None))
    with pytest.raises(nat.SppError, match="workspace too small"):
        ws = torch.empty(16, dtype=torch.uint8, device="cuda")
        nat.check(L.spp_csr_sum_backward_gather(p(rowptr), p(col), 10, 20, col.numel(), p(g), 8, 8, 1.0, p(gx), p(ws), 16,
                                                None))
    with pytest.raises(nat.SppError, match="node ids"):
        nat.check(L.spp_csr_sum_forward_table(p(rowptr), p(col), 10, p(g), 0, 8, 10, None, 8, 1.0, p(gx), 8, None))


# ---------------------------------------------------------------------------------------------- the models
def _pair(kind, Fin, C, hid=32, L=3):
    from salient_plusplus_amd.models import GIN, SAGEResInception
    torch.manual_seed(3)
    if kind == "gin":
        hip, ref = GIN(Fin, hid, C, L, dropout=0.0), RefGIN(Fin, hid, C, L, 0.0)
    else:
        hip, ref = SAGEResInception(Fin, hid, C, L, dropout=0.0), RefSAGERI(Fin, hid, C, L, 0.0)
    ref.load_state_dict(hip.state_dict())                   # the same module tree: the reference's checkpoints load
    hip.load_state_dict(ref.state_dict())
    return hip.cuda(), ref.cuda()


@pytest.mark.parametrize("kind", ["gin", "sageri"])
def test_models_match_the_reference_modules(kind):
    batches, C = _batches(100, n_batches=2)
    hip, ref = _pair(kind, 100, C)
    for b in batches:
        T0, end = int(b.adjs[0].size[1]), int(b.adjs[-1].size[1])
        assert end < T0                                      # the residual case: end_size smaller than T
        hip.eval(), ref.eval()
        with torch.no_grad():
            _close(hip(b.x, b.adjs), ref(b.x, b.adjs), 1e-4, "eval output")
        hip.train(), ref.train()
        oh, lh, gh = _step(hip, b.x, b.adjs, b.y)
        orf, lr, gr = _step(ref, b.x, b.adjs, b.y)
        _close(oh, orf, 1e-4, "train output")
        _close(lh, lr, 1e-5, "loss")
        assert gh.keys() == gr.keys()
        for n in gr:
            _close(gh[n], gr[n], 1e-3, n)
        bh, br = dict(hip.named_buffers()), dict(ref.named_buffers())
        assert bh.keys() == br.keys()
        for n in br:
            if "running" in n:
                _close(bh[n], br[n], 1e-4, n)
            else:
                assert torch.equal(bh[n].cpu(), br[n].cpu()), n


def test_sage_res_inception_concatenates_the_residual_added_rows():
    """the check above fails for a model that concatenates the activations taken before the residual add"""
    batches, C = _batches(100, n_batches=1)
    b = batches[0]
    hip, ref = _pair("sageri", 100, C)
    torch.nn.init.normal_(hip.res_linears[0].weight, std=0.5)
    ref.load_state_dict(hip.state_dict())
    hip.eval(), ref.eval()

    class PreResidual(RefSAGERI):                            # the careless rewrite
        def forward(self, _x, adjs):
            x = _x.to(torch.float)
            end_size = adjs[-1][-1][1]
            collect = [x[:end_size]]
            for k, (adj_t, _, size) in enumerate(adjs):
                x_target = x[:size[1]]
                h = F.leaky_relu(self.bns[k](self.convs[k]((x, x_target), adj_t)))
                collect.append(h[:end_size].clone())
                x = h + self.res_linears[k](x_target)
            return torch.log_softmax(self.mlp(torch.cat(collect, -1)), dim=-1)

    wrong = PreResidual(100, 32, C, 3, 0.0).cuda().eval()
    wrong.load_state_dict(hip.state_dict())
    with torch.no_grad():
        got, want, bad = hip(b.x, b.adjs), ref(b.x, b.adjs), wrong(b.x, b.adjs)
    _close(got, want, 1e-4, "output")
    assert (bad - want).abs().max() > 1e-2


@pytest.mark.parametrize("kw", [{}, {"table_features": True}])
def test_gin_on_the_delivered_batches(kw):
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.models import GIN
    batches, C = _batches(128, n_batches=3, seed=1, **kw)
    torch.manual_seed(5)
    model = GIN(128, 64, C, 3, dropout=0.0).cuda().train()
    for b in batches:
        if kw:
            assert isinstance(b.x, fs.TableRows)
            xm = b.x.materialize()
        else:
            assert isinstance(b.x, torch.Tensor)
            xm = b.x.float()                                 # the reference's x.to(torch.float)
        _, la, ga = _step(model, b.x, b.adjs, b.y)
        _, lb, gb = _step(model, xm, b.adjs, b.y)
        _close(la, lb, 1e-5, "loss")
        for n in gb:
            _close(ga[n], gb[n], 1e-5, n)


def _rank_cfg(g, rank, P, offsets, nb, bs, fs):
    from salient_plusplus_amd.fast_trainer.samplers import FastSamplerConfig
    lo, hi = int(offsets[rank]), int(offsets[rank + 1])
    T_ = torch.from_numpy
    idx = g["idx"][(len(g["idx"]) * rank) // P:(len(g["idx"]) * (rank + 1)) // P]
    cut = (hi - lo) // 3
    return FastSamplerConfig(
        x_cpu=T_(g["x"][lo:hi][cut:].copy()), x_gpu=T_(g["x"][lo:hi][:cut].copy()).cuda(), y=T_(g["y"]).unsqueeze(-1),
        rowptr=T_(g["rowptr"]), col=T_(g["col"]), idx=T_(idx), batch_size=bs, sizes=SIZES, skip_nonfull_batch=False,
        pin_memory=False, distributed=True, partition_book=fs.RangePartitionBook(rank, P, T_(np.asarray(offsets))),
        cache=fs.Cache(), force_exact_num_batches=True, exact_num_batches=nb, count_remote_frequency=False,
        use_cache=False)


@pytest.mark.parametrize("F_", [100, 7])
def test_gin_on_row_references_of_partitioned_ranks(F_, monkeypatch):
    """row_refs=True on two in-process ranks (native exchange): GIN's first layer sums the rows at their addresses"""
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler
    from salient_plusplus_amd.fast_trainer.transferers import DeviceDistributedPrefetcher
    from salient_plusplus_amd.models import GIN
    monkeypatch.setenv("SPP_EXCHANGE_ISSUE", "consumer")
    monkeypatch.setenv("SPP_DIST_TRANSPORT", "rccl")
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_a.npz")))
    n = g["rowptr"].shape[0] - 1
    g["x"] = np.random.default_rng(9).standard_normal((n, F_)).astype(np.float16)
    P, offsets, nb = 2, [0, 1400, n], 3
    C = int(g["y"].max()) + 1
    comms = fs.NativeComm.local(P)
    errors, seen = [], []

    def rank_main(rank):
        it = None
        try:
            torch.cuda.set_device(0)
            fs.set_native_comm(comms[rank])
            torch.manual_seed(11)
            model = GIN(F_, 32, C, 3, dropout=0.0).cuda().train()
            it = iter(FastSampler(2, 6, _rank_cfg(g, rank, P, offsets, nb, 16, fs), row_refs=True))
            for (b,) in DeviceDistributedPrefetcher([torch.device("cuda", 0)], it, True):
                assert isinstance(b.x, fs.RowRefs)
                _, la, ga = _step(model, b.x, b.adjs, b.y)
                _, lb, gb = _step(model, b.x.materialize(), b.adjs, b.y)
                _close(la, lb, 1e-5, "loss")
                for k in gb:
                    _close(ga[k], gb[k], 1e-5, k)
                seen.append(rank)
            it.session.close()
        except BaseException as e:  # noqa: BLE001
            import traceback
            errors.append(f"rank {rank}: {e}\n{traceback.format_exc()}")
            if it is not None:
                it.session.close()
            comms[rank].close()
        finally:
            fs.set_native_comm(None)

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(240)
    hung = [t for t in ts if t.is_alive()]
    for c in comms:
        c.close()
    assert not errors, "\n".join(errors)
    assert not hung, "rank thread hung"
    assert sorted(seen) == [0] * nb + [1] * nb
    fs.clear_resident_cache()


@pytest.mark.parametrize("kind", ["gin", "sageri"])
def test_ten_adam_steps_lower_the_loss(kind):
    from salient_plusplus_amd.models import GIN, SAGEResInception
    batches, C = _batches(100, n_batches=1, seed=2)
    b = batches[0]
    torch.manual_seed(0)
    model = (GIN if kind == "gin" else SAGEResInception)(100, 64, C, 3).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)

    def eval_loss():                                         # train mode (batch statistics), the same dropout masks
        torch.manual_seed(123)
        with torch.no_grad():
            return float(F.nll_loss(model(b.x, b.adjs), b.y.reshape(-1)))

    before = eval_loss()
    model.train()
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        F.nll_loss(model(b.x, b.adjs), b.y.reshape(-1)).backward()
        opt.step()
    assert eval_loss() < before


@pytest.mark.parametrize("kind", ["gin", "sageri"])
def test_dropout_defaults_act_in_train_mode_only(kind):
    from salient_plusplus_amd.models import GIN, SAGEResInception
    batches, C = _batches(100, n_batches=1, seed=4)
    b = batches[0]
    model = (GIN if kind == "gin" else SAGEResInception)(100, 64, C, 3).cuda()
    with torch.no_grad():
        model.train()
        a, c = model(b.x, b.adjs), model(b.x, b.adjs)
        assert not torch.equal(a, c)
        model.eval()
        assert torch.equal(model(b.x, b.adjs), model(b.x, b.adjs))
