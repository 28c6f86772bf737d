"""GPU: the four models under torch.autocast("cuda", dtype=torch.bfloat16) against the same weights in fp32.

Tolerances (relative Frobenius errors of one step on a sampled batch, see _errors): the output within 1e-2; every
parameter gradient within 6e-2 (SAGE, GAT), 1e-1 (SAGEResInception) and 3e-1 (GIN), and -- for SAGE, GIN and
SAGEResInception -- within 1.5x (+ 5e-3) of the error that torch's own bf16 autocast gives on the plain-torch
restatement of the model.  Measured on an MI355X: outputs 4e-4 .. 2e-3; the largest gradient errors 4.4e-2 (SAGE),
2.4e-2 (GAT), 7e-2 (SAGEResInception) and 0.22 (GIN); SAGE's are below the restatement's, GIN's and
SAGEResInception's within 20 % of them.  Under fp16 autocast the HIP
nodes run their fp32 path, so SAGE's output is the no-autocast output exactly."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

# per-parameter bounds (see _errors); GIN and SAGEResInception carry most of their bf16 error in torch's BatchNorm /
# Linear chain, and the models with a torch restatement are also held to that restatement's own bf16-autocast error
REL_TOL = {"sage": 6e-2, "gat": 6e-2, "sageresinception": 1e-1, "gin": 3e-1}
OUT_TOL = 1e-2
MODELS = ["sage", "gat", "gin", "sageresinception"]


@pytest.fixture(autouse=True)
def _entries_exist():
    """first: the bf16 entries exist (the parent's SAGE and GAT must not run under autocast: they misread bf16 rows)"""
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    assert hasattr(L, "spp_agg_forward") and hasattr(L, "spp_agg_backward"), "spp_agg_forward is not exported"


def _bf16():
    return torch.autocast("cuda", dtype=torch.bfloat16)


def _model(kind, Fin, C, hid=64, L=3):
    from salient_plusplus_amd.models import get_model_type
    cls = get_model_type(kind)
    kw = {"dropout": 0.0} if kind in ("gin", "sageresinception") else {}
    m = cls(Fin, hid, C, L, **kw).cuda()
    # dropout off: SAGE and GAT fix p = 0.5 in train mode (eval), GIN and SAGEResInception take dropout=0 (train mode,
    # batch statistics)
    return m.eval() if kind in ("sage", "gat") else m.train()


def _reference(kind, model, Fin, C):
    """the torch restatement of the model (plain torch ops, the same weights), or None"""
    import bench
    from test_gpu_gin_sage_ri import RefGIN, RefSAGERI
    if kind == "sage":
        ref = bench.TorchSAGE(Fin, 64, C, 3).cuda().eval()
        for i in range(3):
            ref.lin_l[i].weight.data.copy_(model.convs[i].lin_l.weight.data)
            ref.lin_r[i].weight.data.copy_(model.convs[i].lin_r.weight.data)
        return ref
    if kind in ("gin", "sageresinception"):
        ref = (RefGIN if kind == "gin" else RefSAGERI)(Fin, 64, C, 3, 0.0).cuda().train()
        ref.load_state_dict(model.state_dict())
        return ref
    return None


def _run(model, x, adjs, y, amp=None):
    model.zero_grad(set_to_none=True)
    with (amp if amp is not None else torch.autocast("cuda", enabled=False)):
        out = model(x, adjs)
        loss = F.nll_loss(out, y.reshape(-1))
    loss.backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-30))


def _errors(model, x, adjs, y):
    """(output error, {parameter: gradient error}) of a bf16-autocast step against the fp32 step of the same model.
    A gradient's error is ||g_bf16 - g_fp32|| / max(||g_fp32||, 1e-2 ||all fp32 gradients||): gradients that are ~0 by
    construction (a Linear bias in front of BatchNorm, GAT's att_dst away from the LeakyReLU kink) are measured against
    the step's gradient scale, not against their own rounding noise."""
    out32, g32 = _run(model, x, adjs, y)
    out16, g16 = _run(model, x, adjs, y, _bf16())
    assert torch.isfinite(out16).all() and out16.dtype == torch.float32
    assert set(g16) == set(g32) and len(g32) == len(list(model.parameters()))
    tot = float(torch.sqrt(sum((g.float() ** 2).sum() for g in g32.values())))
    errs = {}
    for n in g32:
        assert g16[n].dtype == torch.float32, n
        errs[n] = float((g16[n] - g32[n]).norm()) / max(float(g32[n].norm()), 1e-2 * tot)
    return _rel(out16, out32), errs


@pytest.mark.parametrize("kind", MODELS)
def test_bf16_autocast_matches_fp32_within_tolerance(kind):
    from test_gpu_gin_sage_ri import _batches
    batches, C = _batches(128, n_batches=1, seed=4)
    b = batches[0]
    torch.manual_seed(1)
    model = _model(kind, 128, C)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    out_err, errs = _errors(model, b.x, b.adjs, b.y)
    assert all(v.dtype == state[k].dtype and v.shape == state[k].shape for k, v in model.state_dict().items())
    assert set(model.state_dict()) == set(state)
    print(f"\nAMP_REL_ERR {kind} out {out_err:.3e} max-grad {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert out_err < OUT_TOL
    bad = {k: v for k, v in errs.items() if not v < REL_TOL[kind]}
    assert not bad, bad
    ref = _reference(kind, model, 128, C)
    if ref is not None:                                        # no worse than torch's own bf16 autocast of the restatement
        ref_out_err, ref_errs = _errors(ref, b.x.float(), b.adjs, b.y)
        names = {n: n for n in errs} if kind != "sage" else \
            {f"convs.{i}.lin_{s}.weight": f"lin_{s}.{i}.weight" for i in range(3) for s in "lr"}
        print(f"AMP_REL_ERR {kind} torch restatement: out {ref_out_err:.3e} max-grad {max(ref_errs.values()):.3e}")
        worse = {n: (errs[n], ref_errs[names[n]]) for n in errs if not errs[n] <= 1.5 * ref_errs[names[n]] + 5e-3}
        assert not worse, worse


@pytest.mark.parametrize("tdtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kind", ["sage", "gin"])
def test_table_rows_and_row_refs_give_the_dense_bf16_output(kind, tdtype):
    """the first layer reads TableRows / RowRefs in place under bf16 autocast: same rows, same order, same bits"""
    from salient_plusplus_amd.fast_sampler import RowRefs, TableRows
    from test_gpu_gin_sage_ri import _batches
    batches, C = _batches(128, n_batches=1, seed=6)
    b = batches[0]
    S = b.x.size(0)
    gen = torch.Generator().manual_seed(9)
    table = torch.randn((3 * S, 128), generator=gen).to(tdtype).cuda()
    n_id = torch.randint(0, 3 * S, (S,), generator=gen).cuda()
    dense = table[n_id].contiguous()
    addr = (table.data_ptr() + n_id * table.stride(0) * table.element_size()).contiguous()
    torch.manual_seed(2)
    model = _model(kind, 128, C)
    outs = []
    for x in (dense, TableRows(table, n_id), RowRefs(addr, n_id, 128, tdtype, None, (table,))):
        with torch.no_grad(), _bf16():
            outs.append(model(x, b.adjs))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


@pytest.mark.parametrize("kind", MODELS)
def test_fp16_autocast_runs_the_fp32_path(kind):
    from test_gpu_gin_sage_ri import _batches
    batches, C = _batches(128, n_batches=1, seed=7)
    b = batches[0]
    torch.manual_seed(3)
    model = _model(kind, 128, C)
    fp16 = torch.autocast("cuda", dtype=torch.float16)
    if kind == "sage":
        with torch.no_grad():
            plain = model(b.x, b.adjs)
            with fp16:
                amp = model(b.x, b.adjs)
        assert amp.dtype == torch.float32 and torch.equal(amp, plain)
        model.train()                                            # dropout masks from the same seeds
        torch.manual_seed(11)
        plain, g_plain = _run(model, b.x, b.adjs, b.y)
        torch.manual_seed(11)
        amp, g_amp = _run(model, b.x, b.adjs, b.y, fp16)
        assert torch.equal(amp, plain)
        for n in g_plain:                                        # (the backward's fp32 atomics: order not fixed)
            torch.testing.assert_close(g_amp[n], g_plain[n], rtol=1e-3, atol=1e-6)
    else:
        out, grads = _run(model, b.x, b.adjs, b.y, fp16)
        assert torch.isfinite(out).all()
        for n, g in grads.items():
            assert g.dtype == torch.float32 and torch.isfinite(g).all(), n


def test_end_to_end_training_learns_under_bf16_autocast():
    """test_end_to_end_training_learns_through_the_data_path with the step wrapped in bf16 autocast: the same bars"""
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig
    from salient_plusplus_amd.fast_trainer.shufflers import Shuffler
    from salient_plusplus_amd.fast_trainer.transferers import DevicePrefetcher
    from salient_plusplus_amd.models import SAGE
    from salient_plusplus_amd.synthetic import make_graph
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n, Fin, C = 6000, 16, 4
    rowptr, col = make_graph(n, 30000, 5, dev)
    x = torch.randn((n, Fin), device=dev)
    deg = (rowptr[1:] - rowptr[:-1]).clamp(min=1)
    row = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
    nb_mean = torch.zeros_like(x).index_add_(0, row, x[col]) / deg.unsqueeze(-1)
    w_self, w_nb = torch.randn((Fin, C), device=dev), torch.randn((Fin, C), device=dev)
    y = (x @ w_self + 3.0 * (nb_mean @ w_nb)).argmax(-1)
    perm = torch.randperm(n, device=dev)
    train, test = perm[:4500], perm[4500:]

    def loader(idx, bs):
        cfg = FastSamplerConfig(
            x_cpu=x.half(), x_gpu=torch.empty(0), y=y.unsqueeze(-1), rowptr=rowptr, col=col, idx=idx, batch_size=bs,
            sizes=[10, 10], skip_nonfull_batch=False, pin_memory=False, distributed=False, partition_book=None,
            cache=fs.Cache(), force_exact_num_batches=True, exact_num_batches=max(1, idx.numel() // bs),
            count_remote_frequency=False, use_cache=False)
        return FastSampler(2, 8, cfg)

    model = SAGE(Fin, 64, C, 2).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    shuffler = Shuffler(train)
    sampler = loader(train, 256)
    first = last = None
    for epoch in range(6):
        shuffler.set_epoch(epoch)
        sampler.idx = shuffler.get_idx()
        model.train()
        for (b,) in DevicePrefetcher([dev], iter(sampler)):
            opt.zero_grad(set_to_none=True)
            with _bf16():
                loss = F.nll_loss(model(b.x, b.adjs), b.y.reshape(-1))
            loss.backward()
            opt.step()
            first = float(loss.detach()) if first is None else first
            last = float(loss.detach())
    assert all(p.dtype == torch.float32 for p in model.parameters())
    assert last < 0.6 * first, (first, last)
    model.eval()
    hit = tot = 0
    with torch.no_grad(), _bf16():
        for (b,) in DevicePrefetcher([dev], iter(loader(test, 250))):
            pred = model(b.x, b.adjs).argmax(-1)
            hit += int((pred == b.y.reshape(-1)).sum())
            tot += pred.numel()
    assert tot == test.numel() and hit / tot > 0.6, hit / tot        # chance is 0.25


# ---- one call path: every aggregation of SAGE, GIN and SAGEResInception goes through the descriptor entries ----
_AGG_ALLOWED = {"spp_agg_forward", "spp_agg_forward_fp8", "spp_agg_backward", "spp_sage_operand_backward_workspace_bytes"}
_AGG_PREFIXES = ("spp_agg_", "spp_csr_mean_", "spp_csr_sum_", "spp_sage_operand_", "spp_relu_dropout_backward_pre")
# (last hop's targets, maxdeg, sources of the last hop, sources of the first hop): the small chain is far below the
# gather threshold E * 256 >= 1 << 22 of the hidden layer's hop, the large one above it (about 24 k edges: 6.1 M)
_CHAINS = {"small": (64, 5, 200, 500), "large": (3000, 16, 3500, 6000)}


class _Recorder:
    """the native library with every entry's name noted as it is called (spp_agg_backward: with the descriptor's form)"""

    def __init__(self, lib):
        self._lib, self.names, self.forms = lib, set(), set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.add(name)
            if name == "spp_agg_backward":
                self.forms.add(args[0]._obj.form)
            return fn(*args)
        return call


def _chain(which):
    """a 2-hop MFG chain (outermost hop first) with fp32 features [S0, 128] and labels for the last hop's targets"""
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    T, maxdeg, S1, S0 = _CHAINS[which]
    g = torch.Generator().manual_seed(T)
    adjs = []
    for S, Th in ((S0, S1), (S1, T)):
        deg = torch.randint(0, maxdeg + 1, (Th,), generator=g)
        rowptr = torch.zeros(Th + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(deg, 0)
        col = torch.randint(0, S, (int(rowptr[-1]),), generator=g)
        adjs.append((SparseTensor(rowptr=rowptr.cuda(), col=col.cuda(), sparse_sizes=(Th, S)), None, (S, Th)))
    x = torch.randn((S0, 128), generator=g).cuda()
    y = torch.randint(0, 10, (T,), generator=g).cuda()
    return x, adjs, y


@pytest.mark.parametrize("which", ["small", "large"])
def test_every_aggregation_goes_through_the_descriptor_entries(which, monkeypatch):
    """One seeded training step of SAGE, GIN and SAGEResInception (2 layers, hidden 256) on fp32 rows, fp16 rows, under
    bf16 autocast and (SAGE, GIN) over a TableRows: no positional aggregation entry is called, SAGE's backward takes the
    scatter form on the small chain and the gather form on the large one, and on both sides of that threshold the fp32
    SAGE equals its plain-torch restatement (eval mode) within test_sage_matches_plain_torch_on_a_sampled_batch's
    tolerances."""
    import bench
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_sampler import TableRows
    x, adjs, y = _chain(which)
    E = adjs[1][0].csr()[1].numel()
    assert (E * 256 >= 1 << 22) == (which == "large"), E
    table = torch.randn((2 * x.size(0), 128), generator=torch.Generator().manual_seed(5)).cuda()
    n_id = torch.randint(0, table.size(0), (x.size(0),), generator=torch.Generator().manual_seed(6)).cuda()
    rec = _Recorder(nat.load())
    monkeypatch.setattr(models.nat, "load", lambda: rec)
    forms = {}
    for kind in ("sage", "gin", "sageresinception"):
        torch.manual_seed(7)
        model = models.get_model_type(kind)(128, 256, 10, 2).cuda().train()
        runs = [(x, None), (x.half(), None), (x, _bf16())]
        if kind != "sageresinception":
            runs.append((TableRows(table, n_id), None))
        for rows, amp in runs:
            torch.manual_seed(8)
            out, grads = _run(model, rows, adjs, y, amp)
            assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())
        forms[kind], rec.forms = rec.forms, set()
    agg = {n for n in rec.names if n.startswith(_AGG_PREFIXES)}
    assert {"spp_agg_forward", "spp_agg_backward"} <= agg <= _AGG_ALLOWED, sorted(agg - _AGG_ALLOWED)
    want_form = nat.SPP_AGG_GATHER if which == "large" else nat.SPP_AGG_SCATTER
    assert forms["sage"] == {want_form} and forms["gin"] == {want_form}, forms
    # the fp32 stack against plain torch ops on the same weights
    torch.manual_seed(0)
    hip = models.SAGE(128, 256, 10, 2).cuda().eval()
    ref = bench.TorchSAGE(128, 256, 10, 2).cuda().eval()
    for i in range(2):
        ref.lin_l[i].weight.data.copy_(hip.convs[i].lin_l.weight.data)
        ref.lin_r[i].weight.data.copy_(hip.convs[i].lin_r.weight.data)
    out_h, out_r = hip(x, adjs), ref(x, adjs)
    torch.testing.assert_close(out_h, out_r, rtol=1e-4, atol=1e-5)
    F.nll_loss(out_h, y).backward()
    F.nll_loss(out_r, y).backward()
    assert rec.forms == {want_form}
    for i in range(2):
        torch.testing.assert_close(hip.convs[i].lin_l.weight.grad, ref.lin_l[i].weight.grad, rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(hip.convs[i].lin_r.weight.grad, ref.lin_r[i].weight.grad, rtol=1e-3, atol=1e-6)
