"""CPU-only: the f3p entries (spp_bn_act_forward / spp_bn_act_backward, include/spp.h) are exported and refuse what
the contract lists before any launch, in a message that starts with the entry's own name; models.batch_norm_act on CPU
tensors is the plain torch composition bit for bit; and the fused_norm flag of GIN / SAGEResInception changes neither
the module tree nor, on the CPU, a single bit of the output.  ctypes descriptors and fake non-NULL pointers: a refusal
dereferences nothing and enqueues nothing."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_FAKE = 0x10000                                               # 16-byte aligned, never dereferenced
SPP_OK, SPP_ERR_INVALID = 0, -1
ENTRIES = ["spp_bn_act_forward", "spp_bn_act_backward"]


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def _desc(nat, L, **over):
    """a descriptor both entries accept: 100 rows of C = 8 fp32 columns, training, relu, p = 0.1"""
    kw = dict(z_elem=0, r_elem=0, y_elem=0, g_elem=0, act=nat.SPP_BN_ACT_RELU, training=1, negative_slope=0.01, p=0.1,
              eps=1e-5, momentum=0.1, seed=7, n=100, C=8, z_dev=_FAKE, gamma_dev=_FAKE, beta_dev=_FAKE,
              running_mean_dev=_FAKE, running_var_dev=_FAKE, num_batches_tracked_dev=_FAKE, r_dev=None, y_dev=_FAKE,
              mean_dev=_FAKE, invstd_dev=_FAKE, g_dev=_FAKE, dz_dev=_FAKE, dgamma_dev=_FAKE, dbeta_dev=_FAKE,
              workspace_dev=_FAKE, workspace_bytes=None)
    kw.update(over)
    if kw["workspace_bytes"] is None:
        kw["workspace_bytes"] = int(L.spp_bn_act_workspace_bytes(max(kw["n"], 0), max(kw["C"], 1)))
    return nat.BnActDesc(**kw)


# (class, descriptor changes, the word of the class, the entries it applies to)
REFUSALS = [
    ("one row in training", dict(n=1), b"more than 1 value per channel", ENTRIES),
    ("no rows in training", dict(n=0), b"more than 1 value per channel", ENTRIES),
    ("negative n", dict(n=-3, training=0), b"negative n", ENTRIES),
    ("C = 0", dict(C=0), b"C = 0", ENTRIES),
    ("negative C", dict(C=-8), b"C = -8", ENTRIES),
    ("p = 1", dict(p=1.0), b"[0, 1)", ENTRIES),
    ("negative p", dict(p=-0.1), b"[0, 1)", ENTRIES),
    ("NaN p", dict(p=float("nan")), b"[0, 1)", ENTRIES),
    ("unknown act", dict(act=3), b"activation code", ENTRIES),
    ("negative act", dict(act=-1), b"activation code", ENTRIES),
    ("fp16 z", dict(z_elem=1), b"element code", ENTRIES),
    ("fp8 z", dict(z_elem=3), b"element code", ENTRIES),
    ("unknown y element", dict(y_elem=9), b"element code", ["spp_bn_act_forward"]),
    ("fp16 residual", dict(r_dev=_FAKE, r_elem=1), b"element code", ["spp_bn_act_forward"]),
    ("fp16 gradient", dict(g_elem=1), b"element code", ["spp_bn_act_backward"]),
    ("NULL z", dict(z_dev=None), b"NULL buffer", ENTRIES),
    ("NULL gamma", dict(gamma_dev=None), b"NULL buffer", ENTRIES),
    ("NULL beta", dict(beta_dev=None), b"NULL buffer", ENTRIES),
    ("NULL mean", dict(mean_dev=None), b"NULL buffer", ENTRIES),
    ("NULL invstd", dict(invstd_dev=None), b"NULL buffer", ENTRIES),
    ("NULL y", dict(y_dev=None), b"NULL buffer", ["spp_bn_act_forward"]),
    ("NULL g", dict(g_dev=None), b"NULL buffer", ["spp_bn_act_backward"]),
    ("NULL dz", dict(dz_dev=None), b"NULL buffer", ["spp_bn_act_backward"]),
    ("NULL dgamma", dict(dgamma_dev=None), b"NULL buffer", ["spp_bn_act_backward"]),
    ("NULL dbeta", dict(dbeta_dev=None), b"NULL buffer", ["spp_bn_act_backward"]),
    ("eval without running statistics", dict(training=0, running_mean_dev=None, running_var_dev=None), b"NULL buffer",
     ["spp_bn_act_forward"]),
    ("one running buffer", dict(running_var_dev=None), b"come together", ["spp_bn_act_forward"]),
    ("cumulative average without its counter", dict(momentum=-1.0, num_batches_tracked_dev=None), b"NULL buffer",
     ["spp_bn_act_forward"]),
    ("missing workspace", dict(workspace_dev=None), b"workspace", ENTRIES),
    ("misaligned workspace", dict(workspace_dev=_FAKE + 8), b"workspace", ENTRIES),
    ("short workspace", dict(workspace_bytes=16), b"workspace", ENTRIES),
]


def test_the_entries_are_exported_and_the_abi_version_stays():
    nat, L = _lib()
    for name in ENTRIES + ["spp_bn_act_workspace_bytes", "spp_bn_act_slab_rows"]:
        assert hasattr(L, name), name
    assert L.spp_abi_version() == 6
    R = int(L.spp_bn_act_slab_rows())
    assert R >= 2
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    assert f"#define SPP_BN_ACT_SLAB_ROWS {R}\n" in header    # the published constant is the one the kernels use
    # three floats per column and slab, never less than one aligned piece
    assert L.spp_bn_act_workspace_bytes(2 * R + 1, 47) == 3 * 47 * 12
    assert L.spp_bn_act_workspace_bytes(1, 1) == 16 and L.spp_bn_act_workspace_bytes(0, 256) == 16


@pytest.mark.parametrize("what,over,word,entries", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_entry(what, over, word, entries):
    nat, L = _lib()
    for entry in entries:
        d = _desc(nat, L, **over)
        assert getattr(L, entry)(ctypes.byref(d), None) == SPP_ERR_INVALID, (entry, what)
        msg = L.spp_last_error()
        assert msg.startswith(entry.encode() + b":") and word in msg, (entry, what, msg)


def test_null_descriptor_and_the_empty_eval_call():
    nat, L = _lib()
    for entry in ENTRIES:
        assert getattr(L, entry)(None, None) == SPP_ERR_INVALID
        assert L.spp_last_error().startswith(entry.encode() + b": NULL descriptor")
        # n == 0 in eval: success before any device call, without a workspace
        d = _desc(nat, L, n=0, training=0, workspace_dev=None, workspace_bytes=0)
        assert getattr(L, entry)(ctypes.byref(d), None) == SPP_OK, L.spp_last_error()


# ---------------------------------------------------------------------------------------------- batch_norm_act on the CPU
def _composition(z, bn, act, slope, p, training, r):
    was = bn.training
    bn.train(training)
    h = bn(z)
    bn.train(was)
    h = F.relu(h) if act == "relu" else F.leaky_relu(h, slope) if act == "leaky_relu" else h
    h = F.dropout(h, p, training)
    return h if r is None else h + r


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", ["none", "relu", "leaky_relu"])
@pytest.mark.parametrize("with_r", [False, True])
def test_cpu_tensors_take_the_torch_composition_bit_for_bit(act, training, with_r, momentum):
    from salient_plusplus_amd.models import batch_norm_act
    g = torch.Generator().manual_seed(11)
    z0 = torch.randn((37, 12), generator=g) * 2 + 1
    r0 = torch.randn((37, 12), generator=g)
    w = torch.randn((37, 12), generator=g)
    res = []
    for fn in (batch_norm_act, None):
        torch.manual_seed(0)
        bn = torch.nn.BatchNorm1d(12, momentum=momentum)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5), bn.bias.uniform_(-1, 1)
            bn.running_mean.uniform_(-1, 1), bn.running_var.uniform_(0.5, 2)
        bn.train(not training)                                # the argument, not the module's mode, decides
        z, r = z0.clone().requires_grad_(True), (r0.clone().requires_grad_(True) if with_r else None)
        if fn is not None:
            y = fn(z, bn, act=act, negative_slope=0.02, p=0.0, training=training, residual=r)
        else:
            y = _composition(z, bn, act, 0.02, 0.0, training, r)
        assert bn.training == (not training)
        (y * w).sum().backward()
        res.append((y.detach(), z.grad, bn.weight.grad, bn.bias.grad, r.grad if with_r else None,
                    bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()))
    for a, b in zip(*res):
        assert (a is None and b is None) or torch.equal(a, b)
    assert int(res[0][-1]) == (1 if training else 0)
    if with_r:
        assert torch.equal(res[0][4], w)                      # the residual's gradient is g itself


def test_training_defaults_to_the_modules_mode_and_bad_arguments_raise():
    from salient_plusplus_amd.models import batch_norm_act
    bn = torch.nn.BatchNorm1d(4)
    z = torch.randn(9, 4)
    bn.eval()
    assert torch.equal(batch_norm_act(z, bn), bn(z)) and int(bn.num_batches_tracked) == 0
    bn.train()
    batch_norm_act(z, bn)
    assert int(bn.num_batches_tracked) == 1
    with pytest.raises(ValueError, match="act must be one of"):
        batch_norm_act(z, bn, act="gelu")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        batch_norm_act(z[:1], bn)
    # modules the kernels do not cover run the composition
    plain = torch.nn.BatchNorm1d(4, affine=False, track_running_stats=False)
    assert torch.equal(batch_norm_act(z, plain, act="relu"), F.relu(plain(z)))


# ---------------------------------------------------------------------------------------------- the model flags
def _models(kind, fused):
    from salient_plusplus_amd.models import GIN, SAGEResInception
    torch.manual_seed(2)
    cls = GIN if kind == "gin" else SAGEResInception
    return cls(10, 16, 5, 3, dropout=0.0, **({"fused_norm": True} if fused else {}))


@pytest.mark.parametrize("kind", ["gin", "sageri"])
def test_fused_norm_keeps_the_module_tree_and_the_state_dict(kind):
    plain, fused = _models(kind, False), _models(kind, True)
    assert plain.fused_norm is False and fused.fused_norm is True          # the default is off
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf)
    assert all(sp[k].shape == sf[k].shape and sp[k].dtype == sf[k].dtype for k in sp)
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in fused.named_modules()]
    assert [type(m) for m in plain.modules()] == [type(m) for m in fused.modules()]
    plain.load_state_dict(sf)
    fused.load_state_dict(sp)


class _Adj:
    def __init__(self, rowptr, col):
        self.rowptr, self.col = rowptr, col

    def csr(self):
        return self.rowptr, self.col, None


@pytest.mark.parametrize("kind", ["gin", "sageri"])
def test_on_the_cpu_both_variants_give_identical_train_mode_outputs(kind, monkeypatch):
    """the aggregation needs a GPU, so it is replaced by its index_add_ restatement; everything behind it is the model's"""
    from salient_plusplus_amd import models as M

    def agg(x, rowptr, col, T, mean):
        cnt = rowptr[1:] - rowptr[:-1]
        row = torch.repeat_interleave(torch.arange(T), cnt)
        out = torch.zeros((T, x.size(1))).index_add_(0, row, x.float()[col])
        return out / cnt.clamp(min=1).unsqueeze(-1) if mean else out

    class Sum:
        @staticmethod
        def apply(x, rowptr, col, T, s):
            return agg(x, rowptr, col, T, False) + s * x[:T]

    class Mean:
        @staticmethod
        def apply(x, rowptr, col, T, concat):
            m = agg(x, rowptr, col, T, True)
            return torch.cat([m, x[:T]], dim=1) if concat else m

    class Tall:
        @staticmethod
        def apply(a, w):
            return a @ w.t()

    monkeypatch.setattr(M, "_SumAggregate", Sum)
    monkeypatch.setattr(M, "_MeanAggregate", Mean)
    monkeypatch.setattr(M, "_TallLinear", Tall)
    calls = []
    real = M.batch_norm_act
    monkeypatch.setattr(M, "batch_norm_act", lambda *a, **k: calls.append(k["act"]) or real(*a, **k))
    monkeypatch.setattr(M, "mean_aggregate", lambda x, rowptr, col, T: agg(x, rowptr, col, T, True))
    g = torch.Generator().manual_seed(4)
    sizes = [(40, 20), (20, 9), (9, 4)]
    adjs = []
    for S, T in sizes:
        deg = torch.randint(0, 5, (T,), generator=g)
        rowptr = torch.zeros(T + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(deg, 0)
        adjs.append((_Adj(rowptr, torch.randint(0, S, (int(rowptr[-1]),), generator=g)), None, (S, T)))
    x = torch.randn((40, 10), generator=g)
    plain, fused = _models(kind, False).train(), _models(kind, True).train()
    fused.load_state_dict(plain.state_dict())
    a = plain(x, adjs)
    assert calls == []                                        # flag off: the modules themselves
    b = fused(x, adjs)
    assert calls == ["relu" if kind == "gin" else "leaky_relu"] * 3
    assert torch.equal(a, b)
    for (n, u), (_, v) in zip(plain.named_buffers(), fused.named_buffers()):
        assert torch.equal(u, v), n
