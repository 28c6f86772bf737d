"""CPU: attention dropout of TransformerConv (spp.h f4a: spp_transformer_forward_drop / spp_transformer_backward_drop)
without a device.  The two entries are exported, bound and declared with the documented argument list; they refuse what
the header says in the order it says, p included; T == 0 enqueues nothing.  The float64 restatement of
tests/transformer_drop_f64.py is checked on its own: its closed-form gradients are autograd's, a correct fp32
computation of the dropped formulas stays inside every bound, and three planted faults leave them."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transformer_drop_f64 as XD  # noqa: E402
import transformer_f64 as X  # noqa: E402

DROP = {"spp_transformer_forward_drop": "spp_transformer_forward",
        "spp_transformer_backward_drop": "spp_transformer_backward"}
F32 = torch.float32
CC = 8                               # channels per head of the restatement's own checks


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


def test_symbols_are_exported_bound_and_declared():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, base in DROP.items():
        assert hasattr(L, name), name
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and args == nat.SIGNATURES[base][1] + [C.c_float, C.c_int32, C.c_uint64], name
        decl = re.search(r"\bspp_status\s+%s\s*\((.*?)\);" % name, src, re.S).group(1)
        assert re.sub(r"\s+", " ", decl) == \
            "const spp_transformer_desc* desc, void* stream, float p, int32_t training, uint64_t seed"
    assert "#define SPP_ABI_VERSION 6" in header and L.spp_abi_version() == 6
    fields = re.search(r"typedef struct spp_transformer_desc \{(.*?)\} spp_transformer_desc;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in nat.TransformerDesc._fields_]   # the descriptor is untouched


_MEM = (C.c_char * 128)()
_PTRS = {"rowptr_dev", "col_dev", "q_dev", "k_dev", "v_dev", "out_dev", "row_max_dev", "row_sum_dev", "grad_out_dev",
         "grad_q_dev", "grad_k_dev", "grad_v_dev"}


def _desc(**kw):
    """a descriptor that passes every check (the pointers are host addresses: no check dereferences one)"""
    nat, _ = _lib()
    ok = C.addressof(_MEM) + (-C.addressof(_MEM)) % 16
    d = dict(heads=4, x_elem=0, scale=0.25, rowptr_dev=ok, col_dev=ok, num_targets=3, num_sources=5, C=16, q_dev=ok,
             q_stride_elems=64, k_dev=ok, k_stride_elems=128, v_dev=ok, v_stride_elems=128, out_dev=ok,
             row_max_dev=ok, row_sum_dev=ok, grad_out_dev=ok, grad_q_dev=ok, grad_k_dev=ok, grad_v_dev=ok)
    for k, v in kw.items():
        d[k] = (ok + v if v is not None else None) if k in _PTRS else v
    return nat.TransformerDesc(**d)


NAN = float("nan")
# (descriptor fields, p, a word of the message): the refusals of spp.h f3y in their order with p right after the shape;
# most cases also plant the NEXT stage's fault to show which refusal comes first
REFUSALS = [
    (dict(heads=3), 2.0, "heads"), (dict(heads=0), 0.5, "heads"),
    (dict(x_elem=3), 2.0, "element code"),
    (dict(C=10), 2.0, "C % 4"), (dict(C=0), 0.5, "C % 4"),
    (dict(C=12), 2.0, "power of two"),
    (dict(heads=8, C=256), 2.0, "<= 1024"),
    (dict(num_targets=-1), 2.0, "T <= S"), (dict(num_targets=6), NAN, "T <= S"),      # a bad shape before p
    (dict(), 1.0, "0 <= p < 1"), (dict(), -0.25, "0 <= p < 1"), (dict(), NAN, "0 <= p < 1"), (dict(), 1.5, "0 <= p < 1"),
    (dict(num_targets=0), 1.0, "0 <= p < 1"), (dict(num_targets=0), NAN, "0 <= p < 1"),          # before the T == 0 return
    (dict(q_stride_elems=60), -0.25, "0 <= p < 1"), (dict(k_stride_elems=66), 1.5, "0 <= p < 1"),   # before a bad stride
    (dict(q_dev=None), NAN, "0 <= p < 1"), (dict(rowptr_dev=None), 1.0, "0 <= p < 1"),           # before a NULL row
    (dict(scale=0.0), 1.0, "0 <= p < 1"), (dict(scale=NAN), -0.25, "0 <= p < 1"),                # before a bad scale
    (dict(q_stride_elems=60, q_dev=None), 0.5, "stride"), (dict(v_stride_elems=32), 0.0, "stride"),
    (dict(rowptr_dev=None, k_dev=8), 0.5, "NULL"), (dict(out_dev=None, q_dev=8), 0.5, "NULL"),
    (dict(row_sum_dev=None), 0.6, "NULL"), (dict(v_dev=None), 0.0, "NULL"),
    (dict(q_dev=8, scale=0.0), 0.5, "misaligned"), (dict(v_dev=8), 0.5, "misaligned"), (dict(col_dev=4), 0.6, "misaligned"),
    (dict(scale=0.0), 0.5, "scale"), (dict(scale=-1.0), 0.0, "scale"), (dict(scale=float("inf")), 0.6, "scale"),
    (dict(scale=NAN), 0.5, "scale"),
]


def _refused(entry, fields, p, word, training=1):
    _, L = _lib()
    d = _desc(**fields)
    assert getattr(L, entry)(C.byref(d), None, p, training, 7) == -1, (entry, fields, p)
    msg = L.spp_last_error().decode()
    assert entry in msg and word in msg, (fields, p, msg)


@pytest.mark.parametrize("entry", list(DROP))
def test_refusals_in_the_documented_order(entry):
    _, L = _lib()
    assert getattr(L, entry)(None, None, 0.5, 1, 7) == -1 and "NULL descriptor" in L.spp_last_error().decode()
    for fields, p, word in REFUSALS:
        _refused(entry, fields, p, word)
    for p in (1.0, -0.25, NAN, 1.5):                                          # in eval mode too
        _refused(entry, dict(), p, "0 <= p < 1", training=0)
        _refused(entry, dict(num_targets=0, q_dev=None), p, "0 <= p < 1", training=0)


def test_the_backwards_own_refusals():
    entry = "spp_transformer_backward_drop"
    _refused(entry, dict(grad_out_dev=None), 0.5, "NULL")
    _refused(entry, dict(grad_q_dev=None), 0.5, "NULL")
    _refused(entry, dict(grad_q_dev=None, out_dev=4), 0.5, "NULL")            # NULL pointers before alignment
    _refused(entry, dict(grad_q_dev=None), 1.0, "0 <= p < 1")                 # p before the backward's buffers
    _refused(entry, dict(num_targets=-1, grad_out_dev=None), 1.0, "T <= S")   # the shape before p
    for k in ("grad_out_dev", "grad_q_dev", "grad_k_dev", "grad_v_dev"):
        _refused(entry, {k: 8}, 0.5, "misaligned")
        _refused(entry, {k: 8}, NAN, "0 <= p < 1")
    _refused(entry, dict(grad_k_dev=8, scale=0.0), 0.5, "misaligned")         # alignment before the scale
    _, L = _lib()                                                             # grad_k / grad_v may be NULL: T == 0 below;
    d = _desc(grad_k_dev=None, grad_v_dev=None, num_targets=0)                # (with T > 0 the entry would launch)
    assert L.spp_transformer_backward_drop(C.byref(d), None, 0.5, 1, 7) == 0


def test_no_targets_returns_ok_with_null_buffers():
    _, L = _lib()
    d = _desc(num_targets=0, q_dev=None, k_dev=None, v_dev=None, out_dev=None, rowptr_dev=None, row_max_dev=None,
              row_sum_dev=None, grad_out_dev=None, grad_q_dev=None, grad_k_dev=None, grad_v_dev=None, col_dev=None)
    for entry in DROP:
        for p, training in ((0.6, 1), (0.0, 1), (0.6, 0)):
            assert getattr(L, entry)(C.byref(d), None, p, training, 7) == 0, (entry, p, training)


# ------------------------------------------------------------------------------------------------ the restatement
def _plain_formula(ent, q, k, v, scale, keep, ds):
    """row by row, nothing shared with the helpers; keep [E, H] as the keep rule lays it out (CSR position)"""
    rows = []
    for t in range(ent.T):
        b, e = int(ent.rowptr[t]), int(ent.rowptr[t + 1])
        if b == e:
            rows.append(torch.zeros_like(q[t]))
            continue
        idx = ent.col[b:e]
        e_ = torch.einsum("hc,nhc->nh", q[t], k[idx]) * scale
        rows.append(torch.einsum("nh,nhc->hc", torch.softmax(e_, 0) * keep[b:e].double() * ds, v[idx]))
    return torch.stack(rows)


def _cases_present(ent, keep):
    """the hop has an empty row and a one-entry row, and the mask drops every entry of some (target, head)"""
    dropped = XD.all_dropped(ent, torch.as_tensor(keep))
    assert bool((ent.n == 0).any()) and bool((ent.n == 1).any()) and bool(dropped.any())
    return dropped


@pytest.mark.parametrize("S", [200, 70])
@pytest.mark.parametrize("H", [1, 4])
def test_closed_form_gradients_are_autograds(H, S):
    ent = X.entries_of(X.planted_hop(70, S))
    scale = X.scale32(CC)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-12)   # noqa: E731
    for p in (0.6, 0.5):
        keep, ke = XD.mask(ent, H, p, 11 + H)
        assert keep.shape == (ent.E, H) and 0 < int(keep.sum()) < keep.size
        dropped = _cases_present(ent, keep)
        q, k, v, g = (t.double() for t in X.inputs("model", ent, H, CC, F32))
        bw = XD.backward_drop(ent, q, k, v, g, scale, ke, p)
        empty = ent.n == 0
        assert bool((bw.fw.out[empty] == 0).all()) and bool((bw.fw.b_out[empty] == 0).all())
        assert bool((bw.fw.out[dropped] == 0).all()) and bool((bw.fw.b_out[dropped] == 0).all())
        # autograd of the float64 forward_drop itself
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = XD.forward_drop(ent, *leaves, scale, ke, p).out
        out.backward(g)
        close(bw.fw.out, out.detach())
        for got, leaf in zip((bw.gq, bw.gk, bw.gv), leaves):
            close(got, leaf.grad)
        # and of a row-by-row formula that shares nothing with it
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = _plain_formula(ent, *leaves, scale, torch.from_numpy(keep), XD.scale_of(p))
        out.backward(g)
        close(bw.fw.out, out.detach())
        for got, leaf in zip((bw.gq, bw.gk, bw.gv), leaves):
            close(got, leaf.grad)
        # row_max / row_sum and their bounds are the p = 0 restatement's own
        fw = X.forward(ent, q, k, v, scale)
        assert torch.equal(bw.fw.row_max, fw.row_max) and torch.equal(bw.fw.row_sum, fw.row_sum)
        assert torch.equal(bw.fw.bm, fw.bm) and torch.equal(bw.fw.bs, fw.bs)


def _emu(ent, q, k, v, g, scale, ke, p, fault=None, ke_bwd=None):
    """the dropped formulas in fp32 torch ops over the entry list (two-pass softmax), with a planted fault.
    ke [E, H] float: the mask per entry; ke_bwd: the backward's (another seed's: a fault)"""
    r, s, T, S = ent.row, ent.col, ent.T, ent.S
    H = q.size(1)
    q, k, v = q.float(), k.float(), v.float()
    sc = torch.tensor(scale, dtype=F32)
    ds = torch.tensor(XD.scale_of(p), dtype=F32)
    e = (q[r] * k[s]).sum(2) * sc
    m = torch.full((T, H), -float("inf")).scatter_reduce(0, r.unsqueeze(1).expand(-1, H), e, "amax")
    kf = ke.float()
    kb = kf if ke_bwd is None else ke_bwd.float()
    w = torch.exp(e - m[r])
    ssum = torch.zeros((T, H)).index_add_(0, r, w)
    alpha = w / ssum[r]
    if fault == "renormalised_over_kept":                       # the softmax over the kept entries only, no 1 / (1 - p)
        kept = torch.zeros((T, H)).index_add_(0, r, w * kf)
        fwd_w = torch.where(kf > 0, w / kept[r].clamp(min=1e-30), torch.zeros_like(w))
    else:
        fwd_w = kf * ds * alpha
    out = torch.zeros((T,) + tuple(v.shape[1:])).index_add_(0, r, fwd_w.unsqueeze(2) * v[s])
    go = (g * out).sum(2)
    gh = (g[r] * v[s]).sum(2)
    d = kb * ds
    ge = alpha * (d * gh - go[r])
    if fault == "dropped_send_nothing":                         # ge without the -alpha go term on dropped entries
        ge = torch.where(kb > 0, ge, torch.zeros_like(ge))
    ges = (ge * sc).unsqueeze(2)
    gq = torch.zeros_like(out).index_add_(0, r, ges * k[s])
    gk = torch.zeros((S,) + tuple(k.shape[1:])).index_add_(0, s, ges * q[r])
    gv = torch.zeros((S,) + tuple(v.shape[1:])).index_add_(0, s, (d * alpha).unsqueeze(2) * g[r])
    m = torch.where(ent.n.unsqueeze(1) > 0, m, torch.zeros_like(m))
    return dict(out=out, row_max=m, row_sum=ssum, gq=gq, gk=gk, gv=gv)


def _ratios(got, bw):
    fw = bw.fw
    ref = dict(out=(fw.out, fw.b_out), row_max=(fw.row_max, fw.bm), row_sum=(fw.row_sum, fw.bs), gq=(bw.gq, bw.b_gq),
               gk=(bw.gk, bw.b_gk), gv=(bw.gv, bw.b_gv))
    return {k: X.worst(got[k], *ref[k])[0] for k in ref}


@pytest.mark.parametrize("name", X.REGIMES)
@pytest.mark.parametrize("H", [1, 4])
def test_a_correct_fp32_computation_stays_inside_the_bounds(H, name):
    ent = X.entries_of(X.planted_hop(70, 200))
    scale = X.scale32(CC)
    for p in (0.5, 0.6):
        keep, ke = XD.mask(ent, H, p, 5)
        _cases_present(ent, keep)
        q, k, v, g = X.inputs(name, ent, H, CC, F32)
        bw = XD.backward_drop(ent, q, k, v, g, scale, ke, p)
        ratios = _ratios(_emu(ent, q, k, v, g, scale, ke, p), bw)
        print(f"TRANSFORMER_DROP_HOST {name} H={H} p={p} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("fault", [None, "dropped_send_nothing", "other_seed_in_backward", "renormalised_over_kept"])
def test_a_planted_fault_leaves_the_bounds(fault):
    ent = X.entries_of(X.planted_hop(70, 200))
    H, p, seed = 2, 0.6, 5
    scale = X.scale32(CC)
    keep, ke = XD.mask(ent, H, p, seed)
    _cases_present(ent, keep)
    ke_bwd = XD.mask(ent, H, p, seed + 1)[1] if fault == "other_seed_in_backward" else None
    for name in X.REGIMES:
        q, k, v, g = X.inputs(name, ent, H, CC, F32)
        bw = XD.backward_drop(ent, q, k, v, g, scale, ke, p)
        over = max(_ratios(_emu(ent, q, k, v, g, scale, ke, p, fault, ke_bwd), bw).values())
        if fault is None:
            assert over <= 1.0, (name, over)                   # the emulation itself is inside
        elif over > 1.0:
            return
    assert fault is None, f"{fault}: inside every bound in every regime"
