"""Exact layer-wise inference at papers scale: one ``layerwise_inference`` of SAGE 3 x 256 over make_workload("S-papers")
with bf16 activations, timed per layer, and layer 1's slabs once more through the hop kernel (spp_agg_forward: MEAN,
``rowptr + t0``, the full matrix as the Dense source) for comparison.

    python tools/inference_profile.py [--workload S-papers] [--rows-per-slab 1048576] [--hidden 256] [--json out.json]
    python tools/inference_profile.py --model gat [--heads 4] [--repeats 3] ...
    python tools/inference_profile.py --model gatv2 [--heads 4] [--share-weights] [--repeats 3] ...
    python tools/inference_profile.py --model sageresinception [--nodes 1500000] [--torch-epilogue] [--repeats 3] ...
    python tools/inference_profile.py --model gcn [--repeats 3] ...      (``gcn_leg``: the weighted kernels against the sum)
    python tools/inference_profile.py --evaluate [--repeats 3] ...
    python tools/inference_profile.py --parts 8 --workload S-products [--repeats 5] ...
    python tools/inference_profile.py --parts 8 --model gat --workload S-products [--heads 1] [--repeats 9] ...
    python tools/inference_profile.py --fp8 [--repeats 5] ...

``--model gat``: GAT 3 x hidden at ``--heads`` through spp_graph_gat_forward, ``--repeats`` whole passes in one process
(the first warms up code objects and the GEMM library's choices; every pass is reported).  Its bytes are the mean's plus
the logits: 4 * H per entry (a_src) and 8 * H per target (a_src of the self loop, a_dst).

``--model gatv2``: GATv2 3 x hidden at ``--heads`` (1, 2, 4 or 8; ``--share-weights``) through spp_graph_gatv2_forward inside
``gatv2_inference``, passes as for gat.  Run it in the same session as ``--model gat`` at the same heads and width, which is its
yardstick.  At S-papers the last layer's projected rows are [N, heads * Cp] twice (172 classes pad to Cp = 256): heads = 1, or
``--share-weights`` with fewer classes, is what fits one device (inference._gatv2_layer has the arithmetic).
``--model transformer``: GraphTransformer 3 x hidden at ``--heads`` (``--beta``: the gated skip) through
spp_graph_transformer_forward inside ``layerwise_inference``, passes as for gatv2.  Five [N, hidden] matrices are live
(inference._transformer_layer has the arithmetic): S-papers at hidden 256 does not fit one device.

``--model sageresinception``: SAGEResInception 3 x hidden scored at a random sample of ``--nodes`` nodes; per layer the
aggregation seconds as above, the epilogue seconds (events around every spp_resinc_epilogue call, summed; bytes: z, the
residual row and the output row, bf16 each), the whole layer (layer 3's includes the head) and the whole call.
``--torch-epilogue`` runs the same pass with the layer tail restated as torch ops, the kernel's yardstick.

``--evaluate``: the same SAGE 3 x hidden through ``evaluate`` with random labels (a fifth of them -1).  Events around every
``classify_rows`` call, summed (algorithmic bytes: rows * C * sizeof + 16 * rows), and around the torch tail it replaces,
run on the same tile in the same pass right behind it (both behind a 300 us spin kernel, so that the device finds them
queued and the events time the device, not the host): ``log_softmax(dtype=float32)``, the copy into a [tile, C] fp32
buffer, ``argmax`` and ``nll_loss`` of that buffer.  Before the timed passes, ``torch.cuda.max_memory_allocated`` above the
baseline for one ``evaluate`` and for one ``layerwise_inference`` followed by ``argmax``.

``--parts P``: the cost of the owner lookup.  The workload's matrix cut into P equal row ranges, each copied into an
allocation of its own on the one GPU, and every slab's MEAN aggregated twice: ``spp_graph_agg_forward`` on the whole
matrix (the baseline) and ``spp_graph_agg_parts_forward`` on the parts, at the table's own width (fp16) and at ``--hidden``
(bf16 rows); ``--repeats`` alternating passes after one warm-up pass of each, every pass reported, the ratio taken
between the medians.  One slab's outputs are compared bit for bit first.

``--parts P --model gat``: the same for the attention.  A random bf16 h [N, hidden] and fp32 logits [N, 2 * heads], cut
into P equal row ranges, an allocation per part and kind; every slab attended twice: ``spp_graph_gat_forward`` on the
whole matrices and ``spp_graph_gat_parts_forward`` on the parts, alternating, after one slab is compared bit for bit.

``--fp8``: layer 1's aggregation from an fp8 table read in place.  The workload's fp16 table quantised to e4m3 on the
device (``fp8.quantize_e4m3``), and every slab's OPERAND aggregation with a bf16 output -- SAGE's first layer as the driver
launches it -- run twice: ``spp_graph_agg_forward`` on the fp16 table (the baseline; its kernels are the parent commit's,
instruction for instruction) and ``spp_graph_agg_forward_fp8`` on the e4m3 table; ``--repeats`` alternating passes after one
warm-up pass of each, every pass reported, the ratio taken between the medians.  Then the whole table once through
``spp_fp8_rows_f32`` in the drivers' GEMM tiles (what GAT's first projection reads).

Per layer: seconds of the aggregation alone (events around every slab's launch, the drivers' ``inference._agg_launch`` /
``_gat_launch`` replaced by a timed one for the run, summed), edges/s, and the algorithmic bytes/s
E * F * s (rows) + 16 * T + 8 * E (indices) + T * W * s_out (output); plus the seconds of the whole layer (aggregation,
GEMM, activation write).  Also the maximum degree and the share of rows and entries above C."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-papers")
    ap.add_argument("--rows-per-slab", type=int, default=1 << 20)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--classes", type=int, default=172)
    ap.add_argument("--json", default=None)
    ap.add_argument("--model", choices=("sage", "gat", "gatv2", "transformer", "sageresinception", "gcn"), default="sage")
    ap.add_argument("--beta", action="store_true", help="transformer: every conv's beta gate (torch ops per slab)")
    ap.add_argument("--share-weights", action="store_true", help="gatv2: lin_r is lin_l (one projection, x_r = x_l)")
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1_500_000, help="sageresinception: nodes scored (0 = all)")
    ap.add_argument("--torch-epilogue", action="store_true", help="sageresinception: the layer tail as torch ops")
    ap.add_argument("--evaluate", action="store_true", help="sage: the pass through evaluate, its tail against the torch tail")
    ap.add_argument("--parts", type=int, default=0, help="P > 0: time the aggregation over P row ranges against the whole matrix")
    ap.add_argument("--fp8", action="store_true", help="time layer 1's aggregation from the table as fp8, read in place, against fp16")
    a = ap.parse_args()
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import SAGE, _agg_forward
    from salient_plusplus_amd.synthetic import make_workload
    dev = torch.device("cuda", 0)
    t0 = time.time()
    wl = make_workload(a.workload, device=dev)
    torch.cuda.synchronize()
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, E, Cc = wl.num_nodes, col.numel(), inf.graph_agg_chunk()
    deg = rowptr[1:] - rowptr[:-1]
    long_rows = deg > Cc
    res = {"workload": a.workload, "nodes": N, "entries": E, "chunk": Cc, "max_degree": int(deg.max()),
           "rows_above_chunk": int(long_rows.sum()), "entries_above_chunk": int(deg[long_rows].sum()),
           "rows_per_slab": a.rows_per_slab, "build_s": round(time.time() - t0, 1), "layers": []}
    del deg, long_rows
    print(json.dumps({k: v for k, v in res.items() if k != "layers"}), flush=True)
    if a.fp8:
        return fp8_leg(a, wl, res)
    if a.parts > 0:
        return gat_parts_leg(a, wl, res) if a.model == "gat" else parts_leg(a, wl, res)
    if a.model == "gat":
        return gat_leg(a, wl, res)
    if a.model == "gatv2":
        return gatv2_leg(a, wl, res)
    if a.model == "transformer":
        return transformer_leg(a, wl, res)
    if a.model == "sageresinception":
        return resinc_leg(a, wl, res)
    if a.model == "gcn":
        return gcn_leg(a, wl, res)
    if a.evaluate:
        return evaluate_leg(a, wl, res)

    # the aggregation of every slab, timed by events inside the one layerwise_inference call
    spans = []
    inner = inf._agg_launch

    def timed(xm, *args, **kw):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        out = inner(xm, *args, **kw)
        e.record()
        spans.append((xm.size(1), xm.element_size(), out.size(0), out.size(1) * out.element_size(), b, e))
        return out
    inf._agg_launch = timed
    torch.manual_seed(0)
    model = SAGE(x.size(1), a.hidden, a.classes, 3).to(dev)
    torch.cuda.synchronize()
    t0 = time.time()
    out = inf.layerwise_inference(model, x, rowptr, col, rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    res["total_s"] = round(time.time() - t0, 3)
    inf._agg_launch = inner
    assert out.shape == (N, a.classes) and bool(torch.isfinite(out[:: max(1, N // 4096)]).all())
    del out
    slabs = -(-N // a.rows_per_slab)
    for layer in range(3):
        part = spans[layer * slabs:(layer + 1) * slabs]
        F_, s_in = part[0][0], part[0][1]
        agg_s = sum(b.elapsed_time(e) for *_x, b, e in part) / 1e3
        nbytes = E * F_ * s_in + 16 * N + 8 * E + sum(T * w for _f, _s, T, w, _b, _e in part)
        res["layers"].append({"layer": layer + 1, "F": F_, "x_bytes_per_elem": s_in, "agg_s": round(agg_s, 4),
                              "edges_per_s": round(E / agg_s), "algorithmic_TBps": round(nbytes / agg_s / 1e12, 3)})
        print(json.dumps(res["layers"][-1]), flush=True)

    # layer 1's slabs through the hop kernel: lpr lanes walk each row serially, whatever its length
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hop_s, worst = 0.0, (0.0, 0)
    for s in range(0, N, a.rows_per_slab):
        T = min(a.rows_per_slab, N - s)
        b.record()
        o = _agg_forward(nat.SPP_AGG_MEAN, rowptr[s:], col, T, x, torch.bfloat16)
        e.record()
        e.synchronize()
        ms = b.elapsed_time(e)
        hop_s += ms / 1e3
        worst = max(worst, (ms / 1e3, s))
        del o
    res["layer1_hop_kernel_s"] = round(hop_s, 4)
    res["layer1_hop_kernel_worst_slab"] = {"row0": worst[1], "s": round(worst[0], 4)}
    print(json.dumps({k: res[k] for k in ("total_s", "layer1_hop_kernel_s", "layer1_hop_kernel_worst_slab")}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def gcn_leg(a, wl, res):
    """``--model gcn``: (1) the weighted kernel pair against the plain sum on the same rows -- every slab of the table
    (F = 128 fp16 -> fp32) through ``graph_aggregate(epilogue="sum")``, ``graph_weighted_aggregate()`` (weights of one)
    and ``graph_weighted_aggregate(dinv=...)`` (gcn_norm formed in the kernel), one warm-up pass over all slabs and then
    ``--repeats`` passes with the three alternating slab by slab, events around each call, the median pass per variant;
    (2) one ``layerwise_inference`` of GCN 3 x hidden (bf16 activations), ``normalize`` False and True, next to SAGE's
    on the same graph in the same process, the median of ``--repeats`` each after a warm-up"""
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GCN, SAGE
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, dev = x.size(0), x.device
    res.update(model="gcn", F=x.size(1), x_bytes_per_elem=x.element_size())
    ws = torch.empty(inf.graph_agg_workspace_bytes(min(a.rows_per_slab, N)), dtype=torch.uint8, device=dev)
    out = torch.empty((min(a.rows_per_slab, N), x.size(1)), dtype=torch.float32, device=dev)
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    dinv = inf.gcn_dinv(rowptr)
    e.record()
    e.synchronize()
    res["gcn_dinv_s"] = round(b.elapsed_time(e) / 1e3, 4)
    variants = {
        "sum": lambda s, T: inf.graph_aggregate(x, rowptr, col, row0=s, num_targets=T, epilogue="sum", workspace=ws),
        "weighted_ones": lambda s, T: inf.graph_weighted_aggregate(x, rowptr, col, row0=s, num_targets=T, out=out[:T],
                                                                   workspace=ws),
        "weighted_dinv": lambda s, T: inf.graph_weighted_aggregate(x, rowptr, col, dinv=dinv, fill=1, row0=s,
                                                                   num_targets=T, out=out[:T], workspace=ws),
    }
    passes = {k: [] for k in variants}
    for p in range(a.repeats + 1):                        # pass 0 warms up
        tot = dict.fromkeys(variants, 0.0)
        for s in range(0, N, a.rows_per_slab):
            T = min(a.rows_per_slab, N - s)
            for k, fn in variants.items():
                b.record()
                o = fn(s, T)
                e.record()
                e.synchronize()
                tot[k] += b.elapsed_time(e) / 1e3
                del o
        if p:
            for k in variants:
                passes[k].append(round(tot[k], 4))
    med = {k: sorted(v)[len(v) // 2] for k, v in passes.items()}
    res["kernel_passes_s"], res["kernel_median_s"] = passes, med
    res["ratio_ones_over_sum"] = round(med["weighted_ones"] / med["sum"], 3)
    res["ratio_dinv_over_sum"] = round(med["weighted_dinv"] / med["sum"], 3)
    print(json.dumps({k: res[k] for k in ("gcn_dinv_s", "kernel_median_s", "ratio_ones_over_sum", "ratio_dinv_over_sum")}),
          flush=True)
    del out, dinv
    torch.manual_seed(0)
    models = {"sage": SAGE(x.size(1), a.hidden, a.classes, 3), "gcn": GCN(x.size(1), a.hidden, a.classes, 3),
              "gcn_normalize": GCN(x.size(1), a.hidden, a.classes, 3, normalize=True)}
    res["layerwise_inference_s"] = {}
    for name, model in models.items():
        model = model.to(dev)
        times = []
        for p in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.time()
            lp = inf.layerwise_inference(model, x, rowptr, col, rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)
            torch.cuda.synchronize()
            if p:
                times.append(round(time.time() - t0, 3))
            assert lp.shape == (N, a.classes)
            del lp
        res["layerwise_inference_s"][name] = {"passes": times, "median": sorted(times)[len(times) // 2]}
        print(json.dumps({name: res["layerwise_inference_s"][name]}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def _torch_tail(z, scale, shift, *, negative_slope, residual=None, row0=None, row_ids=None, out=None, out_dtype=None):
    """resinc_epilogue's contract restated as torch ops (the yardstick of --torch-epilogue): the affine BatchNorm, the
    leaky_relu, the residual rows and the write into the slab, each its own element-wise pass"""
    y = torch.nn.functional.leaky_relu(z.float() * scale + shift, negative_slope)
    if residual is not None:
        y += (residual[row_ids] if row_ids is not None else residual[row0:row0 + z.size(0)]).float()
    out.copy_(y)
    return out


def resinc_leg(a, wl, res):
    """SAGEResInception 3 x hidden, bf16 activations, scored at a sample of ``--nodes`` nodes (``acc`` for all N does
    not fit at papers scale): per layer the aggregation and the epilogue (events around every call, summed), the whole
    layer, and the whole call; ``--repeats`` passes, the first a warm-up"""
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import SAGEResInception
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, L = wl.num_nodes, 3
    res.update(model="sageresinception", torch_epilogue=bool(a.torch_epilogue), passes=[])
    res.pop("layers")
    torch.manual_seed(0)
    nodes = torch.randperm(N, device=x.device)[:min(a.nodes, N)] if a.nodes > 0 else None
    res["scored_nodes"] = int(nodes.numel()) if nodes is not None else N
    model = SAGEResInception(x.size(1), a.hidden, a.classes, L).to(x.device)
    agg, epi, marks = [], [], []
    inner_agg, inner_epi = inf._agg_launch, inf.resinc_epilogue
    tail = _torch_tail if a.torch_epilogue else inner_epi

    def timed(fn, spans):
        def call(first, *args, **kw):
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            out = fn(first, *args, **kw)
            e.record()
            spans.append((first.size(0), b, e))
            return out
        return call

    def timed_agg(xm, *args, **kw):                       # a layer begins with the first slab's aggregation of a matrix
        if not marks or marks[-1][0] != xm.data_ptr():
            m = torch.cuda.Event(enable_timing=True)
            m.record()
            marks.append((xm.data_ptr(), len(agg), len(epi), m))
        return timed(inner_agg, agg)(xm, *args, **kw)
    inf._agg_launch, inf.resinc_epilogue = timed_agg, timed(tail, epi)
    try:
        for rep in range(a.repeats):
            del agg[:], epi[:], marks[:]
            torch.cuda.synchronize()
            t0 = time.time()
            out = inf.layerwise_inference(model, x, rowptr, col, nodes=nodes, rows_per_slab=a.rows_per_slab,
                                          act_dtype=torch.bfloat16)
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            torch.cuda.synchronize()
            one = {"pass": rep, "total_s": round(time.time() - t0, 3), "layers": []}
            assert out.shape == (res["scored_nodes"], a.classes) and bool(torch.isfinite(out[:: max(1, out.size(0) // 4096)]).all())
            del out
            assert len(marks) == L, len(marks)
            for k, (_ptr, a0, e0, m) in enumerate(marks):
                a1, e1, nxt = (marks[k + 1][1], marks[k + 1][2], marks[k + 1][3]) if k + 1 < L else (len(agg), len(epi), end)
                rows = sum(n for n, _b, _e in epi[e0:e1])
                epi_s = sum(b.elapsed_time(e) for _n, b, e in epi[e0:e1]) / 1e3
                # z, the residual row and the output row, bf16 each (layer 1: the residual is the tile's other half)
                one["layers"].append({"layer": k + 1, "rows": rows, "epilogue_calls": e1 - e0,
                                      "agg_s": round(sum(b.elapsed_time(e) for _n, b, e in agg[a0:a1]) / 1e3, 4),
                                      "epilogue_s": round(epi_s, 4),
                                      "epilogue_algorithmic_TBps": round(3 * 2 * rows * a.hidden / epi_s / 1e12, 3),
                                      "layer_s": round(m.elapsed_time(nxt) / 1e3, 4)})
            res["passes"].append(one)
            print(json.dumps(one), flush=True)
    finally:
        inf._agg_launch, inf.resinc_epilogue = inner_agg, inner_epi
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def evaluate_leg(a, wl, res):
    """SAGE 3 x hidden, bf16 activations, through ``evaluate``: peak memory against ``layerwise_inference`` + argmax
    first (one untimed pass each, which also warms up), then ``--repeats`` passes with every ``classify_rows`` call and
    the torch tail on the same tile timed by events"""
    import torch.nn.functional as F
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import SAGE
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, dev = wl.num_nodes, x.device
    res.update(model="sage", evaluate=True, classes=a.classes, passes=[])
    res.pop("layers")
    torch.manual_seed(0)
    model = SAGE(x.size(1), a.hidden, a.classes, 3).to(dev)
    y = torch.randint(0, a.classes, (N,), device=dev)
    y[::5] = -1
    kw = dict(rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base, round(time.time() - t0, 3)

    ev, ev_peak, ev_s = peak(lambda: inf.evaluate(model, x, rowptr, col, y, **kw))
    pred = ev.pred
    res["evaluate"] = {"peak_bytes_above_baseline": ev_peak, "first_pass_s": ev_s, "labelled": ev.labelled,
                       "correct": ev.correct, "loss": ev.loss}
    del ev
    lp_pred, lp_peak, lp_s = peak(lambda: inf.layerwise_inference(model, x, rowptr, col, **kw).argmax(-1))
    res["layerwise_inference_then_argmax"] = {"peak_bytes_above_baseline": lp_peak, "first_pass_s": lp_s,
                                              "matrix_bytes": N * a.classes * 4,
                                              "pred_equal_to_evaluate": bool(torch.equal(lp_pred, pred))}
    del lp_pred, pred
    print(json.dumps({k: res[k] for k in ("evaluate", "layerwise_inference_then_argmax")}), flush=True)

    # With an idle device an event pair times the host's way through the wrapper, not the kernel: a spin kernel of about
    # 300 us ahead of every timed tile keeps the queue full while the host enqueues both tails behind it.
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    b.record()
    torch.cuda._sleep(20_000_000)
    e.record()
    e.synchronize()
    spin = int(300e-6 * 20_000_000 / (b.elapsed_time(e) / 1e3))
    res["spin_cycles_per_tile"] = spin
    spans = []
    inner = inf.classify_rows
    buf = torch.empty((inf._GEMM_ROWS, a.classes), dtype=torch.float32, device=dev)      # the tile's rows of ``out``
    wrong = torch.zeros((), dtype=torch.int64, device=dev)

    def timed(z, labels=None, *, row0=None, **kw2):
        ev3 = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda._sleep(spin)
        ev3[0].record()
        out = inner(z, labels, row0=row0, **kw2)
        ev3[1].record()
        rows = buf[:z.size(0)]
        rows.copy_(torch.log_softmax(z, dim=-1, dtype=torch.float32))
        p = rows.argmax(-1)
        F.nll_loss(rows, labels[row0:row0 + z.size(0)], ignore_index=-1, reduction="none")
        ev3[2].record()
        wrong.add_((p != out[0]).sum())
        spans.append((z.size(0), z.size(1), z.element_size(), ev3))
        return out
    inf.classify_rows = timed
    try:
        for rep in range(a.repeats):
            del spans[:]
            wrong.zero_()
            torch.cuda.synchronize()
            t0 = time.time()
            ev = inf.evaluate(model, x, rowptr, col, y, **kw)
            torch.cuda.synchronize()
            total = time.time() - t0
            k_s = sum(e[0].elapsed_time(e[1]) for *_x, e in spans) / 1e3
            t_s = sum(e[1].elapsed_time(e[2]) for *_x, e in spans) / 1e3
            nbytes = sum(n * Cn * es + 16 * n for n, Cn, es, _e in spans)
            one = {"pass": rep, "total_s_with_both_tails_and_spins": round(total, 3), "calls": len(spans),
                   "rows": sum(n for n, *_r in spans), "classify_rows_s": round(k_s, 5), "torch_tail_s": round(t_s, 5),
                   "torch_over_kernel": round(t_s / k_s, 2), "algorithmic_bytes": nbytes,
                   "classify_rows_algorithmic_TBps": round(nbytes / k_s / 1e12, 3),
                   "fraction_of_8_TBps_hbm_peak": round(nbytes / k_s / 8e12, 3),
                   "rows_where_torch_argmax_differs": int(wrong), "correct": ev.correct, "loss": ev.loss}
            res["passes"].append(one)
            print(json.dumps(one), flush=True)
            del ev
    finally:
        inf.classify_rows = inner
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


SWEEPS = 10     # sweeps over all slabs inside one timed window of the --parts leg (seconds are per sweep)


def parts_leg(a, wl, res):
    from salient_plusplus_amd import inference as inf
    rowptr, col = wl.rowptr, wl.col
    N, E, P = wl.num_nodes, col.numel(), a.parts
    off = [N * p // P for p in range(P + 1)]
    res.update(parts=P, part_offsets=off, widths=[])
    res.pop("layers")
    ws = torch.empty(inf.graph_agg_workspace_bytes(min(a.rows_per_slab, N)), dtype=torch.uint8, device=rowptr.device)
    torch.manual_seed(0)
    for x in (wl.x, torch.randn((N, a.hidden), device=rowptr.device).to(torch.bfloat16)):
        stride = x.stride(0)
        parts = []
        for p in range(P):                               # an allocation per part, rows as far apart as the matrix's
            buf = torch.empty((off[p + 1] - off[p], stride), dtype=x.dtype, device=x.device)[:, :x.size(1)]
            buf.copy_(x[off[p]:off[p + 1]])
            parts.append(buf)
        slabs = [(s, min(a.rows_per_slab, N - s)) for s in range(0, N, a.rows_per_slab)]

        def whole(s, T):
            return inf.graph_aggregate(x, rowptr, col, row0=s, num_targets=T, out_dtype=torch.bfloat16, workspace=ws)

        def parted(s, T):
            return inf.graph_aggregate_parts(parts, off, rowptr, col, row0=s, num_targets=T, out_dtype=torch.bfloat16,
                                             workspace=ws)
        s0, T0 = slabs[len(slabs) // 2]
        assert torch.equal(whole(s0, T0).view(torch.int16), parted(s0, T0).view(torch.int16)), "the parts change bits"
        times = {"whole": [], "parts": []}
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(a.repeats + 1):                 # (pass 0 warms up both)
            for name, fn in (("whole", whole), ("parts", parted)):
                torch.cuda.synchronize()
                b.record()
                for _sweep in range(SWEEPS):
                    for s, T in slabs:
                        fn(s, T)
                e.record()
                e.synchronize()
                if rep:
                    times[name].append(round(b.elapsed_time(e) / 1e3 / SWEEPS, 6))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        nbytes = E * x.size(1) * x.element_size() + 16 * N + 8 * E + N * x.size(1) * 2
        one = {"F": x.size(1), "x_dtype": str(x.dtype), "x_stride_elems": stride, "whole_s": times["whole"],
               "parts_s": times["parts"], "whole_median_s": med["whole"], "parts_median_s": med["parts"],
               "ratio_parts_over_whole": round(med["parts"] / med["whole"], 4),
               "whole_algorithmic_TBps": round(nbytes / med["whole"] / 1e12, 3)}
        res["widths"].append(one)
        print(json.dumps(one), flush=True)
        del parts
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def fp8_leg(a, wl, res):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd import inference as inf
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, E, F_ = wl.num_nodes, col.numel(), wl.x.size(1)
    res.pop("layers")
    t0 = time.time()
    x8 = inf.Fp8Table(fp8.quantize_e4m3(x))
    torch.cuda.synchronize()
    res.update(fp8=True, F=F_, quantise_s=round(time.time() - t0, 1), epilogue="operand", out_dtype="bfloat16")
    ws = torch.empty(inf.graph_agg_workspace_bytes(min(a.rows_per_slab, N)), dtype=torch.uint8, device=x.device)
    slabs = [(s, min(a.rows_per_slab, N - s)) for s in range(0, N, a.rows_per_slab)]
    out = torch.empty((min(a.rows_per_slab, N), 2 * F_), dtype=torch.bfloat16, device=x.device)

    def run(table):
        for s, T in slabs:
            inf._agg_launch(table, rowptr, col, "operand", 0.0, s, None, T, out[:T], ws)
    times = {"fp16": [], "fp8": []}
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(a.repeats + 1):                     # (pass 0 warms up both)
        for name, table in (("fp16", x), ("fp8", x8)):
            torch.cuda.synchronize()
            b.record()
            run(table)
            e.record()
            e.synchronize()
            assert bool(torch.isfinite(out[:: max(1, out.size(0) // 4096)].float()).all())
            if rep:
                times[name].append(round(b.elapsed_time(e) / 1e3, 5))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    nbytes = {k: (E + N) * F_ * w + 16 * N + 8 * E + N * 2 * F_ * 2 for k, w in (("fp16", 2), ("fp8", 1))}
    res.update(fp16_s=times["fp16"], fp8_s=times["fp8"], fp16_median_s=med["fp16"], fp8_median_s=med["fp8"],
               ratio_fp8_over_fp16=round(med["fp8"] / med["fp16"], 4),
               fp16_algorithmic_TBps=round(nbytes["fp16"] / med["fp16"] / 1e12, 3),
               fp8_algorithmic_TBps=round(nbytes["fp8"] / med["fp8"] / 1e12, 3))
    # the whole table as the drivers' fp32 GEMM tiles (one buffer: the tiles' consumer is not what is timed)
    tile = torch.empty((inf._GEMM_ROWS, F_), dtype=torch.float32, device=x.device)
    tiles_s = []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize()
        b.record()
        for r in range(0, N, inf._GEMM_ROWS):
            x8.rows_f32(tile[:min(inf._GEMM_ROWS, N - r)], r)
        e.record()
        e.synchronize()
        if rep:
            tiles_s.append(round(b.elapsed_time(e) / 1e3, 5))
    tmed = sorted(tiles_s)[len(tiles_s) // 2]
    res.update(rows_f32_s=tiles_s, rows_f32_median_s=tmed, rows_f32_algorithmic_TBps=round(N * F_ * 5 / tmed / 1e12, 3))
    print(json.dumps({k: v for k, v in res.items() if k.startswith(("fp", "ratio", "rows_f32", "quant"))}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def gat_parts_leg(a, wl, res):
    from salient_plusplus_amd import inference as inf
    rowptr, col = wl.rowptr, wl.col
    dev = rowptr.device
    N, E, P, H = wl.num_nodes, col.numel(), a.parts, a.heads
    off = [N * p // P for p in range(P + 1)]
    res.update(model="gat", heads=H, chunk=inf.graph_gat_chunk(), parts=P, part_offsets=off)
    res.pop("layers")
    ws = torch.empty(inf.graph_gat_workspace_bytes(min(a.rows_per_slab, N)), dtype=torch.uint8, device=dev)
    torch.manual_seed(0)
    h = torch.randn((N, a.hidden), device=dev).to(torch.bfloat16)
    logits = torch.randn((N, 2 * H), device=dev)
    a_src, a_dst = logits[:, :H].contiguous(), logits[:, H:].contiguous()

    def cut(m):                                          # an allocation per part, rows as far apart as the matrix's
        parts = []
        for p in range(P):
            buf = torch.empty((off[p + 1] - off[p], m.stride(0)), dtype=m.dtype, device=dev)[:, :m.size(1)]
            buf.copy_(m[off[p]:off[p + 1]])
            parts.append(buf)
        return parts
    hp, lp = cut(h), cut(logits)
    del logits
    slabs = [(s, min(a.rows_per_slab, N - s)) for s in range(0, N, a.rows_per_slab)]
    kw = dict(heads=H, relu=True, out_dtype=torch.bfloat16, workspace=ws)

    def whole(s, T):
        return inf.graph_gat_aggregate(h, a_src, a_dst, rowptr, col, row0=s, num_targets=T, **kw)

    def parted(s, T):
        return inf.graph_gat_aggregate_parts(hp, lp, off, rowptr, col, row0=s, num_targets=T, **kw)
    s0, T0 = slabs[len(slabs) // 2]
    assert torch.equal(whole(s0, T0).view(torch.int16), parted(s0, T0).view(torch.int16)), "the parts change bits"
    times = {"whole": [], "parts": []}
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(a.repeats + 1):                     # (pass 0 warms up both)
        for name, fn in (("whole", whole), ("parts", parted)):
            torch.cuda.synchronize()
            b.record()
            for _sweep in range(SWEEPS):
                for s, T in slabs:
                    fn(s, T)
            e.record()
            e.synchronize()
            if rep:
                times[name].append(round(b.elapsed_time(e) / 1e3 / SWEEPS, 6))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    nbytes = E * a.hidden * 2 + 16 * N + 8 * E + N * a.hidden * 2 + 4 * H * E + 8 * H * N
    res.update(F=a.hidden, x_dtype=str(h.dtype), x_stride_elems=h.stride(0), whole_s=times["whole"],
               parts_s=times["parts"], whole_median_s=med["whole"], parts_median_s=med["parts"],
               ratio_parts_over_whole=round(med["parts"] / med["whole"], 4),
               whole_algorithmic_TBps=round(nbytes / med["whole"] / 1e12, 3))
    print(json.dumps({k: res[k] for k in ("F", "heads", "whole_s", "parts_s", "whole_median_s", "parts_median_s",
                                          "ratio_parts_over_whole", "whole_algorithmic_TBps")}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def gat_leg(a, wl, res):
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GAT
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, E, H = wl.num_nodes, col.numel(), a.heads
    res.update(model="gat", heads=H, chunk=inf.graph_gat_chunk(), passes=[])
    spans = []
    inner = inf._gat_launch

    def timed(h, *args):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        out = inner(h, *args)
        e.record()
        spans.append((h.size(1), h.element_size(), out.size(0), out.size(1) * out.element_size(), b, e))
        return out
    inf._gat_launch = timed
    torch.manual_seed(0)
    model = GAT(x.size(1), a.hidden, a.classes, 3, heads=H).to(x.device)
    slabs = -(-N // a.rows_per_slab)
    for rep in range(a.repeats):
        del spans[:]
        torch.cuda.synchronize()
        t0 = time.time()
        out = inf.layerwise_inference(model, x, rowptr, col, rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        one = {"pass": rep, "total_s": round(time.time() - t0, 3), "layers": []}
        assert out.shape == (N, a.classes) and bool(torch.isfinite(out[:: max(1, N // 4096)]).all())
        del out
        for layer in range(3):
            part = spans[layer * slabs:(layer + 1) * slabs]
            F_, s_in = part[0][0], part[0][1]
            agg_s = sum(b.elapsed_time(e) for *_x, b, e in part) / 1e3
            nbytes = E * F_ * s_in + 16 * N + 8 * E + sum(T * w for _f, _s, T, w, _b, _e in part) + 4 * H * E + 8 * H * N
            one["layers"].append({"layer": layer + 1, "F": F_, "x_bytes_per_elem": s_in, "agg_s": round(agg_s, 4),
                                  "edges_per_s": round(E / agg_s), "algorithmic_TBps": round(nbytes / agg_s / 1e12, 3)})
        res["passes"].append(one)
        print(json.dumps(one), flush=True)
    inf._gat_launch = inner
    res.pop("layers")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def gatv2_leg(a, wl, res):
    """``gat_leg`` for GATv2: the slabs' ``inference._gatv2_launch`` timed inside whole ``gatv2_inference`` passes.  The
    bytes: the entries' rows of x_l, per target its rows of x_l (the self loop) and x_r, the indices and the output."""
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GATv2
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, E, H = wl.num_nodes, col.numel(), a.heads
    res.update(model="gatv2", heads=H, share_weights=bool(a.share_weights), chunk=inf.graph_gatv2_chunk(), passes=[])
    spans = []
    inner = inf._gatv2_launch

    def timed(x_l, *args):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        out = inner(x_l, *args)
        e.record()
        spans.append((x_l.size(1), x_l.element_size(), out.size(0), out.size(1) * out.element_size(), b, e))
        return out
    inf._gatv2_launch = timed
    torch.manual_seed(0)
    model = GATv2(x.size(1), a.hidden, a.classes, 3, heads=H, share_weights=a.share_weights).to(x.device)
    slabs = -(-N // a.rows_per_slab)
    for rep in range(a.repeats):
        del spans[:]
        torch.cuda.synchronize()
        t0 = time.time()
        out = inf.gatv2_inference(model, x, rowptr, col, rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        one = {"pass": rep, "total_s": round(time.time() - t0, 3), "layers": []}
        assert out.shape == (N, a.classes) and bool(torch.isfinite(out[:: max(1, N // 4096)]).all())
        del out
        for layer in range(3):
            part = spans[layer * slabs:(layer + 1) * slabs]
            F_, s_in = part[0][0], part[0][1]                # (the last layer's F is heads * the padded classes)
            agg_s = sum(b.elapsed_time(e) for *_x, b, e in part) / 1e3
            nbytes = (E + 2 * N) * F_ * s_in + 16 * N + 8 * E + sum(T * w for _f, _s, T, w, _b, _e in part)
            one["layers"].append({"layer": layer + 1, "F": F_, "x_bytes_per_elem": s_in, "agg_s": round(agg_s, 4),
                                  "edges_per_s": round(E / agg_s), "algorithmic_TBps": round(nbytes / agg_s / 1e12, 3)})
        res["passes"].append(one)
        print(json.dumps(one), flush=True)
    inf._gatv2_launch = inner
    res.pop("layers")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def transformer_leg(a, wl, res):
    """``gatv2_leg`` for GraphTransformer: the slabs' ``inference._transformer_launch`` timed inside whole
    ``layerwise_inference`` passes.  The bytes: the entries' rows of k and v, per target its rows of q and (when the
    kernel adds it) skip, the indices and the output."""
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import GraphTransformer
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N, E, H = wl.num_nodes, col.numel(), a.heads
    res.update(model="transformer", heads=H, beta=bool(a.beta), chunk=inf.graph_transformer_chunk(), passes=[])
    spans = []
    inner = inf._transformer_launch

    def timed(q, k, v, skip, *args):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        out = inner(q, k, v, skip, *args)
        e.record()
        spans.append((q.size(1), q.element_size(), out.size(0), out.size(1) * out.element_size(), skip is not None, b, e))
        return out
    inf._transformer_launch = timed
    torch.manual_seed(0)
    model = GraphTransformer(x.size(1), a.hidden, a.classes, 3, heads=H, beta=a.beta).to(x.device)
    slabs = -(-N // a.rows_per_slab)
    for rep in range(a.repeats):
        del spans[:]
        torch.cuda.synchronize()
        t0 = time.time()
        out = inf.layerwise_inference(model, x, rowptr, col, rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        one = {"pass": rep, "total_s": round(time.time() - t0, 3), "layers": []}
        assert out.shape == (N, a.classes) and bool(torch.isfinite(out[:: max(1, N // 4096)]).all())
        del out
        for layer in range(3):
            part = spans[layer * slabs:(layer + 1) * slabs]
            F_, s_in, fused = part[0][0], part[0][1], part[0][4]      # (the last layer's F is heads * the padded classes)
            agg_s = sum(b.elapsed_time(e) for *_x, b, e in part) / 1e3
            nbytes = (2 * E + (2 if fused else 1) * N) * F_ * s_in + 16 * N + 8 * E + sum(p[2] * p[3] for p in part)
            one["layers"].append({"layer": layer + 1, "F": F_, "x_bytes_per_elem": s_in, "agg_s": round(agg_s, 4),
                                  "edges_per_s": round(E / agg_s), "algorithmic_TBps": round(nbytes / agg_s / 1e12, 3)})
        one["kernel_s"] = round(sum(l["agg_s"] for l in one["layers"]), 4)
        one["kernel_share"] = round(one["kernel_s"] / one["total_s"], 3)
        res["passes"].append(one)
        print(json.dumps(one), flush=True)
    inf._transformer_launch = inner
    res.pop("layers")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
