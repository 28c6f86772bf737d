"""Scoring a few nodes exactly: ``layerwise_inference(nodes=ids)`` (every layer but the last over all N nodes: the
baseline) against ``field_inference(ids)`` through a reused ``ReceptiveFields`` (the nodes within L - 1 hops only), for a
SAGE 3 x hidden model with bf16 activations and ``--nodes`` random nodes of a synthetic workload.

    python tools/field_inference_profile.py --workload S-products [--nodes 1024] [--repeats 3] [--json out.json]
    python tools/field_inference_profile.py --workload S-papers --json profiles/field_inference_papers.json

One warm-up call of each (code objects, the GEMM library's choices, the allocator's pool), then ``--repeats`` alternating
pairs; every call is timed by the host clock around a device synchronise and reported, with the peak of
``torch.cuda.max_memory_allocated`` above what was allocated when the call began.  The two results are compared bit for
bit.  The phases of the field path come from one more call in which ``_field_mark``, ``_field_rows`` and the layer loop
(``_score``) are each wrapped in a synchronise and a clock: mark, rows, layers, and "number" = the rest of the call (the
distinct ids, and per hop the compaction of the flags, the slots' scatter and the flags' clear; the degree prefix sum).
Also recorded: the field's ``sizes`` and edges, and the seconds and bytes of making the ``ReceptiveFields`` (once per
graph)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    """(result, seconds, peak bytes above the start) of fn(), the device idle before and after"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-products")
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--classes", type=int, default=172)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--rows-per-slab", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from salient_plusplus_amd import inference as inf
    from salient_plusplus_amd.models import SAGE
    from salient_plusplus_amd.synthetic import make_workload
    if not torch.cuda.is_available():
        raise SystemExit("field_inference_profile: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    t0 = time.time()
    wl = make_workload(a.workload, device=dev)
    torch.cuda.synchronize()
    x, rowptr, col = wl.x, wl.rowptr, wl.col
    N = wl.num_nodes
    res = {"workload": a.workload, "nodes": N, "entries": col.numel(), "scored": a.nodes, "model": f"SAGE {a.layers} x {a.hidden}",
           "classes": a.classes, "act_dtype": "bfloat16", "rows_per_slab": a.rows_per_slab, "build_s": round(time.time() - t0, 1)}
    g = torch.Generator(device=dev).manual_seed(7)
    ids = torch.randint(0, N, (a.nodes,), generator=g, device=dev)
    torch.manual_seed(0)
    model = SAGE(x.size(1), a.hidden, a.classes, a.layers).to(dev)
    kw = dict(rows_per_slab=a.rows_per_slab, act_dtype=torch.bfloat16)

    fields, s, nbytes = _timed(lambda: inf.ReceptiveFields(rowptr, col))
    res["receptive_fields"] = {"make_s": round(s, 4), "bytes": nbytes}
    field, s, _ = _timed(lambda: fields.field(ids, a.layers - 1))
    res["field"] = {"sizes": field.sizes, "edges": field.col.numel(), "share_of_graph": round(field.sizes[-1] / N, 5),
                    "first_build_s": round(s, 4)}
    del field
    print(json.dumps(res), flush=True)

    def baseline():
        return inf.layerwise_inference(model, x, rowptr, col, nodes=ids, **kw)

    def over_field():
        return inf.field_inference(model, x, rowptr, col, ids, fields=fields, **kw)

    want, s_b, _ = _timed(baseline)                           # warm-up, and the comparison
    got, s_f, _ = _timed(over_field)
    res["warm_up"] = {"layerwise_s": round(s_b, 4), "field_s": round(s_f, 4)}
    res["bit_identical"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    del want, got
    res["passes"] = []
    for k in range(a.repeats):
        _o, s_b, m_b = _timed(baseline)
        del _o
        _o, s_f, m_f = _timed(over_field)
        del _o
        res["passes"].append({"pass": k, "layerwise_s": round(s_b, 5), "layerwise_peak_bytes": m_b,
                              "field_s": round(s_f, 5), "field_peak_bytes": m_f})
        print(json.dumps(res["passes"][-1]), flush=True)
    med = lambda key: sorted(p[key] for p in res["passes"])[len(res["passes"]) // 2]     # noqa: E731
    res["median"] = {"layerwise_s": med("layerwise_s"), "field_s": med("field_s"),
                     "layerwise_over_field": round(med("layerwise_s") / med("field_s"), 2),
                     "rows_ratio_N_over_field": round(N / max(res["field"]["sizes"][-1], 1), 2)}

    # the phases, in a call of their own: every wrapped step starts and ends with an idle device
    phase = {"mark_s": 0.0, "rows_s": 0.0, "layers_s": 0.0}
    inner = {"mark_s": ("_field_mark", inf._field_mark), "rows_s": ("_field_rows", inf._field_rows),
             "layers_s": ("_score", inf._score)}

    def wrap(key, fn):
        def run(*args, **kwargs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*args, **kwargs)
            torch.cuda.synchronize()
            phase[key] += time.perf_counter() - t
            return out
        return run
    for key, (name, fn) in inner.items():
        setattr(inf, name, wrap(key, fn))
    try:
        _o, s, _ = _timed(over_field)
    finally:
        for _key, (name, fn) in inner.items():
            setattr(inf, name, fn)
    phase["number_s"] = s - sum(phase.values())
    res["phases"] = {k: round(v, 5) for k, v in phase.items()}
    res["phases"]["call_s"] = round(s, 5)
    print(json.dumps({k: res[k] for k in ("bit_identical", "median", "phases")}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
