"""CPU-only: the host side of aggregation and layer-wise inference over a row-partitioned table -- the ctypes layout of
spp_graph_agg_parts_desc against the header, every refusal of spp_graph_agg_parts_forward by message (the entry validates
before it touches a device), the Python checks of inference.graph_aggregate_parts and
inference.partitioned_layerwise_inference, the resident_partition accessor's refusals, and LocalPeers' failure rule."""
import ctypes
import os
import subprocess
import tempfile
import threading
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_agg_parts_desc_layout_matches_header():
    """sizeof, SPP_GRAPH_AGG_MAX_PARTS and every field offset, cross-checked by compiling the header with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.GraphAggPartsDesc._fields_]
    offs = ", ".join(f"offsetof(spp_graph_agg_parts_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { SPP_GRAPH_AGG_MAX_PARTS, sizeof(spp_graph_agg_parts_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [nat.SPP_GRAPH_AGG_MAX_PARTS, ctypes.sizeof(nat.GraphAggPartsDesc)] \
        + [getattr(nat.GraphAggPartsDesc, n).offset for n in names]
    assert nat.SPP_GRAPH_AGG_MAX_PARTS == 16


def _desc(nat, offsets=(0, 2, 4), bases=(0x1000, 0x2000), **kw):
    """a descriptor every check accepts (nothing is launched: the workspace is missing), then altered by ``kw``"""
    d = nat.GraphAggPartsDesc(epilogue=nat.SPP_AGG_MEAN, x_elem=nat.SPP_ELEM_F16, out_elem=nat.SPP_ELEM_F32,
                              num_parts=len(offsets) - 1, rowptr_dev=0x100, col_dev=0x200, x_stride_elems=8, F=8,
                              target_row0=0, num_targets=4, out_dev=0x3000)
    for i, v in enumerate(offsets):
        d.part_offsets[i] = v
    for i, v in enumerate(bases):
        d.x_parts_dev[i] = v or None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_refuses_by_message_before_any_device_call():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    L = nat.load()
    assert "spp_graph_agg_parts_forward" in nat.SIGNATURES and L.spp_abi_version() == 6
    ws = (ctypes.c_ubyte * 256)()
    wsp = ctypes.c_void_p((ctypes.addressof(ws) + 15) // 16 * 16)

    def refused(d, *needles, workspace=wsp, nbytes=128):
        assert L.spp_graph_agg_parts_forward(ctypes.byref(d) if d is not None else None, workspace, nbytes, None) == -1
        msg = L.spp_last_error().decode()
        assert msg.startswith("spp_graph_agg_parts_forward"), msg
        for n in needles:
            assert n in msg, (n, msg)

    refused(None, "NULL descriptor")
    refused(_desc(nat, num_parts=0), "num_parts 0")
    refused(_desc(nat, num_parts=17), "num_parts 17")
    refused(_desc(nat, offsets=(1, 2, 4)), "part_offsets[0]")
    refused(_desc(nat, offsets=(0, 3, 2)), "part_offsets decrease")
    refused(_desc(nat, bases=(0x1000, 0)), "part 1", "NULL")
    refused(_desc(nat, x_elem=nat.SPP_ELEM_FP8_E4M3), "fp8")
    # ... and everything spp_graph_agg_forward refuses
    refused(_desc(nat, epilogue=nat.SPP_AGG_OPERAND_ACT), "epilogue")
    refused(_desc(nat, x_elem=9), "element code")
    refused(_desc(nat, out_elem=nat.SPP_ELEM_F16), "element code")
    refused(_desc(nat, target_ids_dev=0x400), "not both")
    refused(_desc(nat, target_row0=-1), "one of them")
    refused(_desc(nat, num_targets=-1), "negative size")
    refused(_desc(nat, target_row0=3, num_targets=2), "leaves the graph's 4 rows")
    refused(_desc(nat, out_stride_elems=4), "output stride")
    refused(_desc(nat), "workspace", workspace=None, nbytes=0)
    refused(_desc(nat), "workspace", nbytes=16)
    refused(_desc(nat, rowptr_dev=None), "NULL buffer")
    refused(_desc(nat, x_stride_elems=4), "row stride")
    refused(_desc(nat, out_dev=0x3004), "aligned to 4 elements")          # the vector form's output rule
    # an empty part may have a NULL base, and a call without targets is complete before any launch
    ok = _desc(nat, offsets=(0, 0, 4, 4), bases=(0, 0x1000, 0), num_targets=0)
    assert L.spp_graph_agg_parts_forward(ctypes.byref(ok), wsp, 128, None) == 0


def _tiny(P=2):
    x = torch.zeros((4, 8), dtype=torch.float16)
    return [x[:2], x[2:]], [0, 2, 4], torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, 1, 2, 3])


def test_graph_aggregate_parts_validates_its_arguments():
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.fast_sampler import P2PPeers
    from salient_plusplus_amd.inference import graph_aggregate_parts as gap
    parts, off, rowptr, col = _tiny()
    slab = dict(row0=0, num_targets=4)
    with pytest.raises(ValueError, match="part_offsets must hold"):
        gap(parts, [0], rowptr, col, **slab)
    with pytest.raises(ValueError, match="part_offsets must hold"):
        gap(parts, list(range(18)), rowptr, col, **slab)
    with pytest.raises(ValueError, match="start at 0 and never decrease"):
        gap(parts, [0, 3, 2], rowptr, col, **slab)
    with pytest.raises(ValueError, match="start at 0"):
        gap(parts, [1, 2, 4], rowptr, col, **slab)
    with pytest.raises(ValueError, match="3 parts for 2 ranges"):
        gap(parts + [None], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="part 1 has 2 rows"):
        gap(parts, [0, 2, 5], rowptr, col, **slab)
    with pytest.raises(ValueError, match="is None"):
        gap([parts[0], None], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one dtype and one row width"):               # mixed dtypes
        gap([parts[0], parts[1].float()], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one dtype and one row width"):               # mixed widths
        gap([parts[0], parts[1][:, :4]], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="one row stride"):                            # mixed strides
        gap([parts[0], torch.zeros((2, 16), dtype=torch.float16)[:, :8]], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="different devices"):
        gap([parts[0], torch.zeros((2, 8), dtype=torch.float16, device="meta")], off, rowptr, col, **slab)
    with pytest.raises(TypeError, match="fp8"):
        gap([parts[0], fp8.quantize_e4m3(torch.zeros((2, 16)))], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="2-D"):
        gap([parts[0], parts[1].double()], off, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="requires grad"):
        gap([parts[0], parts[1].clone().requires_grad_()], off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="every part is empty"):
        gap([None, parts[0][:0]], [0, 0, 0], rowptr[:1], col, row0=0, num_targets=0)
    with pytest.raises(ValueError, match="one row per node"):
        gap(parts, off, rowptr[:-1], col, **slab)
    with pytest.raises(ValueError, match="int64"):
        gap(parts, off, rowptr.int(), col, **slab)
    with pytest.raises(ValueError, match="not both"):
        gap(parts, off, rowptr, col, target_ids=torch.tensor([0]), **slab)
    with pytest.raises(ValueError, match="either as a slab"):
        gap(parts, off, rowptr, col)
    with pytest.raises(ValueError, match="both row0 and num_targets"):
        gap(parts, off, rowptr, col, row0=0)
    with pytest.raises(ValueError, match="leaves the graph"):
        gap(parts, off, rowptr, col, row0=3, num_targets=2)
    with pytest.raises(ValueError, match="target_ids"):
        gap(parts, off, rowptr, col, target_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="epilogue"):
        gap(parts, off, rowptr, col, epilogue="operand_act", **slab)
    with pytest.raises(ValueError, match="out_dtype"):
        gap(parts, off, rowptr, col, out_dtype=torch.float16, **slab)
    with pytest.raises(ValueError, match="out must be"):
        gap(parts, off, rowptr, col, out=torch.zeros((4, 9)), **slab)
    # the P2PPeers form: addresses only, so the element type and the width come from the caller
    peers = P2PPeers([0x1000, 0x2000], 16)
    with pytest.raises(ValueError, match="needs dtype="):
        gap(peers, off, rowptr, col, **slab)
    with pytest.raises(ValueError, match="peer tables for 3 parts"):
        gap(peers, [0, 2, 4, 4], rowptr, col, dtype=torch.float16, F=8, **slab)
    with pytest.raises(ValueError, match="has no address"):
        gap(P2PPeers([0x1000, 0], 16), off, rowptr, col, dtype=torch.float16, F=8, **slab)
    with pytest.raises(ValueError, match="no multiple of the element size"):
        gap(P2PPeers([0x1000, 0x2000], 18), off, rowptr, col, dtype=torch.float32, F=4, **slab)
    with pytest.raises(ValueError, match="describe a P2PPeers source"):
        gap(parts, off, rowptr, col, dtype=torch.float16, **slab)
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        from salient_plusplus_amd import _native as nat
        with pytest.raises(nat.SppError):
            gap(parts, off, rowptr, col, **slab)


class _NoPeers:
    def share(self, t):
        raise AssertionError("refused calls publish nothing")

    barrier = close = share


def test_partitioned_inference_validates_and_models_refuse_with_a_reason():
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import partitioned_layerwise_inference as pli
    from salient_plusplus_amd.models import GAT, GIN, SAGE, SAGEResInception
    parts, off, rowptr, col = _tiny()
    x = parts[1]
    kw = dict(part_offsets=off, rank=1, peers=_NoPeers())
    sage = SAGE(8, 4, 2, 2)
    for admitted in (GAT(8, 4, 2, 2), SAGEResInception(8, 4, 2, 2)):     # past the model filter: the next check answers
        with pytest.raises(TypeError, match="^partitioned_layerwise_inference: an fp8 feature table"):
            pli(admitted, fp8.quantize_e4m3(torch.zeros((2, 16))), rowptr, col, **kw)
        with pytest.raises(ValueError, match="^partitioned_layerwise_inference: rank 2 outside"):
            pli(admitted, x, rowptr, col, **{**kw, "rank": 2})
    with pytest.raises(NotImplementedError, match="^partitioned_layerwise_inference: implemented for SAGE, GIN, GAT and "
                                                  "SAGEResInception, not Linear$"):
        pli(torch.nn.Linear(8, 2), x, rowptr, col, **kw)
    with pytest.raises(TypeError, match="fp8 feature table"):
        pli(sage, fp8.quantize_e4m3(torch.zeros((2, 16))), rowptr, col, **kw)
    with pytest.raises(ValueError, match="rank 2 outside"):
        pli(sage, x, rowptr, col, **{**kw, "rank": 2})
    with pytest.raises(ValueError, match="x_local has 2 rows"):
        pli(sage, x, rowptr, col, **{**kw, "part_offsets": [0, 1, 4]})
    with pytest.raises(ValueError, match="one row per node"):
        pli(sage, x, rowptr[:-1], col, **kw)
    with pytest.raises(ValueError, match="act_dtype"):
        pli(sage, x, rowptr, col, act_dtype=torch.float16, **kw)
    with pytest.raises(ValueError, match="rows_per_slab"):
        pli(GIN(8, 4, 2, 2), x, rowptr, col, rows_per_slab=0, **kw)
    with pytest.raises(ValueError, match="nodes must be"):
        pli(sage, x, rowptr, col, nodes=torch.tensor([0.5]), **kw)
    for bad in ([1], [4], [2, 3, 0]):                        # global ids of another rank's range, or outside the graph
        with pytest.raises(ValueError, match=r"outside rank 1's range \[2, 4\)"):
            pli(sage, x, rowptr, col, nodes=torch.tensor(bad), **kw)
    with pytest.raises(TypeError, match="peers must provide"):
        pli(sage, x, rowptr, col, **{**kw, "peers": object()})
    assert sage.training                                      # a refused call leaves the mode alone
    if not torch.cuda.is_available():
        from salient_plusplus_amd import _native as nat
        with pytest.raises(nat.SppError):
            pli(sage, x, rowptr, col, nodes=torch.tensor([3, 2]), **kw)
        assert sage.training


def test_resident_partition_refuses_what_it_cannot_hand_out():
    from salient_plusplus_amd import fast_sampler as fs
    from salient_plusplus_amd import fp8
    cfg = fs.Config()
    cfg.rowptr, cfg.col = torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    cfg.x_cpu = torch.zeros((1, 16))
    with pytest.raises(RuntimeError, match="not a distributed configuration"):
        fs.resident_partition(cfg)
    cfg.distributed = True
    cfg.partition_book = fs.RangePartitionBook(0, 2, torch.tensor([0, 1, 2]))
    cfg.x_gpu = fp8.quantize_e4m3(torch.zeros((1, 16)))
    with pytest.raises(RuntimeError, match="fp8"):
        fs.resident_partition(cfg)
    cfg.x_gpu = torch.empty(0)
    cfg.partition_book = fs.RangePartitionBook(2, 2, torch.tensor([0, 1, 2]))
    with pytest.raises(RuntimeError, match="rank 2 outside"):
        fs.resident_partition(cfg)
    cfg.partition_book = fs.RangePartitionBook(0, 2, torch.tensor([0, 1, 2]))
    cfg.x_cpu = None
    with pytest.raises(RuntimeError, match="no feature table"):
        fs.resident_partition(cfg)
    with pytest.raises(RuntimeError, match="distributed"):    # resident_graph keeps refusing such a configuration
        fs.resident_graph(cfg)


def test_local_peers_one_failing_rank_fails_the_others_within_the_timeout():
    """rank 1 raises where it would publish its tensor and aborts the barrier, as the driver does for a rank that fails:
    ranks 0 and 2 raise at once instead of waiting for it (the barrier's own timeout is far longer than the test)"""
    from salient_plusplus_amd.inference import LocalPeers
    peers = LocalPeers(3, timeout=30.0)
    seen, t0 = {}, time.monotonic()

    def rank(r):
        try:
            peers.bind(r)
            if r == 1:
                raise KeyError("rank 1 fails")
            peers.share(torch.zeros((2, 4)))
            seen[r] = "returned"
        except BaseException as e:  # noqa: BLE001
            peers.abort()
            seen[r] = e

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(20)
    assert not any(t.is_alive() for t in ts) and time.monotonic() - t0 < 10
    assert isinstance(seen[1], KeyError)
    for r in (0, 2):
        assert isinstance(seen[r], RuntimeError) and "another rank failed" in str(seen[r])
    with pytest.raises(RuntimeError, match="bind"):
        LocalPeers(2).share(torch.zeros((1, 4)))
    # and the working case: both ranks get both addresses and the common stride
    ok = LocalPeers(2, timeout=30.0)
    got = {}
    tabs = [torch.zeros((3, 4)), torch.zeros((0, 4))]

    def good(r):
        ok.bind(r)
        got[r] = ok.share(tabs[r])

    ts = [threading.Thread(target=good, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(20)
    assert got[0].ptrs == got[1].ptrs == [tabs[0].data_ptr(), 0] and got[0].stride == 16
