"""CPU-only: the refusals that the four graph-kernel entries share -- spp_graph_agg_forward, spp_graph_agg_parts_forward,
spp_graph_gat_forward and spp_graph_gat_parts_forward validate the element codes, the targets, the sizes, the strides,
the workspace, the buffers and the vector form's output rule the same way.  Every class is put to every entry: status
-1, a message that starts with the entry's own name and carries the class's word.  ctypes descriptors and fake non-NULL
pointers; a refusal dereferences nothing and enqueues nothing, and an empty call returns 0 before any device call."""
import ctypes

import pytest

_FAKE = 0x10000                                               # 16-byte aligned, never dereferenced
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)
ENTRIES = ["spp_graph_agg_forward", "spp_graph_agg_parts_forward", "spp_graph_gat_forward", "spp_graph_gat_parts_forward"]
PARTS_ENTRIES = [e for e in ENTRIES if "parts" in e]


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def _desc(nat, entry, offsets=(0, 4, 10), bases=(_FAKE, 2 * _FAKE), **over):
    """a descriptor of ``entry`` that passes every check: ten rows of F = 8 fp32 columns (two heads of four: the vector
    form), the slab of the first four targets; with parts, the rows [0, 4) and [4, 10).  ``over`` alters it."""
    kw = dict(x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, rowptr_dev=_FAKE, col_dev=_FAKE, x_stride_elems=8, F=8,
              target_row0=0, target_ids_dev=None, num_targets=4, out_dev=_FAKE, out_stride_elems=0)
    gat, parts = "gat" in entry, "parts" in entry
    kw.update(dict(heads=2, relu=0, negative_slope=0.2) if gat else dict(epilogue=nat.SPP_AGG_MEAN))
    if parts:
        kw.update(num_parts=len(offsets) - 1)
    else:
        kw.update(dict(x_dev=_FAKE, x_rows=10), **(dict(a_src_dev=_FAKE, a_dst_dev=_FAKE) if gat else {}))
    kw.update(over)
    cls = {"spp_graph_agg_forward": nat.GraphAggDesc, "spp_graph_agg_parts_forward": nat.GraphAggPartsDesc,
           "spp_graph_gat_forward": nat.GraphGatDesc, "spp_graph_gat_parts_forward": nat.GraphGatPartsDesc}[entry]
    d = cls(**kw)
    if parts:
        for i, v in enumerate(offsets):
            d.part_offsets[i] = v
        for i, v in enumerate(bases):
            if gat:
                d.h_parts_dev[i], d.a_parts_dev[i] = v or None, v or None
            else:
                d.x_parts_dev[i] = v or None
    return d


def _call(nat, L, entry, over, ws=_FAKE, nbytes=None):
    d = _desc(nat, entry, **over)
    if nbytes is None:
        nbytes = 16 + 8 * max(int(d.num_targets), 0)          # spp_graph_*_workspace_bytes(num_targets)
    return getattr(L, entry)(ctypes.byref(d), ctypes.c_void_p(ws), nbytes, None)


# (class, descriptor changes, workspace changes, the word of the class)
SHARED_REFUSALS = [
    ("unknown x element code", dict(x_elem=9), {}, b"element code"),
    ("fp16 output", dict(out_elem=1), {}, b"element code"),
    ("fp8 rows", dict(x_elem=3), {}, b"fp8"),
    ("slab and list both", dict(target_ids_dev=_FAKE), {}, b"not both"),
    ("slab and list neither", dict(target_row0=-1), {}, b"one of them"),
    ("negative num_targets", dict(num_targets=-1), {}, b"negative size"),
    ("negative F", dict(F=-4), {}, b"negative size"),
    ("slab leaves the graph", dict(target_row0=8, num_targets=4), {}, b"leaves the graph's 10 rows"),
    ("out stride too small", dict(out_stride_elems=4), {}, b"smaller than the output row"),
    ("x stride too small", dict(x_stride_elems=4), {}, b"smaller than the row"),
    ("missing workspace", {}, dict(ws=None, nbytes=0), b"workspace"),
    ("short workspace", {}, dict(nbytes=16), b"workspace"),
    ("misaligned workspace", {}, dict(ws=_FAKE + 8), b"workspace"),
    ("NULL rowptr", dict(rowptr_dev=None), {}, b"NULL buffer"),
    ("NULL col", dict(col_dev=None), {}, b"NULL buffer"),
    ("NULL out", dict(out_dev=None), {}, b"NULL buffer"),
    ("misaligned out base (vector form)", dict(out_dev=_FAKE + 4), {}, b"aligned to 4 elements"),
    ("misaligned out stride (vector form)", dict(out_stride_elems=10), {}, b"aligned to 4 elements"),
]
WHOLE_REFUSALS = [                                            # the entries that take one matrix
    ("negative x_rows", dict(x_rows=-1), {}, b"negative size"),
    ("NULL x", dict(x_dev=None), {}, b"NULL buffer"),
]
PARTS_REFUSALS = [                                            # the entries that take row ranges
    ("no parts", dict(num_parts=0), {}, b"num_parts 0"),
    ("too many parts", dict(num_parts=17), {}, b"num_parts 17"),
    ("offsets do not start at 0", dict(offsets=(1, 4, 10)), {}, b"part_offsets[0]"),
    ("offsets decrease", dict(offsets=(0, 5, 4)), {}, b"part_offsets decrease"),
    ("NULL base of a non-empty part", dict(bases=(_FAKE, 0)), {}, b"NULL"),
]
CASES = ([(e, *r) for e in ENTRIES for r in SHARED_REFUSALS]
         + [(e, *r) for e in ENTRIES if e not in PARTS_ENTRIES for r in WHOLE_REFUSALS]
         + [(e, *r) for e in PARTS_ENTRIES for r in PARTS_REFUSALS])


@pytest.mark.parametrize("entry,what,over,call,word", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_every_entry_refuses_every_shared_class_by_its_own_name(entry, what, over, call, word):
    nat, L = _lib()
    assert _call(nat, L, entry, over, **call) == SPP_ERR_INVALID, what
    msg = L.spp_last_error()
    assert msg.startswith(entry.encode() + b":") and word in msg, (what, msg)
    if what == "NULL base of a non-empty part":
        assert b"part 1" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_calls_return_ok_before_any_buffer_is_looked_at(entry):
    nat, L = _lib()
    for over in (dict(num_targets=0), dict(F=0), dict(num_targets=0, F=0),
                 dict(num_targets=0, rowptr_dev=None, col_dev=None, out_dev=None)):
        assert _call(nat, L, entry, over) == SPP_OK, (over, L.spp_last_error())
    if entry in PARTS_ENTRIES:                                # an empty part owns no row: its bases may be NULL
        assert _call(nat, L, entry, dict(num_targets=0, offsets=(0, 0, 10, 10), bases=(0, _FAKE, 0))) == SPP_OK
