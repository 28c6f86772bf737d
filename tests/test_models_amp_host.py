"""CPU-only: the C ABI of bf16 mixed precision -- the element codes, the aggregation descriptors and their two entries
(include/spp.h) -- is declared, bound by ctypes with the header's layout, and exported; the models' autocast test."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENTRIES = ["spp_agg_forward", "spp_agg_backward"]
DESCS = {"spp_agg_fwd_desc": "AggFwdDesc", "spp_agg_bwd_desc": "AggBwdDesc"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spp.h")).read(), flags=re.S)


def test_header_declares_the_codes_descriptors_and_entries():
    from salient_plusplus_amd import _native as nat
    src = _header()
    codes = {"SPP_ELEM_F32": 0, "SPP_ELEM_F16": 1, "SPP_ELEM_BF16": 2, "SPP_AGG_DENSE": 0, "SPP_AGG_TABLE": 1,
             "SPP_AGG_ROWS": 2, "SPP_AGG_MEAN": 0, "SPP_AGG_OPERAND": 1, "SPP_AGG_OPERAND_ACT": 2, "SPP_AGG_SUM": 3,
             "SPP_AGG_SCATTER": 0, "SPP_AGG_GATHER": 1}
    for name, value in codes.items():
        assert re.search(r"\b" + name + r"\s*=\s*" + str(value) + r"\b", src), name
        assert getattr(nat, name) == value, name
    for c_name in DESCS:
        assert re.search(r"typedef struct " + c_name + r"\s*\{.*?\}\s*" + c_name + ";", src, re.S), c_name
    assert re.search(r"\bspp_agg_forward\s*\(\s*const spp_agg_fwd_desc\s*\*", src)
    assert re.search(r"\bspp_agg_backward\s*\(\s*const spp_agg_bwd_desc\s*\*", src)
    for name in ENTRIES:
        assert name in nat.SIGNATURES, name
    assert nat.SIGNATURES["spp_agg_forward"][1][0]._type_ is nat.AggFwdDesc
    assert nat.SIGNATURES["spp_agg_backward"][1][0]._type_ is nat.AggBwdDesc


def test_descriptor_layouts_match_a_gcc_compile_of_the_header():
    """sizeof and every field's offset, as in test_struct_layouts_match_header"""
    from salient_plusplus_amd import _native as nat
    lines = []
    for c_name, py_name in DESCS.items():
        lines.append(f'printf("{c_name} size %zu\\n", sizeof({c_name}));')
        for field, _t in getattr(nat, py_name)._fields_:
            lines.append(f'printf("{c_name} {field} %zu\\n", offsetof({c_name}, {field}));')
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"spp.h\"\nint main(void) {\n" + "\n".join(lines) + \
        "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([exe]).decode().splitlines()}
    for c_name, py_name in DESCS.items():
        S = getattr(nat, py_name)
        assert got[(c_name, "size")] == ctypes.sizeof(S), c_name
        for field, _t in S._fields_:
            assert got[(c_name, field)] == getattr(S, field).offset, (c_name, field)


def test_entries_are_exported_when_the_library_exists():
    from salient_plusplus_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        return
    L = nat.load()
    for name in ENTRIES:
        assert hasattr(L, name), f"{name} not exported"


def test_the_bf16_decision_follows_the_autocast_state():
    """models.amp_bf16: bf16 CUDA autocast only (querying the CUDA autocast state needs no device)"""
    from salient_plusplus_amd import models
    assert not models.amp_bf16()
    assert models._ELEM == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
