"""Host-only: the C header and the ctypes table agree on nt_semi_implicit_rollout (ten parameters, the argument order of the
other fused rollouts)."""
import ctypes as C
import os
import re

from newton_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "newton_hip.h")


def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"nt_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/newton_hip.h"
    return [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).split(",")]


def test_header_and_ctypes_table_declare_the_rollout_with_ten_parameters():
    args = _declaration("nt_semi_implicit_rollout")
    assert len(args) == 10
    restype, argtypes = _lib.SYMBOLS["nt_semi_implicit_rollout"]
    assert restype is C.c_int32 and len(argtypes) == 10
    # same order and conventions as nt_featherstone_rollout / nt_xpbd_rollout, with this solver's parameter struct
    fs = _declaration("nt_featherstone_rollout")
    assert [a.replace("nt_featherstone_params", "nt_semi_implicit_params") for a in fs] == args
    assert argtypes[0] == C.POINTER(_lib.nt_model) and argtypes[1] == C.POINTER(_lib.nt_semi_implicit_params)
    assert argtypes[2:] == _lib.SYMBOLS["nt_featherstone_rollout"][1][2:] == _lib.SYMBOLS["nt_xpbd_rollout"][1][2:]
    assert re.search(r"^ \*\s+nt_semi_implicit_rollout\s+<-", open(HEADER).read(), re.M)  # the entry-point table at the top
