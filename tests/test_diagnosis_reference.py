"""The FitError diagnosis boundary without a device: the reference reduction (tests/diagnosis_reference.py) on a
hand-computed case, and the ABI -- the header declares ksg_schedule_one_diag / ksg_schedule_batch_diag with the
ksg_diagnosis layout ksg/abi.py mirrors, and libksg.so exports both."""
import ctypes as C
import os
import re

from diagnosis_reference import (NUM_REASONS, empty, fill, fit_error_text, hand_case, hand_expected, reduce_eval,
                                 reference_stream)
from ksg import abi
from oracle_binding import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ksg.h")).read()


def test_hand_computed_case():
    """Four nodes, four different rejections, every number written down by hand (diagnosis_reference.hand_case)."""
    nodes, existing, pod = hand_case()
    o = fill(oracle({}), nodes, existing)
    (res, d), = reference_stream(o, [pod])
    want_res, want_d, want_text = hand_expected()
    assert res == want_res
    assert d == want_d
    assert fit_error_text(d) == want_text
    # the reason bins count statuses, not nodes: `short` is in two of them
    assert sum(d["reason_nodes"]) == 5 and d["failed_nodes"] == 4
    # the same cycle, node by node, as the oracle reports it
    _, ev = o.schedule_one(o.compile(pod), assume=False, evaluate=True)
    ix = {n: i for i, n in enumerate(o.node_names())}
    assert [ev["node_code"][ix[n]] for n in ("tainted", "short", "elsewhere", "full")] == [3, 2, 3, 2]


def test_a_schedulable_cycle_has_an_all_zero_diagnosis():
    nodes, existing, pod = hand_case()
    pod["spec"]["containers"][0]["resources"]["requests"] = {"cpu": "500m", "memory": "500Mi"}  # `short` takes it
    o = fill(oracle({}), nodes, existing)
    (res, d), = reference_stream(o, [pod])
    assert res[0] == abi.SUCCESS and res[3] == 1
    assert d == empty(4)


def test_plugin_none_nodes_count_without_a_plugin_bit():
    """A node outside a PreFilterResult (matchFields) has code 3, plugin 255 and the PreFilter reason: it is a failed,
    unresolvable node in the PreFilter bin, and sets no plugin bit."""
    ev = {"prefilter_code": 0, "prefilter_plugin": 255, "node_code": [3, 2, 0], "node_plugin": [255, 5, 255],
          "node_reasons": [1 << 16, 1 << 7, 0]}
    d = reduce_eval(abi.UNSCHEDULABLE, ev, 3)
    assert (d["failed_nodes"], d["unresolvable_nodes"], d["unschedulable_plugins"]) == (2, 1, 1 << 5)
    assert d["reason_nodes"][16] == 1 and d["reason_nodes"][7] == 1 and sum(d["plugin_nodes"]) == 1


def test_header_declares_and_library_exports_the_diagnosed_calls():
    from test_abi_cpu import _ensure_built, declared_symbols
    syms = declared_symbols()
    assert "ksg_schedule_one_diag" in syms and "ksg_schedule_batch_diag" in syms
    assert re.search(r"#define\s+KSG_ABI_VERSION\s+3\b", HEADER)
    assert re.search(r"#define\s+KSG_NUM_REASONS\s+17\b", HEADER) and NUM_REASONS == 17
    lib = C.CDLL(_ensure_built())
    assert hasattr(lib, "ksg_schedule_one_diag") and hasattr(lib, "ksg_schedule_batch_diag")


def test_python_structure_follows_the_header():
    """ksg/abi.py's Diagnosis has the header's fields in the header's order (all 32-bit: no padding to disagree on)."""
    body = re.search(r"typedef struct ksg_diagnosis \{(.*?)\} ksg_diagnosis;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", f).strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in abi.Diagnosis._fields_]
    assert C.sizeof(abi.Diagnosis) == 4 * (6 + abi.NUM_PLUGINS + NUM_REASONS)
