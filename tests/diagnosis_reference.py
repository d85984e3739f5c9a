"""The FitError diagnosis (include/ksg.h ksg_diagnosis) as a test reference, from the oracle alone.

By definition a pod's diagnosis is the reduction of the evaluation output of its own cycle -- node_code, node_plugin
and node_reasons over the nodes with a non-zero code -- so the reference drives the oracle pod by pod
(schedule_one(h, assume=True, evaluate=True): pod i sees the assumes of pods 0..i-1 and none later) and reduces each
cycle's eval dict here, in Python.  Nothing of the code under test is involved.

Only tests/ use this module.
"""
from ksg.abi import NUM_PLUGINS, PLUGIN_ID, PLUGIN_NONE, REASONS, UNSCHEDULABLE, UNSCHEDULABLE_AND_UNRESOLVABLE
from ksg.objects import NodeW, PodW

NUM_REASONS = len(REASONS)  # KSG_R_* bits 0..16
FIT_ERROR = (UNSCHEDULABLE, UNSCHEDULABLE_AND_UNRESOLVABLE)


def empty(num_nodes, prefilter_code=0, prefilter_plugin=PLUGIN_NONE):
    return {"num_nodes": num_nodes, "failed_nodes": 0, "unresolvable_nodes": 0, "unschedulable_plugins": 0,
            "prefilter_code": prefilter_code, "prefilter_plugin": prefilter_plugin,
            "plugin_nodes": [0] * NUM_PLUGINS, "reason_nodes": [0] * NUM_REASONS}


def reduce_eval(status, ev, num_nodes):
    """ksg_diagnosis (as Diagnosis.as_dict()) of a cycle that ended with `status` and evaluation output `ev`."""
    d = empty(num_nodes, ev["prefilter_code"], ev["prefilter_plugin"])
    if status not in FIT_ERROR:
        return d
    for i in range(num_nodes):
        code, plugin, reasons = ev["node_code"][i], ev["node_plugin"][i], ev["node_reasons"][i]
        if code == 0:
            continue
        d["failed_nodes"] += 1
        d["unresolvable_nodes"] += code == UNSCHEDULABLE_AND_UNRESOLVABLE
        if plugin != PLUGIN_NONE:  # (255: outside a PreFilterResult, or a PreFilter rejection -- no plugin bit)
            d["plugin_nodes"][plugin] += 1
            d["unschedulable_plugins"] |= 1 << plugin
        for r in range(NUM_REASONS):
            d["reason_nodes"][r] += reasons >> r & 1
    return d


def fill(backend, nodes, existing=(), namespaces=(), objects=()):
    for ns in namespaces:
        backend.upsert_namespace(ns)
    for o in objects:
        backend.upsert_object(o)
    for n in nodes:
        backend.add_node(n)
    for p in existing:
        backend.add_pod(p)
    return backend


def reference_stream(o, pods, assume=True):
    """The oracle context `o` driven pod by pod -> [(result tuple, diagnosis dict)] (and o has assumed the pods)."""
    out = []
    n = o.num_nodes()
    for p in pods:
        r, ev = o.schedule_one(o.compile(p), assume=assume, evaluate=True)
        out.append((r.as_tuple(), reduce_eval(r.status, ev, n)))
    return out


def fit_error_text(d):
    """FitError.Error() (framework/types.go:1146-1180) from a diagnosis dict: "<count> <reason>" strings, sorted."""
    parts = sorted(f"{d['reason_nodes'][r]} {REASONS[r]}" for r in range(NUM_REASONS) if d["reason_nodes"][r])
    return f"0/{d['num_nodes']} nodes are available: " + ", ".join(parts) + "."


# ---- the hand-computed four-node case -------------------------------------------------------------------------
def hand_case():
    """-> (nodes, existing pods, the pod).  The pod asks for 2 cpu / 2Gi on a disk=ssd node and tolerates nothing:
      tainted   disk=ssd, roomy, taint dedicated=x:NoSchedule  -> TaintToleration, UnschedulableAndUnresolvable
      short     disk=ssd, 4 cpu / 8Gi with 3 cpu / 7Gi bound   -> NodeResourcesFit, Unschedulable: cpu AND memory
      elsewhere disk=hdd, roomy                                -> NodeAffinity (the nodeSelector), Unresolvable
      full      disk=ssd, roomy, pods: 1 with one pod bound    -> NodeResourcesFit, Unschedulable: Too many pods"""
    big = {"cpu": "16", "memory": "64Gi", "pods": "110"}
    nodes = [
        NodeW("tainted").capacity(big).label("disk", "ssd")
        .taints([{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]).obj(),
        NodeW("short").capacity({"cpu": "4", "memory": "8Gi", "pods": "110"}).label("disk", "ssd").obj(),
        NodeW("elsewhere").capacity(big).label("disk", "hdd").obj(),
        NodeW("full").capacity(dict(big, pods="1")).label("disk", "ssd").obj(),
    ]
    existing = [
        PodW("hog").container(image="i", requests={"cpu": "3", "memory": "7Gi"}).node("short").obj(),
        PodW("sitter").container(image="i", requests={"cpu": "100m", "memory": "100Mi"}).node("full").obj(),
    ]
    pod = PodW("picky").container(image="i", requests={"cpu": "2", "memory": "2Gi"}).node_selector({"disk": "ssd"}).obj()
    return nodes, existing, pod


TAINT, NA, FIT = PLUGIN_ID["TaintToleration"], PLUGIN_ID["NodeAffinity"], PLUGIN_ID["NodeResourcesFit"]
R_TAINT, R_NA_POD, R_TOO_MANY, R_CPU, R_MEM = 2, 3, 6, 7, 8  # KSG_R_* bit numbers (ksg.h)


def hand_expected():
    """Worked out by hand from hand_case(): (ksg_result tuple, diagnosis dict, FitError text)."""
    d = empty(4)
    d["failed_nodes"] = 4
    d["unresolvable_nodes"] = 2  # tainted, elsewhere
    d["unschedulable_plugins"] = 1 << TAINT | 1 << NA | 1 << FIT
    d["plugin_nodes"][TAINT] = 1
    d["plugin_nodes"][NA] = 1
    d["plugin_nodes"][FIT] = 2  # short, full
    for r in (R_TAINT, R_NA_POD, R_TOO_MANY, R_CPU, R_MEM):
        d["reason_nodes"][r] = 1  # `short` is in both the cpu and the memory bin
    text = ("0/4 nodes are available: 1 Insufficient cpu, 1 Insufficient memory, 1 Too many pods, "
            "1 node(s) didn't match Pod's node affinity/selector, 1 node(s) had untolerated taint(s).")
    return (UNSCHEDULABLE, -1, 4, 0, 0), d, text
