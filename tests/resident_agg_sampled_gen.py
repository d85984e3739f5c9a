"""Inputs for sampled pods on the per-pod API (ksg_schedule_one through the resident k_agg_loop's sampling instances,
config "residentAggSampled"; DESIGN.md §4.5 "Resident k_agg_loop"), beside tests/agg_sampled_gen.py's clusters and
streams, which the single calls reuse as they are: the oracle's batch semantics are sequential single cycles.

mixed_reference(): node-local pods between PodTopologySpread pods in one resident launch.  No pod of that cluster
carries an affinity term, so the node-local pods stay node-local; the stream opens with two of them, which the resident
k_sched_loop serves before the first pod-table pod starts k_agg_loop's launch, which then takes every later pod.

handover_reference(): single calls, a batch, single calls, an informer event, a forget, an idle gap and more calls than
one resident launch takes, with the oracle's result for each.

tests/test_resident_agg_sampled_inputs.py states on the oracle alone what the streams must exercise."""
import functools
import json

import agg_sampled_gen as gen
from ksg.objects import NodeW

MAX_LAUNCH_PODS = 1024  # desc.h kLoopMaxPods: a resident launch ends after this many pods


def template_of(pod):
    """The pod but for its name and uid: equal for pods stamped from one template."""
    p = json.loads(json.dumps(pod))
    p["metadata"].pop("name", None)
    p["metadata"].pop("uid", None)
    return json.dumps(p, sort_keys=True)


def plain(name):  # node-local: no PodTopologySpread constraint, no affinity term
    return gen.base(name, "plain", cpu="300m", ipa=False).obj()


def spread_only(name, k):
    """Pod-table pods without affinity terms: zone DoNotSchedule + hostname ScheduleAnyway, or (every third) the
    hostname spread honouring node affinity and taints."""
    if k % 3 == 2:
        return gen.base(name, "hs", ipa=False).spread(1, gen.HOST, "DoNotSchedule", gen.sel("hs"),
                                                      node_affinity_policy="Honor", node_taints_policy="Honor").obj()
    return (gen.base(name, "zs", ipa=False).spread(2, gen.ZONE, "DoNotSchedule", gen.sel("zs"))
            .spread(1, gen.HOST, "ScheduleAnyway", gen.sel("zs"))).obj()


MIXED_LEAD = 2  # node-local pods before the first pod-table pod


def mixed_stream(n_pods=62):
    """plain, plain, then groups of {zs, zs, hs, plain, plain}: a zs pod after a zs pod (the same template), a zs
    pod after a plain pod, a plain pod after an hs pod."""
    pods, k = [plain(f"lead{j}") for j in range(MIXED_LEAD)], 0
    for j in range(n_pods - MIXED_LEAD):
        if j % 5 >= 3:
            pods.append(plain(f"plain{j}"))
        else:
            pods.append(spread_only(f"class{k}", k))
            k += 1
    return pods


@functools.lru_cache(maxsize=None)
def mixed_reference(pct=30):
    """(context config, nodes, bound pods, pods, [Cycle]): 600 nodes, no bound pod."""
    nodes, _ = gen.shape_cluster("600")
    cfg = {"percentageOfNodesToScore": pct}
    pods = mixed_stream()
    want, o = gen.run_oracle(cfg, nodes, [], pods)
    o.close()
    return cfg, nodes, [], pods, want


def is_node_local(pod):
    return pod["metadata"]["labels"]["app"] == "plain"


# ---- the hand-over of nextStartNodeIndex ---------------------------------------------------------------------------
# (step, argument): "one" n single calls, "calls" n single calls issued back to back from native code, "batch" n pods
# in one schedule_batch, "add_node" an informer event, "forget" the pod placed last, "sleep" seconds without a call
HANDOVER = (("one", 40), ("batch", 30), ("one", 20), ("add_node", "extra-node"), ("one", 10), ("forget", None),
            ("one", 10), ("sleep", 0.1), ("one", 10), ("calls", MAX_LAUNCH_PODS + 16))
HANDOVER_SHAPE, HANDOVER_PCT = "257", 30


def extra_node(name):
    return (NodeW(name).label(gen.HOST, name).label(gen.ZONE, "z1")
            .capacity({"cpu": "64", "memory": "256Gi", "pods": "500"}).obj())


@functools.lru_cache(maxsize=None)
def handover_reference():
    """(context config, nodes, bound pods, [(step, argument, pods, [result tuple])]) through one oracle context."""
    nodes, bound = gen.shape_cluster(HANDOVER_SHAPE)
    cfg = dict(gen.SHAPES[HANDOVER_SHAPE][3], percentageOfNodesToScore=HANDOVER_PCT)
    total = sum(a for s, a in HANDOVER if s in ("one", "calls", "batch"))
    stream = gen.stream("three", True, total)
    o = gen.fill(gen.oracle(gen.oracle_cfg(cfg)), nodes, bound)
    steps, at, last = [], 0, None
    for step, arg in HANDOVER:
        pods, res = [], []
        if step in ("one", "calls", "batch"):
            pods = stream[at:at + arg]
            at += arg
            for p in pods:
                h = o.compile(p)
                r = o.schedule_one(h, assume=True)[0].as_tuple()
                res.append(r)
                if r[0] == 0 and r[1] >= 0:
                    last = h
        elif step == "add_node":
            o.add_node(extra_node(arg))
        elif step == "forget":
            o.forget(last)
        steps.append((step, arg, pods, res))
    o.close()
    return cfg, nodes, bound, steps
