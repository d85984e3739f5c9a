"""k_sched_loop's lean selection path (loopLeanSelect, default on): for a pod that scores and whose raw
TaintToleration and NodeAffinity scores are 0 on every node (DF_RAW0), the selection wave sweeps and reduces
exchange A's counts granule only and phase 2 adds one constant to every fixed score.

Every GPU case schedules one stream three ways -- the CPU oracle, a scheduler with "loopLeanSelect": false (the
general path for every pod) and the default scheduler -- and requires equal result tuples pod by pod and a device
mirror equal to the host's.  The oracle's and the key-off scheduler's results are computed once per case.
"""
import functools

import pytest

from fuzz_gen import namespaces
from oracle_binding import oracle

gpu = pytest.mark.gpu

ZONES_PREFERRED = ["zone-3", "zone-7"]
KINDS = ("plain", "tolerating", "preferred", "tolerating-again")


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def _mixed_nodes(n_nodes):
    """SchedulingBasic's heterogeneous nodes (zone labels), one in three with a PreferNoSchedule taint."""
    from ksg.synth import scheduling_basic
    nodes, init, _ = scheduling_basic(n_nodes, n_nodes // 5, 0, hetero=True)
    for i, n in enumerate(nodes):
        if i % 3 == 1:
            n["spec"]["taints"] = [{"key": "soft", "value": "yes", "effect": "PreferNoSchedule"}]
    return nodes, init


def _mixed_pod(k):
    """Four kinds in turn: a plain pod (general path: a taint of the cluster is not tolerated), the same pod
    tolerating everything (lean), a pod with a preferred node-affinity term (general), the tolerating pod again
    (lean) -- lean and general pods follow each other in both orders."""
    from ksg.objects import PodW
    kind = k % 4
    p = PodW(f"mix-{k}", "default").container(
        requests={"cpu": f"{100 + 50 * (k % 5)}m", "memory": f"{100 + 100 * (k % 7)}Mi"})
    if kind in (1, 3):
        p.tolerations([{"operator": "Exists"}])
    elif kind == 2:
        p.node_affinity_preferred([(5, {"matchExpressions": [
            {"key": "topology.kubernetes.io/zone", "operator": "In", "values": ZONES_PREFERRED}]})])
    return p.obj()


def _mixed(n_nodes, n_pods, cfg):
    nodes, init = _mixed_nodes(n_nodes)
    return cfg, nodes, init, [_mixed_pod(k) for k in range(n_pods)]


def _basic(n_nodes, n_init, n_pods, hetero, cfg):
    from ksg.synth import scheduling_basic
    nodes, init, pods = scheduling_basic(n_nodes, n_init, n_pods, hetero=hetero)
    return cfg, nodes, init, pods


def _flips():
    """Every pod takes more than half a node's cpu: the chosen node turns infeasible for the next pod, and the
    pods beyond one per node find no node at all."""
    from ksg.objects import PodW
    from ksg.synth import node_default
    nodes = [node_default(f"node-{i:06d}") for i in range(150)]
    pods = [PodW(f"big-{k}", "default").container(requests={"cpu": "2100m", "memory": "500Mi"}).obj()
            for k in range(170)]
    return {}, nodes, [], pods


CASES = {
    # three 128-node units, the last with 44 nodes
    "mixed-300": lambda: _mixed(300, 240, {}),
    # the constant addend: TaintToleration's weight 5, and the plugin absent (addend 0)
    "mixed-300-tt-weight-5": lambda: _mixed(300, 240, {"scoreWeights": {"TaintToleration": "5"}}),
    "mixed-300-tt-disabled": lambda: _mixed(300, 240, {"disabledPlugins": ["TaintToleration"]}),
    # all-tied cluster, one workgroup with two units: only the pre-order key decides
    "tied-200-wg1": lambda: _basic(200, 40, 250, False, {"loopWorkgroups": 1}),
    # a lean pod on the cut path: endn and processedNodes
    "pct30": lambda: _basic(700, 140, 300, True, {"percentageOfNodesToScore": 30}),
    "feasibility-flips": _flips,
    # the NW = 4 and the unsplit instances
    "mixed-300-unit-256": lambda: _mixed(300, 240, {"loopUnit": 256}),
    "mixed-300-unsplit": lambda: _mixed(300, 240, {"loopSplitEval": False}),
    # 66 workgroups: more than one sweep round
    "sweep-rounds-8400": lambda: _basic(8400, 500, 120, True, {}),
}
MIXED = [n for n in CASES if n.startswith("mixed-300")]


def _load(b, nodes, init):
    for ns in namespaces():
        b.upsert_namespace(ns)
    for n in nodes:
        b.add_node(n)
    for p in init:
        b.add_pod(p)
    return b


@functools.lru_cache(maxsize=None)
def _oracle_results(name):
    """(the case, the oracle's result tuples)"""
    case = CASES[name]()
    cfg, nodes, init, pods = case
    o = _load(oracle(dict(cfg)), nodes, init)
    return case, o.node_names(), [o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in pods]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(the case, the oracle's result tuples, the result tuples with loopLeanSelect false)"""
    from ksg.native import Scheduler
    case, names, want = _oracle_results(name)
    cfg, nodes, init, pods = case
    g = _load(Scheduler(dict(cfg, loopLeanSelect=False)), nodes, init)
    assert g.node_names() == names
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    assert g.kernel_stats()[3] == "k_sched_loop"
    assert g.lean_pods() == (0, 0)  # counted only while the key is on
    general = [r.as_tuple() for r in rs]
    g.close()
    return case, want, general


def test_mixed_stream_has_every_kind():
    """No GPU: the mixed stream holds at least 60 pods of each kind, and the oracle places pods of each kind."""
    (_, _, _, pods), _, want = _oracle_results("mixed-300")
    for kind in range(4):
        mine = [want[k] for k in range(len(pods)) if k % 4 == kind]
        assert len(mine) >= 60, (KINDS[kind], len(mine))
        assert sum(1 for r in mine if r[0] == 0) >= 1, f"no {KINDS[kind]} pod placed"


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_lean_select_matches_oracle_and_general(native, name):
    (cfg, nodes, init, pods), want, general = _reference(name)
    g = _load(native(dict(cfg)), nodes, init)
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    ms, by, ran, kernel = g.kernel_stats()
    assert kernel == "k_sched_loop"
    for k in range(len(pods)):
        assert rs[k].as_tuple() == want[k], f"{name} pod {k}: {rs[k].as_tuple()} != oracle {want[k]}"
        assert rs[k].as_tuple() == general[k], f"{name} pod {k}: {rs[k].as_tuple()} != key off {general[k]}"
    assert g.compare_mirror(sync=False) == (0, -1)
    lean, gen = g.lean_pods()
    g.close()
    assert lean + gen == ran, (lean, gen, ran)
    if name in MIXED:  # both paths ran, in turn
        assert lean > 0 and gen > 0, (lean, gen)
        if name != "mixed-300-tt-disabled":  # (without the plugin the plain pods' raw scores are 0 too)
            assert (lean, gen) == (len(pods) // 2, len(pods) // 2)
    else:  # pod-default pods on clusters without taints: every pod is lean
        assert gen == 0 and lean == len(pods), (lean, gen)
    if name == "feasibility-flips":  # one pod per node, then no feasible node
        assert [r.status == 0 for r in rs] == [True] * 150 + [False] * 20


@gpu
@pytest.mark.parametrize("mask", [1, 2, 4])
def test_lean_select_parts_alone(native, mask):
    """loopLeanSelect as a number enables the path's parts one by one (the measurements' switch): the lean sweep,
    the lean phase 2, phase 1's unreduced maxima -- each alone gives the same results."""
    (cfg, nodes, init, pods), want, general = _reference("mixed-300")
    g = _load(native(dict(cfg, loopLeanSelect=mask)), nodes, init)
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    assert g.kernel_stats()[3] == "k_sched_loop"
    for k in range(len(pods)):
        assert rs[k].as_tuple() == want[k], f"mask {mask} pod {k}: {rs[k].as_tuple()} != oracle {want[k]}"
        assert rs[k].as_tuple() == general[k], f"mask {mask} pod {k}: {rs[k].as_tuple()} != key off {general[k]}"
    assert g.compare_mirror(sync=False) == (0, -1)
    assert g.lean_pods() == (len(pods) // 2, len(pods) // 2)
    g.close()


@gpu
def test_lean_select_resident_calls(native):
    """60 single-pod calls of the mixed stream through the resident loop."""
    (cfg, nodes, init, pods), names, want = _oracle_results("mixed-300")
    off = _load(native(dict(cfg, loopLeanSelect=False)), nodes, init)
    g = _load(native(dict(cfg)), nodes, init)
    assert g.node_names() == names
    for k in range(60):
        r0 = off.schedule_one(off.compile(pods[k]), assume=True)[0].as_tuple()
        r1 = g.schedule_one(g.compile(pods[k]), assume=True)[0].as_tuple()
        assert r1 == want[k], f"call {k}: {r1} != oracle {want[k]}"
        assert r1 == r0, f"call {k}: {r1} != key off {r0}"
    assert g.compare_mirror(sync=False) == (0, -1)
    assert off.lean_pods() == (0, 0)
    assert g.lean_pods() == (30, 30)
    off.close()
    g.close()
