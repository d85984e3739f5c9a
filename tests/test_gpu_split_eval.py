"""k_sched_loop's split instance (loopSplitEval, the default for unsharded 128-node-unit batch runs): the
"as it is" and the "as if the previous pod landed here" evaluations of phase 1 on separate waves.

Every case compares each pod's result with the CPU oracle and with a second scheduler that runs the
unsplit instance ("loopSplitEval": false), under both role placements of the split instance
(loopWaveMap 0 and 1).  The oracle's and the unsplit scheduler's results are computed once per case.
"""
import functools

import pytest

from fuzz_gen import namespaces, rand_cluster, rand_pod
from oracle_binding import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def _units(n_nodes, wg, hetero):
    from ksg.synth import scheduling_basic
    nodes, init, pods = scheduling_basic(n_nodes, n_nodes // 5, 250, hetero=hetero)
    return ({"loopWorkgroups": wg} if wg else {}), nodes, init, pods


def _prepared_and_fixup(hetero):
    """test_sched_loop_prepared_and_fixup_paths' stream: rounds with and without a prepared evaluation."""
    from ksg.objects import PodW
    from ksg.synth import scheduling_basic
    nodes, init, base = scheduling_basic(1500, 200, 180, hetero=hetero)
    pods = []
    for k, p in enumerate(base):
        if k % 7 in (3, 4):  # two host-port pods in a row: the second cannot be prepared
            p = PodW(f"hp{k}", uid=f"hp{k}").container(requests={"cpu": "100m"}).host_port(8000 + k % 5).obj()
        elif k % 11 == 5:
            p = PodW(f"na{k}", uid=f"na{k}").container(requests={"cpu": "200m"}).node_affinity_in(
                "kubernetes.io/hostname", [nodes[j]["metadata"]["name"] for j in range(k % 9, 1500, 13)]).obj()
        pods.append(p)
    return {}, nodes, init, pods


def _flips():
    """Every pod takes more than half a node's cpu: the chosen node turns infeasible for the next pod, and
    the pods beyond one per node find no node at all."""
    from ksg.objects import PodW
    from ksg.synth import node_default
    nodes = [node_default(f"node-{i:06d}") for i in range(150)]
    pods = [PodW(f"big-{k}", "default").container(requests={"cpu": "2100m", "memory": "500Mi"}).obj()
            for k in range(170)]
    return {}, nodes, [], pods


def _basic(n_nodes, n_init, n_pods, cfg):
    from ksg.synth import scheduling_basic
    nodes, init, pods = scheduling_basic(n_nodes, n_init, n_pods, hetero=True)
    return cfg, nodes, init, pods


def _random(seed):
    rng, cfg, nodes, existing, names = rand_cluster(seed, n_nodes=800, n_existing=100, topology=False)
    return dict(cfg), nodes, existing, [rand_pod(rng, k, names, topology=False) for k in range(200)]


CASES = {
    # one workgroup, two units, the last one partial
    "units-200-wg1-hetero": lambda: _units(200, 1, True),
    "units-200-wg1-tied": lambda: _units(200, 1, False),
    # three units, the last with 44 nodes
    "units-300-hetero": lambda: _units(300, 0, True),
    "units-300-tied": lambda: _units(300, 0, False),
    # nine units over five workgroups: one or two each
    "units-1100-wg5-hetero": lambda: _units(1100, 5, True),
    "units-1100-wg5-tied": lambda: _units(1100, 5, False),
    "prepared-fixup-hetero": lambda: _prepared_and_fixup(True),
    "prepared-fixup-tied": lambda: _prepared_and_fixup(False),
    "feasibility-flips": _flips,
    "pct30": lambda: _basic(700, 140, 300, {"percentageOfNodesToScore": 30}),
    "sweep-rounds-8400": lambda: _basic(8400, 500, 120, {}),  # 66 workgroups: more than one sweep round
    "chunks-and-launches": lambda: _basic(700, 100, 600, {}),
    "random-9701": lambda: _random(9701),
    "random-9702": lambda: _random(9702),
}


def _load(b, nodes, init):
    for ns in namespaces():
        b.upsert_namespace(ns)
    for n in nodes:
        b.add_node(n)
    for p in init:
        b.add_pod(p)
    return b


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(the case, the oracle's result tuples, the unsplit instance's result tuples)"""
    from ksg.native import Scheduler
    case = CASES[name]()
    cfg, nodes, init, pods = case
    o = _load(oracle(dict(cfg)), nodes, init)
    want = [o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in pods]
    g = _load(Scheduler(dict(cfg, loopSplitEval=False)), nodes, init)
    assert g.node_names() == o.node_names()
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    assert g.kernel_stats()[3] == "k_sched_loop"
    unsplit = [r.as_tuple() for r in rs]
    g.close()
    return case, want, unsplit


@pytest.mark.parametrize("wave_map", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_split_eval_matches_oracle_and_unsplit(native, name, wave_map):
    (cfg, nodes, init, pods), want, unsplit = _reference(name)
    g = _load(native(dict(cfg, loopWaveMap=wave_map)), nodes, init)
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    assert g.kernel_stats()[3] == "k_sched_loop"
    for k in range(len(pods)):
        assert rs[k].as_tuple() == want[k], f"{name} map {wave_map} pod {k}: {rs[k].as_tuple()} != oracle {want[k]}"
        assert rs[k].as_tuple() == unsplit[k], f"{name} map {wave_map} pod {k}: {rs[k].as_tuple()} != unsplit {unsplit[k]}"
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()
    if name.startswith("units-200"):  # the chosen nodes fall in both units and in both evaluation waves
        at = {(r.node_index // 128, r.node_index % 128 // 64) for r in rs if r.status == 0}
        assert {u for u, _ in at} == {0, 1} and {v for _, v in at} == {0, 1}, at
    if name == "feasibility-flips":  # one pod per node, then no feasible node
        assert [r.status == 0 for r in rs] == [True] * 150 + [False] * 20
