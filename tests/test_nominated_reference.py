"""The test reference for filtering with other pods' nominations (tests/nominated_reference.py) checked by
itself, on the CPU: with an empty nominator it is the oracle's own scheduling cycle, and a hand-computed case pins
what a nomination of equal or higher priority does to a node's status (RunFilterPluginsWithNominatedPods,
framework.go:1211-1294).  tests/test_gpu_nominated_pods.py then holds the device to this reference."""
import copy

from fuzz_gen import namespaces, rand_cluster, rand_pod
from ksg.abi import PLUGIN_ID
from nominated_reference import NominatedReference
from nominator_scenario import node, pod
from oracle_binding import oracle

R_INSUFFICIENT_CPU = 1 << 7  # KSG_R_INSUFFICIENT_CPU


def test_empty_nominator_is_the_oracle_cycle():
    """130 nodes, 40 existing pods, 60 pods (every node-local feature, PodTopologySpread and InterPodAffinity
    included): tuple by tuple the helper is oracle.schedule_one(assume=True)."""
    rng, cfg, nodes, existing, names = rand_cluster(11, n_nodes=130, n_existing=40)
    ref = NominatedReference(cfg, nodes, existing, namespaces=namespaces())
    o = oracle(cfg)
    for ns in namespaces():
        o.upsert_namespace(ns)
    for n in nodes:
        o.add_node(n)
    for p in existing:
        o.add_pod(p)
    assert ref.names == o.node_names()
    placed = 0
    for k in range(60):
        p = rand_pod(rng, k, names)
        want = o.schedule_one(o.compile(p), assume=True)[0].as_tuple()
        got = ref.schedule(copy.deepcopy(p))
        assert got == want, (k, got, want)
        placed += want[0] == 0
    assert placed > 20


def test_hand_computed_case():
    """Four nodes of 4 cpu; a priority-100 pod of 3500m is nominated to n1."""
    nodes = [node(f"n{k}") for k in range(4)]
    ref = NominatedReference({}, nodes, [], namespaces=[{"metadata": {"name": "default"}}])
    n1 = ref.index["n1"]
    ref.add_nominated_pod(pod("hi", prio=100, cpu="3500m", nominated="n1"))

    d = {}
    r = ref.schedule(pod("low", prio=0, cpu="1"), assume=False, detail=d)
    ev = d["ev"]
    assert (ev["node_code"][n1], ev["node_plugin"][n1], ev["node_reasons"][n1]) == \
        (2, PLUGIN_ID["NodeResourcesFit"], R_INSUFFICIENT_CPU)  # Unschedulable, exactly "Insufficient cpu"
    assert [c for i, c in enumerate(ev["node_code"]) if i != n1] == [0, 0, 0]
    assert r[0] == 0 and r[3] == 3 and r[1] != n1
    ref.next_start = 0

    r = ref.schedule(pod("top", prio=200, cpu="1"), assume=False)  # a higher priority: the nomination is not added
    assert r[0] == 0 and r[3] == 4
    ref.next_start = 0

    # the nominated pod itself: its own record is not in its G; its nominated node alone, feasible
    r = ref.schedule(pod("hi", prio=100, cpu="3500m", nominated="n1"))
    assert r == (0, n1, 1, 1, 0)
    assert ref.next_start == 0 and not ref.nominator  # nextStartNodeIndex stays; the assume ended the nomination

    d = {}
    r = ref.schedule(pod("low2", prio=0, cpu="1"), assume=False, detail=d)  # n1 holds the 3500m for real now
    assert (d["ev"]["node_code"][n1], d["ev"]["node_reasons"][n1]) == (2, R_INSUFFICIENT_CPU)
    assert r[3] == 3
    d = {}
    r = ref.schedule(pod("tiny", prio=0, cpu="500m"), assume=False, detail=d)  # exactly what is left of n1
    assert d["ev"]["node_code"][n1] == 0 and r[3] == 4
