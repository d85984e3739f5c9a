"""tests/nominated_preempt_reference.py against the oracle where the oracle can answer (nothing nominated, or
nominees only node-local filters read), against literals worked out by hand, and the streams' reach: the inputs of
tests/test_gpu_nominated_preempt.py do exercise the steps only the two passes decide.  No GPU."""
import copy
import functools
import random

import pytest

from nominated_preempt_reference import (NAMESPACES2, SIZES, NominatedPreemptReference, hand_cases, stream_reference)
from nominated_reference import NominatedReference
from oracle_binding import oracle
from test_gpu_preempt import build, cluster, mk_pod, pdbs, spread_cluster


def preempt_args(rng):
    args = {"offset": rng.randrange(1000), "now": 1704067200 * 10 ** 9 + rng.randrange(3600) * 10 ** 9,
            "pdbs": pdbs(rng), "allNodes": rng.random() < 0.3, "listCandidates": True,
            "minCandidateNodesPercentage": rng.choice([0, 10, 40, 100]),
            "minCandidateNodesAbsolute": rng.choice([1, 3, 100])}
    return args


@pytest.mark.parametrize("seed", range(3))
def test_equals_the_oracle_with_nothing_nominated(seed):
    """test_gpu_preempt.cluster inputs, PodDisruptionBudgets included, some calls actuated: the restated dry run (the
    victim order, the PDB split, the reprieve, the cut, the pick) equals the oracle's own."""
    rng, nodes, existing = cluster(seed, 40 + 30 * seed, 6)
    orc = build(oracle, nodes, existing)
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    found = 0
    for q in range(10):
        pod = mk_pod(f"pre{q}", rng, prio=rng.choice([100, 500, 1000]), big=True)
        args = preempt_args(rng)
        r, d = orc.preempt(orc.compile(pod), args)
        got = ref.preempt(pod, args)
        assert got[0] == r.as_tuple(), (q, got[0], r.as_tuple())
        assert got[1] == d, q
        found += r.status == 0
        if r.status == 0 and q % 3 == 0:  # the victims go, the pod binds: NodeInfo.Pods order changes on both
            for uid in d["victims"]:
                orc.remove_pod(uid)
                ref.remove_pod(uid)
            p2 = dict(pod, spec=dict(pod["spec"], nodeName=d["selected"]))
            orc.add_pod(p2)
            ref.add_pod(p2)
    assert found > 0
    assert ref.counters() == {"closed": 0, "granted": 0, "kept": 0, "skipped": 0, "differs": 0}


def test_equals_the_oracle_on_spread_preemptors():
    """Victims that move the preemptor's own spread counts, nothing nominated."""
    rng, nodes, existing = spread_cluster(100, 40)
    orc = build(oracle, nodes, existing)
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    for q in range(6):
        pod = mk_pod(f"pre{q}", rng, prio=rng.choice([500, 1000]), big=True)
        pod["metadata"]["namespace"] = "default"
        pod["metadata"]["labels"] = {"app": rng.choice(["a", "b"])}
        pod["spec"]["topologySpreadConstraints"] = [
            {"maxSkew": rng.choice([1, 2]), "topologyKey": k, "whenUnsatisfiable": "DoNotSchedule",
             "labelSelector": {"matchLabels": {"app": rng.choice(["a", "b"])}}}
            for k in rng.sample(["topology.kubernetes.io/zone", "kubernetes.io/hostname"], rng.choice([1, 2]))]
        args = dict(preempt_args(rng), now=1704153600 * 10 ** 9)
        r, d = orc.preempt(orc.compile(pod), args)
        assert ref.preempt(pod, args) == (r.as_tuple(), d), q


@pytest.mark.parametrize("seed", range(2))
def test_equals_the_one_pass_reference_on_node_local_nominees(seed):
    """The inputs of test_gpu_nominated_pods.test_preemption_under_nominations: only NodeResourcesFit and NodePorts read
    the nominees, so adding G everywhere in one pass (NominatedReference.preempt) is exact."""
    from test_gpu_nominated_pods import nominee
    rng, nodes, existing = cluster(300 + seed, 40 + 20 * seed, 6)
    one = NominatedReference({}, nodes, existing, NAMESPACES2)
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    for k in range(10):
        q = nominee(f"nom{k}", [1000, 500, 100][k % 3], rng.choice(ref.names), cpu=rng.choice(["500m", "1500m"]),
                    port=8080 if k % 4 == 0 else None, gpu=1 if k % 5 == 1 else None)
        one.add_nominated_pod(q)
        ref.add_nominated_pod(q)
    for q in range(8):
        pod = mk_pod(f"pre{q}", rng, prio=500, big=True)
        args = {"offset": rng.randrange(1000), "now": 1704067200 * 10 ** 9 + rng.randrange(3600) * 10 ** 9,
                "pdbs": pdbs(rng), "allNodes": rng.random() < 0.3, "listCandidates": True,
                "minCandidateNodesPercentage": rng.choice([10, 40, 100]),
                "minCandidateNodesAbsolute": rng.choice([1, 3, 100])}
        assert ref.preempt(pod, args) == one.preempt(pod, args), q
    c = ref.counters()
    assert (c["closed"], c["granted"], c["kept"], c["differs"]) == (0, 0, 0, 0)


CASES = hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_computed_cases(case):
    name, nodes, existing, noms, pod, args, want, cands, selected, reach = case
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    for q in noms:
        ref.add_nominated_pod(q)
    before = copy.deepcopy(ref.order)
    got, d = ref.preempt(pod, args)
    assert got == want, (name, got, want)
    assert {c["node"]: c["victims"] for c in d["candidates"]} == cands, (name, d)
    assert d["selected"] == selected
    assert d["victims"] == (cands[selected] if selected else [])
    for k, v in reach.items():
        assert ref.counters()[k] == v, (name, ref.counters())
    # the dry run left the oracle context as it found it: the same call again gives the same answer
    assert ref.order == before and ref.preempt(pod, args) == (got, d)


def test_hand_cases_differ_without_the_nominee():
    """Cases 1 and 3 without their nominee: n0 is a candidate, and v is reprieved."""
    by = {c[0]: c for c in CASES}
    for name, want in (("closes", {"n0": ["f0"], "n1": ["f1"]}), ("keeps", {"n0": ["f0"], "n1": ["f1"], "n2": ["f2"]})):
        _, nodes, existing, _, pod, args, *_ = by[name]
        ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
        _, d = ref.preempt(pod, args)
        assert {c["node"]: c["victims"] for c in d["candidates"]} == want, (name, d)


@functools.lru_cache(maxsize=None)
def reference(family, n_nodes):
    return stream_reference(family, n_nodes)


@pytest.mark.parametrize("family", ["directed", "random"])
def test_streams_reach_the_two_pass_steps(family):
    """Per stream family, over its sizes: nodes only pass 1 closes, nodes only the nominee would grant, reprieves only
    pass 1 refuses, and calls whose outcome neither simplification gives."""
    total = {}
    for n in SIZES:
        for k, v in reference(family, n)[5].items():
            total[k] = total.get(k, 0) + v
    assert total["closed"] >= 3 and total["granted"] >= 3 and total["kept"] >= 3 and total["differs"] >= 3, total


def test_streams_hold_outcomes_of_every_kind():
    ok = none = cut = 0
    for family in ("directed", "random"):
        for n in SIZES:
            for (res, d) in reference(family, n)[4]:
                ok += res[0] == 0
                none += res[1] == 2
                cut += 0 < res[4] < res[3] and res[4] == d["numCandidates"]
    assert ok >= 10 and none >= 1 and cut >= 3, (ok, none, cut)


def test_rng_is_not_shared():
    """Two builds of one stream are the same stream (the GPU tests cache theirs separately)."""
    random.seed(1)
    a = stream_reference("directed", 9)
    random.seed(2)
    assert stream_reference("directed", 9)[4] == a[4]
