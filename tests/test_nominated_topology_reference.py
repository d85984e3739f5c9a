"""tests/nominated_topology_reference.py against hand-computed literals, and the directed streams' conditions: the
reference the device is compared with (tests/test_gpu_nominated_topology.py) must itself give what
RunFilterPluginsWithNominatedPods gives where a nominee moves a spread or affinity count, and the streams must in
fact reach those pairs.  CPU only (the oracle)."""
import functools

import pytest

from nominated_topology_reference import (NAMESPACE, SIZES, NominatedTopologyReference, hand_cases, stream_reference)

CASES = hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_computed_cases(case):
    name, nodes, existing, noms, pod, failing, (status, evaluated, feasible) = case
    ref = NominatedTopologyReference({}, nodes, existing, NAMESPACE)
    for q in noms:
        ref.add_nominated_pod(q)
    d = {}
    got = ref.schedule(pod, assume=False, detail=d)
    ev = d["ev"]
    for nm, i in ref.index.items():
        st = (ev["node_code"][i], ev["node_plugin"][i], ev["node_reasons"][i])
        if nm in failing:
            assert st == failing[nm], (name, nm, st)
        else:
            assert st[0] == 0, (name, nm, st)
    assert (got[0], got[2], got[3]) == (status, evaluated, feasible), (name, got)
    assert (got[1] >= 0) == (status == 0)


def test_hand_cases_reach_their_counters():
    """(i) closes n1 and leaves its zone-mate; (iv) grants on n1 only in pass 1; (vii) is the Skip."""
    seen = {}
    for name, nodes, existing, noms, pod, _, _ in CASES:
        ref = NominatedTopologyReference({}, nodes, existing, NAMESPACE)
        for q in noms:
            ref.add_nominated_pod(q)
        ref.schedule(pod, assume=False)
        seen[name] = ref.counters()
    assert seen["i"] == {"closed": 1, "granted": 0, "split": 1, "skipped": 0}
    assert seen["ii"] == {"closed": 0, "granted": 0, "split": 0, "skipped": 0}
    assert seen["iii"] == {"closed": 1, "granted": 0, "split": 1, "skipped": 0}
    assert seen["iv"] == {"closed": 0, "granted": 1, "split": 0, "skipped": 0}
    assert seen["vi"] == {"closed": 1, "granted": 0, "split": 1, "skipped": 0}
    assert seen["vii"] == {"closed": 0, "granted": 0, "split": 0, "skipped": 1}
    assert seen["viii"] == {"closed": 1, "granted": 0, "split": 1, "skipped": 0}


@functools.lru_cache(maxsize=None)
def directed(n_nodes):
    return stream_reference("directed", n_nodes)


@pytest.mark.parametrize("n_nodes", SIZES)
def test_directed_streams_reach_the_new_pairs(n_nodes):
    """Conditions on the inputs: each directed stream does close nodes by a nominee's count, does meet an affinity
    only a nominee satisfies, does leave a closed node's zone-mates feasible, and does meet the Skip."""
    *_, want, c = directed(n_nodes)
    assert c["closed"] >= 5 and c["granted"] >= 3 and c["split"] >= 3 and c["skipped"] >= 1, c
    assert sum(t[0] == 0 for t, _ in want) > 10
