"""ksg_preempt for a preemptor whose spread or affinity counts the nominated pods move ({"nominatedPods":
"EvaluateAll", "preemptNominatedPods": "EvaluateAll"}) against tests/nominated_preempt_reference.py:
the result and the whole candidate listing, on both dry-run kernels (the device-resident segments and the host-staged
records) and both stores (registers and the per-node workspace).  The marked preemptor runs k_nom_topo behind
k_aggregate, the two-pass status pass and the two-pass instances of k_preempt / k_preempt_seg."""
import copy
import functools

import pytest

from ksg.abi import KSG_ENOTSUP, KsgError
from nominated_preempt_reference import (ARGS, NAMESPACES2, NOW, PREEMPT_ALL, SIZES, NominatedPreemptReference,
                                         hand_cases, low, stream_reference, zoned)
from nominated_topology_reference import HOST, ZONE, labelled, pod_affinity, spread
from nominator_scenario import pod as plain_pod

pytestmark = pytest.mark.gpu

VARIANTS = ({}, {"debugHostStaged": True}, {"debugWideDryRun": True}, {"debugHostStaged": True, "debugWideDryRun": True})


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def device(native, nodes, existing, noms=(), cfg=PREEMPT_ALL):
    g = native(dict(cfg))
    for ns in NAMESPACES2:
        g.upsert_namespace(ns)
    for n in nodes:
        g.add_node(n)
    for p in existing:
        g.add_pod(p)
    for q in noms:
        g.add_nominated_pod(q)
    return g


def compare(g, pod, args, want, tag=""):
    """The call on the four device variants against (result tuple, detail)."""
    args = dict(args, listCandidates=True)
    for extra in VARIANTS:
        r, d = g.preempt(g.compile(pod), dict(args, **extra))
        assert r.as_tuple() == want[0], (tag, extra, r.as_tuple(), want[0])
        assert d == want[1], (tag, extra, d, want[1])


# ---- 1. the hand-computed cases -----------------------------------------------------------------------------------
CASES = hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_computed_cases_on_the_device(native, case):
    name, nodes, existing, noms, pod, args, want, cands, selected, _ = case
    g = device(native, nodes, existing, noms)
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    for q in noms:
        ref.add_nominated_pod(q)
    for extra in VARIANTS:  # the literals first
        r, d = g.preempt(g.compile(pod), dict(args, **extra))
        assert r.as_tuple() == want, (name, extra, r.as_tuple(), want)
        assert {c["node"]: c["victims"] for c in d["candidates"]} == cands, (name, extra, d)
        assert d["selected"] == selected
    compare(g, pod, args, ref.preempt(pod, args), name)
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 2. directed and random streams -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(family, n_nodes):
    return stream_reference(family, n_nodes)


@pytest.mark.parametrize("n_nodes", SIZES)
@pytest.mark.parametrize("family", ["directed", "random"])
def test_streams_match_reference(native, family, n_nodes):
    """Nominees on snapshot indices 0 (two), 255, 256, the last one and outside the snapshot, above, at and below the
    preemptors' priority; zone and hostname keys; both potential-node modes; offsets and numCandidates that put the
    cut inside the list."""
    nodes, existing, noms, calls, want, _ = reference(family, n_nodes)
    g = device(native, nodes, existing, noms)
    for k, (pod, args) in enumerate(calls):
        compare(g, pod, args, want[k], f"call {k}")
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 3. the segment path's two victim words ---------------------------------------------------------------------------
def test_sixty_six_victims_decided_by_the_nominee(native):
    """n0 holds 66 priority-0 web pods (v00 the most important); n1 and n2 one priority-100 web pod each.  The
    preemptor (app=web) spreads over the hostname with maxSkew 61.  With c victims back and the nominee (app=web) on
    n0, pass 1 sees c + 1 + 1 - 1 <= 61: v00..v59 are reprieved and each of v60..v65 -- the segment's victim bits
    60..63 of the first word and 0..1 of the second -- is refused by the nominee's count alone (pass 2, c + 1 - 1,
    would take one more)."""
    nodes = zoned(3, 3)
    for nd in nodes:
        for key in ("allocatable", "capacity"):
            nd["status"][key]["pods"] = "110"
    existing = []
    for k in range(66):
        p = low(f"v{k:02d}", "n0", cpu="10m", app="web")
        p["status"]["startTime"] = f"2024-01-01T00:{k // 60:02d}:{k % 60:02d}Z"
        existing.append(p)
    for k in (1, 2):
        p = low(f"k{k}", f"n{k}", cpu="10m", app="web")
        p["spec"]["priority"] = 100
        existing.append(p)
    nom = labelled(plain_pod("nom", prio=100, cpu="100m", nominated="n0"), app="web")
    pod = spread(labelled(plain_pod("pre", prio=50, cpu="100m"), app="web"), HOST, "web", max_skew=61)
    g = device(native, nodes, existing, [nom])
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    ref.add_nominated_pod(nom)
    want = ref.preempt(pod, ARGS)
    assert want[1]["victims"] == [f"v{k}" for k in range(60, 66)] and want[1]["selected"] == "n0"
    assert ref.counters()["kept"] == 6
    compare(g, pod, ARGS, want)
    g.delete_nominated_pod("nom")  # without the nominee v60 is reprieved too
    ref.delete_nominated_pod("nom")
    want = ref.preempt(pod, ARGS)
    assert want[1]["victims"] == [f"v{k}" for k in range(61, 66)]
    compare(g, pod, ARGS, want)
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 4. a preemptor that is itself nominated ------------------------------------------------------------------------
def test_the_preemptor_s_own_nomination_is_not_in_g(native):
    """The "keeps" case with the preemptor itself nominated to n0 (app=web: it would count) and another nominee,
    app=db, on n2 (it marks the preemptor and counts nowhere): v is reprieved on n0."""
    _, nodes, existing, _, pod, args, *_ = next(c for c in CASES if c[0] == "keeps")
    me = copy.deepcopy(pod)
    me["status"]["nominatedNodeName"] = "n0"
    other = labelled(plain_pod("other", prio=100, cpu="100m", nominated="n2"), app="db")
    g = device(native, nodes, existing, [me, other])
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    for q in (me, other):
        ref.add_nominated_pod(q)
    want = ref.preempt(me, args)
    assert {c["node"]: c["victims"] for c in want[1]["candidates"]} == {"n0": ["f0"], "n1": ["f1"], "n2": ["f2"]}
    compare(g, me, args, want)
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 5. a PreemptionBasic-shaped stream of spread-constrained preemptors ---------------------------------------------
def test_preemption_basic_stream_of_spread_preemptors(native):
    """12 full nodes in 3 zones; six priority-100 pods that spread over the zones (DoNotSchedule, matching their own
    label): failed cycle -> ksg_preempt -> the victims deleted -> nominated -> the next preemptor, which sees the
    earlier ones as nominees that count in its constraint -> the nominees' own cycles.  No call is refused and every
    step equals the reference."""
    nodes = zoned(12, 3)
    lows = []
    for k in range(12):
        for j in range(4):
            p = low(f"low-{k}-{j}", f"n{k}", cpu="900m", app="low")
            p["status"]["startTime"] = f"2024-01-01T00:{k:02d}:{j:02d}Z"
            lows.append(p)
    g = device(native, nodes, lows)
    ref = NominatedPreemptReference({}, nodes, lows, NAMESPACES2)
    pending, marked = [], 0
    for q in range(6):
        hi = spread(labelled(plain_pod(f"hi{q}", prio=100, cpu="2"), app="hi"), ZONE, "hi")
        want = ref.schedule(hi)
        assert want[0] == 2  # the cluster is full, or the room is spoken for
        assert g.schedule_one(g.compile(hi), assume=True)[0].as_tuple() == want, q
        args = {"offset": q, "now": NOW, "listCandidates": True, "minCandidateNodesPercentage": 100,
                "minCandidateNodesAbsolute": 100}
        want = ref.preempt(hi, args)
        assert want[0][0] == 0, (q, want)
        compare(g, hi, args, want, f"hi{q}")
        for uid in want[1]["victims"]:
            g.remove_pod(uid)
            ref.remove_pod(uid)
        hi = copy.deepcopy(hi)
        hi["status"]["nominatedNodeName"] = want[1]["selected"]
        g.add_nominated_pod(hi)
        ref.add_nominated_pod(hi)
        pending.append(hi)
        marked += q > 0
    c = ref.counters()
    assert marked == 5 and c["closed"] >= 3 and c["differs"] >= 1, c
    for p in pending:  # the nominees' own cycles
        want = ref.schedule(p)
        assert g.schedule_one(g.compile(p), assume=True)[0].as_tuple() == want, p["metadata"]["name"]
        assert want[0] == 0
    assert not ref.nominator
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 6. the config ----------------------------------------------------------------------------------------------------
def test_config_validation(native):
    for cfg in ({"preemptNominatedPods": "EvaluateAll"}, {"preemptNominatedPods": "EvaluateAll", "nominatedPods": "Evaluate"},
                {"preemptNominatedPods": "EvaluateAll", "nominatedPods": "Refuse"}):
        with pytest.raises(KsgError, match="preemptNominatedPods.*nominatedPods"):
            native(cfg)
    with pytest.raises(KsgError, match='preemptNominatedPods: Unsupported value "bogus"'):
        native({"nominatedPods": "EvaluateAll", "preemptNominatedPods": "bogus"})
    native(dict(PREEMPT_ALL)).close()
    native({"nominatedPods": "EvaluateAll", "preemptNominatedPods": "Refuse"}).close()
    native({"preemptNominatedPods": "Refuse"}).close()


@pytest.mark.parametrize("cfg", [{"nominatedPods": "EvaluateAll"},
                                 {"nominatedPods": "EvaluateAll", "preemptNominatedPods": "Refuse"}])
def test_without_the_key_the_three_pairs_are_refused_as_before(native, cfg):
    nodes = zoned(6, 2)
    g = device(native, nodes, [], [plain_pod("hi", prio=100, nominated="n1")], cfg=cfg)
    sel = "x"
    dns = spread(plain_pod("dns"), ZONE, sel)
    anti = pod_affinity(plain_pod("anti"), "podAntiAffinity", HOST, sel)
    nom_anti = pod_affinity(plain_pod("hi-anti", prio=100, nominated="n2"), "podAntiAffinity", HOST, sel)

    def refused(pod, cond):
        with pytest.raises(KsgError) as e:
            g.preempt(g.compile(pod), {"offset": 0})
        assert f"rc={KSG_ENOTSUP}" in str(e.value) and cond in str(e.value), str(e.value)

    refused(dns, "(a)")
    refused(anti, "(b)")
    g.add_nominated_pod(nom_anti)
    refused(plain_pod("plain"), "(c)")
    # and with the key none is
    g2 = device(native, nodes, [], [plain_pod("hi", prio=100, nominated="n1"), nom_anti])
    for p in (dns, anti, plain_pod("plain")):
        r, _ = g2.preempt(g2.compile(p), {"offset": 0})
        assert r.reason == 2  # nothing fails as Unschedulable on the empty cluster: no candidates
    assert g2.compare_mirror(sync=True) == (0, -1)
