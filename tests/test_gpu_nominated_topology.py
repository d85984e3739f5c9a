"""Nominated pods that move spread or affinity counts, on the device ({"nominatedPods": "EvaluateAll"}, DESIGN.md
§4.10) against tests/nominated_topology_reference.py, pod by pod.  Such a pod is marked by the host, leaves both
persistent loops, and runs k_nom_topo behind k_aggregate and the two-pass instances of the node pass; the reference
does the literal two passes, each node's nominees added for that node alone.  Every test creates an "EvaluateAll"
context."""
import copy
import functools
import uuid

import pytest

from diagnosis_reference import reduce_eval
from fuzz_gen import namespaces
from ksg.abi import KSG_ENOTSUP, KsgError
from nominated_reference import eval_fields
from nominated_topology_reference import (EVALUATE_ALL, HOST, NAMESPACE, SIZES, ZONE, NominatedTopologyReference,
                                          bound, hand_cases, labelled, pod_affinity, spread, stream_reference,
                                          zoned_nodes)
from nominator_scenario import pod as plain_pod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def device(native, cfg, nodes, existing, nss=(), noms=()):
    g = native(dict(cfg, **EVALUATE_ALL))
    for ns in nss:
        g.upsert_namespace(ns)
    for n in nodes:
        g.add_node(n)
    for p in existing:
        g.add_pod(p)
    for q in noms:
        g.add_nominated_pod(q)
    return g


def check_eval(eg, d, n, tag):
    code, plug, reas, mask, norm, total = eval_fields(d, n)
    assert eg["node_code"] == code, f"{tag}: node_code"
    assert eg["node_plugin"] == plug, f"{tag}: node_plugin"
    assert eg["node_reasons"] == reas, f"{tag}: node_reasons"
    if len(d["feasible"]) > 1:  # scored: the scores never see a nominee
        w = d["weights"]
        assert eg["score_plugin_mask"] == mask, f"{tag}: score mask {eg['score_plugin_mask']:#x} != {mask:#x}"
        for p in range(len(norm)):
            for i in d["feasible"]:
                assert eg["normalized_scores"][p][i] == norm[p][i], f"{tag}: normalized score, plugin {p} node {i}"
                assert eg["plugin_scores"][p][i] == norm[p][i] * w.get(p, 0) * (mask >> p & 1), \
                    f"{tag}: plugin score, plugin {p} node {i}"
        for i in d["feasible"]:
            assert eg["total_scores"][i] == total[i], f"{tag}: total score, node {i}"


# ---- 1. the hand-computed cases -----------------------------------------------------------------------------------
CASES = hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_computed_cases_on_the_device(native, case):
    name, nodes, existing, noms, pod, failing, (status, evaluated, feasible) = case
    g = device(native, {}, nodes, existing, NAMESPACE, noms)
    ref = NominatedTopologyReference({}, nodes, existing, NAMESPACE)
    for q in noms:
        ref.add_nominated_pod(q)
    d = {}
    want = ref.schedule(pod, assume=False, detail=d)
    d["weights"] = ref.weights
    rg, eg = g.schedule_one(g.compile(pod), assume=False, evaluate=True)
    for nm, i in ref.index.items():  # the literals first, then everything against the reference
        st = (eg["node_code"][i], eg["node_plugin"][i], eg["node_reasons"][i])
        assert st == failing[nm] if nm in failing else st[0] == 0, (name, nm, st)
    assert rg.as_tuple() == want, (name, rg.as_tuple(), want)
    assert (rg.status, rg.evaluated_nodes, rg.feasible_nodes) == (status, evaluated, feasible)
    check_eval(eg, d, len(nodes), name)
    # the same cycle without evaluation output, then assumed
    assert g.schedule_one(g.compile(pod), assume=False)[0].as_tuple() == ref.schedule(pod, assume=False)
    assert g.schedule_one(g.compile(pod), assume=True)[0].as_tuple() == ref.schedule(pod, assume=True)
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 2. directed and random streams -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(family, n_nodes):
    return stream_reference(family, n_nodes)


def marked(pod, noms, names):
    """The host's mark (Engine::check_nominations): the pod would see a nominee on a snapshot node and (a) has a
    DoNotSchedule constraint, (b) a required pod (anti-)affinity term, or (c) such a nominee has a required
    anti-affinity term.  (The streams' profiles have no default DoNotSchedule constraints.)"""
    prio = lambda p: int(p["spec"].get("priority") or 0)  # noqa: E731
    req = lambda p, kind: ((p["spec"].get("affinity") or {}).get(kind) or {}).get(  # noqa: E731
        "requiredDuringSchedulingIgnoredDuringExecution")
    seen = [q for q in noms if q["metadata"]["uid"] != pod["metadata"]["uid"] and prio(q) >= prio(pod)
            and q["status"].get("nominatedNodeName") in names]
    if not seen:
        return False
    dns = any(c["whenUnsatisfiable"] == "DoNotSchedule" for c in pod["spec"].get("topologySpreadConstraints") or [])
    return bool(dns or req(pod, "podAffinity") or req(pod, "podAntiAffinity")
                or any(req(q, "podAntiAffinity") for q in seen))


@pytest.mark.parametrize("mode", ["batch", "calls", "eval"])
@pytest.mark.parametrize("n_nodes", SIZES)
@pytest.mark.parametrize("family", ["directed", "random"])
def test_streams_match_reference(native, family, n_nodes, mode):
    cfg, nodes, existing, noms, pods, want, _ = reference(family, n_nodes)
    g = device(native, cfg, nodes, existing, namespaces(), noms)
    if mode == "batch":
        got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
        for k in range(len(pods)):
            assert got[k] == want[k][0], f"pod {k}: {got[k]} != reference {want[k][0]}"
        # the batch ran as runs that end at the nominees' own cycles; in the last one the marked pods took the
        # per-pod launches: a loop ran at most the others
        names = set(g.node_names())
        own = {q["metadata"]["uid"] for q in noms}
        last = max(k for k, p in enumerate(pods) if p["metadata"]["uid"] in own) + 1
        tail = pods[last:]
        left = [q for q in noms if all(q["metadata"]["uid"] != p["metadata"]["uid"] for p in pods[:last])]
        n_marked = sum(marked(p, left, names) for p in tail)
        assert n_marked >= 1
        _, _, launches, kernel = g.kernel_stats()
        if kernel != "k_filter_score":
            assert launches <= len(tail) - n_marked, (kernel, launches, len(tail), n_marked)
    else:
        for k, p in enumerate(pods):
            rg, eg = g.schedule_one(g.compile(p), assume=True, evaluate=mode == "eval")
            assert rg.as_tuple() == want[k][0], f"pod {k}: {rg.as_tuple()} != reference {want[k][0]}"
            if eg is not None and want[k][1]["feasible"]:  # (not the pod's own nominated node tried alone)
                check_eval(eg, want[k][1], n_nodes, f"pod {k}")
    assert g.compare_mirror(sync=True) == (0, -1)  # the deltas leaked nothing into the mirror or the pod table
    assert g.loop_stats() == (0, 0)


# ---- 3. marked pods leave the loop, unmarked pods of the same batch stay ---------------------------------------------
def test_marked_pods_take_the_launch_path_unmarked_stay_in_the_loop(native):
    """48 plain pods and 16 spread-constrained ones in one batch under two nominations without anti-affinity terms:
    only the 16 are in a pair (a)-(c).  k_sched_loop runs exactly the 48."""
    nodes = zoned_nodes(130, 3)
    noms = [labelled(plain_pod(f"nom{k}", prio=100, cpu="100m", nominated=f"n{[0, 129][k]}"), app="web")
            for k in range(2)]
    g = device(native, {}, nodes, [], NAMESPACE, noms)
    ref = NominatedTopologyReference({}, nodes, [], NAMESPACE)
    for q in noms:
        ref.add_nominated_pod(q)
    pods = []
    for k in range(64):
        p = labelled(plain_pod(f"p{k}", cpu="100m"), app="web")
        pods.append(spread(p, HOST, "web") if k % 4 == 3 else p)
    got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    _, _, launches, kernel = g.kernel_stats()
    assert (kernel, launches) == ("k_sched_loop", 48)
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k}: {got[k]} != reference {want}"
    assert ref.closed >= 2  # the first spread pods found a nominated node closed by the nominee's count alone
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


# ---- 4. a batch that holds the nominees themselves ------------------------------------------------------------------
def test_batch_holding_the_nominees_themselves(native):
    """Spread pods before, between and after the cycles of two nominees of the same node: the pods before each see
    its count on n1 only in n1's pass 1, the pods after it see it bound (every node of the zone does)."""
    nodes = zoned_nodes(8, 2)
    a = labelled(plain_pod("A", prio=100, cpu="100m", nominated="n1"), app="web")
    b = labelled(plain_pod("B", prio=50, cpu="100m", nominated="n1"), app="web")
    g = device(native, {}, nodes, [], NAMESPACE, [a, b])
    ref = NominatedTopologyReference({}, nodes, [], NAMESPACE)
    for q in (a, b):
        ref.add_nominated_pod(q)
    sp = lambda k, prio: spread(labelled(plain_pod(f"p{k}", prio=prio, cpu="100m"), app="web"), ZONE, "web")  # noqa: E731
    pods = [sp(k, 0) for k in range(4)] + [b] + [sp(k, 60) for k in range(4, 8)] + [a] + [sp(k, 0) for k in range(8, 12)]
    got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k} ({p['metadata']['name']}): {got[k]} != reference {want}"
    assert ref.closed >= 1 and not ref.nominator
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 5. the pod's own nominated node with others nominated to it ------------------------------------------------------
@pytest.mark.parametrize("app", ["web", "db"])
def test_own_nominated_node_under_other_nominations(native, app):
    """The pod is nominated to n1 and so is a higher-priority pod: evaluateNominatedNode filters n1 alone with the
    other nominee added.  app=web: the nominee's count breaks the skew on n1 and the full pass follows; app=db: it
    does not count and the pod goes to n1."""
    nodes = zoned_nodes(4, 2)
    existing = [bound(f"e{k}", f"n{k}", app="web") for k in range(2)]
    hi = labelled(plain_pod("hi", prio=100, nominated="n1"), app=app)
    g = device(native, {}, nodes, existing, NAMESPACE, [hi])
    ref = NominatedTopologyReference({}, nodes, existing, NAMESPACE)
    ref.add_nominated_pod(hi)
    me = spread(labelled(plain_pod("me", prio=10, nominated="n1"), app="web"), ZONE, "web")
    for b_ in (g, ref):
        b_.add_nominated_pod(me)
    d = {}
    want = ref.schedule(me, assume=False, detail=d)
    d["weights"] = ref.weights
    rg, eg = g.schedule_one(g.compile(me), assume=False, evaluate=True)
    assert rg.as_tuple() == want
    n1 = ref.index["n1"]
    if app == "web":
        assert want[0] == 0 and want[1] != n1 and want[3] == 3
        check_eval(eg, d, 4, "own nominated node failed alone")
    else:
        assert want == (0, n1, 1, 1, 0)
    assert g.schedule_one(g.compile(me), assume=True)[0].as_tuple() == ref.schedule(me, assume=True)
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 6. the sampled pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "calls"])
def test_sampled_pass(native, mode):
    """percentageOfNodesToScore 50 on 600 nodes: numFeasibleNodesToFind is 300; the nominated nodes sit inside the
    first rotation window and are closed to the spread pods by their nominees' counts."""
    nodes = zoned_nodes(600, 3)
    cfg = {"percentageOfNodesToScore": 50}
    ref = NominatedTopologyReference(cfg, nodes, [], NAMESPACE)
    noms = [labelled(plain_pod(f"nom{k}", prio=[100, 0][k % 2], cpu="100m", nominated=ref.names[ix]), app="web")
            for k, ix in enumerate([0, 3, 17, 64, 255, 256, 299])]
    g = device(native, cfg, nodes, [], NAMESPACE, noms)
    for q in noms:
        ref.add_nominated_pod(q)
    pods = []
    for k in range(24):
        p = labelled(plain_pod(f"p{k}", prio=[0, 100][k % 2], cpu="100m"), app="web")
        if k % 3 == 0:
            spread(p, HOST, "web")
        elif k % 3 == 1:
            pod_affinity(p, "podAntiAffinity", HOST, "web")
        pods.append(p)
    if mode == "batch":
        got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    else:
        got = [g.schedule_one(g.compile(p), assume=True)[0].as_tuple() for p in pods]
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k}: {got[k]} != reference {want}"
        assert want[3] == 300
    assert got[0][2] > 300 and ref.closed >= 8  # the first window held nodes only the nominees' counts closed
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 7. the diagnosis ------------------------------------------------------------------------------------------------
def test_batch_diagnosis_follows_the_merged_statuses(native):
    """ksg_schedule_batch_diag: each pod's row is the reduction of its merged statuses (st1 where pass 1 failed, else
    st0) -- here pods whose required affinity only nominees satisfy (unschedulable: every node fails in pass 2) and
    spread pods a nominee's count closes one node to."""
    nodes = zoned_nodes(9, 3)
    existing = [bound("e0", "n4", app="web")]
    noms = [labelled(plain_pod(f"nom{k}", prio=100, cpu="100m", nominated=f"n{[0, 0, 8][k]}"), app=["db", "web", "db"][k])
            for k in range(3)]
    g = device(native, {}, nodes, existing, NAMESPACE, noms)
    ref = NominatedTopologyReference({}, nodes, existing, NAMESPACE)
    for q in noms:
        ref.add_nominated_pod(q)
    pods = []
    for k in range(12):
        p = labelled(plain_pod(f"p{k}", cpu="100m"), app="web")
        if k % 3 == 0:
            pod_affinity(p, "podAffinity", ZONE, "db")
        elif k % 3 == 1:
            spread(p, ZONE, "web")
        else:
            pod_affinity(spread(p, HOST, "web"), "podAntiAffinity", ZONE, "db")
        pods.append(p)
    rs, ds = g.schedule_batch_diag([g.compile(p) for p in pods], assume=True)
    unsched = 0
    for k, p in enumerate(pods):
        d = {}
        want = ref.schedule(p, detail=d)
        assert rs[k].as_tuple() == want, f"pod {k}: {rs[k].as_tuple()} != reference {want}"
        assert ds[k].as_dict() == reduce_eval(want[0], d["ev"], 9), f"pod {k}: diagnosis"
        unsched += want[0] == 2
    assert unsched >= 4 and ref.granted >= 4
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 8. what is still refused, and the config ---------------------------------------------------------------------------
def refusal_pods():
    sel = {"matchLabels": {"app": "x"}}
    dns = plain_pod("dns")
    dns["spec"]["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": ZONE,
                                                 "whenUnsatisfiable": "DoNotSchedule", "labelSelector": sel}]
    anti = plain_pod("anti")
    anti["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"topologyKey": HOST, "labelSelector": sel}]}}
    nom_anti = copy.deepcopy(anti)
    nom_anti["metadata"].update(name="hi-anti", uid="hi-anti")
    nom_anti["status"]["nominatedNodeName"] = "n2"
    return dns, anti, plain_pod("plain"), nom_anti


def refused(g, fn, cond):
    with pytest.raises(KsgError) as e:
        fn()
    assert f"rc={KSG_ENOTSUP}" in str(e.value) and cond in str(e.value), str(e.value)


def test_preempt_of_a_marked_pod_is_still_refused(native):
    g = device(native, {}, zoned_nodes(6, 2), [], NAMESPACE, [plain_pod("hi", prio=100, nominated="n1")])
    dns, anti, plain, nom_anti = refusal_pods()
    refused(g, lambda: g.preempt(g.compile(dns), {"offset": 0}), "(a)")
    assert "default/dns" in g.last_error()
    refused(g, lambda: g.preempt(g.compile(anti), {"offset": 0}), "(b)")
    g.add_nominated_pod(nom_anti)
    refused(g, lambda: g.preempt(g.compile(plain), {"offset": 0}), "(c)")
    # the same pods are scheduled
    for p in (dns, anti, plain):
        assert g.schedule_one(g.compile(p))[0].status == 0
    assert g.compare_mirror(sync=True) == (0, -1)


def test_evaluate_still_refuses_the_same_pods(native):
    """"Evaluate" beside "EvaluateAll": the three pods the new value schedules are refused there as before."""
    dns, anti, plain, nom_anti = refusal_pods()
    ga = device(native, {}, zoned_nodes(6, 2), [], NAMESPACE, [plain_pod("hi", prio=100, nominated="n1")])
    ge = native({"nominatedPods": "Evaluate"})
    ge.upsert_namespace(NAMESPACE[0])
    for n in zoned_nodes(6, 2):
        ge.add_node(n)
    ge.add_nominated_pod(plain_pod("hi", prio=100, nominated="n1"))
    refused(ge, lambda: ge.schedule_one(ge.compile(dns)), "(a)")
    refused(ge, lambda: ge.schedule_one(ge.compile(anti)), "(b)")
    refused(ge, lambda: ge.schedule_batch([ge.compile(plain_pod("b0")), ge.compile(anti)]), "(b)")
    for g_ in (ga, ge):
        g_.add_nominated_pod(nom_anti)
    refused(ge, lambda: ge.schedule_one(ge.compile(plain)), "(c)")
    for p in (dns, anti, plain):
        assert ga.schedule_one(ga.compile(p))[0].status == 0
    got = ga.schedule_batch([ga.compile(plain_pod("b0")), ga.compile(plain_pod("b1"))])
    assert [r.status for r in got] == [0, 0]


def test_config_validation(native):
    with pytest.raises(KsgError, match='"Refuse", "Evaluate" or "EvaluateAll"'):
        native({"nominatedPods": "bogus"})
    native(dict(EVALUATE_ALL)).close()
    with pytest.raises(KsgError, match="nominatedPods \"EvaluateAll\".*node-sharded"):
        native({"nominatedPods": "EvaluateAll", "featureGates": {"OpportunisticBatching": False},
                "distributed": {"worldSize": 2, "rank": 0, "localGroup": f"t-{uuid.uuid4().hex[:8]}"}})
