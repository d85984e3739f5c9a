"""ksg_schedule_one_diag / ksg_schedule_batch_diag on the device against tests/diagnosis_reference.py (the oracle
driven pod by pod, each failing cycle's evaluation output reduced in Python): every pod's ksg_result and its whole
ksg_diagnosis, as of the pod's own cycle."""
import copy
import functools
import uuid

import pytest

from diagnosis_reference import (FIT_ERROR, empty, fill, fit_error_text, hand_case, hand_expected, reduce_eval,
                                 reference_stream)
from fuzz_gen import namespaces, rand_cluster, rand_pod
from ksg.abi import KSG_ENOTSUP, PLUGIN_ID, KsgError
from ksg.objects import NodeW, PodW
from nominated_reference import NominatedReference
from oracle_binding import oracle

pytestmark = pytest.mark.gpu

NSS = [{"metadata": {"name": "default"}}]
# the five ways a diagnosed stream runs: the batch call under four loop settings, and the one-pod call
MODES = {
    "unit128": ({"loopUnit": 128}, "batch"),
    "unit256": ({"loopUnit": 256}, "batch"),
    "launch": ({"persistentLoop": False}, "batch"),
    "noagg": ({"aggLoop": False}, "batch"),
    "resident-one": ({"residentLoop": True}, "one"),
}


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def run_diag(g, pods, how):
    """-> [(result tuple, diagnosis dict)] of the stream through the batch call or pod by pod."""
    if how == "batch":
        rs, ds = g.schedule_batch_diag([g.compile(p) for p in pods], assume=True)
        return [(r.as_tuple(), d.as_dict()) for r, d in zip(rs, ds)]
    out = []
    n = g.num_nodes()
    for k, p in enumerate(pods):
        r, ev, d = g.schedule_one_diag(g.compile(p), assume=True, evaluate=k % 2 == 1)
        if ev is not None:  # the diagnosis is the reduction of the arrays the same call returned
            assert d.as_dict() == reduce_eval(r.status, ev, n), f"pod {k}: diagnosis != reduction of its own eval output"
        out.append((r.as_tuple(), d.as_dict()))
    return out


def check(g, got, want, tag=""):
    assert len(got) == len(want)
    for k, ((rg, dg), (ro, do)) in enumerate(zip(got, want)):
        assert rg == ro, f"{tag} pod {k}: result {rg} != reference {ro}"
        assert dg == do, f"{tag} pod {k} (status {ro[0]}): diagnosis\n {dg}\n != reference\n {do}"
        if ro[0] not in FIT_ERROR:  # every counter 0, num_nodes still filled
            assert dg == empty(do["num_nodes"], do["prefilter_code"], do["prefilter_plugin"])
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


def pair(native, cfg, nodes, existing=(), nss=NSS, objects=()):
    ocfg = {k: v for k, v in cfg.items() if k not in ("loopUnit", "persistentLoop", "aggLoop", "residentLoop")}
    return fill(native(dict(cfg, device=0)), nodes, existing, nss, objects), fill(oracle(ocfg), nodes, existing, nss, objects)


# ---- 1. the hand-computed case ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["one", "batch"])
def test_hand_computed_case(native, how):
    nodes, existing, pod = hand_case()
    g = fill(native({"device": 0}), nodes, existing, NSS)
    want_res, want_d, want_text = hand_expected()
    (res, d), = run_diag(g, [pod], how)
    assert res == want_res
    assert d == want_d
    assert fit_error_text(d) == want_text
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 2. random streams ----------------------------------------------------------------------------------------------
CFG_OF = {9: 0, 130: 3, 257: 1, 600: 5}


def random_case(n_nodes):
    """A fuzz_gen stream of 60 pods on a cluster short of room: small clusters get 10-cpu nodes and few bound pods,
    large ones 1-cpu nodes with a 4-cpu node every sixth, so that part of the stream finds no node."""
    rng, cfg, nodes, existing, names = rand_cluster(7300 + n_nodes, n_nodes=n_nodes, n_existing=40 if n_nodes >= 100 else 6,
                                                    cfg_index=CFG_OF[n_nodes])
    for k in range(n_nodes):
        if n_nodes < 100 and k % 3:
            nodes[k]["spec"].pop("taints", None)
            nodes[k]["spec"].pop("unschedulable", None)
        for key in ("allocatable", "capacity"):
            if n_nodes < 100:
                nodes[k]["status"][key].update({"cpu": "10", "memory": "20Gi", "pods": "110"})
            elif k % 6 != 1:
                nodes[k]["status"][key].update({"cpu": "1", "memory": "2Gi"})
            else:
                nodes[k]["status"][key].update({"cpu": "4", "memory": "8Gi", "pods": "110"})
    pods = [rand_pod(rng, k, names) for k in range(60)]
    return cfg, nodes, existing, pods


@functools.lru_cache(maxsize=None)
def random_reference(n_nodes):
    """The case and the reference's outcome per pod, computed once for every mode."""
    cfg, nodes, existing, pods = random_case(n_nodes)
    want = reference_stream(fill(oracle(cfg), nodes, existing, namespaces()), pods)
    failed = sum(r[0] in FIT_ERROR for r, _ in want)
    assert 5 <= failed <= len(pods) // 2, failed  # on the reference alone: no case passes by diagnosing nothing
    assert all(d["failed_nodes"] > 0 for r, d in want if r[0] in FIT_ERROR and not d["prefilter_code"])
    return cfg, nodes, existing, pods, want


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n_nodes", [9, 130, 257, 600])
def test_random_streams_match_reference(native, n_nodes, mode):
    cfg, nodes, existing, pods, want = random_reference(n_nodes)
    extra, how = MODES[mode]
    g = fill(native(dict(cfg, device=0, **extra)), nodes, existing, namespaces())
    check(g, run_diag(g, pods, how), want, f"{n_nodes} nodes, {mode}:")


@pytest.mark.parametrize("n_nodes", [9, 130, 257, 600])
def test_diagnosed_and_plain_batches_agree(native, n_nodes):
    """Two identical contexts: ksg_schedule_batch_diag returns what ksg_schedule_batch returns."""
    cfg, nodes, existing, pods, want = random_reference(n_nodes)
    a = fill(native(dict(cfg, device=0)), nodes, existing, namespaces())
    b = fill(native(dict(cfg, device=0)), nodes, existing, namespaces())
    plain = [r.as_tuple() for r in a.schedule_batch([a.compile(p) for p in pods], assume=True)]
    diag = [r for r, _ in run_diag(b, pods, "batch")]
    assert plain == diag == [r for r, _ in want]
    assert a.compare_mirror(sync=True) == (0, -1) and b.compare_mirror(sync=True) == (0, -1)


# ---- 3. placements within a run -------------------------------------------------------------------------------------
def box(name, cpu="4", mem="8Gi", pods="20", taint=False, labels=None):
    w = NodeW(name).capacity({"cpu": cpu, "memory": mem, "pods": pods}).label("kubernetes.io/hostname", name)
    for k, v in (labels or {}).items():
        w.label(k, v)
    if taint:
        w.taints([{"key": "dedicated", "value": "x", "effect": "NoSchedule"}])
    return w.obj()


def ask(name, cpu, mem="100Mi"):
    return PodW(name).container(image="i", requests={"cpu": cpu, "memory": mem})


TWO_BOXES = [box("u0"), box("u1"), box("t0", taint=True)]


def in_loop(g, mode):
    """Node-local pods of a diagnosed batch stay in k_sched_loop (its diagnosing instances reduce in the loop)."""
    if MODES[mode][1] == "batch":
        assert g.kernel_stats()[3] == ("k_filter_score" if mode == "launch" else "k_sched_loop")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_failing_pods_at_every_place_of_a_run(native, mode):
    """A failing pod first, two in a row, one between pods that land on the nodes which then turn it away in a
    different way, and one last.  `mid` and `late` are the same pod: at mid's cycle u0 and u1 are short of cpu only;
    by late's, the pods after mid have taken their memory too."""
    pods = [ask("first", "5").obj(),                       # fails first in the run: more cpu than any node has
            ask("a", "3").obj(), ask("b", "3").obj(),      # one on each box
            ask("mid", "2", "5Gi").obj(),                  # cpu on u0 and u1
            ask("mid2", "2", "5Gi").obj(),                 # two failing pods in a row
            ask("c", "500m", "6Gi").obj(), ask("d", "500m", "6Gi").obj(),  # land where mid was turned away
            ask("late", "2", "5Gi").obj()]                 # cpu and memory now; last in the run
    extra, how = MODES[mode]
    g, o = pair(native, extra, TWO_BOXES)
    want = reference_stream(o, pods)
    assert [r[0] for r, _ in want] == [2, 0, 0, 2, 2, 0, 0, 2]
    cpu, mem = 7, 8
    assert want[3][1]["reason_nodes"][cpu] == 2 and want[3][1]["reason_nodes"][mem] == 0
    assert want[7][1]["reason_nodes"][cpu] == 2 and want[7][1]["reason_nodes"][mem] == 2  # the as-of-its-own-cycle state
    assert want[0][1]["unresolvable_nodes"] == 3 and want[3][1]["unresolvable_nodes"] == 1
    check(g, run_diag(g, pods, how), want, mode)
    in_loop(g, mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_pod_of_the_batch_fails(native, mode):
    pods = [ask(f"f{k}", "5" if k % 2 else "4500m", "9Gi" if k % 3 == 0 else "1Gi").obj() for k in range(12)]
    extra, how = MODES[mode]
    g, o = pair(native, extra, TWO_BOXES)
    want = reference_stream(o, pods)
    assert all(r == (2, -1, 3, 0, 0) for r, _ in want)
    check(g, run_diag(g, pods, how), want, mode)
    in_loop(g, mode)


# ---- 4. pod classes ---------------------------------------------------------------------------------------------------
def zoned():
    """za0, za1 in zone a, zb0 (tainted) in zone b; two app=web pods and one app=db pod bound in zone a."""
    nodes = [box("za0", labels={"topology.kubernetes.io/zone": "a"}), box("za1", labels={"topology.kubernetes.io/zone": "a"}),
             box("zb0", taint=True, labels={"topology.kubernetes.io/zone": "b"})]
    existing = [PodW("w0").label("app", "web").container(image="i", requests={"cpu": "100m"}).node("za0").obj(),
                PodW("w1").label("app", "web").container(image="i", requests={"cpu": "100m"}).node("za0").obj(),
                PodW("db0").label("app", "db").container(image="i", requests={"cpu": "100m"}).node("za0").obj(),
                PodW("db1").label("app", "db").container(image="i", requests={"cpu": "100m"}).node("za1").obj()]
    return nodes, existing


@pytest.mark.parametrize("mode", sorted(MODES))
def test_spread_and_anti_affinity_pods_that_fail(native, mode):
    """k_agg_loop's class: a DoNotSchedule spread pod whose only untainted zone is too full, and a pod with a required
    anti-affinity term against a pod on every untainted node, among pods of the same class that do land."""
    nodes, existing = zoned()
    web = {"matchLabels": {"app": "web"}}
    spread = lambda name, skew: PodW(name).label("app", "web").container(image="i", requests={"cpu": "100m"}) \
        .spread(skew, "topology.kubernetes.io/zone", "DoNotSchedule", web).obj()
    anti = lambda name, app: PodW(name).label("app", "x").container(image="i", requests={"cpu": "100m"}) \
        .pod_affinity("kubernetes.io/hostname", {"matchLabels": {"app": app}}, anti=True).obj()
    pods = [spread("s-ok", 5), spread("s-fail", 1), anti("a-fail", "db"), anti("a-ok", "nothing"), spread("s-fail2", 2),
            anti("a-fail2", "db")]
    extra, how = MODES[mode]
    g, o = pair(native, extra, nodes, existing)
    want = reference_stream(o, pods)
    assert [r[0] for r, _ in want] == [0, 2, 2, 0, 2, 2]
    pts, ipa = PLUGIN_ID["PodTopologySpread"], PLUGIN_ID["InterPodAffinity"]
    assert want[1][1]["plugin_nodes"][pts] == 2 and want[1][1]["reason_nodes"][12] == 2
    assert want[2][1]["plugin_nodes"][ipa] == 2 and want[2][1]["reason_nodes"][14] == 2
    check(g, run_diag(g, pods, how), want, mode)


@pytest.mark.parametrize("how", ["batch", "one"])
def test_prefilter_rejection_and_matchfields_subset(native, how):
    """An empty PreFilterResult (matchFields naming no node: every node is outside it), a PreFilter rejection (two
    matchFields that exclude each other: every node carries NodeAffinity's PreFilter status), a PreFilterResult subset
    whose nodes are full (the nodes outside it carry no plugin: failed, unresolvable, in the PreFilter bin, no plugin
    bit), and a pod whose own nominated node fails alone and then everything else does too (that node counts once)."""
    field = lambda names: [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": names}]}]
    nowhere = ask("nowhere", "1").node_affinity_required(field(["no-such-node"])).obj()
    reject = ask("reject", "1").node_affinity_required([{"matchFields": field(["u0"])[0]["matchFields"] +
                                                         field(["u1"])[0]["matchFields"]}]).obj()
    subset = ask("subset", "3").node_affinity_required(field(["u0", "t0"])).obj()
    own = ask("own", "3").obj()
    own["status"] = {"nominatedNodeName": "u1"}
    pods = [ask("a", "3").obj(), ask("b", "3").obj(), nowhere, reject, subset, own, ask("fits", "1").obj()]
    g, o = pair(native, {}, TWO_BOXES)
    want = reference_stream(o, pods)
    assert [r[0] for r, _ in want] == [0, 0, 2, 2, 2, 2, 0]
    assert want[2][1]["unschedulable_plugins"] == 0 and want[2][1]["reason_nodes"][16] == 3
    na = PLUGIN_ID["NodeAffinity"]
    assert (want[3][1]["prefilter_code"], want[3][1]["prefilter_plugin"], want[3][1]["plugin_nodes"][na]) == (3, na, 3)
    sub = want[4][1]
    assert sub["failed_nodes"] == 3 and sub["reason_nodes"][16] == 1 and sum(sub["plugin_nodes"]) == 2
    assert want[5][1]["failed_nodes"] == 3  # u1 once
    check(g, run_diag(g, pods, how), want, how)


def test_sampled_profile_with_no_feasible_node(native):
    """percentageOfNodesToScore 10 on 130 nodes: the sampled pass stops at 100 feasible nodes, but a pod with none has
    evaluated every node, so its row covers all 130."""
    nodes = [box(f"n{k:03d}", cpu="2", taint=k % 13 == 0) for k in range(130)]
    pods = [ask(f"p{k}", "1").obj() for k in range(6)] + [ask("big", "3").obj(), ask("p6", "2").obj(),
                                                          ask("big2", "2500m", "9Gi").obj()]
    g, o = pair(native, {"percentageOfNodesToScore": 10}, nodes)
    want = reference_stream(o, pods)
    assert [r[0] for r, _ in want] == [0] * 6 + [2, 0, 2]
    assert want[0][0][3] == 100 and want[6][1]["failed_nodes"] == 130 and want[6][1]["num_nodes"] == 130
    check(g, run_diag(g, pods, "batch"), want)
    g2 = fill(native({"percentageOfNodesToScore": 10, "device": 0}), nodes, (), NSS)
    check(g2, run_diag(g2, pods, "one"), want)


def test_stream_under_nominations(native):
    """{"nominatedPods": "Evaluate"}: the diagnosis carries the with-nominees status.  Four of six nodes hold a
    priority-100 nomination of 3500m; once the two free nodes are taken, a priority-0 pod of 1 cpu fails on all six
    with Insufficient cpu -- four of them only because of the nominations -- while a priority-200 pod still lands."""
    nodes = [box(f"n{k}") for k in range(6)]
    nom = lambda k: {"metadata": {"name": f"nom{k}", "namespace": "default", "uid": f"nom{k}"},
                     "spec": {"priority": 100, "containers": [{"name": "c", "image": "i",
                                                               "resources": {"requests": {"cpu": "3500m"}}}]},
                     "status": {"nominatedNodeName": f"n{k}"}}
    def prio(p, v):
        p["spec"]["priority"] = v
        return p
    pods = [prio(ask("l0", "3500m").obj(), 0), prio(ask("l1", "3500m").obj(), 0), prio(ask("low", "1").obj(), 0),
            prio(ask("top", "1").obj(), 200), prio(ask("low2", "1").obj(), 50), copy.deepcopy(nom(2)),
            prio(ask("low3", "1").obj(), 0)]
    for how in ("batch", "one"):
        g = fill(native({"nominatedPods": "Evaluate", "device": 0}), nodes, (), NSS)
        ref = NominatedReference({}, nodes, [], NSS)
        for k in range(4):
            g.add_nominated_pod(nom(k))
            ref.add_nominated_pod(nom(k))
        want = []
        for p in pods:
            d = {}
            t = ref.schedule(p, detail=d)
            want.append((t, reduce_eval(t[0], d["ev"], 6)))
        assert [t[0] for t, _ in want] == [0, 0, 2, 0, 2, 0, 2]
        assert want[2][1]["reason_nodes"][7] == 6 and ref.flips >= 4
        check(g, run_diag(g, pods, how), want, how)


# ---- 5. what is refused -----------------------------------------------------------------------------------------------
def test_sharded_context_refuses_both_calls(native):
    name = f"diag-{uuid.uuid4().hex[:8]}"
    ranks = [native({"device": 0, "featureGates": {"OpportunisticBatching": False},
                     "distributed": {"worldSize": 2, "rank": r, "localGroup": name}}) for r in range(2)]
    for s in ranks:
        fill(s, TWO_BOXES, (), NSS)
    s = ranks[0]
    h = s.compile(ask("p", "1").obj())
    for call in (lambda: s.schedule_one_diag(h), lambda: s.schedule_batch_diag([h])):
        with pytest.raises(KsgError, match=f"rc={KSG_ENOTSUP}"):
            call()
    for s in ranks:
        s.close()
