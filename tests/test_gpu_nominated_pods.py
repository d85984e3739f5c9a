"""Filtering with other pods' nominations on the device ({"nominatedPods": "Evaluate"}) against
tests/nominated_reference.py, pod by pod: RunFilterPluginsWithNominatedPods (framework.go:1211-1294) adds the pods
nominated to a node of equal or higher priority before filtering it; scores never see them.  The device does it in
one pass (the filters on the node's core plus those pods, the scores on the core as it is); the reference does the
literal two passes, so these tests check that shortcut on every path a node is filtered on: the launch path with
evaluation output, both persistent loops (batch and resident ring), the pod's own nominated node, the sampled pass
and DefaultPreemption's dry run."""
import copy
import functools
import random

import pytest

from fuzz_gen import namespaces, rand_cluster, rand_pod
from ksg.abi import KSG_ENOTSUP, PLUGIN_ID, KsgError
from nominated_reference import NominatedReference, eval_fields
from nominator_scenario import node as plain_node, pod as plain_pod

pytestmark = pytest.mark.gpu

EVALUATE = {"nominatedPods": "Evaluate"}
R_INSUFFICIENT_CPU = 1 << 7


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def device(native, cfg, nodes, existing, nss=(), objects=()):
    g = native(dict(cfg, **EVALUATE))
    for ns in nss:
        g.upsert_namespace(ns)
    for o in objects:
        g.upsert_object(o)
    for n in nodes:
        g.add_node(n)
    for p in existing:
        g.add_pod(p)
    return g


def nominate(pod, node):
    pod = copy.deepcopy(pod)
    pod["status"] = dict(pod.get("status") or {}, nominatedNodeName=node)
    return pod


def nominee(name, prio, node, cpu="1", mem="1Gi", port=None, gpu=None, ns="default"):
    req = {"cpu": cpu, "memory": mem}
    if gpu:
        req["example.com/gpu"] = str(gpu)
    c = {"name": "c", "image": "i", "resources": {"requests": req}}
    if port:
        c["ports"] = [{"containerPort": 8080, "hostPort": port, "protocol": "TCP"}]
    return {"metadata": {"name": name, "namespace": ns, "uid": name, "labels": {"app": "nominee"}},
            "spec": {"priority": prio, "containers": [c]}, "status": {"nominatedNodeName": node}}


def check_eval(eg, d, n, tag):
    code, plug, reas, mask, norm, total = eval_fields(d, n)
    assert eg["node_code"] == code, f"{tag}: node_code"
    assert eg["node_plugin"] == plug, f"{tag}: node_plugin"
    assert eg["node_reasons"] == reas, f"{tag}: node_reasons"
    if len(d["feasible"]) > 1:  # scored
        w = d["weights"]
        assert eg["score_plugin_mask"] == mask, f"{tag}: score mask {eg['score_plugin_mask']:#x} != {mask:#x}"
        for p in range(len(norm)):
            for i in d["feasible"]:
                assert eg["normalized_scores"][p][i] == norm[p][i], f"{tag}: normalized score, plugin {p} node {i}"
                assert eg["plugin_scores"][p][i] == norm[p][i] * w.get(p, 0) * (mask >> p & 1), \
                    f"{tag}: plugin score, plugin {p} node {i}"
        for i in d["feasible"]:
            assert eg["total_scores"][i] == total[i], f"{tag}: total score, node {i}"


# ---- 1. the hand-computed case --------------------------------------------------------------------------------
def test_hand_computed_case_on_the_device(native):
    nodes = [plain_node(f"n{k}") for k in range(4)]
    nss = [{"metadata": {"name": "default"}}]
    g = device(native, {}, nodes, [], nss)
    ref = NominatedReference({}, nodes, [], nss)
    n1 = ref.index["n1"]
    hi = plain_pod("hi", prio=100, cpu="3500m", nominated="n1")
    g.add_nominated_pod(hi)
    ref.add_nominated_pod(hi)

    def one(p, assume, tag):
        d = {}
        want = ref.schedule(p, assume=assume, detail=d)
        d["weights"] = ref.weights
        rg, eg = g.schedule_one(g.compile(p), assume=assume, evaluate=True)
        assert rg.as_tuple() == want, (tag, rg.as_tuple(), want)
        if d["feasible"]:
            check_eval(eg, d, 4, tag)
        return rg, eg

    r, e = one(plain_pod("low", prio=0, cpu="1"), False, "priority 0 under a priority-100 nomination")
    assert (e["node_code"][n1], e["node_plugin"][n1], e["node_reasons"][n1]) == \
        (2, PLUGIN_ID["NodeResourcesFit"], R_INSUFFICIENT_CPU)
    assert r.feasible_nodes == 3
    # (an evaluation without an assume is a cycle too: both sides moved nextStartNodeIndex alike)
    r, e = one(plain_pod("top", prio=200, cpu="1"), False, "priority 200: the nomination is not added")
    assert r.feasible_nodes == 4 and e["node_code"][n1] == 0
    r, _ = one(hi, True, "the nominated pod itself")
    assert r.as_tuple() == (0, n1, 1, 1, 0)
    r, e = one(plain_pod("low2", prio=0, cpu="1"), False, "the 3500m are on n1 for real")
    assert r.feasible_nodes == 3 and e["node_reasons"][n1] == R_INSUFFICIENT_CPU
    r, e = one(plain_pod("tiny", prio=0, cpu="500m"), False, "what is left of n1")
    assert r.feasible_nodes == 4
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 2. random streams ------------------------------------------------------------------------------------------
CFG_OF = {9: 0, 130: 3, 257: 1, 600: 5}


def random_case(n_nodes):
    rng, cfg, nodes, existing, names = rand_cluster(9100 + n_nodes, n_nodes=n_nodes, n_existing=60,
                                                    cfg_index=CFG_OF[n_nodes])
    for k in range(n_nodes):
        for key in ("allocatable", "capacity"):
            if n_nodes < 100:  # one wave of roomy nodes, so that the stream is not over when they are full
                nodes[k]["status"][key].update({"cpu": "8", "memory": "32Gi", "pods": "110"})
            if k % 7 == 0:  # a few nodes where the pod count decides
                nodes[k]["status"][key]["pods"] = "3"
    return rng, cfg, nodes, existing, names


def random_nominees(rng, order):
    """6 to 10 nominees of priorities {0, 50, 100}: on snapshot index 0 (two of them), 255, 256, the last index, a
    name outside the snapshot and random nodes; some with a host port the stream asks for, some with a gpu."""
    n = len(order)
    where = [0, 0, 255, 256, n - 1, -1] + [rng.randrange(n) for _ in range(rng.randint(0, 4))]
    out = []
    for k, ix in enumerate(where):
        if ix >= n:
            ix = rng.randrange(n)
        out.append(nominee(f"nom{k}", rng.choice([0, 50, 100]), order[ix] if ix >= 0 else "no-such-node",
                           cpu=rng.choice(["5", "6", "7"] if n < 100 else ["500m", "1", "2", "3"]), mem=rng.choice(["512Mi", "2Gi", "6Gi"]),
                           port=80 if k % 3 == 0 else None, gpu=1 if k % 4 == 1 else None))
    out[0]["spec"]["priority"], out[1]["spec"]["priority"] = 100, 50  # index 0: two records, one above the other
    return out


def random_stream(rng, names, noms):
    pods = []
    for k in range(80):
        p = rand_pod(rng, k, names, topology=False)
        p["spec"]["priority"] = rng.choice([0, 50, 100])
        if k % 9 == 4:
            p["spec"]["containers"][0]["ports"] = [{"containerPort": 8080, "hostPort": 80, "protocol": "TCP"}]
        if k % 11 == 5:
            p["spec"]["containers"][0].setdefault("resources", {}).setdefault("requests", {})["example.com/gpu"] = "1"
        pods.append(p)
    # the nominees' own cycles, inside the stream: index 0's lower one while the upper is still nominated there,
    # then one on a random node
    pods.insert(30, copy.deepcopy(noms[1]))
    pods.insert(55, copy.deepcopy(noms[-1]))
    return pods


@functools.lru_cache(maxsize=None)
def random_reference(n_nodes):
    """The case and the reference's outcome per pod, computed once for the three modes."""
    rng, cfg, nodes, existing, names = random_case(n_nodes)
    ref = NominatedReference(cfg, nodes, existing, namespaces())
    noms = random_nominees(rng, ref.names)
    for q in noms:
        ref.add_nominated_pod(q)
    pods = random_stream(rng, names, noms)
    want = []
    for p in pods:
        d = {}
        t = ref.schedule(p, detail=d)
        d["weights"] = ref.weights
        want.append((t, d))
    assert sum(t[0] == 0 for t, _ in want) > 10 and ref.flips > 10  # the nominations do decide node statuses
    return cfg, nodes, existing, noms, pods, want


@pytest.mark.parametrize("mode", ["batch", "calls", "eval"])
@pytest.mark.parametrize("n_nodes", [9, 130, 257, 600])
def test_random_streams_match_reference(native, n_nodes, mode):
    cfg, nodes, existing, noms, pods, want = random_reference(n_nodes)
    g = device(native, cfg, nodes, existing, namespaces())
    for q in noms:
        g.add_nominated_pod(q)
    if mode == "batch":
        got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
        for k in range(len(pods)):
            assert got[k] == want[k][0], f"pod {k}: {got[k]} != reference {want[k][0]}"
    else:
        for k, p in enumerate(pods):
            rg, eg = g.schedule_one(g.compile(p), assume=True, evaluate=mode == "eval")
            assert rg.as_tuple() == want[k][0], f"pod {k}: {rg.as_tuple()} != reference {want[k][0]}"
            if eg is not None and want[k][1]["feasible"]:  # (not the pod's own nominated node tried alone)
                check_eval(eg, want[k][1], n_nodes, f"pod {k}")
    assert g.compare_mirror(sync=True) == (0, -1)  # the overlay leaked nothing into the mirror
    assert g.loop_stats() == (0, 0)


# ---- 3. batch order -----------------------------------------------------------------------------------------------
def test_batch_holding_the_nominees_themselves(native):
    """One batch with two nominated pods among plain ones: the pods before each see its nomination, the pods after
    it see it placed for real (A, on its nominated node) or gone (B, whose nominated node A's nomination fills)."""
    nodes = [plain_node(f"n{k}") for k in range(8)]
    nss = [{"metadata": {"name": "default"}}]
    g = device(native, {}, nodes, [], nss)
    ref = NominatedReference({}, nodes, [], nss)
    a = plain_pod("A", prio=100, cpu="3000m", nominated="n1")
    b = plain_pod("B", prio=50, cpu="2000m", nominated="n1")
    for b_ in (g, ref):
        b_.add_nominated_pod(a)
        b_.add_nominated_pod(b)
    pods = ([plain_pod(f"p{k}", prio=0, cpu="1") for k in range(5)] + [b] +
            [plain_pod(f"p{k}", prio=60, cpu="1500m") for k in range(5, 10)] + [a] +
            [plain_pod(f"p{k}", prio=0, cpu="1") for k in range(10, 15)])
    got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    n1 = ref.index["n1"]
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k} ({p['metadata']['name']}): {got[k]} != reference {want}"
    assert got[5][0] == 0 and got[5][1] != n1     # B: n1 failed alone under A's nomination, the full pass placed it
    assert got[11] == (0, n1, 1, 1, 0)            # A: its nominated node alone
    assert all(t[1] != n1 for t in got[:11])      # before A: n1 holds 5000m, then 3000m, of nominations
    assert g.compare_mirror(sync=True) == (0, -1)


def test_batch_under_a_nomination_stays_in_the_loop(native):
    """256 plain pods in one batch while a pod outside it holds a nomination: k_sched_loop runs them."""
    nodes = [plain_node(f"n{k:03d}") for k in range(200)]
    nss = [{"metadata": {"name": "default"}}]
    g = device(native, {}, nodes, [], nss)
    ref = NominatedReference({}, nodes, [], nss)
    held = plain_pod("held", prio=0, cpu="3800m", nominated="n017")
    g.add_nominated_pod(held)
    ref.add_nominated_pod(held)
    pods = [plain_pod(f"p{k}", prio=0, cpu="500m") for k in range(256)]
    got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    assert g.kernel_stats()[3] == "k_sched_loop"
    n17 = ref.index["n017"]
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k}: {got[k]} != reference {want}"
    assert all(t[1] != n17 and t[3] == 199 for t in got)
    assert g.loop_stats() == (0, 0)


# ---- 4. k_agg_loop's class ------------------------------------------------------------------------------------
def test_agg_loop_class(native):
    """300 nodes in 3 zones; a Service selects the pods, so the System default constraints score them; every
    third pod carries a ScheduleAnyway constraint and a preferred anti-affinity term of its own instead."""
    from ksg.synth import default_topology_spreading
    nodes, init, pods, objects = default_topology_spreading(300, 300, 260)
    for k, p in enumerate(pods):
        p["spec"]["containers"][0]["resources"] = {"requests": {"cpu": "500m", "memory": "1Gi"}}
        if k % 3 == 2:
            p["spec"]["topologySpreadConstraints"] = [{
                "maxSkew": 2, "topologyKey": "topology.kubernetes.io/zone", "whenUnsatisfiable": "ScheduleAnyway",
                "labelSelector": {"matchLabels": {"app": "scheduler-perf"}}}]
            p["spec"]["affinity"] = {"podAntiAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [{
                "weight": 10, "podAffinityTerm": {"topologyKey": "kubernetes.io/hostname",
                                                   "labelSelector": {"matchLabels": {"app": "scheduler-perf"}}}}]}}
    g = device(native, {}, nodes, init, namespaces(), objects)
    ref = NominatedReference({}, nodes, init, namespaces(), objects)
    rng = random.Random(4)
    for k in range(8):  # nominations that leave no room for a 500m pod on their nodes
        q = nominee(f"nom{k}", rng.choice([0, 100]), ref.names[[0, 255, 256, 299, 7, 100, 150, 290][k]], cpu="3700m",
                    ns="service-ns")
        g.add_nominated_pod(q)
        ref.add_nominated_pod(q)
    got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    assert g.kernel_stats()[3] == "k_agg_loop"
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k}: {got[k]} != reference {want}"
    assert all(t[0] == 0 and t[3] < 300 for t in got)
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


# ---- 5. what is still refused -----------------------------------------------------------------------------------
def test_remaining_refusal(native):
    nodes = [plain_node(f"n{k}") for k in range(6)]
    for k, n in enumerate(nodes):
        n["metadata"]["labels"]["topology.kubernetes.io/zone"] = f"z{k % 2}"
    nss = [{"metadata": {"name": "default"}}]
    g = device(native, {}, nodes, [], nss)
    sel = {"matchLabels": {"app": "x"}}
    dns = plain_pod("dns")
    dns["spec"]["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": "topology.kubernetes.io/zone",
                                                 "whenUnsatisfiable": "DoNotSchedule", "labelSelector": sel}]
    anti = plain_pod("anti")
    anti["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"topologyKey": "kubernetes.io/hostname", "labelSelector": sel}]}}
    plain = plain_pod("plain")

    def refused(fn, cond):
        with pytest.raises(KsgError) as e:
            fn()
        assert f"rc={KSG_ENOTSUP}" in str(e.value) and cond in str(e.value), str(e.value)

    g.add_nominated_pod(plain_pod("hi", prio=100, nominated="n1"))
    refused(lambda: g.schedule_one(g.compile(dns)), "(a)")
    assert "default/dns" in g.last_error()
    refused(lambda: g.schedule_one(g.compile(anti)), "(b)")
    assert "default/anti" in g.last_error()
    refused(lambda: g.schedule_batch([g.compile(plain_pod("b0")), g.compile(anti)]), "(b)")  # the whole batch
    nom_anti = copy.deepcopy(anti)
    nom_anti["metadata"].update(name="hi-anti", uid="hi-anti")
    g.add_nominated_pod(nominate(nom_anti, "n2"))
    refused(lambda: g.schedule_one(g.compile(plain)), "(c)")
    assert "default/plain" in g.last_error()
    refused(lambda: g.preempt(g.compile(plain), {"offset": 0}), "(c)")
    g.delete_nominated_pod("hi-anti")
    # nothing was scheduled, and the next plain call on the same context succeeds, under the nomination
    r = g.schedule_one(g.compile(plain))[0]
    assert r.as_tuple()[0] == 0 and r.feasible_nodes == 6 and r.evaluated_nodes == 6
    assert g.compare_mirror(sync=True) == (0, -1)
    # the same pods with no nomination of equal or higher priority present are scheduled normally
    hi_dns, hi_anti = copy.deepcopy(dns), copy.deepcopy(anti)
    hi_dns["spec"]["priority"] = hi_anti["spec"]["priority"] = 200
    assert g.schedule_one(g.compile(hi_dns))[0].status == 0
    assert g.schedule_one(g.compile(hi_anti))[0].status == 0
    g.delete_nominated_pod("hi")
    assert g.schedule_one(g.compile(dns))[0].status == 0
    assert g.schedule_one(g.compile(anti))[0].status == 0


# ---- 6. preemption under nominations ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_preemption_under_nominations(native, seed):
    from test_gpu_preempt import cluster, mk_pod, pdbs
    rng, nodes, existing = cluster(300 + seed, 40 + 20 * seed, 6)
    nss = [{"metadata": {"name": "default"}}, {"metadata": {"name": "team"}}]
    g = device(native, {}, nodes, existing, nss)
    ref = NominatedReference({}, nodes, existing, nss)
    for k in range(10):  # nominees above, at and below the preemptors' priority (500)
        q = nominee(f"nom{k}", [1000, 500, 100][k % 3], rng.choice(ref.names), cpu=rng.choice(["500m", "1500m"]),
                    port=8080 if k % 4 == 0 else None, gpu=1 if k % 5 == 1 else None)
        g.add_nominated_pod(q)
        ref.add_nominated_pod(q)
    found = 0
    for q in range(8):
        pod = mk_pod(f"pre{q}", rng, prio=500, big=True)
        args = {"offset": rng.randrange(1000), "now": 1704067200 * 10 ** 9 + rng.randrange(3600) * 10 ** 9,
                "pdbs": pdbs(rng), "allNodes": rng.random() < 0.3, "listCandidates": True,
                "minCandidateNodesPercentage": rng.choice([10, 40, 100]), "minCandidateNodesAbsolute": rng.choice([1, 3, 100])}
        want, dwant = ref.preempt(pod, args)
        for extra in ({}, {"debugHostStaged": True}, {"debugWideDryRun": True},
                      {"debugHostStaged": True, "debugWideDryRun": True}):
            r, d = g.preempt(g.compile(pod), dict(args, **extra))
            assert r.as_tuple() == want, (q, extra, r.as_tuple(), want)
            assert d == dwant, (q, extra)
        found += want[0] == 0
    assert found > 0


# ---- 7. a PreemptionBasic-shaped stream ---------------------------------------------------------------------------
def test_preemption_basic_stream(native):
    """40 nodes filled by low-priority pods, then high-priority pods: each failed cycle is ksg_preempt, the victims
    removed, the pod nominated, other pods scheduled while nominations are outstanding, then the nominee's own
    cycle.  No call is refused and every step equals the reference."""
    nodes = [plain_node(f"n{k:02d}") for k in range(40)]
    nss = [{"metadata": {"name": "default"}}]
    low = []
    for k in range(40):
        for j in range(4):
            p = plain_pod(f"low-{k}-{j}", prio=0, cpu="900m")
            p["spec"]["nodeName"] = f"n{k:02d}"
            p["status"]["startTime"] = f"2024-01-01T00:{k:02d}:{j:02d}Z"
            low.append(p)
    g = device(native, {}, nodes, low, nss)
    ref = NominatedReference({}, nodes, low, nss)
    pending, most = [], 0

    def cycle(p, tag):
        want = ref.schedule(p)
        got = g.schedule_one(g.compile(p), assume=True)[0].as_tuple()
        assert got == want, (tag, got, want)
        return got

    for q in range(6):
        hi = plain_pod(f"hi{q}", prio=100, cpu="2")
        assert cycle(hi, f"hi{q}")[0] == 2  # the cluster is full
        args = {"offset": q, "now": 1704067200 * 10 ** 9, "listCandidates": True}
        want, dwant = ref.preempt(hi, args)
        r, d = g.preempt(g.compile(hi), args)
        assert r.as_tuple() == want and d == dwant, q
        assert want[0] == 0
        for uid in d["victims"]:
            g.remove_pod(uid)
            ref.remove_pod(uid)
        hi = nominate(hi, d["selected"])
        g.add_nominated_pod(hi)
        ref.add_nominated_pod(hi)
        pending.append(hi)
        most = max(most, len(ref.nominator))
        # other pods while the nominations are outstanding: the room the victims left is spoken for
        for j in range(3):
            cycle(plain_pod(f"other{q}-{j}", prio=0, cpu="300m"), f"other{q}-{j}")
        got = [t.as_tuple() for t in g.schedule_batch([g.compile(plain_pod(f"ob{q}-{j}", prio=100, cpu="300m"))
                                                       for j in range(2)], assume=True)]
        for j in range(2):
            assert got[j] == ref.schedule(plain_pod(f"ob{q}-{j}", prio=100, cpu="300m")), (q, j)
        if q % 2:  # the nominees' own cycles, two at a time
            for p in pending:
                t = cycle(p, p["metadata"]["name"])
                assert t[0] == 0 and t[2:] == (1, 1, 0), t
            pending = []
    assert most >= 2  # at least two nominations were outstanding at once
    assert not ref.nominator
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


# ---- 8. sampling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "calls"])
def test_sampled_pass(native, mode):
    """percentageOfNodesToScore 40 on 300 nodes: numFeasibleNodesToFind is 120, more than 120 nodes fit every pod,
    and the nominations sit inside the first rotation window."""
    nodes = [plain_node(f"n{k:03d}") for k in range(300)]
    nss = [{"metadata": {"name": "default"}}]
    cfg = {"percentageOfNodesToScore": 40}
    g = device(native, cfg, nodes, [], nss)
    ref = NominatedReference(cfg, nodes, [], nss)
    for k, ix in enumerate([0, 3, 17, 64, 100, 119]):
        q = nominee(f"nom{k}", [100, 0][k % 2], ref.names[ix], cpu="3800m")
        g.add_nominated_pod(q)
        ref.add_nominated_pod(q)
    pods = [plain_pod(f"p{k}", prio=[0, 100][k % 2], cpu="500m") for k in range(40)]
    if mode == "batch":
        got = [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
    else:
        got = [g.schedule_one(g.compile(p), assume=True)[0].as_tuple() for p in pods]
    for k, p in enumerate(pods):
        want = ref.schedule(p)
        assert got[k] == want, f"pod {k}: {got[k]} != reference {want}"
        assert want[3] == 120
    assert got[0][2] > 120  # the first window held nominated nodes the priority-0 pod could not take
    assert g.compare_mirror(sync=True) == (0, -1)


# ---- 9. config validation -----------------------------------------------------------------------------------------
def test_config_validation(native):
    import uuid
    with pytest.raises(KsgError, match="nominatedPods"):
        native({"nominatedPods": "bogus"})
    native({"nominatedPods": "Refuse"}).close()
    with pytest.raises(KsgError, match="nominatedPods.*node-sharded"):
        native({"nominatedPods": "Evaluate", "featureGates": {"OpportunisticBatching": False},
                "distributed": {"worldSize": 2, "rank": 0, "localGroup": f"t-{uuid.uuid4().hex[:8]}"}})
