"""ksg_schedule_batch_diag for k_agg_loop's pod classes (PodTopologySpread / InterPodAffinity pods): the diagnosing
instances of the loop reduce a failing pod's statuses inside the loop, so these pods stay in
k_agg_loop in a diagnosed batch.  Reference: tests/diagnosis_reference.py (the oracle pod by pod, each failing cycle's
evaluation output reduced in Python).

These are the first tests that compare the plugin, code and reason bits of a failing status computed inside
k_agg_loop with anything: the loop itself only ever consumed "feasible or not".

Every case is a batch of more than one pod through schedule_batch_diag; where every pod of the batch is of the
loop's class the case asserts that the loop ran all of them.  The conditions on the inputs (enough FitErrors of the
class, a PodTopologySpread bin, an InterPodAffinity bin) are asserted on the reference alone, before the device is
touched."""
import copy
import functools

import pytest

from diagnosis_reference import FIT_ERROR, empty, fill, reduce_eval, reference_stream
from fuzz_gen import APPS, namespaces, rand_cluster, rand_pod
from ksg.abi import PLUGIN_ID
from ksg.objects import NodeW, PodW
from nominated_reference import NominatedReference
from oracle_binding import oracle

pytestmark = pytest.mark.gpu

HOST, ZONE = "kubernetes.io/hostname", "topology.kubernetes.io/zone"
NSS = [{"metadata": {"name": "default"}}]
PTS, IPA = PLUGIN_ID["PodTopologySpread"], PLUGIN_ID["InterPodAffinity"]
# KSG_R_* bit numbers (ksg.h; ksg.abi.REASONS in the same order)
(R_UNSCHED, R_NODENAME, R_TAINT, R_NA, R_NA_ENF, R_PORTS, R_TOO_MANY, R_CPU, R_MEM, R_EPH, R_SCALAR, R_PTS_LABEL,
 R_PTS_SKEW, R_IPA_AFF, R_IPA_ANTI, R_IPA_EXIST, R_PREFILTER) = range(17)
LOOP_KEYS = ("loopUnit", "persistentLoop", "aggLoop", "aggLoopDebug", "loopWorkgroups", "pipelineFirstChunk")


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def run_diag(g, pods):
    rs, ds = g.schedule_batch_diag([g.compile(p) for p in pods], assume=True)
    return [(r.as_tuple(), d.as_dict()) for r, d in zip(rs, ds)]


def check(g, got, want, tag=""):
    """tests/test_gpu_diagnosis.py's check(): every pod's result and whole diagnosis, empty rows for the pods that
    are no FitError, the mirror equal to the host's cache, no loop gave up."""
    assert len(got) == len(want)
    for k, ((rg, dg), (ro, do)) in enumerate(zip(got, want)):
        assert rg == ro, f"{tag} pod {k}: result {rg} != reference {ro}"
        assert dg == do, f"{tag} pod {k} (status {ro[0]}): diagnosis\n {dg}\n != reference\n {do}"
        if ro[0] not in FIT_ERROR:
            assert dg == empty(do["num_nodes"], do["prefilter_code"], do["prefilter_plugin"])
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


def all_in_agg_loop(g, n_pods):
    """Every pod of the last batch ran in k_agg_loop (the parent ran a diagnosed batch's on the per-pod launches)."""
    assert g.kernel_stats()[2:] == (n_pods, "k_agg_loop")


def input_conditions(want, klass, pts=True, ipa=True):
    """On the reference alone: at least 5 FitError pods among the pods of the loop's class (indices `klass`), one of
    them with a PodTopologySpread bin and one with an InterPodAffinity bin, and no PreFilter outcome among them."""
    failed = [want[k][1] for k in klass if want[k][0][0] in FIT_ERROR]
    assert len(failed) >= 5, len(failed)
    assert all(d["failed_nodes"] == d["num_nodes"] and d["prefilter_code"] == 0 for d in failed)
    assert not pts or any(d["plugin_nodes"][PTS] > 0 for d in failed)
    assert not ipa or any(d["plugin_nodes"][IPA] > 0 for d in failed)


def reference(cfg, nodes, existing, pods, nss=NSS, objects=()):
    ocfg = {k: v for k, v in cfg.items() if k not in LOOP_KEYS}
    return reference_stream(fill(oracle(ocfg), nodes, existing, nss, objects), pods)


def device(native, cfg, nodes, existing, nss=NSS, objects=()):
    return fill(native(dict(cfg, device=0)), nodes, existing, nss, objects)


def web(app="web"):
    return {"matchLabels": {"app": app}}


# the two flavours of a loop-class pod that fails nowhere by itself: a ScheduleAnyway hostname constraint (the run
# takes the PodTopologySpread-scoring instance) or a required anti-affinity term that matches nothing (the other one)
def soft(p):
    return p.spread(3, HOST, "ScheduleAnyway", web())


def anti_nothing(p):
    return p.pod_affinity(HOST, web("nothing"), anti=True)


FLAVOURS = {"soft": soft, "anti": anti_nothing}


# ---- 1. every failing status the class can produce --------------------------------------------------------------
N1 = 70  # one full wave and a partly filled one
TOL_UNSCHED = {"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoSchedule"}
TOL_DED = {"key": "dedicated", "operator": "Exists", "effect": "NoSchedule"}


def status_cluster():
    """70 nodes, every one unschedulable and tainted dedicated=x:NoSchedule, 4 cpu / 8Gi / 10Gi ephemeral / 2 gpus,
    room for 4 pods and two bound already: `hot-k` (app=hot, host port 8080) and, on the first node of each zone, a
    `guard` with a required zone anti-affinity term against app=victim (a plain `sitter` elsewhere)."""
    nodes, existing = [], []
    for k in range(N1):
        name = f"n{k:03d}"
        nodes.append(NodeW(name).capacity({"cpu": "4", "memory": "8Gi", "pods": "4", "ephemeral-storage": "10Gi",
                                           "example.com/gpu": "2"})
                     .label(HOST, name).label(ZONE, "ab"[k % 2]).unschedulable()
                     .taints([{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]).obj())
        existing.append(PodW(f"hot-{k}").label("app", "hot").container(image="i", requests={"cpu": "10m"})
                        .host_port(8080).node(name).obj())
        second = PodW(f"second-{k}").label("app", "sitter").container(image="i", requests={"cpu": "10m"}).node(name)
        if k < 2:
            second.pod_affinity(ZONE, web("victim"), anti=True)
        existing.append(second.obj())
    return nodes, existing


def status_stream(flavour):
    """Pods that each fail on all 70 nodes for one reason, between pods that land; then 140 small pods of which the
    last find every node full (Too many pods)."""
    mk = FLAVOURS[flavour]
    def base(name, cpu="100m", tol=(TOL_UNSCHED, TOL_DED), app="x", **req):
        p = PodW(name).label("app", app).container(image="i", requests=dict({"cpu": cpu}, **req))
        p.tolerations(list(tol))
        return mk(p)
    ok = lambda name: base(name).obj()
    nodename = base("nodename").obj()
    nodename["spec"]["nodeName"] = "no-such-node"
    pods = [
        base("unsched", tol=(TOL_DED,)).obj(),
        ok("ok0"),
        nodename,
        base("taint", tol=(TOL_UNSCHED,)).obj(),
        base("affinity").node_selector({"disk": "nvme"}).obj(),
        ok("ok1"),
        base("port").host_port(8080).obj(),
        base("cpu", cpu="5").obj(),
        base("mem", memory="9Gi").obj(),
        ok("ok2"),
        base("eph", **{"ephemeral-storage": "11Gi"}).obj(),
        base("gpu", **{"example.com/gpu": "3"}).obj(),
        base("cpu-mem", cpu="5", memory="9Gi").obj(),
        # every node holds an app=hot pod and 1000 domains are asked for: the minimum counts as 0, skew 2 > 1
        base("skew", app="hot").spread(1, HOST, "DoNotSchedule", web("hot"), min_domains=1000).obj(),
        ok("ok3"),
        base("label").spread(1, "rack", "DoNotSchedule", web("hot")).obj(),
        base("pod-aff").pod_affinity(HOST, web("nobody")).obj(),
        base("pod-anti").pod_affinity(ZONE, web("hot"), anti=True).obj(),
        base("existing-anti", app="victim").obj(),
        ok("ok4"),
    ]
    pods += [base(f"fill{k}", cpu="10m").obj() for k in range(2 * N1)]
    return pods


ALONE = [(R_UNSCHED, 3), (R_NODENAME, 3), (R_TAINT, 3), (R_NA, 3), (R_PORTS, 2), (R_TOO_MANY, 2), (R_CPU, 3), (R_MEM, 3),
         (R_EPH, 3), (R_SCALAR, 3), (R_PTS_SKEW, 2), (R_PTS_LABEL, 3), (R_IPA_AFF, 3), (R_IPA_ANTI, 2), (R_IPA_EXIST, 2)]


@functools.lru_cache(maxsize=None)
def status_reference(flavour):
    nodes, existing = status_cluster()
    pods = status_stream(flavour)
    want = reference({}, nodes, existing, pods)
    input_conditions(want, range(len(pods)))
    failed = [d for r, d in want if r[0] in FIT_ERROR]
    for bit, code in ALONE:  # a pod that fails on every node for this reason alone, with this code
        assert any(d["reason_nodes"][bit] == N1 and sum(d["reason_nodes"]) == N1 and
                   d["unresolvable_nodes"] == (N1 if code == 3 else 0) for d in failed), bit
    assert any(d["reason_nodes"][R_CPU] == N1 and d["reason_nodes"][R_MEM] == N1 for d in failed)
    assert sum(r[0] == 0 for r, _ in want) >= 5 + N1 // 2
    return nodes, existing, pods, want


@pytest.mark.parametrize("debug", [0, 2, 4, 32])
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_every_failing_status_of_the_class(native, flavour, debug):
    """aggLoopDebug 2: the generic filter path (no DF_LFAST); 4: no same-template shortcut; 32: no template cache."""
    nodes, existing, pods, want = status_reference(flavour)
    g = device(native, {"aggLoopDebug": debug} if debug else {}, nodes, existing)
    check(g, run_diag(g, pods), want, f"{flavour}, aggLoopDebug {debug}:")
    all_in_agg_loop(g, len(pods))


# ---- 2. shapes ------------------------------------------------------------------------------------------------------
def class_pod(rng, k, names):
    """A fuzz_gen pod of the loop's class: no PreFilterResult subset, and one of a ScheduleAnyway hostname constraint,
    a DoNotSchedule constraint over its own app, a required anti-affinity term or a required affinity term."""
    o = rand_pod(rng, k, names, topology=False)
    na = o["spec"].get("affinity", {}).get("nodeAffinity", {}).get("requiredDuringSchedulingIgnoredDuringExecution")
    if na and any("matchFields" in t for t in na["nodeSelectorTerms"]):
        del o["spec"]["affinity"]["nodeAffinity"]["requiredDuringSchedulingIgnoredDuringExecution"]
    p = PodW.__new__(PodW)
    p.o = o
    app = o["metadata"]["labels"]["app"]
    r = rng.random()
    if r < 0.3:
        p.spread(rng.randint(1, 3), HOST, "ScheduleAnyway", web(rng.choice(APPS)))
    elif r < 0.55:
        p.spread(1, rng.choice([ZONE, HOST, "disk"]), "DoNotSchedule", web(app))
    elif r < 0.85:
        p.pod_affinity(rng.choice([ZONE, HOST]), web(rng.choice(APPS)), anti=True)
    else:
        p.pod_affinity(ZONE, web(rng.choice(APPS)))
    return p.obj()


SHAPES = {  # name: (nodes, fuzz_gen config, seed, extra context config)
    "9": (9, 0, 41009, {}),
    "130": (130, 3, 41130, {}),
    "257": (257, 1, 41259, {}),
    "600": (600, 5, 41601, {}),
    "600-one-workgroup": (600, 5, 41601, {"loopWorkgroups": 1}),
}


@functools.lru_cache(maxsize=None)
def shape_reference(n_nodes, cfg_index, seed):
    """60 class pods on a cluster short of room (tests/test_gpu_diagnosis.py's random_case): small clusters get
    10-cpu nodes and few bound pods, large ones 1-cpu nodes with a 4-cpu node every sixth."""
    rng, cfg, nodes, existing, names = rand_cluster(seed, n_nodes=n_nodes, n_existing=40 if n_nodes >= 100 else 6,
                                                    cfg_index=cfg_index)
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
    pods = [class_pod(rng, k, names) for k in range(60)]
    want = reference(cfg, nodes, existing, pods, namespaces())
    input_conditions(want, range(len(pods)))
    assert sum(r[0] == 0 for r, _ in want) >= 20
    return cfg, nodes, existing, pods, want


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_random_class_streams(native, shape):
    """9 nodes: one partly filled wave; 257: two workgroups, the second with one node; 600 nodes with
    "loopWorkgroups": 1: a workgroup owns two 256-node blocks, so waves 4-7 hold nodes too, one of them partly."""
    n_nodes, cfg_index, seed, extra = SHAPES[shape]
    cfg, nodes, existing, pods, want = shape_reference(n_nodes, cfg_index, seed)
    g = device(native, dict(cfg, **extra), nodes, existing, namespaces())
    check(g, run_diag(g, pods), want, shape)
    assert g.kernel_stats()[3] == "k_agg_loop"


# ---- 3. places in a run -------------------------------------------------------------------------------------------
def box(name, zone, cpu="4"):
    return NodeW(name).capacity({"cpu": cpu, "memory": "8Gi", "pods": "20"}).label(HOST, name).label(ZONE, zone).obj()


def small(name, app, cpu="100m"):
    return PodW(name).label("app", app).container(image="i", requests={"cpu": cpu})


FOUR_BOXES = [box("za0", "a"), box("za1", "a"), box("zb0", "b"), box("zb1", "b")]
TWO_DBS = [small("db0", "db").node("za0").obj(), small("db1", "db").node("zb0").obj()]


def places_stream():
    solo = lambda k: small(f"solo{k}", "solo").pod_affinity(HOST, web("solo"), anti=True).obj()  # one per node
    spread = lambda name, cpu="100m": small(name, "web", cpu).spread(1, ZONE, "DoNotSchedule", web()).obj()
    return [
        small("first", "x").pod_affinity(ZONE, web("db"), anti=True).obj(),  # 0: fails, first in the run
        solo(0), solo(1), solo(2), solo(3),                                   # 1-4: one on each node
        solo(4), solo(5),                     # 5, 6: two failures in a row, pods of their template on both sides
        spread("w0"),                         # 7: another template after a failure
        solo(6),                              # 8: fails
        spread("w1"),                         # 9: another, cached template after a failure
        solo(7),                              # 10: fails
        spread("w2"),                         # 11: zones now hold 2 and 1 web pods
        spread("big", cpu="5"),               # 12: app=web, fails on cpu; placed, it would have moved the minimum
        spread("w3"),                         # 13: must still see 2 and 1: only the emptier zone takes it
        spread("w4"),                         # 14
        solo(8),                              # 15: fails, last in the run
    ]


@functools.lru_cache(maxsize=None)
def places_reference():
    pods = places_stream()
    want = reference({}, FOUR_BOXES, TWO_DBS, pods)
    assert [r[0] for r, _ in want] == [2, 0, 0, 0, 0, 2, 2, 0, 2, 0, 2, 0, 2, 0, 0, 2]
    input_conditions(want, range(len(pods)), pts=False)
    zone = lambda k: "a" if want[k][0][1] < 2 else "b"
    assert sorted(zone(k) for k in (7, 9, 11)) in (["a", "a", "b"], ["a", "b", "b"])
    fuller = "a" if [zone(k) for k in (7, 9, 11)].count("a") == 2 else "b"
    assert zone(13) != fuller and want[13][0][3] == 2  # two feasible nodes: the failed pod 12 is in no count
    assert want[12][1]["reason_nodes"][R_CPU] == 4 and want[0][1]["reason_nodes"][R_IPA_ANTI] == 4
    assert want[5][1]["reason_nodes"][R_IPA_ANTI] == 4 and want[5][1] == want[6][1]
    return pods, want


@pytest.mark.parametrize("debug", [0, 32])
def test_failing_pods_at_every_place_of_a_run(native, debug):
    pods, want = places_reference()
    g = device(native, {"aggLoopDebug": debug} if debug else {}, FOUR_BOXES, TWO_DBS)
    check(g, run_diag(g, pods), want, f"aggLoopDebug {debug}:")
    all_in_agg_loop(g, len(pods))


# ---- 4. the PodTopologySpread-scoring instances, and both instances of more than 64 workgroups -------------------
SERVICE = {"apiVersion": "v1", "kind": "Service", "metadata": {"name": "svc", "namespace": "default"},
           "spec": {"selector": {"app": "svc"}}}


def grid(n, zones="abc"):
    """n 4-cpu nodes over three zones; an app=db pod bound in each zone."""
    nodes = [box(f"g{k:05d}", zones[k % len(zones)]) for k in range(n)]
    existing = [small(f"db{z}", "db").node(f"g{k:05d}").obj() for k, z in enumerate(zones)]
    return nodes, existing


def scored_stream(n_ok=3):
    """Pods the Service selects, without constraints of their own (the System defaults: ScheduleAnyway on hostname and
    zone), and pods with their own ScheduleAnyway constraints; of both kinds some that fail."""
    own = lambda name, cpu="100m": small(name, "own", cpu).spread(2, ZONE, "ScheduleAnyway", web("own")) \
        .spread(1, HOST, "ScheduleAnyway", web("own"))
    pods = []
    for k in range(n_ok):
        pods += [small(f"s{k}", "svc").obj(), own(f"o{k}").obj()]
    pods += [
        small("s-cpu", "svc", cpu="5").obj(),
        own("o-label").spread(1, "rack", "DoNotSchedule", web("own")).obj(),
        small("s-ok", "svc").obj(),
        own("o-anti").pod_affinity(ZONE, web("db"), anti=True).obj(),
        own("o-mem").container(image="i", requests={"memory": "9Gi"}).obj(),
        own("o-ok").obj(),
        small("s-mem", "svc").container(image="i", requests={"memory": "9Gi"}).obj(),
        own("o-aff").pod_affinity(HOST, web("nobody")).obj(),
        small("s-last", "svc", cpu="4500m").obj(),
    ]
    return pods


def unscored_stream():
    """The same outcomes from pods without PodTopologySpread scoring (a required anti-affinity term matching nothing)."""
    mk = lambda name, cpu="100m": anti_nothing(small(name, "x", cpu))
    return [
        mk("a0").obj(), mk("a1").obj(),
        mk("a-cpu", cpu="5").obj(),
        mk("a-label").spread(1, "rack", "DoNotSchedule", web("x")).obj(),
        mk("a2").obj(),
        mk("a-anti").pod_affinity(ZONE, web("db"), anti=True).obj(),
        mk("a-mem").container(image="i", requests={"memory": "9Gi"}).obj(),
        mk("a3").obj(),
        mk("a-aff").pod_affinity(HOST, web("nobody")).obj(),
        mk("a-last", cpu="4500m").obj(),
    ]


@functools.lru_cache(maxsize=None)
def grid_reference(n, scored):
    nodes, existing = grid(n)
    pods = scored_stream() if scored else unscored_stream()
    objects = (SERVICE,) if scored else ()
    want = reference({}, nodes, existing, pods, NSS, objects)
    input_conditions(want, range(len(pods)))
    assert sum(r[0] == 0 for r, _ in want) >= 4
    return nodes, existing, pods, objects, want


@pytest.mark.parametrize("n", [130, 600])
def test_pts_scoring_instance(native, n):
    nodes, existing, pods, objects, want = grid_reference(n, True)
    g = device(native, {}, nodes, existing, NSS, objects)
    check(g, run_diag(g, pods), want, f"{n} nodes:")
    all_in_agg_loop(g, len(pods))


BIG = 64 * 256 + 6  # 65 node blocks: 65 workgroups, the instances that sweep more than one round of 64 participants


@pytest.mark.parametrize("scored", [False, True])
def test_more_than_64_workgroups(native, scored):
    nodes, existing, pods, objects, want = grid_reference(BIG, scored)
    g = device(native, {}, nodes, existing, NSS, objects)
    check(g, run_diag(g, pods), want, f"scored {scored}:")
    all_in_agg_loop(g, len(pods))


# ---- 5. mixed batches -----------------------------------------------------------------------------------------------
def mixed_stream():
    """Node-local and loop-class pods two by two (runs alternate between k_sched_loop and k_agg_loop), an own-nominated
    pod and a matchFields subset pod of the class on the per-pod launches; 48 pods in chunks from 8 pods on."""
    pods, klass = [], []
    for k in range(48):
        if k == 13:
            p = soft(small("own-nominated", "web", cpu="4100m")).obj()
            p["status"] = {"nominatedNodeName": "g00001"}
        elif k == 29:
            p = soft(small("subset", "web", cpu="3500m")).node_affinity_required(
                [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": ["g00000", "g00002"]}]}]).obj()
        elif k % 4 < 2:
            p = small(f"plain{k}", "plain", cpu="5" if k % 8 == 0 else "700m").obj()
        else:
            klass.append(k)
            mk = soft if k % 8 < 4 else anti_nothing
            if k % 12 == 2:
                p = mk(small(f"k-cpu{k}", "web", cpu="4500m")).obj()
            elif k % 12 == 6:
                p = mk(small(f"k-anti{k}", "web")).pod_affinity(ZONE, web("db"), anti=True).obj()
            elif k % 12 == 10:
                p = mk(small(f"k-label{k}", "web")).spread(1, "rack", "DoNotSchedule", web()).obj()
            else:
                p = mk(small(f"k{k}", "web", cpu="700m")).obj()
        pods.append(p)
    return pods, klass


@functools.lru_cache(maxsize=None)
def mixed_reference():
    nodes, existing = grid(9)
    pods, klass = mixed_stream()
    want = reference({}, nodes, existing, pods)
    input_conditions(want, klass)
    plain = [k for k in range(len(pods)) if k not in klass and k not in (13, 29)]
    assert sum(want[k][0][0] in FIT_ERROR for k in plain) >= 3
    assert want[29][0][0] in FIT_ERROR and want[29][1]["reason_nodes"][R_PREFILTER] == 7  # outside the subset
    assert want[13][0][0] in FIT_ERROR  # its nominated node fails alone, then every node does
    return nodes, existing, pods, want


def test_mixed_batch_over_chunks(native):
    nodes, existing, pods, want = mixed_reference()
    g = device(native, {"pipelineFirstChunk": 8}, nodes, existing)
    check(g, run_diag(g, pods), want)


# ---- 6. under {"nominatedPods": "Evaluate"} ------------------------------------------------------------------------
def nominee(k):
    return {"metadata": {"name": f"nom{k}", "namespace": "default", "uid": f"nom{k}"},
            "spec": {"priority": 100, "containers": [{"name": "c", "image": "i",
                                                      "resources": {"requests": {"cpu": "3500m"}}}]},
            "status": {"nominatedNodeName": f"n{k}"}}


@functools.lru_cache(maxsize=None)
def nominations_reference():
    nodes = [box(f"n{k}", "ab"[k % 2]) for k in range(6)]
    def pod(name, cpu, prio):
        p = soft(small(name, "web", cpu)).obj()
        p["spec"]["priority"] = prio
        return p
    pods = [pod("l0", "3500m", 0), pod("l1", "3500m", 0), pod("low", "1", 0), pod("top", "1", 200), pod("low2", "1", 50),
            pod("low3", "1", 0), pod("top2", "1", 200), pod("low4", "1", 10), pod("low5", "1", 0)]
    ref = NominatedReference({}, nodes, [], NSS)
    for k in range(4):
        ref.add_nominated_pod(nominee(k))
    want = []
    for p in pods:
        d = {}
        t = ref.schedule(copy.deepcopy(p), detail=d)
        want.append((t, reduce_eval(t[0], d["ev"], 6)))
    assert [t[0] for t, _ in want] == [0, 0, 2, 0, 2, 2, 0, 2, 2]
    input_conditions(want, range(len(pods)), pts=False, ipa=False)
    assert want[2][1]["reason_nodes"][R_CPU] == 6 and ref.flips >= 4
    return nodes, pods, want


def test_class_stream_under_nominations(native):
    """Loop-class pods without DoNotSchedule constraints or required terms (a ScheduleAnyway hostname constraint) are
    not refused.  Four of six nodes hold a priority-100 nomination of 3500m; once the two free nodes are taken, the
    priority-0 pods of 1 cpu fail on all six with Insufficient cpu -- on four of them only because of the nominations
    -- while a priority-200 pod still lands.  (No PodTopologySpread / InterPodAffinity bin can occur in this class.)"""
    nodes, pods, want = nominations_reference()
    g = device(native, {"nominatedPods": "Evaluate"}, nodes, [])
    for k in range(4):
        g.add_nominated_pod(nominee(k))
    check(g, run_diag(g, pods), want)
    all_in_agg_loop(g, len(pods))


# ---- 7. plain and diagnosed agree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["status-soft", "status-anti", "130", "600"])
def test_diagnosed_and_plain_batches_agree(native, case):
    """Two identical contexts: ksg_schedule_batch_diag returns what ksg_schedule_batch returns, both from k_agg_loop."""
    if case.startswith("status-"):
        nodes, existing, pods, want = status_reference(case[7:])
        cfg, nss = {}, NSS
    else:
        n_nodes, cfg_index, seed, _ = SHAPES[case]
        cfg, nodes, existing, pods, want = shape_reference(n_nodes, cfg_index, seed)
        nss = namespaces()
    a = device(native, cfg, nodes, existing, nss)
    b = device(native, cfg, nodes, existing, nss)
    plain = [r.as_tuple() for r in a.schedule_batch([a.compile(p) for p in pods], assume=True)]
    diag = [r for r, _ in run_diag(b, pods)]
    assert plain == diag == [r for r, _ in want]
    assert a.kernel_stats()[3] == b.kernel_stats()[3] == "k_agg_loop"
    assert a.compare_mirror(sync=True) == (0, -1) and b.compare_mirror(sync=True) == (0, -1)
