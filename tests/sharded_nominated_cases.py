"""The streams of tests/test_gpu_sharded_nominated.py and their references, computed once each from oracle parts only,
and the per-rank figures tests/test_sharded_nominated_reference.py checks on them: which rank's node range
(shard_range's rule: blocks floor(NB * r / W) .. floor(NB * (r + 1) / W) of 256 nodes) decides what.

Only tests/ use this module."""
import copy
import functools
import random

from fuzz_gen import namespaces, rand_cluster
from ksg.abi import SUCCESS
from ksg.objects import PodW
from nominated_reference import NominatedReference
from oracle_binding import oracle
from test_gpu_nominated import _nominate, _stream
from test_gpu_nominated_pods import nominee, random_case, random_nominees, random_stream

GATE_OFF = {"OpportunisticBatching": False}  # as on every node-sharded context
BLOCK = 256
OWN_MODES = [(100, "batch"), (30, "batch"), (0, "calls"), (100, "eval")]
EVAL_NODES = [9, 130, 257, 600]


def shard_ranges(n, world):
    nb = (n + BLOCK - 1) // BLOCK
    return [(min(nb * r // world * BLOCK, n), min(nb * (r + 1) // world * BLOCK, n)) for r in range(world)]


def per_rank(indices, n, world):
    return [sum(a <= i < b for i in indices) for a, b in shard_ranges(n, world)]


def _filled(backend, nodes, existing, nss, objects=()):
    for ns in nss:
        backend.upsert_namespace(ns)
    for o in objects:
        backend.upsert_object(o)
    for nd in nodes:
        backend.add_node(nd)
    for p in existing:
        backend.add_pod(p)
    return backend


# ---- the pod's own nominated node ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _own_case(pct, mode):
    """test_gpu_nominated.py::test_random_nominations_match_oracle's 700-node stream behind three directed pods: small
    pods nominated to a node of the last block that takes them, and to snapshot indices 255 and 256.
    -> cfg, nodes, existing, pods, [(oracle result tuple, evaluation output)], and per pod the snapshot index of its
    nominated node with what became of it there ("placed" / "failed"; pods without one are absent)."""
    rng, cfg, nodes, existing, names = rand_cluster(5150 + pct + len(mode), n_nodes=700, n_existing=150)
    cfg = dict(cfg, percentageOfNodesToScore=pct)
    ocfg = dict(cfg, featureGates=GATE_OFF)
    # (every node processed: behind a percentageOfNodesToScore cut a node carries no status, which reads as Success)
    probe = _filled(oracle(dict(ocfg, percentageOfNodesToScore=100)), nodes, existing, namespaces())
    order = probe.node_names()
    small = lambda name: PodW(name, uid=name).req({"cpu": "50m", "memory": "16Mi"}).obj()
    _, ev = probe.schedule_one(probe.compile(small("probe")), assume=False, evaluate=True)
    last = next(i for i in range(2 * BLOCK, len(order)) if ev["node_code"][i] == SUCCESS)
    directed = [_nominate(small(f"d{i}"), order[i]) for i in (last, 255, 256)]
    pods = directed + _stream(rng, names, 160)
    o = _filled(oracle(ocfg), nodes, existing, namespaces())
    index = {nm: i for i, nm in enumerate(order)}
    want, fate = [], {}
    for k, p in enumerate(pods):
        r, e = o.schedule_one(o.compile(p), assume=True, evaluate=True)
        want.append((r.as_tuple(), e))
        nn = index.get((p.get("status") or {}).get("nominatedNodeName") or "", -1)
        # (a PreFilter rejection or an empty PreFilterResult ends the cycle before the nominated node: nothing evaluated)
        if nn < 0 or e["prefilter_code"] or r.evaluated_nodes == 0:
            continue
        # evaluateNominatedNode took the node: it alone was evaluated, and nothing scored
        fate[k] = (nn, "placed" if r.as_tuple() == (0, nn, 1, 1, 0) else "failed")
    return cfg, nodes, existing, pods, want, fate


def own_reference(pct, mode):
    return _own_case(pct, mode)[:5]


def own_fates(pct, mode):
    return _own_case(pct, mode)[5]


# ---- nominatedPods "Evaluate" -------------------------------------------------------------------------------------------
class CountingReference(NominatedReference):
    """NominatedReference that also keeps where the nominated pods alone made a node a failure (its `flips`, by
    snapshot index)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.flipped = []

    def evaluate(self, pod):
        h, ev, ev2 = super().evaluate(pod)
        self.flipped += [i for i, (c1, c2) in enumerate(zip(ev["node_code"], ev2["node_code"]))
                         if c2 == SUCCESS and c1 != SUCCESS]
        return h, ev, ev2


@functools.lru_cache(maxsize=None)
def _evaluate_reference(n_nodes):
    rng, cfg, nodes, existing, names = random_case(n_nodes)
    ref = CountingReference(dict(cfg, featureGates=GATE_OFF), nodes, existing, namespaces())
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
    assert len(ref.flipped) == ref.flips
    return cfg, nodes, existing, noms, pods, want, list(ref.flipped)


def evaluate_reference(n_nodes):
    """test_gpu_nominated_pods.py's random case at n_nodes, OpportunisticBatching off."""
    return _evaluate_reference(n_nodes)[:6]


def evaluate_flips(n_nodes):
    return _evaluate_reference(n_nodes)[6]


# ---- preemption end to end ------------------------------------------------------------------------------------------------
def preemption_steps():
    """test_gpu_nominated_pods.py::test_preemption_basic_stream's shape on 300 full nodes (two blocks), as steps with the
    reference's answers: [(nodes, bound pods, namespaces), ("one", pod, result), ("preempt", pod, args, result, detail),
    ("remove", uid), ("nominate", pod), ("batch", pods, results), ...]."""
    from nominator_scenario import node as plain_node, pod as plain_pod
    nodes = [plain_node(f"n{k:03d}") for k in range(300)]
    nss = [{"metadata": {"name": "default"}}]
    low = []
    for k in range(300):
        for j in range(4):
            p = plain_pod(f"low-{k}-{j}", prio=0, cpu="900m")
            p["spec"]["nodeName"] = f"n{k:03d}"
            p["status"]["startTime"] = f"2024-01-01T{k // 60:02d}:{k % 60:02d}:{j:02d}Z"
            low.append(p)
    ref = NominatedReference({"featureGates": GATE_OFF}, nodes, low, nss)
    steps = [(nodes, low, nss)]
    one = lambda p: steps.append(("one", p, ref.schedule(p)))  # noqa: E731
    pending, chosen, most = [], [], 0
    for q in range(6):
        hi = plain_pod(f"hi{q}", prio=100, cpu="2")
        one(hi)
        assert steps[-1][2][0] == 2  # the cluster is full
        args = {"offset": 131 * q, "now": 1704067200 * 10 ** 9, "listCandidates": True}
        want, dwant = ref.preempt(hi, args)
        assert want[0] == 0
        steps.append(("preempt", hi, args, want, dwant))
        for uid in dwant["victims"]:
            ref.remove_pod(uid)
            steps.append(("remove", uid))
        hi = _nominate(hi, dwant["selected"])
        chosen.append(ref.index[dwant["selected"]])
        ref.add_nominated_pod(hi)
        steps.append(("nominate", hi))
        pending.append(hi)
        most = max(most, len(ref.nominator))
        for j in range(3):  # other pods while the nominations are outstanding: the room the victims left is spoken for
            one(plain_pod(f"other{q}-{j}", prio=0, cpu="300m"))
        batch = [plain_pod(f"ob{q}-{j}", prio=100, cpu="300m") for j in range(2)]
        steps.append(("batch", batch, [ref.schedule(p) for p in batch]))
        if q % 2:  # the nominees' own cycles, two at a time
            for p in pending:
                one(p)
                assert steps[-1][2][0] == 0 and steps[-1][2][2:] == (1, 1, 0)
            pending = []
    assert most >= 2 and not ref.nominator
    assert min(chosen) < BLOCK <= max(chosen), chosen  # nominated nodes in both ranks' ranges
    return steps


def preemption_all_steps(n_nodes=288):
    """test_gpu_nominated_preempt.py::test_preemption_basic_stream_of_spread_preemptors' shape on two blocks of full nodes
    in 3 zones, for "nominatedPods": "EvaluateAll" + "preemptNominatedPods": "EvaluateAll": priority-100 pods that
    spread over the zones (DoNotSchedule, matching their own label) -- failed cycle, ksg_preempt, the victims deleted,
    nominated on every rank, other pods under the nominations, the next preemptor (which sees the earlier ones as
    nominees that count in its constraint), then the nominees' own cycles.  Steps as preemption_steps, against
    nominated_preempt_reference.  -> (steps, the reference's counters)."""
    from nominated_preempt_reference import NAMESPACES2, NOW, NominatedPreemptReference, low, zoned
    from nominated_topology_reference import ZONE, labelled, spread
    from nominator_scenario import pod as plain_pod
    nodes = zoned(n_nodes, 3)
    lows = []
    for k in range(n_nodes):
        for j in range(4):
            p = low(f"low-{k}-{j}", f"n{k}", cpu="900m", app="low")
            # (the latest start times, which pickOneNodeForPreemption prefers, lie scattered: node i * 119 % n has rank i)
            t = next(i for i in range(n_nodes) if i * 119 % n_nodes == k)
            p["status"]["startTime"] = f"2024-01-01T{t // 60:02d}:{t % 60:02d}:{j:02d}Z"
            lows.append(p)
    ref = NominatedPreemptReference({"featureGates": GATE_OFF}, nodes, lows, NAMESPACES2)
    steps = [(nodes, lows, NAMESPACES2)]
    one = lambda p: steps.append(("one", p, ref.schedule(p)))  # noqa: E731
    pending, chosen = [], []
    for q in range(5):
        hi = spread(labelled(plain_pod(f"hi{q}", prio=100, cpu="2"), app="hi"), ZONE, "hi")
        one(hi)
        assert steps[-1][2][0] == 2  # the cluster is full, or the room is spoken for
        args = {"offset": 67 * q, "now": NOW, "listCandidates": True, "minCandidateNodesPercentage": 100,
                "minCandidateNodesAbsolute": 100}
        want, dwant = ref.preempt(hi, args)
        assert want[0] == 0, (q, want)
        steps.append(("preempt", hi, args, want, dwant))
        for uid in dwant["victims"]:
            ref.remove_pod(uid)
            steps.append(("remove", uid))
        hi = _nominate(hi, dwant["selected"])
        chosen.append(ref.index[dwant["selected"]])
        ref.add_nominated_pod(hi)
        steps.append(("nominate", hi))
        pending.append(hi)
        # others under the nominations: the room the victims left is spoken for.  (Of the preemptors' priority: a later
        # dry run then never lists them as victims, whose uids of assumed pods each backend numbers in its own way)
        for j in range(2):
            one(plain_pod(f"other{q}-{j}", prio=100, cpu="300m"))
    c = ref.counters()
    assert c["closed"] >= 3 and c["differs"] >= 1, c  # the nominees decide statuses and reprieves
    for p in pending:  # the nominees' own cycles
        one(p)
        assert steps[-1][2][0] == 0
    assert not ref.nominator
    assert min(chosen) < BLOCK <= max(chosen), chosen  # nominated nodes in both ranks' ranges
    return steps, c


# ---- k_agg_loop's class ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def agg_class_case():
    """test_gpu_nominated_pods.py::test_agg_loop_class's pods and nominations: 300 nodes in 3 zones (two blocks), a
    Service selecting the pods, every third pod with a ScheduleAnyway constraint and a preferred anti-affinity term."""
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
    cfg = {}
    ref = NominatedReference(dict(cfg, featureGates=GATE_OFF), nodes, init, namespaces(), objects)
    rng = random.Random(4)
    noms = [nominee(f"nom{k}", rng.choice([0, 100]), ref.names[[0, 255, 256, 299, 7, 100, 150, 290][k]], cpu="3700m",
                    ns="service-ns") for k in range(8)]
    for q in noms:
        ref.add_nominated_pod(q)
    want = [ref.schedule(copy.deepcopy(p)) for p in pods]
    return cfg, nodes, init, objects, noms, pods, want
