"""RunFilterPluginsWithNominatedPods (framework/runtime/framework.go:1211-1294) for the pairs in which the nominated
pods move a count PodTopologySpread or InterPodAffinity reads -- what a context created with
{"nominatedPods": "EvaluateAll"} must reproduce (include/ksg.h).  Built from oracle parts only.

NominatedReference adds every nominee at once for pass 1, which is exact while only node-local filters read them.
Here a nominee moves per-domain counts, and the reference adds node n's nominees for node n's pass 1 only (the cloned
PreFilter state gets their AddPod; another node of the same zone sees none of it).  So for a pod p:

* pass 2: one evaluation on the oracle context as it is (st0).
* pass 1, per snapshot node n with non-empty G(p, n): one evaluation with only G(p, n) added as bound pods, of which
  node n's status is kept (st1).  The oracle recomputes PreFilter from scratch; for both plugins that equals the
  incremental AddPod (pure additions, criticalPaths then holds the true minimum) -- but for the Skip rule: PreFilter
  runs once, without nominees, and a plugin that returned Skip runs in neither pass.  PodTopologySpread's Skip depends
  on the pod alone.  InterPodAffinity's depends on the existing pods, so a pass-1 status of InterPodAffinity counts as
  Success when InterPodAffinity's PreFilter on the context as it is returned Skip (it is the last filter: everything
  before it passed).
* the node's status is st1 if that is not Success, else st0.  No monotonicity: a required affinity that only a nominee
  satisfies passes pass 1 and fails pass 2.

Counters (conditions on a stream's inputs, not measurements):
  closed   st1 fails in PodTopologySpread or InterPodAffinity while st0 is Success
  granted  st0 is an InterPodAffinity affinity failure while st1 is Success
  split    a feasible node without G that shares a zone with a `closed` node of the same cycle
  skipped  a nominee's anti-affinity term matches p while InterPodAffinity is skipped

Only tests/ use this module.
"""
import copy

from fuzz_gen import APPS, rand_cluster, rand_pod
from ksg.abi import PLUGIN_ID, SKIP, SUCCESS, UNSCHEDULABLE, UNSCHEDULABLE_AND_UNRESOLVABLE
from nominated_reference import NominatedReference
from nominator_scenario import node as plain_node, pod as plain_pod

ZONE = "topology.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"
PTS, IPA = PLUGIN_ID["PodTopologySpread"], PLUGIN_ID["InterPodAffinity"]
R_PTS_SKEW, R_IPA_AFFINITY, R_IPA_ANTI, R_IPA_EXISTING_ANTI = 1 << 12, 1 << 13, 1 << 14, 1 << 15
EVALUATE_ALL = {"nominatedPods": "EvaluateAll"}


class NominatedTopologyReference(NominatedReference):
    def __init__(self, cfg, nodes, existing, namespaces=(), objects=()):
        super().__init__(cfg, nodes, existing, namespaces, objects)
        zone = {n["metadata"]["name"]: (n["metadata"].get("labels") or {}).get(ZONE) for n in nodes}
        self.zone = [zone[name] for name in self.names]
        self.closed = self.granted = self.split = self.skipped = 0

    def evaluate(self, pod):
        plain = copy.deepcopy(pod)
        plain["status"] = {k: v for k, v in (pod.get("status") or {}).items() if k != "nominatedNodeName"}
        h = self.A.compile(plain)
        _, ev2 = self.A.schedule_one(h, assume=False, evaluate=True)
        ev = dict(ev2, node_code=list(ev2["node_code"]), node_plugin=list(ev2["node_plugin"]),
                  node_reasons=list(ev2["node_reasons"]))
        by_node = {}
        for q, ix in self.g(pod):
            by_node.setdefault(ix, []).append((q, ix))
        if not by_node:
            return h, ev, ev2
        ipa_skipped = self.A.run_filter_plugin(h, IPA)[0] == SKIP
        closed_zones = set()
        for i, gi in sorted(by_node.items()):
            _, ev1 = self._with_g(gi, lambda: self.A.schedule_one(h, assume=False, evaluate=True))
            st1 = (ev1["node_code"][i], ev1["node_plugin"][i], ev1["node_reasons"][i])
            if st1[0] != SUCCESS and st1[1] == IPA and ipa_skipped:
                self.skipped += 1
                st1 = (SUCCESS, ev2["node_plugin"][i], 0)
            if st1[0] != SUCCESS:
                if ev2["node_code"][i] == SUCCESS:
                    self.flips += 1
                    if st1[1] in (PTS, IPA):
                        self.closed += 1
                        closed_zones.add(self.zone[i])
                ev["node_code"][i], ev["node_plugin"][i], ev["node_reasons"][i] = st1
            elif (ev2["node_code"][i] != SUCCESS and ev2["node_plugin"][i] == IPA
                  and ev2["node_reasons"][i] & R_IPA_AFFINITY):
                self.granted += 1
        closed_zones.discard(None)
        for i in range(len(self.names)):
            if i not in by_node and ev["node_code"][i] == SUCCESS and self.zone[i] in closed_zones:
                self.split += 1
        return h, ev, ev2

    def counters(self):
        return {"closed": self.closed, "granted": self.granted, "split": self.split, "skipped": self.skipped}


# ---- hand-computed cases ------------------------------------------------------------------------------------------
def zoned_nodes(n, zones):
    nodes = [plain_node(f"n{k}") for k in range(n)]
    for k, nd in enumerate(nodes):
        nd["metadata"]["labels"][ZONE] = f"z{k % zones}"
    return nodes


def labelled(p, **labels):
    p["metadata"]["labels"] = dict(labels)
    return p


def bound(name, node, **labels):
    p = labelled(plain_pod(name), **labels)
    p["spec"]["nodeName"] = node
    return p


def spread(p, key, app, max_skew=1):
    p["spec"]["topologySpreadConstraints"] = [{"maxSkew": max_skew, "topologyKey": key,
                                               "whenUnsatisfiable": "DoNotSchedule",
                                               "labelSelector": {"matchLabels": {"app": app}}}]
    return p


def pod_affinity(p, kind, key, app):
    p["spec"].setdefault("affinity", {})[kind] = {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"topologyKey": key, "labelSelector": {"matchLabels": {"app": app}}}]}
    return p


def hand_cases():
    """-> [(name, nodes, existing, nominees, pod, {node name: (code, plugin, reasons)} of the failing nodes,
    (status, EvaluatedNodes, FeasibleNodes))], each worked out by hand; every node not listed is feasible.  Nodes
    n0..n3 lie in zones z0 z1 z0 z1 (n0..n5 in z0 z1 z2 z0 z1 z2 for (iii)); nominees have priority 100, the pod 0."""
    skew = (UNSCHEDULABLE, PTS, R_PTS_SKEW)
    aff = (UNSCHEDULABLE_AND_UNRESOLVABLE, IPA, R_IPA_AFFINITY)
    anti = (UNSCHEDULABLE, IPA, R_IPA_ANTI)
    exanti = (UNSCHEDULABLE, IPA, R_IPA_EXISTING_ANTI)
    nom = lambda name, node, **labels: labelled(plain_pod(name, prio=100, nominated=node), **labels)  # noqa: E731
    web = lambda: labelled(plain_pod("p"), app="web")  # noqa: E731
    anti_nom = pod_affinity(nom("nom", "n1", app="db"), "podAntiAffinity", HOST, "web")
    hater = pod_affinity(bound("e0", "n0", app="db"), "podAntiAffinity", HOST, "web")
    return [
        # zones 1/1, minimum 1.  n1 with the nominee: z1 = 2, the other zone keeps the minimum 1: 2 + 1 - 1 > 1.
        # n3, z1 too, sees no nominee: 1 + 1 - 1.
        ("i", zoned_nodes(4, 2), [bound("e0", "n0", app="web"), bound("e1", "n1", app="web")],
         [nom("nom", "n1", app="web")], spread(web(), ZONE, "web"), {"n1": skew}, (SUCCESS, 4, 3)),
        # zones 0/1, minimum 0: z1's nodes fail in both passes (1 + 1 - 0).  n0 with the nominee: z0 = 1, and z0 held
        # the minimum alone, so the minimum rises to 1 with it: 1 + 1 - 1.
        ("ii", zoned_nodes(4, 2), [bound("e1", "n1", app="web")], [nom("nom", "n0", app="web")],
         spread(web(), ZONE, "web"), {"n1": skew, "n3": skew}, (SUCCESS, 4, 2)),
        # zones 0/0/1: two zones hold the minimum 0, so it stays 0 when n0's zone rises to 1: 1 + 1 - 0 > 1.
        ("iii", zoned_nodes(6, 3), [bound("e2", "n2", app="web")], [nom("nom", "n0", app="web")],
         spread(web(), ZONE, "web"), {"n0": skew, "n2": skew, "n5": skew}, (SUCCESS, 6, 3)),
        # a required affinity only the nominee satisfies: pass 1 succeeds on n1, pass 2 fails everywhere.
        ("iv", zoned_nodes(4, 2), [], [nom("nom", "n1", app="db")],
         pod_affinity(web(), "podAffinity", ZONE, "db"), {f"n{k}": aff for k in range(4)}, (UNSCHEDULABLE, 4, 0)),
        # the pod matches its own affinity term and no pod matches anywhere: feasible everywhere (pass 2); on n1
        # pass 1 finds the nominee in n1's zone.
        ("v", zoned_nodes(4, 2), [], [nom("nom", "n1", app="web")],
         pod_affinity(web(), "podAffinity", ZONE, "web"), {}, (SUCCESS, 4, 4)),
        # anti-affinity over the zone: n1 fails with its nominee added, its zone-mate n3 never sees it.
        ("vi", zoned_nodes(4, 2), [], [nom("nom", "n1", app="db")],
         pod_affinity(web(), "podAntiAffinity", ZONE, "db"), {"n1": anti}, (SUCCESS, 4, 3)),
        # the nominee's anti-affinity term matches the pod, but InterPodAffinity's PreFilter skipped: never checked.
        ("vii", zoned_nodes(4, 2), [], [anti_nom], web(), {}, (SUCCESS, 4, 4)),
        # the same with an existing pod whose anti-affinity term matches the pod: no Skip, n0 fails in both passes and
        # n1 with its nominee added.
        ("viii", zoned_nodes(4, 2), [hater], [copy.deepcopy(anti_nom)], web(), {"n0": exanti, "n1": exanti},
         (SUCCESS, 4, 2)),
    ]


NAMESPACE = [{"metadata": {"name": "default"}}]


# ---- streams --------------------------------------------------------------------------------------------------------
SIZES = [9, 130, 257, 600]
CFG_OF = {9: 0, 130: 6, 257: 0, 600: 7}
N_EXISTING = {9: 12, 130: 60, 257: 60, 600: 60}
N_PODS = 38  # + the two nominees' own cycles


def topology_nominees(rng, order, ns_of=lambda k: "default"):
    """6 to 10 nominees of priorities {0, 50, 100}: on snapshot index 0 (two of them), 255, 256, the last index, a name
    outside the snapshot and random nodes; labels from the stream's vocabulary, every third one with a required
    anti-affinity term."""
    n = len(order)
    where = [0, 0, 255, 256, n - 1, -1] + [rng.randrange(n) for _ in range(rng.randint(0, 4))]
    out = []
    for k, ix in enumerate(where):
        if ix >= n:
            ix = rng.randrange(n)
        q = plain_pod(f"nom{k}", prio=rng.choice([0, 50, 100]), cpu="100m",
                      nominated=order[ix] if ix >= 0 else "no-such-node")
        q["metadata"]["namespace"] = ns_of(k)
        q["metadata"]["labels"] = {"app": APPS[k % len(APPS)], "tier": rng.choice(["fe", "be"])}
        if k % 3 == 2:
            pod_affinity(q, "podAntiAffinity", rng.choice([HOST, ZONE]), "cache")
        out.append(q)
    out[0]["spec"]["priority"], out[1]["spec"]["priority"] = 100, 50  # index 0: two records, one above the other
    return out


def roomy(nodes):
    for nd in nodes:  # the topology filters decide, not taints or resources
        nd["spec"] = {k: v for k, v in (nd.get("spec") or {}).items() if k not in ("taints", "unschedulable")}
        for key in ("allocatable", "capacity"):
            nd["status"][key].update({"cpu": "64", "memory": "256Gi", "pods": "110"})
    return nodes


def directed_pod(rng, k, names):
    """Pods of priority 0 in `default` whose spread constraints and affinity terms select the nominees' labels."""
    kind = k % 6
    if kind == 5:
        p = rand_pod(rng, k, names, ns="default")
        p["spec"]["priority"] = 0
        return p
    p = labelled(plain_pod(f"p{k}", cpu="100m"), app=["web", "web", "batch", "batch", "cache"][kind])
    if kind == 0:
        spread(p, HOST, "web")
    elif kind == 1:
        spread(p, ZONE, "web", max_skew=rng.choice([1, 2]))
    elif kind == 2:
        pod_affinity(p, "podAffinity", HOST, ["web", "db"][k // 6 % 2])
    elif kind == 3:
        pod_affinity(p, "podAntiAffinity", ZONE, rng.choice(["web", "db"]))
    return p  # kind 4: a plain pod the nominees' anti-affinity terms (against app=cache) match


def directed_case(n_nodes):
    rng, cfg, nodes, existing, names = rand_cluster(7300 + n_nodes, n_nodes=n_nodes, n_existing=N_EXISTING[n_nodes],
                                                    cfg_index=CFG_OF[n_nodes], topology=False)
    for p in existing:
        p["metadata"]["namespace"] = "default"
    pods = [directed_pod(rng, k, names) for k in range(N_PODS)]
    return rng, cfg, roomy(nodes), existing, pods


def random_case(n_nodes):
    rng, cfg, nodes, existing, names = rand_cluster(8300 + n_nodes, n_nodes=n_nodes, n_existing=N_EXISTING[n_nodes],
                                                    cfg_index=CFG_OF[n_nodes])
    pods = []
    for k in range(N_PODS):
        p = rand_pod(rng, k, names)
        p["spec"]["priority"] = rng.choice([0, 50, 100])
        pods.append(p)
    return rng, cfg, nodes, existing, pods


def stream_reference(family, n_nodes):
    """-> (cfg, nodes, existing, nominees, pods, [(result tuple, detail)], counters): the case and the reference's
    outcome per pod, every pod assumed.  The nominees' own cycles are inside the stream."""
    from fuzz_gen import NAMESPACES, namespaces
    rng, cfg, nodes, existing, pods = (directed_case if family == "directed" else random_case)(n_nodes)
    ref = NominatedTopologyReference(cfg, nodes, existing, namespaces())
    ns_of = (lambda k: "default") if family == "directed" else (lambda k: NAMESPACES[k % len(NAMESPACES)][0])
    noms = topology_nominees(rng, ref.names, ns_of)
    for q in noms:
        ref.add_nominated_pod(q)
    pods = list(pods)
    pods.insert(25, copy.deepcopy(noms[1]))
    pods.insert(33, copy.deepcopy(noms[-1]))
    want = []
    for p in pods:
        d = {}
        t = ref.schedule(p, detail=d)
        d["weights"] = ref.weights
        want.append((t, d))
    return cfg, nodes, existing, noms, pods, want, ref.counters()
