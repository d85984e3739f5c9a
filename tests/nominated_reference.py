"""RunFilterPluginsWithNominatedPods (framework/runtime/framework.go:1211-1294) as a test reference, built from
oracle parts only (never from the code under test) -- what a context created with {"nominatedPods": "Evaluate"}
must reproduce (include/ksg.h ksg_add_nominated_pod).

The oracle refuses a call in which a pod would see another pod's nomination, so this keeps the nominator in
Python and one oracle context `A` that is never told about nominations.  For a pod p:

* G(p, n): the pods nominated to snapshot node n with priority >= p's and another uid (addGENominatedPods).
* pass 1: every pod of G(p, .) is temporarily added to A, bound to its nominated node under a prefixed uid
  (NodeInfo.AddPodInfo), p is evaluated (no assume), and the pods are removed again.  In the supported class the
  filters that read them (NodeResourcesFit, NodePorts) are node-local, so adding all nominees at once equals adding
  each node's own.
* pass 2: the same evaluation on A as it is.
* a node's status is pass 1's if that is not Success on a node with non-empty G, else pass 2's -- and pass 1
  Success must imply pass 2 Success (asserted: the monotonicity the device's single pass relies on).
* scores never see nominated pods: each plugin of A's score_plugin_mask is run over the feasible list
  (A.run_score_plugin), weighted with the profile's weights and summed; the node is Go's heap.Init + Pop.
* the feasible list is walked in rotated order from the helper's own nextStartNodeIndex, the PreFilterResult subset
  and the percentageOfNodesToScore cut applied as the oracle applies them (sequentially: the walk ends at the
  (K+1)-th feasible node; nextStartNodeIndex advances by the nodes processed).  A always scores every node.
* a pod whose own status.nominatedNodeName is a snapshot node tries that node alone first (evaluateNominatedNode):
  feasible -> (0, node, 1, 1, 0) and nextStartNodeIndex stays.  Such pods carry no matchFields affinity.
* an assume binds the pod in A and ends its nomination (schedule_one.go:1131-1134).
* preemption: A.preempt with G(p, .) temporarily added (nominees have priority >= the preemptor's: never victims).

Only tests/ use this module.
"""
import copy

from ksg.abi import ERROR, NUM_PLUGINS, SKIP, SUCCESS, UNSCHEDULABLE, UNSCHEDULABLE_AND_UNRESOLVABLE
from oracle_binding import oracle
from shim_replay import SCORE_ORDER, CycleEval, enabled_plugins, heap_init_pop, profile_weights

NOM_PREFIX = "nominee~"


def num_feasible_nodes_to_find(pct, num_all):
    """numFeasibleNodesToFind (schedule_one.go:858-884; minFeasibleNodesToFind 100, the adaptive 50 - n / 125)."""
    if num_all < 100:
        return num_all
    p = pct
    if p == 0:
        p = max(50 - num_all // 125, 5)
    if p >= 100:
        return num_all
    return max(num_all * p // 100, 100)


class NominatedReference:
    def __init__(self, cfg, nodes, existing, namespaces=(), objects=()):
        self.cfg = {k: v for k, v in cfg.items() if k not in ("nominatedPods", "device")}
        self.pct = int(self.cfg.pop("percentageOfNodesToScore", 100))
        self.A = oracle(self.cfg)
        for ns in namespaces:
            self.A.upsert_namespace(ns)
        for o in objects:
            self.A.upsert_object(o)
        for n in nodes:
            self.A.add_node(n)
        for p in existing:
            self.A.add_pod(p)
        self.names = self.A.node_names()
        self.index = {n: i for i, n in enumerate(self.names)}
        self.weights = profile_weights(self.cfg)
        self.enabled = set(enabled_plugins(self.cfg))
        self.nominator = {}  # uid -> pod (status.nominatedNodeName set)
        self.next_start = 0
        self.bound = 0
        self.flips = 0  # node statuses so far that only the nominated pods made a failure

    # ---- the nominator ------------------------------------------------------------------------------------------
    def add_nominated_pod(self, pod):
        uid = pod["metadata"]["uid"]
        self.nominator.pop(uid, None)
        if (pod.get("status") or {}).get("nominatedNodeName"):
            self.nominator[uid] = copy.deepcopy(pod)

    def delete_nominated_pod(self, uid):
        self.nominator.pop(uid, None)

    @staticmethod
    def _prio(pod):
        return int(pod["spec"].get("priority") or 0)

    def g(self, pod):
        """G(pod, .): [(nominee, snapshot index)] over every snapshot node."""
        out = []
        for uid, q in sorted(self.nominator.items()):
            ix = self.index.get(q["status"]["nominatedNodeName"], -1)
            if uid != pod["metadata"]["uid"] and self._prio(q) >= self._prio(pod) and ix >= 0:
                out.append((q, ix))
        return out

    def _with_g(self, g, fn):
        """fn() with every pod of g added to A, bound to its nominated node under a prefixed uid."""
        added = []
        try:
            for q, ix in g:
                b = copy.deepcopy(q)
                b["metadata"]["uid"] = NOM_PREFIX + q["metadata"]["uid"]
                b["metadata"]["name"] = NOM_PREFIX + q["metadata"]["name"]
                b["spec"]["nodeName"] = self.names[ix]
                b["status"] = {k: v for k, v in b["status"].items() if k != "nominatedNodeName"}
                self.A.add_pod(b)
                added.append(b["metadata"]["uid"])
            return fn()
        finally:
            for uid in added:
                self.A.remove_pod(uid)

    # ---- one cycle ----------------------------------------------------------------------------------------------
    def evaluate(self, pod):
        """-> (handle on A, the node statuses RunFilterPluginsWithNominatedPods gives, pass 2's evaluation)."""
        plain = copy.deepcopy(pod)
        plain["status"] = {k: v for k, v in (pod.get("status") or {}).items() if k != "nominatedNodeName"}
        h = self.A.compile(plain)
        _, ev2 = self.A.schedule_one(h, assume=False, evaluate=True)
        g = self.g(pod)
        ev = dict(ev2, node_code=list(ev2["node_code"]), node_plugin=list(ev2["node_plugin"]),
                  node_reasons=list(ev2["node_reasons"]))
        if g:
            _, ev1 = self._with_g(g, lambda: self.A.schedule_one(h, assume=False, evaluate=True))
            for i in {ix for _, ix in g}:
                if ev1["node_code"][i] != SUCCESS:
                    self.flips += ev2["node_code"][i] == SUCCESS  # (a node the nominations alone close to the pod)
                    ev["node_code"][i] = ev1["node_code"][i]
                    ev["node_plugin"][i] = ev1["node_plugin"][i]
                    ev["node_reasons"][i] = ev1["node_reasons"][i]
                else:  # the monotonicity the device's single pass relies on
                    assert ev2["node_code"][i] == SUCCESS, (pod["metadata"]["name"], i, ev2["node_code"][i])
        return h, ev, ev2

    def scores(self, h, ev2, feasible):
        """-> (status, {plugin: normalized scores by snapshot index}) over the feasible list, nominated pods unseen."""
        out = {}
        for p in SCORE_ORDER:
            if p not in self.enabled or not (ev2["score_plugin_mask"] >> p & 1):
                continue
            st, _, nrm = self.A.run_score_plugin(h, p, nodes=feasible)
            if st == SKIP:
                continue
            if st != SUCCESS:
                return ERROR, {}
            out[p] = nrm
        return SUCCESS, out

    def schedule(self, pod, assume=True, detail=None):
        """One scheduling cycle of pod -> (status, node index, EvaluatedNodes, FeasibleNodes, TotalScore).
        detail (a dict): filled with the merged evaluation and the scores (evaluation-output comparisons)."""
        h, ev, ev2 = self.evaluate(pod)
        if detail is not None:
            detail.update(ev=ev, feasible=[], norm={}, totals={})
        res = self._cycle(pod, h, ev, ev2, detail)
        self.A.release(h)
        if assume and res[0] == SUCCESS and res[1] >= 0:
            self.assume(pod, res[1])
        return res

    def assume(self, pod, node_index):
        b = copy.deepcopy(pod)
        b["spec"]["nodeName"] = self.names[node_index]
        self.bound += 1
        b["metadata"]["uid"] = pod["metadata"]["uid"] + "#ref" + str(self.bound)
        self.A.add_pod(b)
        self.nominator.pop(pod["metadata"]["uid"], None)

    def _cycle(self, pod, h, ev, ev2, detail):
        n = len(self.names)
        ce = CycleEval(ev)
        if ce.pre_code == UNSCHEDULABLE_AND_UNRESOLVABLE or ce.pre_code == UNSCHEDULABLE:
            return (UNSCHEDULABLE, -1, 0, 0, 0)
        if ce.pre_code != SUCCESS:
            return (ERROR, -1, 0, 0, 0)
        if ce.pre_result is not None and not ce.pre_result:
            return (UNSCHEDULABLE, -1, 0, 0, 0)
        nodes = list(range(n)) if ce.pre_result is None else sorted(ce.pre_result)
        # evaluateNominatedNode: the pod's own nominated node alone first
        nn = self.index.get((pod.get("status") or {}).get("nominatedNodeName") or "", -1)
        nom_failed = -1
        if nn >= 0:
            if ev["node_code"][nn] == SUCCESS:
                return (SUCCESS, nn, 1, 1, 0)
            nom_failed = nn
        # findNodesThatPassFilters: rotated order, the sequential cut
        k_find = num_feasible_nodes_to_find(self.pct, len(nodes))
        feasible, failed, visited = [], 0, len(nodes)
        for i in range(len(nodes)):
            node = nodes[(self.next_start + i) % len(nodes)]
            if ev["node_code"][node] == SUCCESS:
                if len(feasible) + 1 > k_find:
                    visited = i
                    break
                feasible.append(node)
            else:
                failed += 1
        if nom_failed >= 0 and nom_failed not in {nodes[(self.next_start + i) % len(nodes)] for i in range(visited)}:
            failed += 1  # NodeToStatus holds the nominated node's status once
        self.next_start = (self.next_start + len(feasible) + failed) % n
        if detail is not None:
            detail["feasible"] = list(feasible)
        if not feasible:
            return (UNSCHEDULABLE, -1, failed, 0, 0)
        if len(feasible) == 1:
            return (SUCCESS, feasible[0], 1 + failed, 1, 0)
        st, norm = self.scores(h, ev2, feasible)
        if st != SUCCESS:
            return (ERROR, -1, 0, 0, 0)
        totals = [sum(norm[p][node] * self.weights[p] for p in norm) for node in feasible]
        if not any(p in self.enabled for p in SCORE_ORDER):
            totals = [1] * len(feasible)  # no score plugins (schedule_one.go:948-957)
        if detail is not None:
            detail["norm"] = norm
            detail["totals"] = dict(zip(feasible, totals))
        node = heap_init_pop(list(zip(totals, feasible)))
        return (SUCCESS, node, len(feasible) + failed, len(feasible), totals[feasible.index(node)])

    # ---- DefaultPreemption ----------------------------------------------------------------------------------------
    def preempt(self, pod, args):
        """-> (PreemptResult tuple, detail) of A.preempt with G(pod, .) added for the call."""
        h = self.A.compile(pod)
        r, d = self._with_g(self.g(pod), lambda: self.A.preempt(h, args))
        self.A.release(h)
        return r.as_tuple(), d

    def remove_pod(self, uid):
        self.A.remove_pod(uid)

    def add_pod(self, pod):
        self.A.add_pod(pod)


def eval_fields(detail, n):
    """The evaluation output the device must give for the cycle `detail` describes: (node_code, node_plugin,
    node_reasons, score mask over the scored plugins, normalized, weighted and total scores by snapshot index)."""
    ev = detail["ev"]
    norm = [[0] * n for _ in range(NUM_PLUGINS)]
    for p, v in detail["norm"].items():
        for i in detail["feasible"]:
            norm[p][i] = v[i]
    total = [0] * n
    for i, t in detail["totals"].items():
        total[i] = t
    mask = 0
    for p in detail["norm"]:
        mask |= 1 << p
    return ev["node_code"], ev["node_plugin"], ev["node_reasons"], mask, norm, total
