"""DefaultPreemption's dry run (default_preemption.go:252-354, preemption.go:174-457) with every filter call going
through RunFilterPluginsWithNominatedPods (framework.go:1211-1294), for the pairs in which the nominated pods move a
count PodTopologySpread or InterPodAffinity reads -- what a context created with {"nominatedPods": "EvaluateAll",
"preemptNominatedPods": "EvaluateAll"} must reproduce in ksg_preempt (include/ksg.h).  Built from
oracle parts only.

The oracle refuses a preemption that sees a nomination, and two of its runs (with and without G) cannot be composed:
which victim is reprieved depends on the combined status of each step.  So the dry run is restated here, and only the
filter verdicts come from the oracle context A:

* the potential nodes come from the two-pass statuses of the failed cycle (NominatedTopologyReference.evaluate);
* per potential node n, in rotated order from the offset: the potential victims (lower priority, NodeInfo.Pods order)
  are removed from A (A.remove_pod); the node must pass; the victims are sorted (MoreImportantPod, stable), split by
  filterPodsWithPDBViolation, and reprieved one at a time (A.add_pod), violating ones first; a victim stays a victim
  when the node no longer passes with it.  Afterwards node n is rebuilt in A exactly as it was;
* "the node passes" is one step of RunFilterPluginsWithNominatedPods on A as the dry run holds it: pass 1 with
  G(p, n) -- node n's nominees only -- added as bound pods (NominatedReference._with_g), node n's status of
  A.schedule_one(h, assume=False, evaluate=True); pass 2, only if pass 1 succeeded, the same without G.  The step's
  status is pass 1's failure, else pass 2's.  The oracle recomputes PreFilter per evaluation, which equals the
  incremental AddPod / RemovePod for both plugins, but for the Skip rule: PreFilter ran once, on the cluster as it
  is, and a plugin that returned Skip runs in neither pass -- a pass-1 InterPodAffinity failure counts as Success
  when InterPodAffinity's PreFilter on A as the call found it returned Skip;
* DryRunPreemption's cut with parallelism 1, candidateList.add's caps, and pickOneNodeForPreemption's five criteria.

NodeInfo.Pods order decides ties of the stable sort; RemovePod moves the last pod into the hole.  The class mirrors
that order per node (`order`) through add_pod / remove_pod / assume and restores it in A after every dry run.

Counters (conditions on a stream's inputs, not measurements):
  closed   nodes whose all-victims-removed check passes pass 2 but fails pass 1 in PodTopologySpread / InterPodAffinity
  granted  nodes whose all-victims-removed check passes pass 1 while pass 2 is an InterPodAffinity affinity failure
  kept     reprieve steps refused by a pass-1 PodTopologySpread / InterPodAffinity failure alone (pass 2 would pass)
  skipped  pass-1 InterPodAffinity failures ignored because InterPodAffinity's PreFilter skipped
  differs  calls whose outcome differs from NominatedReference.preempt (G added everywhere, one pass) and also
           from A.preempt with nothing nominated

Only tests/ use this module.
"""
import calendar
import copy
import random
import time

from ksg.abi import (PREEMPT_NO_CANDIDATES, PREEMPT_NOT_ELIGIBLE, PREEMPT_OK, SKIP, SUCCESS, UNSCHEDULABLE,
                     UNSCHEDULABLE_AND_UNRESOLVABLE)
from nominated_reference import NominatedReference
from nominated_topology_reference import (HOST, IPA, PTS, R_IPA_AFFINITY, ZONE, NominatedTopologyReference, bound,
                                          labelled, pod_affinity, spread)
from nominator_scenario import node as plain_node, pod as plain_pod

PREEMPT_ALL = {"nominatedPods": "EvaluateAll", "preemptNominatedPods": "EvaluateAll"}
NOW = 1704153600 * 10 ** 9  # past every start time of the generators below


def start_ns(pod, now):
    """GetPodStartTime: status.startTime, or the call's clock."""
    t = (pod.get("status") or {}).get("startTime")
    if not t:
        return now
    return calendar.timegm(time.strptime(t, "%Y-%m-%dT%H:%M:%SZ")) * 10 ** 9


def selector_matches(sel, labels):
    """metav1.LabelSelector against a label map (matchLabels and matchExpressions In / NotIn / Exists / DoesNotExist)."""
    for k, v in (sel.get("matchLabels") or {}).items():
        if labels.get(k) != v:
            return False
    for e in sel.get("matchExpressions") or []:
        op, k, vals = e["operator"], e["key"], e.get("values") or []
        ok = {"In": k in labels and labels[k] in vals, "NotIn": k not in labels or labels[k] not in vals,
              "Exists": k in labels, "DoesNotExist": k not in labels}[op]
        if not ok:
            return False
    return True


def terminating_by_preemption(pod):
    if not pod["metadata"].get("deletionTimestamp"):
        return False
    return any(c.get("type") == "DisruptionTarget" and c.get("status") == "True"
               and c.get("reason") == "PreemptionByScheduler" for c in (pod.get("status") or {}).get("conditions") or [])


class NominatedPreemptReference(NominatedTopologyReference):
    def __init__(self, cfg, nodes, existing, namespaces=(), objects=()):
        cfg = {k: v for k, v in cfg.items() if k != "preemptNominatedPods"}
        super().__init__(cfg, nodes, existing, namespaces, objects)
        self.order = {name: [] for name in self.names}  # node -> uids in NodeInfo.Pods order
        self.pods = {}                                  # uid -> the bound pod
        for p in existing:
            self._track(p)
        # the dry run's own counters (evaluate() keeps counting the failed cycles in closed / granted / skipped)
        self.dry = {"closed": 0, "granted": 0, "kept": 0, "skipped": 0, "differs": 0}

    # ---- the cluster, mirrored -----------------------------------------------------------------------------------
    def _track(self, pod):
        node = pod["spec"].get("nodeName")
        if node in self.order:
            self.order[node].append(pod["metadata"]["uid"])
            self.pods[pod["metadata"]["uid"]] = copy.deepcopy(pod)

    def add_pod(self, pod):
        self.A.add_pod(pod)
        self._track(pod)

    def remove_pod(self, uid):
        self.A.remove_pod(uid)
        p = self.pods.pop(uid, None)
        if p is not None:  # NodeInfo.RemovePod: the last pod moves into the hole
            o = self.order[p["spec"]["nodeName"]]
            o[o.index(uid)] = o[-1]
            o.pop()

    def assume(self, pod, node_index):
        b = copy.deepcopy(pod)
        b["spec"]["nodeName"] = self.names[node_index]
        self.bound += 1
        b["metadata"]["uid"] = pod["metadata"]["uid"] + "#ref" + str(self.bound)
        self.add_pod(b)
        self.nominator.pop(pod["metadata"]["uid"], None)

    def _rebuild(self, name):
        for uid in self.order[name]:
            self.A.remove_pod(uid)
        for uid in self.order[name]:
            self.A.add_pod(self.pods[uid])

    # ---- one filter call of SelectVictimsOnNode ------------------------------------------------------------------------
    def _status(self, h, i, g=()):
        _, ev = self._with_g(list(g), lambda: self.A.schedule_one(h, assume=False, evaluate=True))
        return ev["node_code"][i], ev["node_plugin"][i], ev["node_reasons"][i]

    def _step(self, h, i, gi, ipa_skipped):
        """-> (passes, pass 1 failed in PodTopologySpread / InterPodAffinity, pass 1's status, pass 2's or None)."""
        if not gi:
            st0 = self._status(h, i)
            return st0[0] == SUCCESS, False, None, st0
        st1 = self._status(h, i, gi)
        if st1[0] != SUCCESS and st1[1] == IPA and ipa_skipped:
            self.dry["skipped"] += 1
            st1 = (SUCCESS, 0, 0)
        if st1[0] != SUCCESS:
            return False, st1[1] in (PTS, IPA), st1, None
        st0 = self._status(h, i)
        return st0[0] == SUCCESS, False, st1, st0

    def _select_victims(self, h, pod, i, gi, pdbs, now, ipa_skipped):
        """SelectVictimsOnNode on snapshot node i -> (victim uids in order, numPDBViolations) or None."""
        name = self.names[i]
        prio = self._prio(pod)
        pot = [uid for uid in self.order[name] if self._prio(self.pods[uid]) < prio]
        if not pot:
            return None
        gone = set()  # the pods of node i that A lacks right now

        def take(uid):
            self.A.remove_pod(uid)
            gone.add(uid)

        def give(uid):
            self.A.add_pod(self.pods[uid])
            gone.discard(uid)
        try:
            for uid in pot:
                take(uid)
            ok, topo1, st1, st0 = self._step(h, i, gi, ipa_skipped)
            if gi and topo1 and self._status(h, i)[0] == SUCCESS:
                self.dry["closed"] += 1
            if gi and st1 is not None and st1[0] == SUCCESS and st0 is not None and st0[0] != SUCCESS \
                    and st0[1] == IPA and st0[2] & R_IPA_AFFINITY:
                self.dry["granted"] += 1
            if not ok:
                return None
            key = lambda uid: (-self._prio(self.pods[uid]), start_ns(self.pods[uid], now))  # noqa: E731
            pot.sort(key=key)  # stable: equal keys keep NodeInfo.Pods order
            allowed = [int((b.get("status") or {}).get("disruptionsAllowed", 0)) for b in pdbs]
            violating, non_violating = [], []
            for uid in pot:
                p = self.pods[uid]
                labels = p["metadata"].get("labels") or {}
                v = False
                if labels:
                    for k, b in enumerate(pdbs):
                        sel = (b.get("spec") or {}).get("selector")
                        if sel is None or not (sel.get("matchLabels") or sel.get("matchExpressions")):
                            continue  # nil: Nothing; empty: matches nothing here
                        bns = (b.get("metadata") or {}).get("namespace") or "default"
                        if bns != p["metadata"].get("namespace", "default") or not selector_matches(sel, labels):
                            continue
                        if p["metadata"]["name"] in ((b.get("status") or {}).get("disruptedPods") or {}):
                            continue
                        allowed[k] -= 1
                        if allowed[k] < 0:
                            v = True
                (violating if v else non_violating).append(uid)
            victims, nviol = [], 0
            for group in (violating, non_violating):
                for uid in group:
                    give(uid)
                    ok, topo1, _, _ = self._step(h, i, gi, ipa_skipped)
                    if ok:
                        continue
                    if topo1 and self._status(h, i)[0] == SUCCESS:
                        self.dry["kept"] += 1
                    take(uid)
                    victims.append(uid)
                    nviol += group is violating
            if violating and non_violating:
                victims.sort(key=key)
            if not victims:
                return None
            return victims, nviol
        finally:
            # put node i back in A as NodeInfo.Pods held it
            for uid in sorted(gone):
                self.A.add_pod(self.pods[uid])
            self._rebuild(name)

    # ---- DefaultPreemption PostFilter ------------------------------------------------------------------------------------
    def preempt(self, pod, args):
        """-> (PreemptResult tuple, detail) in the shape of A.preempt with listCandidates."""
        args = dict(args or {})
        now = int(args.get("now", time.time_ns()))
        pct = int(args.get("minCandidateNodesPercentage", 10))
        absn = int(args.get("minCandidateNodesAbsolute", 100))
        listing = bool(args.get("listCandidates"))
        pdbs = list(args.get("pdbs") or [])
        out = self._preempt(pod, now, pct, absn, listing, pdbs, int(args.get("offset", 0)), bool(args.get("allNodes")))
        # `differs`: against G added everywhere in one pass, and against no nominations at all
        one_pass = NominatedReference.preempt(self, pod, args)
        hp = self.A.compile(pod)
        r0, d0 = self.A.preempt(hp, args)
        self.A.release(hp)
        if out != one_pass and out != (r0.as_tuple(), d0):
            self.dry["differs"] += 1
        return out

    def _preempt(self, pod, now, pct, absn, listing, pdbs, offset_in, all_nodes):
        n = len(self.names)
        if pod["spec"].get("preemptionPolicy") == "Never":
            return ((UNSCHEDULABLE, PREEMPT_NOT_ELIGIBLE, -1, 0, 0, 0, 0),
                    {"message": "not eligible due to preemptionPolicy=Never.", "candidates": []})
        h, ev, _ = self.evaluate(pod)  # the failed cycle's two-pass NodeToStatus
        try:
            code = ev["node_code"]
            nn = self.index.get((pod.get("status") or {}).get("nominatedNodeName") or "", -1)
            if nn >= 0 and code[nn] != UNSCHEDULABLE_AND_UNRESOLVABLE:
                for uid in self.order[self.names[nn]]:
                    p = self.pods[uid]
                    if self._prio(p) < self._prio(pod) and terminating_by_preemption(p):
                        return ((UNSCHEDULABLE, PREEMPT_NOT_ELIGIBLE, -1, 0, 0, 0, 0),
                                {"message": "not eligible due to a terminating pod on the nominated node.",
                                 "candidates": []})
            pot = [i for i in range(n) if all_nodes or code[i] == UNSCHEDULABLE]
            P = len(pot)
            nv, vl = [], []
            offset = ncand = 0
            if P > 0 and ev["prefilter_code"] == SUCCESS:
                offset = offset_in % P
                ncand = min(max(P * pct // 100, absn), P)
                by_node = {}
                for q, ix in self.g(pod):
                    by_node.setdefault(ix, []).append((q, ix))
                ipa_skipped = bool(by_node) and self.A.run_filter_plugin(h, IPA)[0] == SKIP
                for k in range(P):
                    i = pot[(offset + k) % P]
                    v = self._select_victims(h, pod, i, by_node.get(i, ()), pdbs, now, ipa_skipped)
                    if v is None:
                        continue
                    lst = nv if v[1] == 0 else vl
                    if len(lst) < ncand:
                        lst.append((i, v[0], v[1]))
                    if nv and len(nv) + len(vl) >= ncand:
                        break
        finally:
            self.A.release(h)
        cands = nv + vl
        best = -1
        if len(cands) == 1:
            best = 0
        elif cands:
            prio = lambda uid: self._prio(self.pods[uid])  # noqa: E731

            def earliest(vs):  # util.GetEarliestPodStartTime
                t, mp = start_ns(self.pods[vs[0]], now), prio(vs[0])
                for uid in vs:
                    if prio(uid) == mp:
                        t = min(t, start_ns(self.pods[uid], now))
                    elif prio(uid) > mp:
                        mp, t = prio(uid), start_ns(self.pods[uid], now)
                return t
            fs = [lambda c: -c[2], lambda c: -prio(c[1][0]), lambda c: -sum(prio(u) + 2 ** 31 for u in c[1]),
                  lambda c: -len(c[1]), lambda c: earliest(c[1])]
            alive = list(range(len(cands)))
            for f in fs:
                mx = max(f(cands[k]) for k in alive)
                alive = [k for k in alive if f(cands[k]) == mx]
                if len(alive) == 1:
                    break
            best = alive[0]
        msg = ""
        if best >= 0:
            res = (SUCCESS, PREEMPT_OK, cands[best][0], P, len(cands), len(cands[best][1]), cands[best][2])
        else:
            res = (UNSCHEDULABLE, PREEMPT_NO_CANDIDATES, -1, P, len(cands), 0, 0)
            msg = f"0/{n} nodes are available: preemption is not helpful for scheduling."
        detail = {"offset": offset, "numCandidates": ncand, "potential": P, "message": msg,
                  "candidates": [{"node": self.names[i], "numPDBViolations": nviol, "victims": list(vs)}
                                 for i, vs, nviol in cands] if listing else [],
                  "selected": self.names[cands[best][0]] if best >= 0 else None,
                  "victims": list(cands[best][1]) if best >= 0 else []}
        return res, detail

    def counters(self):
        return dict(self.dry)


# ---- hand-computed cases ------------------------------------------------------------------------------------------
ARGS = {"offset": 0, "now": NOW, "listCandidates": True, "minCandidateNodesPercentage": 100,
        "minCandidateNodesAbsolute": 100}


def low(name, node, cpu="3", sec=0, **labels):
    p = bound(name, node, **labels)
    p["spec"]["containers"][0]["resources"]["requests"]["cpu"] = cpu
    p["status"]["startTime"] = f"2024-01-01T00:00:{sec:02d}Z"
    return p


def zoned(n, zones, cpu="4"):
    nodes = [plain_node(f"n{k}", cpu=cpu) for k in range(n)]
    for k, nd in enumerate(nodes):
        nd["metadata"]["labels"][ZONE] = f"z{k % zones}"
    return nodes


def hand_cases():
    """-> [(name, nodes, existing, nominees, preemptor, args, result tuple, {node: victims} of every candidate,
    selected node or None, counters that must be reached)].  Nodes have 4 CPUs (n0, n1, ... in zones z0, z1, z0, ...);
    the preemptor has priority 50 and asks for 2 CPUs, the low pods priority 0, the nominees priority 100."""
    nom = lambda name, node, cpu="100m", **labels: labelled(  # noqa: E731
        plain_pod(name, prio=100, cpu=cpu, nominated=node), **labels)
    pre = lambda **labels: labelled(plain_pod("pre", prio=50, cpu="2"), **labels)  # noqa: E731
    cases = []
    # 1. zone spread over app=web, maxSkew 1.  A priority-100 web pod on n0 (z0) and on n1 (z1), and a 3-CPU
    # priority-0 pod on each: both nodes fail NodeResourcesFit in the cycle.  n0 with f0 gone: z0 = 1, minimum 1:
    # 1 + 1 - 1 fits (pass 2); with the nominee (app=web) added z0 = 2: 2 + 1 - 1 > 1 -- closed although every victim
    # is gone.  n1 has no nominee: f1 goes, the node passes, f1 does not fit back.
    cases.append(("closes", zoned(2, 2), [low("w0", "n0", cpu="500m", app="web"), low("f0", "n0", app="x"),
                                          low("w1", "n1", cpu="500m", app="web"), low("f1", "n1", app="x")],
                  [nom("nom", "n0", app="web")], spread(pre(app="web"), ZONE, "web"), ARGS,
                  (SUCCESS, PREEMPT_OK, 1, 2, 1, 1, 0), {"n1": ["f1"]}, "n1", {"closed": 1}))
    for p in cases[-1][2]:
        if p["metadata"]["name"].startswith("w"):
            p["spec"]["priority"] = 100
    # 2. required affinity to app=db over the hostname; only the nominee on n0 is app=db.  n0 and n1 are full.
    # Pass 1 on n0 passes with the nominee, pass 2 fails everywhere (UnschedulableAndUnresolvable): the failed
    # cycle leaves no potential node; with allNodes n0's check passes pass 1 and fails pass 2 -- no candidate.
    cases.append(("granted-only", zoned(2, 2), [low("f0", "n0", app="x"), low("f1", "n1", app="x")],
                  [nom("nom", "n0", app="db")], pod_affinity(pre(app="web"), "podAffinity", HOST, "db"),
                  dict(ARGS, allNodes=True), (UNSCHEDULABLE, PREEMPT_NO_CANDIDATES, -1, 2, 0, 0, 0), {}, None,
                  {"granted": 1}))
    # 3. hostname spread over app=web, maxSkew 1.  Every node holds a 2.5-CPU priority-0 pod (it must go), n1 and n2 a
    # priority-100 web pod, n0 a priority-0 web pod v.  n0 with f0 and v gone: counts 0 / 1 / 1; with the nominee
    # (app=web) n0 = 1 and the minimum 1: passes both passes.  f0 does not fit back.  v back: pass 2 sees n0 = 1,
    # minimum 1: 1 + 1 - 1 fits -- without the nominee v is reprieved; pass 1 sees n0 = 2, the minimum 1 (the others):
    # 2 + 1 - 1 > 1 -- v stays a victim.  n1 and n2 give up their filler alone and win on the summed priorities; their
    # victims started at the same second, so the first candidate, n1, is selected.
    ex = [low("f0", "n0", cpu="2500m", app="x"), low("v", "n0", cpu="500m", sec=1, app="web"),
          low("f1", "n1", cpu="2500m", app="x"), low("f2", "n2", cpu="2500m", app="x"),
          low("k1", "n1", cpu="500m", app="web"), low("k2", "n2", cpu="500m", app="web")]
    for p in ex:
        if p["metadata"]["name"].startswith("k"):
            p["spec"]["priority"] = 100
    cases.append(("keeps", zoned(3, 3), ex, [nom("nom", "n0", app="web")], spread(pre(app="web"), HOST, "web"), ARGS,
                  (SUCCESS, PREEMPT_OK, 1, 3, 3, 1, 0), {"n0": ["f0", "v"], "n1": ["f1"], "n2": ["f2"]}, "n1",
                  {"kept": 1}))
    # 4. the nominee on n0 has a required anti-affinity term against app=web (the preemptor); no existing pod has one
    # and the preemptor has no term: InterPodAffinity's PreFilter skipped, the nominee's term is never checked and n0
    # is a candidate like n1.  All criteria tie but the last: n1's victim started later.
    hater = pod_affinity(nom("nom", "n0", app="db"), "podAntiAffinity", HOST, "web")
    cases.append(("skipped", zoned(2, 2), [low("f0", "n0", app="x"), low("f1", "n1", sec=5, app="x")], [hater],
                  pre(app="web"), ARGS, (SUCCESS, PREEMPT_OK, 1, 2, 2, 1, 0), {"n0": ["f0"], "n1": ["f1"]}, "n1",
                  {"skipped": 1}))
    return cases


NAMESPACES2 = [{"metadata": {"name": "default"}}, {"metadata": {"name": "team"}}]


# ---- streams --------------------------------------------------------------------------------------------------------
SIZES = [9, 130, 257]
N_CALLS = 14


def stream_nodes(n):
    """n nodes of 4 CPUs in 3 zones, hostname-labelled."""
    nodes = zoned(n, 3)
    for k, nd in enumerate(nodes):
        nd["metadata"]["name"] = f"n{k:03d}"
        nd["metadata"]["labels"][HOST] = f"n{k:03d}"
    return nodes


def stream_existing(rng, nodes):
    """Every node full: a 2.5-CPU priority-0 filler, and one to three 400m pods of priority 0 / 10 / 100 labelled
    app=web / db / cache, some with a required anti-affinity term against app=web."""
    out = []
    for k, nd in enumerate(nodes):
        name = nd["metadata"]["name"]
        out.append(low(f"f{k}", name, cpu="2500m", sec=rng.randrange(60), app="x"))
        for j in range(rng.randint(1, 3)):
            p = low(f"s{k}-{j}", name, cpu="400m", sec=rng.randrange(60), app=rng.choice(["web", "web", "db", "cache"]))
            p["spec"]["priority"] = rng.choice([0, 0, 10, 100])
            if rng.random() < 0.05:
                pod_affinity(p, "podAntiAffinity", HOST, "web")
            out.append(p)
    return out


def stream_nominees(rng, names):
    """Nominees of priorities 100 / 50 / 10 (the preemptors have 50) on snapshot indices 0 (two of them), 255, 256, the
    last one, a name outside the snapshot and random nodes; every fourth one with a required anti-affinity term."""
    n = len(names)
    where = [0, 0, 255, 256, n - 1, -1] + [rng.randrange(n) for _ in range(max(4, n // 6))]
    out = []
    for k, ix in enumerate(where):
        if ix >= n:
            ix = rng.randrange(n)
        q = labelled(plain_pod(f"nom{k}", prio=[100, 50, 10][k % 3], cpu="100m",
                               nominated=names[ix] if ix >= 0 else "no-such-node"),
                     app=["web", "db", "web", "cache"][k % 4])
        if k % 4 == 3:
            pod_affinity(q, "podAntiAffinity", rng.choice([HOST, ZONE]), "web")
        out.append(q)
    return out


def stream_preemptor(rng, k, family):
    p = labelled(plain_pod(f"pre{k}", prio=50, cpu="2"), app=rng.choice(["web", "db"]))
    kind = k % 5 if family == "directed" else rng.randrange(6)
    if kind == 0:
        spread(p, HOST, "web", max_skew=rng.choice([1, 2]))
    elif kind == 1:
        spread(p, ZONE, "web", max_skew=rng.choice([1, 2, 3]))
    elif kind == 2:
        key = HOST if family == "directed" else rng.choice([HOST, ZONE])
        pod_affinity(p, "podAffinity", key, rng.choice(["db", "cache"]))
    elif kind == 3:
        pod_affinity(p, "podAntiAffinity", rng.choice([HOST, ZONE]), rng.choice(["db", "cache"]))
    elif kind == 4:
        spread(p, HOST, "web")
        pod_affinity(p, "podAffinity", HOST, "db")
    return p  # kind 5: a plain pod (the nominees' anti-affinity terms may still mark it)


def stream_args(rng, k, n):
    return {"offset": rng.randrange(4 * n), "now": NOW, "listCandidates": True, "allNodes": k % 3 == 2,
            "minCandidateNodesPercentage": rng.choice([10, 50, 100]),
            "minCandidateNodesAbsolute": rng.choice([1, 3, 100]),
            "pdbs": [{"metadata": {"namespace": "default"}, "spec": {"selector": {"matchLabels": {"app": "web"}}},
                      "status": {"disruptionsAllowed": rng.randrange(2)}}] if k % 4 == 1 else []}


def stream_case(family, n_nodes):
    rng = random.Random((9100 if family == "directed" else 9200) + n_nodes)
    nodes = stream_nodes(n_nodes)
    existing = stream_existing(rng, nodes)
    return rng, nodes, existing


def stream_reference(family, n_nodes):
    """-> (nodes, existing, nominees, [(preemptor, args)], [(result tuple, detail)], counters).  Nothing is actuated:
    every call sees the same cluster and nominator."""
    rng, nodes, existing = stream_case(family, n_nodes)
    ref = NominatedPreemptReference({}, nodes, existing, NAMESPACES2)
    noms = stream_nominees(rng, ref.names)
    for q in noms:
        ref.add_nominated_pod(q)
    calls, want = [], []
    for k in range(N_CALLS):
        pod = stream_preemptor(rng, k, family)
        args = stream_args(rng, k, n_nodes)
        calls.append((pod, args))
        want.append(ref.preempt(pod, args))
    return nodes, existing, noms, calls, want, ref.counters()
