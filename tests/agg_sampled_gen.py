"""Inputs for sampled pods inside k_agg_loop (percentageOfNodesToScore < 100 for PodTopologySpread / InterPodAffinity
pods; DESIGN.md §4.5 "Inside k_agg_loop"): a cluster whose cut feasible list differs from its full feasible list in
every quantity the loop's kept-list exchange carries, the pod streams, and the oracle's results for them.

The cluster.  Two or three large zones and one rare zone of 3 or 4 nodes.  The snapshot list goes round the zones, so
the rare zone's nodes sit at its front: a rotation start past them with a cut before the wrap keeps none of them.
Only they carry the extremes of what NormalizeScore and PodTopologySpread's PreScore reduce over the feasible list:

* two PreferNoSchedule taints (some large-zone nodes carry one): the TaintToleration maximum is 2 with a rare node
  kept and 1 without, so the one-taint nodes score 50 or 0;
* the label tier=gold, weight 80, beside disk=ssd, weight 20, which some large-zone nodes carry too: the
  NodeAffinity maximum is 100 or 20, so the ssd nodes score 20 or 100;
* three app=hi pods (zone-keyed preferred affinity, weight 10; a large zone holds one) and two app=lo pods on one
  rare node (hostname-keyed preferred anti-affinity, weight 50; one large-zone node holds one): raw InterPodAffinity
  is in [-70, 30] with the rare zone and within [-50, 10] without;
* the zone value "rare" itself: a zone-keyed ScheduleAnyway constraint sees one topology domain more with a rare node
  kept.

Every ninth large-zone node carries a NoSchedule taint no pod tolerates (failures inside the processed range, and the
nodeTaintsPolicy of the hostname spread), and 40 nodes carry pool=small (pods selecting it have F <= K: no cut).

reference() runs the oracle pod by pod with evaluation output and is shared by the CPU test of the input conditions
(tests/test_agg_sampled_inputs.py) and the GPU tests (tests/test_gpu_agg_sampled.py)."""
import functools

from ksg.objects import NodeW, PodW
from oracle_binding import oracle

HOST, ZONE = "kubernetes.io/hostname", "topology.kubernetes.io/zone"
NSS = [{"metadata": {"name": "default"}}]
NO_SCORE = {"disabledPlugins": ["TaintToleration", "NodeAffinity", "NodeResourcesFit", "PodTopologySpread",
                                "InterPodAffinity", "NodeResourcesBalancedAllocation", "ImageLocality"],
            # (PodTopologySpread is off, so OpportunisticBatching would act and its signed pods leave the loops)
            "featureGates": {"OpportunisticBatching": False}}
# context keys the oracle does not take
LOOP_KEYS = ("loopUnit", "persistentLoop", "aggLoop", "aggLoopDebug", "aggLoopSampled", "loopWorkgroups",
             "pipelineFirstChunk", "device")
BIG = 64 * 256 + 6  # 65 node blocks: the instances that sweep more than one round of 64 workgroups
WG = 512            # node slots of one k_agg_loop workgroup


def prefer_no(key):
    return {"key": key, "value": "x", "effect": "PreferNoSchedule"}


def cluster(n, zones=3, rare=3):
    """(nodes, bound pods).  The rare zone's nodes are added so that the zone round-robin puts them at indices
    zones, 2 * zones + 1, ... of the snapshot list (asserted on the oracle's list by the CPU test)."""
    nodes, large = [], 0
    names = {"rare": [], "large": []}
    for k in range(n):
        name = f"n{k:05d}"
        w = NodeW(name).label(HOST, name).capacity({"cpu": "64", "memory": "256Gi", "pods": "500"})
        if k % (zones + 1) == zones and len(names["rare"]) < rare:
            w.label(ZONE, "rare").label("tier", "gold").label("disk", "ssd").taints([prefer_no("a"), prefer_no("b")])
            names["rare"].append(name)
        else:
            w.label(ZONE, f"z{large % zones}")
            if large % 7 == 3:
                w.label("disk", "ssd")
            if large % 5 == 2:
                w.taints([prefer_no("a")])
            elif large % 9 == 4:
                w.taints([{"key": "dedicated", "value": "x", "effect": "NoSchedule"}])
            if large % max(n // 40, 1) == 1:
                w.label("pool", "small")
            names["large"].append(name)
            large += 1
        nodes.append(w.obj())
    r, lg = names["rare"], names["large"]
    bound = []

    def bind(name, app, node):
        bound.append(PodW(name, uid=name).label("app", app).container(image="i", requests={"cpu": "100m"})
                     .node(node).obj())
    for k in range(3):
        bind(f"hi{k}", "hi", r[k % len(r)])
    bind("hi-large", "hi", lg[0])  # zone z0: one app=hi pod
    bind("lo0", "lo", r[1])
    bind("lo1", "lo", r[1])
    bind("lo-large", "lo", lg[1])
    for k in range(3):  # what the required affinity template follows: one app=db pod per large zone
        bind(f"db{k}", "db", lg[2 + k])
    return nodes, bound


# ---- pod templates ---------------------------------------------------------------------------------------------
def sel(app):
    return {"matchLabels": {"app": app}}


def base(name, app, cpu="200m", ipa=True):
    """Every template scores the rare zone's extremes: the preferred node-affinity terms and (ipa) the preferred
    (anti-)affinity terms; no pod tolerates a taint."""
    p = (PodW(name, uid=name).label("app", app).container(image="i", requests={"cpu": cpu})
         .node_affinity_preferred([(80, {"matchExpressions": [{"key": "tier", "operator": "In", "values": ["gold"]}]}),
                                   (20, {"matchExpressions": [{"key": "disk", "operator": "In", "values": ["ssd"]}]})]))
    return p.pod_affinity_preferred(10, ZONE, sel("hi")).pod_affinity_preferred(50, HOST, sel("lo"), anti=True) if ipa else p


def t_anti(name, soft):  # a required anti-affinity term that matches nothing
    p = base(name, "web").pod_affinity(HOST, sel("nothing"), anti=True)
    return (p.spread(2, ZONE, "ScheduleAnyway", sel("web")).spread(1, HOST, "ScheduleAnyway", sel("web")) if soft else p).obj()


def t_zone(name, soft):  # zone-keyed DoNotSchedule spread (shared counts)
    p = base(name, "zs").spread(2, ZONE, "DoNotSchedule", sel("zs"))
    return (p.spread(1, ZONE, "ScheduleAnyway", sel("web")) if soft else p).obj()


def t_hostdns(name, soft):  # hostname spread honouring node affinity and taints: node-local minima ("unfolded")
    return base(name, "hs").spread(1, HOST, "DoNotSchedule", sel("hs"), node_affinity_policy="Honor",
                                   node_taints_policy="Honor").obj()


def t_aff(name, soft):  # required affinity to the app=db pods' zones (every large zone; not the rare one)
    p = base(name, "follow").pod_affinity(ZONE, sel("db"))
    return (p.spread(3, HOST, "ScheduleAnyway", sel("follow")) if soft else p).obj()


def t_solo(name, soft):  # one per node
    return base(name, "solo").pod_affinity(HOST, sel("solo"), anti=True).obj()


def t_nowhere(name, soft):  # fits nowhere: F = 0
    p = base(name, "web", cpu="1000").pod_affinity(HOST, sel("nothing"), anti=True)
    return (p.spread(2, ZONE, "ScheduleAnyway", sel("web")).spread(1, HOST, "ScheduleAnyway", sel("web")) if soft else p).obj()


def t_small(name, soft):  # the pool=small nodes only: F <= K, no cut
    p = base(name, "web").pod_affinity(HOST, sel("nothing"), anti=True).node_selector({"pool": "small"})
    return (p.spread(1, HOST, "ScheduleAnyway", sel("web")) if soft else p).obj()


STREAMS = ("same", "three", "five")


def stream(kind, soft, n_pods=96):
    """same: one template repeated (the same-template shortcut); three: three templates in turn, one of them the
    hostname DoNotSchedule spread; five: five templates in a fixed irregular order (template-cache evictions happen
    with more than the cache's slots in flight: the unplaceable and the pool=small pods add two more).  In every
    stream pods that fit nowhere and pods with F <= K stand between cut pods."""
    turn = {"same": [t_anti], "three": [t_anti, t_zone, t_hostdns],
            "five": [t_anti, t_hostdns, t_zone, t_aff, t_solo, t_zone, t_anti, t_solo, t_aff, t_hostdns, t_anti]}[kind]
    pods = []
    for k in range(n_pods):
        if k % 16 == 5:
            mk = t_nowhere
        elif k % 16 in (9, 10):
            mk = t_small
        else:
            mk = turn[k % len(turn)]
        pods.append(mk(f"{kind}-{k}", soft))
    return pods


# ---- the oracle, pod by pod ------------------------------------------------------------------------------------
def fill(b, nodes, bound, nss=NSS):
    for ns in nss:
        b.upsert_namespace(ns)
    for n in nodes:
        b.add_node(n)
    for p in bound:
        b.add_pod(p)
    return b


def oracle_cfg(cfg):
    return {k: v for k, v in cfg.items() if k not in LOOP_KEYS}


class Cycle:
    """One pod's cycle in the oracle: its result tuple, nextStartNodeIndex before it, and the kept nodes (the
    feasible list: the nodes with a TotalScore in the evaluation output, or the only feasible node)."""

    def __init__(self, result, start, kept, n):
        self.result, self.start, self.kept, self.n = result, start, kept, n
        self.status, self.node, self.evaluated, self.feasible, self.total = result

    @property
    def placed(self):
        return self.status == 0 and self.node >= 0

    @property
    def cut(self):  # findNodesThatPassFilters stopped early
        return self.placed and self.evaluated < self.n

    @property
    def end(self):  # the (K+1)-th feasible node, where it stopped
        return (self.start + self.evaluated) % self.n

    @property
    def wraps(self):  # the processed range runs past the end of the list
        return self.cut and self.start + self.evaluated > self.n


def run_oracle(cfg, nodes, bound, pods, o=None):
    """[Cycle] of pods through one oracle context (a new one unless given), each assumed before the next."""
    o = o or fill(oracle(oracle_cfg(cfg)), nodes, bound)
    n = o.num_nodes()
    # nextStartNodeIndex is not exported: it starts at 0 and advances by processedNodes, which is EvaluatedNodes
    # for every pod without a nominated node (schedule_one.go:686-687; FitError: the failed nodes, all of them)
    start = getattr(o, "_start", 0)
    out = []
    for p in pods:
        r, ev = o.schedule_one(o.compile(p), assume=True, evaluate=True)
        t = r.as_tuple()
        if t[0] == 0 and t[3] == 1:
            kept = [t[1]]
        elif t[0] == 0:
            kept = [i for i in range(n) if ev["node_code"][i] == 0 and ev["total_scores"][i] != 0]
            assert len(kept) == t[3], (len(kept), t)  # every kept node has a TotalScore > 0 here
        else:
            kept = []
        out.append(Cycle(t, start, kept, n))
        start = (start + t[2]) % n
    o._start = start
    return out, o


# ---- the cases the GPU tests run; the CPU test states the conditions on each ------------------------------------
SHAPES = {  # name: (nodes, zones, rare nodes, extra context config) -- tests/test_gpu_diagnosis_agg.py's sizes
    "9": (9, 2, 3, {}),                                   # N < 100: the rotation is carried, no list is cut
    "130": (130, 2, 3, {}),                               # K = 100, one workgroup
    "257": (257, 3, 4, {}),                               # two workgroups, the second with one node
    "600": (600, 2, 3, {}),
    "600-one-workgroup": (600, 2, 3, {"loopWorkgroups": 1}),  # a workgroup owns two node blocks and a part
    "big": (BIG, 3, 4, {}),
}


@functools.lru_cache(maxsize=None)
def shape_cluster(shape):
    n, zones, rare, _ = SHAPES[shape]
    return cluster(n, zones, rare)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, soft, pct, no_score=False, n_pods=96):
    """(context config, nodes, bound pods, pods, [Cycle]) of one stream on one shape."""
    nodes, bound = shape_cluster(shape)
    cfg = dict(SHAPES[shape][3], percentageOfNodesToScore=pct, **(NO_SCORE if no_score else {}))
    pods = stream(kind, soft, n_pods)
    want, o = run_oracle(cfg, nodes, bound, pods)
    o.close()
    return cfg, nodes, bound, pods, want


def rare_indices(names, nodes):
    """Snapshot indices (names: a backend's node_names()) of the rare zone's nodes."""
    rare = {n["metadata"]["name"] for n in nodes if n["metadata"]["labels"][ZONE] == "rare"}
    return sorted(i for i, name in enumerate(names) if name in rare)
