"""Streams for k_sched_same's sampled instance (config "loopSameSampled"): same-template runs whose
nextStartNodeIndex lives on the device -- percentageOfNodesToScore below 100 (0, upstream's adaptive default,
included) or a nominated pod in the batch -- each stream built around one boundary of the cut, of the rotation or of
the routing.  Shared by test_same_sampled_inputs.py (the oracle alone: each stream contains the boundary it claims) and
test_gpu_same_sampled.py.

A stream is same_template_gen's dict: cfg, nodes, bound, batches; a batch is a list of (pod, template) pairs.  The
template is the key of the pod's template when k_sched_same can take the pod, None when only k_sched_loop can, and
NOT_LOOP for a pod no k_sched_loop run holds (ksg_debug_same_pods counts it on neither side).
"""
import functools

import norm_edge_gen as gen
import same_template_gen as st

NOT_LOOP = "<not a loop pod>"
NO_SCORE = {"disabledPlugins": ["TaintToleration", "NodeAffinity", "NodeResourcesFit", "PodTopologySpread",
                                "InterPodAffinity", "NodeResourcesBalancedAllocation", "ImageLocality"],
            # (PodTopologySpread is off, so OpportunisticBatching would act and its signed pods leave the loops)
            "featureGates": {"OpportunisticBatching": False}}


def num_to_find(n, pct):
    """numFeasibleNodesToFind (schedule_one.go:858-884)."""
    if n < 100:
        return n
    if pct == 0:
        pct = max(5, 50 - n // 125)
    return n if pct >= 100 else max(100, n * pct // 100)


def counts(batch, enabled=True, min_run=st.MIN_RUN):
    """(taken, not_taken) of ksg_debug_same_pods for one batch: same_template_gen.dispatch over the loop pods; a pod
    of another path ends the stretches on both sides of it and is counted nowhere."""
    keys = [None if k == NOT_LOOP else k for _, k in batch]
    taken, other = st.dispatch(keys, min_run=min_run, enabled=enabled)
    return taken, other - sum(k == NOT_LOOP for _, k in batch)


def _pct(p, **cfg):
    return dict(cfg, percentageOfNodesToScore=p)


def cut(n, pct, pods=48):
    return st._stream(st._nodes(n), [st._stamp("a", 0, pods, cpu=500)], _pct(pct))


def slots(n):
    return st._stream(st._nodes(n), [st._stamp("a", 0, 24, cpu=500)], _pct(0))


def holes_nodes(n):
    """same_template_gen.holes()'s node pattern over n nodes: five sizes, a NoSchedule taint on every sixth node, every
    ninth unschedulable."""
    nodes = []
    for i in range(n):
        nd = gen.node(i, cpu_milli=(3000, 4500, 7000, 9500, 16000)[i % 5], mem=(8 + i % 7) << 30,
                      taints=[st.NOSCHED] if i % 6 == 2 else None)
        if i % 9 == 4:
            nd["spec"]["unschedulable"] = True
        nodes.append(nd)
    return nodes


def holes():
    return st._stream(holes_nodes(260), [st._stamp("a", 0, 60, cpu=700, mem=900 * gen.MIB)], _pct(45))


def fill():  # 150 nodes that each hold 3 template pods: the cut, then F = K, then F = 99 ... 0; two batches
    return st._stream(st._nodes(150, sizes=(1500,)),
                      [st._stamp("a", 0, 230, cpu=500, mem=gen.MIB), st._stamp("a", 230, 240, cpu=500, mem=gen.MIB)], _pct(10))


def most():  # MostAllocated under a moving window: the best node leaves the window and comes back
    cfg = _pct(10, nodeResourcesFit={"scoringStrategy": {"type": "MostAllocated"}})
    return st._stream(st._nodes(260, sizes=(3000,)), [st._stamp("a", 0, 120, cpu=500, mem=gen.MIB)], cfg)


def ties():  # one score throughout: the pre-order key over the cut list's positions decides alone
    return st._stream(st._nodes(120, sizes=(8000,)), [st._stamp("a", 0, 120, cpu=100)], _pct(10))


def handover():
    """A x 20, a pod of another request (k_sched_loop), A x 20, a pod with a required matchFields name subset (the
    per-pod launches), A x 20, a PodTopologySpread pod (k_agg_loop's sampling instance), A x 20: rot_out passes
    between all four kinds of launch, in both directions."""
    nodes = st._nodes(130)
    sub = gen.pod("sub-0", "a", cpu=300)
    sub["spec"]["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [gen.name_of(nodes[i])]}]}
        for i in range(20, 60)]}}}
    pts = gen.pod("pts-0", "spread", cpu=300)
    pts["spec"]["topologySpreadConstraints"] = [gen.spread(gen.HOSTNAME, "spread", 1)]
    b = (st._stamp("a", 0, 20, cpu=300) + st._stamp("b", 0, 1, cpu=450) + st._stamp("a", 100, 20, cpu=300) +
         [(sub, NOT_LOOP)] + st._stamp("a", 200, 20, cpu=300) + [(pts, NOT_LOOP)] + st._stamp("a", 300, 20, cpu=300))
    return st._stream(nodes, [b], _pct(30))


def noscore():  # no score plugin: DF_NO_SCORE pods stay in k_sched_loop (K = 1)
    return st._stream(st._nodes(130), [[(p, None) for p, _ in st._stamp("a", 0, 24, cpu=500)]], _pct(30, **NO_SCORE))


def nominated():
    """percentageOfNodesToScore 100, one pod of the batch with status.nominatedNodeName: nextStartNodeIndex lives on the
    device for the whole batch; it is carried and never moves."""
    nodes = st._nodes(130)
    b = st._stamp("a", 0, 39, cpu=500)
    nom = gen.pod("nominated-0", "a", cpu=500)
    nom["status"] = {"nominatedNodeName": gen.name_of(nodes[30])}
    b[17:17] = [(nom, NOT_LOOP)]
    return st._stream(nodes, [b], _pct(100))


STREAMS = {
    "cut-100": functools.partial(cut, 100, 0), "cut-101": functools.partial(cut, 101, 0),
    "cut-130": functools.partial(cut, 130, 30),
    "slots-513": functools.partial(slots, st.SCAN_THREADS + 1), "capacity-8192": functools.partial(slots, st.CAPACITY),
    "over-8193": functools.partial(slots, st.CAPACITY + 1),
    "holes-260": holes, "fill-150": fill, "most-260": most, "ties-120": ties, "handover": handover,
    "noscore": noscore, "nominated-at-100": nominated,
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The stream and the oracle's result tuples, batch by batch (computed once, shared, never changed)."""
    from oracle_binding import oracle
    s = STREAMS[name]()
    o = gen.load(oracle(dict(s["cfg"])), s["nodes"], s["bound"])
    want = tuple(tuple(o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p, _ in b) for b in s["batches"])
    o.close()
    return s, want
