"""Streams for k_sched_same's carry (config "loopSameCarry"): batches large enough for the chunked
pipeline, so that consecutive k_sched_same launches of one batch hand their cached state on, each stream built around
one edge of the carry: a launch of another kind between two runs, a node count at one of the kernel's boundaries, a
sampled run whose cut list changes across a launch boundary, a batch boundary with a cluster event on it.  Shared by
test_same_carry_inputs.py (the oracle alone: each stream contains what it claims) and test_gpu_same_carry.py.

A stream is same_template_gen's dict: cfg, nodes, bound, batches, and optionally
  events  events[k] is the list of steps applied to both backends before batch k (apply_events),
  native  config keys only the product library reads (the oracle never sees them), and
  drains  drains[k] is the list of chunk starts of batch k before which the host's pipeline drains (carry_counts).
A batch is a list of (pod, template) pairs with same_sampled_gen's keys: the template's key, None when only
k_sched_loop can take the pod, NOT_LOOP for a pod of another path.

STREAMS maps a name to (builder, expect): expect is ksg_debug_same_carry's cumulative (loaded, filled) after every
batch with the key on, as literals -- carry_counts is a model of the host's rule and is itself checked against them.
"""
import functools

import norm_edge_gen as gen
import same_sampled_gen as sg
import same_template_gen as st

NOT_LOOP = sg.NOT_LOOP
POSITIONS = (100, 191, 192)  # inside a chunk; the last pod of a chunk; the first pod of a chunk (chunk_bounds(300))


def carry_counts(templates, enabled=True, drains=()):
    """(loaded, filled) of one batch with these template keys: within a pipeline chunk a stretch of at least MIN_RUN
    pods of one template is a k_sched_same launch, which loads iff the launch before it -- of any kernel, on any
    path -- was a k_sched_same run of its template.  Every other pod launches something (k_sched_loop for a key of
    None or a short stretch, k_agg_loop or the per-pod kernels for NOT_LOOP), and that forgets the carry.  (A pod that
    launches nothing -- a PreFilter error -- would leave it alone; no stream here has one.)  enabled: the cluster
    is within k_sched_same's capacity.  drains: the chunk starts before which the pipeline drains (a re-layout of the
    mirror or grown staging buffers), which forgets the carry too."""
    n = len(templates)
    if n <= 1 or not enabled:
        return 0, 0
    loaded = filled = 0
    prev, lo = None, 0
    for hi in st.chunk_bounds(n):
        if lo in drains:
            prev = None
        i = lo
        while i < hi:
            e = i + 1
            if templates[i] is not None and templates[i] != NOT_LOOP:
                while e < hi and e - i < st.LOOP_MAX_PODS and templates[e] == templates[i]:
                    e += 1
            if e - i >= st.MIN_RUN:
                if prev == templates[i]:
                    loaded += 1
                else:
                    filled += 1
                prev = templates[i]
            else:  # k_sched_loop, k_agg_loop or the per-pod launches take it
                prev = None
            i = e
        lo = hi
    return loaded, filled


def batch_counts(s, k, enabled=True):
    """carry_counts of batch k of a stream."""
    return carry_counts([key for _, key in s["batches"][k]], enabled, s["drains"][k] if "drains" in s else ())


def apply_events(b, steps):
    """Cluster events on a backend (product or oracle)."""
    for kind, arg in steps:
        if kind == "add_node":
            b.add_node(arg)
        elif kind == "remove_node":
            b.remove_node(arg)
        else:
            raise ValueError(kind)


# ---- the four first cases (one batch each) ---------------------------------------------------------------------------
def runs_out():  # 40 nodes that hold 8 template pods each, 400 pods: F reaches 0 in a later chunk, an unschedulable tail
    return st._stream(st._nodes(40, sizes=(4000,)), [st._stamp("a", 0, 400, cpu=500, mem=gen.MIB)])


def same_winner():  # MostAllocated: the node that wins a chunk's last pods wins the next chunk's first
    s = st.most()
    return st._stream(s["nodes"], [st._stamp("a", 0, 300, cpu=500, mem=gen.MIB)], s["cfg"])


def sampled():  # K = max(100, 128 * 50 / 100) = 100 < 128: every pod is cut, the rotation crosses the launches
    return st._stream(st._nodes(128), [st._stamp("a", 0, 300, cpu=20, mem=gen.MIB)], {"percentageOfNodesToScore": 50})


def template_change():  # 140 x A, 20 x B, 140 x A: the run behind B fills
    b = st._stamp("a", 0, 140, cpu=20, mem=gen.MIB) + st._stamp("b", 0, 20, cpu=30, mem=gen.MIB) + \
        st._stamp("a", 200, 140, cpu=20, mem=gen.MIB)
    return st._stream(st._nodes(64), [b])


# ---- node counts -----------------------------------------------------------------------------------------------------
def node_count(n, pct=None, native=None):
    """One batch of 300 pods, five launches; every node stays feasible and the winners cross the ballot groups (64
    nodes) and the scan lanes' slots (512 nodes)."""
    s = st._stream(st._nodes(n), [st._stamp("a", 0, 300, cpu=100, mem=gen.MIB)],
                   None if pct is None else {"percentageOfNodesToScore": pct})
    if native:
        s["native"] = dict(native)
    return s


def last_node_wins(n):
    """node_count(n) with a last node fifty times the size of the largest: in node_count(513) node 512, alone in its
    slot, wins in the first launch only; here it wins and loses inside the second launch, which selects from its
    loaded total."""
    s = node_count(n)
    s["nodes"][-1] = gen.node(n - 1, cpu_milli=400000, mem=1024 << 30, pods=1000)
    return s


# ---- sampled ---------------------------------------------------------------------------------------------------------
FLIPS_K = 100  # numFeasibleNodesToFind(150, 10)


def sampled_flips():
    """150 nodes that hold 3 template pods each, K = 100, batches of 400 and 300 pods: launches load while the cut is
    active with nodes already full (pod 317), with F < K (pod 367), and in batch 1 with F = 18 and with F = 0."""
    b0 = st._stamp("a", 0, 400, cpu=500, mem=gen.MIB)
    b1 = st._stamp("a", 400, 300, cpu=500, mem=gen.MIB)
    return st._stream(st._nodes(150, sizes=(1500,)), [b0, b1], {"percentageOfNodesToScore": 10})


def sampled_holes():  # F = 117 of 260 = K: the cut's end node moves over infeasible nodes, launch after launch
    return st._stream(sg.holes_nodes(260), [st._stamp("a", 0, 300, cpu=700, mem=900 * gen.MIB)],
                      {"percentageOfNodesToScore": 45})


# ---- a launch of another kind between two runs -------------------------------------------------------------------------
INTERLOPER_CPU = 3000  # of a 4000 / 6000 / 8000 m node: the node it lands on changes rank for the A pods behind it


def _interloper(kind, nodes):
    if kind == "loop":  # another template: a stretch of one, k_sched_loop
        return st._stamp("b", 0, 1, cpu=INTERLOPER_CPU, mem=gen.MIB)[0]
    if kind == "port":  # a host port: a loop pod k_sched_same does not take
        p = gen.pod("port-0", "a", cpu=INTERLOPER_CPU, mem=gen.MIB)
        p["spec"]["containers"][0]["ports"] = [{"containerPort": 80, "hostPort": 8080, "protocol": "TCP"}]
        return p, None
    if kind == "agg":  # own spread constraints: k_agg_loop
        p = gen.pod("pts-0", "spread", cpu=INTERLOPER_CPU, mem=gen.MIB)
        p["spec"]["topologySpreadConstraints"] = [gen.spread(gen.HOSTNAME, "spread", 1)]
        return p, NOT_LOOP
    if kind == "subset":  # a required matchFields name subset: the per-pod launches
        p = gen.pod("sub-0", "a", cpu=INTERLOPER_CPU, mem=gen.MIB)
        p["spec"]["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
            {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [gen.name_of(nodes[i])]}]}
            for i in range(20, 60)]}}}
        return p, NOT_LOOP
    raise ValueError(kind)


def interloper(kind, at, rotdev=None):
    """300 template-A pods on 64 nodes; the pod at index `at` is replaced by one pod of another path (kind None:
    left out, the stream the inputs test compares with).

    rotdev (default: for "subset"): percentageOfNodesToScore 50.  64 nodes are never cut, but nextStartNodeIndex then
    lives on the device, and only then does a pod with a PreFilterResult node subset leave the loops for the per-pod
    launches (Engine::loop_ok: k_sched_loop takes it otherwise); the A runs are k_sched_same's sampled instance, and
    the subset pod's 40 processed nodes move the rotation start of every pod behind it.

    The chunk after the first in which the batch's first k_agg_loop pod is compiled outgrows the staging sized from
    chunk 0 (the pod's program and arena), so the pipeline drains before that chunk's first launch ("drains", the
    pod indices): the host forgets the carry there as well."""
    nodes = st._nodes(64)
    b = st._stamp("a", 0, 300, cpu=20, mem=gen.MIB)
    b[at:at + 1] = [] if kind is None else [_interloper(kind, nodes)]
    s = st._stream(nodes, [b], {"percentageOfNodesToScore": 50} if (kind == "subset" if rotdev is None else rotdev) else None)
    if kind == "agg":
        s["drains"] = [[max(x for x in [0] + st.chunk_bounds(300) if x <= at)]]
    return s


# ---- batches and cluster events ----------------------------------------------------------------------------------------
def events():
    """Three batches of 300 template-A pods; nodes 60..129 (with the pods on them) leave between batches 0 and 1, 70
    fresh nodes join between batches 1 and 2.  The carry buffer keeps the previous batch's words and its last tag."""
    nodes = st._nodes(130)
    fresh = [gen.node(i, cpu_milli=(4000, 6000, 8000)[i % 3]) for i in range(130, 200)]
    s = st._stream(nodes, [st._stamp("a", 300 * k, 300, cpu=20, mem=gen.MIB) for k in range(3)])
    s["events"] = [[], [("remove_node", gen.name_of(nodes[i])) for i in range(60, 130)], [("add_node", nd) for nd in fresh]]
    return s


FIRST = {"runs-out": (runs_out, ((4, 1),)), "same-winner": (same_winner, ((4, 1),)), "sampled": (sampled, ((4, 1),)),
         "template-change": (template_change, ((4, 3),))}

STREAMS = {
    **FIRST,
    **{f"nodes-{n}": (functools.partial(node_count, n), ((4, 1),)) for n in (63, 65, st.SCAN_THREADS + 1, st.CAPACITY)},
    "nodes-513-last": (functools.partial(last_node_wins, st.SCAN_THREADS + 1), ((4, 1),)),
    "nodes-8193": (functools.partial(node_count, st.CAPACITY + 1), ((0, 0),)),
    "nodes-8192-pct0": (functools.partial(node_count, st.CAPACITY, 0), ((4, 1),)),
    "sampled-flips": (sampled_flips, ((4, 1), (8, 2))),
    "sampled-holes": (sampled_holes, ((4, 1),)),
    **{f"interloper-{kind}-{at}": (functools.partial(interloper, kind, at), ((4, 2) if at == 100 else (3, 2),))
       for kind in ("loop", "port", "subset") for at in POSITIONS},
    # (the drain before pod 32 costs the launch there its load; before pod 192 it changes nothing)
    "interloper-agg-100": (functools.partial(interloper, "agg", 100), ((3, 3),)),
    "interloper-agg-191": (functools.partial(interloper, "agg", 191), ((2, 3),)),
    "interloper-agg-192": (functools.partial(interloper, "agg", 192), ((3, 2),)),
    "events": (events, ((4, 1), (8, 2), (12, 3))),
    "verify": (functools.partial(node_count, 65, None, {"compileMemo": "verify"}), ((4, 1),)),
}


def run_oracle(s):
    """The oracle's result tuples of a stream, batch by batch."""
    from oracle_binding import oracle
    o = gen.load(oracle(dict(s["cfg"])), s["nodes"], s["bound"])
    want = []
    for k, b in enumerate(s["batches"]):
        apply_events(o, s.get("events", [[]] * (k + 1))[k])
        want.append(tuple(o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p, _ in b))
    o.close()
    return tuple(want)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The stream, the oracle's result tuples batch by batch and the expected carry counts (computed once, shared,
    never changed)."""
    build, expect = STREAMS[name]
    s = build()
    return s, run_oracle(s), expect
