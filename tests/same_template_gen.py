"""Streams for k_sched_same: batches of pods stamped from few templates, each stream built around
one boundary of the kernel or of the host's dispatch rule.  Shared by test_same_template_inputs.py (the streams
against the oracle alone: each contains the boundary it claims) and test_gpu_same_template.py.

A stream is a dict: cfg, nodes, bound, batches.  A batch is a list of (pod, template) pairs; template is the key of
the pod's template when k_sched_same can take the pod, else None.  Every pod of every stream is one k_sched_loop
takes, so the dispatch rule leaves exactly two outcomes per pod.
"""
import functools

import norm_edge_gen as gen

MIN_RUN = 16          # config loopSameMinRun's default (host.hpp)
SCAN_THREADS = 512    # desc.h kSameScanWaves * 64: nodes per slot of the scan lanes
CAPACITY = 8192       # desc.h kSameMaxNodes
LOOP_MAX_PODS = 1024  # desc.h kLoopMaxPods
FIRST_CHUNK = 32      # config pipelineFirstChunk's default
NOSCHED = {"key": "same/keep-out", "value": "v", "effect": "NoSchedule"}
IMAGE = "same.example/app:1"


def chunk_bounds(n):
    """Engine::run_batch's pipeline chunks of an n-pod batch (ends, ascending)."""
    bnd = []
    if n >= 256:
        r, prev = n, 0
        while r > 32:
            take = min(FIRST_CHUNK if prev == 0 else min((r * 3 + 4) // 5, 5 * prev), r)
            bnd.append(n - r + take)
            r -= take
            prev = take
    if not bnd or bnd[-1] != n:
        bnd.append(n)
    return bnd


def dispatch(templates, min_run=MIN_RUN, enabled=True):
    """(taken, not_taken) of ksg_debug_same_pods for one batch of loop pods with these template keys: a batch of one
    pod runs no loop; within a pipeline chunk, a maximal stretch of one template (at most LOOP_MAX_PODS pods) of at
    least min_run pods goes to k_sched_same."""
    n = len(templates)
    if n <= 1:
        return 0, 0
    taken, lo = 0, 0
    for hi in chunk_bounds(n):
        i = lo
        while i < hi:
            e = i + 1
            if templates[i] is not None:
                while e < hi and e - i < LOOP_MAX_PODS and templates[e] == templates[i]:
                    e += 1
                if enabled and e - i >= min_run:
                    taken += e - i
            i = e
        lo = hi
    return taken, n - taken


def _nodes(n, sizes=(4000, 6000, 8000), mem=16 << 30, pods=110, **kw):
    return [gen.node(i, cpu_milli=sizes[i % len(sizes)], mem=mem, pods=pods, **kw) for i in range(n)]


def _stamp(tag, k, count, **kw):
    """`count` pods of one template: they differ in name and uid only."""
    return [(gen.pod(f"{tag}-{k + j}", tag, **kw), tag) for j in range(count)]


def _stream(nodes, batches, cfg=None, bound=()):
    return {"cfg": dict(cfg or {}), "nodes": nodes, "bound": list(bound), "batches": batches}


def node_count(n):
    return _stream(_nodes(n), [_stamp("a", 0, 24, cpu=500)])


def flip_cpu():  # 5 nodes that each hold exactly 3 template pods: F = 5 ... 1 ... 0, an unschedulable tail
    return _stream(_nodes(5, sizes=(1500,)), [_stamp("a", 0, 20, cpu=500, mem=gen.MIB)])


def flip_pods():  # the pod-count limit binds: 2 pods per node
    return _stream(_nodes(5, sizes=(8000,), pods=2), [_stamp("a", 0, 20, cpu=100, mem=gen.MIB)])


def holes():
    nodes = []
    for i in range(40):
        nd = gen.node(i, cpu_milli=(3000, 4500, 7000, 9500, 16000)[i % 5], mem=(8 + i % 7) << 30,
                      taints=[NOSCHED] if i % 6 == 2 else None)
        if i % 9 == 4:
            nd["spec"]["unschedulable"] = True
        nodes.append(nd)
    return _stream(nodes, [_stamp("a", 0, 30, cpu=700, mem=900 * gen.MIB)])


def ties():  # identical empty nodes, 3x as many pods: every selection is the pre-order key's
    return _stream(_nodes(12, sizes=(8000,)), [_stamp("a", 0, 36, cpu=100)])


def most():  # MostAllocated on nodes that hold 6 pods: the same node wins 6 times in a row
    cfg = {"nodeResourcesFit": {"scoringStrategy": {"type": "MostAllocated"}}}
    return _stream(_nodes(6, sizes=(3000,)), [_stamp("a", 0, 30, cpu=500, mem=gen.MIB)], cfg)


def image():  # the pod's image on a third of the nodes
    nodes = [gen.node(i, cpu_milli=(4000, 6000)[i % 2], images=[(IMAGE, 600 * gen.MIB)] if i % 3 == 1 else None)
             for i in range(30)]
    return _stream(nodes, [_stamp("a", 0, 32, cpu=300, images=(IMAGE,))])


def boundaries():  # A x minRun, B x 1, A x (minRun - 1), B x (minRun + 1); B differs in its requests
    b = (_stamp("a", 0, MIN_RUN, cpu=300) + _stamp("b", 0, 1, cpu=450) + _stamp("a", 100, MIN_RUN - 1, cpu=300) +
         _stamp("b", 100, MIN_RUN + 1, cpu=450))
    return _stream(_nodes(20), [b])


def ineligible():  # inside a run: a host-port pod, a pod with preferred node affinity, a nodeSelector pod
    port = gen.pod("port-0", "a", cpu=300)
    port["spec"]["containers"][0]["ports"] = [{"containerPort": 80, "hostPort": 8080, "protocol": "TCP"}]
    pref = gen.pod("pref-0", "a", cpu=300)
    pref["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        gen._pref(5, "zone3", "In", ["z1"])]}}
    sel = gen.pod("sel-0", "a", cpu=300)
    sel["spec"]["nodeSelector"] = {"pick": "yes"}
    nodes = _nodes(20)
    for i in (3, 11):
        nodes[i]["metadata"]["labels"]["pick"] = "yes"
    b = (_stamp("a", 0, 20, cpu=300) + [(port, None)] + _stamp("a", 100, 20, cpu=300) + [(pref, None)] +
         _stamp("a", 200, 20, cpu=300) + [(sel, "sel")] + _stamp("a", 300, 20, cpu=300))
    return _stream(nodes, [b])


def batch_sizes():  # batches of 1, minRun - 1 and minRun pods, then the chunked pipeline, then kLoopMaxPods + 1
    nodes = _nodes(24, sizes=(16000, 24000), mem=64 << 30, pods=110)
    out, k = [], 0
    for n in (1, MIN_RUN - 1, MIN_RUN, 300, LOOP_MAX_PODS + 1):
        out.append(_stamp("a", k, n, cpu=10, mem=gen.MIB))
        k += n
    return _stream(nodes, out)


STREAMS = {
    **{f"nodes-{n}": functools.partial(node_count, n)
       for n in (1, 63, 64, 65, SCAN_THREADS, SCAN_THREADS + 1, CAPACITY, CAPACITY + 1)},
    "flip-cpu": flip_cpu, "flip-pods": flip_pods, "holes": holes, "ties": ties, "most": most, "image": image,
    "boundaries": boundaries, "ineligible": ineligible, "batch-sizes": batch_sizes,
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
