"""Inputs for the FitError diagnosis on k_sched_same's runs and on k_agg_loop's sampling instances (configs
"loopSameDiag" / "aggLoopSampledDiag"), and their reference: tests/diagnosis_reference.py -- the
oracle pod by pod, each failing cycle's evaluation output reduced in Python.  Shared by
test_diag_fast_paths_inputs.py (the oracle alone: every stream holds what it claims), test_gpu_diag_same.py and
test_gpu_diag_agg_sampled.py; a reference is computed once per stream and never changed.

A same-template stream: cfg, nodes, bound, batches, where a batch is a list of (pod, template key) pairs as in
same_template_gen.py (None: a pod k_sched_same cannot follow with its neighbours).  An agg stream: cfg, nodes,
bound, objects, pods (one batch)."""
import functools

import norm_edge_gen as gen
import same_sampled_gen as ss
import same_template_gen as st
from diagnosis_reference import FIT_ERROR, fill, reference_stream
from ksg.objects import NodeW, PodW
from oracle_binding import oracle

MIB, GIB = gen.MIB, 1024 * gen.MIB
HOST, ZONE = "kubernetes.io/hostname", "topology.kubernetes.io/zone"
NSS = [{"metadata": {"name": "default"}}]
# context keys the oracle does not take
LOOP_KEYS = ("loopUnit", "persistentLoop", "aggLoop", "aggLoopDebug", "aggLoopSampled", "aggLoopSampledDiag",
             "loopSameDiag", "loopSameSampled", "loopSameTemplate", "loopWorkgroups", "pipelineFirstChunk", "device")


def oracle_cfg(cfg):
    return {k: v for k, v in cfg.items() if k not in LOOP_KEYS}


def sampled(cfg, n):
    """The context cuts feasible lists on this cluster (numFeasibleNodesToFind < N)."""
    return ss.num_to_find(n, cfg.get("percentageOfNodesToScore", 100)) < n


# =====================================================================================================================
# k_sched_same
# =====================================================================================================================
PERIOD = 36  # nodes i with i % 36 < 6 turn the template pod away, each kind in its own way; the others take it


def same_cluster(n):
    """(nodes, bound).  Of every 36 nodes one each is unschedulable, carries an untolerated NoSchedule taint, is short
    of cpu, of memory, of both (a Fit status with two reason bits), and full by pod count; the other 30 hold one
    template pod (1 cpu / 2 GiB), every seventh node three (2 cpu / 3 GiB: full, it is short of cpu and memory)."""
    nodes, bound = [], []
    for i in range(n):
        kind = i % PERIOD
        cpu, mem, pods, taints = (2000, 3 * GIB, 110, None) if i % 7 == 3 else (1000, 2 * GIB, 110, None)
        if kind == 1:
            taints = [st.NOSCHED]
        elif kind == 2:
            cpu = 300
        elif kind == 3:
            mem = 256 * MIB
        elif kind == 4:
            cpu, mem = 300, 256 * MIB
        elif kind == 5:
            pods = 1
        nd = gen.node(i, cpu_milli=cpu, mem=mem, pods=pods, taints=taints)
        if kind == 0:
            nd["spec"]["unschedulable"] = True
        if kind == 5:
            bound.append(gen.pod(f"sitter-{i}", "sit", cpu=10, mem=MIB, node_name=gen.name_of(nd)))
        nodes.append(nd)
    return nodes, bound


def room(n):
    """Template pods "a" the cluster holds."""
    return sum((3 if i % 7 == 3 else 1) for i in range(n) if i % PERIOD >= 6)


def tmpl(tag, k, count):
    """`count` pods of one template, numbered from k.  a: the template that fills the cluster; b: a smaller one that
    still lands once a no longer does (and takes the node's memory: a second failing run of a sees other reasons); s: a
    tiny one that never fails; big: asks for more cpu than any node has (and 1 GiB: two reason bits on the nodes short of
    memory)."""
    kw = {"a": dict(cpu=600, mem=GIB), "b": dict(cpu=350, mem=900 * MIB), "s": dict(cpu=10, mem=MIB),
          "big": dict(cpu=5000, mem=GIB)}[tag]
    return st._stamp(tag, k, count, **kw)


def same_case(case, n, pct):
    nodes, bound = same_cluster(n)
    cfg = {"percentageOfNodesToScore": pct}
    r = room(n)
    if case == "a":    # the run's first pod already fails: an earlier batch filled the cluster
        batches = [tmpl("a", 0, r), tmpl("a", r, 24)]
    elif case == "b":  # fills the cluster and fails from the middle on
        batches = [tmpl("a", 0, r + 24)]
    elif case == "c":  # runs without a failure around pods of another template that fail
        batches = [tmpl("s", 0, 20) + tmpl("big", 0, 5) + tmpl("s", 20, 20)]
    elif case == "d":  # a failing run, a smaller template that still lands (k_sched_loop: a short run), a second failing run
        batches = [tmpl("a", 0, r + 20) + tmpl("b", 0, 3) + tmpl("a", r + 20, 20)]
    elif case == "e":  # more pods than one launch takes, in one pipeline chunk: the second launch starts with F == 0
        cfg["pipelineFirstChunk"] = 1100
        batches = [tmpl("a", 0, 1100)]
    elif case == "f":  # one pod short of loopSameMinRun: k_sched_loop's
        batches = [tmpl("a", 0, r), tmpl("a", r, st.MIN_RUN - 1)]
    else:
        raise KeyError(case)
    return {"cfg": cfg, "nodes": nodes, "bound": bound, "batches": batches}


def same_taken(s, batch):
    """(taken, not_taken) of ksg_debug_same_pods for one batch of the stream."""
    if s["cfg"].get("pipelineFirstChunk", st.FIRST_CHUNK) >= len(batch) >= 256:  # one chunk: stretches of <= 1024 pods
        keys = [k for _, k in batch]
        assert len(set(keys)) == 1
        tail = len(batch) % st.LOOP_MAX_PODS
        taken = len(batch) - (tail if tail < st.MIN_RUN else 0)
        return taken, len(batch) - taken
    return ss.counts(batch)


SAME_SIZES = (9, 130, 257, 600)
SAME_PCTS = (100, 0, 30)
SAME_CASES = [(c, n, p) for n in SAME_SIZES for p in SAME_PCTS for c in "abcdf"] + [("e", 9, p) for p in SAME_PCTS]


@functools.lru_cache(maxsize=None)
def same_reference(case, n, pct):
    """(stream, per batch [(result tuple, diagnosis dict)])."""
    s = same_case(case, n, pct)
    o = gen.load(oracle(oracle_cfg(s["cfg"])), s["nodes"], s["bound"])
    want = tuple(tuple(reference_stream(o, [p for p, _ in b])) for b in s["batches"])
    o.close()
    return s, want


# =====================================================================================================================
# k_agg_loop's sampling instances
# =====================================================================================================================
TOL_UNSCHED = {"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoSchedule"}
TOL_DED = {"key": "dedicated", "operator": "Exists", "effect": "NoSchedule"}
BIG = 64 * 256 + 6  # 65 node blocks: the instances that sweep more than one round of 64 workgroups


def web(app="web"):
    return {"matchLabels": {"app": app}}


# the two flavours of a loop-class pod that fails nowhere by itself (tests/test_gpu_diagnosis_agg.py): a ScheduleAnyway
# hostname constraint (the PodTopologySpread-scoring twins) or a required anti-affinity term that matches nothing
def soft(p):
    return p.spread(3, HOST, "ScheduleAnyway", web())


def anti_nothing(p):
    return p.pod_affinity(HOST, web("nothing"), anti=True)


FLAVOURS = {"soft": soft, "anti": anti_nothing}


def status_cluster(n):
    """n nodes, every one unschedulable and tainted dedicated=x:NoSchedule, 4 cpu / 8Gi / 10Gi ephemeral / 2 gpus, room
    for 3 pods and two bound already: `hot-k` (app=hot, host port 8080) and, on the first node of each zone, a `guard`
    with a required zone anti-affinity term against app=victim (a plain `sitter` elsewhere)."""
    nodes, existing = [], []
    for k in range(n):
        name = f"n{k:03d}"
        nodes.append(NodeW(name).capacity({"cpu": "4", "memory": "8Gi", "pods": "3", "ephemeral-storage": "10Gi",
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


def status_stream(flavour, n):
    """Pods that land, then pods that each fail on all n nodes for one reason between pods that land, then n small
    pods of which the last find every node full (Too many pods)."""
    mk = FLAVOURS[flavour]

    def base(name, cpu="100m", tol=(TOL_UNSCHED, TOL_DED), app="x", **req):
        p = PodW(name).label("app", app).container(image="i", requests=dict({"cpu": cpu}, **req))
        p.tolerations(list(tol))
        return mk(p)
    ok = lambda name: base(name).obj()  # noqa: E731
    nodename = base("nodename").obj()
    nodename["spec"]["nodeName"] = "no-such-node"
    pods = [
        ok("ok0"), ok("ok1"),
        base("unsched", tol=(TOL_DED,)).obj(),
        ok("ok2"),
        nodename,
        base("taint", tol=(TOL_UNSCHED,)).obj(),
        base("affinity").node_selector({"disk": "nvme"}).obj(),
        ok("ok3"),
        base("port").host_port(8080).obj(),
        base("cpu", cpu="5").obj(),
        base("mem", memory="9Gi").obj(),
        ok("ok4"),
        base("eph", **{"ephemeral-storage": "11Gi"}).obj(),
        base("gpu", **{"example.com/gpu": "3"}).obj(),
        base("cpu-mem", cpu="5", memory="9Gi").obj(),
        # every node holds an app=hot pod and 1000 domains are asked for: the minimum counts as 0, skew 2 > 1
        base("skew", app="hot").spread(1, HOST, "DoNotSchedule", web("hot"), min_domains=1000).obj(),
        ok("ok5"),
        base("label").spread(1, "rack", "DoNotSchedule", web("hot")).obj(),
        base("pod-aff").pod_affinity(HOST, web("nobody")).obj(),
        base("pod-anti").pod_affinity(ZONE, web("hot"), anti=True).obj(),
        base("existing-anti", app="victim").obj(),
        ok("ok6"),
    ]
    pods += [base(f"fill{k}", cpu="10m").obj() for k in range(n)]
    return pods


def box(name, zone, cpu="4"):
    return NodeW(name).capacity({"cpu": cpu, "memory": "8Gi", "pods": "20"}).label(HOST, name).label(ZONE, zone).obj()


def small(name, app, cpu="100m"):
    return PodW(name).label("app", app).container(image="i", requests={"cpu": cpu})


def grid(n, zones="abc"):
    """n 4-cpu nodes over three zones; an app=db pod bound in each zone."""
    nodes = [box(f"g{k:05d}", zones[k % len(zones)]) for k in range(n)]
    existing = [small(f"db{z}", "db").node(f"g{k:05d}").obj() for k, z in enumerate(zones)]
    return nodes, existing


def grid_stream(flavour):
    """Pods of one flavour on the grid: some land, some fail on every node for one reason."""
    mk = lambda name, cpu="100m": FLAVOURS[flavour](small(name, "web", cpu))  # noqa: E731
    return [
        mk("a0").obj(), mk("a1").obj(),
        mk("a-cpu", cpu="5").obj(),
        mk("a-label").spread(1, "rack", "DoNotSchedule", web()).obj(),
        mk("a2").obj(),
        mk("a-anti").pod_affinity(ZONE, web("db"), anti=True).obj(),
        mk("a-mem").container(image="i", requests={"memory": "9Gi"}).obj(),
        mk("a3").obj(),
        mk("a-aff").pod_affinity(HOST, web("nobody")).obj(),
        mk("a-last", cpu="4500m").obj(),
    ]


def mixed_stream():
    """Node-local pods (k_sched_loop's class) and pods of both flavours in runs of two, on the grid: pods of every kind
    that land and that fail.  -> (pods, indices of the k_agg_loop-class pods)."""
    pods, klass = [], []
    for k in range(48):
        if k % 4 < 2:
            p = small(f"plain{k}", "plain", cpu="5" if k % 16 == 8 else "30m")
            if k and k % 16 == 0:  # (a second container: more memory than any node has)
                p.container(image="i", requests={"memory": "9Gi"})
            pods.append(p.obj())
            continue
        klass.append(k)
        mk = soft if k % 8 < 4 else anti_nothing
        if k % 12 == 2:
            p = mk(small(f"k-cpu{k}", "web", cpu="4500m")).obj()
        elif k % 12 == 6:
            p = mk(small(f"k-anti{k}", "web")).pod_affinity(ZONE, web("db"), anti=True).obj()
        elif k % 12 == 10:
            p = mk(small(f"k-label{k}", "web")).spread(1, "rack", "DoNotSchedule", web()).obj()
        else:
            p = mk(small(f"k{k}", "web", cpu="30m")).obj()
        pods.append(p)
    return pods, klass


# name: (stream kind, nodes, flavour, percentage, extra context config)
AGG_CASES = {}
for _n in (130, 257, 600):
    for _pct in (0, 30):
        for _fl in sorted(FLAVOURS):
            AGG_CASES[f"status-{_n}-{_fl}-pct{_pct}"] = ("status", _n, _fl, _pct, {})
for _fl in sorted(FLAVOURS):
    AGG_CASES[f"status-600-one-workgroup-{_fl}"] = ("status", 600, _fl, 30, {"loopWorkgroups": 1})
    AGG_CASES[f"grid-65-workgroups-{_fl}"] = ("grid", BIG, _fl, 45, {})
    for _dbg in (2, 32):  # the generic filter path; the template cache off
        AGG_CASES[f"status-257-{_fl}-debug{_dbg}"] = ("status", 257, _fl, 0, {"aggLoopDebug": _dbg})
AGG_CASES["mixed-130"] = ("mixed", 130, None, 30, {})


@functools.lru_cache(maxsize=None)
def _agg_stream(kind, n, flavour):
    if kind == "status":
        nodes, bound = status_cluster(n)
        return nodes, bound, status_stream(flavour, n), None
    nodes, bound = grid(n)
    if kind == "grid":
        return nodes, bound, grid_stream(flavour), None
    pods, klass = mixed_stream()
    return nodes, bound, pods, klass


@functools.lru_cache(maxsize=None)
def _agg_want(kind, n, flavour, pct):
    nodes, bound, pods, _ = _agg_stream(kind, n, flavour)
    o = fill(oracle({"percentageOfNodesToScore": pct}), nodes, bound, NSS)
    want = tuple(reference_stream(o, pods))
    o.close()
    return want


def agg_reference(name):
    """(cfg, nodes, bound, pods, indices of the k_agg_loop-class pods or None for all, [(result, diagnosis)])."""
    kind, n, flavour, pct, extra = AGG_CASES[name]
    nodes, bound, pods, klass = _agg_stream(kind, n, flavour)
    return dict(extra, percentageOfNodesToScore=pct), nodes, bound, pods, klass, _agg_want(kind, n, flavour, pct)


# ---- the conditions every stream meets, on the reference alone ------------------------------------------------------
def input_conditions(want, n, k_cut):
    """want: [(result tuple, diagnosis)] of one stream in order; k_cut: numFeasibleNodesToFind when the context cuts
    lists on this cluster, else None."""
    failed = [d for r, d in want if r[0] in FIT_ERROR]
    assert len(failed) >= 5, len(failed)
    plugins = {p for d in failed for p, c in enumerate(d["plugin_nodes"]) if c}
    reasons = {b for d in failed for b, c in enumerate(d["reason_nodes"]) if c}
    assert len(plugins) >= 3 and len(reasons) >= 4, (plugins, reasons)
    if k_cut is not None:
        first = next(k for k, (r, _) in enumerate(want) if r[0] in FIT_ERROR)
        # a placed pod whose list was cut: K feasible nodes found, and the search stopped before the last node
        assert any(r[0] == 0 and r[3] == k_cut and r[2] < n for r, _ in want[:first]), "no cut before the first failure"
        assert all(r[2] == n for r, _ in want if r[0] in FIT_ERROR)
