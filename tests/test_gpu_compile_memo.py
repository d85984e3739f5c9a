"""The compile memo (config "compileMemo") against the oracle, with "verify" on: every program the memo
hands out is also compiled in full and compared byte for byte inside the library, so a stale entry fails the call.

1. every stream of same_template_gen.py under "verify": the oracle's results, k_sched_same's dispatch counts, a clean
   mirror, and ksg_debug_compile_memo EQUAL to what the stream's template keys give;
2. invalidation: one cache event between two batches of one template -- the first pod behind it is compiled in full;
3. a 300-pod batch (the chunked pipeline: later chunks compile while earlier assumes are not in the shadow yet);
4. "off": no counts, the same results.
"""
import copy
import json

import pytest

import norm_edge_gen as gen
import same_template_gen as st

pytestmark = pytest.mark.gpu
VERIFY = {"compileMemo": "verify"}


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def memo_key(pod):
    """A pod's template as the memo sees it: the object without its name and uid; None for a pod whose program is
    not node-local whatever the cluster holds (own spread constraints or pod (anti-)affinity, a nomination, a node name)."""
    p = copy.deepcopy(pod)
    p["metadata"].pop("name", None)
    p["metadata"].pop("uid", None)
    spec, status = p.get("spec") or {}, p.get("status") or {}
    aff = spec.get("affinity") or {}
    if (spec.get("topologySpreadConstraints") or aff.get("podAffinity") or aff.get("podAntiAffinity") or
            spec.get("nodeName") or status.get("nominatedNodeName")):
        return None
    return json.dumps(p, sort_keys=True)


class Counter:
    """hits / misses the compiles of a context must show: a pod hits iff it is memo-eligible and the last
    memo-eligible compile had its key (and nothing invalidated the entry since: invalidate())."""

    def __init__(self):
        self.hits = self.misses = 0
        self.last = None

    def invalidate(self):
        self.last = None

    def compile(self, pod, eligible=True):
        k = memo_key(pod) if eligible else None
        if k is not None and k == self.last:
            self.hits += 1
        else:
            self.misses += 1
        if k is not None:
            self.last = k


# ---- 1. every stream, verify mode --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(st.STREAMS))
def test_stream_verify(native, name):
    s, want = st.reference(name)
    g = gen.load(native(dict(s["cfg"], **VERIFY)), s["nodes"], s["bound"])
    cnt = Counter()
    taken = other = 0
    fits = len(s["nodes"]) <= st.CAPACITY
    for k, batch in enumerate(s["batches"]):
        rs = g.schedule_batch([g.compile(p) for p, _ in batch], assume=True)
        got = [r.as_tuple() for r in rs]
        for q in range(len(batch)):
            assert got[q] == want[k][q], f"batch {k} pod {q}: {got[q]} != oracle {want[k][q]}"
        t, o = st.dispatch([key for _, key in batch], enabled=fits)
        taken += t
        other += o
        assert g.same_pods() == (taken, other), (k, g.same_pods(), (taken, other))
        assert g.compare_mirror(sync=False) == (0, -1)
        assert g.loop_stats() == (0, 0)
        for p, _ in batch:
            cnt.compile(p)
        assert g.compile_memo() == (cnt.hits, cnt.misses), (k, g.compile_memo(), (cnt.hits, cnt.misses))
    assert cnt.hits > 0
    if name in ("boundaries", "ineligible"):  # the streams that change the template inside a batch
        assert cnt.misses > len(s["batches"])
    g.close()


# ---- 2. invalidation ---------------------------------------------------------------------------------------------------
IMAGE = "memo.example/app:1"
KEEP_OUT = {"key": "memo/keep-out", "value": "v", "effect": "NoSchedule"}
SYSTEM_SPREAD = {}  # the default profile: PodTopologySpread's system-default constraints
SERVICE = {"apiVersion": "v1", "kind": "Service", "metadata": {"name": "svc", "namespace": "default"},
           "spec": {"selector": {"app": "tpl"}}}


def _template(k, count):
    return [gen.pod(f"tpl-{k + j}", "tpl", cpu=200, mem=64 * gen.MIB, images=(IMAGE,)) for j in range(count)]


def _ev_tainted_node(b):
    b.add_node(gen.node(100, cpu_milli=64000, taints=[KEEP_OUT]))


def _ev_image(b):
    b.update_node(gen.node(3, cpu_milli=6000, images=[(IMAGE, 700 * gen.MIB)]))


def _ev_remove_node(b):
    b.remove_node(gen.node(5)["metadata"]["name"])


def _ev_anti_pod(b):
    p = gen.pod("anti-0", "other", cpu=100, node_name=gen.node(1)["metadata"]["name"])
    b.add_pod(gen.add_pod_terms(p, "podAntiAffinity", required=[gen.term("kubernetes.io/hostname", "tpl")]))


def _ev_nominate(b):
    q = gen.pod("nominee-0", "other", cpu=3000)
    q["spec"]["priority"] = 100
    q["status"] = {"nominatedNodeName": gen.node(2)["metadata"]["name"]}
    b.add_nominated_pod(q)


def _ev_service(b):
    b.upsert_object(SERVICE)


# event -> (config, the event, the second batch's pods stay memo-eligible)
EVENTS = {
    "tainted-node-added": ({}, _ev_tainted_node, True),
    "image-added": ({}, _ev_image, True),
    "node-removed": ({}, _ev_remove_node, True),
    "anti-affinity-pod-bound": ({}, _ev_anti_pod, False),   # the template turns DF_AGGREGATE
    "pod-nominated": ({"nominatedPods": "Evaluate"}, _ev_nominate, False),  # a nominee table is in use
    "service-added": (SYSTEM_SPREAD, _ev_service, False),   # the template gets default spread constraints
}


@pytest.mark.parametrize("name", list(EVENTS))
def test_invalidation(native, name):
    cfg, event, eligible = EVENTS[name]
    nodes = [gen.node(i, cpu_milli=6000) for i in range(8)]
    if name == "pod-nominated":
        from nominated_reference import NominatedReference
        ref = NominatedReference(cfg, nodes, [], [{"metadata": {"name": "default"}}])
        want_of = lambda p: ref.schedule(p, assume=True)  # noqa: E731
    else:
        from oracle_binding import oracle
        ref = gen.load(oracle(dict(cfg)), nodes, [])
        want_of = lambda p: ref.schedule_one(ref.compile(p), assume=True)[0].as_tuple()  # noqa: E731
    g = gen.load(native(dict(cfg, **VERIFY)), nodes, [])
    cnt = Counter()
    for half in range(2):
        pods = _template(20 * half, 20)
        if half:
            event(g)
            event(ref)
            cnt.invalidate()
        before = g.compile_memo()
        rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
        for q, p in enumerate(pods):
            assert rs[q].as_tuple() == want_of(p), (name, half, q)
        for p in pods:
            cnt.compile(p, eligible or not half)
        hits, misses = g.compile_memo()
        assert misses > before[1], f"{name}: the first pod after the event was not compiled in full"
        assert (hits, misses) == (cnt.hits, cnt.misses), (name, half, (hits, misses), (cnt.hits, cnt.misses))
        assert g.compare_mirror(sync=False) == (0, -1)
        assert g.loop_stats() == (0, 0)
    assert cnt.hits == (38 if eligible else 19)
    g.close()


# ---- 3. later chunks ---------------------------------------------------------------------------------------------------
def test_later_chunks(native):
    from oracle_binding import oracle
    nodes = [gen.node(i, cpu_milli=(16000, 24000)[i % 2], mem=64 << 30) for i in range(64)]
    pods = [gen.pod(f"chunk-{j}", "tpl", cpu=50, mem=8 * gen.MIB) for j in range(300)]
    assert len(st.chunk_bounds(len(pods))) > 1  # the chunked pipeline
    o = gen.load(oracle({}), nodes, [])
    want = [o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in pods]
    o.close()
    g = gen.load(native(dict(VERIFY)), nodes, [])
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    assert [r.as_tuple() for r in rs] == want
    assert g.compile_memo() == (299, 1)
    assert g.same_pods() == st.dispatch(["tpl"] * 300)
    assert g.compare_mirror(sync=False) == (0, -1)
    assert g.loop_stats() == (0, 0)
    g.close()


# ---- 4. off ------------------------------------------------------------------------------------------------------------
def test_off(native):
    s, want = st.reference("boundaries")
    g = gen.load(native(dict(s["cfg"], compileMemo="off")), s["nodes"], s["bound"])
    for k, batch in enumerate(s["batches"]):
        rs = g.schedule_batch([g.compile(p) for p, _ in batch], assume=True)
        assert [r.as_tuple() for r in rs] == list(want[k])
    assert g.compile_memo() == (0, 0)
    g.close()


def test_bad_value(native):
    from ksg.abi import KsgError
    with pytest.raises(KsgError):
        native({"compileMemo": "maybe"})
