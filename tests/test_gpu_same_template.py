"""k_sched_same against the oracle and against k_sched_loop.

Every stream of same_template_gen.py is scheduled three ways -- the oracle, a context with loopSameTemplate false
(k_sched_loop as before) and a default context -- and compared pod by pod on all five result fields.  After every
batch the device mirror must equal the host's shadow, no loop may have given up, and ksg_debug_same_pods must EQUAL
the counts the dispatch rule gives for the stream (same_template_gen.dispatch): no case passes by falling back.
"""
import pytest

import norm_edge_gen as gen
import same_template_gen as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def _run(native, s, want, enabled):
    cfg = dict(s["cfg"])
    if not enabled:
        cfg["loopSameTemplate"] = False
    g = gen.load(native(cfg), s["nodes"], s["bound"])
    taken = other = 0
    fits = len(s["nodes"]) <= st.CAPACITY
    for k, batch in enumerate(s["batches"]):
        rs = g.schedule_batch([g.compile(p) for p, _ in batch], assume=True)
        got = [r.as_tuple() for r in rs]
        for q in range(len(batch)):
            assert got[q] == want[k][q], f"batch {k} pod {q} (same={enabled}): {got[q]} != oracle {want[k][q]}"
        t, o = st.dispatch([key for _, key in batch], enabled=enabled and fits)
        taken += t
        other += o
        assert g.same_pods() == (taken, other), (k, g.same_pods(), (taken, other))
        assert g.compare_mirror(sync=False) == (0, -1)
        assert g.loop_stats() == (0, 0)
    g.close()
    return taken


@pytest.mark.parametrize("name", list(st.STREAMS))
def test_stream(native, name):
    s, want = st.reference(name)
    assert _run(native, s, want, False) == 0
    taken = _run(native, s, want, True)
    assert (taken > 0) == (name != f"nodes-{st.CAPACITY + 1}"), taken  # past the capacity: the old loop


def test_sched_same_pairs(native):
    """The host's predicate: pods stamped from one template match whatever their name and uid; different requests, a
    toleration or an image do not."""
    nodes = st._nodes(8)  # a taint and an image in the cluster: the toleration and the image change the program
    nodes[0] = gen.node(0, taints=[st.NOSCHED])
    nodes[1] = gen.node(1, images=[("same.example/other:2", 500 * gen.MIB)])
    g = gen.load(native({}), nodes, [])
    a = gen.pod("pair-a", "app", cpu=300)
    b = gen.pod("pair-b-with-a-longer-name", "app", cpu=300)
    req = gen.pod("pair-c", "app", cpu=301)
    tol = gen.pod("pair-d", "app", cpu=300)
    tol["spec"]["tolerations"] = [{"key": st.NOSCHED["key"], "operator": "Exists", "effect": "NoSchedule"}]
    img = gen.pod("pair-e", "app", cpu=300, images=("same.example/other:2",))
    port = gen.pod("pair-f", "app", cpu=300)
    port["spec"]["containers"][0]["ports"] = [{"containerPort": 80, "hostPort": 8080, "protocol": "TCP"}]
    h = {k: g.compile(p) for k, p in dict(a=a, b=b, req=req, tol=tol, img=img, port=port).items()}
    assert g.sched_same(h["a"], h["b"]) and g.sched_same(h["b"], h["a"]) and g.sched_same(h["a"], h["a"])
    for k in ("req", "tol", "img"):
        assert not g.sched_same(h["a"], h[k]) and not g.sched_same(h[k], h["a"]), k
    assert not g.sched_same(h["port"], h["port"])  # a pod with a host port is no pod of such a run
    g.close()
