"""k_sched_same's carry (config "loopSameCarry"): the launches of one batch hand their cached state
on, so every launch after the first of consecutive runs of one template loads it instead of evaluating its fill.

Each stream of same_carry_gen.py has batches large enough for the chunked pipeline and is scheduled with the key false
and true; both must equal the oracle pod by pod on all five result fields, leave the mirror equal to the host's shadow
and no loop given up, and ksg_debug_same_carry must EQUAL the counts the stream's table states: no case passes by
filling, and none by loading what it should not (a launch of another kind in between, another batch, a cluster
event).  test_same_carry_inputs.py shows, on the oracle alone, that each stream contains the edge it claims.
"""
import pytest

import norm_edge_gen as gen
import same_carry_gen as cg
import same_sampled_gen as sg
import same_template_gen as st
from same_carry_gen import carry_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def _run(native, s, want, carry, diag=False, expect=None):
    g = gen.load(native(dict(s["cfg"], loopSameCarry=carry, **s.get("native", {}))), s["nodes"], s["bound"])
    loaded = filled = taken = other = 0
    rows = []
    for k, batch in enumerate(s["batches"]):
        if "events" in s:
            cg.apply_events(g, s["events"][k])
        fits = len(g.node_names()) <= st.CAPACITY
        hs = [g.compile(p) for p, _ in batch]
        if diag:
            rs, ds = g.schedule_batch_diag(hs, assume=True)
            rows.append([d.as_dict() for d in ds])
        else:
            rs = g.schedule_batch(hs, assume=True)
        got = [r.as_tuple() for r in rs]
        for q in range(len(batch)):
            assert got[q] == want[k][q], f"batch {k} pod {q} (carry={carry}): {got[q]} != oracle {want[k][q]}"
        a, b = cg.batch_counts(s, k, enabled=fits)
        loaded += a
        filled += b
        if expect is not None:  # the table's literal, not the model
            assert (loaded, filled) == expect[k], (k, (loaded, filled), expect[k])
        assert g.same_carry() == ((loaded, filled) if carry else (0, 0)), (k, g.same_carry(), (loaded, filled))
        t, o = sg.counts(batch, enabled=fits)
        taken += t
        other += o
        assert g.same_pods() == (taken, other), (k, g.same_pods(), (taken, other))
        assert g.same_pods()[0] > 0 or not fits
        assert g.compare_mirror(sync=False) == (0, -1)
        assert g.loop_stats() == (0, 0)
    g.close()
    return loaded, rows


@pytest.mark.parametrize("name", list(cg.FIRST))
def test_case(native, name):
    s, want, expect = cg.reference(name)
    _run(native, s, want, False)
    loaded, _ = _run(native, s, want, True, expect=expect)
    assert loaded >= 3, loaded  # the case does carry
    if name == "runs-out":  # the tail is unschedulable: ballots with no feasible node were carried
        assert sum(1 for t in want[0] if t[1] < 0) == 400 - 40 * 8
    if name == "template-change":
        assert carry_counts(["a"] * 140 + ["b"] * 20 + ["a"] * 140) == (4, 3)  # B, and the A run behind it, fill


@pytest.mark.parametrize("name", [k for k in cg.STREAMS if k not in cg.FIRST])
def test_stream(native, name):
    """The edges: a launch of another kind between two runs (the host forgets the carry: a stale one names the
    interloper's node with its old total and ballots), node counts at the kernel's boundaries, sampled runs whose cut
    list changes across the launches, batch boundaries with cluster events, the compile memo's verify mode."""
    s, want, expect = cg.reference(name)
    _run(native, s, want, False, expect=expect)
    loaded, _ = _run(native, s, want, True, expect=expect)
    assert loaded == expect[-1][0]
    if name == "nodes-8193":  # beyond k_sched_same's capacity: k_sched_loop takes every pod, nothing is carried
        assert len(s["nodes"]) > st.CAPACITY and expect == ((0, 0),)
    else:
        assert loaded >= 2, loaded  # the stream does carry (interloper-agg-191: two loads, three fills)


def test_diagnosed(native):
    """k_same_diag between the launches does not block the carry; the diagnosis rows equal the uncarried run's."""
    s, want, expect = cg.reference("runs-out")
    _, off = _run(native, s, want, False, diag=True)
    loaded, on = _run(native, s, want, True, diag=True, expect=expect)
    assert loaded >= 3
    assert on == off
    assert all(r["failed_nodes"] == 40 for r in on[0][320:]), "the tail's FitErrors name every node"


def test_diagnosed_sampled(native):
    """The same with the sampled instance, over two batches whose feasible list runs out under the cut."""
    s, want, expect = cg.reference("sampled-flips")
    _, off = _run(native, s, want, False, diag=True, expect=expect)
    loaded, on = _run(native, s, want, True, diag=True, expect=expect)
    assert loaded == 8
    assert on == off
    tail = [(k, q) for k, w in enumerate(want) for q, t in enumerate(w) if t[1] < 0]
    assert len(tail) == 250
    assert all(on[k][q]["failed_nodes"] == 150 for k, q in tail), "every unschedulable pod's FitError names every node"
