"""The k_sched_same streams (same_template_gen.py) against the oracle alone: each contains the boundary it claims.
No GPU.  The host's sched_same predicate compiles pods, which takes a context on a device: its pairs are in
test_gpu_same_template.py (test_sched_same_pairs).
"""
import itertools

import pytest

import same_template_gen as st


def _runs(keys):
    return [(k, len(list(g))) for k, g in itertools.groupby(keys)]


@pytest.mark.parametrize("name", ["flip-cpu", "flip-pods"])
def test_feasible_count_reaches_zero(name):
    s, want = st.reference(name)
    (w,) = want
    per_node = 3 if name == "flip-cpu" else 2
    placed = 5 * per_node
    feas = [t[3] for t in w]
    assert [t[0] for t in w] == [0] * placed + [2] * (len(w) - placed), w  # 2: Unschedulable
    assert sorted(set(feas), reverse=True) == [5, 4, 3, 2, 1, 0], feas  # every F on the way down
    assert feas == sorted(feas, reverse=True) and feas[placed:] == [0] * (len(w) - placed)
    nodes = [t[1] for t in w[:placed]]
    assert all(nodes.count(i) == per_node for i in range(5)), nodes


def test_most_allocated_repeats_its_winner():
    _, ((*w,),) = st.reference("most")
    runs = _runs([t[1] for t in w])
    assert runs[:5] == [(runs[k][0], 6) for k in range(5)], runs  # 6 consecutive equal winners, five times
    assert len({n for n, _ in runs[:5]}) == 5


def test_ties_are_decided_by_position():
    _, ((*w,),) = st.reference("ties")
    assert all(t[0] == 0 and t[3] == 12 for t in w)
    first = [t for t in w[:12]]
    assert len({t[4] for t in first}) == 1 and len({t[1] for t in first}) == 12, first  # one score, twelve nodes


def test_static_holes_and_image():
    s, ((*w,),) = st.reference("holes")
    closed = sum(1 for i in range(40) if i % 6 == 2 or i % 9 == 4)
    assert w[0][3] == 40 - closed and len({t[4] for t in w}) > 5, w[0]
    s, ((*w,),) = st.reference("image")
    holders = {i for i in range(30) if i % 3 == 1}
    assert all(t[1] in holders for t in w[:10]), [t[1] for t in w]  # ImageLocality decides


def test_template_boundaries():
    s, _ = st.reference("boundaries")
    keys = [k for _, k in s["batches"][0]]
    assert _runs(keys) == [("a", st.MIN_RUN), ("b", 1), ("a", st.MIN_RUN - 1), ("b", st.MIN_RUN + 1)]
    assert st.dispatch(keys) == (2 * st.MIN_RUN + 1, st.MIN_RUN)
    s, _ = st.reference("ineligible")
    keys = [k for _, k in s["batches"][0]]
    assert _runs(keys) == [("a", 20), (None, 1), ("a", 20), (None, 1), ("a", 20), ("sel", 1), ("a", 20)]
    assert st.dispatch(keys) == (80, 3)
    _, ((*w,),) = st.reference("ineligible")
    assert w[62][3] == 2 and w[62][1] in (3, 11), w[62]  # the nodeSelector pod: two feasible nodes


def test_dispatch_rule():
    assert st.chunk_bounds(255) == [255]
    assert st.chunk_bounds(300) == [32, 192, 257, 283, 300]  # chunks of 32, 160, 65, 26 and 17 pods
    assert st.dispatch(["a"]) == (0, 0)
    assert st.dispatch(["a"] * (st.MIN_RUN - 1)) == (0, st.MIN_RUN - 1)
    assert st.dispatch(["a"] * st.MIN_RUN) == (st.MIN_RUN, 0)
    assert st.dispatch(["a"] * st.MIN_RUN, enabled=False) == (0, st.MIN_RUN)
    assert st.dispatch(["a"] * 300) == (300, 0)
    assert st.dispatch(["a"] * 31 + ["b"] * 269) == (299, 1)  # b's first pod ends chunk 0: a stretch of one
    assert st.dispatch(["a"] * (st.LOOP_MAX_PODS + 1)) == (st.LOOP_MAX_PODS + 1, 0)
    assert st.dispatch([None] * 40) == (0, 40)
    s, want = st.reference("batch-sizes")
    assert [len(b) for b in s["batches"]] == [1, st.MIN_RUN - 1, st.MIN_RUN, 300, st.LOOP_MAX_PODS + 1]
    assert all(t[0] == 0 for w in want for t in w)
