"""The streams of k_sched_same's sampled instance (same_sampled_gen.py) against the oracle alone: each contains the
boundary it claims.  No GPU.  Result tuples are (status, node, EvaluatedNodes, FeasibleNodes, TotalScore).
"""
import itertools

import pytest

import same_sampled_gen as sg
import same_template_gen as st


def _one(name):
    s, (w,) = sg.reference(name)
    return s, list(w)


def test_num_to_find():
    assert [sg.num_to_find(n, 0) for n in (99, 100, 101, 513, 5000, 8192)] == [99, 100, 100, 235, 500, 409]
    assert sg.num_to_find(130, 30) == 100 and sg.num_to_find(260, 45) == 117 and sg.num_to_find(150, 10) == 100
    assert sg.num_to_find(130, 100) == 130


def test_cut_begins_at_101_nodes():
    s, w = _one("cut-100")  # numFeasibleNodesToFind never cuts 100 nodes: the rotation is carried but stands still
    assert all(t[0] == 0 and t[2] == 100 and t[3] == 100 for t in w), w
    for name, n in (("cut-101", 101), ("cut-130", 130)):
        s, w = _one(name)
        assert len(s["nodes"]) == n and 40 <= len(w) <= 60
        assert all(t[0] == 0 and t[3] == 100 and t[2] < n for t in w), w  # every pod cut
        assert len({t[1] for t in w}) == len(w)  # each on a node of its own
        assert sum(t[2] for t in w) > 10 * n  # the rotation wraps the node list many times


def test_slots_and_capacity():
    s, w = _one("slots-513")
    assert all(t[0] == 0 and t[3] == 235 for t in w), w
    s, w = _one("capacity-8192")
    assert len(s["nodes"]) == st.CAPACITY and all(t[0] == 0 and t[3] == 409 for t in w), w
    assert [t[1] for t in w[:3]] == [128, 410, 818], w[:3]
    s, w = _one("over-8193")
    assert len(s["nodes"]) == st.CAPACITY + 1 and all(t[0] == 0 and t[3] < len(s["nodes"]) for t in w)
    for name in ("slots-513", "capacity-8192", "over-8193"):
        s, _ = sg.reference(name)
        assert sg.counts(s["batches"][0]) == (24, 0)  # (the dispatch rule alone: the capacity is the test's to apply)


def test_processed_varies_with_the_failures_before_the_end_node():
    s, w = _one("holes-260")
    assert all(t[0] == 0 and t[3] == 117 for t in w), w
    assert {t[2] for t in w} == {161, 162, 163}, sorted({t[2] for t in w})


def test_fill_crosses_from_the_cut_to_an_empty_list():
    s, (w0, w1) = sg.reference("fill-150")
    assert len(w0) == 230 and len(w1) == 240
    assert all(t[0] == 0 and t[3] == 100 and t[2] < 150 for t in w0), "batch 0: every pod cut"
    assert [t[0] for t in w1] == [0] * 220 + [2] * 20  # 2: Unschedulable
    w = list(w0) + list(w1)
    cut = [t for t in w if t[2] < 150]
    assert cut == w[:230 + 120]  # 120 pods of batch 1 are cut while ballots flip under the cut
    # EvaluatedNodes climbs from 100 towards 150 (not monotonically: it depends on where the window starts)
    ev = [t[2] for t in cut]
    assert ev[0] == 100 and min(ev) == 100 and max(ev[-5:]) == 149 and len(set(ev)) >= 30, sorted(set(ev))
    last = len(cut) - 1  # the last cut pod (F = K + 1) and the first uncut one (F = K = 100) are consecutive
    assert w[last][3] == 100 and w[last][2] < 150 and w[last + 1][2:4] == (150, 100), (w[last], w[last + 1])
    feas = [t[3] for t in w[last + 1:]]
    assert feas == sorted(feas, reverse=True) and set(range(0, 100)) <= set(feas), feas
    assert feas[-20:] == [0] * 20


def test_most_allocated_leaves_the_window_and_returns():
    s, w = _one("most-260")
    nodes = [t[1] for t in w]
    assert all(t[0] == 0 and t[3] == 100 and t[2] < 260 for t in w), "all cut"
    assert all(a != b for a, b in zip(nodes, nodes[1:])), nodes  # no two consecutive pods on one node
    returns = sum(nodes[k] in nodes[:k] for k in range(len(nodes)))
    assert returns >= 90, returns


def test_ties_follow_the_cut_lists_positions():
    s, w = _one("ties-120")
    assert all(t[0] == 0 and t[3] == 100 for t in w), w
    assert len({t[4] for t in w}) == 1 and len({t[1] for t in w}) == 120
    assert [t[1] for t in w[:8]] == [0, 100, 80, 60, 40, 20, 1, 101], [t[1] for t in w[:8]]


def test_handover_shapes():
    s, w = _one("handover")
    keys = [k for _, k in s["batches"][0]]
    runs = [(k, len(list(g))) for k, g in itertools.groupby(keys)]
    assert runs == [("a", 20), ("b", 1), ("a", 20), (sg.NOT_LOOP, 1), ("a", 20), (sg.NOT_LOOP, 1), ("a", 20)]
    assert sg.counts(s["batches"][0]) == (80, 1) and sg.counts(s["batches"][0], enabled=False) == (0, 81)
    assert all(t[0] == 0 for t in w)
    assert w[41][3] == 40 and 20 <= w[41][1] < 60, w[41]  # the matchFields pod: its 40 named nodes
    assert sum(t[3] == 100 and t[2] < 130 for t in w) >= 80  # every template pod is cut


def test_noscore_and_nominated():
    s, w = _one("noscore")
    assert all(t[0] == 0 and t[3] == 1 for t in w), w  # numNodesToFind is 1 without score plugins
    assert sg.counts(s["batches"][0]) == (0, 24)
    s, w = _one("nominated-at-100")
    assert w[17][:4] == (0, 30, 1, 1), w[17]  # placed on its nominated node, alone
    assert all(t[0] == 0 and t[2] == 130 and t[3] == 130 for k, t in enumerate(w) if k != 17)
    assert sg.counts(s["batches"][0]) == (39, 0) and sg.counts(s["batches"][0], enabled=False) == (0, 39)
