"""The streams of k_sched_same's carry (same_carry_gen.py) against the oracle alone: each contains what it claims, and
carry_counts -- the test's model of the host's rule -- reproduces the expected counts its table states as literals.
No GPU.  Result tuples are (status, node, EvaluatedNodes, FeasibleNodes, TotalScore).
"""
import collections
import functools

import pytest

import same_carry_gen as cg
import same_sampled_gen as sg
import same_template_gen as st


def _cumulative(s):
    out, loaded, filled = [], 0, 0
    fits = len(s["nodes"]) <= st.CAPACITY  # (no stream's events take it across the capacity)
    for k in range(len(s["batches"])):
        a, f = cg.batch_counts(s, k, enabled=fits)
        loaded += a
        filled += f
        out.append((loaded, filled))
    return tuple(out)


@pytest.mark.parametrize("name", list(cg.STREAMS))
def test_carry_counts_reproduces_the_literals(name):
    build, expect = cg.STREAMS[name]
    s = build()
    assert len(expect) == len(s["batches"])
    assert _cumulative(s) == expect, (name, _cumulative(s), expect)


def test_carry_counts_rule():
    assert st.chunk_bounds(300) == [32, 192, 257, 283, 300] and st.chunk_bounds(400) == [32, 192, 317, 367, 387, 400]
    assert cg.carry_counts(["a"] * 140 + ["b"] * 20 + ["a"] * 140) == (4, 3)  # B, and the A run behind it, fill
    assert cg.carry_counts(["a"] * 300, enabled=False) == (0, 0)
    assert cg.carry_counts(["a"]) == (0, 0) and cg.carry_counts(["a"] * 255) == (0, 1)
    assert cg.carry_counts(["a"] * 400) == (4, 1)  # the last 13 pods are a k_sched_loop launch
    assert cg.carry_counts([None] * 300) == (0, 0)  # pods k_sched_same does not take are no stretch of a template
    assert cg.carry_counts([cg.NOT_LOOP] * 300) == (0, 0)
    for key in (None, cg.NOT_LOOP, "b"):  # any launch between two runs forgets the carry
        assert cg.carry_counts(["a"] * 100 + [key] + ["a"] * 199) == (4, 2), key
        assert cg.carry_counts(["a"] * 191 + [key] + ["a"] * 108) == (3, 2), key
        assert cg.carry_counts(["a"] * 192 + [key] + ["a"] * 107) == (3, 2), key
        # ... the 11 pods it leaves of its chunk go to k_sched_loop: fills at 0 and 192, loads at 32, 257 and 283
        assert cg.carry_counts(["a"] * 180 + [key] + ["a"] * 119) == (3, 2), key
    # a pipeline drain before a chunk forgets the carry as a launch of another kind does
    assert cg.carry_counts(["a"] * 300, drains=[32]) == (3, 2) and cg.carry_counts(["a"] * 300, drains=[0]) == (4, 1)
    assert cg.carry_counts(["a"] * 192 + [None] + ["a"] * 107, drains=[192]) == (3, 2)


def test_sampled_flips():
    s, (w0, w1), _ = cg.reference("sampled-flips")
    K = cg.FLIPS_K
    assert sg.num_to_find(len(s["nodes"]), s["cfg"]["percentageOfNodesToScore"]) == K and len(s["nodes"]) == 150
    assert st.chunk_bounds(len(w0)) == [32, 192, 317, 367, 387, 400] and st.chunk_bounds(len(w1)) == [32, 192, 257, 283, 300]
    # pod 317 starts a launch: the cut is active (F > K, so K are found and more are evaluated), nodes are full
    assert w0[317][3] == K and w0[317][2] > K, w0[317]
    per_node = collections.Counter(t[1] for t in w0[:317])
    assert sum(1 for c in per_node.values() if c == 3) >= 1 and max(per_node.values()) == 3, per_node
    assert 150 - sum(1 for c in per_node.values() if c == 3) > K
    # pod 367 starts a launch with F < K: no cut, every node evaluated
    assert 0 < w0[367][3] < K and w0[367][2] == 150, w0[367]
    assert all(t[0] == 0 for t in w0)
    # batch 1: launches that start with F in (0, K), and with F = 0
    starts = [w1[q][3] for q in [0] + st.chunk_bounds(len(w1))[:-1]]
    assert any(0 < f < K for f in starts[1:]) and any(f == 0 for f in starts[1:]), starts
    assert sum(1 for w in (w0, w1) for t in w if t[1] < 0) == 250
    assert [t[0] for t in w1] == [0] * 50 + [2] * 250  # 2: Unschedulable


def test_sampled_holes():
    s, (w,), _ = cg.reference("sampled-holes")
    assert len(w) == 300 and all(t[0] == 0 for t in w)
    assert all(t[3] < len(s["nodes"]) for t in w) and {t[3] for t in w} == {117}
    assert len({t[2] for t in w}) >= 2 and all(t[2] < len(s["nodes"]) for t in w), sorted({t[2] for t in w})


@pytest.mark.parametrize("name", ["nodes-63", "nodes-65", "nodes-513", "nodes-8192", "nodes-8192-pct0", "nodes-8193"])
def test_node_counts(name):
    s, (w,), _ = cg.reference(name)
    n = len(s["nodes"])
    assert n == int(name.split("-")[1]) and len(w) == 300 and st.chunk_bounds(300) == [32, 192, 257, 283, 300]
    assert all(t[0] == 0 for t in w)
    if name.endswith("pct0"):
        assert all(t[3] == sg.num_to_find(n, 0) == 409 and t[2] < n for t in w)  # every pod is cut
        assert len({t[1] // 64 for t in w}) > 64  # the window walks the node range
    else:
        assert all(t[2] == n and t[3] == n for t in w)  # every node stays feasible
    winners = {t[1] for t in w}
    assert any(i // 64 == (n - 1) // 64 for i in winners), "a winner in the last ballot group"
    if n > st.SCAN_THREADS:
        assert any(i // st.SCAN_THREADS > 0 for i in winners), "a winner in a slot other than 0"
    if n >= st.CAPACITY:  # ballot groups 64..127 (scan_groups' second half) and the upper slots, in every launch
        for lo, hi in zip([0] + st.chunk_bounds(300), st.chunk_bounds(300)):
            assert any(t[1] // 64 >= 64 for t in w[lo:hi]) and any(t[1] // st.SCAN_THREADS > 0 for t in w[lo:hi]), (lo, hi)


def test_last_node_wins_in_a_carried_launch():
    s, (w,), _ = cg.reference("nodes-513-last")
    n = len(s["nodes"])
    assert n == st.SCAN_THREADS + 1 and all(t[0] == 0 and t[2] == n and t[3] == n for t in w)
    _, (plain,), _ = cg.reference("nodes-513")
    assert [q for q, t in enumerate(plain) if t[1] == n - 1] == [10, 11, 12]  # the plain stream: the first launch only
    wins = [t[1] == n - 1 for t in w]
    assert all(wins[:32])
    second = wins[32:192]  # the launch that loads: the last node wins, loses, and wins again
    lost = second.index(False)
    assert 0 < lost and True in second[lost:] and False in wins[192:], [q for q, x in enumerate(wins) if not x]


@functools.lru_cache(maxsize=None)
def _without(at, rotdev):
    (w,) = cg.run_oracle(cg.interloper(None, at, rotdev))
    return w


@pytest.mark.parametrize("name", [k for k in cg.STREAMS if k.startswith("interloper-")])
def test_interloper_changes_what_follows(name):
    s, (w,), _ = cg.reference(name)
    _, kind, at = name.split("-")
    at = int(at)
    keys = [k for _, k in s["batches"][0]]
    assert len(keys) == 300 and keys[:at] == ["a"] * at and keys[at + 1:] == ["a"] * (299 - at)
    assert keys[at] == {"loop": "b", "port": None, "agg": cg.NOT_LOOP, "subset": cg.NOT_LOOP}[kind]
    assert sg.counts(s["batches"][0]) == (299, 0 if keys[at] == cg.NOT_LOOP else 1)
    assert all(t[0] == 0 for t in w)
    assert w[at][1] >= 0, w[at]  # the interloper is placed
    # only under a device-resident rotation does the subset pod leave k_sched_loop for the per-pod launches
    assert ("percentageOfNodesToScore" in s["cfg"]) == (kind == "subset")
    assert s.get("drains") == ({100: [[32]], 191: [[32]], 192: [[192]]}[at] if kind == "agg" else None)
    if kind == "subset":
        assert w[at][2:4] == (40, 40) and 20 <= w[at][1] < 60, w[at]
        assert all(t[2:4] == (64, 64) for q, t in enumerate(w) if q != at)  # 64 nodes: no pod is cut
    # left out, the A pods behind it get other results: a carry kept across it cannot pass unnoticed
    base = _without(at, kind == "subset")
    assert w[:at] == base[:at]
    differ = [q for q in range(at + 1, 300) if w[q] != base[q - 1]]
    assert differ, "no A pod behind the interloper notices it"
    # ... already within the launch that would load the stale state
    nxt = min(b for b in st.chunk_bounds(300) if b > at + 1)
    assert differ[0] < nxt, (differ[0], nxt)


def test_events_shapes():
    s, want, expect = cg.reference("events")
    assert [len(b) for b in s["batches"]] == [300, 300, 300] and len(s["events"]) == 3 and s["events"][0] == []
    assert [len(e) for e in s["events"]] == [0, 70, 70]
    assert {k for k, _ in s["events"][1]} == {"remove_node"} and {k for k, _ in s["events"][2]} == {"add_node"}
    assert [{t[3] for t in w} for w in want] == [{130}, {60}, {130}]  # the node count each batch saw
    assert any(t[1] >= 60 for t in want[0]), "pods were on the removed nodes"
    assert any(t[1] >= 60 for t in want[2]), "the fresh nodes win pods"
    assert all(t[0] == 0 for w in want for t in w)
