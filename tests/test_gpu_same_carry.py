"""k_sched_same's carry (config "loopSameCarry"): the launches of one batch hand their cached state
on, so every launch after the first of consecutive runs of one template loads it instead of evaluating its fill.

Each case is one batch large enough for the chunked pipeline, scheduled with the key true and false; both must equal
the oracle pod by pod on all five result fields, leave the mirror equal to the host's shadow and no loop given up, and
ksg_debug_same_carry must EQUAL the counts the launch sequence gives (carry_counts): no case passes by filling.
"""
import functools

import pytest

import norm_edge_gen as gen
import same_template_gen as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def carry_counts(templates):
    """(loaded, filled) of one batch: within a pipeline chunk a stretch of at least MIN_RUN pods of one template is a
    k_sched_same launch, which loads iff the launch before it (of any kernel) was a k_sched_same run of its template."""
    n = len(templates)
    if n <= 1:
        return 0, 0
    loaded = filled = 0
    prev, lo = None, 0
    for hi in st.chunk_bounds(n):
        i = lo
        while i < hi:
            e = i + 1
            while e < hi and e - i < st.LOOP_MAX_PODS and templates[e] == templates[i]:
                e += 1
            if e - i >= st.MIN_RUN:
                if prev == templates[i]:
                    loaded += 1
                else:
                    filled += 1
                prev = templates[i]
            else:  # k_sched_loop takes it
                prev = None
            i = e
        lo = hi
    return loaded, filled


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


CASES = {"runs-out": runs_out, "same-winner": same_winner, "sampled": sampled, "template-change": template_change}


@functools.lru_cache(maxsize=None)
def reference(name):
    from oracle_binding import oracle
    s = CASES[name]()
    o = gen.load(oracle(dict(s["cfg"])), s["nodes"], s["bound"])
    want = tuple(tuple(o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p, _ in b) for b in s["batches"])
    o.close()
    return s, want


def _run(native, s, want, carry, diag=False):
    g = gen.load(native(dict(s["cfg"], loopSameCarry=carry)), s["nodes"], s["bound"])
    loaded = filled = 0
    rows = []
    for k, batch in enumerate(s["batches"]):
        hs = [g.compile(p) for p, _ in batch]
        if diag:
            rs, ds = g.schedule_batch_diag(hs, assume=True)
            rows.append([d.as_dict() for d in ds])
        else:
            rs = g.schedule_batch(hs, assume=True)
        got = [r.as_tuple() for r in rs]
        for q in range(len(batch)):
            assert got[q] == want[k][q], f"batch {k} pod {q} (carry={carry}): {got[q]} != oracle {want[k][q]}"
        a, b = carry_counts([key for _, key in batch])
        loaded += a
        filled += b
        assert g.same_carry() == ((loaded, filled) if carry else (0, 0)), (k, g.same_carry(), (loaded, filled))
        assert g.same_pods()[0] > 0
        assert g.compare_mirror(sync=False) == (0, -1)
        assert g.loop_stats() == (0, 0)
    g.close()
    return loaded, rows


@pytest.mark.parametrize("name", list(CASES))
def test_case(native, name):
    s, want = reference(name)
    _run(native, s, want, False)
    loaded, _ = _run(native, s, want, True)
    assert loaded >= 3, loaded  # the case does carry
    if name == "runs-out":  # the tail is unschedulable: ballots with no feasible node were carried
        assert sum(1 for t in want[0] if t[1] < 0) == 400 - 40 * 8
    if name == "template-change":
        assert carry_counts(["a"] * 140 + ["b"] * 20 + ["a"] * 140) == (4, 3)  # B, and the A run behind it, fill


def test_diagnosed(native):
    """k_same_diag between the launches does not block the carry; the diagnosis rows equal the uncarried run's."""
    s, want = reference("runs-out")
    _, off = _run(native, s, want, False, diag=True)
    loaded, on = _run(native, s, want, True, diag=True)
    assert loaded >= 3
    assert on == off
    assert all(r["failed_nodes"] == 40 for r in on[0][320:]), "the tail's FitErrors name every node"
