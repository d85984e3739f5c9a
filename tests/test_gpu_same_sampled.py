"""k_sched_same's sampled instance (config "loopSameSampled") against the oracle and k_sched_loop.

Every stream of same_sampled_gen.py is scheduled three ways -- the oracle, a context with loopSameSampled false (the
routing as before: sampled pods in k_sched_loop) and a default context -- and compared pod by pod on all five result
fields.  After every batch the device mirror must equal the host's shadow, no loop may have given up, and
ksg_debug_same_pods must EQUAL the counts the dispatch rule gives for the stream: no case passes by falling back.
"""
import pytest

import norm_edge_gen as gen
import same_sampled_gen as sg
import same_template_gen as st

pytestmark = pytest.mark.gpu

# the streams k_sched_same takes nothing of: past its capacity, and the no-score profile (DF_NO_SCORE)
NOT_TAKEN = (f"over-{st.CAPACITY + 1}", "noscore")


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def _run(native, s, want, enabled):
    cfg = dict(s["cfg"])
    if not enabled:
        cfg["loopSameSampled"] = False
    g = gen.load(native(cfg), s["nodes"], s["bound"])
    taken = other = 0
    fits = len(s["nodes"]) <= st.CAPACITY
    for k, batch in enumerate(s["batches"]):
        rs = g.schedule_batch([g.compile(p) for p, _ in batch], assume=True)
        got = [r.as_tuple() for r in rs]
        for q in range(len(batch)):
            assert got[q] == want[k][q], f"batch {k} pod {q} (sampled={enabled}): {got[q]} != oracle {want[k][q]}"
        t, o = sg.counts(batch, enabled=enabled and fits)
        taken += t
        other += o
        assert g.same_pods() == (taken, other), (k, g.same_pods(), (taken, other))
        assert g.compare_mirror(sync=False) == (0, -1)
        assert g.loop_stats() == (0, 0)
    g.close()
    return taken


@pytest.mark.parametrize("name", list(sg.STREAMS))
def test_stream(native, name):
    s, want = sg.reference(name)
    assert _run(native, s, want, False) == 0
    taken = _run(native, s, want, True)
    assert (taken > 0) == (name not in NOT_TAKEN), taken
