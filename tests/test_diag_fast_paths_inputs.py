"""The streams of tests/diag_fast_paths_gen.py against the oracle alone (no device): each holds what the GPU tests of
the FitError diagnosis on k_sched_same's runs and k_agg_loop's sampling instances rely on -- enough FitErrors with
several plugin and reason bins and, where the context samples, a cut list before the first failure and failing pods
that evaluated every node."""
import pytest

import diag_fast_paths_gen as dg
import same_sampled_gen as ss
from diagnosis_reference import FIT_ERROR


def k_cut(cfg, n):
    return ss.num_to_find(n, cfg["percentageOfNodesToScore"]) if dg.sampled(cfg, n) else None


@pytest.mark.parametrize("case,n,pct", dg.SAME_CASES, ids=[f"{c}-{n}-pct{p}" for c, n, p in dg.SAME_CASES])
def test_same_template_streams(case, n, pct):
    s, want = dg.same_reference(case, n, pct)
    flat = [x for b in want for x in b]
    dg.input_conditions(flat, n, k_cut(s["cfg"], n))
    status = [r[0] for r, _ in flat]
    first = next(k for k, c in enumerate(status) if c in FIT_ERROR)
    if case in "abef":  # the template fills the cluster, then every pod of it fails with one and the same diagnosis
        assert first == dg.room(n) and all(c in FIT_ERROR for c in status[first:])
        assert all(d == flat[first][1] for _, d in flat[first:])
        assert len(status) - first >= (20 if case in "be" else dg.st.MIN_RUN - 1)
    if case == "a":
        assert want[1][0][0][0] in FIT_ERROR  # the second batch's run starts with a failure
    if case == "c":
        assert [k for k, c in enumerate(status) if c in FIT_ERROR] == list(range(20, 25))
    if case == "d":
        r = dg.room(n)
        assert all(c in FIT_ERROR for c in status[r:r + 20]) and all(c == 0 for c in status[r + 20:r + 23])
        assert all(c in FIT_ERROR for c in status[r + 23:])
        assert flat[r][1] != flat[r + 23][1]  # the smaller pods moved the second run's reasons
    if case == "e":
        assert dg.same_taken(s, s["batches"][0]) == (1100, 0) and first < dg.st.LOOP_MAX_PODS < len(status)
    if case == "f":
        assert dg.same_taken(s, s["batches"][1]) == (0, dg.st.MIN_RUN - 1)
    # a Fit status with two reason bits (the node short of cpu and memory) in every failing diagnosis of template a
    if case in "abdef":
        d = flat[first][1]
        assert d["reason_nodes"][7] > 0 and d["reason_nodes"][8] > 0 and sum(d["reason_nodes"]) > d["failed_nodes"]


@pytest.mark.parametrize("name", sorted(dg.AGG_CASES))
def test_agg_sampled_streams(name):
    cfg, nodes, bound, pods, klass, want = dg.agg_reference(name)
    n = len(nodes)
    assert dg.sampled(cfg, n)
    dg.input_conditions(want, n, k_cut(cfg, n))
    if klass is not None:  # the mixed batch: FitErrors of both loops' classes
        assert sum(want[k][0][0] in FIT_ERROR for k in klass) >= 5
        assert sum(want[k][0][0] in FIT_ERROR for k in range(len(pods)) if k not in klass) >= 3
    if name.startswith("status-"):  # the tail finds every node full
        assert all(r[0] in FIT_ERROR and d["reason_nodes"][6] == n for r, d in want[-5:])
