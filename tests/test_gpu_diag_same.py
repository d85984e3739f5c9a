"""ksg_schedule_batch_diag over k_sched_same's runs (config "loopSameDiag"): a diagnosed batch's
same-template stretches run in k_sched_same -- instance 0 at percentageOfNodesToScore 100, the sampled instance at 0
and 30 -- and k_same_diag behind each run reduces its FitErrors, a suffix of the run, from the mirror as the run
leaves it.

Reference: tests/diagnosis_reference.py (the oracle pod by pod, each failing cycle's evaluation output reduced in
Python), through tests/diag_fast_paths_gen.py; tests/test_diag_fast_paths_inputs.py states on the oracle alone what
each stream holds.  Every case asserts ksg_debug_same_pods: the pods of the stretches that qualify ran in
k_sched_same (without the feature a diagnosed batch takes none), and schedules the stream twice more on fresh
contexts -- with "loopSameDiag": false (the same results and diagnoses from k_sched_loop) and undiagnosed (the same
results)."""
import pytest

import diag_fast_paths_gen as dg
from diagnosis_reference import FIT_ERROR, empty
from norm_edge_gen import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def check(g, got, want, tag=""):
    """tests/test_gpu_diagnosis.py's check(), per batch (the mirror and the loops: after the last one)."""
    assert len(got) == len(want)
    for k, ((rg, dg_), (ro, do)) in enumerate(zip(got, want)):
        assert rg == ro, f"{tag} pod {k}: result {rg} != reference {ro}"
        assert dg_ == do, f"{tag} pod {k} (status {ro[0]}): diagnosis\n {dg_}\n != reference\n {do}"
        if ro[0] not in FIT_ERROR:
            assert dg_ == empty(do["num_nodes"], do["prefilter_code"], do["prefilter_plugin"])


def settled(g):
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


def run_stream(native, s, want, extra, diag, tag):
    """The stream's batches on a fresh context -> [per batch results (and diagnoses)], same_pods() after each batch."""
    g = load(native(dict(s["cfg"], device=0, **extra)), s["nodes"], s["bound"])
    out, counts = [], []
    for k, (b, w) in enumerate(zip(s["batches"], want)):
        hs = [g.compile(p) for p, _ in b]
        if diag:
            rs, ds = g.schedule_batch_diag(hs, assume=True)
            got = [(r.as_tuple(), d.as_dict()) for r, d in zip(rs, ds)]
            check(g, got, w, f"{tag} batch {k}:")
        else:
            got = [r.as_tuple() for r in g.schedule_batch(hs, assume=True)]
            assert got == [r for r, _ in w], f"{tag} batch {k}"
        out.append(got)
        counts.append(g.same_pods())
    settled(g)
    g.close()
    return out, counts


@pytest.mark.parametrize("case,n,pct", dg.SAME_CASES, ids=[f"{c}-{n}-pct{p}" for c, n, p in dg.SAME_CASES])
def test_diagnosed_same_template_runs(native, case, n, pct):
    """a: the run's first pod already fails; b: the run fills the cluster and fails from the middle on; c: runs
    without a failure around failing pods of another template (their rows stay empty); d: a failing run, a smaller
    template that still lands in k_sched_loop, a second failing run (rot_out and the mirror pass between k_sched_same,
    k_same_diag and k_sched_loop); e: 1100 pods in one chunk -- two launches, the second starts with F == 0; f: a run
    one pod short of loopSameMinRun stays in k_sched_loop."""
    s, want = dg.same_reference(case, n, pct)
    tag = f"{case}, {n} nodes, pct {pct}"
    on, counts = run_stream(native, s, want, {}, True, tag)
    taken = other = 0
    for k, b in enumerate(s["batches"]):
        t, o = dg.same_taken(s, b)
        taken += t
        other += o
        assert counts[k] == (taken, other), (tag, k, counts[k], (taken, other))
    last = dg.same_taken(s, s["batches"][-1])[0]  # the batch with the failures: in k_sched_same, but for case f
    assert (last == 0) == (case == "f"), last
    off, counts_off = run_stream(native, s, want, {"loopSameDiag": False}, True, tag + ", loopSameDiag false")
    assert off == on
    assert all(c[0] == 0 for c in counts_off), counts_off
    plain, _ = run_stream(native, s, want, {}, False, tag + ", undiagnosed")
    assert plain == [[r for r, _ in b] for b in on]
