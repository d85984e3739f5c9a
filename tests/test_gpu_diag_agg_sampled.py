"""ksg_schedule_batch_diag for sampled PodTopologySpread / InterPodAffinity pods (percentageOfNodesToScore below 100;
config "aggLoopSampledDiag"): they run in the diagnosing twins of k_agg_loop's sampling instances,
which reduce a failing pod's statuses inside the loop -- a sampled pod without a feasible node has no cut and
evaluated every node.

Reference: tests/diagnosis_reference.py (the oracle pod by pod, each failing cycle's evaluation output reduced in
Python), through tests/diag_fast_paths_gen.py, whose streams follow tests/test_gpu_diagnosis_agg.py's: pods that each
fail on every node for one reason between pods that land, and a tail that finds every node full, in the two flavours
(`soft`: the PodTopologySpread-scoring twins; `anti`: the others).  tests/test_diag_fast_paths_inputs.py states on the
oracle alone what each stream holds (among it: a cut list before the first failure).  Where every pod of the batch is
of the loop's class the case asserts that the loop ran all of them -- without the feature a diagnosed batch's sampled
pods run on the per-pod launches."""
import pytest

import diag_fast_paths_gen as dg
from diagnosis_reference import FIT_ERROR, empty, fill

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def run_diag(g, pods):
    rs, ds = g.schedule_batch_diag([g.compile(p) for p in pods], assume=True)
    return [(r.as_tuple(), d.as_dict()) for r, d in zip(rs, ds)]


def check(g, got, want, tag=""):
    """tests/test_gpu_diagnosis.py's check()."""
    assert len(got) == len(want)
    for k, ((rg, dg_), (ro, do)) in enumerate(zip(got, want)):
        assert rg == ro, f"{tag} pod {k}: result {rg} != reference {ro}"
        assert dg_ == do, f"{tag} pod {k} (status {ro[0]}): diagnosis\n {dg_}\n != reference\n {do}"
        if ro[0] not in FIT_ERROR:
            assert dg_ == empty(do["num_nodes"], do["prefilter_code"], do["prefilter_plugin"])
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


def device(native, cfg, nodes, bound):
    return fill(native(dict(cfg, device=0)), nodes, bound, dg.NSS)


@pytest.mark.parametrize("name", sorted(dg.AGG_CASES))
def test_sampled_class_pods_are_diagnosed_in_the_loop(native, name):
    """130 nodes: K = 100 in one workgroup; 257: two workgroups, the second with one node; 600: three, or one that owns
    every node block ("loopWorkgroups": 1); 65 workgroups: the instances that sweep more than one round; aggLoopDebug 2:
    the generic filter path, 32: no template cache; mixed: node-local and loop-class pods in one batch."""
    cfg, nodes, bound, pods, klass, want = dg.agg_reference(name)
    g = device(native, cfg, nodes, bound)
    got = run_diag(g, pods)
    if klass is None:  # every pod of the batch is of the loop's class
        assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    check(g, got, want, name)
    g.close()


@pytest.mark.parametrize("flavour", sorted(dg.FLAVOURS))
def test_the_key_turns_it_off(native, flavour):
    """"aggLoopSampledDiag": false: the same results and diagnoses from the per-pod launches and k_diag_reduce; and an
    undiagnosed batch returns the same results from k_agg_loop's sampling instances."""
    cfg, nodes, bound, pods, _, want = dg.agg_reference(f"status-257-{flavour}-pct0")
    g = device(native, dict(cfg, aggLoopSampledDiag=False), nodes, bound)
    got = run_diag(g, pods)
    assert g.kernel_stats()[3] != "k_agg_loop"
    check(g, got, want, "aggLoopSampledDiag false:")
    g.close()
    p = device(native, cfg, nodes, bound)
    plain = [r.as_tuple() for r in p.schedule_batch([p.compile(x) for x in pods], assume=True)]
    assert p.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    assert plain == [r for r, _ in want]
    assert p.compare_mirror(sync=True) == (0, -1) and p.loop_stats() == (0, 0)
    p.close()
