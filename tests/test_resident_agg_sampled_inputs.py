"""The inputs of tests/test_gpu_resident_agg_sampled.py (sampled pods on the per-pod API, in the resident k_agg_loop),
checked on the oracle alone: no device.  tests/test_agg_sampled_inputs.py states the conditions on
tests/agg_sampled_gen.py's streams, which the single calls reuse; these are the conditions on the streams
tests/resident_agg_sampled_gen.py adds.  They are conditions on the inputs, not measurements."""
import agg_sampled_gen as gen
import resident_agg_sampled_gen as rgen


def test_mixed_stream_puts_cut_pods_behind_same_template_and_node_local_pods():
    """In one resident launch a cut pod's rotation start arrives with its doorbell, also when phase 1 ran ahead of it
    on the previous pod's program: at least 5 cut pods directly follow a pod of the same template, and at least 3 cut
    pod-table pods directly follow a node-local pod.  Node-local pods are cut too, and one follows a pod-table pod."""
    cfg, nodes, bound, pods, want = rgen.mixed_reference()
    assert len(pods) == len(want) and all(c.placed for c in want)
    assert all(rgen.is_node_local(p) for p in pods[:rgen.MIXED_LEAD]) and not rgen.is_node_local(pods[rgen.MIXED_LEAD])
    tpl = [rgen.template_of(p) for p in pods]
    local = [rgen.is_node_local(p) for p in pods]
    pairs = range(rgen.MIXED_LEAD + 1, len(pods))  # both pods of the pair in k_agg_loop's launch
    same = [k for k in pairs if want[k].cut and not local[k] and tpl[k] == tpl[k - 1]]
    after_local = [k for k in pairs if want[k].cut and not local[k] and local[k - 1]]
    local_after_class = [k for k in pairs if want[k].cut and local[k] and not local[k - 1]]
    assert len(same) >= 5, same
    assert len(after_local) >= 3, after_local
    assert len(local_after_class) >= 3, local_after_class
    # the cut pods' lists have numFeasibleNodesToFind nodes
    assert {c.feasible for c in want if c.cut} == {180}  # 30 % of 600


def test_same_stream_is_one_template_with_cut_pods_in_a_row():
    """agg_sampled_gen's "same" stream, which takes the copied program and phase 1 ahead of the doorbell."""
    for shape, pct in (("257", 0), ("600", 30)):
        cfg, nodes, bound, pods, want = gen.reference(shape, "same", True, pct)
        tpl = [rgen.template_of(p) for p in pods]
        assert sum(want[k].cut and tpl[k] == tpl[k - 1] for k in range(1, len(pods))) >= 5


def test_handover_steps_cut_on_both_sides_of_every_event():
    """Every scheduling step of the hand-over sequence holds cut pods, the rotation start moves across every step, and
    the stream is longer than one resident launch."""
    cfg, nodes, bound, steps = rgen.handover_reference()
    n = len(nodes)
    sched = [(s, a, res) for s, a, pods, res in steps if res]
    assert [s for s, _, _ in sched] == ["one", "batch", "one", "one", "one", "one", "calls"]
    for s, a, res in sched:
        assert len(res) == a
        # (after the node add the list has n + 1 nodes)
        assert sum(r[0] == 0 and r[2] <= n - 1 for r in res) >= 3, (s, a)
    assert sched[-1][1] > rgen.MAX_LAUNCH_PODS
    assert [s for s, _, _, _ in steps].count("sleep") == 1
    assert {"add_node", "forget"} <= {s for s, _, _, _ in steps}


def test_binding_exposes_resident_calls():
    from ksg.native import Scheduler
    assert callable(getattr(Scheduler, "resident_calls"))
