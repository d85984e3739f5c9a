"""Sampled pods on the per-pod API (config "residentAggSampled", default on; DESIGN.md §4.5 "Resident k_agg_loop"):
with percentageOfNodesToScore below 100 (0, upstream's adaptive default, included), ksg_schedule_one of a
PodTopologySpread / InterPodAffinity pod is served by the resident k_agg_loop's sampling instances, which cut the
feasible list; nextStartNodeIndex stays the host's and travels with every doorbell.

Every comparison is against the oracle pod by pod -- the whole result tuple -- and every case ends with the mirror equal
to the host's cache and no loop give-up.  The streams are tests/agg_sampled_gen.py's and
tests/resident_agg_sampled_gen.py's; tests/test_agg_sampled_inputs.py and tests/test_resident_agg_sampled_inputs.py
check on the oracle alone what they exercise."""
import time

import pytest

import agg_sampled_gen as gen
import resident_agg_sampled_gen as rgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def device(native, cfg, nodes, bound):
    return gen.fill(native(dict(cfg, device=0)), nodes, bound)


def calls(g, pods):
    return [g.schedule_one(g.compile(p), assume=True)[0].as_tuple() for p in pods]


def check(g, got, want, tag=""):
    assert len(got) == len(want)
    for k, (rg, c) in enumerate(zip(got, want)):
        ro = c.result if isinstance(c, gen.Cycle) else c
        assert rg == ro, f"{tag} pod {k}: {rg} != oracle {ro}"
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


# ---- 1. the routing ------------------------------------------------------------------------------------------------
def test_sampled_single_calls_run_in_the_resident_loop_and_the_key_turns_it_off(native):
    """percentageOfNodesToScore 0 (adaptive: 48 % of 257 nodes): every call is served by the resident k_agg_loop; with
    "residentAggSampled": false every call takes the per-pod launches.  Both equal the oracle."""
    cfg, nodes, bound, pods, want = gen.reference("257", "three", True, 0)
    assert sum(c.cut for c in want) >= 5
    g = device(native, cfg, nodes, bound)
    got = calls(g, pods)
    assert g.resident_calls() == (0, len(pods), 0)
    check(g, got, want, "on:")
    off = device(native, dict(cfg, residentAggSampled=False), nodes, bound)
    got_off = calls(off, pods)
    assert off.resident_calls() == (0, 0, len(pods))
    check(off, got_off, want, "off:")


# ---- 2. shapes, percentages, the doorbell's forms ------------------------------------------------------------------
SHAPES = ["9", "130", "257", "600", "600-one-workgroup"]


@pytest.mark.parametrize("debug", [0, 8], ids=["copied", "staged"])
@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "no-ahead"])
@pytest.mark.parametrize("kind", ["five", "same"])
@pytest.mark.parametrize("pct", [0, 7, 30, 55])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_percentages(native, shape, pct, kind, ahead, debug):
    """The shapes and percentages of the batch test (tests/test_gpu_agg_sampled.py), pod by pod: the streams with
    ScheduleAnyway constraints at percentages 0 and 30, the ones without at 7 and 55.  "five": five templates in an
    irregular order.  "same": one template repeated -- the program is copied in LDS and patched from the doorbell
    (RING_SAME), and phase 1 of a pod ran at the end of the pod before it, against that pod's rotation start
    (residentAhead); a cut pod then counts the nodes before its own start from the ballots.  aggLoopDebug 8 stages
    every pod's program over PCIe instead."""
    soft = pct in (0, 30)
    cfg, nodes, bound, pods, want = gen.reference(shape, kind, soft, pct)
    g = device(native, dict(cfg, residentAhead=ahead, aggLoopDebug=debug), nodes, bound)
    got = calls(g, pods)
    assert g.resident_calls() == (0, len(pods), 0)
    check(g, got, want, f"{shape} {kind} pct {pct} residentAhead {ahead} aggLoopDebug {debug}:")


# ---- 3. more than 64 workgroups ------------------------------------------------------------------------------------
@pytest.mark.parametrize("relay", [1, 1 << 20], ids=["relayed", "direct"])
@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
def test_more_than_64_workgroups(native, soft, relay):
    """64 * 256 + 6 nodes: 65 workgroups, the four-round instance (without the PodTopologySpread raw-score guess); the
    doorbell relayed by workgroup 0 through device memory, and read by every workgroup from the host."""
    cfg, nodes, bound, pods, want = gen.reference("big", "three", soft, 45, n_pods=16)
    g = device(native, dict(cfg, ringRelayMinWorkgroups=relay), nodes, bound)
    got = calls(g, pods)
    assert g.resident_calls() == (0, len(pods), 0)
    check(g, got, want, f"soft {soft} ringRelayMinWorkgroups {relay}:")


# ---- 4. the hand-over of nextStartNodeIndex ------------------------------------------------------------------------
def test_rotation_is_handed_over_between_calls_batches_events_and_launches(native):
    """Single calls, a batch of sampled pods (k_agg_loop's batch sampling instances), single calls again, a node add,
    a forget, a gap longer than the resident launch's idle window, and more calls than one launch takes (a relaunch
    mid-stream): every result equals the oracle's, so every nextStartNodeIndex was the one the previous cycle left."""
    cfg, nodes, bound, steps = rgen.handover_reference()
    g = device(native, cfg, nodes, bound)
    last, single = None, 0
    for k, (step, arg, pods, want) in enumerate(steps):
        if step in ("one", "calls", "batch"):
            hs = [g.compile(p) for p in pods]
            if step == "one":
                got = [g.schedule_one(h, assume=True)[0].as_tuple() for h in hs]
            elif step == "calls":
                got = [r.as_tuple() for r in g.schedule_calls(hs, assume=True)[0]]
            else:
                got = [r.as_tuple() for r in g.schedule_batch(hs, assume=True)]
                assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
            single += len(pods) if step != "batch" else 0
            for j, (rg, ro) in enumerate(zip(got, want)):
                assert rg == ro, f"step {k} ({step}) pod {j}: {rg} != oracle {ro}"
                if rg[0] == 0 and rg[1] >= 0:
                    last = hs[j]
        elif step == "add_node":
            g.add_node(rgen.extra_node(arg))
        elif step == "forget":
            g.forget(last)
        elif step == "sleep":
            time.sleep(arg)
    assert g.resident_calls() == (0, single, 0)
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


# ---- 5. node-local pods in the same launch -------------------------------------------------------------------------
def test_node_local_pods_between_pod_table_pods(native):
    """600 nodes at 30 %: the two leading node-local pods are served by the resident k_sched_loop; the first
    pod-table pod starts k_agg_loop's launch, which then takes the node-local pods between the others too."""
    cfg, nodes, bound, pods, want = rgen.mixed_reference(30)
    g = device(native, cfg, nodes, bound)
    got = calls(g, pods)
    assert g.resident_calls() == (rgen.MIXED_LEAD, len(pods) - rgen.MIXED_LEAD, 0)
    check(g, got, want)


# ---- 6. unchanged behaviour ----------------------------------------------------------------------------------------
def test_percentage_100_is_the_same_with_the_key_on_or_off(native):
    """Nothing is sampled: the existing resident instance serves every call whatever the key says."""
    cfg, nodes, bound, pods, want = gen.reference("130", "five", True, 100)
    assert not any(c.cut for c in want)
    out = []
    for key in (True, False):
        g = device(native, dict(cfg, residentAggSampled=key), nodes, bound)
        got = calls(g, pods)
        assert g.resident_calls() == (0, len(pods), 0)
        check(g, got, want, f"residentAggSampled {key}:")
        out.append(got)
    assert out[0] == out[1]
