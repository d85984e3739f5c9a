"""Sampled pods inside k_agg_loop (config "aggLoopSampled", default on; DESIGN.md §4.5 "Inside k_agg_loop"): with
percentageOfNodesToScore below 100 (0, upstream's adaptive default, included), a no-score profile or a nominated pod
in the batch, a batch's PodTopologySpread / InterPodAffinity pods run in the persistent loop's sampling instances,
which cut the feasible list and carry nextStartNodeIndex themselves.

Every comparison is against the oracle pod by pod -- node, TotalScore, FeasibleNodes, EvaluatedNodes (the whole result
tuple) -- and every stream ends with the mirror equal to the host's cache and no loop give-up.  The inputs are
tests/agg_sampled_gen.py's; tests/test_agg_sampled_inputs.py checks on the oracle alone that they exercise the cut."""
import functools

import pytest

import agg_sampled_gen as gen
from oracle_binding import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


def device(native, cfg, nodes, bound):
    return gen.fill(native(dict(cfg, device=0)), nodes, bound)


def run(g, pods):
    return [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]


def check(g, got, want, tag=""):
    assert len(got) == len(want)
    for k, (rg, c) in enumerate(zip(got, want)):
        ro = c.result if isinstance(c, gen.Cycle) else c
        assert rg == ro, f"{tag} pod {k}: {rg} != oracle {ro}"
    assert g.compare_mirror(sync=True) == (0, -1)
    assert g.loop_stats() == (0, 0)


# ---- 1. the routing ------------------------------------------------------------------------------------------------
def test_sampled_batch_runs_in_the_loop_and_the_key_turns_it_off(native):
    """percentageOfNodesToScore 0 (adaptive: 48 % of 257 nodes): the batch's last run is k_agg_loop's; with
    "aggLoopSampled": false it takes the per-pod launches.  Both equal the oracle."""
    cfg, nodes, bound, pods, want = gen.reference("257", "three", True, 0)
    assert sum(c.cut for c in want) >= 5
    g = device(native, cfg, nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    check(g, got, want, "on:")
    off = device(native, dict(cfg, aggLoopSampled=False), nodes, bound)
    got_off = run(off, pods)
    assert off.kernel_stats()[3] == "k_filter_score"
    check(off, got_off, want, "off:")


# ---- 2. shapes, percentages, the no-score profile ----------------------------------------------------------------
SHAPES = ["9", "130", "257", "600", "600-one-workgroup"]


@pytest.mark.parametrize("pct", [0, 7, 30, 55])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_percentages(native, shape, pct):
    """9 nodes: N < 100, the rotation is carried and nothing is cut; 130: K = 100 in one workgroup; 257: two
    workgroups, the second with one node; 600, and 600 with one workgroup owning every node block.  The streams with
    ScheduleAnyway constraints (the PodTopologySpread-scoring instances) at percentages 0 and 30, the ones without at 7
    and 55."""
    soft = pct in (0, 30)
    cfg, nodes, bound, pods, want = gen.reference(shape, "five", soft, pct)
    g = device(native, cfg, nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    check(g, got, want, f"{shape} pct {pct}:")


@pytest.mark.parametrize("pct", [100, 20])
@pytest.mark.parametrize("shape", ["130", "600"])
def test_no_score_profile(native, shape, pct):
    """No score plugin (tests/test_gpu_parity.py's NO_SCORE: the seven score plugins disabled): numNodesToFind is 1
    whatever the percentage (schedule_one.go:780-782), so every pod with two feasible nodes is cut to one and the
    rotation advances by the failures before the second.  A plugin is disabled as a whole, so in this profile the
    streams' pods have no PodTopologySpread / InterPodAffinity work left and no pod is of k_agg_loop's class: the
    case pins that the new admission rule leaves the profile's routing and results alone."""
    cfg, nodes, bound, pods, want = gen.reference(shape, "three", False, pct, no_score=True)
    assert sum(c.placed and c.feasible == 1 and c.evaluated < c.n for c in want) >= 20
    g = device(native, cfg, nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[3] == "k_sched_loop"
    check(g, got, want, f"{shape} no-score pct {pct}:")


# ---- 3. both instance families -----------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
@pytest.mark.parametrize("kind", gen.STREAMS)
def test_with_and_without_schedule_anyway_constraints(native, kind, soft):
    cfg, nodes, bound, pods, want = gen.reference("600", kind, soft, 30)
    g = device(native, cfg, nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    check(g, got, want, f"{kind} soft {soft}:")


@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
def test_more_than_64_workgroups(native, soft):
    """64 * 256 + 6 nodes: 65 workgroups, the instances whose sweeps take more than one round of 64 participants."""
    cfg, nodes, bound, pods, want = gen.reference("big", "three", soft, 45, n_pods=16)
    g = device(native, cfg, nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    check(g, got, want, f"soft {soft}:")


# ---- 4. the loop's shortcuts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", [0, 1, 4, 32])
@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
@pytest.mark.parametrize("kind", ["three", "five"])
def test_shortcuts_agree(native, kind, soft, debug):
    """aggLoopDebug 1: no fold (every pod gathers after the placement before it), 4: no same-template shortcut, 32: no
    template cache.  All equal the oracle, so they equal each other."""
    cfg, nodes, bound, pods, want = gen.reference("257", kind, soft, 7)
    g = device(native, dict(cfg, aggLoopDebug=debug), nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
    check(g, got, want, f"{kind} soft {soft} aggLoopDebug {debug}:")


# ---- 5. mixed batches --------------------------------------------------------------------------------------------
def plain(name):  # node-local: a k_sched_loop pod, sampled too
    return gen.base(name, "plain", cpu="300m", ipa=False).obj()


def spread_only(name, k):
    """Loop-class pods without affinity terms (no pod of the cluster carries one, so the plain pods stay node-local):
    zone DoNotSchedule + hostname ScheduleAnyway, or the hostname spread honouring node affinity and taints."""
    if k % 3 == 2:
        return gen.base(name, "hs", ipa=False).spread(1, gen.HOST, "DoNotSchedule", gen.sel("hs"), node_affinity_policy="Honor",
                                                      node_taints_policy="Honor")
    return (gen.base(name, "zs", ipa=False).spread(2, gen.ZONE, "DoNotSchedule", gen.sel("zs"))
            .spread(1, gen.HOST, "ScheduleAnyway", gen.sel("zs")))


def subset(name, names):
    """matchFields: a PreFilterResult subset, on the per-pod launches.  One term per node name: the Filter's field
    selector takes a single value per requirement (terms are ORed), the PreFilterResult is the union."""
    return spread_only(name, 2).node_affinity_required(
        [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": [n]}]} for n in names]).obj()


@functools.lru_cache(maxsize=None)
def mixed_reference(pct):
    """Two consecutive batches of 48: loop-class pods in runs of three, node-local pods in runs of two between them,
    one matchFields pod in each batch.  The rotation crosses k_agg_loop, k_sched_loop and the launches."""
    nodes, _ = gen.shape_cluster("600")
    bound = []  # (no bound pod with an affinity term either)
    cfg = {"percentageOfNodesToScore": pct}
    batches, k = [], 0
    for b in range(2):
        pods = []
        for j in range(48):
            if j == 20:
                pods.append(subset(f"sub{b}", [f"n{x:05d}" for x in range(50 + 100 * b, 170 + 100 * b)]))
            elif j % 5 >= 3:
                pods.append(plain(f"plain{b}-{j}"))
            else:
                pods.append(spread_only(f"class{k}", k).obj())
                k += 1
        batches.append(pods)
    want, o = gen.run_oracle(cfg, nodes, bound, batches[0])
    want2, o = gen.run_oracle(cfg, nodes, bound, batches[1], o)
    o.close()
    for pods, w in zip(batches, (want, want2)):
        assert all(c.placed for c in w) and w[20].feasible > 1
        for app in ("plain", "zs", "hs"):  # cut pods of both loops' classes
            assert sum(c.cut for p, c in zip(pods, w) if p["metadata"]["labels"]["app"] == app) >= 5, app
    return cfg, nodes, bound, batches, [want, want2]


@pytest.mark.parametrize("pct", [0, 30])
def test_rotation_crosses_both_loops_and_the_launch_path(native, pct):
    cfg, nodes, bound, batches, wants = mixed_reference(pct)
    g = device(native, cfg, nodes, bound)
    for b, (pods, want) in enumerate(zip(batches, wants)):
        got = run(g, pods)
        ms, by, launches, kernel = g.kernel_stats()
        assert (launches, kernel) == (sum(p["metadata"]["labels"]["app"] != "plain" for p in pods) - 1, "k_agg_loop")
        check(g, got, want, f"batch {b}:")


@functools.lru_cache(maxsize=None)
def nominated_reference():
    """percentageOfNodesToScore 100 and one pod with status.nominatedNodeName in the batch: nextStartNodeIndex lives
    on the device for the whole batch (the nominated pod's outcome decides whether it moves)."""
    nodes, bound = gen.shape_cluster("257")
    pods = gen.stream("three", False, 40)
    nom = plain("nominated")
    nom["status"] = {"nominatedNodeName": "n00030"}
    pods[17:17] = [nom]
    o = gen.fill(oracle({}), nodes, bound)
    want = [o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in pods]
    assert want[17][:4] == (0, o.node_names().index("n00030"), 1, 1)  # placed on its nominated node, alone
    o.close()
    return nodes, bound, pods, want


def test_one_nominated_pod_leaves_the_others_in_the_loop(native):
    nodes, bound, pods, want = nominated_reference()
    g = device(native, {}, nodes, bound)
    got = run(g, pods)
    assert g.kernel_stats()[2:] == (len(pods) - 1, "k_agg_loop")
    check(g, got, want)


# ---- 6. unchanged behaviour ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
@pytest.mark.parametrize("kind", gen.STREAMS)
def test_percentage_100_is_the_same_with_the_key_on_or_off(native, kind, soft):
    cfg, nodes, bound, pods, want = gen.reference("600", kind, soft, 100)
    assert not any(c.cut for c in want)
    out = []
    for key in (True, False):
        g = device(native, dict(cfg, aggLoopSampled=key), nodes, bound)
        got = run(g, pods)
        assert g.kernel_stats()[2:] == (len(pods), "k_agg_loop")
        check(g, got, want, f"aggLoopSampled {key}:")
        out.append(got)
    assert out[0] == out[1]
