"""Nominated pods on node-sharded contexts created with "distributed": {..., "nominations": true} (DESIGN.md §6
"Nominated pods when sharded"): a pod's own status.nominatedNodeName (the owner rank's single-node pass, its outcome on
every replica behind one all-reduce) and the other pods' nominations under nominatedPods "Evaluate" (the nominee table
staged alike on every rank: the all-reduce path, and both persistent loops over the device exchange).

In-process groups, each rank driven from its own thread with a deadline.  Every test checks on every rank that the
results equal the reference pod by pod, that no loop gave up or was re-run, and that the mirror equals the cache.
References: the oracle (own nominations) and tests/nominated_reference.py ("Evaluate"), OpportunisticBatching off as
on every node-sharded context.  tests/test_sharded_nominated_reference.py checks, on the references alone, that every
non-empty rank's range decides something in these streams."""
import functools
import re
import uuid

import pytest

from fuzz_gen import namespaces
from ksg.abi import KSG_EINVAL, KsgError
from nominated_reference import NominatedReference
from nominated_preempt_reference import NAMESPACES2, PREEMPT_ALL, hand_cases as preempt_hand_cases
from nominated_topology_reference import (NAMESPACE as TOPO_NAMESPACE, SIZES, NominatedTopologyReference,
                                          hand_cases as topology_hand_cases, stream_reference)
from nominator_scenario import node as plain_node, pod as plain_pod
from sharded_nominated_cases import (EVAL_NODES, GATE_OFF, OWN_MODES, agg_class_case, evaluate_reference,
                                     own_reference, preemption_all_steps, preemption_steps)
from test_gpu_nominated_pods import check_eval, nominee
from test_gpu_sharded_diagnosis import close, on_ranks

pytestmark = pytest.mark.gpu

TOPO_CASES = topology_hand_cases()
PREEMPT_CASES = preempt_hand_cases()


def group(world, cfg, nodes, existing=(), nss=(), objects=(), nominations=True, extra=None):
    """W in-process ranks on one device, every one holding the whole cluster.  nominations: the opt-in of every rank,
    or one value per rank; None leaves the key out.  extra: further "distributed" keys."""
    from ksg.native import Scheduler
    name = f"sn-{uuid.uuid4().hex[:8]}"
    flags = nominations if isinstance(nominations, (list, tuple)) else [nominations] * world
    ranks = []
    for r in range(world):
        dist = dict(extra or {}, worldSize=world, rank=r, localGroup=name)
        if flags[r] is not None:
            dist["nominations"] = flags[r]
        s = Scheduler(dict(cfg, device=0, featureGates=GATE_OFF, distributed=dist))
        for ns in nss:
            s.upsert_namespace(ns)
        for o in objects:
            s.upsert_object(o)
        for n in nodes:
            s.add_node(n)
        for p in existing:
            s.add_pod(p)
        ranks.append(s)
    return ranks


def nominate_all(ranks, noms):
    """The same ksg_add_nominated_pod calls on every rank, in the same order (the opt-in's contract)."""
    for s in ranks:
        for q in noms:
            s.add_nominated_pod(q)


def run(ranks, pods, mode):
    """-> per rank [(result tuple, evaluation output or None)]: one batch, one-pod calls, or those with output."""
    def work(r, s):
        if mode == "batch":
            return [(t.as_tuple(), None) for t in s.schedule_batch([s.compile(p) for p in pods], assume=True)]
        out = []
        for p in pods:
            res, ev = s.schedule_one(s.compile(p), assume=True, evaluate=mode == "eval")
            out.append((res.as_tuple(), ev))
        return out

    got = on_ranks(ranks, work)
    errs = [f"rank {r}: {g!r}" for r, g in enumerate(got) if isinstance(g, Exception)]
    if errs:
        pytest.fail("\n".join(errs), pytrace=False)
    return got


def healthy(ranks, tag):
    for r, s in enumerate(ranks):
        assert s.loop_stats() == (0, 0), f"{tag} rank {r}: loop give-ups / re-runs"
        assert s.compare_mirror(sync=True)[0] == 0, f"{tag} rank {r}: mirror != cache"


# ---- 1. the opt-in ----------------------------------------------------------------------------------------------------
def test_nominations_key_needs_a_transport():
    from ksg.native import Scheduler
    with pytest.raises(Exception, match="distributed.nominations"):
        Scheduler({"device": 0, "distributed": {"worldSize": 1, "rank": 0, "nominations": True}})


def test_ranks_that_disagree_get_einval_and_schedule_nothing():
    nodes = [plain_node(f"n{k}") for k in range(4)]
    nss = [{"metadata": {"name": "default"}}]
    ranks = group(2, {}, nodes, (), nss, nominations=[True, False])
    pod = plain_pod("p", prio=0, cpu="1")

    def call(r, s):
        h = s.compile(pod)
        codes = []
        for f in (lambda: s.schedule_one(h, assume=True), lambda: s.schedule_batch([h], assume=True)):
            with pytest.raises(KsgError, match="distributed.nominations") as e:
                f()
            codes.append(int(re.search(r"rc=(-?\d+)", str(e.value)).group(1)))
        return codes

    got = on_ranks(ranks, call)
    assert got == [[KSG_EINVAL, KSG_EINVAL]] * 2, got
    for s in ranks:  # nothing was scheduled on either replica: no assume reached the cache (4 node events)
        assert s.compare_mirror(sync=True)[0] == 0 and s.generation()[1] == len(nodes)
    close(ranks)


def test_all_three_values_are_accepted_and_a_nominated_pod_compiles():
    nodes = [plain_node(f"n{k}") for k in range(4)]
    for cfg in ({"nominatedPods": "Refuse"}, {"nominatedPods": "Evaluate"}, {"nominatedPods": "EvaluateAll"},
                {"nominatedPods": "EvaluateAll", "preemptNominatedPods": "EvaluateAll"}):
        ranks = group(2, cfg, nodes, (), [{"metadata": {"name": "default"}}])
        for s in ranks:
            s.compile(plain_pod("own", prio=0, cpu="1", nominated="n1"))
        close(ranks)


def test_rccl_single_rank_runs_a_stream_under_evaluate():
    """The RCCL transport on the one rank a one-GPU machine can host: the loops' overlay instances with the RCCL ranks'
    default device exchange, the nominees' own cycles over the all-reduce path."""
    from ksg.native import Scheduler, comm_unique_id
    cfg, nodes, existing, noms, pods, want = evaluate_reference(257)
    s = Scheduler(dict(cfg, device=0, featureGates=GATE_OFF, nominatedPods="Evaluate",
                       distributed={"worldSize": 1, "rank": 0, "ncclId": comm_unique_id(), "nominations": True}))
    for ns in namespaces():
        s.upsert_namespace(ns)
    for n in nodes:
        s.add_node(n)
    for p in existing:
        s.add_pod(p)
    nominate_all([s], noms)
    got = run([s], pods, "batch")[0]
    for k in range(len(pods)):
        assert got[k][0] == want[k][0], f"pod {k}: {got[k][0]} != reference {want[k][0]}"
    healthy([s], "RCCL W=1:")
    s.close()


# ---- 2. the pod's own nominated node against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("pct,mode", OWN_MODES)
def test_own_nominations_match_oracle(pct, mode, world, dx):
    """700 nodes, three blocks: W = 2 owns [0, 256) and [256, 700), W = 3 a block each.  Pods nominated to nodes of
    every rank's range are placed there, or fail there alone and go through the full pass (the failed node once in
    EvaluatedNodes and nextStartNodeIndex), with directed pods at snapshot indices 255, 256 and in the last block."""
    cfg, nodes, existing, pods, want = own_reference(pct, mode)
    ranks = group(world, dict(cfg, deviceExchange=dx), nodes, existing, namespaces())
    got = run(ranks, pods, mode)
    tag = f"pct {pct}, {mode}, W={world}, deviceExchange={dx}:"
    for r in range(world):
        for k in range(len(pods)):
            assert got[r][k][0] == want[k][0], f"{tag} rank {r} pod {k}: {got[r][k][0]} != oracle {want[k][0]}"
            if mode == "eval":
                assert got[r][k][1] == want[k][1], f"{tag} rank {r} pod {k}: evaluation output differs"
    healthy(ranks, tag)
    close(ranks)


# ---- 3. "Evaluate" against NominatedReference ---------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
@pytest.mark.parametrize("mode", ["batch", "eval"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_nodes", EVAL_NODES)
def test_evaluate_matches_reference(n_nodes, world, mode, dx):
    """9 and 130 nodes: one block, every rank but the last is empty; 257: two blocks, the second of one node (W = 3:
    rank 0 empty); 600: three blocks.  The streams hold two nominees' own cycles."""
    cfg, nodes, existing, noms, pods, want = evaluate_reference(n_nodes)
    ranks = group(world, dict(cfg, nominatedPods="Evaluate", deviceExchange=dx), nodes, existing, namespaces())
    nominate_all(ranks, noms)
    got = run(ranks, pods, mode)
    tag = f"{n_nodes} nodes, {mode}, W={world}, deviceExchange={dx}:"
    for r in range(world):
        for k in range(len(pods)):
            assert got[r][k][0] == want[k][0], f"{tag} rank {r} pod {k}: {got[r][k][0]} != reference {want[k][0]}"
            if mode == "eval" and want[k][1]["feasible"]:  # (not the pod's own nominated node tried alone)
                check_eval(got[r][k][1], want[k][1], n_nodes, f"{tag} rank {r} pod {k}")
    healthy(ranks, tag)
    close(ranks)


# ---- 4. a batch holding the nominees themselves -------------------------------------------------------------------------
def test_batch_holding_the_nominees_themselves_keeps_plain_pods_in_the_loop():
    """The A/B case of test_gpu_nominated_pods on a W = 2 deviceExchange group: each nominated pod is a run of its
    own, so the plain pods around them still run in k_sched_loop."""
    nodes = [plain_node(f"n{k}") for k in range(8)]
    nss = [{"metadata": {"name": "default"}}]
    ranks = group(2, {"nominatedPods": "Evaluate", "deviceExchange": True}, nodes, (), nss)
    ref = NominatedReference({"featureGates": GATE_OFF}, nodes, [], nss)
    a = plain_pod("A", prio=100, cpu="3000m", nominated="n1")
    b = plain_pod("B", prio=50, cpu="2000m", nominated="n1")
    nominate_all(ranks + [ref], [a, b])
    pods = ([plain_pod(f"p{k}", prio=0, cpu="1") for k in range(5)] + [b] +
            [plain_pod(f"p{k}", prio=60, cpu="1500m") for k in range(5, 10)] + [a] +
            [plain_pod(f"p{k}", prio=0, cpu="1") for k in range(10, 15)])
    got = run(ranks, pods, "batch")
    want = [ref.schedule(p) for p in pods]
    n1 = ref.index["n1"]
    assert want[5][0] == 0 and want[5][1] != n1 and want[11] == (0, n1, 1, 1, 0)
    for r, s in enumerate(ranks):
        assert [t for t, _ in got[r]] == want, f"rank {r}"
        assert s.kernel_stats()[3] == "k_sched_loop", f"rank {r}: {s.kernel_stats()}"  # the last run: p10..p14
        # every one of the three plain runs went to k_sched_loop: all 15 plain pods were handed to it, A and B never
        assert sum(s.lean_pods()) == 15, f"rank {r}: {s.lean_pods()}"
    healthy(ranks, "A/B batch:")
    close(ranks)


# ---- 5. k_agg_loop's class under nominations ------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_agg_loop_class_under_nominations(world):
    cfg, nodes, init, objects, noms, pods, want = agg_class_case()
    ranks = group(world, dict(cfg, nominatedPods="Evaluate", deviceExchange=True), nodes, init, namespaces(), objects)
    nominate_all(ranks, noms)
    got = run(ranks, pods, "batch")
    for r, s in enumerate(ranks):
        for k in range(len(pods)):
            assert got[r][k][0] == want[k], f"W={world} rank {r} pod {k}: {got[r][k][0]} != reference {want[k]}"
        assert s.kernel_stats()[3] == "k_agg_loop", f"rank {r}: {s.kernel_stats()}"
    healthy(ranks, f"agg class, W={world}:")
    close(ranks)


# ---- 6. "EvaluateAll" ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def topology_reference(family, n_nodes):
    return stream_reference(family, n_nodes)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", TOPO_CASES, ids=[c[0] for c in TOPO_CASES])
def test_evaluate_all_hand_computed_cases_on_every_rank(case, world):
    """nominated_topology_reference's hand-computed cases (the only ones whose expected statuses are literals): every
    rank returns the literal status of every failing node in the gathered evaluation output, the literal result, and
    the reference's; then the same cycle without output, and assumed."""
    name, nodes, existing, noms, pod, failing, (status, evaluated, feasible) = case
    ranks = group(world, {"nominatedPods": "EvaluateAll"}, nodes, existing, TOPO_NAMESPACE)
    nominate_all(ranks, noms)
    ref = NominatedTopologyReference({"featureGates": GATE_OFF}, nodes, existing, TOPO_NAMESPACE)
    for q in noms:
        ref.add_nominated_pod(q)
    d = {}
    want = ref.schedule(pod, assume=False, detail=d)
    d["weights"] = ref.weights
    want2, want3 = ref.schedule(pod, assume=False), ref.schedule(pod, assume=True)

    def call(r, s):
        rg, eg = s.schedule_one(s.compile(pod), assume=False, evaluate=True)
        for nm, i in ref.index.items():
            st = (eg["node_code"][i], eg["node_plugin"][i], eg["node_reasons"][i])
            assert st == failing[nm] if nm in failing else st[0] == 0, (name, r, nm, st)
        assert rg.as_tuple() == want, (name, r, rg.as_tuple(), want)
        assert (rg.status, rg.evaluated_nodes, rg.feasible_nodes) == (status, evaluated, feasible)
        check_eval(eg, d, len(nodes), f"{name} rank {r}")
        assert s.schedule_one(s.compile(pod), assume=False)[0].as_tuple() == want2, (name, r)
        assert s.schedule_one(s.compile(pod), assume=True)[0].as_tuple() == want3, (name, r)
        return True

    assert on_ranks(ranks, call) == [True] * world
    healthy(ranks, f"{name}, W={world}:")
    close(ranks)


@pytest.mark.parametrize("mode,dx", [("batch", True), ("batch", False), ("eval", False)], ids=["batch-devx", "batch", "eval"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_nodes", SIZES)
@pytest.mark.parametrize("family", ["directed", "random"])
def test_evaluate_all_streams_match_reference(family, n_nodes, world, mode, dx):
    """test_gpu_nominated_topology.py's streams: marked pods (a nominee may move a spread or affinity count they read)
    take the all-reduce path with k_nom_topo's deltas replicated and the two-pass instances over the rank's blocks;
    the nominees' own cycles take the two-pass owner pass."""
    cfg, nodes, existing, noms, pods, want, _ = topology_reference(family, n_nodes)
    ranks = group(world, dict(cfg, nominatedPods="EvaluateAll", deviceExchange=dx), nodes, existing, namespaces())
    nominate_all(ranks, noms)
    got = run(ranks, pods, mode)
    tag = f"{family}, {n_nodes} nodes, {mode}, W={world}, deviceExchange={dx}:"
    for r in range(world):
        for k in range(len(pods)):
            assert got[r][k][0] == want[k][0], f"{tag} rank {r} pod {k}: {got[r][k][0]} != reference {want[k][0]}"
            if mode == "eval" and want[k][1]["feasible"]:
                check_eval(got[r][k][1], want[k][1], n_nodes, f"{tag} rank {r} pod {k}")
    healthy(ranks, tag)
    close(ranks)


# ---- 7. preemption end to end -------------------------------------------------------------------------------------------
def test_preemption_stream_end_to_end():
    """preempt -> delete the victims -> nominate on every rank -> schedule others under the nomination -> the nominee's
    own cycle, on a W = 2 group under "Evaluate" (300 nodes: both ranks own nodes).  Every rank replays the steps with
    the reference's answers; ksg_preempt is replicated per rank and returns the same node and victims on each."""
    steps = preemption_steps()
    nodes, low, nss = steps[0]
    ranks = group(2, {"nominatedPods": "Evaluate", "deviceExchange": True}, nodes, low, nss)
    got = on_ranks(ranks, lambda r, s: replay(r, s, steps[1:]))
    assert got == [True, True], got
    healthy(ranks, "preemption stream:")
    close(ranks)


def replay(r, s, steps):
    """One rank's side of a stream of steps (sharded_nominated_cases.preemption_steps) against the reference's answers."""
    for k, st in enumerate(steps):
        if st[0] == "one":
            got = s.schedule_one(s.compile(st[1]), assume=True)[0].as_tuple()
            assert got == st[2], f"rank {r} step {k} ({st[1]['metadata']['name']}): {got} != reference {st[2]}"
        elif st[0] == "batch":
            got = [t.as_tuple() for t in s.schedule_batch([s.compile(p) for p in st[1]], assume=True)]
            assert got == st[2], f"rank {r} step {k}: {got} != reference {st[2]}"
        elif st[0] == "preempt":
            res, d = s.preempt(s.compile(st[1]), st[2])
            assert res.as_tuple() == st[3], f"rank {r} step {k}: preempt {res.as_tuple()} != reference {st[3]}"
            assert d == st[4], f"rank {r} step {k}: preempt detail {d} != reference {st[4]}"
        elif st[0] == "remove":
            s.remove_pod(st[1])
        else:
            s.add_nominated_pod(st[1])
    return True


@pytest.mark.parametrize("dx", [True, False], ids=["devx", "allreduce"])
def test_preemption_stream_end_to_end_under_evaluate_all(dx):
    """The same shape under "nominatedPods": "EvaluateAll" + "preemptNominatedPods": "EvaluateAll", against
    nominated_preempt_reference: spread-constrained preemptors on 288 full nodes in 3 zones (two blocks).  Each failed
    cycle is a marked pod's (k_nom_topo replicated, the two-pass instances over the rank's blocks), each ksg_preempt
    the replicated two-pass dry run with the rank's own table staged; every rank returns the same node and victims,
    and the nominated nodes lie in both ranks' ranges."""
    steps, _ = preemption_all_steps()
    nodes, lows, nss = steps[0]
    ranks = group(2, dict(PREEMPT_ALL, deviceExchange=dx), nodes, lows, nss)
    got = on_ranks(ranks, lambda r, s: replay(r, s, steps[1:]))
    assert got == [True, True], got
    healthy(ranks, f"EvaluateAll preemption stream, deviceExchange={dx}:")
    close(ranks)


@pytest.mark.parametrize("case", PREEMPT_CASES, ids=[c[0] for c in PREEMPT_CASES])
def test_preempt_hand_computed_cases_on_every_rank(case):
    """nominated_preempt_reference's hand-computed dry runs on a W = 2 group: the literals on every rank."""
    name, nodes, existing, noms, pod, args, want, cands, selected, _ = case
    ranks = group(2, dict(PREEMPT_ALL), nodes, existing, NAMESPACES2)
    nominate_all(ranks, noms)

    def call(r, s):
        for extra in ({}, {"debugHostStaged": True}):
            res, d = s.preempt(s.compile(pod), dict(args, **extra))
            assert res.as_tuple() == want, (name, r, extra, res.as_tuple(), want)
            assert {c["node"]: c["victims"] for c in d["candidates"]} == cands, (name, r, extra, d)
            assert d["selected"] == selected
        return True

    assert on_ranks(ranks, call) == [True, True]
    healthy(ranks, name)
    close(ranks)


# ---- 8. a diagnosed stream under nominations ------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
def test_diagnosed_stream_with_own_nominations(dx):
    """"diagnosis": true and "nominations": true together: the 700-node stream of case 2 through
    ksg_schedule_batch_diag.  A failed nominated node's status word is stored by its owner rank and counted in that
    rank's rows once, as the node's status of the full pass."""
    from diagnosis_reference import fill, reference_stream
    from oracle_binding import oracle
    from test_gpu_diagnosis import run_diag
    cfg, nodes, existing, pods, _ = own_reference(100, "batch")
    want = reference_stream(fill(oracle(dict(cfg, featureGates=GATE_OFF)), nodes, existing, namespaces()), pods)
    assert sum(r[0] == 2 for r, _ in want) >= 3
    ranks = group(2, dict(cfg, deviceExchange=dx), nodes, existing, namespaces(), extra={"diagnosis": True})
    got = on_ranks(ranks, lambda r, s: run_diag(s, pods, "batch"))
    for r, s in enumerate(ranks):
        assert not isinstance(got[r], Exception), got[r]
        for k, ((rg, dg), (ro, do)) in enumerate(zip(got[r], want)):
            assert rg == ro, f"rank {r} pod {k}: result {rg} != reference {ro}"
            assert dg == do, f"rank {r} pod {k} (status {ro[0]}): diagnosis\n {dg}\n != reference\n {do}"
    healthy(ranks, f"diagnosed, deviceExchange={dx}:")
    close(ranks)


# ---- 9. which group kernel a launch dispatches ------------------------------------------------------------------------------
def test_nothing_nominated_dispatches_the_plain_group_kernel():
    """By the dispatched kernel's name (ksg_debug_group_loop_kernel: the runtime's name of the function the leader
    launched): without the opt-in, and with it while nothing is nominated, a group's batch runs the same
    k_sched_loop_group instance as before; with a nomination outstanding it runs k_sched_loop_group_nom."""
    from ksg.native import group_loop_kernel
    nodes = [plain_node(f"n{k:03d}") for k in range(40)]
    nss = [{"metadata": {"name": "default"}}]
    pods = [plain_pod(f"p{k}", prio=0, cpu="500m") for k in range(8)]
    names = []
    for cfg, flag, noms in (({}, None, []), ({"nominatedPods": "Evaluate"}, True, []),
                            ({"nominatedPods": "Evaluate"}, True, [nominee("held", 100, "n003", cpu="3")])):
        ranks = group(2, dict(cfg, deviceExchange=True), nodes, (), nss, nominations=flag)
        nominate_all(ranks, noms)
        got = run(ranks, pods, "batch")
        assert all(t[0] == 0 for t, _ in got[0]) and got[0] == got[1]
        assert {s.kernel_stats()[3] for s in ranks} == {"k_sched_loop"}
        names.append(group_loop_kernel())
        healthy(ranks, f"{cfg}, {flag}, {len(noms)} nominees:")
        close(ranks)
    # (the template arguments follow the name at once: "I" in the mangled symbol, "<" if the runtime demangles it)
    assert re.search(r"k_sched_loop_group[I<]", names[0]), names
    assert names[1] == names[0], names
    assert re.search(r"k_sched_loop_group_nom[I<]", names[2]), names


# ---- 10. a mismatched nominee table never launches a group's loop ---------------------------------------------------------
def test_table_staged_on_one_rank_only_launches_nothing():
    """The ranks break the contract (one receives a nomination the other does not): the leader's check at the group
    launch returns KSG_EINVAL on every rank instead of running different instances."""
    nodes = [plain_node(f"n{k:03d}") for k in range(40)]
    nss = [{"metadata": {"name": "default"}}]
    ranks = group(2, {"nominatedPods": "Evaluate", "deviceExchange": True}, nodes, (), nss)
    ranks[1].add_nominated_pod(nominee("held", 100, "n003", cpu="3"))
    pods = [plain_pod(f"p{k}", prio=0, cpu="500m") for k in range(8)]

    def call(r, s):
        with pytest.raises(KsgError, match="nominee table") as e:
            s.schedule_batch([s.compile(p) for p in pods], assume=True)
        return int(re.search(r"rc=(-?\d+)", str(e.value)).group(1))

    assert on_ranks(ranks, call) == [KSG_EINVAL, KSG_EINVAL]
    close(ranks)
