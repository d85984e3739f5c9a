"""ksg_schedule_one_diag / ksg_schedule_batch_diag on node-sharded contexts created with
"distributed": {..., "diagnosis": true} (DESIGN.md §6 "Diagnosis when sharded"): the calls are collective, every rank
returns the same results and the same complete, cluster-wide ksg_diagnosis per pod.

Reference: tests/diagnosis_reference.py (the oracle pod by pod, each failing cycle's evaluation output reduced in
Python), OpportunisticBatching off as on every node-sharded context.  Every test drives each rank from its own
thread, checks every rank's (result, diagnosis) of every pod, and that no rank's loop gave up or was re-run and that
every rank's mirror equals its cache."""
import functools
import re
import threading
import time
import uuid

import pytest

from diagnosis_reference import FIT_ERROR, fill, reduce_eval, reference_stream
from fuzz_gen import namespaces
from ksg.abi import KSG_EINVAL, KSG_ENOTSUP, PLUGIN_ID, KsgError
from ksg.objects import PodW
from oracle_binding import oracle
from test_gpu_diagnosis import NSS, ask, box, random_case, run_diag

pytestmark = pytest.mark.gpu

GATE_OFF = {"OpportunisticBatching": False}
DEVICE_KEYS = ("loopUnit", "deviceExchange")
ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"


def group(world, cfg, nodes, existing=(), nss=NSS, diagnosis=True):
    """W in-process ranks on one device, every one holding the whole cluster.  diagnosis: the opt-in of every rank,
    or one value per rank; None leaves the key out."""
    from ksg.native import Scheduler
    name = f"sd-{uuid.uuid4().hex[:8]}"
    flags = diagnosis if isinstance(diagnosis, (list, tuple)) else [diagnosis] * world
    ranks = []
    for r in range(world):
        dist = {"worldSize": world, "rank": r, "localGroup": name}
        if flags[r] is not None:
            dist["diagnosis"] = flags[r]
        ranks.append(fill(Scheduler(dict(cfg, device=0, featureGates=GATE_OFF, distributed=dist)), nodes, existing, nss))
    return ranks


def reference(cfg, nodes, existing=(), nss=NSS):
    ocfg = {k: v for k, v in cfg.items() if k not in DEVICE_KEYS}
    return fill(oracle(dict(ocfg, featureGates=GATE_OFF)), nodes, existing, nss)


def on_ranks(ranks, fn, timeout=120):
    """fn(rank index, context) on every rank at once, a thread each -> [fn's value or the exception it raised].
    A thread still alive at the deadline fails the test at once; nothing further is started."""
    out = [None] * len(ranks)

    def work(r):
        try:
            out[r] = fn(r, ranks[r])
        except Exception as e:  # handed to the caller
            out[r] = e

    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(len(ranks))]
    for t in ts:
        t.start()
    deadline = time.monotonic() + timeout
    for t in ts:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(ts) if t.is_alive()]
    if alive:
        pytest.fail(f"ranks {alive} did not return from a collective call within {timeout} s", pytrace=False)
    return out


def run_all(ranks, pods, how="batch"):
    got = on_ranks(ranks, lambda r, s: run_diag(s, pods, how))
    errs = [f"rank {r}: {g}" for r, g in enumerate(got) if isinstance(g, Exception)]
    if errs:
        pytest.fail("\n".join(errs), pytrace=False)
    return got


def check_all(ranks, got, want, tag=""):
    for r, (s, mine) in enumerate(zip(ranks, got)):
        assert len(mine) == len(want)
        for k, ((rg, dg), (ro, do)) in enumerate(zip(mine, want)):
            assert rg == ro, f"{tag} rank {r} pod {k}: result {rg} != reference {ro}"
            assert dg == do, f"{tag} rank {r} pod {k} (status {ro[0]}): diagnosis\n {dg}\n != reference\n {do}"
        assert s.loop_stats() == (0, 0), f"{tag} rank {r}: loop give-ups / re-runs"
        assert s.compare_mirror(sync=True)[0] == 0, f"{tag} rank {r}: mirror != cache"


def close(ranks):
    for s in ranks:
        s.close()


def dominant(ranks):
    return {s.kernel_stats()[3] for s in ranks}


def every_rank_contributes(ranks, o_fresh, pods):
    """On the reference's evaluation output alone: every FitError pod has a failed node in every rank's shard_range(),
    so a rank whose share is lost, or a sum that is skipped, changes the answer."""
    spans = [s.shard_range() for s in ranks]
    assert all(n > 0 for _, n in spans), spans
    fails = 0
    for k, p in enumerate(pods):
        r, ev = o_fresh.schedule_one(o_fresh.compile(p), assume=True, evaluate=True)
        if r.status not in FIT_ERROR:
            continue
        fails += 1
        for a, n in spans:
            assert any(ev["node_code"][a:a + n]), f"pod {k}: no failed node in [{a}, {a + n})"
    assert fails > 0
    return spans


# ---- 1. random streams ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_reference(n_nodes):
    cfg, nodes, existing, pods = random_case(n_nodes)
    want = reference_stream(reference(cfg, nodes, existing, namespaces()), pods)
    failed = sum(r[0] in FIT_ERROR for r, _ in want)
    assert 5 <= failed <= len(pods) // 2, failed
    assert all(d["failed_nodes"] > 0 for r, d in want if r[0] in FIT_ERROR and not d["prefilter_code"])
    return cfg, nodes, existing, pods, want


@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_nodes", [9, 130, 257, 600])
def test_random_streams_match_reference(n_nodes, world, dx):
    """9 and 130 nodes: one block, every rank but one is empty; 257: two blocks, the second of one node (W = 3: one
    empty rank); 600: three blocks."""
    cfg, nodes, existing, pods, want = random_reference(n_nodes)
    ranks = group(world, dict(cfg, deviceExchange=dx), nodes, existing, namespaces())
    check_all(ranks, run_all(ranks, pods), want, f"{n_nodes} nodes, W={world}, deviceExchange={dx}:")
    close(ranks)


# ---- 2. both ranks contribute, k_sched_loop ---------------------------------------------------------------------------
def two_block_cluster():
    """300 nodes, two blocks: the first 256 have 2 cpu / 8Gi, the other 44 have 4 cpu / 2Gi and every fourth of those
    is tainted -- a pod too big for all of them fails on cpu in block 0 and on memory or the taint in block 1."""
    return [box(f"n{k:03d}", cpu="2", mem="8Gi") if k < 256 else box(f"n{k:03d}", cpu="4", mem="2Gi", taint=k % 4 == 0)
            for k in range(300)]


def two_block_stream():
    lo = lambda name: ask(name, "1", "4Gi").obj()     # fits block 0 only (memory)
    hi = lambda name: ask(name, "3", "1Gi").obj()     # fits block 1 only (cpu)
    return ([ask("first", "5").obj()] + [f(f"a{k}") for k, f in enumerate([lo, hi] * 3)] +
            [ask("mid", "3", "3Gi").obj(), ask("mid2", "3", "9Gi").obj()] + [f(f"c{k}") for k, f in enumerate([hi, lo] * 3)] +
            [ask("late", "3", "3Gi").obj(), ask("last", "5", "9Gi").obj()])


@pytest.mark.parametrize("unit", [None, 256])
def test_both_ranks_contribute_in_k_sched_loop(unit):
    nodes, pods = two_block_cluster(), two_block_stream()
    cfg = {"deviceExchange": True}
    if unit:
        cfg["loopUnit"] = unit
    want = reference_stream(reference(cfg, nodes), pods)
    assert [r[0] for r, _ in want] == [2] + [0] * 6 + [2, 2] + [0] * 6 + [2, 2]
    landed = [r[1] for r, _ in want if r[0] == 0]
    assert any(i < 256 for i in landed) and any(i >= 256 for i in landed)  # pods land on both ranks' nodes
    cpu, mem, taint = 7, 8, 2
    mid = want[7][1]
    # block 0 and the three block-1 nodes a0..a5 took are short of cpu, the rest of block 1 of memory or tainted
    assert mid["reason_nodes"][cpu] == 259 and mid["reason_nodes"][mem] == 33 and mid["reason_nodes"][taint] == 11
    ranks = group(2, cfg, nodes)
    assert every_rank_contributes(ranks, reference(cfg, nodes), pods) == [(0, 256), (256, 44)]
    check_all(ranks, run_all(ranks, pods), want, f"unit {unit}:")
    assert dominant(ranks) == {"k_sched_loop"}
    close(ranks)


# ---- 3. every pod fails -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_every_pod_of_the_batch_fails(world):
    """Rows of consecutive pods do not leak into each other (W = 3: rank 0 is empty)."""
    nodes = two_block_cluster()
    pods = [ask(f"f{k}", "5" if k % 2 else "4500m", "9Gi" if k % 3 == 0 else "1Gi").obj() for k in range(12)]
    cfg = {"deviceExchange": True}
    want = reference_stream(reference(cfg, nodes), pods)
    assert all(r == (2, -1, 300, 0, 0) for r, _ in want)
    assert want[0][1]["reason_nodes"][8] == 289 and want[1][1]["reason_nodes"][8] == 0  # memory: every third pod
    ranks = group(world, cfg, nodes)
    check_all(ranks, run_all(ranks, pods), want, f"W={world}:")
    assert dominant(ranks) == {"k_sched_loop"}
    close(ranks)


# ---- 4. k_agg_loop's class --------------------------------------------------------------------------------------------
def zoned_520():
    """500 nodes in zone a, 20 tainted nodes in zone b (three blocks); two app=web pods and one app=db pod in zone a."""
    nodes = [box(f"za{k:03d}", labels={ZONE: "a"}) for k in range(500)] + \
            [box(f"zb{k:02d}", taint=True, labels={ZONE: "b"}) for k in range(20)]
    small = lambda name, app, node: PodW(name).label("app", app).container(image="i", requests={"cpu": "100m"}).node(node).obj()
    return nodes, [small("w0", "web", "za000"), small("w1", "web", "za300"), small("db0", "db", "za499")]


def class_stream(anyway):
    web = {"matchLabels": {"app": "web"}}

    def spread(name, skew):
        p = PodW(name).label("app", "web").container(image="i", requests={"cpu": "100m"}).spread(skew, ZONE, "DoNotSchedule", web)
        return (p.spread(1, HOST, "ScheduleAnyway", web) if anyway else p).obj()

    anti = lambda name, app: PodW(name).label("app", "x").container(image="i", requests={"cpu": "100m"}) \
        .pod_affinity(ZONE, {"matchLabels": {"app": app}}, anti=True).obj()
    return [spread("s-ok", 5), spread("s-fail", 1), anti("a-fail", "db"), anti("a-ok", "nothing"), spread("s-fail2", 2),
            anti("a-fail2", "db"), spread("s-ok2", 6), anti("a-ok2", "nothing")]


@pytest.mark.parametrize("world,anyway", [(2, False), (3, False), (2, True)])
def test_spread_and_anti_affinity_pods_that_fail(world, anyway):
    """DoNotSchedule spread pods whose only untainted zone is too full, and pods with a required anti-affinity term
    against a pod of that zone, among pods of the class that land; one case with a ScheduleAnyway constraint too."""
    nodes, existing = zoned_520()
    pods = class_stream(anyway)
    cfg = {"deviceExchange": True}
    want = reference_stream(reference(cfg, nodes, existing), pods)
    assert [r[0] for r, _ in want] == [0, 2, 2, 0, 2, 2, 0, 0]
    pts, ipa = PLUGIN_ID["PodTopologySpread"], PLUGIN_ID["InterPodAffinity"]
    assert want[1][1]["plugin_nodes"][pts] == 500 and want[2][1]["plugin_nodes"][ipa] == 500
    ranks = group(world, cfg, nodes, existing)
    spans = every_rank_contributes(ranks, reference(cfg, nodes, existing), pods)
    assert len(spans) == world
    check_all(ranks, run_all(ranks, pods), want, f"W={world}, ScheduleAnyway={anyway}:")
    assert dominant(ranks) == {"k_agg_loop"}
    close(ranks)


# ---- 5. PreFilter cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
@pytest.mark.parametrize("how", ["batch", "one"])
def test_prefilter_rejection_and_matchfields_subset(how, dx):
    """An empty PreFilterResult, a PreFilter rejection, and a PreFilterResult subset whose nodes are full: each rank
    counts the nodes of its own range as the unsharded launch path counts all of them."""
    field = lambda names: [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": names}]}]
    nodes = two_block_cluster()
    nowhere = ask("nowhere", "1").node_affinity_required(field(["no-such-node"])).obj()
    reject = ask("reject", "1").node_affinity_required([{"matchFields": field(["n000"])[0]["matchFields"] +
                                                         field(["n299"])[0]["matchFields"]}]).obj()
    subset = ask("subset", "3", "3Gi").node_affinity_required(field(["n001", "n298", "n296"])).obj()
    pods = [ask("a", "1").obj(), ask("b", "3", "1Gi").obj(), nowhere, reject, subset, ask("fits", "1").obj()]
    cfg = {"deviceExchange": dx}
    want = reference_stream(reference(cfg, nodes), pods)
    assert [r[0] for r, _ in want] == [0, 0, 2, 2, 2, 0]
    assert want[2][1]["unschedulable_plugins"] == 0 and want[2][1]["reason_nodes"][16] == 300
    na = PLUGIN_ID["NodeAffinity"]
    assert (want[3][1]["prefilter_code"], want[3][1]["prefilter_plugin"], want[3][1]["plugin_nodes"][na]) == (3, na, 300)
    sub = want[4][1]
    assert sub["failed_nodes"] == 300 and sub["reason_nodes"][16] == 297 and sum(sub["plugin_nodes"]) == 3
    ranks = group(2, cfg, nodes)
    check_all(ranks, run_all(ranks, pods, how), want, f"{how}, deviceExchange={dx}:")
    close(ranks)


# ---- 6. sampled profile -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
def test_sampled_profile_with_no_feasible_node(dx):
    """percentageOfNodesToScore 10 on 300 nodes: the sampled pass stops at 100 feasible nodes, but a pod with none has
    evaluated every node, so its rows cover all 300."""
    nodes = [box(f"n{k:03d}", cpu="2", taint=k % 13 == 0) for k in range(300)]
    pods = [ask(f"p{k}", "1").obj() for k in range(6)] + [ask("big", "3").obj(), ask("p6", "2").obj(),
                                                          ask("big2", "2500m", "9Gi").obj()]
    cfg = {"percentageOfNodesToScore": 10, "deviceExchange": dx}
    want = reference_stream(reference(cfg, nodes), pods)
    assert [r[0] for r, _ in want] == [0] * 6 + [2, 0, 2]
    assert want[0][0][3] == 100 and want[6][1]["failed_nodes"] == 300 and want[6][1]["num_nodes"] == 300
    ranks = group(2, cfg, nodes)
    check_all(ranks, run_all(ranks, pods), want, f"deviceExchange={dx}:")
    close(ranks)


# ---- 7. the one-pod call with evaluation output -------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_one_pod_call_diagnosis_is_the_reduction_of_its_own_eval_output(world):
    """Every rank's diagnosis equals reduce_eval of the gathered evaluation output the same call returned."""
    nodes, pods = two_block_cluster(), two_block_stream()
    want = reference_stream(reference({}, nodes), pods)
    ranks = group(world, {}, nodes)

    def one_by_one(r, s):
        out = []
        for k, p in enumerate(pods):
            res, ev, d = s.schedule_one_diag(s.compile(p), assume=True, evaluate=True)
            assert d.as_dict() == reduce_eval(res.status, ev, 300), f"rank {r} pod {k}"
            out.append((res.as_tuple(), d.as_dict()))
        return out

    got = on_ranks(ranks, one_by_one)
    assert not [g for g in got if isinstance(g, Exception)], got
    check_all(ranks, got, want, f"W={world}:")
    close(ranks)


# ---- 8. diagnosed and plain sharded batches agree ---------------------------------------------------------------------
@pytest.mark.parametrize("dx", [False, True], ids=["allreduce", "devx"])
def test_diagnosed_and_plain_sharded_batches_agree(dx):
    cfg, nodes, existing, pods, want = random_reference(600)
    cfg = dict(cfg, deviceExchange=dx)
    plain = group(2, cfg, nodes, existing, namespaces(), diagnosis=None)
    diag = group(2, cfg, nodes, existing, namespaces())
    a = on_ranks(plain, lambda r, s: [x.as_tuple() for x in s.schedule_batch([s.compile(p) for p in pods], assume=True)])
    b = run_all(diag, pods)
    assert not [g for g in a if isinstance(g, Exception)], a
    for r in range(2):
        assert a[r] == [res for res, _ in b[r]] == [res for res, _ in want], f"rank {r}"
    close(plain + diag)


# ---- 9. the RCCL transport at worldSize 1 -----------------------------------------------------------------------------
def test_rccl_transport_single_rank_sums_and_matches_reference():
    """ncclAllReduce(ncclInt32, ncclSum) on the one rank a one-GPU machine can host; the loops' unsplit diagnosing
    instances run with the RCCL ranks' default device exchange."""
    from ksg.native import Scheduler, comm_unique_id
    cfg, nodes, existing, pods, want = random_reference(600)
    s = fill(Scheduler(dict(cfg, device=0, featureGates=GATE_OFF,
                            distributed={"worldSize": 1, "rank": 0, "ncclId": comm_unique_id(), "diagnosis": True})),
             nodes, existing, namespaces())
    check_all([s], run_all([s], pods), want, "RCCL W=1:")
    s.close()


# ---- 10. the opt-in ---------------------------------------------------------------------------------------------------
def test_diagnosis_key_needs_a_sharded_context():
    from ksg.native import Scheduler
    with pytest.raises(Exception, match="distributed.diagnosis"):
        Scheduler({"device": 0, "distributed": {"worldSize": 1, "rank": 0, "diagnosis": True}})


def test_ranks_that_disagree_get_einval_and_schedule_nothing():
    nodes = [box("u0"), box("u1"), box("t0", taint=True)]
    ranks = group(2, {}, nodes, diagnosis=[True, False])
    pod = ask("p", "1").obj()

    def call(r, s):
        h = s.compile(pod)
        codes = []
        for f in (lambda: s.schedule_one_diag(h), lambda: s.schedule_batch_diag([h])):
            with pytest.raises(KsgError) as e:
                f()
            codes.append(int(re.search(r"rc=(-?\d+)", str(e.value)).group(1)))
        return codes

    got = on_ranks(ranks, call)
    assert got == [[KSG_EINVAL, KSG_EINVAL]] * 2, got
    # nothing was scheduled: a plain collective batch still places the pod on a cluster nobody touched
    plain = on_ranks(ranks, lambda r, s: [x.as_tuple() for x in s.schedule_batch([s.compile(pod)], assume=True)])
    want = reference({}, nodes)
    assert plain == [[want.schedule_one(want.compile(pod), assume=True)[0].as_tuple()]] * 2, plain
    close(ranks)


@pytest.mark.parametrize("flag", [None, False])
def test_default_still_refuses(flag):
    ranks = group(2, {}, [box("u0"), box("u1"), box("t0", taint=True)], diagnosis=flag)
    s = ranks[0]  # one rank alone, from this thread: a refusal waits for no peer
    h = s.compile(ask("p", "1").obj())
    for call in (lambda: s.schedule_one_diag(h), lambda: s.schedule_batch_diag([h])):
        with pytest.raises(KsgError, match=f"rc={KSG_ENOTSUP}"):
            call()
    close(ranks)
