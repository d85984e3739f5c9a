"""NormalizeScore and the weighted sum on the device -- node_total (the launch path), loop_total (k_sched_loop,
the resident ring), agg_total and the inline PodTopologySpread normalisation (k_agg_loop), k_select_shard's
NormStats rebuilt from the exchange words (node-sharded groups) -- with the PodTopologySpread raw score,
RequestedToCapacityRatio and ImageLocality, at the inputs where their arithmetic can go wrong:
norm_edge_gen's ipa, pts, defaultnorm, image and rtcr streams under every profile of theirs.

Every path is compared pod by pod with the CPU oracle, whose result tuples are computed once per stream.
Inside a loop only the result tuple is visible; tests/test_norm_edge_inputs.py holds the conditions under which
these streams turn a wrong score into a wrong tuple, and checks the oracle itself against a plain restatement.
Every case asserts that no loop gave up (a recovered give-up must not pass for a clean run), every unsharded
case ends with the device mirror compared against the host cache.

Findings: none; every path returned the oracle's tuples on every stream.
"""
import functools

import pytest

import norm_edge_gen as gen
from norm_edge_gen import load
from oracle_binding import oracle
from test_gpu_sharded import _group, _run_ranks

pytestmark = pytest.mark.gpu

IDS = [f"{f}-{p}" for f, p in gen.STREAMS]
LOOP = {"ipa": "k_agg_loop", "pts": "k_agg_loop", "defaultnorm": "k_sched_loop", "image": "k_sched_loop",
        "rtcr": "k_sched_loop"}
GATE_OFF = {"featureGates": {"OpportunisticBatching": False}}  # what a node-sharded group runs under (_group)


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


@functools.lru_cache(maxsize=None)
def _reference(family, profile, sharded=False):
    """(config, nodes, bound pods, steps, the oracle's result tuples of the steps' pods)."""
    nodes, bound, steps = gen.stream(family)
    cfg = dict(gen.PROFILES[family][profile], **(GATE_OFF if sharded else {}))
    o = load(oracle(dict(cfg)), nodes, bound)
    want = []
    for step in steps:
        if step[0] == "pod":
            want.append(o.schedule_one(o.compile(step[1]), assume=True)[0].as_tuple())
        else:
            gen.apply_step(o, step)
    o.close()
    return cfg, nodes, bound, steps, want


def _check(tag, got, want):
    assert len(got) == len(want)
    for k in range(len(want)):
        assert got[k] == want[k], f"{tag} pod {k}: {got[k]} != oracle {want[k]}"


def _batch(native, family, profile, extra, kernel):
    cfg, nodes, bound, steps, want = _reference(family, profile)
    g = load(native(dict(cfg, **extra)), nodes, bound)
    got = []
    for pre, pods in gen.runs(steps):
        for step in pre:
            gen.apply_step(g, step)
        got += [r.as_tuple() for r in g.schedule_batch([g.compile(p) for p in pods], assume=True)]
        if kernel:
            assert g.kernel_stats()[3] == kernel
    _check(f"{family}/{profile} {extra}", got, want)
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_launch_path_with_evaluation(native, family, profile):
    """The per-pod launch path (node_total in k_select): per-node codes, reasons, per-plugin vectors, normalised
    scores and totals too."""
    cfg, nodes, bound, steps, want = _reference(family, profile)
    g, o = load(native(dict(cfg)), nodes, bound), load(oracle(dict(cfg)), nodes, bound)
    assert g.node_names() == o.node_names()
    k = 0
    for step in steps:
        if step[0] != "pod":
            for b in (g, o):
                gen.apply_step(b, step)
            assert g.node_names() == o.node_names()
            continue
        rg, eg = g.schedule_one(g.compile(step[1]), assume=True, evaluate=True)
        ro, eo = o.schedule_one(o.compile(step[1]), assume=True, evaluate=True)
        assert rg.as_tuple() == ro.as_tuple() == want[k], f"pod {k}: {rg.as_tuple()} != oracle {ro.as_tuple()}"
        for key in eo:
            assert eg[key] == eo[key], f"pod {k}: eval[{key}] differs"
        k += 1
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()
    o.close()


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_batch_defaults(native, family, profile):
    _batch(native, family, profile, {}, LOOP[family])


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_batch_one_workgroup(native, family, profile):
    _batch(native, family, profile, {"loopWorkgroups": 1}, LOOP[family])


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_batch_without_persistent_loop(native, family, profile):
    _batch(native, family, profile, {"persistentLoop": False}, None)


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_resident_ring_single_calls(native, family, profile):
    """ksg_schedule_one without evaluation output: the resident ring."""
    cfg, nodes, bound, steps, want = _reference(family, profile)
    g = load(native(dict(cfg)), nodes, bound)
    got = []
    for step in steps:
        if step[0] == "pod":
            got.append(g.schedule_one(g.compile(step[1]), assume=True)[0].as_tuple())
        else:
            gen.apply_step(g, step)
    _check(f"{family}/{profile} ring", got, want)
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


@pytest.mark.parametrize("exchange", [False, True], ids=["allreduce", "deviceExchange"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_node_sharded_group(family, profile, world, exchange):
    """An in-process node-sharded group: k_select_shard's NormStats from the exchange words (the
    InterPodAffinity minimum travels complemented), or, with deviceExchange, the loops across ranks."""
    cfg, nodes, bound, steps, want = _reference(family, profile, sharded=True)
    ranks, o = _group(world, dict(cfg, **({"deviceExchange": True} if exchange else {})), nodes, bound)
    o.close()
    got = [[] for _ in ranks]
    for pre, pods in gen.runs(steps):
        for step in pre:
            for s in ranks:
                gen.apply_step(s, step)
        out = _run_ranks(ranks, pods, 64)
        if exchange:
            assert {s.kernel_stats()[3] for s in ranks} == {LOOP[family]}
        for r in range(world):
            got[r] += out[r]
    for r in range(world):
        _check(f"{family}/{profile} W={world} rank {r}", got[r], want)
    stats = [s.loop_stats() for s in ranks]
    assert all(st == (0, 0) for st in stats), f"persistent-loop give-ups / re-runs per rank: {stats}"
    for s in ranks:
        s.close()
