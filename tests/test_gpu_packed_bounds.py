"""The persistent loops' packed fields on both sides of the host-side guards that protect them.

The loops carry values in fields whose widths only the host enforces:

  weights    Engine::loop_bounds_ok: wsum * 100 < 2^19 over the pod's active score plugins, so that TotalScore
             stays under 2^19 and the packed key (TotalScore << 29 | pre-order key) under 48 bits
  preferred  Engine::loop_bounds_ok: the preferred NodeAffinity terms' |weight| sum < 2^24 - 1, because the raw
             sum plus one rides a 24-bit granule field (exchange A)
  spread     the compile stage's raw_bound < kAggPtsRawMax = 2^24 - 2, with maxSkew entering the bound directly:
             k_agg_loop carries the raw PodTopologySpread score in 24 bits of exchange PX, as a uint32_t with
             ~0u for "ignored" inside the workgroup

For each guard, one configuration sits on the last value inside and one on the first value outside; the edge
values are restated below from the code.  Each side runs as a k_sched_loop batch, as a k_agg_loop batch (the same
pods with a ScheduleAnyway hostname constraint), through the resident ring and in a W = 2 deviceExchange group,
pod by pod against the CPU oracle.  The inside must run in the loop, with values that use the field's top bit
(asserted from the oracle); the outside must not.  The spread guard is found by a ladder of maxSkew values: every
rung matches the oracle, the lowest runs in k_agg_loop with raw scores >= 2^23, the rungs from 2^24 - 2 on do
not, and once a rung leaves the loop every higher one stays out.

Preferred weights: every other pod's terms are all positive, so that a node's raw sum reaches the whole 2^24 - 2
(raw + 1 = 2^24 - 1, the field's top value); the others carry a negative term, because the guard sums absolute
values.  Its nodes are a subset of a larger positive term's, so that no raw sum is negative: the loops' exchange
encodes raw
TaintToleration / NodeAffinity maxima as unsigned (+1), and a negative NormalizeScore result is a framework
error in the reference, which no loop reproduces.

What these cases can and cannot tell apart: `<=` for `<` in the preferred-weight guard fails the four
preferred-out cases that name a kernel.  The same change in the other two guards is no change: wsum * 100 is a
multiple of 100 and never equals 2^19, and raw_bound, a sum of logarithm products plus maxSkew, does not land on
2^24 - 2.  Those guards are pinned from both sides (5242 / 5243, and the ladder's last rung inside and first rung
outside), not on equality.

Findings: none; both sides of every guard returned the oracle's tuples on every path.
"""
import functools
import random

import pytest

import norm_edge_gen as gen
from norm_edge_gen import load
from oracle_binding import oracle
from test_gpu_sharded import _group, _run_ranks

pytestmark = pytest.mark.gpu

# Engine::loop_bounds_ok: `if (wsum * 100 >= ((int64_t)1 << 19)) return false;`
WSUM_IN = ((1 << 19) - 1) // 100  # 5242: 100 * wsum = 524 200, the last multiple of 100 below 2^19
WSUM_OUT = WSUM_IN + 1            # 5243: 524 300 >= 2^19
# Engine::loop_bounds_ok: `return pref < ((int64_t)1 << 24) - 1;` over the preferred terms' |weight|
PREF_IN, PREF_OUT = (1 << 24) - 2, (1 << 24) - 1
# desc.h: kAggPtsRawMax = ((int64_t)1 << 24) - 2 (engine.cpp: raw_bound < kAggPtsRawMax)
PTS_RAW_MAX = (1 << 24) - 2
LADDER = [1 << 23, (1 << 24) - 20000, (1 << 24) - 10000, (1 << 24) - 5000, (1 << 24) - 1000, (1 << 24) - 100,
          (1 << 24) - 3, PTS_RAW_MAX, 1 << 24, (1 << 31) - 1]
GATE_OFF = {"featureGates": {"OpportunisticBatching": False}}
# the default weights of the plugins a pod with preferred NodeAffinity terms scores with (TaintToleration 3,
# NodeAffinity 2, BalancedAllocation 1, ImageLocality 1) besides NodeResourcesFit; a spread pod adds
# PodTopologySpread 2
OTHERS = {"k_sched_loop": 7, "k_agg_loop": 9}


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


@functools.lru_cache(maxsize=None)
def _cluster():
    rng = random.Random("packed-bounds")
    nodes = []
    for i in range(gen.N_NODES):
        lab = gen.topo_labels(i)
        if i % 4 == 1:
            lab["tier"] = "gold"
        nodes.append(gen.node(i, cpu_milli=rng.choice([4000, 8000, 16000]), labels=lab,
                              taints=[gen.PREFER_NO] if i % 11 == 3 else None))
    names = [gen.name_of(n) for n in nodes]
    bound = [gen.pod(f"bound-{k}", "svc", cpu=rng.choice([100, 500, 900]), mem=rng.choice([1, 2, 3]) << 29,
                     node_name=names[rng.randrange(gen.N_NODES)]) for k in range(150)]
    bound += [gen.pod(f"bound-full-{i}", "full", cpu=10, mem=gen.MIB, node_name=names[i]) for i in range(gen.N_NODES)]
    return nodes, bound


def _with_spread(p, max_skew=1):
    q = dict(p, spec=dict(p["spec"]))
    q["spec"]["topologySpreadConstraints"] = [gen.spread(gen.HOSTNAME, "full", max_skew)]
    return q


def _pods(tag, n, terms, seed):
    rng = random.Random(f"packed-{seed}")
    out = []
    for k in range(n):
        p = gen.pod(f"{tag}-{k}", "full", cpu=rng.choice([100, 250, 500]), mem=rng.choice([1, 2]) << 28)
        p["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": terms(rng)}}
        out.append(p)
    return out


def _small_terms(rng):
    return [gen._pref(rng.choice([7, 13, 29]), "zone3", "In", [f"z{rng.randrange(3)}"]), gen._pref(3, "tier", "Exists")]


def _big_terms(total):
    """|weights| summing to `total`: nodes in z0 that are gold and in d0-d9 match every positive term, nodes outside
    z0 without a tier and beyond d9 match none, the rest sit in between.  Every other pod's terms are all positive (a
    node's raw sum reaches `total`: the field's top value at 2^24 - 2), the others carry a negative term whose nodes
    are z0 nodes, so that no raw sum is below 0."""
    count = [0]

    def terms(rng):
        count[0] += 1
        out = [gen._pref(16000000, "zone3", "In", ["z0"]), gen._pref(777000, "tier", "Exists")]
        if count[0] % 2:
            return out + [gen._pref(total - 16777000, "zone29", "In", [f"d{k}" for k in range(10)])]
        neg = {"weight": -100, "preference": {"matchExpressions": [
            {"key": "zone3", "operator": "In", "values": ["z0"]}, {"key": "zone7", "operator": "In", "values": ["s1"]}]}}
        return out + [neg, gen._pref(total - 16777100, "zone29", "In", [f"d{k}" for k in range(10)])]
    return terms


# guard, side -> (config of the kernel class, pods)
def _case(guard, side, kernel):
    if guard == "weights":
        fit = (WSUM_IN if side == "in" else WSUM_OUT) - OTHERS[kernel]
        cfg, pods = {"scoreWeights": {"NodeResourcesFit": str(fit)}}, _pods("w", 48, _small_terms, 1)
    else:
        cfg, pods = {}, _pods("p", 48, _big_terms(PREF_IN if side == "in" else PREF_OUT), 2)
    if kernel == "k_agg_loop":
        pods = [_with_spread(p) for p in pods]
    return cfg, pods


@functools.lru_cache(maxsize=None)
def _reference(guard, side, kernel, sharded=False):
    cfg, pods = _case(guard, side, kernel)
    cfg = dict(cfg, **(GATE_OFF if sharded else {}))
    nodes, bound = _cluster()
    o = load(oracle(dict(cfg)), nodes, bound)
    if guard == "preferred":  # nodes that match every term, none, and in between: 100 * r / mx is not constant
        total = PREF_IN if side == "in" else PREF_OUT
        for k, top in ((0, total), (1, total - 100)):  # all positive; with the negative term
            _, raw, norm = o.run_score_plugin(o.compile(pods[k]), "NodeAffinity")
            assert max(raw) == top and min(raw) == 0 and len(set(raw)) >= 6 and len(set(norm)) >= 4, sorted(set(raw))
    want = [o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in pods]
    o.close()
    assert all(w[0] == 0 for w in want), want
    if guard == "weights" and side == "in":  # the key's top bit is in use
        assert all(w[4] >= 1 << 18 for w in want), [w[4] for w in want]
    return cfg, pods, want


def _check(tag, got, want):
    assert len(got) == len(want)
    for k in range(len(want)):
        assert got[k] == want[k], f"{tag} pod {k}: {got[k]} != oracle {want[k]}"


def _expect(side, kernel, name):
    if side == "in":
        assert name == kernel, name
    else:
        assert name == "k_filter_score", name


CASES = [(g, s, k) for g in ("weights", "preferred") for s in ("in", "out") for k in ("k_sched_loop", "k_agg_loop")]
CASE_IDS = [f"{g}-{s}-{k}" for g, s, k in CASES]


@pytest.mark.parametrize("guard,side,kernel", CASES, ids=CASE_IDS)
def test_batch(native, guard, side, kernel):
    cfg, pods, want = _reference(guard, side, kernel)
    nodes, bound = _cluster()
    g = load(native(dict(cfg)), nodes, bound)
    rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
    _expect(side, kernel, g.kernel_stats()[3])
    _check(f"{guard}/{side} {kernel}", [r.as_tuple() for r in rs], want)
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


@pytest.mark.parametrize("guard,side,kernel", CASES, ids=CASE_IDS)
def test_resident_ring(native, guard, side, kernel):
    cfg, pods, want = _reference(guard, side, kernel)
    nodes, bound = _cluster()
    g = load(native(dict(cfg)), nodes, bound)
    got = [g.schedule_one(g.compile(p), assume=True)[0].as_tuple() for p in pods]
    _check(f"{guard}/{side} {kernel} ring", got, want)
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


@pytest.mark.parametrize("guard,side,kernel", CASES, ids=CASE_IDS)
def test_device_exchange_group(guard, side, kernel):
    cfg, pods, want = _reference(guard, side, kernel, sharded=True)
    nodes, bound = _cluster()
    ranks, o = _group(2, dict(cfg, deviceExchange=True), nodes, bound)
    o.close()
    got = _run_ranks(ranks, pods, len(pods))
    for s in ranks:
        _expect(side, kernel, s.kernel_stats()[3])
    for r in range(2):
        _check(f"{guard}/{side} {kernel} rank {r}", got[r], want)
    stats = [s.loop_stats() for s in ranks]
    assert all(st == (0, 0) for st in stats), stats
    for s in ranks:
        s.close()


# ---- the PodTopologySpread raw bound: a ladder of maxSkew values ---------------------------------------------
def _rung_pods(rung, skew):
    rng = random.Random(f"ladder-{rung}")
    return [_with_spread(gen.pod(f"l{rung}-{k}", "full", cpu=rng.choice([100, 250, 500])), skew) for k in range(16)]


@functools.lru_cache(maxsize=None)
def _ladder_reference(sharded=False):
    """Per rung the oracle's tuples, one context through the whole ladder; the lowest rung's winners' raw scores
    are at least 2^23 (every node hosts a matching pod: count >= 1, weight log(202), plus maxSkew - 1)."""
    nodes, bound = _cluster()
    o = load(oracle(dict(GATE_OFF if sharded else {})), nodes, bound)
    want = [[o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in _rung_pods(r, skew)]
            for r, skew in enumerate(LADDER)]
    o.close()
    assert all(w[0] == 0 for rung in want for w in rung)
    return want


def _ladder_verdict(kernels):
    """kernels: the kernel name per rung."""
    assert kernels[0] == "k_agg_loop", kernels
    out = [k != "k_agg_loop" for k in kernels]
    for r, skew in enumerate(LADDER):
        if skew >= PTS_RAW_MAX:
            assert out[r], (skew, kernels)
        if r and out[r - 1]:
            assert out[r], f"maxSkew {skew} is back in the loop: {kernels}"
        if out[r]:
            assert kernels[r] == "k_filter_score", kernels


def test_spread_ladder_batch(native):
    want = _ladder_reference()
    nodes, bound = _cluster()
    g = load(native({}), nodes, bound)
    kernels = []
    for r, skew in enumerate(LADDER):
        rs = g.schedule_batch([g.compile(p) for p in _rung_pods(r, skew)], assume=True)
        kernels.append(g.kernel_stats()[3])
        _check(f"maxSkew {skew}", [x.as_tuple() for x in rs], want[r])
    print("ladder:", list(zip(LADDER, kernels)))
    _ladder_verdict(kernels)
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


def test_spread_ladder_resident_ring(native):
    want = _ladder_reference()
    nodes, bound = _cluster()
    g = load(native({}), nodes, bound)
    for r, skew in enumerate(LADDER):
        got = [g.schedule_one(g.compile(p), assume=True)[0].as_tuple() for p in _rung_pods(r, skew)]
        _check(f"maxSkew {skew} ring", got, want[r])
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


def test_spread_ladder_device_exchange_group():
    want = _ladder_reference(sharded=True)
    nodes, bound = _cluster()
    ranks, o = _group(2, {"deviceExchange": True}, nodes, bound)
    o.close()
    kernels = []
    for r, skew in enumerate(LADDER):
        got = _run_ranks(ranks, _rung_pods(r, skew), 16)
        names = {s.kernel_stats()[3] for s in ranks}
        assert len(names) == 1, names
        kernels.append(names.pop())
        for k in range(2):
            _check(f"maxSkew {skew} rank {k}", got[k], want[r])
    _ladder_verdict(kernels)
    stats = [s.loop_stats() for s in ranks]
    assert all(st == (0, 0) for st in stats), stats
    for s in ranks:
        s.close()


def test_two_constraints_past_2_32_on_the_launch_path(native):
    """Two constraints of maxSkew 2^31 - 1 on keys where every node counts a matching pod: the raw score,
    2 * (2^31 - 2) + counts * weights, passes 2^32.  Per-node evaluation output against the oracle's."""
    nodes, bound = _cluster()
    g, o = load(native({}), nodes, bound), load(oracle({}), nodes, bound)
    big = (1 << 31) - 1
    for k in range(6):
        p = gen.pod(f"two-{k}", "full", cpu=100 + 50 * k)
        p["spec"]["topologySpreadConstraints"] = [gen.spread(gen.HOSTNAME, "full", big), gen.spread("zone3", "full", big - k)]
        rg, eg = g.schedule_one(g.compile(p), assume=True, evaluate=True)
        ro, eo = o.schedule_one(o.compile(p), assume=True, evaluate=True)
        assert rg.as_tuple() == ro.as_tuple(), f"pod {k}: {rg.as_tuple()} != oracle {ro.as_tuple()}"
        assert ro.status == 0
        for key in eo:
            assert eg[key] == eo[key], f"pod {k}: eval[{key}] differs"
    assert g.loop_stats() == (0, 0)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()
    o.close()
