"""The straight-line default-plugin evaluation (eval_core_fast: DF_FAST in k_sched_loop and the resident ring,
DF_LFAST in k_agg_loop) at the quantities where its own arithmetic can go wrong -- edge_gen's degenerate,
boundary and magnitude streams -- and the generic evaluation the host switches to once an allocatable
reaches (1 << 52) / 100 (the over stream), under LeastAllocated, MostAllocated and Fit / BalancedAllocation
weights that differ.

Every path is compared pod by pod with the CPU oracle, whose results are computed once per stream.  Inside a
loop only the result tuple is visible; tests/test_edge_inputs.py holds the conditions under which these
streams turn a wrong score into a wrong tuple.  Every case ends with the device mirror compared against the
host cache: the assumes' int64 sums at 2^45-scale values.
"""
import functools

import pytest

import edge_gen
from edge_gen import load
from oracle_binding import oracle

pytestmark = pytest.mark.gpu

STREAMS = [(f, p) for f in edge_gen.FAMILIES for p in edge_gen.CONFIGS]
IDS = [f"{f}-{p}" for f, p in STREAMS]


@pytest.fixture(scope="module")
def native():
    from ksg.native import Scheduler
    return Scheduler


@functools.lru_cache(maxsize=None)
def _reference(family, profile, spread=False):
    """(config, nodes, bound pods, incoming pods, the oracle's result tuples); spread: the pods with one
    ScheduleAnyway hostname constraint each (k_agg_loop's class)."""
    nodes, bound, incoming = edge_gen.stream(family)
    if spread:
        incoming = [edge_gen.with_hostname_spread(p) for p in incoming]
    cfg = edge_gen.CONFIGS[profile]
    o = load(oracle(dict(cfg)), nodes, bound)
    want = [o.schedule_one(o.compile(p), assume=True)[0].as_tuple() for p in incoming]
    o.close()
    return cfg, nodes, bound, incoming, want


def _check(tag, got, want):
    assert len(got) == len(want)
    for k in range(len(want)):
        assert got[k] == want[k], f"{tag} pod {k}: {got[k]} != oracle {want[k]}"


def _batch(native, family, profile, extra, kernel="k_sched_loop", spread=False):
    cfg, nodes, bound, incoming, want = _reference(family, profile, spread)
    g = load(native(dict(cfg, **extra)), nodes, bound)
    rs = g.schedule_batch([g.compile(p) for p in incoming], assume=True)
    if kernel:
        assert g.kernel_stats()[3] == kernel
    _check(f"{family}/{profile} {extra}", [r.as_tuple() for r in rs], want)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


@pytest.mark.parametrize("family,profile", STREAMS, ids=IDS)
def test_launch_path_with_evaluation(native, family, profile):
    """The per-pod launch path (k_filter_score's generic eval_node): per-node codes, reasons, per-plugin
    vectors and totals too."""
    cfg, nodes, bound, incoming, want = _reference(family, profile)
    g, o = load(native(dict(cfg)), nodes, bound), load(oracle(dict(cfg)), nodes, bound)
    assert g.node_names() == o.node_names()
    for k, p in enumerate(incoming):
        rg, eg = g.schedule_one(g.compile(p), assume=True, evaluate=True)
        ro, eo = o.schedule_one(o.compile(p), assume=True, evaluate=True)
        assert rg.as_tuple() == ro.as_tuple() == want[k], f"pod {k}: {rg.as_tuple()} != oracle {ro.as_tuple()}"
        for key in eo:
            assert eg[key] == eo[key], f"pod {k}: eval[{key}] differs"
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()
    o.close()


@pytest.mark.parametrize("family,profile", STREAMS, ids=IDS)
def test_batch_defaults(native, family, profile):
    """schedule_batch at the defaults: k_sched_loop's split instance over 128-node units."""
    _batch(native, family, profile, {})


@pytest.mark.parametrize("extra", [{"loopSplitEval": False}, {"loopUnit": 256}, {"loopWorkgroups": 1}],
                         ids=["unsplit", "unit256", "wg1"])
@pytest.mark.parametrize("family,profile", STREAMS, ids=IDS)
def test_batch_loop_variants(native, family, profile, extra):
    _batch(native, family, profile, extra)


@pytest.mark.parametrize("family,profile", STREAMS, ids=IDS)
def test_batch_without_persistent_loop(native, family, profile):
    _batch(native, family, profile, {"persistentLoop": False}, kernel=None)


@pytest.mark.parametrize("family,profile", STREAMS, ids=IDS)
def test_resident_ring_single_calls(native, family, profile):
    """ksg_schedule_one without evaluation output: the resident ring."""
    cfg, nodes, bound, incoming, want = _reference(family, profile)
    g = load(native(dict(cfg)), nodes, bound)
    got = [g.schedule_one(g.compile(p), assume=True)[0].as_tuple() for p in incoming]
    _check(f"{family}/{profile} ring", got, want)
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()


@pytest.mark.parametrize("family,profile", STREAMS, ids=IDS)
def test_agg_loop_local_fast(native, family, profile):
    """The same pods with a ScheduleAnyway hostname spread constraint: k_agg_loop, whose node-local plugins
    take eval_core_fast (DF_LFAST)."""
    _batch(native, family, profile, {}, kernel="k_agg_loop", spread=True)


def test_crossing_the_bound_mid_stream(native):
    """A magnitude cluster below the bound (straight-line evaluation), then add_node with memory at the bound
    (every later pod takes the generic one), then update_node raising another node's memory in place: batches
    and single calls, pod by pod against the oracle."""
    nodes, bound, incoming = edge_gen.stream("magnitude")
    g, o = load(native({}), nodes, bound), load(oracle({}), nodes, bound)

    def batch(pods, tag):
        rs = g.schedule_batch([g.compile(p) for p in pods], assume=True)
        assert g.kernel_stats()[3] == "k_sched_loop"
        for k, p in enumerate(pods):
            ro, _ = o.schedule_one(o.compile(p), assume=True)
            assert rs[k].as_tuple() == ro.as_tuple(), f"{tag} pod {k}: {rs[k].as_tuple()} != oracle {ro.as_tuple()}"

    batch(incoming[:40], "below the bound")
    late = edge_gen.node(900, 64000, edge_gen.BOUND, 110)
    for b in (g, o):
        b.add_node(late)
    assert g.node_names() == o.node_names()
    batch(incoming[40:70], "after add_node at the bound")
    for k, p in enumerate(incoming[70:90]):
        rg, _ = g.schedule_one(g.compile(p), assume=True)
        ro, _ = o.schedule_one(o.compile(p), assume=True)
        assert rg.as_tuple() == ro.as_tuple(), f"single call {k}: {rg.as_tuple()} != oracle {ro.as_tuple()}"
    raised = edge_gen.node(17, 64000, (1 << 55) + 3, 110)
    for b in (g, o):
        b.update_node(raised)
    assert g.node_names() == o.node_names()
    batch(incoming[90:], "after update_node past the bound")
    assert g.compare_mirror(sync=False) == (0, -1)
    g.close()
    o.close()
