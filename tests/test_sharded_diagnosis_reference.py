"""The rule the node-sharded FitError diagnosis relies on, without a device: every bin of the diagnosis
is additive over a partition of the nodes.  The oracle's evaluation output of each failing cycle is split at the ranks'
block ranges -- rank r of W owns the 256-node blocks [NB*r//W, NB*(r+1)//W) -- each slice is reduced with the bins of
diagnosis_reference.reduce_eval, and the slices' sum must be the reduction of the whole."""
import functools

import pytest

from diagnosis_reference import FIT_ERROR, NUM_REASONS, fill, reduce_eval
from fuzz_gen import namespaces
from ksg.abi import NUM_PLUGINS
from oracle_binding import oracle
from test_gpu_diagnosis import random_case

BLOCK = 256
ARRAYS = ("node_code", "node_plugin", "node_reasons")


def shard_nodes(n, world, rank):
    """[lo, hi): the snapshot indices of rank `rank` of `world` (Engine::shard_range)."""
    nb = (n + BLOCK - 1) // BLOCK
    return min(n, nb * rank // world * BLOCK), min(n, nb * (rank + 1) // world * BLOCK)


def reduce_slice(status, ev, lo, hi):
    part = dict(ev, **{k: ev[k][lo:hi] for k in ARRAYS})
    return reduce_eval(status, part, hi - lo)


def add_up(parts, whole):
    """The host's side of the sum: the counters added, the plugin mask and the cycle-wide fields derived."""
    d = dict(whole, failed_nodes=0, unresolvable_nodes=0, unschedulable_plugins=0,
             plugin_nodes=[0] * NUM_PLUGINS, reason_nodes=[0] * NUM_REASONS)
    for p in parts:
        d["failed_nodes"] += p["failed_nodes"]
        d["unresolvable_nodes"] += p["unresolvable_nodes"]
        d["plugin_nodes"] = [a + b for a, b in zip(d["plugin_nodes"], p["plugin_nodes"])]
        d["reason_nodes"] = [a + b for a, b in zip(d["reason_nodes"], p["reason_nodes"])]
    for q, c in enumerate(d["plugin_nodes"]):
        d["unschedulable_plugins"] |= (c > 0) << q
    return d


@functools.lru_cache(maxsize=None)
def cycles(n_nodes):
    """[(status, evaluation output)] of the random case's stream on the oracle, OpportunisticBatching off as on a
    node-sharded context."""
    cfg, nodes, existing, pods = random_case(n_nodes)
    o = fill(oracle(dict(cfg, featureGates={"OpportunisticBatching": False})), nodes, existing, namespaces())
    out = []
    for p in pods:
        r, ev = o.schedule_one(o.compile(p), assume=True, evaluate=True)
        out.append((r.status, ev))
    return out


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("n_nodes", [9, 130, 257, 600])
def test_slices_of_the_block_ranges_add_up_to_the_whole(n_nodes, world):
    spans = [shard_nodes(n_nodes, world, r) for r in range(world)]
    assert spans[0][0] == 0 and spans[-1][1] == n_nodes
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))  # a partition, empty shards included
    failing = 0
    for k, (status, ev) in enumerate(cycles(n_nodes)):
        whole = reduce_eval(status, ev, n_nodes)
        parts = [reduce_slice(status, ev, lo, hi) for lo, hi in spans]
        assert add_up(parts, whole) == whole, f"pod {k}"
        if status in FIT_ERROR and whole["failed_nodes"]:
            failing += 1
            # the reason bins count statuses, not nodes: they may exceed failed_nodes, and still add up
            assert sum(whole["reason_nodes"]) >= whole["failed_nodes"]
    assert failing >= 5
