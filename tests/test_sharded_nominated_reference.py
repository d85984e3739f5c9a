"""What tests/test_gpu_sharded_nominated.py's streams decide in each rank's node range, on the references alone (no
device): a rank whose share of the work is lost -- its owner pass never published, its blocks filtered without the
nominee table -- then changes some pod's answer, so the GPU tests cannot pass by one rank's work alone.

Ranges follow shard_range's rule: rank r of W holds the 256-node blocks floor(NB * r / W) .. floor(NB * (r + 1) / W)."""
import pytest

from sharded_nominated_cases import (EVAL_NODES, OWN_MODES, evaluate_flips, evaluate_reference, own_fates,
                                     own_reference, per_rank, shard_ranges)


def test_shard_ranges_follow_the_block_rule():
    assert shard_ranges(700, 2) == [(0, 256), (256, 700)]
    assert shard_ranges(700, 3) == [(0, 256), (256, 512), (512, 700)]
    assert shard_ranges(600, 3) == [(0, 256), (256, 512), (512, 600)]
    assert shard_ranges(257, 2) == [(0, 256), (256, 257)]
    assert shard_ranges(257, 3) == [(0, 0), (0, 256), (256, 257)]
    assert shard_ranges(130, 2) == [(0, 0), (0, 130)] and shard_ranges(9, 3) == [(0, 0), (0, 0), (0, 9)]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("pct,mode", OWN_MODES)
def test_every_rank_owns_a_placed_and_a_failed_nominated_node(pct, mode, world):
    """In every rank's range at least one pod is placed on its own nominated node and at least one fails there alone
    and goes on to the full pass; the directed pods sit at snapshot indices 255, 256 and in the last block."""
    _, nodes, _, pods, want = own_reference(pct, mode)
    fates = own_fates(pct, mode)
    placed = per_rank([nn for nn, f in fates.values() if f == "placed"], len(nodes), world)
    failed = per_rank([nn for nn, f in fates.values() if f == "failed"], len(nodes), world)
    print(f"pct {pct}, {mode}, W={world}: placed on own node per rank {placed}, failed alone per rank {failed}")
    assert all(n > 0 for _, n in [(a, b - a) for a, b in shard_ranges(len(nodes), world)])
    assert all(c > 0 for c in placed), placed
    assert all(c > 0 for c in failed), failed
    assert fates[0][1] == "placed" and fates[0][0] >= 512  # the directed pod of the last block
    assert [fates[k][0] for k in (1, 2)] == [255, 256]
    # a pod that failed alone was evaluated on more than its nominated node
    assert all(want[k][0][2] > 1 or want[k][0][0] != 0 for k, (_, f) in fates.items() if f == "failed")


# the nominees alone close these many node statuses per rank (an empty range: none)
FLIPS = {(600, 2): [32, 11], (600, 3): [32, 9, 2], (257, 2): [12, 3], (257, 3): [0, 12, 3], (130, 2): [0, 38],
         (9, 2): [0, 27]}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_nodes", EVAL_NODES)
def test_nominees_alone_close_a_node_in_every_non_empty_range(n_nodes, world):
    flips = per_rank(evaluate_flips(n_nodes), n_nodes, world)
    print(f"{n_nodes} nodes, W={world}: statuses only the nominees make a failure, per rank {flips}")
    for (a, b), c in zip(shard_ranges(n_nodes, world), flips):
        assert (c > 0) == (b > a), (n_nodes, world, flips)
    if (n_nodes, world) in FLIPS:
        assert flips == FLIPS[(n_nodes, world)]
    _, _, _, noms, pods, want = evaluate_reference(n_nodes)
    own = [k for k, p in enumerate(pods) if (p.get("status") or {}).get("nominatedNodeName")]
    assert len(own) == 2  # the stream holds two nominees' own cycles
