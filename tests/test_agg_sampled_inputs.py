"""The inputs of tests/test_gpu_agg_sampled.py (sampled pods inside k_agg_loop), checked on the oracle alone: no device.

tests/agg_sampled_gen.py builds a cluster whose cut feasible list differs from its full feasible list in every
quantity the loop's kept-list exchange carries.  These tests state the conditions the streams must meet for the GPU
comparison to exercise the cut, and check them on the oracle's per-pod evaluation output.  They are conditions on the
inputs, not measurements."""
import pytest

import agg_sampled_gen as gen
from oracle_binding import oracle

SHAPES_OVER_100 = ["130", "257", "600"]
PCTS = [0, 7, 30, 55]


def _rare(shape):
    nodes, bound = gen.shape_cluster(shape)
    o = gen.fill(oracle({}), nodes, bound)
    names = o.node_names()
    o.close()
    return gen.rare_indices(names, nodes), names


@pytest.mark.parametrize("shape", sorted(gen.SHAPES))
def test_rare_zone_sits_at_the_front_of_the_snapshot_list(shape):
    n, zones, rare, _ = gen.SHAPES[shape]
    idx, names = _rare(shape)
    assert len(names) == n and len(idx) == rare and 3 <= rare <= 4
    assert max(idx) < rare * (zones + 1), idx  # the zone round-robin: one rare node per round, from the first on


def _classes(shape, want):
    idx = set(_rare(shape)[0])
    placed = [c for c in want if c.placed]
    cut = [c for c in placed if c.cut]
    return {
        "placed": placed,
        "cut": cut,
        "cut, no kept node in the rare zone": [c for c in cut if not idx & set(c.kept)],
        "cut, a kept node in the rare zone": [c for c in cut if idx & set(c.kept)],
        "wraps": [c for c in placed if c.wraps],
        "end node in another workgroup's range than the chosen node": [c for c in cut if c.end // gen.WG != c.node // gen.WG],
        "no cut": [c for c in placed if not c.cut],
        "F = 0": [c for c in want if c.status != 0],
    }


@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
@pytest.mark.parametrize("kind", gen.STREAMS)
@pytest.mark.parametrize("shape", SHAPES_OVER_100)
def test_stream_meets_the_input_conditions(shape, kind, soft, pct):
    """Per stream and shape with N > 100: at least 5 placed pods with the cut active (EvaluatedNodes < N), 5 with the
    cut active and no kept node in the rare zone, 5 whose processed range wraps past the end of the list, and -- with
    more than one workgroup's worth of nodes -- 5 whose (K+1)-th node lies in another 512-node range than the chosen
    node.  Also pods that fit nowhere and placed pods without a cut between them."""
    cfg, nodes, bound, pods, want = gen.reference(shape, kind, soft, pct)
    n = len(nodes)
    cl = _classes(shape, want)
    need = ["cut", "cut, no kept node in the rare zone", "cut, a kept node in the rare zone", "wraps", "no cut", "F = 0"]
    if n > gen.WG:
        need.append("end node in another workgroup's range than the chosen node")
    for k in need:
        assert len(cl[k]) >= 5, f"{k}: {len(cl[k])}"
    # the cut pods' lists have numFeasibleNodesToFind nodes, one length per context
    assert len({c.feasible for c in cl["cut"]}) == 1 and 100 <= cl["cut"][0].feasible < n
    # pods without a cut stand between cut pods, and so do the unplaceable ones
    order = ["cut" if c.cut else "none" if c.placed else "f0" for c in want]
    assert any(order[k - 1] == "cut" and order[k] != "cut" and "cut" in order[k + 1:k + 3] for k in range(1, len(order) - 2))
    assert any(order[k - 1] == "cut" and order[k] == "f0" for k in range(1, len(order)))


def _through(cfg, nodes, bound, pods):
    o = gen.fill(oracle(gen.oracle_cfg(cfg)), nodes, bound)
    for p in pods:
        o.schedule_one(o.compile(p), assume=True)
    return o


@pytest.mark.parametrize("kind", gen.STREAMS)
def test_kept_list_differs_from_the_full_list_in_every_reduced_quantity(kind):
    """On one cut pod whose kept list holds no rare node: the maxima of raw TaintToleration, NodeAffinity and
    InterPodAffinity and the InterPodAffinity minimum over the kept nodes differ from those over all feasible nodes,
    and the full list has one zone more.  (The full list: the same cycle at percentageOfNodesToScore 100; raw scores
    from the oracle's per-plugin passes on the state the pod's cycle sees.)"""
    shape, soft, pct = "257", True, 7
    cfg, nodes, bound, pods, want = gen.reference(shape, kind, soft, pct)
    idx = set(_rare(shape)[0])
    k = next(k for k, c in enumerate(want) if c.cut and not idx & set(c.kept))
    kept = want[k].kept
    o = _through(dict(cfg, percentageOfNodesToScore=100), nodes, bound, pods[:k])
    h = o.compile(pods[k])
    r, ev = o.schedule_one(h, assume=False, evaluate=True)
    full = [i for i in range(len(nodes)) if ev["node_code"][i] == 0 and ev["total_scores"][i] != 0]
    assert len(full) == r.feasible_nodes > len(kept) and idx & set(full) and set(kept) <= set(full)
    for plugin in ("TaintToleration", "NodeAffinity", "InterPodAffinity"):
        _, raw, _ = o.run_score_plugin(h, plugin)
        assert max(raw[i] for i in full) > max(raw[i] for i in kept), plugin
        if plugin == "InterPodAffinity":
            assert min(raw[i] for i in full) < min(raw[i] for i in kept), plugin
    by_name = {n["metadata"]["name"]: n for n in nodes}
    zones = lambda ids: {by_name[o.node_names()[i]]["metadata"]["labels"][gen.ZONE] for i in ids}
    assert zones(full) == zones(kept) | {"rare"} and "rare" not in zones(kept)
    o.close()


def test_big_shape_meets_the_conditions():
    """The case for the instances that sweep more than one round of workgroups: 16 pods at 64 * 256 + 6 nodes."""
    for soft in (False, True):
        cfg, nodes, bound, pods, want = gen.reference("big", "three", soft, 45, n_pods=16)
        cl = _classes("big", want)
        for k in ("cut", "cut, no kept node in the rare zone", "wraps",
                  "end node in another workgroup's range than the chosen node"):
            assert len(cl[k]) >= 5, f"{k}: {len(cl[k])}"
        assert len(cl["F = 0"]) >= 1 and len(cl["no cut"]) >= 1


def test_nine_nodes_never_cut():
    """N < 100: every node is to be found; the rotation still advances by N per pod."""
    cfg, nodes, bound, pods, want = gen.reference("9", "five", True, 7)
    assert not any(c.cut for c in want) and sum(c.placed for c in want) >= 20
