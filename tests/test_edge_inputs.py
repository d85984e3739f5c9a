"""The edge-quantity streams (edge_gen.py) on the CPU: the oracle against a plain restatement, and the
conditions under which a wrong score on the device would show.

1. The oracle's NodeResourcesFit (LeastAllocated, MostAllocated) and NodeResourcesBalancedAllocation scores on
   every feasible node of every family, pod after pod with the assumes in between, against edge_gen.Restated
   (Python integers; Python floats for BalancedAllocation).

2. Inside a persistent loop only the result tuple is visible, so a wrong score shows only where it moves the
   winner or the winner's TotalScore.  Per stream (family x profile), from the oracle alone:
     - at least 90 % of the pods are placed,
     - the winners cover at least 20 distinct nodes,
     - for at least one third of the placed pods another feasible node's TotalScore is within 1 of the winner's,
     - some node wins in both 128-node units and in both 64-lane halves.
   And on the boundary family's BalancedAllocation inputs (every feasible node of every pod, with the pod),
   int((1 - std) * 100) of two mutants differs from the restatement's: a * (1 / b) in place of a / b on at
   least 1 % of them, a binary32 chain on at least 15 %.

Measured for the committed generators (seed 0): MEASURED below holds placed / distinct winners / close
runner-ups of the 130 pods of every stream (worst: over under MostAllocated, 130 / 44 / 47), and
MEASURED_MUTANTS the boundary family's counts (23 573 inputs: a * (1 / b) differs on 383, 1.62 %; binary32 on
4 069, 17.26 %).  test_measured_values_are_current keeps them in step with edge_gen.

What test_oracle_matches_restatement[over-most] found: the over variant's node 190 has 2^55 + 3 bytes of
memory.  The oracle's parse_quantity_milli and the product's parse_quantity held every quantity in int64
milli-units and saturated at 2^63 - 1 of them, so that node was decoded with 9 223 372 036 854 776 bytes
(2^53.03), where NodeInfo.SetNode takes Quantity.Value(), exact up to 2^63 - 1 (framework/types.go NewResource /
Resource.Add).  First difference: pod 2 on node 190, requested (6400m, 18 014 398 509 480) plus the pod's
(100m, 549 755 813 888): BalancedAllocation 75 where the restatement (and Go) give 74.  Both decoders now carry
milli-units in 128 bits and saturate at the int64 range of Value() / MilliValue().
"""
import functools

import pytest

import edge_gen
from edge_gen import load
from ksg.abi import PLUGIN_ID
from oracle_binding import oracle

P_FIT, P_BAL = PLUGIN_ID["NodeResourcesFit"], PLUGIN_ID["NodeResourcesBalancedAllocation"]

# family, profile -> (placed, distinct winners, placed pods with a runner-up within 1)
MEASURED = {
    ("degenerate", "least"): (130, 63, 120),
    ("degenerate", "most"): (130, 42, 64),
    ("degenerate", "weights"): (130, 63, 95),
    ("boundary", "least"): (130, 75, 115),
    ("boundary", "most"): (130, 58, 53),
    ("boundary", "weights"): (130, 71, 70),
    ("magnitude", "least"): (130, 80, 111),
    ("magnitude", "most"): (130, 56, 56),
    ("magnitude", "weights"): (130, 80, 72),
    ("over", "least"): (130, 68, 109),
    ("over", "most"): (130, 44, 47),
    ("over", "weights"): (130, 67, 79),
}
# the boundary family's BalancedAllocation inputs: (inputs, a * (1 / b) differs: 1.62 %, binary32 differs: 17.26 %)
MEASURED_MUTANTS = (23573, 383, 4069)


@functools.lru_cache(maxsize=None)
def run(family, profile):
    """One oracle pass over a stream: per pod (result tuple, eval dict) with the evaluation output kept."""
    nodes, bound, incoming = edge_gen.stream(family)
    o = load(oracle(dict(edge_gen.CONFIGS[profile])), nodes, bound)
    assert o.node_names() == [n["metadata"]["name"] for n in nodes]
    out = []
    for p in incoming:
        r, ev = o.schedule_one(o.compile(p), assume=True, evaluate=True)
        out.append((r.as_tuple(), ev))
    o.close()
    return nodes, bound, incoming, out


@pytest.mark.parametrize("profile", ["least", "most"])
@pytest.mark.parametrize("family", edge_gen.FAMILIES)
def test_oracle_matches_restatement(family, profile):
    nodes, bound, incoming, out = run(family, profile)
    st = edge_gen.Restated(nodes, bound)
    checked = 0
    for k, (p, (res, ev)) in enumerate(zip(incoming, out)):
        rest = set()
        for i in range(len(nodes)):
            if ev["node_code"][i] != 0:
                continue
            want_fit, want_bal = st.fit(i, p, profile == "most"), st.balanced(i, p)
            got_fit, got_bal = ev["plugin_scores"][P_FIT][i], ev["plugin_scores"][P_BAL][i]
            assert (got_fit, got_bal) == (want_fit, want_bal), (
                f"{family}/{profile} pod {k} node {i}: oracle Fit {got_fit} Balanced {got_bal}, restated {want_fit} "
                f"{want_bal}; allocatable {st.alloc[i]} requested {st.req[i]} non-zero {st.nz[i]} pod {p['spec']}")
            rest.add(ev["total_scores"][i] - want_fit - want_bal)
            checked += 1
        assert len(rest) <= 1, rest  # the other plugins score every node of these clusters alike
        if res[0] == 0:
            st.add(res[1], p)
    assert checked > 5000, checked


def facts(family, profile):
    nodes, _, incoming, out = run(family, profile)
    placed = close = 0
    winners = set()
    for res, ev in out:
        if res[0] != 0:
            continue
        placed += 1
        winners.add(res[1])
        assert ev["total_scores"][res[1]] == res[4]
        close += any(ev["node_code"][i] == 0 and i != res[1] and abs(ev["total_scores"][i] - res[4]) <= 1
                     for i in range(len(nodes)))
    return placed, winners, close


@pytest.mark.parametrize("profile", list(edge_gen.CONFIGS))
@pytest.mark.parametrize("family", edge_gen.FAMILIES)
def test_streams_can_show_a_wrong_score(family, profile):
    placed, winners, close = facts(family, profile)
    print(f"{family}/{profile}: placed {placed} of {edge_gen.N_PODS}, {len(winners)} distinct winners, {close} close")
    assert placed * 10 >= edge_gen.N_PODS * 9, placed
    assert len(winners) >= 20, sorted(winners)
    assert close * 3 >= placed, (close, placed)
    assert {i // 128 for i in winners} == {0, 1}, sorted(winners)
    assert {i % 128 // 64 for i in winners} == {0, 1}, sorted(winners)


def mutant_counts():
    nodes, bound, incoming, out = run("boundary", "least")
    st = edge_gen.Restated(nodes, bound)
    n = rcp = f32 = 0
    for p, (res, ev) in zip(incoming, out):
        for i in range(len(nodes)):
            if ev["node_code"][i] != 0:
                continue
            _, with_, alloc = st.balanced_inputs(i, p)
            want = edge_gen.bal_f64(with_, alloc)
            n += 1
            rcp += edge_gen.bal_mul_rcp(with_, alloc) != want
            f32 += edge_gen.bal_f32(with_, alloc) != want
        if res[0] == 0:
            st.add(res[1], p)
    return n, rcp, f32


def test_boundary_pairs_separate_the_balanced_mutants():
    n, rcp, f32 = mutant_counts()
    print(f"boundary: {n} inputs, a*(1/b) differs on {rcp} ({100 * rcp / n:.2f} %), binary32 on {f32} ({100 * f32 / n:.2f} %)")
    assert n > 10000
    assert rcp * 100 >= n, (rcp, n)
    assert f32 * 100 >= 15 * n, (f32, n)


def test_measured_values_are_current():
    """MEASURED is what the committed generators give: a change of edge_gen shows here."""
    got = {(f, p): (lambda a, w, c: (a, len(w), c))(*facts(f, p)) for f in edge_gen.FAMILIES for p in edge_gen.CONFIGS}
    assert got == MEASURED, got
    assert mutant_counts() == MEASURED_MUTANTS, mutant_counts()
