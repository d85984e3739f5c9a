"""The normalisation-edge streams (norm_edge_gen.py) on the CPU: the oracle against a plain restatement, and
the conditions under which a wrong score on the device would show.

1. The oracle's evaluation output -- every score plugin's weighted score and the TotalScore on every feasible
   node of every pod, for every family and profile, with the assumes (and the image family's remove_node /
   update_node) in between -- against norm_edge_gen.Model: DefaultNormalizeScore in both directions, the
   PodTopologySpread score and its NormalizeScore, InterPodAffinity's NormalizeScore, the ImageLocality sum,
   clamp and scale, the RequestedToCapacityRatio shape and round, in Python integers and floats.

2. Inside a persistent loop only the result tuple is visible, so a wrong score shows only where it moves the
   winner or the winner's TotalScore.  Per family, from the reference alone: every mutant of
   norm_edge_gen.MUTANTS changes a plugin score of the oracle's winning node on at least 5 placed pods; per
   stream, at least 90 % of the pods are placed, the winners cover at least 20 distinct nodes, and some node
   wins in both 128-node units and in both 64-lane halves.  And the branches the families are for are taken:
   BRANCHES below counts, per stream, the pods with an ignored PodTopologySpread node, with mx == 0, with
   max == min, with no raw InterPodAffinity score above 0, with no topologyScore entry, and the rest.

   Two mutants cannot meet the condition, for any generator: `<=` for `<` at ImageLocality's lower threshold
   and `>=` for `>` at its upper one.  calculatePriority clamps, so at sum == threshold both forms give the
   threshold.  test_clamp_strictness_changes_nothing checks that on every evaluated node (the stream holds sums
   exactly on both thresholds); the mutants that can show -- either clamp missing, and size * numNodes / N in
   integers -- stand in for them.

Measured for the committed generators (seed 0): MEASURED holds placed / distinct winners / pods on which each
mutant shows, per stream; test_measured_values_are_current keeps it in step with norm_edge_gen.

Findings: none in the oracle.  All seven plugin scores and the TotalScore of the 222 926 (pod, feasible node)
pairs equal the restatement's.
"""
import functools

import pytest

import norm_edge_gen as gen
from norm_edge_gen import Model, load
from oracle_binding import load as oracle_lib
from oracle_binding import oracle

PLUGINS = (gen.P_TAINT, gen.P_NA, gen.P_FIT, gen.P_PTS, gen.P_IPA, gen.P_BAL, gen.P_IMG)
IDS = [f"{f}-{p}" for f, p in gen.STREAMS]

# family, profile -> (placed, distinct winners, {mutant: placed pods on whose winning node it changes a plugin score})
MEASURED = {('ipa', 'default'): (130, 86, {'integer division': 26, 'multiply first': 26}),
 ('ipa', 'hard5'): (130, 86, {'integer division': 26, 'multiply first': 26}),
 ('ipa', 'ignore'): (130, 93, {'integer division': 26, 'multiply first': 26}),
 ('pts', 'default'): (130, 117, {'mx - r': 92, 'mx == 0 branch': 30}),
 ('defaultnorm', 'default'): (130, 65, {'mx == 0 branch': 52}),
 ('defaultnorm', 'added'): (130, 38, {'mx == 0 branch': 26}),
 ('image', 'default'): (130,
                        97,
                        {'<= at the lower threshold': 0,
                         '>= at the upper threshold': 0,
                         'no lower clamp': 21,
                         'no upper clamp': 7,
                         'integer scale': 39}),
 ('rtcr', 'descending'): (130, 65, {'truncation': 82, 'round half even': 34, 'floor in the shape': 104}),
 ('rtcr', 'ascending'): (130, 41, {'truncation': 33, 'round half even': 10, 'floor in the shape': 0}),
 ('rtcr', 'point'): (130, 88, {'truncation': 0, 'round half even': 0, 'floor in the shape': 0})}
# family, profile -> {branch: pods that take it}
BRANCHES = {('ipa', 'default'): {'no topologyScore entry': 18,
                      'max == min': 13,
                      'all raw <= 0, min < 0': 21,
                      'min < 0 < max': 72,
                      'a float pair': 26},
 ('ipa', 'hard5'): {'no topologyScore entry': 18,
                    'max == min': 13,
                    'all raw <= 0, min < 0': 21,
                    'min < 0 < max': 72,
                    'a float pair': 26},
 ('ipa', 'ignore'): {'no topologyScore entry': 26,
                     'max == min': 13,
                     'all raw <= 0, min < 0': 21,
                     'min < 0 < max': 64,
                     'a float pair': 26},
 ('pts', 'default'): {'ignored node': 84, 'mx == 0': 30, 'mn > 0': 92, 'mn == mx > 0': 11, 'raw >= 2^31 - 2': 10},
 ('defaultnorm', 'default'): {'taints: mx == 0': 26,
                              'taints: 100 * r / mx no integer': 21,
                              'affinity: mx == 0': 26,
                              'affinity: three or more values': 40},
 ('defaultnorm', 'added'): {'taints: mx == 0': 26,
                            'taints: 100 * r / mx no integer': 21,
                            'affinity: mx == 0': 0,
                            'affinity: three or more values': 130},
 ('rtcr', 'descending'): {'k + 0.5, k even': 130,
                          'k + 0.5, k odd': 130,
                          'a resource dropped (s <= 0)': 79,
                          'no resource left': 0},
 ('rtcr', 'ascending'): {'k + 0.5, k even': 129,
                         'k + 0.5, k odd': 118,
                         'a resource dropped (s <= 0)': 130,
                         'no resource left': 130},
 ('rtcr', 'point'): {'k + 0.5, k even': 0,
                     'k + 0.5, k odd': 0,
                     'a resource dropped (s <= 0)': 0,
                     'no resource left': 0}}


def go_log(x):
    return oracle_lib().ksgo_go_log(x)


@functools.lru_cache(maxsize=None)
def run(family, profile):
    """One oracle pass over a stream: per pod (pod, result tuple, eval dict, snapshot node names)."""
    nodes, bound, steps = gen.stream(family)
    o = load(oracle(dict(gen.PROFILES[family][profile])), nodes, bound)
    assert o.node_names() == [gen.name_of(n) for n in nodes]
    out = []
    for step in steps:
        if step[0] == "pod":
            r, ev = o.schedule_one(o.compile(step[1]), assume=True, evaluate=True)
            out.append((r.as_tuple(), ev, o.node_names()))
        else:
            gen.apply_step(o, step)
            out.append(None)
    o.close()
    return nodes, bound, steps, out


def walk(family, profile):
    """The restatement stepped along the oracle's placements: yields (model, pod, result, eval, names, feasible)."""
    nodes, bound, steps, out = run(family, profile)
    model = Model(gen.PROFILES[family][profile], nodes, bound, go_log)
    for step, got in zip(steps, out):
        if step[0] != "pod":
            model.apply(step)
            continue
        res, ev, names = got
        assert names == list(model.nodes), "snapshot order"
        feasible = [i for i in range(len(names)) if ev["node_code"][i] == 0]
        yield model, step[1], res, ev, names, feasible
        if res[0] == 0:
            model.add_pod(names[res[1]], step[1])


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_oracle_matches_restatement(family, profile):
    checked = 0
    for k, (model, p, res, ev, names, feasible) in enumerate(walk(family, profile)):
        per, totals = model.scores(p, [names[i] for i in feasible])
        for at, i in enumerate(feasible):
            for pl in PLUGINS:
                got, want = ev["plugin_scores"][pl][i], per[pl][at]
                assert got == want, (f"{family}/{profile} pod {k} ({p['metadata']['name']}) node {i} plugin {pl}: oracle "
                                     f"{got}, restated {want}; spec {p['spec']}")
            assert ev["total_scores"][i] == totals[at], f"{family}/{profile} pod {k} node {i}: total"
            checked += 1
        if res[0] == 0:
            assert res[4] == totals[feasible.index(res[1])]
    print(f"{family}/{profile}: {checked} (pod, node) pairs")
    assert checked > 5000, checked


@functools.lru_cache(maxsize=None)
def facts(family, profile):
    """(placed, winners, {mutant: pods on which it changes a plugin score of the winning node})."""
    placed, winners = 0, set()
    shown = {name: 0 for name in gen.MUTANTS[family]}
    for model, p, res, ev, names, feasible in walk(family, profile):
        if res[0] != 0:
            continue
        placed += 1
        winners.add(res[1])
        fnames, at = [names[i] for i in feasible], feasible.index(res[1])
        ref, _ = model.scores(p, fnames)
        for name, rules in gen.MUTANTS[family].items():
            model.rules, keep = rules, model.rules
            mut, _ = model.scores(p, fnames)
            model.rules = keep
            shown[name] += any(mut[pl][at] != ref[pl][at] for pl in PLUGINS)
    return placed, winners, shown


@pytest.mark.parametrize("family,profile", gen.STREAMS, ids=IDS)
def test_streams_can_show_a_wrong_score(family, profile):
    placed, winners, shown = facts(family, profile)
    print(f"{family}/{profile}: placed {placed} of {gen.N_PODS}, {len(winners)} distinct winners, mutants {shown}")
    assert placed * 10 >= gen.N_PODS * 9, placed
    assert len(winners) >= 20, sorted(winners)
    assert {i // 128 for i in winners} == {0, 1}, sorted(winners)
    assert {i % 128 // 64 for i in winners} == {0, 1}, sorted(winners)


@pytest.mark.parametrize("family", gen.FAMILIES)
def test_mutants_show_on_the_winning_node(family):
    for name in gen.MUTANTS[family]:
        n = sum(facts(family, profile)[2][name] for profile in gen.PROFILES[family])
        print(f"{family}: {name}: {n} placed pods")
        if (family, name) in gen.EQUIVALENT:
            assert n == 0, (name, n)
        else:
            assert n >= 5, (name, n)


def test_clamp_strictness_changes_nothing():
    """`<=` / `>=` at ImageLocality's thresholds: no score differs on any evaluated node, and the stream has
    sums exactly on the lower threshold and on the upper one (of one and of two containers)."""
    at_lo = at_hi = nodes_seen = 0
    for model, p, res, ev, names, feasible in walk("image", "default"):
        pod = gen._PodRec(p)
        feas = [model.nodes[names[i]] for i in feasible]
        ref = model.image(pod, feas)
        for name in ("<= at the lower threshold", ">= at the upper threshold"):
            model.rules, keep = gen.MUTANTS["image"][name], model.rules
            assert model.image(pod, feas) == ref, name
            model.rules = keep
        sums = [model.image_sum(pod, n) for n in feas]
        at_lo += gen.MIN_T in sums
        at_hi += gen.MAX_T1 * len(pod.images) in sums
        nodes_seen += len(feas)
    print(f"image: {nodes_seen} nodes, pods with a sum on the lower threshold {at_lo}, on the upper {at_hi}")
    assert at_lo >= 3 and at_hi >= 3, (at_lo, at_hi)


@functools.lru_cache(maxsize=None)
def branches(family, profile):
    """Pods per branch of the normalisations, from the restatement's raw scores."""
    b = {}

    def hit(name, cond):
        b[name] = b.get(name, 0) + bool(cond)

    for model, p, res, ev, names, feasible in walk(family, profile):
        pod, feas = gen._PodRec(p), [model.nodes[names[i]] for i in feasible]
        if family == "pts":
            raw = model.pts_raw(pod, feas)
            live = [r for r in raw if r is not None]
            hit("ignored node", len(live) < len(raw))
            hit("mx == 0", max(live) == 0)
            hit("mn > 0", min(live) > 0)
            hit("mn == mx > 0", min(live) == max(live) > 0)
            hit("raw >= 2^31 - 2", max(live) >= gen.BIG_SKEW - 1)
        elif family == "ipa":
            raw = model.ipa_raw(pod, feas)
            hit("no topologyScore entry", raw is None)
            if raw is not None:
                hit("max == min", max(raw) == min(raw))
                hit("all raw <= 0, min < 0", max(raw) <= 0 and min(raw) < 0)
                hit("min < 0 < max", min(raw) < 0 < max(raw))
                hit("a float pair", any((r - min(raw), max(raw) - min(raw)) in gen.FLOAT_PAIRS for r in raw))
        elif family == "defaultnorm":
            per, _ = model.scores(p, [n.name for n in feas])
            t = [x // model.weights[gen.P_TAINT] for x in per[gen.P_TAINT]]
            hit("taints: mx == 0", min(t) == 100 and pod.tolerations)
            hit("taints: 100 * r / mx no integer", any(x not in (0, 25, 50, 75, 100) for x in t))
            if pod.preferred is not None or model.added:
                a = [x // model.weights[gen.P_NA] for x in per[gen.P_NA]]
                hit("affinity: mx == 0", max(a) == 0)
                hit("affinity: three or more values", len(set(a)) >= 3)
        elif family == "rtcr":
            q = [model.rtcr_quotient(pod, n) for n in feas]
            hit("k + 0.5, k even", any(ws and 2 * num % (2 * ws) == ws and num // ws % 2 == 0 for num, ws in q))
            hit("k + 0.5, k odd", any(ws and 2 * num % (2 * ws) == ws and num // ws % 2 == 1 for num, ws in q))
            hit("a resource dropped (s <= 0)", any(ws < (4 if n.alloc[2] else 2) for (num, ws), n in zip(q, feas)))
            hit("no resource left", any(ws == 0 for num, ws in q))
    return b


@pytest.mark.parametrize("family", [f for f in gen.FAMILIES if f != "image"])
def test_branches_are_taken(family):
    """Every branch on at least 3 pods of some profile of the family (the single-point RTCR shape scores every
    node 70 and the addedAffinity terms always match some node: not every profile has every branch)."""
    total = {}
    for profile in gen.PROFILES[family]:
        b = branches(family, profile)
        print(f"{family}/{profile}: {b}")
        for name, n in b.items():
            total[name] = max(total.get(name, 0), n)
    assert all(n >= 3 for n in total.values()), total


def test_measured_values_are_current():
    """MEASURED and BRANCHES are what the committed generators give: a change of norm_edge_gen shows here."""
    got = {s: (lambda a, w, m: (a, len(w), m))(*facts(*s)) for s in gen.STREAMS}
    assert got == MEASURED, got
    gotb = {s: branches(*s) for s in gen.STREAMS if s[0] != "image"}
    assert gotb == BRANCHES, gotb
