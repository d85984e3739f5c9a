"""Seeded clusters and pod streams that sit on the edges of NormalizeScore, the weighted sum, the
PodTopologySpread raw score, RequestedToCapacityRatio and ImageLocality, and a plain restatement of them.

fuzz_gen's random streams use weights 1-100, a few pods per domain, four image sizes and one RTCR shape: they
almost never land where these expressions are fragile.  The families here do:

  ipa          preferred (anti-)affinity terms whose weights and matching-pod counts put (r - min, max - min) on
               the 13 pairs below 400 where int64(100.0 * (float64(r - min) / float64(max - min))) differs from
               100 * (r - min) / (max - min) (FLOAT_PAIRS, enumerated here), with min at 0 and below it; pods with
               anti-affinity only (every raw score <= 0), pods whose terms match nothing anywhere (no topologyScore
               entry: PreScore skips), pods on which every node scores alike (max == min), cluster-wide pods over
               the 3-, 7- and 29-domain keys, and bound pods with preferred and required terms of their own
               (symmetry, hardPodAffinityWeight).  Profiles: default, hardPodAffinityWeight 5,
               ignorePreferredTermsOfExistingPods
  pts          one and two ScheduleAnyway constraints on hostname and the 3-, 7- and 29-domain keys, nodes that
               lack a key (raw -1), pods for which every raw score is 0 (mx == 0), maxSkew 1, 3 and 2^31 - 1, a
               single-domain slice selected by a nodeSelector under nodeAffinityPolicy Honor
  defaultnorm  0-4 PreferNoSchedule taints with partial tolerations (a pod that tolerates them all: mx == 0, every
               node 100), preferred NodeAffinity sums whose 100 * r / mx is not an integer, preferences that match
               no node; profiles: default, addedAffinity preferred terms
  image        sums at 23 MiB - 1, 23 MiB, 1000 MiB * containers and above, size * numNodes / N that is no
               integer (IMAGE_AIMED: sizes at which the float form is one short of the integer form right on a
               score step), 1-3 containers, an init container, a repeated image, an image no node has, one image
               reported with different sizes by different nodes (the first registrant fixes the size), and half-way
               a remove_node of that first registrant and an update_node that changes a node's image list
  rtcr         three RequestedToCapacityRatio profiles (descending, ascending with a zero-score first segment,
               single point), cpu and memory equally weighted so that the quotient lands on k + 0.5, and
               ephemeral-storage (weight 2) that some nodes lack

Every stream is 200 hostname-labelled nodes (two 128-node units, the second partial), 150-400 bound pods and
about 130 incoming pods, as plain JSON objects; a stream's steps are ("pod", pod), ("remove_node", name) and
("update_node", node).  Zone-like keys come with 3, 7 and 29 domains, and some nodes lack each.

Model is the restatement: node and pod state in Python integers and floats, no call into the oracle (but for
ksgo_go_log, the reference's logarithm, which is pinned elsewhere).
"""
import math
import random

N_NODES, N_PODS = 200, 130
MIB = 1024 * 1024
FAMILIES = ["ipa", "pts", "defaultnorm", "image", "rtcr"]
HOSTNAME = "kubernetes.io/hostname"


def _rtcr(shape):
    return {"nodeResourcesFit": {"scoringStrategy": {
        "type": "RequestedToCapacityRatio",
        "resources": [{"name": "cpu", "weight": 1}, {"name": "memory", "weight": 1},
                      {"name": "ephemeral-storage", "weight": 2}],
        "requestedToCapacityRatio": {"shape": [{"utilization": u, "score": s} for u, s in shape]}}}}


def _pref(weight, key, op, values=None):
    e = {"key": key, "operator": op}
    if values is not None:
        e["values"] = list(values)
    return {"weight": weight, "preference": {"matchExpressions": [e]}}


PROFILES = {
    "ipa": {
        "default": {},
        "hard5": {"interPodAffinity": {"hardPodAffinityWeight": 5}},
        "ignore": {"interPodAffinity": {"ignorePreferredTermsOfExistingPods": True}},
    },
    "pts": {"default": {}},
    "defaultnorm": {
        "default": {},
        "added": {"nodeAffinity": {"addedAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
            _pref(11, "zone3", "In", ["z1"]), _pref(3, "zone29", "In", ["d5", "d6", "d7"])]}}},
    },
    "image": {"default": {}},
    "rtcr": {
        "descending": _rtcr([(0, 10), (60, 3), (100, 0)]),
        "ascending": _rtcr([(0, 0), (40, 0), (100, 10)]),
        "point": _rtcr([(50, 7)]),
    },
}
STREAMS = [(f, p) for f in FAMILIES for p in PROFILES[f]]


# ---- objects ----------------------------------------------------------------------------------------------
def topo_labels(i):
    name = f"norm-{i:04d}"
    lab = {HOSTNAME: name, "region": "r1", "grp": f"g{i % 67}"}
    if i % 10 != 9:
        lab["zone3"] = f"z{i % 3}"
    if i % 13 != 12:
        lab["zone7"] = f"s{i * 3 % 7}"
    if i % 17 != 16:
        lab["zone29"] = f"d{i % 29}"
    return lab


def node(i, cpu_milli=8000, mem=16 << 30, pods=110, eph=None, taints=None, images=None, labels=None):
    name = f"norm-{i:04d}"
    alloc = {"cpu": f"{cpu_milli}m", "memory": str(mem), "pods": str(pods)}
    if eph is not None:
        alloc["ephemeral-storage"] = str(eph)
    n = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": name, "labels": dict(labels or topo_labels(i))},
         "spec": {}, "status": {"allocatable": alloc, "capacity": alloc}}
    if taints:
        n["spec"]["taints"] = [dict(t) for t in taints]
    if images:
        n["status"]["images"] = [{"names": [nm], "sizeBytes": int(sz)} for nm, sz in images]
    return n


def pod(name, app, cpu=100, mem=256 * MIB, eph=None, node_name=None, images=("norm.example/none:1",), init_image=None):
    def ctr(k, img, c, m, e):
        r = {"cpu": f"{c}m", "memory": str(m)}
        if e is not None:
            r["ephemeral-storage"] = str(e)
        return {"name": f"c{k}", "image": img, "resources": {"requests": r}}

    cs = [ctr(k, img, cpu if k == 0 else 1, mem if k == 0 else 1, eph if k == 0 else None) for k, img in enumerate(images)]
    p = {"apiVersion": "v1", "kind": "Pod",
         "metadata": {"name": name, "namespace": "default", "uid": name, "labels": {"app": app}},
         "spec": {"containers": cs}, "status": {}}
    if init_image is not None:
        p["spec"]["initContainers"] = [ctr(9, init_image, 1, 1, None)]
    if node_name:
        p["spec"]["nodeName"] = node_name
    return p


def term(key, app):
    return {"topologyKey": key, "labelSelector": {"matchLabels": {"app": app}}}


def add_pod_terms(p, kind, preferred=(), required=()):
    """kind: podAffinity / podAntiAffinity; preferred: (weight, term) pairs; required: terms."""
    a = p["spec"].setdefault("affinity", {}).setdefault(kind, {})
    if preferred:
        a.setdefault("preferredDuringSchedulingIgnoredDuringExecution", []).extend(
            {"weight": w, "podAffinityTerm": t} for w, t in preferred)
    if required:
        a.setdefault("requiredDuringSchedulingIgnoredDuringExecution", []).extend(required)
    return p


def spread(key, app, max_skew, honor=None):
    c = {"maxSkew": max_skew, "topologyKey": key, "whenUnsatisfiable": "ScheduleAnyway",
         "labelSelector": {"matchLabels": {"app": app}}}
    if honor is not None:
        c["nodeAffinityPolicy"] = honor
    return c


def name_of(n):
    return n["metadata"]["name"]


# ---- ipa --------------------------------------------------------------------------------------------------
def float_pairs(limit=400):
    """(r - min, max - min) below `limit` where the reference's float form and the integer form differ."""
    return [(a, d) for d in range(1, limit) for a in range(d + 1) if int(100.0 * (a / d)) != 100 * a // d]


FLOAT_PAIRS = float_pairs()
PREFER_NO = {"key": "norm/busy", "value": "v", "effect": "PreferNoSchedule"}


def _factor(v):
    """v = weight * count with weight <= 100 and the fewest pods (at most 8), or None."""
    for c in range(1, 9):
        if v % c == 0 and v // c <= 100:
            return v // c, c
    return None


def _ipa(rng):
    # groups of three nodes (g, g + 67, g + 134) selected by the grp label: within one, the raw scores are
    # min, min + a, min + d for a pair (a, d); the min and the max node carry a PreferNoSchedule taint, so that
    # the node in between -- the one whose normalised score the pair decides -- wins by TaintToleration
    groups = [(g, [g, g + 67, g + 134]) for g in range(66)]
    aimed = []  # (group, pair, negative minimum)
    for k, pr in enumerate(FLOAT_PAIRS + FLOAT_PAIRS):
        aimed.append((groups[2 * k + 1], pr, k >= len(FLOAT_PAIRS)))
    tainted, bound = set(), []
    plan = []
    for (g, members), (a, d), neg in aimed:
        rot = g % 3
        lo, mid, hi = members[rot], members[(rot + 1) % 3], members[(rot + 2) % 3]
        tainted |= {lo, hi}
        # the minimum node's raw score is -m
        m = rng.choice([m for m in range(3, 90) if m != a and all(_factor(abs(v - m)) for v in (a, d))]) if neg else 0
        wants = [(mid, a - m, "a"), (hi, d - m, "d")] + ([(lo, -m, "m")] if neg else [])
        terms = []
        for at, v, tag in wants:
            if v == 0:
                continue
            w, c = _factor(abs(v))
            app = f"{tag}{g}"
            for j in range(c):
                bound.append(pod(f"bound-{tag}{g}-{j}", app, node_name=f"norm-{at:04d}"))
            terms.append((v > 0, w, term(HOSTNAME, app)))
        plan.append((g, terms))
    nodes = [node(i, taints=[PREFER_NO] if i in tainted else None) for i in range(N_NODES)]
    names = [name_of(n) for n in nodes]
    # service pods the cluster-wide terms select, uneven over the domains
    for k in range(110):
        i = rng.choice([rng.randrange(N_NODES), rng.randrange(40), 3 * rng.randrange(20)])
        bound.append(pod(f"bound-svc-{k}", rng.choice(["web", "web", "db", "cache"]), node_name=names[i]))
    # bound pods with terms of their own towards the incoming pods' labels (front / back)
    for k in range(40):
        p = pod(f"bound-own-{k}", "own", node_name=names[rng.randrange(N_NODES)])
        key = rng.choice(["zone3", "zone7", "zone29", HOSTNAME])
        r = k % 4
        if r == 0:
            add_pod_terms(p, "podAffinity", preferred=[(rng.randrange(1, 101), term(key, "front"))])
        elif r == 1:
            add_pod_terms(p, "podAntiAffinity", preferred=[(rng.randrange(1, 101), term(key, "back"))])
        elif r == 2:
            add_pod_terms(p, "podAffinity", required=[term(key, "front")])
        else:
            add_pod_terms(p, "podAffinity", preferred=[(rng.randrange(1, 101), term(key, "back"))], required=[term(key, "own")])
            add_pod_terms(p, "podAntiAffinity", preferred=[(rng.randrange(1, 101), term("zone3", "front"))])
        bound.append(p)
    incoming = []
    for g, terms in plan:
        p = pod(f"in-aim-{g}", "aimed")
        p["spec"]["nodeSelector"] = {"grp": f"g{g}"}
        add_pod_terms(p, "podAffinity", preferred=[(w, t) for pos, w, t in terms if pos])
        add_pod_terms(p, "podAntiAffinity", preferred=[(w, t) for pos, w, t in terms if not pos])
        incoming.append(p)
    keys = ["zone3", "zone7", "zone29", HOSTNAME]
    k = 0
    while len(incoming) < N_PODS:
        kind = k % 8
        k += 1
        app = rng.choice(["front", "back", "plain"])
        p = pod(f"in-{k}", app, cpu=rng.choice([100, 250, 500]))
        wt = lambda: rng.choice([1, 3, 29, 57, 58, 87, 100, rng.randrange(1, 101)])
        if kind in (0, 1):  # affinity and anti-affinity over two keys
            add_pod_terms(p, "podAffinity", preferred=[(wt(), term(rng.choice(keys), rng.choice(["web", "db"])))])
            add_pod_terms(p, "podAntiAffinity", preferred=[(wt(), term(rng.choice(keys), rng.choice(["web", "cache"])))])
        elif kind == 2:  # anti-affinity only: every raw score <= 0 (bound pods' own terms aside: app plain)
            p["metadata"]["labels"]["app"] = "plain"
            add_pod_terms(p, "podAntiAffinity", preferred=[(wt(), term(rng.choice(keys), "web")), (wt(), term("zone29", "db"))])
        elif kind == 3:  # terms that match nothing, and a label no bound pod's term selects
            p["metadata"]["labels"]["app"] = "plain"
            add_pod_terms(p, "podAffinity", preferred=[(wt(), term(rng.choice(keys), "nobody"))])
        elif kind == 4:  # every node alike: one domain
            p["metadata"]["labels"]["app"] = "plain"
            add_pod_terms(p, rng.choice(["podAffinity", "podAntiAffinity"]), preferred=[(wt(), term("region", "web"))])
        elif kind == 5:  # no terms: the bound pods' own terms alone
            pass
        elif kind == 6:  # small weights beside the bound pods' required terms towards "front": hardPodAffinityWeight shows
            p["metadata"]["labels"]["app"] = "front"
            add_pod_terms(p, "podAffinity", preferred=[(rng.randrange(1, 4), term(rng.choice(keys), "front")),
                                                       (rng.randrange(1, 4), term("zone7", "web"))])
        else:
            add_pod_terms(p, "podAntiAffinity", preferred=[(wt(), term(HOSTNAME, rng.choice(["front", "back"])))])
            add_pod_terms(p, "podAffinity", preferred=[(wt(), term("zone7", "cache"))])
        incoming.append(p)
    rng.shuffle(incoming)
    return nodes, bound, [("pod", p) for p in incoming]


# ---- pts --------------------------------------------------------------------------------------------------
BIG_SKEW = (1 << 31) - 1


def _pts(rng):
    nodes = [node(i) for i in range(N_NODES)]
    names = [name_of(n) for n in nodes]
    bound = []
    for k in range(200):
        i = rng.choice([rng.randrange(N_NODES), rng.randrange(60), 3 * rng.randrange(30), 7 * rng.randrange(20)])
        bound.append(pod(f"bound-{k}", rng.choice(["web", "web", "db", "cache"]), node_name=names[i]))
    for i in range(N_NODES):  # every node hosts a "full" pod: the minimum raw score of its spread is above 0
        bound.append(pod(f"bound-full-{i}", "full", cpu=10, mem=MIB, node_name=names[i]))
    keys = [HOSTNAME, "zone3", "zone7", "zone29"]
    incoming = []
    for k in range(N_PODS):
        kind = k % 13
        app = rng.choice(["web", "db", "cache"])
        p = pod(f"in-{k}", app, cpu=rng.choice([100, 250]))
        skew = rng.choice([1, 1, 3])
        if kind in (0, 1, 2):
            cs = [spread(keys[k // 13 % 4], app, skew)]
        elif kind in (3, 4):
            a, b = rng.sample(keys, 2)
            cs = [spread(a, app, skew), spread(b, rng.choice(["web", "db"]), rng.choice([1, 3]))]
        elif kind == 5:  # nothing matches and maxSkew 1: every raw score 0
            cs = [spread(rng.choice(keys), "nobody", 1)]
        elif kind == 6:
            cs = [spread(HOSTNAME, "nobody", 1), spread(rng.choice(keys[1:]), "nobody", 1)]
        elif kind == 7:  # one domain: the zone3 slice of the nodeSelector, under Honor
            z = f"z{rng.randrange(3)}"
            p["spec"]["nodeSelector"] = {"zone3": z}
            cs = [spread("zone3", app, skew, honor="Honor")]
        elif kind == 8:
            p["spec"]["nodeSelector"] = {"zone7": f"s{rng.randrange(7)}"}
            cs = [spread("zone7", "nobody", 1, honor="Honor"), spread(HOSTNAME, "nobody", 1)]
        elif kind == 9:
            cs = [spread(rng.choice(keys), app, BIG_SKEW)]
        elif kind == 10:  # the minimum above 0 with maxSkew 1: every node hosts one "full" pod
            p["metadata"]["labels"]["app"] = "full"
            cs = [spread(HOSTNAME, "full", 1)]
        elif kind == 11:
            cs = [spread("zone29", "full", 3), spread(HOSTNAME, app, 1)]
        else:
            cs = [spread(rng.choice(keys), app, 3, honor="Ignore")]
        p["spec"]["topologySpreadConstraints"] = cs
        incoming.append(p)
    return nodes, bound, [("pod", p) for p in incoming]


# ---- defaultnorm ------------------------------------------------------------------------------------------
TAINTS = [{"key": f"norm/t{k}", "value": "v" if k % 2 else "w", "effect": "PreferNoSchedule"} for k in range(4)]


def _defaultnorm(rng):
    nodes = []
    for i in range(N_NODES):
        lab = topo_labels(i)
        if i % 4 == 1:
            lab["tier"] = "gold"
        if i % 6 == 2:
            lab["disk"] = rng.choice(["ssd", "hdd"])
        cnt = i * 7 % 5
        nodes.append(node(i, taints=rng.sample(TAINTS, cnt), labels=lab, cpu_milli=rng.choice([4000, 8000])))
    names = [name_of(n) for n in nodes]
    bound = [pod(f"bound-{k}", "svc", cpu=rng.choice([100, 500, 900]), mem=rng.choice([1, 2, 3]) << 29,
                 node_name=names[rng.randrange(N_NODES)]) for k in range(200)]

    def tol(t, how):
        if how == 0:
            return {"key": t["key"], "operator": "Exists", "effect": "PreferNoSchedule"}
        if how == 1:
            return {"key": t["key"], "operator": "Equal", "value": t["value"]}  # every effect
        if how == 2:
            return {"key": t["key"], "operator": "Equal", "value": "other", "effect": "PreferNoSchedule"}  # no match
        return {"key": t["key"], "operator": "Exists", "effect": "NoSchedule"}  # not the PreferNoSchedule one

    prefs = [lambda w: _pref(w, "zone3", "In", ["z0"]), lambda w: _pref(w, "zone7", "In", ["s1", "s4"]),
             lambda w: _pref(w, "zone29", "NotIn", ["d0", "d1", "d2", "d3"]), lambda w: _pref(w, "tier", "Exists"),
             lambda w: _pref(w, "disk", "In", ["ssd"]), lambda w: _pref(w, "zone29", "DoesNotExist")]
    incoming = []
    for k in range(N_PODS):
        kind = k % 10
        p = pod(f"in-{k}", "norm", cpu=rng.choice([100, 250, 500]), mem=rng.choice([1, 2]) << 28)
        if kind in (0, 1, 2, 3):  # partial tolerations
            p["spec"]["tolerations"] = [tol(t, rng.randrange(4)) for t in rng.sample(TAINTS, rng.randrange(1, 4))]
        elif kind == 4:  # tolerates every PreferNoSchedule taint: mx == 0, every node 100
            p["spec"]["tolerations"] = [rng.choice([{"operator": "Exists"}, {"operator": "Exists", "effect": "PreferNoSchedule"}])]
        elif kind == 5:
            p["spec"]["tolerations"] = [tol(t, 0) for t in TAINTS]
        if kind in (1, 2, 5, 6, 7):  # sums of odd weights: 100 * r / mx is rarely an integer
            ws = rng.sample([7, 13, 29, 3, 41, 97, 1, 100], rng.randrange(1, 4))
            p["spec"].setdefault("affinity", {})["nodeAffinity"] = {"preferredDuringSchedulingIgnoredDuringExecution": [
                f(w) for f, w in zip(rng.sample(prefs, len(ws)), ws)]}
        elif kind in (8, 9):  # preferences that match no node
            p["spec"].setdefault("affinity", {})["nodeAffinity"] = {"preferredDuringSchedulingIgnoredDuringExecution": [
                _pref(rng.randrange(1, 101), "zone3", "In", ["nowhere"]), _pref(5, "absent", "Exists")]}
        incoming.append(p)
    return nodes, bound, [("pod", p) for p in incoming]


# ---- image ------------------------------------------------------------------------------------------------
MIN_T, MAX_T1 = 23 * MIB, 1000 * MIB
FIRST, SOLO = 9, 21  # the differing-size image's first registrant (pods: 0, never hosts); the updated node


def image_aimed(n_nodes, holder_counts=range(3, 60)):
    """[(size, score step j, holders)]: sizes whose scaled value size * holders / n_nodes is exactly the least sum
    at which a one-container pod's score steps to j, and whose float form
    int64(float64(size) * (float64(holders) / float64(n_nodes))) is one short of it."""
    out = []
    span = MAX_T1 - MIN_T
    for h in holder_counts:
        for j in range(1, 100):
            t = MIN_T + -(-j * span // 100)  # the least sum that scores j
            if t * n_nodes % h == 0 and int(float(t * n_nodes // h) * (float(h) / float(n_nodes))) == t - 1:
                out.append((t * n_nodes // h, j, h))
    return out


# for the whole cluster (the stream's first half) and for the 199 nodes left after the remove_node (its second)
IMAGE_AIMED = image_aimed(N_NODES)
IMAGE_AIMED_LATE = image_aimed(N_NODES - 1)


def _image(rng):
    half = list(range(0, N_NODES, 2))  # 100 holders: the scaled size is half the size
    sets = {
        "norm.example/lo:1": (2 * MIN_T - 2, half),              # scaled 23 MiB - 1
        "norm.example/min:1": (2 * MIN_T, half),                 # 23 MiB
        "norm.example/min1:1": (2 * MIN_T + 2, half),            # 23 MiB + 1
        "norm.example/max1:1": (2 * MAX_T1 - 2, half),           # 1000 MiB - 1
        "norm.example/max:1": (2 * MAX_T1, half),                # 1000 MiB: the threshold of one container
        "norm.example/over:1": (2 * MAX_T1 + 2, half),           # 1000 MiB + 1
        "norm.example/huge:1": (9000 * MIB, list(range(1, N_NODES, 2))),
        "norm.example/mid:1": (1234567891, [i for i in range(N_NODES) if i % 3 == 0]),
        "norm.example/untagged": (777 * MIB + 1, [i for i in range(N_NODES) if i % 5 == 1]),  # ":latest" is appended
    }
    aimed = ([], [])
    for late, table in enumerate((IMAGE_AIMED, IMAGE_AIMED_LATE)):
        for k, (size, j, h) in enumerate(table):
            holders = rng.sample([i for i in range(N_NODES) if i not in (FIRST, SOLO)], h)
            nm = f"norm.example/aim{late}-{k}:1"
            sets[nm] = (size, holders)
            aimed[late].append(nm)
    per_node = [[] for _ in range(N_NODES)]
    for nm, (s, holders) in sets.items():
        for i in holders:
            per_node[i].append((nm + (":latest" if nm.endswith("untagged") else ""), s))
    # one image, two sizes: node FIRST registers it first with 3000 MiB, 59 later nodes say 400 MiB
    dup = "norm.example/dup:1"
    per_node[FIRST].append((dup, 3000 * MIB))
    for i in range(30, 148, 2):
        per_node[i].append((dup, 400 * MIB))
    per_node[SOLO] = [("norm.example/solo:1", 5000 * MIB), (dup, 400 * MIB)] + per_node[SOLO]
    nodes = [node(i, images=per_node[i], pods=0 if i == FIRST else 110, cpu_milli=rng.choice([4000, 8000]))
             for i in range(N_NODES)]
    names = [name_of(n) for n in nodes]
    bound = [pod(f"bound-{k}", "svc", cpu=rng.choice([100, 300, 700]), mem=rng.choice([1, 2, 3]) << 28,
                 node_name=names[rng.choice([i for i in range(N_NODES) if i != FIRST])]) for k in range(180)]
    common = [nm for nm in sets if "aim" not in nm]
    steps = []
    for k in range(N_PODS):
        kind = k % 10
        init = None
        if kind in (0, 1, 2):
            tab = aimed[k >= N_PODS // 2]
            imgs = [tab[(k // 10 * 3 + kind) % len(tab)]]
        elif kind == 3:
            imgs = [rng.choice(common)]
        elif kind == 4:
            imgs = rng.sample(common, 2)
        elif kind == 5:
            imgs = rng.sample(common, 3)
        elif kind == 6:  # the same image twice: counted twice, and the threshold is two containers'
            nm = rng.choice(["norm.example/max:1", "norm.example/over:1", "norm.example/mid:1", dup])
            imgs = [nm, nm]
        elif kind == 7:
            imgs = [rng.choice([dup, "norm.example/solo:1", "norm.example/untagged"])]
        elif kind == 8:
            imgs = [rng.choice(["norm.example/nowhere:1", "norm.example/lo:1", "norm.example/min:1"])]
        else:
            imgs = [rng.choice(common)]
            init = rng.choice(common + [dup])
        if k == N_PODS // 2:
            steps.append(("remove_node", names[FIRST]))
            upd = node(SOLO, images=[("norm.example/solo:1", 700 * MIB), ("norm.example/mid:1", 1234567891)],
                       cpu_milli=int(nodes[SOLO]["status"]["allocatable"]["cpu"][:-1]))
            steps.append(("update_node", upd))
        steps.append(("pod", pod(f"in-{k}", "img", cpu=rng.choice([100, 200]), images=imgs, init_image=init)))
    return nodes, bound, steps


# ---- rtcr -------------------------------------------------------------------------------------------------
def _rtcr_family(rng):
    nodes = []
    for i in range(N_NODES):
        cpu = rng.choice([2000, 4000, 5000, 8000])
        mem = rng.choice([4, 8, 10, 16]) << 30
        eph = None if i % 3 == 2 else rng.choice([100, 250]) << 30
        nodes.append(node(i, cpu_milli=cpu, mem=mem, eph=eph, pods=rng.choice([4, 6, 110])))
    names = [name_of(n) for n in nodes]
    bound = []
    for k in range(300):
        i = rng.randrange(N_NODES)
        a = nodes[i]["status"]["allocatable"]
        cpu = int(a["cpu"][:-1]) * rng.choice([5, 10, 15, 20, 35]) // 100
        mem = int(a["memory"]) * rng.choice([5, 10, 20, 30]) // 100 + rng.choice([0, 1])
        eph = int(a["ephemeral-storage"]) * rng.choice([10, 30, 50]) // 100 if "ephemeral-storage" in a and k % 2 else None
        bound.append(pod(f"bound-{k}", "svc", cpu=cpu, mem=mem, eph=eph, node_name=names[i]))
    incoming = []
    for k in range(N_PODS):
        eph = rng.choice([None, None, 1 << 30, 20 << 30])
        incoming.append(pod(f"in-{k}", "rtcr", cpu=rng.choice([50, 100, 200, 400, 1000]),
                            mem=rng.choice([1 << 27, 1 << 28, 3 << 28, 1 << 30, (1 << 30) + 1]), eph=eph))
    return nodes, bound, [("pod", p) for p in incoming]


def stream(family, seed=0):
    """-> (nodes, bound pods, steps) of one family, deterministic in (family, seed)."""
    rng = random.Random(f"norm-{family}-{seed}")
    return {"ipa": _ipa, "pts": _pts, "defaultnorm": _defaultnorm, "image": _image, "rtcr": _rtcr_family}[family](rng)


def load(b, nodes, bound):
    b.upsert_namespace({"metadata": {"name": "default"}})
    for n in nodes:
        b.add_node(n)
    for p in bound:
        b.add_pod(p)
    return b


def apply_step(b, step):
    """A non-pod step on a backend (product or oracle)."""
    if step[0] == "remove_node":
        b.remove_node(step[1])
    elif step[0] == "update_node":
        b.update_node(step[1])
    else:
        raise ValueError(step[0])


def runs(steps):
    """The steps as [(non-pod steps before the run, [pods])]: what a batch path submits together."""
    out, pre, cur = [], [], []
    for s in steps:
        if s[0] == "pod":
            cur.append(s[1])
        else:
            if cur:
                out.append((pre, cur))
                pre, cur = [], []
            pre.append(s)
    if cur or pre:
        out.append((pre, cur))
    return out


def pods_of(steps):
    return [s[1] for s in steps if s[0] == "pod"]


# ---- the plain restatement ----------------------------------------------------------------------------------
P_TAINT, P_NA, P_FIT, P_PTS, P_IPA, P_BAL, P_IMG = 2, 3, 5, 6, 7, 8, 9  # ksg.abi.PLUGINS indices
DEFAULT_WEIGHTS = {P_TAINT: 3, P_NA: 2, P_FIT: 1, P_PTS: 2, P_IPA: 2, P_BAL: 1, P_IMG: 1}
PLUGIN_NAMES = {"TaintToleration": P_TAINT, "NodeAffinity": P_NA, "NodeResourcesFit": P_FIT, "PodTopologySpread": P_PTS,
                "InterPodAffinity": P_IPA, "NodeResourcesBalancedAllocation": P_BAL, "ImageLocality": P_IMG}


def go_div(a, b):
    """Go's integer division: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def go_round(x):
    """math.Round: half away from zero (x - trunc(x) is exact in binary64)."""
    t = math.trunc(x)
    if abs(x - t) >= 0.5:
        t += 1 if x > 0 else -1
    return t


def round_half_even(x):
    t = math.trunc(x)
    f = abs(x - t)
    if f > 0.5 or (f == 0.5 and t % 2):
        t += 1 if x > 0 else -1
    return t


def milli(q):
    return int(q[:-1]) if q.endswith("m") else int(q) * 1000


def normalized_image(name):
    return name + ":latest" if name.rfind(":") <= name.rfind("/") else name


class Rules:
    """The expressions under test, one method each; a mutant overrides one."""

    def default_normalize(self, raw, reverse):  # helper/normalize_score.go
        mx = max([0] + list(raw))
        if mx == 0:
            return [self.default_zero(reverse) for _ in raw]
        return [100 - go_div(100 * r, mx) if reverse else go_div(100 * r, mx) for r in raw]

    def default_zero(self, reverse):
        return 100 if reverse else 0

    def pts_normalize(self, raw):  # raw None: an ignored node
        live = [r for r in raw if r is not None]
        mn, mx = min(live, default=0), max([0] + live)
        return [0 if r is None else self.pts_zero() if mx == 0 else self.pts_one(r, mn, mx) for r in raw]

    def pts_zero(self):
        return 100

    def pts_one(self, r, mn, mx):
        return go_div(100 * (mx + mn - r), mx)

    def ipa_normalize(self, raw):
        mn, mx = min(raw), max(raw)
        return [self.ipa_one(r - mn, mx - mn) if mx > mn else 0 for r in raw]

    def ipa_one(self, a, d):
        return int(100.0 * (float(a) / float(d)))

    def image_scaled(self, size, holders, total):
        return int(float(size) * (float(holders) / float(total)))

    def image_priority(self, s, count):
        lo, hi = MIN_T, MAX_T1 * count
        s = self.image_clamp(s, lo, hi)
        return go_div(100 * (s - lo), hi - lo)

    def image_clamp(self, s, lo, hi):
        return lo if s < lo else hi if s > hi else s

    def shape(self, shape, p):  # helper/shape_score.go; shape: (utilization, score * 10)
        for i, (u, s) in enumerate(shape):
            if p <= u:
                if i == 0:
                    return shape[0][1]
                u0, s0 = shape[i - 1]
                return s0 + self.shape_div((s - s0) * (p - u0), u - u0)
        return shape[-1][1]

    def shape_div(self, a, b):
        return go_div(a, b)

    def rtcr_round(self, x):
        return go_round(x)


def mutant(**methods):
    return type("Mutant", (Rules,), methods)()


MUTANTS = {
    "ipa": {
        "integer division": mutant(ipa_one=lambda self, a, d: 100 * a // d),
        "multiply first": mutant(ipa_one=lambda self, a, d: int(100.0 * float(a) / float(d))),
    },
    "pts": {
        "mx - r": mutant(pts_one=lambda self, r, mn, mx: go_div(100 * (mx - r), mx)),
        "mx == 0 branch": mutant(pts_zero=lambda self: 0),
    },
    "defaultnorm": {
        "mx == 0 branch": mutant(default_zero=lambda self, reverse: 0 if reverse else 100),
    },
    "image": {
        # `<=` for `<` (or `>=` for `>`) in a clamp changes no value: at s == T both sides give T (EQUIVALENT, and
        # the CPU module checks that on sums that sit on both thresholds).  The mutants that can show are a
        # missing clamp on either side and the scaled size in integers.
        "<= at the lower threshold": mutant(image_clamp=lambda self, s, lo, hi: lo if s <= lo else hi if s > hi else s),
        ">= at the upper threshold": mutant(image_clamp=lambda self, s, lo, hi: lo if s < lo else hi if s >= hi else s),
        "no lower clamp": mutant(image_clamp=lambda self, s, lo, hi: hi if s > hi else s),
        "no upper clamp": mutant(image_clamp=lambda self, s, lo, hi: lo if s < lo else s),
        "integer scale": mutant(image_scaled=lambda self, size, holders, total: size * holders // total),
    },
    "rtcr": {
        "truncation": mutant(rtcr_round=lambda self, x: math.trunc(x)),
        "round half even": mutant(rtcr_round=lambda self, x: round_half_even(x)),
        "floor in the shape": mutant(shape_div=lambda self, a, b: a // b),
    },
}
EQUIVALENT = {("image", "<= at the lower threshold"), ("image", ">= at the upper threshold")}


def _terms(p, kind, which):
    a = p["spec"].get("affinity", {}).get(kind, {})
    if which == "required":
        return [(t["topologyKey"], t["labelSelector"]["matchLabels"]) for t in
                a.get("requiredDuringSchedulingIgnoredDuringExecution", [])]
    return [(t["weight"], (t["podAffinityTerm"]["topologyKey"], t["podAffinityTerm"]["labelSelector"]["matchLabels"]))
            for t in a.get("preferredDuringSchedulingIgnoredDuringExecution", [])]


def _sel_matches(sel, labels):
    return all(labels.get(k) == v for k, v in sel.items())


def _expr_matches(e, labels):
    op, k = e["operator"], e["key"]
    if op == "In":
        return k in labels and labels[k] in e["values"]
    if op == "NotIn":
        return k not in labels or labels[k] not in e["values"]
    if op == "Exists":
        return k in labels
    if op == "DoesNotExist":
        return k not in labels
    raise ValueError(op)


def _tolerates(tol, taint):
    if tol.get("effect") and tol["effect"] != taint["effect"]:
        return False
    if tol.get("key") and tol["key"] != taint["key"]:
        return False
    if tol.get("operator", "Equal") == "Exists":
        return True
    return tol.get("value", "") == taint.get("value", "")


class _PodRec:
    def __init__(self, p):
        self.labels = p["metadata"]["labels"]
        self.pref_aff, self.pref_anti = _terms(p, "podAffinity", "preferred"), _terms(p, "podAntiAffinity", "preferred")
        self.req_aff = _terms(p, "podAffinity", "required")
        a = p["spec"].get("affinity", {})
        self.has_affinity = "podAffinity" in a or "podAntiAffinity" in a
        cs, ini = p["spec"]["containers"], p["spec"].get("initContainers", [])

        def req(c, name, default):
            r = c.get("resources", {}).get("requests", {})
            if name not in r:
                return default
            return milli(r[name]) if name == "cpu" else int(r[name])

        def total(name, default):
            return max([sum(req(c, name, default) for c in cs)] + [req(c, name, default) for c in ini])

        self.cpu, self.mem, self.eph = total("cpu", 0), total("memory", 0), total("ephemeral-storage", 0)
        self.nz_cpu, self.nz_mem = total("cpu", 100), total("memory", 200 * MIB)
        self.images = [c["image"] for c in ini] + [c["image"] for c in cs]
        self.tolerations = p["spec"].get("tolerations", [])
        self.node_selector = p["spec"].get("nodeSelector", {})
        na = p["spec"].get("affinity", {}).get("nodeAffinity", {})
        self.preferred = na.get("preferredDuringSchedulingIgnoredDuringExecution")
        self.spread = p["spec"].get("topologySpreadConstraints", [])


class _NodeRec:
    def __init__(self, n):
        self.name = name_of(n)
        self.labels = n["metadata"]["labels"]
        self.taints = n["spec"].get("taints", [])
        a = n["status"]["allocatable"]
        self.alloc = (milli(a["cpu"]), int(a["memory"]), int(a.get("ephemeral-storage", 0)))
        self.images = [(nm, im["sizeBytes"]) for im in n["status"].get("images", []) for nm in im["names"]]
        self.pods = []
        self.req, self.nz = [0, 0, 0], [0, 0]


class Model:
    """Cluster state in Python objects and the seven score plugins of a pod over a feasible node list: integers
    for the integer parts, Python floats (IEEE binary64, unfused) where the reference uses float64."""

    def __init__(self, cfg, nodes, bound, go_log, rules=None):
        self.rules = rules or Rules()
        self.go_log = go_log
        self.weights = dict(DEFAULT_WEIGHTS)
        for k, v in cfg.get("scoreWeights", {}).items():
            self.weights[PLUGIN_NAMES[k]] = int(v)
        ipa = cfg.get("interPodAffinity", {})
        self.hard, self.ignore = ipa.get("hardPodAffinityWeight", 1), ipa.get("ignorePreferredTermsOfExistingPods", False)
        self.added = cfg.get("nodeAffinity", {}).get("addedAffinity", {}).get("preferredDuringSchedulingIgnoredDuringExecution")
        ss = cfg.get("nodeResourcesFit", {}).get("scoringStrategy", {})
        self.rtcr = None
        if ss.get("type") == "RequestedToCapacityRatio":
            res = [(["cpu", "memory", "ephemeral-storage"].index(r["name"]), r["weight"]) for r in ss["resources"]]
            self.rtcr = (res, [(s["utilization"], s["score"] * 10) for s in ss["requestedToCapacityRatio"]["shape"]])
        self.nodes, self.image_states = {}, {}
        for n in nodes:
            self.add_node(n)
        for p in bound:
            self.add_pod(p["spec"]["nodeName"], p)

    # -- cache --
    def add_node(self, n):
        rec = _NodeRec(n)
        self.nodes[rec.name] = rec
        for nm, size in rec.images:  # the first node to register an image fixes its size (cache.go addNodeImageStates)
            st = self.image_states.setdefault(nm, [size, set()])
            st[1].add(rec.name)
        return rec

    def _drop_images(self, rec):
        for nm, _ in rec.images:
            st = self.image_states.get(nm)
            if st:
                st[1].discard(rec.name)
                if not st[1]:
                    del self.image_states[nm]

    def remove_node(self, name):
        self._drop_images(self.nodes.pop(name))

    def update_node(self, n):
        old = self.nodes[name_of(n)]
        self._drop_images(old)
        order = list(self.nodes)
        rec = self.add_node(n)
        rec.pods, rec.req, rec.nz = old.pods, old.req, old.nz
        self.nodes = {k: self.nodes[k] for k in order}

    def apply(self, step):
        getattr(self, step[0])(step[1])

    def add_pod(self, node_name, p):
        rec, n = _PodRec(p), self.nodes[node_name]
        n.pods.append(rec)
        for k, v in enumerate((rec.cpu, rec.mem, rec.eph)):
            n.req[k] += v
        n.nz[0] += rec.nz_cpu
        n.nz[1] += rec.nz_mem

    # -- plugins: each returns {node name: normalised score} or None (PreScore skips) --
    def taint(self, pod, feas):
        tols = [t for t in pod.tolerations if not t.get("effect") or t["effect"] == "PreferNoSchedule"]
        raw = [sum(1 for t in n.taints if t["effect"] == "PreferNoSchedule" and not any(_tolerates(x, t) for x in tols))
               for n in feas]
        return self.rules.default_normalize(raw, True)

    def node_affinity(self, pod, feas):
        if pod.preferred is None and not self.added:
            return None

        def score(terms, n):
            return sum(t["weight"] for t in terms or []
                       if all(_expr_matches(e, n.labels) for e in t["preference"]["matchExpressions"]))

        return self.rules.default_normalize([score(self.added, n) + score(pod.preferred, n) for n in feas], False)

    def fit(self, pod, feas):
        out = []
        for n in feas:
            requested = (n.nz[0] + pod.nz_cpu, n.nz[1] + pod.nz_mem, n.req[2] + pod.eph)
            if self.rtcr is None:  # LeastAllocated over cpu and memory
                num = ws = 0
                for k in range(2):
                    if n.alloc[k]:
                        num += 0 if requested[k] > n.alloc[k] else (n.alloc[k] - requested[k]) * 100 // n.alloc[k]
                        ws += 1
                out.append(num // ws if ws else 0)
                continue
            num, ws = self.rtcr_quotient(pod, n)
            out.append(self.rules.rtcr_round(float(num) / float(ws)) if ws else 0)
        return out

    def rtcr_quotient(self, pod, n):
        """(weighted sum, weight sum) of the RequestedToCapacityRatio score of pod on node n."""
        res, shape = self.rtcr
        requested = (n.nz[0] + pod.nz_cpu, n.nz[1] + pod.nz_mem, n.req[2] + pod.eph)
        num = ws = 0
        for k, w in res:
            if n.alloc[k]:
                s = self.rules.shape(shape, 100 if requested[k] > n.alloc[k] else requested[k] * 100 // n.alloc[k])
                if s > 0:
                    num, ws = num + s * w, ws + w
        return num, ws

    def balanced(self, pod, feas):
        if pod.cpu == 0 and pod.mem == 0:
            return None

        def bal(req, alloc):
            f = [min(float(req[k]) / float(alloc[k]), 1.0) for k in range(2) if alloc[k]]
            std = abs((f[0] - f[1]) / 2) if len(f) == 2 else 0.0
            return int((1 - std) * 100.0)

        return [50 + go_div(50 + bal((n.req[0] + pod.cpu, n.req[1] + pod.mem), n.alloc) - bal(n.req, n.alloc), 2) for n in feas]

    def image(self, pod, feas):
        total = len(self.nodes)
        out = []
        for n in feas:
            have = {nm for nm, _ in n.images}
            s = 0
            for img in pod.images:
                nm = normalized_image(img)
                if nm in have:
                    size, holders = self.image_states[nm]
                    s += self.rules.image_scaled(size, len(holders), total)
            out.append(self.rules.image_priority(s, len(pod.images)))
        return out

    def image_sum(self, pod, n):
        have = {nm for nm, _ in n.images}
        return sum(self.rules.image_scaled(self.image_states[nm][0], len(self.image_states[nm][1]), len(self.nodes))
                   for nm in map(normalized_image, pod.images) if nm in have)

    def pts_raw(self, pod, feas):
        """Raw PodTopologySpread scores of the feasible nodes (None: ignored), or None when PreScore skips."""
        cs = pod.spread
        if not cs or not feas:
            return None
        keys = [c["topologyKey"] for c in cs]
        live = [n for n in feas if all(k in n.labels for k in keys)]
        counts = [{} if k == HOSTNAME else {n.labels[k]: 0 for n in live} for k in keys]
        weight = [self.go_log(float((len(live) if k == HOSTNAME else len(counts[i])) + 2)) for i, k in enumerate(keys)]

        def matching(n, c):
            return sum(1 for e in n.pods if _sel_matches(c["labelSelector"]["matchLabels"], e.labels))

        for n in self.nodes.values():
            if not all(k in n.labels for k in keys):
                continue
            for i, c in enumerate(cs):
                if c.get("nodeAffinityPolicy", "Honor") == "Honor" and not _sel_matches(pod.node_selector, n.labels):
                    continue
                if keys[i] != HOSTNAME and n.labels[keys[i]] in counts[i]:
                    counts[i][n.labels[keys[i]]] += matching(n, c)
        out = []
        for n in feas:
            if n not in live:
                out.append(None)
                continue
            score = 0.0
            for i, c in enumerate(cs):
                cnt = matching(n, c) if keys[i] == HOSTNAME else counts[i][n.labels[keys[i]]]
                score += float(cnt) * weight[i] + float(c["maxSkew"] - 1)
            out.append(go_round(score))
        return out

    def pts(self, pod, feas):
        raw = self.pts_raw(pod, feas)
        return None if raw is None else self.rules.pts_normalize(raw)

    def ipa_raw(self, pod, feas):
        has = bool(pod.pref_aff or pod.pref_anti)
        if self.ignore and not has:
            return None
        topo, hit = {}, False
        for n in self.nodes.values():
            for e in n.pods if has else [e for e in n.pods if e.has_affinity]:
                pairs = [(t, w, e.labels) for w, t in pod.pref_aff] + [(t, -w, e.labels) for w, t in pod.pref_anti]
                if self.hard > 0:
                    pairs += [(t, self.hard, pod.labels) for t in e.req_aff]
                pairs += [(t, w, pod.labels) for w, t in e.pref_aff] + [(t, -w, pod.labels) for w, t in e.pref_anti]
                for (key, sel), w, target in pairs:
                    if _sel_matches(sel, target) and key in n.labels:
                        topo[(key, n.labels[key])] = topo.get((key, n.labels[key]), 0) + w
                        hit = True
        if not hit:
            return None
        return [sum(v for (key, val), v in topo.items() if n.labels.get(key) == val) for n in feas]

    def ipa(self, pod, feas):
        raw = self.ipa_raw(pod, feas)
        return None if raw is None else self.rules.ipa_normalize(raw)

    def scores(self, p, feasible_names):
        """{plugin: [weighted score per feasible node]} and the totals."""
        pod, feas = _PodRec(p), [self.nodes[nm] for nm in feasible_names]
        per = {}
        for pl, fn in ((P_TAINT, self.taint), (P_NA, self.node_affinity), (P_FIT, self.fit), (P_PTS, self.pts),
                       (P_IPA, self.ipa), (P_BAL, self.balanced), (P_IMG, self.image)):
            s = fn(pod, feas)
            per[pl] = [0] * len(feas) if s is None else [x * self.weights[pl] for x in s]
        return per, [sum(per[pl][i] for pl in per) for i in range(len(feas))]
