"""Seeded clusters and pod streams of edge quantities for the default-plugin score path.

fuzz_gen and ksg.synth draw 2-16 cores, 4-32 Gi and requests from a short list of round values: no node has
a zero allocatable, nothing comes near 2^45, and an unstructured (requested, allocatable) pair almost never
sits where a truncation flips on one ulp.  The families here do:

  degenerate  allocatable cpu 0 / 1m, memory 0 / 1 byte, pods 0 / 1 / 3 among ordinary nodes; bound pods
              that request more than their node's allocatable; incoming pods with no requests at all (the
              non-zero defaults 100m / 209715200 bytes score Fit, BalancedAllocation is skipped), with
              explicit 0 requests, with cpu only, memory only, 1m, prime byte counts, ephemeral-storage
  boundary    exact quotients that are integers or one short of one: cpu allocatable at multiples of 50m
              and 100m, memory allocatable at powers of two, bound requests summing to exactly k % (cpu)
              and j eighths (memory) of the allocatable, the same sums +-1 unit, and incoming requests that
              keep the sums on that grid
  magnitude   memory (and some cpu) allocatable up to BOUND - 1 with requests of 2^39 and more, so that
              (allocatable - requested) * 100 approaches 2^52
  over        magnitude with three nodes at BOUND, BOUND + 12345 and 2^55 + 3: the context leaves the
              straight-line evaluation for the generic one

Every stream is 200 hostname-labelled nodes (two 128-node units, the last one partial), about 200 bound pods
and 130 incoming pods, as plain JSON objects.  Pod-count capacities are small on many nodes so that a
MostAllocated profile, which keeps choosing the fullest node, has to move on.
"""
import random

BOUND = (1 << 52) // 100  # the host leaves DF_FAST / DF_LFAST once any cpu / memory allocatable reaches it
DEFAULT_CPU, DEFAULT_MEM = 100, 200 * 1024 * 1024  # GetNonzeroRequests' defaults (milli-cpu, bytes)
N_NODES, N_PODS = 200, 130
FAMILIES = ["degenerate", "boundary", "magnitude", "over"]
PRIMES = [1, 2, 3, 7, 1009, 65537, 1048573, 16777259, 268435459, 1073741827]


def node(i, cpu_milli, mem, pods, eph=None):
    name = f"edge-{i:04d}"
    alloc = {"cpu": f"{cpu_milli}m", "memory": str(mem), "pods": str(pods)}
    if eph is not None:
        alloc["ephemeral-storage"] = str(eph)
    return {"apiVersion": "v1", "kind": "Node",
            "metadata": {"name": name, "labels": {"kubernetes.io/hostname": name}},
            "spec": {}, "status": {"allocatable": alloc, "capacity": alloc}}


def pod(name, requests, node_name=None):
    """requests None: a container without a resources.requests map at all."""
    c = {"name": "c", "image": "edge.example/none:1"}
    if requests is not None:
        c["resources"] = {"requests": dict(requests)}
    p = {"apiVersion": "v1", "kind": "Pod",
         "metadata": {"name": name, "namespace": "default", "uid": name, "labels": {"app": "edge"}},
         "spec": {"containers": [c]}, "status": {}}
    if node_name:
        p["spec"]["nodeName"] = node_name
    return p


def _req(cpu=None, mem=None, eph=None):
    r = {}
    if cpu is not None:
        r["cpu"] = f"{cpu}m"
    if mem is not None:
        r["memory"] = str(mem)
    if eph is not None:
        r["ephemeral-storage"] = str(eph)
    return r


def _pods_cap(rng):
    return rng.choice([3, 4, 6, 6, 110])


# ---- degenerate -------------------------------------------------------------------------------------------
def _degenerate(rng):
    nodes, bound = [], []
    for i in range(N_NODES):
        k = i % 8
        cpu = rng.choice([300, 450, 700, 999, 1001, 1500, 2300, 2500])
        mem = rng.choice([1 << 28, (1 << 29) + 1, 805306357, (1 << 30) - 1, 3 << 29, 2147483659, 1 << 32])
        pods = _pods_cap(rng)
        eph = rng.choice([None, 10 ** 9, 1 << 31])
        if k == 1:
            cpu = rng.choice([0, 1])
        elif k == 3:
            mem = rng.choice([0, 1])
        elif k == 5:
            pods = rng.choice([0, 1, 3])
        elif k == 7 and i % 16 == 7:
            cpu, mem = rng.choice([0, 1]), rng.choice([0, 1])
        nodes.append(node(i, cpu, mem, pods, eph))
    for k in range(N_NODES):
        i = rng.randrange(N_NODES)
        n = nodes[i]["status"]["allocatable"]
        acpu, amem = int(n["cpu"][:-1]), int(n["memory"])
        r = rng.random()
        if r < 0.2:  # more than the node has: add_pod takes it, requested > allocatable
            q = _req(acpu + rng.choice([1, 50, 4000]), amem + rng.choice([1, 1 << 20, 1 << 33]))
        elif r < 0.3:
            q = None
        elif r < 0.4:
            q = _req(0, 0)
        else:
            q = _req(rng.choice([1, 50, 99, 100, 250]), rng.choice(PRIMES + [1 << 26, 1 << 27]))
        bound.append(pod(f"bound-{k}", q, nodes[i]["metadata"]["name"]))
    incoming = []
    for k in range(N_PODS):
        kind = k % 10
        if kind == 0:
            q = None
        elif kind == 1:
            q = _req(0, 0)
        elif kind == 2:
            q = _req(cpu=rng.choice([1, 50, 101, 250]))
        elif kind == 3:
            q = _req(mem=rng.choice(PRIMES))
        elif kind == 4:
            q = _req(1, rng.choice(PRIMES))
        elif kind == 5:
            q = _req(rng.choice([10, 100]), rng.choice([1 << 20, 1 << 26]), eph=rng.choice([1, 10 ** 8, 1 << 30]))
        elif kind == 6:
            q = {}
        elif kind == 7:
            q = _req(cpu=0, mem=rng.choice([1, 1 << 27]))
        elif kind == 8:
            q = _req(cpu=rng.choice([1, 299]), mem=0)
        else:
            q = _req(rng.choice([99, 100, 101, 333]), rng.choice([DEFAULT_MEM - 1, DEFAULT_MEM, DEFAULT_MEM + 1]))
        incoming.append(pod(f"in-{k}", q))
    return nodes, bound, incoming


# ---- boundary ---------------------------------------------------------------------------------------------
# BalancedAllocation truncates (1 - |f_cpu - f_mem| / 2) * 100, whose exact value is an integer where
# |f_cpu - f_mem| is a multiple of 1/50: there the binary64 result sits within an ulp of the integer and any
# other rounding of the chain flips the truncation.  The node classes are s * (4000m, 2^32 bytes); a node whose
# cpu stands at a / 200 and whose memory at j / 8 of the allocatable is on that grid when a - 25 j is a multiple
# of 4, and a pod of x * 20m and y * 2^29 bytes keeps it there on every class when x - 25 y is a multiple of 16.
B_SCALES = [(1, 2), (1, 1), (1, 1), (2, 1), (2, 1), (4, 1)]  # s as (numerator, denominator)
B_ODD = [(1050, 1 << 30), (2500, 1 << 31), (6400, 1 << 33), (1600, 1 << 30), (3200, 1 << 34)]  # off the grid
B_PODS = [(9, 1), (25, 1), (2, 2), (18, 2), (11, 3), (41, 1), (16, 0), (34, 2)]


def _boundary(rng):
    nodes, bound = [], []
    for i in range(N_NODES):
        if i % 20 == 19:
            cpu, mem = rng.choice(B_ODD)
        else:
            num, den = rng.choice(B_SCALES)
            cpu, mem = 4000 * num // den, (1 << 32) * num // den
        nodes.append(node(i, cpu, mem, _pods_cap(rng)))
    # One bound pod per node: cpu at exactly a / 200, memory at j eighths.  On two nodes in five the memory is
    # one byte off: the exact score is then 1e-9 to either side of an integer, which binary64 resolves and a
    # narrower format does not.  One node in ten has its cpu 1m off (a hundredth of a point: off the grid).
    for i in range(N_NODES):
        n = nodes[i]["status"]["allocatable"]
        acpu, amem = int(n["cpu"][:-1]), int(n["memory"])
        j = rng.randrange(0, 6)
        a = (rng.randrange(25, 44) if rng.random() < 0.6 else rng.randrange(0, 25)) * 4 + 25 * j % 4
        cpu = acpu * a // 200 + (rng.choice([1, -1]) if i % 10 == 3 else 0)
        mem = amem * j // 8 + (rng.choice([1, -1]) if i % 5 in (1, 2) else 0)
        bound.append(pod(f"bound-{i}", _req(max(cpu, 0), max(mem, 0)), nodes[i]["metadata"]["name"]))
    incoming = []
    for k in range(N_PODS):
        x, y = rng.choice(B_PODS)
        cpu, mem = 20 * x, (1 << 29) * y
        r = rng.random()
        if r < 0.03:
            q = _req(cpu=cpu + 1)
        elif r < 0.06:
            q = _req(mem=mem + 1)
        elif r < 0.12:
            q = _req(cpu + rng.choice([1, -1]), mem + rng.choice([0, 1, -1]) if mem else mem)
        else:
            q = _req(cpu, mem)
        incoming.append(pod(f"in-{k}", q))
    return nodes, bound, incoming


# ---- magnitude / over -------------------------------------------------------------------------------------
M_MEM = [BOUND - 1, BOUND - 2, BOUND - 1, 1 << 45, (1 << 45) - 1, (1 << 44) + 12347, 3 << 43, (1 << 45) + (1 << 39),
         1 << 42, (1 << 43) - 1]
OVER_MEM = [BOUND, BOUND + 12345, (1 << 55) + 3]
OVER_AT = [5, 77, 190]  # node indices of the over variant's three large nodes (both units)


def _magnitude(rng, over):
    nodes, bound = [], []
    # Nodes come in twins (2k, 2k + 1): the same allocatable and the same fill but for one byte, so the fuller
    # one's score has a neighbour within a point; most twins have room for one more pod only, so that a
    # MostAllocated profile moves from node to node.
    for i in range(0, N_NODES, 2):
        mem = rng.choice(M_MEM) if rng.random() < 0.7 else rng.randrange(1 << 41, BOUND)
        cpu = rng.choice([4000, 16000, 64000, 96000])
        if i // 2 % 9 == 4:  # cpu at the bound too (milli-cpu)
            cpu = rng.choice([BOUND - 1, (1 << 45) + 1, (1 << 44) - 1])
        pods = rng.choice([2, 2, 2, 3, 6, 8])
        fill_cpu = cpu * rng.choice([10, 20, 30, 40, 50]) // 100
        fill_mem = mem * rng.choice([10, 20, 30, 40, 50]) // 100 + rng.choice([0, 1, 12345])
        for t in range(2):
            m = OVER_MEM[OVER_AT.index(i + t)] if over and i + t in OVER_AT else mem
            nodes.append(node(i + t, cpu, m, pods))
            bound.append(pod(f"bound-{i + t}", _req(fill_cpu, fill_mem + t), nodes[i + t]["metadata"]["name"]))
    incoming = []
    for k in range(N_PODS):
        mem = rng.choice([1 << 39, (1 << 39) + 1, 1 << 40, (1 << 40) - 1, 3 << 39, 1 << 41, (1 << 42) + 7])
        cpu = rng.choice([100, 250, 1000, 1999])
        r = rng.random()
        if r < 0.1:
            q = _req(cpu=cpu)  # memory by the 200 MiB default: (allocatable - requested) * 100 at its largest
        elif r < 0.2:
            q = _req(rng.choice([1 << 39, (1 << 40) + 1]), mem)  # fits the large-cpu nodes only
        elif r < 0.25:
            q = None
        else:
            q = _req(cpu, mem)
        incoming.append(pod(f"in-{k}", q))
    return nodes, bound, incoming


def stream(family, seed=0):
    """-> (nodes, bound pods, incoming pods) of one family, deterministic in (family, seed)."""
    rng = random.Random(f"edge-{family}-{seed}")
    if family == "degenerate":
        return _degenerate(rng)
    if family == "boundary":
        return _boundary(rng)
    if family in ("magnitude", "over"):
        return _magnitude(rng, family == "over")
    raise ValueError(family)


CONFIGS = {
    "least": {},
    "most": {"nodeResourcesFit": {"scoringStrategy": {"type": "MostAllocated"}}},
    "weights": {"scoreWeights": {"NodeResourcesFit": "3", "NodeResourcesBalancedAllocation": "2"}},
}


def load(b, nodes, bound):
    """A backend (product or oracle) with the stream's namespace, nodes and bound pods."""
    b.upsert_namespace({"metadata": {"name": "default"}})
    for n in nodes:
        b.add_node(n)
    for p in bound:
        b.add_pod(p)
    return b


def with_hostname_spread(p):
    """The same pod with one ScheduleAnyway hostname spread constraint: a PodTopologySpread score pod, which
    k_agg_loop takes (its node-local plugins by the straight-line evaluation, DF_LFAST)."""
    q = dict(p, spec=dict(p["spec"]))
    q["spec"]["topologySpreadConstraints"] = [{
        "maxSkew": 1, "topologyKey": "kubernetes.io/hostname", "whenUnsatisfiable": "ScheduleAnyway",
        "labelSelector": {"matchLabels": {"app": "edge"}}}]
    return q


# ---- the plain restatement ----------------------------------------------------------------------------------
def milli(q):
    return int(q[:-1]) if q.endswith("m") else int(q) * 1000


def pod_requests(p):
    """(cpu, memory) actual requests and (cpu, memory) non-zero requests of a one-container pod."""
    r = p["spec"]["containers"][0].get("resources", {}).get("requests", {})
    cpu = milli(r["cpu"]) if "cpu" in r else 0
    mem = int(r["memory"]) if "memory" in r else 0
    return (cpu, mem), (cpu if "cpu" in r else DEFAULT_CPU, mem if "memory" in r else DEFAULT_MEM)


class Restated:
    """Node state (allocatable, Requested, NonZeroRequested) tracked in Python integers, and the
    NodeResourcesFit / NodeResourcesBalancedAllocation scores of a pod on a node: integers for the integer
    parts, Python floats (IEEE binary64, unfused) for BalancedAllocation."""

    def __init__(self, nodes, bound):
        self.index = {n["metadata"]["name"]: i for i, n in enumerate(nodes)}
        self.alloc = [(milli(n["status"]["allocatable"]["cpu"]), int(n["status"]["allocatable"]["memory"])) for n in nodes]
        self.req = [[0, 0] for _ in nodes]
        self.nz = [[0, 0] for _ in nodes]
        for p in bound:
            self.add(self.index[p["spec"]["nodeName"]], p)

    def add(self, i, p):
        act, nz = pod_requests(p)
        for k in range(2):
            self.req[i][k] += act[k]
            self.nz[i][k] += nz[k]

    def fit(self, i, p, most):
        _, nz = pod_requests(p)
        num = ws = 0
        for k in range(2):
            alloc, req = self.alloc[i][k], self.nz[i][k] + nz[k]
            if alloc == 0:
                continue
            if most:
                s = min(req, alloc) * 100 // alloc
            else:
                s = 0 if req > alloc else (alloc - req) * 100 // alloc
            num += s
            ws += 1
        return num // ws if ws else 0

    def balanced_inputs(self, i, p):
        act, _ = pod_requests(p)
        (ac, am), (rc, rm) = self.alloc[i], self.req[i]
        return (rc, rm), (rc + act[0], rm + act[1]), (ac, am)

    def balanced(self, i, p, bal=None):
        act, _ = pod_requests(p)
        if act == (0, 0):
            return 0  # PreScore skips a pod that requests neither cpu nor memory
        without, with_, alloc = self.balanced_inputs(i, p)
        bal = bal or bal_f64
        return 50 + (50 + bal(with_, alloc) - bal(without, alloc)) // 2


def _bal(req, alloc, frac):
    f = [min(frac(req[k], alloc[k]), 1.0) if alloc[k] != 0 else 0.0 for k in range(2)]
    std = abs(f[0] - f[1]) / 2 if alloc[0] != 0 and alloc[1] != 0 else 0.0
    return std


def bal_f64(req, alloc):
    return int((1 - _bal(req, alloc, lambda a, b: a / b)) * 100)


def bal_mul_rcp(req, alloc):
    """mutant: a * (1 / b) in place of a / b"""
    return int((1 - _bal(req, alloc, lambda a, b: a * (1 / b))) * 100)


def bal_f32(req, alloc):
    """mutant: the whole chain in binary32"""
    import numpy as np
    f32 = np.float32
    f = [min(f32(req[k]) / f32(alloc[k]), f32(1)) if alloc[k] != 0 else f32(0) for k in range(2)]
    std = abs(f[0] - f[1]) / f32(2) if alloc[0] != 0 and alloc[1] != 0 else f32(0)
    return int((f32(1) - std) * f32(100))
