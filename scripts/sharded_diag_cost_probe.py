"""scripts/sharded_diag_cost_probe.py -- what the FitError diagnosis costs on a node-sharded context (information, not
a gate; DESIGN.md §6 "Diagnosis when sharded").  An in-process group of W = 2 ranks with the device exchange, 5000
nodes per rank, 1000-pod batches: wall microseconds per pod (the slower rank's) of ksg_schedule_batch, of
ksg_schedule_batch_diag with no failing pod and with 10 failing pods per batch, for SchedulingBasic (k_sched_loop) and
TopologySpreading (k_agg_loop).  Both ranks share one GPU, so this shows the mechanism's cost on the device and the
host, not a multi-GPU figure: the cross-GPU sum over xGMI is not in it.

    python scripts/sharded_diag_cost_probe.py [plain]      # "plain": ksg_schedule_batch only (a library without the opt-in)
Prints one JSON line."""
import copy
import gc
import json
import os
import sys
import threading
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the repository
sys.path.insert(0, os.path.join(ROOT, "kubernetes-kubernetes_amd"))
from ksg.native import Scheduler  # noqa: E402
from ksg.synth import scheduling_basic, topology_spreading  # noqa: E402

W, PER_RANK, BATCH, REPS, WARM = 2, 5000, 1000, 6, 2


def too_big(p):
    p = copy.deepcopy(p)
    p["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "64"
    return p


def no_zone(p):
    p = copy.deepcopy(p)
    p["spec"]["topologySpreadConstraints"][0].update(topologyKey="no-such-key")
    return p


def group(nodes, init, nss, diagnosis):
    name = f"cost-{uuid.uuid4().hex[:6]}"
    ranks = []
    for r in range(W):
        dist = {"worldSize": W, "rank": r, "localGroup": name}
        if diagnosis:
            dist["diagnosis"] = True
        s = Scheduler({"device": 0, "deviceExchange": True, "featureGates": {"OpportunisticBatching": False},
                       "distributed": dist})
        for ns in nss:
            s.upsert_namespace({"metadata": {"name": ns}})
        for n in nodes:
            s.add_node(n)
        for p in init:
            s.add_pod(p)
        ranks.append(s)
    return ranks


def measure(nodes, init, nss, pods, nfail, spoil, diag):
    batches = []
    for rep in range(REPS):
        b = pods[rep * BATCH:(rep + 1) * BATCH]
        if nfail:
            step = BATCH // nfail
            b = [spoil(p) if k % step == step // 2 else p for k, p in enumerate(b)]
        batches.append(b)
    ranks = group(nodes, init, nss, diag)
    hs = [[[s.compile(p) for p in b] for b in batches] for s in ranks]
    us = [[0.0] * REPS for _ in ranks]
    kus = [[0.0] * REPS for _ in ranks]  # the dominant loop's own time per pod (HIP events on its dispatches)
    failed = [0] * W
    errs = []
    gate = threading.Barrier(W)

    def work(r):
        try:
            for k in range(REPS):
                gate.wait(timeout=120)
                t0 = time.perf_counter()
                if diag:
                    rs, ds = ranks[r].schedule_batch_diag(hs[r][k], assume=True)
                    assert all((d.failed_nodes == len(nodes)) == (x.status == 2) for x, d in zip(rs, ds))
                else:
                    rs = ranks[r].schedule_batch(hs[r][k], assume=True)
                us[r][k] = (time.perf_counter() - t0) * 1e6 / BATCH
                kus[r][k] = ranks[r].kernel_stats()[0] * 1e3
                failed[r] = sum(x.status == 2 for x in rs)
        except Exception as e:  # reported below
            errs.append((r, repr(e)))
            gate.abort()

    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(W)]
    gc.collect()
    gc.disable()  # (a collection of the streams' many dicts inside a timed batch costs milliseconds)
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    gc.enable()
    if errs or any(t.is_alive() for t in ts):
        raise SystemExit(f"sharded_diag_cost_probe: {errs or 'a rank did not return'}")
    out = {"us_per_pod": [round(max(us[r][k] for r in range(W)), 3) for k in range(WARM, REPS)],
           "kernel_us_per_pod": [round(max(kus[r][k] for r in range(W)), 3) for k in range(WARM, REPS)],
           "failed_per_batch": failed[0], "kernel": ranks[0].kernel_stats()[3],
           "loop_stats": [s.loop_stats() for s in ranks]}
    for s in ranks:
        s.close()
    return out


plain_only = len(sys.argv) > 1 and sys.argv[1] == "plain"
out = {}
for wl, gen, nss, spoil in (("basic", scheduling_basic, ["default"], too_big),
                            ("spreading", topology_spreading, ["sched-0", "sched-1"], no_zone)):
    nodes, init, pods = gen(W * PER_RANK, 1000, BATCH * REPS)
    out[f"{wl}_plain"] = measure(nodes, init, nss, pods, 0, spoil, False)
    if not plain_only:
        out[f"{wl}_diag_0_failing"] = measure(nodes, init, nss, pods, 0, spoil, True)
        out[f"{wl}_diag_10_failing"] = measure(nodes, init, nss, pods, 10, spoil, True)
print(json.dumps(out))
