"""scripts/sharded_nominations_cost_probe.py -- what nominated pods cost on a node-sharded context (information, not a
gate; DESIGN.md §6 "Nominated pods when sharded").  An in-process group of W = 2 ranks with the device exchange, 5000
nodes per rank, 1000-pod batches of SchedulingBasic (k_sched_loop) and TopologySpreading (k_agg_loop): the dominant
loop's own time per pod and the wall microseconds per pod (the slower rank's) of ksg_schedule_batch
  * without the opt-in ("plain": also what a library from before the opt-in runs, KSG_LIB),
  * with "nominations": true and nothing nominated,
  * with nominatedPods "Evaluate" and 8 priority-0 nominations outstanding (pods outside the stream; SchedulingBasic
    only),
  * with one pod of every batch carrying status.nominatedNodeName (a run of its own over the all-reduce path; the
    plain pods around it stay in the loop).
Each k_sched_loop row records the group kernel its last launch dispatched, by the runtime's name of it
(ksg_debug_group_loop_kernel), and the probe asserts that with nothing nominated that is the plain row's kernel, and
k_sched_loop_group_nom under nominations.
Both ranks share one GPU, so this shows the mechanism's cost on the device and the host, not a multi-GPU figure.

    python scripts/sharded_nominations_cost_probe.py [plain]   # "plain": the first row only
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
from ksg.native import Scheduler, group_loop_kernel  # noqa: E402
from ksg.synth import scheduling_basic, topology_spreading  # noqa: E402

W, PER_RANK, BATCH, REPS, WARM = 2, 5000, 1000, 6, 2


def group(nodes, init, nss, optin, evaluate):
    name = f"cost-{uuid.uuid4().hex[:6]}"
    ranks = []
    for r in range(W):
        dist = {"worldSize": W, "rank": r, "localGroup": name}
        if optin:
            dist["nominations"] = True
        cfg = {"device": 0, "deviceExchange": True, "featureGates": {"OpportunisticBatching": False}, "distributed": dist}
        if evaluate:
            cfg["nominatedPods"] = "Evaluate"
        s = Scheduler(cfg)
        for ns in nss:
            s.upsert_namespace({"metadata": {"name": ns}})
        for n in nodes:
            s.add_node(n)
        for p in init:
            s.add_pod(p)
        ranks.append(s)
    return ranks


def nominee(k, node, ns):
    return {"metadata": {"name": f"held{k}", "namespace": ns, "uid": f"held{k}"},
            "spec": {"priority": 0, "containers": [{"name": "c", "image": "i",
                                                    "resources": {"requests": {"cpu": "100m", "memory": "64Mi"}}}]},
            "status": {"nominatedNodeName": node}}


def measure(nodes, init, nss, pods, optin=False, held=0, own=False):
    batches = [pods[rep * BATCH:(rep + 1) * BATCH] for rep in range(REPS)]
    ranks = group(nodes, init, nss, optin, held > 0)
    names = ranks[0].node_names()
    if own:  # the pod in the middle of every batch: nominated to a node of rank 1's range, rank 0's the next time
        for rep, b in enumerate(batches):
            p = copy.deepcopy(b[BATCH // 2])
            p["status"] = dict(p.get("status") or {}, nominatedNodeName=names[(PER_RANK + 17 * rep) % len(names) if rep % 2 else 17 * rep])
            batches[rep] = b[:BATCH // 2] + [p] + b[BATCH // 2 + 1:]
    for s in ranks:
        for k in range(held):
            s.add_nominated_pod(nominee(k, names[k * (len(names) // held) + 3], nss[0]))
    hs = [[[s.compile(p) for p in b] for b in batches] for s in ranks]
    us = [[0.0] * REPS for _ in ranks]
    kus = [[0.0] * REPS for _ in ranks]  # the dominant loop's own time per pod (HIP events on its dispatches)
    errs = []
    gate = threading.Barrier(W)

    def work(r):
        try:
            for k in range(REPS):
                gate.wait(timeout=120)
                t0 = time.perf_counter()
                rs = ranks[r].schedule_batch(hs[r][k], assume=True)
                us[r][k] = (time.perf_counter() - t0) * 1e6 / BATCH
                kus[r][k] = ranks[r].kernel_stats()[0] * 1e3
                assert all(x.status == 0 for x in rs)
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
        raise SystemExit(f"sharded_nominations_cost_probe: {errs or 'a rank did not return'}")
    out = {"us_per_pod": [round(max(us[r][k] for r in range(W)), 3) for k in range(WARM, REPS)],
           "kernel_us_per_pod": [round(max(kus[r][k] for r in range(W)), 3) for k in range(WARM, REPS)],
           "kernel": ranks[0].kernel_stats()[3], "loop_stats": [s.loop_stats() for s in ranks]}
    if out["kernel"] == "k_sched_loop":  # the instance the group's last launch dispatched, by the runtime's name of it
        out["dispatched"] = group_loop_kernel()  # (None: a library from before ksg_debug_group_loop_kernel)
    for s in ranks:
        s.close()
    return out


plain_only = len(sys.argv) > 1 and sys.argv[1] == "plain"
out = {}
for wl, gen, nss in (("basic", scheduling_basic, ["default"]), ("spreading", topology_spreading, ["sched-0", "sched-1"])):
    nodes, init, pods = gen(W * PER_RANK, 1000, BATCH * REPS)
    out[f"{wl}_plain"] = measure(nodes, init, nss, pods)
    if not plain_only:
        out[f"{wl}_optin_nothing_nominated"] = measure(nodes, init, nss, pods, optin=True)
        if wl == "basic":  # (TopologySpreading's pods have a DoNotSchedule constraint: "Evaluate" refuses that pair)
            out[f"{wl}_8_nominations_outstanding"] = measure(nodes, init, nss, pods, optin=True, held=8)
            # with nothing nominated the group kernel dispatched is the plain batch's; under nominations the overlay's
            plain, on, held = (out[f"{wl}_{k}"]["dispatched"] for k in ("plain", "optin_nothing_nominated",
                                                                         "8_nominations_outstanding"))
            assert "k_sched_loop_group" in plain and "_nom" not in plain and on == plain, (plain, on)
            assert "k_sched_loop_group_nom" in held, held
        out[f"{wl}_own_nominated_pod_per_batch"] = measure(nodes, init, nss, pods, optin=True, own=True)
print(json.dumps(out))
