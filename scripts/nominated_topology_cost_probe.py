"""scripts/nominated_topology_cost_probe.py -- what a marked pod costs (config nominatedPods "EvaluateAll", DESIGN.md
§4.10): one 1000-pod batch on 5000 nodes, wall time of ksg_schedule_batch per pod (handles compiled before), for
  spread_no_nominations     TopologySpreading's pods (zone spread, DoNotSchedule), nothing nominated: k_agg_loop
  plain_8_nominations       SchedulingBasic's pods under 8 nominations: "Evaluate"'s class, k_sched_loop
  spread_8_nominations      the spread pods under the same 8 nominations: marked, the per-pod launches + k_nom_topo
Information, not a gate."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the repository
sys.path.insert(0, os.path.join(ROOT, "kubernetes-kubernetes_amd"))
from ksg.native import Scheduler  # noqa: E402
from ksg.synth import pod_default, topology_spreading  # noqa: E402

nodes, init, spread_pods = topology_spreading(5000, 1000, 4000)
plain_pods = [pod_default(f"plain-{k}", ns="sched-1") for k in range(4000)]
out = {}
for tag, nnom, pods in (("spread_no_nominations", 0, spread_pods), ("plain_8_nominations", 8, plain_pods),
                        ("spread_8_nominations", 8, spread_pods)):
    g = Scheduler({"nominatedPods": "EvaluateAll"})
    for ns in ("sched-0", "sched-1"):
        g.upsert_namespace({"metadata": {"name": ns}})
    for n in nodes:
        g.add_node(n)
    for p in init:
        g.add_pod(p)
    names = g.node_names()
    for k in range(nnom):
        g.add_nominated_pod({"metadata": {"name": f"nom{k}", "namespace": "sched-1", "uid": f"nom{k}",
                                          "labels": {"color": "blue"}},
                             "spec": {"priority": 0, "containers": [{"name": "c", "image": "i", "resources": {
                                 "requests": {"cpu": "500m", "memory": "1Gi"}}}]},
                             "status": {"nominatedNodeName": names[k * 600 + 5]}})
    runs = []
    for rep in range(4):  # 1000 pods per batch; the first is warm-up
        hs = [g.compile(p) for p in pods[rep * 1000:(rep + 1) * 1000]]
        t0 = time.perf_counter()
        rs = g.schedule_batch(hs, assume=True)
        dt = time.perf_counter() - t0
        assert all(r.status == 0 for r in rs)
        runs.append((round(dt * 1e6 / len(hs), 2), g.kernel_stats()[3]))
    out[tag] = {"wall_us_per_pod": [r[0] for r in runs[1:]], "kernel": runs[-1][1]}
    g.close()
print(json.dumps(out))
