"""scripts/nominated_cost_probe.py -- one SchedulingBasic-shaped batch on 5000 nodes, with and without 8 outstanding priority-0 nominations:
k_sched_loop's time per pod from ksg_last_batch_kernel_stats (information, not a gate)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the repository
sys.path.insert(0, os.path.join(ROOT, "kubernetes-kubernetes_amd"))
from ksg.native import Scheduler  # noqa: E402
from ksg.synth import scheduling_basic  # noqa: E402

nodes, init, pods = scheduling_basic(5000, 1000, 7000)
out = {}
for tag, nnom, cfg in (("refuse_config_no_nominations", 0, {}), ("evaluate_no_nominations", 0, {"nominatedPods": "Evaluate"}),
                       ("evaluate_8_nominations", 8, {"nominatedPods": "Evaluate"})):
    g = Scheduler(cfg)
    g.upsert_namespace({"metadata": {"name": "default"}})
    for n in nodes:
        g.add_node(n)
    for p in init:
        g.add_pod(p)
    names = g.node_names()
    for k in range(nnom):
        g.add_nominated_pod({"metadata": {"name": f"nom{k}", "namespace": "default", "uid": f"nom{k}"},
                             "spec": {"priority": 0, "containers": [{"name": "c", "image": "i", "resources": {
                                 "requests": {"cpu": "500m", "memory": "1Gi"}}}]},
                             "status": {"nominatedNodeName": names[k * 600 + 5]}})
    runs = []
    for rep in range(7):  # 1000 pods per batch; the first two are warm-up
        hs = [g.compile(p) for p in pods[rep * 1000:(rep + 1) * 1000]]
        rs = g.schedule_batch(hs, assume=True)
        ms, _, n, kern = g.kernel_stats()
        assert all(r.status == 0 for r in rs)
        runs.append((round(ms * 1000, 3), n, kern))
    out[tag] = {"us_per_pod": [r[0] for r in runs[2:]], "pods_in_loop": runs[-1][1], "kernel": runs[-1][2]}
    g.close()
print(json.dumps(out))
