"""What ksg_preempt costs a spread-constrained preemptor with and without nominations that mark it (config
preemptNominatedPods "EvaluateAll"), in the shape of scripts/bench_preempt.py: N nodes of 4 CPUs in
three zones, 4 low-priority pods of 900m on each, one priority-10 preemptor of 3000m with a DoNotSchedule zone
constraint over its own label.  Nothing is actuated: the same PostFilter is timed `--calls` times after a warm-up.

  unmarked   nothing nominated: the one-pass instances (k_filter_score, k_preempt_seg<PreemptRegs>)
  marked     8 pods of the preemptor's label and priority nominated to 8 nodes: k_nom_topo, k_filter_score_nt and
             k_preempt_seg<PreemptRegs, true>

--config plain runs the unmarked case on a context created with {"nominatedPods": "EvaluateAll"} alone, which a
library without the new key takes too (KSG_LIB).  Prints one JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-kubernetes_amd"))

ZONE = "topology.kubernetes.io/zone"


def node(i):
    return {"apiVersion": "v1", "kind": "Node", "metadata": {"name": f"n{i:05d}", "labels": {ZONE: f"z{i % 3}"}},
            "spec": {}, "status": {"capacity": {"pods": "110", "cpu": "4", "memory": "32Gi"},
                                   "allocatable": {"pods": "110", "cpu": "4", "memory": "32Gi"}}}


def pod(name, prio, cpu, node_name=None, start=None, nominated=None, app="low"):
    p = {"apiVersion": "v1", "kind": "Pod",
         "metadata": {"name": name, "namespace": "default", "uid": name, "labels": {"app": app}},
         "spec": {"priority": prio, "containers": [{"name": "c", "image": "i", "resources": {
             "requests": {"cpu": cpu, "memory": "500Mi"}}}]}, "status": {}}
    if node_name:
        p["spec"]["nodeName"] = node_name
    if start is not None:
        p["status"]["startTime"] = f"2024-01-01T00:{start // 60 % 60:02d}:{start % 60:02d}Z"
    if nominated:
        p["status"]["nominatedNodeName"] = nominated
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--config", choices=["plain", "preempt"], default="preempt")
    a = ap.parse_args()
    from ksg.native import Scheduler
    cfg = {"nominatedPods": "EvaluateAll"}
    if a.config == "preempt":
        cfg["preemptNominatedPods"] = "EvaluateAll"
    g = Scheduler(cfg)
    g.upsert_namespace({"metadata": {"name": "default"}})
    for i in range(a.nodes):
        g.add_node(node(i))
    for i in range(a.nodes):
        for k in range(4):
            g.add_pod(pod(f"low-{i}-{k}", 0, "900m", f"n{i:05d}", start=(i * 4 + k) % 3600))
    pre = pod("pre", 10, "3000m", app="hi")
    pre["spec"]["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "DoNotSchedule",
                                                 "labelSelector": {"matchLabels": {"app": "hi"}}}]
    h = g.compile(pre)
    args = {"offset": 0, "now": 1704153600 * 10 ** 9}

    def measure(case):
        for q in range(20):
            g.preempt(h, dict(args, offset=q * 7919))
        ts = []
        for q in range(a.calls):
            t0 = time.perf_counter()
            r, _ = g.preempt(h, dict(args, offset=q * 7919))
            ts.append(time.perf_counter() - t0)
        assert r.status == 0
        print(json.dumps({"case": case, "config": cfg, "nodes": a.nodes, "calls": a.calls,
                          "postfilter_us_per_call_median": round(statistics.median(ts) * 1e6, 1),
                          "postfilter_us_per_call_mean": round(statistics.fmean(ts) * 1e6, 1),
                          "candidates": r.num_candidates, "potential": r.num_potential}), flush=True)

    measure("unmarked")
    if a.config == "preempt":
        for k in range(8):
            g.add_nominated_pod(pod(f"nom{k}", 10, "500m", nominated=f"n{k * (a.nodes // 8):05d}", app="hi"))
        measure("marked, 8 nominations")


if __name__ == "__main__":
    main()
