"""scripts/diag_cost_probe.py -- what a FitError diagnosis costs (information, not a gate).
One 1000-pod SchedulingBasic batch on 5000 nodes with 0 / 10 / 500 unschedulable pods (pods asking for more cpu than
any node has, spread evenly over the batch), and one k_agg_loop-class stream (TopologySpreading, 10 of 1000 pods
with a zone spread no zone satisfies): wall microseconds per pod of ksg_schedule_batch against
ksg_schedule_batch_diag, and against the only alternative without it -- ksg_schedule_batch, then one
ksg_schedule_one with full evaluation output per failed pod (which sees the end-of-batch state, not the pod's own
cycle).  Prints one JSON line.

--config '<json>' is merged into every context's config (as bench.py's --extra-config), e.g.
'{"percentageOfNodesToScore": 0}' or '{"loopSameDiag": false, "aggLoopSampledDiag": false}'; KSG_LIB names another
build of the library.  Besides the wall times, each mode reports the kernel of its last batch (kernel_stats) and
the pods k_sched_same took and left (same_pods), where the library has the call."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the repository
sys.path.insert(0, os.path.join(ROOT, "kubernetes-kubernetes_amd"))
from ksg.abi import Result  # noqa: E402
from ksg.native import Scheduler  # noqa: E402
from ksg.synth import scheduling_basic, topology_spreading  # noqa: E402

BATCH, REPS, WARM = 1000, 6, 2

ap = argparse.ArgumentParser()
ap.add_argument("--config", default=None, help="JSON object merged into the context's config")
ap.add_argument("--modes", default="plain,diag,plain+eval", help="the calls to time (comma-separated)")
ARGS = ap.parse_args()
CFG = json.loads(ARGS.config or "{}")
MODES = tuple(ARGS.modes.split(","))


def too_big(p):
    p = copy.deepcopy(p)
    p["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "64"
    return p


def no_zone(p):
    p = copy.deepcopy(p)
    p["spec"]["topologySpreadConstraints"][0].update(topologyKey="no-such-key")
    return p


def context(nodes, init, nss):
    g = Scheduler(dict(CFG))
    for ns in nss:
        g.upsert_namespace({"metadata": {"name": ns}})
    for n in nodes:
        g.add_node(n)
    for p in init:
        g.add_pod(p)
    return g


def stream(pods, nfail, spoil):
    """REPS batches of BATCH pods, nfail of each spoiled (every BATCH // nfail-th)."""
    out = []
    for rep in range(REPS):
        b = pods[rep * BATCH:(rep + 1) * BATCH]
        if nfail:
            step = BATCH // nfail
            b = [spoil(p) if k % step == step // 2 else p for k, p in enumerate(b)]
        out.append(b)
    return out


def measure(nodes, init, nss, batches, mode):
    g = context(nodes, init, nss)
    us, failed, kern, same = [], 0, None, None
    ev, r1 = g._eval_alloc(), Result()  # the full ksg_eval_out, allocated once (no per-call Python lists)
    for b in batches:
        hs = [g.compile(p) for p in b]
        t0 = time.perf_counter()
        if mode == "diag":
            rs, ds = g.schedule_batch_diag(hs, assume=True)
            assert all((d.failed_nodes == len(nodes)) == (r.status == 2) for r, d in zip(rs, ds))
            kern = g.kernel_stats()[3]
        else:
            rs = g.schedule_batch(hs, assume=True)
            kern = g.kernel_stats()[3]
            if mode == "plain+eval":  # today's only source of a diagnosis: a second, evaluated cycle per failed pod
                for h, r in zip(hs, rs):
                    if r.status == 2:
                        g._chk(g.f["schedule_one"](g.ctx, h, 0, C.byref(r1), C.byref(ev)), "schedule_one")
        us.append((time.perf_counter() - t0) * 1e6 / len(b))
        failed = sum(r.status == 2 for r in rs)
    try:
        same = list(g.same_pods())
    except Exception:  # a library from before ksg_debug_same_pods
        pass
    g.close()
    return {"us_per_pod": [round(x, 3) for x in us[WARM:]], "failed_per_batch": failed, "kernel": kern, "same_pods": same}


out = {}
nodes, init, pods = scheduling_basic(5000, 1000, BATCH * REPS)
for nfail in (0, 10, 500):
    bs = stream(pods, nfail, too_big)
    out[f"basic_{nfail}_unschedulable"] = {m: measure(nodes, init, ["default"], bs, m) for m in MODES}
nodes, init, pods = topology_spreading(5000, 1000, BATCH * REPS)
bs = stream(pods, 10, no_zone)
out["spreading_10_unschedulable"] = {m: measure(nodes, init, ["sched-0", "sched-1"], bs, m) for m in MODES}
out["config"] = CFG
print(json.dumps(out))
