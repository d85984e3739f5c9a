"""Summarise a C2 step's host trace and kernel trace (profiles/compile_memo_*.txt).

  python scripts/compile_memo_trace.py htrace <stderr log of a KSG_HOST_TRACE=1 bench.py run>
  python scripts/compile_memo_trace.py kernels <rocprofv3 --kernel-trace run_results.db> [dispatches per step]

htrace:  per 1000-pod batch, each chunk's compile time (us, and us per pod) and the time its launch was enqueued,
         relative to the batch's start; the wait for every chunk's results.
kernels: per step, every k_sched_same dispatch's start, duration and the idle gap before it, relative to the step's first
         dispatch.  A step is `dispatches per step` consecutive dispatches (the chunk plan's launches: 7 for 1000 pods
         of one template) when given, else a new step begins after a gap of more than 600 us.
"""
import re
import sqlite3
import sys


def htrace(path):
    tok = re.compile(r" (\d+):([a-z0-9]+?)(?:=(\d+)|0)(?= |$)")  # " <us>:<mark>=<arg>", or " <us>:<mark>0" without one
    nb = 0
    for line in open(path, errors="replace"):
        if not line.startswith("[htrace"):
            continue
        ev = [(m.group(2), int(m.group(3)) if m.group(3) else None, int(m.group(1))) for m in tok.finditer(line.rstrip())]
        if not ev or ev[0][0] != "batch" or ev[0][1] != 1000:
            continue
        nb += 1
        t0 = ev[0][2]
        out, comp_at, comp_from, comp_total, first_loop = [], None, 0, 0, None
        for what, a, t in ev:
            if what == "compile":
                comp_at, comp_from = t, a
            elif what == "compiled" and comp_at is not None:
                n = a - comp_from
                comp_total += t - comp_at
                out.append(f"compile[{comp_from},{a}) {t - comp_at}us ({(t - comp_at) / max(n, 1):.2f}/pod) done@{t - t0}")
                comp_at = None
            elif what == "loop":
                first_loop = first_loop if first_loop is not None else t - t0
                out.append(f"launch[{a}]@{t - t0}")
            elif what in ("mirror", "waited", "ret"):
                out.append(f"{what}{'' if a is None else a}@{t - t0}")
        print(f"batch {nb}: first launch @{first_loop}us, later chunks' compile {comp_total}us, "
              f"return @{ev[-1][2] - t0}us :: " + " ".join(out))


def kernels(path, per_step=0):
    c = sqlite3.connect(path)
    rows = list(c.execute("select start, end from kernels where name like '%k_sched_same%' order by start"))
    steps, cur = [], []
    for s, e in rows:
        if cur and (len(cur) == per_step if per_step else s - cur[-1][1] > 600_000):
            steps.append(cur)
            cur = []
        cur.append((s, e))
    if cur:
        steps.append(cur)
    for k, st in enumerate(steps):
        t0 = st[0][0]
        busy = sum(e - s for s, e in st) / 1e3
        span = (st[-1][1] - t0) / 1e3
        parts = []
        for i, (s, e) in enumerate(st):
            gap = (s - st[i - 1][1]) / 1e3 if i else 0.0
            parts.append(f"[gap {gap:.0f} @{(s - t0) / 1e3:.0f} dur {(e - s) / 1e3:.0f}]")
        print(f"step {k}: {len(st)} dispatches, span {span:.0f}us busy {busy:.0f}us idle {span - busy:.0f}us :: " + " ".join(parts))


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    else:
        htrace(sys.argv[2])
