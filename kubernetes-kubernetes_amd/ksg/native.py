"""Loader for the product library lib/libksg.so (HIP kernels for gfx950 + the C ABI).

There is deliberately no fallback: if the library is missing, fails to load, or no HIP
device is visible, `Scheduler(...)` raises.  The parity oracle lives in oracle/ and is
never reachable from here.
"""
import ctypes as C
import os

from .abi import Backend, KsgError

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("KSG_LIB") or os.path.join(PKG, "lib", "libksg.so")  # KSG_LIB: the diagnostic build
HEADER = os.path.join(os.path.dirname(PKG), "include", "ksg.h")

_lib = None


def load():
    """dlopen libksg.so (raises KsgError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise KsgError(f"{LIB} not built: run `make -C {PKG}` or __graft_entry__.build()")
        lib = C.CDLL(LIB)
        lib.ksg_last_batch_kernel_stats.restype = C.c_int
        lib.ksg_last_batch_kernel_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.ksg_comm_unique_id.restype = C.c_int
        lib.ksg_comm_unique_id.argtypes = [C.c_char_p, C.c_size_t]
        lib.ksg_create_error.restype = C.c_char_p
        lib.ksg_shard_range.restype = C.c_int
        lib.ksg_shard_range.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.ksg_debug_relayouts.restype = C.c_int
        lib.ksg_debug_relayouts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.ksg_generation.restype = C.c_int
        lib.ksg_generation.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.ksg_debug_compare_mirror.restype = C.c_int
        lib.ksg_debug_compare_mirror.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.ksg_debug_batching.restype = C.c_int
        lib.ksg_debug_batching.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.ksg_debug_loop_stats.restype = C.c_int
        lib.ksg_debug_loop_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        from .abi import Result
        lib.ksg_debug_schedule_calls.restype = C.c_int
        lib.ksg_debug_schedule_calls.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_uint32,
                                                 C.POINTER(Result), C.POINTER(C.c_double)]
        _lib = lib
    return _lib


def _diag_calls():
    """ksg_schedule_one_diag / ksg_schedule_batch_diag (ABI 3), bound on first use: not in abi._sig, which the
    oracle's library shares, and not in load(), so that KSG_LIB may still name a library built before them."""
    lib = load()
    if not getattr(lib, "_ksg_diag_bound", False):
        from .abi import Diagnosis, EvalOut, Result
        lib.ksg_schedule_one_diag.restype = C.c_int
        lib.ksg_schedule_one_diag.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(Result), C.POINTER(EvalOut),
                                              C.POINTER(Diagnosis)]
        lib.ksg_schedule_batch_diag.restype = C.c_int
        lib.ksg_schedule_batch_diag.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_uint32,
                                                C.POINTER(Result), C.POINTER(Diagnosis)]
        lib._ksg_diag_bound = True
    return lib.ksg_schedule_one_diag, lib.ksg_schedule_batch_diag


class Scheduler(Backend):
    """One kube-scheduler profile + cache mirror resident in HBM (ksg_create)."""

    def __init__(self, config=None):
        super().__init__(load(), "ksg_", config)

    def schedule_one_diag(self, handle, assume=True, evaluate=False):
        """ksg_schedule_one_diag -> (Result, eval dict or None, Diagnosis): the cycle with its FitError reduced on
        the device (every counter 0 unless the cycle ended unschedulable)."""
        from .abi import FLAG_ASSUME, Diagnosis, Result
        r, dg = Result(), Diagnosis()
        ev = self._eval_alloc() if evaluate else None
        self._chk(_diag_calls()[0](self.ctx, handle, FLAG_ASSUME if assume else 0, C.byref(r),
                                                 C.byref(ev) if evaluate else None, C.byref(dg)), "schedule_one_diag")
        return r, (self._eval_dict(ev) if evaluate else None), dg

    def schedule_batch_diag(self, handles, assume=True):
        """ksg_schedule_batch_diag -> ([Result], [Diagnosis]): pod i's diagnosis is as of its own cycle (the
        assumes of pods 0..i-1 applied, none later)."""
        from .abi import FLAG_ASSUME, Diagnosis, Result
        n = len(handles)
        hs = (C.c_int32 * n)(*handles)
        rs = (Result * n)()
        ds = (Diagnosis * n)()
        self._chk(_diag_calls()[1](self.ctx, hs, n, FLAG_ASSUME if assume else 0, rs, ds),
                  "schedule_batch_diag")
        return [rs[i] for i in range(n)], [ds[i] for i in range(n)]

    def kernel_stats(self):
        """(avg ms, algorithmic bytes, launches, kernel name) of the last batch: per k_filter_score
        launch, or per pod inside a persistent loop (k_sched_loop, k_agg_loop) when most pods ran there
        (launches: the pods that loop ran)."""
        ms, by, n, k = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
        self._chk(self.lib.ksg_last_batch_kernel_stats(self.ctx, C.byref(ms), C.byref(by), C.byref(n), C.byref(k)),
                  "kernel_stats")
        return ms.value, by.value, n.value, {1: "k_sched_loop", 2: "k_agg_loop"}.get(k.value, "k_filter_score")

    def compare_mirror(self, sync=False):
        """(differing nodes + pod-table slots, first difference) between the device mirror and the
        host cache shadow (ksg_debug_compare_mirror); sync: rebuild a stale mirror first."""
        nd, first = C.c_int32(), C.c_int32()
        self._chk(self.lib.ksg_debug_compare_mirror(self.ctx, 1 if sync else 0, C.byref(nd), C.byref(first)),
                  "compare_mirror")
        return nd.value, first.value

    def generation(self):
        """(node-list rebuilds, cache mutations applied) -- ksg_generation, the plugin shim's consistency check."""
        lg, ev = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.ksg_generation(self.ctx, C.byref(lg), C.byref(ev)), "generation")
        return lg.value, ev.value

    def batching(self):
        """(pods placed by an OpportunisticBatching hint, scheduling cycles counted) -- ksg_debug_batching."""
        h, c = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.ksg_debug_batching(self.ctx, C.byref(h), C.byref(c)), "batching")
        return h.value, c.value

    def loop_stats(self):
        """(batches whose persistent loop gave up, batches an in-process group re-ran over the all-reduce
        path) so far (ksg_debug_loop_stats)."""
        g, r = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.ksg_debug_loop_stats(self.ctx, C.byref(g), C.byref(r)), "loop_stats")
        return g.value, r.value

    def lean_pods(self):
        """(lean, general): the pods handed to k_sched_loop so far, while loopLeanSelect was on, that its lean
        selection path takes and that it does not (ksg_debug_lean_pods; bound on first use, so that KSG_LIB may
        still name a library built before it)."""
        fn = self.lib.ksg_debug_lean_pods
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(fn(self.ctx, C.byref(a), C.byref(b)), "lean_pods")
        return a.value, b.value

    def compile_memo(self):
        """(hits, misses): the scheduling cycles' host compiles so far that copied the compile memo's program, and
        that compiled in full (ksg_debug_compile_memo; bound on first use, as lean_pods)."""
        fn = self.lib.ksg_debug_compile_memo
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(fn(self.ctx, C.byref(a), C.byref(b)), "compile_memo")
        return a.value, b.value

    def same_carry(self):
        """(loaded, filled): the k_sched_same launches so far that loaded the previous launch's carried state, and
        that evaluated their fill (ksg_debug_same_carry; bound on first use, as lean_pods)."""
        fn = self.lib.ksg_debug_same_carry
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(fn(self.ctx, C.byref(a), C.byref(b)), "same_carry")
        return a.value, b.value

    def same_pods(self):
        """(taken, not_taken): the pods of k_sched_loop's runs so far that k_sched_same ran, and that k_sched_loop
        ran (ksg_debug_same_pods; bound on first use, as lean_pods)."""
        fn = self.lib.ksg_debug_same_pods
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(fn(self.ctx, C.byref(a), C.byref(b)), "same_pods")
        return a.value, b.value

    def resident_calls(self):
        """(sched, agg, launch): the schedule_one(assume=True) calls without evaluation or diagnosis so far that the
        resident k_sched_loop served, that the resident k_agg_loop served, and that took the launch path
        (ksg_debug_resident_calls; bound on first use, as lean_pods)."""
        fn = self.lib.ksg_debug_resident_calls
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        a, b, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(fn(self.ctx, C.byref(a), C.byref(b), C.byref(l)), "resident_calls")
        return a.value, b.value, l.value

    def sched_same(self, handle_a, handle_b):
        """Whether pod b may follow pod a in a k_sched_same run (ksg_debug_sched_same; schedules nothing)."""
        fn = self.lib.ksg_debug_sched_same
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        rc = fn(self.ctx, handle_a, handle_b)
        if rc < 0:
            self._chk(rc, "sched_same")
        return rc == 1

    def relayouts(self):
        """(full mirror rebuilds, gather re-layouts) so far (ksg_debug_relayouts)."""
        f, g = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.ksg_debug_relayouts(self.ctx, C.byref(f), C.byref(g)), "relayouts")
        return f.value, g.value

    def schedule_calls(self, handles, assume=True):
        """ksg_schedule_one for each handle, back to back from native code (ksg_debug_schedule_calls):
        (results, mean wall µs per call)."""
        from .abi import FLAG_ASSUME, Result
        n = len(handles)
        hs = (C.c_int32 * n)(*handles)
        rs = (Result * n)()
        us = C.c_double()
        self._chk(self.lib.ksg_debug_schedule_calls(self.ctx, hs, n, FLAG_ASSUME if assume else 0, rs, C.byref(us)),
                  "schedule_calls")
        return [rs[i] for i in range(n)], us.value

    def shard_range(self):
        """(first snapshot index, node count) this rank evaluates (node-sharded contexts)."""
        a, n = C.c_int32(), C.c_int32()
        self._chk(self.lib.ksg_shard_range(self.ctx, C.byref(a), C.byref(n)), "shard_range")
        return a.value, n.value


def group_loop_kernel():
    """The k_sched_loop instance an in-process group's last loop launch dispatched in this process, as the runtime
    names it (ksg_debug_group_loop_kernel; "" before the first such launch, None with a library built before it)."""
    lib = load()
    if not hasattr(lib, "ksg_debug_group_loop_kernel"):
        return None
    fn = lib.ksg_debug_group_loop_kernel
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(512)
    rc = fn(buf, 512)
    if rc < 0:
        raise KsgError(f"ksg_debug_group_loop_kernel: rc={rc}")
    return buf.value.decode()


def comm_unique_id():
    """ncclGetUniqueId as hex (rank 0 creates it; every rank passes it as distributed.ncclId)."""
    lib = load()
    buf = C.create_string_buffer(512)
    rc = lib.ksg_comm_unique_id(buf, 512)
    if rc < 0:
        raise KsgError(f"ksg_comm_unique_id: rc={rc}: {lib.ksg_create_error().decode(errors='replace')}")
    return buf.value.decode()
