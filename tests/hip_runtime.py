"""The HIP runtime instance that libagpt_hip.so itself is bound to, from Python: streams, events and device-to-device copies for the
tests that order their own GPU work with the library's (test_gpu_streams.py).  A stream or event handle means something only to the
runtime copy that created it, so the copy is found, not assumed: after ag.lib() is loaded, in a process that has not imported torch
(whose wheel carries a libamdhip64 of its own), exactly one libamdhip64 is mapped, and that file is opened.  Device memory comes from
Context.alloc."""
import ctypes as C
import time

import ag_pathtracer_amd as ag

hipSuccess, hipErrorNotReady = 0, 600
hipStreamNonBlocking = 1
hipMemcpyDeviceToDevice = 3


def mapped_runtimes():
    """the libamdhip64 files mapped into this process, by path"""
    with open("/proc/self/maps") as f:
        return sorted({ln.split(None, 5)[5].strip() for ln in f if "libamdhip64" in ln and len(ln.split(None, 5)) == 6})


class HipError(RuntimeError):
    pass


class Runtime:
    def __init__(self):
        ag.lib()
        paths = mapped_runtimes()
        assert len(paths) == 1, "expected exactly one libamdhip64 mapped beside libagpt_hip.so (was torch imported in this process?): %s" % paths
        self.path = paths[0]
        L = self.L = C.CDLL(self.path)
        vp = C.c_void_p
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(vp), C.c_uint]), ("hipStreamDestroy", [vp]), ("hipStreamSynchronize", [vp]),
                           ("hipStreamQuery", [vp]), ("hipMemcpyAsync", [vp, vp, C.c_size_t, C.c_int, vp]), ("hipEventCreate", [C.POINTER(vp)]),
                           ("hipEventRecord", [vp, vp]), ("hipEventSynchronize", [vp]), ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp]),
                           ("hipEventDestroy", [vp])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = C.c_int

    def _check(self, rc, what):
        if rc != hipSuccess:
            raise HipError("%s failed: hipError_t %d" % (what, rc))

    def stream_create(self):
        """a stream created with hipStreamNonBlocking: nothing orders it with the null stream"""
        s = C.c_void_p()
        self._check(self.L.hipStreamCreateWithFlags(C.byref(s), hipStreamNonBlocking), "hipStreamCreateWithFlags")
        assert s.value
        return s.value

    def stream_destroy(self, s):
        self._check(self.L.hipStreamDestroy(C.c_void_p(s)), "hipStreamDestroy")

    def stream_synchronize(self, s):
        self._check(self.L.hipStreamSynchronize(C.c_void_p(s)), "hipStreamSynchronize")

    def stream_query(self, s):
        """hipSuccess (everything enqueued on s is done) or hipErrorNotReady"""
        rc = self.L.hipStreamQuery(C.c_void_p(s))
        if rc not in (hipSuccess, hipErrorNotReady):
            raise HipError("hipStreamQuery failed: hipError_t %d" % rc)
        return rc

    def copy_async(self, dst, src, nbytes, s):
        """device to device, enqueued on s"""
        self._check(self.L.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, hipMemcpyDeviceToDevice, C.c_void_p(s)), "hipMemcpyAsync")

    def event_create(self):
        e = C.c_void_p()
        self._check(self.L.hipEventCreate(C.byref(e)), "hipEventCreate")
        return e.value

    def event_record(self, e, s):
        self._check(self.L.hipEventRecord(C.c_void_p(e), C.c_void_p(s)), "hipEventRecord")

    def event_synchronize(self, e):
        self._check(self.L.hipEventSynchronize(C.c_void_p(e)), "hipEventSynchronize")

    def event_elapsed_ms(self, a, b):
        ms = C.c_float(0)
        self._check(self.L.hipEventElapsedTime(C.byref(ms), C.c_void_p(a), C.c_void_p(b)), "hipEventElapsedTime")
        return float(ms.value)

    def event_destroy(self, e):
        self._check(self.L.hipEventDestroy(C.c_void_p(e)), "hipEventDestroy")


_RUNTIME = None


def runtime():
    global _RUNTIME
    if _RUNTIME is None:
        _RUNTIME = Runtime()
    return _RUNTIME


class Delay:
    """A chain of large device-to-device copies between two scratch buffers: GPU work of a known duration that the host enqueues in
    microseconds and does not wait for.  The chain is sized once, by measurement with two events on the stream it is measured on:
    `copies` copies of `nbytes` take `ms`."""
    NBYTES = 512 << 20
    TARGET_MS = 60.0

    def __init__(self, ctx, stream):
        hip = self.hip = runtime()
        self.ctx = ctx
        self.a, self.b = ctx.alloc(self.NBYTES), ctx.alloc(self.NBYTES)
        ctx.memset(self.a, 0, self.NBYTES)
        ctx.memset(self.b, 0, self.NBYTES)
        self.copies = 4
        self.enqueue(stream)                    # (the first copies pay for the runtime's own set-up)
        hip.stream_synchronize(stream)
        probe = self.measure(stream)
        self.copies = max(4, min(4096, int(self.TARGET_MS / (probe / self.copies)) + 1))
        self.ms = self.measure(stream)

    def enqueue(self, stream):
        for k in range(self.copies):
            src, dst = (self.a, self.b) if k % 2 == 0 else (self.b, self.a)
            self.hip.copy_async(dst, src, self.NBYTES, stream)

    def measure(self, stream):
        hip = self.hip
        e0, e1 = hip.event_create(), hip.event_create()
        try:
            hip.event_record(e0, stream)
            t0 = time.perf_counter()
            self.enqueue(stream)
            self.enqueue_ms = 1e3 * (time.perf_counter() - t0)
            hip.event_record(e1, stream)
            hip.event_synchronize(e1)
            return hip.event_elapsed_ms(e0, e1)
        finally:
            hip.event_destroy(e0)
            hip.event_destroy(e1)

    def free(self):
        self.ctx.free(self.a)
        self.ctx.free(self.b)
