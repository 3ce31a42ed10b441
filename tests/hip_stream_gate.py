"""Caller-owned HIP streams and a bounded gate for them (TEST INFRASTRUCTURE for tests/test_gpu_streams.py).

The stream handles come from the HIP runtime that libhefx.so itself is linked to -- the already loaded libamdhip64,
reached through libhefx.so's own handle -- and not from torch.cuda.Stream: torch may carry a runtime copy of
its own, and a stream handle of that copy means nothing to the engine's.

The GATE holds a stream shut for a fixed time while the host goes on submitting behind it: a host function
(hipLaunchHostFunc) that sleeps HOLD_SECONDS and then sets `opened`.  Nothing the host must release is involved -- no
stream memory wait, no event that might never be recorded, no spinning kernel: if the test dies, the stream opens by
itself.  `opened` turns "this entry returned while the stream was still shut" into a condition instead of a timing."""
from __future__ import annotations

import ctypes as C
import time

HOLD_SECONDS = 0.4
HIP_STREAM_NON_BLOCKING = 0x01

_hip = None
_HOSTFN = C.CFUNCTYPE(None, C.c_void_p)


def hip():
    """the HIP runtime of libhefx.so: symbols looked up through the library's own handle resolve in its dependencies, i.e.
    in the very libamdhip64 the engine calls (already loaded with it), whatever other copy the process may hold"""
    global _hip
    if _hip is not None:
        return _hip
    from seal_fyp_logistic_regression_amd import capi
    capi.lib()
    h = C.CDLL(capi.library_path(), mode=C.RTLD_GLOBAL)  # already mapped: a second handle to the same object
    h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    h.hipStreamQuery.argtypes = [C.c_void_p]
    h.hipLaunchHostFunc.argtypes = [C.c_void_p, _HOSTFN, C.c_void_p]
    h.hipGetErrorString.argtypes = [C.c_int]
    h.hipGetErrorString.restype = C.c_char_p
    for f in (h.hipStreamCreateWithFlags, h.hipStreamDestroy, h.hipStreamSynchronize, h.hipStreamWaitEvent, h.hipStreamQuery, h.hipLaunchHostFunc):
        f.restype = C.c_int
    _hip = h
    return h


def _chk(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {hip().hipGetErrorString(rc).decode()}")


class Stream:
    """a non-blocking stream (hipStreamNonBlocking: no implicit ordering with the default stream); `.handle` is what the
    Engine methods take as stream="""

    def __init__(self):
        s = C.c_void_p()
        _chk(hip().hipStreamCreateWithFlags(C.byref(s), HIP_STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")
        self.handle = s.value
        self._gates = []

    def wait_event(self, event):
        """hipStreamWaitEvent (the C-ABI has no entry for it); `event` from Engine.event()"""
        _chk(hip().hipStreamWaitEvent(self.handle, event, 0), "hipStreamWaitEvent")

    def idle(self) -> bool:
        return hip().hipStreamQuery(self.handle) == 0

    def gate(self, seconds: float = HOLD_SECONDS) -> "Gate":
        g = Gate(self, seconds)
        self._gates.append(g)  # the callback object must outlive the call
        return g

    def destroy(self):
        if self.handle:
            # a gate's callback must have run before its ctypes thunk may go: wait, then destroy, then drop the gates
            _chk(hip().hipStreamSynchronize(self.handle), "hipStreamSynchronize")
            _chk(hip().hipStreamDestroy(self.handle), "hipStreamDestroy")
            self.handle = None
        self._gates.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()


class Gate:
    """shuts `stream` for `seconds` from the moment the stream reaches it; `opened` is False until then"""

    def __init__(self, stream: Stream, seconds: float):
        self.opened = False
        self.entered = False

        def hold(_):
            self.entered = True
            time.sleep(seconds)
            self.opened = True

        self._fn = _HOSTFN(hold)
        _chk(hip().hipLaunchHostFunc(stream.handle, self._fn, None), "hipLaunchHostFunc")
