"""The HIP runtime that libsparkbam_hip.so itself links, through ctypes (test infrastructure).

A test that hands the library a stream or a device pointer of its own has to make them with the
runtime instance the library uses: torch, when it was imported earlier in the run, brings a second
libamdhip64.so with no device state of ours, and a stream handle of that instance means nothing to
the library.  runtime() loads the library first and then asks for the runtime by its soname, which
the loader answers with the instance already mapped for it.

Only what the tests need is wrapped: a non-blocking stream (create, destroy, query, synchronize),
device memory (malloc, free, memcpy, memcpy_async), hipMemGetInfo and hipLaunchHostFunc.  Page-locked
host memory comes from sb.PinnedBuffer.

Gate makes ordering observable without guessing how long a kernel runs.  It is a host function
enqueued on a stream; its callback waits on a threading.Event, so the work enqueued behind a closed
gate has not run -- exactly, not probably.  The callback makes no HIP call and waits at most
GATE_WAIT_S; a threading.Timer opens the gate GATE_OPEN_S after it was enqueued whatever else
happens, so no wait is unbounded and nothing spins on the device.  A test checks the premise right
before the call under test: the gate is closed and the stream answers not-ready."""
import ctypes as C
import threading

from pkg import sb

HIP_SUCCESS, HIP_ERROR_NOT_READY = 0, 600
STREAM_NON_BLOCKING = 1
H2D, D2H, D2D = 1, 2, 3  # hipMemcpyKind
GATE_OPEN_S, GATE_WAIT_S = 0.1, 10.0

_HOST_FN = C.CFUNCTYPE(None, C.c_void_p)  # hipHostFn_t
_hip = None


class HipError(RuntimeError):
    pass


def runtime():
    global _hip
    if _hip is None:
        sb.lib()  # (the runtime is mapped with the library: the soname below resolves to that instance)
        h = C.CDLL("libamdhip64.so.7")
        P, SZ = C.c_void_p, C.c_size_t
        for name, args in (("hipMemGetInfo", [C.POINTER(SZ), C.POINTER(SZ)]),
                           ("hipStreamCreateWithFlags", [C.POINTER(P), C.c_uint]),
                           ("hipStreamDestroy", [P]), ("hipStreamQuery", [P]), ("hipStreamSynchronize", [P]),
                           ("hipMalloc", [C.POINTER(P), SZ]), ("hipFree", [P]),
                           ("hipMemcpy", [P, P, SZ, C.c_int]), ("hipMemcpyAsync", [P, P, SZ, C.c_int, P]),
                           ("hipLaunchHostFunc", [P, _HOST_FN, P])):
            f = getattr(h, name)
            f.argtypes, f.restype = args, C.c_int
        _hip = h
    return _hip


def _ok(rc, what):
    if rc != HIP_SUCCESS:
        raise HipError("%s: hipError_t %d" % (what, rc))


def mem_get_info():
    """(free, total) device bytes as the library's runtime reports them."""
    free, total = C.c_size_t(), C.c_size_t()
    _ok(runtime().hipMemGetInfo(C.byref(free), C.byref(total)), "hipMemGetInfo")
    return free.value, total.value


def stream_create():
    """A non-blocking stream: its handle as an int (what sb.Context(stream=...) takes)."""
    s = C.c_void_p()
    _ok(runtime().hipStreamCreateWithFlags(C.byref(s), STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")
    return s.value


def stream_destroy(s):
    _ok(runtime().hipStreamDestroy(s), "hipStreamDestroy")


def stream_ready(s):
    """hipStreamQuery: True when everything enqueued on `s` has completed, False when not yet."""
    rc = runtime().hipStreamQuery(s)
    if rc not in (HIP_SUCCESS, HIP_ERROR_NOT_READY):
        _ok(rc, "hipStreamQuery")
    return rc == HIP_SUCCESS


def stream_synchronize(s):
    _ok(runtime().hipStreamSynchronize(s), "hipStreamSynchronize")


def malloc(n):
    p = C.c_void_p()
    _ok(runtime().hipMalloc(C.byref(p), max(int(n), 1)), "hipMalloc")
    return p.value


def free(p):
    _ok(runtime().hipFree(p), "hipFree")


def _addr(x):
    """A device pointer (int) or the address of a numpy array's bytes."""
    return x.ctypes.data if hasattr(x, "ctypes") else int(x)


def memcpy(dst, src, n, kind):
    """Synchronous copy of n bytes; dst / src: a device pointer (int) or a numpy array."""
    _ok(runtime().hipMemcpy(_addr(dst), _addr(src), int(n), kind), "hipMemcpy")


def memcpy_async(dst, src, n, kind, stream):
    """Copy of n bytes enqueued on `stream`; a host side must be page-locked and outlive the copy."""
    _ok(runtime().hipMemcpyAsync(_addr(dst), _addr(src), int(n), kind, stream), "hipMemcpyAsync")


_LIVE = []  # the callbacks of gates not yet run: the runtime holds their addresses


class Gate:
    """A host function on `stream` that returns once open() was called (or GATE_WAIT_S passed)."""

    def __init__(self, stream):
        self.stream = stream
        self.event = threading.Event()
        self.entered = threading.Event()
        self.left = threading.Event()

        def wait(_user):  # runs on a thread of the runtime: no HIP call in here
            self.entered.set()
            self.event.wait(GATE_WAIT_S)
            self.left.set()

        self._fn = _HOST_FN(wait)
        _LIVE.append(self)
        _ok(runtime().hipLaunchHostFunc(stream, self._fn, None), "hipLaunchHostFunc")
        self._timer = threading.Timer(GATE_OPEN_S, self.event.set)
        self._timer.daemon = True
        self._timer.start()

    def closed(self):
        return not self.event.is_set()

    def open(self):
        self.event.set()

    def finish(self):
        """Open the gate and drain the stream (teardown: before anything behind the gate is freed)."""
        self.open()
        self._timer.cancel()
        stream_synchronize(self.stream)
        assert self.left.wait(GATE_WAIT_S)
        if self in _LIVE:
            _LIVE.remove(self)
