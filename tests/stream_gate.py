"""A timed gate on a non-blocking HIP stream, for the ordering tests of tests/test_streams.py (a plain helper module).

Gate mechanism: hipLaunchHostFunc.  gate.close(s) enqueues a host function on `s` that waits on a threading.Event with the timeout G;
whatever is enqueued on `s` afterwards stays behind it until the test calls gate.open() or G seconds have passed, whichever is first.
The gate can therefore never hold a stream for longer than G and nothing can hang.  The callback calls no HIP function; its CFUNCTYPE
object is kept alive by the gate; the binding's CDLL calls release the GIL, so the callback runs while the main thread sits inside the
library.  An event recorded right behind the host function is the host's view of the gate: hipEventQuery answers not-ready while it is
closed.

G = 0.1 s, the starting value: on an MI355X neither condition below failed with it for a reason other than a library bug, so it was
not raised.  G is no tolerance on any result: a case decides nothing unless the harness has SEEN the gate closed after an asynchronous
call returned (event not ready, open() not yet called), or opened by its timeout before a synchronising call returned; it fails
otherwise.  A blocked host function does not stall other streams on this runtime (test_gate_holds_one_stream_only), so no other
gate was needed.  Observed GPU time of tests/test_streams.py on an MI355X: 21 s for its 279 GPU tests (about 150 synchronising
cases at G each; an asynchronous case takes about 20 ms).

Runtime: the HIP runtime libbmsp.so already loaded, found through /proc/self/maps, so there is one runtime in the process.

bmsp_memcpy_d2h / bmsp_memcpy_h2d synchronise the DEVICE (they are the library's synchronous copies), so they return only once a
closed gate has opened.  What the harness reads while a gate is closed it reads itself: hipMemcpyAsync on a second non-blocking
stream (Side.read below), which waits for nothing but that stream.
"""
import ctypes as C
import threading
import time
import numpy as np

G = 0.1

hipStreamNonBlocking = 1
hipSuccess, hipErrorNotReady = 0, 600
_D2H, _D2D, _H2D = 2, 3, 1
_HOSTFN = C.CFUNCTYPE(None, C.c_void_p)

_H = None


def _hip():
    """the HIP runtime libbmsp.so runs on (the same loaded file, so one runtime in the process)."""
    global _H
    if _H is not None:
        return _H
    path = None
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            path = line.split()[-1]
            break
    assert path, "libamdhip64 is not loaded"
    H = C.CDLL(path)
    vp = C.c_void_p
    H.hipStreamCreate.argtypes = [C.POINTER(vp)]
    H.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    H.hipStreamSynchronize.argtypes = [vp]
    H.hipStreamDestroy.argtypes = [vp]
    H.hipStreamQuery.argtypes = [vp]
    H.hipLaunchHostFunc.argtypes = [vp, _HOSTFN, vp]
    H.hipEventCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    H.hipEventRecord.argtypes = [vp, vp]
    H.hipEventQuery.argtypes = [vp]
    H.hipEventDestroy.argtypes = [vp]
    H.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    H.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]
    H.hipGetLastError.argtypes = []
    _H = H
    return H


def hip_check(status, what=""):
    assert status == hipSuccess, "HIP error %d %s" % (status, what)


def new_stream():
    """a non-blocking stream (no implicit ordering against the null stream): what PyTorch's streams are."""
    s = C.c_void_p()
    hip_check(_hip().hipStreamCreateWithFlags(C.byref(s), hipStreamNonBlocking), "hipStreamCreateWithFlags")
    return s


def destroy_stream(s):
    H = _hip()
    H.hipStreamSynchronize(s)
    H.hipStreamDestroy(s)


def stream_sync(s):
    hip_check(_hip().hipStreamSynchronize(s), "hipStreamSynchronize")


def memcpy_d2d_async(dst, src, nbytes, s):
    if nbytes:
        hip_check(_hip().hipMemcpyAsync(dst, src, nbytes, _D2D, s), "hipMemcpyAsync d2d")


def memset_async(dst, byte, nbytes, s):
    if nbytes:
        hip_check(_hip().hipMemsetAsync(dst, byte, nbytes, s), "hipMemsetAsync")


class Side:
    """a second non-blocking stream for what the harness itself reads or writes while a gate is closed."""

    def __init__(self):
        self.s = new_stream()

    def read(self, ptr, n, dtype):
        out = np.empty(n, dtype)
        if out.nbytes:
            hip_check(_hip().hipMemcpyAsync(out.ctypes.data, ptr, out.nbytes, _D2H, self.s), "hipMemcpyAsync d2h")
            stream_sync(self.s)
        return out

    def fill(self, ptr, byte, nbytes):
        memset_async(ptr, byte, nbytes, self.s)
        stream_sync(self.s)

    def close(self):
        if self.s is not None:
            destroy_stream(self.s)
            self.s = None


class Gate:
    """one closing of one stream.  close(s) -> [work behind the gate] -> open() -> hipStreamSynchronize."""

    def __init__(self, timeout=G):
        self.timeout = timeout
        self._ev = threading.Event()
        self._entered = threading.Event()
        self._left = threading.Event()
        self._open_called = False
        self.timed_out = False
        self._hip_event = C.c_void_p()
        self._stream = None

        def wait(_):
            self._entered.set()
            self.timed_out = not self._ev.wait(self.timeout)
            self._left.set()

        self._cb = _HOSTFN(wait)   # kept alive as long as the gate

    def close(self, s):
        H = _hip()
        self._stream = s
        hip_check(H.hipLaunchHostFunc(s, self._cb, None), "hipLaunchHostFunc")
        hip_check(H.hipEventCreateWithFlags(C.byref(self._hip_event), 2), "hipEventCreateWithFlags")   # hipEventDisableTiming
        hip_check(H.hipEventRecord(self._hip_event, s), "hipEventRecord")
        return self

    def is_closed(self):
        """the host function has not returned, open() has not been called and the event behind the gate is not ready."""
        if self._open_called or self._left.is_set():
            return False
        q = _hip().hipEventQuery(self._hip_event)
        if q == hipErrorNotReady:
            _hip().hipGetLastError()
            return not self._left.is_set()
        hip_check(q, "hipEventQuery")
        return False

    def opened_by_timeout(self):
        """the host function ran to its time limit: everything enqueued behind it waited the whole G."""
        return self._left.is_set() and self.timed_out and not self._open_called

    def open(self):
        self._open_called = True
        self._ev.set()

    def finish(self):
        """opens the gate if it is still closed, waits for the stream and releases the event."""
        self.open()
        if self._stream is not None:
            stream_sync(self._stream)
        if self._hip_event:
            _hip().hipEventDestroy(self._hip_event)
            self._hip_event = C.c_void_p()


def wait_until(pred, limit=2.0):
    """polls pred() for at most `limit` seconds (no fixed sleep); returns its last value"""
    t0 = time.monotonic()
    while not pred():
        if time.monotonic() - t0 > limit:
            return False
        time.sleep(0.0005)
    return True
