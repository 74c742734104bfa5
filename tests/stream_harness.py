"""What the stream-ordering tests share (test_stream_solver.py, test_stream_pose.py, test_stream_queries.py): the HIP runtime bound
through ctypes -- never torch's, whose stream handles belong to another copy of the runtime --, non-blocking streams with a GATE in
front of every call, poisoned device inputs and outputs, and one sequence of calls run twice.

The gate is a bounded delay queued on a stream: a host function that sleeps GATE_MS (hipLaunchHostFunc).  It never waits for the
test thread, so a call that is complete on return behind it cannot deadlock.  An event recorded behind the gate is queried right before the call under test is entered: it must not be ready.
That assertion, not the sleep's length, is what makes a case mean something (profiles/stream_measured.md: why 20 ms).

Poison: a device input holds ANOTHER valid batch (the case's own rolled by one instance) until a copy queued behind the gate
replaces it, so a read that does not wait for the stream computes the neighbour's answer; a device output starts as all-ones bytes
(a NaN as float64, -1 as int32), so a call that returns before its output is written leaves that behind.  Outputs are read back with
a plain hipMemcpy, on the null stream, which does not wait for device work on a non-blocking stream
(test_stream_solver.test_positive_control_of_the_read_back).  It does queue up behind a HOST-to-device copy that is pending on another
stream (profiles/stream_measured.md), and the copies of a call's device inputs are such copies: had the call returned without
draining its stream, the read could wait out the gate and find a finished output.  So a call with outputs is held to more than its
poison: right after it returns, before anything is read, hipStreamQuery of its stream must say that nothing is pending.

A sequence is a function of (Run, handle).  Run() is the reference: null stream, host arrays.  Run(lane, like=reference.rec) is the
test: every call behind a gate of the lane the handle is on, device arrays in and out.  Both record what they read under the same
keys; assert_same_records compares byte for byte."""
import ctypes as C
import time

import numpy as np

GATE_MS = 20
HIP_SUCCESS, HIP_NOT_READY = 0, 600
H2D, D2H, D2D = 1, 2, 3
_HOSTFN = C.CFUNCTYPE(None, C.c_void_p)

_hip = None


def hip():
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so")
        vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
        h.hipSetDevice.argtypes = [C.c_int]
        h.hipMalloc.argtypes = [vpp, C.c_size_t]
        h.hipFree.argtypes = [vp]
        h.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        h.hipStreamCreateWithFlags.argtypes = [vpp, C.c_uint]
        h.hipStreamDestroy.argtypes = [vp]
        h.hipStreamSynchronize.argtypes = [vp]
        h.hipStreamQuery.argtypes = [vp]
        h.hipHostMalloc.argtypes = [vpp, C.c_size_t, C.c_uint]
        h.hipHostFree.argtypes = [vp]
        h.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        h.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]
        h.hipEventCreate.argtypes = [vpp]
        h.hipEventRecord.argtypes = [vp, vp]
        h.hipEventQuery.argtypes = [vp]
        h.hipEventDestroy.argtypes = [vp]
        h.hipLaunchHostFunc.argtypes = [vp, _HOSTFN, vp]
        _chk(h.hipSetDevice(0), "hipSetDevice")
        _hip = h
    return _hip


def _chk(rc, what):
    if rc != HIP_SUCCESS:
        raise RuntimeError("%s failed with HIP error %d" % (what, rc))


def _sleep_gate(_):
    time.sleep(GATE_MS * 1e-3)


_SLEEP = _HOSTFN(_sleep_gate)   # (referenced for the life of the module: the runtime calls it from a thread of its own)


class Pinned:
    """page-locked host memory holding a copy of `a`, as a numpy array (.a)"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.p = C.c_void_p()
        self.nbytes = max(a.nbytes, 1)
        _chk(hip().hipHostMalloc(C.byref(self.p), self.nbytes, 0), "hipHostMalloc")
        self.a = np.frombuffer((C.c_char * self.nbytes).from_address(self.p.value), dtype=a.dtype, count=a.size).reshape(a.shape)
        self.a[...] = a

    def free(self):
        if self.p is not None:
            self.a = None
            hip().hipHostFree(self.p)
            self.p = None


class DevBuf:
    """device memory that the bindings take for a device array (data_ptr / is_cuda / numel), filled from `a` by a plain hipMemcpy"""
    is_cuda = True

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype, self.size, self.nbytes = a.shape, a.dtype, a.size, a.nbytes
        self.p = C.c_void_p()
        _chk(hip().hipMalloc(C.byref(self.p), max(a.nbytes, 1)), "hipMalloc")
        if a.nbytes:
            _chk(hip().hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D), "hipMemcpy")

    def data_ptr(self):
        return self.p.value

    def numel(self):
        return self.size

    def element_size(self):
        return self.dtype.itemsize

    def is_contiguous(self):
        return True

    def read(self):
        """the contents now, through the null stream: no wait for any non-blocking stream"""
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            _chk(hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, self.nbytes, D2H), "hipMemcpy")
        return out

    def free(self):
        if self.p is not None:
            hip().hipFree(self.p)
            self.p = None


def poison_like(a):
    """an array of a's shape and type with every byte 0xff: NaN as a float, -1 as an int"""
    a = np.asarray(a)
    return np.frombuffer(b"\xff" * a.nbytes, dtype=a.dtype).reshape(a.shape).copy()


class Lane:
    """a non-blocking stream and the gates queued on it"""

    def __init__(self):
        self.stream = C.c_void_p()
        _chk(hip().hipStreamCreateWithFlags(C.byref(self.stream), 1), "hipStreamCreateWithFlags")   # hipStreamNonBlocking
        self.events, self.gates = [], 0

    @property
    def ptr(self):
        return self.stream.value

    def gate(self):
        """queues the delay and an event behind it -> the event"""
        h = hip()
        _chk(h.hipLaunchHostFunc(self.stream, _SLEEP, None), "hipLaunchHostFunc")
        ev = C.c_void_p()
        _chk(h.hipEventCreate(C.byref(ev)), "hipEventCreate")
        _chk(h.hipEventRecord(ev, self.stream), "hipEventRecord")
        self.events.append(ev)
        self.gates += 1
        return ev

    def closed(self, ev):
        rc = hip().hipEventQuery(ev)
        if rc not in (HIP_SUCCESS, HIP_NOT_READY):
            raise RuntimeError("hipEventQuery failed with HIP error %d" % rc)
        return rc == HIP_NOT_READY

    def copy_in(self, dev, pinned):
        _chk(hip().hipMemcpyAsync(dev.p, pinned.p, dev.nbytes, H2D, self.stream), "hipMemcpyAsync")

    def copy_dev(self, dst, src):
        _chk(hip().hipMemcpyAsync(dst.p, src.p, dst.nbytes, D2D, self.stream), "hipMemcpyAsync")

    def memset(self, dev, byte):
        _chk(hip().hipMemsetAsync(dev.p, byte, dev.nbytes, self.stream), "hipMemsetAsync")

    def read_through(self, dev):
        """dev's contents, copied on THIS stream (the positive control's second stream)"""
        pin = Pinned(np.zeros(dev.shape, dtype=dev.dtype))
        try:
            _chk(hip().hipMemcpyAsync(pin.p, dev.p, dev.nbytes, D2H, self.stream), "hipMemcpyAsync")
            self.synchronize()
            return pin.a.copy()
        finally:
            pin.free()

    def synchronize(self):
        _chk(hip().hipStreamSynchronize(self.stream), "hipStreamSynchronize")

    def drained(self):
        """nothing queued on the stream is pending (hipStreamQuery)"""
        rc = hip().hipStreamQuery(self.stream)
        if rc not in (HIP_SUCCESS, HIP_NOT_READY):
            raise RuntimeError("hipStreamQuery failed with HIP error %d" % rc)
        return rc == HIP_SUCCESS

    def close(self):
        """after every handle on the stream is closed"""
        if self.stream is None:
            return
        h = hip()
        h.hipStreamSynchronize(self.stream)
        for ev in self.events:
            h.hipEventDestroy(ev)
        h.hipStreamDestroy(self.stream)
        self.stream, self.events = None, []


class Run:
    """One run of a sequence.  Run(): the reference -- inputs are the host arrays, calls are made as they are, results are the host
    arrays the bindings return.  Run(lane, like=reference.rec): every call behind a gate on `lane` (asserted closed when the call is
    entered), per-instance inputs as device arrays that hold the wrong batch until a copy behind the gate, results into poisoned
    device arrays read back right after the call."""

    def __init__(self, lane=None, like=None, host_inputs=False):
        self.lane, self.like, self.rec, self.keep, self.pending, self.host_inputs = lane, like, {}, [], [], host_inputs
        self.gated, self.in_call = lane is not None, False

    def on(self, lane):
        """the calls that follow are gated on `lane` (the handle was moved there)"""
        self.lane = lane

    def inp(self, x, dtype=np.float64):
        """a per-instance input of the next call"""
        x = np.ascontiguousarray(x, dtype=dtype)
        if not self.gated or self.host_inputs:
            return x
        assert not self.in_call, "Run.inp inside the call it is for: nothing would stage it behind the gate"
        dev, pin = DevBuf(np.roll(x, 1, axis=0)), Pinned(x)
        self.keep += [dev, pin]
        self.pending.append((dev, pin))
        return dev

    def do(self, fn, *a, **kw):
        if not self.gated:
            return fn(*a, **kw)
        ev = self.lane.gate()
        for dev, pin in self.pending:
            self.lane.copy_in(dev, pin)
        self.pending = []
        assert self.lane.closed(ev), "the gate was open when the call was entered: the case proves nothing (raise GATE_MS)"
        self.in_call = True
        try:
            return fn(*a, **kw)
        finally:
            self.in_call = False

    def get(self, key, fn):
        """fn(out) is a getter or query with one output: recorded under `key`.  out is None on the reference run."""
        return self.get_n([key], lambda outs: fn(None if outs is None else outs[0]), single=True)

    def get_n(self, keys, fn, specs=None, single=False):
        """fn(outs) with several outputs, in the order of `keys` (a key None: an output the call is not asked for).  specs = a (shape,
        dtype) per output: the reference run hands poisoned host arrays of those to the same out= (the raw layout of the C call, and
        the same bytes where the call writes nothing); without specs it takes what fn(None) returns."""
        if not self.gated:
            if specs is not None:
                outs = [None if k is None else poison_like(np.empty(shape, dtype=dtype)) for k, (shape, dtype) in zip(keys, specs)]
                self.do(fn, outs)
                r = outs
            else:
                r = self.do(fn, None)
                r = (r,) if single else tuple(r)
            assert len(r) == len(keys), (keys, len(r))
            for k, v in zip(keys, r):
                if k is not None:
                    assert k not in self.rec, k
                    self.rec[k] = np.array(v)
            return
        outs = [None if k is None else DevBuf(poison_like(self.like[k])) for k in keys]
        self.keep += [o for o in outs if o is not None]
        self.do(fn, outs)
        drained = self.lane.drained()   # (asked before the read: the read below may itself wait for a pending copy)
        for k, o in zip(keys, outs):
            if k is not None:
                self.rec[k] = o.read()   # right after the call, no synchronisation of ours
        assert drained, "%s: the call returned with work still queued on its stream: its outputs are not complete on return" % (keys,)

    def put(self, key, value):
        """a value the call returned on the host (counts, flags, statistics)"""
        assert key not in self.rec, key
        self.rec[key] = np.array(value)

    def close(self):
        if self.lane is not None and self.lane.stream is not None:
            self.lane.synchronize()
        for b in self.keep:
            b.free()
        self.keep = []


def assert_same_records(got, want, what=""):
    assert list(got) == list(want), (what, [k for k in want if k not in got], [k for k in got if k not in want])
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            nan = int(np.isnan(g).sum()) if g.dtype.kind == "f" else int((g == -1).sum())
            rows = np.flatnonzero((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(axis=1)) if g.ndim else []
            raise AssertionError("%s: %s differs from the null-stream run in %d of %d rows (first %s); %d poisoned entries left"
                                 % (what, k, len(rows), g.shape[0] if g.ndim else 1, [int(r) for r in rows[:5]], nan))


def run_both(make, sequence, lanes=1, what="", host_inputs=False):
    """`sequence(run, handle)` on a fresh handle on the null stream with host arrays, then on a fresh handle moved to a non-blocking
    stream with a gate before every call and device arrays (host_inputs: the inputs stay host arrays, through the library's staging
    buffers): byte-equal records.  -> (reference records, number of gates)"""
    ref = Run()
    s = make()
    try:
        sequence(ref, s)
    finally:
        s.close()
    ls = [Lane() for _ in range(lanes)]
    run = Run(ls[0], like=ref.rec, host_inputs=host_inputs)
    run.lanes = ls
    s = None
    try:
        s = make()
        s.set_stream(ls[0].ptr)
        sequence(run, s)
        assert_same_records(run.rec, ref.rec, what)
        gates = sum(l.gates for l in ls)
        assert gates > 0
        return ref.rec, gates
    finally:
        for l in ls:
            l.synchronize()
        if s is not None:
            s.close()
        run.close()
        for l in ls:
            l.close()
