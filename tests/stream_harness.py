"""Stream-order harness (tests/test_streams_gpu.py uses it): runs one device call on a non-blocking side stream in a way
that turns an ordering mistake into a wrong answer every time, not into a rare race.

While the call under test is being enqueued, the side stream `s` is still busy with a delay, the call's input tensors hold
a DECOY (a valid input of the same shape from another seed), its outputs a sentinel and its workspace 0xA5 bytes.  The
true inputs arrive by a device-to-device copy that is queued on `s` behind the delay, and right behind the call the
outputs are cloned, the decoy goes back over the inputs and 0xA5 over the workspace -- all on `s`.  So

  - a kernel or memset launched on another stream than `s` runs at once: it reads the decoy, and what it writes is
    covered by the sentinel that `s` puts over the outputs after the delay;
  - work the library forked to a stream of its own and did not join back is cloned too early, or has its inputs and its
    workspace overwritten under it;
  - a blocking read-back through the null stream sees the 0xA5 workspace;
  - a call that blocks the host is seen by the delay's event, which must not have completed when an entry point that
    the header calls asynchronous returns.

A Case is three phases -- prepare (default stream, then a full synchronise), enqueue (everything on `s`, no waiting)
and finish -- so that two cases can be in flight on two streams at once; run() is the three in a row.
"""
from __future__ import annotations

import numpy as np

SENTINEL = 0x5A   # every byte of an output before the call
WORK_FILL = 0xA5  # every byte of a workspace before and after the call
SENTINEL32 = 0x5A5A5A5A


class Delay:
    """Device work of about `ms` milliseconds on a stream.  torch.cuda._sleep where it behaves (its time grows with its
    argument), otherwise a chain of large elementwise operations; calibrated once with events.  The figure is not a
    criterion of any test: the delay is long enough iff the in-flight query in Case.enqueue holds."""

    def __init__(self, dev, ms: float = 50.0):
        import torch
        self.ms = ms
        self.dev = dev
        self.cycles = 0
        self.reps = 0
        torch.cuda.synchronize()
        if hasattr(torch.cuda, "_sleep"):
            t1, t2 = self._time(lambda: torch.cuda._sleep(2_000_000)), self._time(lambda: torch.cuda._sleep(20_000_000))
            if t2 > 1.0 and t2 > 4.0 * t1:
                self.cycles = max(1, int(20_000_000 * ms / t2))
        if not self.cycles:
            self.x = torch.ones(32 << 20, dtype=torch.float32, device=dev)
            self._chain(8)
            per = self._time(lambda: self._chain(64)) / 64
            self.reps = max(1, int(ms / max(per, 1e-3)) + 1)
        self.measured_ms = self._time(self)

    def _chain(self, reps):
        for _ in range(reps):
            self.x.mul_(1.0)

    @staticmethod
    def _time(fn) -> float:
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def __call__(self):
        """enqueue the delay on torch's current stream"""
        import torch
        if self.cycles:
            torch.cuda._sleep(self.cycles)
        else:
            self._chain(self.reps)


def self_test(delay: Delay) -> None:
    """The harness's own proof that it can fail, and that the runtime does not serialise a side stream with the default
    one: a fill queued behind the delay on `s` must not be visible to a clone taken at once on the default stream."""
    import torch
    x = torch.zeros(1 << 20, dtype=torch.int32, device=delay.dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        delay()
        x.fill_(1)
    y = x.clone()
    torch.cuda.synchronize()
    assert int(y.abs().sum()) == 0, "the default stream waited for a side stream: no test of this module means anything"
    assert int(x.sum()) == x.numel()


def _to_torch(a):
    import torch
    if isinstance(a, torch.Tensor):
        return a
    a = np.array(a)  # (a contiguous, writable copy)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a)


class _In:
    __slots__ = ("t", "true", "decoy", "after_setup")


class Result:
    """outs: the clones of the outputs (numpy, in the order they were declared); ret: what the call returned;
    in_flight: the delay had not finished when the call returned to the host"""

    def __init__(self, outs, ret, in_flight):
        self.outs, self.ret, self.in_flight = outs, ret, in_flight


class Case:
    """One call on a side stream.  Declare the tensors with inp() / out() / work(), then set `call` (and `setup`):
    callables of the stream, run with that stream as torch's current one."""

    def __init__(self, dev, name: str = ""):
        self.dev, self.name = dev, name
        self.inputs: list[_In] = []
        self.outputs = []
        self.mids = []
        self.works = []
        self.call = None
        self.setup = None
        self._clones = None

    # ---- declaration -----------------------------------------------------------------------------------------------
    def inp(self, true, decoy, after_setup: bool = False, offset: int = 0):
        """an input tensor: holds `decoy` until the true value is copied in on the side stream -- in front of the setup
        call, or (after_setup: an input that only the call under test reads) behind it.  offset: the tensor starts that
        many bytes into its buffer (uint8 inputs)."""
        import torch
        tt, dt = _to_torch(true), _to_torch(decoy)
        assert tt.shape == dt.shape and tt.dtype == dt.dtype, "the decoy must have the true input's shape and type"
        i = _In()
        i.true, i.decoy, i.after_setup = tt.to(self.dev).contiguous(), dt.to(self.dev).contiguous(), after_setup
        if offset:
            assert tt.dtype == torch.uint8 and tt.dim() == 1
            i.t = torch.zeros(tt.numel() + offset + 16, dtype=torch.uint8, device=self.dev)[offset:offset + tt.numel()]
        else:
            i.t = torch.empty_like(i.true)
        i.t.copy_(i.decoy)
        self.inputs.append(i)
        return i.t

    def out(self, shape, dtype):
        """an output tensor: sentinel bytes in front of the call, cloned behind it"""
        import torch
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        self.outputs.append(t)
        return t

    def mid(self, shape, dtype):
        """a tensor the setup call writes and the call under test reads (cloned as well, behind the outputs)"""
        import torch
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        self.mids.append(t)
        return t

    def work(self, nbytes: int):
        import torch
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.dev)
        self.works.append(t)
        return t

    # ---- the three phases ------------------------------------------------------------------------------------------
    def _fill(self, tensors, byte):
        import torch
        for t in tensors:
            t.view(-1).view(torch.uint8).fill_(byte)

    def prepare(self, warm: bool = True) -> None:
        """default stream: (once through the call on the decoy, so that no first-use cost of the runtime -- loading a code
        object, growing a memory pool -- is taken for the call blocking;) sentinels; then a full synchronise"""
        import torch
        if warm:
            if self.setup is not None:
                self.setup(torch.cuda.current_stream())
            self.call(torch.cuda.current_stream())
        for i in self.inputs:
            i.t.copy_(i.decoy)
        self._fill(self.outputs + self.mids, SENTINEL)
        self._fill(self.works, WORK_FILL)
        torch.cuda.synchronize()

    def enqueue(self, s, delay: Delay, asynchronous: bool = True):
        import torch
        with torch.cuda.stream(s):
            delay()
            self._fill(self.outputs + self.mids, SENTINEL)
            for i in self.inputs:
                if not (i.after_setup and self.setup is not None):
                    i.t.copy_(i.true, non_blocking=True)
            if self.setup is not None:
                self.setup(s)
                delay()  # (a setup call may synchronise: the call under test gets a delay of its own)
                self._fill(self.outputs, SENTINEL)
                for i in self.inputs:
                    if i.after_setup:
                        i.t.copy_(i.true, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
            self._ret = self.call(s)
            self._in_flight = not ev.query()
            self._clones = [t.clone() for t in self.outputs + self.mids]
            for i in self.inputs:
                i.t.copy_(i.decoy, non_blocking=True)
            self._fill(self.works, WORK_FILL)
        self._stream = s
        if asynchronous:
            assert self._in_flight, (f"{self.name}: the delay on the side stream had finished when the call returned: the "
                                     f"call blocked the host (or took longer to enqueue than the {delay.measured_ms:.0f} ms delay)")
        return self

    def finish(self, synchronize: bool = True) -> Result:
        """synchronize=False: no stream synchronise by the test; the clones are read with a synchronous copy on `s`"""
        import torch
        if synchronize:
            self._stream.synchronize()
            outs = [c.cpu().numpy() for c in self._clones]
        else:
            with torch.cuda.stream(self._stream):
                outs = [c.cpu().numpy() for c in self._clones]
        return Result(outs, self._ret, self._in_flight)


def run(case: Case, delay: Delay, asynchronous: bool = True, stream=None, synchronize: bool = True, warm: bool = True) -> Result:
    import torch
    case.prepare(warm)
    s = stream if stream is not None else torch.cuda.Stream()
    case.enqueue(s, delay, asynchronous)
    return case.finish(synchronize)
