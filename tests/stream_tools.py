"""Helpers of tests/test_stream_order_gpu.py: device work that keeps a stream busy, and the two ways a call is run there -
alone and synchronously (the reference), or on a side stream behind busy work with its inputs arriving late.

Only ordinary, terminating device work: `busy` is torch.cuda._sleep (a kernel that counts clock ticks down and exits), sized
once per process with device events. Nothing spins on a flag."""
import numpy as np

BUSY_MS = 200.0
_TICKS_PER_MS = None


def ticks_per_ms():
    """Clock ticks of torch.cuda._sleep per millisecond, measured once with device events (at least 20 ms of sleep timed)."""
    global _TICKS_PER_MS
    import torch
    if _TICKS_PER_MS is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(100_000)
        torch.cuda.synchronize()
        n, ms = 2_000_000, 0.0
        for _ in range(8):                                   # at most 8 doublings x 8: terminates whatever the clock rate
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 20.0:
                break
            n *= 8
        assert ms >= 20.0, f"torch.cuda._sleep({n}) took {ms} ms: cannot size the busy work"
        _TICKS_PER_MS = n / ms
    return _TICKS_PER_MS


def busy(stream, ms=BUSY_MS):
    """Queue work on `stream` that runs for at least `ms` milliseconds; returns at once."""
    import torch
    n = int(ms * 1.05 * ticks_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(n)


def to_dev(arrays):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


def to_np(tensors):
    return [t.cpu().numpy() for t in tensors]


def serial(call, wrong, real):
    """The reference: `call(dev, None)` on the default stream, synchronised after every step. The same two calls the side-stream
    run makes (first with the legal-but-wrong inputs, then with the real ones), so that calls which change the handle
    (appends) leave it in the same state."""
    import torch
    dev = to_dev(wrong)
    call(dev, None)
    torch.cuda.synchronize()
    for k, v in real.items():
        dev[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    torch.cuda.synchronize()
    out = to_np(call(dev, None))
    torch.cuda.synchronize()
    return out


def late_producer(call, wrong, real, s, with_block_only=False):
    """On stream s: one first call of the same shape with the wrong inputs (takes first-use workspace growth out), then
    busy(s) -> the real inputs copied in from pinned memory -> call(dev, s) -> a consumer that clones the outputs.
    Returns (clones as numpy, was s still busy when the call had returned). Neither the device nor the default stream is
    synchronised between the busy work and s.synchronize()."""
    import torch
    dev = to_dev(wrong)
    pin = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in real.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(dev, None if with_block_only else s)
    s.synchronize()
    with torch.cuda.stream(s):
        busy(s)
        for k in pin:
            dev[k].copy_(pin[k], non_blocking=True)
        outs = call(dev, None if with_block_only else s)
        clones = [o.clone() for o in outs]
    pending = not s.query()
    s.synchronize()
    return to_np(clones), pending


def assert_same(got, ref, what=""):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(g, r, err_msg=f"{what} output {i}")
