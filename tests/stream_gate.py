"""A gate and a canary on a non-blocking stream, built from the C ABI alone (tests/test_gpu_streams.py, tests/stream_first_use_worker.py).

Gate(st) puts on the stream `st` (qmg_stream_create: hipStreamNonBlocking), in order: an event, a run of large qmg_memcpy_d2d copies between
two gate buffers that takes long compared with enqueueing a call, a second event, and a qmg_memcpy_d2d of the double 1.0 into an 8-byte canary
that holds 0xFF bytes.  Whatever is enqueued on `st` behind the gate cannot start before the canary is written.

gate.closed() reads the canary with a synchronous qmg_memcpy_d2h on the NULL stream, which is not ordered against a non-blocking stream, and
is True while the canary still holds the poison.  A caller that enqueues work on `st` and then sees a closed gate knows that none of that work
has run yet; a kernel of it that escaped to the null stream was enqueued before the canary read and the read is ordered behind it on the null
stream, so it provably ran while the gate was shut -- before its inputs existed.  The gate's length never decides a test: the canary does.
"""
import importlib

import numpy as np

qmg = importlib.import_module("quantum-mg_amd")

GATE_BYTES = 256 << 20     # each of the two gate buffers; one copy moves this many bytes
POISON8 = np.full(8, 0xFF, dtype=np.uint8)

_shared = {}


def _buffers():
    """The two gate buffers, the canary, the constant 1.0 and the two events; made once per process and kept."""
    if not _shared:
        _shared["a"] = qmg.DeviceArray.zeros(GATE_BYTES, np.uint8)
        _shared["b"] = qmg.DeviceArray.zeros(GATE_BYTES, np.uint8)
        _shared["canary"] = qmg.DeviceArray.from_host(POISON8)
        _shared["one"] = qmg.DeviceArray.from_host(np.ones(1, dtype=np.float64))
        _shared["ev"] = (qmg.event_create(), qmg.event_create())
        qmg.sync()
    return _shared


def copy_ms(st, reps=8):
    """Device time of one gate copy on `st` (synchronises `st`): what the number of copies of a gate of a given length is worked out from."""
    g = _buffers()
    e0, e1 = g["ev"]
    qmg.memcpy_d2d(g["b"], g["a"], GATE_BYTES, stream=st)     # first touch
    qmg.event_record(e0, stream=st)
    for _ in range(reps):
        qmg.memcpy_d2d(g["b"], g["a"], GATE_BYTES, stream=st)
    qmg.event_record(e1, stream=st)
    qmg.sync(st)
    return qmg.event_elapsed_ms(e0, e1) / reps


class Gate:
    """`copies` gate copies and then the canary on `st`.  One gate at a time: the buffers, the canary and the events are shared."""

    def __init__(self, st, copies):
        assert st, "the gate needs a created (non-blocking) stream: the null stream would order the canary read behind it"
        g = self.g = _buffers()
        self.st, self.copies = st, int(copies)
        qmg.memcpy_h2d(g["canary"], POISON8)          # synchronous, null stream; nothing is in flight on `st` between two gates
        e0, e1 = g["ev"]
        qmg.event_record(e0, stream=st)
        for _ in range(self.copies):
            qmg.memcpy_d2d(g["b"], g["a"], GATE_BYTES, stream=st)
        qmg.event_record(e1, stream=st)
        qmg.memcpy_d2d(g["canary"], g["one"], 8, stream=st)

    def closed(self):
        """True while the canary still holds the poison; a synchronous null-stream read that does not wait for `st`."""
        got = np.zeros(8, dtype=np.uint8)
        qmg.memcpy_d2h(got, self.g["canary"])
        return bool(np.array_equal(got, POISON8))

    def length_ms(self):
        """Device time between the gate's two events; call after `st` has been synchronised."""
        return qmg.event_elapsed_ms(*self.g["ev"])
