"""The harness of the stream-ordering tests (tests/test_stream_order_cases.py on the CPU tier, tests/test_gpu_stream_order.py on the GPU): decoys and the probe.

include/sjgpu.h promises that a device-resident entry point's work "is ordered with whatever else the caller enqueued" on the caller's stream.  A test that
hands over inputs that were complete long ago, on the NULL stream, and reads the outputs after a host wait cannot see a launch, a clear or a copy that went to
another stream.  late_call() below can: the inputs become real only behind a delay on a side stream, the NULL stream is kept busy for longer, the outputs are
consumed on the side stream without a host wait, and poison and decoys are written back behind the consumer.

DECOYS, NEVER GARBAGE.  A misordered read must give a wrong answer, never a wild address: what an input holds before the real bytes arrive is a valid input of
exactly the same shape.  For a document: the same length, every structural byte, quote and backslash at the same offset, other values (decoy_document).  For
rows of cells: the same tags, other value words (decoy_cells).  For inputs that hold only structure (a structural list, a document table) the decoy is the
product of the decoy document, and equals the real one.  Two calls take ANY bytes as valid input and answer with one bit that a value-only decoy cannot change
(the UTF-8 verdict, the quote parity); their decoys differ from the real input in one byte (break_utf8, flip_parity)."""
import math
import time

import numpy as np

POISON = 0x5A
SCRATCH_BYTES = 256 << 20
MIN_MS, MAX_MS, RETURN_FACTOR = 20.0, 200.0, 100


# ---- decoys ---------------------------------------------------------------------------------------------------------------------------------------
def string_masks(a):
    """-> (inside, escaped): bytes strictly between two unescaped quotes; bytes behind an escaping backslash"""
    a = np.asarray(a, np.uint8)
    n = len(a)
    at = np.arange(n, dtype=np.int64)
    bs = a == 0x5C
    starts = bs & ~np.concatenate([[False], bs[:-1]])
    run_start = np.maximum.accumulate(np.where(starts, at, 0))
    escaping = bs & (((at - run_start) & 1) == 0)  # the 1st, 3rd, ... backslash of a run escapes what follows it
    escaped = np.concatenate([[False], escaping[:-1]])
    quotes = (a == 0x22) & ~escaped
    inside = ((np.cumsum(quotes) & 1) == 1) & ~quotes
    return inside, escaped


def decoy_document(data):
    """The decoy of a document: ASCII digits 1..8 outside strings become the next digit; letters a..y / A..Y inside strings become the next letter, except the
    letter of an escape and the four hex digits behind a backslash-u.  Nothing else changes: same length, same structural bytes, quotes and backslashes."""
    a = np.ascontiguousarray(data, np.uint8)
    inside, escaped = string_masks(a)
    hexes = np.zeros(len(a) + 4, bool)
    for u in np.flatnonzero(escaped & (a == ord("u"))):
        hexes[u + 1: u + 5] = True
    hexes = hexes[: len(a)]
    letters = inside & ~escaped & ~hexes & (((a >= ord("a")) & (a <= ord("y"))) | ((a >= ord("A")) & (a <= ord("Y"))))
    digits = ~inside & (a >= ord("1")) & (a <= ord("8"))
    out = a.copy()
    out[letters | digits] += 1
    return out


def decoy_cells(values):
    """the decoy of rows of cells: the same tags go with these words -- every word differs, and every integer changes its sign (the census counts those)"""
    return np.ascontiguousarray(values, np.uint64) ^ np.uint64((1 << 63) | 1)


def break_utf8(data):
    """the document with the second byte of one multi-byte character, near the middle, replaced by 0xFF: the same length, not UTF-8"""
    a = np.ascontiguousarray(data, np.uint8).copy()
    cont = np.flatnonzero((a & 0xC0) == 0x80)
    a[cont[len(cont) // 2]] = 0xFF
    return a


def flip_parity(data):
    """the document with one blank outside a string, near the middle, replaced by a quote: the same length, one unescaped quote more"""
    a = np.ascontiguousarray(data, np.uint8).copy()
    inside, _ = string_masks(a)
    blanks = np.flatnonzero(~inside & (a == 0x20))
    a[blanks[len(blanks) // 2]] = 0x22
    return a


# ---- the delay ------------------------------------------------------------------------------------------------------------------------------------
class Delay:
    """Ordinary device work that keeps a stream busy: copies between two scratch tensors of 256 MiB (pair 0 for the NULL stream, pairs 1 and 2 for side streams).
    pass_ms: one copy, timed with events on an idle stream."""

    def __init__(self):
        import torch
        self.torch = torch
        self.pairs = [(torch.zeros(SCRATCH_BYTES, dtype=torch.uint8, device="cuda"), torch.zeros(SCRATCH_BYTES, dtype=torch.uint8, device="cuda")) for _ in range(3)]  # the NULL stream's, and one per side stream
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        passes = 8
        with torch.cuda.stream(s):
            self.pairs[1][1].copy_(self.pairs[1][0])
            e0.record(s)
            for _ in range(passes):
                self.pairs[1][1].copy_(self.pairs[1][0])
            e1.record(s)
        e1.synchronize()
        self.pass_ms = e0.elapsed_time(e1) / passes
        assert self.pass_ms > 0, f"a copy pass of {SCRATCH_BYTES >> 20} MiB measured {self.pass_ms} ms over {passes} passes: no delay can be built from it"

    def choose(self, return_s, only_enqueues):
        """the repetitions of a delay of at least 20 ms and at least 100 times the warm call's return time, at most 200 ms -> (count, what to say in a message).
        A call that waits for its stream returns after its device work; where 100 times that is more than 200 ms the delay is 200 ms (no gate is asserted
        for such a call).  A call that only enqueues must meet all three bounds."""
        want_ms = max(MIN_MS, RETURN_FACTOR * return_s * 1e3)
        capped = want_ms > MAX_MS
        if capped:
            assert not only_enqueues, f"a call that only enqueues took {return_s * 1e3:.3f} ms to return: no delay of at most {MAX_MS} ms is 100 times that"
            want_ms = MAX_MS
        count = max(1, int(math.ceil(want_ms / self.pass_ms)))
        if count * self.pass_ms > MAX_MS:
            count = max(1, int(MAX_MS / self.pass_ms))
        note = (f"[copy pass {self.pass_ms:.3f} ms, {count} passes = {count * self.pass_ms:.1f} ms of delay, the warm call returned in {return_s * 1e3:.3f} ms"
                f"{', capped at 200 ms' if capped else ''}]")
        return count, note

    def enqueue(self, stream, count, pair):
        src, dst = self.pairs[pair]
        with self.torch.cuda.stream(stream):
            for _ in range(count):
                dst.copy_(src, non_blocking=True)


def concurrent_stream(delay, beside=(), tries=16):
    """A side stream whose work runs beside the NULL stream's -- and beside that of every stream in `beside`, from which it is distinct.  The runtime maps its
    streams onto a few hardware queues, and two streams that share one run one after the other: a side stream behind the NULL stream's delay would make
    every probe inconclusive.  So: keep the other stream busy for 16 passes, give a candidate one pass, and take the first candidate that is done first."""
    import torch
    others = [torch.cuda.default_stream(), *beside]
    for _ in range(tries):
        s = torch.cuda.Stream()
        if any(s.cuda_stream == o.cuda_stream for o in others):
            continue
        ok = True
        for o in others:
            torch.cuda.synchronize()
            other_done, mine = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            delay.enqueue(o, 16, 0)
            other_done.record(o)
            delay.enqueue(s, 1, 1)
            mine.record(s)
            torch.cuda.synchronize()
            ok = ok and mine.elapsed_time(other_done) > 4 * delay.pass_ms
        if ok:
            return s
    raise AssertionError(f"no side stream out of {tries} ran beside the NULL stream{' and the other side stream' if beside else ''} [copy pass {delay.pass_ms:.3f} ms]")


# ---- inputs and cases -------------------------------------------------------------------------------------------------------------------------------
def _device(a, pad=0):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype.names:
        a = a.view(np.int32)
    if pad:
        a = np.concatenate([a, np.zeros(pad, a.dtype)])
    return torch.from_numpy(a.copy()).cuda()


class Late:
    """An input that becomes real late: `live` is what the call reads (it holds the decoy), `real` and `decoy` are device copies of the same shape.
    pad: elements of slack behind the array (zeros in all three: never empty, and nobody depends on them)."""

    def __init__(self, real, decoy=None, pad=0):
        real = np.ascontiguousarray(real)
        decoy = real if decoy is None else np.ascontiguousarray(decoy)
        assert real.shape == decoy.shape and real.dtype == decoy.dtype, "a decoy has exactly the real input's shape"
        self.count = real.size
        self.real, self.decoy = _device(real, pad), _device(decoy, pad)
        self.live = self.decoy.clone()

    @property
    def ptr(self):
        return self.live.data_ptr()


class Case:
    """One probed call.  inputs: Late objects.  outputs: device tensors the call writes and reads nothing of (poisoned before, kept after).  inouts: Late
    objects the call reads AND writes (kept after, never poisoned: poison must not be read as an input).  enqueue(stream) makes the library call and returns
    what it returned; finish(stream, ret), if given, fetches the outcome behind it (it may wait); check(ret, kept) compares -- kept: host copies of the
    outputs, then of the inouts, in order.  only_enqueues: the header says the call only enqueues -- the gate must still be closed when it returns."""

    def __init__(self, name, inputs, outputs, enqueue, check, finish=None, only_enqueues=False, inouts=()):
        self.name, self.inputs, self.outputs, self.inouts = name, list(inputs), list(outputs), list(inouts)
        self.enqueue, self.finish, self.check, self.only_enqueues = enqueue, finish, check, only_enqueues

    def run(self, stream):
        ret = self.enqueue(stream)
        return self.finish(stream, ret) if self.finish else ret


def poison(t):
    import torch
    t.view(torch.uint8).fill_(POISON)


def poisoned(count, dtype):
    """an output tensor of `count` elements (at least one: an address to pass), filled with poison"""
    import torch
    t = torch.empty(max(int(count), 1), dtype=dtype, device="cuda")
    poison(t)
    return t


def host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))


# ---- the probe --------------------------------------------------------------------------------------------------------------------------------------
def noted(note, what, *args):
    """what(*args); an assertion that fails inside it (a return code, the road taken) says the measured figures too"""
    try:
        return what(*args)
    except AssertionError as e:
        raise AssertionError(f"{e} {note}") from e


def late_calls(cases, streams, delay):
    """Probe case k on side stream k (torch.cuda.Streams; one case on one stream is late_call) -> [(what the call returned, the kept outputs on the host, the
    note for messages)].  All calls are enqueued before the outcome of any is fetched.
      1. warm up: every call at the same sizes on the default stream, waited for, twice; the second time the call itself (enqueue, not the fetch of its
         outcome) is timed.  The probed calls allocate nothing.  One delay for all: the longest any case asks for
      2. poison the outputs
      3. load the NULL stream with a delay -- one side-stream delay more than all side streams together, so that it outlasts their consumers (asserted)
      4. on each stream: a delay from the stream's own scratch pair, the event `gate`, the real inputs over the decoys
      5. the library call with that stream; then, when every call is made, the gates of the calls that only enqueue must still be closed
      6. the outcomes are fetched; still on each stream, no host wait: the outputs into `kept`, poison back over the outputs, decoys back over the inputs
      7. wait for the side streams, then for the NULL stream
    Work the library put on the NULL stream is stuck behind that stream's delay: its consumer sees poison.  Work put ahead of the caller's stream sees the
    decoy.  A read left for later sees the decoy (or the poison) of step 6."""
    import torch
    assert len(cases) == len(streams) <= len(delay.pairs) - 1
    null = torch.cuda.default_stream()
    everything = [i for c in cases for i in c.inputs + c.inouts]
    warm = f"[warming up; copy pass {delay.pass_ms:.3f} ms, no delay chosen yet]"
    for i in everything:
        i.live.copy_(i.decoy)
    torch.cuda.synchronize()
    for c in cases:
        noted(f"{c.name} {warm}", c.run, 0)
    torch.cuda.synchronize()
    chosen = []
    for c in cases:
        for i in c.inouts:
            i.live.copy_(i.decoy)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = noted(f"{c.name} {warm}", c.enqueue, 0)
        returned = time.perf_counter() - t0
        if c.finish:
            noted(f"{c.name} {warm}", c.finish, 0, ret)
        torch.cuda.synchronize()
        chosen.append((delay.choose(returned, c.only_enqueues)[0], returned, c))
    count, returned, slowest = max(chosen, key=lambda x: x[0])
    _, note = delay.choose(returned, slowest.only_enqueues)
    null_count = (len(cases) + 1) * count
    names = " + ".join(c.name for c in cases)
    note = f"{names} {note[:-1]}{' (of ' + slowest.name + ')' if len(cases) > 1 else ''}, {null_count} passes on the NULL stream]"
    watched = [c.outputs + [i.live for i in c.inouts] for c in cases]
    kept = [[torch.empty_like(o) for o in w] for w in watched]
    null_done = torch.cuda.Event(enable_timing=True)
    consumed = [torch.cuda.Event(enable_timing=True) for _ in cases]
    gates = [torch.cuda.Event() for _ in cases]
    for i in everything:
        i.live.copy_(i.decoy)
    for c in cases:
        for o in c.outputs:
            poison(o)
    torch.cuda.synchronize()
    delay.enqueue(null, null_count, 0)
    null_done.record(null)
    rets = []
    for k, (c, s) in enumerate(zip(cases, streams)):
        with torch.cuda.stream(s):
            delay.enqueue(s, count, 1 + k)
            gates[k].record(s)
            for i in c.inputs + c.inouts:
                i.live.copy_(i.real, non_blocking=True)
            rets.append(noted(note, c.enqueue, s.cuda_stream))
    gate_open = [c.name for c, g in zip(cases, gates) if c.only_enqueues and g.query()]
    for k, (c, s) in enumerate(zip(cases, streams)):
        with torch.cuda.stream(s):
            if c.finish:
                rets[k] = noted(note, c.finish, s.cuda_stream, rets[k])
            for dst, o in zip(kept[k], watched[k]):
                dst.copy_(o, non_blocking=True)
            consumed[k].record(s)
            for o in c.outputs:
                poison(o)
            for i in c.inputs + c.inouts:
                i.live.copy_(i.decoy, non_blocking=True)
    for s in streams:
        s.synchronize()
    null.synchronize()
    assert not gate_open, (f"the probe was NOT CONCLUSIVE: the gate of {gate_open} had opened when every call had returned, the inputs may have been real "
                           f"before the call was made {note}")
    for c, e in zip(cases, consumed):
        assert e.elapsed_time(null_done) > 0, f"the probe was NOT CONCLUSIVE: the NULL stream's delay ended before the outputs of {c.name} were consumed {note}"
    return [(ret, [host(x) for x in got], note) for ret, got in zip(rets, kept)]


def late_call(case, s, delay):
    """late_calls for one case on one side stream -> (what the call returned, the kept outputs on the host, the note for messages)"""
    return late_calls([case], [s], delay)[0]
