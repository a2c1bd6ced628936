"""The gate harness of tests/test_gpu_streams.py: does an entry point enqueue ALL its device work on the caller's stream, and does it
return without waiting for that stream?  (A plain helper module, no tests in it.)

The construction replaces racing by ordering.  S is a NON-BLOCKING side stream (checked with hipStreamGetFlags: a NULL-stream launch is
not ordered with it).  With everything synchronised, the handles and the input tensors of a call hold a valid state A.  Then, on S and in
this order: the gate (GATE_MIN_MS .. GATE_MAX_MS of ordinary torch work, measured once per session), device-to-device copies that replace
A by a second valid state B (sgx_copy_envs from a snapshot for records, Tensor.copy_ for tensors: nothing comes from pageable host memory,
which would stall the host behind the gate), and the call under test.  A launch, memset or copy of the call that left S runs while the
gate still holds S back, on A, or at least before the copies: it computes from stale but VALID data, and its result differs from the
twin's -- the same handles brought to B and run through the same call on the default stream in the ordinary way.  The comparison is byte
for byte over every output tensor and sgx_export_state of every handle the call writes.

No gated call ever sees anything but valid state, and no output of a gated call is used as an index or an action before it has been
compared: a failing case is a wrong byte, never a fault.

Right after the call returns the harness notes whether S still has work pending (the gate has not even finished: the call did not wait)
and the call's host time; run_case asserts both for every entry point the header does not list as waiting.  The CONTROL run hands the
call the NULL stream while the preparation stays on S: the harness must then see a mismatch, which shows that A and B are
distinguishable for that call and that the gate held.  A case whose control passes is a defect of the test.
"""
import contextlib
import ctypes as C
import functools
import math
import time
from types import SimpleNamespace

import torch

from stratego_env_amd import _lib
from stratego_env_amd.vec_env import VecStrategoEnv

SEED, OFFSET = 0x5EED5712EA, 4000
GATE_MIN_MS, GATE_MAX_MS, GATE_TARGET_MS = 20.0, 200.0, 60.0
STEPS_A, STEPS_B = 10, 25
HIP_STREAM_NON_BLOCKING = 0x01
POISON = 0x5A


@functools.lru_cache(None)
def hip():
    return C.CDLL('libamdhip64.so')


def current_device():
    cur = C.c_int(-1)
    assert hip().hipGetDevice(C.byref(cur)) == 0
    return cur.value


def stream_ptr(stream):
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def is_non_blocking(stream):
    flags = C.c_uint(0)
    assert hip().hipStreamGetFlags(C.c_void_p(stream.cuda_stream), C.byref(flags)) == 0
    return bool(flags.value & HIP_STREAM_NON_BLOCKING)


class Gate:
    """The side streams and the gate: `reps` in-place additions over a 1 GiB tensor, sized once so that they keep a stream busy for about
    GATE_TARGET_MS, then measured with HIP events (`ms`) and held to [GATE_MIN_MS, GATE_MAX_MS]."""

    def __init__(self):
        self.buf = torch.zeros(1 << 28, dtype=torch.float32, device='cuda')
        self.probe = torch.zeros(64, dtype=torch.float32, device='cuda')
        self.S = torch.cuda.Stream()
        self.reps = 4
        unit = self._time() / self.reps                            # (first launch: code loading; timed again below)
        unit = self._time() / self.reps
        self.reps = max(1, min(4000, int(math.ceil(GATE_TARGET_MS / max(unit, 1e-3)))))
        # Streams share a few hardware queues, and two streams on one queue run in submission order whatever their flags say.  S must be a
        # stream that is non-blocking AND overtaken by the NULL stream in fact: NULL-stream work submitted behind the gate finishes while
        # the gate still runs.
        for _ in range(8):
            if is_non_blocking(self.S) and self._null_stream_overtakes():
                break
            self.S = torch.cuda.Stream()
        assert is_non_blocking(self.S), "the side stream is blocking: a NULL-stream launch would be ordered with it and the gate would prove nothing"
        assert self._null_stream_overtakes(), "no side stream found that the NULL stream overtakes: the gate would prove nothing"
        self.S2 = torch.cuda.Stream()
        assert is_non_blocking(self.S2)
        self.ms = self._time()
        assert GATE_MIN_MS <= self.ms <= GATE_MAX_MS, "the gate took %.1f ms, outside [%g, %g]" % (self.ms, GATE_MIN_MS, GATE_MAX_MS)

    def _null_stream_overtakes(self):
        torch.cuda.synchronize()
        self.run(self.S)
        self.probe.add_(1.0)                                       # the default stream is the NULL stream
        done = torch.cuda.Event()
        done.record(torch.cuda.default_stream())
        done.synchronize()
        overtook = not self.S.query()
        torch.cuda.synchronize()
        return overtook

    def run(self, stream):
        with torch.cuda.stream(stream):
            for _ in range(self.reps):
                self.buf.add_(1.0)

    def _time(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(self.S)
        self.run(self.S)
        e1.record(self.S)
        self.S.synchronize()
        return e0.elapsed_time(e1)


@functools.lru_cache(None)
def gate():
    return Gate()


def new_env(name, n, **kw):
    return VecStrategoEnv(name, n, seed=SEED, env_id_offset=OFFSET, auto_reset=True, placement='plain', **kw)


@functools.lru_cache(None)
def material(name, n):
    """The two valid states of n games of a variant, each as a snapshot pool and as the tensors calls take as inputs.  A: reset() and
    STEPS_A rollout steps; B: two resets (another game number) and STEPS_B steps.  Everything is made by the library on the default stream
    (the path the parity suites pin to the oracle) and is never written again."""
    M = SimpleNamespace(name=name, n=n, snap={}, obs={}, mask={}, act={}, player={}, state={}, maps={}, info={})
    e = M.env = new_env(name, n)
    M.L = e._L
    for X, resets, steps in (('A', 1, STEPS_A), ('B', 2, STEPS_B)):
        for _ in range(resets):
            e.reset()
        st, _ = e.export_state()
        M.maps[X] = (st[:, 0].to(torch.int8).reshape(n, -1).contiguous(), st[:, 1].flip(1, 2).to(torch.int8).reshape(n, -1).contiguous())
        e.rollout_steps(steps)
        e.observe()
        e.sample_valid_actions()
        M.snap[X] = e.snapshot()
        M.obs[X], M.mask[X], M.act[X], M.player[X] = e.obs.clone(), e.mask.clone(), e.next_actions.clone(), e.player.clone()
        M.state[X] = tuple(t.clone() for t in e.export_state())
        M.info[X] = e.env_info().clone()
    torch.cuda.synchronize()
    return M


def perm(n, k, c):
    """A permutation i -> (i * m + c) % n of range(n), m the first multiplier >= k coprime to n, as an int32 device tensor."""
    m = k
    while math.gcd(m, n) != 1:
        m += 1
    return ((torch.arange(n, device='cuda', dtype=torch.int64) * m + c) % n).to(torch.int32)


class Case:
    """What one call touches.  handles: (env, {'A': pool, 'B': pool}, staged, compared) -- a staged handle is brought from A to B on the
    side stream behind the gate, one that is not holds A in every run (a call's destination); inputs: (live tensor, its A value, its B
    value); outputs: tensors the call writes.  call(stream pointer, torch stream); warm(): optional, an earlier, ungated call the case
    needs (it runs on the default stream in every preparation, on the state being prepared, which is then loaded afresh)."""

    def __init__(self, M):
        self.M, self.handles, self.inputs, self.outputs, self.keep = M, [], [], [], []
        self.call = self.warm = None

    def env(self, staged=True, compared=True, n=None, **kw):
        e = new_env(self.M.name, n or self.M.n, **kw)
        return self.handle(e, staged, compared)

    def pool(self, staged=False, compared=True):
        return self.env(staged, compared, human_inits=False, outputs=False)

    def handle(self, e, staged=True, compared=True):
        self.handles.append((e, self.M.snap, staged, compared))
        return e

    def inp(self, a, b):
        live = a.clone()
        self.inputs.append((live, a, b))
        return live

    def out(self, *tensors):
        self.outputs.extend(tensors)
        return tensors[0] if len(tensors) == 1 else tensors

    def new(self, shape, dtype):
        return self.out(torch.empty(shape, dtype=dtype, device='cuda'))

    def close(self):
        for e, _, _, _ in self.handles:
            e.close()


def _bytes(t):
    return t.reshape(-1).view(torch.uint8)


def _load(case, X, stream=None, staged_only=False):
    L, sp = case.M.L, stream_ptr(stream)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        for e, snaps, staged, _ in case.handles:
            if staged or not staged_only:
                _lib.check(L.sgx_copy_envs(e._h, None, snaps[X if staged else 'A']._h, None, e.num_envs, sp), L)
        for live, a, b in case.inputs:
            live.copy_(a if X == 'A' else b)


def _prepare(case, X):
    if case.warm:
        _load(case, X)
        case.warm()
    in_out = {live.data_ptr() for live, _, _ in case.inputs}
    for t in case.outputs:
        if t.data_ptr() not in in_out:
            _bytes(t).fill_(POISON)
    _load(case, X)
    torch.cuda.synchronize()


def _collect(case):
    torch.cuda.synchronize()
    got = [_bytes(t).clone() for t in case.outputs]
    for e, _, _, compared in case.handles:
        if compared:
            got.extend(_bytes(t) for t in e.export_state())
    torch.cuda.synchronize()
    return got


def mismatches(got, want):
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if not torch.equal(g, w)]


def twin(case):
    """The ordinary run: state B, the call on the default stream."""
    _prepare(case, 'B')
    case.call(None, torch.cuda.default_stream())
    return _collect(case)


def gated(case, on_side_stream=True):
    """State A; then on S: the gate, the copies A -> B, the call (on S, or -- the control -- on the NULL stream).
    -> (results, S still pending when the call returned, the call's host seconds)."""
    G = gate()
    _prepare(case, 'A')
    home = current_device()
    G.run(G.S)
    _load(case, 'B', G.S, staged_only=True)
    sp, s = (stream_ptr(G.S), G.S) if on_side_stream else (None, torch.cuda.default_stream())
    t0 = time.perf_counter()
    case.call(sp, s)
    host = time.perf_counter() - t0
    pending = not G.S.query()
    assert current_device() == home, "the call changed the caller's current device"
    G.S.synchronize()
    return _collect(case), pending, host


def run_case(case, may_wait=False, label=''):
    """Twin, gated run, control.  Asserts the contract and returns (host seconds, pending) of the gated run."""
    G = gate()
    try:
        want = twin(case)                                          # (also the warm-up: same shapes, first-use allocations, code loading)
        got, pending, host = gated(case)
        print("STREAMS %-44s host %8.1f us  pending %d  gate %.1f ms" % (label, host * 1e6, pending, G.ms))
        if not may_wait:
            assert host * 1e3 < G.ms / 4, "%s: the call took %.2f ms on the host, the gate is %.1f ms: it waited, or the gate is too short to order anything" % (label, host * 1e3, G.ms)
            assert pending, "%s: the side stream had drained when the call returned: the call waited for the device" % label
        bad = mismatches(got, want)
        assert not bad, "%s: results %s differ from the twin's: some of the call's work did not run on the caller's stream behind its inputs" % (label, bad)
        ctl, _, _ = gated(case, on_side_stream=False)
        assert mismatches(ctl, want), "%s: the control (the call on the NULL stream) matched the twin: the case cannot tell A from B, or the gate did not hold" % label
        return host, pending
    finally:
        torch.cuda.synchronize()
        case.close()
