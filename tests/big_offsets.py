"""Helper of tests/test_gpu_big_offsets.py: arenas of several GiB, the games that straddle 2^31 / 2^32 bytes and 2^31 elements, witness
chunks and the memory gate.  (No torch import at module level: tests/test_big_offsets_cpu.py holds the arithmetic without a GPU.)

THE WITNESS.  Every draw is keyed by the global env id, so games [k, k + m) of a handle of N games with env_id_offset 0
produce, byte for byte, what a handle of m games with env_id_offset k produces for the same seed, variant, settings and calls.  The small
handle writes at low offsets -- where the parity suites hold it against the oracle -- and is compared on the device with torch.equal.

THE ARENA.  front guard | payload | 4 KiB back guard, the two NaN words of tests/test_gpu_guard_bands.py.  The front guard turns a wrong
offset into a wrong byte instead of a fault: a product truncated to uint32 lands inside the payload, one sign-extended from int32 at most
2 GiB before it, a 32-bit element index of a 4-byte type at most 8 GiB before it."""
import collections

import numpy as np

GUARD = 4096
GUARD_INT = 0x7FC0DEAD                        # float32 NaN; bytes AD DE C0 7F
POISON_INT = 0x7FA55A5A                       # another one; bytes 5A 5A A5 7F
POISON_BYTES = (0x5A, 0x5A, 0xA5, 0x7F)
GIB = 1 << 30
FRONT_4G = 2 * GIB + GUARD                    # the 4 GiB cases: uint32 truncation, int32 sign extension
FRONT_8G = 8 * GIB + GUARD                    # the 8 GiB cases: a 32-bit element index of a 4-byte type
MAX_HELD = 24 * GIB                           # no test may hold more at once: the machines are shared
HEADROOM = 2 * GIB
_SCAN_WORDS = 1 << 27                         # words per comparison: temporaries of at most 128 MiB of bool

Thresholds = collections.namedtuple('Thresholds', 'b31 b32 e31')


def thresholds(bytes_per_game, item=4):
    """The games that hold byte 2^31, byte 2^32 and element 2^31 (of `item` bytes) of a dense [N, bytes_per_game] tensor: game g covers
    bytes [g * bytes_per_game, (g + 1) * bytes_per_game).  A batch has to be LARGER than the index to reach the boundary."""
    bpg, item = int(bytes_per_game), int(item)
    assert bpg > 0 and item > 0 and bpg % item == 0
    return Thresholds((1 << 31) // bpg, (1 << 32) // bpg, ((1 << 31) * item) // bpg)


def straddlers(n, bytes_per_game, item=4):
    """Sorted games of a batch of n worth an oracle anchor: first, last, and the ones at thresholds() with their left neighbours
    (the neighbour's last byte is the last one below the boundary)."""
    th = thresholds(bytes_per_game, item)
    out = {0, n - 1}
    for g in th:
        for x in (g - 1, g):
            if 0 <= x < n:
                out.add(x)
    return sorted(out)


def witness_chunks(n, chunk, every=1, keep=()):
    """[(k, m)]: the batch [0, n) in witnesses of `chunk` games (the last one shorter).  every > 1: only every `every`-th chunk plus all
    chunks that hold a game of `keep` (reduced coverage, stated by the caller)."""
    n, chunk = int(n), int(chunk)
    assert n > 0 and chunk > 0 and every >= 1
    out = []
    for i, k in enumerate(range(0, n, chunk)):
        m = min(chunk, n - k)
        if i % every == 0 or any(k <= g < k + m for g in keep):
            out.append((k, m))
    return out


def gate(need_bytes, device=0):
    """The memory gate: a test states what it holds at once, witnesses included.  Skips (with the figures) when the device has less than
    that + 2 GiB free; a need above 24 GiB is a mistake in the test."""
    import pytest
    import torch
    need = int(need_bytes)
    assert need <= MAX_HELD, "a test may hold at most 24 GiB at once, this one states %.1f GiB" % (need / GIB)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(device)
    print("memory gate: need %.2f GiB, free %.2f of %.2f GiB" % (need / GIB, free / GIB, total / GIB))
    if free < need + HEADROOM:
        pytest.skip("needs %.2f GiB + 2 GiB headroom of device memory, %.2f GiB free" % (need / GIB, free / GIB))
    return free


def release():
    """after the `del`s of a test: give the arenas back to the device (other tenants, the next test)"""
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


class BigArena:
    """front guard | payload | back guard in one uint8 device tensor.  `t` is the payload as a tensor of `dtype` and `shape`; rows are
    shape[0].  Filled with int32 fills (no arange of the whole length); every check works on bounded pieces."""

    def __init__(self, name, shape, dtype, front_guard_bytes=FRONT_4G, device='cuda'):
        import torch
        self.name, self.shape, self.dtype = name, tuple(int(x) for x in shape), dtype
        self.item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.item
        self.row_bytes = self.nbytes // self.shape[0]
        self.front = int(front_guard_bytes)
        assert self.front % GUARD == 0 and self.front >= GUARD
        self.span = (self.nbytes + 15) & ~15                      # the pad behind the payload keeps the poison: part of the back guard
        self.total = self.front + self.span + GUARD
        raw = torch.empty(self.total + 1024, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % 1024
        self.buf = raw[off:off + self.total]
        del raw
        self.words = self.buf.view(torch.int32)
        self.lo, self.hi = self.front, self.front + self.nbytes
        self.words[:self.front // 4].fill_(GUARD_INT)
        self.words[(self.front + self.span) // 4:].fill_(GUARD_INT)
        self._pat = torch.tensor(POISON_BYTES, dtype=torch.uint8, device=device).repeat(5)
        self.t = self.buf[self.lo:self.hi].view(dtype).view(self.shape)
        assert self.t.data_ptr() % 1024 == 0
        self.poison()

    @property
    def held(self):
        return self.total + 1024

    def poison(self):
        self.words[self.front // 4:(self.front + self.span) // 4].fill_(POISON_INT)

    # ---- bounded scans ----------------------------------------------------------------------------------------------------------
    def _words_differ(self, w0, w1, value):
        """number of int32 words of buf[4 w0 : 4 w1) that are not `value` (a device scalar; no synchronisation)"""
        import torch
        bad = torch.zeros((), dtype=torch.int64, device=self.buf.device)
        for a in range(w0, w1, _SCAN_WORDS):
            bad += (self.words[a:min(a + _SCAN_WORDS, w1)] != value).sum()
        return bad

    def _first_word(self, w0, w1, value, equal):
        import torch
        for a in range(w0, w1, _SCAN_WORDS):
            w = self.words[a:min(a + _SCAN_WORDS, w1)]
            hit = torch.nonzero((w == value) if equal else (w != value))
            if hit.numel():
                return a + int(hit[0])
        return None

    def check_guards(self, what=''):
        import pytest
        f4, p4, t4 = self.front // 4, (self.front + self.span) // 4, self.total // 4
        tail_a = -(-self.hi // 4)                                 # the pad behind the payload (whole words of it) keeps the poison
        bad = int(self._words_differ(0, f4, GUARD_INT) + self._words_differ(p4, t4, GUARD_INT) + self._words_differ(tail_a, p4, POISON_INT))
        if bad == 0:
            return
        w = self._first_word(0, f4, GUARD_INT, False)
        if w is None:
            w = self._first_word(tail_a, p4, POISON_INT, False)
        if w is None:
            w = self._first_word(p4, t4, GUARD_INT, False)
        rel = 4 * w - self.lo
        pytest.fail("%s: %s: %d guard words overwritten, the first at payload-relative byte %d (payload is %d bytes, %d per row; negative = "
                    "before it: row %d counted back from the payload)" % (what, self.name, bad, rel, self.nbytes, self.row_bytes, rel // self.row_bytes))

    def _rows(self, rows):
        a, b = (0, self.shape[0]) if rows is None else (int(rows[0]), int(rows[1]))
        assert 0 <= a <= b <= self.shape[0]
        return a, b

    def poison_words(self, rows=None):
        """how many whole int32 words of the rows [a, b) still hold the poison (device scalar).  No tensor of this suite can hold that
        word as data: it is a NaN as float32, out of range as an action, and no mask / flag / player byte is 0x5A, 0xA5 or 0x7F."""
        import torch
        a, b = self._rows(rows)
        w0, w1 = -(-(self.lo + a * self.row_bytes) // 4), (self.lo + b * self.row_bytes) // 4
        n = torch.zeros((), dtype=torch.int64, device=self.buf.device)
        for s in range(w0, w1, _SCAN_WORDS):
            n += (self.words[s:min(s + _SCAN_WORDS, w1)] == POISON_INT).sum()
        return n

    def check_written(self, what='', rows=None):
        import pytest
        left = int(self.poison_words(rows))
        if left:
            a, b = self._rows(rows)
            w0, w1 = -(-(self.lo + a * self.row_bytes) // 4), (self.lo + b * self.row_bytes) // 4
            rel = 4 * self._first_word(w0, w1, POISON_INT, True) - self.lo
            pytest.fail("%s: %s: %d words of rows [%d, %d) still hold the poison, the first in row %d at byte %d of it (payload byte %d)"
                        % (what, self.name, left, a, b, rel // self.row_bytes, rel % self.row_bytes, rel))

    def unwritten(self, rows):
        """True when EVERY byte of the rows [a, b) still holds the poison (byte exact: ranges need not be word aligned)"""
        import torch
        a, b = self._rows(rows)
        ba, bb = self.lo + a * self.row_bytes, self.lo + b * self.row_bytes
        if ba == bb:
            return True
        wa, wb = -(-ba // 4) * 4, bb // 4 * 4
        if wa >= wb:
            return bool(torch.equal(self.buf[ba:bb], self._pat[ba % 4:ba % 4 + bb - ba]))
        ok = torch.equal(self.buf[ba:wa], self._pat[ba % 4:ba % 4 + wa - ba]) and torch.equal(self.buf[wb:bb], self._pat[:bb - wb])
        return bool(ok) and int(self._words_differ(wa // 4, wb // 4, POISON_INT)) == 0

    def check_unwritten(self, what, rows):
        import pytest
        if not self.unwritten(rows):
            a, b = self._rows(rows)
            w = self._first_word(-(-(self.lo + a * self.row_bytes) // 4), (self.lo + b * self.row_bytes) // 4, POISON_INT, False)
            rel = (4 * w - self.lo) if w is not None else (a * self.row_bytes)
            pytest.fail("%s: %s: rows [%d, %d) must keep the poison, row %d was written (payload byte %d)" % (what, self.name, a, b, rel // self.row_bytes, rel))


def assert_rows_equal(big, small, k, what):
    """big[k : k + m] == small, exactly (torch.equal on the raw bits: NaNs and the sign of zero count); a failure names the first game"""
    import torch
    m = small.shape[0]
    a, b = big[k:k + m], small
    assert a.shape == b.shape and a.dtype == b.dtype, (what, tuple(a.shape), tuple(b.shape))
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    if not torch.equal(a, b):
        g = k + int(torch.nonzero((a.reshape(m, -1) != b.reshape(m, -1)).any(dim=1))[0])
        row_bytes = int(np.prod(big.shape[1:], dtype=np.int64)) * big.element_size()
        raise AssertionError("%s: differs from the witness, first at game %d (its bytes start at %d = 2^31 %+d = 2^32 %+d)"
                             % (what, g, g * row_bytes, g * row_bytes - (1 << 31), g * row_bytes - (1 << 32)))
