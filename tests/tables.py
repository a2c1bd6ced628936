"""Weight tables of the weighted playouts and belief tables of the weighted determinization that the CPU and the GPU tests share (support
code, no tests)."""
import collections
import ctypes as C
import functools

import numpy as np

from tests import determinize_weighted_rule as dwr, weighted_playout_rule as wr
from tests.pool_roots import fives_position

N_DRAWS = 65536


def third_zero_table(seed=0):
    """A seeded random table, values to 4095, about 30 % of the entries 0 (the GPU test uses the same)."""
    rs = np.random.RandomState(seed)
    w = rs.randint(1, 4096, size=wr.SHAPE)
    w[rs.random_sample(wr.SHAPE) < 0.3] = 0
    return w.astype(np.uint16)


def attacks_only_table():
    """Weight 5 for a move onto an occupied cell (a known type, or unknown), 0 for a move onto an empty one."""
    w = np.zeros(wr.SHAPE, dtype=np.uint16)
    w[:, :, 1:] = 5
    return w


def forward_only_table():
    """[8, 1, 1, 1] by direction"""
    w = np.ones(wr.SHAPE, dtype=np.uint16)
    w[0] = 8
    return w


def _p16(w):
    return w.ctypes.data_as(C.POINTER(C.c_uint16))


TABLES = {'random': third_zero_table(0), 'attacks': attacks_only_table(), 'forward': forward_only_table()}


def third_zero_belief(cells, seed=0, shape=None):
    """A seeded random table, values to 4095, a third of the entries 0 (the GPU test uses the same)."""
    rs = np.random.RandomState(seed)
    shape = (2, 12, cells) if shape is None else shape
    w = rs.randint(1, 4096, size=shape)
    w[rs.random_sample(shape) < 1.0 / 3.0] = 0
    return w.astype(np.uint16)


def one_hot_truth(state):
    """Weight 1 exactly where a piece of that type stands, for both players."""
    cells = state.shape[1] * state.shape[2]
    w = np.zeros((2, 12, cells), dtype=np.uint16)
    for p in range(2):
        flat = state[p].reshape(-1)
        for c in np.flatnonzero(flat):
            w[p, flat[c] - 1, c] = 1
    return w


def skewed_fives_table():
    """The table of the distribution test on fives_position() (hidden cells 0, 1, 2, 3 never moved and 9 moved; types 4, 5, 6, 7, flag):
    uneven weights with zeros on the hidden cells -- the flag never on cell 1 where it truly stands, the 6 never on cell 1, the 5 never on
    cell 3 -- chosen on the CPU so that the worlds of expected count below 5 hold less than 5 % of the mass; elsewhere a seeded third-zero
    filling that the position never reads."""
    w = third_zero_belief(25, seed=3).astype(np.int64)
    hid = [0, 1, 2, 3, 9]
    w[1][11 - 1][hid] = [800, 0, 300, 1, 4095]          # (cell 9 has moved: the flag's weight there is never read; cell 3: the rare worlds)
    w[1][7 - 1][hid] = [1, 2, 3, 4, 5]
    w[1][6 - 1][hid] = [5, 0, 1, 2, 2]
    w[1][5 - 1][hid] = [1, 1, 1, 0, 3]
    w[1][4 - 1][hid] = [0, 0, 0, 0, 0]                  # the last instance dealt: one cell is left, whatever it weighs (off_belief counts it)
    return w.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def fives_samples(kind):
    """65,536 worlds of fives_position() for slots 0 .. 65,535 of seed 0, draw 0, with the constant table ('constant': every entry 7) or
    skewed_fives_table() ('skewed') -> (layers int64 [N, 25], off_belief int32 [N]).  Read-only: shared by the tests."""
    st, _ = fives_position()
    table = np.full((2, 12, 25), 7, dtype=np.uint16) if kind == 'constant' else skewed_fives_table()
    layers, off = dwr.sample_layers(st, 1, 1, table, 0, np.arange(N_DRAWS), 0)
    layers.setflags(write=False)
    off.setflags(write=False)
    return layers, off


def chi2_against(layers, probs):
    """Pearson's chi-squared of the sampled worlds against the exact probabilities {layer bytes: Fraction}: every world of expected count
    >= 5 a cell of its own, the others pooled into one.  -> (statistic, degrees of freedom, pooled mass, worlds seen that have
    probability 0)."""
    counts = collections.Counter(row.tobytes() for row in layers)
    n = len(layers)
    impossible = sum(c for k, c in counts.items() if probs.get(k, 0) == 0)
    stat, cells_used, pooled_p, pooled_c = 0.0, 0, 0.0, 0
    for k, p in probs.items():
        e = float(p) * n
        if e >= 5.0:
            stat += (counts.get(k, 0) - e) ** 2 / e
            cells_used += 1
        else:
            pooled_p += float(p)
            pooled_c += counts.get(k, 0)
    if pooled_p > 0:
        stat += (pooled_c - pooled_p * n) ** 2 / (pooled_p * n)
        cells_used += 1
    return stat, cells_used - 1, pooled_p, impossible
