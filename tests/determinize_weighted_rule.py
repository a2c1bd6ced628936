"""The belief-weighted determinization rule (sgx_determinize_weighted) restated in numpy on the reference's int64 [34,R,C]
states: what the device kernel must reproduce bit for bit.  Test infrastructure (it imports oracle/ for the counter RNG); never imported
by the product package.

For a state, its mover, an observer (0 = the mover) and a table uint16 [2][12][cells], with `opp` the observer's opponent:
  H = cells with an opp piece whose public layer says 13, ascending; A = those of H never moved, B = the rest (determinize_rule.hidden_lists);
  c_t = the number of true type t on H;
  a flag or a bomb on a cell of B cannot come from play: the state is returned unchanged with hidden = -1, off_belief = 0;
  w(t, c) = min(table[opp][t - 1][c], 4095) with c the ABSOLUTE cell;
  the types are dealt in the order 11, 12, 10, 9, ..., 1, each its c_t instances one after the other, a counter j = 0, 1, ... running over
  the whole deal; free = H; for the instance of type t with counter j:
    candidates c_0 < ... < c_{m-1} = free & A for t in (11, 12), else free;  W = sum of w(t, c_k);
    r = rng(seed, g, draw, 7, j);
    W > 0:  x = rng_below(r, W), the cell is the first c_k whose inclusive prefix sum exceeds x;
    W == 0: the cell is c_{rng_below(r, m)}, off_belief += 1;
    pieces[opp][cell] = t; the cell leaves free;
  hidden = |H|.
Only the opponent's pieces layer changes."""
from fractions import Fraction

import numpy as np

from oracle import oracle as orc
from tests.determinize_rule import BOMB, FLAG, L_PIECES, chi2_quantile_999, hidden_lists  # noqa: F401  (re-exported for the tests)

STREAM_DETERMINIZE_WEIGHTED = 7
WEIGHT_MAX = 4095
TYPE_ORDER = (11, 12, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1)


def _lists(state, mover, observer):
    """-> (opp, H ascending, A as a set, the instance sequence [t, ...] in dealing order, inconsistent?)."""
    opp, A, B, I, M = hidden_lists(state, mover, observer)
    pieces = state[L_PIECES + opp].reshape(-1)
    H = sorted(A + B)
    types = [int(pieces[c]) for c in H]
    seq = [t for t in TYPE_ORDER for _ in range(types.count(t))]
    bad = any(pieces[c] in (FLAG, BOMB) for c in B)
    return opp, H, set(A), seq, bad


def _weights(table, opp, cells):
    t = np.asarray(table).reshape(2, 12, cells)
    return np.minimum(t[opp].astype(np.int64), WEIGHT_MAX)              # [12][cells]


def determinize_weighted(state, mover, observer, table, seed, g, draw):
    """One state int64 [34,R,C] -> (the sampled world, number of hidden cells or -1, off_belief)."""
    state = np.asarray(state, dtype=np.int64)
    out = state.copy()
    opp, H, A, seq, bad = _lists(state, mover, observer)
    if bad:
        return out, -1, 0
    cells = state.shape[1] * state.shape[2]
    w = _weights(table, opp, cells)
    flat = out[L_PIECES + opp].reshape(-1)                              # (a view: the layer is contiguous)
    free = list(H)
    off = 0
    rows = {}
    for j, t in enumerate(seq):
        if t not in rows:
            rows[t] = w[t - 1].tolist()
        cand = [c for c in free if c in A] if t in (FLAG, BOMB) else free
        ws = [rows[t][c] for c in cand]
        W = sum(ws)
        r = orc.rng(seed, g, draw, STREAM_DETERMINIZE_WEIGHTED, j)
        if W > 0:
            x = orc.rng_below(r, W)
            acc = 0
            for c, wc in zip(cand, ws):
                acc += wc
                if acc > x:
                    cell = c
                    break
        else:
            cell = cand[orc.rng_below(r, len(cand))]
            off += 1
        flat[cell] = t
        free.remove(cell)
    return out, len(H), off


def determinize_weighted_batch(states, movers, observer, tables, seed, env_id_offset, draw, src_index=None):
    """Slot i <- determinize_weighted(states[s], ..., table of record s) with s = src_index[i], g = env_id_offset + i, like the device call.
    tables: [2, 12, cells] (one for all: stride 0) or [n_src, 2, 12, cells] (indexed by s)."""
    states = np.asarray(states, dtype=np.int64)
    tables = np.asarray(tables)
    idx = np.arange(len(states)) if src_index is None else np.asarray(src_index, dtype=np.int64)
    out = np.empty((len(idx),) + states.shape[1:], dtype=np.int64)
    hidden = np.empty(len(idx), dtype=np.int32)
    off = np.empty(len(idx), dtype=np.int32)
    for i, s in enumerate(idx):
        tb = tables if tables.ndim == 3 else tables[s]
        out[i], hidden[i], off[i] = determinize_weighted(states[s], int(movers[s]), observer, tb, seed, env_id_offset + i, draw)
    return out, hidden, off


def sample_layers(state, mover, observer, table, seed, g, draw):
    """determinize_weighted of ONE state for an array of slots g (int array [N]), vectorised over the slots with the array form of the
    counter RNG (tests/draw_stats.py): -> (the opponent's pieces layer of every world, int64 [N, cells]; off_belief int32 [N]).
    tests/test_determinize_weighted_cpu.py holds it against the scalar function above."""
    from tests import draw_stats as ds
    state = np.asarray(state, dtype=np.int64)
    opp, H, A, seq, bad = _lists(state, mover, observer)
    assert not bad
    g = np.asarray(g, dtype=np.int64)
    N, nh = len(g), len(H)
    cells = state.shape[1] * state.shape[2]
    w = _weights(table, opp, cells)[:, H]                                # [12][|H|]
    in_A = np.asarray([c in A for c in H], dtype=bool)
    free = np.ones((N, nh), dtype=bool)
    got = np.zeros((N, nh), dtype=np.int64)
    off = np.zeros(N, dtype=np.int32)
    rows = np.arange(N)
    for j, t in enumerate(seq):
        cand = free & in_A[None, :] if t in (FLAG, BOMB) else free
        ws = np.where(cand, w[t - 1][None, :], 0)
        W = ws.sum(axis=1)
        r = ds.np_rng(seed, g, draw, STREAM_DETERMINIZE_WEIGHTED, j)
        fallback = W == 0
        x = ds.np_rng_below(r, np.where(fallback, cand.sum(axis=1), W))
        cum = np.where(fallback[:, None], np.cumsum(cand, axis=1), np.cumsum(ws, axis=1))
        pick = np.argmax(cum > x[:, None], axis=1)
        assert cand[rows, pick].all()
        got[rows, pick] = t
        free[rows, pick] = False
        off += fallback
    layers = np.tile(state[L_PIECES + opp].reshape(-1), (N, 1))
    layers[:, H] = got
    return layers, off


def world_probabilities(state, mover, observer, table):
    """The EXACT distribution of the rule over worlds, {bytes of the opponent's pieces layer: Fraction}, by enumerating the instance
    sequences (a draw from rng_below(r, W) with r uniform takes candidate k with probability w_k / W up to 2^-32; the fallback is
    uniform over the candidates).  Exponential in the number of hidden cells: at most 7."""
    state = np.asarray(state, dtype=np.int64)
    opp, H, A, seq, bad = _lists(state, mover, observer)
    assert not bad and len(H) <= 7
    cells = state.shape[1] * state.shape[2]
    w = _weights(table, opp, cells)
    base = state[L_PIECES + opp].reshape(-1).copy()
    worlds = {}

    def deal(j, free, assign, p):
        if j == len(seq):
            layer = base.copy()
            for c, t in assign:
                layer[c] = t
            key = layer.tobytes()
            worlds[key] = worlds.get(key, Fraction(0)) + p
            return
        t = seq[j]
        cand = [c for c in free if c in A] if t in (FLAG, BOMB) else list(free)
        ws = [int(w[t - 1][c]) for c in cand]
        W = sum(ws)
        for c, wc in zip(cand, ws):
            q = Fraction(wc, W) if W > 0 else Fraction(1, len(cand))
            if q:
                deal(j + 1, [f for f in free if f != c], assign + [(c, t)], p * q)

    deal(0, list(H), [], Fraction(1))
    return worlds
