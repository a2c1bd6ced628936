"""The determinization rule (sgx_determinize) restated in numpy on the reference's int64 [34,R,C] states: what the device
kernel must reproduce bit for bit.  Test infrastructure (it imports oracle/ for the counter RNG); never imported by the product package.

For a state, its mover and an observer (0 = the mover), with `opp` the observer's opponent:
  H = cells with an opp piece whose public layer says 13, ascending; A = those of H never moved, B = the rest;
  I = the types 11 / 12 found on H in cell order, M = the other types on H in cell order;
  a type of I on a cell of B cannot come from play: the state is returned unchanged with -1;
  Fisher-Yates on L = A (k = |A|-1 .. 1: swap L[k], L[rng_below(rng(seed, g, draw, 5, k), k + 1)]); L[q] <- I[q];
  L2 = L[|I|:] ++ B, Fisher-Yates with counter 1024 + k; L2[q] <- M[q].
Only the opponent's pieces layer changes."""
import numpy as np

from oracle import oracle as orc

STREAM_DETERMINIZE = 5
UNKNOWN, FLAG, BOMB = 13, 11, 12
L_PIECES, L_PO, L_STILL = 0, 3, 32          # + player index (0 = player +1, 1 = player -1)


def _shuffle(cells, seed, g, draw, t0):
    for k in range(len(cells) - 1, 0, -1):
        r = orc.rng_below(orc.rng(seed, g, draw, STREAM_DETERMINIZE, t0 + k), k + 1)
        cells[k], cells[r] = cells[r], cells[k]


def hidden_lists(state, mover, observer=0):
    """-> (opp player index, A, B, I, M) of the rule."""
    o = int(observer) if observer else int(mover)
    opp = 1 if o == 1 else 0
    pieces, po, still = state[L_PIECES + opp].reshape(-1), state[L_PO + opp].reshape(-1), state[L_STILL + opp].reshape(-1)
    H = [int(c) for c in np.flatnonzero((pieces != 0) & (po == UNKNOWN))]
    A = [c for c in H if still[c] != 0]
    B = [c for c in H if still[c] == 0]
    I = [int(pieces[c]) for c in H if pieces[c] in (FLAG, BOMB)]
    M = [int(pieces[c]) for c in H if pieces[c] not in (FLAG, BOMB)]
    return opp, A, B, I, M


def determinize(state, mover, observer, seed, g, draw):
    """One state int64 [34,R,C] -> (the sampled world, number of hidden cells shuffled or -1)."""
    state = np.asarray(state, dtype=np.int64)
    opp, A, B, I, M = hidden_lists(state, mover, observer)
    out = state.copy()
    pieces = state[L_PIECES + opp].reshape(-1)
    if any(pieces[c] in (FLAG, BOMB) for c in B):
        return out, -1
    flat = out[L_PIECES + opp].reshape(-1)               # (a view: the layer is contiguous)
    L = list(A)
    _shuffle(L, seed, g, draw, 0)
    for q, t in enumerate(I):
        flat[L[q]] = t
    L2 = L[len(I):] + B
    _shuffle(L2, seed, g, draw, 1024)
    for q, t in enumerate(M):
        flat[L2[q]] = t
    return out, len(A) + len(B)


def determinize_batch(states, movers, observer, seed, env_id_offset, draw, src_index=None):
    """Slot i <- determinize(states[src_index[i]], ...) with g = env_id_offset + i, like the device call."""
    states = np.asarray(states, dtype=np.int64)
    idx = np.arange(len(states)) if src_index is None else np.asarray(src_index, dtype=np.int64)
    out = np.empty((len(idx),) + states.shape[1:], dtype=np.int64)
    hidden = np.empty(len(idx), dtype=np.int32)
    for i, s in enumerate(idx):
        out[i], hidden[i] = determinize(states[s], int(movers[s]), observer, seed, env_id_offset + i, draw)
    return out, hidden


def chi2_quantile_999(df):
    """0.999 quantile of the chi-squared distribution with df degrees of freedom (Wilson-Hilferty)."""
    z = 3.090232306167813
    return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3
