"""The leaf-value rule (sgx_set_leaf_values) restated in numpy on the reference's int64 [34,R,C] states: what the device
kernels must reproduce bit for bit.  Test infrastructure; never imported by the product package.

A position that is not over is worth, to player p, v(p) = float32(clamp(mine(p) - theirs(p), -limit, limit)) / float32(denom), with
mine / theirs sums of an int16 table T [2][14][cells] over p's own pieces and over the opponent's pieces as p sees them (or, see_all, as
they are).  `scores` is the definition, entry by entry, for one state; `values` the same arithmetic on whole arrays for batches (the CPU
tests hold one against the other); `apply` puts the values where a result's rewards belong."""
import numpy as np

OWN = {1: 0, -1: 1}            # own(p): the layer of p's true pieces
PUB = {1: 3, -1: 4}            # pub(p): what p's opponent knows of p's pieces (13 = unidentified)


def persp(p, cell, cells):
    return cell if p == 1 else cells - 1 - cell


def scores(state, table, see_all=False):
    """-> (S(+1), S(-1)) as Python ints, straight from the definition"""
    L, R, C = state.shape
    cells = R * C
    flat = np.asarray(state).reshape(L, cells)
    out = []
    for p in (1, -1):
        mine = theirs = 0
        for cell in range(cells):
            t = int(flat[OWN[p], cell])
            if t:
                mine += int(table[0][t][persp(p, cell, cells)])
            d = int(flat[OWN[-p] if see_all else PUB[-p], cell])
            if d:
                theirs += int(table[1][d][persp(-p, cell, cells)])
        out.append(mine - theirs)
    return tuple(out)


def value_of(score, limit, denom):
    """float32(clamp(S, -limit, limit)) / float32(denom): one IEEE float32 division"""
    s = np.clip(np.asarray(score, dtype=np.int64), -int(limit), int(limit))
    assert (np.abs(s) <= 1 << 24).all() and 1 <= int(limit) <= int(denom) <= 1 << 24
    return s.astype(np.float32) / np.float32(denom)


def batch_scores(states, table, see_all=False):
    """states int64 [n,34,R,C] -> int64 [n,2]: scores(states[i], ...) for every i, in int32 arithmetic checked for headroom"""
    states = np.asarray(states, dtype=np.int64)
    table = np.asarray(table)
    n, L, R, C = states.shape
    cells = R * C
    assert table.shape == (2, 14, cells)
    flat = states.reshape(n, L, cells)
    T = table.astype(np.int64)
    own_cell = {1: np.arange(cells), -1: cells - 1 - np.arange(cells)}      # persp(p, cell) for every cell
    out = np.zeros((n, 2), dtype=np.int64)
    for col, p in enumerate((1, -1)):
        t = flat[:, OWN[p]]
        d = flat[:, OWN[-p] if see_all else PUB[-p]]
        mine = np.where(t != 0, T[0][np.clip(t, 0, 13), own_cell[p][None, :]], 0).sum(axis=1)
        theirs = np.where(d != 0, T[1][np.clip(d, 0, 13), own_cell[-p][None, :]], 0).sum(axis=1)
        out[:, col] = mine - theirs
    assert (np.abs(out) < 1 << 31).all()                                    # S fits int32
    return out


def values(states, table, limit, denom, see_all=False):
    """-> float32 [n,2]: (v(+1), v(-1)) of every state"""
    return value_of(batch_scores(states, table, see_all), limit, denom)


def apply(reward, done, states, table, limit, denom, see_all=False):
    """The rewards of a result with leaf values: `reward` float32 [n,2] as reported without a table, with the rows of the slots that are
    not over (done == 0) replaced by the values of their final `states`.  -> a new float32 [n,2]."""
    reward = np.array(reward, dtype=np.float32, copy=True)
    open_ = np.asarray(done).reshape(-1) == 0
    if open_.any():
        reward[open_] = values(np.asarray(states)[open_], table, limit, denom, see_all)
    return reward


def known_answer_state():
    """the 3x3 state of the known answers: two pieces per side; +1's scout is revealed, -1's marshal is not"""
    s = np.zeros((34, 3, 3), dtype=np.int64)
    s[0, 0, 0], s[0, 1, 1] = 11, 2            # +1: flag on cell 0, scout on cell 4
    s[3, 0, 0], s[3, 1, 1] = 13, 2
    s[1, 2, 2], s[1, 1, 2] = 11, 10           # -1: flag on cell 8, marshal on cell 5
    s[4, 2, 2], s[4, 1, 2] = 13, 13
    return s


def known_answer_table():
    """asymmetric in the cell: T[h][t][c] = (1 - 2h) * (100 * t + c) -- "mine" rows positive, "theirs" rows NEGATIVE, so that theirs is
    not mistaken for mine and a cell not for its mirror image"""
    t = np.arange(14)[None, :, None] * 100 + np.arange(9)[None, None, :]
    return (t * np.array([1, -1])[:, None, None]).astype(np.int16)


# worked by hand from the definition (cells = 9; persp(-1, c) = 8 - c):
#   mine(+1)  = T0[11][0] + T0[2][4]            = 1100 + 204  = 1304
#   mine(-1)  = T0[11][8 - 8] + T0[10][8 - 5]   = 1100 + 1003 = 2103
#   public:   theirs(+1) = T1[13][8 - 8] + T1[13][8 - 5] = -1300 - 1303 = -2603;  theirs(-1) = T1[13][0] + T1[2][4] = -1300 - 204 = -1504
#   see-all:  theirs(+1) = T1[11][0] + T1[10][3]         = -1100 - 1003 = -2103;  theirs(-1) = T1[11][0] + T1[2][4] = -1100 - 204 = -1304
KNOWN_SCORES = {False: (1304 + 2603, 2103 + 1504), True: (1304 + 2103, 2103 + 1304)}
