"""The piece-origins rule (sgx_set_replay_origins) restated in numpy on the oracle, next to the replay rule it rides on
(tests/replay_rule.py): what the TRACK instantiations of the replay kernel must reproduce bit for bit.  Test infrastructure (it imports
oracle/); never imported by the product package.

own(q) = state layer q (true pieces; index 0 is player +1, 1 is player -1); cells are absolute, r * C + c.
  Start: Lab[q][c] = (origin_in[q][c] if given, else c) where own(q)(root)[c] != 0, and -1 everywhere else.
  Every applied entry taking pos to pos', mover index q, opponent q':
    a = the one cell with own(q)(pos)[a] != 0 and own(q)(pos')[a] == 0;
    Lab'[q] = Lab[q], except Lab'[q][a] = -1 and, if some cell b has own(q)(pos)[b] == 0 and own(q)(pos')[b] != 0, Lab'[q][b] = Lab[q][a];
    Lab'[q'][c] = Lab[q'][c] where own(q')(pos')[c] != 0, else -1.
    (a valid no-op entry moves no piece: there is no cell a and nothing changes)
  Entries passed over or refused change nothing.  Output: Lab at the final position, whole."""
import numpy as np

from tests.replay_rule import STOP_EXHAUSTED, STOP_GAME_OVER, STOP_INVALID, _apply, _env


def own(state, q):
    return np.asarray(state)[q].reshape(-1)


def start_labels(state, origin_in=None):
    """int16 [2, cells] of a root position."""
    cells = np.asarray(state)[0].size
    lab = np.full((2, cells), -1, dtype=np.int16)
    for q in range(2):
        given = np.arange(cells, dtype=np.int16) if origin_in is None else np.asarray(origin_in, dtype=np.int16)[q]
        occ = own(state, q) != 0
        lab[q, occ] = given[occ]
    return lab


def advance(lab, pos, pos_next, q):
    """The labels after one applied entry of mover index q that took state `pos` to `pos_next`."""
    out = lab.copy()
    before, after = own(pos, q) != 0, own(pos_next, q) != 0
    a = np.flatnonzero(before & ~after)
    b = np.flatnonzero(~before & after)
    assert len(a) <= 1 and len(b) <= len(a), "an applied entry moves at most one piece of the mover"
    if len(a):
        out[q, a[0]] = -1
        if len(b):
            out[q, b[0]] = lab[q, a[0]]
    out[1 - q, own(pos_next, 1 - q) == 0] = -1
    return out


def replay_tracked(variant, state, player, actions, length=None, skip_invalid=False, actions_1d=False, allow_piece_oscillation=False, origin_in=None):
    """replay_rule.replay's loop with the labels carried along.  -> (labels int16 [2, cells], final state, player, applied, consumed, stop)."""
    env = _env(variant)
    ru = env.rules
    actions = np.asarray(actions).reshape(-1)
    n = len(actions) if length is None else min(max(int(length), 0), len(actions))
    env.reset(initial_state_override=np.asarray(state, dtype=np.int64), first_player_override=int(player))
    lab = start_labels(env.state, origin_in)
    c = m = 0
    while True:
        if c == n:
            stop = STOP_EXHAUSTED
            break
        if ru.get_game_ended(env.state, 1) != 0:
            stop = STOP_GAME_OVER
            break
        pos, q = env.state.copy(), 0 if int(env.player) == 1 else 1
        if _apply(env, actions[c], actions_1d, allow_piece_oscillation):
            lab = advance(lab, pos, env.state, q)
            m += 1
            c += 1
        elif skip_invalid:
            c += 1
        else:
            stop = STOP_INVALID
            break
    return lab, env.state.copy(), int(env.player), m, c, stop


def replay_tracked_batch(variant, states, players, actions, lengths=None, index=None, skip_invalid=False, actions_1d=False,
                         allow_piece_oscillation=False, origins_in=None):
    """Slot i <- replay_tracked(states[index[i]], actions[i][:lengths[i]], origin_in = origins_in[index[i]]), like the device call.
    -> labels int16 [n, 2, cells]."""
    states = np.asarray(states, dtype=np.int64)
    idx = np.arange(len(actions)) if index is None else np.asarray(index, dtype=np.int64)
    out = np.empty((len(idx), 2, states[0][0].size), dtype=np.int16)
    for i, s in enumerate(idx):
        out[i] = replay_tracked(variant, states[s], int(players[s]), actions[i], None if lengths is None else int(lengths[i]), skip_invalid,
                                actions_1d, allow_piece_oscillation, None if origins_in is None else origins_in[s])[0]
    return out
