"""The weighted playout rule (sgx_playout_weighted) restated in numpy on the oracle: what the device kernel must reproduce bit
for bit.  Test infrastructure (it imports oracle/); never imported by the product package.

Everything is playout_rule.playout's -- the key, the move bound, max_steps, the results -- except how the move is taken from the draw.
For a position that is not over, with mover p: a_0 < ... < a_{n-1} are the set entries of the mover's perspective mask in ascending flat
order (a = pcell * K + ch).  For each: dir = the block of the channel (perspective +r, -r, +c, -c; +r is towards the opponent's setup rows),
t = the mover's true piece type on the start cell, d = what stands on the destination -- the opponent's PUBLIC layer (0 empty, 1..12 a
revealed type, 13 unknown), or with see_all the opponent's TRUE type.  w_i = weights[dir][t][d], W = sum w_i.
r = rng(seed, g, draw, 6, turn), the draw playout_rule takes.  W > 0: x = rng_below(r, W), the move is the first a_i whose inclusive prefix
sum exceeds x.  W == 0: k = rng_below(r, n), the k-th valid move, as playout_rule."""
import numpy as np

from oracle import oracle as orc
from tests import playout_rule as pr

STREAM_PLAYOUT = pr.STREAM_PLAYOUT
SHAPE = (4, 13, 14)


def move_weights(variant, state, player, valid, weights, see_all=False):
    """The weights of the flat perspective actions `valid` of `player` at `state` (int64 [34,R,C], absolute coordinates) -> int64 [len(valid)]."""
    v = pr._variant(variant)
    R, C = v.rows, v.columns
    K = 2 * (R - 1) + 2 * (C - 1) + 1
    state = np.asarray(state)
    own = state[0 if player == 1 else 1]
    there = state[(1 if player == 1 else 0) + (0 if see_all else 3)]          # the opponent's true pieces / what the mover knows of them
    starts = (0, R - 1, 2 * (R - 1), 2 * (R - 1) + (C - 1), K - 1)
    out = np.zeros(len(valid), dtype=np.int64)
    for j, a in enumerate(np.asarray(valid, dtype=np.int64).tolist()):
        pcell, ch = divmod(a, K)
        assert ch < K - 1, "the no-op is not a move"
        direction = max(i for i in range(4) if ch >= starts[i])
        k = ch - starts[direction] + 1
        sr, sc = divmod(pcell, C)
        er, ec = sr + (k if direction == 0 else -k if direction == 1 else 0), sc + (k if direction == 2 else -k if direction == 3 else 0)
        if player == -1:                                               # the perspective of player -1 is the board turned by 180 degrees
            sr, sc, er, ec = R - 1 - sr, C - 1 - sc, R - 1 - er, C - 1 - ec
        t, d = int(own[sr, sc]), int(there[er, ec])
        assert 1 <= t <= 10 and 0 <= d <= 13
        out[j] = int(weights[direction][t][d])
    return out


def pick(r, w):
    """The index of the move the draw r takes among moves of weights w (int64 [n], n >= 1) -> (index, W)."""
    W = int(w.sum())
    assert W < 1 << 32
    if W == 0:
        return orc.rng_below(r, len(w)), 0
    x = orc.rng_below(r, W)
    return int(np.searchsorted(np.cumsum(w), x, side='right')), W


def playout(variant, state, player, seed, g, draw, weights, see_all=False, max_steps=0, trace=None):
    """One position int64 [34,R,C] and its mover -> (final state, player, reward float32 [2], done, ending_invalid, length, n_zero, n_pos):
    playout_rule.playout's six, then how many positions had W == 0 and how many W > 0.  trace (a list): every move is appended as
    (weights of the valid moves, chosen index)."""
    weights = np.asarray(weights)
    assert weights.shape == SHAPE and weights.min() >= 0 and weights.max() <= 4095
    env = pr._env(variant)
    ru = env.rules
    state = np.asarray(state, dtype=np.int64)
    obs = env.reset(initial_state_override=state, first_player_override=int(player))
    turn, max_turns = int(state[5, 0, 0]), int(state[5, 1, 0])
    limit = max(max_turns - turn, 0) + 1
    if max_steps > 0:
        limit = min(limit, int(max_steps))
    over = ru.get_game_ended(state, 1) != 0
    reward = np.zeros(2, dtype=np.float32)
    ending_invalid = False
    if over:
        ending_invalid = ru.get_game_result_is_invalid(state)
        if not ending_invalid:
            reward[:] = ru.get_game_ended(state, 1), ru.get_game_ended(state, -1)
    length = n_zero = n_pos = 0
    while not over and length < limit:
        mask = np.asarray(obs[env.player][env.MASK]).reshape(-1)
        valid = np.flatnonzero(mask)
        assert len(valid) > 0
        turn = int(env.state[5, 0, 0])
        r = orc.rng(seed, g, draw, STREAM_PLAYOUT, turn)
        if len(valid) == 1 and valid[0] == _noop(variant):             # n == 0: the no-op [0, 0, K - 1] of a mover without a move
            k = 0
        else:
            w = move_weights(variant, env.state, env.player, valid, weights, see_all)
            k, W = pick(r, w)
            n_zero += int(W == 0)
            n_pos += int(W > 0)
            if trace is not None:
                trace.append((w, k))
        obs, rewards, dones, infos = env.step({env.player: int(valid[k])})
        length += 1
        if dones['__all__']:
            over = True
            reward[:] = rewards[1], rewards[-1]
            ending_invalid = bool(infos[1]['game_result_was_invalid'])
    return env.state.copy(), int(env.player), reward, int(over), int(ending_invalid), length, n_zero, n_pos


def _noop(variant):
    v = pr._variant(variant)
    return 2 * (v.rows - 1) + 2 * (v.columns - 1)


def playout_batch(variant, states, players, seed, env_id_offset, draw, weights, see_all=False, index=None, max_steps=0):
    """Slot i <- playout(states[index[i]], ...) with g = env_id_offset + i, like the device call.
    -> final states int64 [n,34,R,C], players int8 [n], reward float32 [n,2], done uint8 [n], ending_invalid uint8 [n], length int32 [n],
    n_zero int64 [n], n_pos int64 [n]."""
    states = np.asarray(states, dtype=np.int64)
    idx = np.arange(len(states)) if index is None else np.asarray(index, dtype=np.int64)
    n = len(idx)
    out = np.empty((n,) + states.shape[1:], dtype=np.int64)
    out_players = np.empty(n, dtype=np.int8)
    reward = np.empty((n, 2), dtype=np.float32)
    done = np.empty(n, dtype=np.uint8)
    ending_invalid = np.empty(n, dtype=np.uint8)
    length = np.empty(n, dtype=np.int32)
    n_zero, n_pos = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for i, s in enumerate(idx):
        out[i], out_players[i], reward[i], done[i], ending_invalid[i], length[i], n_zero[i], n_pos[i] = playout(
            variant, states[s], int(players[s]), seed, env_id_offset + i, draw, weights, see_all, max_steps)
    return out, out_players, reward, done, ending_invalid, length, n_zero, n_pos
