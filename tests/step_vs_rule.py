"""The rule of sgx_step_vs restated in numpy on the oracle: what the device kernel must reproduce bit for bit.  Test
infrastructure (it imports oracle/); never imported by the product package.

For one slot: pos = the root with its mover, side = the agent's side, g = the slot's global env id.
  1. invalid = moved = 0, reply = -1.
  2. pos not over, its mover is `side`, an action is given: the action is applied exactly as a step applies it (OracleEnv.step: it raises for
     an out-of-range value and for every move the rules refuse, the no-op of a mover that has a move included).  Refused: invalid = 1, pos
     stays, go to 4.  Applied: moved |= MOVED_AGENT.  (Where the mover is not `side` the action is not looked at.)
  3. pos not over and its mover is not `side`: the bot moves once.  The valid moves and their weights are weighted_playout_rule's
     (move_weights: for the bot as the mover, in the public view or with see_all the true one); r = rng(seed, g, draw, STREAM_REPLY = 8,
     pos's turn counter); the no-op where there is no move, else weighted_playout_rule.pick(r, w).  reply = that action (in the bot's
     perspective), moved |= MOVED_BOT.
  4. the result is pos; reward / done / ending_invalid / player are what a step on it reports (replay_rule words them the same way).
No loop: players alternate, so the bot never moves twice."""
import numpy as np

from oracle import oracle as orc
from tests import replay_rule as rr, weighted_playout_rule as wr

STREAM_REPLY = 8
MOVED_AGENT, MOVED_BOT = 1, 2


def valid_actions(variant, state, player):
    """The set entries of the mover's perspective mask in ascending flat order (the no-op alone for a mover without a move)."""
    env = rr._env(variant)
    obs = env.reset(initial_state_override=np.asarray(state, dtype=np.int64), first_player_override=int(player))
    return np.flatnonzero(np.asarray(obs[env.player][env.MASK]).reshape(-1))


def step_vs(variant, state, player, action, side, seed, g, draw, weights, see_all=False, trace=None):
    """One position int64 [34,R,C], its mover, the agent's action (None: not given) and side -> (final state, player, reward float32 [2],
    done, ending_invalid, invalid, moved, reply).  trace (a list): the bot's draw is appended as (valid moves, their weights, chosen index)."""
    weights = np.asarray(weights)
    assert weights.shape == wr.SHAPE and weights.min() >= 0 and weights.max() <= 4095
    assert side in (1, -1)
    env = rr._env(variant)
    ru = env.rules
    obs = env.reset(initial_state_override=np.asarray(state, dtype=np.int64), first_player_override=int(player))
    over = lambda: ru.get_game_ended(env.state, 1) != 0
    invalid, moved, reply = 0, 0, -1
    if not over() and env.player == side and action is not None:
        try:
            obs = env.step({env.player: int(action)})[0]
            moved |= MOVED_AGENT
        except ValueError:
            invalid = 1
    if not invalid and not over() and env.player != side:
        valid = np.flatnonzero(np.asarray(obs[env.player][env.MASK]).reshape(-1))
        assert len(valid) > 0
        r = orc.rng(seed, g, draw, STREAM_REPLY, int(env.state[5, 0, 0]))
        if len(valid) == 1 and valid[0] == wr._noop(variant):               # n == 0: the no-op of a mover without a move
            k = 0
        else:
            w = wr.move_weights(variant, env.state, env.player, valid, weights, see_all)
            k, _ = wr.pick(r, w)
            if trace is not None:
                trace.append((valid, w, k))
        reply = int(valid[k])
        env.step({env.player: reply})
        moved |= MOVED_BOT
    final = env.state.copy()
    done = over()
    ending_invalid = bool(done and ru.get_game_result_is_invalid(final))
    reward = np.zeros(2, dtype=np.float32)
    if done and not ending_invalid:
        reward[:] = ru.get_game_ended(final, 1), ru.get_game_ended(final, -1)
    return final, int(env.player), reward, int(done), int(ending_invalid), invalid, moved, reply


def step_vs_batch(variant, states, players, actions, sides, seed, env_id_offset, draw, weights, see_all=False, index=None):
    """Slot i <- step_vs(states[index[i]], actions[i], sides[i], ...) with g = env_id_offset + i, like the device call.  actions: [n] or None;
    sides: +1 / -1 or [n] (< 0: -1).
    -> final states int64 [n,34,R,C], players int8 [n], reward float32 [n,2], done uint8 [n], ending_invalid uint8 [n], invalid uint8 [n],
    moved uint8 [n], reply int32 [n]."""
    states = np.asarray(states, dtype=np.int64)
    idx = np.arange(len(states)) if index is None else np.asarray(index, dtype=np.int64)
    n = len(idx)
    sides = np.broadcast_to(np.asarray(sides), (n,))
    out = np.empty((n,) + states.shape[1:], dtype=np.int64)
    out_players = np.empty(n, dtype=np.int8)
    reward = np.empty((n, 2), dtype=np.float32)
    done, ending_invalid = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
    invalid, moved = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
    reply = np.empty(n, dtype=np.int32)
    for i, s in enumerate(idx):
        out[i], out_players[i], reward[i], done[i], ending_invalid[i], invalid[i], moved[i], reply[i] = step_vs(
            variant, states[s], int(players[s]), None if actions is None else int(actions[i]), -1 if sides[i] < 0 else 1, seed, env_id_offset + i,
            draw, weights, see_all)
    return out, out_players, reward, done, ending_invalid, invalid, moved, reply
