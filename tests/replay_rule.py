"""The replay rule (sgx_replay) restated in numpy on the oracle: what the device kernel must reproduce bit for bit.  Test
infrastructure (it imports oracle/); never imported by the product package.

For slot i: pos = states[index[i]] with its mover, len = lengths[i] clamped to [0, max_len], c = m = 0.  Loop:
  1. c == len: stop = 0, end.
  2. pos is over: stop = 1, end (entries after the end of the game are not read).
  3. entry c is applied to pos exactly as a step applies an action: OracleEnv.step for flat spatial actions in the mover's perspective (it
     raises for an out-of-range value -- np.unravel_index -- and for every move the rules refuse, the no-op of a mover that has a move
     included); with actions_1d OracleRules.get_next_state on the absolute 1-D index (an index outside [0, action_size) decodes to cells
     off the board and is refused).  No auto-reset.
  4. valid: m++, c++.   5. invalid with skip_invalid: c++, pos unchanged.   6. invalid without: stop = 2, end; c stays.
reward / done / ending_invalid / player: what a step on the final position reports (0, 0 and done = 0 while the game is not over);
applied = m, consumed = c.  No random draw: a function of (state, list, flags)."""
import numpy as np

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS

STOP_EXHAUSTED, STOP_GAME_OVER, STOP_INVALID = 0, 1, 2
_envs = {}


def _variant(variant):
    return VARIANTS[variant] if isinstance(variant, str) else variant


def _env(variant):
    v = _variant(variant)
    if v.name not in _envs:
        _envs[v.name] = orc.OracleEnv(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts)
    return _envs[v.name]


def _apply(env, action, actions_1d, allow_piece_oscillation):
    """One entry on env's position.  -> True if it was valid (env moved on), False if it was refused (env unchanged)."""
    ru = env.rules
    a = int(action)
    if not actions_1d and not allow_piece_oscillation:
        try:
            env.step({env.player: a})
        except ValueError:
            return False
        return True
    # the same step through the pure functions: spatial index in the mover's perspective -> absolute 1-D index (maenv:684-689)
    if not actions_1d:
        if a < 0 or a >= env.rows * env.columns * env.K:
            return False
        spatial = np.unravel_index(a, (env.rows, env.columns, env.K))
        a = ru.get_action_1d_index_from_player_perspective(ru.get_action_1d_index_from_spatial_index(tuple(int(x) for x in spatial)), env.player)
    if a < 0 or a >= ru.action_size:
        return False
    try:
        env.state, env.player = ru.get_next_state(env.state, env.player, a, allow_piece_oscillation)
    except ValueError:
        return False
    env.player = int(env.player)
    return True


def replay(variant, state, player, actions, length=None, skip_invalid=False, actions_1d=False, allow_piece_oscillation=False):
    """One position int64 [34,R,C], its mover and its list -> (final state, player, reward float32 [2], done, ending_invalid, applied,
    consumed, stop).  length: None = the whole list."""
    env = _env(variant)
    ru = env.rules
    actions = np.asarray(actions).reshape(-1)
    n = len(actions) if length is None else min(max(int(length), 0), len(actions))
    env.reset(initial_state_override=np.asarray(state, dtype=np.int64), first_player_override=int(player))
    c = m = 0
    while True:
        if c == n:
            stop = STOP_EXHAUSTED
            break
        if ru.get_game_ended(env.state, 1) != 0:
            stop = STOP_GAME_OVER
            break
        if _apply(env, actions[c], actions_1d, allow_piece_oscillation):
            m += 1
            c += 1
        elif skip_invalid:
            c += 1
        else:
            stop = STOP_INVALID
            break
    final = env.state.copy()
    over = ru.get_game_ended(final, 1) != 0
    ending_invalid = bool(over and ru.get_game_result_is_invalid(final))
    reward = np.zeros(2, dtype=np.float32)
    if over and not ending_invalid:
        reward[:] = ru.get_game_ended(final, 1), ru.get_game_ended(final, -1)
    return final, int(env.player), reward, int(over), int(ending_invalid), m, c, stop


def replay_batch(variant, states, players, actions, lengths=None, index=None, skip_invalid=False, actions_1d=False, allow_piece_oscillation=False):
    """Slot i <- replay(states[index[i]], actions[i][:lengths[i]], ...), like the device call; actions: [n, L] (any array of lists).
    -> final states int64 [n,34,R,C], players int8 [n], reward float32 [n,2], done uint8 [n], ending_invalid uint8 [n], applied int32 [n],
    consumed int32 [n], stop uint8 [n]."""
    states = np.asarray(states, dtype=np.int64)
    idx = np.arange(len(actions)) if index is None else np.asarray(index, dtype=np.int64)
    n = len(idx)
    out = np.empty((n,) + states.shape[1:], dtype=np.int64)
    out_players = np.empty(n, dtype=np.int8)
    reward = np.empty((n, 2), dtype=np.float32)
    done = np.empty(n, dtype=np.uint8)
    ending_invalid = np.empty(n, dtype=np.uint8)
    applied = np.empty(n, dtype=np.int32)
    consumed = np.empty(n, dtype=np.int32)
    stop = np.empty(n, dtype=np.uint8)
    for i, s in enumerate(idx):
        out[i], out_players[i], reward[i], done[i], ending_invalid[i], applied[i], consumed[i], stop[i] = replay(
            variant, states[s], int(players[s]), actions[i], None if lengths is None else int(lengths[i]), skip_invalid, actions_1d,
            allow_piece_oscillation)
    return out, out_players, reward, done, ending_invalid, applied, consumed, stop
