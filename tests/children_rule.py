"""The expand-all rule (sgx_count_moves / sgx_expand_all) restated in numpy on the oracle: what the device kernels must reproduce
bit for bit.  Test infrastructure (it imports oracle/); never imported by the product package.

For root slot i: pos = states[index[i]] with its mover; m = the mover's valid-action mask in its own perspective (the mask of the env's
observation); count[i] = its moves -- 0 for a finished game and for a mover without a move: the no-op entry [0, 0, K - 1] is never a child.
offsets = the exclusive scan of the counts (int64), total = offsets[n].  Child c: its root is the i with offsets[i] <= c < offsets[i + 1],
its action the (c - offsets[i])-th set entry of m in ascending flat order (the order of tests/playout_rule.py); the child is
OracleEnv.step(action) on reset(initial_state_override=pos): state, mover, and the step's reward / done / ending_invalid.  parent = i;
action = the flat spatial index in the mover's perspective, action_1d = the same move as an absolute 1-D index (maenv:684-689)."""
import numpy as np

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS

_envs = {}


def _variant(variant):
    return VARIANTS[variant] if isinstance(variant, str) else variant


def _env(variant):
    v = _variant(variant)
    if v.name not in _envs:
        _envs[v.name] = orc.OracleEnv(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts)
    return _envs[v.name]


def moves(variant, state, player):
    """One position int64 [34,R,C] and its mover -> its valid actions, ascending (int64 [count]; empty: finished, or no move)."""
    env = _env(variant)
    state = np.asarray(state, dtype=np.int64)
    if env.rules.get_game_ended(state, 1) != 0:
        return np.zeros(0, dtype=np.int64)
    obs = env.reset(initial_state_override=state, first_player_override=int(player))
    valid = np.flatnonzero(np.asarray(obs[env.player][env.MASK]).reshape(-1))
    if len(valid) == 1 and valid[0] == env.K - 1:                  # the no-op only: a mover without a move
        return np.zeros(0, dtype=np.int64)
    assert env.K - 1 not in valid.tolist() or len(valid) == 1
    return valid.astype(np.int64)


def action_1d(variant, action, player):
    """flat spatial index in the mover's perspective -> absolute 1-D index"""
    env = _env(variant)
    ru = env.rules
    spatial = np.unravel_index(int(action), (env.rows, env.columns, env.K))
    return int(ru.get_action_1d_index_from_player_perspective(ru.get_action_1d_index_from_spatial_index(tuple(int(x) for x in spatial)), int(player)))


def child(variant, state, player, action):
    """-> (child state, its mover, reward float32 [2], done, ending_invalid) of the step `action` on the position"""
    env = _env(variant)
    env.reset(initial_state_override=np.asarray(state, dtype=np.int64), first_player_override=int(player))
    obs, rewards, dones, infos = env.step({env.player: int(action)})
    reward = np.zeros(2, dtype=np.float32)
    done, ending_invalid = bool(dones['__all__']), False
    if done:
        reward[:] = rewards[1], rewards[-1]
        ending_invalid = bool(infos[1]['game_result_was_invalid'])
    return env.state.copy(), int(env.player), reward, int(done), int(ending_invalid)


def root_children(variant, state, player):
    """Everything about one root: dict(action int32 [n], action_1d int32 [n], state int64 [n,34,R,C], player int8 [n], reward float32 [n,2],
    done uint8 [n], ending_invalid uint8 [n])."""
    state = np.asarray(state, dtype=np.int64)
    acts = moves(variant, state, player)
    n = len(acts)
    out = {'action': acts.astype(np.int32), 'action_1d': np.asarray([action_1d(variant, a, player) for a in acts], dtype=np.int32),
           'state': np.empty((n,) + state.shape, dtype=np.int64), 'player': np.empty(n, dtype=np.int8),
           'reward': np.empty((n, 2), dtype=np.float32), 'done': np.empty(n, dtype=np.uint8), 'ending_invalid': np.empty(n, dtype=np.uint8)}
    for k, a in enumerate(acts):
        out['state'][k], out['player'][k], out['reward'][k], out['done'][k], out['ending_invalid'][k] = child(variant, state, player, a)
    return out


class Children:
    """All children of the roots states[index[i]] (index None: every state in order), the roots' own children restated once each.
    counts int32 [n], offsets int64 [n + 1], total; window(first, n) -> the children first .. first + n - 1 (clipped to total) as a dict with
    `parent` next to root_children's keys."""

    def __init__(self, variant, states, players, index=None, per_root=None):
        states = np.asarray(states, dtype=np.int64)
        self.index = np.arange(len(states)) if index is None else np.asarray(index, dtype=np.int64)
        self.per_root = per_root if per_root is not None else {}
        for s in sorted(set(self.index.tolist())):
            if s not in self.per_root:
                self.per_root[s] = root_children(variant, states[s], int(players[s]))
        self.counts = np.asarray([len(self.per_root[s]['action']) for s in self.index], dtype=np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts.astype(np.int64))]).astype(np.int64)
        self.total = int(self.offsets[-1])

    def window(self, first=0, n=None):
        last = self.total if n is None else min(first + n, self.total)
        cs = np.arange(first, max(last, first), dtype=np.int64)
        parent = (np.searchsorted(self.offsets, cs, side='right') - 1).astype(np.int32)
        rank = cs - self.offsets[parent]
        out = {'parent': parent}
        for key in ('action', 'action_1d', 'state', 'player', 'reward', 'done', 'ending_invalid'):
            proto = self.per_root[int(self.index[0])][key] if len(self.index) else None
            rows = [self.per_root[int(self.index[p])][key][k] for p, k in zip(parent, rank)]
            out[key] = np.stack(rows) if rows else proto[:0]
        return out
