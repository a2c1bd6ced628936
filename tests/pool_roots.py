"""Roots for the pool-to-pool tests (support code, no tests): the boards, rollout lengths, keys and draws the playout tests take their
roots with and every later pool-to-pool file reuses; golden games as replay inputs; positions sampled along golden games; the agent's
actions of the step-vs tests; the oracle-made start pools and their follower.  Nothing here touches the GPU at import."""
import numpy as np

from oracle import oracle as orc
from stratego_env_amd import setups as S
from stratego_env_amd.config import VARIANTS
from tests import replay_rule as rr, step_vs_rule as sv
from tests.boards import _board
from tests.helpers import FOBS, MASK, POBS, _blank_state, _put, load_games, oracle_env

# ---- playouts: the roots every pool-to-pool file takes -------------------------------------------------------------------------------
DRAWS = (0, 1, 1 << 40)
KEYS = ((0, 0), (0xABCDEF0123, 1000))                    # (seed, env_id_offset) of dst
N_SRC = 24
# board: (rollout steps before the roots are taken, the three max_steps values: 0 = to the end where that fits the budget, else a cap,
#         the unfinished root that 20 slots share: one whose playouts end at different lengths under the cap)
CASES = {
    'micro': (12, (0, 1, 7), 22),                            # 3x4, four games per wave
    'tiny': (20, (0, 1, 7), 23),                             # 4x4, four games per wave
    'fives': (30, (0, 1, 7), 23),                            # 5x5 (odd), two games per wave
    'medium': (60, (0, 1, 7), 23),                           # 6x6, two games per wave (the half-wave variant)
    'octa_barrage': (150, (1, 7, 40), 23),                   # 8x8
    'short_barrage': (60, (0, 1, 7), 23),                    # 10x10, max_turns 100: to the end
    'barrage': (400, (1, 7, 48), 14),                        # 10x10
    'standard2': (400, (1, 7, 24), 17),                      # 15x15, one game per wave
}
GAMES_PER_WORKGROUP = {'fives': 16, 'medium': 8, 'short_barrage': 8}     # Geo::WPB x Geo::GPW of the logic-only launches


def _np(t):
    return t.cpu().numpy()


def _roots(name, steps, n=N_SRC, seed=17):
    """A live env of n games `steps` rollout steps into their games, finished games kept -> (env, states, players, finished)."""
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv(name, n, seed=seed, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(steps, emit_obs=False, emit_mask=False)
    states_t, players_t = env.export_state()
    finished = _np(env.env_info()[:, 2]) != 0
    return env, _np(states_t), _np(players_t), finished


def _playout_results(res):
    return {'reward': _np(res.reward), 'done': _np(res.done), 'ending_invalid': _np(res.ending_invalid), 'player': _np(res.player),
            'length': _np(res.length)}


PLAYOUT_OUT_SPECS = (('reward', 2, 'float32'), ('done', 1, 'uint8'), ('ending_invalid', 1, 'uint8'), ('player', 1, 'int8'), ('length', 1, 'int32'))


def _pool_from(env, name, n):
    """a pool holding the records of `env` (None: of a fresh env after reset())"""
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    own = env is None
    if own:
        env = VecStrategoEnv(name, n, seed=1, auto_reset=False, human_inits=False, placement='plain')
        env.reset()
    pool = PackedStates(name, n)
    st, pl = env.export_state()
    pool._vec.import_state(st, pl)
    if own:
        env.close()
    return pool


# ---- weighted playouts and step-vs: the same roots, and three boards outside the main library ------------------------------------------
# board -> (rollout steps before the roots are taken, the max_steps of draw 0 / 1 / 2): CASES', a cap of 20 where it plays to the end
WEIGHTED_CASES = {name: (CASES[name][0], tuple(c if c else 20 for c in CASES[name][1]))
                  for name in ('micro', 'fives', 'medium', 'octa_barrage', 'barrage', 'standard2')}
WEIGHTED_CASES['c3x40'] = (100, (1, 7, 30))                # K = 83 channels, two games of 32 lanes per wave: the cell's channels in slices
WEIGHTED_CASES['c32x32'] = (40, (1, 7, 20))                # 10-bit cells, 16 cells per lane
WEIGHTED_CASES['c20x20'] = (40, (1, 7, 20))                # the workgroup's LDS with the weight sums passes 64 KB


def _board_roots(name, steps, n=N_SRC, seed=17):
    return _roots(_board(name), steps, n=n, seed=seed)


# ---- replays: golden games and ragged lists --------------------------------------------------------------------------------------------
GOLDEN = ['barrage', 'standard', 'micro', 'tiny', 'fives', 'medium', 'octa_barrage', 'short_barrage', 'short_standard', 'standard2']
# lanes per game of the logic-only launches (Geo::LPG: 16 on boards of up to 16 cells, 32 up to 32 cells and on the two-games-per-wave
# variant of the boards up to 128 cells, else 64): the size of the kernel's prefetch chunk
LPG = {'micro': 16, 'tiny': 16, 'fives': 32, 'medium': 32, 'octa_barrage': 32, 'short_barrage': 32, 'barrage': 32, 'standard2': 64}


def _replay_results(res):
    return {'applied': _np(res.applied), 'consumed': _np(res.consumed), 'stop': _np(res.stop), 'reward': _np(res.reward),
            'done': _np(res.done), 'ending_invalid': _np(res.ending_invalid), 'player': _np(res.player)}


def _golden(name):
    """-> (g, actions int32 [n, longest] padded with -1, lengths int32 [n], errors per game)"""
    g = load_games(name)
    off = g['offsets']
    n = len(off) - 1
    lengths = (off[1:] - off[:-1]).astype(np.int32)
    acts = np.full((n, int(lengths.max())), -1, dtype=np.int32)
    errs = []
    for gi in range(n):
        acts[gi, :lengths[gi]] = g['actions'][off[gi]:off[gi + 1]]
        errs.append(g['errors'][off[gi]:off[gi + 1]].astype(bool))
    return g, acts, lengths, errs


def _golden_roots(name, g):
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    n = len(g['offsets']) - 1
    env = VecStrategoEnv(name, n, seed=1, auto_reset=False, human_inits=False, placement='plain')
    env.reset(torch.from_numpy(g['p1_maps'][:n]), torch.from_numpy(g['p2_maps'][:n]))
    return env


def _make_list(name, state, player, length, rs, inject):
    """A list of `length` entries from a position: random valid moves played forward by the oracle; `inject`: one entry is invalid instead
    (-1, the number of spatial actions, or an in-range move the mask refuses) and the position stays; after the end of the game the list
    goes on with arbitrary in-range entries.  -> (flat spatial entries in the mover's perspective, the same list as absolute 1-D indices)"""
    env = rr._env(name)
    ru = env.rules
    NA, AS = env.rows * env.columns * env.K, ru.action_size
    obs = env.reset(initial_state_override=np.asarray(state, dtype=np.int64), first_player_override=int(player))
    sp, d1 = [], []
    inj_at = int(rs.randint(length)) if (inject and length > 0) else -1
    for t in range(length):
        if ru.get_game_ended(env.state, 1) != 0:
            sp.append(int(rs.randint(NA))); d1.append(int(rs.randint(AS)))
            continue
        mask = np.asarray(obs[env.player][MASK]).reshape(-1)
        if t == inj_at:
            kind = int(rs.randint(3))
            if kind == 0:
                sp.append(-1); d1.append(-1)
            elif kind == 1:
                sp.append(NA); d1.append(AS)
            else:
                zeros = np.flatnonzero(mask == 0)
                sp.append(int(zeros[rs.randint(len(zeros))]))
                zeros1 = np.flatnonzero(ru.get_valid_moves_as_1d_mask(env.state, env.player) == 0)
                d1.append(int(zeros1[rs.randint(len(zeros1))]))
            continue
        valid = np.flatnonzero(mask)
        a = int(valid[rs.randint(len(valid))])
        spatial = tuple(int(x) for x in np.unravel_index(a, (env.rows, env.columns, env.K)))
        sp.append(a)
        d1.append(ru.get_action_1d_index_from_player_perspective(ru.get_action_1d_index_from_spatial_index(spatial), env.player))
        obs, _, _, _ = env.step({env.player: a})
    return sp, d1


def _ragged_lists(name, states, players, idx, rs):
    """-> (spatial int32 [n, L], 1-D int32 [n, L], lengths int32 [n]); the padding holds a valid-looking 0"""
    lpg = LPG[name]
    choices = (0, 1, lpg - 1, lpg, lpg + 1, 2 * lpg + 3)
    n = len(idx)
    lengths = np.asarray([choices[(i + int(rs.randint(2))) % 6] for i in range(n)], dtype=np.int32)
    L = 2 * lpg + 3
    sp = np.zeros((n, L), dtype=np.int32)
    d1 = np.zeros((n, L), dtype=np.int32)
    for i, s in enumerate(idx):
        a, b = _make_list(name, states[s], players[s], int(lengths[i]), rs, inject=(i % 3 == 1))
        sp[i, :lengths[i]], d1[i, :lengths[i]] = a, b
    return sp, d1, lengths


def _layouts(acts, torch):
    """the list tensor in two layouts: dense game-major with a game stride beyond the longest list, and the transposed view of [L, n]"""
    n, L = acts.shape
    wide = torch.full((n, L + 5), -7, dtype=torch.int32, device='cuda')
    wide[:, :L] = torch.from_numpy(acts).cuda()
    dense = wide[:, :L]
    assert dense.stride() == (L + 5, 1)
    tn = torch.from_numpy(np.ascontiguousarray(acts.T)).cuda()
    transposed = tn.T
    assert transposed.stride() == (1, n) and tuple(transposed.shape) == (n, L)
    return (('dense', dense, wide), ('transposed', transposed, tn))


# ---- positions along rollouts and golden games -------------------------------------------------------------------------------------------
def _live_env(name, n, steps, seed):
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv(name, n, seed=seed, auto_reset=True, placement='plain')
    env.reset()
    env.rollout_steps(steps)
    return env


def _sample_states(name, n, rs):
    """states / players sampled along golden games (including terminal ones)."""
    g = load_games(name)
    off = g['offsets']
    env = oracle_env(name)
    states, players = [], []
    gi = 0
    while len(states) < n:
        env.reset(g['p1_maps'][gi].astype(np.int64), g['p2_maps'][gi].astype(np.int64))
        ks = [k for k in range(off[gi], off[gi + 1]) if not g['errors'][k]]
        take = set(rs.choice(len(ks), size=min(len(ks), 12), replace=False).tolist()) | {len(ks) - 1}
        for i, k in enumerate(ks):
            env.step({env.player: int(g['actions'][k])})
            if i in take and len(states) < n:
                states.append(env.state.copy()); players.append(env.player if i != len(ks) - 1 else int(rs.choice([1, -1])))
        gi = (gi + 1) % (len(off) - 1)
    return np.stack(states), np.asarray(players, dtype=np.int8)


def sampled_states(name, n_games=3, every=5):
    """(state, mover) pairs along the first golden games of a variant: the start and every `every`-th position."""
    g = load_games(name)
    off = g['offsets']
    env = oracle_env(name)
    out = []
    for gi in range(min(n_games, len(off) - 1)):
        env.reset(g['p1_maps'][gi].astype(np.int64), g['p2_maps'][gi].astype(np.int64))
        out.append((env.state.copy(), env.player))
        for n, k in enumerate(range(off[gi], off[gi + 1])):
            if g['errors'][k]:
                continue
            _, _, done, _ = env.step({env.player: int(g['actions'][k])})
            if done['__all__']:
                out.append((env.state.copy(), env.player))          # (no special case for finished games)
                break
            if n % every == 0:
                out.append((env.state.copy(), env.player))
    return out


def fives_position():
    """Fives, observer +1: the opponent's five pieces {4, 5, 6, 7, flag} all hidden, four never moved and one moved: 4 * 4! = 96 worlds."""
    st = _blank_state(5, 5, VARIANTS['fives'].max_turns, 6)
    for c, t in enumerate((4, 11, 6, 7)):
        _put(st, -1, 0, c, t)
    _put(st, -1, 1, 4, 5, moved=True)
    for c, t in enumerate((4, 5, 6, 7, 11)):
        _put(st, 1, 4, c, t)
    return st, 96


# ---- step-vs: the agent's actions -------------------------------------------------------------------------------------------------------
VALID, OUT_OF_RANGE, WRONG_PIECE, NOOP = 0, 1, 2, 3
STEP_VS_OUT_SPECS = (('reward', 2, 'float32'), ('done', 1, 'uint8'), ('ending_invalid', 1, 'uint8'), ('player', 1, 'int8'), ('invalid_action', 1, 'uint8'),
                     ('moved', 1, 'uint8'), ('reply_action', 1, 'int32'))


def agent_actions(variant, states, players, index=None, seed=0):
    """One action per slot for the mover of states[index[i]], a seeded mix: mostly a sampled valid action; else a value out of range, a
    valid-looking move of the wrong piece (a move of the OPPONENT's mask, which the mover cannot make) or the no-op while a move exists.
    -> (actions int32 [n], kinds [n]); a kind that a position does not offer falls back to VALID.  (The GPU test uses the same.)"""
    v = VARIANTS[variant] if isinstance(variant, str) else variant
    K = v.spatial_channels
    NA = v.rows * v.columns * K
    noop = K - 1
    idx = np.arange(len(states)) if index is None else np.asarray(index)
    rs = np.random.RandomState(seed)
    actions, kinds = np.empty(len(idx), dtype=np.int32), np.empty(len(idx), dtype=np.int64)
    for i, s in enumerate(idx):
        valid = sv.valid_actions(v, states[s], int(players[s]))
        kind = int(rs.choice([VALID] * 5 + [OUT_OF_RANGE, WRONG_PIECE, NOOP]))
        a = int(valid[rs.randint(len(valid))])
        if kind == OUT_OF_RANGE:
            a = int(rs.choice([-1, NA, NA + 5, 2 ** 31 - 1, -2 ** 31]))
        elif kind == WRONG_PIECE:
            theirs = np.setdiff1d(sv.valid_actions(v, states[s], -int(players[s])), np.append(valid, noop))
            kind, a = (WRONG_PIECE, int(theirs[rs.randint(len(theirs))])) if len(theirs) else (VALID, a)
        elif kind == NOOP:
            kind, a = (NOOP, noop) if valid[0] != noop else (VALID, a)
        actions[i], kinds[i] = a, kind
    return actions, kinds


# ---- start pools: made on the oracle, followed on the oracle -----------------------------------------------------------------------------
STREAM_POOL = 4
SEED, G0 = 0xC0FFEE, 4100
POOL_SEED, POOL_G0, POOL_N = 0x51A7, 900, 24
#        board                 envs steps pool_steps restart_clock  floor    (endings measured on the oracle: 2,711 / 1,230 / 123 / 203 / 59 / 16)
START_POOL_CASES = {'micro': (130, 160, 7, True, 1000),
                    'tiny': (100, 256, 9, True, 500),
                    'fives': (33, 180, 15, True, 60),
                    'short_barrage': (64, 320, 41, True, 100),
                    'barrage': (48, 640, 41, True, 30),
                    'short_standard': (16, 384, 150, False, 8)}


def cvariant_of(v):
    table = S.load_setup_table(v.human_inits) if getattr(v, 'human_inits', None) else None
    return orc.make_cvariant(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, v.initial_state_usable_rows, setups=table)


def make_pool(v, pool_steps, n=POOL_N, seed=POOL_SEED, g0=POOL_G0):
    """The final positions of `n` oracle rollouts of `pool_steps` steps, and their movers."""
    r = orc.rollout_ex(cvariant_of(v), seed, g0, n, pool_steps, want_states=True)
    return r['states'], r['info'][:, 3].astype(np.int8)


class PoolFollower:
    """The start-pool rule on OracleEnv alone.  step() plays one step of every game (auto-reset from the pool) and, given the host copy of
    a slot of GPU outputs, compares whatever tensors it holds."""

    def __init__(self, v, n, states, players, restart_clock, random_first=False, both=False, original=False, seed=SEED, g0=G0, with_obs=True):
        self.v, self.n, self.seed, self.g0 = v, n, seed, g0
        self.states, self.players = np.asarray(states), np.asarray(players)
        self.restart_clock, self.random_first, self.both, self.with_obs = restart_clock, random_first, both, with_obs
        mode = 'both_observations' if both else 'partially_observable'
        self.oenvs = [orc.OracleEnv(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, observation_mode=mode,
                                    obs_channel_mode='original' if original else 'extended') for _ in range(n)]
        self.start_index = np.full(n, -1, dtype=np.int32)
        self.restarts, self.steps, self.touched = 0, 0, set()
        self.first_movers = set()
        self.cur = [None] * n
        for e, oe in enumerate(self.oenvs):
            oe.game_no = -1                # (a fresh handle's counter: the first game a reset starts is number 0)
            self.start(e)

    def start(self, e):
        """the env's next game: from the pool"""
        oe = self.oenvs[e]
        oe.game_no += 1
        g = self.g0 + e
        j = orc.rng_below(orc.rng(self.seed, g, oe.game_no, STREAM_POOL, 0), len(self.states))
        st = self.states[j].copy()
        if self.restart_clock:
            st[5, 0, 0], st[5, 1, 0] = 0, self.v.max_turns
        p = int(self.players[j])
        if self.random_first:
            p = -1 if orc.rng_below(orc.rng(self.seed, g, oe.game_no, STREAM_POOL, 1), 2) == 1 else 1
        o = oe.reset(initial_state_override=st, first_player_override=p)
        self.start_index[e] = j
        self.touched.add(int(j))
        self.first_movers.add(p)
        self.cur[e] = o[p]
        return o

    def drawn(self, e):
        oe = self.oenvs[e]
        return orc.sample_action(self.cur[e][MASK].astype(np.uint8), self.seed, self.g0 + e, oe.game_no, int(oe.state[5, 0, 0]))

    def check_current(self, h, tag='reset'):
        """the outputs of the CURRENT position of every env (after a reset): h = {'obs', 'mask', 'player', 'start_index'[, 'fobs']}"""
        for e, oe in enumerate(self.oenvs):
            o = self.cur[e]
            if 'start_index' in h:
                assert h['start_index'][e] == self.start_index[e], (tag, e, 'start_index')
            assert h['player'][e] == oe.player, (tag, e, 'player')
            assert np.array_equal(o[MASK], h['mask'][e]), (tag, e, 'mask')
            if 'obs' in h:
                assert o[POBS].tobytes() == h['obs'][e].tobytes(), (tag, e, 'observation')
            if 'fobs' in h:
                assert o[FOBS].tobytes() == h['fobs'][e].tobytes(), (tag, e, 'full observation')

    def step(self, acts=None, h=None, tag=''):
        """One step of every game with the actions acts[e] (default: the draw).  h: host arrays of ONE slot, [N, ...] each -- any of mask,
        obs, fobs, reward, done, player, invalid_action, ending_invalid, actions, start_index; compared where present."""
        h = h or {}
        for e, oe in enumerate(self.oenvs):
            a = self.drawn(e) if acts is None else int(acts[e])
            t = (tag, 'step', self.steps, 'env', e)
            o, rew, done, info = oe.step({oe.player: a})              # (the draws are valid actions: the oracle never raises here)
            if 'invalid_action' in h:
                assert h['invalid_action'][e] == 0, t
            if 'done' in h:
                assert bool(h['done'][e]) == done['__all__'], t + ('done',)
            if done['__all__']:
                self.restarts += 1
                if 'reward' in h:
                    assert (h['reward'][e, 0], h['reward'][e, 1]) == (rew[1], rew[-1]), t + ('reward',)
                if 'ending_invalid' in h:
                    assert bool(h['ending_invalid'][e]) == info[1]['game_result_was_invalid'], t + ('ending_invalid',)
                o = self.start(e)
            else:
                if 'reward' in h:
                    assert h['reward'][e, 0] == 0 and h['reward'][e, 1] == 0, t + ('reward',)
                if 'ending_invalid' in h:
                    assert h['ending_invalid'][e] == 0, t
                self.cur[e] = o[oe.player]
            p = oe.player
            if 'player' in h:
                assert h['player'][e] == p, t + ('player',)
            if 'start_index' in h:
                assert h['start_index'][e] == self.start_index[e], t + ('start_index', int(h['start_index'][e]), int(self.start_index[e]))
            if 'mask' in h:
                assert np.array_equal(self.cur[e][MASK], h['mask'][e]), t + ('mask',)
            if 'obs' in h and self.with_obs:
                assert self.cur[e][POBS].tobytes() == h['obs'][e].tobytes(), t + ('observation',)
            if 'fobs' in h:
                assert self.cur[e][FOBS].tobytes() == h['fobs'][e].tobytes(), t + ('full observation',)
            if 'actions' in h:
                assert h['actions'][e] == self.drawn(e), t + ('drawn action',)
        self.steps += 1


def follower_for(name, **kw):
    n, steps, pool_steps, restart, floor = START_POOL_CASES[name]
    v = VARIANTS[name]
    states, players = make_pool(v, pool_steps)
    return PoolFollower(v, n, states, players, restart, **kw), steps, floor
