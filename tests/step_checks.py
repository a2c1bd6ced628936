"""Step checkers the GPU tests and tools/soak_*.py share (support code, no tests): the oracle stepped alongside a GPU rollout, every
output of every step compared.  A test module calls a checker with its parametrised arguments; nothing here touches the GPU at import."""
import hashlib
import os
import re

import numpy as np

from oracle import oracle as orc
from stratego_env_amd import build as hip_build
from stratego_env_amd.config import VARIANTS
from tests.boards import _table
from tests.helpers import FOBS, MASK, POBS, oracle_cvariant, oracle_env
from tests.pool_roots import _sample_states


def _oracle_batch(name, seed, g0, n, observation_mode='partially_observable', channel_mode='extended'):
    """-> (the oracle's variant, n oracle envs at game 0 of env ids g0 .. g0 + n - 1)"""
    v = VARIANTS[name]
    cv = oracle_cvariant(name, setups=_table(name))
    envs = []
    for e in range(n):
        oe = orc.OracleEnv(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, observation_mode=observation_mode,
                           obs_channel_mode=channel_mode)
        oe.reset(initial_state_override=orc.reset_state(cv, seed, g0 + e, 0))
        oe.game_no = 0
        envs.append(oe)
    return cv, envs


def check_step_vs_oracle(name, n_envs, n_steps, garbage, seed_salt=0, require_endings=True, final_obs=True, lane_kernel='auto', emit_obs=True):
    """Random-valid-action rollouts with auto-reset (+ injected garbage actions): every output of every step.
    emit_obs=False (with final_obs=False): the steps pass no observation pointer -- the no-observation kernel kind -- and everything
    else (mask, rewards, flags, sampled action, exported state) is compared as before."""
    assert emit_obs or not final_obs, "final observations need the step's observation: emit_obs %r, final_obs %r" % (emit_obs, final_obs)
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    v = VARIANTS[name]
    seed, g0 = 0xABCDEF12345 + len(name) + 7919 * seed_salt, 1000 + 31 * seed_salt
    env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True, final_obs=final_obs)
    env.set_lane_kernel(lane_kernel)
    cv, oenvs = _oracle_batch(name, seed, g0, n_envs)
    NA = v.num_spatial_actions
    rs = np.random.RandomState(7 + seed_salt)
    obs, mask, player = env.reset()
    obs_h, mask_h, player_h = obs.cpu().numpy(), mask.cpu().numpy(), player.cpu().numpy()
    cur = []
    for e, oe in enumerate(oenvs):
        o = oe._obs(1)
        assert np.array_equal(o[MASK], mask_h[e]) and o[POBS].tobytes() == obs_h[e].tobytes(), (name, 'reset', e)
        assert player_h[e] == 1, (name, 'reset', e, 'player', int(player_h[e]))
        cur.append(o)
    st, pl = env.export_state()
    assert np.array_equal(st.cpu().numpy(), np.stack([oe.state for oe in oenvs])), (name, 'reset', 'state export')
    sampled = env.sample_valid_actions().cpu().numpy()
    games_done = 0
    for t in range(n_steps):
        acts = np.zeros(n_envs, dtype=np.int32)
        for e, oe in enumerate(oenvs):
            a = orc.sample_action(cur[e][MASK].astype(np.uint8), seed, g0 + e, oe.game_no, int(oe.state[5, 0, 0]))
            assert sampled[e] == a, (name, t, e, 'sampler')
            if garbage and rs.rand() < garbage:
                a = int(rs.choice([rs.randint(NA), rs.randint(v.cells) * v.spatial_channels + v.spatial_channels - 1,
                                   -1, NA, NA + 3, (v.cells - 1) * v.spatial_channels + rs.randint(v.spatial_channels)]))
            acts[e] = a
        env.step(torch.from_numpy(acts), want_next_actions=True, emit_obs=emit_obs)
        obs_h, mask_h = env.obs.cpu().numpy(), env.mask.cpu().numpy()
        rew_h, done_h, player_h = env.reward.cpu().numpy(), env.done.cpu().numpy(), env.player.cpu().numpy()
        inv_h, einv_h = env.invalid_action.cpu().numpy(), env.ending_invalid.cpu().numpy()
        fin_h = env.final_obs.cpu().numpy() if final_obs else None
        sampled = env.next_actions.cpu().numpy()
        for e, oe in enumerate(oenvs):
            try:
                o, rew, done, info = oe.step({oe.player: int(acts[e])})
            except ValueError:
                assert inv_h[e] == 1, (name, t, e, acts[e], 'oracle raised, GPU accepted')
                assert not done_h[e], (name, t, e, acts[e], 'a refused action ended the game')
                assert np.array_equal(cur[e][MASK], mask_h[e]) and (not emit_obs or cur[e][POBS].tobytes() == obs_h[e].tobytes()), \
                    (name, t, e, acts[e], 'a refused action changed the mask or the observation')
                assert player_h[e] == oe.player, (name, t, e, 'player after a refused action', int(player_h[e]), oe.player)
                continue
            assert inv_h[e] == 0, (name, t, e, acts[e], 'GPU flagged a move the oracle accepts')
            assert bool(done_h[e]) == done['__all__'], (name, t, e)
            if done['__all__']:
                games_done += 1
                assert (rew_h[e, 0], rew_h[e, 1]) == (rew[1], rew[-1]), (name, t, e, rew_h[e], rew)
                assert bool(einv_h[e]) == info[1]['game_result_was_invalid'], (name, t, e, 'ending_invalid', int(einv_h[e]), info[1]['game_result_was_invalid'])
                for slot, p in ((0, 1), (1, -1)):
                    assert fin_h is None or o[p][POBS].tobytes() == fin_h[e, slot].tobytes(), (name, t, e, 'final obs', p)
                    assert int(o[p][MASK].sum()) == 1 and o[p][MASK][0, 0, -1] == 1, (name, t, e, 'terminal mask of the oracle', p, int(o[p][MASK].sum()))
                oe.game_no += 1
                o = oe.reset(initial_state_override=orc.reset_state(cv, seed, g0 + e, oe.game_no))
            else:
                assert rew_h[e, 0] == 0 and rew_h[e, 1] == 0 and einv_h[e] == 0, (name, t, e, 'a running game', rew_h[e], int(einv_h[e]))
            p = oe.player
            assert player_h[e] == p, (name, t, e)
            assert np.array_equal(o[p][MASK], mask_h[e]), (name, t, e, 'mask')
            assert not emit_obs or o[p][POBS].tobytes() == obs_h[e].tobytes(), (name, t, e, 'obs')
            cur[e] = o[p]
        if t % 50 == 49:
            st, pl = env.export_state()
            assert np.array_equal(st.cpu().numpy(), np.stack([oe.state for oe in oenvs])), (name, t, 'state export')
            assert np.array_equal(pl.cpu().numpy(), np.asarray([oe.player for oe in oenvs], dtype=np.int8)), (name, t, 'player export', pl.cpu().numpy().tolist())
    assert games_done > 0 or not require_endings or name in ('standard', 'standard2', 'medium_standard', 'short_standard', 'c12x12', 'c20x20', 'c17x16', 'c32x32'), \
        (name, n_steps, 'no game ended')
    env.close()


def check_functional_api_vs_oracle(name):
    """Every method of the batched functional API on states sampled along golden games, for both players, against OracleRules."""
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    v = VARIANTS[name]
    rs = np.random.RandomState(11)
    n = 96
    states, players = _sample_states(name, n, rs)
    ru = orc.OracleRules(v.rows, v.columns)
    pe = BatchedStrategoProceduralEnv(name, n)
    assert pe.action_size == ru.action_size and tuple(pe.spatial_action_size) == ru.spatial_action_size, \
        (name, 'action sizes', pe.action_size, ru.action_size, tuple(pe.spatial_action_size), ru.spatial_action_size)
    # masks, perspective, observations, game-ended for BOTH players on every state
    for pl_all in (players, -players):
        m1 = pe.get_valid_moves_as_1d_mask(states, pl_all).cpu().numpy()
        ms = pe.get_valid_moves_as_spatial_mask(states, pl_all).cpu().numpy()
        pp = pe.get_state_from_player_perspective(states, pl_all).cpu().numpy()
        po = pe.get_partially_observable_observation_extended_channels(states, pl_all).cpu().numpy()
        fo = pe.get_fully_observable_observation_extended_channels(states, pl_all).cpu().numpy()
        ge = pe.get_game_ended(states, pl_all).cpu().numpy()
        gi = pe.get_game_result_is_invalid(states).cpu().numpy()
        # the other observation kinds (79-channel, 'original' channels): three launches on packed records first, then the same second pass
        others = []
        for fn_name in ('get_fully_observable_observation_extended_channels', 'get_partially_observable_observation',
                        'get_fully_observable_observation'):
            others.append((fn_name, getattr(pe, fn_name)(states, pl_all).cpu().numpy()))
            assert int(pe.last_sanitised.sum()) == 0, (name, fn_name)
        for e in range(n):
            p = int(pl_all[e])
            for fn_name, got in others:
                assert got[e].tobytes() == getattr(ru, fn_name)(states[e], p).tobytes(), (name, e, fn_name)
            assert np.array_equal(m1[e], ru.get_valid_moves_as_1d_mask(states[e], p)), (name, e, '1d mask')
            assert np.array_equal(ms[e], ru.get_valid_moves_as_spatial_mask(states[e], p)), (name, e, 'spatial mask')
            assert np.array_equal(pp[e], ru.get_state_from_player_perspective(states[e], p)), (name, e, 'perspective')
            assert po[e].tobytes() == ru.get_partially_observable_observation_extended_channels(states[e], p).tobytes(), (name, e, 'partial obs')
            assert fo[e].tobytes() == ru.get_fully_observable_observation_extended_channels(states[e], p).tobytes(), (name, e, 'full obs')
            assert np.float32(ge[e]) == np.float32(ru.get_game_ended(states[e], p)), (name, e, 'game ended', float(ge[e]), ru.get_game_ended(states[e], p))
            assert bool(gi[e]) == ru.get_game_result_is_invalid(states[e]), (name, e, 'result is invalid', bool(gi[e]))
    # transitions: valid moves, garbage indices, the 1-D no-op, with and without oscillation
    for rnd in range(6):
        acts = np.zeros(n, dtype=np.int64)
        for e in range(n):
            mask = ru.get_valid_moves_as_1d_mask(states[e], int(players[e]))
            kind = rs.randint(4)
            if kind < 2:
                acts[e] = rs.choice(np.flatnonzero(mask))
            elif kind == 2:
                acts[e] = rs.randint(-5, ru.action_size + 5)
            else:
                acts[e] = ru.action_size - 1
        for osc in (False, True):
            ns, npl, valid = pe.get_next_state(states, players, acts, allow_piece_oscillation=osc)
            ns, npl, valid = ns.cpu().numpy(), npl.cpu().numpy(), valid.cpu().numpy()
            v2 = pe.is_move_valid_by_1d_index(states, players, acts, allow_piece_oscillation=osc).cpu().numpy()
            for e in range(n):
                want_valid = ru.is_move_valid_by_1d_index(states[e], int(players[e]), int(acts[e]), allow_piece_oscillation=osc)
                assert bool(valid[e]) == want_valid == bool(v2[e]), (name, rnd, e, acts[e], osc)
                if want_valid:
                    w, wp = ru.get_next_state(states[e], int(players[e]), int(acts[e]), allow_piece_oscillation=osc)
                    assert np.array_equal(ns[e], w) and npl[e] == wp, (name, rnd, e, 'next state')
                else:
                    assert np.array_equal(ns[e], states[e]) and npl[e] == players[e], (name, rnd, e, acts[e], osc, 'a refused move changed the state')
    # validity by raw positions (diagonals, out-of-board, long moves)
    pos = rs.randint(-1, max(v.rows, v.columns) + 1, size=(n, 4))
    for osc in (False, True):
        got = pe.is_move_valid_by_position(states, players, pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3], allow_piece_oscillation=osc).cpu().numpy()
        for e in range(n):
            assert bool(got[e]) == ru.is_move_valid_by_position(states[e], int(players[e]), *[int(x) for x in pos[e]], allow_piece_oscillation=osc), \
                (name, e, pos[e].tolist(), osc, 'validity by position', bool(got[e]))
    pe.close()


def digest_both(obs):
    h = hashlib.sha256()
    for p in sorted(obs.keys()):
        h.update(np.ascontiguousarray(obs[p]['valid_actions_mask']).astype(np.uint8).tobytes())
        h.update(np.ascontiguousarray(obs[p]['partial_observation'], dtype=np.float32).tobytes())
        h.update(np.ascontiguousarray(obs[p]['full_observation'], dtype=np.float32).tobytes())
    return int.from_bytes(h.digest()[:8], 'little')


def check_both_obs_vs_oracle(name, n_envs, n_steps, channel_mode):
    """BOTH_OBSERVATIONS rollouts with auto-reset: both observations, the terminal ones and the mask of every step against the oracle."""
    from stratego_env_amd.vec_env import VecStrategoEnv
    seed, g0 = 0x77AA55 + len(name), 500
    env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True, final_obs=True, full_obs=True,
                         obs_channel_mode=channel_mode)
    cv, oenvs = _oracle_batch(name, seed, g0, n_envs, 'both_observations', channel_mode)
    env.reset()
    fobs_h, obs_h, mask_h = env.fobs.cpu().numpy(), env.obs.cpu().numpy(), env.mask.cpu().numpy()
    cur = []
    for e, oe in enumerate(oenvs):
        o = oe._obs(1)
        assert o[FOBS].tobytes() == fobs_h[e].tobytes() and o[POBS].tobytes() == obs_h[e].tobytes(), (name, 'reset', e, 'full or partial obs')
        cur.append(o)
    env.sample_valid_actions()
    ended = 0
    for t in range(n_steps):
        acts = env.next_actions.cpu().numpy().copy()
        env.rollout_step()
        fobs_h, obs_h, mask_h = env.fobs.cpu().numpy(), env.obs.cpu().numpy(), env.mask.cpu().numpy()
        done_h, ff_h, fp_h = env.done.cpu().numpy(), env.final_fobs.cpu().numpy(), env.final_obs.cpu().numpy()
        for e, oe in enumerate(oenvs):
            o, rew, done, info = oe.step({oe.player: int(acts[e])})
            assert bool(done_h[e]) == done['__all__'], (name, t, e, 'done', int(done_h[e]), done['__all__'])
            if done['__all__']:
                ended += 1
                for slot, p in ((0, 1), (1, -1)):
                    assert o[p][FOBS].tobytes() == ff_h[e, slot].tobytes(), (name, t, e, 'final full obs', p)
                    assert o[p][POBS].tobytes() == fp_h[e, slot].tobytes(), (name, t, e, 'final partial obs', p)
                oe.game_no += 1
                o = oe.reset(initial_state_override=orc.reset_state(cv, seed, g0 + e, oe.game_no))
            p = oe.player
            assert o[p][FOBS].tobytes() == fobs_h[e].tobytes(), (name, t, e, 'full obs')
            assert o[p][POBS].tobytes() == obs_h[e].tobytes(), (name, t, e, 'partial obs')
            assert np.array_equal(o[p][MASK], mask_h[e]), (name, t, e, 'mask')
    assert ended > 0 or name in ('standard', 'standard2'), (name, n_steps, 'no game ended')
    env.close()


def _poison(traj):
    import torch
    for k, t in traj.items():
        if t.dtype == torch.float32:
            t.fill_(float('nan'))
        elif t.dtype == torch.int32:
            t.fill_(-12345)
        else:
            t.fill_(0x5A)


class Follower:
    """The oracle stepped alongside a batch of GPU games: check_slot() plays ONE step of every game on the oracle and compares it with one
    slot of a trajectory buffer (already on the host)."""

    def __init__(self, name, seed, g0, n, auto_reset, both=False, with_obs=True):
        self.name, self.seed, self.g0, self.n, self.auto_reset, self.both = name, seed, g0, n, auto_reset, both
        self.with_obs = with_obs               # False: the rollout writes no observation (the no-observation kernel kind): masks, results and draws only
        self.cv, self.oenvs = _oracle_batch(name, seed, g0, n, 'both_observations' if both else 'partially_observable')
        self.cur = [oe._obs(1) for oe in self.oenvs]
        self.finished = [False] * n            # (without auto-reset: a finished game only takes invalid actions from then on)
        self.games_done = 0
        self.steps = 0

    def drawn(self, e):
        """the action the rollout plays next for game e: k-th valid of the current mask, k from the counter RNG (maenv:830-834 for a batch)"""
        oe = self.oenvs[e]
        return orc.sample_action(self.cur[e][MASK].astype(np.uint8), self.seed, self.g0 + e, oe.game_no, int(oe.state[5, 0, 0]))

    def check_reset(self, obs_h, mask_h, fobs_h=None):
        for e in range(self.n):
            o = self.cur[e]
            assert np.array_equal(o[MASK], mask_h[e]) and o[POBS].tobytes() == obs_h[e].tobytes(), (self.name, 'reset', e)
            assert fobs_h is None or o[FOBS].tobytes() == fobs_h[e].tobytes(), (self.name, 'reset', e, 'full observation')

    def check_slot(self, acts, h, s, what):
        """acts[e]: the action game e plays in this step; h: dict of host arrays with a leading slot axis; s: the slot this step wrote."""
        tag = (self.name, what, 'step', self.steps, 'slot', s)
        for e, oe in enumerate(self.oenvs):
            a = int(acts[e])
            try:
                if self.finished[e]:
                    raise ValueError
                o, rew, done, info = oe.step({oe.player: a})
            except ValueError:
                assert h['invalid_action'][s, e] == 1, tag + (e, a, 'the oracle raises, the GPU accepted')
                assert h['done'][s, e] == (1 if self.finished[e] else 0), tag + (e,)
                assert np.array_equal(self.cur[e][MASK], h['mask'][s, e]), tag + (e, 'mask after an invalid action')
                assert not self.with_obs or self.cur[e][POBS].tobytes() == h['obs'][s, e].tobytes(), tag + (e, 'observation after an invalid action')
                assert h['player'][s, e] == oe.player, tag + (e, 'player after an invalid action', int(h['player'][s, e]), oe.player)
                assert h['actions'][s, e] == self.drawn(e), tag + (e, 'draw after an invalid action')
                continue
            assert h['invalid_action'][s, e] == 0, tag + (e, a, 'the GPU flags a move the oracle accepts')
            assert bool(h['done'][s, e]) == done['__all__'], tag + (e, 'done')
            if done['__all__']:
                self.games_done += 1
                assert (h['reward'][s, e, 0], h['reward'][s, e, 1]) == (rew[1], rew[-1]), tag + (e, 'reward')
                assert bool(h['ending_invalid'][s, e]) == info[1]['game_result_was_invalid'], tag + (e, 'ending_invalid')
                if self.auto_reset:
                    oe.game_no += 1
                    o = oe.reset(initial_state_override=orc.reset_state(self.cv, self.seed, self.g0 + e, oe.game_no))
                else:
                    self.finished[e] = True
                    o = {oe.player: o[oe.player]}                     # both terminal observations: the mover's is what the slot holds
            else:
                assert h['reward'][s, e, 0] == 0 and h['reward'][s, e, 1] == 0 and h['ending_invalid'][s, e] == 0, tag + (e,)
            p = oe.player
            assert h['player'][s, e] == p, tag + (e, 'player')
            assert np.array_equal(o[p][MASK], h['mask'][s, e]), tag + (e, 'mask')
            assert not self.with_obs or o[p][POBS].tobytes() == h['obs'][s, e].tobytes(), tag + (e, 'observation')
            if self.both:
                assert o[p][FOBS].tobytes() == h['fobs'][s, e].tobytes(), tag + (e, 'full observation')
            self.cur[e] = o[p]
            assert h['actions'][s, e] == self.drawn(e), tag + (e, 'drawn action')
        self.steps += 1


def _host(traj):
    return {k: t.cpu().numpy() for k, t in traj.items()}


def _multi_kinds():
    from stratego_env_amd import _lib
    return (_lib.LAUNCH_MULTI_STEP_WAVE, _lib.LAUNCH_MULTI_STEP)


def check_every_step_vs_oracle(name, n_envs, chunk, n_calls, garbage, both=False, auto_reset=True, kw=None, emit_obs=True, seed_salt=0):
    """Calls of `chunk` steps into a trajectory buffer of `chunk` slots: every slot of every call against the oracle.  Some games start
    every call from a garbage action (flagged, state unchanged, the same draw again); games end and restart inside the launches and across
    their boundaries."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    v = VARIANTS[name]
    seed, g0 = 0x7A3B00 + 97 * len(name) + n_envs + 104729 * seed_salt, 7000 + 13 * seed_salt       # (tools/soak_trajectory.py varies the salt)
    env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=auto_reset, full_obs=both, **(kw or {}))
    fo = Follower(name, seed, g0, n_envs, auto_reset, both, with_obs=emit_obs)
    env.reset()
    fo.check_reset(env.obs.cpu().numpy(), env.mask.cpu().numpy(), env.fobs.cpu().numpy() if both else None)
    env.sample_valid_actions()
    traj = env.alloc_trajectory(chunk)
    rs = np.random.RandomState(11 + seed_salt)
    NA = v.num_spatial_actions
    for call in range(n_calls):
        nxt = env.next_actions.cpu().numpy().copy()
        for e in range(n_envs):
            assert nxt[e] == fo.drawn(e), (name, call, e, 'the draw a call starts from')
            if rs.rand() < garbage:
                nxt[e] = int(rs.choice([rs.randint(NA), -1, NA + 5, rs.randint(v.cells) * v.spatial_channels + v.spatial_channels - 1]))
        env.next_actions.copy_(torch.from_numpy(nxt))
        _poison(traj)
        env.rollout_trajectory(chunk, traj, emit_obs=emit_obs)
        assert env.last_launch_kind in _multi_kinds(), (name, 'the test must not pass on the per-step kernel')
        if not emit_obs:
            assert bool(torch.isnan(traj['obs']).all()), 'a rollout without an observation pointer must not touch the observation slots'
        h = _host(traj)
        acts = nxt
        for s in range(chunk):
            fo.check_slot(acts, h, s, 'call %d' % call)
            acts = h['actions'][s]
        # the env's own views are the last slot
        assert env.obs.data_ptr() == traj['obs'][chunk - 1].data_ptr() and torch.equal(env.next_actions, traj['actions'][chunk - 1]), \
            (name, call, "the env's own views are not the last slot")
    st, pl = env.export_state()
    assert np.array_equal(st.cpu().numpy(), np.stack([oe.state for oe in fo.oenvs])), (name, 'final states')
    assert np.array_equal(pl.cpu().numpy(), np.asarray([oe.player for oe in fo.oenvs], dtype=np.int8)), (name, 'final players', pl.cpu().numpy().tolist())
    if auto_reset:
        assert fo.games_done > 0 or name in ('standard', 'standard2'), (name, n_calls, chunk, 'no game ended')
    env.close()


def _kernel_resources(tmp_path):
    """{mangled kernel name: {vgpr, sgpr, scratch, lds}} read from the gfx950 code object inside the SHIPPED library (the notes of the
    offload bundle: what the GPU box will run, and seconds instead of the minutes of a fresh hipcc -S)."""
    import shutil
    import subprocess
    llvm = '/opt/rocm/lib/llvm/bin'
    so = tmp_path / 'lib.so'
    hip_build.build()                                  # (a no-op when the library matches the sources: its build id is their hash)
    shutil.copy(hip_build.LIB_PATH, so)
    subprocess.check_call([os.path.join(llvm, 'llvm-objdump'), '--offloading', str(so)], stdout=subprocess.DEVNULL, cwd=str(tmp_path))
    cos = [f for f in os.listdir(tmp_path) if 'gfx950' in f]
    assert len(cos) == 1, cos
    notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', str(tmp_path / cos[0])], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
        g = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        res[re.search(r'\.name:\s+(\S+)', blk).group(1)] = dict(vgpr=g('vgpr_count'), sgpr=g('sgpr_count'), scratch=g('private_segment_fixed_size'),
                                                                 lds=g('group_segment_fixed_size'))
    return res
