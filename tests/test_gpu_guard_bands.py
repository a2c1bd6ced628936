"""Guard bands: no kernel may write outside the caller's tensors, at any pointer phase the contract of include/stratego_mi355x.h allows.

Every output tensor of a call lives in an ARENA (tests/guard_bands.py): guard | payload | guard in one uint8 device tensor whose base is 1 KiB aligned.  The
guards (>= 4 KiB each: more than a 1 KiB store sweep plus a 128-byte line) hold the word 0x7FC0DEAD, the payload is poisoned with the word
0x7FA55A5A -- both NaNs as float32, neither a byte a mask / flag / player can hold nor an action or a state value -- and starts `phase` bytes
past a 1 KiB boundary.  After every library call (and a synchronise) the checks run in this order: (1) every guard byte still holds its
pattern; (2) nothing the call's contract says is written still holds the poison; (3) the payload equals the CPU ORACLE stepped alongside.
A phase the contract refuses is tested by its SGX_EINVAL: the call launches nothing and the arenas keep their poison.

tools/mutant_check.sh runs this file against three builds with a deliberately stray store each (profiles/r07_guard_band_mutants.log)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS
from tests.boards import CUSTOM, registered
from tests.guard_bands import (Arena, F32_ODD_PHASES, F32_QUAD_PHASES, I32_PHASES, U8_PHASES, _compare, _guards, _load_actions, _make, _phase_set, _play,
                               _swap_outputs, _sync, _written_after_step)

pytestmark = pytest.mark.gpu

MASK, POBS, FOBS = 'valid_actions_mask', 'partial_observation', 'full_observation'


@pytest.fixture(autouse=True)
def _custom_names():
    yield from registered(CUSTOM)


def _quad(name):
    return VARIANTS[name].cells % 4 == 0


def _garbage(acts, rs, v, rate):
    acts = acts.copy()
    for e in range(len(acts)):
        if rs.rand() < rate:
            acts[e] = int(rs.choice([-1, v.num_spatial_actions + 5, rs.randint(v.num_spatial_actions)]))
    return acts


# ---- sgx_step / sgx_observe: one launch per step -------------------------------------------------------------------------------------
# batch sizes: 1, one game fewer / more than a workgroup plays (8 on boards of more than 32 cells, 16 on 5x5, 32 on boards of up to 16 cells,
# 4 on 3x40), a prime around 250
STEP_CASES = [
    # name, n_envs, steps, env kwargs, first phase set
    ('barrage', 1, 12, dict(final_obs=True), 0), ('barrage', 7, 22, dict(final_obs=True), 0), ('barrage', 9, 12, dict(final_obs=True, full_obs=True), 3),
    ('barrage', 251, 6, dict(final_obs=True), 1), ('barrage', 9, 8, dict(channel_mode='original', full_obs=True), 5),
    ('standard2', 1, 12, dict(final_obs=True), 0), ('standard2', 7, 12, dict(final_obs=True, full_obs=True), 2), ('standard2', 9, 6, dict(channel_mode='original'), 4),
    ('fives', 15, 24, dict(final_obs=True), 0), ('fives', 17, 12, dict(final_obs=True, full_obs=True), 1), ('fives', 251, 6, dict(final_obs=True), 3),
    ('fives', 1, 12, dict(channel_mode='original', full_obs=True), 2),
    ('medium', 7, 22, dict(final_obs=True), 0), ('medium', 9, 8, dict(final_obs=True, full_obs=True), 6), ('medium', 257, 4, dict(), 2),
    ('octa_barrage', 9, 22, dict(final_obs=True), 4), ('octa_barrage', 1, 8, dict(full_obs=True), 7),
    ('tiny', 31, 22, dict(final_obs=True), 0), ('tiny', 33, 8, dict(final_obs=True, full_obs=True), 5), ('tiny', 1, 8, dict(), 9),
    ('micro', 33, 22, dict(final_obs=True), 2), ('micro', 31, 8, dict(channel_mode='original'), 6), ('micro', 251, 6, dict(final_obs=True), 8),
    ('c3x40', 3, 12, dict(final_obs=True), 0), ('c3x40', 5, 8, dict(final_obs=True), 5),
    ('octa_barrage', 7, 8, dict(final_obs=True), 1), ('octa_barrage', 251, 4, dict(), 3), ('medium', 1, 8, dict(final_obs=True), 4),
    ('standard2', 251, 4, dict(), 1), ('tiny', 251, 6, dict(final_obs=True), 3), ('micro', 1, 8, dict(final_obs=True), 0),
    ('micro', 63, 8, dict(final_obs=True), 4), ('micro', 65, 8, dict(full_obs=True), 7),
]


@pytest.mark.parametrize('name,n_envs,steps,kw,k0', STEP_CASES)
def test_step_and_observe_stay_inside_their_tensors(name, n_envs, steps, kw, k0):
    """sgx_step (67-channel / BOTH / 'original' channels, terminal observations) and sgx_observe: every pair of steps runs one phase set with
    plain and with non-temporal stores; garbage actions and auto-reset included."""
    import torch
    from stratego_env_amd import _lib
    kw = dict(kw)
    env, ora = _make(name, n_envs, auto_reset=True, **kw)
    v, quad = VARIANTS[name], _quad(name)
    rs = np.random.RandomState(n_envs + steps)
    ar = _swap_outputs(env, _phase_set(k0, quad))
    env.reset()
    _sync(env)
    _guards(ar, 'reset')
    for k in ('obs', 'fobs', 'mask', 'player'):
        if k in ar:
            ar[k].check_written('reset')
    _compare({k: ar[k] for k in ('obs', 'fobs', 'mask', 'player') if k in ar}, ora.current(), (name, 'reset'))
    env.sample_valid_actions()
    _sync(env)
    _guards(ar, 'sample')
    assert np.array_equal(ar['next_actions'].host(), ora.current()['next_actions'])
    acts = ar['next_actions'].host().copy()
    for t in range(steps):
        nt = bool(t & 1)
        env.set_nt_stores(nt)
        ar = _swap_outputs(env, _phase_set(k0 + t // 2, quad))
        acts = _garbage(acts, rs, v, 0.1)
        what = (name, n_envs, 'step', t, 'nt', nt, 'phase set', k0 + t // 2)
        env.step(torch.from_numpy(acts), want_next_actions=True)
        _sync(env)
        assert env.last_launch_kind == _lib.LAUNCH_WAVE, what
        x = ora.step(acts)
        _guards(ar, what)
        _written_after_step(ar, x, what)
        _compare(ar, x, what)
        acts = x['next_actions'].copy()
        # sgx_observe of the same position into fresh arenas at the next phase set
        ob = _swap_outputs(env, _phase_set(k0 + t // 2 + 1, quad), names=('obs', 'fobs', 'mask', 'player'))
        env.observe()
        _sync(env)
        _guards(ob, what + ('observe',))
        for a in ob.values():
            a.check_written(what + ('observe',))
        _compare(ob, {k: x[k] for k in ('obs', 'fobs', 'mask', 'player')}, what + ('observe',))
    if name in ('fives', 'tiny', 'micro') and steps >= 20:
        assert ora.games_done > 0, 'no game ended: the terminal observations were never written'
    env.close()


def test_standard_mid_game_uncoded_entries():
    """Standard far enough into the games for captured miners / majors / bombs (values without a 4-bit code): patch_uncoded's whole-quad stores
    next to the sweep, with both store policies, at the last steps of a 330-step rollout."""
    import torch
    env, ora = _make('standard', 9, auto_reset=True, final_obs=True)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    for t in range(330):
        check = t >= 318
        if check:
            env.set_nt_stores(bool(t & 1))
            ar = _swap_outputs(env, _phase_set(t // 2, True))
        env.step(torch.from_numpy(acts), want_next_actions=True)
        x = ora.step(acts)
        if check:
            _sync(env)
            what = ('standard', 'step', t)
            _guards(ar, what)
            _written_after_step(ar, x, what)
            _compare(ar, x, what)
        acts = x['next_actions'].copy()
    thirds = np.stack([c[POBS] for c in ora.cur])
    assert np.any((thirds != 0) & (np.abs(thirds) != 1) & (np.abs(thirds) != 0.5) & (np.abs(thirds) != 0.25) & (np.abs(thirds) != 0.75)), \
        'no uncoded entry in any observation: the rollout is too short for what this test is for'
    env.close()


@pytest.mark.parametrize('name,n_envs', [('barrage', 9), ('fives', 17), ('medium', 7), ('tiny', 33), ('standard2', 3), ('barrage', 1), ('octa_barrage', 251),
                                         ('micro', 63), ('micro', 65), ('c3x40', 5)])
def test_mask_only_steps(name, n_envs):
    """emit_obs=False: the no-observation kernel kind (two games per wave on 6x6 ... 10x10); the mask at every uint8 phase, the observation
    arenas untouched."""
    import torch
    env, ora = _make(name, n_envs, auto_reset=True)
    quad = _quad(name)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    for t in range(len(U8_PHASES)):
        ar = _swap_outputs(env, _phase_set(t, quad))
        what = (name, 'mask-only step', t)
        env.step(torch.from_numpy(acts), want_next_actions=True, emit_obs=False)
        _sync(env)
        x = ora.step(acts)
        _guards(ar, what)
        _written_after_step(ar, x, what, emit_obs=False)
        _compare(ar, x, what, emit_obs=False)
        acts = x['next_actions'].copy()
    env.close()


@pytest.mark.parametrize('name,n_envs,both', [('barrage', 1, False), ('barrage', 7, True), ('octa_barrage', 8, False), ('medium', 3, True), ('standard', 2, False),
                                              ('fives', 2, False)])
def test_step_sync(name, n_envs, both):
    """sgx_step_sync: up to 8 games on a board of more than 32 cells with a multiple of 4 cells run single_kernel (a workgroup per game, all
    eight waves emit: emit_mask / emit_codes with a stride of 512 lanes); 5x5 takes sgx_step + a synchronise behind the same entry point."""
    import torch
    env, ora = _make(name, n_envs, auto_reset=True, full_obs=both, final_obs=True)
    quad = _quad(name)
    env.reset()
    acts = env.sample_valid_actions().cpu().numpy().copy()
    for t in range(len(U8_PHASES)):
        ar = _swap_outputs(env, _phase_set(t, quad))
        what = (name, n_envs, 'step_sync', t)
        env.step_sync(torch.from_numpy(acts))
        x = ora.step(acts)
        _sync(env)
        _guards(ar, what)
        na = ar.pop('next_actions')
        na.check_untouched(what)
        _written_after_step(ar, x, what)
        _compare(ar, x, what)
        acts = x['next_actions'].copy()
    env.close()


@pytest.mark.parametrize('name,n_envs', [('barrage', 9), ('fives', 15), ('standard2', 3), ('micro', 33), ('standard', 7)])
def test_compact_outputs_and_their_decoders(name, n_envs):
    """Compact steps (16-byte aligned records between guards), then sgx_decode_obs / sgx_decode_mask into float32 / uint8 arenas at every
    phase of the contract: decoded bytes = the oracle's."""
    import torch
    env, ora = _make(name, n_envs, auto_reset=True, compact_outputs=True)
    quad = _quad(name)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    shape_o, shape_m = (n_envs, env.R, env.Cc, env.p_channels), (n_envs, env.R, env.Cc, env.K)
    for t in range(len(U8_PHASES)):
        ph = _phase_set(t, quad)
        ar = _swap_outputs(env, dict(ph, obs=F32_QUAD_PHASES[t % 4], mask=F32_QUAD_PHASES[(t + 1) % 4]))
        what = (name, 'compact step', t)
        env.step(torch.from_numpy(acts), want_next_actions=True)
        _sync(env)
        x = ora.step(acts)
        _guards(ar, what)
        for k in ('reward', 'done', 'player', 'invalid_action', 'ending_invalid', 'next_actions'):
            ar[k].check_written(what)
        dec = {'obs': Arena('decoded obs', shape_o, torch.float32, ph['obs'], env.device), 'mask': Arena('decoded mask', shape_m, torch.uint8, ph['mask'], env.device)}
        env.set_nt_stores(bool(t & 1))
        env.decode_obs(out=dec['obs'].t)
        env.decode_mask(out=dec['mask'].t)
        _sync(env)
        _guards(dec, what + ('decode',))
        _guards(ar, what + ('decode',))
        for a in dec.values():
            a.check_written(what + ('decode',))
        _compare(dict(ar, **dec), x, what)
        acts = x['next_actions'].copy()
    env.close()


# ---- multi-step launches -------------------------------------------------------------------------------------------------------------
MULTI_CASES = [('barrage', 7), ('barrage', 9), ('barrage', 251), ('standard2', 1), ('standard2', 9), ('fives', 15), ('fives', 17), ('medium', 9), ('medium', 257),
               ('octa_barrage', 7), ('tiny', 33), ('micro', 31), ('c3x40', 5), ('micro', 521), ('fives', 263)]


@pytest.mark.parametrize('name,n_envs', MULTI_CASES)
def test_step_n_and_chained_rollouts(name, n_envs):
    """sgx_step_n (the multi-step kernel) and sgx_rollout(chains=2) (per-step launches with env_first != 0): the outputs hold the last step's
    results, with BOTH observations and without."""
    from stratego_env_amd import _lib
    both = n_envs % 2 == 1 and name != 'c3x40'
    env, ora = _make(name, n_envs, auto_reset=True, full_obs=both)
    quad = _quad(name)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    k = 0
    for chains, n_steps in ((1, 5), (2, 3), (1, 2), (2, 4), (1, 7), (1, 3)):
        for nt in (False, True):
            env.set_nt_stores(nt)
            ar = _swap_outputs(env, _phase_set(k, quad))
            what = (name, n_envs, 'chains', chains, 'steps', n_steps, 'nt', nt, 'phase set', k)
            k += 1
            _load_actions(env, acts)
            env.rollout_steps(n_steps, chains=chains)
            _sync(env)
            lanes_missed = (ar['obs'].phase | ar['mask'].phase | ar['next_actions'].phase) & 15 or ar['reward'].phase & 7
            # (sgx_rollout splits the batch only when every chain gets whole groups of eight workgroups; smaller batches are sgx_step_n)
            cells = VARIANTS[name].cells
            unit = 64 * (4 if cells <= 16 else 2 if cells <= 32 else 1)
            if chains == 2 and (n_envs // 2) // unit > 0:
                want = (_lib.LAUNCH_WAVE, _lib.LAUNCH_LANE)               # one launch per step and chain: env_first != 0 in the second chain
            else:
                want = (_lib.LAUNCH_MULTI_STEP,) if (cells <= 16 and not both and not lanes_missed) else (_lib.LAUNCH_MULTI_STEP_WAVE,)
            assert env.last_launch_kind in want, what + ('kind', env.last_launch_kind)
            xs = _play(ora, acts, n_steps)
            x = xs[-1]
            x['final'] = {}                                   # (no terminal-observation buffers here)
            _guards(ar, what)
            _written_after_step(ar, x, what)
            _compare(ar, x, what)
            acts = x['next_actions'].copy()
    env.close()


@pytest.mark.parametrize('name,n_envs,n_sets', [('barrage', 9, 3), ('barrage', 7, 11), ('fives', 17, 3), ('fives', 15, 10), ('standard2', 3, 9), ('medium', 9, 3),
                                                 ('micro', 33, 3), ('tiny', 31, 9)])
def test_step_ring(name, n_envs, n_sets):
    """sgx_step_ring with 3 sets (pointers in the kernel arguments) and with more than 8 (the device table): every set its own arenas at its own
    phases; after a call each set holds the step that wrote it last."""
    from stratego_env_amd import _lib
    env, ora = _make(name, n_envs, auto_reset=True, full_obs=(n_sets == 3 and name != 'micro'))
    quad = _quad(name)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    pos = 1
    for call, n_steps in enumerate((n_sets + 2, 2, n_sets)):
        nt = bool(call & 1)
        env.set_nt_stores(nt)
        res = _swap_outputs(env, _phase_set(call, quad), names=('reward', 'done', 'player', 'invalid_action', 'ending_invalid', 'next_actions'))
        sets = []
        for s in range(n_sets):
            ph = _phase_set(3 * call + s, quad)
            sets.append({k: Arena('%s[set %d]' % (k, s), getattr(env, k).shape, getattr(env, k).dtype, ph[k], env.device)
                         for k in ('obs', 'mask', 'fobs') if getattr(env, k) is not None})
        env._ring = [(a['obs'].t, a['mask'].t, a['fobs'].t if 'fobs' in a else None) for a in sets]
        env._ring_ios = (_lib.SgxStepIO * n_sets)()
        env._ring_pos = pos
        what = (name, n_envs, 'ring of', n_sets, 'call', call, 'nt', nt)
        _load_actions(env, acts)
        env.rollout_steps(n_steps, ring=True)
        _sync(env)
        lane = VARIANTS[name].cells <= 16 and env.fobs is None and not any((a['obs'].phase | a['mask'].phase) & 15 for a in sets) and \
            not (res['next_actions'].phase & 15 or res['reward'].phase & 7)
        assert env.last_launch_kind == (_lib.LAUNCH_MULTI_STEP if lane else _lib.LAUNCH_MULTI_STEP_WAVE), what + (env.last_launch_kind,)
        xs = _play(ora, acts, n_steps)
        last = {}
        for i, x in enumerate(xs):
            last[(pos + i) % n_sets] = x
        _guards(res, what)
        for s, a in enumerate(sets):
            _guards(a, what + ('set', s))
            if s in last:
                for t in a.values():
                    t.check_written(what + ('set', s))
                _compare(a, last[s], what + ('set', s))
            else:
                for t in a.values():
                    t.check_untouched(what + ('set', s))
        x = dict(xs[-1], final={})
        _written_after_step(res, x, what)
        _compare(res, x, what)
        acts = xs[-1]['next_actions'].copy()
        pos = (pos + n_steps) % n_sets
    env.close()


@pytest.mark.parametrize('name,n_envs', [('barrage', 9), ('barrage', 7), ('fives', 17), ('standard2', 3), ('medium', 7), ('octa_barrage', 9), ('micro', 33), ('tiny', 31),
                                         ('c3x40', 3), ('micro', 64)])
def test_step_traj(name, n_envs):
    """sgx_step_traj: per-slot results and the action log, first_slot != 0, wrapped around the end of the buffer; the slots a call does not
    reach keep the poison."""
    from stratego_env_amd import _lib
    both = name in ('barrage', 'fives') and n_envs != 7
    env, ora = _make(name, n_envs, auto_reset=True, full_obs=both)
    quad = _quad(name)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    T = 6
    for call, (first, n_steps) in enumerate(((0, 6), (2, 3), (4, 5), (5, 2))):
        nt = bool(call & 1)
        env.set_nt_stores(nt)
        ph = _phase_set(call + (3 if name == 'barrage' else 0), quad)
        shapes = {'obs': (env.obs.shape, env.obs.dtype), 'mask': (env.mask.shape, env.mask.dtype), 'reward': ((n_envs, 2), env.reward.dtype),
                  'done': ((n_envs,), env.done.dtype), 'player': ((n_envs,), env.player.dtype), 'invalid_action': ((n_envs,), env.invalid_action.dtype),
                  'ending_invalid': ((n_envs,), env.ending_invalid.dtype), 'actions': ((n_envs,), env.next_actions.dtype)}
        if both:
            shapes['fobs'] = (env.fobs.shape, env.fobs.dtype)
        ar = {k: Arena('traj[%s]' % k, (T,) + tuple(sh), dt, ph['next_actions' if k == 'actions' else k], env.device) for k, (sh, dt) in shapes.items()}
        na = _swap_outputs(env, {'next_actions': I32_PHASES[call % 4]}, names=('next_actions',))
        traj = {k: a.t for k, a in ar.items()}
        what = (name, n_envs, 'traj call', call, 'first', first, 'steps', n_steps, 'nt', nt)
        _load_actions(env, acts)
        env.rollout_trajectory(n_steps, traj, first_slot=first)
        _sync(env)
        # (the lane kernel also wants every SLOT as aligned as slot 0: slot strides that are multiples of 16 bytes, an even number of envs)
        lane = VARIANTS[name].cells <= 16 and not both and not ((ar['obs'].phase | ar['mask'].phase | na['next_actions'].phase) & 15 or ar['reward'].phase & 7) \
            and n_envs % 2 == 0 and (n_envs * VARIANTS[name].num_spatial_actions) % 16 == 0
        assert not (name == 'micro' and n_envs == 64 and call == 0) or lane
        assert env.last_launch_kind == (_lib.LAUNCH_MULTI_STEP if lane else _lib.LAUNCH_MULTI_STEP_WAVE), what + (env.last_launch_kind,)
        xs = _play(ora, acts, n_steps)
        _guards(ar, what)
        _guards(na, what)
        slots = {(first + i) % T: x for i, x in enumerate(xs)}
        h = {k: a.host() for k, a in ar.items()}
        for k, a in ar.items():
            u = a.unwritten().view(T, -1).cpu().numpy()
            for s in range(T):
                assert (not u[s].any()) if s in slots else u[s].all(), what + (k, 'slot', s, 'written' if s not in slots else 'holds poison')
        for s, x in slots.items():
            legal = x['legal']
            for k in ('mask', 'player', 'done', 'invalid_action'):
                assert np.array_equal(h[k][s], x[k]), what + (k, 'slot', s)
            assert np.array_equal(h['actions'][s], x['next_actions']), what + ('action log', 'slot', s)
            assert np.array_equal(h['reward'][s][legal], x['reward'][legal]) and np.array_equal(h['ending_invalid'][s][legal], x['ending_invalid'][legal]), what + (s,)
            assert h['obs'][s].tobytes() == x['obs'].tobytes(), what + ('obs', 'slot', s)
            assert not both or h['fobs'][s].tobytes() == x['fobs'].tobytes(), what + ('fobs', 'slot', s)
        assert np.array_equal(na['next_actions'].host(), xs[-1]['next_actions'])
        acts = xs[-1]['next_actions'].copy()
    env.close()


def test_lane_board_with_pointers_the_lane_kernels_refuse():
    """Micro with 16-byte aligned tensors runs the one-game-per-lane kernels; with a mask one byte off (or the reward 4 bytes off an 8-byte
    boundary) the SAME calls are played by the wave-per-game kernels -- not an error, and still the oracle's results."""
    import torch
    from stratego_env_amd import _lib
    env, ora = _make('micro', 65, auto_reset=True)
    env.set_lane_kernel(True)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    cases = (({}, _lib.LAUNCH_LANE, _lib.LAUNCH_MULTI_STEP), ({'mask': 1}, _lib.LAUNCH_WAVE, _lib.LAUNCH_MULTI_STEP_WAVE),
             ({'reward': 4}, _lib.LAUNCH_WAVE, _lib.LAUNCH_MULTI_STEP_WAVE), ({'next_actions': 4}, _lib.LAUNCH_LANE, _lib.LAUNCH_MULTI_STEP_WAVE),
             ({'obs': 16, 'mask': 1008}, _lib.LAUNCH_LANE, _lib.LAUNCH_MULTI_STEP))
    for phases, kind1, kindn in cases:
        ar = _swap_outputs(env, phases)
        what = ('micro', 'lane fallback', tuple(phases.items()))
        env.step(torch.from_numpy(acts), want_next_actions=True)       # (the actions of this call come from a torch tensor of its own: aligned)
        _sync(env)
        assert env.last_launch_kind == kind1, what + ('step', env.last_launch_kind)
        x = ora.step(acts)
        _guards(ar, what)
        _written_after_step(ar, x, what)
        _compare(ar, x, what)
        for a in ar.values():
            a.poison()
        _load_actions(env, x['next_actions'])
        env.rollout_steps(3)
        _sync(env)
        assert env.last_launch_kind == kindn, what + ('rollout', env.last_launch_kind)
        x = dict(_play(ora, x['next_actions'].copy(), 3)[-1], final={})
        _guards(ar, what)
        _written_after_step(ar, x, what)
        _compare(ar, x, what)
        acts = x['next_actions'].copy()
    env.close()


# ---- phases the contract refuses: SGX_EINVAL before any launch -----------------------------------------------------------------------
@pytest.mark.parametrize('name', ['barrage', 'medium', 'octa_barrage', 'tiny', 'micro'])
def test_quad_boards_refuse_observation_pointers_off_16_bytes(name):
    """Boards with a multiple of 4 cells store 16 bytes at a time through the observation pointers: phases 4, 8, 12 are SGX_EINVAL from every
    stepping entry point (as from sgx_decode_obs), the message names the pointer, and nothing is written anywhere."""
    import torch
    from stratego_env_amd import _lib
    env, ora = _make(name, 9, auto_reset=True, full_obs=True, final_obs=True)
    env.reset()
    env.sample_valid_actions()
    _sync(env)
    for which in ('obs', 'fobs', 'final_obs', 'final_fobs'):
        for phase in (4, 8, 12):
            ar = _swap_outputs(env, {which: phase, 'mask': 1})
            calls = [('sgx_step', lambda: env.step(env.next_actions, want_next_actions=True)), ('sgx_step_n', lambda: env.rollout_steps(3)),
                     ('sgx_rollout', lambda: env.rollout_steps(3, chains=2)), ('sgx_step_sync', lambda: env.step_sync(env.next_actions))]
            if which in ('obs', 'fobs'):
                calls.append(('sgx_observe', env.observe))
            for fn, call in calls:
                with pytest.raises(_lib.SgxError, match=r'%s: %s_dev must be 16-byte aligned' % (fn, which)):
                    call()
            _sync(env)
            for a in ar.values():
                a.check_guards((name, which, phase))
                a.check_untouched((name, which, phase))
    # ring and trajectory: a misaligned set / slot 0
    ar = _swap_outputs(env, {})
    good = (ar['obs'].t, ar['mask'].t, ar['fobs'].t)
    bad = Arena('obs[set 1]', env.obs.shape, env.obs.dtype, 8, env.device)
    env._ring, env._ring_ios, env._ring_pos = [good, (bad.t, ar['mask'].t, ar['fobs'].t), good], (_lib.SgxStepIO * 3)(), 0
    with pytest.raises(_lib.SgxError, match='sgx_step_ring: obs_dev must be 16-byte aligned'):
        env.rollout_steps(4, ring=True)
    env.obs, env.mask, env.fobs = good
    tr = {k: Arena('traj[%s]' % k, (4,) + tuple(getattr(env, k).shape), getattr(env, k).dtype, 12 if k == 'fobs' else 0, env.device) for k in ('obs', 'mask', 'fobs')}
    with pytest.raises(_lib.SgxError, match='sgx_step_traj: fobs_dev must be 16-byte aligned'):
        env.rollout_trajectory(3, {k: a.t for k, a in tr.items()})
    _sync(env)
    for a in list(ar.values()) + [bad] + list(tr.values()):
        a.check_guards(name)
        a.check_untouched(name)
    # sgx_decode_obs agrees
    cenv, _ = _make(name, 9, compact_outputs=True)
    cenv.reset()
    dec = Arena('decoded obs', (9, cenv.R, cenv.Cc, 67), torch.float32, 4, cenv.device)
    with pytest.raises(_lib.SgxError, match='sgx_decode_obs: obs_dev must be 16-byte aligned'):
        cenv.decode_obs(out=dec.t)
    _sync(cenv)
    dec.check_guards(name)
    dec.check_untouched(name)
    cenv.close()
    env.close()


# ---- the other entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n_envs', [('barrage', 9), ('fives', 17), ('standard2', 3), ('micro', 33), ('c3x40', 3)])
def test_samplers_info_and_export(name, n_envs):
    """sgx_sample_valid and sgx_choose_actions (mask READ at every uint8 phase, actions written at every int32 phase), sgx_get_env_info
    (16-byte aligned: an int4 per game; 4, 8, 12 are SGX_EINVAL), sgx_export_state (16-byte loads / stores: phase 8 is SGX_EINVAL)."""
    import torch
    from stratego_env_amd import _lib
    env, ora = _make(name, n_envs, auto_reset=True)
    quad = _quad(name)
    env.reset()
    env.sample_valid_actions()
    acts = env.next_actions.cpu().numpy().copy()
    for t in range(len(U8_PHASES)):
        ar = _swap_outputs(env, dict(_phase_set(t, quad), mask=U8_PHASES[t]))
        env.step(torch.from_numpy(acts), want_next_actions=True)
        x = ora.step(acts)
        acts = x['next_actions'].copy()
        out = Arena('sampled', (n_envs,), torch.int32, I32_PHASES[t % 4], env.device)
        env.sample_valid_actions(mask=ar['mask'].t, out=out.t)
        cho = Arena('chosen', (n_envs,), torch.int32, I32_PHASES[(t + 2) % 4], env.device)
        lg = Arena('logits', (n_envs, env.R * env.Cc * env.K), torch.float32, F32_ODD_PHASES[t % 6], env.device)
        lg.t.zero_()
        env.choose_actions(lg.t, mask=ar['mask'].t, out=cho.t)
        _sync(env)
        what = (name, 'samplers', t)
        for a in (out, cho, lg):
            a.check_guards(what)
        _guards(ar, what)
        out.check_written(what)
        cho.check_written(what)
        assert np.array_equal(out.host(), x['next_actions']) and np.array_equal(cho.host(), x['next_actions']), what     # (equal logits: the sampler's draw)
    # env info
    info = Arena('info', (n_envs, 4), torch.int32, 112, env.device)
    _lib.check(env._L.sgx_get_env_info(env._h, C.c_void_p(info.t.data_ptr()), env._stream()), env._L)
    _sync(env)
    info.check_guards('info')
    info.check_written('info')
    st, pl = ora.states()
    want = np.stack([st[:, 5, 0, 0], [oe.game_no for oe in ora.envs], st[:, 5, 0, 1], pl.astype(np.int64)], axis=1)
    assert np.array_equal(info.host(), want.astype(np.int32))
    for phase in (4, 8, 12):
        bad = Arena('info', (n_envs, 4), torch.int32, phase, env.device)
        assert env._L.sgx_get_env_info(env._h, C.c_void_p(bad.t.data_ptr()), env._stream()) == -1
        assert b'info_dev must be 16-byte aligned' in env._L.sgx_last_error()
        _sync(env)
        bad.check_guards('info')
        bad.check_untouched('info')
    # export: both store policies, the player bytes at odd phases
    for nt, pphase, sphase in ((False, 1, 16), (True, 3, 1008), (False, 1023, 112)):
        env.set_nt_stores(nt)
        sa = Arena('state', (n_envs, 34, env.R, env.Cc), torch.int64, sphase, env.device)
        pa = Arena('state player', (n_envs,), torch.int8, pphase, env.device)
        _lib.check(env._L.sgx_export_state(env._h, C.c_void_p(sa.t.data_ptr()), C.c_void_p(pa.t.data_ptr()), env._stream()), env._L)
        _sync(env)
        for a in (sa, pa):
            a.check_guards('export')
            a.check_written('export')
        assert np.array_equal(sa.host(), st) and np.array_equal(pa.host(), pl)
    bad = Arena('state', (n_envs, 34, env.R, env.Cc), torch.int64, 8, env.device)
    assert env._L.sgx_export_state(env._h, C.c_void_p(bad.t.data_ptr()), None, env._stream()) == -1
    assert b'state_dev must be 16-byte aligned' in env._L.sgx_last_error()
    _sync(env)
    bad.check_guards('export')
    bad.check_untouched('export')
    env.close()


@pytest.mark.parametrize('name,n_envs', [('barrage', 9), ('fives', 17), ('micro', 33)])
def test_reset_of_a_subset_writes_no_output(name, n_envs):
    """sgx_reset with an env_select subset (the select bytes at an odd address) touches no output tensor; the observe that follows shows new
    games for the selected envs and the old positions for the others."""
    import torch
    from stratego_env_amd import _lib
    env, ora = _make(name, n_envs, auto_reset=False)
    env.reset()
    acts = env.sample_valid_actions().cpu().numpy().copy()
    env.step(torch.from_numpy(acts))
    ora.step(acts)
    ar = _swap_outputs(env, _phase_set(1, _quad(name)))
    sel = Arena('select', (n_envs,), torch.uint8, 3, env.device)
    chosen = [e for e in range(n_envs) if e % 3 == 1]
    sel.t.zero_()
    sel.t[torch.as_tensor(chosen, device=env.device)] = 1
    _lib.check(env._L.sgx_reset(env._h, C.c_void_p(sel.t.data_ptr()), None, None, env._stream()), env._L)
    _sync(env)
    _guards(ar, 'reset subset')
    sel.check_guards('reset subset')
    for a in ar.values():
        a.check_untouched('reset subset')
    for e in chosen:
        oe = ora.envs[e]
        oe.game_no += 1
        ora.cur[e] = oe.reset(initial_state_override=orc.reset_state(ora.cv, ora.seed, ora.g0 + e, oe.game_no))[1]
    env.observe()
    _sync(env)
    _guards(ar, 'observe after reset subset')
    cur = ora.current()
    _compare({k: ar[k] for k in ('obs', 'mask', 'player')}, {k: cur[k] for k in ('obs', 'mask', 'player')}, (name, 'observe after reset subset'))
    env.close()


# ---- the functional API on int64 states ----------------------------------------------------------------------------------------------
def _absolute_1d(ru, acts, players, cols, K):
    """flat perspective actions of the movers -> 1-D indices in absolute coordinates (what SGX_STEP_ACTIONS_1D takes)"""
    out = []
    for a, p in zip(acts, players):
        a = int(a)
        i1 = ru.get_action_1d_index_from_spatial_index((a // (cols * K), (a // K) % cols, a % K))
        out.append(ru.get_action_1d_index_from_player_perspective(i1, int(p)))
    return np.asarray(out, dtype=np.int32)


@pytest.mark.parametrize('name,n_envs', [('barrage', 9), ('fives', 17), ('medium', 7), ('micro', 33)])
def test_step_states_and_state_coordinate_masks(name, n_envs):
    """sgx_step_states: state_out / player_out / sanitised in arenas; the masks of SGX_STEP_MASK_1D and SGX_STEP_MASK_STATE_COORDS
    (emit_mask_mapped) at every uint8 phase.  Next states, players, masks and observations against the oracle's pure functions."""
    import torch
    from stratego_env_amd import _lib
    env, ora = _make(name, n_envs, auto_reset=True)
    v, quad = VARIANTS[name], _quad(name)
    R, Cc = v.rows, v.columns
    ru = orc.OracleRules(R, Cc)
    env.reset()
    acts = env.sample_valid_actions().cpu().numpy().copy()
    for t in range(5):                                   # a few plies in, so that both players move
        env.step(torch.from_numpy(acts), want_next_actions=True)
        acts = ora.step(acts)['next_actions'].copy()
    st, pl = ora.states()
    a1d = _absolute_1d(ru, acts, pl, Cc, env.K)
    nxt = [ru.get_next_state(st[e], int(pl[e]), int(a1d[e])) for e in range(n_envs)]
    probe = orc.OracleEnv(R, Cc, v.max_turns, v.obstacle_locations, v.piece_counts)
    st_in = Arena('state_in', st.shape, torch.int64, 16, env.device)
    st_in.t.copy_(torch.from_numpy(st))
    pl_in = Arena('player_in', (n_envs,), torch.int8, 5, env.device)
    pl_in.t.copy_(torch.from_numpy(pl))
    a_in = Arena('actions', (n_envs,), torch.int32, 4, env.device)
    a_in.t.copy_(torch.from_numpy(a1d))
    for t, flag in enumerate([_lib.STEP_MASK_1D, _lib.STEP_MASK_STATE_COORDS] * 6):
        one_d = flag == _lib.STEP_MASK_1D
        ph = _phase_set(t, quad)
        mshape = (n_envs, R * Cc * (R + Cc) + 1) if one_d else (n_envs, R, Cc, env.K)
        ar = {'mask': Arena('mask', mshape, torch.uint8, U8_PHASES[t % 11], env.device), 'obs': Arena('obs', env.obs.shape, torch.float32, ph['obs'], env.device),
              'state_out': Arena('state_out', st.shape, torch.int64, (112, 1008, 16)[t % 3], env.device),
              'player_out': Arena('player_out', (n_envs,), torch.int8, ph['player'], env.device),
              'sanitised': Arena('sanitised', (n_envs,), torch.uint8, ph['done'], env.device)}
        res = _swap_outputs(env, ph, names=('reward', 'done', 'player', 'invalid_action', 'ending_invalid'))
        env.obs, env.mask = ar['obs'].t, ar['mask'].t
        io = env._fill_io(a_in.t, False, True, True, flag | _lib.STEP_ACTIONS_1D)
        io.auto_reset = 0
        what = (name, 'step_states', '1-D mask' if one_d else 'state-coordinate mask', t)
        with torch.cuda.device(env.device):
            _lib.check(env._L.sgx_step_states(env._h, C.c_void_p(st_in.t.data_ptr()), C.c_void_p(pl_in.t.data_ptr()), C.c_void_p(ar['sanitised'].t.data_ptr()),
                                              C.byref(io), C.c_void_p(ar['state_out'].t.data_ptr()), C.c_void_p(ar['player_out'].t.data_ptr()), 1 + t % 2, env._stream()), env._L)
        _sync(env)
        _guards(ar, what)
        _guards(res, what)
        for a in (st_in, pl_in, a_in):
            a.check_guards(what)
        for a in list(ar.values()) + list(res.values()):
            a.check_written(what)
        assert not ar['sanitised'].host().any() and not res['invalid_action'].host().any(), what
        so, po, mh, oh = ar['state_out'].host(), ar['player_out'].host(), ar['mask'].host(), ar['obs'].host()
        for e in range(n_envs):
            ns, np_ = nxt[e]
            assert np.array_equal(so[e], ns) and po[e] == np_, what + (e, 'next state')
            m = ru.get_valid_moves_as_1d_mask(ns, np_) if one_d else ru.get_valid_moves_as_spatial_mask(ns, np_)
            assert np.array_equal(mh[e].reshape(-1), np.asarray(m).reshape(-1).astype(np.uint8)), what + (e, 'mask')
            probe.reset(initial_state_override=ns, first_player_override=np_)
            assert oh[e].tobytes() == probe._obs(np_)[POBS].tobytes(), what + (e, 'observation of the next mover')
    env.close()


def test_step_states_rejects_a_shifted_overlap():
    """Without the general-state pass a batch may be stepped in place (state_out == state_in, player_out == player_in): equal to the oracle.
    Outputs shifted against the inputs by one state would race between workgroups: SGX_EINVAL, nothing launched -- with the pass on or off."""
    import torch
    from stratego_env_amd import _lib
    n = 9
    env, ora = _make('barrage', n, auto_reset=False)
    ru = orc.OracleRules(env.R, env.Cc)
    env.reset()
    acts = env.sample_valid_actions().cpu().numpy().copy()
    st, pl = ora.states()
    a1d = _absolute_1d(ru, acts, pl, env.Cc, env.K)
    a_in = torch.from_numpy(a1d).to(env.device)
    big = Arena('states', (n + 1,) + st.shape[1:], torch.int64, 16, env.device)
    pls = Arena('players', (n + 1,), torch.int8, 1, env.device)
    res = _swap_outputs(env, {}, names=('reward', 'done', 'player', 'invalid_action', 'ending_invalid'))

    def call(s_in, p_in, s_out, p_out):
        io = env._fill_io(a_in, False, False, False, _lib.STEP_ACTIONS_1D)
        io.auto_reset = 0
        with torch.cuda.device(env.device):
            return env._L.sgx_step_states(env._h, C.c_void_p(s_in.data_ptr()), C.c_void_p(p_in.data_ptr()), None, C.byref(io), C.c_void_p(s_out.data_ptr()),
                                          C.c_void_p(p_out.data_ptr()), 1, env._stream())
    for general in (1, 0):
        _lib.check(env._L.sgx_set_general_states(env._h, general), env._L)
        big.poison(); pls.poison()
        big.t[:n].copy_(torch.from_numpy(st)); pls.t[:n].copy_(torch.from_numpy(pl))
        before = big.buf.clone()
        assert call(big.t[:n], pls.t[:n], big.t[1:], pls.t[:n]) == -1 and b'overlap' in env._L.sgx_last_error()
        assert call(big.t[:n], pls.t[:n], big.t[:n], pls.t[1:]) == -1 and b'overlap' in env._L.sgx_last_error()
        _sync(env)
        assert torch.equal(big.buf, before), 'a refused call wrote states'
        for a in res.values():
            a.check_untouched('refused overlap')
    # in place, pass off: the oracle's next states
    assert call(big.t[:n], pls.t[:n], big.t[:n], pls.t[:n]) == 0, env._L.sgx_last_error()
    _sync(env)
    big.check_guards('in place'); pls.check_guards('in place')
    so, po = big.host(), pls.host()
    for e in range(n):
        ns, _ = ru.get_next_state(st[e], int(pl[e]), int(a1d[e]))
        assert np.array_equal(so[e], ns) and po[e] == -pl[e], ('in place', e)
    assert bool(big.unwritten()[n].all()) and bool(pls.unwritten()[n].all()), 'the state behind the batch was written'
    env.close()


# ---- rollout_trajectory validates every tensor of the dict -----------------------------------------------------------------------------
def test_rollout_trajectory_validates_every_tensor():
    """A caller-built trajectory dict reaches sgx_step_traj as raw pointers: a short `reward`, a wrong-dtype `done`, a non-contiguous
    `player`, an `actions` on the CPU each raise ValueError naming the key, launch nothing and leave the env's own tensors in place."""
    import torch
    env, ora = _make('barrage', 9, auto_reset=True)
    env.reset()
    env.sample_valid_actions()
    T, N = 4, 9
    good = env.alloc_trajectory(T)
    for t in good.values():
        t.fill_(0x5A if t.dtype in (torch.uint8, torch.int8) else 7)
    snap = {k: t.clone() for k, t in good.items()}
    bad = {'reward': torch.zeros((T - 1, N, 2), dtype=torch.float32, device=env.device),
           'done': torch.zeros((T, N), dtype=torch.int32, device=env.device),
           'player': torch.zeros((T, 2 * N), dtype=torch.int8, device=env.device)[:, ::2],
           'actions': torch.zeros((T, N), dtype=torch.int32),
           'invalid_action': torch.zeros((T, N + 1), dtype=torch.uint8, device=env.device),
           'mask': torch.zeros((T,) + tuple(env.mask.shape), dtype=torch.uint8)}
    keep = {k: getattr(env, k) for k in ('obs', 'mask', 'reward', 'done', 'player', 'invalid_action', 'ending_invalid')}
    nxt = env.next_actions.clone()
    for k, t in bad.items():
        with pytest.raises(ValueError, match=r"traj\['%s'\]" % k):
            env.rollout_trajectory(3, dict(good, **{k: t}))
        _sync(env)
        for a, was in keep.items():
            assert getattr(env, a) is was, (k, a)
        assert torch.equal(env.next_actions, nxt)
        for g, t0 in snap.items():
            assert torch.equal(good[g].view(torch.uint8), t0.view(torch.uint8)), (k, g, 'a refused call wrote the trajectory')
    with pytest.raises(ValueError, match='first_slot'):
        env.rollout_trajectory(3, good, first_slot=T)
    # the dict as allocated still works and equals the oracle
    acts = env.next_actions.cpu().numpy().copy()
    env.rollout_trajectory(3, good)
    xs = _play(ora, acts, 3)
    for s, x in enumerate(xs):
        assert np.array_equal(good['mask'][s].cpu().numpy(), x['mask']) and good['obs'][s].cpu().numpy().tobytes() == x['obs'].tobytes()
        assert np.array_equal(good['actions'][s].cpu().numpy(), x['next_actions'])
    env.close()
