"""The multi-step kernels (steps_kernel, lane_steps_kernel: what bench.py times) pinned to the ORACLE at EVERY step, directly.

A rollout into a trajectory buffer (sgx_step_traj: slot t of [T][N]... tensors receives step t's outputs, any number of slots; all steps of
a call in one launch per 256 steps) keeps what every step wrote -- mask bytes, observation bytes (both kinds), rewards, done, player,
invalid-ending flag and the action the step drew -- so every step of a multi-step launch is compared with the oracle stepped alongside
(reference: a fresh observation array per env.step(), impl:905, maenv:447-497, 659-828).  The buffers are poisoned before every call: a step
whose stores were skipped leaves the poison behind and fails the comparison.  Also here: the same through sgx_step_ring with one separate
set per step, the literal BASELINE config-2 check (256 held-out seeds to termination) through the multi-step kernel, and the calls the
multi-step kernels do not cover (one launch per step behind the same entry point)."""
import numpy as np
import pytest

from stratego_env_amd.config import VARIANTS
from tests.step_checks import Follower, _host, _multi_kinds, _poison, check_every_step_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name,n_envs,chunk,n_calls,garbage', [
    ('barrage', 48, 64, 10, 0.2), ('standard', 16, 48, 8, 0.1), ('short_barrage', 64, 40, 8, 0.2), ('octa_barrage', 32, 64, 5, 0.2),
    ('medium', 40, 50, 6, 0.2), ('fives', 33, 30, 6, 0.2), ('standard2', 5, 24, 4, 0.1), ('tiny', 100, 64, 4, 0.2), ('micro', 130, 20, 8, 0.2),
])
def test_every_step_of_a_multi_step_launch_equals_the_oracle(name, n_envs, chunk, n_calls, garbage):
    check_every_step_vs_oracle(name, n_envs, chunk, n_calls, garbage)


@pytest.mark.parametrize('name,n_envs,chunk,n_calls', [('barrage', 24, 48, 6), ('octa_barrage', 16, 40, 4), ('fives', 20, 30, 4)])
def test_every_step_with_both_observations(name, n_envs, chunk, n_calls):
    """BOTH_OBSERVATIONS (the reference's default mode, maenv:53): steps_kernel<..., 1> writes the 79-channel observation as well."""
    check_every_step_vs_oracle(name, n_envs, chunk, n_calls, 0.1, both=True)


@pytest.mark.parametrize('name,n_envs,chunk,n_calls', [('barrage', 45, 64, 8), ('standard', 19, 40, 6), ('octa_barrage', 33, 50, 4), ('medium', 47, 40, 5), ('tiny', 70, 30, 3)])
def test_every_step_of_a_rollout_without_observation(name, n_envs, chunk, n_calls):
    """Mask-only rollouts (no observation pointer): steps_kernel<..., 8> -- on boards of 33 .. 128 cells the TWO-games-per-wave layout
    (Geo<R, C, 2>), ragged batches so that a wave holds one game -- every step's mask, rewards, flags, player and drawn action against the
    oracle; the observation slots stay untouched."""
    check_every_step_vs_oracle(name, n_envs, chunk, n_calls, 0.2, emit_obs=False)


@pytest.mark.parametrize('name,n_envs,chunk,n_calls', [('short_barrage', 48, 64, 4), ('micro', 96, 25, 3)])
def test_every_step_without_auto_reset(name, n_envs, chunk, n_calls):
    """Without auto-reset a finished game stays finished: every later step of the launch draws the no-op of its one-entry mask, which is
    not playable -- flagged invalid, nothing changes."""
    check_every_step_vs_oracle(name, n_envs, chunk, n_calls, 0.0, auto_reset=False)


@pytest.mark.parametrize('name,n_envs,n_steps', [('barrage', 12, 300), ('micro', 70, 530)])
def test_every_step_across_the_256_step_chunks(name, n_envs, n_steps):
    """ONE call longer than a launch may be (256 steps): 256 + 44 steps on Barrage, 256 + 256 + 18 on Micro (lane_steps_kernel goes out in
    chunks as well since this round) -- the boundary is invisible in the slots."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    seed, g0 = 0xC0FFEE + n_steps, 31
    env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)
    fo = Follower(name, seed, g0, n_envs, True)
    env.reset()
    env.sample_valid_actions()
    traj = env.alloc_trajectory(n_steps)
    _poison(traj)
    acts = env.next_actions.cpu().numpy().copy()
    env.rollout_trajectory(n_steps, traj)
    assert env.last_launch_kind in _multi_kinds()
    h = _host(traj)
    for s in range(n_steps):
        fo.check_slot(acts, h, s, 'one call')
        acts = h['actions'][s]
    assert fo.games_done > 0
    env.close()


@pytest.mark.parametrize('name,n_envs', [('barrage', 20), ('tiny', 80)])
def test_slots_wrap_around_from_a_first_slot(name, n_envs):
    """n_steps > n_slots from first_slot != 0: slot (first_slot + t) % T holds step t, the last T steps survive."""
    from stratego_env_amd.vec_env import VecStrategoEnv
    T, n_steps, first = 5, 13, 3
    seed, g0 = 0xBEE5, 900
    env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)
    fo = Follower(name, seed, g0, n_envs, True)
    env.reset()
    env.sample_valid_actions()
    # the oracle needs the outputs of every step to follow the games: a second, twin env writes all 13 steps into 13 slots
    twin = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)
    twin.reset(); twin.sample_valid_actions()
    full = twin.alloc_trajectory(n_steps)
    acts = twin.next_actions.cpu().numpy().copy()
    twin.rollout_trajectory(n_steps, full)
    hf = _host(full)
    for s in range(n_steps):
        fo.check_slot(acts, hf, s, 'twin')
        acts = hf['actions'][s]
    traj = env.alloc_trajectory(T)
    _poison(traj)
    env.rollout_trajectory(n_steps, traj, first_slot=first)
    assert env.last_launch_kind in _multi_kinds()
    h = _host(traj)
    for t in range(n_steps - T, n_steps):
        s = (first + t) % T
        for k in h:
            assert np.array_equal(h[k][s], hf[k][t], equal_nan=(h[k].dtype == np.float32)), (name, k, 'step', t, 'slot', s)
    assert env.obs.data_ptr() == traj['obs'][(first + n_steps - 1) % T].data_ptr()
    env.close(); twin.close()


@pytest.mark.parametrize('S', [8, 21])
def test_ring_of_separate_sets_every_set_equals_the_oracle(S):
    """sgx_step_ring with one separately allocated output set per step (n_sets = n_steps = S: 8 = the most whose pointers fit the kernel
    arguments, 21 = pointers in a device table): every SET's mask and observation against the oracle; the shared results are the last step's."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    for name, n_envs in (('barrage', 40), ('micro', 128)):
        seed, g0 = 0x51DE, 40
        env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)
        fo = Follower(name, seed, g0, n_envs, True)
        env.reset()
        env.sample_valid_actions()
        env.alloc_output_ring(S)
        log = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)    # per-step results / draws of the same games
        log.reset(); log.sample_valid_actions()
        for call in range(6 if S == 8 else 3):
            acts = env.next_actions.cpu().numpy().copy()
            first = env._ring_pos
            for o, m, _ in env._ring:
                o.fill_(float('nan')); m.fill_(0x5A)
            env.rollout_steps(S, ring=True)
            assert env.last_launch_kind in _multi_kinds()
            res = log.alloc_trajectory(S)
            log.rollout_trajectory(S, res)
            hr = _host(res)
            h = dict(hr)
            order = [(first + t) % S for t in range(S)]
            h['obs'] = np.stack([env._ring[s][0].cpu().numpy() for s in order])
            h['mask'] = np.stack([env._ring[s][1].cpu().numpy() for s in order])
            for t in range(S):
                fo.check_slot(acts, h, t, 'ring call %d' % call)
                acts = h['actions'][t]
            for k, t in (('reward', env.reward), ('done', env.done), ('player', env.player), ('ending_invalid', env.ending_invalid)):
                assert np.array_equal(t.cpu().numpy(), hr[k][S - 1]), (name, k)
            assert torch.equal(env.next_actions, res['actions'][S - 1])
        env.close(); log.close()


def test_repeated_ring_entries_over_three_buffers_keep_the_last_three_steps():
    """repeat_output_ring(): 21 ring entries over the three buffers of a ring of 3 (pointers in the device table) -- after a call of n steps the
    three buffers hold the last three steps' outputs, bit for bit what a trajectory of the same games holds in those slots."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    for name, n_envs in (('barrage', 48), ('tiny', 128)):
        seed, g0, E = 0x7AB1E, 16, 21        # (a multiple of 3: consecutive steps never share a buffer across the wrap)
        env = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)
        log = VecStrategoEnv(name, n_envs, seed=seed, env_id_offset=g0, auto_reset=True)
        for e in (env, log):
            e.reset(); e.sample_valid_actions()
        env.alloc_output_ring(3)
        bufs = [o.data_ptr() for o, _, _ in env._ring]
        env.repeat_output_ring(E)
        assert [o.data_ptr() for o, _, _ in env._ring] == [bufs[i % 3] for i in range(E)]
        with pytest.raises(ValueError):
            env.repeat_output_ring(2)
        for n_steps in (E, 7, 33):
            first = env._ring_pos
            env.rollout_steps(n_steps, ring=True)
            assert env.last_launch_kind in _multi_kinds()
            res = log.alloc_trajectory(n_steps)
            log.rollout_trajectory(n_steps, res)
            for back in range(3):
                t = n_steps - 1 - back
                o, m, _ = env._ring[(first + t) % E]
                assert torch.equal(m, res['mask'][t]), (name, n_steps, back)
                assert torch.equal(o.view(torch.int32), res['obs'][t].view(torch.int32)), (name, n_steps, back)
            assert torch.equal(env.next_actions, res['actions'][n_steps - 1])
            assert torch.equal(env.reward, res['reward'][n_steps - 1]) and torch.equal(env.done, res['done'][n_steps - 1])
        env.close(); log.close()


def test_config2_256_heldout_seeds_to_termination_through_the_multi_step_kernel():
    """BASELINE config 2's bit-exact check on the kernel bench.py times: 256 held-out seeds BASE_SEED + 1 .. + 256, env id 0,
    each played by multi-step launches of 64 steps into a 64-slot trajectory buffer until its first game ends -- every step's drawn action,
    mask, observation, reward, done, player and invalid-ending flag against the oracle, and the final state."""
    import torch
    from bench import BASE_SEED
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, n, chunk = 'barrage', 256, 64
    v = VARIANTS[name]
    total_steps = 0
    for i in range(n):
        seed = BASE_SEED + 1 + i
        env = VecStrategoEnv(name, 1, seed=seed, env_id_offset=0, auto_reset=False)
        fo = Follower(name, seed, 0, 1, False)
        env.reset()
        fo.check_reset(env.obs.cpu().numpy(), env.mask.cpu().numpy())
        env.sample_valid_actions()
        traj = env.alloc_trajectory(chunk)
        while not fo.finished[0]:
            acts = env.next_actions.cpu().numpy().copy()
            assert acts[0] == fo.drawn(0)
            _poison(traj)
            env.rollout_trajectory(chunk, traj)
            assert env.last_launch_kind in _multi_kinds()
            h = _host(traj)
            for s in range(chunk):
                fo.check_slot(acts, h, s, 'seed %d' % i)
                acts = h['actions'][s]
            assert fo.steps <= v.max_turns + chunk
        st, _ = env.export_state()
        assert np.array_equal(st.cpu().numpy()[0], fo.oenvs[0].state), (i, 'final state')
        total_steps += fo.steps
        env.close()
    assert total_steps > 256 * 20


@pytest.mark.parametrize('kw,what', [({'obs_channel_mode': 'original'}, "'original' channels"), ({'final_obs': True}, 'terminal observations')])
def test_trajectory_calls_the_multi_step_kernels_do_not_cover(kw, what):
    """Behind the same entry point: one launch per step with the slot's pointers -- every slot equals the same steps played one by one."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    a = VecStrategoEnv('short_barrage', 300, seed=77, auto_reset=True, **kw)
    b = VecStrategoEnv('short_barrage', 300, seed=77, auto_reset=True, **kw)
    a.reset(); b.reset(); a.sample_valid_actions(); b.sample_valid_actions()
    T = 40
    traj = a.alloc_trajectory(T)
    _poison(traj)
    a.rollout_trajectory(T, traj)
    if 'obs_channel_mode' in kw:
        assert a.last_launch_kind == _lib.LAUNCH_WAVE, what
    for s in range(T):
        b.rollout_step()
        for k, t in (('obs', b.obs), ('mask', b.mask), ('reward', b.reward), ('done', b.done), ('player', b.player), ('invalid_action', b.invalid_action),
                     ('ending_invalid', b.ending_invalid), ('actions', b.next_actions)):
            assert torch.equal(traj[k][s], t), (what, k, s)
    if a.final_obs is not None:
        assert torch.equal(a.final_obs, b.final_obs) and bool(a.final_obs.abs().sum() > 0)
    a.close(); b.close()


def test_trajectory_of_compact_outputs():
    """compact_outputs=True: the slots hold the 4-bit codes / mask bits; decoded, every slot is the contract tensor of that step."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    a = VecStrategoEnv('barrage', 500, seed=5, auto_reset=True, compact_outputs=True)
    b = VecStrategoEnv('barrage', 500, seed=5, auto_reset=True)
    a.reset(); b.reset(); a.sample_valid_actions(); b.sample_valid_actions()
    T = 33
    traj = a.alloc_trajectory(T)
    a.rollout_trajectory(T, traj)
    assert a.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE
    for s in range(T):
        b.rollout_step()
        a.obs, a.mask = traj['obs'][s], traj['mask'][s]
        assert torch.equal(a.decode_obs(), b.obs) and torch.equal(a.decode_mask(), b.mask), s
        assert torch.equal(traj['reward'][s], b.reward) and torch.equal(traj['done'][s], b.done) and torch.equal(traj['actions'][s], b.next_actions)
    a.close(); b.close()


def test_trajectory_argument_checks():
    import ctypes as C
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv('barrage', 64, seed=1, auto_reset=True)
    env.reset(); env.sample_valid_actions()
    traj = env.alloc_trajectory(4)
    with pytest.raises(ValueError):
        env.rollout_trajectory(3, traj, first_slot=4)
    before = (env.obs.data_ptr(), env.reward.data_ptr())
    env.rollout_trajectory(0, traj)
    assert (env.obs.data_ptr(), env.reward.data_ptr()) == before
    t = _lib.SgxTrajIO()
    io = env._fill_io(env.next_actions, True, True, True, 0)
    C.memmove(C.byref(t.io), C.byref(io), C.sizeof(_lib.SgxStepIO))
    t.n_slots, t.slot_envs = 4, 63                                   # fewer envs per slot than the handle has
    assert env._L.sgx_step_traj(env._h, C.byref(t), 0, 2, None) == -1
    t.slot_envs, t.n_slots = 64, 0
    assert env._L.sgx_step_traj(env._h, C.byref(t), 0, 2, None) == -1
    env.close()
