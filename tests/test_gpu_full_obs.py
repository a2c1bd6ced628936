"""Fully-observable observation (79 channels) and BOTH_OBSERVATIONS mode on the GPU: vs the oracle and vs vectors
recorded from the reference (tests/golden/games_both_*.npz)."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import GameVersions, ObservationModes
from stratego_env_amd.config import VARIANTS
from tests.boards import _state_from_maps
from tests.helpers import GOLDEN, _load_npz
from tests.step_checks import check_both_obs_vs_oracle, digest_both

pytestmark = pytest.mark.gpu
MASK, POBS, FOBS = 'valid_actions_mask', 'partial_observation', 'full_observation'


@pytest.mark.parametrize('name,n_envs,n_steps', [('barrage', 32, 500), ('standard', 6, 300), ('tiny', 48, 150), ('micro', 48, 80),
                                                 ('fives', 32, 150), ('octa_barrage', 16, 200), ('standard2', 2, 80)])
def test_full_obs_bit_exact_vs_oracle(name, n_envs, n_steps):
    check_both_obs_vs_oracle(name, n_envs, n_steps, 'extended')


@pytest.mark.parametrize('name', ['barrage', 'tiny', 'micro', 'fives'])
def test_facade_both_mode_replays_reference_goldens(name):
    """Default reference config (observation_mode = BOTH_OBSERVATIONS): keys and bytes of both observations."""
    from stratego_env_amd.multiagent_env import StrategoMultiAgentEnv, DEFAULT_CONFIG
    assert DEFAULT_CONFIG['observation_mode'] == ObservationModes.BOTH_OBSERVATIONS
    g = _load_npz(os.path.join(GOLDEN, 'games_both_%s.npz' % name))
    env = StrategoMultiAgentEnv({'version': GameVersions(name)})        # no observation_mode: the default, BOTH
    off = g['offsets']
    for gi in range(min(5, len(off) - 1)):
        obs = env.reset(initial_state_override=_state_from_maps(name, g['p1_maps'][gi], g['p2_maps'][gi]))
        assert sorted(obs[1].keys()) == [FOBS, POBS, MASK]
        assert obs[1][FOBS].shape == (env.rows, env.columns, 79) and obs[1][FOBS].dtype == np.float32
        assert digest_both(obs) == int(g['init_digests'][gi])
        for k in range(off[gi], off[gi + 1]):
            obs, rew, done, info = env.step({env.player: int(g['actions'][k])})
            assert digest_both(obs) == int(g['digests'][k]), (name, gi, k)
            assert done['__all__'] == bool(g['dones'][k])
    env.close()
    env = StrategoMultiAgentEnv({'version': GameVersions(name), 'observation_mode': ObservationModes.FULLY_OBSERVABLE})
    obs = env.reset()
    assert sorted(obs[1].keys()) == [FOBS, MASK] and sorted(env.observation_space.spaces.keys()) == [FOBS, MASK]
    env.close()
