"""More than 8 pieces of one type per side.  The reference's piece_amounts is an unbounded dict (config.py:3-23); the packed record's
capture event counts to 8, so a variant with more pieces of a type chains events of one (layer, cell) key and every reader sums them
(KParams::multi_ev).  Step parity on such a variant, and directed positions where a count crosses 8, 16 and 24."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.boards import MANY_PIECES as CUSTOM, registered
from tests.step_checks import check_step_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _custom_names():
    yield from registered(CUSTOM)


@pytest.mark.parametrize('name,n_envs,n_steps', [('many66', 48, 300), ('many88', 32, 300)])
def test_step_parity_with_more_than_eight_pieces_of_a_type(name, n_envs, n_steps):
    check_step_vs_oracle(name, n_envs, n_steps, 0.1, seed_salt=5)


@pytest.mark.parametrize('channel_mode', ['extended', 'original'])
def test_counts_beyond_eight_chain_events(channel_mode):
    """A p1 scout dies on a p2 bomb on a cell that already holds c captured p1 scouts (c = 7 .. 24: the count crosses the 8 of one
    event, the 16 entries of the normalisation table, and a third event): imported state, observation, step and exported successor
    equal the oracle's; a raw round trip keeps every count."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    v = CUSTOM['many66']
    R = C = 6
    counts = (7, 8, 9, 15, 16, 17, 23, 24)
    n = len(counts)
    ru = orc.OracleRules(R, C)
    states = np.zeros((n, 34, R, C), dtype=np.int64)
    for e, c in enumerate(counts):
        st = states[e]
        st[5, 1, 0] = v.max_turns
        st[5, 0, 0] = 10
        st[0, 2, 0] = 2; st[3, 2, 0] = 13                       # p1 scout, about to attack
        st[1, 3, 0] = 12; st[4, 3, 0] = 13; st[33, 3, 0] = 1     # p2 bomb
        st[0, 0, 5] = 11; st[3, 0, 5] = 13; st[32, 0, 5] = 1     # flags
        st[1, 5, 5] = 11; st[4, 5, 5] = 13; st[33, 5, 5] = 1
        st[1, 5, 0] = 3; st[4, 5, 0] = 13                        # a p2 miner so that nobody is stuck
        st[7 + 2, 3, 0] = c                                      # c p1 scouts already died on the bomb's cell
        st[19 + 3, 1, 1] = 11                                    # and 11 p2 miners somewhere else (two events from the start)
    players = np.ones(n, dtype=np.int8)
    env = VecStrategoEnv('many66', n, seed=3, obs_channel_mode=channel_mode, final_obs=True)
    san = torch.zeros(n, dtype=torch.uint8, device=env.device)
    env.import_state_checked(states, players, san)
    assert int(san.sum()) == 0
    back, _ = env.export_state()
    assert np.array_equal(back.cpu().numpy(), states)
    oenv = orc.OracleEnv(R, C, v.max_turns, v.obstacle_locations, v.piece_counts, obs_channel_mode=channel_mode)
    obs, mask, _ = env.observe()
    a = ru.get_action_spatial_index_from_positions(2, 0, 3, 0)
    a_flat = (a[0] * C + a[1]) * ru.K + a[2]
    for e in range(n):
        o = oenv.reset(initial_state_override=states[e])[1]
        assert o[oenv.POBS].tobytes() == obs[e].cpu().numpy().tobytes(), (e, 'obs before')
        assert np.array_equal(o[oenv.MASK], mask[e].cpu().numpy())
    env.step(torch.full((n,), a_flat, dtype=torch.int32))
    after, pl = env.export_state()
    after, obs_h = after.cpu().numpy(), env.obs.cpu().numpy()
    for e, c in enumerate(counts):
        oenv.reset(initial_state_override=states[e])
        o, rew, done, info = oenv.step({1: a_flat})
        assert not done['__all__'] and int(env.invalid_action[e]) == 0
        assert np.array_equal(after[e], oenv.state), (e, c, np.argwhere(after[e] != oenv.state)[:4])
        assert after[e][7 + 2, 3, 0] == c + 1
        assert o[-1][oenv.POBS].tobytes() == obs_h[e].tobytes(), (e, c, 'obs after')
    env.close()
