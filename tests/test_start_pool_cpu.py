"""Start pools (sgx_set_start_pool): the C ABI's new symbols, and -- oracle only, no GPU -- the rule every game start follows while a
pool is set, played by a follower that the GPU tests (tests/test_gpu_start_pool.py) compare every slot of a multi-step launch with.

The rule (include/stratego_mi355x.h): game `game_no` of env `e` starts from pool record j = rng_below(rng(seed, env_id_offset + e, game_no,
stream 4, 0), n_pool) -- whole: boards, never-moved flags, clock, recent moves, captures -- with the record's mover, or, with a random
first player, -1 when rng_below(rng(..., stream 4, 1), 2) == 1 else +1; restart_clock puts turn = 0 and max_turns = the variant's.

The adequacy test makes sure the inputs of the GPU tests end enough games for those tests to mean something: a floor per case, taken
from the counts measured on the oracle with exactly these inputs (table in START_POOL_CASES)."""
import pytest

from tests.pool_roots import POOL_N, START_POOL_CASES, follower_for


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_start_pool_symbols():
    from stratego_env_amd import _lib
    L = _lib.load()
    for sym in ('sgx_set_start_pool', 'sgx_set_start_index_out', 'sgx_start_pool_size'):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert L.sgx_abi_version() == _lib.ABI_VERSION == 15
    assert (_lib.POOL_RANDOM_FIRST_PLAYER, _lib.POOL_RESTART_CLOCK) == (1, 2)
    assert L.sgx_start_pool_size(None) == 0


def test_set_start_pool_fails_loudly_without_a_handle():
    """No device here, so no handle can exist: every entry point of the feature says so instead of touching anything."""
    from stratego_env_amd import _lib
    L = _lib.load()
    rc = L.sgx_set_start_pool(None, None, 0, 0)
    assert rc < 0 and b'sgx_set_start_pool' in L.sgx_last_error()
    rc = L.sgx_set_start_index_out(None, None)
    assert rc < 0 and b'sgx_set_start_index_out' in L.sgx_last_error()
    with pytest.raises(_lib.SgxError):
        _lib.check(L.sgx_set_start_pool(None, None, 1, 0), L)


# ---- input adequacy, oracle only --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(START_POOL_CASES))
def test_the_inputs_end_enough_games(name):
    """The follower alone, actions from the counter RNG like a rollout: the number of games that end (and restart from the pool) must
    reach the floor of the case -- the GPU test has to reproduce the follower's count exactly."""
    fo, steps, floor = follower_for(name)
    assert len(fo.states) == POOL_N
    for _ in range(steps):
        fo.step()
    print('%s: %d endings in %d x %d steps, %d of %d pool entries touched' % (name, fo.restarts, fo.n, steps, len(fo.touched), POOL_N))
    assert fo.restarts >= floor, (name, fo.restarts, floor)
    assert all(0 <= j < POOL_N for j in fo.touched)
