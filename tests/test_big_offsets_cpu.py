"""The threshold arithmetic of tests/big_offsets.py (no GPU): which games straddle 2^31 / 2^32 bytes and 2^31 elements, and that the
witness chunks tile a batch."""
import pytest

from tests import big_offsets as bo


@pytest.mark.parametrize('bpg,item', [(26800, 4), (31600, 4), (60300, 4), (3216, 4), (3700, 1), (3584, 1), (51300, 4), (27200, 8), (12825, 1), (4, 4), (1 << 31, 1)])
def test_thresholds_name_the_game_that_holds_the_boundary(bpg, item):
    th = bo.thresholds(bpg, item)
    for g, boundary in ((th.b31, 1 << 31), (th.b32, 1 << 32), (th.e31, (1 << 31) * item)):
        assert g * bpg <= boundary < (g + 1) * bpg          # the boundary byte lies in game g: a batch of g + 1 games holds it, one of g games does not


def test_the_sizes_the_cases_are_written_for():
    assert bo.thresholds(26800).b32 + 300 == 160559                       # Barrage observations, 4.3 GB
    assert bo.thresholds(60300, 4).e31 + 100 == 142553                    # Standard2 observations past 2^31 floats
    assert 83000 < bo.thresholds(51300).b32 < 84000                       # Standard2 logits
    assert bo.thresholds(3700, 1).b32 == 1160801                          # Barrage byte masks
    assert bo.thresholds(8, 4).e31 == 1 << 30 and bo.thresholds(8, 8).e31 == 1 << 31


def test_straddlers_are_inside_the_batch_and_sorted():
    n = bo.thresholds(26800).b32 + 300
    s = bo.straddlers(n, 26800)
    th = bo.thresholds(26800)
    assert s == sorted(set(s)) and s[0] == 0 and s[-1] == n - 1
    assert th.b31 in s and th.b31 - 1 in s and th.b32 in s and th.b32 - 1 in s
    assert th.e31 >= n and th.e31 not in s                                # 2^31 floats is beyond this batch
    assert bo.straddlers(10, 26800) == [0, 9]


@pytest.mark.parametrize('n,chunk', [(1, 16384), (16384, 16384), (16385, 16384), (160560, 16384), (7, 3)])
def test_witness_chunks_tile_the_batch(n, chunk):
    ch = bo.witness_chunks(n, chunk)
    assert ch[0][0] == 0 and sum(m for _, m in ch) == n
    for (k0, m0), (k1, _) in zip(ch, ch[1:]):
        assert k0 + m0 == k1 and m0 == chunk
    assert 0 < ch[-1][1] <= chunk


def test_reduced_coverage_keeps_every_straddling_chunk():
    n, chunk = 160560, 16384
    keep = bo.straddlers(n, 26800)
    ch = bo.witness_chunks(n, chunk, every=2, keep=keep)
    assert len(ch) < len(bo.witness_chunks(n, chunk))
    for g in keep:
        assert any(k <= g < k + m for k, m in ch), g
    assert bo.FRONT_4G % 4096 == 0 and bo.FRONT_8G % 4096 == 0 and bo.FRONT_4G > 1 << 31 and bo.FRONT_8G > 1 << 33


def test_create_refuses_a_batch_the_32_bit_launch_quantities_cannot_hold():
    """sgx_create: n_envs outside [1, 2^30] is SGX_EINVAL before the device is touched (so this needs no GPU).  The bound is what keeps
    the int32 xcd_first / xcd_count of a launch, its grid size and the one-workgroup-per-game grids of sgx_reset / sgx_sample_valid in
    range; 1 and 2^30 themselves pass this check."""
    import ctypes as C
    from stratego_env_amd import _lib
    from stratego_env_amd import build as hip_build
    from stratego_env_amd.config import VARIANTS
    hip_build.build()
    lib = _lib.load()
    cfg = _lib.make_config(VARIANTS['micro'])
    for n in (0, -1, (1 << 30) + 1, 1 << 31, 1 << 32, (1 << 32) + 64):
        h = C.c_void_p()
        assert lib.sgx_create(C.byref(cfg), C.c_int64(n), 0, 1, 0, C.byref(h)) == -1 and not h.value, n
        assert b'n_envs out of range' in lib.sgx_last_error(), n
    # the inclusive side: 1 and 2^30 pass THIS check (a device index no machine has ends the call at the next one, before anything is allocated)
    for n in (1, 1 << 30):
        h = C.c_void_p()
        assert lib.sgx_create(C.byref(cfg), C.c_int64(n), 1 << 20, 1, 0, C.byref(h)) != 0 and not h.value, n
        assert b'n_envs out of range' not in lib.sgx_last_error(), (n, lib.sgx_last_error())
