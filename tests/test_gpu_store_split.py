"""The plain share of the observation writes (KParams::plain_lines, sgx_obs.h: emit_codes<..., NT = true>; the rule that chooses it:
stratego_env_amd/csrc/sgx_store_policy.h).  The rule gives a share only to multi-step launches of tens of thousands of games, so here the
count is FORCED through SGX_NT_PLAIN_LINES (read by sgx_create): non-temporal stores with that many leading 128-byte lines of every
game's observation(s) plain -- 0, 1, one sweep (8), 9, one less than all, all, and one far beyond.  Which lines go which way must not
change a byte:

  * a forced env against a twin on 'auto' stepped alongside, and against the CPU oracle;
  * every output of the forced env lives in an arena of tests/test_gpu_guard_bands.py (guard | poisoned payload | guard, guards of 4 KiB)
    at observation phases 0, 16, 112 and 1008 bytes past a 1 KiB boundary, so that the count meets sweeps and lines that start before
    the game's first float; the twin's outputs are poisoned before every call as well;
  * calls of 7 steps in place, into a ring of 3 and into a 4-slot trajectory buffer entered at slot 2 (it wraps), all multi-step
    launches, and one per-step launch under the same forced count (per-step launches and the kernels of BOTH mode take the non-temporal
    path of a forced count but read no count: their cases pin that nothing else changes).

The rule itself, as the host fills it from a live handle (occupancy query, bytes per game, sets), is pinned at the headline's shape through
SGX_STORE_POLICY_DEBUG=1, which makes the library print what it chose."""
import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS
from tests.helpers import oracle_cvariant
from tests.boards import _table
from tests.guard_bands import (Arena, F32_QUAD_PHASES, I32_PHASES, _compare, _guards, _make, _phase_set, _play, _swap_outputs, _sync,
                               _written_after_step)

pytestmark = pytest.mark.gpu

RESULTS = ('reward', 'done', 'player', 'invalid_action', 'ending_invalid', 'next_actions')
BEYOND = 1 << 19
STEPS, SETS, SLOTS, FIRST_SLOT = 7, 3, 4, 2


def _lines(name, both=False):
    v = VARIANTS[name]
    return -(-(v.cells * (79 if both else 67) * 4) // 128)


def _counts(name):
    n = _lines(name)
    return (0, 1, 8, 9, n - 1, n, BEYOND)


def _poison(t):
    import torch
    if t is not None:
        t.view(-1).view(torch.uint8).fill_(0x5A)


def _same(a, b, what):
    import torch
    assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), what


def _pair(name, n, count, both, monkeypatch):
    """(forced env, its oracle, the twin on 'auto'): the same games."""
    from stratego_env_amd.vec_env import VecStrategoEnv
    monkeypatch.setenv('SGX_NT_PLAIN_LINES', str(count))
    forced, ora = _make(name, n, auto_reset=True, full_obs=both)
    monkeypatch.delenv('SGX_NT_PLAIN_LINES')
    twin = VecStrategoEnv(name, n, seed=forced.seed, env_id_offset=forced.env_id_offset, placement='plain', auto_reset=True, full_obs=both)
    for e in (forced, twin):
        e.reset()
        e.sample_valid_actions()
    return forced, ora, twin


def _run_calls(name, n, count, both, k0, monkeypatch, warm=0):      # noqa: C901
    """The four calls; with warm > 0 the oracle is not stepped alongside (too slow that far into the games): the twin stands in call by call
    and the oracle's digest of the very last step closes the run."""
    from stratego_env_amd import _lib
    forced, ora, twin = _pair(name, n, count, both, monkeypatch)
    dev = forced.device
    stepped = warm == 0
    if warm:
        forced.rollout_steps(warm)
        twin.rollout_steps(warm)
        _sync(forced)
        _same(forced.obs, twin.obs, (name, 'warm-up'))
    acts = twin.next_actions.cpu().numpy().copy()
    outs = ('obs', 'mask') + (('fobs',) if both else ())
    phases_seen = set()

    def expect(n_steps):
        return _play(ora, acts, n_steps) if stepped else None

    # ---- in place
    what = (name, n, 'count', count, 'both', both, 'in place')
    ar = _swap_outputs(forced, _phase_set(k0, True))
    phases_seen.add(ar['obs'].phase)
    forced.next_actions.copy_(twin.next_actions)
    for k in outs + RESULTS[:-1]:
        _poison(getattr(twin, k))
    forced.rollout_steps(STEPS)
    twin.rollout_steps(STEPS)
    _sync(forced)
    assert forced.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE and twin.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE, what
    _guards(ar, what)
    for k, a in ar.items():
        a.check_written(what)
        _same(a.t, getattr(twin, k), what + (k,))
    xs = expect(STEPS)
    if stepped:
        _compare(ar, dict(xs[-1], final={}), what)
        acts = xs[-1]['next_actions'].copy()

    # ---- ring of three
    what = (name, n, 'count', count, 'both', both, 'ring')
    res = _swap_outputs(forced, _phase_set(k0 + 1, True), names=RESULTS)
    sets = []
    for s in range(SETS):
        ph = _phase_set(k0 + 1 + s, True)
        sets.append({k: Arena('%s[set %d]' % (k, s), getattr(forced, k).shape, getattr(forced, k).dtype, ph[k], dev) for k in outs})
        phases_seen.add(sets[-1]['obs'].phase)
    forced._ring = [(a['obs'].t, a['mask'].t, a['fobs'].t if both else None) for a in sets]
    forced._ring_ios = (_lib.SgxStepIO * SETS)()
    forced._ring_pos = 1
    twin.alloc_output_ring(SETS, tune=False)
    for tensors in twin._ring:
        for t in tensors:
            _poison(t)
    forced.next_actions.copy_(twin.next_actions)
    forced.rollout_steps(STEPS, ring=True)
    twin.rollout_steps(STEPS, ring=True)
    _sync(forced)
    assert forced.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE and twin.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE, what
    xs = expect(STEPS)
    _guards(res, what)
    for s, a in enumerate(sets):
        _guards(a, what + ('set', s))
        for j, k in enumerate(('obs', 'mask', 'fobs')[:len(outs)]):
            a[k].check_written(what + ('set', s))
            _same(a[k].t, twin._ring[s][j], what + ('set', s, k))
        if stepped:
            last = [x for i, x in enumerate(xs) if (1 + i) % SETS == s][-1]
            _compare(a, last, what + ('set', s))
    for k, a in res.items():
        a.check_written(what)
        _same(a.t, getattr(twin, k), what + (k,))
    if stepped:
        _compare(res, dict(xs[-1], final={}), what)
        acts = xs[-1]['next_actions'].copy()

    # ---- a 4-slot trajectory buffer entered at slot 2: the 7 steps wrap around its end
    what = (name, n, 'count', count, 'both', both, 'trajectory')
    ph = _phase_set(k0 + 2, True)
    shapes = {'obs': (forced.obs.shape, forced.obs.dtype), 'mask': (forced.mask.shape, forced.mask.dtype), 'reward': ((n, 2), forced.reward.dtype),
              'done': ((n,), forced.done.dtype), 'player': ((n,), forced.player.dtype), 'invalid_action': ((n,), forced.invalid_action.dtype),
              'ending_invalid': ((n,), forced.ending_invalid.dtype), 'actions': ((n,), forced.next_actions.dtype)}
    if both:
        shapes['fobs'] = (forced.fobs.shape, forced.fobs.dtype)
    tar = {k: Arena('traj[%s]' % k, (SLOTS,) + tuple(sh), dt, ph['next_actions' if k == 'actions' else k], dev) for k, (sh, dt) in shapes.items()}
    phases_seen.add(tar['obs'].phase)
    na = _swap_outputs(forced, {'next_actions': I32_PHASES[k0 % 4]}, names=('next_actions',))
    ttraj = twin.alloc_trajectory(SLOTS)
    for t in ttraj.values():
        _poison(t)
    forced.next_actions.copy_(twin.next_actions)
    forced.rollout_trajectory(STEPS, {k: a.t for k, a in tar.items()}, first_slot=FIRST_SLOT)
    twin.rollout_trajectory(STEPS, ttraj, first_slot=FIRST_SLOT)
    _sync(forced)
    assert forced.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE and twin.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE, what
    xs = expect(STEPS)
    _guards(tar, what)
    _guards(na, what)
    for k, a in tar.items():
        assert not bool(a.unwritten().any()), what + (k, 'a slot keeps the poison')          # 7 steps reach all 4 slots
        _same(a.t, ttraj[k], what + (k,))
    _same(na['next_actions'].t, twin.next_actions, what + ('next_actions',))
    if stepped:
        h = {k: a.host() for k, a in tar.items()}
        slots = {(FIRST_SLOT + i) % SLOTS: x for i, x in enumerate(xs)}
        for s, x in slots.items():
            for k in ('mask', 'player', 'done', 'invalid_action'):
                assert np.array_equal(h[k][s], x[k]), what + (k, 'slot', s)
            assert np.array_equal(h['actions'][s], x['next_actions']), what + ('action log', 'slot', s)
            assert h['obs'][s].tobytes() == x['obs'].tobytes(), what + ('obs', 'slot', s)
            assert not both or h['fobs'][s].tobytes() == x['fobs'].tobytes(), what + ('fobs', 'slot', s)
        acts = xs[-1]['next_actions'].copy()

    # ---- one launch per step under the same forced count
    what = (name, n, 'count', count, 'both', both, 'per-step launch')
    ar = _swap_outputs(forced, _phase_set(k0 + 3, True))
    phases_seen.add(ar['obs'].phase)
    forced.next_actions.copy_(twin.next_actions)
    for k in outs + RESULTS[:-1]:
        _poison(getattr(twin, k))
    forced.rollout_step()
    twin.rollout_step()
    _sync(forced)
    assert forced.last_launch_kind == _lib.LAUNCH_WAVE and twin.last_launch_kind == _lib.LAUNCH_WAVE, what
    _guards(ar, what)
    for k, a in ar.items():
        a.check_written(what)
        _same(a.t, getattr(twin, k), what + (k,))
    if stepped:
        x = dict(ora.step(acts), final={})
        _written_after_step(ar, x, what)
        _compare(ar, x, what)
    assert phases_seen == set(F32_QUAD_PHASES), "the four calls cover every observation phase a 4-aligned board allows"
    assert int(forced.invalid_action.sum()) == 0
    total = warm + 3 * STEPS + 1
    return forced, twin, ar, total


def _cases():
    out = []
    for name in ('barrage', 'octa_barrage'):              # batches: 1, one workgroup + 1, a prime around 250
        for i, count in enumerate(_counts(name)):
            out += [(name, 1, count, False), (name, 9, count, False)] if name == 'barrage' else [(name, (9, 1)[i % 2], count, False)]
        out.append((name, 251, 9, False))
        out.append((name, 251, _lines(name) - 1, False))
    for i, count in enumerate(_counts('barrage')):           # BOTH mode: the count applies to both observations (the full one has more lines)
        out.append(('barrage', (9, 1, 9, 9, 1, 9, 9)[i], count, True))
    out.append(('barrage', 251, 8, True))
    out.append(('barrage', 9, _lines('barrage', both=True) - 1, True))
    return out


@pytest.mark.parametrize('name,n,count,both', _cases())
def test_forced_plain_lines_change_no_byte(monkeypatch, name, n, count, both):
    forced, twin, _, _ = _run_calls(name, n, count, both, (count + n) % 4, monkeypatch)
    forced.close()
    twin.close()


@pytest.mark.parametrize('count', [1, 8, 9, BEYOND])
def test_standard_mid_game_uncoded_entries_under_a_forced_count(monkeypatch, count):
    """Standard 300 steps into the games: captured miners / majors / bombs give normalised counts without a 4-bit code, so emit_codes<CHECKED>
    leaves their quads out, sends their lines the plain way (line_esc) and patch_uncoded completes them -- next to lines that are plain by
    the count."""
    name, n, warm = 'standard', 9, 300
    forced, twin, ar, total = _run_calls(name, n, count, False, count % 4, monkeypatch, warm=warm)
    h = {k: a.host() for k, a in ar.items()}
    o = h['obs']
    assert np.any((o != 0) & (np.abs(o) != 1) & (np.abs(o) != 0.5) & (np.abs(o) != 0.25) & (np.abs(o) != 0.75)), \
        'no uncoded entry in any observation: the rollout is too short for what this test is for'
    cv = oracle_cvariant(name, setups=_table(name))
    for e in range(n):
        r = orc.rollout_ex(cv, forced.seed, forced.env_id_offset + e, 1, total, threads=1)
        got = orc.step_digest(h['mask'][e], o[e], h['reward'][e], h['done'][e], h['player'][e], h['ending_invalid'][e])
        assert int(r['last_digests'][0]) == got, (name, 'env', e, 'count', count)
    forced.close()
    twin.close()


def test_the_rule_as_the_host_fills_it_at_the_headline_shape(monkeypatch, capfd):
    """65,536 Barrage games on 'auto': in place the resident games' rewrite set fits the budget (all plain); into a ring of three the launch
    keeps non-temporal stores with the share the budget leaves after mask and results -- 72 lines on 256 CUs with 3 resident workgroups
    of 8 games.  What the library printed is checked against the arithmetic of sgx_store_policy.h on the figures it printed, and those
    figures against the device and the kernel (53,232 B of LDS: 3 workgroups per CU)."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    n = 65536
    monkeypatch.setenv('SGX_STORE_POLICY_DEBUG', '1')
    env = VecStrategoEnv('barrage', n, seed=3, auto_reset=True, placement='plain')
    monkeypatch.delenv('SGX_STORE_POLICY_DEBUG')
    env.reset()
    capfd.readouterr()
    env.rollout_steps(2)
    env.alloc_output_ring(3, tune=False)
    env.rollout_steps(3, ring=True)
    torch.cuda.synchronize()
    assert env.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE
    rows = []
    for ln in capfd.readouterr().err.splitlines():
        if ln.startswith('sgx store policy:'):
            w = ln.replace('->', '').split()[3:]
            rows.append({k: int(v) for k, v in zip(w[0::2], w[1::2])})
    assert len(rows) == 2, rows
    obs_b, mask_b, res_b, sweep = 4 * 67 * 100, 37 * 100, 12, 1024
    cus = torch.cuda.get_device_properties(env.device).multi_processor_count
    for r, sets in zip(rows, (1, 3)):
        assert r['kind'] == 0 and r['games'] == n and r['sets'] == sets and r['cus'] == cus and r['games_per_wg'] == 8, r
        assert r['resident_wgs_per_cu'] == 3, r
        resident = min(n, r['cus'] * r['resident_wgs_per_cu'] * r['games_per_wg'])
        assert r['rewrite_set'] == resident * sets * (obs_b + mask_b + res_b), r
        if r['rewrite_set'] <= r['budget']:
            assert r['nt_stores'] == 0, r
        else:
            want = max(0, (r['budget'] // (resident * sets) - mask_b - res_b) // sweep) * 8
            assert r['nt_stores'] == 1 and r['plain_lines'] == min(want, (-(-obs_b // 128)) // 8 * 8), r
    assert rows[0]['nt_stores'] == 0
    assert rows[1]['nt_stores'] == 1 and (cus != 256 or rows[1]['plain_lines'] == 72), rows[1]
    env.close()
