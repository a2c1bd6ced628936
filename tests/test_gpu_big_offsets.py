"""Large offsets: every address a kernel computes from an index, past 2^31 and 2^32 bytes (and 2^31 elements) of ONE tensor.

No other file of the suite hands a kernel a tensor of more than 1.76 GB, so a dropped (int64_t) cast in a per-env base, a slot stride, a
replay stride or a record offset would pass all of them.  Here every case runs the call on a tensor past the boundary it names and
compares it, exactly (torch.equal, no tolerance), with WITNESSES: handles of a few thousand games with env_id_offset = k, which by the
draw contract produce what games [k, k + m) of the big handle produce, at low offsets (tests/big_offsets.py).  The
comparison covers the whole batch, chunk by chunk; the first game, the last game and the games at the boundaries are anchored against the
CPU oracle as well.  The big tensors live in arenas whose front guard (2 GiB, or 8 GiB for the element-index cases) turns a wrong offset
into a wrong byte.  Every tensor is poisoned again BEFORE every call (on the big handle and in the witnesses); after every call the
guards are intact and nothing the call must write holds the poison.  Against the witnesses go, after every call, the small outputs
(rewards, flags, players, actions: whole batch) and, at the END of a sequence, every tensor; the big tensors' contents after the calls
in between are held against the oracle at the anchors only (the same kernel wrote them with the same addressing as the last call).

Every test states what it holds on the device at once (witnesses included), skips below that + 2 GiB of free memory, holds at most 24 GiB
and gives everything back before it returns.

MEASURED on one MI355X (287 GiB free, nothing skipped): `pytest -q -m gpu tests/test_gpu_big_offsets.py` reports 22 passed in 7.14 s
(without the interpreter's start, about 2 s more).  Per test in that run, in seconds: compact steps 0.96; sgx_step x 3 with both
observations 0.90 (it starts the process); pool writes 0.42; pool reads 0.35; lane kernels with uncoded entries 0.34; functional API 0.29;
Standard2 past 2^31 floats 0.21; Micro past 2^31 floats 0.21; mask-only 0.17; ring 0.16; chooser 0.15; plain stores 0.15; sgx_step_n +
export 0.14; replay step-major 0.13, game-major 0.06; decoders 0.11; the five trajectory cases 0.08 each; the refusal under 0.01.  A test that is the
first of its process to allocate a size pays the device allocation: run group by group the same tests took up to 5.1 s (functional
API), 3.8 s (compact steps), 2.4 s (Micro, the trajectory case of 65 Micro games, lane kernels with uncoded entries); inside the whole
GPU suite (904 passed in 281 s) the slowest was 5.9 s.  No coverage was cut: every witness chunk of every batch is compared.

CASES (N, tensor, boundary crossed) -- DESIGN section 6, "Large offsets", has the table:
  step kernels, per-env offset   Barrage, N = 160,559: obs 4.30 GB (fobs 5.07 GB) past 2^31 and 2^32 bytes: sgx_step x 3 with BOTH
                                 observations and the size rule's non-temporal stores; sgx_step x 3 with sgx_set_nt_stores(0); sgx_step_n
                                 of 5 steps (steps_kernel) + sgx_export_state / sgx_get_env_info; sgx_step_ring over 3 sets in three arenas
  element index                  Standard2, N = 142,553 (wave kernels) and Micro, N = 2,671,104 (lane kernels): obs 8.6 GB past 2^31 floats
  lane kernels, uncoded entries  a 4x4 board of three sergeants and a flag per side, N = 2,003,392: obs 8.6 GB past 2^31 floats
  functional API                 Barrage, 158,203 int64 states: state_in / state_out 4.30 GB past 2^32 bytes; sgx_step_states fused and in
                                 three launches with 2 chains, general states every 97th, 1-D masks; sgx_import_state_checked
  mask-only                      Barrage, N = 1,161,101: mask 4.30 GB past 2^32 bytes, two games per wave (what SGX_MUTANT_OFFSET32 breaks)
  slot stride, small batch       sgx_step_traj, N = 64 (Barrage) / 65 (Micro), 3 slots, slot_envs so that slot 1 starts past 2^32 bytes
                                 and slot 2 past 2^31 floats of obs; multi-step launch and one launch per step; first_slot 2
  compact outputs, decoders      Barrage compact, N = 1,198,672: records 4.30 GB past 2^32 bytes; sgx_decode_obs / sgx_decode_mask of
                                 Standard2, N = 142,553, into 8.6 GB past 2^31 floats
  chooser                        Standard2, N = 84,022: logits 4.31 GB past 2^32 bytes, byte mask 1.08 GB past 2^30, the bit mask;
                                 sgx_decode_mask, sgx_choose_actions (T = 0, 1), sgx_sample_valid
  pools, reads                   Standard2 records past 2^32 bytes of `boards`: src_index naming record 0, the straddlers, the last
  pools, writes                  a destination pool of the same size, every record written by each call; witnesses of 2^20 records
  replay strides                 N = 64, int32 lists with step_stride ([T][N_wide]) / game_stride ([N_wide][T]) reaching past 2^32 bytes"""
import ctypes as C

import numpy as np
import pytest

from tests import big_offsets as bo
from tests.big_offsets import BigArena, GIB, GUARD

pytestmark = pytest.mark.gpu

SEED = 0x0B160FF5
SMALL = ('reward', 'done', 'player', 'invalid_action', 'ending_invalid', 'next_actions')


def _handle(name, n, g0=0, **kw):
    """records only (outputs=False): the output tensors are the test's own -- arenas for the big handle, torch.empty for a witness --
    so that no placement search runs and nothing of the big size is allocated twice"""
    from stratego_env_amd.vec_env import VecStrategoEnv
    if kw.get('compact_outputs'):                      # (a compact handle cannot be a records-only pool: its own tensors go at once)
        env = VecStrategoEnv(name, n, seed=SEED, env_id_offset=g0, auto_reset=True, placement='plain', **kw)
        env.obs = env.mask = None
        bo.release()
        return env
    return VecStrategoEnv(name, n, seed=SEED, env_id_offset=g0, auto_reset=True, outputs=False, placement='plain', **kw)


class _Outs:
    """the tensors of one run, by name, in the order they were made; big=True: arenas (front guard `front` for tensors of more than
    2^31 bytes, 4 KiB for the others), else torch.empty"""

    def __init__(self, device, big, front=bo.FRONT_4G):
        self.device, self.big, self.front = device, big, front
        self.t, self.arena = {}, {}

    def make(self, name, shape, dtype, front=None):
        import torch
        if self.big:
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
            a = BigArena(name, shape, dtype, front if front is not None else self.front if nbytes > (1 << 31) else GUARD, self.device)
            self.arena[name], self.t[name] = a, a.t
        else:                                             # what nobody writes (a compact record's padding) is the poison on both sides
            t = torch.empty(tuple(shape), dtype=dtype, device=self.device)
            flat = t.view(-1).view(torch.uint8)
            whole = flat.numel() // 4 * 4
            flat[:whole].view(torch.int32).fill_(bo.POISON_INT)
            flat[whole:] = torch.tensor(bo.POISON_BYTES[:flat.numel() - whole], dtype=torch.uint8, device=self.device)
            self.t[name] = t
        return self.t[name]

    def held(self):
        return sum(a.held for a in self.arena.values()) if self.big else sum(t.numel() * t.element_size() for t in self.t.values())

    def poison(self, keep=('next_actions',)):
        """before a call: every tensor holds the poison again (not `keep`: next_actions is the call's INPUT too), so that "nothing the
        call must write still holds the poison" is a statement about THIS call, on the big handle and in the witnesses alike"""
        import torch
        for k, t in self.t.items():
            if k in keep:
                continue
            if self.big:
                self.arena[k].poison()
            else:
                flat = t.view(-1).view(torch.uint8)
                whole = flat.numel() // 4 * 4
                flat[:whole].view(torch.int32).fill_(bo.POISON_INT)
                flat[whole:] = torch.tensor(bo.POISON_BYTES[:flat.numel() - whole], dtype=torch.uint8, device=self.device)


def _attach(env, outs, full=False, obs=True):
    import torch
    N, R, Cc, K = env.num_envs, env.R, env.Cc, env.K
    if env.compact:
        env.obs = outs.make('obs', (N, env.compact_obs_stride), torch.uint8)
        env.mask = outs.make('mask', (N, env.compact_mask_words), torch.int32)
    else:
        env.obs = outs.make('obs', (N, R, Cc, env.p_channels), torch.float32) if obs else None
        env.mask = outs.make('mask', (N, R, Cc, K), torch.uint8)
    env.fobs = outs.make('fobs', (N, R, Cc, env.f_channels), torch.float32) if full else None
    for k in SMALL:
        t = getattr(env, k)
        setattr(env, k, outs.make(k, t.shape, t.dtype))


# ---- the call sequences: run alike on the big handle and on every witness ------------------------------------------------------------------
# rec(what, steps, written): after every call.  steps = how many steps the call played; written = the tensors it must have written, as
# names, or (name, oracle key, step of this call whose results it holds) where the name is not the oracle's key / not the last step.
def _start(env, outs, rec, full, obs=True):
    _attach(env, outs, full=full, obs=obs)
    env.reset()
    rec('reset', 0, [k for k in ('obs', 'fobs', 'mask', 'player') if k in outs.t])
    outs.poison(keep=('mask',))                       # (the sampler reads the mask)
    env.sample_valid_actions()
    rec('sample', 0, ['next_actions'])


def _all_written(outs):
    return [k for k in ('obs', 'fobs', 'mask') + SMALL if k in outs.t]


def _seq_steps(n_steps, full=False, nt=None, emit_obs=True):
    def seq(env, outs, rec):
        from stratego_env_amd import _lib
        if nt is not None:
            env.set_nt_stores(nt)
        _start(env, outs, rec, full, obs=emit_obs)
        for t in range(n_steps):
            outs.poison()
            env.step(env.next_actions, want_next_actions=True, emit_obs=emit_obs)
            assert env.last_launch_kind == _lib.LAUNCH_WAVE
            rec('sgx_step %d' % t, 1, _all_written(outs))
    return seq


def _seq_step_n(n_steps):
    def seq(env, outs, rec):
        import torch
        from stratego_env_amd import _lib
        _start(env, outs, rec, False)
        outs.poison()
        env.rollout_steps(n_steps)
        assert env.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE, env.last_launch_kind
        rec('sgx_step_n(%d)' % n_steps, n_steps, _all_written(outs))
        N = env.num_envs
        st = outs.make('state', (N, 34, env.R, env.Cc), torch.int64)
        pl = outs.make('state_player', (N,), torch.int8)
        info = outs.make('info', (N, 4), torch.int32)
        with torch.cuda.device(env.device):
            _lib.check(env._L.sgx_export_state(env._h, C.c_void_p(st.data_ptr()), C.c_void_p(pl.data_ptr()), env._stream()), env._L)
            _lib.check(env._L.sgx_get_env_info(env._h, C.c_void_p(info.data_ptr()), env._stream()), env._L)
        rec('export + info', 0, [('state_player', 'player', 0)])
        outs.check_all_written = ('state', 'state_player', 'info')
    return seq


def _seq_ring(n_sets, n_steps):
    def seq(env, outs, rec):
        from stratego_env_amd import _lib
        _start(env, outs, rec, False)
        sets = [(env.obs, env.mask, None)]
        for s in range(1, n_sets):
            sets.append((outs.make('obs[set %d]' % s, env.obs.shape, env.obs.dtype), outs.make('mask[set %d]' % s, env.mask.shape, env.mask.dtype), None))
        env._ring, env._ring_ios, env._ring_pos = sets, (_lib.SgxStepIO * n_sets)(), 1
        outs.poison()
        env.rollout_steps(n_steps, ring=True)
        assert env.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE, env.last_launch_kind
        written = list(SMALL)
        for i in range(n_steps):                      # step i of the call wrote set (1 + i) % n_sets; the last writer of a set stands
            s = (1 + i) % n_sets
            if i + n_sets >= n_steps:
                written += [('obs[set %d]' % s if s else 'obs', 'obs', i), ('mask[set %d]' % s if s else 'mask', 'mask', i)]
        rec('sgx_step_ring(%d sets, %d steps)' % (n_sets, n_steps), n_steps, written)
    return seq


def _norm(written, steps):
    return [(w, w, steps - 1) if isinstance(w, str) else w for w in written]


def _run_against_witnesses(name, n, seq, row_bytes, chunk, front=bo.FRONT_4G, every=1, final_check=None, **handle_kw):
    """The whole procedure of a stepping case; row_bytes: of the tensor whose boundaries name the straddling games."""
    import torch
    from tests.guard_bands import Oracle
    dev = torch.device('cuda', 0)
    anchors = bo.straddlers(n, row_bytes)
    compact = bool(handle_kw.get('compact_outputs'))
    env = _handle(name, n, **handle_kw)
    outs = _Outs(dev, True, front)
    aidx = torch.as_tensor(anchors, device=dev)
    calls = []                                        # per call: (what, steps, written, {small tensor: clone}, {tensor: anchors' rows on the host})

    def rec(what, steps, written):
        torch.cuda.synchronize(dev)
        for a in outs.arena.values():
            a.check_guards((name, n, what))
        wr = _norm(written, steps)
        for k, _, _ in wr:
            if not (compact and k in ('obs', 'mask')):  # (the padding of a compact record is written by nobody: the witnesses' poison decides)
                outs.arena[k].check_written((name, n, what))
        small = {k: outs.t[k].clone() for k, _, _ in wr if outs.t[k].numel() * outs.t[k].element_size() <= (64 << 20)}
        rows = {k: outs.t[k][aidx].cpu().numpy() for k, _, _ in wr}
        calls.append((what, steps, wr, small, rows))
    seq(env, outs, rec)
    for k in getattr(outs, 'check_all_written', ()):
        outs.arena[k].check_written((name, n, 'export'))
    if final_check is not None:
        final_check(outs)
    env.close()
    # ---- the witnesses: the whole batch, chunk by chunk ----------------------------------------------------------------------------------
    chunks = bo.witness_chunks(n, chunk, every=every, keep=anchors)
    for k, m in chunks:
        w = _handle(name, m, g0=k, **handle_kw)
        wo = _Outs(dev, False)
        wcalls = []
        seq(w, wo, lambda what, steps, written: wcalls.append({kk: wo.t[kk].clone() for kk, _, _ in _norm(written, steps) if kk in calls[len(wcalls)][3]}))
        assert len(wcalls) == len(calls)
        for (what, _, _, small, _), ws in zip(calls, wcalls):
            for kk, t in small.items():
                bo.assert_rows_equal(t, ws[kk], k, (name, n, what, kk, 'witness of games [%d, %d)' % (k, k + m)))
        for kk, t in outs.t.items():
            bo.assert_rows_equal(t, wo.t[kk], k, (name, n, 'at the end', kk, 'witness of games [%d, %d)' % (k, k + m)))
        w.close()
        del w, wo, wcalls
    # ---- the oracle anchors --------------------------------------------------------------------------------------------------------------
    for j, g in enumerate(anchors):
        ora = Oracle(name, SEED, g, 1, auto_reset=True)
        acts = None
        for what, steps, wr, _, rows in calls:
            xs = []
            for _ in range(steps):
                xs.append(ora.step(acts))
                acts = xs[-1]['next_actions'].copy()
            if not steps:
                xs = [ora.current()]
                if what == 'sample':
                    acts = xs[0]['next_actions'].copy()
            for kk, key, at in wr:
                x = xs[max(at, 0)]
                if key not in x or (key in ('reward', 'ending_invalid') and not x.get('legal', [True])[0]) or (compact and key in ('obs', 'mask')):
                    continue
                got, want = rows[kk][j], np.asarray(x[key][0])
                assert got.tobytes() == np.ascontiguousarray(want).astype(got.dtype).tobytes(), (name, n, what, kk, 'game', g, 'against the oracle')
    held = outs.held()
    del outs, calls, aidx, rec
    bo.release()
    return held, len(chunks)


def _obs_bytes(name, full=False):
    from stratego_env_amd.config import VARIANTS, PO_OBS_CHANNELS, FO_OBS_CHANNELS
    v = VARIANTS[name]
    return v.rows * v.columns * (FO_OBS_CHANNELS if full else PO_OBS_CHANNELS) * 4


def _mask_bytes(name):
    from stratego_env_amd.config import VARIANTS
    v = VARIANTS[name]
    return v.rows * v.columns * v.spatial_channels


# ---- per-env offsets of the step kernels, 4 GiB class ---------------------------------------------------------------------------------
def _n_barrage():
    return bo.thresholds(_obs_bytes('barrage')).b32 + 300


STEP_PATHS = {
    # path: (sequence, tensors of the big size: observation sets, BOTH?, export?)
    'sgx_step-x3-both-observations': (_seq_steps(3, full=True), 1, True, False),
    'sgx_step-x3-plain-stores': (_seq_steps(3, nt=0), 1, False, False),
    'sgx_step_n-5-and-export': (_seq_step_n(5), 1, False, True),
    'sgx_step_ring-3-sets': (_seq_ring(3, 4), 3, False, False),
}


@pytest.mark.parametrize('path', list(STEP_PATHS))
def test_step_kernels_past_4_gib_of_observations(path):
    """Barrage, N = thresholds(26,800 B).b32 + 300 = 160,559 games: the float32 observation is 4.30 GB (the fully-observable one 5.07 GB, it
    crosses earlier), so games 80,129 and 160,259 hold bytes 2^31 and 2^32.  The store policy is left alone except in the plain-stores path:
    at this size the rule picks non-temporal stores, which no small test takes unforced.  Witnesses of 16,384 games over the whole batch."""
    seq, sets, full, export = STEP_PATHS[path]
    n, chunk = _n_barrage(), 16384
    per_game = sets * (_obs_bytes('barrage') + _mask_bytes('barrage')) + (_obs_bytes('barrage', True) if full else 0) + (34 * 100 * 8 + 40 if export else 0) + 64 + 512
    guards = (sets + (1 if full else 0) + (1 if export else 0)) * bo.FRONT_4G
    need = n * per_game + guards + chunk * per_game + GIB          # + the comparisons' temporaries
    bo.gate(need)
    held, n_chunks = _run_against_witnesses('barrage', n, seq, _obs_bytes('barrage', full), chunk)
    print(path, 'arenas held %.2f GiB, %d witnesses' % (held / GIB, n_chunks))


def test_mask_only_steps_past_4_gib_of_masks():
    """Barrage, N = thresholds(3,700 B, 1).b32 + 300 = 1,161,101 games, no observation tensor at all: 3 mask-only steps (the two-games-per-
    wave launch) into a byte mask of 4.30 GB.  This is the case tools/mutant_check.sh's SGX_MUTANT_OFFSET32 has to fail, naming a game at
    2^32 bytes.  Witnesses of 65,536 games over the whole batch."""
    n, chunk = bo.thresholds(_mask_bytes('barrage'), 1).b32 + 300, 65536
    per_game = _mask_bytes('barrage') + 64 + 512
    bo.gate(n * per_game + bo.FRONT_4G + chunk * per_game + GIB)
    held, n_chunks = _run_against_witnesses('barrage', n, _seq_steps(3, emit_obs=False), _mask_bytes('barrage'), chunk)
    print('mask-only: arenas held %.2f GiB, %d witnesses' % (held / GIB, n_chunks))


# ---- element-index class: past 2^31 floats of one observation tensor (front guard 8 GiB) --------------------------------------------
def _seq_step_then_step_n(n_steps, lane):
    def seq(env, outs, rec):
        from stratego_env_amd import _lib
        if lane:
            env.set_lane_kernel(True)
        _start(env, outs, rec, False)
        outs.poison()
        env.step(env.next_actions, want_next_actions=True)
        assert env.last_launch_kind == (_lib.LAUNCH_LANE if lane else _lib.LAUNCH_WAVE), env.last_launch_kind
        rec('sgx_step', 1, _all_written(outs))
        outs.poison()
        env.rollout_steps(n_steps)
        assert env.last_launch_kind == (_lib.LAUNCH_MULTI_STEP if lane else _lib.LAUNCH_MULTI_STEP_WAVE), env.last_launch_kind
        rec('sgx_step_n(%d)' % n_steps, n_steps, _all_written(outs))
    return seq


@pytest.mark.parametrize('name,chunk', [('standard2', 16384), ('micro', 131072)])
def test_step_kernels_past_2_31_floats_of_observations(name, chunk):
    """The float INDEX of an observation entry passes 2^31 (8 GiB): Standard2 (15x15, 60,300 B per game), N = thresholds(60,300, 4).e31
    + 100 = 142,553 games, 8.6 GB, on the wave kernels (sgx_step, then sgx_step_n of 3 steps); Micro (3,216 B per game), N = 2,671,104
    games (the next multiple of 64 past 2^31 floats + 100 games), on the lane kernels (sgx_set_lane_kernel(1): the per-step lane kernel,
    then lane_steps_kernel).  The arena's front guard is 8 GiB: a 32-bit element index of a 4-byte type lands at most that far before the
    payload.  Witnesses over the whole batch; oracle anchors at 2^31 bytes, 2^32 bytes and 2^31 floats.  (Micro's pieces all have 4-bit
    codes: the lane kernels' uncoded entries are the next test's, on 4x4.)"""
    lane = name == 'micro'
    n = bo.thresholds(_obs_bytes(name), 4).e31 + 100
    if lane:
        n = (n + 63) & ~63
    assert n * _obs_bytes(name) > (1 << 31) * 4
    per_game = _obs_bytes(name) + _mask_bytes(name) + 64 + 1024
    bo.gate(n * per_game + bo.FRONT_8G + chunk * per_game + GIB)
    held, n_chunks = _run_against_witnesses(name, n, _seq_step_then_step_n(3, lane), _obs_bytes(name), chunk, front=bo.FRONT_8G)
    print(name, 'arenas held %.2f GiB, %d witnesses' % (held / GIB, n_chunks))


THIRDS44 = 'thirds44'


def test_lane_kernels_with_uncoded_entries_past_2_31_floats():
    """The lane kernels' uncoded entries (`dstf[unc_idx[k]]`: observation values without a 4-bit code, patched in behind the sweep) at a
    sub-batch base past 2^31 floats: a 4x4 board (lane eligible, a built-in geometry) whose side is three sergeants and a flag on one
    row -- the thirds66 piece set of tests/test_gpu_compact.py on a board the lane kernels take -- so that a captured sergeant
    normalises to 1/3.  4,288 B of observation per game, N = 2,003,392 games (the next multiple of 64 past 2^31 floats + 100 games),
    8.6 GB behind an 8 GiB front guard; the per-step lane kernel, then lane_steps_kernel with 5 steps (a capture takes three plies);
    the launch kinds are asserted, so a refusal of the piece set by the lane kernels would fail here.  The observation written last must
    hold values that are no multiple of 1/4 -- uncoded entries -- in games on both sides of 2^31 floats."""
    from stratego_env_amd import config
    v = config.custom_variant(4, 4, max_turns=60, piece_counts=(0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 1, 0), initial_state_usable_rows=1, name=THIRDS44)
    config.VARIANTS[THIRDS44] = v
    try:
        n = (bo.thresholds(_obs_bytes(THIRDS44), 4).e31 + 100 + 63) & ~63
        chunk = 131072
        per_game = _obs_bytes(THIRDS44) + _mask_bytes(THIRDS44) + 64 + 1024
        bo.gate(n * per_game + bo.FRONT_8G + chunk * per_game + 2 * GIB)
        e31 = bo.thresholds(_obs_bytes(THIRDS44), 4).e31

        def uncoded_on_both_sides(outs):
            obs = outs.t['obs']
            for lo, hi in ((0, e31), (e31, n)):
                seen = 0
                for a in range(lo, hi, 65536):
                    x = obs[a:min(a + 65536, hi)] * 4
                    seen += int((x != x.round()).sum())
                assert seen > 0, 'no uncoded entry in the observations of games [%d, %d): the case does not reach what it is for' % (lo, hi)
        held, n_chunks = _run_against_witnesses(THIRDS44, n, _seq_step_then_step_n(5, True), _obs_bytes(THIRDS44), chunk, front=bo.FRONT_8G,
                                                final_check=uncoded_on_both_sides)
        print(THIRDS44, 'N', n, 'arenas held %.2f GiB, %d witnesses' % (held / GIB, n_chunks))
    finally:
        config.VARIANTS.pop(THIRDS44, None)


# ---- the slot stride of sgx_step_traj with a small batch ------------------------------------------------------------------------------
TRAJ = ('obs', 'mask', 'reward', 'done', 'player', 'invalid_action', 'ending_invalid', 'actions')


def _traj_call(env, t0, slot_envs, n_slots, first, n_steps, per_slot=True):
    """sgx_step_traj on the tensors t0 (name -> slot 0's [slot_envs-strided] tensor) -- VecStrategoEnv.rollout_trajectory passes slot_envs =
    num_envs, so the call is made here"""
    import torch
    from stratego_env_amd import _lib
    env.obs, env.mask = t0['obs'], t0['mask']
    if per_slot:
        env.reward, env.done, env.player = t0['reward'], t0['done'], t0['player']
        env.invalid_action, env.ending_invalid = t0['invalid_action'], t0['ending_invalid']
    io = env._fill_io(env.next_actions, True, True, True, 0)
    t = _lib.SgxTrajIO()
    C.memmove(C.byref(t.io), C.byref(io), C.sizeof(_lib.SgxStepIO))
    t.n_slots, t.results_per_slot, t.slot_envs = n_slots, 1 if per_slot else 0, slot_envs
    t.actions_log_dev = t0['actions'].data_ptr()
    with torch.cuda.device(env.device):
        _lib.check(env._L.sgx_step_traj(env._h, C.byref(t), first, n_steps, env._stream()), env._L)


@pytest.mark.parametrize('name,n,compact,per_step', [('barrage', 64, False, False), ('barrage', 64, False, True), ('micro', 65, False, False), ('micro', 64, False, False),
                                                     ('barrage', 64, True, False)])
def test_step_traj_slot_stride_past_4_gib(name, n, compact, per_step, monkeypatch):
    """sgx_step_traj with 3 slots whose stride, slot_envs games, puts slot 1 past 2^32 bytes and slot 2 past 2^33 bytes = 2^31 floats of
    the observation tensor, with only n = 64 / 65 games in each slot: `set * obs_slot_bytes`, `env + slot * traj_res_envs`, the action
    log's `set * traj_out_envs`.  first_slot = 2 with 3 steps, so the wrap addresses the high slots first.  Each slot equals a dense [3, n]
    trajectory of a twin env (the layout tests/test_gpu_trajectory.py pins to the oracle); the rows [n, slot_envs) of the huge slots keep
    the poison.  per_step: the same with one launch per step (SGX_MULTI_STEP_WAVE=0); compact: the compact records' and bit masks' strides;
    on Micro the big handle runs lane_steps_kernel with 64 and with 65 games (its slot stride is even); of the twins only the one of 64
    games does, the twin of 65 runs steps_kernel."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    if per_step:
        monkeypatch.setenv('SGX_MULTI_STEP_WAVE', '0')
        monkeypatch.setenv('SGX_MULTI_STEP', '0')
    dev = torch.device('cuda', 0)
    kw = dict(seed=SEED, auto_reset=True, placement='plain', compact_outputs=compact)
    env, twin = VecStrategoEnv(name, n, **kw), VecStrategoEnv(name, n, **kw)
    obs_row = int(np.prod(env.obs.shape[1:])) * env.obs.element_size()
    item = env.obs.element_size()
    # slot 1 past 2^32 bytes; slot 2 then lies past 2^33 bytes = 2^31 elements of a float32 tensor; a multiple of 4 keeps the results aligned
    slot_envs = (bo.thresholds(obs_row, item).b32 + 4) & ~3
    assert slot_envs * obs_row > 1 << 32 and 2 * slot_envs * obs_row > (1 << 31) * 4
    rows = 2 * slot_envs + n
    shapes = {'obs': (env.obs.shape[1:], env.obs.dtype), 'mask': (env.mask.shape[1:], env.mask.dtype), 'reward': ((2,), torch.float32), 'done': ((), torch.uint8),
              'player': ((), torch.int8), 'invalid_action': ((), torch.uint8), 'ending_invalid': ((), torch.uint8), 'actions': ((), torch.int32)}
    need = sum(rows * int(np.prod(sh, dtype=np.int64)) * torch.empty((), dtype=dt).element_size() for sh, dt in shapes.values()) + bo.FRONT_8G + GIB
    bo.gate(need)
    ar = {k: BigArena('traj[%s]' % k, (rows,) + tuple(sh), dt, bo.FRONT_8G if k == 'obs' else GUARD, dev) for k, (sh, dt) in shapes.items()}
    for e in (env, twin):
        e.reset()
        e.sample_valid_actions()
    dense = twin.alloc_trajectory(3)
    for k in ('obs', 'mask'):                         # (a compact record's padding is written by nobody: the same poison on both sides)
        dense[k].view(-1).view(torch.int32).fill_(bo.POISON_INT)
    T, first, n_steps = 3, 2, 3
    twin.rollout_trajectory(n_steps, dense, first_slot=first)
    _traj_call(env, {k: a.t[:n] for k, a in ar.items()}, slot_envs, T, first, n_steps)
    torch.cuda.synchronize(dev)
    what = (name, n, 'slot_envs', slot_envs, 'per-step launches' if per_step else 'multi-step launch')
    # (the lane kernel wants every slot as aligned as slot 0: an even slot stride of whole 16 bytes -- slot_envs is a multiple of 4, the
    # twin's stride is its n: 65 Micro games are lane_steps_kernel here and steps_kernel in the twin, one more witness)
    kinds = [_lib.LAUNCH_WAVE if per_step else (_lib.LAUNCH_MULTI_STEP if (name == 'micro' and stride % 2 == 0) else _lib.LAUNCH_MULTI_STEP_WAVE) for stride in (slot_envs, n)]
    assert [env.last_launch_kind, twin.last_launch_kind] == kinds, what + (env.last_launch_kind, twin.last_launch_kind, kinds)
    for k, a in ar.items():
        a.check_guards(what)
        for s in range(T):
            if not (compact and k == 'obs'):
                a.check_written(what + ('slot', s), rows=(s * slot_envs, s * slot_envs + n))
            bo.assert_rows_equal(a.t, dense[k][s], s * slot_envs, what + (k, 'slot', s))
            if s < T - 1:
                a.check_unwritten(what + ('slot', s), rows=(s * slot_envs + n, (s + 1) * slot_envs))
    assert torch.equal(env.next_actions, twin.next_actions)
    env.close(); twin.close()
    del ar, dense, env, twin, a
    bo.release()


# ---- compact outputs and their decoders -----------------------------------------------------------------------------------------------
def test_compact_steps_past_4_gib_of_records():
    """Barrage with compact outputs (3,584 B of codes per game), N = thresholds(3,584, 1).b32 + 300 = 1,198,672 games: `env *
    compact_stride` past 2^32 bytes (the bit masks, `env * MB_WORDS`, stay below: 0.6 GB).  reset, then 2 steps; the compact records and
    bit masks equal those of compact witnesses of 65,536 games over the whole batch, the results are anchored against the oracle."""
    name, chunk = 'barrage', 65536
    env = _handle(name, 8, compact_outputs=True)
    stride, words = env.compact_obs_stride, env.compact_mask_words
    env.close()
    n = bo.thresholds(stride, 1).b32 + 300
    per_game = stride + 4 * words + 64 + 512
    # (a compact handle allocates its own tensors first, and its sampler decodes the bit masks into 3,700 bytes per game)
    bo.gate(n * (per_game + stride + 4 * words + _mask_bytes(name)) + bo.FRONT_4G + chunk * (2 * per_game + _mask_bytes(name)) + GIB)
    held, n_chunks = _run_against_witnesses(name, n, _seq_steps(2), stride, chunk, compact_outputs=True)
    print('compact: stride', stride, 'N', n, 'arenas held %.2f GiB, %d witnesses' % (held / GIB, n_chunks))


def test_decoders_past_2_31_floats():
    """sgx_decode_obs / sgx_decode_mask of Standard2, N = thresholds(60,300, 4).e31 + 100 = 142,553 games (the API decodes a whole handle,
    and 1.2 M decoded Barrage games would be 32 GB): the decoded observation is 8.6 GB, past 2^31 floats, in an arena with an 8 GiB front
    guard; the decoded mask 1.8 GB.  Byte-equal to the UNCOMPACT outputs of witnesses of 16,384 games that played the same step, and to
    the oracle at the anchors."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tests.guard_bands import Oracle
    name, chunk = 'standard2', 16384
    dev = torch.device('cuda', 0)
    n = bo.thresholds(_obs_bytes(name), 4).e31 + 100
    probe = VecStrategoEnv(name, 8, seed=SEED, placement='plain', compact_outputs=True)
    compact_bytes = probe.compact_obs_stride + 4 * probe.compact_mask_words
    probe.close()
    # the decoded tensors, the compact ones, the bytes the sampler decodes the bit masks into, the records and results; a witness without the compact ones
    per_game = _obs_bytes(name) + 2 * _mask_bytes(name) + compact_bytes + 4096
    bo.gate(n * per_game + bo.FRONT_8G + chunk * per_game + GIB)
    env = VecStrategoEnv(name, n, seed=SEED, auto_reset=True, placement='plain', compact_outputs=True)
    env.reset()
    env.sample_valid_actions()
    env.step(env.next_actions, want_next_actions=True)
    dobs = BigArena('decoded obs', (n, env.R, env.Cc, env.p_channels), torch.float32, bo.FRONT_8G, dev)
    dmask = BigArena('decoded mask', (n, env.R, env.Cc, env.K), torch.uint8, GUARD, dev)
    env.decode_obs(out=dobs.t)
    env.decode_mask(out=dmask.t)
    torch.cuda.synchronize(dev)
    for a in (dobs, dmask):
        a.check_guards('decode'); a.check_written('decode')
    for k, m in bo.witness_chunks(n, chunk):
        w = _handle(name, m, g0=k)
        wo = _Outs(dev, False)
        _attach(w, wo)
        w.reset()
        w.sample_valid_actions()
        w.step(w.next_actions, want_next_actions=True)
        where = 'witness of games [%d, %d)' % (k, k + m)
        bo.assert_rows_equal(dobs.t, w.obs, k, ('decoded obs', where))
        bo.assert_rows_equal(dmask.t, w.mask, k, ('decoded mask', where))
        bo.assert_rows_equal(env.next_actions, w.next_actions, k, ('next_actions', where))
        w.close()
        del w, wo
    for g in bo.straddlers(n, _obs_bytes(name)):
        ora = Oracle(name, SEED, g, 1, auto_reset=True)
        x = ora.step(ora.current()['next_actions'])
        assert dobs.t[g].cpu().numpy().tobytes() == x['obs'][0].tobytes() and np.array_equal(dmask.t[g].cpu().numpy(), x['mask'][0]), ('game', g, 'against the oracle')
    env.close()
    del env, dobs, dmask, a
    bo.release()


# ---- the chooser ----------------------------------------------------------------------------------------------------------------------
def test_chooser_past_4_gib_of_logits():
    """Standard2 (12,825 actions, 51,300 B of logits per game), N = thresholds(51,300).b32 + 300 = 84,022 games: logits of 4.31 GB, a
    byte mask of 1.08 GB (past 2^30 bytes; sgx_decode_mask writes it from the bit mask of a compact reset) and the bit mask.
    sgx_choose_actions with T = 0 and T = 1 on both masks and sgx_sample_valid on the bytes: the answers are integers and equal exactly
    what witnesses of 8,192 games with env_id_offset = k choose on the slice [k, k + m) of the SAME logits with masks of their own."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, chunk = 'standard2', 8192
    dev = torch.device('cuda', 0)
    na = _mask_bytes(name)
    n = bo.thresholds(na * 4).b32 + 300
    assert n * na > 1 << 30
    need = n * (na * 5 + 16384) + chunk * (na + 16384) + 2 * GIB
    bo.gate(need)
    kw = dict(seed=SEED, auto_reset=True, placement='plain', compact_outputs=True)
    env = VecStrategoEnv(name, n, **kw)
    env.reset()
    bytes_arena = BigArena('decoded mask', (n, env.R, env.Cc, env.K), torch.uint8, GUARD, dev)
    env.decode_mask(out=bytes_arena.t)
    logits = torch.empty((n, na), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261)
    for k, m in bo.witness_chunks(n, chunk):
        logits[k:k + m].normal_(0.0, 3.0, generator=gen)
    calls = [('bits', 0.0), ('bits', 1.0), ('bytes', 0.0), ('bytes', 1.0), ('sample', None)]
    got = {}
    for c in calls:
        out = BigArena('chosen %s' % (c,), (n,), torch.int32, GUARD, dev)
        if c[0] == 'sample':
            env.sample_valid_actions(mask=bytes_arena.t, out=out.t)
        else:
            env.choose_actions(logits, temperature=c[1], mask=env.mask if c[0] == 'bits' else bytes_arena.t, out=out.t)
        got[c] = out
    torch.cuda.synchronize(dev)
    bytes_arena.check_guards('decode_mask'); bytes_arena.check_written('decode_mask')
    for c, out in got.items():
        out.check_guards(c); out.check_written(c)
        assert int((out.t < 0).sum()) == 0, (c, 'an env without a choice')
    assert not torch.equal(got[('bytes', 0.0)].t, got[('bytes', 1.0)].t), 'argmax and the draw agree everywhere: the logits do not tell them apart'
    for k, m in bo.witness_chunks(n, chunk):
        w = VecStrategoEnv(name, m, env_id_offset=k, **kw)
        w.reset()
        wbytes = w.decode_mask()
        where = 'witness of games [%d, %d)' % (k, k + m)
        bo.assert_rows_equal(env.mask, w.mask, k, ('bit mask', where))
        bo.assert_rows_equal(bytes_arena.t, wbytes, k, ('decoded mask', where))
        for c in calls:
            if c[0] == 'sample':
                out = w.sample_valid_actions(mask=wbytes, out=torch.empty((m,), dtype=torch.int32, device=dev))
            else:
                out = w.choose_actions(logits[k:k + m], temperature=c[1], mask=w.mask if c[0] == 'bits' else wbytes, out=torch.empty((m,), dtype=torch.int32, device=dev))
            bo.assert_rows_equal(got[c].t, out, k, (c, where))
        w.close()
    # anchors: the chosen action is valid in the oracle's mask of that game, and the sampler's is the oracle's draw
    from tests.guard_bands import Oracle
    for g in bo.straddlers(n, na * 4):
        ora = Oracle(name, SEED, g, 1, auto_reset=True)
        cur = ora.current()
        assert np.array_equal(bytes_arena.t[g].cpu().numpy().reshape(-1), cur['mask'][0].reshape(-1)), ('mask of game', g, 'against the oracle')
        assert int(got[('sample', None)].t[g]) == int(cur['next_actions'][0]), ('sampled action of game', g, 'against the oracle')
        row = logits[g].cpu().numpy().astype(np.float64)
        valid = np.flatnonzero(cur['mask'][0].reshape(-1))
        best = valid[np.argmax(row[valid])]
        for kind in ('bits', 'bytes'):
            assert int(got[(kind, 0.0)].t[g]) == int(best), ('argmax of game', g, kind)
            assert int(got[(kind, 1.0)].t[g]) in set(valid.tolist()), ('draw of game', g, kind)
    env.close()
    del env, logits, bytes_arena, got, out
    bo.release()


# ---- replay strides -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['step-major', 'game-major'])
def test_replay_strides_past_4_gib(layout):
    """sgx_replay of 64 Barrage games whose int32 lists lie in a log of 4.58 GB: `env * game_stride + lane * step_stride` and
    `t0 * step_stride`.  step-major: a [T = 520][N_wide = 2,200,000] log, the games are its last 64 columns (step_stride = N_wide: entry t of
    a list lies t x 8.8 MB further, past 2^31 bytes from t = 245 and past 2^32 from t = 489).  game-major: a dense [N_wide][T] log, the
    games are 64 rows spread evenly up to the last one (game_stride = 34,920 x 520: game 30 starts past 2^31 bytes, game 60 past 2^32; the
    LAST rows alone would move the offset into the base pointer and test no product).  The lists are what the games drew in 520 rollout
    steps; lengths straddle the prefetch chunk (32 entries) and reach the end.  Results and records equal the same lists given densely."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, n, T, wide = 'barrage', 64, 520, 2200000
    dev = torch.device('cuda', 0)
    bo.gate(wide * T * 4 + GIB)
    env = VecStrategoEnv(name, n, seed=SEED, auto_reset=False, placement='plain')
    env.reset()
    roots = env.snapshot()
    env.sample_valid_actions()
    lists = torch.empty((n, T), dtype=torch.int32, device=dev)
    for t in range(T):
        lists[:, t] = env.next_actions
        env.rollout_step()
    lengths = torch.as_tensor([(T, T - 1, 0, 1, 31, 32, 33, 67, 243, 245, 487, 489, 300, 64, 65, 519)[i % 16] for i in range(n)], dtype=torch.int32, device=dev)
    log = torch.full((T, wide) if layout == 'step-major' else (wide, T), -7, dtype=torch.int32, device=dev)
    if layout == 'step-major':
        log[:, wide - n:] = lists.T
        view = log[:, wide - n:].T
        assert view.stride() == (1, wide) and (T - 1) * wide * 4 > 1 << 32
    else:
        step = (wide - 1) // (n - 1)
        log[::step][:n] = lists
        view = log[::step][:n]
        assert view.stride() == (step * T, 1) and (n - 1) * step * T * 4 > 1 << 32 and view.data_ptr() == log.data_ptr()
    assert tuple(view.shape) == (n, T) and torch.equal(view, lists)
    got, want = PackedStates(name, n, seed=SEED), PackedStates(name, n, seed=SEED)
    res = got.replay(roots, view, lengths=lengths)
    ref = want.replay(roots, lists, lengths=lengths)
    torch.cuda.synchronize(dev)
    for k in ('applied', 'consumed', 'stop', 'reward', 'done', 'ending_invalid', 'player'):
        bo.assert_rows_equal(getattr(res, k), getattr(ref, k), 0, (layout, k))
    (gs, gp), (ws, wp) = got.unpack(), want.unpack()
    assert torch.equal(gs, ws) and torch.equal(gp, wp), (layout, 'records')
    # anchor: the longest lists end where the env itself stands after T steps
    es, ep = env.export_state()
    full = torch.nonzero(lengths == T).flatten()
    assert torch.equal(gs[full], es[full]) and torch.equal(gp[full], ep[full]), (layout, 'the replayed games are not where the env went')
    for p in (got, want, roots, env):
        p.close()
    del log, view, lists, got, want, roots, env
    bo.release()


# ---- pools past 4 GiB: reads through src_index -------------------------------------------------------------------------------------
def _same(a, b, what):
    """tensors, or tuples of tensors, bit for bit"""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, what + (i,))
    elif a is not None or b is not None:
        bo.assert_rows_equal(a if a.dim() else a.reshape(1), b if b.dim() else b.reshape(1), 0, what)


def test_pool_reads_past_4_gib_of_records():
    """Standard2 (15x15, the largest packed record of the main library), a pool of thresholds(record bytes, 1).b32 + 300 records: more
    than 2^32 bytes of `boards`, filled by sgx_copy_envs from 256 mid-game records (src_index = i % 256; sgx_state_keys over ALL records
    then equals the 256 keys tiled: the copy's writes and the keys' reads over the whole pool).  A dst of 256 slots reads it through
    src_index lists naming record 0, the records that straddle 2^31 and 2^32 bytes, the last record, and duplicates of these:
    sgx_copy_envs, sgx_expand (+ the 1-D mask), sgx_determinize, sgx_determinize_weighted with a shared table and with one table per
    record (a second pool whose BELIEF tensor passes 2^32 bytes: the `s_rec * belief_stride` product), sgx_playout and
    sgx_playout_weighted (max_steps 8), sgx_replay untracked and tracked (origins_in indexed by the high src_index), sgx_count_moves +
    sgx_expand_all, sgx_state_keys with an index -- leaf values set on dst.  The witness is the same call with `src` a pool of six
    records that holds copies of the named ones at indices 0..5: every output and dst's records are byte-equal."""
    import torch
    from stratego_env_amd import leaf_values as LV
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, m, n = 'standard2', 256, 256
    dev = torch.device('cuda', 0)
    small = VecStrategoEnv(name, m, seed=SEED, auto_reset=False, placement='plain')
    small.reset()
    small.rollout_steps(120, emit_obs=False, emit_mask=False)
    rec, cells = small.record_bytes, small.R * small.Cc
    th = bo.thresholds(rec, 1)
    NP = th.b32 + 300
    table_bytes = 2 * 12 * cells * 2
    tb = bo.thresholds(table_bytes, 1)
    N2 = tb.b32 + 300
    bo.gate(NP * (rec + 4 * cells + 16) + N2 * (rec + table_bytes) + 2 * GIB)
    pool = PackedStates(name, NP, seed=SEED)
    pool.copy_from(small, src_index=torch.arange(NP, dtype=torch.int32, device=dev) % m)
    keys_small = small.state_keys(wide=True)
    keys_all = pool.state_keys(wide=True)
    assert torch.equal(keys_all, keys_small[torch.arange(NP, device=dev) % m]), 'the filled pool is not the 256 records tiled'
    del keys_all
    named = [0, th.b31 - 1, th.b31, th.b32 - 1, th.b32, NP - 1]
    assert named == sorted(set(named)) and (NP - 1) * rec > 1 << 32
    wit = PackedStates(name, len(named), seed=SEED)
    wit.copy_from(small, src_index=torch.as_tensor([g % m for g in named], dtype=torch.int32, device=dev))
    rs = np.random.RandomState(7)
    pick = np.concatenate([np.arange(len(named)), rs.randint(len(named), size=n - len(named))])
    widx = torch.as_tensor(pick, dtype=torch.int32, device=dev)
    idx = torch.as_tensor(np.asarray(named)[pick], dtype=torch.int32, device=dev)
    first_valid = wit.valid_moves_as_1d_mask().to(torch.int32).argmax(dim=1).to(torch.int32)       # an absolute 1-D move every named record's mover has
    acts = first_valid[widx.long()].clone()
    acts[5::7] = 0                                                                                 # and some refused ones
    lists = torch.stack([acts, torch.as_tensor(rs.randint(0, cells * 28, size=n), dtype=torch.int32, device=dev)], dim=1).contiguous()
    lengths = torch.as_tensor(np.arange(n) % 3, dtype=torch.int32, device=dev)
    origins = torch.randint(-1, 2 * cells, (NP, 2, cells), dtype=torch.int16, device=dev)
    w_origins = origins[torch.as_tensor(named, device=dev)].contiguous()
    beliefs = torch.randint(0, 4096, (2, 12, cells), dtype=torch.int16, device=dev)
    weights = rs.randint(0, 4096, size=(4, 13, 14))
    a, b = PackedStates(name, n, seed=SEED + 1, env_id_offset=7), PackedStates(name, n, seed=SEED + 1, env_id_offset=7)
    ca, cb = PackedStates(name, 4096, seed=SEED + 2), PackedStates(name, 4096, seed=SEED + 2)
    for p in (a, b, ca, cb):
        p.set_leaf_values(LV.material(name), 900, LV.side_total(name))
    mask_a = torch.empty((n, a._vec.variant.action_size), dtype=torch.uint8, device=dev)
    mask_b = torch.empty_like(mask_a)

    def res_tuple(r):
        return tuple(getattr(r, k) for k in ('reward', 'done', 'ending_invalid', 'player', 'length', 'applied', 'consumed', 'stop', 'origins', 'parent', 'action', 'total')
                     if getattr(r, k, None) is not None)
    calls = [
        ('sgx_copy_envs', lambda d, s, i, big: None if d.copy_from(s, src_index=i) else None),
        ('sgx_expand', lambda d, s, i, big: tuple(t.clone() for t in d.expand(s, acts, parent_index=i, mask_1d_out=mask_a if big else mask_b))),
        ('sgx_determinize', lambda d, s, i, big: d.determinize(s, src_index=i, draw=3)),
        ('sgx_determinize_weighted, shared table', lambda d, s, i, big: d.determinize(s, src_index=i, draw=4, beliefs=beliefs, return_off_belief=True)),
        ('sgx_playout', lambda d, s, i, big: res_tuple(d.playout(s, src_index=i, max_steps=8, draw=1))),
        ('sgx_playout_weighted', lambda d, s, i, big: res_tuple(d.playout(s, src_index=i, max_steps=8, draw=2, weights=weights))),
        ('sgx_replay', lambda d, s, i, big: res_tuple(d.replay(s, lists, lengths=lengths, src_index=i, actions_1d=True))),
        ('sgx_replay, tracked', lambda d, s, i, big: res_tuple(d.replay(s, lists, lengths=lengths, src_index=i, actions_1d=True, origins_in=origins if big else w_origins))),
        ('sgx_state_keys', lambda d, s, i, big: (s.state_keys(index=i, wide=True), s.state_keys(index=i, observer=0, clock=False))),
        ('sgx_count_moves', lambda d, s, i, big: s.count_moves(index=i)),
    ]
    for what, call in calls:
        got, want = call(a, pool, idx, True), call(b, wit, widx, False)
        torch.cuda.synchronize(dev)
        _same(got, want, (what,))
        _same(a.unpack(), b.unpack(), (what, 'records of dst'))
    _same(mask_a, mask_b, ('sgx_expand', '1-D mask'))
    counts, offsets = pool.count_moves(index=idx[:24])
    assert int(counts.sum()) > 0 and int(offsets[-1]) <= 4096, int(offsets[-1])
    ra, rb = ca.expand_all(pool, src_index=idx[:24], offsets=offsets), cb.expand_all(wit, src_index=widx[:24])
    torch.cuda.synchronize(dev)
    total = int(ra.total)
    assert total == int(rb.total) == int(offsets[-1]) and total > 24
    _same((ra.parent, ra.action), (rb.parent, rb.action), ('sgx_expand_all', 'parent / action'))       # (-1 behind the last child)
    for k in ('reward', 'done', 'ending_invalid', 'player'):                                            # (slots behind the last child are not written)
        _same(getattr(ra, k)[:total], getattr(rb, k)[:total], ('sgx_expand_all', k))
    _same(ca.unpack(), cb.unpack(), ('sgx_expand_all', 'children'))
    # anchor: the record read at the high indices is the mid-game record of `small` it was copied from
    a.copy_from(pool, src_index=idx)
    st_a, st_small = a.unpack()[0], small.export_state()[0]
    assert torch.equal(st_a, st_small[(idx.long() % m)]), 'a high record read back is not the record that was copied there'
    del origins, pool
    bo.release()
    # ---- one belief table per record, the tensor past 2^32 bytes ------------------------------------------------------------------------
    pool2 = PackedStates(name, N2, seed=SEED)
    pool2.copy_from(small, src_index=torch.arange(N2, dtype=torch.int32, device=dev) % m)
    named2 = [0, tb.b31 - 1, tb.b31, tb.b32 - 1, tb.b32, N2 - 1]
    wit2 = PackedStates(name, len(named2), seed=SEED)
    wit2.copy_from(small, src_index=torch.as_tensor([g % m for g in named2], dtype=torch.int32, device=dev))
    tables = torch.zeros((N2, 2, 12, cells), dtype=torch.int16, device=dev)
    assert tables.numel() * 2 > 1 << 32
    w_tables = torch.randint(0, 4096, (len(named2), 2, 12, cells), dtype=torch.int16, device=dev)
    tables[torch.as_tensor(named2, device=dev)] = w_tables
    idx2 = torch.as_tensor(np.asarray(named2)[pick], dtype=torch.int32, device=dev)
    got = a.determinize(pool2, src_index=idx2, draw=5, beliefs=tables, return_off_belief=True, validate=False)
    want = b.determinize(wit2, src_index=widx, draw=5, beliefs=w_tables, return_off_belief=True, validate=False)
    torch.cuda.synchronize(dev)
    _same(got, want, ('sgx_determinize_weighted, one table per record',))
    _same(a.unpack(), b.unpack(), ('sgx_determinize_weighted, one table per record', 'records of dst'))
    assert int((got[0] > 0).sum()) > 0, 'no record had a hidden piece to deal'
    for p in (a, b, ca, cb, wit, wit2, pool2, small):
        p.close()
    del tables, pool2, a, b, ca, cb
    bo.release()


# ---- refusals: sizes a 32-bit launch quantity cannot hold -------------------------------------------------------------------------------
def test_copy_envs_refuses_a_count_its_grid_cannot_hold():
    """sgx_copy_envs with BOTH index arrays is bounded by no handle's size: n >= 2^31 (the grid is a 32-bit count of (n + 3) / 4
    workgroups, and no int32 index tensor of a caller is that long) is SGX_EINVAL before any launch -- two pools of 8 records, nothing
    is read through the index pointers and dst keeps its records.  (n_envs itself is bounded by sgx_create:
    tests/test_big_offsets_cpu.py.)"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    a, b = PackedStates('micro', 8, seed=1), PackedStates('micro', 8, seed=2)
    before = a.unpack()[0].clone()
    idx = torch.zeros((8,), dtype=torch.int32, device=a.device)
    L, st = a._vec._L, a._vec._stream()
    for n in (1 << 31, (1 << 34) + 5, 1 << 62):
        assert L.sgx_copy_envs(a._vec._h, C.c_void_p(idx.data_ptr()), b._vec._h, C.c_void_p(idx.data_ptr()), C.c_int64(n), st) == -1, n
        assert b'sgx_copy_envs: n must be in [0, 2^31)' in L.sgx_last_error(), L.sgx_last_error()
    assert L.sgx_copy_envs(a._vec._h, None, b._vec._h, None, C.c_int64(9), st) == -1 and b'n out of range' in L.sgx_last_error()
    torch.cuda.synchronize(a.device)
    assert torch.equal(a.unpack()[0], before), 'a refused copy wrote records'
    assert L.sgx_copy_envs(a._vec._h, C.c_void_p(idx.data_ptr()), b._vec._h, C.c_void_p(idx.data_ptr()), C.c_int64(8), st) == 0
    a.close(); b.close()


# ---- pools past 4 GiB: writes -------------------------------------------------------------------------------------------------------------
def test_pool_writes_past_4_gib_of_records():
    """A DESTINATION pool of as many Standard2 records as the pool of the read case (more than 2^32 bytes of `boards`), every record
    written by each call: sgx_copy_envs, sgx_expand, sgx_determinize, sgx_playout with max_steps = 1, sgx_replay with lists of length 0,
    1 and 2, and sgx_state_keys over all records.  Witnesses of 2^20 records with env_id_offset = k over the whole pool, reading a source
    of their own with the same records at low indices.  The records are compared through their wide position keys (128 bits of every
    record: the int64 export of 1.7 M Standard2 states would be 100 GB) and every output tensor directly; the records around 2^31 and
    2^32 bytes and the last 128, copied into a small pool and unpacked, byte for byte."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, m, chunk = 'standard2', 256, 1 << 20
    dev = torch.device('cuda', 0)
    small = VecStrategoEnv(name, m, seed=SEED, auto_reset=False, placement='plain')
    small.reset()
    small.rollout_steps(120, emit_obs=False, emit_mask=False)
    rec, cells = small.record_bytes, small.R * small.Cc
    NP = bo.thresholds(rec, 1).b32 + 300
    bo.gate(2 * NP * (rec + 64) + 2 * chunk * (rec + 64) + 2 * GIB)
    first_valid = PackedStates(name, m, seed=SEED)
    first_valid.copy_from(small)
    fv = first_valid.valid_moves_as_1d_mask().to(torch.int32).argmax(dim=1).to(torch.int32)
    first_valid.close()

    def fill(p, k):
        """records [k, k + p.n) of the tiled source, and the inputs of the calls for them"""
        g = torch.arange(k, k + p.n, device=dev)
        p.copy_from(small, src_index=(g % m).to(torch.int32))
        acts = fv[g % m].clone()
        acts[g % 7 == 5] = 0
        lists = torch.stack([acts, ((g * 2654435761) % (cells * 28)).to(torch.int32)], dim=1).contiguous()
        return acts, lists, (g % 3).to(torch.int32)

    def run(src, dst, inputs):
        acts, lists, lengths = inputs
        out = []
        dst.copy_from(src)
        out.append(('sgx_copy_envs', (), dst.state_keys(wide=True)))
        valid, player = dst.expand(src, acts)
        out.append(('sgx_expand', (valid.clone(), player.clone()), dst.state_keys(wide=True)))
        out.append(('sgx_determinize', (dst.determinize(src, draw=2),), dst.state_keys(wide=True)))
        r = dst.playout(src, max_steps=1, draw=3)
        out.append(('sgx_playout', (r.reward, r.done, r.ending_invalid, r.player, r.length), dst.state_keys(wide=True)))
        r = dst.replay(src, lists, lengths=lengths, actions_1d=True)
        out.append(('sgx_replay', (r.applied, r.consumed, r.stop, r.reward, r.done, r.ending_invalid, r.player), dst.state_keys(wide=True)))
        out.append(('sgx_state_keys, information set', (), dst.state_keys(observer=0, clock=False)))
        return out
    src, dst = PackedStates(name, NP, seed=SEED), PackedStates(name, NP, seed=SEED + 3)
    got = run(src, dst, fill(src, 0))
    torch.cuda.synchronize(dev)
    # byte for byte where it matters: the records around 2^31 and 2^32 bytes and the last ones, as the last call (sgx_replay) left them
    th = bo.thresholds(rec, 1)
    window = sorted(set(g for c in (th.b31, th.b32, NP - 64) for g in range(c - 64, c + 64) if 0 <= g < NP))
    win = PackedStates(name, len(window), seed=SEED)
    win.copy_from(dst, src_index=torch.as_tensor(window, dtype=torch.int32, device=dev))
    win_states, win_players = win.unpack()
    win.close()
    for k, n_w in bo.witness_chunks(NP, chunk):
        wsrc, wdst = PackedStates(name, n_w, seed=SEED, env_id_offset=k), PackedStates(name, n_w, seed=SEED + 3, env_id_offset=k)
        want = run(wsrc, wdst, fill(wsrc, k))
        for (what, outs_g, keys_g), (_, outs_w, keys_w) in zip(got, want):
            where = (what, 'witness of records [%d, %d)' % (k, k + n_w))
            bo.assert_rows_equal(keys_g, keys_w, k, where + ('records, by their keys',))
            for i, (a, b) in enumerate(zip(outs_g, outs_w)):
                bo.assert_rows_equal(a, b, k, where + ('output', i))
        sel = [i for i, g in enumerate(window) if k <= g < k + n_w]
        if sel:
            wwin = PackedStates(name, len(sel), seed=SEED)
            wwin.copy_from(wdst, src_index=torch.as_tensor([window[i] - k for i in sel], dtype=torch.int32, device=dev))
            ws, wp = wwin.unpack()
            at = torch.as_tensor(sel, device=dev)
            assert torch.equal(win_states[at], ws) and torch.equal(win_players[at], wp), ('records', window[sel[0]], '..', window[sel[-1]], 'byte for byte')
            wwin.close()
        wsrc.close(); wdst.close()
        del wsrc, wdst, want
    assert int((got[2][1][0] > 0).sum()) > NP // 2 and int(got[1][1][0].sum()) > NP // 2, 'the calls had nothing to do'
    src.close(); dst.close(); small.close()
    del src, dst, got
    bo.release()


# ---- the functional API on int64 states past 4 GiB -----------------------------------------------------------------------------------
def _states_sequence(env, st_in, pl_in, outs, three_launch_chains):
    """What case 6 calls, alike on the big handle and on a witness (the int64 states are the caller's: a witness takes a slice):
    sgx_step_states observing (no actions, the 1-D mask in state coordinates) -> the first valid move of every state; sgx_step_states on
    the fused path (one launch on 10x10: next states, players, the next 1-D mask); sgx_step_states on the three-launch path (a 79-channel
    observation is asked for, `three_launch_chains` chains: import, step, export per chain at env_first = c * per); then
    sgx_import_state_checked and the wide keys of the imported records.  Every call runs the general-state pass (on by default)."""
    import torch
    from stratego_env_amd import _lib
    n, R, Cc = env.num_envs, env.R, env.Cc
    AS = env.variant.action_size
    u8, i8 = torch.uint8, torch.int8

    def call(actions, flags, mask, fobs, s_out, p_out, san, chains):
        io = env._fill_io(actions if actions is not None else env.next_actions, False, False, False, flags)
        io.auto_reset = 0
        if actions is None:
            io.actions_dev = None
        io.mask_dev = mask.data_ptr() if mask is not None else None
        io.fobs_dev = fobs.data_ptr() if fobs is not None else None
        with torch.cuda.device(env.device):
            _lib.check(env._L.sgx_step_states(env._h, C.c_void_p(st_in.data_ptr()), C.c_void_p(pl_in.data_ptr()), C.c_void_p(san.data_ptr()), C.byref(io),
                                              C.c_void_p(s_out.data_ptr()) if s_out is not None else None, C.c_void_p(p_out.data_ptr()) if p_out is not None else None,
                                              chains, env._stream()), env._L)
    for k in ('reward', 'done', 'player', 'invalid_action', 'ending_invalid'):
        t = getattr(env, k)
        setattr(env, k, outs.make(k, t.shape, t.dtype))
    mask0 = outs.make('mask of the given states', (n, AS), u8)
    call(None, _lib.STEP_MASK_1D, mask0, None, None, None, outs.make('sanitised, observe', (n,), u8), 1)
    acts = outs.make('first valid move', (n,), torch.int32)
    acts.copy_(mask0.to(torch.int32).argmax(dim=1).to(torch.int32) if n <= 32768 else
               torch.cat([mask0[a:a + 32768].to(torch.int32).argmax(dim=1) for a in range(0, n, 32768)]).to(torch.int32))
    call(acts, _lib.STEP_ACTIONS_1D | _lib.STEP_MASK_1D, outs.make('mask of the next states', (n, AS), u8), None,
         outs.make('state_out, fused', (n, 34, R, Cc), torch.int64), outs.make('player_out, fused', (n,), i8), outs.make('sanitised, fused', (n,), u8), 2)
    fused_results = {k: getattr(env, k).clone() for k in ('reward', 'done', 'invalid_action', 'ending_invalid')}
    # (this observation gets the 4 KiB guard: three 2 GiB guards do not fit the 24 GiB of a test, and the step kernel's `env * floats per
    # game` into a 79-channel tensor of this size is the BOTH-observations case above, in an arena with the big guard)
    call(acts, _lib.STEP_ACTIONS_1D, None, outs.make('fobs of the next states', (n, R, Cc, env.f_channels), torch.float32, front=GUARD),
         outs.make('state_out, three launches', (n, 34, R, Cc), torch.int64), outs.make('player_out, three launches', (n,), i8),
         outs.make('sanitised, three launches', (n,), u8), three_launch_chains)
    san_imp = outs.make('sanitised, import', (n,), u8)
    env.import_state_checked(st_in, pl_in, san_imp)
    outs.t['keys of the imported records'] = env.state_keys(wide=True)
    for k, t in fused_results.items():
        outs.t[k + ', fused'] = t


def test_step_states_and_import_past_4_gib_of_states():
    """sgx_step_states / sgx_import_state_checked on Barrage int64 states (27,200 B each), N = thresholds(27,200, 8).b32 + 300 =
    158,203 states: state_in and both state_out tensors are 4.30 GB, past 2^31 and 2^32 bytes.  The states are 1,024 real positions (6
    plies into their games) tiled over the batch -- a wrapped offset reads another position -- with every 97th state one of 64 of
    helpers.general_states, which the packed record cannot carry: the redo pass (general states, on) then addresses states up to the
    last one through its list.  The fused path (one launch) and the three-launch path with 2 chains (import / step / export per chain,
    the second chain from env_first = per) both write next states; the 1-D masks in state coordinates of the given and of the next
    states; then the import alone and the keys of what it wrote.  state_out of the two paths must agree; everything equals witnesses of
    8,192 states on SLICES of the same tensors over the whole batch; the next states of the anchors (first, last, straddlers that are
    real positions) equal the oracle's get_next_state."""
    import torch
    from oracle import oracle as orc
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tests.helpers import general_states
    name, chunk, tile, every = 'barrage', 8192, 1024, 97
    dev = torch.device('cuda', 0)
    state_bytes = 34 * 100 * 8
    n = bo.thresholds(state_bytes, 8).b32 + 300
    per_state = 3 * state_bytes + _obs_bytes(name, True) + 2 * 2001 + 1024
    bo.gate(n * per_state + 2 * bo.FRONT_4G + chunk * per_state + GIB)
    seedling = VecStrategoEnv(name, tile, seed=SEED, auto_reset=False, placement='plain')
    seedling.reset()
    seedling.rollout_steps(6)
    st_t, pl_t = seedling.export_state()
    seedling.close()
    gs, gp = general_states(name, 64, np.random.RandomState(97))
    gs, gp = torch.from_numpy(gs).to(dev), torch.from_numpy(gp).to(dev)
    st_in = torch.empty((n, 34, 10, 10), dtype=torch.int64, device=dev)
    pl_in = torch.empty((n,), dtype=torch.int8, device=dev)
    for a in range(0, n, 16384):
        g = torch.arange(a, min(a + 16384, n), device=dev)
        st_in[g], pl_in[g] = st_t[g % tile], pl_t[g % tile]
    g = torch.arange(0, n, every, device=dev)
    st_in[g], pl_in[g] = gs[(g // every) % 64], gp[(g // every) % 64]
    assert (n - 1) // every * every * state_bytes > 1 << 32, 'a general state lies past 2^32 bytes'
    env = _handle(name, n)
    outs = _Outs(dev, True)
    _states_sequence(env, st_in, pl_in, outs, 2)
    torch.cuda.synchronize(dev)
    for k, a in outs.arena.items():
        a.check_guards(k)
        a.check_written(k)
    assert torch.equal(outs.t['state_out, fused'], outs.t['state_out, three launches']) and torch.equal(outs.t['player_out, fused'], outs.t['player_out, three launches'])
    flagged = outs.t['sanitised, import']
    real = torch.ones((n,), dtype=torch.bool, device=dev)
    real[::every] = False
    b32 = bo.thresholds(state_bytes, 8).b32
    assert int(flagged[real].sum()) == 0, 'a position reached by play was altered on import'
    assert int(flagged[b32:].sum()) > 0, 'no state past 2^32 bytes is on the redo list: the general-state pass does not reach what this test is for'
    assert int(outs.t['invalid_action'][real].sum()) == 0 and int(outs.t['sanitised, fused'][real].sum()) == 0, 'a real position: its first valid move refused, or altered'
    env.close()
    for k, m in bo.witness_chunks(n, chunk):
        w = _handle(name, m)
        wo = _Outs(dev, False)
        _states_sequence(w, st_in[k:k + m], pl_in[k:k + m], wo, 1 if (k // chunk) % 2 else 2)
        assert list(wo.t) == list(outs.t)
        for kk, t in outs.t.items():
            bo.assert_rows_equal(t, wo.t[kk], k, (kk, 'witness of states [%d, %d)' % (k, k + m)))
        w.close()
        del w, wo
    ru = orc.OracleRules(10, 10)
    so, po, acts = outs.t['state_out, fused'], outs.t['player_out, fused'], outs.t['first valid move']
    anchors = [x for x in bo.straddlers(n, state_bytes, 8) if x % every]
    assert len(anchors) >= 4
    for x in anchors:
        ns, np_ = ru.get_next_state(st_in[x].cpu().numpy(), int(pl_in[x]), int(acts[x]))
        assert np.array_equal(so[x].cpu().numpy(), ns) and int(po[x]) == int(np_), ('state', x, 'against the oracle')
    del outs, st_in, pl_in, so, po, acts, flagged, real
    bo.release()
