"""The one table of stream cases (support code, no tests): for every entry point of include/stratego_mi355x.h that takes a `void *stream`,
the builders of its cases for the gate harness (tests/stream_gate.py) and CASES, the table itself.  tests/test_gpu_streams.py runs every
row; tests/test_streams_cpu.py holds the table against the header, so a new entry point cannot ship without a row HERE -- the table does
not depend on which test modules were imported.  A builder fills a stream_gate.Case: its handles, staged inputs, compared outputs and
`call(stream pointer, stream)`; a row's optional `after(case)` runs once run_case has passed.  Nothing here touches the GPU at import."""
import ctypes as C
from collections import namedtuple

import numpy as np

from tests.pool_roots import STEP_VS_OUT_SPECS

Spec = namedtuple('Spec', 'id entries variant n build may_wait after')
N_BARRAGE, N_FIVES, N_MICRO = 17, 17, 65     # one workgroup's games plus 1 (10x10: 8 waves of one game, or of two without an observation; 5x5: two per wave; 3x4: 64 per wave)
N_CHAINS = 129                               # the smallest batch sgx_rollout / sgx_step_states split into two chains (units of 64 games), plus 1
N_STEPS = 20
SGX_STEPS_MAX_PER_LAUNCH = 256               # (stratego_mi355x.hip) 257 steps leave one to launch_set_step and its action-log copy


def _chk(c, rc):
    from stratego_env_amd import _lib
    _lib.check(rc, c.M.L)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _io(env, actions, want_next=False, obs=True, mask=True, flags=0, auto_reset=None, chained=False):
    """A private copy of the sgx_step_io the env's own tensors make; chained: next_actions_dev == actions_dev (the rollout calls)."""
    from stratego_env_amd import _lib
    io = _lib.SgxStepIO()
    C.memmove(C.byref(io), C.byref(env._fill_io(actions, want_next, obs, mask, flags)), C.sizeof(io))
    if auto_reset is not None:
        io.auto_reset = auto_reset
    if chained:
        io.next_actions_dev = io.actions_dev
    return io


def _results(c, env, obs=True, mask=True, next_actions=False):
    c.out(env.reward, env.done, env.player, env.invalid_action, env.ending_invalid)
    if obs:
        c.out(env.obs)
    if mask:
        c.out(env.mask)
    if next_actions:
        c.out(env.next_actions)


def _kind(c, env, want):
    got = c.M.L.sgx_last_launch_kind(env._h)
    assert got == want, "the call took launch kind %d, the case is about kind %d" % (got, want)


def _reset(kind):
    def build(c):
        import torch
        M, L = c.M, c.M.L
        e = c.env()
        sel = m1 = m2 = None
        if kind == 'maps':
            i = torch.arange(M.n, device='cuda')
            sel = c.inp((i % 2 == 0).to(torch.uint8), (i % 3 == 0).to(torch.uint8))
            m1, m2 = c.inp(M.maps['A'][0], M.maps['B'][0]), c.inp(M.maps['A'][1], M.maps['B'][1])
        if kind == 'pool':
            e.set_start_states(M.snap['A'])                # (no game of A is over on this board)
            c.out(e.start_index)
        c.call = lambda sp, s: _chk(c, L.sgx_reset(e._h, _p(sel), _p(m1), _p(m2), sp))
    return build


def _observe(c):
    e = c.env()
    c.out(e.obs, e.mask, e.player)
    c.call = lambda sp, s: _chk(c, c.M.L.sgx_observe(e._h, _p(e.obs), None, _p(e.mask), _p(e.player), 0, sp))


def _step(kind):
    def build(c):
        from stratego_env_amd import _lib
        M, L = c.M, c.M.L
        e = c.env(compact_outputs=(kind == 'compact'), n=3 if kind == 'sync_single' else None)
        want_kind = None
        if kind == 'lane':
            _chk(c, L.sgx_set_lane_kernel(e._h, 1))
            want_kind = _lib.LAUNCH_LANE
        if kind == 'pool':
            e.set_start_states(M.snap['A'])
            c.out(e.start_index)
        a = c.inp(M.act['A'][:e.num_envs].contiguous(), M.act['B'][:e.num_envs].contiguous())
        obs = kind != 'mask_only'
        sync = kind.startswith('sync')
        io = _io(e, a, want_next=not sync, obs=obs)
        _results(c, e, obs=obs, next_actions=not sync)

        def call(sp, s):
            _chk(c, (L.sgx_step_sync if sync else L.sgx_step)(e._h, C.byref(io), sp))
            if want_kind is not None:
                _kind(c, e, want_kind)
        c.call = call
    return build


def _step_n(want_kind_name):
    def build(c):
        from stratego_env_amd import _lib
        e = c.env()
        a = c.inp(c.M.act['A'], c.M.act['B'])
        io = _io(e, a, chained=True)
        _results(c, e)
        c.out(a)

        def call(sp, s):
            _chk(c, c.M.L.sgx_step_n(e._h, C.byref(io), N_STEPS, sp))
            _kind(c, e, getattr(_lib, want_kind_name))
        c.call = call
    return build


def _ring_sets(c, e, a, n_sets):
    """n_sets output sets that differ in their observation / mask tensors (all of them outputs of the case) -> the sgx_step_io array."""
    import torch
    from stratego_env_amd import _lib
    ios = (_lib.SgxStepIO * n_sets)()
    for k in range(n_sets):
        obs, mask = torch.empty_like(e.obs), torch.empty_like(e.mask)
        c.out(obs, mask)
        ios[k] = _io(e, a, chained=True)
        ios[k].obs_dev, ios[k].mask_dev = obs.data_ptr(), mask.data_ptr()
    return ios


def _ring(n_sets, mode='one'):
    """mode 'one': one call.  'alternate': ring R1 then ring R2 (both of n_sets sets) in one gated section, after an ungated call with R2:
    both gated calls CHANGE the ring, and the second one's upload comes while the first one's is still held behind the gate -- with one
    staging buffer guarded by a host wait that call blocked until the gate had drained (pending was false).  'same_ring_two_streams': ring
    R on the caller's stream, then R again on a second side stream ordered behind it by an event (the table was uploaded elsewhere).
    'two_rings_two_streams': R1 on the caller's stream, then R2 on the second stream behind an event: the upload of R2 must not overtake the
    launch that still reads R1's table.  Both rings are valid memory; before ring_tab_ev was recorded behind the READERS this last case was
    a race that could pass -- it is here to hold the fix, not because it failed."""
    def build(c):
        import torch
        from stratego_env_amd import _lib
        from tests import stream_gate as sg
        L = c.M.L
        e = c.env()
        a = c.inp(c.M.act['A'], c.M.act['B'])
        _results(c, e, obs=False, mask=False)
        c.out(a)
        r1 = _ring_sets(c, e, a, n_sets)
        r2 = _ring_sets(c, e, a, n_sets) if mode in ('alternate', 'two_rings_two_streams') else r1

        def ring(ios, first, sp):
            _chk(c, L.sgx_step_ring(e._h, ios, n_sets, first, N_STEPS, sp))
            _kind(c, e, _lib.LAUNCH_MULTI_STEP_WAVE)       # (one launch for all steps: with 9 sets the one that reads the device table)

        def behind(s):                                     # the second side stream waits for what `s` holds
            ev = torch.cuda.Event()
            ev.record(s)
            sg.gate().S2.wait_event(ev)
            return sg.stream_ptr(sg.gate().S2)
        if mode == 'one':
            c.call = lambda sp, s: ring(r1, 1, sp)
        elif mode == 'alternate':
            c.warm = lambda: ring(r2, 0, None)
            c.call = lambda sp, s: (ring(r1, 0, sp), ring(r2, N_STEPS % n_sets, sp))
        else:
            c.call = lambda sp, s: (ring(r1, 0, sp), ring(r2, N_STEPS % n_sets, behind(s)))
    return build


def _traj(n_slots, n_steps, multi_step=True):
    def build(c):
        import torch
        from stratego_env_amd import _lib
        M, L = c.M, c.M.L
        e = c.env()
        if not multi_step:
            _chk(c, L.sgx_set_multi_step(e._h, 0))
        a = c.inp(M.act['A'], M.act['B'])
        tr = e.alloc_trajectory(n_slots)
        t = _lib.SgxTrajIO()
        t.io = _io(e, a, chained=True)
        t.io.obs_dev, t.io.mask_dev, t.io.reward_dev, t.io.done_dev = (tr[k].data_ptr() for k in ('obs', 'mask', 'reward', 'done'))
        t.io.player_dev, t.io.invalid_action_dev, t.io.ending_invalid_dev = (tr[k].data_ptr() for k in ('player', 'invalid_action', 'ending_invalid'))
        t.n_slots, t.results_per_slot, t.slot_envs, t.actions_log_dev = n_slots, 1, M.n, tr['actions'].data_ptr()
        c.out(a, *(tr[k] for k in sorted(tr)))
        c.call = lambda sp, s: _chk(c, L.sgx_step_traj(e._h, C.byref(t), 1, n_steps, sp))
    return build


def _rollout(chains, then_export=False):
    """then_export: a consumer on the caller's stream right behind the chained call must see every chain's games (the join), as the chains
    must have seen B (the fork)."""
    def build(c):
        import torch
        L = c.M.L
        e = c.env()
        a = c.inp(c.M.act['A'], c.M.act['B'])
        io = _io(e, a, chained=True)
        _results(c, e)
        c.out(a)
        st = pl = None
        if then_export:
            st, pl = (c.out(torch.empty_like(t)) for t in c.M.state['A'])

        def call(sp, s):
            _chk(c, L.sgx_rollout(e._h, C.byref(io), N_STEPS, chains, sp))
            if then_export:
                _chk(c, L.sgx_export_state(e._h, _p(st), _p(pl), sp))
        c.call = call
    return build


def _sample_valid(c):
    import torch
    e = c.env()
    m = c.inp(c.M.mask['A'], c.M.mask['B'])
    out = c.new((c.M.n,), torch.int32)
    c.call = lambda sp, s: _chk(c, c.M.L.sgx_sample_valid(e._h, _p(m), _p(out), sp))


def _choose(c):
    import torch
    e = c.env()
    m = c.inp(c.M.mask['A'], c.M.mask['B'])
    g = torch.Generator(device='cuda').manual_seed(5)
    lg = c.inp(*(torch.randn((c.M.n, m[0].numel()), device='cuda', generator=g) for _ in 'AB'))
    out = c.new((c.M.n,), torch.int32)
    c.call = lambda sp, s: _chk(c, c.M.L.sgx_choose_actions(e._h, _p(lg), _p(m), C.c_float(1.0), 0, _p(out), sp))


def _decode(what):
    def build(c):
        import torch
        M, L = c.M, c.M.L
        from tests import stream_gate as sg
        e = c.handle(sg.new_env(M.name, M.n, compact_outputs=True), staged=False, compared=False)
        packed = {}
        for X in 'AB':
            e.restore(M.snap[X])
            packed[X] = (e.obs.clone(), e.mask.clone())
        torch.cuda.synchronize()
        if what == 'obs':
            src, out = c.inp(packed['A'][0], packed['B'][0]), c.out(torch.empty_like(M.obs['A']))
            c.call = lambda sp, s: _chk(c, L.sgx_decode_obs(e._h, _p(src), _p(out), sp))
        else:
            src, out = c.inp(packed['A'][1], packed['B'][1]), c.out(torch.empty_like(M.mask['A']))
            c.call = lambda sp, s: _chk(c, L.sgx_decode_mask(e._h, _p(src), _p(out), sp))
    return build


def _export(c):
    import torch
    e = c.env()
    st, pl = (c.out(torch.empty_like(t)) for t in c.M.state['A'])
    c.call = lambda sp, s: _chk(c, c.M.L.sgx_export_state(e._h, _p(st), _p(pl), sp))


def _import(checked):
    def build(c):
        import torch
        M, L = c.M, c.M.L
        e = c.env(staged=False)                            # the destination: holds A until the call
        st, pl = c.inp(M.state['A'][0], M.state['B'][0]), c.inp(M.state['A'][1], M.state['B'][1])
        if checked:
            san = c.new((M.n,), torch.uint8)
            c.call = lambda sp, s: _chk(c, L.sgx_import_state_checked(e._h, _p(st), _p(pl), _p(san), sp))
        else:
            c.call = lambda sp, s: _chk(c, L.sgx_import_state(e._h, _p(st), _p(pl), sp))
    return build


def _env_info(c):
    import torch
    e = c.env()
    out = c.new((c.M.n, 4), torch.int32)
    c.call = lambda sp, s: _chk(c, c.M.L.sgx_get_env_info(e._h, _p(out), sp))


def _step_states(chains=1, general=False):
    """general: every second state carries a third non-zero recent-move cell of player +1 (layer 6), which the packed record cannot hold:
    the import flags it and the second, general-state pass redoes it from the caller's int64 input."""
    def build(c):
        import torch
        M, L = c.M, c.M.L
        e = c.env(staged=False)
        _chk(c, L.sgx_set_general_states(e._h, 1))
        states = {X: M.state[X][0].clone() for X in 'AB'}
        if general:
            for st in states.values():
                st[1::2, 6, 0, :3] = 1
        st_in, pl_in = c.inp(states['A'], states['B']), c.inp(M.state['A'][1], M.state['B'][1])
        a = c.inp(M.act['A'], M.act['B'])
        io = _io(e, a, auto_reset=0)
        _results(c, e)
        st_out, pl_out, san = c.out(torch.empty_like(st_in)), c.out(torch.empty_like(pl_in)), c.new((M.n,), torch.uint8)
        c.call = lambda sp, s: _chk(c, L.sgx_step_states(e._h, _p(st_in), _p(pl_in), _p(san), C.byref(io), _p(st_out), _p(pl_out), chains, sp))
    return build


def _pools(c, dst_env=False):
    """(dst, src, the index list of the roots): src goes from A to B behind the gate, dst holds A until the call writes it."""
    from tests import stream_gate as sg
    src = c.pool(staged=True, compared=False)
    dst = c.env(staged=False) if dst_env else c.pool(staged=False)
    idx = {'A': sg.perm(c.M.n, 3, 1), 'B': sg.perm(c.M.n, 5, 2)}
    return dst, src, c.inp(idx['A'], idx['B']), idx


def _copy_envs(c):
    from tests import stream_gate as sg
    dst, src, si, _ = _pools(c)
    di = c.inp(sg.perm(c.M.n, 7, 0), sg.perm(c.M.n, 2, 3))
    c.call = lambda sp, s: _chk(c, c.M.L.sgx_copy_envs(dst._h, _p(di), src._h, _p(si), c.M.n, sp))


def _expand(c):
    M = c.M
    dst, src, si, idx = _pools(c, dst_env=True)
    a = c.inp(*(M.act[X][idx[X].long()].contiguous() for X in 'AB'))        # each root's own valid action
    io = _io(dst, a, auto_reset=0)
    _results(c, dst)
    c.call = lambda sp, s: _chk(c, M.L.sgx_expand(dst._h, src._h, _p(si), C.byref(io), sp))


def _determinize(weighted):
    def build(c):
        import torch
        M, L = c.M, c.M.L
        dst, src, si, _ = _pools(c)
        hidden = c.new((M.n,), torch.int32)
        if not weighted:
            c.call = lambda sp, s: _chk(c, L.sgx_determinize(dst._h, src._h, _p(si), 0, 7, _p(hidden), sp))
            return
        cells = M.env.R * M.env.Cc
        g = torch.Generator(device='cuda').manual_seed(11)
        belief = c.inp(*(torch.randint(0, 4096, (2, 12, cells), device='cuda', generator=g).to(torch.int16) for _ in 'AB'))   # written on S
        off = c.new((M.n,), torch.int32)
        c.call = lambda sp, s: _chk(c, L.sgx_determinize_weighted(dst._h, src._h, _p(si), 0, _p(belief), 0, 7, _p(hidden), _p(off), sp))
    return build


def _playout(weighted):
    def build(c):
        import torch
        from stratego_env_amd import _lib
        M, L = c.M, c.M.L
        dst, src, si, _ = _pools(c)
        n = M.n
        rew, done, einv, pl, ln = (c.new((n, 2), torch.float32), c.new((n,), torch.uint8), c.new((n,), torch.uint8), c.new((n,), torch.int8),
                                   c.new((n,), torch.int32))
        io = _lib.SgxPlayoutIO(rew.data_ptr(), done.data_ptr(), einv.data_ptr(), pl.data_ptr(), ln.data_ptr(), 30, 0)
        if not weighted:
            c.call = lambda sp, s: _chk(c, L.sgx_playout(dst._h, src._h, _p(si), C.byref(io), 9, sp))
            return
        w = np.ascontiguousarray(np.random.RandomState(3).randint(1, 4096, size=_lib.PLAYOUT_WEIGHTS_SHAPE), dtype=np.uint16)   # (host memory)
        c.keep.append(w)
        c.call = lambda sp, s: _chk(c, L.sgx_playout_weighted(dst._h, src._h, _p(si), C.byref(io), w.ctypes.data_as(C.POINTER(C.c_uint16)), 0, 9, sp))
    return build


CELLS = 100                                                # of the 10x10 boards the tracked replay's case runs on


def _labels(n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (n, 2, CELLS), generator=g, dtype=torch.int16).cuda()


def _replay(tracked):
    """tracked: with sgx_set_replay_origins on -- the setter takes no stream and launches nothing, the label work goes to the call's stream
    like the rest"""
    def build(c):
        import torch
        from stratego_env_amd import _lib
        M, L, n, LEN = c.M, c.M.L, c.M.n, 4
        dst, src, si, idx = _pools(c)
        lists = {}
        for X in 'AB':
            first = M.act[X][idx[X].long()]                # each root's own valid action, then entries that are mostly invalid (skipped)
            lists[X] = torch.stack([first] + [first.roll(k) for k in range(1, LEN)], 1).contiguous()
        acts = c.inp(lists['A'], lists['B'])               # written on S
        if tracked:
            origin_in = c.inp(_labels(n, 1), _labels(n, 2))    # a staged input: written on S behind the gate
            origin_out = c.new((n, 2, CELLS), torch.int16)     # a compared output
        ap, co, stop = c.new((n,), torch.int32), c.new((n,), torch.int32), c.new((n,), torch.uint8)
        rew, done, einv, pl = c.new((n, 2), torch.float32), c.new((n,), torch.uint8), c.new((n,), torch.uint8), c.new((n,), torch.int8)
        io = _lib.SgxReplayIO(acts.data_ptr(), None, ap.data_ptr(), co.data_ptr(), stop.data_ptr(), rew.data_ptr(), done.data_ptr(), einv.data_ptr(),
                              pl.data_ptr(), LEN, 1, n * LEN, LEN, _lib.REPLAY_SKIP_INVALID)
        if tracked:
            _chk(c, L.sgx_set_replay_origins(dst._h, _p(origin_in), _p(origin_out)))      # (the setting: no stream, no launch)

        def call(sp, s):
            _chk(c, L.sgx_replay(dst._h, src._h, _p(si), C.byref(io), sp))
            if tracked:
                _kind(c, dst, _lib.LAUNCH_REPLAY_TRACKED)
        c.call = call
    return build


N_ROOTS = 2 * 256 + 1                                      # three blocks of the offsets scan (SCAN_BLOCK = 256), the last with one root


def _count_moves(own_counts):
    def build(c):
        import torch
        M, L = c.M, c.M.L
        src = c.pool(staged=True, compared=False)
        i = torch.arange(N_ROOTS, device='cuda')
        si = c.inp(((i * 3 + 1) % M.n).to(torch.int32), ((i * 5 + 2) % M.n).to(torch.int32))
        counts = c.new((N_ROOTS,), torch.int32) if own_counts else None
        offsets = c.new((N_ROOTS + 1,), torch.int64)
        c.call = lambda sp, s: _chk(c, L.sgx_count_moves(src._h, _p(si), N_ROOTS, _p(counts), _p(offsets), sp))
    return build


def _expand_all(c):
    import torch
    from stratego_env_amd import _lib
    M, L, n = c.M, c.M.L, c.M.n
    dst, src, si, idx = _pools(c)
    offs = c.inp(*(M.snap[X].count_moves(idx[X])[1] for X in 'AB'))          # what sgx_count_moves says of each state's roots
    torch.cuda.synchronize()
    par, act = c.new((n,), torch.int32), c.new((n,), torch.int32)
    rew, done, einv, pl = c.new((n, 2), torch.float32), c.new((n,), torch.uint8), c.new((n,), torch.uint8), c.new((n,), torch.int8)
    io = _lib.SgxChildrenIO(offs.data_ptr(), par.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(), einv.data_ptr(), pl.data_ptr(),
                            n, 0, n, 0, 0)
    c.call = lambda sp, s: _chk(c, L.sgx_expand_all(dst._h, src._h, _p(si), C.byref(io), sp))


def _state_keys(wide):
    def build(c):
        import torch
        from stratego_env_amd import _lib
        M, L, n = c.M, c.M.L, c.M.n
        _, src, si, _ = _pools(c)
        keys = c.new((n, 2) if wide else (n,), torch.int64)
        view, flags = (0, _lib.KEYS_WIDE) if wide else (_lib.KEYS_VIEW_STATE, 0)
        c.call = lambda sp, s: _chk(c, L.sgx_state_keys(src._h, _p(si), n, view, flags, _p(keys), sp))
    return build


def _step_vs(c):
    """dst holds A until the call writes it; src, the index list, the agent's actions and sides go from A to B behind the gate (in A the
    agent is each root's mover: its move, then the reply; in B it is the other side: the bot alone)"""
    import torch
    from stratego_env_amd import _lib
    M, L, n = c.M, c.M.L, c.M.n
    dst, src, si, idx = _pools(c)
    actions = c.inp(*(M.act[X][idx[X].long()] for X in 'AB'))            # each root's own valid action (written on S)
    agent = c.inp(*(torch.where(M.player[X][idx[X].long()] * s > 0, 1, -1).to(torch.int8) for X, s in (('A', 1), ('B', -1))))
    outs = [c.new((n, w) if w > 1 else (n,), getattr(torch, t)) for _, w, t in STEP_VS_OUT_SPECS]
    io = _lib.SgxVsIO(actions.data_ptr(), agent.data_ptr(), *[t.data_ptr() for t in outs], 0, 0)
    w = np.ascontiguousarray(np.random.RandomState(3).randint(1, 4096, size=_lib.PLAYOUT_WEIGHTS_SHAPE), dtype=np.uint16)   # (host memory)
    c.keep.append(w)
    c.call = lambda sp, s: _chk(c, L.sgx_step_vs(dst._h, src._h, _p(si), C.byref(io), w.ctypes.data_as(C.POINTER(C.c_uint16)), 9, sp))


LEAF_LIMIT, LEAF_DENOM = (1 << 24) - 5, (1 << 24) - 3      # no sum of piece values reaches the limit: the sums themselves come out


def _playout_leaf_values(c):
    """sgx_playout with leaf values set on dst (a random int16 table with distinct entries): all its work on the caller's stream, no wait"""
    _playout(False)(c)
    dst = c.handles[1][0]                                                      # (_pools: src first, then dst)
    L = c.M.L
    T = (np.random.RandomState(7).permutation(65536)[:2 * 14 * CELLS] - 32768).astype(np.int16).reshape(2, 14, CELLS)
    assert L.sgx_set_leaf_values(dst._h, T.ctypes.data_as(C.c_void_p), LEAF_LIMIT, LEAF_DENOM, 0) == 0, L.sgx_last_error()
    assert L.sgx_leaf_values_set(dst._h) == 1, "the table is not set on dst"


def _cut_off_playouts_carry_values(c):
    reward, done = c.outputs[0], c.outputs[1]
    open_ = done == 0
    assert bool(open_.any()) and bool((reward[open_] != 0).any()), "cut-off playouts carry values"


def _case(id, entries, variant, n, build, may_wait=False, after=None):
    return Spec(id, tuple(entries.split()), variant, n, build, may_wait, after)


CASES = [
    # stepping calls
    _case('reset-all', 'sgx_reset', 'barrage', N_BARRAGE, _reset('all')),
    _case('reset-selection-with-maps', 'sgx_reset', 'barrage', N_BARRAGE, _reset('maps')),
    _case('reset-start-pool', 'sgx_reset', 'barrage', N_BARRAGE, _reset('pool')),
    _case('observe', 'sgx_observe', 'barrage', N_BARRAGE, _observe),
    _case('step-wave', 'sgx_step', 'barrage', N_BARRAGE, _step('wave')),
    _case('step-two-per-wave', 'sgx_step', 'fives', N_FIVES, _step('wave')),
    _case('step-lane', 'sgx_step', 'micro', N_MICRO, _step('lane')),
    _case('step-start-pool', 'sgx_step', 'barrage', N_BARRAGE, _step('pool')),
    _case('step-compact', 'sgx_step', 'barrage', N_BARRAGE, _step('compact')),
    _case('step-mask-only', 'sgx_step', 'barrage', N_BARRAGE, _step('mask_only')),
    _case('step-sync', 'sgx_step_sync', 'barrage', N_BARRAGE, _step('sync'), may_wait=True),
    _case('step-sync-single-kernel', 'sgx_step_sync', 'barrage', N_BARRAGE, _step('sync_single'), may_wait=True),
    # multi-step calls
    _case('step-n-wave', 'sgx_step_n', 'barrage', N_BARRAGE, _step_n('LAUNCH_MULTI_STEP_WAVE')),
    _case('step-n-lane', 'sgx_step_n', 'micro', N_MICRO, _step_n('LAUNCH_MULTI_STEP')),
    _case('ring-3-sets', 'sgx_step_ring', 'barrage', N_BARRAGE, _ring(3)),
    _case('ring-9-sets-table', 'sgx_step_ring', 'barrage', N_BARRAGE, _ring(9)),
    _case('ring-9-sets-alternating', 'sgx_step_ring', 'barrage', N_BARRAGE, _ring(9, 'alternate')),
    _case('ring-9-sets-same-ring-two-streams', 'sgx_step_ring', 'barrage', N_BARRAGE, _ring(9, 'same_ring_two_streams')),
    _case('ring-9-sets-two-rings-two-streams', 'sgx_step_ring', 'barrage', N_BARRAGE, _ring(9, 'two_rings_two_streams')),
    _case('traj-action-log-odd-step', 'sgx_step_traj', 'barrage', N_BARRAGE, _traj(4, SGX_STEPS_MAX_PER_LAUNCH + 1)),
    _case('traj-action-log-step-by-step', 'sgx_step_traj', 'barrage', N_BARRAGE, _traj(N_STEPS, N_STEPS, multi_step=False)),
    _case('rollout-1-chain', 'sgx_rollout', 'barrage', N_BARRAGE, _rollout(1)),
    _case('rollout-2-chains-then-export', 'sgx_rollout sgx_export_state', 'barrage', N_CHAINS, _rollout(2, then_export=True)),
    # samplers, decoders, state calls
    _case('sample-valid', 'sgx_sample_valid', 'barrage', N_BARRAGE, _sample_valid),
    _case('choose-actions-wave', 'sgx_choose_actions', 'barrage', N_BARRAGE, _choose),
    _case('choose-actions-four-per-wave', 'sgx_choose_actions', 'micro', N_MICRO, _choose),
    _case('decode-obs', 'sgx_decode_obs', 'barrage', N_BARRAGE, _decode('obs')),
    _case('decode-mask', 'sgx_decode_mask', 'barrage', N_BARRAGE, _decode('mask')),
    _case('export-state', 'sgx_export_state', 'barrage', N_BARRAGE, _export),
    _case('import-state', 'sgx_import_state', 'barrage', N_BARRAGE, _import(False)),
    _case('import-state-checked', 'sgx_import_state_checked', 'fives', N_FIVES, _import(True)),
    _case('env-info', 'sgx_get_env_info', 'barrage', N_BARRAGE, _env_info),
    # sgx_step_states
    _case('step-states-fused', 'sgx_step_states', 'barrage', N_BARRAGE, _step_states()),
    _case('step-states-three-launches', 'sgx_step_states', 'fives', N_FIVES, _step_states()),
    _case('step-states-general-second-pass', 'sgx_step_states', 'barrage', N_BARRAGE, _step_states(general=True)),
    _case('step-states-three-launches-second-pass', 'sgx_step_states', 'fives', N_FIVES, _step_states(general=True)),
    _case('step-states-2-chains', 'sgx_step_states', 'fives', N_CHAINS, _step_states(chains=2)),
    # pool to pool, index lists written on S
    _case('copy-envs', 'sgx_copy_envs', 'barrage', N_BARRAGE, _copy_envs),
    _case('expand', 'sgx_expand', 'barrage', N_BARRAGE, _expand),
    _case('determinize', 'sgx_determinize', 'barrage', N_BARRAGE, _determinize(False)),
    _case('determinize-weighted', 'sgx_determinize_weighted', 'barrage', N_BARRAGE, _determinize(True)),
    _case('playout', 'sgx_playout', 'barrage', N_BARRAGE, _playout(False)),
    _case('playout-weighted', 'sgx_playout_weighted', 'barrage', N_BARRAGE, _playout(True)),
    _case('playout-leaf-values', 'sgx_playout', 'barrage', N_BARRAGE, _playout_leaf_values, after=_cut_off_playouts_carry_values),
    _case('replay', 'sgx_replay', 'barrage', N_BARRAGE, _replay(False)),
    _case('replay-tracked', 'sgx_replay', 'barrage', N_BARRAGE, _replay(True)),
    _case('count-moves', 'sgx_count_moves', 'barrage', N_BARRAGE, _count_moves(True)),
    _case('count-moves-scratch-counts', 'sgx_count_moves', 'barrage', N_BARRAGE, _count_moves(False)),
    _case('expand-all', 'sgx_expand_all', 'barrage', N_BARRAGE, _expand_all),
    _case('state-keys', 'sgx_state_keys', 'barrage', N_BARRAGE, _state_keys(False)),
    _case('state-keys-wide', 'sgx_state_keys', 'barrage', N_BARRAGE, _state_keys(True)),
    _case('step-vs', 'sgx_step_vs', 'barrage', N_BARRAGE, _step_vs),
]
