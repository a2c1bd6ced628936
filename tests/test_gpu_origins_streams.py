"""The tracked replay (sgx_set_replay_origins + sgx_replay) under the header's stream contract: the label work goes to the
call's stream like the rest and the call does not wait.  One case of the gate harness (tests/stream_gate.py), built like the `replay` row of
tests/test_gpu_streams.py -- the setter takes no stream and launches nothing, so the call under test is sgx_replay with the setting on --
and one data-only check of the Python wrapper."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

N_BARRAGE = 17                                     # one workgroup's games plus 1, as tests/test_gpu_streams.py takes it
CELLS = 100


def _labels(n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (n, 2, CELLS), generator=g, dtype=torch.int16).cuda()


def _replay_tracked(c):
    import torch
    from stratego_env_amd import _lib
    from tests.test_gpu_streams import _chk, _p, _pools
    M, L, n, LEN = c.M, c.M.L, c.M.n, 4
    dst, src, si, idx = _pools(c)
    lists = {}
    for X in 'AB':
        first = M.act[X][idx[X].long()]                    # each root's own valid action, then entries that are mostly invalid (skipped)
        lists[X] = torch.stack([first] + [first.roll(k) for k in range(1, LEN)], 1).contiguous()
    acts = c.inp(lists['A'], lists['B'])                   # written on S
    origin_in = c.inp(_labels(n, 1), _labels(n, 2))        # a staged input: written on S behind the gate
    origin_out = c.new((n, 2, CELLS), torch.int16)         # a compared output
    ap, co, stop = c.new((n,), torch.int32), c.new((n,), torch.int32), c.new((n,), torch.uint8)
    rew, done, einv, pl = c.new((n, 2), torch.float32), c.new((n,), torch.uint8), c.new((n,), torch.uint8), c.new((n,), torch.int8)
    io = _lib.SgxReplayIO(acts.data_ptr(), None, ap.data_ptr(), co.data_ptr(), stop.data_ptr(), rew.data_ptr(), done.data_ptr(), einv.data_ptr(),
                          pl.data_ptr(), LEN, 1, n * LEN, LEN, _lib.REPLAY_SKIP_INVALID)
    _chk(c, L.sgx_set_replay_origins(dst._h, _p(origin_in), _p(origin_out)))      # (the setting: no stream, no launch)

    def call(sp, s):
        _chk(c, L.sgx_replay(dst._h, src._h, _p(si), C.byref(io), sp))
        assert L.sgx_last_launch_kind(dst._h) == _lib.LAUNCH_REPLAY_TRACKED
    c.call = call


def test_tracked_replay_runs_on_its_stream_and_does_not_wait():
    """Twin, gated run and NULL-stream control (run_case asserts that the control mismatches); not may_wait."""
    import torch
    from tests import stream_gate as sg
    torch.cuda.set_device(0)
    case = sg.Case(sg.material('barrage', N_BARRAGE))
    _replay_tracked(case)
    sg.run_case(case, may_wait=False, label='replay-tracked')


def test_the_python_wrapper_passes_the_current_stream():
    """PackedStates.replay(track_origins=True) inside `with torch.cuda.stream(S)` behind the gate: data only.  A wrapper that passed another
    stream than the current one would compute from state A."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from tests import stream_gate as sg
    name, n = 'barrage', N_BARRAGE
    M, G = sg.material(name, n), sg.gate()
    env = sg.new_env(name, n)
    dst = PackedStates(name, n, seed=sg.SEED, env_id_offset=sg.OFFSET)
    acts = {X: torch.stack([M.act[X], M.act[X].roll(1), M.act[X].roll(2)], 1).contiguous() for X in 'AB'}
    labels = {'A': _labels(n, 1), 'B': _labels(n, 2)}
    acts_live, labels_live = acts['A'].clone(), labels['A'].clone()

    def run():
        env.restore(M.snap['B'])
        acts_live.copy_(acts['B'])
        labels_live.copy_(labels['B'])
        rp = dst.replay(env, acts_live, skip_invalid=True, origins_in=labels_live)
        return [sg._bytes(t).clone() for t in (rp.origins, rp.applied, rp.consumed, rp.stop, rp.reward, rp.done, rp.player, *dst.unpack())]

    want = run()                                           # the default stream (also the warm-up of every allocation)
    torch.cuda.synchronize()
    env.restore(M.snap['A'])
    acts_live.copy_(acts['A'])
    labels_live.copy_(labels['A'])
    dst.copy_from(M.snap['A'])
    torch.cuda.synchronize()
    G.run(G.S)
    with torch.cuda.stream(G.S):
        got = run()
    G.S.synchronize()
    torch.cuda.synchronize()
    bad = sg.mismatches(got, want)
    assert not bad, "results %s differ from the default-stream run: the wrapper did not pass the current stream" % bad
    assert not dst._vec._L.sgx_replay_origins_set(dst._vec._h)
    env.close(); dst.close()
