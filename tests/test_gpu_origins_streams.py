"""The tracked replay (sgx_set_replay_origins + sgx_replay) under the header's stream contract: the label work goes to the
call's stream like the rest and the call does not wait.  The case of the gate harness is the row `replay-tracked` of the one table
(tests/stream_cases.py, run by tests/test_gpu_streams.py); here is the data-only check of the Python wrapper."""
import pytest

from tests.stream_cases import N_BARRAGE, _labels

pytestmark = pytest.mark.gpu


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
