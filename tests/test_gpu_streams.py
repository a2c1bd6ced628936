"""The header's stream contract, entry point by entry point (include/stratego_mi355x.h: "all device work is enqueued on `stream` ... and
is asynchronous; the entry points that wait for the device are ...").  tests/stream_gate.py has the construction: behind a gate on a
non-blocking side stream the inputs of a call are replaced (A -> B) and the call is issued; whatever part of it left the stream computes
from A and differs, byte for byte, from the twin run on the default stream.  Every case runs three times: twin, gated (data, `pending`,
host time below a quarter of the gate), and the control on the NULL stream, which must be REPORTED as a mismatch.

tests/stream_cases.py has the builders and CASES, the one table: every row of it runs here.  tests/test_streams_cpu.py holds the table
against the header: every prototype with a `void *stream` parameter is a row or an exclusion there, and the header's list of waiting entry
points is the set marked may_wait.

Measured on an MI355X (gate: 58.8 ms in 164 additions over 1 GiB; host time of the gated call in microseconds, one run):
  reset-all 7.6; reset-selection-with-maps 6.3; reset-start-pool 6.8; observe 6.0; step-wave 5.2; step-two-per-wave 5.2
  step-lane 5.2; step-start-pool 4.7; step-compact 4.9; step-mask-only 4.9; step-sync 58183 (waits)
  step-sync-single-kernel 58247 (waits); step-n-wave 6.2; step-n-lane 5.5; ring-3-sets 6.7; ring-9-sets-table 9.9
  ring-9-sets-alternating 43.6; ring-9-sets-same-ring-two-streams 23.6; ring-9-sets-two-rings-two-streams 30.5
  traj-action-log-odd-step 10.2; traj-action-log-step-by-step 99.5; rollout-1-chain 6.2; rollout-2-chains-then-export 108
  sample-valid 4.9; choose-actions-wave 6.7; choose-actions-four-per-wave 5.7; decode-obs 5.4; decode-mask 5.3; export-state 5.0
  import-state 5.4; import-state-checked 5.2; env-info 4.7; step-states-fused 12.7; step-states-three-launches 18.0
  step-states-general-second-pass 12.1; step-states-three-launches-second-pass 17.3; step-states-2-chains 40.9; copy-envs 6.2
  expand 5.4; determinize 6.4; determinize-weighted 6.8; playout 5.1; playout-weighted 15.7; replay 5.9; count-moves 12.4
  count-moves-scratch-counts 11.4; expand-all 5.5; state-keys 5.6; state-keys-wide 5.1
Every row but the two of sgx_step_sync returned with the gate pending; its NULL-stream control was reported as a mismatch in every row.
"""
import pytest

from tests.stream_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case_id', [c.id for c in CASES])
def test_call_runs_on_its_stream_and_does_not_wait(case_id):
    """Twin, gated run and NULL-stream control of one row of the table (tests/stream_gate.py: run_case), then the row's own closing check
    where it has one.  After every call the HIP runtime's current device is what it was."""
    import torch
    from tests import stream_gate as sg
    spec = {c.id: c for c in CASES}[case_id]
    torch.cuda.set_device(0)
    case = sg.Case(sg.material(spec.variant, spec.n))
    spec.build(case)
    sg.run_case(case, may_wait=spec.may_wait, label=case_id)
    if spec.after is not None:
        spec.after(case)


def test_the_side_stream_is_non_blocking_and_the_gate_is_long_enough():
    """The premises: S does not synchronise with the NULL stream, and the gate lasts 20 .. 200 ms (the floor is about 50 times the enqueue
    cost of the longest call here, some 40 launches)."""
    from tests import stream_gate as sg
    G = sg.gate()
    assert sg.is_non_blocking(G.S) and sg.is_non_blocking(G.S2)
    assert sg.GATE_MIN_MS <= G.ms <= sg.GATE_MAX_MS
    print("STREAMS gate %.1f ms in %d launches" % (G.ms, G.reps))


def test_python_wrappers_pass_the_current_stream():
    """VecStrategoEnv.rollout_steps / rollout_trajectory / replay / count_moves / state_keys and PackedStates.determinize / playout /
    expand_all / valid_moves_as_1d_mask (its sgx_observe) inside `with torch.cuda.stream(S)` behind the gate: data only.  A wrapper that
    passed another stream than the current one would compute from state A."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from tests import stream_gate as sg
    name, n = 'barrage', 17
    M, G = sg.material(name, n), sg.gate()
    env = sg.new_env(name, n)
    dst = PackedStates(name, n, seed=sg.SEED, env_id_offset=sg.OFFSET)
    traj = env.alloc_trajectory(4)
    acts = {X: torch.stack([M.act[X], M.act[X].roll(1), M.act[X].roll(2)], 1).contiguous() for X in 'AB'}
    acts_live = acts['A'].clone()
    idx = sg.perm(n, 3, 1)

    def flat(*ts):
        return [sg._bytes(t).clone() for t in ts]

    def everything():
        out = []
        env.restore(M.snap['B'])
        acts_live.copy_(acts['B'])
        c, o = env.count_moves(idx)
        out += flat(c, o, env.state_keys(idx, observer=0, wide=True))
        out += flat(dst.determinize(env, draw=3), *dst.unpack())
        r = dst.playout(env, max_steps=30, draw=5)
        out += flat(r.reward, r.done, r.ending_invalid, r.player, r.length, *dst.unpack())
        ch = dst.expand_all(env, src_index=idx)
        out += flat(ch.parent, ch.action, ch.reward, ch.done, ch.ending_invalid, ch.player, ch.offsets, *dst.unpack())
        out += flat(dst.valid_moves_as_1d_mask())
        rp = dst.replay(env, acts_live, skip_invalid=True)
        out += flat(rp.applied, rp.consumed, rp.stop, rp.reward, rp.done, rp.player, *dst.unpack())
        env.rollout_steps(20)
        out += flat(env.obs, env.mask, env.reward, env.done, env.player, env.next_actions)
        env.rollout_trajectory(7, traj)
        out += flat(*(traj[k] for k in sorted(traj)), *env.export_state())
        return out

    want = everything()                                    # the default stream (also the warm-up of every allocation)
    torch.cuda.synchronize()
    env.restore(M.snap['A'])
    acts_live.copy_(acts['A'])
    dst.copy_from(M.snap['A'])
    for t in traj.values():
        sg._bytes(t).fill_(sg.POISON)
    torch.cuda.synchronize()
    G.run(G.S)
    with torch.cuda.stream(G.S):
        got = everything()
    G.S.synchronize()
    torch.cuda.synchronize()
    bad = sg.mismatches(got, want)
    assert not bad, "results %s differ from the default-stream run: a wrapper did not pass the current stream" % bad
    env.close(); dst.close()
