"""sgx_replay against the way the same positions were reached before it existed, on the same start records and the same recorded actions.

Workload: 65,536 Barrage games from reset() (setups from the variant's table), T = 200 recorded actions per game (random valid moves; a game that ends earlier stops there).
  replay dense   one sgx_replay launch, pool to pool, actions as a dense game-major [N, T] tensor (step_stride 1: a chunk is one line)
  replay [T][N]  the same launch on the transposed view of the [T, N] log (the layout of a trajectory's action log: one entry per line)
  per step       the parent commit's way: sgx_copy_envs of the start records into a live handle, then T launches of
                 env.step(actions[t], emit_obs=False, emit_mask=False)
  rollout_steps  for scale: rollout_steps(T, emit_obs=False, emit_mask=False) on the same start records, which draws its own actions --
                 the floor of an in-LDS loop with a mask and a draw per move (the copy and the first draw are not timed)
The four run interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up of one each; every repetition, min and
median are printed.  The tool checks that both replays and the per-step run leave the same records.
    python tools/replay_bench.py [variant] [--games N] [--steps T]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, REPEATS = 65536, 200, 5


def main():
    import torch
    from stratego_env_amd import _lib, build as hip_build
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tools.kernel_notes import kernel_notes
    args = sys.argv[1:]
    name = next((a for a in args if not a.startswith('--') and not a.isdigit()), 'barrage')
    n = int(args[args.index('--games') + 1]) if '--games' in args else N
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else T

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)                                            # ms

    env = VecStrategoEnv(name, n, seed=9, auto_reset=False, placement='plain')
    env.reset()
    start, dst = PackedStates(name, n), PackedStates(name, n)
    start.copy_from(env)
    L = env._L
    log = torch.empty((steps, n), dtype=torch.int32, device=env.device)      # [T][N]
    for t in range(steps):
        over = env.env_info()[:, 2] != 0
        drawn = env.sample_valid_actions()
        log[t] = torch.where(over, torch.full_like(drawn, -1), drawn)       # (a finished game: an entry no replay reads)
        env.step(log[t], emit_obs=False)
    want = env.export_state()[0]
    played = env.env_info()[:, 0].float()
    dense = log.T.contiguous()                                               # [N][T]
    out = {}

    def replay_dense():
        out['dense'] = dst.replay(start, dense)

    def replay_tn():
        out['tn'] = dst.replay(start, log.T)

    def per_step():
        _lib.check(L.sgx_copy_envs(env._h, None, start._vec._h, None, n, env._stream()), L)
        for t in range(steps):
            env.step(log[t], emit_obs=False, emit_mask=False)

    def prepare_rollout():
        _lib.check(L.sgx_copy_envs(env._h, None, start._vec._h, None, n, env._stream()), L)
        env.observe(emit_obs=False)
        env.sample_valid_actions()

    def rollout():
        env.rollout_steps(steps, emit_obs=False, emit_mask=False)

    # warm-up, and all three ways reach the same records
    replay_dense()
    assert torch.equal(dst.unpack()[0], want), "replay (dense) == the recorded run"
    replay_tn()
    assert torch.equal(dst.unpack()[0], want), "replay ([T][N]) == the recorded run"
    per_step()
    assert torch.equal(env.export_state()[0], want), "per-step replay == the recorded run"
    prepare_rollout(); rollout()
    res = out['dense']
    assert torch.equal(res.applied.float(), played) and not bool((res.stop == 2).any())
    kinds = (('replay dense', replay_dense), ('replay [T][N]', replay_tn), ('per step', per_step), ('rollout_steps', rollout))
    ts = {k: [] for k, _ in kinds}
    for _ in range(REPEATS):
        for k, fn in kinds:
            if fn is rollout:
                prepare_rollout()
            ts[k].append(timed(fn))
    moves = float(played.sum())
    print("%s, %d games, %d recorded actions per game; moves applied per replay: %.0f (mean %.1f per game, %d games ended early)"
          % (name, n, steps, moves, moves / n, int((res.stop == 1).sum())), flush=True)
    for k, _ in kinds:
        t = sorted(ts[k])
        print("%-14s %s ms (min %.3f, median %.3f; %.2f G moves/s by the median)" % (k, " / ".join("%.3f" % x for x in ts[k]), t[0], t[len(t) // 2],
                                                                                 (n * steps if k == 'rollout_steps' else moves) / t[len(t) // 2] / 1e6), flush=True)
    med = lambda k: sorted(ts[k])[REPEATS // 2]
    print("per step / replay dense: %.2fx; per step / replay [T][N]: %.2fx; replay dense / rollout_steps: %.2fx (medians)"
          % (med('per step') / med('replay dense'), med('per step') / med('replay [T][N]'), med('replay dense') / med('rollout_steps')), flush=True)
    for x in (start, dst, env):
        x.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'replay_kernel' in kname:
            print("%-70s vgpr %3d sgpr %3d scratch %4d lds %6d" % (kname[:70], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
