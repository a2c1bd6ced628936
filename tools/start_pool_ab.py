"""A rollout whose games start from a start pool (VecStrategoEnv.set_curriculum: every auto-reset loads a record of the table) against the
same rollout with sampled setups: 65,536 Barrage games, launches of 256 steps (steps_kernel_pool / steps_kernel), HIP-event time after a
warm-up launch, three repeats each, interleaved.  A start happens about once per game, so the two should be within noise of each other.
Then the same with ONE launch per step (set_multi_step(False): steps_kernel_pool with n_steps = 1 against step_kernel) -- what env.step()
pays per step while a pool is set.
    python tools/start_pool_ab.py [curriculum file] [games] [variant]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from stratego_env_amd import _lib  # noqa: E402
from stratego_env_amd.vec_env import VecStrategoEnv  # noqa: E402

STEPS, REPEATS = 256, 3


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / STEPS


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'curriculum_barrage.npz')
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    name = sys.argv[3] if len(sys.argv) > 3 else 'barrage'
    envs = {}
    for what in ('sampled setups', 'start pool'):
        e = VecStrategoEnv(name, n, seed=9, auto_reset=True)
        if what == 'start pool':
            e.set_curriculum(path)
        e.reset()
        e.rollout_steps(STEPS)                                   # warm-up launch (also: games are in their middle)
        assert e.last_launch_kind == _lib.LAUNCH_MULTI_STEP_WAVE
        envs[what] = e
    ts = {k: [] for k in envs}
    ended = {k: 0 for k in envs}
    for _ in range(REPEATS):
        for k, e in envs.items():
            g0 = int(e.env_info()[:, 1].sum())
            ts[k].append(timed(lambda: e.rollout_steps(STEPS)))
            ended[k] += int(e.env_info()[:, 1].sum()) - g0
    per_step = {k: [] for k in envs}
    for e in envs.values():
        e.set_multi_step(False)
        e.rollout_steps(8)
    for _ in range(REPEATS):
        for k, e in envs.items():
            per_step[k].append(timed(lambda: e.rollout_steps(STEPS)))
    for k in envs:
        print("%-15s one launch per step: %s us per step (median %.1f)" % (k, " / ".join("%.1f" % t for t in per_step[k]), sorted(per_step[k])[1]), flush=True)
    for k, e in envs.items():
        print("%-15s %d %s games, launches of %d steps: %s us per step (median %.1f), %.1f M env steps/s; %d games started in the timed launches; invalid actions: %d"
              % (k, n, name, STEPS, " / ".join("%.1f" % t for t in ts[k]), sorted(ts[k])[1], n / sorted(ts[k])[1], ended[k], int(e.invalid_action.sum())), flush=True)
        e.close()


if __name__ == '__main__':
    main()
