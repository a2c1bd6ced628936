"""Leaf values fused into the launch that makes the position, against the two-pass way they replace, on the same roots.

Workload: 65,536 roots of the variant, 100 rollout steps after reset() (setups from the variant's table, no auto-reset).
  expand_all   one window of CAPACITY children:
               fused     sgx_expand_all into a pool with a table set
               two-pass  sgx_expand_all into the pool with the table cleared, then evaluate() in place with the table set
                         (the setter waits for the device, so the two halves are timed apart and added)
  playout      max_steps 16 / 32 / 64, one playout per root:
               fused     sgx_playout into a pool with a table set
               two-pass  sgx_playout with the table cleared, then evaluate() in place
               to the end   sgx_playout with max_steps 0: what PIMC pays without leaf values
The runs are interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up of one each; median and range are
printed, then the ratios by the medians.  The tool checks that fused and two-pass report the same rewards.
    python tools/leaf_values_bench.py [variant] [--games N] [--steps T] [--capacity C]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, CAPACITY, REPEATS = 65536, 100, 262144, 7
CAPS = (16, 32, 64)


def main():
    import torch
    from stratego_env_amd import leaf_values
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    args = sys.argv[1:]
    name = next((a for a in args if not a.startswith('--') and not a.isdigit()), 'barrage')
    n = int(args[args.index('--games') + 1]) if '--games' in args else N
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else T
    cap = int(args[args.index('--capacity') + 1]) if '--capacity' in args else CAPACITY

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out                                       # ms

    env = VecStrategoEnv(name, n, seed=9, auto_reset=False, placement='plain')
    env.reset()
    env.rollout_steps(steps, emit_obs=False, emit_mask=False)
    roots = PackedStates(name, n)
    roots.copy_from(env)
    env.close()
    v = roots._vec.variant
    table = leaf_values.with_advance(leaf_values.material(v), 1, rows=v.rows)
    denom = 2 * leaf_values.side_total(v)
    setting = (table, denom - 1, denom)
    _, offsets = roots.count_moves()
    total = int(offsets[-1])
    m = min(cap, total)
    kids_fused, kids_plain = PackedStates(name, m), PackedStates(name, m)
    play_fused, play_plain = PackedStates(name, n, seed=3), PackedStates(name, n, seed=3)
    for p in (kids_fused, play_fused):
        p.set_leaf_values(*setting, see_all=True)

    def two_pass(pool, call):
        """-> (ms of the call without a table, ms of evaluate() in place, the rewards)"""
        pool.clear_leaf_values()
        t0, _ = timed(call)
        pool.set_leaf_values(*setting, see_all=True)
        t1, reward = timed(pool.evaluate)
        return t0, t1, reward

    runs = [('expand_all', lambda: kids_fused.expand_all(roots, offsets=offsets, first_child=0).reward, kids_plain,
             lambda: kids_plain.expand_all(roots, offsets=offsets, first_child=0), m)]
    for c in CAPS:
        runs.append(('playout max_steps %d' % c, (lambda c=c: play_fused.playout(roots, max_steps=c, draw=1).reward), play_plain,
                     (lambda c=c: play_plain.playout(roots, max_steps=c, draw=1)), n))
    to_the_end = lambda: play_plain.playout(roots, max_steps=0, draw=1)
    # warm-up, and the two ways report the same rewards
    for what, fused, pool, plain, _ in runs:
        a = fused()
        _, _, b = two_pass(pool, plain)
        assert torch.equal(a, b), "%s: fused and two-pass rewards differ" % what
    play_plain.clear_leaf_values()
    to_the_end()
    ts = {}
    for _ in range(REPEATS):
        for what, fused, pool, plain, _ in runs:
            ts.setdefault((what, 'fused'), []).append(timed(fused)[0])
            t0, t1, _ = two_pass(pool, plain)
            ts.setdefault((what, 'plain call'), []).append(t0)
            ts.setdefault((what, 'evaluate'), []).append(t1)
            ts.setdefault((what, 'two-pass'), []).append(t0 + t1)
        play_plain.clear_leaf_values()
        ts.setdefault(('playout to the end', 'plain call'), []).append(timed(to_the_end)[0])
    med = lambda k: sorted(ts[k])[REPEATS // 2]
    print("%s, %d roots %d rollout steps after reset(), %d children in all, one window of %d; table: material + advance, see-all, [2, 14, %d] int16"
          % (name, n, steps, total, m, table.shape[2]), flush=True)
    for k in ts:
        t = sorted(ts[k])
        print("%-22s %-10s median %8.3f ms  range %8.3f .. %8.3f  (%d runs)" % (k[0], k[1], med(k), t[0], t[-1], REPEATS), flush=True)
    for what, _, _, _, items in runs:
        f, tp = med((what, 'fused')), med((what, 'two-pass'))
        print("%-22s two-pass / fused = %.2fx; fused / plain call = %.3fx; %.3f G positions/s fused"
              % (what, tp / f, f / med((what, 'plain call')), items / f / 1e6), flush=True)
    end = med(('playout to the end', 'plain call'))
    for c in CAPS:
        print("playout to the end / max_steps %d with leaf values = %.2fx (%.3f ms against %.3f ms)"
              % (c, end / med(('playout max_steps %d' % c, 'fused')), end, med(('playout max_steps %d' % c, 'fused'))), flush=True)
    for x in (roots, kids_fused, kids_plain, play_fused, play_plain):
        x.close()


if __name__ == '__main__':
    main()
