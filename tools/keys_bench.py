"""state_keys against the way a caller could tell positions apart before it, on the same records.

Workload: 65,536 records, 100 rollout steps after reset() (setups from the variant's table, no auto-reset), Barrage and Standard.
  (a) state        sgx_state_keys, the state key
  (b) mover        ... the information-set key of each record's mover (view 0)
  (c) plus / minus ... of player +1 / of player -1
  (d) no clock     ... the state key without turn count and max turns
  (e) wide         ... the state key, both words
  (f) unpack       what the parent commit has: unpack() to the int64 [n,34,R,C] states alone
  (g) unpack+dot   ... and one torch reduction of them against a fixed tensor of odd int64 weights (a multiply-add hash: the cheapest identity
                   torch arithmetic gives), plus the mover's term
All run interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up of one each; every repetition, min and
median are printed, then records/s by the median and the ratios (f)/(a) and (g)/(a).  The tool checks the keys of the first records
against the numpy restatement of the rule (tests/keys_rule.py) and that (a) and (g) split the records into the same groups.
    python tools/keys_bench.py [variant ...] [--games N] [--steps T]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, REPEATS = 65536, 100, 5


def bench(name, n, steps):
    import numpy as np
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tests import keys_rule as kr

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
    env.rollout_steps(steps, emit_obs=False, emit_mask=False)
    pool = PackedStates(name, n)
    pool.copy_from(env)
    env.close()
    dev = pool.device
    v = pool._vec.variant
    rec_bytes = int(pool._vec._L.sgx_record_bytes(pool._vec._h))
    gen = torch.Generator(device='cpu').manual_seed(1)
    weights = (torch.randint(-(1 << 62), 1 << 62, (34 * v.rows * v.columns,), generator=gen, dtype=torch.int64) | 1).to(dev)
    out = {}

    def keys(**kw):
        def fn():
            out['keys'] = pool.state_keys(**kw)
        return fn

    def unpack():
        out['states'], out['players'] = pool.unpack()

    def unpack_dot():
        unpack()
        out['dot'] = (out['states'].reshape(n, -1) * weights).sum(dim=1) + out['players'].to(torch.int64) * 0x2545F4914F6CDD1D

    kinds = (('(a) state', keys()), ('(b) mover', keys(observer=0)), ('(c) plus', keys(observer=1)), ('(c) minus', keys(observer=-1)),
             ('(d) no clock', keys(clock=False)), ('(e) wide', keys(wide=True)), ('(f) unpack', unpack), ('(g) unpack+dot', unpack_dot))
    for _, fn in kinds:                                                      # warm-up
        fn()
    # the keys are the rule's, and both identities split the records into the same groups
    m = 256
    st, pl = out['states'][:m].cpu().numpy(), out['players'][:m].cpu().numpy()
    for kw in (dict(), dict(observer=0), dict(clock=False)):
        got = pool.state_keys(index=torch.arange(m, dtype=torch.int32), **kw).cpu().numpy()
        assert np.array_equal(got, kr.as_int64(kr.keys(st, pl, **kw))), kw
    state_keys = pool.state_keys()
    n_keys, n_dot = int(torch.unique(state_keys).numel()), int(torch.unique(out['dot']).numel())
    assert n_keys == n_dot == int(torch.unique(torch.stack([state_keys, out['dot']], dim=1), dim=0).shape[0]), (n_keys, n_dot)

    ts = {k: [] for k, _ in kinds}
    for _ in range(REPEATS):
        for k, fn in kinds:
            ts[k].append(timed(fn))
    print("%s, %d records %d rollout steps after reset(), %d distinct positions; a record is %d B (%.1f MB read, %.1f MB of keys written), an int64 state %d B"
          % (name, n, steps, n_keys, rec_bytes, n * rec_bytes / 1e6, n * 8 / 1e6, 34 * v.rows * v.columns * 8), flush=True)
    med = lambda k: sorted(ts[k])[REPEATS // 2]
    for k, _ in kinds:
        t = sorted(ts[k])
        print("%-15s %s ms (min %.3f, median %.3f; %.3f G records/s by the median)" % (k, " / ".join("%.3f" % x for x in ts[k]), t[0], med(k), n / med(k) / 1e6),
              flush=True)
    print("(a) reads its records at %.2f TB/s; (f) / (a): %.1fx; (g) / (a): %.1fx (medians)"
          % (n * rec_bytes / med('(a) state') / 1e9, med('(f) unpack') / med('(a) state'), med('(g) unpack+dot') / med('(a) state')), flush=True)
    pool.close()


def main():
    from stratego_env_amd import build as hip_build
    from tools.kernel_notes import kernel_notes, short_name
    args = sys.argv[1:]
    names = [a for i, a in enumerate(args) if not a.startswith('--') and not a.isdigit()] or ['barrage', 'standard']
    n = int(args[args.index('--games') + 1]) if '--games' in args else N
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else T
    for name in names:
        bench(name, n, steps)
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'keys_kernel' in kname:
            print("%-40s vgpr %3d sgpr %3d scratch %4d lds %6d" % (short_name(kname), r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
