"""What an agent decision against the built-in opponent costs (sgx_step_vs): 65,536 games, 100 random-valid steps into their
games (auto-reset on, so every game is running), per variant:
  (a) step_vs in place            sgx_step_vs on the live env: the agent's move and the bot's reply, no observation
  (b) gather+replay+playout+scatter   what it replaces on the parent's API: sgx_copy_envs into a pool, sgx_replay of one action,
                                  sgx_playout_weighted with max_steps = 1, sgx_copy_envs back through an index (no per-slot side, no refusals)
  (c) logic-only step             one env.step without observation and mask
  (d) VsBotVecEnv.step            per agent decision: step_vs, reset of the finished games, the bot's opening call, one observe
      two env.step with outputs   the self-play loop's two full steps per agent decision (rollout_step twice: the fused sampler included)
  playout_weighted / replay       max_steps = 20 / 20 recorded actions, this build and -- with --parent-lib PATH, a build of the parent
                                  commit's sources -- the parent's library in the same process on the same records: the existing kernels
                                  are the code they were (profiles/step_vs_kernel_notes.txt)
All interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up; median and min ... max are printed and written
to --out (default profiles/step_vs_bench.log).
    python tools/step_vs_bench.py [barrage standard] [--games N] [--parent-lib PATH] [--out PATH]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, REPEATS, LEN = 65536, 9, 20
NEW_SYMBOLS = ('sgx_step_vs',)


def load_parent(path):
    """The parent commit's library under this package's binding: it lacks the entry point this commit adds, which no call here makes on
    it; the symbol is bound to this build's so that the binding is complete."""
    from stratego_env_amd import _lib
    raw, here = C.CDLL(path), C.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        try:
            getattr(raw, sym)
        except AttributeError:
            setattr(raw, sym, getattr(here, sym))
    L = _lib._bind(raw)
    assert L.sgx_abi_version() == _lib.ABI_VERSION
    L.build_id = L.sgx_build_id().decode('ascii', 'replace')
    _lib._libs[path] = L
    return L


def bench(name, n, parent, say):
    import torch
    from stratego_env_amd import _lib, playout_policies as pol
    from stratego_env_amd.procedural_env import PackedStates, StepVsResult
    from stratego_env_amd.vec_env import VecStrategoEnv
    from stratego_env_amd.vs_env import VsBotVecEnv

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3                                      # us

    table = pol.capture_biased(name)
    dev = torch.device('cuda', 0)
    sides = torch.where(torch.arange(n, device=dev) % 2 == 0, 1, -1).to(torch.int8)
    everyone = torch.arange(n, dtype=torch.int32, device=dev)

    def live(lib_path=None):
        e = VecStrategoEnv(name, n, seed=9, auto_reset=True, placement='plain', outputs=True, lib_path=lib_path)
        e.reset()
        e.rollout_steps(100, emit_obs=False, emit_mask=False)
        return e

    def valid_actions(e):
        e.observe(emit_obs=False)
        return e.sample_valid_actions().clone()

    env, env_c = live(), live()
    tmp, sink = PackedStates(name, n, seed=9), PackedStates(name, n, seed=9)
    res = StepVsResult.empty(n, dev)
    env.step_vs(valid_actions(env), sides, table, out=res)                   # from here on every running game has its agent to move
    state = {}

    def replaced():
        tmp.copy_from(env, src_index=everyone)
        tmp.replay(tmp, state['acts'].view(n, 1))
        tmp.playout(tmp, max_steps=1, weights=table, draw=state['rep'])
        sink.copy_from(tmp, dst_index=everyone)

    # the existing kernels: LEN recorded actions from a snapshot, and weighted playouts of LEN moves, in this build and in the parent's
    start = env_c.snapshot()
    log = torch.empty((LEN, n), dtype=torch.int32, device=dev)
    for t in range(LEN):
        log[t] = valid_actions(env_c)
        env_c.step(log[t], emit_obs=False, emit_mask=False)
    dense = log.T.contiguous()
    dst = PackedStates(name, n, seed=9)
    # ((b) first: it reads the positions the actions were sampled for, (a) then moves them on)
    kinds = [('(b) gather+replay+playout+scatter', replaced),
             ('(a) step_vs in place', lambda: env.step_vs(state['acts'], sides, table, draw=state['rep'], out=res)),
             ('(c) logic-only step', lambda: env_c.step(state['acts_c'], emit_obs=False, emit_mask=False)),
             ('replay %d, this build' % LEN, lambda: dst.replay(start, dense)),
             ('playout_weighted %d, this build' % LEN, lambda: dst.playout(start, max_steps=LEN, weights=table, draw=3))]
    closing = [env, env_c, tmp, sink, start, dst]
    if parent:
        load_parent(parent)
        p_start = VecStrategoEnv(name, n, seed=9, human_inits=False, outputs=False, lib_path=parent)
        p_dst = VecStrategoEnv(name, n, seed=9, human_inits=False, outputs=False, lib_path=parent)
        p_start.import_state(*start.export_state())                          # the same positions
        wp = table.ctypes.data_as(C.POINTER(C.c_uint16))
        out5 = [torch.empty((n, 2), dtype=torch.float32, device=dev)] + [torch.empty((n,), dtype=t, device=dev) for t in (torch.uint8, torch.uint8, torch.int8, torch.int32)]
        pio = _lib.SgxPlayoutIO(*[t.data_ptr() for t in out5], LEN, 0)
        kinds += [('replay %d, parent' % LEN, lambda: p_dst.replay(p_start, dense)),
                  ('playout_weighted %d, parent' % LEN,
                   lambda: _lib.check(p_dst._L.sgx_playout_weighted(p_dst._h, p_start._h, None, C.byref(pio), wp, 0, 3, p_dst._stream()), p_dst._L))]
        closing += [p_start, p_dst]
    ts = {k: [] for k, _ in kinds}
    for rep in range(REPEATS + 1):                                          # (the first repetition is the warm-up)
        state.update(rep=rep + 1, acts=valid_actions(env), acts_c=valid_actions(env_c))
        for k, fn in kinds:
            t = timed(fn)
            if rep:
                ts[k].append(t)
    if parent:                                                              # the same records from both builds
        dst.playout(start, max_steps=LEN, weights=table, draw=3)
        state['same'] = bool(torch.equal(dst.unpack()[0], p_dst.export_state()[0]))
    for x in closing:
        x.close()

    # (d): the wrapper's decision against the self-play loop's two full steps, both with observation and mask, default placement
    vs = VsBotVecEnv(name, n, opponent=table, agent=sides, seed=9)
    vs.reset()
    two = VecStrategoEnv(name, n, seed=9, auto_reset=True)
    two.reset()
    two.rollout_steps(100)
    for _ in range(50):
        vs.step(vs.env.sample_valid_actions())

    def two_steps():
        two.rollout_step()
        two.rollout_step()
    kinds_d = [('(d) VsBotVecEnv.step', lambda: vs.step(state['acts'])), ('    two env.step with outputs', two_steps)]
    for k, _ in kinds_d:
        ts[k] = []
    for rep in range(REPEATS + 1):
        state['acts'] = vs.env.sample_valid_actions().clone()
        for k, fn in kinds_d:
            t = timed(fn)
            if rep:
                ts[k].append(t)
    vs.close(); two.close()
    med = lambda k: sorted(ts[k])[len(ts[k]) // 2]
    say("%s, %d games, 100 steps in, %d repetitions, us per call: median (min ... max)" % (name, n, REPEATS))
    for k in ts:
        say("  %-36s %9.1f (%9.1f ... %9.1f)" % (k, med(k), min(ts[k]), max(ts[k])))
    say("  (a) / (b) %.3f; (a) / (c) %.3f; (d) / two steps %.3f (medians)"
        % (med('(a) step_vs in place') / med('(b) gather+replay+playout+scatter'), med('(a) step_vs in place') / med('(c) logic-only step'),
           med('(d) VsBotVecEnv.step') / med('    two env.step with outputs')))
    if parent:
        for k in ('replay %d' % LEN, 'playout_weighted %d' % LEN):
            say("  %s: this build / parent %.3f (medians)" % (k, med(k + ', this build') / med(k + ', parent')))
        say("  the weighted playouts of both builds end in the same positions: %s" % state['same'])


def main():
    args = sys.argv[1:]
    opts = {'--games': N, '--parent-lib': None, '--out': os.path.join(ROOT, 'profiles', 'step_vs_bench.log')}
    for k in opts:
        if k in args:
            opts[k] = args[args.index(k) + 1]
    skip = {args.index(k) + 1 for k in opts if k in args}
    names = [a for i, a in enumerate(args) if not a.startswith('--') and i not in skip] or ['barrage', 'standard']
    from stratego_env_amd import build as hip_build
    from tools.kernel_notes import kernel_notes
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say("tools/step_vs_bench.py, library build id %s%s" % (hip_build.source_hash(), ', parent library given' if opts['--parent-lib'] else ''))
    for name in names:
        bench(name, int(opts['--games']), opts['--parent-lib'], say)
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'step_vs_kernel' in kname and 'ILi10ELi10ELi' in kname:
            say("%-72s vgpr %3d sgpr %3d scratch %4d lds %6d" % (kname[:72], r['vgpr'], r['sgpr'], r['scratch'], r['lds']))
    with open(opts['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
