"""In-process A/B of the store policy of MULTI-STEP launches on ONE env object and ONE set of placed buffers: does a multi-step launch
whose waves rewrite their own games' lines every n_sets steps keep those lines in the 256 MiB Infinity Cache when they leave as plain
stores?  The launch's policy today ('auto') is keyed on the launch's total observation bytes x sets, which for 65,536 Barrage games is
1.76 GB in place and 5.3 GB for the ring of three: all whole lines non-temporal.  What a resident wave rewrites within reach is far less
(6,144 resident waves x 30,512 B = 188 MB in place).  The buffers are placed as bench.py places them (tune_placement, then
alloc_output_ring), the policies alternate round by round, every call is `--call-steps` steps (one launch at the default 256) between HIP
events.

    python tools/store_split_ab.py [--games 65536] [--version barrage] [--steps-in 100] [--rounds 6] [--call-steps 256] [--sets 3]
                                   [--legs in_place,ring] [--counts 0,24,48,...] [--no-plain] [--baseline auto|nt] [--log profiles/store_split_ab.log]

--counts: next to 'auto' (and 'plain' unless --no-plain) one policy per count: non-temporal stores with that many leading 128-byte lines
of every game's observation plain (SGX_NT_PLAIN_LINES, read when a handle is created: every count gets a handle of its own -- the same
games, as far into them -- that writes the FIRST handle's buffers).

Prints, per leg, every round's us per step for each policy, then min / median / max, and the verdict by the protocol of DESIGN.md
section 4.2: a policy wins against the baseline (the first policy: 'auto', or with --baseline nt every whole line non-temporal, which is
what 'auto' chose for these launches before the rule looked at the resident games) where its MEDIAN is below the baseline's MINIMUM.  --log appends the same lines to a file."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from stratego_env_amd import _lib  # noqa: E402
from stratego_env_amd.vec_env import VecStrategoEnv  # noqa: E402


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=65536)
    ap.add_argument('--version', default='barrage')
    ap.add_argument('--steps-in', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--call-steps', type=int, default=256)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--legs', default='in_place,ring')
    ap.add_argument('--placement-gb', type=float, default=8.0)
    ap.add_argument('--placement-wide-gb', type=float, default=64.0)
    ap.add_argument('--counts', default='')
    ap.add_argument('--no-plain', action='store_true')
    ap.add_argument('--baseline', default='auto', choices=('auto', 'nt'))
    ap.add_argument('--log', default=None)
    args = ap.parse_args()
    logf = open(args.log, 'a') if args.log else None

    def say(line):
        print(line, flush=True)
        if logf:
            logf.write(line + '\n')
            logf.flush()

    x = torch.empty(1 << 28, device='cuda')          # out of the idle power state
    t0 = time.time()
    while time.time() - t0 < 2.0:
        x.fill_(1.0)
        torch.cuda.synchronize()
    del x
    env = VecStrategoEnv(args.version, args.games, seed=0x5712A7E60, auto_reset=True, placement='plain')
    env.reset()
    free, _ = torch.cuda.mem_get_info()
    cap = int(free * 0.4)
    budget = min(max(int(args.placement_gb * (1 << 30)), 4 * env.obs.numel() * 4), cap)
    wide = min(int(args.placement_wide_gb * (1 << 30)), cap)
    streams = env.obs.numel() * 4 > 300e6
    rep = env.tune_placement(None, max_extra_bytes=budget if streams else 0, wide_extra_bytes=wide)
    t = (rep.get('wide') or {}).get('obs') if (rep.get('wide') or {}).get('used') else rep.get('obs')
    legs = args.legs.split(',')
    if 'ring' in legs:
        env.alloc_output_ring(args.sets, tune=streams and budget >= env.obs.numel() * 4, max_extra_bytes=budget, wide_extra_bytes=wide)
    obs_b, mask_b = env.obs[0].numel() * 4, env.mask[0].numel()
    say("# store_split_ab: %d %s games, build id %s, %d B observation + %d B mask per game, %d steps in, %d rounds of %d-step calls%s" % (
        args.games, args.version, env.build_id, obs_b, mask_b, args.steps_in, args.rounds, args.call_steps,
        ", placement kept %.1f us (observe launch)" % min(t) if t else ""))
    env.rollout_steps(args.steps_in)
    torch.cuda.synchronize()
    # 'nt' = every whole line non-temporal: what 'auto' chose for these launches before the rule looked at the resident games
    policies = ([('nt', env, True)] if args.baseline == 'nt' else []) + [('auto', env, 'auto')] + ([] if args.no_plain else [('plain', env, False)])
    for count in [int(c) for c in args.counts.split(',') if c != '']:
        os.environ['SGX_NT_PLAIN_LINES'] = str(count)
        try:
            e = VecStrategoEnv(args.version, args.games, seed=0x5712A7E60, auto_reset=True, placement='plain')
        finally:
            del os.environ['SGX_NT_PLAIN_LINES']
        e.reset()
        e.rollout_steps(args.steps_in)
        torch.cuda.synchronize()
        e.obs, e.mask = env.obs, env.mask                      # from here on it writes the first handle's buffers
        if env._ring:
            e._ring, e._ring_owners = list(env._ring), list(env._ring_owners)
            e._ring_ios, e._ring_pos = (_lib.SgxStepIO * len(e._ring))(), 0
        torch.cuda.empty_cache()
        policies.append(('n=%d' % count, e, 'auto'))
    for leg in legs:
        ring = leg == 'ring'
        call_of = lambda e: (lambda k: e.rollout_steps(k, ring=True)) if ring else (lambda k: e.rollout_steps(k))     # noqa: E731
        what = "ring of %d placed sets (%.2f GB)" % (args.sets, args.sets * args.games * obs_b / 1e9) if ring else "in place (%.2f GB)" % (args.games * obs_b / 1e9)
        us = {name: [] for name, _, _ in policies}
        for name, e, mode in policies:                # one untimed call each: first-use work of either path stays out of round 0
            e.set_nt_stores(mode)
            call_of(e)(args.call_steps)
        for rnd in range(args.rounds):
            for name, e, mode in (policies if rnd % 2 == 0 else policies[::-1]):
                e.set_nt_stores(mode)
                us[name].append(timed(call_of(e), args.call_steps))
                assert e.last_launch_kind in (_lib.LAUNCH_MULTI_STEP, _lib.LAUNCH_MULTI_STEP_WAVE), "not a multi-step launch"
            say("%-8s round %d: %s" % (leg, rnd, "   ".join("%s %7.1f us" % (name, us[name][-1]) for name, _, _ in policies)))
        env.set_nt_stores('auto')
        say("%-8s %s" % (leg, what))
        base = policies[0][0]
        a = us[base]
        for name, _, _ in policies:
            v = us[name]
            med = statistics.median(v)
            if name == base:
                verdict = ""
            elif med < min(a):
                verdict = "WINS against %s (median below its minimum %.1f: %+.1f %%)" % (base, min(a), 100 * (med / statistics.median(a) - 1))
            elif statistics.median(a) < min(v):
                verdict = "LOSES against %s (whose median %.1f is below this minimum: %+.1f %%)" % (base, statistics.median(a), 100 * (med / statistics.median(a) - 1))
            else:
                verdict = "level with %s within the spread" % base
            say("%-8s %-6s: min %7.1f  median %7.1f  max %7.1f us per step  %s" % (leg, name, min(v), med, max(v), verdict))
    for _, e, _ in policies:
        assert int(e.invalid_action.sum()) == 0
    for _, e, _ in policies[::-1]:
        if e is not env:
            e.obs = e.mask = e._ring = e._ring_owners = None
            e.close()
    env.close()


if __name__ == '__main__':
    main()
