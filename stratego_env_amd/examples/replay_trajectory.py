"""Keep start records and actions instead of observations, and re-render the observation of any (game, t) when it is sampled.

    python -m stratego_env_amd.examples.replay_trajectory [--version fives] [--games 8] [--steps 12] [--samples 6]

A learner that keeps every step's observation of a rollout stores R x C x 67 floats per game and step.  The position at step t is a function
of the game's start record and its first t actions, so this loop keeps only those -- 4 bytes per game and step -- and rolls out without
writing an observation at all.  When the learner samples (game, t) pairs, one replay launch puts those positions into a small env
(VecStrategoEnv.replay: src_index picks the start record, lengths says how many of the game's actions to apply) and observe() renders
them.  The check at the end plays the same actions step by step with observations switched on and compares.
"""
import argparse

import torch

from stratego_env_amd.procedural_env import PackedStates
from stratego_env_amd.vec_env import VecStrategoEnv


def record_rollout(env, start, n_steps):
    """Snapshot the start records of `env` into the pool `start`, then play n_steps random valid moves per game without rendering an
    observation.  -> actions int32 [n_steps, N]: the action each game played at each step (the [T][N] layout of a trajectory's action log)."""
    start.copy_from(env)
    actions = torch.empty((n_steps, env.num_envs), dtype=torch.int32, device=env.device)
    for t in range(n_steps):
        actions[t] = env.sample_valid_actions()
        env.step(actions[t], emit_obs=False)
    return actions


def rerender(view, start, actions, game, t):
    """The observations, masks and movers of the sampled pairs (game[i], t[i]): slot i of `view` becomes start record game[i] advanced by the
    first t[i] actions of that game, then observe().  actions: the [T, N] log."""
    lists = actions.T[game.long()]                                # [S, T]: the sampled games' lists
    res = view.replay(start, lists, lengths=t, src_index=game)
    assert bool((res.stop != 2).all()), "a recorded action is valid where it was played"
    return view.observe()


def rerender_check(version='fives', games=8, steps=12, samples=6, seed=3):
    """Roll out, re-render `samples` random (game, t) pairs and compare them with a step-by-step run.  -> the number of pairs compared."""
    env = VecStrategoEnv(version, games, seed=seed, auto_reset=False, human_inits=False)
    env.reset()
    start = PackedStates(version, games)
    actions = record_rollout(env, start, steps)
    played = env.env_info()[:, 0]                                 # moves each game really played (a finished game stops counting)
    gen = torch.Generator().manual_seed(seed)
    game = torch.randint(0, games, (samples,), generator=gen).to(device=env.device, dtype=torch.int32)
    t = (torch.rand(samples, generator=gen).to(env.device) * (played[game.long()] + 1).float()).floor().to(torch.int32)
    t = torch.minimum(t, played[game.long()])

    view = VecStrategoEnv(version, samples, seed=seed, auto_reset=False, human_inits=False)
    obs, mask, player = rerender(view, start, actions, game, t)

    # the same positions from a run that renders every step: a replay of length 0 is a copy of the start records
    ref = VecStrategoEnv(version, games, seed=seed, auto_reset=False, human_inits=False)
    ref.replay(start, actions[:0].T)
    ref_obs, ref_mask, ref_player = ref.observe()
    checked = 0
    for step in range(steps + 1):
        for i in (t == step).nonzero().flatten().tolist():
            g = int(game[i])
            assert torch.equal(obs[i], ref_obs[g]) and torch.equal(mask[i], ref_mask[g]) and int(player[i]) == int(ref_player[g]), (g, step)
            checked += 1
        if step < steps:
            ref_obs, ref_mask, _, _, ref_player = ref.step(actions[step])
    for x in (env, start, view, ref):
        x.close()
    return checked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--version', default='fives')
    ap.add_argument('--games', type=int, default=8)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--samples', type=int, default=6)
    args = ap.parse_args()
    n = rerender_check(args.version, args.games, args.steps, args.samples)
    print("%d sampled (game, t) pairs re-rendered from start records + actions: byte-equal to the step-by-step run" % n)


if __name__ == '__main__':
    main()
