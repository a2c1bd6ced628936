"""From a recorded trajectory to belief-weighted worlds: track every piece back to its setup cell, so that a prior over setups follows the moves.

    python -m stratego_env_amd.examples.tracked_beliefs [--games 256] [--steps 60] [--draws 4]

beliefs.setup_prior says where humans deploy each piece type -- a statement about SETUP cells.  A determinization asks about the cells the
hidden pieces stand on NOW, and the record does not say which piece is which.  This loop keeps what a learner keeps anyway, the start records
and the [T][N] action log of rollout_trajectory, and gets the missing map from one launch: a tracked replay (replay(..., track_origins=True))
plays the log and reports, for every piece on the board at step t, the cell it started on.  beliefs.follow reads the prior through that map
into one table per game, and determinize(..., beliefs=...) deals the hidden pieces by it.

Printed: the share of hidden pieces that were dealt their true type, for the uniform deal, the plain setup prior (indexed by the cell a piece
stands on now) and the followed one.  The games are Barrage games from human setups played with uniformly random moves.
"""
import argparse

import torch

from stratego_env_amd import beliefs
from stratego_env_amd.procedural_env import PackedStates
from stratego_env_amd.vec_env import VecStrategoEnv


def record(env, start, steps):
    """Snapshot the start records of `env` into `start`, play `steps` random valid moves per game in one rollout_trajectory call and return the
    actions PLAYED, int32 [steps, N].  The trajectory's action log holds what every step DREW -- the action the next step plays -- so the
    list of a game is the draw before the call followed by the log without its last row."""
    start.copy_from(env)
    first = env.sample_valid_actions().clone()
    traj = env.alloc_trajectory(steps, results=False)
    env.rollout_trajectory(steps, traj)
    return torch.cat([first[None], traj['actions'][:steps - 1]])


def true_type_share(now, worlds, observer, table, draws):
    """Deal the hidden pieces of every record of `now` `draws` times by `table` (None: uniformly) and count how often a hidden piece got
    its true type.  -> (hits, hidden pieces dealt)."""
    state, player = now.unpack()
    n, cells = state.shape[0], state.shape[2] * state.shape[3]
    own, pub = state[:, 0:2].reshape(n, 2, cells), state[:, 3:5].reshape(n, 2, cells)
    who = player.long() if observer == 0 else torch.full_like(player.long(), observer)      # (0: each record's mover)
    opp = (who > 0).long()                                           # index of the observer's opponent: 1 where the observer is player +1
    pick = opp.view(n, 1, 1).expand(n, 1, cells)
    truth, shown = own.gather(1, pick)[:, 0], pub.gather(1, pick)[:, 0]
    hidden = (truth != 0) & (shown == 13)
    hits = total = 0
    for d in range(draws):
        if table is None:
            worlds.determinize(now, observer=observer, draw=d)
        else:
            worlds.determinize(now, observer=observer, draw=d, beliefs=table, validate=False)
        dealt = worlds.unpack()[0][:, 0:2].reshape(n, 2, cells).gather(1, pick)[:, 0]
        hits += int(((dealt == truth) & hidden).sum())
        total += int(hidden.sum())
    return hits, total


def run(games=256, steps=60, draws=4, seed=11, version='barrage'):
    """-> {'uniform' / 'setup_prior' / 'followed': share of hidden pieces dealt their true type} at step `steps` of `games` games."""
    env = VecStrategoEnv(version, games, seed=seed, auto_reset=False)     # setups from the variant's table of human setups
    env.reset()
    start, now, worlds = PackedStates(version, games), PackedStates(version, games), PackedStates(version, games, seed=seed + 1)
    try:
        played = record(env, start, steps)
        res = now.replay(start, played.T, track_origins=True)            # the [T][N] log as it is; a finished game stops at its end
        assert bool((res.stop != 2).all()), "a recorded action is valid where it was played"
        assert torch.equal(now.unpack()[0], env.export_state()[0]), "the replay reaches the position the rollout left"
        prior = torch.from_numpy(beliefs.setup_prior(version).astype('int16')).to(env.device)
        followed = beliefs.follow(prior, res.origins)                    # int16 [games, 2, 12, cells]
        out = {}
        for label, table in (('uniform', None), ('setup_prior', prior), ('followed', followed)):
            hits, total = true_type_share(now, worlds, 0, table, draws)   # observer 0: each record's mover
            out[label] = hits / max(total, 1)
        out['hidden_pieces'] = total // max(draws, 1)
        lab = res.origins.long()
        out['walked'] = int(((lab >= 0) & (lab != torch.arange(lab.shape[2], device=lab.device))).sum())
        return out
    finally:
        for x in (start, now, worlds, env):
            x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=256)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--draws', type=int, default=4)
    args = ap.parse_args()
    r = run(args.games, args.steps, args.draws)
    print("%d Barrage games, %d moves in: %d hidden pieces per deal, %d pieces off their setup cell" % (args.games, args.steps, r['hidden_pieces'], r['walked']))
    for k in ('uniform', 'setup_prior', 'followed'):
        print("%-12s %.4f of the hidden pieces dealt their true type" % (k, r[k]))


if __name__ == '__main__':
    main()
