"""Perfect-information Monte Carlo move choice for B live games at once, on the device: the loop playouts were built for.

    python -m stratego_env_amd.examples.pimc_move_chooser [--version fives] [--games 8] [--worlds 4] [--steps 6] [--biased] [--setup-prior]
                                                          [--max-steps 16 --leaf]

For every game the mover does not see the opponent's piece types.  PIMC samples W worlds that look the same to the mover
(PackedStates.determinize), tries every valid root action in every world (PackedStates.expand, whose parent_index fans the worlds out over
the actions), plays each child to the end with random moves (PackedStates.playout) and picks the action with the best mean result from the
mover's side -- or, with max_steps and a leaf-value table, only max_steps moves deep, the position reached scored by the table
(PackedStates.set_leaf_values): without the table a playout that is cut off reports 0, 0 and says nothing.  Three library calls and plain torch around them; nothing leaves the device until the chosen actions do, and the live env
is only read.
"""
import argparse

import torch

from stratego_env_amd.procedural_env import PackedStates
from stratego_env_amd.vec_env import VecStrategoEnv


def choose_moves(env, n_worlds=4, draw=0, seed=0, max_steps=0, weights=None, see_all=True, beliefs=None, leaf=None, origins=None):
    """env: a live VecStrategoEnv of B games.  -> (actions int64 [B]: the chosen absolute 1-D action per game, -1 where the game is over;
    values float32 [B, action_size]: the mean playout result of every valid root action from the root mover's side, -inf elsewhere).
    The worlds and the playouts are keyed by (seed, slot, draw): the same arguments give the same choice.
    weights: None = uniformly random playouts; else a [4, 13, 14] weight table (stratego_env_amd.playout_policies) the playouts draw their
    moves by; see_all (with weights only): the playout players look at the sampled world's true piece types, as PIMC assumes.
    beliefs: None = worlds sampled uniformly; else a [2, 12, cells] belief table (stratego_env_amd.beliefs; numpy or a device tensor) the
    hidden pieces are dealt by (PackedStates.determinize(..., beliefs=...)).
    origins (with beliefs): int16 device tensor [B, 2, cells], the cell every piece of every game stood on at its setup -- the labels of a
    tracked replay of the games' action logs from their start records (replay(..., track_origins=True).origins).  `beliefs` is then read
    as a prior over SETUP cells and carried along the moves (stratego_env_amd.beliefs.follow): one table per game.
    leaf: None = a playout cut off by max_steps counts 0; else (table, limit, denom) as PackedStates.set_leaf_values takes them
    (stratego_env_amd.leaf_values builds tables): the position a cut-off playout reached is scored by the table, on the sampled world's
    true pieces."""
    B, W, dev = env.num_envs, int(n_worlds), env.device
    dev_index = dev.index
    info = env.env_info()
    mover, live = info[:, 3].to(torch.int8), info[:, 2] == 0
    # W worlds per game, world-major: slot w * B + b is world w of game b
    worlds = PackedStates(env.variant, B * W, device=dev_index, seed=seed)
    children = None
    try:
        game_of_world = torch.arange(B, dtype=torch.int32, device=dev).repeat(W)
        if origins is not None:
            if beliefs is None:
                raise ValueError("origins carry a prior over setup cells along the moves: pass beliefs")
            from stratego_env_amd.beliefs import follow
            prior = beliefs if isinstance(beliefs, torch.Tensor) else torch.from_numpy(beliefs.astype('int32'))
            beliefs = follow(prior.to(dev), origins)                  # [B, 2, 12, cells]: the table of game b for every world of b
        if beliefs is None:
            worlds.determinize(env, src_index=game_of_world, observer=0, draw=draw)
        else:
            worlds.determinize(env, src_index=game_of_world, observer=0, draw=draw, beliefs=beliefs)
        # the mover's valid actions are the same in every world of a game: world 0 speaks for all
        mask = worlds.valid_moves_as_1d_mask()[:B] != 0
        mask &= live[:, None]
        A = mask.shape[1]
        values = torch.full((B, A), float('-inf'), dtype=torch.float32, device=dev)
        game, action = mask.nonzero(as_tuple=True)                    # the M (game, action) pairs to try
        M = int(game.numel())
        if M:
            # child slot w * M + m: action m's move played in world w of its game
            parent = (torch.arange(W, device=dev)[:, None] * B + game[None, :]).reshape(-1).to(torch.int32)
            children = PackedStates(env.variant, W * M, device=dev_index, seed=seed)
            valid, _ = children.expand(worlds, action.repeat(W).to(torch.int32), parent_index=parent)
            assert bool(valid.all())
            if leaf is not None:
                table, limit, denom = leaf
                children.set_leaf_values(table, limit, denom, see_all=True)
            res = children.playout(children, max_steps=max_steps, draw=draw, weights=weights,
                                   see_all=see_all and weights is not None)          # in place: the children are scratch
            value = res.value_for(mover[game].repeat(W))
            sums = torch.zeros(B * A, dtype=torch.float32, device=dev)
            sums.index_add_(0, (game * A + action).repeat(W), value)
            values = torch.where(mask, sums.view(B, A) / W, values)
        actions = torch.where(mask.any(dim=1), values.argmax(dim=1), torch.full((B,), -1, dtype=torch.int64, device=dev))
        return actions, values
    finally:
        worlds.close()
        if children is not None:
            children.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--version', default='fives')
    ap.add_argument('--games', type=int, default=8)
    ap.add_argument('--worlds', type=int, default=4)
    ap.add_argument('--steps', type=int, default=6, help='random moves played before the choice')
    ap.add_argument('--biased', action='store_true', help='playouts that prefer winning attacks and forward moves (playout_policies.capture_biased)')
    ap.add_argument('--max-steps', type=int, default=0, help='moves per playout (0 = to the end of the game)')
    ap.add_argument('--leaf', action='store_true', help='score cut-off playouts by material and advance (leaf_values.material / with_advance)')
    ap.add_argument('--setup-prior', action='store_true',
                    help="worlds dealt by where humans place their pieces (beliefs.setup_prior; --version barrage or standard)")
    args = ap.parse_args()
    env = VecStrategoEnv(args.version, args.games, seed=1, auto_reset=False)
    env.reset()
    env.rollout_steps(args.steps)
    weights = None
    if args.biased:
        from stratego_env_amd.playout_policies import capture_biased
        weights = capture_biased(args.version)
    beliefs = None
    if args.setup_prior:
        from stratego_env_amd.beliefs import setup_prior
        beliefs = setup_prior(args.version)
    leaf = None
    if args.leaf:
        from stratego_env_amd import leaf_values
        denom = 2 * leaf_values.side_total(args.version)
        leaf = (leaf_values.with_advance(leaf_values.material(args.version), 1, rows=env.variant.rows), denom - 1, denom)
    actions, values = choose_moves(env, args.worlds, max_steps=args.max_steps, weights=weights, beliefs=beliefs, leaf=leaf)
    for b, a in enumerate(actions.tolist()):
        if a < 0:
            print("game %d: over" % b)
        else:
            print("game %d: action %d, mean playout value %+.3f over %d worlds (%d actions tried)"
                  % (b, a, float(values[b, a]), args.worlds, int(torch.isfinite(values[b]).sum())))
    env.close()


if __name__ == '__main__':
    main()
