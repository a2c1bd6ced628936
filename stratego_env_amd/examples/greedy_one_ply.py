"""A greedy one-ply move choice for a pool of positions, on the device: every child of every root scored in the launch that makes it.

    python -m stratego_env_amd.examples.greedy_one_ply [--version fives] [--games 8] [--steps 6]

count_moves numbers the children, expand_all writes them into a pool that has a leaf-value table set (PackedStates.set_leaf_values) -- so the
reward it reports for a child whose game goes on is the child's material-and-position value, not 0 -- and a segmented arg-max in torch picks,
per root, the child that is best from the root mover's side.  One pass over the children; no second launch reads them back.
"""
import argparse

import torch

from stratego_env_amd import leaf_values
from stratego_env_amd.procedural_env import PackedStates
from stratego_env_amd.vec_env import VecStrategoEnv


def greedy_moves(roots, table, limit, denom, see_all=True):
    """roots: a PackedStates of B positions.  -> (actions int64 [B]: the absolute 1-D action of the best child per root, the first of equals,
    -1 where the root has no move; values float32 [B]: that child's reward from the root mover's side, -inf where there is none).
    table / limit / denom / see_all: as PackedStates.set_leaf_values takes them; see_all=True scores the true pieces (a determinized
    world, or a perfect-information game)."""
    dev = roots.device
    B = roots.n
    mover = roots._vec.env_info()[:, 3].to(torch.int8)
    _, offsets = roots.count_moves()
    total = int(offsets[-1])                                               # (the one synchronisation)
    actions = torch.full((B,), -1, dtype=torch.int64, device=dev)
    values = torch.full((B,), float('-inf'), dtype=torch.float32, device=dev)
    if total == 0:
        return actions, values
    children = PackedStates(roots._vec.variant, total, device=dev.index)
    try:
        children.set_leaf_values(table, limit, denom, see_all=see_all)
        res = children.expand_all(roots, offsets=offsets, actions_1d=True)
        parent = res.parent.long()
        value = res.value_for(mover[parent])
        values.scatter_reduce_(0, parent, value, reduce='amax')
        # the first child that reaches its root's best value
        number = torch.arange(total, device=dev)
        first = torch.full((B,), total, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, parent, torch.where(value == values[parent], number, torch.full_like(number, total)), reduce='amin')
        has = first < total
        actions[has] = res.action[first[has]].long()
        return actions, values
    finally:
        children.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--version', default='fives')
    ap.add_argument('--games', type=int, default=8)
    ap.add_argument('--steps', type=int, default=6, help='random moves played before the choice')
    ap.add_argument('--advance', type=int, default=1, help='bonus per row a movable piece has advanced')
    args = ap.parse_args()
    env = VecStrategoEnv(args.version, args.games, seed=1, auto_reset=False)
    env.reset()
    env.rollout_steps(args.steps)
    roots = PackedStates(env.variant, args.games, device=env.device.index)
    roots.copy_from(env)
    table = leaf_values.with_advance(leaf_values.material(env.variant), args.advance, rows=env.variant.rows)
    denom = 2 * leaf_values.side_total(env.variant)
    actions, values = greedy_moves(roots, table, denom - 1, denom)
    for b, a in enumerate(actions.tolist()):
        print("game %d: %s" % (b, "no move" if a < 0 else "action %d, value %+.4f" % (a, float(values[b]))))
    roots.close()
    env.close()


if __name__ == '__main__':
    main()
