"""Belief tables for weighted determinization (PackedStates.determinize(..., beliefs=...), sgx_determinize_weighted).  Host only, plain
numpy; move a table to the device with torch.from_numpy(table.astype(numpy.int32)).cuda().  (`follow` alone also takes device tensors.)

A table is uint16 [2, 12, cells], read as beliefs[player index of the piece's owner][type - 1][absolute cell], every entry in [0, 4095]:
  player     0 = player +1, 1 = player -1 (as the layers of a state are); a determinization reads the block of the observer's OPPONENT;
  type       1..12 (spy .. marshal, 11 = flag, 12 = bomb) at index type - 1;
  cell       r * columns + c in ABSOLUTE board coordinates, not in a player's perspective.
The hidden types are dealt one instance after the other (flags, bombs, then 10 .. 1), each onto a free hidden cell drawn with probability
weight / (sum of the weights of the free candidate cells).  A weight of 0 is never taken while a candidate has a positive one; where all
candidates weigh 0 the draw is uniform and the world counts it in off_belief.  The weights steer this sequential deal: they are NOT the
marginals of the sampled worlds (a cell an earlier type took is gone for the later ones)."""
import numpy as np

from .config import get_variant
from .setups import load_setup_table

WEIGHT_MAX = 4095
TYPES = 12
FLAG, BOMB = 11, 12


def shape(variant):
    """(2, 12, cells) of a variant (a name or a Variant)."""
    v = get_variant(variant)
    return (2, TYPES, v.rows * v.columns)


def uniform(variant):
    """Every (type, cell) the same weight 1: samples uniformly over the consistent worlds, the distribution of the unweighted
    determinization (any constant >= 1 does)."""
    return np.ones(shape(variant), dtype=np.uint16)


def _scale_counts(x, top):
    """Non-negative integers -> [0, 4095] with `top` -> 4095: floor(x * 4095 / top + 1/2) in integer arithmetic, and at least 1 where
    x > 0."""
    x = np.asarray(x, dtype=np.int64)
    if top <= 0:
        return np.zeros_like(x)
    w = (2 * WEIGHT_MAX * x + top) // (2 * top)
    return np.where(x > 0, np.maximum(w, 1), 0)


def from_probabilities(p):
    """float [..., 2, 12, cells] (probabilities, or any non-negative scores) -> uint16 of the same shape.  Every [12, cells] block -- one
    player's types of one table -- is scaled on its own so that its maximum becomes 4095 (a block of zeros stays zeros).
    Rounding: floor(p * 4095 / max + 1/2), halves up; an entry > 0 that would round to 0 becomes 1, so that only what the caller called
    impossible has weight 0.  Ratios below 1 : 4095 inside a block are therefore flattened to 1 : 4095.  ValueError for negative or
    non-finite entries."""
    p = np.asarray(p, dtype=np.float64)
    if p.ndim < 3 or p.shape[-3] != 2 or p.shape[-2] != TYPES:
        raise ValueError("beliefs must have shape [..., 2, 12, cells] (got %s)" % (tuple(p.shape),))
    if not np.isfinite(p).all() or (p < 0).any():
        raise ValueError("beliefs must be finite and >= 0")
    top = p.max(axis=(-2, -1), keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.floor(np.where(top > 0, p * (WEIGHT_MAX / np.where(top > 0, top, 1.0)), 0.0) + 0.5)
    w = np.where(p > 0, np.clip(w, 1, WEIGHT_MAX), 0)
    return w.astype(np.uint16)


def setup_counts(name):
    """int64 [2, 12, cells]: over ALL rows of the shipped setup table `name` ('barrage' or 'standard'), how often type t stands on absolute
    cell c at the start of a game in which that player was dealt the row (setups.own_side_maps and the 180-degree turn of player -1's
    side, as a reset places them)."""
    v = get_variant(name)
    R, C, U = v.rows, v.columns, v.initial_state_usable_rows
    table = load_setup_table(name)                                  # [n, U * C] piece codes in Gravon string order
    s = table.reshape(-1, U, C)
    counts = np.zeros((2, TYPES, R * C), dtype=np.int64)
    for t in range(1, TYPES + 1):
        per_cell = (s == t).sum(axis=0)                             # [U, C] in string order: string row U-1-r is board row r
        own = per_cell[::-1]                                        # player +1: absolute (r, c) <- s[(U-1-r) * C + c]
        board = np.zeros((R, C), dtype=np.int64)
        board[:U] = own
        counts[0, t - 1] = board.reshape(-1)
        board = np.zeros((R, C), dtype=np.int64)
        board[R - U:] = per_cell                                    # player -1: absolute (R-1-r, c) <- s[(U-1-r) * C + c]
        counts[1, t - 1] = board.reshape(-1)
    return counts


def setup_prior(name):
    """A ready-made table from the setups humans chose (the shipped Gravon tables: 'barrage' or 'standard').  For each player the counts of
    setup_counts are scaled so that the player's largest count becomes 4095 (floor(count * 4095 / max + 1/2); a count > 0 stays >= 1): on
    its own setup rows a hidden piece is drawn where players put that type.  On every cell outside the player's setup rows only a piece
    that has moved can stand: a movable type (1..10) gets, on each of those cells, its mean weight over the setup-row cells, rounded half
    up and at least 1; flag and bomb get 0 there.
    A heuristic prior on where humans place pieces -- not a posterior: it knows nothing of the moves played, and the weights of a moved
    piece's cells say only how common the type is.  `follow` turns it into a table per game that does know where each piece started."""
    v = get_variant(name)
    R, C, U = v.rows, v.columns, v.initial_state_usable_rows
    counts = setup_counts(name)
    out = np.zeros(counts.shape, dtype=np.int64)
    for p in range(2):
        w = _scale_counts(counts[p], int(counts[p].max()))          # [12, cells]
        rows = np.zeros(R, dtype=bool)
        if p == 0:
            rows[:U] = True
        else:
            rows[R - U:] = True
        inside = np.repeat(rows, C)                                 # [cells]: the player's setup rows
        n_in = int(inside.sum())
        for t in range(1, TYPES + 1):
            if t in (FLAG, BOMB):
                w[t - 1, ~inside] = 0
            else:
                total = int(w[t - 1, inside].sum())
                w[t - 1, ~inside] = max(1, (2 * total + n_in) // (2 * n_in))
        out[p] = w
    return out.astype(np.uint16)


def follow(prior, origins):
    """A prior over SETUP cells carried along the moves of every game: out[i][p][t][c] = prior[(i,) p][t][origins[i][p][c]] where the
    label lies in [0, cells), else 0.  origins: int16 [n, 2, cells], the labels of a tracked replay from the games' start positions
    (replay(..., track_origins=True).origins; sgx_set_replay_origins): origins[i][p][c] is the cell the piece of player index p on cell c of
    game i stood on at the start, -1 where it has none.  prior: [2, 12, cells] (one for all games) or [n, 2, 12, cells].
    -> [n, 2, 12, cells] of prior's dtype, one table per record as determinize(..., beliefs=...) takes it: the weight of type t on a cell
    is what the prior said of type t on the cell its piece was DEPLOYED on, so a piece that walked off its setup rows keeps the weights
    of where it came from, and a one-hot prior on the true setup stays one-hot on the truth.  Cells without a piece get weight 0 for every
    type; a determinization never reads them.
    numpy in -> numpy out; torch tensors in (both on one device) -> a tensor there, nothing synchronised.  The device form gathers each
    player's transposed [cells, 12] block (per game: [n, cells, 12]) with the [n, cells] labels, so no index as large as the result is built."""
    if isinstance(prior, np.ndarray) and isinstance(origins, np.ndarray):
        o = origins.astype(np.int64)
        if o.ndim != 3 or o.shape[1] != 2:
            raise ValueError("origins must have shape [n, 2, cells] (got %s)" % (tuple(origins.shape),))
        n, _, cells = o.shape
        if tuple(prior.shape) not in ((2, TYPES, cells), (n, 2, TYPES, cells)):
            raise ValueError("prior must have shape [2, 12, %d] or [%d, 2, 12, %d] (got %s)" % (cells, n, cells, tuple(prior.shape)))
        ok = (o >= 0) & (o < cells)
        idx = np.where(ok, o, 0)
        out = np.empty((n, 2, TYPES, cells), dtype=prior.dtype)
        for p in range(2):
            if prior.ndim == 3:
                out[:, p] = prior[p].T[idx[:, p]].transpose(0, 2, 1)                         # [cells, 12] rows by label
            else:
                out[:, p] = np.take_along_axis(prior[:, p], idx[:, p, None, :], axis=2)
        return out * ok[:, :, None, :].astype(prior.dtype)
    import torch
    if not isinstance(prior, torch.Tensor) or not isinstance(origins, torch.Tensor):
        raise ValueError("follow takes numpy arrays, or torch tensors on one device")
    if origins.dim() != 3 or origins.shape[1] != 2:
        raise ValueError("origins must have shape [n, 2, cells] (got %s)" % (tuple(origins.shape),))
    n, _, cells = (int(x) for x in origins.shape)
    if tuple(prior.shape) not in ((2, TYPES, cells), (n, 2, TYPES, cells)) or prior.device != origins.device:
        raise ValueError("prior must have shape [2, 12, %d] or [%d, 2, 12, %d] on the labels' device (got %s on %s)"
                         % (cells, n, cells, tuple(prior.shape), prior.device))
    o = origins.to(torch.int64)
    ok = (o >= 0) & (o < cells)
    idx = torch.where(ok, o, torch.zeros_like(o))
    out = torch.empty((n, 2, TYPES, cells), dtype=prior.dtype, device=prior.device)
    for p in range(2):
        if prior.dim() == 3:
            rows = prior[p].t().contiguous()[idx[:, p]]                                      # [n, cells, 12]
        else:
            rows = torch.gather(prior[:, p].transpose(1, 2), 1, idx[:, p, :, None].expand(n, cells, TYPES))
        out[:, p] = (rows * ok[:, p, :, None].to(prior.dtype)).transpose(1, 2)
    return out
