"""BatchedStrategoProceduralEnv: the reference's functional operator API (StrategoProceduralEnv,
game/stratego_procedural_env.py:20-181) for a batch of caller-provided states.

Every method is a pure function of (states int64 [N,34,R,C] in the reference layout, players [N], actions [N]) and returns
fresh tensors, like the reference's methods do for one state.  Game logic runs in the HIP kernels: the states are imported
into a scratch handle (`sgx_import_state`), stepped / observed there, and exported again; tree-search style callers keep
their states on the device.  Where the reference raises ValueError for an invalid move, `get_next_state` returns a
`valid` mask and leaves that state unchanged.

Limits (documented in DESIGN.md): states must be reachable ones -- at most two non-zero recent-move cells per player and
no more captured pieces than pieces exist; the obstacle layer must equal the variant's (it is a per-handle constant).  Every
import reports which states it had to alter (`last_sanitised`, uint8 [N]; `strict=True` raises ValueError instead).

Every call imports the states it is given.  A caller that asks several questions about the SAME batch can hold it loaded:

    with env.loaded(states, players):
        mask = env.get_valid_moves_as_1d_mask(states, players)
        obs = env.get_partially_observable_observation_extended_channels(states, players)

(inside the scope, calls given the same tensor OBJECTS skip the import; the caller promises not to write to them meanwhile).
Search callers avoid the 27 KB int64 layout altogether with PackedStates (pack / expand / unpack below).
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib, index_algebra as ia
from .config import NUM_STATE_LAYERS, get_variant
from .vec_env import VecStrategoEnv

# layer pairs swapped by the perspective flip (impl:645-675)
_SWAP_A = [0, 3, 6, 32] + list(range(8, 20))
_SWAP_B = [1, 4, 7, 33] + list(range(20, 32))


def _ptr_or_none(t):
    return t.data_ptr() if t is not None else None


def playout_weights(weights):
    """A weight table of a weighted playout as the library takes it: contiguous uint16 [4, 13, 14] on the host, every entry in [0, 4095].
    `weights`: an array-like of any integer dtype (numpy, or a CPU tensor) of that shape; ValueError for anything else."""
    if isinstance(weights, torch.Tensor):
        if weights.is_cuda:
            raise ValueError("weights is read on the host: pass a numpy array or a CPU tensor")
        weights = weights.numpy()
    w = np.asarray(weights)
    if w.dtype.kind not in 'iu':
        raise ValueError("weights must have an integer dtype (got %s): round them yourself (playout_policies documents how it rounds)" % w.dtype)
    if w.shape != _lib.PLAYOUT_WEIGHTS_SHAPE:
        raise ValueError("weights must have shape [4, 13, 14] = [direction][moving piece][target] (got %s)" % (tuple(w.shape),))
    if w.size and (int(w.min()) < 0 or int(w.max()) > _lib.PLAYOUT_WEIGHT_MAX):
        bad = np.argwhere((w < 0) | (w > _lib.PLAYOUT_WEIGHT_MAX))[0]
        raise ValueError("weights[%d][%d][%d] = %d is outside [0, %d]" % (bad[0], bad[1], bad[2], int(w[tuple(bad)]), _lib.PLAYOUT_WEIGHT_MAX))
    return np.ascontiguousarray(w, dtype=np.uint16)


def leaf_table(table, cells):
    """A leaf-value table as the library takes it: contiguous int16 [2, 14, cells] on the host.  `table`: an array-like of any integer
    dtype (numpy, or a CPU tensor) of that shape with every entry within int16; ValueError for anything else."""
    if isinstance(table, torch.Tensor):
        if table.is_cuda:
            raise ValueError("the leaf-value table is read on the host: pass a numpy array or a CPU tensor")
        table = table.numpy()
    t = np.asarray(table)
    if t.dtype.kind not in 'iu':
        raise ValueError("the leaf-value table must have an integer dtype (got %s): round it yourself (leaf_values documents how it rounds)" % t.dtype)
    if t.shape != (2, 14, cells):
        raise ValueError("the leaf-value table must have shape [2, 14, %d] = [mine / theirs][piece][cell] (got %s)" % (cells, tuple(t.shape)))
    if t.size and (int(t.min()) < -32768 or int(t.max()) > 32767):
        bad = np.argwhere((t < -32768) | (t > 32767))[0]
        raise ValueError("table[%d][%d][%d] = %d is outside int16" % (bad[0], bad[1], bad[2], int(t[tuple(bad)])))
    return np.ascontiguousarray(t, dtype=np.int16)


def leaf_scale(limit, denom):
    """(limit, denom) of a leaf-value setting as ints; ValueError unless 1 <= limit <= denom <= 2^24."""
    limit, denom = int(limit), int(denom)
    if not 1 <= limit <= denom <= _lib.LEAF_MAX_DENOM:
        raise ValueError("1 <= limit <= denom <= 2^24 is required (got limit = %d, denom = %d)" % (limit, denom))
    return limit, denom


class BatchedStrategoProceduralEnv:
    def __init__(self, version, batch_size, device=0):
        self.variant = get_variant(version)
        v = self.variant
        if v.rows < 3 or v.columns < 3:
            raise ValueError("Both rows and columns have to be at least 3")                        # penv:28-30
        self.rows, self.columns = v.rows, v.columns
        self.batch_size = int(batch_size)
        self.action_size = v.action_size                                                            # penv:34
        self.spatial_action_size = v.spatial_action_size                                            # penv:35
        self._vec = VecStrategoEnv(v, batch_size, device=device, human_inits=False)
        self.device = self._vec.device
        self._held = None            # (states, players) objects held loaded by a `with env.loaded(...)` scope
        self._scratch_is_held = False
        self._held_exact = True      # False: the held states include ones the packed record cannot carry -> no reuse inside the scope
        self.strict = False          # True: ValueError when an import had to alter a state (sanitised)
        self.last_sanitised = torch.zeros((self.batch_size,), dtype=torch.uint8, device=self.device)
        self._obstacles = torch.from_numpy(v.obstacle_map().astype(np.int64)).to(self.device)

    # ---- helpers ---------------------------------------------------------------------------------------------
    def _players(self, players):
        p = torch.as_tensor(players).to(device=self.device, dtype=torch.int8).reshape(self.batch_size).contiguous()
        return p

    def _load(self, states, players):
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(st.shape) != (self.batch_size, NUM_STATE_LAYERS, self.rows, self.columns):
            raise ValueError("states must have shape (batch, 34, rows, columns)")
        pl = self._players(players)
        vec = self._vec
        if self._held is not None and self._scratch_is_held and states is self._held[0] and players is self._held[1]:
            return st, pl                                   # inside `with env.loaded(states, players)`: already in the scratch handle
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_import_state_checked(vec._h, st.data_ptr(), pl.data_ptr(), self.last_sanitised.data_ptr(),
                                                       vec._stream()), vec._L)
        self._scratch_is_held = self._held is not None and self._held_exact and states is self._held[0] and players is self._held[1]
        if self.strict and bool(self.last_sanitised.any()):
            raise ValueError("state is not one the packed record can carry (unreachable by play): see sgx_import_state_checked")
        return st, pl

    def _scratch_changed(self):
        """The scratch handle no longer holds the states of an enclosing `loaded` scope (a move was applied to it)."""
        self._scratch_is_held = False

    @contextlib.contextmanager
    def loaded(self, states, players):
        """Opt-in: import `states` once and let the calls inside the scope that are given the same tensor objects reuse the
        import.  The caller promises not to modify the tensors inside the scope (writes through other libraries or streams
        are invisible to this class); outside a scope every call imports.

        Results do not depend on the scope: if the import had to alter any of the states -- general (unreachable) states the packed
        record cannot carry -- nothing is reused and the calls inside the scope import like calls outside it, through sgx_step_states'
        general-state pass.  `last_sanitised` therefore means the same on both paths: what still had to be altered after every pass
        the call ran; `strict=True` raises on exactly that."""
        prev = (self._held, self._held_exact)
        self._held = (states, players)
        self._scratch_is_held = False
        self._held_exact = True
        try:
            strict, self.strict = self.strict, False
            try:
                self._load(states, players)
            finally:
                self.strict = strict
            if bool(self.last_sanitised.any()):              # one device -> host round trip per scope
                self._held_exact = False
                self._scratch_is_held = False
            yield self
        finally:
            self._held, self._held_exact = prev
            self._scratch_is_held = False

    def _in_loaded_scope(self, states, players):
        return self._held is not None and self._scratch_is_held and states is self._held[0] and players is self._held[1]

    def _step_states(self, states, players, actions, flags, export=False, mask_out=None, positions=False, out=None, obs_out=None, fobs_out=None):
        """sgx_step_states: import -> step (actions given) or observe (actions None) -> optional export, one library call (one
        launch on boards of more than 32 cells).  -> (new_states, new_players) or None."""
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(st.shape) != (self.batch_size, NUM_STATE_LAYERS, self.rows, self.columns):
            raise ValueError("states must have shape (batch, 34, rows, columns)")
        pl = self._players(players)
        vec = self._vec
        if out is not None:                                  # caller-provided successor tensors (benchmarks: same memory every call)
            new_states, new_players = out
        else:
            new_states = torch.empty_like(st) if export else None
            new_players = torch.empty((self.batch_size,), dtype=torch.int8, device=self.device) if export else None
        io = vec._fill_io(actions if actions is not None else vec.next_actions, False, False, False, flags)
        io.auto_reset = 0
        if actions is None:
            io.actions_dev = None
        io.mask_dev = mask_out.data_ptr() if mask_out is not None else None
        io.obs_dev = obs_out.data_ptr() if obs_out is not None else None
        io.fobs_dev = fobs_out.data_ptr() if fobs_out is not None else None
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_step_states(vec._h, st.data_ptr(), pl.data_ptr(), self.last_sanitised.data_ptr(), io,
                                              _ptr_or_none(new_states), _ptr_or_none(new_players), 2, vec._stream()), vec._L)
        vec._next_actions_fresh = False
        self._scratch_is_held = (actions is None and self._held is not None and self._held_exact and states is self._held[0] and players is self._held[1])
        if self.strict and bool(self.last_sanitised.any()):
            raise ValueError("state is not one the packed record can carry (unreachable by play): see sgx_import_state_checked")
        return (new_states, new_players) if export else None

    def _mask_in_state_coordinates(self, one_dim):
        """Mask of the loaded states' movers, indexed in the states' own coordinates (no perspective flip), rendered by the
        kernel: SGX_STEP_MASK_1D -> uint8 [N, action_size], SGX_STEP_MASK_STATE_COORDS -> uint8 [N, R, C, K]."""
        vec = self._vec
        shape = (self.batch_size, self.action_size) if one_dim else (self.batch_size,) + tuple(self.spatial_action_size)
        out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_observe(vec._h, None, None, out.data_ptr(), None,
                                          _lib.STEP_MASK_1D if one_dim else _lib.STEP_MASK_STATE_COORDS, vec._stream()), vec._L)
        return out

    # ---- state construction / transition -----------------------------------------------------------------------
    def create_initial_state(self, player_1_initial_piece_maps, player_2_initial_piece_maps):      # penv:38-60
        """own-side piece maps int [N,R,C] -> states (obstacle map and max_turns come from the variant)."""
        self._vec.reset(player_1_initial_piece_maps, player_2_initial_piece_maps)
        self._scratch_changed()
        st, _ = self._vec.export_state()
        return st

    def get_next_state(self, states, players, action_indices, allow_piece_oscillation=False):      # penv:148-155
        """-> (new_states, new_players int8, valid bool).  action_indices: absolute 1-D indices (impl:262-277)."""
        flags = _lib.STEP_ACTIONS_1D | (_lib.STEP_ALLOW_OSCILLATION if allow_piece_oscillation else 0)
        a = torch.as_tensor(action_indices).to(device=self.device, dtype=torch.int32).reshape(self.batch_size).contiguous()
        if self._held is not None and self._scratch_is_held and states is self._held[0] and players is self._held[1]:
            self._vec.step(a, emit_obs=False, emit_mask=False, flags=flags)          # inside `loaded`: the states are in the handle
            self._scratch_changed()
            new_states, new_players = self._vec.export_state()
            return new_states, new_players, self._vec.invalid_action == 0
        new_states, new_players = self._step_states(states, players, a, flags, export=True)
        return new_states, new_players, self._vec.invalid_action == 0

    def is_move_valid_by_1d_index(self, states, players, action_indices, allow_piece_oscillation=False):   # penv:94-99
        flags = _lib.STEP_ACTIONS_1D | (_lib.STEP_ALLOW_OSCILLATION if allow_piece_oscillation else 0)
        a = torch.as_tensor(action_indices).to(device=self.device, dtype=torch.int32).reshape(self.batch_size).contiguous()
        if self._in_loaded_scope(states, players):
            self._vec.step(a, emit_obs=False, emit_mask=False, flags=flags)
            self._scratch_changed()
        else:
            self._step_states(states, players, a, flags)
        return self._vec.invalid_action == 0

    def is_move_valid_by_position(self, states, players, start_r, start_c, end_r, end_c, allow_piece_oscillation=False):  # penv:87-92
        pos = torch.stack([torch.as_tensor(x).to(device=self.device, dtype=torch.int32).reshape(self.batch_size)
                           for x in (start_r, start_c, end_r, end_c)], dim=1).contiguous()
        flags = _lib.STEP_ACTIONS_POSITIONS | (_lib.STEP_ALLOW_OSCILLATION if allow_piece_oscillation else 0)
        if self._in_loaded_scope(states, players):
            self._vec.step(pos.view(-1), emit_obs=False, emit_mask=False, flags=flags)
            self._scratch_changed()
        else:
            self._step_states(states, players, pos.view(-1), flags)       # (one call: states the packed record cannot carry are redone exactly)
        return self._vec.invalid_action == 0

    # ---- masks ---------------------------------------------------------------------------------------------------
    def get_valid_moves_as_spatial_mask(self, states, players):                                     # penv:127-128
        """uint8 [N,R,C,K] in the coordinates of the given states (no perspective flip), like impl:399-517."""
        if not self._in_loaded_scope(states, players):
            out = torch.empty((self.batch_size,) + tuple(self.spatial_action_size), dtype=torch.uint8, device=self.device)
            self._step_states(states, players, None, _lib.STEP_MASK_STATE_COORDS, mask_out=out)
            return out
        return self._mask_in_state_coordinates(one_dim=False)

    def get_valid_moves_as_1d_mask(self, states, players, player_perspective=False):                # penv:74-80
        """uint8 [N, action_size] in the coordinates of the given states, like impl:520-642 (last element = no-op).
        player_perspective=True first flips the states of player -1 (penv:76-77) and then, like the reference, still
        asks for player -1's moves on the flipped state."""
        if player_perspective:
            states = self.get_state_from_player_perspective(states, players)
        if not self._in_loaded_scope(states, players):
            out = torch.empty((self.batch_size, self.action_size), dtype=torch.uint8, device=self.device)
            self._step_states(states, players, None, _lib.STEP_MASK_1D, mask_out=out)
            return out
        return self._mask_in_state_coordinates(one_dim=True)

    def get_dict_of_valid_moves_by_position(self, states, players):                                 # penv:82-85 / impl:1400-1429
        """One dict per state: "start_r,start_c" -> [[end_r, end_c], ...] in ascending 1-D index order."""
        masks = self.get_valid_moves_as_1d_mask(states, players).cpu().numpy()
        out = []
        for m in masks:
            d = {}
            for idx in np.flatnonzero(m):
                if idx == self.action_size - 1:                                                      # impl:355-367
                    raise ValueError("Action is a no-op so it doesn't translate to an actual action")
                sr, sc, er, ec = (int(x) for x in ia.positions_from_1d(self.rows, self.columns, int(idx)))
                d.setdefault("{},{}".format(sr, sc), []).append([er, ec])
            out.append(d)
        return out

    def get_serializable_string_for_fully_observable_state(self, states):                           # penv:175-177
        """pickle of the raw 33-channel observation from player 1's side, one bytes object per state."""
        from pickle import dumps
        obs = self.get_fully_observable_observation(states, np.ones(self.batch_size, dtype=np.int8)).cpu().numpy()
        return [dumps(np.ascontiguousarray(o)) for o in obs]

    def get_serializable_string_for_partially_observable_state(self, states):                       # penv:179-181
        from pickle import dumps
        obs = self.get_partially_observable_observation(states, np.ones(self.batch_size, dtype=np.int8)).cpu().numpy()
        return [dumps(np.ascontiguousarray(o)) for o in obs]

    @staticmethod
    def print_board_to_console(state, partially_observable=False, hide_still_piece_markers=True):  # penv:183-214
        """Text rendering of ONE state (int [34,R,C]): player 1's pieces as positive codes, player -1's (true or
        partially-observable layer) as negative codes, "R" for obstacles; row and column 0 at the bottom right."""
        st = state.cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
        _, rows, columns = st.shape
        enemy_layer = 4 if partially_observable else 1
        rule = "\n       " + "-" * (rows * 6 + 1)
        lines = ["    COL" + "".join("  {}  ".format(str(c).rjust(2)) for c in range(columns - 1, -1, -1)) + rule]
        for r in range(rows - 1, -1, -1):
            cells = []
            for c in range(columns - 1, -1, -1):
                item = ""
                if st[0, r, c] != 0:
                    item = str(st[0, r, c])
                elif st[enemy_layer, r, c] != 0:
                    item = str(-1 * st[enemy_layer, r, c])
                elif st[2, r, c] != 0:
                    item = "R"
                if not hide_still_piece_markers:
                    item += "a" if st[32, r, c] == 1 else ""
                    item += "b" if st[33, r, c] == 1 else ""
                cells.append(item.rjust(4) + " |")
            lines.append("Row {} |".format(str(r).rjust(2)) + "".join(cells) + rule)
        print("\n".join(lines))

    # ---- observations (raw, as the reference's operator layer returns them; maenv normalises afterwards) -----------
    def get_partially_observable_observation_extended_channels(self, states, players):             # penv:171-173
        return self._observe_raw(states, players, full=False, original=False)

    def get_fully_observable_observation_extended_channels(self, states, players):                 # penv:166-169
        return self._observe_raw(states, players, full=True, original=False)

    def _observe_raw(self, states, players, full, original):
        """One raw (un-normalised) observation kind into a fresh tensor; nothing else is rendered."""
        vec = self._vec
        if original:
            ch = _lib.FO_OBS_CHANNELS_ORIGINAL if full else _lib.PO_OBS_CHANNELS_ORIGINAL
        else:
            ch = _lib.FO_OBS_CHANNELS if full else _lib.PO_OBS_CHANNELS
        out = torch.empty((self.batch_size, self.rows, self.columns, ch), dtype=torch.float32, device=self.device)
        flags = _lib.STEP_RAW_OBS | (_lib.STEP_ORIGINAL_CHANNELS if original else 0)
        if not self._in_loaded_scope(states, players):
            # through sgx_step_states (observe): states the packed record cannot carry are redone exactly (every kind, boards <= 256 cells)
            self._step_states(states, players, None, flags, obs_out=None if full else out, fobs_out=out if full else None)
            return out
        self._load(states, players)
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_observe(vec._h, None if full else out.data_ptr(), out.data_ptr() if full else None, None, None,
                                          flags, vec._stream()), vec._L)
        return out

    def get_partially_observable_observation(self, states, players):                               # penv:162-164
        """Deprecated 32-channel observation holding piece values (impl:1153-1197), raw."""
        return self._observe_raw(states, players, full=False, original=True)

    def get_fully_observable_observation(self, states, players):                                   # penv:157-160
        """Deprecated 33-channel observation (impl:1075-1123), raw."""
        return self._observe_raw(states, players, full=True, original=True)

    # ---- pure tensor functions (no kernel needed) -------------------------------------------------------------------
    def get_state_from_player_perspective(self, states, players):                                   # penv:101-103 / impl:645-675
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64)
        pl = self._players(players)
        flipped = st.clone()
        f = st.flip(dims=(2, 3))
        flipped[:, _SWAP_A] = f[:, _SWAP_B]
        flipped[:, _SWAP_B] = f[:, _SWAP_A]
        flipped[:, 2] = f[:, 2]
        return torch.where((pl < 0).view(-1, 1, 1, 1), flipped, st)

    def get_game_ended(self, states, players):                                                      # penv:141-143 / impl:834-842
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64)
        pl = self._players(players).to(torch.float32)
        over, winner = st[:, 5, 0, 1] != 0, st[:, 5, 0, 2].to(torch.float32)
        val = torch.where(winner == 0, torch.full_like(winner, 1e-4), winner * pl)
        return torch.where(over, val, torch.zeros_like(val))

    def get_heuristic_rewards_from_move(self, states, players, action_indices, reward_matrix):     # impl:852-891
        """reward_matrix[moved own piece type, piece type on the destination] per state; 0 for the no-op.  Like the
        reference, the move is assumed valid (absolute 1-D indices, impl:262-277)."""
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64)
        pl = self._players(players)
        a = torch.as_tensor(action_indices).to(device=self.device, dtype=torch.int64).reshape(self.batch_size)
        rm = torch.as_tensor(reward_matrix).to(device=self.device, dtype=torch.float32)
        R, C = self.rows, self.columns
        noop = a == self.action_size - 1
        a = torch.where(noop, torch.zeros_like(a), a)
        start, k = a // (R + C), a % (R + C)                                                        # impl:350-383
        sr, sc = start // C, start % C
        er = torch.where(k < R, k, sr)
        ec = torch.where(k < R, sc, k - R)
        n = torch.arange(self.batch_size, device=self.device)
        own_layer = (pl < 0).to(torch.int64)                                                        # impl:172-174
        moved = st[n, own_layer, sr, sc]
        dest = st[n, 1 - own_layer, er, ec]
        return torch.where(noop, torch.zeros((), dtype=torch.float32, device=self.device), rm[moved, dest])

    def get_game_result_is_invalid(self, states):                                                   # penv:145-146 / impl:845-849
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64)
        return (st[:, 5, 0, 1] != 0) & (st[:, 5, 1, 1] != 0)

    # ---- index converters (batched numpy/torch-friendly; impl:262-396, 678-720) ------------------------------------------
    def get_action_1d_index_from_positions(self, sr, sc, er, ec):
        return ia.action_1d_from_positions(self.rows, self.columns, sr, sc, er, ec)

    def get_action_positions_from_1d_index(self, action_index):
        idx = np.asarray(action_index, dtype=np.int64)
        if np.any(idx == self.action_size - 1):
            raise ValueError("Action is a no-op so it doesn't translate to an actual action")     # impl:355-367
        return ia.positions_from_1d(self.rows, self.columns, idx)

    def get_action_1d_index_from_spatial_index(self, spatial_index):
        r, c, ch = spatial_index
        return ia.action_1d_from_spatial(self.rows, self.columns, r, c, ch)

    def get_action_spatial_index_from_positions(self, sr, sc, er, ec):
        r, c, ch = ia.spatial_from_positions(self.rows, self.columns, sr, sc, er, ec)
        if np.any(ch < 0):
            raise ValueError("diagonal or null move")                                              # impl:288-306
        return r, c, ch

    def get_action_positions_from_spatial_index(self, spatial_index):
        r, c, ch = spatial_index
        return ia.positions_from_spatial(self.rows, self.columns, r, c, ch)

    def get_action_positions_from_player_perspective(self, player, sr, sc, er, ec):
        if player == 1:
            return sr, sc, er, ec
        return ia.flip_positions(self.rows, self.columns, *(np.asarray(x, dtype=np.int64) for x in (sr, sc, er, ec)))

    def get_action_1d_index_from_player_perspective(self, action_index, player):
        return ia.action_1d_from_player_perspective(self.rows, self.columns, action_index, player)

    def get_action_spatial_index_from_1d_index(self, action_index):                                 # penv:135-139
        sr, sc, er, ec = self.get_action_positions_from_1d_index(action_index)
        return self.get_action_spatial_index_from_positions(sr, sc, er, ec)

    # ---- packed states: search nodes kept in the library's records (no int64 import / export per call) ---------------
    def new_packed(self, n=None, seed=0, env_id_offset=0):
        """An empty pool of `n` packed states of this variant (default: batch_size).  seed / env_id_offset key the pool's own random
        draws (PackedStates.determinize)."""
        return PackedStates(self.variant, self.batch_size if n is None else n, self.device, seed=seed, env_id_offset=env_id_offset)

    def pack(self, states, players, out=None):
        """int64 [n,34,R,C] + players -> PackedStates (`out` or a new pool); `sanitised` uint8 [n] reports altered states."""
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64).contiguous()
        out = out if out is not None else self.new_packed(st.shape[0])
        out._vec.import_state_checked(st, players, out.sanitised)
        if self.strict and bool(out.sanitised.any()):
            raise ValueError("state is not one the packed record can carry (unreachable by play)")
        return out

    def determinize(self, states, players, observer=0, draw=0, beliefs=None, return_off_belief=False, validate=True):
        """One sampled world per state for imperfect-information search: the hidden pieces of the observer's opponent dealt again
        (PackedStates.determinize: pack -> determinize into a scratch pool -> unpack, for callers on the reference layout).
        observer: 0 = each state's `players` entry, +1 / -1 = that player for all.  -> (states int64 [n,34,R,C], hidden int32 [n]);
        hidden[i] = -1 marks a state with a flag or a bomb on a moved hidden cell, returned unchanged.  beliefs / return_off_belief /
        validate: as PackedStates.determinize takes them (a [2, 12, cells] table for all states or one per state); with
        return_off_belief -> (states, hidden, off_belief).  No reference counterpart."""
        src = self.pack(states, players)
        try:
            dst = self.new_packed(src.n)
            try:
                if beliefs is not None or return_off_belief:
                    res = dst.determinize(src, observer=observer, draw=draw, beliefs=beliefs, return_off_belief=return_off_belief, validate=validate)
                    return (dst.unpack()[0],) + (tuple(res) if return_off_belief else (res,))
                hidden = dst.determinize(src, observer=observer, draw=draw)
                return dst.unpack()[0], hidden
            finally:
                dst.close()
        finally:
            src.close()

    def playout(self, states, players, max_steps=0, draw=0, return_states=False, weights=None, see_all=False):
        """Every state played to the end of its game with uniformly random valid moves (PackedStates.playout: pack -> playout into a scratch
        pool -> unpack when asked, for callers on the reference layout).  max_steps: 0 = to the end, else at most that many moves.
        weights / see_all: a [4, 13, 14] weight table for the moves instead of uniform draws, as PackedStates.playout takes it.
        -> PlayoutResult (reward [n,2], done, ending_invalid, player, length; value_for(player)); with return_states
        (result, final states int64 [n,34,R,C], their players int8 [n]).  No reference counterpart: the loop of
        examples/basic_game_loop.py run to dones['__all__'], as a function of a state."""
        src = self.pack(states, players)
        try:
            dst = self.new_packed(src.n)
            try:
                res = dst.playout(src, max_steps=max_steps, draw=draw, weights=weights, see_all=see_all)
                if not return_states:
                    return res
                final, final_players = dst.unpack()
                return res, final, final_players
            finally:
                dst.close()
        finally:
            src.close()

    def replay(self, states, players, actions, lengths=None, skip_invalid=False, actions_1d=True, allow_piece_oscillation=False, return_states=True,
               track_origins=False, origins_in=None):
        """Every state advanced by its list of actions, all moves in one launch (PackedStates.replay: pack -> replay into a scratch pool ->
        unpack, for callers on the reference layout).  actions: int32 [n, L]; absolute 1-D indices as get_next_state takes them
        (actions_1d=False: flat spatial indices in the mover's perspective); lengths: int32 [n] (None: L for all).
        -> (ReplayResult, states int64 [n,34,R,C], players int8 [n]); with return_states=False the ReplayResult alone.  The same as L calls
        of get_next_state that stop at the end of the game and -- unless skip_invalid -- at the first invalid action.
        track_origins / origins_in: as PackedStates.replay takes them; ReplayResult.origins then holds every piece's cell in `states`."""
        src = self.pack(states, players)
        try:
            dst = self.new_packed(src.n)
            try:
                res = dst.replay(src, actions, lengths=lengths, skip_invalid=skip_invalid, actions_1d=actions_1d,
                                 allow_piece_oscillation=allow_piece_oscillation, track_origins=track_origins, origins_in=origins_in)
                if not return_states:
                    return res
                final, final_players = dst.unpack()
                return res, final, final_players
            finally:
                dst.close()
        finally:
            src.close()

    def expand_all(self, states, players):
        """Every valid move of every state applied: all children of a batch of nodes (PackedStates.expand_all: pack -> count -> expand into a
        scratch pool of at most batch_size records, window after window -> unpack, for callers on the reference layout).
        -> (children int64 [M,34,R,C], child_players int8 [M], parent int32 [M], action_1d int32 [M]): child j is
        get_next_state(states[parent[j]], players[parent[j]], action_1d[j]); parents ascend, and the children of one parent come in the
        ascending order of the mover's perspective mask (PackedStates.expand_all), which for player -1 is the descending order of start
        cells in absolute coordinates.  Finished states and movers without a move have no child.  M is read from the device (one
        synchronisation)."""
        src = self.pack(states, players)
        try:
            _, offsets = src.count_moves()
            total = int(offsets[-1])
            cap = max(1, min(total, self.batch_size))
            dst = self.new_packed(cap)
            try:
                out = ([], [], [], [])
                for first in range(0, total, cap):
                    m = min(cap, total - first)
                    res = dst.expand_all(src, offsets=offsets, first_child=first, n=m, actions_1d=True)
                    st, pl = dst.unpack()
                    for lst, t in zip(out, (st, pl, res.parent, res.action)):
                        lst.append(t[:m])
                if not out[0]:
                    st, pl = dst.unpack()
                    return st[:0], pl[:0], torch.empty((0,), dtype=torch.int32, device=self.device), torch.empty((0,), dtype=torch.int32, device=self.device)
                return tuple(torch.cat(lst) for lst in out)
            finally:
                dst.close()
        finally:
            src.close()

    def state_keys(self, states, players, observer=None, clock=True, wide=False):
        """The position key of every state (PackedStates.state_keys: pack -> keys, for callers on the reference layout): int64 [n] ([n, 2]
        with wide) on the device.  observer=None: the state key, equal exactly when state and player are equal; 0 (each state's `players`
        entry) / +1 / -1: that player's information-set key; clock=False leaves turn count and max turns out.  The key is that of the state
        the packed record carries, so a state the import had to alter gets the key of what it was altered to.  Like the other one-call
        functions that go through `pack` (determinize, playout, replay, expand_all), and for any n: strict=True raises ValueError on such
        a state, and `last_sanitised` -- batch_size entries, written by the calls that import into the env's own handle -- is left
        alone; a caller who wants the flags without strict packs the states itself (`pack(...).sanitised`, then PackedStates.state_keys).
        No reference counterpart."""
        src = self.pack(states, players)
        try:
            return src.state_keys(observer=observer, clock=clock, wide=wide)
        finally:
            src.close()

    def evaluate(self, states, players, table, limit, denom, see_all=False):
        """The leaf values of every state by a piece-square table (PackedStates.set_leaf_values / evaluate: pack -> evaluate in place, for
        callers on the reference layout): float32 [n, 2] on the device = (v(+1), v(-1)) of a state that is not over, the final rewards of
        a finished one.  table / limit / denom / see_all: as PackedStates.set_leaf_values takes them.  No reference counterpart."""
        src = self.pack(states, players)
        try:
            return src.set_leaf_values(table, limit, denom, see_all=see_all).evaluate()
        finally:
            src.close()

    def close(self):
        self._vec.close()


class PlayoutResult:
    """What PackedStates.playout reports per slot (device tensors): reward float32 [n,2] = the final position's rewards of players +1 / -1
    (+-1 for a win, the reference's tie value, 0, 0 for a max-turn ending and for a playout cut off by max_steps -- with
    set_leaf_values on the pool a cut-off playout reports the leaf values of the position it reached instead), done uint8 (0 = cut off),
    ending_invalid uint8 (the max-turn tie), player int8 (the mover at the final position), length int32 (moves played)."""

    def __init__(self, reward, done, ending_invalid, player, length):
        self.reward, self.done, self.ending_invalid, self.player, self.length = reward, done, ending_invalid, player, length

    def value_for(self, player):
        """The reward column of `player` per slot: +1 / -1 for all, or an int8 tensor [n] of +-1 (a search wants the value from the root
        mover's side).  -> float32 [n]."""
        if isinstance(player, int):
            if player not in (1, -1):
                raise ValueError("player must be +1 or -1")
            return self.reward[:, 0 if player == 1 else 1]
        p = torch.as_tensor(player).to(device=self.reward.device).reshape(-1)
        return torch.where(p > 0, self.reward[:, 0], self.reward[:, 1])


class StepVsResult:
    """What step_vs reports per slot (device tensors), of the position the call reached: reward float32 [n,2], done uint8, ending_invalid
    uint8, player int8 (its mover) as for a playout; invalid_action uint8 (1 = the agent's action was refused: position unchanged, the bot
    stayed still), moved uint8 (bit 0: the agent moved, bit 1: the bot), reply_action int32 (the bot's move as a flat spatial index in
    the BOT's perspective -- what replay takes --, -1 = none)."""

    def __init__(self, reward, done, ending_invalid, player, invalid_action, moved, reply_action):
        self.reward, self.done, self.ending_invalid, self.player = reward, done, ending_invalid, player
        self.invalid_action, self.moved, self.reply_action = invalid_action, moved, reply_action

    @classmethod
    def empty(cls, n, device):
        u8 = lambda: torch.empty((n,), dtype=torch.uint8, device=device)
        return cls(torch.empty((n, 2), dtype=torch.float32, device=device), u8(), u8(), torch.empty((n,), dtype=torch.int8, device=device),
                   u8(), u8(), torch.empty((n,), dtype=torch.int32, device=device))

    value_for = PlayoutResult.value_for


class ReplayResult:
    """What replay reports per slot (device tensors): applied int32 (moves applied), consumed int32 (entries gone past, applied or
    skipped), stop uint8 (0 = the list was exhausted, 1 = the game was over, 2 = an invalid action: entry `consumed` is the offending one),
    and, of the final position as for a playout, reward float32 [n,2], done uint8, ending_invalid uint8, player int8.
    origins: int16 [n, 2, cells] of a replay with track_origins (the root cell -- or the given label -- of the piece of player index p on
    absolute cell c of the final position, -1 where it has none), else None."""

    def __init__(self, applied, consumed, stop, reward, done, ending_invalid, player, origins=None):
        self.applied, self.consumed, self.stop = applied, consumed, stop
        self.reward, self.done, self.ending_invalid, self.player = reward, done, ending_invalid, player
        self.origins = origins

    value_for = PlayoutResult.value_for


class ChildrenResult:
    """What PackedStates.expand_all reports per slot of its window (device tensors): parent int32 (the position of the child's root in the root
    list, -1 = no child in this slot), action int32 (the move that made the child, -1 = no child), and of the step that made the child
    reward float32 [n,2], done uint8, ending_invalid uint8, player int8 (the mover AT the child) -- these four are unwritten where parent is
    -1.  offsets int64 [n_roots + 1] are the roots' child numbers (count_moves) and total = offsets[n_roots] a device scalar: int(total) is
    the one synchronisation a caller may choose."""

    def __init__(self, parent, action, reward, done, ending_invalid, player, offsets, total):
        self.parent, self.action = parent, action
        self.reward, self.done, self.ending_invalid, self.player = reward, done, ending_invalid, player
        self.offsets, self.total = offsets, total

    value_for = PlayoutResult.value_for


class PackedStates:
    """A pool of n game states in the library's packed records (0.5 KB each for Barrage against 27 KB in the reference's int64
    layout), for tree-search callers of get_next_state (penv:148-155): nodes are expanded pool-to-pool with `expand`, copied with
    `copy_from`, and only converted to the reference layout when somebody wants to look at them (`unpack`)."""

    def __init__(self, version, n, device=0, seed=0, env_id_offset=0):
        # records only: no observation / mask tensors
        self._vec = VecStrategoEnv(version, n, device=device, seed=seed, env_id_offset=env_id_offset, human_inits=False, outputs=False)
        self.n = int(n)
        self.device = self._vec.device
        self.sanitised = torch.zeros((self.n,), dtype=torch.uint8, device=self.device)

    def unpack(self):
        """-> (states int64 [n,34,R,C], players int8 [n])."""
        return self._vec.export_state()

    def copy_from(self, src, src_index=None, dst_index=None, n=None):
        """records src[src_index[i]] -> self[dst_index[i]] (index tensors int32 on the device, None = identity).  `src`: a PackedStates or a
        live VecStrategoEnv of the same variant (a snapshot of start records)."""
        vec = self._vec
        src_vec = src._vec if isinstance(src, PackedStates) else src
        if src_vec is vec and (src_index is not None or dst_index is not None):
            raise ValueError("an indexed copy inside one pool would race (records read and rewritten by one launch): copy into another pool")
        si = None if src_index is None else torch.as_tensor(src_index).to(device=self.device, dtype=torch.int32).contiguous()
        di = None if dst_index is None else torch.as_tensor(dst_index).to(device=self.device, dtype=torch.int32).contiguous()
        if n is None:
            n = si.numel() if si is not None else di.numel() if di is not None else min(self.n, src_vec.num_envs)
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_copy_envs(vec._h, None if di is None else di.data_ptr(), src_vec._h,
                                            None if si is None else si.data_ptr(), int(n), vec._stream()), vec._L)
        return self

    def expand(self, parents, action_indices, parent_index=None, allow_piece_oscillation=False, mask_1d_out=None):
        """get_next_state for every slot i of this pool: self[i] = next_state(parents[parent_index[i]], action_indices[i])
        (absolute 1-D actions, impl:262-277).  -> (valid bool [n], players int8 [n] of the successors); where the move is invalid
        the slot holds a copy of the parent.  mask_1d_out: optional uint8 [n, action_size] receiving the successors'
        get_valid_moves_as_1d_mask in the same launch."""
        vec = self._vec
        if parents is self and parent_index is not None:
            raise ValueError("in-place expansion through parent_index would race (a parent may be overwritten before it is read): "
                             "expand into another pool")
        a = torch.as_tensor(action_indices).to(device=self.device, dtype=torch.int32).reshape(self.n).contiguous()
        pi = None if parent_index is None else torch.as_tensor(parent_index).to(device=self.device, dtype=torch.int32).reshape(self.n).contiguous()
        flags = _lib.STEP_ACTIONS_1D | (_lib.STEP_ALLOW_OSCILLATION if allow_piece_oscillation else 0)
        if mask_1d_out is not None:
            assert mask_1d_out.dtype == torch.uint8 and mask_1d_out.is_contiguous() and mask_1d_out.shape[0] == self.n
            flags |= _lib.STEP_MASK_1D
        io = vec._fill_io(a, False, False, False, flags)
        io.auto_reset = 0
        io.mask_dev = mask_1d_out.data_ptr() if mask_1d_out is not None else None
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_expand(vec._h, parents._vec._h, None if pi is None else pi.data_ptr(), io, vec._stream()), vec._L)
        vec._next_actions_fresh = False
        return vec.invalid_action == 0, vec.player

    def _belief_table(self, beliefs, n_src, validate):
        """beliefs of `determinize` -> (a contiguous 16-bit device tensor, the stride between two records' tables in elements: 0 = shared)."""
        v = self._vec.variant
        cells = v.rows * v.columns
        b = beliefs
        if isinstance(b, np.ndarray):
            b = torch.from_numpy(b.astype(np.int32) if b.dtype == np.uint16 else b)
        if not isinstance(b, torch.Tensor) or b.is_floating_point() or b.is_complex() or b.dtype == torch.bool:
            raise ValueError("beliefs must be an integer tensor (stratego_env_amd.beliefs builds tables and documents how it rounds)")
        b = b.to(self.device).contiguous()
        table = 2 * 12 * cells
        if tuple(b.shape) == (2, 12, cells):
            stride = 0
        elif tuple(b.shape) == (n_src, 2, 12, cells):
            stride = table
        else:
            raise ValueError("beliefs must have shape [2, 12, %d] (one table for all records) or [%d, 2, 12, %d] (one per record of src), got %s"
                             % (cells, n_src, cells, tuple(b.shape)))
        sixteen = (torch.int16,) + ((torch.uint16,) if hasattr(torch, 'uint16') else ())
        if validate:
            wide = b if b.dtype not in sixteen else b.view(torch.int16).to(torch.int32) & 0xFFFF
            if bool(((wide < 0) | (wide > _lib.BELIEF_WEIGHT_MAX)).any()):                  # (the one synchronisation)
                raise ValueError("beliefs must lie in [0, %d]" % _lib.BELIEF_WEIGHT_MAX)
        if b.dtype not in sixteen:
            b = b.to(torch.int16)                                   # (the low 16 bits: the library reads them as uint16)
        return b, stride

    def determinize(self, src, src_index=None, observer=0, draw=0, beliefs=None, return_off_belief=False, validate=True):
        """Sample a world the observer cannot tell from the real one into every slot i of this pool: self[i] = src[src_index[i]] with the
        hidden pieces of the observer's opponent (its pieces the public board shows as unknown) dealt again, uniformly over all assignments
        that keep the flag and the bombs on never-moved cells.  Everything else of the record -- and so the observer's partial observation and
        valid moves -- stays what it was.  `src`: a PackedStates (this pool itself for an in-place call without src_index) or a live
        VecStrategoEnv of the same variant; observer: 0 = each record's mover, +1 / -1 = that player for all; the shuffle is keyed by
        (this pool's seed, its env_id_offset + i, draw), so another `draw` gives independent worlds of the same roots.
        -> hidden int32 [n]: the number of hidden cells shuffled, -1 where a flag or a bomb sits on a moved hidden cell (play cannot produce
        that; the record is copied unchanged).  The worlds agree with the record's public layers, not with the full move history.
        beliefs: None = the uniform deal above (exactly the sgx_determinize call); else an integer device tensor [2, 12, cells] (one table
        for all records) or [src's n, 2, 12, cells] (the table of record src_index[i] for slot i), read as beliefs[owner's player index]
        [type - 1][absolute cell] with entries in [0, 4095] (stratego_env_amd.beliefs builds them): the hidden types are dealt instance by
        instance -- flags, bombs, then 10 .. 1 -- each onto a free hidden cell drawn with probability proportional to its weight for the
        type (sgx_determinize_weighted; the rule is in include/stratego_mi355x.h; another RNG stream, so other worlds than the uniform
        call's even for a constant table).  The range check costs one synchronisation: validate=False skips it (the library clamps
        entries to 4095), and a tensor that is int16 already is passed without a copy.  The weights steer the deal, they are not the
        marginals of the worlds.  return_off_belief (with beliefs): -> (hidden, off_belief int32 [n]), off_belief[i] = how many pieces
        of world i stand on a cell whose weight for their type is 0 (every candidate weighed 0 at that draw); 0 for a record copied unchanged."""
        vec = self._vec
        src_vec = src._vec if isinstance(src, PackedStates) else src
        if src_vec is vec and src_index is not None:
            raise ValueError("in-place determinization through src_index would race (a record may be overwritten before it is read): "
                             "determinize into another pool")
        if beliefs is None and return_off_belief:
            raise ValueError("off_belief counts draws outside a belief: pass beliefs")
        si = None if src_index is None else torch.as_tensor(src_index).to(device=self.device, dtype=torch.int32).reshape(self.n).contiguous()
        hidden = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        if beliefs is None:
            with torch.cuda.device(self.device):
                _lib.check(vec._L.sgx_determinize(vec._h, src_vec._h, None if si is None else si.data_ptr(), int(observer),
                                                  int(draw) & 0xFFFFFFFFFFFFFFFF, hidden.data_ptr(), vec._stream()), vec._L)
            vec._next_actions_fresh = False
            return hidden
        table, stride = self._belief_table(beliefs, src_vec.num_envs, validate)
        off = torch.empty((self.n,), dtype=torch.int32, device=self.device) if return_off_belief else None
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_determinize_weighted(vec._h, src_vec._h, None if si is None else si.data_ptr(), int(observer),
                                                       table.data_ptr(), stride, int(draw) & 0xFFFFFFFFFFFFFFFF, hidden.data_ptr(),
                                                       _ptr_or_none(off), vec._stream()), vec._L)
        vec._next_actions_fresh = False
        return (hidden, off) if return_off_belief else hidden

    def playout(self, src, src_index=None, max_steps=0, draw=0, weights=None, see_all=False):
        """Play src[src_index[i]] to the end of its game with uniformly random valid moves, for every slot i of this pool, in one launch
        (sgx_playout; the rule is in include/stratego_mi355x.h): self[i] becomes the final position, `src` stays what it was.  `src`: a
        PackedStates (this pool itself for an in-place call without src_index) or a live VecStrategoEnv of the same variant; max_steps: 0 =
        to the end, else at most that many moves; the moves are keyed by (this pool's seed, its env_id_offset + i, draw, the position's turn),
        so many slots of one root -- and another `draw` -- play different games.  -> PlayoutResult.
        weights: None = uniform (exactly the sgx_playout call); else a [4, 13, 14] array-like of integers in [0, 4095] (numpy or a CPU tensor,
        stratego_env_amd.playout_policies builds them): a move is drawn with probability proportional to weights[direction][moving piece]
        [what stands on the target cell] (sgx_playout_weighted, with the same key).  The target is what the mover's partial observation
        shows (0 = empty, 1..12 = a revealed type, 13 = unknown); see_all=True reads the opponent's true type instead (0..12), the usual
        choice inside a determinized world.  The table is read before the call returns."""
        vec = self._vec
        table = None if weights is None else playout_weights(weights)
        if table is None and see_all:
            raise ValueError("see_all chooses what a weight table is indexed with: pass weights")
        src_vec = src._vec if isinstance(src, PackedStates) else src
        if src_vec is vec and src_index is not None:
            raise ValueError("in-place playouts through src_index would race (a record may be overwritten before it is read): "
                             "play out into another pool")
        si = None if src_index is None else torch.as_tensor(src_index).to(device=self.device, dtype=torch.int32).reshape(self.n).contiguous()
        res = PlayoutResult(torch.empty((self.n, 2), dtype=torch.float32, device=self.device),
                            torch.empty((self.n,), dtype=torch.uint8, device=self.device),
                            torch.empty((self.n,), dtype=torch.uint8, device=self.device),
                            torch.empty((self.n,), dtype=torch.int8, device=self.device),
                            torch.empty((self.n,), dtype=torch.int32, device=self.device))
        io = _lib.SgxPlayoutIO(res.reward.data_ptr(), res.done.data_ptr(), res.ending_invalid.data_ptr(), res.player.data_ptr(),
                               res.length.data_ptr(), int(max_steps), 0)
        with torch.cuda.device(self.device):
            if table is None:
                _lib.check(vec._L.sgx_playout(vec._h, src_vec._h, None if si is None else si.data_ptr(), io, int(draw) & 0xFFFFFFFFFFFFFFFF,
                                              vec._stream()), vec._L)
            else:
                _lib.check(vec._L.sgx_playout_weighted(vec._h, src_vec._h, None if si is None else si.data_ptr(), io,
                                                       table.ctypes.data_as(C.POINTER(C.c_uint16)), _lib.PLAYOUT_SEE_ALL if see_all else 0,
                                                       int(draw) & 0xFFFFFFFFFFFFFFFF, vec._stream()), vec._L)
        vec._next_actions_fresh = False
        return res

    def step_vs(self, src, actions, agent, weights, see_all=False, draw=0, src_index=None):
        """self[i] = src[src_index[i]] after the agent's move actions[i] and the reply of the table bot `weights`, both in one launch
        (sgx_step_vs; the rule is in include/stratego_mi355x.h); `src` stays what it was.  `src`: a PackedStates (this pool itself for an
        in-place call without src_index) or a live VecStrategoEnv of the same variant.  actions: int32 [n] flat spatial indices in the
        mover's perspective, or None (the bot opens where it is to move); agent: +1 / -1 or an int8 tensor [n]; weights, see_all: as
        playout takes them, for the bot; draw: the key of the replies.  -> StepVsResult.  (VecStrategoEnv.step_vs is the same call
        with a live env as the destination.)"""
        return self._vec.step_vs(actions, agent, weights, see_all=see_all, draw=draw, src=src, src_index=src_index)

    def replay(self, src, actions, lengths=None, src_index=None, skip_invalid=False, actions_1d=False, allow_piece_oscillation=False,
               track_origins=False, origins_in=None):
        """self[i] = src[src_index[i]] advanced by the list actions[i, :lengths[i]], every move in one launch (sgx_replay; the rule is in
        include/stratego_mi355x.h); `src` stays what it was.  `src`: a PackedStates (this pool itself for an in-place call without
        src_index) or a live VecStrategoEnv of the same variant.  actions: int32 device tensor [n, L] with any non-negative strides, taken
        as it is (the transposed [T, N] action log of a trajectory needs no copy); lengths int32 [n] (None: L for all).  skip_invalid: an
        invalid entry is passed over, else it ends the replay (stop == 2); actions_1d: absolute 1-D indices as `expand` takes them, else
        flat spatial indices in the mover's perspective as env.step() takes them.  -> ReplayResult.  (VecStrategoEnv.replay is the same
        call with a live env as the destination.)
        track_origins: ReplayResult.origins = int16 [n, 2, cells], the cell in `src` of every piece of the final position (-1 on cells
        without one): piece identity, which the record does not carry -- beliefs.follow turns a setup prior into per-record belief tables
        with it.  origins_in: int16 device tensor [src's n, 2, cells], labels the roots already carry (an earlier replay's origins, to
        chain two replays; or any piece ids), carried verbatim."""
        return self._vec.replay(src, actions, lengths=lengths, src_index=src_index, skip_invalid=skip_invalid, actions_1d=actions_1d,
                                allow_piece_oscillation=allow_piece_oscillation, track_origins=track_origins, origins_in=origins_in)

    def count_moves(self, index=None):
        """-> (counts int32 [n], offsets int64 [n + 1]): the valid moves of record index[i] (None: every record in order) and their exclusive
        scan, on the device without a synchronisation (VecStrategoEnv.count_moves)."""
        return self._vec.count_moves(index)

    def state_keys(self, index=None, observer=None, clock=True, wide=False):
        """-> int64 [n] ([n, 2] with wide): the position key of record index[i] (None: every record in order), on the device without a
        synchronisation -- the state key (observer=None) or the information-set key of observer 0 (each record's mover) / +1 / -1; clock=False
        leaves turn count and max turns out (VecStrategoEnv.state_keys)."""
        return self._vec.state_keys(index, observer=observer, clock=clock, wide=wide)

    def expand_all(self, src, src_index=None, offsets=None, first_child=0, n=None, actions_1d=False):
        """All children of the roots src[src_index[i]] (None: every record of src in order), no action list needed: slot j of this pool
        becomes child first_child + j of the list of all children -- roots in order, each root's moves in the ascending flat order of its
        mover's perspective mask -- in one launch (sgx_expand_all; the rule is in include/stratego_mi355x.h).  `src`: another PackedStates or
        a live VecStrategoEnv of the same variant, only read.  offsets: what count_moves(src_index) of `src` returned (None: counted here);
        n: the slots of this call's window (None: the whole pool) -- a level with more children than the pool is walked with first_child =
        0, n, 2n, ...; slots past the last child keep their records and report parent = action = -1.  actions_1d: `action` holds absolute
        1-D indices as `expand` takes them instead of flat spatial indices in the mover's perspective as env.step() takes them (the order of
        the children is the same).  -> ChildrenResult (no synchronisation; int(res.total) is the caller's)."""
        vec = self._vec
        src_vec = src._vec if isinstance(src, PackedStates) else src
        if src_vec is vec:
            raise ValueError("expand_all inside one pool would overwrite roots with children: expand into another pool")
        dev = self.device
        si = None if src_index is None else torch.as_tensor(src_index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        n_roots = src_vec.num_envs if si is None else int(si.numel())
        if offsets is None:
            offsets = src_vec.count_moves(si)[1]
        elif not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.device != dev or not offsets.is_contiguous() \
                or offsets.numel() != n_roots + 1:
            raise ValueError("offsets must be the contiguous int64 device tensor [%d] that count_moves returned for these roots" % (n_roots + 1))
        n = self.n if n is None else int(n)
        m = max(n, 0)
        res = ChildrenResult(torch.empty((m,), dtype=torch.int32, device=dev), torch.empty((m,), dtype=torch.int32, device=dev),
                             torch.empty((m, 2), dtype=torch.float32, device=dev), torch.empty((m,), dtype=torch.uint8, device=dev),
                             torch.empty((m,), dtype=torch.uint8, device=dev), torch.empty((m,), dtype=torch.int8, device=dev),
                             offsets, offsets[n_roots])
        p = (lambda t: t.data_ptr()) if m else (lambda t: None)
        io = _lib.SgxChildrenIO(offsets.data_ptr(), p(res.parent), p(res.action), p(res.reward), p(res.done), p(res.ending_invalid), p(res.player),
                                n_roots, int(first_child), n, _lib.CHILDREN_ACTIONS_1D if actions_1d else 0, 0)
        with torch.cuda.device(dev):
            _lib.check(vec._L.sgx_expand_all(vec._h, src_vec._h, None if si is None or n_roots == 0 else si.data_ptr(), io, vec._stream()), vec._L)
        vec._next_actions_fresh = False
        return res

    def set_leaf_values(self, table, limit, denom, see_all=False):
        """Leaf values for the calls this pool is the DESTINATION of (sgx_set_leaf_values; the rule is in include/stratego_mi355x.h):
        playout, replay and expand_all then report, for every slot whose position is not over, reward = (v(+1), v(-1)) instead of 0, 0,
        with v(p) = clamp(mine(p) - theirs(p), -limit, limit) / denom.  table: an integer array-like [2, 14, cells] within int16
        (stratego_env_amd.leaf_values builds them): table[0][t][cell] is the worth of an own piece of type t (1..12) on `cell` of its
        owner's perspective, table[1][d][cell] the worth of an opponent's piece shown as d (1..12 revealed, 13 unknown; see_all=True:
        its true type) on `cell` of that opponent's perspective.  1 <= limit <= denom <= 2^24.  Shape and range are checked on the host;
        the call waits for the device once (launches in flight keep the table they started with).  The table is a setting of this pool,
        not part of its records: copies and snapshots do not carry it."""
        vec = self._vec
        t = leaf_table(table, vec.variant.rows * vec.variant.columns)
        limit, denom = leaf_scale(limit, denom)
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_set_leaf_values(vec._h, t.ctypes.data_as(C.c_void_p), limit, denom, _lib.LEAF_SEE_ALL if see_all else 0), vec._L)
        return self

    def clear_leaf_values(self):
        """Positions that are not over report 0, 0 again (waits for the device if a table was set)."""
        vec = self._vec
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_set_leaf_values(vec._h, None, 0, 0, 0), vec._L)
        return self

    @property
    def leaf_values_set(self):
        return bool(self._vec._L.sgx_leaf_values_set(self._vec._h))

    def evaluate(self, src=None, src_index=None):
        """The leaf values of src[src_index[i]] (None: of this pool's own records, in place) by this pool's table: float32 [n, 2] on the
        device, (v(+1), v(-1)) for a position that is not over and the final rewards for a finished one.  It is the replay of an empty
        list (max_len = 0): with another pool as `src` the records are copied here on the way.  Raises if no table is set."""
        if not self.leaf_values_set:
            raise ValueError("evaluate needs leaf values: call set_leaf_values first")
        empty = torch.empty((self.n, 0), dtype=torch.int32, device=self.device)
        return self._vec.replay(self if src is None else src, empty, src_index=src_index).reward

    @property
    def last_launch_kind(self):
        return self._vec.last_launch_kind

    def valid_moves_as_1d_mask(self):
        out = torch.empty((self.n, self._vec.variant.action_size), dtype=torch.uint8, device=self.device)
        vec = self._vec
        with torch.cuda.device(self.device):
            _lib.check(vec._L.sgx_observe(vec._h, None, None, out.data_ptr(), None, _lib.STEP_MASK_1D, vec._stream()), vec._L)
        return out

    def close(self):
        self._vec.close()


class _LateBound:
    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        owner = self._owner
        attr = getattr(owner._current(), name)
        if not callable(attr):
            return attr
        return lambda *a, **k: getattr(owner._current(), name)(*a, **k)


def _variant_obstacles(version):
    return get_variant(version).obstacle_map() != 0


def _default_variant(rows, columns, obstacle_map=None):
    """The reference's StrategoProceduralEnv is built from (rows, columns) only.  For a board size one of the reference's variants
    has, that variant with the most pieces (its capture-event capacity covers the others), else a custom variant of that size;
    the obstacle cells are the caller's (they are a per-handle constant here, taken from the first state / obstacle map seen)."""
    import dataclasses
    from .config import VARIANTS, custom_variant
    cands = [v for v in VARIANTS.values() if v.rows == rows and v.columns == columns]
    v = max(cands, key=lambda v: sum(v.piece_counts)) if cands else custom_variant(rows, columns)
    if obstacle_map is not None:
        obst = tuple((int(r), int(c)) for r, c in zip(*np.nonzero(np.asarray(obstacle_map))))
        if obst != tuple(sorted(v.obstacle_locations)):
            v = dataclasses.replace(v, name='%s_obstacles_%x' % (v.name, hash(obst) & 0xFFFFFFFF), obstacle_locations=obst, human_inits='')
    return v


class StrategoProceduralEnv:
    """The reference class of the same name (penv:20-214) for ONE state at a time: same constructor, method names,
    argument meaning, return types (numpy int64 states and masks, float32 observations, Python scalars) and errors.  It is
    what `StrategoMultiAgentEnv.base_env` is; every call runs the HIP kernels through a one-game
    BatchedStrategoProceduralEnv (use that class directly for throughput)."""

    def __init__(self, rows, columns, version=None, device=0):
        if rows < 3 or columns < 3:
            raise ValueError("Both rows and columns have to be at least 3 (you passed rows: {} columns: {})."
                             .format(rows, columns))                                                # penv:28-30
        self.rows, self.columns = np.int64(rows), np.int64(columns)
        self.action_size = np.int64(ia.action_size(int(rows), int(columns)))                        # penv:34
        k = ia.spatial_channels(int(rows), int(columns))
        self.spatial_action_size = (np.int64(rows), np.int64(columns), np.int64(k))                 # penv:35
        if int(rows) * int(columns) > 256:
            raise ValueError("boards of more than 256 cells are not supported ({} x {})".format(rows, columns))
        self._version = version
        self._device = device
        self._by_obstacles = {}      # obstacle map bytes -> one-state batched env (obstacles are a per-handle constant)
        self._batched = None

    def _for_obstacles(self, obstacle_map):
        """The one-state batched env whose handle carries these obstacle cells (the reference reads them from every state)."""
        ob = np.ascontiguousarray(np.asarray(obstacle_map) != 0)
        key = ob.tobytes()
        b = self._by_obstacles.get(key)
        if b is None:
            v = self._version if self._version is not None else _default_variant(int(self.rows), int(self.columns), ob)
            b = BatchedStrategoProceduralEnv(v, 1, device=self._device)
            b.strict = True          # a state the packed record cannot carry is an error here, never silently altered
            self._by_obstacles[key] = b
        self._batched = b
        return b

    @property
    def _b(self):
        """The one-state env the call goes to.  Methods are written `self._b.method(self._state(state), ...)`: Python evaluates
        `self._b` BEFORE the arguments, and `_state()` is what selects the env (by the state's obstacle layer) -- so this returns
        a proxy that picks the env when the method is finally called."""
        return _LateBound(self)

    def _current(self):
        if self._batched is None:
            self._for_obstacles(np.zeros((int(self.rows), int(self.columns)), dtype=bool) if self._version is None
                                else _variant_obstacles(self._version))
        return self._batched

    def _state(self, state):
        st = np.asarray(state, dtype=np.int64)
        if st.shape != (NUM_STATE_LAYERS, int(self.rows), int(self.columns)):
            raise ValueError("state must have shape (34, rows, columns)")
        if self._version is None:
            self._for_obstacles(st[2])
        if not np.array_equal(st[2] != 0, self._b.variant.obstacle_map() != 0):
            raise ValueError("the state's obstacle layer differs from the %s variant's (a per-handle constant here)" % self._version)
        return st[None]

    @staticmethod
    def _pl(player):
        return np.asarray([int(player)], dtype=np.int8)

    # ---- state construction / transition ---------------------------------------------------------------------------
    def create_initial_state(self, obstacle_map, player_1_initial_piece_map, player_2_initial_piece_map, max_turns):
        correct_shape = (int(self.rows), int(self.columns))
        for name, m in (("obstacle map", obstacle_map), ("player_1_initial_piece_map map", player_1_initial_piece_map),
                        ("player_2_initial_piece_map map", player_2_initial_piece_map)):
            if tuple(np.shape(m)) != correct_shape:
                raise ValueError("{} needs to be of shape {}, was {}".format(name, correct_shape, np.shape(m)))   # penv:44-55
        if self._version is None:
            self._for_obstacles(obstacle_map)
        elif not np.array_equal(np.asarray(obstacle_map) != 0, self._b.variant.obstacle_map() != 0):
            raise ValueError("obstacle_map differs from the %s variant's (a per-handle constant here)" % self._version)
        st = self._b.create_initial_state(np.asarray(player_1_initial_piece_map, dtype=np.int8)[None],
                                          np.asarray(player_2_initial_piece_map, dtype=np.int8)[None])[0].cpu().numpy()
        st[5, 1, 0] = int(max_turns)                                                                # StateData.MAX_TURNS (impl:247)
        return st

    def get_next_state(self, state, player, action_index, allow_piece_oscillation=False):          # penv:148-155
        ns, _, ok = self._b.get_next_state(self._state(state), self._pl(player), np.asarray([int(action_index)], dtype=np.int64),
                                           allow_piece_oscillation=allow_piece_oscillation)
        if not bool(ok[0]):
            raise ValueError("Couldn't get the next state because the move wasn't valid.")          # impl:902
        return ns[0].cpu().numpy(), player * -1

    def is_move_valid_by_position(self, state, player, start_r, start_c, end_r, end_c, allow_piece_oscillation=False):
        return bool(self._b.is_move_valid_by_position(self._state(state), self._pl(player), [int(start_r)], [int(start_c)],
                                                      [int(end_r)], [int(end_c)], allow_piece_oscillation)[0])

    def is_move_valid_by_1d_index(self, state, player, action_index, allow_piece_oscillation=False):
        return bool(self._b.is_move_valid_by_1d_index(self._state(state), self._pl(player), [int(action_index)],
                                                      allow_piece_oscillation)[0])

    # ---- masks -------------------------------------------------------------------------------------------------------
    def get_valid_moves_as_1d_mask(self, state, player, player_perspective=False):                  # penv:74-80
        m = self._b.get_valid_moves_as_1d_mask(self._state(state), self._pl(player), player_perspective=player_perspective)
        return m[0].cpu().numpy().astype(np.int64)

    def get_valid_moves_as_spatial_mask(self, state, player):                                       # penv:127-128
        return self._b.get_valid_moves_as_spatial_mask(self._state(state), self._pl(player))[0].cpu().numpy().astype(np.int64)

    def get_dict_of_valid_moves_by_position(self, state, player):                                   # penv:82-85
        return self._b.get_dict_of_valid_moves_by_position(self._state(state), self._pl(player))[0]

    # ---- observations (raw) --------------------------------------------------------------------------------------------
    def get_fully_observable_observation(self, state, player):                                      # penv:157-160
        return self._b.get_fully_observable_observation(self._state(state), self._pl(player))[0].cpu().numpy()

    def get_partially_observable_observation(self, state, player):                                  # penv:162-164
        return self._b.get_partially_observable_observation(self._state(state), self._pl(player))[0].cpu().numpy()

    def get_fully_observable_observation_extended_channels(self, state, player):                    # penv:166-169
        return self._b.get_fully_observable_observation_extended_channels(self._state(state), self._pl(player))[0].cpu().numpy()

    def get_partially_observable_observation_extended_channels(self, state, player):                # penv:171-173
        return self._b.get_partially_observable_observation_extended_channels(self._state(state), self._pl(player))[0].cpu().numpy()

    def get_serializable_string_for_fully_observable_state(self, state):                            # penv:175-177
        return self._b.get_serializable_string_for_fully_observable_state(self._state(state))[0]

    def get_serializable_string_for_partially_observable_state(self, state):                        # penv:179-181
        return self._b.get_serializable_string_for_partially_observable_state(self._state(state))[0]

    def print_board_to_console(self, state, partially_observable=False, hide_still_piece_markers=True):   # penv:183-214
        BatchedStrategoProceduralEnv.print_board_to_console(state, partially_observable, hide_still_piece_markers)

    # ---- state algebra -------------------------------------------------------------------------------------------------
    def get_state_from_player_perspective(self, state, player):                                     # penv:101-103
        st = np.asarray(state, dtype=np.int64)
        return self._b.get_state_from_player_perspective(st[None], self._pl(player))[0].cpu().numpy()

    def get_game_ended(self, state, player):                                                        # penv:141-143
        return np.float32(self._b.get_game_ended(np.asarray(state, dtype=np.int64)[None], self._pl(player))[0].item())

    def get_game_result_is_invalid(self, state):                                                    # penv:145-146
        return bool(self._b.get_game_result_is_invalid(np.asarray(state, dtype=np.int64)[None])[0])

    # ---- index converters (scalars, like the reference) ---------------------------------------------------------------
    def get_action_1d_index_from_positions(self, start_r, start_c, end_r, end_c):                   # penv:62-66
        return np.int64(self._b.get_action_1d_index_from_positions(int(start_r), int(start_c), int(end_r), int(end_c)))

    def get_action_positions_from_1d_index(self, action_index):                                     # penv:68-72
        return tuple(np.int64(x) for x in self._b.get_action_positions_from_1d_index(int(action_index)))

    def get_action_positions_from_player_perspective(self, player, start_r, start_c, end_r, end_c):   # penv:105-108
        return tuple(np.int64(x) for x in self._b.get_action_positions_from_player_perspective(
            int(player), int(start_r), int(start_c), int(end_r), int(end_c)))

    def get_action_1d_index_from_player_perspective(self, action_index, player):                    # penv:110-115
        return np.int64(self._b.get_action_1d_index_from_player_perspective(int(action_index), int(player)))

    def get_action_spatial_index_from_positions(self, start_r, start_c, end_r, end_c):              # penv:117-121
        return tuple(np.int64(x) for x in self._b.get_action_spatial_index_from_positions(int(start_r), int(start_c),
                                                                                          int(end_r), int(end_c)))

    def get_action_positions_from_spatial_index(self, spatial_index):                               # penv:123-125
        r, c, ch = (int(x) for x in spatial_index)
        return tuple(np.int64(x) for x in self._b.get_action_positions_from_spatial_index((r, c, ch)))

    def get_action_1d_index_from_spatial_index(self, spatial_index):                                # penv:130-133
        r, c, ch = (int(x) for x in spatial_index)
        return np.int64(self._b.get_action_1d_index_from_spatial_index((r, c, ch)))

    def get_action_spatial_index_from_1d_index(self, action_index):                                 # penv:135-139
        return tuple(np.int64(x) for x in self._b.get_action_spatial_index_from_1d_index(int(action_index)))

    def close(self):
        for b in self._by_obstacles.values():
            b.close()
        self._by_obstacles = {}
        self._batched = None
