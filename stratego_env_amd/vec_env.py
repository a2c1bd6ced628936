"""VecStrategoEnv: N concurrent games on one MI355X, torch tensors in / out.

The batched counterpart of StrategoMultiAgentEnv (reference stratego_multiagent_env.py:316-834): every
call goes through the C ABI in include/stratego_mi355x.h to the HIP kernels; PyTorch only owns the device
buffers and the stream.  Outputs are written in place into preallocated tensors:

    obs      float32 [N, R, C, 67]   normalised partial observation of each env's next mover
    fobs     float32 [N, R, C, 79]   normalised fully-observable observation (only with full_obs=True)
                                     (32 / 33 channels with obs_channel_mode='original')
    mask     uint8   [N, R, C, K]    valid-actions mask of the next mover (flat index = action)
    reward   float32 [N, 2]          rewards of player +1 / -1 (non-zero only when done)
    done     uint8   [N]
    player   int8    [N]             next mover (+1 / -1)
    invalid_action uint8 [N]         the reference would have raised ValueError; env unchanged
    ending_invalid uint8 [N]         game ended by max_turns ('game_result_was_invalid')

There is no CPU fallback: construction fails if the HIP library is missing or no GPU is visible.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

from . import _lib
from .config import (FO_OBS_CHANNELS, FO_OBS_CHANNELS_ORIGINAL, PO_OBS_CHANNELS, PO_OBS_CHANNELS_ORIGINAL, NUM_STATE_LAYERS,
                     get_variant)
from .setups import load_setup_table


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def check_choose_tensors(num_envs, n_actions, mask_words, device, mask, out):
    """What choose_actions() requires of `mask` and `out` before their addresses go to the library, on plain descriptions so that it
    needs no handle: mask / out = (dtype, device, numel, is_contiguous).  mask: uint8 / bool bytes [N, NA] or int32 words
    [N, mask_words] (the bit mask of a compact step); out: int32 [N]; both contiguous and on `device`.  -> True for a bit mask;
    ValueError otherwise."""
    for what, (dtype, dev, numel, contiguous) in (('mask', mask), ('out', out)):
        if dev != device:
            raise ValueError("choose_actions: %s is on %s, the env on %s" % (what, dev, device))
        if not contiguous:
            raise ValueError("choose_actions: %s must be contiguous" % what)
    bits = mask[0] == torch.int32
    if not bits and mask[0] not in (torch.uint8, torch.bool):
        raise ValueError("choose_actions: mask must be uint8 / bool bytes or the int32 bit mask of a compact step, not %s" % (mask[0],))
    want = num_envs * (mask_words if bits else n_actions)
    if mask[2] != want:
        raise ValueError("choose_actions: mask holds %d elements, num_envs x %s is %d"
                         % (mask[2], 'compact_mask_words' if bits else 'rows x columns x ways_to_move', want))
    if out[0] != torch.int32:
        raise ValueError("choose_actions: out must be int32, not %s" % (out[0],))
    if out[2] != num_envs:
        raise ValueError("choose_actions: out holds %d entries for %d envs" % (out[2], num_envs))
    return bits


class _OutputsOwner:
    """One sgx_alloc_outputs allocation.  It is freed when the LAST reference goes: the env holds one, and so does every tensor
    that views the buffers (torch keeps the object behind __cuda_array_interface__ alive as long as the tensor's storage), so a
    tensor handed out by step() / rollout_steps() / observe() stays valid after env.close(), `del env` or another
    tune_placement() -- like the torch-owned buffers it replaces."""

    def __init__(self, lib, out):
        self._L, self.out = lib, out

    def __del__(self):
        # Runs wherever the garbage collector drops the last tensor.  sgx_free_outputs selects the buffers' device for the free and
        # puts the calling thread's device back (DeviceGuard); at interpreter shutdown the HIP runtime may already be gone and the
        # process's memory is released anyway: nothing to do then.
        # (module globals may already be None at shutdown, and an import here would raise: everything inside the try)
        try:
            if sys is None or sys.is_finalizing():
                return
            self._L.sgx_free_outputs(None, C.byref(self.out))      # (works without the handle: the record names its device)
        except Exception:
            pass


class _DeviceBuffer:
    """A library-owned device allocation seen through __cuda_array_interface__ (zero-copy into a torch tensor)."""

    def __init__(self, ptr, shape, typestr, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2,
                                         'strides': None}


def _wrap_device(ptr, shape, dtype, device, owner):
    typestr = {torch.float32: '<f4', torch.uint8: '|u1'}[dtype]
    t = torch.as_tensor(_DeviceBuffer(ptr, shape, typestr, owner), device=device)
    assert t.data_ptr() == int(ptr) and t.dtype == dtype
    return t


class VecStrategoEnv:
    def __init__(self, version='barrage', num_envs=1, device=0, seed=0, env_id_offset=0, human_inits=None,
                 auto_reset=False, final_obs=False, full_obs=False, lib_path=None, obs_channel_mode='extended', compact_outputs=False,
                 outputs=True, placement=None):
        """human_inits: None = use the Gravon table when the variant has one (util.py:301-319), False = uniformly
        random back-row placement (util.py:33-53), True = require the table.
        obs_channel_mode: 'extended' (67 / 79 one-hot channels) or 'original' (the deprecated 32 / 33 value channels,
        maenv:67, 368-375).
        outputs=False: a pool of game records without observation / mask tensors (`obs`, `mask`, `fobs` are None): what
        snapshot() and the packed search pools of procedural_env hold -- 0.5 KB per Barrage game instead of 31 KB.
        placement: 'search' (default) = the first reset() of all envs moves obs / mask / fobs into library-owned buffers picked by the bounded
        placement search (tune_placement(): ~10 ms, at most min(8 GiB, a quarter of the free device memory) held beyond the buffers for a
        moment; which physical memory an allocation gets decides 0.76-0.93 against 0.95-1.04 of the roofline) -- only
        where there are placement classes (observations of more than 300 MB, not compact); 'plain' = torch.empty tensors, always.  None =
        the environment variable SGX_PLACEMENT, else 'search'.  (Use the tensors reset() / step() RETURN, or env.obs / env.mask read
        after the first reset(): that reset may replace the ones allocated here.)"""
        if obs_channel_mode not in ('extended', 'original'):
            raise ValueError("obs_channel_mode must be 'extended' or 'original'")
        placement = placement if placement is not None else (os.environ.get('SGX_PLACEMENT') or 'search')
        if placement not in ('plain', 'search'):
            raise ValueError("placement must be 'plain' or 'search' (SGX_PLACEMENT=%r)" % placement)
        self._placement_pending = placement == 'search'
        self.placement_report = None         # what the search of placement='search' saw (tune_placement's report)
        # compact_outputs=True (opt-in): `obs` is uint8 [N, compact_obs_stride] -- the 4-bit codes the float32 observation decodes from --
        # and `mask` int32 [N, compact_mask_words] -- one bit per action: 1/8 of the bytes per step.  decode_obs() / decode_mask() give the
        # contract tensors, byte-identical to a non-compact step (include/stratego_mi355x.h: SGX_STEP_COMPACT_OBS).
        self.compact = bool(compact_outputs)
        if self.compact and (final_obs or full_obs or obs_channel_mode != 'extended'):
            raise ValueError("compact_outputs comes with the 67-channel partial observation only (no final_obs / full_obs / original channels)")
        self.obs_channel_mode = obs_channel_mode
        self._mode_flags = _lib.STEP_ORIGINAL_CHANNELS if obs_channel_mode == 'original' else 0
        if compact_outputs:
            self._mode_flags |= _lib.STEP_COMPACT_OBS | _lib.STEP_COMPACT_MASK
        self.p_channels = PO_OBS_CHANNELS_ORIGINAL if obs_channel_mode == 'original' else PO_OBS_CHANNELS
        self.f_channels = FO_OBS_CHANNELS_ORIGINAL if obs_channel_mode == 'original' else FO_OBS_CHANNELS
        if not torch.cuda.is_available():
            raise _lib.SgxError("VecStrategoEnv needs a HIP device (torch.cuda.is_available() is False); no CPU fallback")
        self.variant = get_variant(version)
        v = self.variant
        self._L = _lib.load_for_geometry(v.rows, v.columns, lib_path)
        self.num_envs = int(num_envs)
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.env_id_offset = int(env_id_offset)
        self.auto_reset = bool(auto_reset)
        self.R, self.Cc, self.K = v.rows, v.columns, v.spatial_channels
        self._cfg = _lib.make_config(v)
        h = C.c_void_p()
        _lib.check(self._L.sgx_create(C.byref(self._cfg), self.num_envs, self.device.index, self.seed,
                                      self.env_id_offset, C.byref(h)), self._L)
        self._h = h
        if human_inits is None:
            human_inits = bool(v.human_inits)
        if human_inits:
            if not v.human_inits:
                raise ValueError("Human inits not supported with {} game version".format(v.name))  # util.py:310
            table = np.ascontiguousarray(load_setup_table(v.human_inits))
            _lib.check(self._L.sgx_set_setup_table(self._h, table.ctypes.data_as(C.c_void_p), table.shape[0]), self._L)
        self.human_inits = bool(human_inits)
        N, R, Cc, K, dev = self.num_envs, self.R, self.Cc, self.K, self.device
        self.has_outputs = bool(outputs)
        if not outputs:
            if compact_outputs or final_obs or full_obs:
                raise ValueError("outputs=False is a pool of records: no compact_outputs / final_obs / full_obs")
            self.obs = self.mask = None
        elif self.compact:
            self.compact_obs_stride = int(self._L.sgx_compact_obs_stride(self._h))
            self.compact_mask_words = int(self._L.sgx_compact_mask_words(self._h))
            self.obs = torch.empty((N, self.compact_obs_stride), dtype=torch.uint8, device=dev)
            self.mask = torch.empty((N, self.compact_mask_words), dtype=torch.int32, device=dev)
            self._mask_bytes = None
        else:
            self.obs = torch.empty((N, R, Cc, self.p_channels), dtype=torch.float32, device=dev)
            self.mask = torch.empty((N, R, Cc, K), dtype=torch.uint8, device=dev)
        self.reward = torch.zeros((N, 2), dtype=torch.float32, device=dev)
        self.done = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.player = torch.ones((N,), dtype=torch.int8, device=dev)
        self.invalid_action = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.ending_invalid = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.final_obs = torch.zeros((N, 2, R, Cc, self.p_channels), dtype=torch.float32, device=dev) if final_obs else None
        # fully-observable observation (ObservationModes FULLY_OBSERVABLE / BOTH_OBSERVATIONS), float32 [N,R,C,79]
        self.fobs = torch.empty((N, R, Cc, self.f_channels), dtype=torch.float32, device=dev) if full_obs else None
        self.final_fobs = (torch.zeros((N, 2, R, Cc, self.f_channels), dtype=torch.float32, device=dev)
                           if (full_obs and final_obs) else None)
        self.next_actions = torch.zeros((N,), dtype=torch.int32, device=dev)
        self._io = _lib.SgxStepIO()
        self._next_actions_fresh = False      # next_actions holds a draw for the CURRENT position of every env
        self._ring = self._ring_owners = self._ring_ios = None     # alloc_output_ring()
        self._ring_pos = 0
        self._outputs_owner = self._outputs = None                 # tune_placement()
        self.placement_peak_extra_bytes = 0
        self.start_index = None              # set_start_states(): int32 [N], the pool index of every env's current game
        self._start_winners = None           # set_curriculum(): the table's `winner` column on the device

    # ---- lifecycle -----------------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None):
            if getattr(self, '_outputs_owner', None) is not None:
                # library-owned buffers: the env lets go of its views too, so that the memory is freed now unless the caller still
                # holds a tensor of it (which then stays valid)
                self.obs = self.mask = self.fobs = None
            self._ring = self._ring_owners = None      # (tensors of the ring a caller still holds keep their buffers alive)
            self._release_outputs()
            self._L.sgx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def decode_obs(self, out=None):
        """compact_outputs only: the contract observation float32 [N,R,C,67] of the current compact `obs` (sgx_decode_obs)."""
        assert self.compact
        if out is None:
            out = torch.empty((self.num_envs, self.R, self.Cc, self.p_channels), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_decode_obs(self._h, _ptr(self.obs), _ptr(out), self._stream()), self._L)
        return out

    def decode_mask(self, out=None):
        """compact_outputs only: the contract mask uint8 [N,R,C,K] of the current bit mask (sgx_decode_mask)."""
        assert self.compact
        if out is None:
            out = torch.empty((self.num_envs, self.R, self.Cc, self.K), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_decode_mask(self._h, _ptr(self.mask), _ptr(out), self._stream()), self._L)
        return out

    def set_nt_stores(self, mode='auto'):
        """Store policy of the observation writes (sgx_set_nt_stores): 'auto' (by the launch's output size), False or True.
        Results are identical in every mode; it only moves the launch time."""
        if mode is None or mode == 'auto' or (mode == -1 and mode is not True):
            m = -1
        elif mode is True or mode is False or mode in (0, 1):
            m = int(mode)
        else:
            raise ValueError("set_nt_stores: 'auto', True or False")
        _lib.check(self._L.sgx_set_nt_stores(self._h, m), self._L)

    def set_lane_kernel(self, mode='auto'):
        """Kernel choice on boards of at most 16 cells (sgx_set_lane_kernel): 'auto' / True = one game per lane where the call is
        eligible, False = always the wave-per-game kernel.  Results are identical either way."""
        m = -1 if mode in ('auto', None) else int(bool(mode))
        _lib.check(self._L.sgx_set_lane_kernel(self._h, m), self._L)

    def set_steps_barrier(self, mode=-1):
        """Multi-step launches of the wave-per-game kernel: a barrier between the 8 waves of a workgroup before every step?  -1 (default) = where
        it pays (long rings / trajectory buffers of float32 observations: include/stratego_mi355x.h), 0 = never, 1 = always (sgx_set_steps_barrier).  Results
        are identical in every mode."""
        _lib.check(self._L.sgx_set_steps_barrier(self._h, int(mode)), self._L)

    def set_half_wave(self, on=True):
        """Launches without an observation (mask-only / logic-only steps and rollouts, search expansion) on boards of 33 .. 128 cells: True
        (default) = two games per wave, False = one (sgx_set_half_wave).  Results are identical either way."""
        _lib.check(self._L.sgx_set_half_wave(self._h, 1 if on else 0), self._L)

    def set_multi_step(self, on=True):
        """rollout_steps() on boards of at most 16 cells: True (default) = all steps of a call in one launch where eligible
        (sgx_set_multi_step: the games stay in registers, the logic of step t + 1 runs under the stores of step t); False = one launch
        per step.  Results are identical either way."""
        _lib.check(self._L.sgx_set_multi_step(self._h, 1 if on else 0), self._L)

    @property
    def last_launch_kind(self):
        """Which kernel the last step / observe launch was: _lib.LAUNCH_WAVE, LAUNCH_LANE, LAUNCH_MULTI_STEP or LAUNCH_MULTI_STEP_WAVE (sgx_last_launch_kind)."""
        return int(self._L.sgx_last_launch_kind(self._h))

    def set_xcd_skew(self, per_mille='auto'):
        """Shares of the eight XCDs in a launch (sgx_set_xcd_skew): 'auto' (100 per mille more for the even XCDs when the launch streams
        past the Infinity Cache, equal shares otherwise) or 0 .. 900.  Results are identical for every value."""
        _lib.check(self._L.sgx_set_xcd_skew(self._h, -1 if per_mille in ('auto', None) else int(per_mille)), self._L)

    def set_xcd_shares(self, per_mille=None):
        """Explicit shares of the eight XCDs (per mille of the mean share), None = back to the set_xcd_skew rule."""
        arr = None if per_mille is None else (C.c_int32 * 8)(*[int(x) for x in per_mille])
        _lib.check(self._L.sgx_set_xcd_shares(self._h, arr), self._L)

    # ---- API -----------------------------------------------------------------------------------------
    def reset(self, p1_maps=None, p2_maps=None, env_select=None, observe=True):
        """Start new games (all envs, or those with env_select[i] != 0) and return (obs, mask, player).

        p1_maps / p2_maps: int8 [N, R, C] own-side piece maps (create_initial_state inputs, penv:38-60);
        omit both to sample setups on the device.  observe=False: the records only, nothing is rendered and None is returned (a caller
        that moves on before it looks: vs_env.VsBotVecEnv lets the bot open first)."""
        sel = None
        if env_select is not None:
            sel = env_select.to(device=self.device, dtype=torch.uint8).contiguous()
        m1 = m2 = None
        if p1_maps is not None:
            m1 = torch.as_tensor(p1_maps).to(device=self.device, dtype=torch.int8).contiguous().reshape(self.num_envs, -1)
            m2 = torch.as_tensor(p2_maps).to(device=self.device, dtype=torch.int8).contiguous().reshape(self.num_envs, -1)
            assert m1.shape[1] == self.R * self.Cc and m2.shape == m1.shape
            pieces = self.variant.max_pieces_on_board    # the record's capture-event list holds 2 x pieces entries
            if int(torch.maximum((m1 != 0).sum(1).max(), (m2 != 0).sum(1).max())) > pieces:
                raise ValueError("a piece map holds more pieces than the %s variant has (%d per side)" % (self.variant.name, pieces))
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_reset(self._h, _ptr(sel), _ptr(m1), _ptr(m2), self._stream()), self._L)
        self._next_actions_fresh = False
        if self._placement_pending and sel is None:
            # placement='search': once, now that every record holds a game the trial launches can render
            self._placement_pending = False
            if self.has_outputs and not self.compact and self.obs.numel() * 4 > 300e6:
                free, _ = torch.cuda.mem_get_info(self.device)
                try:
                    self.placement_report = self.tune_placement(max_extra_bytes=min(8 << 30, free // 4))
                except RuntimeError as e:          # (no memory for candidates next to another tenant: the plain tensors stay)
                    self.placement_report = {'failed': str(e)}
        return self.observe() if observe else None

    # ---- start pools: games that start from given positions (maenv:519-527, util.py:374-387 for a batch) -------------------------
    @property
    def start_pool_size(self):
        """Number of records in the start pool (sgx_start_pool_size); 0 = none, games start from sampled setups."""
        return int(self._L.sgx_start_pool_size(self._h))

    def set_start_states(self, states, players=None, first_player='stored', restart_clock=False):
        """From now on every game start that would sample a setup -- reset() without maps (also with env_select) and every auto-reset of
        step() / step_sync() / rollout_steps() / rollout_trajectory(), also in the middle of a multi-step launch -- starts from one of
        the given positions instead, drawn per (seed, env id, game number) on the device (sgx_set_start_pool).

        states: int64 [n,34,R,C] in the reference layout with players int8 [n] (the movers), or a PackedStates / an outputs=False
        VecStrategoEnv of the same variant (its records, `players` unused).  first_player: 'stored' = the position's mover, 'random' =
        +1 / -1 drawn per game (maenv:523).  restart_clock: turn = 0 and max_turns = the variant's in every position (util.py:382-383).
        The positions are COPIED: the argument may be changed or closed afterwards.  Raises ValueError naming the indices of positions
        the packed record cannot carry (import_state_checked flags them `sanitised`) or whose game is over.  Explicit maps passed to
        reset() still win; clear_start_states() goes back to sampled setups.  `start_index` (int32 [N]) holds the pool index of every
        env's current game after the next reset() and after every step (reset() with explicit maps writes -1; such a game has no pool row).  Games already running
        go on; call reset() to start all of them from the pool."""
        if first_player not in ('stored', 'random'):
            raise ValueError("first_player must be 'stored' or 'random'")
        own = None
        src = getattr(states, '_vec', states)
        if isinstance(src, VecStrategoEnv):
            pool, n = src, src.num_envs
        else:
            st = torch.as_tensor(states).to(device=self.device, dtype=torch.int64).contiguous()
            if st.dim() != 4 or tuple(st.shape[1:]) != (NUM_STATE_LAYERS, self.R, self.Cc) or st.shape[0] < 1:
                raise ValueError("states must be int64 [n, %d, %d, %d] with n >= 1" % (NUM_STATE_LAYERS, self.R, self.Cc))
            n = int(st.shape[0])
            if players is None:
                raise ValueError("set_start_states: int64 states come with players int8 [n] (the movers)")
            pl = torch.as_tensor(players).to(device=self.device, dtype=torch.int8).contiguous().reshape(-1)
            if pl.numel() != n or bool(((pl != 1) & (pl != -1)).any()):
                raise ValueError("players must be int8 [n] of +1 / -1")
            own = pool = VecStrategoEnv(self.variant, n, device=self.device.index, seed=self.seed, human_inits=False, outputs=False)
            san = torch.zeros((n,), dtype=torch.uint8, device=self.device)
            pool.import_state_checked(st, pl, san)
            bad = san.nonzero().reshape(-1).tolist()
            if bad:
                pool.close()
                raise ValueError("set_start_states: the packed record cannot carry the positions %s (sanitised on import)" % bad)
        try:
            over = pool.env_info()[:, 2].nonzero().reshape(-1).tolist()
            if over:
                raise ValueError("set_start_states: the game of the positions %s is over" % over)
            flags = (_lib.POOL_RANDOM_FIRST_PLAYER if first_player == 'random' else 0) | (_lib.POOL_RESTART_CLOCK if restart_clock else 0)
            try:
                with torch.cuda.device(self.device):
                    _lib.check(self._L.sgx_set_start_pool(self._h, pool._h, n, flags), self._L)
            except _lib.SgxError as e:
                raise ValueError(str(e))
        finally:
            if own is not None:
                own.close()
        if self.start_index is None:
            self.start_index = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
        _lib.check(self._L.sgx_set_start_index_out(self._h, _ptr(self.start_index)), self._L)
        self._start_winners = None

    def clear_start_states(self):
        """Back to sampled setups (Gravon table / random placement): from here on bit for bit what an env that never had a pool does."""
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_set_start_pool(self._h, None, 0, 0), self._L)
        _lib.check(self._L.sgx_set_start_index_out(self._h, None), self._L)
        self.start_index = self._start_winners = None

    def set_curriculum(self, path_or_pair):
        """The reference's curriculum start states for a batch (curriculum_start_states_path, maenv:519-527; get_random_curriculum_init_fn,
        util.py:374-387): a file load_curriculum_start_states reads (.npz / HDF5), or a (states, winners) pair.  Every game starts from a
        position of the table with turn 0, the variant's max_turns and a random first mover; `start_winner` tells who the table says is
        likely to win the env's current game ("player 1" of the reference's player_map; 0 for a game explicit maps started)."""
        if isinstance(path_or_pair, (tuple, list)):
            states, winners = path_or_pair
        else:
            from .multiagent_env import load_curriculum_start_states
            states, winners = load_curriculum_start_states(path_or_pair)
        states = np.asarray(states).reshape((-1, NUM_STATE_LAYERS, self.R, self.Cc)).astype(np.int64)
        winners = np.asarray(winners).reshape(-1).astype(np.int8)
        if winners.shape[0] != states.shape[0]:
            raise ValueError("set_curriculum: %d states, %d winners" % (states.shape[0], winners.shape[0]))
        # (the table's own movers are never used: the first mover is drawn per game, maenv:523)
        self.set_start_states(states, np.ones(states.shape[0], dtype=np.int8), first_player='random', restart_clock=True)
        self._start_winners = torch.from_numpy(winners).to(self.device)

    @property
    def start_winner(self):
        """set_curriculum(): int8 [N], the table's `winner` of every env's current game (winners[start_index])."""
        if self._start_winners is None:
            raise ValueError("start_winner needs set_curriculum()")
        idx = self.start_index.long()
        w = self._start_winners[idx.clamp(min=0)]
        return torch.where(idx >= 0, w, torch.zeros_like(w))       # (0: a game explicit maps started has no row of the table)

    def observe(self, raw=False, emit_obs=True, emit_mask=True):
        """_get_current_obs for every env (no state change); emit_obs / emit_mask = False skip those outputs."""
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_observe(self._h, _ptr(self.obs) if emit_obs else None, _ptr(self.fobs) if emit_obs else None,
                                           _ptr(self.mask) if emit_mask else None, _ptr(self.player),
                                           (_lib.STEP_RAW_OBS if raw else 0) | self._mode_flags, self._stream()), self._L)
        return self.obs, self.mask, self.player

    def tune_placement(self, trials=None, max_extra_bytes=8 << 30, wide_extra_bytes=0):
        """tune_placement_once with `max_extra_bytes`; if that budget held no candidate of the fast class (none >= 14 % below the
        slowest one) and `wide_extra_bytes` is larger, a second pass spreads the same number of candidates over that wider budget and is
        kept only if it found something faster (partial-observation buffers that stream past the Infinity Cache only).  Returns the
        first pass's report, with report['wide'] = {'obs': [...], 'used': bool, 'peak_extra_bytes': int} when the second pass ran."""
        rep = self.tune_placement_once(trials, max_extra_bytes)
        t = rep.get('obs') or []
        streams = self.obs.numel() * 4 > 300e6
        if t and streams and wide_extra_bytes > max_extra_bytes and min(t) > 0.86 * max(t) and self.fobs is None:
            first = (self.obs, self.mask, self._outputs_owner, self._outputs, self.placement_peak_extra_bytes)
            rep2 = self.tune_placement_once(trials, wide_extra_bytes)
            t2 = rep2.get('obs') or []
            used = bool(t2) and min(t2) < min(t)
            rep['wide'] = {'obs': t2, 'used': used, 'peak_extra_bytes': self.placement_peak_extra_bytes}
            if not used:
                self.obs, self.mask, self._outputs_owner, self._outputs, self.placement_peak_extra_bytes = first
                self.observe()
        return rep

    def tune_placement_once(self, trials=None, max_extra_bytes=8 << 30):
        """Move the big output tensors (obs, fobs, mask) into library-owned buffers picked by a bounded placement trial
        (sgx_alloc_outputs).

        Measured on MI355X: device memory comes in regions of two kinds; an observation buffer lying inside one region runs at
        that region's rate (about 350 or 380-395 us per launch of 65,536 Barrage games), one whose pages mix both kinds at
        313-325 us, and which of these a plain allocation gets depends on what was allocated before it.  The library tries
        up to `trials` candidate allocations, each behind a padding allocation of growing size that is released again, times a
        few state-preserving sgx_observe launches on each and keeps the fastest; it never holds more than `max_extra_bytes`
        beyond the buffers it returns.  Call after reset().  Returns the per-candidate launch times in microseconds:
        {'obs': [...], ('fobs': [...])}; [0] is the plain first allocation."""
        if self.compact:
            raise ValueError("tune_placement: compact outputs (235 MB per 65,536 Barrage games) fit the Infinity Cache and have no placement classes")
        out = _lib.SgxOutputs()
        flags = self._mode_flags | (_lib.OUT_FULL_OBS if self.fobs is not None else 0)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_alloc_outputs(self._h, flags, int(max_extra_bytes), int(trials or _lib.OUT_MAX_TRIALS),
                                                 self._stream(), C.byref(out)), self._L)
        owner = _OutputsOwner(self._L, out)
        self._outputs_owner = owner          # replaces the env's reference to an earlier allocation (its tensors keep theirs)
        self._outputs = out
        N, R, Cc, K = self.num_envs, self.R, self.Cc, self.K
        self.obs = _wrap_device(out.obs_dev, (N, R, Cc, self.p_channels), torch.float32, self.device, owner)
        self.mask = _wrap_device(out.mask_dev, (N, R, Cc, K), torch.uint8, self.device, owner)
        report = {'obs': [float(x) for x in out.trial_us[:out.n_trials]]}
        if out.fobs_dev:
            self.fobs = _wrap_device(out.fobs_dev, (N, R, Cc, self.f_channels), torch.float32, self.device, owner)
            report['fobs'] = [float(x) for x in out.ftrial_us[:out.n_ftrials]]
        self.placement_peak_extra_bytes = int(out.peak_extra_bytes)
        self.observe()
        return report

    @property
    def record_bytes(self):
        """Bytes of one game's packed state record in device memory (sgx_record_bytes): read once and written once per step."""
        return int(self._L.sgx_record_bytes(self._h))

    @property
    def build_id(self):
        """Hash of the sources the loaded library was compiled from (sgx_build_id)."""
        return self._L.sgx_build_id().decode('ascii', 'replace')

    def alloc_output_ring(self, n_sets, tune=None, max_extra_bytes=8 << 30, trials=None, wide_extra_bytes=0):
        """A ring of `n_sets` output sets (obs, mask[, fobs]) for rollout_steps(..., ring=True): step i writes set i mod n_sets -- a
        rollout into a trajectory buffer that keeps the last n_sets steps (sgx_step_ring).  Set 0 is the env's current set; the others
        are torch.empty tensors or, with tune=True (the default, tune=None, where the env's own set came from the placement search --
        placement='search' or tune_placement()), library-owned buffers from the placement trial (one sgx_alloc_outputs each; a set
        whose search ends more than 3 % above the env's own set is searched once more over `wide_extra_bytes`, like tune_placement's
        wide pass, and the faster of the two is kept; if the extra sets turn out more than 3 % faster than the env's own set, that one
        is searched once more against them).  Returns the per-set trial reports (None for untuned sets and for set 0 unless it was
        searched again: {'obs', 'used', 'target_us', 'before_us'} then)."""
        n_sets = int(n_sets)
        if n_sets < 1:
            raise ValueError("n_sets must be >= 1")
        if tune is None:
            tune = getattr(self, '_outputs', None) is not None and not self.compact
        # every extra set should be as fast as the env's own: the searches go on until a candidate is within 3 % of what the first
        # search kept (sgx_set_placement_target), inside the same budget
        target = 0.0
        if tune and not self.compact and getattr(self, '_outputs', None) is not None and self._outputs.n_trials > 0:
            target = min(float(x) for x in self._outputs.trial_us[:self._outputs.n_trials])
        if not self.has_outputs:
            raise ValueError("alloc_output_ring: this env was created with outputs=False")
        try:      # (whatever a placement call raises midway, the handle's search target goes back to 0: a later tune_placement() must not chase a stale one)
            _lib.check(self._L.sgx_set_placement_target(self._h, C.c_float(target)), self._L)
            N, R, Cc, K, dev = self.num_envs, self.R, self.Cc, self.K, self.device
            self._ring = [(self.obs, self.mask, self.fobs)]
            self._ring_owners = [getattr(self, '_outputs_owner', None)]
            reports = [None]
            for _ in range(1, n_sets):
                if tune and not self.compact:
                    out = _lib.SgxOutputs()
                    flags = self._mode_flags | (_lib.OUT_FULL_OBS if self.fobs is not None else 0)
                    with torch.cuda.device(self.device):
                        _lib.check(self._L.sgx_alloc_outputs(self._h, flags, int(max_extra_bytes), int(trials or _lib.OUT_MAX_TRIALS),
                                                             self._stream(), C.byref(out)), self._L)
                    owner = _OutputsOwner(self._L, out)
                    times = [float(x) for x in out.trial_us[:out.n_trials]]
                    report = {'obs': times}
                    if target > 0 and times and min(times) > 1.03 * target and wide_extra_bytes > max_extra_bytes:
                        out2 = _lib.SgxOutputs()
                        with torch.cuda.device(self.device):
                            _lib.check(self._L.sgx_alloc_outputs(self._h, flags, int(wide_extra_bytes), int(trials or _lib.OUT_MAX_TRIALS),
                                                                 self._stream(), C.byref(out2)), self._L)
                        owner2 = _OutputsOwner(self._L, out2)
                        times2 = [float(x) for x in out2.trial_us[:out2.n_trials]]
                        report['wide'] = {'obs': times2, 'used': bool(times2) and min(times2) < min(times)}
                        if report['wide']['used']:
                            out, owner = out2, owner2          # (the first search's buffers go with their owner)
                            report['obs'] = times + times2     # min() over both = what is kept
                        del out2, owner2
                    obs = _wrap_device(out.obs_dev, (N, R, Cc, self.p_channels), torch.float32, dev, owner)
                    mask = _wrap_device(out.mask_dev, (N, R, Cc, K), torch.uint8, dev, owner)
                    fobs = _wrap_device(out.fobs_dev, (N, R, Cc, self.f_channels), torch.float32, dev, owner) if out.fobs_dev else None
                    reports.append(report)
                    self._ring_owners.append(owner)
                else:
                    obs, mask = torch.empty_like(self.obs), torch.empty_like(self.mask)       # (compact outputs: the same compact shapes)
                    fobs = torch.empty((N, R, Cc, self.f_channels), dtype=torch.float32, device=dev) if self.fobs is not None else None
                    reports.append(None)
                    self._ring_owners.append(None)
                self._ring.append((obs, mask, fobs))
            # The other way round: the env's OWN set may be the slow one (its search ran first, with no target -- one box: 298.5 us after 82
            # candidates, then 274-281 us for the extra sets).  It is searched once more, against the best of the others, and replaced if
            # that finds something faster; reports[0] = {'obs': [...], 'used': bool} then.
            best_extra = min([min(r['obs']) for r in reports[1:] if r and r.get('obs')] or [0.0])
            if target > 0 and 0 < best_extra < 0.97 * target and self.fobs is None:
                _lib.check(self._L.sgx_set_placement_target(self._h, C.c_float(best_extra)), self._L)
                first = (self.obs, self.mask, self._outputs_owner, self._outputs, self.placement_peak_extra_bytes)
                rep0 = self.tune_placement_once(trials, max(int(max_extra_bytes), int(wide_extra_bytes)))
                used = bool(rep0.get('obs')) and min(rep0['obs']) < target
                if not used:
                    self.obs, self.mask, self._outputs_owner, self._outputs, self.placement_peak_extra_bytes = first
                    self.observe()
                self._ring[0] = (self.obs, self.mask, self.fobs)
                self._ring_owners[0] = self._outputs_owner
                reports[0] = {'obs': rep0.get('obs') or [], 'used': used, 'target_us': best_extra, 'before_us': target}
        except BaseException:
            self._ring = self._ring_owners = None      # (no half-built ring)
            raise
        finally:
            _lib.check(self._L.sgx_set_placement_target(self._h, C.c_float(0.0)), self._L)
        self._ring_pos = 1 % n_sets          # set 0 holds the current position's outputs: the next step writes set 1
        self._ring_ios = (_lib.SgxStepIO * n_sets)()
        return reports

    def repeat_output_ring(self, n_entries):
        """The ring of alloc_output_ring() as a ring of `n_entries` entries over the SAME buffers (entry i = set i mod n_sets): what a long
        ring costs on the memory of a short one -- beyond 8 entries sgx_step_ring reads the pointers from a device table (bench.py's trajectory leg
        times exactly this).  The buffers are rewritten every n_sets steps as before."""
        if not self._ring:
            raise ValueError("repeat_output_ring() needs alloc_output_ring() first")
        n_entries, base = int(n_entries), len(self._ring)
        if n_entries < base:
            raise ValueError("repeat_output_ring: fewer entries than the ring has sets")
        pos = (self._ring_pos - 1) % base              # the set holding the current position's outputs keeps that role
        self._ring = [self._ring[i % base] for i in range(n_entries)]
        self._ring_owners = [self._ring_owners[i % base] for i in range(n_entries)]
        self._ring_pos = (pos + 1) % n_entries
        self._ring_ios = (_lib.SgxStepIO * n_entries)()

    def _release_outputs(self):
        """Drops the env's own reference to library-owned output buffers; they are freed when the last tensor viewing them goes."""
        self._outputs_owner = None
        self._outputs = None

    def step(self, actions, want_next_actions=False, emit_obs=True, emit_mask=True, flags=0):
        """One env.step() for every env.  actions: int32 [N] flat (R,C,K) indices in each mover's perspective."""
        a = actions
        if a.dtype != torch.int32 or a.device != self.device or not a.is_contiguous():
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        assert a.numel() == self.num_envs * (4 if (flags & _lib.STEP_ACTIONS_POSITIONS) else 1)
        io = self._fill_io(a, want_next_actions, emit_obs, emit_mask, flags)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_step(self._h, C.byref(io), self._stream()), self._L)
        self._next_actions_fresh = bool(want_next_actions)
        return self.obs, self.mask, self.reward, self.done, self.player

    def step_sync(self, actions, emit_obs=True, emit_mask=True, flags=0):
        """step() and wait until the outputs are complete (sgx_step_sync): the latency path of a handful of games -- up to 8 games on
        a 4-aligned board of more than 32 cells run one workgroup per game and the call returns as soon as the kernel has published
        its outputs, without a stream synchronisation."""
        a = actions
        if a.dtype != torch.int32 or a.device != self.device or not a.is_contiguous():
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        assert a.numel() == self.num_envs * (4 if (flags & _lib.STEP_ACTIONS_POSITIONS) else 1)
        io = self._fill_io(a, False, emit_obs, emit_mask, flags)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_step_sync(self._h, C.byref(io), self._stream()), self._L)
        self._next_actions_fresh = False
        return self.obs, self.mask, self.reward, self.done, self.player

    def _fill_io(self, a, want_next_actions, emit_obs, emit_mask, flags):
        io = self._io
        io.actions_dev = a.data_ptr()
        io.obs_dev = self.obs.data_ptr() if (emit_obs and self.obs is not None) else None
        io.fobs_dev = self.fobs.data_ptr() if (emit_obs and self.fobs is not None) else None
        io.final_fobs_dev = self.final_fobs.data_ptr() if self.final_fobs is not None else None
        io.mask_dev = self.mask.data_ptr() if (emit_mask and self.mask is not None) else None
        io.reward_dev = self.reward.data_ptr()
        io.done_dev = self.done.data_ptr()
        io.player_dev = self.player.data_ptr()
        io.invalid_action_dev = self.invalid_action.data_ptr()
        io.ending_invalid_dev = self.ending_invalid.data_ptr()
        io.final_obs_dev = self.final_obs.data_ptr() if self.final_obs is not None else None
        io.next_actions_dev = self.next_actions.data_ptr() if want_next_actions else None
        io.auto_reset = 1 if self.auto_reset else 0
        io.flags = int(flags) | self._mode_flags
        return io

    def rollout_step(self):
        """Random-valid-action rollout step: plays `next_actions` (drawn by the previous call, or now if there is no
        current draw) and draws the next."""
        if not self._next_actions_fresh:
            self.sample_valid_actions()
        return self.step(self.next_actions, want_next_actions=True)

    def rollout_steps(self, n_steps, chains=1, ring=False, emit_obs=True, emit_mask=True):
        """`n_steps` rollout steps enqueued by one library call (sgx_step_n): same results as calling rollout_step()
        n_steps times, without a Python round trip per step (toy boards are launch-bound otherwise).  chains > 1 (sgx_rollout):
        the batch is split into that many contiguous ranges of games whose launches overlap on streams of their own; chains = 0 /
        'auto': the multi-step launch where the call is eligible, else as many chains as the library's measured rule says (2 on boards of
        up to 36 cells and on odd boards, else 1).
        ring=True (after alloc_output_ring): the steps write the ring's output sets in turn (sgx_step_ring); self.obs / self.mask /
        self.fobs are the set the LAST step wrote afterwards.  emit_obs / emit_mask = False: rollouts that write no observation / no mask
        (logic-only playouts, e.g. of a search).  Where the call is eligible all steps run in ONE launch (sgx_set_multi_step): the games stay on
        the chip between the steps."""
        if not self._next_actions_fresh:
            self.sample_valid_actions()
        if ring:
            if not self._ring:
                raise ValueError("rollout_steps(ring=True) needs alloc_output_ring() first")
            n_sets, n_steps = len(self._ring), int(n_steps)
            for k, (obs, mask, fobs) in enumerate(self._ring):
                self.obs, self.mask, self.fobs = obs, mask, fobs
                io = self._fill_io(self.next_actions, True, emit_obs, emit_mask, 0)
                C.memmove(C.byref(self._ring_ios[k]), C.byref(io), C.sizeof(_lib.SgxStepIO))
            first = self._ring_pos
            with torch.cuda.device(self.device):
                _lib.check(self._L.sgx_step_ring(self._h, self._ring_ios, n_sets, first, n_steps, self._stream()), self._L)
            last = (first + n_steps - 1) % n_sets if n_steps > 0 else (first - 1) % n_sets
            self.obs, self.mask, self.fobs = self._ring[last]
            self._ring_pos = (first + n_steps) % n_sets
            return self.obs, self.mask, self.reward, self.done, self.player
        io = self._fill_io(self.next_actions, True, emit_obs, emit_mask, 0)
        with torch.cuda.device(self.device):
            if chains in (0, 'auto') or chains > 1:        # 0 / 'auto': the library's measured rule (2 chains on small and odd boards)
                _lib.check(self._L.sgx_rollout(self._h, C.byref(io), int(n_steps), 0 if chains == 'auto' else int(chains), self._stream()), self._L)
            else:
                _lib.check(self._L.sgx_step_n(self._h, C.byref(io), int(n_steps), self._stream()), self._L)
        return self.obs, self.mask, self.reward, self.done, self.player

    # ---- trajectory buffers: a fresh slice per step, like the reference's fresh arrays per env.step() (impl:905, maenv:447-497) ------
    def alloc_trajectory(self, n_slots, results=True, actions=True):
        """Tensors with a leading slot axis for rollout_trajectory(): obs [T,N,R,C,67], mask [T,N,R,C,K] (fobs [T,N,R,C,79] with
        full_obs=True; the compact shapes with compact_outputs=True), and -- results=True -- reward [T,N,2], done / invalid_action /
        ending_invalid [T,N], player [T,N]; actions=True: the action every env DREW in the step, int32 [T,N] (the action the next step
        plays: chosen from the observation and mask of the same slot).  Returns a dict of torch tensors."""
        if not self.has_outputs:
            raise ValueError("alloc_trajectory: this env was created with outputs=False")
        T, N, dev = int(n_slots), self.num_envs, self.device
        if T < 1:
            raise ValueError("n_slots must be >= 1")
        traj = {'obs': torch.empty((T,) + tuple(self.obs.shape), dtype=self.obs.dtype, device=dev),
                'mask': torch.empty((T,) + tuple(self.mask.shape), dtype=self.mask.dtype, device=dev)}
        if self.fobs is not None:
            traj['fobs'] = torch.empty((T,) + tuple(self.fobs.shape), dtype=torch.float32, device=dev)
        if results:
            traj['reward'] = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
            for k, dt in (('done', torch.uint8), ('invalid_action', torch.uint8), ('ending_invalid', torch.uint8), ('player', torch.int8)):
                traj[k] = torch.zeros((T, N), dtype=dt, device=dev)
        if actions:
            traj['actions'] = torch.zeros((T, N), dtype=torch.int32, device=dev)
        if results and self.start_index is not None:       # a start pool is set: the pool index of the game every slot's outputs belong to
            traj['start_index'] = torch.full((T, N), -1, dtype=torch.int32, device=dev)
        return traj

    def rollout_trajectory(self, n_steps, traj, first_slot=0, emit_obs=True, emit_mask=True):
        """`n_steps` random-valid-action rollout steps (like rollout_steps) whose step t writes slot (first_slot + t) % T of the
        tensors of `traj` (alloc_trajectory): one library call (sgx_step_traj), and where the call is eligible ONE launch per 256 steps
        (sgx_set_multi_step) -- for any number of slots.  Afterwards self.obs / self.mask / self.fobs (and, if `traj` holds per-slot
        results, self.reward / done / player / invalid_action / ending_invalid) are views of the slot the LAST step wrote; next_actions
        holds the last draw.  Returns `traj`."""
        n_steps = int(n_steps)
        T = int(traj['obs'].shape[0])
        if not 0 <= first_slot < T:
            raise ValueError("first_slot out of range")
        if (self.fobs is not None) != ('fobs' in traj):
            raise ValueError("traj['fobs'] goes with full_obs=True")
        per_slot = 'reward' in traj
        # every tensor of the dict reaches sgx_step_traj as a raw pointer with ONE slot stride (num_envs): all of them are checked here,
        # before anything is launched or any tensor of the env is swapped
        N = self.num_envs
        want = {'obs': (tuple(self.obs.shape), self.obs.dtype), 'mask': (tuple(self.mask.shape), self.mask.dtype)}
        if 'fobs' in traj:
            want['fobs'] = (tuple(self.fobs.shape), torch.float32)
        if per_slot:
            want.update({'reward': ((N, 2), torch.float32), 'done': ((N,), torch.uint8), 'player': ((N,), torch.int8),
                         'invalid_action': ((N,), torch.uint8), 'ending_invalid': ((N,), torch.uint8)})
        if 'actions' in traj:
            want['actions'] = ((N,), torch.int32)
        if self.start_index is not None and per_slot and 'start_index' not in traj:
            # (per-slot results put step t's pool index at slot t too: the env's own [N] tensor has no room for that)
            raise ValueError("a start pool is set: this trajectory needs traj['start_index'] (allocate it again with alloc_trajectory)")
        if 'start_index' in traj:
            if self.start_index is None:
                raise ValueError("traj['start_index'] goes with a start pool (set_start_states)")
            if not per_slot:
                raise ValueError("traj['start_index'] goes with per-slot results (alloc_trajectory(results=True))")
            want['start_index'] = ((N,), torch.int32)
        for k, (shape, dtype) in want.items():
            t = traj.get(k)
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != (T,) + shape or t.dtype != dtype or not t.is_contiguous() or t.device != self.device):
                raise ValueError("traj['%s'] must be a contiguous [%d, %s] %s tensor on %s (alloc_trajectory makes them)"
                                 % (k, T, ', '.join(map(str, shape)), dtype, self.device))
        if not self._next_actions_fresh:
            self.sample_valid_actions()
        keep = (self.obs, self.mask, self.fobs, self.reward, self.done, self.player, self.invalid_action, self.ending_invalid)
        keep_si = self.start_index

        def point_start_index(t):
            if keep_si is not None:
                self.start_index = t
                _lib.check(self._L.sgx_set_start_index_out(self._h, _ptr(t)), self._L)

        def views(slot):
            self.obs, self.mask, self.fobs = traj['obs'][slot], traj['mask'][slot], (traj['fobs'][slot] if 'fobs' in traj else None)
            if per_slot:
                self.reward, self.done, self.player = traj['reward'][slot], traj['done'][slot], traj['player'][slot]
                self.invalid_action, self.ending_invalid = traj['invalid_action'][slot], traj['ending_invalid'][slot]
        try:
            views(0)
            if 'start_index' in traj:
                point_start_index(traj['start_index'][0])          # (the library adds slot * num_envs, like for `done`)
            io = self._fill_io(self.next_actions, True, emit_obs, emit_mask, 0)
            t = _lib.SgxTrajIO()
            C.memmove(C.byref(t.io), C.byref(io), C.sizeof(_lib.SgxStepIO))
            t.n_slots, t.results_per_slot, t.slot_envs = T, 1 if per_slot else 0, self.num_envs
            t.actions_log_dev = traj['actions'].data_ptr() if 'actions' in traj else None
            with torch.cuda.device(self.device):
                _lib.check(self._L.sgx_step_traj(self._h, C.byref(t), int(first_slot), n_steps, self._stream()), self._L)
        except BaseException:
            (self.obs, self.mask, self.fobs, self.reward, self.done, self.player, self.invalid_action, self.ending_invalid) = keep
            point_start_index(keep_si)
            raise
        if n_steps == 0:
            (self.obs, self.mask, self.fobs, self.reward, self.done, self.player, self.invalid_action, self.ending_invalid) = keep
            point_start_index(keep_si)
        else:
            views((first_slot + n_steps - 1) % T)
            if 'start_index' in traj:                              # like `done`: the env's own view is the last slot written
                point_start_index(traj['start_index'][(first_slot + n_steps - 1) % T])
        return traj

    def choose_actions(self, logits, temperature=1.0, mask=None, out=None):
        """The reference's chooser for a batch (examples/basic_game_loop.py:6-31): one action per game drawn from
        softmax(logits / temperature) over the VALID actions of `mask` (default: the current mask -- bytes, or the bit mask of
        compact_outputs=True), on the device (sgx_choose_actions).  logits: float32 [N, R, C, K] (or [N, R*C*K]) from the caller's
        policy.  temperature 0 = argmax.  The draw is keyed by (seed, global env id, game, turn) like the fused sampler's, and with equal
        logits it is that sampler's action.  Weights are 2^23 fixed point: an action less than 2^-23 as likely as the most likely one is
        never drawn; an env whose valid actions ALL have -inf / NaN logits (or whose mask is empty) gets -1, which step() would flag as
        an invalid action.  `mask` and `out` go to the library as they are: a tensor on another device, not contiguous, of another dtype
        or size is a ValueError before anything is launched (check_choose_tensors).  -> int32 [N] (`out` or next_actions: ready for step())."""
        lg = logits
        if lg.dtype != torch.float32 or lg.device != self.device or not lg.is_contiguous():
            lg = lg.to(device=self.device, dtype=torch.float32).contiguous()
        if lg.numel() != self.num_envs * self.R * self.Cc * self.K:
            raise ValueError("logits must hold num_envs x rows x columns x ways_to_move floats")
        own = mask is None
        mask = self.mask if mask is None else mask
        out = self.next_actions if out is None else out
        words = 0
        if mask.dtype == torch.int32:
            words = self.compact_mask_words if self.compact else int(self._L.sgx_compact_mask_words(self._h))
        bits = check_choose_tensors(self.num_envs, self.R * self.Cc * self.K, words, self.device,
                                    *((t.dtype, t.device, t.numel(), t.is_contiguous()) for t in (mask, out)))
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_choose_actions(self._h, _ptr(lg), _ptr(mask), C.c_float(float(temperature)),
                                                  _lib.STEP_COMPACT_MASK if bits else 0, _ptr(out), self._stream()), self._L)
        if own and out is self.next_actions:
            self._next_actions_fresh = False      # (a policy's choice, not the uniform draw rollout_step() plays)
        return out

    # ---- snapshots: the packed records of every game, in a pool without output tensors -------------------------------
    def snapshot(self, out=None):
        """Copy every game's packed record (boards, counters, game number: everything the counter RNG and the rules depend on)
        into a pool of records without output tensors (`out`, or a new one): sgx_copy_envs.  restore() puts it back.
        A start pool (set_start_states) is NOT part of a snapshot: the records carry the game numbers, so the restored games draw the
        same start positions again only while the same pool is set."""
        snap = out if out is not None else VecStrategoEnv(self.variant, self.num_envs, device=self.device.index, seed=self.seed,
                                                          env_id_offset=self.env_id_offset, human_inits=False, outputs=False)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_copy_envs(snap._h, None, self._h, None, self.num_envs, self._stream()), self._L)
        return snap

    def restore(self, snap):
        """The inverse of snapshot(): every game continues from the snapshot's position; returns observe() of it (the outputs and the
        next random draw are those of the restored position again)."""
        if snap.num_envs != self.num_envs:
            raise ValueError("restore: the snapshot holds %d games, this env %d" % (snap.num_envs, self.num_envs))
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_copy_envs(self._h, None, snap._h, None, self.num_envs, self._stream()), self._L)
        self._next_actions_fresh = False
        return self.observe()

    def replay(self, src, actions, lengths=None, src_index=None, skip_invalid=False, actions_1d=False, allow_piece_oscillation=False,
               track_origins=False, origins_in=None):
        """Every game i of this env becomes src[src_index[i]] advanced by its list actions[i, :lengths[i]], all moves in one launch
        (sgx_replay; the rule is in include/stratego_mi355x.h); `src` stays what it was.  A following observe() renders the replayed
        positions' observations and masks: with start records and recorded actions a learner re-renders any (game, t) it samples instead
        of keeping every step's observation.
        src: a PackedStates, a snapshot() or another VecStrategoEnv of the same variant (this env itself for an in-place call without
        src_index).  actions: int32 device tensor [n, L] with ANY non-negative strides, passed through as they are -- traj['actions'][:T].T
        is taken without a copy.  lengths: int32 [n] (None: L for all).  skip_invalid: an invalid entry is passed over instead of ending
        the replay; actions_1d: entries are absolute 1-D indices (get_next_state's) instead of flat spatial indices in the mover's
        perspective.  No auto-reset: a replay stops at the end of its game.  -> ReplayResult.
        track_origins: the same replay also tracks every piece back to the cell it stood on in `src` (sgx_set_replay_origins; the rule is in
        the header): ReplayResult.origins is int16 [n, 2, cells], origins[i][p][c] = the root cell of the piece of player index p (0 = +1,
        1 = -1) on absolute cell c of the final position, -1 where it has none -- what beliefs.follow takes.  origins_in (implies
        track_origins): an int16 device tensor [src's n, 2, cells] of labels the roots already carry (the origins of an earlier replay, or
        any piece ids), read at record src_index[i] and carried verbatim instead of the cells' own indices.  Every other result, and the
        records, are what the untracked call gives."""
        from .procedural_env import ReplayResult
        n, dev = self.num_envs, self.device
        src_vec = getattr(src, '_vec', src)
        if src_vec is self and src_index is not None:
            raise ValueError("an in-place replay through src_index would race (a record may be overwritten before it is read): "
                             "replay into another pool")
        a = actions
        if not isinstance(a, torch.Tensor) or a.dtype != torch.int32 or a.device != dev:
            a = torch.as_tensor(a).to(device=dev, dtype=torch.int32)
        if a.dim() != 2 or a.shape[0] != n:
            raise ValueError("actions must be an int32 tensor [%d, L]" % n)
        L = int(a.shape[1])
        game_stride, step_stride = (int(x) for x in a.stride())
        if n * L == 0:
            game_stride = step_stride = 0
        if game_stride < 0 or step_stride < 0:
            raise ValueError("actions must have non-negative strides")
        elems = a.untyped_storage().nbytes() // 4 - int(a.storage_offset())          # what the view can address from its first element
        ln = None if lengths is None else torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).reshape(n).contiguous()
        si = None if src_index is None else torch.as_tensor(src_index).to(device=dev, dtype=torch.int32).reshape(n).contiguous()
        res = ReplayResult(torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev),
                           torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.float32, device=dev),
                           torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev),
                           torch.empty((n,), dtype=torch.int8, device=dev))
        flags = ((_lib.REPLAY_SKIP_INVALID if skip_invalid else 0) | (_lib.REPLAY_ACTIONS_1D if actions_1d else 0)
                 | (_lib.REPLAY_ALLOW_OSCILLATION if allow_piece_oscillation else 0))
        io = _lib.SgxReplayIO(a.data_ptr() if L else None, _ptr(ln), res.applied.data_ptr(), res.consumed.data_ptr(), res.stop.data_ptr(),
                              res.reward.data_ptr(), res.done.data_ptr(), res.ending_invalid.data_ptr(), res.player.data_ptr(),
                              game_stride, step_stride, elems, L, flags)
        if origins_in is not None:
            cells = self.R * self.Cc
            if not isinstance(origins_in, torch.Tensor) or origins_in.dtype != torch.int16 or origins_in.device != dev or not origins_in.is_contiguous() \
                    or tuple(origins_in.shape) != (src_vec.num_envs, 2, cells):
                raise ValueError("origins_in must be a contiguous int16 device tensor [%d, 2, %d] (one block of labels per record of src)"
                                 % (src_vec.num_envs, cells))
            track_origins = True
        if not track_origins:
            with torch.cuda.device(dev):
                _lib.check(self._L.sgx_replay(self._h, src_vec._h, _ptr(si), C.byref(io), self._stream()), self._L)
        else:
            res.origins = torch.empty((n, 2, self.R * self.Cc), dtype=torch.int16, device=dev)
            _lib.check(self._L.sgx_set_replay_origins(self._h, _ptr(origins_in), res.origins.data_ptr()), self._L)
            try:
                with torch.cuda.device(dev):
                    _lib.check(self._L.sgx_replay(self._h, src_vec._h, _ptr(si), C.byref(io), self._stream()), self._L)
            finally:                                                 # the setting lasts for this call alone, also when it raises
                self._L.sgx_set_replay_origins(self._h, None, None)
        self._next_actions_fresh = False
        return res

    def step_vs(self, actions, agent, weights, see_all=False, draw=0, src=None, src_index=None, out=None):
        """The agent's move and a table bot's reply for every game, in ONE launch that writes no observation (sgx_step_vs; the rule is in
        include/stratego_mi355x.h).  Where the game is not over and the agent is to move, actions[i] is applied as step() applies it (a
        refused action leaves the position alone: invalid_action = 1, the bot stays still); where the bot is to move then -- or from the
        start, the agent not being the mover -- it moves once, drawn from `weights` as a weighted playout draws its moves.  There is no
        auto-reset and a finished game is left as it is, so afterwards every game that is neither over nor refused has the agent to move;
        observe() renders it.
        actions: int32 [N] flat (R,C,K) indices in the mover's perspective, or None: no agent moves, the bot opens where it is to move.
        agent: +1 / -1, or an int8 tensor [N] of the agent's side per game (< 0: -1).  weights: [4, 13, 14] integers in [0, 4095]
        (stratego_env_amd.playout_policies), read before the call returns; see_all=True lets the bot see the agent's true piece types,
        the default is what its partial observation shows.  draw: the replies are keyed by (seed, env id, draw, turn): pass another
        one with every call.  src / src_index: the positions come from src[src_index[i]] (a PackedStates, a snapshot or another env)
        instead of this env's own.  out: a StepVsResult to fill instead of a new one.
        -> StepVsResult: reward [N,2], done, ending_invalid, player (of the position reached), invalid_action, moved (bit 0: the agent,
        bit 1: the bot), reply_action (the bot's move in the bot's perspective, -1 = none)."""
        from .procedural_env import StepVsResult, playout_weights
        n, dev = self.num_envs, self.device
        table = playout_weights(weights)
        src_vec = self if src is None else getattr(src, '_vec', src)
        if src_vec is self and src_index is not None:
            raise ValueError("an in-place step_vs through src_index would race (a record may be overwritten before it is read): "
                             "step into another pool")
        a = None
        if actions is not None:
            a = actions
            if not isinstance(a, torch.Tensor) or a.dtype != torch.int32 or a.device != dev or not a.is_contiguous():
                a = torch.as_tensor(a).to(device=dev, dtype=torch.int32).contiguous()
            if a.numel() != n:
                raise ValueError("actions must hold one int32 per game (%d)" % n)
        side, sides = 1, None
        if isinstance(agent, (int, np.integer)):
            if int(agent) not in (1, -1):
                raise ValueError("agent must be +1, -1 or an int8 tensor [N]")
            side = int(agent)
        else:
            sides = agent
            if not isinstance(sides, torch.Tensor) or sides.dtype != torch.int8 or sides.device != dev or not sides.is_contiguous():
                sides = torch.as_tensor(sides).to(device=dev, dtype=torch.int8).contiguous()
            if sides.numel() != n:
                raise ValueError("agent must be +1, -1 or an int8 tensor [N]")
        si = None if src_index is None else torch.as_tensor(src_index).to(device=dev, dtype=torch.int32).reshape(n).contiguous()
        res = out if out is not None else StepVsResult.empty(n, dev)
        io = _lib.SgxVsIO(_ptr(a), _ptr(sides), res.reward.data_ptr(), res.done.data_ptr(), res.ending_invalid.data_ptr(), res.player.data_ptr(),
                          res.invalid_action.data_ptr(), res.moved.data_ptr(), res.reply_action.data_ptr(), side, _lib.VS_SEE_ALL if see_all else 0)
        with torch.cuda.device(dev):
            _lib.check(self._L.sgx_step_vs(self._h, src_vec._h, _ptr(si), C.byref(io), table.ctypes.data_as(C.POINTER(C.c_uint16)),
                                           int(draw) & 0xFFFFFFFFFFFFFFFF, self._stream()), self._L)
        self._next_actions_fresh = False
        return res

    def count_moves(self, index=None):
        """The number of valid moves of every game's mover and their exclusive scan (sgx_count_moves; the rule is in
        include/stratego_mi355x.h): root slot i is game index[i] (int32 [n], any length, repeats allowed; None: every game in order).
        -> (counts int32 [n], offsets int64 [n + 1]) on the device, no synchronisation: counts[i] is 0 for a finished game and for a mover
        without a move, offsets[i] is the number of the first child of root i and offsets[n] the total (PackedStates.expand_all takes them)."""
        dev = self.device
        idx = None if index is None else torch.as_tensor(index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        n = self.num_envs if idx is None else int(idx.numel())
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._L.sgx_count_moves(self._h, _ptr(idx) if n else None, n, _ptr(counts) if n else None, _ptr(offsets), self._stream()), self._L)
        return counts, offsets

    def state_keys(self, index=None, observer=None, clock=True, wide=False):
        """One 64-bit position key per game, straight from the packed records in one launch (sgx_state_keys; the rule is in
        include/stratego_mi355x.h): slot i is game index[i] (int32 [n], any length, repeats allowed; None: every game in order).
        observer=None: the state key, equal exactly when the reference state and the mover are equal; observer 0 / +1 / -1 (as determinize
        takes them: each game's mover / that player): the information-set key, equal exactly when everything that player can see is equal --
        every world determinize deals for an observer keeps that observer's key.  clock=False leaves turn count and max turns out
        (transpositions reached in another number of moves match); wide=True adds a second, independent word.
        -> int64 [n] ([n, 2] with wide) on the device, no synchronisation: the key's BIT PATTERN (torch sorts and uniques int64)."""
        dev = self.device
        if observer is not None and int(observer) not in (-1, 0, 1):
            raise ValueError("observer must be None (the state key), 0 (each game's mover), +1 or -1")
        idx = None if index is None else torch.as_tensor(index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        n = self.num_envs if idx is None else int(idx.numel())
        keys = torch.empty((n, 2) if wide else (n,), dtype=torch.int64, device=dev)
        view = _lib.KEYS_VIEW_STATE if observer is None else int(observer)
        flags = (0 if clock else _lib.KEYS_NO_CLOCK) | (_lib.KEYS_WIDE if wide else 0)
        if n:
            with torch.cuda.device(dev):
                _lib.check(self._L.sgx_state_keys(self._h, _ptr(idx), n, view, flags, _ptr(keys), self._stream()), self._L)
        return keys

    def sample_valid_actions(self, mask=None, out=None):
        """Uniformly random valid action per env from `mask` (default: the current one) -- maenv:830-834."""
        own = mask is None or mask is self.mask
        mask = self.mask if mask is None else mask
        out = self.next_actions if out is None else out
        src = mask
        if own and self.compact:                 # the standalone sampler reads mask BYTES: expand the bit mask first
            self._mask_bytes = self.decode_mask(self._mask_bytes)
            src = self._mask_bytes
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_sample_valid(self._h, _ptr(src), _ptr(out), self._stream()), self._L)
        if own and out is self.next_actions:
            self._next_actions_fresh = True
        return out

    def export_state(self):
        """(state int64 [N,34,R,C] in the reference layout, player int8 [N])."""
        st = torch.empty((self.num_envs, NUM_STATE_LAYERS, self.R, self.Cc), dtype=torch.int64, device=self.device)
        pl = torch.empty((self.num_envs,), dtype=torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_export_state(self._h, _ptr(st), _ptr(pl), self._stream()), self._L)
        return st, pl

    def import_state(self, state, player=None):
        st = torch.as_tensor(state).to(device=self.device, dtype=torch.int64).contiguous()
        assert tuple(st.shape) == (self.num_envs, NUM_STATE_LAYERS, self.R, self.Cc)
        pl = None
        if player is not None:
            pl = torch.as_tensor(player).to(device=self.device, dtype=torch.int8).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_import_state(self._h, _ptr(st), _ptr(pl), self._stream()), self._L)
        self._next_actions_fresh = False
        return self.observe()

    def import_state_checked(self, state, player, sanitised):
        """import_state without the observe, reporting altered states in `sanitised` (uint8 [N], see sgx_import_state_checked)."""
        st = torch.as_tensor(state).to(device=self.device, dtype=torch.int64).contiguous()
        assert tuple(st.shape) == (self.num_envs, NUM_STATE_LAYERS, self.R, self.Cc)
        pl = None if player is None else torch.as_tensor(player).to(device=self.device, dtype=torch.int8).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_import_state_checked(self._h, _ptr(st), _ptr(pl), _ptr(sanitised), self._stream()), self._L)
        self._next_actions_fresh = False

    def env_info(self):
        """int32 [N,4]: turn count, game number, game_over, current player."""
        out = torch.empty((self.num_envs, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.sgx_get_env_info(self._h, _ptr(out), self._stream()), self._L)
        return out
