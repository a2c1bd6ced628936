/*
 * stratego_mi355x.h -- C ABI of libstratego_mi355x.so, the MI355X (gfx950) batched Stratego env.
 *
 * The reference (JBLanier/stratego_env) has no FFI: its seam is the Python class
 * StrategoProceduralEnv (stratego_env/game/stratego_procedural_env.py:20-181) under
 * StrategoMultiAgentEnv (stratego_env/stratego_multiagent_env.py:316-834).  Each entry point below
 * names the reference interface it replaces for a batch of N independent games.  Conventions:
 *   - plain C, no C++/torch types; every *_dev pointer is a DEVICE pointer owned by the caller
 *     (e.g. a torch tensor's data_ptr()); the library owns only its internal state tensor;
 *   - all device work is enqueued on `stream` (a hipStream_t passed as void*, NULL = default stream)
 *     and is asynchronous; the entry points that wait for the device are sgx_create, sgx_destroy,
 *     sgx_set_setup_table, sgx_set_start_pool, sgx_set_leaf_values, sgx_time_observe, sgx_mem_probe, sgx_store_probe, sgx_step_sync, sgx_host_free, sgx_alloc_outputs and
 *     sgx_free_outputs;
 *     every other entry point returns once its work is enqueued, whatever `stream` still holds, and every launch, memset and copy of a
 *     call that is more than one of them goes to `stream` (sgx_rollout and sgx_step_states with chains > 1 fork streams of the handle off
 *     `stream` and join them back into it: a consumer on `stream` sees every chain's games, and the chains see what `stream` held before
 *     the call).  One exception: a call may wait for the device when it is the FIRST of its kind on the handle or when its batch GROWS --
 *     it then allocates, or frees and reallocates, scratch of the handle (the chain streams of sgx_rollout / sgx_step_states, the flags
 *     and redo list of sgx_step_states, the count and scan scratch of sgx_count_moves when n_roots grows, the pointer table of
 *     sgx_step_ring with more than 8 sets when the ring gets longer, the completion word of sgx_step_sync, a kernel's first launch); a
 *     second call with the same shapes does not wait.  A ring of more than 8 sets may change from call to call, and one handle's ring
 *     calls may come from different streams, without a host wait: the table's uploads and readers are ordered on the device
 *     (tests/test_gpu_streams.py holds all of this, entry point by entry point);
 *   - return 0 on success, a negative SGX_E* code on failure (sgx_last_error() has the text);
 *     nothing throws across the ABI; invalid *actions* are not API errors: they are reported per env
 *     in invalid_action[] with that env's state left unchanged (the reference raises ValueError,
 *     stratego_procedural_impl.py:899-902 -- the Python facade turns the flag back into ValueError);
 *   - a handle is bound to one device and is not thread-safe; different handles are independent.  Every entry point runs on its
 *     handle's device and restores the calling thread's current HIP device before it returns (also on errors): one process may drive
 *     handles on several GPUs, and a caller inside a torch.cuda.device(...) scope keeps its device;
 *
 * Data layouts (C order):
 *   obs    float32 [N][R][C][67]   normalised partial observation of the env's NEXT mover, mover's
 *                                  perspective (impl:1335-1397 + maenv:261-313,388-391,506-508)
 *   mask   uint8   [N][R][C][K]    valid-actions mask of the next mover, K = 2(R-1)+2(C-1)+1
 *                                  (impl:399-517; the reference dtype is int64 with values 0/1)
 *   action int32   [N]             flat index into (R,C,K) in the MOVER's perspective (maenv:684-689)
 *   state  int64   [N][34][R][C]   the reference's own state layout, absolute coordinates (impl:16-60)
 */
#ifndef STRATEGO_MI355X_H
#define STRATEGO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGX_ABI_VERSION 15       /* (sgx_count_moves, sgx_expand_all and sgx_children_io are additions within v15: new entry points and a new
                                    struct, no existing layout or signature changed; sgx_playout_weighted is an addition within v15 too:
                                    a new entry point on sgx_playout_io as it is; so is sgx_determinize_weighted; so are sgx_step_vs and
                                    its sgx_vs_io) */
#define SGX_MAX_CELLS 1024       /* rows*cols <= 1024 (largest reference variant: 15x15 = 225; the reference's StrategoProceduralEnv
                                    takes any size, penv:27-36: boards of more than 256 cells use 10-bit cell indices in the record) */
#define SGX_PO_OBS_CHANNELS 67   /* impl:1332 */
#define SGX_FO_OBS_CHANNELS 79   /* impl:1227 */
#define SGX_PO_OBS_CHANNELS_ORIGINAL 32   /* impl:1148, obs_channel_mode='original' (maenv:67, 368-375) */
#define SGX_FO_OBS_CHANNELS_ORIGINAL 33   /* impl:1070 */
#define SGX_STATE_LAYERS 34      /* impl:109 */
#define SGX_OBS_LUT_STRIDE 16    /* entries per channel in the normalisation LUT */
#define SGX_MAX_PIECES_PER_TYPE 127   /* config 'piece_amounts' per piece type (the reference's dict is unbounded, config.py:3-23; a side
                                         never has more pieces than usable cells anyway) */

enum {
    SGX_OK = 0,
    SGX_EINVAL = -1,   /* bad argument / unsupported board size */
    SGX_ENOMEM = -2,   /* device allocation failed */
    SGX_EDEVICE = -3,  /* HIP runtime error (no device, launch failure, ...) */
    SGX_ESTATE = -4    /* call not valid in the handle's current state (e.g. no setup table) */
};

/* Game variant = one of the reference's *_STRATEGO_CONFIG dicts (game/config.py:3-313). */
typedef struct sgx_config {
    int32_t rows, cols;               /* >= 3 each (penv:28-30), rows*cols <= SGX_MAX_CELLS */
    int32_t max_turns;                /* config 'max_turns' -> StateData.MAX_TURNS (impl:247) */
    int32_t usable_rows;              /* config 'initial_state_usable_rows' */
    int32_t piece_counts[12];         /* config 'piece_amounts' for piece codes 1..12 (SPY..BOMB), <= SGX_MAX_PIECES_PER_TYPE each */
    int32_t capture_capacity;         /* most pieces ONE side can have on the board, 0 = sum of piece_counts.  An env_config that
                                         overrides 'piece_amounts' changes the normalisation constants only (maenv:323-326, 370-382)
                                         while the setups keep the version's pieces: sizes the capture-event list */
    uint8_t obstacles[SGX_MAX_CELLS]; /* config 'obstacle_locations' as a row-major rows*cols 0/1 map */
} sgx_config;

typedef struct sgx_env sgx_env; /* opaque handle */

/* Buffers of one batched step.  Replaces StrategoMultiAgentEnv.step(action_dict) (maenv:659-828) +
 * _get_current_obs (maenv:447-497) for N envs.  Nullable members may be NULL to skip that output. */
typedef struct sgx_step_io {
    const int32_t *actions_dev;    /* [N]   in : action of each env's current mover */
    float *obs_dev;                /* [N,R,C,67] out (nullable): partial observation (ObservationModes PARTIALLY / BOTH) */
    float *fobs_dev;               /* [N,R,C,79] out (nullable): fully-observable observation (FULLY / BOTH),
                                      impl:1230-1303 + maenv:202-258, 499-501 */
    uint8_t *mask_dev;             /* [N,R,C,K]  out (nullable) */
    float *reward_dev;             /* [N,2] out: rewards[+1], rewards[-1]; 0,0 while running (maenv:769, 777-805) */
    uint8_t *done_dev;             /* [N]   out: dones["__all__"] */
    int8_t *player_dev;            /* [N]   out: the next mover, +1 / -1 (after auto-reset: +1) */
    uint8_t *invalid_action_dev;   /* [N]   out: 1 where the reference would raise; state unchanged */
    uint8_t *ending_invalid_dev;   /* [N]   out: infos['game_result_was_invalid'] (max-turn tie, maenv:777-782) */
    float *final_obs_dev;          /* [N,2,R,C,67] out (nullable): on terminal steps, the terminal observation of
                                      player +1 (slot 0) and -1 (slot 1) (maenv:772-773); untouched otherwise */
    float *final_fobs_dev;         /* [N,2,R,C,79] out (nullable): the same for the fully-observable observation */
    int32_t *next_actions_dev;     /* [N] out (nullable): a uniformly random valid action for the next mover, drawn
                                      with the handle's counter RNG keyed by (seed, global env id, game, turn);
                                      the batched counterpart of sample_random_valid_action (maenv:830-834) */
    int32_t auto_reset;            /* 1: an env that finishes starts its next game inside the same call
                                      (obs/mask/player then describe the new game's first mover) */
    int32_t flags;                 /* SGX_STEP_* bits, 0 for the env.step() path */
} sgx_step_io;

/* Alignment of device pointers.  What each pointer needs follows from the widest store (or load) a kernel issues through it; every entry
 * point checks its pointers on the host BEFORE it launches anything and returns SGX_EINVAL with a message that names the pointer and the
 * alignment ("sgx_step: obs_dev must be 16-byte aligned").  A pointer that passes is handled at every phase it can then have:
 * tests/test_gpu_guard_bands.py runs each kernel family with its tensors at those phases between guard bands and finds no byte written
 * outside them.  "Quad boards" are those whose cell count rows*cols is a multiple of 4 (10x10, 8x8, 6x6, 4x4, 3x4), "odd boards" the rest
 * (15x15, 5x5).  Members of sgx_step_io, for sgx_step, sgx_step_sync, sgx_observe (its arguments of the same names), sgx_step_n,
 * sgx_step_ring (every set), sgx_step_traj (slot 0; the slots behind it are then as aligned), sgx_rollout, sgx_expand, sgx_step_states:
 *   actions_dev          4   (16 with SGX_STEP_ACTIONS_POSITIONS: one 16-byte load per game)
 *   next_actions_dev     4
 *   obs_dev              16 on quad boards (16-byte stores at 16-byte steps from the pointer), 4 on odd boards (any float phase: the
 *                        kernels write the partial first / last 16 bytes of a game as single floats); 16 with SGX_STEP_COMPACT_OBS
 *   fobs_dev             as obs_dev
 *   final_obs_dev        as obs_dev
 *   final_fobs_dev       as obs_dev
 *   mask_dev             1   (any address, on every board and for SGX_STEP_MASK_1D / SGX_STEP_MASK_STATE_COORDS: partial 16-byte chunks
 *                        of a game leave byte by byte unless the pointer is 4-byte aligned); 16 with SGX_STEP_COMPACT_MASK
 *   reward_dev           4
 *   done_dev             1
 *   player_dev           1
 *   invalid_action_dev   1
 *   ending_invalid_dev   1
 * The multi-step launches of the one-game-per-lane kernel (sgx_set_lane_kernel) additionally want 16-byte aligned obs_dev, mask_dev and
 * actions_dev and an 8-byte aligned reward_dev; a call that misses this is not an error: the wave-per-game kernels play it, with the same
 * results.  Other entry points:
 *   sgx_traj_io.actions_log_dev                               4
 *   sgx_decode_obs       compact_dev 16; obs_dev as above (16 on quad boards, 4 on odd boards)
 *   sgx_decode_mask      bits_dev 16; mask_dev 1
 *   sgx_sample_valid     mask_dev 1; actions_dev 4
 *   sgx_choose_actions   logits_dev 4; mask_dev 1 (4 with SGX_STEP_COMPACT_MASK); actions_dev 4
 *   sgx_export_state / sgx_import_state / sgx_import_state_checked / sgx_step_states:
 *                        state_dev, state_in_dev, state_out_dev 16 (the int64 layers travel as 16-byte loads / stores);
 *                        player_dev, player_in_dev, player_out_dev, sanitised_dev 1
 *   sgx_get_env_info     info_dev 16 (one 16-byte store per game)
 *   sgx_reset            env_select_dev, p1_maps_dev, p2_maps_dev 1
 *   sgx_set_start_index_out   start_index_dev 4
 *   sgx_expand / sgx_copy_envs   src_index_dev, dst_index_dev 4
 *   sgx_determinize              src_index_dev, hidden_dev 4
 *   sgx_determinize_weighted     src_index_dev, hidden_dev, off_belief_dev 4; belief_dev 4 (its rows are read as 2-byte elements; every
 *                                record's table starts an even number of elements behind it)
 *   sgx_playout                  src_index_dev, reward_dev, length_dev 4; done_dev, ending_invalid_dev, player_dev 1
 *   sgx_playout_weighted         as sgx_playout; `weights` is HOST memory, read before the call returns (any uint16_t alignment): the
 *                                contract has nothing to add for it
 *   sgx_step_vs                  src_index_dev, actions_dev, reward_dev, reply_action_dev 4; agent_dev, done_dev, ending_invalid_dev, player_dev,
 *                                invalid_action_dev, moved_dev 1; `weights` is HOST memory, as for sgx_playout_weighted
 *   sgx_replay                   src_index_dev, actions_dev, lengths_dev, applied_dev, consumed_dev, reward_dev 4; stop_dev, done_dev, ending_invalid_dev, player_dev 1
 *   sgx_set_replay_origins       origin_in_dev, origin_out_dev 4 (their elements are read and written as 2-byte values; an odd board's rows
 *                                start at any 2-byte phase from there)
 *   sgx_count_moves              src_index_dev, counts_dev 4; offsets_dev 16
 *   sgx_expand_all               src_index_dev, parent_dev, action_dev, reward_dev 4; offsets_dev 16; done_dev, ending_invalid_dev, player_dev 1
 *   sgx_state_keys               src_index_dev 4; keys_dev 8 (16 with SGX_KEYS_WIDE: one 16-byte store per record)
 *   sgx_mem_probe        ptr_dev 1024;   sgx_store_probe   ptr_dev 16
 * Change note: these rejections are new error returns for pointers that were never legal (the stores they guard were issued unchecked
 * before; only sgx_decode_obs and the compact path refused them); no struct or signature changed, so SGX_ABI_VERSION stays. */

/* sgx_step_io.flags: the functional StrategoProceduralEnv API on caller-provided states (import -> step -> export) */
#define SGX_STEP_ACTIONS_1D 1         /* actions_dev holds absolute-coordinate 1-D indices (impl:262-277), as
                                         get_next_state / is_move_valid_by_1d_index take them (penv:94-99, 148-155) */
#define SGX_STEP_ALLOW_OSCILLATION 2  /* allow_piece_oscillation=True: skip the two-square check of the MOVE (impl:771-777);
                                         masks still apply it, as in the reference */
#define SGX_STEP_RAW_OBS 4            /* observations un-normalised, as penv:166-173 return them */
#define SGX_STEP_ACTIONS_POSITIONS 8   /* actions_dev is int32 [N][4] = (start_r, start_c, end_r, end_c) in absolute coordinates
                                         (is_move_valid_by_position, penv:87-92) */
/* env_config['obs_channel_mode'] == 'original' (maenv:67, 368-375, 465-467, 484-486): the deprecated value-channel
 * observations.  obs_dev / final_obs_dev then have 32 channels (impl:1126-1197) and fobs_dev / final_fobs_dev 33
 * (impl:1048-1123), normalised with the constants of maenv:87-199. */
#define SGX_STEP_ORIGINAL_CHANNELS 16
/* Masks of the functional API are indexed in the coordinates of the given STATE, not in the mover's perspective:
 * SGX_STEP_MASK_1D: mask_dev is uint8 [N][R*C*(R+C)+1], get_valid_moves_as_1d_mask (penv:74-80, impl:520-642) of the current mover;
 * SGX_STEP_MASK_STATE_COORDS: mask_dev is uint8 [N][R][C][K] as get_valid_moves_as_spatial_mask(state, player) returns it for
 * the current mover WITHOUT the perspective flip (penv:127-128, impl:399-517; identical to the default for player +1).
 * Both are also accepted by sgx_observe; they cannot be combined with fobs_dev / final_fobs_dev or SGX_STEP_ORIGINAL_CHANNELS. */
#define SGX_STEP_MASK_1D 32
#define SGX_STEP_MASK_STATE_COORDS 64

/* Compact outputs (opt-in; never the default).  The float32 observation is 85 % of a step's bytes and the step kernel already sits on
 * the write roofline, so the only way past it is to write less: with SGX_STEP_COMPACT_OBS obs_dev receives, per game, the kernel's own
 * 4-bit code buffer -- uint8 [N][sgx_compact_obs_stride(h)]: ceil(R*C*67 / 2) bytes of codes (nibble e = float e of the [R,C,67]
 * observation, low nibble first; code c decodes to sext(c) / 4, code 8 marks an entry without a code), padded to 16 bytes; a 16-byte
 * header {int32 n, 0, 0, 0}; n x {uint32 entry, float32 value} for the marked entries (captured counts that normalise to thirds /
 * fifths); padded to whole 128-byte lines (10x10: 3,584 B for Barrage instead of 26,800 B).  With SGX_STEP_COMPACT_MASK mask_dev
 * receives the mask as bits, uint32 [N][sgx_compact_mask_words(h)], bit a of the game's words = flat action a (10x10: 480 B instead of
 * 3,700 B).  sgx_decode_obs / sgx_decode_mask expand a batch of them with the step kernel's own emission code: the float32 / uint8
 * results are byte-identical to what the step writes without the flags (tests/test_gpu_compact.py).  Accepted by sgx_step, sgx_observe,
 * sgx_step_n, sgx_rollout and sgx_step_ring for the 67-channel partial observation of an 'extended' channel mode and masks in the
 * mover's perspective (no fobs_dev / final_obs_dev / original channels / state-coordinate masks; 16-byte aligned buffers).  No reference
 * counterpart: the reference's contract is the float32 observation (impl:1335-1397 + maenv:506-508), which the decode ops deliver. */
#define SGX_STEP_COMPACT_OBS 128
#define SGX_STEP_COMPACT_MASK 256
int64_t sgx_compact_obs_stride(const sgx_env *h);
int64_t sgx_compact_mask_words(const sgx_env *h);
int sgx_decode_obs(sgx_env *h, const uint8_t *compact_dev, float *obs_dev /* [N,R,C,67] */, void *stream);
int sgx_decode_mask(sgx_env *h, const uint32_t *bits_dev, uint8_t *mask_dev /* [N,R,C,K] */, void *stream);

/* Library / geometry queries (penv:32-36: action_size, spatial_action_size). */
int sgx_abi_version(void);
/* Hash of the sources the loaded binary was compiled from (the first 16 hex digits of SHA-256 over the files of stratego_env_amd/csrc and this
 * header, stratego_env_amd/build.py: source_hash; "unknown" for a build outside build.py).  The Python binding refuses a library whose
 * id differs from the sources next to it, bench.py and smoke() print it: the tested binary is tied to the tested source.  The same
 * string follows the marker "SGX_BUILD_ID=" in the file, so it can be read without loading the library. */
const char *sgx_build_id(void);
/* 1 if kernels for this board size are compiled into the library.  Every reference variant is (10x10, 15x15, 8x8, 6x6, 5x5, 4x4, 3x4);
 * the reference's StrategoProceduralEnv(rows, columns) takes ANY size >= 3 (penv:27-36): for other sizes (rows * cols <= SGX_MAX_CELLS)
 * the same sources are compiled into a library of their own with -DSGX_EXTRA_R=<rows> -DSGX_EXTRA_C=<cols> -DSGX_ONLY_EXTRA
 * (stratego_env_amd/build.py build_geometry does it on first use). */
int sgx_supports_geometry(int32_t rows, int32_t cols);
const char *sgx_last_error(void);
int64_t sgx_num_envs(const sgx_env *h);
/* Bytes of one game's packed state record in device memory (a multiple of 128: 512 for Barrage, 640 for
 * Standard).  One env.step() reads it once and writes it once: with the outputs it is the byte minimum B_min of a step that bench.py's
 * roofline is priced on.  No reference counterpart (the reference's state is int64 [34,R,C] = 27,200 B at 10x10, impl:69-163). */
int64_t sgx_record_bytes(const sgx_env *h);
int sgx_spatial_channels(const sgx_env *h);          /* K */
int64_t sgx_num_spatial_actions(const sgx_env *h);   /* R*C*K = Discrete(n) of maenv:362 */
int64_t sgx_action_size_1d(const sgx_env *h);        /* R*C*(R+C)+1 (impl:252-254) */

/* Host-only: fills lut[67*SGX_OBS_LUT_STRIDE] with the float32 bit-exact normalised value of every
 * (channel, raw integer value) pair: entry [ch*16 + clamp(v + bias_ch, 0, 15)] where bias is 3 for the two
 * recent-moves channels (raw -3..1) and 0 elsewhere.  Replaces the arithmetic of
 * normalize_p_observation (maenv:506-508) with the constants of maenv:261-313, 388-391. */
int sgx_build_obs_lut(const sgx_config *cfg, float *lut);
/* Same for the 79 fully-observable channels: lut[79*SGX_OBS_LUT_STRIDE] (maenv:202-258, 393-396, 499-501). */
int sgx_build_full_obs_lut(const sgx_config *cfg, float *lut);
/* Same for obs_channel_mode='original': lut[32*SGX_OBS_LUT_STRIDE] (full == 0; maenv:146-199) or
 * lut[33*SGX_OBS_LUT_STRIDE] (full != 0; maenv:87-143). */
int sgx_build_original_obs_lut(const sgx_config *cfg, int32_t full, float *lut);

/* StrategoMultiAgentEnv.__init__ (maenv:318-445) for a batch: allocates the device state of n_envs games on
 * `device`.  Env i of this handle has global id env_id_offset + i; all random draws are keyed by
 * (seed, global id, game number, turn), so trajectories do not depend on how the batch is sharded.
 * A limit of the key: the RNG's first mix takes seed + 0x9E3779B97F4A7C15 * (global id + 1), so (seed, g) and
 * (seed + 0x9E3779B97F4A7C15, g - 1) name the same stream: two handles whose seeds differ by exactly that constant (mod 2^64) play the
 * same games shifted by one env id.  Seeds that differ by anything else -- s + 1, s + (1 << 32) -- give independent games
 * (tests/test_draws_cpu.py, tests/test_gpu_draws.py).  The arithmetic stays as it is: recorded trajectories are keyed on it.
 * n_envs must lie in [1, 2^30]: anything else is SGX_EINVAL before the device is touched.  The bound is what keeps every 32-bit
 * quantity of a launch in range -- the grid size, the XCD shares xcd_first / xcd_count, one workgroup per game in sgx_reset and
 * sgx_sample_valid; the byte offsets of games, slots, records and lists are 64-bit everywhere (tests/test_gpu_big_offsets.py). */
int sgx_create(const sgx_config *cfg, int64_t n_envs, int device, uint64_t seed, int64_t env_id_offset, sgx_env **out);
int sgx_destroy(sgx_env *h);

/* Store policy of the observation writes of sgx_step / sgx_observe.  Lines a wave writes whole can leave as non-temporal stores:
 * faster when a launch's observations do not fit the 256 MiB Infinity Cache, slower when they do.
 * mode -1 (default): decided per launch from the observation bytes it writes (> 300 MB: non-temporal); 0: never; 1: always.
 * The environment variable SGX_NT=0|1|auto sets the default of handles created afterwards.  Results are identical in every
 * mode (tests/test_gpu_nt_stores.py runs the parity suites with the mode forced).  No reference counterpart. */
int sgx_set_nt_stores(sgx_env *h, int32_t mode);

/* Kernel choice on boards of at most 16 cells with a multiple of 4 cells (Micro 3x4, Tiny 4x4).  A second kernel plays ONE GAME PER LANE
 * there (64 games per wave, boards as nibbles in registers; docs/DESIGN_rounds_4-5.md section 3.3).  It is eligible for sgx_step / sgx_observe / sgx_step_n /
 * sgx_rollout / sgx_step_ring calls that ask for the 67-channel partial observation of an 'extended' channel mode (or none), masks in the
 * mover's perspective, no terminal-observation buffers and 16-byte aligned output tensors.  Measured: its game logic is twice as fast
 * (65,536 Micro games without outputs 13 against 26 us, mask only 15 against 30 us), but with the observation emitted one launch is slower
 * (51 against 42 us: one wave per SIMD, nothing overlaps its logic with its stores).  mode -1 (default): the lane kernel for eligible
 * calls that emit NO observation, the wave-per-game kernel otherwise; 0: never; 1: for every eligible call.  SGX_LANE=0|1|auto sets the
 * default of handles created afterwards.  Results are identical either way (tests/test_gpu_lane_kernel.py).  No reference counterpart. */
int sgx_set_lane_kernel(sgx_env *h, int32_t mode);

/* Multi-step launches.  A rollout call -- sgx_step_n / sgx_step_ring: n_steps >= 2 consecutive steps, each playing the action the one
 * before drew -- runs its steps in ONE launch (launches of at most 256 steps, on every board) where it is eligible: flat perspective actions,
 * masks in the mover's perspective, an 'extended' channel mode, output sets that differ in their observation / mask tensors only (any number
 * of them: beyond 8 sets sgx_step_ring passes their pointers through a small device table; a trajectory buffer in ONE allocation goes through
 * sgx_step_traj, which names its slots by a stride).
 *  - Boards of more than 16 cells (steps_kernel): a workgroup stages its games once and every wave plays its game step after step -- the
 *    dense boards, never-moved flags, recent-move codes and capture events stay in LDS, the record's scalars and the drawn action in
 *    registers; every step's outputs are written like those of a launch of its own; the record is read once and written once per LAUNCH.
 *    No barrier after the prologue: the waves drift out of phase, one wave's stores run under another's game logic.  The 67-channel kind,
 *    BOTH observations, compact outputs and calls without an observation.  65,536 Barrage games into a ring of three output sets:
 *    284-287 -> 246-249 us per step; 262,144 Standard games 1,210-1,233 -> 977-991 us (DESIGN.md sections 3 and 4).
 *  - Boards of at most 16 cells with a multiple of 4 cells, the 67-channel kind with an observation tensor (lane_steps_kernel): a 256-thread
 *    workgroup keeps 64 games in the registers of one wave, which plays step t + 1 while the other three waves store the observations of
 *    step t.  65,536 Micro games 42.1 -> 29.2 us per step.
 * Same results as n_steps launches of sgx_step (tests/test_gpu_multi_step.py, tests/test_gpu_lane_kernel.py).  mode 1 (default): on; 0: one
 * launch per step.  SGX_MULTI_STEP=0 sets the default of handles created afterwards (SGX_MULTI_STEP_WAVE=0: the first kind only off);
 * sgx_set_lane_kernel(h, 0) switches the second kind off as well.  No reference counterpart. */
int sgx_set_multi_step(sgx_env *h, int32_t mode);
/* Launches that write NO observation (sgx_expand, mask-only and logic-only steps / rollouts: no obs_dev / fobs_dev / final_*_dev, no compact
 * outputs) are bound by instruction issue, not by memory; on boards of 33 .. 128 cells they play TWO games per wave (32 lanes per game): 65,536
 * Barrage games, logic-only rollout 60.6 -> 33.7 us per step, search expansion 0.96 -> 1.75 G states/s.  Same results
 * (the parity suites of the no-observation kind run on it).  mode 1 (default): two games per wave where the board allows it; 0: one game
 * per wave everywhere (A/B measurements: tools/half_wave_ab.py).  The environment variable SGX_HALF_WAVE=0|1 sets the default of handles
 * created afterwards.  No reference counterpart. */
int sgx_set_half_wave(sgx_env *h, int32_t mode);
/* Multi-step launches of the wave-per-game kernel (sgx_step_n / sgx_step_ring / sgx_step_traj on boards of more than 16 cells): should the waves of a
 * workgroup -- 8 adjacent games -- meet at a barrier before every step?  Without it they drift apart within a few steps, which lets one wave's
 * stores run under another's game logic; on a LONG ring or trajectory buffer that drift spreads a workgroup's writes over up to 8 sets at a time,
 * and a launch whose resident waves cycle through more sets than the address translation caches hold pages for runs 1-7 %
 * faster with the waves in step (64-slot trajectory buffer of 65,536 Barrage games: 295 -> 282 us per step).  mode -1 (default): the barrier where
 * it was measured to pay -- float32 observations, one game per wave (36 .. 225 cells), from 9 sets / slots on 10x10 and from 16 elsewhere; 0: never;
 * 1: in every multi-step launch (A/B runs and the parity tests).  Same results in every mode (tests/test_gpu_multi_step.py).
 * SGX_STEPS_BARRIER=-1|0|1 sets the default of handles created afterwards.  No reference counterpart. */
int sgx_set_steps_barrier(sgx_env *h, int32_t mode);

/* Which kernel the handle's last sgx_step / sgx_observe / sgx_step_n / sgx_step_ring / sgx_rollout / sgx_expand launch was (diagnostics,
 * benchmarks that price a launch by its own bytes, tests that must not pass on another kernel): */
#define SGX_LAUNCH_WAVE 0        /* one wave per game (boards of up to 32 cells: a wave's lanes shared by 2 or 4 games), one launch per step */
#define SGX_LAUNCH_LANE 1        /* one game per lane (boards of at most 16 cells), one launch per step */
#define SGX_LAUNCH_MULTI_STEP 2  /* one game per lane, all steps of the call in one launch (sgx_set_multi_step) */
#define SGX_LAUNCH_MULTI_STEP_WAVE 3   /* one wave per game, all steps of the call in one launch: the boards stay in LDS between the steps */
#define SGX_LAUNCH_PLAYOUT 4     /* sgx_playout: one wave per game, every move of the playout in one launch (set on dst) */
#define SGX_LAUNCH_REPLAY 5      /* sgx_replay: one wave per game, every entry of the action list in one launch (set on dst) */
#define SGX_LAUNCH_CHILDREN 6    /* sgx_expand_all: one wave per child, root found from the offsets, mask regenerated, move applied (set on dst) */
#define SGX_LAUNCH_PLAYOUT_WEIGHTED 7   /* sgx_playout_weighted: sgx_playout's launch with the weighted draw (set on dst) */
#define SGX_LAUNCH_REPLAY_TRACKED 8      /* sgx_replay while dst has sgx_set_replay_origins set: sgx_replay's launch, with the piece labels (set on dst) */
#define SGX_LAUNCH_STEP_VS 9             /* sgx_step_vs: one wave per game, the agent's move and the bot's reply in one launch (set on dst) */
int sgx_last_launch_kind(const sgx_env *h);

/* Shares of the eight XCDs in a launch of sgx_step / sgx_observe.  Under a saturating write stream the odd XCDs of MI355X drain their
 * eighth of the games ~20 % slower than the even ones, so with equal eighths the even XCDs idle at the end of every launch; the
 * library gives the even XCD of each pair `per_mille` more than the mean share and the odd one as much less (DESIGN.md section 3:
 * -3 ... -5 % launch time where the write stream bounds the kernel: 8x8 and 10x10 boards; +3 ... +7 % where the game logic shares the
 * critical path: 6x6, 15x15, Micro).  -1 (default): 100 per mille on boards of 64 .. 100 cells when a launch's observations do not fit
 * the Infinity Cache, equal shares otherwise; 0: always equal; 1 .. 900: always that.  SGX_XCD_SKEW=<per mille>|auto sets the default of
 * handles created afterwards.  Which workgroup plays which game cannot change any result.  No reference counterpart. */
int sgx_set_xcd_skew(sgx_env *h, int32_t per_mille);
/* The general form: a share per XCD, per mille of the mean share (NULL: back to the sgx_set_xcd_skew rule); sgx_get_xcd_shares returns
 * what a streaming launch of the handle uses (*explicit_out, nullable: 1 if set by sgx_set_xcd_shares). */
int sgx_set_xcd_shares(sgx_env *h, const int32_t *per_mille /* [8] or NULL */);
int sgx_get_xcd_shares(sgx_env *h, int32_t *per_mille /* [8] */, int32_t *explicit_out);

/* Upload a human-setup table (game/inits/{barrage,standard}_human_inits.py decoded to piece codes, util.py:154-180):
 * table_host is uint8 [n_setups][usable_rows*cols] in Gravon string order.  Replaces get_random_human_init_fn
 * (util.py:301-319).  Without a table, sampled resets place pieces uniformly at random in the usable rows
 * (get_random_initial_state_fn, util.py:13-53). */
int sgx_set_setup_table(sgx_env *h, const uint8_t *table_host, int64_t n_setups);

/* reset() (maenv:513-657) for the envs selected by env_select_dev (uint8 [N], NULL = all).
 * p1_maps_dev / p2_maps_dev: int8 [N][R*C] own-side piece maps, the inputs of create_initial_state
 * (penv:38-60 -> impl:211-249); pass NULL for both to sample setups (table or random placement).
 * Starts game number 0 (explicit maps) or the env's next game number (sampled).  Player +1 moves first -- unless the handle has a
 * start pool (sgx_set_start_pool below): NULL maps then start every selected env from a pool record, with that record's first mover. */
int sgx_reset(sgx_env *h, const uint8_t *env_select_dev, const int8_t *p1_maps_dev, const int8_t *p2_maps_dev, void *stream);

/* Start pools: games that start from GIVEN positions instead of sampled setups -- the reference's curriculum start states
 * (curriculum_start_states_path, maenv:519-527; get_random_curriculum_init_fn, util.py:374-387), endgame training, evaluation from fixed
 * test positions, search roots -- without leaving the batched path.  (Added without a struct or signature change: SGX_ABI_VERSION stays.)
 *
 * sgx_set_start_pool COPIES records [0, n_pool) of `pool` -- a handle of the same variant, board and device, typically one filled through
 * sgx_import_state_checked or sgx_copy_envs -- into a buffer `h` owns (the pool handle may be destroyed or rewritten afterwards); pool =
 * NULL clears it.  It waits for the device, and a previous buffer is freed only then.  While a pool is set, EVERY game start that would
 * sample a setup -- sgx_reset with NULL maps (with or without env_select_dev) and every auto-reset of sgx_step, sgx_step_sync, sgx_step_n,
 * sgx_rollout, sgx_step_ring and sgx_step_traj, also in the middle of a multi-step launch -- instead
 *   1. draws j = rng_below(r, n_pool), r = the counter RNG's value for (seed, env_id_offset + env, game_no, stream STREAM_POOL = 4,
 *      counter 0): a stream of its own, no other draw moves; game_no is the env's own counter, advanced exactly as without a pool;
 *   2. loads record j whole: the four stored boards, the never-moved bitmaps, turn, max_turns, the recent-move pairs and the capture
 *      events with their count; the env's game_no replaces the record's and the flags become the mover bit alone;
 *   3. takes the record's mover as the first mover, or with SGX_POOL_RANDOM_FIRST_PLAYER (maenv:523) player -1 when
 *      rng_below(r', 2) == 1 (r': the same stream, counter 1), else +1;
 *   4. writes the mask, the observation, the sampled next action and player_dev of THAT position and mover.
 * SGX_POOL_RESTART_CLOCK (util.py:382-383: turn = 0, max_turns = the handle's) is applied ONCE, to the private copy.
 * Explicit maps passed to sgx_reset still win over the pool; with no pool set nothing changes anywhere, and clearing the pool restores
 * that behaviour bit for bit.  While a pool is set, sampled setups need not be possible (the "more pieces than usable cells" refusal of
 * sgx_reset / auto_reset applies only without one).  SGX_EINVAL, with nothing launched, for: a pool of another variant, board, record
 * size or device; n_pool < 1 or larger than the pool handle; an unknown flag; a record whose game is over (the message names the first
 * such index).  Not covered (SGX_EINVAL while a pool is set): auto_reset in launches with SGX_STEP_MASK_1D / _MASK_STATE_COORDS and in
 * sgx_step_states.  sgx_start_pool_size: n_pool, 0 = none.
 *
 * sgx_set_start_index_out: int32 [N] (NULL = none) that every sgx_reset and every step of a handle WITH a pool (not: sgx_observe, sgx_expand,
 * sgx_step_states and steps with SGX_STEP_MASK_1D / _MASK_STATE_COORDS, which run the ordinary kernels and leave it alone) writes the pool index of
 * the env's CURRENT game into -- the game its new observation belongs to.  (A game that explicit maps started has no pool index: sgx_reset
 * writes -1 for it, and its steps write the draw of its game number, which names no start.)  Addressed like
 * sgx_step_io.done_dev: sgx_step_traj with results_per_slot writes step t's at start_index_dev[env + slot * slot_envs] (the buffer is
 * then [n_slots][slot_envs]); at a slot with done = 1 the FINISHED game's index is the previous slot's.  The index is a function of
 * (seed, env id, game number): a snapshot restored under the same pool reproduces it. */
#define SGX_POOL_RANDOM_FIRST_PLAYER 1
#define SGX_POOL_RESTART_CLOCK       2   /* turn = 0, max_turns = the handle's: util.py:382-383 */
int sgx_set_start_pool(sgx_env *h, sgx_env *pool /* NULL = clear */, int64_t n_pool, int32_t flags);
int sgx_set_start_index_out(sgx_env *h, int32_t *start_index_dev /* NULL = none */);
int64_t sgx_start_pool_size(const sgx_env *h);   /* 0 = none */

/* _get_current_obs (maenv:447-497) for every env's current mover, no state change.
 * obs_dev, fobs_dev, mask_dev and player_dev are laid out as in sgx_step_io; each is nullable.
 * flags: 0 or any of SGX_STEP_RAW_OBS, SGX_STEP_ORIGINAL_CHANNELS, SGX_STEP_MASK_1D, SGX_STEP_MASK_STATE_COORDS. */
int sgx_observe(sgx_env *h, float *obs_dev, float *fobs_dev, uint8_t *mask_dev, int8_t *player_dev, int32_t flags, void *stream);

/* Average duration in microseconds of `launches` sgx_observe calls writing obs_dev / mask_dev (either may be NULL), measured
 * with HIP events on `stream`; synchronises that stream.  The caller owns the output buffers, and on MI355X the same kernel
 * runs 312-400 us depending on WHICH allocation the observation buffer is: a host allocates a few
 * candidates, times each with this call and keeps the fastest (what VecStrategoEnv.tune_placement does from Python).
 * No reference counterpart. */
int sgx_time_observe(sgx_env *h, float *obs_dev, uint8_t *mask_dev, int32_t launches, void *stream, float *microseconds);

/* Write-stream rate (GB/s) of the device memory range [ptr_dev, ptr_dev + bytes) under the step kernel's store pattern: one wave
 * per 26 KiB segment, 1 KiB non-temporal store instructions, eight concurrent fronts -- the observation stream without the game.
 * OVERWRITES the range.  On MI355X device memory comes in large regions of two kinds that differ by ~25 % under this pattern (and
 * not under a sequential fill); a host that allocates its own output tensors can tell with this call which kind
 * an allocation is.  ptr_dev 1 KiB aligned; `launches` timed launches after one untimed; synchronises `stream`.  No reference
 * counterpart. */
int sgx_mem_probe(int device, void *ptr_dev, int64_t bytes, int32_t launches, void *stream, float *gb_per_s);

/* The store stream of the step kernel WITHOUT the game, for pricing the roofline against what the memory takes from exactly this store
 * shape (bench.py: roofline.store_peak_measured).  One wave per `seg_bytes` segment (a multiple of 16; 26,800 = one 10x10 observation),
 * eight waves per 512-thread workgroup at 6 waves per SIMD, workgroups mapped to segments like games to workgroups (eight contiguous XCD
 * ranges); a wave sweeps its segment in 16-byte-per-lane store instructions on 1 KiB ADDRESS boundaries, whole 128-byte lines
 * non-temporal, the two edge lines a segment shares with its neighbours through L2 -- emit_codes' pattern (sgx_obs.h).  The range
 * [ptr_dev, ptr_dev + bytes) holds floor(bytes / seg_bytes) segments; ONE launch writes all of them `passes` times, pass after pass, so a
 * launch of passes x bytes >> 288 MB (L2 + Infinity Cache) leaves a negligible share of its bytes in the caches when it ends.
 * payload: 0 = zeros, 1 = observation-like floats (0 / 1 / -1 / 0.5 from a per-lane code pattern), 2 = incompressible bits (a hash of
 * the address and the launch number).  nt_stores: 0 = plain stores, 1 = whole lines non-temporal, N >= 2 = every N-th 1 KiB sweep plain and the
 * others non-temporal (the step kernel's own mix: its mask leaves as plain stores through L2).  How many store streams the memory sees at once is the probe's other axis -- the step kernel's waves
 * do not store back to back: waves_per_cu = resident waves per CU (0 = the kernel's own 24; 16 or 8: fewer resident workgroups), pace =
 * sleeps of 64 cycles after every 1 KiB sweep (0 .. 4096), persistent != 0 = a grid of the RESIDENT workgroups only, every wave walking
 * segment after segment for the whole launch (long-lived waves, like the multi-step kernel's; 0 = one short-lived workgroup per eight
 * segments and pass, like one launch per step); dwell > 1 (persistent waves only) = a wave writes its segment `dwell` times before it moves
 * on, cycling through `ring` (1 .. 8) equal sub-ranges of the buffer -- a wave of the multi-step kernel rewrites its game's observation
 * step after step, in place or into the sets of a ring; a launch then writes passes x dwell x (one sub-range's segments).  bench.py sweeps
 * these and reports the best rate of the non-rewriting configurations as roofline.store_peak_measured.
 * OVERWRITES the range.  Returns the average duration of `launches` timed launches (HIP events on `stream`, one untimed launch first;
 * synchronises the stream) and bytes written per launch / that time.  No reference counterpart. */
#define SGX_PROBE_ZEROS 0
#define SGX_PROBE_OBS_LIKE 1
#define SGX_PROBE_RANDOM 2
int sgx_store_probe(int device, void *ptr_dev, int64_t bytes, int32_t seg_bytes, int32_t passes, int32_t payload, int32_t nt_stores,
                    int32_t waves_per_cu, int32_t pace, int32_t persistent, int32_t dwell, int32_t ring, int32_t launches, void *stream,
                    float *microseconds_per_launch, float *gb_per_s);

/* Library-owned output buffers with a bounded placement trial.  On MI355X the same launch takes
 * 313-400 us depending on which physical memory backs the big observation buffer: device memory comes in regions of two
 * kinds, a buffer lying inside one region runs at that region's rate (~350 or ~380-395 us for 65,536 Barrage games), and
 * only a buffer whose pages MIX both kinds reaches the fast class (313-325 us).  Which one a plain allocation gets depends
 * on what was allocated before it.  sgx_alloc_outputs allocates the mask buffer, then tries up to `max_trials` candidate
 * allocations of the observation buffer (and of the fully-observable one with SGX_OUT_FULL_OBS): before each candidate a
 * padding allocation of growing size (steps of an eighth of the buffer, or -- under a budget wider than `max_trials` such steps -- of
 * the budget divided by the number of candidates, so that a generous budget is sampled evenly) is made and released again afterwards,
 * which moves the candidate to other buddy blocks;
 * each candidate is timed with a few sgx_observe launches (no state change) and only the fastest so far is kept.  The trial
 * stops early once the kept candidate is >= 17 % faster than the slowest one seen (the fast class), or eight candidates after the first one
 * that is >= 9 % faster.  At no time does the trial hold more than `max_extra_bytes`
 * beyond the buffers it returns (0 or max_trials <= 1: no trial, first allocation).  Channel counts follow `flags` (SGX_STEP_ORIGINAL_CHANNELS).  Waits for the device.  No reference counterpart. */
#define SGX_OUT_FULL_OBS 1024         /* also allocate fobs_dev [N,R,C,79] (or 33) */
#define SGX_OUT_MAX_TRIALS 64
typedef struct sgx_outputs {
    float *obs_dev;                /* [N,R,C,67] (32 with SGX_STEP_ORIGINAL_CHANNELS) */
    float *fobs_dev;               /* [N,R,C,79] (33) or NULL */
    uint8_t *mask_dev;             /* [N,R,C,K] */
    int64_t obs_bytes, fobs_bytes, mask_bytes;
    int64_t peak_extra_bytes;      /* most memory the trial held beyond the returned buffers */
    int32_t n_trials, n_ftrials;   /* candidates timed for obs_dev / fobs_dev */
    float trial_us[SGX_OUT_MAX_TRIALS];    /* sgx_observe launch time with each obs candidate; [0] = the plain first allocation */
    float ftrial_us[SGX_OUT_MAX_TRIALS];   /* the same for fobs_dev */
    int32_t device;                /* the device the buffers live on (sgx_free_outputs works without the handle) */
    int32_t reserved_;
} sgx_outputs;
int sgx_alloc_outputs(sgx_env *h, int32_t flags, int64_t max_extra_bytes, int32_t max_trials, void *stream, sgx_outputs *out);
/* A target for the searches that follow: with target_us > 0 sgx_alloc_outputs keeps trying candidates (inside its budget) until one is
 * within 3 % of the target instead of applying its own stop rules -- for a RING of output sets (sgx_step_ring), whose every set should
 * be as fast as the first one (target = the observe-launch time the first search kept); 0 (default) = the stop rules above. */
int sgx_set_placement_target(sgx_env *h, float target_us);
/* Frees the buffers of `out` (h may be NULL, also after sgx_destroy of the handle that allocated them: the buffers belong to
 * whoever holds the sgx_outputs -- the Python binding ties them to the tensors that view them). */
int sgx_free_outputs(sgx_env *h, sgx_outputs *out);

/* One batched env.step(): see sgx_step_io. */
int sgx_step(sgx_env *h, const sgx_step_io *io, void *stream);

/* Single-game latency (config 1: one game behind the reference's dict API).  sgx_host_alloc returns pinned host memory the device
 * can address (*dev_ptr is its device alias): with sgx_step_io's output pointers -- and actions_dev -- pointing into it the step
 * kernel writes a game's ~30 KB of outputs straight to host memory, and sgx_step_sync (= sgx_step + wait until the outputs are
 * complete) makes env.step() ONE library call: no upload, no download, no second launch.  Meant for a handful of games; batches
 * belong in HBM.  Up to 8 games on a board of more than 32 cells with a multiple of 4 cells, 'extended' channel modes, are played by a
 * kernel of their own -- one workgroup per game: one wave plays the move, all eight emit the mask and the observations -- which
 * publishes its completion in a host-mapped word that sgx_step_sync polls -- spinning for about a millisecond (a step is ~6 us), then
 * yielding the core between polls, then backing off to sleeps of 2 ... 64 us, looking at the stream so that a failed launch ends the
 * wait: a long wait costs the host next to nothing -- and the call returns when the outputs are visible to the host,
 * typically before `stream` has retired the kernel (later work on `stream` is ordered behind it as usual).  Every other case is
 * sgx_step + hipStreamSynchronize.  Same results either way (tests/test_gpu_step_sync.py).
 * No reference counterpart (the reference is one game per object on the host, maenv:659-828). */
int sgx_host_alloc(sgx_env *h, int64_t bytes, void **host_ptr, void **dev_ptr);
int sgx_host_free(sgx_env *h, void *host_ptr);
int sgx_step_sync(sgx_env *h, const sgx_step_io *io, void *stream);

/* n_steps consecutive sgx_step calls with the same buffers, enqueued back to back without returning to the host language (ONE launch for
 * all of them where the call is eligible: sgx_set_multi_step): the random-action game loop of examples/basic_game_loop.py:34-63 (sample a valid action, step, repeat) for N games.
 * Requires io->next_actions_dev == io->actions_dev, so that every step plays the action the previous one drew; the
 * output buffers hold the last step's results afterwards.  (Toy boards finish a batched step in tens of microseconds:
 * driving them one call at a time from Python is launch-bound.) */
int sgx_step_n(sgx_env *h, const sgx_step_io *io, int32_t n_steps, void *stream);

/* sgx_step_n over a RING of output sets: step i of the call writes its outputs through ios[(first_set + i) % n_sets] -- a rollout
 * into a trajectory buffer that keeps the last n_sets steps' observations and masks (what a learner stores per step) instead of
 * overwriting one set in place.  Every set must name the same actions_dev == next_actions_dev (the one chain of drawn actions) and the
 * same auto_reset / flags.  With n_sets sets of a size whose sum exceeds the 256 MiB Infinity Cache, no line written by one step can
 * still sit in that cache when it is written again: bench.py's DRAM-side roofline figure (roofline.frac_dram) is measured this way.
 * Same game trajectories as sgx_step_n (tests/test_gpu_parity.py).  No reference counterpart beyond the loop of
 * examples/basic_game_loop.py:34-63. */
int sgx_step_ring(sgx_env *h, const sgx_step_io *ios, int32_t n_sets, int32_t first_set, int32_t n_steps, void *stream);

/* sgx_step_n into a TRAJECTORY buffer: step t of the call (t = 0 .. n_steps-1) writes its outputs into slot (first_slot + t) % n_slots of
 * tensors that carry a leading slot axis -- obs float32 [n_slots][slot_envs][R][C][67], mask uint8 [n_slots][slot_envs][R][C][K], ... --
 * named by the pointers of slot 0 (`io`) and ONE stride, `slot_envs` (>= N; = N for dense [T][N]... tensors).  This is the batched
 * counterpart of what the reference's caller gets: a FRESH observation / mask array from every env.step() (impl:905, maenv:447-497), so a
 * learner that keeps T steps keeps T arrays.  Unlike sgx_step_ring the number of slots is not limited (n_slots = n_steps = 64 ... 1024 is the
 * intended use), and with results_per_slot != 0 the per-step results are kept as well: reward float32 [n_slots][slot_envs][2], done /
 * invalid_action / ending_invalid uint8 [n_slots][slot_envs], player int8 [n_slots][slot_envs] (0: they are overwritten in place like
 * sgx_step_n's).  actions_log_dev (nullable) int32 [n_slots][slot_envs] receives the action every env DREW in the step -- the action the
 * next step plays, i.e. the action chosen from the observation / mask of the same slot: (obs_t, mask_t, action_t) line up, and
 * reward / done of slot t + 1 are what that action earned.  final_obs_dev / final_fobs_dev have no slot axis (they are written on
 * terminal steps only).  io->actions_dev == io->next_actions_dev (the chain of drawn actions, int32 [N], no slot axis); tensors that are
 * NULL in `io` are skipped.  Where the call is eligible for the multi-step kernels (sgx_set_multi_step) all steps run in ONE launch
 * (launches of at most 256 steps); everything else takes one launch per step with the same results (tests/test_gpu_trajectory.py compares
 * every slot with the oracle stepped alongside).  Compact outputs: the slot strides are those of the compact tensors
 * (uint8 [n_slots][slot_envs][sgx_compact_obs_stride], uint32 [n_slots][slot_envs][sgx_compact_mask_words]). */
typedef struct sgx_traj_io {
    sgx_step_io io;               /* the tensors of slot 0 */
    int32_t n_slots;              /* >= 1 */
    int32_t results_per_slot;     /* 0: reward / done / player / invalid_action / ending_invalid in place; != 0: [n_slots][slot_envs]... */
    int64_t slot_envs;            /* envs per slot of every tensor that has a slot axis, >= N */
    int32_t *actions_log_dev;     /* [n_slots][slot_envs] out (nullable): the action drawn in each step */
} sgx_traj_io;
int sgx_step_traj(sgx_env *h, const sgx_traj_io *t, int32_t first_slot, int32_t n_steps, void *stream);

/* sgx_step_n with the batch split into `chains` (1..SGX_MAX_CHAINS) contiguous ranges of games, each range playing its n_steps on a
 * stream of its own: games never interact, so the ranges' launches may overlap, and the ramp-up / drain of one range's step is filled
 * by the other's (a launch that lasts tens of microseconds spends a third of its time with the chip half empty).  The caller's
 * stream waits for all chains; results are identical to sgx_step_n.  Measured with chains = 2 on 65,536 games: Micro 41.3 -> 37.2 us per
 * step of all games, 5x5 107.6 -> 96.0 us, 8x8 198 -> 183 us, Barrage 322 -> 304 us (docs/DESIGN_rounds_1-3.md).  chains = 0 lets the
 * library choose by the rule measured on the current kernels (2 for boards of up to 36 cells and for boards whose cell count is no
 * multiple of 4, else 1: 8x8 and 10x10 launches already stream at the memory rate and lose 2-5 % to a second chain) -- after trying
 * the multi-step launch of sgx_set_multi_step, which is faster than any number of chains wherever the call is eligible.  No reference
 * counterpart. */
#define SGX_MAX_CHAINS 4
int sgx_rollout(sgx_env *h, const sgx_step_io *io, int32_t n_steps, int32_t chains, void *stream);

/* sample_random_valid_action (maenv:830-834) for a batch of masks laid out as mask_dev of sgx_step_io:
 * picks the k-th set byte, k drawn with the same counter RNG as next_actions_dev (identical results). */
int sgx_sample_valid(sgx_env *h, const uint8_t *mask_dev, int32_t *actions_dev, void *stream);

/* nnet_choose_action_example (examples/basic_game_loop.py:6-31 with softmax of examples/util.py:4-47) for a batch, on the device: the
 * caller's policy writes logits float32 [N][R*C*K] in the shape of the valid-actions mask; invalid actions get probability 0, the rest
 * softmax((logits - max) / temperature), and ONE action per game is drawn from it -- one wave per game, logits and mask read once.
 * mask_dev: the mask the step kernel wrote, uint8 [N][R*C*K], or with flags = SGX_STEP_COMPACT_MASK the bit mask uint32
 * [N][sgx_compact_mask_words] of a compact step.  temperature: a divisor, > 0; 0 = argmax (ties drawn uniformly).
 * The draw is keyed like next_actions_dev -- counter RNG on (seed, global env id, game number, turn) -- and sampling is fixed point:
 * weight of a valid action = floor(exp2((logit - max) * log2(e) / temperature + 23)), i.e. 2^23 for the maximum, exact integer sums,
 * inverse CDF in ascending action order.  A result depends on nothing but (logits, mask, seed, game, turn), and with equal logits it IS
 * sgx_sample_valid's action.  The truncation means an action whose probability relative to the most likely one is below 2^-23
 * (~1.2e-7) has weight 0 and is never drawn.  NaN logits count as -inf.  actions_dev[i] = -1 where NO action can be drawn: the mask
 * is empty, or every valid action's logit is -inf / NaN -- the caller must not feed that -1 to sgx_step (it is an invalid action); a
 * terminal env's mask holds the no-op only, which is drawn like any other action.
 * No policy network lives in this library: the logits are the caller's. */
int sgx_choose_actions(sgx_env *h, const float *logits_dev, const void *mask_dev, float temperature, int32_t flags, int32_t *actions_dev, void *stream);

/* INTERNAL_STATE observation component / reset(initial_state_override=...) (maenv:494-495, 551-553):
 * convert between the library's packed int8 state and the reference's int64 [N,34,R,C] layout
 * (absolute coordinates).  player_dev int8 [N] = current mover (nullable on export; NULL on import = +1). */
int sgx_export_state(sgx_env *h, int64_t *state_dev, int8_t *player_dev, void *stream);
int sgx_import_state(sgx_env *h, const int64_t *state_dev, const int8_t *player_dev, void *stream);
/* The same import with a report: the reference's pure functions accept ANY int64 [34,R,C] (impl:399-517, 894-1045), the packed
 * record only what play can produce.  sanitised_dev uint8 [N] (nullable) is set to 1 for every state the import had to alter:
 * a value outside its layer's range (-> 0), more than two non-zero recent-move cells of one player (the rest dropped), more
 * captured pieces than 2 x pieces per side (the surplus dropped), an obstacle layer that differs from the variant's (the
 * variant's is used), a player that is not +1 / -1; 0 otherwise -- results for flagged states may differ from the reference's. */
int sgx_import_state_checked(sgx_env *h, const int64_t *state_dev, const int8_t *player_dev, uint8_t *sanitised_dev, void *stream);

/* The functional operator API on caller-provided int64 states in one call: sgx_import_state_checked -> sgx_step -> sgx_export_state
 * (state_out_dev NULL: no export -- is_move_valid_*, masks and observations of the given states), i.e. get_next_state (penv:148-155)
 * for a batch.  The batch is split into `chains` (1..SGX_MAX_CHAINS) ranges of states on streams of their own, so that one range's
 * 27 KB-per-state reads overlap another's writes; the caller's stream waits for all of them.  io as in sgx_step with the SGX_STEP_*
 * flags of the functional API; no auto_reset, no next_actions_dev; io->actions_dev NULL = sgx_observe of the given states (their
 * movers' masks / observations, nothing is played).  The handle's own states are overwritten.  On boards of more than 32 cells with
 * the 67-channel observation kind the three steps are ONE launch (a 128-thread block per state, the packed record never leaves
 * LDS): 65,536 Barrage states 745 -> ~640 us; `chains` only matters on the other paths.
 * NO ALIASING while the general-state pass is on (the default, see sgx_set_general_states; boards of up to 256 cells): that pass reads
 * state_in_dev / player_in_dev again after the outputs have been written, so state_out_dev must not overlap state_in_dev and
 * player_out_dev must not overlap player_in_dev -- SGX_EINVAL otherwise.  With the pass off, stepping a batch in place is fine (every
 * state is read completely before its successor is written): state_out_dev == state_in_dev, player_out_dev == player_in_dev.  Any OTHER
 * overlap (outputs shifted against the inputs by some states) is SGX_EINVAL in either mode: one workgroup would write what another has
 * yet to read. */
int sgx_step_states(sgx_env *h, const int64_t *state_in_dev, const int8_t *player_in_dev, uint8_t *sanitised_dev,
                    const sgx_step_io *io, int64_t *state_out_dev, int8_t *player_out_dev, int32_t chains, void *stream);

/* General states in sgx_step_states.  The reference's pure functions accept ANY int64 [34,R,C] (penv:74-155); the packed record carries what
 * play can produce.  On boards of up to 256 cells sgx_step_states runs a second pass over the states its import had to alter (behind the
 * one-launch path above, or behind the three launches of the other paths: boards of up to 32 cells, the 79-channel and 'original'
 * observation kinds): they are redone from the caller's int64 input on a general-state variant of the kernels -- dense recent-move
 * layers, a capture event for every (layer, cell) pair, counts up to 32,768, captured-count channels beyond the 16-entry table
 * normalised by the reference's own float32 arithmetic (maenv:506-508) -- so that get_next_state, is_move_valid_*, the masks and every
 * observation kind of such states equal the reference's (not covered: boards of more than 256 cells; state-coordinate masks requested
 * together with a 79-channel or 'original' observation); sanitised_dev then reports only what still had to be altered
 * (values outside their layer's range, an obstacle layer that differs from the variant's, a player that is not +1 / -1).  mode 1 (default):
 * on; 0: off (flagged states keep the first pass' sanitised results).  SGX_GENERAL_STATES=0|1 sets the default of handles created
 * afterwards.  Costs one launch of early-exit blocks (~2 % of a get_next_state call) when no state is flagged. */
int sgx_set_general_states(sgx_env *h, int32_t mode);

/* Search callers (MCTS on get_next_state, penv:148-155) keep their nodes in the packed records instead of paying the 27 KB
 * int64 import / export per state: handles of the same variant on the same device act as node pools.
 * sgx_copy_envs: records src[src_index[i]] -> dst[dst_index[i]] for i < n (an index array may be NULL = identity).
 * sgx_expand: one env.step() per env i of `dst`, reading the game from record src_index[i] of `src` (i when NULL) and writing
 * the successor to record i of `dst`; where the action is invalid (invalid_action[i] = 1) record i becomes a copy of the
 * parent.  `io` as in sgx_step (flags SGX_STEP_ACTIONS_1D / _POSITIONS / _ALLOW_OSCILLATION / _RAW_OBS / _MASK_*; no auto_reset,
 * no fully-observable / original-channel outputs); src == dst with a NULL index is sgx_step.  Inside ONE handle an indexed
 * copy / expansion would race (a wave reads a record another wave of the same launch rewrites): sgx_expand with src == dst and
 * a non-NULL index, and sgx_copy_envs with src == dst and any index, return SGX_EINVAL -- use a second handle as the target.
 * sgx_copy_envs: n in [0, 2^31), else SGX_EINVAL before any launch (with two index arrays no handle's size bounds it).
 * No reference counterpart beyond get_next_state itself. */
int sgx_copy_envs(sgx_env *dst, const int32_t *dst_index_dev, sgx_env *src, const int32_t *src_index_dev, int64_t n, void *stream);
int sgx_expand(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_step_io *io, void *stream);

/* Determinization for imperfect-information search (determinized MCTS, ISMCTS, PIMC rollouts): every slot i of `dst` becomes record
 * src_index[i] of `src` (i when NULL) with the HIDDEN pieces of the observer's opponent dealt again, so that a search expanding from it does
 * not see the true types.  observer: 0 = each record's mover, +1 / -1 = that player for every record.  Hidden cells are the opponent's
 * pieces whose public board says 13 (unknown); their types are permuted uniformly over all assignments that keep the flag and the bombs on
 * never-moved cells.  Nothing else of the record changes: public boards, never-moved bitmaps, scalars, recent moves, capture events and
 * the observer's own pieces are copied bit for bit, so the observer's partial observation and valid-move mask are what they were.  The
 * shuffle is keyed by (dst's seed, dst's env_id_offset + i, draw) on an RNG stream of its own: the same call gives the same worlds, another
 * `draw` gives independent ones, and no draw of a rollout moves.  hidden_dev: int32 [dst's N] (NULL = not wanted) = number of hidden cells that
 * were shuffled; -1 marks a record with a flag or a bomb on a moved hidden cell, which play cannot produce: it is copied unchanged.
 * A sampled world agrees with everything the record tracks (what the reference's state tracks), NOT with the full move history: a piece that
 * has acted in ways only some types can may still be dealt another type (sgx_determinize_weighted takes such knowledge as weights).  src == dst with a NULL index works in place; with an index it
 * would race and is SGX_EINVAL, like an observer outside {-1, 0, 1}, a handle of another variant or a misaligned pointer (4 bytes).
 * No reference counterpart. */
int sgx_determinize(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, int32_t observer, uint64_t draw, int32_t *hidden_dev, void *stream);

/* Determinization from a belief: sgx_determinize with caller-given weights of (opponent type, cell) in the place of the uniform deal -- a
 * network or a prior over setups (stratego_env_amd/beliefs.py; carried along the moves of each game by the labels of a tracked replay,
 * sgx_set_replay_origins, and beliefs.follow) says where the opponent's pieces are likely to stand, and the worlds are drawn accordingly, in the same single launch, pool to pool, with the same key and the same guarantees.
 * THE RULE (tests/determinize_weighted_rule.py restates it in numpy, bit for bit).  For slot i of dst:
 *   s = src_index[i] (i when the index is NULL), g = dst's env_id_offset + i.
 *   opp, H, A, B are exactly those of sgx_determinize: opp = the observer's opponent, H = opp's cells whose public layer says 13, A = the
 *   cells of H that never moved, B = the rest; c_t = the number of pieces of true type t on H.
 *   A flag or a bomb on a cell of B: the record is copied unchanged, hidden = -1, off_belief = 0.
 *   Tb = belief_dev + s * belief_stride (in uint16 elements; belief_stride == 0: one table for all records).  A table is uint16
 *   [2][12][cells]: [opp's player index: 0 = player +1, 1 = player -1, as the record's layers are][t - 1 for t = 1..12][ABSOLUTE cell].
 *   w(t, c) = min(Tb[(opp * 12 + t - 1) * cells + c], SGX_BELIEF_WEIGHT_MAX = 4095).  The clamp is part of the rule: the table is device
 *   memory, which the host cannot range-check.
 *   The types are dealt in the order 11 (flag), 12 (bomb), 10, 9, ..., 1; type t has c_t instances, one after the other; a counter
 *   j = 0, 1, ... runs over all instances of the deal.  The order is a function of the public multiset of hidden types alone, never of
 *   where the pieces truly stand.  free = H.  For the instance of type t with counter j:
 *     the candidates c_0 < ... < c_{m-1} are the cells of free that lie in A when t is 11 or 12, else all cells of free, ascending;
 *     W = the sum of the w(t, c_k) (32-bit: 1,024 cells x 4,095);
 *     r = rng(dst's seed, g, draw, STREAM_DETERMINIZE_WEIGHTED = 7, j) with the library's counter RNG;
 *     W > 0:  x = rng_below(r, W); the cell is the first c_k whose inclusive prefix sum w(t, c_0) + ... + w(t, c_k) exceeds x -- the
 *             sampler of sgx_playout_weighted;
 *     W == 0: k = rng_below(r, m), the cell is c_k, and off_belief counts one more;
 *     pieces[opp][cell] = t, and the cell leaves free.
 *   m >= 1 at every draw: the immovable types come first and go to A only, |I| <= |A| in a record that is not refused, and afterwards as many
 *   cells are free as instances remain -- dealing by type instance cannot dead-end, whatever the weights.
 *   hidden = |H|; off_belief = the number of instances that landed on a cell whose weight for their type is 0 (a caller may discard such
 *   worlds: the belief called them impossible).
 * Consequences (all tested): only bytes of pieces[opp] change, so the observer's observation, valid-move mask and information-set key
 * (sgx_state_keys) are what they were; the multiset of hidden types is kept and flags and bombs stay on never-moved cells; a cell of weight
 * 0 is never taken while a candidate of positive weight exists; a table whose entries are all the same constant c >= 1 samples UNIFORMLY
 * over the worlds -- the distribution of sgx_determinize, though not its worlds: the algorithm and the RNG stream are others; a table
 * that is one-hot on the truth returns the source record bit for bit with off_belief = 0.  The weights steer a sequential deal: they are
 * NOT the marginals of the result (a cell that an earlier type took is gone for the later ones).
 * STREAM_DETERMINIZE_WEIGHTED is a stream of its own: no existing draw moves.  belief_dev is DEVICE memory, only read.  hidden_dev,
 * off_belief_dev: int32 [dst's N], each nullable.  src == dst with a NULL index works in place (a record is read whole before it is
 * written).  SGX_EINVAL, before anything is launched, under this function's name: everything sgx_determinize refuses (handles of other
 * variants or devices, a NULL index with src smaller than dst, the in-place call with an index, an observer outside {-1, 0, 1});
 * belief_dev == NULL; belief_stride negative, odd, or positive and below 2 * 12 * cells; src_index_dev, belief_dev, hidden_dev or
 * off_belief_dev not 4-byte aligned.  An addition within v15: no existing struct or signature changed, SGX_ABI_VERSION stays.
 * No reference counterpart. */
#define SGX_BELIEF_WEIGHT_MAX 4095
int sgx_determinize_weighted(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, int32_t observer,
                             const uint16_t *belief_dev, int64_t belief_stride, uint64_t draw,
                             int32_t *hidden_dev, int32_t *off_belief_dev, void *stream);

/* Playouts: every slot of `dst` plays a position of `src` to the end of its game with uniformly random valid moves, in ONE launch, and
 * reports who won -- what a determinized-MCTS / ISMCTS / PIMC caller does with a sampled world (sgx_determinize) or an expanded node
 * (sgx_expand).  N = dst's number of envs.  THE RULE (tests/playout_rule.py restates it on the CPU oracle, bit for bit):
 *   For slot i of dst: g = dst's env_id_offset + i, pos = record src_index[i] of src (i when the index is NULL).
 *   limit = max(pos.max_turns - pos.turn, 0) + 1, cut to max_steps when max_steps > 0.  (Every applied move advances the turn counter and
 *   the max-turn ending fires at turn >= max_turns, so no game outlasts the bound: the bound ends the device loop, the game state alone never does.)
 *   While pos is not over and fewer than `limit` moves have been played: m = the valid-action mask of pos's mover in the mover's perspective
 *   (what sgx_step writes to mask_dev), n = its number of set entries; the move is the k-th set entry in ascending flat order,
 *   k = rng_below(rng(dst's seed, g, draw, STREAM_PLAYOUT = 6, turn), max(n, 1)) with the library's counter RNG, turn = pos's turn counter (sgx_get_env_info) -- the
 *   action of sgx_sample_valid with another RNG word; the move is applied exactly as sgx_step applies it.
 *   STREAM_PLAYOUT is a stream of its own, so no draw of a rollout, a setup, a pool or a determinization moves; `draw` stands where the
 *   rollouts' key has the game number, as in sgx_determinize: the same call gives the same games, another draw independent ones.
 *   Afterwards dst[i] is the final position, whole (a copy of the root where nothing was played); reward / done / ending_invalid / player are
 *   what a step of sgx_step on that final position reports -- a finished game reports its result on every step: +-1 for a win, the
 *   reference's tie value, and 0, 0 for a max-turn ending and for a playout that was cut off (done = 0); length = the moves played.
 * There is no auto-reset, and nothing of src changes unless src == dst.  src == dst with a NULL index works in place (a game's record is
 * read whole before it is written); with an index it would race like sgx_expand and is SGX_EINVAL.  Also SGX_EINVAL, before anything is
 * launched: handles of different variants or devices, a NULL index with src smaller than dst, max_steps < 0, flags != 0, a misaligned
 * pointer (reward_dev, length_dev, src_index_dev 4 bytes; the byte tensors any address), a dst with a start pool set.
 * Sets dst's sgx_last_launch_kind to SGX_LAUNCH_PLAYOUT.  Added without a change to an existing struct or signature: SGX_ABI_VERSION stays.
 * Reference counterpart: none -- the loop of examples/basic_game_loop.py:34-63 run to dones['__all__'], as a function of a state. */
typedef struct sgx_playout_io {
    float   *reward_dev;          /* [N,2] out (nullable): rewards[+1], rewards[-1] of the FINAL position */
    uint8_t *done_dev;            /* [N]   out (nullable): 1 = the playout reached the end of its game, 0 = cut off by max_steps */
    uint8_t *ending_invalid_dev;  /* [N]   out (nullable): the max-turn tie (maenv:777-782) */
    int8_t  *player_dev;          /* [N]   out (nullable): the mover at the final position */
    int32_t *length_dev;          /* [N]   out (nullable): moves played, 0 for a root that was already over */
    int32_t  max_steps;           /* 0 = to the end of the game; > 0 = at most this many moves; < 0 = SGX_EINVAL */
    int32_t  flags;               /* 0 (anything else SGX_EINVAL) */
} sgx_playout_io;                 /* 5 pointers + 2 int32 = 48 bytes */
int sgx_playout(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_playout_io *io, uint64_t draw, void *stream);

/* Weighted playouts: sgx_playout with a policy.  Move a is drawn with probability proportional to a caller-given weight of (direction,
 * moving piece, what stands on the target cell) -- attack what you beat, do not attack what beats you, walk forward -- in the same single
 * launch, with the same key, pool to pool.  THE RULE (tests/weighted_playout_rule.py restates it on the CPU oracle, bit for bit):
 *   weights: uint16 [4][13][14], every entry in [0, SGX_PLAYOUT_WEIGHT_MAX = 4095], read as weights[dir][t][d].
 *   For a position that is not over, with mover p: a_0 < ... < a_{n-1} are the set entries of the mover's perspective mask in ascending
 *   flat order (a = pcell * K + ch): exactly the moves sgx_playout ranks.  For each move:
 *     dir = which of the four channel blocks the move's ch lies in, in the order of the mask's channels: perspective +r ([0, R-1)), -r
 *           ([R-1, 2(R-1))), +c ([2(R-1), 2(R-1) + C-1)), -c (the C-1 after that).  Player +1 sets up on rows 0 .. usable_rows-1 and player
 *           -1 on the opposite rows, and a mover's perspective is the board turned so that its own rows are the low ones: dir 0 is FORWARD,
 *           towards the opponent's setup rows, for either player; 1 is backward, 2 and 3 sideways.
 *     t   = the mover's true piece type on the start cell (1..10).
 *     d   = what stands on the destination.  By default (the public view) the value of the OPPONENT'S PUBLIC LAYER there: 0 = empty,
 *           1..12 = a revealed type, 13 = a piece the mover has not identified -- what the mover's partial observation shows.  With
 *           SGX_PLAYOUT_SEE_ALL the opponent's TRUE type there (0..12): the usual choice inside a determinized world.
 *     w_i = weights[dir][t][d];  W = the sum of the w_i (32-bit: on any board of at most 1,024 cells 4095 x the most valid moves stays
 *           below 2^32).
 *   r = rng(dst's seed, env_id_offset + i, draw, STREAM_PLAYOUT = 6, the position's turn): the SAME draw sgx_playout takes.
 *     n == 0: the no-op, as in sgx_playout.
 *     W > 0:  x = rng_below(r, W); the move is the first a_i whose inclusive prefix sum w_0 + ... + w_i exceeds x.
 *     W == 0: k = rng_below(r, n), the k-th valid move, exactly as sgx_playout.
 *   Everything else is sgx_playout's: the move bound, max_steps, the results, length, the final record, src only read, the in-place call
 *   without an index.
 * Two consequences (both tested): a table whose entries are all the same constant c >= 1 plays, bit for bit, the games sgx_playout plays
 * (floor(floor(h c n / 2^32) / c) = floor(h n / 2^32)); a move of weight 0 is never drawn while another valid move has a weight > 0.
 * io is sgx_playout_io as it is, io->flags must still be 0.  `weights` is HOST memory (its name carries no _dev and the alignment contract
 * has nothing to add): it is read before the call returns -- the table travels in the launch's own arguments -- so the caller may change
 * or free it at once, and two calls on one stream with different tables each play with their own.
 * SGX_EINVAL, before anything is launched: weights == NULL; an entry above 4095 (the message names the first offender's indices); unknown
 * policy_flags bits; and everything sgx_playout refuses, under this function's name.  Sets dst's sgx_last_launch_kind to
 * SGX_LAUNCH_PLAYOUT_WEIGHTED.  An addition within v15: no existing struct or signature changed, SGX_ABI_VERSION stays.
 * Reference counterpart: none as a playout; the table is what get_heuristic_rewards_from_move(state, player, action,
 * reward_matrix[moved type, target type]) (impl:852-891) looks up, with a direction added
 * (stratego_env_amd/playout_policies.py: from_reward_matrix, capture_biased). */
#define SGX_PLAYOUT_SEE_ALL 1          /* policy_flags: d is the opponent's true type on the target cell, not what the mover has seen of it */
#define SGX_PLAYOUT_WEIGHT_MAX 4095
int sgx_playout_weighted(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_playout_io *io,
                         const uint16_t *weights /* HOST memory, [4][13][14] */, int32_t policy_flags, uint64_t draw, void *stream);

/* Play against a built-in opponent: the agent's move and the reply of a table bot -- the policy of sgx_playout_weighted playing one side of
 * a LIVE game -- in ONE launch that writes no observation: an agent decision against a fixed opponent costs one sgx_observe, not the two
 * full steps of a host loop that merges two action sources.  N = dst's number of envs.  THE RULE (tests/step_vs_rule.py restates it on
 * the CPU oracle, bit for bit):
 *   For slot i of dst: pos = record src_index[i] of src (i when the index is NULL), side = the agent's side (agent_dev[i] < 0: -1, else
 *   +1; `agent` when agent_dev is NULL), g = dst's env_id_offset + i.
 *   1. invalid = moved = 0, reply = -1.
 *   2. If pos is not over, its mover is `side` and actions_dev is given: actions_dev[i] is applied to pos exactly as sgx_step applies an
 *      action -- the same decode (flat spatial index in the mover's perspective), the same validity checks (an out-of-range value, a move
 *      the rules refuse, the no-op of a mover that has a move), the same endings; no auto-reset.  Refused: invalid = 1, pos stays what
 *      it was, go to 4.  Applied: moved |= SGX_VS_MOVED_AGENT.  (Where the mover is not `side` the entry is not read as a move.)
 *   3. If pos is not over and its mover is not `side`, the bot moves once: the valid moves a_0 < ... < a_{n-1}, dir, t, d, w_i and W are
 *      those of sgx_playout_weighted's rule, taken for the bot as the mover, in the public view -- the bot does not cheat -- or with
 *      SGX_VS_SEE_ALL the true one; r = rng(dst's seed, g, draw, STREAM_REPLY = 8, pos's turn counter).  n == 0: the no-op.  W > 0:
 *      x = rng_below(r, W), the first a_i whose inclusive prefix sum exceeds x.  W == 0: the rng_below(r, n)-th valid move.  The move is
 *      applied as a step applies it; reply = that action, moved |= SGX_VS_MOVED_BOT.  Players alternate, so there is never a second bot
 *      move: the rule has no loop.
 *   4. dst[i] = pos, whole.  reward / done / ending_invalid / player are what a step on that position reports, as sgx_playout words it: a
 *      finished position reports its result on every call.
 * Consequences (all tested): after the call every slot that is not over and not `invalid` has `side` to move; a slot that was over is
 * copied, whatever its action; actions_dev == NULL is "the bot opens where it is its turn", every other slot a copy; a table whose
 * entries are all the same constant c >= 1 draws uniformly over the bot's valid moves; a move of weight 0 is never drawn while another
 * valid move has a weight > 0.
 * STREAM_REPLY is a stream of its own: no existing draw moves.  `draw` stands where the rollouts' key has the game number: a caller that
 * steps a live env passes another draw with every call (the same call gives the same replies).  src == dst with a NULL index works in
 * place -- the live-env call (a game's record is read whole before it is written); with an index it would race and is SGX_EINVAL.  Also
 * SGX_EINVAL, before anything is launched, under this function's name: everything sgx_playout_weighted refuses (weights == NULL, an entry
 * above 4095, NULL handles or io, handles of different variants or devices, a NULL index with src smaller than dst, a misaligned
 * src_index_dev or reward_dev) EXCEPT a start pool on dst; `agent` outside {+1, -1} with agent_dev == NULL; unknown flags bits;
 * actions_dev or reply_action_dev not 4-byte aligned.  A dst with a start pool set IS accepted (a curriculum env is the main customer):
 * the call never restarts a game and writes no start index; restarts are the caller's sgx_reset.  Leaf values set on dst are not used:
 * this is live stepping, like sgx_step.  Asynchronous on `stream`; `weights` is HOST memory, read before the call returns, so two calls
 * on one stream with different tables each play with their own.  Sets dst's sgx_last_launch_kind to SGX_LAUNCH_STEP_VS.  An addition
 * within v15: no existing struct or signature changed, SGX_ABI_VERSION stays.
 * Reference counterpart: the vs_bot branch of StrategoMultiAgentEnv (maenv:573-619), whose opponent is an external bot behind a socket. */
#define SGX_VS_SEE_ALL 1           /* flags: the bot looks at the agent's TRUE types (as SGX_PLAYOUT_SEE_ALL); default: the public view */
#define SGX_VS_MOVED_AGENT 1       /* bits of moved_dev */
#define SGX_VS_MOVED_BOT   2
typedef struct sgx_vs_io {
    const int32_t *actions_dev;    /* [N] nullable: the agent's action, flat spatial index in the mover's perspective, as sgx_step takes it */
    const int8_t  *agent_dev;      /* [N] nullable: the agent's side per slot, < 0 = player -1, else +1; NULL = `agent` for every slot */
    float   *reward_dev;           /* [N,2] out, nullable: rewards[+1], rewards[-1] of the FINAL position, as sgx_playout reports them */
    uint8_t *done_dev, *ending_invalid_dev;   /* [N] out, nullable */
    int8_t  *player_dev;           /* [N] out, nullable: the mover at the final position */
    uint8_t *invalid_action_dev;   /* [N] out, nullable: 1 = the agent's action was refused as sgx_step refuses it; position unchanged, the bot did not move */
    uint8_t *moved_dev;            /* [N] out, nullable: SGX_VS_MOVED_* */
    int32_t *reply_action_dev;     /* [N] out, nullable: the bot's move, flat spatial index in the BOT's perspective (what sgx_replay takes); -1 = none */
    int32_t  agent;                /* +1 / -1, read when agent_dev is NULL */
    int32_t  flags;                /* SGX_VS_SEE_ALL */
} sgx_vs_io;                       /* 9 pointers + 2 int32 = 80 bytes */
int sgx_step_vs(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_vs_io *io,
                const uint16_t *weights /* HOST memory, [4][13][14], entries <= SGX_PLAYOUT_WEIGHT_MAX */, uint64_t draw, void *stream);

/* Replay: every slot of `dst` becomes a position of `src` advanced by a GIVEN list of actions, all entries in ONE launch -- what a learner
 * that kept start records and the action log of sgx_step_traj does to get back to (game, t), what a search does to re-derive a node from
 * its root and the path to it, and how a recorded game is played.  N = dst's number of envs.  THE RULE (tests/replay_rule.py restates it on
 * the CPU oracle, bit for bit):
 *   For slot i of dst: pos = record src_index[i] of src (i when the index is NULL); len = lengths_dev[i] clamped to [0, max_len] (max_len
 *   when lengths_dev is NULL); entry t of the list is actions_dev[i * game_stride + t * step_stride]; c = m = 0.  Then, repeatedly:
 *     1. c == len: stop = 0, end (the list is exhausted).
 *     2. pos is over: stop = 1, end.  Entries after the end of the game are not read.
 *     3. entry c is applied to pos exactly as sgx_step applies an action: the same decode (flat spatial index in the mover's perspective;
 *        with SGX_REPLAY_ACTIONS_1D an absolute 1-D index as sgx_expand takes it), the same validity checks -- an out-of-range value
 *        (np.unravel_index raises) and a no-op while the mover has a move are invalid --, the same endings, and no auto-reset.
 *     4. valid: m++, c++.
 *     5. invalid with SGX_REPLAY_SKIP_INVALID: c++, pos unchanged.
 *     6. invalid without it: stop = 2, end; c is not advanced, so entry c is the offending one.
 *   A count (len <= max_len) bounds the loop; the game state alone never does.
 *   Afterwards dst[i] is pos, whole (a copy of the root where nothing was applied); reward / done / ending_invalid / player are what a step
 *   of sgx_step on that final position reports, as sgx_playout reports them (0, 0 and done = 0 for a game that is not over);
 *   applied = m, consumed = c.
 * There is no random draw anywhere: the result is a function of (record, list, flags), dst's seed does not enter.  There is no auto-reset,
 * and nothing of src changes unless src == dst.  src == dst with a NULL index works in place (a game's record is read whole before it is
 * written); with an index it would race like sgx_expand and is SGX_EINVAL.  Also SGX_EINVAL, before anything is launched: handles of
 * different variants or devices, a NULL index with src smaller than dst, max_len < 0, unknown flag bits, a negative stride, actions_dev
 * NULL with max_len > 0, (N - 1) * game_stride + (max_len - 1) * step_stride >= actions_elems, a misaligned pointer (actions_dev,
 * lengths_dev, applied_dev, consumed_dev, reward_dev, src_index_dev 4 bytes; the byte tensors any address), a dst with a start pool set.
 * max_len == 0 is legal: a copy, with the roots' own results reported.
 * Strides are in elements and may be anything >= 0: (L, 1) is a dense game-major [N][L] tensor, (1, slot_envs) the [T][N] action log of
 * sgx_step_traj (actions_log_dev) as it is; a game's lanes fetch a chunk of consecutive entries per load, so step_stride == 1 reads whole
 * lines and any other stride one entry per line.
 * Sets dst's sgx_last_launch_kind to SGX_LAUNCH_REPLAY.  Added without a change to an existing struct or signature: SGX_ABI_VERSION stays.
 * Reference counterpart: none -- env.step() in a loop over a recorded list (examples/basic_game_loop.py:34-63), as a function of a state. */
#define SGX_REPLAY_SKIP_INVALID      1   /* an invalid action is passed over (position unchanged) and the replay goes on */
#define SGX_REPLAY_ACTIONS_1D        2   /* entries are absolute 1-D indices (as sgx_expand's SGX_STEP_ACTIONS_1D); default: flat spatial, mover's perspective (as sgx_step) */
#define SGX_REPLAY_ALLOW_OSCILLATION 4   /* as SGX_STEP_ALLOW_OSCILLATION */
typedef struct sgx_replay_io {
    const int32_t *actions_dev;   /* entry t of slot i: actions_dev[i*game_stride + t*step_stride] */
    const int32_t *lengths_dev;   /* [N] nullable (= max_len for all); clamped to [0, max_len] */
    int32_t *applied_dev;         /* [N] out, nullable: moves applied */
    int32_t *consumed_dev;        /* [N] out, nullable: entries gone past (applied or skipped) */
    uint8_t *stop_dev;            /* [N] out, nullable: 0 list exhausted, 1 game over, 2 invalid action */
    float   *reward_dev;          /* [N,2] out, nullable: rewards[+1], rewards[-1] of the FINAL position */
    uint8_t *done_dev, *ending_invalid_dev;   /* [N] out, nullable */
    int8_t  *player_dev;          /* [N] out, nullable: the mover at the final position */
    int64_t game_stride, step_stride;         /* in elements, >= 0: (L,1) dense game-major, (1,slot_envs) the trajectory's [T][N] log */
    int64_t actions_elems;        /* int32 elements addressable from actions_dev: the host checks the last index against it */
    int32_t max_len, flags;
} sgx_replay_io;                  /* 9 pointers + 3 int64 + 2 int32 = 104 bytes */
int sgx_replay(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_replay_io *io, void *stream);

/* Piece origins: a replay that also says, for every piece on the board at its end, WHICH piece it is -- by default the cell it stood on at
 * the replay's root.  The record cannot say that (it carries types, what the opponent has seen, and which cells never moved, not identity),
 * and a setup prior is a statement about setup cells: with the origins of a replay from the setup, "what stands on cell c now" becomes "what
 * was deployed on cell origin[c]" (stratego_env_amd.beliefs.follow), which is what sgx_determinize_weighted's per-record tables want.
 * A SETTING OF THE dst HANDLE, like sgx_set_start_index_out: while origin_out_dev is set, every sgx_replay whose dst is h also tracks the
 * labels, on the call's stream like the rest of its work, and sets dst's sgx_last_launch_kind to SGX_LAUNCH_REPLAY_TRACKED.  The setter
 * stores the two caller-owned device pointers, launches nothing and waits for nothing; the caller keeps the tensors alive while the setting
 * holds.  Every byte sgx_replay writes without the setting -- the records and the seven result tensors, with or without leaf values on dst --
 * it writes the same with it; without the setting nothing changes anywhere.
 *   origin_out_dev  int16 [dst N][2][cells]       written whole for every slot
 *   origin_in_dev   int16 [src envs][2][cells]    nullable; read at record s = src_index[i] (i without an index), as belief_dev is addressed
 *   Player index 0 is player +1 and 1 is player -1, as the state's layers; cells are absolute, cell = r * C + c.
 * THE RULE is defined on the reference states the replay passes through, not on the record (tests/origins_rule.py restates it in numpy on
 * the CPU oracle).  own(q) = state layer q (true pieces).
 *   Start: Lab[q][c] = (origin_in[s][q][c] if origin_in_dev is given, else c) where own(q)(root)[c] != 0, and -1 everywhere else.  A given
 *   label is an opaque int16 carried verbatim (origins are the default, any piece id works); what origin_in holds on empty cells is ignored.
 *   Every applied entry (step 4 of the replay's rule) taking pos to pos', mover index q, opponent q':
 *     a = the one cell with own(q)(pos)[a] != 0 and own(q)(pos')[a] == 0;
 *     Lab'[q] = Lab[q], except Lab'[q][a] = -1, and, if some cell b has own(q)(pos)[b] == 0 and own(q)(pos')[b] != 0 (the mover stands there
 *     after a move to an empty cell or a won attack), Lab'[q][b] = Lab[q][a];
 *     Lab'[q'][c] = Lab[q'][c] where own(q')(pos')[c] != 0, else -1.
 *   So a lost or drawn attack drops the mover's label, a won or drawn attack the defender's; a flag capture is a won attack.  (A valid no-op
 *   entry -- the mover has no move -- moves no piece: no cell a, nothing changes.)  Entries passed over (SGX_REPLAY_SKIP_INVALID) or refused
 *   change nothing.
 *   Output: Lab at the final position, whole, for every slot; a copy-only call (max_len == 0) writes the start labels.
 * Aliasing, checked by sgx_replay before anything is launched: with a NULL src_index_dev origin_in_dev == origin_out_dev is legal (a game's
 * labels are read whole before they are written, as its record is); any other overlap of the ranges src envs * 2 * cells and N * 2 * cells
 * elements, and with an index any overlap at all, is SGX_EINVAL.  Also SGX_EINVAL, from the setter: a NULL handle, a pointer that is not
 * 4-byte aligned.  A NULL origin_out_dev clears the setting (origin_in_dev is then ignored).
 * The setting is not game state: sgx_copy_envs, snapshots and start pools do not carry it, and sgx_destroy frees nothing for it.  Live
 * stepping, playouts and sgx_expand_all do not track.  Added without a change to an existing struct or signature: SGX_ABI_VERSION stays.
 * Reference counterpart: none -- a dict of piece ids kept by the caller next to env.step() in a loop. */
int sgx_set_replay_origins(sgx_env *h, const int16_t *origin_in_dev /* nullable */, int16_t *origin_out_dev /* NULL = clear */);
int sgx_replay_origins_set(const sgx_env *h);   /* 1 / 0 */

/* Expand all: every valid move of every root, pool to pool -- "all children of these nodes", what MCTS / ISMCTS node expansion, an
 * exhaustive shallow search and a perft-style check of the move generator start with -- without a mask, a nonzero() or an action list on
 * the host.  sgx_count_moves counts the moves per root and scans the counts into offsets; sgx_expand_all writes a window of the children.
 * THE RULE (tests/children_rule.py restates it on the CPU oracle, bit for bit):
 *   For root slot i in [0, n_roots): pos = record src_index[i] of src (i when the index is NULL); m = the valid-action mask of pos's mover
 *   in its own perspective (the bits sgx_observe writes for that record).
 *   count[i] = the number of moves in m: 0 for a finished game and for a mover without a move -- the no-op entry is never a child.
 *   offsets[0] = 0, offsets[i + 1] = offsets[i] + count[i], as int64; total = offsets[n_roots].
 *   Child c in [0, total): its root is the i with offsets[i] <= c < offsets[i + 1], its rank k = c - offsets[i], its action a the k-th set
 *   entry of m in ascending flat order (the order the playout's sampler and sgx_sample_valid count in).
 *   A call covers the window [first_child, first_child + n_children): slot j of dst belongs to child c = first_child + j.
 *   c < total: dst[j] = pos advanced by a exactly as sgx_step applies an action (the same endings, no auto-reset); parent[j] = i (the
 *   position in the root list, not src_index[i]); action[j] = a, the flat spatial index in the mover's perspective that sgx_step, sgx_replay
 *   and sgx_choose_actions take -- with SGX_CHILDREN_ACTIONS_1D the absolute 1-D index sgx_expand takes (SGX_STEP_ACTIONS_1D), through the
 *   map of the 1-D mask emission (SGX_STEP_MASK_1D); the ORDER of the children is the perspective order in both forms; reward[j], done[j],
 *   ending_invalid[j], player[j] = what that step reports for the child.
 *   c >= total: record j of dst is left as it was, parent[j] = action[j] = -1, the other outputs are not written.
 *   The kernel regenerates the root's mask and so knows the true count: a rank k >= count[i] (offsets that do not belong to these roots) is
 *   a "no child" slot like c >= total, never an out-of-range read; the search of offsets takes a constant number of steps and stays inside
 *   [0, n_roots) whatever the array holds (offsets_dev must hold n_roots + 1 readable entries).
 * Nothing is drawn: dst's seed does not enter.  src is only read.
 * SGX_EINVAL, before anything is launched: a NULL handle or io; handles of different devices or variants; src == dst (children would
 * overwrite roots); a dst with a start pool set; n_children > dst's envs; a negative n_roots, n_children or first_child (n_roots < 2^31);
 * without an index n_roots > src's envs; unknown flag bits; offsets_dev NULL; a misaligned pointer (offsets_dev 16 bytes; src_index_dev,
 * counts_dev, parent_dev, action_dev, reward_dev 4; the byte tensors any address).  n_roots == 0: sgx_count_moves writes offsets[0] = 0 and
 * launches no kernel; n_children == 0: sgx_expand_all launches nothing.  sgx_expand_all sets dst's sgx_last_launch_kind to
 * SGX_LAUNCH_CHILDREN.  The scan's scratch (and the counts when counts_dev is NULL) lives in the src handle: allocated at first use, freed
 * by sgx_destroy; no workgroup of the scan waits on another.  Added without a change to an existing struct or signature: SGX_ABI_VERSION
 * stays.  Reference counterpart: none -- get_next_state over np.nonzero(get_valid_moves_as_1d_mask) in a Python loop (penv:96-155). */
#define SGX_CHILDREN_ACTIONS_1D 1    /* action_dev holds absolute 1-D indices (as sgx_expand takes); default: flat spatial, mover's perspective */
int sgx_count_moves(sgx_env *src, const int32_t *src_index_dev, int64_t n_roots, int32_t *counts_dev /* [n_roots], nullable */,
                    int64_t *offsets_dev /* [n_roots + 1] */, void *stream);
typedef struct sgx_children_io {
    const int64_t *offsets_dev;   /* [n_roots + 1], from sgx_count_moves */
    int32_t *parent_dev, *action_dev;            /* [n_children] out, nullable */
    float   *reward_dev;          /* [n_children][2] out, nullable: rewards[+1], rewards[-1] of the step that made the child */
    uint8_t *done_dev, *ending_invalid_dev;      /* [n_children] out, nullable */
    int8_t  *player_dev;          /* [n_children] out, nullable: the mover at the child */
    int64_t n_roots, first_child, n_children;
    int32_t flags, reserved;
} sgx_children_io;                /* 7 pointers + 3 int64 + 2 int32 = 88 bytes */
int sgx_expand_all(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_children_io *io, void *stream);

/* Leaf values: what a position that is NOT over is worth, by a piece-square table -- so that a playout cut off by max_steps, a replayed
 * prefix and every child of sgx_expand_all carry an estimate where they reported 0, 0.  A SETTING OF THE dst HANDLE, like sgx_set_start_pool:
 * sgx_playout, sgx_playout_weighted, sgx_replay and sgx_expand_all pick it up from their dst; sgx_replay with max_len == 0 is the
 * stand-alone "score this pool" call.  No existing struct or signature changed: SGX_ABI_VERSION stays.
 * THE RULE is defined on the reference state, not on the record layout (tests/leaf_values_rule.py restates it in numpy, known answers
 * included).  For state int64 [34][R][C] (absolute coordinates), cells = R * C, cell = r * C + c, and the table T = int16 [2][14][cells]:
 *   own(p)  = layer 0 for player +1, layer 1 for -1 (true pieces, 1..12);
 *   pub(p)  = layer 3 for +1, layer 4 for -1 (what p's opponent knows of p's pieces: 1..12 identified, 13 unidentified);
 *   persp(p, cell) = cell for +1, cells - 1 - cell for -1: the board turned into the owner's perspective, so a table row means "this far
 *     advanced" for either player;
 *   mine(p)   = the sum of T[0][t][persp(p, cell)], t = state[own(p)][cell], over the non-zero cells of own(p);
 *   theirs(p) = the sum of T[1][d][persp(-p, cell)] over the non-zero cells of the layer d is read from: d = state[pub(-p)][cell] (what p
 *     sees; the default), or with SGX_LEAF_SEE_ALL d = state[own(-p)][cell] (the usual choice inside a determinized world);
 *     rows T[.][0] and T[0][13] are never read;
 *   S(p) = mine(p) - theirs(p) in int32 (|S| <= 2 * 1,024 * 32,768);
 *   v(p) = float32(clamp(S(p), -limit, limit)) / float32(denom): ONE IEEE division of two integers of magnitude <= 2^24.
 * With a table set on dst, every slot whose reported position is not over gets reward[+1] = v(+1), reward[-1] = v(-1) -- in the public
 * view each is that player's OWN estimate, not the negative of the other's.  done, ending_invalid, player, length, applied / consumed /
 * stop, parent / action and the records written are what they are without a table; a finished position reports what it reports without
 * one (0, 0 for a max-turn ending and an invalid ending, the 1e-4 of a tie included); "no child" slots of sgx_expand_all are still not
 * written; nothing is drawn.  With no table set every byte of every output is what it was.  sgx_step and all live-env stepping, sgx_expand
 * and sgx_step_states never use the table.  limit < denom keeps leaf values strictly inside a win's +-1.
 * table_host is HOST memory, copied into a device buffer the handle owns (freed by sgx_destroy); NULL clears the setting and ignores the
 * other arguments.  The call WAITS FOR THE DEVICE: launches in flight finish with the table they were launched with, and the old buffer is
 * freed only then; every later launch takes the new one.  The table is a setting, not game state: sgx_copy_envs, snapshots and start pools
 * do not carry it.  SGX_EINVAL, before anything is uploaded: a NULL handle, limit or denom outside 1 <= limit <= denom <= 2^24, unknown
 * flag bits.  Reference counterpart: none -- a Python evaluation of every leaf state on the host. */
#define SGX_LEAF_SEE_ALL 1             /* flags: the opponent's pieces are valued by their true types, not by what the player has seen of them */
int sgx_set_leaf_values(sgx_env *h, const int16_t *table_host /* [2][14][cells], NULL = clear */, int32_t limit, int32_t denom, int32_t flags);
int sgx_leaf_values_set(const sgx_env *h);   /* 1 / 0 */

/* Position keys: one 64-bit key per packed record (two with SGX_KEYS_WIDE), in one launch straight from the record -- what a transposition
 * table, the node map of ISMCTS, the deduplication of a start pool and "have I seen this root" need, without an unpack to the int64 layers.
 * Two views: the STATE key is equal exactly when the reference state (its 34 layers) and the mover are equal; the INFORMATION-SET key of
 * a player is equal exactly when everything that player can see is equal -- both up to a 64-bit collision (2^-64 per pair; the wide key's
 * second word is an independent hash of the same features).
 * THE RULE is defined on the reference state, not on the record layout (tests/keys_rule.py restates it in numpy, known answers included):
 *   sm_fin(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (64-bit, the library's finaliser)
 *   feat(word, slot, value) = sm_fin(SALT[word] + 0x9E3779B97F4A7C15 * (((slot mod 2^32) << 32 | (value mod 2^32)) + 1)),
 *   SALT = {0x5347584B45595330, 0x5347584B45595331}; value is taken in two's complement.
 *   For state int64 [34][R][C] (absolute coordinates) with mover `player`: x = the XOR of
 *     feat(word, l * 1024 + cell, state[l][cell]) over every NON-ZERO entry of every layer l except 2 (obstacles: a constant of the variant),
 *       5 (the scalars, below) and, for an information-set key, the true-piece layer of the observer's opponent (layer 1 for observer +1,
 *       layer 0 for observer -1); cell = r * C + c;
 *     feat(word, 5 * 1024 + i, s_i) for the scalars s_0 .. s_3 = game over [5][0][1], winner [5][0][2], ending invalid [5][1][1], the mover --
 *       and, unless SGX_KEYS_NO_CLOCK, s_4 = turn count [5][0][0], s_5 = max turns [5][1][0] -- hashed whether zero or not;
 *     feat(word, 5 * 1024 + 6, observer) for an information-set key (observer = +1 / -1 after view 0 has been resolved to the mover).
 *   key = sm_fin(x).  Word 0 is the 64-bit key; SGX_KEYS_WIDE adds word 1.
 * So: with the clock two positions share a state key exactly when layers and mover agree; SGX_KEYS_NO_CLOCK leaves turn count and max turns
 * out, so transpositions reached in another number of moves match; an information-set key covers the observer's own pieces, both public
 * layers, the recent-move layers, the capture counts, the never-moved layers, the scalars, the mover and who observes -- every world
 * sgx_determinize deals for observer p copies those bit for bit and so has the information-set key of its root.  The game number is not in
 * the reference state and not in the key.  A capture count is hashed as the count: on a variant with more than 8 pieces of a type the
 * chained events of one (layer, cell) are summed first.  Like sgx_determinize the information-set key follows the tracked state, not the
 * move history.
 * keys_dev[i] (keys_dev[2i], keys_dev[2i + 1] with SGX_KEYS_WIDE) = the key of record src_index_dev[i] of src, of record i when the index is
 * NULL (then n <= src's envs); index entries must be valid records of src, as for sgx_count_moves.  src is only read -- a pool, or a live env
 * between launches; the call is asynchronous on `stream`, restores the caller's device, launches nothing for n == 0 and leaves
 * sgx_last_launch_kind alone.  SGX_EINVAL, before anything is launched: a NULL handle or keys_dev, n outside [0, 2^31), without an index
 * n > src's envs, a view outside {-1, 0, 1, SGX_KEYS_VIEW_STATE}, unknown flag bits, a misaligned pointer (keys_dev 8 bytes, 16 with
 * SGX_KEYS_WIDE; src_index_dev 4).  Added without a change to an existing struct or signature: SGX_ABI_VERSION stays.
 * Reference counterpart: none -- hashing state.tobytes() and the player on the host. */
#define SGX_KEYS_VIEW_STATE 2      /* view: 0 = each record's mover, +1 / -1 = that player (as sgx_determinize's observer), 2 = state key */
#define SGX_KEYS_NO_CLOCK 1        /* flags: turn count and max turns stay out of the key */
#define SGX_KEYS_WIDE     2        /* keys_dev is uint64 [n][2]: word 0 and word 1 (a 128-bit key) */
int sgx_state_keys(sgx_env *src, const int32_t *src_index_dev, int64_t n, int32_t view, int32_t flags, uint64_t *keys_dev, void *stream);

/* Per-env bookkeeping: int32 [N][4] = {turn count, game number, game_over, current player}. */
int sgx_get_env_info(sgx_env *h, int32_t *info_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STRATEGO_MI355X_H */
