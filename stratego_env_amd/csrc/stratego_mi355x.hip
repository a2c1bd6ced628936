// stratego_mi355x.hip -- HIP kernels (gfx950 / CDNA4) and C-ABI of the batched Stratego env.
//
// One wavefront (64 lanes) per game; boards of <= 32 cells share a wave between 2 or 4 games (Geo::LPG lanes per game).
// A game's compact state record (4 dense int8 boards + bitmaps + scalars + capture events, whole 128-byte lines) is expanded
// to 32 boards in LDS, the move is applied there, the next mover's valid-actions mask is built in LDS as bits and its
// 67-channel normalised observation is rendered straight into line-aligned 16-byte global stores.
// HBM-bound integer/byte work: no MFMA.  See DESIGN.md for the data layout and byte accounting.
// Device code lives in the sgx_*.h headers included below (one translation unit, in this order); this file holds the error
// plumbing and the host side of the C ABI.
//
// Reference functions reproduced (paths relative to /root/reference/stratego_env):
//   game/stratego_procedural_impl.py  (impl)   stratego_multiagent_env.py (maenv)   game/util.py (util)
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <sched.h>
#include <time.h>
#include <string.h>
#include <string>
#include <vector>

#include "stratego_mi355x.h"

#define SGX_API extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, const char *detail = "") {
    char buf[512];
    snprintf(buf, sizeof(buf), fmt, detail);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(SGX_EDEVICE, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

// Every entry point that touches the device runs on the handle's device and puts the caller's current device back on every
// return path: a process that drives several handles on several GPUs (SURVEY 8e's other layout: one thread + stream per GPU), or
// that sits inside a torch.cuda.device(...) scope, never finds its device switched under it.
struct DeviceGuard {
    int prev = -1;
    bool restore = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            restore = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (restore) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define SGX_ON_DEVICE(dev)                                                                                      \
    DeviceGuard device_guard_(dev);                                                                             \
    if (device_guard_.err != hipSuccess) return fail(SGX_EDEVICE, "selecting the handle's device: %s", hipGetErrorString(device_guard_.err))

// Hash of the sources this binary was compiled from (stratego_env_amd/build.py: source_hash() over csrc/* and the ABI header,
// passed as -DSGX_BUILD_ID): _lib.load() refuses a library whose id differs from the sources next to it, build.needs_build()
// reads the marker straight from the file.
#ifndef SGX_BUILD_ID
#define SGX_BUILD_ID "unknown"
#endif
const char g_build_id[] = "SGX_BUILD_ID=" SGX_BUILD_ID;

}  // namespace

#include "sgx_store_policy.h"
#include "sgx_layout.h"
#include "sgx_obs.h"
#include "sgx_mask.h"
#include "sgx_setup.h"
#include "sgx_step.h"
#include "sgx_pool_frame.h"
#include "sgx_playout.h"
#include "sgx_step_vs.h"
#include "sgx_replay.h"
#include "sgx_children.h"
#include "sgx_keys.h"
#include "sgx_lane.h"
#include "sgx_lane_kernel.h"
#include "sgx_aux_kernels.h"
#include "sgx_determinize_weighted.h"
#include "sgx_choose.h"
#include "sgx_mem.h"


// =============================================================================================
// Host side: handle + C ABI
// =============================================================================================
struct sgx_env {
    sgx_config cfg;
    int64_t n_envs;
    int device;
    uint64_t seed;
    int64_t env_id_offset;
    int8_t *boards;
    DevTables *tab;
    uint8_t *setups;
    int64_t n_setups;
    int rec_bytes;
    int sc_off;
    int max_events;
    int K;
    unsigned long long *stamps;  // SGX_STAMPS builds only
    int map_mode, map_arg;       // SGX_MAP experiment (group_of_block)
    int xcd_skew;                // sgx_set_xcd_skew: per mille more work for the even XCDs; -1 = by the launch's output size
    int xcd_explicit;            // xcd_w was set by sgx_set_xcd_shares: it overrides the skew rule
    int32_t xcd_w[8];            // shares of the eight XCDs, per mille of the mean share (sum 8000)
    int nt_mode;                 // sgx_set_nt_stores: -1 = by the launch's output size, 0 = never, 1 = always
    int plain_lines_forced;      // SGX_NT_PLAIN_LINES: -1 = the rule of sgx_store_policy.h, else non-temporal stores with this many leading plain lines
    int cus;                     // compute units of the device
    int steps_wg_per_cu[2][2];   // resident workgroups per CU of steps_kernel / steps_kernel_pool<R, C, KIND 0 | 1> (occupancy query at first use; 0 = not asked yet)
    int policy_debug;            // SGX_STORE_POLICY_DEBUG=1: steps_policy prints what it chose to stderr whenever the choice changes
    int policy_printed[4];       // ... the last choice printed (sets, nt_stores, plain_lines, resident workgroups per CU)
    int lane_mode;               // sgx_set_lane_kernel: 0 = never the lane-per-game kernel, otherwise wherever it is eligible
    float placement_target_us;   // sgx_set_placement_target: sgx_alloc_outputs searches on until a candidate is within 3 % of it (0 = its own stop rules)
    hipStream_t chain_stream[SGX_MAX_CHAINS];   // sgx_rollout: created on first use
    hipEvent_t chain_fork, chain_join[SGX_MAX_CHAINS];
    // sgx_step_sync on a handful of games (single_kernel): a host-mapped word the kernel publishes its sequence number in, and the
    // device counter of finished workgroups; created on first use
    uint32_t *sync_flag_host, *sync_flag_dev, *sync_count;
    uint32_t sync_seq;
    int no_single;               // SGX_NO_SINGLE=1: sgx_step_sync never takes the single_kernel path (A/B measurements)
    uint8_t *san_flags;          // sgx_step_states: per-state "had to be altered" flags when the caller passes none (created on first use)
    int32_t *redo_list;          // sgx_step_states: [n_envs] ids of the states the first pass had to alter, then the counter (created on first use)
    int general_states;          // sgx_set_general_states: 0 = flagged states stay sanitised, otherwise the second, general-state pass redoes them
    int no_multi_step;           // SGX_MULTI_STEP=0 (or a runtime that refuses the LDS size): sgx_step_n / sgx_step_ring never take lane_steps_kernel
    int multi_step_attr;         // lane_steps_kernel's dynamic-LDS attribute has been raised
    int multi_step_attr_pool;    // ... and lane_steps_kernel_pool's
    int last_kind;               // sgx_last_launch_kind: which kernel the last step / observe launch of this handle was
    int multi_step_wave;         // SGX_MULTI_STEP_WAVE: the multi-step launch of the wave-per-game kernels (steps_kernel) too
    int steps_barrier;           // sgx_set_steps_barrier / SGX_STEPS_BARRIER: -1 auto (long rings that render float32 observations: steps_kernel), 0 never, 1 always
    int half_wave;               // SGX_HALF_WAVE: launches without an observation play two games per wave where the board allows it (Geo<R, C, 2>)
    // sgx_step_ring with more output sets than fit the kernel arguments: the sets' pointers in a device table, written by ring_table_kernel
    // from its own launch arguments (no staging buffer, so no upload ever waits on the host).  ring_tab_host is a plain host mirror of what
    // the table holds; ring_tab_ev is recorded behind every upload AND behind every launch that reads the table, on ring_tab_stream: whoever
    // touches the table next from another stream waits for it on the device.
    void **ring_tab_dev, **ring_tab_host;
    int ring_tab_cap, ring_tab_n;
    hipEvent_t ring_tab_ev;
    hipStream_t ring_tab_stream;
    // sgx_set_start_pool: the handle's OWN copy of the pool's records (NULL = none: games start from sampled setups), their number and the
    // SGX_POOL_* flags the kernels look at; sgx_set_start_index_out: where the launches write the pool index of every env's current game
    int8_t *pool;
    int64_t n_pool;
    int pool_flags;
    int32_t *start_index;
    // sgx_count_moves: the counts when the caller takes none, and the block sums of the offsets scan (created on first use, grown on demand)
    int32_t *count_scratch;
    int64_t *scan_sums;
    int64_t count_scratch_cap, scan_sums_cap;
    // sgx_set_leaf_values: the handle's device copy of the table (int16 [LEAF_ROWS][cells], zeros behind the caller's 28 rows; NULL = none)
    // and what goes with it into the launches this handle is dst of
    int16_t *leaf_table;
    int32_t leaf_limit, leaf_denom, leaf_see_all;
    // sgx_set_replay_origins: the caller's label tensors (origin_out NULL = none); while set, sgx_replay with this handle as dst tracks labels
    const int16_t *origin_in;
    int16_t *origin_out;
};

namespace {

// Board sizes compiled into this library.  Every reference variant (game/config.py) is built in; any other size (rows, cols >= 3,
// rows * cols <= SGX_MAX_CELLS) gets a library of its own, compiled from the same sources with -DSGX_EXTRA_R=<rows>
// -DSGX_EXTRA_C=<cols> -DSGX_ONLY_EXTRA (stratego_env_amd/build.py: build_geometry), like the reference's
// StrategoProceduralEnv(rows, columns) accepts any size (penv:27-36).
#ifdef SGX_ONLY_EXTRA
#define SGX_BUILTIN_GEOMETRIES(X, A)
#else
#define SGX_BUILTIN_GEOMETRIES(X, A) X(A, 10, 10) X(A, 15, 15) X(A, 8, 8) X(A, 6, 6) X(A, 5, 5) X(A, 4, 4) X(A, 3, 4)
#endif
#ifdef SGX_EXTRA_R
#define SGX_EXTRA_GEOMETRY(X, A) X(A, SGX_EXTRA_R, SGX_EXTRA_C)
static_assert(SGX_EXTRA_R >= 3 && SGX_EXTRA_C >= 3 && SGX_EXTRA_R * SGX_EXTRA_C <= SGX_MAX_CELLS, "SGX_EXTRA_R x SGX_EXTRA_C out of range");
#else
#define SGX_EXTRA_GEOMETRY(X, A)
#endif
#define SGX_ALL_GEOMETRIES(X, A) SGX_BUILTIN_GEOMETRIES(X, A) SGX_EXTRA_GEOMETRY(X, A)

bool supported_geometry(int r, int c) {
#define SGX_MATCH(A, R, C) if (r == (R) && c == (C)) return true;
    SGX_ALL_GEOMETRIES(SGX_MATCH, _)
#undef SGX_MATCH
    return false;
}

template <int N> using int_c = std::integral_constant<int, N>;
template <bool B> using bool_c = std::integral_constant<bool, B>;

// The one place a board size becomes template arguments: calls f(int_c<R>, int_c<C>) for the handle's board (the callee reads them as
// decltype(r)::value); a launch that only some boards have sits under `if constexpr` inside f.
template <class F>
int for_geometry(const sgx_env *h, F &&f) {
    const int r = h->cfg.rows, c = h->cfg.cols;
#define SGX_DISPATCH_ONE(A, R, C) if (r == (R) && c == (C)) { f(int_c<(R)>(), int_c<(C)>()); return SGX_OK; }
    SGX_ALL_GEOMETRIES(SGX_DISPATCH_ONE, _)
#undef SGX_DISPATCH_ONE
    return fail(SGX_EINVAL, "unsupported board size%s");
}

// bytes of one game's compact observation record (SGX_STEP_COMPACT_OBS): 4-bit codes padded to 16 B, a 16-byte header, then room for
// every entry that can be without a code (capture events + the four recent-move pairs) as {uint32 entry, float value}; whole 128-byte lines
int compact_capacity(const sgx_env *h) { return h->max_events + 4; }
int compact_obs_stride(const sgx_env *h) {
    const int nib = ((h->cfg.rows * h->cfg.cols * OBS_CH + 1) / 2 + 15) & ~15;
    return (nib + 16 + 8 * compact_capacity(h) + 127) & ~127;
}
int mask_words(const sgx_env *h) {
    const int na = h->cfg.rows * h->cfg.cols * h->K;
    return (((na + 31) / 32 + 1) + 3) & ~3;                          // Geo::MB_WORDS
}

KParams make_params(const sgx_env *h) {
    KParams p;
    memset(&p, 0, sizeof(p));
    p.boards = h->boards;
    p.tab = h->tab;
    p.setups = h->setups;
    p.n_setups = (int32_t)h->n_setups;
    p.max_turns = h->cfg.max_turns;
    p.usable_rows = h->cfg.usable_rows;
    for (int i = 0; i < 12; ++i) p.piece_counts[i] = h->cfg.piece_counts[i];
    p.rec_bytes = h->rec_bytes;
    p.max_events = h->max_events;
    for (int i = 0; i < 12; ++i)
        if (h->cfg.piece_counts[i] > EV_COUNT_MAX) p.multi_ev = 1;
    p.compact_stride = compact_obs_stride(h);
    p.n_envs = h->n_envs;
    p.seed = h->seed;
    p.env_id_offset = h->env_id_offset;
#ifdef SGX_STAMPS
    p.stamps = h->stamps;
#endif
    return p;
}

// what the *_pool kernels take next to KParams; start_index moved on by `index_off` entries (a step of an sgx_step_traj call as a launch of its own)
PoolParams make_pool_params(const sgx_env *h, int64_t index_off = 0) {
    PoolParams pp;
    pp.pool = h->pool;
    pp.n_pool = (int32_t)h->n_pool;
    pp.pool_flags = h->pool_flags;
    pp.start_index = (h->pool && h->start_index) ? h->start_index + index_off : nullptr;
    return pp;
}

int check_cfg(const sgx_config *cfg) {
    if (!cfg) return fail(SGX_EINVAL, "cfg is NULL%s");
    if (cfg->rows < 3 || cfg->cols < 3) return fail(SGX_EINVAL, "Both rows and columns have to be at least 3%s");
    if (cfg->rows * cfg->cols > SGX_MAX_CELLS) return fail(SGX_EINVAL, "rows*cols exceeds SGX_MAX_CELLS%s");
    if (cfg->usable_rows < 1 || cfg->usable_rows * 2 > cfg->rows) return fail(SGX_EINVAL, "usable_rows out of range%s");
    for (int i = 0; i < 12; ++i) {
        if (cfg->piece_counts[i] < 0) return fail(SGX_EINVAL, "negative piece count%s");
        // (a capture event counts to 8 = the scouts of Standard; a variant with more pieces of one type chains events: KParams::multi_ev)
        if (cfg->piece_counts[i] > SGX_MAX_PIECES_PER_TYPE) return fail(SGX_EINVAL, "more than 127 pieces of one type per side%s");
    }
    // (more pieces than usable cells is legal for a handle that never samples random setups: an env_config that overrides
    //  'piece_amounts' changes the normalisation only; sgx_reset checks it where it matters)
    if (cfg->capture_capacity < 0 || 2 * cfg->capture_capacity > cfg->rows * cfg->cols) return fail(SGX_EINVAL, "capture_capacity out of range%s");
    return SGX_OK;
}

}  // namespace

// sampled setups without a table place piece_counts pieces on the usable back rows: they have to fit
static int check_random_setups(const sgx_env *h) {
    if (h->setups || h->pool) return SGX_OK;          // (a start pool: no game start samples a setup)
    int total = 0;
    for (int i = 0; i < 12; ++i) total += h->cfg.piece_counts[i];
    if (total > h->cfg.usable_rows * h->cfg.cols) return fail(SGX_EINVAL, "random setups: more pieces than usable cells%s");
    return SGX_OK;
}

SGX_API int sgx_abi_version(void) { return SGX_ABI_VERSION; }
SGX_API const char *sgx_build_id(void) { return g_build_id + 13; }
SGX_API int sgx_supports_geometry(int32_t rows, int32_t cols) { return supported_geometry(rows, cols) ? 1 : 0; }
SGX_API const char *sgx_last_error(void) { return g_last_error.c_str(); }
SGX_API int64_t sgx_num_envs(const sgx_env *h) { return h ? h->n_envs : 0; }
SGX_API int64_t sgx_record_bytes(const sgx_env *h) { return h ? h->rec_bytes : 0; }
SGX_API int sgx_spatial_channels(const sgx_env *h) { return h ? h->K : 0; }
SGX_API int64_t sgx_num_spatial_actions(const sgx_env *h) { return h ? (int64_t)h->cfg.rows * h->cfg.cols * h->K : 0; }
SGX_API int64_t sgx_action_size_1d(const sgx_env *h) {
    return h ? (int64_t)h->cfg.rows * h->cfg.cols * (h->cfg.rows + h->cfg.cols) + 1 : 0;
}

// Normalisation LUT [channels][LUT_STRIDE]: entry i of a channel's row = the float32 the reference produces for board value i
// (recent-moves channels: value i - 3).  Extended channel layout = [n_own_true][n_enemy_true][13 own PO][13 enemy PO]
// [obstacle][2 recent][12+12 captured][2 still]; partial has no enemy-true block (impl:1306-1332 vs impl:1200-1227);
// highs/lows maenv:202-313.  Original layout (value channels): partial impl:1126-1148 with maenv:146-199, full impl:1048-1070
// with maenv:87-143.  ranges/mids maenv:388-396, (x - mid) / range in float32 maenv:499-508.
static int lut_channels(bool full, bool original) {
    return original ? (full ? SGX_FO_OBS_CHANNELS_ORIGINAL : SGX_PO_OBS_CHANNELS_ORIGINAL) : (full ? FOBS_CH : OBS_CH);
}
static void build_lut(const sgx_config *cfg, bool full, float *lut, bool raw_values = false, bool original = false) {
    const int nch = lut_channels(full, original);
    enum { ONEHOT, VALUE, RECENT };
    float hi[FOBS_CH], lo[FOBS_CH];
    int kind[FOBS_CH], type[FOBS_CH];
    int rec0, cap0;
    for (int ch = 0; ch < nch; ++ch) { hi[ch] = 1.0f; lo[ch] = -1.0f; kind[ch] = VALUE; type[ch] = 0; }
    if (!original) {
        const int n_true = full ? 24 : 12, po_end = n_true + 26;
        for (int ch = 0; ch < po_end; ++ch) {          // one-hot piece channels: raw = (board value == piece type)
            kind[ch] = ONEHOT;
            type[ch] = ch < n_true ? ch % 12 + 1       // true pieces: types 1..12
                                   : (ch - n_true) % 13 + 1;   // PO pieces: types 1..13
        }
        rec0 = po_end + 1; cap0 = po_end + 3;
        for (int ch = cap0; ch < cap0 + 24; ++ch) { hi[ch] = 8.0f; lo[ch] = 0.0f; }
    } else {
        for (int ch = 0; ch < nch; ++ch) { hi[ch] = 2.0f; lo[ch] = 0.0f; }   // obstacles, captured, still
        if (full) {
            hi[0] = hi[1] = (float)SP_BOMB; hi[5] = hi[6] = (float)SP_UNKNOWN;
            rec0 = 3; cap0 = 7;
        } else {
            hi[0] = (float)SP_BOMB; hi[1] = hi[2] = (float)SP_UNKNOWN;
            rec0 = 4; cap0 = 6;
        }
    }
    kind[rec0] = kind[rec0 + 1] = RECENT;
    hi[rec0] = hi[rec0 + 1] = 1.0f; lo[rec0] = lo[rec0 + 1] = -3.0f;   // RecentMoves JUST_CAME_FROM .. JUST_ARRIVED_AND_CANT_DOUBLE_BACK
    for (int t = 1; t <= 12; ++t)
        if (cfg->piece_counts[t - 1] > 1) hi[cap0 + t - 1] = hi[cap0 + 12 + t - 1] = (float)cfg->piece_counts[t - 1];
    for (int ch = 0; ch < nch; ++ch) {
        volatile float range = (hi[ch] - lo[ch]) / 2.0f, mid = (hi[ch] + lo[ch]) / 2.0f;
        for (int i = 0; i < LUT_STRIDE; ++i) {
            float raw;
            if (kind[ch] == ONEHOT) raw = (i == type[ch]) ? 1.0f : 0.0f;
            else if (kind[ch] == RECENT) raw = (float)(i - 3);
            else raw = (float)i;
            volatile float d = raw - mid;        // two IEEE float32 roundings, as numpy does
            lut[ch * LUT_STRIDE + i] = raw_values ? raw : d / range;
        }
    }
}

// 'extended' observations are rendered from 4-bit codes (sgx_obs.h): code c decodes to sext(c) / 4.  Templates of the channel
// defaults and the codes of captured counts / recent-move codes, derived from the LUTs themselves.
static int float_code(float f) {
    for (int c = 0; c < 16; ++c)
        if (c != CODE_ESC && (float)(c < 8 ? c : c - 16) / 4.0f == f) return c;    // (CODE_ESC marks uncoded entries)
    return CODE_NONE;
}
static int build_code_tables(const sgx_config *cfg, DevTables *tab) {
    const int rc_cells = cfg->rows * cfg->cols;
    float dense[2][FOBS_CH * LUT_STRIDE];
    for (int raw = 0; raw < 2; ++raw) {
        for (int full = 0; full < 2; ++full) {
            build_lut(cfg, full != 0, dense[full], raw != 0, false);
            const int nch = full ? FOBS_CH : OBS_CH, rec0 = full ? 51 : 39;
            uint8_t *t = tab->tmpl[2 * raw + full];
            memset(t, 0, TMPL_MAX_BYTES);
            for (int ch = 0; ch < nch; ++ch) {
                const bool rec = ch == rec0 || ch == rec0 + 1;
                const int code = float_code(dense[full][ch * LUT_STRIDE + (rec ? 3 : 0)]);
                if (code == CODE_NONE) return fail(SGX_EINVAL, "a channel default has no 4-bit code%s");
                // indicator channels (one-hot blocks, obstacle, never-moved): the value of a set entry must decode from NIB_ONE
                const int n_true = full ? 24 : 12, po_end = n_true + 26;
                int set_index = -1;
                if (ch < n_true) set_index = ch % 12 + 1;
                else if (ch < po_end) set_index = (ch - n_true) % 13 + 1;
                else if (ch == po_end || ch >= nch - 2) set_index = 1;
                if (set_index >= 0 && float_code(dense[full][ch * LUT_STRIDE + set_index]) != NIB_ONE)
                    return fail(SGX_EINVAL, "an indicator channel's set value is not 1.0%s");
                for (int cell = 0; cell < rc_cells; ++cell) {
                    const int e = cell * nch + ch;
                    t[e >> 1] |= (uint8_t)(code << (4 * (e & 1)));
                }
            }
        }
        uint8_t *ct = tab->codetab[raw];
        memset(ct, CODE_NONE, CODETAB_BYTES);
        for (int t = 0; t < 12; ++t)
            for (int v = 0; v < LUT_STRIDE; ++v) {
                // own and enemy block, partial and full kind: the same normalisation per piece type (maenv:288-298 / 229-239)
                const float f = dense[0][(41 + t) * LUT_STRIDE + v];
                if (f != dense[0][(53 + t) * LUT_STRIDE + v] || f != dense[1][(53 + t) * LUT_STRIDE + v] || f != dense[1][(65 + t) * LUT_STRIDE + v])
                    return fail(SGX_EINVAL, "captured-count channels of one piece type are normalised differently%s");
                ct[16 * t + v] = (uint8_t)float_code(f);
            }
        for (int v = 0; v < 5; ++v) {
            const float f = dense[0][39 * LUT_STRIDE + v];
            if (f != dense[0][40 * LUT_STRIDE + v] || f != dense[1][51 * LUT_STRIDE + v] || f != dense[1][52 * LUT_STRIDE + v])
                return fail(SGX_EINVAL, "recent-move channels are normalised differently%s");
            ct[CODETAB_REC + v] = (uint8_t)float_code(f);
        }
    }
    return SGX_OK;
}

SGX_API int sgx_build_obs_lut(const sgx_config *cfg, float *lut) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!lut) return fail(SGX_EINVAL, "lut is NULL%s");
    build_lut(cfg, false, lut);
    return SGX_OK;
}

SGX_API int sgx_build_full_obs_lut(const sgx_config *cfg, float *lut) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!lut) return fail(SGX_EINVAL, "lut is NULL%s");
    build_lut(cfg, true, lut);
    return SGX_OK;
}

SGX_API int sgx_build_original_obs_lut(const sgx_config *cfg, int32_t full, float *lut) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!lut) return fail(SGX_EINVAL, "lut is NULL%s");
    build_lut(cfg, full != 0, lut, false, true);
    return SGX_OK;
}

SGX_API int sgx_create(const sgx_config *cfg, int64_t n_envs, int device, uint64_t seed, int64_t env_id_offset, sgx_env **out) {
    if (!out) return fail(SGX_EINVAL, "out is NULL%s");
    *out = nullptr;
    if (int rc = check_cfg(cfg)) return rc;
    if (!supported_geometry(cfg->rows, cfg->cols))
        return fail(SGX_EINVAL, "board size not compiled into this library (built in: 10x10, 15x15, 8x8, 6x6, 5x5, 4x4, 3x4; any other size: "
                                "build the same sources with -DSGX_EXTRA_R=<rows> -DSGX_EXTRA_C=<cols>, stratego_env_amd/build.py build_geometry)%s");
    if (n_envs <= 0 || n_envs > (int64_t)1 << 30) return fail(SGX_EINVAL, "n_envs out of range%s");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(SGX_EDEVICE, "no HIP device available: %s", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(SGX_EINVAL, "device index out of range%s");
    SGX_ON_DEVICE(device);
    sgx_env *h = new sgx_env();
    memset(h, 0, sizeof(*h));
    h->cfg = *cfg;
    h->n_envs = n_envs;
    h->device = device;
    h->seed = seed;
    h->env_id_offset = env_id_offset;
    h->nt_mode = -1;
    if (const char *e = getenv("SGX_NT")) {           // SGX_NT=0|1|auto: the default of sgx_set_nt_stores for new handles
        if (!strcmp(e, "0")) h->nt_mode = 0;
        else if (!strcmp(e, "1")) h->nt_mode = 1;
    }
    h->plain_lines_forced = -1;
    if (const char *e = getenv("SGX_NT_PLAIN_LINES")) {     // SGX_NT_PLAIN_LINES=<count>: non-temporal stores with that many leading plain lines; -1 = auto
        char *end = nullptr;
        const long v = strtol(e, &end, 10);                  // ("auto", "" or any other text that is not a number: unset)
        if (end != e && *end == 0) h->plain_lines_forced = v < 0 ? -1 : v > 0x7FFF ? 0x7FFF : (int)v;   // (KParams carries it in a halfword; no board has 2,600 lines)
    }
    if (const char *e = getenv("SGX_STORE_POLICY_DEBUG")) {
        h->policy_debug = !strcmp(e, "1");
        h->policy_printed[0] = -1;
    }
    h->lane_mode = -1;
    h->general_states = 1;
    if (const char *e = getenv("SGX_GENERAL_STATES")) h->general_states = atoi(e);
    if (const char *e = getenv("SGX_LANE")) { if (!strcmp(e, "0")) h->lane_mode = 0; else if (!strcmp(e, "1")) h->lane_mode = 1; }   // SGX_LANE=0|1|auto
    h->xcd_skew = -1;
    if (const char *e = getenv("SGX_XCD_SKEW")) { if (strcmp(e, "auto")) h->xcd_skew = atoi(e); }   // SGX_XCD_SKEW=<per mille>|auto
    if (h->xcd_skew > 900) h->xcd_skew = 900;
    if (const char *e = getenv("SGX_NO_SINGLE")) h->no_single = atoi(e);
    if (const char *e = getenv("SGX_MULTI_STEP")) h->no_multi_step = !strcmp(e, "0");
    h->multi_step_wave = 1;
    if (const char *e = getenv("SGX_MULTI_STEP_WAVE")) h->multi_step_wave = strcmp(e, "0") != 0;
    h->half_wave = 1;
    if (const char *e = getenv("SGX_HALF_WAVE")) h->half_wave = strcmp(e, "0") != 0;
    h->steps_barrier = -1;
    if (const char *e = getenv("SGX_STEPS_BARRIER")) h->steps_barrier = !strcmp(e, "0") ? 0 : !strcmp(e, "1") ? 1 : -1;
    if (const char *e = getenv("SGX_MAP")) { h->map_mode = atoi(e); if (const char *c = strchr(e, ',')) h->map_arg = atoi(c + 1); }
    const int rc_cells = cfg->rows * cfg->cols;
    {
        int pieces = 0;
        for (int i = 0; i < 12; ++i) pieces += cfg->piece_counts[i];
        if (cfg->capture_capacity > pieces) pieces = cfg->capture_capacity;
        h->max_events = 2 * pieces;                                   // every piece can be captured once
        // ... and both sides together never have more pieces than the board has cells: Geo::EVL_MAX = rows * cols bounds the LDS event
        // lists and StateIO::IMG (an env_config that overrides 'piece_amounts' for the normalisation only -- Micro with Standard's 40
        // pieces -- would ask for 80 events on 12 cells otherwise)
        if (h->max_events > rc_cells) h->max_events = rc_cells;
        const int st_off = (STORED_BOARDS * ((rc_cells + 3) & ~3) + 15) & ~15, sb = (((rc_cells + 7) / 8) + 15) & ~15;
        const int sc_off = st_off + 2 * sb;
        h->sc_off = sc_off;
        h->rec_bytes = (sc_off + 32 + (rc_cells > 256 ? 4 : 2) * h->max_events + 127) & ~127;   // whole 128-byte lines per game (Geo::ev_t events)
    }
    h->K = 2 * (cfg->rows - 1) + 2 * (cfg->cols - 1) + 1;
    DevTables host_tab;
    memset(&host_tab, 0, sizeof(host_tab));
    {   // ABI LUTs [channels][16] -> device placement (rows at lut_row(ch), see LUT_ROW_PITCH)
        float dense[FOBS_CH * LUT_STRIDE];
        for (int k = 0; k < 8; ++k) {
            const bool original = (k & 4) != 0, raw = (k & 2) != 0, full = (k & 1) != 0;
            build_lut(cfg, full, dense, raw, original);
            for (int ch = 0; ch < lut_channels(full, original); ++ch)
                for (int i = 0; i < LUT_STRIDE; ++i) host_tab.lut[k][lut_row(ch) + i] = dense[ch * LUT_STRIDE + i];
        }
    }
    memcpy(host_tab.obstacles, cfg->obstacles, rc_cells);
    if (int rc = build_code_tables(cfg, &host_tab)) { delete h; return rc; }
    for (int a = 0; a < 16; ++a)
        for (int d = 0; d < 16; ++d) host_tab.combat[16 * a + d] = (uint8_t)combat_outcome(a, d);
    if (hipMalloc((void **)&h->boards, (size_t)n_envs * h->rec_bytes) != hipSuccess ||
        hipMalloc((void **)&h->tab, sizeof(DevTables)) != hipSuccess) {
        sgx_destroy(h);
        return fail(SGX_ENOMEM, "device allocation failed%s");
    }
#define HIP_TRY_OR_DESTROY(expr)                                                             \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) { sgx_destroy(h); return fail(SGX_EDEVICE, #expr ": %s", hipGetErrorString(e_)); } \
    } while (0)
    HIP_TRY_OR_DESTROY(hipMemset(h->boards, 0, (size_t)n_envs * h->rec_bytes));
    HIP_TRY_OR_DESTROY(hipMemcpy(h->tab, &host_tab, sizeof(DevTables), hipMemcpyHostToDevice));
#ifdef SGX_STAMPS
    HIP_TRY_OR_DESTROY(hipMalloc((void **)&h->stamps, (size_t)n_envs * 16 * sizeof(unsigned long long)));
    HIP_TRY_OR_DESTROY(hipMemset(h->stamps, 0, (size_t)n_envs * 16 * sizeof(unsigned long long)));
#endif
    init_scal_kernel<<<(unsigned)((n_envs + 255) / 256), 256>>>(h->boards, h->rec_bytes, h->sc_off, n_envs, cfg->max_turns);
    HIP_TRY_OR_DESTROY(hipGetLastError());
    HIP_TRY_OR_DESTROY(hipDeviceSynchronize());
#undef HIP_TRY_OR_DESTROY
    *out = h;
    return SGX_OK;
}

SGX_API int sgx_destroy(sgx_env *h) {
    if (!h) return SGX_OK;
    // teardown is best effort: there is nobody to report a failed free to
    DeviceGuard device_guard_(h->device);
    (void)hipDeviceSynchronize();
    if (h->boards) (void)hipFree(h->boards);
    if (h->tab) (void)hipFree(h->tab);
    if (h->setups) (void)hipFree(h->setups);
    if (h->pool) (void)hipFree(h->pool);
    if (h->stamps) (void)hipFree(h->stamps);
    for (int c = 0; c < SGX_MAX_CHAINS; ++c) {
        if (h->chain_stream[c]) (void)hipStreamDestroy(h->chain_stream[c]);
        if (h->chain_join[c]) (void)hipEventDestroy(h->chain_join[c]);
    }
    if (h->chain_fork) (void)hipEventDestroy(h->chain_fork);
    if (h->sync_flag_host) (void)hipHostFree(h->sync_flag_host);
    if (h->sync_count) (void)hipFree(h->sync_count);
    if (h->san_flags) (void)hipFree(h->san_flags);
    if (h->redo_list) (void)hipFree(h->redo_list);
    if (h->ring_tab_dev) (void)hipFree(h->ring_tab_dev);
    free(h->ring_tab_host);
    if (h->ring_tab_ev) (void)hipEventDestroy(h->ring_tab_ev);
    if (h->count_scratch) (void)hipFree(h->count_scratch);
    if (h->scan_sums) (void)hipFree(h->scan_sums);
    if (h->leaf_table) (void)hipFree(h->leaf_table);
    delete h;
    return SGX_OK;
}

SGX_API int sgx_set_nt_stores(sgx_env *h, int32_t mode) {
    if (!h || mode < -1 || mode > 1) return fail(SGX_EINVAL, "sgx_set_nt_stores: mode must be -1 (auto), 0 or 1%s");
    h->nt_mode = mode;
    return SGX_OK;
}

SGX_API int sgx_set_placement_target(sgx_env *h, float target_us) {
    if (!h || !(target_us >= 0.f)) return fail(SGX_EINVAL, "sgx_set_placement_target: target_us must be >= 0%s");
    h->placement_target_us = target_us;
    return SGX_OK;
}

SGX_API int sgx_set_general_states(sgx_env *h, int32_t mode) {
    if (!h || mode < 0 || mode > 1) return fail(SGX_EINVAL, "sgx_set_general_states: mode must be 0 or 1%s");
    h->general_states = mode;
    return SGX_OK;
}

SGX_API int sgx_last_launch_kind(const sgx_env *h) { return h ? h->last_kind : -1; }

SGX_API int sgx_set_multi_step(sgx_env *h, int32_t mode) {
    if (!h || mode < 0 || mode > 1) return fail(SGX_EINVAL, "sgx_set_multi_step: mode must be 0 or 1%s");
    h->no_multi_step = mode ? 0 : 1;
    return SGX_OK;
}

SGX_API int sgx_set_half_wave(sgx_env *h, int32_t mode) {
    if (!h || mode < 0 || mode > 1) return fail(SGX_EINVAL, "sgx_set_half_wave: mode must be 0 or 1%s");
    h->half_wave = mode;
    return SGX_OK;
}

SGX_API int sgx_set_steps_barrier(sgx_env *h, int32_t mode) {
    if (!h || mode < -1 || mode > 1) return fail(SGX_EINVAL, "sgx_set_steps_barrier: mode must be -1 (auto), 0 or 1%s");
    h->steps_barrier = mode;
    return SGX_OK;
}

SGX_API int sgx_set_lane_kernel(sgx_env *h, int32_t mode) {
    if (!h || mode < -1 || mode > 1) return fail(SGX_EINVAL, "sgx_set_lane_kernel: mode must be -1 (auto), 0 or 1%s");
    h->lane_mode = mode;
    return SGX_OK;
}

static void launch_shares(const sgx_env *h, bool streaming, int32_t *w);

SGX_API int sgx_set_xcd_skew(sgx_env *h, int32_t per_mille) {
    if (!h || per_mille < -1 || per_mille > 900) return fail(SGX_EINVAL, "sgx_set_xcd_skew: -1 (auto) or 0 .. 900 per mille%s");
    h->xcd_skew = per_mille;
    h->xcd_explicit = 0;
    return SGX_OK;
}

SGX_API int sgx_set_xcd_shares(sgx_env *h, const int32_t *per_mille) {
    if (!h) return fail(SGX_EINVAL, "handle is NULL%s");
    if (!per_mille) { h->xcd_explicit = 0; return SGX_OK; }
    for (int x = 0; x < 8; ++x)
        if (per_mille[x] < 1 || per_mille[x] > 8000) return fail(SGX_EINVAL, "sgx_set_xcd_shares: every share must be 1 .. 8000 per mille%s");
    for (int x = 0; x < 8; ++x) h->xcd_w[x] = per_mille[x];
    h->xcd_explicit = 1;
    return SGX_OK;
}

SGX_API int sgx_get_xcd_shares(sgx_env *h, int32_t *per_mille, int32_t *calibrated) {
    if (!h || !per_mille) return fail(SGX_EINVAL, "NULL argument%s");
    launch_shares(h, true, per_mille);
    if (calibrated) *calibrated = h->xcd_explicit;
    return SGX_OK;
}

SGX_API int sgx_set_setup_table(sgx_env *h, const uint8_t *table_host, int64_t n_setups) {
    if (!h || !table_host || n_setups <= 0 || n_setups > 0x7fffffff) return fail(SGX_EINVAL, "bad setup table%s");
    SGX_ON_DEVICE(h->device);
    const size_t bytes = (size_t)n_setups * h->cfg.usable_rows * h->cfg.cols;
    for (size_t i = 0; i < bytes; ++i)
        if (table_host[i] > 12) return fail(SGX_EINVAL, "setup table holds a piece code > 12%s");
    if (h->setups) { HIP_TRY(hipFree(h->setups)); h->setups = nullptr; }
    HIP_TRY(hipMalloc((void **)&h->setups, bytes));
    HIP_TRY(hipMemcpy(h->setups, table_host, bytes, hipMemcpyHostToDevice));
    h->n_setups = n_setups;
    return SGX_OK;
}

namespace { int same_variant(const sgx_env *a, const sgx_env *b); }
static int check_aligned(const char *fn, const char *name, const void *ptr, int align);

SGX_API int sgx_set_start_pool(sgx_env *h, sgx_env *pool, int64_t n_pool, int32_t flags) {
    if (!h) return fail(SGX_EINVAL, "sgx_set_start_pool: handle is NULL%s");
    if (!pool) {                                             // clear: games start from sampled setups again
        if (!h->pool) return SGX_OK;
        SGX_ON_DEVICE(h->device);
        HIP_TRY(hipDeviceSynchronize());                     // (no launch that reads the buffer is in flight when it goes)
        HIP_TRY(hipFree(h->pool));
        h->pool = nullptr; h->n_pool = 0; h->pool_flags = 0;
        return SGX_OK;
    }
    if (flags & ~(SGX_POOL_RANDOM_FIRST_PLAYER | SGX_POOL_RESTART_CLOCK)) return fail(SGX_EINVAL, "sgx_set_start_pool: unknown flag%s");
    if (pool->cfg.rows != h->cfg.rows || pool->cfg.cols != h->cfg.cols) return fail(SGX_EINVAL, "sgx_set_start_pool: the pool was created for another board size%s");
    if (int rc = same_variant(h, pool)) return rc;
    if (n_pool < 1 || n_pool > pool->n_envs || n_pool > 0x7fffffff) {
        char buf[160];
        snprintf(buf, sizeof(buf), "sgx_set_start_pool: n_pool = %lld, the pool handle holds %lld records", (long long)n_pool, (long long)pool->n_envs);
        return fail(SGX_EINVAL, "%s", buf);
    }
    SGX_ON_DEVICE(h->device);
    HIP_TRY(hipDeviceSynchronize());                         // the pool's records are complete; nothing reads the previous buffer any more
    // the records' scalars on the host: no finished game may be a start state, and SGX_POOL_RESTART_CLOCK is applied here, once
    std::vector<int32_t> sc((size_t)n_pool * 8);
    HIP_TRY(hipMemcpy2D(sc.data(), 32, pool->boards + pool->sc_off, (size_t)pool->rec_bytes, 32, (size_t)n_pool, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_pool; ++i)
        if (sc[8 * i + 1] & F_OVER) {
            char buf[160];
            snprintf(buf, sizeof(buf), "sgx_set_start_pool: the game of pool record %lld is over (a start state must have a next move)", (long long)i);
            return fail(SGX_EINVAL, "%s", buf);
        }
    int8_t *buf_dev = nullptr;
    const size_t bytes = (size_t)n_pool * h->rec_bytes;
    if (hipMalloc((void **)&buf_dev, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(SGX_ENOMEM, "sgx_set_start_pool: device allocation failed%s"); }
    hipError_t e = hipMemcpy(buf_dev, pool->boards, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && (flags & SGX_POOL_RESTART_CLOCK)) {                   // util.py:382-383: turn 0, the handle's max_turns
        for (int64_t i = 0; i < n_pool; ++i) { sc[8 * i] = 0; sc[8 * i + 2] = h->cfg.max_turns; }
        e = hipMemcpy2D(buf_dev + h->sc_off, (size_t)h->rec_bytes, sc.data(), 32, 32, (size_t)n_pool, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(buf_dev); return fail(SGX_EDEVICE, "sgx_set_start_pool: %s", hipGetErrorString(e)); }
    if (h->pool) (void)hipFree(h->pool);                     // (the device is idle: see above)
    h->pool = buf_dev;
    h->n_pool = n_pool;
    h->pool_flags = flags & SGX_POOL_RANDOM_FIRST_PLAYER;
    return SGX_OK;
}

SGX_API int sgx_set_leaf_values(sgx_env *h, const int16_t *table_host, int32_t limit, int32_t denom, int32_t flags) {
    if (!h) return fail(SGX_EINVAL, "sgx_set_leaf_values: handle is NULL%s");
    if (!table_host) {                                       // clear: positions that are not over report 0, 0 again
        if (!h->leaf_table) return SGX_OK;
        SGX_ON_DEVICE(h->device);
        HIP_TRY(hipDeviceSynchronize());                     // (no launch that reads the buffer is in flight when it goes)
        HIP_TRY(hipFree(h->leaf_table));
        h->leaf_table = nullptr; h->leaf_limit = h->leaf_denom = h->leaf_see_all = 0;
        return SGX_OK;
    }
    if (denom < 1 || denom > (1 << 24) || limit < 1 || limit > denom)
        return fail(SGX_EINVAL, "%s", ("sgx_set_leaf_values: 1 <= limit <= denom <= 2^24 is required (got limit = " + std::to_string(limit) + ", denom = " + std::to_string(denom) + ")").c_str());
    if (flags & ~SGX_LEAF_SEE_ALL) return fail(SGX_EINVAL, "sgx_set_leaf_values: unknown flag bits%s");
    SGX_ON_DEVICE(h->device);
    const size_t cells = (size_t)h->cfg.rows * h->cfg.cols;
    std::vector<int16_t> rows((size_t)LEAF_ROWS * cells, 0);
    memcpy(rows.data(), table_host, 2 * LEAF_HALF * cells * sizeof(int16_t));
    int16_t *buf_dev = nullptr;
    if (hipMalloc((void **)&buf_dev, rows.size() * sizeof(int16_t)) != hipSuccess) { (void)hipGetLastError(); return fail(SGX_ENOMEM, "sgx_set_leaf_values: device allocation failed%s"); }
    hipError_t e = hipMemcpy(buf_dev, rows.data(), rows.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();         // the launches in flight have finished with the old table: it goes only now
    if (e != hipSuccess) { (void)hipFree(buf_dev); return fail(SGX_EDEVICE, "sgx_set_leaf_values: %s", hipGetErrorString(e)); }
    if (h->leaf_table) (void)hipFree(h->leaf_table);
    h->leaf_table = buf_dev;
    h->leaf_limit = limit; h->leaf_denom = denom; h->leaf_see_all = (flags & SGX_LEAF_SEE_ALL) ? 1 : 0;
    return SGX_OK;
}

SGX_API int sgx_leaf_values_set(const sgx_env *h) { return (h && h->leaf_table) ? 1 : 0; }

SGX_API int sgx_set_replay_origins(sgx_env *h, const int16_t *origin_in_dev, int16_t *origin_out_dev) {
    // the pointers first: what can be said about them needs no handle
    if (int rc = check_aligned("sgx_set_replay_origins", "origin_out_dev", origin_out_dev, 4)) return rc;
    if (origin_out_dev)
        if (int rc = check_aligned("sgx_set_replay_origins", "origin_in_dev", origin_in_dev, 4)) return rc;
    if (!h) return fail(SGX_EINVAL, "sgx_set_replay_origins: handle is NULL%s");
    if (!origin_out_dev) { h->origin_in = nullptr; h->origin_out = nullptr; return SGX_OK; }      // clear (origin_in_dev is ignored)
    h->origin_in = origin_in_dev;
    h->origin_out = origin_out_dev;
    return SGX_OK;
}

SGX_API int sgx_replay_origins_set(const sgx_env *h) { return (h && h->origin_out) ? 1 : 0; }

SGX_API int sgx_set_start_index_out(sgx_env *h, int32_t *start_index_dev) {
    if (!h) return fail(SGX_EINVAL, "sgx_set_start_index_out: handle is NULL%s");
    if (int rc = check_aligned("sgx_set_start_index_out", "start_index_dev", start_index_dev, 4)) return rc;
    h->start_index = start_index_dev;
    return SGX_OK;
}

SGX_API int64_t sgx_start_pool_size(const sgx_env *h) { return (h && h->pool) ? h->n_pool : 0; }

SGX_API int sgx_reset(sgx_env *h, const uint8_t *env_select_dev, const int8_t *p1_maps_dev, const int8_t *p2_maps_dev, void *stream) {
    if (!h) return fail(SGX_EINVAL, "handle is NULL%s");
    if ((p1_maps_dev == nullptr) != (p2_maps_dev == nullptr)) return fail(SGX_EINVAL, "pass both piece maps or neither%s");
    if (!p1_maps_dev)
        if (int rc = check_random_setups(h)) return rc;
    SGX_ON_DEVICE(h->device);
    if (h->pool) {
        const KParams p = make_params(h);
        const PoolParams pp = make_pool_params(h);
        const unsigned grid = (unsigned)h->n_envs;
        if (!p1_maps_dev) {         // every selected env starts from a record of the start pool
            reset_pool_kernel<<<grid, 64, 0, (hipStream_t)stream>>>(p, pp, env_select_dev, h->sc_off);
            HIP_TRY(hipGetLastError());
            return SGX_OK;
        }
        if (pp.start_index) {       // explicit maps win over the pool: such a game has no pool index
            start_index_none_kernel<<<(grid + 255) / 256, 256, 0, (hipStream_t)stream>>>(pp.start_index, env_select_dev, h->n_envs);
            HIP_TRY(hipGetLastError());
        }
    }
    ResetParams rp;
    rp.k = make_params(h);
    rp.select = env_select_dev;
    rp.p1_maps = p1_maps_dev;
    rp.p2_maps = p2_maps_dev;
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            reset_kernel<decltype(r)::value, decltype(c)::value><<<(unsigned)h->n_envs, 64, 0, (hipStream_t)stream>>>(rp);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

// Beyond what the 256 MiB Infinity Cache absorbs a launch's kernels use non-temporal stores for the lines a wave writes whole (measured
// crossover between 281 and 316 MB on four board sizes, sgx_obs.h).  What has to fit is what is written between two writes of one line:
// the whole launch (x its output sets) for a per-step launch -- this rule; only what the RESIDENT games write for a multi-step launch of
// steps_kernel, whose waves keep their games (steps_policy below).  Both rules and their constants (SGX_CACHE_FIT_BYTES,
// SGX_PLAIN_BUDGET_BYTES): sgx_store_policy.h.
static bool past_cache(int64_t bytes) { return !sgx_store_fits_launch(bytes); }
// non-temporal stores for a launch that writes `bytes`: sgx_set_nt_stores, else SGX_NT_PLAIN_LINES, else by the size.  A forced count
// comes with non-temporal stores for EVERY launch of the handle, whatever its size and kernel (lane kernels, states_kernel, small per-step
// launches that the size rule would store plain): it is a knob for tests and sweeps of the split, not an override of the split alone, and
// not a way to tune one ring in production.
static int nt_for(const sgx_env *h, int64_t bytes) { return h->nt_mode >= 0 ? h->nt_mode : h->plain_lines_forced >= 0 ? 1 : (past_cache(bytes) ? 1 : 0); }

// float32 observation bytes one launch writes
static int64_t launch_obs_bytes(const sgx_env *h, const KParams &p) {
    const bool original = (p.io.flags & SGX_STEP_ORIGINAL_CHANNELS) != 0;
    const int64_t cells = (int64_t)h->cfg.rows * h->cfg.cols;
    int64_t bytes = 0;
    if (p.io.obs_dev) bytes += h->n_envs * cells * lut_channels(false, original) * 4;
    if (p.io.fobs_dev) bytes += h->n_envs * cells * lut_channels(true, original) * 4;
    return bytes;
}

// Workgroup-groups per XCD for `groups` groups of games from the shares w[8] (per mille of the mean share): KParams::xcd_first /
// xcd_count; returns the grid size (8 x the largest share).
#define SGX_XCD_SKEW_DEFAULT 100
static unsigned shares_for(KParams &p, int64_t groups, const int32_t *w) {
    int64_t sum = 0, cnt[8], given = 0;
    for (int x = 0; x < 8; ++x) sum += w[x];
    for (int x = 0; x < 8; ++x) { cnt[x] = groups * w[x] / sum; given += cnt[x]; }
    for (int x = 0; given < groups; x = (x + 1) & 7) { cnt[x] += 1; given += 1; }          // the remainder, one group each
    int64_t at = 0, mx = 1;
    for (int x = 0; x < 8; ++x) {
        p.xcd_first[x] = (int32_t)at;
        p.xcd_count[x] = (int32_t)cnt[x];
        at += cnt[x];
        if (cnt[x] > mx) mx = cnt[x];
    }
    return (unsigned)(8 * mx);
}
// the shares of a launch: explicit ones, else the odd-even skew where the launch is a saturating write stream
static void launch_shares(const sgx_env *h, bool streaming, int32_t *w) {
    if (h->xcd_explicit) { for (int x = 0; x < 8; ++x) w[x] = h->xcd_w[x]; return; }
    // measured in one process on one set of buffers (tools/skew_ab.py, profiles/r03_skew_ab.log): 10x10 -3 ... -5 %, 8x8 -5 %; 6x6,
    // 15x15 and Micro, where the game logic shares the critical path, +3 ... +7 %
    const int cells = h->cfg.rows * h->cfg.cols;
    const int skew = h->xcd_skew < 0 ? ((streaming && cells >= 64 && cells <= 100) ? SGX_XCD_SKEW_DEFAULT : 0) : h->xcd_skew;
    for (int x = 0; x < 8; ++x) w[x] = (x & 1) ? 1000 - skew : 1000 + skew;
}

// What every step launch takes from the handle: the SGX_MAP experiment, non-temporal stores and the XCD shares w.  `sets`: output sets
// written round-robin (sgx_step_ring): a line is written again only after `sets` launches, so what has to fit the cache for plain stores
// to pay is the observations of all of them.
static void launch_setup(const sgx_env *h, KParams &p, int sets, int32_t *w) {
    p.map_mode = h->map_mode; p.map_arg = h->map_arg;
    const int64_t bytes = launch_obs_bytes(h, p) * sets;
    p.nt_stores = nt_for(h, bytes);
    // sgx_set_nt_stores(1) keeps its meaning (every whole line non-temporal); the multi-step launches of steps_kernel get their own
    // count from steps_policy
    p.plain_lines = (int16_t)((h->nt_mode < 0 && h->plain_lines_forced >= 0) ? h->plain_lines_forced : 0);
    launch_shares(h, past_cache(bytes), w);                   // unequal XCD shares (sgx_layout.h: group_of_block)
}
// the grid of a launch that plays `games` games per workgroup (Geo::WPB x Geo::GPW, the lane kernels' 64) over the envs [env_first, n_envs)
static unsigned grid_for(KParams &p, int64_t games, const int32_t *w) { return shares_for(p, (p.n_envs - p.env_first + games - 1) / games, w); }
template <class G>
unsigned geo_grid(KParams &p, const int32_t *w) { return grid_for(p, G::WPB * G::GPW, w); }

// The variant of a wave-per-game launch of observation kind KIND: two games per wave (Geo<R, C, 2>) for the launches without an observation
// on the boards that allow it (half_wave_ok) unless sgx_set_half_wave / SGX_HALF_WAVE switched it off, else one.  Calls f(int_c<VAR>).
template <int R, int C, int KIND, class F>
void with_half_wave(const sgx_env *h, F &&f) {
    if constexpr (KIND == 8 && half_wave_ok<R, C>())
        if (h->half_wave) return f(int_c<2>());
    f(int_c<0>());
}

// The lane-per-game kernel plays this launch?  (sgx_lane_kernel.h: what it covers; everything else is the wave-per-game kernel.)
static bool lane_eligible(const sgx_env *h, const KParams &p, bool full, bool original, bool multi_step = false) {
    const int cells = h->cfg.rows * h->cfg.cols;
    auto aligned = [](const void *ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; };
    // -1 (auto): only where it is the faster kernel -- launches that emit no observation (2 x on Micro / Tiny, docs/DESIGN_rounds_4-5.md section 3.3) and
    // the fused multi-step launches of sgx_step_n / sgx_step_ring (lane_steps_kernel: the logic of step t + 1 under the stores of step t)
    if (h->lane_mode < 0 && p.io.obs_dev && !multi_step) return false;
    return h->lane_mode != 0 && !p.multi_ev && !(p.io.flags & (SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK)) && cells <= 16 && cells % 4 == 0 && !full && !original && h->map_mode == 0 &&
           !(p.io.flags & (SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS)) && !p.src_boards && !p.io.final_obs_dev && !p.io.final_fobs_dev &&
           (h->rec_bytes == 128 || h->rec_bytes == 256) && (p.env_first & 63) == 0 &&
           aligned(p.io.obs_dev, 16) && aligned(p.io.mask_dev, 16) && aligned(p.io.reward_dev, 8) && aligned(p.io.actions_dev, 16);
}

static int check_step_io(sgx_env *h, const KParams &p) {
    if (p.mode == 0 && p.io.auto_reset) return check_random_setups(h);
    return SGX_OK;
}

// The pointer contract of include/stratego_mi355x.h ("Alignment of device pointers"), checked by every entry point BEFORE it launches
// anything: a pointer the kernels' stores cannot take is SGX_EINVAL with its name and the alignment it needs, never a launch.
static int check_aligned(const char *fn, const char *name, const void *ptr, int align) {
    if ((reinterpret_cast<uintptr_t>(ptr) & (uintptr_t)(align - 1)) == 0) return SGX_OK;       // (NULL passes: nullable or refused elsewhere)
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: %s must be %d-byte aligned", fn, name, align);
    return fail(SGX_EINVAL, "%s", buf);
}
// Every *_dev member of sgx_step_io (tests/test_cabi_cpu.py holds this table against the struct and the header's contract).  Observations
// leave as 16-byte stores on boards whose cell count is a multiple of 4 (emit_codes / emit_obs_lut / patch_uncoded: f32x4 at dst + 16 q), as
// dwords at the edges of a game on the others; compact outputs are int4 copies; position actions are one int4 load per game; the byte
// outputs are written byte by byte wherever a dword would not be the caller's (emit_mask, emit_mask_mapped).
static int check_io_pointers(const sgx_env *h, const sgx_step_io &io, const char *fn) {
    const int quad = (h->cfg.rows * h->cfg.cols) % 4 == 0 ? 16 : 4;
    const struct { const char *name; const void *ptr; int align; } tab[] = {
        {"actions_dev", io.actions_dev, (io.flags & SGX_STEP_ACTIONS_POSITIONS) ? 16 : 4},
        {"obs_dev", io.obs_dev, (io.flags & SGX_STEP_COMPACT_OBS) ? 16 : quad},
        {"fobs_dev", io.fobs_dev, quad},
        {"mask_dev", io.mask_dev, (io.flags & SGX_STEP_COMPACT_MASK) ? 16 : 1},
        {"reward_dev", io.reward_dev, 4},
        {"done_dev", io.done_dev, 1},
        {"player_dev", io.player_dev, 1},
        {"invalid_action_dev", io.invalid_action_dev, 1},
        {"ending_invalid_dev", io.ending_invalid_dev, 1},
        {"final_obs_dev", io.final_obs_dev, quad},
        {"final_fobs_dev", io.final_fobs_dev, quad},
        {"next_actions_dev", io.next_actions_dev, 4},
    };
    for (const auto &e : tab)
        if (int rc = check_aligned(fn, e.name, e.ptr, e.align)) return rc;
    return SGX_OK;
}

// The output sets of a rollout call: sgx_step_n (one set, in place), sgx_step_ring (n_sets separate sets: ios[0 .. n_sets)), or the slots of
// an sgx_step_traj trajectory buffer (strided: ios[0] names slot 0, slot s lies s x the byte strides further; KParams::traj_* carry the
// strides of the per-step results and of the action log).
struct OutSets {
    const sgx_step_io *ios;
    int32_t n_sets;
    bool strided;
    int64_t obs_b, fobs_b, mask_b;
};

static int launch_step(sgx_env *h, const KParams &p_in, void *stream, int ring_sets = 1, int64_t start_index_off = 0, bool allow_pool = true);

// The stream of an INNER launch of a call that is more than one launch.  Always the caller's -- except in the test-the-tests build
// -DSGX_MUTANT_NULL_STREAM (tools/mutant_check.sh, off in every shipped build), where the scan of sgx_count_moves' block sums and the
// action-log copy of a single trajectory step go to the NULL stream: tests/test_gpu_streams.py has to notice.
#ifdef SGX_MUTANT_NULL_STREAM
#define SGX_INNER_STREAM(stream) ((hipStream_t) nullptr)
#else
#define SGX_INNER_STREAM(stream) ((hipStream_t)(stream))
#endif

// ONE step of a rollout call as a launch of its own, writing output set / slot `set`: what the multi-step launches fall back to (calls
// they do not cover, the odd step a chunk leaves over).
static int launch_set_step(sgx_env *h, const KParams &p_in, const OutSets &sets, int32_t set, void *stream) {
    KParams p1 = p_in;
    p1.mode = 0;
    if (!sets.strided) {
        p1.io = sets.ios[set];
        return launch_step(h, p1, stream, sets.n_sets);
    }
    sgx_step_io io = sets.ios[0];
    auto at = [](auto *ptr, int64_t bytes) { return ptr ? reinterpret_cast<decltype(ptr)>(reinterpret_cast<char *>(ptr) + bytes) : ptr; };
    io.obs_dev = at(io.obs_dev, set * sets.obs_b);
    io.fobs_dev = at(io.fobs_dev, set * sets.fobs_b);
    io.mask_dev = at(io.mask_dev, set * sets.mask_b);
    const int64_t r = set * p_in.traj_res_envs;
    io.reward_dev = at(io.reward_dev, 8 * r);
    io.done_dev = at(io.done_dev, r);
    io.player_dev = at(io.player_dev, r);
    io.invalid_action_dev = at(io.invalid_action_dev, r);
    io.ending_invalid_dev = at(io.ending_invalid_dev, r);
    p1.io = io;
    if (int rc = launch_step(h, p1, stream, sets.n_sets, r)) return rc;        // (r: start_index moves on like the results)
    if (p_in.traj_act_log && io.next_actions_dev)
        HIP_TRY(hipMemcpyAsync(p_in.traj_act_log + set * p_in.traj_out_envs, io.next_actions_dev, (size_t)h->n_envs * sizeof(int32_t), hipMemcpyDeviceToDevice,
                               SGX_INNER_STREAM(stream)));
    return SGX_OK;
}

// More separate output sets than the kernel arguments hold (sgx_step_ring with n_sets > 8, e.g. a ring of 64 sets that each came from its own
// placement search): the pointers of the sets go into a device table -- [obs x n][fobs x n][mask x n] -- that the multi-step kernels read with
// scalar loads.  Written only when the ring changed, by launches on `stream` that carry the pointers in their own arguments: the host never
// waits, whatever the stream still holds.  The table is one per handle and streams may alternate on it: ring_tab_ev orders every upload
// behind the launches that still read the previous table, and every reader behind the upload (ring_table_done records it).
#define SGX_RING_TAB_CHUNK 32
struct RingTabChunk { void *ptr[SGX_RING_TAB_CHUNK]; };
__global__ void ring_table_kernel(void **__restrict__ tab, const RingTabChunk chunk, const int n) {
    const int i = (int)threadIdx.x;
    if (i < n) tab[i] = chunk.ptr[i];
}

static int upload_ring_table(sgx_env *h, const OutSets &sets, hipStream_t stream, void ***tab_out) {
    const int n = sets.n_sets;
    if (n > h->ring_tab_cap) {                                 // (growth: hipFree waits for the launches that still read the old table)
        void **host = (void **)malloc((size_t)3 * n * sizeof(void *));
        if (!host) return fail(SGX_ENOMEM, "sgx_step_ring: host allocation failed (ring table)%s");
        if (h->ring_tab_dev) HIP_TRY(hipFree(h->ring_tab_dev));
        free(h->ring_tab_host);
        h->ring_tab_dev = nullptr;
        h->ring_tab_host = host;
        h->ring_tab_cap = h->ring_tab_n = 0;
        HIP_TRY(hipMalloc((void **)&h->ring_tab_dev, (size_t)3 * n * sizeof(void *)));
        h->ring_tab_cap = n;
    }
    if (!h->ring_tab_ev) {
        HIP_TRY(hipEventCreateWithFlags(&h->ring_tab_ev, hipEventDisableTiming));
        h->ring_tab_stream = stream;                           // (nothing recorded yet: nothing to wait for)
    }
    // what other streams did with the table so far -- uploads and reads -- comes first
    if (h->ring_tab_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, h->ring_tab_ev, 0));
    std::vector<void *> want((size_t)3 * n);
    for (int k = 0; k < n; ++k) {
        want[k] = sets.ios[k].obs_dev;
        want[n + k] = sets.ios[k].fobs_dev;
        want[2 * n + k] = sets.ios[k].mask_dev;
    }
    const bool same = h->ring_tab_n == n && memcmp(h->ring_tab_host, want.data(), want.size() * sizeof(void *)) == 0;
    if (!same) {
        // (laid out for n sets: a smaller ring after a larger one re-packs the three sections)
        for (size_t at = 0; at < want.size(); at += SGX_RING_TAB_CHUNK) {
            RingTabChunk chunk;
            const int now = (int)(want.size() - at < SGX_RING_TAB_CHUNK ? want.size() - at : SGX_RING_TAB_CHUNK);
            memset(&chunk, 0, sizeof(chunk));
            memcpy(chunk.ptr, want.data() + at, (size_t)now * sizeof(void *));
            ring_table_kernel<<<1, 64, 0, stream>>>(h->ring_tab_dev + at, chunk, now);
        }
        HIP_TRY(hipGetLastError());
        memcpy(h->ring_tab_host, want.data(), want.size() * sizeof(void *));
        h->ring_tab_n = n;
        HIP_TRY(hipEventRecord(h->ring_tab_ev, stream));       // (should the launch behind it never come, readers elsewhere still find the upload)
        h->ring_tab_stream = stream;
    }
    *tab_out = h->ring_tab_dev;
    return SGX_OK;
}

// Behind the launches that read the ring table: the next upload, from any stream, waits for them.
static int ring_table_done(sgx_env *h, hipStream_t stream) {
    HIP_TRY(hipEventRecord(h->ring_tab_ev, stream));
    h->ring_tab_stream = stream;
    return SGX_OK;
}

// A rollout call goes out in launches of at most SGX_STEPS_MAX_PER_LAUNCH steps (a workgroup should not own the chip for seconds: work on
// other streams, or a second rank sharing the GPU, gets in between the launches).
#define SGX_STEPS_MAX_PER_LAUNCH 256

// sgx_step_n / sgx_step_ring / sgx_step_traj on boards of at most 16 cells: the steps in launches of lane_steps_kernel (sgx_lane_kernel.h)
// where the call is eligible -- the lane kernel's conditions for every output set, flat perspective actions, observations wanted.
// (p.io: the outputs of the call's first set.)
static bool lane_steps_ok(const sgx_env *h, const KParams &p, const OutSets &sets) {
    if (h->lane_mode == 0 || !p.io.obs_dev || (p.io.flags & (SGX_STEP_ACTIONS_1D | SGX_STEP_ACTIONS_POSITIONS))) return false;
    if (sets.strided) {
        const bool full = p.io.fobs_dev || p.io.final_fobs_dev, original = (p.io.flags & SGX_STEP_ORIGINAL_CHANNELS) != 0;
        // every slot as aligned as slot 0 (the kernel's 16-byte stores), per-slot results as aligned as the results of slot 0
        return lane_eligible(h, p, full, original, true) && !((sets.obs_b | sets.mask_b) & 15) && !(p.traj_res_envs & 1);
    }
    for (int32_t k = 0; k < sets.n_sets; ++k) {
        KParams pk = p;
        pk.io = sets.ios[k];
        const bool full = pk.io.fobs_dev || pk.io.final_fobs_dev, original = (pk.io.flags & SGX_STEP_ORIGINAL_CHANNELS) != 0;
        if (!pk.io.obs_dev || !lane_eligible(h, pk, full, original, true)) return false;
    }
    return true;
}

// The same for the wave-per-game kernels (steps_kernel, sgx_step.h): the steps of an sgx_step_n / sgx_step_ring / sgx_step_traj call in launches
// of up to 256 steps -- the games' boards stay in LDS, the record travels once per launch, the waves drift out of phase -- for the 67-channel
// 'extended' kind, BOTH observations, compact outputs and launches without an observation; perspective actions and masks; any number of
// separate output sets, or any number of slots of a trajectory buffer.
static bool wave_steps_ok(const sgx_env *h, const KParams &p, const OutSets &sets) {
    const sgx_step_io &io0 = p.io;
    if (!h->multi_step_wave || h->map_mode != 0) return false;
    if (io0.flags & (SGX_STEP_ACTIONS_1D | SGX_STEP_ACTIONS_POSITIONS | SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS | SGX_STEP_ORIGINAL_CHANNELS)) return false;
    const bool compact = (io0.flags & (SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK)) != 0;
    const bool full = io0.fobs_dev || io0.final_fobs_dev;
    const bool no_obs = !io0.obs_dev && !io0.fobs_dev && !io0.final_obs_dev && !io0.final_fobs_dev && !compact;
    auto misaligned = [](const sgx_step_io &io) { return ((reinterpret_cast<uintptr_t>(io.obs_dev) | reinterpret_cast<uintptr_t>(io.mask_dev)) & 15) != 0; };
    if (compact && (full || io0.final_obs_dev)) return false;             // (launch_step refuses these: let it say so)
    if (compact && misaligned(io0)) return false;
    // Logic-only rollouts (no observation pointer) on 3x4: the lane-per-game kernel, one launch per step, stays ahead of this kernel's multi-step
    // launch there -- 65,536 Micro games mask only 14.9 against 18.2 us per step, no outputs 13.4 against 15.7; 262,144 games 44 against 65 --
    // while on 4x4 the multi-step launch wins (Tiny 15.0 against 17.5 us, 262,144 games 56 against 74: tools/noobs_small_ab.py,
    // profiles/r06_noobs_small_ab.log)
    if (no_obs && h->cfg.rows * h->cfg.cols <= 12 && lane_eligible(h, p, false, false)) return false;
    if (sets.strided) return !(compact && ((sets.obs_b | sets.mask_b) & 15));
    for (int32_t k = 0; k < sets.n_sets; ++k) {
        const sgx_step_io &io = sets.ios[k];
        // every set has the tensors the first one has
        if (io.final_obs_dev != io0.final_obs_dev || io.final_fobs_dev != io0.final_fobs_dev || (io.obs_dev == nullptr) != (io0.obs_dev == nullptr) ||
            (io.fobs_dev == nullptr) != (io0.fobs_dev == nullptr) || (io.mask_dev == nullptr) != (io0.mask_dev == nullptr)) return false;
        if (compact && misaligned(io)) return false;
    }
    return true;
}

// Separate output sets differ in their observation / mask tensors only: the multi-step kernels write the per-step results through the first
// set's pointers.
static bool sets_share_results(const OutSets &sets, const sgx_step_io &io0) {
    if (sets.strided) return true;
    for (int32_t k = 0; k < sets.n_sets; ++k) {
        const sgx_step_io &io = sets.ios[k];
        if (io.reward_dev != io0.reward_dev || io.done_dev != io0.done_dev || io.player_dev != io0.player_dev || io.invalid_action_dev != io0.invalid_action_dev ||
            io.ending_invalid_dev != io0.ending_invalid_dev) return false;
    }
    return true;
}

// One launch of lane_steps_kernel: sp.n_steps steps from set sp.first_set.  *ok = false: this runtime keeps workgroups to 64 KiB of LDS
// (nothing was launched; the handle plays per-step launches from now on).
static int steps_launch(sgx_env *h, StepsParams &sp, KParams &p, const int32_t *w, hipStream_t stream, bool *ok) {
    *ok = false;
    return for_geometry(h, [&](auto r, auto c) {
        constexpr int R = decltype(r)::value, C = decltype(c)::value;
        if constexpr (lane_geometry<Geo<R, C>>()) {
            const unsigned grid = grid_for(p, 64, w);
            const size_t dyn = 2 * 64 * (size_t)(p.rec_bytes + 16);
            // more than 64 KiB of LDS per workgroup has to be asked for, once per kernel symbol (`done`: the handle's note that it was)
            auto raise_lds = [&](const void *kernel, int &done) {
                if (dyn + sizeof(StepsLds<Geo<R, C>>) <= 64 * 1024 || done) return true;
                if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) {
                    (void)hipGetLastError();
                    h->no_multi_step = 1;
                    return false;
                }
                done = 1;
                return true;
            };
            if (!raise_lds(reinterpret_cast<const void *>(&lane_steps_kernel<R, C>), h->multi_step_attr)) return;
            sp.k = p;
            if (h->pool) {
                if (!raise_lds(reinterpret_cast<const void *>(&lane_steps_kernel_pool<R, C>), h->multi_step_attr_pool)) return;
                lane_steps_kernel_pool<R, C><<<grid, 64 * (1 + KSTEP_EMITTERS), dyn, stream>>>(sp, make_pool_params(h));
            } else
                lane_steps_kernel<R, C><<<grid, 64 * (1 + KSTEP_EMITTERS), dyn, stream>>>(sp);
            *ok = true;
        }
    });
}

// The store policy of a multi-step launch of steps_kernel<R, C, KIND> (4-aligned boards, float32 observations) where the launch's own size
// asks for non-temporal stores and nothing is forced: by what the RESIDENT games rewrite (sgx_store_policy.h).  The resident workgroups per
// CU come from the occupancy query, asked once per kernel and handle.
template <int R, int C, int KIND>
static int steps_policy(sgx_env *h, KParams &p, int32_t n_sets) {
    if (h->nt_mode >= 0 || h->plain_lines_forced >= 0 || !p.nt_stores || (p.io.flags & SGX_STEP_ORIGINAL_CHANNELS)) return SGX_OK;
    using G = Geo<R, C, 0>;
    const int pool = h->pool ? 1 : 0;
    if (!h->cus) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        h->cus = cus;
    }
    if (!h->steps_wg_per_cu[KIND][pool]) {
        int wgs = 0;
        if (pool) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, steps_kernel_pool<R, C, KIND, 0>, 64 * G::WPB, 0));
        else HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, steps_kernel<R, C, KIND, 0>, 64 * G::WPB, 0));
        h->steps_wg_per_cu[KIND][pool] = wgs > 0 ? wgs : 1;
    }
    const int64_t cells = (int64_t)R * C;
    sgx_store_shape s;
    s.cus = h->cus; s.wg_per_cu = h->steps_wg_per_cu[KIND][pool]; s.games_per_wg = G::WPB * G::GPW;
    s.games = p.n_envs - p.env_first; s.sets = n_sets;
    s.obs_bytes = p.io.obs_dev ? cells * lut_channels(false, false) * 4 : 0;
    s.fobs_bytes = p.io.fobs_dev ? cells * lut_channels(true, false) * 4 : 0;
    s.mask_bytes = p.io.mask_dev ? cells * h->K : 0;
    // BOTH mode (kind 1): all plain where the rewrite set fits, no share otherwise -- its kernels do not read a count (sgx_step.h)
    s.budget = SGX_PLAIN_BUDGET_BYTES; s.split = KIND == 0 ? SGX_STORE_SPLIT_DEFAULT : 0;
    const sgx_store_policy pol = sgx_store_policy_multi_step(&s);
    p.nt_stores = pol.nt_stores; p.plain_lines = (int16_t)(KIND == 0 ? pol.plain_lines : 0);
    const int now[4] = {n_sets, p.nt_stores, p.plain_lines, s.wg_per_cu};
    if (h->policy_debug && memcmp(now, h->policy_printed, sizeof(now)) != 0) {
        memcpy(h->policy_printed, now, sizeof(now));
        fprintf(stderr, "sgx store policy: kind %d games %lld sets %d cus %d resident_wgs_per_cu %d games_per_wg %d rewrite_set %lld budget %lld -> nt_stores %d plain_lines %d\n",
                KIND, (long long)s.games, (int)n_sets, s.cus, s.wg_per_cu, s.games_per_wg, (long long)sgx_store_rewrite_set(&s), (long long)s.budget,
                (int)p.nt_stores, (int)p.plain_lines);
    }
    return SGX_OK;
}

// One launch of steps_kernel.
static int steps_launch(sgx_env *h, WaveStepsParams &sp, KParams &p, const int32_t *w, hipStream_t stream, bool *ok) {
    const sgx_step_io &io = p.io;
    const bool compact = (io.flags & (SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK)) != 0;
    const bool no_obs = !io.obs_dev && !io.fobs_dev && !io.final_obs_dev && !io.final_fobs_dev && !compact;
    const int kind = compact ? 4 : no_obs ? 8 : (io.fobs_dev || io.final_fobs_dev) ? 1 : 0;
    // A barrier per step between the waves of a workgroup: on a long ring or trajectory buffer (the resident waves cycle through more sets than
    // the address translation caches hold pages for: DESIGN.md section 4.4) the workgroup's games then write one set at a time.  In-process A/B
    // of the two modes, drifting -> in step (tools/barrier_footprint_ab.py; profiles/r06_barrier_boards_ab.log, r06_barrier_footprint_ab.log):
    //   10x10  trajectory buffer of 12 / 16 / 64 slots -1.1 / -1.7 / -4.1 %, rings of 12 / 16 / 24 / 32 / 64 separate sets -1.1 / -1.9 / -2.9 / -3.3 /
    //          -4.2 %, ring of 3 (tuned buffers) 243.6 -> 242.1 us
    //   6x6    16 / 32 / 64 slots -4.2 / -6.3 / -9.3 %, rings of 12 / 24 / 32 / 64 sets +1.7 / +0.1 / -7.2 / -7.3 %
    //   8x8    16 / 32 / 64 slots -2.2 / -2.4 / -2.8 %, rings of 12 ... 64 sets 0.0 ... -0.9 %
    //   15x15  16 / 32 / 64 slots -2.0 / -2.3 / -2.4 %, rings of 24 ... 64 sets +1.0 ... -0.2 %, of 8 / 12 sets +2 ... +3 %
    //   5x5 (two games per wave) +3 ... +9 % on rings, -4 / +6 % on 64 slots by batch size;  launches that render no float32 observation
    //   (compact, mask-only, logic-only) +3 ... +8 %
    // so: float32 observations, one game per wave (36 .. 225 cells), from 9 sets / slots on 10x10 and from 16 elsewhere.  Never on a launch with a
    // partly empty last workgroup (its missing waves have left the kernel).
    const int cells = h->cfg.rows * h->cfg.cols;
    const bool pays = (kind == 0 || kind == 1) && cells >= 36 && cells <= 225 && sp.n_sets >= (cells == 100 ? WSTEPS_MAX_SETS + 1 : 16);
    const bool want_barrier = h->steps_barrier > 0 || (h->steps_barrier < 0 && pays);
    *ok = true;
    int policy_rc = SGX_OK;
    const int geo_rc = for_geometry(h, [&](auto r, auto c) {
        constexpr int R = decltype(r)::value, C = decltype(c)::value;
        auto launch = [&](auto kind_c) {
            constexpr int KIND = decltype(kind_c)::value;
            with_half_wave<R, C, KIND>(h, [&](auto var) {
                constexpr int VAR = decltype(var)::value;
                using G = Geo<R, C, VAR>;
                const unsigned grid = geo_grid<G>(p, w);
                if constexpr ((KIND == 0 || KIND == 1) && VAR == 0 && (R * C) % 4 == 0) {
                    if (int rc = steps_policy<R, C, KIND>(h, p, sp.n_sets)) { policy_rc = rc; return; }
                }
                sp.k = p;
                sp.barrier = want_barrier && (p.n_envs - p.env_first) % (G::WPB * G::GPW) == 0;
                if (h->pool) steps_kernel_pool<R, C, KIND, VAR><<<grid, 64 * G::WPB, 0, stream>>>(WaveStepsParamsPool{sp, make_pool_params(h)});
                else steps_kernel<R, C, KIND, VAR><<<grid, 64 * G::WPB, 0, stream>>>(sp);
            });
        };
        if (kind == 0) launch(int_c<0>());
        else if (kind == 1) launch(int_c<1>());
        else if (kind == 4) launch(int_c<4>());
        else launch(int_c<8>());
    });
    return geo_rc ? geo_rc : policy_rc;
}

// All n_steps of a rollout call -- output sets first, first + 1, ... round-robin -- in the multi-step launches of one kernel family (SP =
// StepsParams: lane_steps_kernel, WaveStepsParams: steps_kernel) where the call is eligible for it; *launched tells.
template <class SP>
static int multi_step(sgx_env *h, const KParams &p_in, const OutSets &sets, int32_t first, int32_t n_steps, void *stream, bool *launched) {
    constexpr bool lane = std::is_same<SP, StepsParams>::value;
    *launched = false;
    const int32_t n_sets = sets.n_sets;
    KParams p = p_in;
    p.mode = 0;
    p.io = sets.ios[sets.strided ? 0 : first];
    if (n_steps < 2 || h->no_multi_step || !(lane ? lane_steps_ok(h, p, sets) : wave_steps_ok(h, p, sets)) || !sets_share_results(sets, p.io)) return SGX_OK;
    if (int rc = check_step_io(h, p)) return rc;
    SP sp;
    memset(&sp, 0, sizeof(sp));
    sp.n_sets = n_sets;
    if (sets.strided) {
        sp.strided = 1;
        sp.obs_slot_bytes = sets.obs_b; sp.mask_slot_bytes = sets.mask_b;
        sp.obs[0] = p.io.obs_dev; sp.mask[0] = p.io.mask_dev;
        if constexpr (!lane) { sp.fobs_slot_bytes = sets.fobs_b; sp.fobs[0] = p.io.fobs_dev; }
    } else if (n_sets > (int32_t)std::extent<decltype(sp.obs)>::value) {      // more separate sets than the kernel arguments hold: a device table
        void **tab = nullptr;
        if (int rc = upload_ring_table(h, sets, (hipStream_t)stream, &tab)) return rc;
        sp.strided = 2;
        sp.obs_tab = reinterpret_cast<float *const *>(tab);
        sp.mask_tab = reinterpret_cast<uint8_t *const *>(tab + 2 * n_sets);
        if constexpr (!lane) sp.fobs_tab = reinterpret_cast<float *const *>(tab + n_sets);
    } else
        for (int32_t k = 0; k < n_sets; ++k) {
            sp.obs[k] = sets.ios[k].obs_dev; sp.mask[k] = sets.ios[k].mask_dev;
            if constexpr (!lane) sp.fobs[k] = sets.ios[k].fobs_dev;
        }
    int32_t w[8];
    launch_setup(h, p, n_sets, w);
    for (int32_t done = 0; done < n_steps; ) {
        const int32_t now = n_steps - done > SGX_STEPS_MAX_PER_LAUNCH ? SGX_STEPS_MAX_PER_LAUNCH : n_steps - done;
        const int32_t set = (int32_t)(((int64_t)first + done) % n_sets);
        if (now < 2) {                                                      // a single step left over: the ordinary launch
            if (int rc = launch_set_step(h, p_in, sets, set, stream)) return rc;
        } else {
            sp.n_steps = now; sp.first_set = set;
            bool ok = false;
            if (int rc = steps_launch(h, sp, p, w, (hipStream_t)stream, &ok)) return rc;
            if (!ok) {
                if (done == 0) return SGX_OK;                               // (not this runtime: nothing was launched)
                return fail(SGX_EDEVICE, "lane_steps_kernel became unavailable in the middle of a call%s");
            }
            HIP_TRY(hipGetLastError());
        }
        done += now;
    }
    if (sp.strided == 2)
        if (int rc = ring_table_done(h, (hipStream_t)stream)) return rc;
    *launched = true;
    h->last_kind = lane ? SGX_LAUNCH_MULTI_STEP : SGX_LAUNCH_MULTI_STEP_WAVE;
    return SGX_OK;
}

// The multi-step launch of a rollout call: the lane-per-game kernel's where the call is eligible for it, else the wave-per-game kernels'.
static int multi_steps(sgx_env *h, const KParams &p, const OutSets &sets, int32_t first, int32_t n_steps, void *stream, bool *launched) {
    if (int rc = multi_step<StepsParams>(h, p, sets, first, n_steps, stream, launched)) return rc;
    if (*launched) return SGX_OK;
    return multi_step<WaveStepsParams>(h, p, sets, first, n_steps, stream, launched);
}

// The steps of sgx_step_n / sgx_step_ring / sgx_step_traj: a multi-step launch, else one launch per step.
static int play_steps(sgx_env *h, const KParams &p, const OutSets &sets, int32_t first, int32_t n_steps, void *stream) {
    bool launched = false;
    if (int rc = multi_steps(h, p, sets, first, n_steps, stream, &launched)) return rc;
    for (int32_t i = 0; i < n_steps && !launched; ++i)
        if (int rc = launch_set_step(h, p, sets, (int32_t)(((int64_t)first + i) % sets.n_sets), stream)) return rc;
    return SGX_OK;
}

static int launch_step(sgx_env *h, const KParams &p_in, void *stream, int ring_sets, int64_t start_index_off, bool allow_pool) {
    KParams p = p_in;
    if (int rc = check_step_io(h, p)) return rc;
    int32_t w[8];
    launch_setup(h, p, ring_sets, w);
    const hipStream_t st = (hipStream_t)stream;
    const bool full = p.io.fobs_dev || p.io.final_fobs_dev, original = (p.io.flags & SGX_STEP_ORIGINAL_CHANNELS) != 0;
    const bool compact = (p.io.flags & (SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK)) != 0;
    // a handle with a start pool steps through the *_pool kernels (an auto-reset loads a pool record; every step writes start_index)
    const bool pool = allow_pool && h->pool != nullptr && p.mode == 0;
    const PoolParams pool_params = make_pool_params(h, start_index_off);
    if (compact) {
        // compact outputs: the 67-channel 'extended' observation as 4-bit codes / the mover's-perspective mask as bits, nothing else
        if (full || original || p.io.final_obs_dev || p.src_boards || (p.io.flags & (SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS)))
            return fail(SGX_EINVAL, "compact outputs come with the 67-channel partial observation and the perspective mask only (no fobs / final_obs / original channels / state-coordinate masks)%s");
        if ((reinterpret_cast<uintptr_t>(p.io.obs_dev) | reinterpret_cast<uintptr_t>(p.io.mask_dev)) & 15)
            return fail(SGX_EINVAL, "compact outputs need 16-byte aligned obs_dev / mask_dev%s");
    }
    if (lane_eligible(h, p, full, original)) {
        // boards of at most 16 cells: one game per lane, 64 games per wave (sgx_lane_kernel.h)
        if (int rc = for_geometry(h, [&](auto r, auto c) {
                constexpr int R = decltype(r)::value, C = decltype(c)::value;
                if constexpr (lane_geometry<Geo<R, C>>()) {
                    const unsigned grid = grid_for(p, 64, w);
                    const size_t dyn = 64 * (size_t)(p.rec_bytes + 16);
                    if (p.mode) lane_kernel<R, C, true><<<grid, 64, dyn, st>>>(p);
                    else if (pool) lane_kernel_pool<R, C><<<grid, 64, dyn, st>>>(p, pool_params);
                    else lane_kernel<R, C, false><<<grid, 64, dyn, st>>>(p);
                }
            })) return rc;
        HIP_TRY(hipGetLastError());
        h->last_kind = SGX_LAUNCH_LANE;
        return SGX_OK;
    }
    // no observation pointer at all (search expansions, mask-only steps, logic-only rollouts): the kind without observation tables
    const bool no_obs = !p.io.obs_dev && !p.io.fobs_dev && !p.io.final_obs_dev && !p.io.final_fobs_dev && !compact;
    const bool mapped = (p.io.flags & (SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS)) || p.src_boards;
    if (mapped && (full || (original && !no_obs))) return fail(SGX_EINVAL, "state-coordinate masks and sgx_expand come with the 67-channel partial observation only%s");
    const int kind = compact ? 4 : no_obs ? 8 : (full ? 1 : 0) + (original ? 2 : 0);      // (sgx_layout.h: ObsKind)
    if (pool && mapped && p.io.auto_reset)
        return fail(SGX_EINVAL, "a handle with a start pool does not auto-reset in launches with state-coordinate masks (SGX_STEP_MASK_1D / _STATE_COORDS)%s");
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            auto launch = [&](auto kind_c, auto mapped_c) {
                constexpr int KIND = decltype(kind_c)::value;
                constexpr bool MAPPED = decltype(mapped_c)::value;
                with_half_wave<R, C, KIND>(h, [&](auto var) {
                    constexpr int VAR = decltype(var)::value;
                    using G = Geo<R, C, VAR>;
                    const unsigned grid = geo_grid<G>(p, w);
                    if (p.mode) observe_kernel<R, C, KIND, MAPPED, VAR><<<grid, 64 * G::WPB, 0, st>>>(p);
                    else if constexpr (!MAPPED) {
                        if (pool) {             // one step of steps_kernel_pool, writing the launch's own tensors
                            WaveStepsParams sp;
                            memset(&sp, 0, sizeof(sp));
                            sp.k = p;
                            sp.k.traj_res_envs = sp.k.traj_out_envs = 0;       // (a step of an sgx_step_traj call: launch_set_step has moved the pointers)
                            sp.k.traj_act_log = nullptr;
                            sp.k.plain_lines = 0;                              // (a per-step launch: no plain share, SGX_NT_PLAIN_LINES or not)
                            sp.n_steps = sp.n_sets = 1;
                            sp.obs[0] = p.io.obs_dev; sp.fobs[0] = p.io.fobs_dev; sp.mask[0] = p.io.mask_dev;
                            steps_kernel_pool<R, C, KIND, VAR><<<grid, 64 * G::WPB, 0, st>>>(WaveStepsParamsPool{sp, pool_params});
                        } else step_kernel<R, C, KIND, MAPPED, VAR><<<grid, 64 * G::WPB, 0, st>>>(p);
                    } else step_kernel<R, C, KIND, MAPPED, VAR><<<grid, 64 * G::WPB, 0, st>>>(p);
                });
            };
            if (mapped) {
                if (kind == 8) launch(int_c<8>(), bool_c<true>());
                else launch(int_c<0>(), bool_c<true>());
            } else if (kind == 0) launch(int_c<0>(), bool_c<false>());
            else if (kind == 1) launch(int_c<1>(), bool_c<false>());
            else if (kind == 2) launch(int_c<2>(), bool_c<false>());
            else if (kind == 3) launch(int_c<3>(), bool_c<false>());
            else if (kind == 4) launch(int_c<4>(), bool_c<false>());
            else launch(int_c<8>(), bool_c<false>());
        })) return rc;
    HIP_TRY(hipGetLastError());
    h->last_kind = SGX_LAUNCH_WAVE;
    return SGX_OK;
}

SGX_API int sgx_observe(sgx_env *h, float *obs_dev, float *fobs_dev, uint8_t *mask_dev, int8_t *player_dev, int32_t flags, void *stream) {
    if (!h) return fail(SGX_EINVAL, "handle is NULL%s");
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    p.mode = 1;
    p.io.obs_dev = obs_dev;
    p.io.fobs_dev = fobs_dev;
    p.io.flags = flags & (SGX_STEP_RAW_OBS | SGX_STEP_ORIGINAL_CHANNELS | SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS | SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK);
    p.io.mask_dev = mask_dev;
    p.io.player_dev = player_dev;
    if (int rc = check_io_pointers(h, p.io, "sgx_observe")) return rc;
    return launch_step(h, p, stream);
}

namespace {
// Two timing events, destroyed with the pair (err: how creating them went).  time(): the milliseconds `launches` calls of launch() -- an
// SGX_* code each -- take on `stream`, after one untimed first touch; the first launch's error, else a failed event call as SGX_EDEVICE
// with the message `what` (a format for the HIP error string).
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err;
    EventPair() {
        err = hipEventCreate(&e0);
        if (err == hipSuccess) err = hipEventCreate(&e1);
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    template <class F>
    int time(hipStream_t stream, int32_t launches, const char *what, float *ms, F &&launch) {
        if (int rc = launch()) return rc;
        hipError_t e = hipEventRecord(e0, stream);
        for (int32_t i = 0; i < launches; ++i)
            if (int rc = launch()) return rc;
        if (e == hipSuccess) e = hipEventRecord(e1, stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
        return e == hipSuccess ? SGX_OK : fail(SGX_EDEVICE, what, hipGetErrorString(e));
    }
};
}  // namespace

SGX_API int sgx_time_observe(sgx_env *h, float *obs_dev, uint8_t *mask_dev, int32_t launches, void *stream, float *microseconds) {
    if (!h || !microseconds || launches <= 0) return fail(SGX_EINVAL, "bad argument%s");
    SGX_ON_DEVICE(h->device);
    EventPair ev;
    if (ev.err != hipSuccess) return fail(SGX_EDEVICE, "hipEventCreate: %s", hipGetErrorString(ev.err));
    float ms = 0.f;
    if (int rc = ev.time((hipStream_t)stream, launches, "timing events: %s", &ms,
                         [&] { return sgx_observe(h, obs_dev, nullptr, mask_dev, nullptr, 0, stream); })) return rc;
    *microseconds = ms * 1000.f / (float)launches;
    return SGX_OK;
}

// ---- device-memory probe: GB/s of `launches` probe launches over [ptr, ptr + bytes)
SGX_API int sgx_mem_probe(int device, void *ptr_dev, int64_t bytes, int32_t launches, void *stream, float *gb_per_s) {
    if (!ptr_dev || !gb_per_s || launches <= 0 || bytes <= 0) return fail(SGX_EINVAL, "sgx_mem_probe: bad argument%s");
    if ((reinterpret_cast<uintptr_t>(ptr_dev) & 1023) != 0) return fail(SGX_EINVAL, "sgx_mem_probe: the range must start on a 1 KiB boundary%s");
    SGX_ON_DEVICE(device);
    const int64_t n_seg = bytes / PROBE_SEG;
    if (n_seg < 1) return fail(SGX_EINVAL, "sgx_mem_probe: range shorter than one 26 KiB segment%s");
    EventPair ev;
    if (ev.err != hipSuccess) return fail(SGX_EDEVICE, "hipEventCreate: %s", hipGetErrorString(ev.err));
    const int64_t want = ((int64_t)1 << 30) / PROBE_SEG;                      // at least ~1 GiB of stores per launch
    const int64_t passes = n_seg >= want ? 1 : (want + n_seg - 1) / n_seg, n_waves = n_seg * passes;
    const unsigned grid = (unsigned)((((n_waves + 7) / 8) + 7) & ~(int64_t)7);
    const hipStream_t st = (hipStream_t)stream;
    float ms = 0.f;
    if (int rc = ev.time(st, launches, "sgx_mem_probe: %s", &ms, [&] {
            mem_probe_kernel<<<grid, 512, 0, st>>>((char *)ptr_dev, n_seg, n_waves);
            return SGX_OK;
        })) return rc;
    *gb_per_s = (float)((double)n_waves * PROBE_SEG * launches / (ms * 1e-3) / 1e9);
    return SGX_OK;
}

// The step kernel's store stream without the game (sgx_mem.h: store_probe_kernel): what the memory takes from exactly this store shape.
SGX_API int sgx_store_probe(int device, void *ptr_dev, int64_t bytes, int32_t seg_bytes, int32_t passes, int32_t payload, int32_t nt_stores,
                            int32_t waves_per_cu, int32_t pace, int32_t persistent, int32_t dwell, int32_t ring, int32_t launches, void *stream,
                            float *microseconds_per_launch, float *gb_per_s) {
    if (!ptr_dev || !microseconds_per_launch || !gb_per_s || launches <= 0 || passes <= 0 || bytes <= 0) return fail(SGX_EINVAL, "sgx_store_probe: bad argument%s");
    if (seg_bytes < 16 || (seg_bytes & 15) || (reinterpret_cast<uintptr_t>(ptr_dev) & 15)) return fail(SGX_EINVAL, "sgx_store_probe: segments and the range are 16-byte aligned%s");
    if (payload < 0 || payload > 2) return fail(SGX_EINVAL, "sgx_store_probe: payload 0 (zeros), 1 (observation-like) or 2 (random bits)%s");
    if (pace < 0 || pace > 4096) return fail(SGX_EINVAL, "sgx_store_probe: pace 0 .. 4096%s");
    if (waves_per_cu != 0 && waves_per_cu != 8 && waves_per_cu != 16 && waves_per_cu != 24) return fail(SGX_EINVAL, "sgx_store_probe: waves_per_cu 0 (= 24), 8, 16 or 24%s");
    if (dwell < 1 || ring < 1 || ring > 8 || (dwell > 1 && !persistent)) return fail(SGX_EINVAL, "sgx_store_probe: dwell >= 1 (> 1 with persistent waves only), ring 1 .. 8%s");
    // `ring` sub-ranges of equal size (whole segments, 1 KiB aligned starts); a pass covers ONE sub-range's segments
    const int64_t ring_bytes = ring > 1 ? ((bytes / ring) & ~(int64_t)1023) : 0;
    const int64_t n_seg = (((ring > 1 ? ring_bytes : bytes) / seg_bytes)) & ~(int64_t)63;   // eight waves per workgroup, eight XCD shares
    if (n_seg < 64) return fail(SGX_EINVAL, "sgx_store_probe: the range holds fewer than 64 segments%s");
    const int64_t groups_per_pass = n_seg / 8;
    int64_t grid = groups_per_pass * passes;
    if (grid > 0x7fffffff) return fail(SGX_EINVAL, "sgx_store_probe: passes x segments exceed one grid%s");
    SGX_ON_DEVICE(device);
    if (persistent) {                                                          // the resident workgroups only: CUs x (waves per CU / 8)
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        const int64_t resident = (int64_t)prop.multiProcessorCount * ((waves_per_cu ? waves_per_cu : 24) / 8);
        if (resident < grid) grid = resident & ~(int64_t)7;
    }
    hipStream_t st = (hipStream_t)stream;
    // resident workgroups per CU through unused dynamic LDS: 160 KiB per CU / (what one workgroup asks for)
    const size_t dyn = waves_per_cu == 8 ? 100 * 1024 : waves_per_cu == 16 ? 60 * 1024 : 0;
    if (dyn > 64 * 1024) {
        hipError_t ea = hipSuccess;
        if (payload == 0) ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&store_probe_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        else if (payload == 1) ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&store_probe_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        else ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&store_probe_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        if (ea != hipSuccess) return fail(SGX_EDEVICE, "sgx_store_probe: %s", hipGetErrorString(ea));
    }
    EventPair ev;
    if (ev.err != hipSuccess) return fail(SGX_EDEVICE, "sgx_store_probe: %s", hipGetErrorString(ev.err));
    static uint32_t salt = 0x5EED5EEDu;
    float ms = 0.f;
    if (int rc = ev.time(st, launches, "sgx_store_probe: %s", &ms, [&] {
            salt = salt * 1664525u + 1013904223u;
            if (payload == 0) store_probe_kernel<0><<<(unsigned)grid, 512, dyn, st>>>((char *)ptr_dev, groups_per_pass, passes, seg_bytes, nt_stores, salt, pace, persistent ? 1 : 0, dwell, ring, ring_bytes);
            else if (payload == 1) store_probe_kernel<1><<<(unsigned)grid, 512, dyn, st>>>((char *)ptr_dev, groups_per_pass, passes, seg_bytes, nt_stores, salt, pace, persistent ? 1 : 0, dwell, ring, ring_bytes);
            else store_probe_kernel<2><<<(unsigned)grid, 512, dyn, st>>>((char *)ptr_dev, groups_per_pass, passes, seg_bytes, nt_stores, salt, pace, persistent ? 1 : 0, dwell, ring, ring_bytes);
            return SGX_OK;
        })) return rc;
    *microseconds_per_launch = ms * 1000.f / (float)launches;
    *gb_per_s = (float)((double)n_seg * seg_bytes * passes * dwell * launches / (ms * 1e-3) / 1e9);
    return SGX_OK;
}

// ---- library-owned output buffers with a bounded placement trial
namespace {

struct TrialCtx {
    sgx_env *h;
    void *stream;
    int32_t flags;
    EventPair ev;
};

// average launch time of 6 sgx_observe launches writing the given buffers (one untimed first touch)
int time_candidate(TrialCtx &c, float *obs, float *fobs, uint8_t *mask, float *us) {
    const int launches = 6;
    float ms = 0.f;
    if (int rc = c.ev.time((hipStream_t)c.stream, launches, "timing events: %s", &ms,
                           [&] { return sgx_observe(c.h, obs, fobs, mask, nullptr, c.flags, c.stream); })) return rc;
    *us = ms * 1000.f / (float)launches;
    return SGX_OK;
}

// Picks the fastest of up to max_trials allocations of `bytes`.  Candidate k > 0 is allocated behind a padding allocation of
// k * step bytes, which is released again before the candidate is timed, so that at most (candidate + padding) is held beyond
// the buffer that is kept.  `which` = 0: the candidate is the partial observation buffer, 1: the fully-observable one.
int pick_buffer(TrialCtx &c, int which, size_t bytes, float *obs_fixed, uint8_t *mask, int64_t max_extra, int32_t max_trials,
                float **best_out, float *trial_us, int32_t *n_trials, int64_t *peak_extra) {
    float *best = nullptr;
    if (hipMalloc((void **)&best, bytes) != hipSuccess) return fail(SGX_ENOMEM, "device allocation failed (output buffer)%s");
    *best_out = best;
    *n_trials = 0;
    const bool can_try = max_trials > 1 && max_extra >= (int64_t)bytes;
    if (!can_try) return SGX_OK;
    float best_us = 0.f;
    int rc = time_candidate(c, which ? obs_fixed : best, which ? best : nullptr, mask, &best_us);
    if (rc != SGX_OK) return rc;
    trial_us[0] = best_us;
    *n_trials = 1;
    const float target = which == 0 ? c.h->placement_target_us : 0.f;      // (the target is a partial-observation launch time)
    if (target > 0.f && best_us <= 1.03f * target) return SGX_OK;
    const size_t room = (size_t)max_extra - bytes;                        // what the padding may take
    size_t step = bytes / 8;                                              // (a big buffer leaves little room: smaller steps then)
    if (step * 12 > room) step = room / 12;
    // a generous budget is spread over all of it: with max_extra_bytes far beyond 32 x bytes / 8 the candidates sample the whole range
    const int32_t n_cand = (max_trials < SGX_OUT_MAX_TRIALS ? max_trials : SGX_OUT_MAX_TRIALS) - 1;
    const bool spread = n_cand > 0 && room / (size_t)n_cand > step;
    if (spread) step = room / (size_t)n_cand;
    step = (step + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    if (spread && step > ((size_t)2 << 20) && step * (size_t)n_cand > room) step -= (size_t)2 << 20;      // (the last candidate must fit too)
    int first_good = -1;
    for (int k = 1; k < max_trials && k < SGX_OUT_MAX_TRIALS; ++k) {
        const size_t pad_bytes = (size_t)k * step;
        if (pad_bytes > room) break;
        void *pad = nullptr;
        float *cand = nullptr;
        if (hipMalloc(&pad, pad_bytes) != hipSuccess) { (void)hipGetLastError(); break; }         // memory is short: settle
        if (hipMalloc((void **)&cand, bytes) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(pad); break; }
        if ((int64_t)(pad_bytes + bytes) > *peak_extra) *peak_extra = (int64_t)(pad_bytes + bytes);
        (void)hipFree(pad);
        float us = 0.f;
        rc = time_candidate(c, which ? obs_fixed : cand, which ? cand : nullptr, mask, &us);
        if (rc != SGX_OK) { (void)hipFree(cand); return rc; }
        trial_us[k] = us;
        *n_trials = k + 1;
        if (us < best_us) { (void)hipFree(best); best = cand; best_us = us; *best_out = best; }
        else (void)hipFree(cand);
        // Early stop: the classes lie >= 10 % apart; once the kept candidate beats the slowest one seen by
        // that much the fast class has been found and more candidates would only cost start-up time.  (A run of equally slow
        // candidates is no reason to stop: fast memory was found behind six and more slow candidates on several boxes.)
        // Two steps: the classes are ~255-265 / 300-310 / 320-330 / ~345 us (65,536 Barrage games): a candidate 9 % below the slowest may
        // be the middle class only, so the search goes on for up to eight more candidates and stops at once at 17 % (fast class: 272-277 us after 335-340 us;
        // 282 us, 16 %, is not the best a box has).
        if (target > 0.f) {                           // a ring of output sets: every set as fast as the first one (sgx_set_placement_target)
            if (best_us <= 1.03f * target) break;
            continue;
        }
        float worst = 0.f;
        for (int j = 0; j <= k; ++j) worst = trial_us[j] > worst ? trial_us[j] : worst;
        if (k >= 2 && best_us < 0.83f * worst) break;
        if (k >= 2 && best_us < 0.91f * worst && first_good < 0) first_good = k;
        if (first_good >= 0 && k - first_good >= 8) break;
    }
    return SGX_OK;
}

}  // namespace

SGX_API int sgx_free_outputs(sgx_env *h, sgx_outputs *out) {
    if (!out) return fail(SGX_EINVAL, "NULL argument%s");
    if (!out->obs_dev && !out->fobs_dev && !out->mask_dev) return SGX_OK;
    SGX_ON_DEVICE(h ? h->device : out->device);
    HIP_TRY(hipDeviceSynchronize());
    if (out->obs_dev) (void)hipFree(out->obs_dev);
    if (out->fobs_dev) (void)hipFree(out->fobs_dev);
    if (out->mask_dev) (void)hipFree(out->mask_dev);
    out->obs_dev = out->fobs_dev = nullptr;
    out->mask_dev = nullptr;
    return SGX_OK;
}

SGX_API int sgx_alloc_outputs(sgx_env *h, int32_t flags, int64_t max_extra_bytes, int32_t max_trials, void *stream, sgx_outputs *out) {
    if (!h || !out) return fail(SGX_EINVAL, "NULL argument%s");
    if (flags & ~(SGX_OUT_FULL_OBS | SGX_STEP_ORIGINAL_CHANNELS)) return fail(SGX_EINVAL, "sgx_alloc_outputs: unknown flag%s");
    memset(out, 0, sizeof(*out));
    out->device = h->device;
    SGX_ON_DEVICE(h->device);
    const bool original = (flags & SGX_STEP_ORIGINAL_CHANNELS) != 0, full = (flags & SGX_OUT_FULL_OBS) != 0;
    const int64_t cells = (int64_t)h->cfg.rows * h->cfg.cols;
    out->obs_bytes = h->n_envs * cells * lut_channels(false, original) * 4;
    out->fobs_bytes = full ? h->n_envs * cells * lut_channels(true, original) * 4 : 0;
    out->mask_bytes = h->n_envs * cells * h->K;
    if (hipMalloc((void **)&out->mask_dev, (size_t)out->mask_bytes) != hipSuccess) return fail(SGX_ENOMEM, "device allocation failed (mask buffer)%s");
    TrialCtx c{h, stream, flags & SGX_STEP_ORIGINAL_CHANNELS};
    int rc = c.ev.err != hipSuccess ? fail(SGX_EDEVICE, "hipEventCreate failed%s") : SGX_OK;
    if (rc == SGX_OK)
        rc = pick_buffer(c, 0, (size_t)out->obs_bytes, nullptr, out->mask_dev, max_extra_bytes, max_trials, &out->obs_dev, out->trial_us,
                         &out->n_trials, &out->peak_extra_bytes);
    if (rc == SGX_OK && full)
        rc = pick_buffer(c, 1, (size_t)out->fobs_bytes, out->obs_dev, out->mask_dev, max_extra_bytes, max_trials, &out->fobs_dev, out->ftrial_us,
                         &out->n_ftrials, &out->peak_extra_bytes);
    if (rc != SGX_OK) {
        const std::string keep = g_last_error;
        (void)sgx_free_outputs(h, out);
        g_last_error = keep;
        return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    return SGX_OK;
}

SGX_API int sgx_step(sgx_env *h, const sgx_step_io *io, void *stream) {
    if (!h || !io) return fail(SGX_EINVAL, "handle or io is NULL%s");
    if (!io->actions_dev) return fail(SGX_EINVAL, "actions_dev is NULL%s");
    if (int rc = check_io_pointers(h, *io, "sgx_step")) return rc;
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    p.mode = 0;
    p.io = *io;
    return launch_step(h, p, stream);
}

// ---- single-game latency (the N = 1 facade): outputs in device-addressable pinned host memory, one call per env.step()
SGX_API int sgx_host_alloc(sgx_env *h, int64_t bytes, void **host_ptr, void **dev_ptr) {
    if (!h || !host_ptr || !dev_ptr || bytes <= 0) return fail(SGX_EINVAL, "sgx_host_alloc: bad argument%s");
    SGX_ON_DEVICE(h->device);
    void *p = nullptr, *d = nullptr;
    // fine-grained (coherent) whatever HIP_HOST_COHERENT says: sgx_step_sync's polled path returns as soon as the kernel has published
    // its completion word, usually before the kernel has retired -- the outputs in this slab must be visible to the host at that
    // moment, which coarse-grained host memory guarantees only at the end of the kernel
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return fail(SGX_ENOMEM, "pinned host allocation failed%s"); }
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(p); return fail(SGX_EDEVICE, "hipHostGetDevicePointer failed%s"); }
    memset(p, 0, (size_t)bytes);
    *host_ptr = p;
    *dev_ptr = d;
    return SGX_OK;
}

SGX_API int sgx_host_free(sgx_env *h, void *host_ptr) {
    if (!host_ptr) return SGX_OK;
    int dev = 0;
    if (h) dev = h->device;
    else HIP_TRY(hipGetDevice(&dev));
    SGX_ON_DEVICE(dev);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipHostFree(host_ptr));
    return SGX_OK;
}

// env.step() and wait for its outputs.  A handful of games on a 4-aligned one-game-per-wave board in an 'extended' channel mode (the
// N = 1 facade) run as single_kernel -- one workgroup per game, completion published in a host-mapped word this call polls; anything
// else is sgx_step + hipStreamSynchronize.
#define SGX_SINGLE_MAX_ENVS 8
namespace {
int step_single(sgx_env *h, const KParams &p, bool full, hipStream_t stream, bool *launched) {
    *launched = false;
    if (!h->sync_count) {
        // all three resources into locals, published to the handle only when every step has succeeded (a half-initialised handle would
        // launch single_kernel with a NULL workgroup counter on the next call)
        void *hp = nullptr, *dp = nullptr;
        uint32_t *cnt = nullptr;
        hipError_t e = hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent);   // (fine-grained whatever HIP_HOST_COHERENT says: the kernel's release store must be visible while it still runs)
        if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, hp, 0);
        if (e == hipSuccess) { memset(hp, 0, 64); e = hipMalloc((void **)&cnt, 64); }
        if (e == hipSuccess) e = hipMemset(cnt, 0, 64);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (cnt) (void)hipFree(cnt);
            if (hp) (void)hipHostFree(hp);
            return fail(SGX_EDEVICE, "sgx_step_sync: completion word: %s", hipGetErrorString(e));
        }
        h->sync_flag_host = (uint32_t *)hp;
        h->sync_flag_dev = (uint32_t *)dp;
        h->sync_count = cnt;
    }
    const uint32_t seq = ++h->sync_seq;
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            if constexpr (Geo<R, C>::LPG == 64 && !Geo<R, C>::WIDE && (R * C) % 4 == 0) {
                if (h->pool && full) single_kernel_pool<R, C, 1><<<(unsigned)h->n_envs, 64 * SINGLE_WAVES, 0, stream>>>(p, make_pool_params(h), h->sync_count, h->sync_flag_dev, seq);
                else if (h->pool) single_kernel_pool<R, C, 0><<<(unsigned)h->n_envs, 64 * SINGLE_WAVES, 0, stream>>>(p, make_pool_params(h), h->sync_count, h->sync_flag_dev, seq);
                else if (full) single_kernel<R, C, 1><<<(unsigned)h->n_envs, 64 * SINGLE_WAVES, 0, stream>>>(p, h->sync_count, h->sync_flag_dev, seq);
                else single_kernel<R, C, 0><<<(unsigned)h->n_envs, 64 * SINGLE_WAVES, 0, stream>>>(p, h->sync_count, h->sync_flag_dev, seq);
                *launched = true;
            }
        })) return rc;
    if (!*launched) return SGX_OK;
    HIP_TRY(hipGetLastError());
    // poll the word the last workgroup writes after a system-scope fence; look at the stream now and then, so that a launch that
    // failed on the device ends the wait with its error instead of hanging
    volatile uint32_t *flag = h->sync_flag_host;
    // a step is ~6 us of kernel: spin with `pause` for the first ~2^14 polls (about a millisecond); then yield the core between polls
    // for ~4,000 polls; then BACK OFF -- sleep between polls, 2 us doubling up to 64 us -- so that a long wait (a queue backed up behind
    // other work, a device that hangs) costs next to nothing on the host.  From the yielding phase on the stream is looked at every 256th
    // poll (every poll once sleeping), so that a launch that failed on the device ends the wait with its error instead of hanging.
    for (uint32_t spins = 0; *flag != seq; ++spins) {
        const bool slow = spins >= (1u << 14), sleeping = spins >= (1u << 14) + 4096u;
        if (sleeping) {
            const uint32_t k = (spins - ((1u << 14) + 4096u)) >> 4;                  // 16 polls per back-off level
            struct timespec ts = {0, (long)(2000u << (k < 5u ? k : 5u))};
            nanosleep(&ts, nullptr);
        } else if (slow) sched_yield();
        else __builtin_ia32_pause();
        if (sleeping || (slow && (spins & 0xFF) == 0)) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) break;                          // the kernel has retired: its stores are visible
            if (q != hipErrorNotReady) return fail(SGX_EDEVICE, "sgx_step_sync: %s", hipGetErrorString(q));
            (void)hipGetLastError();
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return SGX_OK;
}
}  // namespace

SGX_API int sgx_step_sync(sgx_env *h, const sgx_step_io *io, void *stream) {
    if (!h || !io) return fail(SGX_EINVAL, "handle or io is NULL%s");
    if (!io->actions_dev) return fail(SGX_EINVAL, "actions_dev is NULL%s");
    if (int rc = check_io_pointers(h, *io, "sgx_step_sync")) return rc;
    const bool original = (io->flags & SGX_STEP_ORIGINAL_CHANNELS) != 0;
    if (h->n_envs <= SGX_SINGLE_MAX_ENVS && !original && !(io->flags & (SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS | SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK)) && h->map_mode == 0 &&
        !h->no_single) {
        SGX_ON_DEVICE(h->device);
        KParams p = make_params(h);
        p.mode = 0;
        p.io = *io;
        if (int rc = check_step_io(h, p)) return rc;
        bool launched = false;
        if (int rc = step_single(h, p, io->fobs_dev || io->final_fobs_dev, (hipStream_t)stream, &launched)) return rc;
        if (launched) return SGX_OK;
    }
    if (int rc = sgx_step(h, io, stream)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SGX_OK;
}

// Forks `chains` streams of the handle off the caller's (created on first use, with their join events): each waits for what `stream`
// holds so far.
static int fork_chains(sgx_env *h, int chains, hipStream_t stream) {
    if (!h->chain_fork) HIP_TRY(hipEventCreateWithFlags(&h->chain_fork, hipEventDisableTiming));
    for (int c = 0; c < chains; ++c) {
        if (!h->chain_stream[c]) HIP_TRY(hipStreamCreateWithFlags(&h->chain_stream[c], hipStreamNonBlocking));
        if (!h->chain_join[c]) HIP_TRY(hipEventCreateWithFlags(&h->chain_join[c], hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(h->chain_fork, stream));
    for (int c = 0; c < chains; ++c) HIP_TRY(hipStreamWaitEvent(h->chain_stream[c], h->chain_fork, 0));
    return SGX_OK;
}

// Joins the chains' streams into the caller's: records every chain's join event and makes `stream` wait for it.  Returns `rc` (the
// error of the launches, which wins) or the first error of the joining itself.
static int join_chains(sgx_env *h, int chains, hipStream_t stream, int rc) {
    const std::string keep = g_last_error;
    hipError_t first = hipSuccess;
    for (int c = 0; c < chains; ++c) {
        hipError_t e = hipEventRecord(h->chain_join[c], h->chain_stream[c]);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, h->chain_join[c], 0);
        if (e != hipSuccess && first == hipSuccess) first = e;
    }
    if (rc != SGX_OK) { g_last_error = keep; return rc; }
    if (first != hipSuccess) return fail(SGX_EDEVICE, "joining the chains: %s", hipGetErrorString(first));
    return SGX_OK;
}

SGX_API int sgx_step_n(sgx_env *h, const sgx_step_io *io, int32_t n_steps, void *stream) {
    if (!h || !io) return fail(SGX_EINVAL, "handle or io is NULL%s");
    if (!io->actions_dev || io->next_actions_dev != io->actions_dev)
        return fail(SGX_EINVAL, "sgx_step_n needs next_actions_dev == actions_dev (each step plays the action the previous one drew)%s");
    if (n_steps < 0) return fail(SGX_EINVAL, "n_steps is negative%s");
    if (int rc = check_io_pointers(h, *io, "sgx_step_n")) return rc;
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    p.mode = 0;
    p.io = *io;
    return play_steps(h, p, OutSets{io, 1, false, 0, 0, 0}, 0, n_steps, stream);
}

SGX_API int sgx_step_ring(sgx_env *h, const sgx_step_io *ios, int32_t n_sets, int32_t first_set, int32_t n_steps, void *stream) {
    if (!h || !ios) return fail(SGX_EINVAL, "handle or ios is NULL%s");
    if (n_sets < 1 || first_set < 0 || first_set >= n_sets || n_steps < 0) return fail(SGX_EINVAL, "sgx_step_ring: n_sets, first_set or n_steps out of range%s");
    for (int32_t k = 0; k < n_sets; ++k) {
        if (!ios[k].actions_dev || ios[k].next_actions_dev != ios[k].actions_dev || ios[k].actions_dev != ios[0].actions_dev)
            return fail(SGX_EINVAL, "sgx_step_ring: every set needs next_actions_dev == actions_dev == the first set's (each step plays the action the previous one drew)%s");
        if (ios[k].auto_reset != ios[0].auto_reset || ios[k].flags != ios[0].flags)
            return fail(SGX_EINVAL, "sgx_step_ring: the sets differ in auto_reset or flags%s");
        if (int rc = check_io_pointers(h, ios[k], "sgx_step_ring")) return rc;
    }
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    p.mode = 0;
    return play_steps(h, p, OutSets{ios, n_sets, false, 0, 0, 0}, first_set, n_steps, stream);
}

// sgx_step_n into a trajectory buffer: slot (first_slot + t) % n_slots of tensors with a leading slot axis receives step t's outputs.
SGX_API int sgx_step_traj(sgx_env *h, const sgx_traj_io *t, int32_t first_slot, int32_t n_steps, void *stream) {
    if (!h || !t) return fail(SGX_EINVAL, "handle or t is NULL%s");
    const sgx_step_io &io = t->io;
    if (!io.actions_dev || io.next_actions_dev != io.actions_dev)
        return fail(SGX_EINVAL, "sgx_step_traj needs next_actions_dev == actions_dev (each step plays the action the previous one drew)%s");
    if (t->n_slots < 1 || first_slot < 0 || first_slot >= t->n_slots || n_steps < 0) return fail(SGX_EINVAL, "sgx_step_traj: n_slots, first_slot or n_steps out of range%s");
    if (t->slot_envs < h->n_envs) return fail(SGX_EINVAL, "sgx_step_traj: slot_envs is smaller than the number of envs%s");
    // (slot s of a tensor lies s x slot_envs games further: as aligned as slot 0 wherever slot 0 passes -- a game's float32 observation is a
    // multiple of 16 bytes on the boards that need 16, compact records are padded to 128 bytes and the bit masks to 16)
    if (int rc = check_io_pointers(h, io, "sgx_step_traj")) return rc;
    if (int rc = check_aligned("sgx_step_traj", "actions_log_dev", t->actions_log_dev, 4)) return rc;
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    p.mode = 0;
    p.io = io;
    p.traj_out_envs = t->slot_envs;
    p.traj_res_envs = t->results_per_slot ? t->slot_envs : 0;
    p.traj_act_log = t->actions_log_dev;
    // bytes between the slots of each tensor, by the layout the flags ask for
    const bool original = (io.flags & SGX_STEP_ORIGINAL_CHANNELS) != 0;
    const int64_t cells = (int64_t)h->cfg.rows * h->cfg.cols;
    const int64_t obs_env = (io.flags & SGX_STEP_COMPACT_OBS) ? compact_obs_stride(h) : cells * lut_channels(false, original) * 4;
    const int64_t mask_env = (io.flags & SGX_STEP_COMPACT_MASK) ? 4 * (int64_t)mask_words(h)
                           : (io.flags & SGX_STEP_MASK_1D)      ? cells * (h->cfg.rows + h->cfg.cols) + 1 : cells * h->K;
    const OutSets slots{&t->io, t->n_slots, true, io.obs_dev ? t->slot_envs * obs_env : 0, io.fobs_dev ? t->slot_envs * cells * lut_channels(true, original) * 4 : 0,
                        io.mask_dev ? t->slot_envs * mask_env : 0};
    return play_steps(h, p, slots, first_slot, n_steps, stream);
}

SGX_API int sgx_rollout(sgx_env *h, const sgx_step_io *io, int32_t n_steps, int32_t chains, void *stream) {
    if (!h || !io) return fail(SGX_EINVAL, "handle or io is NULL%s");
    if (!io->actions_dev || io->next_actions_dev != io->actions_dev)
        return fail(SGX_EINVAL, "sgx_rollout needs next_actions_dev == actions_dev (each step plays the action the previous one drew)%s");
    if (n_steps < 0 || chains < 0 || chains > SGX_MAX_CHAINS) return fail(SGX_EINVAL, "n_steps or chains out of range%s");
    if (int rc = check_io_pointers(h, *io, "sgx_rollout")) return rc;
    // games per chain: a multiple of what eight workgroups play, so that every chain keeps the XCD-aware map
    const int cells = h->cfg.rows * h->cfg.cols;
    // chains = 0: the measured rule (profiles/r04_variant_bench.log, 65,536 games in place): two chains gain where one launch leaves
    // the chip part empty -- boards of up to 36 cells (Micro +19 %, Tiny +4 %, 5x5 +3 %, 6x6 +5 %) and boards whose cell count is no
    // multiple of 4 (15x15 +4 %) -- and lose 2-5 % on 8x8 / 10x10, whose single launch already streams at the memory rate
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    p.mode = 0;
    p.io = *io;
    if (chains == 0) {
        // ... and since round 5 something better than chains of launches where the call is eligible: all steps in ONE launch -- boards of
        // at most 16 cells lane_steps_kernel (Micro 29 us per step against 35 with two chains), the other boards steps_kernel, faster than
        // two chains of launches on every board since its parameter reads are scalar loads (6x6: 97-99 against 101 us per step, 5x5: 71
        // against 91; profiles/r05_variant_bench.log)
        bool launched = false;
        if (int rc = multi_steps(h, p, OutSets{io, 1, false, 0, 0, 0}, 0, n_steps, stream, &launched)) return rc;
        if (launched) return SGX_OK;
        chains = (cells <= 36 || cells % 4 != 0) ? 2 : 1;
    }
    const int64_t unit = 8 * 8 * (cells <= 16 ? 4 : (cells <= 32 ? 2 : 1));     // 8 workgroups x SGX_WPB waves x Geo::GPW games
    int64_t per = (h->n_envs / chains) / unit * unit;
    if (chains == 1 || per == 0 || n_steps == 0) return sgx_step_n(h, io, n_steps, stream);
    if (int rc = fork_chains(h, chains, (hipStream_t)stream)) return rc;
    // Submission order: blocks of steps chain by chain.  (Alternating the stream with every launch costs more than the overlap
    // gains -- 65,536 Micro games: 107 us per step against 44 us with one chain; each switch of the submitting queue is a host
    // round trip.)
    const int block = 32;                                    // (4 ... 1000 measured within 3 % of each other)
    int rc = SGX_OK;
    for (int32_t i0 = 0; i0 < n_steps && rc == SGX_OK; i0 += block)
        for (int c = 0; c < chains && rc == SGX_OK; ++c) {
            KParams pc = p;
            pc.env_first = c * per;
            pc.n_envs = c == chains - 1 ? h->n_envs : (c + 1) * per;
            for (int32_t i = i0; i < n_steps && i < i0 + block && rc == SGX_OK; ++i) rc = launch_step(h, pc, (void *)h->chain_stream[c]);
        }
    // the caller's stream waits for every chain that was forked -- also when a launch failed half way: what is already enqueued still
    // writes the caller's buffers and must stay ordered before whatever the caller enqueues next
    return join_chains(h, chains, (hipStream_t)stream, rc);
}

SGX_API int64_t sgx_compact_obs_stride(const sgx_env *h) { return h ? compact_obs_stride(h) : 0; }
SGX_API int64_t sgx_compact_mask_words(const sgx_env *h) { return h ? mask_words(h) : 0; }

SGX_API int sgx_decode_obs(sgx_env *h, const uint8_t *compact_dev, float *obs_dev, void *stream) {
    if (!h || !compact_dev || !obs_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (reinterpret_cast<uintptr_t>(compact_dev) & 15) return fail(SGX_EINVAL, "sgx_decode_obs: compact_dev must be 16-byte aligned%s");
    if ((reinterpret_cast<uintptr_t>(obs_dev) & 15) && (h->cfg.rows * h->cfg.cols) % 4 == 0)
        return fail(SGX_EINVAL, "sgx_decode_obs: obs_dev must be 16-byte aligned%s");
    if (int rc = check_aligned("sgx_decode_obs", "obs_dev", obs_dev, 4)) return rc;
    SGX_ON_DEVICE(h->device);
    const int nt = nt_for(h, h->n_envs * (int64_t)h->cfg.rows * h->cfg.cols * OBS_CH * 4);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            using G = Geo<R, C>;
            const unsigned grid = (unsigned)((h->n_envs + G::WPB * G::GPW - 1) / (G::WPB * G::GPW));
            decode_obs_kernel<R, C><<<grid, 64 * G::WPB, 0, (hipStream_t)stream>>>(compact_dev, compact_obs_stride(h), compact_capacity(h), obs_dev, h->n_envs, nt);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

SGX_API int sgx_decode_mask(sgx_env *h, const uint32_t *bits_dev, uint8_t *mask_dev, void *stream) {
    if (!h || !bits_dev || !mask_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (reinterpret_cast<uintptr_t>(bits_dev) & 15) return fail(SGX_EINVAL, "sgx_decode_mask: bits_dev must be 16-byte aligned%s");
    SGX_ON_DEVICE(h->device);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            using G = Geo<R, C>;
            const unsigned grid = (unsigned)((h->n_envs + G::WPB * G::GPW - 1) / (G::WPB * G::GPW));
            decode_mask_kernel<R, C><<<grid, 64 * G::WPB, 0, (hipStream_t)stream>>>(bits_dev, mask_dev, h->n_envs);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

SGX_API int sgx_sample_valid(sgx_env *h, const uint8_t *mask_dev, int32_t *actions_dev, void *stream) {
    if (!h || !mask_dev || !actions_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (int rc = check_aligned("sgx_sample_valid", "actions_dev", actions_dev, 4)) return rc;
    SGX_ON_DEVICE(h->device);
    KParams p = make_params(h);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            sample_kernel<decltype(r)::value, decltype(c)::value><<<(unsigned)h->n_envs, 64, 0, (hipStream_t)stream>>>(p, mask_dev, actions_dev);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

// The chooser of the reference's game loop for a batch (loop:6-31, examples/util.py:4-47): masked softmax over caller logits, one sample per game.
SGX_API int sgx_choose_actions(sgx_env *h, const float *logits_dev, const void *mask_dev, float temperature, int32_t flags, int32_t *actions_dev, void *stream) {
    if (!h || !logits_dev || !mask_dev || !actions_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (!(temperature >= 0.f) || temperature > 3.0e38f) return fail(SGX_EINVAL, "sgx_choose_actions: temperature must be finite and >= 0 (0 = argmax)%s");
    if (flags & ~SGX_STEP_COMPACT_MASK) return fail(SGX_EINVAL, "sgx_choose_actions: the only flag is SGX_STEP_COMPACT_MASK%s");
    const bool bits = (flags & SGX_STEP_COMPACT_MASK) != 0;
    if ((reinterpret_cast<uintptr_t>(logits_dev) & 3) || (bits && (reinterpret_cast<uintptr_t>(mask_dev) & 3)))
        return fail(SGX_EINVAL, "sgx_choose_actions: logits_dev (and a compact mask_dev) must be 4-byte aligned%s");
    if (int rc = check_aligned("sgx_choose_actions", "actions_dev", actions_dev, 4)) return rc;
    SGX_ON_DEVICE(h->device);
    const KParams p = make_params(h);
    const float scale = temperature == 0.f ? __builtin_inff() : 1.4426950408889634f / temperature;     // (+inf: every weight below the maximum's is 0)
    const int64_t na = (int64_t)h->cfg.rows * h->cfg.cols * h->K;
    // rows of 4 actions per lane where every game's logits start on a 16-byte and its mask on a 4-byte boundary
    const bool vec4 = na % 4 == 0 && !(reinterpret_cast<uintptr_t>(logits_dev) & 15) && !(reinterpret_cast<uintptr_t>(mask_dev) & 3);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            auto launch = [&](auto vec, auto bits_c) {
                constexpr int V = decltype(vec)::value;
                constexpr bool B = decltype(bits_c)::value;
                using CG = ChooseGeo<Geo<R, C>, V>;
                choose_kernel<R, C, V, B><<<(unsigned)((h->n_envs + CG::GAMES - 1) / CG::GAMES), 64 * CG::WAVES, 0, (hipStream_t)stream>>>(
                    p, logits_dev, mask_dev, scale, actions_dev);
            };
            auto with_bits = [&](auto vec) {
                if (bits) launch(vec, bool_c<true>());
                else launch(vec, bool_c<false>());
            };
            if constexpr (Geo<R, C>::NA % 4 == 0) {
                if (vec4) return with_bits(int_c<4>());
            }
            with_bits(int_c<1>());
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

namespace {
// export / import of the envs [p.env_first, p.n_envs) of the handle
// one state per workgroup, mapped onto the XCDs like the step's workgroups (group_of_block): contiguous ranges of states per XCD
// (tools/states_ab.py, 65,536 Barrage states through sgx_step_states: 689 us against 736 us with the linear map; these kernels read as
// much as they write and the odd / even skew of the write-only step does not pay here: 697 us at 100 per mille, 702 at 150)
unsigned state_grid(const sgx_env *h, KParams &p) {
    int32_t w[8];
    launch_shares(h, false, w);
    p.map_mode = h->map_mode; p.map_arg = h->map_arg;
    return shares_for(p, p.n_envs - p.env_first, w);
}
// bytes of the batch's int64 states
int64_t state_bytes(const sgx_env *h) { return h->n_envs * (int64_t)SGX_STATE_LAYERS * h->cfg.rows * h->cfg.cols * 8; }
int launch_export(sgx_env *h, const KParams &p_in, int64_t *state_dev, int8_t *player_dev, hipStream_t stream) {
    // (the int64 layout is 27 KB per 10x10 state: past the Infinity Cache the layers leave as non-temporal stores, like the observations)
    const int nt = nt_for(h, state_bytes(h));
    KParams p = p_in;
    const unsigned grid = state_grid(h, p);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            export_kernel<decltype(r)::value, decltype(c)::value><<<grid, 256, 0, stream>>>(p, state_dev, player_dev, nt);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}
int launch_import(sgx_env *h, const KParams &p_in, const int64_t *state_dev, const int8_t *player_dev, uint8_t *sanitised_dev, hipStream_t stream) {
    KParams p = p_in;
    const unsigned grid = state_grid(h, p);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            import_kernel<decltype(r)::value, decltype(c)::value><<<grid, 256, 0, stream>>>(p, state_dev, player_dev, sanitised_dev);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}
}  // namespace

SGX_API int sgx_export_state(sgx_env *h, int64_t *state_dev, int8_t *player_dev, void *stream) {
    if (!h || !state_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (int rc = check_aligned("sgx_export_state", "state_dev", state_dev, 16)) return rc;
    SGX_ON_DEVICE(h->device);
    return launch_export(h, make_params(h), state_dev, player_dev, (hipStream_t)stream);
}

SGX_API int sgx_import_state_checked(sgx_env *h, const int64_t *state_dev, const int8_t *player_dev, uint8_t *sanitised_dev, void *stream) {
    if (!h || !state_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (int rc = check_aligned("sgx_import_state", "state_dev", state_dev, 16)) return rc;
    SGX_ON_DEVICE(h->device);
    return launch_import(h, make_params(h), state_dev, player_dev, sanitised_dev, (hipStream_t)stream);
}

namespace {
// sgx_step_states' list of the states its first pass had to alter: created on first use, emptied (on the caller's stream) before every
// first pass; p.flag_list / p.flag_count make the imports of that pass append to it
int redo_list_reset(sgx_env *h, KParams &p, hipStream_t stream) {
    if (!h->redo_list) HIP_TRY(hipMalloc((void **)&h->redo_list, ((size_t)h->n_envs + 1) * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(h->redo_list + h->n_envs, 0, sizeof(int32_t), stream));
    p.flag_list = h->redo_list;
    p.flag_count = h->redo_list + h->n_envs;
    return SGX_OK;
}
// the general-state pass: a small persistent grid that walks the list
unsigned redo_grid(const sgx_env *h) { return (unsigned)(h->n_envs < 2048 ? h->n_envs : 2048); }
// f(bool_c<MAPPED>, bool_c<OBS>): the states_kernel instantiation of sgx_step_states' outputs (state-coordinate masks, an observation)
template <class F>
void with_states_io(bool mapped, bool obs, F &&f) {
    if (mapped && obs) f(bool_c<true>(), bool_c<true>());
    else if (mapped) f(bool_c<true>(), bool_c<false>());
    else if (obs) f(bool_c<false>(), bool_c<true>());
    else f(bool_c<false>(), bool_c<false>());
}
}  // namespace

// get_next_state (penv:148-155) and friends on caller-provided int64 states in ONE call: import -> step -> export, the batch split
// into `chains` ranges of states that run on streams of their own, so that one range's reads overlap another's writes.
SGX_API int sgx_step_states(sgx_env *h, const int64_t *state_in_dev, const int8_t *player_in_dev, uint8_t *sanitised_dev,
                            const sgx_step_io *io, int64_t *state_out_dev, int8_t *player_out_dev, int32_t chains, void *stream) {
    if (!h || !state_in_dev || !io) return fail(SGX_EINVAL, "NULL argument%s");
    if (io->auto_reset || io->next_actions_dev) return fail(SGX_EINVAL, "sgx_step_states: no auto_reset, no sampled next actions%s");
    if (io->flags & (SGX_STEP_COMPACT_OBS | SGX_STEP_COMPACT_MASK)) return fail(SGX_EINVAL, "sgx_step_states: no compact outputs%s");
    if (chains < 1 || chains > SGX_MAX_CHAINS) return fail(SGX_EINVAL, "chains out of range%s");
    if (int rc = check_io_pointers(h, *io, "sgx_step_states")) return rc;
    if (int rc = check_aligned("sgx_step_states", "state_in_dev", state_in_dev, 16)) return rc;      // (16-byte loads / stores of the int64 layers)
    if (int rc = check_aligned("sgx_step_states", "state_out_dev", state_out_dev, 16)) return rc;
    const int cells = h->cfg.rows * h->cfg.cols;
    const bool kind0 = !io->fobs_dev && !io->final_fobs_dev && !(io->flags & SGX_STEP_ORIGINAL_CHANNELS);
    const bool mapped = (io->flags & (SGX_STEP_MASK_1D | SGX_STEP_MASK_STATE_COORDS)) != 0;
    const bool obs = io->obs_dev || io->final_obs_dev;
    // one-game-per-wave boards, partial-observation kinds: ONE fused launch, the record never leaves LDS between the three steps
    const bool fused = kind0 && cells > 32 && cells <= 256;
    // Second pass (sgx_set_general_states, on by default): the states the first pass had to alter -- more than two recent-move cells per
    // player, more capture cells than pieces, more than 8 captures on a cell: things play cannot produce but penv's pure functions
    // accept -- are redone from the caller's int64 input on the general-state variant of the geometry (Geo<R, C, 1>); every other
    // block of that launch leaves at once.  Not: boards of more than 256 cells; state-coordinate masks together with another observation
    // kind (which the fused path does not take).
    const bool general = h->general_states != 0 && cells <= 256 && (kind0 || !mapped);
    auto overlap = [](const void *a, int64_t na, const void *b, int64_t nb) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
        return a && b && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
    };
    const bool states_overlap = overlap(state_in_dev, state_bytes(h), state_out_dev, state_bytes(h));
    const bool players_overlap = overlap(player_in_dev, h->n_envs, player_out_dev, h->n_envs);
    if (general) {
        // The general-state pass re-reads the caller's INPUT after the first pass has written the outputs: a state stepped in place would
        // be redone from its own successor (stepped twice, or judged invalid) without anybody noticing.
        if (states_overlap || players_overlap)
            return fail(SGX_EINVAL, "sgx_step_states: state_out_dev / player_out_dev overlap the inputs, which the general-state pass reads again "
                                    "after the outputs are written; pass distinct buffers or switch the pass off (sgx_set_general_states(h, 0))%s");
    } else {
        // No second pass: a batch may be stepped IN PLACE (state_out_dev == state_in_dev, player_out_dev == player_in_dev: the workgroup of
        // state i reads state i completely before it writes its successor, and touches no other state).  Any other overlap -- outputs
        // shifted by some states against the inputs -- makes one workgroup write what another one has yet to read.
        if ((states_overlap && state_out_dev != state_in_dev) || (players_overlap && player_out_dev != player_in_dev))
            return fail(SGX_EINVAL, "sgx_step_states: state_out_dev / player_out_dev overlap the inputs without being the same pointers "
                                    "(in place is fine with the general-state pass off; a shifted overlap races between workgroups)%s");
    }
    SGX_ON_DEVICE(h->device);
    const int64_t unit = 64;
    int64_t per = (h->n_envs / chains) / unit * unit;
    if (per == 0) chains = 1;
    KParams p = make_params(h);
    p.mode = io->actions_dev ? 0 : 1;        // no actions: observe -- masks / observations of the given states, nothing is played
    p.io = *io;
    if (h->pool && p.mode == 0 && io->auto_reset)
        return fail(SGX_EINVAL, "sgx_step_states does not auto-reset on a handle with a start pool (its states are the caller's)%s");
    if (int rc = check_step_io(h, p)) return rc;
    // the general-state pass needs the flags even when the caller did not ask for them
    uint8_t *flags_dev = sanitised_dev;
    if (general && !flags_dev) {
        if (!h->san_flags) HIP_TRY(hipMalloc((void **)&h->san_flags, (size_t)h->n_envs));
        flags_dev = h->san_flags;
    }
    if (general)
        if (int rc = redo_list_reset(h, p, (hipStream_t)stream)) return rc;       // (before the chains fork: their imports append to the list)
    int32_t *const redo_count = h->redo_list ? h->redo_list + h->n_envs : nullptr;
    const int nt = nt_for(h, state_bytes(h));
    const hipStream_t st = (hipStream_t)stream;
    if (fused) {
        const unsigned grid = state_grid(h, p), grid_big = redo_grid(h);
        p.nt_stores = nt_for(h, launch_obs_bytes(h, p));
        KParams pbig = p;                                   // the general-state pass appends nothing
        pbig.flag_list = pbig.flag_count = nullptr;
        auto pass = [&](auto var) {
            constexpr int VAR = decltype(var)::value;
            return for_geometry(h, [&](auto r, auto c) {
                constexpr int R = decltype(r)::value, C = decltype(c)::value;
                if constexpr (Geo<R, C>::LPG == 64 && !Geo<R, C>::WIDE)
                    with_states_io(mapped, obs, [&](auto m, auto o) {
                        constexpr bool M = decltype(m)::value, O = decltype(o)::value;
                        states_kernel<R, C, M, O, VAR><<<VAR ? grid_big : grid, states_threads<M, O>(), 0, st>>>(
                            VAR ? pbig : p, state_in_dev, player_in_dev, flags_dev, state_out_dev, player_out_dev, nt, h->redo_list, redo_count);
                    });
            });
        };
        if (int rc = pass(int_c<0>())) return rc;
        HIP_TRY(hipGetLastError());
        if (general) {
            if (int rc = pass(int_c<1>())) return rc;
            HIP_TRY(hipGetLastError());
        }
        return SGX_OK;
    }
    // What the fused path above does not cover takes the three-launch path on packed records -- boards of up to 32 cells (several games per
    // wave) and the other observation kinds (79-channel, 'original' channels).  States the packed records cannot carry are then redone,
    // like above, by the general-state variant of the fused kernel, which is one game per wave on every board and takes the observation
    // kind as a parameter.
    auto second_pass = [&]() -> int {
        if (!general) return SGX_OK;
        KParams q = p;
        q.env_first = 0;
        q.n_envs = h->n_envs;
        q.flag_list = q.flag_count = nullptr;
        const unsigned grid = redo_grid(h);
        q.nt_stores = nt_for(h, launch_obs_bytes(h, q));
        const int kindx = ((io->fobs_dev || io->final_fobs_dev) ? 1 : 0) | ((io->flags & SGX_STEP_ORIGINAL_CHANNELS) ? 2 : 0);
        if (int rc = for_geometry(h, [&](auto r, auto c) {
                constexpr int R = decltype(r)::value, C = decltype(c)::value;
                if constexpr (!Geo<R, C>::WIDE) {
                    auto kind_pass = [&](auto kx) {
                        states_kernel<R, C, false, true, 1, decltype(kx)::value><<<grid, states_threads<false, true>(), 0, st>>>(
                            q, state_in_dev, player_in_dev, flags_dev, state_out_dev, player_out_dev, nt, h->redo_list, redo_count);
                    };
                    if (kindx == 1) kind_pass(int_c<1>());
                    else if (kindx == 2) kind_pass(int_c<2>());
                    else if (kindx == 3) kind_pass(int_c<3>());
                    else if constexpr (Geo<R, C>::LPG != 64)
                        with_states_io(mapped, obs, [&](auto m, auto o) {
                            constexpr bool M = decltype(m)::value, O = decltype(o)::value;
                            states_kernel<R, C, M, O, 1><<<grid, states_threads<M, O>(), 0, st>>>(
                                q, state_in_dev, player_in_dev, flags_dev, state_out_dev, player_out_dev, nt, h->redo_list, redo_count);
                        });
                }
            })) return rc;
        HIP_TRY(hipGetLastError());
        return SGX_OK;
    };
    if (chains == 1) {
        if (int rc = launch_import(h, p, state_in_dev, player_in_dev, flags_dev, st)) return rc;
        if (int rc = launch_step(h, p, stream, 1, 0, false)) return rc;      // (caller-provided states: no game starts here, no pool kernels)
        if (state_out_dev)
            if (int rc = launch_export(h, p, state_out_dev, player_out_dev, st)) return rc;
        return second_pass();
    }
    if (int rc = fork_chains(h, chains, st)) return rc;
    int rc = SGX_OK;
    for (int c = 0; c < chains && rc == SGX_OK; ++c) {
        KParams pc = p;
        pc.env_first = c * per;
        pc.n_envs = c == chains - 1 ? h->n_envs : (c + 1) * per;
        rc = launch_import(h, pc, state_in_dev, player_in_dev, flags_dev, h->chain_stream[c]);
        if (rc == SGX_OK) rc = launch_step(h, pc, (void *)h->chain_stream[c], 1, 0, false);
        if (rc == SGX_OK && state_out_dev) rc = launch_export(h, pc, state_out_dev, player_out_dev, h->chain_stream[c]);
    }
    rc = join_chains(h, chains, st, rc);     // (also after a failed launch: see sgx_rollout)
    return rc != SGX_OK ? rc : second_pass();
}

SGX_API int sgx_import_state(sgx_env *h, const int64_t *state_dev, const int8_t *player_dev, void *stream) {
    return sgx_import_state_checked(h, state_dev, player_dev, nullptr, stream);
}

namespace {
int same_variant(const sgx_env *a, const sgx_env *b) {
    if (a->device != b->device) return fail(SGX_EINVAL, "the two handles live on different devices%s");
    if (memcmp(&a->cfg, &b->cfg, sizeof(sgx_config)) != 0 || a->rec_bytes != b->rec_bytes)
        return fail(SGX_EINVAL, "the two handles were created for different variants%s");
    return SGX_OK;
}
}  // namespace

SGX_API int sgx_copy_envs(sgx_env *dst, const int32_t *dst_index_dev, sgx_env *src, const int32_t *src_index_dev, int64_t n, void *stream) {
    if (!dst || !src) return fail(SGX_EINVAL, "handle is NULL%s");
    if (int rc = same_variant(dst, src)) return rc;
    if (n < 0 || (!dst_index_dev && n > dst->n_envs) || (!src_index_dev && n > src->n_envs)) return fail(SGX_EINVAL, "n out of range%s");
    // (with both index arrays nothing else bounds n: the grid is a 32-bit count of (n + 3) / 4 workgroups)
    if (n > 0x7fffffff) return fail(SGX_EINVAL, "sgx_copy_envs: n must be in [0, 2^31)%s");
    // inside one pool a wave may read a record another wave of the same launch rewrites: only the identity copy is race-free
    if (dst == src && (dst_index_dev || src_index_dev))
        return fail(SGX_EINVAL, "sgx_copy_envs: an indexed copy inside one handle would race; stage through a second handle%s");
    if (n == 0 || dst == src) return SGX_OK;
    if (int rc = check_aligned("sgx_copy_envs", "dst_index_dev", dst_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_copy_envs", "src_index_dev", src_index_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    copy_records_kernel<<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(dst->boards, dst_index_dev, src->boards, src_index_dev, dst->rec_bytes, n);
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

namespace {
// Where the roots of a pool-to-pool call come from (sgx_expand, sgx_determinize, sgx_playout, sgx_replay, sgx_expand_all): slot i of the
// launch reads record src_index[i] (i when NULL) of src, so src is dst's variant on dst's device and, without an index, has the `needed`
// (`needed_name`) records.  Inside one pool a wave would read a record that another wave of the same launch rewrites -- through an index (a
// gather or a permutation) that silently mixes roots and results; the identity call is safe where slot i is written from record i alone (a
// wave holds its whole record in LDS before it writes): `in_place_ok`.
int check_root_source(const char *fn, const sgx_env *dst, const sgx_env *src, const int32_t *src_index_dev, int64_t needed, const char *needed_name, bool in_place_ok = true) {
    auto refuse = [&](const char *what) { return fail(SGX_EINVAL, "%s", (std::string(fn) + ": " + what).c_str()); };
    if (same_variant(dst, src) != SGX_OK) return refuse(g_last_error.c_str());
    if (!src_index_dev && src->n_envs < needed) return refuse((std::string("without src_index_dev the source handle needs at least as many envs as ") + needed_name).c_str());
    if (src == dst && !in_place_ok) return refuse("src == dst (the results would overwrite the roots); use a second handle as dst");
    if (src == dst && src_index_dev) return refuse("src == dst with an index array would race; use a second handle as dst");
    return SGX_OK;
}
// The kernels that play from a record into dst's pool never restart a game
int refuse_start_pool(const char *fn, const sgx_env *dst) {
    if (!dst->pool) return SGX_OK;
    return fail(SGX_EINVAL, "%s", (std::string(fn) + ": dst has a start pool set (this call never restarts a game); clear it or use another handle as dst").c_str());
}

// The KParams of a pool-to-pool launch: dst's, the roots from src (io all NULL / 0: spatial actions in the mover's perspective, no
// auto-reset, no per-step output)
KParams pool_params(const sgx_env *dst, const sgx_env *src, const int32_t *src_index_dev, int mode) {
    KParams p = make_params(dst);
    p.mode = mode;
    p.src_boards = src->boards;
    p.src_index = src_index_dev;
    return p;
}
template <class IO>
ResultOut result_out(const IO &io) { return ResultOut{io.reward_dev, io.done_dev, io.ending_invalid_dev, io.player_dev}; }

// One launch of a pool-to-pool kernel (sgx_pool_frame.h) over sp.k's envs: the geometry of the logic-only launches.  K names the kernel
// template: K::kernel<R, C, VAR>() is the instantiation.
// (LEAF: the instantiation that evaluates positions that are not over, launched when dst has leaf values set -- launch_leaf_or_plain)
template <bool LEAF> struct PlayoutK { template <int R, int C, int VAR> static auto kernel() { return &playout_kernel<R, C, VAR, LEAF>; } };
template <bool LEAF> struct WeightedPlayoutK { template <int R, int C, int VAR> static auto kernel() { return &playout_weighted_kernel<R, C, VAR, LEAF>; } };
template <bool LEAF> struct ReplayK { template <int R, int C, int VAR> static auto kernel() { return &replay_kernel<R, C, VAR, LEAF>; } };
template <bool LEAF> struct ReplayTrackedK { template <int R, int C, int VAR> static auto kernel() { return &replay_kernel<R, C, VAR, LEAF, true>; } };
struct CountK { template <int R, int C, int VAR> static auto kernel() { return &count_kernel<R, C, VAR>; } };
template <bool LEAF> struct ChildrenK { template <int R, int C, int VAR> static auto kernel() { return &children_kernel<R, C, VAR, LEAF>; } };
template <class K, class SP>
int launch_pool_kernel(const sgx_env *h, SP &sp, void *stream) {
    int32_t w[8];
    launch_setup(h, sp.k, 1, w);
    if (int rc = for_geometry(h, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            with_half_wave<R, C, 8>(h, [&](auto var) {
                constexpr int VAR = decltype(var)::value;
                using G = Geo<R, C, VAR>;
                const unsigned grid = geo_grid<G>(sp.k, w);
                K::template kernel<R, C, VAR>()<<<grid, 64 * G::WPB, 0, (hipStream_t)stream>>>(sp);
            });
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

// A launch of one of the four kernels that end in store_results, for dst: with leaf values set (sgx_set_leaf_values) the table travels in the
// launch's parameters and the LEAF instantiation runs; without, the parameters' leaf block stays zero and the plain instantiation runs.
template <template <bool> class K, class SP>
int launch_leaf_or_plain(const sgx_env *dst, SP &sp, void *stream) {
    if (!dst->leaf_table) return launch_pool_kernel<K<false>>(dst, sp, stream);
    sp.leaf = LeafParams{dst->leaf_table, dst->leaf_limit, dst->leaf_denom, dst->leaf_see_all, 0};
    return launch_pool_kernel<K<true>>(dst, sp, stream);
}

// handle scratch of at least `elems` elements (hipFree waits for the launches that still read the old one)
template <class T>
int grow_scratch(T **buf, int64_t *cap, int64_t elems) {
    if (*cap >= elems) return SGX_OK;
    if (*buf) { HIP_TRY(hipFree(*buf)); *buf = nullptr; *cap = 0; }
    const int64_t want = elems + elems / 2;
    HIP_TRY(hipMalloc((void **)buf, (size_t)want * sizeof(T)));
    *cap = want;
    return SGX_OK;
}
}  // namespace

SGX_API int sgx_expand(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_step_io *io, void *stream) {
    if (!dst || !src || !io) return fail(SGX_EINVAL, "handle or io is NULL%s");
    if (!io->actions_dev) return fail(SGX_EINVAL, "actions_dev is NULL%s");
    if (int rc = check_root_source("sgx_expand", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    if (io->auto_reset) return fail(SGX_EINVAL, "sgx_expand does not auto-reset%s");
    if (io->fobs_dev || io->final_fobs_dev || (io->flags & SGX_STEP_ORIGINAL_CHANNELS))
        return fail(SGX_EINVAL, "sgx_expand renders the 67-channel partial observation only%s");
    if (int rc = check_io_pointers(dst, *io, "sgx_expand")) return rc;
    if (int rc = check_aligned("sgx_expand", "src_index_dev", src_index_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    KParams p = pool_params(dst, src, src_index_dev, 0);
    p.io = *io;
    return launch_step(dst, p, stream);
}

SGX_API int sgx_determinize(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, int32_t observer, uint64_t draw, int32_t *hidden_dev, void *stream) {
    if (!dst || !src) return fail(SGX_EINVAL, "handle is NULL%s");
    if (int rc = check_root_source("sgx_determinize", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    if (observer < -1 || observer > 1) return fail(SGX_EINVAL, "sgx_determinize: observer must be 0 (each record's mover), +1 or -1%s");
    if (int rc = check_aligned("sgx_determinize", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_determinize", "hidden_dev", hidden_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    const int cells = dst->cfg.rows * dst->cfg.cols, S = (cells + 3) & ~3, sb = (((cells + 7) / 8) + 15) & ~15;
    determinize_kernel<<<(unsigned)((dst->n_envs + 3) / 4), 256, 4 * det_lds_bytes(dst->rec_bytes, cells), (hipStream_t)stream>>>(
        dst->boards, src->boards, src_index_dev, hidden_dev, dst->n_envs, dst->seed, dst->env_id_offset, draw, observer, S, dst->sc_off - 2 * sb, sb,
        dst->sc_off, dst->rec_bytes, cells);
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

SGX_API int sgx_determinize_weighted(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, int32_t observer, const uint16_t *belief_dev,
                                     int64_t belief_stride, uint64_t draw, int32_t *hidden_dev, int32_t *off_belief_dev, void *stream) {
    if (!dst || !src) return fail(SGX_EINVAL, "sgx_determinize_weighted: handle is NULL%s");
    if (int rc = check_root_source("sgx_determinize_weighted", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    if (observer < -1 || observer > 1) return fail(SGX_EINVAL, "sgx_determinize_weighted: observer must be 0 (each record's mover), +1 or -1%s");
    if (!belief_dev) return fail(SGX_EINVAL, "sgx_determinize_weighted: belief_dev is NULL%s");
    const int cells = dst->cfg.rows * dst->cfg.cols, S = (cells + 3) & ~3, sb = (((cells + 7) / 8) + 15) & ~15;
    const int64_t table = 2 * (int64_t)DETW_TYPES * cells;
    if (belief_stride < 0 || (belief_stride & 1) || (belief_stride > 0 && belief_stride < table))
        return fail(SGX_EINVAL, "%s", ("sgx_determinize_weighted: belief_stride must be 0 (one table for all records) or an even number of uint16 elements of at least 2 * 12 * cells = " +
                                       std::to_string(table) + " (got " + std::to_string(belief_stride) + ")").c_str());
    if (int rc = check_aligned("sgx_determinize_weighted", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_determinize_weighted", "belief_dev", belief_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_determinize_weighted", "hidden_dev", hidden_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_determinize_weighted", "off_belief_dev", off_belief_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    determinize_weighted_kernel<<<(unsigned)((dst->n_envs + 3) / 4), 256, 4 * detw_lds_bytes(dst->rec_bytes, cells), (hipStream_t)stream>>>(
        dst->boards, src->boards, src_index_dev, belief_dev, belief_stride, hidden_dev, off_belief_dev, dst->n_envs, dst->seed, dst->env_id_offset, draw,
        observer, S, dst->sc_off - 2 * sb, sb, dst->sc_off, dst->rec_bytes, cells);
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

SGX_API int sgx_playout(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_playout_io *io, uint64_t draw, void *stream) {
    if (!dst || !src || !io) return fail(SGX_EINVAL, "sgx_playout: handle or io is NULL%s");
    if (int rc = check_root_source("sgx_playout", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    if (io->max_steps < 0) return fail(SGX_EINVAL, "sgx_playout: max_steps must be 0 (to the end of the game) or the most moves to play%s");
    if (io->flags != 0) return fail(SGX_EINVAL, "sgx_playout: flags must be 0%s");
    if (int rc = refuse_start_pool("sgx_playout", dst)) return rc;
    if (int rc = check_aligned("sgx_playout", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_playout", "reward_dev", io->reward_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_playout", "length_dev", io->length_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    PlayoutParams sp{pool_params(dst, src, src_index_dev, 0), PlayParams{draw, result_out(*io), io->length_dev, io->max_steps}};
    if (int rc = launch_leaf_or_plain<PlayoutK>(dst, sp, stream)) return rc;
    dst->last_kind = SGX_LAUNCH_PLAYOUT;
    return SGX_OK;
}

SGX_API int sgx_playout_weighted(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_playout_io *io, const uint16_t *weights, int32_t policy_flags,
                                 uint64_t draw, void *stream) {
    // the policy first: what can be said about it needs no handle
    if (!weights) return fail(SGX_EINVAL, "sgx_playout_weighted: weights is NULL%s");
    for (int i = 0; i < WT_ENTRIES; ++i)
        if (weights[i] > SGX_PLAYOUT_WEIGHT_MAX)
            return fail(SGX_EINVAL, "%s", ("sgx_playout_weighted: weights[" + std::to_string(i / (WT_TYPES * WT_TARGETS)) + "][" + std::to_string(i / WT_TARGETS % WT_TYPES) +
                                           "][" + std::to_string(i % WT_TARGETS) + "] = " + std::to_string((int)weights[i]) + " exceeds " +
                                           std::to_string(SGX_PLAYOUT_WEIGHT_MAX)).c_str());
    if (policy_flags & ~SGX_PLAYOUT_SEE_ALL) return fail(SGX_EINVAL, "sgx_playout_weighted: unknown policy_flags bits%s");
    if (!dst || !src || !io) return fail(SGX_EINVAL, "sgx_playout_weighted: handle or io is NULL%s");
    if (int rc = check_root_source("sgx_playout_weighted", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    if (io->max_steps < 0) return fail(SGX_EINVAL, "sgx_playout_weighted: max_steps must be 0 (to the end of the game) or the most moves to play%s");
    if (io->flags != 0) return fail(SGX_EINVAL, "sgx_playout_weighted: flags must be 0%s");
    if (int rc = refuse_start_pool("sgx_playout_weighted", dst)) return rc;
    if (int rc = check_aligned("sgx_playout_weighted", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_playout_weighted", "reward_dev", io->reward_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_playout_weighted", "length_dev", io->length_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    WeightedPlayoutParams sp{pool_params(dst, src, src_index_dev, 0), PlayParams{draw, result_out(*io), io->length_dev, io->max_steps},
                             (policy_flags & SGX_PLAYOUT_SEE_ALL) ? 1 : 0, 0, {}};
    memcpy(sp.weights, weights, sizeof(sp.weights));       // the table leaves with the launch's arguments: the caller's copy is free again
    if (int rc = launch_leaf_or_plain<WeightedPlayoutK>(dst, sp, stream)) return rc;
    dst->last_kind = SGX_LAUNCH_PLAYOUT_WEIGHTED;
    return SGX_OK;
}

namespace {
struct StepVsK { template <int R, int C, int VAR> static auto kernel() { return &step_vs_kernel<R, C, VAR>; } };
}  // namespace

SGX_API int sgx_step_vs(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_vs_io *io, const uint16_t *weights, uint64_t draw, void *stream) {
    // the policy first, as in sgx_playout_weighted: what can be said about it needs no handle
    if (!weights) return fail(SGX_EINVAL, "sgx_step_vs: weights is NULL%s");
    for (int i = 0; i < WT_ENTRIES; ++i)
        if (weights[i] > SGX_PLAYOUT_WEIGHT_MAX)
            return fail(SGX_EINVAL, "%s", ("sgx_step_vs: weights[" + std::to_string(i / (WT_TYPES * WT_TARGETS)) + "][" + std::to_string(i / WT_TARGETS % WT_TYPES) + "][" +
                                           std::to_string(i % WT_TARGETS) + "] = " + std::to_string((int)weights[i]) + " exceeds " + std::to_string(SGX_PLAYOUT_WEIGHT_MAX)).c_str());
    if (!dst || !src || !io) return fail(SGX_EINVAL, "sgx_step_vs: handle or io is NULL%s");
    if (io->flags & ~SGX_VS_SEE_ALL) return fail(SGX_EINVAL, "sgx_step_vs: unknown flags bits%s");
    if (!io->agent_dev && io->agent != 1 && io->agent != -1) return fail(SGX_EINVAL, "sgx_step_vs: agent must be +1 or -1 when agent_dev is NULL%s");
    if (int rc = check_root_source("sgx_step_vs", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    // (a dst with a start pool is accepted: the call never restarts a game and writes no start index, restarts are the caller's sgx_reset)
    if (int rc = check_aligned("sgx_step_vs", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_step_vs", "actions_dev", io->actions_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_step_vs", "reward_dev", io->reward_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_step_vs", "reply_action_dev", io->reply_action_dev, 4)) return rc;
    SGX_ON_DEVICE(dst->device);
    StepVsParams sp{pool_params(dst, src, src_index_dev, 0), PlayParams{draw, result_out(*io), nullptr, 0},
                    VsArgs{io->actions_dev, io->agent_dev, io->invalid_action_dev, io->moved_dev, io->reply_action_dev, io->agent_dev ? 1 : io->agent,
                           (io->flags & SGX_VS_SEE_ALL) ? 1 : 0},
                    {}};
    memcpy(sp.weights, weights, sizeof(sp.weights));       // the table leaves with the launch's arguments: the caller's copy is free again
    if (int rc = launch_pool_kernel<StepVsK>(dst, sp, stream)) return rc;
    dst->last_kind = SGX_LAUNCH_STEP_VS;
    return SGX_OK;
}

SGX_API int sgx_replay(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_replay_io *io, void *stream) {
    if (!dst || !src || !io) return fail(SGX_EINVAL, "sgx_replay: handle or io is NULL%s");
    if (int rc = check_root_source("sgx_replay", dst, src, src_index_dev, dst->n_envs, "dst")) return rc;
    if (io->max_len < 0) return fail(SGX_EINVAL, "sgx_replay: max_len must not be negative%s");
    if (io->flags & ~(SGX_REPLAY_SKIP_INVALID | SGX_REPLAY_ACTIONS_1D | SGX_REPLAY_ALLOW_OSCILLATION)) return fail(SGX_EINVAL, "sgx_replay: unknown flag bits%s");
    if (io->game_stride < 0 || io->step_stride < 0) return fail(SGX_EINVAL, "sgx_replay: game_stride and step_stride must not be negative%s");
    if (io->max_len > 0) {
        if (!io->actions_dev) return fail(SGX_EINVAL, "sgx_replay: actions_dev is NULL with max_len > 0%s");
        // the last index the kernel may read, (N - 1) * game_stride + (max_len - 1) * step_stride, against what the caller says is addressable
        // (128-bit arithmetic: two int64 products)
        const __int128 last = (__int128)(dst->n_envs - 1) * io->game_stride + (__int128)(io->max_len - 1) * io->step_stride;
        if (last >= (__int128)io->actions_elems)
            return fail(SGX_EINVAL, "sgx_replay: (N - 1) * game_stride + (max_len - 1) * step_stride reaches past actions_elems%s");
    }
    if (int rc = refuse_start_pool("sgx_replay", dst)) return rc;
    if (int rc = check_aligned("sgx_replay", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_replay", "actions_dev", io->actions_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_replay", "lengths_dev", io->lengths_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_replay", "applied_dev", io->applied_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_replay", "consumed_dev", io->consumed_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_replay", "reward_dev", io->reward_dev, 4)) return rc;
    if (dst->origin_out && dst->origin_in) {
        // piece origins (sgx_set_replay_origins): a game's labels are read whole before they are written, as its record is -- so the one
        // legal overlap of the two tensors is slot i reading what slot i writes
        const int64_t per = 2 * (int64_t)dst->cfg.rows * dst->cfg.cols;
        const int16_t *in0 = dst->origin_in, *in1 = in0 + src->n_envs * per, *out0 = dst->origin_out, *out1 = out0 + dst->n_envs * per;
        const bool overlap = (uintptr_t)in0 < (uintptr_t)out1 && (uintptr_t)out0 < (uintptr_t)in1;
        if (overlap && src_index_dev) return fail(SGX_EINVAL, "sgx_replay: origin_in_dev overlaps origin_out_dev with an index array (a slot would read labels another has written)%s");
        if (overlap && in0 != out0) return fail(SGX_EINVAL, "sgx_replay: origin_in_dev and origin_out_dev overlap without being equal%s");
    }
    SGX_ON_DEVICE(dst->device);
    const KParams kp = pool_params(dst, src, src_index_dev, 0);
    const ReplayArgs ra{io->actions_dev, io->lengths_dev, io->applied_dev, io->consumed_dev, io->stop_dev, result_out(*io), io->game_stride, io->step_stride, io->max_len,
                        (io->flags & SGX_REPLAY_SKIP_INVALID) ? 1 : 0};
    // the step's decode flags the replay's flags translate to
    const int step_flags = ((io->flags & SGX_REPLAY_ACTIONS_1D) ? SGX_STEP_ACTIONS_1D : 0) | ((io->flags & SGX_REPLAY_ALLOW_OSCILLATION) ? SGX_STEP_ALLOW_OSCILLATION : 0);
    if (dst->origin_out) {                                    // the TRACK instantiations: the same game, and the labels
        ReplayTrackedParams sp{kp, ra, LeafParams{}, OriginArgs{dst->origin_in, dst->origin_out}};
        sp.k.io.flags = step_flags;
        if (int rc = launch_leaf_or_plain<ReplayTrackedK>(dst, sp, stream)) return rc;
        dst->last_kind = SGX_LAUNCH_REPLAY_TRACKED;
        return SGX_OK;
    }
    ReplayParams sp{kp, ra};
    sp.k.io.flags = step_flags;
    if (int rc = launch_leaf_or_plain<ReplayK>(dst, sp, stream)) return rc;
    dst->last_kind = SGX_LAUNCH_REPLAY;
    return SGX_OK;
}

SGX_API int sgx_count_moves(sgx_env *src, const int32_t *src_index_dev, int64_t n_roots, int32_t *counts_dev, int64_t *offsets_dev, void *stream) {
    if (!src) return fail(SGX_EINVAL, "sgx_count_moves: handle is NULL%s");
    if (!offsets_dev) return fail(SGX_EINVAL, "sgx_count_moves: offsets_dev is NULL%s");
    if (n_roots < 0 || n_roots > 0x7fffffff) return fail(SGX_EINVAL, "sgx_count_moves: n_roots must be in [0, 2^31)%s");
    if (!src_index_dev && n_roots > src->n_envs) return fail(SGX_EINVAL, "sgx_count_moves: without src_index_dev n_roots must not exceed the handle's envs%s");
    if (int rc = check_aligned("sgx_count_moves", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_count_moves", "counts_dev", counts_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_count_moves", "offsets_dev", offsets_dev, 16)) return rc;
    SGX_ON_DEVICE(src->device);
    if (n_roots == 0) {
        HIP_TRY(hipMemsetAsync(offsets_dev, 0, sizeof(int64_t), (hipStream_t)stream));
        return SGX_OK;
    }
    const int64_t n_blocks = (n_roots + SCAN_BLOCK - 1) / SCAN_BLOCK;
    if (!counts_dev) {
        if (int rc = grow_scratch(&src->count_scratch, &src->count_scratch_cap, n_roots)) return rc;
        counts_dev = src->count_scratch;
    }
    if (int rc = grow_scratch(&src->scan_sums, &src->scan_sums_cap, n_blocks)) return rc;
    CountParams sp{pool_params(src, src, src_index_dev, 1), counts_dev};          // (nothing of the handle is written)
    sp.k.n_envs = n_roots;
    if (int rc = launch_pool_kernel<CountK>(src, sp, stream)) return rc;
    scan_sums_kernel<<<(unsigned)n_blocks, SCAN_BLOCK, 0, (hipStream_t)stream>>>(counts_dev, src->scan_sums, n_roots);
    scan_bases_kernel<<<1, SCAN_BLOCK, 0, SGX_INNER_STREAM(stream)>>>(src->scan_sums, n_blocks);
    scan_offsets_kernel<<<(unsigned)n_blocks, SCAN_BLOCK, 0, (hipStream_t)stream>>>(counts_dev, src->scan_sums, offsets_dev, n_roots);
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

SGX_API int sgx_expand_all(sgx_env *dst, sgx_env *src, const int32_t *src_index_dev, const sgx_children_io *io, void *stream) {
    if (!dst || !src || !io) return fail(SGX_EINVAL, "sgx_expand_all: handle or io is NULL%s");
    if (io->n_roots < 0 || io->n_roots > 0x7fffffff || io->n_children < 0 || io->first_child < 0)
        return fail(SGX_EINVAL, "sgx_expand_all: n_roots (below 2^31), n_children and first_child must not be negative%s");
    if (int rc = check_root_source("sgx_expand_all", dst, src, src_index_dev, io->n_roots, "n_roots", false)) return rc;
    if (int rc = refuse_start_pool("sgx_expand_all", dst)) return rc;
    if (io->n_children > dst->n_envs) return fail(SGX_EINVAL, "sgx_expand_all: n_children exceeds dst's envs%s");
    if (io->flags & ~SGX_CHILDREN_ACTIONS_1D) return fail(SGX_EINVAL, "sgx_expand_all: unknown flag bits%s");
    if (!io->offsets_dev) return fail(SGX_EINVAL, "sgx_expand_all: offsets_dev is NULL%s");
    if (int rc = check_aligned("sgx_expand_all", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_expand_all", "offsets_dev", io->offsets_dev, 16)) return rc;
    if (int rc = check_aligned("sgx_expand_all", "parent_dev", io->parent_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_expand_all", "action_dev", io->action_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_expand_all", "reward_dev", io->reward_dev, 4)) return rc;
    dst->last_kind = SGX_LAUNCH_CHILDREN;
    if (io->n_children == 0) return SGX_OK;
    SGX_ON_DEVICE(dst->device);
    ChildrenParams sp{pool_params(dst, src, src_index_dev, 0),
                      ChildrenArgs{io->offsets_dev, io->parent_dev, io->action_dev, result_out(*io), io->n_roots, io->first_child, (io->flags & SGX_CHILDREN_ACTIONS_1D) ? 1 : 0}};
    sp.k.n_envs = io->n_children;
    return launch_leaf_or_plain<ChildrenK>(dst, sp, stream);
}

SGX_API int sgx_state_keys(sgx_env *src, const int32_t *src_index_dev, int64_t n, int32_t view, int32_t flags, uint64_t *keys_dev, void *stream) {
    if (!src) return fail(SGX_EINVAL, "sgx_state_keys: handle is NULL%s");
    if (!keys_dev) return fail(SGX_EINVAL, "sgx_state_keys: keys_dev is NULL%s");
    if (n < 0 || n > 0x7fffffff) return fail(SGX_EINVAL, "sgx_state_keys: n must be in [0, 2^31)%s");
    if (!src_index_dev && n > src->n_envs) return fail(SGX_EINVAL, "sgx_state_keys: without src_index_dev n must not exceed the handle's envs%s");
    if (view != SGX_KEYS_VIEW_STATE && (view < -1 || view > 1))
        return fail(SGX_EINVAL, "sgx_state_keys: view must be 0 (each record's mover), +1, -1 or SGX_KEYS_VIEW_STATE%s");
    if (flags & ~(SGX_KEYS_NO_CLOCK | SGX_KEYS_WIDE)) return fail(SGX_EINVAL, "sgx_state_keys: unknown flag bits%s");
    if (int rc = check_aligned("sgx_state_keys", "src_index_dev", src_index_dev, 4)) return rc;
    if (int rc = check_aligned("sgx_state_keys", "keys_dev", keys_dev, (flags & SGX_KEYS_WIDE) ? 16 : 8)) return rc;
    if (n == 0) return SGX_OK;
    SGX_ON_DEVICE(src->device);
    const KParams k = make_params(src);
    const KeysParams p{src->boards, src_index_dev, keys_dev, n, src->rec_bytes, src->max_events, k.multi_ev, view, flags & SGX_KEYS_NO_CLOCK};
    if (int rc = for_geometry(src, [&](auto r, auto c) {
            constexpr int R = decltype(r)::value, C = decltype(c)::value;
            constexpr int PER_BLOCK = KEYS_THREADS / Geo<R, C>::LPG;                 // records per workgroup
            const unsigned grid = (unsigned)((n + PER_BLOCK - 1) / PER_BLOCK);
            if (flags & SGX_KEYS_WIDE) keys_kernel<R, C, true><<<grid, KEYS_THREADS, 0, (hipStream_t)stream>>>(p);
            else keys_kernel<R, C, false><<<grid, KEYS_THREADS, 0, (hipStream_t)stream>>>(p);
        })) return rc;
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

SGX_API int sgx_get_env_info(sgx_env *h, int32_t *info_dev, void *stream) {
    if (!h || !info_dev) return fail(SGX_EINVAL, "NULL argument%s");
    if (int rc = check_aligned("sgx_get_env_info", "info_dev", info_dev, 16)) return rc;      // (info_kernel: one int4 store per game)
    SGX_ON_DEVICE(h->device);
    info_kernel<<<(unsigned)((h->n_envs + 255) / 256), 256, 0, (hipStream_t)stream>>>(h->boards, h->rec_bytes, h->sc_off, info_dev, h->n_envs);
    HIP_TRY(hipGetLastError());
    return SGX_OK;
}

#ifdef SGX_STAMPS
// diagnostic build only (tools/phase_stamps.py): device pointer of the [N][16] stamp buffer
SGX_API void *sgx_debug_stamps(sgx_env *h) { return h ? (void *)h->stamps : nullptr; }
#endif
