// Store policy of a launch's observation writes: non-temporal or plain, and -- for the multi-step launches of the wave-per-game kernel --
// how many leading 128-byte lines of each game's observation leave as plain stores (KParams::nt_stores / plain_lines, sgx_obs.h: emit_codes;
// the kernels of BOTH mode read no count: their launches get split = 0 and fobs_plain_lines stays a figure of this function only).  Pure host arithmetic: no HIP, no handle; compiled on its own by tests/test_store_policy_cpu.py.
//
// Two rewrite distances.  A per-step launch writes a line again after the WHOLE batch (x the output sets of a ring): plain stores pay
// where launch bytes x sets fit the Infinity Cache (sgx_store_fits_launch, the rule of every launch before this header existed).  In a
// multi-step launch of steps_kernel a wave keeps its game for all steps of the launch and writes the game's lines again after `sets`
// steps: what has to fit is only
//     min(resident games, games) x sets x bytes per game,        resident games = CUs x resident workgroups per CU x games per workgroup
// -- 256 CUs x 3 workgroups x 8 games = 6,144 games for steps_kernel<10,10,0> (53,232 B of LDS per workgroup).  65,536 Barrage games in
// place: 6,144 x 30,512 B = 188 MB where the per-step measure sees 1.76 GB; the ring of three: 562 MB where it sees 5.3 GB.
#ifndef SGX_STORE_POLICY_H
#define SGX_STORE_POLICY_H
#include <stdint.h>

// A launch's observations (x sets) up to this many bytes stay in the 256 MiB Infinity Cache between two writes of a line: measured
// crossover between 281 and 316 MB on four board sizes (sgx_obs.h).
#define SGX_CACHE_FIT_BYTES ((int64_t)300 * 1000 * 1000)
// What the plain-stored part of a multi-step launch's rewrite set (mask and results included) may take while the non-temporal rest streams
// past it.  Measured, 65,536 Barrage games, one process, placed buffers, policies alternated (tools/store_split_ab.py,
// profiles/store_split_ab.log), us per step against every whole line non-temporal (236-242):
//   in place (188 MB rewritten within reach)    all plain 232
//   ring of 2   56 ... 208 lines plain (131 ... 373 MB) and all plain 233
//   ring of 3   24 ... 152 lines (125 ... 427 MB) 232-233;  176 lines (484 MB) 244;  all plain (562 MB) 259-266
//   ring of 4   24 / 48 / 96 lines (167 ... 393 MB) 233
//   ring of 8   8 lines (233 MB) 242 against 246;  24 lines (333 MB) level with none
// The gain is a plateau, not a slope: any share from three sweeps up to about 400 MB buys the same 2.5-4 %, and in place 104 lines, 208
// lines and all plain are equal.  That is NOT what absorption in proportion to capacity would look like, so the mechanism is not
// established and "mask + results + share <= budget" is not a model of it: the budget arithmetic is an empirically safe way to pick a
// share inside the plateau on every ring length measured, nothing more.  The constant is the largest that is not slower than its smaller
// neighbour on ALL rows -- 333 MB loses the ring of 8's gain, 250 MB keeps every row: in place all plain, rings of 2 / 3 / 4 / 8 get
// 128 / 72 / 48 / 8 lines.  The rows above come from the sweeps of two earlier builds of these kernels (same store text); the deciding
// one, the ring of 8, is thin there (one session, 241.8 median against a minimum of 242.5).  The log's last section repeats the rings of
// 4 and 8 and the ring of 3 at 152 / 176 lines on the build as committed.
#define SGX_PLAIN_BUDGET_BYTES ((int64_t)250 * 1000 * 1000)
// A rewrite set beyond the budget: 1 = the observation(s) get the share of the budget that mask and results leave, 0 = no plain share
// (the rule before the split).  1 by the rows above: the ring of three at the rule's 72 lines 233.1 us against 239.2 (minimum 237.1).
#define SGX_STORE_SPLIT_DEFAULT 1
#define SGX_STORE_LINE_BYTES 128
#define SGX_STORE_SWEEP_LINES 8          // emit_codes writes 1 KiB per sweep of a wave: the split moves by whole sweeps
#define SGX_RESULT_BYTES 12              // two float32 rewards, done, invalid_action, ending_invalid, player

typedef struct sgx_store_shape {
    int32_t cus;                 // compute units of the device
    int32_t wg_per_cu;           // resident workgroups per CU of the kernel that plays the launch (occupancy query)
    int32_t games_per_wg;        // games a workgroup plays at a time (waves per workgroup x games per wave)
    int64_t games;               // games of the launch
    int32_t sets;                // output sets of a ring / slots of a trajectory buffer; 1 = in place
    int64_t obs_bytes, fobs_bytes, mask_bytes;      // per game; 0 = the launch does not write it
    int64_t budget;              // SGX_PLAIN_BUDGET_BYTES
    int32_t split;               // SGX_STORE_SPLIT_DEFAULT; 0: a rewrite set beyond the budget gets no plain share (everything whole non-temporal)
} sgx_store_shape;

typedef struct sgx_store_policy {
    int32_t nt_stores;           // 1: whole lines beyond the plain share leave as non-temporal stores
    int32_t plain_lines;         // leading lines of each game's observation that leave as plain stores (nt_stores = 1 only)
    int32_t fobs_plain_lines;    // the same for the fully observable observation
} sgx_store_policy;

static inline int32_t sgx_store_lines(int64_t bytes) { return (int32_t)((bytes + SGX_STORE_LINE_BYTES - 1) / SGX_STORE_LINE_BYTES); }
// the most lines of an observation of `bytes` a split gives: whole sweeps, never more than the observation has
static inline int32_t sgx_store_max_plain_lines(int64_t bytes) { return sgx_store_lines(bytes) / SGX_STORE_SWEEP_LINES * SGX_STORE_SWEEP_LINES; }

// per-step launches, lane kernels, states_kernel, the store probe: by the bytes the launch writes before a line is written again
static inline int sgx_store_fits_launch(int64_t launch_bytes_times_sets) { return launch_bytes_times_sets <= SGX_CACHE_FIT_BYTES; }

static inline int64_t sgx_store_resident_games(const sgx_store_shape *s) {
    const int64_t resident = (int64_t)s->cus * s->wg_per_cu * s->games_per_wg;
    return resident < s->games ? resident : s->games;
}
// bytes written between two writes of one line by the games that are on the chip together
static inline int64_t sgx_store_rewrite_set(const sgx_store_shape *s) {
    return sgx_store_resident_games(s) * s->sets * (s->obs_bytes + s->fobs_bytes + s->mask_bytes + SGX_RESULT_BYTES);
}

// multi-step launches of the wave-per-game kernel
static inline sgx_store_policy sgx_store_policy_multi_step(const sgx_store_shape *s) {
    sgx_store_policy out = {1, 0, 0};
    if (sgx_store_rewrite_set(s) <= s->budget) {                     // everything the resident games rewrite fits: all plain
        out.nt_stores = 0;
        out.plain_lines = sgx_store_max_plain_lines(s->obs_bytes);    // (not read by a launch with nt_stores = 0)
        out.fobs_plain_lines = sgx_store_max_plain_lines(s->fobs_bytes);
        return out;
    }
    if (!s->split) return out;
    const int64_t slots = sgx_store_resident_games(s) * s->sets;     // (game, set) pairs whose lines are written within reach
    const int64_t per = slots > 0 ? s->budget / slots - s->mask_bytes - SGX_RESULT_BYTES : 0;
    const int64_t sweep = (int64_t)SGX_STORE_SWEEP_LINES * SGX_STORE_LINE_BYTES;
    int64_t sweeps = per > 0 ? per / sweep : 0;                      // below one sweep: as before, everything whole non-temporal
    const int64_t obs_sweeps = sgx_store_max_plain_lines(s->obs_bytes) / SGX_STORE_SWEEP_LINES;
    const int64_t fobs_sweeps = sgx_store_max_plain_lines(s->fobs_bytes) / SGX_STORE_SWEEP_LINES;
    const int64_t to_obs = sweeps < obs_sweeps ? sweeps : obs_sweeps;
    sweeps -= to_obs;
    const int64_t to_fobs = sweeps < fobs_sweeps ? sweeps : fobs_sweeps;
    out.plain_lines = (int32_t)to_obs * SGX_STORE_SWEEP_LINES;
    out.fobs_plain_lines = (int32_t)to_fobs * SGX_STORE_SWEEP_LINES;
    return out;
}
#endif
