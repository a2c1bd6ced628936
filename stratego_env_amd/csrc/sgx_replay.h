// sgx_replay.h -- replay_kernel: given action lists played from packed records, pool to pool, in one launch (sgx_replay)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// What replay_kernel takes next to KParams (k.boards = dst's records, k.src_boards / k.src_index = where the roots come from, k.io.flags =
// the step's decode flags the replay's flags translate to): the action lists and their layout, the lengths, and the result tensors (each
// nullable).
struct ReplayArgs {
    const int32_t *actions, *lengths;
    int32_t *applied, *consumed;
    uint8_t *stop;
    float *reward;
    uint8_t *done, *ending_invalid;
    int8_t *player;
    int64_t game_stride, step_stride;
    int32_t max_len, skip_invalid;
};
struct ReplayParams {
    KParams k;
    ReplayArgs rep;
};

// One chunk of a game's list: lane j of the game's LPG lanes takes entry t0 + j, one load instruction per chunk (contiguous 4 * LPG bytes
// with step_stride == 1, one entry per line otherwise).  Entries at or beyond `len` are not loaded.
// (t0 is 64 bits wide: with step_stride == 0 a list may be as long as an int32 counts, and c + LPG must not wrap)
__device__ __forceinline__ int replay_chunk(const int32_t *lane_entry0, const int64_t step_stride, const int64_t t0, const int lane, const int len) {
    int v = 0;
    if (t0 + lane < (int64_t)len) v = lane_entry0[t0 * step_stride];
    return v;
}

// playout_kernel's shape (one wave per game, two or four games per wave on the smaller boards, the no-observation kind; the root staged once,
// the boards in LDS and the scalars in the carry, write_record and the results after the loop; no barrier in the loop, no atomics, nothing
// between waves) with the move taken from memory instead of the sampler: env_step<PLAY = 3> stages the root, env_step<PLAY = 4> applies one
// entry.  No mask is generated anywhere -- a replayed move asks what sgx_expand's asks, whether the next mover has a move at all.
// THE ACTION STREAM stays off the step's dependent chain: the game's lanes hold two chunks of LPG entries in two registers, `cur` and `nxt`,
// both requested before the workgroup stages its tables; a move takes its entry from `cur` with a cross-lane read inside the game's own lanes,
// and when a chunk is used up `nxt` becomes `cur` and the chunk after it is requested -- LPG moves before its first entry is needed.
// The loop is bounded by a COUNT, len <= max_len; it advances one entry per pass whether the entry was applied or passed over.
// Games that share a wave stop at different counts: every condition of the loop is per game, so a stopped game's lanes are masked off while
// its wave-mates go on.
template <int R_, int C_, int VAR = 0>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (steps_waves_per_simd<Geo<R_, C_, VAR>, 8>())) void replay_kernel(const ReplayParams SP) {
    using G = Geo<R_, C_, VAR>;
    constexpr int KIND = 8;
    const SGX_KERNARG ReplayParams *top = kernarg_of(SP);
    const SGX_KERNARG KParams &P = top->k;
    __shared__ Lds<G, ObsKind<KIND>::NIB_CH> LW[G::WPB * G::GPW];
    __shared__ alignas(16) uint8_t shared[shared_table_bytes<G, KIND>()];
    __shared__ alignas(16) uint8_t obst_s[G::OBST_BYTES + COMBAT_BYTES];
    const int lane = threadIdx.x & (G::LPG - 1), slot = threadIdx.x / G::LPG;
    const int64_t env = P.env_first + group_of_block(P) * (G::WPB * G::GPW) + slot;
    // the root's record, the list's length and its first two chunks: all requested before the workgroup stages its tables
    const int4 zero4 = make_int4(0, 0, 0, 0);
    GameInput in{zero4, zero4, zero4, 0, nullptr};
    int len = 0, cur = 0, nxt = 0;
    const int32_t *lane_entry0 = nullptr;              // this lane's entry of chunk 0: entry `lane` of the game's list
    if (env < P.n_envs) {
        in.src = reinterpret_cast<const int4 *>(P.src_boards + (int64_t)(P.src_index ? P.src_index[env] : env) * (int64_t)P.rec_bytes);
        load_record<G>(P, in.src, lane, in.rq0, in.rq1);
        const int max_len = top->rep.max_len;
        const int32_t *lengths = top->rep.lengths;
        len = lengths ? min(max(lengths[env], 0), max_len) : max_len;
        lane_entry0 = top->rep.actions + env * top->rep.game_stride + (int64_t)lane * top->rep.step_stride;
        cur = replay_chunk(lane_entry0, top->rep.step_stride, 0, lane, len);
        nxt = replay_chunk(lane_entry0, top->rep.step_stride, G::LPG, lane, len);
    }
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    __syncthreads();   // from here on every wave works on its own games, to the ends of their lists
    if (env >= P.n_envs) return;
    StepCarry carry{0, 0, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, 0};
    // the root: its record staged (a copy of the step of its own, so that the record's registers are dead in the loop)
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, PoolParams, 3>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry, false);
    int c = 0, m = 0, stop = 0;
    for (;;) {
        if (c >= len) break;                                            // the list is exhausted (stop = 0)
        if (carry.flags & F_OVER) { stop = 1; break; }                   // the game is over: what follows in the list is not read
        const SGX_KERNARG ReplayParams *tp = top;
        int lane_t = lane, slot_t = slot;
        // (the step's reads of the parameters start here, and what a step derives from the lane is recomputed in every step: steps_kernel)
        asm volatile("" : "+s"(tp), "+v"(lane_t), "+v"(slot_t));
        carry.na = __shfl(cur, c & (G::LPG - 1), G::LPG);               // entry c: held by lane c mod LPG of this game
        const int turn_before = carry.turn;
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, PoolParams, 4>(tp->k, LW[slot_t], shared, obst_s, env, lane_t, in, nullptr, nullptr, &carry,
                                                                                               false);
        const bool valid = carry.turn != turn_before;                   // (every valid action on an unfinished game advances the counter)
        if (!valid && !tp->rep.skip_invalid) { stop = 2; break; }        // entry c is the offending one: c stays
        m += valid ? 1 : 0;
        ++c;
        if ((c & (G::LPG - 1)) == 0) {                                   // the chunk is used up: the next one arrived LPG moves ago
            cur = nxt;
            nxt = replay_chunk(lane_entry0, tp->rep.step_stride, (int64_t)c + G::LPG, lane_t, len);
        }
    }
    // ---- the results: what a step on the final position reports (env_step's rewards / dones)
    const int flags = carry.flags;
    const bool over = (flags & F_OVER) != 0, end_invalid = over && (flags & F_END_INVALID);
    float rew_p1 = 0.f, rew_m1 = 0.f;
    if (over && !end_invalid) {
        const int w = (flags & F_WIN_P1) ? 1 : (flags & F_WIN_M1) ? -1 : 0;
        rew_p1 = w == 0 ? 1e-4f : (float)w;     // impl:838-840
        rew_m1 = w == 0 ? 1e-4f : (float)-w;
    }
    float *const o_reward = top->rep.reward;
    uint8_t *const o_done = top->rep.done, *const o_end_invalid = top->rep.ending_invalid, *const o_stop = top->rep.stop;
    int8_t *const o_player = top->rep.player;
    int32_t *const o_applied = top->rep.applied, *const o_consumed = top->rep.consumed;
    if (lane < 2 && o_reward) o_reward[2 * env + lane] = lane ? rew_m1 : rew_p1;
    if (lane == 0 && o_done) o_done[env] = over ? 1 : 0;
    if (lane == 0 && o_end_invalid) o_end_invalid[env] = end_invalid ? 1 : 0;
    if (lane == 0 && o_player) o_player[env] = (int8_t)((flags & F_PLAYER_M1) ? -1 : 1);
    if (lane == 0 && o_stop) o_stop[env] = (uint8_t)stop;
    if (lane == 0 && o_applied) o_applied[env] = m;
    if (lane == 0 && o_consumed) o_consumed[env] = c;
    // ---- the final position, whole (a copy of the root where nothing was applied)
    write_record(LW[slot], P.boards + env * (int64_t)P.rec_bytes, P.rec_bytes, make_int4(carry.turn, flags, carry.max_turns, carry.game_no),
                 make_int4(carry.n_events, carry.rp0, carry.rp1, 0), carry.n_events, lane);
}

}  // namespace
