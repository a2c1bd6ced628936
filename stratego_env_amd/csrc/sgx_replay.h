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
    ResultOut out;
    int64_t game_stride, step_stride;
    int32_t max_len, skip_invalid;
};
struct ReplayParams {
    KParams k;
    ReplayArgs rep;
    LeafParams leaf;      // read by the LEAF instantiation alone
};

// One chunk of a game's list: lane j of the game's LPG lanes takes entry t0 + j, one load instruction per chunk (contiguous 4 * LPG bytes
// with step_stride == 1, one entry per line otherwise).  Entries at or beyond `len` are not loaded.
// (t0 is 64 bits wide: with step_stride == 0 a list may be as long as an int32 counts, and c + LPG must not wrap)
__device__ __forceinline__ int replay_chunk(const int32_t *lane_entry0, const int64_t step_stride, const int64_t t0, const int lane, const int len) {
    int v = 0;
    if (t0 + lane < (int64_t)len) v = lane_entry0[t0 * step_stride];
    return v;
}

// The frame (sgx_pool_frame.h) with the move taken from memory instead of a sampler: PLAY_ROOT_GIVEN stages the root, PLAY_MOVE_GIVEN applies
// one entry.  No mask is generated anywhere -- a replayed move asks what sgx_expand's asks, whether the next mover has a move at all.
// THE ACTION STREAM stays off the step's dependent chain: the game's lanes hold two chunks of LPG entries in two registers, `cur` and `nxt`,
// both requested before the workgroup stages its tables; a move takes its entry from `cur` with a cross-lane read inside the game's own lanes,
// and when a chunk is used up `nxt` becomes `cur` and the chunk after it is requested -- LPG moves before its first entry is needed.
// The loop is bounded by a COUNT, len <= max_len; it advances one entry per pass whether the entry was applied or passed over.
template <int R_, int C_, int VAR = 0, bool LEAF = false>
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
    GameInput in = empty_input();
    int len = 0, cur = 0, nxt = 0;
    const int32_t *lane_entry0 = nullptr;              // this lane's entry of chunk 0: entry `lane` of the game's list
    if (env < P.n_envs) {
        fetch_root<G>(P, env, lane, in);
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
    StepCarry carry = pool_carry(0);
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, PoolParams, PLAY_ROOT_GIVEN>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry, false);
    int c = 0, m = 0, stop = 0;
    for (;;) {
        if (c >= len) break;                                            // the list is exhausted (stop = 0)
        if (carry.flags & F_OVER) { stop = 1; break; }                   // the game is over: what follows in the list is not read
        const SGX_KERNARG ReplayParams *tp = top;
        int lane_t = lane, slot_t = slot;
        asm volatile("" : "+s"(tp), "+v"(lane_t), "+v"(slot_t));
        carry.na = __shfl(cur, c & (G::LPG - 1), G::LPG);               // entry c: held by lane c mod LPG of this game
        const int turn_before = carry.turn;
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, PoolParams, PLAY_MOVE_GIVEN>(tp->k, LW[slot_t], shared, obst_s, env, lane_t, in, nullptr, nullptr,
                                                                                                             &carry, false);
        const bool valid = carry.turn != turn_before;                   // (every valid action on an unfinished game advances the counter)
        if (!valid && !tp->rep.skip_invalid) { stop = 2; break; }        // entry c is the offending one: c stays
        m += valid ? 1 : 0;
        ++c;
        if ((c & (G::LPG - 1)) == 0) {                                   // the chunk is used up: the next one arrived LPG moves ago
            cur = nxt;
            nxt = replay_chunk(lane_entry0, tp->rep.step_stride, (int64_t)c + G::LPG, lane_t, len);
        }
    }
    if constexpr (LEAF) store_results_leaf(LW[slot], top->rep.out, top->leaf, env, lane, carry.flags);
    else store_results(top->rep.out, env, lane, carry.flags);
    uint8_t *const o_stop = top->rep.stop;
    int32_t *const o_applied = top->rep.applied, *const o_consumed = top->rep.consumed;
    if (lane == 0 && o_stop) o_stop[env] = (uint8_t)stop;
    if (lane == 0 && o_applied) o_applied[env] = m;
    if (lane == 0 && o_consumed) o_consumed[env] = c;
    write_final_record(LW[slot], P, env, carry, lane);
}

}  // namespace
