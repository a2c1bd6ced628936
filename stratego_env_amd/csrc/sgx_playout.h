// sgx_playout.h -- playout_kernel: random games to the end, pool to pool, in one launch (sgx_playout)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// What playout_kernel takes next to KParams (k.boards = dst's records, k.src_boards / k.src_index = where the roots come from, k.seed /
// k.env_id_offset = dst's): the key's `draw`, the cap on the moves, and the five result tensors (each nullable).
struct PlayParams {
    uint64_t draw;
    ResultOut out;
    int32_t *length;
    int32_t max_steps;
};
struct PlayoutParams {
    KParams k;
    PlayParams play;
    LeafParams leaf;      // read by the LEAF instantiation alone
};

// The frame (sgx_pool_frame.h) around the sampler: PLAY_ROOT_DRAW generates the root's mask and draws the first action, then PLAY_MOVE_DRAW
// plays move after move.
// The loop is bounded by a COUNT: every applied move advances the turn counter and the max-turn ending fires at turn >= max_turns, so a game
// that starts at `turn` has at most max(max_turns - turn, 0) + 1 moves left (the + 1: a root at or past its last turn that is not over yet
// still plays the move that ends it).  A game that were not over after that many moves would be reported like one cut off by max_steps.
template <int R_, int C_, int VAR = 0, bool LEAF = false>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (steps_waves_per_simd<Geo<R_, C_, VAR>, 8>())) void playout_kernel(const PlayoutParams SP) {
    using G = Geo<R_, C_, VAR>;
    constexpr int KIND = 8;
    const SGX_KERNARG PlayoutParams *top = kernarg_of(SP);
    const SGX_KERNARG KParams &P = top->k;
    __shared__ Lds<G, ObsKind<KIND>::NIB_CH> LW[G::WPB * G::GPW];
    __shared__ alignas(16) uint8_t shared[shared_table_bytes<G, KIND>()];
    __shared__ alignas(16) uint8_t obst_s[G::OBST_BYTES + COMBAT_BYTES];
    const int lane = threadIdx.x & (G::LPG - 1), slot = threadIdx.x / G::LPG;
    const int64_t env = P.env_first + group_of_block(P) * (G::WPB * G::GPW) + slot;
    GameInput in = empty_input();
    if (env < P.n_envs) fetch_root<G>(P, env, lane, in);
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    __syncthreads();   // from here on every wave works on its own games, to their ends
    if (env >= P.n_envs) return;
    StepCarry carry = pool_carry(0);
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, PLAY_ROOT_DRAW>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr,
                                                                                                                     &carry, false, &top->play);
    const int max_steps = top->play.max_steps;
    int limit = max(carry.max_turns - carry.turn, 0) + 1;
    if (max_steps > 0) limit = min(limit, max_steps);
    int t = 0;
    for (; t < limit && !(carry.flags & F_OVER); ++t) {
        const SGX_KERNARG PlayoutParams *tp = top;
        int lane_t = lane, slot_t = slot;
        asm volatile("" : "+s"(tp), "+v"(lane_t), "+v"(slot_t));
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, PLAY_MOVE_DRAW>(tp->k, LW[slot_t], shared, obst_s, env, lane_t, in, nullptr,
                                                                                                                         nullptr, &carry, false, &tp->play);
    }
    if constexpr (LEAF) store_results_leaf(LW[slot], top->play.out, top->leaf, env, lane, carry.flags);
    else store_results(top->play.out, env, lane, carry.flags);
    int32_t *const o_length = top->play.length;
    if (lane == 0 && o_length) o_length[env] = t;
    write_final_record(LW[slot], P, env, carry, lane);
}

// sgx_playout_weighted: playout_kernel's parameters, then the policy -- whether the target of a move is looked up in the opponent's true
// pieces (SGX_PLAYOUT_SEE_ALL) and the weight table itself, BY VALUE: 1,456 bytes in the launch's own argument block (the whole block stays
// far below the 4 KiB an argument block may have), so every launch plays with the table its call was given, whatever the host does to its
// copy afterwards, with no device buffer to own, fill or free.
struct WeightedPlayoutParams {
    KParams k;
    PlayParams play;
    int32_t see_all, reserved;
    uint16_t weights[WT_ENTRIES];
    LeafParams leaf;      // read by the LEAF instantiation alone
};
static_assert(sizeof(WeightedPlayoutParams) <= 4096 && offsetof(WeightedPlayoutParams, weights) % 4 == 0, "the table travels in the kernel arguments");

// the occupancy promise of playout_weighted_kernel: playout_kernel's, or what the workgroup's LDS with the table and the weight sums allows
template <class G>
constexpr int weighted_waves_per_simd() {
    constexpr int per_wg = G::WPB * G::GPW * ((int)sizeof(Lds<G, ObsKind<8>::NIB_CH>) + 4 * G::CNT_PAD) + shared_table_bytes<G, 8>() + G::OBST_BYTES + COMBAT_BYTES + 2 * WT_ENTRIES;
    constexpr int w = ((160 * 1024) / per_wg) * G::WPB / 4, want = steps_waves_per_simd<G, 8>();
    return w < 1 ? 1 : (w < want ? w : want);
}

// playout_kernel with the weighted draw (sgx_mask.h: draw_weighted) in the place of the uniform one.  The passes of env_step only COUNT
// (PLAY_ROOT_COUNT / PLAY_MOVE_COUNT: the mask bits stay in LDS, the number of valid moves comes back in the carry) and the kernel draws
// from what they left.  The workgroup stages the table into LDS with its other shared tables, before its one barrier; the per-cell weight
// sums are an LDS array of this kernel, one row per game.
template <int R_, int C_, int VAR = 0, bool LEAF = false>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (weighted_waves_per_simd<Geo<R_, C_, VAR>>())) void playout_weighted_kernel(const WeightedPlayoutParams SP) {
    using G = Geo<R_, C_, VAR>;
    constexpr int KIND = 8;
    const SGX_KERNARG WeightedPlayoutParams *top = kernarg_of(SP);
    const SGX_KERNARG KParams &P = top->k;
    __shared__ Lds<G, ObsKind<KIND>::NIB_CH> LW[G::WPB * G::GPW];
    __shared__ alignas(16) uint8_t shared[shared_table_bytes<G, KIND>()];
    __shared__ alignas(16) uint8_t obst_s[G::OBST_BYTES + COMBAT_BYTES];
    __shared__ alignas(16) uint16_t wtab[WT_ENTRIES];
    __shared__ alignas(16) uint32_t wsum[G::WPB * G::GPW][G::CNT_PAD];
    const int lane = threadIdx.x & (G::LPG - 1), slot = threadIdx.x / G::LPG;
    const int64_t env = P.env_first + group_of_block(P) * (G::WPB * G::GPW) + slot;
    GameInput in = empty_input();
    if (env < P.n_envs) fetch_root<G>(P, env, lane, in);
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    for (int i = threadIdx.x; i < WT_ENTRIES / 2; i += 64 * G::WPB)
        reinterpret_cast<uint32_t *>(wtab)[i] = reinterpret_cast<const SGX_KERNARG uint32_t *>(top->weights)[i];
    __syncthreads();   // from here on every wave works on its own games, to their ends
    if (env >= P.n_envs) return;
    const bool see_all = top->see_all != 0;
    StepCarry carry = pool_carry(0);
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, PLAY_ROOT_COUNT>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr,
                                                                                                                      &carry, false, &top->play);
    // the draw of sgx_playout for the position the carry holds, taken by the weights
    auto draw = [&](const SGX_KERNARG WeightedPlayoutParams *tp, const int slot_t, const int lane_t) {
        const uint64_t r = sgx_rng(tp->k.seed, (uint64_t)(tp->k.env_id_offset + env), tp->play.draw, STREAM_PLAYOUT, (uint32_t)carry.turn);
        carry.na = draw_weighted(LW[slot_t], wsum[slot_t], wtab, (carry.flags & F_PLAYER_M1) ? 1 : 0, see_all, carry.na, r, lane_t);
    };
    if (!(carry.flags & F_OVER)) draw(top, slot, lane);
    const int max_steps = top->play.max_steps;
    int limit = max(carry.max_turns - carry.turn, 0) + 1;
    if (max_steps > 0) limit = min(limit, max_steps);
    int t = 0;
    for (; t < limit && !(carry.flags & F_OVER); ++t) {
        const SGX_KERNARG WeightedPlayoutParams *tp = top;
        int lane_t = lane, slot_t = slot;
        asm volatile("" : "+s"(tp), "+v"(lane_t), "+v"(slot_t));
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, PLAY_MOVE_COUNT>(tp->k, LW[slot_t], shared, obst_s, env, lane_t, in, nullptr,
                                                                                                                          nullptr, &carry, false, &tp->play);
        if (!(carry.flags & F_OVER)) draw(tp, slot_t, lane_t);
    }
    if constexpr (LEAF) store_results_leaf(LW[slot], top->play.out, top->leaf, env, lane, carry.flags);
    else store_results(top->play.out, env, lane, carry.flags);
    int32_t *const o_length = top->play.length;
    if (lane == 0 && o_length) o_length[env] = t;
    write_final_record(LW[slot], P, env, carry, lane);
}

}  // namespace
