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
};

// The frame (sgx_pool_frame.h) around the sampler: PLAY_ROOT_DRAW generates the root's mask and draws the first action, then PLAY_MOVE_DRAW
// plays move after move.
// The loop is bounded by a COUNT: every applied move advances the turn counter and the max-turn ending fires at turn >= max_turns, so a game
// that starts at `turn` has at most max(max_turns - turn, 0) + 1 moves left (the + 1: a root at or past its last turn that is not over yet
// still plays the move that ends it).  A game that were not over after that many moves would be reported like one cut off by max_steps.
template <int R_, int C_, int VAR = 0>
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
    store_results(top->play.out, env, lane, carry.flags);
    int32_t *const o_length = top->play.length;
    if (lane == 0 && o_length) o_length[env] = t;
    write_final_record(LW[slot], P, env, carry, lane);
}

}  // namespace
