// sgx_playout.h -- playout_kernel: random games to the end, pool to pool, in one launch (sgx_playout)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// What playout_kernel takes next to KParams (k.boards = dst's records, k.src_boards / k.src_index = where the roots come from, k.seed /
// k.env_id_offset = dst's): the key's `draw`, the cap on the moves, and the five result tensors (each nullable).
struct PlayParams {
    uint64_t draw;
    float *reward;
    uint8_t *done, *ending_invalid;
    int8_t *player;
    int32_t *length;
    int32_t max_steps;
};
struct PlayoutParams {
    KParams k;
    PlayParams play;
};

// One wave per game (two games per wave with VAR = 2, Geo's own two or four on boards of up to 32 cells), the no-observation kind.  The root
// is staged once, env_step<PLAY = 1> generates its mask and draws the first action, then env_step<PLAY = 2> plays move after move with the
// boards in LDS and the scalars in the carry, as steps_kernel does; nothing leaves the wave before the loop has ended.
// The loop is bounded by a COUNT: every applied move advances the turn counter and the max-turn ending fires at turn >= max_turns, so a game
// that starts at `turn` has at most max(max_turns - turn, 0) + 1 moves left (the + 1: a root at or past its last turn that is not over yet
// still plays the move that ends it).  A game that were not over after that many moves would be reported like one cut off by max_steps.
// Games that share a wave end at different times: the loop's condition is per game, so a finished game's lanes are masked off while the
// wave goes on with the others (the divergence a ragged batch already has at env >= n_envs); no barrier, no atomics, no exchange between waves.
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
    // the root's record: slot src_index[env] (env when NULL) of the source's records, requested before the workgroup stages its tables
    const int4 zero4 = make_int4(0, 0, 0, 0);
    GameInput in{zero4, zero4, zero4, 0, nullptr};
    if (env < P.n_envs) {
        in.src = reinterpret_cast<const int4 *>(P.src_boards + (int64_t)(P.src_index ? P.src_index[env] : env) * (int64_t)P.rec_bytes);
        load_record<G>(P, in.src, lane, in.rq0, in.rq1);
    }
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    __syncthreads();   // from here on every wave works on its own games, to their ends
    if (env >= P.n_envs) return;
    StepCarry carry{0, 0, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, 0};
    // the root: its record staged, its mover's mask generated, the first action drawn (a copy of the step of its own, so that the record's
    // registers are dead in the loop)
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, 1>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry,
                                                                                                        false, &top->play);
    const int max_steps = top->play.max_steps;
    int limit = max(carry.max_turns - carry.turn, 0) + 1;
    if (max_steps > 0) limit = min(limit, max_steps);
    int t = 0;
    for (; t < limit && !(carry.flags & F_OVER); ++t) {
        const SGX_KERNARG PlayoutParams *tp = top;
        int lane_t = lane, slot_t = slot;
        // (the step's reads of the parameters start here, and what a step derives from the lane is recomputed in every step: steps_kernel)
        asm volatile("" : "+s"(tp), "+v"(lane_t), "+v"(slot_t));
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, 2>(tp->k, LW[slot_t], shared, obst_s, env, lane_t, in, nullptr, nullptr,
                                                                                                            &carry, false, &tp->play);
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
    float *const o_reward = top->play.reward;
    uint8_t *const o_done = top->play.done, *const o_end_invalid = top->play.ending_invalid;
    int8_t *const o_player = top->play.player;
    int32_t *const o_length = top->play.length;
    if (lane < 2 && o_reward) o_reward[2 * env + lane] = lane ? rew_m1 : rew_p1;
    if (lane == 0 && o_done) o_done[env] = over ? 1 : 0;
    if (lane == 0 && o_end_invalid) o_end_invalid[env] = end_invalid ? 1 : 0;
    if (lane == 0 && o_player) o_player[env] = (int8_t)((flags & F_PLAYER_M1) ? -1 : 1);
    if (lane == 0 && o_length) o_length[env] = t;
    // ---- the final position, whole (a copy of the root where nothing was played)
    write_record(LW[slot], P.boards + env * (int64_t)P.rec_bytes, P.rec_bytes, make_int4(carry.turn, flags, carry.max_turns, carry.game_no),
                 make_int4(carry.n_events, carry.rp0, carry.rp1, 0), carry.n_events, lane);
}

}  // namespace
