// sgx_step_vs.h -- step_vs_kernel: the agent's move and a table bot's reply, pool to pool (or in place), in one launch (sgx_step_vs)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// What step_vs_kernel takes next to KParams and playout_weighted_kernel's PlayParams (draw = the key's `draw`, out = the four result tensors;
// length stays NULL and max_steps 0: nothing here counts moves): the agent's actions and sides, the three outputs of its own (each nullable).
struct VsArgs {
    const int32_t *actions;      // [N] nullable: NULL = no agent moves, the bot opens where it is to move
    const int8_t *agent_dev;     // [N] nullable: < 0 = the agent plays -1; NULL = `agent` for every slot
    uint8_t *invalid_action, *moved;
    int32_t *reply_action;
    int32_t agent, see_all;
};
// The table travels BY VALUE in the launch's own argument block, as in WeightedPlayoutParams: every launch plays with the table its call
// was given.
struct StepVsParams {
    KParams k;
    PlayParams play;
    VsArgs vs;
    uint16_t weights[WT_ENTRIES];
};
static_assert(sizeof(StepVsParams) <= 4096 && offsetof(StepVsParams, weights) % 4 == 0, "the table travels in the kernel arguments");

constexpr int VS_MOVED_AGENT = 1, VS_MOVED_BOT = 2;      // SGX_VS_MOVED_*

// The frame (sgx_pool_frame.h) with playout_weighted_kernel's LDS and occupancy promise, and a STRAIGHT LINE in the place of its loop:
//   PLAY_ROOT_COUNT stages the root and leaves its mover's mask bits and count;
//   where the agent is to move and an action is given, one PLAY_MOVE_COUNT applies it as a step applies an action -- the pass's own decode
//   and validity checks stand before every use of the value, and a refused action leaves the carry's turn counter where it was (sgx_step.h)
//   -- and leaves the next mover's bits and count;
//   where the bot is to move then (players alternate: after the agent's move, or at the root), one draw_weighted from those bits with the
//   key's STREAM_REPLY word, and one PLAY_MOVE_GIVEN applies the drawn move (nothing is drawn after it: whether the next mover has a move
//   is all the endings ask).
// Nothing is bounded by the game's state: two conditions per game, no loop.  The agent's action and side are read once, with the record,
// before the barrier, and only for env < n_envs; every condition behind the barrier is per game, so wave-mates diverge as they do in
// playout_weighted_kernel when their games end at different moves.
template <int R_, int C_, int VAR = 0>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (weighted_waves_per_simd<Geo<R_, C_, VAR>>())) void step_vs_kernel(const StepVsParams SP) {
    using G = Geo<R_, C_, VAR>;
    constexpr int KIND = 8;
    const SGX_KERNARG StepVsParams *top = kernarg_of(SP);
    const SGX_KERNARG KParams &P = top->k;
    __shared__ Lds<G, ObsKind<KIND>::NIB_CH> LW[G::WPB * G::GPW];
    __shared__ alignas(16) uint8_t shared[shared_table_bytes<G, KIND>()];
    __shared__ alignas(16) uint8_t obst_s[G::OBST_BYTES + COMBAT_BYTES];
    __shared__ alignas(16) uint16_t wtab[WT_ENTRIES];
    __shared__ alignas(16) uint32_t wsum[G::WPB * G::GPW][G::CNT_PAD];
    const int lane = threadIdx.x & (G::LPG - 1), slot = threadIdx.x / G::LPG;
    const int64_t env = P.env_first + group_of_block(P) * (G::WPB * G::GPW) + slot;
    // the root's record, the agent's action and its side: all requested before the workgroup stages its tables
    GameInput in = empty_input();
    int a_agent = 0, side = 1;
    bool given = false;
    if (env < P.n_envs) {
        fetch_root<G>(P, env, lane, in);
        const int32_t *const actions = top->vs.actions;
        const int8_t *const agent_dev = top->vs.agent_dev;
        given = actions != nullptr;
        if (actions) a_agent = actions[env];
        side = agent_dev ? (agent_dev[env] < 0 ? -1 : 1) : top->vs.agent;
    }
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    for (int i = threadIdx.x; i < WT_ENTRIES / 2; i += 64 * G::WPB)
        reinterpret_cast<uint32_t *>(wtab)[i] = reinterpret_cast<const SGX_KERNARG uint32_t *>(top->weights)[i];
    __syncthreads();   // from here on every wave works on its own games
    if (env >= P.n_envs) return;
    StepCarry carry = pool_carry(0);
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, PLAY_ROOT_COUNT>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr,
                                                                                                                      &carry, false, &top->play);
    int invalid = 0, moved = 0, reply = -1;
    if (!(carry.flags & F_OVER) && given && ((carry.flags & F_PLAYER_M1) ? -1 : 1) == side) {
        const int turn_before = carry.turn;
        carry.na = a_agent;
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, SGX_KERNARG PlayParams, PLAY_MOVE_COUNT>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr,
                                                                                                                          &carry, false, &top->play);
        if (carry.turn != turn_before) moved = VS_MOVED_AGENT;          // (every valid action on an unfinished game advances the counter)
        else invalid = 1;
    }
    if (!invalid && !(carry.flags & F_OVER) && ((carry.flags & F_PLAYER_M1) ? -1 : 1) != side) {
        const uint64_t r = sgx_rng(P.seed, (uint64_t)(P.env_id_offset + env), top->play.draw, STREAM_REPLY, (uint32_t)carry.turn);
        reply = draw_weighted(LW[slot], wsum[slot], wtab, (carry.flags & F_PLAYER_M1) ? 1 : 0, top->vs.see_all != 0, carry.na, r, lane);
        carry.na = reply;
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, PoolParams, PLAY_MOVE_GIVEN>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry,
                                                                                                             false);
        moved |= VS_MOVED_BOT;
    }
    store_results(top->play.out, env, lane, carry.flags);
    uint8_t *const o_invalid = top->vs.invalid_action, *const o_moved = top->vs.moved;
    int32_t *const o_reply = top->vs.reply_action;
    if (lane == 0 && o_invalid) o_invalid[env] = (uint8_t)invalid;
    if (lane == 0 && o_moved) o_moved[env] = (uint8_t)moved;
    if (lane == 0 && o_reply) o_reply[env] = reply;
    write_final_record(LW[slot], P, env, carry, lane);
}

}  // namespace
