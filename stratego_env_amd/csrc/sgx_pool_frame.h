// sgx_pool_frame.h -- the frame of the pool-to-pool kernels: playout_kernel, replay_kernel, count_kernel, children_kernel
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// THE FRAME.  A pool-to-pool kernel reads root records from one pool (k.src_boards / k.src_index) and writes whole records into another
// (k.boards).  One wave per game (two games per wave with VAR = 2, Geo's own two or four on boards of up to 32 cells), the no-observation
// kind, steps_kernel's launch bounds.  Every kernel of the family has this shape:
//   1. fetch_root requests the root's record -- with whatever else the kernel reads once (a list's first chunks, the offsets) -- BEFORE the
//      workgroup stages its tables (stage_tables), so that the two round trips overlap; then the one barrier, after which every wave
//      works on its own games: no barrier in a loop, no atomics, nothing between waves.  Games that share a wave end at different times:
//      every condition after the barrier is per game, so a finished game's lanes are masked off while the wave goes on with the others
//      (the divergence a ragged batch already has at env >= n_envs).
//   2. a ROOT pass of env_step (play_is_root) stages the record into the wave's LDS and fills the carry (pool_carry).  It is a copy of the
//      step of its own, not the first trip of the loop, so that the record's registers are dead in the loop.
//   3. MOVE passes play on with the boards in LDS and the scalars in the carry, as steps_kernel does; nothing leaves the wave meanwhile.
//      A loop of them opens every trip with an empty asm statement that takes fresh copies of the kernarg pointer, the lane and the slot:
//      the step's reads of the parameters start there, and what a step derives from the lane is recomputed in every step (steps_kernel).
//   4. store_results and write_final_record: what a step on the final position reports, and the position, whole.
// The three __shared__ arrays stay three declarations in each kernel: bundled into one struct they take 16 bytes of padding in every one.

// The result tensors every kernel of the family that ends in a position offers (each nullable)
struct ResultOut {
    float *reward;
    uint8_t *done, *ending_invalid;
    int8_t *player;
};

__device__ __forceinline__ GameInput empty_input() {
    const int4 zero4 = make_int4(0, 0, 0, 0);
    return GameInput{zero4, zero4, zero4, 0, nullptr};
}

// the root's record: slot i of the source (source_record), requested as load_record requests it
template <class G, class KP>
__device__ __forceinline__ void fetch_root(const KP &P, const int64_t i, const int lane, GameInput &in) {
    in.src = reinterpret_cast<const int4 *>(source_record(P, i));
    load_record<G>(P, in.src, lane, in.rq0, in.rq1);
}

// the carry a ROOT pass fills; na: what the pass takes there (PLAY_ROOT_KTH's rank) or what the kernel reads where no pass ran
__device__ __forceinline__ StepCarry pool_carry(const int na) {
    return StepCarry{/* turn, flags, max_turns, game_no */ 0, 0, 0, 0, /* n_events, rp0, rp1 */ 0, 0, 0, na, /* dirty */ false, nullptr, nullptr, nullptr, /* slot */ 0};
}

// what a step on the position with these flags reports (env_step's rewards / dones)
template <class RO>
__device__ __forceinline__ void store_results(const RO &out, const int64_t env, const int lane, const int flags) {
    const bool over = (flags & F_OVER) != 0, end_invalid = over && (flags & F_END_INVALID);
    float rew_p1 = 0.f, rew_m1 = 0.f;
    if (over && !end_invalid) {
        const int w = (flags & F_WIN_P1) ? 1 : (flags & F_WIN_M1) ? -1 : 0;
        rew_p1 = w == 0 ? 1e-4f : (float)w;     // impl:838-840
        rew_m1 = w == 0 ? 1e-4f : (float)-w;
    }
    float *const o_reward = out.reward;
    uint8_t *const o_done = out.done, *const o_end_invalid = out.ending_invalid;
    int8_t *const o_player = out.player;
    if (lane < 2 && o_reward) o_reward[2 * env + lane] = lane ? rew_m1 : rew_p1;
    if (lane == 0 && o_done) o_done[env] = over ? 1 : 0;
    if (lane == 0 && o_end_invalid) o_end_invalid[env] = end_invalid ? 1 : 0;
    if (lane == 0 && o_player) o_player[env] = (int8_t)((flags & F_PLAYER_M1) ? -1 : 1);
}

// the position the carry and the wave's LDS hold, whole, into slot env of dst (a copy of the root where nothing was played)
template <class G, int NB, class KP>
__device__ __forceinline__ void write_final_record(Lds<G, NB> &L, const KP &P, const int64_t env, const StepCarry &carry, const int lane) {
    write_record(L, P.boards + env * (int64_t)P.rec_bytes, P.rec_bytes, make_int4(carry.turn, carry.flags, carry.max_turns, carry.game_no),
                 make_int4(carry.n_events, carry.rp0, carry.rp1, 0), carry.n_events, lane);
}

}  // namespace
