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

// ---------------------------------------------------------------------------------------------
// Leaf values (sgx_set_leaf_values): a position that is not over reports v(+1), v(-1) instead of 0, 0 -- THE RULE is in the ABI header,
// restated in tests/leaf_values_rule.py.  Every kernel of the family has a second instantiation, LEAF, that the host launches when dst has a
// table set; the instantiations without it are the code they were (profiles/leaf_values_kernel_notes.txt).
// The table is the handle's device copy of the caller's int16 [2][14][cells], LEAF_ROWS rows of `cells` entries with zeros behind the 28 the
// caller gave: a board byte is masked to 4 bits before it becomes a row, so whatever a record holds the reads stay inside the buffer.
// It is read through L2, not staged into LDS: a game reads two entries per piece (at most 160 of the 2,800 on 10x10), a workgroup of
// sgx_expand_all lives for eight children, and the LDS of these kernels is what sets their occupancy on the larger boards.
// ---------------------------------------------------------------------------------------------
constexpr int LEAF_ROWS = 32, LEAF_HALF = 14;        // rows of the device buffer; rows of one half of the table ("mine", then "theirs")
struct LeafParams {
    const int16_t *table;
    int32_t limit, denom, see_all, reserved;
};

// S(+1), S(-1) of the position in the wave's LDS, in every lane of the game: a game's lanes walk its cells, CPL per lane, and reduce
// their two partial sums over the game's own lanes (DPP rows and a read inside the game: nothing depends on a wave-mate's lanes)
template <class G, int NB>
__device__ __forceinline__ void leaf_sums(const Lds<G, NB> &L, const int16_t *__restrict__ table, const bool see_all, const int lane, int &s_p1, int &s_m1) {
    constexpr int RC = G::RC;
    const int8_t *own_p1 = L.b[B_PIECES], *own_m1 = L.b[B_PIECES + 1];
    const int8_t *seen_p1 = L.b[see_all ? B_PIECES : B_PO], *seen_m1 = L.b[(see_all ? B_PIECES : B_PO) + 1];   // what the opponent takes them for
    const int16_t *__restrict__ mine = table, *__restrict__ theirs = table + LEAF_HALF * RC;
    int a = 0, b = 0;
#pragma unroll
    for (int cc = 0; cc < G::CPL; ++cc) {
        const int i = lane + G::LPG * cc;
        if (i < RC) {
            const int t_p1 = own_p1[i] & 15, t_m1 = own_m1[i] & 15, d_p1 = seen_p1[i] & 15, d_m1 = seen_m1[i] & 15;
            const int j = RC - 1 - i;                                   // the cell in -1's perspective
            if (t_p1) a += mine[t_p1 * RC + i];
            if (d_m1) a -= theirs[d_m1 * RC + j];
            if (t_m1) b += mine[t_m1 * RC + j];
            if (d_p1) b -= theirs[d_p1 * RC + i];
        }
    }
    s_p1 = glane<G>(gscan_incl<G>(a), G::LPG - 1);
    s_m1 = glane<G>(gscan_incl<G>(b), G::LPG - 1);
}

// store_results of the LEAF instantiations: the same, but for the rewards of a position that is not over
template <class G, int NB, class RO, class LP>
__device__ __forceinline__ void store_results_leaf(const Lds<G, NB> &L, const RO &out, const LP &leaf, const int64_t env, const int lane, const int flags) {
    const bool over = (flags & F_OVER) != 0, end_invalid = over && (flags & F_END_INVALID);
    float rew_p1 = 0.f, rew_m1 = 0.f;
    if (over && !end_invalid) {
        const int w = (flags & F_WIN_P1) ? 1 : (flags & F_WIN_M1) ? -1 : 0;
        rew_p1 = w == 0 ? 1e-4f : (float)w;     // impl:838-840
        rew_m1 = w == 0 ? 1e-4f : (float)-w;
    }
    if (!over) {                                // (per game: wave-mates that are over skip it)
        wave_sync<G>();                         // the boards are as the last pass left them
        int s_p1, s_m1;
        leaf_sums(L, leaf.table, leaf.see_all != 0, lane, s_p1, s_m1);
        const int limit = leaf.limit;
        const float denom = (float)leaf.denom;
        rew_p1 = (float)min(max(s_p1, -limit), limit) / denom;
        rew_m1 = (float)min(max(s_m1, -limit), limit) / denom;
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
