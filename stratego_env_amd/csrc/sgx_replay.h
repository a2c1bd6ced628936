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
// Piece origins (sgx_set_replay_origins): the TRACK instantiations take ReplayParams with the two label tensors behind it, so that the
// untracked instantiations keep the kernel arguments -- and the code -- they had.
struct OriginArgs {
    const int16_t *in;    // int16 [src envs][2][cells], nullable: the labels the roots come with (NULL: every piece's own cell)
    int16_t *out;         // int16 [dst N][2][cells]
};
struct ReplayTrackedParams {
    KParams k;
    ReplayArgs rep;
    LeafParams leaf;
    OriginArgs org;
};
template <bool TRACK> struct ReplayParamsOf { using type = ReplayParams; };
template <> struct ReplayParamsOf<true> { using type = ReplayTrackedParams; };

// One chunk of a game's list: lane j of the game's LPG lanes takes entry t0 + j, one load instruction per chunk (contiguous 4 * LPG bytes
// with step_stride == 1, one entry per line otherwise).  Entries at or beyond `len` are not loaded.
// (t0 is 64 bits wide: with step_stride == 0 a list may be as long as an int32 counts, and c + LPG must not wrap)
__device__ __forceinline__ int replay_chunk(const int32_t *lane_entry0, const int64_t step_stride, const int64_t t0, const int lane, const int len) {
    int v = 0;
    if (t0 + lane < (int64_t)len) v = lane_entry0[t0 * step_stride];
    return v;
}

// PIECE ORIGINS (the TRACK instantiations; THE RULE is in the ABI header, restated in tests/origins_rule.py).
// Where the labels live: in REGISTERS.  A lane owns the cells lane + LPG * cc the frame's cell loops give it (leaf_sums, the never-moved
// bitmaps) and keeps one 32-bit word per cell -- player +1's label in the low half, player -1's in the high half -- CPL VGPRs per lane: 1 up to
// 8x8, 2 on 10x10 (HALF: 4), 4 on 15x15, 16 at 1,024 cells.  In LDS they would be 4 * cells bytes per game in a family whose LDS already
// sets the occupancy of the larger boards (Geo::WPB), read and written through the one LDS pipeline the step itself waits on.
// How a and b are found: by COMPARING the own-piece bytes of the lane's cells after the MOVE pass with an occupancy word the lane keeps
// (bit cc: player +1 stands on cell cc of this lane, bit 16 + cc: player -1; CPL <= 16 = SGX_MAX_CELLS / 64).  That is the rule as the
// header words it -- it never looks at the action, so both action forms, the no-op entry (no cell changes) and every ending go one way -- and
// it costs 2 * CPL LDS byte reads per applied move and no second decode.  The one label that changes its lane travels with one ballot
// and one cross-lane read inside the game's own lanes (glane: v_readlane on one-game waves, ds_bpermute below).
// Off the dependent chain: the next MOVE pass depends on the boards in LDS, the carry and the next entry, never on a label, and DS
// operations of a wave retire in issue order -- the reads of this update are issued before the next pass writes a board byte, and the
// label arithmetic is free to overlap that pass.  The root's given labels are requested with the record and the list's first chunks,
// before the barrier.
template <class G>
struct OriginLabels {
    static_assert(G::CPL <= 16, "the occupancy word holds 16 cells per lane and player");
    int lab[G::CPL];
    uint32_t occ;
};

// the given labels of root record s (or every cell's own index), requested before the barrier; what a cell without a piece holds is dropped
// in origins_start
template <class G>
__device__ __forceinline__ void origins_fetch(OriginLabels<G> &T, const int16_t *__restrict__ in, const int64_t s, const int lane) {
    constexpr int RC = G::RC;
#pragma unroll
    for (int cc = 0; cc < G::CPL; ++cc) {
        const int i = lane + G::LPG * cc;
        int v = i | (i << 16);
        if (in && i < RC) {
            const int16_t *p = in + s * (int64_t)(2 * RC);
            v = (int)(uint16_t)p[i] | ((int)(uint16_t)p[RC + i] << 16);
        }
        T.lab[cc] = v;
    }
    T.occ = 0;
}

// Start: a label stands where own(q)(root) has a piece, -1 everywhere else (the boards are in LDS: after the ROOT pass)
template <class G, int NB>
__device__ __forceinline__ void origins_start(const Lds<G, NB> &L, OriginLabels<G> &T, const int lane) {
    wave_sync<G>();
    const int8_t *own_p1 = L.b[B_PIECES], *own_m1 = L.b[B_PIECES + 1];
    uint32_t occ = 0;
#pragma unroll
    for (int cc = 0; cc < G::CPL; ++cc) {
        const int i = lane + G::LPG * cc;
        bool o_p1 = false, o_m1 = false;
        if (i < G::RC) { o_p1 = own_p1[i] != 0; o_m1 = own_m1[i] != 0; }
        T.lab[cc] |= (o_p1 ? 0 : 0xFFFF) | (o_m1 ? 0 : (int)0xFFFF0000u);
        occ |= ((uint32_t)o_p1 << cc) | ((uint32_t)o_m1 << (16 + cc));
    }
    T.occ = occ;
}

// One applied entry, mover index q: the cell the mover left (a) gives its label up, the cell it stands on now (b, if any) takes it, and
// an opponent's cell that is empty now loses its label.  All of it per game: the ballot and the read stay inside the game's lanes.
template <class G, int NB>
__device__ __forceinline__ void origins_move(const Lds<G, NB> &L, OriginLabels<G> &T, const int q, const int lane) {
    wave_sync<G>();                                                     // the boards are as the MOVE pass left them
    const int8_t *own_q = L.b[B_PIECES + q], *own_o = L.b[B_PIECES + 1 - q];
    const int sh_q = 16 * q, sh_o = 16 - sh_q;
    const uint32_t was = T.occ;
    uint32_t now = 0, arrive = 0;
    int moved = 0;
    bool leaves = false;
#pragma unroll
    for (int cc = 0; cc < G::CPL; ++cc) {
        const int i = lane + G::LPG * cc;
        bool n_q = false, n_o = false;
        if (i < G::RC) { n_q = own_q[i] != 0; n_o = own_o[i] != 0; }
        const bool w_q = (was >> (sh_q + cc)) & 1u, w_o = (was >> (sh_o + cc)) & 1u;
        if (w_q && !n_q) { moved = (T.lab[cc] >> sh_q) & 0xFFFF; leaves = true; T.lab[cc] |= (int)(0xFFFFu << sh_q); }
        if (w_o && !n_o) T.lab[cc] |= (int)(0xFFFFu << sh_o);
        arrive |= (uint32_t)(!w_q && n_q) << cc;
        now |= ((uint32_t)n_q << (sh_q + cc)) | ((uint32_t)n_o << (sh_o + cc));
    }
    T.occ = now;
    const unsigned long long from = gballot<G>(leaves);                 // one lane of the game, or none (the no-op entry: nothing arrives)
    const int v = glane<G>(moved, from ? __ffsll((long long)from) - 1 : 0);
#pragma unroll
    for (int cc = 0; cc < G::CPL; ++cc)
        if ((arrive >> cc) & 1u) T.lab[cc] = (int)(((uint32_t)T.lab[cc] & ~(0xFFFFu << sh_q)) | ((uint32_t)v << sh_q));
}

// Output: the labels of the final position, whole: int16 [2][cells] of slot env
template <class G>
__device__ __forceinline__ void origins_store(const OriginLabels<G> &T, int16_t *out, const int64_t env, const int lane) {
    constexpr int RC = G::RC;
    int16_t *o = out + env * (int64_t)(2 * RC);
#pragma unroll
    for (int cc = 0; cc < G::CPL; ++cc) {
        const int i = lane + G::LPG * cc;
        if (i < RC) {
            o[i] = (int16_t)(T.lab[cc] & 0xFFFF);
            o[RC + i] = (int16_t)((unsigned)T.lab[cc] >> 16);
        }
    }
}

// The frame (sgx_pool_frame.h) with the move taken from memory instead of a sampler: PLAY_ROOT_GIVEN stages the root, PLAY_MOVE_GIVEN applies
// one entry.  No mask is generated anywhere -- a replayed move asks what sgx_expand's asks, whether the next mover has a move at all.
// THE ACTION STREAM stays off the step's dependent chain: the game's lanes hold two chunks of LPG entries in two registers, `cur` and `nxt`,
// both requested before the workgroup stages its tables; a move takes its entry from `cur` with a cross-lane read inside the game's own lanes,
// and when a chunk is used up `nxt` becomes `cur` and the chunk after it is requested -- LPG moves before its first entry is needed.
// The loop is bounded by a COUNT, len <= max_len; it advances one entry per pass whether the entry was applied or passed over.
// TRACK: the instantiations that also carry piece labels (above), launched while dst has sgx_set_replay_origins set; every step they take on
// the game is the untracked kernel's, so every byte that one writes is written the same.
template <int R_, int C_, int VAR = 0, bool LEAF = false, bool TRACK = false>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (steps_waves_per_simd<Geo<R_, C_, VAR>, 8>())) void replay_kernel(const typename ReplayParamsOf<TRACK>::type SP) {
    using G = Geo<R_, C_, VAR>;
    using SPT = typename ReplayParamsOf<TRACK>::type;
    constexpr int KIND = 8;
    const SGX_KERNARG SPT *top = kernarg_of(SP);
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
    OriginLabels<G> track;
    if (env < P.n_envs) {
        fetch_root<G>(P, env, lane, in);
        if constexpr (TRACK) origins_fetch(track, top->org.in, P.src_index ? (int64_t)P.src_index[env] : env, lane);
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
    if constexpr (TRACK) origins_start(LW[slot], track, lane);
    int c = 0, m = 0, stop = 0;
    for (;;) {
        if (c >= len) break;                                            // the list is exhausted (stop = 0)
        if (carry.flags & F_OVER) { stop = 1; break; }                   // the game is over: what follows in the list is not read
        const SGX_KERNARG SPT *tp = top;
        int lane_t = lane, slot_t = slot;
        asm volatile("" : "+s"(tp), "+v"(lane_t), "+v"(slot_t));
        carry.na = __shfl(cur, c & (G::LPG - 1), G::LPG);               // entry c: held by lane c mod LPG of this game
        const int turn_before = carry.turn, mover = (carry.flags & F_PLAYER_M1) ? 1 : 0;
        env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, PoolParams, PLAY_MOVE_GIVEN>(tp->k, LW[slot_t], shared, obst_s, env, lane_t, in, nullptr, nullptr,
                                                                                                             &carry, false);
        const bool valid = carry.turn != turn_before;                   // (every valid action on an unfinished game advances the counter)
        if (!valid && !tp->rep.skip_invalid) { stop = 2; break; }        // entry c is the offending one: c stays
        m += valid ? 1 : 0;
        if constexpr (TRACK)
            if (valid) origins_move(LW[slot_t], track, mover, lane_t);
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
    if constexpr (TRACK) origins_store(track, top->org.out, env, lane);
}

}  // namespace
