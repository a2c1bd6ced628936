// lane_harness.hip -- TEST INFRASTRUCTURE: the lane-per-game logic of stratego_env_amd/csrc/sgx_lane.h compiled for the HOST
// (hipcc --offload-host-only), so that tests/test_lane_logic_cpu.py can play it against the CPU oracle step by step without a GPU.
// Nothing in the product loads this library; the device kernel that wraps the same functions is tested on the GPU (-m gpu).
// One entry point per board size: an env.step() on the reference's int64 [34,R,C] state, like so_env_step3 of the oracle.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <string.h>

#include "stratego_mi355x.h"
#include "sgx_layout.h"
#include "sgx_lane.h"

namespace {

template <class G>
void from_state(const int64_t *st, int player, LaneGame &g, uint16_t *ev, uint32_t &obst) {
    constexpr int RC = G::RC, C = G::C;
    memset(&g, 0, sizeof(g));
    obst = 0;
    for (int i = 0; i < RC; ++i) {
        g.pc[0] = lg_set(g.pc[0], i, (int)st[0 * RC + i]);
        g.pc[1] = lg_set(g.pc[1], i, (int)st[1 * RC + i]);
        g.po[0] = lg_set(g.po[0], i, (int)st[3 * RC + i]);
        g.po[1] = lg_set(g.po[1], i, (int)st[4 * RC + i]);
        if (st[2 * RC + i]) obst |= 1u << i;
        if (st[32 * RC + i]) g.still[0] |= 1u << i;
        if (st[33 * RC + i]) g.still[1] |= 1u << i;
    }
    g.turn = (int)st[5 * RC + 0];
    g.flags = (st[5 * RC + 1] ? F_OVER : 0) | (st[5 * RC + 2] > 0 ? F_WIN_P1 : st[5 * RC + 2] < 0 ? F_WIN_M1 : 0) | (st[5 * RC + C + 1] ? F_END_INVALID : 0) |
              (player < 0 ? F_PLAYER_M1 : 0);
    g.max_turns = (int)st[5 * RC + C];
    for (int pl = 0; pl < 2; ++pl) {
        int found = 0, pair = 0;
        for (int i = 0; i < RC && found < 2; ++i)
            if (st[(6 + pl) * RC + i]) { pair |= G::make_pair(i, (int)st[(6 + pl) * RC + i]) << (16 * found); ++found; }
        if (pl) g.rp1 = pair; else g.rp0 = pair;
    }
    for (int key = 0; key < 24; ++key)
        for (int i = 0; i < RC; ++i)
            if (st[(8 + key) * RC + i] > 0 && g.n_events < (int)G::EVL_MAX)
                ev[g.n_events++] = (uint16_t)((((int)st[(8 + key) * RC + i] - 1) << G::EV_COUNT_SHIFT) | (key << G::CELL_BITS) | i);
}

template <class G>
void to_state(const LaneGame &g, const uint16_t *ev, uint32_t obst, int64_t *st) {
    constexpr int RC = G::RC, C = G::C;
    memset(st, 0, sizeof(int64_t) * 34 * RC);
    for (int i = 0; i < RC; ++i) {
        st[0 * RC + i] = lg_nib(g.pc[0], i); st[1 * RC + i] = lg_nib(g.pc[1], i);
        st[3 * RC + i] = lg_nib(g.po[0], i); st[4 * RC + i] = lg_nib(g.po[1], i);
        st[2 * RC + i] = (obst >> i) & 1u;
        st[32 * RC + i] = (g.still[0] >> i) & 1u; st[33 * RC + i] = (g.still[1] >> i) & 1u;
    }
    st[5 * RC + 0] = g.turn;
    st[5 * RC + 1] = (g.flags & F_OVER) ? 1 : 0;
    st[5 * RC + 2] = (g.flags & F_WIN_P1) ? 1 : (g.flags & F_WIN_M1) ? -1 : 0;
    st[5 * RC + C] = g.max_turns;
    st[5 * RC + C + 1] = (g.flags & F_END_INVALID) ? 1 : 0;
    for (int pl = 0; pl < 2; ++pl) {
        const int rp = pl ? g.rp1 : g.rp0;
        for (int k = 0; k < 2; ++k) {
            const int pr = (rp >> (16 * k)) & 0xFFFF;
            if (G::pair_code(pr) != 0) st[(6 + pl) * RC + G::pair_cell(pr)] = G::pair_code(pr);
        }
    }
    for (int i = 0; i < g.n_events; ++i) {
        const int e = ev[i], key = (e >> G::CELL_BITS) & 31, cell = e & G::CELL_MASK;
        st[(8 + key) * RC + cell] = (e >> G::EV_COUNT_SHIFT) + 1;
    }
}

// What a call may add to a plain step (lh_play): auto-reset, from sampled setups (piece_counts / usable_rows) or, n_pool > 0, from a start
// pool of n_pool positions [34,R,C] with their movers, packed into records by lane_store; *start_index receives the pool index.
struct Restart {
    int auto_reset, usable_rows, n_pool, pool_flags;
    const int32_t *piece_counts;
    uint64_t seed, gid;
    const int64_t *pool_states;
    const int32_t *pool_players;
    int32_t *start_index;
};

// One env.step() (mode 0) or observation (mode 1) on `state` / `*player` (both updated): lane_play of sgx_lane.h, the function the device
// kernels call, as game 0 of a host KParams whose result pointers are host scalars.  The game is number 0 of env `gid`.  out_flags: bit 0
// invalid action, bit 1 done, bit 2 ending invalid; mask: uint8 [NA] of the next mover; kth: the flat index of the k-th valid action of
// that mask for k = k_sample; rewards for +1 / -1 (mode 1 writes no results, like the kernel).  The record round trip (lane_store ->
// lane_load on the packed layout) is part of every call.
template <class G>
int step(int64_t *state, int *player_io, int action, const int32_t *pos, int step_flags, int mode, int max_events, int k_sample, uint8_t *mask_out,
         int *nvalid_out, int *kth_out, float *rewards, int *out_flags, const Restart &rs = Restart{}) {
    constexpr int REC = 256;                                // bytes of a record of a board of at most 16 cells
    if (rs.n_pool > 16) return -2;
    LaneGame g0;
    alignas(16) uint8_t rec[REC], pool[16 * REC];
    memset(rec, 0, sizeof(rec));
    memset(pool, 0, sizeof(pool));
    uint16_t *ev = reinterpret_cast<uint16_t *>(rec + G::EVL_OFF);
    uint32_t obst, pool_obst;
    from_state<G>(state, *player_io, g0, ev, obst);
    lane_store<G>(g0, rec);
    for (int j = 0; j < rs.n_pool; ++j) {
        from_state<G>(rs.pool_states + (size_t)j * 34 * G::RC, rs.pool_players[j], g0, reinterpret_cast<uint16_t *>(pool + j * REC + G::EVL_OFF), pool_obst);
        lane_store<G>(g0, pool + j * REC);
    }
    LaneGame g;
    lane_load<G>(g, rec);                                   // through the packed record, as the kernel sees a game
    uint8_t combat[256];
    for (int a = 0; a < 16; ++a)
        for (int d = 0; d < 16; ++d) combat[16 * a + d] = (uint8_t)combat_outcome(a, d);
    alignas(8) float rew[2] = {0.f, 0.f};
    uint8_t done = 0, invalid = 0, end_invalid = 0;
    int8_t player = 0;
    KParams P;
    memset(&P, 0, sizeof(P));
    P.usable_rows = rs.usable_rows; P.rec_bytes = REC; P.max_events = max_events; P.n_envs = 1; P.seed = rs.seed; P.env_id_offset = (int64_t)rs.gid;
    for (int t = 0; t < 12; ++t) P.piece_counts[t] = rs.piece_counts ? rs.piece_counts[t] : 0;
    P.io.reward_dev = rew; P.io.done_dev = &done; P.io.invalid_action_dev = &invalid; P.io.ending_invalid_dev = &end_invalid; P.io.player_dev = &player;
    P.io.auto_reset = rs.auto_reset; P.io.flags = step_flags;
    const PoolParams PP{reinterpret_cast<const int8_t *>(pool), rs.n_pool, rs.pool_flags, rs.start_index};
    const int4 p4 = make_int4(pos[0], pos[1], pos[2], pos[3]);
    uint32_t V[G::K - 1];
    const int nvalid = mode       ? lane_play<G, true, false>(g, ev, V, P, &PP, action, p4, obst, combat, 0, 0, true).nvalid
                       : rs.n_pool ? lane_play<G, false, true>(g, ev, V, P, &PP, action, p4, obst, combat, 0, 0, true).nvalid
                                   : lane_play<G, false, false>(g, ev, V, P, &PP, action, p4, obst, combat, 0, 0, true).nvalid;
    rewards[0] = rew[0]; rewards[1] = rew[1];
    *out_flags = (invalid ? 1 : 0) | (done ? 2 : 0) | (end_invalid ? 4 : 0);
    uint32_t *mw = reinterpret_cast<uint32_t *>(mask_out);
    *kth_out = lane_emit_mask<G>(V, nvalid == 0, k_sample, [&](int j, uint32_t d) { mw[j] = d; });
    *nvalid_out = nvalid;
    lane_store<G>(g, rec);
    LaneGame g2;
    lane_load<G>(g2, rec);
    to_state<G>(g2, ev, obst, state);
    *player_io = player;
    return 0;
}

template <class G>
int sample(const int32_t *piece_counts, int usable_rows, uint64_t seed, uint64_t gid, uint64_t j, int max_turns, uint32_t obst, int64_t *state) {
    LaneGame g;
    memset(&g, 0, sizeof(g));
    uint16_t ev[16] = {0};
    lane_sample_boards<G>(g, nullptr, 0, usable_rows, piece_counts, seed, gid, j);
    g.max_turns = max_turns;
    to_state<G>(g, ev, obst, state);
    return 0;
}

}  // namespace

#define LH_API extern "C" __attribute__((visibility("default")))
// the board sizes the harness is instantiated for: `return CALL;` with G = the board's Geo, -1 for any other size
#define LH_ON_BOARD(CALL)                                        \
    if (R == 3 && C == 4) { using G = Geo<3, 4>; return CALL; }  \
    if (R == 4 && C == 4) { using G = Geo<4, 4>; return CALL; }  \
    if (R == 4 && C == 3) { using G = Geo<4, 3>; return CALL; }  \
    return -1

LH_API int lh_step(int R, int C, int64_t *state, int *player_io, int action, const int32_t *pos, int step_flags, int mode, int max_events,
                   int k_sample, uint8_t *mask_out, int *nvalid_out, int *kth_out, float *rewards, int *out_flags) {
    LH_ON_BOARD(step<G>(state, player_io, action, pos, step_flags, mode, max_events, k_sample, mask_out, nvalid_out, kth_out, rewards, out_flags));
}

// lh_step (mode 0, spatial actions) with auto-reset: see Restart
LH_API int lh_play(int R, int C, int64_t *state, int *player_io, int action, int step_flags, int max_events, uint8_t *mask_out, float *rewards, int *out_flags,
                   int usable_rows, const int32_t *piece_counts, uint64_t seed, uint64_t gid, int n_pool, int pool_flags, const int64_t *pool_states,
                   const int32_t *pool_players, int32_t *start_index) {
    const int32_t pos[4] = {0, 0, 0, 0};
    int nvalid, kth;
    const Restart rs{1, usable_rows, n_pool, pool_flags, piece_counts, seed, gid, pool_states, pool_players, start_index};
    LH_ON_BOARD(step<G>(state, player_io, action, pos, step_flags, 0, max_events, 0, mask_out, &nvalid, &kth, rewards, out_flags, rs));
}

LH_API int lh_sample(int R, int C, const int32_t *piece_counts, int usable_rows, uint64_t seed, uint64_t gid, uint64_t j, int max_turns,
                     uint32_t obst, int64_t *state) {
    LH_ON_BOARD(sample<G>(piece_counts, usable_rows, seed, gid, j, max_turns, obst, state));
}
