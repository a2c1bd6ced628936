// sgx_children.h -- count_kernel, the offsets scan and children_kernel: every valid move of every root, pool to pool (sgx_count_moves,
// sgx_expand_all)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// The count: root slot i -> the number of valid moves of its mover (what gen_mask returns).  The frame (sgx_pool_frame.h) up to its ROOT
// pass, PLAY_ROOT_COUNT; no record is written.  k.n_envs = n_roots, k.src_boards / k.src_index = where the roots come from.
// ---------------------------------------------------------------------------------------------
struct CountParams {
    KParams k;
    int32_t *counts;
};

template <int R_, int C_, int VAR = 0>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (steps_waves_per_simd<Geo<R_, C_, VAR>, 8>())) void count_kernel(const CountParams SP) {
    using G = Geo<R_, C_, VAR>;
    constexpr int KIND = 8;
    const SGX_KERNARG CountParams *top = kernarg_of(SP);
    const SGX_KERNARG KParams &P = top->k;
    __shared__ Lds<G, ObsKind<KIND>::NIB_CH> LW[G::WPB * G::GPW];
    __shared__ alignas(16) uint8_t shared[shared_table_bytes<G, KIND>()];
    __shared__ alignas(16) uint8_t obst_s[G::OBST_BYTES + COMBAT_BYTES];
    const int lane = threadIdx.x & (G::LPG - 1), slot = threadIdx.x / G::LPG;
    const int64_t env = P.env_first + group_of_block(P) * (G::WPB * G::GPW) + slot;
    GameInput in = empty_input();
    if (env < P.n_envs) fetch_root<G>(P, env, lane, in);
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    __syncthreads();   // the one barrier: from here on every wave works on its own games
    if (env >= P.n_envs) return;
    StepCarry carry = pool_carry(0);
    env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, PoolParams, PLAY_ROOT_COUNT>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry, false);
    if (lane == 0) top->counts[env] = carry.na;
}

// ---------------------------------------------------------------------------------------------
// The offsets: an exclusive scan of the counts into int64, offsets[n] = the total.  Three plain passes, each a launch of its own, so that no
// workgroup ever waits on another: (1) the sum of every block of SCAN_BLOCK counts, (2) ONE workgroup turns the block sums into their
// exclusive scan, striding over them in chunks of SCAN_BLOCK with a running carry, (3) every block scans its counts again on top of its base.
// ---------------------------------------------------------------------------------------------
constexpr int SCAN_BLOCK = 256;             // counts per workgroup of passes 1 and 3 (one per thread); sums per chunk of pass 2

// inclusive scan of one value per thread over the SCAN_BLOCK threads of a workgroup; *total = the sum of all of them
__device__ inline int64_t block_scan_incl(int64_t v, int64_t *wave_sums, int64_t *total) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t up = __shfl_up(v, d, 64);
        if (l >= d) v += up;
    }
    __syncthreads();                        // (wave_sums may still be read by the call before this one)
    if (l == 63) wave_sums[w] = v;
    __syncthreads();
    int64_t base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < SCAN_BLOCK / 64; ++i) {
        const int64_t s = wave_sums[i];
        if (i < w) base += s;
        all += s;
    }
    *total = all;
    return v + base;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_sums_kernel(const int32_t *__restrict__ counts, int64_t *__restrict__ sums, const int64_t n) {
    __shared__ int64_t wave_sums[SCAN_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int64_t total;
    block_scan_incl(i < n ? (int64_t)counts[i] : 0, wave_sums, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_bases_kernel(int64_t *__restrict__ sums, const int64_t n_blocks) {
    __shared__ int64_t wave_sums[SCAN_BLOCK / 64];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < n_blocks; c0 += SCAN_BLOCK) {      // (uniform per workgroup: the barriers inside are reached by all)
        const int64_t i = c0 + threadIdx.x;
        const int64_t v = i < n_blocks ? sums[i] : 0;
        int64_t total;
        const int64_t incl = block_scan_incl(v, wave_sums, &total);
        if (i < n_blocks) sums[i] = carry + incl - v;
        carry += total;
    }
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_offsets_kernel(const int32_t *__restrict__ counts, const int64_t *__restrict__ sums,
                                                                   int64_t *__restrict__ offsets, const int64_t n) {
    __shared__ int64_t wave_sums[SCAN_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int64_t v = i < n ? (int64_t)counts[i] : 0, base = sums[blockIdx.x];
    int64_t total;
    const int64_t incl = block_scan_incl(v, wave_sums, &total);
    if (i < n) offsets[i] = base + incl - v;
    if (i == n - 1) offsets[n] = base + incl;
}

// ---------------------------------------------------------------------------------------------
// The children: slot j of dst = child first_child + j.  The frame (sgx_pool_frame.h): the game's lanes find root and rank from `offsets`,
// PLAY_ROOT_KTH generates the root's mask and takes the rank-th valid action, PLAY_MOVE_GIVEN applies it as a given action.
// ---------------------------------------------------------------------------------------------
struct ChildrenArgs {
    const int64_t *offsets;
    int32_t *parent, *action;
    ResultOut out;
    int64_t n_roots, first_child;
    int32_t actions_1d;
};
struct ChildrenParams {
    KParams k;
    ChildrenArgs ch;
    LeafParams leaf;      // read by the LEAF instantiation alone
};

// The root of child c: the LAST i in [0, n_roots) with offsets[i] <= c (roots without a move share their offset with the next one), found by
// the game's LPG lanes together: every round they probe LPG evenly spaced entries of [lo, hi) and keep the stretch behind the last probe that
// is <= c, so a round divides the range by LPG + 1 -- 4 rounds for 17 million roots with 64 lanes, 6 with 16.  Whatever the array holds: the
// probes lie inside [lo + 1, hi), the result inside [0, n_roots), and the round count is a constant.
template <class G>
__device__ __forceinline__ int64_t root_of_child(const int64_t *__restrict__ offsets, const int64_t n_roots, const int64_t c, const int lane) {
    int64_t lo = 0, hi = n_roots;
    for (int round = 0; round < 16; ++round) {                  // ((LPG + 1)^16 > 2^63 for LPG >= 16)
        const int64_t span = hi - lo;
        if (span <= 1) break;
        const int64_t step = (span + G::LPG) / (G::LPG + 1);    // >= 1, and LPG * step >= span - step: the last stretch is no longer than the others
        const int64_t p = lo + (int64_t)(lane + 1) * step;
        const bool le = p < hi && offsets[p] <= c;
        const int64_t n_le = __popcll(gballot<G>(le));          // (monotone offsets: the probes <= c are the first n_le)
        lo += n_le * step;                                      // <= the last probe inside the range: < hi
        hi = min(lo + step, hi);
    }
    return lo;
}

// flat spatial action in the perspective of the mover (player index qi) -> the absolute 1-D index sgx_expand takes: the inverse of Src1D, the
// map of the 1-D mask emission (impl:262-277 after the flip of impl:698-720).  `a` is a valid move: on the board, never the no-op.
template <class G>
__device__ inline int action_1d_of(const int a, const int qi) {
    constexpr int R = G::R, C = G::C, K = G::K, MPA = G::MPA;
    const int cell = a / K, ch = a - cell * K;
    int sr = cell / C, sc = cell - sr * C, er = sr, ec = sc;
    if (ch < R - 1) er = sr + ch + 1;
    else if (ch < 2 * (R - 1)) er = sr - (ch - (R - 1) + 1);
    else if (ch < 2 * (R - 1) + (C - 1)) ec = sc + (ch - 2 * (R - 1) + 1);
    else ec = sc - (ch - (2 * (R - 1) + (C - 1)) + 1);
    if (qi) { sr = R - 1 - sr; sc = C - 1 - sc; er = R - 1 - er; ec = C - 1 - ec; }
    return (sr * C + sc) * MPA + ((er != sr) ? er : R + ec);
}

template <int R_, int C_, int VAR = 0, bool LEAF = false>
__global__ __launch_bounds__((64 * Geo<R_, C_, VAR>::WPB), (steps_waves_per_simd<Geo<R_, C_, VAR>, 8>())) void children_kernel(const ChildrenParams SP) {
    using G = Geo<R_, C_, VAR>;
    constexpr int KIND = 8;
    const SGX_KERNARG ChildrenParams *top = kernarg_of(SP);
    const SGX_KERNARG KParams &P = top->k;
    __shared__ Lds<G, ObsKind<KIND>::NIB_CH> LW[G::WPB * G::GPW];
    __shared__ alignas(16) uint8_t shared[shared_table_bytes<G, KIND>()];
    __shared__ alignas(16) uint8_t obst_s[G::OBST_BYTES + COMBAT_BYTES];
    const int lane = threadIdx.x & (G::LPG - 1), slot = threadIdx.x / G::LPG;
    const int64_t env = P.env_first + group_of_block(P) * (G::WPB * G::GPW) + slot;     // the slot of dst (k.n_envs = n_children)
    // root, rank and the root's record: all requested before the workgroup stages its tables
    GameInput in = empty_input();
    int64_t root = -1;
    int rank = 0;
    if (env < P.n_envs) {
        const int64_t *offsets = top->ch.offsets;
        const int64_t n_roots = top->ch.n_roots, c = top->ch.first_child + env;
        if (n_roots > 0 && c < offsets[n_roots]) {
            const int64_t i = root_of_child<G>(offsets, n_roots, c, lane);
            const int64_t k = c - offsets[i];
            if (k >= 0 && k < 0x7fffffff) {                     // (anything else: offsets that do not belong to these roots)
                root = i;
                rank = (int)k;
                fetch_root<G>(P, i, lane, in);
            }
        }
    }
    stage_tables<G, KIND>(P, shared, obst_s, threadIdx.x, 64 * G::WPB);
    __syncthreads();   // from here on every wave works on its own games
    if (env >= P.n_envs) return;
    int32_t *const o_parent = top->ch.parent, *const o_action = top->ch.action;
    StepCarry carry = pool_carry(rank);                         // the rank in, the rank-th valid action out (-1: the root has no such move)
    if (root >= 0)
        env_step<R_, C_, KIND, false, false, VAR, 1, false, SGX_KERNARG KParams, PoolParams, PLAY_ROOT_KTH>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry, false);
    const int a = carry.na;
    if (root < 0 || a < 0) {                                    // no child: dst's record stays what it was
        if (lane == 0 && o_parent) o_parent[env] = -1;
        if (lane == 0 && o_action) o_action[env] = -1;
        return;
    }
    const int qi = (carry.flags & F_PLAYER_M1) ? 1 : 0;         // the root's mover
    env_step<R_, C_, KIND, false, false, VAR, 2, false, SGX_KERNARG KParams, PoolParams, PLAY_MOVE_GIVEN>(P, LW[slot], shared, obst_s, env, lane, in, nullptr, nullptr, &carry, false);
    if (lane == 0 && o_parent) o_parent[env] = (int32_t)root;
    if (lane == 0 && o_action) o_action[env] = top->ch.actions_1d ? action_1d_of<G>(a, qi) : a;
    if constexpr (LEAF) store_results_leaf(LW[slot], top->ch.out, top->leaf, env, lane, carry.flags);
    else store_results(top->ch.out, env, lane, carry.flags);      // what the step that made the child reports
    write_final_record(LW[slot], P, env, carry, lane);
}

}  // namespace
