// sgx_determinize_weighted.h -- determinize_weighted_kernel: sgx_determinize with a belief (sgx_determinize_weighted)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip after sgx_aux_kernels.h (one translation unit).
#pragma once

namespace {

// Record i of `dst` becomes record src_idx[i] of `src` with the hidden pieces of the observer's opponent dealt again by the caller's
// per-cell type weights.  THE RULE is in include/stratego_mi355x.h (tests/determinize_weighted_rule.py restates it): the hidden types
// are dealt instance by instance -- flags, bombs, then 10 .. 1 -- each onto a free hidden cell drawn with probability proportional to
// the weight of (type, cell), flags and bombs onto never-moved cells only; a draw whose candidates all weigh 0 falls back to a uniform
// one and counts in off_belief.
// The shape of determinize_kernel: one wave per record, four per workgroup, the record layout as arguments (one kernel for every
// board of up to 1,024 cells), the record staged whole in LDS before anything is written and stored as whole 16-byte lines.
// Lane l owns cells l, l + 64, ... (at most 16): bit k of `freeb` / `stillb` says that cell l + 64 k is a free hidden cell / a
// never-moved hidden cell, nibble k of `dealt` is the type the cell received.  Per wave in LDS: the record image | the weight row of
// the type being dealt (uint16 per cell, clamped, read from the table ONCE per type with coalesced 2-byte loads and reused by all of
// the type's instances).  Every draw is two walks over the ceil(cells / 64) slices: the lanes' own sums and one DPP reduction for W,
// then per slice a DPP inclusive scan on top of the running base and a ballot for the first prefix above x.  No atomics, no scratch.
__host__ __device__ constexpr int detw_lds_bytes(int rec_bytes, int cells) { return rec_bytes + (((cells + 63) & ~63) * 2); }

constexpr int DETW_WEIGHT_MAX = 4095, DETW_TYPES = 12;

__global__ __launch_bounds__(256) void determinize_weighted_kernel(int8_t *dst, const int8_t *src, const int32_t *__restrict__ src_idx,
                                                                   const uint16_t *__restrict__ belief, const int64_t belief_stride,
                                                                   int32_t *__restrict__ hidden, int32_t *__restrict__ off_belief, const int64_t n,
                                                                   const uint64_t seed, const int64_t env_id_offset, const uint64_t draw,
                                                                   const int observer, const int S, const int st_off, const int sb,
                                                                   const int sc_off, const int rec_bytes, const int cells) {
    extern __shared__ int4 detw_lds[];
    const int64_t i = blockIdx.x * (int64_t)(blockDim.x / 64) + threadIdx.x / 64;
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    uint8_t *img = reinterpret_cast<uint8_t *>(detw_lds) + (threadIdx.x / 64) * detw_lds_bytes(rec_bytes, cells);
    uint16_t *wrow = reinterpret_cast<uint16_t *>(img + rec_bytes);                 // [ceil(cells / 64) * 64]
    const int64_t s_rec = src_idx ? src_idx[i] : i;
    const int4 *s = reinterpret_cast<const int4 *>(src + s_rec * rec_bytes);
    for (int q = lane; q < rec_bytes / 16; q += 64) reinterpret_cast<int4 *>(img)[q] = s[q];
    wave_sync<Geo<10, 10>>();
    const int flags = reinterpret_cast<const int4 *>(img + sc_off)[0].y;
    const int opp = (observer ? observer : ((flags & F_PLAYER_M1) ? -1 : 1)) == 1 ? 1 : 0;      // player index of the observer's opponent
    uint8_t *pieces = img + (B_PIECES + opp) * S;
    const uint8_t *po = img + (B_PO + opp) * S;
    const uint32_t *still = reinterpret_cast<const uint32_t *>(img + st_off + opp * sb);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int slices = (cells + 63) >> 6;
    // H and A as bits of the lanes that own the cells; a flag or a bomb on a moved hidden cell refuses the record
    uint32_t hidb = 0, stillb = 0;
    int nH = 0;
    bool bad = false;
    for (int k = 0; k < slices; ++k) {
        const int cell = 64 * k + lane, cc = cell < cells ? cell : 0;
        const int t = pieces[cc], p = po[cc];
        const uint32_t w = still[cc >> 5];
        const bool hid = cell < cells && t != 0 && p == SP_UNKNOWN;
        const bool st = hid && ((w >> (cell & 31)) & 1u) != 0;
        const bool fb = hid && (t == SP_FLAG || t == SP_BOMB);
        hidb |= (uint32_t)hid << k;
        stillb |= (uint32_t)st << k;
        nH += __popcll(__ballot(hid));
        bad = bad || __ballot(fb && !st) != 0;
    }
    int n_off = 0;
    if (!bad && nH > 0) {
        const uint64_t g = (uint64_t)(env_id_offset + i);
        const uint16_t *tb = belief + s_rec * belief_stride + (int64_t)opp * DETW_TYPES * cells;
        uint32_t freeb = hidb;
        uint64_t dealt = 0;
        uint32_t j = 0;
        for (int ti = 0; ti < DETW_TYPES; ++ti) {
            const int t = ti == 0 ? SP_FLAG : ti == 1 ? SP_BOMB : 12 - ti;             // 11, 12, 10, 9, ..., 1
            int c_t = 0;                                                                // instances of the type on H (the true pieces are still in the image)
            for (int k = 0; k < slices; ++k) {
                const int cell = 64 * k + lane;
                c_t += __popcll(__ballot(((hidb >> k) & 1u) != 0 && pieces[cell < cells ? cell : 0] == t));
            }
            if (c_t == 0) continue;
            wave_sync<Geo<10, 10>>();                                                   // (the draws of the type before have read their row)
            const uint16_t *row = tb + (int64_t)(t - 1) * cells;
            for (int k = 0; k < slices; ++k) {
                const int cell = 64 * k + lane;
                const int w = cell < cells ? (int)row[cell] : 0;
                wrow[cell] = (uint16_t)(w < DETW_WEIGHT_MAX ? w : DETW_WEIGHT_MAX);
            }
            wave_sync<Geo<10, 10>>();
            const uint32_t allowed = t >= SP_FLAG ? stillb : 0xFFFFFFFFu;               // flags and bombs: never-moved cells only
            for (int inst = 0; inst < c_t; ++inst, ++j) {
                const uint32_t cand = freeb & allowed;
                int mine = 0, m = 0;
                for (int k = 0; k < slices; ++k) {
                    const bool c = ((cand >> k) & 1u) != 0;
                    mine += c ? (int)wrow[64 * k + lane] : 0;
                    m += __popcll(__ballot(c));
                }
                const uint32_t W = (uint32_t)__builtin_amdgcn_readlane(gscan_incl<Geo<10, 10>>(mine), 63);
                const uint64_t r = sgx_rng(seed, g, draw, STREAM_DETERMINIZE_WEIGHTED, j);
                int cell = -1;
                if (W > 0) {
                    const int x = (int)rng_below(r, W);
                    int base = 0;
                    for (int k = 0; k < slices; ++k) {
                        const int w = ((cand >> k) & 1u) ? (int)wrow[64 * k + lane] : 0;
                        const int incl = base + gscan_incl<Geo<10, 10>>(w);
                        const unsigned long long above = __ballot(incl > x);          // (the first lane above x holds a weight > 0: a candidate)
                        if (above) { cell = 64 * k + __ffsll((long long)above) - 1; break; }
                        base = __builtin_amdgcn_readlane(incl, 63);
                    }
                } else {
                    int kk = (int)rng_below(r, (uint32_t)m);
                    for (int k = 0; k < slices; ++k) {
                        const unsigned long long b = __ballot(((cand >> k) & 1u) != 0);
                        const int nb = __popcll(b);
                        if (kk < nb) {
                            const unsigned long long hit = __ballot(((b >> lane) & 1ull) != 0 && __popcll(b & below) == kk);
                            cell = 64 * k + __ffsll((long long)hit) - 1;
                            break;
                        }
                        kk -= nb;
                    }
                    ++n_off;
                }
                if (cell >= 0 && lane == (cell & 63)) {
                    freeb &= ~(1u << (cell >> 6));
                    dealt |= (uint64_t)t << (4 * (cell >> 6));
                }
            }
        }
        wave_sync<Geo<10, 10>>();
        for (int k = 0; k < slices; ++k) {
            const int nt = (int)((dealt >> (4 * k)) & 15u);
            if (((hidb >> k) & 1u) && nt) pieces[64 * k + lane] = (uint8_t)nt;
        }
        wave_sync<Geo<10, 10>>();
    }
    int4 *d = reinterpret_cast<int4 *>(dst + i * (int64_t)rec_bytes);
    for (int q = lane; q < rec_bytes / 16; q += 64) d[q] = reinterpret_cast<const int4 *>(img)[q];
    if (lane == 0) {
        if (hidden) hidden[i] = bad ? -1 : nH;
        if (off_belief) off_belief[i] = n_off;
    }
}

}  // namespace
