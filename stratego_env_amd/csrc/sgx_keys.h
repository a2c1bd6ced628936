// sgx_keys.h -- keys_kernel: one 64-bit (or 128-bit) position key per packed record, state view or information-set view (sgx_state_keys)
// Part of libstratego_mi355x.so; included by stratego_mi355x.hip in this order (one translation unit).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// THE RULE lives in include/stratego_mi355x.h (sgx_state_keys) and is restated in numpy in tests/keys_rule.py: the key of a position is
// sm_fin of the XOR of one hash per FEATURE of the reference state -- a non-zero (layer, cell, value), a scalar, the mover, the observer.
// A record holds every feature somewhere in its bytes (what export_from_image unfolds into the 34 layers), so the key is a function of the
// record bytes alone: Geo::LPG lanes per record read it as 16-byte quads (load_record), each lane hashes the features its own quads hold,
// and XOR -- which does not care about the order -- combines them, first in the lane's registers and then across the record's lanes.
// No LDS, no table, no barrier, no atomic; one lane stores 8 or 16 bytes.
// ---------------------------------------------------------------------------------------------
constexpr uint64_t KEY_SALT0 = 0x5347584B45595330ull, KEY_SALT1 = 0x5347584B45595331ull;      // "SGXKEYS0" / "SGXKEYS1"
constexpr uint64_t KEY_GOLD = 0x9E3779B97F4A7C15ull;
constexpr int KEY_SLOTS = 1024;             // slots of a layer: slot = layer * KEY_SLOTS + cell (SGX_MAX_CELLS cells); layer 5 holds the scalars
enum { KEY_SC_OVER = 0, KEY_SC_WINNER = 1, KEY_SC_END_INVALID = 2, KEY_SC_MOVER = 3, KEY_SC_TURN = 4, KEY_SC_MAX_TURNS = 5, KEY_SC_OBSERVER = 6 };
constexpr int KEYS_THREADS = 256;           // threads per workgroup: 4 / 8 / 16 records

struct KeysParams {
    const int8_t *boards;                   // the source's records
    const int32_t *src_index;               // record of slot i: src_index[i] (i when NULL)
    uint64_t *keys;                         // [n] or, WIDE_KEY, [n][2]
    int64_t n;
    int32_t rec_bytes, max_events, multi_ev;
    int32_t view;                           // SGX_KEYS_VIEW_STATE, or the observer: 0 = each record's mover, +1 / -1
    int32_t flags;                          // SGX_KEYS_NO_CLOCK
};

// the two words of a key under construction (word 1 only where the caller wants 128 bits)
template <bool WIDE_KEY>
struct KeyAcc {
    uint64_t w0 = 0, w1 = 0;
    __device__ __forceinline__ void add(const int slot, const int value) {
        const uint64_t g = KEY_GOLD * ((((uint64_t)(uint32_t)slot << 32) | (uint32_t)value) + 1ull);
        w0 ^= sm_fin(KEY_SALT0 + g);
        if constexpr (WIDE_KEY) w1 ^= sm_fin(KEY_SALT1 + g);
    }
};

// the features quad q of a record holds (v: its 16 bytes): cells of the four dense boards, bits of the two never-moved bitmaps, capture
// events.  (The 32 bytes of scalars are one lane's work: key_scalars.)  skip_board: the dense board an information-set key leaves out, -1 = none.
template <class G, bool WIDE_KEY>
__device__ __forceinline__ void key_quad(KeyAcc<WIDE_KEY> &acc, const SGX_KERNARG KeysParams &P, const int8_t *rec, const int q, const int4 v, const int skip_board,
                                         const int n_events) {
    constexpr int RC = G::RC, S = G::S;
    const int off = 16 * q;
    const int w[4] = {v.x, v.y, v.z, v.w};
    if (off < G::ST_OFF) {                                       // dense boards 0..3 = impl layers 0, 1, 3, 4 (S is a multiple of 4: a dword lies in one board)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int byte0 = off + 4 * d;
            if (w[d] == 0 || byte0 >= STORED_BOARDS * S) continue;
            const int b = byte0 / S, cell0 = byte0 - b * S;
            if (b == skip_board) continue;
            const int layer = b < 2 ? b : b + 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int val = (int)(int8_t)(w[d] >> (8 * k));
                if (val != 0 && cell0 + k < RC) acc.add(layer * KEY_SLOTS + cell0 + k, val);
            }
        }
    } else if (off < G::SC_OFF) {                                // never-moved bitmaps = impl layers 32 / 33, bit i = cell i
        const int rel = off - G::ST_OFF, p = rel >= G::SB ? 1 : 0, bit0 = 8 * (rel - p * G::SB);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t bits = (uint32_t)w[d];
            while (bits) {
                const int cell = bit0 + 32 * d + __builtin_ctz(bits);
                bits &= bits - 1;
                if (cell < RC) acc.add((32 + p) * KEY_SLOTS + cell, 1);
            }
        }
    } else if (off >= G::EVL_OFF) {                              // capture events = impl layers 8 .. 31: the count of one (layer, cell)
        using ev_t = typename G::ev_t;
        constexpr int PER_Q = 16 / G::EV_BYTES, PER_W = 4 / G::EV_BYTES;
        const int e0 = (off - G::EVL_OFF) / G::EV_BYTES;
        const ev_t *evl = reinterpret_cast<const ev_t *>(rec + G::EVL_OFF);
#pragma unroll
        for (int j = 0; j < PER_Q; ++j) {
            const int i = e0 + j;
            if (i >= n_events) break;
            const uint32_t e = PER_W == 1 ? (uint32_t)w[j] : ((uint32_t)w[j / PER_W] >> (16 * (j % PER_W))) & 0xFFFFu;
            const int key = (int)(e >> G::CELL_BITS) & 31, cell = (int)e & G::CELL_MASK;
            if (key >= 24 || cell >= RC) continue;
            int count = (int)(e >> G::EV_COUNT_SHIFT) + 1;
            if (P.multi_ev) {                                    // chained events of one key: the first one speaks for all, with the sum (merged_event)
                const uint32_t mine = e & (uint32_t)G::EV_KEY_MASK;
                bool first = true;
                for (int t = 0; t < n_events; ++t) {
                    const uint32_t o = (uint32_t)evl[t];
                    if (t == i || (o & (uint32_t)G::EV_KEY_MASK) != mine) continue;
                    if (t < i) { first = false; break; }
                    count += (int)(o >> G::EV_COUNT_SHIFT) + 1;
                }
                if (!first) continue;
            }
            acc.add((8 + key) * KEY_SLOTS + cell, count);
        }
    }
}

// the scalars of the record (sc: turn, flags, max_turns, game number; sc2: events, recent pairs of +1, of -1): what layer 5 and the mover say,
// hashed whether zero or not; the four recent-move pairs = impl layers 6 / 7; the observer of an information-set key (0: a state key)
template <class G, bool WIDE_KEY>
__device__ __forceinline__ void key_scalars(KeyAcc<WIDE_KEY> &acc, const int4 sc, const int4 sc2, const bool clock, const int observer) {
    const int fl = sc.y;
    acc.add(5 * KEY_SLOTS + KEY_SC_OVER, (fl & F_OVER) ? 1 : 0);
    acc.add(5 * KEY_SLOTS + KEY_SC_WINNER, (fl & F_WIN_P1) ? 1 : (fl & F_WIN_M1) ? -1 : 0);
    acc.add(5 * KEY_SLOTS + KEY_SC_END_INVALID, (fl & F_END_INVALID) ? 1 : 0);
    acc.add(5 * KEY_SLOTS + KEY_SC_MOVER, (fl & F_PLAYER_M1) ? -1 : 1);
    if (clock) {
        acc.add(5 * KEY_SLOTS + KEY_SC_TURN, sc.x);
        acc.add(5 * KEY_SLOTS + KEY_SC_MAX_TURNS, sc.z);
    }
    if (observer) acc.add(5 * KEY_SLOTS + KEY_SC_OBSERVER, observer);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int pr = (((t >> 1) ? sc2.z : sc2.y) >> (16 * (t & 1))) & 0xFFFF;
        if ((pr >> G::CELL_BITS) && G::pair_cell(pr) < G::RC) acc.add((6 + (t >> 1)) * KEY_SLOTS + G::pair_cell(pr), G::pair_code(pr));
    }
}

template <int R_, int C_, bool WIDE_KEY>
__global__ __launch_bounds__(KEYS_THREADS) void keys_kernel(const KeysParams SP) {
    using G = Geo<R_, C_>;
    constexpr int LPG = G::LPG, Q_REC = (G::ST_OFF + G::TAIL_BYTES) / 16, NLOAD = (Q_REC + LPG - 1) / LPG;
    const SGX_KERNARG KeysParams &P = *kernarg_of(SP);
    const int lane = threadIdx.x & (LPG - 1);
    const int64_t i = (int64_t)blockIdx.x * (KEYS_THREADS / LPG) + threadIdx.x / LPG;
    if (i >= P.n) return;                                        // (per record: the lanes of a record leave together)
    const int32_t *const index = P.src_index;
    const int8_t *const rec = P.boards + (int64_t)(index ? index[i] : (int32_t)i) * (int64_t)P.rec_bytes;
    const int4 *const src = reinterpret_cast<const int4 *>(rec);
    const int nq = min(P.rec_bytes >> 4, Q_REC);
    // every lane asks for the two scalar quads (one address per record: a broadcast) -- the observer and the length of the event list
    // come from them -- and for its own quads of the record, all before the first hash
    const int4 sc = src[G::SC_OFF / 16], sc2 = src[G::SC_OFF / 16 + 1];
    int4 rq0 = make_int4(0, 0, 0, 0), rq1 = rq0;
    load_record<G>(P, src, lane, rq0, rq1);
    const int mover = (sc.y & F_PLAYER_M1) ? -1 : 1;
    const int observer = P.view == SGX_KEYS_VIEW_STATE ? 0 : (P.view == 0 ? mover : P.view);
    const int skip_board = observer == 0 ? -1 : (observer == 1 ? B_PIECES + 1 : B_PIECES + 0);      // the TRUE pieces of the observer's opponent
    const int n_events = min(min(sc2.x, P.max_events), (int)G::EVL_MAX);
    KeyAcc<WIDE_KEY> acc;
    if constexpr (NLOAD <= 2) {
        if (lane < nq) key_quad<G>(acc, P, rec, lane, rq0, skip_board, n_events);
        if constexpr (NLOAD > 1)
            if (lane + LPG < nq) key_quad<G>(acc, P, rec, lane + LPG, rq1, skip_board, n_events);
    } else {                                                     // WIDE boards: a record of several KiB, walked in a loop
        for (int q = lane; q < nq; q += LPG) key_quad<G>(acc, P, rec, q, src[q], skip_board, n_events);
    }
    if (lane == LPG - 1) key_scalars<G>(acc, sc, sc2, !(P.flags & SGX_KEYS_NO_CLOCK), observer);   // (the last lane holds the fewest quads)
#pragma unroll
    for (int d = 1; d < LPG; d <<= 1) {
        acc.w0 ^= __shfl_xor(acc.w0, d, LPG);
        if constexpr (WIDE_KEY) acc.w1 ^= __shfl_xor(acc.w1, d, LPG);
    }
    if (lane == 0) {
        if constexpr (WIDE_KEY) {
            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u64x2 *>(P.keys + 2 * i) = u64x2{sm_fin(acc.w0), sm_fin(acc.w1)};
        } else {
            P.keys[i] = sm_fin(acc.w0);
        }
    }
}

}  // namespace
