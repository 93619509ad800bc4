// ambc_lz4hc.hip -- id 9 as "ambc-lz4 hc v1" (AMBC_FLAG_LZ4HC) for gfx950: hash
// chains and a one-step lazy parse, byte for byte ambc_lz4hc_model's frames
// (ambc_lz4hc_model.cpp states the parse).
//
// A later encoder like k_dict / k_deflate: k_encode has run with id 9 masked
// off, and id 9 -- the highest id -- takes a chunk iff its frame + 18 is strictly
// below the best so far.  One workgroup of 256 threads per chunk, everything in
// LDS:
//
//   chain   prev[i] = the nearest j < i with h(j) == h(i).  Wave 0 inserts the
//           positions window by window (64 at a time, in order): a position's
//           predecessor inside its window comes from ballots over the hash
//           bits, the first of a hash in the window takes head[h] of the
//           earlier windows, the last of a hash becomes head[h].  That is the
//           serial insert's chain exactly.
//   match   per tile of 1024 positions, one position per thread and step: walk
//           prev[] for at most LZ4HC_DEPTH entries, 4-byte check, common
//           prefix 4 bytes at a time, capped at n - 5 - i; ties stay with the
//           nearest.  A position's match depends on nothing else.
//   select  wave 0 walks the tile's (len, off) table 64 positions at a time:
//           the next position with a match by ballot, the lazy step by two
//           readlanes, and every sequence the window selects is emitted at once
//           (prefix sums give the output offsets) as in k_encode's LZ4.  The
//           next tile starts where the walk stands, so positions under a long
//           match are never searched.
//   exit    the walk gives up as soon as the emitted sequences plus the
//           pending literals cannot stay below the best so far; chunks whose
//           best is already below any LZ4 block's minimum never start.
//
// The frame goes to the chunk's slot; where a Dictionary / DEFLATE payload
// (ids 2 / 5) or a raw copy already lies there, to the slot's upper half (the slot is
// 2 C + 64 bytes, both payloads below C) and to the front only once it has won.
//
// LDS per workgroup and waves per SIMD (160 KiB per CU, 4 waves per workgroup),
// DESIGN "ambc-lz4 hc v1":
//   CMAX  1024: 15.0 KiB, 8      2048: 18.0 KiB, 8      4096: 24.0 KiB, 6
//   CMAX  8192: 36.0 KiB, 4     16384: 60.0 KiB, 2
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ambc_internal.h"
#include "ambc_wave.h"

namespace ambc {
namespace {

constexpr uint32_t HC_NT = 256;       // threads per workgroup
constexpr uint32_t HC_TILE = 1024;    // positions per match tile
constexpr uint32_t HC_NONE = 0xFFFFu; // no predecessor (positions stay below 16384)
constexpr uint32_t HC_UNKNOWN = 0xFFFFFFFFu;   // the next position's match lies in the next tile

template <int CMAX>
struct HcSmem {
    alignas(16) uint32_t ch[CMAX / 4 + 4];   // the chunk, zero padded (dwords: positions are read unaligned)
    uint16_t prev[CMAX];
    uint16_t head[1u << LZ4HC_HASH_BITS];
    uint16_t tlen[HC_TILE];
    uint16_t toff[HC_TILE];
    uint32_t base, done, res;
};

__device__ __forceinline__ uint32_t rd32(const uint32_t* w, uint32_t i) {
    return __builtin_amdgcn_alignbyte(w[(i >> 2) + 1], w[i >> 2], i & 3u);
}

// the one-block LZ4F frame of k_encode's LZ4 (ambc_encode.hip: xxh32_desc,
// ext_len, ext_byte, lz4_hdr_byte), restated so that file stays as it is
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ uint32_t xxh32_desc(uint32_t n) {
    const uint32_t P1 = 2654435761U, P2 = 2246822519U, P3 = 3266489917U, P4 = 668265263U, P5 = 374761393U;
    uint32_t h = P5 + 10u;
    h = rotl32(h + (0x68u | 0x40u << 8 | (n & 0xFFFFu) << 16) * P3, 17) * P4;
    h = rotl32(h + (n >> 16) * P3, 17) * P4;
    h = rotl32(h + 0u * P5, 11) * P1;
    h = rotl32(h + 0u * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t ext_len(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }
__device__ __forceinline__ uint32_t ext_byte(uint32_t v, uint32_t xl, uint32_t t) {
    return t + 1 < xl ? 255u : (v - 15) % 255u;
}
__device__ __forceinline__ uint8_t lz4_hdr_byte(uint32_t q, uint32_t n, uint32_t bs) {
    if (q < 4) return (uint8_t)(0x184D2204u >> (8 * q));
    if (q == 4) return 0x68;   // FLG: v01, block independence, content size
    if (q == 5) return 0x40;   // BD: 64 KiB max block
    if (q < 14) return q < 10 ? (uint8_t)(n >> (8 * (q - 6))) : 0;
    if (q == 14) return (uint8_t)((xxh32_desc(n) >> 8) & 0xFF);
    return (uint8_t)(bs >> (8 * (q - 15)));
}

template <int CMAX>
__global__ __launch_bounds__(HC_NT) void k_lz4hc(EncArgs A) {
    constexpr uint32_t HB = LZ4HC_HASH_BITS;
    __shared__ HcSmem<CMAX> S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = blockIdx.x;
    const uint64_t pos0 = (uint64_t)k * A.chunk_size;
    const uint32_t n = (uint32_t)min((uint64_t)A.chunk_size, A.n_total - pos0);
    const bool force = A.flags & ENC_FORCE;
    if (n == 0 || n > (uint32_t)CMAX) return;
    if (!force && !(((A.method_mask >> 9) & 1u) && A.pref_min[9] <= n && n <= A.pref_max[9])) return;
    // the bar from the winner so far (adaptive_compressor.py:559-579): id 9 wins
    // iff block + 23 + 18 < T.  Any LZ4 block of n >= 13 bytes holds a literal,
    // one match of at most n - 6 bytes and the last five bytes: 10 + ext(n - 10)
    uint32_t w = 255, T = n;
    if (!force) {
        w = A.ids[k];
        T = w == 255 ? n : A.plen[k] + HDR;
        if (n < 13 || T <= 51 + ext_len(n - 10)) return;
    }
    const uint32_t budget = force ? n : T - 41;   // the block must stay below it
    uint8_t* const slot = A.slots + (uint64_t)k * A.slot_stride;
    // a payload that already lies in the slot (ids 2 / 5, or a raw chunk that is not
    // read in place) stays whole until id 9 has won
    const bool staged = w == 2 || w == 5 || (!force && w == 255 && !(A.flags & ENC_RAW_IN_PLACE));
    uint8_t* const dst = staged ? slot + ((A.chunk_size + 15u) & ~15u) : slot;
    uint8_t* const blk = dst + 19;
    const uint8_t* src = A.in + pos0;
    uint8_t* const chb = reinterpret_cast<uint8_t*>(S.ch);

    {
        uint32_t done = 0;
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const uint32_t nv = n >> 4;
            for (uint32_t q = tid; q < nv; q += HC_NT)
                reinterpret_cast<uint4*>(S.ch)[q] = reinterpret_cast<const uint4*>(src)[q];
            done = nv << 4;
        }
        for (uint32_t i = done + tid; i < n; i += HC_NT) chb[i] = src[i];
        for (uint32_t i = n + tid; i < (uint32_t)CMAX + 16; i += HC_NT) chb[i] = 0;
        for (uint32_t i = tid; i < (1u << HB); i += HC_NT) S.head[i] = (uint16_t)HC_NONE;
    }
    const int mlim = (int)n - 12;   // last match start; < 0: none
    if (tid == 0) {
        S.base = 0;
        S.done = mlim < 0;
        S.res = 0;
    }
    __syncthreads();

    // ---- the chains, by wave 0 in window order ----
    if (wave == 0) {
#pragma unroll 1
        for (int wb = 0; wb <= mlim; wb += 64) {
            const uint32_t i = (uint32_t)wb + lane;
            const bool in = (int)i <= mlim;
            const uint32_t h = (rd32(S.ch, in ? i : 0u) * 2654435761u) >> (32 - HB);
            uint64_t peers = __ballot(in);
#pragma unroll
            for (uint32_t b = 0; b < HB; b++) {
                const uint64_t m = __ballot((h >> b) & 1u);
                peers &= ((h >> b) & 1u) ? m : ~m;
            }
            const uint64_t lower = peers & ((1ull << lane) - 1ull);
            const uint64_t higher = peers & ~((2ull << lane) - 1ull);
            if (in) {
                const uint32_t pv = lower ? (uint32_t)wb + 63u - (uint32_t)__clzll((long long)lower) : S.head[h];
                S.prev[i] = (uint16_t)pv;
                if (!higher) S.head[h] = (uint16_t)i;
            }
            wave_sync();
        }
    }

    uint32_t emitted = 0, anchor = 0;   // wave 0's walk state
    bool alive = true;
    while (true) {
        __syncthreads();
        const uint32_t base = S.base;
        if (S.done) break;
        const uint32_t tend = min(base + HC_TILE, (uint32_t)mlim + 1u);
        // ---- every position's match ----
        for (uint32_t i = base + tid; i < tend; i += HC_NT) {
            const uint32_t v = rd32(S.ch, i), cap = n - 5u - i;
            uint32_t best = 0, boff = 0;
            uint32_t j = S.prev[i];
#pragma unroll 1
            for (uint32_t c = 0; c < LZ4HC_DEPTH && j != HC_NONE; c++) {
                if (rd32(S.ch, j) == v) {
                    uint32_t L = 4;
                    while (L < cap) {
                        const uint32_t x = rd32(S.ch, i + L) ^ rd32(S.ch, j + L);
                        if (x) { L += (uint32_t)__builtin_ctz(x) >> 3; break; }
                        L += 4;
                    }
                    L = min(L, cap);
                    if (L > best) { best = L; boff = i - j; }
                    if (L == cap) break;   // no farther candidate can be longer
                }
                j = S.prev[j];
            }
            S.tlen[i - base] = (uint16_t)best;
            S.toff[i - base] = (uint16_t)boff;
        }
        __syncthreads();
        // ---- wave 0: the lazy walk over the tile, emitting as it goes ----
        if (wave == 0) {
            uint32_t p = base;
            bool stop = false;
#pragma unroll 1
            for (uint32_t wb = base; wb < tend && !stop && alive; wb += 64) {
                if (p >= wb + 64) continue;
                const uint32_t i = wb + lane;
                const uint32_t L = i < tend ? (uint32_t)S.tlen[i - base] : 0u;
                const uint32_t off = i < tend ? (uint32_t)S.toff[i - base] : 0u;
                uint32_t Ln = 0;   // the next position's length (0 past the last match start)
                if ((int)(i + 1) <= mlim) Ln = i + 1 < tend ? (uint32_t)S.tlen[i + 1 - base] : HC_UNKNOWN;
                const uint64_t vm = __ballot(L >= 4);
                uint64_t sel = 0;
                uint32_t aend = anchor;
                while (true) {
                    p = uniform_u32(p);
                    const uint32_t rel = p - wb;
                    if (rel >= 64) break;
                    const uint64_t m = vm & (~0ull << rel);
                    if (!m) { p = wb + 64; break; }
                    const uint32_t q = uniform_u32((uint32_t)__builtin_ctzll(m));
                    const uint32_t Lq = readlane(L, q), Lq1 = readlane(Ln, q);
                    if (Lq1 == HC_UNKNOWN) { p = wb + q; stop = true; break; }   // the next tile starts here
                    if (Lq1 > Lq) { p = wb + q + 1; continue; }                  // lazy: this byte is a literal
                    sel |= 1ull << q;
                    p = wb + q + Lq;
                    aend = p;
                }
                if (sel) {
                    // every selected lane emits its own sequence: literals from the
                    // previous selected match's end (exclusive max-scan), output
                    // offset = exclusive prefix sum of the sequence sizes
                    const bool me = (sel >> lane) & 1ull;
                    const int pe = wave_excl_max(me ? (int)(i + L) : -1, (int)anchor);
                    const uint32_t lit = me ? i - (uint32_t)pe : 0u;
                    const uint32_t ml = me ? L - 4 : 0u;
                    const uint32_t xl = ext_len(lit), xm = ext_len(ml);
                    const uint32_t sz = me ? 3 + xl + lit + xm : 0u;
                    const uint32_t incl = wave_incl_sum(sz);
                    const uint32_t tot = readlane(incl, 63);
                    // the block ends with a token at least: it cannot stay below the budget
                    if (emitted + tot + 1 >= budget) { alive = false; break; }
                    const uint32_t q0 = emitted + incl - sz;   // token
                    const uint32_t ql = q0 + 1 + xl;           // first literal
                    if (me) {
                        blk[q0] = (uint8_t)((lit >= 15 ? 15 : lit) << 4 | (ml >= 15 ? 15 : ml));
                        blk[ql + lit] = (uint8_t)off;
                        blk[ql + lit + 1] = (uint8_t)(off >> 8);
                        for (uint32_t t = 0; t < xl; t++) blk[q0 + 1 + t] = (uint8_t)ext_byte(lit, xl, t);
                        for (uint32_t t = 0; t < xm; t++) blk[ql + lit + 2 + t] = (uint8_t)ext_byte(ml, xm, t);
                    }
                    // literals inside the window, one byte per lane: a lane no selected
                    // match covers and a selected match follows belongs to that
                    // sequence (its pe is that sequence's literal start); the first
                    // sequence's literals from before the window by the whole wave
                    const uint64_t rest = sel >> lane;
                    const uint32_t nx = rest ? lane + (uint32_t)__builtin_ctzll(rest) : lane;
                    const uint32_t qn = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(nx << 2), (int)ql);
                    if (!me && rest && (int)i >= pe) blk[qn + (i - (uint32_t)pe)] = chb[i];
                    if (anchor < wb) {
                        const uint32_t d0 = readlane(ql, (uint32_t)__builtin_ctzll(sel));
                        const uint32_t len = wb - anchor;
                        for (uint32_t t = lane; t < len; t += 64) blk[d0 + t] = chb[anchor + t];
                    }
                    emitted = uniform_u32(emitted + tot);
                    anchor = uniform_u32(aend);
                }
                // the literals the walk has passed are in the block whatever follows
                const uint32_t seen = min(p, n);
                if (seen > anchor && emitted + (seen - anchor) + 1 >= budget) { alive = false; break; }
            }
            if (lane == 0) {
                S.base = p;
                S.done = !alive || (int)p > mlim;
            }
        }
    }

    // ---- final literals, frame header, block size, end mark ----
    if (wave == 0) {
        uint32_t fin = 0, flit = 0, fxl = 0;
        if (alive) {
            flit = n - anchor;
            fxl = ext_len(flit);
            fin = 1 + fxl + flit;
            if (emitted + fin >= budget) alive = false;
        }
        uint32_t res = 0;
        if (alive) {
            const uint32_t blen = emitted + fin;
            uint8_t* o = blk + emitted;
            for (uint32_t t = lane; t < fin + 4; t += 64) {
                uint32_t b;
                if (t == 0) b = (flit >= 15 ? 15 : flit) << 4;
                else if (t < 1 + fxl) b = ext_byte(flit, fxl, t - 1);
                else if (t < fin) b = chb[anchor + t - 1 - fxl];
                else b = 0;   // end mark
                o[t] = (uint8_t)b;
            }
            if (lane < 19) dst[lane] = lz4_hdr_byte(lane, n, blen);
            res = blen + 23;
        } else if (force) {
            // stored block: 15 B header, size | 0x80000000, raw bytes, end mark (LZ4F rule)
            for (uint32_t t = lane; t < n + 4; t += 64) blk[t] = t < n ? chb[t] : 0;
            if (lane < 19) dst[lane] = lz4_hdr_byte(lane, n, n | 0x80000000u);
            res = n + 23;
        }
        if (lane == 0) S.res = res;
    }
    __syncthreads();
    const uint32_t res = S.res;
    if (!res) return;
    if (staged) {   // (slot and its upper half are 16-byte aligned; the slot holds 2 C + 64 bytes)
        const uint4* s4 = reinterpret_cast<const uint4*>(dst);
        uint4* d4 = reinterpret_cast<uint4*>(slot);
        for (uint32_t q = tid; q < (res + 15) / 16; q += HC_NT) d4[q] = s4[q];
    }
    if (tid == 0) {
        A.ids[k] = 9;
        A.plen[k] = res;
        A.sizes[k] = (uint64_t)HDR + res;
        if (A.pending) A.pending[k] = 0;
    }
}

template <int CMAX>
hipError_t launch_lz4hc_t(const EncArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_lz4hc<CMAX>, dim3(a.n_chunks), dim3(HC_NT), 0, s, a);
    return hipGetLastError();
}

}  // namespace

// chunk_size <= LZ4HC_MAX_CHUNK (check_params)
hipError_t launch_lz4hc(const EncArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return hipSuccess;
    const uint32_t C = a.chunk_size;
    if (C > LZ4HC_MAX_CHUNK) return hipErrorInvalidValue;
    if (C <= 1024) return launch_lz4hc_t<1024>(a, s);
    if (C <= 2048) return launch_lz4hc_t<2048>(a, s);
    if (C <= 4096) return launch_lz4hc_t<4096>(a, s);
    if (C <= 8192) return launch_lz4hc_t<8192>(a, s);
    return launch_lz4hc_t<16384>(a, s);
}

}  // namespace ambc
