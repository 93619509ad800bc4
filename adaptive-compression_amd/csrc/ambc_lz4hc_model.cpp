// ambc_lz4hc_model.cpp -- "ambc-lz4 hc v1", the serial statement of the parse
// k_lz4hc (ambc_lz4hc.hip) computes in parallel.  Host only: no context, no
// device (like ambc_split_body / ambc_debug_walk).
//
//   hash     h(i) = (u32le(d+i) * 2654435761) >> (32 - LZ4HC_HASH_BITS)
//   chain    of i: the positions j < i with h(j) == h(i), nearest first; the
//            first LZ4HC_DEPTH of them are examined
//   match    at i <= n-12: among examined j with u32le(d+j) == u32le(d+i) the
//            longest common prefix, capped at n-5-i (LZ4 block end rules);
//            ties to the nearest j; none when no length >= 4 exists
//   select   from p = anchor = 0 while p <= n-12:
//              len(p) < 4                          -> p += 1
//              p+1 <= n-12 and len(p+1) > len(p)   -> p += 1  (one-step lazy)
//              else  sequence (literals anchor..p, offset, len); p += len; anchor = p
//            final literals anchor..n; n < 13: one literal run
//   frame    the one-block LZ4F layout of "ambc-lz4 greedy v2": 15-B header with
//            the content size, block size (bit 31: stored, when the block would
//            not shrink), block, 4-B end mark
//
// A match is a function of the position alone, so the kernel computes every
// position's independently and the two produce the same bytes.
#include <cstring>
#include <vector>

#include "../../include/ambc.h"
#include "ambc_consts.h"
#include "ambc_hostutil.h"

namespace ambc {
namespace {

inline uint32_t rd32le(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32 (seed 0) of the 10-byte frame descriptor: FLG, BD, 8-byte content size
uint32_t xxh32_desc(const uint8_t* d) {
    const uint32_t P1 = 2654435761U, P2 = 2246822519U, P3 = 3266489917U, P4 = 668265263U, P5 = 374761393U;
    uint32_t h = P5 + 10u;
    h = rotl(h + rd32le(d) * P3, 17) * P4;
    h = rotl(h + rd32le(d + 4) * P3, 17) * P4;
    h = rotl(h + d[8] * P5, 11) * P1;
    h = rotl(h + d[9] * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

struct Out {
    uint8_t* p;      // nullptr: size only
    uint64_t o = 0;
    void put(uint8_t b) { if (p) p[o] = b; o++; }
    void ext(uint32_t v) {   // length extension bytes for v >= 15
        v -= 15;
        while (v >= 255) { put(255); v -= 255; }
        put((uint8_t)v);
    }
    void copy(const uint8_t* s, uint32_t len) { if (p) std::memcpy(p + o, s, len); o += len; }
};

struct Match { uint32_t len, off; };

// the block of d[0, n), n <= 65536; out == nullptr: its size
uint64_t hc_block(const uint8_t* d, uint32_t n, uint8_t* out, uint32_t HB, uint32_t K) {
    Out w{out};
    uint32_t anchor = 0;
    if (n >= 13) {
        const uint32_t mlim = n - 12;
        const int32_t NONE = -1;
        std::vector<int32_t> head((size_t)1 << HB, NONE), prev(mlim + 1, NONE);
        for (uint32_t i = 0; i <= mlim; i++) {
            const uint32_t h = (rd32le(d + i) * 2654435761u) >> (32 - HB);
            prev[i] = head[h];
            head[h] = (int32_t)i;
        }
        auto match_at = [&](uint32_t i) {
            Match m{0, 0};
            const uint32_t v = rd32le(d + i), cap = n - 5 - i;
            int32_t j = prev[i];
            for (uint32_t k = 0; k < K && j != NONE; k++, j = prev[j]) {
                if (rd32le(d + j) != v) continue;
                uint32_t L = 4;
                while (L < cap && d[j + L] == d[i + L]) L++;
                if (L > m.len) { m.len = L; m.off = i - (uint32_t)j; }
                if (L == cap) break;   // no farther candidate can be longer
            }
            return m;
        };
        uint32_t p = 0;
        Match cur = match_at(0);
        while (p <= mlim) {
            Match nxt{0, 0};
            if (p + 1 <= mlim) nxt = match_at(p + 1);
            if (cur.len < 4 || nxt.len > cur.len) { p++; cur = nxt; continue; }
            const uint32_t lit = p - anchor, ml = cur.len - 4;
            w.put((uint8_t)((lit >= 15 ? 15 : lit) << 4 | (ml >= 15 ? 15 : ml)));
            if (lit >= 15) w.ext(lit);
            w.copy(d + anchor, lit);
            w.put((uint8_t)cur.off);
            w.put((uint8_t)(cur.off >> 8));
            if (ml >= 15) w.ext(ml);
            p += cur.len;
            anchor = p;
            if (p <= mlim) cur = match_at(p);
        }
    }
    const uint32_t lit = n - anchor;
    w.put((uint8_t)((lit >= 15 ? 15 : lit) << 4));
    if (lit >= 15) w.ext(lit);
    w.copy(d + anchor, lit);
    return w.o;
}

}  // namespace

}  // namespace ambc

using namespace ambc;

// the model with explicit constants (scripts/lz4hc_ratio.py's sweep over them)
extern "C" int ambc_lz4hc_model_ex(const uint8_t* in, uint32_t n, uint32_t HB, uint32_t K, uint8_t* out,
                                   uint32_t out_cap, uint32_t* out_len) {
    if (!out_len || (!in && n) || (!out && out_cap)) return fail(AMBC_E_INVAL, "NULL argument");
    if (n == 0) { *out_len = 0; return AMBC_OK; }          // LZ4Compression.compress: empty -> b''
    if (n > AMBC_MAX_CHUNK) return fail(AMBC_E_INVAL, "ambc_lz4hc_model takes at most 65536 bytes (one LZ4 block)");
    if (HB < 8 || HB > 16 || K < 1) return fail(AMBC_E_INVAL, "hash bits in [8, 16], depth >= 1");
    const uint64_t blk = hc_block(in, n, nullptr, HB, K);
    const bool stored = blk >= n;
    const uint64_t total = 15 + 4 + (stored ? n : blk) + 4;
    *out_len = (uint32_t)total;
    if (total > out_cap) return fail(AMBC_E_CAPACITY, "output buffer too small");
    uint8_t* h = out;
    h[0] = 0x04; h[1] = 0x22; h[2] = 0x4D; h[3] = 0x18;
    h[4] = 0x68; h[5] = 0x40;
    for (int b = 0; b < 8; b++) h[6 + b] = (uint8_t)((uint64_t)n >> (8 * b));
    h[14] = (uint8_t)((xxh32_desc(h + 4) >> 8) & 0xFF);
    const uint32_t bs = stored ? (n | 0x80000000u) : (uint32_t)blk;
    for (int b = 0; b < 4; b++) out[15 + b] = (uint8_t)(bs >> (8 * b));
    if (stored) std::memcpy(out + 19, in, n);
    else hc_block(in, n, out + 19, HB, K);
    std::memset(out + total - 4, 0, 4);
    return AMBC_OK;
}

extern "C" int ambc_lz4hc_model(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t out_cap, uint32_t* out_len) {
    return ambc_lz4hc_model_ex(in, n, LZ4HC_HASH_BITS, LZ4HC_DEPTH, out, out_cap, out_len);
}
