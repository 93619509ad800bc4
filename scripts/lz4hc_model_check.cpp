// Stand-alone sanitizer check of ambc_lz4hc_model (host code, no GPU):
//   c++ -std=c++17 -g -fsanitize=address,undefined -Iinclude scripts/lz4hc_model_check.cpp \
//       adaptive-compression_amd/csrc/ambc_lz4hc_model.cpp -o lz4hc_model_check && ./lz4hc_model_check
// Every case's frame is written into an exactly sized heap buffer (an overrun
// is an ASan report) and its block is decoded back with a bounds-checked decoder.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ambc.h"

namespace ambc { thread_local std::string g_err; }

static bool decode(const uint8_t* b, size_t bl, std::vector<uint8_t>& out, size_t n) {
    size_t p = 0;
    while (p < bl) {
        const uint8_t tok = b[p++];
        size_t lit = tok >> 4;
        if (lit == 15) { uint8_t x; do { if (p >= bl) return false; x = b[p++]; lit += x; } while (x == 255); }
        if (p + lit > bl) return false;
        out.insert(out.end(), b + p, b + p + lit);
        p += lit;
        if (p == bl) break;
        if (p + 2 > bl) return false;
        const size_t off = b[p] | b[p + 1] << 8;
        p += 2;
        size_t ml = tok & 15;
        if (ml == 15) { uint8_t x; do { if (p >= bl) return false; x = b[p++]; ml += x; } while (x == 255); }
        ml += 4;
        if (off == 0 || off > out.size()) return false;
        for (size_t t = 0; t < ml; t++) out.push_back(out[out.size() - off]);
    }
    return out.size() == n;
}

static int check(const std::vector<uint8_t>& d) {
    uint32_t len = 0;
    const uint32_t n = (uint32_t)d.size();
    int rc = ambc_lz4hc_model(d.data(), n, nullptr, 0, &len);
    if (n == 0) return rc == AMBC_OK && len == 0 ? 0 : 1;
    if (rc != AMBC_E_CAPACITY || len > n + 23) return 1;
    std::vector<uint8_t> fr(len);
    if (ambc_lz4hc_model(d.data(), n, fr.data(), len, &len) != AMBC_OK) return 1;
    const uint32_t bs = fr[15] | fr[16] << 8 | fr[17] << 16 | (uint32_t)fr[18] << 24;
    if (bs & 0x80000000u) return std::memcmp(fr.data() + 19, d.data(), n) != 0;
    std::vector<uint8_t> out;
    return !(decode(fr.data() + 19, bs, out, n) && out == d);
}

int main() {
    std::vector<std::vector<uint8_t>> cases;
    for (size_t n : {0, 1, 4, 12, 13, 16, 17, 64}) {
        std::vector<uint8_t> v(n);
        for (size_t i = 0; i < n; i++) v[i] = (uint8_t)(i % 7);
        cases.push_back(v);
    }
    cases.emplace_back(4096, 0);
    cases.emplace_back(13, 'a');
    cases.emplace_back(16384, 0);
    cases.emplace_back(65536, 0);
    { std::vector<uint8_t> v; for (int r = 0; r < 300; r++) for (char c : std::string("abcdefghijkl")) v.push_back((uint8_t)c); cases.push_back(v); }
    uint64_t s = 88172645463325252ull;
    auto rnd = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    { std::vector<uint8_t> v(4096); for (auto& b : v) b = (uint8_t)rnd(); cases.push_back(v); }
    { std::vector<uint8_t> v(52); for (auto& b : v) b = (uint8_t)rnd(); v.insert(v.end(), v.begin() + 10, v.begin() + 22); cases.push_back(v); }
    for (size_t n : {1000u, 4096u, 16384u, 65536u}) {   // text-like: few symbols, repeats
        std::vector<uint8_t> v(n);
        for (auto& b : v) b = (uint8_t)("etaoin shrdlu"[rnd() % 13]);
        for (size_t i = 100; i + 40 < n; i += 97) std::memcpy(&v[i], &v[i - 90], 30);
        cases.push_back(v);
    }
    int bad = 0;
    for (size_t i = 0; i < cases.size(); i++)
        if (check(cases[i])) { std::printf("case %zu (n = %zu) failed\n", i, cases[i].size()); bad++; }
    std::printf("%zu cases, %d failed\n", cases.size(), bad);
    return bad != 0;
}
