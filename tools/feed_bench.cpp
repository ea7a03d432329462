// feed_bench.cpp -- host range-coder packs fed from 8-lane rows of 13-bit groups, one / two / three packs in lock-step (no GPU).
//   g++ -O2 -std=c++17 tools/feed_bench.cpp nblic-image-compression_amd/csrc/build/range_coder_x8.o -o /tmp/feed_bench
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../nblic-image-compression_amd/csrc/range_coder.h"
using namespace nblic;
int main(int argc, char **argv) {
    const size_t n = argc > 1 ? size_t(atol(argv[1])) : size_t(1) << 22;      // bins per lane
    std::mt19937 rng(1);
    std::vector<std::vector<uint16_t>> s(24, std::vector<uint16_t>(n));
    for (auto &v : s) for (auto &e : v) { const uint32_t p = 1 + rng() % 4095; e = uint16_t(p | ((rng() % 4096 < p) ? 0x8000u : 0u)); }
    if (argc > 2) {                                          // real records: <prefix>K.u16 for K = 0.. (as many as exist, reused in turn), n of each
        int have = 0;
        for (int l = 0; l < 24; l++) {
            char path[512];
            snprintf(path, sizeof path, "%s%d.u16", argv[2], l);
            FILE *f = fopen(path, "rb");
            if (f) { if (fread(s[l].data(), 2, n, f) != n) { fprintf(stderr, "%s is shorter than %zu records\n", path, n); return 1; } fclose(f); have = l + 1; }
            else if (have) s[l] = s[l % have];
            else { fprintf(stderr, "no %s\n", path); return 1; }
        }
        printf("records from %s* (%d files)\n", argv[2], have);
    }
    uint64_t *rows[3];
    size_t len[24];
    for (int p = 0; p < 3; p++) {
        rows[p] = (uint64_t *)aligned_alloc(64, group_words(n) * 8);
        memset(rows[p], 0, group_words(n) * 8);
        for (int l = 0; l < 8; l++) { len[8 * p + l] = n; pack_groups_host(rows[p], l, s[8 * p + l].data(), n); }
    }
    std::vector<std::vector<uint8_t>> out(24, std::vector<uint8_t>(2 * n + 64));
    uint8_t *outs[24]; size_t caps[24], lens[3][24];
    for (int l = 0; l < 24; l++) { outs[l] = out[l].data(); caps[l] = out[l].size(); }
    for (int rep = 0; rep < 3; rep++) {
        for (int np = 1; np <= 3; np++) {
            RangeX8 x[3];
            RangeX8 *packs[3] = {&x[0], &x[1], &x[2]};
            for (int p = 0; p < np; p++) x[p].begin(8, outs + 8 * p, caps + 8 * p);
            auto t0 = std::chrono::steady_clock::now();
            feed_packs(packs, np, rows, len);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (int p = 0; p < np; p++) x[p].end(lens[np - 1] + 8 * p);
            printf("%d pack%s: %.0f Mbins/s\n", np, np > 1 ? "s" : " ", 8.0 * np * n / dt / 1e6);
        }
        printf("same lengths: %d %d\n", !memcmp(lens[0], lens[1], 8 * sizeof(size_t)), !memcmp(lens[1], lens[2], 16 * sizeof(size_t)));
    }
    return 0;
}
