// Stand-alone check of csrc/q_rans.h (host only): the quotient routines -- floor(x / f) without a divide -- on the operand
// set of nblic_amd_qcoder_selftest against 64-bit division (every f in 1 .. 32767), and the resumed lane
// (q_rans_encode_host, every budget around a 256-word window) against the plain pass, with the output buffer cut to the
// exact length (a word more would be an overrun the sanitizer reports) and one word short.  Build and run:
//   g++ -std=c++17 -O2 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o q_rans_check tools/q_rans_check.cpp && ./q_rans_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nblic-image-compression_amd/csrc/q_entropy.cpp"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int lane_case(int h, int w, const std::vector<uint16_t> &qy, std::vector<uint32_t> hist) {
    const size_t n = size_t(h) * size_t(w);
    CHECK(qy.size() == n);
    if (hist.empty()) { hist.assign(12 * 256, 0); for (uint16_t e : qy) hist[(e & 0xFF) * 256 + (e >> 8)]++; }
    CHECK(q_words_ok(qy.data(), n, hist.data()));
    std::vector<uint16_t> plain(2 * n + 4096);
    const long want = q_entropy_encode(plain.data(), plain.size(), h, w, qy.data(), hist.data());
    CHECK(want >= 6);
    plain.resize(size_t(want));
    for (long budget : {0L, 1L, 2L, 255L, 256L, 257L, 4096L}) {
        std::vector<uint16_t> s(static_cast<size_t>(want));                 // the exact capacity
        CHECK(q_rans_encode_host(s.data(), s.size(), h, w, qy.data(), hist.data(), budget) == want);
        CHECK(s == plain);
        std::vector<uint16_t> cut(size_t(want) - 1);
        CHECK(q_rans_encode_host(cut.data(), cut.size(), h, w, qy.data(), hist.data(), budget) == -1);
    }
    return 0;
}

int main() {
    unsigned long long bad = 0, checked = 0;
    for (uint32_t f = 1; f <= 32767; f++)
        for (uint32_t k = 0; k < kQRansSelftestCount; k++) { bad += q_rans_selftest_one(k, f); checked++; }
    if (bad) { fprintf(stderr, "FAILED: %llu of %llu quotients differ from 64-bit division\n", bad, checked); return 1; }
    CHECK(q_rans_selftest_operand(0, 7) == (1u << 16) && q_rans_selftest_operand(1, 7) == 0xFFFFFFFFu);
    CHECK(q_rans_selftest_operand(kQRansSelftestFixed + 1, 7) == (7u << 17));
    // the spans of a launch tile the symbols it takes, last first, and never leave [left - take, left)
    for (uint32_t left : {1u, 2u, 255u, 256u, 257u, 511u, 512u, 513u, 70001u})
        for (uint32_t budget : {1u, 2u, 255u, 256u, 257u, 4096u, 1u << 20}) {
            const uint32_t take = q_rans_take(left, budget);
            uint32_t next = left;
            for (uint32_t r = 0; r < q_rans_rounds(left, take); r++) {
                const QRansSpan sp = q_rans_span(left, take, r);
                CHECK(sp.hi > sp.lo && sp.hi <= kQRansWindow && sp.window * kQRansWindow + sp.hi == next);
                next = sp.window * kQRansWindow + sp.lo;
            }
            CHECK(next == left - take);
            const QRansSpan none = q_rans_span(left, take, q_rans_rounds(left, take));
            CHECK(none.hi == none.lo);
        }
    std::mt19937 rng(21);
    auto uniform = [&](size_t n, int levels, int syms) {
        std::vector<uint16_t> qy(n);
        for (auto &e : qy) e = uint16_t(rng() % unsigned(levels)) | uint16_t((rng() % unsigned(syms)) << 8);
        return qy;
    };
    if (lane_case(40, 37, uniform(40 * 37, 12, 256), {})) return 1;
    if (lane_case(1, 1, uniform(1, 12, 256), {})) return 1;
    for (int n : {255, 256, 257}) if (lane_case(1, n, uniform(size_t(n), 12, 256), {})) return 1;
    if (lane_case(23, 150, uniform(23 * 150, 12, 3), {})) return 1;
    {   // f = 1, coded in a run: every step renormalises
        std::vector<uint16_t> qy = uniform(3000, 3, 256);
        for (size_t t = 0; t < 1000; t++) qy[t] = uint16_t(3 | (5 << 8));
        for (size_t t = 2250; t < 3000; t++) qy[t] = uint16_t(3 | (5 << 8));
        std::vector<uint32_t> hist(12 * 256, 0);
        for (uint16_t e : qy) hist[(e & 0xFF) * 256 + (e >> 8)]++;
        hist[3 * 256 + 5] = 1; hist[3 * 256 + 9] = 10000000;
        if (lane_case(30, 100, qy, hist)) return 1;
    }
    {   // one used symbol (f = 32767) in a run; levels never coded
        std::vector<uint16_t> qy = uniform(2570, 7, 4);
        for (size_t t = 514; t < 514 + 1285; t++) qy[t] = uint16_t(7 | (200 << 8));
        if (lane_case(10, 257, qy, {})) return 1;
    }
    printf("q_rans_check ok (%llu quotients)\n", checked);
    return 0;
}
