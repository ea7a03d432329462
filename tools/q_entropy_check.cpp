// Stand-alone check of q_entropy.cpp (host only): the effort-0 entropy stage with entry rows, on records made here -- 40 x 37
// words drawn over 12 levels and 256 symbols with an entry in front of every row, an image whose levels have one used
// symbol or none, one row, one column, no entry rows at all -- decoded again from every reported (state, words emitted) by
// a plain rANS decoder, with the output buffer cut to the exact length (a byte more would be an overrun the sanitizer
// reports) and one word short.  Build with the sanitizers and run:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o q_entropy_check tools/q_entropy_check.cpp && ./q_entropy_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nblic-image-compression_amd/csrc/q_entropy.cpp"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// Decodes pixels [t0, n) from the coder the entry names and checks symbols, the stream's end and the final state.
static int decode_from(const std::vector<uint16_t> &s, long q_pos, const uint32_t *freq, const uint32_t *start, const std::vector<uint16_t> &qy,
                       size_t t0, uint32_t x, unsigned long long words_before) {
    const size_t total = s.size() - size_t(q_pos) - 2;                  // renormalisation words of the whole pass
    CHECK(words_before <= total);
    size_t at = size_t(q_pos) + 2 + (total - size_t(words_before));
    for (size_t t = t0; t < qy.size(); t++) {
        const uint32_t lv = qy[t] & 0xFF, low = x & (kQNormSum - 1);
        uint32_t y = 0;
        while (y < 255 && !(freq[lv * 256 + y] && low < start[lv * 256 + y] + freq[lv * 256 + y])) y++;
        CHECK(y == uint32_t(qy[t] >> 8));
        x = (x >> kQNormBits) * freq[lv * 256 + y] + low - start[lv * 256 + y];
        if (x < (1u << kQAnsBits)) { CHECK(at < s.size()); x = (x << kQAnsBits) | s[at++]; }
    }
    CHECK(at == s.size());
    CHECK(x == (1u << kQAnsBits));                                       // where the encoder's pass began
    return 0;
}

static int run_case(int h, int w, const std::vector<uint16_t> &qy, const std::vector<int> &rows) {
    const size_t n = size_t(h) * size_t(w);
    CHECK(qy.size() == n);
    std::vector<uint32_t> hist(12 * 256, 0);
    for (uint16_t e : qy) hist[(e & 0xFF) * 256 + (e >> 8)]++;
    CHECK(q_words_ok(qy.data(), n, hist.data()));
    std::vector<uint16_t> plain(2 * n + 4096);
    const long want = q_entropy_encode(plain.data(), plain.size(), h, w, qy.data(), hist.data());
    CHECK(want >= 6);
    plain.resize(size_t(want));
    // the exact capacity: every word of the buffer is the stream's
    std::vector<uint16_t> s(static_cast<size_t>(want));
    std::vector<QEntryState> at(rows.size());
    const long got = q_entropy_encode_entries(s.data(), s.size(), h, w, qy.data(), hist.data(), rows.data(), int(rows.size()), at.data());
    CHECK(got == want && s == plain);                                    // the entry rows do not show in the stream
    std::vector<uint16_t> cut(size_t(want) - 1);
    CHECK(q_entropy_encode_entries(cut.data(), cut.size(), h, w, qy.data(), hist.data(), rows.data(), int(rows.size()), at.data()) == -1);
    CHECK(q_entropy_encode_entries(s.data(), s.size(), h, w, qy.data(), hist.data(), rows.data(), int(rows.size()), at.data()) == want);
    std::vector<uint32_t> freq(12 * 256), start(12 * 256);
    int hh = 0, ww = 0;
    const long q_pos = q_decode_tables(s.data(), s.size(), &hh, &ww, freq.data(), start.data(), nullptr);
    CHECK(q_pos >= 4 && hh == h && ww == w);
    if (decode_from(s, q_pos, freq.data(), start.data(), qy, 0, (uint32_t(s[size_t(q_pos)]) << 16) | s[size_t(q_pos) + 1], s.size() - size_t(q_pos) - 2)) return 1;
    for (size_t k = 0; k < rows.size(); k++)
        if (decode_from(s, q_pos, freq.data(), start.data(), qy, size_t(rows[k]) * size_t(w), at[k].state, at[k].words)) return 1;
    return 0;
}

int main() {
    std::mt19937 rng(20);
    auto uniform = [&](int h, int w, int levels, int syms) {
        std::vector<uint16_t> qy(size_t(h) * size_t(w));
        for (auto &e : qy) e = uint16_t(rng() % unsigned(levels)) | uint16_t((rng() % unsigned(syms)) << 8);
        return qy;
    };
    auto every = [](int h, int r) { std::vector<int> v; for (int i = r; i < h; i += r) v.push_back(i); return v; };
    if (run_case(40, 37, uniform(40, 37, 12, 256), every(40, 1))) return 1;
    if (run_case(40, 37, uniform(40, 37, 12, 256), every(40, 5))) return 1;
    if (run_case(40, 37, uniform(40, 37, 12, 256), {})) return 1;
    if (run_case(23, 150, uniform(23, 150, 12, 3), every(23, 7))) return 1;      // skewed: few words are emitted
    {   // every level has one used symbol (levels 0 .. 5) or none (6 .. 11): q_normalise's special cases
        std::vector<uint16_t> qy(size_t(17) * 28);
        for (size_t t = 0; t < qy.size(); t++) { const unsigned lv = unsigned(t % 6); qy[t] = uint16_t(lv | ((lv == 5 ? 255u : 40u * lv) << 8)); }
        if (run_case(17, 28, qy, every(17, 1))) return 1;
    }
    if (run_case(9, 1, uniform(9, 1, 12, 256), every(9, 1))) return 1;
    if (run_case(1, 9, uniform(1, 9, 12, 256), {})) return 1;
    {   // refusals: rows out of range or out of order, and nothing is written
        const std::vector<uint16_t> qy = uniform(5, 4, 2, 2);
        std::vector<uint32_t> hist(12 * 256, 0);
        for (uint16_t e : qy) hist[(e & 0xFF) * 256 + (e >> 8)]++;
        std::vector<uint16_t> out(64, 0xA7A7);
        QEntryState at[3];
        const int bad[4][2] = {{0, 2}, {2, 5}, {3, 3}, {4, 2}};
        for (auto &b : bad) CHECK(q_entropy_encode_entries(out.data(), out.size(), 5, 4, qy.data(), hist.data(), b, 2, at) == -2);
        for (uint16_t v : out) CHECK(v == 0xA7A7);
        std::vector<uint16_t> wrong = qy;
        wrong[7] = 12;                                                   // a level above 11
        CHECK(!q_words_ok(wrong.data(), wrong.size(), hist.data()));
        wrong[7] = uint16_t(1 | (9 << 8));                               // a symbol the histogram does not count
        CHECK(!q_words_ok(wrong.data(), wrong.size(), hist.data()));
    }
    printf("q_entropy_check ok\n");
    return 0;
}
