// Stand-alone check of index_entries.h (host only): the size of an index, entries that wait for their window while the
// stream is emitted in pieces of every size, the assembly of the index around them, the job list of an indexed batch
// decode, the rule that cuts an encoder's bands at the entry rows, and which image of a batch gets an index.  Build with the
// sanitizers and run (tests/test_index_entries_host.py does):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o index_entries_check tools/index_entries_check.cpp && ./index_entries_check
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../nblic-image-compression_amd/csrc/index_entries.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool sealed_ok(const uint8_t *p, size_t n) {
    uint8_t d[32];
    sha256_of(p, n - 32, d);
    return memcmp(d, p + n - 32, 32) == 0;
}

// A synthetic stream of `len` bytes emitted in pieces of at most `piece` bytes; an entry in front of every `gap`-th byte
// (its window: the four bytes from there), written straight into an index buffer as the indexed batch does.
static int run(size_t len, size_t piece, size_t gap, int w, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<uint8_t> stream(len);
    for (auto &b : stream) b = uint8_t(rng());
    const size_t eb = index_entry_bytes(0, w, 1), window_at = kCheckpointHeadBytes + 24;
    const int count = int((len - 4) / gap);                              // every entry's window lies inside the stream
    std::vector<uint8_t> index(index_total_bytes(count, eb), 0xEE);
    PendingEntries pe;
    size_t emitted = 0; int made = 0;
    std::vector<unsigned long long> at;
    while (emitted < len) {
        size_t n = 1 + rng() % piece;
        if (n > len - emitted) n = len - emitted;
        // a band ends where an entry is due: the piece is cut there, as a band is cut at an entry row
        const size_t next_entry = size_t(made + 1) * gap;
        if (made < count && emitted < next_entry && emitted + n > next_entry) n = next_entry - emitted;
        pe.bytes(emitted, stream.data() + emitted, stream.data() + emitted + n);
        pe.bytes(emitted, stream.data() + emitted, stream.data() + emitted + n);      // handing bytes over twice changes nothing
        emitted += n;
        if (made < count && emitted == next_entry) {
            uint8_t *ck = index.data() + index_entry_at(made, eb);
            for (size_t k = 0; k < eb - 32; k++) ck[k] = uint8_t(made + k);
            pe.add(ck, eb, window_at, emitted);
            at.push_back(emitted);
            made++;
        }
    }
    CHECK(made == count && pe.waiting.empty() && pe.sealed == count && pe.fed == len);
    uint8_t head[kIndexHeadBytes];
    memset(head, 0x5A, sizeof head);
    index_close(index.data(), head, count, eb);
    CHECK(memcmp(index.data(), head, sizeof head) == 0 && sealed_ok(index.data(), index.size()));
    for (int k = 0; k < count; k++) {
        const uint8_t *ck = index.data() + index_entry_at(k, eb);
        unsigned long long n;
        memcpy(&n, ck - 8, 8);
        CHECK(n == eb && sealed_ok(ck, eb));
        uint32_t win;
        memcpy(&win, ck + window_at, 4);
        const uint8_t *s = stream.data() + at[size_t(k)];
        CHECK(win == (uint32_t(s[0]) << 24 | uint32_t(s[1]) << 16 | uint32_t(s[2]) << 8 | uint32_t(s[3])));
        CHECK(ck[0] == uint8_t(k) && ck[window_at + 4] == uint8_t(k + window_at + 4));    // nothing else of the entry was touched
    }
    return 0;
}

// The job list of an indexed batch decode on random mixes: every wanted row in exactly one job, rounds within the cap, an
// image's segments in rounds that never increase with the segment number.
static int plan_runs(unsigned seed) {
    std::mt19937 rng(seed);
    const int n = 1 + int(rng() % 12);
    std::vector<IndexedPlanImage> im;
    for (int k = 0; k < n; k++) {
        const int kind = int(rng() % 4) == 3, h = 2 + int(rng() % 70), every = 1 + int(rng() % unsigned(h - 1));
        const int r0 = int(rng() % unsigned(h)), r1 = r0 + 1 + int(rng() % unsigned(h - r0));
        im.push_back(IndexedPlanImage{kind, kind ? 0 : 1 + int(rng() % 3), h, 1 + int(rng() % 300), every, (rng() & 1) ? 0 : r0, (rng() & 1) ? h : r1});
        if (im.back().row1 <= im.back().row0) im.back().row1 = h;
    }
    for (int cap : {0, 1, 2, 3, 7}) {
        std::vector<IndexedJob> jobs;
        CHECK(indexed_decode_plan(im.data(), n, cap, jobs) && !jobs.empty());
        std::vector<std::vector<int>> hits(static_cast<size_t>(n));
        for (int k = 0; k < n; k++) hits[size_t(k)].assign(size_t(im[size_t(k)].h), 0);
        std::vector<int> per_round(jobs.size(), 0), last_round(size_t(n), -1), last_seg(size_t(n), 1 << 30);
        for (size_t j = 0; j < jobs.size(); j++) {
            const IndexedJob &J = jobs[j];
            const IndexedPlanImage &I = im[size_t(J.image)];
            const int end = J.end_row ? J.end_row : I.h;
            CHECK(J.first_row == J.segment * I.every && end > J.first_row && end <= I.h && (J.end_row == 0) == (end == I.h));
            CHECK(J.cls == indexed_class(I.kind, I.effort) && J.round >= 0 && size_t(J.round) < jobs.size());
            CHECK(j == 0 || J.round >= jobs[j - 1].round);
            CHECK(J.segment < last_seg[size_t(J.image)] && J.round >= last_round[size_t(J.image)]);      // listed last to first, rounds never decrease
            last_seg[size_t(J.image)] = J.segment; last_round[size_t(J.image)] = J.round;
            CHECK(++per_round[size_t(J.round)] <= (cap > 0 ? cap : int(jobs.size())) && (cap > 0 || J.round == 0));
            for (int r = J.first_row; r < end; r++) hits[size_t(J.image)][size_t(r)]++;
        }
        for (int k = 0; k < n; k++)
            for (int r = 0; r < im[size_t(k)].h; r++) {
                const bool wanted = r >= im[size_t(k)].row0 && r < im[size_t(k)].row1;
                CHECK(hits[size_t(k)][size_t(r)] <= 1 && (!wanted || hits[size_t(k)][size_t(r)] == 1));
            }
    }
    return 0;
}

// The band rule, exhaustively: the cuts of an h-row image in bands of at most `band` rows with an entry every `every` rows
// tile [0, h) in order, no cut has a multiple of `every` strictly inside it, and the cuts flagged "an entry behind this
// band" are exactly those that end at R, 2R, ..., ((h - 1) / R) R.
static int band_rule(int h, int band, int every) {
    std::vector<int> flagged;
    int row0 = 0, cuts = 0;
    while (row0 < h) {
        const BandCut c = index_band_cut(row0, band, h, every);
        CHECK(c.rows >= 1 && c.rows <= band && row0 + c.rows <= h && ++cuts <= h);
        if (every >= 1)
            for (int r = row0 + 1; r < row0 + c.rows; r++) CHECK(r % every != 0);
        if (c.entry) flagged.push_back(row0 + c.rows);
        row0 += c.rows;
    }
    CHECK(row0 == h);
    const int count = every >= 1 ? (h - 1) / every : 0;
    CHECK(int(flagged.size()) == count);
    for (int e = 0; e < count; e++) CHECK(flagged[size_t(e)] == (e + 1) * every);
    return 0;
}

// The admission rule against index_bytes: no index when R < 1 or R >= h, otherwise (h - 1) / R entries of
// index_entry_bytes each when the buffer holds index_bytes, and "too small" below that or for a codec without an index.
static int admission(int kind, int effort, int h, int w, int every) {
    const long need = index_bytes(kind, h, w, effort, every);
    const bool possible = every >= 1 && every < h;
    const IndexAdmission none = index_admit(kind, effort, h, w, every, 0);
    CHECK(none.every == 0 && none.count == 0 && none.entry_bytes == 0 && none.too_small == possible);
    if (!possible) { CHECK(need < 0 && !index_admit(kind, effort, h, w, every, ~size_t(0)).too_small); return 0; }
    const IndexAdmission all = index_admit(kind, effort, h, w, every, ~size_t(0));
    if (need < 0) { CHECK(all.every == 0 && all.too_small); return 0; }
    CHECK(index_admit(kind, effort, h, w, every, size_t(need) - 1).too_small);
    for (const IndexAdmission &a : {all, index_admit(kind, effort, h, w, every, size_t(need))}) {
        CHECK(!a.too_small && a.every == every && a.count == (h - 1) / every && a.entry_bytes == index_entry_bytes(kind, w, effort));
        CHECK(long(index_total_bytes(a.count, a.entry_bytes)) == need);
    }
    return 0;
}

int main() {
    for (int h = 1; h <= 40; h++)
        for (int band = 1; band <= h; band++)
            for (int every = 0; every <= h + 1; every++)
                if (band_rule(h, band, every)) return 1;
    for (int h : {1, 2, 3, 7, 40, 65535})
        for (int every : {-1, 0, 1, 2, 3, 6, 7, 39, 40, 41, 65534, 65535})
            for (int mode : {1, 2, 3, 4, 16, 17})                        // kind * 16 + effort: NBLIC -e1 .. -e3, -e4 (none), QNBLIC, QNBLIC effort 1 (none)
                if (admission(mode / 16, mode % 16, h, 37, every)) return 1;
    // sizes: head 96 | count x (8 | 168 + body + 32) | 32
    CHECK(index_bytes(0, 40, 37, 1, 5) == long(96 + 32 + 7 * (8 + 200 + 86080 + 74)));
    CHECK(index_bytes(0, 40, 37, 1, 39) == long(96 + 32 + 1 * (8 + 200 + 86080 + 74)));
    CHECK(index_bytes(0, 2, 1, 1, 1) == long(96 + 32 + 8 + 200 + 86080 + 2));
    CHECK(index_bytes(0, 23, 150, 2, 4) == long(96 + 32 + 5 * (8 + 200 + 86080 + 300 + 512 * 150)));
    CHECK(index_bytes(0, 23, 150, 3, 22) == long(96 + 32 + 8 + 200 + 86080 + 300 + 1024 * 150));
    CHECK(index_bytes(1, 64, 96, 0, 16) == long(96 + 32 + 3 * (8 + 200 + 12352 + 192 + 24576)));
    CHECK(index_bytes(0, 40, 37, 1, 0) == -1 && index_bytes(0, 40, 37, 1, 40) == -1 && index_bytes(0, 40, 37, 0, 5) == -1);
    CHECK(index_bytes(0, 40, 37, 4, 5) == -1 && index_bytes(1, 40, 37, 1, 5) == -1 && index_bytes(2, 40, 37, 1, 5) == -1);
    CHECK(index_bytes(0, 65536, 37, 1, 5) == -1 && index_bytes(0, 40, 0, 1, 5) == -1);
    // entries whose windows are completed by the same piece, one byte at a time, by a later piece, by the last four bytes
    unsigned seed = 1;
    for (size_t len : {8u, 9u, 64u, 1000u, 4099u})
        for (size_t piece : {1u, 2u, 3u, 5u, 64u, 5000u})
            for (size_t gap : {1u, 2u, 4u, 7u, 100u}) {
                if (gap + 4 > len) continue;
                if ((len - 4) / gap > 64) continue;                      // hundreds of 86 KB entries a few bytes apart: len 64's cases again, minutes under the sanitizers
                if (run(len, piece, gap, 1 + int(seed % 40), seed)) return 1;
                seed++;
            }
    for (unsigned p = 1; p <= 200; p++)
        if (plan_runs(p)) return 1;
    std::vector<IndexedJob> none;
    const IndexedPlanImage bad[2] = {{0, 1, 20, 30, 4, 0, 20}, {0, 1, 20, 30, 4, 5, 21}};
    CHECK(!indexed_decode_plan(bad, 2, 0, none) && none.empty() && !indexed_decode_plan(bad, 0, 0, none) && indexed_decode_plan(bad, 1, 0, none) && none.size() == 5);
    printf("index_entries_check ok: %u runs, 200 plans\n", seed - 1);
    return 0;
}
