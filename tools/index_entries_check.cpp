// Stand-alone check of index_entries.h (host only): the size of an index, entries that wait for their window while the
// stream is emitted in pieces of every size, and the assembly of the index around them.  Build with the sanitizers and run:
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

int main() {
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
                if (run(len, piece, gap, 1 + int(seed % 40), seed)) return 1;
                seed++;
            }
    printf("index_entries_check ok: %u runs\n", seed - 1);
    return 0;
}
