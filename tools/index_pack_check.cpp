// Stand-alone check of index_pack.h (host only): indexes put together here, byte by byte, pack and unpack to themselves for
// every kind and effort, odd widths, one and many entries, untouched, sparsely changed and full-range random tables; the
// fallbacks (rank bytes that are not the inverse, doubles the int64 form does not reproduce) go through their raw flags; cut,
// damaged and junk inputs are refused without a read outside the buffer.  Build with the sanitizers and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o index_pack_check tools/index_pack_check.cpp && ./index_pack_check
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../nblic-image-compression_amd/csrc/index_pack.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

enum Fill { kUntouched, kSparse, kRandom, kRandomIntB, kWide };

static void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
static void put_double(uint8_t *p, double v) { memcpy(p, &v, 8); }

// The body of a fresh decoder: the tables pack_initial names, everything else zero.
static void initial_body(std::vector<uint8_t> &body, const PackPart *P, int n) {
    for (int j = 0; j < n; j++)
        if (P[j].code == kCodeDiff || P[j].code == kCodeXor)
            for (uint32_t i = 0; i < P[j].bytes / P[j].unit; i++) store_unit(body.data() + P[j].at + size_t(i) * P[j].unit, P[j].unit, pack_initial(P[j].init, i));
    for (int j = 0; j < n; j++)
        if (P[j].code == kCodeRank) rank_inverse(body.data() + P[j + 1].at, body.data() + P[j].at);
}

static std::vector<uint8_t> make_index(int kind, int h, int w, int effort, int every, Fill fill, std::mt19937 &rng) {
    const int count = (h - 1) / every;
    const size_t eb = index_entry_bytes(kind, w, effort), bb = index_record_bytes(kind, w, effort);
    std::vector<uint8_t> ix(index_total_bytes(count, eb), 0);
    uint8_t head[kIndexHeadBytes] = {0};
    memcpy(head, "NBLSIDX1", 8);
    const int32_t f[9] = {1, kind, h, w, 0, 3, effort, every, count};
    memcpy(head + 8, f, sizeof f);
    for (size_t k = 56; k < kIndexHeadBytes; k++) head[k] = uint8_t(rng());
    PackPart P[kPackMaxParts];
    const int n = pack_parts(kind, w, effort, P);
    std::vector<uint8_t> body(bb, 0);
    initial_body(body, P, n);
    for (int k = 0; k < count; k++) {
        uint8_t *e = ix.data() + index_entry_at(k, eb);
        for (size_t i = 0; i < kCheckpointHeadBytes; i++) e[i] = uint8_t(rng());
        if (fill == kRandom || fill == kRandomIntB) {
            for (auto &b : body) b = uint8_t(rng());
            if (fill == kRandomIntB)
                for (int j = 0; j < n; j++) {
                    if (P[j].code == kCodeInt64)
                        for (uint32_t i = 0; i < P[j].bytes / 8; i++)
                            put_double(body.data() + P[j].at + size_t(i) * 8, double(int64_t(rng()) - (int64_t(1) << 31)) * double(1 << (rng() % 20)));
                    if (P[j].code == kCodeRank) rank_inverse(body.data() + P[j + 1].at, body.data() + P[j].at);
                }
        } else if (fill == kWide) {                                         // full-range contexts, counters and B (widths 32, 16, 63), the rest untouched
            for (int j = 0; j < n; j++) {
                const PackPart &p = P[j];
                if (p.code == kCodeDiff && p.init != kInitHits) for (uint32_t i = 0; i < p.bytes; i++) body[p.at + i] = uint8_t(rng());
                if (p.code == kCodeInt64)
                    for (uint32_t i = 0; i < p.bytes / 8; i++) put_double(body.data() + p.at + size_t(i) * 8, double((int64_t(rng()) << 30) * (rng() & 1 ? 1 : -1)));
            }
        } else if (fill == kSparse) {
            for (int j = 0; j < n; j++) {
                const PackPart &p = P[j];
                uint8_t *t = body.data() + p.at;
                if (p.code == kCodeNone) { for (uint32_t i = 0; i < p.bytes; i++) t[i] = uint8_t(rng()); continue; }
                if (p.code == kCodeRank) continue;
                const uint32_t units = p.bytes / p.unit;
                for (int c = 0; c < 40; c++) {
                    const uint32_t i = rng() % units;
                    if (p.code == kCodeInt64) put_double(t + size_t(i) * 8, double(int(rng() % 2000000) - 1000000));
                    else if (p.init == kInitSyms || p.unit == 2) t[size_t(i) * p.unit] = uint8_t(rng() % 20);
                    else put32(t + size_t(i) * 4, uint32_t(load_unit(t + size_t(i) * 4, 4)) + rng() % 300 - 150);
                }
            }
            for (int j = 0; j < n; j++) if (P[j].code == kCodeRank) rank_inverse(body.data() + P[j + 1].at, body.data() + P[j].at);
        }
        memcpy(e + kCheckpointHeadBytes, body.data(), bb);
        seal(e, eb);
    }
    index_close(ix.data(), head, count, eb);
    return ix;
}

static int round_trip(const std::vector<uint8_t> &ix, bool smaller, std::vector<uint8_t> *packed_out = nullptr) {
    std::vector<uint8_t> packed, back;
    CHECK(pack_index(ix.data(), ix.size(), packed));
    PackedView V;
    CHECK(packed_walk(packed.data(), packed.size(), V));
    CHECK(packed.size() <= index_pack_bound(V.H.count, V.entry_bytes));
    CHECK(index_pack_bound(V.H.count, V.entry_bytes) == ix.size() + 32 + 33 * size_t(V.H.count));
    CHECK(index_is_packed(packed.data(), packed.size()) && !index_is_packed(ix.data(), ix.size()));
    CHECK(index_unpacked_bytes(packed.data(), packed.size()) == ix.size());
    CHECK(unpack_index(packed.data(), packed.size(), back));
    CHECK(back == ix);
    if (smaller) CHECK(packed.size() < ix.size());
    if (packed_out) *packed_out = packed;
    return 0;
}

static void rehash(std::vector<uint8_t> &p, const PackedView &V, int k) {
    const PackedEntry &E = V.ent[size_t(k)];
    sha256_of(p.data() + E.head_at, E.seal_at + 32 - E.head_at, p.data() + E.seal_at + 32);
    seal(p.data(), p.size());
}

static int refusals(std::mt19937 &rng) {
    const std::vector<uint8_t> ix = make_index(0, 7, 5, 2, 2, kSparse, rng);
    std::vector<uint8_t> good, out;
    if (round_trip(ix, true, &good)) return 1;
    PackedView V, W;
    CHECK(packed_walk(good.data(), good.size(), V));
    // cut at every structural boundary (and one byte to either side), the seal made right again where there is room for one
    std::vector<size_t> cuts = {0, 8, kIndexHeadBytes, kPackedHeadBytes, good.size() - 32, good.size() - 1};
    for (const PackedEntry &E : V.ent) {
        cuts.push_back(E.head_at - 8); cuts.push_back(E.head_at); cuts.push_back(E.head_at + kCheckpointHeadBytes); cuts.push_back(E.seal_at); cuts.push_back(E.seal_at + 32);
        for (int j = 0; j < V.n_parts; j++) cuts.push_back(E.part_at[j]);
    }
    for (size_t c : cuts)
        for (int d = -1; d <= 1; d++) {
            const size_t n = c + size_t(d);
            if (n >= good.size()) continue;
            std::vector<uint8_t> cut(good.begin(), good.begin() + ptrdiff_t(n));
            CHECK(!packed_walk(cut.data(), cut.size(), W) && !unpack_index(cut.data(), cut.size(), out));
            if (n >= 32 && n + 32 != good.size()) {
                cut.resize(n + 32);
                seal(cut.data(), cut.size());
                CHECK(!packed_walk(cut.data(), cut.size(), W) && !unpack_index(cut.data(), cut.size(), out));
            }
        }
    // a width byte outside its unit's range (part 1: 4-byte units), hashes made right
    {
        std::vector<uint8_t> b = good;
        CHECK(V.ent[1].part_flag[1] == kPartCoded);
        b[V.ent[1].part_at[1]] = 33;
        rehash(b, V, 1);
        CHECK(!packed_walk(b.data(), b.size(), W) && !unpack_index(b.data(), b.size(), out));
        b[V.ent[1].part_at[1]] = 32;                                        // in range, but the lengths no longer add up
        rehash(b, V, 1);
        CHECK(!packed_walk(b.data(), b.size(), W));
    }
    // a packed length pointing past the end
    {
        std::vector<uint8_t> b = good;
        const unsigned long long len = b.size();
        memcpy(b.data() + V.ent[2].head_at - 8, &len, 8);
        seal(b.data(), b.size());
        CHECK(!packed_walk(b.data(), b.size(), W) && !unpack_index(b.data(), b.size(), out));
        const unsigned long long huge = ~0ull - 7;
        memcpy(b.data() + V.ent[0].head_at - 8, &huge, 8);
        seal(b.data(), b.size());
        CHECK(!packed_walk(b.data(), b.size(), W));
    }
    // a flipped payload bit: the entry's hash catches it; with the hashes made right the walk passes and unpack's seal refuses
    {
        std::vector<uint8_t> b = good;
        const size_t at = V.ent[1].seal_at - 3;                              // inside the raw rows, the last part
        b[at] ^= 4;
        seal(b.data(), b.size());
        CHECK(!packed_walk(b.data(), b.size(), W));
        rehash(b, V, 1);
        CHECK(packed_walk(b.data(), b.size(), W));
        CHECK(!unpack_index(b.data(), b.size(), out) && out.empty());
    }
    // junk
    for (int t = 0; t < 300; t++) {
        std::vector<uint8_t> j(rng() % 600);
        for (auto &b : j) b = uint8_t(rng());
        if (t & 1 && j.size() >= 8) memcpy(j.data(), "NBLSIDXP", 8);
        CHECK(!packed_walk(j.data(), j.size(), W) && !unpack_index(j.data(), j.size(), out) && !pack_index(j.data(), j.size(), out));
    }
    CHECK(!pack_index(good.data(), good.size(), out));                        // a packed index is not packed again
    CHECK(!pack_index(ix.data(), ix.size() - 1, out) && !pack_index(nullptr, 0, out) && !packed_walk(nullptr, 0, W));
    return 0;
}

static int fallbacks(std::mt19937 &rng) {
    for (int which = 0; which < 5; which++) {
        std::vector<uint8_t> ix = make_index(0, 5, 6, 2, 2, kSparse, rng);
        const size_t eb = index_entry_bytes(0, 6, 2);
        PackPart P[kPackMaxParts];
        const int n = pack_parts(0, 6, 2, P);
        uint8_t *e = ix.data() + index_entry_at(1, eb), *body = e + kCheckpointHeadBytes;
        int part = 6;
        CHECK(n == 8 && P[6].code == kCodeInt64 && P[4].code == kCodeRank);
        const uint64_t nan_bits = 0x7FF8000000000001ull;
        switch (which) {
            case 0: part = 4; body[P[4].at + 7] ^= 1; break;                  // rank bytes that are not the inverse
            case 1: put_double(body + P[6].at + 16, 0.5); break;
            case 2: put_double(body + P[6].at + 16, -0.0); break;
            case 3: put_double(body + P[6].at + 16, 9223372036854775808.0); break;
            default: memcpy(body + P[6].at + 16, &nan_bits, 8); break;
        }
        seal(e, eb);
        seal(ix.data(), ix.size());
        std::vector<uint8_t> packed;
        if (round_trip(ix, true, &packed)) return 1;
        PackedView V;
        CHECK(packed_walk(packed.data(), packed.size(), V));
        CHECK(V.ent[1].part_flag[part] == kPartRaw && V.ent[0].part_flag[part] != kPartRaw);
    }
    return 0;
}

int main() {
    std::mt19937 rng(12345);
    // the bit fields: a few thousand seeded random tables of every width
    for (int t = 0; t < 4000; t++) {
        const uint32_t bits = rng() % 65, n = t == 0 ? 65 : t == 1 ? 127 : 1 + rng() % 200;      // (last blocks of 1 and of 63 units first)
        std::vector<uint64_t> v(n);
        for (auto &x : v) x = ((uint64_t(rng()) << 32) | rng()) & unit_mask(bits) & (rng() % 4 ? ~0ull : unit_mask(rng() % 65));
        std::vector<uint8_t> out;
        code_blocks(v.data(), n, out);
        const size_t nb = (n + 63) / 64;
        size_t at = nb;
        for (size_t b = 0; b < nb; b++) {
            CHECK(out[b] <= bits);
            for (size_t i = b * 64; i < n && i < (b + 1) * 64; i++) CHECK(get_bits(out.data() + at, (i - b * 64) * out[b], out[b]) == v[i]);
            at += 8 * size_t(out[b]);
        }
        CHECK(at == out.size());
        const uint32_t ub = 16 << (rng() % 3);
        const uint64_t d = ((uint64_t(rng()) << 32) | rng()) & unit_mask(ub);
        CHECK(unzigzag(zigzag(d, ub), ub) == d);
    }
    // every kind and effort; odd W, W = 2 mod 4; one entry and 64; last blocks of 1 unit (W = 8 x 64 + 1 ... per column 64
    // doubles: W columns are whole blocks, so the short blocks come from the rows: 2 W = 4 x 64 + 4 -> W = 130; 63: W = 126)
    const struct { int kind, h, w, effort, every; } shapes[] = {
        {0, 5, 3, 1, 2}, {0, 6, 6, 2, 5}, {0, 4, 7, 3, 1}, {1, 9, 5, 0, 2}, {1, 3, 10, 0, 2}, {0, 65, 4, 1, 1}, {1, 65, 2, 0, 1},
        {0, 3, 130, 1, 2}, {0, 3, 126, 2, 2}, {0, 20, 24, 1, 19}};
    int runs = 0;
    for (const auto &s : shapes)
        for (Fill f : {kUntouched, kSparse, kRandom, kRandomIntB, kWide}) {
            if (s.h == 65 && f != kSparse) continue;                         // the long chains: once each is enough
            const std::vector<uint8_t> ix = make_index(s.kind, s.h, s.w, s.effort, s.every, f, rng);
            if (round_trip(ix, f == kUntouched || f == kSparse || f == kWide)) return 1;
            runs++;
        }
    // untouched tables: every block has width 0
    {
        const std::vector<uint8_t> ix = make_index(0, 5, 4, 3, 2, kUntouched, rng);
        std::vector<uint8_t> packed;
        if (round_trip(ix, true, &packed)) return 1;
        PackedView V;
        CHECK(packed_walk(packed.data(), packed.size(), V));
        for (const PackedEntry &E : V.ent)
            for (int j = 0; j < V.n_parts; j++) {
                if (V.parts[j].code == kCodeRank) CHECK(E.part_flag[j] == kPartLeftOut);
                if (E.part_flag[j] != kPartCoded) continue;
                for (uint32_t b = 0; b < part_blocks(V.parts[j]); b++) CHECK(packed[E.part_at[j] + b] == 0);
            }
    }
    // seeded random indexes of small shapes
    for (int t = 0; t < 24; t++) {
        const int kind = int(rng() % 4 == 0), effort = kind ? 0 : 1 + int(rng() % 3), h = 2 + int(rng() % 6), w = 1 + int(rng() % 40);
        const std::vector<uint8_t> ix = make_index(kind, h, w, effort, 1 + int(rng() % (h - 1)), Fill(rng() % 4), rng);
        if (round_trip(ix, false)) return 1;
        runs++;
    }
    if (fallbacks(rng) || refusals(rng)) return 1;
    printf("index_pack_check ok: %d indexes\n", runs);
    return 0;
}
