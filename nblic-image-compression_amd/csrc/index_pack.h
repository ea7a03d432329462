// index_pack.h -- the PACKED form of a seek index: the same information as the index of index_entries.h, delta-coded entry
// against entry and bit-packed.  It converts to and from that index byte for byte.  No HIP, no device: the stand-alone
// check (tools/index_pack_check.cpp) compiles this file alone, under the sanitizers.  (Little-endian hosts, as everywhere.)
//
// Layout:
//   head (96)          the IndexHead of the index it stands for, with the magic "NBLSIDXP" and version kPackedVersion
//   unpacked seal (32) the last 32 bytes of that index: the SHA-256 unpack_index must arrive at
//   count x (uint64 packed length | packed entry)
//   SHA-256 of everything before it
// A packed entry:  checkpoint head (168, verbatim) | body | the entry's own seal (32, verbatim) | SHA-256 of this packed
// entry up to here.  The body is one flag byte -- kBodyRaw: the entry's body follows verbatim; kBodyCoded: its parts follow,
// in the order pack_parts lists them.  A part is one flag byte and its data:
//   kPartRaw      the part's bytes, verbatim
//   kPartLeftOut  nothing (the symbol -> rank bytes: the inverse of the rank -> symbol bytes, rank_inverse)
//   kPartCoded    the part as units of `unit` bytes, each turned into a VALUE against a base -- kCodeDiff: zig-zag of the
//                 signed difference (modulo the unit) to the same unit of the previous entry, for entry 0 to the table a fresh
//                 decoder starts from (pack_initial); kCodeXor: the unit XOR that base; kCodeInt64: zig-zag of the double
//                 converted to int64, no base -- and the values cut into blocks of 64 (the last may be short): first ONE WIDTH
//                 BYTE b per block, the bits of its largest value (0 .. 8 unit), all blocks' together; then per block 8 b
//                 payload bytes, lane i's value at bit i b, little-endian.  A block of zeros costs its width byte alone, and
//                 a block's payload starts at 8 x (the sum of the width bytes in front of it) behind the width bytes.
#pragma once
#include <math.h>

#include "index_entries.h"

namespace nblic {

constexpr size_t kPackedHeadBytes = kIndexHeadBytes + 32;
constexpr uint32_t kPackedVersion = 1, kUnpackedVersion = 1;
constexpr int kPackMaxParts = 8, kPackBlock = 64;
enum : uint8_t { kBodyRaw = 0, kBodyCoded = 1 };
enum : uint8_t { kPartRaw = 0, kPartCoded = 1, kPartLeftOut = 2 };
enum : uint32_t { kCodeNone = 0, kCodeDiff = 1, kCodeXor = 2, kCodeInt64 = 3, kCodeRank = 4 };
enum : uint32_t { kInitZero = 0, kInitCounters = 1, kInitHits = 2, kInitSyms = 3 };
constexpr uint32_t kPackMapSyms = 20, kPackMappers = 512;               // model.h kMapSyms; the re-mappers of a record

// One part of an entry's body: where it lies, how it is coded.  Raw parts (kCodeNone) are walked in 4-byte units, the last
// one possibly short.
struct PackPart { uint32_t at, bytes, unit, code, init; };
inline uint32_t part_units(const PackPart &p) { return (p.bytes + p.unit - 1) / p.unit; }
inline uint32_t part_blocks(const PackPart &p) { return (part_units(p) + kPackBlock - 1) / kPackBlock; }

// The parts of a body, in body order; 0: kind / effort out of range.  The record's tables: serial_engine.h kRecCount ...
inline int pack_parts(int kind, int w, int effort, PackPart *P) {
    if (index_record_bytes(kind, w, effort) == 0 || w < 1 || w > kIndexMaxSide) return 0;
    const uint32_t rows = 2 * uint32_t(w);
    int n = 0;
    P[n++] = PackPart{0, 64, 4, kCodeNone, kInitZero};                              // SerialState
    if (kind == 0) {
        const uint32_t b_bytes = uint32_t(effort == 3 ? 1024 : effort == 2 ? 512 : 0) * uint32_t(w);
        P[n++] = PackPart{64, 2048 * 4, 4, kCodeDiff, kInitZero};                     // context biases
        P[n++] = PackPart{64 + 8192, 4096 * 4, 2, kCodeDiff, kInitCounters};          // counters, c0 | c1 << 16: the halves
        P[n++] = PackPart{64 + 24576, 10240 * 4, 4, kCodeDiff, kInitHits};            // re-mapper hit counts
        P[n++] = PackPart{64 + 65536, 10240, 4, kCodeRank, kInitZero};                // symbol -> rank bytes
        P[n++] = PackPart{64 + 75776, 10240, 4, kCodeXor, kInitSyms};                 // rank -> symbol bytes
        if (b_bytes) P[n++] = PackPart{uint32_t(kNblicRecordBytes), b_bytes, 8, kCodeInt64, kInitZero};
        P[n++] = PackPart{uint32_t(kNblicRecordBytes) + b_bytes, rows, 4, kCodeNone, kInitZero};
    } else {
        P[n++] = PackPart{64, 3072 * 4, 4, kCodeDiff, kInitZero};                     // contexts
        P[n++] = PackPart{uint32_t(kQnblicRecordBytes), rows, 4, kCodeNone, kInitZero};
        P[n++] = PackPart{uint32_t(kQnblicRecordBytes) + rows, uint32_t(kQnblicTableBytes), 4, kCodeXor, kInitZero};
    }
    return n;
}
static_assert(64 + 86016 == kNblicRecordBytes && 64 + 12288 == kQnblicRecordBytes, "the parts cover the records");

enum : int { kPartCounters = 2, kPartRank = 4, kPartSyms = 5, kQPartTab = 3 };        // where pack_parts puts them

// Unit i of the table a fresh decoder starts from (serial_engine.hip k_serial_decode, i0 == 0).
inline uint64_t pack_initial(uint32_t init, uint32_t i) {
    switch (init) {
        case kInitCounters: return 32;                                             // kWeightOne, both halves
        case kInitHits: return 2 * (kPackMapSyms - 1 - i % kPackMapSyms);
        case kInitSyms: return 0x03020100u + 0x04040404u * (i % (kPackMapSyms / 4));  // bytes 4 i .. 4 i + 3, each modulo 20
        default: return 0;
    }
}

// A packed index is never larger than this: every body stored raw.
constexpr size_t index_pack_bound(int count, size_t entry_bytes) {
    return kPackedHeadBytes + size_t(count) * (8 + entry_bytes + 1 + 32) + 32;
}

// ---- units, values, blocks ---------------------------------------------------------------------------------------------------
inline uint64_t unit_mask(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }
inline uint64_t load_unit(const uint8_t *p, uint32_t bytes) { uint64_t v = 0; memcpy(&v, p, bytes); return v; }
inline void store_unit(uint8_t *p, uint32_t bytes, uint64_t v) { memcpy(p, &v, bytes); }
inline uint64_t zigzag(uint64_t d, uint32_t bits) {                              // d: a signed difference modulo 2^bits
    const uint64_t sign = (d >> (bits - 1)) & 1;
    return ((d << 1) ^ (sign ? ~0ull : 0ull)) & unit_mask(bits);
}
inline uint64_t unzigzag(uint64_t z, uint32_t bits) { return ((z >> 1) ^ ((z & 1) ? ~0ull : 0ull)) & unit_mask(bits); }
inline uint32_t bits_of(uint64_t v) { uint32_t b = 0; while (v) { b++; v >>= 1; } return b; }

inline void put_bits(uint8_t *p, size_t bit, uint32_t bits, uint64_t v) {
    size_t at = bit >> 3;
    uint32_t sh = uint32_t(bit & 7);
    while (bits) {
        const uint32_t take = 8 - sh < bits ? 8 - sh : bits;
        p[at] = uint8_t(p[at] | ((v & ((1u << take) - 1)) << sh));
        v >>= take; bits -= take; at++; sh = 0;
    }
}
inline uint64_t get_bits(const uint8_t *p, size_t bit, uint32_t bits) {
    size_t at = bit >> 3;
    uint32_t sh = uint32_t(bit & 7), got = 0;
    uint64_t v = 0;
    while (got < bits) {
        const uint32_t take = 8 - sh < bits - got ? 8 - sh : bits - got;
        v |= uint64_t((p[at] >> sh) & ((1u << take) - 1)) << got;
        got += take; at++; sh = 0;
    }
    return v;
}

// n values as blocks: the width bytes, then the payloads.
inline void code_blocks(const uint64_t *v, size_t n, std::vector<uint8_t> &out) {
    const size_t nb = (n + kPackBlock - 1) / kPackBlock, w_at = out.size();
    out.resize(w_at + nb);
    for (size_t b = 0; b < nb; b++) {
        uint64_t m = 0;
        for (size_t i = b * kPackBlock; i < n && i < (b + 1) * kPackBlock; i++) m |= v[i];
        out[w_at + b] = uint8_t(bits_of(m));
    }
    for (size_t b = 0; b < nb; b++) {
        const uint32_t width = out[w_at + b];
        const size_t at = out.size();
        out.resize(at + 8 * size_t(width), 0);
        for (size_t i = b * kPackBlock; i < n && i < (b + 1) * kPackBlock; i++) put_bits(out.data() + at, (i - b * kPackBlock) * width, width, v[i]);
    }
}

// The symbol -> rank bytes as k_index_capture rebuilds them from the rank -> symbol bytes: rank[m][s] = the last i at which
// sym[m][i] == s, 0 for a symbol the re-mapper does not name.
inline void rank_inverse(const uint8_t *sym, uint8_t *rank) {
    for (uint32_t m = 0; m < kPackMappers; m++)
        for (uint32_t s = 0; s < kPackMapSyms; s++) {
            uint8_t r = 0;
            for (uint32_t i = 0; i < kPackMapSyms; i++) if (sym[m * kPackMapSyms + i] == s) r = uint8_t(i);
            rank[m * kPackMapSyms + s] = r;
        }
}

// A double the int64 form reproduces bit for bit: an integer of magnitude < 2^62, not -0.0.
inline bool double_packs(const uint8_t *p, int64_t &out) {
    double v;
    memcpy(&v, p, 8);
    if (!(v == v) || !(fabs(v) < 4611686018427387904.0)) return false;
    const int64_t i = int64_t(v);
    const double back = double(i);
    if (memcmp(&back, p, 8) != 0) return false;                                 // not an integer, or -0.0
    out = i;
    return true;
}

// ---- packing -----------------------------------------------------------------------------------------------------------------
// The coded body of an entry (`prev`: the previous entry's body, null for entry 0), its flag byte included, appended to out.
inline void pack_body(const uint8_t *prev, const uint8_t *body, size_t body_bytes, const PackPart *P, int n_parts, std::vector<uint8_t> &out) {
    const size_t start = out.size();
    out.push_back(kBodyCoded);
    std::vector<uint64_t> v;
    for (int k = 0; k < n_parts; k++) {
        const PackPart &p = P[k];
        const uint8_t *src = body + p.at;
        uint8_t flag = kPartRaw;
        if (p.code == kCodeDiff || p.code == kCodeXor) {
            const uint32_t n = p.bytes / p.unit, bits = 8 * p.unit;
            v.resize(n);
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t x = load_unit(src + size_t(i) * p.unit, p.unit);
                const uint64_t base = prev ? load_unit(prev + p.at + size_t(i) * p.unit, p.unit) : pack_initial(p.init, i);
                v[i] = p.code == kCodeDiff ? zigzag((x - base) & unit_mask(bits), bits) : x ^ base;
            }
            flag = kPartCoded;
        } else if (p.code == kCodeInt64) {
            const uint32_t n = p.bytes / 8;
            v.resize(n);
            flag = kPartCoded;
            for (uint32_t i = 0; i < n && flag == kPartCoded; i++) {
                int64_t x;
                if (double_packs(src + size_t(i) * 8, x)) v[i] = zigzag(uint64_t(x), 64); else flag = kPartRaw;
            }
        } else if (p.code == kCodeRank) {
            std::vector<uint8_t> inv(p.bytes);
            rank_inverse(body + P[k + 1].at, inv.data());                       // the rank -> symbol bytes are the next part
            if (memcmp(inv.data(), src, p.bytes) == 0) flag = kPartLeftOut;
        }
        out.push_back(flag);
        if (flag == kPartCoded) code_blocks(v.data(), v.size(), out);
        else if (flag == kPartRaw) out.insert(out.end(), src, src + p.bytes);
    }
    if (out.size() - start >= 1 + body_bytes) {                                  // coding did not make it smaller
        out.resize(start);
        out.push_back(kBodyRaw);
        out.insert(out.end(), body, body + body_bytes);
    }
}

// The fields of an IndexHead that this file needs, read by offset (pipeline.hip asserts the offsets against the struct).
struct PackHead { uint32_t version; int kind, h, w, effort, every, count; };
constexpr size_t kHeadVersionAt = 8, kHeadKindAt = 12, kHeadHAt = 16, kHeadWAt = 20, kHeadEffortAt = 32, kHeadEveryAt = 36, kHeadCountAt = 40;
inline bool pack_head(const uint8_t *p, size_t n, const char *magic, uint32_t version, PackHead &H) {
    if (!p || n < kIndexHeadBytes || memcmp(p, magic, 8) != 0) return false;
    int32_t f[9];
    memcpy(f, p + kHeadVersionAt, sizeof f);
    H = PackHead{uint32_t(f[0]), f[1], f[2], f[3], f[6], f[7], f[8]};
    return H.version == version && index_bytes(H.kind, H.h, H.w, H.effort, H.every) >= 0 && H.count == (H.h - 1) / H.every;
}

inline bool index_is_packed(const void *p, size_t n) { return p && n >= 8 && memcmp(p, "NBLSIDXP", 8) == 0; }
// The size of the index a packed one stands for, from its head alone; 0: not a packed index's head.
inline size_t index_unpacked_bytes(const void *p, size_t n) {
    PackHead H;
    if (!pack_head(static_cast<const uint8_t *>(p), n, "NBLSIDXP", kPackedVersion, H)) return 0;
    return index_total_bytes(H.count, index_entry_bytes(H.kind, H.w, H.effort));
}

// An index (structurally sound: head, lengths; its hashes are NOT looked at here) as a packed one.  false: refused.
inline bool pack_index(const void *index, size_t n, std::vector<uint8_t> &out) {
    const uint8_t *p = static_cast<const uint8_t *>(index);
    PackHead H;
    out.clear();
    if (!pack_head(p, n, "NBLSIDX1", kUnpackedVersion, H)) return false;
    const size_t eb = index_entry_bytes(H.kind, H.w, H.effort), body_bytes = index_record_bytes(H.kind, H.w, H.effort);
    if (n != index_total_bytes(H.count, eb)) return false;
    PackPart P[kPackMaxParts];
    const int n_parts = pack_parts(H.kind, H.w, H.effort, P);
    out.insert(out.end(), p, p + kIndexHeadBytes);
    memcpy(out.data(), "NBLSIDXP", 8);
    const uint32_t version = kPackedVersion;
    memcpy(out.data() + kHeadVersionAt, &version, 4);
    out.insert(out.end(), p + n - 32, p + n);
    const uint8_t *prev = nullptr;
    for (int k = 0; k < H.count; k++) {
        const uint8_t *e = p + index_entry_at(k, eb);
        unsigned long long len;
        memcpy(&len, e - 8, 8);
        if (len != eb) { out.clear(); return false; }
        const size_t len_at = out.size();
        out.resize(len_at + 8);
        out.insert(out.end(), e, e + kCheckpointHeadBytes);
        pack_body(prev, e + kCheckpointHeadBytes, body_bytes, P, n_parts, out);
        out.insert(out.end(), e + eb - 32, e + eb);
        const size_t hashed = out.size() - (len_at + 8);
        out.resize(out.size() + 32);
        sha256_of(out.data() + len_at + 8, hashed, out.data() + out.size() - 32);
        len = hashed + 32;
        memcpy(out.data() + len_at, &len, 8);
        prev = e + kCheckpointHeadBytes;
    }
    out.resize(out.size() + 32);
    seal(out.data(), out.size());
    return true;
}

// ---- reading: the structural walk every reader starts with -------------------------------------------------------------------
// Where the entries of a packed index and the parts of their bodies lie.  For a body stored raw every part is kPartRaw at its
// place in that body.  part_at: the part's data (behind its flag byte), in bytes from the start of the packed index.
struct PackedEntry {
    size_t head_at, seal_at;
    size_t part_at[kPackMaxParts];
    uint8_t part_flag[kPackMaxParts];
};
struct PackedView {
    PackHead H;
    PackPart parts[kPackMaxParts];
    int n_parts = 0;
    size_t body_bytes = 0, entry_bytes = 0;
    std::vector<PackedEntry> ent;
};

// Every length, flag and width byte of a packed index, its entries' hashes and its own: after this, nothing a reader (host
// or device) derives from the flags and width bytes lies outside [0, n).  false: refused.
inline bool packed_walk(const void *packed, size_t n, PackedView &V) {
    const uint8_t *p = static_cast<const uint8_t *>(packed);
    V.ent.clear();
    if (!p || n < kPackedHeadBytes + 32 || !pack_head(p, n, "NBLSIDXP", kPackedVersion, V.H)) return false;
    uint8_t d[32];
    sha256_of(p, n - 32, d);
    if (memcmp(d, p + n - 32, 32) != 0) return false;
    V.n_parts = pack_parts(V.H.kind, V.H.w, V.H.effort, V.parts);
    V.body_bytes = index_record_bytes(V.H.kind, V.H.w, V.H.effort);
    V.entry_bytes = index_entry_bytes(V.H.kind, V.H.w, V.H.effort);
    const size_t end = n - 32;
    size_t at = kPackedHeadBytes;
    for (int k = 0; k < V.H.count; k++) {
        unsigned long long len;
        if (end - at < 8) return false;
        memcpy(&len, p + at, 8);
        at += 8;
        if (len > end - at || len < kCheckpointHeadBytes + 1 + 64) return false;
        const size_t stop = at + size_t(len) - 64;                               // the entry's seal, then the packed entry's hash
        sha256_of(p + at, size_t(len) - 32, d);
        if (memcmp(d, p + stop + 32, 32) != 0) return false;
        PackedEntry E{};
        E.head_at = at; E.seal_at = stop;
        size_t q = at + kCheckpointHeadBytes;
        const uint8_t body_flag = p[q++];
        if (body_flag == kBodyRaw) {
            if (stop - q != V.body_bytes) return false;
            for (int j = 0; j < V.n_parts; j++) { E.part_at[j] = q + V.parts[j].at; E.part_flag[j] = kPartRaw; }
        } else if (body_flag == kBodyCoded) {
            for (int j = 0; j < V.n_parts; j++) {
                const PackPart &P = V.parts[j];
                if (q >= stop) return false;
                const uint8_t flag = p[q++];
                E.part_flag[j] = flag; E.part_at[j] = q;
                if (flag == kPartRaw) {
                    if (stop - q < P.bytes) return false;
                    q += P.bytes;
                } else if (flag == kPartLeftOut) {
                    if (P.code != kCodeRank) return false;
                } else if (flag == kPartCoded) {
                    if (P.code != kCodeDiff && P.code != kCodeXor && P.code != kCodeInt64) return false;
                    const size_t nb = part_blocks(P);
                    if (stop - q < nb) return false;
                    size_t payload = 0;
                    for (size_t b = 0; b < nb; b++) {
                        if (p[q + b] > 8 * P.unit) return false;
                        payload += 8 * size_t(p[q + b]);
                    }
                    q += nb;
                    if (stop - q < payload) return false;
                    q += payload;
                } else {
                    return false;
                }
            }
            if (q != stop) return false;
        } else {
            return false;
        }
        V.ent.push_back(E);
        at += size_t(len);
    }
    return at == end;
}

// Part j of entry k of a walked index into out (the part's bytes); prev: the same part of entry k - 1 (null for entry 0);
// sym: for a left-out rank part, this entry's rank -> symbol bytes.
inline void unpack_part(const uint8_t *p, const PackedView &V, int k, int j, const uint8_t *prev, const uint8_t *sym, uint8_t *out) {
    const PackPart &P = V.parts[j];
    const PackedEntry &E = V.ent[size_t(k)];
    const uint8_t *src = p + E.part_at[j];
    if (E.part_flag[j] == kPartRaw) { memcpy(out, src, P.bytes); return; }
    if (E.part_flag[j] == kPartLeftOut) { rank_inverse(sym, out); return; }
    const uint32_t n = P.bytes / P.unit, bits = 8 * P.unit;
    const size_t nb = part_blocks(P);
    const uint8_t *payload = src + nb;
    for (size_t b = 0; b < nb; b++) {
        const uint32_t width = src[b];
        for (uint32_t i = uint32_t(b) * kPackBlock; i < n && i < (uint32_t(b) + 1) * kPackBlock; i++) {
            const uint64_t v = get_bits(payload, size_t(i - b * kPackBlock) * width, width);
            uint64_t x;
            if (P.code == kCodeInt64) {
                const double dv = double(int64_t(unzigzag(v, 64)));
                memcpy(&x, &dv, 8);
            } else {
                const uint64_t base = prev ? load_unit(prev + size_t(i) * P.unit, P.unit) : pack_initial(P.init, i);
                x = P.code == kCodeDiff ? (base + unzigzag(v, bits)) & unit_mask(bits) : v ^ base;
            }
            store_unit(out + size_t(i) * P.unit, P.unit, x);
        }
        payload += 8 * size_t(width);
    }
}

// The body of entry k of a walked index (prev: the body of entry k - 1, null for entry 0).
inline void unpack_body(const uint8_t *p, const PackedView &V, int k, const uint8_t *prev, uint8_t *body) {
    int rank = -1;
    for (int j = 0; j < V.n_parts; j++) {
        if (V.ent[size_t(k)].part_flag[j] == kPartLeftOut) { rank = j; continue; }
        unpack_part(p, V, k, j, prev ? prev + V.parts[j].at : nullptr, nullptr, body + V.parts[j].at);
    }
    if (rank >= 0) unpack_part(p, V, k, rank, nullptr, body + V.parts[rank + 1].at, body + V.parts[rank].at);
}

// The index a packed one stands for.  Every entry is re-derived and sealed again; a seal that differs from the stored one, or
// a final seal that does, is a refusal.  false: refused (out is empty then).
inline bool unpack_index(const void *packed, size_t n, std::vector<uint8_t> &out) {
    const uint8_t *p = static_cast<const uint8_t *>(packed);
    PackedView V;
    out.clear();
    if (!packed_walk(p, n, V)) return false;
    const size_t eb = V.entry_bytes;
    out.assign(index_total_bytes(V.H.count, eb), 0);
    memcpy(out.data(), p, kIndexHeadBytes);
    memcpy(out.data(), "NBLSIDX1", 8);
    const uint32_t version = kUnpackedVersion;
    memcpy(out.data() + kHeadVersionAt, &version, 4);
    const uint8_t *prev = nullptr;
    for (int k = 0; k < V.H.count; k++) {
        uint8_t *e = out.data() + index_entry_at(k, eb);
        const unsigned long long len = eb;
        memcpy(e - 8, &len, 8);
        memcpy(e, p + V.ent[size_t(k)].head_at, kCheckpointHeadBytes);
        unpack_body(p, V, k, prev, e + kCheckpointHeadBytes);
        seal(e, eb);
        if (memcmp(e + eb - 32, p + V.ent[size_t(k)].seal_at, 32) != 0) { out.clear(); return false; }
        prev = e + kCheckpointHeadBytes;
    }
    seal(out.data(), out.size());
    if (memcmp(out.data() + out.size() - 32, p + kIndexHeadBytes, 32) != 0) { out.clear(); return false; }
    return true;
}

}  // namespace nblic
