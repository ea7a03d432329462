// index_entries.h -- the host-only part of writing a seek index while encoding (pipeline.hip: the band encoder and the
// indexed batch): how large an index is, where its entries sit, which rows they stand in front of and how an encoder's
// bands are cut there, which image of a batch gets an index, and the entries that WAIT.  An entry written down at
// an entry row lacks one field, the decoder's 4-byte window: the four stream bytes behind the entry's position, which
// the coder has not emitted yet (the final flush always provides them).  PendingEntries hands every emitted stream
// byte to the entries that wait for it and seals an entry once its window is complete.  The job list of an indexed batch
// decode and the launch schedule of a batch index build are laid out here too.  No HIP, no device: the stand-alone
// checks (tools/index_entries_check.cpp, tools/index_build_plan_check.cpp) compile this file alone, under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "sha256.h"

namespace nblic {

inline void sha256_of(const void *p, size_t n, uint8_t out[32]) {
    Sha256 s;
    s.update(static_cast<const uint8_t *>(p), n);
    s.digest(out);
}
// A sealed record: a head (magic, format version, ...), a body, and the SHA-256 of both in its last 32 bytes.
inline void seal(uint8_t *buf, size_t n) { sha256_of(buf, n - 32, buf + n - 32); }

// ---- sizes (pipeline.hip asserts them against the structs and constants they stand for) --------------------------------
constexpr size_t kIndexHeadBytes = 96, kCheckpointHeadBytes = 168;                   // IndexHead, DecodeCheckpoint
constexpr size_t kNblicRecordBytes = 86080, kQnblicRecordBytes = 12352, kQnblicTableBytes = 24576;   // kDecodeStateBytes, kQDecodeStateBytes, kQTab
constexpr int kIndexMaxSide = 65535;                                                 // NBLIC_MAX_HEIGHT / _WIDTH, and QNBLIC's

// The body of one entry: the decoder's state record, B (efforts 2 / 3: 512 / 1024 bytes per column), the two rows above
// the entry row, the QNBLIC tables.  0 = kind / effort out of range.
inline size_t index_record_bytes(int kind, int w, int effort) {
    if (kind == 0 && effort >= 1 && effort <= 3) return kNblicRecordBytes + 2 * size_t(w) + (effort == 3 ? 1024 : effort == 2 ? 512 : 0) * size_t(w);
    if (kind == 1 && effort == 0) return kQnblicRecordBytes + 2 * size_t(w) + kQnblicTableBytes;
    return 0;
}
// One sealed entry: checkpoint head, body, SHA-256.
inline size_t index_entry_bytes(int kind, int w, int effort) { return kCheckpointHeadBytes + index_record_bytes(kind, w, effort) + 32; }
// Layout of an index: head | count x (uint64 length | entry) | SHA-256.
inline size_t index_entry_at(int k, size_t entry_bytes) { return kIndexHeadBytes + size_t(k) * (8 + entry_bytes) + 8; }   // entry k, 0-based (its length sits in the 8 bytes before)
inline size_t index_total_bytes(int count, size_t entry_bytes) { return kIndexHeadBytes + size_t(count) * (8 + entry_bytes) + 32; }

// nblic_amd_index_bytes: the one place that knows the size of an index.
inline long index_bytes(int kind, int h, int w, int effort, int every_rows) {
    if (h < 1 || w < 1 || h > kIndexMaxSide || w > kIndexMaxSide || every_rows < 1 || every_rows >= h) return -1;
    if (index_record_bytes(kind, w, effort) == 0) return -1;
    return long(index_total_bytes((h - 1) / every_rows, index_entry_bytes(kind, w, effort)));
}

// ---- where the entries are: the one statement of the rule every index writer follows -------------------------------------
// An entry stands in front of row r when r is a multiple of R and r < h, and an encoder's band never crosses such a row.
// The next band of an image that has coded rows [0, row0) (row0 < h), `band` rows at most; every < 1: no index, no cut.
struct BandCut { int rows; bool entry; };                                // entry: an entry is written behind this band
inline BandCut index_band_cut(int row0, int band, int h, int every) {
    int rows = band < h - row0 ? band : h - row0;
    if (every < 1) return BandCut{rows, false};
    const int to_entry = every - row0 % every;                           // rows up to the next multiple of R
    if (to_entry < rows) rows = to_entry;
    return BandCut{rows, rows == to_entry && row0 + rows < h};
}
// Whether an image whose caller offers `cap` bytes for an index every R rows gets one: every = 0 when none is possible
// (R < 1 or R >= h; index_bytes refuses the same), too_small when there is one and it does not fit (or the codec has none).
struct IndexAdmission { int every, count; size_t entry_bytes; bool too_small; };
inline IndexAdmission index_admit(int kind, int effort, int h, int w, int every_rows, size_t cap) {
    if (every_rows < 1 || every_rows >= h) return IndexAdmission{0, 0, 0, false};
    const long need = index_bytes(kind, h, w, effort, every_rows);
    if (need < 0 || cap < size_t(need)) return IndexAdmission{0, 0, 0, true};
    return IndexAdmission{every_rows, (h - 1) / every_rows, index_entry_bytes(kind, w, effort), false};
}

// Head and entry lengths around `count` entries that already sit at index_entry_at(k), then the seal.
inline void index_close(uint8_t *p, const void *head, int count, size_t entry_bytes) {
    memcpy(p, head, kIndexHeadBytes);
    const unsigned long long n = entry_bytes;
    for (int k = 0; k < count; k++) memcpy(p + index_entry_at(k, entry_bytes) - 8, &n, 8);
    seal(p, index_total_bytes(count, entry_bytes));
}

// ---- the job list of an indexed batch decode (nblic_amd_indexed_decode_plan; pipeline.hip decode_batch_indexed) ----------
// Image k of a call wants rows [row0, row1) of an h-row image whose index has an entry every R rows: its segments
// row0 / R .. (row1 - 1) / R all run, each from its entry (segment 0 from the stream's start), the last one stopping in
// front of row1.  The segments of all images form ONE list, cut into rounds of at most `cap` segments (cap <= 0: one
// round).  Two rules fix the order.  Images are taken class by class (cls = kind * 4 + effort, what one launch can
// carry), so a round's jobs of one class are neighbours and share a launch.  Within an image the segments are listed from
// the last to the first: the rows above a segment come from its entry and lie in the plane BEFORE the segment that owns
// them decodes, so a higher segment must never run in a later round than a lower one.
struct IndexedJob { int image, segment, first_row, end_row, cls, round; };   // end_row 0: the job runs to the image's last row
struct IndexedPlanImage { int kind, effort, h, w, every, row0, row1; };
inline int indexed_class(int kind, int effort) { return kind * 4 + effort; }
// false: an image whose fields are out of range (nothing is appended then).
inline bool indexed_decode_plan(const IndexedPlanImage *im, int n, int cap, std::vector<IndexedJob> &jobs) {
    jobs.clear();
    if (n < 1 || !im) return false;
    std::vector<int> order;
    for (int k = 0; k < n; k++) {
        const IndexedPlanImage &I = im[k];
        if (index_record_bytes(I.kind, I.w, I.effort) == 0 || I.h < 1 || I.w < 1 || I.h > kIndexMaxSide || I.w > kIndexMaxSide || I.every < 1 ||
            I.row0 < 0 || I.row1 <= I.row0 || I.row1 > I.h) return false;
        order.push_back(k);
    }
    for (int a = 1; a < n; a++)                                          // stable, by class
        for (int b = a; b > 0 && indexed_class(im[order[size_t(b)]].kind, im[order[size_t(b)]].effort) <
                                     indexed_class(im[order[size_t(b - 1)]].kind, im[order[size_t(b - 1)]].effort); b--) {
            const int t = order[size_t(b)]; order[size_t(b)] = order[size_t(b - 1)]; order[size_t(b - 1)] = t;
        }
    for (int k : order) {
        const IndexedPlanImage &I = im[k];
        const int s0 = I.row0 / I.every, s1 = (I.row1 - 1) / I.every;
        for (int s = s1; s >= s0; s--) {
            const int end = s == s1 ? (I.row1 < I.h ? I.row1 : 0) : (s + 1) * I.every;
            const int round = cap > 0 ? int(jobs.size() / size_t(cap)) : 0;
            jobs.push_back(IndexedJob{k, s, s * I.every, end, indexed_class(I.kind, I.effort), round});
        }
    }
    return true;
}

// ---- the launch schedule of a batch index build (nblic_amd_index_build_plan; pipeline.hip index_build_batch) --------------
// Image k of a call is decoded from its first row to its last, `rows` rows per launch at most, and stops in front of every
// entry row R, 2R, ... below h (SerialJob::end_row): a launch advances it by min(rows, next entry row - row), and by
// min(rows, h - row) behind the last entry.  While no stream fails that is all there is to know, so the whole call is laid
// out here before anything runs: the images of a class (indexed_class: what one launch can carry) share its launches, a
// class needs as many as its slowest image, and an entry is captured behind the launch in which its image reaches its row.
// Entries are listed class by class, within a class by that launch, so the entries one capture launch takes are neighbours.
struct BuildPlanImage { int kind, effort, h, w, every, rows; };           // rows: what one launch covers (>= 1)
struct BuildEntry { int image, row, cls, launch; };                       // launch: 0-based, counted within the class
constexpr int kBuildClasses = 8;
struct BuildPlan { int launches[kBuildClasses]; std::vector<BuildEntry> entries; };
// false: an image whose fields are out of range (the plan is empty then).
inline bool index_build_plan(const BuildPlanImage *im, int n, BuildPlan &P) {
    P.entries.clear();
    for (int c = 0; c < kBuildClasses; c++) P.launches[c] = 0;
    if (n < 1 || !im) return false;
    for (int k = 0; k < n; k++) {
        const BuildPlanImage &I = im[k];
        if (index_bytes(I.kind, I.h, I.w, I.effort, I.every) < 0 || I.rows < 1 || indexed_class(I.kind, I.effort) >= kBuildClasses) return false;
    }
    for (int c = 0; c < kBuildClasses; c++) {
        const size_t first = P.entries.size();
        for (int k = 0; k < n; k++) {
            const BuildPlanImage &I = im[k];
            if (indexed_class(I.kind, I.effort) != c) continue;
            const int count = (I.h - 1) / I.every;
            const int per_segment = (I.every + I.rows - 1) / I.rows;                 // launches from one entry row to the next
            const int tail = (I.h - count * I.every + I.rows - 1) / I.rows;          // and from the last one to the end (>= 1)
            for (int e = 1; e <= count; e++) P.entries.push_back(BuildEntry{k, e * I.every, c, e * per_segment - 1});
            const long total = long(count) * per_segment + tail;                     // <= 65534 + 65535
            if (total > P.launches[c]) P.launches[c] = int(total);
        }
        // by launch, stable: images stay in the caller's order within a launch (counting sort over the class's launches)
        std::vector<BuildEntry> part(P.entries.begin() + ptrdiff_t(first), P.entries.end());
        std::vector<size_t> at(size_t(P.launches[c]) + 1, 0);
        for (const BuildEntry &e : part) at[size_t(e.launch) + 1]++;
        for (size_t l = 1; l < at.size(); l++) at[l] += at[l - 1];
        for (const BuildEntry &e : part) P.entries[first + at[size_t(e.launch)]++] = e;
    }
    return true;
}

// ---- entries that wait for their window ----------------------------------------------------------------------------------
struct PendingEntries {
    struct Entry {
        uint8_t *ck; size_t bytes;      // the entry (head | body | room for the seal); the memory is the caller's and stays where it is
        size_t window_at;               // where its 32-bit window goes, in bytes from ck
        unsigned long long at;          // the window is stream bytes [at, at + 4)
        int got; uint32_t window;
    };
    std::vector<Entry> waiting;         // in row order
    unsigned long long fed = 0;         // stream bytes handed to the waiting entries so far
    int sealed = 0;

    void add(uint8_t *ck, size_t bytes, size_t window_at, unsigned long long at) { waiting.push_back(Entry{ck, bytes, window_at, at, 0, 0u}); }

    // Stream bytes [base, base + (end - out)) have been emitted and lie at [out, end).  Bytes handed over before are skipped.
    void bytes(unsigned long long base, const uint8_t *out, const uint8_t *end) {
        const unsigned long long stop = base + (unsigned long long)(end - out);
        for (unsigned long long a = fed > base ? fed : base; a < stop && !waiting.empty(); a++)
            for (auto &e : waiting)
                if (a >= e.at && a < e.at + 4) { e.window = (e.window << 8) | out[a - base]; e.got++; }
        fed = fed > stop ? fed : stop;
        while (!waiting.empty() && waiting.front().got == 4) {
            const Entry &e = waiting.front();
            memcpy(e.ck + e.window_at, &e.window, 4);
            seal(e.ck, e.bytes);
            waiting.erase(waiting.begin());
            sealed++;
        }
    }
};

}  // namespace nblic
