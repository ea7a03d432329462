// copy_engine_check.cpp -- csrc/copy_engine.h alone, with its own main, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -o copy_engine_check tools/copy_engine_check.cpp -ldl
// The chunk ring of code_packs (run_chunk_ring, chunk_pieces) is driven through the function table with a FAKE engine:
// copies are done by a worker thread with memcpy, some time after they were issued; signals are atomics.  The "runtime"
// side is a fake too (its copies happen when the chunk is waited for).  Swept: 1-3 packs, 1-9 chunks (the ring wraps at
// three), lanes of unequal length -- among them lanes and whole packs with nothing in the last chunks -- and, for every
// shape, an error injected at every status-returning call in turn (as a status, and for the copies also as a completion
// signal that goes negative).  In every case each lane's words reach the consumer exactly as they lie in the source,
// and the counters say who carried which chunk.  Also: the library that is not there.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <vector>

#include "../nblic-image-compression_amd/csrc/copy_engine.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "copy_engine_check: %s failed (line %d)\n", #x, __LINE__); exit(1); } } while (0)

namespace {

constexpr uint64_t kGpu = 0x1111, kHost = 0x2222;
constexpr size_t kGroupWords = 13 * 8, kGroupBins = 64, kLanes = 8;

struct Range { const char *base; size_t bytes; uint64_t owner; };
struct Job { void *dst; const void *src; size_t bytes; std::atomic<int64_t> *sig; bool bad; };

// ---- the fake HSA runtime (one at a time: the table holds plain functions) ----------------------------------------------
struct Fake {
    std::vector<Range> ranges;
    long calls = 0, fail_at = -1;                                    // status-returning calls so far; which of them fails
    bool bad_completion = false;                                     // a failing COPY returns success and its chunk's signal ends negative
    long failed_call = -1; const char *failed_what = "";
    size_t issuing = 0, failed_chunk = 0;                            // the chunk whose pieces are being issued (set by the test's pieces())
    long inits = 0, shut_downs = 0, created = 0, destroyed = 0, copies = 0, copies_after_failure = 0;
    bool wrong_agent = false;
    std::mutex m; std::condition_variable cv; std::deque<Job> q; bool stop = false;
    std::thread worker;
    void start() {
        worker = std::thread([this] {
            for (;;) {
                Job j;
                {
                    std::unique_lock<std::mutex> l(m);
                    cv.wait(l, [this] { return stop || !q.empty(); });
                    if (q.empty()) return;
                    j = q.front(); q.pop_front();
                }
                std::this_thread::sleep_for(std::chrono::microseconds(30));
                if (!j.bad) memcpy(j.dst, j.src, j.bytes);
                if (j.bad) bad_sig = j.sig;                          // (this thread alone counts a signal down: it was set before its copies were queued)
                const int64_t left = j.sig->load() - 1;
                j.sig->store(left == 0 && bad_sig == j.sig ? -1 : left);      // the chunk's last copy reports the error, HSA's way: a negative value
                if (left == 0 && bad_sig == j.sig) bad_sig = nullptr;
            }
        });
    }
    std::atomic<int64_t> *bad_sig = nullptr;                         // the signal whose chunk must end in an error (worker thread only)
    void finish() {
        { std::lock_guard<std::mutex> l(m); stop = true; }
        cv.notify_all();
        if (worker.joinable()) worker.join();
    }
    bool fails(const char *what) {
        const bool f = calls++ == fail_at;
        if (f) { failed_call = calls - 1; failed_what = what; failed_chunk = issuing; }
        return f;
    }
};
Fake *F = nullptr;

int f_init() { if (F->fails("init")) return 4096; F->inits++; return 0; }
int f_shut_down() { F->shut_downs++; return 0; }
int f_pointer_info(const void *p, HsaPointerInfo *info, void *(*)(size_t), uint32_t *, void **) {
    CHECK(info->size == sizeof(HsaPointerInfo));
    if (F->fails("pointer_info")) return 4097;
    info->type = 0;
    for (const Range &r : F->ranges)
        if (static_cast<const char *>(p) >= r.base && static_cast<const char *>(p) < r.base + r.bytes) {
            info->type = 1; info->agent_base = info->host_base = const_cast<char *>(r.base); info->bytes = r.bytes; info->owner = r.owner;
        }
    return 0;
}
int f_async_copy(void *dst, uint64_t dst_agent, const void *src, uint64_t src_agent, size_t bytes, uint32_t n_deps, const uint64_t *, uint64_t done) {
    CHECK(n_deps == 0);
    if (F->failed_call >= 0) F->copies_after_failure++;
    const bool f = F->fails("async_copy");
    if (f && !F->bad_completion) return 4098;
    if (dst_agent != kHost || src_agent != kGpu) F->wrong_agent = true;
    F->copies++;
    { std::lock_guard<std::mutex> l(F->m); F->q.push_back(Job{dst, src, bytes, reinterpret_cast<std::atomic<int64_t> *>(done), f}); }
    F->cv.notify_all();
    return 0;
}
int f_signal_create(int64_t initial, uint32_t, const uint64_t *, uint64_t *out) {
    if (F->fails("signal_create")) return 4099;
    *out = reinterpret_cast<uint64_t>(new std::atomic<int64_t>(initial));
    F->created++;
    return 0;
}
int f_signal_destroy(uint64_t s) { delete reinterpret_cast<std::atomic<int64_t> *>(s); F->destroyed++; return 0; }
void f_signal_store(uint64_t s, int64_t v) { reinterpret_cast<std::atomic<int64_t> *>(s)->store(v); }
int64_t f_signal_load(uint64_t s) { return reinterpret_cast<std::atomic<int64_t> *>(s)->load(); }

HsaApi fake_api() {
    HsaApi a;
    a.init = f_init; a.shut_down = f_shut_down; a.pointer_info = f_pointer_info; a.async_copy = f_async_copy;
    a.signal_create = f_signal_create; a.signal_destroy = f_signal_destroy; a.signal_store = f_signal_store; a.signal_load = f_signal_load;
    return a;
}

// ---- the fake runtime: a chunk's copies happen when it is waited for ---------------------------------------------------------
struct FakeRuntime {
    std::vector<CopyPiece> pending[kChunkSlots];
    long issued = 0;
    bool issue(size_t c, const CopyPiece *pc, int n) { pending[c % kChunkSlots].assign(pc, pc + n); issued++; return true; }
    bool wait(size_t c) {
        for (const CopyPiece &p : pending[c % kChunkSlots]) memcpy(p.dst, p.src, p.bytes);
        pending[c % kChunkSlots].clear();
        return true;
    }
};

// ---- one take of code_packs ---------------------------------------------------------------------------------------------
struct Shape { int n_packs; size_t chunk_groups; size_t bins[kChunkPieces][kLanes]; };

// Lanes of unequal length whose longest spans exactly `chunks` chunks; variant picks where the others end.
Shape make_shape(int n_packs, size_t chunks, int variant) {
    Shape s{};
    s.n_packs = n_packs; s.chunk_groups = 4;
    const size_t longest = ((chunks - 1) * s.chunk_groups + 1 + size_t(variant)) * kGroupBins - (variant == 1 ? 17 : 0);     // 1, 2 or 3 groups into the last chunk
    for (int p = 0; p < n_packs; p++)
        for (size_t k = 0; k < kLanes; k++) {
            size_t n = longest;
            if (p > 0 || k > 0) n = longest * ((7 * size_t(p) + 3 * k + size_t(variant)) % 11) / 11 + (k == 3 ? 1 : 0);      // from nothing at all to almost everything
            if (p == n_packs - 1 && p > 0 && variant == 2) n = n * (chunks > 1 ? chunks - 1 : 1) / (2 * chunks);                // a whole pack that ends chunks early
            if (p > 0 && k >= 5 + size_t(variant)) n = 0;                                                                      // packs of fewer than eight images
            s.bins[p][k] = n;
        }
    return s;
}

struct Expect { long engine, runtime, fallbacks; };

// Runs one take.  e == nullptr: no engine object at all.  Returns the status-returning calls the fake saw.
long run_take(const Shape &s, CopyEngine *e, Fake *fake, Expect *got) {
    size_t groups[kChunkPieces] = {0}, most = 0;
    for (int p = 0; p < s.n_packs; p++) {
        for (size_t k = 0; k < kLanes; k++) groups[p] = std::max(groups[p], (s.bins[p][k] + kGroupBins - 1) / kGroupBins);
        most = std::max(most, groups[p]);
    }
    const size_t chunks = (most + s.chunk_groups - 1) / s.chunk_groups, chunk = s.chunk_groups * kGroupBins;
    const size_t pack_words = s.chunk_groups * kGroupWords;
    std::vector<uint64_t> src[kChunkPieces];
    const uint64_t *rows[kChunkPieces] = {nullptr};
    for (int p = 0; p < s.n_packs; p++) {
        src[p].resize(std::max<size_t>(groups[p], 1) * kGroupWords);
        for (size_t i = 0; i < src[p].size(); i++) src[p][i] = (uint64_t(p + 1) << 56) ^ (i * 0x9E3779B97F4A7C15ull);
        rows[p] = src[p].data();
    }
    std::vector<uint64_t> ring(size_t(kChunkSlots) * kChunkPieces * pack_words, 0xEEEEEEEEEEEEEEEEull);
    auto slot = [&](size_t c, int p) { return ring.data() + (size_t(c % kChunkSlots) * kChunkPieces + size_t(p)) * pack_words; };
    if (fake) {
        fake->ranges.clear();
        for (int p = 0; p < s.n_packs; p++) fake->ranges.push_back(Range{reinterpret_cast<const char *>(src[p].data()), src[p].size() * 8, kGpu});
        fake->ranges.push_back(Range{reinterpret_cast<const char *>(ring.data()), ring.size() * 8, kHost});
    }
    EngineLane lane;
    uint64_t sigs[kChunkSlots] = {0};
    if (e && e->on())
        for (int k = 0; k < kChunkSlots; k++) {
            if (e->api().signal_create(0, 0, nullptr, &sigs[k]) != 0) { e->fail("hsa_signal_create", -1); break; }
            lane.sig[k] = sigs[k];
        }
    std::vector<uint64_t> out[kChunkPieces][kLanes];
    FakeRuntime rt;
    auto pieces = [&](size_t c, CopyPiece *pc) { if (fake) fake->issuing = c; return chunk_pieces(c, s.n_packs, groups, s.chunk_groups, kGroupWords, rows, slot, pc); };
    size_t consumed = 0;
    auto consume = [&](size_t c) {
        CHECK(c == consumed++);
        for (int p = 0; p < s.n_packs; p++) {
            const uint64_t *r = slot(c, p);
            for (size_t k = 0; k < kLanes; k++) {
                const size_t all = s.bins[p][k], off = c * chunk, len = off >= all ? 0 : std::min(chunk, all - off);
                for (size_t g = 0; g < (len + kGroupBins - 1) / kGroupBins; g++)
                    for (size_t j = 0; j < 13; j++) out[p][k].push_back(r[(13 * g + j) * kLanes + k]);
            }
            std::fill(slot(c, p), slot(c, p) + pack_words, 0xEEEEEEEEEEEEEEEEull);      // what is consumed is gone: a chunk read twice or too early shows
        }
    };
    double issue_s = 0, wait_s = 0;
    CHECK(run_chunk_ring(e, lane, chunks, rt, pieces, consume, &issue_s, &wait_s));
    CHECK(consumed == chunks);
    for (int k = 0; k < kChunkSlots; k++) CHECK(!lane.by_engine[k]);
    for (int p = 0; p < s.n_packs; p++)
        for (size_t k = 0; k < kLanes; k++) {
            std::vector<uint64_t> want;
            for (size_t g = 0; g < (s.bins[p][k] + kGroupBins - 1) / kGroupBins; g++)
                for (size_t j = 0; j < 13; j++) want.push_back(src[p][(13 * g + j) * kLanes + k]);
            CHECK(out[p][k] == want);
        }
    for (uint64_t h : sigs) if (h) e->api().signal_destroy(h);
    long st[4] = {0, 0, 0, 0};
    if (e) e->stats(st);
    *got = Expect{st[0], st[1], st[2]};
    CHECK(!e || st[0] + st[1] == long(chunks));                      // every chunk was carried by somebody, once
    CHECK(!e || rt.issued == st[1]);
    CHECK(e || rt.issued == long(chunks));
    return fake ? fake->calls : 0;
}

long run_with_fake(const Shape &s, long fail_at, bool bad_completion, Expect *got, Fake *report) {
    Fake fake;
    fake.fail_at = fail_at; fake.bad_completion = bad_completion;
    F = &fake;
    fake.start();
    long calls;
    {
        CopyEngine e;
        const bool opened = e.open_with(fake_api());
        CHECK(opened == !(fail_at == 0));                            // call 0 is hsa_init
        calls = run_take(s, &e, &fake, got);
        long st[4]; e.stats(st);
        CHECK(st[3] == (opened ? 1 : 0));
    }
    fake.finish();
    CHECK(fake.inits == fake.shut_downs && fake.created == fake.destroyed && !fake.wrong_agent && fake.q.empty());
    CHECK(fake.copies_after_failure == 0 || bad_completion);         // sticky: after an error status nothing more is issued on the engine
    report->failed_call = fake.failed_call; report->failed_what = fake.failed_what; report->failed_chunk = fake.failed_chunk; report->copies = fake.copies;
    F = nullptr;
    return calls;
}

}  // namespace

int main() {
    long takes = 0, injections = 0;
    for (int n_packs = 1; n_packs <= kChunkPieces; n_packs++)
        for (size_t chunks = 1; chunks <= 9; chunks++)
            for (int variant = 0; variant < 3; variant++) {
                const Shape s = make_shape(n_packs, chunks, variant);
                Expect got{}; Fake rep;
                // no engine object, and an engine whose library is not there: everything through the runtime
                run_take(s, nullptr, nullptr, &got);
                {
                    CopyEngine none;
                    CHECK(!none.open("libno-such-hsa-runtime") && !none.available() && !none.on());
                    run_take(s, &none, nullptr, &got);
                    CHECK(got.engine == 0 && got.runtime == long(chunks) && got.fallbacks == 0);
                }
                // the engine, no error
                const long calls = run_with_fake(s, -1, false, &got, &rep);
                CHECK(got.engine == long(chunks) && got.runtime == 0 && got.fallbacks == 0 && rep.failed_call == -1);
                CHECK(calls >= 1 + kChunkSlots + 2 + long(chunks));   // init, three signals, two agents, a copy per chunk at the least
                takes += 3;
                // an error at every call in turn
                for (long at = 0; at < calls; at++)
                    for (int bad = 0; bad < 2; bad++) {
                        run_with_fake(s, at, bad != 0, &got, &rep);
                        CHECK(rep.failed_call == at);
                        const bool copy = !strcmp(rep.failed_what, "async_copy");
                        const long c = long(rep.failed_chunk);
                        Expect want{};
                        const bool lookup = !strcmp(rep.failed_what, "pointer_info");
                        if (!copy && !lookup) want = Expect{0, long(chunks), 0};                                       // init, signal_create: the engine was never on
                        else if (!bad || lookup) want = Expect{c, long(chunks) - c, 1};                                // the chunks in flight arrive; chunk c and all after it: the runtime
                        else { const long e = c + std::min<long>(kChunkSlots - 1, long(chunks) - 1 - c); want = Expect{e, long(chunks) - e, 1}; }   // seen when c is waited for: the next two are on the engine already
                        if (got.engine != want.engine || got.runtime != want.runtime || got.fallbacks != want.fallbacks) {
                            fprintf(stderr, "packs %d chunks %zu variant %d, %s fails at call %ld (%s, chunk %ld): engine/runtime/fallbacks %ld/%ld/%ld, expected %ld/%ld/%ld\n",
                                    n_packs, chunks, variant, rep.failed_what, at, bad ? "completion" : "status", c, got.engine, got.runtime, got.fallbacks, want.engine, want.runtime, want.fallbacks);
                            return 1;
                        }
                        injections++;
                    }
            }
    // the real loader, in a process that has no HSA runtime: not found, nothing resolved
    HsaApi api;
    CHECK(hsa_api_load(api) == nullptr && !api.complete());
    CopyEngine e;
    CHECK(!e.open() && !e.available());
    printf("copy_engine_check ok: %ld takes, %ld injected errors\n", takes, injections);
    return 0;
}
