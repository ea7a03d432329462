// copy_engine.h -- "copy device memory to the host on a DMA engine and tell me when it is done", and the chunk ring of
// the coder threads that uses it.  Host-only C++: no HIP type appears here, so tools/copy_engine_check.cpp can drive all
// of it with a fake engine.
//
// Why: the HIP runtime this library runs under performs every chunk copy of code_packs with a blit KERNEL, which holds a
// compute hardware queue for the ~1 ms the PCIe transfer takes; the group kernels that share the queue wait behind it
// (DESIGN.md section 4).  A copy on an SDMA engine occupies no compute queue.  No HIP call of that runtime asks for one,
// but the HSA runtime underneath is loaded in the process, and hsa_amd_memory_async_copy is what the HIP runtime itself
// calls when it does use SDMA.  So: find the loaded libhsa-runtime64 (no new link dependency), resolve eight entry
// points, and issue the chunk copies there.  Anything missing, and any error later, leaves the library on hipMemcpyAsync
// exactly as before.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <type_traits>

#include <dlfcn.h>
#include <link.h>

namespace nblic {

// hsa_amd_pointer_info_t as far as agentOwner.  The runtime fills as many bytes as `size` announces (the structure only
// grows within a major version), so the short form is what every version has.
struct HsaPointerInfo {
    uint32_t size; uint32_t type;                                    // type 1: allocated by the runtime (device memory, hipHostMalloc)
    void *agent_base; void *host_base; size_t bytes; void *user;
    uint64_t owner;                                                  // hsa_agent_t of the pool's owner
};

// The entry points, as a table so that a test can substitute a fake.  Handles (hsa_agent_t, hsa_signal_t) are structs of
// one uint64_t, passed like one; hsa_status_t is an int, 0 = success; hsa_signal_value_t is int64_t.
struct HsaApi {
    int (*init)() = nullptr;
    int (*shut_down)() = nullptr;
    int (*pointer_info)(const void *p, HsaPointerInfo *info, void *(*alloc)(size_t), uint32_t *n_accessible, void **accessible) = nullptr;
    int (*async_copy)(void *dst, uint64_t dst_agent, const void *src, uint64_t src_agent, size_t bytes, uint32_t n_deps, const uint64_t *deps, uint64_t done) = nullptr;
    int (*signal_create)(int64_t initial, uint32_t n_consumers, const uint64_t *consumers, uint64_t *signal) = nullptr;
    int (*signal_destroy)(uint64_t signal) = nullptr;
    void (*signal_store)(uint64_t signal, int64_t value) = nullptr;  // hsa_signal_store_relaxed
    int64_t (*signal_load)(uint64_t signal) = nullptr;               // hsa_signal_load_scacquire
    bool complete() const { return init && shut_down && pointer_info && async_copy && signal_create && signal_destroy && signal_store && signal_load; }
};

// Fills `api` from the object already loaded in this process whose name contains `needle`; returns the dlopen handle
// (RTLD_NOLOAD: a reference to the loaded object, never a second copy) or null with `api` incomplete.
inline void *hsa_api_load(HsaApi &api, const char *needle = "libhsa-runtime64") {
    struct Find { const char *needle; char path[4096]; } f{needle, {0}};
    dl_iterate_phdr([](dl_phdr_info *info, size_t, void *vp) -> int {
        Find *q = static_cast<Find *>(vp);
        if (!info->dlpi_name || !strstr(info->dlpi_name, q->needle) || strlen(info->dlpi_name) >= sizeof q->path) return 0;
        strcpy(q->path, info->dlpi_name);
        return 1;
    }, &f);
    if (!f.path[0]) return nullptr;
    void *h = dlopen(f.path, RTLD_NOW | RTLD_NOLOAD);
    if (!h) return nullptr;
    auto get = [&](auto &fn, const char *name) { fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name)); };
    get(api.init, "hsa_init"); get(api.shut_down, "hsa_shut_down");
    get(api.pointer_info, "hsa_amd_pointer_info"); get(api.async_copy, "hsa_amd_memory_async_copy");
    get(api.signal_create, "hsa_signal_create"); get(api.signal_destroy, "hsa_signal_destroy");
    get(api.signal_store, "hsa_signal_store_relaxed"); get(api.signal_load, "hsa_signal_load_scacquire");
    if (!api.complete()) { dlclose(h); api = HsaApi{}; return nullptr; }
    return h;
}

// One context's engine: the table, whether it may be used, and what happened.  Threads share it; the counters are atomic
// and `failed` is sticky: after the first HSA error every later chunk of the context goes through the runtime.
class CopyEngine {
    HsaApi api_{};
    void *lib_ = nullptr;
    bool up_ = false;                                                // our hsa_init is outstanding
    std::atomic<bool> failed_{false};
    std::atomic<long> engine_chunks_{0}, runtime_chunks_{0}, fallbacks_{0};
public:
    CopyEngine() = default;
    CopyEngine(const CopyEngine &) = delete;
    CopyEngine &operator=(const CopyEngine &) = delete;
    ~CopyEngine() { close(); }
    // The loaded HSA runtime, holding it up with an hsa_init of our own until close().  false: not there (nothing is logged:
    // a process without it is an ordinary case).
    bool open(const char *needle = "libhsa-runtime64") {
        close();
        lib_ = hsa_api_load(api_, needle);
        if (!lib_) return false;
        return start();
    }
    bool open_with(const HsaApi &api) {                              // a table from somewhere else (tests)
        close();
        api_ = api;
        if (!api_.complete()) { api_ = HsaApi{}; return false; }
        return start();
    }
    void close() {
        if (up_) api_.shut_down();
        if (lib_) dlclose(lib_);
        up_ = false; lib_ = nullptr; api_ = HsaApi{};
    }
    bool available() const { return up_; }
    bool on() const { return up_ && !failed_.load(std::memory_order_relaxed); }
    const HsaApi &api() const { return api_; }
    // An HSA call failed: no chunk is issued on the engine from now on.  One line, once.
    void fail(const char *what, long status) {
        if (!failed_.exchange(true)) fprintf(stderr, "[nblic_amd] copy engine: %s failed (%ld); chunk copies go through hipMemcpyAsync from here on\n", what, status);
    }
    void count_engine() { engine_chunks_++; }
    void count_runtime() { runtime_chunks_++; }
    void count_fallback() { fallbacks_++; }
    // chunks that arrived by the engine, chunks handed to the runtime, chunks handed to the runtime BECAUSE the engine
    // failed on them (issued in part, or completed with an error), whether the engine is available
    void stats(long out[4]) const { out[0] = engine_chunks_; out[1] = runtime_chunks_; out[2] = fallbacks_; out[3] = up_ ? 1 : 0; }
private:
    bool start() {
        if (api_.init() != 0) { if (lib_) dlclose(lib_); lib_ = nullptr; api_ = HsaApi{}; return false; }
        up_ = true;
        return true;
    }
};

struct CopyPiece { void *dst; const void *src; size_t bytes; };
constexpr int kChunkPieces = 3;                                      // copies per chunk: one per pack (pipeline.hip kMaxPacks)
constexpr int kChunkSlots = 3;                                       // ring slots per coder thread (pipeline.hip kRingDepth)

// The pieces of chunk c of up to three packs: pack p has groups[p] groups of group_words 64-bit words in device memory at
// rows[p]; a chunk is chunk_groups groups of every pack that still has some; slot(c, p) is where the piece lands.
template <class SlotOf>
inline int chunk_pieces(size_t c, int n_packs, const size_t *groups, size_t chunk_groups, size_t group_words, const uint64_t *const *rows,
                        SlotOf slot, CopyPiece *out) {
    int n = 0;
    for (int p = 0; p < n_packs; p++) {
        const size_t g0 = c * chunk_groups;
        if (g0 >= groups[p]) continue;
        const size_t words = (chunk_groups < groups[p] - g0 ? chunk_groups : groups[p] - g0) * group_words;
        out[n++] = CopyPiece{slot(c, p), rows[p] + g0 * group_words, words * sizeof(uint64_t)};
    }
    return n;
}

// One coder thread's side of the engine: a completion signal per ring slot (views: the thread owns them, hip_owned.h
// HsaSignal), who carries the chunk that is in each slot, and the two agents, looked up once.
struct EngineLane {
    uint64_t sig[kChunkSlots] = {0, 0, 0};
    bool by_engine[kChunkSlots] = {false, false, false};             // the slot's chunk was issued on the engine and has not been seen complete
    uint64_t src_agent = 0, dst_agent = 0;
    const char *src_base = nullptr, *dst_base = nullptr;             // the allocations the agents were read from
    size_t src_bytes = 0, dst_bytes = 0;
    bool ready() const { return sig[0] && sig[1] && sig[2]; }
};

namespace copy_detail {
constexpr auto kPoll = std::chrono::microseconds(100);               // a sleeping poll, as wait_chunk's: CPU seconds are what the rank is short of
constexpr double kStallSeconds = 20.0;                               // a chunk is a few ms on the link

inline bool inside(const void *p, size_t n, const char *base, size_t bytes) {
    const char *q = static_cast<const char *>(p);
    return base && q >= base && n <= bytes && size_t(q - base) <= bytes - n;
}
// The agent that owns the runtime allocation p lies in.  Memory the runtime did not allocate itself (registered pages,
// plain pages) is refused: the ring is runtime memory whenever the engine is on.
inline bool owner_of(CopyEngine &e, const void *p, size_t n, uint64_t *agent, const char **base, size_t *bytes) {
    HsaPointerInfo info{};
    info.size = sizeof info;
    const int st = e.api().pointer_info(p, &info, nullptr, nullptr, nullptr);
    if (st != 0) { e.fail("hsa_amd_pointer_info", st); return false; }
    if (info.type != 1 || !info.owner) { e.fail("hsa_amd_pointer_info (not the runtime's memory)", long(info.type)); return false; }
    *agent = info.owner; *base = static_cast<const char *>(info.host_base ? info.host_base : info.agent_base); *bytes = info.bytes;
    if (!inside(p, n, *base, *bytes)) { e.fail("hsa_amd_pointer_info (piece outside its allocation)", 0); return false; }
    return true;
}
// Sleeps until the slot's signal is at or below `until`; false: it went negative (the engine reports an error) or did
// not move for kStallSeconds.
inline bool wait_signal(CopyEngine &e, uint64_t sig, int64_t until, double *wait_s) {
    const auto w0 = std::chrono::steady_clock::now();
    bool ok = true;
    for (;;) {
        const int64_t v = e.api().signal_load(sig);
        if (v < 0) { e.fail("a chunk copy (completion signal)", long(v)); ok = false; break; }
        if (v <= until) break;
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() > kStallSeconds) { e.fail("a chunk copy (no completion)", long(v)); ok = false; break; }
        std::this_thread::sleep_for(kPoll);
    }
    if (wait_s) *wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    return ok;
}
// All n pieces of a chunk on the engine, the slot's signal counting them down, no dependency signals.  false: an HSA
// call failed; the engine is marked, and whatever part of the chunk was issued has been waited for, so the caller can
// issue the WHOLE chunk again through the runtime into the same slot.
inline bool engine_issue(CopyEngine &e, EngineLane &l, int slot, const CopyPiece *pc, int n) {
    for (int k = 0; k < n; k++) {
        if (!inside(pc[k].src, pc[k].bytes, l.src_base, l.src_bytes) && !owner_of(e, pc[k].src, pc[k].bytes, &l.src_agent, &l.src_base, &l.src_bytes)) return false;
        if (!inside(pc[k].dst, pc[k].bytes, l.dst_base, l.dst_bytes) && !owner_of(e, pc[k].dst, pc[k].bytes, &l.dst_agent, &l.dst_base, &l.dst_bytes)) return false;
    }
    e.api().signal_store(l.sig[slot], n);
    for (int k = 0; k < n; k++) {                                    // (the packs of a take sit in allocations of their own, all of the one device: one source agent)
        const int st = e.api().async_copy(pc[k].dst, l.dst_agent, pc[k].src, l.src_agent, pc[k].bytes, 0, nullptr, l.sig[slot]);
        if (st != 0) {
            e.fail("hsa_amd_memory_async_copy", st);
            wait_signal(e, l.sig[slot], n - k, nullptr);              // the k copies that were issued
            return false;
        }
    }
    l.by_engine[slot] = true;
    return true;
}
}  // namespace copy_detail

// Waits (bounded) for every chunk still on the engine: before a ring or a signal is released on an error path.
inline void engine_drain(CopyEngine *e, EngineLane &l) {
    for (int s = 0; s < kChunkSlots; s++) {
        if (e && l.by_engine[s]) copy_detail::wait_signal(*e, l.sig[s], 0, nullptr);
        l.by_engine[s] = false;
    }
}

// The chunk ring of code_packs: chunks 0 .. chunks-1 travel through kChunkSlots slots, chunk c+2 being issued before
// chunk c is consumed.  pieces(c, out) -> n names a chunk's copies; consume(c) reads slot c % kChunkSlots.  A chunk goes
// on the engine while it is on, and through `rt` otherwise:
//   rt.issue(c, pieces, n)   queue the copies and whatever marks their completion (hipMemcpyAsync + an event record)
//   rt.wait(c)               sleep until that mark is reached
// An engine error at issue or at completion hands the whole chunk to rt, into the same slot, before it is consumed.
// e == nullptr: everything through rt.  issue_s / wait_s: time spent queueing / waiting (reporting; may be null).
template <class Runtime, class Pieces, class Consume>
inline bool run_chunk_ring(CopyEngine *e, EngineLane &l, size_t chunks, Runtime &rt, Pieces pieces, Consume consume, double *issue_s, double *wait_s) {
    auto to_runtime = [&](size_t c, const CopyPiece *pc, int n) -> bool {
        if (!rt.issue(c, pc, n)) return false;
        if (e && n > 0) e->count_runtime();
        return true;
    };
    auto issue = [&](size_t c) -> bool {
        CopyPiece pc[kChunkPieces];
        const int n = pieces(c, pc), slot = int(c % size_t(kChunkSlots));
        l.by_engine[slot] = false;
        if (e && n > 0 && e->on() && l.ready()) {
            if (copy_detail::engine_issue(*e, l, slot, pc, n)) return true;
            e->count_fallback();
        }
        return to_runtime(c, pc, n);
    };
    auto wait = [&](size_t c) -> bool {
        const int slot = int(c % size_t(kChunkSlots));
        if (l.by_engine[slot]) {
            const bool ok = copy_detail::wait_signal(*e, l.sig[slot], 0, wait_s);
            l.by_engine[slot] = false;
            if (ok) { e->count_engine(); return true; }
            e->count_fallback();
            CopyPiece pc[kChunkPieces];
            const int n = pieces(c, pc);
            if (!to_runtime(c, pc, n)) return false;
        }
        return rt.wait(c);
    };
    auto run = [&]() -> bool {
        for (size_t c = 0; c + 1 < size_t(kChunkSlots) && c < chunks; c++) if (!issue(c)) return false;
        for (size_t c = 0; c < chunks; c++) {
            const auto i0 = std::chrono::steady_clock::now();
            if (c + kChunkSlots - 1 < chunks && !issue(c + kChunkSlots - 1)) return false;      // its ring slot was consumed one chunk ago
            if (issue_s) *issue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - i0).count();
            if (!wait(c)) return false;
            consume(c);
        }
        return true;
    };
    const bool ok = run();
    if (!ok) engine_drain(e, l);
    return ok;
}

}  // namespace nblic
