// hip_owned.h -- move-only owners of the HIP resources the host pipeline holds: device memory, runtime-pinned and
// page-locked host memory, streams, events.  Every acquire and every release of such a resource is in this file, and
// each one counts itself in g_live (nblic_amd_debug_live), so "nothing leaks" can be checked on a card that other
// processes share.  Members are destroyed in reverse order of declaration: an object declares its stream first, so
// its buffers go before the stream does; what has to happen before that (joining threads, synchronising the stream,
// hipSetDevice) stays with the object.  The completion signals of the copy engine (copy_engine.h) are owned here too.
#pragma once
#include <hip/hip_runtime.h>

#include "copy_engine.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include <sys/mman.h>

namespace nblic {

enum Live { kLiveDevice, kLivePinned, kLiveLocked, kLiveSync };      // sync: streams + events + completion signals
inline std::atomic<long> g_live[4];
inline void live_add(Live k, long d) { g_live[k].fetch_add(d, std::memory_order_relaxed); }

// Where a buffer lives: device memory (the library's one hipMalloc and one hipFree), or host memory pinned by the
// runtime (job records and totals the GPU copies to and from).
struct DeviceMem {
    static constexpr Live kind = kLiveDevice;
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { hipFree(p); }
};
struct PinnedMem {
    static constexpr Live kind = kLivePinned;
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { hipHostFree(p); }
};

// One buffer of T and its capacity (in T): they change together or not at all.  Contents are never kept, and the old
// block is released BEFORE the new one is allocated: at this project's sizes the two do not fit side by side.
template <class T, class Mem> class Buf {
    T *p_ = nullptr; size_t cap_ = 0;
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    ~Buf() { reset(); }
    void reset() {
        if (p_) { Mem::put(p_); live_add(Mem::kind, -1); }
        p_ = nullptr; cap_ = 0;
    }
    hipError_t alloc(size_t count) {                                 // exactly count
        reset();
        const hipError_t e = Mem::get((void **)&p_, count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        if (p_) { cap_ = count; live_add(Mem::kind, 1); }
        return e;
    }
    hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : alloc(count); }     // grow-only
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using Pinned = Buf<T, PinnedMem>;

// The rows of one PACK in device memory: the 13-bit groups of up to eight images of a group launch, eight lanes side by
// side, rows[(13 g + j) * 8 + lane] (kernels_e1.h E1Job::pack_rows) -- what k_pack_rows writes and a coder thread copies
// chunk by chunk.  Counted as device memory.  Grow-only; sized in bins of the pack's longest lane.
class PackRows {
    DevBuf<uint64_t> rows_;
public:
    static constexpr size_t kLanes = 8, kWordsPerGroup = 13, kBinsPerGroup = 64;
    static constexpr size_t words(size_t bins) { return (bins + kBinsPerGroup - 1) / kBinsPerGroup * kWordsPerGroup * kLanes; }
    hipError_t reserve_bins(size_t bins) {                           // an eighth of slack: the next pack is rarely much longer
        const size_t need = words(bins ? bins : 1);                  // never null: the kernels read a null pack_rows as "not packed"
        return need <= rows_.capacity() ? hipSuccess : rows_.alloc(need + need / 8 + kWordsPerGroup * kLanes);
    }
    uint64_t *get() const { return rows_.get(); }
    size_t capacity_words() const { return rows_.capacity(); }
};

// Device buffers that die together.  The pool owns; the raw pointers it hands out are views (E1Buffers, the band
// decoder's workspace).
class DevPool {
    std::vector<DevBuf<uint8_t>> blocks_;
public:
    void reset() { blocks_.clear(); }
    // Releases the block behind p (if it is the pool's), allocates count and points p at it (null after a failure).
    template <class T> hipError_t renew(T *&p, size_t count) {
        auto it = std::find_if(blocks_.begin(), blocks_.end(), [&](const DevBuf<uint8_t> &b) { return b.get() == reinterpret_cast<uint8_t *>(p); });
        if (it == blocks_.end()) { blocks_.emplace_back(); it = blocks_.end() - 1; }
        const hipError_t e = it->alloc(count ? count * sizeof(T) : 1);
        p = reinterpret_cast<T *>(it->get());
        return e;
    }
    template <class T> T *make(size_t count) { T *p = nullptr; renew(p, count); return p; }     // null: failed
    size_t bytes() const { size_t n = 0; for (auto &b : blocks_) n += b.capacity(); return n; }
};

// Host memory the coder threads READ at full speed: ordinary pages, first touched by the thread that will read them
// (so they sit on its NUMA node), then page-locked in place.  hipHostMalloc'ed memory reads 14-18 % slower from these
// threads (measured: 1650 vs 1950 Mbins/s through the sixteen-lane coder, tools/pinned_coder_bench.py); it is the
// fall-back when registration is refused, or disabled with NBLIC_AMD_HOSTMALLOC.  Counted in 16-bit words.
class Locked {
    uint16_t *p_ = nullptr; size_t words_ = 0; bool runtime_ = false;      // runtime_: p_ came from hipHostMalloc
public:
    Locked() = default;
    Locked(Locked &&o) noexcept : p_(std::exchange(o.p_, nullptr)), words_(std::exchange(o.words_, 0)), runtime_(o.runtime_) {}
    ~Locked() { reset(); }
    void reset() {
        if (!p_) return;
        if (runtime_) hipHostFree(p_);
        else { hipHostUnregister(p_); free(p_); }
        live_add(kLiveLocked, -1);
        p_ = nullptr; words_ = 0;
    }
    bool alloc(size_t words, bool from_runtime = false) {            // releases what it holds first.  from_runtime: hipHostMalloc at once (a ring the copy engine writes)
        reset();
        const size_t bytes = (words * sizeof(uint16_t) + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
        void *p = from_runtime || getenv("NBLIC_AMD_HOSTMALLOC") ? nullptr : aligned_alloc(size_t(2) << 20, bytes);
        if (p) {
            madvise(p, bytes, MADV_HUGEPAGE);
            memset(p, 0, bytes);
            if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { free(p); p = nullptr; }
        }
        runtime_ = !p;                                               // registration refused (or disabled): the runtime's own pinned memory
        if (!p && hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return false;
        p_ = static_cast<uint16_t *>(p); words_ = words;
        live_add(kLiveLocked, 1);
        return true;
    }
    operator uint16_t *() const { return p_; }
    size_t capacity() const { return words_; }
};

// A stream or an event, created here (and then destroyed here) or lent by somebody who outlives this object.
template <class H, hipError_t (*Create)(H *, unsigned), hipError_t (*Destroy)(H)> class Sync {
    H h_ = nullptr; bool own_ = false;
public:
    Sync() = default;
    Sync(Sync &&o) noexcept : h_(std::exchange(o.h_, nullptr)), own_(std::exchange(o.own_, false)) {}
    Sync &operator=(Sync &&o) noexcept { std::swap(h_, o.h_); std::swap(own_, o.own_); return *this; }
    ~Sync() { if (own_) { Destroy(h_); live_add(kLiveSync, -1); } }
    static Sync lent(H h) { Sync r; r.h_ = h; return r; }
    hipError_t create(unsigned flags) {                              // once, and not over a lent one
        if (h_) return hipErrorInvalidValue;
        const hipError_t e = Create(&h_, flags);
        if (e == hipSuccess) { own_ = true; live_add(kLiveSync, 1); } else h_ = nullptr;
        return e;
    }
    operator H() const { return h_; }
};
using Stream = Sync<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event = Sync<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

// A completion signal of the HSA runtime, created and destroyed through the copy engine's table (which outlives it).
// Counted with the streams and events.
class HsaSignal {
    const HsaApi *api_ = nullptr; uint64_t h_ = 0;
public:
    HsaSignal() = default;
    HsaSignal(HsaSignal &&o) noexcept : api_(std::exchange(o.api_, nullptr)), h_(std::exchange(o.h_, 0)) {}
    HsaSignal &operator=(HsaSignal &&o) noexcept { std::swap(api_, o.api_); std::swap(h_, o.h_); return *this; }
    ~HsaSignal() { if (h_) { api_->signal_destroy(h_); live_add(kLiveSync, -1); } }
    bool create(const HsaApi &api, int64_t initial) {                // once
        if (h_ || api.signal_create(initial, 0, nullptr, &h_) != 0) return false;
        if (!h_) return false;
        api_ = &api; live_add(kLiveSync, 1);
        return true;
    }
    uint64_t handle() const { return h_; }
};

}  // namespace nblic
