// pipeline.hip -- host side of libnblic_amd.so: workspaces, streams, the serial range-coder
// stage (S6) on host threads, and the C ABI declared in include/nblic_amd.h.
//
// Images in flight are split into GROUPS that share every kernel launch (a driver thread and a HIP
// stream per group).  A finished image's coded bins stay in an HBM buffer of a pool -- a pack's rows (13 bits per bin,
// laid out for the AVX-512 lanes inside the group launch: up to eight images of a launch are a pack), or u16 per
// bin for an image on its own -- until a coder thread streams them to the host chunk by chunk through its own pinned ring
// and turns them into the byte-exact range-coder stream (NBLIC.c:552-586), while the GPU is already
// working on the next groups.  The rank's CPU share is what bounds the pipeline, so nothing here spins:
// drivers sleep on a condition variable, coder threads poll for a chunk with 100 us sleeps.  Three kinds of group: staged -n0 -e1 encode, QNBLIC (effort 0) encode,
// and the serial modes (near > 0, efforts 2/3), whose front half is the one-wave-per-image model
// stage of serial_engine.hip and whose entropy stages are the same parallel kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include <pthread.h>
#include <sched.h>
#include <fcntl.h>
#include <unistd.h>

#include "../../include/nblic_amd.h"
#include "device_coder.h"
#include "hip_owned.h"
#include "index_entries.h"
#include "index_pack.h"
#include "kernels_e1.h"
#include "lsq_f64.h"
#include "model.h"
#include "q_device_coder.h"
#include "q_entropy.h"
#include "queue_plan.h"
#include "range_coder.h"
#include "serial_engine.h"
#include "sha256.h"

struct nblic_amd_ctx;

namespace nblic {

#define HIP_OK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "[nblic_amd] %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return false;                                                                     \
        }                                                                                     \
    } while (0)

// NBLIC_AMD_DBG: OR-able measurement aids, read once per process.  Bits 8 and 256 mean something to the
// kernels and travel there in E1Job::dbg (kernels_e1.h); the rest are the host's.
enum DbgFlag : int {
    kDbgDeviceOnly = 16,      // bins are produced but neither copied nor coded: device side alone
    kDbgReport = 32,          // coder / driver accounting on stderr when a batch ends
    kDbgTrace = 64,           // timeline of groups and coder takes on stderr
    kDbgFeedOnly = 128,       // bins reach the host but are not coded
    kDbgNoCopy = 1024,        // (with kDbgFeedOnly) no copy
};
static int dbg_flags() {
    static const int flags = [] { const char *v = getenv("NBLIC_AMD_DBG"); return v ? atoi(v) : 0; }();
    return flags;
}

// ---- S6: 32-bit carry-less binary range coder (NBLIC.c:527-586), encoder side ------------
// (range_coder.h: resumable, because the coder threads stream the bins from HBM in chunks)
void RangeScalar::feed(const uint16_t *coded, size_t n) {
    if (overflow) return;
    uint32_t l = lo, h = hi;
    uint8_t *q = p;
    for (size_t r = 0; r < n; r++) {
        uint32_t e = coded[r];
        uint32_t cut = l + uint32_t((uint64_t(h - l) * (e & 0xFFFu)) >> 12);
        bool one = (e >> 15) != 0;
        h = one ? cut : h;
        l = one ? l : cut + 1;
        while (((l ^ h) >> 24) == 0) {
            if (q == end) { overflow = true; return; }
            *q++ = uint8_t(h >> 24);
            l <<= 8;
            h = (h << 8) | 0xFFu;
        }
    }
    lo = l; hi = h; p = q;
}

size_t RangeScalar::finish() {
    if (overflow) return SIZE_MAX;
    uint32_t l = lo;
    for (int k = 0; k < 4; k++) { *p++ = uint8_t(l >> 24); l <<= 8; }
    return size_t(p - out);
}

// Returns the number of bytes written, or SIZE_MAX if `cap` bytes were not enough.
size_t range_code(const uint16_t *coded, size_t n, uint8_t *out, size_t cap) {
    if (cap < 4) return SIZE_MAX;
    RangeScalar r;
    r.begin(out, cap);
    r.feed(coded, n);
    return r.finish();
}


void write_header(uint8_t *p, int h, int w, int near, int k_step, int effort) {   // NBLIC.c:682-694
    memcpy(p, "NBLIC0.3", 8);
    p[8] = 1;
    p[9] = uint8_t(h >> 8); p[10] = uint8_t(h);
    p[11] = uint8_t(w >> 8); p[12] = uint8_t(w);
    p[13] = uint8_t(near); p[14] = uint8_t(k_step); p[15] = uint8_t(effort);
}

bool size_ok(int h, int w, long max_px) {                                          // NBLIC.c:717-729
    return h > 0 && w > 0 && h <= NBLIC_MAX_HEIGHT && w <= NBLIC_MAX_WIDTH && long(h) * long(w) <= max_px;
}

// ---- an image between the GPU and the coder threads ----------------------------------------
// The backlog lives in HBM: a finished image's coded bins stay in a device buffer until a coder
// thread streams them to the host chunk by chunk (its own small pinned ring), so the pinned host
// memory is per THREAD, not per image, and the GPU never waits for host buffers.
using CodedBuf = DevBuf<uint16_t>;                                 // device; one image's coded bins (QNBLIC: pairs + histograms)
// Bins per lane per chunk of the host ring.  Every chunk costs the GPU a copy per pack (which the runtime
// performs with a blit kernel) that has to find room between the encoder's own kernels: with 1 Mbin
// chunks the coder threads waited for their
// next chunk 15-20 % of the time (4.7 Gpx/s), with 4 Mbin chunks 3 % (5.2 Gpx/s).
constexpr size_t kChunkBins = size_t(1) << 22;
constexpr int kCopyStreams = 8;
constexpr int kRingDepth = 3;                                      // ring slots per coder thread: the chunk being coded + the next two on their way (two slots: 6.14-6.30 Gpx/s, three: 6.35-6.38)
constexpr int kMaxTake = 24;                                       // images one coder thread codes together (three AVX-512 packs; NBLIC_AMD_MAX_TAKE=16: two)
constexpr int kMaxPacks = kMaxTake / int(kPackLanes);
static_assert(kRingDepth == kChunkSlots && kMaxPacks == kChunkPieces, "copy_engine.h carries the ring's shape for its stand-alone check");

}  // namespace nblic
// One submitted batch (nblic_amd_encode_batch_begin .. _end); `remaining` is guarded by ctx->fm.
struct nblic_amd_batch { int remaining = 0; int n_images = 0; long *lens = nullptr; bool ok = true; bool submitted = false; };   // submitted: every image has been handed to a group (guarded by ctx->fm)
namespace nblic {

struct ReadyImage {                                                  // everything a coder thread needs
    int cb, job, h, w;
    uint32_t n_ev;
    unsigned char *const *outs; const size_t *caps; long *lens;      // -e1: byte streams; effort 0: uint16_t streams, caps/lens in words
    int kind;                                                        // 0 / 2 = NBLIC range coder, 1 = QNBLIC entropy stage
    ::nblic_amd_batch *batch;                                        // whose completion this image counts towards
    int near, k_step, effort;                                        // header fields (NBLIC.c:682-694)
    int pack_n, pack_lane;                                           // pack_n >= 2: lane pack_lane of a pack of pack_n images whose rows are in pbufs[cb]; 1: on its own, u16 records in cbufs[cb]
};

// ---- one image in flight -------------------------------------------------------------------
struct Slot {
    E1Buffers b{};                    // the kernels' view; `mem` owns what it points at, except img, coded and totals (borrowed)
    DevPool mem;
    size_t px_cap = 0, ev_cap = 0;    // what the pixel-sized / event-sized buffers of b hold
    DevBuf<uint8_t> d_img;            // device copy when the caller hands a host image
    int cb = -1;                      // coded-bin buffer (HBM) this image's back half writes to
    int job = -1, h = 0, w = 0;       // current image
    int near = 0, effort = 1;         // its mode (kind 2 groups; 0 / 1 otherwise)
    uint32_t n_ev = 0;
    int pack_n = 1, pack_lane = 0;    // its place in a pack of the current launch (launch_back); cb is then the PACK's buffer, shared by its lanes
    // serial modes: reconstruction (near > 0) and least-squares statistics (efforts 2/3)
    DevBuf<uint8_t> d_recon; DevBuf<double> d_stats;
    SerialState *d_state = nullptr;   // what the model stage carries from launch to launch (serial_engine.h); in `mem`
};

// ---- a group of images that shares every kernel launch ---------------------------------------
// What a driver thread sleeps on while its group's front half runs (a host function queued behind the front half
// sets `ready`).  hipEventSynchronize is NOT a sleep here, whatever the event's flags say: measured, a driver burnt
// 35 ms of CPU per 55 ms wait, 1.1 of the rank's 16 CPUs between the six of them -- quota the coder threads need.
struct CollectFrom;                                    // below: what the _from calls hand down

struct GroupWait { std::mutex m; std::condition_variable cv; bool ready = false; };

struct Group {
    int id = 0;
    std::unique_ptr<GroupWait> front = std::make_unique<GroupWait>();
    Stream stream;
    Event done, tm_ev[kE1Marks];
    Event released;                                    // hipEventReleaseToSystem, recorded behind the back half: what the copy engine reads has left L2 (launch_back)
    E1Timers tm{};                                     // its events are tm_ev's
    std::vector<Slot> slots;
    Pinned<E1Job> h_jobs; DevBuf<E1Job> d_jobs;        // pinned host / device job records
    Pinned<SerialJob> h_sjobs; DevBuf<SerialJob> d_sjobs;   // the same images for the serial model stage (kind 2)
    unsigned char *const *recons = nullptr;            // kind 2: where each image's reconstruction goes (host; entries may be null)
    Pinned<uint32_t> h_totals; DevBuf<uint32_t> d_totals;   // kTotalsStride words per slot
    int n_jobs = 0;
    bool tm_pending = false;                           // timer events recorded, not yet read
    ::nblic_amd_ctx *ctx = nullptr;
    // the batch this group currently serves (valid from launch_back until its coders finish)
    unsigned char *const *outs = nullptr; const size_t *caps = nullptr; long *lens = nullptr;
    int kind = 0;
    ::nblic_amd_batch *batch = nullptr;
    // hand-over to the group's driver thread (guarded by ctx->dm)
    const uint8_t *const *imgs = nullptr; bool on_device = false; bool has_work = false;
    // the indexed effort-0 batch (qidx_driver), whose driver holds the group: page-locked buffers of the images in flight
    // (words | histograms | entry records | rows), the ring of queued steps' job records, tasks and totals, the staged
    // records.  Grow-only; allocated by the first such call
    std::vector<Locked> qidx_bufs; std::vector<Event> qidx_ready;
    Pinned<E1Job> qidx_jobs; Pinned<IndexRecordTask> qidx_tasks; Pinned<uint32_t> qidx_totals;
    DevBuf<IndexRecordTask> qidx_d_tasks; DevBuf<uint8_t> qidx_d_recs;
    // the _from calls (at the end: no member that existed before has moved).  Where the images lie, handed over with imgs /
    // on_device (guarded by ctx->dm; null: imgs / on_device say it)
    const CollectFrom *from = nullptr;
    // collection (collect.h): the tasks of the launch that is being put together, and their device copy.  Allocated by the
    // first call that collects; an indexed effort-0 batch uses one stretch of them per queued step
    Pinned<CollectTask> h_ctasks; DevBuf<CollectTask> d_ctasks; int n_ctasks = 0;
    Event ct_ev[2]; bool ct_pending = false;           // nblic_amd_enable_timing: the marks around a k_collect launch that nobody has read yet
    // reconstructions to device memory (nblic_amd_encode_batch_modes_from_to): the delivery tasks of the group's images and
    // their device copy.  Grow-only; allocated by the first call that delivers one
    Pinned<DeliverTask> h_dtasks; DevBuf<DeliverTask> d_dtasks;
};

}  // namespace nblic

using namespace nblic;

struct nblic_amd_ctx {
    int device = 0;
    long max_px = kMaxPixels;
    bool timing = false;
    uint64_t timing_mask = ~0ull;            // stages to time (kernels_e1.h E1Timers::mask)
    bool simd = false;                    // AVX-512 host: up to sixteen images per coder thread (two packs in lock-step)
    std::vector<Group> groups;
    std::mutex api;                       // one batch at a time per context
    std::mutex fm;                        // free groups / free coded-bin buffers / outstanding work
    std::condition_variable fcv;
    std::deque<int> free_groups;
    const bool trace = (dbg_flags() & kDbgTrace) != 0;   // timeline of groups and coder takes on stderr
    std::chrono::steady_clock::time_point t_batch;
    double now() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_batch).count(); }
    int coders_wanted = 0;                   // coder threads of this context (set before they start: pinning needs it)
    int max_take = kMaxTake;                 // images a coder thread takes together: 24 = three AVX-512 packs (NBLIC_AMD_MAX_TAKE=16: two, for A/B runs)
    std::vector<Stream> copy_streams;        // shared by the coder threads (device -> host chunk copies)
    CopyEngine engine;                       // the chunks of packs on a DMA engine instead (NBLIC_AMD_COPY_ENGINE=0: never opened); outlives the coder threads' signals
    size_t chunk_bins = kChunkBins;          // bins per lane per chunk (NBLIC_AMD_CHUNK_BINS shrinks it, for tests of the chunk boundaries)
    std::vector<CodedBuf> cbufs;             // one image's u16 records (images coded on their own; QNBLIC: pairs + histograms)
    std::deque<int> free_cbufs;              // both pools hand out the buffer returned last: memory is allocated for the backlog there is, not for the pool's size
    std::vector<PackRows> pbufs;             // one pack's rows (k_pack_rows writes them)
    std::deque<int> free_pbufs;
    int coding = 0;                       // images handed to the GPU whose streams are not finished yet
    // coder threads
    std::vector<std::thread> coders;
    std::mutex rm;
    std::condition_variable rcv;
    std::deque<ReadyImage> ready;
    int idle_coders = 0;
    int batch_to_come = 0;                // images of the running batch that have not reached `ready` yet (guarded by rm)
    bool stop = false;
    // One driver thread per group: a group's launch sequence has a host round trip in the middle
    // (the event count sizes the back half) and may wait for a coded-bin buffer; with a thread each,
    // one group waiting never keeps the others from being launched.
    std::vector<std::thread> drivers;
    std::mutex dm;
    std::condition_variable dcv;
    bool stop_drivers = false;
    std::atomic<bool> broken{false};         // a thread of the context could not set itself up (sticky); a failure of one image is recorded in ITS batch
    // reporting
    double stage_ms[kE1Kernels] = {0};
    long stage_launches = 0;
    double total_bins = 0, coder_s = 0;
    double pack_bins = 0, pack_s = 0;     // the part of the above coded in packs (2..16 images per thread)
    double wait_s = 0, issue_s = 0;       // of coder_s: waiting for bins to arrive from HBM / queueing the next chunk
    double driver_cpu_s = 0, driver_front_cpu_s = 0, driver_wait_cpu_s = 0; long driver_launches = 0;   // CPU time of the driver threads (reporting)
    long takes[kMaxTake + 1] = {0};       // how many times a thread took k images together
    std::mutex stat_m;
    // Submission is asynchronous: _begin only queues the batch; the submitter thread hands its images to the groups
    // (which blocks while every group is busy), so a caller can keep several batches ahead of the pipeline.
    struct SubmitItem {
        ::nblic_amd_batch *b; int kind;       // 0 NBLIC (per image near / effort), 1 QNBLIC (outs are uint16_t streams, caps / lens in words)
        int n; const uint8_t *const *imgs; bool on_device; const int *hs, *ws;
        uint8_t *const *outs; const size_t *caps; long *lens; const int *nears, *efforts; unsigned char *const *recons;
        const CollectFrom *from = nullptr;    // the _from calls: imgs / on_device / hs / ws are its own (collect_plan)
    };
    std::thread submitter;
    std::mutex sm;
    std::condition_variable scv;
    std::deque<SubmitItem> sq;
    bool stop_submit = false;
    int queued_images = 0;                // images of batches still waiting in sq (guarded by rm, like batch_to_come)
    // device coder (device_coder.hip): pack threads that hand 64 queued images at a time to one wave each
    std::vector<std::thread> dev_coders;
    int dev_min_outstanding = 0;          // a pack is taken only while at least this many images of the submitted batches are unfinished
    double dev_bins = 0; long dev_packs = 0, dev_images = 0;
    // device rANS stage of effort 0 (q_device_coder.hip): ONE thread with one stream and a rolling job list (qdev_main)
    std::thread qdev;                     // started by the first nblic_amd_set_device_qcoder that names mode 1 or 2; sleeps in mode 0
    int qmode = 0;                        // 0 host, 1 device, 2 shared (guarded by rm)
    uint32_t q_budget = 0;                // symbols per launch (guarded by rm); 0 until the first set call
    double qdev_symbols = 0, qdev_kernel_ms = 0; long qdev_launches = 0, qdev_images = 0;   // guarded by stat_m
    // decode batches (nblic_amd_decode_batch): a stream of their own and grow-only device / pinned arenas
    Stream dec_stream, dec_stream2;                                    // decode_batch alternates its chunks between the two
    DevBuf<uint8_t> dec_arena;
    DevBuf<SerialJob> dec_jobs;
    int index_round_segments = 0;         // > 0: at most this many segments per round of the indexed decode (nblic_amd_set_index_round)
    int serial_rows = 0;                  // rows per launch of the serial kernels; 0 = sized for a few seconds per launch (nblic_amd_set_serial_rows)
    DevBuf<unsigned long long> d_redo;          // device: pixels whose least-squares system 0 / 1 was redone with integers (SerialJob::redo of every job of the context)
    double idx_split[5] = {0}; long idx_steps = 0;   // the last indexed batch, summed over its group steps: front, totals read-back, back half + entry records, copies (GPU ms); coder wait (host ms).  Guarded by stat_m
    double idxbuild_split[4] = {0};       // the last batch index build: host checks, uploads and seeding, the decode-and-capture launches, the finish (host ms).  Guarded by stat_m
    double idxdec_split[4] = {0};         // the last indexed batch decode: host checks, uploads, rounds and chain check, copy-out (host ms).  Guarded by stat_m
    int long_min = 0, long_block = 0;     // nblic_amd_set_long_chains as given (0: the default); what a job record carries is long_chains_of()
    long long_counts[8] = {0};            // nblic_amd_long_chain_stats: summed from the totals records the front halves leave.  Guarded by stat_m
    long serial_launch_count = 0;         // launches of the serial model / decode kernels since the context was created (reporting, tests)
    size_t feed_chunk = size_t(1) << 20;  // bytes per step in which the drop-in decoders fetch a stream of unknown length (nblic_amd_set_feed_chunk)
    long fed_bytes = 0;                   // bytes the last drop-in decode read from the caller's stream
    int feed_pipe[2] = {-1, -1};          // safe_copy: the kernel does the reading
    DevBuf<DeliverTask> dec_deliver;      // nblic_amd_decode_batch_to: the chunks' delivery tasks (grow-only, like dec_jobs)
    DevBuf<StackDeliverTask> dec_runs;    // nblic_amd_decode_batch_to_ex_stack: the runs of the call's k_deliver_stack launch and
    DevBuf<StackSlice> dec_slices;        // their slice records (grow-only too)
    std::atomic<long> collect_counts[4] = {};   // nblic_amd_collect_stats: images in place, images collected, k_collect launches, pixels collected
    double collect_ms = 0; long collect_timed = 0;   // nblic_amd_collect_ms: GPU time of the k_collect launches that were timed, and how many.  Guarded by stat_m
    std::atomic<long> color_counts[2] = {};     // nblic_amd_color_plan_stats: k_color_cost launches, pixels read (three per frame position)
    double color_ms = 0;                        // nblic_amd_color_plan_stats: GPU time of the last nblic_amd_color_plan's launch.  Guarded by stat_m
    std::atomic<long> stack_counts[4] = {};     // nblic_amd_stack_plan_stats: k_stack_cost launches, source elements read, k_deliver_stack launches, runs delivered
    double stack_ms = 0, stack_deliver_ms = 0;  // GPU time of the last nblic_amd_stack_plan's launch / of the last timed k_deliver_stack launch.  Guarded by stat_m
    long deliver_tasks = 0, deliver_strided = 0;     // nblic_amd_deliver_stats: of the last call that delivers.  Guarded by stat_m (at the end: no member has moved)
    DevBuf<DeepDeliverTask> dec_deep;           // nblic_amd_decode_batch_to_ex_deep: the tasks of the call's k_deliver_deep launch (grow-only)
    std::atomic<long> deep_counts[4] = {};      // nblic_amd_deep_plan_stats: k_deep_cost, k_collect_deep and k_deliver_deep launches, deep images planned
    double deep_ms[3] = {0, 0, 0};              // GPU time of the last k_deep_cost, k_collect_deep and k_deliver_deep launch of a plan, an encoder and a decoder.  Guarded by stat_m
    QueuePlan queue_plan;                       // nblic_amd_queue_plan_stats: how the group streams were spread over the hardware queues (queue_plan.h); written once, by create_ex
};

namespace nblic {

// ---- the small protocols under ctx->fm: groups, coded-bin buffers, outstanding images --------------------------------
// A free group of the context (waits for one: every group busy is the back-pressure on submission).
static int take_group(nblic_amd_ctx *c) {
    std::unique_lock<std::mutex> l(c->fm);
    c->fcv.wait(l, [c] { return !c->free_groups.empty(); });
    const int id = c->free_groups.front();
    c->free_groups.pop_front();
    return id;
}

static void release_group(nblic_amd_ctx *c, int id) {
    { std::lock_guard<std::mutex> g(c->fm); c->free_groups.push_back(id); }
    c->fcv.notify_all();
}

static bool nothing_outstanding(nblic_amd_ctx *c) {
    std::lock_guard<std::mutex> l(c->fm);
    return c->coding == 0;
}

// The coded-bin buffer a slot took for an image that will not reach a coder goes back to the pool.
static void return_coded(nblic_amd_ctx *c, Slot &s) {
    if (s.cb < 0) return;
    {
        std::lock_guard<std::mutex> l(c->fm);
        if (s.pack_n <= 1) c->free_cbufs.push_front(s.cb);
        else if (s.pack_lane == 0) c->free_pbufs.push_front(s.cb);       // a pack's buffer goes back once, with its first lane
    }
    s.cb = -1; s.pack_n = 1; s.pack_lane = 0;
    c->fcv.notify_all();
}

// n images are finished (lens written): their coded-bin buffers go back, and they are counted off their batches and
// off the context's outstanding work.
static void finish_images(nblic_amd_ctx *c, const ReadyImage *im, int n) {
    {
        std::lock_guard<std::mutex> l(c->fm);
        for (int k = 0; k < n; k++) {
            if (im[k].pack_n <= 1) c->free_cbufs.push_front(im[k].cb);
            else if (im[k].pack_lane == 0) c->free_pbufs.push_front(im[k].cb);   // whole packs are taken and finished together
            im[k].batch->remaining -= 1;
        }
        c->coding -= n;
    }
    c->fcv.notify_all();
}

// Where an NBLIC image's coder bytes go: the caller's capacity clamped (SIZE_MAX means "no limit"), the 16-byte header
// written if it fits.  Returns the first byte after the header; *room = bytes the coder may write there.
static uint8_t *begin_stream_out(const ReadyImage &im, size_t *room) {
    const size_t cap = std::min(im.caps[im.job], size_t(1) << 46);
    *room = cap >= size_t(kHeaderBytes) ? cap - kHeaderBytes : 0;
    if (cap >= size_t(kHeaderBytes)) write_header(im.outs[im.job], im.h, im.w, im.near, im.k_step, im.effort);
    return im.outs[im.job] + kHeaderBytes;
}

// ---- the queue plan's probe (queue_plan.h): "does stream b wait behind stream a?" -------------------------------------
// A wave that reads the clock until `ticks` have passed, `cap` times at the most, so it ends whatever the clock does.  It
// writes nothing.
__global__ void k_queue_probe_busy(unsigned long long ticks, unsigned cap) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (unsigned i = 0; i < cap; i++) {
        if (__builtin_amdgcn_s_memtime() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(16);
    }
}
__global__ void k_queue_probe_empty() {}

struct QueueProbe {
    static constexpr unsigned kCap = 20000;                          // each turn of the loop sleeps ~1000 clocks: some 10 ms at the most
    static constexpr double kWantMs = 1.0;
    unsigned long long ticks = 2000000;                              // ~1 ms: s_memtime counts shader clocks here (2-2.4 GHz); calibrate() measures what that is and corrects it once where the clock is another
    double busy_ms = 0;                                              // the busy kernel alone, launch to drained, as the host sees it
    static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    // The busy kernel's own duration on stream a: the least of three.  kProbeFree: measured and usable.
    int measure(hipStream_t a) {
        busy_ms = 1e30;
        for (int rep = 0; rep < 3; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            hipLaunchKernelGGL(k_queue_probe_busy, dim3(1), dim3(64), 0, a, ticks, kCap);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return kProbeError;
            busy_ms = std::min(busy_ms, ms_since(t0));
        }
        return kProbeFree;
    }
    int calibrate(hipStream_t a) {
        hipLaunchKernelGGL(k_queue_probe_empty, dim3(1), dim3(64), 0, a);              // the code object is loaded and the stream has its queue before anything is timed
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return kProbeError;
        int r = measure(a);
        if (r != kProbeFree) return r;
        if (busy_ms < 0.5 * kWantMs && busy_ms > 0.001) {            // a faster clock than assumed: once more with the ticks scaled (the cap still bounds the kernel)
            ticks = (unsigned long long)(double(ticks) * kWantMs / busy_ms);
            if ((r = measure(a)) != kProbeFree) return r;
        }
        return busy_ms >= 0.3 * kWantMs && busy_ms <= 20.0 * kWantMs ? kProbeFree : kProbeInconclusive;
    }
    // b waits behind a when an empty kernel on b, launched behind the busy kernel on a, takes more than half the busy
    // kernel's duration to drain in EVERY one of three repetitions: on one queue all are slow, on two one fast one is
    // enough, so what other tenants of the card do can only err toward "free".
    int blocks(hipStream_t a, hipStream_t b) {
        for (int rep = 0; rep < 3; rep++) {
            hipLaunchKernelGGL(k_queue_probe_busy, dim3(1), dim3(64), 0, a, ticks, kCap);
            if (hipGetLastError() != hipSuccess) return kProbeError;
            const auto t0 = std::chrono::steady_clock::now();
            hipLaunchKernelGGL(k_queue_probe_empty, dim3(1), dim3(64), 0, b);
            const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(b) == hipSuccess;
            const double ms = ms_since(t0);
            if (hipStreamSynchronize(a) != hipSuccess || !ok) return kProbeError;
            if (ms < 0.5 * busy_ms) return kProbeFree;
        }
        return kProbeBlocks;
    }
};

// The group streams of a context with three groups or more, spread over the hardware queues the process has (queue_plan.h):
// streams[g] is group g's, or the vector is empty and every group creates its own, as the runtime deals them.  Runs on
// the creating thread before any other thread of the context exists.
static void plan_group_streams(nblic_amd_ctx *c, int n_groups, std::vector<Stream> &streams) {
    QueuePlan &p = c->queue_plan;
    p.n_groups = n_groups;
    if (n_groups < 3) { p.state = kPlanFewGroups; return; }
    if (const char *v = getenv("NBLIC_AMD_QUEUE_PLAN")) if (atoi(v) == 0) { p.state = kPlanSwitchedOff; }
    if (p.state != kPlanSwitchedOff) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<Stream> cand;
        QueueProbe probe;
        bool calibrated = false;
        p = plan_queues(n_groups,
            [&]() -> int {
                cand.emplace_back();
                if (cand.back().create(hipStreamNonBlocking) != hipSuccess) { cand.pop_back(); return -1; }
                return int(cand.size()) - 1;
            },
            [&](int a, int b) -> int {
                if (!calibrated) { const int r = probe.calibrate(cand[size_t(a)]); if (r != kProbeFree) return r; calibrated = true; }
                return probe.blocks(cand[size_t(a)], cand[size_t(b)]);
            },
            [&](int id) { cand[size_t(id)] = Stream(); });
        if (p.state == kPlanOn) for (int id : p.chosen) streams.push_back(std::move(cand[size_t(id)]));
        p.plan_ms = QueueProbe::ms_since(t0);
    }
    if (p.state != kPlanOn) fprintf(stderr, "[nblic_amd] queue plan off (%s): one stream per group as the runtime deals them\n", queue_plan_state_name(p.state));
}

static bool group_init(Group &g, int id, int n_slots, nblic_amd_ctx *c, Stream *planned = nullptr) {
    g.id = id; g.ctx = c;
    g.slots.resize(size_t(n_slots));
    if (planned) g.stream = std::move(*planned);
    else HIP_OK(g.stream.create(hipStreamNonBlocking));
    HIP_OK(g.done.create(hipEventDisableTiming | hipEventBlockingSync));
    if (c->engine.available()) HIP_OK(g.released.create(hipEventDisableTiming | hipEventReleaseToSystem));
    for (int k = 0; k < kE1Marks; k++) { HIP_OK(g.tm_ev[k].create(hipEventDefault)); g.tm.ev[k] = g.tm_ev[k]; }
    HIP_OK(g.h_jobs.alloc(size_t(n_slots))); HIP_OK(g.d_jobs.alloc(size_t(n_slots)));
    HIP_OK(g.h_sjobs.alloc(size_t(n_slots))); HIP_OK(g.d_sjobs.alloc(size_t(n_slots)));
    HIP_OK(g.h_totals.alloc(size_t(n_slots) * kTotalsSlot)); HIP_OK(g.d_totals.alloc(size_t(n_slots) * kTotalsSlot));
    for (int k = 0; k < n_slots; k++) {
        Slot &s = g.slots[size_t(k)];
        DevPool &m = s.mem;
        HIP_OK(m.renew(s.b.table, size_t(4096) * kMaxSegments)); HIP_OK(m.renew(s.b.scan_sums, (size_t(1) << 20) / sizeof(uint32_t)));
        s.b.totals = g.d_totals + size_t(k) * kTotalsSlot;
        HIP_OK(m.renew(s.b.ctx_state, 4096));                                        // 2048 (NBLIC) or 3072 (QNBLIC) contexts
        HIP_OK(m.renew(s.b.qhist, 12 * 256)); HIP_OK(m.renew(s.b.map_state, 512 * 60)); HIP_OK(m.renew(s.b.cnt_state, 4096 * 2));
        HIP_OK(m.renew(s.b.win_base, 4097 + 4096)); HIP_OK(m.renew(s.b.blk_base, 4097)); HIP_OK(m.renew(s.b.mblk_base, 513)); HIP_OK(m.renew(s.b.mend_cnt, 512 * 20)); HIP_OK(m.renew(s.b.dbg_out, 4096));
        HIP_OK(hipMemset(s.b.dbg_out, 0, 4096 * sizeof(unsigned long long)));
        uint8_t *state = nullptr;
        HIP_OK(m.renew(state, kModelStateBytes));
        s.d_state = reinterpret_cast<SerialState *>(state);
    }
    return true;
}

// The event-sized / pixel-sized buffers of a slot grow together; while they do their capacity is 0, so after a failure half way the next call replaces them all.
static bool ensure_events(Slot &s, size_t n_ev) {
    if (n_ev <= s.ev_cap) return true;
    const size_t cap = n_ev + n_ev / 8 + 1024;
    DevPool &m = s.mem;
    s.ev_cap = 0;
    HIP_OK(m.renew(s.b.events, cap)); HIP_OK(m.renew(s.b.tin, 2 * cap + kStreamPad)); HIP_OK(m.renew(s.b.tpos, cap + 64));
    HIP_OK(m.renew(s.b.tout, 2 * cap + kStreamPad)); HIP_OK(m.renew(s.b.win_recs, (2 * cap / 512 + 4096 + 8) * 24));
    s.ev_cap = cap;
    return true;
}

static bool ensure_pixels(Slot &s, size_t n, bool with_events = true) {
    if (n > s.px_cap) {
        DevPool &m = s.mem;
        s.px_cap = 0;
        HIP_OK(m.renew(s.b.rec1, n)); HIP_OK(m.renew(s.b.s2in, n + kStreamPad)); HIP_OK(m.renew(s.b.pos2, n)); HIP_OK(m.renew(s.b.s2out, n + kStreamPad));
        HIP_OK(m.renew(s.b.pxs, n)); HIP_OK(m.renew(s.b.s3in, n + kStreamPad)); HIP_OK(m.renew(s.b.pos3, n)); HIP_OK(m.renew(s.b.s3out, n + kStreamPad));
        HIP_OK(m.renew(s.b.z, n)); HIP_OK(m.renew(s.b.cnt, n)); HIP_OK(m.renew(s.b.ev_off, n));
        HIP_OK(m.renew(s.b.blk_end, n / 4096 + 4096 + 64)); HIP_OK(m.renew(s.b.blk_ok, n / 4096 + 4096 + 64));
        HIP_OK(m.renew(s.b.blk_cand, 2 * (n / 4096 + 4096 + 64))); HIP_OK(m.renew(s.b.blk_item, n / 4096 + 64)); HIP_OK(m.renew(s.b.blk_tab, 128 * (n / 4096 + 64)));
        HIP_OK(m.renew(s.b.mblk_cnt, 20 * (n / kLongBlockMin + 512))); HIP_OK(m.renew(s.b.mblk_perm, 4 * (n / kLongBlockMin + 512)));
        s.px_cap = n;
    }
    return with_events ? ensure_events(s, 5 * n) : true;   // typical images need 4.3-4.5 bins/px (ensure_events adds 1/8); grown on demand
}

// ---- job records: the only code that fills an E1Job, or a SerialJob for the encoders' model stage -------------------
// The back half's view of a job: the buffers as they are now (the event-sized ones may have grown, `coded` is known)
// and the bin count with its partition plan.
static void e1_job_back(E1Job &J, const E1Buffers &b, uint32_t n_ev, uint64_t *pack_rows = nullptr, int pack_lane = 0) {
    J.b = b; J.n_ev = n_ev; J.pe = make_plan(n_ev, kTouchSegments);
    J.pack_rows = pack_rows; J.pack_lane = pack_lane;
}

// The job of `rows` x w pixels in workspace b as a front half sees it: no bins yet (their count is its result).
// near is 0 for the staged -e1 and the QNBLIC kernels, which use the lossless constants whatever the record says;
// dbg is NBLIC_AMD_DBG for the staged -e1 kernels and 0 for everything else.
// Long chains: what nblic_amd_set_long_chains left in the context, as a job record carries it.
constexpr int kLongMinDefault = 65536, kLongBlockDefault = 4096;
struct LongChains { int min_records, block_records; };
static LongChains long_chains_of(const nblic_amd_ctx *c) {
    if (c->long_min < 0) return LongChains{-1, 0};
    return LongChains{c->long_min ? c->long_min : kLongMinDefault, std::max(c->long_block ? c->long_block : kLongBlockDefault, kLongBlockMin)};
}
// the block counts of one image's front half, from its totals record
static void count_long_chains(nblic_amd_ctx *c, const uint32_t *totals) {
    std::lock_guard<std::mutex> l(c->stat_m);
    c->long_counts[0] += totals[kLongS2Met]; c->long_counts[1] += totals[kLongS2Table]; c->long_counts[2] += totals[kLongS2Serial];
    c->long_counts[3] += totals[kLongS3Split]; c->long_counts[4] += totals[kLongS3Accepted]; c->long_counts[5] += totals[kLongS3Missed];
}

static E1Job e1_job_front(const E1Buffers &b, int rows, int w, int near, int dbg, LongChains lc) {
    E1Job J{};
    J.h = rows; J.w = w; J.n = uint32_t(size_t(rows) * size_t(w)); J.pp = make_plan(J.n); J.dbg = dbg;
    J.long_min = lc.min_records; J.long_block = lc.block_records;
    J.near = near; J.k_step = k_step_for_near(near); J.ktab = level_shift_table(J.k_step);
    e1_job_back(J, b, 0);
    return J;
}

// The front job of the band [row0, row0 + rows) of a w-wide plane on the device, in workspace b: the band encoder's and the
// indexed batches'.
static E1Job band_job_front(const nblic_amd_ctx *c, E1Buffers b, const uint8_t *plane, int row0, int rows, int w, int near) {
    b.img = plane + size_t(row0) * size_t(w);
    E1Job J = e1_job_front(b, rows, w, near, 0, long_chains_of(c));
    J.row0 = row0;
    return J;
}

// The job of k_serial_model for an image of h x w: `rows` rows per launch, whose records go to b.rec1 / b.pxs from
// index 0 on (out_row0: the image row that sits there -- 0, or the first row of a band).
static SerialJob model_job(const uint8_t *img, uint8_t *recon, const E1Buffers &b, double *stats, SerialState *state, int h, int w,
                           int near, int effort, int rows, int out_row0, unsigned long long *redo) {
    SerialJob Q{};
    Q.img = img; Q.recon = recon; Q.rec1 = b.rec1; Q.pxs = b.pxs; Q.stats = stats; Q.state = state;
    Q.h = h; Q.w = w; Q.near = near; Q.k_step = k_step_for_near(near); Q.effort = effort;
    Q.rows = rows; Q.out_row0 = out_row0; Q.redo = redo;
    return Q;
}

// ---- collection from caller-owned device memory (collect.h, serial_engine.h k_collect) ------------------------------------
// What the _from calls hand down: one source per image, one format and one quantisation per call, and what collect_plan
// (below, beside the delivery's checks) made of them on the host: per image refused, used where it lies, or collected
// by a task; and the arguments of the parent call -- plane pointers (in place: the source; else null), heights, widths
// (a refused image: 0 x 0, which the parent refuses).
enum : uint8_t { kSrcRefused = 0, kSrcInPlace = 1, kSrcCollect = 2 };
struct CollectFrom {
    const nblic_amd_src *srcs; uint32_t format; float scale, bias;
    std::vector<uint8_t> modes;                                          // not empty: sources 3f, 3f + 1, 3f + 2 are R, G, B of frame f, coded in colour mode modes[f] (color_plan.h)
    std::vector<uint8_t> slice_modes; int depth = 0;                     // not empty: source s * depth + d is slice d of stack s, in slice mode slice_modes[s * depth + d] (stack.h)
    std::vector<uint8_t> how;
    std::vector<CollectTask> tasks;                                      // kSrcCollect: all but dst, px0, px1 and first_chunk
    std::vector<const uint8_t *> imgs; std::vector<int> hs, ws;
    // nblic_amd_encode_batch_modes_from_to: where image k's reconstruction goes (recon_ok[k]) -- a task that lacks only src,
    // src_bytes and gate, which the group that encodes the image knows.  Empty: no reconstruction leaves by this door
    std::vector<DeliverTask> recon_tasks; std::vector<uint8_t> recon_ok;
};

// Room for n tasks in group g.
static bool collect_room(Group &g, size_t n) {
    if (g.h_ctasks.capacity() >= n) return true;
    HIP_OK(hipStreamSynchronize(g.stream));                              // (a queued upload may still read the old block)
    HIP_OK(g.h_ctasks.alloc(n)); HIP_OK(g.d_ctasks.alloc(n));
    return true;
}
static void collect_begin(Group &g) { g.n_ctasks = 0; }
// Appends the task that collects pixels [px0, px1) of image k's flat plane into the plane at dst (16-byte aligned).
static bool collect_add(Group &g, const CollectFrom &from, int k, uint8_t *dst, uint32_t px0, uint32_t px1, size_t at = 0) {
    if (at + size_t(g.n_ctasks) >= g.h_ctasks.capacity()) return false;
    CollectTask &T = g.h_ctasks[at + size_t(g.n_ctasks++)];
    T = from.tasks[size_t(k)];
    T.dst = dst; T.px0 = px0; T.px1 = px1;
    if (px0 == 0) { g.ctx->collect_counts[1]++; g.ctx->collect_counts[3] += long(T.rows) * long(T.cols); }
    return true;
}
// The marks of group g's last timed k_collect launch, added to the context's figures.  wait: for a launch still running
// (else it is left for later).  false: the marks are still in use.
static bool collect_timing_read(Group &g, bool wait) {
    if (!g.ct_pending) return true;
    if (!wait && hipEventQuery(g.ct_ev[1]) != hipSuccess) { (void)hipGetLastError(); return false; }
    float ms = 0.f;
    if (hipEventSynchronize(g.ct_ev[1]) == hipSuccess && hipEventElapsedTime(&ms, g.ct_ev[0], g.ct_ev[1]) == hipSuccess) {
        std::lock_guard<std::mutex> l(g.ctx->stat_m);
        g.ctx->collect_ms += ms; g.ctx->collect_timed++;
    }
    g.ct_pending = false;
    return true;
}

// ONE k_collect launch over the tasks appended since collect_begin, queued on st (none: nothing is queued).  With
// nblic_amd_enable_timing the launch stands between two marks of the group, when the pair is free: the steps an indexed
// effort-0 batch queues ahead are not all timed (nblic_amd_collect_ms says how many were).
static bool collect_flush(Group &g, hipStream_t st, size_t at = 0) {
    if (g.n_ctasks == 0) return true;
    const bool timed = g.ctx->timing && collect_timing_read(g, false) && (g.ct_ev[0] || (g.ct_ev[0].create(hipEventDefault) == hipSuccess && g.ct_ev[1].create(hipEventDefault) == hipSuccess));
    CollectTask *h = g.h_ctasks + at, *d = g.d_ctasks + at;
    unsigned long long chunks = 0;
    for (int i = 0; i < g.n_ctasks; i++) { h[i].first_chunk = uint32_t(chunks); chunks += collect_task_chunks(h[i]); }
    if (chunks >= (1ull << 31)) return false;
    HIP_OK(hipMemcpyAsync(d, h, size_t(g.n_ctasks) * sizeof(CollectTask), hipMemcpyHostToDevice, st));
    if (timed) HIP_OK(hipEventRecord(g.ct_ev[0], st));
    if (!collect_launch(d, g.n_ctasks, uint32_t(chunks), st)) return false;
    if (timed) { HIP_OK(hipEventRecord(g.ct_ev[1], st)); g.ct_pending = true; }
    g.ctx->collect_counts[2]++;
    g.n_ctasks = 0;
    return true;
}

// The reconstructions of group g's images into the caller's device memory: ONE k_deliver launch on the group's stream,
// behind the launches that made the planes.  An image's plane is its reconstruction (near > 0), or what was encoded -- the
// collected plane, or the source where it lies.  gated: by the serial model's record, so an image that failed there leaves
// zeros.  Their tasks count for nblic_amd_deliver_stats.
static bool recon_deliver(Group &g, const CollectFrom *from, bool gated) {
    if (!from || from->recon_tasks.empty()) return true;
    if (g.h_dtasks.capacity() < g.slots.size()) {
        HIP_OK(hipStreamSynchronize(g.stream));                          // (a queued upload may still read the old block)
        HIP_OK(g.h_dtasks.alloc(g.slots.size())); HIP_OK(g.d_dtasks.alloc(g.slots.size()));
    }
    int n = 0;
    long strided = 0;
    unsigned long long chunks = 0;
    for (int k = 0; k < g.n_jobs; k++) {
        const Slot &s = g.slots[size_t(k)];
        if (!from->recon_ok[size_t(s.job)]) continue;
        DeliverTask &T = g.h_dtasks[n++];
        T = from->recon_tasks[size_t(s.job)];
        T.src = s.near > 0 ? s.d_recon.get() : s.b.img; T.src_bytes = size_t(s.h) * size_t(s.w);
        T.gate = gated ? s.d_state : nullptr;
        T.first_chunk = uint32_t(chunks); chunks += deliver_task_chunks(T);
        strided += deliver_strided(T) ? 1 : 0;
    }
    if (n == 0) return true;
    if (chunks >= (1ull << 31)) return false;
    HIP_OK(hipMemcpyAsync(g.d_dtasks, g.h_dtasks, size_t(n) * sizeof(DeliverTask), hipMemcpyHostToDevice, g.stream));
    if (!deliver_launch(g.d_dtasks, n, uint32_t(chunks), g.stream)) return false;
    std::lock_guard<std::mutex> l(g.ctx->stat_m);
    g.ctx->deliver_tasks += n; g.ctx->deliver_strided += strided;
    return true;
}

// What every front half starts with for slot k of group g (which already carries job / h / w / near): its workspace,
// its input plane on the device -- the caller's, a copy on the group's stream, or a source that the group's k_collect
// launch (collect_flush, once the slots have begun) writes into the slot's d_img -- and its job record.
static bool slot_begin(Group &g, int k, const uint8_t *const *imgs, bool on_device, bool with_events, int dbg, const CollectFrom *from = nullptr) {
    Slot &s = g.slots[size_t(k)];
    const size_t n = size_t(s.h) * size_t(s.w);
    if (!ensure_pixels(s, n, with_events)) return false;
    if (from && from->how[size_t(s.job)] == kSrcCollect) {
        HIP_OK(s.d_img.reserve(n));
        if (!collect_add(g, *from, s.job, s.d_img, 0, uint32_t(n))) return false;
        s.b.img = s.d_img;
    } else if (on_device) {
        if (from) g.ctx->collect_counts[0]++;
        s.b.img = imgs[s.job];
    } else {
        HIP_OK(s.d_img.reserve(n));
        HIP_OK(hipMemcpyAsync(s.d_img, imgs[s.job], n, hipMemcpyHostToDevice, g.stream));
        s.b.img = s.d_img;
    }
    s.n_ev = 0; s.pack_n = 1; s.pack_lane = 0;                     // (a pack is made in launch_back, for that launch only)
    g.h_jobs[k] = e1_job_front(s.b, s.h, s.w, s.near, dbg, long_chains_of(g.ctx));
    return true;
}

// Front half for the images assigned to group g (slots 0..n_jobs-1 already carry job/h/w).
static bool launch_front(nblic_amd_ctx *c, Group &g, const uint8_t *const *imgs, bool on_device, const CollectFrom *from = nullptr) {
    collect_begin(g);
    if (from && !collect_room(g, g.slots.size())) return false;
    for (int k = 0; k < g.n_jobs; k++)
        if (!slot_begin(g, k, imgs, on_device, true, dbg_flags(), from)) return false;
    if (!collect_flush(g, g.stream)) return false;
    if (!recon_deliver(g, from, false)) return false;
    for (int k = 0; k < g.n_jobs && from && g.recons; k++) {             // -n0 -e1: the reconstruction IS the collected plane
        const Slot &s = g.slots[size_t(k)];
        if (from->how[size_t(s.job)] == kSrcCollect && g.recons[s.job])
            HIP_OK(hipMemcpyAsync(g.recons[s.job], s.d_img, size_t(s.h) * size_t(s.w), hipMemcpyDeviceToHost, g.stream));
    }
    HIP_OK(hipMemcpyAsync(g.d_jobs, g.h_jobs, size_t(g.n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, g.stream));
    g.tm.mask = c->timing_mask;
    e1_launch_front(g.d_jobs, g.h_jobs, g.n_jobs, g.stream, c->timing ? &g.tm : nullptr);
    HIP_OK(hipMemcpyAsync(g.h_totals, g.d_totals, size_t(g.n_jobs) * kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    return true;
}

// Front half of a serial-mode group (near > 0 and / or efforts 2, 3): model state init, the serial
// model stage (one wave per image, all images of the group side by side; the slots are ordered by
// effort, one launch per effort present), the reconstructions on their way back to the host, then
// the re-mapper partition and chains and the bin counts.
static bool launch_front_serial(nblic_amd_ctx *c, Group &g, const uint8_t *const *imgs, bool on_device, const CollectFrom *from = nullptr) {
    collect_begin(g);
    if (from && !collect_room(g, g.slots.size())) return false;
    for (int k = 0; k < g.n_jobs; k++) {
        if (!slot_begin(g, k, imgs, on_device, true, 0, from)) return false;
        Slot &s = g.slots[size_t(k)];
        const size_t n = size_t(s.h) * size_t(s.w);
        const bool wide = !serial_model_rows_fit(s.w);                   // rows do not fit in LDS: taps come from the reconstruction in memory
        const bool want_recon = s.near > 0 || wide;
        if (want_recon) HIP_OK(s.d_recon.reserve(n));
        const size_t st = stats_doubles(s.effort, s.w);
        HIP_OK(s.d_stats.reserve(st));
        if (st) HIP_OK(hipMemsetAsync(s.d_stats, 0, st * sizeof(double), g.stream));         // NBLIC.c:789
        g.h_sjobs[k] = model_job(s.b.img, want_recon ? s.d_recon.get() : nullptr, s.b, s.d_stats, s.d_state, s.h, s.w, s.near, s.effort,
                                 serial_rows_per_launch(s.h, s.w, s.effort, c->serial_rows), 0, c->d_redo);
        HIP_OK(hipMemsetAsync(s.d_state, 0, sizeof(SerialState), g.stream));               // a fresh image: row 0, running
    }
    if (!collect_flush(g, g.stream)) return false;
    HIP_OK(hipMemcpyAsync(g.d_jobs, g.h_jobs, size_t(g.n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, g.stream));
    HIP_OK(hipMemcpyAsync(g.d_sjobs, g.h_sjobs, size_t(g.n_jobs) * sizeof(SerialJob), hipMemcpyHostToDevice, g.stream));
    e1_launch_init(g.d_jobs, g.n_jobs, g.stream);
    for (int k0 = 0; k0 < g.n_jobs;) {
        int k1 = k0 + 1;
        while (k1 < g.n_jobs && g.slots[size_t(k1)].effort == g.slots[size_t(k0)].effort) k1++;
        // an image is worked through `rows` rows per launch (its state record carries it from one to the next), so no
        // kernel runs longer than a few seconds however large the image; images that are done return at once
        int launches = 1;
        for (int k = k0; k < k1; k++) launches = std::max(launches, serial_launches(g.h_sjobs[k].h, g.h_sjobs[k].rows));
        for (int l = 0; l < launches; l++)
            if (!serial_model_launch(g.d_sjobs + k0, g.h_sjobs + k0, k1 - k0, g.stream)) return false;
        { std::lock_guard<std::mutex> sl(c->stat_m); c->serial_launch_count += launches; }
        k0 = k1;
    }
    if (!recon_deliver(g, from, true)) return false;
    for (int k = 0; k < g.n_jobs; k++) {                                 // the encoder leaves the reconstruction in the caller's plane (NBLIC.c:876)
        Slot &s = g.slots[size_t(k)];
        unsigned char *dst = g.recons ? g.recons[s.job] : nullptr;
        if (!dst) continue;
        const size_t n = size_t(s.h) * size_t(s.w);
        if (s.near > 0) HIP_OK(hipMemcpyAsync(dst, s.d_recon, n, hipMemcpyDeviceToHost, g.stream));
        else if (!on_device && dst != imgs[s.job]) memcpy(dst, imgs[s.job], n);
        else if (on_device) HIP_OK(hipMemcpyAsync(dst, s.b.img, n, hipMemcpyDeviceToHost, g.stream));      // (the caller's plane, or the collected one)
    }
    e1_launch_front_pre(g.d_jobs, g.h_jobs, g.n_jobs, g.stream);
    HIP_OK(hipMemcpyAsync(g.h_totals, g.d_totals, size_t(g.n_jobs) * kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    return true;
}

// ---- bins leave HBM in the layout the host coder wants ---------------------------------------
// A host coder thread codes up to 24 images at once: three AVX-512 registers of eight 64-bit lanes in lock-step
// (range_coder_x8.cpp).  What a register consumes is a PACK: 64 bins of each of its eight lanes as thirteen 64-bit words
// of 13-bit codes, the eight lanes of a word side by side -- one aligned 64-byte load per four steps, and the link
// carries 13 bits per bin instead of 16.  The pack is fixed when a group is LAUNCHED (launch_back: up to eight
// consecutive jobs, the job's place is the lane) and its rows are written inside that launch, on the group's own stream
// (kernels_e1.hip: k_mix leaves every image's groups in a stream of its own, k_pack_rows transposes a pack's streams
// into its PackRows buffer).  A chunk of a pack is then ONE contiguous copy from the pack buffer into the thread's ring:
// the copy streams carry nothing but copies and event records.  A coder thread takes one to three whole packs.
// Images that are coded on their own (a group of one, the tail of a batch, the band encoder, QNBLIC) keep the plain u16 records and the scalar coder.
// (Measured and rejected: a kernel that stores the rows straight into the mapped host ring.  The PCIe-bound waves crowd
// the encoder's own kernels off the GPU: 4.6 -> 2.4 Gpx/s chip-wide, 3.34 / 2.68 / 2.46 Gpx/s with 16 / 48 / 128
// workgroups per chunk against 5.5 with a staging pass + runtime copy.)

// What a coder thread owns: page-locked rings, so chunks c+1 and c+2 land while chunk c is coded.  Its device->host
// copies go through one of the context's few copy streams: a stream per thread would outnumber the hardware queues,
// and streams that share a hardware queue with a group's kernels have their copies stuck behind those kernels.
struct CoderThread {
    hipStream_t stream = nullptr;                        // one of the context's copy streams
    Event ev[kRingDepth];
    Locked ring;                                         // a lone image's u16 chunks: kRingDepth slots of ring_chunk bins
    Locked pring;                                        // packs: kRingDepth slots of kMaxPacks x pring_groups groups x 13 words x 8 lanes
    Locked whole;                                        // one whole QNBLIC image (its rANS runs last pixel first)
    RangeX8 x8, x8b, x8c;
    RangeScalar x1;
    double wait_s = 0, issue_s = 0;                      // time spent waiting for chunks / inside the runtime calls that queue a chunk (reporting)
    CopyEngine *engine = nullptr;                        // the context's, when the chunks of packs may travel on a DMA engine (copy_engine.h)
    HsaSignal sig[kRingDepth];                           // ... then one completion signal per slot of pring
    EngineLane lane;
    bool init(int device, hipStream_t copy_stream, CopyEngine *eng) {
        HIP_OK(hipSetDevice(device));
        stream = copy_stream;
        for (auto &e : ev) HIP_OK(e.create(hipEventDisableTiming | hipEventBlockingSync));
        if (eng && eng->on()) {
            engine = eng;
            for (int k = 0; k < kRingDepth; k++) {
                if (!sig[k].create(eng->api(), 0)) { eng->fail("hsa_signal_create", -1); break; }
                lane.sig[k] = sig[k].handle();
            }
        }
        return true;
    }
    // The rings are sized by what the thread has actually been asked to code and only grow: a context that codes one
    // small image through the drop-in entry points pins kilobytes, the bench's threads end up at
    // 3 slots x 3 packs x 64 Ki groups x 832 B = 491 MB each.
    size_t ring_chunk = 0, pring_groups = 0;
    bool ensure_ring(size_t chunk) {
        chunk = (chunk + 4095) & ~size_t(4095);
        if (chunk > ring_chunk) {
            ring_chunk = chunk;
            if (!ring.alloc(kRingDepth * ring_chunk)) { ring_chunk = 0; fprintf(stderr, "[nblic_amd] cannot allocate the coder thread's ring\n"); return false; }
        }
        return true;
    }
    size_t pack_words() const { return pring_groups * kGroupWords * kPackLanes; }                 // 64-bit words of one pack in one slot
    bool ensure_pack_ring(size_t groups) {
        groups = (groups + 63) & ~size_t(63);
        if (groups > pring_groups) {
            pring_groups = groups;
            // (with the engine the ring is the runtime's own pinned memory: the engine is given the agent that owns an allocation,
            // and pages registered in place have none -- hip_owned.h Locked on what that costs the reading thread)
            if (!pring.alloc(kRingDepth * size_t(kMaxPacks) * pack_words() * 4, engine != nullptr)) { pring_groups = 0; fprintf(stderr, "[nblic_amd] cannot allocate the coder thread's pack ring\n"); return false; }
        }
        return true;
    }
    uint16_t *slot(size_t chunk) { return ring + size_t(chunk % kRingDepth) * ring_chunk; }
    uint64_t *pack_slot(size_t chunk, int pack) { return reinterpret_cast<uint64_t *>(static_cast<uint16_t *>(pring)) + (size_t(chunk % kRingDepth) * size_t(kMaxPacks) + size_t(pack)) * pack_words(); }
};

// A sleeping poll: hipEventSynchronize spins through the wait (see GroupWait), and CPU time is what the rank is
// short of; a chunk is ~30 ms of coding, so 100 us of extra latency on its arrival is nothing.
// (Measured and rejected: sleeping on a condition variable woken by a host function behind the copy, as the
// driver threads do.  A host function holds its stream until it has run, two threads share a copy stream,
// and the chunks arrived so much later that the threads fell back to packs of eight: 6.1 -> 4.0 Gpx/s.)
static bool wait_chunk(CoderThread &t, hipEvent_t e) {
    const auto w0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(e);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { fprintf(stderr, "[nblic_amd] HIP error: %s\n", hipGetErrorString(q)); return false; }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    t.wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    return true;
}

// One image on its own: its u16 records stream from HBM chunk by chunk into the scalar coder.  *len = coder bytes or SIZE_MAX.
static bool code_single(CoderThread &t, const uint16_t *dev, size_t n, uint8_t *dst, size_t cap, size_t *len, size_t chunk_bins) {
    if (!t.ensure_ring(n < chunk_bins ? n + 4 : chunk_bins)) return false;
    const size_t chunks = (n + chunk_bins - 1) / chunk_bins;                         // chunk_bins <= kChunkBins, the ring's slot size
    auto chunk_len = [&](size_t c) { const size_t off = c * chunk_bins; return off >= n ? size_t(0) : std::min(n - off, chunk_bins); };
    auto issue = [&](size_t c) -> bool {
        HIP_OK(hipMemcpyAsync(t.slot(c), dev + c * chunk_bins, chunk_len(c) * sizeof(uint16_t), hipMemcpyDeviceToHost, t.stream));
        HIP_OK(hipEventRecord(t.ev[c % kRingDepth], t.stream));
        return true;
    };
    t.x1.begin(dst, cap);
    for (size_t c = 0; c + 1 < size_t(kRingDepth) && c < chunks; c++) if (!issue(c)) return false;
    for (size_t c = 0; c < chunks; c++) {
        const auto i0 = std::chrono::steady_clock::now();
        if (c + kRingDepth - 1 < chunks && !issue(c + kRingDepth - 1)) return false;      // its ring slot was consumed one chunk ago
        t.issue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - i0).count();
        if (!wait_chunk(t, t.ev[c % kRingDepth])) return false;
        t.x1.feed(t.slot(c), chunk_len(c));
    }
    *len = t.x1.finish();
    return true;
}

// One to three PACKS: chunk by chunk -- one contiguous copy per pack -- through the AVX-512 coders in lock-step (a lone
// pack is bound by the latency of its own dependent chain, a second one rides along almost for free, a third on what
// the core's ports have left).  n[8 p + lane] = bins of the image in lane `lane` of pack p (0 = no image); dst, caps and
// lens likewise.  pack_n[p] = images of pack p, in lanes 0 .. pack_n[p] - 1.
static bool code_packs(CoderThread &t, int n_packs, const uint64_t *const *dev_rows, const int *pack_n, const size_t *n, uint8_t *const *dst,
                       const size_t *caps, size_t *lens, size_t chunk_bins) {
    size_t groups[kMaxPacks] = {0}, most = 0;
    for (int p = 0; p < n_packs; p++) {
        for (int k = 0; k < pack_n[p]; k++) groups[p] = std::max(groups[p], (n[kPackLanes * p + k] + kGroupBins - 1) / kGroupBins);
        most = std::max(most, groups[p]);
    }
    const size_t chunk_groups = std::min(chunk_bins / kGroupBins, most ? most : size_t(1));
    if (!t.ensure_pack_ring(chunk_groups)) return false;
    const size_t chunks = (most + chunk_groups - 1) / chunk_groups, chunk = chunk_groups * kGroupBins;
    // Who carries a chunk (copy_engine.h run_chunk_ring): a DMA engine while the context's is on -- one
    // hsa_amd_memory_async_copy per pack, the slot's signal counting them down -- and otherwise, or after an engine
    // error, the runtime on the thread's copy stream, which in this pipeline means its blit kernel whatever was tried:
    // ring from hipHostMalloc instead of hipHostRegister, 2 / 4 / 8 copy streams, the copy cut into 8 or 16 MB pieces
    // (DESIGN.md section 4).  The engine reads memory, not L2: the rows were released to the system by the event the
    // group's stream records behind its back half (launch_back).
    struct RuntimeCopies {
        CoderThread &t;
        bool issue(size_t c, const CopyPiece *pc, int n) {
            for (int k = 0; k < n; k++) HIP_OK(hipMemcpyAsync(pc[k].dst, pc[k].src, pc[k].bytes, hipMemcpyDeviceToHost, t.stream));
            HIP_OK(hipEventRecord(t.ev[c % kRingDepth], t.stream));
            return true;
        }
        bool wait(size_t c) { return wait_chunk(t, t.ev[c % kRingDepth]); }
    } runtime{t};
    auto pieces = [&](size_t c, CopyPiece *out) -> int {
        if (dbg_flags() & kDbgNoCopy) return 0;
        return chunk_pieces(c, n_packs, groups, chunk_groups, kGroupWords * kPackLanes, dev_rows, [&](size_t cc, int p) { return t.pack_slot(cc, p); }, out);
    };
    RangeX8 *const packs[kMaxPacks] = {&t.x8, &t.x8b, &t.x8c};
    for (int p = 0; p < n_packs; p++) packs[p]->begin(pack_n[p], dst + kPackLanes * p, caps + kPackLanes * p);
    auto consume = [&](size_t c) {
        size_t len[kMaxTake] = {0};
        const uint64_t *rows_p[kMaxPacks] = {nullptr};
        for (int p = 0; p < n_packs; p++) {
            rows_p[p] = t.pack_slot(c, p);
            for (int k = 0; k < pack_n[p]; k++) {
                const size_t all = n[kPackLanes * p + k], off = c * chunk;
                len[kPackLanes * p + k] = off >= all ? 0 : std::min(chunk, all - off);
            }
        }
        if (!(dbg_flags() & kDbgFeedOnly)) feed_packs(packs, n_packs, rows_p, len);
    };
    if (!run_chunk_ring(t.engine, t.lane, chunks, runtime, pieces, consume, &t.issue_s, &t.wait_s)) return false;
    for (int p = 0; p < n_packs; p++) packs[p]->end(lens + kPackLanes * p);
    return true;
}

// Coder thread.  Measured on the GPU box (EPYC 9575F), per thread: one stream alone 400-510 Mbins/s; one pack of eight
// 1300, two packs in lock-step 1950-2000, three 2200-2400 -- at 2.5x / 3.4x the latency of a stream coded alone.  The
// host's CPU share (16 cores, enforced as a quota) is dear, so what counts is bins per CPU-second.  What a thread takes:
//   packs at the front of the queue: as many whole packs as are there, up to three (max_take / 8).  Mid-batch (images
//       still to come, and at least four per thread outstanding) it waits for a full set -- the ~30-45 ms it takes for
//       three to be queued -- when every other thread is busy, and for at least two while others are idle too (the
//       start of a batch, or the GPU side not keeping up): a lone pack costs twice the CPU time per bin.  At the tail it
//       takes what is there.  A wait ends when something that is not a pack follows the packs at the front.
//   an image on its own: that image (the scalar coder).  Whether an image is packed is decided when its group is
//       launched (launch_back).
// (Alternatives ranked with a discrete-event model of arrivals and coder speeds, tools/coder_policy_sim.py, then in situ.)
static int coder_take(const nblic_amd_ctx *c) {                  // call with c->rm held; 0 = nothing to take; else the number of IMAGES
    const size_t q = c->ready.size();
    if (q == 0) return 0;
    const ReadyImage &f = c->ready.front();
    if (f.kind == 1) return c->qmode == 1 ? 0 : 1;               // device mode: the device-qcoder thread takes it (and wakes the coders when it has)
    if (f.pack_n <= 1) return 1;
    const int max_packs = std::max(1, c->max_take / int(kPackLanes));
    int packs = 0; size_t imgs = 0;
    bool more_may_join = true;
    for (size_t i = 0; i < q && packs < max_packs;) {            // whole packs at the front (a pack is queued in one piece, lane 0 first)
        const ReadyImage &r = c->ready[i];
        if (r.kind == 1 || r.pack_n <= 1) { more_may_join = false; break; }
        imgs += size_t(r.pack_n); i += size_t(r.pack_n); packs++;
    }
    const size_t left = q + size_t(c->batch_to_come), threads = c->coders.size();
    if (more_may_join && c->batch_to_come > 0 && left >= 4 * threads) {
        const int want = c->idle_coders <= 1 ? max_packs : std::min(max_packs, 2);
        if (packs < want) return 0;
    }
    return int(imgs);
}

// One logical CPU per physical core of the process's affinity mask (the lowest-numbered sibling that is allowed).
// NBLIC_AMD_PIN=1 pins coder thread i to core i of the mask (when there are enough cores), so that two coders --
// each a dependent chain per AVX-512 lane that keeps its core's vector unit busy by itself -- never share the SMT
// siblings of one core.  Off by default: measured on the GPU box, alternating runs, 5712 / 5356 Mpx/s pinned against
// 5642 / 5642 left to the scheduler -- a pinned thread cannot step aside when a driver or runtime thread is put on
// its CPU, and under the box's CPU quota that costs as much as the pinning saves.
static std::vector<int> primary_cpus() {
    std::vector<int> out;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) != 0) return out;
    std::vector<int> cores;
    for (int cpu = 0; cpu < CPU_SETSIZE; cpu++) {
        if (!CPU_ISSET(cpu, &set)) continue;
        char path[96];
        snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", cpu);
        int first = cpu;
        if (FILE *f = fopen(path, "r")) { if (fscanf(f, "%d", &first) != 1) first = cpu; fclose(f); }
        if (std::find(cores.begin(), cores.end(), first) == cores.end()) { cores.push_back(first); out.push_back(cpu); }
    }
    return out;
}

static void coder_main(nblic_amd_ctx *c, int index) {
    pthread_setname_np(pthread_self(), "nblic-coder");         // (thread names: who uses the rank's CPU share, tools/thread_cpu.py)
    {
        static const std::vector<int> cpus = primary_cpus();
        static const bool pin = getenv("NBLIC_AMD_PIN") && atoi(getenv("NBLIC_AMD_PIN")) != 0;
        static const int pin_raw = getenv("NBLIC_AMD_PIN") ? atoi(getenv("NBLIC_AMD_PIN")) : 0;
        if (pin_raw >= 100) {                                     // experiment: coder i on logical CPU (pin_raw - 100) + i, whatever the process's mask
            cpu_set_t one;
            CPU_ZERO(&one);
            CPU_SET(pin_raw - 100 + index, &one);
            pthread_setaffinity_np(pthread_self(), sizeof one, &one);
        } else if (pin && c->coders_wanted > 1 && cpus.size() >= size_t(c->coders_wanted)) {
            cpu_set_t one;
            CPU_ZERO(&one);
            static std::atomic<unsigned> next_core{0};            // across contexts: a second context's threads take the next cores
            CPU_SET(cpus[size_t(next_core++ % cpus.size())], &one);
            pthread_setaffinity_np(pthread_self(), sizeof one, &one);
        }
    }
    CoderThread t;
    if (!t.init(c->device, c->copy_streams[size_t(index) % c->copy_streams.size()], &c->engine)) c->broken = true;
    for (;;) {
        ReadyImage im[kMaxTake];
        int take = 0;
        {
            std::unique_lock<std::mutex> l(c->rm);
            c->idle_coders++;
            c->rcv.wait(l, [c] { return c->stop || coder_take(c) > 0; });
            if (c->ready.empty()) break;
            take = coder_take(c);
            if (take == 0) break;                                // shutdown while waiting for a pack to fill
            c->idle_coders--;
            for (int k = 0; k < take; k++) { im[k] = c->ready.front(); c->ready.pop_front(); }
        }
        if (im[0].kind == 1) {                               // QNBLIC: histogram normalisation + rANS, one image per thread
            const ReadyImage &q = im[0];
            const size_t n = size_t(q.h) * size_t(q.w), n_pad = (n + 1) & ~size_t(1), words = n_pad + 2 * 12 * 256;
            bool ok = true;
            if (t.whole.capacity() < words) ok = t.whole.alloc(words + 1024);
            ok = ok && hipMemcpyAsync(t.whole, c->cbufs[size_t(q.cb)], words * sizeof(uint16_t), hipMemcpyDeviceToHost, t.stream) == hipSuccess &&
                 hipEventRecord(t.ev[0], t.stream) == hipSuccess && hipEventSynchronize(t.ev[0]) == hipSuccess;
            long words_out = -1;
            if (ok) {
                const uint32_t *hist = reinterpret_cast<const uint32_t *>(t.whole + n_pad);
                words_out = q_entropy_encode(reinterpret_cast<uint16_t *>(q.outs[q.job]), q.caps[q.job], q.h, q.w, t.whole, hist);
                if (words_out < 0) fprintf(stderr, "[nblic_amd] image %d: output buffer of %zu words is too small\n", q.job, q.caps[q.job]);
            }
            q.lens[q.job] = words_out;                           // -1: the batch this image belongs to reports the failure
            finish_images(c, im, 1);
            continue;
        }
        auto t0 = std::chrono::steady_clock::now();
        if (c->trace) fprintf(stderr, "[trace] %.3f coder %d takes %d\n", c->now(), index, take);
        size_t n[kMaxTake] = {0}, caps[kMaxTake] = {0}, lens[kMaxTake] = {0}; uint8_t *dst[kMaxTake] = {nullptr};
        int at[kMaxTake];                                        // image k of the take sits at at[k] of the arrays above: 8 p + lane for packs, 0 for an image on its own
        const uint64_t *rows[kMaxPacks] = {nullptr}; int pack_n[kMaxPacks] = {0};
        int n_packs = 0;
        double bins = 0;
        for (int k = 0; k < take; k++) {
            if (im[k].pack_n > 1 && im[k].pack_lane == 0) { rows[n_packs] = c->pbufs[size_t(im[k].cb)].get(); pack_n[n_packs] = im[k].pack_n; n_packs++; }
            at[k] = im[k].pack_n > 1 ? int(kPackLanes) * (n_packs - 1) + im[k].pack_lane : 0;
            n[at[k]] = im[k].n_ev; bins += double(im[k].n_ev);
            dst[at[k]] = begin_stream_out(im[k], &caps[at[k]]);
        }
        bool ok = true;
        if (dbg_flags() & kDbgDeviceOnly) {}
        else if (n_packs > 0) ok = code_packs(t, n_packs, rows, pack_n, n, dst, caps, lens, c->chunk_bins);
        else ok = code_single(t, c->cbufs[size_t(im[0].cb)], n[0], dst[0], caps[0], &lens[0], c->chunk_bins);
        if (!ok) {
            hipDeviceSynchronize();
            for (int k = 0; k < take; k++) lens[at[k]] = SIZE_MAX;
        }
        for (int k = 0; k < take; k++) {
            const size_t l = lens[at[k]];
            if (l == SIZE_MAX) fprintf(stderr, "[nblic_amd] image %d: output buffer of %zu bytes is too small\n", im[k].job, im[k].caps[im[k].job]);
            im[k].lens[im[k].job] = l == SIZE_MAX ? -1 : long(kHeaderBytes + l);
        }
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (c->trace) fprintf(stderr, "[trace] %.3f coder %d finished %d in %.3f s\n", c->now(), index, take, dt);
        { std::lock_guard<std::mutex> l(c->stat_m); c->total_bins += bins; c->coder_s += dt; if (take > 1) { c->pack_bins += bins; c->pack_s += dt; } c->wait_s += t.wait_s; t.wait_s = 0; c->issue_s += t.issue_s; t.issue_s = 0; c->takes[take]++; }
        finish_images(c, im, take);
    }
}

// ---- device coder pack threads -----------------------------------------------------------------
// A pack thread waits until the queue holds a full pack BEYOND what the host coder threads can take
// at once (they keep priority: a host core codes an image forty times faster than a lane) and until
// enough work is outstanding that the pack's latency (seconds) cannot become the tail of the batch;
// then it hands up to 64 images to one wave, sleeps in a blocking stream wait, copies the coder bytes
// to the callers' buffers and completes the images exactly as a host coder thread does.
constexpr int kDevPack = 64;
// Symbols a launch of the device rANS stage (q_device_coder.hip) advances a job by when the caller names none: what a
// lane codes in about 10 ms.  Measured (profiles/r21_device_qcoder_ab.json): 2.9-3.3 M symbols/s per lane, 20-22 ms per
// launch of 65536 symbols, whether 64 or 2048 lanes are live.
constexpr uint32_t kQSymbolsPerLaunch = 1u << 15;

static int dev_take(const nblic_amd_ctx *c) {                  // call with c->rm held
    const size_t q = c->ready.size();
    const size_t reserve = c->simd ? c->coders.size() * size_t(kMaxTake) / 2 : c->coders.size();
    if (q < size_t(kDevPack) + reserve) return 0;
    if (int(q) + c->batch_to_come + c->queued_images < c->dev_min_outstanding) return 0;
    // whole units from the back of the queue -- an image on its own, or a pack, which is queued in one piece and whose
    // buffer goes back with all of its lanes -- as many as fit a wave's 64 lanes
    size_t i = q; int n = 0;
    while (i > 0) {
        const ReadyImage &r = c->ready[i - 1];
        if (r.kind == 1) return 0;                               // QNBLIC images are host work
        const int unit = r.pack_n > 1 ? r.pack_n : 1;
        if (n + unit > kDevPack) break;
        n += unit; i -= size_t(unit);
    }
    return n;
}

static void dev_coder_main(nblic_amd_ctx *c, int index) {
    pthread_setname_np(pthread_self(), "nblic-devcoder");
    (void)index;
    Stream st;
    Event done;
    Pinned<RcJob> h_jobs; DevBuf<RcJob> d_jobs;
    Pinned<uint32_t> h_lens; DevBuf<uint32_t> d_lens;
    DevBuf<uint8_t> d_out;
    bool ok = hipSetDevice(c->device) == hipSuccess && st.create(hipStreamNonBlocking) == hipSuccess &&
              done.create(hipEventDisableTiming | hipEventBlockingSync) == hipSuccess &&
              h_jobs.alloc(kDevPack) == hipSuccess && d_jobs.alloc(kDevPack) == hipSuccess &&
              h_lens.alloc(kDevPack) == hipSuccess && d_lens.alloc(kDevPack) == hipSuccess;
    if (!ok) c->broken = true;
    for (;;) {
        ReadyImage im[kDevPack];
        int take = 0;
        {
            std::unique_lock<std::mutex> l(c->rm);
            c->rcv.wait(l, [c] { return c->stop || dev_take(c) > 0; });
            if (c->stop) break;
            take = dev_take(c);
            for (int k = 0; k < take; k++) { im[k] = c->ready.back(); c->ready.pop_back(); }   // the NEWEST images: the oldest are the host threads' next packs
        }
        if (take == 0) continue;
        // output slots on the device: worst case seen is 1.0025 B/px + 20
        size_t need = 0, off[kDevPack];
        for (int k = 0; k < take; k++) { off[k] = need; need += (size_t(im[k].h) * size_t(im[k].w) * 9 / 8 + 4096 + 255) & ~size_t(255); }
        bool good = ok;
        good = good && d_out.reserve(need) == hipSuccess;
        double bins = 0;
        uint8_t *dst[kDevPack];
        for (int k = 0; k < take && good; k++) {
            size_t room;
            dst[k] = begin_stream_out(im[k], &room);
            const size_t cap = std::min(room, (k + 1 < take ? off[k + 1] : need) - off[k]);
            const bool packed = im[k].pack_n > 1;                // a lane of a pack: read from the pack's rows
            h_jobs[k] = RcJob{packed ? nullptr : c->cbufs[size_t(im[k].cb)].get(), packed ? c->pbufs[size_t(im[k].cb)].get() : nullptr, uint32_t(im[k].pack_lane),
                              d_out + off[k], d_lens + k, im[k].n_ev, uint32_t(cap < 0xFFFFFFF0u ? cap : 0xFFFFFFF0u)};
            bins += double(im[k].n_ev);
        }
        good = good && hipMemcpyAsync(d_jobs, h_jobs, size_t(take) * sizeof(RcJob), hipMemcpyHostToDevice, st) == hipSuccess &&
               device_range_code(d_jobs, take, st) &&
               hipMemcpyAsync(h_lens, d_lens, size_t(take) * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
               hipEventRecord(done, st) == hipSuccess && hipEventSynchronize(done) == hipSuccess;
        for (int k = 0; k < take; k++) {
            long len = -1;
            if (good && h_lens[k] != 0xFFFFFFFFu) {
                if (hipMemcpyAsync(dst[k], d_out + off[k], h_lens[k], hipMemcpyDeviceToHost, st) == hipSuccess) len = long(kHeaderBytes) + long(h_lens[k]);
            } else if (good) {
                fprintf(stderr, "[nblic_amd] image %d: output buffer of %zu bytes is too small\n", im[k].job, im[k].caps[im[k].job]);
            }
            im[k].lens[im[k].job] = len;
        }
        if (hipStreamSynchronize(st) != hipSuccess) good = false;
        if (!good) { for (int k = 0; k < take; k++) im[k].lens[im[k].job] = -1; }
        { std::lock_guard<std::mutex> l(c->stat_m); c->dev_bins += bins; c->dev_packs++; c->dev_images += take; }
        finish_images(c, im, take);
    }
}

// ---- device-qcoder thread: QNBLIC's rANS pass on the GPU (q_device_coder.hip) ---------------------------------------------
// One thread per context, one stream.  Every launch of k_q_rans_lanes holds a wave per 64 images for its whole
// duration, so launches are bounded (q_budget symbols per job) and there is no hand-out of packs: the thread keeps a
// ROLLING list of job slots whose records stay in device memory.  Per turn it admits what its mode lets it take, reads
// each newcomer's raw histogram back (12 KB), runs the front matter on the host straight into the caller's buffer,
// uploads the table and the record, launches over all slots up to the highest live one, reads one word per slot back,
// retires the finished jobs (their words are copied behind the front matter, the coded-bin buffer goes back) and goes
// round again.  While nobody waits to be admitted TWO launches are queued per wait (kQAhead): the job set is the same
// for both, and a job that the first one finishes is an idle lane in the second.
// The words are written IN PLACE, downwards from the end of the image's coded-bin buffer (pairs | pad | raw histogram):
// a pass never emits more words than it has consumed symbols, so the words stay above every symbol still to be read,
// and the histogram they overwrite was read back before the first launch.
constexpr int kQAhead = 2;
constexpr size_t kQHistWords = 2 * 12 * 256;                     // the raw histogram in 16-bit words (launch_q)

static int qdev_take(const nblic_amd_ctx *c) {                  // call with c->rm held: how many QNBLIC images the thread may take now
    int q = 0;
    if (c->qmode == 1) { for (const ReadyImage &r : c->ready) q += r.kind == 1; return q; }
    if (c->qmode != 2 || c->idle_coders > 0) return 0;          // shared: only while no host coder thread is idle,
    size_t i = c->ready.size();                                  //   the newest ones, and one image per host thread stays
    while (i > c->coders.size() && c->ready[i - 1].kind == 1) { i--; q++; }
    return q;
}

static void qdev_main(nblic_amd_ctx *c) {
    pthread_setname_np(pthread_self(), "nblic-qdevcoder");
    struct LiveJob { ReadyImage im; long front = 0; bool used = false; };
    const size_t slots = (c->cbufs.size() + 63) & ~size_t(63);  // an image in flight holds a coded-bin buffer: never more jobs than buffers
    Stream st; Event t0, t1;
    DevBuf<QRansJob> d_jobs; DevBuf<uint32_t> d_tables, d_results;
    Pinned<QRansJob> h_jobs; Pinned<uint32_t> h_tables, h_results, h_hist;
    std::vector<LiveJob> live(slots);
    std::vector<uint32_t> freq(kQRansTable), start(kQRansTable);
    bool ok = hipSetDevice(c->device) == hipSuccess && st.create(hipStreamNonBlocking) == hipSuccess &&
              t0.create(hipEventDefault) == hipSuccess && t1.create(hipEventDefault) == hipSuccess &&
              d_jobs.alloc(slots) == hipSuccess && d_tables.alloc(slots * kQRansTable) == hipSuccess && d_results.alloc(slots) == hipSuccess &&
              h_jobs.alloc(slots) == hipSuccess && h_tables.alloc(slots * kQRansTable) == hipSuccess && h_results.alloc(slots) == hipSuccess &&
              h_hist.alloc(slots * kQRansTable) == hipSuccess &&
              hipMemset(d_jobs, 0, slots * sizeof(QRansJob)) == hipSuccess;          // live == 0: every slot empty
    if (!ok) { fprintf(stderr, "[nblic_amd] device qcoder: could not set itself up (%s)\n", hipGetErrorString(hipGetLastError())); c->broken = true; }
    size_t n_live = 0;
    for (;;) {
        std::vector<size_t> fresh;
        bool more_waiting = false;
        uint32_t budget;
        {
            std::unique_lock<std::mutex> l(c->rm);
            if (n_live == 0) c->rcv.wait(l, [c] { return c->stop || qdev_take(c) > 0; });
            if (c->stop && n_live == 0) break;
            int take = qdev_take(c);
            budget = c->q_budget ? c->q_budget : kQSymbolsPerLaunch;
            size_t slot = 0;
            for (size_t i = c->ready.size(); i-- > 0 && take > 0;) {            // from the back: the newest
                if (c->ready[i].kind != 1) continue;
                while (slot < slots && live[slot].used) slot++;
                if (slot == slots) break;
                live[slot].im = c->ready[i]; live[slot].used = true; live[slot].front = 0;
                c->ready.erase(c->ready.begin() + long(i));
                fresh.push_back(slot); take--;
            }
            more_waiting = c->batch_to_come > 0 || c->queued_images > 0;       // newcomers may arrive during the next launch
        }
        if (!fresh.empty()) c->rcv.notify_all();                                 // a coder thread may find its kind of image at the front now
        n_live += fresh.size();
        bool good = ok;
        // front matter of the newcomers: raw histograms back, scaled and coded on the host, tables and records up
        for (size_t slot : fresh) {
            const ReadyImage &q = live[slot].im;
            const size_t n = size_t(q.h) * size_t(q.w), n_pad = (n + 1) & ~size_t(1);
            good = good && hipMemcpyAsync(h_hist + slot * kQRansTable, c->cbufs[size_t(q.cb)] + n_pad, kQRansTable * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
        }
        if (!fresh.empty()) good = hipStreamSynchronize(st) == hipSuccess && good;
        for (size_t slot : fresh) {
            LiveJob &L = live[slot];
            const ReadyImage &q = L.im;
            const size_t n = size_t(q.h) * size_t(q.w), n_pad = (n + 1) & ~size_t(1);
            L.front = good ? q_entropy_front(reinterpret_cast<uint16_t *>(q.outs[q.job]), q.caps[q.job], q.h, q.w, h_hist + slot * kQRansTable, freq.data(), start.data()) : -1;
            if (L.front < 0) continue;                                           // no room for the front matter (or a failure): retired below, never launched
            q_rans_table(freq.data(), start.data(), h_tables + slot * kQRansTable);
            QRansJob &J = h_jobs[slot];
            uint16_t *const buf = c->cbufs[size_t(q.cb)];
            J.words = buf; J.table = d_tables + slot * kQRansTable; J.out_end = buf + n_pad + kQHistWords; J.result = d_results + slot;
            J.cap = uint32_t(std::min<size_t>(q.caps[q.job] - size_t(L.front), 0xFFFFFFF0u));
            J.live = 1u;
            q_rans_begin(J.st, uint32_t(n), J.cap);
            h_results[slot] = 0u;
            good = good && hipMemcpyAsync(d_tables + slot * kQRansTable, h_tables + slot * kQRansTable, kQRansTable * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess &&
                   hipMemcpyAsync(d_results + slot, h_results + slot, sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess &&
                   hipMemcpyAsync(d_jobs + slot, h_jobs + slot, sizeof(QRansJob), hipMemcpyHostToDevice, st) == hipSuccess;
        }
        size_t top = 0;
        for (size_t k = 0; k < slots; k++) if (live[k].used) top = k + 1;
        const int launches = more_waiting ? 1 : kQAhead;
        float ms = 0.f;
        good = good && hipEventRecord(t0, st) == hipSuccess;
        for (int k = 0; good && k < launches; k++) good = device_q_rans(d_jobs, int(top), budget, st);
        good = good && hipEventRecord(t1, st) == hipSuccess &&
               hipMemcpyAsync(h_results, d_results, top * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
        good = hipStreamSynchronize(st) == hipSuccess && good;
        if (good && hipEventElapsedTime(&ms, t0, t1) != hipSuccess) ms = 0.f;
        // retire: finished jobs, jobs without room for their front matter, and after a failure every job
        std::vector<size_t> gone;
        double symbols = 0;
        for (size_t k = 0; k < top; k++) {
            LiveJob &L = live[k];
            if (!L.used) continue;
            const ReadyImage &q = L.im;
            const uint32_t r = good && L.front >= 0 ? h_results[k] : 0xFFFFFFFFu;
            if (r == 0u) continue;                                               // still coding
            const size_t n = size_t(q.h) * size_t(q.w), n_pad = (n + 1) & ~size_t(1);
            long len = -1;
            if (r != 0xFFFFFFFFu && hipMemcpyAsync(reinterpret_cast<uint16_t *>(q.outs[q.job]) + L.front, c->cbufs[size_t(q.cb)] + n_pad + kQHistWords - r,
                                                   size_t(r) * sizeof(uint16_t), hipMemcpyDeviceToHost, st) == hipSuccess) len = L.front + long(r);
            else if (good) fprintf(stderr, "[nblic_amd] image %d: output buffer of %zu words is too small\n", q.job, q.caps[q.job]);
            q.lens[q.job] = len;
            symbols += double(n);
            gone.push_back(k);
        }
        if (!gone.empty() && hipStreamSynchronize(st) != hipSuccess) { for (size_t k : gone) live[k].im.lens[live[k].im.job] = -1; good = false; }
        if (!good) fprintf(stderr, "[nblic_amd] device qcoder: a turn failed (%s): %zu images report -1\n", hipGetErrorString(hipGetLastError()), gone.size());
        if (!good && ok) {                                                      // the slots' records on the device are of no use any more
            if (hipMemset(d_jobs, 0, slots * sizeof(QRansJob)) != hipSuccess) { ok = false; c->broken = true; }
        }
        { std::lock_guard<std::mutex> l(c->stat_m); c->qdev_symbols += symbols; c->qdev_launches += good ? launches : 0; c->qdev_images += long(gone.size()); c->qdev_kernel_ms += double(ms); }
        for (size_t k : gone) { finish_images(c, &live[k].im, 1); live[k].used = false; }
        n_live -= gone.size();
    }
}

// Takes a coded-bin buffer of at least `words` for slot s (waits for one if the coder threads are
// behind: that is the pipeline's back-pressure).
static bool acquire_coded(nblic_amd_ctx *c, Slot &s, size_t words) {
    {
        std::unique_lock<std::mutex> l(c->fm);
        c->fcv.wait(l, [c] { return !c->free_cbufs.empty(); });
        s.cb = c->free_cbufs.front(); c->free_cbufs.pop_front();
    }
    CodedBuf &cb = c->cbufs[size_t(s.cb)];
    if (cb.capacity() < words) HIP_OK(cb.alloc(words + words / 8 + 1024));
    return true;
}

// Takes a buffer for the rows of one pack whose longest image has max_ev bins (waits like acquire_coded).
static bool acquire_pack(nblic_amd_ctx *c, int *id, size_t max_ev) {
    {
        std::unique_lock<std::mutex> l(c->fm);
        c->fcv.wait(l, [c] { return !c->free_pbufs.empty(); });
        *id = c->free_pbufs.front(); c->free_pbufs.pop_front();
    }
    HIP_OK(c->pbufs[size_t(*id)].reserve_bins(max_ev));
    return true;
}

// Runs on a HIP runtime thread when the group's kernels have finished: queues the images for the
// coder threads and hands the device workspace back.  (No HIP calls in here.)
static void on_group_done(void *vp) {
    Group *gp = static_cast<Group *>(vp);
    nblic_amd_ctx *c = gp->ctx;
    if (c->trace) fprintf(stderr, "[trace] %.3f group %d done (%d images)\n", c->now(), gp->id, gp->n_jobs);
    if (gp->kind == 1) for (int k = 0; k < gp->n_jobs; k++) count_long_chains(c, gp->h_totals + size_t(k) * kTotalsSlot);   // (NBLIC: launch_back has)
    {
        std::lock_guard<std::mutex> l(c->rm);
        for (int k = 0; k < gp->n_jobs; k++) {
            const Slot &s = gp->slots[size_t(k)];
            c->ready.push_back(ReadyImage{s.cb, s.job, s.h, s.w, s.n_ev, gp->outs, gp->caps, gp->lens, gp->kind, gp->batch, s.near, k_step_for_near(s.near), s.effort, s.pack_n, s.pack_lane});
        }
        c->batch_to_come -= gp->n_jobs;
    }
    c->rcv.notify_all();
    release_group(c, gp->id);
}

static double thread_cpu_s();
static bool launch_back(nblic_amd_ctx *c, Group &g, bool with_coders, bool general = false, bool force_pack = false) {
    // a BLOCKING wait: a spinning one per driver thread would take cores from the coder threads
    const double w0 = thread_cpu_s();
    { std::lock_guard<std::mutex> l(g.front->m); g.front->ready = false; }
    HIP_OK(hipLaunchHostFunc(g.stream, [](void *p) {
        GroupWait *w = static_cast<GroupWait *>(p);
        { std::lock_guard<std::mutex> l(w->m); w->ready = true; }
        w->cv.notify_one();
    }, g.front.get()));
    {   // a sleep, but not an unconditional one: if the stream has faulted the host function may never run
        std::unique_lock<std::mutex> l(g.front->m);
        while (!g.front->cv.wait_for(l, std::chrono::milliseconds(50), [&] { return g.front->ready; })) {
            l.unlock();
            const hipError_t q = hipStreamQuery(g.stream);
            l.lock();
            if (q != hipSuccess && q != hipErrorNotReady) { fprintf(stderr, "[nblic_amd] group %d: %s while waiting for the front half\n", g.id, hipGetErrorString(q)); return false; }
        }
    }
    { std::lock_guard<std::mutex> l(c->stat_m); c->driver_wait_cpu_s += thread_cpu_s() - w0; }
    for (int k = 0; k < g.n_jobs; k++) {
        Slot &s = g.slots[size_t(k)];
        s.n_ev = g.h_totals[size_t(k) * kTotalsSlot + 2];
        count_long_chains(c, g.h_totals + size_t(k) * kTotalsSlot);
        s.pack_n = 1; s.pack_lane = 0;
        if (s.n_ev >= 0x7FFFFFFFu) { fprintf(stderr, "[nblic_amd] event count overflow\n"); return false; }
        if (!ensure_events(s, s.n_ev)) return false;
    }
    // Packs: up to eight consecutive jobs of the launch are coded together by one AVX-512 register of a coder thread
    // (E1Job::pack_rows).  Not packed: a job on its own; hosts without AVX-512; and everything launched while at most two images per coder thread are outstanding -- queued,
    // in flight on the GPU (this launch included) or still to be submitted: the tail of a batch or a short batch, where
    // an image per thread finishes sooner than a pack per thread.
    bool packing = force_pack || (with_coders && c->simd && g.n_jobs >= 2);      // force_pack: the layout hook (nblic_amd_debug_pack_rows)
    if (packing && !force_pack) {
        std::lock_guard<std::mutex> l(c->rm);
        packing = c->ready.size() + size_t(c->batch_to_come) + size_t(c->queued_images) > 2 * c->coders.size();
    }
    for (int k0 = 0; k0 < g.n_jobs; k0 += int(kPackLanes)) {
        const int cnt = std::min(int(kPackLanes), g.n_jobs - k0);
        int pack_id = -1;
        if (packing && cnt >= 2) {
            size_t max_ev = 0;
            for (int k = k0; k < k0 + cnt; k++) max_ev = std::max(max_ev, size_t(g.slots[size_t(k)].n_ev));
            if (!acquire_pack(c, &pack_id, max_ev)) {            // the buffer is taken, its memory is not there: hand it back
                if (pack_id >= 0) { std::lock_guard<std::mutex> l(c->fm); c->free_pbufs.push_front(pack_id); }
                return false;
            }
        }
        for (int k = k0; k < k0 + cnt; k++) {
            Slot &s = g.slots[size_t(k)];
            if (pack_id >= 0) {
                s.cb = pack_id; s.pack_n = cnt; s.pack_lane = k - k0;
                s.b.coded = nullptr;
            } else {
                // the coded bins go straight into a pool buffer that outlives this group's turn on the slot
                if (!acquire_coded(c, s, size_t(s.n_ev) + 8)) return false;
                s.b.coded = c->cbufs[size_t(s.cb)];
            }
            e1_job_back(g.h_jobs[k], s.b, s.n_ev, pack_id >= 0 ? c->pbufs[size_t(pack_id)].get() : nullptr, s.pack_lane);
        }
    }
    HIP_OK(hipMemcpyAsync(g.d_jobs, g.h_jobs, size_t(g.n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, g.stream));
    e1_launch_back(g.d_jobs, g.h_jobs, g.n_jobs, g.stream, (c->timing && !general) ? &g.tm : nullptr, general);
    g.tm_pending = c->timing && !general;
    // A pack becomes takeable in on_group_done.  Its reader may be a DMA engine, which reads memory and not L2: the rows
    // k_mix and k_pack_rows wrote are released at system scope HERE, by this event, not by whatever the host function does.
    if (with_coders && c->engine.available()) HIP_OK(hipEventRecord(g.released, g.stream));
    if (with_coders) HIP_OK(hipLaunchHostFunc(g.stream, on_group_done, &g));       // the caller has counted the images in ctx->coding
    return true;
}

static void collect_timing(nblic_amd_ctx *c, Group &g) {
    if (!g.tm_pending) return;
    g.tm_pending = false;
    int last = -1;
    for (int k = 0; k < kE1Kernels; k++) if ((g.tm.mask >> k) & 1ull) last = k;
    if (last < 0 || hipEventSynchronize(g.tm.ev[last + 1]) != hipSuccess) return;
    for (int k = 0; k < kE1Kernels; k++) {
        float ms = 0.f;
        if (((g.tm.mask >> k) & 1ull) && hipEventElapsedTime(&ms, g.tm.ev[k], g.tm.ev[k + 1]) == hipSuccess) c->stage_ms[k] += ms;
    }
    c->stage_launches++;
}

static bool launch_q(nblic_amd_ctx *c, Group &g, const uint8_t *const *imgs, bool on_device, const CollectFrom *from);

static double thread_cpu_s() {
    timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return double(ts.tv_sec) + 1e-9 * double(ts.tv_nsec);
}

static void driver_main(nblic_amd_ctx *c, int id) {
    pthread_setname_np(pthread_self(), "nblic-driver");
    Group &g = c->groups[size_t(id)];
    if (hipSetDevice(c->device) != hipSuccess) fprintf(stderr, "[nblic_amd] driver thread: cannot select device %d\n", c->device);
    for (;;) {
        {
            std::unique_lock<std::mutex> l(c->dm);
            c->dcv.wait(l, [&] { return c->stop_drivers || g.has_work; });
            if (!g.has_work) return;
            g.has_work = false;
        }
        const double cpu0 = thread_cpu_s();
        const bool ok = g.kind == 0 ? (launch_front(c, g, g.imgs, g.on_device, g.from) && launch_back(c, g, true))
                      : g.kind == 2 ? (launch_front_serial(c, g, g.imgs, g.on_device, g.from) && launch_back(c, g, true, true))
                                    : launch_q(c, g, g.imgs, g.on_device, g.from);
        { std::lock_guard<std::mutex> l(c->stat_m); c->driver_cpu_s += thread_cpu_s() - cpu0; c->driver_launches++; }
        if (!ok) {
            hipStreamSynchronize(g.stream);
            for (int k = 0; k < g.n_jobs; k++) return_coded(c, g.slots[size_t(k)]);   // what the failed launch had already taken
            { std::lock_guard<std::mutex> l(c->rm); c->batch_to_come -= g.n_jobs; }
            c->rcv.notify_all();                                 // a pack may be waiting for images that will not come
            { std::lock_guard<std::mutex> l(c->fm); c->coding -= g.n_jobs; g.batch->remaining -= g.n_jobs; g.batch->ok = false; }
            release_group(c, id);
        }
    }
}

// The images are counted as outstanding BEFORE the driver thread is woken, so the batch's final
// wait cannot slip through between the hand-over and the launch.
static void start_group(nblic_amd_ctx *c, Group &g, const uint8_t *const *imgs, bool on_device, const CollectFrom *from) {
    { std::lock_guard<std::mutex> l(c->fm); c->coding += g.n_jobs; g.batch->remaining += g.n_jobs; }
    { std::lock_guard<std::mutex> l(c->dm); g.imgs = imgs; g.on_device = on_device; g.from = from; g.has_work = true; }
    c->dcv.notify_all();
}

// Groups are started one after the other and run concurrently on the GPU (a stream each); the
// host codes finished groups while the GPU is busy with the following ones.
// Submission half of a batch: hands the images to the groups (blocks only while all groups are
// busy, i.e. until the GPU is down to its last few groups of this batch).  The coder threads and the
// groups still in flight finish on their own; encode_wait() collects.  Several batches may be
// outstanding: the next one fills the pipeline while this one drains.
static void encode_submit(nblic_amd_ctx *c, const nblic_amd_ctx::SubmitItem &it) {
    nblic_amd_batch *const b = it.b;
    if (nothing_outstanding(c)) {                                 // start the reporting afresh
        for (auto &gr : c->groups) gr.tm_pending = false;         // (timer events of earlier batches that nobody collected belong to THEIR figures, not to this batch's)
        for (auto &v : c->stage_ms) v = 0;
        c->stage_launches = 0;
        c->total_bins = 0; c->coder_s = 0; c->pack_bins = 0; c->pack_s = 0; c->wait_s = 0; c->issue_s = 0; c->driver_cpu_s = 0; c->driver_wait_cpu_s = 0; c->driver_launches = 0; for (auto &v : c->takes) v = 0;
        c->dev_bins = 0; c->dev_packs = 0; c->dev_images = 0;
        c->t_batch = std::chrono::steady_clock::now();
    }
    b->n_images = it.n; b->lens = it.lens;
    for (int k = 0; k < it.n; k++) it.lens[k] = -1;
    // modes: (near, effort) clamped as the reference clamps them (NBLIC.c:768-770); -n0 -e1 images take the
    // staged pipeline (kind 0), everything else the serial model stage (kind 2); a QNBLIC batch is one class of its
    // own (kind 1).  Images are handed out kind by kind and, inside kind 2, effort by effort, so a group's launches
    // are homogeneous.
    auto near_of = [&](int k) { return it.nears ? iclip(it.nears[k], 0, kMaxNear) : 0; };
    auto effort_of = [&](int k) { return it.efforts ? iclip(it.efforts[k], 1, 3) : 1; };
    auto class_of = [&](int k) { return it.kind == 1 ? 4 : (near_of(k) == 0 && effort_of(k) == 1) ? 0 : effort_of(k); };   // 0 staged; 1..3 serial by effort; 4 QNBLIC
    auto kind_of = [&](int k) { const int cls = class_of(k); return cls == 0 ? 0 : (cls == 4 ? 1 : 2); };
    std::vector<int> order;
    order.reserve(size_t(it.n));
    for (int cls = 0; cls <= 4; cls++)
        for (int k = 0; k < it.n; k++) {
            if (class_of(k) != cls) continue;
            if (!size_ok(it.hs[k], it.ws[k], c->max_px)) { b->ok = false; continue; }
            order.push_back(k);
        }
    { std::lock_guard<std::mutex> l(c->rm); c->batch_to_come += int(order.size()); }
    size_t next = 0;
    while (next < order.size()) {
        Group &g = c->groups[size_t(take_group(c))];
        collect_timing(c, g);                               // events of its previous use are complete by now
        const int kind = kind_of(order[next]);
        g.outs = it.outs; g.caps = it.caps; g.lens = it.lens; g.kind = kind; g.batch = b; g.recons = it.recons;
        g.n_jobs = 0;
        while (next < order.size() && g.n_jobs < int(g.slots.size()) && kind_of(order[next]) == kind) {
            const int k = order[next++];
            Slot &s = g.slots[size_t(g.n_jobs++)];
            s.job = k; s.h = it.hs[k]; s.w = it.ws[k]; s.cb = -1; s.pack_n = 1; s.pack_lane = 0; s.near = near_of(k); s.effort = effort_of(k);
            unsigned char *const rec = it.recons ? it.recons[k] : nullptr;
            const bool collected = it.from && it.from->how[size_t(k)] == kSrcCollect;      // (launch_front copies the collected plane)
            if (kind == 0 && rec && !collected) {         // -n0 -e1: the reconstruction IS the input (NBLIC.c:876 rewrites the same bytes)
                const size_t n = size_t(s.h) * size_t(s.w);
                if (it.on_device) { if (hipMemcpy(rec, it.imgs[k], n, hipMemcpyDeviceToHost) != hipSuccess) b->ok = false; }
                else if (rec != it.imgs[k]) memcpy(rec, it.imgs[k], n);
            }
        }
        start_group(c, g, it.imgs, it.on_device, it.from);
    }
}

static void submitter_main(nblic_amd_ctx *c) {
    pthread_setname_np(pthread_self(), "nblic-submit");
    if (hipSetDevice(c->device) != hipSuccess) c->broken = true;
    for (;;) {
        nblic_amd_ctx::SubmitItem it;
        {
            std::unique_lock<std::mutex> l(c->sm);
            c->scv.wait(l, [c] { return c->stop_submit || !c->sq.empty(); });
            if (c->sq.empty()) return;
            it = c->sq.front(); c->sq.pop_front();
        }
        {
            std::lock_guard<std::mutex> g(c->api);
            { std::lock_guard<std::mutex> l(c->rm); c->queued_images -= it.n; }         // from here on they are counted in batch_to_come
            encode_submit(c, it);
        }
        { std::lock_guard<std::mutex> l(c->fm); it.b->submitted = true; }
        c->fcv.notify_all();
    }
}

static void queue_batch(nblic_amd_ctx *c, const nblic_amd_ctx::SubmitItem &it) {
    for (int k = 0; k < it.n; k++) it.lens[k] = -1;
    { std::lock_guard<std::mutex> l(c->rm); c->queued_images += it.n; }
    { std::lock_guard<std::mutex> l(c->sm); c->sq.push_back(it); }
    c->scv.notify_all();
}

static void report_coders(nblic_amd_ctx *c) {                        // NBLIC_AMD_DBG & 32, when nothing is outstanding
    if (!(dbg_flags() & kDbgReport) || !nothing_outstanding(c)) return;
    fprintf(stderr, "[nblic_amd] coder: singles %.0f Mbins in %.2f thread-s (%.0f Mbins/s), packs %.0f Mbins in %.2f thread-s (%.0f Mbins/s)\n",
            (c->total_bins - c->pack_bins) / 1e6, c->coder_s - c->pack_s, (c->total_bins - c->pack_bins) / 1e6 / (c->coder_s - c->pack_s + 1e-9),
            c->pack_bins / 1e6, c->pack_s, c->pack_bins / 1e6 / (c->pack_s + 1e-9));
    fprintf(stderr, "[nblic_amd] coder: %.2f thread-s of that queueing chunks (runtime calls)\n", c->issue_s);
    fprintf(stderr, "[nblic_amd] drivers: %.2f CPU-s in %ld group launches (%.1f ms each), %.2f CPU-s of that inside the wait for the front half\n",
            c->driver_cpu_s, c->driver_launches, 1e3 * c->driver_cpu_s / double(c->driver_launches ? c->driver_launches : 1), c->driver_wait_cpu_s);
    long t2 = 0, t9 = 0, t17 = 0;
    for (int k = 2; k <= 7; k++) t2 += c->takes[k];
    for (int k = 9; k <= 15; k++) t9 += c->takes[k];
    for (int k = 17; k < kMaxTake; k++) t17 += c->takes[k];
    // (a take is whole packs now: 2-8 images are one pack, 9-16 two, 17-24 three)
    fprintf(stderr, "[nblic_amd] coder: %.2f thread-s of that waiting for chunks; takes of 1/2-7/8/9-15/16/17-23/24 images: %ld/%ld/%ld/%ld/%ld/%ld/%ld\n", c->wait_s,
            c->takes[1], t2, c->takes[8], t9, c->takes[16], t17, c->takes[kMaxTake]);
}

static bool encode_wait(nblic_amd_ctx *c, nblic_amd_batch *b) {
    {   // wait for the coder threads (and with them every group's GPU work) of THIS batch
        std::unique_lock<std::mutex> l(c->fm);
        c->fcv.wait(l, [b] { return b->submitted && b->remaining == 0; });
    }
    bool ok = b->ok;
    for (int k = 0; k < b->n_images; k++) if (b->lens[k] < 0) ok = false;
    return ok;
}

// A whole batch on the caller's thread: queued like any other, then waited for -- for ITS images only, whatever else
// is outstanding on the context.  The caller must not hold c->api (the submitter takes it).
static bool run_batch(nblic_amd_ctx *c, nblic_amd_ctx::SubmitItem it) {
    if (it.n < 0 || hipSetDevice(c->device) != hipSuccess) return false;
    nblic_amd_batch b;
    it.b = &b;
    queue_batch(c, it);
    return encode_wait(c, &b) && !c->broken;
}

// ---- QNBLIC (effort 0): model on the GPU, entropy stage on a coder thread ---------------------
static bool launch_q(nblic_amd_ctx *c, Group &g, const uint8_t *const *imgs, bool on_device, const CollectFrom *from) {
    collect_begin(g);
    if (from && !collect_room(g, g.slots.size())) return false;
    for (int k = 0; k < g.n_jobs; k++)
        if (!slot_begin(g, k, imgs, on_device, false, 0, from)) return false;
    if (!collect_flush(g, g.stream)) return false;
    HIP_OK(hipMemcpyAsync(g.d_jobs, g.h_jobs, size_t(g.n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, g.stream));
    q_launch_model(g.d_jobs, g.h_jobs, g.n_jobs, g.stream);
    g.tm_pending = false;
    for (int k = 0; k < g.n_jobs; k++) {
        Slot &s = g.slots[size_t(k)];
        const size_t n = size_t(s.h) * size_t(s.w), n_pad = (n + 1) & ~size_t(1), need = n_pad + 2 * 12 * 256;
        if (!acquire_coded(c, s, need)) return false;
        uint16_t *dst = c->cbufs[size_t(s.cb)];
        HIP_OK(hipMemcpyAsync(dst, s.b.pxs, n * sizeof(uint16_t), hipMemcpyDeviceToDevice, g.stream));
        HIP_OK(hipMemcpyAsync(dst + n_pad, s.b.qhist, 12 * 256 * sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream));
    }
    // the block counts of the context chains (nblic_amd_long_chain_stats); on_group_done adds them up
    HIP_OK(hipMemcpyAsync(g.h_totals, g.d_totals, size_t(g.n_jobs) * kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    HIP_OK(hipLaunchHostFunc(g.stream, on_group_done, &g));
    return true;
}

// ---- decoders: every stream of a batch side by side, one wave per image (serial_engine.hip) -----

struct DecodeItem { int k, h, w, near, k_step, effort, kind; size_t len; long q_pos; int qtab; };      // kind 0 NBLIC, 1 QNBLIC; q_pos: first rANS word; qtab: which parsed table set

constexpr int kDecodeChunk = 1024;                                                         // images per chunk of decode_batch (above the lean decoder's threshold)
constexpr size_t kQTab = 2 * 12 * 256 * sizeof(uint32_t);                                   // QNBLIC: frequencies, cumulative starts (the kernel derives its symbol index from them)
static size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

// ---- what every decoder (and the band encoder's records) shares: one place for each decision ---------------------------
// The codec fields a stream header, a checkpoint or an index names (NBLIC.c:717-729, QNBLIC.c:475-486).
static bool codec_fields_ok(int kind, int h, int w, int near, int k_step, int effort, long max_px) {
    if (!size_ok(h, w, max_px)) return false;
    if (kind == 0) return near >= 0 && near <= kMaxNear && k_step >= kMinKStep && k_step <= kLevels && effort >= 1 && effort <= 3;
    return kind == 1 && near == 0 && effort == 0 && k_step == kMinKStep;
}

// Sizes of one image's decode: its state record, its least-squares statistics [B | F] (efforts 2 / 3; B is the first
// half), the rows one launch covers.
static size_t record_state_bytes(int kind) { return kind ? kQDecodeStateBytes : kDecodeStateBytes; }
static size_t lsq_stats_bytes(int kind, int effort, int w) { return stats_doubles(kind ? 0 : effort, w) * sizeof(double); }
static int rows_per_launch(const DecodeItem &it, int override_rows) { return serial_rows_per_launch(it.h, it.w, it.kind ? 1 : it.effort, override_rows); }
static unsigned long long first_pos(const DecodeItem &it) { return it.kind ? (unsigned long long)(it.q_pos) * 2ull : (unsigned long long)(kHeaderBytes); }
static size_t stream_buf_bytes(size_t n) { return up256(n + 2048); }                      // a device copy of n stream bytes (upload_stream)

// QNBLIC: the header and the twelve histogram tables in front of the rANS words -- at most 4 + 12 x 256 16-bit codes
// (q_entropy.cpp q_read_hist) -- from the n bytes at p into a kQTab buffer.  Returns the index of the first rANS word,
// or -1 when the tables do not parse from those bytes.
static long q_parse_tables(const unsigned char *p, size_t n, uint8_t *tab) {
    uint16_t words[4 + 12 * 256];
    const size_t n_words = std::min(n / 2, sizeof words / 2);
    memcpy(words, p, n_words * 2);
    uint32_t *freq = reinterpret_cast<uint32_t *>(tab);
    int hh = 0, ww = 0;
    return q_decode_tables(words, n_words, &hh, &ww, freq, freq + 12 * 256, nullptr);
}

// Header of a stream of which `len` bytes are in hand (NBLIC.c:698-745, QNBLIC.c:475-486).  false = not a stream this
// library decodes (or refused: size, parameters); true = fields filled in (`it` is left alone otherwise).
static bool parse_stream_header(const unsigned char *p, size_t len, long max_px, DecodeItem &it) {
    DecodeItem h = it;
    if (len >= size_t(kHeaderBytes) && memcmp(p, "NBLIC0.3", 8) == 0) {
        if (p[8] > 1) return false;                                      // n_channel
        h.kind = 0; h.h = (p[9] << 8) | p[10]; h.w = (p[11] << 8) | p[12]; h.near = p[13]; h.k_step = p[14]; h.effort = p[15];
    } else if (len >= 8 && p[0] == 'Q' && p[1] == '0' && p[2] == '.' && p[3] == '2') {
        uint16_t q[4];
        memcpy(q, p, 8);
        h.kind = 1; h.h = q[2]; h.w = q[3]; h.near = h.effort = 0; h.k_step = kMinKStep;
    } else {
        return false;
    }
    if (!codec_fields_ok(h.kind, h.h, h.w, h.near, h.k_step, h.effort, max_px)) return false;
    it = h;
    return true;
}

// A stream's description from the `len` bytes of it at p: the header, it.len, and for QNBLIC the tables (into tab) and
// q_pos.  A complete stream (partial = false) is refused unless it holds what the decoder reads before the first pixel:
// NBLIC the header and the coder's first four bytes, QNBLIC the tables and the four bytes of the rANS state.  The prefix
// of a stream still being fed (partial) needs more while its header or tables are not all there -- the tables are at
// most 12 x 256 codes, so 64 KB that do not parse never will.
enum class Described { ok, more, refused };
static Described describe_stream(const unsigned char *p, size_t len, bool partial, long max_px, DecodeItem &it, std::vector<uint8_t> &tab) {
    if (partial && len < ((len >= 1 && p[0] == 'Q') ? size_t(8) : size_t(kHeaderBytes))) return Described::more;
    if (!parse_stream_header(p, len, max_px, it)) return Described::refused;
    it.len = len;
    if (it.kind == 0) return partial || len >= size_t(kHeaderBytes) + 4 ? Described::ok : Described::refused;
    tab.assign(kQTab, 0);
    it.q_pos = q_parse_tables(p, len, tab.data());
    if (it.q_pos < 0) return partial && len < 65536 ? Described::more : Described::refused;
    return partial || size_t(it.q_pos) * 2 + 4 <= len ? Described::ok : Described::refused;
}

// The decode job of an item.  The buffers are the driver's: the plane (recon; recon_row0 the image row at its index 0),
// the stream (stream_off its absolute offset), the state record, the statistics, the QNBLIC tables; end_row 0 = h.
static SerialJob decode_job(const DecodeItem &it, uint8_t *recon, int recon_row0, const uint8_t *stream, unsigned long long stream_off,
                            SerialState *state, double *stats, const uint8_t *tab, int rows, int end_row, unsigned long long *redo) {
    SerialJob J{};
    J.redo = redo;
    J.recon = recon; J.recon_row0 = recon_row0;
    J.stream = stream; J.stream_off = stream_off;
    J.state = state; J.stats = stats;
    J.h = it.h; J.w = it.w; J.near = it.near; J.k_step = it.k_step; J.effort = it.effort;
    J.rows = rows; J.end_row = end_row;
    if (it.kind) { J.q_freq = reinterpret_cast<const uint32_t *>(tab); J.q_start = J.q_freq + 12 * 256; J.q_slot = nullptr; }
    return J;
}

// n stream bytes into a device buffer of stream_buf_bytes(n) bytes, zeros from n & ~3 to its end: the window reads whole
// 512-byte blocks past the end.
static bool upload_stream(uint8_t *d, const unsigned char *src, size_t n, hipStream_t st) {
    const size_t z = n & ~size_t(3);
    return hipMemsetAsync(d + z, 0, stream_buf_bytes(n) - z, st) == hipSuccess && hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, st) == hipSuccess;
}

// A sealed record (index_entries.h: sha256_of, seal): a head (magic, format version, ...), a body, and the SHA-256 of both
// in its last 32 bytes.
// The head (into H) and the body of the len bytes at p if they are a sealed record of this magic and version; else null.
template <class Head> static const uint8_t *sealed_body(const void *p, size_t len, const char *magic, uint32_t version, Head &H) {
    uint8_t d[32];
    if (!p || len < sizeof(Head) + 32) return nullptr;
    memcpy(&H, p, sizeof H);
    sha256_of(p, len - 32, d);
    const uint8_t *b = static_cast<const uint8_t *>(p);
    return memcmp(H.magic, magic, 8) == 0 && H.version == version && memcmp(d, b + len - 32, 32) == 0 ? b + sizeof H : nullptr;
}

// A decoder checkpoint (NBLDCKPT): this head, the body (RecordLayout), sealed.  The band decoder's checkpoint and every
// entry of a seek index.
constexpr uint32_t kDecodeCheckpointVersion = 1;
struct DecodeCheckpoint {              // followed by: state record | B | two rows above next_row | QNBLIC tables | SHA-256 of all before it
    char magic[8];                     // "NBLDCKPT"
    uint32_t version;                  // kDecodeCheckpointVersion
    int32_t kind, h, w, near, k_step, effort, band_rows, next_row;
    uint32_t reserved;
    unsigned long long feed_from;      // absolute stream offset from which the resumed decoder must be fed (pos & ~511)
    unsigned long long body_bytes;     // bytes between this head and the checksum
    Sha256 rows_sha;                   // of rows [0, next_row)
};
static_assert(std::is_trivially_copyable<DecodeCheckpoint>::value, "written and read as bytes");
static_assert(sizeof(DecodeCheckpoint) == kCheckpointHeadBytes && kDecodeStateBytes == kNblicRecordBytes && kQDecodeStateBytes == kQnblicRecordBytes &&
              kQTab == kQnblicTableBytes && NBLIC_MAX_HEIGHT == kIndexMaxSide && NBLIC_MAX_WIDTH == kIndexMaxSide, "index_entries.h states these sizes for host-only code");
constexpr unsigned long long kMaxStreamPos = 1ull << 48;   // no stream this library decodes comes near it

// Where the parts of a decoder record's body are, in bytes from its start (the state record is at 0).
struct RecordLayout { size_t b, b_bytes, rows, tab, bytes; };
static RecordLayout record_layout(int kind, int w, int effort) {
    RecordLayout L;
    L.b = record_state_bytes(kind);
    L.b_bytes = lsq_stats_bytes(kind, effort, w) / 2;
    L.rows = L.b + L.b_bytes;
    L.tab = L.rows + 2 * size_t(w);
    L.bytes = L.tab + (kind ? kQTab : 0);
    return L;
}

static DecodeCheckpoint decode_head(const DecodeItem &it, int band_rows, int next_row, unsigned long long feed_from, const Sha256 &rows_sha) {
    DecodeCheckpoint H{};
    memcpy(H.magic, "NBLDCKPT", 8);
    H.version = kDecodeCheckpointVersion;
    H.kind = it.kind; H.h = it.h; H.w = it.w; H.near = it.near; H.k_step = it.k_step; H.effort = it.effort;
    H.band_rows = band_rows; H.next_row = next_row;
    H.feed_from = feed_from;
    H.body_bytes = record_layout(it.kind, it.w, it.effort).bytes;
    H.rows_sha = rows_sha;
    return H;
}

// The two rows above row r as a record holds them (decoder and encoder alike): rows [r - n, r), n = min(r, 2), at byte
// (2 - n) w of a 2 w-byte slot, zeros in front.  Between a plane on the device (plane_row0: the image row at its index 0)
// and a slot, queued on st.
struct RowsAbove { int first, n; size_t at; };
static RowsAbove rows_above(int r, int w) { const int n = r < 2 ? r : 2; return RowsAbove{r - n, n, size_t(2 - n) * size_t(w)}; }
static bool rows_above_out(uint8_t *slot, const uint8_t *plane, int plane_row0, int r, int w, hipStream_t st) {
    const RowsAbove A = rows_above(r, w);
    memset(slot, 0, A.at);
    return A.n == 0 || hipMemcpyAsync(slot + A.at, plane + size_t(A.first - plane_row0) * size_t(w), size_t(A.n) * size_t(w), hipMemcpyDeviceToHost, st) == hipSuccess;
}
static bool rows_above_in(uint8_t *plane, int plane_row0, const uint8_t *slot, int r, int w, hipStream_t st) {
    const RowsAbove A = rows_above(r, w);
    return A.n == 0 || hipMemcpyAsync(plane + size_t(A.first - plane_row0) * size_t(w), slot + A.at, size_t(A.n) * size_t(w), hipMemcpyHostToDevice, st) == hipSuccess;
}

// Adaptive state a record carries that the kernels divide by or index with.  A counter pair {c0, c1}: the probability
// divides by c0 + c1, and the counter walks (kernels_e1.hip k_counter_epochs) start from a sum of at most kCountLimit;
// neither half ever falls below 1 (k_init_state, counter_add).  A re-mapper: symbol -> rank and rank -> symbol are
// inverse permutations of 0 .. 19.  B: sums of pixel products, never NaN or infinite.
static bool counter_ok(int c0, int c1) { return c0 >= 1 && c1 >= 1 && c0 + c1 <= kCountLimit; }
template <class T> static bool remapper_ok(const T *rank_of, const T *sym_at) {
    for (int z = 0; z < kMapSyms; z++) {
        const int y = int(sym_at[z]);
        if (y < 0 || y >= kMapSyms || int(rank_of[y]) != z) return false;
    }
    return true;
}
static bool finite_doubles(const uint8_t *p, size_t bytes) {
    for (size_t k = 0; k < bytes; k += 8) {
        double v;
        memcpy(&v, p + k, 8);
        if (!(v == v) || v - v != 0.0) return false;
    }
    return true;
}

// One launch round of a (codec, effort) class: every job advances by its `rows`.
static bool decode_launch(const DecodeItem &first, const SerialJob *d_jobs, const SerialJob *h_jobs, int n, hipStream_t st, bool whole_streams) {
    return first.kind == 1 ? serial_qdecode_launch(d_jobs, h_jobs, n, st) : serial_decode_launch(d_jobs, h_jobs, n, st, whole_streams);
}

// ---- delivery to caller-owned device memory (deliver.h, serial_engine.h k_deliver) ----------------------------------------
// What the _to calls hand down: one destination per image with its step and normalisation, one format per call.  The
// calls without a step make theirs here (dests_ex): the element size, and the call's scale / bias in every image.
// modes (the _color calls; NBLIC_AMD_FORMAT_RCT: every one 0x0D): images 3f, 3f + 1, 3f + 2 are the three planes of frame f
// in colour mode modes[f] (color_plan.h), and the channels coded as differences are put together again on the way out
// (deliver.h: a task with a reference).  A frame of mode 0 is three images like any other.
// slice_modes / depth (the _stack calls, stack.h): image s * depth + d is slice d of stack s; a run of differences is put
// together again by ONE task of k_deliver_stack, a key slice without a delta behind it goes through k_deliver like any image.
struct DeliverTo {
    const nblic_amd_dest_ex *dests; uint32_t format; const uint8_t *modes = nullptr;
    const uint8_t *slice_modes = nullptr; int depth = 0;
    // deep_modes (the _deep calls, deep.h): streams 2i and 2i + 1 are the high and the low plane of deep image i, dests[i] is
    // its destination and deep_format the destinations' format in the deep calls' own numbering (`format` is not read)
    const uint8_t *deep_modes = nullptr; uint32_t deep_format = 0;
    uint32_t mode_of(int k) const { return modes ? modes[k / 3] : 0u; }  // of the frame image k belongs to
    bool skipped(int k) const { return slice_modes && !dests[k].ptr && dests[k].cap_bytes == 0; }      // a slice decoded as a reference only
    bool stack_has_delta(int k) const {                                  // does the stack image k belongs to hold a delta slice?
        if (!slice_modes) return false;
        const int s = k - k % depth;
        for (int i = s; i < s + depth; i++) if (slice_modes[i] == kStackDelta) return true;
        return false;
    }
};

// The depth and the slice modes of a _stack call (stack.h), as the entry points hand them down.
struct StackArg { int depth; const unsigned char *modes; };

// NBLIC_AMD_FORMAT_RCT in a format argument of a _from or a _to_ex call: is it there?  It is taken off.
static bool format_rct(int &format) {
    const bool rct = format >= 0 && (format & NBLIC_AMD_FORMAT_RCT) != 0;
    if (rct) format &= ~NBLIC_AMD_FORMAT_RCT;
    return rct;
}

// Every frame's mode 0x0D: what the flag stands for in the _color calls' terms.
static std::vector<uint8_t> rct_modes(int n) { return std::vector<uint8_t>(size_t(std::max(n, 0) / 3), uint8_t(kColorRct)); }
// The modes of a _color call: n / 3 valid bytes?
static bool color_modes_ok(int n, const unsigned char *modes) {
    if (n < 0 || n % 3 != 0 || !modes) return false;
    for (int f = 0; f < n / 3; f++) if (!color_mode_valid(modes[f])) return false;
    return true;
}

// Do the three tasks of a colour frame name the same window (in rows and columns of the image)?
static bool same_window(const DeliverTask &a, const DeliverTask &b) { return a.row0 == b.row0 && a.row1 == b.row1 && a.col0 == b.col0 && a.col1 == b.col1; }

static std::vector<nblic_amd_dest_ex> dests_ex(const nblic_amd_dest *dests, int n, int format, float scale, float bias) {
    std::vector<nblic_amd_dest_ex> ex(size_t(std::max(n, 0)));
    for (size_t k = 0; k < ex.size(); k++) {
        const nblic_amd_dest &D = dests[k];
        ex[k] = nblic_amd_dest_ex{D.ptr, D.pitch_bytes, deliver_elem(uint32_t(format)), D.cap_bytes, D.row0, D.row1, D.col0, D.col1, scale, bias};
    }
    return ex;
}

static bool deliver_args_ok(int format, float scale, float bias) {
    if (format < 0 || format >= int(kDeliverFormats)) return false;
    if (!(scale - scale == 0.0f) || !(bias - bias == 0.0f)) return false;                // NaN, infinite
    return format != int(kDeliverU8) || (scale == 1.0f && bias == 0.0f);
}

// Does the runtime report [ptr, ptr + extent) as device memory of this context's device, inside ONE allocation?  What the
// delivery asks of a destination and the collection of a source.
static bool device_range_ok(const nblic_amd_ctx *c, const void *ptr, unsigned long long extent) {
    hipPointerAttribute_t A;
    void *base = nullptr;
    size_t size = 0;
    if (hipPointerGetAttributes(&A, ptr) != hipSuccess ||
        hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t *>(&base), &size, const_cast<void *>(ptr)) != hipSuccess) {
        (void)hipGetLastError();                                         // (a pointer the runtime does not know is an error to it, not to this context)
        return false;
    }
    if (A.type != hipMemoryTypeDevice || A.device != c->device) return false;
    return uintptr_t(ptr) >= uintptr_t(base) && uintptr_t(ptr) - uintptr_t(base) + extent <= size;
}

// The window destination k names in an image of h x w, and the task that fills it -- all but src, src_bytes, gate and zero,
// which are the caller's.  false: refused, on the host, before anything of the image is launched: the window is empty or
// outside the image, the pointer, the pitch or the step is no multiple of the element size or is below it, the step or the
// pitch is beyond its limit, a contiguous destination's pitch is below its row, the scale or the bias is not finite (or not
// 1 / 0 for uint8), the window does not fit cap_bytes, or the runtime does not know the pointer as memory of this context's
// device that holds the whole extent.
static bool deliver_dest_task(const nblic_amd_ctx *c, const DeliverTo &to, int k, int h, int w, DeliverTask &T) {
    const nblic_amd_dest_ex &D = to.dests[k];
    T = DeliverTask{};
    T.row0 = D.row0; T.row1 = D.row1 ? D.row1 : h; T.col0 = D.col0; T.col1 = D.col1 ? D.col1 : w;
    if (T.row0 < 0 || T.row1 <= T.row0 || T.row1 > h || T.col0 < 0 || T.col1 <= T.col0 || T.col1 > w) return false;
    if (to.skipped(k)) {                                                 // a _stack call's slice that is decoded as a reference only: the window, and no destination
        T.src_pitch = uint32_t(w); T.format = to.format; T.dst_step = deliver_elem(to.format);
        return true;
    }
    if (!deliver_args_ok(int(to.format), D.scale, D.bias)) return false;
    const size_t elem = deliver_elem(to.format), rows = size_t(T.row1 - T.row0), cols = size_t(T.col1 - T.col0);
    if (!D.ptr || uintptr_t(D.ptr) % elem || D.pitch_bytes % elem || D.step_bytes % elem || D.step_bytes < elem || D.step_bytes > kDeliverMaxStep) return false;
    if (D.pitch_bytes < (D.step_bytes == elem ? cols * elem : elem) || D.pitch_bytes > kDeliverMaxPitch) return false;
    const unsigned long long extent = deliver_extent(uint32_t(rows), uint32_t(cols), to.format, D.pitch_bytes, D.step_bytes);
    if (extent > D.cap_bytes || !device_range_ok(c, D.ptr, extent)) return false;
    T.dst =static_cast<uint8_t *>(D.ptr); T.dst_pitch = D.pitch_bytes; T.dst_step = uint32_t(D.step_bytes);
    T.src_pitch = uint32_t(w);
    T.format = to.format; T.scale = D.scale; T.bias = D.bias;
    return deliver_task_chunks(T) < (1ull << 31) / kDeliverChunkUnits;
}

// The tasks' places in ONE k_deliver launch, their upload to d_tasks and the launch, queued on st.  `c`: the context whose
// nblic_amd_deliver_stats count them (null: the zeros after a failure are not counted).
// deliver_place: the places alone, counted and held against the limits of one launch.
static bool deliver_place(DeliverTask *tasks, size_t n, nblic_amd_ctx *c, unsigned long long &chunks) {
    long strided = 0;
    chunks = 0;
    for (size_t i = 0; i < n; i++) { tasks[i].first_chunk = uint32_t(chunks); chunks += deliver_task_chunks(tasks[i]); strided += deliver_strided(tasks[i]) ? 1 : 0; }
    if (c && n) { std::lock_guard<std::mutex> l(c->stat_m); c->deliver_tasks += long(n); c->deliver_strided += strided; }
    return chunks < (1ull << 31) && n < (size_t(1) << 30);
}
static bool deliver_queue(DeliverTask *tasks, size_t n, DeliverTask *d_tasks, hipStream_t st, nblic_amd_ctx *c = nullptr) {
    unsigned long long chunks = 0;
    const bool fits = deliver_place(tasks, n, c, chunks);
    if (n == 0) return true;
    if (!fits) return false;
    return hipMemcpyAsync(d_tasks, tasks, n * sizeof(DeliverTask), hipMemcpyHostToDevice, st) == hipSuccess && deliver_launch(d_tasks, int(n), uint32_t(chunks), st);
}

static void deliver_stats_reset(nblic_amd_ctx *c) {
    if (!c) return;
    std::lock_guard<std::mutex> l(c->stat_m);
    c->deliver_tasks = c->deliver_strided = 0;
}

// After a device failure: zero bytes into every window, by the same kernel, as far as the stream still works.
static void deliver_zeros(std::vector<DeliverTask> &tasks, hipStream_t st) {
    tasks.erase(std::remove_if(tasks.begin(), tasks.end(), [](const DeliverTask &T) { return !T.dst; }), tasks.end());      // (a _stack call's skipped slices have no window to zero)
    if (tasks.empty() || !st) return;
    DevBuf<DeliverTask> d_tasks;
    for (DeliverTask &T : tasks) { T.zero = 1; T.gate = nullptr; }
    if (d_tasks.alloc(tasks.size()) == hipSuccess && deliver_queue(tasks.data(), tasks.size(), d_tasks, st)) hipStreamSynchronize(st);
}

// ---- the delivery of a _deep call (deep.h, serial_engine.h k_deliver_deep) ------------------------------------------------------
// Stream k of a _deep call is plane k % 2 of deep image k / 2, decoded into a plane of h x w like any image.  The window that
// the image's destination names, as a task WITHOUT a destination (dst null: k_deliver never sees it) -- row0 .. col1 and
// src_pitch; src, src_bytes, gate and zero are the caller's.  false: refused on the host, as deliver_dest_task refuses, and a
// uint16 / int16 destination whose signedness contradicts the image's mode.
static bool deep_dest_window(const nblic_amd_ctx *c, const DeliverTo &to, int k, int h, int w, DeliverTask &T) {
    const nblic_amd_dest_ex &D = to.dests[k / 2];
    const uint32_t mode = to.deep_modes[k / 2], format = to.deep_format;
    T = DeliverTask{};
    T.row0 = D.row0; T.row1 = D.row1 ? D.row1 : h; T.col0 = D.col0; T.col1 = D.col1 ? D.col1 : w;
    if (T.row0 < 0 || T.row1 <= T.row0 || T.row1 > h || T.col0 < 0 || T.col1 <= T.col0 || T.col1 > w) return false;
    if ((format == kDeepToU16 && (mode & kDeepSigned)) || (format == kDeepToI16 && !(mode & kDeepSigned))) return false;
    if (!(D.scale - D.scale == 0.0f) || !(D.bias - D.bias == 0.0f) || (format <= kDeepToI16 && (D.scale != 1.0f || D.bias != 0.0f))) return false;
    const size_t elem = deep_dest_elem(format), rows = size_t(T.row1 - T.row0), cols = size_t(T.col1 - T.col0);
    if (!D.ptr || uintptr_t(D.ptr) % elem || D.pitch_bytes % elem || D.step_bytes % elem || D.step_bytes < elem || D.step_bytes > kDeliverMaxStep) return false;
    if (D.pitch_bytes < (D.step_bytes == elem ? cols * elem : elem) || D.pitch_bytes > kDeliverMaxPitch) return false;
    const unsigned long long extent = deep_dest_extent(uint32_t(rows), uint32_t(cols), format, D.pitch_bytes, D.step_bytes);
    if (extent > D.cap_bytes || !device_range_ok(c, D.ptr, extent)) return false;
    T.src_pitch = uint32_t(w);
    return true;
}
// The task of deep image i from the two planes' window tasks (above, with src, src_bytes, gate and zero filled in; their row0
// counts from the first row of src, which may differ between the planes).
static DeepDeliverTask deep_deliver_task(const DeliverTo &to, int i, const DeliverTask &H, const DeliverTask &L) {
    const nblic_amd_dest_ex &D = to.dests[i];
    const size_t skip_h = size_t(H.row0) * size_t(H.src_pitch), skip_l = size_t(L.row0) * size_t(L.src_pitch);
    DeepDeliverTask T{};
    T.hi = H.src + skip_h; T.hi_bytes = H.src_bytes - skip_h; T.gate_hi = H.gate;
    T.lo = L.src + skip_l; T.lo_bytes = L.src_bytes - skip_l; T.gate_lo = L.gate;
    T.dst = static_cast<uint8_t *>(D.ptr); T.dst_pitch = D.pitch_bytes; T.dst_step = uint32_t(D.step_bytes);
    T.src_pitch = H.src_pitch; T.rows = uint32_t(H.row1 - H.row0); T.col0 = uint32_t(H.col0); T.col1 = uint32_t(H.col1);
    T.format = to.deep_format; T.mode = to.deep_modes[i]; T.scale = D.scale; T.bias = D.bias;
    T.zero = (H.zero || L.zero) ? 1u : 0u;
    return T;
}
// The tasks' places in ONE k_deliver_deep launch, their upload to d_tasks and the launch, queued on st.  marks: two events,
// made here and recorded around the launch (nblic_amd_deep_plan_stats).
static bool deliver_deep_queue(nblic_amd_ctx *c, DeepDeliverTask *tasks, size_t n, DeepDeliverTask *d_tasks, hipStream_t st, Event *marks = nullptr) {
    unsigned long long chunks = 0;
    for (size_t i = 0; i < n; i++) { tasks[i].first_chunk = uint32_t(chunks); chunks += deep_deliver_chunks(tasks[i]); }
    if (n == 0) return true;
    if (!d_tasks || chunks >= (1ull << 31) || n >= (size_t(1) << 30)) return false;
    if (c) c->deep_counts[2] += 1;
    if (hipMemcpyAsync(d_tasks, tasks, n * sizeof(DeepDeliverTask), hipMemcpyHostToDevice, st) != hipSuccess) return false;
    if (marks && (marks[0].create(hipEventDefault) != hipSuccess || marks[1].create(hipEventDefault) != hipSuccess || hipEventRecord(marks[0], st) != hipSuccess)) return false;
    if (!deliver_deep_launch(d_tasks, int(n), uint32_t(chunks), st)) return false;
    return !marks || hipEventRecord(marks[1], st) == hipSuccess;
}
// After the stream has been waited for: the GPU time between two recorded marks into slot `which` of the context's deep figures.
static void deep_timed(nblic_amd_ctx *c, Event *marks, int which) {
    float ms = 0.0f;
    if (marks[0] && marks[1] && hipEventElapsedTime(&ms, marks[0], marks[1]) == hipSuccess) { std::lock_guard<std::mutex> l(c->stat_m); c->deep_ms[which] = double(ms); }
}
// After a device failure: zero bytes into the window of every deep image both of whose planes were accepted (of[k]: stream
// k's window task, null for none), by the same kernel, as far as the stream still works.
static void deliver_deep_zeros(const DeliverTo &to, const std::vector<const DeliverTask *> &of, hipStream_t st) {
    std::vector<DeepDeliverTask> tasks;
    for (size_t k = 0; k + 1 < of.size(); k += 2) {
        if (!of[k] || !of[k + 1]) continue;
        DeepDeliverTask T = deep_deliver_task(to, int(k / 2), *of[k], *of[k + 1]);
        T.zero = 1; T.gate_hi = T.gate_lo = nullptr;
        tasks.push_back(T);
    }
    if (tasks.empty() || !st) return;
    DevBuf<DeepDeliverTask> d_tasks;
    if (d_tasks.alloc(tasks.size()) == hipSuccess && deliver_deep_queue(nullptr, tasks.data(), tasks.size(), d_tasks, st)) hipStreamSynchronize(st);
}

// ---- the delivery of a _stack call (stack.h, serial_engine.h k_deliver_stack) ---------------------------------------------------
// What a _stack call launches: the tasks of k_deliver for its lone key slices, and the runs with their slice records.
struct StackDelivery {
    std::vector<DeliverTask> plain; std::vector<StackDeliverTask> runs; std::vector<StackSlice> slices;
    Event t0, t1;                                                        // around the call's delivery launches (nblic_amd_stack_plan_stats)
};

// of[k]: image k's task as k_deliver would take it -- its window, its plane from row 0 on, its gate, zero for a plane known to
// be bad, dst null for a skipped slice -- or null for an image that is not live (a stack with a delta is live as a whole).
static void stack_delivery_plan(const DeliverTo &to, int n, const std::vector<const DeliverTask *> &of, StackDelivery &P) {
    for (int s = 0; s + to.depth <= n; s += to.depth)
        for (int d = 0; d < to.depth;) {
            const int len = int(stack_run_len(to.slice_modes + s, uint32_t(d), uint32_t(to.depth)));
            const DeliverTask *K = of[size_t(s + d)];
            if (len == 1) {
                if (K && K->dst) P.plain.push_back(*K);
                d++;
                continue;
            }
            bool live = true, wanted = false;
            for (int i = 0; i < len; i++) { const DeliverTask *T = of[size_t(s + d + i)]; live = live && T; wanted = wanted || (T && T->dst); }
            if (live && wanted) {
                StackDeliverTask R{};
                R.first_slice = uint32_t(P.slices.size()); R.count = uint32_t(len);
                R.rows = uint32_t(K->row1 - K->row0); R.col0 = uint32_t(K->col0); R.col1 = uint32_t(K->col1); R.src_pitch = K->src_pitch; R.format = K->format;
                for (int i = 0; i < len; i++) {
                    const DeliverTask &T = *of[size_t(s + d + i)];
                    const size_t skip = size_t(T.row0) * size_t(T.src_pitch);
                    StackSlice S{};
                    S.src = T.src + skip; S.src_bytes = T.src_bytes - skip; S.gate = T.gate;
                    S.dst = T.dst; S.dst_pitch = T.dst_pitch; S.dst_step = T.dst_step; S.scale = T.scale; S.bias = T.bias; S.zero = T.zero;
                    P.slices.push_back(S);
                }
                P.runs.push_back(R);
            }
            d += len;
        }
}

// The runs' places in ONE k_deliver_stack launch, held against its limits, and the upload of the two tables, queued on st.
static bool deliver_stack_upload(StackDeliverTask *runs, size_t n, const StackSlice *slices, size_t n_slices, StackDeliverTask *d_runs, StackSlice *d_slices,
                                 hipStream_t st, unsigned long long &chunks) {
    chunks = 0;
    for (size_t i = 0; i < n; i++) { runs[i].first_chunk = uint32_t(chunks); chunks += stack_task_chunks(runs[i]); }
    if (n == 0) return true;
    if (chunks >= (1ull << 31) || n >= (size_t(1) << 30) || n_slices >= (size_t(1) << 30)) return false;
    return hipMemcpyAsync(d_runs, runs, n * sizeof(StackDeliverTask), hipMemcpyHostToDevice, st) == hipSuccess &&
           hipMemcpyAsync(d_slices, slices, n_slices * sizeof(StackSlice), hipMemcpyHostToDevice, st) == hipSuccess;
}

// At most one launch of each kernel for the call, queued on st: the three tables go up first (d_plain, d_runs, d_slices: room
// for P's, the caller's, alive until the stream has been waited for), then the launches between the two events.
static bool stack_delivery_queue(nblic_amd_ctx *c, StackDelivery &P, DeliverTask *d_plain, StackDeliverTask *d_runs, StackSlice *d_slices, hipStream_t st) {
    if ((!P.plain.empty() && !d_plain) || (!P.runs.empty() && (!d_runs || !d_slices))) return false;
    unsigned long long plain_chunks = 0, run_chunks = 0;
    if (!deliver_place(P.plain.data(), P.plain.size(), c, plain_chunks)) return false;
    if (!P.plain.empty() && hipMemcpyAsync(d_plain, P.plain.data(), P.plain.size() * sizeof(DeliverTask), hipMemcpyHostToDevice, st) != hipSuccess) return false;
    if (!deliver_stack_upload(P.runs.data(), P.runs.size(), P.slices.data(), P.slices.size(), d_runs, d_slices, st, run_chunks)) return false;
    if (P.t0.create(hipEventDefault) != hipSuccess || P.t1.create(hipEventDefault) != hipSuccess || hipEventRecord(P.t0, st) != hipSuccess) return false;
    if (!deliver_launch(d_plain, int(P.plain.size()), uint32_t(plain_chunks), st)) return false;
    if (!P.runs.empty()) {
        c->stack_counts[2] += 1; c->stack_counts[3] += long(P.runs.size());
        if (!deliver_stack_launch(d_runs, int(P.runs.size()), d_slices, uint32_t(run_chunks), st)) return false;
    }
    return hipEventRecord(P.t1, st) == hipSuccess;
}
// After the stream has been waited for: the GPU time of the call's delivery launches.
static void stack_delivery_timed(nblic_amd_ctx *c, const StackDelivery &P) {
    float ms = 0.0f;
    if (P.t0 && P.t1 && hipEventElapsedTime(&ms, P.t0, P.t1) == hipSuccess) { std::lock_guard<std::mutex> l(c->stat_m); c->stack_deliver_ms = double(ms); }
}

// ---- the sources of the _from calls, checked on the host (CollectFrom, above slot_begin) ------------------------------------
// Source k as a task -- all but dst, px0, px1 and first_chunk, which are the launch's -- and what becomes of it.  Refused,
// before anything of the image is launched: rows or cols the encoder does not take, a pointer, pitch or step that is no
// multiple of the element size or is below it, a step above 2^20 or a pitch above 2^40 bytes, an extent that cap_bytes
// does not hold, or that the runtime does not know as memory of this context's device inside one allocation.
static uint8_t collect_src_task(const nblic_amd_ctx *c, const CollectFrom &from, int k, CollectTask &T) {
    const nblic_amd_src &S = from.srcs[k];
    T = CollectTask{};
    if (!size_ok(S.rows, S.cols, c->max_px) || S.pitch_bytes > kCollectMaxPitch || S.step_bytes > kCollectMaxStep) return kSrcRefused;
    T.src = static_cast<const uint8_t *>(S.ptr);
    T.pitch = S.pitch_bytes; T.step = uint32_t(S.step_bytes);
    T.rows = uint32_t(S.rows); T.cols = uint32_t(S.cols); T.px0 = 0; T.px1 = T.rows * T.cols;
    T.format = from.format; T.scale = from.scale; T.bias = from.bias;
    if (!collect_source_ok(T, S.cap_bytes) || !device_range_ok(c, S.ptr, collect_extent(T.rows, T.cols, T.format, T.pitch, T.step))) return kSrcRefused;
    return collect_in_place(T.format, T.pitch, T.step, T.cols) ? kSrcInPlace : kSrcCollect;
}

// Every source of a call: how it is taken, its task, and the parent call's imgs / heights / widths.
static void collect_plan(const nblic_amd_ctx *c, CollectFrom &from, int n) {
    const size_t count = size_t(n);
    from.how.assign(count, kSrcRefused); from.tasks.assign(count, CollectTask{});
    from.imgs.assign(count, nullptr); from.hs.assign(count, 0); from.ws.assign(count, 0);
    for (int k = 0; k < n; k++) {
        const size_t i = size_t(k);
        from.how[i] = collect_src_task(c, from, k, from.tasks[i]);
        if (from.how[i] == kSrcRefused) continue;
        from.hs[i] = from.srcs[k].rows; from.ws[i] = from.srcs[k].cols;
        if (from.how[i] == kSrcInPlace) from.imgs[i] = from.tasks[i].src;
    }
    // Slice stacks: a delta slice becomes a task with the SOURCE of the slice before it as its reference (stack.h) --
    // collected even where it could be used in place -- and a key slice stays what it was.  A stack with a delta and a
    // refused source, or sources of unequal size, is refused as a whole; a stack of keys only is `depth` images like any other.
    if (!from.slice_modes.empty()) {
        const size_t D = size_t(from.depth);
        for (size_t s = 0; s + D <= count; s += D) {
            bool delta = false, ok = true;
            for (size_t i = s; i < s + D; i++) {
                delta = delta || from.slice_modes[i] == kStackDelta;
                ok = ok && from.how[i] != kSrcRefused && from.hs[i] == from.hs[s] && from.ws[i] == from.ws[s];
            }
            if (!delta) continue;
            for (size_t i = s; i < s + D; i++) {
                if (!ok) { from.how[i] = kSrcRefused; from.imgs[i] = nullptr; from.hs[i] = from.ws[i] = 0; continue; }
                if (from.slice_modes[i] != kStackDelta) continue;
                const CollectTask &B = from.tasks[i - 1];
                CollectTask &T = from.tasks[i];
                T.ref = B.src; T.ref_pitch = B.pitch; T.ref_step = B.step;
                from.how[i] = kSrcCollect; from.imgs[i] = nullptr;
            }
        }
    }
    if (from.modes.empty()) return;
    // Colour frames: a channel that the frame's mode codes as a difference becomes a task with the base channel's SOURCE as
    // its reference (collect.h) -- collected even where it could be used in place -- and the others stay what they were.  A
    // frame with a difference and a refused source, or sources of unequal size, is refused as a whole; a frame of mode 0 is
    // three images like any other.
    for (size_t f = 0; f + 2 < count; f += 3) {
        const uint32_t mode = from.modes[f / 3];
        if (mode == kColorPlain) continue;
        bool ok = true;
        for (size_t i = f; i < f + 3; i++) ok = ok && from.how[i] != kSrcRefused && from.hs[i] == from.hs[f] && from.ws[i] == from.ws[f];
        for (size_t i = f; i < f + 3; i++) {
            if (!ok) { from.how[i] = kSrcRefused; from.imgs[i] = nullptr; from.hs[i] = from.ws[i] = 0; continue; }
            const int ref = color_mode_ref(mode, uint32_t(i - f));
            if (ref < 0) continue;
            const CollectTask &B = from.tasks[f + size_t(ref)];
            CollectTask &T = from.tasks[i];
            T.ref = B.src; T.ref_pitch = B.pitch; T.ref_step = B.step;
            from.how[i] = kSrcCollect; from.imgs[i] = nullptr;
        }
    }
}

// Parses and validates the headers, uploads the streams (their lengths are known here: running dry is an error),
// works every (codec, effort) class present through its launches -- `rows` rows of every image per launch, the
// state records carry the images from one launch to the next -- and copies the planes back.  status[k] = 0 / -1.
static bool decode_batch(nblic_amd_ctx *c, int n, const unsigned char *const *streams, const size_t *lens,
                         unsigned char *const *imgs, const size_t *img_caps, int *hs, int *ws, int *nears, int *efforts, int *status,
                         const DeliverTo *to = nullptr) {
    if (hipSetDevice(c->device) != hipSuccess) return false;
    std::vector<DecodeItem> items;
    std::vector<DeliverTask> deliveries;                                // `to`: one per item, in the items' order (below)
    std::vector<std::vector<uint8_t>> qtabs;                            // per QNBLIC item, alive until the copies have been made
    size_t arena = 0;
    for (int k = 0; k < n; k++) {
        status[k] = -1; hs[k] = ws[k] = 0; nears[k] = efforts[k] = 0;
        DecodeItem it{k, 0, 0, 0, 0, 0, 0, 0, -1, -1};
        std::vector<uint8_t> tab;                                        // QNBLIC: histogram tables parsed on the host; a stream whose tables
        const Described r = describe_stream(streams[k], lens[k], false, c->max_px, it, tab);     // do not parse never reaches the GPU
        if (it.h > 0) { hs[k] = it.h; ws[k] = it.w; nears[k] = it.near; efforts[k] = it.effort; }     // the header parsed
        if (r != Described::ok) continue;
        if (to) {                                                        // the planes stay on the device: a window of each goes to the caller's memory there
            DeliverTask T;
            if (!(to->deep_modes ? deep_dest_window(c, *to, k, it.h, it.w, T) : deliver_dest_task(c, *to, k, it.h, it.w, T))) continue;
            T.first_chunk = uint32_t(k);                                 // (until the sort below: the image it belongs to)
            deliveries.push_back(T);
        } else if (size_t(it.h) * size_t(it.w) > img_caps[k]) continue;
        if (it.kind == 1) {
            it.qtab = int(qtabs.size());
            qtabs.push_back(std::move(tab));
        }
        items.push_back(it);
        arena += stream_buf_bytes(it.len) + up256(size_t(it.h) * size_t(it.w)) + up256(lsq_stats_bytes(it.kind, it.effort, it.w)) +
                 up256(record_state_bytes(it.kind)) + (it.kind ? up256(kQTab) : 0);
    }
    if (to && to->modes) {
        // a colour frame with a difference stands or falls as a whole: three lossless planes of one size, three destinations of one window
        auto bytes_of = [](const DecodeItem &it) {
            return stream_buf_bytes(it.len) + up256(size_t(it.h) * size_t(it.w)) + up256(lsq_stats_bytes(it.kind, it.effort, it.w)) + up256(record_state_bytes(it.kind)) + (it.kind ? up256(kQTab) : 0);
        };
        std::vector<int> at(size_t(n), -1);
        for (size_t i = 0; i < items.size(); i++) at[size_t(items[i].k)] = int(i);
        std::vector<uint8_t> keep(items.size(), 0);
        for (int f = 0; f + 2 < n; f += 3) {
            const int a = at[size_t(f)], b = at[size_t(f) + 1], d = at[size_t(f) + 2];
            if (to->mode_of(f) == kColorPlain) {                         // three images like any other
                for (int i : {a, b, d}) if (i >= 0) keep[size_t(i)] = 1;
                continue;
            }
            if (a < 0 || b < 0 || d < 0) continue;
            const DecodeItem &A = items[size_t(a)], &B = items[size_t(b)], &D = items[size_t(d)];
            if (A.h != B.h || A.h != D.h || A.w != B.w || A.w != D.w || A.near || B.near || D.near) continue;
            if (!same_window(deliveries[size_t(a)], deliveries[size_t(b)]) || !same_window(deliveries[size_t(a)], deliveries[size_t(d)])) continue;
            keep[size_t(a)] = keep[size_t(b)] = keep[size_t(d)] = 1;
        }
        std::vector<DecodeItem> kept_items; std::vector<DeliverTask> kept_tasks;
        for (size_t i = 0; i < items.size(); i++) {
            if (keep[i]) { kept_items.push_back(items[i]); kept_tasks.push_back(deliveries[i]); }
            else arena -= bytes_of(items[i]);
        }
        items.swap(kept_items); deliveries.swap(kept_tasks);
    }
    if (to && to->slice_modes) {
        // a stack with a delta stands or falls as a whole: slices of one size and one window, lossless inside its runs
        auto bytes_of = [](const DecodeItem &it) {
            return stream_buf_bytes(it.len) + up256(size_t(it.h) * size_t(it.w)) + up256(lsq_stats_bytes(it.kind, it.effort, it.w)) + up256(record_state_bytes(it.kind)) + (it.kind ? up256(kQTab) : 0);
        };
        std::vector<int> at(size_t(n), -1);
        for (size_t i = 0; i < items.size(); i++) at[size_t(items[i].k)] = int(i);
        std::vector<uint8_t> keep(items.size(), 1);
        for (int s = 0; s + to->depth <= n; s += to->depth) {
            if (!to->stack_has_delta(s)) continue;                       // `depth` images like any other
            bool ok = true;
            for (int k = s; k < s + to->depth && ok; k++) {
                const int i = at[size_t(k)], i0 = at[size_t(s)];
                ok = i >= 0 && i0 >= 0 && items[size_t(i)].h == items[size_t(i0)].h && items[size_t(i)].w == items[size_t(i0)].w &&
                     same_window(deliveries[size_t(i)], deliveries[size_t(i0)]);
                const bool in_run = to->slice_modes[k] == kStackDelta || (k + 1 < s + to->depth && to->slice_modes[k + 1] == kStackDelta);
                ok = ok && !(in_run && items[size_t(i)].near);
            }
            if (!ok) for (int k = s; k < s + to->depth; k++) if (at[size_t(k)] >= 0) keep[size_t(at[size_t(k)])] = 0;
        }
        std::vector<DecodeItem> kept_items; std::vector<DeliverTask> kept_tasks;
        for (size_t i = 0; i < items.size(); i++) {
            if (keep[i]) { kept_items.push_back(items[i]); kept_tasks.push_back(deliveries[i]); }
            else arena -= bytes_of(items[i]);
        }
        items.swap(kept_items); deliveries.swap(kept_tasks);
    }
    if (to && to->deep_modes) {
        // a deep image stands or falls as a whole: two planes of one size
        auto bytes_of = [](const DecodeItem &it) {
            return stream_buf_bytes(it.len) + up256(size_t(it.h) * size_t(it.w)) + up256(lsq_stats_bytes(it.kind, it.effort, it.w)) + up256(record_state_bytes(it.kind)) + (it.kind ? up256(kQTab) : 0);
        };
        std::vector<int> at(size_t(n), -1);
        for (size_t i = 0; i < items.size(); i++) at[size_t(items[i].k)] = int(i);
        std::vector<DecodeItem> kept_items; std::vector<DeliverTask> kept_tasks;
        for (size_t i = 0; i < items.size(); i++) {
            const int other = at[size_t(items[i].k ^ 1)];
            if (other >= 0 && items[size_t(other)].h == items[i].h && items[size_t(other)].w == items[i].w) { kept_items.push_back(items[i]); kept_tasks.push_back(deliveries[i]); }
            else arena -= bytes_of(items[i]);
        }
        items.swap(kept_items); deliveries.swap(kept_tasks);
    }
    if (items.empty()) return true;
    std::stable_sort(items.begin(), items.end(), [](const DecodeItem &a, const DecodeItem &b) { return a.kind * 4 + a.effort < b.kind * 4 + b.effort; });
    const int m = int(items.size());
    HIP_OK(c->dec_arena.reserve(arena)); HIP_OK(c->dec_jobs.reserve(size_t(m)));      // grow-only, like every workspace
    if (to) {
        HIP_OK(c->dec_deliver.reserve(size_t(m)));
        std::vector<DeliverTask> sorted;
        for (const DecodeItem &it : items)
            sorted.push_back(*std::find_if(deliveries.begin(), deliveries.end(), [&](const DeliverTask &T) { return T.first_chunk == uint32_t(it.k); }));
        deliveries.swap(sorted);
    }
    std::vector<SerialJob> jobs(static_cast<size_t>(m));
    std::vector<SerialState> heads(static_cast<size_t>(m));
    std::vector<uint8_t *> d_streams(static_cast<size_t>(m)), d_tabs(static_cast<size_t>(m), nullptr);
    size_t off = 0;
    for (int i = 0; i < m; i++) {                                        // the arena's layout
        const DecodeItem &it = items[size_t(i)];
        d_streams[size_t(i)] = c->dec_arena + off; off += stream_buf_bytes(it.len);
        uint8_t *recon = c->dec_arena + off; off += up256(size_t(it.h) * size_t(it.w));
        const size_t sb = lsq_stats_bytes(it.kind, it.effort, it.w);
        double *stats = sb ? reinterpret_cast<double *>(c->dec_arena + off) : nullptr; off += up256(sb);
        SerialState *state = reinterpret_cast<SerialState *>(c->dec_arena + off); off += up256(record_state_bytes(it.kind));
        if (it.kind == 1) { d_tabs[size_t(i)] = c->dec_arena + off; off += up256(kQTab); }
        jobs[size_t(i)] = decode_job(it, recon, 0, d_streams[size_t(i)], 0, state, stats, d_tabs[size_t(i)], rows_per_launch(it, c->serial_rows), 0, c->d_redo);
        SerialState &H = heads[size_t(i)];
        H = SerialState{};
        H.pos = first_pos(it); H.avail = it.len; H.final_ = 1;
        if (to) {                                                        // gated by the job's record: a stream that fails on the device leaves zeros
            DeliverTask &T = deliveries[size_t(i)];
            T.src = recon; T.src_bytes = up256(size_t(it.h) * size_t(it.w)); T.gate = state;
        }
    }
    const bool rct = to && to->modes, stack = to && to->slice_modes, deep = to && to->deep_modes;
    if (rct) {                                                           // every task of a frame with a difference is gated by its three records; a difference refers to the base's plane
        std::vector<int> at(size_t(n), -1);
        for (int i = 0; i < m; i++) at[size_t(items[size_t(i)].k)] = i;
        for (int i = 0; i < m; i++) {
            const int k = items[size_t(i)].k, f = k - k % 3;
            const uint32_t mode = to->mode_of(k);
            if (mode == kColorPlain) continue;
            DeliverTask &T = deliveries[size_t(i)];
            T.gate = jobs[size_t(at[size_t(f)])].state; T.gate2 = jobs[size_t(at[size_t(f) + 1])].state; T.gate3 = jobs[size_t(at[size_t(f) + 2])].state;
            const int ref = color_mode_ref(mode, uint32_t(k % 3));
            if (ref < 0) continue;
            const DeliverTask &B = deliveries[size_t(at[size_t(f) + size_t(ref)])];
            const size_t skip = size_t(T.row0) * size_t(T.src_pitch);
            T.ref = B.src + skip; T.ref_bytes = B.src_bytes - skip; T.ref_pitch = T.src_pitch;
        }
    }
    // Chunks of one (codec, effort) class, at most kDecodeChunk images each, alternate between two streams: a chunk's uploads,
    // its launches (`rows` rows of every image per launch) and its copies back are all on ITS stream, and the host issues
    // upload + launches of chunk n before it waits for the planes of chunk n - 1 -- so one chunk computes while the other's
    // bytes cross the bus (the caller's memory is pageable: those copies hold the host thread, not the other stream).
    struct Chunk { int i0, i1; hipStream_t st; };
    std::vector<Chunk> chunks;
    for (int i0 = 0; i0 < m;) {
        int i1 = i0 + 1;
        while (i1 < m && i1 - i0 < kDecodeChunk && items[size_t(i1)].kind == items[size_t(i0)].kind && items[size_t(i1)].effort == items[size_t(i0)].effort) i1++;
        chunks.push_back(Chunk{i0, i1, (chunks.size() & 1) ? c->dec_stream2 : c->dec_stream});
        i0 = i1;
    }
    auto fail = [&](const char *what) {
        fprintf(stderr, "[nblic_amd] decode: %s failed\n", what);
        hipStreamSynchronize(c->dec_stream); hipStreamSynchronize(c->dec_stream2);
        if (to && to->deep_modes) {
            std::vector<const DeliverTask *> of(size_t(n), nullptr);
            for (size_t i = 0; i < items.size(); i++) of[size_t(items[i].k)] = &deliveries[i];
            deliver_deep_zeros(*to, of, c->dec_stream);
        } else if (to) deliver_zeros(deliveries, c->dec_stream);
        return false;
    };
    auto upload_and_launch = [&](const Chunk &ch) {
        hipStream_t st = ch.st;
        for (int i = ch.i0; i < ch.i1; i++) {
            const DecodeItem &it = items[size_t(i)];
            const SerialJob &J = jobs[size_t(i)];
            if (J.stats && hipMemsetAsync(J.stats, 0, lsq_stats_bytes(it.kind, it.effort, it.w), st) != hipSuccess) return false;
            if (!upload_stream(d_streams[size_t(i)], streams[it.k], it.len, st)) return false;
            if (hipMemcpyAsync(J.state, &heads[size_t(i)], sizeof(SerialState), hipMemcpyHostToDevice, st) != hipSuccess) return false;
            if (it.kind == 1 && hipMemcpyAsync(d_tabs[size_t(i)], qtabs[size_t(it.qtab)].data(), kQTab, hipMemcpyHostToDevice, st) != hipSuccess) return false;
        }
        if (hipMemcpyAsync(c->dec_jobs + ch.i0, jobs.data() + ch.i0, size_t(ch.i1 - ch.i0) * sizeof(SerialJob), hipMemcpyHostToDevice, st) != hipSuccess) return false;
        int launches = 1;
        for (int i = ch.i0; i < ch.i1; i++) launches = std::max(launches, serial_launches(jobs[size_t(i)].h, jobs[size_t(i)].rows));
        for (int l = 0; l < launches; l++)
            if (!decode_launch(items[size_t(ch.i0)], c->dec_jobs + ch.i0, jobs.data() + ch.i0, ch.i1 - ch.i0, st, true)) return false;
        { std::lock_guard<std::mutex> l(c->stat_m); c->serial_launch_count += launches; }
        return true;
    };
    auto download = [&](const Chunk &ch) {
        for (int i = ch.i0; i < ch.i1; i++) {
            const DecodeItem &it = items[size_t(i)];
            if (hipMemcpyAsync(&heads[size_t(i)], jobs[size_t(i)].state, sizeof(SerialState), hipMemcpyDeviceToHost, ch.st) != hipSuccess) return false;
            if (!to && hipMemcpyAsync(imgs[it.k], jobs[size_t(i)].recon, size_t(it.h) * size_t(it.w), hipMemcpyDeviceToHost, ch.st) != hipSuccess) return false;
        }
        // the chunk's windows: ONE launch on its stream, behind its decode launches (colour frames: one for the call, below)
        return !to || rct || stack || deep || deliver_queue(deliveries.data() + ch.i0, size_t(ch.i1 - ch.i0), c->dec_deliver + ch.i0, ch.st, c);
    };
    for (size_t n = 0; n < chunks.size(); n++) {
        if (n >= 2 && hipStreamSynchronize(chunks[n].st) != hipSuccess) return fail("a chunk");      // heads[] of chunk n - 2 have landed before its stream is reused (its H2D reads heads of chunk n)
        if (!upload_and_launch(chunks[n])) return fail("a launch");
        if (n >= 1 && !download(chunks[n - 1])) return fail("a copy");
    }
    if (!download(chunks.back())) return fail("a copy");
    if (rct) {
        // The planes of a frame may lie in chunks of both streams, and the arena keeps them all: ONE delivery launch for the
        // call on the first stream, behind an event that marks the end of the second one's work.
        Event done2;
        if (done2.create(hipEventDisableTiming) != hipSuccess || hipEventRecord(done2, c->dec_stream2) != hipSuccess ||
            hipStreamWaitEvent(c->dec_stream, done2, 0) != hipSuccess ||
            !deliver_queue(deliveries.data(), deliveries.size(), c->dec_deliver, c->dec_stream, c)) return fail("the colour delivery");
        if (hipStreamSynchronize(c->dec_stream) != hipSuccess) return fail("the colour delivery");      // (done2 goes when this block ends)
    }
    if (stack) {
        // As for colour frames: the planes of a run may lie in chunks of both streams.  ONE k_deliver launch for the lone key
        // slices and ONE k_deliver_stack launch for the runs, on the first stream behind the end of the second one's work.
        std::vector<const DeliverTask *> of(size_t(n), nullptr);
        for (int i = 0; i < m; i++) of[size_t(items[size_t(i)].k)] = &deliveries[size_t(i)];
        StackDelivery plan;
        stack_delivery_plan(*to, n, of, plan);                           // (no more plain tasks than items: dec_deliver holds them)
        Event done2;
        if (c->dec_runs.reserve(std::max<size_t>(plan.runs.size(), 1)) != hipSuccess || c->dec_slices.reserve(std::max<size_t>(plan.slices.size(), 1)) != hipSuccess ||
            done2.create(hipEventDisableTiming) != hipSuccess || hipEventRecord(done2, c->dec_stream2) != hipSuccess ||
            hipStreamWaitEvent(c->dec_stream, done2, 0) != hipSuccess ||
            !stack_delivery_queue(c, plan, c->dec_deliver, c->dec_runs, c->dec_slices, c->dec_stream)) return fail("the stack delivery");
        if (hipStreamSynchronize(c->dec_stream) != hipSuccess) return fail("the stack delivery");      // (done2 goes when this block ends)
        stack_delivery_timed(c, plan);
    }
    if (deep) {
        // As for colour frames: the two planes of an image may lie in chunks of both streams.  ONE k_deliver_deep launch for
        // the call, a task per deep image gated by both planes' records, on the first stream behind the second one's work.
        std::vector<int> at(size_t(n), -1);
        for (int i = 0; i < m; i++) at[size_t(items[size_t(i)].k)] = i;
        std::vector<DeepDeliverTask> tasks;
        for (int k = 0; k + 1 < n; k += 2)
            if (at[size_t(k)] >= 0 && at[size_t(k) + 1] >= 0) tasks.push_back(deep_deliver_task(*to, k / 2, deliveries[size_t(at[size_t(k)])], deliveries[size_t(at[size_t(k) + 1])]));
        Event done2, marks[2];
        if (c->dec_deep.reserve(std::max<size_t>(tasks.size(), 1)) != hipSuccess ||
            done2.create(hipEventDisableTiming) != hipSuccess || hipEventRecord(done2, c->dec_stream2) != hipSuccess ||
            hipStreamWaitEvent(c->dec_stream, done2, 0) != hipSuccess ||
            !deliver_deep_queue(c, tasks.data(), tasks.size(), c->dec_deep, c->dec_stream, marks)) return fail("the deep delivery");
        if (hipStreamSynchronize(c->dec_stream) != hipSuccess) return fail("the deep delivery");       // (done2 goes when this block ends)
        deep_timed(c, marks, 2);
    }
    if (hipStreamSynchronize(c->dec_stream) != hipSuccess || hipStreamSynchronize(c->dec_stream2) != hipSuccess) return fail("the last chunk");
    for (int i = 0; i < m; i++) status[items[size_t(i)].k] = heads[size_t(i)].status == kDone ? 0 : -1;
    if (deep)                                                            // what the gates did on the device: an image with a failed plane has zeros
        for (int k = 0; k + 1 < n; k += 2)
            if (status[k] != 0 || status[k + 1] != 0) status[k] = status[k + 1] = -1;
    if (stack)                                                           // what the gates did on the device: behind a failed plane of a run, no delivered slice has its pixels
        for (int s = 0; s + to->depth <= n; s += to->depth)
            for (int d = 1, bad = status[s] != 0; d < to->depth; d++) {
                if (to->slice_modes[s + d] == kStackKey) bad = 0;
                bad = bad || status[s + d] != 0;
                if (bad && !to->skipped(s + d)) status[s + d] = -1;
            }
    if (rct)                                                             // what the gates did on the device: a frame with a failed plane has none
        for (int f = 0; f + 2 < n; f += 3)
            if (to->mode_of(f) != kColorPlain && (status[f] != 0 || status[f + 1] != 0 || status[f + 2] != 0)) status[f] = status[f + 1] = status[f + 2] = -1;
    return true;
}

// ---- the drop-in decoders: a stream whose length nobody tells us ------------------------------------
// The reference's decoders take no length (NBLIC.h:72, QNBLIC.h:16): they read what the encoder wrote, byte by byte.
// The shims run a band decoder (nblic_amd_dstream, decode_dropin below) and feed it the stream in steps of `feed_chunk`
// bytes ON DEMAND -- it asks for input when the kernel stops in front of a row it is about to run short in (SerialState
// kStarved), the next step is copied in, it goes on -- so that no byte beyond what the decoder consumes plus one step
// and the starvation margin is read from the caller's buffer.  Every step is copied by the KERNEL (write(2) into a
// pipe, read back): where the caller's memory ends (the next page unmapped or protected, a file mapping past its end)
// the copy comes back short instead of raising a signal, and a stream that sits right at the end of a mapping is read
// exactly to its last byte.
static size_t safe_copy(nblic_amd_ctx *c, void *dst, const void *src, size_t n) {
    if (c->feed_pipe[0] < 0) {
        if (pipe(c->feed_pipe) != 0) { c->feed_pipe[0] = c->feed_pipe[1] = -1; return 0; }
        // never block: nobody else reads this pipe, so a write that does not fit would wait for ever (a process over its
        // pipe quota gets single-page pipes)
        fcntl(c->feed_pipe[1], F_SETFL, fcntl(c->feed_pipe[1], F_GETFL) | O_NONBLOCK);
        fcntl(c->feed_pipe[0], F_SETFD, FD_CLOEXEC); fcntl(c->feed_pipe[1], F_SETFD, FD_CLOEXEC);
    }
    const size_t page = size_t(sysconf(_SC_PAGESIZE));
    const long pipe_cap = fcntl(c->feed_pipe[1], F_GETPIPE_SZ);
    const size_t burst = pipe_cap >= long(page) ? (size_t(pipe_cap) < size_t(65536) ? size_t(pipe_cap) & ~(page - 1) : size_t(65536)) : page;
    size_t done = 0;
    while (done < n) {
        // The pipe takes a write in page-sized pieces and DROPS a piece it could only copy in part, so the pieces have to
        // coincide with the source's pages: first the bytes up to the next page boundary, then whole pages (64 KB at a time:
        // what a fresh pipe holds, so the write never blocks).  A write that comes back short then ends exactly where the
        // readable memory ends.
        const size_t addr = size_t(reinterpret_cast<uintptr_t>(src)) + done;
        const size_t to_boundary = page - (addr & (page - 1));
        size_t want = (addr & (page - 1)) ? to_boundary : burst;               // what the pipe holds: a short return then means "memory ends", never "pipe full"
        if (want > n - done) want = n - done;
        const ssize_t k = write(c->feed_pipe[1], static_cast<const char *>(src) + done, want);
        if (k <= 0) break;                                                          // EFAULT: not one more byte can be read
        size_t got = 0;
        while (got < size_t(k)) {
            const ssize_t r = read(c->feed_pipe[0], static_cast<char *>(dst) + done + got, size_t(k) - got);
            if (r <= 0) return done + got;
            got += size_t(r);
        }
        done += size_t(k);
        if (size_t(k) < want) break;                                                // stopped at the end of the readable memory
    }
    return done;
}

// ---- one image in ROW BANDS: bounded workspace, bounded launches, suspend and resume ----------------
// The serial modes' model stage is resumable row by row (serial_engine.h), and the entropy stages carry their
// adaptive state -- the 512 re-mappers, the 4096 counters -- in small per-image tables from launch to launch
// (kernels_e1.hip k_mapper_chains / k_counter_epochs read and write map_state / cnt_state).  So an image of any
// size can be worked through band by band: model stage for the band's rows -> re-mapper partition and chains,
// binarisation, counter partition, epochs, probabilities, mix for THOSE pixels -> the band's coded bins to the
// host -> the range coder, which is resumable too, carries on.  The device workspace is that of one band
// (config 5 of BASELINE.json, 268 Mpixel at effort 3, would need 32 GB in one piece), no kernel runs longer than
// a band, and between bands EVERYTHING the encoder carries is small enough to be written down: a checkpoint
// (model state record, the least-squares column statistics, the two tables, the coder interval, a running SHA-256
// of the bytes emitted so far) from which another call -- another process -- carries on.
// The checkpoint is framed as the decoder's (DecodeCheckpoint): a head with its format version and body length, the body,
// sealed.  Every field is checked on the host (stream_check) before a resume allocates anything.
constexpr uint32_t kEncodeCheckpointVersion = 1;
struct EncodeCheckpoint {               // followed by: model state record | B | map_state | cnt_state | two rows above next_row (if kept) | SHA-256 of all before it
    char magic[8];                      // "NBLECKPT"
    uint32_t version;                   // kEncodeCheckpointVersion
    int32_t h, w, near, effort, band_rows, next_row;
    uint32_t lo, hi;                    // coder interval (NBLIC.c:527-533)
    uint32_t reserved;                  // zero
    unsigned long long bytes_total;     // stream bytes emitted so far, header included
    Sha256 sha;                         // of exactly those bytes
    unsigned long long stats_bytes, recon_bytes;   // of B and of the rows above (0 or 2 w)
    unsigned long long body_bytes;      // bytes between this head and the checksum
};
static_assert(sizeof(EncodeCheckpoint) == 184 && std::is_trivially_copyable<EncodeCheckpoint>::value, "written and read as bytes");
constexpr size_t kMapStateBytes = 512 * 60 * sizeof(int), kCntStateBytes = 4096 * 2 * sizeof(int);

// near > 0, or rows too wide for the model kernel's LDS: the encoder keeps a whole reconstruction on the device
static bool encoder_keeps_recon(int near, int w) { return near > 0 || !serial_model_rows_fit(w); }

// Where the parts of an encoder checkpoint's body are, in bytes from its start (the model state record is at 0).
struct EncodeLayout { size_t b, b_bytes, map, cnt, rows, rows_bytes, bytes; };
static EncodeLayout encode_layout(int w, int near, int effort) {
    EncodeLayout L;
    L.b = kModelStateBytes;
    L.b_bytes = lsq_stats_bytes(0, effort, w) / 2;                       // the column statistics B; the row pre-pass F is recomputed
    L.map = L.b + L.b_bytes;
    L.cnt = L.map + kMapStateBytes;
    L.rows = L.cnt + kCntStateBytes;
    L.rows_bytes = encoder_keeps_recon(near, w) ? 2 * size_t(w) : 0;
    L.bytes = L.rows + L.rows_bytes;
    return L;
}

// Every field of an encoder checkpoint, on the host alone.  0 = valid (head filled in), -1 = refused.
static int stream_check(const void *ck, size_t len, long max_px, EncodeCheckpoint &H) {
    const uint8_t *body = sealed_body(ck, len, "NBLECKPT", kEncodeCheckpointVersion, H);
    if (!body || !codec_fields_ok(0, H.h, H.w, H.near, k_step_for_near(H.near), H.effort, max_px) || H.reserved != 0) return -1;
    if (H.band_rows < 1 || H.band_rows > H.h || H.next_row < 1 || H.next_row >= H.h) return -1;
    if (H.bytes_total == 0 || H.sha.total != H.bytes_total || H.lo >= H.hi) return -1;
    const EncodeLayout L = encode_layout(H.w, H.near, H.effort);
    if (H.stats_bytes != L.b_bytes || H.recon_bytes != L.rows_bytes || H.body_bytes != L.bytes || len != sizeof H + L.bytes + 32) return -1;
    SerialState S;
    memcpy(&S, body, sizeof S);
    if (S.status != kRunning || S.next_row != H.next_row) return -1;
    if (!finite_doubles(body + L.b, L.b_bytes)) return -1;
    int32_t st[60];
    for (int m = 0; m < 512; m++) {                                      // k_mapper_chains: symbol -> rank, rank -> symbol, hit counts
        memcpy(st, body + L.map + size_t(m) * sizeof st, sizeof st);
        if (!remapper_ok(st, st + kMapSyms)) return -1;
    }
    for (int k = 0; k < 4096; k++) {                                     // k_counter_epochs: {c0, c1}
        int32_t c[2];
        memcpy(c, body + L.cnt + size_t(k) * sizeof c, sizeof c);
        if (!counter_ok(c[0], c[1])) return -1;
    }
    return 0;
}

}  // namespace nblic

struct nblic_amd_stream {
    nblic_amd_ctx *c = nullptr;
    int gid = -1;
    int h = 0, w = 0, near = 0, effort = 1, k_step = 3, band_rows = 1, next_row = 0;
    int first_row = 0;                                                  // the first row THIS object coded (> 0 after a resume)
    const uint8_t *d_img = nullptr; nblic::DevBuf<uint8_t> own_img;    // the whole plane on the device (the caller's, or a copy)
    nblic::DevBuf<uint8_t> d_recon;                                     // whole reconstruction (near > 0 or rows too wide for LDS)
    nblic::DevBuf<double> d_stats; size_t stats_bytes = 0;              // [B | F], efforts 2 / 3
    nblic::DevBuf<uint16_t> d_coded;                                    // one band's coded bins
    nblic::Locked h_coded;                                              // the same, page-locked host memory
    uint32_t lo = 0, hi = 0xFFFFFFFFu;
    unsigned long long bytes_total = 0;
    nblic::Sha256 sha;
    bool finished = false, failed = false;
    bool ran = false;                                                   // this object's first _run has been called
    int front = 0;                                                      // nblic_amd_stream_set_front: 0 serial model stage, 1 staged kernels (-n0 -e1 only)
    long bands = 0;
    double model_ms = 0;
    // seek index (nblic_amd_stream_set_index): an entry in front of every row index_every, 2 index_every, ...  An entry
    // waits for the four stream bytes that follow its position (the decoder's window) before it is sealed.
    int index_every = 0;
    nblic::PendingEntries pending;                                      // (index_entries.h) views of the entries below that still wait
    std::vector<std::vector<uint8_t>> entries;                          // in row order; sealed unless `pending` still names it
    nblic::Sha256 rows_sha;                                             // of the reconstruction rows coded so far
    std::vector<uint8_t> band_rows_host;
};

namespace nblic {

static void stream_free(nblic_amd_stream *s) {
    if (!s) return;
    nblic_amd_ctx *const c = s->c; const int gid = s->gid;
    if (c) hipSetDevice(c->device);
    delete s;                                                            // its buffers, before the group serves somebody else
    if (c && gid >= 0) release_group(c, gid);
}

// The rows per band of an encoder: what its caller asks for, or what one launch covers.
static int encoder_band_rows(int band_rows, int h, int w, int effort) { return band_rows > 0 ? std::min(band_rows, h) : serial_rows_per_launch(h, w, effort, 0); }

static nblic_amd_stream *stream_open(nblic_amd_ctx *c, const unsigned char *img, bool on_device, int h, int w, int near, int effort, int band_rows) {
    if (!c || !img || !size_ok(h, w, c->max_px) || hipSetDevice(c->device) != hipSuccess) return nullptr;
    auto *s = new nblic_amd_stream;
    s->c = c; s->h = h; s->w = w; s->near = iclip(near, 0, kMaxNear); s->effort = iclip(effort, 1, 3); s->k_step = k_step_for_near(s->near);
    s->band_rows = encoder_band_rows(band_rows, h, w, s->effort);
    s->gid = take_group(c);   // for as long as the stream lives: its first slot's band workspace, its stream, its pinned job records
    Group &g = c->groups[size_t(s->gid)];
    const size_t n = size_t(h) * size_t(w);
    bool ok = true;
    if (on_device) s->d_img = img;
    else ok = s->own_img.alloc(n) == hipSuccess && hipMemcpyAsync(s->own_img, img, n, hipMemcpyHostToDevice, g.stream) == hipSuccess && (s->d_img = s->own_img, true);
    if (ok && encoder_keeps_recon(s->near, w)) ok = s->d_recon.alloc(n) == hipSuccess;
    s->stats_bytes = lsq_stats_bytes(0, s->effort, w);
    if (ok && s->stats_bytes) ok = s->d_stats.alloc(s->stats_bytes / sizeof(double)) == hipSuccess && hipMemsetAsync(s->d_stats, 0, s->stats_bytes, g.stream) == hipSuccess;   // NBLIC.c:789
    Slot &sl = g.slots[0];
    ok = ok && ensure_pixels(sl, size_t(s->band_rows) * size_t(w));
    if (!ok) { fprintf(stderr, "[nblic_amd] stream: cannot set up the band workspace\n"); stream_free(s); return nullptr; }
    return s;
}

// the band workspace as the kernels see it for the band that starts at row i0: the band's rows of the plane, the band's bins
static E1Buffers stream_band_buffers(const nblic_amd_stream *s, const Slot &sl, int i0) {
    E1Buffers b = sl.b;
    b.img = s->d_img + size_t(i0) * size_t(s->w); b.coded = s->d_coded;
    return b;
}

// the front-half job records of the band that starts at row i0
static void stream_band_jobs(nblic_amd_stream *s, Group &g, int i0, int rows) {
    const Slot &sl = g.slots[0];
    g.h_jobs[0] = band_job_front(g.ctx, stream_band_buffers(s, sl, i0), s->d_img, i0, rows, s->w, s->near);
    g.h_sjobs[0] = model_job(s->d_img, s->d_recon, sl.b, s->d_stats, sl.d_state, s->h, s->w, s->near, s->effort, rows, i0, g.ctx->d_redo);
}

// ---- the STAGED front of a band (nblic_amd_stream_set_front, -n0 -e1) ------------------------------------------------
// Lossless -e1 has no prediction chain (kernels_e1.hip S1), so a band's model stage can run on the key-partitioned
// kernels instead of the one wave of k_serial_model.  The model state record stays what the encoder carries from band
// to band -- checkpoints and index entries are read from it -- so a staged band takes the record's biases into
// ctx_state, runs S1 .. S2 .. on its rows (e1_launch_front_band: every chain starts from its table entry and writes
// its end state back), and leaves the record as k_serial_model<0, 1> leaves it after the same rows: next_row, status,
// `bias` (never moved at effort 1: lsq::kBiasInit), and the biases -- which the model kernel does not write back after
// the image's last row.
__global__ void __launch_bounds__(256) k_band_record_out(SerialState *__restrict__ st, const int *__restrict__ ctx_state, int next_row, int done) {
    const int k = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (!done && k < kContexts) reinterpret_cast<int *>(st + 1)[k] = ctx_state[k];
    if (k == 0) { st->next_row = next_row; st->bias = lsq::kBiasInit; st->status = done ? kDone : kRunning; }
}

// The front half of the band [i0, i0 + rows) on the staged kernels; e_model is recorded behind the last launch of S2.
static bool stream_front_staged(nblic_amd_stream *s, Group &g, int i0, int rows, hipEvent_t e_model) {
    Slot &sl = g.slots[0];
    const hipStream_t st = g.stream;
    // row 0: k_init_state has zeroed ctx_state, and the record's table is not written yet (the model kernel starts from zeros too)
    if (i0 > 0 && hipMemcpyAsync(sl.b.ctx_state, reinterpret_cast<const int *>(sl.d_state + 1), size_t(kContexts) * sizeof(int),
                                 hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    e1_launch_front_band(g.d_jobs, g.h_jobs, 1, st, e_model);
    hipLaunchKernelGGL(k_band_record_out, dim3(kContexts / 256), dim3(256), 0, st, sl.d_state, sl.b.ctx_state, i0 + rows, int(i0 + rows >= s->h));
    // rows too wide for the model kernel's LDS: the encoder keeps a reconstruction, which the checkpoint's two rows come from
    const size_t at = size_t(i0) * size_t(s->w);
    if (s->d_recon.get() && hipMemcpyAsync(s->d_recon.get() + at, s->d_img + at, size_t(rows) * size_t(s->w), hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    return hipGetLastError() == hipSuccess;
}

static bool stream_index_band(nblic_amd_stream *s, int i0, int rows, bool entry, const uint8_t *out, const uint8_t *end, uint32_t lo, uint32_t hi);
static void stream_index_bytes(nblic_amd_stream *s, const uint8_t *out, const uint8_t *end);

// Runs bands until the image is finished or the budget is spent.  1 finished, 0 suspended between two bands, -1 error.
static int stream_run(nblic_amd_stream *s, double budget_s, unsigned char *out, size_t cap, size_t *out_len) {
    *out_len = 0;
    if (!s || s->failed) return -1;
    if (s->finished) return 1;
    nblic_amd_ctx *c = s->c;
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    s->ran = true;
    const bool staged = s->front == 1;
    Group &g = c->groups[size_t(s->gid)];
    Slot &sl = g.slots[0];
    const auto t0 = std::chrono::steady_clock::now();
    auto fail = [&](const char *what) { fprintf(stderr, "[nblic_amd] stream: %s\n", what); s->failed = true; hipStreamSynchronize(g.stream); return -1; };
    uint8_t *p = out;
    if (s->bytes_total == 0) {                                          // a fresh image: header, tables, state record
        if (cap < size_t(kHeaderBytes) + 4) return fail("output buffer too small");
        write_header(p, s->h, s->w, s->near, s->k_step, s->effort);
        p += kHeaderBytes;
        stream_band_jobs(s, g, 0, 1);
        if (hipMemcpyAsync(g.d_jobs, g.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, g.stream) != hipSuccess) return fail("upload");
        e1_launch_init(g.d_jobs, 1, g.stream);
        if (hipMemsetAsync(sl.d_state, 0, sizeof(SerialState), g.stream) != hipSuccess) return fail("state");
    }
    RangeScalar rc;
    rc.begin(p, cap - size_t(p - out));
    rc.lo = s->lo; rc.hi = s->hi;
    while (s->next_row < s->h) {
        const int i0 = s->next_row;
        const BandCut cut = index_band_cut(i0, s->band_rows, s->h, s->index_every);      // a band never crosses an entry row
        const int rows = cut.rows;
        stream_band_jobs(s, g, i0, rows);
        hipEvent_t e0 = g.tm.ev[0], e1 = g.tm.ev[1];
        if (hipMemcpyAsync(g.d_jobs, g.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, g.stream) != hipSuccess ||
            (!staged && hipMemcpyAsync(g.d_sjobs, g.h_sjobs, sizeof(SerialJob), hipMemcpyHostToDevice, g.stream) != hipSuccess)) return fail("upload");
        hipEventRecord(e0, g.stream);
        if (staged) {
            if (!stream_front_staged(s, g, i0, rows, e1)) return fail("staged front");
        } else {
            if (!serial_model_launch(g.d_sjobs, g.h_sjobs, 1, g.stream)) return fail("model launch");
            hipEventRecord(e1, g.stream);
            e1_launch_front_pre(g.d_jobs, g.h_jobs, 1, g.stream);
        }
        if (hipMemcpyAsync(g.h_totals, g.d_totals, kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
            hipStreamSynchronize(g.stream) != hipSuccess) return fail("front half");
        { float ms = 0.f; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) s->model_ms += ms; }
        const uint32_t n_ev = g.h_totals[2];
        count_long_chains(g.ctx, g.h_totals);
        if (n_ev >= 0x7FFFFFFFu || !ensure_events(sl, n_ev)) return fail("bin count");
        if (size_t(n_ev) + 8 > std::min(s->d_coded.capacity(), s->h_coded.capacity())) {
            const size_t cap = size_t(n_ev) + size_t(n_ev) / 4 + 4096;
            if (s->d_coded.alloc(cap) != hipSuccess) return fail("coded bins");
            if (!s->h_coded.alloc(cap)) return fail("pinned bins");
        }
        e1_job_back(g.h_jobs[0], stream_band_buffers(s, sl, i0), n_ev);
        if (hipMemcpyAsync(g.d_jobs, g.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, g.stream) != hipSuccess) return fail("upload");
        e1_launch_back(g.d_jobs, g.h_jobs, 1, g.stream, nullptr, true);
        if (n_ev && hipMemcpyAsync(s->h_coded, s->d_coded, size_t(n_ev) * sizeof(uint16_t), hipMemcpyDeviceToHost, g.stream) != hipSuccess) return fail("bins to the host");
        if (hipStreamSynchronize(g.stream) != hipSuccess) return fail("back half");
        rc.feed(s->h_coded, n_ev);
        if (rc.overflow) return fail("output buffer too small");
        s->next_row = i0 + rows; s->bands++;
        if (!staged) { std::lock_guard<std::mutex> l(c->stat_m); c->serial_launch_count++; }
        if (s->index_every > 0 && !stream_index_band(s, i0, rows, cut.entry, out, rc.p, rc.lo, rc.hi)) return fail("index entry");
        if (budget_s > 0 && s->next_row < s->h && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= budget_s) break;
    }
    s->lo = rc.lo; s->hi = rc.hi;
    size_t n = size_t(rc.p - out);
    if (s->next_row >= s->h) {
        const size_t body = rc.finish();                                 // the four flush bytes (NBLIC.c:576-586)
        if (body == SIZE_MAX) return fail("output buffer too small");
        n = size_t(rc.p - out);
        s->finished = true;
    }
    if (s->index_every > 0) stream_index_bytes(s, out, out + n);
    s->sha.update(out, n);
    s->bytes_total += n;
    *out_len = n;
    return s->finished ? 1 : 0;
}

// The checkpoint of an encoder between two bands; 0 when there is nothing to resume (never run, finished or failed: a
// finished encoder resumed would emit its four flush bytes again).
static size_t stream_checkpoint(nblic_amd_stream *s, void *buf, size_t cap) {
    if (s->failed || s->finished || s->bytes_total == 0) return 0;
    const EncodeLayout L = encode_layout(s->w, s->near, s->effort);
    const size_t need = sizeof(EncodeCheckpoint) + L.bytes + 32;
    if (!buf || cap < need) return need;
    if (hipSetDevice(s->c->device) != hipSuccess) return 0;
    Group &g = s->c->groups[size_t(s->gid)];
    Slot &sl = g.slots[0];
    EncodeCheckpoint H{};
    memcpy(H.magic, "NBLECKPT", 8);
    H.version = kEncodeCheckpointVersion;
    H.h = s->h; H.w = s->w; H.near = s->near; H.effort = s->effort; H.band_rows = s->band_rows; H.next_row = s->next_row;
    H.lo = s->lo; H.hi = s->hi; H.bytes_total = s->bytes_total; H.sha = s->sha;
    H.stats_bytes = L.b_bytes; H.recon_bytes = L.rows_bytes; H.body_bytes = L.bytes;
    uint8_t *p = static_cast<uint8_t *>(buf), *body = p + sizeof H;
    memcpy(p, &H, sizeof H);
    const hipStream_t st = g.stream;
    bool ok = hipMemcpyAsync(body, sl.d_state, kModelStateBytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
              (!L.b_bytes || hipMemcpyAsync(body + L.b, s->d_stats, L.b_bytes, hipMemcpyDeviceToHost, st) == hipSuccess) &&
              hipMemcpyAsync(body + L.map, sl.b.map_state, kMapStateBytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
              hipMemcpyAsync(body + L.cnt, sl.b.cnt_state, kCntStateBytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
              (!L.rows_bytes || rows_above_out(body + L.rows, s->d_recon, 0, s->next_row, s->w, st)) &&
              hipStreamSynchronize(st) == hipSuccess;
    if (!ok) return 0;
    seal(p, need);
    return need;
}

static nblic_amd_stream *stream_resume(nblic_amd_ctx *c, const unsigned char *img, bool on_device, const void *ck, size_t ck_len) {
    EncodeCheckpoint H;
    if (!c || stream_check(ck, ck_len, c->max_px, H) != 0) return nullptr;
    nblic_amd_stream *s = stream_open(c, img, on_device, H.h, H.w, H.near, H.effort, H.band_rows);
    if (!s) return nullptr;
    const EncodeLayout L = encode_layout(H.w, H.near, H.effort);
    Group &g = c->groups[size_t(s->gid)];
    Slot &sl = g.slots[0];
    s->next_row = s->first_row = H.next_row; s->lo = H.lo; s->hi = H.hi; s->bytes_total = H.bytes_total; s->sha = H.sha;
    const uint8_t *body = static_cast<const uint8_t *>(ck) + sizeof H;
    const hipStream_t st = g.stream;                                     // behind stream_open's uploads
    const bool ok = hipMemcpyAsync(sl.d_state, body, kModelStateBytes, hipMemcpyHostToDevice, st) == hipSuccess &&
                    (!L.b_bytes || hipMemcpyAsync(s->d_stats, body + L.b, L.b_bytes, hipMemcpyHostToDevice, st) == hipSuccess) &&
                    hipMemcpyAsync(sl.b.map_state, body + L.map, kMapStateBytes, hipMemcpyHostToDevice, st) == hipSuccess &&
                    hipMemcpyAsync(sl.b.cnt_state, body + L.cnt, kCntStateBytes, hipMemcpyHostToDevice, st) == hipSuccess &&
                    (!L.rows_bytes || rows_above_in(s->d_recon, 0, body + L.rows, s->next_row, s->w, st)) &&
                    hipStreamSynchronize(st) == hipSuccess;
    if (!ok) { stream_free(s); return nullptr; }
    return s;
}

// ---- a stream decoded in ROW BANDS: bounded workspace, fed piece by piece, rows as they finish ----------------
// The decoders are resumable row by row (serial_engine.h): what crosses a row boundary is the state record, the
// least-squares column statistics B and the two rows above.  So a band decoder needs, whatever the image height:
//   (band_rows + 2) x w reconstruction rows   the two rows above the band at index 0 / 1 (SerialJob::recon_row0), the
//                                             band's rows after them; after a launch the last two rows move to the front
//   2 x w x stats_stride(effort) doubles      [B | F], efforts 2 / 3, plus a snapshot of B (below)
//   one state record, 2 x w bytes of carry, the QNBLIC tables
//   a stream window of win_cap bytes          from absolute offset pos & ~511 (SerialJob::stream_off), + 2 KB of padding
//                                             for the 512-byte block fetches beyond what is there
// The caller's bytes are kept on the host only from the window's base on.  `final_` is set only when the window holds
// the rest of a stream the caller has declared complete; a launch that stops for want of bytes (kStarved) and finds
// nothing more to put in the window returns "needs input" instead of launching again.
//
// kStarvedMidRow (a row dearer than starve_margin(w), i.e. more than four bytes per pixel: no valid stream seen so far
// comes near it) leaves the launch's rows unfinished, and the non-lean decoder -- a band decoder always launches one
// image, so never the lean one -- has then changed nothing in the state record but its status.  What it HAS changed in
// place is B (every pixel's update).  So B is copied aside before every launch of effort 2 / 3 and copied back after a
// mid-row stop; the band is then run again from the same record once the window holds more bytes (the caller feeds more,
// or, when the window was what ran out, the window grows: the only case in which the workspace grows).
// The checkpoint: DecodeCheckpoint (the record layer above).
// Every field of a checkpoint, before anything of it reaches the device.  0 = valid (head filled in), -1 = refused.
// The parts of that check, which a packed index entry (index_pack.h) goes through piece by piece: the head's fields and the
// record's header; the NBLIC tables a resumed launch loads (every value an index can come from); the QNBLIC tables.
static bool checkpoint_fields_ok(const DecodeCheckpoint &H, const SerialState &S, long max_px) {
    if (!codec_fields_ok(H.kind, H.h, H.w, H.near, H.k_step, H.effort, max_px)) return false;
    if (H.band_rows < 1 || H.band_rows > H.h || H.next_row < 0 || H.next_row >= H.h) return false;
    if (H.body_bytes != record_layout(H.kind, H.w, H.effort).bytes) return false;
    if (H.rows_sha.total != (unsigned long long)(H.next_row) * (unsigned long long)(H.w)) return false;
    const unsigned long long first = H.kind ? 8 : (unsigned long long)(kHeaderBytes);
    return S.status == kRunning && S.next_row == H.next_row && S.pos >= first && S.pos < kMaxStreamPos && (S.pos & ~511ull) == H.feed_from;
}
static bool nblic_tables_ok(const uint8_t *cnt, const uint8_t *rank, const uint8_t *sym) {
    for (int k = 0; k < kLevels * kTreeNodes; k++) {
        uint32_t c;
        memcpy(&c, cnt + size_t(k) * 4, 4);
        if (!counter_ok(int(c & 0xFFFFu), int(c >> 16))) return false;
    }
    for (int m = 0; m < 512; m++)
        if (!remapper_ok(rank + m * kMapSyms, sym + m * kMapSyms)) return false;
    return true;
}
static bool qtab_ok(const uint8_t *tab) {                                 // the twelve frequency tables and their cumulative starts
    std::vector<uint32_t> t(2 * 12 * 256);
    memcpy(t.data(), tab, kQTab);
    const uint32_t *freq = t.data(), *start = t.data() + 12 * 256;
    for (int l = 0; l < 12; l++) {
        uint32_t acc = 0;
        for (int s = 0; s < 256; s++) {
            if (start[l * 256 + s] != acc || freq[l * 256 + s] > 32768u) return false;
            acc += freq[l * 256 + s];
        }
        if (acc != 32768u) return false;
    }
    return true;
}
static int dstream_check(const void *ck, size_t len, long max_px, DecodeCheckpoint &H) {
    const uint8_t *body = sealed_body(ck, len, "NBLDCKPT", kDecodeCheckpointVersion, H);
    if (!body || !codec_fields_ok(H.kind, H.h, H.w, H.near, H.k_step, H.effort, max_px)) return -1;
    const RecordLayout L = record_layout(H.kind, H.w, H.effort);
    if (H.body_bytes != L.bytes || len != sizeof H + H.body_bytes + 32) return -1;
    SerialState S;
    memcpy(&S, body, sizeof S);
    if (!checkpoint_fields_ok(H, S, max_px)) return -1;
    const uint8_t *tab = body + sizeof S;
    if (H.kind == 0 && H.next_row > 0 &&
        !nblic_tables_ok(tab + size_t(kContexts) * 4, tab + size_t(kRecRank) * 4, tab + size_t(kRecSym) * 4)) return -1;
    if (!finite_doubles(body + L.b, L.b_bytes)) return -1;
    if (H.kind == 1 && !qtab_ok(body + L.tab)) return -1;
    return 0;
}

}  // namespace nblic

struct nblic_amd_dstream {
    nblic_amd_ctx *c = nullptr;
    int device = 0;
    nblic::Stream st;                                    // this object's own, or lent by decode_dropin: the context's dec_stream
    int band_rows_req = 0;
    // the header (kind 0 NBLIC, 1 QNBLIC) and the workspace it sizes
    bool have_head = false, refused = false, failed = false, done = false;
    nblic::DecodeItem it{};
    int band_rows = 0;
    nblic::DevPool mem;                                  // owns the workspace: what the pointers below see
    uint8_t *d_rows = nullptr, *d_carry = nullptr, *d_win = nullptr, *d_tab = nullptr;
    double *d_stats = nullptr, *d_snap = nullptr;
    nblic::SerialState *d_state = nullptr;
    nblic::SerialJob *d_job = nullptr;
    size_t stats_bytes = 0, win_cap = 0;
    std::vector<uint8_t> qtab;                           // QNBLIC: host copy of the tables (they travel with a checkpoint)
    // the stream as fed: bytes [pend_off, pend_off + pend.size()) of it; [win_off, win_off + win_len) are on the device
    std::vector<uint8_t> pend;
    unsigned long long pend_off = 0, win_off = 0, win_len = 0;
    bool complete = false;
    // progress
    nblic::SerialState H{};                              // the record's header as of the last finished launch
    int row0 = 0;                                        // image row at d_rows[0]: max(0, H.next_row - 2)
    int stop_row = 0;                                    // > 0: _run stops in front of this row (index_build: the entry rows)
    nblic::Sha256 sha;
    long launches = 0;
};

namespace nblic {

static void dstream_free(nblic_amd_dstream *d) {
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess && d->st) hipStreamSynchronize(d->st);
    delete d;                                                            // the workspace, then the stream
}

static size_t dstream_win_cap(int band_rows, int w) {
    const size_t want = 2 * size_t(band_rows) * size_t(w) + 2 * starve_margin(w);
    const size_t cap = want > (size_t(4) << 20) ? want : (size_t(4) << 20);
    return (cap + 511) & ~size_t(511);
}

// The workspace of a header that has just been parsed (or of a checkpoint): depends on band_rows and w, never on h.
static bool dstream_setup(nblic_amd_dstream *d) {
    const DecodeItem &it = d->it;
    d->band_rows = rows_per_launch(it, d->band_rows_req);
    d->stats_bytes = lsq_stats_bytes(it.kind, it.effort, it.w);
    d->win_cap = dstream_win_cap(d->band_rows, it.w);
    const size_t rows_bytes = size_t(d->band_rows + 2) * size_t(it.w);
    DevPool &m = d->mem;
    bool ok = (d->d_rows = m.make<uint8_t>(rows_bytes)) && (d->d_carry = m.make<uint8_t>(2 * size_t(it.w))) &&
              (d->d_win = m.make<uint8_t>(d->win_cap + 2048)) &&
              (d->d_state = reinterpret_cast<SerialState *>(m.make<uint8_t>(up256(record_state_bytes(it.kind))))) &&
              (d->d_job = m.make<SerialJob>(1));
    if (ok && d->stats_bytes) ok = (d->d_stats = m.make<double>(d->stats_bytes / sizeof(double))) && (d->d_snap = m.make<double>(d->stats_bytes / 2 / sizeof(double))) &&
                                   hipMemsetAsync(d->d_stats, 0, d->stats_bytes, d->st) == hipSuccess;     // NBLIC.c:789
    if (ok && it.kind) ok = (d->d_tab = m.make<uint8_t>(kQTab)) != nullptr;
    ok = ok && hipMemsetAsync(d->d_state, 0, up256(record_state_bytes(it.kind)), d->st) == hipSuccess &&
         hipMemsetAsync(d->d_rows, 0, rows_bytes, d->st) == hipSuccess && hipMemsetAsync(d->d_win, 0, d->win_cap + 2048, d->st) == hipSuccess;
    if (!ok) { fprintf(stderr, "[nblic_amd] band decoder: cannot set up the workspace\n"); m.reset(); return false; }     // (the caller marks d failed or frees it: nothing looks at the workspace again)
    return true;
}

// The header (QNBLIC: and its tables) from the bytes fed so far.  Sets have_head or refused; neither: not all there yet.
static void dstream_try_header(nblic_amd_dstream *d) {
    if (d->have_head || d->refused) return;
    DecodeItem it{0, 0, 0, 0, 0, 0, 0, 0, -1, -1};
    const Described r = describe_stream(d->pend.data(), d->pend.size(), true, d->c->max_px, it, d->qtab);
    if (r != Described::ok) {                                            // what is not there yet never will be once the stream is complete
        if (r == Described::refused || d->complete) d->refused = true;
        return;
    }
    d->it = it;
    if (!dstream_setup(d)) { d->failed = true; return; }
    if (it.kind == 1 && hipMemcpyAsync(d->d_tab, d->qtab.data(), kQTab, hipMemcpyHostToDevice, d->st) != hipSuccess) { d->failed = true; return; }
    d->H = SerialState{};
    d->H.pos = first_pos(it);
    d->win_off = d->win_len = 0;
    d->have_head = true;
}

// Slides the device window to the record's position and tops it up from what has been fed.
static bool dstream_fill_window(nblic_amd_dstream *d) {
    const unsigned long long base = d->H.pos & ~511ull, pend_end = d->pend_off + d->pend.size();
    if (base < d->pend_off) return false;                               // bytes the decoder needs were never fed (resume fed from the wrong offset)
    if (base != d->win_off) { d->win_off = base; d->win_len = 0; }
    const unsigned long long want_end = std::min(pend_end, base + d->win_cap);
    const unsigned long long have_end = d->win_off + d->win_len;
    if (want_end > have_end) {
        if (hipMemcpyAsync(d->d_win + (have_end - base), d->pend.data() + (have_end - d->pend_off), size_t(want_end - have_end), hipMemcpyHostToDevice, d->st) != hipSuccess ||
            hipStreamSynchronize(d->st) != hipSuccess) return false;
        d->win_len = want_end - base;
    }
    if (base > d->pend_off) {                                            // keep only the bytes at or after the window base
        d->pend.erase(d->pend.begin(), d->pend.begin() + ptrdiff_t(base - d->pend_off));
        d->pend_off = base;
    }
    return true;
}

static bool dstream_window_holds_all_fed(const nblic_amd_dstream *d) { return d->win_off + d->win_len == d->pend_off + d->pend.size(); }

// 1 finished, 0 suspended (budget spent, or rows_out full), 2 needs input, -1 error.
static int dstream_run(nblic_amd_dstream *d, double budget_s, unsigned char *rows_out, size_t cap, int *first_row, int *end_row) {
    int first = d->have_head ? d->H.next_row : 0, end = first;
    auto report = [&](int rc) { if (first_row) *first_row = first; if (end_row) *end_row = end; return rc; };
    if (d->failed || d->refused) return report(-1);
    if (d->done) return report(1);
    if (hipSetDevice(d->device) != hipSuccess) return report(-1);
    dstream_try_header(d);
    if (d->failed || d->refused) return report(-1);
    if (!d->have_head) return report(d->complete ? -1 : 2);
    const DecodeItem &it = d->it;
    const size_t w = size_t(it.w);
    first = end = d->H.next_row;
    auto fail = [&](const char *what) { fprintf(stderr, "[nblic_amd] band decoder: %s\n", what); d->failed = true; hipStreamSynchronize(d->st); return report(-1); };
    if (!rows_out || cap < size_t(std::min(d->band_rows, it.h - first)) * w) return report(-1);    // rows_out holds less than the next band (nothing has happened)
    const auto t0 = std::chrono::steady_clock::now();
    size_t written = 0;                                                  // rows in rows_out
    const int limit = d->stop_row > 0 ? std::min(d->stop_row, it.h) : it.h;
    while (d->H.next_row < limit) {
        const int i0 = d->H.next_row, rows = std::min(d->band_rows, limit - i0);
        if ((written + size_t(rows)) * w > cap) return report(0);                 // rows_out is full
        if (!dstream_fill_window(d)) return fail("stream window");
        const bool final_ = d->complete && dstream_window_holds_all_fed(d);
        const SerialJob J = decode_job(it, d->d_rows, d->row0, d->d_win, d->win_off, d->d_state, d->d_stats, d->d_tab, rows, 0, d->c->d_redo);
        SerialState S = d->H;
        S.avail = d->win_off + d->win_len; S.final_ = final_ ? 1 : 0; S.status = kRunning;
        if (d->d_snap && hipMemcpyAsync(d->d_snap, d->d_stats, d->stats_bytes / 2, hipMemcpyDeviceToDevice, d->st) != hipSuccess) return fail("snapshot");
        if (hipMemcpyAsync(d->d_state, &S, sizeof S, hipMemcpyHostToDevice, d->st) != hipSuccess ||
            hipMemcpyAsync(d->d_job, &J, sizeof J, hipMemcpyHostToDevice, d->st) != hipSuccess) return fail("upload");
        if (!decode_launch(it, d->d_job, &J, 1, d->st, false)) return fail("launch");
        if (hipMemcpyAsync(&S, d->d_state, sizeof S, hipMemcpyDeviceToHost, d->st) != hipSuccess || hipStreamSynchronize(d->st) != hipSuccess) return fail("state");
        d->launches++;
        { std::lock_guard<std::mutex> l(d->c->stat_m); d->c->serial_launch_count++; }
        if (S.status == kFailed) return fail("the stream is damaged or ends too early");
        if (S.status == kStarvedMidRow) {
            // nothing of the launch is kept: B back from the snapshot, the record's header is still d->H (see above)
            if (d->d_snap && (hipMemcpyAsync(d->d_stats, d->d_snap, d->stats_bytes / 2, hipMemcpyDeviceToDevice, d->st) != hipSuccess ||
                              hipStreamSynchronize(d->st) != hipSuccess)) return fail("restore");
            if (dstream_window_holds_all_fed(d)) return report(2);       // more bytes have to come first
            // the window itself was too small for the row: grow it (the caller has fed the bytes)
            const size_t cap2 = d->win_cap * 2;
            if (d->mem.renew(d->d_win, cap2 + 2048) != hipSuccess || hipMemsetAsync(d->d_win, 0, cap2 + 2048, d->st) != hipSuccess) return fail("window");
            d->win_cap = cap2; d->win_len = 0;
            continue;
        }
        const int at = S.next_row;
        if (at < i0 || at > i0 + rows) return fail("decoder state");
        if (at > i0) {                                                   // rows [i0, at) are final: to the caller, into the hash, the last two to the front
            const size_t n = size_t(at - i0) * w;
            if (hipMemcpyAsync(rows_out + written * w, d->d_rows + size_t(i0 - d->row0) * w, n, hipMemcpyDeviceToHost, d->st) != hipSuccess) return fail("rows to the host");
            const int r0 = std::max(0, at - 2);
            if (r0 > d->row0) {
                const size_t keep = size_t(at - r0) * w;
                if (hipMemcpyAsync(d->d_carry, d->d_rows + size_t(r0 - d->row0) * w, keep, hipMemcpyDeviceToDevice, d->st) != hipSuccess ||
                    hipMemcpyAsync(d->d_rows, d->d_carry, keep, hipMemcpyDeviceToDevice, d->st) != hipSuccess) return fail("carry");
                d->row0 = r0;
            }
            if (hipStreamSynchronize(d->st) != hipSuccess) return fail("rows to the host");
            d->sha.update(rows_out + written * w, n);
            written += size_t(at - i0);
            end = at;
        }
        const bool moved = S.pos != d->H.pos || at > i0;
        d->H = S;
        d->H.status = kRunning;
        if (S.status == kDone) { d->done = true; break; }
        if (S.status == kStarved && !moved && dstream_window_holds_all_fed(d)) { d->H.status = kRunning; return report(2); }
        if (S.status == kStarved && !moved) return fail("no progress");
        if (budget_s > 0 && d->H.next_row < it.h && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= budget_s) return report(0);
    }
    return report(d->done ? 1 : 0);
}

// The decoder's record in front of row H.next_row, with band_rows and rows_sha as its head is to say (the API: the
// decoder's own; index_build: the index spacing and the canonical row hash).
static size_t dstream_checkpoint(nblic_amd_dstream *d, void *buf, size_t cap, int band_rows, const Sha256 &rows_sha) {
    if (!d->have_head || d->failed || d->done) return 0;
    const DecodeItem &it = d->it;
    const RecordLayout L = record_layout(it.kind, it.w, it.effort);
    const size_t need = sizeof(DecodeCheckpoint) + L.bytes + 32;
    if (!buf || cap < need) return need;
    if (hipSetDevice(d->device) != hipSuccess) return 0;
    const DecodeCheckpoint H = decode_head(it, band_rows, d->H.next_row, d->H.pos & ~511ull, rows_sha);
    uint8_t *p = static_cast<uint8_t *>(buf), *body = p + sizeof H;
    memcpy(p, &H, sizeof H);
    const bool ok = hipMemcpyAsync(body, d->d_state, L.b, hipMemcpyDeviceToHost, d->st) == hipSuccess &&
                    (!L.b_bytes || hipMemcpyAsync(body + L.b, d->d_stats, L.b_bytes, hipMemcpyDeviceToHost, d->st) == hipSuccess) &&
                    rows_above_out(body + L.rows, d->d_rows, d->row0, d->H.next_row, it.w, d->st) &&
                    hipStreamSynchronize(d->st) == hipSuccess;
    if (!ok) return 0;
    SerialState S = d->H;                                                // the header as the host holds it (the device copy may say kStarved)
    S.status = kRunning; S.avail = 0; S.final_ = 0;
    memcpy(body, &S, sizeof S);
    if (it.kind) memcpy(body + L.tab, d->qtab.data(), kQTab);
    seal(p, need);
    return need;
}

// st: a stream the caller keeps for the object's lifetime; nullptr: one of its own
static nblic_amd_dstream *dstream_new(nblic_amd_ctx *c, int band_rows, hipStream_t st = nullptr) {
    if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
    auto *d = new nblic_amd_dstream;
    d->c = c; d->device = c->device; d->band_rows_req = band_rows; d->st = Stream::lent(st);
    if (!st && d->st.create(hipStreamNonBlocking) != hipSuccess) { dstream_free(d); return nullptr; }
    return d;
}

static nblic_amd_dstream *dstream_resume(nblic_amd_ctx *c, const void *ck, size_t len) {
    if (!c) return nullptr;
    DecodeCheckpoint H;
    if (dstream_check(ck, len, c->max_px, H) != 0) return nullptr;
    nblic_amd_dstream *d = dstream_new(c, H.band_rows);
    if (!d) return nullptr;
    d->it = DecodeItem{0, H.h, H.w, H.near, H.k_step, H.effort, H.kind, 0, -1, -1};
    if (!dstream_setup(d) || d->band_rows != H.band_rows) { dstream_free(d); return nullptr; }
    const RecordLayout L = record_layout(H.kind, H.w, H.effort);
    const uint8_t *body = static_cast<const uint8_t *>(ck) + sizeof H;
    memcpy(&d->H, body, sizeof(SerialState));
    d->sha = H.rows_sha;
    d->row0 = std::max(0, H.next_row - 2);
    bool ok = hipMemcpyAsync(d->d_state, body, L.b, hipMemcpyHostToDevice, d->st) == hipSuccess &&
              (!L.b_bytes || hipMemcpyAsync(d->d_stats, body + L.b, L.b_bytes, hipMemcpyHostToDevice, d->st) == hipSuccess) &&
              rows_above_in(d->d_rows, d->row0, body + L.rows, H.next_row, H.w, d->st);
    if (H.kind) {
        d->qtab.assign(body + L.tab, body + L.tab + kQTab);
        ok = ok && hipMemcpyAsync(d->d_tab, d->qtab.data(), kQTab, hipMemcpyHostToDevice, d->st) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(d->st) == hipSuccess;
    if (!ok) { dstream_free(d); return nullptr; }
    d->pend_off = d->win_off = H.feed_from; d->win_len = 0;
    d->have_head = true;
    return d;
}

// The drop-in decoders (see safe_copy): ONE stream that starts at p, through a band decoder, rows straight into img;
// *ph .. *peffort receive the header fields.  0 / -1.  The caller holds c->api, so the decoder may run on dec_stream
// (a stream of its own costs about 3 ms per call to create and destroy).
static int decode_dropin(nblic_amd_ctx *c, const unsigned char *p, bool qnblic, unsigned char *img, int *ph, int *pw, int *pnear, int *peffort) {
    c->fed_bytes = 0;
    nblic_amd_dstream *d = dstream_new(c, c->serial_rows, c->dec_stream);
    if (!d) return -1;
    const size_t step = std::max(size_t(4096), c->feed_chunk);
    int rc = 2;
    while (rc == 2 && !d->complete) {                                    // the next step only when the decoder asks for it
        const size_t have = d->pend.size();
        d->pend.resize(have + step);
        const size_t got = safe_copy(c, d->pend.data() + have, p + c->fed_bytes, step);
        d->pend.resize(have + got);
        d->complete = got < step;                                        // the caller's memory ends here
        c->fed_bytes += long(got);
        const bool had_head = d->have_head;
        dstream_try_header(d);
        if (d->refused || d->failed) break;
        if (!d->have_head) continue;
        const DecodeItem &it = d->it;
        if (!had_head) {
            if ((it.kind == 1) != qnblic) break;                         // before any launch: cli.cpp tries QNBLICdecompress on every file first
            *ph = it.h; *pw = it.w;
            if (pnear) *pnear = it.near;
            if (peffort) *peffort = it.effort;
        }
        const size_t r0 = size_t(d->H.next_row), w = size_t(it.w);
        rc = dstream_run(d, 0.0, img + r0 * w, (size_t(it.h) - r0) * w, nullptr, nullptr);
    }
    dstream_free(d);
    return rc == 1 ? 0 : -1;
}

// ---- seek index: decoder checkpoints every R rows, kept next to the stream ------------------------------------------
// A band decoder's checkpoint taken in front of row r is an ENTRY POINT: rows [r, h) decode from it alone.  An index is a
// list of them, one in front of every row R, 2R, ... below h, bound to one stream by its length and SHA-256.  The stream
// itself is untouched.  Layout: IndexHead | count x (uint64 length | NBLDCKPT checkpoint with band_rows = R) | SHA-256 of
// all before it.  An entry is the decoder record (kDecodeStateBytes, ~86 KB; QNBLIC 12 KB + the 24 KB tables), B
// (efforts 2 / 3: 512 / 1024 bytes per column) and the two rows above r.
constexpr uint32_t kIndexVersion = 1;
struct IndexHead {
    char magic[8];                     // "NBLSIDX1"
    uint32_t version;                  // kIndexVersion
    int32_t kind, h, w, near, k_step, effort, every_rows, count;
    uint32_t reserved[3];              // zero
    unsigned long long stream_len;
    uint8_t stream_sha[32];
};
static_assert(sizeof(IndexHead) == kIndexHeadBytes, "written and read as bytes");
static_assert(offsetof(IndexHead, version) == kHeadVersionAt && offsetof(IndexHead, kind) == kHeadKindAt && offsetof(IndexHead, h) == kHeadHAt &&
              offsetof(IndexHead, w) == kHeadWAt && offsetof(IndexHead, effort) == kHeadEffortAt && offsetof(IndexHead, every_rows) == kHeadEveryAt &&
              offsetof(IndexHead, count) == kHeadCountAt && kIndexVersion == kUnpackedVersion && kMapSyms == int(kPackMapSyms) &&
              kCodeRank == kUnpackCodeRank, "index_pack.h reads these fields by offset");

static IndexHead index_head(const DecodeItem &it, int every, int count, unsigned long long stream_len) {     // all but stream_sha
    IndexHead H{};
    memcpy(H.magic, "NBLSIDX1", 8);
    H.version = kIndexVersion;
    H.kind = it.kind; H.h = it.h; H.w = it.w; H.near = it.near; H.k_step = it.k_step; H.effort = it.effort;
    H.every_rows = every; H.count = count;
    H.stream_len = stream_len;
    return H;
}

struct IndexView {                     // a checked index: its head and where its entries are
    IndexHead H;
    RecordLayout L;                    // of every entry's body
    std::vector<const uint8_t *> ent;  // entry k + 1 (the checkpoint in front of row (k + 1) R) at ent[k]: its head (verbatim in a packed index too)
    const uint8_t *body(int k) const { return ent[size_t(k - 1)] + sizeof(DecodeCheckpoint); }     // entry k, 1-based; an unpacked index only
    bool packed = false;               // a packed index (index_pack.h): P says where the parts of its entries' bodies lie
    PackedView P;
};

// A checkpoint's running row hash, written canonically: the bytes of the partial block past total % 64 are whatever
// earlier updates left there, and which those are depends on how the rows were cut into updates.
static Sha256 canonical_sha(Sha256 s) {
    const size_t fill = size_t(s.total & 63);
    memset(s.block + fill, 0, sizeof s.block - fill);
    return s;
}

// The head of the index entry in front of row `row` at ck, and behind it the header of its record: S as the coder stands
// there (pos, interval or rANS state, and whatever else of the header the writer holds), rows_sha over rows [0, row).  The
// rest of the body and the seal are the caller's.  Every encoder's index and index_build_batch's go through here.
static void index_entry_head(uint8_t *ck, const DecodeItem &it, int every, int row, SerialState S, const Sha256 &rows_sha) {
    S.next_row = row; S.status = kRunning;
    const DecodeCheckpoint H = decode_head(it, every, row, S.pos & ~511ull, canonical_sha(rows_sha));
    memcpy(ck, &H, sizeof H);
    memcpy(ck + sizeof H, &S, sizeof S);
}

// Every field of an index, every entry (dstream_check), and -- when `stream` is given -- that it is the stream the index
// was made for.  Host only.  0 = valid (V filled in), -1 = refused.
static bool index_head_ok(const IndexHead &H, long max_px) {
    if (!codec_fields_ok(H.kind, H.h, H.w, H.near, H.k_step, H.effort, max_px) || H.reserved[0] != 0 || H.reserved[1] != 0 || H.reserved[2] != 0) return false;
    if (H.every_rows < 1 || H.every_rows >= H.h || H.count != (H.h - 1) / H.every_rows) return false;
    return H.stream_len < kMaxStreamPos;
}
static bool index_entry_head_ok(const IndexHead &H, const DecodeCheckpoint &C, const SerialState &S, int k) {     // entry k, 0-based
    return C.kind == H.kind && C.h == H.h && C.w == H.w && C.near == H.near && C.k_step == H.k_step && C.effort == H.effort &&
           C.band_rows == H.every_rows && C.next_row == (k + 1) * H.every_rows && C.feed_from <= H.stream_len && S.pos <= H.stream_len;
}
static bool index_stream_ok(const IndexHead &H, const void *stream, size_t slen, long max_px) {
    if (slen != H.stream_len) return false;
    DecodeItem it{0, 0, 0, 0, 0, 0, 0, slen, -1, -1};
    if (!parse_stream_header(static_cast<const uint8_t *>(stream), slen, max_px, it)) return false;
    if (it.kind != H.kind || it.h != H.h || it.w != H.w || it.near != H.near || it.k_step != H.k_step || it.effort != H.effort) return false;
    uint8_t d[32];
    sha256_of(stream, slen, d);
    return memcmp(d, H.stream_sha, 32) == 0;
}

// The same for a PACKED index, in its packed form: the structural walk (every length, flag and width byte, every packed
// entry's hash), the head, every entry's head and record header, and the table values a resumed launch depends on -- the
// counters, the re-mappers, a raw B, the QNBLIC tables -- each re-derived from its own part alone, entry after entry.  The
// entries' own seals and the final seal are NOT re-derived here: unpack_index does that.
static int packed_index_check(const void *idx, size_t ilen, const void *stream, size_t slen, long max_px, IndexView &V) {
    const uint8_t *p = static_cast<const uint8_t *>(idx);
    V.ent.clear();
    V.packed = true;
    if (!packed_walk(idx, ilen, V.P)) return -1;
    IndexHead &H = V.H;
    memcpy(&H, p, sizeof H);
    if (!index_head_ok(H, max_px)) return -1;
    V.L = record_layout(H.kind, H.w, H.effort);
    const PackedView &P = V.P;
    if (P.body_bytes != V.L.bytes) return -1;
    std::vector<uint8_t> tab[2][3];                                      // this entry's and the previous one's: counters | rank | syms, or the QNBLIC tables
    const int want[3] = {H.kind ? kQPartTab : kPartCounters, H.kind ? -1 : kPartRank, H.kind ? -1 : kPartSyms};
    for (int k = 0; k < H.count; k++) {
        const PackedEntry &E = P.ent[size_t(k)];
        DecodeCheckpoint C;
        SerialState S;
        memcpy(&C, p + E.head_at, sizeof C);
        memcpy(&S, p + E.part_at[0], sizeof S);                          // (a part that is not coded is always stored raw)
        if (memcmp(C.magic, "NBLDCKPT", 8) != 0 || C.version != kDecodeCheckpointVersion || !checkpoint_fields_ok(C, S, max_px) ||
            !index_entry_head_ok(H, C, S, k)) return -1;
        auto &cur = tab[k & 1], &prev = tab[(k & 1) ^ 1];
        for (int t : {0, 2, 1}) {                                        // the rank bytes last: left out, they come from the syms
            const int j = want[t];
            if (j < 0) continue;
            cur[t].resize(P.parts[j].bytes);
            unpack_part(p, P, k, j, k ? prev[t].data() : nullptr, t == 1 ? cur[2].data() : nullptr, cur[t].data());
        }
        if (H.kind ? !qtab_ok(cur[0].data()) : !nblic_tables_ok(cur[0].data(), cur[1].data(), cur[2].data())) return -1;
        for (int j = 0; j < P.n_parts; j++)
            if (P.parts[j].code == kCodeInt64 && E.part_flag[j] == kPartRaw && !finite_doubles(p + E.part_at[j], P.parts[j].bytes)) return -1;
        V.ent.push_back(p + E.head_at);
    }
    return stream && !index_stream_ok(H, stream, slen, max_px) ? -1 : 0;
}

static int index_check(const void *idx, size_t ilen, const void *stream, size_t slen, long max_px, IndexView &V) {
    if (index_is_packed(idx, ilen)) return packed_index_check(idx, ilen, stream, slen, max_px, V);
    IndexHead &H = V.H;
    V.packed = false;
    if (!sealed_body(idx, ilen, "NBLSIDX1", kIndexVersion, H)) return -1;
    const uint8_t *p = static_cast<const uint8_t *>(idx);
    if (!index_head_ok(H, max_px)) return -1;
    V.L = record_layout(H.kind, H.w, H.effort);
    V.ent.clear();
    size_t at = sizeof H;
    const size_t end = ilen - 32;
    for (int k = 0; k < H.count; k++) {
        unsigned long long n;
        if (end - at < 8) return -1;
        memcpy(&n, p + at, 8);
        at += 8;
        if (n > end - at) return -1;
        DecodeCheckpoint C;
        if (dstream_check(p + at, size_t(n), max_px, C) != 0) return -1;
        SerialState S;
        memcpy(&S, p + at + sizeof C, sizeof S);
        if (!index_entry_head_ok(H, C, S, k)) return -1;
        V.ent.push_back(p + at);
        at += size_t(n);
    }
    if (at != end) return -1;
    return stream && !index_stream_ok(H, stream, slen, max_px) ? -1 : 0;
}

// One band-decoder pass with band_rows = R, a checkpoint in front of every row R, 2R, ...; the pass runs to the end of the
// image, so a stream that does not decode gets no index.  With out == NULL or cap too small only the size (the stream is
// only described; ctx may then be NULL).  -1: a stream this library does not decode, R < 1 or R >= h.
static long index_build(nblic_amd_ctx *c, const unsigned char *stream, size_t slen, int every, unsigned char *out, size_t cap) {
    if (!stream) return -1;
    DecodeItem it{0, 0, 0, 0, 0, 0, 0, 0, -1, -1};
    std::vector<uint8_t> qtab;
    if (describe_stream(stream, slen, false, c ? c->max_px : kMaxPixels, it, qtab) != Described::ok) return -1;
    if (every < 1 || every >= it.h) return -1;
    const int count = (it.h - 1) / every;
    const size_t eb = index_entry_bytes(it.kind, it.w, it.effort);
    const size_t need = index_total_bytes(count, eb);
    if (eb != sizeof(DecodeCheckpoint) + record_layout(it.kind, it.w, it.effort).bytes + 32) return -1;     // (the two descriptions of an entry agree)
    if (!out || cap < need) return long(need);
    if (!c) return -1;
    IndexHead H = index_head(it, every, count, slen);
    sha256_of(stream, slen, H.stream_sha);
    memcpy(out, &H, sizeof H);
    // the pass runs in bands of at most serial_rows_per_launch rows (a launch lasts seconds at most); the entries say R
    const int band = std::min(every, rows_per_launch(it, c->serial_rows));
    nblic_amd_dstream *d = dstream_new(c, band);
    if (!d) return -1;
    d->pend.assign(stream, stream + slen);
    d->complete = true;
    std::vector<uint8_t> rows(size_t(band) * size_t(it.w));
    size_t at = sizeof H;
    bool ok = true;
    for (int k = 1; ok && k <= count + 1; k++) {
        const int limit = k <= count ? k * every : it.h;
        d->stop_row = limit;
        int rc;
        do rc = dstream_run(d, 0.0, rows.data(), rows.size(), nullptr, nullptr);
        while (rc == 0 && d->H.next_row < limit);
        if (k > count) { ok = rc == 1; break; }
        ok = rc == 0 && d->H.next_row == limit;
        if (!ok) break;
        const unsigned long long n = eb;
        memcpy(out + at, &n, 8);
        // R as the band height, the row hash canonical (the band encoder's index is byte-identical)
        ok = dstream_checkpoint(d, out + at + 8, eb, every, canonical_sha(d->sha)) == eb;
        at += 8 + eb;
    }
    if (!ok) fprintf(stderr, "[nblic_amd] index: the stream does not decode\n");
    dstream_free(d);
    if (!ok) return -1;
    seal(out, need);
    return long(need);
}

// ---- the band ENCODER's index: the decoder's entry record, converted from the encoder's state at an entry row -------
// The encoder carries the same adaptive state as the decoder in other layouts (kernels_e1.hip): the model record holds
// the 2048 context biases and `bias`; cnt_state the 4096 counters as {c0, c1} pairs keyed parity | tree / 2 | node
// (touch_of); map_state per re-mapper 60 ints: symbol -> rank, rank -> symbol, hit counts by rank (k_init_state,
// k_mapper_chains).  The coder: the decoder's interval is the encoder's, and it has read the four bytes that follow
// the ones emitted (NBLIC.c:527-586): pos = emitted + 4, window = those four bytes -- not written yet when the row is
// reached, so the entry waits for them (the final flush always provides them).

// The stream bytes emitted by this call so far, [out, end): what the pending entries are waiting for.
static void stream_index_bytes(nblic_amd_stream *s, const uint8_t *out, const uint8_t *end) {
    s->pending.bytes(s->bytes_total, out, end);
}
constexpr size_t kEntryWindowAt = sizeof(DecodeCheckpoint) + offsetof(SerialState, window);     // where an entry's window goes

// After the band [i0, i0 + rows) has been coded: the bytes it emitted go to the pending entries, its rows into the row
// hash, and behind a band that ends on an entry row (`entry`: index_band_cut) the entry is written down (all but its window).
static bool stream_index_band(nblic_amd_stream *s, int i0, int rows, bool entry, const uint8_t *out, const uint8_t *end, uint32_t lo, uint32_t hi) {
    stream_index_bytes(s, out, end);
    const size_t w = size_t(s->w), at = size_t(i0) * w;
    const uint8_t *plane = s->near > 0 ? s->d_recon : s->d_img;       // lossless: the reconstruction is the input
    Group &g = s->c->groups[size_t(s->gid)];
    Slot &sl = g.slots[0];
    s->band_rows_host.resize(size_t(rows) * w);
    if (hipMemcpyAsync(s->band_rows_host.data(), plane + at, size_t(rows) * w, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) return false;
    s->rows_sha.update(s->band_rows_host.data(), s->band_rows_host.size());
    const int r = i0 + rows, R = s->index_every;
    if (!entry) return true;
    const DecodeItem it{0, s->h, s->w, s->near, s->k_step, s->effort, 0, 0, -1, -1};
    const RecordLayout L = record_layout(0, s->w, s->effort);
    std::vector<uint8_t> ck(sizeof(DecodeCheckpoint) + L.bytes + 32, 0);
    std::vector<uint8_t> model(kModelStateBytes);
    std::vector<int32_t> map(512 * 60), cnt(4096 * 2);
    uint8_t *rec = ck.data() + sizeof(DecodeCheckpoint);
    bool ok = hipMemcpyAsync(model.data(), sl.d_state, kModelStateBytes, hipMemcpyDeviceToHost, g.stream) == hipSuccess &&
              hipMemcpyAsync(map.data(), sl.b.map_state, kMapStateBytes, hipMemcpyDeviceToHost, g.stream) == hipSuccess &&
              hipMemcpyAsync(cnt.data(), sl.b.cnt_state, kCntStateBytes, hipMemcpyDeviceToHost, g.stream) == hipSuccess &&
              rows_above_out(rec + L.rows, plane, 0, r, s->w, g.stream);
    if (L.b_bytes) ok = ok && hipMemcpyAsync(rec + L.b, s->d_stats, L.b_bytes, hipMemcpyDeviceToHost, g.stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(g.stream) != hipSuccess) return false;
    SerialState M;
    memcpy(&M, model.data(), sizeof M);
    SerialState S{};
    const unsigned long long emitted = s->bytes_total + (unsigned long long)(end - out);
    S.pos = emitted + 4; S.lo = lo; S.hi = hi; S.bias = M.bias;
    index_entry_head(ck.data(), it, R, r, S, s->rows_sha);
    uint8_t *tab = rec + sizeof S;
    memcpy(tab, model.data() + sizeof M, size_t(kContexts) * 4);                       // context biases
    uint32_t *dcnt = reinterpret_cast<uint32_t *>(tab) + kContexts;                   // counters, tree-major
    for (int key = 0; key < 4096; key++) {
        const int tree = ((key >> 8) & 7) * 2 + (key >> 11), node = key & 255;
        const uint32_t c = uint32_t(cnt[size_t(key) * 2]) | (uint32_t(cnt[size_t(key) * 2 + 1]) << 16);
        memcpy(dcnt + tree * kTreeNodes + node, &c, 4);
    }
    int32_t *hits = reinterpret_cast<int32_t *>(tab) + kRecCount;
    uint8_t *rank = tab + size_t(kRecRank) * 4, *sym = tab + size_t(kRecSym) * 4;
    for (int m = 0; m < 512; m++)
        for (int k = 0; k < kMapSyms; k++) {
            rank[m * kMapSyms + k] = uint8_t(map[size_t(m) * 60 + k]);
            sym[m * kMapSyms + k] = uint8_t(map[size_t(m) * 60 + 20 + k]);
            memcpy(hits + m * kMapSyms + k, &map[size_t(m) * 60 + 40 + k], 4);
        }
    s->entries.push_back(std::move(ck));                               // (moving the vector leaves its bytes where they are)
    s->pending.add(s->entries.back().data(), s->entries.back().size(), kEntryWindowAt, emitted);
    return true;
}

// Which front the object's bands run on; before its first _run.  The staged one is -n0 -e1 alone.
static int stream_set_front(nblic_amd_stream *s, int front) {
    if (!s || s->ran || s->failed || front < 0 || front > 1) return -1;
    if (front == 1 && (s->near != 0 || s->effort != 1)) return -1;
    s->front = front;
    return 0;
}

static int stream_set_index(nblic_amd_stream *s, int every) {
    if (!s || s->bytes_total != 0 || s->first_row != 0 || every < 1 || every >= s->h) return -1;
    s->index_every = every;
    return 0;
}

// The index of a finished image whose every band this object coded; 0 otherwise.  Same layout as index_build.
static size_t stream_index(nblic_amd_stream *s, void *buf, size_t cap) {
    if (!s || s->index_every <= 0 || s->first_row != 0 || !s->finished || !s->pending.waiting.empty()) return 0;
    const int count = (s->h - 1) / s->index_every;
    if (int(s->entries.size()) != count) return 0;
    const size_t eb = index_entry_bytes(0, s->w, s->effort), need = index_total_bytes(count, eb);
    for (const auto &e : s->entries) if (e.size() != eb) return 0;
    if (!buf || cap < need) return need;
    IndexHead H = index_head(DecodeItem{0, s->h, s->w, s->near, s->k_step, s->effort, 0, 0, -1, -1}, s->index_every, count, s->bytes_total);
    s->sha.digest(H.stream_sha);
    uint8_t *p = static_cast<uint8_t *>(buf);
    for (int k = 0; k < count; k++) memcpy(p + index_entry_at(k, eb), s->entries[size_t(k)].data(), eb);
    index_close(p, &H, count, eb);
    return need;
}

// ---- the INDEXED BATCH: many -n0 -e1 images and their seek indexes, a group of images stepped through row bands together ----
// What the band encoder does for one image per object (staged front, an entry record at every entry row), done for a
// whole group per launch sequence: every live slot of a group holds one image in progress, a STEP carries one band of each
// -- the jobs differ in row0, in height and in width -- and a slot whose image has ended takes the batch's next image at
// the next step.  Nothing in a band's front or back half depends on the range coder, so the bins and entry records of step t
// are coded by worker threads, one task per image and band, while the GPU runs step t + 1; a step's bins, records and (for
// device inputs) rows land in one of two sets of page-locked buffers.  The model tables are the slot's three tables and stay
// on the device from band to band; an entry's decoder record is made there (k_index_records).
struct IdxPool {                                                         // worker threads of one call
    std::mutex m; std::condition_variable cv; std::deque<std::function<void()>> q; bool stop = false;
    std::vector<std::thread> th;
    void start(int n) {
        for (int i = 0; i < n; i++)
            th.emplace_back([this] {
                for (;;) {
                    std::function<void()> f;
                    {
                        std::unique_lock<std::mutex> l(m);
                        cv.wait(l, [this] { return stop || !q.empty(); });
                        if (q.empty()) return;
                        f = std::move(q.front()); q.pop_front();
                    }
                    f();
                }
            });
    }
    void post(std::function<void()> f) { { std::lock_guard<std::mutex> l(m); q.push_back(std::move(f)); } cv.notify_one(); }
    ~IdxPool() { { std::lock_guard<std::mutex> l(m); stop = true; } cv.notify_all(); for (auto &t : th) t.join(); }
};
struct IdxPendingTasks {                                                 // the tasks of one group's step that have not ended
    std::mutex m; std::condition_variable cv; int left = 0;
    void add(int n) { std::lock_guard<std::mutex> l(m); left += n; }
    void done() { { std::lock_guard<std::mutex> l(m); left--; } cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> l(m); cv.wait(l, [this] { return left == 0; }); }
};

// The FRAME of a call, for this codec and for effort 0 below (indexed_batch): the arguments are checked and every image that
// can be refused is refused before anything is launched, the admitted ones are handed out one by one to the drivers -- one
// thread per group the call uses, each holding its group for the whole call (idx_run_driver) -- and the results are closed
// once the drivers have ended.  What a codec adds is its IdxCodec: five facts and the step loop of its driver.
struct IdxCall;
struct IdxSplit { double ms[5] = {0}; long steps = 0; };                 // nblic_amd_indexed_batch_split's figures, of one driver or summed
struct IdxCodec {
    int kind, effort;
    size_t min_out, max_out;                                             // in elements of `outs` (bytes; effort 0: 16-bit words): below min_out the image is refused, the capacity is clamped to max_out
    void (*driver)(IdxCall &, Group &, IdxSplit &);                      // steps the group's slots through the batch's images
};
// The NBLIC coder of an image between its first band and its last (-e1 alone): interval, bytes emitted, the running SHA-256 of
// the stream and of the rows, the entries that wait for their window.  Touched by one task at a time.
struct IdxCoder {
    RangeScalar rc;
    unsigned long long emitted = 0;                                      // stream bytes so far, header included
    Sha256 stream_sha, rows_sha;
    PendingEntries pending;
    int made = 0;
    std::atomic<bool> failed{false};                                     // out of room: the driver drops the image at its next step
};
struct IdxImage {                                                        // one admitted image and the index being written into the caller's buffer
    int k = 0, h = 0, w = 0, every = 0, count = 0;                       // every: 0 = no index wanted (or none possible); count: its entries
    const uint8_t *host_plane = nullptr;                                 // host input: the rows are hashed from it
    bool on_device = false, collect = false;                             // its rows are on the device alone; a source that k_collect writes into the slot's d_img, band by band
    void *out = nullptr; size_t cap = 0;                                 // in the codec's elements
    uint8_t *index = nullptr; size_t entry_bytes = 0;
    IdxCoder nb;
};
struct IdxCall {
    const IdxCodec &codec; nblic_amd_ctx *c; int n; const unsigned char *const *imgs; bool on_device; int band_rows; long *lens, *ilens;
    const CollectFrom *from;                                             // the _from calls: imgs / on_device are its own; null otherwise
    std::vector<std::unique_ptr<IdxImage>> images;                       // by position in the batch; empty: refused before the call started
    std::atomic<int> next{0};
    std::atomic<bool> failed{false};                                     // a device-side failure: the call is over
    IdxPool pool;
    std::mutex m; IdxSplit split;                                        // summed over the groups (guarded by m)
    void fail(const IdxImage &I) { lens[I.k] = -1; if (I.every) ilens[I.k] = -1; }
    IdxImage *next_image() {                                             // the batch's next admitted image; nullptr: all are taken
        for (;;) {
            const int j = next.fetch_add(1);
            if (j >= n) return nullptr;
            if (images[size_t(j)]) return images[size_t(j)].get();
        }
    }
};
struct IdxLive { IdxImage *im = nullptr; int row0 = 0, band = 0; const uint8_t *plane = nullptr; };     // the image a slot works on, rows [0, row0) queued

// Image I's plane where slot s's kernels read it: a device input as it is, a host input copied into the slot on st, a
// source in the slot's d_img, where every step collects the rows of its band (idx_collect_band).
// nullptr: the copy could not be queued.
static const uint8_t *idx_plane(const IdxCall &q, const IdxImage &I, Slot &s, hipStream_t st) {
    const size_t n = size_t(I.h) * size_t(I.w);
    if (I.collect) return s.d_img.reserve(n) == hipSuccess ? s.d_img.get() : nullptr;
    if (I.on_device) { if (q.from) q.c->collect_counts[0]++; return q.imgs[I.k]; }
    if (s.d_img.reserve(n) != hipSuccess || hipMemcpyAsync(s.d_img, q.imgs[I.k], n, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
    return s.d_img;
}

// jobs[j]: the front job of the next band of live slot L (workspace s), cut by the band rule.  true: an entry stands behind
// the band, and the task that makes its decoder record at byte rec_at of the step's records has been appended.
static bool idx_band_job(nblic_amd_ctx *c, const IdxLive &L, const Slot &s, E1Job *jobs, int j, IndexRecordTask *tasks, int &n_tasks, size_t rec_at) {
    const BandCut cut = index_band_cut(L.row0, L.band, L.im->h, L.im->every);
    jobs[j] = band_job_front(c, s.b, L.plane, L.row0, cut.rows, L.im->w, 0);
    if (cut.entry) tasks[n_tasks++] = IndexRecordTask{j, 0, (unsigned long long)(rec_at)};
    return cut.entry;
}

// The rows of job J's band, of a source, into their place in the slot's plane: a task of the step's ONE k_collect launch.
static bool idx_collect_band(const IdxCall &q, Group &g, const IdxLive &L, const E1Job &J, size_t at) {
    if (!L.im->collect) return true;
    const uint32_t w = uint32_t(L.im->w), px0 = uint32_t(L.row0) * w;
    return collect_add(g, *q.from, L.im->k, const_cast<uint8_t *>(L.plane), px0, px0 + uint32_t(J.h) * w, at);
}

// One driver thread: takes a group, runs the codec's driver on it, adds its figures to the call's.
static void idx_run_driver(IdxCall &q) {
    nblic_amd_ctx *c = q.c;
    if (hipSetDevice(c->device) != hipSuccess) { q.failed = true; return; }
    const int gid = take_group(c);
    IdxSplit sp;
    q.codec.driver(q, c->groups[size_t(gid)], sp);                       // (everything the driver owns goes before the group is released)
    {
        std::lock_guard<std::mutex> l(q.m);
        for (int k = 0; k < 5; k++) q.split.ms[k] += sp.ms[k];
        q.split.steps += sp.steps;
    }
    release_group(c, gid);
}

struct IdxBand {                                                         // what a task codes: one band of one image
    IdxImage *im; int i0, rows; const uint16_t *bins; uint32_t n_ev; const uint8_t *rows_host, *rec; bool last;
};

// The band [i0, i0 + rows) of an image has been coded on the device: range-code its bins, hash its rows, hand the new stream
// bytes to the waiting entries, write down the entry in front of row i0 + rows if there is one, and end the image with its
// last band.
static void idx_code_band(IdxCall &q, const IdxBand &b) {
    IdxImage &I = *b.im;
    IdxCoder &C = I.nb;
    if (C.failed) return;
    auto fail = [&] { C.failed = true; q.fail(I); };
    uint8_t *const out = static_cast<uint8_t *>(I.out);
    const DecodeItem it{0, I.h, I.w, 0, k_step_for_near(0), 1, 0, 0, -1, -1};
    if (b.i0 == 0) {
        write_header(out, I.h, I.w, 0, k_step_for_near(0), 1);
        C.rc.begin(out + kHeaderBytes, I.cap - kHeaderBytes);
        C.stream_sha.update(out, kHeaderBytes);
        C.emitted = kHeaderBytes;
    }
    const uint8_t *const from = C.rc.p;
    C.rc.feed(b.bins, b.n_ev);
    if (C.rc.overflow || (b.last && C.rc.finish() == SIZE_MAX)) return fail();
    C.pending.bytes(C.emitted, from, C.rc.p);
    C.stream_sha.update(from, size_t(C.rc.p - from));
    C.emitted += (unsigned long long)(C.rc.p - from);
    if (I.every) C.rows_sha.update(b.rows_host, size_t(b.rows) * size_t(I.w));
    if (b.rec) {                                                         // an entry row: everything but the window, which waits
        uint8_t *ck = I.index + index_entry_at(C.made, I.entry_bytes), *rec = ck + sizeof(DecodeCheckpoint);
        memcpy(rec, b.rec, kDecodeStateBytes + 2 * size_t(I.w));
        SerialState S;
        memcpy(&S, rec, sizeof S);                                       // zero but for `bias` (k_index_records)
        S.pos = C.emitted + 4; S.lo = C.rc.lo; S.hi = C.rc.hi;
        index_entry_head(ck, it, I.every, b.i0 + b.rows, S, C.rows_sha);
        C.pending.add(ck, I.entry_bytes, kEntryWindowAt, C.emitted);
        C.made++;
    }
    if (!b.last) return;
    q.lens[I.k] = long(C.emitted);
    if (!I.every) return;
    if (C.made != I.count || !C.pending.waiting.empty()) { q.ilens[I.k] = -1; return; }     // (cannot happen: the flush provides every window)
    IndexHead H = index_head(it, I.every, I.count, C.emitted);
    C.stream_sha.digest(H.stream_sha);
    index_close(I.index, &H, I.count, I.entry_bytes);
    q.ilens[I.k] = long(index_total_bytes(I.count, I.entry_bytes));
}

// The step loop of -e1: a step waits for its totals in the middle, and for the tasks of the step before at its end.
static void idx_driver(IdxCall &q, Group &g, IdxSplit &sp) {
    nblic_amd_ctx *c = q.c;
    const hipStream_t st = g.stream;
    const int n_slots = int(g.slots.size());
    std::vector<IdxLive> live{size_t(n_slots)};
    struct Set { Locked bins, recs, rows; } sets[2];                     // what a step's tasks read (Locked counts 16-bit words)
    DevBuf<uint16_t> d_bins; DevBuf<uint8_t> d_recs;
    Pinned<IndexRecordTask> h_tasks; DevBuf<IndexRecordTask> d_tasks;
    IdxPendingTasks tasks_left;
    std::vector<int> slot_of(size_t(n_slots), 0);
    std::vector<size_t> bins_at(size_t(n_slots), 0), rec_at(size_t(n_slots), 0), rows_at(size_t(n_slots), 0);
    bool ok = h_tasks.alloc(size_t(n_slots)) == hipSuccess && d_tasks.alloc(size_t(n_slots)) == hipSuccess && (!q.from || collect_room(g, size_t(n_slots)));
    auto grow = [](Locked &b, size_t bytes) { return bytes <= b.capacity() * 2 || b.alloc((bytes + bytes / 4 + 4096) / 2); };
    for (long t = 0; ok && !q.failed; t++) {
        // ---- which image each slot works on
        for (int k = 0; k < n_slots; k++) {
            IdxLive &L = live[size_t(k)];
            if (L.im && (L.row0 >= L.im->h || L.im->nb.failed)) L.im = nullptr;
            IdxImage *I = L.im ? nullptr : q.next_image();
            if (!I) continue;
            Slot &s = g.slots[size_t(k)];
            L.band = encoder_band_rows(q.band_rows, I->h, I->w, 1);
            if (!(ok = ensure_pixels(s, size_t(L.band) * size_t(I->w)) && (L.plane = idx_plane(q, *I, s, st)) != nullptr)) break;
            L.im = I; L.row0 = 0;
        }
        if (!ok) break;
        // ---- 1. job records of the live slots, and the tasks of the bands that end on an entry row
        int n_jobs = 0, n_tasks = 0; size_t rec_bytes = 0;
        collect_begin(g);
        for (int k = 0; k < n_slots && ok; k++) {
            const IdxLive &L = live[size_t(k)];
            if (!L.im) continue;
            const bool entry = idx_band_job(c, L, g.slots[size_t(k)], g.h_jobs, n_jobs, h_tasks, n_tasks, rec_bytes);
            ok = idx_collect_band(q, g, L, g.h_jobs[n_jobs], 0);
            rec_at[size_t(n_jobs)] = entry ? rec_bytes : SIZE_MAX;
            if (entry) rec_bytes += up256(kDecodeStateBytes + 2 * size_t(L.im->w));
            slot_of[size_t(n_jobs++)] = k;
        }
        if (n_jobs == 0 || !ok) break;
        hipEvent_t *ev = g.tm.ev;                                        // marks of the step's five parts
        ok = hipMemcpyAsync(g.d_jobs, g.h_jobs, size_t(n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, st) == hipSuccess;
        if (!ok) break;
        hipEventRecord(ev[0], st);
        if (!(ok = collect_flush(g, st))) break;                         // the bands of the sources: one launch
        // ---- 2. / 3. fresh tables for the jobs that start an image, then the front half of every band
        for (int j = 0; j < n_jobs; j++) if (g.h_jobs[j].row0 == 0) e1_launch_init(g.d_jobs + j, 1, st);
        e1_launch_front_band(g.d_jobs, g.h_jobs, n_jobs, st);
        hipEventRecord(ev[1], st);
        // ---- 4. totals
        ok = hipMemcpyAsync(g.h_totals, g.d_totals, size_t(n_slots) * kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
        hipEventRecord(ev[2], st);
        if (!ok || hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { ok = false; break; }
        // ---- 5. the back half: bins of all jobs side by side in one buffer
        size_t n_bins = 0, rows_bytes = 0;
        for (int j = 0; j < n_jobs && ok; j++) {
            const int k = slot_of[size_t(j)];
            const uint32_t n_ev = g.h_totals[size_t(k) * kTotalsSlot + 2];
            count_long_chains(c, g.h_totals + size_t(k) * kTotalsSlot);
            ok = n_ev < 0x7FFFFFFFu && ensure_events(g.slots[size_t(k)], n_ev);
            bins_at[size_t(j)] = n_bins;
            n_bins += (size_t(n_ev) + 64 + 63) & ~size_t(63);
            rows_at[size_t(j)] = rows_bytes;
            if (live[size_t(k)].im->on_device && live[size_t(k)].im->every) rows_bytes += size_t(g.h_jobs[j].n);
        }
        if (!ok) break;
        Set &S = sets[t & 1];                                            // free: the tasks of step t - 2 ended before step t - 1 was handed over
        ok = (n_bins <= d_bins.capacity() || d_bins.alloc(n_bins + n_bins / 4 + 4096) == hipSuccess) &&
             (rec_bytes <= d_recs.capacity() || d_recs.alloc(rec_bytes) == hipSuccess) &&
             grow(S.bins, n_bins * 2) && grow(S.recs, rec_bytes) && grow(S.rows, rows_bytes);
        if (!ok) break;
        for (int j = 0; j < n_jobs; j++) {
            E1Buffers b = g.slots[size_t(slot_of[size_t(j)])].b;
            b.img = g.h_jobs[j].b.img; b.coded = d_bins + bins_at[size_t(j)];
            e1_job_back(g.h_jobs[j], b, g.h_totals[size_t(slot_of[size_t(j)]) * kTotalsSlot + 2]);
        }
        ok = hipMemcpyAsync(g.d_jobs, g.h_jobs, size_t(n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, st) == hipSuccess &&
             (!n_tasks || hipMemcpyAsync(d_tasks, h_tasks, size_t(n_tasks) * sizeof(IndexRecordTask), hipMemcpyHostToDevice, st) == hipSuccess);
        if (!ok) break;
        hipEventRecord(ev[3], st);
        e1_launch_back(g.d_jobs, g.h_jobs, n_jobs, st, nullptr, true);
        // ---- 6. the decoder records of the jobs whose band ends on an entry row
        e1_launch_index_records(g.d_jobs, d_tasks, n_tasks, d_recs, st);
        hipEventRecord(ev[4], st);
        // ---- 7. one copy of the step's bins, one of its records (and the rows of device inputs, for the row hash)
        ok = hipMemcpyAsync(static_cast<uint16_t *>(S.bins), d_bins, n_bins * sizeof(uint16_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
             (!rec_bytes || hipMemcpyAsync(static_cast<uint16_t *>(S.recs), d_recs, rec_bytes, hipMemcpyDeviceToHost, st) == hipSuccess);
        uint8_t *const rows_host = reinterpret_cast<uint8_t *>(static_cast<uint16_t *>(S.rows));
        for (int j = 0; j < n_jobs && ok; j++)
            if (live[size_t(slot_of[size_t(j)])].im->on_device && live[size_t(slot_of[size_t(j)])].im->every)
                ok = hipMemcpyAsync(rows_host + rows_at[size_t(j)], g.h_jobs[j].b.img, size_t(g.h_jobs[j].n), hipMemcpyDeviceToHost, st) == hipSuccess;
        hipEventRecord(ev[5], st);
        if (!ok || hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { ok = false; break; }
        for (int k = 0; k < 4; k++) {
            float ms = 0.f;
            const int a = k < 2 ? k : k + 1;                             // (2 -> 3 is the host's sizing of the back half)
            if (hipEventElapsedTime(&ms, ev[a], ev[a + 1]) == hipSuccess) sp.ms[k] += ms;
        }
        const auto w0 = std::chrono::steady_clock::now();
        tasks_left.wait();                                               // step t - 1 is coded: an image's bands are coded in order
        sp.ms[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        sp.steps++;
        tasks_left.add(n_jobs);
        const uint8_t *const recs_host = reinterpret_cast<const uint8_t *>(static_cast<uint16_t *>(S.recs));
        for (int j = 0; j < n_jobs; j++) {
            IdxLive &L = live[size_t(slot_of[size_t(j)])];
            IdxImage *I = L.im;
            const int rows = g.h_jobs[j].h;
            const uint8_t *rows_src = !I->every ? nullptr : I->on_device ? rows_host + rows_at[size_t(j)] : I->host_plane + size_t(L.row0) * size_t(I->w);
            const IdxBand b{I, L.row0, rows, static_cast<uint16_t *>(S.bins) + bins_at[size_t(j)], g.h_jobs[j].n_ev, rows_src,
                            rec_at[size_t(j)] == SIZE_MAX ? nullptr : recs_host + rec_at[size_t(j)], L.row0 + rows >= I->h};
            q.pool.post([&q, &tasks_left, b] { idx_code_band(q, b); tasks_left.done(); });
            L.row0 += rows;
        }
    }
    if (!ok) { q.failed = true; fprintf(stderr, "[nblic_amd] indexed batch: a device step failed\n"); }
    hipStreamSynchronize(st);
    tasks_left.wait();
}

// ---- the INDEXED effort-0 BATCH: QNBLIC streams and their seek indexes, a group of images stepped through row bands -------
// The indexed batch above for effort 0.  QNBLIC's model stage is parallel already (q_launch_model), it is lossless, and its
// decoder record is 64 bytes and 3072 contexts, so a step is one launch sequence -- q_launch_model_band, then the records
// of the jobs whose band ends on an entry row -- and three kinds of copies: the band's level | symbol words into the
// IMAGE's page-locked buffer, its entry record, and at the image's last band the histograms (and, for a device input, the
// rows the index hashes).  Nothing on the host sizes anything in between, so a driver does not wait for a step: it queues
// up to kQIdxDepth steps ahead (the ring of job records the queued copies still read, and four timing marks a step) and
// otherwise stops only for a free image buffer.  An image's entropy stage cannot start before its last word is on the
// host -- the histograms are final only then -- so every image in flight holds 2 bytes per pixel of page-locked memory
// (plus its records: 12,352 + 2 w bytes an entry, and 1 byte per pixel more for a device input whose index is wanted); a
// group has 2 x its slots of them, one per slot that is being stepped and as many again for the images the workers are
// coding.  The stage runs on a worker thread: q_entropy_encode_entries, then the entries -- the rANS pass runs last pixel
// first, so what it holds once pixel r w is coded is what the decoder holds in front of row r (q_entropy.cpp).
constexpr int kQIdxDepth = 8;
static_assert(kQIdxDepth * 4 <= kE1Marks, "a queued step's four marks are timing events of the group");

// An image's page-locked buffer, in bytes: words | histograms | entry records | rows [0, count * every) of a device input.
struct QIdxLayout { size_t hist, recs, rec_stride, rows, bytes; };
static QIdxLayout qidx_layout(const IdxImage &I, bool on_device) {
    QIdxLayout L;
    L.hist = up256(2 * size_t(I.h) * size_t(I.w));
    L.recs = L.hist + 12 * 256 * sizeof(uint32_t);
    L.rec_stride = up256(kQDecodeStateBytes + 2 * size_t(I.w));
    L.rows = L.recs + size_t(I.count) * L.rec_stride;
    L.bytes = L.rows + (on_device ? size_t(I.count) * size_t(I.every) * size_t(I.w) : 0);
    return L;
}
struct QIdxFree {                                                        // a driver's image buffers: taken when an image starts, given back by its worker.  Shared (shared_ptr) by the driver and the tasks it posts: whoever lets go last destroys it
    std::mutex m; std::condition_variable cv; std::vector<int> free; int out = 0;
    int take() { std::unique_lock<std::mutex> l(m); cv.wait(l, [this] { return !free.empty(); }); const int b = free.back(); free.pop_back(); out++; return b; }
    void give(int b) { { std::lock_guard<std::mutex> l(m); free.push_back(b); out--; } cv.notify_all(); }
    void wait_all() { std::unique_lock<std::mutex> l(m); cv.wait(l, [this] { return out == 0; }); }
};

// An image's last band has been queued; `ready` is recorded behind its copies.  The entropy stage, then the index.
static void qidx_finish(IdxCall &q, const IdxImage &I, const uint8_t *base, const QIdxLayout &L, hipEvent_t ready) {
    if (hipSetDevice(q.c->device) != hipSuccess || hipEventSynchronize(ready) != hipSuccess) { q.failed = true; return q.fail(I); }
    uint16_t *const out = static_cast<uint16_t *>(I.out);
    std::vector<int> rows(size_t(I.count));
    std::vector<QEntryState> at(size_t(I.count));
    for (int e = 0; e < I.count; e++) rows[size_t(e)] = (e + 1) * I.every;
    const long words = q_entropy_encode_entries(out, I.cap, I.h, I.w, reinterpret_cast<const uint16_t *>(base),
                                                reinterpret_cast<const uint32_t *>(base + L.hist), rows.data(), I.count, at.data());
    if (words < 0) {
        fprintf(stderr, "[nblic_amd] image %d: output buffer of %zu words is too small\n", I.k, I.cap);
        return q.fail(I);
    }
    q.lens[I.k] = words;
    if (!I.every) return;
    const size_t stream_bytes = size_t(words) * 2;
    std::vector<uint8_t> tab(kQTab);
    const long q_pos = q_parse_tables(reinterpret_cast<const unsigned char *>(out), stream_bytes, tab.data());
    if (q_pos < 0) { q.ilens[I.k] = -1; return; }                        // (cannot happen: the tables were written a moment ago)
    const unsigned long long emitted = (unsigned long long)(words - q_pos - 2);       // renormalisation words of the whole pass
    const DecodeItem it{0, I.h, I.w, 0, kMinKStep, 0, 1, stream_bytes, q_pos, -1};
    const RecordLayout R = record_layout(1, I.w, 0);
    const uint8_t *plane = I.host_plane ? I.host_plane : base + L.rows;
    Sha256 rows_sha;
    for (int e = 0; e < I.count; e++) {
        rows_sha.update(plane + size_t(e) * size_t(I.every) * size_t(I.w), size_t(I.every) * size_t(I.w));
        uint8_t *ck = I.index + index_entry_at(e, I.entry_bytes), *rec = ck + sizeof(DecodeCheckpoint);
        memcpy(rec, base + L.recs + size_t(e) * L.rec_stride, kQDecodeStateBytes + 2 * size_t(I.w));
        SerialState S{};                                                 // every other field as the band decoder's checkpoint leaves it: zero
        S.lo = at[size_t(e)].state;
        S.pos = first_pos(it) + 4 + 2 * (emitted - at[size_t(e)].words);  // the two words of the initial state, then one per renormalisation of the pixels above
        index_entry_head(ck, it, I.every, rows[size_t(e)], S, rows_sha);
        memcpy(rec + R.tab, tab.data(), kQTab);
        seal(ck, I.entry_bytes);
    }
    IndexHead H = index_head(it, I.every, I.count, stream_bytes);
    sha256_of(out, stream_bytes, H.stream_sha);
    index_close(I.index, &H, I.count, I.entry_bytes);
    q.ilens[I.k] = long(index_total_bytes(I.count, I.entry_bytes));
}

// The step loop of effort 0: queues kQIdxDepth steps ahead and stops only for a free image buffer.
static void qidx_driver(IdxCall &q, Group &g, IdxSplit &sp) {
    nblic_amd_ctx *c = q.c;
    const hipStream_t st = g.stream;
    const int n_slots = int(g.slots.size()), n_bufs = 2 * n_slots;
    struct Live : IdxLive { int buf = -1; QIdxLayout lay{}; };
    std::vector<Live> live{size_t(n_slots)};
    const auto bufs = std::make_shared<QIdxFree>();
    std::vector<int> slot_of(size_t(n_slots), 0), ring_jobs(size_t(kQIdxDepth), 0), ring_slot(size_t(kQIdxDepth) * size_t(n_slots), 0);
    std::vector<size_t> rec_at(size_t(n_slots), 0);
    const size_t rec_room = up256(kQDecodeStateBytes + 2 * size_t(NBLIC_MAX_WIDTH));
    bool ok = true;
    if (g.qidx_bufs.empty()) {                                           // the group's first call of this kind
        g.qidx_bufs.resize(size_t(n_bufs));
        g.qidx_ready.resize(size_t(n_bufs));
        for (auto &e : g.qidx_ready) ok = ok && e.create(hipEventDisableTiming | hipEventBlockingSync) == hipSuccess;
        ok = ok && g.qidx_jobs.alloc(size_t(kQIdxDepth) * size_t(n_slots)) == hipSuccess && g.qidx_tasks.alloc(size_t(kQIdxDepth) * size_t(n_slots)) == hipSuccess &&
             g.qidx_totals.alloc(size_t(kQIdxDepth) * size_t(n_slots) * kTotalsSlot) == hipSuccess && g.qidx_d_tasks.alloc(size_t(n_slots)) == hipSuccess &&
             g.qidx_d_recs.alloc(size_t(n_slots) * rec_room) == hipSuccess;
        if (!ok) { g.qidx_bufs.clear(); g.qidx_ready.clear(); }
    }
    ok = ok && (!q.from || collect_room(g, size_t(kQIdxDepth) * size_t(n_slots)));
    for (int b = 0; ok && b < n_bufs; b++) bufs->free.push_back(b);
    hipEvent_t *ev = g.tm.ev;                                            // four marks a queued step
    // Step t - kQIdxDepth has left the GPU: its ring entry is free, its marks and its block counts are read.
    auto retire = [&](int e) {
        if (ring_jobs[size_t(e)] == 0) return true;
        if (hipEventSynchronize(ev[4 * e + 3]) != hipSuccess) return false;
        for (int k = 0; k < 3; k++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[4 * e + k], ev[4 * e + k + 1]) == hipSuccess) sp.ms[k == 0 ? 0 : k + 1] += ms;
        }
        for (int j = 0; j < ring_jobs[size_t(e)]; j++)
            count_long_chains(c, g.qidx_totals + (size_t(e) * size_t(n_slots) + size_t(ring_slot[size_t(e) * size_t(n_slots) + size_t(j)])) * kTotalsSlot);
        ring_jobs[size_t(e)] = 0;
        return true;
    };
    for (long t = 0; ok && !q.failed; t++) {
        const int e = int(t % kQIdxDepth);
        if (!(ok = retire(e))) break;
        // ---- which image each slot works on
        for (int k = 0; k < n_slots; k++) {
            Live &L = live[size_t(k)];
            if (L.im && L.row0 >= L.im->h) L.im = nullptr;               // (its worker has the buffer)
            IdxImage *I = L.im ? nullptr : q.next_image();
            if (!I) continue;
            Slot &s = g.slots[size_t(k)];
            const auto w0 = std::chrono::steady_clock::now();
            L.buf = bufs->take();                                         // every buffer out: the workers are behind
            sp.ms[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
            L.im = I; L.row0 = 0;
            L.lay = qidx_layout(*I, I->on_device && I->every);
            Locked &B = g.qidx_bufs[size_t(L.buf)];
            L.band = encoder_band_rows(q.band_rows, I->h, I->w, 1);
            const size_t n = size_t(I->h) * size_t(I->w), band_px = size_t(L.band) * size_t(I->w);
            // a workspace that has to grow is still read by the steps in the queue
            if ((band_px > s.px_cap || ((!I->on_device || I->collect) && n > s.d_img.capacity())) && hipStreamSynchronize(st) != hipSuccess) { ok = false; break; }
            if (!(ok = (L.lay.bytes <= B.capacity() * 2 || B.alloc((L.lay.bytes + L.lay.bytes / 8 + 4096) / 2)) && ensure_pixels(s, band_px, false) &&
                       (L.plane = idx_plane(q, *I, s, st)) != nullptr)) break;
        }
        if (!ok) break;
        // ---- 1. job records of the live slots, and the tasks of the bands that end on an entry row
        E1Job *const hj = g.qidx_jobs + size_t(e) * size_t(n_slots);
        IndexRecordTask *const ht = g.qidx_tasks + size_t(e) * size_t(n_slots);
        int n_jobs = 0, n_tasks = 0;
        const size_t ct_at = size_t(e) * size_t(n_slots);                // the step's stretch of the group's collect tasks
        collect_begin(g);
        for (int k = 0; k < n_slots && ok; k++) {
            const Live &L = live[size_t(k)];
            if (!L.im) continue;
            const size_t at = size_t(n_tasks) * rec_room;
            rec_at[size_t(n_jobs)] = idx_band_job(c, L, g.slots[size_t(k)], hj, n_jobs, ht, n_tasks, at) ? at : SIZE_MAX;
            ok = idx_collect_band(q, g, L, hj[n_jobs], ct_at);
            ring_slot[size_t(e) * size_t(n_slots) + size_t(n_jobs)] = k;
            slot_of[size_t(n_jobs++)] = k;
        }
        if (n_jobs == 0 || !ok) break;
        ok = hipMemcpyAsync(g.d_jobs, hj, size_t(n_jobs) * sizeof(E1Job), hipMemcpyHostToDevice, st) == hipSuccess &&
             (!n_tasks || hipMemcpyAsync(g.qidx_d_tasks, ht, size_t(n_tasks) * sizeof(IndexRecordTask), hipMemcpyHostToDevice, st) == hipSuccess);
        if (!ok) break;
        hipEventRecord(ev[4 * e], st);
        if (!(ok = collect_flush(g, st, ct_at))) break;                  // the bands of the sources: one launch
        // ---- 2. the model stage of every band, 3. the decoder records
        q_launch_model_band(g.d_jobs, hj, n_jobs, st);
        hipEventRecord(ev[4 * e + 1], st);
        q_launch_index_records(g.d_jobs, g.qidx_d_tasks, n_tasks, g.qidx_d_recs, st);
        hipEventRecord(ev[4 * e + 2], st);
        // ---- 4. the band's words and its record into the image's buffer; behind an image's last band its histograms
        //         (and a device input's rows), and the image goes to a worker
        ok = hipMemcpyAsync(g.qidx_totals + size_t(e) * size_t(n_slots) * kTotalsSlot, g.d_totals, size_t(n_slots) * kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
        for (int j = 0; j < n_jobs && ok; j++) {
            const int k = slot_of[size_t(j)];
            Live &L = live[size_t(k)];
            IdxImage *I = L.im;
            const Slot &s = g.slots[size_t(k)];
            uint8_t *const base = reinterpret_cast<uint8_t *>(static_cast<uint16_t *>(g.qidx_bufs[size_t(L.buf)]));
            const int rows = hj[j].h, r = L.row0 + rows;
            ok = hipMemcpyAsync(base + 2 * size_t(L.row0) * size_t(I->w), s.b.pxs, size_t(hj[j].n) * sizeof(uint16_t), hipMemcpyDeviceToHost, st) == hipSuccess;
            if (ok && rec_at[size_t(j)] != SIZE_MAX)
                ok = hipMemcpyAsync(base + L.lay.recs + size_t(r / I->every - 1) * L.lay.rec_stride, g.qidx_d_recs + rec_at[size_t(j)],
                                    kQDecodeStateBytes + 2 * size_t(I->w), hipMemcpyDeviceToHost, st) == hipSuccess;
            L.row0 = r;
            if (!ok || r < I->h) continue;
            const hipEvent_t ready = g.qidx_ready[size_t(L.buf)];
            ok = hipMemcpyAsync(base + L.lay.hist, s.b.qhist, 12 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
                 (L.lay.bytes == L.lay.rows || hipMemcpyAsync(base + L.lay.rows, L.plane, L.lay.bytes - L.lay.rows, hipMemcpyDeviceToHost, st) == hipSuccess) &&
                 hipEventRecord(ready, st) == hipSuccess;
            if (!ok) { L.row0 = 0; continue; }                           // (not handed over: the driver gives the buffer back below)
            const QIdxLayout lay = L.lay; const int buf = L.buf;
            q.pool.post([&q, bufs, I, base, lay, ready, buf] { qidx_finish(q, *I, base, lay, ready); bufs->give(buf); });
        }
        hipEventRecord(ev[4 * e + 3], st);
        ring_jobs[size_t(e)] = n_jobs;
        sp.steps++;
    }
    if (!ok) { q.failed = true; fprintf(stderr, "[nblic_amd] indexed effort-0 batch: a device step failed\n"); }
    const bool drained = hipStreamSynchronize(st) == hipSuccess;
    for (int e = 0; e < kQIdxDepth && ok && drained; e++) retire(e);
    for (auto &L : live) if (L.im && L.row0 < L.im->h && L.buf >= 0) bufs->give(L.buf);    // images the call ended under
    bufs->wait_all();
}

// ---- the frame itself ------------------------------------------------------------------------------------------------------
static const IdxCodec kIdxNblic{0, 1, size_t(kHeaderBytes) + 4, size_t(1) << 46, idx_driver};      // lossless -e1: `outs` in bytes
static const IdxCodec kIdxQnblic{1, 0, 6, size_t(1) << 45, qidx_driver};                           // effort 0: `outs` in 16-bit words

template <class Out>                                                     // unsigned char or uint16_t: what the codec's lengths count
static int indexed_batch(const IdxCodec &F, nblic_amd_ctx *c, int n, const unsigned char *const *imgs, bool on_device, const int *hs, const int *ws, const int *every,
                         int band_rows, Out *const *outs, const size_t *caps, long *lens, unsigned char *const *indexes, const size_t *icaps, long *ilens,
                         const CollectFrom *from = nullptr) {
    // `from`: imgs / on_device / hs / ws are collect_plan's (an image it refused is 0 x 0 and has no plane)
    if (!c || c->broken || n < 1 || !imgs || !hs || !ws || !every || !outs || !caps || !lens || (indexes && (!icaps || !ilens))) return -1;
    for (int k = 0; k < n; k++) if (every[k] < 0 || (!from && !imgs[k]) || !outs[k]) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    IdxCall q{F, c, n, imgs, on_device, band_rows, lens, ilens, from};
    q.images.resize(size_t(n));
    int n_live = 0;
    for (int k = 0; k < n; k++) {                                        // what can be refused is refused before anything is launched
        lens[k] = -1;
        if (ilens) ilens[k] = from && from->how[size_t(k)] == kSrcRefused ? -1 : 0;       // (a refused source: no stream and no index)
        if (!size_ok(hs[k], ws[k], c->max_px) || caps[k] < F.min_out) continue;
        auto I = std::make_unique<IdxImage>();
        I->k = k; I->h = hs[k]; I->w = ws[k]; I->out = outs[k]; I->cap = std::min(caps[k], F.max_out);
        I->host_plane = on_device ? nullptr : imgs[k];
        I->on_device = on_device; I->collect = from && from->how[size_t(k)] == kSrcCollect;
        if (indexes && indexes[k]) {
            const IndexAdmission A = index_admit(F.kind, F.effort, hs[k], ws[k], every[k], icaps[k]);
            if (A.too_small) ilens[k] = -1;                              // the stream is still delivered
            else { I->every = A.every; I->count = A.count; I->entry_bytes = A.entry_bytes; I->index = indexes[k]; }
        }
        q.images[size_t(k)] = std::move(I);
        n_live++;
    }
    if (n_live) {
        const int group_size = int(c->groups[0].slots.size());
        const int n_drivers = std::min(int(c->groups.size()), (n_live + group_size - 1) / group_size);
        q.pool.start(std::max(1, c->coders_wanted));
        std::vector<std::thread> drivers;
        for (int i = 0; i < n_drivers; i++) drivers.emplace_back([&q] { idx_run_driver(q); });
        for (auto &t : drivers) t.join();
    }
    {
        std::lock_guard<std::mutex> l(c->stat_m);
        for (int k = 0; k < 5; k++) c->idx_split[k] = q.split.ms[k];
        c->idx_steps = q.split.steps;
    }
    bool all = !q.failed;
    for (int k = 0; k < n; k++) {
        if (q.failed && q.images[size_t(k)]) q.fail(*q.images[size_t(k)]);
        all = all && lens[k] >= 0 && (!ilens || ilens[k] >= 0);
    }
    return all ? 0 : -1;
}

// ---- the INDEXED BATCH DECODE: the segments and row ranges of many streams in one call ----------------------------------
// The one indexed decode (nblic_amd_decode_indexed and nblic_amd_decode_rows are calls of it with one image): the host
// checks run on worker threads (one image: on the calling thread), every accepted image's stream (or, for a row range, its tail from the first entry's
// feed_from) and its index go up ONCE, the index verbatim, and all segments of all images form one job list
// (indexed_decode_plan: rounds that bound the per-segment memory, classes that share a launch; more segments than CUs take
// the lean image).  A round's segments are set up by k_index_seed straight from the uploaded index and their final records
// and B are compared with the next entries by k_index_chain before the round's buffers are reused; the rows part of that
// comparison runs once, after the last round -- at R = 1 the two rows above an entry belong to two segments that may run
// in different rounds.  Only the verdict words and one SerialState per image come back.
constexpr size_t kIndexedRoundBytes = size_t(1) << 30;   // device memory of one round's per-segment records and statistics

struct IdxDecImage {
    int k = 0;                          // the caller's image
    bool ok = false;
    IndexView V;
    DecodeItem it{};
    std::vector<uint8_t> qtab;
    int row0 = 0, row1 = 0, base = 0, seg0 = 0, seg1 = 0;       // rows wanted, first row of the device plane, first and last segment
    unsigned long long stream_off = 0;
    size_t out_bytes = 0;
    uint8_t *d_stream = nullptr, *d_index = nullptr, *d_plane = nullptr, *d_tab = nullptr;
    uint32_t *d_verdict = nullptr;      // one word per inner boundary, from boundary seg0 | seg0 + 1 on
    SerialState last{};                 // the last segment's final header
    DeliverTask deliver{};              // decode_batch_indexed_to: the image's window and destination
    bool live = false, bad = false;     // accepted by the host checks; found damaged after the decode
    size_t plane_bytes = 0;             // readable from d_plane
    // a packed index: where its parts lie (for the device), the payload offsets, and this round's unpacked entries
    unsigned long long *d_desc = nullptr; uint32_t *d_offs = nullptr;
    IndexUnpackTask unpack{};           // all but the round's fields
    uint8_t *d_unpacked = nullptr; int unpacked_first = 0;       // entry unpacked_first (1-based) lies at d_unpacked, the next ones unpack.out_stride apart
};

// The device's view of a checked packed index: its parts without the QNBLIC tables (nothing on the device reads an entry's),
// and where every part of entries 0 .. walk - 1 lies.
static void idxdec_unpack_task(const IndexView &V, int walk, IndexUnpackTask &T, std::vector<unsigned long long> &desc) {
    const PackedView &P = V.P;
    T = IndexUnpackTask{};
    std::vector<int> parts;
    for (int j = 0; j < P.n_parts; j++) {
        const PackPart &p = P.parts[j];
        if (p.at >= V.L.tab) continue;
        T.part[parts.size()] = IndexUnpackPart{p.at, p.bytes, p.unit, p.code, p.init, T.blocks};
        T.blocks += part_blocks(p);
        parts.push_back(j);
    }
    T.n_parts = uint32_t(parts.size());
    T.walk = uint32_t(walk);
    T.out_stride = uint32_t((V.L.tab + 15) & ~size_t(15));
    desc.clear();
    for (int e = 0; e < walk; e++)
        for (int j : parts) desc.push_back((unsigned long long)(P.ent[size_t(e)].part_at[j]) | ((unsigned long long)(P.ent[size_t(e)].part_flag[j]) << 56));
}

// A task's place in a launch: the waves and workgroups of the tasks in front of it (serial_engine.h first_*).  The scan launch
// takes the task as idxdec_unpack_task made it; a round's launch the entries it stores, [first_out, walk), and where.
static void idxdec_place_scan(IndexUnpackTask T, uint32_t &scan_waves, std::vector<IndexUnpackTask> &tasks) {
    T.first_scan_wave = scan_waves; scan_waves += index_unpack_scan_waves(T);
    tasks.push_back(T);
}
static void idxdec_place_round(IndexUnpackTask T, uint8_t *out, int walk, int first_out, uint32_t &waves, uint32_t &groups, std::vector<IndexUnpackTask> &tasks) {
    T.out = out; T.walk = uint32_t(walk); T.first_out = uint32_t(first_out);
    T.first_wave = waves; waves += index_unpack_waves(T);
    T.first_rank_group = groups; groups += index_unpack_rank_groups(T);
    tasks.push_back(T);
}

static bool idxdec_upload_tasks(std::vector<IndexTask> &tasks, bool seed, IndexTask *d_tasks, uint32_t &chunks, hipStream_t st) {
    chunks = 0;
    for (auto &t : tasks) { t.first_chunk = chunks; chunks += index_task_chunks(t, seed); }
    return tasks.empty() || hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(IndexTask), hipMemcpyHostToDevice, st) == hipSuccess;
}

static int decode_batch_indexed(nblic_amd_ctx *c, int n, const unsigned char *const *streams, const size_t *slens, const void *const *indexes,
                                const size_t *ilens, const int *row0, const int *row1, unsigned char *const *outs, const size_t *caps,
                                int *hs, int *ws, int *nears, int *efforts, int *status, const DeliverTo *to = nullptr) {
    // `to`: the rows go to the caller's device memory (k_deliver) instead of outs; row0 / row1 / outs / caps are not read
    if (!c || c->broken || n < 1 || !streams || !slens || !indexes || !ilens || (!to && (!outs || !caps)) || !hs || !ws || !nears || !efforts || !status) return -1;
    if ((row0 == nullptr) != (row1 == nullptr)) return -1;
    for (int k = 0; k < n; k++) if (!streams[k] || !indexes[k] || (!to && !outs[k])) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    using Clock = std::chrono::steady_clock;
    auto ms_since = [](Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); };
    double split[4] = {0, 0, 0, 0};
    auto t0 = Clock::now();
    // the host half: index against stream, the stream's description -- nothing of an image goes up before it has passed
    std::vector<IdxDecImage> all{size_t(n)};
    auto host_check = [&](int k) {
        IdxDecImage &I = all[size_t(k)];
        I.k = k;
        I.it = DecodeItem{k, 0, 0, 0, 0, 0, 0, 0, -1, -1};
        I.ok = index_check(indexes[k], ilens[k], streams[k], slens[k], c->max_px, I.V) == 0 &&
               describe_stream(streams[k], slens[k], false, c->max_px, I.it, I.qtab) == Described::ok;
    };
    if (n == 1) {
        host_check(0);                                                   // (the single calls: no thread is worth starting for one image)
    } else {
        IdxPool pool;
        IdxPendingTasks pending;
        pending.add(n);
        pool.start(std::max(1, std::min(n, c->coders_wanted)));
        for (int k = 0; k < n; k++) pool.post([&, k] { host_check(k); pending.done(); });
        pending.wait();
    }
    split[0] = ms_since(t0);
    std::vector<IdxDecImage *> live;
    std::vector<IndexedPlanImage> plan_in;
    size_t per_seg_max = 1;
    for (int k = 0; k < n; k++) {
        IdxDecImage &I = all[size_t(k)];
        status[k] = -1; hs[k] = ws[k] = 0; nears[k] = efforts[k] = 0;
        if (!I.ok) continue;
        const DecodeItem &it = I.it;
        hs[k] = it.h; ws[k] = it.w; nears[k] = it.near; efforts[k] = it.effort;
        if (to) {                                                        // the window's rows choose the segments; its columns do not shorten the decode
            if (!(to->deep_modes ? deep_dest_window(c, *to, k, it.h, it.w, I.deliver) : deliver_dest_task(c, *to, k, it.h, it.w, I.deliver))) continue;
            I.row0 = I.deliver.row0; I.row1 = I.deliver.row1;
        } else {
            I.row0 = row0 ? row0[k] : 0; I.row1 = row1 ? row1[k] : it.h;
        }
        if (I.row0 < 0 || I.row1 <= I.row0 || I.row1 > it.h) continue;
        I.out_bytes = size_t(I.row1 - I.row0) * size_t(it.w);
        if (!to && caps[k] < I.out_bytes) continue;
        const int R = I.V.H.every_rows;
        I.seg0 = I.row0 / R; I.seg1 = (I.row1 - 1) / R;
        I.base = std::max(0, I.seg0 * R - 2);
        if (I.seg0 > 0) {                                                // <= slen (index_check)
            DecodeCheckpoint E;
            memcpy(&E, I.V.ent[size_t(I.seg0 - 1)], sizeof E);
            I.stream_off = E.feed_from;
        }
        // (a round's segments s .. t of an image need its entries s .. t + 1 unpacked: no more than two per segment)
        per_seg_max = std::max(per_seg_max, up256(I.V.L.b) + up256(2 * I.V.L.b_bytes) + (I.V.packed ? 2 * up256(I.V.L.tab + 15) : 0));
        I.live = true;
    }
    if (to && to->modes)                                                 // a colour frame with a difference stands or falls as a whole: three lossless planes of one size, one window
        for (int f = 0; f + 2 < n; f += 3) {
            if (to->mode_of(f) == kColorPlain) continue;
            IdxDecImage &A = all[size_t(f)], &B = all[size_t(f) + 1], &D = all[size_t(f) + 2];
            const bool ok = A.live && B.live && D.live && A.it.h == B.it.h && A.it.h == D.it.h && A.it.w == B.it.w && A.it.w == D.it.w &&
                            !A.it.near && !B.it.near && !D.it.near && same_window(A.deliver, B.deliver) && same_window(A.deliver, D.deliver);
            if (!ok) A.live = B.live = D.live = false;
        }
    if (to && to->slice_modes)                                           // a stack with a delta stands or falls as a whole: slices of one size and one window, lossless inside its runs
        for (int s = 0; s + to->depth <= n; s += to->depth) {
            if (!to->stack_has_delta(s)) continue;
            const IdxDecImage &A = all[size_t(s)];
            bool ok = true;
            for (int k = s; k < s + to->depth && ok; k++) {
                const IdxDecImage &I = all[size_t(k)];
                const bool in_run = to->slice_modes[k] == kStackDelta || (k + 1 < s + to->depth && to->slice_modes[k + 1] == kStackDelta);
                ok = A.live && I.live && I.it.h == A.it.h && I.it.w == A.it.w && same_window(I.deliver, A.deliver) && !(in_run && I.it.near);
            }
            if (!ok) for (int k = s; k < s + to->depth; k++) all[size_t(k)].live = false;
        }
    if (to && to->deep_modes)                                            // a deep image stands or falls as a whole: two planes of one size
        for (int k = 0; k + 1 < n; k += 2) {
            IdxDecImage &A = all[size_t(k)], &B = all[size_t(k) + 1];
            if (!(A.live && B.live && A.it.h == B.it.h && A.it.w == B.it.w)) A.live = B.live = false;
        }
    for (int k = 0; k < n; k++) {
        IdxDecImage &I = all[size_t(k)];
        if (!I.live) continue;
        plan_in.push_back(IndexedPlanImage{I.it.kind, I.it.effort, I.it.h, I.it.w, I.V.H.every_rows, I.row0, I.row1});
        live.push_back(&I);
    }
    if (live.empty()) return -1;
    size_t cap = std::max<size_t>(1, kIndexedRoundBytes / per_seg_max);
    if (c->index_round_segments > 0) cap = std::min(cap, size_t(c->index_round_segments));
    std::vector<IndexedJob> plan;
    if (!indexed_decode_plan(plan_in.data(), int(plan_in.size()), int(std::min<size_t>(cap, size_t(1) << 30)), plan)) return -1;

    // from here on a failure is the device's: every accepted image fails, and nothing unverified stays in its buffer
    Stream st;                                                           // declared before the buffers: they go first
    DevPool mem;
    auto fail = [&](const char *what) {
        fprintf(stderr, "[nblic_amd] indexed batch decode: %s\n", what);
        if (st) hipStreamSynchronize(st);
        for (IdxDecImage *I : live) { status[I->k] = -1; if (!to) memset(outs[I->k], 0, I->out_bytes); }
        if (to && to->deep_modes) {
            std::vector<const DeliverTask *> of(size_t(n), nullptr);
            for (IdxDecImage *I : live) of[size_t(I->k)] = &I->deliver;
            deliver_deep_zeros(*to, of, st);
        } else if (to) {
            std::vector<DeliverTask> zeros;
            for (IdxDecImage *I : live) zeros.push_back(I->deliver);
            deliver_zeros(zeros, st);
        }
        return -1;
    };
    if (st.create(hipStreamNonBlocking) != hipSuccess) return fail("cannot create a stream");
    t0 = Clock::now();
    size_t n_bounds = 0;
    for (IdxDecImage *I : live) n_bounds += size_t(I->seg1 - I->seg0);
    // (device blocks are carved out of few allocations, every part at a multiple of 256 bytes: a call with one image makes three)
    const size_t verdict_bytes = up256(std::max<size_t>(1, n_bounds) * sizeof(uint32_t));
    const size_t unpack_task_bytes = up256(live.size() * sizeof(IndexUnpackTask));
    uint8_t *d_call = mem.make<uint8_t>(verdict_bytes + unpack_task_bytes + (to ? live.size() * sizeof(DeliverTask) : 0));
    uint32_t *d_verdicts = reinterpret_cast<uint32_t *>(d_call);
    if (!d_verdicts || hipMemsetAsync(d_verdicts, 0, std::max<size_t>(1, n_bounds) * sizeof(uint32_t), st) != hipSuccess) return fail("cannot allocate the workspace");
    {
        size_t at = 0;
        for (IdxDecImage *I : live) {
            const DecodeItem &it = I->it;
            const size_t win = size_t(it.len - I->stream_off), ilen = ilens[I->k];
            I->d_verdict = d_verdicts + at; at += size_t(I->seg1 - I->seg0);
            const size_t index_bytes = up256(ilen + 16);                    // (the kernels read whole aligned words around an entry)
            const size_t plane_bytes = up256(size_t(I->row1 - I->base) * size_t(it.w));
            I->d_stream = mem.make<uint8_t>(stream_buf_bytes(win) + index_bytes + plane_bytes + (it.kind ? kQTab : 0));
            if (!I->d_stream) return fail("cannot allocate the workspace");
            I->d_index = I->d_stream + stream_buf_bytes(win);
            I->d_plane = I->d_index + index_bytes;
            if (to) {                                                    // the window's rows count from the plane's first: row `base` of the image
                I->deliver.src = I->d_plane; I->deliver.src_bytes = plane_bytes; I->plane_bytes = plane_bytes;
                I->deliver.row0 -= I->base; I->deliver.row1 -= I->base;
            }
            if (it.kind) I->d_tab = I->d_plane + plane_bytes;
            if (!upload_stream(I->d_stream, streams[I->k] + I->stream_off, win, st) ||
                hipMemcpyAsync(I->d_index, indexes[I->k], ilen, hipMemcpyHostToDevice, st) != hipSuccess ||
                (it.kind && hipMemcpyAsync(I->d_tab, I->qtab.data(), kQTab, hipMemcpyHostToDevice, st) != hipSuccess)) return fail("upload");
        }
    }
    // the packed indexes among them: where their parts lie, and every block's payload offset (one scan launch for the call)
    std::vector<std::vector<unsigned long long>> descs(live.size());
    std::vector<IndexUnpackTask> unpacks;
    IndexUnpackTask *d_unpacks = reinterpret_cast<IndexUnpackTask *>(d_call + verdict_bytes);
    {
        uint32_t scan_waves = 0;
        for (size_t i = 0; i < live.size(); i++) {
            IdxDecImage *I = live[i];
            if (!I->V.packed) continue;
            const int walk = I->seg1;                                    // entries 1 .. seg1, 0-based 0 .. walk - 1, are all this call reads
            idxdec_unpack_task(I->V, walk, I->unpack, descs[i]);
            I->d_desc = mem.make<unsigned long long>(std::max<size_t>(1, descs[i].size()));
            I->d_offs = mem.make<uint32_t>(std::max<size_t>(1, size_t(walk) * I->unpack.blocks));
            if (!I->d_desc || !I->d_offs) return fail("cannot allocate the workspace");
            if (!descs[i].empty() && hipMemcpyAsync(I->d_desc, descs[i].data(), descs[i].size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload");
            I->unpack.packed = I->d_index; I->unpack.desc = I->d_desc; I->unpack.offs = I->d_offs;
            if (walk == 0) continue;
            idxdec_place_scan(I->unpack, scan_waves, unpacks);
        }
        if (!unpacks.empty() && (hipMemcpyAsync(d_unpacks, unpacks.data(), unpacks.size() * sizeof(IndexUnpackTask), hipMemcpyHostToDevice, st) != hipSuccess ||
                                 !index_unpack_scan_launch(d_unpacks, int(unpacks.size()), scan_waves, st))) return fail("launch");
    }
    // the rounds' shared buffers: records and statistics, jobs, tasks
    const int n_rounds = plan.back().round + 1;
    std::vector<size_t> round_begin(size_t(n_rounds) + 1, plan.size());
    size_t rec_bytes_max = 0, jobs_max = 0, unpacked_max = 0;
    for (size_t j = plan.size(); j-- > 0;) round_begin[size_t(plan[j].round)] = j;
    // the entries (1-based) of image I that a round's segments [s_lo, s_hi] read: every seed but segment 0's, the one behind each
    auto round_entries = [](const IdxDecImage &I, int s_lo, int s_hi, int &first, int &last) {
        first = std::max(1, s_lo); last = std::min(s_hi + 1, I.seg1);    // (the last segment of the range ends at no boundary; seg1 <= count)
    };
    for (int r = 0; r < n_rounds; r++) {
        size_t bytes = 0, unpacked = 0;
        for (size_t j = round_begin[size_t(r)]; j < round_begin[size_t(r) + 1]; j++) {
            const IdxDecImage &I = *live[size_t(plan[j].image)];
            const RecordLayout &L = I.V.L;
            bytes += up256(L.b) + up256(2 * L.b_bytes);
            if (I.V.packed && (j + 1 == round_begin[size_t(r) + 1] || plan[j + 1].image != plan[j].image)) {     // the image's last job of the round: its lowest segment
                size_t a = j;
                while (a > round_begin[size_t(r)] && plan[a - 1].image == plan[j].image) a--;
                int first, last;
                round_entries(I, plan[j].segment, plan[a].segment, first, last);
                if (last >= first) unpacked += up256(size_t(last - first + 1) * I.unpack.out_stride);
            }
        }
        rec_bytes_max = std::max(rec_bytes_max, bytes);
        unpacked_max = std::max(unpacked_max, unpacked);
        jobs_max = std::max(jobs_max, round_begin[size_t(r) + 1] - round_begin[size_t(r)]);
    }
    const size_t round_part[5] = {up256(rec_bytes_max), up256(jobs_max * sizeof(SerialJob)), up256(std::max(jobs_max, n_bounds) * sizeof(IndexTask)),
                                  up256(jobs_max * sizeof(IndexTask)), up256(unpacked_max)};
    uint8_t *d_recs = mem.make<uint8_t>(round_part[0] + round_part[1] + round_part[2] + round_part[3] + round_part[4]);
    if (!d_recs) return fail("cannot allocate the workspace");
    SerialJob *d_jobs = reinterpret_cast<SerialJob *>(d_recs + round_part[0]);
    IndexTask *d_tasks = reinterpret_cast<IndexTask *>(d_recs + round_part[0] + round_part[1]);
    IndexTask *d_tasks2 = reinterpret_cast<IndexTask *>(d_recs + round_part[0] + round_part[1] + round_part[2]);
    uint8_t *d_unpacked = d_recs + round_part[0] + round_part[1] + round_part[2] + round_part[3];
    if (hipStreamSynchronize(st) != hipSuccess) return fail("upload");
    split[1] = ms_since(t0);
    t0 = Clock::now();
    // the part of an entry a task names: record, B, rows above row r of image I
    auto entry_task = [&](const IdxDecImage &I, int e, uint8_t *rec, uint8_t *stats, uint32_t parts) {
        const RecordLayout &L = I.V.L;
        const int r = e * I.V.H.every_rows;
        const RowsAbove A = rows_above(r, I.it.w);
        IndexTask T{};
        bool rows_direct = false;                                        // T.entry is the row slot itself, not the body
        if (e > 0 && I.V.packed) {
            if (parts == kChainRows) {                                   // after the last round: the rows lie raw in the packed index
                const PackedEntry &E = I.V.P.ent[size_t(e - 1)];
                int j = 0;
                while (I.V.P.parts[j].at != L.rows) j++;
                T.entry = I.d_index + E.part_at[j];
                rows_direct = true;
            } else {
                T.entry = I.d_unpacked + size_t(e - I.unpacked_first) * I.unpack.out_stride;
            }
        } else {
            T.entry = e > 0 ? I.d_index + size_t(I.V.body(e) - static_cast<const uint8_t *>(indexes[I.k])) : nullptr;
        }
        T.rec = rec; T.stats = stats;
        T.rows = I.d_plane + size_t(A.first - I.base) * size_t(I.it.w);
        T.avail = I.it.len; T.first_pos = first_pos(I.it);
        T.rec_bytes = (parts & kChainRecord) ? uint32_t(L.b) : 0u;
        T.b_bytes = (parts & kChainB) ? uint32_t(L.b_bytes) : 0u;
        T.rows_bytes = (parts & kChainRows) && e > 0 ? uint32_t(size_t(A.n) * size_t(I.it.w)) : 0u;
        T.b_at = uint32_t(L.b); T.rows_at = uint32_t((rows_direct ? 0 : L.rows) + A.at);
        T.kind = uint32_t(I.it.kind);
        return T;
    };
    std::vector<SerialJob> jobs(jobs_max);
    std::vector<IndexTask> seeds, chains;
    long launches_total = 0;
    for (int r = 0; r < n_rounds; r++) {
        const size_t j0 = round_begin[size_t(r)], j1 = round_begin[size_t(r) + 1];
        seeds.clear(); chains.clear(); unpacks.clear();
        // the packed images of the round: their entries, unpacked
        {
            size_t at = 0;
            uint32_t waves = 0, groups = 0;
            for (size_t j = j0; j < j1;) {
                size_t b = j + 1;
                while (b < j1 && plan[b].image == plan[j].image) b++;
                IdxDecImage &I = *live[size_t(plan[j].image)];
                int first = 1, last = 0;
                if (I.V.packed) round_entries(I, plan[b - 1].segment, plan[j].segment, first, last);
                if (last >= first) {
                    I.d_unpacked = d_unpacked + at; I.unpacked_first = first;
                    at += up256(size_t(last - first + 1) * I.unpack.out_stride);
                    idxdec_place_round(I.unpack, I.d_unpacked, last, first - 1, waves, groups, unpacks);
                }
                j = b;
            }
            if (!unpacks.empty() && (hipMemcpyAsync(d_unpacks, unpacks.data(), unpacks.size() * sizeof(IndexUnpackTask), hipMemcpyHostToDevice, st) != hipSuccess ||
                                     !index_unpack_launch(d_unpacks, int(unpacks.size()), waves, groups, st))) return fail("launch");
        }
        size_t at = 0;
        for (size_t j = j0; j < j1; j++) {
            const IndexedJob &P = plan[j];
            IdxDecImage &I = *live[size_t(P.image)];
            const RecordLayout &L = I.V.L;
            uint8_t *rec = d_recs + at; at += up256(L.b);
            uint8_t *stats = L.b_bytes ? d_recs + at : nullptr; at += up256(2 * L.b_bytes);
            jobs[j - j0] = decode_job(I.it, I.d_plane, I.base, I.d_stream, I.stream_off, reinterpret_cast<SerialState *>(rec), reinterpret_cast<double *>(stats),
                                      I.d_tab, rows_per_launch(I.it, c->serial_rows), P.end_row, c->d_redo);
            seeds.push_back(entry_task(I, P.segment, rec, stats, kChainRecord | kChainB | kChainRows));
            if (P.segment < I.seg1) {                                    // its end is an inner boundary: record and B now, the rows after the last round
                IndexTask T = entry_task(I, P.segment + 1, rec, stats, kChainRecord | kChainB);
                T.verdict = I.d_verdict + (P.segment - I.seg0);
                chains.push_back(T);
            }
        }
        uint32_t seed_chunks = 0, chain_chunks = 0;
        if (!idxdec_upload_tasks(seeds, true, d_tasks, seed_chunks, st) || !idxdec_upload_tasks(chains, false, d_tasks2, chain_chunks, st) ||
            hipMemcpyAsync(d_jobs, jobs.data(), (j1 - j0) * sizeof(SerialJob), hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload");
        if (!index_seed_launch(d_tasks, int(seeds.size()), seed_chunks, st)) return fail("launch");
        for (size_t a = j0; a < j1;) {                                   // one launch sequence per class present
            size_t b = a + 1;
            int launches = 1;
            while (b < j1 && plan[b].cls == plan[a].cls) b++;
            for (size_t j = a; j < b; j++) {
                const IndexedJob &P = plan[j];
                const SerialJob &J = jobs[j - j0];
                launches = std::max(launches, serial_launches((P.end_row ? P.end_row : J.h) - P.first_row, J.rows));
            }
            for (int l = 0; l < launches; l++)
                if (!decode_launch(live[size_t(plan[a].image)]->it, d_jobs + (a - j0), jobs.data() + (a - j0), int(b - a), st, true)) return fail("launch");
            launches_total += launches;
            a = b;
        }
        if (!index_chain_launch(d_tasks2, int(chains.size()), chain_chunks, st)) return fail("launch");
        for (size_t j = j0; j < j1; j++) {
            IdxDecImage &I = *live[size_t(plan[j].image)];
            if (plan[j].segment == I.seg1 && hipMemcpyAsync(&I.last, jobs[j - j0].state, sizeof(SerialState), hipMemcpyDeviceToHost, st) != hipSuccess) return fail("state");
        }
        if (hipStreamSynchronize(st) != hipSuccess) return fail("a round");       // the records, `jobs` and the task arrays are reused by the next round
    }
    { std::lock_guard<std::mutex> l(c->stat_m); c->serial_launch_count += launches_total; }
    // every row is final now: the rows part of every boundary, then the verdicts
    chains.clear();
    for (IdxDecImage *I : live)
        for (int s = I->seg0; s < I->seg1; s++) {
            IndexTask T = entry_task(*I, s + 1, nullptr, nullptr, kChainRows);
            T.verdict = I->d_verdict + (s - I->seg0);
            if (T.rows_bytes) chains.push_back(T);
        }
    uint32_t chain_chunks = 0;
    std::vector<uint32_t> verdicts(std::max<size_t>(1, n_bounds));
    if (!idxdec_upload_tasks(chains, false, d_tasks, chain_chunks, st) || !index_chain_launch(d_tasks, int(chains.size()), chain_chunks, st) ||
        hipMemcpyAsync(verdicts.data(), d_verdicts, verdicts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail("the chain check");
    split[2] = ms_since(t0);
    t0 = Clock::now();
    bool every = true;
    std::vector<DeliverTask> deliveries;
    for (IdxDecImage *I : live) {
        uint32_t bad = 0;
        for (int s = I->seg0; s < I->seg1; s++) bad |= verdicts[size_t(I->d_verdict - d_verdicts) + size_t(s - I->seg0)];
        const bool ended = I->row1 == I->it.h ? I->last.status == kDone : (I->last.status == kRunning && I->last.next_row == I->row1);
        I->bad = bad || !ended;
        if (I->bad)
            fprintf(stderr, "[nblic_amd] indexed batch decode: image %d: %s\n", I->k,
                    bad ? "a segment does not end where the next entry starts (index and stream disagree)" : "the stream is damaged or ends too early");
    }
    if (to && to->modes)                                                 // a frame with a damaged plane has none; a difference refers to the base's plane, whose first row may be another
        for (IdxDecImage *I : live) {
            const size_t f = size_t(I->k - I->k % 3);
            const int ref = color_mode_ref(to->mode_of(I->k), uint32_t(I->k % 3));
            if (ref < 0) continue;
            IdxDecImage &G = all[f + size_t(ref)];
            if (all[f].bad || all[f + 1].bad || all[f + 2].bad) continue;
            const size_t skip = size_t(I->row0 - G.base) * size_t(I->it.w);
            I->deliver.ref = G.d_plane + skip; I->deliver.ref_bytes = G.plane_bytes - skip; I->deliver.ref_pitch = uint32_t(I->it.w);
        }
    const bool stack = to && to->slice_modes;
    StackDelivery stack_plan;
    if (stack) {
        // ONE k_deliver launch for the lone key slices and ONE k_deliver_stack launch for the runs: a damaged plane is known
        // here, so it and every later slice of its run get zeros (the record's zero) and -1; a skipped slice has its plane's status.
        std::vector<const DeliverTask *> of(size_t(n), nullptr);
        for (IdxDecImage *I : live) {
            I->deliver.zero = I->bad ? 1u : 0u;
            of[size_t(I->k)] = &I->deliver;
            status[I->k] = I->bad ? -1 : 0;
        }
        stack_delivery_plan(*to, n, of, stack_plan);
        // (the call's workspace is a pool of its own: the three tables are three more blocks of it)
        if (!stack_delivery_queue(c, stack_plan, mem.make<DeliverTask>(stack_plan.plain.size()), mem.make<StackDeliverTask>(stack_plan.runs.size()),
                                  mem.make<StackSlice>(stack_plan.slices.size()), st)) return fail("delivery");
        for (int s = 0; s + to->depth <= n; s += to->depth)
            for (int d = 1, bad = status[s] != 0; d < to->depth; d++) {
                if (to->slice_modes[s + d] == kStackKey) bad = 0;
                bad = bad || status[s + d] != 0;
                if (bad && !to->skipped(s + d)) status[s + d] = -1;
            }
    }
    const bool deep = to && to->deep_modes;
    std::vector<DeepDeliverTask> deep_tasks;                             // (alive until the stream has been waited for)
    Event deep_marks[2];
    if (deep) {
        // ONE k_deliver_deep launch, a task per deep image: a damaged plane is known here, so its image gets zeros and -1 for both
        for (int k = 0; k + 1 < n; k += 2) {
            IdxDecImage &A = all[size_t(k)], &B = all[size_t(k) + 1];
            if (!A.live || !B.live) continue;
            A.deliver.zero = B.deliver.zero = (A.bad || B.bad) ? 1u : 0u;
            deep_tasks.push_back(deep_deliver_task(*to, k / 2, A.deliver, B.deliver));
            status[k] = status[k + 1] = (A.bad || B.bad) ? -1 : 0;
        }
        if (!deliver_deep_queue(c, deep_tasks.data(), deep_tasks.size(), mem.make<DeepDeliverTask>(deep_tasks.size()), st, deep_marks)) return fail("delivery");
    }
    if (!stack && !deep) for (IdxDecImage *I : live) {
        const size_t f = size_t(I->k - I->k % 3);
        if (I->bad || (to && to->mode_of(I->k) != kColorPlain && (all[f].bad || all[f + 1].bad || all[f + 2].bad))) {
            if (to) { I->deliver.zero = 1; deliveries.push_back(I->deliver); }
            else memset(outs[I->k], 0, I->out_bytes);
            continue;
        }
        if (to) deliveries.push_back(I->deliver);
        else if (hipMemcpyAsync(outs[I->k], I->d_plane + size_t(I->row0 - I->base) * size_t(I->it.w), I->out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return fail("rows");
        status[I->k] = 0;
    }
    // `to`: ONE launch delivers every live image's window -- zeros for the images that failed above
    if (to && !deliver_queue(deliveries.data(), deliveries.size(), reinterpret_cast<DeliverTask *>(d_call + verdict_bytes + unpack_task_bytes), st, c)) return fail("delivery");
    if (hipStreamSynchronize(st) != hipSuccess) return fail("rows");
    if (stack) stack_delivery_timed(c, stack_plan);
    if (deep) deep_timed(c, deep_marks, 2);
    split[3] = ms_since(t0);
    { std::lock_guard<std::mutex> l(c->stat_m); for (int k = 0; k < 4; k++) c->idxdec_split[k] = split[k]; }
    for (int k = 0; k < n; k++) every = every && status[k] == 0;
    return every ? 0 : -1;
}

// ---- the BATCH INDEX BUILD: the seek indexes of many streams from one decode pass -----------------------------------------
// What index_build does for one stream per call -- one wave of the band decoder, a host round trip at every band and every
// entry -- done for many: every accepted stream goes up once and is decoded whole, side by side with the others of its
// class, and stops in front of each of its entry rows (SerialJob::end_row), where k_index_capture turns the device state
// into the entry's body and moves end_row on.  While no stream fails a job's progress is known beforehand, so the launches
// of the whole call and the capture tasks behind each are laid out on the host (index_entries.h index_build_plan), uploaded
// once and queued back to back; the host waits once, then worker threads put the indexes together -- heads, row hashes,
// seals -- from one copy of each image's staged bodies and one of its plane.
struct IdxBuildImage {
    int k = 0;                          // the caller's image
    bool ok = false;                    // described
    DecodeItem it{};
    std::vector<uint8_t> qtab;
    int every = 0, count = 0;
    RecordLayout L{};
    size_t entry_bytes = 0, need = 0, stride = 0, plane_bytes = 0;      // stride: of one staged body
    uint8_t *d_stream = nullptr, *d_plane = nullptr, *d_rec = nullptr, *d_stats = nullptr, *d_tab = nullptr, *d_stage = nullptr;
    SerialState last{};                 // the record's header after the last launch
    bool good = false;
};
static size_t build_stage_stride(const RecordLayout &L) { return (L.tab + 15) & ~size_t(15); }      // record | B | the row slot

static IndexCaptureTask capture_task(const DecodeItem &it, const RecordLayout &L, int row, int next_end, const uint8_t *rec, const uint8_t *stats,
                                     const uint8_t *plane, int plane_row0, uint8_t *out, SerialJob *job) {
    const RowsAbove A = rows_above(row, it.w);
    IndexCaptureTask T{};
    T.rec = rec; T.stats = L.b_bytes ? stats : nullptr;
    T.rows = plane + size_t(A.first - plane_row0) * size_t(it.w);
    T.out = out; T.job = job;
    T.row = row; T.next_end = next_end;
    T.rec_bytes = uint32_t(L.b); T.b_bytes = uint32_t(L.b_bytes);
    T.rows_lead = uint32_t(A.at); T.rows_bytes = uint32_t(size_t(A.n) * size_t(it.w));
    T.kind = uint32_t(it.kind);
    return T;
}

static int index_build_batch(nblic_amd_ctx *c, int n, const unsigned char *const *streams, const size_t *slens, const int *every_rows,
                             unsigned char *const *indexes, const size_t *icaps, long *ilens, unsigned char *const *planes, const size_t *pcaps,
                             int *hs, int *ws, int *nears, int *efforts, int *status) {
    if (!c || c->broken || n < 1 || !streams || !slens || !every_rows || !indexes || !icaps || !ilens || (planes && !pcaps) || !hs || !ws || !nears ||
        !efforts || !status) return -1;
    for (int k = 0; k < n; k++) if (!streams[k] || !indexes[k]) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    using Clock = std::chrono::steady_clock;
    auto ms_since = [](Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); };
    double split[4] = {0, 0, 0, 0};
    auto t0 = Clock::now();
    std::vector<IdxBuildImage> all{size_t(n)};
    IdxPool pool;
    IdxPendingTasks pending;
    const int n_workers = std::max(1, std::min(n, c->coders_wanted));
    pool.start(n_workers);
    pending.add(n);
    for (int k = 0; k < n; k++)
        pool.post([&, k] {
            IdxBuildImage &I = all[size_t(k)];
            I.k = k;
            I.it = DecodeItem{k, 0, 0, 0, 0, 0, 0, 0, -1, -1};
            I.ok = describe_stream(streams[k], slens[k], false, c->max_px, I.it, I.qtab) == Described::ok;
            pending.done();
        });
    pending.wait();
    split[0] = ms_since(t0);
    std::vector<IdxBuildImage *> live;
    for (int k = 0; k < n; k++) {
        IdxBuildImage &I = all[size_t(k)];
        status[k] = -1; ilens[k] = -1; hs[k] = ws[k] = 0; nears[k] = efforts[k] = 0;
        if (!I.ok) continue;
        const DecodeItem &it = I.it;
        hs[k] = it.h; ws[k] = it.w; nears[k] = it.near; efforts[k] = it.effort;
        const long need = index_bytes(it.kind, it.h, it.w, it.effort, every_rows[k]);     // -1: every_rows < 1 or >= h, as index_build refuses it
        I.plane_bytes = size_t(it.h) * size_t(it.w);
        if (need < 0 || icaps[k] < size_t(need) || (planes && planes[k] && pcaps[k] < I.plane_bytes)) continue;
        I.every = every_rows[k]; I.count = (it.h - 1) / I.every;
        I.L = record_layout(it.kind, it.w, it.effort);
        I.entry_bytes = index_entry_bytes(it.kind, it.w, it.effort); I.need = size_t(need);
        I.stride = build_stage_stride(I.L);
        if (I.entry_bytes != sizeof(DecodeCheckpoint) + I.L.bytes + 32) continue;        // (the two descriptions of an entry agree)
        live.push_back(&I);
    }
    if (live.empty()) return -1;
    std::stable_sort(live.begin(), live.end(), [](const IdxBuildImage *a, const IdxBuildImage *b) {
        return indexed_class(a->it.kind, a->it.effort) < indexed_class(b->it.kind, b->it.effort); });
    const size_t m = live.size();
    std::vector<BuildPlanImage> plan_in;
    for (const IdxBuildImage *I : live) plan_in.push_back(BuildPlanImage{I->it.kind, I->it.effort, I->it.h, I->it.w, I->every, rows_per_launch(I->it, c->serial_rows)});
    BuildPlan plan;
    if (!index_build_plan(plan_in.data(), int(m), plan)) return -1;

    // from here on a failure is the device's: every accepted image fails, and nothing unverified stays in its buffers
    Stream st;                                                           // declared before the buffers: they go first
    std::vector<Stream> copy_st{size_t(std::min(n_workers, 4))};        // the finish: the workers' copies share these (a stream costs milliseconds to make)
    std::vector<std::mutex> copy_m{copy_st.size()};
    DevPool mem;
    auto drop = [&](const IdxBuildImage &I) {
        status[I.k] = -1; ilens[I.k] = -1;
        memset(indexes[I.k], 0, I.need);
        if (planes && planes[I.k]) memset(planes[I.k], 0, I.plane_bytes);
    };
    auto fail = [&](const char *what) {
        fprintf(stderr, "[nblic_amd] batch index build: %s\n", what);
        if (st) hipStreamSynchronize(st);
        for (const IdxBuildImage *I : live) drop(*I);
        return -1;
    };
    if (st.create(hipStreamNonBlocking) != hipSuccess) return fail("cannot create a stream");
    for (Stream &s : copy_st) if (s.create(hipStreamNonBlocking) != hipSuccess) return fail("cannot create a stream");
    t0 = Clock::now();
    std::vector<SerialJob> jobs(m);
    std::vector<IndexTask> seeds;
    SerialJob *d_jobs = mem.make<SerialJob>(m);
    IndexTask *d_seeds = mem.make<IndexTask>(m);
    IndexCaptureTask *d_caps = mem.make<IndexCaptureTask>(std::max<size_t>(1, plan.entries.size()));
    if (!d_jobs || !d_seeds || !d_caps) return fail("cannot allocate the workspace");
    size_t arena_bytes = 0;                                              // one block for all images: stream, plane, record, [B | F], tables, staged bodies
    for (const IdxBuildImage *I : live)
        arena_bytes += stream_buf_bytes(I->it.len) + up256(I->plane_bytes) + up256(I->L.b) + up256(2 * I->L.b_bytes) + (I->it.kind ? up256(kQTab) : 0) +
                       up256(size_t(I->count) * I->stride);
    uint8_t *arena = mem.make<uint8_t>(arena_bytes);
    if (!arena) return fail("cannot allocate the workspace");
    for (size_t i = 0, at = 0; i < m; i++) {
        IdxBuildImage &I = *live[i];
        const DecodeItem &it = I.it;
        I.d_stream = arena + at; at += stream_buf_bytes(it.len);
        I.d_plane = arena + at; at += up256(I.plane_bytes);
        I.d_rec = arena + at; at += up256(I.L.b);
        if (I.L.b_bytes) { I.d_stats = arena + at; at += up256(2 * I.L.b_bytes); }
        if (it.kind) { I.d_tab = arena + at; at += up256(kQTab); }
        I.d_stage = arena + at; at += up256(size_t(I.count) * I.stride);
        // a body that was never captured must not pass for one: the finish tells by its header
        if (hipMemsetAsync(I.d_stage, 0xFF, size_t(I.count) * I.stride, st) != hipSuccess) return fail("upload");
        if (!upload_stream(I.d_stream, streams[I.k], it.len, st) ||
            (it.kind && hipMemcpyAsync(I.d_tab, I.qtab.data(), kQTab, hipMemcpyHostToDevice, st) != hipSuccess)) return fail("upload");
        jobs[i] = decode_job(it, I.d_plane, 0, I.d_stream, 0, reinterpret_cast<SerialState *>(I.d_rec), reinterpret_cast<double *>(I.d_stats), I.d_tab,
                             plan_in[i].rows, I.every, c->d_redo);
        IndexTask T{};                                                   // segment 0 of an indexed decode: zeros, pos, avail, final_ = 1; zeros in [B | F]
        T.rec = I.d_rec; T.stats = I.d_stats;
        T.avail = it.len; T.first_pos = first_pos(it);
        T.rec_bytes = uint32_t(I.L.b); T.b_bytes = uint32_t(I.L.b_bytes);
        T.kind = uint32_t(it.kind);
        seeds.push_back(T);
    }
    // the capture tasks, in the plan's order; first_chunk counts from the first task of the same launch
    std::vector<IndexCaptureTask> caps;
    struct CaptureRun { size_t first; int n; uint32_t chunks; };
    std::vector<std::vector<CaptureRun>> runs(kBuildClasses);
    for (int cls = 0; cls < kBuildClasses; cls++) runs[size_t(cls)].assign(size_t(plan.launches[cls]), CaptureRun{0, 0, 0u});
    for (const BuildEntry &E : plan.entries) {
        IdxBuildImage &I = *live[size_t(E.image)];
        const int e = E.row / I.every;                                   // 1-based
        IndexCaptureTask T = capture_task(I.it, I.L, E.row, e < I.count ? E.row + I.every : 0, I.d_rec, I.d_stats, I.d_plane, 0,
                                          I.d_stage + size_t(e - 1) * I.stride, d_jobs + E.image);
        CaptureRun &R = runs[size_t(E.cls)][size_t(E.launch)];
        if (R.n == 0) R.first = caps.size();
        T.first_chunk = R.chunks;
        R.n++; R.chunks += index_capture_chunks(T);
        caps.push_back(T);
    }
    uint32_t seed_chunks = 0;
    if (!idxdec_upload_tasks(seeds, true, d_seeds, seed_chunks, st) ||
        hipMemcpyAsync(d_jobs, jobs.data(), m * sizeof(SerialJob), hipMemcpyHostToDevice, st) != hipSuccess ||
        (!caps.empty() && hipMemcpyAsync(d_caps, caps.data(), caps.size() * sizeof(IndexCaptureTask), hipMemcpyHostToDevice, st) != hipSuccess) ||
        !index_seed_launch(d_seeds, int(m), seed_chunks, st)) return fail("upload");
    if (hipStreamSynchronize(st) != hipSuccess) return fail("upload");
    split[1] = ms_since(t0);
    t0 = Clock::now();
    long launches_total = 0;
    for (size_t a = 0; a < m;) {                                         // class by class: decode launch, capture launch, ... -- no wait in between
        size_t b = a + 1;
        const int cls = indexed_class(live[a]->it.kind, live[a]->it.effort);
        while (b < m && indexed_class(live[b]->it.kind, live[b]->it.effort) == cls) b++;
        for (int l = 0; l < plan.launches[cls]; l++) {
            const CaptureRun &R = runs[size_t(cls)][size_t(l)];
            if (!decode_launch(live[a]->it, d_jobs + a, jobs.data() + a, int(b - a), st, true) ||
                !index_capture_launch(d_caps + R.first, R.n, R.chunks, st)) return fail("launch");
        }
        launches_total += plan.launches[cls];
        a = b;
    }
    for (size_t i = 0; i < m; i++)
        if (hipMemcpyAsync(&live[i]->last, live[i]->d_rec, sizeof(SerialState), hipMemcpyDeviceToHost, st) != hipSuccess) return fail("state");
    if (hipStreamSynchronize(st) != hipSuccess) return fail("the launches");
    { std::lock_guard<std::mutex> l(c->stat_m); c->serial_launch_count += launches_total; }
    split[2] = ms_since(t0);
    t0 = Clock::now();
    // the finish, one task per image on the workers (its two copies on one of the call's copy streams, one image at a time per stream)
    std::atomic<bool> device_failed{false};
    pending.add(int(m));
    for (size_t i = 0; i < m; i++)
        pool.post([&, i] {
            IdxBuildImage &I = *live[i];
            const DecodeItem &it = I.it;
            [&] {
                if (I.last.status != kDone) {
                    fprintf(stderr, "[nblic_amd] batch index build: image %d: the stream is damaged or ends too early\n", I.k);
                    return;
                }
                std::vector<uint8_t> stage(size_t(I.count) * I.stride), own_plane;
                uint8_t *plane = planes && planes[I.k] ? planes[I.k] : nullptr;
                if (!plane) { own_plane.resize(I.plane_bytes); plane = own_plane.data(); }
                bool copied;
                {
                    const size_t sid = i % copy_st.size();
                    std::lock_guard<std::mutex> l(copy_m[sid]);
                    hipStream_t cs = copy_st[sid];
                    copied = hipSetDevice(c->device) == hipSuccess &&
                             hipMemcpyAsync(stage.data(), I.d_stage, stage.size(), hipMemcpyDeviceToHost, cs) == hipSuccess &&
                             hipMemcpyAsync(plane, I.d_plane, I.plane_bytes, hipMemcpyDeviceToHost, cs) == hipSuccess &&
                             hipStreamSynchronize(cs) == hipSuccess;
                }
                if (!copied) { device_failed = true; return; }
                uint8_t *out = indexes[I.k];
                IndexHead H = index_head(it, I.every, I.count, it.len);
                sha256_of(streams[I.k], it.len, H.stream_sha);
                Sha256 rows_sha;
                const size_t w = size_t(it.w);
                for (int e = 1; e <= I.count; e++) {
                    const int row = e * I.every;
                    rows_sha.update(plane + size_t(row - I.every) * w, size_t(I.every) * w);
                    const uint8_t *body = stage.data() + size_t(e - 1) * I.stride;
                    SerialState S;
                    memcpy(&S, body, sizeof S);
                    if (S.next_row != row || S.status != kRunning) return;           // (an entry that was not captured: the plan and the device disagree)
                    uint8_t *ck = out + index_entry_at(e - 1, I.entry_bytes), *rec = ck + sizeof(DecodeCheckpoint);
                    memcpy(rec, body, I.L.tab);
                    index_entry_head(ck, it, I.every, row, S, rows_sha);
                    if (it.kind) memcpy(rec + I.L.tab, I.qtab.data(), kQTab);
                    seal(ck, I.entry_bytes);
                }
                index_close(out, &H, I.count, I.entry_bytes);
                I.good = true;
            }();
            pending.done();
        });
    pending.wait();
    if (device_failed) return fail("copies to the host");
    bool every = true;
    for (IdxBuildImage *I : live) {
        if (!I->good) { drop(*I); continue; }
        status[I->k] = 0; ilens[I->k] = long(I->need);
    }
    split[3] = ms_since(t0);
    { std::lock_guard<std::mutex> l(c->stat_m); for (int k = 0; k < 4; k++) c->idxbuild_split[k] = split[k]; }
    for (int k = 0; k < n; k++) every = every && status[k] == 0;
    return every ? 0 : -1;
}

// ---- default context behind the drop-in entry points ---------------------------------------
static nblic_amd_ctx *g_default = nullptr;
static std::mutex g_default_m;

static nblic_amd_ctx *default_ctx() {
    std::lock_guard<std::mutex> g(g_default_m);
    if (!g_default) {
        const char *dev = getenv("NBLIC_AMD_DEVICE");
        g_default = nblic_amd_create(dev ? atoi(dev) : 0, 2, 2);
    }
    return g_default;
}

// ---- what the three cost plans share (colour, slice stacks, deep pixels) ----------------------------------------------------------
// The tasks' places in ONE launch of a cost kernel -- first_chunk, from tiles_of(task) -- the limits, counted() (the launch is
// going to be made: the context's counters), the upload of the task table, and of a second table if the launch has one, and
// launch(d_tasks, n, tiles), all queued on st.  The sums are the caller's to set.
template <class Task, class TilesOf, class Counted, class Launch, class Second = char>
static bool cost_queue(Task *tasks, size_t n, Task *d_tasks, hipStream_t st, TilesOf tiles_of, Counted counted, Launch launch,
                       const Second *second = nullptr, size_t n_second = 0, Second *d_second = nullptr) {
    unsigned long long tiles = 0;
    for (size_t i = 0; i < n; i++) { tasks[i].first_chunk = uint32_t(tiles); tiles += tiles_of(tasks[i]); }
    if (n == 0) return true;
    if (tiles >= (1ull << 31) || n >= (size_t(1) << 30) || n_second >= (size_t(1) << 30)) return false;
    counted();
    return hipMemcpyAsync(d_tasks, tasks, n * sizeof(Task), hipMemcpyHostToDevice, st) == hipSuccess &&
           (!second || hipMemcpyAsync(d_second, second, n_second * sizeof(Second), hipMemcpyHostToDevice, st) == hipSuccess) &&
           launch(d_tasks, int(n), uint32_t(tiles));
}

// A plan's device side: a table of 64-bit sums, set to given values, filled by ONE timed queue step and copied back once.
// It owns the stream, the two events and the device memory -- the sums, and the task tables the plan makes from `mem`
// between begin and run, so that nothing is allocated between the events.
struct SumsRun {
    Stream st;
    Event t0, t1;
    DevPool mem;
    unsigned long long *d_sums = nullptr;
    bool begin(size_t n_sums) {
        d_sums = mem.make<unsigned long long>(n_sums);
        return d_sums && st.create(hipStreamNonBlocking) == hipSuccess && t0.create(hipEventDefault) == hipSuccess && t1.create(hipEventDefault) == hipSuccess;
    }
    // sums: the initial values, then the results.  queue(stream) queues the uploads and the launch; the GPU time it took goes
    // to *ms (guarded by c->stat_m).  false: a HIP call failed.
    template <class Queue> bool run(nblic_amd_ctx *c, std::vector<unsigned long long> &sums, double *ms, Queue queue) {
        const size_t bytes = sums.size() * sizeof(unsigned long long);
        const bool ok = [&]() -> bool {                                  // the launch, then ONE copy of the whole table
            HIP_OK(hipMemcpyAsync(d_sums, sums.data(), bytes, hipMemcpyHostToDevice, st));
            HIP_OK(hipEventRecord(t0, st));
            if (!queue(hipStream_t(st))) return false;
            HIP_OK(hipEventRecord(t1, st));
            HIP_OK(hipMemcpyAsync(sums.data(), d_sums, bytes, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            return true;
        }();
        if (st) hipStreamSynchronize(st);
        if (!ok) return false;
        float t = 0.0f;
        if (hipEventElapsedTime(&t, t0, t1) == hipSuccess) { std::lock_guard<std::mutex> l(c->stat_m); *ms = double(t); }
        return true;
    }
};

// ---- the kernel test bench: what the debug entry points of the pixel-side kernels stage alike --------------------------------------
// INPUTS, each at a byte offset inside a region of its own that is larger and filled with one byte; OUTPUTS, each a region
// filled with one byte that comes back whole in the caller's buffer; optionally a table of GATE records.  An entry point
// registers them, allocates, builds its tasks on the device addresses, and runs: the fills and the uploads, its launch, ONE
// copy back.  The numbers the tests' guards see are here: a SOURCE (the collect side) lies in 0xFF -- NaN in every float
// format, 255 as a pixel -- with 256 more bytes behind it; a PLANE (the deliver side) lies in zeros, may be read for
// up256(bytes) as the decoders' planes allow, and has 16 more bytes behind that; an output is filled with 0x5A.
class DebugBench {
    struct Input { const void *src; size_t bytes, at, offset, region; uint8_t fill; };     // the region: [at, at + region) of d_in_
    struct Output { void *dst; size_t bytes, at; uint8_t fill; };
    Stream st_;
    DevPool mem_;
    std::vector<Input> in_;
    std::vector<Output> out_;
    std::vector<SerialState> gates_;
    size_t in_total_ = 0, out_total_ = 0;
    uint8_t *d_in_ = nullptr, *d_out_ = nullptr;
    SerialState *d_gates_ = nullptr;
    size_t input(const void *src, size_t bytes, size_t offset, uint8_t fill, size_t span) {
        in_.push_back(Input{src, bytes, in_total_, offset, up256(offset + span), fill});
        in_total_ += in_.back().region;
        return in_.size() - 1;
    }
public:
    static constexpr size_t kGuard = 256;                            // in front of and behind a plane that a collect-side kernel writes
    // Each returns the number of what it registered, for in() and out().
    size_t source(const void *src, size_t bytes, size_t offset) { return input(src, bytes, offset, 0xFF, bytes + 256); }
    size_t plane(const void *src, size_t bytes, size_t offset) { return input(src, bytes, offset, 0x00, up256(bytes) + 16); }
    size_t output(void *dst, size_t bytes, uint8_t fill = 0x5A) {
        out_.push_back(Output{dst, bytes, out_total_, fill});
        out_total_ += up256(bytes);
        return out_.size() - 1;
    }
    void gates(const int *status, size_t n) {
        gates_.resize(n);
        for (size_t k = 0; k < n; k++) gates_[k].status = status[k];
    }
    bool alloc(int device) {                                         // false: a HIP call failed
        if (hipSetDevice(device) != hipSuccess) return false;
        d_in_ = mem_.make<uint8_t>(in_total_); d_out_ = mem_.make<uint8_t>(out_total_); d_gates_ = mem_.make<SerialState>(gates_.size());
        return d_in_ && d_out_ && d_gates_ && st_.create(hipStreamNonBlocking) == hipSuccess;
    }
    template <class T> T *table(size_t n) { return mem_.make<T>(n); }                      // null: failed
    uint8_t *in(size_t k) const { return d_in_ + in_[k].at + in_[k].offset; }              // where the first byte of input k lies
    uint8_t *out(size_t k) const { return d_out_ + out_[k].at; }
    SerialState *gate(size_t k) const { return d_gates_ + k; }
    // The fills, the gates and the inputs; launch(stream); every output back in ONE copy and into the callers' buffers.
    // 0, or -2: a HIP call failed.
    template <class Launch> int run(Launch launch) {
        std::vector<uint8_t> back(out_total_);
        const bool ok = [&]() -> bool {
            for (const Input &r : in_) HIP_OK(hipMemsetAsync(d_in_ + r.at, r.fill, r.region, st_));
            for (const Output &r : out_) if (r.bytes) HIP_OK(hipMemsetAsync(d_out_ + r.at, r.fill, up256(r.bytes), st_));
            if (!gates_.empty()) HIP_OK(hipMemcpyAsync(d_gates_, gates_.data(), gates_.size() * sizeof(SerialState), hipMemcpyHostToDevice, st_));
            for (const Input &r : in_) if (r.bytes) HIP_OK(hipMemcpyAsync(d_in_ + r.at + r.offset, r.src, r.bytes, hipMemcpyHostToDevice, st_));
            if (!launch(hipStream_t(st_))) return false;
            if (out_total_) HIP_OK(hipMemcpyAsync(back.data(), d_out_, out_total_, hipMemcpyDeviceToHost, st_));
            HIP_OK(hipStreamSynchronize(st_));
            return true;
        }();
        if (st_) hipStreamSynchronize(st_);
        if (!ok) return -2;
        for (const Output &r : out_) memcpy(r.dst, back.data() + r.at, r.bytes);
        return 0;
    }
};

}  // namespace nblic

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

size_t nblic_amd_range_code(const uint16_t *coded, size_t n, unsigned char *out, size_t cap) {
    return range_code(coded, n, out, cap);
}

int nblic_amd_range_code_multi(const uint16_t *const *coded, const size_t *n, int count, unsigned char *const *outs,
                               const size_t *caps, size_t *lens) {
    if (count < 0) return -1;
    if (have_avx512()) {
        for (int k = 0; k < count; k += 16) range_code_x8(coded + k, n + k, count - k < 16 ? count - k : 16, outs + k, caps + k, lens + k);
        return 1;
    }
    for (int k = 0; k < count; k++) lens[k] = range_code(coded[k], n[k], outs[k], caps[k]);
    return 0;
}

// The coder threads' walk over chunks of packs, minus the GPU: every pack's chunk laid out by pack_groups_host (the
// layout's reference) in a 64-byte aligned buffer of its own and fed through feed_packs.
static int code_packs_host(int n_packs, const int *pack_n, const uint16_t *const *coded, const size_t *n, unsigned char *const *outs,
                           const size_t *caps, size_t *lens, size_t chunk) {
    RangeX8 x[kMaxPacks];
    RangeX8 *packs[kMaxPacks] = {&x[0], &x[1], &x[2]};
    size_t n_max = 0;
    for (int p = 0; p < n_packs; p++) {
        x[p].begin(pack_n[p], outs + kPackLanes * p, caps + kPackLanes * p);
        for (int k = 0; k < pack_n[p]; k++) n_max = std::max(n_max, n[kPackLanes * p + k]);
    }
    const size_t rows_words = group_words(chunk);
    uint64_t *rows[kMaxPacks] = {nullptr};
    for (int p = 0; p < n_packs; p++)
        if (!(rows[p] = static_cast<uint64_t *>(aligned_alloc(64, (rows_words * sizeof(uint64_t) + 63) & ~size_t(63))))) { for (int q = 0; q < p; q++) free(rows[q]); return -1; }
    for (size_t off = 0; off < n_max; off += chunk) {
        size_t len[kMaxTake] = {0};
        for (int p = 0; p < n_packs; p++) {
            memset(rows[p], 0, rows_words * sizeof(uint64_t));
            for (int k = 0; k < pack_n[p]; k++) {
                const size_t at = kPackLanes * p + k;
                len[at] = off >= n[at] ? 0 : std::min(n[at] - off, chunk);
                pack_groups_host(rows[p], k, coded[at] + off, len[at]);
            }
        }
        feed_packs(packs, n_packs, rows, len);
    }
    for (int p = 0; p < n_packs; p++) { free(rows[p]); x[p].end(lens + kPackLanes * p); }
    return 0;
}

int nblic_amd_range_code_chunked(const uint16_t *const *coded, const size_t *n, int count, unsigned char *const *outs,
                                 const size_t *caps, size_t *lens, size_t chunk) {
    if (count < 1 || count > kMaxTake || chunk == 0) return -1;
    if (!(count > 1 && have_avx512())) {                       // one after the other through the scalar coder
        for (int k = 0; k < count; k++) {
            RangeScalar r;
            r.begin(outs[k], caps[k]);
            for (size_t off = 0; off < n[k]; off += chunk) r.feed(coded[k] + off, n[k] - off < chunk ? n[k] - off : chunk);
            lens[k] = r.finish();
        }
        return 0;
    }
    // consecutive eights are packs, as the groups' launches make them; any chunk length goes (every chunk is laid out from its own group 0)
    const int n_packs = (count + int(kPackLanes) - 1) / int(kPackLanes);
    int pack_n[kMaxPacks] = {0};
    for (int p = 0; p < n_packs; p++) pack_n[p] = std::min(int(kPackLanes), count - int(kPackLanes) * p);
    return code_packs_host(n_packs, pack_n, coded, n, outs, caps, lens, chunk);   // stream k is lane k % 8 of pack k / 8: the arrays are already indexed 8 p + lane
}

void nblic_amd_pack_groups_host(uint64_t *rows, int lane, const uint16_t *coded, size_t n) { pack_groups_host(rows, lane, coded, n); }

int nblic_amd_range_code_packs(int n_packs, const int *pack_n, const uint16_t *const *coded, const size_t *n, unsigned char *const *outs,
                               const size_t *caps, size_t *lens, size_t chunk) {
    if (n_packs < 1 || n_packs > kMaxPacks || chunk < kGroupBins || chunk % kGroupBins != 0) return -1;
    for (int p = 0; p < n_packs; p++) if (pack_n[p] < 1 || pack_n[p] > int(kPackLanes)) return -1;
    if (!have_avx512()) {                                      // what the coder threads do on such a host: every image on its own
        for (int p = 0; p < n_packs; p++)
            for (int k = 0; k < pack_n[p]; k++) {
                const size_t at = kPackLanes * size_t(p) + size_t(k);
                RangeScalar r;
                r.begin(outs[at], caps[at]);
                for (size_t off = 0; off < n[at]; off += chunk) r.feed(coded[at] + off, std::min(n[at] - off, chunk));
                lens[at] = r.finish();
            }
        return 1;
    }
    return code_packs_host(n_packs, pack_n, coded, n, outs, caps, lens, chunk);
}

int nblic_amd_selftest(nblic_amd_ctx *c) {
    if (!c || hipSetDevice(c->device) != hipSuccess) return -1;
    return e1_selftest(c->groups[0].stream);
}

void nblic_amd_syn1(unsigned char *img, int h, int w, uint32_t seed) {
    uint32_t xs = seed;
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            xs ^= xs << 13; xs ^= xs >> 17; xs ^= xs << 5;
            int t = ((i + 2 * j) >> 3) & 511;
            int base = iabs(t - 256); if (base > 255) base = 255;
            int v = ((base * 3) >> 2) + 32 + ((i ^ j) & 15) + int(xs & 7) + int((xs >> 3) & 7) - 7;
            img[size_t(i) * size_t(w) + size_t(j)] = uint8_t(iclip(v, 0, 255));
        }
}

const char *nblic_amd_version(void) { return "nblic_amd 0.2 (NBLIC v0.3 bitstream, gfx950)"; }

nblic_amd_ctx *nblic_amd_create_ex(int device, int n_groups, int group_size, int n_coders, int n_host_buffers) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        fprintf(stderr, "[nblic_amd] no HIP device available -- this library has no CPU fallback\n");
        return nullptr;
    }
    if (device < 0 || device >= count || hipSetDevice(device) != hipSuccess) {
        fprintf(stderr, "[nblic_amd] cannot select HIP device %d of %d\n", device, count);
        return nullptr;
    }
    if (n_groups < 1) n_groups = 1;
    if (group_size < 1) group_size = 1;
    if (n_coders < 1) n_coders = 1;
    if (n_host_buffers < n_groups * group_size + kMaxTake) n_host_buffers = n_groups * group_size + kMaxTake;   // groups in flight + one pack filling
    auto *c = new nblic_amd_ctx;
    c->device = device;
    c->simd = have_avx512() && !getenv("NBLIC_AMD_NO_SIMD");
    {   // NBLIC_AMD_COPY_ENGINE=0 leaves every copy with the runtime; so does a process without the HSA runtime's entry points
        const char *ce = getenv("NBLIC_AMD_COPY_ENGINE");
        if (!ce || atoi(ce) != 0) c->engine.open();
    }
    c->groups.resize(size_t(n_groups));
    std::vector<Stream> planned;                                     // empty: every group creates its own
    plan_group_streams(c, n_groups, planned);
    for (int i = 0; i < n_groups; i++) {
        if (!group_init(c->groups[size_t(i)], i, group_size, c, planned.empty() ? nullptr : &planned[size_t(i)])) { nblic_amd_destroy(c); return nullptr; }
        c->free_groups.push_back(i);
    }
    c->cbufs.resize(size_t(n_host_buffers));
    for (int i = 0; i < n_host_buffers; i++) c->free_cbufs.push_back(i);
    // the same backlog counted in packs: n_host_buffers images' worth of bins, a pack per group in flight at the least.
    // An image takes a buffer of ONE of the two pools, and no more images are in flight than before, so the backlog in
    // HBM is what it was: both pools hand out the buffer returned last (push_front on return; the u16 pool used to
    // rotate), and a buffer's memory is allocated at its first use, so neither pool allocates beyond the backlog there is.
    const int n_pack_buffers = std::max(n_groups * ((group_size + int(kPackLanes) - 1) / int(kPackLanes)) + kMaxPacks, n_host_buffers / int(kPackLanes));
    c->pbufs.resize(size_t(n_pack_buffers));
    for (int i = 0; i < n_pack_buffers; i++) c->free_pbufs.push_back(i);
    if (c->dec_stream.create(hipStreamNonBlocking) != hipSuccess || c->d_redo.alloc(2) != hipSuccess || hipMemset(c->d_redo, 0, 2 * sizeof(unsigned long long)) != hipSuccess ||
        c->dec_stream2.create(hipStreamNonBlocking) != hipSuccess) { nblic_amd_destroy(c); return nullptr; }
    // (Measured and rejected: creating the copy streams with the highest stream priority, so that the
    // coder threads' short interleave kernels and copies overtake the encoder's long kernels -- the
    // pipeline drops from 4.9 to 3.1 Gpx/s.)
    if (const char *cb = getenv("NBLIC_AMD_CHUNK_BINS")) {
        const size_t v = size_t(atol(cb));
        if (v >= 4096 && v <= kChunkBins) c->chunk_bins = v & ~(kGroupBins - 1);     // chunks start on a group boundary
    }
    int n_copy = n_coders < kCopyStreams ? n_coders : kCopyStreams;
    if (const char *cs = getenv("NBLIC_AMD_COPY_STREAMS")) { const int v = atoi(cs); if (v >= 1 && v <= 32) n_copy = v; }   // experiments with the copy engines
    c->copy_streams.resize(size_t(n_copy));
    for (auto &cs : c->copy_streams)
        if (cs.create(hipStreamNonBlocking) != hipSuccess) { nblic_amd_destroy(c); return nullptr; }
    c->coders_wanted = n_coders;
    if (const char *mt = getenv("NBLIC_AMD_MAX_TAKE")) { const int v = atoi(mt); if (v >= 2 && v <= kMaxTake) c->max_take = v; }
    for (int i = 0; i < n_coders; i++) c->coders.emplace_back(coder_main, c, i);
    for (int i = 0; i < n_groups; i++) c->drivers.emplace_back(driver_main, c, i);
    c->submitter = std::thread(submitter_main, c);
    return c;
}

nblic_amd_ctx *nblic_amd_create(int device, int n_slots, int n_coders) {
    // images in flight are split into groups that share kernel launches: two groups, so the GPU
    // works on one while the host codes the other
    if (n_slots < 1) n_slots = 1;
    int n_groups = n_slots >= 2 ? 2 : 1;
    return nblic_amd_create_ex(device, n_groups, (n_slots + n_groups - 1) / n_groups, n_coders, 2 * n_slots);
}

void nblic_amd_destroy(nblic_amd_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    { std::lock_guard<std::mutex> l(c->sm); c->stop_submit = true; }
    c->scv.notify_all();
    if (c->submitter.joinable()) c->submitter.join();
    { std::lock_guard<std::mutex> l(c->rm); c->stop = true; }
    c->rcv.notify_all();
    for (auto &t : c->coders) t.join();
    for (auto &t : c->dev_coders) t.join();
    if (c->qdev.joinable()) c->qdev.join();
    { std::lock_guard<std::mutex> l(c->dm); c->stop_drivers = true; }
    c->dcv.notify_all();
    for (auto &t : c->drivers) t.join();
    if (c->feed_pipe[0] >= 0) { close(c->feed_pipe[0]); close(c->feed_pipe[1]); }
    delete c;                                                                // every thread has ended: the members release what they own
}

void nblic_amd_debug_takes(nblic_amd_ctx *c, long takes[25]) {
    static_assert(kMaxTake == 24, "the header says 25 counts");
    std::lock_guard<std::mutex> l(c->stat_m);
    for (int k = 0; k <= kMaxTake; k++) takes[k] = c->takes[k];
}

long nblic_amd_debug_pack_rows(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, const int *heights, const int *widths,
                               unsigned long long *rows, size_t rows_words, unsigned short *const *coded, unsigned int *n_bins) {
    if (!c || n_images < 2 || n_images > int(kPackLanes)) return -1;
    for (int k = 0; k < n_images; k++) if (!size_ok(heights[k], widths[k], c->max_px)) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    const int id = take_group(c);
    Group &grp = c->groups[size_t(id)];
    long words = -1;
    auto run = [&](bool packed) -> bool {                      // the group's two halves as a driver runs them, packing forced or off
        grp.n_jobs = n_images;
        for (int k = 0; k < n_images; k++) { Slot &s = grp.slots[size_t(k)]; s.job = k; s.h = heights[k]; s.w = widths[k]; s.cb = -1; s.near = 0; s.effort = 1; }
        const bool ok = launch_front(c, grp, imgs, false) && launch_back(c, grp, false, false, packed) && hipStreamSynchronize(grp.stream) == hipSuccess;
        grp.tm_pending = false;
        return ok;
    };
    auto give_back = [&] { for (int k = 0; k < n_images; k++) return_coded(c, grp.slots[size_t(k)]); };
    if (int(grp.slots.size()) >= n_images) {
        bool ok = run(true) && grp.slots[0].pack_n == n_images;
        if (ok) {
            size_t max_ev = 0;
            for (int k = 0; k < n_images; k++) max_ev = std::max(max_ev, size_t(grp.slots[size_t(k)].n_ev));
            const size_t w = PackRows::words(max_ev);
            ok = w <= rows_words && hipMemcpy(rows, c->pbufs[size_t(grp.slots[0].cb)].get(), w * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess;
            if (ok) words = long(w);
        }
        give_back();
        ok = ok && run(false);
        for (int k = 0; k < n_images && ok; k++) {
            const Slot &s = grp.slots[size_t(k)];
            ok = s.cb >= 0 && s.n_ev <= n_bins[k] && hipMemcpy(coded[k], c->cbufs[size_t(s.cb)].get(), size_t(s.n_ev) * sizeof(uint16_t), hipMemcpyDeviceToHost) == hipSuccess;
            n_bins[k] = s.n_ev;
        }
        give_back();
        if (!ok) words = -1;
    }
    release_group(c, id);
    return words;
}

int nblic_amd_debug_device_code(nblic_amd_ctx *c, int n_jobs, const unsigned short *const *records, const size_t *record_words,
                                const int *pack_of, const int *lane_of, int n_packs, const unsigned long long *const *pack_rows,
                                const size_t *pack_words, const unsigned int *n_bins, const unsigned int *caps,
                                unsigned char *const *outs, long *lens) {
    constexpr int kMaxJobs = 4096;
    constexpr size_t kMaxBytes = size_t(1) << 30, kGuard = 64, kGroupWords = PackRows::kWordsPerGroup * PackRows::kLanes;
    constexpr uint8_t kPattern = 0xA5;
    if (!c || n_jobs < 1 || n_jobs > kMaxJobs || n_packs < 0 || n_packs > kMaxJobs) return -1;
    if (!records || !record_words || !pack_of || !lane_of || !n_bins || !caps || !outs || !lens) return -1;
    if (n_packs > 0 && (!pack_rows || !pack_words)) return -1;
    auto align = [](size_t v) { return (v + 255) & ~size_t(255); };
    // the input arena: every pack's rows, then every single image's records, each 256-byte aligned
    const size_t nj = size_t(n_jobs);
    std::vector<size_t> pack_at(size_t(n_packs) + 1), in_at(nj), out_at(nj);
    size_t in_bytes = 0, out_bytes = kGuard;                                  // a guard in front of the first output too
    for (int p = 0; p < n_packs; p++) {
        if (!pack_rows[p] || pack_words[p] % kGroupWords != 0 || pack_words[p] > kMaxBytes / 8) return -1;
        pack_at[size_t(p)] = in_bytes;
        in_bytes += align(pack_words[p] * sizeof(uint64_t) + 1);              // (+ 1: an empty pack still has an address of its own)
    }
    for (int k = 0; k < n_jobs; k++) {
        const size_t n = n_bins[k];
        if (records[k]) {
            const size_t need = std::max<size_t>((n + 255) / 256, 1) * 256;   // whole 512-byte windows; an empty stream has one
            if (record_words[k] < need || record_words[k] > kMaxBytes / 2) return -1;
            in_at[size_t(k)] = in_bytes;
            in_bytes += align(record_words[k] * sizeof(uint16_t));
        } else {
            if (pack_of[k] < 0 || pack_of[k] >= n_packs || lane_of[k] < 0 || lane_of[k] >= int(PackRows::kLanes)) return -1;
            if (pack_words[pack_of[k]] < PackRows::words(n)) return -1;
        }
        if (caps[k] > 0 && !outs[k]) return -1;
        out_at[size_t(k)] = out_bytes;
        out_bytes += (size_t(caps[k]) + kGuard + 63) & ~size_t(63);           // the output, then 64..127 bytes of guard
        if (in_bytes > kMaxBytes || out_bytes > kMaxBytes) return -1;
    }
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    Stream st;
    DevBuf<uint8_t> d_in, d_out; DevBuf<RcJob> d_jobs; DevBuf<uint32_t> d_lens;
    Pinned<RcJob> h_jobs; Pinned<uint32_t> h_lens;
    std::vector<uint8_t> h_in(std::max<size_t>(in_bytes, 256), 0), h_out(out_bytes, kPattern);
    for (int p = 0; p < n_packs; p++) memcpy(h_in.data() + pack_at[size_t(p)], pack_rows[p], pack_words[p] * sizeof(uint64_t));
    for (int k = 0; k < n_jobs; k++) if (records[k]) memcpy(h_in.data() + in_at[size_t(k)], records[k], record_words[k] * sizeof(uint16_t));
    bool ok = st.create(hipStreamNonBlocking) == hipSuccess && d_in.alloc(h_in.size()) == hipSuccess && d_out.alloc(out_bytes) == hipSuccess &&
              d_jobs.alloc(size_t(n_jobs)) == hipSuccess && d_lens.alloc(size_t(n_jobs)) == hipSuccess &&
              h_jobs.alloc(size_t(n_jobs)) == hipSuccess && h_lens.alloc(size_t(n_jobs)) == hipSuccess;
    if (ok) {
        for (int k = 0; k < n_jobs; k++) {
            const bool packed = !records[k];
            h_jobs[k] = RcJob{packed ? nullptr : reinterpret_cast<const uint16_t *>(d_in.get() + in_at[size_t(k)]),
                              packed ? reinterpret_cast<const uint64_t *>(d_in.get() + pack_at[size_t(pack_of[k])]) : nullptr, packed ? uint32_t(lane_of[k]) : 0u,
                              d_out.get() + out_at[size_t(k)], d_lens.get() + k, n_bins[k], caps[k]};
            h_lens[k] = 0xFFFFFFFEu;                                          // neither a length nor "did not fit": the kernel must write every one
        }
        ok = hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_out, h_out.data(), out_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_lens, h_lens, size_t(n_jobs) * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_jobs, h_jobs, size_t(n_jobs) * sizeof(RcJob), hipMemcpyHostToDevice, st) == hipSuccess &&
             device_range_code(d_jobs, n_jobs, st) &&
             hipMemcpyAsync(h_lens, d_lens, size_t(n_jobs) * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipMemcpyAsync(h_out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = hipStreamSynchronize(st) == hipSuccess && ok;
    }
    if (!ok) return -2;
    // everything the kernel may not have written still holds the pattern: guards, and an output beyond its reported length
    bool intact = true;
    size_t at = 0;
    auto pattern_to = [&](size_t end) { for (; at < end; at++) intact = intact && h_out[at] == kPattern; };
    for (int k = 0; k < n_jobs; k++) {
        const uint32_t len = h_lens[k];
        if (len != 0xFFFFFFFFu && len > caps[k]) { intact = false; lens[k] = -1; continue; }      // a length beyond cap (or none written)
        pattern_to(out_at[size_t(k)]);
        lens[k] = len == 0xFFFFFFFFu ? -1 : long(len);
        if (len != 0xFFFFFFFFu) { memcpy(outs[k], h_out.data() + at, len); at += len; }
        else at += caps[k];                                                   // did not fit: the kernel wrote what it liked below cap
    }
    pattern_to(out_bytes);
    return intact ? 0 : -3;
}

// ---- the staged pipeline behind S1 on caller-made records (tests/test_chain_kernels.py) --------------------------------
// A carried-in table is accepted when some sequence of records can have left it there.
static bool ctx_table_ok(const int *v, int keys, int extreme) {
    for (int k = 0; k < keys; k++) if (v[k] < -extreme || v[k] > extreme) return false;
    return true;
}
static bool map_table_ok(const int *t) {             // per re-mapper: symbol -> rank, rank -> symbol (inverse permutations of 0..19), hit counts by rank
    for (int key = 0; key < 512; key++) {
        const int *rank_of = t + key * 3 * kMapSyms, *sym_at = rank_of + kMapSyms, *count = sym_at + kMapSyms;
        for (int k = 0; k < kMapSyms; k++) {
            if (rank_of[k] < 0 || rank_of[k] >= kMapSyms || sym_at[rank_of[k]] != k) return false;
            if (count[k] < 0 || count[k] > (1 << 30)) return false;
        }
    }
    return true;
}
static bool cnt_table_ok(const int *t) {
    for (int k = 0; k < 4096; k++) if (!counter_ok(t[2 * k], t[2 * k + 1])) return false;
    return true;
}
constexpr size_t kDebugMaxRecords = size_t(1) << 22;

int nblic_amd_debug_model_stages(nblic_amd_ctx *c, int model, size_t n, const unsigned char *x, const unsigned int *rec1,
                                 const int *ctx_state_in, const int *map_state_in, unsigned short *pxs, unsigned char *z,
                                 unsigned char *cnt, unsigned int *qhist, unsigned int *blk_base, unsigned char *blk_ok,
                                 size_t blk_ok_cap, int *ctx_state_out, int *map_state_out) {
    if (!c || (model != 0 && model != 1) || n < 1 || n > kDebugMaxRecords) return -1;
    const bool q = model == 1;
    const int keys = q ? 3072 : kContexts;
    if (!x || !rec1 || !pxs || !blk_base || !blk_ok || !ctx_state_out) return -1;
    if (q ? (!qhist || map_state_in) : (!z || !cnt || !map_state_out)) return -1;
    if (blk_ok_cap < n / 4096 + size_t(keys)) return -1;                    // every chain has one partial block at the most
    for (size_t t = 0; t < n; t++) {
        const uint32_t r = rec1[t];
        if (q) { if ((r >> 8) >= 3072u) return -1; continue; }              // (the level is the address's high bits: 0..11)
        const Level L = s1_level(r);
        if ((r >> 27) != 0u || ((r >> 25) & 3u) == 3u || L.qw > kWeightOne / 2 || L.qv < 0 || L.qv >= kLevels) return -1;
    }
    if (ctx_state_in && !ctx_table_ok(ctx_state_in, keys, q ? (1 << 20) : 32576)) return -1;
    if (map_state_in && !map_table_ok(map_state_in)) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    const int id = take_group(c);
    Group &grp = c->groups[size_t(id)];
    Slot &s = grp.slots[0];
    const bool ok = [&]() -> bool {
        grp.n_jobs = 1; s.job = 0; s.h = 1; s.w = int(n); s.near = 0; s.effort = q ? 0 : 1; s.n_ev = 0;
        if (!ensure_pixels(s, n, false)) return false;
        HIP_OK(s.d_img.reserve(n));
        s.b.img = s.d_img;
        grp.h_jobs[0] = e1_job_front(s.b, 1, int(n), 0, q ? 0 : dbg_flags(), long_chains_of(c));
        hipStream_t st = grp.stream;
        HIP_OK(hipMemcpyAsync(s.d_img, x, n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s.b.rec1, rec1, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(grp.d_jobs, grp.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, st));
        // a table that is not given is k_init_state's; a given one goes in behind it, or instead of it
        if (!ctx_state_in || (!q && !map_state_in)) e1_launch_init(grp.d_jobs, 1, st);
        else if (q) HIP_OK(hipMemsetAsync(s.b.qhist, 0, 12 * 256 * sizeof(uint32_t), st));
        if (ctx_state_in) HIP_OK(hipMemcpyAsync(s.b.ctx_state, ctx_state_in, size_t(keys) * sizeof(int), hipMemcpyHostToDevice, st));
        if (map_state_in) HIP_OK(hipMemcpyAsync(s.b.map_state, map_state_in, size_t(512) * 60 * sizeof(int), hipMemcpyHostToDevice, st));
        if (q) q_launch_model_stages(grp.d_jobs, grp.h_jobs, 1, st); else e1_launch_model_stages(grp.d_jobs, grp.h_jobs, 1, st);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(pxs, s.b.pxs, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(blk_base, s.b.blk_base, size_t(keys + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(ctx_state_out, s.b.ctx_state, size_t(keys) * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(grp.h_totals, grp.d_totals, kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (q) {
            HIP_OK(hipMemcpyAsync(qhist, s.b.qhist, 12 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        } else {
            HIP_OK(hipMemcpyAsync(z, s.b.z, n, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(cnt, s.b.cnt, n, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(map_state_out, s.b.map_state, size_t(512) * 60 * sizeof(int), hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipStreamSynchronize(st));
        count_long_chains(c, grp.h_totals);
        const size_t blocks = blk_base[keys];
        if (blocks > blk_ok_cap) return false;
        HIP_OK(hipMemcpy(blk_ok, s.b.blk_ok, blocks, hipMemcpyDeviceToHost));
        return true;
    }();
    grp.tm_pending = false;
    release_group(c, id);
    return ok ? 0 : -2;
}

int nblic_amd_debug_back_half(nblic_amd_ctx *c, size_t n_ev, const unsigned int *events, const int *cnt_state_in,
                              unsigned short *coded, int *cnt_state_out, unsigned int *totals) {
    if (!c || n_ev < 1 || n_ev > kDebugMaxRecords || !events || !coded || !cnt_state_out || !totals) return -1;
    for (size_t r = 0; r < n_ev; r++) {
        const uint32_t e = events[r];
        const int d = ev_qu(e) - ev_qv(e);
        if ((e >> 22) != 0u || d < -1 || d > 1 || ev_qw(e) > kWeightOne / 2) return -1;
    }
    if (cnt_state_in && !cnt_table_ok(cnt_state_in)) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    const int id = take_group(c);
    Group &grp = c->groups[size_t(id)];
    Slot &s = grp.slots[0];
    DevBuf<uint16_t> d_coded;                                               // (a production image's comes from the context's pool and goes to a coder thread)
    const bool ok = [&]() -> bool {
        grp.n_jobs = 1; s.job = 0; s.h = 0; s.w = 0; s.near = 0; s.effort = 1; s.n_ev = uint32_t(n_ev);
        if (!ensure_events(s, n_ev)) return false;
        HIP_OK(d_coded.alloc(n_ev));
        E1Job J = e1_job_front(s.b, 0, 0, 0, dbg_flags(), long_chains_of(c));
        E1Buffers b = s.b;
        b.coded = d_coded;
        e1_job_back(J, b, uint32_t(n_ev));
        grp.h_jobs[0] = J;
        hipStream_t st = grp.stream;
        HIP_OK(hipMemcpyAsync(s.b.events, events, n_ev * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(grp.d_jobs, grp.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(s.b.totals, 0, kTotalsSlot * sizeof(uint32_t), st));
        if (cnt_state_in) HIP_OK(hipMemcpyAsync(s.b.cnt_state, cnt_state_in, size_t(4096) * 2 * sizeof(int), hipMemcpyHostToDevice, st));
        else e1_launch_init(grp.d_jobs, 1, st);
        e1_launch_back_stages(grp.d_jobs, grp.h_jobs, 1, st);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(coded, d_coded, n_ev * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(cnt_state_out, s.b.cnt_state, size_t(4096) * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(totals, s.b.totals, kTotalsStride * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }();
    s.n_ev = 0;
    grp.tm_pending = false;
    release_group(c, id);
    return ok ? 0 : -2;
}

// ---- the entropy front of the serial modes on caller-made records (tests/test_entropy_front.py) -----------------------
// What stream_run does for a serial-mode band between k_serial_model and the host coder, once, on arrays the caller owns.
int nblic_amd_debug_entropy_front(nblic_amd_ctx *c, size_t n, const unsigned char *x, const unsigned int *rec1, const unsigned short *pxs,
                                  int near, const int *map_state_in, const int *cnt_state_in, unsigned char *z, unsigned char *cnt,
                                  unsigned int *pos3, unsigned int *ev_off, unsigned int *events, size_t events_cap,
                                  unsigned short *coded, int *map_state_out, int *cnt_state_out, unsigned int *totals) {
    if (!c || n < 1 || n > kDebugMaxRecords || near < 0 || near > kMaxNear) return -1;
    if (!x || !rec1 || !pxs || !z || !cnt || !pos3 || !ev_off || !events || !coded || !map_state_out || !cnt_state_out || !totals) return -1;
    for (size_t t = 0; t < n; t++) {
        const uint32_t r = rec1[t];
        const Level L = s1_level(r);
        if ((r >> 27) != 0u || ((r >> 25) & 3u) == 3u || L.qw > kWeightOne / 2 || L.qv < 0 || L.qv >= kLevels) return -1;
        if (pxs[t] >= 512u) return -1;                                      // px | sign << 8: the re-mapper's key is 2 px + sign
    }
    if (map_state_in && !map_table_ok(map_state_in)) return -1;
    if (cnt_state_in && !cnt_table_ok(cnt_state_in)) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    const int id = take_group(c);
    Group &grp = c->groups[size_t(id)];
    Slot &s = grp.slots[0];
    DevBuf<uint16_t> d_coded;
    int rc = 0;
    const bool ok = [&]() -> bool {
        grp.n_jobs = 1; s.job = 0; s.h = 1; s.w = int(n); s.near = near; s.effort = 1; s.n_ev = 0;
        if (!ensure_pixels(s, n, false)) return false;
        HIP_OK(s.d_img.reserve(n));
        s.b.img = s.d_img;
        grp.h_jobs[0] = e1_job_front(s.b, 1, int(n), near, 0, long_chains_of(c));              // the one place that pairs k_step and ktab with near
        hipStream_t st = grp.stream;
        HIP_OK(hipMemcpyAsync(s.d_img, x, n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s.b.rec1, rec1, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s.b.pxs, pxs, n * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(grp.d_jobs, grp.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(s.b.totals, 0, kTotalsSlot * sizeof(uint32_t), st));
        // a table that is not given is k_init_state's; a given one goes in behind it, or instead of it
        if (!map_state_in || !cnt_state_in) e1_launch_init(grp.d_jobs, 1, st);
        if (map_state_in) HIP_OK(hipMemcpyAsync(s.b.map_state, map_state_in, size_t(512) * 60 * sizeof(int), hipMemcpyHostToDevice, st));
        if (cnt_state_in) HIP_OK(hipMemcpyAsync(s.b.cnt_state, cnt_state_in, size_t(4096) * 2 * sizeof(int), hipMemcpyHostToDevice, st));
        e1_launch_front_pre(grp.d_jobs, grp.h_jobs, 1, st);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(grp.h_totals, grp.d_totals, kTotalsSlot * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const uint32_t n_ev = grp.h_totals[2];
        count_long_chains(c, grp.h_totals);
        totals[2] = n_ev;
        if (size_t(n_ev) > events_cap) { rc = -3; return true; }
        if (n_ev >= 0x7FFFFFFFu || !ensure_events(s, n_ev)) return false;
        HIP_OK(d_coded.alloc(size_t(n_ev) + 8));
        E1Buffers b = s.b;
        b.coded = d_coded;
        e1_job_back(grp.h_jobs[0], b, n_ev);
        HIP_OK(hipMemcpyAsync(grp.d_jobs, grp.h_jobs, sizeof(E1Job), hipMemcpyHostToDevice, st));
        e1_launch_back(grp.d_jobs, grp.h_jobs, 1, st, nullptr, true);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(z, s.b.z, n, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(cnt, s.b.cnt, n, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(pos3, s.b.pos3, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(ev_off, s.b.ev_off, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (n_ev) {
            HIP_OK(hipMemcpyAsync(events, s.b.events, size_t(n_ev) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(coded, d_coded, size_t(n_ev) * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipMemcpyAsync(map_state_out, s.b.map_state, size_t(512) * 60 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(cnt_state_out, s.b.cnt_state, size_t(4096) * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(totals, s.b.totals, kTotalsStride * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }();
    s.n_ev = 0; s.near = 0;
    grp.tm_pending = false;
    release_group(c, id);
    return ok ? rc : -2;
}

// ---- k_index_seed and k_index_chain on caller-made bytes (tests/test_indexed_batch_decode.py) ----------------------------
// The index goes up at byte `base_offset` of a larger buffer, so the tests choose the residue of every entry's address.
int nblic_amd_debug_index_kernels(nblic_amd_ctx *c, const void *index, size_t index_bytes, size_t base_offset, int entry, unsigned long long avail,
                                  unsigned long long first_pos, unsigned char *rec_out, unsigned char *stats_out, unsigned char *rows_out,
                                  const unsigned char *final_rec, size_t final_rec_bytes, const unsigned char *final_b, size_t final_b_bytes,
                                  const unsigned char *final_rows, size_t final_rows_bytes, unsigned int *verdict) {
    IndexView V;
    if (!c || !index || !rec_out || !stats_out || !rows_out || base_offset > 4096 || index_check(index, index_bytes, nullptr, 0, c->max_px, V) != 0 || V.packed) return -1;
    if (entry < 0 || entry > V.H.count) return -1;
    const bool chain = final_rec || final_b || final_rows || verdict;
    const RecordLayout &L = V.L;
    const size_t w = size_t(V.H.w);
    const RowsAbove A = rows_above(entry * V.H.every_rows, V.H.w);
    const size_t rows_bytes = size_t(A.n) * w;
    if (chain && (entry < 1 || !final_rec || !verdict || (L.b_bytes && !final_b) || (rows_bytes && !final_rows) || final_rec_bytes < L.b ||
                  final_b_bytes < L.b_bytes || final_rows_bytes < rows_bytes)) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    constexpr size_t kGuard = 256;
    constexpr uint8_t kPattern = 0xA7;
    Stream st;
    DevPool mem;
    const size_t rec_b = up256(L.b), stats_b = up256(2 * L.b_bytes), plane_b = up256(2 * w), word_b = 256;
    const size_t out_bytes = rec_b + stats_b + plane_b + word_b + 4 * kGuard;
    uint8_t *d_index = mem.make<uint8_t>(up256(base_offset + index_bytes + 16));
    uint8_t *d_out = mem.make<uint8_t>(out_bytes);
    IndexTask *d_task = mem.make<IndexTask>(1);
    if (!d_index || !d_out || !d_task || st.create(hipStreamNonBlocking) != hipSuccess) return -2;
    uint8_t *d_rec = d_out, *d_stats = d_rec + rec_b + kGuard, *d_plane = d_stats + stats_b + kGuard, *d_word = d_plane + plane_b + kGuard;
    const size_t used[4] = {L.b, 2 * L.b_bytes, 2 * w, chain ? sizeof(uint32_t) : 0};
    uint8_t *const parts[4] = {d_rec, d_stats, d_plane, d_word};
    const size_t room[4] = {rec_b + kGuard, stats_b + kGuard, plane_b + kGuard, word_b + kGuard};
    std::vector<uint8_t> back(out_bytes);
    const bool ok = [&]() -> bool {
        HIP_OK(hipMemsetAsync(d_index, 0, up256(base_offset + index_bytes + 16), st));
        HIP_OK(hipMemcpyAsync(d_index + base_offset, index, index_bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(d_out, kPattern, out_bytes, st));
        IndexTask T{};
        T.entry = entry > 0 ? d_index + base_offset + size_t(V.body(entry) - static_cast<const uint8_t *>(index)) : nullptr;
        T.rec = d_rec; T.stats = L.b_bytes ? d_stats : nullptr;
        T.rows = d_plane + A.at;                                         // the plane here is the 2 w bytes of rows [r - 2, r)
        T.avail = avail; T.first_pos = first_pos;
        T.rec_bytes = uint32_t(L.b); T.b_bytes = uint32_t(L.b_bytes); T.rows_bytes = entry > 0 ? uint32_t(rows_bytes) : 0u;
        T.b_at = uint32_t(L.b); T.rows_at = uint32_t(L.rows + A.at);
        T.kind = uint32_t(V.H.kind);
        T.verdict = reinterpret_cast<uint32_t *>(d_word);
        if (chain) {
            HIP_OK(hipMemcpyAsync(d_rec, final_rec, L.b, hipMemcpyHostToDevice, st));
            if (L.b_bytes) HIP_OK(hipMemcpyAsync(d_stats, final_b, L.b_bytes, hipMemcpyHostToDevice, st));
            if (rows_bytes) HIP_OK(hipMemcpyAsync(d_plane + A.at, final_rows, rows_bytes, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemsetAsync(d_word, 0, sizeof(uint32_t), st));
        }
        HIP_OK(hipMemcpyAsync(d_task, &T, sizeof T, hipMemcpyHostToDevice, st));
        if (!(chain ? index_chain_launch(d_task, 1, index_task_chunks(T, false), st) : index_seed_launch(d_task, 1, index_task_chunks(T, true), st))) return false;
        HIP_OK(hipMemcpyAsync(back.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }();
    if (st) hipStreamSynchronize(st);
    if (!ok) return -2;
    for (int k = 0; k < 4; k++) {                                        // everything behind what a part may hold is still the pattern
        const size_t at = size_t(parts[k] - d_out);
        for (size_t i = used[k]; i < room[k]; i++)
            if (back[at + i] != kPattern) return -3;
    }
    if (chain) {
        memcpy(verdict, back.data() + (d_word - d_out), sizeof(uint32_t));
        return 0;
    }
    memcpy(rec_out, back.data(), L.b);
    memcpy(stats_out, back.data() + (d_stats - d_out), 2 * L.b_bytes);
    memcpy(rows_out, back.data() + (d_plane - d_out), 2 * w);
    return 0;
}

// ---- k_index_capture on caller-made bytes (tests/test_index_build_batch.py) ------------------------------------------------
// ONE launch, one task: the record, B and the rows above `row` go up verbatim (the rows at byte plane_offset of a zeroed
// buffer, so the tests choose the residue of the plane's address) and the staged body comes back.
int nblic_amd_debug_index_capture(nblic_amd_ctx *c, int kind, int effort, int width, int row, int next_end, const unsigned char *record, size_t record_bytes,
                                  const unsigned char *b, size_t b_bytes, const unsigned char *rows, size_t rows_bytes, size_t plane_offset,
                                  unsigned char *body_out, size_t body_cap, int *end_row_out) {
    if (!c || !record || !rows || !body_out || !end_row_out || index_record_bytes(kind, width, effort) == 0 || width < 1 || width > kIndexMaxSide ||
        row < 1 || row > kIndexMaxSide || next_end < 0 || plane_offset > 4096) return -1;
    const DecodeItem it{0, kIndexMaxSide, width, 0, kMinKStep, effort, kind, 0, -1, -1};
    const RecordLayout L = record_layout(kind, width, effort);
    const RowsAbove A = rows_above(row, width);
    if (record_bytes != L.b || b_bytes != L.b_bytes || (b_bytes && !b) || rows_bytes != size_t(A.n) * size_t(width) || body_cap < L.tab) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    constexpr size_t kGuard = 256;
    constexpr uint8_t kPattern = 0xA7;
    const size_t used = build_stage_stride(L), out_bytes = used + kGuard, plane_bytes = up256(plane_offset + rows_bytes + 16);
    Stream st;
    DevPool mem;
    uint8_t *d_rec = mem.make<uint8_t>(up256(L.b)), *d_stats = mem.make<uint8_t>(up256(2 * L.b_bytes)), *d_plane = mem.make<uint8_t>(plane_bytes);
    uint8_t *d_out = mem.make<uint8_t>(out_bytes);
    SerialJob *d_job = mem.make<SerialJob>(1);
    IndexCaptureTask *d_task = mem.make<IndexCaptureTask>(1);
    if (!d_rec || !d_stats || !d_plane || !d_out || !d_job || !d_task || st.create(hipStreamNonBlocking) != hipSuccess) return -2;
    std::vector<uint8_t> back(out_bytes);
    SerialJob J{};
    J.end_row = row;
    bool acted = false;
    const bool ok = [&]() -> bool {
        HIP_OK(hipMemcpyAsync(d_rec, record, L.b, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(d_stats, 0, up256(2 * L.b_bytes), st));
        if (L.b_bytes) HIP_OK(hipMemcpyAsync(d_stats, b, L.b_bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(d_plane, 0, plane_bytes, st));
        HIP_OK(hipMemcpyAsync(d_plane + plane_offset, rows, rows_bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(d_out, kPattern, out_bytes, st));
        HIP_OK(hipMemcpyAsync(d_job, &J, sizeof J, hipMemcpyHostToDevice, st));
        // the plane here holds rows [row - n, row) alone, from plane_offset on
        IndexCaptureTask T = capture_task(it, L, row, next_end, d_rec, d_stats, d_plane + plane_offset, A.first, d_out, d_job);
        HIP_OK(hipMemcpyAsync(d_task, &T, sizeof T, hipMemcpyHostToDevice, st));
        if (!index_capture_launch(d_task, 1, index_capture_chunks(T), st)) return false;
        HIP_OK(hipMemcpyAsync(back.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&J, d_job, sizeof J, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }();
    if (st) hipStreamSynchronize(st);
    if (!ok) return -2;
    SerialState S;
    memcpy(&S, record, sizeof S);
    acted = S.status == kRunning && S.next_row == row;
    for (size_t i = acted ? used : 0; i < out_bytes; i++)
        if (back[i] != kPattern) return -3;
    for (size_t i = L.tab; acted && i < used; i++)                        // the last unit is filled up with zeros
        if (back[i] != 0) return -3;
    memcpy(body_out, back.data(), L.tab);
    *end_row_out = J.end_row;
    return 0;
}

// ---- k_index_unpack_scan, k_index_unpack and k_index_unpack_rank on caller-made bytes (tests/test_index_unpack_kernels.py) --
// ONE scan launch and ONE unpack launch (the rank kernel with it) over n packed indexes as n tasks, made by idxdec_unpack_task
// and placed as decode_batch_indexed places them.  What is accepted is what the kernels' memory safety rests on -- packed_walk,
// which has read every length, flag and width byte, and a sound head -- and NOT the table checks of packed_index_check: the
// tests feed the kernels values those refuse.
int nblic_amd_debug_index_unpack(nblic_amd_ctx *c, int n, const void *const *packed, const size_t *packed_bytes, const size_t *base_offsets,
                                 const int *walks, const int *first_outs, unsigned char *const *outs, const size_t *caps, size_t *out_strides) {
    constexpr int kMaxTasks = 8;
    constexpr size_t kGuard = 256;
    constexpr uint8_t kPattern = 0xA7;
    if (!c || n < 1 || n > kMaxTasks || !packed || !packed_bytes || !base_offsets || !walks || !first_outs || !outs || !caps || !out_strides) return -1;
    const size_t count = size_t(n);
    std::vector<IndexView> views(count);
    std::vector<IndexUnpackTask> made(count);
    std::vector<std::vector<unsigned long long>> descs(count);
    std::vector<size_t> used(count), out_at(count), index_at(count), desc_at(count), offs_at(count);
    size_t out_bytes = 0, index_bytes = 0, desc_words = 0, offs_words = 0;
    for (int k = 0; k < n; k++) {
        IndexView &V = views[size_t(k)];
        if (!packed[k] || !outs[k] || base_offsets[k] > 4096 || !packed_walk(packed[k], packed_bytes[k], V.P)) return -1;
        memcpy(&V.H, packed[k], sizeof V.H);
        if (!index_head_ok(V.H, c->max_px)) return -1;
        V.packed = true;
        V.L = record_layout(V.H.kind, V.H.w, V.H.effort);
        if (V.P.body_bytes != V.L.bytes || walks[k] < 1 || walks[k] > V.H.count || first_outs[k] < 0 || first_outs[k] >= walks[k]) return -1;
        idxdec_unpack_task(V, walks[k], made[size_t(k)], descs[size_t(k)]);
        used[size_t(k)] = size_t(walks[k] - first_outs[k]) * made[size_t(k)].out_stride;
        if (caps[k] < used[size_t(k)] + kGuard) return -1;
        out_at[size_t(k)] = out_bytes; out_bytes += up256(used[size_t(k)]) + kGuard;
        index_at[size_t(k)] = index_bytes; index_bytes += up256(base_offsets[k] + packed_bytes[k] + 16);      // (the kernels read whole aligned words)
        desc_at[size_t(k)] = desc_words; desc_words += descs[size_t(k)].size();
        offs_at[size_t(k)] = offs_words; offs_words += size_t(walks[k]) * made[size_t(k)].blocks;
    }
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    Stream st;
    DevPool mem;
    uint8_t *d_index = mem.make<uint8_t>(index_bytes), *d_out = mem.make<uint8_t>(out_bytes);
    unsigned long long *d_desc = mem.make<unsigned long long>(desc_words);
    uint32_t *d_offs = mem.make<uint32_t>(offs_words);
    IndexUnpackTask *d_tasks = mem.make<IndexUnpackTask>(size_t(n));
    if (!d_index || !d_out || !d_desc || !d_offs || !d_tasks || st.create(hipStreamNonBlocking) != hipSuccess) return -2;
    std::vector<uint8_t> back(out_bytes);
    const bool ok = [&]() -> bool {
        HIP_OK(hipMemsetAsync(d_index, 0, index_bytes, st));
        HIP_OK(hipMemsetAsync(d_offs, 0, offs_words * sizeof(uint32_t), st));
        HIP_OK(hipMemsetAsync(d_out, kPattern, out_bytes, st));
        std::vector<IndexUnpackTask> scans, rounds;
        uint32_t scan_waves = 0, waves = 0, groups = 0;
        for (int k = 0; k < n; k++) {
            const size_t i = size_t(k);
            IndexUnpackTask &T = made[i];
            T.packed = d_index + index_at[i] + base_offsets[k]; T.desc = d_desc + desc_at[i]; T.offs = d_offs + offs_at[i];
            HIP_OK(hipMemcpyAsync(d_index + index_at[i] + base_offsets[k], packed[k], packed_bytes[k], hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(d_desc + desc_at[i], descs[i].data(), descs[i].size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
            idxdec_place_scan(T, scan_waves, scans);
            idxdec_place_round(T, d_out + out_at[i], walks[k], first_outs[k], waves, groups, rounds);
        }
        HIP_OK(hipMemcpyAsync(d_tasks, scans.data(), scans.size() * sizeof(IndexUnpackTask), hipMemcpyHostToDevice, st));
        if (!index_unpack_scan_launch(d_tasks, n, scan_waves, st)) return false;
        HIP_OK(hipStreamSynchronize(st));                                // (the task array is reused)
        HIP_OK(hipMemcpyAsync(d_tasks, rounds.data(), rounds.size() * sizeof(IndexUnpackTask), hipMemcpyHostToDevice, st));
        if (!index_unpack_launch(d_tasks, n, waves, groups, st)) return false;
        HIP_OK(hipMemcpyAsync(back.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }();
    if (st) hipStreamSynchronize(st);
    if (!ok) return -2;
    for (int k = 0; k < n; k++) {                                        // everything behind the stored entries is still the pattern
        const size_t i = size_t(k), room = up256(used[i]) + kGuard;
        for (size_t at = used[i]; at < room; at++)
            if (back[out_at[i] + at] != kPattern) return -3;
    }
    for (int k = 0; k < n; k++) {
        memcpy(outs[k], back.data() + out_at[size_t(k)], used[size_t(k)] + kGuard);
        out_strides[k] = made[size_t(k)].out_stride;
    }
    return 0;
}

// ---- k_deliver on caller-made planes (tests/test_decode_to_device.py), and its host walk (tests/test_deliver_host.py) -------
// (step 0 stands for the element size: the hooks without a step)
static bool debug_deliver_task(DeliverTask &T, int plane_rows, int width, const int *window, int format, float scale, float bias, int zero, size_t pitch, size_t step) {
    if (plane_rows < 1 || width < 1 || !window || !deliver_args_ok(format, scale, bias) || step > kDeliverMaxStep) return false;
    T = DeliverTask{};
    T.src_pitch = uint32_t(width);
    T.row0 = window[0]; T.row1 = window[1]; T.col0 = window[2]; T.col1 = window[3];
    T.format = uint32_t(format); T.scale = scale; T.bias = bias; T.zero = zero ? 1u : 0u;
    T.dst_pitch = pitch; T.dst_step = step ? uint32_t(step) : deliver_elem(T.format);
    return pitch <= (size_t(1) << 40);
}

// The reference of a debug task: the plane at `ref` has ref_rows rows of the task's width; the task names it from its
// window's first row on.  false: it does not reach that row.
static bool debug_deliver_ref(DeliverTask &T, const uint8_t *ref, int ref_rows, size_t readable) {
    if (ref_rows <= T.row0 || size_t(T.row0) * T.src_pitch > readable) return false;
    T.ref = ref + size_t(T.row0) * T.src_pitch; T.ref_pitch = T.src_pitch; T.ref_bytes = readable - size_t(T.row0) * T.src_pitch;
    return true;
}

// (ref: the reference plane of the _ref hook, ref_rows x width bytes; three gate statuses with it, one without)
static int debug_deliver_host(const unsigned char *plane, int plane_rows, int width, const int *window, int format, float scale, float bias, int zero,
                              int gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset, size_t pitch_bytes, size_t step_bytes,
                              unsigned long long *units, unsigned long long *chunks, const unsigned char *ref = nullptr, int ref_rows = 0,
                              int gate2_status = -1, int gate3_status = -1) {
    DeliverTask T;
    if (!plane || !out || !debug_deliver_task(T, plane_rows, width, window, format, scale, bias, zero, pitch_bytes, step_bytes)) return -1;
    T.src = plane; T.src_bytes = size_t(plane_rows) * size_t(width);
    T.dst = out + dst_offset;
    if (ref && (ref_rows < 1 || !debug_deliver_ref(T, ref, ref_rows, size_t(ref_rows) * size_t(width)))) return -1;
    if (dst_offset > out_bytes || !deliver_task_ok(T, uint32_t(plane_rows))) return -1;
    if (deliver_extent(uint32_t(T.row1 - T.row0), uint32_t(T.col1 - T.col0), T.format, pitch_bytes, T.dst_step) > out_bytes - dst_offset) return -1;
    if (units) *units = deliver_task_units(T);
    if (chunks) *chunks = deliver_task_chunks(T);
    deliver_host(T, gate_status == -1 ? int(kDone) : gate_status, gate2_status == -1 ? int(kDone) : gate2_status, gate3_status == -1 ? int(kDone) : gate3_status);
    return 0;
}
// (refs: the reference planes of the _ref hook, ref_rows[k] x widths[k] bytes each; three gate statuses per task with them, one without)
static int debug_deliver(nblic_amd_ctx *c, int n, const unsigned char *const *planes, const size_t *plane_bytes, const size_t *base_offsets,
                         const int *plane_rows, const int *widths, const int *windows, const int *formats, const float *scales, const float *biases,
                         const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets, const size_t *out_bytes, unsigned char *const *outs,
                         const int *gate_status, const unsigned char *const *refs = nullptr, const size_t *ref_base_offsets = nullptr, const int *ref_rows = nullptr) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !planes || !plane_bytes || !base_offsets || !plane_rows || !widths || !windows || !formats || !scales || !biases ||
        !zeros || !pitches || !dst_offsets || !out_bytes || !outs || !gate_status) return -1;
    const size_t count = size_t(n);
    std::vector<DeliverTask> tasks(count);
    std::vector<size_t> plane_in(count), ref_in(count, 0);
    const size_t n_gates = refs ? 3 : 1;                                 // statuses, and records on the device, per task
    DebugBench bench;
    for (int k = 0; k < n; k++) {
        const size_t i = size_t(k);
        DeliverTask &T = tasks[i];
        if (!planes[k] || !outs[k] || base_offsets[k] > 15 || !debug_deliver_task(T, plane_rows[k], widths[k], windows + 4 * i, formats[k], scales[k], biases[k], zeros[k], pitches[k], steps ? steps[k] : 0))
            return -1;
        if (plane_bytes[k] != size_t(plane_rows[k]) * size_t(widths[k]) || plane_bytes[k] > (size_t(1) << 30) || out_bytes[k] > (size_t(1) << 30) || dst_offsets[k] > out_bytes[k]) return -1;
        T.src_bytes = up256(plane_bytes[k]);
        plane_in[i] = bench.plane(planes[k], plane_bytes[k], base_offsets[k]);
        if (refs && refs[k]) {
            if (ref_base_offsets[k] > 15 || ref_rows[k] < 1 || size_t(ref_rows[k]) * size_t(widths[k]) > (size_t(1) << 30)) return -1;
            ref_in[i] = bench.plane(refs[k], size_t(ref_rows[k]) * size_t(widths[k]), ref_base_offsets[k]);
        }
        bench.output(outs[k], out_bytes[k]);
    }
    bench.gates(gate_status, count * n_gates);
    DeliverTask *d_tasks = bench.alloc(c->device) ? bench.table<DeliverTask>(count) : nullptr;
    if (!d_tasks) return -2;
    for (int k = 0; k < n; k++) {                                        // the addresses are known now: the rest of the checks
        const size_t i = size_t(k);
        DeliverTask &T = tasks[i];
        T.src = bench.in(plane_in[i]);
        T.dst = bench.out(i) + dst_offsets[k];
        if (gate_status[n_gates * i] != -1) T.gate = bench.gate(n_gates * i);
        if (refs) {
            if (gate_status[3 * i + 1] != -1) T.gate2 = bench.gate(3 * i + 1);
            if (gate_status[3 * i + 2] != -1) T.gate3 = bench.gate(3 * i + 2);
            if (refs[k] && !debug_deliver_ref(T, bench.in(ref_in[i]), ref_rows[k], up256(size_t(ref_rows[k]) * size_t(widths[k])))) return -1;
        }
        if (!deliver_task_ok(T, uint32_t(plane_rows[k])) || (T.ref && uint32_t(ref_rows[k]) < uint32_t(T.row1)) ||
            deliver_extent(uint32_t(T.row1 - T.row0), uint32_t(T.col1 - T.col0), T.format, T.dst_pitch, T.dst_step) > out_bytes[k] - dst_offsets[k]) return -1;
    }
    return bench.run([&](hipStream_t st) { deliver_stats_reset(c); return deliver_queue(tasks.data(), count, d_tasks, st, c); });
}

// Host only: the shared unit walk (deliver.h deliver_host) over the caller's plane of plane_rows x width into out + dst_offset,
// one unit after the other.  The unit grid follows the destination's address as the kernel's does, so a caller that wants
// the grid of a device buffer hands in `out` at the same residue of 16.  units / chunks: what a launch would count for the task.
int nblic_amd_debug_deliver_host(const unsigned char *plane, int plane_rows, int width, const int *window, int format, float scale, float bias, int zero,
                                 int gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset, size_t pitch_bytes,
                                 unsigned long long *units, unsigned long long *chunks) {
    return debug_deliver_host(plane, plane_rows, width, window, format, scale, bias, zero, gate_status, out, out_bytes, dst_offset, pitch_bytes, 0, units, chunks);
}
int nblic_amd_debug_deliver_host_ex(const unsigned char *plane, int plane_rows, int width, const int *window, int format, float scale, float bias, int zero,
                                    int gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset, size_t pitch_bytes, size_t step_bytes,
                                    unsigned long long *units, unsigned long long *chunks) {
    if (step_bytes == 0) return -1;
    return debug_deliver_host(plane, plane_rows, width, window, format, scale, bias, zero, gate_status, out, out_bytes, dst_offset, pitch_bytes, step_bytes, units, chunks);
}
// The host walk of a task with a reference plane (ref_rows x width bytes; NULL: none) and three gate statuses; step_bytes 0
// stands for the element size.
int nblic_amd_debug_deliver_ref_host(const unsigned char *plane, int plane_rows, int width, const unsigned char *ref, int ref_rows, const int *window, int format,
                                     float scale, float bias, int zero, const int *gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset,
                                     size_t pitch_bytes, size_t step_bytes, unsigned long long *units, unsigned long long *chunks) {
    if (!gate_status) return -1;
    return debug_deliver_host(plane, plane_rows, width, window, format, scale, bias, zero, gate_status[0], out, out_bytes, dst_offset, pitch_bytes, step_bytes, units, chunks,
                              ref, ref_rows, gate_status[1], gate_status[2]);
}

// ONE k_deliver launch over n caller-made planes as n tasks.  Plane k (plane_rows[k] x widths[k]) is uploaded at byte
// base_offsets[k] (0 .. 15) of a zeroed region that is larger; the task may read up256(rows * width) bytes from there, as the
// decoders' planes allow.  Destination k lies at byte dst_offsets[k] of a buffer of out_bytes[k] bytes filled with 0x5A, which
// comes back whole in outs[k].  gate_status[k] != -1 is put into a SerialState on the device, the task's gate.  windows: four
// ints per task (row0, row1, col0, col1).  -1: refused; -2: a HIP call failed.
int nblic_amd_debug_deliver(nblic_amd_ctx *c, int n, const unsigned char *const *planes, const size_t *plane_bytes, const size_t *base_offsets,
                            const int *plane_rows, const int *widths, const int *windows, const int *formats, const float *scales, const float *biases,
                            const int *zeros, const size_t *pitches, const size_t *dst_offsets, const size_t *out_bytes, unsigned char *const *outs,
                            const int *gate_status) {
    return debug_deliver(c, n, planes, plane_bytes, base_offsets, plane_rows, widths, windows, formats, scales, biases, zeros, pitches, nullptr, dst_offsets, out_bytes, outs, gate_status);
}
int nblic_amd_debug_deliver_ex(nblic_amd_ctx *c, int n, const unsigned char *const *planes, const size_t *plane_bytes, const size_t *base_offsets,
                               const int *plane_rows, const int *widths, const int *windows, const int *formats, const float *scales, const float *biases,
                               const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets, const size_t *out_bytes,
                               unsigned char *const *outs, const int *gate_status) {
    if (!steps) return -1;
    for (int k = 0; k < n; k++) if (steps[k] == 0) return -1;
    return debug_deliver(c, n, planes, plane_bytes, base_offsets, plane_rows, widths, windows, formats, scales, biases, zeros, pitches, steps, dst_offsets, out_bytes, outs, gate_status);
}
// ONE k_deliver launch like nblic_amd_debug_deliver_ex (steps may be NULL: the element size) over tasks that may have a
// reference: refs[k] (NULL: none) is a plane of ref_rows[k] x widths[k] bytes, uploaded at byte ref_base_offsets[k] (0 .. 15)
// of a zeroed region like the planes.  gate_status: THREE ints per task, each as in nblic_amd_debug_deliver.
int nblic_amd_debug_deliver_ref(nblic_amd_ctx *c, int n, const unsigned char *const *planes, const size_t *plane_bytes, const size_t *base_offsets,
                                const unsigned char *const *refs, const size_t *ref_base_offsets, const int *ref_rows,
                                const int *plane_rows, const int *widths, const int *windows, const int *formats, const float *scales, const float *biases,
                                const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets, const size_t *out_bytes,
                                unsigned char *const *outs, const int *gate_status) {
    if (!refs || !ref_base_offsets || !ref_rows) return -1;
    return debug_deliver(c, n, planes, plane_bytes, base_offsets, plane_rows, widths, windows, formats, scales, biases, zeros, pitches, steps, dst_offsets, out_bytes, outs, gate_status,
                         refs, ref_base_offsets, ref_rows);
}

// ---- k_collect on caller-made sources (tests/test_encode_from_device.py), and its host walk (tests/test_collect_host.py) ------
static bool debug_collect_task(CollectTask &T, const void *src, int rows, int cols, int format, float scale, float bias, size_t pitch, size_t step, const int *range) {
    if (!deliver_args_ok(format, scale, bias) || rows < 1 || cols < 1 || rows > int(kCollectMaxSide) || cols > int(kCollectMaxSide) || step > kCollectMaxStep) return false;
    T = CollectTask{};
    T.src = static_cast<const uint8_t *>(src);
    T.pitch = pitch; T.step = uint32_t(step);
    T.rows = uint32_t(rows); T.cols = uint32_t(cols);
    T.px0 = range ? uint32_t(range[0]) : 0u; T.px1 = range && range[1] ? uint32_t(range[1]) : T.rows * T.cols;
    T.format = uint32_t(format); T.scale = scale; T.bias = bias;
    return !range || (range[0] >= 0 && range[1] >= 0);
}
static bool debug_collect_ref(CollectTask &T, const void *ref, size_t pitch, size_t step) {
    if (step > 0xFFFFFFFFull) return false;                              // (collect_source_ok holds it against its limit)
    T.ref = static_cast<const uint8_t *>(ref); T.ref_pitch = pitch; T.ref_step = uint32_t(step);
    return true;
}
static int debug_collect_host(const void *src, size_t cap_bytes, const void *ref, size_t ref_cap_bytes, size_t ref_pitch_bytes, size_t ref_step_bytes, int rows, int cols,
                              size_t pitch_bytes, size_t step_bytes, int format, float scale, float bias, const int *range, unsigned char *out, size_t out_bytes,
                              unsigned long long *units, unsigned long long *chunks) {
    CollectTask T;
    if (!src || !out || !debug_collect_task(T, src, rows, cols, format, scale, bias, pitch_bytes, step_bytes, range)) return -1;
    T.dst = out;
    if (ref && !debug_collect_ref(T, ref, ref_pitch_bytes, ref_step_bytes)) return -1;
    if (!collect_task_ok(T, cap_bytes, ref_cap_bytes) || size_t(T.rows) * size_t(T.cols) > out_bytes) return -1;
    if (units) *units = collect_task_units(T);
    if (chunks) *chunks = collect_task_chunks(T);
    collect_host(T);
    return 0;
}
// What the collect-side entry points ask of a task's plane: out_bytes = a guard, up256(rows x cols), a guard.
static bool debug_plane_out_ok(int rows, int cols, size_t out_bytes) {
    const size_t plane = size_t(rows) * size_t(cols);
    return plane <= (size_t(1) << 30) && out_bytes == DebugBench::kGuard + up256(plane) + DebugBench::kGuard;
}
static int debug_collect(nblic_amd_ctx *c, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                         const void *const *refs, const size_t *ref_bytes, const size_t *ref_base_offsets, const size_t *ref_pitches, const size_t *ref_steps,
                         const int *rows, const int *cols, const size_t *pitches, const size_t *steps, const int *formats, const float *scales, const float *biases,
                         const int *ranges, unsigned char *const *outs, const size_t *out_bytes) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !srcs || !src_bytes || !base_offsets || !rows || !cols || !pitches || !steps || !formats || !scales || !biases || !outs || !out_bytes) return -1;
    const size_t count = size_t(n);
    std::vector<CollectTask> tasks(count);
    std::vector<size_t> src_in(count), ref_in(count, 0);
    DebugBench bench;
    for (int k = 0; k < n; k++) {
        const size_t i = size_t(k);
        if (!srcs[k] || !outs[k] || base_offsets[k] > 255 || src_bytes[k] > (size_t(1) << 30) ||
            !debug_collect_task(tasks[i], nullptr, rows[k], cols[k], formats[k], scales[k], biases[k], pitches[k], steps[k], ranges ? ranges + 2 * i : nullptr)) return -1;
        if (!debug_plane_out_ok(rows[k], cols[k], out_bytes[k])) return -1;
        src_in[i] = bench.source(srcs[k], src_bytes[k], base_offsets[k]);
        if (refs && refs[k]) {
            if (ref_base_offsets[k] > 255 || ref_bytes[k] > (size_t(1) << 30)) return -1;
            ref_in[i] = bench.source(refs[k], ref_bytes[k], ref_base_offsets[k]);
        }
        bench.output(outs[k], out_bytes[k]);
    }
    CollectTask *d_tasks = bench.alloc(c->device) ? bench.table<CollectTask>(count) : nullptr;
    if (!d_tasks) return -2;
    unsigned long long chunks = 0;
    for (int k = 0; k < n; k++) {                                        // the addresses are known now: the rest of the checks
        const size_t i = size_t(k);
        CollectTask &T = tasks[i];
        T.src = bench.in(src_in[i]);
        T.dst = bench.out(i) + DebugBench::kGuard;
        if (refs && refs[k] && !debug_collect_ref(T, bench.in(ref_in[i]), ref_pitches[k], ref_steps[k])) return -1;
        if (!collect_task_ok(T, src_bytes[k], T.ref ? ref_bytes[k] : 0)) return -1;                // nothing outside the uploaded bytes is the task's to read
        T.first_chunk = uint32_t(chunks); chunks += collect_task_chunks(T);
    }
    if (chunks >= (1ull << 31)) return -1;
    return bench.run([&](hipStream_t st) {
        return hipMemcpyAsync(d_tasks, tasks.data(), count * sizeof(CollectTask), hipMemcpyHostToDevice, st) == hipSuccess && collect_launch(d_tasks, n, uint32_t(chunks), st);
    });
}

// Host only: the shared unit walk (collect.h collect_host) over the source at src -- cap_bytes readable from there -- into
// the plane at out, which must be a multiple of 16 and hold rows x cols bytes.  range: the pixels [px0, px1) of the flat plane
// (NULL: all of it; px1 == 0: to the end).  -1: refused.
int nblic_amd_debug_collect_host(const void *src, size_t cap_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int format, float scale,
                                 float bias, const int *range, unsigned char *out, size_t out_bytes, unsigned long long *units, unsigned long long *chunks) {
    return debug_collect_host(src, cap_bytes, nullptr, 0, 0, 0, rows, cols, pitch_bytes, step_bytes, format, scale, bias, range, out, out_bytes, units, chunks);
}
// The same with a reference source (NULL: none): ref_cap_bytes readable from ref, its own pitch and step.
int nblic_amd_debug_collect_ref_host(const void *src, size_t cap_bytes, const void *ref, size_t ref_cap_bytes, size_t ref_pitch_bytes, size_t ref_step_bytes,
                                     int rows, int cols, size_t pitch_bytes, size_t step_bytes, int format, float scale, float bias, const int *range,
                                     unsigned char *out, size_t out_bytes, unsigned long long *units, unsigned long long *chunks) {
    return debug_collect_host(src, cap_bytes, ref, ref_cap_bytes, ref_pitch_bytes, ref_step_bytes, rows, cols, pitch_bytes, step_bytes, format, scale, bias, range, out, out_bytes, units, chunks);
}
// ONE k_collect launch over n caller-made sources as n tasks.  The bytes of source k (src_bytes[k] of them) are uploaded at
// byte base_offsets[k] (0 .. 255) of a region filled with 0xFF -- NaN in every float format, 255 as a pixel -- that is larger;
// the image's element (0, 0) is the first of them.  Plane k (rows x cols bytes) lies at byte 256 of a region filled with
// 0x5A, which comes back whole in outs[k]: out_bytes[k] = 256 + up256(rows x cols) + 256.  ranges: two ints per task
// (px0, px1; px1 == 0: to the end) or NULL.  -1: refused; -2: a HIP call failed.
int nblic_amd_debug_collect(nblic_amd_ctx *c, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets, const int *rows,
                            const int *cols, const size_t *pitches, const size_t *steps, const int *formats, const float *scales, const float *biases,
                            const int *ranges, unsigned char *const *outs, const size_t *out_bytes) {
    return debug_collect(c, n, srcs, src_bytes, base_offsets, nullptr, nullptr, nullptr, nullptr, nullptr, rows, cols, pitches, steps, formats, scales, biases, ranges, outs, out_bytes);
}
// The same launch over tasks that may have a reference: refs[k] (NULL: none) is a second source of ref_bytes[k] bytes with
// its own pitch and step, uploaded at byte ref_base_offsets[k] (0 .. 255) of a region of its own like the sources'.
int nblic_amd_debug_collect_ref(nblic_amd_ctx *c, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                                const void *const *refs, const size_t *ref_bytes, const size_t *ref_base_offsets, const size_t *ref_pitches, const size_t *ref_steps,
                                const int *rows, const int *cols, const size_t *pitches, const size_t *steps, const int *formats, const float *scales, const float *biases,
                                const int *ranges, unsigned char *const *outs, const size_t *out_bytes) {
    if (!refs || !ref_bytes || !ref_base_offsets || !ref_pitches || !ref_steps) return -1;
    return debug_collect(c, n, srcs, src_bytes, base_offsets, refs, ref_bytes, ref_base_offsets, ref_pitches, ref_steps, rows, cols, pitches, steps, formats, scales, biases, ranges, outs, out_bytes);
}

// Call it when nothing is outstanding on the context: it reads the groups' marks.
int nblic_amd_collect_ms(nblic_amd_ctx *c, double *ms, long *timed_launches) {
    if (!c || !ms || !timed_launches || hipSetDevice(c->device) != hipSuccess) return -1;
    std::lock_guard<std::mutex> g(c->api);
    for (auto &grp : c->groups) collect_timing_read(grp, true);
    std::lock_guard<std::mutex> l(c->stat_m);
    *ms = c->collect_ms; *timed_launches = c->collect_timed;
    return 0;
}

int nblic_amd_collect_stats(nblic_amd_ctx *c, long out[4]) {
    if (!c || !out) return -1;
    for (int k = 0; k < 4; k++) out[k] = c->collect_counts[k].load();
    return 0;
}

// ---- the colour plan: costs on the device, the choice on the host (color_plan.h, serial_engine.h k_color_cost) --------------
// ONE k_color_cost launch over the tasks, queued on st (cost_queue).  The costs are the caller's to zero.
static bool color_cost_queue(nblic_amd_ctx *c, ColorCostTask *tasks, size_t n, ColorCostTask *d_tasks, hipStream_t st) {
    return cost_queue(tasks, n, d_tasks, st, color_task_tiles, [&] {
        unsigned long long pixels = 0;
        for (size_t i = 0; i < n; i++) pixels += 3ull * tasks[i].rows * tasks[i].cols;
        c->color_counts[0] += 1; c->color_counts[1] += long(pixels);
    }, [&](const ColorCostTask *d, int m, uint32_t tiles) { return color_cost_launch(d, m, tiles, st); });
}

int nblic_amd_color_plan(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                         unsigned char *frame_modes, unsigned long long *costs) {
    if (!c || c->broken || n_images < 0 || n_images % 3 != 0 || !srcs || !frame_modes || format >= int(kCollectFormats) || !deliver_args_ok(format, scale, bias) ||
        hipSetDevice(c->device) != hipSuccess) return -1;
    const size_t frames = size_t(n_images) / 3;
    std::lock_guard<std::mutex> g(c->api);
    CollectFrom from{};
    from.srcs = srcs; from.format = uint32_t(format); from.scale = scale; from.bias = bias;
    std::vector<ColorCostTask> tasks;
    std::vector<size_t> frame_of;
    for (size_t f = 0; f < frames; f++) {                                // a frame with a refused source, or sources of unequal size: 0xFF, and nothing is launched for it
        ColorCostTask T{};
        bool ok = true;
        for (int ch = 0; ch < 3; ch++) {
            CollectTask S;
            ok = ok && collect_src_task(c, from, int(3 * f) + ch, S) != kSrcRefused && (ch == 0 || (S.rows == T.rows && S.cols == T.cols));
            if (!ok) break;
            T.src[ch] = S.src; T.pitch[ch] = S.pitch; T.step[ch] = S.step; T.rows = S.rows; T.cols = S.cols;
        }
        frame_modes[f] = uint8_t(kColorRefused);
        if (!ok) continue;
        T.format = uint32_t(format); T.scale = scale; T.bias = bias;
        tasks.push_back(T); frame_of.push_back(f);
    }
    std::vector<unsigned long long> sums(tasks.size() * kColorCosts, 0ull);
    if (!tasks.empty()) {
        SumsRun run;
        ColorCostTask *d_tasks = run.begin(sums.size()) ? run.mem.make<ColorCostTask>(tasks.size()) : nullptr;
        if (!d_tasks) return -1;
        for (size_t i = 0; i < tasks.size(); i++) tasks[i].costs = run.d_sums + i * kColorCosts;
        if (!run.run(c, sums, &c->color_ms, [&](hipStream_t st) { return color_cost_queue(c, tasks.data(), tasks.size(), d_tasks, st); })) return -1;
    }
    if (costs) std::fill(costs, costs + frames * kColorCosts, 0ull);
    for (size_t i = 0; i < tasks.size(); i++) {
        if (costs) memcpy(costs + frame_of[i] * kColorCosts, &sums[i * kColorCosts], kColorCosts * sizeof(unsigned long long));
        frame_modes[frame_of[i]] = color_choose(&sums[i * kColorCosts]);
    }
    return 0;
}

unsigned char nblic_amd_color_choose(const unsigned long long costs[9]) { return costs ? color_choose(costs) : uint8_t(kColorRefused); }
int nblic_amd_color_mode_valid(int mode) { return mode >= 0 && mode < 256 && color_mode_valid(uint32_t(mode)) ? 1 : 0; }
int nblic_amd_color_mode_ref(int mode, int channel) {
    return nblic_amd_color_mode_valid(mode) && channel >= 0 && channel < 3 ? color_mode_ref(uint32_t(mode), uint32_t(channel)) : -2;
}

int nblic_amd_color_plan_stats(nblic_amd_ctx *c, long out[2], double *last_plan_ms) {
    if (!c || !out) return -1;
    for (int k = 0; k < 2; k++) out[k] = c->color_counts[k].load();
    if (last_plan_ms) { std::lock_guard<std::mutex> l(c->stat_m); *last_plan_ms = c->color_ms; }
    return 0;
}

// A debug frame's task: all but the sources' addresses and costs.  false: an argument no task can hold.
static bool debug_color_task(ColorCostTask &T, const size_t *pitches, const size_t *steps, int rows, int cols, int format, float scale, float bias) {
    T = ColorCostTask{};
    if (rows < 1 || cols < 1 || format < 0 || format >= int(kCollectFormats)) return false;
    for (int ch = 0; ch < 3; ch++) {
        if (steps[ch] > 0xFFFFFFFFull) return false;                     // (collect_source_ok holds it against its limit)
        T.pitch[ch] = pitches[ch]; T.step[ch] = uint32_t(steps[ch]);
    }
    T.rows = uint32_t(rows); T.cols = uint32_t(cols); T.format = uint32_t(format); T.scale = scale; T.bias = bias;
    return true;
}

// Host only: the shared tile walk (color_plan.h color_cost_host) over the three sources of ONE frame, cap_bytes[ch] readable
// from srcs[ch].  costs: the nine sums; tiles: how many the kernel would run.  -1: refused.
int nblic_amd_debug_color_cost_host(const void *const *srcs, const size_t *cap_bytes, const size_t *pitches, const size_t *steps, int rows, int cols,
                                    int format, float scale, float bias, unsigned long long *costs, unsigned long long *tiles) {
    ColorCostTask T;
    if (!srcs || !cap_bytes || !pitches || !steps || !costs || !debug_color_task(T, pitches, steps, rows, cols, format, scale, bias)) return -1;
    unsigned long long caps[3];
    for (int ch = 0; ch < 3; ch++) { T.src[ch] = static_cast<const uint8_t *>(srcs[ch]); caps[ch] = cap_bytes[ch]; }
    T.costs = costs;
    if (!color_task_ok(T, caps)) return -1;
    if (tiles) *tiles = color_task_tiles(T);
    for (uint32_t k = 0; k < kColorCosts; k++) costs[k] = 0;
    color_cost_host(T);
    return 0;
}

// ONE k_color_cost launch over n caller-made frames as n tasks.  Three sources per frame (index 3 k + channel), each uploaded
// at byte base_offsets[] (0 .. 255) of a region of its own filled with 0xFF that is larger, as nblic_amd_debug_collect does.
// costs: nine sums per frame.  -1: refused; -2: a HIP call failed.
int nblic_amd_debug_color_cost(nblic_amd_ctx *c, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                               const size_t *pitches, const size_t *steps, const int *rows, const int *cols, const int *formats,
                               const float *scales, const float *biases, unsigned long long *costs) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !srcs || !src_bytes || !base_offsets || !pitches || !steps || !rows || !cols || !formats || !scales || !biases || !costs) return -1;
    const size_t count = size_t(n);
    std::vector<ColorCostTask> tasks(count);
    DebugBench bench;
    for (size_t i = 0; i < count; i++) {
        if (!debug_color_task(tasks[i], pitches + 3 * i, steps + 3 * i, rows[i], cols[i], formats[i], scales[i], biases[i])) return -1;
        for (size_t s = 3 * i; s < 3 * i + 3; s++) {
            if (!srcs[s] || base_offsets[s] > 255 || src_bytes[s] > (size_t(1) << 30)) return -1;
            bench.source(srcs[s], src_bytes[s], base_offsets[s]);
        }
    }
    bench.output(costs, count * kColorCosts * sizeof(unsigned long long), 0);
    ColorCostTask *d_tasks = bench.alloc(c->device) ? bench.table<ColorCostTask>(count) : nullptr;
    if (!d_tasks) return -2;
    for (size_t i = 0; i < count; i++) {                                 // the addresses are known now: the rest of the checks
        ColorCostTask &T = tasks[i];
        unsigned long long caps[3];
        for (size_t ch = 0; ch < 3; ch++) { T.src[ch] = bench.in(3 * i + ch); caps[ch] = src_bytes[3 * i + ch]; }
        T.costs = reinterpret_cast<unsigned long long *>(bench.out(0)) + i * kColorCosts;
        if (!color_task_ok(T, caps)) return -1;                          // nothing outside the uploaded bytes is the task's to read
    }
    return bench.run([&](hipStream_t st) { return color_cost_queue(c, tasks.data(), count, d_tasks, st); });
}

// ---- slice stacks: the plan, and the two kernels on caller-made inputs (stack.h) ---------------------------------------------
// ONE k_stack_cost launch over the tasks and their slices, queued on st (cost_queue).  The costs are the caller's to zero.
static bool stack_cost_queue(nblic_amd_ctx *c, StackCostTask *tasks, size_t n, const StackCostSlice *slices, size_t n_slices, StackCostTask *d_tasks,
                             StackCostSlice *d_slices, hipStream_t st) {
    return cost_queue(tasks, n, d_tasks, st, stack_task_tiles, [&] {
        unsigned long long pixels = 0;
        for (size_t i = 0; i < n; i++) pixels += (unsigned long long)(tasks[i].count) * tasks[i].rows * tasks[i].cols;
        c->stack_counts[0] += 1; c->stack_counts[1] += long(pixels);
    }, [&](const StackCostTask *d, int m, uint32_t tiles) { return stack_cost_launch(d, m, d_slices, tiles, st); }, slices, n_slices, d_slices);
}

int nblic_amd_stack_plan(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias, int depth, int key_every,
                         unsigned char *slice_modes, unsigned long long *costs) {
    if (!c || c->broken || n_images < 0 || depth < 1 || n_images % depth != 0 || key_every < 0 || !srcs || !slice_modes || format >= int(kCollectFormats) ||
        !deliver_args_ok(format, scale, bias) || hipSetDevice(c->device) != hipSuccess) return -1;
    const size_t D = size_t(depth), stacks = size_t(n_images) / D;
    std::lock_guard<std::mutex> g(c->api);
    CollectFrom from{};
    from.srcs = srcs; from.format = uint32_t(format); from.scale = scale; from.bias = bias;
    std::vector<StackCostTask> tasks;
    std::vector<StackCostSlice> slices;
    std::vector<size_t> stack_of;
    for (size_t s = 0; s < stacks; s++) {                                // a stack with a refused source, or sources of unequal size: 0xFF, and nothing is launched for it
        StackCostTask T{};
        T.first_slice = uint32_t(slices.size()); T.count = uint32_t(D);
        bool ok = true;
        for (size_t d = 0; d < D && ok; d++) {
            CollectTask S;
            ok = collect_src_task(c, from, int(s * D + d), S) != kSrcRefused && (d == 0 || (S.rows == T.rows && S.cols == T.cols));
            if (!ok) break;
            T.rows = S.rows; T.cols = S.cols;
            slices.push_back(StackCostSlice{S.src, S.pitch, S.step, 0u});
        }
        for (size_t d = 0; d < D; d++) slice_modes[s * D + d] = uint8_t(kStackRefused);
        if (!ok) { slices.resize(T.first_slice); continue; }
        T.format = uint32_t(format); T.scale = scale; T.bias = bias;
        tasks.push_back(T); stack_of.push_back(s);
    }
    std::vector<unsigned long long> sums(tasks.size() * D * 2, 0ull);
    if (!tasks.empty()) {
        SumsRun run;
        StackCostTask *d_tasks = run.begin(sums.size()) ? run.mem.make<StackCostTask>(tasks.size()) : nullptr;
        StackCostSlice *d_slices = d_tasks ? run.mem.make<StackCostSlice>(slices.size()) : nullptr;
        if (!d_slices) return -1;
        for (size_t i = 0; i < tasks.size(); i++) tasks[i].costs = run.d_sums + i * D * 2;
        if (!run.run(c, sums, &c->stack_ms, [&](hipStream_t st) { return stack_cost_queue(c, tasks.data(), tasks.size(), slices.data(), slices.size(), d_tasks, d_slices, st); })) return -1;
    }
    if (costs) std::fill(costs, costs + size_t(n_images) * 2, 0ull);
    for (size_t i = 0; i < tasks.size(); i++) {
        const size_t s = stack_of[i];
        if (costs) memcpy(costs + s * D * 2, &sums[i * D * 2], D * 2 * sizeof(unsigned long long));
        for (size_t d = 0; d < D; d++)
            slice_modes[s * D + d] = stack_slice_mode(uint32_t(d), uint32_t(key_every), sums[(i * D + d) * 2], sums[(i * D + d) * 2 + 1]);
    }
    return 0;
}

int nblic_amd_stack_choose(unsigned long long intra, unsigned long long delta) { return int(stack_choose(intra, delta)); }
int nblic_amd_stack_slice_mode(int d, int key_every, unsigned long long intra, unsigned long long delta) {
    return d < 0 || key_every < 0 ? -1 : int(stack_slice_mode(uint32_t(d), uint32_t(key_every), intra, delta));
}
int nblic_amd_stack_mode_valid(int mode) { return mode >= 0 && mode < 256 && stack_mode_valid(uint32_t(mode)) ? 1 : 0; }
int nblic_amd_stack_modes_valid(int n_images, int depth, const unsigned char *slice_modes) { return stack_modes_ok(n_images, depth, slice_modes) ? 1 : 0; }

int nblic_amd_stack_plan_stats(nblic_amd_ctx *c, long out[4], double *last_ms) {
    if (!c || !out) return -1;
    for (int k = 0; k < 4; k++) out[k] = c->stack_counts[k].load();
    if (last_ms) { std::lock_guard<std::mutex> l(c->stat_m); last_ms[0] = c->stack_ms; last_ms[1] = c->stack_deliver_ms; }
    return 0;
}

// A debug stack's task: all but the sources' addresses and costs.  false: an argument no task can hold.
static bool debug_stack_cost_task(StackCostTask &T, int count, int rows, int cols, int format, float scale, float bias) {
    T = StackCostTask{};
    if (count < 1 || count > 65536 || rows < 1 || cols < 1 || format < 0 || format >= int(kCollectFormats)) return false;
    T.count = uint32_t(count); T.rows = uint32_t(rows); T.cols = uint32_t(cols); T.format = uint32_t(format); T.scale = scale; T.bias = bias;
    return true;
}

// Host only: the shared tile walk (stack.h stack_cost_host) over the `count` sources of ONE stack, cap_bytes[d] readable from
// srcs[d].  costs: two sums per slice (intra, delta); tiles: how many workgroups the kernel would run.  -1: refused.
int nblic_amd_debug_stack_cost_host(int count, const void *const *srcs, const size_t *cap_bytes, const size_t *pitches, const size_t *steps, int rows, int cols,
                                    int format, float scale, float bias, unsigned long long *costs, unsigned long long *tiles) {
    StackCostTask T;
    if (!srcs || !cap_bytes || !pitches || !steps || !costs || !debug_stack_cost_task(T, count, rows, cols, format, scale, bias)) return -1;
    std::vector<StackCostSlice> slices(static_cast<size_t>(count));
    std::vector<unsigned long long> caps(static_cast<size_t>(count));
    for (int d = 0; d < count; d++) {
        if (steps[d] > 0xFFFFFFFFull) return -1;
        slices[size_t(d)] = StackCostSlice{static_cast<const uint8_t *>(srcs[d]), pitches[d], uint32_t(steps[d]), 0u};
        caps[size_t(d)] = cap_bytes[d];
    }
    T.costs = costs;
    if (!stack_cost_task_ok(T, slices.data(), caps.data())) return -1;
    if (tiles) *tiles = stack_task_tiles(T);
    for (int k = 0; k < 2 * count; k++) costs[k] = 0;
    stack_cost_host(T, slices.data());
    return 0;
}

// ONE k_stack_cost launch over n caller-made stacks as n tasks.  Stack k has counts[k] sources; srcs / src_bytes /
// base_offsets / pitches / steps have one entry per source, the stacks' one after the other, each source uploaded at byte
// base_offsets[] (0 .. 255) of a region of its own filled with 0xFF that is larger.  costs: two sums per source.
// -1: refused; -2: a HIP call failed.
int nblic_amd_debug_stack_cost(nblic_amd_ctx *c, int n, const int *counts, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                               const size_t *pitches, const size_t *steps, const int *rows, const int *cols, const int *formats,
                               const float *scales, const float *biases, unsigned long long *costs) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !counts || !srcs || !src_bytes || !base_offsets || !pitches || !steps || !rows || !cols || !formats || !scales || !biases || !costs) return -1;
    const size_t count = size_t(n);
    std::vector<StackCostTask> tasks(count);
    std::vector<StackCostSlice> slices;
    DebugBench bench;
    for (size_t i = 0; i < count; i++) {
        if (!debug_stack_cost_task(tasks[i], counts[i], rows[i], cols[i], formats[i], scales[i], biases[i]) || slices.size() + size_t(counts[i]) > (size_t(1) << 20)) return -1;
        tasks[i].first_slice = uint32_t(slices.size());
        for (int d = 0; d < counts[i]; d++) {
            const size_t s = slices.size();
            if (!srcs[s] || base_offsets[s] > 255 || src_bytes[s] > (size_t(1) << 30) || steps[s] > 0xFFFFFFFFull) return -1;
            bench.source(srcs[s], src_bytes[s], base_offsets[s]);
            slices.push_back(StackCostSlice{nullptr, pitches[s], uint32_t(steps[s]), 0u});
        }
    }
    bench.output(costs, slices.size() * 2 * sizeof(unsigned long long), 0);
    StackCostTask *d_tasks = bench.alloc(c->device) ? bench.table<StackCostTask>(count) : nullptr;
    StackCostSlice *d_slices = d_tasks ? bench.table<StackCostSlice>(slices.size()) : nullptr;
    if (!d_slices) return -2;
    for (size_t i = 0; i < count; i++) {                                 // the addresses are known now: the rest of the checks
        StackCostTask &T = tasks[i];
        std::vector<unsigned long long> caps(T.count);
        for (uint32_t d = 0; d < T.count; d++) {
            const size_t s = T.first_slice + d;
            slices[s].src = bench.in(s); caps[d] = src_bytes[s];
        }
        T.costs = reinterpret_cast<unsigned long long *>(bench.out(0)) + size_t(T.first_slice) * 2;
        if (!stack_cost_task_ok(T, slices.data(), caps.data())) return -1;      // nothing outside the uploaded bytes is the task's to read
    }
    return bench.run([&](hipStream_t st) { return stack_cost_queue(c, tasks.data(), count, slices.data(), slices.size(), d_tasks, d_slices, st); });
}

// A debug run's task and slice records: all but the addresses.  window: row0, row1, col0, col1 of planes of plane_rows x
// width; per slice a scale, a bias, a zero flag, a pitch and a step (0: the element size).  false: an argument no task can hold.
static bool debug_stack_run(StackDeliverTask &R, StackSlice *S, int count, int plane_rows, int width, const int *window, int format, const float *scales,
                            const float *biases, const int *zeros, const size_t *pitches, const size_t *steps) {
    R = StackDeliverTask{};
    if (count < 1 || count > 65536 || plane_rows < 1 || width < 1 || !window || format < 0 || format >= int(kDeliverFormats)) return false;
    if (window[0] < 0 || window[1] <= window[0] || window[1] > plane_rows || window[2] < 0 || window[3] <= window[2] || window[3] > width) return false;
    R.count = uint32_t(count); R.rows = uint32_t(window[1] - window[0]); R.col0 = uint32_t(window[2]); R.col1 = uint32_t(window[3]);
    R.src_pitch = uint32_t(width); R.format = uint32_t(format);
    for (int d = 0; d < count; d++) {
        if (!deliver_args_ok(format, scales[d], biases[d]) || steps[d] > kDeliverMaxStep || pitches[d] > (size_t(1) << 40)) return false;
        S[d] = StackSlice{};
        S[d].scale = scales[d]; S[d].bias = biases[d]; S[d].zero = zeros[d] ? 1u : 0u;
        S[d].dst_pitch = pitches[d]; S[d].dst_step = steps[d] ? uint32_t(steps[d]) : deliver_elem(R.format);
    }
    return true;
}
// Does slice S of run R, with a destination, stay inside the out_bytes - dst_offset bytes behind it?
static bool debug_stack_fits(const StackDeliverTask &R, const StackSlice &S, size_t out_bytes, size_t dst_offset) {
    return dst_offset <= out_bytes && deliver_extent(R.rows, R.col1 - R.col0, R.format, S.dst_pitch, S.dst_step) <= out_bytes - dst_offset;
}

// Host only: the shared walk (stack.h stack_deliver_host) over ONE run of `count` caller-made planes of plane_rows x width
// bytes each; slice d goes to outs[d] + dst_offsets[d] (outs[d] NULL: a skipped slice), gate_status[d] stands for its gate
// (-1: none).  units / chunks: what a launch would count for the task.  -1: refused.
int nblic_amd_debug_stack_deliver_host(int count, const unsigned char *const *planes, int plane_rows, int width, const int *window, int format,
                                       const float *scales, const float *biases, const int *zeros, const int *gate_status, unsigned char *const *outs,
                                       const size_t *out_bytes, const size_t *dst_offsets, const size_t *pitches, const size_t *steps,
                                       unsigned long long *units, unsigned long long *chunks) {
    if (!planes || !scales || !biases || !zeros || !gate_status || !outs || !out_bytes || !dst_offsets || !pitches || !steps || count < 1 || count > 65536) return -1;
    StackDeliverTask R;
    std::vector<StackSlice> S(static_cast<size_t>(count));
    if (!debug_stack_run(R, S.data(), count, plane_rows, width, window, format, scales, biases, zeros, pitches, steps)) return -1;
    std::vector<int> gates(static_cast<size_t>(count));
    const size_t skip = size_t(window[0]) * size_t(width);
    for (int d = 0; d < count; d++) {
        if (!planes[d]) return -1;
        S[size_t(d)].src = planes[d] + skip; S[size_t(d)].src_bytes = size_t(plane_rows) * size_t(width) - skip;
        if (outs[d]) {
            if (!debug_stack_fits(R, S[size_t(d)], out_bytes[d], dst_offsets[d])) return -1;
            S[size_t(d)].dst = outs[d] + dst_offsets[d];
        }
        gates[size_t(d)] = gate_status[d] == -1 ? int(kDone) : gate_status[d];
    }
    if (!stack_task_ok(R, S.data())) return -1;
    if (units) *units = stack_task_units(R);
    if (chunks) *chunks = stack_task_chunks(R);
    stack_deliver_host(R, S.data(), gates.data());
    return 0;
}

// ONE k_deliver_stack launch over n caller-made runs as n tasks.  Run k has counts[k] planes of plane_rows[k] x widths[k]
// bytes; planes / base_offsets / scales / biases / zeros / pitches / steps / dst_offsets / out_bytes / outs / gate_status have
// one entry per plane, the runs' one after the other.  A plane is uploaded at byte base_offsets[] (0 .. 15) of a zeroed
// region that is larger and may be read for up256(rows * width) bytes, as the decoders' planes allow; a destination lies at
// byte dst_offsets[] of a buffer of out_bytes[] bytes filled with 0x5A, which comes back whole in outs[] (NULL: a skipped
// slice); gate_status[] != -1 is put into a SerialState on the device, the slice's gate.  -1: refused; -2: a HIP call failed.
int nblic_amd_debug_stack_deliver(nblic_amd_ctx *c, int n, const int *counts, const unsigned char *const *planes, const size_t *base_offsets,
                                  const int *plane_rows, const int *widths, const int *windows, const int *formats, const float *scales, const float *biases,
                                  const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets, const size_t *out_bytes,
                                  unsigned char *const *outs, const int *gate_status) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !counts || !planes || !base_offsets || !plane_rows || !widths || !windows || !formats || !scales || !biases ||
        !zeros || !pitches || !steps || !dst_offsets || !out_bytes || !outs || !gate_status) return -1;
    const size_t count = size_t(n);
    size_t total = 0;
    for (size_t i = 0; i < count; i++) { if (counts[i] < 1 || counts[i] > 65536) return -1; total += size_t(counts[i]); }
    if (total > (size_t(1) << 20)) return -1;
    std::vector<StackDeliverTask> runs(count);
    std::vector<StackSlice> S(total);
    std::vector<size_t> out_of(total, 0), plane_len(total);
    DebugBench bench;
    size_t s0 = 0;
    for (size_t i = 0; i < count; i++) {
        if (!debug_stack_run(runs[i], S.data() + s0, counts[i], plane_rows[i], widths[i], windows + 4 * i, formats[i], scales + s0, biases + s0, zeros + s0, pitches + s0, steps + s0)) return -1;
        runs[i].first_slice = uint32_t(s0);
        const size_t bytes = size_t(plane_rows[i]) * size_t(widths[i]);
        if (bytes > (size_t(1) << 30)) return -1;
        for (size_t s = s0; s < s0 + size_t(counts[i]); s++) {
            if (!planes[s] || base_offsets[s] > 15 || out_bytes[s] > (size_t(1) << 30)) return -1;
            if (outs[s] && !debug_stack_fits(runs[i], S[s], out_bytes[s], dst_offsets[s])) return -1;
            plane_len[s] = bytes;
            bench.plane(planes[s], bytes, base_offsets[s]);
            if (outs[s]) out_of[s] = bench.output(outs[s], out_bytes[s]);
        }
        s0 += size_t(counts[i]);
    }
    bench.gates(gate_status, total);
    StackDeliverTask *d_runs = bench.alloc(c->device) ? bench.table<StackDeliverTask>(count) : nullptr;
    StackSlice *d_slices = d_runs ? bench.table<StackSlice>(total) : nullptr;
    if (!d_slices) return -2;
    for (size_t i = 0; i < count; i++) {                                 // the addresses are known now: the rest of the checks
        const size_t skip = size_t(windows[4 * i]) * size_t(widths[i]);
        for (size_t s = runs[i].first_slice; s < size_t(runs[i].first_slice) + runs[i].count; s++) {
            S[s].src = bench.in(s) + skip; S[s].src_bytes = up256(plane_len[s]) - skip;
            if (outs[s]) S[s].dst = bench.out(out_of[s]) + dst_offsets[s];
            if (gate_status[s] != -1) S[s].gate = bench.gate(s);
        }
        if (!stack_task_ok(runs[i], S.data())) return -1;
    }
    return bench.run([&](hipStream_t st) {
        c->stack_counts[2] += 1; c->stack_counts[3] += long(count);
        unsigned long long chunks = 0;
        return deliver_stack_upload(runs.data(), count, S.data(), total, d_runs, d_slices, st, chunks) && deliver_stack_launch(d_runs, n, d_slices, uint32_t(chunks), st);
    });
}

void nblic_amd_debug_live(long counts[4]) { for (int k = 0; k < 4; k++) counts[k] = g_live[k].load(std::memory_order_relaxed); }

int nblic_amd_debug_workspaces(nblic_amd_ctx *c, int group, int slot, long out[8]) {
    if (!c || !out) return -1;
    std::lock_guard<std::mutex> g(c->api);                                   // no batch of this context is in flight
    if (group < 0) {
        long held[2] = {0, 0}, cap[2] = {0, 0};
        std::lock_guard<std::mutex> l(c->fm);
        for (const CodedBuf &b : c->cbufs) { held[0] += b.get() != nullptr; cap[0] += long(b.capacity()); }
        for (const PackRows &p : c->pbufs) { held[1] += p.get() != nullptr; cap[1] += long(p.capacity_words()); }
        out[0] = long(c->cbufs.size()); out[1] = held[0]; out[2] = cap[0];
        out[3] = long(c->pbufs.size()); out[4] = held[1]; out[5] = cap[1];
        out[6] = long(c->dec_arena.capacity()); out[7] = long(c->dec_jobs.capacity());
        return 0;
    }
    if (size_t(group) >= c->groups.size() || slot < 0 || size_t(slot) >= c->groups[size_t(group)].slots.size()) return -1;
    const Slot &s = c->groups[size_t(group)].slots[size_t(slot)];
    out[0] = long(s.px_cap); out[1] = long(s.ev_cap); out[2] = long(s.mem.bytes());
    out[3] = long(reinterpret_cast<uintptr_t>(s.b.rec1)); out[4] = long(reinterpret_cast<uintptr_t>(s.b.events));
    out[5] = long(s.d_img.capacity()); out[6] = long(s.d_recon.capacity()); out[7] = long(s.d_stats.capacity());
    return 0;
}

int nblic_amd_copy_stats(nblic_amd_ctx *c, long out[4]) {
    if (!c || !out) return -1;
    c->engine.stats(out);
    return 0;
}

int nblic_amd_queue_plan_stats(nblic_amd_ctx *c, long out[40], double *plan_ms) {
    static_assert(kPlanMaxClasses == 32, "the header says 8 + 32 values");
    if (!c || !out) return -1;
    const QueuePlan &p = c->queue_plan;                              // written once, before create_ex returned
    std::fill(out, out + 40, 0L);
    out[0] = p.state; out[1] = p.classes; out[2] = p.candidates; out[3] = p.n_groups; out[4] = p.spread(); out[5] = p.unplanned_spread();
    for (int k = 0; k < p.classes; k++) out[8 + k] = p.groups_per_class[k];
    if (plan_ms) *plan_ms = p.plan_ms;
    return 0;
}

void nblic_amd_set_max_pixels(nblic_amd_ctx *c, long max_pixels) {
    if (!c) c = default_ctx();                                               // NULL: the context behind the drop-in entry points
    if (c) c->max_px = max_pixels > 0 ? max_pixels : kMaxPixels;
}
void nblic_amd_set_serial_rows(nblic_amd_ctx *c, int rows) {
    if (!c) c = default_ctx();
    if (c) { std::lock_guard<std::mutex> g(c->api); c->serial_rows = rows > 0 ? rows : 0; }
}
void nblic_amd_set_long_chains(nblic_amd_ctx *c, int min_records, int block_records) {
    if (!c) c = default_ctx();
    if (c) { std::lock_guard<std::mutex> g(c->api); c->long_min = min_records < 0 ? -1 : min_records; c->long_block = block_records > 0 ? block_records : 0; }
}
int nblic_amd_long_chain_stats(nblic_amd_ctx *c, long counts[8], int reset) {
    if (!c) c = default_ctx();
    if (!c || !counts) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    for (int k = 0; k < 8; k++) { counts[k] = c->long_counts[k]; if (reset) c->long_counts[k] = 0; }
    return 0;
}
long nblic_amd_serial_launches(nblic_amd_ctx *c) {
    if (!c) c = default_ctx();
    if (!c) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    return c->serial_launch_count;
}
int nblic_amd_lsq_redo_counts(nblic_amd_ctx *c, unsigned long long counts[2], int reset) {
    if (!c) c = default_ctx();
    if (!c || !counts) return -1;
    std::lock_guard<std::mutex> g(c->api);                                   // no batch of this context is in flight
    unsigned long long v[2] = {0, 0};
    if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(v, c->d_redo, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (reset && hipMemset(c->d_redo, 0, sizeof v) != hipSuccess) return -1;
    counts[0] = v[0]; counts[1] = v[1];
    return 0;
}
void nblic_amd_set_feed_chunk(nblic_amd_ctx *c, size_t bytes) {
    if (!c) c = default_ctx();
    if (c) { std::lock_guard<std::mutex> g(c->api); c->feed_chunk = bytes ? bytes : (size_t(1) << 20); }
}
long nblic_amd_last_fed_bytes(nblic_amd_ctx *c) {
    if (!c) c = default_ctx();
    return c ? c->fed_bytes : -1;
}
void nblic_amd_enable_timing(nblic_amd_ctx *c, int on) { c->timing = on != 0; c->timing_mask = on == 2 ? kRooflineStages : ~0ull; }

int nblic_amd_stage_times(nblic_amd_ctx *c, double *ms, const char **names, int cap) {
    int n = kE1Kernels;
    for (int k = 0; k < n && k < cap; k++) { ms[k] = c->stage_ms[k]; if (names) names[k] = kE1StageNames[k]; }
    return n < cap ? n : cap;
}

long nblic_amd_last_launches(nblic_amd_ctx *c) { return c->stage_launches; }

void nblic_amd_last_stats(nblic_amd_ctx *c, double *total_bins, double *coder_seconds_sum) {
    if (total_bins) *total_bins = c->total_bins;
    if (coder_seconds_sum) *coder_seconds_sum = c->coder_s;
}

int nblic_amd_encode_batch(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                           const int *heights, const int *widths, unsigned char *const *outs, const size_t *out_caps,
                           long *out_lens) {
    if (!c) return -1;
    const bool ok = run_batch(c, nblic_amd_ctx::SubmitItem{nullptr, 0, n_images, imgs, imgs_on_device != 0, heights, widths, outs, out_caps, out_lens, nullptr, nullptr, nullptr});
    if (nothing_outstanding(c)) for (auto &g : c->groups) collect_timing(c, g);
    report_coders(c);
    return ok ? 0 : -1;
}

nblic_amd_batch *nblic_amd_encode_batch_begin(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                              const int *heights, const int *widths, unsigned char *const *outs,
                                              const size_t *out_caps, long *out_lens) {
    if (!c || n_images < 0 || hipSetDevice(c->device) != hipSuccess) return nullptr;
    auto *b = new nblic_amd_batch;
    queue_batch(c, nblic_amd_ctx::SubmitItem{b, 0, n_images, imgs, imgs_on_device != 0, heights, widths, outs, out_caps, out_lens, nullptr, nullptr, nullptr});
    return b;
}

int nblic_amd_encode_batch_end(nblic_amd_ctx *c, nblic_amd_batch *b) {
    if (!c || !b) return -1;
    const bool ok = encode_wait(c, b) && !c->broken;         // b->ok and b->lens: this batch's images only
    report_coders(c);
    delete b;
    return ok ? 0 : -1;
}

long nblic_amd_debug_stage(nblic_amd_ctx *c, const unsigned char *img, int h, int w, int which, void *out, size_t out_bytes) {
    if (!c || !size_ok(h, w, c->max_px)) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    const int id = take_group(c);
    Group &grp = c->groups[size_t(id)];
    Slot &s = grp.slots[0];
    grp.n_jobs = 1; s.job = 0; s.h = h; s.w = w; s.cb = -1; s.pack_n = 1; s.pack_lane = 0; s.near = 0; s.effort = 1;
    const uint8_t *imgs[1] = {img};
    long count = -1;
    size_t n = size_t(h) * size_t(w);
    if (launch_front(c, grp, imgs, false) && launch_back(c, grp, false) && hipStreamSynchronize(grp.stream) == hipSuccess) {
        grp.tm_pending = false;
        const void *src = nullptr; size_t esz = 0, cnt = 0;
        switch (which) {
            case 0: src = s.b.rec1; esz = 4; cnt = n; break;
            case 1: src = s.b.pxs; esz = 2; cnt = n; break;
            case 2: src = s.b.z; esz = 1; cnt = n; break;
            case 3: src = s.b.cnt; esz = 1; cnt = n; break;
            case 4: src = s.b.events; esz = 4; cnt = s.n_ev; break;
            case 5: src = s.b.coded; esz = 2; cnt = s.n_ev; break;
            case 6: src = s.b.dbg_out; esz = 8; cnt = 4096; break;
            case 7: src = s.b.totals; esz = 4; cnt = size_t(kTotalsStride); break;       // [kWideTouchFlag]: 32-bit touch positions were needed
            default: break;
        }
        if (src && cnt * esz <= out_bytes && hipMemcpy(out, src, cnt * esz, hipMemcpyDeviceToHost) == hipSuccess) count = long(cnt);
    }
    return_coded(c, s);
    release_group(c, id);
    return count;
}

int nblic_amd_encode_batch_modes(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                 const int *heights, const int *widths, const int *nears, const int *efforts,
                                 unsigned char *const *outs, const size_t *out_caps, long *out_lens, unsigned char *const *recons) {
    if (!c) return -1;
    return run_batch(c, nblic_amd_ctx::SubmitItem{nullptr, 0, n_images, imgs, imgs_on_device != 0, heights, widths, outs, out_caps, out_lens, nears, efforts, recons}) ? 0 : -1;
}

int nblic_amd_decode_batch(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                           unsigned char *const *imgs, const size_t *img_caps, int *heights, int *widths, int *nears, int *efforts,
                           int *status) {
    if (!c || n_images < 0) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (!decode_batch(c, n_images, streams, stream_lens, imgs, img_caps, heights, widths, nears, efforts, status)) return -1;
    for (int k = 0; k < n_images; k++) if (status[k] != 0) return -1;
    return 0;
}

int nblic_amd_decode_batch_to(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens, const nblic_amd_dest *dests,
                              int format, float scale, float bias, int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!dests || n_images < 0 || !deliver_args_ok(format, scale, bias)) return -1;
    const std::vector<nblic_amd_dest_ex> ex = dests_ex(dests, n_images, format, scale, bias);
    return nblic_amd_decode_batch_to_ex(c, n_images, streams, stream_lens, ex.data(), format, heights, widths, nears, efforts, status);
}
static int decode_batch_to_modes(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens, const nblic_amd_dest_ex *dests,
                                 int format, const uint8_t *modes, int *heights, int *widths, int *nears, int *efforts, int *status, const StackArg *stack = nullptr) {
    if (!c || c->broken || n_images < 0 || !streams || !stream_lens || !dests || !heights || !widths || !nears || !efforts || !status || format < 0 || format >= int(kDeliverFormats)) return -1;
    for (int k = 0; k < n_images; k++) if (!streams[k]) return -1;
    if (stack && !stack_modes_ok(n_images, stack->depth, stack->modes)) return -1;
    DeliverTo to{dests, uint32_t(format), modes};
    if (stack) { to.slice_modes = stack->modes; to.depth = stack->depth; }
    std::lock_guard<std::mutex> g(c->api);
    deliver_stats_reset(c);
    if (!decode_batch(c, n_images, streams, stream_lens, nullptr, nullptr, heights, widths, nears, efforts, status, &to)) return -1;
    for (int k = 0; k < n_images; k++) if (status[k] != 0) return -1;
    return 0;
}
int nblic_amd_deliver_stats(nblic_amd_ctx *c, long out[2]) {
    if (!c || !out) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    out[0] = c->deliver_tasks; out[1] = c->deliver_strided;
    return 0;
}

nblic_amd_stream *nblic_amd_stream_begin(nblic_amd_ctx *c, const unsigned char *img, int img_on_device, int height, int width, int near, int effort, int band_rows) {
    return stream_open(c, img, img_on_device != 0, height, width, near, effort, band_rows);
}
nblic_amd_stream *nblic_amd_stream_resume(nblic_amd_ctx *c, const unsigned char *img, int img_on_device, const void *checkpoint, size_t checkpoint_bytes) {
    return stream_resume(c, img, img_on_device != 0, checkpoint, checkpoint_bytes);
}
int nblic_amd_stream_run(nblic_amd_stream *s, double budget_seconds, unsigned char *out, size_t out_cap, size_t *out_len) {
    size_t n = 0;
    const int rc = stream_run(s, budget_seconds, out, out_cap, &n);
    if (out_len) *out_len = n;
    return rc;
}
size_t nblic_amd_stream_checkpoint(nblic_amd_stream *s, void *buf, size_t cap) { return s ? stream_checkpoint(s, buf, cap) : 0; }
int nblic_amd_stream_progress(nblic_amd_stream *s, int *rows_done, unsigned long long *bytes_total, unsigned char sha256[32], double *model_ms) {
    if (!s) return -1;
    if (rows_done) *rows_done = s->next_row;
    if (bytes_total) *bytes_total = s->bytes_total;
    if (sha256) s->sha.digest(sha256);
    if (model_ms) *model_ms = s->model_ms;
    return s->failed ? -1 : (s->finished ? 1 : 0);
}
int nblic_amd_stream_recon(nblic_amd_stream *s, unsigned char *plane, int *first_row, int *end_row) {
    if (!s || !plane || s->failed || hipSetDevice(s->c->device) != hipSuccess) return -1;
    if (first_row) *first_row = s->first_row;
    if (end_row) *end_row = s->next_row;
    const size_t at = size_t(s->first_row) * size_t(s->w), n = size_t(s->next_row - s->first_row) * size_t(s->w);
    if (n == 0) return 0;
    // lossless: the reconstruction IS the input (NBLIC.c:876 rewrites the same bytes)
    return hipMemcpy(plane + at, (s->near > 0 ? s->d_recon : s->d_img) + at, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
void nblic_amd_stream_end(nblic_amd_stream *s) { stream_free(s); }
int nblic_amd_stream_set_index(nblic_amd_stream *s, int every_rows) { return stream_set_index(s, every_rows); }
size_t nblic_amd_stream_index(nblic_amd_stream *s, void *buf, size_t cap) { return stream_index(s, buf, cap); }
int nblic_amd_stream_set_front(nblic_amd_stream *s, int front) { return stream_set_front(s, front); }

nblic_amd_dstream *nblic_amd_dstream_begin(nblic_amd_ctx *c, int band_rows) { return dstream_new(c, band_rows); }
nblic_amd_dstream *nblic_amd_dstream_resume(nblic_amd_ctx *c, const void *checkpoint, size_t bytes) { return dstream_resume(c, checkpoint, bytes); }
int nblic_amd_stream_check(nblic_amd_ctx *c, const void *checkpoint, size_t bytes) {
    EncodeCheckpoint H;
    return stream_check(checkpoint, bytes, c ? c->max_px : kMaxPixels, H);
}
int nblic_amd_dstream_check(nblic_amd_ctx *c, const void *checkpoint, size_t bytes) {
    DecodeCheckpoint H;
    return dstream_check(checkpoint, bytes, c ? c->max_px : kMaxPixels, H);
}
int nblic_amd_dstream_feed(nblic_amd_dstream *d, const unsigned char *bytes, size_t n, int final_) {
    if (!d || d->failed || (n && !bytes) || (d->complete && n)) return -1;
    d->pend.insert(d->pend.end(), bytes, bytes + n);
    if (final_) d->complete = true;
    return 0;
}
int nblic_amd_dstream_info(nblic_amd_dstream *d, int *kind, int *height, int *width, int *near, int *effort) {
    if (!d) return -1;
    if (!d->have_head && !d->refused && !d->failed && hipSetDevice(d->device) == hipSuccess) dstream_try_header(d);
    if (d->refused || (d->failed && !d->have_head)) return -1;
    if (!d->have_head) return 0;
    if (kind) *kind = d->it.kind;
    if (height) *height = d->it.h;
    if (width) *width = d->it.w;
    if (near) *near = d->it.near;
    if (effort) *effort = d->it.effort;
    return 1;
}
int nblic_amd_dstream_run(nblic_amd_dstream *d, double budget_seconds, unsigned char *rows_out, size_t cap, int *first_row, int *end_row) {
    if (!d) return -1;
    return dstream_run(d, budget_seconds, rows_out, cap, first_row, end_row);
}
int nblic_amd_dstream_progress(nblic_amd_dstream *d, int *rows_done, unsigned long long *feed_from, unsigned char sha256[32], size_t *device_bytes) {
    if (!d) return -1;
    if (rows_done) *rows_done = d->have_head ? d->H.next_row : 0;
    if (feed_from) *feed_from = d->have_head ? (d->H.pos & ~511ull) : 0ull;
    if (sha256) { Sha256 copy = d->sha; copy.digest(sha256); }
    if (device_bytes) *device_bytes = d->mem.bytes();
    return (d->failed || d->refused) ? -1 : (d->done ? 1 : 0);
}
size_t nblic_amd_dstream_checkpoint(nblic_amd_dstream *d, void *buf, size_t cap) { return d ? dstream_checkpoint(d, buf, cap, d->band_rows, d->sha) : 0; }
void nblic_amd_dstream_end(nblic_amd_dstream *d) { dstream_free(d); }

void nblic_amd_set_index_round(nblic_amd_ctx *c, int segments) { if (c) c->index_round_segments = segments > 0 ? segments : 0; }
int nblic_amd_index_check(nblic_amd_ctx *c, const void *index, size_t index_bytes, const unsigned char *stream, size_t stream_bytes) {
    IndexView V;
    return index_check(index, index_bytes, stream, stream_bytes, c ? c->max_px : kMaxPixels, V);
}
int nblic_amd_index_is_packed(const void *index, size_t index_bytes) { return index_is_packed(index, index_bytes) ? 1 : 0; }
size_t nblic_amd_index_unpacked_bytes(const void *packed, size_t packed_bytes) { return index_unpacked_bytes(packed, packed_bytes); }
size_t nblic_amd_index_pack_bound(const void *index, size_t index_bytes) {
    PackHead H;
    if (!pack_head(static_cast<const uint8_t *>(index), index_bytes, "NBLSIDX1", kUnpackedVersion, H)) return 0;
    return index_pack_bound(H.count, index_entry_bytes(H.kind, H.w, H.effort));
}
long nblic_amd_index_pack(const void *index, size_t index_bytes, unsigned char *out, size_t cap) {
    IndexView V;
    std::vector<uint8_t> packed;
    if (index_is_packed(index, index_bytes) || index_check(index, index_bytes, nullptr, 0, kMaxPixels, V) != 0 || !pack_index(index, index_bytes, packed)) return -1;
    if (out && cap >= packed.size()) memcpy(out, packed.data(), packed.size());
    return long(packed.size());
}
long nblic_amd_index_unpack(const void *packed, size_t packed_bytes, unsigned char *out, size_t cap) {
    const size_t need = index_unpacked_bytes(packed, packed_bytes);
    if (need == 0) return -1;
    if (!out || cap < need) {                                            // the size alone -- of a packed index that passes its structural walk
        PackedView V;
        return packed_walk(packed, packed_bytes, V) ? long(need) : -1;
    }
    std::vector<uint8_t> index;
    if (!unpack_index(packed, packed_bytes, index) || index.size() != need) return -1;
    memcpy(out, index.data(), need);
    return long(need);
}
long nblic_amd_index_build(nblic_amd_ctx *c, const unsigned char *stream, size_t stream_bytes, int every_rows, unsigned char *out, size_t cap) {
    return index_build(c, stream, stream_bytes, every_rows, out, cap);
}
int nblic_amd_encode_batch_indexed(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                   const int *heights, const int *widths, const int *every_rows, int band_rows,
                                   unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                   unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    return indexed_batch(kIdxNblic, c, n_images, imgs, imgs_on_device != 0, heights, widths, every_rows, band_rows, outs, out_caps, out_lens, indexes, index_caps, index_lens);
}
int nblic_amd_qencode_batch_indexed(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                    const int *heights, const int *widths, const int *every_rows, int band_rows,
                                    uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words,
                                    unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    return indexed_batch(kIdxQnblic, c, n_images, imgs, imgs_on_device != 0, heights, widths, every_rows, band_rows, outs, out_caps_words, out_len_words, indexes, index_caps, index_lens);
}

int nblic_amd_decode_batch_to_ex(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens, const nblic_amd_dest_ex *dests,
                                 int format, int *heights, int *widths, int *nears, int *efforts, int *status) {
    const bool rct = format_rct(format);
    if (rct && (n_images < 0 || n_images % 3 != 0)) return -1;
    const std::vector<uint8_t> modes = rct_modes(rct ? n_images : 0);
    return decode_batch_to_modes(c, n_images, streams, stream_lens, dests, format, rct ? modes.data() : nullptr, heights, widths, nears, efforts, status);
}
int nblic_amd_decode_batch_to_ex_color(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens, const nblic_amd_dest_ex *dests,
                                       int format, const unsigned char *frame_modes, int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!color_modes_ok(n_images, frame_modes)) return -1;
    return decode_batch_to_modes(c, n_images, streams, stream_lens, dests, format, frame_modes, heights, widths, nears, efforts, status);
}

// ---- ENCODE FROM DEVICE MEMORY: the four batch encoders on sources instead of planes ------------------------------------------
// What every _from call starts with: the whole-call refusals, then the sources checked one by one (collect_plan).
// frame_modes: the _color calls' (one valid byte per frame); NULL: none but what NBLIC_AMD_FORMAT_RCT in `format` says.
// stack: the _stack calls' depth and slice modes (StackArg, beside DeliverTo), which do not go with colour frames.
// The near rule of a _stack call: near > 0 only on a key slice whose successor in the stack, if any, is a key slice too (a
// plane off by +-near would wrap in the difference, and would drift along the run).
static bool stack_nears_ok(int n, const StackArg &stack, const int *nears) {
    if (!nears) return true;
    for (int k = 0; k < n; k++) {
        if (nears[k] <= 0) continue;
        if (stack.modes[k] != kStackKey || ((k + 1) % stack.depth != 0 && stack.modes[k + 1] != kStackKey)) return false;
    }
    return true;
}
static bool collect_from_begin(nblic_amd_ctx *c, int n, const nblic_amd_src *srcs, int format, float scale, float bias, CollectFrom &from,
                               const unsigned char *frame_modes = nullptr, const StackArg *stack = nullptr) {
    if (stack) {
        if (frame_modes || format < 0 || format >= int(kCollectFormats) || !stack_modes_ok(n, stack->depth, stack->modes)) return false;
        from.slice_modes.assign(stack->modes, stack->modes + n); from.depth = stack->depth;
    }
    if (frame_modes) {
        if (!color_modes_ok(n, frame_modes)) return false;
        from.modes.assign(frame_modes, frame_modes + n / 3);
    } else if (format_rct(format)) {
        if (n < 0 || n % 3 != 0) return false;
        from.modes = rct_modes(n);
    }
    if (!c || c->broken || n < 0 || !srcs || !deliver_args_ok(format, scale, bias) || hipSetDevice(c->device) != hipSuccess) return false;
    from.srcs = srcs; from.format = uint32_t(format); from.scale = scale; from.bias = bias;
    collect_plan(c, from, n);
    return true;
}

static int encode_batch_modes_from(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                   const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                   unsigned char *const *recons, const unsigned char *frame_modes, const StackArg *stack = nullptr) {
    CollectFrom from{};
    if (stack && (!stack_modes_ok(n_images, stack->depth, stack->modes) || !stack_nears_ok(n_images, *stack, nears))) return -1;
    if (format >= 0 && (format & NBLIC_AMD_FORMAT_RCT) && !frame_modes && nears)         // a difference plane off by +-near wraps to +-255 in R or B
        for (int k = 0; k < n_images; k++) if (nears[k] > 0) return -1;
    if (frame_modes && nears && color_modes_ok(n_images, frame_modes))   // the same, frame by frame: mode 0 has no difference plane
        for (int k = 0; k < n_images; k++) if (nears[k] > 0 && frame_modes[k / 3] != kColorPlain) return -1;
    if (!collect_from_begin(c, n_images, srcs, format, scale, bias, from, frame_modes, stack)) return -1;
    const bool ok = run_batch(c, nblic_amd_ctx::SubmitItem{nullptr, 0, n_images, from.imgs.data(), true, from.hs.data(), from.ws.data(), outs, out_caps, out_lens, nears, efforts, recons, &from});
    if (nothing_outstanding(c)) for (auto &g : c->groups) collect_timing(c, g);       // (nblic_amd_stage_times, as nblic_amd_encode_batch leaves them)
    return ok ? 0 : -1;
}
int nblic_amd_encode_batch_modes_from(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                      const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                      unsigned char *const *recons) {
    return encode_batch_modes_from(c, n_images, srcs, format, scale, bias, nears, efforts, outs, out_caps, out_lens, recons, nullptr);
}
int nblic_amd_encode_batch_modes_from_color(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                            const unsigned char *frame_modes, const int *nears, const int *efforts, unsigned char *const *outs,
                                            const size_t *out_caps, long *out_lens, unsigned char *const *recons) {
    if (!frame_modes || format < 0 || format >= int(kCollectFormats)) return -1;
    return encode_batch_modes_from(c, n_images, srcs, format, scale, bias, nears, efforts, outs, out_caps, out_lens, recons, frame_modes);
}
int nblic_amd_encode_batch_modes_from_to(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                         const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                         const nblic_amd_dest_ex *recons, int recon_format) {
    CollectFrom from{};
    if (!recons || recon_format < 0 || recon_format >= int(kDeliverFormats) || format < 0 || format >= int(kCollectFormats)) return -1;      // (no colour frames here)
    if (!collect_from_begin(c, n_images, srcs, format, scale, bias, from)) return -1;
    const DeliverTo to{recons, uint32_t(recon_format)};
    from.recon_tasks.assign(size_t(n_images), DeliverTask{}); from.recon_ok.assign(size_t(n_images), 0);
    for (int k = 0; k < n_images; k++)                                   // a refused destination costs the reconstruction, not the stream
        from.recon_ok[size_t(k)] = from.how[size_t(k)] != kSrcRefused && recons[k].ptr && deliver_dest_task(c, to, k, from.hs[size_t(k)], from.ws[size_t(k)], from.recon_tasks[size_t(k)]);
    deliver_stats_reset(c);
    const bool ok = run_batch(c, nblic_amd_ctx::SubmitItem{nullptr, 0, n_images, from.imgs.data(), true, from.hs.data(), from.ws.data(), outs, out_caps, out_lens, nears, efforts, nullptr, &from});
    if (nothing_outstanding(c)) for (auto &g : c->groups) collect_timing(c, g);
    return ok ? 0 : -1;
}
static int qencode_batch_from(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                              uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words, const unsigned char *frame_modes,
                              const StackArg *stack = nullptr) {
    CollectFrom from{};
    if (!collect_from_begin(c, n_images, srcs, format, scale, bias, from, frame_modes, stack)) return -1;
    return run_batch(c, nblic_amd_ctx::SubmitItem{nullptr, 1, n_images, from.imgs.data(), true, from.hs.data(), from.ws.data(), reinterpret_cast<unsigned char *const *>(outs),
                                                  out_caps_words, out_len_words, nullptr, nullptr, nullptr, &from}) ? 0 : -1;
}
int nblic_amd_qencode_batch_from(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                 uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words) {
    return qencode_batch_from(c, n_images, srcs, format, scale, bias, outs, out_caps_words, out_len_words, nullptr);
}
int nblic_amd_qencode_batch_from_color(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                       const unsigned char *frame_modes, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words) {
    if (!frame_modes || format < 0 || format >= int(kCollectFormats)) return -1;
    return qencode_batch_from(c, n_images, srcs, format, scale, bias, outs, out_caps_words, out_len_words, frame_modes);
}
extern "C++" template <class Out>
static int indexed_batch_from(const IdxCodec &F, nblic_amd_ctx *c, int n, const nblic_amd_src *srcs, int format, float scale, float bias, const int *every, int band_rows,
                              Out *const *outs, const size_t *caps, long *lens, unsigned char *const *indexes, const size_t *icaps, long *ilens,
                              const unsigned char *frame_modes = nullptr, const StackArg *stack = nullptr) {
    CollectFrom from{};
    if (n < 1 || !collect_from_begin(c, n, srcs, format, scale, bias, from, frame_modes, stack)) return -1;
    return indexed_batch(F, c, n, from.imgs.data(), true, from.hs.data(), from.ws.data(), every, band_rows, outs, caps, lens, indexes, icaps, ilens, &from);
}
int nblic_amd_encode_batch_indexed_from(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                        const int *every_rows, int band_rows, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                        unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    return indexed_batch_from(kIdxNblic, c, n_images, srcs, format, scale, bias, every_rows, band_rows, outs, out_caps, out_lens, indexes, index_caps, index_lens);
}
int nblic_amd_qencode_batch_indexed_from(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                         const int *every_rows, int band_rows, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words,
                                         unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    return indexed_batch_from(kIdxQnblic, c, n_images, srcs, format, scale, bias, every_rows, band_rows, outs, out_caps_words, out_len_words, indexes, index_caps, index_lens);
}

int nblic_amd_encode_batch_indexed_from_color(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                              const unsigned char *frame_modes, const int *every_rows, int band_rows, unsigned char *const *outs,
                                              const size_t *out_caps, long *out_lens, unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    if (!frame_modes || format < 0 || format >= int(kCollectFormats)) return -1;
    return indexed_batch_from(kIdxNblic, c, n_images, srcs, format, scale, bias, every_rows, band_rows, outs, out_caps, out_lens, indexes, index_caps, index_lens, frame_modes);
}
int nblic_amd_qencode_batch_indexed_from_color(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                               const unsigned char *frame_modes, const int *every_rows, int band_rows, uint16_t *const *outs,
                                               const size_t *out_caps_words, long *out_len_words, unsigned char *const *indexes, const size_t *index_caps,
                                               long *index_lens) {
    if (!frame_modes || format < 0 || format >= int(kCollectFormats)) return -1;
    return indexed_batch_from(kIdxQnblic, c, n_images, srcs, format, scale, bias, every_rows, band_rows, outs, out_caps_words, out_len_words, indexes, index_caps, index_lens, frame_modes);
}
// The _stack siblings of the four _from encoders (stack.h): image s * depth + d is slice d of stack s, coded in slice_modes[].
int nblic_amd_encode_batch_modes_from_stack(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                            int depth, const unsigned char *slice_modes, const int *nears, const int *efforts, unsigned char *const *outs,
                                            const size_t *out_caps, long *out_lens, unsigned char *const *recons) {
    const StackArg stack{depth, slice_modes};
    return encode_batch_modes_from(c, n_images, srcs, format, scale, bias, nears, efforts, outs, out_caps, out_lens, recons, nullptr, &stack);
}
int nblic_amd_qencode_batch_from_stack(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                       int depth, const unsigned char *slice_modes, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words) {
    const StackArg stack{depth, slice_modes};
    return qencode_batch_from(c, n_images, srcs, format, scale, bias, outs, out_caps_words, out_len_words, nullptr, &stack);
}
int nblic_amd_encode_batch_indexed_from_stack(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                              int depth, const unsigned char *slice_modes, const int *every_rows, int band_rows, unsigned char *const *outs,
                                              const size_t *out_caps, long *out_lens, unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    const StackArg stack{depth, slice_modes};
    return indexed_batch_from(kIdxNblic, c, n_images, srcs, format, scale, bias, every_rows, band_rows, outs, out_caps, out_lens, indexes, index_caps, index_lens, nullptr, &stack);
}
int nblic_amd_qencode_batch_indexed_from_stack(nblic_amd_ctx *c, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                               int depth, const unsigned char *slice_modes, const int *every_rows, int band_rows, uint16_t *const *outs,
                                               const size_t *out_caps_words, long *out_len_words, unsigned char *const *indexes, const size_t *index_caps,
                                               long *index_lens) {
    const StackArg stack{depth, slice_modes};
    return indexed_batch_from(kIdxQnblic, c, n_images, srcs, format, scale, bias, every_rows, band_rows, outs, out_caps_words, out_len_words, indexes, index_caps, index_lens, nullptr, &stack);
}

long nblic_amd_debug_q_entropy(int height, int width, const uint16_t *words, const unsigned int *hist, const int *entry_rows, int n_entries,
                               uint16_t *out, size_t cap_words, unsigned int *states, unsigned long long *words_emitted) {
    if (!words || !hist || !out || n_entries < 0 || (n_entries > 0 && (!entry_rows || !states || !words_emitted))) return -2;
    if (height < 1 || width < 1 || height > kIndexMaxSide || width > kIndexMaxSide) return -2;
    if (!q_words_ok(words, size_t(height) * size_t(width), hist)) return -2;
    std::vector<QEntryState> at;
    at.resize(size_t(n_entries));
    const long n = q_entropy_encode_entries(out, cap_words, height, width, words, hist, entry_rows, n_entries, at.data());
    for (int k = 0; n >= 0 && k < n_entries; k++) { states[k] = at[size_t(k)].state; words_emitted[k] = at[size_t(k)].words; }
    return n;
}
long nblic_amd_index_bytes(int kind, int height, int width, int effort, int every_rows) { return index_bytes(kind, height, width, effort, every_rows); }
long nblic_amd_indexed_batch_split(nblic_amd_ctx *c, double ms[5]) {
    if (!c || !ms) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    for (int k = 0; k < 5; k++) ms[k] = c->idx_split[k];
    return c->idx_steps;
}
int nblic_amd_decode_indexed(nblic_amd_ctx *c, const unsigned char *stream, size_t stream_bytes, const void *index, size_t index_bytes,
                             unsigned char *img, size_t img_cap) {
    int h, w, near, effort, status;                                      // one image of the batch call, the whole plane
    return decode_batch_indexed(c, 1, &stream, &stream_bytes, &index, &index_bytes, nullptr, nullptr, &img, &img_cap, &h, &w, &near, &effort, &status);
}
int nblic_amd_decode_batch_indexed(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                   const void *const *indexes, const size_t *index_lens, const int *row0, const int *row1,
                                   unsigned char *const *outs, const size_t *out_caps, int *heights, int *widths, int *nears, int *efforts, int *status) {
    return decode_batch_indexed(c, n_images, streams, stream_lens, indexes, index_lens, row0, row1, outs, out_caps, heights, widths, nears, efforts, status);
}
int nblic_amd_decode_batch_indexed_to(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                      const void *const *indexes, const size_t *index_lens, const nblic_amd_dest *dests, int format, float scale, float bias,
                                      int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!dests || n_images < 0 || !deliver_args_ok(format, scale, bias)) return -1;
    const std::vector<nblic_amd_dest_ex> ex = dests_ex(dests, n_images, format, scale, bias);
    return nblic_amd_decode_batch_indexed_to_ex(c, n_images, streams, stream_lens, indexes, index_lens, ex.data(), format, heights, widths, nears, efforts, status);
}
int nblic_amd_decode_batch_indexed_to_ex(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                         const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                         int *heights, int *widths, int *nears, int *efforts, int *status) {
    const bool rct = format_rct(format);
    if (!dests || format < 0 || format >= int(kDeliverFormats) || (rct && (n_images < 0 || n_images % 3 != 0))) return -1;
    const std::vector<uint8_t> modes = rct_modes(rct ? n_images : 0);
    const DeliverTo to{dests, uint32_t(format), rct ? modes.data() : nullptr};
    deliver_stats_reset(c);
    return decode_batch_indexed(c, n_images, streams, stream_lens, indexes, index_lens, nullptr, nullptr, nullptr, nullptr, heights, widths, nears, efforts, status, &to);
}
// The _stack siblings of the two _to_ex decoders (stack.h).
int nblic_amd_decode_batch_to_ex_stack(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens, const nblic_amd_dest_ex *dests,
                                       int format, int depth, const unsigned char *slice_modes, int *heights, int *widths, int *nears, int *efforts, int *status) {
    const StackArg stack{depth, slice_modes};
    return decode_batch_to_modes(c, n_images, streams, stream_lens, dests, format, nullptr, heights, widths, nears, efforts, status, &stack);
}
int nblic_amd_decode_batch_indexed_to_ex_stack(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                               const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                               int depth, const unsigned char *slice_modes, int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!dests || format < 0 || format >= int(kDeliverFormats) || !stack_modes_ok(n_images, depth, slice_modes)) return -1;
    DeliverTo to{dests, uint32_t(format)};
    to.slice_modes = slice_modes; to.depth = depth;
    deliver_stats_reset(c);
    return decode_batch_indexed(c, n_images, streams, stream_lens, indexes, index_lens, nullptr, nullptr, nullptr, nullptr, heights, widths, nears, efforts, status, &to);
}
int nblic_amd_decode_batch_indexed_to_ex_color(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                               const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                               const unsigned char *frame_modes, int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!dests || format < 0 || format >= int(kDeliverFormats) || !color_modes_ok(n_images, frame_modes)) return -1;
    const DeliverTo to{dests, uint32_t(format), frame_modes};
    deliver_stats_reset(c);
    return decode_batch_indexed(c, n_images, streams, stream_lens, indexes, index_lens, nullptr, nullptr, nullptr, nullptr, heights, widths, nears, efforts, status, &to);
}
// ---- DEEP PIXELS: 16-bit images as a high and a (folded) low plane (deep.h) ------------------------------------------------------
// A deep source as the checks see it: an image the encoders take, deep.h's rules, and device memory of this context's device.
static bool deep_src_ok(const nblic_amd_ctx *c, const nblic_amd_src &S, int deep_format) {
    if (!size_ok(S.rows, S.cols, c->max_px) || S.step_bytes > kCollectMaxStep) return false;
    if (!deep_source_ok(static_cast<const uint8_t *>(S.ptr), S.pitch_bytes, S.step_bytes, uint32_t(S.rows), uint32_t(S.cols), uint32_t(deep_format), S.cap_bytes)) return false;
    return device_range_ok(c, S.ptr, deep_src_extent(uint32_t(S.rows), uint32_t(S.cols), S.pitch_bytes, S.step_bytes));
}
static bool deep_modes_ok(int n_deep, const unsigned char *modes, int deep_format) {          // valid bytes whose bit 1 is the source format's
    if (n_deep < 0 || !modes || deep_format < 0 || deep_format >= int(kDeepSrcFormats)) return false;
    for (int i = 0; i < n_deep; i++)
        if (!deep_mode_valid(modes[i]) || ((modes[i] & kDeepSigned) != 0) != (deep_format == int(kDeepI16))) return false;
    return true;
}

// ONE k_deep_cost launch over the tasks, queued on st (cost_queue).  The sums are the caller's to set.
static bool deep_cost_queue(nblic_amd_ctx *c, DeepCostTask *tasks, size_t n, DeepCostTask *d_tasks, hipStream_t st) {
    return cost_queue(tasks, n, d_tasks, st, deep_task_tiles, [&] { c->deep_counts[0] += 1; c->deep_counts[3] += long(n); },
                      [&](const DeepCostTask *d, int m, uint32_t tiles) { return deep_cost_launch(d, m, tiles, st); });
}
// What the sums of n tasks hold before a launch: zero costs, the largest u as the minimum, zero as the maximum.
static std::vector<unsigned long long> deep_sums_initial(size_t n) {
    std::vector<unsigned long long> v(n * kDeepSums, 0ull);
    for (size_t i = 0; i < n; i++) v[i * kDeepSums + 3] = 0xFFFFull;
    return v;
}

int nblic_amd_deep_plan(nblic_amd_ctx *c, int n_deep, const nblic_amd_src *srcs, int deep_format, unsigned char *modes, unsigned long long *costs,
                        unsigned int *ranges) {
    if (!c || c->broken || n_deep < 0 || !srcs || !modes || deep_format < 0 || deep_format >= int(kDeepSrcFormats) || hipSetDevice(c->device) != hipSuccess) return -1;
    std::lock_guard<std::mutex> g(c->api);
    const size_t count = size_t(n_deep);
    std::vector<DeepCostTask> tasks;
    std::vector<size_t> image_of;
    for (size_t i = 0; i < count; i++) {                                 // a refused source: 0xFF, and nothing is launched for it
        modes[i] = uint8_t(kDeepRefused);
        if (costs) costs[3 * i] = costs[3 * i + 1] = costs[3 * i + 2] = 0;
        if (ranges) ranges[2 * i] = ranges[2 * i + 1] = 0;
        const nblic_amd_src &S = srcs[i];
        if (!deep_src_ok(c, S, deep_format)) continue;
        DeepCostTask T{};
        T.src = static_cast<const uint8_t *>(S.ptr); T.pitch = S.pitch_bytes; T.step = uint32_t(S.step_bytes);
        T.rows = uint32_t(S.rows); T.cols = uint32_t(S.cols); T.format = uint32_t(deep_format);
        tasks.push_back(T); image_of.push_back(i);
    }
    if (tasks.empty()) return 0;
    const size_t m = tasks.size();
    std::vector<unsigned long long> sums = deep_sums_initial(m);
    SumsRun run;
    DeepCostTask *d_tasks = run.begin(sums.size()) ? run.mem.make<DeepCostTask>(m) : nullptr;
    if (!d_tasks) return -1;
    for (size_t i = 0; i < m; i++) tasks[i].sums = run.d_sums + i * kDeepSums;
    if (!run.run(c, sums, &c->deep_ms[0], [&](hipStream_t st) { return deep_cost_queue(c, tasks.data(), m, d_tasks, st); })) return -1;
    for (size_t i = 0; i < m; i++) {
        const size_t k = image_of[i];
        const unsigned long long *s = &sums[i * kDeepSums];
        modes[k] = deep_choose(s, uint32_t(deep_format));
        if (costs) { costs[3 * k] = s[0]; costs[3 * k + 1] = s[1]; costs[3 * k + 2] = s[2]; }
        if (ranges) { ranges[2 * k] = uint32_t(s[3]); ranges[2 * k + 1] = uint32_t(s[4]); }
    }
    return 0;
}
int nblic_amd_deep_choose(const unsigned long long *costs, int deep_format) {
    return !costs || deep_format < 0 || deep_format >= int(kDeepSrcFormats) ? -1 : int(deep_choose(costs, uint32_t(deep_format)));
}
int nblic_amd_deep_mode_valid(int mode) { return mode >= 0 && mode < 256 && deep_mode_valid(uint32_t(mode)) ? 1 : 0; }
int nblic_amd_deep_plan_stats(nblic_amd_ctx *c, long out[4], double *last_ms) {
    if (!c || !out) return -1;
    for (int k = 0; k < 4; k++) out[k] = c->deep_counts[k].load();
    if (last_ms) { std::lock_guard<std::mutex> l(c->stat_m); for (int k = 0; k < 3; k++) last_ms[k] = c->deep_ms[k]; }
    return 0;
}

// The planes of a _from_deep call: ONE k_collect_deep launch writes both planes of every accepted image into a block of the
// call's own, and the parent encoder takes them from there IN PLACE as 2 * n_deep uint8 sources (streams 2i and 2i + 1) -- the
// block stands where the planes that the groups would collect into stand for any other source.  A refused image becomes two
// sources that the parent refuses.  false: the whole call is refused, nothing was launched.
struct DeepPlanes { DevPool mem; std::vector<nblic_amd_src> srcs; };
static bool deep_collect(nblic_amd_ctx *c, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes, DeepPlanes &P) {
    if (!c || c->broken || !srcs || n_deep > (1 << 29) || !deep_modes_ok(n_deep, modes, deep_format) || hipSetDevice(c->device) != hipSuccess) return false;
    const size_t count = size_t(n_deep);
    P.srcs.assign(2 * count, nblic_amd_src{nullptr, 0, 0, 0, 0, 0});
    std::vector<DeepCollectTask> tasks;
    std::vector<size_t> at;
    size_t total = 0;
    unsigned long long chunks = 0;
    for (size_t i = 0; i < count; i++) {
        const nblic_amd_src &S = srcs[i];
        if (!deep_src_ok(c, S, deep_format)) continue;
        const size_t plane = size_t(S.rows) * size_t(S.cols);
        for (uint32_t part : {uint32_t(kDeepHigh), (modes[i] & kDeepFold) ? uint32_t(kDeepLowFolded) : uint32_t(kDeepLow)}) {
            DeepCollectTask T{};
            T.src = static_cast<const uint8_t *>(S.ptr); T.pitch = S.pitch_bytes; T.step = uint32_t(S.step_bytes);
            T.rows = uint32_t(S.rows); T.cols = uint32_t(S.cols); T.px0 = 0; T.px1 = T.rows * T.cols;
            T.format = uint32_t(deep_format); T.part = part;
            T.first_chunk = uint32_t(chunks); chunks += deep_collect_chunks(T);
            tasks.push_back(T); at.push_back(total); total += up256(plane);
        }
        for (size_t j = 2 * i; j < 2 * i + 2; j++) P.srcs[j] = nblic_amd_src{nullptr, size_t(S.cols), 1, plane, S.rows, S.cols};
    }
    if (tasks.empty()) return true;
    if (chunks >= (1ull << 31)) return false;
    Stream st;
    Event marks[2];
    uint8_t *d_planes = P.mem.make<uint8_t>(total);
    DeepCollectTask *d_tasks = P.mem.make<DeepCollectTask>(tasks.size());
    if (!d_planes || !d_tasks || st.create(hipStreamNonBlocking) != hipSuccess || marks[0].create(hipEventDefault) != hipSuccess || marks[1].create(hipEventDefault) != hipSuccess) return false;
    size_t t = 0;
    for (size_t j = 0; j < 2 * count; j++) {
        if (!P.srcs[j].rows) continue;
        tasks[t].dst = d_planes + at[t];
        P.srcs[j].ptr = tasks[t].dst;
        t++;
    }
    const bool ok = [&]() -> bool {
        HIP_OK(hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(DeepCollectTask), hipMemcpyHostToDevice, st));
        c->deep_counts[1] += 1;
        HIP_OK(hipEventRecord(marks[0], st));
        if (!collect_deep_launch(d_tasks, int(tasks.size()), uint32_t(chunks), st)) return false;
        HIP_OK(hipEventRecord(marks[1], st));
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }();
    if (st) hipStreamSynchronize(st);
    if (ok) deep_timed(c, marks, 1);
    return ok;
}
// The near rule of a _deep call: the high plane is lossless.
static bool deep_nears_ok(int n_deep, const int *nears) {
    for (int i = 0; nears && i < n_deep; i++) if (nears[2 * i] != 0) return false;
    return true;
}

// The _deep siblings of the four _from encoders: streams 2i and 2i + 1 are the high and the low plane of deep image i.
int nblic_amd_encode_batch_modes_from_deep(nblic_amd_ctx *c, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                           const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                           unsigned char *const *recons) {
    DeepPlanes P;
    if (!outs || !out_caps || !out_lens || n_deep < 0 || !deep_nears_ok(n_deep, nears) || !deep_collect(c, n_deep, srcs, deep_format, modes, P)) return -1;
    return encode_batch_modes_from(c, 2 * n_deep, P.srcs.data(), int(kCollectU8), 1.0f, 0.0f, nears, efforts, outs, out_caps, out_lens, recons, nullptr);
}
int nblic_amd_qencode_batch_from_deep(nblic_amd_ctx *c, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                      uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words) {
    DeepPlanes P;
    if (!outs || !out_caps_words || !out_len_words || n_deep < 0 || !deep_collect(c, n_deep, srcs, deep_format, modes, P)) return -1;
    return qencode_batch_from(c, 2 * n_deep, P.srcs.data(), int(kCollectU8), 1.0f, 0.0f, outs, out_caps_words, out_len_words, nullptr);
}
int nblic_amd_encode_batch_indexed_from_deep(nblic_amd_ctx *c, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                             const int *every_rows, int band_rows, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                             unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    DeepPlanes P;
    if (!every_rows || !outs || !out_caps || !out_lens || !indexes || !index_caps || !index_lens || n_deep < 1 || !deep_collect(c, n_deep, srcs, deep_format, modes, P)) return -1;
    return indexed_batch_from(kIdxNblic, c, 2 * n_deep, P.srcs.data(), int(kCollectU8), 1.0f, 0.0f, every_rows, band_rows, outs, out_caps, out_lens, indexes, index_caps, index_lens);
}
int nblic_amd_qencode_batch_indexed_from_deep(nblic_amd_ctx *c, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                              const int *every_rows, int band_rows, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words,
                                              unsigned char *const *indexes, const size_t *index_caps, long *index_lens) {
    DeepPlanes P;
    if (!every_rows || !outs || !out_caps_words || !out_len_words || !indexes || !index_caps || !index_lens || n_deep < 1 || !deep_collect(c, n_deep, srcs, deep_format, modes, P)) return -1;
    return indexed_batch_from(kIdxQnblic, c, 2 * n_deep, P.srcs.data(), int(kCollectU8), 1.0f, 0.0f, every_rows, band_rows, outs, out_caps_words, out_len_words, indexes, index_caps, index_lens);
}

// The _deep siblings of the two _to_ex decoders: 2 * n_deep streams, n_deep destinations and mode bytes.
static bool deep_to_ok(int n_deep, const nblic_amd_dest_ex *dests, int format, const unsigned char *modes) {
    if (n_deep < 0 || n_deep > (1 << 29) || !dests || !modes || format < 0 || format >= int(kDeepDestFormats)) return false;
    for (int i = 0; i < n_deep; i++) if (!deep_mode_valid(modes[i])) return false;
    return true;
}
int nblic_amd_decode_batch_to_ex_deep(nblic_amd_ctx *c, int n_deep, const unsigned char *const *streams, const size_t *stream_lens, const nblic_amd_dest_ex *dests,
                                      int format, const unsigned char *modes, int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!c || c->broken || !streams || !stream_lens || !heights || !widths || !nears || !efforts || !status || !deep_to_ok(n_deep, dests, format, modes)) return -1;
    const int n = 2 * n_deep;
    for (int k = 0; k < n; k++) if (!streams[k]) return -1;
    DeliverTo to{dests, 0u};
    to.deep_modes = modes; to.deep_format = uint32_t(format);
    std::lock_guard<std::mutex> g(c->api);
    if (!decode_batch(c, n, streams, stream_lens, nullptr, nullptr, heights, widths, nears, efforts, status, &to)) return -1;
    for (int k = 0; k < n; k++) if (status[k] != 0) return -1;
    return 0;
}
int nblic_amd_decode_batch_indexed_to_ex_deep(nblic_amd_ctx *c, int n_deep, const unsigned char *const *streams, const size_t *stream_lens,
                                              const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                              const unsigned char *modes, int *heights, int *widths, int *nears, int *efforts, int *status) {
    if (!deep_to_ok(n_deep, dests, format, modes)) return -1;
    DeliverTo to{dests, 0u};
    to.deep_modes = modes; to.deep_format = uint32_t(format);
    return decode_batch_indexed(c, 2 * n_deep, streams, stream_lens, indexes, index_lens, nullptr, nullptr, nullptr, nullptr, heights, widths, nears, efforts, status, &to);
}

// ---- the three deep kernels on caller-made inputs, and their host walks (tests/test_deep_host.py, tests/test_deep_kernels.py) ----
static bool debug_deep_collect_task(DeepCollectTask &T, int rows, int cols, size_t pitch, size_t step, int deep_format, int part, const int *range) {
    if (rows < 1 || cols < 1 || rows > int(kCollectMaxSide) || cols > int(kCollectMaxSide) || step > kCollectMaxStep || deep_format < 0 || part < 0) return false;
    T = DeepCollectTask{};
    T.pitch = pitch; T.step = uint32_t(step); T.rows = uint32_t(rows); T.cols = uint32_t(cols);
    T.px0 = range ? uint32_t(range[0]) : 0u; T.px1 = range && range[1] ? uint32_t(range[1]) : T.rows * T.cols;
    T.format = uint32_t(deep_format); T.part = uint32_t(part);
    return !range || (range[0] >= 0 && range[1] >= 0);
}
// Host only: the shared unit walk (deep.h deep_collect_host) over the source at src -- cap_bytes readable from there -- into
// the plane at out, which must be a multiple of 16 and hold rows x cols bytes.  range: the pixels [px0, px1) of the flat plane
// (NULL: all of it; px1 == 0: to the end).  -1: refused.
int nblic_amd_debug_deep_collect_host(const void *src, size_t cap_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int deep_format, int part,
                                      const int *range, unsigned char *out, size_t out_bytes, unsigned long long *units, unsigned long long *chunks) {
    DeepCollectTask T;
    if (!src || !out || !debug_deep_collect_task(T, rows, cols, pitch_bytes, step_bytes, deep_format, part, range)) return -1;
    T.src = static_cast<const uint8_t *>(src); T.dst = out;
    if (!deep_collect_task_ok(T, cap_bytes) || size_t(T.rows) * size_t(T.cols) > out_bytes) return -1;
    if (units) *units = deep_collect_units(T);
    if (chunks) *chunks = deep_collect_chunks(T);
    deep_collect_host(T);
    return 0;
}
// ONE k_collect_deep launch over n caller-made sources as n tasks, laid out as nblic_amd_debug_collect lays its own out: the
// bytes of source k at byte base_offsets[k] (0 .. 255) of a region filled with 0xFF that is larger, plane k at byte 256 of a
// region filled with 0x5A, which comes back whole in outs[k]: out_bytes[k] = 256 + up256(rows x cols) + 256.
int nblic_amd_debug_deep_collect(nblic_amd_ctx *c, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets, const int *rows,
                                 const int *cols, const size_t *pitches, const size_t *steps, const int *deep_formats, const int *parts, const int *ranges,
                                 unsigned char *const *outs, const size_t *out_bytes) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !srcs || !src_bytes || !base_offsets || !rows || !cols || !pitches || !steps || !deep_formats || !parts || !outs || !out_bytes) return -1;
    const size_t count = size_t(n);
    std::vector<DeepCollectTask> tasks(count);
    DebugBench bench;
    for (int k = 0; k < n; k++) {
        const size_t i = size_t(k);
        if (!srcs[k] || !outs[k] || base_offsets[k] > 255 || src_bytes[k] > (size_t(1) << 30) ||
            !debug_deep_collect_task(tasks[i], rows[k], cols[k], pitches[k], steps[k], deep_formats[k], parts[k], ranges ? ranges + 2 * i : nullptr)) return -1;
        if (!debug_plane_out_ok(rows[k], cols[k], out_bytes[k])) return -1;
        bench.source(srcs[k], src_bytes[k], base_offsets[k]);
        bench.output(outs[k], out_bytes[k]);
    }
    DeepCollectTask *d_tasks = bench.alloc(c->device) ? bench.table<DeepCollectTask>(count) : nullptr;
    if (!d_tasks) return -2;
    unsigned long long chunks = 0;
    for (size_t i = 0; i < count; i++) {                                 // the addresses are known now: the rest of the checks
        DeepCollectTask &T = tasks[i];
        T.src = bench.in(i);
        T.dst = bench.out(i) + DebugBench::kGuard;
        if (!deep_collect_task_ok(T, src_bytes[i])) return -1;           // nothing outside the uploaded bytes is the task's to read
        T.first_chunk = uint32_t(chunks); chunks += deep_collect_chunks(T);
    }
    if (chunks >= (1ull << 31)) return -1;
    return bench.run([&](hipStream_t st) {
        if (hipMemcpyAsync(d_tasks, tasks.data(), count * sizeof(DeepCollectTask), hipMemcpyHostToDevice, st) != hipSuccess) return false;
        c->deep_counts[1] += 1;
        return collect_deep_launch(d_tasks, n, uint32_t(chunks), st);
    });
}

// A debug deep delivery's task: all but the addresses.  window: row0, row1, col0, col1 of planes of plane_rows x width.
static bool debug_deep_deliver_task(DeepDeliverTask &T, int plane_rows, int width, const int *window, int format, int mode, float scale, float bias, int zero,
                                    size_t pitch, size_t step) {
    if (plane_rows < 1 || width < 1 || !window || format < 0 || format >= int(kDeepDestFormats) || mode < 0 || mode > 255 || step > kDeliverMaxStep || pitch > (size_t(1) << 40)) return false;
    if (window[0] < 0 || window[1] <= window[0] || window[1] > plane_rows || window[2] < 0 || window[3] <= window[2] || window[3] > width) return false;
    T = DeepDeliverTask{};
    T.src_pitch = uint32_t(width); T.rows = uint32_t(window[1] - window[0]); T.col0 = uint32_t(window[2]); T.col1 = uint32_t(window[3]);
    T.format = uint32_t(format); T.mode = uint32_t(mode); T.scale = scale; T.bias = bias; T.zero = zero ? 1u : 0u;
    T.dst_pitch = pitch; T.dst_step = step ? uint32_t(step) : deep_dest_elem(T.format);
    return true;
}
// Host only: the shared unit walk (deep.h deep_deliver_host) over the caller's two planes of plane_rows x width bytes into
// out + dst_offset.  The unit grid follows the destination's address as the kernel's does.  gate_status: two ints, the
// statuses of the high and the low plane's gate records (-1: none).  step_bytes 0 stands for the element size.
int nblic_amd_debug_deep_deliver_host(const unsigned char *hi, const unsigned char *lo, int plane_rows, int width, const int *window, int format, int mode,
                                      float scale, float bias, int zero, const int *gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset,
                                      size_t pitch_bytes, size_t step_bytes, unsigned long long *units, unsigned long long *chunks) {
    DeepDeliverTask T;
    if (!hi || !lo || !out || !gate_status || !debug_deep_deliver_task(T, plane_rows, width, window, format, mode, scale, bias, zero, pitch_bytes, step_bytes)) return -1;
    const size_t skip = size_t(window[0]) * size_t(width), bytes = size_t(plane_rows) * size_t(width) - skip;
    T.hi = hi + skip; T.lo = lo + skip; T.hi_bytes = T.lo_bytes = bytes;
    T.dst = out + dst_offset;
    if (dst_offset > out_bytes || !deep_deliver_task_ok(T)) return -1;
    if (deep_dest_extent(T.rows, T.col1 - T.col0, T.format, T.dst_pitch, T.dst_step) > out_bytes - dst_offset) return -1;
    if (units) *units = deep_deliver_units(T);
    if (chunks) *chunks = deep_deliver_chunks(T);
    deep_deliver_host(T, gate_status[0] == -1 ? int(kDone) : gate_status[0], gate_status[1] == -1 ? int(kDone) : gate_status[1]);
    return 0;
}
// ONE k_deliver_deep launch over n caller-made plane pairs as n tasks, laid out as nblic_amd_debug_deliver lays its own out:
// a plane at byte base_offsets[] (0 .. 15; two entries per task: high, low) of a zeroed region of its own that may be read
// for up256(rows * width) bytes, destination k at byte dst_offsets[k] of a buffer of out_bytes[k] bytes filled with 0x5A, which
// comes back whole in outs[k]; gate_status: two ints per task.
int nblic_amd_debug_deep_deliver(nblic_amd_ctx *c, int n, const unsigned char *const *his, const unsigned char *const *los, const size_t *base_offsets,
                                 const int *plane_rows, const int *widths, const int *windows, const int *formats, const int *modes, const float *scales,
                                 const float *biases, const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets,
                                 const size_t *out_bytes, unsigned char *const *outs, const int *gate_status) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !his || !los || !base_offsets || !plane_rows || !widths || !windows || !formats || !modes || !scales || !biases ||
        !zeros || !pitches || !steps || !dst_offsets || !out_bytes || !outs || !gate_status) return -1;
    const size_t count = size_t(n);
    std::vector<DeepDeliverTask> tasks(count);
    std::vector<size_t> plane_len(count);
    DebugBench bench;
    for (int k = 0; k < n; k++) {
        const size_t i = size_t(k);
        if (!his[k] || !los[k] || !outs[k] || base_offsets[2 * i] > 15 || base_offsets[2 * i + 1] > 15 ||
            !debug_deep_deliver_task(tasks[i], plane_rows[k], widths[k], windows + 4 * i, formats[k], modes[k], scales[k], biases[k], zeros[k], pitches[k], steps[k])) return -1;
        plane_len[i] = size_t(plane_rows[k]) * size_t(widths[k]);
        if (plane_len[i] > (size_t(1) << 30) || out_bytes[k] > (size_t(1) << 30) || dst_offsets[k] > out_bytes[k]) return -1;
        bench.plane(his[k], plane_len[i], base_offsets[2 * i]);          // inputs 2 i and 2 i + 1
        bench.plane(los[k], plane_len[i], base_offsets[2 * i + 1]);
        bench.output(outs[k], out_bytes[k]);
    }
    bench.gates(gate_status, 2 * count);
    DeepDeliverTask *d_tasks = bench.alloc(c->device) ? bench.table<DeepDeliverTask>(count) : nullptr;
    if (!d_tasks) return -2;
    for (int k = 0; k < n; k++) {                                        // the addresses are known now: the rest of the checks
        const size_t i = size_t(k);
        DeepDeliverTask &T = tasks[i];
        const size_t skip = size_t(windows[4 * i]) * size_t(widths[k]);
        T.hi = bench.in(2 * i) + skip; T.lo = bench.in(2 * i + 1) + skip;
        T.hi_bytes = T.lo_bytes = up256(plane_len[i]) - skip;
        T.dst = bench.out(i) + dst_offsets[k];
        if (gate_status[2 * i] != -1) T.gate_hi = bench.gate(2 * i);
        if (gate_status[2 * i + 1] != -1) T.gate_lo = bench.gate(2 * i + 1);
        if (!deep_deliver_task_ok(T) || deep_dest_extent(T.rows, T.col1 - T.col0, T.format, T.dst_pitch, T.dst_step) > out_bytes[k] - dst_offsets[k]) return -1;
    }
    return bench.run([&](hipStream_t st) { return deliver_deep_queue(c, tasks.data(), count, d_tasks, st); });
}

static bool debug_deep_cost_task(DeepCostTask &T, int rows, int cols, size_t pitch, size_t step, int deep_format) {
    if (rows < 1 || cols < 1 || rows > int(kCollectMaxSide) || cols > int(kCollectMaxSide) || step > kCollectMaxStep || deep_format < 0) return false;
    T = DeepCostTask{};
    T.pitch = pitch; T.step = uint32_t(step); T.rows = uint32_t(rows); T.cols = uint32_t(cols); T.format = uint32_t(deep_format);
    return true;
}
// Host only: the shared tile walk (deep.h deep_cost_host) over ONE source, cap_bytes readable from src.  sums: the costs of
// the high, the low and the folded low plane, then min and max of u; tiles (may be NULL): the kernel's workgroups.
int nblic_amd_debug_deep_cost_host(const void *src, size_t cap_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int deep_format,
                                   unsigned long long *sums, unsigned long long *tiles) {
    DeepCostTask T;
    if (!src || !sums || !debug_deep_cost_task(T, rows, cols, pitch_bytes, step_bytes, deep_format)) return -1;
    T.src = static_cast<const uint8_t *>(src); T.sums = sums;
    if (!deep_cost_task_ok(T, cap_bytes)) return -1;
    if (tiles) *tiles = deep_task_tiles(T);
    const std::vector<unsigned long long> init = deep_sums_initial(1);
    memcpy(sums, init.data(), kDeepSums * sizeof(unsigned long long));
    deep_cost_host(T);
    return 0;
}
// ONE k_deep_cost launch over n caller-made sources as n tasks, each uploaded at byte base_offsets[k] (0 .. 255) of a region
// of its own filled with 0xFF that is larger.  sums: five numbers per task.
int nblic_amd_debug_deep_cost(nblic_amd_ctx *c, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets, const int *rows,
                              const int *cols, const size_t *pitches, const size_t *steps, const int *deep_formats, unsigned long long *sums) {
    constexpr int kMaxTasks = 65536;
    if (!c || n < 1 || n > kMaxTasks || !srcs || !src_bytes || !base_offsets || !rows || !cols || !pitches || !steps || !deep_formats || !sums) return -1;
    const size_t count = size_t(n);
    std::vector<DeepCostTask> tasks(count);
    DebugBench bench;
    for (size_t i = 0; i < count; i++) {
        if (!srcs[i] || base_offsets[i] > 255 || src_bytes[i] > (size_t(1) << 30) || !debug_deep_cost_task(tasks[i], rows[i], cols[i], pitches[i], steps[i], deep_formats[i])) return -1;
        bench.source(srcs[i], src_bytes[i], base_offsets[i]);
    }
    const std::vector<unsigned long long> init = deep_sums_initial(count);
    bench.output(sums, init.size() * sizeof(unsigned long long), 0);
    DeepCostTask *d_tasks = bench.alloc(c->device) ? bench.table<DeepCostTask>(count) : nullptr;
    if (!d_tasks) return -2;
    unsigned long long *d_sums = reinterpret_cast<unsigned long long *>(bench.out(0));
    for (size_t i = 0; i < count; i++) {                                 // the addresses are known now: the rest of the checks
        tasks[i].src = bench.in(i); tasks[i].sums = d_sums + i * kDeepSums;
        if (!deep_cost_task_ok(tasks[i], src_bytes[i])) return -1;       // nothing outside the uploaded bytes is the task's to read
    }
    return bench.run([&](hipStream_t st) {
        return hipMemcpyAsync(d_sums, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st) == hipSuccess &&
               deep_cost_queue(c, tasks.data(), count, d_tasks, st);
    });
}

int nblic_amd_indexed_decode_split(nblic_amd_ctx *c, double ms[4]) {
    if (!c || !ms) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    for (int k = 0; k < 4; k++) ms[k] = c->idxdec_split[k];
    return 0;
}
long nblic_amd_indexed_decode_plan(int n_images, const int *kinds, const int *efforts, const int *heights, const int *widths, const int *every_rows,
                                   const int *row0, const int *row1, int round_segments, int *jobs, size_t jobs_cap) {
    if (n_images < 1 || !kinds || !efforts || !heights || !widths || !every_rows || (row0 == nullptr) != (row1 == nullptr)) return -1;
    std::vector<IndexedPlanImage> im;
    for (int k = 0; k < n_images; k++)
        im.push_back(IndexedPlanImage{kinds[k], efforts[k], heights[k], widths[k], every_rows[k], row0 ? row0[k] : 0, row1 ? row1[k] : heights[k]});
    std::vector<IndexedJob> plan;
    if (!indexed_decode_plan(im.data(), n_images, round_segments, plan)) return -1;
    if (jobs && jobs_cap >= plan.size())
        for (size_t j = 0; j < plan.size(); j++) {
            const IndexedJob &P = plan[j];
            const int v[6] = {P.image, P.segment, P.first_row, P.end_row, P.cls, P.round};
            memcpy(jobs + 6 * j, v, sizeof v);
        }
    return long(plan.size());
}
int nblic_amd_index_build_batch(nblic_amd_ctx *c, int n_images, const unsigned char *const *streams, const size_t *stream_lens, const int *every_rows,
                                unsigned char *const *indexes, const size_t *index_caps, long *index_lens, unsigned char *const *planes,
                                const size_t *plane_caps, int *heights, int *widths, int *nears, int *efforts, int *status) {
    return index_build_batch(c, n_images, streams, stream_lens, every_rows, indexes, index_caps, index_lens, planes, plane_caps, heights, widths, nears, efforts, status);
}
int nblic_amd_index_build_split(nblic_amd_ctx *c, double ms[4]) {
    if (!c || !ms) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    for (int k = 0; k < 4; k++) ms[k] = c->idxbuild_split[k];
    return 0;
}
long nblic_amd_index_build_plan(int n_images, const int *kinds, const int *efforts, const int *heights, const int *widths, const int *every_rows,
                                int serial_rows, int *class_launches, int *entries, size_t entries_cap) {
    if (n_images < 1 || !kinds || !efforts || !heights || !widths || !every_rows || serial_rows < 0) return -1;
    std::vector<BuildPlanImage> im;
    for (int k = 0; k < n_images; k++) {
        if (index_bytes(kinds[k], heights[k], widths[k], efforts[k], every_rows[k]) < 0) return -1;
        const DecodeItem it{k, heights[k], widths[k], 0, kMinKStep, efforts[k], kinds[k], 0, -1, -1};
        im.push_back(BuildPlanImage{kinds[k], efforts[k], heights[k], widths[k], every_rows[k], rows_per_launch(it, serial_rows)});
    }
    BuildPlan plan;
    if (!index_build_plan(im.data(), n_images, plan)) return -1;
    if (class_launches) memcpy(class_launches, plan.launches, sizeof plan.launches);
    if (entries && entries_cap >= plan.entries.size())
        for (size_t j = 0; j < plan.entries.size(); j++) {
            const BuildEntry &E = plan.entries[j];
            const int v[4] = {E.image, E.row, E.cls, E.launch};
            memcpy(entries + 4 * j, v, sizeof v);
        }
    return long(plan.entries.size());
}
int nblic_amd_decode_rows(nblic_amd_ctx *c, const unsigned char *stream, size_t stream_bytes, const void *index, size_t index_bytes, int row0,
                          int row1, unsigned char *out, size_t cap) {
    int h, w, near, effort, status;                                      // one image of the batch call, one range
    return decode_batch_indexed(c, 1, &stream, &stream_bytes, &index, &index_bytes, &row0, &row1, &out, &cap, &h, &w, &near, &effort, &status);
}

int nblic_amd_set_device_coder(nblic_amd_ctx *c, int n_packs, int min_outstanding) {
    if (!c || n_packs < 0 || n_packs > 64) return -1;
    std::lock_guard<std::mutex> g(c->api);
    { std::lock_guard<std::mutex> l(c->rm); c->dev_min_outstanding = min_outstanding > 0 ? min_outstanding : 0; }
    while (int(c->dev_coders.size()) < n_packs) c->dev_coders.emplace_back(dev_coder_main, c, int(c->dev_coders.size()));
    return int(c->dev_coders.size());
}

void nblic_amd_device_coder_stats(nblic_amd_ctx *c, double *bins, long *packs, long *images) {
    std::lock_guard<std::mutex> l(c->stat_m);
    if (bins) *bins = c->dev_bins;
    if (packs) *packs = c->dev_packs;
    if (images) *images = c->dev_images;
}

int nblic_amd_serial_selftest(nblic_amd_ctx *c) {
    if (!c || hipSetDevice(c->device) != hipSuccess) return -1;
    return serial_selftest(c->dec_stream);
}

int nblic_amd_serial_plan(int decode, int effort, int images, int width, int whole_streams) {
    if (images < 1 || width < 1 || effort < 0 || effort > 3 || (effort == 0 && !decode)) return -1;
    if (effort == 0) return serial_qdecode_plan(width);
    return decode ? serial_decode_plan(images, width, whole_streams != 0) : serial_model_plan(effort, images, width);
}

int nblic_amd_lsq_probe(nblic_amd_ctx *c, int n, int waves, int count, const double *stats, const signed char *regressors, const int *bias,
                        double *out_f64, long long *out_i64) {
    if (!c || !stats || !regressors || !bias || !out_f64 || !out_i64 || hipSetDevice(c->device) != hipSuccess) return -1;
    std::lock_guard<std::mutex> g(c->api);
    return serial_lsq_probe(c->dec_stream, n, waves, count, stats, reinterpret_cast<const int8_t *>(regressors), bias, out_f64, out_i64) ? 0 : -1;
}

// ---- the device rANS stage of effort 0 (q_device_coder.hip) on its own ----------------------------------------------------
int nblic_amd_set_device_qcoder(nblic_amd_ctx *c, int mode, long symbols_per_launch) {
    if (!c) c = default_ctx();
    if (!c || mode < 0 || mode > 2 || symbols_per_launch < 0) return -1;
    std::lock_guard<std::mutex> g(c->api);
    if (mode != 0 && !c->qdev.joinable()) c->qdev = std::thread(qdev_main, c);
    {
        std::lock_guard<std::mutex> l(c->rm);
        c->qmode = mode;
        c->q_budget = symbols_per_launch == 0 ? kQSymbolsPerLaunch : uint32_t(std::min<long>(symbols_per_launch, 1L << 30));
    }
    c->rcv.notify_all();
    return mode;
}

int nblic_amd_device_qcoder_stats(nblic_amd_ctx *c, double *symbols, long *launches, long *images, double *kernel_ms) {
    if (!c) c = default_ctx();
    if (!c) return -1;
    std::lock_guard<std::mutex> l(c->stat_m);
    if (symbols) *symbols = c->qdev_symbols;
    if (launches) *launches = c->qdev_launches;
    if (images) *images = c->qdev_images;
    if (kernel_ms) *kernel_ms = c->qdev_kernel_ms;
    return 0;
}

int nblic_amd_qcoder_selftest(nblic_amd_ctx *c) {
    if (!c) c = default_ctx();
    if (!c || hipSetDevice(c->device) != hipSuccess) return -1;
    std::lock_guard<std::mutex> g(c->api);
    const long bad = device_q_quot_selftest(c->dec_stream);
    return bad < 0 ? -1 : int(std::min<long>(bad, 0x7FFFFFFF));
}

long nblic_amd_debug_q_rans_host(int height, int width, const uint16_t *words, const unsigned int *hist, long symbols_per_launch,
                                 uint16_t *out, size_t cap_words) {
    if (!words || !hist || !out) return -2;
    if (height < 1 || width < 1 || height > kIndexMaxSide || width > kIndexMaxSide) return -2;
    if (!q_words_ok(words, size_t(height) * size_t(width), hist)) return -2;
    return q_rans_encode_host(out, cap_words, height, width, words, hist, symbols_per_launch);
}

int nblic_amd_debug_device_q_entropy(nblic_amd_ctx *c, int n_jobs, const uint16_t *const *words, const unsigned int *n_symbols,
                                     const unsigned int *const *hists, const size_t *caps_words, long symbols_per_launch,
                                     uint16_t *const *outs, long *lens) {
    constexpr int kMaxJobs = 4096;
    constexpr size_t kMaxBytes = size_t(1) << 30, kGuard = 64, kMaxSymbols = size_t(1) << 24, kMaxLaunches = 8192;
    constexpr uint8_t kPattern = 0xA5;
    if (!c || n_jobs < 1 || n_jobs > kMaxJobs || !words || !n_symbols || !hists || !caps_words || !outs || !lens || symbols_per_launch < 0) return -1;
    auto align = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t nj = size_t(n_jobs);
    const uint32_t budget = symbols_per_launch == 0 ? kQSymbolsPerLaunch : uint32_t(std::min<long>(symbols_per_launch, long(kMaxSymbols)));
    std::vector<size_t> in_at(nj), out_at(nj), cap_body(nj);
    std::vector<long> front(nj);
    std::vector<uint32_t> tables(nj * kQRansTable), freq(kQRansTable), start(kQRansTable);
    size_t in_bytes = 0, out_bytes = kGuard, n_max = 0;                         // a guard in front of the first region too
    for (int k = 0; k < n_jobs; k++) {
        const size_t n = n_symbols[k];
        if (!words[k] || !hists[k] || n < 1 || n > kMaxSymbols || (caps_words[k] > 0 && !outs[k]) || caps_words[k] > kMaxBytes / 2) return -1;
        if (!q_words_ok(words[k], n, hists[k])) return -1;
        n_max = std::max(n_max, n);
        in_at[size_t(k)] = in_bytes;
        in_bytes += align((n + kQRansWindow - 1) / kQRansWindow * kQRansWindow * sizeof(uint16_t));       // whole 512-byte windows, the caller's padding included
        if (in_bytes > kMaxBytes) return -1;
    }
    if ((n_max + budget - 1) / budget > kMaxLaunches) return -1;
    // the front matter, on the host and straight into the caller's buffers: a region's capacity is what it leaves
    for (int k = 0; k < n_jobs; k++) {
        // the header names the widest image of n pixels (the pass does not look at it): w the largest divisor of n below 65536
        const size_t n = n_symbols[k];
        size_t w = std::min<size_t>(n, 65535);
        while (n % w != 0) w--;
        if (n / w > 65535) return -1;
        const int h = int(n / w);
        front[size_t(k)] = q_entropy_front(outs[k], caps_words[k], h, int(w), hists[k], freq.data(), start.data());
        q_rans_table(freq.data(), start.data(), tables.data() + size_t(k) * kQRansTable);
        cap_body[size_t(k)] = front[size_t(k)] < 0 ? 0 : caps_words[k] - size_t(front[size_t(k)]);
        out_at[size_t(k)] = out_bytes;
        out_bytes += (cap_body[size_t(k)] * sizeof(uint16_t) + kGuard + 63) & ~size_t(63);                // the region, then 64 .. 127 bytes of guard
        if (out_bytes > kMaxBytes) return -1;
    }
    std::lock_guard<std::mutex> g(c->api);
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    Stream st;
    DevBuf<uint8_t> d_in, d_out; DevBuf<uint32_t> d_tables, d_results; DevBuf<QRansJob> d_jobs;
    Pinned<QRansJob> h_jobs; Pinned<uint32_t> h_results;
    std::vector<uint8_t> h_in(std::max<size_t>(in_bytes, 256), 0), h_out(out_bytes, kPattern);
    for (int k = 0; k < n_jobs; k++)
        memcpy(h_in.data() + in_at[size_t(k)], words[k], (size_t(n_symbols[k]) + kQRansWindow - 1) / kQRansWindow * kQRansWindow * sizeof(uint16_t));
    bool ok = st.create(hipStreamNonBlocking) == hipSuccess && d_in.alloc(h_in.size()) == hipSuccess && d_out.alloc(out_bytes) == hipSuccess &&
              d_tables.alloc(tables.size()) == hipSuccess && d_results.alloc(nj) == hipSuccess && d_jobs.alloc(nj) == hipSuccess &&
              h_jobs.alloc(nj) == hipSuccess && h_results.alloc(nj) == hipSuccess;
    if (ok) {
        for (int k = 0; k < n_jobs; k++) {
            QRansJob &J = h_jobs[k];
            J.words = reinterpret_cast<const uint16_t *>(d_in.get() + in_at[size_t(k)]);
            J.table = d_tables.get() + size_t(k) * kQRansTable;
            J.out_end = reinterpret_cast<uint16_t *>(d_out.get() + out_at[size_t(k)]) + cap_body[size_t(k)];
            J.result = d_results.get() + k;
            J.cap = uint32_t(cap_body[size_t(k)]);
            J.live = front[size_t(k)] < 0 ? 0u : 1u;                             // no room for the front matter: never launched, reports -1
            q_rans_begin(J.st, n_symbols[k], J.cap);
            h_results[k] = 0u;
        }
        ok = hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_out, h_out.data(), out_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_tables, tables.data(), tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_results, h_results, nj * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_jobs, h_jobs, nj * sizeof(QRansJob), hipMemcpyHostToDevice, st) == hipSuccess;
        for (size_t done = 0; ok && done < n_max; done += budget) ok = device_q_rans(d_jobs, n_jobs, budget, st);   // the resumed sequence: every record stays on the device
        ok = ok && hipMemcpyAsync(h_results, d_results, nj * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipMemcpyAsync(h_out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = hipStreamSynchronize(st) == hipSuccess && ok;
    }
    if (!ok) return -2;
    // everything the kernel may not have written still holds the pattern: the guards, and a region in front of its reported words
    bool intact = true;
    size_t at = 0;
    auto pattern_to = [&](size_t end) { for (; at < end; at++) intact = intact && h_out[at] == kPattern; };
    for (int k = 0; k < n_jobs; k++) {
        const uint32_t r = h_results[k];
        const size_t region = cap_body[size_t(k)] * sizeof(uint16_t);
        pattern_to(out_at[size_t(k)]);
        lens[k] = -1;
        if (front[size_t(k)] < 0) { if (r != 0u) intact = false; pattern_to(out_at[size_t(k)] + region); continue; }
        if (r == 0xFFFFFFFFu) { at += region; continue; }                      // did not fit: the kernel wrote what it liked inside the region
        if (r < 2u || size_t(r) > cap_body[size_t(k)]) { intact = false; at += region; continue; }       // no length written, or one beyond the region
        pattern_to(out_at[size_t(k)] + region - size_t(r) * sizeof(uint16_t));
        memcpy(outs[k] + front[size_t(k)], h_out.data() + at, size_t(r) * sizeof(uint16_t));
        at += size_t(r) * sizeof(uint16_t);
        lens[k] = front[size_t(k)] + long(r);
    }
    pattern_to(out_bytes);
    return intact ? 0 : -3;
}

// ---- drop-in entry points --------------------------------------------------------------------
int NBLICcompress(int verbose, unsigned char *p_buf, unsigned char *p_img, int height, int width, int *p_near, int *p_effort) {
    (void)verbose;
    *p_near = iclip(*p_near, 0, kMaxNear);                                   // NBLIC.c:768
    *p_effort = iclip(*p_effort, 1, 3);                                      // NBLIC.c:770
    int k_step = k_step_for_near(*p_near);
    write_header(p_buf, height, width, *p_near, k_step, *p_effort);          // the reference writes it before validating
    nblic_amd_ctx *c = default_ctx();
    if (!c) return -1;
    if (!size_ok(height, width, c->max_px)) return -1;                       // NBLIC.h:31 unless nblic_amd_set_max_pixels(NULL, ...) raised it
    const bool serial_mode = !(*p_near == 0 && *p_effort == 1);
    if (serial_mode && size_t(height) * size_t(width) > (size_t(1) << 23)) {
        // a large image of a raster-serial mode: row bands (one band's workspace instead of 120 bytes per pixel of the
        // whole image, one model launch per band) -- the same bytes
        nblic_amd_stream *st = stream_open(c, p_img, false, height, width, *p_near, *p_effort, 0);
        if (!st) return -1;
        size_t n = 0;
        int rc = stream_run(st, 0.0, p_buf, size_t(1) << 46, &n);            // the reference ABI carries no capacity
        if (rc == 1 && *p_near > 0) { int r0 = 0, r1 = 0; rc = nblic_amd_stream_recon(st, p_img, &r0, &r1) == 0 ? 1 : -1; }   // NBLIC.c:876
        stream_free(st);
        return rc == 1 && n < (size_t(1) << 31) ? int(n) : -1;
    }
    const unsigned char *imgs[1] = {p_img};
    unsigned char *outs[1] = {p_buf}, *recons[1] = {p_img};
    size_t caps[1] = {SIZE_MAX};
    long lens[1] = {-1};
    if (nblic_amd_encode_batch_modes(c, 1, imgs, 0, &height, &width, p_near, p_effort, outs, caps, lens, recons) != 0) return -1;
    return int(lens[0]);
}

int NBLICdecompress(int verbose, unsigned char *p_buf, unsigned char *p_img, int *p_height, int *p_width, int *p_near, int *p_effort) {
    (void)verbose;
    nblic_amd_ctx *c = default_ctx();
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->api);
    return decode_dropin(c, p_buf, false, p_img, p_height, p_width, p_near, p_effort);          // NBLIC.c:698-712, :924-926
}

int nblic_amd_qencode_batch(nblic_amd_ctx *c, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                            const int *heights, const int *widths, uint16_t *const *outs, const size_t *out_caps_words,
                            long *out_len_words) {
    if (!c) return -1;
    return run_batch(c, nblic_amd_ctx::SubmitItem{nullptr, 1, n_images, imgs, imgs_on_device != 0, heights, widths, reinterpret_cast<unsigned char *const *>(outs),
                                                  out_caps_words, out_len_words, nullptr, nullptr, nullptr}) ? 0 : -1;
}

int QNBLICcompress(uint16_t *p_buf, unsigned char *p_img, int height, int width) {
    nblic_amd_ctx *c = default_ctx();
    if (!c) return -1;
    if (!size_ok(height, width, c->max_px)) return -1;                       // QNBLIC.c:575
    const unsigned char *imgs[1] = {p_img};
    uint16_t *outs[1] = {p_buf};
    size_t caps[1] = {SIZE_MAX / 4};                                          // the reference ABI carries no capacity
    long lens[1] = {-1};
    if (nblic_amd_qencode_batch(c, 1, imgs, 0, &height, &width, outs, caps, lens) != 0) return -1;
    return int(lens[0]);
}
int QNBLICdecompress(uint16_t *p_buf, unsigned char *p_img, int *p_height, int *p_width) {
    nblic_amd_ctx *c = default_ctx();
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->api);
    return decode_dropin(c, reinterpret_cast<const unsigned char *>(p_buf), true, p_img, p_height, p_width, nullptr, nullptr);   // QNBLIC.c:475-555
}
int QNBLICcompressMultiThread(uint16_t *p_buf, unsigned char *p_img, int height, int width) {
    return QNBLICcompress(p_buf, p_img, height, width);                      // QNBLIC.c:872-883: same stream either way
}

}  // extern "C"
