// kernels_e1.h -- launch interface of the staged -e1 lossless kernels (kernels_e1.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nblic {

constexpr uint32_t kMaxSegments = 1024;   // waves per partition pass (pixel partitions)
// The touch partition keeps 4096 output runs open per wave; with 1024 waves per image that is
// 4 M partially written lines (512 MB) -- more than the 256 MB Infinity Cache, and rocprof showed
// 9x write amplification.  256 waves per image keep the open lines of a launch resident.
constexpr uint32_t kTouchSegments = 256;
constexpr int kTotalsStride = 8, kWideTouchFlag = 4;      // words per image in the totals array; index of the wide-position flag
// The spare words of an image's totals count the S2 blocks of its last front half (kernels_e1.hip k_bias_blocks ..
// k_bias_replay): warm-up copies met / resolved through a candidate table / replayed serially in order.
constexpr int kLongS2Met = 5, kLongS2Table = 6, kLongS2Serial = 7;
// The device array has kTotalsSlot words per image: the totals record, then the re-mapper chains' counts (k_map_plan ..
// k_map_check): chains cut into blocks / blocks whose guessed start permutation was right / blocks replayed after a miss.
constexpr int kTotalsSlot = 16, kLongS3Split = 8, kLongS3Accepted = 9, kLongS3Missed = 10;
constexpr int kLongBlockMin = 128;         // records per block of a cut re-mapper chain, at least (sizes mblk_cnt / mblk_perm)

struct SegPlan { int nseg; uint32_t seg_len; };
SegPlan make_plan(uint32_t n_items, uint32_t max_segments = kMaxSegments);

// Device buffers of one image in flight.  Pixel-sized arrays hold n = h*w entries,
// event-sized arrays hold ev_cap entries.
constexpr size_t kStreamPad = 512;         // u16 records of slack after every key-sorted stream

struct E1Buffers {
    const uint8_t *img;      // n      input plane (lossless: also the reconstruction)
    uint32_t *rec1;          // n      S1 record (model.h pack_s1)
    uint16_t *s2in;          // n+pad  px0 | err<<8, grouped by context
    uint32_t *pos2;          // n      where pixel t sits in s2in / s2out
    uint16_t *s2out;         // n+pad  px | sign<<8, same order as s2in
    uint16_t *pxs;           // n      px | sign<<8 back in raster order
    uint16_t *s3in;          // n+pad  y (< 20), grouped by re-mapper
    uint32_t *pos3;          // n      where pixel t sits in s3in / s3out, or 0x80000000 | y (bypass)
    uint16_t *s3out;         // n+pad  z, same order as s3in
    uint8_t  *z;             // n      coded symbol, raster order
    uint8_t  *cnt;           // n      bins per pixel
    uint32_t *ev_off;        // n      exclusive scan of cnt
    uint32_t *table;         // 4096 * kMaxSegments   partition histogram / offsets
    uint32_t *scan_sums;     // scan scratch
    uint32_t *totals;        // [kTotalsSlot] item totals: adr, mapper, events, touches; [kWideTouchFlag] 1 = this image needs 32-bit touch positions; [kLongS2Met ..] block counts of S2
    int      *ctx_state;     // 2048
    int      *map_state;     // 512 * 60
    int      *cnt_state;     // 4096 * 2
    uint32_t *events;        // ev_cap        model.h pack_event
    uint16_t *tin;           // 2*ev_cap+pad  touch payloads grouped by counter
    uint64_t *tpos;          // ev_cap + 64   two u32 arrays (even trees, odd trees): position of the event's touch in tin/tout (28 bits, all ones = none) with qw / bin / parity in the top four bits (kernels_e1.hip pack_pos); plain 32-bit positions, ~0 = none, for an image with >= 2^28 - 1 touches
    uint16_t *tout;          // 2*ev_cap+pad  P(bin==1) before each touch, same order as tin
    uint32_t *blk_base;      // 2049          first block of every context chain (+ total)
    int      *blk_end;       // n/4096+2048   context state at the end of each block
    uint8_t  *blk_ok;        // n/4096+2048   1 = the block's warm-up copies met (its output is exact)
    int      *blk_cand;      // 2 * (n/4096+2048)  per block whose copies did not meet: the lower copy at its first record (after k_bias_fixup: the exact state there), its table (-1 = none)
    uint32_t *blk_item;      // n/4096+64     table -> block
    int      *blk_tab;       // 128 * (n/4096+64)  per table: the block's end state from each of the 128 candidate start states
    uint32_t *mblk_base;     // 513           first block of every cut re-mapper chain (+ total); a chain that is not cut has none
    uint32_t *mblk_cnt;      // 20 * (n/128+512)   per block: hits by SYMBOL at its first record (k_map_hist leaves the block's own histogram, k_map_prefix the sums)
    uint32_t *mend_cnt;      // 512 * 20      hits by symbol behind a cut chain's last record
    uint64_t *mblk_perm;     // 4 * (n/128+512)    per block: symbol -> rank (Perm20) it was started with, and at its end
    uint32_t *qhist;         // 12 * 256      QNBLIC symbol histograms per activity level
    unsigned long long *dbg_out;   // 4096 words of in-kernel cycle stamps, written only when E1Job::dbg & 8
    uint32_t *win_base;      // 4097 + 4096   first window record of every counter chain (+ total); chain keys, longest first
    uint32_t *win_recs;      // 24 words per 512-touch window: entry state + halving epochs (kernels_e1.hip WinRec)
    uint16_t *coded;         // ev_cap        prob | bin<<15 for the host range coder
};

// One image of a group.  The array of jobs lives in device memory; every kernel picks its job
// from the last grid dimension.
struct E1Job {
    E1Buffers b;
    int h, w;
    uint32_t n;          // h * w
    SegPlan pp;          // partition plan over pixels
    uint32_t n_ev;       // bins (known after the front half)
    SegPlan pe;          // partition plan over bins
    int dbg;             // timing experiments only (NBLIC_AMD_DBG); 0 in normal operation
    int near, k_step;    // serial modes only (the staged -e1 kernels use the lossless constants 0 and 3)
    uint64_t ktab;       // model.h level_shift_table(k_step)
    int long_min, long_block;   // long chains (nblic_amd_set_long_chains): a re-mapper chain of >= long_min records is cut into blocks of long_block;
                                // long_min < 0 = none is, and context-chain blocks whose copies did not meet are replayed serially, in order
    int row0;            // the image row at index 0 of b.img / b.rec1: 0 for a whole image; a row band of the band encoder
                         // (e1_launch_front_band) has h = its rows, b.img = plane + row0 * w, and the plane goes on above b.img
    // Where the coded bins go.  pack_rows == nullptr: b.coded, one u16 (prob | bin << 15) per bin, for an image that is
    // coded on its own.  Otherwise the image is lane pack_lane (0..7) of a PACK: up to eight consecutive jobs of the launch
    // that share pack_rows and that one AVX-512 register of a host coder thread codes together.  k_mix leaves such an
    // image's bins as 13-bit groups (range_coder.h: thirteen 64-bit words per 64 bins) back to back in b.tin, whose touch
    // payloads are dead by then, and k_pack_rows lays the pack's streams side by side:
    // pack_rows[(13 * g + j) * 8 + pack_lane] = word j of bins 64 g .. 64 g + 63 (zero where a lane has no bin).
    uint64_t *pack_rows;
    int pack_lane;
};

// One HIP event before every kernel launch (and one after the last): interval k is exactly
// launch k of the sequence below, measured on the stream it runs on.  A launch covers the
// whole group of images.
constexpr int kE1Kernels = 31;
constexpr int kE1Marks = kE1Kernels + 1;
struct E1Timers { hipEvent_t ev[kE1Marks]; uint64_t mask = ~0ull; };     // mask: bit k = stage k is timed (events k and k + 1 are recorded)
constexpr uint64_t kRooflineStages = (1ull << 1) | (1ull << 26);            // k_predict (S1) and k_touch_scatter: what the bench line's rooflines need
static const char *const kE1StageNames[kE1Kernels] = {
    "k_init_state", "k_predict",
    "k_adr_count", "scan_reduce.adr", "scan_sums.adr", "scan_apply.adr", "k_adr_scatter",
    "k_plan_blocks", "k_bias_blocks", "k_bias_fixup",
    "k_map_count", "scan_reduce.map", "scan_sums.map", "scan_apply.map", "k_map_scatter",
    "k_mapper_chains",
    "k_count_bins", "scan_reduce.bins", "scan_sums.bins", "scan_apply.bins",
    "host_gap",
    "k_emit_bins",
    "k_touch_count", "scan_reduce.touch", "scan_sums.touch", "scan_apply.touch", "k_touch_scatter",
    "k_plan_windows", "k_counter_epochs", "k_counter_probs",
    "k_mix+k_pack_rows"};      // one interval: k_mix, and k_pack_rows behind it when the launch has packs

int e1_selftest(hipStream_t s);     // 0 = DPP wave scan agrees with the shuffle scan
// d_jobs: device copy of h_jobs[0..n_jobs).  The host copy is only read to size the grids.
void e1_launch_front(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, E1Timers *tm);
// The same sequence for ROW BANDS of -n0 -e1 images (E1Job::row0): no k_init_state -- ctx_state, map_state and cnt_state hold
// what the rows above left, every chain kernel starts from them and writes its end state back -- and S1 takes a pixel's
// fall-backs from its row in the image, reading the two rows above a band from the plane.  Untimed; `model_done`, if
// given, is recorded behind k_bias_fixup (S1 .. S2 is what replaces the serial model stage).
void e1_launch_front_band(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, hipEvent_t model_done = nullptr);
void e1_launch_back(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, E1Timers *tm, bool general = false);
// serial modes (near > 0, efforts 2/3): model state init, then -- after the caller has run the serial
// model stage (serial_engine.h) that leaves rec1 and px | sign per pixel -- the re-mapper partition,
// the re-mapper chains and the bin counts; e1_launch_back(..., general = true) finishes the job
void e1_launch_init(const E1Job *d_jobs, int n_jobs, hipStream_t s);
// Seek-index entry records of row bands (the indexed batch, pipeline.hip).  For every task, one workgroup converts the model
// tables of job `job` -- as its band's front and back halves left them -- into the DECODER's state record (serial_engine.h:
// SerialState, the 2048 context biases, the 4096 counters c0 | c1 << 16 tree-major, the re-mappers' hit counts, symbol -> rank
// and rank -> symbol bytes) followed by the two image rows above the row behind the band, at out + `out`.  The header is
// zero but for `bias`; the coder fields are the host's, which knows them once the band is coded.
struct IndexRecordTask { int job, reserved; unsigned long long out; };     // out: byte offset of the record, a multiple of 4
void e1_launch_index_records(const E1Job *d_jobs, const IndexRecordTask *d_tasks, int n_tasks, uint8_t *d_out, hipStream_t s);
void e1_launch_front_pre(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s);
// QNBLIC (effort 0) model stage for a group: leaves level | symbol << 8 per pixel in `pxs` and the
// 12 x 256 histograms in `qhist`; the entropy stage (normalise, histogram code, rANS) is host work.
void q_launch_model(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s);
// The same for ROW BANDS of effort-0 images (E1Job::row0; the indexed effort-0 batch, pipeline.hip), the counterpart of
// e1_launch_front_band: k_init_state runs for the jobs with row0 == 0 alone, the context chains start from the slot's
// ctx_state and leave their end state there, the window's rows 0 / 1 rules follow the row in the IMAGE and the rows above a
// band are read from the plane, and k_q_symbols adds the band's counts to the slot's qhist; pxs holds level | symbol << 8
// of the band's pixels.  The jobs of a launch differ in row0, height and width.
void q_launch_model_band(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s);
// QNBLIC's sibling of e1_launch_index_records: per task the decoder record of job `job` -- a zero SerialState (all of it
// is the host's), then the 3072 contexts as its band's chains left them, which is how the decoder keeps them -- followed by
// the two image rows above the row behind the band, at out + `out`: kQDecodeStateBytes + 2 w bytes.
void q_launch_index_records(const E1Job *d_jobs, const IndexRecordTask *d_tasks, int n_tasks, uint8_t *d_out, hipStream_t s);
// The same launch sequences from caller-made records instead of an image (the debug entries of pipeline.hip,
// tests/test_chain_kernels.py): the front half behind S1 from b.rec1 (model.h pack_s1) and b.img (h * w = n values, read as
// a flat array), QNBLIC's model stage behind k_q_predict from b.rec1 (px0 | adr << 8), the back half behind k_emit_bins
// from b.events and n_ev.  Nothing is initialised: the model tables are the caller's (band semantics; e1_launch_init writes
// an image's first ones).
void e1_launch_model_stages(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s);
void q_launch_model_stages(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s);
void e1_launch_back_stages(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s);

}  // namespace nblic
