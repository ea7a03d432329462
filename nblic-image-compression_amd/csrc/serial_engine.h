// serial_engine.h -- the raster-serial part of NBLIC on the GPU (serial_engine.hip).
//
// Every mode other than -n0 -e1 encode has a chain that runs pixel by pixel through the whole image
// (SURVEY.md section 0.4): near-lossless encode predicts from RECONSTRUCTED neighbours, efforts 2/3
// carry least-squares statistics and a global regularisation strength from pixel to pixel, and every
// decoder needs the previous pixel before it can decode the next.  What is serial differs, though:
//
//   encode (any near, any effort)   only prediction, context bias and quantisation are a chain; the
//       adaptive re-mappers, the binarisation, the counters and the range coder never feed back into
//       a pixel value.  k_serial_model runs that chain -- ONE WAVE PER IMAGE, hundreds of images side
//       by side -- and leaves per pixel the same records the staged -e1 front half leaves
//       (rec1, px | sign); the entropy stages then run on the key-partitioned kernels of
//       kernels_e1.hip and the host range coder, exactly as for -n0 -e1.
//   decode (NBLIC, any mode)        the whole loop is one chain: k_serial_decode, one wave per image,
//       model state (contexts, counters, re-mappers) in LDS.
//   decode (QNBLIC)                 k_serial_qdecode, one wave per image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deliver.h"
#include "collect.h"
#include "color_plan.h"
#include "stack.h"
#include "deep.h"

namespace nblic {

// ---- resumable launches ---------------------------------------------------------------------------
// A serial kernel never has to run an image in one piece: everything its chain carries across a ROW boundary lives
// in a small per-image state record in device memory, a launch works on at most `rows` rows from the row the record
// names, and the next launch picks up there.  What crosses a row boundary:
//   model stage (encode)   the 2048 context biases; the least-squares regularisation strength `bias` (NBLIC.c:762 --
//       never reset); the column statistics B are in memory anyway (SerialJob::stats), the running row statistics E
//       are reset per row (NBLIC.c:818), the row pre-pass F is recomputed per row; the two rows above come back from
//       the reconstruction (or, lossless, from the input plane);
//   NBLIC decoder          the same plus the 4096 counters, the 512 re-mappers, the coder interval and its 4-byte
//       window, and the position in the stream;
//   QNBLIC decoder         the 3072 contexts, the rANS state and the position in the stream.
// Header of the record (SerialState), then the tables.  The host zeroes the header before the first launch.
struct SerialState {
    int next_row;              // first row the next launch works on (0: fresh image -- the launch initialises the tables itself)
    int status;                // kRunning / kDone / kFailed / kStarved / kStarvedMidRow
    unsigned long long pos;    // decoders: next stream byte to consume
    uint32_t lo, hi, window;   // decoders: coder interval and window (QNBLIC: lo = rANS state)
    int bias;                  // efforts 2/3
    unsigned long long avail;  // decoders, written by the HOST before a launch: stream bytes present in device memory
    int final_;                // decoders, written by the host: 1 = `avail` is the whole stream (running dry is an error), 0 = more may follow
    int pad[5];
};
static_assert(sizeof(SerialState) == 64, "header is sixteen words");
enum : int { kRunning = 0, kDone = 1, kFailed = -1, kStarved = 2, kStarvedMidRow = 3 };
// kStarved: a decoder of a stream that is still being fed stopped cleanly in front of row next_row because fewer than
// starve_margin(w) bytes were left -- feed more, set status back to kRunning, launch again.  kStarvedMidRow: it ran dry
// inside a row although the margin was there (a row that costs more than four bytes per pixel: never seen, possible
// for a damaged stream); the record is then NOT resumable as it stands: the lean decoder has changed the hit counts in
// it and every decoder has changed B in place.  The band decoder (pipeline.hip, nblic_amd_dstream; the drop-in decoders
// run it too) never launches the lean one and restores B from a copy taken before the launch.
constexpr size_t starve_margin(int w) { return size_t(4) * size_t(w) + 1024; }
constexpr size_t kModelStateBytes = sizeof(SerialState) + 2048 * sizeof(int);
constexpr size_t kDecodeStateBytes = sizeof(SerialState) + (2048 + 4096 + 512 * 20) * sizeof(int) + 2 * 512 * 20;
// word offsets of the decoder record's tables after SerialState: context biases and counters, then the re-mappers' hit
// counts (kRecCount), symbol -> rank (kRecRank) and rank -> symbol (kRecSym) bytes.  The lean decoder keeps the hit
// counts there and never writes the symbol -> rank bytes back (serial_engine.hip DecodeLdsLean).
constexpr int kRecCount = 2048 + 4096, kRecRank = kRecCount + 512 * 20, kRecSym = kRecRank + 512 * 20 / 4;
constexpr size_t kQDecodeStateBytes = sizeof(SerialState) + 3072 * sizeof(int);

// One image of a serial launch (array in device memory, job = blockIdx.x).
struct SerialJob {
    const uint8_t *img;        // encode: the plane to code (never written)
    uint8_t *recon;            // encode: reconstruction (may be null when near == 0 and the rows fit in LDS); decode: the decoded plane
    uint32_t *rec1;            // encode out: S1 record per pixel (model.h pack_s1)
    uint16_t *pxs;             // encode out: px | sign << 8 per pixel
    const uint8_t *stream;     // decode in: the .nblic stream (header included); how much of it is there is SerialState::avail
    double *stats;             // efforts 2/3: 2 * w * stats_stride(effort) doubles, zeroed (column sums, then the row pre-pass)
    SerialState *state;        // resumable state (above): kModelStateBytes / kDecodeStateBytes / kQDecodeStateBytes
    int h, w, near, k_step, effort;
    int rows;                  // rows per launch (>= 1)
    int out_row0;              // encode: the row whose records sit at index 0 of rec1 / pxs (0, or the first row of the band they hold)
    int recon_row0;            // decode: the image row stored at index 0 of recon (0: the whole plane; a band decoder: the first row it holds)
    unsigned long long stream_off;   // decode: absolute stream offset of byte 0 of `stream` (a multiple of 512; SerialState::pos / avail stay absolute)
    int end_row;               // decode: the job stops in front of this row (0: h).  Reaching end_row < h leaves the record as a band
                               // boundary leaves it (tables written back, status kRunning, next_row == end_row); further launches return at once
    unsigned long long *redo;  // efforts 2/3: two counters the launch adds to -- pixels whose system 0 / system 1 of the least squares left the
                               // exact range of the doubles and were redone with 64-bit integers (lsq_f64.h Guard).  Jobs may share a pair; null: not counted
    // QNBLIC decode only
    const uint32_t *q_freq, *q_start; const uint8_t *q_slot;      // 12 x 256 frequencies and cumulative starts; q_slot: unused (the kernel searches q_start)
};

constexpr int stats_stride(int effort) { return effort == 3 ? 128 : (effort == 2 ? 64 : 0); }   // doubles per pixel column per array
inline size_t stats_doubles(int effort, int w) { return size_t(2) * size_t(w) * size_t(stats_stride(effort)); }

// Rows one launch should cover so that it lasts a few seconds at most (a pixel of effort 2 / 3 costs about four / eight
// times a pixel of effort 1); `override_rows` > 0 (nblic_amd_set_serial_rows) wins.
inline int serial_rows_per_launch(int h, int w, int effort, int override_rows) {
    if (override_rows > 0) return override_rows < h ? override_rows : h;
    const long budget = (long(1) << 22) / (effort == 3 ? 8 : (effort == 2 ? 4 : 1));
    long rows = budget / (w > 0 ? w : 1);
    if (rows < 1) rows = 1;
    return int(rows < h ? rows : h);
}
inline int serial_launches(int h, int rows) { return (h + rows - 1) / rows; }

// true when the three rows a pixel's taps can touch fit in the LDS the model kernel has left, i.e. the kernel will keep
// them there; otherwise it reads its taps from SerialJob::recon, which then has to be there even for lossless jobs
bool serial_model_rows_fit(int w);
// The kernel variant a launch of n images (widest: max_w) gets, as the launchers below decide it: kPlanTwoWaves (model,
// effort 3: a second wave per image), kPlanLean (decoders: the lean LDS image), kPlanRowsInLds (the widest image's rows
// are cached in LDS; a kernel compares per job, so narrower jobs of the same launch still are).
enum : int { kPlanTwoWaves = 1, kPlanLean = 2, kPlanRowsInLds = 4 };
int serial_model_plan(int effort, int n, int max_w);
int serial_decode_plan(int n, int max_w, bool whole_streams);
int serial_qdecode_plan(int max_w);                                  // the QNBLIC decoder: one LDS image, kPlanRowsInLds or 0

// d_jobs[0..n): all of one effort (1, 2 or 3); h_jobs: host copy, read to size the launch.  ONE launch: every job
// advances by its `rows`; call serial_launches(h, rows) times (maximum over the jobs) to finish them.
bool serial_model_launch(const SerialJob *d_jobs, const SerialJob *h_jobs, int n, hipStream_t s);
bool serial_decode_launch(const SerialJob *d_jobs, const SerialJob *h_jobs, int n, hipStream_t s, bool whole_streams);   // whole_streams: every job's stream is final (SerialState::final_)
bool serial_qdecode_launch(const SerialJob *d_jobs, const SerialJob *h_jobs, int n, hipStream_t s);
// ---- an indexed batch decode's segment set-up and chain check, on the device ----------------------------------------------
// The index of an image is uploaded as it is, so an entry's body -- state record | B | the two rows above -- lies at ANY
// address: an entry is 8 + 168 + body + 32 bytes and the body holds 2 w bytes of rows, so at odd w successive records sit
// at 2 mod 4 and at w = 2 mod 4 the doubles of B sit at 4 mod 8.  Both kernels read the entry as aligned 32-bit words
// shifted into place (or byte by byte, for the rows); what they write is the library's own and aligned, except the rows
// of the plane.  A task's bytes are cut into chunks of kIndexChunkBytes, one workgroup each (a 4 MB B and its F are 512 of them).
//   k_index_seed   one task per segment: the record the segment starts from (the entry's, or zeros with pos = first_pos
//                  for segment 0; status kRunning, avail, final_ = 1), B into the first half of [B | F], zeros into F, and
//                  the rows above into the plane.
//   k_index_chain  one task per inner boundary: the segment's final record, B and plane rows against the next entry.  Of the
//                  record's header next_row, pos, lo and bias must be the entry's and status kRunning (NBLIC: hi and window
//                  too; QNBLIC keeps its state in lo alone); avail, final_ and the padding are the host's and skipped.  The
//                  tables must be the entry's, for NBLIC without the words [kRecRank, kRecSym): the lean decoder never
//                  writes them back, and the index check has verified that the entry's are the inverse of its rank ->
//                  symbol bytes, which ARE compared.  A part that differs ORs its bit into the boundary's verdict word
//                  (kChainRecord / kChainB / kChainRows); a part whose byte count is 0 is skipped.
struct IndexTask {
    const uint8_t *entry;                  // the entry's body inside the uploaded index; seed: null = segment 0
    uint8_t *rec;                          // the segment's state record
    uint8_t *stats;                        // [B | F]; null when the mode has none
    uint8_t *rows;                         // the plane byte of the first row rows_above names (rows_bytes of them follow)
    uint32_t *verdict;                     // chain: the boundary's verdict word (zeroed by the host)
    unsigned long long avail, first_pos;   // seed: SerialState::avail, and pos of segment 0
    uint32_t rec_bytes, b_bytes, rows_bytes;   // of the record and of B (multiples of 16), of the rows (any)
    uint32_t b_at, rows_at;                // where B and the rows lie in the entry's body
    uint32_t kind;                         // 0 NBLIC, 1 QNBLIC
    uint32_t first_chunk;                  // chunks of the tasks in front of this one
    uint32_t pad;
};
static_assert(sizeof(IndexTask) == 88, "uploaded as bytes");
enum : uint32_t { kChainRecord = 1, kChainB = 2, kChainRows = 4 };
constexpr uint32_t kIndexChunkBytes = 16384;
// Chunks of one task: record | B (seed: and F behind it) | rows, in 16-byte units.
inline uint32_t index_task_units(const IndexTask &t, bool seed) { return t.rec_bytes / 16 + (seed ? 2 : 1) * (t.b_bytes / 16) + (t.rows_bytes + 15) / 16; }
inline uint32_t index_task_chunks(const IndexTask &t, bool seed) { return (index_task_units(t, seed) + kIndexChunkBytes / 16 - 1) / (kIndexChunkBytes / 16); }
// d_tasks[0..n) with first_chunk filled in, `chunks` their sum.  false: the launch failed.
bool index_seed_launch(const IndexTask *d_tasks, int n, uint32_t chunks, hipStream_t s);
bool index_chain_launch(const IndexTask *d_tasks, int n, uint32_t chunks, hipStream_t s);

// ---- a batch index build's entry capture, on the device: the inverse of k_index_seed -------------------------------------
// A decode job that has stopped in front of an entry row (SerialJob::end_row) holds everything that entry's body is made
// of: its record, B in the first half of [B | F], the two rows above in the plane.  k_index_capture, one task per (job,
// entry), writes that body -- record | B | the 2 w-byte row slot -- to a 16-byte-aligned place in the image's staging buffer,
// from where the host moves it to its place in the index (any address) while it hashes it; the kernel stores whole
// aligned 16-byte units only, the slot's last one filled up with zeros.  A task ACTS only when the job's record says
// status kRunning and next_row == row, and writes nothing otherwise: a job that failed, or has not arrived, captures nothing.
//   the record   the header as a checkpoint holds it (pipeline.hip dstream_checkpoint): status kRunning, avail, final_ and the
//                padding zero, the rest verbatim; the tables verbatim -- except NBLIC's symbol -> rank bytes [kRecRank,
//                kRecSym), which the lean decoder never writes back: they are rebuilt as the inverse of the rank -> symbol
//                bytes, rank[m][sym[m][i]] = i, for either decoder image (0 for a symbol the rank -> symbol bytes do not name)
//   the rows     read byte by byte: the plane lies at any address
// The workgroup of a task's chunk 0 then sets the job's end_row to next_end (the next entry row; 0 behind the last), which
// nothing else in the launch reads.
struct IndexCaptureTask {
    const uint8_t *rec;                    // the job's state record
    const uint8_t *stats;                  // [B | F]; null when the mode has none
    const uint8_t *rows;                   // the plane byte of the first row rows_above names (rows_bytes of them follow)
    uint8_t *out;                          // the staged body (a multiple of 16)
    SerialJob *job;                        // the job in the launches' job array
    int row, next_end;
    uint32_t rec_bytes, b_bytes;           // of the record and of B (multiples of 16)
    uint32_t rows_lead, rows_bytes;        // the slot: rows_lead zeros, then rows_bytes from the plane (together 2 w)
    uint32_t kind;                         // 0 NBLIC, 1 QNBLIC
    uint32_t first_chunk;                  // chunks of the launch's tasks in front of this one
};
static_assert(sizeof(IndexCaptureTask) == 72, "uploaded as bytes");
inline uint32_t index_capture_units(const IndexCaptureTask &t) { return t.rec_bytes / 16 + t.b_bytes / 16 + (t.rows_lead + t.rows_bytes + 15) / 16; }
inline uint32_t index_capture_chunks(const IndexCaptureTask &t) { return (index_capture_units(t) + kIndexChunkBytes / 16 - 1) / (kIndexChunkBytes / 16); }
// d_tasks[0..n) with first_chunk filled in (from 0), `chunks` their sum.  false: the launch failed.
bool index_capture_launch(const IndexCaptureTask *d_tasks, int n, uint32_t chunks, hipStream_t s);

// ---- delivery: a window of each decoded plane into caller-owned device memory (deliver.h) ------------------------------------
// k_deliver, in the family of the kernels above: tasks with first_chunk, one workgroup per chunk of kDeliverChunkUnits units,
// a unit = at most sixteen pixels of one row whose destination starts at a multiple of 16 bytes.  The source row starts at
// any byte (odd widths, any col0) and is read as aligned words shifted into place; the destination gets 16-byte stores but
// for a row's head and tail.  uint8 is a copy; float16 / bfloat16 / float32 are float(px) * scale + bias, two roundings, then
// round-to-nearest-even into the format.  A task with `zero`, or with a gate record that is not kDone, writes zero bytes.
// A task with a reference plane (a colour frame's R - G or B - G) delivers (px + ref - 128) & 255 in place of px.
// d_tasks[0..n) with first_chunk filled in (from 0), `chunks` their sum.  false: the launch failed.
bool deliver_launch(const DeliverTask *d_tasks, int n, uint32_t chunks, hipStream_t s);

// ---- collection: images out of caller-owned device memory into the encoders' contiguous planes (collect.h) -------------------
// k_collect, the delivery's twin: tasks with first_chunk, one workgroup per chunk of kCollectChunkUnits units, a unit =
// sixteen consecutive bytes of the flat plane at a multiple of 16.  The source has any pitch and any step between the pixels
// of a row; uint8 is a copy, float16 / bfloat16 / float32 are float(x) * scale + bias, two roundings, NaN to 0, clamped to
// [0, 255] and rounded to nearest even.  A task with a reference source writes (own - ref + 128) & 255 of the two pixels.
// d_tasks[0..n) with first_chunk filled in (from 0), `chunks` their sum.
// false: the launch failed.
bool collect_launch(const CollectTask *d_tasks, int n, uint32_t chunks, hipStream_t s);

// ---- the cost of a colour frame's nine candidate planes (color_plan.h ColorCostTask) ------------------------------------------
// k_color_cost, beside k_collect: tasks with first_chunk, one workgroup per tile of kCostTile x kCostTile pixels of one
// frame (cost_tile.h).  The workgroup stages the tile's R, G, B pixels -- quantised by k_collect's loader, each source element once -- with
// one row above and one column to the left in LDS, computes the nine residual costs of every pixel from there, and adds its
// nine sums (lanes, then waves in LDS) to the task's costs with one 64-bit atomic each: integer adds, so the result does
// not depend on the launch's geometry or order.  The costs are zeroed by the caller.  d_tasks[0..n) with first_chunk
// filled in (from 0), `tiles` their sum.  false: the launch failed.
bool color_cost_launch(const ColorCostTask *d_tasks, int n, uint32_t tiles, hipStream_t s);

// ---- slice stacks (stack.h) ---------------------------------------------------------------------------------------------------
// k_deliver_stack, beside k_deliver: one task is one RUN -- a key slice and the delta slices behind it -- with its slices in
// d_slices.  A lane walks the run's slices for its unit of sixteen window pixels with the running pixels in registers, so
// no task waits for another one's output and every plane byte of the window is read once.  d_tasks[0..n) with first_chunk
// filled in (from 0), `chunks` their sum.  false: the launch failed.
bool deliver_stack_launch(const StackDeliverTask *d_tasks, int n, const StackSlice *d_slices, uint32_t chunks, hipStream_t s);
// k_stack_cost, beside k_color_cost: one task is one STACK with its sources in d_slices, one workgroup per tile position.
// The workgroup walks the slices with two LDS tile buffers and adds two sums per slice -- the slice's own cost and that of
// its difference against the slice before -- to the task's costs (zeroed by the caller) with 64-bit atomics.
bool stack_cost_launch(const StackCostTask *d_tasks, int n, const StackCostSlice *d_slices, uint32_t tiles, hipStream_t s);

// ---- deep pixels (deep.h) ------------------------------------------------------------------------------------------------------
// k_collect_deep, beside k_collect: one task is one PLANE of a 16-bit source -- high, low or folded low -- in k_collect's
// units; sixteen neighbouring elements are read as eight aligned words where the step is 2 and the address allows.
bool collect_deep_launch(const DeepCollectTask *d_tasks, int n, uint32_t chunks, hipStream_t s);
// k_deliver_deep, beside k_deliver: one task is one deep image -- both planes, both gates, the mode, the window -- in
// k_deliver's units; a contiguous uint16 unit is two 16-byte stores, a float32 unit four.
bool deliver_deep_launch(const DeepDeliverTask *d_tasks, int n, uint32_t chunks, hipStream_t s);
// k_deep_cost, beside k_color_cost: one workgroup per tile of one image; three sums, the minimum and the maximum of u per
// image, by 64-bit atomics (sums zeroed, min 0xFFFF and max 0 before the launch: the caller's).
bool deep_cost_launch(const DeepCostTask *d_tasks, int n, uint32_t tiles, hipStream_t s);

// ---- a packed index (index_pack.h), expanded on the device ------------------------------------------------------------------
// A packed index is uploaded as it is (any address).  The bodies of the entries a round needs are written, unpacked, into an
// aligned buffer -- record | B | the row slot, `out_stride` apart; the QNBLIC tables are not: nothing on the device reads an
// entry's -- and the IndexTask::entry pointers of k_index_seed and k_index_chain point there.  Three launches:
//   k_index_unpack_scan  one wave per (image, entry, coded part): the payload offset of every block, an exclusive scan of the
//                        part's width bytes, 64 blocks per step across the lanes.  Once per call: `offs` serves every round.
//   k_index_unpack       one wave per (image, part, block), one unit per lane.  The differences chain from entry to entry, so
//                        the wave walks entries 0 .. walk - 1 in order with each lane's running value in a register, reads
//                        the block's width byte b and takes its b bits out of the aligned 32-bit words around them, and
//                        stores the unit -- one aligned 2-, 4- or 8-byte store -- for the entries from `first_out` on.
//   k_index_unpack_rank  the symbol -> rank bytes a packed entry leaves out, from the unpacked rank -> symbol bytes, as
//                        k_index_capture rebuilds them; one workgroup per (image, stored entry).
// desc[e * n_parts + j] = where part j of entry e lies in the packed index (its data, behind its flag byte) | flag << 56, from
// the host's check, which has walked every width byte: nothing the kernels read lies outside the packed index.
struct IndexUnpackPart { uint32_t out_at, bytes, unit, code, init, first_block; };       // index_pack.h PackPart, and the blocks in front
struct IndexUnpackTask {
    const uint8_t *packed;
    const unsigned long long *desc;
    uint32_t *offs;                        // [entry][blocks]: a block's payload, in bytes from its part's data
    uint8_t *out;                          // entries first_out .. walk - 1 (0-based), out_stride apart (a multiple of 16)
    uint32_t walk, first_out, out_stride, n_parts;
    uint32_t blocks;                       // of all parts together
    uint32_t first_wave, first_scan_wave, first_rank_group;   // waves / workgroups of the tasks in front of this one
    IndexUnpackPart part[8];
};
static_assert(sizeof(IndexUnpackTask) == 256, "uploaded as bytes");
constexpr unsigned long long kUnpackDescAt = (1ull << 56) - 1;
inline uint32_t index_unpack_waves(const IndexUnpackTask &t) { return t.blocks; }
inline uint32_t index_unpack_scan_waves(const IndexUnpackTask &t) { return t.walk * t.n_parts; }
constexpr uint32_t kUnpackCodeRank = 4;                                                  // index_pack.h kCodeRank (pipeline.hip asserts it)
inline uint32_t index_unpack_rank_groups(const IndexUnpackTask &t) {                     // one per stored entry of a mode that has re-mappers
    for (uint32_t j = 0; j < t.n_parts; j++) if (t.part[j].code == kUnpackCodeRank) return t.walk - t.first_out;
    return 0;
}
// d_tasks[0..n) with the first_* fields filled in; the totals of each.  false: the launch failed.
bool index_unpack_scan_launch(const IndexUnpackTask *d_tasks, int n, uint32_t scan_waves, hipStream_t s);
bool index_unpack_launch(const IndexUnpackTask *d_tasks, int n, uint32_t waves, uint32_t rank_groups, hipStream_t s);

// Both least-squares solvers of the serial kernels on `count` given systems, no image and no coder (tests): stats = count x vec_len(n)
// integer-valued statistics [s | b | A], vn = count x 10 regressors, bias = the regularisation strength the pixel starts from (the two
// systems of an item are the ones bias_pair makes of it).  n = 6 or 10; waves = 2 (n = 10 only) runs the two-wave hand-over.  Per item
// out_f64[12] = the double path's clamped Q12 predictions of system 0 / 1, then the Guard maxima (product, entry, quotient, pivot) of
// system 0 and of system 1; out_i64[14] = what the kernels' own predict / solve_one + take_other deliver (p1, p2, ok1, ok2), the double
// path's ok of system 0 / 1, its Guard verdicts, the integer path's raw Q12 sums, its ok of system 0 / 1, and the redo counts the item
// added.  Both paths are always computed.  false: a HIP call failed or the arguments are out of range.
bool serial_lsq_probe(hipStream_t s, int n, int waves, int count, const double *stats, const int8_t *vn, const int *bias, double *out_f64, long long *out_i64);
int serial_selftest(hipStream_t s);                    // device check of the double-carried divisions against 64-bit integers and of the half-wave exchange; 0 = pass

}  // namespace nblic
