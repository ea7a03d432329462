/*
 * nblic_amd.h -- C ABI of libnblic_amd.so, the MI355X-native drop-in for the NBLIC v0.3
 * codec entry points.  Plain pointers and sizes only; no torch / HIP types.
 *
 * Section 1 re-declares the reference's own API with identical names, argument meaning and
 * return conventions, so a caller of the reference library (its only caller is main(),
 * src/NBLIC_main.c:184-188,223-226) links against this library unchanged.
 * Section 2 is additive: a context + batch interface that keeps several images in flight per
 * GPU (the reference has no equivalent; it is what bench.py and the Python host layer use).
 *
 * The compute path is HIP only.  If no gfx950 device is usable every entry point that has to
 * compute returns -1 after printing a diagnostic to stderr -- there is no CPU fallback.
 */
#ifndef NBLIC_AMD_H
#define NBLIC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* limits, same values as the reference (src/NBLIC.h:29-31, src/QNBLIC.h:9-11) */
#define NBLIC_MAX_HEIGHT     65535
#define NBLIC_MAX_WIDTH      65535
#define NBLIC_MAX_IMG_SIZE   100000000
#define QNBLIC_MAX_HEIGHT    65535
#define QNBLIC_MAX_WIDTH     65535
#define QNBLIC_MAX_IMG_SIZE  100000000

/* ---- 1. drop-in entry points -------------------------------------------------------- */

/* Replaces NBLICcompress (src/NBLIC.h:54, src/NBLIC.c:915).
 * verbose  : accepted, ignored on the GPU path (the reference prints row progress).
 * p_buf    : caller-owned output, no capacity argument (reference contract); worst case seen
 *            is ~1.0025 B/px + 20, the reference CLI provides 2 B/px.
 * p_img    : 8-bit gray, row-major, stride == width.  WRITTEN: receives the reconstruction
 *            (identical bytes when *p_near == 0), as the reference does at NBLIC.c:876.
 * p_near   : clamped to [0,9] and written back.   p_effort : clamped to [1,3], written back.
 * returns  : stream length in BYTES, or -1.                                              */
int NBLICcompress(int verbose, unsigned char *p_buf, unsigned char *p_img, int height, int width,
                  int *p_near, int *p_effort);

/* Replaces NBLICdecompress (src/NBLIC.h:72, src/NBLIC.c:924).  All four int outputs are
 * parsed from the 16-byte header.  returns 0 or -1.                                       */
int NBLICdecompress(int verbose, unsigned char *p_buf, unsigned char *p_img, int *p_height, int *p_width,
                    int *p_near, int *p_effort);

/* Replace QNBLICcompress / QNBLICdecompress / QNBLICcompressMultiThread (src/QNBLIC.h:14-18,
 * src/QNBLIC.c:562,493,872).  Effort 0, lossless only.  compress returns the length in
 * 16-bit WORDS (the reference's caller doubles it, NBLIC_main.c:184-186) or -1.           */
int QNBLICcompress(uint16_t *p_buf, unsigned char *p_img, int height, int width);
int QNBLICdecompress(uint16_t *p_buf, unsigned char *p_img, int *p_height, int *p_width);
int QNBLICcompressMultiThread(uint16_t *p_buf, unsigned char *p_img, int height, int width);

/* ---- 2. additive context / batch API ------------------------------------------------- */

typedef struct nblic_amd_ctx nblic_amd_ctx;

/* device   : HIP device ordinal.
 * n_slots  : images kept in flight on the GPU (each owns a stream and a workspace); >= 1.
 * n_coders : host threads running the serial range-coder stage; >= 1.
 * returns NULL (and prints why) when the device cannot be used.                            */
nblic_amd_ctx *nblic_amd_create(int device, int n_slots, int n_coders);

/* Same, with the split of the images in flight spelled out: n_groups groups of group_size
 * images.  A group shares every kernel launch (its serial chains run side by side); while the
 * host codes one group the GPU works on the next.  n_host_buffers (raised to at least
 * n_groups * group_size + 16) buffers IN HBM hold coded-bin streams waiting for a coder thread,
 * so the device workspace of an image is free again as soon as its kernels have finished; the
 * coder threads stream the bins to the host through a small pinned ring of their own.  (The
 * parameter keeps its name from when these buffers were pinned host memory.)
 * nblic_amd_create uses two groups and 2 * n_slots buffers.                                   */
nblic_amd_ctx *nblic_amd_create_ex(int device, int n_groups, int group_size, int n_coders, int n_host_buffers);
void nblic_amd_destroy(nblic_amd_ctx *ctx);

/* Encode n_images gray planes at -n0 -e1 (lossless) into byte-exact .nblic streams.
 * imgs[k]        : plane k, heights[k] x widths[k], stride == width.
 * imgs_on_device : 0 = host pointers, 1 = device (HBM) pointers on the context's device.
 * outs[k]        : host buffer for stream k, out_caps[k] bytes (checked; -1 if too small).
 * out_lens[k]    : receives the stream length in bytes, or -1 for that image.
 * returns 0 when every image succeeded, -1 otherwise.                                      */
int nblic_amd_encode_batch(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                           const int *heights, const int *widths, unsigned char *const *outs,
                           const size_t *out_caps, long *out_lens);

/* The same batch in two halves, so that several batches can be in flight: _begin only QUEUES the
 * batch and returns at once -- a submitter thread of the context hands its images to the GPU
 * pipeline later (waiting while every group is busy), so the argument arrays are read AFTER _begin
 * has returned; _end waits until every stream of THAT batch has been written and returns 0 / -1
 * like nblic_amd_encode_batch: -1 when one of THIS batch's images failed (a failure in another
 * batch in flight does not show here) or when the context itself is unusable.  While batch k
 * drains through the host coder threads (~0.8 s for the last packs) batch k+1 is already filling
 * the GPU: a continuous feed never sees the pipeline's fill and drain.  All argument arrays and
 * buffers of a batch must stay valid, and its outputs untouched, until its _end; batches may be
 * ended in any order.                                                                          */
typedef struct nblic_amd_batch nblic_amd_batch;
nblic_amd_batch *nblic_amd_encode_batch_begin(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs,
                                              int imgs_on_device, const int *heights, const int *widths,
                                              unsigned char *const *outs, const size_t *out_caps, long *out_lens);
int nblic_amd_encode_batch_end(nblic_amd_ctx *ctx, nblic_amd_batch *batch);

/* Same for effort 0 (QNBLIC): the per-pixel model runs on the GPU, the entropy stage (histogram
 * normalisation, histogram code, rANS) on a coder thread.  outs[k] are uint16_t buffers; capacities
 * and lengths are in 16-bit WORDS, like QNBLICcompress's return value.                         */
int nblic_amd_qencode_batch(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                            const int *heights, const int *widths, uint16_t *const *outs, const size_t *out_caps_words,
                            long *out_len_words);

/* Any mode, many images: the batch form of NBLICcompress (src/NBLIC.h:54, src/NBLIC.c:749-908, :915).
 * nears[k] / efforts[k] : image k's -n / -e, clamped to [0,9] / [1,3] exactly as the reference clamps them
 *                  (either array may be NULL: 0 / 1).  -n0 -e1 images take the staged pipeline; every other
 *                  mode is raster-serial in its prediction (reconstructed neighbours, least-squares
 *                  statistics), so its model stage runs ONE WAVE PER IMAGE with all images of the batch side
 *                  by side -- size the context (n_groups x group_size) for the number of images you want in
 *                  flight -- and its entropy stages on the same parallel kernels and host coder threads.
 * recons        : NULL, or per image NULL / a host buffer of h*w bytes that receives the reconstruction the
 *                  reference leaves in p_img (NBLIC.c:876); may be the (host) input plane itself.
 * Everything else as nblic_amd_encode_batch.  returns 0 / -1.                                        */
int nblic_amd_encode_batch_modes(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                 const int *heights, const int *widths, const int *nears, const int *efforts,
                                 unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                 unsigned char *const *recons);

/* The batch form of NBLICdecompress / QNBLICdecompress (src/NBLIC.h:72, src/QNBLIC.h:16; the codec is told
 * from the magic like src/NBLIC_main.c:223-226 does): n_images streams decoded side by side, one wave each.
 * streams[k] / stream_lens[k] : the stream and its length in BYTES (unlike the reference ABI, which takes none).
 * imgs[k] / img_caps[k]       : host buffer for the plane and its size in bytes.
 * heights / widths / nears / efforts : outputs parsed from the headers (QNBLIC: near = effort = 0).
 * status[k]                   : 0, or -1 for that stream (bad header, plane too large, stream exhausted).
 * returns 0 when every stream decoded, -1 otherwise.                                                 */
int nblic_amd_decode_batch(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                           unsigned char *const *imgs, const size_t *img_caps, int *heights, int *widths, int *nears,
                           int *efforts, int *status);

/* Opt-in: the range-coder stage (src/NBLIC.c:552-586) on the GPU as a SUPPLEMENT to the host coder threads.
 * n_packs pack threads are started (they sleep unless there is work); each hands 64 queued images at a time to
 * one wave of the GPU, ONE LANE PER IMAGE (~17 Mbins/s per image: a 4096^2 frame takes seconds, but 64 of them
 * take the same seconds and none of their bins cross PCIe).  A pack is taken only when the queue of finished
 * images holds 64 more than the host threads can take at once, and only while at least min_outstanding images
 * of the submitted batches are unfinished -- set it to (pack latency x the host threads' image rate) so that a
 * pack can never become the tail of the work.  The streams are byte-identical either way.  Returns the number
 * of pack threads, or -1.  Size n_host_buffers (nblic_amd_create_ex) 64 x n_packs larger than without.       */
int nblic_amd_set_device_coder(nblic_amd_ctx *ctx, int n_packs, int min_outstanding);
/* What the device coder did since the context was last idle: bins coded, packs launched, images coded. */
void nblic_amd_device_coder_stats(nblic_amd_ctx *ctx, double *bins, long *packs, long *images);

/* Who moved the chunks of coded bins of this context's PACKS to the host since it was created.  While the HSA runtime
 * loaded in the process offers its copy entry points (and NBLIC_AMD_COPY_ENGINE is not 0) a chunk travels on a DMA
 * engine, which occupies no compute queue; otherwise, and from the first engine error on, through hipMemcpyAsync.
 *   out[0] chunks that arrived by the engine            out[2] chunks handed to the runtime because the engine failed on them
 *   out[1] chunks handed to the runtime                 out[3] 1 when the engine is available to this context, else 0
 * No output byte depends on the path.  Returns 0, -1 for bad arguments.                                          */
int nblic_amd_copy_stats(nblic_amd_ctx *ctx, long out[4]);

/* How the context's group streams were spread over the hardware queues of the process when it was created.  A process
 * has a few in-order hardware queues and the runtime deals every stream to one of them by a rule of its own; a context
 * of three groups or more therefore creates candidate streams, sorts them into classes with a probe ("does a short
 * kernel on b wait behind a 1 ms kernel on a?"; the least of three repetitions decides), gives the groups streams whose
 * classes hold numbers of groups that differ by one at the most, and destroys the rest.  It asks the runtime for no
 * queue it would not have given anyway.  NBLIC_AMD_QUEUE_PLAN=0 (read at creation) switches the plan off.
 *   out[0] 0 the plan is on; otherwise every group created its own stream, as the runtime dealt them, because
 *          1 the context has fewer than three groups (nothing ran)   2 the switch   3 one class only was found
 *          4 a probe was inconclusive                               5 a call of the runtime failed
 *   out[1] classes found (the hardware queues the candidates reached; 0 when the classification did not finish)
 *   out[2] candidate streams created            out[3] groups of the context
 *   out[4] largest minus smallest number of groups over the classes found, as planned
 *   out[5] the same for the first out[3] candidates: what not planning would have given
 *   out[8 + k], k < out[1]: groups in class k (0 on: they sum to out[3]; 3: all in class 0)
 * *plan_ms (may be NULL): host milliseconds the plan took.  No output byte depends on any of this.  Returns 0, -1 for
 * bad arguments.                                                                                                  */
int nblic_amd_queue_plan_stats(nblic_amd_ctx *ctx, long out[40], double *plan_ms);

/* Opt-in: raise the pixel-count limit above NBLIC_MAX_IMG_SIZE for this context (config 5 of
 * BASELINE.json exceeds the reference's own limit, src/NBLIC.h:31).  0 restores the reference limit.
 * ctx == NULL addresses the context behind the drop-in entry points of section 1.                   */
void nblic_amd_set_max_pixels(nblic_amd_ctx *ctx, long max_pixels);

/* The raster-serial kernels (the model stage of near > 0 / efforts 2, 3 encodes, every decoder) are RESUMABLE:
 * whatever their chain carries across a row boundary lives in a per-image state record on the device, a launch works
 * on at most `rows` rows of every image, and the next launch picks up where it stopped -- so no kernel runs longer
 * than a few seconds however large the image (config 5 of BASELINE.json is a 268 Mpixel frame at effort 3).
 * rows > 0 fixes the rows per launch (tests use it to force many resumptions); 0 = sized automatically.
 * ctx == NULL addresses the context behind the drop-in entry points.  nblic_amd_serial_launches: launches of the
 * serial kernels since the context was created.                                                              */
void nblic_amd_set_serial_rows(nblic_amd_ctx *ctx, int rows);
long nblic_amd_serial_launches(nblic_amd_ctx *ctx);

/* Long chains.  The staged kernels (-n0 -e1, QNBLIC's model stage, the staged band front, the indexed batch) replay each
 * table entry's records as one chain, and on flat, saturated or document-like content one entry holds nearly all of
 * them.  The context-bias chains are cut into blocks of 4096 records whose start state is found by running two copies
 * from the extreme states over the 3072 records before the block; where the copies do not meet (a constant error parks
 * them up to 127 apart) the block is replayed from each of the at most 128 states between them, which leaves a table
 * "start state -> end state", the chain's blocks are then walked with one look-up each, and the outputs are written
 * a lane per block.  No output byte depends on any of this.
 * The re-mapper chains' hit counts never decay and belong to symbols, so the counts by symbol at any record are the chain's
 * start counts plus a histogram prefix; only the permutation at a block's first record is unknown.  A chain of at least
 * min_records records is cut into blocks of block_records: every block is replayed from a GUESSED permutation (symbols by
 * descending count, ties in the chain's starting order, refined over the block before), and accepted, in order, only if
 * the guess is the block before's true end permutation -- otherwise it is replayed from the true state.  A wrong guess
 * costs time, never a byte.
 *   min_records, block_records: 0 = the defaults (65536, 4096); block_records is at least 128.
 *   min_records < 0  turns both parts off: blocks whose copies did not meet are replayed in order by one lane per chain
 *   and no re-mapper chain is cut -- the launch sequence before either existed (A/B runs, an escape hatch).
 * Both values travel in every job record.  No output byte depends on either.
 * nblic_amd_long_chain_stats: blocks since the context was created or last reset (reset != 0 clears after reading):
 *   counts[0] context-chain blocks whose copies met      counts[3] re-mapper chains cut into blocks
 *   counts[1] ... resolved through a table                counts[4] re-mapper blocks whose guessed start was right
 *   counts[2] ... replayed serially, in order             counts[5] re-mapper blocks replayed after a wrong guess
 *   counts[6], counts[7] are 0.  counts[2] is 0 on every input unless min_records < 0.  The device words ride in the
 * totals record every front half already reads back.  ctx == NULL addresses the context behind the drop-in entry points.
 * Returns 0, -1 for bad arguments.                                                                              */
void nblic_amd_set_long_chains(nblic_amd_ctx *ctx, int min_records, int block_records);
int nblic_amd_long_chain_stats(nblic_amd_ctx *ctx, long counts[8], int reset);

/* Efforts 2 / 3 carry the reference's int64 least squares in doubles and redo a pixel with plain 64-bit integers when
 * one of its two systems leaves the range in which the doubles are exact.  counts[0] / counts[1]: the pixels
 * whose system 0 / system 1 did, over every encode and decode of the context since it was created or last reset
 * (reset != 0 clears the pair after reading it; 64-bit counters; a decoder launch that is thrown away and run again
 * because it ran dry inside a row adds nothing).  Reporting and tests: hard-edged content (text, charts) coded
 * near-lossless reaches the redo, photographs practically never.  ctx == NULL addresses the context behind the drop-in
 * entry points.  Call it between batches.  Returns 0, or -1.                                                       */
int nblic_amd_lsq_redo_counts(nblic_amd_ctx *ctx, unsigned long long counts[2], int reset);

/* Which variant of the serial kernels a launch of `images` images of one effort (1..3), the widest `width` pixels wide,
 * gets -- decided by the very functions the launchers go by (reporting, tests; no device needed).  decode == 0: the
 * model stage of an encode; decode != 0: the NBLIC decoder (whole_streams: every stream is there in full, as in
 * nblic_amd_decode_batch).  Bits: 1 = two waves per image (effort-3 encodes of few images), 2 = the lean decoder image
 * (many streams side by side), 4 = the rows of the widest image are kept in LDS (otherwise its taps come from memory).
 * decode != 0 with effort 0: the QNBLIC decoder, which has one LDS image for any number of streams -- bit 4 alone.
 * Returns -1 for arguments out of range.                                                                             */
int nblic_amd_serial_plan(int decode, int effort, int images, int width, int whole_streams);

/* ONE image of any mode, worked through in ROW BANDS (src/NBLIC.c:749-908 is one loop over the rows; every piece of
 * state it carries from row to row is small).  Per band: the model stage for the band's rows, the entropy stages for
 * those pixels (their adaptive tables carried from band to band), the band's bins through the range coder.  The device
 * workspace is one band's whatever the image size, no kernel runs longer than a band, and between two bands the
 * encoder can be SUSPENDED: nblic_amd_stream_checkpoint writes down everything it carries (a few hundred KB plus
 * 8 * width * (1 + n + n^2) bytes of least-squares statistics at efforts 2 / 3), nblic_amd_stream_resume -- in
 * another call, another process, on another GPU -- carries on from there.  The stream's bytes are identical to
 * NBLICcompress's.  A running SHA-256 of the bytes emitted travels with the checkpoint, so a run that never holds the
 * whole stream in one place can still be checked against a golden hash.
 *   _begin    img: the whole plane (host or device; it must stay valid until _end).  band_rows <= 0: sized automatically.
 *             Takes one group of the context until _end.  NULL on failure.
 *   _run      codes bands until the image is finished (returns 1) or budget_seconds (> 0) have passed (returns 0); the
 *             stream bytes produced by THIS call are written to out (out_cap is checked, -1 if too small) and counted
 *             in *out_len: concatenate the pieces of successive calls.
 *   _progress rows finished, bytes emitted so far, their SHA-256, milliseconds spent in the model kernel; returns 1 / 0 / -1.
 *   _checkpoint  writes the checkpoint into buf (cap bytes) and returns its size; with buf == NULL or cap too small it
 *             only returns the size needed; 0 before the first _run, after the image is finished or after a failure.
 *             Valid between two _run calls.
 *   _resume   a checkpoint of _checkpoint; every field is checked (magic, format version, checksum over the whole body,
 *             sizes against the geometry and mode, the header fields, the state and its tables) before anything is
 *             allocated or reaches the device: NULL if any is off.  A damaged checkpoint is refused, and so is one
 *             written by an earlier build ("NBLCKPT1").  img must be the plane the checkpoint was taken from.
 *   _check    the same checks alone, on the host (no device is touched; ctx may be NULL, it only supplies the pixel
 *             limit): 0 valid, -1 refused.
 *   _recon    the reconstruction the reference leaves in p_img (NBLIC.c:876), as far as THIS object has produced it:
 *             rows [*first_row, *end_row) are written at their place in `plane` (a whole h x w plane); an object resumed
 *             from a checkpoint starts at the checkpoint's row, the rows before it came out of the earlier objects.   */
typedef struct nblic_amd_stream nblic_amd_stream;
nblic_amd_stream *nblic_amd_stream_begin(nblic_amd_ctx *ctx, const unsigned char *img, int img_on_device, int height, int width,
                                         int near, int effort, int band_rows);
nblic_amd_stream *nblic_amd_stream_resume(nblic_amd_ctx *ctx, const unsigned char *img, int img_on_device, const void *checkpoint,
                                          size_t checkpoint_bytes);
int nblic_amd_stream_run(nblic_amd_stream *s, double budget_seconds, unsigned char *out, size_t out_cap, size_t *out_len);
size_t nblic_amd_stream_checkpoint(nblic_amd_stream *s, void *buf, size_t cap);
int nblic_amd_stream_check(nblic_amd_ctx *ctx, const void *checkpoint, size_t bytes);
int nblic_amd_stream_progress(nblic_amd_stream *s, int *rows_done, unsigned long long *bytes_total, unsigned char sha256[32], double *model_ms);
int nblic_amd_stream_recon(nblic_amd_stream *s, unsigned char *plane, int *first_row, int *end_row);
void nblic_amd_stream_end(nblic_amd_stream *s);
/* The band encoder's SEEK INDEX (nblic_amd_index_* below), at no extra decode: _set_index, before the first _run, asks
 * for an entry in front of every row every_rows, 2 every_rows, ... (1 <= every_rows < height; 0 / -1); bands are then
 * cut short at those rows, which never shows in the stream.  _index, after the image is finished, writes the index
 * into buf (cap bytes) and returns its size (buf == NULL or cap too small: only the size); it is byte-identical to
 * nblic_amd_index_build(every_rows) of the same stream.  0 for an object that was resumed from a checkpoint or never
 * asked for an index. */
int nblic_amd_stream_set_index(nblic_amd_stream *s, int every_rows);
size_t nblic_amd_stream_index(nblic_amd_stream *s, void *buf, size_t cap);
/* The FRONT a band's model stage runs on, per object: after _begin or _resume and before that object's first _run
 * (0 / -1; -1 too for s == NULL, for a front other than 0 or 1, and for a mode the front does not take -- a refusal
 * launches nothing and leaves the object as it was).
 *   0  serial (the default): the one-wave model kernel of the serial modes, every near and effort.
 *   1  staged: the band's rows go through the key-partitioned kernels of the batch pipeline (prediction, partition
 *      by context, context-bias chains).  -n0 -e1 only: lossless -e1 is the one mode without a pixel-to-pixel
 *      prediction chain.
 * The stream bytes, the checkpoints and the index are byte-identical under both; the front is a property of the
 * object, not of the checkpoint, so a checkpoint written under one front resumes under the other.  _progress's
 * model_ms is the serial model kernel under front 0, the launches that replace it under front 1. */
int nblic_amd_stream_set_front(nblic_amd_stream *s, int front);

/* ONE stream DECODED in ROW BANDS (src/NBLIC.c:807-898 is a single pass over the rows): the caller feeds the stream in
 * pieces of any size as it arrives and takes the rows as they are finished; the device workspace depends on band_rows
 * and the width, never on the height ((band_rows + 2) x width reconstruction rows, the least-squares statistics at
 * efforts 2 / 3, one state record, a stream window of max(4 MiB, 2 x band_rows x width + 8 x width + 2048) bytes), and
 * between two _run calls the decoder can be SUSPENDED: nblic_amd_dstream_checkpoint writes down everything it carries,
 * nblic_amd_dstream_resume -- in another call, another process, on another GPU -- carries on from there, fed from the
 * checkpoint's feed_from offset on.  A running SHA-256 of every decoded row travels with the checkpoint, so a split
 * decode can be checked against a golden reconstruction hash without ever holding the plane.  NBLIC and QNBLIC streams
 * alike (told apart by the magic); the context's pixel limit (nblic_amd_set_max_pixels) applies.  Each object has a HIP
 * stream and a workspace of its own, so it can run next to batches, band encoders and other band decoders of its context;
 * one object is driven by one thread at a time.
 *   _begin    band_rows <= 0: sized automatically (a launch of a few seconds).  NULL on failure.
 *   _resume   a checkpoint of _checkpoint; every field is checked (magic, format version, checksum over the whole body,
 *             sizes against the geometry, the header fields, the state) before anything reaches the device: NULL if any is off.
 *   _check    the same checks alone, on the host (no device is touched): 0 valid, -1 refused.
 *   _feed     appends n bytes of the stream (after a resume: the stream from feed_from on); final_ != 0: the stream ends
 *             with these bytes.  Only the bytes from the decoder's window on are kept.  0 / -1.
 *   _info     1 once the header (QNBLIC: and its tables) is in, 0 not yet, -1 refused (not a stream this library decodes).
 *   _run      decodes until the image is finished (returns 1), budget_seconds (> 0) have passed or rows_out is full
 *             (returns 0), or the fed bytes run out before the stream is complete (returns 2: feed more, call again); -1
 *             on error (damaged or truncated stream, rows_out smaller than the next band).  The rows finished by THIS call
 *             are written to rows_out one after the other (cap bytes, at least min(band_rows, rows left) x width) and are
 *             rows [*first_row, *end_row) of the image.
 *   _progress rows finished, the offset the stream would have to be fed from after a checkpoint taken now, the SHA-256 of
 *             the rows finished so far, device bytes held; returns 1 finished / 0 / -1 failed.
 *   _checkpoint  writes the checkpoint into buf (cap bytes) and returns its size; with buf == NULL or cap too small it only
 *             returns the size needed; 0 before the header is in or after the image is finished.  Valid between two _run calls. */
typedef struct nblic_amd_dstream nblic_amd_dstream;
nblic_amd_dstream *nblic_amd_dstream_begin(nblic_amd_ctx *ctx, int band_rows);
nblic_amd_dstream *nblic_amd_dstream_resume(nblic_amd_ctx *ctx, const void *checkpoint, size_t bytes);
int nblic_amd_dstream_check(nblic_amd_ctx *ctx, const void *checkpoint, size_t bytes);
int nblic_amd_dstream_feed(nblic_amd_dstream *d, const unsigned char *bytes, size_t n, int final_);
int nblic_amd_dstream_info(nblic_amd_dstream *d, int *kind, int *height, int *width, int *near, int *effort);
int nblic_amd_dstream_run(nblic_amd_dstream *d, double budget_seconds, unsigned char *rows_out, size_t cap, int *first_row, int *end_row);
int nblic_amd_dstream_progress(nblic_amd_dstream *d, int *rows_done, unsigned long long *feed_from, unsigned char sha256[32],
                               size_t *device_bytes);
size_t nblic_amd_dstream_checkpoint(nblic_amd_dstream *d, void *buf, size_t cap);
void nblic_amd_dstream_end(nblic_amd_dstream *d);

/* SEEK INDEX: band-decoder checkpoints (the _checkpoint format above, band_rows = R) taken in front of every row R, 2R, ...
 * below the height, kept NEXT TO the stream -- the stream's bytes do not change, and an index can be made for any stream,
 * the reference's included.  Each entry is an entry point: the rows below it decode without the rows above.  So one image
 * decodes as (h - 1) / R + 1 segments side by side, one wave each, and any row range decodes from the entry at or above it.
 * An index is bound to one stream (its length and SHA-256) and checksummed as a whole and entry by entry.
 * SIZE: a 96-byte head, 32 bytes of checksum, and per entry 8 + 200 bytes (length, checkpoint head, its checksum) + a body of:
 *   NBLIC      the decoder record (86,080 bytes) + 2 x width (the rows above the entry), + 512 x width (-e2) / 1024 x width
 *              (-e3) bytes of least-squares statistics.  At -e2 / -e3 an index is large unless R is large: a 16384 x 16384
 *              -e3 image at R = 1024 has 15 entries of 16.9 MB, 254 MB in all.
 *   QNBLIC     the record (12,352 bytes) + 2 x width + the 24,576 bytes of frequency tables.
 *   _check          every field of the index and of each entry (nblic_amd_dstream_check), the entries' rows R, 2R, ... and
 *                   their geometry against the head; with stream != NULL also that it is the stream the index was made for.
 *                   Host only (no device is touched): 0 valid, -1 refused.  The decoders below run it before any launch.
 *   _build          the index of `stream` (one serial band-decoder pass over the whole image, which must decode) into out
 *                   (cap bytes); returns its size.  With out == NULL or cap too small it only returns the size needed
 *                   (ctx may then be NULL).  -1:
 *                   not a stream this library decodes, every_rows < 1 or every_rows >= height, or the stream does not decode.
 *   decode_indexed  the whole plane into img (img_cap >= height x width) from the whole stream and its index, every segment
 *                   side by side.  Each segment's final state, statistics and last two rows are compared with the next
 *                   entry: any difference refuses the result (-1, img zeroed: no unverified pixel is left there).  0 on
 *                   success.  Segments run in rounds of at most 1 GiB of per-segment state;
 *                   nblic_amd_set_index_round(ctx, n > 0) caps a round at n segments (0: the memory bound alone).
 *   decode_rows     rows [row0, row1) alone into out (cap >= (row1 - row0) x width): the segments row0 / R .. (row1 - 1) / R
 *                   side by side, the first from the last entry at or above row0, and every entry strictly inside the
 *                   range compared with the end of the segment in front of it as decode_indexed compares them (-1, the
 *                   (row1 - row0) x width bytes zeroed).  Nothing else is written.  0 / -1.
 * Both are nblic_amd_decode_batch_indexed (below) with one image: its host check, its rules for a refused image (-1, nothing
 * launched, the buffer untouched) and its verification on the device are theirs, and a context without a usable device
 * refuses them.  Each call has a HIP stream and a workspace of its own, so it can run next to batches and band coders of
 * its context. */
void nblic_amd_set_index_round(nblic_amd_ctx *ctx, int segments);
int nblic_amd_index_check(nblic_amd_ctx *ctx, const void *index, size_t index_bytes, const unsigned char *stream, size_t stream_bytes);
long nblic_amd_index_build(nblic_amd_ctx *ctx, const unsigned char *stream, size_t stream_bytes, int every_rows, unsigned char *out, size_t cap);
int nblic_amd_decode_indexed(nblic_amd_ctx *ctx, const unsigned char *stream, size_t stream_bytes, const void *index, size_t index_bytes,
                             unsigned char *img, size_t img_cap);
int nblic_amd_decode_rows(nblic_amd_ctx *ctx, const unsigned char *stream, size_t stream_bytes, const void *index, size_t index_bytes,
                          int row0, int row1, unsigned char *out, size_t cap);

/* PACKED SEEK INDEX: the same information as a seek index, delta-coded entry against entry and bit-packed (magic
 * "NBLSIDXP"; the format: DESIGN.md section 6).  It converts to and from the index byte for byte, and every function that
 * READS an index takes either form: index_check, decode_indexed, decode_rows and decode_batch_indexed (packed and
 * unpacked indexes in any mix; a packed one is checked in its packed form, as index_check checks it, and expanded on the
 * device only; the seals of the unpacked form it stores are re-derived by index_unpack alone).  Everything that WRITES an
 * index writes the unpacked form; packing is one host call on the result.  All five are host only and need no context.
 *   index_pack         `index` (one nblic_amd_index_check accepts) as a packed index into out.  Returns its size -- written
 *                      only when cap is large enough (nblic_amd_index_pack_bound is) -- or -1: an index the check refuses.
 *   index_pack_bound   no packed form of `index` (its head is read) is larger: its own size + 32 + 33 per entry.  0: not an
 *                      index's head.
 *   index_unpack       the index a packed one stands for into out (cap >= nblic_amd_index_unpacked_bytes).  Every entry is
 *                      re-derived and sealed again; a seal that differs from the stored one is a refusal.  Returns the size
 *                      (with out == NULL or cap too small: the size alone), or -1.
 *   index_unpacked_bytes   from the packed index's head; 0: not a packed index's head.
 *   index_is_packed    1 when the bytes start with the packed magic. */
long nblic_amd_index_pack(const void *index, size_t index_bytes, unsigned char *out, size_t cap);
size_t nblic_amd_index_pack_bound(const void *index, size_t index_bytes);
long nblic_amd_index_unpack(const void *packed, size_t packed_bytes, unsigned char *out, size_t cap);
size_t nblic_amd_index_unpacked_bytes(const void *packed, size_t packed_bytes);
int nblic_amd_index_is_packed(const void *index, size_t index_bytes);

/* INDEXED BATCH ENCODE: many lossless -n0 -e1 images AND their seek indexes in one call.  Image k gets its byte-exact
 * .nblic stream and, when 1 <= every_rows[k] < heights[k], the seek index nblic_amd_index_build(every_rows[k]) would make
 * for that stream, byte for byte -- without the serial decode index_build costs.  A group of images is stepped through
 * row bands together: each launch sequence carries one band of every image of the group (images of different heights,
 * widths and every_rows, at different rows), a slot whose image has ended takes the next image of the batch, and the
 * bins of a step are range-coded on worker threads (as many as the context has coder threads) while the next step is on
 * the GPU.  The device workspace is one band per slot, whatever the heights; it belongs to the context and only grows.
 *   every_rows[k]   0, or >= heights[k]: the image is encoded with no index and index_lens[k] = 0 (index_build refuses
 *                   that geometry too).  A negative value refuses the whole call.
 *   indexes         NULL, or an array whose entries may be NULL: that image's index is not wanted (index_lens[k] = 0).
 *                   index_caps and index_lens are required unless indexes is NULL.  nblic_amd_index_bytes gives the size.
 *   band_rows       rows per band; <= 0 sizes it as nblic_amd_stream_begin does.  A band never crosses a multiple of the
 *                   image's every_rows while its index is being written.  No choice of band_rows shows in the bytes.
 *   per image       out_lens[k] = -1 when out_caps[k] is too small or the size is refused (limits above);
 *                   index_lens[k] = -1 when index_caps[k] is too small -- the stream is still delivered -- or the stream
 *                   failed.  The call returns -1 if any entry is -1, 0 otherwise; the other images are unaffected.
 *   whole call      -1, nothing launched: n_images < 1, a null array or image or output, a negative every_rows, a context
 *                   without a usable device.
 * Lossless -e1 only: near-lossless and efforts 2 / 3 need the serial model stage, a reconstruction and the least-squares
 * statistics per image (nblic_amd_stream_* writes their indexes, one image per object).
 * The call takes groups of the context as a band encoder does -- up to min(groups, ceil(n_images / group size)) of them,
 * each for the whole call -- so it runs next to batches, band coders and decoders of the same context, and blocks while
 * no group is free.  imgs_on_device as for nblic_amd_encode_batch; host planes are hashed where they are (lossless: the
 * reconstruction is the input), device planes have each band's rows copied back for the index's row hash.
 * nblic_amd_index_bytes: the size of the index of a stream of this geometry; host only, no device, no context.  kind 0
 * NBLIC (effort 1..3), 1 QNBLIC (effort 0).  -1 for every_rows < 1 or >= height, or fields out of range.
 * nblic_amd_indexed_batch_split (reporting): the context's last indexed batch of either kind (this call or
 * nblic_amd_qencode_batch_indexed) summed over its group steps -- ms[0] front halves (effort 0: the model stage), [1] totals
 * read-back, [2] back halves and entry records, [3] copies to the host (GPU time, milliseconds), [4] the drivers' wait for
 * the coder threads (host milliseconds); returns the number of group steps, -1 without a context.  The effort-0 batch has no
 * totals read-back and no back half: there [1] reads 0, [2] is the entry records alone, and [4] is the drivers' wait for
 * a free image buffer, which is how its workers hold a driver back. */
int nblic_amd_encode_batch_indexed(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                   const int *heights, const int *widths, const int *every_rows, int band_rows,
                                   unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                   unsigned char *const *indexes, const size_t *index_caps, long *index_lens);
long nblic_amd_index_bytes(int kind, int height, int width, int effort, int every_rows);
long nblic_amd_indexed_batch_split(nblic_amd_ctx *ctx, double ms[5]);

/* INDEXED EFFORT-0 BATCH ENCODE: many QNBLIC images AND their seek indexes in one call.  Image k gets the stream
 * nblic_amd_qencode_batch and QNBLICcompress write for it, byte for byte (outs[k] are uint16_t buffers; capacities and
 * lengths in 16-bit WORDS), and, when 1 <= every_rows[k] < heights[k], the seek index nblic_amd_index_build(every_rows[k])
 * would make for that stream, byte for byte -- nblic_amd_index_bytes(1, h, w, 0, every_rows[k]) bytes -- without the serial
 * decode index_build costs.  A group of images is stepped through row bands together as in nblic_amd_encode_batch_indexed:
 * a launch sequence carries the model stage of one band of every image of the group and the decoder records of the bands
 * that end on an entry row; nothing on the host sizes anything in between, so a group's steps are queued ahead (eight at
 * most) without a wait.  every_rows, indexes, band_rows, the per-image results and what refuses the whole call are exactly
 * nblic_amd_encode_batch_indexed's (above); a stream buffer of fewer than 6 words is refused like a refused size.
 *   per image in flight   an image's histograms are final only with its last band, so its entropy stage -- normalisation,
 *                   histogram code and the rANS pass, on a worker thread of the call (as many as the context has coder
 *                   threads) -- starts when all its level | symbol words are on the host: the call holds 2 bytes per pixel
 *                   of page-locked memory per image in flight, plus 12,352 + 2 x width bytes per entry, plus 1 byte per
 *                   pixel for a device-resident input whose index is wanted (the rows the index hashes).  A group has
 *                   2 x (its slots) such buffers: one per image being stepped and as many for images being coded; a
 *                   slot whose image has ended takes the next image only when a buffer is free.  They belong to the
 *                   context and only grow, as the device workspace (one band per slot) does.
 *   the entries     the rANS pass runs last pixel first, so its state once pixel every_rows x width x j has been coded is
 *                   the state the decoder holds in front of that row; the worker reads state and position off the pass.
 * Lossless effort 0 only: it is the one other mode whose model stage runs on the partitioned kernels and whose
 * reconstruction is the input (near-lossless and efforts 2 / 3: see above).  No choice of band_rows shows in any byte.
 * The call takes groups of the context as nblic_amd_encode_batch_indexed does, each for the whole call, and runs next to
 * batches, band coders and decoders of the same context.  nblic_amd_indexed_batch_split reports it (above). */
int nblic_amd_qencode_batch_indexed(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs, int imgs_on_device,
                                    const int *heights, const int *widths, const int *every_rows, int band_rows,
                                    uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words,
                                    unsigned char *const *indexes, const size_t *index_caps, long *index_lens);

/* INDEXED BATCH DECODE: the segments of many streams, or one row range of each, in one call.  Image k is a stream and its
 * seek index; NBLIC in any mode and QNBLIC, any geometry and any R may share a call.  row0 and row1 both NULL: whole
 * planes; otherwise rows [row0[k], row1[k]) of image k.  outs[k] is a host buffer of out_caps[k] bytes.
 *   host check      nblic_amd_index_check(index, stream) and the stream's description, on worker threads of the call (as
 *                   many as the context has coder threads).  No byte of an image reaches the device before it has passed.
 *   segments        with k0 = row0 / R and k1 the segment that holds row1 - 1, segments k0 .. k1 all run side by side,
 *                   segment 0 from the stream's start and segment s from entry s; the last one stops in front of row1.
 *                   The stream goes up once per image (a row range: from the first entry's feed_from on) and the index
 *                   verbatim, in one copy; a kernel sets every segment up from the uploaded entry (its record, B, the two
 *                   rows above) wherever that entry happens to lie.
 *   job list        all segments of all accepted images form one list (nblic_amd_indexed_decode_plan); the segments of a
 *                   (codec, effort) class share a launch, so a call with many segments takes the decoders' lean image.
 *   rounds          at most 1 GiB of per-segment state per round, and nblic_amd_set_index_round(ctx, n) caps a round at n
 *                   segments here too.  Within an image a higher segment never runs in a later round than a lower one.
 *   verification    every inner boundary of an image is checked ON THE DEVICE: the segment's final record, B and last two
 *                   rows against the next entry (k_index_chain, has the fields).  The last segment of
 *                   a whole plane must end the image, that of a range must stand in front of row1.  Only one word per
 *                   boundary and one 64-byte header per image are read back.
 *   per image       status[k] = 0, or -1: the host check refused it, a row range outside 0 <= row0 < row1 <= height,
 *                   out_caps[k] below (row1 - row0) x width (height x width for a whole plane) -- such an image takes no
 *                   further part in the call and its buffer is not written -- or a boundary differs or a segment fails:
 *                   then outs[k] is zeroed over the bytes that would have been written.  Nothing else is written to outs[k].
 *                   heights / widths / nears / efforts [k] are filled in for every image that passed the host check.
 *   whole call      0 when every status is 0, else -1.  -1 with nothing launched or allocated and status untouched:
 *                   n_images < 1, a null array, stream, index or output, exactly one of row0 / row1 NULL, a context without
 *                   a usable device.
 * The call has a HIP stream and a workspace of its own: the streams, indexes and planes (or row ranges) of all accepted
 * images are in device memory together, so a caller with more than the device holds splits its batch.
 * nblic_amd_indexed_decode_split (reporting): the context's last call as host milliseconds -- ms[0] the host checks,
 * [1] allocation and uploads, [2] the rounds with their chain check, [3] the copies to the host; 0, -1 without a context.
 * nblic_amd_indexed_decode_plan: the job list alone; host only, no device, no context.  Image k is kinds[k] (0 NBLIC,
 * 1 QNBLIC), efforts[k], heights[k] x widths[k], an entry every every_rows[k] rows, rows [row0[k], row1[k]) (both NULL:
 * whole planes); round_segments <= 0: one round.  Job j is the six ints jobs[6 j ..]: image, segment, first row, end_row
 * (0: the image's last row), class (kind * 4 + effort) and round; jobs are listed round by round, class by class within
 * a round, and an image's segments from the last to the first.  Returns the number of jobs (jobs is filled when it is
 * not NULL and jobs_cap, in jobs, suffices), -1 for fields out of range. */
int nblic_amd_decode_batch_indexed(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                   const void *const *indexes, const size_t *index_lens, const int *row0, const int *row1,
                                   unsigned char *const *outs, const size_t *out_caps, int *heights, int *widths, int *nears,
                                   int *efforts, int *status);
int nblic_amd_indexed_decode_split(nblic_amd_ctx *ctx, double ms[4]);
long nblic_amd_indexed_decode_plan(int n_images, const int *kinds, const int *efforts, const int *heights, const int *widths,
                                   const int *every_rows, const int *row0, const int *row1, int round_segments, int *jobs,
                                   size_t jobs_cap);

/* DECODE TO DEVICE MEMORY: a window of every image of a batch straight into caller-owned device memory, as pixels or as
 * normalised floats.  The encoders take device pointers; these two calls are the decoders' counterpart for a consumer on
 * the GPU (a loader that wants a crop of each frame in a batch tensor): no pixel crosses the bus, only the verdict words and
 * one 64-byte header per image reach the host.
 *   the window      rows [row0, row1) x columns [col0, col1) of image k; row1 == 0 / col1 == 0 stand for the image's
 *                   height / width.  The ROWS choose the segments an indexed decode runs, as row0 / row1 of
 *                   nblic_amd_decode_batch_indexed do; the COLUMNS do not shorten the decode (the model needs whole rows),
 *                   they only choose what is delivered.
 *   the destination element (r, c) of the window goes to ptr + r x pitch_bytes + c x element size.  ptr is device memory of
 *                   the context's device and, like pitch_bytes, a multiple of the element size; cap_bytes is what may be
 *                   written from ptr on.  Nothing outside the window's rows is written: pitch gaps stay as they were.
 *   format          0 uint8 (a copy; scale must be 1 and bias 0), 1 float16, 2 bfloat16, 3 float32: float(px) x scale, rounded
 *                   to float, + bias, rounded to float -- never fused -- then rounded to nearest even into the format, so
 *                   numpy's float32(px) * float32(scale) + float32(bias), converted, is the same bits.
 *   delivery        ONE kernel launch (k_deliver) per call (decode_batch_to: per chunk of 64 images)
 *                   delivers every window, after the verification that nblic_amd_decode_batch_indexed makes on the device.
 *   per image       status[k] = 0, or -1.  REFUSED on the host, before anything of it is launched, with its destination not
 *                   written and the other images unaffected: what the host call refuses, and a destination whose ptr the
 *                   runtime (hipPointerGetAttributes) does not report as device memory of the context's device, whose ptr or
 *                   pitch_bytes is no multiple of the element size, whose pitch_bytes is below the window's row, whose window
 *                   is empty or outside the image, or with (rows - 1) x pitch_bytes + cols x element size > cap_bytes or
 *                   beyond the end of the allocation ptr lies in.  FAILED on the device (a boundary differs, the stream is
 *                   damaged or ends early): the window is filled with zero bytes (+0.0, not bias).
 *   whole call      0 when every status is 0, else -1.  -1 with nothing launched: what the host call refuses, a NULL dests,
 *                   an unknown format, a scale or bias that is not finite, uint8 with scale != 1 or bias != 0.  If the device
 *                   fails, every accepted image's window is zeroed where the stream still works and every status is -1.
 * Overlapping destinations are the caller's business: the windows are written in no defined order.  The calls return when
 * the data is complete (they synchronise their own stream), and they order themselves against NOTHING the caller has queued
 * on streams of its own: a destination must not be in use by pending work when the call is made.
 * nblic_amd_decode_batch_indexed_to is nblic_amd_decode_batch_indexed with that delivery in place of the copies to the
 * host (nblic_amd_indexed_decode_split's ms[3] is then the delivery); nblic_amd_decode_batch_to is nblic_amd_decode_batch
 * likewise, each window gated ON THE DEVICE by its image's decoder record: a stream that fails there leaves zeros. */
/* REVERSIBLE COLOUR TRANSFORM: RGB frames in the _from encoders and the _to_ex decoders.  OR'ed into their `format` argument,
 * NBLIC_AMD_FORMAT_RCT makes images 3f, 3f + 1, 3f + 2 of the call the R, G, B of frame f, and the three streams of a
 * frame those of the planes
 *     t_R = (R - G + 128) mod 256,    t_G = G,    t_B = (B - G + 128) mod 256
 * (JPEG-LS's transform; 8-bit wrap-around arithmetic, the offset keeps small differences in mid-range), which the decoders
 * undo on the way out: R = (t_R + G - 128) mod 256, B = (t_B + G - 128) mod 256, then the destination's scale and bias.
 * There is no container and no change to a stream: each of the three is an ordinary .nblic / QNBLIC stream, byte for byte
 * what the same call without the flag returns for the transformed plane, seek index included -- so a decoder that knows
 * nothing of the transform (the reference tool, the calls here without the flag) yields the TRANSFORMED planes.  The
 * transform happens inside k_collect and k_deliver: R and B are collected with the caller's G source
 * as their reference, and delivered with the decoded G plane as theirs.  Lossless only: with near > 0 an error of +-near
 * on a difference plane can wrap to +-255 on R or B.
 *   accepted by     nblic_amd_encode_batch_modes_from (near = 0 for every image), nblic_amd_qencode_batch_from,
 *                   nblic_amd_encode_batch_indexed_from, nblic_amd_qencode_batch_indexed_from, nblic_amd_decode_batch_to_ex,
 *                   nblic_amd_decode_batch_indexed_to_ex.  Every other call takes the flag for an unknown format.
 *   whole call      -1 with nothing launched or written: n_images % 3 != 0; an image with near > 0;
 *                   nblic_amd_encode_batch_modes_from_to (there is no reconstruction of a lossless frame to deliver).
 *   encode          the three sources of a frame have equal rows and cols and one format, scale and bias; the pixel of a
 *                   source element is what it is without the flag, and the differences are taken of those pixels.  A frame
 *                   with a source that is refused, or with sources of unequal size, is refused AS A WHOLE: three empty
 *                   results, nothing launched for it.  R and B are always collected (never used in place); a contiguous
 *                   uint8 G still is.
 *   decode          the three streams of a frame have equal height and width and near = 0; they may differ in codec, effort
 *                   and index.  The three destinations name the same window.  A frame with a refused image or destination
 *                   is refused as a whole and not written; a frame with a plane that fails on the device gets zeros in all
 *                   three windows; either way its three statuses are -1.  nblic_amd_decode_batch_to_ex delivers the colour
 *                   frames of a call in ONE launch behind the work of both of its streams (an event wait), since the
 *                   planes of a frame may be of different (codec, effort) classes.
 * The gain on photographs is UNMEASURED: no colour photograph was at hand (README.md says what was measured instead).
 * The calls with the flag are the _color calls (PER-FRAME COLOUR MODES, below) with every frame's mode NBLIC_AMD_COLOR_RCT. */
#define NBLIC_AMD_FORMAT_RCT 0x100
typedef struct nblic_amd_dest {
    void  *ptr;          /* device memory on the context's device                          */
    size_t pitch_bytes;  /* between rows; >= (col1 - col0) x element size, a multiple of it */
    size_t cap_bytes;    /* readable / writable bytes from ptr                             */
    int    row0, row1, col0, col1;   /* the window; row1 == 0 / col1 == 0: to the image's last row / column */
} nblic_amd_dest;
int nblic_amd_decode_batch_indexed_to(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                      const void *const *indexes, const size_t *index_lens, const nblic_amd_dest *dests, int format,
                                      float scale, float bias, int *heights, int *widths, int *nears, int *efforts, int *status);
int nblic_amd_decode_batch_to(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                              const nblic_amd_dest *dests, int format, float scale, float bias, int *heights, int *widths,
                              int *nears, int *efforts, int *status);

/* DECODE TO ANY DEVICE LAYOUT: the two calls above with a destination that has, like a source of the _from calls below, a
 * step between the elements of a row, and its own normalisation -- the colours of a uint8 [N, H, W, 3] batch, or the
 * channels of a channels-last float16 tensor with a mean and a std per channel, are written where they lie.
 *   the destination element (r, c) of the window goes to ptr + r x pitch_bytes + c x step_bytes, as float(px) x scale + bias
 *                   in the call's format (above).  Nothing else is written: the bytes between the elements and the pitch
 *                   gaps keep their contents.  step_bytes == element size is the destination of the calls above, with their
 *                   rule (pitch_bytes >= the window's row).  step_bytes > element size is a STRIDED destination: it may
 *                   have any pitch_bytes, so a transposed view works.
 *   per image       REFUSED, with its destination not written and the other images unaffected: what the calls above
 *                   refuse, and a destination whose ptr, pitch_bytes or step_bytes is no multiple of the element size or is
 *                   below it; step_bytes > 2^20 or pitch_bytes > 2^40; (rows - 1) x pitch_bytes + (cols - 1) x step_bytes
 *                   + element size > cap_bytes or beyond the end of the allocation ptr lies in; a scale or bias that is
 *                   not finite; uint8 with scale != 1 or bias != 0.
 *   whole call      -1 with nothing launched: what the host call refuses, a NULL dests, an unknown format.
 * The two calls above ARE these calls, with step_bytes = element size and the call's scale / bias in every destination
 * (their whole-call -1 for a scale or bias they refuse stays).  One k_deliver launch carries contiguous and strided
 * destinations mixed.
 * nblic_amd_deliver_stats: out[0] the delivery tasks that the last call on this context that delivers (the four _to calls,
 * nblic_amd_encode_batch_modes_from_to, nblic_amd_debug_deliver, nblic_amd_debug_deliver_ex) queued, out[1] the strided ones among them.  0, -1 for a null pointer. */
typedef struct nblic_amd_dest_ex {
    void  *ptr;          /* device memory on the context's device                              */
    size_t pitch_bytes;  /* between rows                                                       */
    size_t step_bytes;   /* between neighbouring elements of a row (element size: contiguous)  */
    size_t cap_bytes;    /* writable bytes from ptr                                            */
    int    row0, row1, col0, col1;   /* the window; row1 == 0 / col1 == 0: to the image's last row / column */
    float  scale, bias;  /* float formats: float(px) x scale + bias; uint8: 1 and 0            */
} nblic_amd_dest_ex;
int nblic_amd_decode_batch_indexed_to_ex(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                         const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                         int *heights, int *widths, int *nears, int *efforts, int *status);
int nblic_amd_decode_batch_to_ex(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                 const nblic_amd_dest_ex *dests, int format, int *heights, int *widths, int *nears, int *efforts,
                                 int *status);
int nblic_amd_deliver_stats(nblic_amd_ctx *ctx, long out[2]);

/* ENCODE FROM DEVICE MEMORY: the batch encoders on images that lie in caller-owned device memory in ANY layout -- a crop
 * of a larger frame, a pitched surface, one channel of an [N, C, H, W] tensor, one colour of an interleaved H x W x 3 frame
 * -- as pixels or as floats that are quantised to 8 bits on the way.  The counterpart of the two calls above: a batch goes
 * device memory -> streams (+ seek indexes) -> device memory without a pixel in host memory of the caller's.
 *   the source      element (r, c) of image k is read at ptr + r x pitch_bytes + c x step_bytes.  The image IS the window: a
 *                   crop offsets ptr.  ptr is device memory of the context's device; ptr, pitch_bytes and step_bytes are
 *                   multiples of the element size and not below it; cap_bytes is what may be read from ptr on.  Nothing
 *                   outside the elements of the image is read: pitch gaps and the bytes between the pixels are not touched.
 *   format          0 uint8 (the pixel is the element; scale must be 1 and bias 0), 1 float16, 2 bfloat16, 3 float32: the
 *                   pixel is float(x) x scale, rounded to float, + bias, rounded to float -- never fused -- NaN to 0,
 *                   everything else clamped to [0, 255] and rounded to nearest, ties to even: numpy's
 *                   clip(rint(float32(x) * float32(scale) + float32(bias)), 0, 255) with NaN as 0 is the same bits.
 *                   "Lossless" means lossless with respect to this collected plane.
 *   collection      a uint8 source with step_bytes == 1 and pitch_bytes == cols is used where it lies, at the cost of
 *                   imgs_on_device = 1.  Every other one is written into the workspace of the slot that encodes it -- the
 *                   buffer a host plane is uploaded into -- by k_collect: ONE launch for the images of
 *                   a group's front half, and in the indexed calls one per group step, for the rows of the step's bands.
 *   per image       REFUSED on the host, before anything of it is launched, with the other images unaffected -- out_lens[k]
 *                   = -1 and, in the indexed calls, index_lens[k] = -1: rows or cols the encoder does not take; a ptr,
 *                   pitch_bytes or step_bytes that is no multiple of the element size or is below it; step_bytes > 2^20 or
 *                   pitch_bytes > 2^40; (rows - 1) x pitch_bytes + (cols - 1) x step_bytes + element size > cap_bytes or
 *                   beyond the end of the allocation ptr lies in; a ptr the runtime (hipPointerGetAttributes) does not
 *                   report as device memory of the context's device.
 *   whole call      -1 with nothing launched: what the parent call refuses, a NULL srcs, an unknown format, a scale or bias
 *                   that is not finite, uint8 with scale != 1 or bias != 0.
 * Sources may overlap: they are only read.  The calls return when the streams are complete, and they order themselves
 * against NOTHING the caller has queued on streams of its own: a source must not be in use by pending work when the call is
 * made, and must stay valid and unchanged until it returns.
 * Each call is its parent -- nblic_amd_encode_batch_modes (NULL nears / efforts: -n0 -e1 on the staged pipeline; recons stay
 * host buffers), nblic_amd_qencode_batch, nblic_amd_encode_batch_indexed, nblic_amd_qencode_batch_indexed -- with srcs,
 * format, scale, bias in place of imgs, imgs_on_device, heights, widths, and returns byte for byte what the parent returns
 * for the collected planes, indexes included.  There is no asynchronous _begin / _end pair and no nblic_amd_stream_* on
 * sources; reconstructions go to device memory by nblic_amd_encode_batch_modes_from_to.
 * nblic_amd_collect_stats: since the context was created, out[0] images used in place, [1] images collected, [2] k_collect
 * launches, [3] pixels collected.  Returns 0, -1 for a null pointer.
 * nblic_amd_collect_ms: while nblic_amd_enable_timing is on, a k_collect launch stands between two events of its group;
 * *ms is the GPU time of the launches timed since the context was created and *timed_launches their number (a group has
 * one pair of events, so of the steps that an indexed effort-0 batch queues ahead only those that find it free are
 * timed).  Call it when no batch is outstanding.  Returns 0, -1 for a null pointer. */
typedef struct nblic_amd_src {
    const void *ptr;        /* element (0, 0) of the image, device memory of the context's device */
    size_t pitch_bytes;     /* between rows                                                        */
    size_t step_bytes;      /* between neighbouring pixels of a row (element size: contiguous)     */
    size_t cap_bytes;       /* readable bytes from ptr                                             */
    int    rows, cols;      /* the image: height and width of what is encoded                      */
} nblic_amd_src;
int nblic_amd_encode_batch_modes_from(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                      const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps,
                                      long *out_lens, unsigned char *const *recons);
int nblic_amd_qencode_batch_from(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                 uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words);
/* RECONSTRUCTIONS TO DEVICE MEMORY: nblic_amd_encode_batch_modes_from with, in place of the host recons, one
 * nblic_amd_dest_ex per image (above: window, pitch, step, scale and bias as for a decode) and their format: the plane a
 * decoder of the stream produces goes to the caller's device memory next to the source, and no plane reaches the host.
 * A destination with a NULL ptr asks for no reconstruction of its image.
 *   what is delivered  near > 0: the reconstruction the model stage keeps on the device.  near == 0: the plane that was
 *                   encoded -- the collected one, or the source where it lies.
 *   delivery        after the model stage of a group's images, ONE k_deliver launch on the group's own stream.  In the serial
 *                   modes (near > 0, or effort 2 / 3) a task is gated by the model's record: an image that fails there
 *                   leaves zeros in its window.
 *   per image       a destination that the _to_ex calls would refuse costs THAT IMAGE'S RECONSTRUCTION ONLY: it is not
 *                   written, and the image's stream is written as if none had been asked for.  A refused source has neither.
 *   whole call      -1 with nothing launched: what nblic_amd_encode_batch_modes_from refuses, a NULL recons, an unknown
 *                   recon_format.
 * The streams are byte for byte those of nblic_amd_encode_batch_modes_from.  nblic_amd_deliver_stats counts the call's
 * tasks.  There is no such call for QNBLIC (lossless: the reconstruction is the source), the indexed encoders or
 * _begin / _end. */
int nblic_amd_encode_batch_modes_from_to(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                         const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps,
                                         long *out_lens, const nblic_amd_dest_ex *recons, int recon_format);
int nblic_amd_encode_batch_indexed_from(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale,
                                        float bias, const int *every_rows, int band_rows, unsigned char *const *outs,
                                        const size_t *out_caps, long *out_lens, unsigned char *const *indexes,
                                        const size_t *index_caps, long *index_lens);
int nblic_amd_qencode_batch_indexed_from(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale,
                                         float bias, const int *every_rows, int band_rows, uint16_t *const *outs,
                                         const size_t *out_caps_words, long *out_len_words, unsigned char *const *indexes,
                                         const size_t *index_caps, long *index_lens);
int nblic_amd_collect_stats(nblic_amd_ctx *ctx, long out[4]);
int nblic_amd_collect_ms(nblic_amd_ctx *ctx, double *ms, long *timed_launches);

/* BATCH INDEX BUILD: the seek indexes of many streams from ONE decode pass.  nblic_amd_index_build takes one stream per
 * call and pays a host round trip at every band and every entry; this call takes n streams -- NBLIC in any mode and QNBLIC,
 * written by this library or by the reference; any mix of geometries and of R = every_rows[k] -- and writes into
 * indexes[k] (index_caps[k] bytes; nblic_amd_index_bytes gives the size) byte for byte what
 * nblic_amd_index_build(stream k, every_rows[k]) writes.  planes (may be NULL, and so may its entries) receives the decoded
 * planes, so decoding an archive and indexing it costs one pass; plane_caps is required unless planes is NULL.
 *   host check      the stream's description, on worker threads of the call (as many as the context has coder threads).
 *                   No byte of an image reaches the device before it has passed.
 *   decode pass     every accepted stream goes up once and is decoded whole, the images of a (codec, effort) class side
 *                   by side in the same launches (more than 256 of a class: the decoders' lean image).  A job stops in
 *                   front of each of its entry rows; after every decode launch a capture kernel turns the device state of
 *                   the jobs that stand there into the entries' bodies (record, B, the two rows above) and lets them go on.
 *   schedule        a job's progress is known beforehand while it does not fail, so the launches of the whole call are
 *                   laid out on the host first (nblic_amd_index_build_plan), uploaded once and queued back to back: the
 *                   host waits once.  nblic_amd_set_serial_rows bounds the rows of a launch here too, and shows in no byte.
 *   finish          worker threads fetch each image's staged bodies and its plane in one copy each and write the index:
 *                   heads, the canonical running SHA-256 of the rows above every entry, the QNBLIC tables, the seals.
 *   per image       status[k] = 0 and index_lens[k] = the index's size, or status[k] = -1 and index_lens[k] = -1: not a
 *                   stream this library decodes, every_rows[k] < 1 or >= height (as nblic_amd_index_build refuses it),
 *                   index_caps[k] or plane_caps[k] too small -- such an image takes no further part in the call and its
 *                   buffers are not written -- or the stream does not decode to its end: then indexes[k] (and planes[k])
 *                   are zeroed over the bytes that would have been written.  Nothing else is written to them.
 *                   heights / widths / nears / efforts [k] are filled in for every stream whose description passed.
 *   whole call      0 when every status is 0, else -1.  -1 with nothing launched or allocated and status untouched:
 *                   n_images < 1, a null array (planes excepted), stream or index buffer, a context without a usable device.
 * The call has a HIP stream of its own for the uploads and launches, up to four more for the finish's copies, and one
 * workspace, so it runs next to everything else of its context.  All accepted
 * images are in device memory together -- per image its stream, its whole plane, one decoder record, [B | F] and a staging
 * buffer for its entries' bodies -- so a caller with more than the device holds splits its batch.
 * nblic_amd_index_build_split (reporting): the context's last call as host milliseconds -- ms[0] the host checks,
 * [1] allocation, uploads and seeding, [2] the decode and capture launches, [3] the finish; 0, -1 without a context.
 * nblic_amd_index_build_plan: the schedule alone; host only, no device, no context.  Image k is kinds[k] (0 NBLIC,
 * 1 QNBLIC), efforts[k], heights[k] x widths[k], an entry every every_rows[k] rows; serial_rows as
 * nblic_amd_set_serial_rows (0: automatic).  class_launches (may be NULL) receives eight ints: the decode launches of class
 * kind * 4 + effort.  Entry j is the four ints entries[4 j ..]: image, entry row, class, and the 0-based decode launch of
 * that class behind which it is captured; entries are listed class by class and, within a class, by that launch.
 * Returns the number of entries (entries is filled when it is not NULL and entries_cap, in entries, suffices), -1 for
 * fields out of range. */
int nblic_amd_index_build_batch(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                const int *every_rows, unsigned char *const *indexes, const size_t *index_caps, long *index_lens,
                                unsigned char *const *planes, const size_t *plane_caps, int *heights, int *widths, int *nears,
                                int *efforts, int *status);
int nblic_amd_index_build_split(nblic_amd_ctx *ctx, double ms[4]);
long nblic_amd_index_build_plan(int n_images, const int *kinds, const int *efforts, const int *heights, const int *widths,
                                const int *every_rows, int serial_rows, int *class_launches, int *entries, size_t entries_cap);

/* The reference's decoders take no stream length (src/NBLIC.h:72, src/QNBLIC.h:16).  NBLICdecompress / QNBLICdecompress
 * therefore run a band decoder (nblic_amd_dstream above, band_rows as set by nblic_amd_set_serial_rows) and fetch the
 * caller's stream ON DEMAND in steps of `bytes` (default 1 MiB, at least 4096): the decoder stops in front of a row when
 * it is about to run short, the next step is copied in, it resumes.  No byte beyond the last one the decoder consumes
 * plus one step and the starvation margin is read, and each step is copied by the kernel (a pipe write), so a stream
 * that ends right in front of an unmapped page is read exactly to its end instead of faulting.  There is no cap on the
 * stream's length, the device workspace is the band decoder's, and the rows are written into p_img as they finish
 * (after a failure, those decoded before it may be there).  ctx == NULL: the drop-in context.
 * nblic_amd_last_fed_bytes: how many bytes the last drop-in decode read from the caller's buffer.                      */
void nblic_amd_set_feed_chunk(nblic_amd_ctx *ctx, size_t bytes);
long nblic_amd_last_fed_bytes(nblic_amd_ctx *ctx);

/* Per-kernel device times of the LAST nblic_amd_encode_batch: one HIP event in front of every
 * launch, on the stream the kernel runs on, summed over the batch's group launches (divide by
 * nblic_amd_last_launches() for the average launch duration).  Writes up to `cap` entries
 * of milliseconds into ms[] and matching static strings into names[]; returns the count.
 * Timing is recorded only after nblic_amd_enable_timing(ctx, 1) (every stage) or (ctx, 2): only
 * k_predict and k_touch_scatter, the two stages the bench line reports against a roof -- thirty-two
 * events per group launch cost the pipeline 2 % of its throughput, four do not; untimed stages read 0. */
void nblic_amd_enable_timing(nblic_amd_ctx *ctx, int on);
int nblic_amd_stage_times(nblic_amd_ctx *ctx, double *ms, const char **names, int cap);

/* How many group launches the last batch took (each kernel of the sequence is launched once
 * per group of images); the entries of nblic_amd_stage_times() are sums over these launches. */
long nblic_amd_last_launches(nblic_amd_ctx *ctx);

/* Bins coded / host range-coder seconds summed over the last batch (for reporting). */
void nblic_amd_last_stats(nblic_amd_ctx *ctx, double *total_bins, double *coder_seconds_sum);

/* Stage-level debug hook used by the parity tests: runs the staged -e1 pipeline on ONE host
 * image and copies the named intermediate array back.  which: 0 rec1(u32) 1 pxs(u16) 2 z(u8)
 * 3 cnt(u8) 4 events(u32) 5 coded(u16).  Returns the element count, or -1.                 */
long nblic_amd_debug_stage(nblic_amd_ctx *ctx, const unsigned char *img, int height, int width, int which,
                           void *out, size_t out_bytes);

/* Debug hook used by the leak tests: what the library holds right now, over every context of the process --
 * counts[0] device allocations, [1] runtime-pinned host allocations, [2] page-locked host buffers of the coder threads
 * and band encoders, [3] streams + events.  Needs no context and makes no GPU call.                                  */
void nblic_amd_debug_live(long counts[4]);

/* Debug hook used by the workspace-history tests: a read-only report of the grow-only device workspaces, so that a test
 * can tell that a call ran in the memory an earlier call left (capacities and addresses unchanged) and not in fresh one.
 * group >= 0: slot `slot` of group `group` --
 *   out[0] px_cap, out[1] ev_cap: entries the pixel-sized / event-sized buffers hold   out[2] bytes of the slot's pool
 *   out[3], out[4] the addresses of rec1 and events, as integers (0: not allocated yet)
 *   out[5], out[6], out[7] capacities of the slot's image copy (bytes), reconstruction (bytes) and LSQ statistics (doubles)
 * group < 0 (slot is ignored): the context --
 *   out[0] coded-bin buffers, out[1] how many of them hold memory, out[2] their summed capacity in 16-bit records
 *   out[3] pack buffers, out[4] how many of them hold memory, out[5] their summed capacity in 64-bit words
 *   out[6] bytes of the decode arena   out[7] job records the decode batches' device array holds
 * Launches nothing, allocates nothing and changes nothing; call it while no batch of the context is in flight.  Returns
 * 0, -1 for a null pointer or a group / slot the context does not have.                                              */
int nblic_amd_debug_workspaces(nblic_amd_ctx *ctx, int group, int slot, long out[8]);

/* Debug hook used by the hand-over tests: takes[k] = how many times a host coder thread took k images together since
 * the last batch began (k = 0..24; 1 = an image on its own, the scalar coder; more = whole packs).               */
void nblic_amd_debug_takes(nblic_amd_ctx *ctx, long takes[25]);

/* Debug hook used by the hand-over tests: runs 2..8 host images as ONE pack of one group launch (the context's groups
 * must have that many slots) and copies the pack's device rows back -- rows[(13 g + j) * 8 + lane], 13-bit groups of
 * lane `lane`, PackRows in csrc/hip_owned.h -- then runs the same images unpacked and copies every image's u16 records
 * to coded[k] (n_bins[k]: capacity in, count out).  Returns the 64-bit words written to rows, or -1.                 */
long nblic_amd_debug_pack_rows(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *imgs, const int *heights, const int *widths,
                               unsigned long long *rows, size_t rows_words, unsigned short *const *coded, unsigned int *n_bins);

/* Debug hook used by the device coder's tests: ONE launch of the range coder's kernel (csrc/device_coder.hip, one wave
 * lane per job) on jobs the caller supplies, 1..4096 of them.  Job k is
 *   an image on its own  (records[k] != NULL): record_words[k] u16 records, prob | bin << 15, which the caller has padded
 *     to the end of the last 512-byte window of its n_bins[k] bins (an empty stream: to one whole window);
 *   a lane of a pack     (records[k] == NULL): lane lane_of[k] (0..7) of pack pack_of[k] (0..n_packs-1); pack p is
 *     pack_words[p] 64-bit words, a multiple of 104, rows[(13 g + j) * 8 + lane] as above, and holds at least the
 *     13 * ceil(n_bins[k] / 64) word rows of the job's groups.
 * Records and rows are uploaded verbatim (256-byte aligned): every word the kernel reads is the caller's.  Job k codes
 * n_bins[k] bins into a device buffer of caps[k] bytes that is followed by a guard of at least 64 patterned bytes;
 * lens[k] is the byte count (flush included) and outs[k], caps[k] bytes, receives them -- or lens[k] is -1: caps[k] was
 * too small.  Returns 0; -1 for arguments it refuses (a null pointer, a lane above 7, a pack index out of range, rows or
 * records shorter than stated above; nothing is launched); -2 when a HIP call failed; -3 when a byte outside what the
 * kernel may write -- a guard, or an output's bytes beyond the length it reported -- has changed.                      */
int nblic_amd_debug_device_code(nblic_amd_ctx *ctx, int n_jobs, const unsigned short *const *records, const size_t *record_words,
                                const int *pack_of, const int *lane_of, int n_packs, const unsigned long long *const *pack_rows,
                                const size_t *pack_words, const unsigned int *n_bins, const unsigned int *caps,
                                unsigned char *const *outs, long *lens);

/* The device rANS stage of effort 0 (csrc/q_device_coder.hip, k_q_rans_lanes: one wave lane per image, launches that
 * resume from a record in device memory; the lane's arithmetic and resumption are csrc/q_rans.h, shared with the host).
 *
 * nblic_amd_set_device_qcoder puts it into the batch pipeline.  ctx == NULL addresses the drop-in context.  mode:
 *   0  host (the default): effort-0 images are coded by the host coder threads, as without this call; the thread sleeps
 *   1  device: every effort-0 image of nblic_amd_qencode_batch and of the QNBLIC*compress drop-ins goes to the device
 *      stage; the coder threads take none
 *   2  shared: the device thread takes the newest waiting effort-0 images, all but one per host coder thread, and only
 *      while no host coder thread is idle.  Bytes are identical; who codes which image is a race
 * One thread per context (started by the first call that names mode 1 or 2) keeps a rolling list of jobs on one stream;
 * every launch advances every job by at most symbols_per_launch symbols (0: the default), and two launches are queued
 * per wait while no image waits to be admitted.  Returns the mode set, or -1.  To be called between batches.
 * Sizing n_host_buffers (nblic_amd_create_ex) for mode 1: an image being coded on the device holds its coded-bin buffer,
 * 2 bytes per pixel of HBM, for as long as its lane takes -- pixels / lane rate, seconds for a large frame -- and the
 * model stage waits for a free buffer before it launches an image.  So n_host_buffers is the number of lanes that can
 * be in flight: give it the batch size (or as many images as the HBM left over holds) or the model stage is throttled
 * to the lanes' pace.  nblic_amd_qencode_batch_indexed does not use the device stage.
 * nblic_amd_device_qcoder_stats: totals since the context was created -- symbols coded by retired jobs, kernel launches,
 * images, and the GPU time between the first and the last launch of every wait, in ms.  Returns 0, or -1.
 *
 * The three calls below run the stage on its own.
 *
 * nblic_amd_qcoder_selftest: the kernel's quotient routines (floor(x / f) without a divide) on the device against 64-bit
 * division, for every f in 1 .. 32767 crossed with 1 << 16, 2^32 - 1, the powers of two and their neighbours, 4096
 * xorshift values and (1 << 17) * f with its two neighbours.  ctx == NULL: the drop-in context.  Returns the number of
 * mismatches, or -1.
 *
 * nblic_amd_debug_q_rans_host: host only, no context.  QNBLIC's entropy stage on height x width caller-made words
 * (level | symbol << 8) and their 12 x 256 raw counts, with the pass run by ONE lane of csrc/q_rans.h that stops every
 * symbols_per_launch symbols (<= 0: never) and resumes from its record.  Returns the stream's words (front matter
 * included; the bytes of nblic_amd_debug_q_entropy), -1 when cap_words is too small, -2 for arguments it refuses.
 *
 * nblic_amd_debug_device_q_entropy: a resumed launch sequence of k_q_rans_lanes on 1 .. 4096 caller-made jobs.  Job k is
 * n_symbols[k] words (1 .. 1 << 24), which the caller has padded to the end of the last 512-byte window -- words[k] holds
 * ceil(n / 256) * 256 of them and all are uploaded verbatim, 256-byte aligned; the kernel fetches the padding and must
 * not use it -- and the 12 x 256 raw counts hists[k].  outs[k] has room for caps_words[k] words.  The front matter is
 * written there by the host (its header names the image of n pixels whose width is the largest divisor of n below
 * 65536; an n without two sides below 65536, such as a prime above 65535, is refused with -1); the lane gets a device region of what is left, followed by a guard of at least 64 patterned bytes, and every
 * launch advances every unfinished job by symbols_per_launch symbols (0: the default).  lens[k] is the stream's words,
 * or -1: caps_words[k] was too small (a job without room for its front matter is not launched at all).
 * Returns 0; -1 for arguments it refuses (a null pointer, a word that names a level above 11 or a symbol its histogram
 * does not count, sizes out of range, more than 8192 launches; nothing is launched); -2 when a HIP call failed; -3 when
 * a guard byte, or a byte of a region in front of the words it reported, has changed.                                   */
int nblic_amd_set_device_qcoder(nblic_amd_ctx *ctx, int mode, long symbols_per_launch);
int nblic_amd_device_qcoder_stats(nblic_amd_ctx *ctx, double *symbols, long *launches, long *images, double *kernel_ms);
int nblic_amd_qcoder_selftest(nblic_amd_ctx *ctx);
long nblic_amd_debug_q_rans_host(int height, int width, const uint16_t *words, const unsigned int *hist, long symbols_per_launch,
                                 uint16_t *out, size_t cap_words);
int nblic_amd_debug_device_q_entropy(nblic_amd_ctx *ctx, int n_jobs, const uint16_t *const *words, const unsigned int *n_symbols,
                                     const unsigned int *const *hists, const size_t *caps_words, long symbols_per_launch,
                                     uint16_t *const *outs, long *lens);

/* Debug hook used by the chain kernels' tests: ONE launch sequence of the staged model stages BEHIND S1 on n records the
 * caller supplies (1 .. 1 << 22), as one job.  x[n] are the pixel values, rec1[n] the S1 records, both uploaded verbatim.
 *   model 0 (NBLIC -e1): rec1 is csrc/model.h pack_s1 (px0 | adr << 8 | qw << 19 | qu's low bit << 24 | qv_rel << 25).  Runs
 *     k_adr_count -> scan -> k_adr_scatter -> k_plan_blocks -> k_bias_blocks -> k_bias_fixup -> k_map_count -> scan ->
 *     k_map_scatter -> k_mapper_chains -> k_count_bins -> scan: what the front half runs behind k_predict.  Writes
 *     pxs[n] (px | sign << 8), z[n], cnt[n], blk_base[2049], ctx_state_out[2048], map_state_out[512 * 60]; qhist is unused.
 *   model 1 (QNBLIC): rec1 is px0 | adr << 8 with adr < 3072.  Runs k_adr_count -> scan -> k_adr_scatter -> k_plan_blocks ->
 *     k_bias_blocks -> k_bias_fixup -> k_q_symbols: what the model stage runs behind k_q_predict.  Writes pxs[n]
 *     (level | symbol << 8), qhist[12 * 256], blk_base[3073], ctx_state_out[3072]; z, cnt and map_state_out are unused and
 *     map_state_in must be NULL.
 * Both write blk_ok[blk_base[keys]], one byte per 4096-record block of every context chain in key order: 1 = the block's
 * warm-up copies met (or it is the chain's first block).  blk_ok_cap, its capacity, must be at least n / 4096 + keys.
 * ctx_state_in / map_state_in: NULL = the tables of an image's first row (k_init_state); otherwise they are uploaded
 * and the chains start from them, as a row band's do (when every table the model has is given, k_init_state is not
 * launched).  Buffers are the workspace of a group slot of the context (counted by nblic_amd_debug_live).
 * Returns 0; -1, with nothing launched or allocated, for what it refuses: a null pointer, n outside the range, blk_ok_cap
 * too small, a record S1 cannot write (model 0: a bit above 26, qv_rel 3, qw > 16, qv outside 0..15; model 1: an address
 * >= 3072 or a bit above it), a table no sequence of records leaves (|bias| > 32576, model 1: > 1 << 20; re-mapper tables
 * that are not inverse permutations of 0..19, a negative hit count); -2 when a HIP call failed.                          */
int nblic_amd_debug_model_stages(nblic_amd_ctx *ctx, int model, size_t n, const unsigned char *x, const unsigned int *rec1,
                                 const int *ctx_state_in, const int *map_state_in, unsigned short *pxs, unsigned char *z,
                                 unsigned char *cnt, unsigned int *qhist, unsigned int *blk_base, unsigned char *blk_ok,
                                 size_t blk_ok_cap, int *ctx_state_out, int *map_state_out);

/* Debug hook used by the chain kernels' tests: ONE launch sequence of the back half BEHIND k_emit_bins on n_ev bin events
 * the caller supplies (1 .. 1 << 22; csrc/model.h pack_event: qu | qv << 4 | node << 8 | qw << 16 | bin << 21), uploaded
 * verbatim, as one job on its own (not packed): k_touch_count -> scan -> k_touch_scatter -> k_plan_windows ->
 * k_counter_epochs -> k_counter_probs -> k_mix.  Writes coded[n_ev] (prob | bin << 15), cnt_state_out[4096 * 2]
 * (c0, c1 per counter, counter = parity * 2048 + (tree >> 1) * 256 + node) and totals[8] (the job's totals words:
 * [3] the touch count, [4] 1 = 32-bit touch positions were used).  cnt_state_in: NULL = every counter (32, 32);
 * otherwise uploaded, k_init_state is not launched.
 * Equal trees with a non-zero qw are accepted: the binarisation walk (model.h walk_symbol) sets qv = qu when the two
 * levels fall into different groups of k_step levels, and again after every escalation, while the event keeps the
 * pixel's qw -- such an event touches its one counter twice, with 32 - qw and then qw.  quantise() also gives
 * qv = qu + 1 with qw 0 (the second touch is dropped).
 * Returns 0; -1, with nothing launched or allocated, for a null pointer, n_ev outside the range, an event the walk cannot
 * emit (|qu - qv| > 1, qw > 16, a bit above 21 -- where a level above 15 would end up) or a counter no sequence of
 * touches leaves (c0 or c1 < 1, c0 + c1 > 8192); -2 when a HIP call failed.                                            */
int nblic_amd_debug_back_half(nblic_amd_ctx *ctx, size_t n_ev, const unsigned int *events, const int *cnt_state_in,
                              unsigned short *coded, int *cnt_state_out, unsigned int *totals);

/* Debug hook used by the entropy front's tests: ONE launch sequence of what a serial-mode band of the band encoder runs
 * between k_serial_model and the host coder, on n records the caller supplies (1 .. 1 << 22), as one job of 1 x n pixels.
 * x[n] are the pixel values, rec1[n] the S1 records (csrc/model.h pack_s1; only the levels and qw are read), pxs[n] the
 * corrected predictions px | sign << 8 -- what k_serial_model leaves per pixel -- all uploaded verbatim; near is 0..9.
 * The job record is filled as the encoders fill it, which pairs k_step = clip(3 + 2 near, 3, 16) and its level table
 * with near; then k_map_count_pre -> scan -> k_map_scatter<general> -> k_mapper_chains -> k_count_bins<general> -> scan,
 * the event total is read, the event-sized buffers are sized, and k_emit_bins<general> -> k_touch_count -> scan ->
 * k_touch_scatter -> k_plan_windows -> k_counter_epochs -> k_counter_probs -> k_mix (unpacked) follow.
 * Writes z[n], cnt[n] (bins per record), pos3[n] (the record's place in the re-mapper partition, or 0x80000000 | y for a
 * symbol >= 20), ev_off[n] (exclusive scan of cnt), events[total] (pack_event words), coded[total] (prob | bin << 15),
 * map_state_out[512 * 60], cnt_state_out[4096 * 2] and totals[8] (the job's totals words: [1] records in the re-mapper
 * partition, [2] events, [3] touches, [4] 1 = 32-bit touch positions).  events_cap is the capacity of events and coded.
 * map_state_in / cnt_state_in: NULL = the tables of an image's first row (k_init_state); otherwise uploaded, and the
 * chains start from them, as a later band's do (when both are given k_init_state is not launched).
 * There is no free k_step: the encoder kernels are valid for the paired step only -- near 0 with k_step 16 would need 256
 * bins for symbol 255, and cnt is a byte.  (The decoders take any pair; tests/test_foreign_streams.py.)
 * Returns 0; -1, with nothing launched or allocated, for what it refuses: a null pointer, n outside the range, near
 * outside 0..9, a pxs word >= 512, a record nblic_amd_debug_model_stages refuses, a table it or nblic_amd_debug_back_half
 * refuses; -2 when a HIP call failed; -3 when the event total (then in totals[2]) exceeds events_cap: the back half was
 * not launched and no other output is written.                                                                        */
int nblic_amd_debug_entropy_front(nblic_amd_ctx *ctx, size_t n, const unsigned char *x, const unsigned int *rec1,
                                  const unsigned short *pxs, int near, const int *map_state_in, const int *cnt_state_in,
                                  unsigned char *z, unsigned char *cnt, unsigned int *pos3, unsigned int *ev_off,
                                  unsigned int *events, size_t events_cap, unsigned short *coded, int *map_state_out,
                                  int *cnt_state_out, unsigned int *totals);

/* Debug hook used by the indexed batch decode's tests: ONE launch of k_index_seed, or of k_index_chain, on caller-made
 * bytes.  `index` (one nblic_amd_index_check accepts) is uploaded at byte base_offset (0 .. 4096) of a larger zeroed
 * buffer, so the caller chooses the residue of every entry's address; `entry` is 1-based, 0 = segment 0 (seed only).
 *   seed (final_rec, final_b, final_rows and verdict all NULL): the task of segment `entry` with SerialState::avail =
 *       avail and, for entry 0, pos = first_pos.  Writes rec_out (the record: 86,080 bytes, QNBLIC 12,352), stats_out
 *       ([B | F]: 2 x (512 / 1024 x width) bytes at -e2 / -e3, else nothing) and rows_out: the 2 x width bytes of a plane
 *       that holds rows [r - 2, r) of the entry's row r, filled with 0xA7 before the launch.
 *   chain (verdict != NULL): final_rec, final_b (may be NULL when the mode has no B) and final_rows -- the plane rows
 *       [r - n, r), n = min(r, 2) -- are uploaded as a segment's final state and compared with `entry`; *verdict = 0, or
 *       the OR of 1 (record), 2 (B), 4 (rows).  Nothing else is written.
 * Every device output is followed by a patterned guard.  Returns 0; -1, with nothing launched or allocated: a null
 * pointer, an index that is refused, entry outside the index, a final_* buffer shorter than the kernel reads; -2 when a
 * HIP call failed; -3 when a byte behind an output has changed. */
int nblic_amd_debug_index_kernels(nblic_amd_ctx *ctx, const void *index, size_t index_bytes, size_t base_offset, int entry,
                                  unsigned long long avail, unsigned long long first_pos, unsigned char *rec_out,
                                  unsigned char *stats_out, unsigned char *rows_out, const unsigned char *final_rec,
                                  size_t final_rec_bytes, const unsigned char *final_b, size_t final_b_bytes,
                                  const unsigned char *final_rows, size_t final_rows_bytes, unsigned int *verdict);

/* Debug hook used by the batch index build's tests: ONE launch of k_index_capture, one task, on caller-made bytes.
 * `record` (86,080 bytes; QNBLIC 12,352), `b` (512 / 1024 x width bytes at -e2 / -e3, else none) and `rows` -- the plane rows
 * [row - n, row), n = min(row, 2), uploaded at byte plane_offset (0 .. 4096) of a zeroed buffer -- are the state of a job
 * whose end_row is `row`.  body_out receives the staged body, record | B | the 2 x width row slot; *end_row_out the job's
 * end_row after the launch (next_end when the task acted).  A record whose status is not 0 or whose next_row is not `row`
 * makes the task write nothing: body_out is then all 0xA7, the pattern the output held before, and *end_row_out = row.
 * The output is followed by a patterned guard.  Returns 0; -1, with nothing launched or allocated: a null pointer, kind /
 * effort / width / row out of range, a buffer whose size is not what the geometry says, body_cap too small; -2 when a HIP
 * call failed; -3 when a byte behind the output has changed. */
int nblic_amd_debug_index_capture(nblic_amd_ctx *ctx, int kind, int effort, int width, int row, int next_end,
                                  const unsigned char *record, size_t record_bytes, const unsigned char *b, size_t b_bytes,
                                  const unsigned char *rows, size_t rows_bytes, size_t plane_offset, unsigned char *body_out,
                                  size_t body_cap, int *end_row_out);

/* Debug hook used by the packed index's device tests: ONE launch of k_index_unpack_scan and ONE unpack launch
 * (k_index_unpack, then k_index_unpack_rank) over n packed indexes (1 .. 8) as n tasks, set up and placed in the launches as
 * nblic_amd_decode_batch_indexed does it.  Index k is uploaded at byte base_offsets[k] (0 .. 4096) of a zeroed, larger
 * buffer, so the caller chooses the residue of its address; its entries 0 .. walks[k] - 1 (0-based; 1 <= walk <= count) are
 * walked and those from first_outs[k] (0 <= first_out < walk) on are stored, out_strides[k] bytes apart: each the entry's
 * body without the QNBLIC tables, record | B | the row slot; the bytes between its end and the stride are not defined.
 * outs[k] receives these (walk - first_out) x out_stride bytes and, behind them, the first 256 bytes of the patterned
 * guard as they were read back; caps[k] must hold both.  The device buffer holds 0xA7 everywhere before the launch.
 *
 * The hook accepts EXACTLY what the kernels' memory safety rests on: the structural walk of the packed form (every length,
 * flag, width byte and hash) and a sound index head.  It does NOT apply the checks nblic_amd_index_check makes on the
 * values of the tables (counter ranges, re-mapper bytes, finite B, the QNBLIC tables): the tests feed the kernels packings
 * of values those checks refuse -- full-range differences, NaN, rank bytes that are no inverse.  Nothing of its output is
 * decoded from.
 * Returns 0; -1, with nothing launched or allocated: a null pointer, n out of range, an index the walk or the head check
 * refuses, walk or first_out out of range, a cap too small; -2 when a HIP call failed; -3 when a guard byte has changed. */
int nblic_amd_debug_index_unpack(nblic_amd_ctx *ctx, int n, const void *const *packed, const size_t *packed_bytes,
                                 const size_t *base_offsets, const int *walks, const int *first_outs,
                                 unsigned char *const *outs, const size_t *caps, size_t *out_strides);

/* Debug hooks used by the delivery's tests (nblic_amd_decode_batch_indexed_to).  A task is a plane of plane_rows x width
 * bytes, a window of four ints (row0, row1, col0, col1: 0 <= row0 < row1 <= plane_rows, 0 <= col0 < col1 <= width -- no 0
 * stands for "to the end" here), a format with its scale and bias, a `zero` flag (zero bytes instead of pixels) and a
 * destination: a byte offset into an output buffer and a row pitch.
 * nblic_amd_debug_deliver_host: host only, no context, no device.  It runs the unit walk the kernel shares with the host
 * (csrc/deliver.h) over the caller's plane into out + dst_offset, one unit after the other; the unit grid follows the
 * destination's address modulo 16, as on the device.  gate_status: -1 or 1 deliver, anything else writes zeros.  units /
 * chunks (may be NULL) receive what a launch counts for the task: rows x ((cols + 16 / elem - 1 + 15) / 16) units, 1024
 * to a chunk.
 * nblic_amd_debug_deliver: ONE k_deliver launch over n tasks (1 .. 65536).  Plane k is uploaded at byte base_offsets[k]
 * (0 .. 15) of a zeroed, larger device buffer, and the kernel may read up256(plane_rows x width) bytes from there -- what
 * the decoders' planes allow it.  Destination k lies at byte dst_offsets[k] of a device buffer of out_bytes[k] bytes (at a
 * multiple of 256) that holds 0x5A everywhere before the launch and comes back whole in outs[k].  gate_status[k] != -1 is
 * put into a decoder record's header on the device, which the task is gated by: 1 (done) delivers, anything else zeros.
 * Both return 0; -1, with nothing launched or written, for a null pointer, a window outside the plane, a format, scale or
 * bias the calls refuse, a destination or pitch that is no multiple of the element size, a pitch below the window's row,
 * or a window that does not fit the output buffer from its offset on; nblic_amd_debug_deliver -2 when a HIP call failed. */
int nblic_amd_debug_deliver_host(const unsigned char *plane, int plane_rows, int width, const int *window, int format, float scale,
                                 float bias, int zero, int gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset,
                                 size_t pitch_bytes, unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_deliver(nblic_amd_ctx *ctx, int n, const unsigned char *const *planes, const size_t *plane_bytes,
                            const size_t *base_offsets, const int *plane_rows, const int *widths, const int *windows,
                            const int *formats, const float *scales, const float *biases, const int *zeros, const size_t *pitches,
                            const size_t *dst_offsets, const size_t *out_bytes, unsigned char *const *outs, const int *gate_status);
/* The two hooks above with a destination step: step_bytes / steps[k] are the bytes between neighbouring elements of a
 * destination row.  The element size is the task of the hooks above, byte for byte; anything larger is a strided task
 * (csrc/deliver.h): element (r, c) of the window goes to r x pitch + c x step from the destination's offset, units are
 * sixteen consecutive pixels of a row -- rows x ((cols + 15) / 16) of them -- and the pitch may be anything from the element
 * size up.  They refuse (-1) as above, and a step that is no multiple of the element size, is below it or above 2^20, and
 * a window whose last element, at (rows - 1) x pitch + (cols - 1) x step, does not fit the output buffer. */
int nblic_amd_debug_deliver_host_ex(const unsigned char *plane, int plane_rows, int width, const int *window, int format, float scale,
                                    float bias, int zero, int gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset,
                                    size_t pitch_bytes, size_t step_bytes, unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_deliver_ex(nblic_amd_ctx *ctx, int n, const unsigned char *const *planes, const size_t *plane_bytes,
                               const size_t *base_offsets, const int *plane_rows, const int *widths, const int *windows,
                               const int *formats, const float *scales, const float *biases, const int *zeros, const size_t *pitches,
                               const size_t *steps, const size_t *dst_offsets, const size_t *out_bytes, unsigned char *const *outs,
                               const int *gate_status);

/* Debug hooks used by the collection's tests (the _from encoders), the twins of the two above.  A task is a source -- its
 * bytes, the image's rows x cols, a pitch and a step in bytes, a format with its scale and bias -- and optionally a range of
 * two ints (px0, px1): the pixels of the flat rows x cols plane it writes (px1 == 0: to the end; NULL: all of it), as the
 * indexed batch collects the rows of a band.
 * nblic_amd_debug_collect_host: host only, no context, no device.  It runs the unit walk the kernel shares with the host
 * (csrc/collect.h) over the source at src (cap_bytes readable) into out, which must be a multiple of 16 and hold rows x cols
 * bytes.  units / chunks (may be NULL) receive what a launch counts for the task: (px1 + 15) / 16 - px0 / 16 units, 1024
 * to a chunk.
 * nblic_amd_debug_collect: ONE k_collect launch over n tasks (1 .. 65536).  The src_bytes[k] bytes of source k are uploaded
 * at byte base_offsets[k] (0 .. 255) of a larger device buffer that holds 0xFF everywhere else (NaN in every float format);
 * element (0, 0) is the first of them, and the task is refused unless the image's extent fits src_bytes[k].  Plane k lies at
 * byte 256 of a device buffer of out_bytes[k] = 256 + rows x cols rounded up to 256 + 256 bytes that holds 0x5A everywhere
 * before the launch and comes back whole in outs[k].
 * Both return 0; -1, with nothing launched or written, for a null pointer or anything the _from calls refuse of a source,
 * a range outside the plane or a buffer of the wrong size; nblic_amd_debug_collect -2 when a HIP call failed. */
int nblic_amd_debug_collect_host(const void *src, size_t cap_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int format,
                                 float scale, float bias, const int *range, unsigned char *out, size_t out_bytes,
                                 unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_collect(nblic_amd_ctx *ctx, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                            const int *rows, const int *cols, const size_t *pitches, const size_t *steps, const int *formats,
                            const float *scales, const float *biases, const int *ranges, unsigned char *const *outs,
                            const size_t *out_bytes);

/* Debug hooks used by the colour transform's tests (REVERSIBLE COLOUR TRANSFORM, above): the four hooks above on tasks that
 * may have a REFERENCE (csrc/collect.h, csrc/deliver.h), each ONE launch or one host walk; a task without one is the
 * task of the hooks above, byte for byte, and both kinds go into the same launch.
 * nblic_amd_debug_collect_ref_host / nblic_amd_debug_collect_ref: ref / refs[k] (NULL: none) is a second source of the
 * task's rows x cols and format with its own pitch and step in bytes -- ref_cap_bytes / ref_bytes[k] readable, uploaded at
 * byte ref_base_offsets[k] (0 .. 255) of a region of its own -- and a pixel is (own - ref + 128) mod 256 of the two
 * quantised elements.  They refuse (-1) what the hooks above refuse, and a reference that a source would be refused for.
 * nblic_amd_debug_deliver_ref_host / nblic_amd_debug_deliver_ref: ref / refs[k] (NULL: none) is a plane of ref_rows x width
 * bytes (uploaded at byte ref_base_offsets[k], 0 .. 15, of a zeroed region), and an element is made of
 * (plane + ref - 128) mod 256.  gate_status: THREE ints per task, each as in nblic_amd_debug_deliver; a task delivers
 * when none of them says otherwise.  step_bytes / steps: as in the _ex hooks; 0 or a NULL steps: the element size.  They
 * refuse (-1) what the hooks above refuse, and a reference that does not hold the window's rows. */
int nblic_amd_debug_collect_ref_host(const void *src, size_t cap_bytes, const void *ref, size_t ref_cap_bytes, size_t ref_pitch_bytes,
                                     size_t ref_step_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int format,
                                     float scale, float bias, const int *range, unsigned char *out, size_t out_bytes,
                                     unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_collect_ref(nblic_amd_ctx *ctx, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                                const void *const *refs, const size_t *ref_bytes, const size_t *ref_base_offsets,
                                const size_t *ref_pitches, const size_t *ref_steps, const int *rows, const int *cols,
                                const size_t *pitches, const size_t *steps, const int *formats, const float *scales,
                                const float *biases, const int *ranges, unsigned char *const *outs, const size_t *out_bytes);
int nblic_amd_debug_deliver_ref_host(const unsigned char *plane, int plane_rows, int width, const unsigned char *ref, int ref_rows,
                                     const int *window, int format, float scale, float bias, int zero, const int *gate_status,
                                     unsigned char *out, size_t out_bytes, size_t dst_offset, size_t pitch_bytes, size_t step_bytes,
                                     unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_deliver_ref(nblic_amd_ctx *ctx, int n, const unsigned char *const *planes, const size_t *plane_bytes,
                                const size_t *base_offsets, const unsigned char *const *refs, const size_t *ref_base_offsets,
                                const int *ref_rows, const int *plane_rows, const int *widths, const int *windows, const int *formats,
                                const float *scales, const float *biases, const int *zeros, const size_t *pitches, const size_t *steps,
                                const size_t *dst_offsets, const size_t *out_bytes, unsigned char *const *outs, const int *gate_status);

/* PER-FRAME COLOUR MODES: the transform chosen frame by frame from costs measured on the device.
 * A frame's MODE is one byte.  Bits 0..1: the base channel b (0 = R, 1 = G, 2 = B).  Bit 2: the lower-numbered of the two
 * other channels is coded as (c - b + 128) mod 256.  Bit 3: the same for the higher-numbered one.  The base, and a channel
 * whose bit is clear, are coded as they are.  Valid: 0 (plain, the only spelling of "no difference") and b | 4, b | 8,
 * b | 12 for b = 0 .. 2 -- ten modes; NBLIC_AMD_COLOR_RCT (base G, both differences) is what NBLIC_AMD_FORMAT_RCT does.
 * The reference of a difference is always the caller's SOURCE of the base channel on encode and the DECODED base plane on
 * decode; there are no chains of differences.  Nothing in a stream says which mode it was coded in: the caller keeps the
 * byte with the frame's three streams.
 *
 * nblic_amd_color_plan measures and chooses.  Images 3f .. 3f + 2 of srcs are R, G, B of frame f (sources as the _from
 * calls take them, one format, scale and bias).  ONE launch of k_color_cost computes, per frame, the COST of nine planes --
 * R, G, B, R-G, R-B, G-R, G-B, B-R, B-G in this order, X-Y being (X - Y + 128) mod 256 of the pixels k_collect would write:
 * the sum over the pixels of 2 * bitlen(|e|) + 1, e the residual (wrapped to -128 .. 127) of the MED prediction from W, N
 * and NW of the same plane (row 0: W; column 0: N; (0, 0): 128), integers only, unsigned 64-bit sums that depend on nothing
 * but the pixels -- the table comes back in one copy, and the host chooses by nblic_amd_color_choose:
 *     with base b, channel c takes its difference only if 64 * cost(c - b) < 63 * cost(c) (a design margin: a difference
 *     that does not clearly win should not cost the frame its readability by plain decoders);
 *     total(b) = cost(b) + the cheaper alternative, under that rule, of each other channel; the smallest total wins,
 *     ties go to G, then R, then B; a winner without a difference is mode 0.
 * The rule is part of the interface: two builds plan alike.
 *   frame_modes   n_images / 3 bytes; 0xFF for a frame with a source the _from calls refuse or with sources of unequal size
 *                 (nothing is launched for it, its costs are zero, the other frames are unaffected)
 *   costs         NULL, or nine sums per frame
 *   -1            nothing launched: n_images % 3 != 0, a null srcs or frame_modes, an unknown format (NBLIC_AMD_FORMAT_RCT
 *                 included), a scale or bias the _from calls refuse; or a HIP call failed.
 * nblic_amd_color_plan_stats: out[0] launches of k_color_cost, out[1] source elements read, since the context was made;
 * last_plan_ms (may be NULL): GPU milliseconds of the last nblic_amd_color_plan's launch.
 *
 * The six _color calls are the four _from encoders and the two _to_ex decoders with `frame_modes` (one byte per frame,
 * n_images / 3 of them) in place of NBLIC_AMD_FORMAT_RCT, which they do not take; the calls with the flag are these with
 * every mode NBLIC_AMD_COLOR_RCT.  Each plane of a frame takes its reference from the mode; a plane that is no difference
 * and is contiguous uint8 is still used in place.  A frame with a difference follows the flag's frame rules (a refused
 * member refuses the frame; every delivery task of the frame is gated by all three planes; a plane that fails leaves
 * zeros in all three windows); a frame of mode 0 is three independent images, exactly as without the flag.
 *   -1, nothing launched or written: an invalid mode byte (0xFF is one); n_images % 3 != 0; in
 *   nblic_amd_encode_batch_modes_from_color, near > 0 on an image of a frame whose mode is not 0.
 * nblic_amd_encode_batch_modes_from_to has no sibling. */
#define NBLIC_AMD_COLOR_PLAIN 0
#define NBLIC_AMD_COLOR_RCT 0x0D
int nblic_amd_color_plan(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                         unsigned char *frame_modes, unsigned long long *costs);
unsigned char nblic_amd_color_choose(const unsigned long long costs[9]);     /* host only, pure; NULL: 0xFF */
int nblic_amd_color_mode_valid(int mode);                                    /* 1 / 0 */
int nblic_amd_color_mode_ref(int mode, int channel);                         /* the channel plane `channel` is taken against; -1: none; -2: invalid */
int nblic_amd_color_plan_stats(nblic_amd_ctx *ctx, long out[2], double *last_plan_ms);
int nblic_amd_encode_batch_modes_from_color(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                            const unsigned char *frame_modes, const int *nears, const int *efforts, unsigned char *const *outs,
                                            const size_t *out_caps, long *out_lens, unsigned char *const *recons);
int nblic_amd_qencode_batch_from_color(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                       const unsigned char *frame_modes, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words);
int nblic_amd_encode_batch_indexed_from_color(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                              const unsigned char *frame_modes, const int *every_rows, int band_rows, unsigned char *const *outs,
                                              const size_t *out_caps, long *out_lens, unsigned char *const *indexes, const size_t *index_caps, long *index_lens);
int nblic_amd_qencode_batch_indexed_from_color(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                               const unsigned char *frame_modes, const int *every_rows, int band_rows, uint16_t *const *outs,
                                               const size_t *out_caps_words, long *out_len_words, unsigned char *const *indexes, const size_t *index_caps,
                                               long *index_lens);
int nblic_amd_decode_batch_to_ex_color(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                       const nblic_amd_dest_ex *dests, int format, const unsigned char *frame_modes, int *heights, int *widths,
                                       int *nears, int *efforts, int *status);
int nblic_amd_decode_batch_indexed_to_ex_color(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                               const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                               const unsigned char *frame_modes, int *heights, int *widths, int *nears, int *efforts, int *status);
/* Debug hooks used by the colour plan's tests: the cost kernel and its host walk alone (csrc/color_plan.h).
 * nblic_amd_debug_color_cost_host: ONE frame, host only: srcs / cap_bytes / pitches / steps have three entries (R, G, B),
 * cap_bytes[ch] readable from srcs[ch]; costs receives the nine sums, tiles (may be NULL) the kernel's workgroups.
 * nblic_amd_debug_color_cost: ONE k_color_cost launch over n frames: srcs / src_bytes / base_offsets / pitches / steps have
 * three entries per frame (3 k + channel), each source uploaded at byte base_offsets[] (0 .. 255) of a region of its own
 * filled with 0xFF; costs receives nine sums per frame.  -1: refused (what a source of nblic_amd_debug_collect is refused
 * for); -2: a HIP call failed. */
int nblic_amd_debug_color_cost_host(const void *const *srcs, const size_t *cap_bytes, const size_t *pitches, const size_t *steps, int rows, int cols,
                                    int format, float scale, float bias, unsigned long long *costs, unsigned long long *tiles);
int nblic_amd_debug_color_cost(nblic_amd_ctx *ctx, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                               const size_t *pitches, const size_t *steps, const int *rows, const int *cols, const int *formats,
                               const float *scales, const float *biases, unsigned long long *costs);

/* SLICE STACKS: the images of a call as stacks of `depth` slices -- the slices of a CT or microscopy volume, the frames of a
 * static camera, a burst -- a slice coded as it is or against the slice before it (csrc/stack.h).
 *   depth         D >= 1, n_images % D == 0; image s * D + d is slice d of stack s (n-major, as a [N, D, H, W] tensor is read).
 *                 The slices of a stack have one size.
 *   slice_modes   one byte per image.  0 (NBLIC_AMD_SLICE_KEY): coded as it is.  1 (NBLIC_AMD_SLICE_DELTA): coded as
 *                 (x_d - x_{d-1} + 128) mod 256, both the pixels k_collect would write.  Slice 0 of every stack must be 0.
 *                 Every other byte is invalid; 0xFF is what nblic_amd_stack_plan gives the slices of a stack it refuses.
 * A RUN is a key slice and the delta slices that follow it; restoring is x_d = (t_d + x_{d-1} - 128) mod 256 along the run.
 * The streams are ordinary .nblic / QNBLIC streams of those planes: nothing in them names the mode, the caller keeps the
 * bytes, and a decoder without them yields the difference planes.  LOSSLESS ONLY inside a run: near > 0 is
 * allowed only on a key slice whose successor in the stack (if any) is a key slice too.
 *
 * ENCODE: the four _from_stack calls are the four _from encoders with depth and slice_modes.  A delta slice is collected
 * with the caller's SOURCE of the slice before it as its reference (no new kernel; collected even where it could be used in
 * place); key slices stay what they were.  A stack with a delta and a refused or unequal-size source is refused as a whole
 * (every length -1); a stack of keys only is D images like any other.  Every stream and index is byte for byte what the call
 * without _stack returns for the difference plane.
 *   -1, nothing launched: an invalid byte, depth < 1, n_images % depth != 0, the near rule above, NBLIC_AMD_FORMAT_RCT in format.
 *
 * DECODE: the two _to_ex_stack calls are the two _to_ex decoders with depth and slice_modes.  A run with a delta is delivered
 * by ONE task of a second kernel, k_deliver_stack, whose lanes carry the running pixels of sixteen window pixels from the
 * key slice to the run's last one in registers; a key slice without a delta behind it goes through k_deliver as before: at
 * most one launch of each kernel per call (in nblic_amd_decode_batch_to_ex_stack behind the work of both of its streams).
 *   same window   the slices of a stack with a delta share ONE window after defaulting (with an index the window's rows
 *                 choose the segments of every slice; the slices' indexes may differ)
 *   refused       status -1 for every slice, nothing written, nothing launched, for a stack with a delta and: a member that
 *                 does not parse, unequal sizes, near > 0 inside a run, unequal windows, or a refused destination
 *   skipped       a destination with ptr == NULL and cap_bytes == 0: the slice is decoded as a reference only; its window
 *                 fields still count for the "same window" rule; its status is that of its plane
 *   failure       slice d is delivered only if every plane of its run from the key through d decoded: otherwise d and every
 *                 later slice of the run get zeros and status -1; earlier slices, other runs and other stacks are unaffected
 *   random access hand in the streams key .. target of one run with one destination (the others skipped)
 *   -1 for the call: an invalid byte, depth < 1, n_images % depth != 0.
 *
 * PLAN: nblic_amd_stack_plan measures and chooses.  ONE launch of k_stack_cost computes two COSTS per slice (the cost of
 * nblic_amd_color_plan: the sum of 2 * bitlen(|e|) + 1 over the MED residuals): INTRA, of the slice itself, and DELTA, of
 * its difference plane against the slice before (0 for slice 0) -- against that slice's SOURCE whatever its own mode, so
 * the choices are independent of each other and the exhaustive best of a stack is two encodes, all keys and all deltas.
 * The host chooses by nblic_amd_stack_choose: 1 iff 64 * delta < 63 * intra (the colour plan's margin; equality gives 0).
 * The rule is part of the interface.  key_every = K > 0 forces every slice with d % K == 0 to a key (0: only slice 0).
 *   slice_modes   n_images bytes; 0xFF for all slices of a stack with a source the _from calls refuse or sources of unequal
 *                 size (nothing is launched for it, its costs are zero, the other stacks are unaffected)
 *   costs         NULL, or two sums per image (intra, delta)
 *   -1            nothing launched: the call-level errors of nblic_amd_color_plan (but the count rule), depth < 1,
 *                 n_images % depth != 0, key_every < 0; or a HIP call failed.
 * nblic_amd_stack_plan_stats: out[0] launches of k_stack_cost, out[1] source elements read, out[2] launches of
 * k_deliver_stack, out[3] runs delivered, since the context was made; last_ms (may be NULL), two values: GPU milliseconds
 * of the last nblic_amd_stack_plan's launch, and of the delivery launches of the last _to_ex_stack call.
 * The gain on real volumes and sequences is UNMEASURED: none was at hand (README.md says what was measured instead). */
#define NBLIC_AMD_SLICE_KEY 0
#define NBLIC_AMD_SLICE_DELTA 1
int nblic_amd_stack_plan(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias, int depth, int key_every,
                         unsigned char *slice_modes, unsigned long long *costs);
int nblic_amd_stack_choose(unsigned long long intra, unsigned long long delta);      /* host only, pure: 1 / 0 */
int nblic_amd_stack_slice_mode(int d, int key_every, unsigned long long intra, unsigned long long delta);     /* what the plan gives slice d: 1 / 0; -1: d or key_every < 0 */
int nblic_amd_stack_mode_valid(int mode);                                            /* 1 / 0 */
int nblic_amd_stack_modes_valid(int n_images, int depth, const unsigned char *slice_modes);     /* the bytes of a call: 1 / 0 */
int nblic_amd_stack_plan_stats(nblic_amd_ctx *ctx, long out[4], double last_ms[2]);
int nblic_amd_encode_batch_modes_from_stack(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                            int depth, const unsigned char *slice_modes, const int *nears, const int *efforts, unsigned char *const *outs,
                                            const size_t *out_caps, long *out_lens, unsigned char *const *recons);
int nblic_amd_qencode_batch_from_stack(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                       int depth, const unsigned char *slice_modes, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words);
int nblic_amd_encode_batch_indexed_from_stack(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                              int depth, const unsigned char *slice_modes, const int *every_rows, int band_rows, unsigned char *const *outs,
                                              const size_t *out_caps, long *out_lens, unsigned char *const *indexes, const size_t *index_caps, long *index_lens);
int nblic_amd_qencode_batch_indexed_from_stack(nblic_amd_ctx *ctx, int n_images, const nblic_amd_src *srcs, int format, float scale, float bias,
                                               int depth, const unsigned char *slice_modes, const int *every_rows, int band_rows, uint16_t *const *outs,
                                               const size_t *out_caps_words, long *out_len_words, unsigned char *const *indexes, const size_t *index_caps,
                                               long *index_lens);
int nblic_amd_decode_batch_to_ex_stack(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                       const nblic_amd_dest_ex *dests, int format, int depth, const unsigned char *slice_modes, int *heights, int *widths,
                                       int *nears, int *efforts, int *status);
int nblic_amd_decode_batch_indexed_to_ex_stack(nblic_amd_ctx *ctx, int n_images, const unsigned char *const *streams, const size_t *stream_lens,
                                               const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                               int depth, const unsigned char *slice_modes, int *heights, int *widths, int *nears, int *efforts, int *status);
/* Debug hooks used by the stacks' tests: the two kernels and their host walks alone (csrc/stack.h).
 * nblic_amd_debug_stack_deliver_host: ONE run of `count` caller-made planes of plane_rows x width bytes, host only: window is
 * row0, row1, col0, col1; slice d goes to outs[d] + dst_offsets[d] in out_bytes[d] bytes with pitches[d] and steps[d] (0: the
 * element size), outs[d] NULL: a skipped slice; zeros[d] != 0: the plane is known to be bad; gate_status[d]: the status of its
 * gate record (-1: none).  units / chunks (may be NULL): what a launch would count.
 * nblic_amd_debug_stack_deliver: ONE k_deliver_stack launch over n runs; run k has counts[k] planes, and the per-plane
 * arrays hold the runs' entries one after the other.  A plane is uploaded at byte base_offsets[] (0 .. 15) of a zeroed region
 * of its own; a destination lies at byte dst_offsets[] of a buffer of out_bytes[] bytes filled with 0x5A, which comes back
 * whole in outs[].
 * nblic_amd_debug_stack_cost_host: ONE stack of `count` sources, host only; costs receives two sums per source, tiles (may be
 * NULL) the kernel's workgroups.  nblic_amd_debug_stack_cost: ONE k_stack_cost launch over n stacks of counts[k] sources,
 * each uploaded at byte base_offsets[] (0 .. 255) of a region of its own filled with 0xFF.
 * -1: refused; -2: a HIP call failed. */
int nblic_amd_debug_stack_deliver_host(int count, const unsigned char *const *planes, int plane_rows, int width, const int *window, int format,
                                       const float *scales, const float *biases, const int *zeros, const int *gate_status, unsigned char *const *outs,
                                       const size_t *out_bytes, const size_t *dst_offsets, const size_t *pitches, const size_t *steps,
                                       unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_stack_deliver(nblic_amd_ctx *ctx, int n, const int *counts, const unsigned char *const *planes, const size_t *base_offsets,
                                  const int *plane_rows, const int *widths, const int *windows, const int *formats, const float *scales, const float *biases,
                                  const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets, const size_t *out_bytes,
                                  unsigned char *const *outs, const int *gate_status);
int nblic_amd_debug_stack_cost_host(int count, const void *const *srcs, const size_t *cap_bytes, const size_t *pitches, const size_t *steps, int rows, int cols,
                                    int format, float scale, float bias, unsigned long long *costs, unsigned long long *tiles);
int nblic_amd_debug_stack_cost(nblic_amd_ctx *ctx, int n, const int *counts, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets,
                               const size_t *pitches, const size_t *steps, const int *rows, const int *cols, const int *formats,
                               const float *scales, const float *biases, unsigned long long *costs);

/* DEEP PIXELS: an image of 16-bit elements -- uint16, or int16 such as Hounsfield units -- coded as TWO ordinary 8-bit
 * images, a HIGH and a LOW plane (csrc/deep.h).  With u the element as an unsigned 16-bit number
 * (uint16: u = x; int16: u = x + 32768, the sign bit flipped): hi = u >> 8, lo = u & 255.
 *   streams       a call on n_deep images has 2 x n_deep streams: stream 2k is the HIGH plane of deep image k, stream 2k + 1
 *                 its LOW plane.  Every per-stream array (outs, caps, lens, nears, efforts, every_rows, indexes, status,
 *                 heights, ...) has 2 x n_deep entries; srcs, dests and modes have n_deep.  There is no container and no new
 *                 stream format: each stream and index is byte for byte what the call without _deep returns for that 8-bit
 *                 plane, and a plain decoder -- the reference tool included -- gets the two planes back.
 *   modes         one byte per deep image, which the CALLER keeps with the image's two streams (nothing in them names it).
 *                 Bit 0 (NBLIC_AMD_DEEP_FOLD): the low plane holds 255 - lo wherever hi is odd -- the sawtooth of the low
 *                 byte, which jumps by 255 whenever the high byte steps, becomes a continuous triangle wave.  Bit 1
 *                 (NBLIC_AMD_DEEP_SIGNED): the source was int16, the value is u - 32768.  Valid: 0 .. 3; 0xFF is what
 *                 nblic_amd_deep_plan gives an image it refuses.
 *   deep_format   of a source: 0 uint16 (NBLIC_AMD_DEEP_U16), 1 int16 (NBLIC_AMD_DEEP_I16).  Of a destination: 0 uint16, 1 int16,
 *                 2 float16, 3 bfloat16, 4 float32 (NBLIC_AMD_DEEP_TO_*).  The numbering is the deep calls' own; the calls
 *                 without _deep keep refusing format 4 and above.
 * ENCODE: the four _from_deep calls are the four _from encoders on 16-bit sources: nblic_amd_src with pointer, pitch and
 * step multiples of 2, no scale and no bias -- a 16-bit integer is coded as it is.  ONE launch of k_collect_deep writes both
 * planes of every image (one task per plane) into a block of the call's own, which the encoder then uses in place.
 *   near          the high plane must be lossless: a non-zero nears[2k] refuses the whole call.  The low plane may have any
 *                 near: its reconstruction stays in 0 .. 255 and the high byte is exact, and the fold is an isometry of the
 *                 low byte, so the restored value differs from the source by AT MOST nears[2k + 1], folded or not.
 *   recons        host buffers of the two planes' reconstructions, as nblic_amd_encode_batch_modes_from leaves them.
 * DECODE: the two _to_ex_deep calls are the two _to_ex decoders with one nblic_amd_dest_ex per deep image: window, row range
 * and index semantics are theirs.  ONE launch of k_deliver_deep joins the planes: uint16 / int16 get the value, the float
 * formats float(v) x scale + bias with v the unsigned or signed value (exact as a float), two float32 roundings, never
 * fused, then round-to-nearest-even into the format (a float16 overflow goes to infinity).
 * REFUSED, the whole call (-1, nothing launched): a mode byte that is not valid (0xFF included); on encode a mode whose bit 1
 * disagrees with deep_format; a NULL array; an unknown format.
 * REFUSED, that image alone (both streams -1, nothing written, the others unaffected): a source or destination that fails
 * the pointer, pitch, step, cap or device checks of the calls without _deep (element size 2, or 4 for float32); a size the
 * encoder does not take; on decode two streams of unequal size, and a uint16 / int16 destination whose signedness
 * contradicts the mode's bit 1; scale != 1 or bias != 0 with an integer destination.
 * A plane that fails on the device: zeros in the image's window and -1 for both of its streams.
 * PLAN: nblic_amd_deep_plan measures and chooses.  ONE launch of k_deep_cost computes per image the COSTS of its three
 * candidate planes -- high, low, folded low: the sum over the pixels of 2 x bitlen(|e|) + 1, e the MED residual NOT wrapped
 * mod 256 (a wrapped residual would rate the sawtooth's jumps at nothing) -- and the minimum and maximum of u.
 * nblic_amd_deep_choose is THE RULE (pure, host only): fold iff cost(folded low) < cost(low), ties are plain, no margin;
 * bit 1 from deep_format.  costs (may be NULL): n_deep x 3; ranges (may be NULL): n_deep x 2, min and max of u -- so a
 * caller sees that the data fits 8 or 12 bits.  A source the encoders refuse: mode 0xFF, zeros, nothing launched for it.
 * nblic_amd_deep_plan_stats: out[0] launches of k_deep_cost, [1] of k_collect_deep, [2] of k_deliver_deep, [3] images
 * costed, since the context was made; last_ms (may be NULL), three values: GPU milliseconds of the last plan's k_deep_cost
 * launch, of the last _from_deep call's k_collect_deep launch and of the last _to_ex_deep call's k_deliver_deep launch. */
#define NBLIC_AMD_DEEP_FOLD 1
#define NBLIC_AMD_DEEP_SIGNED 2
#define NBLIC_AMD_DEEP_U16 0
#define NBLIC_AMD_DEEP_I16 1
#define NBLIC_AMD_DEEP_TO_U16 0
#define NBLIC_AMD_DEEP_TO_I16 1
#define NBLIC_AMD_DEEP_TO_F16 2
#define NBLIC_AMD_DEEP_TO_BF16 3
#define NBLIC_AMD_DEEP_TO_F32 4
int nblic_amd_deep_plan(nblic_amd_ctx *ctx, int n_deep, const nblic_amd_src *srcs, int deep_format, unsigned char *modes, unsigned long long *costs,
                        unsigned int *ranges);
int nblic_amd_deep_choose(const unsigned long long costs[3], int deep_format);       /* host only, pure: the mode byte; -1: NULL or an unknown format */
int nblic_amd_deep_mode_valid(int mode);                                             /* 1 / 0 */
int nblic_amd_deep_plan_stats(nblic_amd_ctx *ctx, long out[4], double last_ms[3]);
int nblic_amd_encode_batch_modes_from_deep(nblic_amd_ctx *ctx, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                           const int *nears, const int *efforts, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                           unsigned char *const *recons);
int nblic_amd_qencode_batch_from_deep(nblic_amd_ctx *ctx, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                      uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words);
int nblic_amd_encode_batch_indexed_from_deep(nblic_amd_ctx *ctx, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                             const int *every_rows, int band_rows, unsigned char *const *outs, const size_t *out_caps, long *out_lens,
                                             unsigned char *const *indexes, const size_t *index_caps, long *index_lens);
int nblic_amd_qencode_batch_indexed_from_deep(nblic_amd_ctx *ctx, int n_deep, const nblic_amd_src *srcs, int deep_format, const unsigned char *modes,
                                              const int *every_rows, int band_rows, uint16_t *const *outs, const size_t *out_caps_words, long *out_len_words,
                                              unsigned char *const *indexes, const size_t *index_caps, long *index_lens);
int nblic_amd_decode_batch_to_ex_deep(nblic_amd_ctx *ctx, int n_deep, const unsigned char *const *streams, const size_t *stream_lens,
                                      const nblic_amd_dest_ex *dests, int format, const unsigned char *modes, int *heights, int *widths, int *nears,
                                      int *efforts, int *status);
int nblic_amd_decode_batch_indexed_to_ex_deep(nblic_amd_ctx *ctx, int n_deep, const unsigned char *const *streams, const size_t *stream_lens,
                                              const void *const *indexes, const size_t *index_lens, const nblic_amd_dest_ex *dests, int format,
                                              const unsigned char *modes, int *heights, int *widths, int *nears, int *efforts, int *status);
/* Debug hooks used by the deep tests: the three kernels and their host walks alone (csrc/deep.h), one launch or one walk each.
 * nblic_amd_debug_deep_collect(_host): as nblic_amd_debug_collect(_host) with a deep_format and a part (0 high, 1 low,
 * 2 folded low) in place of format, scale and bias.
 * nblic_amd_debug_deep_deliver(_host): as nblic_amd_debug_deliver_ex / _host_ex with two planes per task (base_offsets and
 * gate_status: two entries per task, high then low), a destination format of the deep numbering and a mode byte; steps 0:
 * the element size.
 * nblic_amd_debug_deep_cost(_host): sums receives five numbers per source -- the costs of the high, the low and the folded
 * low plane, min and max of u; tiles (may be NULL) the kernel's workgroups.  Each source is uploaded at byte base_offsets[]
 * (0 .. 255) of a region of its own filled with 0xFF.  -1: refused; -2: a HIP call failed. */
int nblic_amd_debug_deep_collect_host(const void *src, size_t cap_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int deep_format, int part,
                                      const int *range, unsigned char *out, size_t out_bytes, unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_deep_collect(nblic_amd_ctx *ctx, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets, const int *rows,
                                 const int *cols, const size_t *pitches, const size_t *steps, const int *deep_formats, const int *parts, const int *ranges,
                                 unsigned char *const *outs, const size_t *out_bytes);
int nblic_amd_debug_deep_deliver_host(const unsigned char *hi, const unsigned char *lo, int plane_rows, int width, const int *window, int format, int mode,
                                      float scale, float bias, int zero, const int *gate_status, unsigned char *out, size_t out_bytes, size_t dst_offset,
                                      size_t pitch_bytes, size_t step_bytes, unsigned long long *units, unsigned long long *chunks);
int nblic_amd_debug_deep_deliver(nblic_amd_ctx *ctx, int n, const unsigned char *const *his, const unsigned char *const *los, const size_t *base_offsets,
                                 const int *plane_rows, const int *widths, const int *windows, const int *formats, const int *modes, const float *scales,
                                 const float *biases, const int *zeros, const size_t *pitches, const size_t *steps, const size_t *dst_offsets,
                                 const size_t *out_bytes, unsigned char *const *outs, const int *gate_status);
int nblic_amd_debug_deep_cost_host(const void *src, size_t cap_bytes, int rows, int cols, size_t pitch_bytes, size_t step_bytes, int deep_format,
                                   unsigned long long *sums, unsigned long long *tiles);
int nblic_amd_debug_deep_cost(nblic_amd_ctx *ctx, int n, const void *const *srcs, const size_t *src_bytes, const size_t *base_offsets, const int *rows,
                              const int *cols, const size_t *pitches, const size_t *steps, const int *deep_formats, unsigned long long *sums);

/* Debug hook used by the indexed effort-0 batch's host tests: QNBLIC's entropy stage (histogram normalisation, histogram
 * code, the rANS pass) on caller-made records, reporting the coder in front of entry rows as the batch's workers read it.
 * Host only: no context, no device.  words[height x width] = level | symbol << 8 per pixel, hist[12 x 256] the counts
 * per level and symbol; entry_rows[n_entries] rows 0 < r < height in ascending order (n_entries may be 0).  Writes the
 * stream into out (cap_words 16-bit words) and per entry row r: states[k] = the rANS state once pixel r x width has been
 * coded (the pass runs last pixel first), words_emitted[k] = the renormalisation words emitted by then.  With W such words
 * in all -- the stream's rANS part is W + 2 words -- a decoder in front of row r holds states[k] and has consumed
 * 2 + W - words_emitted[k] words of it.  Returns the stream's length in words; -1 when cap_words is too small; -2, with
 * nothing written, for a null pointer, a size out of range, entry rows out of range or order, a word whose level is
 * above 11 or whose symbol its level's histogram does not count. */
long nblic_amd_debug_q_entropy(int height, int width, const uint16_t *words, const unsigned int *hist, const int *entry_rows,
                               int n_entries, uint16_t *out, size_t cap_words, unsigned int *states,
                               unsigned long long *words_emitted);

/* Device self-test of the wave primitives the chain kernels rely on (DPP prefix sum against the
 * shuffle formulation).  Returns the number of mismatching lanes (0 = pass) or -1.           */
int nblic_amd_selftest(nblic_amd_ctx *ctx);

/* The host half of the path on its own: the serial range-coder stage (src/NBLIC.c:552-586) over
 * n coded bins (u16 each: probability of a 1 in 1/4096 in bits 0-11, the bin in bit 15).
 * Writes at most cap bytes (coder bytes + 4 flush bytes, no header); returns the byte count or
 * (size_t)-1 when cap is too small.  Needs no GPU.                                         */
size_t nblic_amd_range_code(const uint16_t *coded, size_t n, unsigned char *out, size_t cap);

/* Synthetic benchmark frame "SYN-1" (SURVEY.md 8d): xorshift32 noise on a triangular ramp with a
 * 16-level texture; deterministic, integer only.  Host function, needs no GPU.              */
void nblic_amd_syn1(unsigned char *img, int height, int width, uint32_t seed);

/* Same stage for `count` independent streams.  On hosts with AVX-512 eight streams are coded at
 * once in the eight 64-bit lanes of a vector register (returns 1), otherwise one after the other
 * (returns 0); the bytes are identical either way.  lens[k] = byte count or (size_t)-1.       */
int nblic_amd_range_code_multi(const uint16_t *const *coded, const size_t *n, int count, unsigned char *const *outs,
                               const size_t *caps, size_t *lens);

/* The same streams fed `chunk` bins at a time through the RESUMABLE coders, exactly as the coder
 * threads do when they stream an image's bins from HBM (one stream: scalar coder; more: consecutive
 * eights are AVX-512 packs, one to three in lock-step; any chunk length).  Host function; exists so that the
 * chunked path can be checked without a GPU.  Returns 0, or -1 for count outside 1..24 or chunk == 0.           */
int nblic_amd_range_code_chunked(const uint16_t *const *coded, const size_t *n, int count, unsigned char *const *outs,
                                 const size_t *caps, size_t *lens, size_t chunk);

/* The layout's reference: ORs the 13-bit codes of one lane's n records into zeroed 8-lane rows,
 * rows[(13 g + j) * 8 + lane] (csrc/range_coder.h).  Host function.                                               */
void nblic_amd_pack_groups_host(uint64_t *rows, int lane, const uint16_t *coded, size_t n);

/* The coder threads' pack feed, minus the GPU: n_packs (1..3) packs of pack_n[p] (1..8) streams each, coded in
 * lock-step from 8-lane rows of 13-bit groups, `chunk` bins (a multiple of 64) at a time.  Every array is indexed
 * 8 p + lane: stream `lane` of pack p.  lens[8 p + lane] = byte count or (size_t)-1.  Returns 0; 1 on a host without
 * AVX-512 (every stream through the scalar coder, as the coder threads do there); -1 for arguments out of range.   */
int nblic_amd_range_code_packs(int n_packs, const int *pack_n, const uint16_t *const *coded, const size_t *n, unsigned char *const *outs,
                               const size_t *caps, size_t *lens, size_t chunk);

/* ---- 3. front end: image files and the reference tool's command line (host only) ----------------- */

/* The reference tool's main() (src/NBLIC_main.c:139-254) on this library: same switch grammar (groups
 * such as "-cn2e2V"), same PGM-then-BMP probing of the input (:168-169), -n0 -e0 -> QNBLIC with the word
 * count doubled (:182-188), QNBLIC-then-NBLIC decoding (:223-226), ".bmp" suffix -> BMP output (:233).
 * Returns 0, or -1 after printing an "***Error" line.  The `nblic_codec_amd` executable is this call.  */
int nblic_amd_cli_main(int argc, char **argv);

/* The parsed command line (tests of the grammar): fields[0..7] = decompress, near, effort, verbose,
 * multithread, large-image opt-in (-L), device (-g<N>, -1 = unset), have_src | have_dst << 1.            */
void nblic_amd_cli_parse(int argc, char **argv, int *fields, char *src, char *dst, size_t cap);

/* Reads an 8-bit gray image the way the reference's front end does (src/FileIO.c:81-131 binary PGM, then
 * :170-225 8-bit BMP: bottom-up rows, 4-byte row padding, pixel = palette index).  Writes h*w bytes (row
 * major, top-down) to px.  Returns 1 = PGM, 2 = BMP, 0 = neither, -1 = cap too small (*h, *w still set). */
int nblic_amd_read_gray(const char *path, unsigned char *px, size_t cap, int *h, int *w);

/* Writes "P5\n<w> <h>\n255\n" + pixels (src/FileIO.c:141-159), or with as_bmp != 0 the 1078-byte header
 * (identity gray palette) + bottom-up padded rows (src/FileIO.c:229-287).  Returns 0 / -1.               */
int nblic_amd_write_gray(const char *path, const unsigned char *px, int h, int w, int as_bmp);

/* Device self-test of the serial kernels' arithmetic: the double-carried truncating divisions of the
 * least-squares predictor against 64-bit integer division on 65536 operand triples.  0 = pass.   */
int nblic_amd_serial_selftest(nblic_amd_ctx *ctx);

/* Test entry point: both least-squares solvers of the serial kernels on `count` given systems, no image and no coder.
 * stats: count x (1 + n + n*n) integer-valued statistics [s | b | A]; regressors: count x 10; bias: per item the
 * regularisation strength the pixel starts from (its two systems are regularised with the pair around it).  n = 6
 * (effort 2) or 10 (effort 3); waves = 2 (n = 10) runs the two-wave kernel's hand-over of system 1.  Per item
 *   out_f64[12]: double path -- clamped Q12 prediction of system 0, 1; largest product, entry, quotient, pivot of
 *                system 0; the same of system 1;
 *   out_i64[14]: what the kernels deliver for the pixel -- p1, p2, ok1, ok2; the double path's ok of system 0, 1 and
 *                whether its magnitudes stayed in the exact range (0, 1); the integer path's raw Q12 sum of system 0, 1
 *                and its ok (0, 1); the redo counts the item raised (0, 1).
 * Both paths are always computed.  Returns 0, or -1.                                                           */
int nblic_amd_lsq_probe(nblic_amd_ctx *ctx, int n, int waves, int count, const double *stats, const signed char *regressors, const int *bias,
                        double *out_f64, long long *out_i64);

const char *nblic_amd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NBLIC_AMD_H */
