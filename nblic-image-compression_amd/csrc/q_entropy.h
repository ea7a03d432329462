// q_entropy.h -- the host half of the QNBLIC (effort 0) path as the pipeline calls it (q_entropy.cpp).  No HIP, no device.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nblic {

// What the coder holds in front of an entry row r (the indexed effort-0 batch, pipeline.hip): the rANS pass runs LAST PIXEL
// FIRST, so its state once pixel r * w has been coded -- and before pixel r * w - 1 is looked at -- is the state a decoder
// holds when it has decoded (and renormalised after) pixel r * w - 1: the decoder undoes the pass step by step.  `words`
// counts the renormalisation words emitted up to that moment, the one pixel r * w itself may have cost included; the
// decoder has then consumed all the others, so with W words in all (the two final ones aside) it stands
// 2 * (2 + W - words) bytes behind the first rANS word of the reversed stream.
struct QEntryState { uint32_t state, reserved; unsigned long long words; };

// Entropy stage of QNBLICcompress.  qy[t] = level | symbol << 8; hist = 12 x 256 raw counts.
// Returns the stream length in 16-bit words (header included) or -1 if cap_words is too small.
long q_entropy_encode(uint16_t *out, size_t cap_words, int h, int w, const uint16_t *qy, const uint32_t *hist_in);
// The same stage.  entry_rows[0 .. n_entries): rows 0 < r < h in ascending order; entries[k] receives the coder in front
// of row entry_rows[k] (above).  The stream does not depend on them.  Also -2: entry rows that are out of range or out of
// order (nothing is written then).
long q_entropy_encode_entries(uint16_t *out, size_t cap_words, int h, int w, const uint16_t *qy, const uint32_t *hist_in,
                              const int *entry_rows, int n_entries, QEntryState *entries);
// The front matter alone: header words, then per level the scaled histogram's code; freq / start (12 x 256 each) receive
// the tables the pass codes with.  Returns the words written, or -1 if cap_words is too small.
long q_entropy_front(uint16_t *out, size_t cap_words, int h, int w, const uint32_t *hist_in, uint32_t *freq, uint32_t *start);
// freq / start as the packed table of q_rans.h (12 x 256 entries of f | start << 16; 0 for a symbol never coded).
void q_rans_table(const uint32_t *freq, const uint32_t *start, uint32_t *table);
// q_entropy_encode's stream, made by one lane of q_rans.h that is resumed every symbols_per_launch symbols (<= 0: never).
long q_rans_encode_host(uint16_t *out, size_t cap_words, int h, int w, const uint16_t *qy, const uint32_t *hist_in, long symbols_per_launch);
// true when every word names a level below 12 and a symbol its level's histogram counts: what the pass divides by.
bool q_words_ok(const uint16_t *qy, size_t n, const uint32_t *hist);
// Decoder front matter (q_entropy.cpp).
long q_decode_tables(const uint16_t *in, size_t n_words, int *h, int *w, uint32_t *freq, uint32_t *start, uint8_t *slot);

}  // namespace nblic
