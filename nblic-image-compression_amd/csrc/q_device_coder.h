// q_device_coder.h -- QNBLIC's rANS pass on the GPU, one lane per image, in resumed launches (q_device_coder.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "q_rans.h"

namespace nblic {

// One image of the device stage (array in device memory; lane = index & 63 of wave index / 64).  The host fills a
// record once; from then on `st` and `live` are the kernel's, launch after launch, until it has written `result`.
struct QRansJob {
    const uint16_t *words;     // level | symbol << 8 per pixel; 256-byte aligned, readable to the end of the 512-byte window that holds the last pixel.
                               //   What stands behind the last pixel is fetched and never used
    const uint32_t *table;     // the image's 12 x 256 entries of f | start << 16 (q_rans.h)
    uint16_t *out_end;         // one past the last word of the output region: word k of the pass goes to out_end[-1 - k].
                               //   May be the end of the buffer `words` points into: the pass never emits more words than it has consumed symbols
    uint32_t *result;          // written once, by the launch that codes pixel 0: the words of the pass (flush included), or 0xFFFFFFFF when cap was too small
    uint32_t cap;              // words of the output region
    uint32_t live;             // 1: to be advanced; 0: an empty slot, or a finished job
    QRansState st;             // q_rans_begin; what a launch leaves for the next
};

// One launch: every live job advances by at most `budget` symbols (>= 1).
bool device_q_rans(QRansJob *d_jobs, int n_jobs, uint32_t budget, hipStream_t s);
// The quotient routines of q_rans.h on the device against 64-bit division (q_rans_selftest_count operands per f, every
// f in 1 .. 32767).  Returns the number of mismatches, or -1.
long device_q_quot_selftest(hipStream_t s);

}  // namespace nblic
