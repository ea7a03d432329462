// device_coder.h -- the range-coder stage on the GPU, one lane per image (device_coder.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nblic {

// One image of a device-coder launch (array in device memory; lane = index & 63 of wave index / 64).
struct RcJob {
    const uint16_t *coded;     // an image on its own: prob | bin << 15 per bin; 256-byte aligned, readable to the end of its last 512-byte window
    const uint64_t *rows;      // a lane of a pack (then coded is null): the pack's rows, rows[(13 g + j) * 8 + lane] (kernels_e1.h E1Job::pack_rows);
    uint32_t lane;             //   only the word rows of groups that hold a bin of this image are read (13 * ceil(n / 64))
    uint8_t *out;              // device buffer for the coder bytes (no header)
    uint32_t *len_out;         // bytes written (flush included), or 0xFFFFFFFF when cap was too small
    uint32_t n, cap;
};

bool device_range_code(const RcJob *d_jobs, int n_jobs, hipStream_t s);

}  // namespace nblic
