// q_device_coder.hip -- the rANS pass of QNBLIC (effort 0; q_entropy.cpp, QNBLIC.c:238-253) on the GPU, one LANE per
// image, in launches that resume.
//
// The pass is one dependent chain per image -- per symbol a compare, a quotient by a table constant and an update -- so a
// lane is slow and the GPU's offer is width, as for the range coder (device_coder.hip, whose staging this kernel keeps):
// 64 jobs per block, rounds that are uniform across the wave, per round ONE coalesced fetch per stream of the aligned
// 512-byte window that holds its next 256 symbols, the windows parked in LDS rows padded to 65 words, the next round's
// 64 requests in flight while the current one is walked.  What differs:
//   backward windows   the pass runs last pixel first, so a job's windows are walked from the last one down and each
//                      window from its last position down.  The first window of a launch is partial (the image ends
//                      inside it, or the previous launch stopped there): q_rans_span (q_rans.h) gives every round's
//                      positions [lo, hi) and nothing outside them is translated or walked -- behind an image's last pixel
//                      stand the pipeline's pad word and raw histogram, or the words this job has already emitted.
//   lookups off the chain   every image has its own table of 12 x 256 (f, start) pairs.  A quarter of a window at a
//                      time, the whole wave translates the parked words of all 64 streams into their table entries
//                      (64 gathers per thread, independent of one another and of every coder), and parks those in a second
//                      LDS tile; a lane's walk then reads LDS only and its chain is q_rans_put: the renormalisation
//                      compare, the quotient (float estimate from below + one correction, 24-bit multiplies) and the update.
//                      1 / f comes from v_rcp_f32 in the walk, off the chain as well; (a 64-bit entry with 1 / f in it would
//                      need a 33 KB tile for 64 positions, and the two tiles together more than 64 KB of LDS.)
//   resumable          a launch advances every live job by at most `budget` symbols and leaves x, the symbols left, the
//                      words emitted and the overflow flag in the job's record; its duration depends on the budget,
//                      never on an image's size.
//   output             word k of the pass goes to out_end[-1 - k]: descending addresses, the order the decoder reads.
//                      A region that is too small sets the overflow flag; the job goes on consuming, stores nothing more
//                      and reports 0xFFFFFFFF.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_owned.h"
#include "q_device_coder.h"

namespace nblic {

#define NB_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kQRowWords = 65;                                   // of both tiles: u32x2 of a raw window, entries of a quarter
constexpr uint32_t kQQuarter = 64;                               // positions translated and walked together

__device__ inline uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), d, 64)));
    return v;
}
__device__ inline uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, uint32_t(__shfl_xor(int(v), d, 64)));
    return v;
}

__global__ void __launch_bounds__(64) k_q_rans_lanes(QRansJob *jobs, int n_jobs, uint32_t budget) {
    __shared__ u32x2 raw[64 * kQRowWords];
    __shared__ uint32_t tile[64 * kQRowWords];
    const int lane = int(threadIdx.x);
    const int id = int(blockIdx.x) * 64 + lane;
    const bool have = id < n_jobs;
    QRansJob *const job = jobs + (have ? id : n_jobs - 1);
    const bool live = have && job->live != 0u;
    QRansState s = job->st;
    const uint32_t left0 = live ? s.left : 0u;
    const uint32_t take = q_rans_take(left0, budget);
    const uint32_t my_rounds = q_rans_rounds(left0, take);
    const uint32_t rounds = wave_max(my_rounds);                   // wave-uniform: the job with the most windows sets their number
    const uint32_t top = left0 ? (left0 - 1u) / kQRansWindow : 0u;
    uint16_t *const out_end = job->out_end;
    const uint32_t cap = job->cap;

    // the pointers of the 64 streams and tables, fetched per stream with readlane (wave-uniform addresses)
    const uintptr_t src = uintptr_t(job->words), tab = uintptr_t(job->table);
    const uint32_t p_lo = uint32_t(src), p_hi = uint32_t(src >> 32), t_lo = uint32_t(tab), t_hi = uint32_t(tab >> 32);
    auto window = [&](int l, uint32_t round) {
        const uint32_t r_l = uint32_t(__builtin_amdgcn_readlane(int(my_rounds), l));
        if (r_l == 0u) return u32x2{0u, 0u};                      // an empty slot or a finished job: its pointer is not followed
        const uint64_t base = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(p_hi), l))) << 32) | uint32_t(__builtin_amdgcn_readlane(int(p_lo), l));
        const uint32_t w = uint32_t(__builtin_amdgcn_readlane(int(top), l)) - (round < r_l ? round : r_l - 1u);   // done for this launch: its last window again
        return ((NB_GLOBAL const u32x2 *)base)[size_t(w) * 64u + uint32_t(lane)];
    };
    u32x2 regs[64];
    if (rounds) {
#pragma unroll
        for (int l = 0; l < 64; l++) regs[l] = window(l, 0u);
    }
    for (uint32_t round = 0; round < rounds; round++) {
#pragma unroll
        for (int l = 0; l < 64; l++) raw[l * kQRowWords + lane] = regs[l];
        __syncthreads();
        if (round + 1 < rounds) {                                 // next round's windows: issued now, consumed after the walk
#pragma unroll
            for (int l = 0; l < 64; l++) regs[l] = window(l, round + 1u);
        }
        const QRansSpan sp = q_rans_span(left0, take, round);      // this lane's positions of its window; lo == hi: none
        const bool any = sp.hi > sp.lo;
        const uint32_t hi_max = wave_max(any ? sp.hi : 0u), lo_min = wave_min(any ? sp.lo : kQRansWindow);
        for (uint32_t quarter = (hi_max + kQQuarter - 1u) / kQQuarter; quarter-- > lo_min / kQQuarter;) {
            const uint32_t p0 = quarter * kQQuarter;
            // translate: stream l's words at p0 .. p0 + 63 into their table entries, one position per thread
#pragma unroll 8
            for (int l = 0; l < 64; l++) {
                const uint32_t lo_l = uint32_t(__builtin_amdgcn_readlane(int(sp.lo), l)), hi_l = uint32_t(__builtin_amdgcn_readlane(int(sp.hi), l));
                if (hi_l <= p0 || lo_l >= p0 + kQQuarter || hi_l <= lo_l) continue;                       // wave-uniform
                const uint64_t base = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(t_hi), l))) << 32) | uint32_t(__builtin_amdgcn_readlane(int(t_lo), l));
                const uint32_t p = p0 + uint32_t(lane);
                uint32_t e = 0u;
                if (p >= lo_l && p < hi_l) {
                    const uint32_t word = reinterpret_cast<const uint16_t *>(raw + l * kQRowWords)[p];
                    e = ((NB_GLOBAL const uint32_t *)base)[q_rans_index(word)];
                }
                tile[l * kQRowWords + lane] = e;
            }
            __syncthreads();
            // walk: this lane's positions of the quarter, last first, four entries fetched ahead of their steps
            // (a stream without positions in this quarter was skipped above, so its row is stale, and a group of four reaches
            // beyond [lo, hi): such entries, and the reciprocal of a zero one, are fetched and dropped -- the [lo, hi) gate in
            // front of q_rans_put is what keeps them out of every coder)
            const uint32_t i_hi = min(hi_max - p0, kQQuarter), i_lo = lo_min > p0 ? lo_min - p0 : 0u;
            for (uint32_t g = (i_hi + 3u) / 4u; g-- > i_lo / 4u;) {
                uint32_t e[4]; float rf[4];
#pragma unroll
                for (int k = 0; k < 4; k++) { e[k] = tile[lane * kQRowWords + int(g) * 4 + k]; rf[k] = q_rans_rcp(e[k] & 0xFFFFu); }
#pragma unroll
                for (int k = 3; k >= 0; k--) {
                    const uint32_t p = p0 + g * 4u + uint32_t(k);
                    if (p >= sp.lo && p < sp.hi) q_rans_put(s, e[k], rf[k], out_end, cap);
                }
            }
            __syncthreads();
        }
    }
    if (live) {
        s.left = left0 - take;
        if (s.left == 0u) {
            const uint32_t words = q_rans_flush(s, out_end, cap);
            ((NB_GLOBAL uint32_t *)job->result)[0] = words;
            job->live = 0u;
        }
        job->st = s;
    }
}

bool device_q_rans(QRansJob *d_jobs, int n_jobs, uint32_t budget, hipStream_t s) {
    if (n_jobs <= 0) return true;
    hipLaunchKernelGGL(k_q_rans_lanes, dim3(unsigned((n_jobs + 63) / 64)), dim3(64), 0, s, d_jobs, n_jobs, budget ? budget : 1u);
    return hipGetLastError() == hipSuccess;
}

// ---- the quotient against 64-bit division ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_q_quot_selftest(unsigned long long *bad) {
    const uint32_t f = blockIdx.x + 1u;                            // 1 .. 32767
    uint32_t mine = 0u;
    for (uint32_t k = threadIdx.x; k < kQRansSelftestCount; k += 256u) mine += q_rans_selftest_one(k, f);
    if (mine) atomicAdd(bad, (unsigned long long)mine);
}

long device_q_quot_selftest(hipStream_t s) {
    DevBuf<unsigned long long> d_bad; Pinned<unsigned long long> h_bad;
    if (d_bad.alloc(1) != hipSuccess || h_bad.alloc(1) != hipSuccess || hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_q_quot_selftest, dim3(32767), dim3(256), 0, s, d_bad.get());
    const bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h_bad, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s) == hipSuccess;
    if (hipStreamSynchronize(s) != hipSuccess || !ok) return -1;
    return long(h_bad[0]);
}

}  // namespace nblic
