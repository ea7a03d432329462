// kernels_e1.hip -- hand-written gfx950 kernels for the -e1 lossless NBLIC encoder.
//
// The reference codes pixels in raster order through four pieces of adaptive state
// (NBLIC.c:752-756: context-bias table, symbol re-mappers, binary counter trees, coder
// interval).  Each table ENTRY is an independent chain, so the state is replayed one key
// at a time over a stable (raster-order-preserving) partition of the work items:
//
//   k_predict            S1  stateless, one lane per pixel        -> rec1[t]
//   partition by adr     (count -> scan -> scatter)               -> s2in[]  grouped by context, pos2[t]
//   k_bias_blocks/_fixup S2  one LANE per 4096-record block of a context chain (monotone coupling; blocks whose copies
//                            did not meet: k_bias_tabulate / k_bias_replay)                  -> s2out[] (state >> 7)
//   partition by px|sign (gathers s2out through pos2)             -> s3in[]  grouped by re-mapper, pos3[t]
//   k_mapper_chains      S3  one LANE per re-mapper chain (16 per wave), counts in LDS -> s3out[] (z, same order);
//                            a chain that holds most of an image is cut into blocks (k_map_plan .. k_map_check)
//   k_count_bins/k_emit_bins  S4 stateless (gathers z through pos3)     -> events[r]
//   partition by counter (even / odd trees; hot chains staged in LDS) -> tin[] grouped by counter, two position arrays
//   k_counter_epochs     S5a one WAVE per counter chain: resolves the halvings        -> win_recs[]
//   k_counter_probs      S5b one WAVE per 512-touch window: P before every touch      -> tout[] (same order as tin)
//   k_mix                gathers the two P through the position arrays, mixes, packs  -> coded[r] (u16) for the host coder
//
// The chain kernels are the serial part, so they touch memory only as dense streams of 2-byte
// records in key-sorted order: every global request of a chain kernel is one coalesced 512-byte
// line run staged through LDS.  The scatter/gather between raster order and key order is done
// by the surrounding full-occupancy passes, which hide its latency behind thousands of waves.
//
// Wave64 throughout; no MFMA (nothing here is a contraction).  Every launch covers a GROUP of
// images (E1Job array in device memory, job = last grid dimension), so the serial chains of
// many images run side by side on different CUs by construction.
#include <hip/hip_runtime.h>
#include "model.h"
#include "kernels_e1.h"
#include "lsq_f64.h"
#include "serial_engine.h"

namespace nblic {

// ------------------------------------------------------------------------------------------
// wave helpers
// ------------------------------------------------------------------------------------------
// Pointers that are read out of the job record are generic ("flat") to the compiler; telling it
// they are global memory turns flat_load/flat_store into global_load/global_store and keeps the
// LDS counter out of every memory wait.
#define NB_GLOBAL __attribute__((address_space(1)))
// plain clang vectors: unlike HIP's uint2/uint4 classes they can be loaded/stored through
// address-space-qualified pointers
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ NB_GLOBAL T *gptr(T *p) {
    return (NB_GLOBAL T *)p;
}

__device__ __forceinline__ int lane_id() { return int(threadIdx.x & 63); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// Workgroups are dealt to the 8 XCDs round-robin (blocks b and b + 8 share an XCD, each XCD has an L2 of
// its own), so with the plain blockIdx -> work mapping every L2 sees every 8th piece of a raster-ordered
// pass: a gather through key-sorted positions then pulls each 64-byte line of a chain into all eight L2s
// (8x the fetches), and a scatter leaves every line partially written in eight places.  With this mapping
// XCD c works on the c-th CONTIGUOUS eighth of the pass, so a chain's lines are fetched / completed once.
// The launch pads gridDim.x to a multiple of 8 (the kernels' own range checks drop the surplus blocks); if
// the hardware deals differently nothing breaks, the mapping is a bijection either way.
__device__ __forceinline__ uint32_t xcd_block() {
    const uint32_t b = blockIdx.x, per = gridDim.x >> 3;
    return (b & 7u) * per + (b >> 3);
}

// the 32-bit LDS address of an object in __shared__ memory (for hand-issued ds_ instructions)
template <class T>
__device__ __forceinline__ uint32_t lds_address(const T *p) {
    return uint32_t(uintptr_t((const __attribute__((address_space(3))) T *)p));
}

// Mask of the valid lanes holding the same BITS-bit key as this lane.  Per key bit: the bit spread over the lane's
// word (v_bfe_i32: 0 or ~0), one compare for the ballot of the lanes that have it set, and the lanes that DIFFER from
// this one in that bit are ballot ^ spread -- accumulated with ORs, inverted once at the end.  Six VALU operations per
// bit; the scatter kernels' walks are bound by VALU issue (a wave64 operation occupies its SIMD for four cycles, and
// k_touch_scatter holds two waves per SIMD), and the first formulation -- a select between the ballot and its
// complement per bit, with the validity folded into every ballot -- compiled to twelve.
template <int BITS>
__device__ __forceinline__ uint64_t match_lanes(uint32_t key, bool valid) {
    uint32_t dlo = 0u, dhi = 0u;
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const int spread = __builtin_amdgcn_sbfe(int(key), uint32_t(b), 1u);
        const uint64_t set = __builtin_amdgcn_ballot_w64(spread != 0);          // invalid lanes vote too; they are masked out below
        dlo |= uint32_t(set) ^ uint32_t(spread);
        dhi |= uint32_t(set >> 32) ^ uint32_t(spread);
    }
    const uint64_t m = ~((uint64_t(dhi) << 32) | dlo) & __builtin_amdgcn_ballot_w64(valid);
    return valid ? m : 0ull;
}

// inclusive wave prefix sum (64 lanes)
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(v, d, 64);
        if (lane_id() >= d) v += o;
    }
    return v;
}

// Same prefix sum on the DPP crossbar (no LDS round trips): Kogge-Stone inside each 16-lane
// row with row_shr, then row_bcast:15 into rows 1/3 and row_bcast:31 into rows 2/3.
__device__ __forceinline__ uint32_t wave_scan_incl_dpp(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xf, 0xf, true));    // row_shr:1
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xf, 0xf, true));    // row_shr:2
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xf, 0xf, true));    // row_shr:4
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xf, 0xf, true));    // row_shr:8
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1,3
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2,3
    return v;
}

// P(bin==1) = floor(4096 * c1 / (c0 + c1)) without the integer-divide expansion: c1 and the sum
// are < 2^14, so 4096*c1 and the sum are exact floats, the reciprocal estimate is off by far
// less than one, and one remainder check makes the quotient exact.
__device__ __forceinline__ uint32_t prob_one(int c1, int sum) {
    int n = c1 << 12;
    int q = int(float(n) * __builtin_amdgcn_rcpf(float(sum)));
    int r = n - q * sum;
    q += (r >= sum) - (r < 0);
    return uint32_t(q);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), d, 64)));
    return v;
}

__device__ __forceinline__ uint32_t read_lane(uint32_t v, int l) { return uint32_t(__builtin_amdgcn_readlane(int(v), l)); }
// v_writelane_b32: lane `l` of the result takes the uniform `value`, the other lanes keep `old`
template <int L>
__device__ __forceinline__ int write_lane(int value, int old) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(value), "n"(L));
    return old;
}
// three registers at one run-time lane (the lane select goes through m0: one SGPR operand per VOP)
__device__ __forceinline__ void write_lane3(int l, int a, int b, int c, int &ra, int &rb, int &rc) {
    asm("s_mov_b32 m0, %6\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %4, m0\n\tv_writelane_b32 %2, %5, m0"
        : "+v"(ra), "+v"(rb), "+v"(rc) : "s"(a), "s"(b), "s"(c), "s"(l) : "m0");
}

// Lane-per-key streaming: each of the wave's 64 lanes owns one run of 2-byte records
// in[r .. end) and must replace every record by step(record) in order.  Per round the wave
// stages, for each stream, the aligned 512-byte window that holds its next records with ONE
// coalesced request (64 lanes x 8 B of the same stream), every lane then walks its own LDS row
// in place, and the windows are written back the same way.  All 64 requests of the NEXT round
// are in flight (128 VGPRs) while the current round is walked, so the serial walk never waits on
// HBM.  Rows are padded to 65 words so the walk (all lanes on the same column of different
// rows) is bank-conflict free.  Arrays must be padded by 512 B: a window may extend past the
// last record, and finished streams keep re-reading their last window.  Records before
// `out_from` are walked (warm-up) but never written back.
constexpr int kRowWords = 65;

template <class StepFn>
__device__ __forceinline__ void run_lane_streams(NB_GLOBAL const uint16_t *in, NB_GLOBAL uint16_t *out, uint32_t r,
                                                 const uint32_t end, const uint32_t out_from, u32x2 *stage, StepFn step,
                                                 NB_GLOBAL unsigned long long *dbg = nullptr) {
    const int lane = lane_id();
    unsigned long long t_stage = 0, t_walk = 0, t_flush = 0, rounds = 0, t0 = 0;
#define NB_STAMP(acc) do { if (dbg) { unsigned long long t1_ = __builtin_amdgcn_s_memtime(); acc += t1_ - t0; t0 = t1_; } } while (0)
    if (dbg) t0 = __builtin_amdgcn_s_memtime();
    const auto in_w = (NB_GLOBAL const u32x2 *)in;
    const auto out_w = (NB_GLOBAL u32x2 *)out;
    bool live = r < end;
    uint64_t active = __ballot(live);
    if (active == 0ull) return;
    uint32_t base = r & ~3u;                                 // window = records [base, base + 256)
    u32x2 regs[64];
#pragma unroll
    for (int l = 0; l < 64; l++) regs[l] = in_w[(read_lane(base, l) >> 2) + lane];
    for (;;) {
        const uint32_t cur_r = r, cur_base = base;
        const uint32_t cur_stop = live ? min(end, base + 256u) : r;
        const uint64_t cur_active = active;
        const bool cur_live = live;
#pragma unroll
        for (int l = 0; l < 64; l++) stage[l * kRowWords + lane] = regs[l];
        __syncthreads();
        r = cur_stop; live = r < end; active = __ballot(live); base = r & ~3u;
        if (active != 0ull) {                                // next round's windows: issue now, use after the walk
#pragma unroll
            for (int l = 0; l < 64; l++) regs[l] = in_w[(read_lane(base, l) >> 2) + lane];
        }
        NB_STAMP(t_stage);
        const int c0 = int(cur_r - cur_base), c1 = int(cur_stop - cur_base);   // ---- walk own row: columns [c0, c1)
        for (int wi = 0; wi < 64; wi++) {
            const bool mine = cur_live && wi * 4 + 3 >= c0 && wi * 4 < c1;
            if (__ballot(mine) == 0ull) continue;
            if (mine) {
                u32x2 w = stage[lane * kRowWords + wi];
                uint32_t rec[4] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int col = wi * 4 + k;
                    if (col >= c0 && col < c1) rec[k] = step(rec[k], cur_base + uint32_t(col)) & 0xFFFFu;
                }
                stage[lane * kRowWords + wi] = u32x2{rec[0] | (rec[1] << 16), rec[2] | (rec[3] << 16)};
            }
        }
        __syncthreads();
        NB_STAMP(t_walk);
        for (int l = 0; l < 64; l++) {                       // ---- write windows back
            if (((cur_active >> l) & 1ull) == 0ull) continue;
            const uint32_t b = read_lane(cur_base, l), lo = max(read_lane(cur_r, l), read_lane(out_from, l)), hi = read_lane(cur_stop, l);
            const uint32_t idx = b + uint32_t(lane) * 4u;
            if (idx + 4u <= lo || idx >= hi) continue;
            const u32x2 w = stage[l * kRowWords + lane];
            if (idx >= lo && idx + 4u <= hi) {
                out_w[idx >> 2] = w;
            } else {                                         // window edge: only this stream's records
                const uint32_t rec[4] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16};
#pragma unroll
                for (int k = 0; k < 4; k++) if (idx + k >= lo && idx + k < hi) out[idx + k] = uint16_t(rec[k]);
            }
        }
        __syncthreads();
        NB_STAMP(t_flush); rounds++;
        if (active == 0ull) break;
    }
    if (dbg && lane == 0) { dbg[0] = t_stage; dbg[1] = t_walk; dbg[2] = t_flush; dbg[3] = rounds; }
#undef NB_STAMP
}

// ------------------------------------------------------------------------------------------
// S1: predictor, activity level, context address.  NBLIC.c:287-410.
// In lossless mode the reconstruction IS the input, so S1 carries no state at all: every pixel is
// a function of the 12 input pixels around it and of the prediction of its left neighbour
// (err_prev, NBLIC.c:808/:878).  The stage is the one bandwidth-shaped kernel of the path (1 B/px
// in, a 4-byte record out), so it is written for wide memory operations and few instructions:
//
//   k_predict_rows    the interior: a lane owns EIGHT consecutive pixels of one row (columns 8.. of rows
//                     2..).  Three 16-byte loads (rows i, i-1, i-2, columns j0-4 .. j0+11) give it every tap
//                     of its run in registers; it predicts the pixel left of the run once (9 predictions
//                     per 8 pixels, nothing re-read, no cross-lane traffic), walks the run carrying the
//                     previous prediction, and stores the eight records as two 16-byte stores.  The
//                     level interpolation's integer divide is a 201-entry LDS table.
//   k_predict_border  everything with a fall-back tap (rows 0-1; the first 8 and the last 4-11 columns of
//                     the other rows; images narrower than 20): one lane per pixel, byte loads, the chained
//                     fall-backs of model.h sample_taps.  < 1 % of a large frame.
// ------------------------------------------------------------------------------------------
typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));    // a 16-byte load / store at any byte address
typedef uint32_t u32x4_dw __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int interior_runs(int w) { return w >= 20 ? (w - 12) / 8 : 0; }   // runs of 8 columns from column 8; taps reach j0-4 .. j0+11

// BAND (a row band of the band encoder, e1_launch_front_band): b.img / b.rec1 start at image row J.row0, the plane goes
// on above b.img, and what decides a pixel's fall-backs is its row in the IMAGE.  The batch pipeline launches <false>.
template <bool BAND>
__global__ void __launch_bounds__(256) k_predict_rows(const E1Job *__restrict__ jobs) {
    __shared__ uint16_t qlut[208];                                        // activity (clipped to 200) -> qu | qv << 4 | qw << 8
    if (threadIdx.x < 208) {
        const Level L = quantise(threadIdx.x < 200 ? int(threadIdx.x) : 200);
        qlut[threadIdx.x] = uint16_t(L.qu | (L.qv << 4) | (L.qw << 8));
    }
    __syncthreads();
    const E1Job &J = jobs[blockIdx.z];
    const int w = J.w;
    // i: the row's index in b.img / b.rec1.  A band visits its rows 0 and 1 too: they are interior rows when two image
    // rows lie above them, and the three loads below then reach above b.img, into the plane.
    const int run = int(blockIdx.x) * 256 + int(threadIdx.x), i = BAND ? int(blockIdx.y) : int(blockIdx.y) + 2;
    if (i >= J.h || run >= interior_runs(w)) return;
    if (BAND && J.row0 + i < 2) return;
    const int j0 = 8 + 8 * run;
    const auto at = gptr(J.b.img) + (size_t(i) * size_t(w) + size_t(j0 - 4));
    const u32x4 r0 = *(NB_GLOBAL const u32x4_any *)at;
    const u32x4 r1 = *(NB_GLOBAL const u32x4_any *)(at - w);
    const u32x4 r2 = *(NB_GLOBAL const u32x4_any *)(at - 2 * size_t(w));
    auto px = [](const u32x4 &v, int k) { return int((v[k >> 2] >> (8 * (k & 3))) & 0xFFu); };   // k is a constant after unrolling
    auto taps_at = [&](int c) {                                           // window column c = image column j0 - 4 + c
        Taps n;
        n.a = px(r0, c - 1); n.e = px(r0, c - 2);
        n.b = px(r1, c); n.c = px(r1, c - 1); n.d = px(r1, c + 1); n.q = px(r1, c - 2); n.t = px(r1, c + 2);
        n.f = px(r2, c); n.g = px(r2, c + 1); n.h = px(r2, c - 1); n.r = px(r2, c + 2); n.s = px(r2, c - 2);
        return n;
    };
    int px_left = predict(taps_at(3));                                    // the pixel left of the run
    uint32_t rec[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const Taps n = taps_at(4 + q);
        const int px0 = predict(n);
        const int delta = activity(n, clip_err(n.a, px_left));
        const uint32_t e = qlut[delta < 200 ? delta : 200];
        const Level L{int(e & 15u), int((e >> 4) & 15u), int(e >> 8)};
        rec[q] = pack_s1(px0, context_address(n, L.qu, px0), L);
        px_left = px0;
    }
    const auto out = gptr(J.b.rec1) + (size_t(i) * size_t(w) + size_t(j0));
    *(NB_GLOBAL u32x4_dw *)out = u32x4{rec[0], rec[1], rec[2], rec[3]};
    *(NB_GLOBAL u32x4_dw *)(out + 4) = u32x4{rec[4], rec[5], rec[6], rec[7]};
}

// top == 1: rows 0 and 1, every column (grid.y = 2);  top == 0: rows 2.., the columns k_predict_rows leaves out.
// BAND: `top` takes the band's rows that are image rows 0 / 1 (none when row0 >= 2), the other launch (grid.y = the band's
// rows) the rest; sample_taps sees the row in the image, and reads relative to the plane.
template <bool BAND>
__global__ void __launch_bounds__(64) k_predict_border(const E1Job *__restrict__ jobs, int top) {
    const E1Job &J = jobs[blockIdx.z];
    const int w = J.w;
    const int i = top || BAND ? int(blockIdx.y) : int(blockIdx.y) + 2;   // the row's index in b.img / b.rec1
    const int row0 = BAND ? J.row0 : 0;
    if (BAND && (row0 + i < 2) != (top != 0)) return;
    int j = int(blockIdx.x) * 64 + int(threadIdx.x);
    if (!top) {
        const int first_right = 8 + 8 * interior_runs(w);                 // == w when there is no interior at all
        if (interior_runs(w) == 0) { if (blockIdx.x) return; }
        else j = j < 8 ? j : first_right + (j - 8);
    }
    if (i >= J.h || j >= w) return;
    const auto img = gptr(J.b.img);
    auto pix = [&](int r, int c) {                                        // r: row in the image
        if (BAND) return int(img[(ptrdiff_t(r) - ptrdiff_t(row0)) * ptrdiff_t(w) + ptrdiff_t(c)]);
        return int(img[size_t(r) * size_t(w) + size_t(c)]);
    };
    Taps n = sample_taps(pix, w, row0 + i, j);
    int px0 = predict(n);
    int err_prev = 0;
    if (j > 0) {
        Taps m = sample_taps(pix, w, row0 + i, j - 1);
        err_prev = clip_err(n.a, predict(m));
    }
    Level L = quantise(activity(n, err_prev));
    gptr(J.b.rec1)[size_t(i) * size_t(w) + size_t(j)] = pack_s1(px0, context_address(n, L.qu, px0), L);
}

// ------------------------------------------------------------------------------------------
// Stable partition = per-segment histogram -> exclusive scan of table[key][segment] ->
// ranked scatter.  One wave owns one segment (a contiguous run of items in raster order)
// and keeps its histogram / running offsets in its own LDS slice, so no barriers are needed.
// ------------------------------------------------------------------------------------------
template <int NKEYS>
__device__ __forceinline__ void lds_fill(uint32_t *slice, uint32_t v) {
    for (int k = lane_id(); k < NKEYS; k += 64) slice[k] = v;
}

// ---- the two context models that share the partition + coupled-chain machinery -------------
// NBLIC -e1 (NBLIC.c:413-428): 2048 contexts, clipped 8-bit error, v' = (127 v + 256 e + 64) >> 7,
// |v| <= 32576, consumer reads v >> 7.   QNBLIC (QNBLIC.c:176-188): 3072 contexts, unclipped
// 9-bit error, v' = (127 v + 2048 e + 63) >> 7, |v| <= 522303, consumer reads v >> 10.
struct NbModel {
    static constexpr int kKeys = kContexts, kKeyBits = 11, kExtreme = 32576, kOutShift = kCtxScale - 1, kScanSel = 0;
    static __device__ __forceinline__ uint32_t key(uint32_t rec) { return uint32_t(s1_adr(rec)); }
    static __device__ __forceinline__ uint16_t err_rec(int x, uint32_t rec) { return uint16_t(clip_err(x, s1_px0(rec)) & 0xFF); }
    static __device__ __forceinline__ int err_of(uint32_t rec16) { return int(int8_t(rec16)); }
    static __device__ __forceinline__ int update(int v, int e) { return bias_update(v, e); }
};
struct QModel {
    static constexpr int kKeys = 3072, kKeyBits = 12, kExtreme = 1 << 20, kOutShift = 10, kScanSel = 4;
    static __device__ __forceinline__ uint32_t key(uint32_t rec) { return (rec >> 8) & 0xFFFu; }
    static __device__ __forceinline__ uint16_t err_rec(int x, uint32_t rec) { return uint16_t((x - int(rec & 0xFF)) & 0xFFFF); }
    static __device__ __forceinline__ int err_of(uint32_t rec16) { return int(int16_t(rec16)); }
    static __device__ __forceinline__ int update(int v, int e) { return (v * 128 - v + e * 2048 + 63) >> 7; }
};

// ---- partition 1: pixels by context address ------------------------------------------------
template <class M>
__global__ void __launch_bounds__(256) k_adr_count(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t lds[4][M::kKeys];
    const E1Job &J = jobs[blockIdx.y];
    const auto rec1 = gptr(J.b.rec1); const auto table = gptr(J.b.table);
    const uint32_t n = J.n; const SegPlan plan = J.pp;
    int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    // the scan that follows raises this flag for an image with too many touches for 28-bit positions (k_touch_scatter)
    if (seg == 0 && lane_id() == 0) gptr(J.b.totals)[kWideTouchFlag] = (J.dbg & 256) ? 1u : 0u;   // (NBLIC_AMD_DBG & 256: plain 32-bit positions for every image -- tests, A/B runs)
    uint32_t *hist = lds[threadIdx.x >> 6];
    lds_fill<M::kKeys>(hist, 0);
    uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n, lo + plan.seg_len);
    for (uint32_t base = lo; base < hi; base += 512) {            // eight rows of loads in flight (see k_touch_count)
        uint32_t r[8];
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = rec1[min(base + 64u * uint32_t(k) + uint32_t(lane_id()), hi - 1)];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (base + 64u * uint32_t(k) + uint32_t(lane_id()) < hi) atomicAdd(&hist[M::key(r[k])], 1u);
    }
    for (int k = lane_id(); k < M::kKeys; k += 64) table[size_t(k) * plan.nseg + seg] = hist[k];
}

template <class M>
__global__ void __launch_bounds__(256) k_adr_scatter(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t lds[4][M::kKeys];
    const E1Job &J = jobs[blockIdx.y];
    const auto rec1 = gptr(J.b.rec1); const auto x = gptr(J.b.img);
    const auto table = gptr(J.b.table); const auto s2in = gptr(J.b.s2in); const auto pos2 = gptr(J.b.pos2);
    const uint32_t n = J.n; const SegPlan plan = J.pp;
    int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    uint32_t *off = lds[threadIdx.x >> 6];
    for (int k = lane_id(); k < M::kKeys; k += 64) off[k] = table[size_t(k) * plan.nseg + seg];
    uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n, lo + plan.seg_len);
    // rows are fetched eight at a time, one group ahead, with clamped addresses (see k_touch_scatter:
    // a load consumed while stores are in flight drains them all, so the drain is paid per group)
    if (lo >= hi) return;
    constexpr int kRows = 8;
    uint32_t cur_r[kRows], nxt_r[kRows], cur_x[kRows], nxt_x[kRows];
    auto fetch = [&](uint32_t base, uint32_t (&rr)[kRows], uint32_t (&xx)[kRows]) {
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const uint32_t t = min(base + 64u * uint32_t(k) + uint32_t(lane_id()), hi - 1);
            rr[k] = rec1[t]; xx[k] = x[t];
        }
    };
    fetch(lo, cur_r, cur_x);
    for (uint32_t gbase = lo; gbase < hi; gbase += 64u * kRows) {
        fetch(gbase + 64u * kRows, nxt_r, nxt_x);
#pragma unroll 1
        for (int k = 0; k < kRows && gbase + 64u * uint32_t(k) < hi; k++) {
            const uint32_t t = gbase + 64u * uint32_t(k) + uint32_t(lane_id());
            const bool valid = t < hi;
            const uint32_t r = cur_r[k];
            const uint32_t key = M::key(r);
            const uint64_t same = match_lanes<M::kKeyBits>(key, valid);
            if (valid) {
                const uint32_t rank = __popcll(same & lanes_below());
                const uint32_t pos = off[key] + rank;
                s2in[pos] = M::err_rec(int(cur_x[k]), r);
                pos2[t] = pos;
                if (rank == 0) off[key] += uint32_t(__popcll(same));
            }
        }
#pragma unroll
        for (int k = 0; k < kRows; k++) { cur_r[k] = nxt_r[k]; cur_x[k] = nxt_x[k]; }
    }
}

// ---- S2: context-bias chains (NBLIC.c:413-428), parallel in TIME by monotone coupling -------
// The chain itself only needs the clipped error of each pixel and only has to publish the
// state it held BEFORE that pixel: record in = err (low byte), record out = v >> 7, from which
// the consumer rebuilds sign = out & 1 and px = clip(px0 + (out >> 1) + sign).
//
// v' = (127 v + 256 e + 64) >> 7 is non-decreasing in v and |v| <= 32576.  So if two copies
// started from -32576 and +32576 are fed the same errors and meet, every possible start has met
// them: the state is known EXACTLY without knowing where it came from.  On image data they meet
// within ~2100 records (the error dithers the floor).  Each chain is therefore cut into blocks
// of kBiasBlock records; a lane warms both copies up over the kBiasWarm records before its
// block, takes the common state if they met, and replays its block.  Blocks whose copies did
// not meet (flat regions: a constant error parks them 127 apart) are resolved through TABLES:
//
// The gap of the two copies obeys g' <= ceil(127 g / 128), so after kBiasWarm records it is below kBiasCands
// whatever the errors were (from 2 * kExtreme: 869 steps for NbModel, 1311 for QModel), and by monotonicity
// the true state at the block's first record is one of the <= 128 values [va, vb].  k_bias_tabulate replays the
// block from every candidate -- a lane each, all lanes on the same record -- and keeps only the end states; k_bias_fixup
// then walks a chain's blocks with ONE look-up per block (a candidate's image lies inside the next block's
// [va, vb]: a copy started earlier at an extreme stays inside one started later), which leaves every such block's exact
// start state, and k_bias_replay writes their outputs, a lane per block.  With E1Job::long_min < 0 none of this runs
// and such blocks are replayed from their predecessor's end state by k_bias_fixup, in order -- exact too, but serial.
constexpr uint32_t kBiasBlock = 4096, kBiasWarm = 3072;
constexpr int kBiasCands = 128;
// tables of an image: only a chain's blocks behind its first can fail to meet
__device__ __forceinline__ uint32_t bias_table_cap(const E1Job &J) { return J.n / kBiasBlock + 1u; }

// blocks per chain -> exclusive scan -> blk_base[kKeys + 1]; one 1024-thread block per job
template <class M>
__global__ void __launch_bounds__(1024) k_plan_blocks(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t part[16];
    const E1Job &J = jobs[blockIdx.y];
    const auto table = gptr(J.b.table); const auto blk_base = gptr(J.b.blk_base);
    const int nseg = J.pp.nseg;
    constexpr int kPer = M::kKeys / 1024;
    uint32_t cnt[kPer], sum = 0;
    for (int k = 0; k < kPer; k++) {
        int key = int(threadIdx.x) * kPer + k;
        uint32_t start = table[size_t(key) * nseg];
        uint32_t end = key + 1 < M::kKeys ? table[size_t(key + 1) * nseg] : J.n;
        cnt[k] = (end - start + kBiasBlock - 1) / kBiasBlock;
        sum += cnt[k];
    }
    uint32_t incl = wave_scan_incl(sum);
    if (lane_id() == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t pre = incl - sum;
    for (int wv = 0; wv < int(threadIdx.x >> 6); wv++) pre += part[wv];
    for (int k = 0; k < kPer; k++) { blk_base[threadIdx.x * kPer + k] = pre; pre += cnt[k]; }
    if (threadIdx.x == 1023) blk_base[M::kKeys] = pre;
    if (threadIdx.x < 3) { gptr(J.b.totals)[kLongS2Met + threadIdx.x] = 0u; gptr(J.b.totals)[kLongS3Split + threadIdx.x] = 0u; }   // the block counts of this front half
}

// which chain owns block `item`?  the largest key with blk_base[key] <= item
template <class M>
__device__ __forceinline__ int chain_of_block(NB_GLOBAL const uint32_t *blk_base, uint32_t item) {
    int lo = 0, hi = M::kKeys;                                        // invariant: blk_base[lo] <= item < blk_base[hi]
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (blk_base[mid] <= item) lo = mid; else hi = mid; }
    return lo;
}

// one LANE per block of any chain; grid.x is an upper bound on the block count
template <class M>
__global__ void __launch_bounds__(64) k_bias_blocks(const E1Job *__restrict__ jobs) {
    __shared__ u32x2 stage[64 * kRowWords];
    const E1Job &J = jobs[blockIdx.y];
    const auto s2in = gptr(J.b.s2in); const auto s2out = gptr(J.b.s2out); const auto table = gptr(J.b.table);
    const auto blk_base = gptr(J.b.blk_base); const auto blk_end = gptr(J.b.blk_end);
    const uint32_t n_items = blk_base[M::kKeys];
    const uint32_t item = blockIdx.x * 64u + threadIdx.x;
    if (blockIdx.x * 64u >= n_items) return;                          // whole wave idle
    const bool have = item < n_items;
    const int key = have ? chain_of_block<M>(blk_base, item) : 0;
    const int nseg = J.pp.nseg;
    const uint32_t c_start = table[size_t(key) * nseg];
    const uint32_t c_end = key + 1 < M::kKeys ? table[size_t(key + 1) * nseg] : J.n;
    const uint32_t blk = have ? item - blk_base[key] : 0u;
    const uint32_t b_start = c_start + blk * kBiasBlock;
    const uint32_t b_end = have ? min(c_end, b_start + kBiasBlock) : 0u;
    const uint32_t w_start = (blk == 0u || b_start - c_start <= kBiasWarm) ? c_start : b_start - kBiasWarm;
    // warming up from the chain's own first record starts from its true state: both copies equal
    const bool exact = w_start == c_start;
    const int v0 = gptr(J.b.ctx_state)[key];
    int va = exact ? v0 : -M::kExtreme, vb = exact ? v0 : M::kExtreme;
    bool met = false;
    int va0 = 0, vb0 = 0;                                             // the copies at the block's first record
    run_lane_streams(s2in, s2out, have ? w_start : 0u, b_end, b_start, stage, [&](uint32_t rec, uint32_t idx) {
        const int e = M::err_of(rec);
        if (idx == b_start) { met = va == vb; va0 = va; vb0 = vb; }   // did the two copies meet during the warm-up?
        uint32_t o = uint32_t(va >> M::kOutShift);
        va = M::update(va, e);
        if (idx < b_start) vb = M::update(vb, e);                     // warm-up: carry the second copy too
        return o;
    });
    if (have) { blk_end[item] = va; gptr(J.b.blk_ok)[item] = uint8_t(met); }
    const uint64_t n_met = __ballot(have && met);
    if (lane_id() == 0 && n_met) atomicAdd(J.b.totals + kLongS2Met, uint32_t(__popcll(n_met)));
    if (have && !met && J.long_min >= 0) {
        int table = -1;                                               // (the gap bound and the table count cannot fail; a block without a table is replayed in order)
        if (vb0 - va0 < kBiasCands) {
            const uint32_t t = atomicAdd(J.b.totals + kLongS2Table, 1u);
            if (t < bias_table_cap(J)) { table = int(t); gptr(J.b.blk_item)[t] = item; }
        }
        gptr(J.b.blk_cand)[2 * size_t(item)] = va0; gptr(J.b.blk_cand)[2 * size_t(item) + 1] = table;
    }
}

// one 128-lane workgroup per table: lane k replays the block from va + k and keeps the end state
template <class M>
__global__ void __launch_bounds__(kBiasCands) k_bias_tabulate(const E1Job *__restrict__ jobs) {
    __shared__ u32x2 recs[kBiasBlock / 4];
    const E1Job &J = jobs[blockIdx.y];
    const uint32_t t = blockIdx.x;
    if (t >= min(gptr(J.b.totals)[kLongS2Table], bias_table_cap(J))) return;
    const auto s2in = gptr(J.b.s2in); const auto table = gptr(J.b.table); const auto blk_base = gptr(J.b.blk_base);
    const uint32_t item = gptr(J.b.blk_item)[t];
    const int key = chain_of_block<M>(blk_base, item);
    const int nseg = J.pp.nseg;
    const uint32_t c_start = table[size_t(key) * nseg];
    const uint32_t c_end = key + 1 < M::kKeys ? table[size_t(key + 1) * nseg] : J.n;
    const uint32_t b_start = c_start + (item - blk_base[key]) * kBiasBlock;
    const uint32_t len = min(c_end, b_start + kBiasBlock) - b_start;
    const auto rec16 = reinterpret_cast<uint16_t *>(recs);
    for (uint32_t i = threadIdx.x; i < len; i += uint32_t(kBiasCands)) rec16[i] = s2in[b_start + i];
    __syncthreads();
    int v = min(gptr(J.b.blk_cand)[2 * size_t(item)] + int(threadIdx.x), M::kExtreme);
    uint32_t q = 0;                                                   // every lane reads the same word: an LDS broadcast
#pragma unroll 4
    for (; q < len / 4u; q++) {
        const u32x2 w = recs[q];
        v = M::update(v, M::err_of(w.x & 0xFFFFu)); v = M::update(v, M::err_of(w.x >> 16));
        v = M::update(v, M::err_of(w.y & 0xFFFFu)); v = M::update(v, M::err_of(w.y >> 16));
    }
    for (uint32_t i = q * 4u; i < len; i++) v = M::update(v, M::err_of(rec16[i]));
    gptr(J.b.blk_tab)[size_t(t) * kBiasCands + threadIdx.x] = v;
}

// one lane per chain: walks its blocks in order -- a met block's end state is known, a block with a table takes it from
// there (and leaves its exact start state for k_bias_replay), a block with neither is replayed here -- and publishes the
// final state
template <class M>
__global__ void __launch_bounds__(64) k_bias_fixup(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto s2in = gptr(J.b.s2in); const auto s2out = gptr(J.b.s2out); const auto table = gptr(J.b.table);
    const auto blk_base = gptr(J.b.blk_base); const auto blk_end = gptr(J.b.blk_end); const auto blk_ok = gptr(J.b.blk_ok);
    const int key = int(blockIdx.x) * 64 + int(threadIdx.x);
    const int nseg = J.pp.nseg;
    const uint32_t c_start = table[size_t(key) * nseg];
    const uint32_t c_end = key + 1 < M::kKeys ? table[size_t(key + 1) * nseg] : J.n;
    const uint32_t first = blk_base[key], count = blk_base[key + 1] - first;
    const auto blk_cand = gptr(J.b.blk_cand); const auto blk_tab = gptr(J.b.blk_tab);
    int v = gptr(J.b.ctx_state)[key];
    uint32_t serial = 0;
    for (uint32_t b = 0; b < count; b++) {
        if (blk_ok[first + b]) { v = blk_end[first + b]; continue; }
        const int tab = J.long_min >= 0 ? blk_cand[2 * size_t(first + b) + 1] : -1;
        if (tab >= 0) {
            const int va = blk_cand[2 * size_t(first + b)];
            blk_cand[2 * size_t(first + b)] = v;
            v = blk_tab[size_t(tab) * kBiasCands + size_t(iclip(v - va, 0, kBiasCands - 1))];
            blk_end[first + b] = v;
            continue;
        }
        serial++;
        const uint32_t lo = c_start + b * kBiasBlock, hi = min(c_end, lo + kBiasBlock);
        for (uint32_t r = lo; r < hi; r++) {
            s2out[r] = uint16_t(v >> M::kOutShift);
            v = M::update(v, M::err_of(s2in[r]));
        }
        blk_end[first + b] = v;
    }
    gptr(J.b.ctx_state)[key] = v;
    if (serial) atomicAdd(J.b.totals + kLongS2Serial, serial);
}

// one lane per table: the block's outputs from its exact start state
template <class M>
__global__ void __launch_bounds__(64) k_bias_replay(const E1Job *__restrict__ jobs) {
    __shared__ u32x2 stage[64 * kRowWords];
    const E1Job &J = jobs[blockIdx.y];
    const uint32_t n_tabs = min(gptr(J.b.totals)[kLongS2Table], bias_table_cap(J));
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (blockIdx.x * 64u >= n_tabs) return;                           // whole wave idle
    const bool have = t < n_tabs;
    const auto s2in = gptr(J.b.s2in); const auto s2out = gptr(J.b.s2out); const auto table = gptr(J.b.table);
    const auto blk_base = gptr(J.b.blk_base);
    const uint32_t item = have ? gptr(J.b.blk_item)[t] : 0u;
    const int key = have ? chain_of_block<M>(blk_base, item) : 0;
    const int nseg = J.pp.nseg;
    const uint32_t c_start = table[size_t(key) * nseg];
    const uint32_t c_end = key + 1 < M::kKeys ? table[size_t(key + 1) * nseg] : J.n;
    const uint32_t b_start = have ? c_start + (item - blk_base[key]) * kBiasBlock : 0u;
    const uint32_t b_end = have ? min(c_end, b_start + kBiasBlock) : 0u;
    int v = have ? gptr(J.b.blk_cand)[2 * size_t(item)] : 0;
    run_lane_streams(s2in, s2out, b_start, b_end, b_start, stage, [&](uint32_t rec, uint32_t) {
        const uint32_t o = uint32_t(v >> M::kOutShift);
        v = M::update(v, M::err_of(rec));
        return o;
    });
}

// ---- partition 2: pixels by (px, sign) (512 keys); symbols >= 20 bypass the re-mapper -----
// k_map_count also brings S2's output back to raster order (gather through pos2).
// GEN = the job's own near (the serial modes); otherwise the lossless constant, so the divide folds away
template <bool GEN = false>
__device__ __forceinline__ bool mapper_item(int x, uint32_t ps, uint32_t &key, int &y, const NearParams &np = NearParams{0, 1, 65537}) {
    int px = int(ps & 0xFF), sign = int(ps >> 8);
    y = GEN ? residual_to_symbol(x, px, sign, np) : residual_to_symbol(x, px, sign, 0);
    key = uint32_t(px) * 2u + uint32_t(sign);
    return y < kMapSyms;
}

__global__ void __launch_bounds__(256) k_map_count(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t lds[4][512];
    const E1Job &J = jobs[blockIdx.y];
    const auto x = gptr(J.b.img); const auto s2out = gptr(J.b.s2out);
    const auto pos2 = gptr(J.b.pos2); const auto pxs = gptr(J.b.pxs); const auto table = gptr(J.b.table);
    const auto rec1 = gptr(J.b.rec1);
    const uint32_t n = J.n; const SegPlan plan = J.pp;
    int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    // the scan that follows raises this flag for an image with too many touches for 28-bit positions (k_touch_scatter)
    if (seg == 0 && lane_id() == 0) gptr(J.b.totals)[kWideTouchFlag] = (J.dbg & 256) ? 1u : 0u;   // (NBLIC_AMD_DBG & 256: plain 32-bit positions for every image -- tests, A/B runs)
    uint32_t *hist = lds[threadIdx.x >> 6];
    lds_fill<512>(hist, 0);
    uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n, lo + plan.seg_len);
    // Two dependent loads per pixel (position, then the chain's output there): the positions of the
    // NEXT eight rows are fetched a group ahead, the eight gathers of the current group go out
    // together, so the loop pays one gather latency per 512 pixels instead of two per 64.
    if (lo < hi) {
        constexpr int kRows = 8;
        uint32_t p_cur[kRows], p_nxt[kRows], r_cur[kRows], r_nxt[kRows], x_cur[kRows], x_nxt[kRows];
        auto fetch = [&](uint32_t base, uint32_t (&pp)[kRows], uint32_t (&rr)[kRows], uint32_t (&xx)[kRows]) {
#pragma unroll
            for (int k = 0; k < kRows; k++) {
                const uint32_t t = min(base + 64u * uint32_t(k) + uint32_t(lane_id()), hi - 1);
                pp[k] = pos2[t]; rr[k] = rec1[t]; xx[k] = x[t];
            }
        };
        fetch(lo, p_cur, r_cur, x_cur);
        for (uint32_t gbase = lo; gbase < hi; gbase += 64u * kRows) {
            fetch(gbase + 64u * kRows, p_nxt, r_nxt, x_nxt);
            uint32_t v[kRows];
#pragma unroll
            for (int k = 0; k < kRows; k++) v[k] = s2out[p_cur[k]];
#pragma unroll
            for (int k = 0; k < kRows; k++) {
                const uint32_t t = gbase + 64u * uint32_t(k) + uint32_t(lane_id());
                if (t < hi) {
                    const int vs = int(int16_t(v[k]));                 // context state >> 7 as the chain saw it
                    const int sign = vs & 1;
                    const uint16_t ps = uint16_t(iclip(s1_px0(r_cur[k]) + (vs >> 1) + sign, 0, kMaxVal) | (sign << 8));
                    uint32_t key; int y;
                    pxs[t] = ps;
                    if (mapper_item(int(x_cur[k]), ps, key, y)) atomicAdd(&hist[key], 1u);
                }
            }
#pragma unroll
            for (int k = 0; k < kRows; k++) { p_cur[k] = p_nxt[k]; r_cur[k] = r_nxt[k]; x_cur[k] = x_nxt[k]; }
        }
    }
    for (int k = lane_id(); k < 512; k += 64) table[size_t(k) * plan.nseg + seg] = hist[k];
}

// The same histogram when px | sign was left in raster order by the serial model stage
// (serial_engine.hip k_serial_model): no gather, the job's own near.
__global__ void __launch_bounds__(256) k_map_count_pre(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t lds[4][512];
    const E1Job &J = jobs[blockIdx.y];
    const auto x = gptr(J.b.img); const auto pxs = gptr(J.b.pxs); const auto table = gptr(J.b.table);
    const uint32_t n = J.n; const SegPlan plan = J.pp;
    const NearParams np = near_params(J.near);
    int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    // the scan that follows raises this flag for an image with too many touches for 28-bit positions (k_touch_scatter)
    if (seg == 0 && lane_id() == 0) gptr(J.b.totals)[kWideTouchFlag] = (J.dbg & 256) ? 1u : 0u;   // (NBLIC_AMD_DBG & 256: plain 32-bit positions for every image -- tests, A/B runs)
    if (seg == 0 && lane_id() < 3) { gptr(J.b.totals)[kLongS2Met + lane_id()] = 0u; gptr(J.b.totals)[kLongS3Split + lane_id()] = 0u; }   // no S2 on this path; the re-mapper chains count from zero
    uint32_t *hist = lds[threadIdx.x >> 6];
    lds_fill<512>(hist, 0);
    uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n, lo + plan.seg_len);
    for (uint32_t base = lo; base < hi; base += 512) {
        uint32_t p[8], xx[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { const uint32_t t = min(base + 64u * uint32_t(k) + uint32_t(lane_id()), hi - 1); p[k] = pxs[t]; xx[k] = x[t]; }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t key; int y;
            if (base + 64u * uint32_t(k) + uint32_t(lane_id()) < hi && mapper_item<true>(int(xx[k]), p[k], key, y, np)) atomicAdd(&hist[key], 1u);
        }
    }
    for (int k = lane_id(); k < 512; k += 64) table[size_t(k) * plan.nseg + seg] = hist[k];
}

// pos3[t] = position of pixel t in s3in/s3out, or 0x80000000 | y when the symbol bypasses the re-mapper
template <bool GEN>
__global__ void __launch_bounds__(256) k_map_scatter(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t lds[4][512];
    const E1Job &J = jobs[blockIdx.y];
    const NearParams np = near_params(GEN ? J.near : 0);
    const auto x = gptr(J.b.img); const auto pxs = gptr(J.b.pxs);
    const auto table = gptr(J.b.table); const auto s3in = gptr(J.b.s3in); const auto pos3 = gptr(J.b.pos3);
    const uint32_t n = J.n; const SegPlan plan = J.pp;
    int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    uint32_t *off = lds[threadIdx.x >> 6];
    for (int k = lane_id(); k < 512; k += 64) off[k] = table[size_t(k) * plan.nseg + seg];
    uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n, lo + plan.seg_len);
    if (lo >= hi) return;
    constexpr int kRows = 8;                                       // eight rows per group, one group ahead (see k_adr_scatter)
    uint32_t cur_p[kRows], nxt_p[kRows], cur_x[kRows], nxt_x[kRows];
    auto fetch = [&](uint32_t base, uint32_t (&pp)[kRows], uint32_t (&xx)[kRows]) {
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const uint32_t t = min(base + 64u * uint32_t(k) + uint32_t(lane_id()), hi - 1);
            pp[k] = pxs[t]; xx[k] = x[t];
        }
    };
    fetch(lo, cur_p, cur_x);
    for (uint32_t gbase = lo; gbase < hi; gbase += 64u * kRows) {
        fetch(gbase + 64u * kRows, nxt_p, nxt_x);
#pragma unroll 1
        for (int k = 0; k < kRows && gbase + 64u * uint32_t(k) < hi; k++) {
            const uint32_t t = gbase + 64u * uint32_t(k) + uint32_t(lane_id());
            uint32_t key = 0; int y = 0;
            const bool in = t < hi;
            const bool valid = mapper_item<GEN>(int(cur_x[k]), cur_p[k], key, y, np) && in;
            if (in && !valid) pos3[t] = 0x80000000u | uint32_t(y);    // y >= 20 codes as itself (NBLIC.c:488)
            const uint64_t same = match_lanes<9>(key, valid);
            if (valid) {
                const uint32_t rank = __popcll(same & lanes_below());
                const uint32_t pos = off[key] + rank;
                s3in[pos] = uint16_t(y);
                pos3[t] = pos;
                if (rank == 0) off[key] += uint32_t(__popcll(same));
            }
        }
#pragma unroll
        for (int k = 0; k < kRows; k++) { cur_p[k] = nxt_p[k]; cur_x[k] = nxt_x[k]; }
    }
}

// ---- S3: re-mapper chains, one lane per (px, sign) (NBLIC.c:470-523) ----------------------
// A step is a dependent LDS round trip (~68 cycles) per table it touches, so the two 20-entry
// permutations (symbol -> rank, rank -> symbol) are kept in REGISTERS, five bits per entry in two
// 64-bit words each; only the 20 counts stay in LDS, laid out [entry][lane] so that the 64
// lanes of a wave hit 64 different banks whatever entry each of them indexes.
struct Perm20 { uint64_t lo, hi; };                                   // entries 0..11 in lo, 12..19 in hi
__device__ __forceinline__ int perm_get(const Perm20 &p, int i) {
    const bool up = i >= 12;
    return int(((up ? p.hi : p.lo) >> (5 * (up ? i - 12 : i))) & 31u);
}
__device__ __forceinline__ void perm_set(Perm20 &p, int i, int v) {
    const bool up = i >= 12;
    const int sh = 5 * (up ? i - 12 : i);
    uint64_t w = up ? p.hi : p.lo;
    w = (w & ~(uint64_t(31) << sh)) | (uint64_t(uint32_t(v)) << sh);
    if (up) p.hi = w; else p.lo = w;
}

constexpr int kPackWords = 13, kPackLanes = 8;     // 64-bit words per lane per group of 64 bins (range_coder.h kGroupWords); lanes of a pack
constexpr int kMapLanes = 16;
// a chain of at least E1Job::long_min records is cut into blocks (k_map_plan .. k_map_check below) and empty here
__device__ __forceinline__ bool map_chain_cut(const E1Job &J, uint32_t len) { return J.long_min >= 0 && len >= uint32_t(max(J.long_min, 1)); }
__global__ void __launch_bounds__(64) k_mapper_chains(const E1Job *__restrict__ jobs) {
    __shared__ int count[kMapSyms][64];
    __shared__ u32x2 stage[64 * kRowWords];
    const E1Job &J = jobs[blockIdx.y];
    const auto s3in = gptr(J.b.s3in); const auto table = gptr(J.b.table);
    const auto total = gptr(J.b.totals) + 1; const auto map_state = gptr(J.b.map_state);
    const auto s3out = gptr(J.b.s3out); const SegPlan plan = J.pp;
    const int lane = int(threadIdx.x);
    // Only kMapLanes lanes of the wave carry a chain: the walk is in lockstep, and the rare swap
    // branch is taken by SOME lane on 73 % of the steps with 64 chains, on 28 % with 16.
    const bool active = lane < kMapLanes;
    const int key = int(blockIdx.x) * kMapLanes + (active ? lane : 0);
    auto st = map_state + size_t(key) * (3 * kMapSyms);
    Perm20 rank_of{0, 0}, sym_at{0, 0};
    for (int k = 0; k < kMapSyms; k++) {
        perm_set(rank_of, k, st[k]); perm_set(sym_at, k, st[kMapSyms + k]); count[k][lane] = st[2 * kMapSyms + k];
    }
    const uint32_t start = active ? table[size_t(key) * plan.nseg] : 0u;
    uint32_t end = !active ? 0u : (key + 1 < 512 ? table[size_t(key + 1) * plan.nseg] : *total);
    if (map_chain_cut(J, end - start)) end = start;                   // k_map_blocks / k_map_check have it (its table entry is written back as it is)
    run_lane_streams(s3in, s3out, start, end, start, stage, [&](uint32_t y, uint32_t) {
        const int zz = perm_get(rank_of, int(y));
        const int up = zz > 0 ? zz - 1 : 0;
        const int c = count[zz][lane] + 1, c_up = count[up][lane];    // both reads in one LDS round trip
        count[zz][lane] = c;
        if (zz > 0 && c_up < c) {                                     // overtake the rank above
            const int other = perm_get(sym_at, up);
            count[zz][lane] = c_up;  count[up][lane] = c;
            perm_set(sym_at, zz, other); perm_set(sym_at, up, int(y));
            perm_set(rank_of, int(y), up); perm_set(rank_of, other, zz);
        }
        return uint32_t(zz);
    }, (J.dbg & 8) ? gptr(J.b.dbg_out) + 64 + blockIdx.x * 4 : nullptr);
    if (active)
        for (int k = 0; k < kMapSyms; k++) {
            st[k] = perm_get(rank_of, k); st[kMapSyms + k] = perm_get(sym_at, k); st[2 * kMapSyms + k] = count[k][lane];
        }
}

// ---- S3 for a chain that holds most of an image: cut into blocks ---------------------------------------------------
// The hit counts never decay and belong to symbols, so the counts BY SYMBOL at any record are the chain's start counts
// plus a histogram prefix -- exact and parallel.  What is not known at a block's first record is the permutation.  So a
// chain of at least E1Job::long_min records is left out of k_mapper_chains (which sees it as empty) and cut into blocks
// of long_block records:
//   k_map_plan    blocks per chain -> mblk_base
//   k_map_hist    a wave per block: its histogram of the 20 symbols
//   k_map_prefix  a wave per chain: counts by symbol at every block's first record, and behind the chain
//   k_map_blocks  a LANE per block: guesses the permutation one block EARLIER -- symbols by descending count, ties in the
//                 order the chain started with (exact for symbols not yet touched) -- refines it over that block's
//                 records, notes what it holds at its own first record and replays its block from there: s3out, the
//                 end permutation.  Blocks 0 and 1 start from the chain's table: exact.
//   k_map_check   a lane per chain, in order: block b stands if what it started with is block b - 1's true end
//                 permutation; otherwise it is replayed here from the true state.  Publishes the chain's end.
// Nothing depends on the guess being right but the time: a tie between symbols that have been hit is decided by which
// of them got there first, which the counts do not say.
__device__ __forceinline__ uint32_t map_block_records(const E1Job &J) { return uint32_t(max(J.long_block, kLongBlockMin)); }
__device__ __forceinline__ void map_chain_range(const E1Job &J, int key, uint32_t &start, uint32_t &end) {
    const auto table = gptr(J.b.table);
    start = table[size_t(key) * J.pp.nseg];
    end = key + 1 < 512 ? table[size_t(key + 1) * J.pp.nseg] : gptr(J.b.totals)[1];
}
__device__ __forceinline__ int map_chain_of_block(NB_GLOBAL const uint32_t *base, uint32_t item) {
    int lo = 0, hi = 512;                                             // invariant: base[lo] <= item < base[hi]
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (base[mid] <= item) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(512) k_map_plan(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t part[8];
    const E1Job &J = jobs[blockIdx.y];
    const int key = int(threadIdx.x);
    uint32_t start, end;
    map_chain_range(J, key, start, end);
    const uint32_t B = map_block_records(J);
    const uint32_t nb = map_chain_cut(J, end - start) ? (end - start + B - 1) / B : 0u;
    const uint32_t incl = wave_scan_incl(nb);
    if (lane_id() == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t pre = incl - nb;
    for (int wv = 0; wv < int(threadIdx.x >> 6); wv++) pre += part[wv];
    gptr(J.b.mblk_base)[key] = pre;
    if (key == 511) gptr(J.b.mblk_base)[512] = pre + nb;
    const uint64_t cut = __ballot(nb != 0u);
    if (lane_id() == 0 && cut) atomicAdd(J.b.totals + kLongS3Split, uint32_t(__popcll(cut)));
}

__global__ void __launch_bounds__(64) k_map_hist(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto base = gptr(J.b.mblk_base); const auto s3in = gptr(J.b.s3in);
    const uint32_t item = blockIdx.x;
    if (item >= base[512]) return;
    const int key = map_chain_of_block(base, item);
    uint32_t c_start, c_end;
    map_chain_range(J, key, c_start, c_end);
    const uint32_t B = map_block_records(J);
    const uint32_t b_start = c_start + (item - base[key]) * B, b_end = min(c_end, b_start + B);
    const int lane = lane_id();
    uint32_t mine = 0;                                                // lane s counts symbol s
    for (uint32_t r = b_start; r < b_end; r += 64u) {
        const uint32_t y = r + uint32_t(lane) < b_end ? uint32_t(s3in[r + uint32_t(lane)]) : 0xFFFFu;
#pragma unroll
        for (int s = 0; s < kMapSyms; s++) {
            const uint64_t m = __ballot(y == uint32_t(s));
            if (lane == s) mine += uint32_t(__popcll(m));
        }
    }
    if (lane < kMapSyms) gptr(J.b.mblk_cnt)[size_t(item) * kMapSyms + lane] = mine;
}

__global__ void __launch_bounds__(64) k_map_prefix(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto base = gptr(J.b.mblk_base); const auto cnt = gptr(J.b.mblk_cnt);
    const int key = int(blockIdx.x), s = lane_id();
    const uint32_t first = base[key], nb = base[key + 1] - first;
    if (nb == 0u || s >= kMapSyms) return;
    const auto st = gptr(J.b.map_state) + size_t(key) * (3 * kMapSyms);
    uint32_t acc = uint32_t(st[2 * kMapSyms + st[s]]);                // the table keeps hits by rank
    for (uint32_t b = 0; b < nb; b++) {
        const size_t at = size_t(first + b) * kMapSyms + s;
        const uint32_t h = cnt[at];
        cnt[at] = acc; acc += h;
    }
    gptr(J.b.mend_cnt)[key * kMapSyms + s] = acc;
}

// one step of a re-mapper chain (NBLIC.c:470-523): the rank of symbol y, then its hit; count[rank][lane] in LDS
__device__ __forceinline__ int mapper_step(Perm20 &rank_of, Perm20 &sym_at, int (*count)[64], int lane, int y) {
    const int zz = perm_get(rank_of, y);
    const int up = zz > 0 ? zz - 1 : 0;
    const int c = count[zz][lane] + 1, c_up = count[up][lane];
    count[zz][lane] = c;
    if (zz > 0 && c_up < c) {
        const int other = perm_get(sym_at, up);
        count[zz][lane] = c_up;  count[up][lane] = c;
        perm_set(sym_at, zz, other); perm_set(sym_at, up, y);
        perm_set(rank_of, y, up); perm_set(rank_of, other, zz);
    }
    return zz;
}

__global__ void __launch_bounds__(64) k_map_blocks(const E1Job *__restrict__ jobs) {
    __shared__ int count[kMapSyms][64];
    __shared__ u32x2 stage[64 * kRowWords];
    const E1Job &J = jobs[blockIdx.y];
    const auto base = gptr(J.b.mblk_base); const auto s3in = gptr(J.b.s3in); const auto s3out = gptr(J.b.s3out);
    const uint32_t n_items = base[512];
    if (blockIdx.x * uint32_t(kMapLanes) >= n_items) return;         // whole wave idle
    const int lane = int(threadIdx.x);
    const uint32_t item = blockIdx.x * uint32_t(kMapLanes) + uint32_t(lane);
    const bool active = lane < kMapLanes && item < n_items;           // kMapLanes blocks per wave: see k_mapper_chains
    const int key = active ? map_chain_of_block(base, item) : 0;
    uint32_t c_start, c_end;
    map_chain_range(J, key, c_start, c_end);
    const uint32_t B = map_block_records(J);
    const uint32_t blk = active ? item - base[key] : 0u;
    const uint32_t b_start = active ? c_start + blk * B : 0u, b_end = active ? min(c_end, b_start + B) : 0u;
    const uint32_t w_start = blk == 0u ? b_start : b_start - B;      // the guess is made a block early
    const uint32_t w_item = blk == 0u ? item : item - 1u;
    const auto st = gptr(J.b.map_state) + size_t(key) * (3 * kMapSyms);
    Perm20 rank_of{0, 0}, sym_at{0, 0};
    {
        uint32_t cs[kMapSyms]; int r0[kMapSyms];
#pragma unroll
        for (int s = 0; s < kMapSyms; s++) { cs[s] = active ? gptr(J.b.mblk_cnt)[size_t(w_item) * kMapSyms + s] : 0u; r0[s] = st[s]; }
#pragma unroll
        for (int s = 0; s < kMapSyms; s++) {
            int r = 0;
            if (blk <= 1u) r = r0[s];                                 // the chain's own table
            else {
#pragma unroll
                for (int t = 0; t < kMapSyms; t++) r += int(cs[t] > cs[s] || (cs[t] == cs[s] && r0[t] < r0[s]));
            }
            perm_set(rank_of, s, r); perm_set(sym_at, r, s);
            count[r][lane] = int(cs[s]);
        }
    }
    Perm20 held = rank_of;                                            // what the lane holds at its block's first record
    run_lane_streams(s3in, s3out, w_start, b_end, b_start, stage, [&](uint32_t y, uint32_t idx) {
        if (idx == b_start) held = rank_of;
        return uint32_t(mapper_step(rank_of, sym_at, count, lane, int(y)));
    });
    if (active) {
        const auto perm = gptr(J.b.mblk_perm) + size_t(item) * 4;
        perm[0] = held.lo; perm[1] = held.hi; perm[2] = rank_of.lo; perm[3] = rank_of.hi;
    }
}

__global__ void __launch_bounds__(64) k_map_check(const E1Job *__restrict__ jobs) {
    __shared__ int count[kMapSyms][64];
    const E1Job &J = jobs[blockIdx.y];
    const auto base = gptr(J.b.mblk_base); const auto s3in = gptr(J.b.s3in); const auto s3out = gptr(J.b.s3out);
    const auto perm = gptr(J.b.mblk_perm); const auto cnt = gptr(J.b.mblk_cnt);
    const int lane = int(threadIdx.x);
    const int key = int(blockIdx.x) * kMapLanes + (lane < kMapLanes ? lane : 0);
    const uint32_t first = base[key], nb = lane < kMapLanes ? base[key + 1] - first : 0u;
    if (nb == 0u) return;
    uint32_t c_start, c_end;
    map_chain_range(J, key, c_start, c_end);
    const uint32_t B = map_block_records(J);
    Perm20 rank_of{perm[size_t(first) * 4 + 2], perm[size_t(first) * 4 + 3]};          // block 0 started from the table: its end is true
    uint32_t accepted = 0, missed = 0;
    for (uint32_t b = 1; b < nb; b++) {
        const size_t it = size_t(first + b);
        if (perm[it * 4] == rank_of.lo && perm[it * 4 + 1] == rank_of.hi) {
            accepted++;
            rank_of = Perm20{perm[it * 4 + 2], perm[it * 4 + 3]};
            continue;
        }
        missed++;
        Perm20 sym_at{0, 0};
        for (int s = 0; s < kMapSyms; s++) {
            const int r = perm_get(rank_of, s);
            perm_set(sym_at, r, s); count[r][lane] = int(cnt[it * kMapSyms + s]);
        }
        const uint32_t lo = c_start + b * B, hi = min(c_end, lo + B);
        for (uint32_t r = lo; r < hi; r += 8u) {                      // eight loads ahead of the eight dependent steps
            uint32_t y[8];
#pragma unroll
            for (int k = 0; k < 8; k++) y[k] = s3in[min(r + uint32_t(k), hi - 1u)];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (r + uint32_t(k) < hi) s3out[r + uint32_t(k)] = uint16_t(mapper_step(rank_of, sym_at, count, lane, int(y[k])));
        }
    }
    const auto st = gptr(J.b.map_state) + size_t(key) * (3 * kMapSyms);
    for (int s = 0; s < kMapSyms; s++) {
        const int r = perm_get(rank_of, s);
        st[s] = r; st[kMapSyms + r] = s; st[2 * kMapSyms + r] = int(gptr(J.b.mend_cnt)[key * kMapSyms + s]);
    }
    if (accepted) atomicAdd(J.b.totals + kLongS3Accepted, accepted);
    if (missed) atomicAdd(J.b.totals + kLongS3Missed, missed);
}

// ---- S4: binarisation (NBLIC.c:640-679); path depends on (qu,qv,qw,z) only ----------------
// GEN = the job's k_step (near-lossless modes), divisions from its level_shift_table
template <bool GEN, class Step>
__device__ __forceinline__ int walk_job(const E1Job &J, int qu, int qv, int z, Step step) {
    return GEN ? walk_symbol_t(J.k_step, J.ktab, qu, qv, z, step) : walk_symbol(kMinKStep, qu, qv, z, step);
}

template <bool GEN>
__global__ void __launch_bounds__(256) k_count_bins(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto rec1 = gptr(J.b.rec1); const auto s3out = gptr(J.b.s3out);
    const auto pos3 = gptr(J.b.pos3); const auto z = gptr(J.b.z); const auto cnt = gptr(J.b.cnt);
    uint32_t t = xcd_block() * 256u + threadIdx.x;
    if (t >= J.n) return;
    Level L = s1_level(rec1[t]);
    uint32_t p = pos3[t];
    int zz = (p >> 31) ? int(p & 0xFF) : int(s3out[p]);           // back to raster order
    z[t] = uint8_t(zz);
    int c = 0;
    walk_job<GEN>(J, L.qu, L.qv, zz, [&](int, int, int, int bin) { c++; return bin; });
    cnt[t] = uint8_t(c);
}

template <bool GEN>
__global__ void __launch_bounds__(256) k_emit_bins(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto rec1 = gptr(J.b.rec1); const auto z = gptr(J.b.z);
    const auto ev_off = gptr(J.b.ev_off); const auto events = gptr(J.b.events);
    uint32_t t = xcd_block() * 256u + threadIdx.x;
    if (t >= J.n) return;
    Level L = s1_level(rec1[t]);
    auto out = events + ev_off[t];
    walk_job<GEN>(J, L.qu, L.qv, int(z[t]), [&](int qu, int qv, int node, int bin) {
        *out++ = pack_event(qu, qv, node, L.qw, bin);
        return bin;
    });
}

// ---- partition 3: counter touches (4096 keys = parity | tree/2 | node) --------------------
// Adjacent levels differ by one, so of an event's two trees exactly one is even and one is
// odd: per parity an event contributes AT MOST one touch, which keeps the ranking a plain
// one-key match.  An event whose two trees coincide touches that one counter twice
// (weights 32-qw then qw, NBLIC.c:635-636) and is carried as a single "double" item.
// Touch payload (u16):  w1[0:6) | w2[6:12) | bin[12] | double[13]
struct Touch { bool valid; uint32_t key; uint32_t payload; int slot; };

__device__ __forceinline__ Touch touch_of(uint32_t e, int parity) {
    // branch-free (selects): the scatter walk is bound by instruction issue, and as nested ifs this compiled to ten branches
    const int qu = ev_qu(e), qv = ev_qv(e), node = ev_node(e), qw = ev_qw(e), bin = ev_bin(e);
    const bool same = qu == qv;                  // one counter touched twice: weights 32-qw then qw, a "double" item
    const bool mine = (qu & 1) == parity;        // tree u is the one of this parity (else tree v, unless the trees coincide)
    Touch t;
    t.valid = mine || (!same && qw != 0);        // a weight-0 touch changes no state and its P is multiplied by 0
    const int tree = mine ? qu : qv;
    const int w1 = mine ? kWeightOne - qw : qw;
    t.slot = mine ? 0 : 1;
    t.key = uint32_t(parity) * 2048u + uint32_t(tree >> 1) * 256u + uint32_t(node);
    t.payload = uint32_t(w1) | (same ? uint32_t(qw) << 6 | 1u << 13 : 0u) | (uint32_t(bin) << 12);
    return t;
}

// (Measured and rejected in round 2: counting inside k_emit_bins while the event is in a register -- a workgroup-wide
// LDS histogram handed to the table with one global atomic per non-empty key after sixteen 256-pixel tiles.  It saves
// this kernel's read of all events (17.8 B/px) and a launch, the two kernels' time under load drops from 13.8 to
// 8.7 ms per launch -- and the pipeline runs 2.5 % SLOWER (5.42 against 5.56 Gpx/s, alternating runs on one box):
// the device-scope atomics land in everybody else's way.  Flushing per tile was worse still: 19.6 ms.)
__global__ void __launch_bounds__(256) k_touch_count(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t lds[4][4096];
    const E1Job &J = jobs[blockIdx.y];
    const auto events = gptr(J.b.events); const auto table = gptr(J.b.table);
    const uint32_t n_ev = J.n_ev; const SegPlan plan = J.pe;
    int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    // the scan that follows raises this flag for an image with too many touches for 28-bit positions (k_touch_scatter)
    if (seg == 0 && lane_id() == 0) gptr(J.b.totals)[kWideTouchFlag] = (J.dbg & 256) ? 1u : 0u;   // (NBLIC_AMD_DBG & 256: plain 32-bit positions for every image -- tests, A/B runs)
    uint32_t *hist = lds[threadIdx.x >> 6];
    lds_fill<4096>(hist, 0);
    uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n_ev, lo + plan.seg_len);
    // eight rows of loads in flight per wave (clamped addresses, no branch around a load): the
    // histogram updates are LDS atomics, so nothing but the load latency paces this loop
    for (uint32_t base = lo; base < hi; base += 512) {
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) e[k] = events[min(base + 64u * uint32_t(k) + uint32_t(lane_id()), hi - 1)];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (base + 64u * uint32_t(k) + uint32_t(lane_id()) < hi) {
                Touch a = touch_of(e[k], 0), b = touch_of(e[k], 1);
                if (a.valid) atomicAdd(&hist[a.key], 1u);
                if (b.valid) atomicAdd(&hist[b.key], 1u);
            }
        }
    }
    for (int k = lane_id(); k < 4096; k += 64) table[size_t(k) * plan.nseg + seg] = hist[k];
}

// One wave per (segment, parity): places its segment's touches of that parity in the chains and
// records where, posP[parity][r] = position of event r's touch in tin[] / tout[] (or kNoTouch).
//
// Written naively this kernel turns every touch into a scattered 2-byte store, and with ~2000
// waves each appending to a few hundred chains far more 64-byte lines are open at once than L2 and
// the MALL hold: measured 7x write amplification on tin[].  But 99 % of the touches fall in at most
// a few hundred of the 4096 chains, and the partition table already says how many touches each
// chain gets from this segment.  So the wave gives its kStageSlots busiest chains an LDS ring each
// and writes those chains in whole aligned 64-byte lines:
//   invariant per staged chain:  tin[.. flushed) is in HBM, [flushed, off) sits in the ring,
//                                flushed >= off & ~31, so a group of <= 32 new touches always fits
//                                (flushed lives in a register: lane s holds it for slot s);
//   a group of more than 32 (flat images) goes straight to HBM after the ring has been drained.
constexpr int kStageSlots = 64, kStageRing = 64;
constexpr uint32_t kNoTouch = 0xFFFFFFFFu;
// narrow position words: pos (28 bits, all ones = no touch) | extra << 28, extra = qw[0:4) in the even-tree word and
// qw[4:6) | bin << 2 | (qu odd) << 3 in the odd-tree word
constexpr int kPosBits = 28;
constexpr uint32_t kPosMask = (1u << kPosBits) - 1u;
__device__ __forceinline__ uint32_t pack_pos(uint32_t pos, uint32_t e, int parity) {
    const uint32_t qw = uint32_t(ev_qw(e));
    const uint32_t extra = parity == 0 ? (qw & 15u) : ((qw >> 4) | (uint32_t(ev_bin(e)) << 2) | (uint32_t(ev_qu(e) & 1) << 3));
    return (pos & kPosMask) | (extra << kPosBits);
}
struct alignas(16) TouchLds {
    uint32_t off[2048];                      // next position of every chain of this parity
    uint16_t ring[kStageSlots][kStageRing];
    uint16_t slot_key[kStageSlots];
    uint8_t slot[2048];                      // chain -> staging slot + 1, 0 = not staged
};

// The whole wave copies ring entries [a, b) of one staged chain to tin[]: a lane per touch, so the
// store is one coalesced run whatever the alignment of a.  (b - a <= 63.)
__device__ __forceinline__ void flush_range(TouchLds &L, NB_GLOBAL uint16_t *tin, int sl, uint32_t a, uint32_t b) {
    const uint32_t e = a + uint32_t(lane_id());
    if (e < b) tin[e] = L.ring[sl][e & (kStageRing - 1)];
}

template <bool STAMP>      // cycle stamps per phase of the walk (E1Job::dbg & 8): compiled out of the production kernel
__global__ void __launch_bounds__(256) k_touch_scatter(const E1Job *__restrict__ jobs) {
    __shared__ TouchLds lds[4];
    const E1Job &J = jobs[blockIdx.y];
    const auto events = gptr(J.b.events); const auto table = gptr(J.b.table);
    const auto tin = gptr(J.b.tin);
    const uint32_t n_ev = J.n_ev; const SegPlan plan = J.pe;
    const int parity = int(blockIdx.z);
    // a position needs 28 bits (kPosBits) for every frame the reference accepts at ordinary bin counts; the four
    // spare bits of the two words carry what k_mix would otherwise re-read the event for (see there).  An image
    // with 2^28 - 1 touches or more sets the flag in the scan and keeps plain 32-bit positions.
    const bool wide = gptr(J.b.totals)[kWideTouchFlag] != 0u;
    const auto posP = (NB_GLOBAL uint32_t *)gptr(J.b.tpos) + size_t(parity) * ((size_t(n_ev) + 63) & ~size_t(63));
    const int seg = int(xcd_block()) * 4 + int(threadIdx.x >> 6);
    if (seg >= plan.nseg) return;
    TouchLds &L = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    constexpr bool stamp = STAMP;
    unsigned long long t_begin = __builtin_amdgcn_s_memtime(), t_match = 0, t_place = 0, t_close = 0, t0 = 0;
    // chain starts and this segment's touch count per chain (32 chains per lane)
    uint32_t cnt[32], most = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const int key = lane + 64 * i, gk = parity * 2048 + key;
        const uint32_t start = table[size_t(gk) * plan.nseg + seg];
        const uint32_t next = seg + 1 < plan.nseg ? table[size_t(gk) * plan.nseg + seg + 1]
                            : (gk + 1 < 4096 ? table[size_t(gk + 1) * plan.nseg] : gptr(J.b.totals)[3]);
        L.off[key] = start;
        cnt[i] = next - start;
        most = max(most, cnt[i]);
    }
    // the smallest threshold that leaves at most kStageSlots chains (binary search, wave-uniform)
    most = wave_max(most);
    uint32_t th_lo = 16, th_hi = max(most + 1, 17u);         // a chain with < 16 touches never fills a line
    while (th_lo < th_hi) {
        const uint32_t mid = (th_lo + th_hi) >> 1;
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < 32; i++) mine += uint32_t(cnt[i] >= mid);
        if (read_lane(wave_scan_incl_dpp(mine), 63) <= uint32_t(kStageSlots)) th_hi = mid; else th_lo = mid + 1;
    }
    {
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < 32; i++) mine += uint32_t(cnt[i] >= th_lo);
        uint32_t id = wave_scan_incl_dpp(mine) - mine;
        L.slot_key[lane] = 0xFFFFu;                           // lane = slot; unused slots stay marked
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int key = lane + 64 * i;
            const bool staged = cnt[i] >= th_lo && id < uint32_t(kStageSlots);
            L.slot[key] = staged ? uint8_t(id + 1) : uint8_t(0);
            if (staged) { L.slot_key[id] = uint16_t(key); id++; }
        }
    }
    const uint32_t my_key = L.slot_key[lane];                 // lane s looks after staging slot s
    uint32_t my_flushed = my_key != 0xFFFFu ? L.off[my_key] : 0u;
    const uint32_t lo = uint32_t(seg) * plan.seg_len, hi = min(n_ev, lo + plan.seg_len);
    auto place = [&](const uint32_t base, const uint32_t e) {
        const uint32_t r = base + lane;
        const Touch t = touch_of(e, parity);
        const bool valid = r < hi && t.valid;
        const uint32_t key = t.key & 2047u;
        if (stamp) t0 = __builtin_amdgcn_s_memtime();
        // asked for before the ballots, consumed after them.  Issued by hand: left to the compiler the two reads are
        // sunk into the `valid` branch behind the match, and their latency is paid instead of hidden.  (LDS operations
        // return in order, so the compiler's own lgkmcnt waits only become more conservative with these in flight.)
        uint32_t chain_off, slot_raw;
        asm volatile("ds_read_b32 %0, %2\n\tds_read_u8 %1, %3"
                     : "=&v"(chain_off), "=&v"(slot_raw) : "v"(lds_address(&L.off[key])), "v"(lds_address(&L.slot[key])) : "memory");
        __builtin_amdgcn_sched_barrier(0);                      // the match stays between the reads and the wait
        const uint64_t same = match_lanes<11>(key, valid);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(chain_off), "+v"(slot_raw) : : "memory");
        const int chain_slot = int(slot_raw) - 1;
        if (stamp) { unsigned long long t1 = __builtin_amdgcn_s_memtime(); t_match += t1 - t0; t0 = t1; }
        uint32_t pos = kNoTouch;
        int slv = -1;
        if (valid) {
            const uint32_t rank = __popcll(same & lanes_below());
            slv = chain_slot;
            pos = chain_off + rank;
            if (slv >= 0 && __popcll(same) <= 32) L.ring[slv][pos & (kStageRing - 1)] = uint16_t(t.payload);
            else tin[pos] = uint16_t(t.payload);
        }
        if (stamp) { unsigned long long t1 = __builtin_amdgcn_s_memtime(); t_place += t1 - t0; t0 = t1; }
        // one lane per chain closes the step; completed lines are then written by the whole wave.
        // flushed lies in old's own 32-touch line (invariant), so whether a line was completed can be
        // read off the positions alone.
        const uint32_t group = uint32_t(__popcll(same));
        const bool leader = valid && (same & lanes_below()) == 0;
        const uint32_t old = pos, now = old + group;            // (leader: rank 0, so pos is the chain's old offset)
        if (leader) L.off[key] = now;
        const int sl = leader ? slv : -1;
        uint64_t todo = __ballot(sl >= 0 && (group > 32 || (now >> 5) > (old >> 5)));
        while (todo) {                                          // wave-uniform; ~1.5 lines per row
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int s_sl = __builtin_amdgcn_readlane(sl, src);
            const uint32_t s_old = read_lane(old, src), s_now = read_lane(now, src);
            const bool big = read_lane(group, src) > 32;        // its touches went straight to HBM: drain what was staged before
            const uint32_t upto = big ? s_old : (s_now & ~31u);
            flush_range(L, tin, s_sl, read_lane(my_flushed, s_sl), upto);
            if (lane == s_sl) my_flushed = big ? s_now : upto;
        }
        if (stamp) { unsigned long long t1 = __builtin_amdgcn_s_memtime(); t_close += t1 - t0; }
        if (r < hi) posP[r] = wide ? pos : pack_pos(pos, e, parity);
    };
    const unsigned long long t_setup = __builtin_amdgcn_s_memtime() - t_begin;
    // The walk is serial in the chain offsets, so the event loads must not be.  On this ISA loads
    // and stores share one in-flight counter and complete out of order with respect to each
    // other, so consuming ANY load while stores are in flight drains them all (~1 us): the events
    // are therefore fetched sixteen 64-event rows at a time, one group ahead (clamped, never
    // branched-over addresses), and the drain is paid once per 1024 events instead of per row.
    if (lo < hi) {
        constexpr int kRows = 16;
        uint32_t cur[kRows], nxt[kRows];
        auto fetch = [&](uint32_t base, uint32_t (&rows)[kRows]) {
#pragma unroll
            for (int k = 0; k < kRows; k++) rows[k] = events[min(base + 64u * uint32_t(k) + uint32_t(lane), hi - 1)];
        };
        fetch(lo, cur);
        for (uint32_t base = lo; base < hi; base += 64u * kRows) {
            fetch(base + 64u * kRows, nxt);
#pragma unroll 1
            for (int k = 0; k < kRows && base + 64u * uint32_t(k) < hi; k++) place(base + 64u * uint32_t(k), cur[k]);
#pragma unroll
            for (int k = 0; k < kRows; k++) cur[k] = nxt[k];
        }
    }
    for (int sl = 0; sl < kStageSlots; sl++) {                  // what is left in the rings
        const uint32_t key = read_lane(my_key, sl);
        if (key != 0xFFFFu) flush_range(L, tin, sl, read_lane(my_flushed, sl), L.off[key]);
    }
    if (stamp && lane == 0 && (seg & 63) == 0) {
        const auto d = gptr(J.b.dbg_out) + 2048 + (parity * 4 + (seg >> 6)) * 8;
        d[0] = __builtin_amdgcn_s_memtime() - t_begin; d[1] = t_setup; d[2] = t_match; d[3] = t_place; d[4] = t_close; d[5] = hi - lo;
    }
}

// ---- S5: counter chains (NBLIC.c:589-637) --------------------------------------------------
// Between two halvings a counter is a pure running sum, and a halving needs the sum to climb
// from <= 4129 past 8192 in steps <= 32, i.e. >= 127 touches.  The work is split in two:
//
//   k_counter_epochs  the SERIAL part, one wave per counter chain.  Walks the chain in aligned
//                     512-touch windows (one 16-byte load per lane, three windows in flight),
//                     prefix-sums the weights on the DPP crossbar and resolves only the halvings:
//                     per window it records the state at entry and, for each halving inside, where
//                     the next epoch starts and from which state.  No division, no per-touch output.
//   k_counter_probs   the PARALLEL part, one wave per window of any chain.  Rebuilds the prefix,
//                     picks each touch's epoch from the record and writes P(bin==1) before the touch.
constexpr int kTpl = 8;                  // touches per lane per window
constexpr uint32_t kWin = 64u * kTpl;    // touches per window
constexpr int kMaxHalv = 5;              // halvings that fit in one window (>= 127 touches apart)

struct WinRec {                          // 24 words
    uint32_t first, start, end;          // window's first touch slot (multiple of 8); chain's [start, end)
    int vb_s, vb_1, n_halv;              // virtual base at entry: state before touch j = vb + exclusive prefix(j)
    struct { int from, vb_s, vb_1; } epoch[kMaxHalv + 1];   // touches >= from use this base instead
};
static_assert(sizeof(WinRec) == 96, "WinRec is read as six 16-byte words");

// Unpacks one lane's eight touches and turns them into window-relative INCLUSIVE prefixes of
// total weight (tin) and of weight that went to bin 1 (oin); lane_t / lane_o are the exclusive
// prefixes at the lane's first touch.
__device__ __forceinline__ void window_prefix(const u32x4 w, uint32_t window, uint32_t start, uint32_t end, int lane,
                                              uint32_t (&pay)[kTpl], int (&tin)[kTpl], int (&oin)[kTpl], int &lane_t, int &lane_o) {
    const uint32_t p[kTpl] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16, w.z & 0xFFFFu, w.z >> 16, w.w & 0xFFFFu, w.w >> 16};
    int tot[kTpl];
#pragma unroll
    for (int k = 0; k < kTpl; k++) { pay[k] = p[k]; tot[k] = int(p[k] & 63) + int((p[k] >> 6) & 63); }
    if (window < start || window + kWin > end) {                       // chain edge (wave-uniform): mask foreign slots
        const uint32_t first = window + uint32_t(lane) * kTpl;
#pragma unroll
        for (int k = 0; k < kTpl; k++) if (first + k < start || first + k >= end) tot[k] = 0;
    }
    int lt = 0, lo = 0;
#pragma unroll
    for (int k = 0; k < kTpl; k++) {
        lt += tot[k]; lo += ((p[k] >> 12) & 1) ? tot[k] : 0;
        tin[k] = lt; oin[k] = lo;
    }
    const uint32_t incl = wave_scan_incl_dpp((uint32_t(lt) << 16) | uint32_t(lo));
    lane_t = int(incl >> 16) - lt; lane_o = int(incl & 0xFFFF) - lo;
#pragma unroll
    for (int k = 0; k < kTpl; k++) { tin[k] += lane_t; oin[k] += lane_o; }
}

// windows per chain -> exclusive scan -> win_base[0..4096]; win_base[4097..] = the chain keys
// ordered longest first (by power-of-two length class), so the kernel's critical path -- the
// hottest chain -- starts in the first round of workgroups.  One 1024-thread block per job.
__global__ void __launch_bounds__(1024) k_plan_windows(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t part[16];
    __shared__ uint32_t klass[32];
    const E1Job &J = jobs[blockIdx.y];
    const auto table = gptr(J.b.table); const auto win_base = gptr(J.b.win_base);
    const uint32_t total = gptr(J.b.totals)[3];
    const int nseg = J.pe.nseg;
    if (threadIdx.x < 32) klass[threadIdx.x] = 0;
    __syncthreads();
    uint32_t cnt[4], sum = 0; int cls[4];
    for (int k = 0; k < 4; k++) {
        int key = int(threadIdx.x) * 4 + k;
        uint32_t start = table[size_t(key) * nseg];
        uint32_t end = key + 1 < 4096 ? table[size_t(key + 1) * nseg] : total;
        cnt[k] = end > start ? (end - (start & ~7u) + kWin - 1) / kWin : 0u;
        sum += cnt[k];
        cls[k] = end > start ? __clz(int(end - start)) : 31;        // 0 = longest
        atomicAdd(&klass[cls[k]], 1u);
    }
    uint32_t incl = wave_scan_incl(sum);
    if (lane_id() == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int c = 0; c < 32; c++) { uint32_t v = klass[c]; klass[c] = run; run += v; }
    }
    uint32_t pre = incl - sum;
    for (int wv = 0; wv < int(threadIdx.x >> 6); wv++) pre += part[wv];
    for (int k = 0; k < 4; k++) { win_base[threadIdx.x * 4 + k] = pre; pre += cnt[k]; }
    if (threadIdx.x == 1023) win_base[4096] = pre;
    __syncthreads();
    for (int k = 0; k < 4; k++) win_base[4097 + atomicAdd(&klass[cls[k]], 1u)] = threadIdx.x * 4 + k;
}

// One lone wave issues at most one instruction every four cycles and pays extra for every
// VALU -> SALU hand-off, so this kernel is written for INSTRUCTION COUNT:
//   * a touch's weights sum to <= 32, so a window's prefix of (total weight, weight to bin 1)
//     fits one packed word (total << 16 | ones); one add / one DPP scan serves both;
//   * the record is assembled in three registers with v_writelane (lane l = words 3l..3l+2) and
//     stored once per window;
//   * a touch that crosses the limit halves the counter exactly once (the sum drops to ~4100 and
//     the second weight is <= 32), which removes the second conditional halving from the scalar
//     arithmetic;
//   * the crossing touch's prefix and payload are fetched with a uniform register index.
__global__ void __launch_bounds__(64) k_counter_epochs(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto tin_g = gptr(J.b.tin); const auto table = gptr(J.b.table);
    const auto cnt_state = (NB_GLOBAL i32x2 *)gptr(J.b.cnt_state);
    const auto recs = gptr(J.b.win_recs);
    const SegPlan plan = J.pe;
    const int key = int(gptr(J.b.win_base)[4097 + blockIdx.x]);
    const int lane = int(threadIdx.x);
    const uint32_t start = table[size_t(key) * plan.nseg];
    const uint32_t end = key + 1 < 4096 ? table[size_t(key + 1) * plan.nseg] : gptr(J.b.totals)[3];
    if (start >= end) return;
    const auto in_w = (NB_GLOBAL const u32x4 *)tin_g;
    uint32_t rec_i = gptr(J.b.win_base)[key];
    i32x2 st = cnt_state[key];
    int base_s = st.x + st.y, base_1 = st.y;                         // wave-uniform running state
    const int dbg = J.dbg;
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
    const uint32_t first_window = start & ~7u;
    int r0 = 0, r1 = int(start), r2 = int(end);                      // record words; lane 0 keeps (window, start, end)
    unsigned n_halv_all = 0;
    // Four windows in flight: the chain is serial, so its memory latency must be covered by
    // depth.  The loop is unrolled by four over NAMED buffers -- rotating one register set at the
    // back edge makes the compiler wait for the load it has only just issued.
    auto process = [&](const u32x4 w, const uint32_t window) {
        // v[0..8]: lane-local packed prefix BEFORE touch k (v[8] = lane total); v[9..12]: the raw payload words
        // (sixteen entries: the indexed read is modelled as touching a whole 16-register tuple, and a
        // 13-entry array would let that tuple overlap the registers of a window still being loaded)
        uint32_t v[16];
        v[13] = v[14] = v[15] = 0;
        v[9] = w.x; v[10] = w.y; v[11] = w.z; v[12] = w.w;
        uint32_t pt[kTpl];
#pragma unroll
        for (int k = 0; k < kTpl; k++) {
            const uint32_t p = v[9 + (k >> 1)] >> (16 * (k & 1));
            const uint32_t tot = (p & 63u) + ((p >> 6) & 63u);
            pt[k] = (tot << 16) | (((p >> 12) & 1u) ? tot : 0u);
        }
        if (window < start || window + kWin > end) {                 // chain edge (wave-uniform): mask foreign slots
            const uint32_t first = window + uint32_t(lane) * kTpl;
#pragma unroll
            for (int k = 0; k < kTpl; k++) if (first + k < start || first + k >= end) pt[k] = 0;
        }
        v[0] = 0;
#pragma unroll
        for (int k = 0; k < kTpl; k++) v[k + 1] = v[k] + pt[k];
        const uint32_t incl = wave_scan_incl_dpp(v[kTpl]);
        const uint32_t lane_ex = incl - v[kTpl];
        int vb_s = base_s, vb_1 = base_1;                            // uniform virtual base of the current epoch
        int n_halv = 0;
        r0 = write_lane<0>(int(window), r0);
        r0 = write_lane<1>(vb_s, r0);
        r1 = write_lane<1>(vb_1, r1);
#pragma unroll 1
        for (;;) {
            // Prefixes are non-decreasing, so "first touch that lifts the sum over the limit" is a
            // rank query: lanes wholly below the threshold form a prefix of the wave.  The packed
            // compare works on the high half; the low half of the threshold is all ones.
            const uint32_t thr = (uint32_t(kCountLimit - vb_s) << 16) | 0xFFFFu;
            const int H = __popcll(__ballot(incl <= thr));
            if (H >= 64) break;
            const uint32_t d = thr - lane_ex;                        // meaningful in lane H, where lane_ex <= thr
            int below = 0;
#pragma unroll
            for (int k = 1; k <= kTpl; k++) below += int(v[k] <= d);
            const int hk = __builtin_amdgcn_readlane(below, H);      // < 8 in lane H
            const uint32_t ex = read_lane(lane_ex + v[hk], H);
            const uint32_t hx = read_lane(v[9 + (hk >> 1)], H) >> (16 * (hk & 1));
            const int t_ex = int(ex >> 16), o_ex = int(ex & 0xFFFFu);
            const int a1 = int(hx & 63u), hw = a1 + int((hx >> 6) & 63u);
            const int one = -int((hx >> 12) & 1u);                   // all ones when the bin is 1
            // counter_add for both weights (NBLIC.c:606-618): exactly one of them halves
            const int s0 = vb_s + t_ex;
            int c1 = vb_1 + o_ex, c0 = s0 - c1;
            const int before = (s0 + a1 > kCountLimit) ? a1 : hw, after = hw - before;
            c1 += before & one; c0 += before & ~one;
            c1 = (c1 + 1) >> 1; c0 = (c0 + 1) >> 1;
            c1 += after & one; c0 += after & ~one;
            vb_s = c0 + c1 - (t_ex + hw);                            // new base = state after it minus its inclusive prefix
            vb_1 = c1 - (o_ex + (hw & one));
            const int slot = 2 + (n_halv < kMaxHalv ? n_halv : kMaxHalv);
            write_lane3(slot, H * kTpl + hk + 1, vb_s, vb_1, r0, r1, r2);
            n_halv++;
        }
        r2 = write_lane<1>(n_halv, r2);
        if (lane < 8) {
            const auto rec = recs + size_t(rec_i) * 24 + lane * 3;
            rec[0] = uint32_t(r0); rec[1] = uint32_t(r1); rec[2] = uint32_t(r2);
        }
        const uint32_t whole = read_lane(incl, 63);
        base_s = vb_s + int(whole >> 16);
        base_1 = vb_1 + int(whole & 0xFFFFu);
        n_halv_all += unsigned(n_halv);
        rec_i++;
    };
    // The prefetch is UNCONDITIONAL (past the chain it re-reads the last window): a load inside a
    // branch makes the number of requests in flight unknown to the compiler, which then waits for
    // all of them -- including the one it has only just issued -- before every window.
    const uint32_t last_window = first_window + ((end - 1 - first_window) / kWin) * kWin;
    auto fetch = [&](uint32_t window) { return in_w[(min(window, last_window) >> 3) + lane]; };
    u32x4 b0 = fetch(first_window), b1 = fetch(first_window + kWin), b2 = fetch(first_window + 2 * kWin), b3 = fetch(first_window + 3 * kWin);
    for (uint32_t window = first_window; window < end; window += 4 * kWin) {
        process(b0, window);
        b0 = fetch(window + 4 * kWin);
        if (window + kWin < end) process(b1, window + kWin);
        b1 = fetch(window + 5 * kWin);
        if (window + 2 * kWin < end) process(b2, window + 2 * kWin);
        b2 = fetch(window + 6 * kWin);
        if (window + 3 * kWin < end) process(b3, window + 3 * kWin);
        b3 = fetch(window + 7 * kWin);
    }
    if (lane == 0) cnt_state[key] = i32x2{base_s - base_1, base_1};
    if ((dbg & 8) && lane == 0 && end - start > 100000u) {
        const auto d = gptr(J.b.dbg_out) + 256 + (key & 255) * 4;
        d[0] = __builtin_amdgcn_s_memtime() - t_begin; d[1] = end - start; d[2] = rec_i - gptr(J.b.win_base)[key]; d[3] = n_halv_all;
    }
}

// one wave per recorded window; grid.x is an upper bound, surplus waves leave at once
__global__ void __launch_bounds__(256) k_counter_probs(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= gptr(J.b.win_base)[4096]) return;
    const int lane = lane_id();
    const auto r = (NB_GLOBAL const u32x4 *)gptr(J.b.win_recs) + size_t(g) * 6;
    const u32x4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5];
    const uint32_t window = r0.x, start = r0.y, end = r0.z;
    const int n_halv = min(int(r1.y), kMaxHalv + 1);
    const int from[kMaxHalv + 1] = {int(r1.z), int(r2.y), int(r3.x), int(r3.w), int(r4.z), int(r5.y)};
    const int hs[kMaxHalv + 1] = {int(r1.w), int(r2.z), int(r3.y), int(r4.x), int(r4.w), int(r5.z)};
    const int h1[kMaxHalv + 1] = {int(r2.x), int(r2.w), int(r3.z), int(r4.y), int(r5.x), int(r5.w)};
    const auto tin_g = gptr(J.b.tin); const auto tout = gptr(J.b.tout);
    const uint32_t first = window + uint32_t(lane) * kTpl;
    const u32x4 w = ((NB_GLOBAL const u32x4 *)tin_g)[first >> 3];
    uint32_t pay[kTpl]; int tin[kTpl], oin[kTpl], lane_t, lane_o;
    window_prefix(w, window, start, end, lane, pay, tin, oin, lane_t, lane_o);
    uint32_t p[kTpl];
#pragma unroll
    for (int k = 0; k < kTpl; k++) {
        const int j = lane * kTpl + k;
        int vs = int(r0.w), v1 = int(r1.x);
#pragma unroll
        for (int h = 0; h <= kMaxHalv; h++) if (h < n_halv && j >= from[h]) { vs = hs[h]; v1 = h1[h]; }
        const int t_ex = k ? tin[k - 1] : lane_t, o_ex = k ? oin[k - 1] : lane_o;
        p[k] = prob_one(v1 + o_ex, vs + t_ex);
    }
    if (first >= start && first + kTpl <= end) {
        ((NB_GLOBAL u32x4 *)tout)[first >> 3] = u32x4{p[0] | (p[1] << 16), p[2] | (p[3] << 16), p[4] | (p[5] << 16), p[6] | (p[7] << 16)};
    } else {
#pragma unroll
        for (int k = 0; k < kTpl; k++) if (first + k >= start && first + k < end) tout[first + k] = uint16_t(p[k]);
    }
}

// ---- mix the two trees' probabilities and pack for the host coder (NBLIC.c:629-633) -------
// k_touch_scatter files an event's touch positions by tree PARITY; tree u is the one with qu's parity, and an event
// without a second touch (both trees equal, or weight 0) mixes its one P with itself.  The two position words also
// carry qw, the bin and qu's parity in their top four bits (pack_pos), so the event itself is not read again
// (4 of 12 bytes per event) -- unless the image has too many touches for 28-bit positions (flag set by the scan).
// P(bin == 1) | bin << 12 of bin r of job J (0 beyond the image's last bin)
__device__ __forceinline__ uint32_t mixed_code(const E1Job &J, uint32_t r, bool wide) {
    if (r >= J.n_ev) return 0u;
    const auto tout = gptr(J.b.tout);
    const auto pos0 = (NB_GLOBAL const uint32_t *)gptr(J.b.tpos);
    const auto pos1 = pos0 + ((size_t(J.n_ev) + 63) & ~size_t(63));
    uint32_t p0 = pos0[r], p1 = pos1[r];
    int qw, bin; bool odd;
    if (wide) {
        const uint32_t e = gptr(J.b.events)[r];
        qw = ev_qw(e); bin = ev_bin(e); odd = (ev_qu(e) & 1) != 0;
    } else {
        qw = int((p0 >> kPosBits) | (((p1 >> kPosBits) & 3u) << 4)); bin = int((p1 >> (kPosBits + 2)) & 1u); odd = (p1 >> 31) != 0u;
        p0 &= kPosMask; p1 &= kPosMask;
        if (p0 == kPosMask) p0 = kNoTouch;
        if (p1 == kPosMask) p1 = kNoTouch;
    }
    const uint32_t at_u = odd ? p1 : p0, other = odd ? p0 : p1, at_v = other == kNoTouch ? at_u : other;
    const int pu = tout[at_u], pv = tout[at_v];
    return uint32_t(mix_prob(pu, pv, qw)) | (uint32_t(bin) << 12);
}

// An image that is coded on its own: one u16 (prob | bin << 15) per bin into b.coded.
// A lane of a PACK (E1Job::pack_rows set): the wave holds the 64 bins of one group, a bin per lane; lanes 0..12 assemble
// the group's thirteen 64-bit words (range_coder.h: codes 4j .. 4j+3 in the low 52 bits; on top the probability of code
// 52 + j or, word 12, the twelve bins of codes 52 .. 63, a slice of the wave's ballot) and store them back to back
// -- 104 contiguous bytes -- into the image's OWN stream of groups in b.tin.  k_pack_rows then lays the streams of a
// pack side by side.  Every group that holds a bin is written whole (zero codes past the last bin).
__global__ void __launch_bounds__(256) k_mix(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const uint32_t r = xcd_block() * 256u + threadIdx.x;
    if ((r & ~63u) >= J.n_ev) return;                                  // the whole wave is beyond the image's bins
    const uint32_t code = mixed_code(J, r, gptr(J.b.totals)[kWideTouchFlag] != 0u);
    if (!J.pack_rows) {
        if (r < J.n_ev) gptr(J.b.coded)[r] = pack_coded(int(code & 0xFFFu), int(code >> 12));
        return;
    }
    const int lane = int(threadIdx.x) & 63;
    const int j = lane < kPackWords ? lane : kPackWords - 1;
    const uint32_t c0 = uint32_t(__builtin_amdgcn_ds_bpermute((4 * j + 0) << 2, int(code)));
    const uint32_t c1 = uint32_t(__builtin_amdgcn_ds_bpermute((4 * j + 1) << 2, int(code)));
    const uint32_t c2 = uint32_t(__builtin_amdgcn_ds_bpermute((4 * j + 2) << 2, int(code)));
    const uint32_t c3 = uint32_t(__builtin_amdgcn_ds_bpermute((4 * j + 3) << 2, int(code)));
    const uint32_t top_prob = uint32_t(__builtin_amdgcn_ds_bpermute((52 + (j < 12 ? j : 0)) << 2, int(code))) & 0xFFFu;
    const uint64_t ones = __ballot((code >> 12) != 0u);
    const uint64_t top = j < 12 ? uint64_t(top_prob) : ((ones >> 52) & 0xFFFull);
    const uint64_t word = uint64_t(c0) | (uint64_t(c1) << 13) | (uint64_t(c2) << 26) | (uint64_t(c3) << 39) | (top << 52);
    if (lane < kPackWords) ((NB_GLOBAL uint64_t *)gptr(J.b.tin))[size_t(r >> 6) * kPackWords + size_t(lane)] = word;
}

// The transposition, once per group launch on the group's own stream: blockIdx.y is a pack (jobs 8 y .. 8 y + 7 of the
// launch, as many of them as share the first one's pack_rows); thread t writes output word t = (13 g + j) * 8 + lane,
// read from word 13 g + j of that lane's stream (zero where the lane has no such group).  A wave reads eight runs of
// contiguous words and writes 512 contiguous bytes: pure streaming, 1.625 bytes per bin in and out.
// (k_mix must walk ONE image at a time, and must not store between the other images' words itself: DESIGN.md 9-1.)
__global__ void __launch_bounds__(256) k_pack_rows(const E1Job *__restrict__ jobs, int n_jobs) {
    const int first = int(blockIdx.y) * kPackLanes;
    const E1Job &J0 = jobs[first];
    if (!J0.pack_rows) return;
    uint32_t most = 0;
    int cnt = 0;
    for (int k = 0; k < kPackLanes && first + k < n_jobs && jobs[first + k].pack_rows == J0.pack_rows; k++) { cnt = k + 1; most = max(most, jobs[first + k].n_ev); }
    const uint32_t groups = (most + 63u) / 64u;
    const size_t t = size_t(xcd_block()) * 256u + threadIdx.x;
    if (t >= size_t(groups) * (kPackWords * kPackLanes)) return;
    const uint32_t g = uint32_t(t / (kPackWords * kPackLanes)), w = uint32_t(t % (kPackWords * kPackLanes));
    const int k = int(w % kPackLanes), j = int(w / kPackLanes);
    uint64_t v = 0;
    if (k < cnt && g * 64u < jobs[first + k].n_ev) v = ((NB_GLOBAL const uint64_t *)gptr(jobs[first + k].b.tin))[size_t(g) * kPackWords + size_t(j)];
    gptr(J0.pack_rows)[t] = v;
}

// ---- seek-index entry records (kernels_e1.h IndexRecordTask) --------------------------------
// One workgroup per entry.  Every global access is a run of consecutive words or bytes over consecutive lanes: the
// counters keep their 256-node runs (a tree's nodes are consecutive keys), and the re-mappers' 60-int records go through
// LDS, 64 re-mappers at a time, so that the three tables they are split into are written as dense streams.
__global__ void __launch_bounds__(256) k_index_records(const E1Job *__restrict__ jobs, const IndexRecordTask *__restrict__ tasks, uint8_t *__restrict__ out) {
    constexpr int kTile = 64;                                             // re-mappers per LDS tile
    __shared__ int tile[kTile * 60];
    const IndexRecordTask T = tasks[blockIdx.x];
    const E1Job &J = jobs[T.job];
    const int t = int(threadIdx.x);
    const auto rec = gptr(out) + T.out;
    const auto words = (NB_GLOBAL uint32_t *)rec;
    constexpr int kHeadWords = int(sizeof(SerialState) / 4), kBiasWord = int(offsetof(SerialState, bias) / 4);
    if (t < kHeadWords) words[t] = t == kBiasWord ? uint32_t(lsq::kBiasInit) : 0u;
    const auto tab = words + kHeadWords;
    const auto ctx_state = gptr(J.b.ctx_state);
    for (int k = t; k < kContexts; k += 256) tab[k] = uint32_t(ctx_state[k]);
    const auto cnt_state = (NB_GLOBAL const i32x2 *)gptr(J.b.cnt_state);
    for (int key = t; key < 4096; key += 256) {
        const i32x2 c = cnt_state[key];
        const int tree = ((key >> 8) & 7) * 2 + (key >> 11), node = key & 255;
        tab[kContexts + tree * kTreeNodes + node] = uint32_t(c.x) | (uint32_t(c.y) << 16);
    }
    const auto map_state = gptr(J.b.map_state);
    const auto rank = rec + sizeof(SerialState) + size_t(kRecRank) * 4, sym = rec + sizeof(SerialState) + size_t(kRecSym) * 4;
    for (int m0 = 0; m0 < 512; m0 += kTile) {
        for (int k = t; k < kTile * 60; k += 256) tile[k] = map_state[m0 * 60 + k];
        __syncthreads();
        for (int k = t; k < kTile * kMapSyms; k += 256) {
            const int m = k / kMapSyms, q = k - m * kMapSyms;
            rank[m0 * kMapSyms + k] = uint8_t(tile[m * 60 + q]);
            sym[m0 * kMapSyms + k] = uint8_t(tile[m * 60 + 20 + q]);
            tab[kRecCount + m0 * kMapSyms + k] = uint32_t(tile[m * 60 + 40 + q]);
        }
        __syncthreads();
    }
    // rows [r - n, r) of the image, n = min(r, 2), behind (2 - n) w zero bytes; r = the row behind the band.  b.img is the
    // band's first row and the plane goes on above it.
    const int w = J.w, r = J.row0 + J.h, n = r < 2 ? r : 2;
    const auto rows = rec + kDecodeStateBytes;
    const auto img = gptr(J.b.img);
    const ptrdiff_t zeros = ptrdiff_t(2 - n) * w, from = ptrdiff_t(J.h - n) * w;
    for (ptrdiff_t k = t; k < 2 * ptrdiff_t(w); k += 256) rows[k] = k < zeros ? uint8_t(0) : img[from + (k - zeros)];
}

// ---- model state init (NBLIC.c:797-804) ---------------------------------------------------
__global__ void k_init_state(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.y];
    const auto ctx_state = gptr(J.b.ctx_state); const auto map_state = gptr(J.b.map_state); const auto cnt_state = (NB_GLOBAL i32x2 *)gptr(J.b.cnt_state);
    int g = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (g < 3072) { ctx_state[g] = 0; gptr(J.b.qhist)[g] = 0; }        // 3072: QNBLIC's context count / 12 x 256 histogram bins
    if (g < 4096) cnt_state[g] = i32x2{kWeightOne, kWeightOne};
    if (g < 512)
        for (int k = 0; k < kMapSyms; k++) {
            map_state[g * 60 + k] = k; map_state[g * 60 + 20 + k] = k; map_state[g * 60 + 40 + k] = 2 * (kMapSyms - 1 - k);
        }
}

// ------------------------------------------------------------------------------------------
// exclusive scan (u32 out) over u32 or u8 input: reduce -> scan block sums -> apply
// ------------------------------------------------------------------------------------------
// WHICH selects the job's array: 0 adr table, 1 mapper table, 2 bin counts (u8), 3 touch table.
constexpr int kScanThreads = 256, kScanPerThread = 16, kScanTile = kScanThreads * kScanPerThread;

template <int WHICH> struct ScanSel;
template <> struct ScanSel<0> { typedef uint32_t T; static __device__ auto in(const E1Job &J) { return gptr(J.b.table); }  static __device__ auto out(const E1Job &J) { return gptr(J.b.table); }  static __device__ uint32_t n(const E1Job &J) { return uint32_t(kContexts) * J.pp.nseg; } };
template <> struct ScanSel<1> { typedef uint32_t T; static __device__ auto in(const E1Job &J) { return gptr(J.b.table); }  static __device__ auto out(const E1Job &J) { return gptr(J.b.table); }  static __device__ uint32_t n(const E1Job &J) { return 512u * J.pp.nseg; } };
template <> struct ScanSel<2> { typedef uint8_t  T; static __device__ auto in(const E1Job &J) { return gptr(J.b.cnt); }    static __device__ auto out(const E1Job &J) { return gptr(J.b.ev_off); } static __device__ uint32_t n(const E1Job &J) { return J.n; } };
template <> struct ScanSel<4> { typedef uint32_t T; static __device__ auto in(const E1Job &J) { return gptr(J.b.table); }  static __device__ auto out(const E1Job &J) { return gptr(J.b.table); }  static __device__ uint32_t n(const E1Job &J) { return 3072u * J.pp.nseg; } };
template <> struct ScanSel<3> { typedef uint32_t T; static __device__ auto in(const E1Job &J) { return gptr(J.b.table); }  static __device__ auto out(const E1Job &J) { return gptr(J.b.table); }  static __device__ uint32_t n(const E1Job &J) { return 4096u * J.pe.nseg; } };

template <int WHICH>
__global__ void __launch_bounds__(kScanThreads) k_scan_reduce(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t part[kScanThreads / 64];
    const E1Job &J = jobs[blockIdx.y];
    const auto in = ScanSel<WHICH>::in(J);
    const uint32_t n = ScanSel<WHICH>::n(J);
    uint32_t base = blockIdx.x * uint32_t(kScanTile) + threadIdx.x * kScanPerThread, s = 0;
    if (blockIdx.x * uint32_t(kScanTile) >= n) return;
    for (int k = 0; k < kScanPerThread; k++) if (base + k < n) s += uint32_t(in[base + k]);
    s = wave_scan_incl(s);
    if (lane_id() == 63) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) gptr(J.b.scan_sums)[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

template <int WHICH>
__global__ void __launch_bounds__(1024) k_scan_sums(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t part[16];
    __shared__ uint32_t carry;
    const E1Job &J = jobs[blockIdx.y];
    const auto sums = gptr(J.b.scan_sums);
    const uint32_t nblocks = (ScanSel<WHICH>::n(J) + kScanTile - 1) / kScanTile;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        uint32_t i = base + threadIdx.x;
        uint32_t v = i < nblocks ? sums[i] : 0u;
        uint32_t incl = wave_scan_incl(v);
        if (lane_id() == 63) part[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t pre = carry;
        for (int wv = 0; wv < int(threadIdx.x >> 6); wv++) pre += part[wv];
        if (i < nblocks) sums[i] = pre + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = pre + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        gptr(J.b.totals)[WHICH & 3] = carry;
        if (WHICH == 3 && carry >= kPosMask) gptr(J.b.totals)[kWideTouchFlag] = 1u;          // touches: too many for 28-bit positions
    }
}

template <int WHICH>
__global__ void __launch_bounds__(kScanThreads) k_scan_apply(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t part[kScanThreads / 64];
    const E1Job &J = jobs[blockIdx.y];
    const auto in = ScanSel<WHICH>::in(J);     // may alias out (each thread re-writes its own items)
    const auto out = ScanSel<WHICH>::out(J);
    const uint32_t n = ScanSel<WHICH>::n(J);
    if (blockIdx.x * uint32_t(kScanTile) >= n) return;
    uint32_t base = blockIdx.x * uint32_t(kScanTile) + threadIdx.x * kScanPerThread;
    uint32_t v[kScanPerThread], s = 0;
    for (int k = 0; k < kScanPerThread; k++) { v[k] = base + k < n ? uint32_t(in[base + k]) : 0u; s += v[k]; }
    uint32_t incl = wave_scan_incl(s);
    if (lane_id() == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t pre = gptr(J.b.scan_sums)[blockIdx.x] + incl - s;
    for (int wv = 0; wv < int(threadIdx.x >> 6); wv++) pre += part[wv];
    for (int k = 0; k < kScanPerThread; k++) { if (base + k < n) out[base + k] = pre; pre += v[k]; }
}

// ------------------------------------------------------------------------------------------
// QNBLIC (effort 0, QNBLIC.c:562-623): stateless predict -> partition by context -> coupled
// context chains -> symbols + per-level histograms.  Shares the partition / chain kernels above.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_q_predict(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.z];
    const int w = J.w;
    int j = int(blockIdx.x) * 256 + int(threadIdx.x);
    int i = int(blockIdx.y);
    if (i >= J.h || j >= w) return;
    const auto img = gptr(J.b.img);
    auto pix = [&](int r, int c) { return int(img[size_t(r) * size_t(w) + size_t(c)]); };
    Taps n = sample_taps_q(pix, w, i, j);
    int px0 = predict_q(n);
    int err_prev = 0;
    if (j > 0) err_prev = pix(i, j - 1) - predict_q(sample_taps_q(pix, w, i, j - 1));
    int qd = level_q(n, err_prev);
    gptr(J.b.rec1)[size_t(i) * size_t(w) + size_t(j)] = uint32_t(px0) | (uint32_t(context_address_q(n, qd, px0)) << 8);
}

// The same for a ROW BAND (E1Job::row0; q_launch_model_band): b.img / b.rec1 start at image row row0, and the window's
// closed form sees the row in the IMAGE -- rows 0 and 1 are special wherever the band starts -- and reads the one or two
// rows above the band from the plane, which goes on above b.img.  A kernel of its own: the whole-image grid above keeps
// its unsigned addressing.
__global__ void __launch_bounds__(256) k_q_predict_band(const E1Job *__restrict__ jobs) {
    const E1Job &J = jobs[blockIdx.z];
    const int w = J.w, row0 = J.row0;
    int j = int(blockIdx.x) * 256 + int(threadIdx.x);
    int i = int(blockIdx.y);                                             // the row's index in b.img / b.rec1
    if (i >= J.h || j >= w) return;
    const auto img = gptr(J.b.img);
    auto pix = [&](int r, int c) { return int(img[(ptrdiff_t(r) - ptrdiff_t(row0)) * ptrdiff_t(w) + ptrdiff_t(c)]); };   // r: row in the image
    Taps n = sample_taps_q(pix, w, row0 + i, j);
    int px0 = predict_q(n);
    int err_prev = 0;
    if (j > 0) err_prev = pix(row0 + i, j - 1) - predict_q(sample_taps_q(pix, w, row0 + i, j - 1));
    int qd = level_q(n, err_prev);
    gptr(J.b.rec1)[size_t(i) * size_t(w) + size_t(j)] = uint32_t(px0) | (uint32_t(context_address_q(n, qd, px0)) << 8);
}

// A band adds its counts to the slot's qhist, which k_init_state zeroes at an image's first band alone.
__global__ void __launch_bounds__(256) k_q_symbols(const E1Job *__restrict__ jobs) {
    __shared__ uint32_t hist[12 * 256];
    const E1Job &J = jobs[blockIdx.y];
    const auto rec1 = gptr(J.b.rec1); const auto x = gptr(J.b.img); const auto s2out = gptr(J.b.s2out);
    const auto pos2 = gptr(J.b.pos2); const auto qy = gptr(J.b.pxs);
    for (int k = int(threadIdx.x); k < 12 * 256; k += 256) hist[k] = 0;
    __syncthreads();
    const uint32_t n = J.n;
    const uint32_t per_block = ((n + gridDim.x - 1) / gridDim.x + 255u) & ~255u;      // a contiguous run of pixels per block, XCD-contiguous
    const uint32_t t_lo = xcd_block() * per_block, t_hi = min(n, t_lo + per_block);
    for (uint32_t t = t_lo + threadIdx.x; t < t_hi; t += 256u) {
        const uint32_t r = rec1[t];
        const int vs = int(int16_t(s2out[pos2[t]]));                 // context state >> 10 as the chain saw it
        const int sign = vs & 1, qd = int(r >> 16);
        const int px = iclip(int(r & 0xFF) + (vs >> 1) + sign, 0, kMaxVal);
        const int y = residual_to_symbol(int(x[t]), px, sign, 0);    // QNBLIC.c:191-202 == NBLIC's map at near 0
        qy[t] = uint16_t(qd | (y << 8));
        atomicAdd(&hist[qd * 256 + y], 1u);
    }
    __syncthreads();
    for (int k = int(threadIdx.x); k < 12 * 256; k += 256) if (hist[k]) atomicAdd(J.b.qhist + k, hist[k]);
}

// QNBLIC's seek-index entry records (kernels_e1.h q_launch_index_records): one workgroup per entry.  The decoder keeps its
// 3072 contexts as the chains keep them (the same v, read as v >> 10), so the record is a zero header, ctx_state verbatim
// and the two rows above the row behind the band -- the layout k_index_capture leaves for kind 1.
__global__ void __launch_bounds__(256) k_q_index_records(const E1Job *__restrict__ jobs, const IndexRecordTask *__restrict__ tasks, uint8_t *__restrict__ out) {
    const IndexRecordTask T = tasks[blockIdx.x];
    const E1Job &J = jobs[T.job];
    const int t = int(threadIdx.x);
    const auto rec = gptr(out) + T.out;
    const auto words = (NB_GLOBAL uint32_t *)rec;
    constexpr int kHeadWords = int(sizeof(SerialState) / 4);
    if (t < kHeadWords) words[t] = 0u;
    const auto ctx_state = gptr(J.b.ctx_state);
    for (int k = t; k < 3072; k += 256) words[kHeadWords + k] = uint32_t(ctx_state[k]);
    // rows [r - n, r) of the image, n = min(r, 2), behind (2 - n) w zero bytes (k_index_records)
    const int w = J.w, r = J.row0 + J.h, n = r < 2 ? r : 2;
    const auto rows = rec + kQDecodeStateBytes;
    const auto img = gptr(J.b.img);
    const ptrdiff_t zeros = ptrdiff_t(2 - n) * w, from = ptrdiff_t(J.h - n) * w;
    for (ptrdiff_t k = t; k < 2 * ptrdiff_t(w); k += 256) rows[k] = k < zeros ? uint8_t(0) : img[from + (k - zeros)];
}

// self-test: the DPP scan must equal the shuffle scan on arbitrary data
__global__ void k_selftest_scan(const uint32_t *in, uint32_t *bad) {
    uint32_t v = in[blockIdx.x * 64 + threadIdx.x];
    if (wave_scan_incl(v) != wave_scan_incl_dpp(v)) atomicAdd(bad, 1u);
}

int e1_selftest(hipStream_t s) {
    uint32_t host[64 * 64], *d_in = nullptr, *d_bad = nullptr, bad = 1;
    uint32_t x = 12345u;
    for (auto &h : host) { x = x * 1664525u + 1013904223u; h = x >> 8; }
    if (hipMalloc((void **)&d_in, sizeof host) != hipSuccess || hipMalloc((void **)&d_bad, 4) != hipSuccess) return -1;
    hipMemcpyAsync(d_in, host, sizeof host, hipMemcpyHostToDevice, s);
    hipMemsetAsync(d_bad, 0, 4, s);
    hipLaunchKernelGGL(k_selftest_scan, dim3(64), dim3(64), 0, s, d_in, d_bad);
    hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    hipFree(d_in); hipFree(d_bad);
    return int(bad);
}

// ------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------
static inline unsigned cdiv(size_t a, size_t b) { return unsigned((a + b - 1) / b); }
static inline unsigned pad8(unsigned v) { return (v + 7u) & ~7u; }       // grids of kernels that use xcd_block()

struct Marker {                       // records one event in front of every launch
    E1Timers *tm; hipStream_t s; int k;
    void operator()() {
        if (tm && (((tm->mask >> k) & 1ull) || (k > 0 && ((tm->mask >> (k - 1)) & 1ull)))) hipEventRecord(tm->ev[k], s);
        k++;
    }
};

template <int WHICH>
static void scan_exclusive(const E1Job *jobs, int n_jobs, uint32_t max_items, hipStream_t s, Marker &mark) {
    unsigned nb = cdiv(max_items, kScanTile);
    if (nb == 0) nb = 1;
    mark(); hipLaunchKernelGGL(k_scan_reduce<WHICH>, dim3(nb, n_jobs), dim3(kScanThreads), 0, s, jobs);
    mark(); hipLaunchKernelGGL(k_scan_sums<WHICH>, dim3(1, n_jobs), dim3(1024), 0, s, jobs);
    mark(); hipLaunchKernelGGL(k_scan_apply<WHICH>, dim3(nb, n_jobs), dim3(kScanThreads), 0, s, jobs);
}

SegPlan make_plan(uint32_t n_items, uint32_t max_segments) {
    SegPlan p;
    uint32_t want = (n_items + max_segments - 1) / max_segments;          // items per segment
    if (want < 1024) want = 1024;
    p.seg_len = (want + 63u) & ~63u;
    p.nseg = int((n_items + p.seg_len - 1) / p.seg_len);
    if (p.nseg < 1) p.nseg = 1;
    return p;
}

// S3: the chains short enough for one lane each, then those that are cut into blocks (6 launches; 1 with long chains off)
static void launch_mapper_chains(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, uint32_t max_n, hipStream_t s) {
    hipLaunchKernelGGL(k_mapper_chains, dim3(512 / kMapLanes, n_jobs), dim3(64), 0, s, d_jobs);
    if (h_jobs[0].long_min < 0) return;
    const unsigned B = unsigned(h_jobs[0].long_block > kLongBlockMin ? h_jobs[0].long_block : kLongBlockMin);
    const unsigned most = max_n / unsigned(h_jobs[0].long_min > 1 ? h_jobs[0].long_min : 1) + 1u;      // cut chains of a job, at most
    const unsigned max_blocks = max_n / B + (most < 512u ? most : 512u);                               // one partial block per chain
    hipLaunchKernelGGL(k_map_plan, dim3(1, n_jobs), dim3(512), 0, s, d_jobs);
    hipLaunchKernelGGL(k_map_hist, dim3(max_blocks, n_jobs), dim3(64), 0, s, d_jobs);
    hipLaunchKernelGGL(k_map_prefix, dim3(512, n_jobs), dim3(64), 0, s, d_jobs);
    hipLaunchKernelGGL(k_map_blocks, dim3(cdiv(max_blocks, kMapLanes), n_jobs), dim3(64), 0, s, d_jobs);
    hipLaunchKernelGGL(k_map_check, dim3(512 / kMapLanes, n_jobs), dim3(64), 0, s, d_jobs);
}

// The front half behind S1, from the S1 records in b.rec1: partition by context, the context chains, partition by
// re-mapper, the re-mapper chains, the bin counts and their scan.  19 launches.  `model_done`, if given, is recorded
// behind k_bias_fixup.
static void front_behind_s1(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, int max_nseg, uint32_t max_n, hipStream_t s, Marker &mark, hipEvent_t model_done) {
    const bool long_chains = h_jobs[0].long_min >= 0;
    const dim3 seg_grid(pad8(cdiv(max_nseg, 4)), n_jobs), px_grid(pad8(cdiv(max_n, 256)), n_jobs);
    mark(); hipLaunchKernelGGL(k_adr_count<NbModel>, seg_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<0>(d_jobs, n_jobs, uint32_t(kContexts) * max_nseg, s, mark);
    mark(); hipLaunchKernelGGL(k_adr_scatter<NbModel>, seg_grid, dim3(256), 0, s, d_jobs);
    mark(); hipLaunchKernelGGL(k_plan_blocks<NbModel>, dim3(1, n_jobs), dim3(1024), 0, s, d_jobs);
    const unsigned max_blocks = max_n / kBiasBlock + unsigned(kContexts);
    mark(); hipLaunchKernelGGL(k_bias_blocks<NbModel>, dim3(cdiv(max_blocks, 64), n_jobs), dim3(64), 0, s, d_jobs);
    mark();                                                     // one timed stage "k_bias_fixup": tables, the walk, the replay
    const unsigned max_tabs = max_n / kBiasBlock + 1u;
    if (long_chains) hipLaunchKernelGGL(k_bias_tabulate<NbModel>, dim3(max_tabs, n_jobs), dim3(kBiasCands), 0, s, d_jobs);
    hipLaunchKernelGGL(k_bias_fixup<NbModel>, dim3(kContexts / 64, n_jobs), dim3(64), 0, s, d_jobs);
    if (long_chains) hipLaunchKernelGGL(k_bias_replay<NbModel>, dim3(cdiv(max_tabs, 64), n_jobs), dim3(64), 0, s, d_jobs);
    if (model_done) hipEventRecord(model_done, s);
    mark(); hipLaunchKernelGGL(k_map_count, seg_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<1>(d_jobs, n_jobs, 512u * max_nseg, s, mark);
    mark(); hipLaunchKernelGGL(k_map_scatter<false>, seg_grid, dim3(256), 0, s, d_jobs);
    mark(); launch_mapper_chains(d_jobs, h_jobs, n_jobs, max_n, s);       // one timed stage "k_mapper_chains": the cut chains' kernels too
    mark(); hipLaunchKernelGGL(k_count_bins<false>, px_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<2>(d_jobs, n_jobs, max_n, s, mark);
    mark();                                                     // start of the host gap (index 20)
}

// Front half for a group of jobs: everything up to the per-pixel bin counts and their scan
// (the event totals are needed on the host before the event buffers can be sized).  18 launches.
// BAND: the jobs are row bands of images whose earlier rows have been coded (E1Job::row0): the model tables are the
// caller's, so nothing is initialised -- every chain kernel starts from the table entry of its key and writes the end
// state back -- and S1 is the band variant.  `model_done` (BAND only) is recorded behind k_bias_fixup.
template <bool BAND>
static void launch_front(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, E1Timers *tm, hipEvent_t model_done) {
    int max_w = 0, max_h = 0, max_nseg = 0; uint32_t max_n = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_w = h_jobs[k].w > max_w ? h_jobs[k].w : max_w; max_h = h_jobs[k].h > max_h ? h_jobs[k].h : max_h;
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_nseg = h_jobs[k].pp.nseg > max_nseg ? h_jobs[k].pp.nseg : max_nseg;
    }
    Marker mark{tm, s, 0};
    if (!BAND) { mark(); hipLaunchKernelGGL(k_init_state, dim3(16, n_jobs), dim3(256), 0, s, d_jobs); }   // (a band launch is not timed by stage: tm is null)
    mark();                                                     // one timed stage "k_predict": interior rows + the two border launches
    if (BAND) {                                                 // which of a band's rows are top rows is the kernels' business (row0)
        int top_rows = 0;                                       // local rows below which some job has an image row 0 / 1: none for every band but an image's first one or two
        for (int k = 0; k < n_jobs; k++) {
            const int t = 2 - h_jobs[k].row0 < h_jobs[k].h ? 2 - h_jobs[k].row0 : h_jobs[k].h;
            top_rows = t > top_rows ? t : top_rows;
        }
        if (max_h > 0 && max_w >= 20) hipLaunchKernelGGL(k_predict_rows<true>, dim3(cdiv((max_w - 12) / 8, 256), max_h, n_jobs), dim3(256), 0, s, d_jobs);
        if (top_rows > 0) hipLaunchKernelGGL(k_predict_border<true>, dim3(cdiv(max_w, 64), top_rows, n_jobs), dim3(64), 0, s, d_jobs, 1);
        hipLaunchKernelGGL(k_predict_border<true>, dim3(1, max_h, n_jobs), dim3(64), 0, s, d_jobs, 0);
    } else {
        if (max_h > 2 && max_w >= 20) hipLaunchKernelGGL(k_predict_rows<false>, dim3(cdiv((max_w - 12) / 8, 256), max_h - 2, n_jobs), dim3(256), 0, s, d_jobs);
        hipLaunchKernelGGL(k_predict_border<false>, dim3(cdiv(max_w, 64), max_h < 2 ? max_h : 2, n_jobs), dim3(64), 0, s, d_jobs, 1);
        if (max_h > 2) hipLaunchKernelGGL(k_predict_border<false>, dim3(1, max_h - 2, n_jobs), dim3(64), 0, s, d_jobs, 0);
    }
    front_behind_s1(d_jobs, h_jobs, n_jobs, max_nseg, max_n, s, mark, BAND ? model_done : nullptr);
}

void e1_launch_front(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, E1Timers *tm) {
    launch_front<false>(d_jobs, h_jobs, n_jobs, s, tm, nullptr);
}

void e1_launch_front_band(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, hipEvent_t model_done) {
    launch_front<true>(d_jobs, h_jobs, n_jobs, s, nullptr, model_done);
}

void e1_launch_model_stages(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s) {
    int max_nseg = 0; uint32_t max_n = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_nseg = h_jobs[k].pp.nseg > max_nseg ? h_jobs[k].pp.nseg : max_nseg;
    }
    Marker mark{nullptr, s, 0};
    front_behind_s1(d_jobs, h_jobs, n_jobs, max_nseg, max_n, s, mark, nullptr);
}

// Front half of the serial modes: rec1 and px | sign per pixel come from the serial model stage
// (k_serial_model, launched by the caller on the same stream before this), so the partition by
// context and the context chains are skipped; near and k_step come from the job.
void e1_launch_front_pre(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s) {
    int max_nseg = 0; uint32_t max_n = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_nseg = h_jobs[k].pp.nseg > max_nseg ? h_jobs[k].pp.nseg : max_nseg;
    }
    const dim3 seg_grid(pad8(cdiv(max_nseg, 4)), n_jobs), px_grid(pad8(cdiv(max_n, 256)), n_jobs);
    Marker mark{nullptr, s, 0};
    hipLaunchKernelGGL(k_map_count_pre, seg_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<1>(d_jobs, n_jobs, 512u * max_nseg, s, mark);
    hipLaunchKernelGGL(k_map_scatter<true>, seg_grid, dim3(256), 0, s, d_jobs);
    launch_mapper_chains(d_jobs, h_jobs, n_jobs, max_n, s);
    hipLaunchKernelGGL(k_count_bins<true>, px_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<2>(d_jobs, n_jobs, max_n, s, mark);
}

void e1_launch_init(const E1Job *d_jobs, int n_jobs, hipStream_t s) {
    hipLaunchKernelGGL(k_init_state, dim3(16, n_jobs), dim3(256), 0, s, d_jobs);
}

void e1_launch_index_records(const E1Job *d_jobs, const IndexRecordTask *d_tasks, int n_tasks, uint8_t *d_out, hipStream_t s) {
    if (n_tasks > 0) hipLaunchKernelGGL(k_index_records, dim3(unsigned(n_tasks)), dim3(256), 0, s, d_jobs, d_tasks, d_out);
}

// The back half behind k_emit_bins, from the bin events in b.events: partition the counter touches, the counter
// chains, the mix; k_pack_rows behind it when the launch has packs.  9 launches (10 with packs).
static void back_behind_emit(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, int max_nseg, uint32_t max_ev, hipStream_t s, Marker &mark) {
    const dim3 seg_grid(pad8(cdiv(max_nseg, 4)), n_jobs);
    mark(); hipLaunchKernelGGL(k_touch_count, seg_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<3>(d_jobs, n_jobs, 4096u * max_nseg, s, mark);
    mark();
    if (h_jobs[0].dbg & 8) hipLaunchKernelGGL(k_touch_scatter<true>, dim3(seg_grid.x, seg_grid.y, 2), dim3(256), 0, s, d_jobs);
    else hipLaunchKernelGGL(k_touch_scatter<false>, dim3(seg_grid.x, seg_grid.y, 2), dim3(256), 0, s, d_jobs);
    mark(); hipLaunchKernelGGL(k_plan_windows, dim3(1, n_jobs), dim3(1024), 0, s, d_jobs);
    mark(); hipLaunchKernelGGL(k_counter_epochs, dim3(4096, n_jobs), dim3(64), 0, s, d_jobs);
    const unsigned max_windows = unsigned(2ull * max_ev / kWin) + 4096u;          // every touch list has <= 2 touches per bin
    mark(); hipLaunchKernelGGL(k_counter_probs, dim3(cdiv(max_windows, 4), n_jobs), dim3(256), 0, s, d_jobs);
    mark(); hipLaunchKernelGGL(k_mix, dim3(pad8(cdiv(max_ev, 256) ? cdiv(max_ev, 256) : 1), n_jobs), dim3(256), 0, s, d_jobs);
    uint32_t pack_ev = 0;                                       // the longest image that sits in a pack
    for (int k = 0; k < n_jobs; k++) if (h_jobs[k].pack_rows && h_jobs[k].n_ev > pack_ev) pack_ev = h_jobs[k].n_ev;
    if (pack_ev) hipLaunchKernelGGL(k_pack_rows, dim3(pad8(cdiv(cdiv(pack_ev, 64) * unsigned(kPackWords * kPackLanes), 256)), cdiv(unsigned(n_jobs), unsigned(kPackLanes))), dim3(256), 0, s, d_jobs, n_jobs);
    mark();                                                     // index 31: end
}

// Back half: needs n_ev / pe filled in the job records and event-sized buffers.  10 launches.
void e1_launch_back(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s, E1Timers *tm, bool general) {
    int max_nseg = 0; uint32_t max_n = 0, max_ev = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_ev = h_jobs[k].n_ev > max_ev ? h_jobs[k].n_ev : max_ev;
        max_nseg = h_jobs[k].pe.nseg > max_nseg ? h_jobs[k].pe.nseg : max_nseg;
    }
    Marker mark{tm, s, 21};
    mark();
    if (general) hipLaunchKernelGGL(k_emit_bins<true>, dim3(pad8(cdiv(max_n, 256)), n_jobs), dim3(256), 0, s, d_jobs);
    else hipLaunchKernelGGL(k_emit_bins<false>, dim3(pad8(cdiv(max_n, 256)), n_jobs), dim3(256), 0, s, d_jobs);
    back_behind_emit(d_jobs, h_jobs, n_jobs, max_nseg, max_ev, s, mark);
}

void e1_launch_back_stages(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s) {
    int max_nseg = 0; uint32_t max_ev = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_ev = h_jobs[k].n_ev > max_ev ? h_jobs[k].n_ev : max_ev; max_nseg = h_jobs[k].pe.nseg > max_nseg ? h_jobs[k].pe.nseg : max_nseg;
    }
    Marker mark{nullptr, s, 22};
    back_behind_emit(d_jobs, h_jobs, n_jobs, max_nseg, max_ev, s, mark);
}

// QNBLIC's model stage behind k_q_predict, from px0 | adr << 8 in b.rec1: partition by context, the context chains, the
// symbols and their histograms.  9 launches.
static void q_behind_predict(const E1Job *d_jobs, int n_jobs, int max_nseg, uint32_t max_n, bool long_chains, hipStream_t s) {
    const dim3 seg_grid(pad8(cdiv(max_nseg, 4)), n_jobs);
    Marker mark{nullptr, s, 0};
    hipLaunchKernelGGL(k_adr_count<QModel>, seg_grid, dim3(256), 0, s, d_jobs);
    scan_exclusive<4>(d_jobs, n_jobs, 3072u * max_nseg, s, mark);
    hipLaunchKernelGGL(k_adr_scatter<QModel>, seg_grid, dim3(256), 0, s, d_jobs);
    hipLaunchKernelGGL(k_plan_blocks<QModel>, dim3(1, n_jobs), dim3(1024), 0, s, d_jobs);
    const unsigned max_blocks = max_n / kBiasBlock + 3072u;
    hipLaunchKernelGGL(k_bias_blocks<QModel>, dim3(cdiv(max_blocks, 64), n_jobs), dim3(64), 0, s, d_jobs);
    const unsigned max_tabs = max_n / kBiasBlock + 1u;
    if (long_chains) hipLaunchKernelGGL(k_bias_tabulate<QModel>, dim3(max_tabs, n_jobs), dim3(kBiasCands), 0, s, d_jobs);
    hipLaunchKernelGGL(k_bias_fixup<QModel>, dim3(3072 / 64, n_jobs), dim3(64), 0, s, d_jobs);
    if (long_chains) hipLaunchKernelGGL(k_bias_replay<QModel>, dim3(cdiv(max_tabs, 64), n_jobs), dim3(64), 0, s, d_jobs);
    unsigned sym_blocks = cdiv(max_n, 256 * 16);                      // 16 pixels per thread: fewer global histogram merges
    hipLaunchKernelGGL(k_q_symbols, dim3(pad8(sym_blocks ? sym_blocks : 1), n_jobs), dim3(256), 0, s, d_jobs);
}

void q_launch_model(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s) {
    int max_w = 0, max_h = 0, max_nseg = 0; uint32_t max_n = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_w = h_jobs[k].w > max_w ? h_jobs[k].w : max_w; max_h = h_jobs[k].h > max_h ? h_jobs[k].h : max_h;
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_nseg = h_jobs[k].pp.nseg > max_nseg ? h_jobs[k].pp.nseg : max_nseg;
    }
    hipLaunchKernelGGL(k_init_state, dim3(16, n_jobs), dim3(256), 0, s, d_jobs);
    hipLaunchKernelGGL(k_q_predict, dim3(cdiv(max_w, 256), max_h, n_jobs), dim3(256), 0, s, d_jobs);
    q_behind_predict(d_jobs, n_jobs, max_nseg, max_n, h_jobs[0].long_min >= 0, s);
}

void q_launch_model_band(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s) {
    int max_w = 0, max_h = 0, max_nseg = 0; uint32_t max_n = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_w = h_jobs[k].w > max_w ? h_jobs[k].w : max_w; max_h = h_jobs[k].h > max_h ? h_jobs[k].h : max_h;
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_nseg = h_jobs[k].pp.nseg > max_nseg ? h_jobs[k].pp.nseg : max_nseg;
    }
    for (int k = 0; k < n_jobs; k++)                                  // fresh contexts and histograms for the jobs that start an image
        if (h_jobs[k].row0 == 0) hipLaunchKernelGGL(k_init_state, dim3(16, 1), dim3(256), 0, s, d_jobs + k);
    hipLaunchKernelGGL(k_q_predict_band, dim3(cdiv(max_w, 256), max_h, n_jobs), dim3(256), 0, s, d_jobs);
    q_behind_predict(d_jobs, n_jobs, max_nseg, max_n, h_jobs[0].long_min >= 0, s);
}

void q_launch_index_records(const E1Job *d_jobs, const IndexRecordTask *d_tasks, int n_tasks, uint8_t *d_out, hipStream_t s) {
    if (n_tasks > 0) hipLaunchKernelGGL(k_q_index_records, dim3(unsigned(n_tasks)), dim3(256), 0, s, d_jobs, d_tasks, d_out);
}

void q_launch_model_stages(const E1Job *d_jobs, const E1Job *h_jobs, int n_jobs, hipStream_t s) {
    int max_nseg = 0; uint32_t max_n = 0;
    for (int k = 0; k < n_jobs; k++) {
        max_n = h_jobs[k].n > max_n ? h_jobs[k].n : max_n; max_nseg = h_jobs[k].pp.nseg > max_nseg ? h_jobs[k].pp.nseg : max_nseg;
    }
    q_behind_predict(d_jobs, n_jobs, max_nseg, max_n, h_jobs[0].long_min >= 0, s);
}

}  // namespace nblic
