// deep.h -- deep pixels: an image of 16-bit elements (uint16, or int16 such as Hounsfield units) as TWO ordinary 8-bit images,
// a HIGH plane and a LOW plane that may be FOLDED.  The mode byte, the tasks, the unit and tile walks, the pixel arithmetic
// and the three costs of an image, shared by the host and the device: the kernels' lanes (serial_engine.hip, k_collect_deep,
// k_deliver_deep and k_deep_cost) and the host-only deep_collect_host, deep_deliver_host and deep_cost_host below call the
// same functions, so the walks and the integer arithmetic are tested without a GPU (tests/test_deep_host.py,
// tools/deep_check.cpp).  The float arithmetic of deep_value has two bodies: the host body is tested without a GPU (the same
// files, and tests/test_float_edges_host.py against an exact reference), the device body by tests/test_float_edges.py
// against the same reference.  Built on collect.h and deliver.h; the tile geometry, the MED prediction, the bit length and the
// host's tile walk live in cost_tile.h.
//
// THE PLANES.  With u the element as an unsigned 16-bit number (uint16: u = x; int16: u = x + 32768, the sign bit flipped):
// hi = u >> 8, lo = u & 255.  Stream 2k of a call is the high plane of deep image k, stream 2k + 1 its low plane; both are
// ordinary streams of those planes and nothing in them names the mode.
//
// THE MODE, one byte per deep image.  Bit 0, the FOLD: the low plane holds 255 - lo wherever hi is odd.  The low byte of a
// smooth signal is a sawtooth that jumps by 255 whenever the high byte steps; folded on the parity of the high byte it is a
// triangle wave -- continuous, |d lo'| <= |d u| -- and the fold is its own inverse given hi.  Bit 1: the source was signed,
// the value is u - 32768.  Valid bytes: 0..3; 0xFF is what the plan gives an image it refuses.
//
// THE COSTS of an image are those of its three candidate planes -- high, low, folded low -- each the sum over its pixels of
// 2 * bitlen(|e|) + 1 with e = p - pred, pred the MED prediction of cost_tile.h (cost_pred).  e is NOT wrapped here
// (|e| <= 255, bitlen <= 8): the one deliberate difference from color_pixel_cost, which wraps mod 256.  A wrapped residual
// would rate the sawtooth's jumps of 255 at nothing -- and those jumps are exactly what the fold removes and what NBLIC, which
// does not wrap its residuals, pays for.
#pragma once
#include "deliver.h"
#include "collect.h"
#include "cost_tile.h"

namespace nblic {

enum : uint32_t { kDeepU16 = 0, kDeepI16 = 1, kDeepSrcFormats = 2 };                                        // deep_format of a source
enum : uint32_t { kDeepHigh = 0, kDeepLow = 1, kDeepLowFolded = 2, kDeepParts = 3 };                        // the plane a collect task writes; the cost table's order
enum : uint32_t { kDeepToU16 = 0, kDeepToI16 = 1, kDeepToF16 = 2, kDeepToBF16 = 3, kDeepToF32 = 4, kDeepDestFormats = 5 };
enum : uint32_t { kDeepFold = 1, kDeepSigned = 2, kDeepRefused = 0xFF };
constexpr uint32_t kDeepSums = 5;                                    // per image: the three costs, then min and max of u

// ---- the mode byte and the rule --------------------------------------------------------------------------------------------------
inline bool deep_mode_valid(uint32_t m) { return m < 4u; }
// THE RULE (part of the interface: two builds plan alike): fold iff cost(folded low) < cost(low), ties are plain -- no margin:
// the colour rule's 63/64 protects planes a plain decoder can read as they are, and a low plane is none.  Bit 1 is the source's.
inline uint8_t deep_choose(const unsigned long long costs[kDeepParts], uint32_t deep_format) {
    return uint8_t((costs[kDeepLowFolded] < costs[kDeepLow] ? kDeepFold : 0u) | (deep_format == kDeepI16 ? kDeepSigned : 0u));
}

// ---- the pixel arithmetic --------------------------------------------------------------------------------------------------------
CL_HD uint32_t deep_u(uint32_t x, uint32_t deep_format) { return (deep_format == kDeepI16 ? x ^ 0x8000u : x) & 0xFFFFu; }
CL_HD uint32_t deep_fold(uint32_t lo, uint32_t hi) { return (hi & 1u) ? 255u - lo : lo; }                   // its own inverse
CL_HD uint32_t deep_part(uint32_t u, uint32_t part) {
    const uint32_t hi = u >> 8, lo = u & 255u;
    return part == kDeepHigh ? hi : (part == kDeepLow ? lo : deep_fold(lo, hi));
}
// u of a pixel of the two planes.
CL_HD uint32_t deep_join(uint32_t hi, uint32_t lo, uint32_t mode) { return (hi << 8) | ((mode & kDeepFold) ? deep_fold(lo, hi) : lo); }

CL_HD uint32_t deep_dest_elem(uint32_t format) { return format == kDeepToF32 ? 4u : 2u; }
// One destination element's bits (in the low elem bytes).  uint16: u; int16: u - 32768 in two's complement; a float format:
// float(v) * scale + bias, v = u or u - 32768 by the mode's bit 1 (exact as a float), both operations rounded to float --
// never fused -- and the result rounded to nearest even into the format as deliver_value does (a binary16 overflow goes to
// infinity: deliver_f16_bits).
CL_HD uint32_t deep_value(uint32_t u, uint32_t mode, uint32_t format, float scale, float bias) {
    if (format == kDeepToU16) return u;
    if (format == kDeepToI16) return u ^ 0x8000u;
    const int val = (mode & kDeepSigned) ? int(u) - 32768 : int(u);
#if defined(__HIP_DEVICE_COMPILE__)
    const float v = __fadd_rn(__fmul_rn(float(val), scale), bias);
    if (format == kDeepToF32) return __float_as_uint(v);
    if (format == kDeepToF16) return uint32_t(__builtin_bit_cast(unsigned short, static_cast<_Float16>(v)));
    return deliver_bf16_bits(__float_as_uint(v));
#else
    volatile float prod = float(val) * scale;                        // (volatile: two roundings whatever the compiler's contraction rule)
    const float v = prod + bias;
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return format == kDeepToF32 ? bits : (format == kDeepToF16 ? deliver_f16_bits(bits) : deliver_bf16_bits(bits));
#endif
}

// ---- collection: one plane of a deep source into the encoders' contiguous uint8 plane ---------------------------------------------
// One task per PLANE: the high and the low plane of an image are two tasks, which may belong to different launches.  The
// units are k_collect's: sixteen consecutive bytes of the flat plane (collect.h collect_unit_of).  No scale and no bias: a
// 16-bit integer is coded as it is.
struct DeepCollectTask {
    const uint8_t *src;                    // element (0, 0) of the image; a multiple of 2
    uint8_t *dst;                          // pixel 0 of the flat plane; a multiple of 16
    unsigned long long pitch;              // bytes between source rows: a multiple of 2
    uint32_t step;                         // bytes between neighbouring elements of a source row: a multiple of 2
    uint32_t rows, cols;
    uint32_t px0, px1;                     // the pixels of the flat plane this task writes: [px0, px1), px1 <= rows * cols
    uint32_t format;                       // kDeepU16 / kDeepI16
    uint32_t part;                         // kDeepHigh / kDeepLow / kDeepLowFolded
    uint32_t first_chunk;                  // chunks of the launch's tasks in front of this one
};
static_assert(sizeof(DeepCollectTask) == 56, "uploaded as bytes");

// The task as the collect task whose unit walk it shares (px0 and px1 are all that walk looks at).
CL_HD CollectTask deep_collect_walk(const DeepCollectTask &t) {
    CollectTask c{};
    c.rows = t.rows; c.cols = t.cols; c.px0 = t.px0; c.px1 = t.px1;
    return c;
}
CL_HD uint32_t deep_collect_units(const DeepCollectTask &t) { return collect_task_units(deep_collect_walk(t)); }
CL_HD uint32_t deep_collect_chunks(const DeepCollectTask &t) { return collect_task_chunks(deep_collect_walk(t)); }

inline unsigned long long deep_src_extent(uint32_t rows, uint32_t cols, unsigned long long pitch, unsigned long long step) {
    return (unsigned long long)(rows - 1) * pitch + (unsigned long long)(cols - 1) * step + 2u;
}
// What a deep SOURCE must satisfy: an image the encoders take, a pointer, pitch and step that are multiples of 2 and not
// below it, within collect.h's limits, and an extent that cap_bytes holds.
inline bool deep_source_ok(const uint8_t *src, unsigned long long pitch, unsigned long long step, uint32_t rows, uint32_t cols, uint32_t format,
                           unsigned long long cap_bytes) {
    if (!src || format >= kDeepSrcFormats) return false;
    if (rows < 1 || cols < 1 || rows > kCollectMaxSide || cols > kCollectMaxSide) return false;
    if (uintptr_t(src) % 2 || pitch % 2 || step % 2 || step < 2 || pitch < 2 || step > kCollectMaxStep || pitch > kCollectMaxPitch) return false;
    return deep_src_extent(rows, cols, pitch, step) <= cap_bytes;
}
inline bool deep_collect_task_ok(const DeepCollectTask &t, unsigned long long cap_bytes) {
    return deep_source_ok(t.src, t.pitch, t.step, t.rows, t.cols, t.format, cap_bytes) && t.part < kDeepParts && t.dst && uintptr_t(t.dst) % 16 == 0 &&
           t.px0 < t.px1 && t.px1 <= t.rows * t.cols;
}

// The host walk: every unit of the task, one after the other, element by element.
inline void deep_collect_host(const DeepCollectTask &t) {
    const CollectTask W = deep_collect_walk(t);
    const uint32_t units = collect_task_units(W);
    for (uint32_t u = 0; u < units; u++) {
        const CollectUnit U = collect_unit_of(W, u);
        uint32_t row = U.p_lo / t.cols, col = U.p_lo - row * t.cols;
        for (uint32_t p = U.p_lo; p < U.p_hi; p++) {
            uint32_t x = 0;
            memcpy(&x, t.src + (unsigned long long)(row) * t.pitch + (unsigned long long)(col) * t.step, 2);     // (little endian: the low two bytes)
            t.dst[p] = uint8_t(deep_part(deep_u(x, t.format), t.part));
            if (++col == t.cols) { col = 0; row++; }
        }
    }
}

// ---- delivery: a window of the two decoded planes of one deep image into caller-owned memory --------------------------------------
// One task per deep image.  The units are k_deliver's: a contiguous destination has units of sixteen window pixels laid on
// 16-byte blocks of the destination row (deliver.h deliver_unit_of: heads and tails), a strided one sixteen consecutive
// window pixels counted from col0 and nothing wider than an element stored.
struct DeepDeliverTask {
    const uint8_t *hi, *lo;                // the planes at the window's FIRST row, column 0
    uint8_t *dst;                          // element (0, 0) of the window goes here; a multiple of the element size
    const SerialState *gate_hi, *gate_lo;  // not null: the image counts only if the status is kDone -- zeros otherwise
    unsigned long long hi_bytes, lo_bytes; // readable bytes from hi / lo: nothing outside them is read
    unsigned long long dst_pitch;          // bytes between destination rows
    uint32_t src_pitch;                    // bytes between the rows of both planes: the image's width
    uint32_t rows;                         // of the window
    uint32_t col0, col1;                   // its columns [col0, col1) of the planes
    uint32_t format;                       // kDeepToU16 .. kDeepToF32
    uint32_t mode;                         // the image's mode byte
    float scale, bias;                     // float formats
    uint32_t zero;                         // != 0: zero bytes instead of pixels
    uint32_t first_chunk;                  // chunks of the launch's tasks in front of this one
    uint32_t dst_step;                     // bytes between neighbouring elements of a destination row: the element size, or more (strided)
    uint32_t pad;
};
static_assert(sizeof(DeepDeliverTask) == 112, "uploaded as bytes");

// The window as the delivery task whose unit walks it shares: the destination and a format of deliver.h's with the same
// element size are all those walks look at.
DL_HD DeliverTask deep_window(const DeepDeliverTask &t) {
    DeliverTask w{};
    w.dst = t.dst; w.dst_pitch = t.dst_pitch; w.dst_step = t.dst_step;
    w.row0 = 0; w.row1 = int(t.rows); w.col0 = int(t.col0); w.col1 = int(t.col1);
    w.format = deep_dest_elem(t.format) == 4u ? uint32_t(kDeliverF32) : uint32_t(kDeliverF16);
    return w;
}
DL_HD unsigned long long deep_deliver_units(const DeepDeliverTask &t) { return deliver_task_units(deep_window(t)); }
DL_HD unsigned long long deep_deliver_chunks(const DeepDeliverTask &t) { return deliver_task_chunks(deep_window(t)); }

// What a task must satisfy before the kernel or the host walk may run it: a valid mode that an integer destination's
// signedness agrees with, a sound window that both planes' readable bytes hold, and a destination as deliver.h asks of it;
// an integer destination takes no scale and no bias.
inline bool deep_deliver_task_ok(const DeepDeliverTask &t) {
    if (!t.hi || !t.lo || !t.dst || t.format >= kDeepDestFormats || !deep_mode_valid(t.mode)) return false;
    if ((t.format == kDeepToU16 && (t.mode & kDeepSigned)) || (t.format == kDeepToI16 && !(t.mode & kDeepSigned))) return false;
    if (t.rows < 1 || t.src_pitch == 0 || t.col1 <= t.col0 || t.col1 > t.src_pitch) return false;
    const unsigned long long need = (unsigned long long)(t.rows - 1) * t.src_pitch + t.col1;
    if (need > t.hi_bytes || need > t.lo_bytes) return false;
    const uint32_t elem = deep_dest_elem(t.format);
    if (uintptr_t(t.dst) % elem || t.dst_pitch % elem || t.dst_step % elem || t.dst_step < elem || t.dst_step > kDeliverMaxStep || t.dst_pitch > kDeliverMaxPitch) return false;
    if (t.dst_pitch < (t.dst_step != elem ? (unsigned long long)(elem) : (unsigned long long)(t.col1 - t.col0) * elem)) return false;
    if (!(t.scale - t.scale == 0.0f) || !(t.bias - t.bias == 0.0f)) return false;          // NaN, infinite
    if (t.format <= kDeepToI16 && (t.scale != 1.0f || t.bias != 0.0f)) return false;
    return deep_deliver_chunks(t) < (1ull << 31) / kDeliverChunkUnits;
}
// Bytes of the destination the window spans: from the first byte written to the one behind the last.
inline unsigned long long deep_dest_extent(uint32_t rows, uint32_t cols, uint32_t format, unsigned long long pitch, unsigned long long step) {
    return (unsigned long long)(rows - 1) * pitch + (unsigned long long)(cols - 1) * step + deep_dest_elem(format);
}

// The host walk: every unit of the task, one after the other, element by element.  gate_hi_status / gate_lo_status stand for
// the gate records' status (the task's own gate pointers are not followed); pass 1 (kDone) for none.
inline void deep_deliver_host(const DeepDeliverTask &t, int gate_hi_status, int gate_lo_status) {
    const uint32_t elem = deep_dest_elem(t.format);
    const DeliverTask W = deep_window(t);
    const bool zero = t.zero != 0 || gate_hi_status != 1 || gate_lo_status != 1, strided = deliver_strided(W);
    const unsigned long long units = deliver_task_units(W);
    for (unsigned long long u = 0; u < units; u++) {
        const DeliverUnit U = strided ? deliver_strided_unit_of(W, uint32_t(u)) : deliver_unit_of(W, uint32_t(u));
        const uint8_t *h = t.hi + size_t(U.row) * t.src_pitch + t.col0, *l = t.lo + size_t(U.row) * t.src_pitch + t.col0;
        uint8_t *d = t.dst + size_t(U.row) * size_t(t.dst_pitch);
        for (uint32_t c = U.c_lo; c < U.c_hi; c++) {
            const uint32_t v = zero ? 0u : deep_value(deep_join(h[c], l[c], t.mode), t.mode, t.format, t.scale, t.bias);
            memcpy(d + size_t(c) * t.dst_step, &v, elem);            // (little endian: the low elem bytes)
        }
    }
}

// ---- the three costs of an image, and the range of its values ---------------------------------------------------------------------
struct DeepCostTask {
    const uint8_t *src;                    // element (0, 0); a multiple of 2
    unsigned long long pitch;              // bytes between source rows
    unsigned long long *sums;              // kDeepSums numbers: the costs of high, low, folded low -- zeroed before the launch, every tile
                                           // adds its share -- then min (0xFFFF before the launch) and max (0) of u
    uint32_t step;                         // bytes between neighbouring elements of a source row
    uint32_t rows, cols;
    uint32_t format;                       // kDeepU16 / kDeepI16
    uint32_t first_chunk;                  // tiles of the launch's tasks in front of this one
    uint32_t pad;
};
static_assert(sizeof(DeepCostTask) == 48, "uploaded as bytes");

CL_HD uint32_t deep_task_tiles(const DeepCostTask &t) { return cost_tiles(t.rows, t.cols); }

// The cost of pixel p with prediction pred, both 0..255: the residual is NOT wrapped (the head of this file says why).
CL_HD uint32_t deep_pixel_cost(uint32_t p, uint32_t pred) { return 2u * cost_bitlen(p > pred ? p - pred : pred - p) + 1u; }

// The three costs of the pixel at (y, x): u, w, n, nw are its own and its neighbours' 16-bit values (neighbours that do not
// exist are not looked at).
template <class Sum>
CL_HD void deep_pixel_costs(uint32_t u, uint32_t w, uint32_t n, uint32_t nw, uint32_t y, uint32_t x, Sum sums[kDeepParts]) {
    for (uint32_t k = 0; k < kDeepParts; k++)
        sums[k] += deep_pixel_cost(deep_part(u, k), cost_pred(deep_part(w, k), deep_part(n, k), deep_part(nw, k), y, x));
}

inline bool deep_cost_task_ok(const DeepCostTask &t, unsigned long long cap_bytes) {
    return deep_source_ok(t.src, t.pitch, t.step, t.rows, t.cols, t.format, cap_bytes) && t.sums != nullptr;
}

// The host walk: every tile of the task, one after the other, pixel by pixel; each element is read where it lies.
inline void deep_cost_host(const DeepCostTask &t) {
    unsigned long long sums[kDeepParts] = {}, lo = t.sums[3], hi = t.sums[4];
    cost_walk_tiles(t.rows, t.cols, [&](const CostTile &T) {
        cost_tile_pixels(T, [&](uint32_t y, uint32_t x) {
            uint32_t v[4];                                           // u, w, n, nw
            cost_neighbours([&](uint32_t yy, uint32_t xx) { return deep_u(cost_element(t.src, t.pitch, t.step, 2, yy, xx), t.format); }, y, x, v);
            deep_pixel_costs(v[0], v[1], v[2], v[3], y, x, sums);
            if (v[0] < lo) lo = v[0];
            if (v[0] > hi) hi = v[0];
        });
    });
    for (uint32_t k = 0; k < kDeepParts; k++) t.sums[k] += sums[k];
    t.sums[3] = lo; t.sums[4] = hi;
}

}  // namespace nblic
