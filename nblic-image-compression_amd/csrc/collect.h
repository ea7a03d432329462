// collect.h -- an image out of caller-owned memory into the encoders' contiguous uint8 plane: any pitch, any step between
// the pixels of a row, pixels or floats that are quantised on the way.  The task, the cut into units and the pixel of one
// source element, shared by the host and the device: the device kernel's lanes (serial_engine.hip, k_collect) and the
// host-only collect_host below call the same functions, so the unit walk is tested without a GPU
// (tests/test_collect_host.py, tools/collect_check.cpp).  The arithmetic and the roundings of collect_value have two
// bodies: the host body is tested without a GPU (the same files, and tests/test_float_edges_host.py against an exact
// reference), the device body by tests/test_float_edges.py against the same reference.  The counterpart of deliver.h.
//
// The collected plane is contiguous (row r starts at byte r * cols) and its base is a multiple of 16 bytes, so a UNIT --
// one lane's work -- is sixteen consecutive bytes of the FLAT plane at a multiple of 16: it runs across row ends whenever
// cols is no multiple of 16.  A task covers the pixels [px0, px1) of the flat plane (a whole image: [0, rows * cols); the
// indexed batch: the rows of one band), so its first and its last unit may be shorter than sixteen pixels.
//
// A task with a REFERENCE writes a difference plane of a colour frame whose three colours are three sources (R - G and
// B - G of the fixed transform; any channel against the base channel of the frame's colour mode, color_plan.h): the
// reference is a second source of the same rows x cols, format, scale and bias -- the caller's base channel, G in the
// fixed transform -- with a pitch and a step of its own, and pixel (row, col) is (own - ref + 128) & 255 of the two
// elements there, each quantised as without a reference.  The reference is read where the caller keeps it, never from
// another task's plane, so the tasks of a launch stay independent of each other.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CL_HD __host__ __device__ inline
#else
#define CL_HD inline
#endif

namespace nblic {

enum : uint32_t { kCollectU8 = 0, kCollectF16 = 1, kCollectBF16 = 2, kCollectF32 = 3, kCollectFormats = 4 };   // the delivery's numbers

struct CollectTask {
    const uint8_t *src;                    // element (0, 0) of the image; a multiple of the element size
    uint8_t *dst;                          // pixel 0 of the flat plane; a multiple of 16
    unsigned long long pitch;              // bytes between source rows: a multiple of the element size
    uint32_t step;                         // bytes between neighbouring pixels of a source row: a multiple of the element size
    uint32_t rows, cols;                   // the image
    uint32_t px0, px1;                     // the pixels of the flat plane this task writes: [px0, px1), px1 <= rows * cols
    uint32_t format;                       // kCollectU8 .. kCollectF32
    float scale, bias;                     // float formats: float(x) * scale, rounded, + bias, rounded, then to a pixel
    uint32_t first_chunk;                  // chunks of the launch's tasks in front of this one
    uint32_t ref_step;                     // bytes between neighbouring pixels of a row of the reference
    const uint8_t *ref;                    // not null: element (0, 0) of the REFERENCE source (below); a multiple of the element size
    unsigned long long ref_pitch;          // bytes between the reference's rows
};
static_assert(sizeof(CollectTask) == 80, "uploaded as bytes");

constexpr uint32_t kCollectUnitPixels = 16;
constexpr uint32_t kCollectChunkUnits = 1024;                        // one workgroup: kIndexChunkBytes / 16 (serial_engine.hip asserts it)
constexpr uint32_t kCollectMaxSide = 65535;                          // NBLIC_MAX_HEIGHT / _WIDTH: rows * cols fits 32 bits
constexpr uint32_t kCollectMaxStep = 1u << 20;
constexpr unsigned long long kCollectMaxPitch = 1ull << 40;

CL_HD uint32_t collect_elem(uint32_t format) { return format == kCollectU8 ? 1u : (format == kCollectF32 ? 4u : 2u); }
CL_HD uint32_t collect_task_units(const CollectTask &t) { return (t.px1 + 15u) / 16u - t.px0 / 16u; }      // (px1 <= 65535^2: no overflow)
CL_HD uint32_t collect_task_chunks(const CollectTask &t) { return (collect_task_units(t) + kCollectChunkUnits - 1) / kCollectChunkUnits; }

// What unit u of a task covers: the pixels [p_lo, p_hi) of the flat plane, inside the sixteen that start at p0 (a multiple
// of 16: byte dst + p0 is the unit's aligned place).
struct CollectUnit { uint32_t p0, p_lo, p_hi; };
CL_HD CollectUnit collect_unit_of(const CollectTask &t, uint32_t u) {
    CollectUnit U;
    U.p0 = (t.px0 / 16u + u) * 16u;
    U.p_lo = U.p0 < t.px0 ? t.px0 : U.p0;
    U.p_hi = t.px1 - U.p0 > 16u ? U.p0 + 16u : t.px1;                // (p0 < px1 for every unit of the task)
    return U;
}

// Byte offset of the source element of image position (row, col).
CL_HD unsigned long long collect_src_at(const CollectTask &t, uint32_t row, uint32_t col) {
    return (unsigned long long)(row) * t.pitch + (unsigned long long)(col) * t.step;
}

// binary16 / bfloat16 bits -> float bits, exact.
CL_HD uint32_t collect_f16_to_f32_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 0x1Fu) return sign | 0x7F800000u | (m << 13);
    if (e != 0) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0) return sign;
    uint32_t k = 0, mm = m;                                          // a subnormal half: m * 2^-24
    while (!(mm & 0x400u)) { mm <<= 1; k++; }
    return sign | ((113u - k) << 23) | ((mm & 0x3FFu) << 13);
}

CL_HD unsigned long long collect_ref_at(const CollectTask &t, uint32_t row, uint32_t col) {
    return (unsigned long long)(row) * t.ref_pitch + (unsigned long long)(col) * t.ref_step;
}

// The pixel of one source element whose bits are in the low elem bytes of x: the element itself, or
// float(x) * scale + bias with both operations rounded to float -- never fused -- NaN to 0, everything else clamped to
// [0, 255] and rounded to nearest, ties to even.
CL_HD uint32_t collect_value(uint32_t x, uint32_t format, float scale, float bias) {
    if (format == kCollectU8) return x & 0xFFu;
    const uint32_t bits = format == kCollectF32 ? x : (format == kCollectBF16 ? (x & 0xFFFFu) << 16 : collect_f16_to_f32_bits(x & 0xFFFFu));
#if defined(__HIP_DEVICE_COMPILE__)
    const float v = __fadd_rn(__fmul_rn(__uint_as_float(bits), scale), bias);
    if (!(v > 0.0f)) return 0u;                                      // NaN, -inf, negatives, both zeros
    if (v >= 255.0f) return 255u;
    return uint32_t(__float2int_rn(v));
#else
    float f;
    memcpy(&f, &bits, 4);
    volatile float prod = f * scale;                                 // (volatile: two roundings whatever the compiler's contraction rule)
    const float v = prod + bias;
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    const uint32_t i = uint32_t(v);                                  // v in (0, 255): truncates
    const float frac = v - float(i);                                 // exact
    return frac > 0.5f || (frac == 0.5f && (i & 1u)) ? i + 1u : i;
#endif
}

// The pixel of a task with a reference: own and ref are collect_value of the two elements.
CL_HD uint32_t collect_rct(uint32_t own, uint32_t ref) { return (own - ref + 128u) & 255u; }

// Bytes from src that an image of rows x cols spans: its last element ends it.
inline unsigned long long collect_extent(uint32_t rows, uint32_t cols, uint32_t format, unsigned long long pitch, unsigned long long step) {
    return (unsigned long long)(rows - 1) * pitch + (unsigned long long)(cols - 1) * step + collect_elem(format);
}

// What a task's SOURCE must satisfy: an image the encoders take, a pointer, pitch and step that are multiples of the
// element size and not below it, a step and a pitch within their limits, an extent that cap_bytes holds, finite scale
// and bias, and uint8 as a plain copy.  A reference is a source of its own: the same rules for its pointer, pitch and
// step, and its extent inside ref_cap_bytes.
inline bool collect_source_ok(const CollectTask &t, unsigned long long cap_bytes, unsigned long long ref_cap_bytes = 0) {
    if (!t.src || t.format >= kCollectFormats) return false;
    if (t.rows < 1 || t.cols < 1 || t.rows > kCollectMaxSide || t.cols > kCollectMaxSide) return false;
    const uint32_t elem = collect_elem(t.format);
    if (uintptr_t(t.src) % elem || t.pitch % elem || t.step % elem || t.step < elem || t.pitch < elem) return false;
    if (t.step > kCollectMaxStep || t.pitch > kCollectMaxPitch) return false;
    if (collect_extent(t.rows, t.cols, t.format, t.pitch, t.step) > cap_bytes) return false;
    if (t.ref) {
        if (uintptr_t(t.ref) % elem || t.ref_pitch % elem || t.ref_step % elem || t.ref_step < elem || t.ref_pitch < elem) return false;
        if (t.ref_step > kCollectMaxStep || t.ref_pitch > kCollectMaxPitch) return false;
        if (collect_extent(t.rows, t.cols, t.format, t.ref_pitch, t.ref_step) > ref_cap_bytes) return false;
    }
    if (!(t.scale - t.scale == 0.0f) || !(t.bias - t.bias == 0.0f)) return false;          // NaN, infinite
    return t.format != kCollectU8 || (t.scale == 1.0f && t.bias == 0.0f);
}
// What a task must satisfy before a kernel or the host walk may run it: such a source, a pixel range inside the plane
// and an aligned destination.
inline bool collect_task_ok(const CollectTask &t, unsigned long long cap_bytes, unsigned long long ref_cap_bytes = 0) {
    return collect_source_ok(t, cap_bytes, ref_cap_bytes) && t.dst && uintptr_t(t.dst) % 16 == 0 && t.px0 < t.px1 && t.px1 <= t.rows * t.cols;
}

// A source that is the collected plane already: nothing has to run for it.
inline bool collect_in_place(uint32_t format, unsigned long long pitch, unsigned long long step, uint32_t cols) {
    return format == kCollectU8 && step == 1 && pitch == cols;
}

// The host walk: every unit of the task, one after the other, element by element.
inline void collect_host(const CollectTask &t) {
    const uint32_t elem = collect_elem(t.format), units = collect_task_units(t);
    for (uint32_t u = 0; u < units; u++) {
        const CollectUnit U = collect_unit_of(t, u);
        uint32_t row = U.p_lo / t.cols, col = U.p_lo - row * t.cols;
        for (uint32_t p = U.p_lo; p < U.p_hi; p++) {
            uint32_t x = 0;
            memcpy(&x, t.src + collect_src_at(t, row, col), elem);   // (little endian: the low elem bytes)
            uint32_t v = collect_value(x, t.format, t.scale, t.bias);
            if (t.ref) {
                uint32_t y = 0;
                memcpy(&y, t.ref + collect_ref_at(t, row, col), elem);
                v = collect_rct(v, collect_value(y, t.format, t.scale, t.bias));
            }
            t.dst[p] = uint8_t(v);
            if (++col == t.cols) { col = 0; row++; }
        }
    }
}

}  // namespace nblic
