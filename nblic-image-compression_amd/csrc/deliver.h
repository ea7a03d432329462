// deliver.h -- a window of a decoded plane into caller-owned memory, as pixels or as normalised floats: the task, the
// cut into units and the value of one element, shared by the host and the device.  The device kernel's lanes
// (serial_engine.hip, k_deliver) and the host-only deliver_host below call the same functions, so the unit walk is tested
// without a GPU (tests/test_deliver_host.py, tools/deliver_check.cpp).  The arithmetic and the roundings of deliver_value
// have two bodies: the host body is tested without a GPU (the same files, and tests/test_float_edges_host.py against an
// exact reference), the device body by tests/test_float_edges.py against the same reference.
//
// A UNIT is one lane's work: at most sixteen pixels of ONE row of the window, laid so that its first element's place in
// the destination row is a multiple of 16 bytes.  The destination row starts at any multiple of the element size, so the
// first unit of a row begins up to 16 / elem - 1 elements in front of the window (it has a head: fewer than sixteen
// pixels) and the last one may end behind it (a tail).  Every row has the same number of units -- the most any row
// alignment needs -- and a unit that no column falls into does nothing.
//
// A STRIDED task (dst_step > the element size: the elements of a destination row lie dst_step bytes apart, as the colours
// of an interleaved frame or the channels of a channels-last tensor do) knows no 16-byte rule: nothing is stored that is
// wider than one element.  Its unit is sixteen consecutive pixels of one row, counted from col0; element (r, c) of the
// window goes to dst + r * dst_pitch + c * dst_step and no other byte is written.
//
// A task with a REFERENCE undoes the reversible colour transform: its plane holds differences (R - G or B - G, + 128,
// mod 256; with per-frame colour modes, color_plan.h: any channel against the frame's base channel), the reference is the
// decoded plane of the base channel (G in the fixed transform) of the same frame -- same width, given from the window's first row on -- and
// the pixel of window position (r, c) is (src + ref - 128) & 255 of the two planes' bytes there; scale, bias and format
// apply to that pixel.  The three planes of a frame stand or fall together: each of its tasks names all three gates.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DL_HD __host__ __device__ inline
#else
#define DL_HD inline
#endif

namespace nblic {

struct SerialState;                                                  // serial_engine.h

enum : uint32_t { kDeliverU8 = 0, kDeliverF16 = 1, kDeliverBF16 = 2, kDeliverF32 = 3, kDeliverFormats = 4 };

struct DeliverTask {
    const uint8_t *src;                    // the plane: row 0, column 0 of what row0 .. col1 count from
    uint8_t *dst;                          // element (row0, col0) goes here; a multiple of the element size
    const SerialState *gate;               // not null: deliver only if its status is kDone, zeros otherwise
    unsigned long long src_bytes;          // readable bytes from src: nothing outside [src, src + src_bytes) is read
    unsigned long long dst_pitch;          // bytes between destination rows: a multiple of the element size; contiguous: >= cols * elem
    uint32_t src_pitch;                    // bytes between source rows: the image's width
    int row0, row1, col0, col1;            // the window [row0, row1) x [col0, col1)
    uint32_t format;                       // kDeliverU8 .. kDeliverF32
    float scale, bias;                     // float formats: float(px) * scale, rounded, + bias, rounded, then to the format
    uint32_t zero;                         // != 0: zero bytes instead of pixels
    uint32_t first_chunk;                  // chunks of the launch's tasks in front of this one
    uint32_t dst_step;                     // bytes between neighbouring elements of a destination row: the element size, or more (strided)
    uint32_t ref_pitch;                    // bytes between the reference's rows: the image's width (= src_pitch)
    const uint8_t *ref;                    // not null: the REFERENCE plane (below) at row row0, column 0
    unsigned long long ref_bytes;          // readable bytes from ref: nothing outside [ref, ref + ref_bytes) is read
    const SerialState *gate2, *gate3;      // further gates, like `gate`: every one that is not null must be kDone
};
static_assert(sizeof(DeliverTask) == 120, "uploaded as bytes");

constexpr uint32_t kDeliverUnitPixels = 16;
constexpr uint32_t kDeliverChunkUnits = 1024;                        // one workgroup: kIndexChunkBytes / 16 (serial_engine.hip asserts it)
constexpr uint32_t kDeliverMaxStep = 1u << 20;                       // bytes; the sources' limit (collect.h kCollectMaxStep)
constexpr unsigned long long kDeliverMaxPitch = 1ull << 40;

DL_HD uint32_t deliver_elem(uint32_t format) { return format == kDeliverU8 ? 1u : (format == kDeliverF32 ? 4u : 2u); }
// Units of one row: cols pixels behind a head gap of at most 16 / elem - 1 elements, sixteen to a unit.
DL_HD uint32_t deliver_row_units(uint32_t cols, uint32_t format) { return (cols + 16u / deliver_elem(format) - 1u + 15u) / 16u; }
// The same for a row whose elements lie `step` bytes apart: a strided row has no head gap.
DL_HD uint32_t deliver_row_units(uint32_t cols, uint32_t format, uint32_t step) {
    return step == deliver_elem(format) ? deliver_row_units(cols, format) : (cols + 15u) / 16u;
}
DL_HD bool deliver_strided(const DeliverTask &t) { return t.dst_step != deliver_elem(t.format); }
DL_HD unsigned long long deliver_task_units(const DeliverTask &t) {
    return (unsigned long long)(uint32_t(t.row1 - t.row0)) * deliver_row_units(uint32_t(t.col1 - t.col0), t.format, t.dst_step);
}
DL_HD unsigned long long deliver_task_chunks(const DeliverTask &t) { return (deliver_task_units(t) + kDeliverChunkUnits - 1) / kDeliverChunkUnits; }

// What unit u of a task covers: row `row` of the window and its columns [c_lo, c_hi) (counted from col0; empty when
// c_lo == c_hi).  The unit's sixteen element slots start at column c0 -- negative in a row's first unit when the row does
// not start at a multiple of 16 bytes -- and slot 0's destination byte, dst + row * dst_pitch + c0 * elem, IS such a multiple.
struct DeliverUnit { uint32_t row; int c0; uint32_t c_lo, c_hi; };
DL_HD DeliverUnit deliver_unit_of(const DeliverTask &t, uint32_t u) {
    const uint32_t cols = uint32_t(t.col1 - t.col0), per_row = deliver_row_units(cols, t.format), elem = deliver_elem(t.format);
    DeliverUnit U;
    U.row = u / per_row;
    const uint32_t j = u - U.row * per_row;
    const uint32_t lead = uint32_t((uintptr_t(t.dst) + (unsigned long long)(U.row) * t.dst_pitch) & 15u) / elem;
    U.c0 = int(16u * j) - int(lead);
    U.c_lo = U.c0 < 0 ? 0u : uint32_t(U.c0);
    U.c_hi = uint32_t(U.c0 + 16) < cols ? uint32_t(U.c0 + 16) : cols;
    if (U.c_lo > U.c_hi) U.c_lo = U.c_hi;
    return U;
}

// Unit u of a strided task: columns [16 j, 16 j + 16) of its row, cut at the window's end.  No head: c0 is never negative.
DL_HD DeliverUnit deliver_strided_unit_of(const DeliverTask &t, uint32_t u) {
    const uint32_t cols = uint32_t(t.col1 - t.col0), per_row = (cols + 15u) / 16u;
    DeliverUnit U;
    U.row = u / per_row;
    U.c_lo = 16u * (u - U.row * per_row);
    U.c0 = int(U.c_lo);
    U.c_hi = U.c_lo + 16u < cols ? U.c_lo + 16u : cols;
    return U;
}

// float -> binary16 / bfloat16 bits, round to nearest even.  Integer arithmetic: the host's reference for what the
// device's conversion instructions deliver (tests/test_decode_to_device.py compares the two).
DL_HD uint32_t deliver_f16_bits(uint32_t f) {
    const uint32_t sign = (f >> 16) & 0x8000u, a = f & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return sign | (a > 0x7F800000u ? 0x7E00u : 0x7C00u);
    if (a >= 0x477FF000u) return sign | 0x7C00u;                      // 65520 and above round to infinity
    if (a >= 0x38800000u) {                                           // a normal half: rebias, round the 13 bits that go
        const uint32_t m = a - 0x38000000u;
        return sign | ((m + 0x0FFFu + ((m >> 13) & 1u)) >> 13);
    }
    if (a <= 0x33000000u) return sign;                                // 2^-25 and below: zero (the tie goes to even)
    const uint32_t shift = 126u - (a >> 23), m = (a & 0x007FFFFFu) | 0x00800000u;      // a subnormal half: m * 2^-shift units of 2^-24
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) r++;
    return sign | r;
}
DL_HD uint32_t deliver_bf16_bits(uint32_t f) {
    if ((f & 0x7FFFFFFFu) > 0x7F800000u) return (f >> 16) | 0x0040u;
    return (f + 0x7FFFu + ((f >> 16) & 1u)) >> 16;
}

// One element's bits (in the low elem bytes): the pixel itself, or float(px) * scale + bias with both operations
// rounded to float -- never fused -- and the result rounded to nearest even into the format.
DL_HD uint32_t deliver_value(uint32_t px, uint32_t format, float scale, float bias) {
    if (format == kDeliverU8) return px;
#if defined(__HIP_DEVICE_COMPILE__)
    const float v = __fadd_rn(__fmul_rn(float(px), scale), bias);
    if (format == kDeliverF32) return __float_as_uint(v);
    if (format == kDeliverF16) return uint32_t(__builtin_bit_cast(unsigned short, static_cast<_Float16>(v)));
    return deliver_bf16_bits(__float_as_uint(v));
#else
    volatile float prod = float(px) * scale;                         // (volatile: two roundings whatever the compiler's contraction rule)
    const float v = prod + bias;
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return format == kDeliverF32 ? bits : (format == kDeliverF16 ? deliver_f16_bits(bits) : deliver_bf16_bits(bits));
#endif
}

// The pixel of a task with a reference: px and ref are the two planes' bytes.
DL_HD uint32_t deliver_rct(uint32_t px, uint32_t ref) { return (px + ref - 128u) & 255u; }

// What a task must satisfy before a kernel or the host walk may run it: a sound window inside a plane of src_rows rows
// that the readable bytes hold, a destination pitch, step and pointer that are multiples of the element size and not
// below it, contiguous rows that do not overlap (a strided task may have any pitch: a transposed view is one), no more
// units than 32 bits count, and uint8 as a plain copy.  A reference has the plane's width as its pitch and holds the
// window's rows inside its readable bytes.
inline bool deliver_task_ok(const DeliverTask &t, uint32_t src_rows) {
    if (!t.src || !t.dst || t.format >= kDeliverFormats || t.src_pitch == 0) return false;
    if (t.row0 < 0 || t.row1 <= t.row0 || uint32_t(t.row1) > src_rows || t.col0 < 0 || t.col1 <= t.col0 || uint32_t(t.col1) > t.src_pitch) return false;
    if ((unsigned long long)(src_rows) * t.src_pitch > t.src_bytes) return false;
    if (t.ref && (t.ref_pitch != t.src_pitch || (unsigned long long)(uint32_t(t.row1 - t.row0 - 1)) * t.ref_pitch + uint32_t(t.col1) > t.ref_bytes)) return false;
    const uint32_t elem = deliver_elem(t.format);
    if (uintptr_t(t.dst) % elem || t.dst_pitch % elem || t.dst_step % elem || t.dst_step < elem || t.dst_step > kDeliverMaxStep || t.dst_pitch > kDeliverMaxPitch) return false;
    if (t.dst_pitch < (deliver_strided(t) ? (unsigned long long)(elem) : (unsigned long long)(uint32_t(t.col1 - t.col0)) * elem)) return false;
    if (!(t.scale - t.scale == 0.0f) || !(t.bias - t.bias == 0.0f)) return false;          // NaN, infinite
    if (t.format == kDeliverU8 && (t.scale != 1.0f || t.bias != 0.0f)) return false;
    return deliver_task_chunks(t) < (1ull << 31) / kDeliverChunkUnits;
}

// Bytes of the destination a window of rows x cols spans: the last row is not padded to the pitch.
inline unsigned long long deliver_extent(uint32_t rows, uint32_t cols, uint32_t format, unsigned long long pitch) {
    return (unsigned long long)(rows - 1) * pitch + (unsigned long long)(cols) * deliver_elem(format);
}
// The same with the row's elements `step` bytes apart: from the first byte written to the one behind the last.
inline unsigned long long deliver_extent(uint32_t rows, uint32_t cols, uint32_t format, unsigned long long pitch, unsigned long long step) {
    return (unsigned long long)(rows - 1) * pitch + (unsigned long long)(cols - 1) * step + deliver_elem(format);
}

// The host walk: every unit of the task, one after the other, element by element.  `gate_status` stands for the gate
// record's status (the task's own gate pointers are not followed); pass 1 (kDone) for none.  gate2_status / gate3_status:
// the same for the second and the third gate.
inline void deliver_host(const DeliverTask &t, int gate_status, int gate2_status = 1, int gate3_status = 1) {
    const uint32_t elem = deliver_elem(t.format);
    const bool zero = t.zero != 0 || gate_status != 1 || gate2_status != 1 || gate3_status != 1;
    const unsigned long long units = deliver_task_units(t);
    const bool strided = deliver_strided(t);
    for (unsigned long long u = 0; u < units; u++) {
        const DeliverUnit U = strided ? deliver_strided_unit_of(t, uint32_t(u)) : deliver_unit_of(t, uint32_t(u));
        const uint8_t *s = t.src + size_t(uint32_t(t.row0) + U.row) * t.src_pitch + uint32_t(t.col0);
        const uint8_t *r = t.ref ? t.ref + size_t(U.row) * t.ref_pitch + uint32_t(t.col0) : nullptr;
        uint8_t *d = t.dst + size_t(U.row) * size_t(t.dst_pitch);
        for (uint32_t c = U.c_lo; c < U.c_hi; c++) {
            const uint32_t v = zero ? 0u : deliver_value(r ? deliver_rct(s[c], r[c]) : uint32_t(s[c]), t.format, t.scale, t.bias);
            memcpy(d + size_t(c) * t.dst_step, &v, elem);            // (little endian: the low elem bytes)
        }
    }
}

}  // namespace nblic
