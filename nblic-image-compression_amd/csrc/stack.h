// stack.h -- slice stacks: the images of a call as stacks of `depth` slices (the slices of a volume, the frames of a static
// camera), a slice coded as it is or as its difference against the slice before it.  The mode byte, the walk over a run of
// differences, the byte arithmetic, the delivery of a run and the two costs of a slice, shared by the host and the device:
// the kernels' lanes (serial_engine.hip, k_deliver_stack and k_stack_cost) and the host-only stack_deliver_host and
// stack_cost_host below call the same functions, so the walks and the arithmetic are tested without a GPU
// (tests/test_stack_host.py, tools/stack_check.cpp).  Built on collect.h, deliver.h and color_plan.h (a slice's cost is a colour
// plane's: color_pixel_cost); the tile geometry, the MED prediction and the host's tile walk live in cost_tile.h.
//
// THE STACK.  A call has a depth D >= 1 and n_images % D == 0; image s * D + d is slice d of stack s (n-major, as a
// [N, D, H, W] tensor is read).  The slices of a stack have one size.
//
// THE SLICE MODE, one byte per image.  0: a KEY slice, coded as it is.  1: a DELTA slice, coded as
// (x_d - x_{d-1} + 128) mod 256, both the pixels k_collect would write.  Slice 0 of every stack is a key.  Every other byte is
// invalid; 0xFF is what the plan gives the slices of a stack it refuses.
//
// A RUN is a key slice and the delta slices that follow it.  Restoring is x_d = (t_d + x_{d-1} - 128) mod 256 along the run:
// a per-pixel running sum, which ONE lane carries in registers from the key to the run's last slice -- no task waits for
// another task's output.  The encode side has no chain at all: the reference of slice d is the caller's SOURCE of slice
// d - 1 (CollectTask::ref).  The streams are ordinary streams of those planes; nothing in them names the mode.
#pragma once
#include "deliver.h"
#include "color_plan.h"

namespace nblic {

enum : uint32_t { kStackKey = 0, kStackDelta = 1, kStackRefused = 0xFF };

// ---- the mode bytes ------------------------------------------------------------------------------------------------------------
inline bool stack_mode_valid(uint32_t m) { return m == kStackKey || m == kStackDelta; }
// The bytes of a call: a depth that divides the count, valid bytes, and a key at the head of every stack.
inline bool stack_modes_ok(long n, long depth, const uint8_t *modes) {
    if (n < 0 || depth < 1 || n % depth != 0 || !modes) return false;
    for (long i = 0; i < n; i++)
        if (!stack_mode_valid(modes[i]) || (i % depth == 0 && modes[i] != kStackKey)) return false;
    return true;
}
// The run walk: slices [d, d + stack_run_len) of a stack are the run whose key is slice d.
inline uint32_t stack_run_len(const uint8_t *stack_modes, uint32_t d, uint32_t depth) {
    uint32_t e = d + 1;
    while (e < depth && stack_modes[e] == kStackDelta) e++;
    return e - d;
}
// THE RULE (part of the interface: two builds plan alike): a slice is a delta iff 64 * delta < 63 * intra -- the colour
// plan's margin; equality is a key.
inline uint8_t stack_choose(unsigned long long intra, unsigned long long delta) {
    return (unsigned __int128)(delta) * 64u < (unsigned __int128)(intra) * 63u ? uint8_t(kStackDelta) : uint8_t(kStackKey);
}

// The mode the plan gives slice d of a stack from its two costs: slice 0, and with key_every = K > 0 every slice with
// d % K == 0, is a key whatever the costs say.
inline uint8_t stack_slice_mode(uint32_t d, uint32_t key_every, unsigned long long intra, unsigned long long delta) {
    return d == 0 || (key_every > 0 && d % key_every == 0) ? uint8_t(kStackKey) : stack_choose(intra, delta);
}

// ---- the byte arithmetic -------------------------------------------------------------------------------------------------------
CL_HD uint32_t stack_delta(uint32_t own, uint32_t prev) { return collect_rct(own, prev); }          // (own - prev + 128) & 255
CL_HD uint32_t stack_restore(uint32_t t, uint32_t prev) { return deliver_rct(t, prev); }            // (t + prev - 128) & 255
// The same for the four bytes of a word at once: a bytewise add without carries between the bytes, then - 128.
CL_HD uint32_t stack_restore4(uint32_t t, uint32_t prev) {
    return (((t & 0x7F7F7F7Fu) + (prev & 0x7F7F7F7Fu)) ^ ((t ^ prev) & 0x80808080u)) ^ 0x80808080u;
}

// ---- the delivery of a run -----------------------------------------------------------------------------------------------------
// One slice of a run: its decoded plane and where its window goes.
struct StackSlice {
    const uint8_t *src;                    // the plane at the window's FIRST row, column 0 (the planes of a run may start at different rows)
    unsigned long long src_bytes;          // readable bytes from src: nothing outside [src, src + src_bytes) is read
    const SerialState *gate;               // not null: the plane counts only if its status is kDone
    uint8_t *dst;                          // element (0, 0) of the window goes here; null: the slice is not delivered (a reference only)
    unsigned long long dst_pitch;          // bytes between destination rows
    uint32_t dst_step;                     // bytes between neighbouring elements of a destination row: the element size, or more
    float scale, bias;                     // float formats, as deliver.h
    uint32_t zero;                         // != 0: the plane is known to be bad -- as a gate that is not kDone
};
static_assert(sizeof(StackSlice) == 56, "uploaded as bytes");

// One run with its slices in a second table: slices[first_slice .. first_slice + count).
struct StackDeliverTask {
    uint32_t first_slice, count;
    uint32_t rows;                         // of the window
    uint32_t col0, col1;                   // its columns [col0, col1) of the planes
    uint32_t src_pitch;                    // bytes between the rows of every plane: the image's width
    uint32_t format;                       // kDeliverU8 .. kDeliverF32, of every destination
    uint32_t first_chunk;                  // chunks of the launch's tasks in front of this one
};
static_assert(sizeof(StackDeliverTask) == 32, "uploaded as bytes");

// The window as the delivery task whose strided unit walk the run shares: a unit is sixteen consecutive window pixels of one
// row, counted from col0 (deliver.h deliver_strided_unit_of).
DL_HD DeliverTask stack_window(const StackDeliverTask &t) {
    DeliverTask w{};
    w.row0 = 0; w.row1 = int(t.rows); w.col0 = int(t.col0); w.col1 = int(t.col1); w.format = t.format;
    return w;
}
DL_HD unsigned long long stack_task_units(const StackDeliverTask &t) { return (unsigned long long)(t.rows) * ((t.col1 - t.col0 + 15u) / 16u); }
DL_HD unsigned long long stack_task_chunks(const StackDeliverTask &t) { return (stack_task_units(t) + kDeliverChunkUnits - 1) / kDeliverChunkUnits; }

// May a lane store a unit's sixteen elements of this slice as whole 16-byte blocks?  A contiguous destination, a full unit,
// and slot 0 at a multiple of 16 bytes; a strided destination never gets a wide store.
DL_HD bool stack_wide_store(const StackSlice &s, uint32_t elem, uint32_t row, uint32_t c_lo, uint32_t c_hi) {
    return s.dst_step == elem && c_hi - c_lo == 16u && ((uintptr_t(s.dst) + (unsigned long long)(row) * s.dst_pitch + (unsigned long long)(c_lo) * elem) & 15u) == 0;
}

// What a task must satisfy before the kernel or the host walk may run it: a sound window that every plane's readable bytes
// hold, and destinations (where there is one) as deliver.h asks of them.
inline bool stack_task_ok(const StackDeliverTask &t, const StackSlice *slices) {
    if (!slices || t.count < 1 || t.format >= kDeliverFormats || t.rows < 1 || t.src_pitch == 0 || t.col1 <= t.col0 || t.col1 > t.src_pitch) return false;
    const uint32_t elem = deliver_elem(t.format), cols = t.col1 - t.col0;
    for (uint32_t d = 0; d < t.count; d++) {
        const StackSlice &s = slices[t.first_slice + d];
        if (!s.src || (unsigned long long)(t.rows - 1) * t.src_pitch + t.col1 > s.src_bytes) return false;
        if (!s.dst) continue;
        if (uintptr_t(s.dst) % elem || s.dst_pitch % elem || s.dst_step % elem || s.dst_step < elem || s.dst_step > kDeliverMaxStep || s.dst_pitch > kDeliverMaxPitch) return false;
        if (s.dst_pitch < (s.dst_step != elem ? (unsigned long long)(elem) : (unsigned long long)(cols) * elem)) return false;
        if (!(s.scale - s.scale == 0.0f) || !(s.bias - s.bias == 0.0f)) return false;
        if (t.format == kDeliverU8 && (s.scale != 1.0f || s.bias != 0.0f)) return false;
    }
    return stack_task_chunks(t) < (1ull << 31) / kDeliverChunkUnits;
}

// The host walk: every unit of the task, one after the other; the run's slices for each, byte by byte.  gate_status[d] stands
// for the gate record of slice d of the task (the slices' own gate pointers are not followed); 1 (kDone) for none.  Slice d is
// delivered only if every plane from the key through d counts; otherwise d and every later slice get zeros.
inline void stack_deliver_host(const StackDeliverTask &t, const StackSlice *slices, const int *gate_status) {
    const uint32_t elem = deliver_elem(t.format);
    const DeliverTask W = stack_window(t);
    const unsigned long long units = stack_task_units(t);
    for (unsigned long long u = 0; u < units; u++) {
        const DeliverUnit U = deliver_strided_unit_of(W, uint32_t(u));
        uint8_t run[16] = {};
        bool ok = true;
        for (uint32_t d = 0; d < t.count; d++) {
            const StackSlice &s = slices[t.first_slice + d];
            ok = ok && !s.zero && (!gate_status || gate_status[d] == 1);
            if (ok) {
                const uint8_t *p = s.src + size_t(U.row) * t.src_pitch + t.col0;
                for (uint32_t c = U.c_lo; c < U.c_hi; c++) run[c - U.c_lo] = uint8_t(d == 0 ? uint32_t(p[c]) : stack_restore(p[c], run[c - U.c_lo]));
            }
            if (!s.dst) continue;
            uint8_t *o = s.dst + size_t(U.row) * size_t(s.dst_pitch);
            for (uint32_t c = U.c_lo; c < U.c_hi; c++) {
                const uint32_t v = ok ? deliver_value(run[c - U.c_lo], t.format, s.scale, s.bias) : 0u;
                memcpy(o + size_t(c) * s.dst_step, &v, elem);        // (little endian: the low elem bytes)
            }
        }
    }
}

// ---- the two costs of a slice --------------------------------------------------------------------------------------------------
// THE COSTS of slice d (color_plan.h's cost: MED residual, 2 * bitlen(|e|) + 1 a pixel): of the slice itself (INTRA), and of
// its difference plane against slice d - 1 (DELTA; 0 for slice 0).  The delta is taken against the SOURCE of d - 1 whatever
// that slice's own mode is, so the choices of a stack's slices are independent of each other.
struct StackCostSlice {
    const uint8_t *src;                    // element (0, 0); a multiple of the element size
    unsigned long long pitch;              // bytes between source rows
    uint32_t step;                         // bytes between neighbouring pixels of a source row
    uint32_t pad;
};
static_assert(sizeof(StackCostSlice) == 24, "uploaded as bytes");

// One stack: count sources of rows x cols in one format, scale and bias, in a second table.
struct StackCostTask {
    unsigned long long *costs;             // two sums per slice (intra, delta), zeroed before the launch: every tile adds its share
    uint32_t first_slice, count;
    uint32_t rows, cols;
    uint32_t format;                       // kCollectU8 .. kCollectF32
    float scale, bias;
    uint32_t first_chunk;                  // tiles of the launch's tasks in front of this one
};
static_assert(sizeof(StackCostTask) == 40, "uploaded as bytes");

CL_HD uint32_t stack_task_tiles(const StackCostTask &t) { return cost_tiles(t.rows, t.cols); }

// Slice d's source as the collect task whose loader and checks it shares (all but dst and the pixel range).
CL_HD CollectTask stack_source(const StackCostTask &t, const StackCostSlice &s) {
    CollectTask c{};
    c.src = s.src; c.pitch = s.pitch; c.step = s.step;
    c.rows = t.rows; c.cols = t.cols; c.px0 = 0; c.px1 = t.rows * t.cols;
    c.format = t.format; c.scale = t.scale; c.bias = t.bias;
    return c;
}

// The two costs of the pixel at (y, x): p, w, n, nw are its own and its neighbours' pixels in the slice, and pp, pw, pn, pnw
// those of the slice before (not looked at when there is none).
template <class Sum>
CL_HD void stack_pixel_costs(uint32_t p, uint32_t w, uint32_t n, uint32_t nw, uint32_t pp, uint32_t pw, uint32_t pn, uint32_t pnw, bool has_prev,
                             uint32_t y, uint32_t x, Sum &intra, Sum &delta) {
    intra += color_pixel_cost(p, cost_pred(w, n, nw, y, x));
    if (has_prev) delta += color_pixel_cost(stack_delta(p, pp), cost_pred(stack_delta(w, pw), stack_delta(n, pn), stack_delta(nw, pnw), y, x));
}

inline bool stack_cost_task_ok(const StackCostTask &t, const StackCostSlice *slices, const unsigned long long *caps) {
    if (!slices || !caps || t.count < 1 || !t.costs) return false;
    for (uint32_t d = 0; d < t.count; d++)
        if (!collect_source_ok(stack_source(t, slices[t.first_slice + d]), caps[d])) return false;
    return true;
}

// The host walk: every tile of the task, one after the other; the stack's slices for each, pixel by pixel; each element is
// read where it lies.
inline void stack_cost_host(const StackCostTask &t, const StackCostSlice *slices) {
    const uint32_t elem = collect_elem(t.format);
    cost_walk_tiles(t.rows, t.cols, [&](const CostTile &T) {
        for (uint32_t d = 0; d < t.count; d++) {
            unsigned long long intra = 0, delta = 0;
            cost_tile_pixels(T, [&](uint32_t y, uint32_t x) {
                uint32_t v[2][4] = {};                               // [this slice, the one before][p, w, n, nw]
                for (uint32_t b = 0; b < (d ? 2u : 1u); b++) {
                    const StackCostSlice &s = slices[t.first_slice + d - b];
                    cost_neighbours([&](uint32_t yy, uint32_t xx) { return collect_value(cost_element(s.src, s.pitch, s.step, elem, yy, xx), t.format, t.scale, t.bias); }, y, x, v[b]);
                }
                stack_pixel_costs(v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3], d > 0, y, x, intra, delta);
            });
            t.costs[2 * d] += intra; t.costs[2 * d + 1] += delta;
        }
    });
}

}  // namespace nblic
