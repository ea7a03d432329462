// color_plan.h -- which colour transform suits a frame: the per-frame colour MODE byte, the COST of a frame's nine candidate
// planes, and the rule that chooses a mode from those costs.  The task, the cut into tiles and the arithmetic of one pixel are
// shared by the host and the device: the kernel's lanes (serial_engine.hip, k_color_cost) and the host-only color_cost_host
// below call the same functions, so the tile walk and the arithmetic are tested without a GPU
// (tests/test_color_plan_host.py, tools/color_plan_check.cpp).  Built on collect.h: a source element becomes a pixel by
// collect_value, so the costs are those of exactly the planes k_collect would write.  The tile geometry, the MED prediction,
// the bit length and the host's tile walk live in cost_tile.h, which stack.h and deep.h share.
//
// THE MODE.  Bits 0..1: the base channel b (0 = R, 1 = G, 2 = B).  Bit 2: the lower-numbered of the two other channels is
// coded as (c - b + 128) mod 256.  Bit 3: the same for the higher-numbered one.  The base, and a channel whose bit is
// clear, are coded as they are.  Valid: 0 (plain -- the only spelling of "no difference") and b | 4, b | 8, b | 12 for
// b = 0..2: ten modes.  0x0D (base G, both differences) is the fixed transform of JPEG-LS.
//
// THE COST of a plane is the sum over its pixels of 2 * bitlen(|e|) + 1, e = (p - pred) wrapped to -128..127, pred the MED
// prediction from W, N, NW of the same plane (row 0: W; column 0: N; (0, 0): 128): the length of an Elias-gamma-like code
// of the residual, integers only.  The nine planes of a frame, in the order of the cost table: R, G, B, R-G, R-B, G-R, G-B,
// B-R, B-G, a difference X-Y being (X - Y + 128) & 255 pixel by pixel.  Sums are unsigned 64-bit and depend on nothing but
// the pixels: integer adds commute.
#pragma once
#include "collect.h"
#include "cost_tile.h"

namespace nblic {

enum : uint32_t { kColorPlain = 0, kColorRct = 0x0D, kColorRefused = 0xFF };
constexpr uint32_t kColorCosts = 9;

// One frame: three sources of rows x cols in one format, scale and bias, and where its nine sums go.
struct ColorCostTask {
    const uint8_t *src[3];                 // element (0, 0) of R, G, B; multiples of the element size
    unsigned long long pitch[3];           // bytes between source rows
    uint32_t step[3];                      // bytes between neighbouring pixels of a source row
    uint32_t rows, cols;
    uint32_t format;                       // kCollectU8 .. kCollectF32
    float scale, bias;
    uint32_t first_chunk;                  // tiles of the launch's tasks in front of this one
    uint32_t pad;
    unsigned long long *costs;             // nine sums, zeroed before the launch: every tile adds its share
};
static_assert(sizeof(ColorCostTask) == 96, "uploaded as bytes");

CL_HD uint32_t color_task_tiles(const ColorCostTask &t) { return cost_tiles(t.rows, t.cols); }
CL_HD CostTile color_tile_of(const ColorCostTask &t, uint32_t k) { return cost_tile_of(t.rows, t.cols, k); }

// The source of channel ch as the collect task whose loader and checks it shares (all but dst and the pixel range).
CL_HD CollectTask color_source(const ColorCostTask &t, uint32_t ch) {
    CollectTask c{};
    c.src = t.src[ch]; c.pitch = t.pitch[ch]; c.step = t.step[ch];
    c.rows = t.rows; c.cols = t.cols; c.px0 = 0; c.px1 = t.rows * t.cols;
    c.format = t.format; c.scale = t.scale; c.bias = t.bias;
    return c;
}

// The cost of pixel p with prediction pred, both 0..255.
CL_HD uint32_t color_pixel_cost(uint32_t p, uint32_t pred) {
    const uint32_t d = (p - pred) & 255u;                            // e = d < 128 ? d : d - 256
    return 2u * cost_bitlen(d < 128u ? d : 256u - d) + 1u;
}

// The nine planes: which channel a plane is made of, and which it is taken against (-1: none).
CL_HD int color_plane_own(uint32_t plane) { return plane < 3 ? int(plane) : int((plane - 3) / 2); }
CL_HD int color_plane_ref(uint32_t plane) {
    if (plane < 3) return -1;
    const int own = int((plane - 3) / 2), k = int((plane - 3) % 2);  // the other two channels in ascending order
    return own == 0 ? 1 + k : (own == 1 ? 2 * k : k);
}
// The place of the difference c - b in the cost table (c != b).
CL_HD uint32_t color_diff_plane(uint32_t c, uint32_t b) { return 3u + 2u * c + (c == 0 ? b - 1u : (c == 1 ? b / 2u : b)); }

// The costs of the pixel at (y, x) whose own and neighbouring pixels are p, w, n, nw of R, G, B: added to sums[9].
template <class Sum>
CL_HD void color_pixel_costs(const uint32_t p[3], const uint32_t w[3], const uint32_t n[3], const uint32_t nw[3], uint32_t y, uint32_t x, Sum sums[kColorCosts]) {
    for (uint32_t k = 0; k < kColorCosts; k++) {
        const int a = color_plane_own(k), r = color_plane_ref(k);
        uint32_t P = p[a], W = w[a], N = n[a], NW = nw[a];
        if (r >= 0) { P = collect_rct(P, p[r]); W = collect_rct(W, w[r]); N = collect_rct(N, n[r]); NW = collect_rct(NW, nw[r]); }
        sums[k] += color_pixel_cost(P, cost_pred(W, N, NW, y, x));
    }
}

// ---- the mode byte -----------------------------------------------------------------------------------------------------------
inline bool color_mode_valid(uint32_t m) { return m == 0 || (m < 16 && (m & 3u) != 3u && (m & 12u) != 0); }
// The channel that plane c (0 = R, 1 = G, 2 = B) of a frame of mode m is taken against; -1: it is coded as it is.
inline int color_mode_ref(uint32_t m, uint32_t c) {
    const uint32_t b = m & 3u;
    if (c == b || !(m & 12u)) return -1;
    const uint32_t lower = b == 0 ? 1u : 0u;                          // the lower-numbered of the two other channels
    return (m & (c == lower ? 4u : 8u)) ? int(b) : -1;
}

// THE RULE (part of the interface: two builds plan alike).  With base b, channel c takes its difference
// only if 64 * cost(c - b) < 63 * cost(c); total(b) = cost(b) + the cheaper alternative of each other channel under that
// rule; the smallest total wins, ties go to G, then R, then B; a winner without a difference is mode 0.
inline uint8_t color_choose(const unsigned long long costs[kColorCosts]) {
    const uint32_t order[3] = {1, 0, 2};
    unsigned long long best_total = 0;
    uint32_t best = 0;
    bool have = false;
    for (uint32_t b : order) {
        const uint32_t lower = b == 0 ? 1u : 0u, higher = b == 2 ? 1u : 2u;
        unsigned long long total = costs[b];
        uint32_t mode = b;
        for (uint32_t c : {lower, higher}) {
            const unsigned long long d = costs[color_diff_plane(c, b)], plain = costs[c];
            const bool take = (unsigned __int128)(d) * 64u < (unsigned __int128)(plain) * 63u;
            total += take ? d : plain;
            if (take) mode |= c == lower ? 4u : 8u;
        }
        if (!have || total < best_total) { have = true; best_total = total; best = mode; }
    }
    return uint8_t((best & 12u) ? best : 0u);
}

// What a task must satisfy before the kernel or the host walk may run it: three sources that collect takes, cap[ch] bytes
// readable from each, and a place for the sums.
inline bool color_task_ok(const ColorCostTask &t, const unsigned long long cap[3]) {
    for (uint32_t ch = 0; ch < 3; ch++)
        if (!collect_source_ok(color_source(t, ch), cap[ch])) return false;
    return t.costs != nullptr;
}

// The host walk: every tile of the task, one after the other, pixel by pixel; each element is read where it lies.
inline void color_cost_host(const ColorCostTask &t) {
    const uint32_t elem = collect_elem(t.format);
    unsigned long long sums[kColorCosts] = {};
    cost_walk_tiles(t.rows, t.cols, [&](const CostTile &T) {
        cost_tile_pixels(T, [&](uint32_t y, uint32_t x) {
            uint32_t p[3], w[3], n[3], nw[3];
            for (uint32_t ch = 0; ch < 3; ch++) {
                uint32_t v[4];
                cost_neighbours([&](uint32_t yy, uint32_t xx) { return collect_value(cost_element(t.src[ch], t.pitch[ch], t.step[ch], elem, yy, xx), t.format, t.scale, t.bias); }, y, x, v);
                p[ch] = v[0]; w[ch] = v[1]; n[ch] = v[2]; nw[ch] = v[3];
            }
            color_pixel_costs(p, w, n, nw, y, x, sums);
        });
    });
    for (uint32_t k = 0; k < kColorCosts; k++) t.costs[k] += sums[k];
}

}  // namespace nblic
