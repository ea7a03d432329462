// cost_tile.h -- what the cost passes over pixels share (color_plan.h, stack.h, deep.h): the cut of an image into TILES, the
// MED prediction, the bit length of a residual, and the host walk over tiles and their pixels.  Host and device call the same
// functions: a cost kernel (serial_engine.hip) runs one workgroup per tile, a host walk one tile after the other, and the
// sums, being integer adds, do not depend on the order.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CT_HD __host__ __device__ inline
#else
#define CT_HD inline
#endif

namespace nblic {

constexpr uint32_t kCostTile = 64;                                   // a workgroup's tile: 64 x 64 pixels, one wave per sixteen rows

CT_HD uint32_t cost_tiles_across(uint32_t cols) { return (cols + kCostTile - 1) / kCostTile; }
CT_HD uint32_t cost_tiles(uint32_t rows, uint32_t cols) { return cost_tiles_across(cols) * ((rows + kCostTile - 1) / kCostTile); }      // (<= 1024^2)

// Tile k of an image, row-major: its rows [y0, y1) and columns [x0, x1), the ends clipped to the image.
struct CostTile { uint32_t y0, x0, y1, x1; };
CT_HD CostTile cost_tile_of(uint32_t rows, uint32_t cols, uint32_t k) {
    const uint32_t across = cost_tiles_across(cols), y0 = (k / across) * kCostTile, x0 = (k % across) * kCostTile;
    return CostTile{y0, x0, rows - y0 > kCostTile ? y0 + kCostTile : rows, cols - x0 > kCostTile ? x0 + kCostTile : cols};
}

// MED of the three neighbours' pixels at image position (y, x); neighbours that do not exist are not looked at.
CT_HD uint32_t cost_pred(uint32_t w, uint32_t n, uint32_t nw, uint32_t y, uint32_t x) {
    if (y == 0) return x == 0 ? 128u : w;
    if (x == 0) return n;
    const uint32_t lo = w < n ? w : n, hi = w < n ? n : w;
    if (nw >= hi) return lo;
    if (nw <= lo) return hi;
    return w + n - nw;
}
CT_HD uint32_t cost_bitlen(uint32_t v) {                             // v <= 255
    uint32_t k = 0;
    while (v) { v >>= 1; k++; }
    return k;
}

// ---- the host walk: every tile of an image, one after the other -- tile(T) -- and every pixel of a tile, row by row ------------
template <class F> inline void cost_walk_tiles(uint32_t rows, uint32_t cols, F &&tile) {
    for (uint32_t k = 0, n = cost_tiles(rows, cols); k < n; k++) tile(cost_tile_of(rows, cols, k));
}
template <class F> inline void cost_tile_pixels(const CostTile &T, F &&pixel) {
    for (uint32_t y = T.y0; y < T.y1; y++)
        for (uint32_t x = T.x0; x < T.x1; x++) pixel(y, x);
}
// The pixel at (y, x) and its neighbours, v = {p, w, n, nw}, each read by at(y, x); one that does not exist is 0 and not read.
template <class At> inline void cost_neighbours(At &&at, uint32_t y, uint32_t x, uint32_t v[4]) {
    v[0] = at(y, x); v[1] = x ? at(y, x - 1) : 0u; v[2] = y ? at(y - 1, x) : 0u; v[3] = x && y ? at(y - 1, x - 1) : 0u;
}
// The element of `elem` bytes at (y, x) of a source, read where it lies (little endian: the low elem bytes).
inline uint32_t cost_element(const uint8_t *src, unsigned long long pitch, unsigned long long step, uint32_t elem, uint32_t y, uint32_t x) {
    uint32_t v = 0;
    memcpy(&v, src + (unsigned long long)(y) * pitch + (unsigned long long)(x) * step, elem);
    return v;
}

}  // namespace nblic
