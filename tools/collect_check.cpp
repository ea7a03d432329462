// Stand-alone check of csrc/collect.h (host only): the refusals, and the unit walk of the collect kernel over a small grid
// of widths, heights, steps, pitches, source residues, formats and pixel ranges.  The source is a heap block of EXACTLY
// the image's extent and the plane one of exactly rows x cols bytes -- a read or a store outside them is an overrun the
// sanitizer reports -- gaps between the elements hold NaN (0xFF), and every byte is compared with a plain loop that knows
// nothing of units and rounds through doubles; the units of a task must tile its pixels in order, each at a multiple of
// 16.  Tasks with a reference (the colour transform's difference planes) have a second block of exactly the reference's
// extent, in a layout of its own, and are compared with (own - ref + 128) mod 256 of the two plain loops' pixels.
// Build and run:
//   g++ -std=c++17 -O2 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o collect_check tools/collect_check.cpp && ./collect_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nblic-image-compression_amd/csrc/collect.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// binary16 bits -> double, by the format's definition.
static double half_value(uint32_t h) {
    const double sign = (h & 0x8000u) ? -1.0 : 1.0;
    const int e = int((h >> 10) & 0x1Fu), m = int(h & 0x3FFu);
    if (e == 0x1F) return m ? NAN : sign * INFINITY;
    return sign * (e ? std::ldexp(1024.0 + m, e - 25) : std::ldexp(double(m), -24));
}

// The pixel of an element, through doubles: each of the two operations is rounded to float by the conversion (a double
// holds the exact product and the exact sum of two floats' worth of bits), then nearbyint (to even) and the clamp.
static uint8_t pixel_ref(uint32_t x, uint32_t format, float scale, float bias) {
    if (format == kCollectU8) return uint8_t(x);
    float f;
    if (format == kCollectF16) f = float(half_value(x));
    else { const uint32_t b = format == kCollectBF16 ? x << 16 : x; memcpy(&f, &b, 4); }
    const float prod = float(double(f) * double(scale));
    const float v = float(double(prod) + double(bias));
    if (v != v) return 0;
    const double r = std::nearbyint(double(v));
    return uint8_t(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
}

static uint32_t element_bits(std::mt19937 &rng, uint32_t format) {
    if (format == kCollectU8) return rng() & 0xFFu;
    const uint32_t kind = rng() % 8;
    float f = kind == 0 ? float(rng() % 512) * 0.5f - 0.5f : (kind == 1 ? float(int(rng() % 2000) - 1000) : float(rng() % 65536) / 65536.0f);
    if (kind == 2) f = -0.0f;
    if (kind == 3) f = (rng() & 1) ? INFINITY : -INFINITY;
    uint32_t bits;
    memcpy(&bits, &f, 4);
    if (kind == 4) bits = 0x7FC00000u | (rng() & 0x80000000u);       // NaN, either sign
    if (kind == 5) bits = rng();                                     // any pattern
    if (format == kCollectF32) return bits;
    if (format == kCollectBF16) return bits >> 16;
    return rng() & 0xFFFFu;                                          // float16: any pattern (all of them are run below)
}

static int one_task(std::mt19937 &rng, uint32_t format, uint32_t rows, uint32_t cols, uint32_t step_elems, size_t slack_elems, bool transposed,
                    size_t residue, float scale, float bias, uint32_t px0, uint32_t px1) {
    const uint32_t elem = collect_elem(format);
    const size_t step = transposed ? (size_t(rows) + slack_elems) * elem : size_t(step_elems) * elem;
    const size_t pitch = transposed ? elem : (size_t(cols - 1) * step_elems + 1 + slack_elems) * elem;
    const size_t extent = size_t(collect_extent(rows, cols, format, pitch, step));
    void *aligned = nullptr, *plane_mem = nullptr;
    CHECK(posix_memalign(&aligned, 16, residue + extent) == 0 && posix_memalign(&plane_mem, 16, size_t(rows) * cols) == 0);
    uint8_t *block = static_cast<uint8_t *>(aligned), *src = block + residue, *plane = static_cast<uint8_t *>(plane_mem);
    memset(block, 0xFF, residue + extent);                           // NaN wherever no element lies
    memset(plane, 0x5A, size_t(rows) * cols);
    std::vector<uint32_t> elems(size_t(rows) * cols);
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < cols; c++) {
            const uint32_t x = element_bits(rng, format);
            elems[size_t(r) * cols + c] = x;
            memcpy(src + size_t(r) * pitch + size_t(c) * step, &x, elem);
        }
    CollectTask T{};
    T.src = src; T.dst = plane; T.pitch = pitch; T.step = uint32_t(step); T.rows = rows; T.cols = cols; T.px0 = px0; T.px1 = px1;
    T.format = format; T.scale = scale; T.bias = bias;
    CHECK(collect_task_ok(T, extent));
    CHECK(!collect_task_ok(T, extent - 1));
    const uint32_t units = collect_task_units(T);
    uint32_t at = px0;
    for (uint32_t u = 0; u < units; u++) {                           // the units tile [px0, px1) in order
        const CollectUnit U = collect_unit_of(T, u);
        CHECK(U.p0 % 16 == 0 && U.p_lo == at && U.p_lo < U.p_hi && U.p_lo >= U.p0 && U.p_hi <= U.p0 + kCollectUnitPixels);
        at = U.p_hi;
    }
    CHECK(at == px1);
    collect_host(T);
    for (uint32_t p = 0; p < rows * cols; p++)
        CHECK(plane[p] == (p >= px0 && p < px1 ? pixel_ref(elems[p], format, scale, bias) : 0x5A));
    free(block); free(plane);
    return 0;
}

// A task with a reference: the own source and the reference in layouts of their own (step and slack in elements), each a
// block of exactly its extent.
static int one_ref_task(std::mt19937 &rng, uint32_t format, uint32_t rows, uint32_t cols, uint32_t step_elems, size_t slack_elems, uint32_t ref_step_elems,
                        size_t ref_slack_elems, size_t residue, size_t ref_residue, float scale, float bias, uint32_t px0, uint32_t px1) {
    const uint32_t elem = collect_elem(format);
    const size_t step = size_t(step_elems) * elem, pitch = (size_t(cols - 1) * step_elems + 1 + slack_elems) * elem;
    const size_t ref_step = size_t(ref_step_elems) * elem, ref_pitch = (size_t(cols - 1) * ref_step_elems + 1 + ref_slack_elems) * elem;
    const size_t extent = size_t(collect_extent(rows, cols, format, pitch, step)), ref_extent = size_t(collect_extent(rows, cols, format, ref_pitch, ref_step));
    void *own_mem = nullptr, *ref_mem = nullptr, *plane_mem = nullptr;
    CHECK(posix_memalign(&own_mem, 16, residue + extent) == 0 && posix_memalign(&ref_mem, 16, ref_residue + ref_extent) == 0 &&
          posix_memalign(&plane_mem, 16, size_t(rows) * cols) == 0);
    uint8_t *src = static_cast<uint8_t *>(own_mem) + residue, *ref = static_cast<uint8_t *>(ref_mem) + ref_residue, *plane = static_cast<uint8_t *>(plane_mem);
    memset(own_mem, 0xFF, residue + extent);
    memset(ref_mem, 0xFF, ref_residue + ref_extent);
    memset(plane, 0x5A, size_t(rows) * cols);
    std::vector<uint32_t> elems(size_t(rows) * cols), ref_elems(size_t(rows) * cols);
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < cols; c++) {
            const uint32_t x = element_bits(rng, format), y = element_bits(rng, format);
            elems[size_t(r) * cols + c] = x; ref_elems[size_t(r) * cols + c] = y;
            memcpy(src + size_t(r) * pitch + size_t(c) * step, &x, elem);
            memcpy(ref + size_t(r) * ref_pitch + size_t(c) * ref_step, &y, elem);
        }
    CollectTask T{};
    T.src = src; T.dst = plane; T.pitch = pitch; T.step = uint32_t(step); T.rows = rows; T.cols = cols; T.px0 = px0; T.px1 = px1;
    T.format = format; T.scale = scale; T.bias = bias;
    T.ref = ref; T.ref_pitch = ref_pitch; T.ref_step = uint32_t(ref_step);
    CHECK(collect_task_ok(T, extent, ref_extent));
    CHECK(!collect_task_ok(T, extent, ref_extent - 1) && !collect_task_ok(T, extent - 1, ref_extent) && !collect_task_ok(T, extent));
    collect_host(T);
    for (uint32_t p = 0; p < rows * cols; p++) {
        const uint8_t want = uint8_t((int(pixel_ref(elems[p], format, scale, bias)) - int(pixel_ref(ref_elems[p], format, scale, bias)) + 128 + 256) % 256);
        CHECK(plane[p] == (p >= px0 && p < px1 ? want : 0x5A));
    }
    free(own_mem); free(ref_mem); free(plane);
    return 0;
}

static int refusals() {
    alignas(16) static uint8_t src[4096], dst[256];
    CollectTask S{};
    S.src = src; S.dst = dst; S.pitch = 64; S.step = 2; S.rows = 4; S.cols = 8; S.px0 = 0; S.px1 = 32; S.format = kCollectF16; S.scale = 255.0f; S.bias = 0.0f;
    const unsigned long long cap = collect_extent(4, 8, kCollectF16, 64, 2);
    CHECK(cap == 3 * 64 + 7 * 2 + 2 && collect_task_ok(S, cap) && !collect_task_ok(S, cap - 1));
    CollectTask T;
    T = S; T.rows = 0; CHECK(!collect_task_ok(T, cap));
    T = S; T.cols = 0; CHECK(!collect_task_ok(T, cap));
    T = S; T.rows = 65536; CHECK(!collect_task_ok(T, ~0ull));
    T = S; T.cols = 65536; CHECK(!collect_task_ok(T, ~0ull));
    T = S; T.src = src + 1; CHECK(!collect_task_ok(T, cap));
    T = S; T.src = nullptr; CHECK(!collect_task_ok(T, cap));
    T = S; T.pitch = 63; CHECK(!collect_task_ok(T, cap));
    T = S; T.step = 3; CHECK(!collect_task_ok(T, ~0ull));
    T = S; T.step = 0; CHECK(!collect_task_ok(T, cap));
    T = S; T.pitch = 0; CHECK(!collect_task_ok(T, cap));
    T = S; T.format = kCollectU8; T.step = 0; CHECK(!collect_task_ok(T, cap));
    T = S; T.step = kCollectMaxStep + 2; CHECK(!collect_task_ok(T, ~0ull));
    T = S; T.step = kCollectMaxStep; CHECK(collect_task_ok(T, ~0ull));
    T = S; T.pitch = kCollectMaxPitch + 2; CHECK(!collect_task_ok(T, ~0ull));
    T = S; T.pitch = kCollectMaxPitch; CHECK(collect_task_ok(T, ~0ull));
    T = S; T.format = kCollectFormats; CHECK(!collect_task_ok(T, cap));
    T = S; T.scale = NAN; CHECK(!collect_task_ok(T, cap));
    T = S; T.bias = INFINITY; CHECK(!collect_task_ok(T, cap));
    T = S; T.format = kCollectU8; T.scale = 1.0f; CHECK(collect_task_ok(T, cap));
    T = S; T.format = kCollectU8; CHECK(!collect_task_ok(T, cap));               // uint8 with scale 255
    T = S; T.format = kCollectU8; T.scale = 1.0f; T.bias = 1.0f; CHECK(!collect_task_ok(T, cap));
    T = S; T.dst = dst + 4; CHECK(!collect_task_ok(T, cap));
    T = S; T.dst = nullptr; CHECK(!collect_task_ok(T, cap));
    T = S; T.px1 = 33; CHECK(!collect_task_ok(T, cap));
    T = S; T.px0 = 32; CHECK(!collect_task_ok(T, cap));
    // a reference is checked like a source, against its own readable bytes
    CollectTask R = S;
    R.ref = src + 2048; R.ref_pitch = 32; R.ref_step = 4;
    const unsigned long long rcap = collect_extent(4, 8, kCollectF16, 32, 4);
    CHECK(collect_task_ok(R, cap, rcap) && !collect_task_ok(R, cap, rcap - 1) && !collect_task_ok(R, cap) && !collect_task_ok(R, cap - 1, rcap));
    T = R; T.ref = src + 2049; CHECK(!collect_task_ok(T, cap, rcap));
    T = R; T.ref_pitch = 33; CHECK(!collect_task_ok(T, cap, ~0ull));
    T = R; T.ref_step = 3; CHECK(!collect_task_ok(T, cap, ~0ull));
    T = R; T.ref_step = 0; CHECK(!collect_task_ok(T, cap, rcap));
    T = R; T.ref_pitch = 0; CHECK(!collect_task_ok(T, cap, rcap));
    T = R; T.ref_step = kCollectMaxStep + 2; CHECK(!collect_task_ok(T, cap, ~0ull));
    T = R; T.ref_step = kCollectMaxStep; CHECK(collect_task_ok(T, cap, ~0ull));
    T = R; T.ref_pitch = kCollectMaxPitch + 2; CHECK(!collect_task_ok(T, cap, ~0ull));
    T = R; T.ref_pitch = kCollectMaxPitch; CHECK(collect_task_ok(T, cap, ~0ull));
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t b = 0; b < 256; b++) CHECK(collect_rct(a, b) == uint32_t((int(a) - int(b) + 128 + 256) % 256));
    CHECK(collect_in_place(kCollectU8, 8, 1, 8) && !collect_in_place(kCollectU8, 9, 1, 8) && !collect_in_place(kCollectU8, 8, 2, 8) && !collect_in_place(kCollectF16, 8, 1, 8));
    return 0;
}

int main() {
    if (refusals()) return 1;
    std::mt19937 rng(23);
    const float norms[][2] = {{1.0f, 0.0f}, {255.0f, 0.0f}, {127.5f, 127.5f}, {0.5f, 0.25f}, {3e38f, 0.0f}, {-1.0f, 255.0f}};
    const uint32_t widths[] = {1, 15, 16, 17, 33}, heights[] = {1, 2, 3}, steps[] = {1, 3, 4};
    long tasks = 0;
    for (uint32_t format = 0; format < kCollectFormats; format++) {
        const uint32_t elem = collect_elem(format);
        for (uint32_t w : widths)
            for (uint32_t h : heights)
                for (size_t residue = 0; residue < 16; residue += elem)
                    for (int layout = 0; layout < 4; layout++) {     // three steps with slack, and transposed
                        const float *nb = format == kCollectU8 ? norms[0] : norms[rng() % 6];
                        const uint32_t n = w * h;
                        uint32_t px0 = 0, px1 = n;
                        if (rng() % 3 == 0) { px0 = rng() % n; px1 = px0 + 1 + rng() % (n - px0); }
                        if (one_task(rng, format, h, w, layout < 3 ? steps[layout] : 1, rng() % 4, layout == 3, residue, nb[0], nb[1], px0, px1)) return 1;
                        tasks++;
                    }
    }
    // a task of more than one chunk, rows that end inside units
    if (one_task(rng, kCollectF16, 130, 129, 1, 3, false, 2, 255.0f, 0.0f, 0, 130 * 129)) return 1;
    if (one_task(rng, kCollectU8, 130, 129, 3, 1, false, 5, 1.0f, 0.0f, 129 * 7, 129 * 100)) return 1;
    tasks += 2;
    // tasks with a reference: own source and reference in every pair of steps, other slack and residue each; pixel ranges;
    // rows that end inside units (17 x 33) and the chunk crossed (129 x 129)
    long referenced = 0;
    for (uint32_t format = 0; format < kCollectFormats; format++) {
        const uint32_t elem = collect_elem(format);
        const uint32_t shapes[][2] = {{1, 1}, {1, 17}, {3, 5}, {17, 33}, {2, 16}, {129, 129}};
        for (auto &hw : shapes)
            for (uint32_t own_step : steps)
                for (uint32_t ref_step : steps) {
                    if (hw[0] == 129 && own_step == 3) continue;
                    const float *nb = format == kCollectU8 ? norms[0] : norms[rng() % 6];
                    const uint32_t n = hw[0] * hw[1];
                    uint32_t px0 = 0, px1 = n;
                    if (rng() % 2 == 0) { px0 = rng() % n; px1 = px0 + 1 + rng() % (n - px0); }
                    if (one_ref_task(rng, format, hw[0], hw[1], own_step, rng() % 4, ref_step, rng() % 4, size_t(rng() % (16 / elem)) * elem,
                                     size_t(rng() % (16 / elem)) * elem, nb[0], nb[1], px0, px1)) return 1;
                    referenced++;
                }
    }
    // every float16 and every bfloat16 pattern, and float32 around every k + 0.5
    for (const float *nb : {norms[0], norms[1], norms[2]})
        for (uint32_t x = 0; x < 65536; x++) {
            CHECK(collect_value(x, kCollectF16, nb[0], nb[1]) == pixel_ref(x, kCollectF16, nb[0], nb[1]));
            CHECK(collect_value(x, kCollectBF16, nb[0], nb[1]) == pixel_ref(x, kCollectBF16, nb[0], nb[1]));
        }
    for (int k = 0; k < 256; k++) {
        const float tie = float(k) + 0.5f;
        for (float f : {std::nextafterf(tie, 0.0f), tie, std::nextafterf(tie, 1e9f)}) {
            uint32_t b;
            memcpy(&b, &f, 4);
            CHECK(collect_value(b, kCollectF32, 1.0f, 0.0f) == pixel_ref(b, kCollectF32, 1.0f, 0.0f));
        }
    }
    const float ties[][2] = {{0.5f, 0}, {1.5f, 2}, {2.5f, 2}, {254.5f, 254}, {255.5f, 255}, {-0.0f, 0}, {INFINITY, 255}, {-INFINITY, 0}, {NAN, 0}};
    for (auto &t : ties) {
        uint32_t b;
        memcpy(&b, &t[0], 4);
        CHECK(collect_value(b, kCollectF32, 1.0f, 0.0f) == uint32_t(t[1]));
    }
    printf("collect_check: %ld tasks and %ld with a reference, the refusals, 2 x 3 x 65536 values, all bytes as expected\n", tasks, referenced);
    return 0;
}
