// Stand-alone check of csrc/stack.h (host only): the run delivery's walk and the cost walk over the host tests' shapes, in all
// four formats, against restatements that know nothing of units, words or tiles.  Every plane and source is a heap block of
// EXACTLY its extent -- a read outside it is an overrun the sanitizer reports -- and every destination a block filled with a
// pattern that is compared whole, so a byte written outside a window shows wherever it lands.  The delivery's
// restatement restores a run byte by byte in wide integers and scatters it element by element; the cost's makes the planes
// with a pixel function that rounds through doubles and walks each plane with its own MED and its own bit length.  Also the
// word arithmetic on every pair of bytes, the mode bytes and the rule.
// Build and run:
//   g++ -std=c++17 -O2 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o stack_check tools/stack_check.cpp && ./stack_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nblic-image-compression_amd/csrc/stack.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int kShapes[][2] = {{1, 1}, {1, 17}, {17, 1}, {3, 5}, {33, 17}, {64, 64}, {65, 65}, {129, 129}, {65, 130}, {130, 65}};
static const int kDepths[] = {1, 2, 3, 5, 9};

static double half_value(uint32_t h) {
    const double sign = (h & 0x8000u) ? -1.0 : 1.0;
    const int e = int((h >> 10) & 0x1Fu), m = int(h & 0x3FFu);
    if (e == 0x1F) return m ? NAN : sign * INFINITY;
    return sign * (e ? std::ldexp(1024.0 + m, e - 25) : std::ldexp(double(m), -24));
}
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
    uint32_t bits;
    memcpy(&bits, &f, 4);
    if (kind == 4) bits = 0x7FC00000u | (rng() & 0x80000000u);
    if (kind == 5) bits = rng();
    if (format == kCollectF32) return bits;
    if (format == kCollectBF16) return bits >> 16;
    return rng() & 0xFFFFu;
}
// One delivered element's bits, restated: the two roundings through doubles, then the format.
static uint32_t element_ref(int px, uint32_t format, float scale, float bias) {
    if (format == kDeliverU8) return uint32_t(px);
    const float prod = float(double(px) * double(scale));
    const float v = float(double(prod) + double(bias));
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return format == kDeliverF32 ? bits : (format == kDeliverF16 ? deliver_f16_bits(bits) : deliver_bf16_bits(bits));
}

// The cost of one plane, restated.
static unsigned long long plane_cost(const std::vector<int> &p, int rows, int cols) {
    unsigned long long sum = 0;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            int pred;
            if (y == 0 && x == 0) pred = 128;
            else if (y == 0) pred = p[size_t(x) - 1];
            else if (x == 0) pred = p[size_t(y - 1) * cols];
            else {
                const int w = p[size_t(y) * cols + x - 1], n = p[size_t(y - 1) * cols + x], nw = p[size_t(y - 1) * cols + x - 1];
                pred = nw >= std::max(w, n) ? std::min(w, n) : (nw <= std::min(w, n) ? std::max(w, n) : w + n - nw);
            }
            int e = ((p[size_t(y) * cols + x] - pred) % 256 + 256) % 256;
            if (e >= 128) e -= 256;
            int a = std::abs(e), len = 0;
            while (a) { a /= 2; len++; }
            sum += 2u * unsigned(len) + 1u;
        }
    return sum;
}

static int check_arithmetic() {
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t want = uint32_t((int(a) + int(b) - 128 + 256) % 256);
            CHECK(stack_restore(a, b) == want);
            CHECK(stack_restore(stack_delta(a, b), b) == a);
            // the byte in every lane of a word, beside neighbours that carry and borrow
            const uint32_t t = a | (0xFFu << 8) | (a << 16) | (0x00u << 24), p = b | (0xFFu << 8) | (b << 16) | (0x7Fu << 24);
            const uint32_t w = stack_restore4(t, p);
            CHECK((w & 0xFFu) == want && ((w >> 16) & 0xFFu) == want && ((w >> 8) & 0xFFu) == stack_restore(0xFF, 0xFF) && (w >> 24) == stack_restore(0, 0x7F));
        }
    return 0;
}

static int check_modes_and_rule() {
    for (uint32_t m = 0; m < 256; m++) CHECK(stack_mode_valid(m) == (m < 2));
    const uint8_t good[6] = {0, 1, 1, 0, 0, 1}, head[6] = {0, 1, 1, 1, 0, 1};
    CHECK(stack_modes_ok(6, 3, good) && stack_modes_ok(6, 6, good) && !stack_modes_ok(6, 3, head) && !stack_modes_ok(6, 4, good) && !stack_modes_ok(6, 0, good));
    CHECK(!stack_modes_ok(6, 3, nullptr) && !stack_modes_ok(-3, 3, good));
    for (uint32_t b = 2; b < 256; b++) { uint8_t bad[6] = {0, 1, uint8_t(b), 0, 0, 1}; CHECK(!stack_modes_ok(6, 3, bad)); }
    const uint8_t last[5] = {0, 1, 1, 1, 0};                              // a lone key behind a run ends the stack
    CHECK(stack_modes_ok(5, 5, last) && stack_run_len(last, 0, 5) == 4 && stack_run_len(last, 4, 5) == 1);
    CHECK(stack_run_len(good, 0, 6) == 3 && stack_run_len(good, 3, 6) == 1 && stack_run_len(good, 4, 6) == 2 && stack_run_len(good, 0, 3) == 3 && stack_run_len(good, 0, 1) == 1);
    CHECK(stack_choose(64, 62) == 1 && stack_choose(64, 63) == 0 && stack_choose(64, 64) == 0 && stack_choose(0, 0) == 0 && stack_choose(6400, 6299) == 1 && stack_choose(6400, 6300) == 0);
    CHECK(stack_slice_mode(0, 0, 100, 1) == 0 && stack_slice_mode(3, 0, 100, 1) == 1 && stack_slice_mode(4, 2, 100, 1) == 0 && stack_slice_mode(3, 2, 100, 1) == 1 &&
          stack_slice_mode(3, 2, 100, 99) == 0 && stack_slice_mode(5, 1, 100, 1) == 0);
    CHECK(stack_choose(1ull << 63, (1ull << 63) - (1ull << 57) - 1) == 1 && stack_choose(1ull << 63, (1ull << 63) - (1ull << 57)) == 0);
    return 0;
}

static int check_deliver(unsigned &runs) {
    std::mt19937 rng(2701);
    unsigned k = 0;
    for (const auto &shape : kShapes)
        for (uint32_t format = 0; format < kDeliverFormats; format++)
            for (int variant = 0; variant < 3; variant++, k++) {
                const int h = shape[0], w = shape[1], depth = kDepths[1 + k % 4];
                const uint32_t elem = deliver_elem(format);
                const size_t D = size_t(depth);
                const int r0 = variant == 1 ? h / 3 : 0, r1 = variant == 1 ? h - h / 4 : h, c0 = variant == 1 ? w / 5 : 0, c1 = variant == 1 ? w - w / 6 : w;
                const int rows = r1 - r0, cols = c1 - c0;
                std::vector<std::vector<int>> x(D, std::vector<int>(size_t(h) * w));      // the slices, and the planes of the run
                std::vector<uint8_t *> planes(D), outs(D, nullptr);
                std::vector<size_t> out_len(D, 0);
                std::vector<StackSlice> S(D);
                std::vector<int> gates(D, 1);
                for (int d = 0; d < depth; d++) {
                    planes[size_t(d)] = static_cast<uint8_t *>(malloc(size_t(h) * w));
                    for (size_t i = 0; i < size_t(h) * w; i++) {
                        x[size_t(d)][i] = d && variant == 2 && rng() % 4 ? (rng() % 2 ? 255 : 0) : int(rng() & 0xFF);
                        planes[size_t(d)][i] = uint8_t(d ? (x[size_t(d)][i] - x[size_t(d) - 1][i] + 128 + 256) % 256 : x[size_t(d)][i]);
                    }
                    StackSlice &s = S[size_t(d)];
                    s = StackSlice{};
                    s.src = planes[size_t(d)] + size_t(r0) * w; s.src_bytes = size_t(h - r0) * w;
                    s.scale = format ? 1.0f / float(1 + (k + d) % 3) : 1.0f; s.bias = format ? -0.5f + 0.25f * float(d % 4) : 0.0f;
                    s.dst_step = variant == 1 ? (2 + d % 2) * elem : elem;
                    s.dst_pitch = variant == 1 ? (cols * (2 + d % 2) + d) * elem : (cols + (variant == 2 ? d : 0)) * elem;
                    if (variant == 1 && d == 1) continue;                // a skipped slice
                    out_len[size_t(d)] = size_t(deliver_extent(uint32_t(rows), uint32_t(cols), format, s.dst_pitch, s.dst_step));
                    void *p = nullptr;
                    if (posix_memalign(&p, 16, out_len[size_t(d)] + 16 * elem) != 0) return 1;
                    outs[size_t(d)] = static_cast<uint8_t *>(p);
                    memset(outs[size_t(d)], 0x5A, out_len[size_t(d)] + 16 * elem);
                    // at a multiple of 16 bytes, or an element behind one; the whole block is compared, so a stray byte inside it shows too
                    s.dst = outs[size_t(d)] + (variant == 0 && d % 2 ? elem : 0);
                }
                if (variant == 2) gates[size_t(depth / 2)] = 2;          // a gate in the middle that is not done
                if (variant == 2 && depth > 3) S[size_t(depth) - 1].zero = 1;
                StackDeliverTask T{};
                T.first_slice = 0; T.count = uint32_t(depth); T.rows = uint32_t(rows); T.col0 = uint32_t(c0); T.col1 = uint32_t(c1); T.src_pitch = uint32_t(w); T.format = format;
                CHECK(stack_task_ok(T, S.data()));
                CHECK(stack_task_units(T) == (unsigned long long)(rows) * ((cols + 15) / 16));
                stack_deliver_host(T, S.data(), gates.data());
                bool ok = true;
                for (int d = 0; d < depth; d++) {
                    const StackSlice &s = S[size_t(d)];
                    ok = ok && gates[size_t(d)] == 1 && !s.zero;
                    if (!s.dst) continue;
                    std::vector<uint8_t> want(out_len[size_t(d)] + 16 * elem, 0x5A);
                    const size_t lead = size_t(s.dst - outs[size_t(d)]);
                    for (int r = 0; r < rows; r++)
                        for (int c = 0; c < cols; c++) {
                            const uint32_t v = ok ? element_ref(x[size_t(d)][size_t(r0 + r) * w + c0 + c], format, s.scale, s.bias) : 0u;
                            memcpy(want.data() + lead + size_t(r) * s.dst_pitch + size_t(c) * s.dst_step, &v, elem);
                        }
                    CHECK(memcmp(want.data(), outs[size_t(d)], want.size()) == 0);
                }
                for (int d = 0; d < depth; d++) { free(planes[size_t(d)]); free(outs[size_t(d)]); }
                runs++;
            }
    // what the checks refuse
    uint8_t plane[64] = {}, out[64 * 4] = {};
    StackSlice s{};
    s.src = plane; s.src_bytes = 64; s.dst = out; s.dst_pitch = 8; s.dst_step = 1; s.scale = 1.0f;
    StackDeliverTask T{};
    T.count = 1; T.rows = 8; T.col0 = 0; T.col1 = 8; T.src_pitch = 8; T.format = kDeliverU8;
    CHECK(stack_task_ok(T, &s));
    { StackDeliverTask B = T; B.rows = 9; CHECK(!stack_task_ok(B, &s)); }
    { StackDeliverTask B = T; B.col1 = 9; CHECK(!stack_task_ok(B, &s)); }
    { StackDeliverTask B = T; B.col0 = 8; CHECK(!stack_task_ok(B, &s)); }
    { StackDeliverTask B = T; B.count = 0; CHECK(!stack_task_ok(B, &s)); }
    { StackDeliverTask B = T; B.format = 4; CHECK(!stack_task_ok(B, &s)); }
    { StackSlice b = s; b.src_bytes = 63; CHECK(!stack_task_ok(T, &b)); }
    { StackSlice b = s; b.dst_pitch = 7; CHECK(!stack_task_ok(T, &b)); }
    { StackSlice b = s; b.scale = 2.0f; CHECK(!stack_task_ok(T, &b)); }
    { StackSlice b = s; b.dst_step = 0; CHECK(!stack_task_ok(T, &b)); }
    { StackSlice b = s; b.dst = nullptr; b.dst_pitch = 0; CHECK(stack_task_ok(T, &b)); }      // a skipped slice has no destination to check
    { StackDeliverTask B = T; B.format = kDeliverF16; StackSlice b = s; b.dst = out + 1; b.dst_pitch = 16; b.dst_step = 2; CHECK(!stack_task_ok(B, &b)); }
    return 0;
}

static int check_cost(unsigned &stacks) {
    std::mt19937 rng(2702);
    unsigned k = 0;
    for (uint32_t format = 0; format < kCollectFormats; format++)
        for (const auto &shape : kShapes)
            for (int layout = 0; layout < 3; layout++, k++) {
                const int rows = shape[0], cols = shape[1], depth = rows * cols < 4096 ? kDepths[k % 5] : kDepths[k % 3];
                const uint32_t elem = collect_elem(format);
                const size_t D = size_t(depth);
                const float scale = format == kCollectU8 ? 1.0f : (k % 3 == 1 ? 255.0f : (k % 3 == 2 ? 127.5f : 1.0f)), bias = format != kCollectU8 && k % 3 == 2 ? 127.5f : 0.0f;
                std::vector<uint8_t *> blocks(D);
                std::vector<StackCostSlice> S(D);
                std::vector<unsigned long long> caps(D);
                std::vector<std::vector<int>> planes(D, std::vector<int>(size_t(rows) * cols));
                for (int d = 0; d < depth; d++) {
                    const size_t step = layout == 1 ? 3 * elem : elem, pitch = layout == 0 ? size_t(cols) * elem : (layout == 1 ? size_t(cols) * 3 * elem : size_t(cols + 1 + (k + d) % 3) * elem);
                    const size_t extent = size_t(collect_extent(uint32_t(rows), uint32_t(cols), format, pitch, step));
                    blocks[size_t(d)] = static_cast<uint8_t *>(malloc(extent));
                    memset(blocks[size_t(d)], 0xFF, extent);
                    for (int y = 0; y < rows; y++)
                        for (int x = 0; x < cols; x++) {
                            uint32_t bits = element_bits(rng, format);
                            if (format == kCollectU8 && d && d % 2 == 0) bits = uint32_t(std::min(255, std::max(0, planes[size_t(d) - 1][size_t(y) * cols + x] + int(rng() % 5) - 2)));
                            memcpy(blocks[size_t(d)] + size_t(y) * pitch + size_t(x) * step, &bits, elem);
                            planes[size_t(d)][size_t(y) * cols + x] = pixel_ref(bits, format, scale, bias);
                        }
                    S[size_t(d)] = StackCostSlice{blocks[size_t(d)], pitch, uint32_t(step), 0u};
                    caps[size_t(d)] = extent;
                }
                std::vector<unsigned long long> sums(D * 2, 0ull);
                StackCostTask T{};
                T.costs = sums.data(); T.first_slice = 0; T.count = uint32_t(depth); T.rows = uint32_t(rows); T.cols = uint32_t(cols);
                T.format = format; T.scale = scale; T.bias = bias;
                CHECK(stack_cost_task_ok(T, S.data(), caps.data()));
                caps[size_t(depth) - 1]--;
                CHECK(!stack_cost_task_ok(T, S.data(), caps.data()));
                CHECK(stack_task_tiles(T) == uint32_t(((rows + 63) / 64) * ((cols + 63) / 64)));
                stack_cost_host(T, S.data());
                for (int d = 0; d < depth; d++) {
                    CHECK(sums[size_t(d) * 2] == plane_cost(planes[size_t(d)], rows, cols));
                    unsigned long long delta = 0;
                    if (d) {
                        std::vector<int> diff(size_t(rows) * cols);
                        for (size_t i = 0; i < diff.size(); i++) diff[i] = (planes[size_t(d)][i] - planes[size_t(d) - 1][i] + 128 + 256) % 256;
                        delta = plane_cost(diff, rows, cols);
                    }
                    CHECK(sums[size_t(d) * 2 + 1] == delta);
                }
                for (uint8_t *b : blocks) free(b);
                stacks++;
            }
    return 0;
}

int main() {
    unsigned runs = 0, stacks = 0;
    if (check_arithmetic() || check_modes_and_rule() || check_deliver(runs) || check_cost(stacks)) return 1;
    printf("stack_check: %u runs delivered and %u stacks of two sums a slice, the byte arithmetic, the mode bytes and the rule, all as expected\n", runs, stacks);
    return 0;
}
