// q_rans.h -- one lane's work of QNBLIC's rANS pass (q_entropy.cpp, QNBLIC.c:238-253), shared by the host and the device:
// the exact quotient without a divide, the step for one symbol, the flush, and how a job's remaining symbols are cut
// into launches, rounds and windows.  The device kernel's lanes (q_device_coder.hip, k_q_rans_lanes) and the host-only
// q_rans_encode_host (q_entropy.cpp) call the same functions, so the arithmetic and the resumption are tested without
// a GPU (tests/test_device_qcoder_host.py, tools/q_rans_check.cpp).
//
// The pass runs LAST PIXEL FIRST over words of level | symbol << 8.  A job's record holds what a launch leaves for the
// next one: the state x, the symbols still to code, the words emitted, the overflow flag.  Words are written at
// DESCENDING addresses from the end of the job's output region -- word k of the pass lands at out_end[-1 - k] -- so the
// region ends in the order the decoder reads (the host pass emits forwards and reverses afterwards).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QR_HD __host__ __device__ inline
#else
#define QR_HD inline
#endif

namespace nblic {

constexpr uint32_t kQRansLevels = 12, kQRansSyms = 256, kQRansTable = kQRansLevels * kQRansSyms;
constexpr uint32_t kQRansWindow = 256;                  // symbols of one 512-byte window
constexpr int kQRansNormBits = 15, kQRansBits = 16;

// What a launch leaves behind for the next one.
struct QRansState {
    uint32_t x;            // the coder; 1 << 16 before the first symbol
    uint32_t left;         // symbols still to code: 0 .. left - 1, the next one is left - 1
    uint32_t pos;          // words emitted so far, those that did not fit included
    uint32_t overflow;     // != 0: a word did not fit the region; the job goes on consuming symbols and stores nothing
};

QR_HD void q_rans_begin(QRansState &s, uint32_t n, uint32_t cap_words) {
    s.x = 1u << kQRansBits; s.left = n; s.pos = 0u; s.overflow = cap_words < 2u ? 1u : 0u;      // the flush alone is two words
}

// One table entry: f | start << 16 (1 <= f <= 32767, start + f <= 32768).
QR_HD uint32_t q_rans_entry(uint32_t f, uint32_t start) { return f | (start << 16); }
// Where a word's entry sits in its image's table.  A level above 11 (no valid word has one) reads the last level's row.
QR_HD uint32_t q_rans_index(uint32_t word) {
    const uint32_t lv = word & 0xFFu;
    return (lv < kQRansLevels ? lv : kQRansLevels - 1u) * kQRansSyms + (word >> 8);
}

QR_HD uint32_t q_rans_mul24(uint32_t a, uint32_t b) {   // both below 2^24, the product below 2^32: a full-rate multiply on the device
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// 1 / f, to within two units in the last place (the device's v_rcp_f32 is good to one).
QR_HD float q_rans_rcp(uint32_t f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(float(f));
#else
    return 1.0f / float(f);
#endif
}

// An estimate of v / f that never exceeds it and falls short by less than v * 2^-19: float(v) and the two products are
// each rounded once (2^-24 relative), rf is within 2^-22 of 1 / f, and the factor 1 - 2^-20 outweighs their sum.
constexpr float kQRansDown = 1.0f - 0x1p-20f;
QR_HD uint32_t q_rans_under(uint32_t v, float rf) { return uint32_t(float(v) * rf * kQRansDown); }

// floor(x / f) for every x in [0, 2^32) and f in [1, 32767], without a divide.  Two estimates from below: the first
// leaves a remainder below (2^13 + 1) f < 2^28, of which the second misses the quotient by one at the most.
QR_HD uint32_t q_rans_quot(uint32_t x, uint32_t f, float rf) {
    const uint32_t q1 = q_rans_under(x, rf);
    const uint32_t r1 = x - q1 * f;
    uint32_t q2 = q_rans_under(r1, rf);
    const uint32_t r2 = r1 - q_rans_mul24(q2, f);
    q2 += r2 >= f ? 1u : 0u;
    return q1 + q2;
}

// The same for x < f << 17, what the pass divides once it has renormalised: the quotient is below 2^17, one estimate
// misses it by less than 2^17 * 2^-19, and its product with f is a 24-bit multiply.  *rem = x - q f.
QR_HD uint32_t q_rans_quot17(uint32_t x, uint32_t f, float rf, uint32_t *rem) {
    uint32_t q = q_rans_under(x, rf);
    uint32_t r = x - q_rans_mul24(q, f);
    const bool more = r >= f;
    q += more ? 1u : 0u;
    r -= more ? f : 0u;
    *rem = r;
    return q;
}

// One symbol (q_entropy.cpp's pass: q = x / f; if q > 2^17 - 1 emit the low word, shift, divide again; x = (x - q f) +
// (q << 15) + start).  q > 2^17 - 1 exactly when x >= f << 17, so the pass decides first and divides once.
// out_end: one past the region's last word; cap: the region's words.
QR_HD void q_rans_put(QRansState &s, uint32_t entry, float rf, uint16_t *out_end, uint32_t cap) {
    const uint32_t f = entry & 0xFFFFu, start = entry >> 16;
    uint32_t x = s.x;
    if (x >= (f << (2 * kQRansBits - kQRansNormBits))) {
        if (s.pos < cap && !s.overflow) out_end[-1 - long(s.pos)] = uint16_t(x); else s.overflow = 1u;
        s.pos++;
        x >>= kQRansBits;
    }
    uint32_t r;
    const uint32_t q = q_rans_quot17(x, f, rf, &r);
    s.x = r + (q << kQRansNormBits) + start;
}

// The flush: two words.  Returns the words of the pass, or 0xFFFFFFFF when the region was too small.
QR_HD uint32_t q_rans_flush(QRansState &s, uint16_t *out_end, uint32_t cap) {
    if (s.overflow || s.pos + 2u > cap) { s.overflow = 1u; s.pos += 2u; return 0xFFFFFFFFu; }
    out_end[-1 - long(s.pos)] = uint16_t(s.x);
    out_end[-2 - long(s.pos)] = uint16_t(s.x >> kQRansBits);
    s.pos += 2u;
    return s.pos;
}

// ---- how a launch cuts a job's remaining symbols ---------------------------------------------------------------------
// A launch with a budget codes `take` symbols of a job, left - take .. left - 1, window by window from the last one
// down: round r of the launch is window (left - 1) / 256 - r, and of that window the positions [lo, hi).  The first
// window of a launch is partial wherever the previous launch (or the image) ended; nothing outside [lo, hi) is used.
struct QRansSpan { uint32_t window, lo, hi; };          // hi == lo: the job has nothing in this round

QR_HD uint32_t q_rans_take(uint32_t left, uint32_t budget) { return left < budget ? left : budget; }
QR_HD uint32_t q_rans_rounds(uint32_t left, uint32_t take) {
    return take ? (left - 1u) / kQRansWindow - (left - take) / kQRansWindow + 1u : 0u;
}
QR_HD QRansSpan q_rans_span(uint32_t left, uint32_t take, uint32_t round) {
    if (round >= q_rans_rounds(left, take)) return QRansSpan{0u, 0u, 0u};
    const uint32_t w = (left - 1u) / kQRansWindow - round, base = w * kQRansWindow, first = left - take;
    const uint32_t lo = first > base ? first - base : 0u;
    const uint32_t hi = left - base < kQRansWindow ? left - base : kQRansWindow;
    return QRansSpan{w, lo, hi};
}

// ---- the operands of the quotient's self-test (device: nblic_amd_qcoder_selftest; host: tools/q_rans_check.cpp) --------
// Per f in 1 .. 32767: the fixed values below, then f << 17 and its two neighbours (where the pass renormalises).
constexpr uint32_t kQRansSelftestFixed = 4 + 3 * 31 + 4096;
constexpr uint32_t kQRansSelftestCount = kQRansSelftestFixed + 3;
QR_HD uint32_t q_rans_selftest_operand(uint32_t k, uint32_t f) {
    if (k == 0) return 1u << kQRansBits;
    if (k == 1) return 0xFFFFFFFFu;
    if (k == 2) return 1u;
    if (k == 3) return 0xFFFFFFFEu;
    if (k < 4 + 3 * 31) { const uint32_t p = 2u << ((k - 4) / 3); return p - 1u + (k - 4) % 3; }          // 2^j - 1, 2^j, 2^j + 1 for j = 1 .. 31
    if (k < kQRansSelftestFixed) {                                                                         // xorshift32 values, a seed per k
        uint32_t v = 0x9E3779B9u * (k + 1u);
        for (int i = 0; i < 3; i++) { v ^= v << 13; v ^= v >> 17; v ^= v << 5; }
        return v ? v : 1u;
    }
    return (f << 17) - 1u + (k - kQRansSelftestFixed);
}
// 0 when both routines agree with 64-bit division on operand k of f, else 1.
QR_HD uint32_t q_rans_selftest_one(uint32_t k, uint32_t f) {
    const uint32_t x = q_rans_selftest_operand(k, f);
    const float rf = q_rans_rcp(f);
    const uint32_t want = uint32_t(uint64_t(x) / uint64_t(f));
    uint32_t bad = q_rans_quot(x, f, rf) != want ? 1u : 0u;
    if (x < (f << 17)) {
        uint32_t r;
        const uint32_t q = q_rans_quot17(x, f, rf, &r);
        bad |= (q != want || r != x - want * f) ? 1u : 0u;
    }
    return bad;
}

}  // namespace nblic
