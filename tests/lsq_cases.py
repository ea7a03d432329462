"""Least-squares systems for the tests of the efforts 2 / 3 solvers (csrc/lsq_f64.h, serial_engine.hip solve_with /
lsq_solve_int): the CPU harness (tests/host_harness.cpp) behind ctypes, the systems it records while it codes hard-edged
planes, and systems placed on the four limits of lsq::Guard.  Pure integers, no RNG: the same systems on every machine.
Not a test module; test_lsq_limits.py, test_host_logic.py and the GPU suites import it."""
import ctypes as C
import os
import subprocess

import numpy as np

import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p = C.POINTER(C.c_uint8)

# lsq_f64.h Guard::ok, stated a second time on purpose: a limit changed there must not change what the tests expect
LIMITS = {"product": 2 ** 62, "entry": 2 ** 44, "quotient": 2 ** 46, "pivot": 2 ** 38}
QUANTITIES = ["product", "entry", "quotient", "pivot"]           # the order of the Guard's maxima in every record
TOP_Q12 = 255 << 12


class HhSystems(C.Structure):
    _fields_ = [("cap", C.c_long), ("count", C.c_long), ("every", C.c_int), ("D", C.POINTER(C.c_double)),
                ("vn", C.POINTER(C.c_int8)), ("bias", C.POINTER(C.c_int)), ("redo", u8p)]


_lib = None


def load_harness():
    global _lib
    if _lib is not None:
        return _lib
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhost_harness.so")
    src = os.path.join(ROOT, "tests", "host_harness.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.hh_model_encode.restype = C.c_long
    lib.hh_model_encode.argtypes = [u8p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.c_long, C.POINTER(C.c_long),
                                    C.POINTER(C.c_long), C.POINTER(HhSystems)]
    lib.hh_lsq_solve.restype = None
    lib.hh_lsq_solve.argtypes = [C.c_int, C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_int8), C.POINTER(C.c_int),
                                 C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    lib.hh_check_divide_free.restype = C.c_long
    lib.hh_check_lane_front.restype = C.c_long
    lib.hh_check_symbol_lanes.restype = C.c_long
    lib.hh_check_lane_front.argtypes = [C.c_int, C.c_int]
    _lib = lib
    return lib


def order_of(effort):
    return {2: 6, 3: 10}.get(effort, 0)


def vec_len(n):
    return 1 + n + n * n


def model_encode(lib, img, near, effort, dump_cap=0, every=0):
    """The harness's encode of one plane: (coded bins, reconstruction, redo solves, (system 0, system 1), systems).
    systems = (D, vn, bias, redo) of the pixels the harness recorded (dump_cap > 0), else None."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    rec = np.empty_like(img)
    coded = np.empty(40 * h * w + 64, np.uint16)
    fb, by = C.c_long(0), (C.c_long * 2)()
    dump, arrays = None, None
    if dump_cap > 0:
        m = vec_len(order_of(effort))
        arrays = (np.zeros((dump_cap, m), np.float64), np.zeros((dump_cap, 10), np.int8), np.zeros(dump_cap, np.int32), np.zeros(dump_cap, np.uint8))
        dump = HhSystems(dump_cap, 0, every, arrays[0].ctypes.data_as(C.POINTER(C.c_double)), arrays[1].ctypes.data_as(C.POINTER(C.c_int8)),
                         arrays[2].ctypes.data_as(C.POINTER(C.c_int)), arrays[3].ctypes.data_as(u8p))
    n = lib.hh_model_encode(img.ctypes.data_as(u8p), rec.ctypes.data_as(u8p), h, w, near, effort, coded.ctypes.data_as(C.POINTER(C.c_uint16)),
                            coded.size, C.byref(fb), by, C.byref(dump) if dump is not None else None)
    systems = None
    if dump is not None:
        assert dump.count <= dump_cap, "the harness recorded more systems than asked for"
        systems = tuple(a[:dump.count].copy() for a in arrays)
    return coded[:n], rec, int(fb.value), (int(by[0]), int(by[1])), systems


def redo_pixels(lib, img, near, effort):
    """(system 0, system 1) solves the CPU harness redoes with integers while it codes the plane."""
    return model_encode(lib, img, near, effort)[3]


def solve_host(lib, n, D, vn, bias):
    """hh_lsq_solve: per item (K, 10) int64 [int p0 p1 | int ok0 ok1 | f64 p0 p1 | f64 ok0 ok1 | guard ok0 ok1] and
    (K, 8) float64 Guard maxima (QUANTITIES of system 0, then of system 1)."""
    D = np.ascontiguousarray(D, np.float64)
    vn = np.ascontiguousarray(vn, np.int8)
    bias = np.ascontiguousarray(bias, np.int32)
    k = bias.shape[0]
    assert D.shape == (k, vec_len(n)) and vn.shape == (k, 10)
    oi, of = np.zeros((k, 10), np.int64), np.zeros((k, 8), np.float64)
    lib.hh_lsq_solve(n, k, D.ctypes.data_as(C.POINTER(C.c_double)), vn.ctypes.data_as(C.POINTER(C.c_int8)), bias.ctypes.data_as(C.POINTER(C.c_int)),
                     oi.ctypes.data_as(C.POINTER(C.c_longlong)), of.ctypes.data_as(C.POINTER(C.c_double)))
    return oi, of


def bias_pair(bias):
    """lsq_f64.h bias_pair (NBLIC.c:837-842)."""
    clip = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    b1 = clip(clip(bias * 21 // 22, -1, bias - 1), 0, 4096)
    b2 = clip(clip(bias * 22 // 21, bias + 1, 4097), 0, 4096)
    return b1, b2


# ---- recorded systems ------------------------------------------------------------------------------------------------
# Planes and modes of the table in DESIGN.md ("what trips the guard"): every redo pixel and as many ordinary ones; plus
# `const` (zero pivots: half its solves have no solution) and `syn1` (row exchanges and pivot ties), every k-th pixel.
def recorded(lib, n):
    effort = 2 if n == 6 else 3
    modes = [(2, 2), (9, 2)] if n == 6 else [(1, 3), (2, 3), (3, 3), (9, 3)]
    planes = [inputs.make_hard("step_v", 64, 64), inputs.make_hard("step_v", 33, 57), inputs.make_hard("step_v", 24, 1500),
              inputs.make_hard("stripes_h", 64, 64), inputs.make_hard("stripes_h", 24, 1500), inputs.make_hard("step_h", 24, 1500),
              inputs.make("checker", 24, 1500)]
    parts = []
    for img in planes:
        for near, _ in modes:
            parts.append(model_encode(lib, img, near, effort, dump_cap=4096)[4])
    parts.append(model_encode(lib, inputs.make("const", 17, 13), 0, effort, dump_cap=4096, every=3)[4])
    parts.append(model_encode(lib, inputs.make("syn1", 64, 64), 0, effort, dump_cap=4096, every=16)[4])
    parts.append(model_encode(lib, inputs.make("syn1", 40, 37), 2, effort, dump_cap=4096, every=8)[4])
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


# ---- systems placed on the limits ----------------------------------------------------------------------------------
# Two families, both made from recorded ORDINARY systems (all four maxima inside the limits):
#  scaled   [b | A] times 2^k, k chosen per limit so that the system's own largest product / entry / pivot lands within a
#           factor two below, on, and a factor two above the limit: dense systems with real row exchanges on either side;
#  planted  the last two rows and columns are cut loose from the rest (zero cross entries) and filled so that ONE
#           magnitude is known exactly.  With i = n-2, j = n-1, the block [[a 0 | bi] [l e | bj]] (|l| <= a) is reached at
#           the last elimination step, row i is its pivot, and the only non-zero product it makes is bi * l; the divisors
#           it adds are a and e, the entries bi, bj - trunc(bi l / a) and e, the quotients (4 vn b + d/2) / d of its two
#           rows.  So  pivot = e,  entry = bj (l = 0),  quotient = vn bj (e = 4, l = 0: (4 vn bj + 2) / 4, which the Guard
#           sees as |vn bj +- 1/2| shortened by 2^-48, i.e. less than one from the integer),  product = bi * l  are set to
#           limit / 2, limit - 1, limit, limit + 1, 2 limit (and, for the product, past 2^63 and 2^64 where the
#           reference's int64 multiply wraps: the integer path must reproduce the wrapped value).  The quotient's factors
#           (QUOTIENT_FACTORS) keep bj below the entry limit: 2^46 - 1 = 47 x ..., 2^46 + 1 = 5 x ...
#           The leading (n-2) x (n-2) part is the recorded system's and eliminates as usual.
# Every item carries the system slot it aims at (the diagonal is set for that slot's regularisation; the other slot's
# differs by (b2 - b1) n, i.e. lands next to the limit too -- except the quotient, whose divisor 4 the other slot's
# regularisation changes altogether), alternating, so slot 1 is filled as often as slot 0.
PRODUCT_FACTORS = [(2 ** 30, 2 ** 31), (2 ** 31 - 1, 2 ** 31 + 1), (2 ** 31, 2 ** 31), (2147549185, 2147418113), (2 ** 32, 2 ** 31),
                   (2 ** 31 + 5, 2 ** 30 - 3), (2 ** 32 + 1, 2 ** 32), (2 ** 33 - 1, 2 ** 31 + 7)]
assert [p * q - 2 ** 62 for p, q in PRODUCT_FACTORS[1:4]] == [-1, 0, 1] and PRODUCT_FACTORS[0][0] * PRODUCT_FACTORS[0][1] == 2 ** 61 \
    and PRODUCT_FACTORS[4][0] * PRODUCT_FACTORS[4][1] == 2 ** 63 and PRODUCT_FACTORS[6][0] * PRODUCT_FACTORS[6][1] > 2 ** 64


QUOTIENT_FACTORS = [(64, 2 ** 39), (47, (2 ** 46 - 1) // 47), (64, 2 ** 40), (5, (2 ** 46 + 1) // 5), (64, 2 ** 41)]     # (vn, bj)
assert [v * b for v, b in QUOTIENT_FACTORS] == [2 ** 45, 2 ** 46 - 1, 2 ** 46, 2 ** 46 + 1, 2 ** 47] and all(b < 2 ** 44 for _, b in QUOTIENT_FACTORS)


def around(limit):
    return [limit // 2, limit - 1, limit, limit + 1, 2 * limit]


def _planted(n, D, vn, bias, slot, a, l, e, bi, bj, vn_j=None):
    """The recorded system with the block planted for system slot `slot`; integers in, float64 row out."""
    i, j = n - 2, n - 1
    bs = bias_pair(int(bias))[slot]
    d = [int(v) for v in D]
    A = lambda r, c: 1 + n + r * n + c
    for r in range(n - 2):
        for c in (i, j):
            d[A(r, c)] = 0
            d[A(c, r)] = 0
    d[A(i, i)] = a - bs * n
    d[A(i, j)] = 0
    d[A(j, i)] = l
    d[A(j, j)] = e - bs * n
    d[1 + i] = bi - bs * 1024
    d[1 + j] = bj - bs * 1024
    v = np.array(vn, np.int8)
    if vn_j is not None:
        v[j] = vn_j
    assert all(abs(x) < 2 ** 52 for x in d)
    return np.array(d, np.float64), v


def limit_placed(lib, n, rec, want):
    """At least `want` systems on the limits from the recorded ones: (D, vn, bias, target), target = (family, quantity, value, slot)."""
    D, vn, bias, redo = rec
    hi, hf = solve_host(lib, n, D, vn, bias)
    ordinary = [k for k in range(len(bias)) if redo[k] == 0 and hi[k, 2] and hi[k, 3] and hi[k, 8] and hi[k, 9]]
    assert len(ordinary) >= 32
    out_D, out_vn, out_bias, targets = [], [], [], []
    t = 0
    while len(out_bias) < want:
        k = ordinary[(t * 7) % len(ordinary)]
        slot, sign = t & 1, -1 if t & 2 else 1
        # scaled: the system's own maxima (of slot `slot`) to the limit
        for qi, q in ((0, "product"), (1, "entry"), (3, "pivot")):
            have = max(hf[k, 4 * slot + qi], 1.0)
            k0 = int(np.ceil(np.log2(LIMITS[q] / have) / (2 if q == "product" else 1)))
            for dk in (-1, 0, 1):
                d = [int(v) * 2 ** (k0 + dk) if idx else int(v) for idx, v in enumerate(D[k])]
                if max(abs(x) for x in d) >= 2 ** 51:
                    continue
                out_D.append(np.array(d, np.float64)); out_vn.append(vn[k]); out_bias.append(bias[k])
                targets.append(("scaled", q, None, slot))
        # planted
        for T in around(LIMITS["pivot"]):
            row, v = _planted(n, D[k], vn[k], bias[k], slot, 2 ** 20 + 3, 0, sign * T, 1000 + t % 977, -(3000 + t % 331))
            out_D.append(row); out_vn.append(v); out_bias.append(bias[k]); targets.append(("planted", "pivot", T, slot))
        for T in around(LIMITS["entry"]):
            row, v = _planted(n, D[k], vn[k], bias[k], slot, 2 ** 20 + 3, 0, 2 ** 36 + t % 1013, 1000 + t % 977, sign * T)
            out_D.append(row); out_vn.append(v); out_bias.append(bias[k]); targets.append(("planted", "entry", T, slot))
        for vq, bq in QUOTIENT_FACTORS:
            row, v = _planted(n, D[k], vn[k], bias[k], slot, 2 ** 20 + 3, 0, 4, 1000 + t % 977, sign * bq, vn_j=vq)
            out_D.append(row); out_vn.append(v); out_bias.append(bias[k]); targets.append(("planted", "quotient", vq * bq, slot))
        for p, q in PRODUCT_FACTORS:
            row, v = _planted(n, D[k], vn[k], bias[k], slot, 2 ** 33 + 2 ** 20 + t % 4099, sign * q, 2 ** 24 + t % 1013, p, 1000 + t % 977)
            out_D.append(row); out_vn.append(v); out_bias.append(bias[k]); targets.append(("planted", "product", p * q, slot))
        t += 1
    return np.array(out_D), np.array(out_vn, np.int8), np.array(out_bias, np.int32), targets


_cache = {}


def systems(lib, n, at_least=4096):
    """Recorded + limit-placed systems of order n and what the host solvers make of them:
    dict(D, vn, bias, targets (None for recorded items), n_recorded, host_i64, host_f64)."""
    if n in _cache:
        return _cache[n]
    rec = recorded(lib, n)
    placed = limit_placed(lib, n, rec, max(at_least - len(rec[2]), 3072))
    D = np.concatenate([rec[0], placed[0]])
    vn = np.concatenate([rec[1], placed[1]])
    bias = np.concatenate([rec[2], placed[2]])
    hi, hf = solve_host(lib, n, D, vn, bias)
    _cache[n] = dict(D=D, vn=vn, bias=bias, targets=[None] * len(rec[2]) + placed[3], n_recorded=len(rec[2]), recorded_redo=rec[3],
                     host_i64=hi, host_f64=hf)
    return _cache[n]


def clamp_q12(p):
    return np.clip(p, 0, TOP_Q12)
