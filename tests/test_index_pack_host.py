"""CPU suite: the packed seek index (csrc/index_pack.h).  Indexes are put together by hand, byte by
byte, as tests/test_seek_index_host.py does, so no call touches a GPU.  ``ref_pack`` below is a NumPy / big-integer
restatement of the format written from DESIGN.md: the library's packed bytes are compared with that independent writer,
not only read back by the library's own reader.

What an index has to satisfy to pass ``nblic_amd_index_check`` bounds what can be packed THROUGH THE LIBRARY: counters obey
c0, c1 >= 1 and c0 + c1 <= 8192 (their halves never differ by 16 bits), B is finite, the rank bytes are the inverse of the
symbol bytes, and every coded part of a real layout is a whole number of 64-unit blocks.  Full-range counters, width-64
fields, NaN, rank bytes that are not the inverse and last blocks of 1 and 63 units are run on index_pack.h itself by
tools/index_pack_check.cpp, which test_standalone_check_under_sanitizers compiles and runs."""
import hashlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = ("nblic_amd_index_pack", "nblic_amd_index_pack_bound", "nblic_amd_index_unpack", "nblic_amd_index_unpacked_bytes",
       "nblic_amd_index_is_packed")
MODES = [(0, 1), (0, 2), (0, 3), (1, 0)]                                       # (kind, effort): NBLIC -e1 .. -e3, QNBLIC
STRIDE = {0: 0, 1: 0, 2: 64, 3: 128}                                           # doubles of B per column


# ---- indexes by hand -------------------------------------------------------------------------------------------------------
def parts(kind, w, effort):
    """(offset in the body, bytes, unit, code, initial table) of every part, in body order."""
    rows = 2 * w
    if kind == 0:
        bb = 8 * STRIDE[effort] * w
        p = [(0, 64, 4, "raw", None), (64, 8192, 4, "diff", "zero"), (64 + 8192, 16384, 2, "diff", "counters"),
             (64 + 24576, 40960, 4, "diff", "hits"), (64 + 65536, 10240, 4, "rank", None), (64 + 75776, 10240, 4, "xor", "syms")]
        if bb:
            p.append((86080, bb, 8, "int64", None))
        return p + [(86080 + bb, rows, 4, "raw", None)]
    return [(0, 64, 4, "raw", None), (64, 12288, 4, "diff", "zero"), (12352, rows, 4, "raw", None), (12352 + rows, 24576, 4, "xor", "zero")]


def initial(name, n):
    """The first n units of a table a fresh decoder starts from."""
    i = np.arange(n, dtype=np.uint64)
    if name == "counters":
        return np.full(n, 32, np.uint64)
    if name == "hits":
        return 2 * (19 - i % 20)
    if name == "syms":
        return (0x03020100 + 0x04040404 * (i % 5)).astype(np.uint64)
    return np.zeros(n, np.uint64)


def rank_inverse(sym):
    sym = np.asarray(sym, np.uint8).reshape(512, 20)
    rank = np.zeros((512, 20), np.uint8)
    m = np.arange(512)
    for i in range(20):                                                        # the last i that names a symbol wins; 0 for one never named
        named = sym[:, i] < 20
        rank[m[named], sym[named, i]] = i
    return rank.reshape(-1)


def fresh_tables(kind, w, effort):
    t = {"ctx": np.zeros(3072 if kind else 2048, np.int32), "rows": np.zeros(2 * w, np.uint8)}
    if kind == 0:
        t["cnt"] = np.full(4096, 32 | (32 << 16), np.uint32)
        t["hits"] = initial("hits", 10240).astype(np.int32)
        t["sym"] = np.tile(np.arange(20, dtype=np.uint8), 512)
        t["rank"] = rank_inverse(t["sym"])
        t["B"] = np.zeros(STRIDE[effort] * w, np.float64)
    else:
        freq = np.zeros((12, 256), np.uint32)
        freq[:, :128] = 256                                                    # every table sums to 32768
        start = np.concatenate([np.zeros((12, 1), np.uint32), np.cumsum(freq, axis=1, dtype=np.uint32)[:, :-1]], axis=1)
        t["tab"] = np.concatenate([freq.reshape(-1), start.reshape(-1)])
    return t


def body_of(kind, next_row, t):
    state = struct.pack("<iiQIIIiQi20x", next_row, 0, 100, 0, 0xFFFFFFFF, 0, 0, 0, 0)
    if kind == 0:
        return b"".join([state, t["ctx"].tobytes(), t["cnt"].tobytes(), t["hits"].tobytes(), t["rank"].tobytes(), t["sym"].tobytes(),
                         t["B"].tobytes(), t["rows"].tobytes()])
    return b"".join([state, t["ctx"].tobytes(), t["rows"].tobytes(), t["tab"].tobytes()])


def entry_of(kind, effort, h, w, every, next_row, t):
    body = body_of(kind, next_row, t)
    sha_state = bytes(32) + struct.pack("<Q", next_row * w) + bytes(64)
    head = b"NBLDCKPT" + struct.pack("<I8iIQQ", 1, kind, h, w, 0, 3, effort, every, next_row, 0, 0, len(body)) + sha_state
    assert len(head) == 168
    return head + body + hashlib.sha256(head + body).digest()


def stream_of(h, w):
    return b"NBLIC0.3" + bytes([1, 0, h, 0, w, 0, 3, 1]) + bytes(range(200)) * 5   # -n0 -e1, k_step 3 (test_seek_index_host.py)


def index_of(kind, effort, h, w, every, tables, stream=b"x" * 700):
    """tables: one dict per entry (fresh_tables, changed at will)."""
    assert len(tables) == (h - 1) // every
    entries = [entry_of(kind, effort, h, w, every, (k + 1) * every, t) for k, t in enumerate(tables)]
    head = b"NBLSIDX1" + struct.pack("<I8i3IQ", 1, kind, h, w, 0, 3, effort, every, len(entries), 0, 0, 0, len(stream)) + hashlib.sha256(stream).digest()
    body = head + b"".join(struct.pack("<Q", len(e)) + e for e in entries)
    return body + hashlib.sha256(body).digest()


def touched(kind, w, effort, count, rng, wide=False):
    """Tables that change from entry to entry as a decode changes them: sparsely and by little -- or, `wide`, everywhere and by
    as much as a valid index allows (contexts and hit counts over the whole 32 bits, B up to +-2^62, counters over their range)."""
    out, t = [], fresh_tables(kind, w, effort)
    for _ in range(count):
        t = {k: v.copy() for k, v in t.items()}
        t["rows"] = rng.integers(0, 256, 2 * w).astype(np.uint8)
        if wide:
            t["ctx"] = rng.integers(-2 ** 31, 2 ** 31, t["ctx"].size).astype(np.int32)
        else:
            at = rng.integers(0, t["ctx"].size, 50)
            t["ctx"][at] += rng.integers(-300, 300, 50).astype(np.int32)
        if kind == 0:
            if wide:
                c0 = rng.integers(1, 8191, 4096)
                t["cnt"] = (c0 | ((rng.integers(1, 8192, 4096) % (8192 - c0) + 1) << 16)).astype(np.uint32)
                t["hits"] = rng.integers(-2 ** 31, 2 ** 31, 10240).astype(np.int32)
                t["B"] = (rng.integers(-2 ** 31 + 1, 2 ** 31, t["B"].size) * 2.0 ** 31).astype(np.float64)
            else:
                at = rng.integers(0, 4096, 60)
                t["cnt"][at] = (rng.integers(1, 4000, 60) | (rng.integers(1, 4000, 60) << 16)).astype(np.uint32)
                at = rng.integers(0, 10240, 60)
                t["hits"][at] += rng.integers(0, 5, 60).astype(np.int32)
                if t["B"].size:
                    at = rng.integers(0, t["B"].size, 80)
                    t["B"][at] += rng.integers(-100000, 100000, 80)
            sym = t["sym"].reshape(512, 20)
            for m in rng.integers(0, 512, 512 if wide else 30):
                sym[m] = rng.permutation(20)
            t["rank"] = rank_inverse(t["sym"])
        out.append(t)
    return out


# ---- the format, restated ------------------------------------------------------------------------------
def code_blocks(values):
    """Width bytes, then payloads: per block of 64 values the bits of the largest, then 8 b bytes, value i at bit i b."""
    widths, payloads = bytearray(), bytearray()
    for b0 in range(0, len(values), 64):
        blk = [int(v) for v in values[b0:b0 + 64]]
        b = max(blk).bit_length()
        widths.append(b)
        payloads += sum(v << (i * b) for i, v in enumerate(blk)).to_bytes(8 * b, "little")
    return bytes(widths + payloads)


def zigzag(d, bits):
    """d: signed differences modulo 2^bits, as Python ints."""
    mask = (1 << bits) - 1
    return [((v << 1) ^ (mask if v >> (bits - 1) else 0)) & mask for v in d]


def ref_pack_body(prev, body, kind, w, effort, marks, at0):
    out = bytearray([1])
    P = parts(kind, w, effort)
    for j, (at, n, unit, code, init) in enumerate(P):
        src = body[at:at + n]
        flag, data = 0, src
        dt = {2: "<u2", 4: "<u4", 8: "<u8"}[unit]
        if code in ("diff", "xor"):
            x = [int(v) for v in np.frombuffer(src, dt)]
            base = [int(v) for v in (np.frombuffer(prev[at:at + n], dt) if prev is not None else initial(init, n // unit))]
            bits = 8 * unit
            vals = zigzag([(a - b) & ((1 << bits) - 1) for a, b in zip(x, base)], bits) if code == "diff" else [a ^ b for a, b in zip(x, base)]
            flag, data = 1, code_blocks(vals)
        elif code == "int64":
            v = np.frombuffer(src, "<f8")
            ok = np.isfinite(v).all() and (np.abs(v) < 2.0 ** 62).all() and (v == np.trunc(v)).all() and not (np.signbit(v) & (v == 0)).any()
            if ok:
                flag, data = 1, code_blocks(zigzag([int(a) & (2 ** 64 - 1) for a in v], 64))
        elif code == "rank":
            if rank_inverse(np.frombuffer(body[P[j + 1][0]:P[j + 1][0] + 10240], np.uint8)).tobytes() == src:
                flag, data = 2, b""
        out.append(flag)
        marks.append(at0 + len(out))                                           # where the part's data starts
        out += data
    if len(out) >= 1 + len(body):
        del marks[-len(P):]
        return bytes([0]) + body
    return bytes(out)


def ref_pack(index, marks=None):
    """The packed form of a (valid) index.  marks, when given, receives every structural boundary of the result."""
    marks = [] if marks is None else marks
    kind, h, w, _, _, effort, every, count = struct.unpack_from("<8i", index, 12)
    out = bytearray(b"NBLSIDXP" + struct.pack("<I", 1) + index[12:96] + index[-32:])
    marks += [8, 96, 128]
    at, prev = 96, None
    for _ in range(count):
        n = struct.unpack_from("<Q", index, at)[0]
        e = index[at + 8:at + 8 + n]
        at += 8 + n
        body = e[168:-32]
        start = len(out) + 8
        pe = bytearray(e[:168])
        marks += [len(out), start, start + 168]
        pe += ref_pack_body(prev, body, kind, w, effort, marks, start + 168)
        marks.append(start + len(pe))
        pe += e[-32:]
        marks.append(start + len(pe))
        pe += hashlib.sha256(pe).digest()
        out += struct.pack("<Q", len(pe)) + pe
        prev = body
    marks.append(len(out))
    return bytes(out + hashlib.sha256(out).digest())


def part_marks(packed, marks, entry, n_parts):
    """Where the data of each part of a coded packed entry starts (its flag byte sits in front)."""
    at = 128
    for _ in range(entry):
        at += 8 + struct.unpack_from("<Q", packed, at)[0]
    first = marks.index(at + 8 + 168) + 1
    return marks[first:first + n_parts]


def reseal(b):
    return b[:-32] + hashlib.sha256(b[:-32]).digest()


def rehash_entries(packed):
    """Every packed entry's hash and the outer one made right again after a change inside."""
    b = bytearray(packed)
    count = struct.unpack_from("<i", b, 40)[0]
    at = 128
    for _ in range(count):
        n = struct.unpack_from("<Q", b, at)[0]
        b[at + 8 + n - 32:at + 8 + n] = hashlib.sha256(b[at + 8:at + 8 + n - 32]).digest()
        at += 8 + n
    return reseal(bytes(b))


def round_trip(pkg, ix, smaller=True):
    packed = pkg.pack_index(ix)
    assert packed == ref_pack(ix), "the library's packed bytes differ from the independent writer's"
    assert pkg.index_is_packed(packed) and not pkg.index_is_packed(ix)
    assert len(packed) <= pkg.pack_index_bound(ix) == len(ix) + 32 + 33 * struct.unpack_from("<i", ix, 40)[0]
    assert pkg.check_index(packed)
    assert pkg.unpack_index(packed) == ix
    assert pkg.index_entries(packed) == pkg.index_entries(ix)
    if smaller:
        assert len(packed) < len(ix)
    return packed


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = open(pkg.INCLUDE).read()
    for name in API:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b" + name + r"\s*\(", text), name


@pytest.mark.parametrize("kind,effort", MODES)
def test_untouched_tables_cost_one_byte_per_block(pkg, kind, effort):
    h, w, every = 7, 5, 2
    ix = index_of(kind, effort, h, w, every, [fresh_tables(kind, w, effort) for _ in range(3)])
    assert pkg.check_index(ix)
    packed = round_trip(pkg, ix)
    coded = sum(-(-n // unit // 64) for _, n, unit, code, _ in parts(kind, w, effort) if code in ("diff", "xor", "int64"))
    raw = sum(n for _, n, _, code, _ in parts(kind, w, effort) if code == "raw")
    per_entry = 8 + 168 + 1 + len(parts(kind, w, effort)) + coded + raw + 64     # every width byte is 0: no payload at all
    lens, at = [], 128
    for _ in range(3):
        lens.append(8 + struct.unpack_from("<Q", packed, at)[0])
        at += lens[-1]
    assert at + 32 == len(packed)
    assert lens[1:] == [per_entry, per_entry]
    assert lens[0] == per_entry if kind == 0 else lens[0] > per_entry          # (QNBLIC's tables are the stream's: entry 0 carries them)


@pytest.mark.parametrize("kind,effort", MODES)
@pytest.mark.parametrize("w", [5, 6])                                          # odd W; W = 2 (mod 4)
def test_changing_tables_round_trip(pkg, kind, effort, w):
    rng = np.random.default_rng(100 * kind + 10 * effort + w)
    ix = index_of(kind, effort, 9, w, 2, touched(kind, w, effort, 4, rng))
    assert pkg.check_index(ix)
    round_trip(pkg, ix)


@pytest.mark.parametrize("kind,effort", [(0, 1), (0, 3), (1, 0)])
def test_full_range_tables_stay_within_the_bound(pkg, kind, effort):
    rng = np.random.default_rng(7 + effort)
    w = 3
    tables = touched(kind, w, effort, 2, rng, wide=True)
    ix = index_of(kind, effort, 5, w, 2, tables)
    assert pkg.check_index(ix)
    packed = round_trip(pkg, ix, smaller=False)
    if kind == 0:                                                              # widths 32 (contexts) and, at -e3, 63 (B)
        marks = []
        ref_pack(ix, marks)
        pm = part_marks(packed, marks, 1, len(parts(kind, w, effort)))
        assert packed[pm[1] - 1] == 1 and 32 in packed[pm[1]:pm[1] + 32]
        assert effort != 3 or (packed[pm[6] - 1] == 1 and 63 in packed[pm[6]:pm[6] + 6])


def test_one_entry_and_sixty_four(pkg):
    rng = np.random.default_rng(3)
    round_trip(pkg, index_of(0, 1, 20, 24, 19, touched(0, 24, 1, 1, rng)))
    round_trip(pkg, index_of(1, 0, 65, 4, 1, touched(1, 4, 0, 64, rng)))
    round_trip(pkg, index_of(0, 1, 65, 3, 1, touched(0, 3, 1, 64, rng)))


@pytest.mark.parametrize("value", [0.5, -0.0, 2.0 ** 63])
def test_b_that_int64_does_not_reproduce_goes_raw(pkg, value):
    rng = np.random.default_rng(11)
    tables = touched(0, 6, 2, 2, rng)
    tables[1]["B"][17] = value
    ix = index_of(0, 2, 5, 6, 2, tables)
    assert pkg.check_index(ix)
    packed = round_trip(pkg, ix)
    marks = []
    ref_pack(ix, marks)
    assert [packed[m - 1] for m in part_marks(packed, marks, 0, 8)] == [0, 1, 1, 1, 2, 1, 1, 0]      # B of entry 0: coded
    assert [packed[m - 1] for m in part_marks(packed, marks, 1, 8)] == [0, 1, 1, 1, 2, 1, 0, 0]      # B of entry 1: raw


def test_what_the_check_refuses_is_not_packed(pkg):
    """NaN in B and rank bytes that are not the inverse never pass nblic_amd_index_check, so pack_index refuses them (the
    raw flags that would carry them are exercised by tools/index_pack_check.cpp)."""
    rng = np.random.default_rng(12)
    for damage in ("nan", "rank"):
        tables = touched(0, 6, 2, 2, rng)
        if damage == "nan":
            tables[1]["B"][3] = np.nan
        else:
            tables[1]["rank"][7] ^= 1
        ix = index_of(0, 2, 5, 6, 2, tables)
        assert not pkg.check_index(ix)
        with pytest.raises(ValueError):
            pkg.pack_index(ix)
    good = index_of(0, 1, 5, 3, 2, touched(0, 3, 1, 2, rng))
    for bad in (b"", b"junk", good[:-1], good[:200], bytes(4096), good[:-32] + bytes(32), pkg.pack_index(good)):
        with pytest.raises(ValueError):
            pkg.pack_index(bad)
        assert pkg.pack_index_bound(bad[:90]) == 0


def refused(pkg, b):
    assert not pkg.check_index(b)
    with pytest.raises(ValueError):
        pkg.unpack_index(b)
    with pytest.raises(ValueError):
        pkg.index_entries(b)


def test_refuses_cut_damaged_and_junk(pkg):
    rng = np.random.default_rng(13)
    ix = index_of(0, 2, 7, 5, 2, touched(0, 5, 2, 3, rng))
    marks = []
    good = ref_pack(ix, marks)
    assert good == pkg.pack_index(ix)
    # cut at every structural boundary, and a byte to either side; the seal made right again where there is room
    for m in sorted(set(marks + [0, len(good) - 1])):
        for n in (m - 1, m, m + 1):
            if 0 <= n < len(good):
                refused(pkg, good[:n])
                if n >= 32 and n + 32 != len(good):
                    refused(pkg, good[:n] + hashlib.sha256(good[:n]).digest())
    # a width byte of 33 for a 4-byte unit (the contexts of entry 1), every hash made right
    n0 = struct.unpack_from("<Q", good, 128)[0]
    ctx1 = part_marks(good, marks, 1, 8)[1]
    b = bytearray(good)
    assert b[ctx1 - 1] == 1 and b[ctx1] <= 32
    b[ctx1] = 33
    refused(pkg, rehash_entries(bytes(b)))
    # a packed length pointing past the end
    for n in (len(good), 2 ** 64 - 8, 0, 100):
        b = bytearray(good)
        struct.pack_into("<Q", b, 128, n)
        refused(pkg, reseal(bytes(b)))
    # a flipped payload bit: the entry's hash catches it
    b = bytearray(good)
    b[ctx1 + 40] ^= 1
    refused(pkg, reseal(bytes(b)))
    # ... and with every hash made right the packed form is sound, but it no longer unpacks to the entry its seal names
    rows1 = 128 + 8 + n0 + 8 + struct.unpack_from("<Q", good, 128 + 8 + n0)[0] - 64 - 3
    b = bytearray(good)
    b[rows1] ^= 4                                                              # inside the raw rows of entry 1
    b = rehash_entries(bytes(b))
    assert pkg.check_index(b)
    with pytest.raises(ValueError):
        pkg.unpack_index(b)
    # junk
    for j in (b"", b"x", b"NBLSIDXP", bytes(128 + 32), bytes(4096), b"NBLSIDXP" + bytes(500), b"NBLSIDXQ" + good[8:],
              good[:8] + struct.pack("<I", 2) + good[12:], good[:-32] + bytes(32), good + b"\0"):
        refused(pkg, j)
    assert pkg.load_library().nblic_amd_index_unpacked_bytes(None, 0) == 0
    assert not pkg.index_is_packed(b"NBLSIDX")


def test_refuses_the_wrong_stream(pkg):
    h, w = 5, 3
    stream = stream_of(h, w)
    rng = np.random.default_rng(14)
    ix = index_of(0, 1, h, w, 2, touched(0, w, 1, 2, rng), stream)
    packed = round_trip(pkg, ix)
    assert pkg.check_index(ix, stream) and pkg.check_index(packed, stream)
    other = stream[:-1] + bytes([stream[-1] ^ 1])
    for s in (other, stream + b"\0", stream_of(h, w + 1)):
        assert not pkg.check_index(packed, s)


def test_entries_out_of_order_are_refused_in_packed_form(pkg):
    """The packed check reads the entry heads as the unpacked one does: rows in order, spacing, feed_from."""
    rng = np.random.default_rng(15)
    good = pkg.pack_index(index_of(0, 1, 7, 3, 2, touched(0, 3, 1, 3, rng)))
    n0 = struct.unpack_from("<Q", good, 128)[0]
    at = 128 + 8 + n0 + 8                                                      # entry 1's checkpoint head
    for off, fmt, v in ((40, "<i", 2), (36, "<i", 3), (48, "<Q", 512), (56, "<Q", 5)):      # next_row, band_rows, feed_from, body_bytes
        b = bytearray(good)
        struct.pack_into(fmt, b, at + off, v)
        assert not pkg.check_index(rehash_entries(bytes(b))), off


def test_standalone_check_under_sanitizers(tmp_path):
    """tools/index_pack_check.cpp: index_pack.h alone, with its own main, under the address and undefined-behaviour
    sanitizers (nothing of it is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "index_pack_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "index_pack_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "index_pack_check ok" in r.stdout
