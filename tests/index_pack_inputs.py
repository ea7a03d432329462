"""Packed seek indexes for the unpack kernels' tests (test_index_pack_inputs_host.py, test_index_unpack_kernels.py): packings
the library's writer never makes of indexes put together by hand (test_index_pack_host.py index_of), and tables chosen
VALUE FIRST, so that every width byte the format allows occurs.  No test functions here.

``pack`` is a writer of the format of DESIGN.md section 6 that is free where csrc/index_pack.h packed_walk is free: any
width byte at or above a block's minimum, any part raw, the rank bytes raw instead of left out, a whole body raw in the
middle of a chain.  With "min" everywhere it writes what test_index_pack_host.ref_pack writes, byte for byte.

``graded_tables`` picks the coded values and derives the tables from them: block k of entry e of every coded part holds
values whose largest has exactly (k + e) mod (8 unit + 1) bits, the top bit in lane 0 (even entries) or lane 63 (odd
ones).  Diff and xor tables follow from the previous entry's.  The doubles of B follow as double(unzigzag(value)), which
has to be an integer of magnitude below 2^62 that a double reproduces: a B block is CAPPED AT 63 BITS (a graded width of
64 becomes 63; width 64 of an 8-byte unit comes from the "full" and "rand" packings alone), a value's magnitude keeps its 53
leading bits, and the lane that carries a block's top bit holds a positive double.  The graded counters are not ones a
decoder can have (their halves differ over the full 16 bits, c0 + c1 may pass 8192); nblic_amd_index_check refuses them, and
the structural walk does not look.

``walk`` reads the flags and width bytes back out of packed bytes; the coverage conditions of the host test are computed
with it from what was written, not from what was asked for.

Fixed seeds, numpy and Python integers only.
"""
import hashlib
import struct

import numpy as np

from test_index_pack_host import fresh_tables, index_of, initial, parts, rank_inverse, touched, zigzag

GEOMETRIES = [((37, 29, 5), (0, 1)), ((37, 29, 5), (0, 2)), ((37, 29, 5), (0, 3)), ((37, 29, 5), (1, 0)),      # 7 entries; odd W
              ((37, 30, 5), (0, 1)), ((37, 30, 5), (0, 2)), ((37, 30, 5), (0, 3)), ((37, 30, 5), (1, 0)),      # B doubles at 4 mod 8
              ((13, 161, 1), (0, 1)), ((13, 161, 1), (1, 0))]                  # 12 entries; a row slot of 322 bytes: two raw blocks, the second short
BASE_OFFSETS = (0, 1, 2, 3)
_DT = {2: "<u2", 4: "<u4", 8: "<u8"}


# ---- the writer ----------------------------------------------------------------------------------------------------------
def _min_widths(vals):
    """Per block of 64 values the bits of the largest."""
    m = np.bitwise_or.reduce(vals.reshape(-1, 64), axis=1)
    return np.array([int(v).bit_length() for v in m], np.int64)


def _blocks(vals, widths):
    """The width bytes, then the payloads: lane i of a block of width b at bit i b, little-endian."""
    nb = widths.size
    bits = np.unpackbits(vals.astype("<u8").view(np.uint8).reshape(nb, 64, 8), axis=-1, bitorder="little")
    keep = np.broadcast_to(np.arange(64)[None, None, :] < widths[:, None, None], bits.shape)
    assert not (bits & ~keep).any(), "a value does not fit its block's width"
    return widths.astype(np.uint8).tobytes() + np.packbits(bits[keep], bitorder="little").tobytes()


def _values(prev, body, part):
    """The values of a coded part (uint64), or None when the int64 form does not reproduce its doubles."""
    at, n, unit, code, init = part
    src = body[at:at + n]
    bits = 8 * unit
    mask = (1 << bits) - 1
    if code == "int64":
        v = np.frombuffer(src, "<f8")
        ok = np.isfinite(v).all() and (np.abs(v) < 2.0 ** 62).all() and (v == np.trunc(v)).all() and not (np.signbit(v) & (v == 0)).any()
        return np.array(zigzag([int(a) & mask for a in v], 64), np.uint64) if ok else None
    x = np.frombuffer(src, _DT[unit]).astype(np.uint64)
    base = np.frombuffer(prev[at:at + n], _DT[unit]).astype(np.uint64) if prev is not None else initial(init, n // unit)
    if code == "xor":
        return x ^ base
    return np.array(zigzag([int(d) for d in (x - base) & np.uint64(mask)], bits), np.uint64)


def _pack_body(prev, body, P, e, choose, rng):
    out = bytearray([1])
    for j, part in enumerate(P):
        at, n, unit, code, _ = part
        src = body[at:at + n]
        how = choose(e, j)
        flag, data = 0, src
        if code == "rank":
            inverse = rank_inverse(np.frombuffer(body[P[j + 1][0]:P[j + 1][0] + n], np.uint8)).tobytes() == src
            assert how in ("min", "leftout", "raw")
            if inverse and how != "raw":
                flag, data = 2, b""
        elif code != "raw" and how != "raw":
            assert how in ("min", "full", "rand")
            vals = _values(prev, body, part)
            if vals is not None:                                               # (doubles the int64 form does not reproduce: raw alone carries them)
                w = _min_widths(vals)
                if how == "full":
                    w = np.full(w.size, 8 * unit, np.int64)
                elif how == "rand":
                    w = rng.integers(w, 8 * unit + 1)
                flag, data = 1, _blocks(vals, w)
        out.append(flag)
        out += data
    body_how = choose(e, None)
    assert body_how in ("min", "coded", "raw")
    if body_how == "raw" or (body_how == "min" and len(out) >= 1 + len(body)):
        return bytes([0]) + body
    return bytes(out)


def pack(index, choose, rng):
    """The packed form of an index with choose(entry, part) -> "min" | "full" | "rand" | "raw" for a coded part ("rand": every
    block a width drawn from its minimum .. 8 unit), "leftout" | "raw" for the rank part, and choose(entry, None) -> "coded" |
    "raw" for the body.  "min" is the library's writer's choice everywhere: the smallest widths, the rank bytes left out when
    they are the inverse, the body raw when coding does not make it smaller.  Every hash is made right."""
    kind, h, w, _, _, effort, every, count = struct.unpack_from("<8i", index, 12)
    P = parts(kind, w, effort)
    out = bytearray(b"NBLSIDXP" + struct.pack("<I", 1) + index[12:96] + index[-32:])
    at, prev = 96, None
    for e in range(count):
        n = struct.unpack_from("<Q", index, at)[0]
        entry = index[at + 8:at + 8 + n]
        at += 8 + n
        body = entry[168:-32]
        pe = entry[:168] + _pack_body(prev, body, P, e, choose, rng) + entry[-32:]
        pe += hashlib.sha256(pe).digest()
        out += struct.pack("<Q", len(pe)) + pe
        prev = body
    return bytes(out + hashlib.sha256(out).digest())


def choose_all(how, P):
    """`how` for every coded part and a coded body ("min": the library's writer's choices); the rank bytes left out where they can be."""
    def choose(e, j):
        if j is None:
            return "min" if how == "min" else "coded"
        return "min" if P[j][3] == "rank" else how
    return choose


_MIX = ("rand", "raw", "min", "full", "raw", "rand", "min")


def choose_mix(P, count):
    """Raw parts in front of coded ones of every kind, the rank bytes raw in every third entry, one raw body mid-chain."""
    def choose(e, j):
        if j is None:
            return "raw" if count >= 3 and e == count // 2 else "coded"
        if P[j][3] == "rank":
            return "raw" if e % 3 == 1 else "leftout"
        return _MIX[(e + j) % 7]
    return choose


def chooser(name, index):
    kind, _, w, _, _, effort, _, count = struct.unpack_from("<8i", index, 12)
    P = parts(kind, w, effort)
    return choose_mix(P, count) if name == "mix" else choose_all(name, P)


# ---- reading the flags and widths back ---------------------------------------------------------------------------------------
def walk(packed):
    """[(body_flag, [(code, unit, flag, data_at, widths or None), ...]), ...] per entry, from the packed bytes; data_at: the
    part's data in bytes from the start."""
    kind, _, w, _, _, effort, _, count = struct.unpack_from("<8i", packed, 12)
    P = parts(kind, w, effort)
    out, at = [], 128
    for _ in range(count):
        n = struct.unpack_from("<Q", packed, at)[0]
        q = at + 8 + 168
        stop = at + 8 + n - 64
        body_flag = packed[q]
        q += 1
        row = []
        for pat, pn, unit, code, _ in P:
            if body_flag == 0:
                row.append((code, unit, 0, q + pat, None))
                continue
            flag = packed[q]
            q += 1
            widths = None
            if flag == 0:
                size = pn
            elif flag == 2:
                size = 0
            else:
                nb = -(-pn // unit // 64)
                widths = list(packed[q:q + nb])
                size = nb + 8 * sum(widths)
            row.append((code, unit, flag, q, widths))
            q += size
        assert q == stop if body_flag else q + P[-1][0] + P[-1][1] == stop
        out.append((body_flag, row))
        at += 8 + n
    assert at + 32 == len(packed)
    return out


def bodies_of(index):
    """The bodies of a hand-made index, by position."""
    count = struct.unpack_from("<i", index, 40)[0]
    out, at = [], 96
    for _ in range(count):
        n = struct.unpack_from("<Q", index, at)[0]
        out.append(index[at + 8 + 168:at + 8 + n - 32])
        at += 8 + n
    return out


# ---- tables, value first -----------------------------------------------------------------------------------------------------
def _unzigzag(v, bits):
    mask = np.uint64((1 << bits) - 1)
    return ((v >> np.uint64(1)) ^ (np.uint64(0) - (v & np.uint64(1)))) & mask


def graded_values(n, unit, e, rng, cap=None):
    """n values (whole blocks of 64): block k's largest has exactly min((k + e) mod (8 unit + 1), cap) bits, in lane 0 (e
    even) or 63 (e odd); the other lanes are random below 2^bits."""
    bits = 8 * unit
    nb = n // 64
    assert nb * 64 == n
    b = (np.arange(nb) + e) % (bits + 1)
    if cap is not None:
        b = np.minimum(b, cap)
    v = rng.integers(0, 2 ** 64, (nb, 64), dtype=np.uint64, endpoint=False)
    lim = np.where(b >= 64, np.uint64(2 ** 64 - 1), (np.uint64(1) << np.minimum(b, 63).astype(np.uint64)) - np.uint64(1))
    v &= lim[:, None]
    lane = 0 if e % 2 == 0 else 63
    top = np.where(b > 0, np.uint64(1) << (np.maximum(b, 1) - 1).astype(np.uint64), np.uint64(0))
    v[:, lane] |= top
    return v.reshape(-1), b


def _graded_doubles(n, e, rng):
    """B of entry e: doubles whose int64 form has the graded values (capped at 63 bits)."""
    v, b = graded_values(n, 8, e, rng, cap=63)
    v = v.reshape(-1, 64)
    lane = 0 if e % 2 == 0 else 63
    v[b >= 2, lane] &= np.uint64(2 ** 64 - 2)                                  # the top lane: an even value, a positive double
    x = _unzigzag(v.reshape(-1), 64).view(np.int64)
    out = np.empty(n, np.float64)
    for i, xi in enumerate(int(a) for a in x):                                 # keep the 53 leading bits of the magnitude
        m = abs(xi)
        drop = max(m.bit_length() - 53, 0)
        m = (m >> drop) << drop
        assert m < 2 ** 62
        out[i] = float(m if xi >= 0 else -m)
    out[out == 0] = 0.0                                                        # (never -0.0)
    return out


def graded_tables(kind, w, effort, count, rng):
    """One dict per entry (fresh_tables' keys): every coded part's values graded, the tables derived from them."""
    P = dict(zip(("ctx", "cnt", "hits", "rank", "sym") if kind == 0 else ("ctx", "rows", "tab"), parts(kind, w, effort)[1:]))
    out, prev = [], None
    for e in range(count):
        t = fresh_tables(kind, w, effort)
        t["rows"] = rng.integers(0, 256, 2 * w).astype(np.uint8)
        for name in (("ctx", "cnt", "hits", "sym") if kind == 0 else ("ctx", "tab")):
            _, n, unit, code, init = P[name]
            bits = 8 * unit
            v, _ = graded_values(n // unit, unit, e, rng)
            base = initial(init, n // unit) if prev is None else np.frombuffer(prev[name].tobytes(), _DT[unit]).astype(np.uint64)
            x = (base + _unzigzag(v, bits)) & np.uint64((1 << bits) - 1) if code == "diff" else base ^ v
            t[name] = np.frombuffer(x.astype(_DT[unit]).tobytes(), t[name].dtype).copy()
        if kind == 0:
            t["rank"] = rank_inverse(t["sym"])
            if t["B"].size:
                t["B"] = _graded_doubles(t["B"].size, e, rng)
        out.append(t)
        prev = t
    return out


def odd_symbols(tables, rng, inverse=True):
    """Symbol bytes with repeats and with values of 20 and more (0 .. 24, so most symbols are named more than once or not at
    all); the rank bytes their rank_inverse -- or, `inverse` False, in every other entry not: only raw carries those."""
    for e, t in enumerate(tables):
        t["sym"] = rng.integers(0, 25, 10240).astype(np.uint8)
        t["rank"] = rank_inverse(t["sym"])
        if not inverse and e % 2 == 1:
            at = rng.integers(0, 10240, 200)
            t["rank"][at] = (t["rank"][at] + 1 + rng.integers(0, 19, 200)) % 20
    return tables


def odd_b(tables):
    """NaN, -0.0, 0.5 and 2^62 in B of every other entry from entry 1 on: only raw carries them, a coded entry follows."""
    for e, t in enumerate(tables):
        if e % 2 == 1:
            n = t["B"].size
            t["B"][[3, n // 2 + 1, n - 1, 64]] = [np.nan, -0.0, 0.5, 2.0 ** 62]
    return tables


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _families(geo, mode):
    """(family, packings) of one geometry and mode.  "real" and "wide" are indexes the library accepts."""
    (h, w, every), (kind, effort) = geo, mode
    fam = [("graded", ("min", "mix")), ("real", ("rand", "mix"))]
    if w == 29:
        fam.append(("wide", ("full",)))
    elif w == 30:
        fam.append(("real", ("full",)))
    if kind == 0 and (h, w) == (37, 29):
        if effort == 1:
            fam += [("symbols", ("min", "mix")), ("badrank", ("min",))]
        else:
            fam.append(("oddb", ("min",)))
    return fam


def make_tables(family, kind, w, effort, count, rng):
    if family == "graded":
        return graded_tables(kind, w, effort, count, rng)
    if family == "wide":
        return touched(kind, w, effort, count, rng, wide=True)
    t = touched(kind, w, effort, count, rng)
    if family in ("symbols", "badrank"):
        return odd_symbols(t, rng, inverse=family == "symbols")
    return odd_b(t) if family == "oddb" else t


_cases = {}


def cases():
    """{(geometry, mode, family, packing): dict(index, packed, bodies, valid)}, made once per process."""
    if _cases:
        return _cases
    for gi, (geo, mode) in enumerate(GEOMETRIES):
        (h, w, every), (kind, effort) = geo, mode
        count = (h - 1) // every
        made = {}
        for fi, (family, packings) in enumerate(_families(geo, mode)):
            if family not in made:
                made[family] = index_of(kind, effort, h, w, every, make_tables(family, kind, w, effort, count, np.random.default_rng(1000 + 10 * gi + fi)))
            index = made[family]
            for pi, packing in enumerate(packings):
                rng = np.random.default_rng(5000 + 100 * gi + 10 * fi + pi)
                _cases[(geo, mode, family, packing)] = dict(index=index, packed=pack(index, chooser(packing, index), rng), bodies=bodies_of(index),
                                                            valid=family in ("real", "wide"))
    return _cases


def case_ids():
    """The keys of cases() without making them (for parametrize)."""
    return [(geo, mode, family, packing) for geo, mode in GEOMETRIES for family, packings in _families(geo, mode) for packing in packings]
