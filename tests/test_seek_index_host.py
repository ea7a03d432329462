"""CPU suite: the seek index's ABI is there, and its host-side validation (nblic_amd_index_check) accepts a well-formed
index and refuses damaged ones.  The index here is put together by hand, byte by byte, so no call touches a GPU."""
import hashlib
import re
import struct

import numpy as np
import pytest

INDEX = ("nblic_amd_index_check", "nblic_amd_index_build", "nblic_amd_decode_indexed", "nblic_amd_decode_rows",
         "nblic_amd_stream_set_index", "nblic_amd_stream_index", "nblic_amd_set_index_round")

H, W, R = 5, 3, 2                      # entries in front of rows 2 and 4
STREAM = b"NBLIC0.3" + bytes([1, 0, H, 0, W, 0, 3, 1]) + bytes(range(200)) * 5      # -n0 -e1, k_step 3


def _entry(next_row):
    """A band-decoder checkpoint of a -n0 -e1 H x W stream in front of `next_row` (the layout of pipeline.hip)."""
    state = struct.pack("<iiQIIIiQi20x", next_row, 0, 100, 0, 0xFFFFFFFF, 0, 0, 0, 0)
    tables = bytes(2048 * 4)                                                  # context biases
    tables += struct.pack("<I", 4 | (4 << 16)) * 4096                         # counters: c0 = c1 = 4
    tables += bytes(512 * 20 * 4)                                             # hit counts
    perm = bytes(range(20)) * 512
    tables += perm + perm                                                     # symbol -> rank and its inverse
    body = state + tables + bytes(2 * W)                                      # + the two rows above (effort 1: no B)
    sha_state = bytes(32) + struct.pack("<Q", next_row * W) + bytes(64)       # running hash of rows [0, next_row)
    head = b"NBLDCKPT" + struct.pack("<I8iIQQ", 1, 0, H, W, 0, 3, 1, R, next_row, 0, 0, len(body)) + sha_state
    ck = head + body
    return ck + hashlib.sha256(ck).digest()


def _index(entries=None, version=1, stream=STREAM):
    entries = [_entry(R), _entry(2 * R)] if entries is None else entries
    head = b"NBLSIDX1" + struct.pack("<I8i3IQ", version, 0, H, W, 0, 3, 1, R, len(entries), 0, 0, 0, len(stream)) + hashlib.sha256(stream).digest()
    assert len(head) == 96
    body = head + b"".join(struct.pack("<Q", len(e)) + e for e in entries)
    return body + hashlib.sha256(body).digest()


def _reseal(b):
    """The outer checksum made right again after a change inside."""
    return b[:-32] + hashlib.sha256(b[:-32]).digest()


def test_symbols_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = open(pkg.INCLUDE).read()
    for name in INDEX:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b" + name + r"\s*\(", text), name


def test_well_formed_index_is_accepted(pkg):
    ix = _index()
    assert pkg.check_index(ix)
    assert pkg.check_index(ix, STREAM)
    ents = pkg.index_entries(ix)
    assert ents == [_entry(R), _entry(2 * R)]
    assert all(pkg.check_decoder_checkpoint(e) for e in ents)


def test_refuses_junk(pkg):
    good = _index()
    bad = [b"", b"x", bytes(96 + 32), bytes(4096), good[:-1], good[:100],
           b"NBLSIDX2" + good[8:],                                            # magic
           _index(version=2),                                                 # format version
           good[:-32] + bytes(32)]                                            # outer checksum
    flip = bytearray(good)
    flip[50] ^= 1                                                             # a head field, the outer checksum left as it was
    bad.append(bytes(flip))
    for b in bad:
        assert not pkg.check_index(b), b[:16]


def test_refuses_damaged_or_misplaced_entries(pkg):
    e1, e2 = _entry(R), _entry(2 * R)
    inner = bytearray(e2)
    inner[-1] ^= 1                                                             # the entry's own checksum
    payload = bytearray(e2)
    payload[300] ^= 1                                                          # a byte inside the entry
    for entries in ([e1, bytes(inner)], [e1, bytes(payload)], [e2, e1], [e1, e1], [e1]):
        assert not pkg.check_index(_index(entries)), "entry damage not caught"
    with pytest.raises(ValueError):
        pkg.index_entries(_index([e1, bytes(inner)]))


def test_refuses_the_wrong_stream(pkg):
    ix = _index()
    other = STREAM[:-1] + bytes([STREAM[-1] ^ 1])                              # same length and header, one byte off
    assert not pkg.check_index(ix, other)
    assert not pkg.check_index(ix, STREAM + b"\0")
    wide = bytearray(STREAM)
    wide[12] = W + 1                                                           # another geometry
    assert not pkg.check_index(_reseal(_index(stream=bytes(wide))), STREAM)


def test_refuses_spacing_outside_the_image(pkg):
    ix = bytearray(_index())
    for r in (0, H):
        b = bytearray(ix)
        b[36:40] = struct.pack("<i", r)
        assert not pkg.check_index(_reseal(bytes(b)))


def test_build_size_query_needs_no_device(pkg):
    """nblic_amd_index_build with out == NULL parses the header alone: the size, or -1 for a spacing outside [1, h)."""
    lib = pkg.load_library()
    buf = np.frombuffer(STREAM, np.uint8).copy()
    p = buf.ctypes.data
    assert lib.nblic_amd_index_build(None, p, buf.size, R, None, 0) == len(_index())
    assert lib.nblic_amd_index_build(None, p, buf.size, 1, None, 0) == 96 + 4 * (8 + 168 + 86080 + 2 * W + 32) + 32
    for r in (0, -1, H, H + 7):
        assert lib.nblic_amd_index_build(None, p, buf.size, r, None, 0) == -1
    assert lib.nblic_amd_index_build(None, p, 15, R, None, 0) == -1          # not even a header
