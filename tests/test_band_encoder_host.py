"""CPU suite: the band encoder's checkpoint validation (nblic_amd_stream_check) accepts a well-formed checkpoint and
refuses damaged ones on the host.  The checkpoints here are put together by hand, byte by byte, so no call touches a
GPU."""
import hashlib
import re
import struct

import pytest

H, W = 5, 3                            # -n0 -e1 at width 3: no B, and the model kernel keeps the rows in LDS (none written down)


def _sha_state(total):
    """A running SHA-256 (sha256.h Sha256) that has absorbed `total` bytes."""
    return bytes(32) + struct.pack("<Q", total) + bytes(64)


def _state(next_row, status=0):
    return struct.pack("<iiQIIIiQi20x", next_row, status, 0, 0, 0, 0, 7, 0, 0)


def _body(next_row, near, effort, w, status=0, perm=None, counter=(32, 32), b_value=0.0):
    """model state record | B | map_state | cnt_state | rows above (near > 0) -- the layout of pipeline.hip."""
    model = _state(next_row, status) + bytes(2048 * 4)                            # header + context biases
    b = struct.pack("<d", b_value) * (2 * w * {2: 64, 3: 128}.get(effort, 0) // 2)
    perm = list(range(20)) if perm is None else perm
    inverse = [perm.index(k) for k in range(20)]
    mapper = struct.pack("<60i", *(perm + inverse + [0] * 20))                    # symbol -> rank, rank -> symbol, hit counts
    counters = struct.pack("<2i", *counter) * 4096
    rows = bytes(range(1, 2 * w + 1)) if near > 0 else b""
    return model + b + mapper * 512 + counters + rows, len(b), len(rows)


def checkpoint(next_row=2, near=0, effort=1, w=W, h=H, band_rows=2, version=1, magic=b"NBLECKPT", record_row=None,
               status=0, perm=None, counter=(32, 32), b_value=0.0, bytes_total=100, sha_total=None, lo=0, hi=0xFFFFFFFF):
    body, b_bytes, rows_bytes = _body(next_row if record_row is None else record_row, near, effort, w, status, perm, counter, b_value)
    head = magic + struct.pack("<I6i3I", version, h, w, near, effort, band_rows, next_row, lo, hi, 0)
    head += struct.pack("<Q", bytes_total) + _sha_state(bytes_total if sha_total is None else sha_total)
    head += struct.pack("<3Q", b_bytes, rows_bytes, len(body))
    assert len(head) == 184
    ck = head + body
    return ck + hashlib.sha256(ck).digest()


def _reseal(b):
    return b[:-32] + hashlib.sha256(b[:-32]).digest()


def _flip(b, at):
    b = bytearray(b)
    b[at] ^= 0x10
    return bytes(b)


def test_symbol_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = open(pkg.INCLUDE).read()
    assert hasattr(lib, "nblic_amd_stream_check") and "nblic_amd_stream_check" in pkg.EXPORTS
    assert re.search(r"\bnblic_amd_stream_check\s*\(", text)


@pytest.mark.parametrize("near,effort", [(0, 1), (0, 3), (2, 2)])
def test_well_formed_checkpoint_is_accepted(pkg, near, effort):
    assert pkg.check_encoder_checkpoint(checkpoint(near=near, effort=effort))
    assert pkg.check_encoder_checkpoint(checkpoint(next_row=1, band_rows=H, near=near, effort=effort))


def test_refuses_junk_truncation_and_damage(pkg):
    good = checkpoint(near=2, effort=2)
    version_bumped = bytearray(good)
    version_bumped[8] += 1
    old = b"NBLCKPT1" + struct.pack("<6i2IQ", H, W, 0, 1, 2, 2, 0, 0xFFFFFFFF, 100) + _sha_state(100) + struct.pack("<2Q", 0, 0)
    old += _body(2, 0, 1, W)[0]
    bad = {"empty": b"", "junk": bytes(len(good)), "short junk": b"x" * 100, "truncated": good[:-1], "cut in the head": good[:100],
           "head": _flip(good, 20), "body": _flip(good, len(good) // 2), "trailer": _flip(good, len(good) - 1),
           "version": _reseal(bytes(version_bumped)), "NBLCKPT1": old, "decoder magic": checkpoint(magic=b"NBLDCKPT"),
           "extended": _reseal(good[:-32] + b"\0" + good[-32:])}
    for name, b in bad.items():
        assert not pkg.check_encoder_checkpoint(b), name


def test_refuses_inconsistent_fields(pkg):
    """Each checkpoint is sealed correctly: only the field check can refuse it."""
    bad = {"next_row mismatch": checkpoint(record_row=3), "status": checkpoint(status=1),
           "next_row 0": checkpoint(next_row=0, record_row=0), "next_row h": checkpoint(next_row=H, record_row=H),
           "band_rows 0": checkpoint(band_rows=0), "band_rows > h": checkpoint(band_rows=H + 1),
           "bytes_total 0": checkpoint(bytes_total=0, sha_total=0), "sha total": checkpoint(sha_total=99),
           "near": checkpoint(near=200), "effort": checkpoint(effort=4), "geometry": checkpoint(h=0),
           "interval": checkpoint(lo=5, hi=5),
           "counter zero": checkpoint(counter=(0, 32)), "counter over the limit": checkpoint(counter=(8192, 1)),
           "B not finite": checkpoint(effort=2, b_value=float("nan")), "B infinite": checkpoint(effort=3, b_value=float("inf"))}
    for name, b in bad.items():
        assert not pkg.check_encoder_checkpoint(b), name


def test_refuses_a_broken_remapper(pkg):
    perm = list(range(20))
    perm[3], perm[4] = perm[4], perm[3]
    assert pkg.check_encoder_checkpoint(checkpoint(perm=perm))                # any permutation with its inverse is taken
    broken = bytearray(checkpoint())
    at = 184 + 64 + 2048 * 4 + 7 * 240                                       # re-mapper 7 (no B at effort 1)
    broken[at + 80:at + 84] = struct.pack("<i", 1)                            # rank -> symbol names symbol 1 twice
    assert not pkg.check_encoder_checkpoint(_reseal(bytes(broken)))
    broken = bytearray(checkpoint())
    broken[at:at + 4] = struct.pack("<i", 20)                                 # symbol -> rank out of range
    assert not pkg.check_encoder_checkpoint(_reseal(bytes(broken)))


def test_recorded_sizes_must_match_the_mode(pkg):
    good = bytearray(checkpoint(near=2, effort=2))
    for at in (160, 168):                                                     # stats_bytes, recon_bytes
        b = bytearray(good)
        b[at] ^= 8
        assert not pkg.check_encoder_checkpoint(_reseal(bytes(b)))
