"""CPU suite: the band decoder's ABI is there, its checkpoint validation refuses damaged input on the host, and the
Python object refuses to exist without a device behind it.  No call here touches a GPU."""
import re

import pytest

DSTREAM = ("nblic_amd_dstream_begin", "nblic_amd_dstream_resume", "nblic_amd_dstream_check", "nblic_amd_dstream_feed",
           "nblic_amd_dstream_info", "nblic_amd_dstream_run", "nblic_amd_dstream_progress", "nblic_amd_dstream_checkpoint",
           "nblic_amd_dstream_end")


def test_symbols_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = open(pkg.INCLUDE).read()
    for name in DSTREAM:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "typedef struct nblic_amd_dstream nblic_amd_dstream;" in text


def test_host_check_refuses_junk(pkg):
    head = b"NBLDCKPT" + (1).to_bytes(4, "little")
    for b in (b"", b"x", bytes(100), bytes(4096), b"NBLCKPT1" + bytes(400), head + bytes(600), (head + bytes(600))[:-1],
              b"NBLDCKPX" + (1).to_bytes(4, "little") + bytes(600), b"NBLDCKPT" + (2).to_bytes(4, "little") + bytes(600)):
        assert not pkg.check_decoder_checkpoint(b), b[:16]


class _Closed:
    handle = None

    def __init__(self, lib):
        self.lib = lib


def test_decoder_without_a_device_raises(pkg):
    with pytest.raises(RuntimeError):
        pkg.BandDecoder(_Closed(pkg.load_library()))
