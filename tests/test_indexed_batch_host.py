"""Host side of the indexed batch (nblic_amd_encode_batch_indexed): the size of an index (nblic_amd_index_bytes), which needs
no device, and what the Python wrapper refuses before it touches the library."""
import numpy as np
import pytest

# layout (include/nblic_amd.h): head 96 | count x (length 8 | checkpoint head 168 + body + seal 32) | seal 32
def expected(kind, h, w, effort, every):
    if kind == 0:
        body = 86080 + 2 * w + {1: 0, 2: 512 * w, 3: 1024 * w}[effort]
    else:
        body = 12352 + 2 * w + 24576
    return 96 + 32 + ((h - 1) // every) * (8 + 200 + body)


GEOMETRIES = [(0, 2, 1, 1, 1), (0, 40, 37, 1, 1), (0, 40, 37, 1, 39), (0, 40, 37, 1, 5), (0, 4096, 4096, 1, 64), (0, 23, 150, 2, 4),
              (0, 23, 150, 3, 22), (0, 65535, 1, 1, 65534), (1, 64, 96, 0, 16), (1, 9, 1, 0, 1), (1, 9, 1, 0, 8)]


@pytest.mark.parametrize("kind,h,w,effort,every", GEOMETRIES)
def test_index_bytes_is_the_documented_layout(pkg, kind, h, w, effort, every):
    assert pkg.index_bytes(kind, h, w, effort, every) == expected(kind, h, w, effort, every)


def test_index_bytes_refuses_what_has_no_index(pkg):
    for every in (0, -1, 40, 41):                                         # R < 1, R >= h
        assert pkg.index_bytes(0, 40, 37, 1, every) == -1
    assert pkg.index_bytes(0, 1, 37, 1, 1) == -1                          # one row: no entry row
    for kind, effort in ((0, 0), (0, 4), (1, 1), (2, 1), (-1, 1)):        # effort / kind out of range
        assert pkg.index_bytes(kind, 40, 37, effort, 5) == -1
    for h, w in ((0, 5), (5, 0), (65536, 5), (5, 65536)):
        assert pkg.index_bytes(0, h, w, 1, 1) == -1


class NoLibrary:
    """Stands where a Context would: any reach for the library fails the test."""
    @property
    def lib(self):
        raise AssertionError("the wrapper touched the library")
    handle = None


def test_wrapper_refuses_before_touching_the_library(pkg):
    imgs = [np.zeros((4, 5), np.uint8)] * 3
    with pytest.raises(ValueError):
        pkg.Context.encode_batch_indexed(NoLibrary(), imgs, -1)
    with pytest.raises(ValueError):
        pkg.Context.encode_batch_indexed(NoLibrary(), imgs, [2, -3, 2])
    with pytest.raises(ValueError):
        pkg.Context.encode_batch_indexed(NoLibrary(), imgs, [2, 2])
    with pytest.raises(ValueError):
        pkg.Context.encode_indexed_ptrs(NoLibrary(), [1, 2, 3], [(4, 5)] * 3, False, [1, 1, 1, 1])
