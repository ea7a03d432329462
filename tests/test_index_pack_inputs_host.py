"""CPU suite: the inputs of test_index_unpack_kernels.py (index_pack_inputs.py) are what they claim to be.  The writer there
is free where the format is free -- widths above the minimum, parts and bodies raw, the rank bytes raw -- and with "min"
everywhere it is the independent writer of test_index_pack_host.py, and the library's; what it writes the library's host
reader takes back to the original bytes.  The coverage conditions at the end are computed from the packed bytes: they say
which paths of the unpack kernels the GPU tests reach, and are fixed here, where no kernel runs."""
import ctypes as C
import struct

import numpy as np
import pytest

import index_pack_inputs as ipi
from test_index_pack_host import MODES, index_of, ref_pack, touched

CASES = ipi.case_ids()
case_id = lambda c: "%dx%d-%d-k%de%d-%s-%s" % (c[0] + c[1] + c[2:])


def structural_size(pkg, packed):
    """nblic_amd_index_unpack(.., NULL, 0): the bare structural walk, the size of the index the packed one stands for."""
    x = np.frombuffer(packed, np.uint8)
    return int(pkg.load_library().nblic_amd_index_unpack(C.c_void_p(x.ctypes.data), x.size, None, 0))


@pytest.mark.parametrize("kind,effort", MODES)
@pytest.mark.parametrize("geo", [(37, 29, 5), (37, 30, 5), (13, 161, 1)])
def test_min_everywhere_is_the_reference_writer(pkg, geo, kind, effort):
    h, w, every = geo
    if h == 13 and (kind, effort) not in ((0, 1), (1, 0)):
        return
    count = (h - 1) // every
    for family in ("real", "wide", "graded", "symbols", "badrank", "oddb"):
        if kind == 1 and family in ("symbols", "badrank", "oddb") or family == "oddb" and effort == 1:
            continue
        ix = index_of(kind, effort, h, w, every, ipi.make_tables(family, kind, w, effort, count, np.random.default_rng(77)))
        mine = ipi.pack(ix, ipi.chooser("min", ix), np.random.default_rng(0))
        assert mine == ref_pack(ix), family
        if family in ("real", "wide"):
            assert pkg.check_index(ix) and mine == pkg.pack_index(ix), family
        else:
            assert not pkg.check_index(ix), family                             # (the library's writer is not asked: it refuses these)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_packing_unpacks_to_the_original(pkg, case):
    c = ipi.cases()[case]
    packed, ix = c["packed"], c["index"]
    assert structural_size(pkg, packed) == len(ix)
    assert pkg.unpack_index(packed) == ix
    if c["valid"]:                                                             # a library-valid index: every packing of it is a valid input today
        assert pkg.check_index(ix) and pkg.check_index(packed)
        assert pkg.index_entries(packed) == pkg.index_entries(ix)
    else:
        assert not pkg.check_index(ix)
    assert len(c["bodies"]) == struct.unpack_from("<i", ix, 40)[0]


def test_the_hook_is_exported_and_refuses_without_a_context(pkg):
    lib = pkg.load_library()
    assert "nblic_amd_debug_index_unpack" in pkg.EXPORTS
    assert lib.nblic_amd_debug_index_unpack(None, 1, None, None, None, None, None, None, None, None) == -1


def test_a_full_packing_may_be_larger_than_the_index(pkg):
    c = ipi.cases()[((37, 29, 5), (1, 0), "wide", "full")]
    assert len(c["packed"]) > len(c["index"]) and pkg.check_index(c["packed"])


def test_the_tables_are_what_they_are_called():
    rng = np.random.default_rng(5)
    sym = ipi.odd_symbols(touched(0, 29, 1, 2, rng), rng)[1]["sym"].reshape(512, 20)
    assert (sym >= 20).any(axis=1).sum() > 400                                  # bytes no symbol has
    assert sum(len(set(r[r < 20])) < (r < 20).sum() for r in sym) > 400         # symbols named more than once
    t = ipi.odd_b(touched(0, 29, 2, 2, rng))[1]["B"]
    assert np.isnan(t[3]) and np.signbit(t[t.size // 2 + 1]) and t[t.size // 2 + 1] == 0 and t[-1] == 0.5 and t[64] == 2.0 ** 62
    g = ipi.graded_tables(0, 29, 3, 7, rng)
    cnt = np.stack([t["cnt"].view("<u2") for t in g]).astype(np.int64)
    step = (np.diff(cnt, axis=0) % 65536)
    assert ((step > 0x7000) & (step < 0x9000)).any(), "no unit-2 difference near half the range: the 16-bit wrap is not reached"
    assert (cnt[:, 0::2] + cnt[:, 1::2] > 8192).any()                           # not counters a decoder has: the hook's acceptance is structural
    for t in g:
        assert np.isfinite(t["B"]).all() and (np.abs(t["B"]) < 2.0 ** 62).all() and (t["B"] == np.trunc(t["B"])).all()


# ---- the coverage conditions: what the GPU tests reach, computed from the packed bytes -----------------------------------
def _walks():
    return {k: ipi.walk(c["packed"]) for k, c in ipi.cases().items()}


def test_every_width_of_every_unit_occurs():
    seen = {2: set(), 4: set(), 8: set()}
    for entries in _walks().values():
        for _, row in entries:
            for code, unit, flag, _, widths in row:
                if flag == 1:
                    seen[unit] |= set(widths)
    for unit in (2, 4, 8):
        assert seen[unit] == set(range(8 * unit + 1)), (unit, sorted(set(range(8 * unit + 1)) - seen[unit]))


def test_graded_packings_carry_their_grades():
    """In the "min" packing of graded tables block k of entry e has the width (k + e) mod (8 unit + 1) -- 63 for B's 64."""
    for key, entries in _walks().items():
        if key[2:] != ("graded", "min"):
            continue
        for e, (body_flag, row) in enumerate(entries):
            assert body_flag == 1
            for code, unit, flag, _, widths in row:
                if code in ("diff", "xor", "int64"):
                    assert flag == 1
                    want = [(k + e) % (8 * unit + 1) for k in range(len(widths))]
                    assert widths == ([min(b, 63) for b in want] if code == "int64" else want), (key, e, code)


def test_wide_fields_at_non_zero_shifts():
    """Unit 8: a block of width 33 .. 63, odd, so that lanes start at every bit of a word and fields straddle three words."""
    odd = set()
    for entries in _walks().values():
        for _, row in entries:
            for code, unit, flag, _, widths in row:
                if flag == 1 and unit == 8:
                    odd |= {b for b in widths if 33 <= b < 64 and b % 2 == 1}
    assert odd == set(range(33, 64, 2))


def test_every_flag_on_every_part_kind():
    seen, bodies = set(), set()
    for entries in _walks().values():
        for body_flag, row in entries:
            bodies.add(body_flag)
            if body_flag == 1:
                seen |= {(code, flag) for code, _, flag, _, _ in row}
    assert bodies == {0, 1}
    assert seen == {("raw", 0), ("diff", 0), ("diff", 1), ("xor", 0), ("xor", 1), ("int64", 0), ("int64", 1), ("rank", 0), ("rank", 2)}


def test_raw_in_front_of_coded_and_a_raw_body_mid_chain():
    after_raw_part, after_raw_body, mid = set(), set(), 0
    for entries in _walks().values():
        for e in range(1, len(entries)):
            (pf, prow), (f, row) = entries[e - 1], entries[e]
            for (code, _, pflag, _, _), (_, _, flag, _, _) in zip(prow, row):
                if f == 1 and flag == 1 and pflag == 0:
                    (after_raw_part if pf == 1 else after_raw_body).add(code)
        mid += sum(1 for e in range(1, len(entries) - 1) if entries[e][0] == 0)
    assert after_raw_part == {"diff", "xor", "int64"} and after_raw_body == {"diff", "xor", "int64"}
    assert mid > 0


def test_part_data_at_every_address_residue():
    """With the base offsets the GPU tests use, the data of every kind of part lies at all four residues of a word."""
    seen = {}
    lengths = set()
    for key, entries in _walks().items():
        lengths.add(len(ipi.cases()[key]["packed"]) % 4)
        for _, row in entries:
            for code, _, flag, at, _ in row:
                if flag != 2:
                    for base in ipi.BASE_OFFSETS:
                        seen.setdefault((code, flag), set()).add((base + at) % 4)
    assert all(v == {0, 1, 2, 3} for v in seen.values()), seen
    assert len(seen) == 8 and len(lengths) > 1


def test_the_raw_row_slot_of_two_blocks_with_a_short_last_unit():
    for key, entries in _walks().items():
        w = key[0][1]
        code, unit, flag, _, _ = entries[0][1][-1 if key[1][0] == 0 else 2]
        assert (code, unit, flag) == ("raw", 4, 0)
        if w == 161:
            assert 2 * w > 64 * 4 and (2 * w) % 4 == 2                          # 81 units: a second block, its last unit two bytes
