"""The coder threads' pack feed without a GPU (nblic_amd_range_code_packs): one to three packs of 8-lane rows of 13-bit
groups, a chunk at a time, in lock-step.  Every lane is compared byte for byte with nblic_amd_range_code of its own
records."""
import numpy as np
import pytest

from coder_inputs import records as _records, runs

CHUNK = 4096
LENGTHS = (1, 51, 52, 53, 63, 64, 65, 4095, 4096, 4097)


def _deal(streams, n_packs):
    """Consecutive streams to n_packs packs, unevenly where they do not divide: 17 go 6 / 6 / 5."""
    out, at = [], 0
    for p in range(n_packs):
        cnt = len(streams) // n_packs + (1 if p < len(streams) % n_packs else 0)
        out.append(streams[at:at + cnt])
        at += cnt
    return out


@pytest.fixture(scope="module")
def feed(pkg):
    if pkg.range_code_multi([np.array([1], np.uint16)])[1] != 1:
        pytest.skip("no AVX-512 on this host: the coder threads code every image on its own and feed_packs never runs")

    def run(packs, chunk=CHUNK, caps=None):
        got, used_simd = pkg.range_code_packs(packs, chunk, caps)
        assert used_simd                                       # the pack feed itself, not the scalar stand-in
        want = [[pkg.range_code(s) for s in p] for p in packs]
        return got, want
    return run


@pytest.mark.parametrize("n_packs", (1, 2, 3))
def test_every_lane_count_and_length(feed, n_packs):
    """1..8 lanes per pack, the lengths around a group (51..65) and around a chunk (4095..4097), rotated through the lanes."""
    rng = np.random.default_rng(100 + n_packs)
    for lanes in range(1, 9):
        packs = [[_records(rng, LENGTHS[(3 * p + lanes + k) % len(LENGTHS)]) for k in range(lanes)] for p in range(n_packs)]
        got, want = feed(packs)
        assert got == want, (n_packs, lanes)


def test_uneven_deal_of_seventeen(feed):
    rng = np.random.default_rng(7)
    streams = [_records(rng, LENGTHS[k % len(LENGTHS)] + 37 * k) for k in range(17)]
    packs = _deal(streams, 3)
    assert [len(p) for p in packs] == [6, 6, 5]
    got, want = feed(packs)
    assert got == want
    for n_packs, count in ((2, 9), (2, 15), (3, 23), (1, 7)):
        got, want = feed(_deal(streams[:count] if count <= 17 else streams + streams[:count - 17], n_packs))
        assert got == want, (n_packs, count)


def test_lanes_end_in_different_groups_and_chunks(feed):
    """Lanes of one pack that end in another group and another chunk each: 0.3 .. 3.2 chunks, and whole packs that have ended
    while another pack goes on."""
    rng = np.random.default_rng(9)
    packs = [[_records(rng, n) for n in (1300, 4096 + 65, 2 * 4096 + 1, 3 * 4096 + 700, 52, 4096 - 64, 2 * 4096, 9000)],
             [_records(rng, n) for n in (64, 200, 4097)],
             [_records(rng, n) for n in (13000, 12999, 1, 8191, 8192)]]
    got, want = feed(packs)
    assert got == want
    got, want = feed(packs, chunk=64)
    assert got == want
    got, want = feed(packs, chunk=1 << 16)                 # everything in one chunk
    assert got == want


def test_long_runs_of_extreme_probabilities(feed):
    """Probabilities 1 and 4095 in long runs: several bytes leave the coder per step."""
    packs = [[np.full(5000, 1 | (1 << 15), np.uint16), np.full(4097, 4095, np.uint16), runs(1, 9000), runs(2, 4096), np.full(6000, 1, np.uint16)],
             [runs(3, 12000), np.full(3000, 4095 | (1 << 15), np.uint16), runs(4, 65)]]
    got, want = feed(packs)
    assert got == want
    assert max(len(b) for p in want for b in p) > 3000      # the runs do produce bytes


def test_one_lane_one_byte_short(feed):
    rng = np.random.default_rng(21)
    packs = _deal([_records(rng, 3000 + 411 * k) for k in range(13)], 2)
    _, want = feed(packs)
    caps = [[len(b) for b in p] for p in want]
    got, _ = feed(packs, caps=caps)
    assert got == want                                     # an exact fit passes
    caps[1][2] -= 1
    got, _ = feed(packs, caps=caps)
    assert got[1][2] is None
    for p in range(2):
        for k in range(len(packs[p])):
            if (p, k) != (1, 2):
                assert got[p][k] == want[p][k], (p, k)


def test_layout_reference_is_what_the_feed_reads(pkg):
    """pack_groups_host with eight lanes: word j of group g of lane l sits at (13 g + j) * 8 + l; codes 4j .. 4j + 3 in the low
    52 bits, the probability of code 52 + j (the bins of codes 52 .. 63 in word 12) on top."""
    rng = np.random.default_rng(3)
    lanes = [_records(rng, n) for n in (130, 64, 1)]
    rows = pkg.pack_groups_host(lanes).reshape(-1, 13, 8)
    assert rows.shape[0] == 3 and not rows[:, :, 3:].any()
    for l, rec in enumerate(lanes):
        for i, r in enumerate(rec):
            code = (int(r) & 0xFFF) | ((int(r) >> 15) << 12)
            g, k = divmod(i, 64)
            if k < 52:
                assert (int(rows[g, k // 4, l]) >> (13 * (k % 4))) & 0x1FFF == code
            else:
                assert int(rows[g, k - 52, l]) >> 52 == code & 0xFFF
                assert (int(rows[g, 12, l]) >> (52 + k - 52)) & 1 == code >> 12
