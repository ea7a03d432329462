"""CPU suite: the record families of entropy_inputs.py reach the regimes they are made for -- computed with plain Python /
numpy and the oracle's general stages alone, before any GPU is involved -- and the references agree with each other:
the symbol formula and the Python walk with orc_s3_near / orc_s4_kstep, the replays with orc_s5."""
import numpy as np
import pytest

import chain_inputs as ci
import entropy_inputs as ei


def symbols(fam):
    return ei.x_to_y(fam["x"], fam["px"], fam["sign"], fam["near"])


def keys(fam):
    return fam["px"].astype(np.int64) * 2 + fam["sign"]


def test_pairs_and_table():
    assert len(ei.PAIRS) == 46 and len(set(ei.PAIRS)) == 46
    for near in ei.NEARS:
        k_step, top, most_bins, most_esc = ei.TABLE[near]
        assert k_step == ei.k_step_of(near) and top == ei.ymax(near), near
        walks = [ei.walk(k_step, qu, qv, z) for qu, qv in ei.PAIRS for z in range(top + 1)]
        assert max(len(ev) for ev, _ in walks) == most_bins and max(esc for _, esc in walks) == most_esc, near
    assert all(ei.ymax(near) < ei.MAP_SYMS for near in (7, 8, 9))            # near >= 7: no symbol bypasses the re-mapper
    y6 = ei.all_triples(6)[3]
    assert set(y6[y6 >= ei.MAP_SYMS]) == {20}                                # near 6: exactly one value does
    # the largest symbol at near 0: a pixel at the far end of the range from a prediction in the other half (x 0 under
    # px >= 128, x 255 under px <= 127; beyond the fold the symbol is distance + fold limit = 255), 512 of 131072 triples
    assert int((ei.all_triples(0)[3] == 255).sum()) == 512
    assert len(ei.walk(16, 0, 0, 255)[0]) == 256                             # why the entry takes no free k_step: cnt is a byte


@pytest.mark.parametrize("near", ei.NEARS)
def test_triples_reach_their_regimes(oracle, near):
    fam = ei.triples(near)
    n = len(fam["x"])
    assert n == 1 << 17
    idx = (fam["x"].astype(np.int64) << 9) | keys(fam)
    assert np.array_equal(np.sort(idx), np.arange(n))                        # every triple once
    assert np.array_equal(np.bincount(keys(fam), minlength=512), np.full(512, 256))
    y = symbols(fam)
    assert set(y.tolist()) == set(range(ei.TABLE[near][1] + 1))              # every symbol 0..ymax
    assert (np.bincount(keys(fam)[y < ei.MAP_SYMS], minlength=512) > 0).all()  # no chain is empty
    assert set(zip(fam["qu"].tolist(), fam["qv"].tolist())) == set(ei.PAIRS) and set(fam["qw"].tolist()) == set(range(17))
    k = keys(fam)
    assert (k[1:] != k[:-1]).mean() > 0.99                                   # neighbours in raster order have different keys
    yo, zo = oracle.s3_near(fam["x"], fam["px"], fam["sign"], near)          # the formula and the replay against the oracle
    mr = ci.mapper_replay(fam["x"], fam["px"], fam["sign"], None, y=y)
    assert np.array_equal(yo, y) and np.array_equal(zo, mr["z"])
    s4 = oracle.s4_kstep(ei.k_step_of(near), fam["qu"], fam["qv"], fam["qw"], zo)
    print(f"triples({near}): {len(s4['cu'])} events, most bins {int(s4['cnt'].max())}")
    assert len(s4["cu"]) < 3 << 20 and int(s4["cnt"].max()) <= 56


@pytest.mark.parametrize("near", ei.NEARS)
def test_walk_grid_reaches_every_cell(oracle, near):
    k_step, top, most_bins, most_esc = ei.TABLE[near]
    cells, esc_seen, bins_seen = set(), 0, 0
    calls = ei.walk_grid(near)
    for fam in calls:
        y = symbols(fam)
        inside = y < ei.MAP_SYMS
        assert np.bincount(keys(fam)[inside], minlength=512).max() <= 1      # a chained record is the first of its chain
        yo, z = oracle.s3_near(fam["x"], fam["px"], fam["sign"], near)
        assert np.array_equal(yo, y) and np.array_equal(z, y)                # so its rank is its symbol
        s4 = oracle.s4_kstep(k_step, fam["qu"], fam["qv"], fam["qw"], z)
        ev = ei.events_of(s4)
        at = 0
        for qu, qv, qw, zz, c in zip(fam["qu"].tolist(), fam["qv"].tolist(), fam["qw"].tolist(), z.tolist(), s4["cnt"].tolist()):
            want, esc = ei.walk(k_step, qu, qv, zz)                          # the Python walk against the oracle's, event by event
            assert c == len(want) <= 56
            assert all(0 <= u < 16 and 0 <= v < 16 and 0 <= node < 256 for u, v, node, _ in want)    # pack_event's fields
            assert ev[at:at + c].tolist() == [int(ci.pack_event(u, v, node, qw, b)) for u, v, node, b in want]
            at += c
            cells.add(((qu, qv), zz, qw))
            esc_seen, bins_seen = max(esc_seen, esc), max(bins_seen, c)
        assert at == len(ev)
    assert {(p, z) for p, z, _ in cells} == {(p, z) for p in ei.PAIRS for z in range(top + 1)}       # no cell is missing
    assert {w for _, _, w in cells} == {0, 1, 15, 16}
    assert (esc_seen, bins_seen) == (most_esc, most_bins)                    # near 0: 5 escalations, near 1: 2
    assert len(calls) == 2 and all(len(f["x"]) <= 6000 for f in calls)


def test_small_families_reach_their_regimes(oracle):
    for near in (1, 6, 9):
        fams = ei.sizes(near)
        assert [len(f["x"]) for f in fams] == list(ei.SIZES)
        y = np.concatenate([symbols(f) for f in fams])
        assert (y < ei.MAP_SYMS).any() and ((y >= ei.MAP_SYMS).any() or near == 9)
    for near in (0, 3, 6):
        fam = ei.bypass_all(near)
        assert (symbols(fam) >= ei.MAP_SYMS).all() and ei.expected(oracle, fam)["chained"] == 0
        assert np.array_equal(ei.expected(oracle, fam)["map_state"], ci.map_init())
    assert len(set(symbols(ei.bypass_all(0)).tolist())) > 200 and set(symbols(ei.bypass_all(6)).tolist()) == {20}
    fam = ei.bypass_none(0)
    assert (symbols(fam) < ei.MAP_SYMS).all() and set(symbols(fam).tolist()) == set(range(20))


def test_one_chain_families(oracle):
    for which, want in (("first", {0}), ("last", {511}), ("both", {0, 511})):
        fam = ei.one_chain(which)
        assert len(fam["x"]) == 70000 and fam["near"] == 2 and set(keys(fam).tolist()) == want
        y = symbols(fam)
        assert set(y.tolist()) == set(range(20))
        mr = ci.mapper_replay(fam["x"], fam["px"], fam["sign"], None, y=y)
        assert sum(swaps for _, _, swaps in mr["chains"].values()) > 20      # the ranks move
        assert np.array_equal(oracle.s3_near(fam["x"], fam["px"], fam["sign"], 2)[1], mr["z"])
    k = keys(ei.one_chain("both"))
    assert 30000 < (k == 0).sum() < 40000 and (k[1:] != k[:-1]).mean() > 0.4


@pytest.mark.parametrize("name", ["sizes", "walk_grid_1", "one_chain_both"])
def test_expectations_agree_with_the_oracle_and_carry(oracle, name):
    """expected() -- mapper_replay, the general S4, counter_replay -- against orc_s5, and cut in two with the tables
    carried against itself whole."""
    fams = {"sizes": ei.sizes(6)[-3:], "walk_grid_1": ei.walk_grid(1), "one_chain_both": [ei.one_chain("both")]}[name]
    for fam in fams:
        whole = ei.expected(oracle, fam)
        s4 = whole["s4"]
        assert np.array_equal(whole["coded"] & 0xFFF, oracle.s5(s4["cu"], s4["cv"], s4["qw"], s4["bin"])), fam["name"]
        assert np.array_equal(whole["coded"] >> 15, s4["bin"]) and whole["n_ev"] == int(whole["cnt"].sum())
        c = min(1300, len(fam["x"]) // 2)
        a = ei.expected(oracle, ei.cut(fam, 0, c))
        b = ei.expected(oracle, ei.cut(fam, c, None), a["map_state"], a["cnt_state"])
        for k in ("z", "cnt", "events", "coded"):
            assert np.array_equal(np.r_[a[k], b[k]], whole[k]), (fam["name"], k)
        assert np.array_equal(b["map_state"], whole["map_state"]) and np.array_equal(b["cnt_state"], whole["cnt_state"])
