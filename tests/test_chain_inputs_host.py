"""CPU suite: the record families of chain_inputs.py reach the regimes they are made for -- computed with the oracle's
array stages and the plain replays alone, before any GPU is involved -- and the references agree with each other:
the replays with orc_s2 / orc_s3 / orc_q_s2 / orc_s5, the two-copy simulation with the true bias wherever the copies met."""
import functools

import numpy as np
import pytest

import chain_inputs as ci


@functools.lru_cache(maxsize=None)
def families(model):
    return ci.model_families(model)


@functools.lru_cache(maxsize=None)
def replayed(model, name):
    return ci.ctx_replay(families(model)[name])


def later(blocks, key=None):
    return [b[2] for b in blocks if b[1] > 0 and (key is None or b[0] == key)]


@pytest.mark.parametrize("model", [0, 1])
def test_context_chain_families_reach_their_regimes(model):
    m = ci.MODEL[model]
    fams = families(model)
    assert all(len(f["adr"]) <= 70000 for f in fams.values())
    for name in ("lengths_noise", "lengths_const"):
        got = np.bincount(fams[name]["adr"], minlength=m["keys"])
        assert [int(got[k]) for k in ci.LENGTH_KEYS[model]] == ci.LENGTHS and got.sum() == sum(ci.LENGTHS)
    met = later(replayed(model, "lengths_noise")["blocks"])
    assert len(met) == 7 and all(met)                                    # every block behind a chain's first meets on noise
    assert not any(later(replayed(model, "lengths_const")["blocks"]))    # and none on a constant error
    keys = ci.LENGTH_KEYS[model]
    blocks = replayed(model, "alternation")["blocks"]
    assert later(blocks, keys[1]) == [True] * 5                          # noise somewhere in every warm-up
    assert later(blocks, keys[4]) == [False, True, False, False]         # a met block between two that did not meet
    assert later(blocks, keys[-2]) == [False] * 5                        # period 2, extreme: never
    end = replayed(model, "bounds")["end"]
    fixed = m["err_mul"] * m["emax"]                                     # the fixed point of a sustained extreme error
    assert end[keys[2]] <= -0.99 * fixed and end[keys[-1]] >= 0.99 * fixed and fixed <= m["extreme"]
    assert np.array_equal(np.bincount(fams["keys_all"]["adr"], minlength=m["keys"]), np.ones(m["keys"], np.int64))
    assert set(fams["key_first"]["adr"]) == {0} and set(fams["key_last"]["adr"]) == {m["keys"] - 1}
    if model == 1:
        assert fams["keys_high"]["adr"].min() == 2048 and len(set(fams["keys_high"]["adr"])) == 1024      # all 12 match bits
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        assert len(fams[f"edge_{n}"]["adr"]) == n
    for name, fam in fams.items():                                       # neighbours in raster order have different keys
        adr = fam["adr"].astype(np.int64)
        if len(set(adr)) > 2 and len(adr) >= 64:
            assert (adr[1:] != adr[:-1]).mean() > 0.4, name


@pytest.mark.parametrize("model", [0, 1])
def test_replays_agree_with_the_oracle(oracle, model):
    for name, fam in families(model).items():
        r = replayed(model, name)
        if model == 0:
            want = ci.orc_model(oracle, fam)
            assert np.array_equal(r["px"], want["px"]) and np.array_equal(r["sign"], want["sign"]), name
            mr = ci.mapper_replay(fam["x"], r["px"], r["sign"])
            assert np.array_equal(mr["y"], want["y"]) and np.array_equal(mr["z"], want["z"]), name
        else:
            y, end = ci.orc_q_s2(oracle, fam["adr"], fam["px0"], fam["x"])
            assert np.array_equal(y, ci.x_to_y(fam["x"], r["px"], r["sign"])) and np.array_equal(end, r["end"]), name
        for key, blk, met, lo, hi, true in r["blocks"]:                  # copies that met hold the chain's true bias
            assert lo <= true <= hi and (not met or lo == true == hi), (name, key, blk)
        assert len(r["blk_ok"]) == int(r["blk_base"][-1])
    # a chain continued from a table is the chain
    fam = families(model)["lengths_noise"]
    whole, c = replayed(model, "lengths_noise"), 23456
    a = ci.ctx_replay(ci.cut(fam, 0, c))
    b = ci.ctx_replay(ci.cut(fam, c, None), a["end"])
    assert np.array_equal(np.r_[a["px"], b["px"]], whole["px"]) and np.array_equal(b["end"], whole["end"])


def test_remapper_family_reaches_its_regimes():
    fam = families(0)["remapper"]
    r = replayed(0, "remapper")
    assert np.array_equal(r["px"], fam["px0"]) and not r["sign"].any()   # the key is 2 px0
    mr = ci.mapper_replay(fam["x"], r["px"], r["sign"])
    chains = mr["chains"]
    assert {s & 3 for s, _, _ in chains.values()} == {0, 1, 2, 3}        # run_lane_streams' 4-record words
    for g, base in enumerate((60, 100, 140)):
        got = [chains[2 * (base + j)] for j in range(8)]
        assert [n for _, n, _ in got] == ci.REMAP_LENGTHS
        if g == 0:
            assert all(swaps >= (n - 4) // 2 for _, n, swaps in got)     # an overtake at every second step
    y = mr["y"]
    px = fam["px0"].astype(np.int64)
    assert set(y[(px >= 100) & (px < 108)]) == set(range(20))            # all twenty in rotation
    assert (y[px >= 140] >= 20).sum() > 100 and (y[px < 140] < 20).all() # bypass symbols, in the third group only


# ---- back half --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def back():
    return ci.back_families()


def test_counter_families_reach_their_regimes():
    fams = back()
    assert all(len(ev) <= 70000 for ev in fams.values())
    counts, starts = ci.chain_layout(fams["alignment"])
    _, targets = ci.align_lengths()
    assert len(targets) == 64 and all(counts[k] == n and starts[k] & 7 == p for k, p, n in targets)
    assert {(p, n + p) for _, p, n in targets} >= {(p, e) for p in range(8) for e in (8, 9, 511, 512, 513, 1024)}
    per_window, lanes, slots = ci.halving_slots(fams["alignment"])
    assert max(per_window.values()) == 4 and min(per_window.values()) == 0 and slots == set(range(8))   # (the carried-state cuts need halvings)
    even, odd, cnt = ci.busy_chains(fams["staging"], ci.SEG)
    assert list(even[:5]) == [63, 64, 64, 40, 6] and odd[2] == 64 and not odd[[0, 1, 3, 4]].any()
    assert {15, 16, 17} <= set(cnt[3]) and (cnt[3] == 16).sum() == 20
    ku, _ = ci.touches_of(fams["staging"])
    fills = (ku[4 * ci.SEG:5 * ci.SEG].reshape(16, 64) == 1234).sum(1)
    assert any(fills[r - 1] <= 32 < fills[r] and fills[r + 1] <= 32 for r in range(1, 15)) and 64 in fills and 32 in fills and 33 in fills
    assert np.array_equal(np.sort(ku[5 * ci.SEG:]), np.arange(4096))      # every counter once
    qu, qv, node, qw, bin_ = ci.event_fields(fams["shapes"])
    shapes = set(zip((qu & 1).tolist(), (qv - qu).tolist(), np.minimum(qw, 17).tolist(), bin_.tolist()))
    assert shapes >= {(par, d, w, b) for par in (0, 1) for d in (-1, 0, 1) for w in (0, 1, 16) for b in (0, 1)}
    assert {0, 15} <= set(qu) and {0, 15} <= set(qv)
    for n in (1, 63, 64, 65, 1024, 1025, 2049):
        assert len(fams[f"size_{n}"]) == n


def test_wide_staging_family_reaches_its_regimes():
    ev = ci.staging_wide_family()
    assert len(ev) == 256 * ci.WIDE_SEG and (max(-(-len(ev) // 256), 1024) + 63) & ~63 == ci.WIDE_SEG      # make_plan's segment length
    even, odd, cnt = ci.busy_chains(ev, ci.WIDE_SEG)
    assert list(even[:3]) == [65, 200, 80] and not odd[:3].any() and max(even[3:].max(), odd[3:].max()) == 0
    assert (cnt[1] >= 17).sum() == 60 and (cnt[2] >= 17).sum() == 80 and (cnt[2] >= 18).sum() == 50   # thresholds 17 and, the tie cut, 18


def test_counter_replay_agrees_with_the_oracle(oracle):
    for name, ev in back().items():
        r = ci.counter_replay(ev)
        assert np.array_equal(r["prob"], ci.orc_s5(oracle, ev)), name
    ev = back()["alignment"]
    whole = ci.counter_replay(ev)
    a = ci.counter_replay(ev[:20001])
    b = ci.counter_replay(ev[20001:], a["end"])
    assert np.array_equal(np.r_[a["prob"], b["prob"]], whole["prob"]) and np.array_equal(b["end"], whole["end"])
