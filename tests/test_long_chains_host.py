"""CPU: why the context chains' unmet blocks can be resolved through 128-entry tables, and that the scheme the kernels
run (long_chain_inputs.s2_scheme) computes what the plain replay computes.

The two coupled copies obey gap' <= ceil(127 gap / 128) whatever the error: both take floor((127 v + c) / 128) of the
same c.  From 2 * extreme that recurrence is at 127 -- its fixed point -- well inside the kBiasWarm records of a warm-up,
so the state at a block's first record is one of at most 128 values, and a table over them is complete."""
import functools

import numpy as np
import pytest

import chain_inputs as ci
import long_chain_inputs as li


@functools.lru_cache(maxsize=None)
def schemes(model):
    return {name: li.s2_scheme(fam) for name, fam in li.s2_families(model).items()}


@pytest.mark.parametrize("model", [0, 1])
def test_gap_recurrence(model):
    m = ci.MODEL[model]
    assert li.gap_steps(2 * m["extreme"]) == li.GAP_STEPS[model] <= li.WARM
    assert -((-127 * 127) // 128) == 127 and -((-127 * 128) // 128) == 127        # 127 is where it stops; 128 still shrinks
    # one step of the two copies never beats the recurrence: every gap up to 300 at a few places, random large ones
    rng = np.random.default_rng(1)
    va = np.r_[np.repeat([-m["extreme"], -1, 0, 77], 301), rng.integers(-m["extreme"], m["extreme"], 20000)]
    gap = np.r_[np.tile(np.arange(301), 4), rng.integers(0, 2 * m["extreme"], 20000)]
    vb = np.minimum(va + gap, m["extreme"])
    for e in (-m["emax"], -1, 0, 1, 5, m["emax"]):
        a, b = ci.ctx_update(model, va, e), ci.ctx_update(model, vb, e)
        assert (b >= a).all() and (b - a <= -((-127 * (vb - va)) // 128)).all()


@pytest.mark.parametrize("model", [0, 1])
def test_gap_after_a_warm_up_on_adversarial_errors(model):
    """Every constant error at once (a lane each), the period-2 extremes in both phases, random errors of three
    amplitudes: after kBiasWarm records the copies are fewer than 128 apart, and ordered."""
    m = ci.MODEL[model]
    em = m["emax"]
    rng = np.random.default_rng(2)
    i = np.arange(li.WARM)
    seqs = [np.full(li.WARM, e) for e in range(-em, em + 1)]
    seqs += [np.where(i % 2 == 0, em, -em), np.where(i % 2 == 0, -em, em)]
    seqs += [rng.integers(-a, a + 1, li.WARM) for a in (1, 12, em) for _ in range(20)]
    e = np.stack(seqs, 1).astype(np.int64)                              # [step][sequence]
    va, vb = np.full(e.shape[1], -m["extreme"], np.int64), np.full(e.shape[1], m["extreme"], np.int64)
    for row in e:
        va, vb = ci.ctx_update(model, va, row), ci.ctx_update(model, vb, row)
    assert (vb >= va).all() and (vb - va < li.CANDS).all()
    assert (vb - va)[:2 * em + 1].max() == 127                          # a constant error really parks them 127 apart


@pytest.mark.parametrize("model", [0, 1])
def test_scheme_equals_the_replay(model):
    for name, s in schemes(model).items():
        r = s["replay"]
        for k in ("px", "sign", "end"):
            assert np.array_equal(s[k], r[k]), (name, k)
        assert s["serial"] == 0 and s["met"] == int(r["blk_ok"].sum()) and s["met"] + s["table"] == len(r["blocks"]), name
    # and with the tables off: the same arrays, every such block counted as replayed in order
    fam = li.s2_families(model)["const5"]
    off = li.s2_scheme(fam, tables=False)
    assert off["table"] == 0 and off["serial"] == schemes(model)["const5"]["table"]
    for k in ("px", "sign", "end"):
        assert np.array_equal(off[k], off["replay"][k]), k


@pytest.mark.parametrize("model", [0, 1])
def test_scheme_from_a_carried_table(model):
    """A row band's semantics: block 0 starts from the table the rows above left."""
    fam = li.s2_families(model)["const5"]
    c = 9000
    a = li.s2_scheme(ci.cut(fam, 0, c))
    b = li.s2_scheme(ci.cut(fam, c, None), a["end"])
    whole = schemes(model)["const5"]
    assert np.array_equal(np.r_[a["px"], b["px"]], whole["px"]) and np.array_equal(np.r_[a["sign"], b["sign"]], whole["sign"])
    assert np.array_equal(b["end"], whole["end"]) and a["table"] == 2 and b["table"] == 2


@pytest.mark.parametrize("model", [0, 1])
def test_candidate_intervals_nest(model):
    """The true state at a block's first record lies between its copies, and every candidate's end state lies between the
    NEXT block's copies: a look-up never leaves the next table, so the tables of a chain compose."""
    seen = 0
    for name, s in schemes(model).items():
        true_at = {(k, b): t for k, b, _, _, _, t in s["replay"]["blocks"]}
        copies = {(k, b): (va, vb) for k, b, _, va, vb, _ in s["replay"]["blocks"]}
        for k, b, va, vb, table in s["tables"]:
            assert va <= true_at[(k, b)] <= vb, (name, k, b)
            assert (np.diff(table) >= 0).all(), (name, k, b)            # monotone in the start state
            if (k, b + 1) in copies:
                lo, hi = copies[(k, b + 1)]
                assert lo <= table[0] and table[vb - va] <= hi, (name, k, b)
                seen += 1
    assert seen >= 8


@pytest.mark.parametrize("model", [0, 1])
def test_regimes(model):
    s = schemes(model)
    assert (s["const5"]["met"], s["const5"]["table"]) == (1, 5)         # six blocks, only the chain's first is exact
    last = {(k, b): met for k, b, met, *_ in s["last_one"]["replay"]["blocks"]}
    keys = ci.LENGTH_KEYS[model]
    assert last[(keys[1], 1)] is False and last[(keys[-1], 2)] is False         # the one-record blocks did not meet
    assert last[(keys[5], 1)] and last[(keys[5], 2)]                            # the noisy chain's did
    assert s["last_one"]["table"] == 3
    burst = [met for k, b, met, *_ in s["alternation"]["replay"]["blocks"] if k == keys[4]]
    assert burst == [True, False, True, False, False]                   # tables on both sides of a met block
    flip = [met for k, b, met, *_ in s["alternation"]["replay"]["blocks"] if k == keys[-2]]
    assert flip == [True] + [False] * 5                                 # period 2, extreme: never met, still < 128 apart
    assert s["lengths_const"]["table"] == sum((n - 1) // li.BLOCK for n in ci.LENGTHS)
    assert s["bounds"]["table"] == 0                                    # (saturated, then a swing to the other bound: the copies meet on the way)
    gaps = [vb - va for name in s for _, _, va, vb, _ in s[name]["tables"]]
    assert 0 < min(gaps) <= max(gaps) == 127


# ---- S3: re-mapper chains cut into blocks ------------------------------------------------------------------------------
S3_NAMES = ["uniform", "lengths", "overtake", "rotation", "stale_tie", "bypass", "wave"]


@functools.lru_cache(maxsize=None)
def s3_case(name):
    """(family, context table, px, sign, the plain replay)."""
    fam, v0 = li.s3_family(name)
    r = ci.ctx_replay(fam, v0)
    assert np.array_equal(r["px"], fam["px0"])                          # the records were steered: px = px0 and the key's sign
    return fam, v0, r["px"], r["sign"], ci.mapper_replay(fam["x"], r["px"], r["sign"])


def blocks_and_chains(replay):
    cut = [n for _, n, _ in replay["chains"].values() if n >= li.S3_MIN]
    return sum(-(-n // li.S3_BLOCK) for n in cut), len(cut)


@pytest.mark.parametrize("name", S3_NAMES)
def test_block_scheme_equals_the_replay(name):
    fam, _, px, sign, want = s3_case(name)
    blocks, chains = blocks_and_chains(want)
    assert chains >= 1
    for kw in (dict(guess=li.guess_wrong, warm=False), dict(warm=False), dict()):
        got = li.s3_scheme(fam["x"], px, sign, **kw)
        assert np.array_equal(got["z"], want["z"]) and np.array_equal(got["end"], want["end"]), (name, kw)
        assert got["split"] == chains and got["accepted"] + got["missed"] == blocks - chains, (name, kw)
        if kw.get("guess") is li.guess_wrong:
            assert got["accepted"] == 0                                 # every block behind a chain's first took the miss path
    off = li.s3_scheme(fam["x"], px, sign, min_records=-1)
    assert np.array_equal(off["z"], want["z"]) and np.array_equal(off["end"], want["end"]) and off["split"] == 0


def test_block_scheme_from_a_carried_table():
    fam, v0, px, sign, want = s3_case("wave")
    c = 5000
    a = li.s3_scheme(fam["x"][:c], px[:c], sign[:c])
    b = li.s3_scheme(fam["x"][c:], px[c:], sign[c:], a["end"])
    assert np.array_equal(np.r_[a["z"], b["z"]], want["z"]) and np.array_equal(b["end"], want["end"])
    assert a["split"] + b["split"] >= 2


def test_block_regimes():
    """Which path each family takes with the kernels' guess (counts, ties in the starting order, one block of warm-up)."""
    def run(name, **kw):
        fam, _, px, sign, _ = s3_case(name)
        return li.s3_scheme(fam["x"], px, sign, **kw)
    u = run("uniform")
    assert (u["split"], u["accepted"], u["missed"]) == (1, 19, 0)       # a flat chain stays the identity
    lengths = {n for _, n, _ in s3_case("lengths")[4]["chains"].values()}
    assert {1023, 1024, 1025, 1279, 1280, 1281} <= lengths and run("lengths")["split"] == 10      # 1023 is not cut
    # the overtake and rotation chains tie at block starts all the time, in the order the chain started with: no miss
    assert run("overtake")["missed"] == 0 and run("rotation")["missed"] == 0
    # a tie made by an overtake is the other way round, and stays: misses until the tie is broken (the second chain)
    st = run("stale_tie")
    assert (st["split"], st["accepted"], st["missed"]) == (2, 1 + 7, 10 + 4)
    assert run("wave", warm=False)["missed"] > run("wave")["missed"]    # random symbols: what a block of warm-up mends
    w = s3_case("wave")[4]["chains"]
    assert sorted(k for k, (_, n, _) in w.items() if n >= li.S3_MIN) == [32 * 5 + 3, 32 * 5 + 12] and len(w) == 16
    by = s3_case("bypass")
    assert (ci.x_to_y(by[0]["x"], by[2], by[3]) >= 20).sum() > 500
    assert {k & 1 for k in s3_case("bypass")[4]["chains"]} == {0, 1}    # chains of either sign
