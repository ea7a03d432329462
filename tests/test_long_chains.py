"""GPU suite (-m gpu): chains that hold most of an image.  The context chains' blocks whose warm-up copies do not meet are
resolved through candidate tables (kernels_e1.hip k_bias_tabulate / k_bias_fixup / k_bias_replay) instead of one lane's
replay in order: every array the launch sequences return is compared for equality with the oracle's array stages and the
plain replays (test_chain_kernels.check_model), the block counts with the CPU restatement of the scheme
(long_chain_inputs.s2_scheme, proved equal to the replay in test_long_chains_host.py), and on every input no block is
replayed serially.  The re-mapper chains of at least min_records records are cut into blocks replayed from a guessed
permutation and checked in order (k_map_plan .. k_map_check): the arrays against the plain replays, the counts of accepted
and missed blocks against the CPU restatement (long_chain_inputs.s3_scheme), with families that take the miss path block
after block.  Then the public paths on images of one flat context, against the oracle's streams.  Every test fails on a
library without nblic_amd_set_long_chains / nblic_amd_long_chain_stats."""
import functools

import numpy as np
import pytest

import chain_inputs as ci
import inputs
import long_chain_inputs as li
from test_chain_kernels import check_model, model_stages

pytestmark = pytest.mark.gpu

S2_NAMES = ["const5", "lengths_const", "alternation", "bounds", "last_one"]


@functools.lru_cache(maxsize=None)
def s2_families(model):
    return li.s2_families(model)


@functools.lru_cache(maxsize=None)
def scheme(model, name):
    return li.s2_scheme(s2_families(model)[name])


@pytest.fixture(scope="module")
def live(gpu_ctx, pkg):
    """What the library held once both groups of the shared context own a whole workspace is what it holds at the end."""
    for _ in range(4):
        gpu_ctx.debug_stage(ci.noise(1, 17 * 13, 100).astype(np.uint8).reshape(17, 13), "coded")
    before = pkg.live_resources()
    yield before
    assert pkg.live_resources() == before


@pytest.fixture
def stats(gpu_ctx):
    """The shared context with the default setting and cleared counts; the default again afterwards."""
    gpu_ctx.set_long_chains(0, 0)
    gpu_ctx.long_chain_stats(reset=True)
    yield gpu_ctx
    gpu_ctx.set_long_chains(0, 0)


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("name", S2_NAMES)
def test_unmet_blocks_through_tables(stats, oracle, live, model, name):
    want = scheme(model, name)
    check_model(stats, oracle, s2_families(model)[name])
    got = stats.long_chain_stats()
    assert got["s2_serial"] == 0
    assert (got["s2_met"], got["s2_table"]) == (want["met"], want["table"]), name
    if name == "const5":
        assert got["s2_table"] == 5


@pytest.mark.parametrize("model", [0, 1])
def test_carried_state(stats, live, model):
    """Two calls, the second from the table the first left: block 0 starts exact, the blocks behind it through tables."""
    fam = s2_families(model)["const5"]
    whole = model_stages(stats, fam)
    for c in (9000, int(np.searchsorted(np.cumsum(fam["adr"] == ci.LENGTH_KEYS[model][3]), ci.BLOCK)) + 1):
        stats.long_chain_stats(reset=True)
        a = model_stages(stats, ci.cut(fam, 0, c))
        b = model_stages(stats, ci.cut(fam, c, None), a["ctx_state"], a.get("map_state"))
        for k in ("pxs", "z", "cnt"):
            if k in whole:
                assert np.array_equal(np.r_[a[k], b[k]], whole[k]), (c, k)
        for k in ("ctx_state", "map_state"):
            if k in whole:
                assert np.array_equal(b[k], whole[k]), (c, k)
        got = stats.long_chain_stats()
        assert got["s2_serial"] == 0 and got["s2_table"] == 4, (c, got)


@pytest.mark.parametrize("model", [0, 1])
def test_switched_off_gives_the_same_arrays(stats, live, model):
    """min_records < 0: the blocks are replayed in order by one lane per chain -- and counted as such."""
    for name in ("const5", "alternation"):
        fam = s2_families(model)[name]
        on = model_stages(stats, fam)
        stats.set_long_chains(-1, 0)
        stats.long_chain_stats(reset=True)
        off = model_stages(stats, fam)
        got = stats.long_chain_stats(reset=True)
        stats.set_long_chains(0, 0)
        assert got["s2_table"] == 0 and got["s2_serial"] == scheme(model, name)["table"] and got["s2_met"] == scheme(model, name)["met"]
        assert on.keys() == off.keys()
        for k in on:
            assert np.array_equal(on[k], off[k]), (name, k)


# ---- S3: re-mapper chains cut into blocks ------------------------------------------------------------------------------
S3_NAMES = ["uniform", "lengths", "overtake", "rotation", "stale_tie", "bypass", "wave"]


@functools.lru_cache(maxsize=None)
def s3_case(name):
    """(family, context table to start from, the context replay, the re-mapper replay, the CPU scheme's counts)."""
    fam, v0 = li.s3_family(name)
    r = ci.ctx_replay(fam, v0)
    return fam, v0, r, ci.mapper_replay(fam["x"], r["px"], r["sign"]), li.s3_scheme(fam["x"], r["px"], r["sign"])


@pytest.fixture
def cut(stats):
    stats.set_long_chains(li.S3_MIN, li.S3_BLOCK)
    return stats


def check_s3(got, r, want):
    assert np.array_equal(got["pxs"], r["px"].astype(np.uint16) | (r["sign"].astype(np.uint16) << 8)), "S2"
    assert np.array_equal(got["ctx_state"], r["end"]), "biases"
    assert np.array_equal(got["z"], want["z"]), "S3"
    assert np.array_equal(got["map_state"], want["end"]), "re-mapper tables"


@pytest.mark.parametrize("name", S3_NAMES)
def test_cut_remapper_chains(cut, live, name):
    fam, v0, r, want, sch = s3_case(name)
    got = model_stages(cut, fam, v0)
    check_s3(got, r, want)
    st = cut.long_chain_stats(reset=True)
    assert st["s2_serial"] == 0
    assert (st["s3_split"], st["s3_accepted"], st["s3_missed"]) == (sch["split"], sch["accepted"], sch["missed"]), st
    blocks = sum(-(-n // li.S3_BLOCK) for _, n, _ in want["chains"].values() if n >= li.S3_MIN)
    assert st["s3_accepted"] + st["s3_missed"] == blocks - st["s3_split"]
    if name == "stale_tie":
        assert st["s3_missed"] == 14                                      # the miss path, block after block
    cut.set_long_chains(-1, 0)                                            # off: identical arrays, nothing cut
    off = model_stages(cut, fam, v0)
    st = cut.long_chain_stats()
    assert (st["s3_split"], st["s3_accepted"], st["s3_missed"]) == (0, 0, 0)
    assert got.keys() == off.keys()
    for k in got:
        assert np.array_equal(got[k], off[k]), (name, k)


def test_cut_chains_from_carried_tables(cut, live):
    fam, v0, r, want, _ = s3_case("wave")
    for c in (5000, 8191):
        a = model_stages(cut, ci.cut(fam, 0, c), v0)
        b = model_stages(cut, ci.cut(fam, c, None), a["ctx_state"], a["map_state"])
        assert np.array_equal(np.r_[a["pxs"], b["pxs"]], r["px"].astype(np.uint16) | (r["sign"].astype(np.uint16) << 8)), c
        assert np.array_equal(np.r_[a["z"], b["z"]], want["z"]), c
        assert np.array_equal(b["map_state"], want["end"]) and np.array_equal(b["ctx_state"], r["end"]), c
    st = cut.long_chain_stats()
    assert st["s3_split"] >= 4 and st["s2_serial"] == 0


# ---- the public paths --------------------------------------------------------------------------------------------------
CONTENTS = ["const", "half-flat", "dark-noise"]
_refs = {}


def reference(oracle, content):
    """(image, the oracle's -n0 -e1 stream, its effort-0 stream): once per content."""
    if content not in _refs:
        img = inputs.syn1(128, 128, int(content[3:])) if content.startswith("syn") else li.image(content, 128, 128)
        img.setflags(write=False)
        _refs[content] = (img, oracle.encode(img, 0, 1)[0], oracle.qencode(img))
    return _refs[content]


@pytest.fixture
def own_ctx(pkg):
    before = pkg.live_resources()
    ctx = pkg.Context(device=0, n_slots=8, n_coders=2, n_groups=1)
    yield ctx
    ctx.close()
    assert pkg.live_resources() == before


def test_encode_batch_flat_frame_among_textured_ones(own_ctx, oracle):
    """One const frame and seven SYN-1 frames in one group of eight: every launch is shared."""
    refs = [reference(oracle, "const")] + [reference(oracle, f"syn{k}") for k in range(1, 8)]
    got = own_ctx.encode_batch([r[0] for r in refs])
    assert got == [r[1] for r in refs]
    st = own_ctx.long_chain_stats()
    assert st["s2_serial"] == 0 and st["s2_table"] >= 2                  # the flat frame: its interior is one chain of several blocks


@pytest.mark.parametrize("content", CONTENTS)
def test_encode_batch(own_ctx, oracle, content):
    img, want, _ = reference(oracle, content)
    assert own_ctx.encode_batch([img]) == [want]
    st = own_ctx.long_chain_stats()
    assert st["s2_serial"] == 0 and st["s2_table"] >= {"const": 2, "half-flat": 1, "dark-noise": 0}[content]


@pytest.mark.parametrize("content", CONTENTS)
def test_qencode_batch(own_ctx, oracle, content):
    img, _, want = reference(oracle, content)
    assert own_ctx.qencode_batch([img]) == [want]
    st = own_ctx.long_chain_stats()
    assert st["s2_serial"] == 0 and st["s2_met"] > 0 and st["s2_table"] >= {"const": 2, "half-flat": 1, "dark-noise": 0}[content]


def test_encode_batch_indexed(pkg, own_ctx, gpu_ctx, oracle):
    refs = [reference(oracle, c) for c in CONTENTS]
    got = own_ctx.encode_batch_indexed([r[0] for r in refs], 32)
    for (s, ix), (img, want, _) in zip(got, refs):
        assert s == want
        assert ix == gpu_ctx.build_index(s, 32)
    assert own_ctx.long_chain_stats()["s2_serial"] == 0


@pytest.mark.parametrize("content", CONTENTS)
def test_staged_band_stream_with_a_resume(pkg, own_ctx, oracle, content):
    """Bands of 16 rows on the staged front, suspended after four bands and resumed in a second object."""
    img, want, _ = reference(oracle, content)
    own_ctx.set_long_chains(512, 128)
    enc = own_ctx.stream(img, 0, 1, band_rows=16, front="staged")
    try:
        parts, done = [], False
        for _ in range(4):
            done, b = enc.run(1e-9)
            parts.append(b)
        assert not done
        ck = enc.checkpoint()
    finally:
        enc.close()
    enc = own_ctx.stream(img, 0, 1, band_rows=16, checkpoint=ck, front="staged")
    try:
        while not done:
            done, b = enc.run()
            parts.append(b)
    finally:
        enc.close()
    assert b"".join(parts) == want
    st = own_ctx.long_chain_stats()
    assert st["s2_serial"] == 0
    if content == "const":
        assert st["s3_split"] >= 8 and st["s3_accepted"] + st["s3_missed"] >= 8 * 8        # every band's flat chain (~1900 records) in blocks of 128


def test_a_band_with_several_blocks(own_ctx, oracle):
    """64 rows of 128 per band: a flat band is one chain of two blocks from a carried table, its second through a table."""
    img, want, _ = reference(oracle, "const")
    enc = own_ctx.stream(img, 0, 1, band_rows=64, front="staged")
    try:
        parts, done = [], False
        while not done:
            done, b = enc.run()
            parts.append(b)
    finally:
        enc.close()
    assert b"".join(parts) == want
    st = own_ctx.long_chain_stats()
    assert st["s2_serial"] == 0 and st["s2_table"] >= 1
