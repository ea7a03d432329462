"""GPU suite (-m gpu): the staged pipeline's kernels behind S1 on their own, on records no image produces.
Context.debug_model_stages / debug_back_half launch the production sequences once on the families of chain_inputs.py
(test_chain_inputs_host.py proves on the CPU which regime each reaches); every output is compared for equality with the
oracle's array stages (orc_s2 / orc_s3 / orc_s4 / orc_q_s2 / orc_s5) and with the plain replays: the tables after the
last record, and blk_ok -- which blocks' warm-up copies met -- against the two-copy simulation."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

EDGES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
COMMON = ["lengths_noise", "lengths_const", "alternation", "bounds", "keys_all", "key_first", "key_last", "edges"]
MODEL_CASES = [(0, n) for n in COMMON + ["remapper"]] + [(1, n) for n in COMMON + ["keys_high"]]
BACK_CASES = ["alignment", "staging", "shapes", "sizes"]


@functools.lru_cache(maxsize=None)
def families(model):
    return ci.model_families(model)


@functools.lru_cache(maxsize=None)
def back():
    return ci.back_families()


@pytest.fixture(scope="module")
def live(gpu_ctx, pkg):
    """What the library held before this module's first call -- once both groups of the shared context own a whole
    workspace, which grows in place from then on -- must be what it holds after the last."""
    for _ in range(4):
        gpu_ctx.debug_stage(ci.noise(1, 17 * 13, 100).astype(np.uint8).reshape(17, 13), "coded")
    before = pkg.live_resources()
    yield before
    assert pkg.live_resources() == before


def model_stages(ctx, fam, ctx_state=None, map_state=None):
    return ctx.debug_model_stages(fam["model"], fam["x"], ci.rec1_of(fam), ctx_state, map_state)


def check_model(ctx, oracle, fam):
    """One launch sequence on a family from an image's first tables, against the oracle and the replays."""
    got = model_stages(ctx, fam)
    r = ci.ctx_replay(fam)
    name = fam["name"]
    if fam["model"] == 0:
        want = ci.orc_model(oracle, fam)
        assert np.array_equal(got["pxs"], want["px"].astype(np.uint16) | (want["sign"].astype(np.uint16) << 8)), (name, "S2")
        assert np.array_equal(got["z"], want["z"]), (name, "S3")
        assert np.array_equal(got["cnt"], want["cnt"]), (name, "S4 counts")
        assert np.array_equal(got["map_state"], ci.mapper_replay(fam["x"], want["px"], want["sign"])["end"]), (name, "re-mapper tables")
    else:
        y, end = ci.orc_q_s2(oracle, fam["adr"], fam["px0"], fam["x"])
        qd = (fam["adr"] >> 8).astype(np.uint16)
        assert np.array_equal(got["pxs"], qd | (y.astype(np.uint16) << 8)), (name, "symbols")
        assert np.array_equal(got["qhist"], np.bincount(qd.astype(np.int64) * 256 + y, minlength=12 * 256)), (name, "histograms")
        assert np.array_equal(got["ctx_state"], end), (name, "biases (orc_q_s2)")
    assert np.array_equal(got["blk_base"], r["blk_base"]), (name, "blk_base")
    assert np.array_equal(got["blk_ok"], r["blk_ok"]), (name, "blk_ok", got["blk_ok"].tolist(), r["blk_ok"].tolist())
    assert np.array_equal(got["ctx_state"], r["end"]), (name, "biases")
    return got


@pytest.mark.parametrize("model,name", MODEL_CASES)
def test_model_stages(gpu_ctx, oracle, live, model, name):
    fams = families(model)
    for fam in ([fams[f"edge_{n}"] for n in EDGES] if name == "edges" else [fams[name]]):
        check_model(gpu_ctx, oracle, fam)


def cuts_of(fam):
    """Three raster indices to cut a family at: early, where its longest chain has exactly one block behind it (a block
    edge), and inside that chain's second block."""
    adr = fam["adr"].astype(np.int64)
    seen = np.cumsum(adr == np.bincount(adr).argmax())
    return [1000, int(np.searchsorted(seen, ci.BLOCK)) + 1, int(np.searchsorted(seen, 5000)) + 1]


@pytest.mark.parametrize("model,name", [(0, "lengths_noise"), (1, "lengths_noise"), (0, "lengths_const"), (0, "remapper")])
def test_model_stages_carried_state(gpu_ctx, live, model, name):
    """Two calls, the second from the tables the first left (a row band's semantics), equal one call."""
    fam = families(model)[name]
    whole = model_stages(gpu_ctx, fam)
    for c in cuts_of(fam) if name != "remapper" else [7, 1300, 2600]:
        a = model_stages(gpu_ctx, ci.cut(fam, 0, c))
        b = model_stages(gpu_ctx, ci.cut(fam, c, None), a["ctx_state"], a.get("map_state"))
        for k in ("pxs", "z", "cnt"):
            if k in whole:
                assert np.array_equal(np.r_[a[k], b[k]], whole[k]), (name, c, k)
        for k in ("ctx_state", "map_state"):
            if k in whole:
                assert np.array_equal(b[k], whole[k]), (name, c, k)
        if model == 1:
            assert np.array_equal(a["qhist"] + b["qhist"], whole["qhist"]), (name, c)


def check_back(ctx, oracle, ev, name, wide=0):
    got = ctx.debug_back_half(ev)
    r = ci.counter_replay(ev)
    counts, _ = ci.chain_layout(ev)
    assert np.array_equal(got["coded"] & 0xFFF, ci.orc_s5(oracle, ev)), (name, "S5")
    assert np.array_equal(got["coded"] >> 12, ci.event_fields(ev)[4] << 3), (name, "bins")
    assert got["totals"][3] == counts.sum() and got["totals"][4] == wide, (name, "totals")
    assert np.array_equal(got["cnt_state"], r["end"]), (name, "counters")
    return got


@pytest.mark.parametrize("name", BACK_CASES)
def test_back_half(gpu_ctx, oracle, live, name):
    fams = back()
    for key in ([f"size_{n}" for n in (1, 63, 64, 65, 1024, 1025, 2049)] if name == "sizes" else [name]):
        check_back(gpu_ctx, oracle, fams[key], key)


def test_back_half_wide_segments(gpu_ctx, oracle, live):
    """Segments with 65 and 200 busy chains need segments of more than 1024 events: a job of 851968."""
    check_back(gpu_ctx, oracle, ci.staging_wide_family(), "staging_wide")


def test_back_half_carried_state(gpu_ctx, live):
    """Cut inside a window, directly before a halving touch and directly behind it: two calls equal one."""
    ev = back()["alignment"]
    whole = gpu_ctx.debug_back_half(ev)
    ku, _ = ci.touches_of(ev)
    key, idx = ci.counter_replay(ev)["halvings"][40]
    at = int(np.flatnonzero(ku == key)[idx])                             # the event whose touch halves that counter
    for c in (at, at + 1, 20001):
        a = gpu_ctx.debug_back_half(ev[:c])
        b = gpu_ctx.debug_back_half(ev[c:], a["cnt_state"])
        assert np.array_equal(np.r_[a["coded"], b["coded"]], whole["coded"]), c
        assert np.array_equal(b["cnt_state"], whole["cnt_state"]), c


def test_back_half_with_plain_32_bit_positions(gpu_ctx, live):
    """The same families under the library's debug switch for plain 32-bit touch positions (k_mix re-reads the events), in
    a process of its own: the switch is read once."""
    code = (
        "import importlib, sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch; torch.cuda.init()\n"
        "import chain_inputs as ci, test_chain_kernels as t\n"
        "from oracle.oracle import Oracle\n"
        "pkg = importlib.import_module('nblic-image-compression_amd')\n"
        "ctx = pkg.Context(0, n_slots=2, n_coders=1)\n"
        "fams = ci.back_families()\n"
        "for name in ('shapes', 'staging', 'size_65'):\n"
        "    t.check_back(ctx, Oracle(), fams[name], name, wide=1)\n"
        "ctx.close()\n"
        "print('wide ok')\n"
    ) % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NBLIC_AMD_DBG="256"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wide ok" in r.stdout, r.stdout + r.stderr


def test_refusals_launch_nothing(gpu_ctx, pkg, oracle, live):
    fam = families(0)["edge_65"]
    qfam = families(1)["edge_65"]
    ev = back()["size_65"]
    before = (gpu_ctx.serial_launches(), pkg.live_resources())

    def refused(call, *args):
        with pytest.raises(ValueError):
            call(*args)
        assert (gpu_ctx.serial_launches(), pkg.live_resources()) == before

    rec = ci.rec1_of(fam)
    for bad in ((int(rec[0]) & ~(31 << 19)) | (17 << 19),               # qw 17
                int(rec[0]) | (3 << 25),                        # no such relation of qv to qu
                int(ci.pack_s1(np.array([7]), np.array([0]), np.array([0]), np.array([-1]), np.array([3]))[0]),      # qv -1
                int(ci.pack_s1(np.array([7]), np.array([0x700]), np.array([15]), np.array([16]), np.array([3]))[0]), # qv 16
                int(rec[0]) | (1 << 27)):
        r = rec.copy()
        r[33] = bad
        refused(gpu_ctx.debug_model_stages, 0, fam["x"], r)
    refused(gpu_ctx.debug_model_stages, 0, fam["x"], None)
    refused(gpu_ctx.debug_model_stages, 0, fam["x"], rec, np.full(2048, 32577, np.int32))
    bad_map = ci.map_init()
    bad_map[60 * 5 + 3] = 4                                               # not a permutation
    refused(gpu_ctx.debug_model_stages, 0, fam["x"], rec, None, bad_map)
    qrec = ci.rec1_of(qfam)
    qrec[7] = 100 | (3072 << 8)
    refused(gpu_ctx.debug_model_stages, 1, qfam["x"], qrec)
    refused(gpu_ctx.debug_model_stages, 1, qfam["x"], ci.rec1_of(qfam), None, ci.map_init())      # QNBLIC has no re-mapper
    refused(gpu_ctx.debug_model_stages, 2, qfam["x"], ci.rec1_of(qfam))
    for bad in (ci.pack_event(4, 6, 0, 3, 1), ci.pack_event(5, 5, 9, 17, 0), int(ev[0]) | (1 << 22)):
        e = ev.copy()
        e[64] = bad
        refused(gpu_ctx.debug_back_half, e)
    refused(gpu_ctx.debug_back_half, np.zeros(0, np.uint32))
    refused(gpu_ctx.debug_back_half, ev, np.zeros(8192, np.int32))       # no counter is ever 0
    refused(gpu_ctx.debug_back_half, ev, np.full(8192, 4097, np.int32))  # nor above the limit
    lib = pkg.load_library()
    assert lib.nblic_amd_debug_model_stages(None, 0, 1, *([None] * 10), 0, None, None) == -1
    assert lib.nblic_amd_debug_back_half(None, 1, None, None, None, None, None) == -1
    check_back(gpu_ctx, oracle, ev, "size_65")                           # and the context still works
