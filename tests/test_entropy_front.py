"""GPU suite (-m gpu): the general instantiations of the entropy front -- k_map_count_pre, k_map_scatter<true>,
k_count_bins<true>, k_emit_bins<true>, which every mode but -n0 -e1 runs behind k_serial_model -- on their own, on records
no image produces.  Context.debug_entropy_front launches a serial-mode band's sequence once on the families of
entropy_inputs.py (test_entropy_inputs_host.py proves on the CPU which regime each reaches); every output is compared for
equality with the oracle's general stages (orc_s3_near / orc_s4_kstep / orc_s5) and the plain replays."""
import numpy as np
import pytest

import chain_inputs as ci
import entropy_inputs as ei
import inputs

pytestmark = pytest.mark.gpu

_want = {}


def want_of(oracle, fam):
    """The expectation of a family from an image's first tables: computed once."""
    if fam["name"] not in _want:
        _want[fam["name"]] = ei.expected(oracle, fam)
    return _want[fam["name"]]


@pytest.fixture(scope="module")
def live(gpu_ctx, pkg):
    """What the library held before this module's first call -- once both groups of the shared context own a whole
    workspace, which grows in place from then on -- must be what it holds after the last."""
    for _ in range(4):
        gpu_ctx.debug_stage(ci.noise(1, 17 * 13, 100).astype(np.uint8).reshape(17, 13), "coded")
    before = pkg.live_resources()
    yield before
    assert pkg.live_resources() == before


def front(ctx, fam, map_state=None, cnt_state=None):
    return ctx.debug_entropy_front(fam["x"], ei.rec1_of(fam), ei.pxs_of(fam), fam["near"], map_state, cnt_state)


def check_pos3(got, fam, y, name):
    """A bypassing symbol is carried in the word itself; every other record's word is its place in the partition by
    re-mapper key -- a permutation of 0 .. total - 1 that keeps raster order within a key: THE stable partition."""
    pos3 = got["pos3"]
    out = y >= ei.MAP_SYMS
    assert np.array_equal(pos3[out], (0x80000000 | y[out]).astype(np.uint32)), (name, "pos3 of bypassing symbols")
    inside = np.flatnonzero(~out)
    key = fam["px"].astype(np.int64)[inside] * 2 + fam["sign"][inside]
    order = inside[np.argsort(key, kind="stable")]
    assert np.array_equal(pos3[order], np.arange(len(inside), dtype=np.uint32)), (name, "pos3: stable partition by key")
    assert got["totals"][1] == len(inside), (name, "partition total")


def check(ctx, oracle, fam):
    """One launch sequence on a family from an image's first tables, against the oracle and the replays."""
    name, near = fam["name"], fam["near"]
    got = front(ctx, fam)
    want = want_of(oracle, fam)
    yo, zo = oracle.s3_near(fam["x"], fam["px"], fam["sign"], near)
    assert np.array_equal(yo, want["y"]), (name, "references: y")
    assert np.array_equal(got["z"], zo) and np.array_equal(got["z"], want["z"]), (name, "S3")
    assert np.array_equal(got["cnt"], want["cnt"]), (name, "S4 counts")
    check_pos3(got, fam, want["y"], name)
    assert np.array_equal(got["ev_off"], want["ev_off"]), (name, "ev_off")
    assert got["n_ev"] == want["n_ev"] and got["totals"][2] == want["n_ev"], (name, "event total")
    assert np.array_equal(got["events"], want["events"]), (name, "S4 events")
    s4 = want["s4"]
    assert np.array_equal(got["coded"] & 0xFFF, oracle.s5(s4["cu"], s4["cv"], s4["qw"], s4["bin"])), (name, "S5")
    assert np.array_equal(got["coded"], want["coded"]), (name, "coded")
    assert np.array_equal(got["map_state"], want["map_state"]), (name, "re-mapper tables")
    assert np.array_equal(got["cnt_state"], want["cnt_state"]), (name, "counters")
    assert got["totals"][3] == ci.chain_layout(want["events"])[0].sum() and got["totals"][4] == 0, (name, "touch total")
    return got


@pytest.mark.parametrize("near", ei.NEARS)
def test_triples(gpu_ctx, oracle, live, near):
    check(gpu_ctx, oracle, ei.triples(near))


@pytest.mark.parametrize("near", ei.NEARS)
def test_walk_grid(gpu_ctx, oracle, live, near):
    for fam in ei.walk_grid(near):
        check(gpu_ctx, oracle, fam)


@pytest.mark.parametrize("near", [1, 6, 9])
def test_sizes(gpu_ctx, oracle, live, near):
    for fam in ei.sizes(near):
        check(gpu_ctx, oracle, fam)


@pytest.mark.parametrize("which,near", [("all", 0), ("all", 3), ("all", 6), ("none", 0)])
def test_bypass(gpu_ctx, oracle, live, which, near):
    got = check(gpu_ctx, oracle, ei.bypass_all(near) if which == "all" else ei.bypass_none(near))
    if which == "all":
        assert got["totals"][1] == 0 and np.array_equal(got["map_state"], ci.map_init())
        assert (got["pos3"] >> 31).all() and np.array_equal(got["pos3"] & 0xFF, got["z"])
    else:
        assert got["totals"][1] == len(got["z"]) and not (got["pos3"] >> 31).any()


@pytest.mark.parametrize("which", ["first", "last", "both"])
def test_one_chain(gpu_ctx, oracle, live, which):
    check(gpu_ctx, oracle, ei.one_chain(which))


def test_near_0_equals_the_lossless_path(gpu_ctx, oracle, live):
    """triples(0)'s pixels and records through the staged model stages (k_map_count, k_map_scatter<false>,
    k_count_bins<false>), then the same pixels and records with px | sign as those stages left them through the general
    kernels at near 0: the same z and cnt, and the events the lossless walk (orc_s4, k_step 3) emits for them."""
    fam = ei.triples(0)
    rec1 = ei.rec1_of(fam)
    lossless = gpu_ctx.debug_model_stages(0, fam["x"], rec1)
    got = gpu_ctx.debug_entropy_front(fam["x"], rec1, lossless["pxs"], 0)
    assert np.array_equal(got["z"], lossless["z"]) and np.array_equal(got["cnt"], lossless["cnt"])
    assert np.array_equal(got["map_state"], lossless["map_state"])
    px, sign = lossless["pxs"] & 0xFF, lossless["pxs"] >> 8
    assert len(set((px.astype(np.int64) * 2 + sign).tolist())) > 400                # (the biases spread the predictions)
    st = oracle.lib
    _, z = oracle.s3_near(fam["x"], px, sign, 0)
    assert np.array_equal(z, got["z"])
    n = len(z)
    import ctypes as C
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    p16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    st.orc_s4.restype = C.c_size_t
    qu, qv, qw = fam["qu"], fam["qv"], fam["qw"]
    ne = st.orc_s4(C.c_size_t(n), p8(qu), p8(qv), p8(qw), p8(z), None, None, None, None, None)
    cu, cv, eq, eb = np.empty(ne, np.uint16), np.empty(ne, np.uint16), np.empty(ne, np.uint8), np.empty(ne, np.uint8)
    st.orc_s4(C.c_size_t(n), p8(qu), p8(qv), p8(qw), p8(z), p16(cu), p16(cv), p8(eq), p8(eb), None)
    assert np.array_equal(got["events"], ei.events_of(dict(cu=cu, cv=cv, qw=eq, bin=eb)))


@pytest.mark.parametrize("k", range(4))
def test_carried_state(gpu_ctx, live, k):
    """Two calls, the second from the tables the first left (a later band's semantics), equal one call."""
    fam = ei.carried_families()[k]
    whole = front(gpu_ctx, fam)
    for c in ei.CARRY_CUTS:
        a = front(gpu_ctx, ei.cut(fam, 0, c))
        b = front(gpu_ctx, ei.cut(fam, c, None), a["map_state"], a["cnt_state"])
        for key in ("z", "cnt", "events", "coded"):
            assert np.array_equal(np.r_[a[key], b[key]], whole[key]), (fam["name"], c, key)
        for key in ("map_state", "cnt_state"):
            assert np.array_equal(b[key], whole[key]), (fam["name"], c, key)


def test_one_table_handed_in(gpu_ctx, oracle, live):
    """A single table goes in behind k_init_state: the other one is an image's first."""
    fam = ei.sizes(6)[-1]
    c = 1300
    a = front(gpu_ctx, ei.cut(fam, 0, c))
    tail = ei.cut(fam, c, None)
    for ms, cs in ((a["map_state"], None), (None, a["cnt_state"])):
        got = front(gpu_ctx, tail, ms, cs)
        want = ei.expected(oracle, tail, ms, cs)
        for key in ("z", "cnt", "events", "coded", "map_state", "cnt_state"):
            assert np.array_equal(got[key], want[key]), (key, ms is None)


def test_event_capacity_is_respected(gpu_ctx, pkg, live):
    """-3: the front half has run, the total is reported, nothing is written to buffers too small for it."""
    fam = ei.sizes(1)[3]
    x, rec, pxs = fam["x"], ei.rec1_of(fam), ei.pxs_of(fam)
    n = len(x)
    whole = front(gpu_ctx, fam)
    before = pkg.live_resources()
    out = [np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(8, 0xEEEEEEEE, np.uint32)]
    tail = [np.full(8, 0xEEEE, np.uint16), np.zeros(512 * 60, np.int32), np.zeros(8192, np.int32), np.zeros(8, np.uint32)]
    ptr = lambda a: a.ctypes.data
    rc = pkg.load_library().nblic_amd_debug_entropy_front(gpu_ctx.handle, n, ptr(x), ptr(rec), ptr(pxs), 1, None, None,
                                                          *[ptr(a) for a in out], 8, *[ptr(a) for a in tail])
    assert rc == -3 and tail[3][2] == whole["n_ev"] > 8
    assert (out[0] == 0xEE).all() and (out[4] == 0xEEEEEEEE).all() and (tail[0] == 0xEEEE).all()
    assert pkg.live_resources() == before


@pytest.mark.parametrize("name", ["kodak05", "blocks", "noise", "syn1", "spikes", "checker"])
def test_chained_with_no_serial_kernel(gpu_ctx, pkg, oracle, live, name):
    """The fused oracle's own records of a plane at near 0..9 x efforts 1..3 through the entry, its coded bins through the
    host range coder: the body of the oracle's stream."""
    plane = inputs.foreign_planes()[name]
    for effort in (1, 2, 3):
        for near in range(10):
            t = oracle.trace(plane, near, effort)
            rec1 = ci.pack_s1(t["px0"], t["adr"], t["qu"].astype(np.int64), t["qv"].astype(np.int64), t["qw"])
            got = gpu_ctx.debug_entropy_front(plane.reshape(-1), rec1, t["px"].astype(np.uint16) | (t["sign"].astype(np.uint16) << 8), near)
            assert np.array_equal(got["z"], t["z"]) and np.array_equal(got["cnt"], t["bins"]), (name, near, effort)
            assert pkg.range_code(got["coded"]) == t["stream"][16:], (name, near, effort)


def test_refusals_launch_nothing(gpu_ctx, pkg, oracle, live):
    fam = ei.sizes(1)[3]                                                # 65 records
    x, rec, pxs = fam["x"], ei.rec1_of(fam), ei.pxs_of(fam)
    before = (gpu_ctx.serial_launches(), pkg.live_resources())

    def refused(*args):
        with pytest.raises(ValueError):
            gpu_ctx.debug_entropy_front(*args)
        assert (gpu_ctx.serial_launches(), pkg.live_resources()) == before

    for near in (-1, 10, 16):
        refused(x, rec, pxs, near)
    refused(None, rec, pxs, 1)
    refused(x, None, pxs, 1)
    refused(x, rec, None, 1)
    refused(x[:0], rec[:0], pxs[:0], 1)                                  # n 0
    for bad in (512, 0x8000 | int(pxs[0])):
        p = pxs.copy()
        p[40] = bad
        refused(x, rec, p, 1)
    for bad in ((int(rec[0]) & ~(31 << 19)) | (17 << 19),               # qw 17
                int(rec[0]) | (3 << 25),                                # no such relation of qv to qu
                int(ci.pack_s1(np.array([7]), np.array([0]), np.array([0]), np.array([-1]), np.array([3]))[0]),      # qv -1
                int(ci.pack_s1(np.array([7]), np.array([0x700]), np.array([15]), np.array([16]), np.array([3]))[0]), # qv 16
                int(rec[0]) | (1 << 27)):
        r = rec.copy()
        r[33] = bad
        refused(x, r, pxs, 1)
    bad_map = ci.map_init()
    bad_map[60 * 5 + 3] = 4                                               # not a permutation
    refused(x, rec, pxs, 1, bad_map)
    refused(x, rec, pxs, 1, None, np.zeros(8192, np.int32))               # no counter is ever 0
    refused(x, rec, pxs, 1, None, np.full(8192, 4097, np.int32))          # nor above the limit
    lib = pkg.load_library()
    assert lib.nblic_amd_debug_entropy_front(None, 1, *([None] * 3), 0, *([None] * 7), 0, *([None] * 4)) == -1
    n = len(x)
    bufs = [np.zeros(64 * n, t) for t in (np.uint8, np.uint8, np.uint32, np.uint32, np.uint32)]
    tail = [np.zeros(64 * n, np.uint16), np.zeros(512 * 60, np.int32), np.zeros(8192, np.int32), np.zeros(8, np.uint32)]
    ptr = lambda a: a.ctypes.data
    args = [ptr(x), ptr(rec), ptr(pxs), 1, None, None] + [ptr(b) for b in bufs] + [64 * n] + [ptr(b) for b in tail]
    for k in (6, 7, 8, 9, 10, 12, 13, 14, 15):                           # every output pointer
        a = list(args)
        a[k] = None
        assert lib.nblic_amd_debug_entropy_front(gpu_ctx.handle, n, *a) == -1, k
    assert lib.nblic_amd_debug_entropy_front(gpu_ctx.handle, (1 << 22) + 1, *args) == -1      # (refused before anything is read)
    assert (gpu_ctx.serial_launches(), pkg.live_resources()) == before
    check(gpu_ctx, oracle, fam)                                          # and the context still works
