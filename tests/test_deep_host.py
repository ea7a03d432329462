"""CPU suite: deep pixels on the host -- the three walks of csrc/deep.h that the kernels' lanes share (collect, deliver, cost)
against numpy expressions written independently in tests/deep_inputs.py, the round trip of every 16-bit value, the rule,
the float formats' edges, and what is refused.  No device: the hooks used here are host only."""
import ctypes as C

import numpy as np
import pytest

import deep_inputs as di


@pytest.fixture(scope="module")
def collect_cases():
    return di.collect_tasks()


@pytest.fixture(scope="module")
def deliver_cases():
    return di.deliver_tasks()


@pytest.fixture(scope="module")
def cost_cases():
    return di.cost_tasks()


def host_collect(pkg, t, info=None):
    return pkg.deep_collect_host(t["full"], t["fmt"], t["part"], pitch=t["pitch"], step=t["step"], offset=t["offset"], rows=t["rows"], cols=t["cols"],
                                 px_range=t.get("px_range"), info=info)


def host_deliver(pkg, t, info=None):
    return pkg.deep_deliver_host(t["hi"], t["lo"], t["window"], t["fmt"], t["mode"], scale=t.get("scale", 1.0), bias=t.get("bias", 0.0), pitch=t.get("pitch"),
                                 offset=t["offset"], out_bytes=t["out_bytes"], zero=t.get("zero", False), gate_status=t.get("gate_status", (-1, -1)),
                                 step=t.get("step"), info=info)


def host_cost(pkg, t, info=None):
    return pkg.deep_cost_host(t["full"], t["fmt"], pitch=t["pitch"], step=t["step"], offset=t["offset"], rows=t["rows"], cols=t["cols"], info=info)


def test_round_trip_of_every_value_and_both_parities(pkg):
    x = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    for signed in (False, True):
        src = x.view(np.int16) if signed else x
        for fold in (0, 1):
            mode = fold | (2 if signed else 0)
            hi, lo = pkg.deep_forward(src, mode)
            want_hi, want_lo = di.planes_numpy(src, fold)
            assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo)
            back = pkg.deep_inverse(hi, lo, mode)
            assert back.dtype == src.dtype and np.array_equal(back, src)
    hi, lo = pkg.deep_forward(x, 1)                              # the fold makes the low byte continuous: neighbours in value differ by at most one
    assert int(np.abs(np.diff(lo.reshape(-1).astype(np.int64))).max()) == 1
    assert int(np.abs(np.diff(pkg.deep_forward(x, 0)[1].reshape(-1).astype(np.int64))).max()) == 255
    with pytest.raises(ValueError):
        pkg.deep_forward(x, 2)                                   # bit 1 and the dtype disagree
    with pytest.raises(ValueError):
        pkg.deep_forward(x.view(np.int16), 1)
    with pytest.raises(ValueError):
        pkg.deep_forward(x.astype(np.uint8), 0)


def test_edge_values_through_the_walks(pkg):
    u = np.array([di.EDGE_U], np.uint16)
    s = np.array([di.EDGE_I16], np.int16)
    for x in (u, s, (u ^ np.uint16(0x8000)).view(np.int16)):
        signed = x.dtype == np.int16
        for part in range(3):
            assert np.array_equal(pkg.deep_collect_host(x, int(signed), part), di.part_numpy(x, part))
        for fold in (0, 1):
            mode = fold | (2 if signed else 0)
            hi, lo = di.planes_numpy(x, fold)
            out = pkg.deep_deliver_host(hi, lo, (0, 1, 0, x.shape[1]), 1 if signed else 0, mode)
            assert np.array_equal(out.view(x.dtype).reshape(x.shape), x)
            f = pkg.deep_deliver_host(hi, lo, (0, 1, 0, x.shape[1]), 4, mode)
            assert np.array_equal(f.view(np.float32).reshape(x.shape), x.astype(np.float32))
    assert np.array_equal(np.asarray(s, np.int64) + 32768, [[0, 32767, 32768]])


def test_collect_walk_against_numpy(pkg, collect_cases):
    for t in collect_cases:
        info = {}
        got = host_collect(pkg, t, info)
        assert np.array_equal(got, di.expected_plane(t)), (t["rows"], t["cols"], t["fmt"], t["part"], t["step"])
        p0, p1 = t.get("px_range", (0, 0))
        p1 = p1 or t["rows"] * t["cols"]
        assert info["units"] == (p1 + 15) // 16 - p0 // 16 and info["chunks"] == (info["units"] + 1023) // 1024
    assert max(t["rows"] * t["cols"] for t in collect_cases) > 16 * 1024


def test_collect_reads_nothing_but_elements(pkg, collect_cases):
    """The bytes between the elements are 0xFF in every layout: a plane that equals numpy's has taken none of them for an
    element, and a cap that ends with the last element is enough."""
    for t in collect_cases:
        cap = (t["rows"] - 1) * t["pitch"] + (t["cols"] - 1) * t["step"] + 2
        got = pkg.deep_collect_host(t["full"], t["fmt"], t["part"], pitch=t["pitch"], step=t["step"], offset=t["offset"], rows=t["rows"], cols=t["cols"], cap=cap)
        assert np.array_equal(got, di.part_numpy(t["image"], t["part"]))
        with pytest.raises(ValueError):
            pkg.deep_collect_host(t["full"], t["fmt"], t["part"], pitch=t["pitch"], step=t["step"], offset=t["offset"], rows=t["rows"], cols=t["cols"], cap=cap - 1)


def test_deliver_walk_against_numpy(pkg, deliver_cases):
    seen = set()
    for t in deliver_cases:
        info = {}
        got = host_deliver(pkg, t, info)
        want = di.expected_buffer(t)
        assert np.array_equal(got, want), (t["window"], t["fmt"], t["mode"], t.get("step"), t.get("gate_status"))
        seen.add((t["fmt"], t["mode"]))
        assert info["chunks"] == (info["units"] + 1023) // 1024
    assert {f for f, _ in seen} == {0, 1, 2, 3, 4} and {m for _, m in seen} == {0, 1, 2, 3}
    assert any(t.get("gate_status", (1, 1)) not in ((1, 1), (-1, -1)) for t in deliver_cases) and any(t.get("zero") for t in deliver_cases)
    assert any(t["offset"] % 16 == 2 and "step" not in t for t in deliver_cases)


def test_float16_edges(pkg):
    """Values above 65504 go to float16 infinity at scale 1 (65520 and above; 65505 .. 65519 round down to 65504), and round as
    numpy rounds with a scale that brings them into range; negative values of an int16 image likewise."""
    u = np.array([[0, 1, 2047, 2048, 2049, 4097, 65503, 65504, 65505, 65519, 65520, 65521, 65535, 32768, 32767, 40001]], np.uint16)
    hi, lo = di.planes_numpy(u, 0)
    win = (0, 1, 0, u.shape[1])
    for scale, bias in ((1.0, 0.0), (0.5, 0.0), (1.0 / 65535.0, 0.0), (1.0, -32768.0), (3.0, 0.25)):
        for fmt, dtype in ((2, np.float16), (4, np.float32)):
            got = pkg.deep_deliver_host(hi, lo, win, fmt, 0, scale=scale, bias=bias).view(dtype)
            with np.errstate(over="ignore"):
                want = ((u.astype(np.float32) * np.float32(scale)) + np.float32(bias)).astype(dtype).reshape(-1)
            assert np.array_equal(got.view(np.uint16 if fmt == 2 else np.uint32), want.view(np.uint16 if fmt == 2 else np.uint32)), (scale, bias, fmt)
    inf = pkg.deep_deliver_host(hi, lo, win, 2, 0).view(np.float16)
    assert np.isinf(inf[10:13]).all() and np.isfinite(inf[:10]).all() and float(inf[9]) == 65504.0
    s = (u ^ np.uint16(0x8000)).view(np.int16)
    shi, slo = di.planes_numpy(s, 1)
    got = pkg.deep_deliver_host(shi, slo, win, 3, 3, scale=0.25, bias=1.0)
    assert np.array_equal(got.view(np.uint16), di.value_bits(di.unsigned_of(s), 3, 3, 0.25, 1.0).reshape(-1))


def test_cost_walk_against_numpy(pkg, cost_cases):
    for t in cost_cases:
        info = {}
        got = host_cost(pkg, t, info)
        assert np.array_equal(got, di.sums_numpy(t["image"])), (t["rows"], t["cols"], t["fmt"], t["step"])
        assert info["tiles"] == ((t["rows"] + 63) // 64) * ((t["cols"] + 63) // 64)


def test_cost_is_not_wrapped(pkg):
    """A sawtooth's jump of 255 costs 2 * 8 + 1, not the 3 of a wrapped residual: the reason the fold is seen at all."""
    x = np.array([[255, 256]], np.uint16)                        # low bytes 255, 0; high bytes 0, 1
    sums = pkg.deep_cost_host(x, 0)
    assert int(sums[1]) == (2 * 7 + 1) + (2 * 8 + 1)             # |255 - 128| = 127, then |0 - 255| = 255
    assert int(sums[2]) == (2 * 7 + 1) + 1                       # folded: 255, 255
    assert pkg.deep_choose(sums[:3], 0) == 1


def test_the_rule(pkg):
    assert pkg.deep_choose([7, 10, 9], 0) == 1 and pkg.deep_choose([7, 10, 9], 1) == 3
    assert pkg.deep_choose([7, 10, 10], 0) == 0 and pkg.deep_choose([7, 10, 10], 1) == 2      # a tie is plain
    assert pkg.deep_choose([7, 9, 10], 0) == 0
    big = 2 ** 64 - 1
    assert pkg.deep_choose([0, big, big - 1], 0) == 1 and pkg.deep_choose([0, big, big], np.int16) == 2      # no margin, at any size
    assert pkg.deep_choose([0, 64, 63], 0) == 1                  # (the colour rule's 63/64 would say no)
    with pytest.raises(ValueError):
        pkg.deep_choose([1, 2, 3], 2)
    assert [pkg.deep_mode_valid(m) for m in (0, 1, 2, 3, 4, 0xFF, -1)] == [True] * 4 + [False] * 3


def test_the_classes_plan_as_the_oracle_encodes(pkg, oracle):
    """On every class the mode chosen from the host walk's costs is the one whose two streams are smaller at -e1, and the
    classes whose costs tie plan as plain.  (deep_inputs says which class of the issue's table was replaced, and why.)"""
    for name, want in di.CLASSES.items():
        x = di.class_image(name)
        sums = pkg.deep_cost_host(x, 0)
        mode = pkg.deep_choose(sums[:3], 0)
        size = []
        for m in (0, 1):
            hi, lo = pkg.deep_forward(x, m)
            size.append(len(oracle.encode(hi, 0, 1)[0]) + len(oracle.encode(lo, 0, 1)[0]))
        print(name, sums.tolist(), size)
        if name in di.TIES:
            assert sums[1] == sums[2] and size[0] == size[1] and mode == 0
        else:
            assert mode == want == (1 if size[1] < size[0] else 0), (name, sums.tolist(), size)
            assert abs(int(sums[1]) - int(sums[2])) >= 0.009 * int(sums[1])          # the proxy's margin on every class that is no tie


def _collect_args(x, **over):
    a = dict(src=x.ctypes.data, cap=x.nbytes, rows=x.shape[0], cols=x.shape[1], pitch=x.strides[0], step=2, fmt=0, part=0, rng=None, out_bytes=None)
    a.update(over)
    return a


def test_refusals_of_the_host_hooks(pkg):
    lib = pkg.load_library()
    x = np.arange(12 * 20, dtype=np.uint16).reshape(12, 20)
    store = np.zeros(x.size + 32, np.uint8)
    out = store[(-store.ctypes.data) % 16:]

    def collect(**over):
        a = _collect_args(x, **over)
        return lib.nblic_amd_debug_deep_collect_host(a["src"], a["cap"], a["rows"], a["cols"], a["pitch"], a["step"], a["fmt"], a["part"], a["rng"],
                                                     out.ctypes.data + over.get("out_shift", 0), x.size if a["out_bytes"] is None else a["out_bytes"], None, None)
    assert collect() == 0
    for bad in (dict(src=None), dict(src=x.ctypes.data + 1), dict(pitch=41), dict(step=3), dict(step=0), dict(step=(1 << 20) + 2), dict(fmt=2), dict(fmt=-1),
                dict(part=3), dict(part=-1), dict(rows=0), dict(cols=65536), dict(cap=x.nbytes - 1), dict(out_shift=8), dict(out_bytes=x.size - 1),
                dict(rng=(C.c_int * 2)(5, 4)), dict(rng=(C.c_int * 2)(0, x.size + 1)), dict(rng=(C.c_int * 2)(-1, 0))):
        assert collect(**bad) == -1, bad
    sums = (C.c_ulonglong * 5)()
    cost = lambda **o: lib.nblic_amd_debug_deep_cost_host(o.get("src", x.ctypes.data), o.get("cap", x.nbytes), 12, 20, o.get("pitch", 40), o.get("step", 2), o.get("fmt", 0),
                                                          o.get("sums", sums), None)
    assert cost() == 0
    for bad in (dict(src=None), dict(sums=None), dict(cap=x.nbytes - 1), dict(pitch=38 + 1), dict(step=1), dict(fmt=2)):
        assert cost(**bad) == -1, bad
    hi, lo = di.planes_numpy(x, 0)
    ok = dict(window=(0, 12, 0, 20), fmt=0, mode=0)
    assert pkg.deep_deliver_host(hi, lo, **ok).size == x.nbytes
    for bad in (dict(mode=2), dict(fmt=1), dict(fmt=1, mode=0), dict(mode=4), dict(mode=0xFF), dict(fmt=5), dict(fmt=-1), dict(window=(0, 13, 0, 20)),
                dict(window=(0, 12, 0, 21)), dict(window=(3, 3, 0, 20)), dict(offset=1), dict(pitch=38), dict(step=3), dict(scale=2.0), dict(bias=1.0),
                dict(fmt=2, scale=float("nan")), dict(fmt=4, offset=2), dict(out_bytes=x.nbytes - 1), dict(step=(1 << 20) + 2)):
        with pytest.raises(ValueError):
            pkg.deep_deliver_host(hi, lo, **{**ok, **bad})
    assert pkg.deep_deliver_host(hi, lo, (0, 12, 0, 20), 1, 2).size == x.nbytes       # int16 takes the signed modes only
