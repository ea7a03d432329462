"""CPU suite: the exact reference of tests/float_edge_inputs.py against numpy and against Python integers, the case against
the older inputs (no witness among them), the witness and regime counts of the new ones, and every domain through the
library's host walks -- the ``#else`` bodies of collect_value, deliver_value and deep_value -- which must equal the reference
everywhere.  tests/test_float_edges.py sends the same domains through the kernels."""
import numpy as np

import collect_inputs
import float_edge_inputs as fe


def _same_f32(got, want):
    """Equal float32 bit patterns, any NaN for any NaN."""
    got, want = np.asarray(got, np.uint32).reshape(-1), np.asarray(want, np.uint32).reshape(-1)
    nan = np.isnan(want.view(np.float32))
    return bool((np.isnan(got.view(np.float32)) == nan).all() and (got[~nan] == want[~nan]).all())


def _numpy_f32(x32, scale, bias):
    """numpy's float32 multiply, then add: two roundings."""
    with np.errstate(all="ignore"):
        prod = x32 * np.float32(scale)
        return (prod + np.float32(bias)).view(np.uint32)


def _numpy_pixels(bits32):
    v = bits32.view(np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(v), 0, np.clip(np.rint(v), 0, 255)).astype(np.uint8)


def _numpy_narrow(bits32, fmt):
    if fmt == 3:
        return bits32
    if fmt == 1:
        with np.errstate(all="ignore"):
            return bits32.view(np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)
    b = bits32.astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)


def _numpy_widen(bits, fmt):
    bits = np.ascontiguousarray(bits)
    if fmt == 1:
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    return bits.view(np.float32) if fmt == 3 else (bits.astype(np.uint32) << 16).view(np.float32)


def test_the_reference_agrees_with_numpy_on_every_domain():
    for d, want in fe.collect_expected():
        x32 = _numpy_widen(d["bits"], d["fmt"])
        assert _same_f32(fe.widen_bits(d["bits"], d["fmt"]), x32.view(np.uint32)), (d["name"], d["fmt"])
        two = fe.contract_f32(fe.widen(d["bits"], d["fmt"]), d["scale"], d["bias"])
        by_numpy = _numpy_f32(x32, d["scale"], d["bias"])
        assert _same_f32(two, by_numpy), (d["name"], d["fmt"], d["scale"], d["bias"])
        assert np.array_equal(want, _numpy_pixels(by_numpy)), (d["name"], d["fmt"], d["scale"], d["bias"])
    px = fe.PIXELS.astype(np.float32)
    for fmt in (1, 2, 3):
        for scale, bias in fe.DELIVER_PAIRS + tuple(fe.DELIVER_FAMILY[::7]):
            by_numpy = _numpy_f32(px, scale, bias)
            assert np.array_equal(fe.contract_f32(fe._of_int(fe.PIXELS), scale, bias), by_numpy), (scale, bias)
            assert np.array_equal(fe.deliver_ref(fe.PIXELS, fmt, scale, bias), _numpy_narrow(by_numpy, fmt)), (fmt, scale, bias)
    for name, (scale, bias) in fe.DEEP_PAIRS.items():
        for signed in (False, True):
            by_numpy = _numpy_f32((fe.DEEP_U - (32768 if signed else 0)).astype(np.float32), scale, bias)
            assert _same_f32(fe.deep_f32(name, signed), by_numpy), (name, signed)
            for fmt in (1, 2, 3):
                assert np.array_equal(fe.narrow_bits(fe.deep_f32(name, signed), fmt), _numpy_narrow(by_numpy, fmt)), (name, signed, fmt)


def test_the_roundings_at_the_formats_ends():
    """The narrowing over every float32 exponent, around 65520, around 2^-25 and among the float16 subnormals; the bfloat16
    NaN; the widening of all 65536 patterns of both half formats; the pixel rule on every half."""
    rng = np.random.default_rng(11)
    bits = np.concatenate([rng.integers(0, 1 << 32, 300000, dtype=np.uint64).astype(np.uint32), np.arange(0x33000000 - 64, 0x33000000 + 64, dtype=np.uint32),
                           np.arange(0x477FE000 - 8, 0x477FF000 + 8, dtype=np.uint32), np.arange(0x38000000, 0x38800000, 0x0FFF, dtype=np.uint32),
                           np.arange(0xB3000000, 0xB8800000, 0x1FFFF, dtype=np.uint32)])
    nan = np.isnan(bits.view(np.float32))
    for fmt in (1, 2):
        assert np.array_equal(fe.narrow_bits(bits, fmt)[~nan], _numpy_narrow(bits, fmt)[~nan]), fmt
    assert fe.narrow_bits(np.array([0x7FC00000, 0xFF800001, 0x7F800001], np.uint32), 2).tolist() == [0x7FC0, 0xFFC0, 0x7FC0]
    assert fe.narrow_bits(np.array([0x7FC00000, 0xFFC00000], np.uint32), 1).tolist() == [0x7E00, 0xFE00]
    every = np.arange(65536, dtype=np.uint32)
    for fmt in (1, 2):
        assert _same_f32(fe.widen_bits(every, fmt), _numpy_widen(every, fmt).view(np.uint32)), fmt
    halves = (np.arange(-20, 600) * 0.5).astype(np.float32)
    assert np.array_equal(fe.pixel_of(halves.view(np.uint32)), np.clip(np.rint(halves), 0, 255).astype(np.uint8))
    assert np.array_equal(fe.pixel_of(bits), _numpy_pixels(bits))


def test_python_integers_give_the_vectorised_reference():
    """The second opinion: every witness input, and a sample of every other domain, one element at a time in Python integers."""
    rng = np.random.default_rng(12)
    checked = 0
    for d, _ in fe.collect_expected():
        flat = d["bits"].reshape(-1)
        pick = flat if d["name"] == "witness set" and d["fmt"] != 3 else flat[rng.integers(0, flat.size, 400)]
        x = fe.widen(pick, d["fmt"])
        two = fe.contract_f32(x, d["scale"], d["bias"])
        for i in np.flatnonzero(~x[3] & ~x[4]):
            assert int(two[i]) == fe.scalar_bits(int(x[0][i]), int(x[1][i]), int(x[2][i]), d["scale"], d["bias"], False), (d["fmt"], d["scale"], d["bias"], hex(int(pick[i])))
            checked += 1
    for name, (scale, bias) in fe.DEEP_PAIRS.items():
        u = rng.integers(0, 65536, 300)
        two = fe.contract_f32(fe._of_int(u - 32768), scale, bias)
        assert [int(v) for v in two] == [fe.scalar_bits(int(v < 32768), abs(int(v) - 32768), 0, scale, bias, False) for v in u], name
    assert checked > 10000


def test_the_older_inputs_hold_no_witness_and_the_new_sets_do():
    """collect_inputs.NORMS over every float16 and bfloat16 pattern: the fused form gives the same float32, element for
    element, so no test on them can tell a contracted kernel from a right one.  The new sets: at least 100 / 50 / 64."""
    for fmt in (1, 2):
        x = fe.widen(collect_inputs.all_patterns(fmt), fmt)
        for scale, bias in collect_inputs.NORMS:
            two, one = fe.contract_f32(x, scale, bias), fe.fused_f32(x, scale, bias)
            assert _same_f32(one, two) and fe.witnesses(fe.pixel_of(two), fe.pixel_of(one)) == 0, (fmt, scale, bias)
    counts = {}
    for fmt in (1, 2, 3):
        scale, bias = fe.COLLECT_WITNESS_PAIR[fmt]
        w = fe.collect_witness_inputs(fmt)
        two, one = fe.collect_ref(w, fmt, scale, bias), fe.collect_ref(w, fmt, scale, bias, fused=True)
        counts[fmt] = (w.size, int(((two > 0) & (two < 255)).sum()), fe.witnesses(two, one))
        assert counts[fmt][2] >= fe.COLLECT_WITNESS_MIN[fmt], (fmt, counts[fmt])
    print("collect witness sets (inputs, pixels inside 1 .. 254, witnesses):", {fe.NAMES[f]: c for f, c in counts.items()})
    assert counts == {1: (909, 886, 128), 2: (368, 354, 62), 3: (32895, 32766, 90)}


def test_large_subnormals_show_a_flushed_denormal():
    """Under 3e38 a kept subnormal of 2^-128 or more is a pixel of 1 or more, a flushed one pixel 0; under (-3e38, 255) a kept
    one is below 255, a flushed one 255.  The bfloat16 subnormals of the all-patterns image are among them."""
    sub = fe.F32_SUBNORMALS
    s, m, e, _, _ = fe._decode(sub)
    lifted = (m >= (1 << 21)) & (s == 0)                       # m * 2^-149 * 3e38 > 0.5
    px = fe.collect_ref(sub, 3, 3e38, 0.0)
    assert int(lifted.sum()) >= 50 and (px[lifted] >= 1).all() and (px[~lifted] == 0).all()
    px = fe.collect_ref(sub, 3, -3e38, 255.0)
    assert (px[lifted] <= 254).all()
    lifted_neg = (m >= (1 << 21)) & (s == 1)
    assert int(lifted.sum() + lifted_neg.sum()) >= 64 and (fe.collect_ref(sub, 3, -3e38, 0.0)[lifted_neg] >= 1).all()
    bf = np.arange(0x0020, 0x0080, dtype=np.uint32)           # bfloat16 subnormals from 2^-128 on
    assert (fe.collect_ref(bf, 2, 3e38, 0.0) >= 1).all()
    in_domain = [d for d, _ in fe.collect_expected() if d["fmt"] == 3 and d["scale"] == 3e38]
    assert len(in_domain) == 1 and np.isin(sub, in_domain[0]["bits"]).all()
    print("float32 subnormals lifted into pixel range under 3e38:", int(lifted.sum()), "positive,", int(lifted_neg.sum()), "negative")


def test_the_deliver_pairs_are_what_the_search_finds():
    found = fe.deliver_search()
    print("deliver witnesses among 256 pixels, by the search over %d pairs:" % len(fe.DELIVER_FAMILY), {fe.NAMES[f]: v for f, v in found.items()})
    assert found == fe.DELIVER_FOUND
    assert found[1][0] == 21 and found[2][0] == 16 and found[3][0] == 158
    px = fe.PIXELS
    assert fe.witnesses(fe.deliver_ref(px, 3, *fe.DELIVER_F32_PAIR), fe.deliver_ref(px, 3, *fe.DELIVER_F32_PAIR, fused=True)) == 158
    assert fe.witnesses(fe.deliver_ref(px, 1, *fe.DELIVER_F32_PAIR), fe.deliver_ref(px, 1, *fe.DELIVER_F32_PAIR, fused=True)) == 0
    assert int(fe.on_tie(fe.contract_f32(fe._of_int(px), *fe.DELIVER_TIE_PAIRS[0]), 1).sum()) == 128
    assert int(fe.on_tie(fe.contract_f32(fe._of_int(px), *fe.DELIVER_TIE_PAIRS[1]), 2).sum()) == 128
    assert int(fe.deliver_ref(px[:1], 3, -1.0, 0.0)[0]) == 0 and int(fe.deliver_ref(px[:1], 3, -1.0, -0.0)[0]) == 0x80000000
    assert int(fe.deliver_ref(px[:1], 1, -1.0, -0.0)[0]) == 0x8000


def test_the_deep_domain_reaches_every_regime():
    r = fe.deep_regimes()
    print("deep deliver regimes (elements, by the reference):", {"%s, %s" % (k[0], fe.NAMES[k[1]]): v for k, v in r.items()})
    for fmt in (1, 2, 3):
        assert r[("infinite", fmt)] > 0 and r[("negative scale", fmt)] > 0 and r[("witness", fmt)] >= 32, (fmt, r)
    assert r[("subnormal", 1)] > 0 and r[("tie", 1)] > 0 and r[("tie", 2)] > 0
    two = fe.narrow_bits(fe.deep_f32("identity", False).reshape(-1)[:65536], 1)
    assert (two[65520:] == 0x7C00).all() and two[65519] == 0x7BFF


# ---- the host walks --------------------------------------------------------------------------------------------------------------
def test_collect_host_equals_the_reference(pkg):
    for k, (d, want) in enumerate(fe.collect_expected()):
        for layout in ("contiguous", "strided"):
            t = fe.collect_task(d, layout, k)
            got = pkg.collect_host(t["raw"], t["fmt"], t["scale"], t["bias"], pitch=t["pitch"], step=t["step"], rows=t["rows"], cols=t["cols"])
            assert np.array_equal(got, want), fe.explain_plane("collect_host, %s, %s" % (d["name"], layout), d["fmt"], d["scale"], d["bias"], d["bits"], got, want)
    t, own, ref, want = fe.collect_ref_task()
    got = pkg.collect_host(t["raw"], 1, t["scale"], t["bias"], pitch=t["pitch"], step=t["step"], rows=t["rows"], cols=t["cols"], ref=ref)
    assert np.array_equal(got, want), fe.explain_plane("collect_host with a reference", 1, t["scale"], t["bias"], own, got, want)


def test_deliver_host_equals_the_reference(pkg):
    for t, want in fe.deliver_tasks() + fe.deliver_ref_tasks():
        got = pkg.deliver_host(t["plane"], t["window"], t["fmt"], t["scale"], t["bias"], pitch=t["pitch"], offset=t["offset"], out_bytes=t["out_bytes"],
                               step=t["step"], ref=t.get("ref"))
        assert np.array_equal(got, want), fe.explain_buffer("deliver_host", t["fmt"], t["scale"], t["bias"], t, fe.PIXEL_PLANE, got, want)


def test_deep_deliver_host_equals_the_reference(pkg):
    inverse = {v: k for k, v in fe.DEEP_FMT.items()}
    for t, want in fe.deep_tasks():
        got = pkg.deep_deliver_host(t["hi"], t["lo"], t["window"], t["fmt"], t["mode"], t["scale"], t["bias"], pitch=t["pitch"], offset=t["offset"],
                                    out_bytes=t["out_bytes"], step=t["step"])
        values = fe.DEEP_U - (32768 if t["mode"] & 2 else 0)
        assert np.array_equal(got, want), fe.explain_buffer("deep_deliver_host, %s, mode %d" % (t["pair"], t["mode"]), inverse[t["fmt"]], t["scale"], t["bias"], t, values, got, want)


def test_stack_deliver_host_equals_the_reference(pkg):
    for t, want, slices in fe.stack_tasks():
        assert all(sorted(x.reshape(-1).tolist()) == list(range(256)) for x in slices)
        got = pkg.stack_deliver_host(t["planes"], t["window"], t["fmt"], t["scales"], t["biases"], t["pitches"], t["steps"], t["offsets"], t["out_bytes"])
        for d, (g, w) in enumerate(zip(got, want)):
            dest = dict(offset=t["offsets"][d], pitch=t["pitches"][d], step=t["steps"][d])
            assert np.array_equal(g, w), fe.explain_buffer("stack_deliver_host, slice %d" % d, t["fmt"], t["scales"][d], t["biases"][d], dest, slices[d], g, w)


def test_the_cost_host_walks_equal_numpy_on_the_reference_planes(pkg):
    for (kind, fmt), (t, planes) in fe.cost_tasks().items():
        assert all(len(np.unique(p)) > 200 for p in planes)
        if kind == "color":
            got = pkg.color_cost_host(t["raws"], t["rows"], t["cols"], fmt, t["pitches"], t["steps"], t["scale"], t["bias"])
            want = pkg.color_cost_numpy(*planes)
        else:
            got = pkg.stack_cost_host(t["raws"], t["rows"], t["cols"], fmt, t["pitches"], t["steps"], t["scale"], t["bias"])
            want = pkg.stack_cost_numpy(planes)
        assert np.array_equal(got, want), (kind, fe.NAMES[fmt], t["scale"], t["bias"], got.tolist(), want.tolist())


def test_a_fused_conversion_would_change_every_launch():
    """What tests/test_float_edges.py can see: the elements of each launch's inputs on which the fused form differs from
    the contract in the final output."""
    seen = {"collect": 0, "deliver": 0, "deliver with a reference": 0, "deep deliver": fe.deep_regimes()[("witness", 1)] + fe.deep_regimes()[("witness", 2)]
            + fe.deep_regimes()[("witness", 3)], "stack deliver": 0}
    for d, want in fe.collect_expected():
        if d["name"] == "witness set":
            seen["collect"] += fe.witnesses(want, fe.collect_ref(d["bits"], d["fmt"], d["scale"], d["bias"], fused=True))
    for t, _ in fe.deliver_tasks():
        seen["deliver"] += fe.witnesses(fe.deliver_ref(t["plane"], t["fmt"], t["scale"], t["bias"]), fe.deliver_ref(t["plane"], t["fmt"], t["scale"], t["bias"], fused=True))
    for t, _ in fe.deliver_ref_tasks():
        seen["deliver with a reference"] += fe.witnesses(fe.deliver_ref(fe.PIXEL_PLANE, t["fmt"], t["scale"], t["bias"]),
                                                         fe.deliver_ref(fe.PIXEL_PLANE, t["fmt"], t["scale"], t["bias"], fused=True))
    for t, _, slices in fe.stack_tasks():
        for x, s, b in zip(slices, t["scales"], t["biases"]):
            seen["stack deliver"] += fe.witnesses(fe.deliver_ref(x, t["fmt"], s, b), fe.deliver_ref(x, t["fmt"], s, b, fused=True))
    print("elements a fused conversion changes, per launch (at least):", seen)
    assert all(v >= 16 for v in seen.values()), seen
