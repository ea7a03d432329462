"""CPU suite: the reversible colour transform on the host.  rct_forward / rct_inverse on the exhaustive frame; the collect
walk with a reference source against rct_forward of the separately collected planes; the delivery walk with a reference
plane against rct_inverse followed by the walk without one; and the references that the task checks refuse."""
import numpy as np
import pytest

from collect_inputs import ELEM, as_values, element_bits, lay_out
from rct_inputs import collect_tasks, deliver_tasks, exhaustive_frame, gated_off_frame, plain_collect_tasks, rct_forward_int16


def test_forward_and_inverse_on_the_exhaustive_frame(pkg):
    r, g, b = exhaustive_frame()
    assert len({(int(x), int(y)) for x, y in zip(r.reshape(-1), g.reshape(-1))}) == 65536
    assert len({(int(x), int(y)) for x, y in zip(b.reshape(-1), g.reshape(-1))}) == 65536
    t = pkg.rct_forward(r, g, b)
    want = rct_forward_int16(r, g, b)
    assert all(a.dtype == np.uint8 and np.array_equal(a, w) for a, w in zip(t, want))
    assert t[0][0, 0] == 128 and t[0][0, 255] == 129 and t[0][255, 0] == 127       # 0 - 0, 0 - 255 and 255 - 0, each + 128 mod 256
    back = pkg.rct_inverse(*t)
    assert all(np.array_equal(a, w) for a, w in zip(back, (r, g, b)))
    with pytest.raises(ValueError):
        pkg.rct_forward(r, g[:, :255], b)
    with pytest.raises(ValueError):
        pkg.rct_inverse(r.astype(np.int16), g, b)


def _collect(pkg, t, with_ref=True, source="raw"):
    pitch, step = (t["pitch"], t["step"]) if source == "raw" else (t["ref_pitch"], t["ref_step"])
    kw = dict(ref=t["ref"], ref_pitch=t["ref_pitch"], ref_step=t["ref_step"]) if with_ref else {}
    return pkg.collect_host(t[source], t["fmt"], t["scale"], t["bias"], pitch=pitch, step=step, rows=t["rows"], cols=t["cols"], px_range=t.get("px_range"), **kw)


def test_collect_walk_with_a_reference(pkg):
    """Every task of the shared list: the walk with a reference equals rct_forward of the two planes the walk collects
    without one, which in turn are numpy's; outside a pixel range the plane keeps its pattern."""
    tasks = collect_tasks()
    assert {t["fmt"] for t in tasks} == {0, 1, 2, 3} and {(t["rows"], t["cols"]) for t in tasks} >= {(1, 1), (1, 17), (3, 5), (17, 33), (129, 129), (256, 256)}
    assert any(t["pitch"] != t["ref_pitch"] and t["step"] != t["ref_step"] for t in tasks)
    assert pkg.collect_units(129, 129) == (1041, 2)
    specials = 0
    for i, t in enumerate(tasks):
        fmt, n = t["fmt"], t["rows"] * t["cols"]
        got = _collect(pkg, t).reshape(-1)
        own = pkg.collect_numpy(as_values(t["bits"], fmt), fmt, t["scale"], t["bias"])
        ref = pkg.collect_numpy(as_values(t["ref_bits"], fmt), fmt, t["scale"], t["bias"])
        px0, px1 = t.get("px_range", (0, 0))
        px1 = px1 or n
        if "px_range" not in t:
            assert np.array_equal(_collect(pkg, t, with_ref=False).reshape(-1), own.reshape(-1)), i
            assert np.array_equal(_collect(pkg, t, with_ref=False, source="ref").reshape(-1), ref.reshape(-1)), i
        want = pkg.rct_forward(own, ref, own)[0].reshape(-1)
        what = (i, {k: v for k, v in t.items() if k not in ("raw", "ref", "bits", "ref_bits")})
        assert np.array_equal(got[px0:px1], want[px0:px1]), what
        assert (got[:px0] == pkg.COLLECT_PATTERN).all() and (got[px1:] == pkg.COLLECT_PATTERN).all(), what
        if fmt:
            v = as_values(t["bits"], fmt) if fmt != 2 else (t["bits"].astype(np.uint32) << 16).view(np.float32)
            with np.errstate(all="ignore"):
                x = v.astype(np.float32) * np.float32(t["scale"]) + np.float32(t["bias"])
                specials |= 1 * bool(np.isnan(x).any()) | 2 * bool((x < 0).any()) | 4 * bool((x > 255).any()) | 8 * bool(((x > 0) & (x < 255) & (x % 1 == 0.5)).any())
    assert specials == 15                                      # NaN, values that clamp at 0 and at 255, and ties all occur
    # a 2-D view as the reference: its strides say where the elements lie
    r, g, b = exhaustive_frame()
    frame = np.ascontiguousarray(np.stack([r, g, b], axis=-1))
    assert np.array_equal(pkg.collect_host(frame[:, :, 2], 0, ref=frame[:, :, 1]), rct_forward_int16(r, g, b)[2])


def test_collect_refuses_a_bad_reference(pkg):
    rng = np.random.default_rng(3)
    bits, ref_bits = element_bits(rng, 1, (6, 9)), element_bits(rng, 1, (6, 9))
    raw, ref = lay_out(bits, 1, 20, 2, 0), lay_out(ref_bits, 1, 40, 4, 0)
    sound = dict(pitch=20, step=2, rows=6, cols=9, ref=ref, ref_pitch=40, ref_step=4)
    pkg.collect_host(raw, 1, **sound)
    for bad in (dict(ref_offset=1), dict(ref_step=3), dict(ref_pitch=41), dict(ref_step=0), dict(ref_cap=ref.size - 1), dict(ref=ref[:-1]),
                dict(ref_step=(1 << 20) + 2, ref_cap=1 << 40), dict(ref_pitch=(1 << 40) + 2, ref_cap=1 << 62), dict(ref_pitch=0)):
        with pytest.raises(ValueError):
            pkg.collect_host(raw, 1, **dict(sound, **bad))
    with pytest.raises(ValueError):                            # a view of another shape
        pkg.collect_host(as_values(bits, 1), 1, ref=as_values(ref_bits, 1)[:, :8])


def _deliver(pkg, t, plane=None, **over):
    kw = dict(pitch=t.get("pitch"), offset=t.get("offset", 0), out_bytes=t.get("out_bytes"), step=t.get("step"))
    kw.update(over)
    return pkg.deliver_host(t["plane"] if plane is None else plane, t["window"], t["fmt"], t.get("scale", 1.0), t.get("bias", 0.0), **kw)


def test_deliver_walk_with_a_reference(pkg):
    """Every task of the shared list: the walk with a reference equals the walk without one over the plane that rct_inverse
    makes, pattern bytes included."""
    tasks = deliver_tasks()
    assert {t["fmt"] for t in tasks} == {0, 1, 2, 3} and any("step" in t for t in tasks) and any("step" not in t and t.get("offset", 0) % 16 for t in tasks)
    assert any(t["window"][2] > 0 and (t["window"][3] - t["window"][2]) % 16 for t in tasks)
    assert pkg.deliver_units(129, 129, 0) == (129 * 9, 2)                 # the 129 x 129 window: two chunks
    for i, t in enumerate(tasks):
        got = _deliver(pkg, t, ref=t["ref"], gate_status=t["gate_status"])
        plain = pkg.rct_inverse(t["plane"], t["ref"], t["plane"])[0]
        want = _deliver(pkg, t, plane=plain)
        assert np.array_equal(got, want), (i, {k: v for k, v in t.items() if k not in ("plane", "ref")})
    # one of the three not done: zeros, whichever it is
    t = tasks[1]
    zeros = _deliver(pkg, t, zero=True)
    for gates in ((0, 1, 1), (1, 2, 1), (1, 1, -7), (3, 3, 3)):
        assert np.array_equal(_deliver(pkg, t, ref=t["ref"], gate_status=gates), zeros), gates
    assert np.array_equal(_deliver(pkg, t, ref=t["ref"], gate_status=(1, 1, 1), zero=True), zeros)
    for t in gated_off_frame():
        got = _deliver(pkg, t, ref=t["ref"], gate_status=t["gate_status"])
        if t["frame"] == 1:
            assert np.array_equal(got, _deliver(pkg, t, zero=True))
        else:
            plain = t["plane"] if t["ref"] is None else pkg.rct_inverse(t["plane"], t["ref"], t["plane"])[0]
            assert np.array_equal(got, _deliver(pkg, t, plane=plain))


def test_deliver_refuses_a_bad_reference(pkg):
    rng = np.random.default_rng(4)
    plane, ref = rng.integers(0, 256, (8, 21), dtype=np.uint8), rng.integers(0, 256, (8, 21), dtype=np.uint8)
    pkg.deliver_host(plane, (2, 8, 3, 21), 1, ref=ref)
    pkg.deliver_host(plane, (2, 6, 3, 21), 1, ref=ref[:6])       # a reference that holds the window's rows and no more
    with pytest.raises(ValueError):                            # ... and one that ends a row early: its extent is beyond its bytes
        pkg.deliver_host(plane, (2, 8, 3, 21), 1, ref=ref[:7])
    with pytest.raises(ValueError):                            # it does not reach the window's first row
        pkg.deliver_host(plane, (2, 8, 3, 21), 1, ref=ref[:2])
    with pytest.raises(ValueError):                            # another width: its pitch is not the plane's
        pkg.deliver_host(plane, (2, 8, 3, 20), 1, ref=ref[:, :20])
    with pytest.raises(ValueError):
        pkg.deliver_host(plane, (2, 8, 3, 21), 1, ref=ref, gate_status=(1, 1))


def test_plain_tasks_are_what_they_were(pkg):
    """A task without a reference through the new hooks is the old hooks' task."""
    for t in plain_collect_tasks():
        a = pkg.collect_host(t["raw"], t["fmt"], t["scale"], t["bias"], pitch=t["pitch"], step=t["step"], rows=t["rows"], cols=t["cols"])
        assert np.array_equal(a, pkg.collect_numpy(as_values(t["bits"], t["fmt"]), t["fmt"], t["scale"], t["bias"]))
    plane = np.arange(7 * 19, dtype=np.uint8).reshape(7, 19)
    for fmt in range(4):
        e = ELEM[fmt]
        a = pkg.deliver_host(plane, (1, 6, 2, 19), fmt, offset=e, gate_status=(1, 1, 1))
        assert np.array_equal(a, pkg.deliver_host(plane, (1, 6, 2, 19), fmt, offset=e))
