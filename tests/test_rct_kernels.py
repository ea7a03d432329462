"""GPU suite (-m gpu): k_collect and k_deliver on tasks with a reference, ONE launch each through the debug hooks
(nblic_amd_debug_collect_ref, nblic_amd_debug_deliver_ref), byte for byte against the host walks on the task lists of
tests/test_rct_host.py: the exhaustive frame, the 129 x 129 chunk crossing, launches that mix referenced and plain tasks,
a delivery launch with one gated-off frame.  Bytes outside the written elements keep their pattern."""
import numpy as np
import pytest

from rct_inputs import collect_tasks, deliver_tasks, gated_off_frame, plain_collect_tasks

pytestmark = pytest.mark.gpu

GUARD = 256
INTERNAL = ("bits", "ref_bits", "frame", "channel")


def _hook(t):
    return {k: v for k, v in t.items() if k not in INTERNAL}


def _shown(t):
    return {k: v for k, v in t.items() if k not in ("raw", "ref", "plane", "bits", "ref_bits")}


def test_collect_kernel_matches_the_host_walk(gpu_ctx, pkg):
    """Referenced tasks of all four formats and plain ones between them, in ONE launch."""
    tasks = collect_tasks()
    plain = plain_collect_tasks()
    for k, t in enumerate(plain):
        tasks.insert(5 + 11 * k, t)
    assert sum(1 for t in tasks if t["ref"] is None) == 4 and sum(1 for t in tasks if t["ref"] is not None) > 100
    assert any((t["rows"], t["cols"]) == (256, 256) for t in tasks) and any((t["rows"], t["cols"]) == (129, 129) and "px_range" not in t for t in tasks)
    live = pkg.live_resources()
    outs = gpu_ctx.debug_collect_ref([_hook(t) for t in tasks])
    assert pkg.live_resources() == live and len(outs) == len(tasks)
    for i, (t, got) in enumerate(zip(tasks, outs)):
        n = t["rows"] * t["cols"]
        kw = dict(ref=t["ref"], ref_pitch=t["ref_pitch"], ref_step=t["ref_step"]) if t["ref"] is not None else {}
        host = pkg.collect_host(t["raw"], t["fmt"], t["scale"], t["bias"], pitch=t["pitch"], step=t["step"], rows=t["rows"], cols=t["cols"],
                                px_range=t.get("px_range"), **kw)
        assert np.array_equal(got[GUARD:GUARD + n], host.reshape(-1)), (i, _shown(t))      # (outside a pixel range both hold the pattern)
        assert (got[:GUARD] == pkg.COLLECT_PATTERN).all() and (got[GUARD + n:] == pkg.COLLECT_PATTERN).all(), (i, _shown(t))
    # the plain hook still runs a plain task, and a bad reference is refused with nothing launched
    t = plain[1]
    old = gpu_ctx.debug_collect([{k: v for k, v in _hook(t).items() if k != "ref"}])[0]
    assert np.array_equal(old, next(o for u, o in zip(tasks, outs) if u is t))
    sound = _hook(tasks[0])
    e = pkg.DELIVER_ELEM[sound["fmt"]]
    for bad in (dict(ref=sound["ref"][:-1]), dict(ref_step=(1 << 20) + e), dict(ref_base_offset=256), dict(ref_pitch=0)):
        with pytest.raises(ValueError):
            gpu_ctx.debug_collect_ref([sound, dict(sound, **bad)])


def _host(pkg, t, size):
    return pkg.deliver_host(t["plane"], t["window"], t["fmt"], t.get("scale", 1.0), t.get("bias", 0.0), pitch=t.get("pitch"), offset=t.get("offset", 0),
                            out_bytes=size, zero=t.get("zero", False), gate_status=t.get("gate_status", -1), step=t.get("step"), ref=t.get("ref"))


def test_deliver_kernel_matches_the_host_walk(gpu_ctx, pkg):
    """Referenced tasks of all four formats -- contiguous with head and tail units, strided, two chunks, the exhaustive
    frame -- two frames of which one is gated off, and plain tasks, in ONE launch."""
    tasks = deliver_tasks() + gated_off_frame()
    rng = np.random.default_rng(5)
    plane = rng.integers(0, 256, (9, 70), dtype=np.uint8)
    for fmt in range(4):
        e = pkg.DELIVER_ELEM[fmt]
        tasks.insert(7 * fmt + 2, dict(plane=plane, window=(1, 9, 3, 70), fmt=fmt, offset=e, out_bytes=e + 8 * 67 * e + 13))
        tasks.insert(9 * fmt + 4, dict(plane=plane, window=(0, 9, 0, 70), fmt=fmt, step=2 * e, gate_status=(1, -1, 0)))       # plain, its third gate not done
    referenced = sum(1 for t in tasks if t.get("ref") is not None)
    assert referenced == 84 and len(tasks) - referenced == 10
    live = pkg.live_resources()
    outs = gpu_ctx.debug_deliver_ref([_hook(t) for t in tasks])
    assert pkg.live_resources() == live
    assert gpu_ctx.deliver_stats() == (len(tasks), sum(1 for t in tasks if "step" in t))
    for i, (t, got) in enumerate(zip(tasks, outs)):
        assert np.array_equal(got, _host(pkg, t, got.size)), (i, _shown(t))
    gated = [(t, o) for t, o in zip(tasks, outs) if t.get("frame") == 1]
    assert len(gated) == 3
    for t, got in gated:                                       # the frame with a plane that is not done: zeros in all three windows, the pattern between
        e = pkg.DELIVER_ELEM[t["fmt"]]
        raw = got[t["offset"]:].reshape(-1)
        cells = raw[:(raw.size // (3 * e)) * 3 * e].reshape(-1, 3 * e)
        assert (cells[:, :e] == 0).all() and (cells[:, e:] == pkg.DELIVER_PATTERN).all()
    sound = _hook(tasks[0])
    for bad in (dict(ref=sound["ref"][:8]), dict(ref=sound["ref"][:, :52]), dict(ref_base_offset=16), dict(gate_status=(1, 1))):
        with pytest.raises(ValueError):
            gpu_ctx.debug_deliver_ref([sound, dict(sound, **bad)])
