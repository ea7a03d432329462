"""GPU suite (-m gpu): the three deep kernels alone -- k_collect_deep, k_deliver_deep and k_deep_cost, each in ONE launch over
the tasks of tests/test_deep_host.py (one of them larger than a chunk), byte for byte against the host walk of the same task
(csrc/deep.h, which the CPU suite holds against numpy), guard bytes intact, and the context's counts up by exactly one launch."""
import numpy as np
import pytest

import deep_inputs as di
from test_deep_host import host_collect, host_cost, host_deliver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first)."""
    c = pkg.Context(device=0, n_slots=2, n_coders=2)
    yield c
    c.close()


def test_collect_kernel_is_the_host_walk(ctx, pkg):
    tasks = di.collect_tasks()
    before = ctx.deep_plan_stats()
    outs = ctx.debug_deep_collect(tasks)
    after = ctx.deep_plan_stats()
    assert after["collect_launches"] == before["collect_launches"] + 1 and after["plan_launches"] == before["plan_launches"]
    chunks = 0
    for t, buf in zip(tasks, outs):
        info = {}
        want = host_collect(pkg, t, info)
        chunks = max(chunks, info["chunks"])
        n = t["rows"] * t["cols"]
        assert np.array_equal(buf[di.GUARD:di.GUARD + n].reshape(t["rows"], t["cols"]), want), (t["rows"], t["cols"], t["fmt"], t["part"], t["step"])
        assert np.array_equal(want, di.expected_plane(t))
        assert (buf[:di.GUARD] == di.PATTERN).all() and (buf[di.GUARD + n:] == di.PATTERN).all()
    assert chunks > 1                                          # one task is larger than a chunk


def test_deliver_kernel_is_the_host_walk(ctx, pkg):
    tasks = di.deliver_tasks()
    before = ctx.deep_plan_stats()
    outs = ctx.debug_deep_deliver(tasks)
    after = ctx.deep_plan_stats()
    assert after["deliver_launches"] == before["deliver_launches"] + 1
    chunks = 0
    for t, buf in zip(tasks, outs):
        info = {}
        want = host_deliver(pkg, t, info)
        chunks = max(chunks, info["chunks"])
        assert np.array_equal(buf, want), (t["window"], t["fmt"], t["mode"], t.get("step"), t.get("gate_status"))
        assert np.array_equal(want, di.expected_buffer(t))     # (guard bytes in front of, between and behind the rows included)
    assert chunks > 1


def test_cost_kernel_is_the_host_walk(ctx, pkg):
    tasks = di.cost_tasks()
    before = ctx.deep_plan_stats()
    sums = ctx.debug_deep_cost(tasks)
    after = ctx.deep_plan_stats()
    assert after["plan_launches"] == before["plan_launches"] + 1 and after["images"] == before["images"] + len(tasks)
    tiles = 0
    for t, got in zip(tasks, sums):
        info = {}
        assert np.array_equal(got, host_cost(pkg, t, info)), (t["rows"], t["cols"], t["fmt"], t["step"])
        tiles = max(tiles, info["tiles"])
    assert tiles > 1


def test_kernel_hooks_refuse(ctx):
    t = di.cost_tasks()[0]
    for bad in (dict(fmt=2), dict(step=3), dict(pitch=1), dict(base_offset=256), dict(rows=0)):
        with pytest.raises(ValueError):
            ctx.debug_deep_cost([{**t, **bad}])
        with pytest.raises(ValueError):
            ctx.debug_deep_collect([{**t, "part": 0, **bad}])
    with pytest.raises(ValueError):
        ctx.debug_deep_collect([{**t, "part": 3}])
    d = di.deliver_tasks()[0]
    for bad in (dict(mode=4), dict(fmt=5), dict(fmt=0, mode=2), dict(fmt=1, mode=1), dict(base_offsets=(16, 0)), dict(out_bytes=d["out_bytes"] - 25)):
        with pytest.raises(ValueError):
            ctx.debug_deep_deliver([{**d, **bad}])
