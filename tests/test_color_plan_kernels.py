"""GPU suite (-m gpu): the cost kernel (serial_engine.hip k_color_cost) against its host walk.  ONE launch carries every
frame of color_plan_inputs.cost_tasks -- all shapes, the four formats, three layouts, odd base offsets -- and all nine
sums of every frame equal the host walk's; the same frames in reverse order exercise the task table; and
``Context.color_plan`` gives a frame with a refused source 0xFF while its neighbours get their modes."""
import numpy as np
import pytest

import color_plan_inputs as ci

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def ctx(pkg, gpu_ctx):
    """A context of this module's own (made after the session's, which initialises torch first)."""
    c = pkg.Context(device=0, n_slots=3, n_coders=3)
    yield c
    c.close()


def _tasks(pkg):
    """The tasks and the host walk's sums, made once."""
    if "tasks" not in _cache:
        tasks = ci.cost_tasks(pkg)
        want = np.stack([pkg.color_cost_host(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"]) for t in tasks])
        _cache["tasks"] = (tasks, want)
    return _cache["tasks"]


def test_one_launch_of_mixed_frames_equals_the_host_walk(ctx, pkg):
    tasks, want = _tasks(pkg)
    before = ctx.color_plan_stats()
    got = ctx.debug_color_cost(tasks)
    after = ctx.color_plan_stats()
    assert after[0] == before[0] + 1 and after[1] - before[1] == sum(3 * t["rows"] * t["cols"] for t in tasks)
    assert got.shape == want.shape
    for k, t in enumerate(tasks):
        assert np.array_equal(got[k], want[k]), (k, t["rows"], t["cols"], t["fmt"], t["layout"], got[k], want[k])


def test_the_frames_in_reverse_order(ctx, pkg):
    tasks, want = _tasks(pkg)
    got = ctx.debug_color_cost(tasks[::-1])
    assert np.array_equal(got, want[::-1])
    assert np.array_equal(ctx.debug_color_cost(tasks[5:6]), want[5:6])          # and one frame alone


def test_debug_hook_refusals(ctx, pkg):
    tasks, _ = _tasks(pkg)
    t = dict(tasks[3])
    for kw in (dict(rows=0), dict(fmt=4), dict(steps=[0, 1, 1]), dict(base_offsets=[256, 0, 0]), dict(cols=t["cols"] + 1), dict(scale=float("inf"))):
        with pytest.raises(ValueError):
            ctx.debug_color_cost([tasks[0], dict(t, **kw)])


def test_plan_marks_a_refused_frame_and_plans_its_neighbours(ctx, pkg):
    import torch
    h, w = 48, 80
    frames = ci.class_frames(h, w)
    want_costs = np.stack([pkg.color_cost_numpy(*fr) for fr in frames])
    want = [pkg.color_choose(c) for c in want_costs]
    src = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 2, 3, 1))).cuda()      # NHWC: step 3
    views = [src[n, :, :, c] for n in range(4) for c in range(3)]
    modes, costs = ctx.color_plan(views, costs=True)
    assert modes.dtype == np.uint8 and modes.tolist() == want and np.array_equal(costs, want_costs)
    ci.check_class_modes(pkg, modes)
    assert ctx.color_plan(src.permute(0, 3, 1, 2)).tolist() == want
    for what in ("a host pointer", "unequal sizes"):
        v = list(views)
        v[4] = torch.from_numpy(np.ascontiguousarray(frames[1, 1])) if what == "a host pointer" else src[1, :h - 1, :, 1]
        modes, costs = ctx.color_plan(v, costs=True)
        assert modes.tolist() == [want[0], pkg.COLOR_REFUSED, want[2], want[3]], what
        assert not costs[1].any() and np.array_equal(costs[[0, 2, 3]], want_costs[[0, 2, 3]]), what
    # float16 channels-last with a scale: the costs are those of the collected planes
    f16 = torch.from_numpy((frames.astype(np.float32) / 255.0).astype(np.float16)).cuda().contiguous(memory_format=torch.channels_last)
    modes, costs = ctx.color_plan(f16, scale=255.0, costs=True)
    assert modes.tolist() == want and np.array_equal(costs, want_costs)
    # the whole call
    for bad in (lambda: ctx.color_plan(views[:8]), lambda: ctx.color_plan(views, scale=float("nan")), lambda: ctx.color_plan(views, scale=2.0)):
        with pytest.raises(ValueError):
            bad()
    srcs, fmt = pkg._srcs_of(views, None, None)
    arr = (pkg.Src * 12)(*[pkg.Src(*[int(x) if i else (int(x) or None) for i, x in enumerate(s)]) for s in srcs])
    out = np.full(4, 7, np.uint8)
    ptr = out.ctypes.data_as(pkg.C.POINTER(pkg.C.c_ubyte))
    launches = ctx.color_plan_stats()[0]
    assert ctx.lib.nblic_amd_color_plan(ctx.handle, 11, arr, fmt, 1.0, 0.0, ptr, None) == -1
    assert ctx.lib.nblic_amd_color_plan(ctx.handle, 12, arr, 4, 1.0, 0.0, ptr, None) == -1
    assert ctx.lib.nblic_amd_color_plan(ctx.handle, 12, arr, fmt | pkg.FORMAT_RCT, 1.0, 0.0, ptr, None) == -1
    assert ctx.lib.nblic_amd_color_plan(ctx.handle, 12, None, fmt, 1.0, 0.0, ptr, None) == -1
    assert out.tolist() == [7] * 4 and ctx.color_plan_stats()[0] == launches
