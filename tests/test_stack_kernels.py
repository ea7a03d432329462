"""GPU suite (-m gpu): the two stack kernels against their host walks (csrc/stack.h), byte for byte.  k_deliver_stack over
the host test's runs -- every shape and format, contiguous destinations that get 16-byte stores and ones that do not,
strided ones, windows, skipped slices, gates that are not done -- in ONE launch, the bytes around every destination intact;
k_stack_cost over every shape, format, layout and depth in ONE launch, the sources at odd offsets in regions of 0xFF."""
import numpy as np
import pytest

import stack_inputs as si
from test_deliver_strided_host import PATTERN
from test_stack_host import _host

pytestmark = pytest.mark.gpu


def test_one_launch_delivers_every_run_as_the_host_walk_does(gpu_ctx, pkg):
    pair, nine = si.wrap_run()                                  # every pair of bytes, and a run whose sums wrap: the word arithmetic on the device
    tasks = si.deliver_tasks(pkg) + [dict(planes=pkg.stack_forward(pair, [0, 1]), window=(0, 256, 0, 256), fmt=0, base_offsets=[0, 5]),
                                     dict(planes=pkg.stack_forward(nine, [0] + [1] * 8), window=(0, 16, 0, 48), fmt=0, offsets=[d % 2 for d in range(9)])]
    # guard bytes behind every destination too: the buffers are longer than the windows need
    for t in tasks:
        d = len(t["planes"])
        r0, r1, c0, c1 = t["window"]
        e = (1, 2, 2, 4)[t["fmt"]]
        steps = t.get("steps", [e] * d)
        pitches = t.get("pitches", [(c1 - c0) * s for s in steps])
        t["out_bytes"] = [o + (r1 - r0 - 1) * p + (c1 - c0 - 1) * s + e + 37 for o, p, s in zip(t["offsets"] if "offsets" in t else [0] * d, pitches, steps)]
    before = gpu_ctx.stack_plan_stats()
    got = gpu_ctx.debug_stack_deliver(tasks)
    after = gpu_ctx.stack_plan_stats()
    assert after["deliver_launches"] == before["deliver_launches"] + 1 and after["runs"] == before["runs"] + len(tasks)
    for k, (task, run) in enumerate(zip(tasks, got)):
        host, want = _host(pkg, task), si.expected_run(task)
        for d, (g, h, w) in enumerate(zip(run, host, want)):
            assert (g is None) == (h is None), (k, d)
            if g is None:
                continue
            assert np.array_equal(g, h), (k, d, task["fmt"], task["window"])
            assert np.array_equal(h, w) and (g[-37:] == PATTERN).all(), (k, d)
    assert np.array_equal(got[-2][1][:65536].reshape(256, 256), pair[1])
    assert all(np.array_equal(g[d % 2:d % 2 + 768].reshape(16, 48), x) for d, (g, x) in enumerate(zip(got[-1], nine)))


def test_runs_of_different_sizes_and_depths_in_one_launch(gpu_ctx, pkg):
    """More than one chunk in a task (129 x 129 rows of nine units), a run of nine beside runs of two, a run of one."""
    rng = np.random.default_rng(33)
    tasks = []
    for h, w, depth, fmt in ((129, 129, 9, 0), (3, 5, 2, 3), (200, 160, 3, 1), (1, 1, 1, 2), (33, 17, 5, 0)):
        slices = si.random_stack(rng, depth, h, w)
        tasks.append(dict(planes=pkg.stack_forward(slices, [0] + [1] * (depth - 1)), window=(0, h, 0, w), fmt=fmt, slices=slices,
                          scales=1.0 if fmt == 0 else 0.5, biases=0.0 if fmt == 0 else -3.0, base_offsets=[(5 * d) % 16 for d in range(depth)]))
    got = gpu_ctx.debug_stack_deliver([{k: v for k, v in t.items() if k != "slices"} for t in tasks])
    for k, (task, run) in enumerate(zip(tasks, got)):
        want = si.expected_run({k_: v for k_, v in task.items() if k_ != "slices"})
        for d, (g, w) in enumerate(zip(run, want)):
            assert np.array_equal(g, w), (k, d)
        if task["fmt"] == 0:
            h, w = task["slices"][0].shape
            assert all(np.array_equal(g.reshape(h, w), x) for g, x in zip(run, task["slices"])), k


def test_the_kernel_refuses_what_the_host_walk_refuses(gpu_ctx, pkg):
    planes = pkg.stack_forward(si.random_stack(np.random.default_rng(34), 3, 8, 20), [0, 1, 1])
    ok = dict(planes=planes, window=(0, 8, 0, 20), fmt=1)
    assert len(gpu_ctx.debug_stack_deliver([ok])[0]) == 3
    for bad in (dict(window=(0, 9, 0, 20)), dict(window=(0, 8, 0, 21)), dict(fmt=4), dict(steps=3), dict(offsets=1), dict(pitches=[40, 38, 40]),
                dict(out_bytes=[320, 319, 320]), dict(scales=[1.0, float("nan"), 1.0]), dict(fmt=0, scales=2.0), dict(base_offsets=16)):
        with pytest.raises(ValueError):
            gpu_ctx.debug_stack_deliver([ok, dict(ok, **bad)])


def test_one_launch_costs_every_stack_as_the_host_walk_does(gpu_ctx, pkg):
    tasks = si.cost_tasks(pkg)
    before = gpu_ctx.stack_plan_stats()
    got = gpu_ctx.debug_stack_cost(tasks)
    after = gpu_ctx.stack_plan_stats()
    assert after["cost_launches"] == before["cost_launches"] + 1
    assert after["elements"] == before["elements"] + sum(len(t["raws"]) * t["rows"] * t["cols"] for t in tasks)
    for k, (t, g) in enumerate(zip(tasks, got)):
        host = pkg.stack_cost_host(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"])
        assert np.array_equal(g, host), (k, t["fmt"], t["rows"], t["cols"], t["layout"], g.tolist(), host.tolist())
        assert np.array_equal(g, pkg.stack_cost_numpy(t["slices"])), k
    # the collect grid: four layouts of one shape as the four slices of a stack, the transposed one among them
    grid = si.grid_cost_tasks(pkg)
    got = gpu_ctx.debug_stack_cost([dict(g, raws=[r[o:] for r, o in zip(g["raws"], g["offsets"])], base_offsets=g["offsets"]) for g in grid])      # (the same residue modulo 16 on the device)
    for k, (g, c) in enumerate(zip(grid, got)):
        assert np.array_equal(c, pkg.stack_cost_numpy(g["slices"])), (k, g["fmt"], g["rows"], g["cols"])
    t = tasks[7]
    with pytest.raises(ValueError):                            # a source a byte short of its extent
        gpu_ctx.debug_stack_cost([dict(t, raws=[r[:-1] if d == 0 else r for d, r in enumerate(t["raws"])])])
    with pytest.raises(ValueError):
        gpu_ctx.debug_stack_cost([dict(t, base_offsets=[256] * len(t["raws"]))])
