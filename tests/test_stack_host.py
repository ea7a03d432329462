"""CPU suite: slice stacks on the host.  ``stack_forward`` / ``stack_inverse`` on every pair of bytes and on a run whose sums
wrap, and on stack_inputs' four mode patterns at its five depths; the run delivery's host walk (csrc/stack.h stack_deliver_host) against a numpy restatement -- the four formats,
contiguous and strided destinations, aligned and not, row and column windows, skipped slices, a gate that is not done in
the middle of a run; the cost walk (stack_cost_host) against the numpy restatement of the plane cost on every shape, format
and layout; the rule, its equality case and the classes' modes; and every invalid byte."""
import numpy as np
import pytest

import stack_inputs as si
from test_deliver_strided_host import PATTERN


def _host(pkg, task, **kw):
    t = {k: v for k, v in task.items() if k != "base_offsets"}
    return pkg.stack_deliver_host(t.pop("planes"), t.pop("window"), t.pop("fmt"), **t, **kw)


def test_forward_and_inverse_on_every_byte_pair_and_a_run_that_wraps(pkg):
    pair, nine = si.wrap_run()
    t = pkg.stack_forward(pair, [0, 1])
    assert np.array_equal(t[0], pair[0]) and np.array_equal(t[1].astype(np.int64), (pair[1].astype(np.int64) - pair[0] + 128) % 256)
    back = pkg.stack_inverse(t, [0, 1])
    assert all(np.array_equal(a, b) for a, b in zip(back, pair))
    assert len(np.unique(t[1])) == 256                         # every difference occurs
    for modes in ([0] + [1] * 8, [0, 1, 1, 0, 1, 1, 1, 0, 1], [0] * 9):
        planes = pkg.stack_forward(nine, modes)
        for d, m in enumerate(modes):
            want = nine[d] if m == 0 else ((nine[d].astype(np.int64) - nine[d - 1] + 128) % 256).astype(np.uint8)
            assert np.array_equal(planes[d], want), (modes, d)
        assert all(np.array_equal(a, b) for a, b in zip(pkg.stack_inverse(planes, modes), nine)), modes
    # the running sum of the all-delta run leaves 0 .. 255 more than once: it wraps
    total = np.cumsum([p.astype(np.int64) - 128 for p in pkg.stack_forward(nine, [0] + [1] * 8)[1:]], axis=0) + nine[0]
    assert total.max() > 255 and total.min() < 0
    # the host walk restores the same run, the word arithmetic's edge cases among its bytes
    got = pkg.stack_deliver_host(pkg.stack_forward(nine, [0] + [1] * 8), (0, 16, 0, 48), 0)
    assert all(np.array_equal(g.reshape(16, 48), x) for g, x in zip(got, nine))
    got = pkg.stack_deliver_host(t, (0, 256, 0, 256), 0)
    assert np.array_equal(got[1].reshape(256, 256), pair[1])


@pytest.mark.parametrize("pattern", si.PATTERNS)
@pytest.mark.parametrize("depth", si.DEPTHS)
def test_every_pattern_and_depth_forward_inverse_and_run_by_run(pkg, pattern, depth):
    """stack_inputs' four mode patterns at its five depths: the forward planes, their inverse, and every run -- a lone key
    slice behind a run among them -- through the host walk, which gives the slices back."""
    modes = si.modes_of(pattern, depth)
    runs = si.runs_of(modes)
    assert modes[0] == 0 and sum(n for _, n in runs) == depth and all(modes[d] == 0 and all(modes[d + 1:d + n]) for d, n in runs)
    if pattern == "a key last" and depth > 1:
        assert runs[-1] == (depth - 1, 1)
    slices = si.random_stack(np.random.default_rng(35 + depth), depth, 7, 19)
    planes = pkg.stack_forward(slices, modes)
    for d, m in enumerate(modes):
        want = slices[d] if m == 0 else ((slices[d].astype(np.int64) - slices[d - 1] + 128) % 256).astype(np.uint8)
        assert np.array_equal(planes[d], want), d
    assert all(np.array_equal(a, b) for a, b in zip(pkg.stack_inverse(planes, modes), slices))
    for d, n in runs:
        got = pkg.stack_deliver_host(planes[d:d + n], (0, 7, 0, 19), 0)
        assert all(np.array_equal(g.reshape(7, 19), x) for g, x in zip(got, slices[d:d + n])), (d, n)
        assert all(np.array_equal(a, b) for a, b in zip(si.restore_bytewise(planes[d:d + n]), slices[d:d + n]))


def test_the_host_walk_matches_a_numpy_restatement(pkg):
    tasks = si.deliver_tasks(pkg)
    assert len(tasks) == 3 * 4 * len(si.SHAPES)
    for k, task in enumerate(tasks):
        info = {}
        got, want = _host(pkg, task, info=info), si.expected_run(task)
        r0, r1, c0, c1 = task["window"]
        assert info["units"] == (r1 - r0) * ((c1 - c0 + 15) // 16) and info["chunks"] == (info["units"] + 1023) // 1024, k
        for d, (g, w) in enumerate(zip(got, want)):
            assert (g is None) == (w is None), (k, d)
            assert g is None or np.array_equal(g, w), (k, d, task["fmt"], task["window"])


def test_a_gate_in_the_middle_zeros_that_slice_and_the_later_ones(pkg):
    rng = np.random.default_rng(30)
    slices = si.random_stack(rng, 5, 9, 21)
    planes = pkg.stack_forward(slices, [0, 1, 1, 1, 1])
    for bad, how in ((2, "gate"), (0, "gate"), (4, "zeros"), (3, "zeros")):
        kw = dict(gate_status=[1 if d != bad else 3 for d in range(5)]) if how == "gate" else dict(zeros=[d == bad for d in range(5)])
        got = pkg.stack_deliver_host(planes, (0, 9, 0, 21), 0, offsets=3, **kw)
        for d in range(5):
            assert np.array_equal(got[d][3:].reshape(9, 21), slices[d] if d < bad else np.zeros((9, 21), np.uint8)), (bad, how, d)
            assert (got[d][:3] == PATTERN).all()
    # a skipped slice still carries the sum; a bad skipped slice still zeros what follows
    got = pkg.stack_deliver_host(planes, (0, 9, 0, 21), 0, skip=[True, True, False, True, False])
    assert got[0] is None and got[1] is None and np.array_equal(got[2].reshape(9, 21), slices[2]) and np.array_equal(got[4].reshape(9, 21), slices[4])
    got = pkg.stack_deliver_host(planes, (0, 9, 0, 21), 0, skip=[True, True, False, True, False], gate_status=[1, 1, 1, 0, 1])
    assert np.array_equal(got[2].reshape(9, 21), slices[2]) and not got[4].any()


def test_the_host_walk_refuses(pkg):
    planes = pkg.stack_forward(si.random_stack(np.random.default_rng(31), 3, 8, 20), [0, 1, 1])
    ok = dict(planes=planes, window=(0, 8, 0, 20), fmt=1)
    assert len(_host(pkg, ok)) == 3
    for bad in (dict(window=(0, 9, 0, 20)), dict(window=(0, 8, 0, 21)), dict(window=(4, 4, 0, 20)), dict(window=(0, 8, 5, 5)), dict(window=(-1, 8, 0, 20)),
                dict(fmt=4), dict(steps=3), dict(steps=1), dict(offsets=1), dict(pitches=[40, 38, 40]), dict(out_bytes=[320, 319, 320]),
                dict(scales=[1.0, float("nan"), 1.0]), dict(biases=float("inf")), dict(fmt=0, scales=[1.0, 2.0, 1.0]), dict(steps=(1 << 20) + 2)):
        with pytest.raises(ValueError):
            _host(pkg, dict(ok, **bad))


def test_the_cost_walk_matches_the_numpy_restatement(pkg):
    tasks = si.cost_tasks(pkg)
    assert len(tasks) == 4 * len(si.SHAPES) * len(si.COST_LAYOUTS) and {len(t["raws"]) for t in tasks} == set(si.DEPTHS)
    for k, t in enumerate(tasks):
        info = {}
        got = pkg.stack_cost_host(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"], info=info)
        assert np.array_equal(got, pkg.stack_cost_numpy(t["slices"])), (k, t["fmt"], t["rows"], t["cols"], t["layout"])
        assert info["tiles"] == ((t["rows"] + 63) // 64) * ((t["cols"] + 63) // 64)
        assert got[0, 1] == 0 and (got[:, 0] >= t["rows"] * t["cols"]).all()
    t = tasks[5]
    with pytest.raises(ValueError):                            # a byte short
        pkg.stack_cost_host(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"], caps=[r.size - (d == len(t["raws"]) - 1) for d, r in enumerate(t["raws"])])
    with pytest.raises(ValueError):
        pkg.stack_cost_host(t["raws"], t["rows"], t["cols"], 4)


def test_the_cost_walk_on_every_shape_format_and_layout_of_the_collect_grid(pkg):
    tasks = si.grid_cost_tasks(pkg)
    assert len(tasks) == 15 * (16 + 8 + 8 + 4)                 # widths x heights x residues of each format
    for k, t in enumerate(tasks):
        got = pkg.stack_cost_host(t["raws"], t["rows"], t["cols"], t["fmt"], t["pitches"], t["steps"], t["scale"], t["bias"], offsets=t["offsets"])
        assert np.array_equal(got, pkg.stack_cost_numpy(t["slices"])), (k, t["fmt"], t["rows"], t["cols"], t["offsets"][0])


def test_the_rule_its_equality_case_and_key_every(pkg):
    assert pkg.stack_choose(64, 62) == 1 and pkg.stack_choose(64, 63) == 0 and pkg.stack_choose(64, 64) == 0
    assert pkg.stack_choose(6400, 6299) == 1 and pkg.stack_choose(6400, 6300) == 0 and pkg.stack_choose(0, 0) == 0
    assert pkg.stack_choose(2 ** 63, 2 ** 63 - 2 ** 57 - 1) == 1 and pkg.stack_choose(2 ** 63, 2 ** 63 - 2 ** 57) == 0        # no overflow in the products
    rng = np.random.default_rng(32)
    for _ in range(200):
        a, b = (int(v) for v in rng.integers(0, 1 << 40, 2))
        assert pkg.stack_choose(a, b) == int(64 * b < 63 * a)
    # key_every: slice 0 and every K-th slice are keys whatever the costs say; the others follow the rule
    costs = np.array([[100, 0]] + [[100, 10], [100, 99]] * 7, np.uint64)[:14]      # two stacks of seven: deltas win on odd places
    rule = [pkg.stack_choose(int(i), int(d)) for i, d in costs]
    for K in (0, 1, 2, 3, 7, 8):
        want = [0 if k % 7 == 0 or (K and (k % 7) % K == 0) else rule[k] for k in range(14)]
        assert pkg.stack_modes_from_costs(costs, 7, K).tolist() == want, K
    with pytest.raises(ValueError):
        pkg.stack_modes_from_costs(costs, 7, -1)
    with pytest.raises(ValueError):
        pkg.stack_modes_from_costs(costs, 5)


def test_the_classes_modes(pkg):
    stacks = si.class_stacks(96, 80)
    for name, stack, want in zip(si.CLASSES, stacks, si.class_modes()):
        costs = pkg.stack_cost_numpy(list(stack))
        modes = pkg.stack_modes_from_costs(costs, len(stack)).tolist()
        assert modes == want, (name, (costs[:, 1] / costs[:, 0]).round(3).tolist())


def test_every_invalid_byte_is_refused(pkg):
    lib = pkg.load_library()
    assert [m for m in range(256) if pkg.stack_mode_valid(m)] == [0, 1]
    assert not pkg.stack_mode_valid(-1) and not pkg.stack_mode_valid(256)
    valid = lambda n, depth, modes: bool(lib.nblic_amd_stack_modes_valid(n, depth, pkg._modes_ptr(np.array(modes, np.uint8))))
    assert valid(6, 3, [0, 1, 1, 0, 0, 1]) and valid(6, 6, [0, 1, 1, 0, 0, 1]) and valid(2, 1, [0, 0]) and valid(0, 4, [0])
    for b in range(2, 256):
        assert not valid(6, 3, [0, 1, b, 0, 0, 1]), b
    assert not valid(6, 3, [0, 1, 1, 1, 0, 1])                   # slice 0 of the second stack is a delta
    assert not valid(6, 4, [0] * 6) and not valid(6, 0, [0] * 6) and not valid(6, -3, [0] * 6) and not valid(2, 1, [0, 1])
    x = np.zeros((4, 4), np.uint8)
    for bad in ([1, 0], [0, 2], [0, 0xFF], [0]):
        with pytest.raises(ValueError):
            pkg.stack_forward([x, x], bad)
        with pytest.raises(ValueError):
            pkg.stack_inverse([x, x], bad)
