"""Stacks for the slice-stack tests (tests/test_stack_host.py on the CPU, tests/test_stack_kernels.py and
tests/test_stack_codec.py on the GPU): the shapes, depths and mode patterns at which the run walk and the tile walk can go
wrong, runs as the dicts that ``Context.debug_stack_deliver`` takes, cost tasks as ``Context.debug_stack_cost`` takes them,
and the four constructed classes of stacks whose modes the rule must find."""
import numpy as np

import inputs
from collect_inputs import ELEM, NORMS, as_values, element_bits, lay_out
from color_plan_inputs import mix
from test_deliver_strided_host import NORMS as DELIVER_NORMS, PATTERN, scatter

# a pixel, one row, one column, a few of each, no multiple of sixteen; one cost tile exactly; a row and a column more; two
# tiles each way plus one
SHAPES = ((1, 1), (1, 17), (17, 1), (3, 5), (33, 17), (64, 64), (65, 65), (129, 129), (65, 130), (130, 65))   # (the last two: 2 x 3 and 3 x 2 tiles)
DEPTHS = (1, 2, 3, 5, 9)
PATTERNS = ("all keys", "all deltas", "a key in the middle", "a key last")


def modes_of(pattern, depth):
    """The mode bytes of one stack of ``depth`` slices."""
    m = [0] + [1] * (depth - 1)
    if pattern == "all keys":
        m = [0] * depth
    elif pattern == "a key in the middle" and depth > 2:
        m[depth // 2] = 0
    elif pattern == "a key last" and depth > 1:
        m[-1] = 0
    return m


def runs_of(modes):
    """[(first slice, length)] of the runs of one stack."""
    out = []
    for d, m in enumerate(modes):
        if m == 0:
            out.append([d, 1])
        else:
            out[-1][1] += 1
    return [tuple(r) for r in out]


def random_stack(rng, depth, h, w):
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(depth)]


def restore_bytewise(planes):
    """A byte-by-byte restatement of a run's restoring in wide integers: [x_0, x_1, ...] from [x_0, t_1, ...]."""
    out = [planes[0].astype(np.int64)]
    for t in planes[1:]:
        out.append((t.astype(np.int64) + out[-1] - 128) % 256)
    return [x.astype(np.uint8) for x in out]


def expected_run(task):
    """What every slice's buffer of a run task holds afterwards, by numpy: the restored window scattered into a buffer of the
    pattern; zeros from the first slice on whose plane does not count; None for a skipped slice."""
    planes = restore_bytewise(task["planes"])
    d = len(planes)
    per = lambda key, default: list(task[key]) if hasattr(task.get(key, default), "__len__") else [task.get(key, default)] * d
    fmt = task["fmt"]
    r0, r1, c0, c1 = task["window"]
    steps = per("steps", ELEM[fmt])
    pitches = task["pitches"] if "pitches" in task else [(c1 - c0) * s for s in steps]
    offsets, skip, zeros, gates = per("offsets", 0), per("skip", False), per("zeros", False), per("gate_status", -1)
    scales, biases = per("scales", 1.0), per("biases", 0.0)
    out, ok = [], True
    for k in range(d):
        ok = ok and not zeros[k] and gates[k] in (-1, 1)
        if skip[k]:
            out.append(None)
            continue
        size = task["out_bytes"][k] if "out_bytes" in task else offsets[k] + (r1 - r0 - 1) * pitches[k] + (c1 - c0 - 1) * steps[k] + ELEM[fmt]
        buf = np.full(size, PATTERN, np.uint8)
        out.append(scatter(buf, planes[k], (r0, r1, c0, c1), fmt, scales[k], biases[k], pitches[k], steps[k], offsets[k], zero=not ok))
    return out


def deliver_tasks(pkg, seed=27):
    """Runs for the delivery kernel and its host walk: every shape whole in every format with contiguous destinations
    (aligned and not: the offsets), strided ones, row and column windows, skipped slices, and a gate that is not done in
    the middle of a run.  The planes are those of ``stack_forward`` of random slices, whose sums wrap."""
    rng = np.random.default_rng(seed)
    tasks, k = [], 0
    for h, w in SHAPES:
        for fmt in range(4):
            depth = DEPTHS[1 + k % 4]
            planes = pkg.stack_forward(random_stack(rng, depth, h, w), [0] + [1] * (depth - 1))
            e = ELEM[fmt]
            scales = [1.0 if fmt == 0 else DELIVER_NORMS[(k + d) % 3][0] for d in range(depth)]
            biases = [0.0 if fmt == 0 else DELIVER_NORMS[(k + d) % 3][1] for d in range(depth)]
            base = dict(planes=planes, fmt=fmt, scales=scales, biases=biases, base_offsets=[(k + 3 * d) % 16 for d in range(depth)])
            # whole, contiguous: slice d starts d elements into its buffer, so some slices get 16-byte stores and some do not
            tasks.append(dict(base, window=(0, h, 0, w), offsets=[(d % 3) * 16 * e + ((d // 3) % 2) * e for d in range(depth)]))
            # a window of rows and columns, strided (the colours of an interleaved frame), a skipped slice
            r0, r1, c0, c1 = h // 3, h - h // 4, w // 5, w - w // 6
            tasks.append(dict(base, window=(r0, r1, c0, c1), steps=[(2 + d % 2) * e for d in range(depth)], skip=[d == 1 for d in range(depth)],
                              pitches=[((c1 - c0) * (2 + d % 2) + d) * e for d in range(depth)], offsets=[d * e for d in range(depth)]))
            # a gate in the middle that is not done (2: failed), a plane known to be bad at the end
            gates = [1 if d % 2 else -1 for d in range(depth)]
            gates[depth // 2] = 2
            tasks.append(dict(base, window=(0, h, 0, w), gate_status=gates, pitches=[(w + d) * e for d in range(depth)]))
            k += 1
    return tasks


def wrap_run():
    """A run of 9 slices of 0 / 255 / random bytes whose sums wrap several times, and a pair of slices that holds all
    256 x 256 pairs of bytes."""
    rng = np.random.default_rng(28)
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    nine = [np.zeros((16, 48), np.uint8), np.full((16, 48), 255, np.uint8)] + [rng.integers(0, 256, (16, 48), dtype=np.uint8) for _ in range(3)] + \
           [np.full((16, 48), 255, np.uint8), np.zeros((16, 48), np.uint8), np.full((16, 48), 128, np.uint8), np.full((16, 48), 255, np.uint8)]
    return [a.copy(), b.copy()], nine


COST_LAYOUTS = ("contiguous", "interleaved", "pitched")


def cost_tasks(pkg, seed=29):
    """Every shape in every format and layout with a depth from DEPTHS, a scale and bias from collect_inputs.NORMS, at odd
    base offsets.  Each task carries ``slices``: the collected uint8 planes by ``collect_numpy``."""
    rng = np.random.default_rng(seed)
    tasks, k = [], 0
    for fmt in range(4):
        e = ELEM[fmt]
        for rows, cols in SHAPES:
            for layout in COST_LAYOUTS:
                depth = DEPTHS[k % len(DEPTHS)] if rows * cols < 4096 else DEPTHS[k % 3]
                scale, bias = NORMS[0] if fmt == 0 else NORMS[k % 3]
                raws, pitches, steps, slices = [], [], [], []
                for d in range(depth):
                    bits = element_bits(rng, fmt, (rows, cols))
                    if d and d % 2 == 0 and fmt == 0:           # a slice close to the one before: small differences
                        bits = (slices[-1].astype(np.int16) + rng.integers(-2, 3, (rows, cols))).clip(0, 255).astype(np.uint8)
                    if layout == "contiguous":
                        pitch, step = cols * e, e
                    elif layout == "interleaved":
                        pitch, step = cols * 3 * e, 3 * e
                    else:
                        pitch, step = (cols + 1 + (k + d) % 3) * e, e
                    raws.append(lay_out(bits, fmt, pitch, step, 0)); pitches.append(pitch); steps.append(step)
                    slices.append(pkg.collect_numpy(as_values(bits, fmt), fmt, scale, bias))
                tasks.append(dict(raws=raws, pitches=pitches, steps=steps, rows=rows, cols=cols, fmt=fmt, scale=scale, bias=bias,
                                  base_offsets=[((2 * k + 1 + 2 * d) * e) % 256 for d in range(depth)], layout=layout, slices=slices))
                k += 1
    return tasks


def grid_cost_tasks(pkg):
    """collect_inputs.grid as stacks: for every format, width, height and residue, the grid's four layouts of that shape
    (three steps with slack in the pitch, and transposed) are the four slices of one stack -- another pitch and step in
    every slice -- under the first one's scale and bias, each source ``residue`` bytes into its buffer."""
    from collect_inputs import grid
    tasks = []
    for fmt in range(4):
        group = []
        for g in grid(fmt):
            group.append(g)
            if len(group) < 4:
                continue
            scale, bias = group[0]["scale"], group[0]["bias"]
            assert len({(x["rows"], x["cols"], x["residue"]) for x in group}) == 1 and [x["layout"] for x in group] == [0, 1, 2, 3]
            tasks.append(dict(raws=[x["raw"] for x in group], pitches=[x["pitch"] for x in group], steps=[x["step"] for x in group], rows=group[0]["rows"],
                              cols=group[0]["cols"], fmt=fmt, scale=scale, bias=bias, offsets=[x["residue"] for x in group], layout="grid",
                              slices=[pkg.collect_numpy(as_values(x["bits"], fmt), fmt, scale, bias) for x in group]))
            group = []
    return tasks


CLASSES = ("static", "independent", "cut", "equal")


def class_stacks(h, w, depth=6, seed=60):
    """[4, depth, h, w] uint8, one stack per class of CLASSES: slices that share a SYN-1 plane (7 parts in 8, the eighth a
    plane of the slice's own seed); planes of independent seeds; the static class with a scene cut at slice 3 (another
    shared plane from there on); equal slices."""
    s = lambda k: inputs.syn1(h, w, seed + k)
    static = np.stack([mix(s(0), s(1 + d)) for d in range(depth)])
    independent = np.stack([s(20 + d) for d in range(depth)])
    cut = np.stack([mix(s(0) if d < 3 else s(40), s(41 + d)) for d in range(depth)])
    equal = np.stack([s(50)] * depth)
    return np.stack([static, independent, cut, equal])


def class_modes(depth=6):
    """What the rule must make of class_stacks: every slice a delta; every slice a key; a key at slice 3 only; every slice
    a delta."""
    deltas = [0] + [1] * (depth - 1)
    cut = list(deltas)
    cut[3] = 0
    return [deltas, [0] * depth, cut, deltas]
