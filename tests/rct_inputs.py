"""Task lists for the colour transform's tests (tests/test_rct_host.py on the CPU, tests/test_rct_kernels.py on the GPU):
collect tasks with a reference source and delivery tasks with a reference plane, at the smallest shapes at which the unit
walks can go wrong, as the dicts that ``Context.debug_collect_ref`` / ``Context.debug_deliver_ref`` take -- plus, per
task, what the numpy reference needs (``bits`` / ``ref_bits``: the elements as bit patterns)."""
import numpy as np

from collect_inputs import ELEM, NORMS, element_bits, lay_out

CHANNEL_NORMS = ((1.0 / 255.0, -0.5), (0.0078125, -1.0), (2.0 / 255.0, 0.25))     # scale / bias of R, G, B in the deliveries


def exhaustive_frame():
    """256 x 256, R[i, j] = i, G[i, j] = j, B[i, j] = 255 - i: every (R, G) and every (B, G) pair once."""
    i, j = np.mgrid[0:256, 0:256]
    return i.astype(np.uint8), j.astype(np.uint8), (255 - i).astype(np.uint8)


def rct_forward_int16(r, g, b):
    """The transform written out in int16 numpy."""
    r, g, b = (np.asarray(v).astype(np.int16) for v in (r, g, b))
    return (((r - g + 128) % 256).astype(np.uint8), g.astype(np.uint8), ((b - g + 128) % 256).astype(np.uint8))


# (rows, cols, px_range or None): a pixel, a row shorter and longer than a unit, rows that end inside units, the
# 16384-pixel chunk crossed (129 x 129 = 16641), and bands that are no multiple of 16 at cols = 33
COLLECT_SHAPES = ((1, 1, None), (1, 17, None), (3, 5, None), (17, 33, None), (129, 129, None), (17, 33, (5 * 33, 12 * 33)), (17, 33, (7 * 33, 0)),
                  (129, 129, (129 * 3, 129 * 128)))


def collect_tasks(seed=25):
    """Referenced collect tasks of all four formats: every shape above with the own source and the reference in DIFFERENT
    layouts (contiguous, stepped, pitched with slack), at different residues; and the exhaustive frame's R and B against G."""
    rng = np.random.default_rng(seed)
    tasks, k = [], 0
    for fmt in range(4):
        e = ELEM[fmt]
        for rows, cols, px in COLLECT_SHAPES:
            for own_step, ref_step in ((1, 1), (3, 1), (1, 4), (2, 3)):
                if rows * cols > 1000 and (own_step, ref_step) in ((3, 1), (2, 3)):       # (the large shapes: two layouts are enough)
                    continue
                bits, ref_bits = element_bits(rng, fmt, (rows, cols)), element_bits(rng, fmt, (rows, cols))
                pitch = ((cols - 1) * own_step + 1 + k % 3) * e
                ref_pitch = ((cols - 1) * ref_step + 1 + (k + 2) % 5) * e
                scale, bias = NORMS[0] if fmt == 0 else NORMS[k % 3]
                t = dict(raw=lay_out(bits, fmt, pitch, own_step * e, 0), ref=lay_out(ref_bits, fmt, ref_pitch, ref_step * e, 0), rows=rows, cols=cols, fmt=fmt,
                         pitch=pitch, step=own_step * e, ref_pitch=ref_pitch, ref_step=ref_step * e, scale=scale, bias=bias,
                         base_offset=(k * e) % 256, ref_base_offset=(7 * k * e) % 256, bits=bits, ref_bits=ref_bits)
                if px:
                    t["px_range"] = px
                tasks.append(t)
                k += 1
    r, g, b = exhaustive_frame()
    for own in (r, b):
        tasks.append(dict(raw=own.copy(), ref=g.copy(), rows=256, cols=256, fmt=0, pitch=256, step=1, ref_pitch=256, ref_step=1, scale=1.0, bias=0.0,
                          base_offset=0, ref_base_offset=4, bits=own, ref_bits=g))
    # the three colours of an interleaved frame: step 3, the reference one byte on
    frame = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for c in (0, 2):
        tasks.append(dict(raw=frame.reshape(-1)[c:].copy(), ref=frame.reshape(-1)[1:].copy(), rows=40, cols=50, fmt=0, pitch=150, step=3, ref_pitch=150, ref_step=3,
                          scale=1.0, bias=0.0, base_offset=c, ref_base_offset=1, bits=frame[:, :, c], ref_bits=frame[:, :, 1]))
    return tasks


def plain_collect_tasks(seed=26):
    """A few tasks without a reference, to mix into a launch."""
    rng = np.random.default_rng(seed)
    tasks = []
    for fmt in range(4):
        e = ELEM[fmt]
        bits = element_bits(rng, fmt, (17, 33))
        scale, bias = NORMS[0] if fmt == 0 else NORMS[1]
        tasks.append(dict(raw=lay_out(bits, fmt, 35 * e, e, 0), ref=None, rows=17, cols=33, fmt=fmt, pitch=35 * e, step=e, scale=scale, bias=bias,
                          base_offset=2 * e, bits=bits))
    return tasks


def deliver_tasks(seed=27):
    """Delivery tasks with a reference, all four formats: contiguous ones whose destination row starts at every kind of
    residue (head and tail units), strided ones, windows with col0 > 0 and a width that is no multiple of 16, a scale and
    bias per channel, the 129 x 129 window of two chunks, the exhaustive frame, and gates of which one is not done."""
    rng = np.random.default_rng(seed)
    small_t, small_g = rng.integers(0, 256, (11, 53), dtype=np.uint8), rng.integers(0, 256, (11, 53), dtype=np.uint8)
    big_t, big_g = rng.integers(0, 256, (131, 140), dtype=np.uint8), rng.integers(0, 256, (131, 140), dtype=np.uint8)
    r, g, b = exhaustive_frame()
    tr, _, tb = rct_forward_int16(r, g, b)
    tasks, k = [], 0
    for fmt in range(4):
        e = ELEM[fmt]
        for window in ((2, 9, 5, 38), (0, 11, 0, 53), (10, 11, 52, 53), (1, 4, 7, 24)):
            for strided in (False, True):
                for gates in ((1, 1, 1), (-1, -1, -1)):
                    cols = window[3] - window[2]
                    scale, bias = (1.0, 0.0) if fmt == 0 else CHANNEL_NORMS[k % 3]
                    offset = (k * e) % 16 if not strided else (k % 3) * e
                    step = 3 * e if strided else e
                    pitch = cols * step + (0, 2 * e)[k % 2]
                    t = dict(plane=small_t, ref=small_g, window=window, fmt=fmt, scale=scale, bias=bias, pitch=pitch, offset=offset, gate_status=gates,
                             base_offset=k % 16, ref_base_offset=(k + 5) % 16)
                    if strided:
                        t["step"] = step
                    need = offset + (window[1] - window[0] - 1) * pitch + (cols - 1) * step + e
                    t["out_bytes"] = need + 19
                    tasks.append(t)
                    k += 1
        scale, bias = (1.0, 0.0) if fmt == 0 else CHANNEL_NORMS[fmt % 3]
        tasks.append(dict(plane=big_t, ref=big_g, window=(1, 130, 3, 132), fmt=fmt, scale=scale, bias=bias, offset=e, gate_status=(1, 1, 1), base_offset=3))
        tasks.append(dict(plane=big_t, ref=big_g, window=(1, 130, 3, 132), fmt=fmt, scale=scale, bias=bias, step=3 * e, offset=2 * e, gate_status=(1, 1, 1)))
        tasks.append(dict(plane=tr, ref=g, window=(0, 256, 0, 256), fmt=fmt, scale=scale, bias=bias, gate_status=(1, 1, 1)))
        tasks.append(dict(plane=tb, ref=g, window=(0, 256, 0, 256), fmt=fmt, scale=scale, bias=bias, step=4 * e, gate_status=(-1, 1, -1)))
    return tasks


def gated_off_frame(fmt=1):
    """A launch of two frames (R, G, B tasks each: the G task has no reference): in the second frame one plane is not done,
    and which one differs from task to task only in what the host walk is told -- every task names all three statuses."""
    rng = np.random.default_rng(28)
    e = ELEM[fmt]
    tasks = []
    for frame, gates in enumerate(((1, 1, 1), (1, 2, 1))):
        planes = [rng.integers(0, 256, (9, 37), dtype=np.uint8) for _ in range(3)]
        for c in range(3):
            tasks.append(dict(plane=planes[c], ref=None if c == 1 else planes[1], window=(1, 8, 2, 35), fmt=fmt, scale=CHANNEL_NORMS[c][0], bias=CHANNEL_NORMS[c][1],
                              step=3 * e, pitch=33 * 3 * e, offset=c * e, gate_status=gates, frame=frame, channel=c))
    return tasks
