"""GPU suite (-m gpu): decode to device memory.  The delivery kernel on caller-made planes (nblic_amd_debug_deliver) against
the host walk and numpy; nblic_amd_decode_batch_indexed_to and nblic_amd_decode_batch_to into torch tensors and views of
them, against the oracle's reconstruction and the numpy expression of the normalisation, bit for bit; images that fail or
are refused; and the host calls on the same inputs, which return what they returned before."""
import numpy as np
import pytest

from test_deliver_host import ELEM, NORMS, PATTERN, expected, layouts, plane_of, values, windows_of
from test_indexed_batch_decode import CASES, GEOMS, _forge, _live, _made

pytestmark = pytest.mark.gpu

DTYPES = ("uint8", "float16", "bfloat16", "float32")


def _torch():
    import torch
    return torch


def _filled(shape, fmt):
    """A device tensor of the format's dtype whose every byte is 0x5A."""
    torch = _torch()
    raw = torch.full((int(np.prod(shape)) * ELEM[fmt],), PATTERN, dtype=torch.uint8, device="cuda")
    return raw.view(getattr(torch, DTYPES[fmt])).reshape(shape)


def _elements(px, fmt, scale, bias):
    """The window in the format's bit pattern, as unsigned integers [rows, cols]."""
    b = values(px, fmt, scale, bias)
    return b if fmt == 0 else b.view(np.uint16 if ELEM[fmt] == 2 else np.uint32)


def _bits(t):
    """A device tensor's elements as unsigned integers of their width."""
    torch = _torch()
    torch.cuda.synchronize()
    e = t.element_size()
    host = t.contiguous().cpu()
    raw = host.view(torch.uint8).numpy().reshape(-1)
    return raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[e]).reshape(tuple(t.shape))


def test_kernel_on_caller_made_planes(gpu_ctx, pkg):
    """Hundreds of tasks of all four formats in ONE launch: planes at every base offset 0 .. 15, destinations at every
    residue the format allows, pitches with slack, narrow and multi-chunk windows, zero flags and gates."""
    tasks = []
    k = 0
    for fmt in range(4):
        e = ELEM[fmt]
        lay = layouts(fmt)
        for w in (1, 15, 16, 17, 131, 149, 150):
            for window in windows_of(w):
                cols, rows = window[3] - window[2], window[1] - window[0]
                if window[0] == 1 and window[2] % 3 and cols not in (1, 17):         # (the CPU grid, thinned: every col0 still occurs)
                    continue
                scale, bias = NORMS[0] if fmt == 0 else NORMS[k % 3]
                slack, offset = lay[k % len(lay)]
                pitch = cols * e + slack
                tasks.append(dict(plane=plane_of(w), window=window, fmt=fmt, scale=scale, bias=bias, pitch=pitch, offset=offset,
                                  out_bytes=offset + (rows - 1) * pitch + cols * e + 21, base_offset=k % 16, zero=False, gate_status=-1))
                k += 1
    big = plane_of(150, 300)
    for fmt in range(4):                                       # more than one chunk, and a plane that ends on a multiple of 256 (no slack behind its last row)
        tasks.append(dict(plane=big, window=(0, 300, 0, 150), fmt=fmt, scale=NORMS[fmt % 3 if fmt else 0][0], bias=NORMS[fmt % 3 if fmt else 0][1],
                          base_offset=5 + fmt, offset=ELEM[fmt]))
        tasks.append(dict(plane=plane_of(16, 16), window=(0, 16, 0, 16), fmt=fmt, base_offset=fmt, offset=0))
        tasks.append(dict(plane=plane_of(16, 16), window=(15, 16, 3, 16), fmt=fmt, base_offset=0, offset=ELEM[fmt] * 3))
    for fmt in (1, 2, 3):                                      # the formats' edges: subnormal results, ties, overflow to infinity, a subnormal scale
        for scale, bias in ((1e-7, 0.0), (2.0 ** -24, 0.0), (2.0 ** -25, 0.0), (3e-8, 0.0), (300.0, -1.0), (1e-45, 0.0), (3.0e38, 0.0), (-1e-7, 0.0)):
            tasks.append(dict(plane=np.arange(256, dtype=np.uint8).reshape(1, 256), window=(0, 1, 0, 256), fmt=fmt, scale=scale, bias=bias,
                              base_offset=len(tasks) % 16, offset=ELEM[fmt] * (len(tasks) % 3)))
    gated = []
    for fmt in range(4):
        for status in (1, 0, 2, 3, -7):
            gated.append(len(tasks))
            tasks.append(dict(plane=plane_of(149), window=(1, 4, 3, 36), fmt=fmt, scale=NORMS[1 if fmt else 0][0], bias=NORMS[1 if fmt else 0][1],
                              pitch=34 * ELEM[fmt], offset=ELEM[fmt], base_offset=status % 16, gate_status=status))
        tasks.append(dict(plane=plane_of(149), window=(0, 5, 0, 149), fmt=fmt, offset=7 * ELEM[fmt], zero=True))
    assert len(tasks) > 400 and {t.get("base_offset", 0) for t in tasks} == set(range(16))
    with _live(pkg):
        outs = gpu_ctx.debug_deliver(tasks)
    assert len(outs) == len(tasks)
    for i, (t, got) in enumerate(zip(tasks, outs)):
        fmt, window = t["fmt"], t["window"]
        e = ELEM[fmt]
        pitch, offset = t.get("pitch", (window[3] - window[2]) * e), t.get("offset", 0)
        scale, bias = t.get("scale", 1.0), t.get("bias", 0.0)
        zero = t.get("zero", False) or t.get("gate_status", -1) not in (-1, 1)
        with np.errstate(over="ignore"):
            want = expected(t["plane"], window, fmt, scale, bias, pitch, offset, got.size, zero=zero)   # numpy, guards included
        assert np.array_equal(got, want), (i, {k: v for k, v in t.items() if k != "plane"})
        host = pkg.deliver_host(t["plane"], window, fmt, scale, bias, pitch=pitch, offset=offset, out_bytes=got.size, zero=t.get("zero", False),
                                gate_status=t.get("gate_status", -1))
        assert np.array_equal(got, host), i
    for i in gated:                                            # (a gate that is not done leaves zeros, not the pattern and not pixels)
        t = tasks[i]
        row = outs[i][t["offset"]:t["offset"] + 33 * ELEM[t["fmt"]]]
        assert row.any() == (t["gate_status"] == 1) and (t["gate_status"] == 1 or not row.any()), i
    with pytest.raises(ValueError):
        gpu_ctx.debug_deliver([dict(plane=plane_of(149), window=(0, 5, 0, 150), fmt=0)])
    with pytest.raises(ValueError):
        gpu_ctx.debug_deliver([dict(plane=plane_of(149), window=(0, 5, 0, 149), fmt=3, offset=2)])
    with pytest.raises(ValueError):
        gpu_ctx.debug_deliver([dict(plane=plane_of(149), window=(0, 5, 0, 149), fmt=0, scale=2.0)])
    with pytest.raises(ValueError):
        gpu_ctx.debug_deliver([dict(plane=plane_of(149), window=(0, 5, 0, 149), fmt=0, base_offset=16)])


def _all_made(gpu_ctx, pkg, oracle, Rs=(1, 3, 7)):
    made = [_made(gpu_ctx, oracle, kind, near, effort, h, w, R) + ((kind, near, effort, h, w, R),)
            for kind, near, effort in CASES for h, w in GEOMS for R in Rs]
    pairs = [(s, pkg.pack_index(ix) if k % 2 else ix) for k, (s, ix, _, _) in enumerate(made)]       # packed and unpacked indexes mixed
    return made, pairs


def test_whole_planes_into_one_uint8_tensor(gpu_ctx, pkg, oracle):
    """Every case x geometry x R in one call, image k into out[k, :h, :w] of one tensor: the oracle's planes, the rest of
    the tensor untouched, and the host call unchanged next to it."""
    made, pairs = _all_made(gpu_ctx, pkg, oracle)
    n = len(made)
    hm, wm = max(h for h, _ in GEOMS) + 1, max(w for _, w in GEOMS) + 3
    out = _filled((n, hm, wm), 0)
    views = [out[k, :rec.shape[0], :rec.shape[1]] for k, (_, _, rec, _) in enumerate(made)]
    host_before = gpu_ctx.decode_batch_indexed(pairs)
    with _live(pkg):
        info = {}
        status = gpu_ctx.decode_batch_indexed_into(pairs, views, info=info)
    assert status == [0] * n and info["rc"] == 0 and info["status"] == status
    got = _bits(out)
    host_after = gpu_ctx.decode_batch_indexed(pairs)
    for k, (_, _, rec, case) in enumerate(made):
        h, w = rec.shape
        assert np.array_equal(got[k, :h, :w], rec), case
        assert (got[k, h:, :] == PATTERN).all() and (got[k, :, w:] == PATTERN).all(), case
        assert np.array_equal(host_before[k], rec) and np.array_equal(host_after[k], rec), case
    assert gpu_ctx.indexed_decode_split()["copy_out"] >= 0
    # a [N, 1, H, W] tensor of equal shapes, given whole
    same = [m for m in made if m[3][3:5] == GEOMS[1]]
    out4 = _filled((len(same), 1) + GEOMS[1], 0)
    assert gpu_ctx.decode_batch_indexed_into([(s, ix) for s, ix, _, _ in same], out4) == [0] * len(same)
    got4 = _bits(out4)
    for k, (_, _, rec, case) in enumerate(same):
        assert np.array_equal(got4[k, 0], rec), case


@pytest.mark.parametrize("fmt", (1, 2, 3))
def test_row_ranges_and_column_windows_into_float_views(gpu_ctx, pkg, oracle, fmt):
    """Row ranges that cross three segments with odd column windows, into views whose row stride is larger than the
    window: the numpy expression on the oracle's plane, bit for bit, and the elements outside the views untouched."""
    scale, bias = NORMS[fmt % 3]
    pairs, rows, cols, want = [], [], [], []
    for i, (kind, near, effort) in enumerate(CASES):
        for (h, w), R in (((67, 150), 7), ((23, 149), 3), ((40, 131), 1)):
            s, ix, rec = _made(gpu_ctx, oracle, kind, near, effort, h, w, R)
            k = ((h - 1) // R) // 2 + 1
            r = (k * R - R - 1, min(h, k * R + 2))
            assert (r[1] - 1) // R - r[0] // R >= 2
            for c in ((1, 18), (w - 33, w), (0, w), (5 + i, 6 + i), (3, 3 + 16 + (i & 1))):
                pairs.append((s, pkg.pack_index(ix) if len(pairs) % 3 == 0 else ix)); rows.append(r); cols.append(c)
                want.append(_elements(rec[r[0]:r[1], c[0]:c[1]], fmt, scale, bias))
    n = len(pairs)
    hm, wm = max(x.shape[0] for x in want) + 2, max(x.shape[1] for x in want) + 5
    out = _filled((n, hm, wm), fmt)
    views = [out[k, 1:1 + x.shape[0], 2 + (k % 3):2 + (k % 3) + x.shape[1]] for k, x in enumerate(want)]
    with _live(pkg):
        status = gpu_ctx.decode_batch_indexed_into(pairs, views, rows=rows, cols=cols, scale=scale, bias=bias)
    assert status == [0] * n
    got = _bits(out)
    fill = int.from_bytes(bytes([PATTERN]) * ELEM[fmt], "little")
    for k, x in enumerate(want):
        c0 = 2 + (k % 3)
        assert np.array_equal(got[k, 1:1 + x.shape[0], c0:c0 + x.shape[1]], x), (k, rows[k], cols[k])
        mask = np.ones((hm, wm), bool)
        mask[1:1 + x.shape[0], c0:c0 + x.shape[1]] = False
        assert (got[k][mask] == fill).all(), (k, rows[k], cols[k])
    # the host call on the same ranges returns the rows it returned before
    host = gpu_ctx.decode_batch_indexed(pairs[::5], rows[::5])
    for g, (s, ix), r in zip(host, pairs[::5], rows[::5]):
        assert g is not None and g.shape[0] == r[1] - r[0]


def test_forged_refused_and_bad_calls(gpu_ctx, pkg, oracle):
    torch = _torch()
    h, w, R = 67, 150, 7
    e1 = [_made(gpu_ctx, oracle, "n", 0, 1, h, w, R, seed) for seed in (5, 6, 7)]
    forged = _forge(e1[1][1], 4, "n", 1, w, "row1")
    assert pkg.check_index(forged, e1[1][0])
    scale, bias = NORMS[1]
    with _live(pkg):
        # a forged entry: its window is all zero, its neighbours are right
        for fmt in (0, 1):
            out = _filled((3, h, w), fmt)
            info = {}
            norm = dict(scale=scale, bias=bias) if fmt else {}
            status = gpu_ctx.decode_batch_indexed_into([(e1[0][0], e1[0][1]), (e1[1][0], forged), (e1[2][0], e1[2][1])], out, info=info, **norm)
            assert status == [0, -1, 0] and info["rc"] == -1
            got = _bits(out)
            assert not got[1].any()
            for k in (0, 2):
                assert np.array_equal(got[k], _elements(e1[k][2], fmt, scale if fmt else 1.0, bias if fmt else 0.0)), (fmt, k)
        # refused images: status -1, the destination keeps its pattern, the neighbours are delivered
        good = (e1[0][0], e1[0][1])
        for fmt, what in ((0, "host pointer"), (1, "pitch"), (3, "misaligned"), (0, "rows outside"), (2, "cols outside"), (1, "cap"), (0, "empty"), (3, "null")):
            e = ELEM[fmt]
            out = _filled((3, h + 1, w + 8), fmt)
            raw = out.view(torch.uint8).reshape(3, -1)
            pitch = (w + 8) * e
            cap = lambda rows, cols: (rows - 1) * pitch + cols * e
            dests = [(out[k].data_ptr(), pitch, cap(h, w), 0, 0, 0, 0) for k in range(3)]
            host = np.full(h * w * e + 64, PATTERN, np.uint8)
            dests[1] = {"host pointer": (host.ctypes.data, w * e, host.size, 0, 0, 0, 0),
                        "pitch": (dests[1][0], (w - 1) * e, 1 << 20, 0, 0, 0, 0),
                        "misaligned": (dests[1][0] + 2, pitch, cap(h, w), 0, 0, 0, 0),
                        "rows outside": (dests[1][0], pitch, cap(h, w), 5, h + 1, 0, 0),
                        "cols outside": (dests[1][0], pitch, cap(h, w), 0, 0, 3, w + 1),
                        "cap": (dests[1][0], pitch, cap(h, w) - 1, 0, 0, 0, 0),
                        "empty": (dests[1][0], pitch, cap(h, w), 4, 4, 0, 0),
                        "null": (0, pitch, cap(h, w), 0, 0, 0, 0)}[what]
            norm = (scale, bias) if fmt else (1.0, 0.0)
            info = {}
            status = gpu_ctx.decode_batch_indexed_to([good, (e1[1][0], e1[1][1]), good], dests, fmt, *norm, info=info)
            assert status == [0, -1, 0] and info["rc"] == -1, what
            torch.cuda.synchronize()
            assert bool((raw[1] == PATTERN).all()), what
            assert (host == PATTERN).all(), what
            got = _bits(out)
            for k in (0, 2):
                assert np.array_equal(got[k, :h, :w], _elements(e1[0][2], fmt, *norm)), (what, k)
        # a tensor whose shape is not the window's, a tensor on the host: refused alone
        out = _filled((2, h, w), 0)
        assert gpu_ctx.decode_batch_indexed_into([good, good], [out[0], out[1, :h - 1]]) == [0, -1]
        assert bool((out[1] == PATTERN).all()) and np.array_equal(_bits(out[0]), e1[0][2])
        cpu = torch.full((h, w), PATTERN, dtype=torch.uint8)
        assert gpu_ctx.decode_batch_indexed_into([good, good], [out[0], cpu]) == [0, -1] and bool((cpu == PATTERN).all())
        # the call refused: nothing launched, nothing written
        before = gpu_ctx.serial_launches()
        out = _filled((1, h, w), 0)
        for kw in (dict(scale=2.0), dict(bias=1.0), dict(scale=float("nan")), dict(bias=float("inf"))):
            info = {}
            assert gpu_ctx.decode_batch_indexed_into([good], out, info=info, **kw) == [-1] and info["rc"] == -1, kw
            assert gpu_ctx.decode_batch_into([good[0]], out, info=info, **kw) == [-1] and info["rc"] == -1, kw
        assert gpu_ctx.decode_batch_indexed_to([good], [(out.data_ptr(), w, h * w, 0, 0, 0, 0)], 4) == [-1]
        assert gpu_ctx.decode_batch_to([good[0]], [(out.data_ptr(), w, h * w, 0, 0, 0, 0)], -1) == [-1]
        assert gpu_ctx.serial_launches() == before and bool((out == PATTERN).all())
        with pytest.raises(ValueError):
            gpu_ctx.decode_batch_indexed_into([good], torch.zeros((1, h, w), dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            gpu_ctx.decode_batch_indexed_into([good], [torch.zeros((w, h), dtype=torch.uint8, device="cuda").t()])
    assert np.array_equal(gpu_ctx.decode_batch_indexed([good])[0], e1[0][2])


def test_decode_batch_into(gpu_ctx, pkg, oracle):
    """The plain batch decode (no index) into device tensors: whole planes and windows, a stream cut short in its payload,
    and decode_batch itself on the same streams."""
    torch = _torch()
    made = [_made(gpu_ctx, oracle, kind, near, effort, h, w, 7) for kind, near, effort in CASES for h, w in GEOMS]
    streams = [s for s, _, _ in made]
    n = len(made)
    host = gpu_ctx.decode_batch(streams)
    hm, wm = max(h for h, _ in GEOMS), max(w for _, w in GEOMS)
    assert gpu_ctx.decode_batch_into(streams[:1], _filled((1,) + made[0][2].shape, 0)) == [0]       # (the context's grow-only task buffer exists from here on)
    with _live(pkg):
        out = _filled((n, hm + 1, wm + 2), 0)
        status = gpu_ctx.decode_batch_into(streams, [out[k, :rec.shape[0], :rec.shape[1]] for k, (_, _, rec) in enumerate(made)])
        assert status == [0] * n
        got = _bits(out)
        for k, (_, _, rec) in enumerate(made):
            h, w = rec.shape
            assert np.array_equal(got[k, :h, :w], rec) and np.array_equal(host[k][0], rec), k
            assert (got[k, h:] == PATTERN).all() and (got[k, :, w:] == PATTERN).all(), k
        for fmt in (1, 2, 3):
            scale, bias = NORMS[fmt % 3]
            rows = [(1 + k % 3, rec.shape[0] - (k % 2)) for k, (_, _, rec) in enumerate(made)]
            cols = [(k % 17, k % 17 + (1, 15, 16, 17, 33)[k % 5]) for k in range(n)]
            want = [_elements(rec[r[0]:r[1], c[0]:c[1]], fmt, scale, bias) for (_, _, rec), r, c in zip(made, rows, cols)]
            out = _filled((n, hm + 1, 40), fmt)
            views = [out[k, 1:1 + x.shape[0], 3:3 + x.shape[1]] for k, x in enumerate(want)]
            assert gpu_ctx.decode_batch_into(streams, views, rows=rows, cols=cols, scale=scale, bias=bias) == [0] * n
            got = _bits(out)
            fill = int.from_bytes(bytes([PATTERN]) * ELEM[fmt], "little")
            for k, x in enumerate(want):
                assert np.array_equal(got[k, 1:1 + x.shape[0], 3:3 + x.shape[1]], x), (fmt, k)
                mask = np.ones(got[k].shape, bool)
                mask[1:1 + x.shape[0], 3:3 + x.shape[1]] = False
                assert (got[k][mask] == fill).all(), (fmt, k)
        # a stream cut short in its payload fails on the device: zeros and -1, the others unaffected
        s0, _, rec0 = made[1]
        cut = s0[:len(s0) * 2 // 3]
        assert gpu_ctx.decode_batch([cut])[0] is None
        out = _filled((3,) + rec0.shape, 1)
        info = {}
        assert gpu_ctx.decode_batch_into([s0, cut, s0], out, scale=NORMS[1][0], bias=NORMS[1][1], info=info) == [0, -1, 0] and info["rc"] == -1
        got = _bits(out)
        assert not got[1].any()
        assert np.array_equal(got[0], _elements(rec0, 1, *NORMS[1])) and np.array_equal(got[2], got[0])
        # refused: a destination on the host, a window outside the image
        cpu = torch.full(rec0.shape, PATTERN, dtype=torch.uint8)
        dev = _filled(rec0.shape, 0)
        assert gpu_ctx.decode_batch_into([s0, s0], [cpu, dev]) == [-1, 0] and bool((cpu == PATTERN).all())
        assert np.array_equal(_bits(dev), rec0)
        dev = _filled(rec0.shape, 0)
        assert gpu_ctx.decode_batch_to([s0], [(dev.data_ptr(), rec0.shape[1], rec0.size, 0, rec0.shape[0] + 1, 0, 0)], 0) == [-1]
        assert bool((dev == PATTERN).all())
    after = gpu_ctx.decode_batch(streams)
    for a, b in zip(host, after):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
