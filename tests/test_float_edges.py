"""GPU suite (-m gpu): the DEVICE bodies of collect_value, deliver_value and deep_value against the exact reference of
tests/float_edge_inputs.py, on the inputs where a conversion that breaks the contract -- a fused multiply-add, a flushed
denormal, another tie rule, another narrowing -- gives another answer.  Every test is one or two launches; the expected
outputs are computed once on the CPU and shared with tests/test_float_edges_host.py, which holds the host bodies to them.
A kernel built with the two operations fused fails the collect, deliver and deep tests here and passes the older ones."""
import numpy as np
import pytest

import float_edge_inputs as fe

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _check_planes(pkg, what, domains, outs, guard):
    for (d, want), got in zip(domains, outs):
        n = want.size
        plane = got[guard:guard + n]
        assert np.array_equal(plane, want.reshape(-1)), fe.explain_plane(what + ", " + d["name"], d["fmt"], d["scale"], d["bias"], d["bits"], plane, want)
        assert (got[:guard] == pkg.COLLECT_PATTERN).all() and (got[guard + n:] == pkg.COLLECT_PATTERN).all(), (what, d["name"], fe.NAMES[d["fmt"]], "a guard byte changed")


def test_k_collect_converts_every_domain_as_the_contract_says(gpu_ctx, pkg):
    """ONE launch carries every collect domain contiguous (aligned words wherever sixteen elements lie in a row), a second
    one the same elements three apart at an odd residue (element by element)."""
    domains = fe.collect_expected()
    for layout in ("contiguous", "strided"):
        outs = gpu_ctx.debug_collect([fe.collect_task(d, layout, k) for k, (d, _) in enumerate(domains)])
        _check_planes(pkg, "k_collect, " + layout, domains, outs, pkg.COLLECT_GUARD)


def test_k_collect_with_a_reference_converts_both_channels(gpu_ctx, pkg):
    t, own, ref, want = fe.collect_ref_task()
    got = gpu_ctx.debug_collect_ref([t])[0]
    g = pkg.COLLECT_GUARD
    plane = got[g:g + want.size]
    assert np.array_equal(plane, want.reshape(-1)), fe.explain_plane("k_collect with a reference (the pixel is own - ref + 128)", 1, t["scale"], t["bias"], own, plane, want)
    assert (got[:g] == pkg.COLLECT_PATTERN).all() and (got[g + want.size:] == pkg.COLLECT_PATTERN).all()


def _strip(t):
    return {k: v for k, v in t.items() if k != "pair"}


def test_k_deliver_makes_every_element_as_the_contract_says(gpu_ctx, pkg):
    tasks = fe.deliver_tasks()
    outs = gpu_ctx.debug_deliver([t for t, _ in tasks])
    for (t, want), got in zip(tasks, outs):
        assert np.array_equal(got, want), fe.explain_buffer("k_deliver", t["fmt"], t["scale"], t["bias"], t, fe.PIXEL_PLANE, got, want)


def test_k_deliver_with_a_reference(gpu_ctx, pkg):
    tasks = fe.deliver_ref_tasks()
    outs = gpu_ctx.debug_deliver_ref([t for t, _ in tasks])
    for (t, want), got in zip(tasks, outs):
        assert np.array_equal(got, want), fe.explain_buffer("k_deliver with a reference", t["fmt"], t["scale"], t["bias"], t, fe.PIXEL_PLANE, got, want)


def test_k_deliver_deep_makes_every_value_as_the_contract_says(gpu_ctx, pkg):
    """All 65536 values, unsigned and signed, into the three float formats under every pair, in ONE launch."""
    tasks = fe.deep_tasks()
    inverse = {v: k for k, v in fe.DEEP_FMT.items()}
    outs = gpu_ctx.debug_deep_deliver([_strip(t) for t, _ in tasks])
    for (t, want), got in zip(tasks, outs):
        values = fe.DEEP_U - (32768 if t["mode"] & 2 else 0)
        assert np.array_equal(got, want), fe.explain_buffer("k_deliver_deep, %s, mode %d" % (t["pair"], t["mode"]), inverse[t["fmt"]], t["scale"], t["bias"], t, values, got, want)


def test_k_deliver_stack_makes_every_slice_as_the_contract_says(gpu_ctx, pkg):
    tasks = fe.stack_tasks()
    runs = gpu_ctx.debug_stack_deliver([t for t, _, _ in tasks])
    for (t, want, slices), run in zip(tasks, runs):
        for d, (g, w) in enumerate(zip(run, want)):
            dest = dict(offset=t["offsets"][d], pitch=t["pitches"][d], step=t["steps"][d])
            assert np.array_equal(g, w), fe.explain_buffer("k_deliver_stack, slice %d" % d, t["fmt"], t["scales"][d], t["biases"][d], dest, slices[d], g, w)


def test_the_cost_kernels_convert_their_sources_as_the_contract_says(gpu_ctx, pkg):
    """k_color_cost and k_stack_cost on float16 and float32 frames of witnesses and specials: numpy's sums on the planes the
    exact reference collects."""
    made = fe.cost_tasks()
    color = gpu_ctx.debug_color_cost([made[("color", fmt)][0] for fmt in (1, 3)])
    stack = gpu_ctx.debug_stack_cost([made[("stack", fmt)][0] for fmt in (1, 3)])
    for k, fmt in enumerate((1, 3)):
        t, planes = made[("color", fmt)]
        want = pkg.color_cost_numpy(*planes)
        assert np.array_equal(color[k], want), ("k_color_cost", fe.NAMES[fmt], t["scale"], t["bias"], color[k].tolist(), want.tolist())
        t, planes = made[("stack", fmt)]
        want = pkg.stack_cost_numpy(planes)
        assert np.array_equal(stack[k], want), ("k_stack_cost", fe.NAMES[fmt], t["scale"], t["bias"], stack[k].tolist(), want.tolist())


@pytest.mark.parametrize("fmt", (1, 3))
def test_encode_batch_from_quantises_the_witnesses_as_the_contract_says(gpu_ctx, pkg, fmt):
    """The public path: a tensor that holds the witness set, and a view of every third column of a wider one, give the
    streams of the planes the exact reference collects."""
    torch = _torch()
    scale, bias = fe.COLLECT_WITNESS_PAIR[fmt]
    w = fe.collect_witness_inputs(fmt)
    bits = fe.as_image(w, 37 if fmt == 1 else 131, w[0]).astype(np.uint16 if fmt == 1 else np.uint32)
    want = fe.collect_ref(bits, fmt, scale, bias)
    assert fe.witnesses(want, fe.collect_ref(bits, fmt, scale, bias, fused=True)) >= fe.COLLECT_WITNESS_MIN[fmt]
    values = bits.view(np.float16 if fmt == 1 else np.float32)
    dense = torch.from_numpy(values).cuda()
    wide = torch.zeros((bits.shape[0], 3 * bits.shape[1] + 1), dtype=dense.dtype, device="cuda")
    wide[:, 1::3] = dense
    torch.cuda.synchronize()
    got = gpu_ctx.encode_batch_from([dense, wide[:, 1::3]], scale=scale, bias=bias)
    streams = gpu_ctx.encode_batch([want])
    if got != streams + streams:                               # say which element: the collected plane, through the kernel alone
        plane = gpu_ctx.debug_collect([dict(raw=bits, rows=bits.shape[0], cols=bits.shape[1], fmt=fmt, scale=scale, bias=bias)])[0]
        plane = plane[pkg.COLLECT_GUARD:pkg.COLLECT_GUARD + want.size]
        detail = fe.explain_plane("k_collect", fmt, scale, bias, bits, plane, want) if not np.array_equal(plane, want.reshape(-1)) else "the collected plane is right"
        raise AssertionError("encode_batch_from: %s scale %r bias %r: the streams differ from those of the reference's plane; %s" % (fe.NAMES[fmt], scale, bias, detail))


@pytest.mark.parametrize("fmt", (1, 2, 3))
def test_decode_batch_into_normalises_as_the_contract_says(gpu_ctx, pkg, fmt):
    torch = _torch()
    _, scale, bias = fe.DELIVER_FOUND[fmt]
    plane = np.ascontiguousarray(np.tile(fe.PIXELS.astype(np.uint8).reshape(16, 16), (2, 3))[:, :47])          # every pixel, rows of 47
    want = fe.deliver_ref(plane, fmt, scale, bias)
    assert fe.witnesses(want, fe.deliver_ref(plane, fmt, scale, bias, fused=True)) >= fe.DELIVER_FOUND[fmt][0]
    streams = gpu_ctx.encode_batch([plane])
    dtype = {1: torch.float16, 2: torch.bfloat16, 3: torch.float32}[fmt]
    out = torch.zeros((1,) + plane.shape, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    assert gpu_ctx.decode_batch_into(streams, out, scale=scale, bias=bias) == [0]
    torch.cuda.synchronize()
    host = out[0].cpu().contiguous()
    got = host.view(torch.int32 if fmt == 3 else torch.int16).numpy().view(np.uint32 if fmt == 3 else np.uint16).astype(np.uint32)
    if not np.array_equal(got, want):
        i = fe.first_difference(got, want)
        raise AssertionError("decode_batch_into: %s scale %r bias %r: %d of %d elements differ, first element %d, pixel %d: got bits 0x%X, the contract gives 0x%X" % (
            fe.NAMES[fmt], scale, bias, int((got != want).sum()), want.size, i, int(plane.reshape(-1)[i]), int(got.reshape(-1)[i]), int(want.reshape(-1)[i])))
