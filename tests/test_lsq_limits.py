"""The two least-squares solvers of efforts 2 / 3 where the exact range of the doubles ends (csrc/lsq_f64.h Guard).

The kernels carry the reference's int64 normal equations in doubles and redo a pixel with plain 64-bit integers
(serial_engine.hip lsq_solve_int) when a magnitude leaves the range in which the doubles are exact.  Here both solvers
run on the device on systems alone -- no image, no coder -- through nblic_amd_lsq_probe, in the three lane layouts the
kernels use, and are compared with tests/host_harness.cpp's solve_int (the reference's int64 algorithm restated; pinned
by the oracle tests of test_host_logic.py).  The systems (tests/lsq_cases.py): recorded ones, which the harness writes
down at every redo pixel and as many ordinary pixels of hard-edged planes (plus `const` and `syn1`), and ones placed
on the four limits.  Every comparison is exact: integers.

The CPU part (unmarked) checks that the systems are what they claim to be; the GPU part is marked `gpu`."""
import numpy as np
import pytest

import inputs
import lsq_cases as L

LAYOUTS = [(6, 1), (10, 1), (10, 2)]        # (order, waves): R = 8, R = 16 on one wave, the two-wave split of effort 3


@pytest.fixture(scope="module")
def harness():
    return L.load_harness()


def _within(maxima):
    """Guard::ok from the four maxima, with the limits as this suite states them."""
    return np.all(np.stack([maxima[:, k] < float(L.LIMITS[q]) for k, q in enumerate(L.QUANTITIES)], 1), 1)


@pytest.mark.parametrize("n", [6, 10])
def test_systems_are_on_both_sides_of_every_limit(harness, n):
    """Set-up of the device test, checked without a GPU: at least 4096 systems; with solve_f64 and the host Guard alone at
    least a quarter of them are inside and at least a quarter outside the exact range, in either system slot; the planted
    magnitude is the Guard's maximum, exactly, in nearly all planted systems (the recorded part of a system may exceed it),
    on every step around every limit; the host Guard's verdict is the four limits as lsq_cases.LIMITS states them; and wherever
    it says `exact`, the doubles gave the reference's integer."""
    S = L.systems(harness, n)
    hi, hf = S["host_i64"], S["host_f64"]
    K = len(S["bias"])
    assert K >= 4096 and S["n_recorded"] >= 256
    redo = S["recorded_redo"]
    assert (redo != 0).sum() >= 64 and (redo == 0).sum() >= (redo != 0).sum()
    for s in (0, 1):
        inside = hi[:, 8 + s] == 1
        assert 4 * inside.sum() >= K and 4 * (~inside).sum() >= K, (n, s, inside.mean())
        assert np.array_equal(inside, _within(hf[:, 4 * s:4 * s + 4])), "Guard::ok is not the four limits"
        both = inside & (hi[:, 2 + s] == 1)
        assert np.array_equal(hi[:, 6 + s][inside], hi[:, 2 + s][inside])
        assert np.array_equal(hi[both, 4 + s], L.clamp_q12(hi[both, s]))
    # no solution (a zero pivot, NBLIC.c:118) is among the systems: `const`
    assert (hi[:, 2] == 0).sum() >= 16
    hits, total, sides = {}, {}, {}
    for k, tg in enumerate(S["targets"]):
        if tg is None or tg[0] != "planted":
            continue
        _, q, T, slot = tg
        got = hf[k, 4 * slot + L.QUANTITIES.index(q)]
        # (the quotient the Guard sees is the estimate (+-4 T + 2) (1 - 2^-48) / 4: T + 1/2 or T - 1/2, shortened by up to 1/2 at 2^47)
        exact = abs(got - T) <= 1 if q == "quotient" else got == float(T)
        hits[q] = hits.get(q, 0) + int(exact)
        total[q] = total.get(q, 0) + 1
        if exact:
            sides.setdefault((q, slot), set()).add(T)
    for q in L.QUANTITIES:
        assert total[q] >= 400 and hits[q] * 10 >= total[q] * 9, (q, hits[q], total[q])
        for slot in (0, 1):
            placed = sides[(q, slot)]
            lim = L.LIMITS[q]
            assert {lim // 2, lim - 1, lim, lim + 1, 2 * lim} <= placed, (q, slot)
    # the products past 2^63 wrap in the reference's int64: they are among the systems, and solve_int still answers
    wrapped = [k for k, tg in enumerate(S["targets"]) if tg is not None and tg[1] == "product" and tg[0] == "planted" and tg[2] >= 2 ** 63]
    assert sum(1 for k in wrapped if hi[k, 2] == 1 and hi[k, 3] == 1) >= 100


def test_hard_edged_planes_reach_the_integer_redo_on_the_cpu(harness):
    """The counts the GPU suites rely on (they ask for at least one redo pixel on the device where the CPU harness
    shows at least eight): 64x64 step_v in every near-lossless mode of efforts 2 / 3, stripes_h at effort 2; all of
    them in system 0.  And none at all for lossless syn1: a counter that counts every pixel cannot pass."""
    for near, effort in [(2, 2), (9, 2), (1, 3), (2, 3), (9, 3)]:
        assert L.redo_pixels(harness, inputs.make_hard("step_v", 64, 64), near, effort)[0] >= 8, (near, effort)
    for near, effort in [(2, 2), (9, 2)]:
        assert L.redo_pixels(harness, inputs.make_hard("stripes_h", 64, 64), near, effort)[0] >= 8, (near, effort)
    for effort in (2, 3):
        assert L.redo_pixels(harness, inputs.syn1(64, 64, 1), 0, effort) == (0, 0)
    # lossless reaches the redo too, rarely: one of 60 random block planes does with several pixels (inputs.make_hard)
    lossless = inputs.make_hard("blocks_lossless", 0, 0)
    assert L.redo_pixels(harness, lossless, 0, 2) == (4, 0) and L.redo_pixels(harness, lossless, 0, 3) == (15, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,waves", LAYOUTS)
def test_device_solvers_equal_the_reference_integers(gpu_ctx, harness, n, waves):
    """serial_engine.hip's own LsqLds / solve_with / lsq_solve_int / predict / solve_one + take_other on >= 4096 systems
    per layout.
      1. the integer path gives solve_int's sum and verdict for EVERY system (the wrapped products included);
      2. wherever the device Guard says `exact`, the double path gives solve_int's (clamped) sum and verdict;
      3. the device Guard is the four limits applied to the maxima it reports, and its verdict is compared with the host
         Guard's: they may differ only where the host's solve_f64 stopped at a zero pivot (it returns before its Guard has
         seen the rest; the device goes on, meets an infinity and redoes the pixel) -- DESIGN.md; the count is printed;
      4. not vacuous: at least a quarter of the systems inside and a quarter outside the exact range, per slot;
    and what the kernels deliver for the pixel (p1, p2, ok1, ok2 after their own redo decision, system 1 of the two-wave
    layout through the xch hand-over) is the reference's integer for every system, with the redo counted where the Guard
    tripped."""
    S = L.systems(harness, n)
    hi = S["host_i64"]
    K = len(S["bias"])
    of, oi = gpu_ctx.lsq_probe(n, waves, S["D"], S["vn"], S["bias"])
    differ = 0
    for s in (0, 1):
        ref_ok, ref_p = hi[:, 2 + s] == 1, hi[:, s]
        # 1
        assert np.array_equal(oi[:, 10 + s] == 1, ref_ok), (n, waves, s)
        assert np.array_equal(oi[ref_ok, 8 + s], ref_p[ref_ok]), (n, waves, s, int((oi[ref_ok, 8 + s] != ref_p[ref_ok]).sum()))
        # 3 (first half) and 4
        exact = oi[:, 6 + s] == 1
        assert np.array_equal(exact, _within(of[:, 2 + 4 * s:6 + 4 * s])), "device Guard::ok is not the four limits"
        assert 4 * exact.sum() >= K and 4 * (~exact).sum() >= K, (n, waves, s, exact.mean())
        # 2
        assert np.array_equal(oi[exact, 4 + s] == 1, ref_ok[exact]), (n, waves, s)
        both = exact & ref_ok
        assert np.array_equal(of[both, s], L.clamp_q12(ref_p[both]).astype(np.float64)), (n, waves, s)
        # 3 (second half)
        host_exact = hi[:, 8 + s] == 1
        mism = exact != host_exact
        assert not np.any(mism & ref_ok), (n, waves, s, int((mism & ref_ok).sum()))
        differ += int(mism.sum())
        # the pixel as the kernels deliver it
        assert np.array_equal(oi[:, 2 + s] == 1, ref_ok), (n, waves, s)
        assert np.array_equal(oi[ref_ok, s], L.clamp_q12(ref_p[ref_ok])), (n, waves, s)
        assert np.array_equal(oi[:, 12 + s], 1 - oi[:, 6 + s]), (n, waves, s)
    print(f"lsq probe n={n} waves={waves}: {K} systems, device/host Guard verdicts differ on {differ} (zero-pivot systems)")
