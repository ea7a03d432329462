"""CPU side of the foreign QNBLIC streams (q_foreign_inputs.py): the tables are what they claim to be, the oracle and the
compiled reference decode every stream to its plane, the host entropy stage codes the same bytes from the same tables,
and the set puts under load what it was made for -- asserted from a plain replay of the decoder's entropy side."""
import hashlib
import time

import numpy as np

import q_foreign_inputs as qf
from oracle.oracle import Reference, out_capacity


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def test_every_table_is_a_fixed_point_of_the_scaling(oracle):
    """Each level sums to 2^15, holds at least two nonzero entries, none above 32767, gives every coded symbol a slot --
    and orc_q_norm_hist returns it unchanged, so the stream carries exactly these tables (read back from the stream)."""
    seen = set()
    for c in qf.cases(oracle):
        if c.policy != "greedy":
            continue
        _, qd, y, counts = qf.models(oracle)[c.plane_name]
        t = c.tables
        assert t.shape == (12, 256) and t.dtype == np.uint32
        for k in range(12):
            case = (c.plane_name, c.family, k)
            assert int(t[k].sum()) == qf.NORM and np.count_nonzero(t[k]) >= 2 and int(t[k].max()) <= qf.NORM - 1, case
            assert np.array_equal(oracle.q_norm_hist(t[k]), t[k]), case
        assert (t[counts > 0] > 0).all(), (c.plane_name, c.family)
        assert np.array_equal(qf.tables_of(c.stream)[2], t), (c.plane_name, c.family)
        seen.add(c.family)
    assert seen == set(qf.FAMILIES)


def test_family_shapes(oracle):
    m = qf.models(oracle)
    plane, qd, y, counts = m["flat_8x8"]
    assert not qd.any() and not y.any()                                   # every pixel: level 0, symbol 0
    for fam, pair in (("far_pair", {0: 1, 128: 32767}), ("far_pair_mirror", {0: 32767, 128: 1})):
        t = qf.case_of(oracle, "flat_8x8", fam).tables
        for k in range(12):
            assert {int(s): int(t[k][s]) for s in np.flatnonzero(t[k])} == pair, (fam, k)
    _, _, _, counts = m["syn1_64x64"]
    t = qf.case_of(oracle, "syn1_64x64", "sparse").tables
    for k in range(12):
        occ = counts[k] > 0
        assert (t[k][occ] == 1).all() and np.count_nonzero(t[k][~occ]) >= 1, k
    assert (qf.case_of(oracle, "syn1_64x64", "uniform").tables == 128).all()
    assert (qf.case_of(oracle, "syn1_64x64", "smoothed").tables > 0).all()
    t = qf.case_of(oracle, "syn1_64x64", "ones_on_254").tables
    assert (np.delete(t, 254, axis=1) == 1).all() and (t[:, 254] == qf.NORM - 255).all()
    r = qf.case_of(oracle, "syn1_64x64", "rotated").tables
    assert np.array_equal(r[0], t[0]) and np.array_equal(r[5], t[5]) and (r[2] == 128).all() and (r[7] == 128).all()
    assert np.array_equal(r[1], qf.case_of(oracle, "syn1_64x64", "sparse").tables[1])
    assert np.array_equal(r[3], qf.case_of(oracle, "syn1_64x64", "smoothed").tables[3])


def test_policies_write_other_codes_than_the_greedy_writer(oracle):
    """Every policy reads back to the same tables (recode asserts it) with, for at least one table, other codes than the
    greedy writer's; between them the streams use all five code shapes, runs with and without the tail nibble, and runs
    of the shortest length the code has and the longest a table can hold (255: all but one symbol)."""
    differs = {p: 0 for p in qf.POLICIES[1:]}
    shapes, run_lengths, tails = {p: set() for p in qf.POLICIES}, set(), set()
    by_key = {}
    for c in qf.cases(oracle):
        by_key[(c.plane_name, c.family, c.policy)] = c
    for (name, fam, policy), c in by_key.items():
        s, q_pos, freq, codes = qf.tables_of(c.stream)
        g = by_key[(name, fam, "greedy")]
        assert s[q_pos:].tobytes() == np.frombuffer(g.stream, np.uint16)[qf.tables_of(g.stream)[1]:].tobytes()      # the body is untouched
        for k in range(12):
            for code in codes[k]:
                shape = "plain" if not code & 0x8000 else {2: "pair", 3: {12: "triple", 13: "quad"}.get(code >> 12, "run")}[code >> 14]
                shapes[policy].add(shape)
                if shape == "run" and policy == "runs":
                    run_lengths.add((code & 0xFF) + 4)
                    tails.add(((code >> 8) & 15) != ((code >> 12) & 1))
        if policy != "greedy" and codes != qf.tables_of(g.stream)[3]:
            differs[policy] += 1
    assert all(n > 0 for n in differs.values()), differs
    assert shapes["greedy"] == {"plain", "pair", "triple", "quad", "run"}
    assert shapes["plain"] == {"plain"} and "run" not in shapes["widest"] and shapes["widest"] >= {"pair", "triple", "quad"}
    assert {4, 255} <= run_lengths and tails == {True, False}


def test_oracle_and_reference_decode_every_stream_to_its_plane(oracle):
    ref = Reference() if Reference.available() else None
    t0 = time.perf_counter()
    n = 0
    for c in qf.cases(oracle):
        case = (c.plane_name, c.family, c.policy)
        assert np.array_equal(oracle.qdecode(c.stream), c.plane), case
        if ref is not None:
            assert np.array_equal(ref.qdecode(c.stream), c.plane), case
        n += 1
    print(f"{n} streams decoded by the oracle{' and the reference' if ref else ''} in {time.perf_counter() - t0:.1f} s")


def test_golden_hashes(oracle):
    """What the compiled reference said of these very streams (golden/make_foreign_q.py): lossless, so the planes' hash is
    the input planes'."""
    stored = qf.golden()
    groups = {}
    for c in qf.cases(oracle):
        groups.setdefault(f"{c.plane_name}/{c.family}", []).append(c)
    assert set(groups) == set(stored)
    for key, cs in groups.items():
        assert [c.policy for c in cs] == list(qf.POLICIES)
        assert sha(b"".join(c.stream for c in cs)) == stored[key]["streams_sha256"], key
        assert sha(b"".join(c.plane.tobytes() for c in cs)) == stored[key]["planes_sha256"], key
        assert sum(len(c.stream) for c in cs) == stored[key]["bytes"], key


def test_host_entropy_stage_codes_the_oracles_bytes_from_the_same_tables(pkg, oracle):
    """pkg.q_entropy_entries(level | symbol << 8, rows, hist=T): the product's scaling leaves T alone too, and its greedy
    writer and rANS pass give the oracle's stream."""
    for c in qf.cases(oracle):
        if c.policy != "greedy":
            continue
        plane, qd, y, _ = qf.models(oracle)[c.plane_name]
        words = (qd.astype(np.uint16) | (y.astype(np.uint16) << 8)).reshape(plane.shape)
        h = plane.shape[0]
        rows = list(range(1, h, max(1, h // 4)))
        stream, entries = pkg.q_entropy_entries(words, rows, hist=c.tables, cap_words=plane.size + qf.MAX_FRONT_WORDS + 2)
        assert stream == c.stream, (c.plane_name, c.family)
        assert len(entries) == len(rows)


def test_the_set_meets_its_conditions(oracle):
    """Conditions, not measurements: a frequency of 1 costs 15 bits, so the families meet them by construction."""
    reps = qf.replays(oracle)
    m = qf.models(oracle)
    widths = {name: v[0].shape[1] for name, v in m.items()}
    heights = {name: v[0].shape[0] for name, v in m.items()}
    for (name, fam), r in sorted(reps.items()):
        print(f"{name:18s} {fam:16s} front {r.front_words:4d} words, rows {min(r.row_words):6d} .. {max(r.row_words):6d} words of {widths[name]:5d} px, "
              f"f=1 {r.f1_share:5.3f}, arms {r.arm_counts}, longest step-over {r.longest_step_over:3d}, y=255 at level 11: {r.y255_at_level_11}")
    # (no pixel takes more than one word, every stream is consumed exactly to its last word: replay() asserts both)
    assert any(2 * max(r.row_words) >= 1.75 * widths[name] for (name, _), r in reps.items())
    assert any(2 * max(r.row_words) >= 1.75 * widths[name] for (name, _), r in reps.items() if widths[name] >= qf.WIDE_CACHED)
    assert any(r.front_words == qf.MAX_FRONT_WORDS == 3076 for r in reps.values())
    cs = qf.cases(oracle)
    assert any(len(c.stream) > out_capacity(*c.plane.shape) for c in cs)
    assert any(len(c.stream) > c.plane.size and c.plane.size > 2000 for c in cs)
    assert any(r.y255_at_level_11 > 0 for r in reps.values())
    for fam in ("far_pair", "far_pair_mirror"):
        r = reps[("flat_8x8", fam)]
        assert r.levels_used == [0]                                      # the far pair's level decides every pixel
    assert reps[("flat_8x8", "far_pair")].f1_share == 1.0 and reps[("flat_8x8", "far_pair_mirror")].f1_share == 0.0
    assert sum(reps[("flat_8x8", "far_pair")].row_words) >= 60 and sum(reps[("flat_8x8", "far_pair_mirror")].row_words) == 0
    # the search arms: at the coarse symbol, the one after, and stepped over -- in foreign streams too
    assert all(sum(r.arm_counts[k] for r in reps.values()) > 0 for k in range(3))
    assert max(r.longest_step_over for r in reps.values()) >= 100
    assert all(len(r.row_words) == heights[name] for (name, _), r in reps.items())


def test_serial_plan_answers_for_the_effort_0_decoder(pkg):
    """One LDS image for any number of streams; rows of 40000 pixels, the widest the suite decoded at effort 0 before, still
    fit next to its tables (3 rows of w + 8 rounded up to 16, in 160 KB less the 28680 bytes of tables and 256), rows of 46000
    do not.  There is no effort-0 model plan: the encoder's stages are the batch pipeline's."""
    lds = pkg.PLAN_ROWS_IN_LDS
    for images in (1, 256, 257, 1000):
        assert pkg.serial_plan(True, 0, images, 1) == lds and pkg.serial_plan(True, 0, images, qf.WIDE_CACHED) == lds
        assert pkg.serial_plan(True, 0, images, qf.WIDE_UNCACHED) == 0 and pkg.serial_plan(True, 0, images, 65535) == 0
    room = (160 * 1024 - 28680 - 256) & ~15
    widest = max(w for w in range(qf.WIDE_CACHED, qf.WIDE_UNCACHED) if 3 * ((w + 8 + 15) & ~15) + 4 <= room)
    assert pkg.serial_plan(True, 0, 1, widest) == lds and pkg.serial_plan(True, 0, 1, widest + 1) == 0
    assert pkg.serial_plan(True, 0, 1, 100, False) == lds                 # (whole_streams makes no difference to it)
    for bad in ((False, 0, 1, 100), (True, 0, 0, 100), (True, 0, 1, 0), (True, -1, 1, 100)):
        try:
            pkg.serial_plan(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)
