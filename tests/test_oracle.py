"""CPU suite: pins the oracle (our CPU restatement) to the reference's outputs.

  * every committed golden stream (generated from the compiled reference by
    tests/golden/make_golden.py) must be reproduced byte for byte, and must decode back;
  * when oracle/_ref is present the oracle is also compared live on further shapes;
  * the staged (key-partitioned) -e1 pipeline must equal the fused engine -- the proof that
    per-key replay is exact.
"""
import hashlib

import numpy as np
import pytest

import inputs


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def test_syn1_python_equals_c():
    from oracle.oracle import syn1
    for (h, w, seed) in [(5, 7, 1), (64, 64, 1), (33, 129, 9)]:
        assert np.array_equal(inputs.syn1(h, w, seed), syn1(h, w, seed))


@pytest.mark.parametrize("content", inputs.CONTENTS)
def test_oracle_reproduces_golden_streams(oracle, golden, content):
    manifest, streams = golden
    for (h, w) in inputs.SMALL_SHAPES:
        img = inputs.make(content, h, w)
        for near, effort in inputs.PARAM_CLASSES:
            cid = inputs.case_id(content, h, w, near, effort)
            want = streams[cid].tobytes()
            got, rec, n_out, e_out, _ = oracle.encode(img, near, effort)
            assert got == want, cid
            m = manifest["small"][cid]
            assert (n_out, e_out) == (m["near_out"], m["effort_out"]), cid
            assert sha(rec.tobytes()) == m["recon_sha256"], cid
            assert int(np.abs(rec.astype(int) - img.astype(int)).max()) <= n_out, cid
            dec = oracle.decode(want)
            assert dec is not None and np.array_equal(dec[0], rec), cid
            assert dec[1:] == (n_out, e_out), cid


def test_known_answer_1x1(oracle):
    # 1x1 image, pixel 77, -n0 -e1 -> 23 bytes
    s = oracle.encode(np.array([[77]], np.uint8), 0, 1)[0]
    assert s.hex() == "4e424c4943302e33010001000100030100000320000000"


@pytest.mark.parametrize("key", ["syn1s1_512x512_n0_e1", "syn1s2_512x512_n0_e1", "syn1s1_512x512_n2_e1",
                                 "syn1s1_256x256_n0_e2", "syn1s1_256x256_n0_e3", "syn1s1_256x256_n2_e2",
                                 "syn1s3_768x512_n0_e1", "syn1s1_1024x1024_n0_e1"])
def test_oracle_matches_large_hashes(oracle, golden, key):
    from oracle.oracle import syn1
    manifest, _ = golden
    m = manifest["large"][key]
    name, dims, n, e = key.split("_")
    seed = int(name[5:]); h, w = map(int, dims.split("x"))
    img = syn1(h, w, seed)
    assert sha(img.tobytes()) == m["input_sha256"]
    s, rec, _, _, _ = oracle.encode(img, int(n[1:]), int(e[1:]))
    assert len(s) == m["len"] and sha(s) == m["sha256"]
    assert sha(rec.tobytes()) == m["recon_sha256"]


def test_survey_appendix_b_constants(golden):
    # the survey's independently measured hashes agree with the regenerated manifest
    manifest, _ = golden
    L = manifest["large"]
    assert L["syn1s1_512x512_n0_e1"]["sha256"].startswith("dadb401b98cd2c62") and L["syn1s1_512x512_n0_e1"]["len"] == 139965
    assert L["syn1s1_4096x4096_n0_e1"]["sha256"].startswith("77d18ede1c1aa384") and L["syn1s1_4096x4096_n0_e1"]["len"] == 8900446
    assert L["syn1s1_512x512_q0"]["sha256"].startswith("50fdb1a0a3cac171")


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 5), (40, 37), (96, 128), (64, 200)])
def test_staged_equals_fused(oracle, shape):
    h, w = shape
    for content in ("noise", "syn1", "checker", "const"):
        img = inputs.make(content, h, w)
        fused = oracle.encode(img, 0, 1)[0]
        staged, n_ev = oracle.encode_staged(img)
        assert staged == fused, (content, shape)
        st = oracle.stages(img)
        assert len(st["prob"]) == n_ev and int(st["ev_count"].sum()) == n_ev
        assert fused[16:] == st["body"]


def test_limits_and_clamps(oracle):
    img = inputs.make("syn1", 8, 8)
    s9 = oracle.encode(img, 9, 1)[0]
    s12, _, n_out, e_out, _ = oracle.encode(img, 12, 0)
    assert s9 == s12 and (n_out, e_out) == (9, 1)           # near clamps to 9, effort 0 -> 1 (NBLIC.c:768-770)
    assert oracle.decode(b"NOTNBLIC" + bytes(32)) is None
    # pixel-count limit (NBLIC.h:31): 10001 x 10000 is refused before any pixel is touched
    big = np.zeros((1, 1), np.uint8)
    from oracle.oracle import _ptr  # noqa
    import ctypes as C
    out = np.empty(64, np.uint8)
    n, e = C.c_int(0), C.c_int(1)
    assert oracle.lib.orc_nblic_encode(_ptr(out), _ptr(big), 10001, 10000, C.byref(n), C.byref(e), 0, None) == -1


def test_oracle_vs_live_reference(oracle):
    """Random shapes and parameters: the reference's streams and decodes stored in tests/golden/reference_fixtures.*
    (make_fixtures.py), and the compiled reference itself wherever oracle/_ref was built."""
    from oracle.oracle import Reference
    meta, stored = inputs.fixtures()
    reference = Reference() if Reference.available() else None
    for k, (img, near, effort) in enumerate(inputs.random_cases()):
        h, w = img.shape
        a = oracle.encode(img, near, effort)
        assert a[0] == stored[f"case_{k}"].tobytes(), (h, w, near, effort)
        assert sha(a[1].tobytes()) == meta["case_recon_sha256"][k], (h, w, near, effort)      # the reference decodes to it
        if reference is not None:
            b = reference.encode(img, near, effort)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), (h, w, near, effort)
            d = reference.decode(a[0])
            assert d is not None and np.array_equal(d[0], a[1])


def test_kstep_entry_point_with_the_paired_step_is_encode(oracle):
    """orc_nblic_encode_kstep given the k_step the encoders derive: encode's bytes and reconstruction; what a decoder's
    header check refuses is refused before anything is coded."""
    for img, near, effort in inputs.random_cases():
        a = oracle.encode(img, near, effort)
        b = oracle.encode(img, near, effort, k_step=inputs.paired_k_step(near))
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and b[2:4] == (near, effort), (img.shape, near, effort)
    img = inputs.make("syn1", 8, 8)
    for near, k_step, effort in ((0, 2, 1), (0, 17, 1), (-1, 3, 1), (10, 16, 1), (0, 3, 0), (0, 3, 4)):
        s, rec, *_ = oracle.encode(img, near, effort, k_step=k_step)
        assert s is None and np.array_equal(rec, img), (near, k_step, effort)


def test_foreign_planes_reach_every_walk_regime(oracle):
    """The coverage condition of the foreign case set (inputs.foreign_planes), from the oracle's own counters, effort 1,
    lossless: at every k_step symbols whose prefix outlasts the decoder's lanes, every level as the starting level,
    every suffix length 0..k_max, escalations to the next tree wherever there is one (k_max = 0 at k_step 16: a valid
    symbol cannot leave its tree)."""
    planes = inputs.foreign_planes()
    assert all(p.size <= 2700 for p in planes.values())
    for k_step in range(3, 17):
        k_max = 15 // k_step
        qu, k, esc, beyond = [0] * 16, [0] * 8, 0, 0
        for plane in planes.values():
            assert oracle.encode(plane, 0, 1, k_step=k_step)[0] is not None
            c = oracle.walk_coverage()
            assert sum(c["qu"]) == sum(c["k"]) == plane.size
            qu = [a + b for a, b in zip(qu, c["qu"])]
            k = [a + b for a, b in zip(k, c["k"])]
            esc += c["escalations"]
            beyond += c["beyond_lanes"]
        print(f"k_step {k_step}: beyond_lanes {beyond}, escalations {esc}, per suffix length {k[:k_max + 1]}, least-used level {min(qu)}")
        assert beyond > 0, k_step
        assert all(v > 0 for v in qu), (k_step, qu)
        assert all(v > 0 for v in k[:k_max + 1]) and not any(k[k_max + 1:]), (k_step, k)
        assert (esc > 0) if k_step <= 15 else (esc == 0), (k_step, esc)


@pytest.mark.parametrize("name", ["kodak05", "blocks", "noise", "syn1", "spikes", "checker"])
def test_foreign_streams_round_trip_and_reference_decodes_them(oracle, name):
    """All 420 (near, k_step, effort) streams of one foreign plane: the oracle decodes each to its own reconstruction,
    within near of the plane; their concatenation has the stored hash, and the stored hash of the planes the compiled
    reference decoded them to (tests/golden/make_foreign.py) is the hash of the oracle's reconstructions.  Wherever
    oracle/_ref was built the reference decodes every stream again, live."""
    from oracle.oracle import Reference
    plane = inputs.foreign_planes()[name]
    stored = inputs.foreign_golden()
    reference = Reference() if Reference.available() else None
    for effort in inputs.FOREIGN_EFFORTS:
        hs, hp = hashlib.sha256(), hashlib.sha256()
        for (near, k_step, _), s, rec in inputs.foreign_streams(oracle, plane, (effort,)):
            case = (name, near, k_step, effort)
            assert s is not None and (s[13], s[14], s[15]) == (near, k_step, effort), case
            assert int(np.abs(rec.astype(int) - plane.astype(int)).max()) <= near, case
            d = oracle.decode(s)
            assert d is not None and np.array_equal(d[0], rec) and d[1:] == (near, effort), case
            if reference is not None:
                r = reference.decode(s)
                assert r is not None and np.array_equal(r[0], rec) and r[1:] == (near, effort), case
            hs.update(s)
            hp.update(rec.tobytes())
        want = stored[f"{name}_e{effort}"]
        assert hs.hexdigest() == want["streams_sha256"], (name, effort)
        assert hp.hexdigest() == want["planes_sha256"], (name, effort)


def test_oracle_on_kodak_matches_reference_and_readme(oracle, golden):
    """BASELINE config 3 content.  The 24 Kodak BMPs are third-party files and are read in place
    (container only); the manifest holds the compiled reference's length + SHA-256 per image, whose
    totals reproduce the reference README's 4.146 bpp (-e1) and 4.227 bpp (-e0).  A 64x96 crop of
    every image is stored with the reference's streams of it (tests/golden/reference_fixtures.*)."""
    import os
    manifest, _ = golden
    k = manifest["kodak_e1"]
    assert len(k) == 24
    total_e1 = sum(v["len"] for v in k.values()); total_e0 = sum(v["q_len"] for v in k.values())
    px = sum(v["shape"][0] * v["shape"][1] for v in k.values())
    assert (total_e1, total_e0, px) == (4891174, 4985986, 9437184)
    assert round(8 * total_e1 / px, 3) == 4.146 and round(8 * total_e0 / px, 3) == 4.227   # README.md:256-257
    meta, stored = inputs.fixtures()
    assert sorted(meta["kodak_crops"]) == sorted(k)
    for name, crop in zip(sorted(meta["kodak_crops"]), stored["kodak_crops"]):     # the crops, everywhere
        want = meta["kodak_crops"][name]
        s = oracle.encode(crop, 0, 1)[0]
        assert (len(s), sha(s)) == (want["len"], want["sha256"]), name
        q = oracle.qencode(crop)
        assert (len(q), sha(q)) == (want["q_len"], want["q_sha256"]), name
    if not os.path.isdir(inputs.KODAK_DIR):                               # the whole images where they can be read
        return
    for name in sorted(k):                                                # all 24 images
        img = inputs.read_gray_bmp(os.path.join(inputs.KODAK_DIR, name))
        assert sha(img.tobytes()) == k[name]["input_sha256"]
        s = oracle.encode(img, 0, 1)[0]
        assert (len(s), sha(s)) == (k[name]["len"], k[name]["sha256"]), name
        q = oracle.qencode(img)
        assert (len(q), sha(q)) == (k[name]["q_len"], k[name]["q_sha256"]), name


@pytest.mark.parametrize("name", ["kodak05", "blocks", "noise", "syn1", "spikes", "checker"])
def test_staged_entropy_front_equals_fused_in_every_mode(oracle, name):
    """The decomposition test_staged_equals_fused proves for lossless -e1, for the modes whose model stage is a serial
    chain: the fused encoder's own records per pixel (orc_nblic_trace) through the general S3 (one re-mapper key at a
    time) -> general S4 -> S5 (one counter at a time) -> S6 give the fused stream's body, at near 0..9 x efforts 1..3
    with the k_step the encoders pair with near."""
    plane = inputs.foreign_planes()[name]
    for effort in (1, 2, 3):
        for near in range(10):
            case = (name, near, effort)
            s, rec, *_ = oracle.encode(plane, near, effort)
            t = oracle.trace(plane, near, effort)
            assert t["stream"] == s and np.array_equal(t["recon"], rec), case
            assert s[14] == inputs.paired_k_step(near), case
            assert np.array_equal(t["adr"] >> 8, t["qu"] >> 1) and int(t["qw"].max()) <= 16, case      # what pack_s1 relies on
            assert int(np.abs(t["qv"].astype(int) - t["qu"].astype(int)).max()) <= 1, case
            y, z = oracle.s3_near(plane, t["px"], t["sign"], near)
            assert np.array_equal(y, t["y"]) and np.array_equal(z, t["z"]), case
            ev = oracle.s4_kstep(s[14], t["qu"], t["qv"], t["qw"], z)
            assert np.array_equal(ev["cnt"], t["bins"]), case
            prob = oracle.s5(ev["cu"], ev["cv"], ev["qw"], ev["bin"])
            assert oracle.s6(prob, ev["bin"]) == s[16:], case


def test_general_stages_at_the_lossless_constants_are_the_lossless_stages(oracle):
    """orc_s3_near at near 0 and orc_s4_kstep at k_step 3 are orc_s3 and orc_s4."""
    for plane in inputs.foreign_planes().values():
        st = oracle.stages(plane)
        y, z = oracle.s3_near(plane, st["px"], st["sign"], 0)
        assert np.array_equal(y, st["y"]) and np.array_equal(z, st["z"])
        ev = oracle.s4_kstep(3, st["qu"], st["qv"], st["qw"], z)
        for a, b in (("cnt", "ev_count"), ("cu", "cu"), ("cv", "cv"), ("qw", "ev_qw"), ("bin", "ev_bin")):
            assert np.array_equal(ev[a], st[b]), a
        t = oracle.trace(plane, 0, 1)                        # and the fused engine's records at -n0 -e1 are S1 / S2's
        for k in ("px0", "adr", "qu", "qv", "qw", "px", "sign", "y", "z"):
            assert np.array_equal(t[k], st[k]), k
