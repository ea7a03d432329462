"""CPU suite: the lane of the device rANS stage of effort 0 (csrc/q_rans.h) as the host runs it.  ``q_rans_host`` codes
with one lane that stops every ``symbols_per_launch`` symbols and resumes from its record; it must give the bytes of
``q_entropy_entries`` (which tests/test_oracle_q.py and tests/test_qindexed_batch_host.py hold to the reference), for
every resume point relative to a 256-word window.  The quotient routine is checked natively by tools/q_rans_check.cpp."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import qcoder_inputs as qi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (1, 2, 255, 256, 257, 4096, 0)                            # 0: everything in one launch

CASES = [("uniform_40x37", lambda: qi.uniform(40 * 37, 1), (40, 37)),
         ("uniform_255", lambda: qi.uniform(255, 2), (1, 255)),
         ("uniform_256", lambda: qi.uniform(256, 3), (256, 1)),
         ("uniform_257", lambda: qi.uniform(257, 4), (1, 257)),
         ("one_pixel", lambda: qi.uniform(1, 5), (1, 1)),
         ("f_one_3000", lambda: qi.f_one(3000, 6), (30, 100)),
         ("one_symbol_2570", lambda: qi.one_symbol(2570, 7), (10, 257)),
         ("skewed_5000", lambda: qi.uniform(5000, 8, levels=2, syms=3), (50, 100))]


@pytest.fixture(scope="module")
def expected(pkg):
    out = {}
    for name, make, shape in CASES:
        words, hist = make()
        out[name] = (words.reshape(shape), hist, pkg.q_entropy_entries(words.reshape(shape), (), hist)[0])
    return out


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_resumed_lane_gives_the_host_stage_bytes(pkg, expected, name, budget):
    words, hist, want = expected[name]
    assert want is not None
    assert pkg.q_rans_host(words, hist, budget) == want


def test_constructions_reach_what_they_claim(pkg, expected):
    """A guard on the INPUTS, not on the lane (it uses the host stage alone): f = 1 run: a word per step; f = 32767 run: no word at all; so the two streams differ in length by far more than
    their symbol counts do."""
    w1, h1, s1 = expected["f_one_3000"]
    w2, h2, s2 = expected["one_symbol_2570"]
    assert len(s1) // 2 > 1000 + 750                                 # every step of the two runs renormalised
    assert len(s2) // 2 < 2570 - 1285 + 64                            # the run of 1285 cost nothing


@pytest.mark.parametrize("name", ["uniform_40x37", "f_one_3000", "one_pixel"])
def test_capacity_exact_fits_and_one_word_less_does_not(pkg, expected, name):
    words, hist, want = expected[name]
    for budget in (0, 7, 256):
        assert pkg.q_rans_host(words, hist, budget, cap_words=len(want) // 2) == want
        assert pkg.q_rans_host(words, hist, budget, cap_words=len(want) // 2 - 1) is None
    assert pkg.q_rans_host(words, hist, 0, cap_words=0) is None


def test_refusals(pkg):
    words, hist = qi.uniform(64, 9)
    bad = words.copy()
    bad[10] = 12
    with pytest.raises(ValueError):
        pkg.q_rans_host(bad.reshape(8, 8), hist, 0)
    hole = hist.copy()
    hole[(int(words[3]) & 0xFF) * 256 + (int(words[3]) >> 8)] = 0
    with pytest.raises(ValueError):
        pkg.q_rans_host(words.reshape(8, 8), hole, 0)


def test_quotient_and_lane_natively(tmp_path):
    """tools/q_rans_check.cpp: the quotient routines on the self-test's operand set against 64-bit division, and the
    resumed lane against the plain pass, with its own main -- under the address and undefined-behaviour sanitizers where
    the host compiler has their runtimes, plainly (and saying so) where it has not: the checks themselves run either way."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler: the project does not build here either"
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if probe.returncode == 0 else []
    print("q_rans_check built", "with the address and undefined-behaviour sanitizers" if flags else "WITHOUT sanitizers: the host compiler lacks their runtimes")
    exe = str(tmp_path / "q_rans_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(ROOT, "tools", "q_rans_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "q_rans_check ok" in r.stdout
