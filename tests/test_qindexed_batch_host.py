"""Host side of the indexed effort-0 batch (nblic_amd_qencode_batch_indexed): the entropy stage that reports the coder in
front of entry rows (nblic_amd_debug_q_entropy, no device), and what the Python wrapper refuses before it touches the
library.

The yardstick is written here from the format alone (QNBLIC: histograms scaled to 2^15, one 32-bit rANS state, 16-bit
words, the pass run last pixel first and its words reversed): ``ref_pass`` is the encoder's pass, which says for every pixel
whether coding it emitted a word -- a property of the INPUT -- and ``decode_from`` is a decoder that reads the produced
stream from a reported (state, words emitted) and must find exactly the symbols of the pixels from the entry row on."""
import bisect
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM, WORD = 15, 16


def read_hist(s, p):
    """One histogram in QNBLIC's compact 16-bit code (five shapes), from word p of s.  Returns (256 frequencies, next p)."""
    h, covered = [], 0

    def put(v):
        nonlocal covered
        if len(h) < 256:
            h.append(v)
            covered += v

    while len(h) < 256 and covered < (1 << NORM):
        code = int(s[p])
        p += 1
        if not code & 0x8000:
            put(code)
        elif code >> 14 == 2:
            put((code >> 7) & 0x7F), put(code & 0x7F)
        elif code >> 12 == 12:
            put((code >> 8) & 15), put((code >> 4) & 15), put(code & 15)
        elif code >> 12 == 13:
            put((code >> 9) & 7), put((code >> 6) & 7), put((code >> 3) & 7), put(code & 7)
        else:
            v, tail = (code >> 12) & 1, (code >> 8) & 15
            for _ in range((code & 0xFF) + 4):
                put(v)
            if tail != v:
                put(tail)
    return h + [0] * (256 - len(h)), p


def tables_of(stream):
    """(words, index of the first rANS word, freq[12][256], start[12][256]) of a QNBLIC stream."""
    s = np.frombuffer(stream, np.uint16)
    assert bytes(stream[:4]) == b"Q0.2"
    p, freq, start = 4, [], []
    for _ in range(12):
        f, p = read_hist(s, p)
        assert sum(f) == 1 << NORM
        freq.append(f)
        start.append([0] + list(np.cumsum(f)[:-1]))
    return s, p, freq, start


def normalise(h):
    """QNBLIC's scaling of one histogram to a sum of 2^15 (IEEE doubles, truncating conversion)."""
    h = [int(v) for v in h]
    used = [s for s in range(256) if h[s]]
    if len(used) < 2:                                                     # no symbol: 0 stands in; the one symbol's neighbour gets a slot
        last = used[0] if used else 0
        out = [0] * 256
        out[last], out[(last + 1) & 255] = (1 << NORM) - 1, 1
        return out
    scale = (1.0 * (1 << NORM)) / sum(h)
    out = [max(int(0.49 + scale * v), 1) if v else 0 for v in h]
    total, s = sum(out), 0
    while total > 1 << NORM:
        if out[s] > 1:
            out[s] -= 1
            total -= 1
        s = (s + 1) & 255
    s = 0
    while total < 1 << NORM:
        if out[s] > 0:
            out[s] += 1
            total += 1
        s = (s + 1) & 255
    return out


def ref_pass(words):
    """The encoder's rANS pass over level | symbol << 8 words, last pixel first.  Returns (the rANS words in stream order,
    emitted[t] = coding pixel t emitted a renormalisation word)."""
    flat = [int(v) for v in np.asarray(words).ravel()]
    hist = np.bincount(np.array([(e & 0xFF) * 256 + (e >> 8) for e in flat]), minlength=12 * 256).reshape(12, 256)
    freq = [normalise(hist[k]) for k in range(12)]
    start = [[0] + list(np.cumsum(f)[:-1]) for f in freq]
    x, out, emitted = 1 << WORD, [], [False] * len(flat)
    for t in range(len(flat) - 1, -1, -1):
        e = flat[t]
        f, s0 = freq[e & 0xFF][e >> 8], int(start[e & 0xFF][e >> 8])
        if x // f > (1 << (2 * WORD - NORM)) - 1:
            out.append(x & 0xFFFF)
            x >>= WORD
            emitted[t] = True
        x = (x % f) + ((x // f) << NORM) + s0
    out += [x & 0xFFFF, x >> WORD]
    return out[::-1], emitted


def decode_from(stream, words, row, state, words_emitted):
    """Decodes the pixels from `row` on out of `stream`, starting from the coder an entry names.  Returns the decoded
    level | symbol << 8 words, having checked that the stream ends where the last pixel ends."""
    s, q_pos, freq, start = tables_of(stream)
    h, w = words.shape
    total = len(s) - q_pos - 2                                            # renormalisation words of the whole pass
    assert 0 <= words_emitted <= total
    at = q_pos + 2 + (total - words_emitted)
    x, got = state, []
    levels = (np.asarray(words).ravel() & 0xFF)[row * w:]
    for lv in levels:
        low = x & ((1 << NORM) - 1)
        y = bisect.bisect_right(start[lv], low) - 1
        while freq[lv][y] == 0:                                           # (symbols without slots share a start)
            y -= 1
        assert start[lv][y] <= low < start[lv][y] + freq[lv][y]
        x = (x >> NORM) * freq[lv][y] + low - int(start[lv][y])
        if x < 1 << WORD:
            x = (x << WORD) | int(s[at])
            at += 1
        got.append(int(lv) | (y << 8))
    assert at == len(s), (row, at, len(s))
    assert x == 1 << WORD                                                 # where the encoder's pass began
    return np.array(got, np.uint16)


def uniform_words(h, w, seed, levels=12, syms=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint16) | (rng.integers(0, syms, (h, w)).astype(np.uint16) << 8))


def check_entries(pkg, words, rows):
    stream, entries = pkg.q_entropy_entries(words, rows)
    assert stream == pkg.q_entropy_entries(words)[0]                      # the entry rows do not show in the stream
    h, w = words.shape
    s, q_pos, _, _ = tables_of(stream)
    assert (int(s[2]), int(s[3])) == (h, w)
    want_rans, emitted = ref_pass(words)
    assert [int(v) for v in s[q_pos:]] == want_rans
    assert len(entries) == len(rows)
    for r, (state, n_words) in zip(rows, entries):
        assert n_words == sum(emitted[r * w:]), r                         # the word pixel r w itself cost is counted
        assert np.array_equal(decode_from(stream, words, r, state, n_words), words.ravel()[r * w:]), r
    first = (int(s[q_pos]) << 16) | int(s[q_pos + 1])                     # and the decoder's own start: row 0, nothing consumed
    assert np.array_equal(decode_from(stream, words, 0, first, len(s) - q_pos - 2), words.ravel())
    return emitted


def test_reported_states_decode_the_rest_of_the_image(pkg):
    """40 x 37 words over 12 levels and 256 symbols, an entry in front of every row: among the entry rows are some whose first
    pixel cost a renormalisation word and some whose first pixel did not -- asserted from the input's own pass."""
    words = uniform_words(40, 37, 20)
    rows = list(range(1, 40))
    _, emitted = ref_pass(words)
    at_row_start = [emitted[r * 37] for r in rows]
    assert any(at_row_start) and not all(at_row_start)
    assert check_entries(pkg, words, rows) == emitted
    check_entries(pkg, words, [5, 10, 15, 20, 25, 30, 35])
    check_entries(pkg, words, [39])


def test_levels_with_one_used_symbol_or_none(pkg):
    """Levels 0 .. 5 use one symbol each (255 among them: its partner wraps to 0), levels 6 .. 11 none."""
    t = np.arange(17 * 28)
    lv = (t % 6).astype(np.uint16)
    words = (lv | (np.where(lv == 5, 255, 40 * lv).astype(np.uint16) << 8)).reshape(17, 28)
    check_entries(pkg, words, list(range(1, 17)))


def test_skewed_and_degenerate_geometries(pkg):
    check_entries(pkg, uniform_words(23, 150, 3, syms=3), [7, 14, 21])        # few words are emitted at all
    check_entries(pkg, uniform_words(9, 1, 4), list(range(1, 9)))
    check_entries(pkg, uniform_words(1, 9, 5), [])


def test_no_entry_rows_is_the_plain_stage(pkg):
    """An empty list: the plain entropy stage's stream, and the capacity is enforced with entry rows as without."""
    words = uniform_words(40, 37, 20)
    stream, entries = pkg.q_entropy_entries(words, [])
    assert entries == []
    s, q_pos, _, _ = tables_of(stream)
    assert [int(v) for v in s[q_pos:]] == ref_pass(words)[0]
    short, _ = pkg.q_entropy_entries(words, [5], cap_words=len(s) - 1)     # one word short: refused, not overrun
    assert short is None
    exact, e = pkg.q_entropy_entries(words, [5], cap_words=len(s))
    assert exact == stream and len(e) == 1


def test_refusals(pkg):
    words = uniform_words(5, 4, 6, levels=2, syms=2)
    for rows in ([0], [5], [3, 3], [4, 2], [-1]):
        with pytest.raises(ValueError):
            pkg.q_entropy_entries(words, rows)
    hist = np.bincount(((words & 0xFF).astype(np.int64) * 256 + (words >> 8)).ravel(), minlength=12 * 256)
    bad = words.copy()
    bad[1, 3] = 1 | (9 << 8)                                              # a symbol the histogram does not count
    with pytest.raises(ValueError):
        pkg.q_entropy_entries(bad, [2], hist=hist)
    bad[1, 3] = 12                                                        # a level above 11
    with pytest.raises(ValueError):
        pkg.q_entropy_entries(bad, [2], hist=hist)


class NoLibrary:
    """Stands where a Context would: any reach for the library fails the test."""
    @property
    def lib(self):
        raise AssertionError("the wrapper touched the library")
    handle = None


def test_wrapper_refuses_before_touching_the_library(pkg):
    imgs = [np.zeros((4, 5), np.uint8)] * 3
    with pytest.raises(ValueError):
        pkg.Context.qencode_batch_indexed(NoLibrary(), imgs, -1)
    with pytest.raises(ValueError):
        pkg.Context.qencode_batch_indexed(NoLibrary(), imgs, [2, -3, 2])
    with pytest.raises(ValueError):
        pkg.Context.qencode_batch_indexed(NoLibrary(), imgs, [2, 2])
    with pytest.raises(ValueError):
        pkg.Context.qencode_indexed_ptrs(NoLibrary(), [1, 2, 3], [(4, 5)] * 3, False, [1, 1, 1, 1])


def test_standalone_check_under_sanitizers(tmp_path):
    """tools/q_entropy_check.cpp: q_entropy.cpp alone, with its own main, under the address and undefined-behaviour
    sanitizers (nothing of it is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler: the project does not build here either"
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the host compiler lacks the sanitizer runtimes")
    exe = str(tmp_path / "q_entropy_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "q_entropy_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "q_entropy_check ok" in r.stdout
