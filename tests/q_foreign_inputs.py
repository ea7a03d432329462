"""Valid QNBLIC (effort 0) streams that no encoder writes, shared by test_q_foreign_host.py, test_q_foreign_streams.py and
golden/make_foreign_q.py.

A QNBLIC stream carries the coder's model itself: twelve 256-entry frequency tables in its front matter, each summing to
2^15.  Every encoder writes the scaling (QNBLIC.c:308-358) of the plane's true counts in the greedy histogram code
(QNBLIC.c:362-459): positive frequencies only on symbols that occur, a few hundred bytes of front matter, a body well
under a byte per pixel.  A decoder must take ANY tables the format allows.  Here they are made from the format alone:

* The scaling has fixed points: a table that sums to 2^15 with at least two nonzero entries, none above 32767, comes back
  unchanged (the scale is 1.0 and (uint32_t)(0.49 + v) == v).  The oracle's entropy stage handed such tables in place of
  the counts (Oracle.qencode_tables) therefore writes a stream that carries exactly them.  FAMILIES are such tables, each
  a function of the plane's true counts so that every coded symbol keeps a nonzero frequency.
* recode() rewrites the front matter of a stream -- the same tables in other code shapes (POLICIES) -- and leaves the body
  alone.
* replay() is a plain rANS decoder over the known (level, symbol) sequence of the plane: it checks that the stream is
  consumed exactly to its last word and reports what the stream puts under load.

QNBLIC is lossless: what every decoder must return is the plane the stream was made from.
"""
import bisect
import json
import os
import time
from collections import namedtuple

import numpy as np

import inputs

NORM_BITS, WORD = 15, 16
NORM = 1 << NORM_BITS
LEVELS, SYMS = 12, 256
MAX_FRONT_WORDS = 4 + LEVELS * SYMS            # the header and one code per symbol: no front matter is longer
WIDE_CACHED, WIDE_UNCACHED = 40000, 46000      # rows of 40000 are the widest the suite decodes at effort 0 and still fit in LDS; 46000 do not


# ---- planes --------------------------------------------------------------------------------------------------------
def planes():
    """name -> plane.  The flat plane is 128 throughout: the first prediction is 128 too, so every pixel is symbol 0 at
    level 0 and a far_pair table on that level decides every pixel of the stream."""
    from oracle.oracle import syn1 as c_syn1
    return {
        "noise_17x13": inputs.noise(17, 13),
        "syn1_64x64": inputs.syn1(64, 64),
        "spikes_32x48": inputs.spikes(),
        "checker_33x70": inputs.make("checker", 33, 70),
        "flat_8x8": np.full((8, 8), 128, np.uint8),
        "noise_1x1": inputs.noise(1, 1),
        "noise_1x300": inputs.noise(1, 300),
        "syn1_2x256": inputs.syn1(2, 256),
        f"syn1_3x{WIDE_CACHED}": c_syn1(3, WIDE_CACHED, 3),
        f"syn1_3x{WIDE_UNCACHED}": c_syn1(3, WIDE_UNCACHED, 3),
    }


# ---- table families: 12 x 256 counts -> 12 x 256 frequencies, every level a fixed point of the scaling -----------------
def _ones_on(counts, s):
    t = np.ones((LEVELS, SYMS), np.uint32)
    t[:, s] = NORM - (SYMS - 1)
    return t


def _second_entry(row, keep):
    """A level must hold two nonzero entries (a single one is rewritten by the scaling): one slot moves from `keep`,
    the level's largest entry, to its neighbour."""
    if np.count_nonzero(row) < 2:
        row[keep] -= 1
        row[(keep + 1) % SYMS] += 1


def _sparse_level(c, level):
    """f = 1 on the symbols that occur; the rest of the 2^15 slots on a symbol that does not occur -- the lowest such on an
    even level (the coded symbols above it sit in the last slots), the highest on an odd one (they all sit in the first
    slots, behind one coarse entry) -- or on symbol 255 when all 256 occur."""
    occ = c > 0
    row = occ.astype(np.uint32)
    free = np.flatnonzero(~occ)
    r = 255 if free.size == 0 else int(free[0] if level % 2 == 0 else free[-1])
    row[r] += NORM - int(occ.sum())
    _second_entry(row, r)
    return row


def _far_pair_level(c, level, mirror):
    """A level with at most one occurring symbol s: {s: 1, s + 128: 32767}, or mirrored {s: 32767, s + 128: 1}.  Any other
    level gets the sparse table."""
    used = np.flatnonzero(c)
    if used.size > 1:
        return _sparse_level(c, level)
    s = int(used[0]) if used.size else 0
    row = np.zeros(SYMS, np.uint32)
    row[s], row[(s + 128) % SYMS] = (NORM - 1, 1) if mirror else (1, NORM - 1)
    return row


def _smoothed_level(c):
    from oracle.oracle import Oracle
    return Oracle().q_norm_hist(c.astype(np.uint32) + 1)


def _per_level(fn):
    return lambda counts: np.stack([fn(counts[k], k) for k in range(LEVELS)]).astype(np.uint32)


def _rotated(counts):
    """Family k % 5 on level k: one stream mixes them."""
    rows = []
    for k in range(LEVELS):
        c = counts[k]
        rows.append([_ones_on(counts, 254)[k], _sparse_level(c, k), np.full(SYMS, NORM // SYMS, np.uint32), _smoothed_level(c),
                     _far_pair_level(c, k, k % 2 == 1)][k % 5])
    return np.stack(rows).astype(np.uint32)


FAMILIES = {
    "ones_on_0": lambda counts: _ones_on(counts, 0),
    "ones_on_128": lambda counts: _ones_on(counts, 128),
    "ones_on_254": lambda counts: _ones_on(counts, 254),
    "ones_on_255": lambda counts: _ones_on(counts, 255),
    "sparse": _per_level(_sparse_level),
    "uniform": lambda counts: np.full((LEVELS, SYMS), NORM // SYMS, np.uint32),
    "smoothed": _per_level(lambda c, k: _smoothed_level(c)),
    "rotated": _rotated,
    "far_pair": _per_level(lambda c, k: _far_pair_level(c, k, False)),
    "far_pair_mirror": _per_level(lambda c, k: _far_pair_level(c, k, True)),
}
FLAT_ONLY = ("far_pair", "far_pair_mirror")


def families_of(plane_name):
    return [f for f in FAMILIES if f not in FLAT_ONLY or plane_name.startswith("flat")]


# ---- the histogram code (QNBLIC.c:362-459), from the format -----------------------------------------------------------
def read_hist(s, p):
    """One histogram from word p of s, the way the reference reads it: it stops when 256 symbols are placed or the
    covered sum reaches 2^15.  Returns (256 frequencies, next p, the codes read).  A code that places a symbol past 255
    is an error here (the reference would write behind its table)."""
    h, covered, p0 = [], 0, p
    while len(h) < SYMS and covered < NORM:
        code = int(s[p])
        p += 1
        if not code & 0x8000:
            vals = [code]
        elif code >> 14 == 2:
            vals = [(code >> 7) & 0x7F, code & 0x7F]
        elif code >> 12 == 12:
            vals = [(code >> 8) & 15, (code >> 4) & 15, code & 15]
        elif code >> 12 == 13:
            vals = [(code >> 9) & 7, (code >> 6) & 7, (code >> 3) & 7, code & 7]
        else:
            v, tail = (code >> 12) & 1, (code >> 8) & 15
            vals = [v] * ((code & 0xFF) + 4) + ([tail] if tail != v else [])
        h += vals
        covered += sum(vals)
        assert len(h) <= SYMS, "a histogram code places a symbol past 255"
    return h + [0] * (SYMS - len(h)), p, [int(v) for v in s[p0:p]]


def tables_of(stream):
    """(words, index of the first rANS word, 12 x 256 frequencies, the codes of every level) of a QNBLIC stream."""
    s = np.frombuffer(stream, np.uint16)
    assert bytes(stream[:4]) == b"Q0.2"
    p, freq, codes = 4, [], []
    for _ in range(LEVELS):
        f, p, c = read_hist(s, p)
        assert sum(f) == NORM
        freq.append(f)
        codes.append(c)
    return s, p, np.array(freq, np.uint32), codes


def _plain(h, i):
    return h[i], 1


def _grouped(h, i):
    """The widest non-run code at symbol i: a quad, a triple, a pair, a plain value.  Never past symbol 255."""
    if i + 3 < SYMS and max(h[i:i + 4]) <= 7:
        return 0xD000 | (h[i] << 9) | (h[i + 1] << 6) | (h[i + 2] << 3) | h[i + 3], 4
    if i + 2 < SYMS and max(h[i:i + 3]) <= 15:
        return 0xC000 | (h[i] << 8) | (h[i + 1] << 4) | h[i + 2], 3
    if i + 1 < SYMS and max(h[i:i + 2]) <= 127:
        return 0x8000 | (h[i] << 7) | h[i + 1], 2
    return _plain(h, i)


RUN_PIECES = (259, 4, 9, 5, 130, 6)              # 259 is the longest run the code can name; a table's longest is 255


def code_hist(h, policy):
    """The codes of one 256-entry table under a policy; they end where the reader stops.
    plain   one 15-bit code per symbol;
    widest  quads, then triples, then pairs wherever the values allow, and no run codes: the greedy writer's order
            with its first choice last;
    runs    every run of 0s or 1s of four and more cut into pieces of RUN_PIECES (4 .. 259) symbols, the run's last piece
            with the tail nibble on every other run and without it on the rest; what is left over in the widest code."""
    h = [int(v) for v in h]
    out, i, covered, k_piece, k_run = [], 0, 0, 0, 0
    while i < SYMS and covered < NORM:
        if policy == "plain":
            code, n = _plain(h, i)
        elif policy == "widest":
            code, n = _grouped(h, i)
        else:
            assert policy == "runs"
            j = i
            while j < SYMS and h[j] == h[i]:
                j += 1
            if h[i] <= 1 and j - i >= 4:
                v = h[i]
                n = min(RUN_PIECES[k_piece % len(RUN_PIECES)], j - i)
                k_piece += 1
                tail = v                                                 # tail == v: no tail
                if i + n == j:                                           # the run's last piece
                    if j < SYMS and h[j] <= 15 and k_run % 2 == 0:
                        tail, n = h[j], n + 1
                    k_run += 1
                code = 0xE000 | (v << 12) | (tail << 8) | (n - (tail != v) - 4)
            else:
                code, n = _grouped(h, i)
        out.append(code)
        covered += sum(h[i:i + n])
        i += n
    return out


POLICIES = ("greedy", "plain", "widest", "runs")


def recode(stream, policy):
    """The stream with the histogram codes of the same tables written under `policy`; header and body as they are."""
    if policy == "greedy":
        return stream
    s, q_pos, freq, _ = tables_of(stream)
    front = [c for k in range(LEVELS) for c in code_hist(freq[k], policy)]
    out = bytes(stream[:8]) + np.array(front, np.uint16).tobytes() + s[q_pos:].tobytes()
    _, q2, freq2, _ = tables_of(out)
    assert np.array_equal(freq2, freq) and q2 == 4 + len(front)
    return out


# ---- a plain replay of the decoder's entropy side ----------------------------------------------------------------------
Replay = namedtuple("Replay", "front_words row_words f1_share arm_counts longest_step_over y255_at_level_11 levels_used")


def replay(stream, h, w, qd, y):
    """Decodes the rANS words of `stream` along the known (level, symbol) sequence.  Asserts that every state names the
    symbol the plane has there, that a pixel takes at most one word, and that the stream ends exactly where the last
    pixel ends, on the state the encoder began with.  Reports
      front_words        16-bit words in front of the rANS state
      row_words          words consumed per row (row 0 without the two of the initial state)
      f1_share           share of the symbols coded with frequency 1
      arm_counts         [n0, n1, n2]: symbols found at the coarse entry's symbol, the one after it, further on --
                         the coarse entry being the last symbol that starts at or below slot (low & ~127)
      longest_step_over  the largest distance beyond the coarse entry's symbol
      y255_at_level_11   symbols 255 coded at level 11
      levels_used        the levels that code at least one pixel"""
    s, q_pos, freq, _ = tables_of(stream)
    assert (int(s[2]), int(s[3])) == (h, w) and len(qd) == len(y) == h * w
    start = np.concatenate([np.zeros((LEVELS, 1), np.int64), np.cumsum(freq, axis=1, dtype=np.int64)[:, :-1]], axis=1)
    f_l, s_l = [list(map(int, r)) for r in freq], [list(map(int, r)) for r in start]
    words = [int(v) for v in s]
    at = q_pos + 2
    x = (words[q_pos] << WORD) | words[q_pos + 1]
    row_words, arms, longest, f1, y255 = [], [0, 0, 0], 0, 0, 0
    qd_l, y_l = [int(v) for v in qd], [int(v) for v in y]
    t = 0
    for _ in range(h):
        at0 = at
        for _ in range(w):
            lv, sym = qd_l[t], y_l[t]
            t += 1
            low = x & (NORM - 1)
            f, s0 = f_l[lv][sym], s_l[lv][sym]
            assert f > 0 and s0 <= low < s0 + f, "the state does not name the plane's symbol"
            d = sym - (bisect.bisect_right(s_l[lv], low & ~127) - 1)
            arms[min(d, 2)] += 1
            longest = max(longest, d)
            f1 += f == 1
            y255 += lv == 11 and sym == 255
            x = (x >> NORM_BITS) * f + low - s0
            if x < 1 << WORD:
                x = (x << WORD) | words[at]
                at += 1
                assert x >= 1 << WORD, "a pixel takes more than one word"
        row_words.append(at - at0)
    assert at == len(words), "the stream is not consumed to its last word"
    assert x == 1 << WORD, "the decoder does not end on the encoder's first state"
    return Replay(q_pos, row_words, f1 / (h * w), arms, longest, y255, sorted(set(qd_l)))


# ---- the set ------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "plane_name family policy plane tables stream")
_CACHE = {}


def models(oracle):
    """plane name -> (plane, qd, y, counts), computed once."""
    if "models" not in _CACHE:
        out = {}
        for name, plane in planes().items():
            plane.setflags(write=False)
            out[name] = (plane,) + tuple(oracle.q_model(plane))
        _CACHE["models"] = out
    return _CACHE["models"]


def cases(oracle):
    """Every (plane, family, policy) stream, coded once per process: plane order, then FAMILIES order, then POLICIES."""
    if "cases" not in _CACHE:
        t0 = time.perf_counter()
        out = []
        for name, (plane, qd, y, counts) in models(oracle).items():
            for fam in families_of(name):
                tables = FAMILIES[fam](counts)
                greedy = oracle.qencode_tables(plane, tables, (qd, y, counts))
                for policy in POLICIES:
                    out.append(Case(name, fam, policy, plane, tables, recode(greedy, policy)))
        _CACHE["cases"] = out
        print(f"oracle: {len(out)} foreign QNBLIC streams, {sum(len(c.stream) for c in out)} bytes, coded in {time.perf_counter() - t0:.1f} s")
    return _CACHE["cases"]


def replays(oracle):
    """(plane name, family) -> Replay of the greedy stream (the policies share its body), once per process."""
    if "replays" not in _CACHE:
        t0 = time.perf_counter()
        m = models(oracle)
        out = {}
        for c in cases(oracle):
            if c.policy == "greedy":
                plane, qd, y, _ = m[c.plane_name]
                out[(c.plane_name, c.family)] = replay(c.stream, plane.shape[0], plane.shape[1], qd, y)
        _CACHE["replays"] = out
        print(f"replay: {len(out)} bodies in {time.perf_counter() - t0:.1f} s")
    return _CACHE["replays"]


def case_of(oracle, plane_name, family, policy="greedy"):
    for c in cases(oracle):
        if (c.plane_name, c.family, c.policy) == (plane_name, family, policy):
            return c
    raise KeyError((plane_name, family, policy))


def golden():
    """tests/golden/foreign_q_streams.json (make_foreign_q.py): per "<plane>/<family>" the SHA-256 of the streams of
    POLICIES concatenated, of the planes the compiled reference decoded them to, and the streams' total length."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign_q_streams.json")) as f:
        return json.load(f)
