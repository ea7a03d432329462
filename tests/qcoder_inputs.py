"""Caller-made jobs for the device rANS stage of effort 0 (csrc/q_rans.h, csrc/q_device_coder.hip): words of
``level | symbol << 8`` and the 12 x 256 raw counts they are coded with.  The counts need not be the words' own: the
stage takes any histogram that counts every symbol the words use, which is how a test reaches tables no image gives."""
import numpy as np


def counted(words):
    w = np.asarray(words, np.uint16).ravel()
    return np.bincount((w & 0xFF).astype(np.int64) * 256 + (w >> 8).astype(np.int64), minlength=12 * 256).astype(np.uint32)


def uniform(n, seed, levels=12, syms=256):
    rng = np.random.default_rng(seed)
    w = (rng.integers(0, levels, n).astype(np.uint16) | (rng.integers(0, syms, n).astype(np.uint16) << 8))
    return w, counted(w)


def f_one(n, seed):
    """Level 3's symbol 5 scales to f = 1 (one count against ten million of symbol 9) and is coded in runs: every step of
    a run renormalises.  Between the runs, ordinary words of other levels."""
    w, _ = uniform(n, seed, levels=3)
    run = np.uint16(3 | (5 << 8))
    w[: n // 3] = run
    w[n - n // 4:] = run                                            # the pass begins inside a run
    hist = counted(w)
    hist[3 * 256 + 5] = 1
    hist[3 * 256 + 9] = 10_000_000
    return w, hist


def one_symbol(n, seed):
    """Level 7 has one used symbol (f = 32767), coded in long runs: no step of a run emits a word; levels 8 .. 11 are never coded."""
    w, _ = uniform(n, seed, levels=7, syms=4)
    w[n // 5: n // 5 + n // 2] = np.uint16(7 | (200 << 8))
    return w, counted(w)


def padded(words, seed):
    """The words with random padding of valid shape (levels below 12, any symbol) up to the end of the last 512-byte window."""
    n = len(words)
    total = (n + 255) // 256 * 256
    pad, _ = uniform(total - n, seed) if total > n else (np.zeros(0, np.uint16), None)
    return np.concatenate([np.asarray(words, np.uint16), pad])


def job(n, seed):
    """Job number `seed` of a wave: the construction rotates so that a wave mixes all three."""
    kind = seed % 3
    if kind == 1 and n >= 8:
        return f_one(n, seed)
    if kind == 2 and n >= 8:
        return one_symbol(n, seed)
    return uniform(n, seed, levels=1 + seed % 12, syms=1 + (seed * 37) % 256)
