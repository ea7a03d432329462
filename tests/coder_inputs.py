"""Record streams for the range coders' tests (u16 per bin: the probability of a 1 in 1/4096 in bits 0-11, the bin in
bit 15), shared by the host pack feed's tests and the device coder's.  Probability 0 is not a record and none of these
makes one."""
import numpy as np


def records(rng, n):
    """n random records: every probability 1..4095, either bin."""
    return rng.integers(1, 4096, n).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 15)


def runs(seed, n):
    """Probabilities 1 and 4095 in runs of 40..900 bins of the likely bin -- nothing leaves the coder for a long time --
    and, one run in four, of the unlikely bin: several bytes per step, long carries of renormalisation."""
    r = np.random.default_rng(seed)
    out = np.empty(n, np.uint16)
    at = 0
    while at < n:
        k = int(r.integers(40, 900))
        p, b = (1, 1) if r.integers(0, 2) else (4095, 0)
        if r.integers(0, 4) == 0:
            b ^= 1                                     # the unlikely bin now and then: long carries of renormalisation
        out[at:at + k] = p | (b << 15)
        at += k
    return out


def every_probability(rng):
    """8190 records in random order: each probability 1..4095 once with either bin."""
    p = np.arange(1, 4096, dtype=np.uint16)
    return rng.permutation(np.concatenate([p, p | np.uint16(1 << 15)]))
