"""Records for the tests of the entropy front's general kernels (test_entropy_inputs_host.py, test_entropy_front.py):
what k_serial_model leaves per pixel -- the pixel x, the corrected prediction px with its sign, the two levels and their
weight -- made so that the symbol, the re-mapper chain and the binarisation walk are chosen here instead of met by an
image, for every near 0..9 with the k_step the encoders pair with it.  With them the plain references: the symbol and
the walk in Python integers, and the expectation of every array the debug entry returns, from the oracle's general
stages and chain_inputs' replays.

Pure integer numpy with fixed seeds; nothing here comes from a kernel.
"""
import functools

import numpy as np

import chain_inputs as ci

NEARS = range(10)
MAP_SYMS = 20                               # model.h kMapSyms: symbols >= 20 bypass the re-mapper
PAIRS = [(qu, qv) for qu in range(16) for qv in (qu, qu + 1, qu - 1) if 0 <= qv < 16]      # the 46 pairs of adjacent levels
SIZES = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049, 4097)
# near -> (k_step, largest symbol, most bins per symbol, most escalations): a CPU transliteration of the walk
TABLE = {0: (3, 255, 33, 5), 1: (5, 85, 56, 2), 2: (7, 51, 52, 0), 3: (9, 37, 38, 0), 4: (11, 29, 30, 0),
         5: (13, 24, 25, 0), 6: (15, 20, 21, 0), 7: (16, 17, 18, 0), 8: (16, 15, 16, 0), 9: (16, 14, 15, 0)}


def k_step_of(near):
    return min(max(3 + 2 * near, 3), 16)


# ---------------------------------------------------------------------------------------------------------------------
# plain references (NBLIC.c:431-466 the symbol, :640-679 the walk)
def x_to_y(x, px, sign, near):
    x, px, sign = (np.asarray(a).astype(np.int64) for a in (x, px, sign))
    w = 2 * near + 1
    ty, q = (np.minimum(px, 255 - px) + near) // w, (np.abs(x - px) + near) // w
    return np.where(q == 0, 0, np.where(q <= ty, 2 * q - ((x >= px).astype(np.int64) ^ sign), q + ty))


def walk(k_step, qu, qv, z):
    """One symbol's bin events [(qu, qv, node, bin)] and its number of escalations to the next level group's tree."""
    k_max = 15 // k_step
    if qv // k_step != qu // k_step:
        qv = qu
    node, ev, esc = 0, [], 0
    while True:
        k = qu // k_step
        b = int((node >> k_max) < (z >> k))
        ev.append((qu, qv, node, b))
        if not b:
            break
        node += 1 << k_max
        if node >= 256:
            node >>= 1
            qu = qv = (k + 1) * k_step
            esc += 1
    node += 1
    for j in range(k - 1, -1, -1):
        b = (z >> j) & 1
        ev.append((qu, qv, node, b))
        node += (1 << j) if b else 1
    return ev, esc


@functools.lru_cache(maxsize=None)
def all_triples(near):
    """x, px, sign, y of all 131072 triples, index = (x << 9) | (px << 1) | sign."""
    i = np.arange(1 << 17)
    x, px, sign = i >> 9, (i >> 1) & 255, i & 1
    return x, px, sign, x_to_y(x, px, sign, near)


def ymax(near):
    return int(all_triples(near)[3].max())


# ---------------------------------------------------------------------------------------------------------------------
def _hash(i):
    v = (np.asarray(i).astype(np.uint64) + np.uint64(0x632BE5AB)) * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    v *= np.uint64(0xBF58476D1CE4E5B9)
    return (v >> np.uint64(32)).astype(np.int64)


def hashed_levels(n, salt=0):
    """A pair of the 46 and a weight 0..16 per record, by a hash of its index."""
    h = _hash(np.arange(n) + salt * 1000003)
    pair = np.array(PAIRS)[h % len(PAIRS)]
    return pair[:, 0], pair[:, 1], (h >> 8) % 17


def family(name, near, x, px, sign, qu, qv, qw):
    a = lambda v, t=np.uint8: np.ascontiguousarray(np.asarray(v).astype(t))
    return dict(name=name, near=int(near), x=a(x), px=a(px), sign=a(sign), qu=a(qu), qv=a(qv), qw=a(qw))


def rec1_of(fam):
    """pack_s1 words: the entropy front reads the levels and the weight; px0 and the address's low bits are filler."""
    qu = fam["qu"].astype(np.int64)
    adr = ((qu >> 1) << 8) | (_hash(np.arange(len(qu))) & 255)
    return ci.pack_s1(fam["px"], adr, qu, fam["qv"].astype(np.int64), fam["qw"])


def pxs_of(fam):
    return fam["px"].astype(np.uint16) | (fam["sign"].astype(np.uint16) << 8)


def cut(fam, a, b):
    return ci.cut(fam, a, b)


@functools.lru_cache(maxsize=None)
def triples(near):
    """All 131072 (x, px, sign) in a fixed shuffled order."""
    x, px, sign, _ = all_triples(near)
    order = np.random.default_rng(1000 + near).permutation(1 << 17)
    return family(f"triples_{near}", near, x[order], px[order], sign[order], *hashed_levels(1 << 17, near))


@functools.lru_cache(maxsize=None)
def walk_grid(near):
    """Every pair x every z in 0..ymax(near), qw cycling 0, 1, 15, 16: a list of calls.  A cell with z >= 20 is a record
    whose (x, px) give that symbol; a cell with z < 20 is the FIRST record of its (px, sign) chain, for which z = y from
    k_init_state's tables -- so a call holds at most 512 of those, one per key."""
    x, px, sign, y = all_triples(near)
    top = ymax(near)
    first = {}                                                          # (symbol) -> triples with it, in index order
    order = np.argsort(y, kind="stable")
    starts = np.searchsorted(y[order], np.arange(top + 2))
    for s in range(top + 1):
        first[s] = order[starts[s]:starts[s + 1]]
    cells = [(p, z) for z in range(top + 1) for p in range(len(PAIRS))]
    low = [c for c in cells if c[1] < MAP_SYMS]
    high = [c for c in cells if c[1] >= MAP_SYMS]
    calls = []
    for c0 in range(0, max(len(low), 1), 512):
        part = low[c0:c0 + 512]
        used, recs = set(), []
        for j, (p, z) in enumerate(part):                               # a key of its own for every chained cell
            cand = first[z]
            at = (j * 37) % len(cand)
            pick = next(t for t in cand[at:].tolist() + cand[:at].tolist() if (t & 511) not in used)
            used.add(pick & 511)
            recs.append((pick, p))
        share = high[(c0 // 512)::max((len(low) + 511) // 512, 1)]       # the bypassing cells, dealt over the calls
        for j, (p, z) in enumerate(share):
            cand = first[z]
            recs.append((int(cand[(j * 101) % len(cand)]), p))
        perm = np.random.default_rng(2000 + near + c0).permutation(len(recs))
        t = np.array([recs[i][0] for i in perm])
        pr = np.array(PAIRS)[[recs[i][1] for i in perm]]
        qw = np.array([0, 1, 15, 16])[np.arange(len(t)) % 4]
        calls.append(family(f"walk_grid_{near}_{len(calls)}", near, x[t], px[t], sign[t], pr[:, 0], pr[:, 1], qw))
    return calls


def noise_records(name, near, n, seed):
    """n records: prediction noise around a random px, any sign, hashed levels; every eighth record a uniform pixel, and
    every sixteenth a triple with the mode's largest symbol."""
    rng = np.random.default_rng(seed)
    px, sign = rng.integers(0, 256, n), rng.integers(0, 2, n)
    x = np.clip(px + ci.noise(seed + 1, n, 40), 0, 255)
    i = np.arange(n)
    x = np.where(i % 8 == 3, rng.integers(0, 256, n), x)
    ax, apx, asign, ay = all_triples(near)
    top = np.flatnonzero(ay == ay.max())
    t = top[rng.integers(0, len(top), n)]
    far = i % 16 == 9
    x, px, sign = np.where(far, ax[t], x), np.where(far, apx[t], px), np.where(far, asign[t], sign)
    return family(name, near, x, px, sign, *hashed_levels(n, seed))


def sizes(near):
    return [noise_records(f"size_{n}_n{near}", near, n, 3000 + 17 * n + near) for n in SIZES]


def _pick(name, near, mask, n, seed):
    x, px, sign, _ = all_triples(near)
    idx = np.flatnonzero(mask)
    t = idx[np.random.default_rng(seed).integers(0, len(idx), n)]
    return family(name, near, x[t], px[t], sign[t], *hashed_levels(n, seed))


def bypass_all(near, n=3000):
    """Every symbol >= 20: nothing enters the re-mapper partition, every chain is empty."""
    return _pick(f"bypass_all_{near}", near, all_triples(near)[3] >= MAP_SYMS, n, 4000 + near)


def bypass_none(near=0, n=3000):
    return _pick(f"bypass_none_{near}", near, all_triples(near)[3] < MAP_SYMS, n, 4100 + near)


ONE_CHAIN_NEAR, ONE_CHAIN_N = 2, 70000


@functools.lru_cache(maxsize=None)
def one_chain(which):
    """70000 records in re-mapper key 0 (px 0, sign 0), in key 511 (px 255, sign 1: the chain whose end is the
    partition's total), or split between the two; every symbol below 20."""
    n, near = ONE_CHAIN_N, ONE_CHAIN_NEAR
    h = _hash(np.arange(n) + 77)
    hi = {"first": np.zeros(n, bool), "last": np.ones(n, bool), "both": (h >> 20) % 2 == 1}[which]
    d = (h >> 3) % 98                                                   # (d + 2) // 5 < 20
    px, sign = np.where(hi, 255, 0), hi.astype(np.int64)
    return family(f"one_chain_{which}", near, np.where(hi, 255 - d, d), px, sign, *hashed_levels(n, 5))


CARRY_CUTS = (7, 1300, 65536)


def carried_families():
    return [triples(4), one_chain("first"), one_chain("last"), one_chain("both")]


# ---------------------------------------------------------------------------------------------------------------------
def events_of(s4):
    """The oracle's S4 events re-packed as the kernels pack them (model.h pack_event)."""
    cu, cv = s4["cu"].astype(np.int64), s4["cv"].astype(np.int64)
    return ci.pack_event(cu >> 8, cv >> 8, cu & 255, s4["qw"], s4["bin"])


def oracle_key_tables(state):
    """cnt_state (c0, c1 per counter in the touch partition's key order) -> the same table in tree-major order."""
    gk = np.arange(4096)
    tree, node = ci.key_counter(gk)
    out = np.zeros((4096, 2), np.int64)
    out[tree * 256 + node] = np.asarray(state).reshape(4096, 2)
    return out


def expected(oracle, fam, map_state=None, cnt_state=None):
    """Everything the debug entry returns for a family, from the references alone: the symbol by the formula above, the
    re-mapper chains by chain_inputs.mapper_replay (from map_state), the walk by the oracle's general S4 at the paired
    k_step, the counters by chain_inputs.counter_replay (from cnt_state)."""
    near = fam["near"]
    y = x_to_y(fam["x"], fam["px"], fam["sign"], near)
    mr = ci.mapper_replay(fam["x"], fam["px"], fam["sign"], map_state, y=y)
    s4 = oracle.s4_kstep(k_step_of(near), fam["qu"], fam["qv"], fam["qw"], mr["z"])
    ev = events_of(s4)
    cr = ci.counter_replay(ev, cnt_state)
    cnt = s4["cnt"].astype(np.int64)
    return dict(y=y, z=mr["z"], cnt=s4["cnt"], ev_off=(np.cumsum(cnt) - cnt).astype(np.uint32), events=ev, n_ev=len(ev),
                coded=cr["prob"] | (ci.event_fields(ev)[4].astype(np.uint16) << 15), map_state=mr["end"], cnt_state=cr["end"],
                chained=int((y < MAP_SYMS).sum()), s4=s4)
