"""Records for the chain and partition kernels' tests (test_chain_inputs_host.py, test_chain_kernels.py): S1 records
and bin events that no image produces, made so that a context chain has a chosen length, a block's warm-up meets or does
not, a counter chain starts at a chosen alignment, a halving falls on a chosen slot of a window, a segment has a chosen
number of busy chains -- and plain CPU replays of the chains (one key at a time, Python integers), which say what each
family reaches and what the tables hold afterwards.

Pure integer numpy with fixed seeds.  Keys are interleaved in raster order in proportion to their chains' lengths with a
seeded jitter, so a 64-item row of a partition kernel always mixes keys.
"""
import ctypes as C

import numpy as np

BLOCK, WARM = 4096, 3072                 # kernels_e1.hip kBiasBlock, kBiasWarm
WIN = 512                                # kernels_e1.hip kWin: touches per window of a counter chain
COUNT_LIMIT = 8192
MODEL = {0: dict(keys=2048, extreme=32576, emax=127, err_mul=256, rnd=64, shift=7),
         1: dict(keys=3072, extreme=1 << 20, emax=255, err_mul=2048, rnd=63, shift=10)}


# ---------------------------------------------------------------------------------------------------------------------
# packing (csrc/model.h)
def pack_s1(px0, adr, qu, qv, qw):
    rel = np.where(qv == qu, 0, np.where(qv > qu, 1, 2)).astype(np.uint32)
    return (px0.astype(np.uint32) | (adr.astype(np.uint32) << 8) | (qw.astype(np.uint32) << 19) |
            ((qu.astype(np.uint32) & 1) << 24) | (rel << 25))


def pack_q(px0, adr):
    return px0.astype(np.uint32) | (adr.astype(np.uint32) << 8)


def pack_event(qu, qv, node, qw, bin_):
    a = lambda v: np.asarray(v).astype(np.uint32)
    return a(qu) | (a(qv) << 4) | (a(node) << 8) | (a(qw) << 16) | (a(bin_) << 21)


def counter_key(tree, node):
    """The touch partition's key of counter (tree, node): even trees first (kernels_e1.hip touch_of)."""
    return (tree & 1) * 2048 + (tree >> 1) * 256 + node


def key_counter(gk):
    gk = np.asarray(gk)
    return ((gk >> 8) & 7) * 2 + (gk >> 11), gk & 255


# ---------------------------------------------------------------------------------------------------------------------
def interleave(counts, seed):
    """counts[key] records per key -> (key of every raster position, its index in the key's chain): chains advance in
    proportion to their lengths, jittered, so neighbours in raster order have different keys."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    key = np.repeat(np.arange(len(counts)), counts)
    idx = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
    rng = np.random.default_rng(seed)
    order = np.argsort((idx + rng.random(n)) / np.repeat(counts, counts), kind="stable")
    return key[order], idx[order]


def _levels(rng, adr):
    """Levels an S1 record can carry for this address: qu = 2 (adr >> 8) + a bit, qv = qu or a neighbour, qw 0..16."""
    n = len(adr)
    qu = 2 * (adr >> 8) + rng.integers(0, 2, n)
    qv = np.clip(qu + rng.integers(-1, 2, n), 0, 15)
    return qu, qv, rng.integers(0, 17, n)


def model_family(name, model, chains, seed):
    """chains: {key: errors of the chain's records, in order}.  px0 is random where the error leaves room, x = px0 + err."""
    m = MODEL[model]
    counts = np.zeros(m["keys"], np.int64)
    for k, e in chains.items():
        counts[k] = len(e)
    adr, idx = interleave(counts, seed)
    err = np.zeros(len(adr), np.int64)
    for k, e in chains.items():
        sel = adr == k
        err[sel] = np.asarray(e, np.int64)[idx[sel]]
    assert np.abs(err).max(initial=0) <= m["emax"]
    rng = np.random.default_rng(seed + 1)
    lo, hi = np.maximum(0, -err), np.minimum(255, 255 - err)
    px0 = lo + (rng.integers(0, 256, len(adr)) % (hi - lo + 1))
    fam = dict(name=name, model=model, adr=adr.astype(np.uint16), px0=px0.astype(np.uint8), x=(px0 + err).astype(np.uint8))
    if model == 0:
        qu, qv, qw = _levels(rng, adr)
        fam.update(qu=qu.astype(np.uint8), qv=qv.astype(np.uint8), qw=qw.astype(np.uint8))
    return fam


def rec1_of(fam):
    if fam["model"] == 1:
        return pack_q(fam["px0"], fam["adr"])
    return pack_s1(fam["px0"], fam["adr"], fam["qu"], fam["qv"], fam["qw"])


def cut(fam, a, b):
    return {k: (v[a:b] if isinstance(v, np.ndarray) else v) for k, v in fam.items()}


def noise(seed, n, amp=12):
    return np.random.default_rng(seed).integers(-amp, amp + 1, n)


LENGTHS = [1, 4095, 4096, 4097, 7167, 7168, 7169, 8192, 8193]
LENGTH_KEYS = {0: [3, 255, 256, 700, 1023, 1024, 1500, 2040, 2047], 1: [3, 255, 256, 1023, 2048, 2049, 2500, 3000, 3071]}


def model_families(model):
    """name -> family.  What each must reach is asserted in test_chain_inputs_host.py."""
    m = MODEL[model]
    last, em = m["keys"] - 1, m["emax"]
    out = {}
    keys = LENGTH_KEYS[model]
    out["lengths_noise"] = model_family("lengths_noise", model, {k: noise(10 + k, n) for k, n in zip(keys, LENGTHS)}, 1)
    out["lengths_const"] = model_family("lengths_const", model, {k: np.full(n, 5 + (k % 7)) for k, n in zip(keys, LENGTHS)}, 2)
    i = np.arange(6 * BLOCK)
    alt = np.where(((i + 1024) // BLOCK) % 2 == 0, noise(3, len(i)), 9)           # noise and constant stretches; a warm-up straddles every change
    flip = np.where(i % 2 == 0, em, -em)                                          # period 2, extreme: the copies never meet
    j = np.arange(4 * BLOCK + 100)
    burst = np.where((j >= 6200) & (j < 8100), noise(4, len(j)), 9)               # constant but for noise inside block 2's warm-up alone: not met, met, not met, not met
    out["alternation"] = model_family("alternation", model, {keys[1]: alt, keys[4]: burst, keys[-2]: flip}, 3)
    out["bounds"] = model_family("bounds", model, {keys[2]: np.r_[np.full(3000, em), np.full(3000, -em)],
                                                   keys[-1]: np.r_[np.full(3000, -em), np.full(3000, em)]}, 4)
    out["keys_all"] = model_family("keys_all", model, {k: noise(k, 1, em) for k in range(m["keys"])}, 5)
    out["key_first"] = model_family("key_first", model, {0: noise(6, 3000, 40)}, 6)
    out["key_last"] = model_family("key_last", model, {last: noise(7, 3000, 40)}, 7)
    if model == 1:
        out["keys_high"] = model_family("keys_high", model, {k: noise(k, 5, 60) for k in range(2048, 3072)}, 8)
    few = [0, 1, 2, 255, 256, last - 1, last]
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049):                            # partition edges: a second segment starts at 1025
        rng = np.random.default_rng(100 + n)
        ks = rng.integers(0, len(few), n)
        out[f"edge_{n}"] = model_family(f"edge_{n}", model, {few[j]: noise(n + j, int((ks == j).sum()), 30) for j in range(len(few)) if (ks == j).any()}, 9 + n)
    if model == 0:
        out["remapper"] = remapper_family()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU replays.  Reference lines: NBLIC.c:413-428 / QNBLIC.c:176-188 (bias), NBLIC.c:431-523 (symbol, re-mapper),
# NBLIC.c:589-637 (counters).
def ctx_update(model, v, e):
    m = MODEL[model]
    return (127 * v + m["err_mul"] * e + m["rnd"]) >> 7


def errors_of(fam):
    e = fam["x"].astype(np.int64) - fam["px0"].astype(np.int64)
    return np.clip(e, -127, 127) if fam["model"] == 0 else e


def ctx_replay(fam, state=None):
    """The context chains one key at a time.  Returns px, sign (raster order), the end table, blk_base, and per block of
    every chain (key order) a tuple (key, block, met, copy_lo, copy_hi, true state at the block's first record): the two
    copies start at -+extreme and run over the kBiasWarm records before the block; block 0 starts from the table."""
    model = fam["model"]
    m = MODEL[model]
    keys, sh = m["keys"], m["shift"]
    adr = fam["adr"].astype(np.int64)
    err = errors_of(fam)
    order = np.argsort(adr, kind="stable")
    counts = np.bincount(adr, minlength=keys)
    starts = np.cumsum(counts) - counts
    end = np.zeros(keys, np.int64) if state is None else np.asarray(state, np.int64).copy()
    out = np.zeros(len(adr), np.int64)
    blocks, blk_base = [], np.zeros(keys + 1, np.int64)
    mul, rnd = m["err_mul"], m["rnd"]
    for k in range(keys):
        blk_base[k + 1] = blk_base[k] + (counts[k] + BLOCK - 1) // BLOCK
        if not counts[k]:
            continue
        idx = order[starts[k]:starts[k] + counts[k]]
        es = err[idx].tolist()
        v, outs, at_block = int(end[k]), [], []
        for j, e in enumerate(es):
            if j % BLOCK == 0:
                at_block.append(v)
            outs.append(v >> sh)
            v = (127 * v + mul * e + rnd) >> 7
        end[k] = v
        out[idx] = outs
        for b, true_v in enumerate(at_block):
            if b == 0:
                blocks.append((k, 0, True, true_v, true_v, true_v))
                continue
            va, vb = -m["extreme"], m["extreme"]
            for e in es[b * BLOCK - WARM:b * BLOCK]:
                va = (127 * va + mul * e + rnd) >> 7
                vb = (127 * vb + mul * e + rnd) >> 7
            blocks.append((k, b, va == vb, va, vb, true_v))
    sign = out & 1
    px = np.clip(fam["px0"].astype(np.int64) + (out >> 1) + sign, 0, 255)
    return dict(px=px.astype(np.uint8), sign=sign.astype(np.uint8), end=end.astype(np.int32), blk_base=blk_base.astype(np.uint32),
                blocks=blocks, blk_ok=np.array([b[2] for b in blocks], np.uint8))


def x_to_y(x, px, sign):
    x, px, sign = (np.asarray(a).astype(np.int64) for a in (x, px, sign))
    ty, d = np.minimum(px, 255 - px), np.abs(x - px)
    return np.where(d == 0, 0, np.where(d <= ty, 2 * d - ((x >= px).astype(np.int64) ^ sign), d + ty))


def y_to_x(y, px, sign):
    ty = min(px, 255 - px)
    if y <= 0:
        return px
    if y <= 2 * ty:
        mag = (y + 1) >> 1
        return px + mag if ((y & 1) ^ sign) else px - mag
    return px + (y - ty) if px < 128 else px - (y - ty)


def map_init():
    t = np.zeros((512, 60), np.int32)
    t[:, 0:20] = np.arange(20)
    t[:, 20:40] = np.arange(20)
    t[:, 40:60] = 2 * (19 - np.arange(20))
    return t.reshape(-1)


def mapper_replay(x, px, sign, state=None, y=None):
    """The re-mapper chains one key (2 px + sign) at a time: z in raster order (a symbol >= 20 codes as itself), the end
    tables (512 x [symbol -> rank, rank -> symbol, hits by rank]), and per key its first position in the partitioned
    stream, its length and its number of overtakes.  y: the symbols, where they are not the lossless ones of x."""
    y = x_to_y(x, px, sign) if y is None else np.asarray(y).astype(np.int64)
    key = np.asarray(px).astype(np.int64) * 2 + np.asarray(sign).astype(np.int64)
    tab = (map_init() if state is None else np.asarray(state, np.int32).copy()).reshape(512, 60)
    z = y.copy()
    inside = y < 20
    order = np.flatnonzero(inside)[np.argsort(key[inside], kind="stable")]
    counts = np.bincount(key[inside], minlength=512)
    starts = np.cumsum(counts) - counts
    info = {}
    for k in np.flatnonzero(counts):
        idx = order[starts[k]:starts[k] + counts[k]]
        rank_of, sym_at, cnt = tab[k, 0:20].tolist(), tab[k, 20:40].tolist(), tab[k, 40:60].tolist()
        zs, swaps = [], 0
        for s in y[idx].tolist():
            r = rank_of[s]
            zs.append(r)
            cnt[r] += 1
            if r > 0 and cnt[r - 1] < cnt[r]:
                other = sym_at[r - 1]
                cnt[r], cnt[r - 1] = cnt[r - 1], cnt[r]
                sym_at[r], sym_at[r - 1] = other, s
                rank_of[s], rank_of[other] = r - 1, r
                swaps += 1
        z[idx] = zs
        tab[k] = rank_of + sym_at + cnt
        info[int(k)] = (int(starts[k]), int(counts[k]), swaps)
    return dict(y=y.astype(np.uint8), z=z.astype(np.uint8), end=tab.reshape(-1), chains=info)


REMAP_LENGTHS = [1, 5, 257, 513, 3, 4, 255, 256]            # in key order: the chains start at 0, 1, 6, 263, 776, ... -- every start & 3


def remapper_family():
    """NBLIC only.  Every record is steered to a context whose bias stays in [0, 128): px = px0 and sign = 0 throughout,
    so the re-mapper key is 2 px0 and each chain's length and symbols are chosen here.  Three groups of eight consecutive
    px0: the two top symbols overtaking each other at every second step, as often as a chain can (y = b b a b b a a b b ...), all twenty symbols in rotation, and the rotation with
    symbols >= 20 (which bypass the re-mapper and are not part of any chain) mixed in."""
    rng = np.random.default_rng(77)
    chains = {}
    for g, base in enumerate((60, 100, 140)):
        for j, n in enumerate(REMAP_LENGTHS):
            i = np.arange(n)
            if g == 0:
                ys = np.r_[1, 1, np.where(((i + 1) // 2) % 2 == 0, 0, 1)][:n]    # ranks 0 and 1 (38 and 36 hits at first): level after two, then an overtake every second step
            elif g == 1:
                ys = (i * 7 + j) % 20
            else:                                                        # a bypass symbol behind every fourth: it is in no chain, the length stays n
                ys = np.insert((i * 3 + j) % 20, np.arange(4, n, 4), 20 + (np.arange(4, n, 4) % 30))
            chains[base + j] = ys
    counts = np.zeros(256, np.int64)
    for p, ys in chains.items():
        counts[p] = len(ys)
    px0s, idx = interleave(counts, 78)
    n = len(px0s)
    v = np.zeros(2048, np.int64)
    adr, x = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for t in range(n):
        p = int(px0s[t])
        xv = y_to_x(int(chains[p][idx[t]]), p, 0)
        e = max(-127, min(127, xv - p))
        nv = (127 * v + 256 * e + 64) >> 7
        quiet = (v >= 0) & (v < 128)
        ok = np.flatnonzero(quiet & (nv >= 0) & (nv < 128))              # a context that stays quiet, spread over the key space;
        if not len(ok):                                                  # or a quiet one that is not used again
            ok = np.flatnonzero(quiet)
        a = int(ok[(t * 37) % len(ok)])
        adr[t], x[t], v[a] = a, xv, nv[a]
    fam = dict(name="remapper", model=0, adr=adr.astype(np.uint16), px0=px0s.astype(np.uint8), x=x.astype(np.uint8))
    qu, qv, qw = _levels(rng, adr)
    fam.update(qu=qu.astype(np.uint8), qv=qv.astype(np.uint8), qw=qw.astype(np.uint8))
    return fam


# ---------------------------------------------------------------------------------------------------------------------
# back half
def event_fields(ev):
    ev = np.asarray(ev, np.uint32).astype(np.int64)
    return ev & 15, (ev >> 4) & 15, (ev >> 8) & 255, (ev >> 16) & 31, (ev >> 21) & 1


def touches_of(ev):
    """Per event the keys of its touches (or -1): [0] tree u's, [1] tree v's -- none when the trees coincide (one counter,
    touched once with both weights) or the weight is 0."""
    qu, qv, node, qw, _ = event_fields(ev)
    ku = counter_key(qu, node)
    kv = np.where((qu != qv) & (qw != 0), counter_key(qv, node), -1)
    return ku, kv


def chain_layout(ev):
    """Touches per key and the chains' starts in the partitioned touch stream (key order, even trees first)."""
    ku, kv = touches_of(ev)
    counts = np.bincount(ku, minlength=4096) + np.bincount(kv[kv >= 0], minlength=4096)
    return counts, np.cumsum(counts) - counts


def counter_replay(ev, state=None):
    """counter_add (NBLIC.c:589-637) touch by touch in event order.  Returns the mixed probability of every event, the end
    table ((c0, c1) per key), and the halvings as (key, index of the halving touch in its chain)."""
    qu, qv, node, qw, bin_ = (a.tolist() for a in event_fields(ev))
    ku, kv = (a.tolist() for a in touches_of(ev))
    st = np.full((4096, 2), 32, np.int64) if state is None else np.asarray(state, np.int64).reshape(4096, 2).copy()
    c0, c1 = st[:, 0].tolist(), st[:, 1].tolist()
    seen = [0] * 4096
    prob, halv = [], []

    def add(k, b, w):
        if b:
            c1[k] += w
        else:
            c0[k] += w
        if c0[k] + c1[k] > COUNT_LIMIT:
            c0[k] = (c0[k] + 1) >> 1
            c1[k] = (c1[k] + 1) >> 1
            halv.append((k, seen[k]))

    for r in range(len(ku)):
        k, w, b = ku[r], qw[r], bin_[r]
        pu = 4096 * c1[k] // (c0[k] + c1[k])
        pv = pu
        if qu[r] == qv[r]:
            add(k, b, 32 - w)
            add(k, b, w)
            seen[k] += 1
        else:
            k2 = counter_key(qv[r], node[r])
            pv = 4096 * c1[k2] // (c0[k2] + c1[k2])
            add(k, b, 32 - w)
            seen[k] += 1
            if kv[r] >= 0:
                add(k2, b, w)
                seen[k2] += 1
        prob.append(min(4095, max(1, (pu * (32 - w) + pv * w + 16) >> 5)))
    return dict(prob=np.array(prob, np.uint16), end=np.stack([c0, c1], 1).astype(np.int32).reshape(-1), halvings=halv)


def halving_slots(ev):
    """Where the halvings of a family fall in the counter kernels' windows: (windows' halving counts over every window of
    every chain, set of lanes, set of lane-local slots)."""
    counts, starts = chain_layout(ev)
    per_window = {}
    for k in np.flatnonzero(counts):
        for wdw in range(((starts[k] & 7) + counts[k] + WIN - 1) // WIN):
            per_window[(int(k), wdw)] = 0
    lanes, slots = set(), set()
    for k, i in counter_replay(ev)["halvings"]:
        pos = int(starts[k] & 7) + i
        per_window[(k, pos // WIN)] += 1
        lanes.add((pos % WIN) >> 3)
        slots.add(pos & 7)
    return per_window, lanes, slots


def _single(keys, rng):
    """One touch of weight 32 per event: both trees the key's own, qw 0."""
    tree, node = key_counter(keys)
    return pack_event(tree, tree, node, 0, rng.integers(0, 2, len(keys)))


def _chains_in_order(lengths, seed, first_key=0):
    """Consecutive keys with these touch counts (single touches), interleaved."""
    counts = np.zeros(4096, np.int64)
    counts[first_key:first_key + len(lengths)] = lengths
    keys, _ = interleave(counts, seed)
    return _single(keys, np.random.default_rng(seed + 1))


def align_lengths():
    """For every alignment p = start & 7 the lengths that cut a window at the chain's first or last slot or bring the extra
    window; a filler chain in front of each sets its start.  Returns (lengths in key order, [(key, p, length)])."""
    lengths, targets, at = [], [], 0
    for p in range(8):
        for ln in (1, 8 - p, 9 - p, 511 - p, 512 - p, 513 - p, 1024 - p, 1500):
            fill = (p - at) % 8 or 8
            lengths.append(fill)
            at += fill
            targets.append((len(lengths), p, ln))
            lengths.append(ln)
            at += ln
    return lengths, targets


def back_families():
    out = {}
    lengths, _ = align_lengths()
    out["alignment"] = _chains_in_order(lengths, 21)
    out["staging"] = staging_family()
    out["shapes"] = shape_events(26, 6000)
    for n in (1, 63, 64, 65, 1024, 1025, 2049):
        out[f"size_{n}"] = shape_events(30 + n, n)
    return out


def shape_events(seed, n):
    """Every shape of event the walk emits, on few counters: qu even and odd; qv = qu, qu + 1, qu - 1; qw 0 (the second
    touch is dropped), 1, 16 and between; levels 0 and 15; either bin."""
    rng = np.random.default_rng(seed)
    qu = rng.choice([0, 1, 2, 7, 8, 14, 15], n)
    qv = np.clip(qu + rng.integers(-1, 2, n), 0, 15)
    qw = rng.choice([0, 1, 16, 5, 11], n)
    return pack_event(qu, qv, rng.choice([0, 1, 255, 17], n), qw, rng.integers(0, 2, n))


SEG = 1024                                # kernels_e1.hip make_plan: a touch segment of a job of up to 262144 events


def _segment(busy, singles, rng, tree_pair=None):
    """One segment's events: busy = {key: touches}, plus `singles` events on keys of their own; shuffled."""
    keys = np.repeat(list(busy), list(busy.values()))
    spare = np.setdiff1d(np.arange(2048), list(busy))[:singles]
    keys = np.concatenate([keys, spare])
    assert len(keys) == SEG
    keys = rng.permutation(keys)
    if tree_pair is None:
        return _single(keys, rng)
    tree, node = key_counter(keys)                                      # two touches per event: the odd neighbour tree gets the same chains
    return pack_event(tree, tree + 1, node, 8, rng.integers(0, 2, len(keys)))


def staging_family():
    """Segments of 1024 events for k_touch_scatter's staging: 63 and 64 chains of 16 touches (64 x 16 fills a segment: a
    tie of every chain at the threshold, in both parities); chains of 15 / 16 / 17 touches; rows in which one staged key
    fills 20, 40, 10, 64, 5 of 64 lanes (ring -> direct store -> ring); all 4096 counters with one touch each."""
    rng = np.random.default_rng(27)
    segs = [_segment({k * 3: 16 for k in range(63)}, 16, rng),
            _segment({k * 2: 16 for k in range(64)}, 0, rng),
            _segment({k * 2: 16 for k in range(64)}, 0, rng, tree_pair=True),
            _segment({**{k: 15 for k in range(0, 20)}, **{k: 16 for k in range(300, 320)}, **{k: 17 for k in range(900, 920)}}, 64, rng)]
    rows = []
    others = np.array([5, 6, 7, 600, 601])                              # staged too (>= 16 touches each in the segment)
    for fill in (20, 40, 10, 64, 5, 33, 32, 31, 48, 2, 64, 64, 1, 40, 40, 12):
        row = np.r_[np.full(fill, 1234), others[rng.integers(0, len(others), 64 - fill)]]
        rows.append(rng.permutation(row))
    segs.append(_single(np.concatenate(rows), rng))
    segs.append(_single(rng.permutation(4096), rng))
    return np.concatenate(segs)


WIDE_SEG = 3328


def staging_wide_family():
    """256 segments of 3328 events (a job of 851968 events: the smallest plan whose segments hold 200 chains of 16
    touches).  Segment 0: 65 chains of 16 (no threshold leaves 64 or fewer but 17: nothing is staged).  Segment 1: 200
    chains -- 40 of 18, 20 of 17, 140 of 16 (threshold 17, 60 staged).  Segment 2: 50 of 20 and 30 of 17 (80 at 17: the tie
    is cut, threshold 18).  The rest: every counter at most once per segment."""
    rng = np.random.default_rng(28)

    def seg(busy):
        keys = np.repeat(list(busy), list(busy.values()))
        spare = rng.permutation(np.setdiff1d(np.arange(4096), list(busy)))[:WIDE_SEG - len(keys)]
        return rng.permutation(np.concatenate([keys, spare]))
    parts = [seg({k * 5: 16 for k in range(65)}),
             seg({**{k: 18 for k in range(0, 40)}, **{k: 17 for k in range(100, 120)}, **{k: 16 for k in range(200, 340)}}),
             seg({**{k: 20 for k in range(500, 550)}, **{k: 17 for k in range(600, 630)}})]
    parts += [rng.permutation(4096)[:WIDE_SEG] for _ in range(253)]
    return _single(np.concatenate(parts), rng)


def busy_chains(ev, seg_len):
    """Per (segment, parity): how many chains have at least 16 touches there."""
    ku, kv = touches_of(ev)
    seg = np.arange(len(ku)) // seg_len
    nseg = int(seg.max()) + 1
    cnt = np.zeros((nseg, 4096), np.int64)
    np.add.at(cnt, (seg, ku), 1)
    np.add.at(cnt, (seg[kv >= 0], kv[kv >= 0]), 1)
    return (cnt[:, :2048] >= 16).sum(1), (cnt[:, 2048:] >= 16).sum(1), cnt


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's array stages (oracle/nblic_staged.c, qnblic_oracle.c)
def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def orc_model(oracle, fam):
    """NBLIC: px, sign (orc_s2), z (orc_s3), bins per record (orc_s4) of a family."""
    L = oracle.lib
    n = len(fam["adr"])
    err = errors_of(fam).astype(np.int8)
    adr, px0, x = (np.ascontiguousarray(fam[k]) for k in ("adr", "px0", "x"))
    px, sign, y, z, cnt = (np.empty(n, np.uint8) for _ in range(5))
    L.orc_s2(C.c_size_t(n), _p(adr, C.c_uint16), _p(px0, C.c_uint8), _p(err, C.c_int8), _p(px, C.c_uint8), _p(sign, C.c_uint8))
    L.orc_s3(C.c_size_t(n), _p(x, C.c_uint8), _p(px, C.c_uint8), _p(sign, C.c_uint8), _p(y, C.c_uint8), _p(z, C.c_uint8))
    L.orc_s4.restype = C.c_size_t
    qu, qv, qw = (np.ascontiguousarray(fam[k]) for k in ("qu", "qv", "qw"))
    L.orc_s4(C.c_size_t(n), _p(qu, C.c_uint8), _p(qv, C.c_uint8), _p(qw, C.c_uint8), _p(z, C.c_uint8), None, None, None, None, _p(cnt, C.c_uint8))
    return dict(px=px, sign=sign, y=y, z=z, cnt=cnt)


def orc_q_s2(oracle, adr, px0, x):
    adr, px0, x = np.ascontiguousarray(adr, np.uint16), np.ascontiguousarray(px0, np.uint8), np.ascontiguousarray(x, np.uint8)
    y, end = np.empty(len(adr), np.uint8), np.zeros(3072, np.int32)
    oracle.lib.orc_q_s2(C.c_size_t(len(adr)), _p(adr, C.c_uint16), _p(px0, C.c_uint8), _p(x, C.c_uint8), _p(y, C.c_uint8), _p(end, C.c_int))
    return y, end


def orc_s5(oracle, ev):
    qu, qv, node, qw, bin_ = event_fields(ev)
    cu, cv = (qu * 256 + node).astype(np.uint16), (qv * 256 + node).astype(np.uint16)
    qw, bin_ = qw.astype(np.uint8), bin_.astype(np.uint8)
    prob = np.empty(len(cu), np.uint16)
    oracle.lib.orc_s5(C.c_size_t(len(cu)), _p(cu, C.c_uint16), _p(cv, C.c_uint16), _p(qw, C.c_uint8), _p(bin_, C.c_uint8), _p(prob, C.c_uint16))
    return prob
