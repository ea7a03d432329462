"""Records and images for the long-chain tests (test_long_chains_host.py, test_long_chains.py): context chains whose
blocks' warm-up copies do not meet, and a plain restatement of what the kernels do with such blocks -- a table of end
states over the candidate start states, one look-up per block along the chain, the outputs from the exact start state
(kernels_e1.hip k_bias_tabulate / k_bias_fixup / k_bias_replay); re-mapper chains of chosen symbols and lengths, and the
same for their blocks: exact counts by symbol, a guessed permutation per block, an in-order check.  Pure integer numpy with fixed seeds; the helpers of
chain_inputs.py make the records and the reference replay.
"""
import numpy as np

import chain_inputs as ci

BLOCK, WARM, CANDS = ci.BLOCK, ci.WARM, 128          # kernels_e1.hip kBiasBlock, kBiasWarm, kBiasCands
GAP_STEPS = {0: 869, 1: 1311}                        # steps of g -> ceil(127 g / 128) from 2 * extreme down to 127


def gap_steps(gap):
    """How many steps of g -> ceil(127 g / 128) bring `gap` to 127, where the recurrence stops."""
    n = 0
    while gap > CANDS - 1:
        gap = -((-127 * gap) // 128)
        n += 1
    return n


def s2_families(model):
    """name -> family; what each reaches is asserted in test_long_chains_host.py."""
    keys = ci.LENGTH_KEYS[model]
    base = ci.model_families(model)
    out = {k: base[k] for k in ("lengths_const", "alternation", "bounds")}
    out["const5"] = ci.model_family("const5", model, {keys[3]: np.full(5 * BLOCK + 100, 9)}, 41)
    # an unmet last block of one record, next to a noisy chain that meets and a second flat one at the key space's end
    out["last_one"] = ci.model_family("last_one", model, {keys[1]: np.full(BLOCK + 1, -3), keys[5]: ci.noise(42, 2 * BLOCK + 7),
                                                          keys[-1]: np.full(2 * BLOCK + 1, ci.MODEL[model]["emax"])}, 43)
    return out


def walk(model, v, errs):
    """The chain over errs from the states v (a numpy array of start states): the end states."""
    m = ci.MODEL[model]
    v = np.asarray(v, np.int64).copy()
    for e in errs:
        v = (127 * v + m["err_mul"] * int(e) + m["rnd"]) >> 7
    return v


def s2_scheme(fam, state=None, tables=True):
    """The context chains as the kernels run them.  Per chain: the blocks' copies (chain_inputs.ctx_replay's two-copy
    simulation says where they stand at each block's first record, and whether they met); a block that did not meet and
    whose copies are fewer than CANDS apart is replayed from each of lower copy + 0 .. 127, end states only; the chain's
    blocks are walked in order with one look-up per such block; every block's outputs then come from its own start state.
    Nothing here reads the true states of ctx_replay.  Returns px, sign, end and the counts (met, table, serial) plus the
    tables as (key, block, lower copy, upper copy, end states) for the nesting test.  tables=False: blocks that did not
    meet are replayed in order (the serial count)."""
    model = fam["model"]
    m = ci.MODEL[model]
    sh, mul, rnd = m["shift"], m["err_mul"], m["rnd"]
    r = ci.ctx_replay(fam, state)
    adr = fam["adr"].astype(np.int64)
    err = ci.errors_of(fam)
    order = np.argsort(adr, kind="stable")
    counts = np.bincount(adr, minlength=m["keys"])
    starts = np.cumsum(counts) - counts
    end = np.zeros(m["keys"], np.int64) if state is None else np.asarray(state, np.int64).copy()
    out = np.zeros(len(adr), np.int64)
    n_met = n_tab = n_serial = 0
    tabs = []
    by_key = {}
    for k, b, met, va, vb, _true in r["blocks"]:
        by_key.setdefault(k, []).append((b, met, va, vb))
    for k, blks in by_key.items():
        idx = order[starts[k]:starts[k] + counts[k]]
        es = err[idx]
        v = int(end[k])
        start_of = []
        for b, met, va, vb in blks:
            seg = es[b * BLOCK:(b + 1) * BLOCK]
            if met:                                                      # the common state (block 0: the table's) is the start
                n_met += 1
                start = v if b == 0 else va
                assert b == 0 or start == v                              # what the walk carries agrees with it
                v = int(walk(model, [start], seg)[0])
            elif tables and vb - va < CANDS:
                n_tab += 1
                table = walk(model, np.minimum(va + np.arange(CANDS), m["extreme"]), seg)
                tabs.append((k, b, va, vb, table))
                assert 0 <= v - va < CANDS
                start, v = v, int(table[v - va])
            else:
                n_serial += 1
                start = v
                v = int(walk(model, [start], seg)[0])
            start_of.append(start)
        end[k] = v
        outs = []
        for (b, *_), s in zip(blks, start_of):                           # the replay: a block at a time, from its start state
            for e in es[b * BLOCK:(b + 1) * BLOCK].tolist():
                outs.append(s >> sh)
                s = (127 * s + mul * e + rnd) >> 7
        out[idx] = outs
    sign = out & 1
    px = np.clip(fam["px0"].astype(np.int64) + (out >> 1) + sign, 0, 255)
    return dict(px=px.astype(np.uint8), sign=sign.astype(np.uint8), end=end.astype(np.int32), met=n_met, table=n_tab,
                serial=n_serial, tables=tabs, replay=r)


# ---------------------------------------------------------------------------------------------------------------------
# images of the public paths: the content classes on which one table entry holds most of a frame
def image(content, h, w, seed=5):
    rng = np.random.default_rng(seed)
    if content == "const":
        return np.full((h, w), 131, np.uint8)
    if content == "half-flat":                         # the upper half flat, the lower half texture
        img = np.full((h, w), 60, np.uint8)
        img[h // 2:] = rng.integers(40, 90, (h - h // 2, w))
        return img
    if content == "dark-noise":
        return rng.integers(0, 3, (h, w)).astype(np.uint8)
    raise ValueError(content)


# ---------------------------------------------------------------------------------------------------------------------
# S3: re-mapper chains cut into blocks (kernels_e1.hip k_map_plan .. k_map_check)
def remap_family(name, chains, seed):
    """NBLIC records whose re-mapper chains are chosen here: chains = {key: symbols}, key = 2 px + sign.  As in
    chain_inputs.remapper_family every record is steered to a context whose bias keeps px = px0 and the sign the key
    wants -- [0, 128) for sign 0, [-128, 0) for sign 1 -- from a table that starts with contexts of either kind.
    Symbols >= 20 bypass the re-mapper and are in no chain.  Returns (family, the context table to start from)."""
    rng = np.random.default_rng(seed)
    counts = np.zeros(512, np.int64)
    for k, ys in chains.items():
        counts[k] = len(ys)
    keys, idx = ci.interleave(counts, seed + 1)
    n = len(keys)
    v0 = np.where(np.arange(2048) % 2 == 0, 0, -64).astype(np.int64)
    v = v0.copy()
    adr, x = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for t in range(n):
        p, s = int(keys[t]) >> 1, int(keys[t]) & 1
        xv = ci.y_to_x(int(chains[int(keys[t])][idx[t]]), p, s)
        e = max(-127, min(127, xv - p))
        nv = (127 * v + 256 * e + 64) >> 7
        lo, hi = (-128, 0) if s else (0, 128)
        fits = (v >= lo) & (v < hi)
        ok = np.flatnonzero(fits & (nv >= lo) & (nv < hi))
        if not len(ok):
            ok = np.flatnonzero(fits)
        a = int(ok[(t * 37) % len(ok)])
        adr[t], x[t], v[a] = a, xv, nv[a]
    fam = dict(name=name, model=0, adr=adr.astype(np.uint16), px0=(keys >> 1).astype(np.uint8), x=x.astype(np.uint8))
    qu, qv, qw = ci._levels(rng, adr)
    fam.update(qu=qu.astype(np.uint8), qv=qv.astype(np.uint8), qw=qw.astype(np.uint8))
    return fam, v0.astype(np.int32)


S3_MIN, S3_BLOCK = 1024, 256


def _overtake(n):
    i = np.arange(n)
    return np.r_[1, 1, np.where(((i + 1) // 2) % 2 == 0, 0, 1)][:n]    # chain_inputs.remapper_family: an overtake every second step


def _rotation(n, j=0, step=7):
    return (np.arange(n) * step + j) % 20


def _with_bypass(ys):
    at = np.arange(4, len(ys), 4)
    return np.insert(ys, at, 20 + (at % 30))


def s3_chain_sets():
    """name -> {key: symbols}.  Keys 2 px (sign 0) and 2 px + 1 (sign 1)."""
    rng = np.random.default_rng(9)
    lengths = [1023, 1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537, 2047, 2049]
    out = {"uniform": {2 * 131: np.zeros(5000, np.int64)},
           "lengths": {2 * (40 + 3 * j): _rotation(n, j, 3) if j % 2 else rng.integers(0, 4, n) for j, n in enumerate(lengths)},
           "overtake": {2 * 70: _overtake(3000), 2 * 90 + 1: _overtake(3000)[::-1].copy()},
           "rotation": {2 * 100: _rotation(3000), 2 * 101: _rotation(2999, 5, 3)},
           "bypass": {2 * 140: _with_bypass(_rotation(2400, 1, 3)), 2 * 141 + 1: _with_bypass(rng.integers(0, 3, 1500))}}
    # symbol 1 overtakes symbol 0, symbol 0 draws level and stays BELOW: a tie the counts cannot read, for as long as
    # neither is hit again -- every block started behind it misses; the second chain breaks the tie half way
    stale = np.r_[1, 1, 1, 0, 3 + np.arange(2996) % 2]                 # (symbols 3 and 4: errors +-2, so the contexts stay where they are)
    mended = stale.copy()
    mended[1500] = 1
    out["stale_tie"] = {2 * 50: stale, 2 * 51 + 1: mended}
    # a wave of k_mapper_chains / k_map_check owns sixteen consecutive keys: two long chains and fourteen short ones
    wave = {32 * 5 + j: rng.integers(0, 6, 3 + 40 * j) for j in range(16)}
    wave[32 * 5 + 3] = np.where(rng.random(2600) < 0.9, 0, rng.integers(0, 20, 2600))
    wave[32 * 5 + 12] = rng.integers(0, 20, 1800)
    out["wave"] = wave
    return out


def s3_family(name):
    return remap_family(name, s3_chain_sets()[name], 50 + len(name))


def guess_by_counts(cnt_sym, rank0):
    """Symbol -> rank by descending count; ties keep the order the chain started with (exact for untouched symbols)."""
    order = sorted(range(20), key=lambda s: (-cnt_sym[s], rank0[s]))
    rank_of = [0] * 20
    for r, s in enumerate(order):
        rank_of[s] = r
    return rank_of


def guess_wrong(cnt_sym, rank0):
    return [19 - r for r in guess_by_counts(cnt_sym, rank0)]


def _run(rank_of, cnt_sym, ys):
    """The chain's step over ys from a permutation and the counts BY SYMBOL (which are exact whatever the permutation):
    ranks out, the end permutation."""
    rank_of = list(rank_of)
    sym_at = [0] * 20
    for s, r in enumerate(rank_of):
        sym_at[r] = s
    cnt = [cnt_sym[sym_at[r]] for r in range(20)]
    zs = []
    for s in ys:
        r = rank_of[s]
        zs.append(r)
        cnt[r] += 1
        if r > 0 and cnt[r - 1] < cnt[r]:
            other = sym_at[r - 1]
            cnt[r], cnt[r - 1] = cnt[r - 1], cnt[r]
            sym_at[r], sym_at[r - 1] = other, s
            rank_of[s], rank_of[other] = r - 1, r
    return zs, rank_of


def s3_scheme(x, px, sign, state=None, min_records=S3_MIN, block_records=S3_BLOCK, guess=guess_by_counts, warm=True):
    """The re-mapper chains as the kernels run them: a chain of at least min_records records is cut into blocks of
    block_records; a histogram per block and its prefix give the exact counts by symbol at every block's start; every
    block is replayed from a GUESSED permutation (warm: the guess is made one block earlier and refined over that block;
    blocks 0 and 1 then start from the chain's own table); in order, block b is accepted only if its guess is block b - 1's
    true end permutation, and replayed from the true state otherwise.  Returns z, end (as chain_inputs.mapper_replay) and
    the counts split / accepted / missed."""
    y = ci.x_to_y(x, px, sign)
    key = np.asarray(px).astype(np.int64) * 2 + np.asarray(sign).astype(np.int64)
    tab = (ci.map_init() if state is None else np.asarray(state, np.int32).copy()).reshape(512, 60)
    z = y.copy()
    inside = y < 20
    order = np.flatnonzero(inside)[np.argsort(key[inside], kind="stable")]
    counts = np.bincount(key[inside], minlength=512)
    starts = np.cumsum(counts) - counts
    split = accepted = missed = 0
    for k in np.flatnonzero(counts):
        idx = order[starts[k]:starts[k] + counts[k]]
        ys = y[idx].tolist()
        rank0, sym0, cnt0 = tab[k, 0:20].tolist(), tab[k, 20:40].tolist(), tab[k, 40:60].tolist()
        cnt_sym = [cnt0[rank0[s]] for s in range(20)]
        B = block_records
        if min_records < 0 or len(ys) < min_records:
            zs, end_rank = _run(rank0, cnt_sym, ys)
            cnt_sym = (np.array(cnt_sym) + np.bincount(ys, minlength=20)).tolist()
        else:
            split += 1
            nb = (len(ys) + B - 1) // B
            at = [cnt_sym]                                               # counts by symbol at every block's start, and at the end
            for b in range(nb):
                at.append((np.array(at[-1]) + np.bincount(ys[b * B:(b + 1) * B], minlength=20)).tolist())
            guesses, ends, outs = [], [], []
            for b in range(nb):                                          # in parallel on the GPU
                if b == 0 or (warm and b == 1):
                    g = rank0 if b == 0 else _run(rank0, at[0], ys[:B])[1]
                elif warm:
                    g = _run(guess(at[b - 1], rank0), at[b - 1], ys[(b - 1) * B:b * B])[1]
                else:
                    g = guess(at[b], rank0)
                zs_b, e = _run(g, at[b], ys[b * B:(b + 1) * B])
                guesses.append(g); ends.append(e); outs.append(zs_b)
            true = ends[0]
            for b in range(1, nb):                                       # in order
                if guesses[b] == true:
                    accepted += 1
                    true = ends[b]
                else:
                    missed += 1
                    outs[b], true = _run(true, at[b], ys[b * B:(b + 1) * B])
            zs, end_rank, cnt_sym = [r for o in outs for r in o], true, at[nb]
        z[idx] = zs
        sym_at = [0] * 20
        for s, r in enumerate(end_rank):
            sym_at[r] = s
        tab[k] = list(end_rank) + sym_at + [cnt_sym[sym_at[r]] for r in range(20)]
    return dict(z=z.astype(np.uint8), end=tab.reshape(-1), split=split, accepted=accepted, missed=missed)
