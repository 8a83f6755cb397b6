"""The rare paths of the two open-addressing tables (csrc/table.hpp) with keys that are CHOSEN, not hashed: probe chains of a known
length, chains that wrap at the table's end, keys that share their low word, keys with a zero word, the probe limit and the full side
list.  mdbg_prev_from_records / mdbg_prev_from_record_bytes take (lo, hi, abundance) as they stand in a file and mdbg_table_lookup takes
any key; the reference keeps these in a phmap<u128, u32> for which every 128-bit value is an ordinary key (graph/CreateMdbg.cpp:3401-3491,
graph/CreateMdbg.hpp:1240-1265).

The home slot is umul64hi(lo ^ (hi >> 17), cap) & ~1 and the home bucket umul64hi(lo ^ (hi >> 17), nb): keys with the same fold
f = lo ^ (hi >> 17) share their home at ANY capacity, so a chain of n keys is n keys of one fold.

Part 1 looks crafted keys up against a Python dict.  Part 2 puts crafted keys around the real ones of a previous table and runs the
look-up, the unitig overlay and the passes above firstK in every form against the oracle, whose previous-abundance map is a sorted array
(oracle/mdbg_oracle.c, orc_abundance_map_get): to it a shadow is one more key that nobody asks for.

Where the probe limit sits in part 2.  A cluster of 97 keys fills every slot its members may probe (probes 0 .. 96), so it exists only
where no other key has its home in those 97 slots and no run of occupied slots reaches them from below: any such key makes some insert
-- which one is up to the order the device takes the rows in -- run past the limit, and mdbg_prev_from_records answers MDBG_ERANGE
(the table of a record file is not grown).  At the load these tables are sized for (0.15 - 0.2, some fifteen foreign homes in any 97
slots) no real key of the large record set has such a neighbourhood.  The clusters of 96 and 97 therefore stand around real keys of a
SMALL input (_limit_scenario), where real keys are found whose folds are alone over what 97 slots span at the smallest capacity a
record file's table can have (5120 slots); the large record set (_scenario) carries every other cluster.  GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import formats
from tests.test_gpu_parity import _assert_tables_equal, _table_form

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MDBG_ERANGE = -5
FORMS = ["slots", "slots_lazy", "slots_never_lazy", "slots_fused", "slots_two_kernels", "slots_two", "slots_round4", "slots_round5",
         "slots_pair_insert", "slots_32_lanes", "buckets"]
SEED = 511                 # of the two large record sets: chosen with the oracle alone, see _scenario
CRAFTED_AB = 1000          # crafted keys have abundances from here on, each its own; no real row comes near


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


# ---- keys -------------------------------------------------------------------------------------------------------------------

def fold(lo, hi):
    return np.uint64(lo) ^ (np.uint64(hi) >> np.uint64(17))


class Keys:
    """The keys in use, so that none is made twice, and the crafted ones with their abundances."""

    def __init__(self, rng, taken=()):
        self.rng = rng
        self.used = set((int(lo), int(hi)) for lo, hi in taken)
        self.crafted = {}                       # (lo, hi) -> abundance
        self.next_ab = CRAFTED_AB

    def add(self, keys):
        """Give every key of the (n, 2) array an abundance of its own; returns the records."""
        rec = np.zeros(len(keys), dtype=formats.ABUNDANCE_DTYPE)
        for i, (lo, hi) in enumerate(keys):
            k = (int(lo), int(hi))
            assert k not in self.crafted
            self.used.add(k)
            self.crafted[k] = self.next_ab
            rec[i] = (lo, hi, self.next_ab)
            self.next_ab += 1
        return rec

    def arrays(self):
        lo = np.array([k[0] for k in self.crafted], dtype=np.uint64)
        hi = np.array([k[1] for k in self.crafted], dtype=np.uint64)
        ab = np.array(list(self.crafted.values()), dtype=np.uint32)
        return lo, hi, ab


def shadows(f, n, rng, used):
    """n distinct keys of fold f, no word zero, none of them in `used` (they are added to it)."""
    out = np.zeros((n, 2), dtype=np.uint64)
    i = 0
    while i < n:
        hi = np.uint64(rng.integers(1, 1 << 64, dtype=np.uint64))
        lo = np.uint64(f) ^ (hi >> np.uint64(17))
        if lo == 0 or (int(lo), int(hi)) in used:
            continue
        assert fold(lo, hi) == np.uint64(f)
        used.add((int(lo), int(hi)))
        out[i] = (lo, hi)
        i += 1
    return out


def twins(lo, hi, n, rng, used):
    """n keys (lo, hi ^ d), 1 <= d < 2^17 distinct: the low word AND the fold of (lo, hi), so they meet it at the first CAS."""
    out = np.zeros((n, 2), dtype=np.uint64)
    i = 0
    while i < n:
        d = np.uint64(rng.integers(1, 1 << 17))
        h = np.uint64(hi) ^ d
        if h == 0 or (int(lo), int(h)) in used:
            continue
        assert fold(lo, h) == fold(lo, hi)
        used.add((int(lo), int(h)))
        out[i] = (lo, h)
        i += 1
    return out


def neighbours(f, n, rng, used):
    """One key of each of the folds f + 1 .. f + n (mod 2^64): a capacity is at most 2^31, so 2^33 consecutive folds share a home (or
    sit in the next one) -- another cluster in the same slots."""
    return np.concatenate([shadows(np.uint64((int(f) + 1 + i) & M64), 1, rng, used) for i in range(n)])


def _records(lo, hi, ab):
    rec = np.zeros(len(lo), dtype=formats.ABUNDANCE_DTYPE)
    rec["lo"], rec["hi"], rec["abundance"] = lo, hi, ab
    return rec


def _expect(table: dict, lo, hi):
    """What the reference's map answers: a record of abundance 1 is not loaded (loadRefinedAbundances), absent gives 0."""
    out = np.zeros(len(lo), dtype=np.uint32)
    for i, (l, h) in enumerate(zip(lo, hi)):
        a = table.get((int(l), int(h)), 0)
        out[i] = 0 if a == 1 else a
    return out


def _check_lookup(t, table: dict, queries, rng):
    q = np.asarray(queries, dtype=np.uint64).reshape(-1, 2)
    q = q[rng.permutation(len(q))]
    got = t.lookup(q[:, 0], q[:, 1])
    exp = _expect(table, q[:, 0], q[:, 1])
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, [(hex(int(q[i, 0])), hex(int(q[i, 1])), int(got[i]), int(exp[i])) for i in bad[:8]]


def _ordinary_table_works(ctx, rng):
    keys = rng.integers(1, 1 << 64, (3000, 2), dtype=np.uint64)
    ab = rng.integers(1, 900, 3000).astype(np.uint32)
    t = ctx.prev_from_records(_records(keys[:, 0], keys[:, 1], ab))
    table = {(int(l), int(h)): int(a) for (l, h), a in zip(keys, ab)}
    _check_lookup(t, table, np.concatenate([keys, rng.integers(1, 1 << 64, (500, 2), dtype=np.uint64)]), rng)


# ---- 1. crafted keys alone ----------------------------------------------------------------------------------------------------

def test_cluster_sizes(ctx):
    """One cluster of each size 1, 2, 3, 4, 7, 48, 96, 97 in one table: 2 fills the home sector, 3 one bucket, 4 spills one, 97 is the
    longest chain that fits (probes 0 .. 96).  Fold 2^64 - 1 -- the LAST sector at any capacity -- has the 48, so its chain runs on
    through slots 0 .. 45, where fold 0's cluster of 7 has its home: the two share a run across the table's end (55 slots, within the
    limit in whatever order the rows arrive).  The other folds are a tenth of the fold space apart, more than 97 slots at the 1024-slot
    floor.  Asked: every key; absent keys of every cluster's fold (they walk the whole chain to an empty slot, to the limit at 97); an
    absent twin of every key; random absent keys; one key of abundance 1 per cluster (a record that is not loaded)."""
    rng = np.random.default_rng(11)
    K = Keys(rng)
    step = (1 << 64) // 10
    plan = [(7, 0), (48, M64), (1, 2 * step), (2, 3 * step + 12345), (3, 4 * step + 1), (4, 5 * step + 99), (96, 6 * step + 7), (97, 8 * step + 3)]
    rec, queries, ones = [], [], []
    for n, f in plan:
        keys = shadows(f, n, rng, K.used)
        rec.append(K.add(keys))
        queries.append(keys)
    present = np.concatenate(queries)
    for n, f in plan:
        queries.append(shadows(f, 5, rng, K.used))                          # absent, same chain
        one = shadows(f, 1, rng, K.used)                                    # in the file with abundance 1: not loaded
        ones.append(_records(one[:, 0], one[:, 1], [1]))
        queries.append(one)
    queries.append(np.concatenate([twins(lo, hi, 1, rng, K.used) for lo, hi in present]))
    queries.append(rng.integers(1, 1 << 64, (400, 2), dtype=np.uint64))
    raw = np.concatenate(rec + ones)
    raw = raw[rng.permutation(len(raw))]
    table = dict(K.crafted)
    assert len(table) == 258
    t = ctx.prev_from_records(raw)
    _check_lookup(t, table, np.concatenate(queries), rng)
    for lo, hi in present:                                                   # one at a time: a wave whose other lanes ask for nothing
        assert int(t.lookup(np.array([lo]), np.array([hi]))[0]) == table[(int(lo), int(hi))]


@pytest.mark.parametrize("layout", ["adjacent", "scattered"])
def test_low_word_twins(ctx, layout):
    """50 base keys with 2 to 6 twins each -- one low word, one home: the claim of a slot by its low word says nothing about whose
    slot it becomes.  Side by side in the record array they meet in one wave; scattered, across waves."""
    rng = np.random.default_rng(12)
    K = Keys(rng)
    groups = []
    for _ in range(50):
        base = shadows(np.uint64(rng.integers(1, 1 << 64, dtype=np.uint64)), 1, rng, K.used)
        groups.append(K.add(np.concatenate([base, twins(base[0, 0], base[0, 1], int(rng.integers(2, 7)), rng, K.used)])))
    filler = rng.integers(1, 1 << 64, (700, 2), dtype=np.uint64)
    fill_ab = rng.integers(2, 900, 700).astype(np.uint32)
    raw = np.concatenate(groups + [_records(filler[:, 0], filler[:, 1], fill_ab)])
    if layout == "scattered":
        raw = raw[rng.permutation(len(raw))]
    table = dict(K.crafted)
    table.update({(int(l), int(h)): int(a) for (l, h), a in zip(filler, fill_ab)})
    lo, hi, _ = K.arrays()
    absent = np.concatenate([twins(l, h, 1, rng, K.used) for l, h in zip(lo, hi)])
    t = ctx.prev_from_records(raw)
    _check_lookup(t, table, np.concatenate([np.stack([lo, hi], 1), filler, absent]), rng)


def _zero_word_keys(rng, n):
    """(0, x), (x, 0) and (0, 0): n keys in all."""
    x = rng.integers(1, 1 << 64, n, dtype=np.uint64)
    keys = np.zeros((n, 2), dtype=np.uint64)
    keys[: n // 2, 1] = x[: n // 2]
    keys[n // 2: n - 1, 0] = x[n // 2: n - 1]
    assert len(set(map(tuple, keys.tolist()))) == n
    return keys


@pytest.mark.parametrize("how", ["adjacent", "scattered", "bytes"])
def test_zero_word_keys(ctx, how):
    """64 keys with a zero word -- the side list's capacity -- first in the record array, so that the 64 lanes of one wave take the
    spin lock together, or scattered among 5000 ordinary keys, or scattered and uploaded as bytes.  All 64 are found; absent zero-word keys give 0.  ("adjacent" did not return before the lanes of
    a wave took the lock in turn: table_exc_upsert, csrc/table.hpp.)"""
    rng = np.random.default_rng(13)
    K = Keys(rng)
    zrec = K.add(_zero_word_keys(rng, 64))
    filler = rng.integers(1, 1 << 64, (5000, 2), dtype=np.uint64)
    fill_ab = rng.integers(2, 900, 5000).astype(np.uint32)
    raw = np.concatenate([zrec, _records(filler[:, 0], filler[:, 1], fill_ab)])
    if how != "adjacent":
        raw = raw[rng.permutation(len(raw))]
    table = dict(K.crafted)
    table.update({(int(l), int(h)): int(a) for (l, h), a in zip(filler, fill_ab)})
    absent = np.array([k for k in _zero_word_keys(rng, 40).tolist() if tuple(k) not in table], dtype=np.uint64)
    assert len(absent) >= 39
    if how == "bytes":
        t = ctx.prev_from_record_bytes(ctx.bytes_from_host(raw.tobytes()), len(raw))
    else:
        t = ctx.prev_from_records(raw)
    lo, hi, _ = K.arrays()
    _check_lookup(t, table, np.concatenate([np.stack([lo, hi], 1), absent, filler[:600], rng.integers(1, 1 << 64, (200, 2), dtype=np.uint64)]), rng)


@pytest.mark.parametrize("which", ["98_keys_of_one_fold", "65_zero_word_keys"])
def test_the_two_limits_are_clean_errors(ctx, which):
    """One key more than a probe sequence or the side list holds: MDBG_ERANGE with a message, and the context goes on working.  Both
    inserts are bounded: table_find_or_insert's loop runs limit + 1 times and then sets `overflow`; table_exc_upsert finds the list
    full under the lock (or, once it is full, before the lock) and sets `overflow`."""
    from metamdbg_amd import capi
    rng = np.random.default_rng(14)
    K = Keys(rng)
    keys = shadows(np.uint64(0x1234567890ABCDEF), 98, rng, K.used) if which == "98_keys_of_one_fold" else _zero_word_keys(rng, 65)
    with pytest.raises(capi.MdbgError) as e:
        ctx.prev_from_records(K.add(keys))
    assert e.value.code == MDBG_ERANGE and "overflow" in str(e.value)
    _ordinary_table_works(ctx, rng)


# ---- 2. crafted keys around real ones -----------------------------------------------------------------------------------------

def _inputs(rng, k, genome_len, n_reads, max_len, unitig_lens, read_span=None):
    """The inputs of test_gpu_parity.test_refined_and_index_vs_oracle: a genome of distinct minimizers, reads = random substrings (of
    its first `read_span`) in either orientation, a quarter with one "error", unitigs = disjoint genome segments."""
    genome = rng.permutation(genome_len).astype(np.uint32)
    span = read_span or genome_len
    rl = []
    for _ in range(n_reads):
        n = int(rng.integers(0, max_len)); a = int(rng.integers(0, max(1, span - n)))
        seg = genome[a:min(a + n, span)]
        if rng.integers(0, 2): seg = seg[::-1]
        seg = seg.copy()
        if len(seg) and rng.integers(0, 4) == 0: seg[int(rng.integers(0, len(seg)))] = genome_len + 1000 + int(rng.integers(0, 50))
        rl.append(seg)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in rl])]).astype(np.uint64)
    mins = np.concatenate(rl).astype(np.uint32)
    return genome, mins, offs


def _unitigs(genome, spans):
    ul = [genome[a:b] for a, b in spans]
    uoffs = np.concatenate([[0], np.cumsum([len(x) for x in ul])]).astype(np.uint64)
    return np.concatenate(ul).astype(np.uint32), uoffs


def _window_keys(orc, mins, offs, kw, at_least):
    """(lo, hi) of every kw-window of the sequences that hold `at_least` minimizers or more."""
    out = set()
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        if b - a >= at_least:
            for i in range(a, b - kw + 1):
                _, _, hi, lo = orc.kminmer_normalize_hash(mins[i:i + kw])
                out.add((lo, hi))
    return out


def _windows_asked(orc, allm, alloff, k):
    """The (k-1)-windows the passes at k look up: those of the sequences that hold a k-window."""
    return _window_keys(orc, allm, alloff, k - 1, k)


def _interleave(rng, singles, blocks):
    """Rows in a random order, the rows of every block staying side by side."""
    items = [singles[i:i + 1] for i in range(len(singles))] + list(blocks)
    return np.concatenate([items[i] for i in rng.permutation(len(items))])


class Scenario:
    pass


def _finish(S, orc, rng, real, K, singles, blocks, uab):
    """The record set, the oracle's previous table with and without the crafted rows (overlaid alike), and what the passes must give."""
    assert int(real["abundance"].max()) < CRAFTED_AB and S.k > 0
    S.real = real
    S.raw = _interleave(rng, np.concatenate(singles), blocks)
    assert len(S.raw) == len(real) + len(K.crafted)
    keys = list(zip(S.raw["lo"].tolist(), S.raw["hi"].tolist()))
    assert len(set(keys)) == len(keys)                                       # a file never holds a key twice
    S.crafted = K.arrays()
    S.uab = uab
    over = [(S.umins[int(S.uoffs[i]): int(S.uoffs[i + 1])], int(a)) for i, a in enumerate(uab) if a != 0xFFFFFFFF]
    S.oprev_plain = orc.PrevAbundance(S.raw.tobytes())
    S.oprev = orc.PrevAbundance(S.raw.tobytes())
    S.oprev.overlay_unitigs(over, S.k - 1)
    S.oprev_real = orc.PrevAbundance(real.tobytes())
    S.oprev_real.overlay_unitigs(over, S.k - 1)
    S.exp, S.exp_real = {}, {}
    for name, prev in (("exp", S.oprev), ("exp_real", S.oprev_real)):
        getattr(S, name).update(refined=orc.kminmer_count_refined(S.allm, S.alloff, S.k, prev), index=orc.kminmer_index(S.allm, S.alloff, S.k, prev),
                                small=orc.small_contigs(S.umins, S.uoffs, S.k, S.k - 1, prev))
    return S


_SCENARIOS = {}


def _scenario(orc, k):
    """A genome of 3000 minimizers, 600 reads, 14 unitigs (four of exactly k - 1 minimizers, the only length the small-contig branch
    flags); the previous table at k - 1 from the oracle; around 300 of its keys a cluster each -- a third 1 to 3 shadows, a third 4 to
    12, the rest shadows, twins of the real key and neighbours --, and clusters around the real keys of the largest and of the smallest
    fold.  The home of the first is within a few slots of the table's end and that of the second within a few slots of slot 0, so the
    two clusters are ONE run of occupied slots across the end, and that run has to stay within the probe limit in whatever order the
    rows arrive: 60 shadows and 8 together, not 60 and 60.  With the keys that live there the run is 78 slots at k = 5 and 63 at k = 13
    for SEED at the capacity mdbg_prev_from_records gives these record sets (laid out on the CPU when the seed was chosen; other seeds
    gave 63 to 109): a change of the table's sizing that lengthens it past 97 shows here as MDBG_ERANGE, not as a wrong answer.  At k = 5 the largest fold has the 60 (its chain wraps at the table's end,
    its twenty full buckets at the image's) and at k = 13 the smallest (a chain that starts where the other's wrap arrives).  Half of the
    clusters have their rows side by side in the file, the real key's among them."""
    if k in _SCENARIOS:
        return _SCENARIOS[k]
    rng = np.random.default_rng(SEED + k)
    S = Scenario()
    S.k = k
    lens = [k - 1] * 4 + [k - 2, k, k + 1, 3] + [int(x) for x in rng.integers(150, 420, 6)]
    starts = 3000 - sum(lens) + np.concatenate([[0], np.cumsum(lens)])       # the unitigs are the genome's end; no read covers the last two
    genome, S.mins, S.offs = _inputs(rng, k, 3000, 600, 80, None, read_span=int(starts[12]))
    S.umins, S.uoffs = _unitigs(genome, list(zip(starts[:-1], starts[1:])))
    S.allm = np.concatenate([S.mins, S.umins]); S.alloff = np.concatenate([S.offs, S.offs[-1] + S.uoffs[1:]])
    real = orc.table_abundance_records(orc.kminmer_count_first(S.allm, S.alloff, k - 1, 0))
    # the windows only those two unitigs have were counted once (the first pass writes such a row only for a rescued read): rows of
    # abundance 1, which are not loaded -- keys the overlay INSERTS, behind whatever shadows they have
    table = dict(zip(zip(real["lo"].tolist(), real["hi"].tolist()), real["abundance"].tolist()))
    once = _window_keys(orc, S.umins, S.uoffs[12:], k - 1, k - 1)
    assert len(once) > 300 and all(table.get(kk, 1) == 1 for kk in once)
    once = sorted(kk for kk in once if kk not in table)
    real = np.concatenate([real, _records([kk[0] for kk in once], [kk[1] for kk in once], [1] * len(once))])
    K = Keys(rng, zip(real["lo"].tolist(), real["hi"].tolist()))
    folds = real["lo"] ^ (real["hi"] >> np.uint64(17))
    top, bottom = int(np.argmax(folds)), int(np.argmin(folds))
    # (a capacity of up to 120 000 slots puts the home of `top` within 60 slots of the end: the chain of 61 wraps)
    assert int(folds[top]) >= M64 - M64 // 2000 and int(folds[bottom]) <= M64 // 2000
    rest = np.setdiff1d(np.arange(len(real)), [top, bottom])
    chosen = rng.choice(rest, 300, replace=False)
    S.shadowed = np.concatenate([chosen, [top, bottom]])
    singles, blocks, in_block = [], [], set()
    for j, r in enumerate(S.shadowed):
        lo, hi, f = real["lo"][r], real["hi"][r], folds[r]
        if j >= 300:
            keys = shadows(f, 60 if (j == 300) == (k == 5) else 8, rng, K.used)
        elif j % 3 == 0:
            keys = shadows(f, int(rng.integers(1, 4)), rng, K.used)
        elif j % 3 == 1:
            keys = shadows(f, int(rng.integers(4, 13)), rng, K.used)
        else:
            keys = np.concatenate([shadows(f, int(rng.integers(1, 5)), rng, K.used), twins(lo, hi, int(rng.integers(1, 4)), rng, K.used),
                                   neighbours(f, int(rng.integers(1, 4)), rng, K.used)])
        rec = K.add(keys)
        if j % 2 == 0:
            rec = np.concatenate([rec, real[r:r + 1]])
            blocks.append(rec[rng.permutation(len(rec))])
            in_block.add(int(r))
        else:
            singles.append(rec)
    singles.append(real[[i for i in range(len(real)) if i not in in_block]])
    # unitig abundances: 0, 1, 2, 5 and "none" over the long unitigs and the short ones alike
    uab = np.array([2, 0, 1, 5, 0xFFFFFFFF, 2, 0, 1, 1, 5, 0xFFFFFFFF, 3, 2, 0], dtype=np.uint32)
    assert len(uab) == len(lens)
    S.asked = _windows_asked(orc, S.allm, S.alloff, k)
    _SCENARIOS[k] = _finish(S, orc, rng, real, K, singles, blocks, uab)
    return S


def _alone(folds, f, before, after):
    """No other fold of `folds` (which holds f once) in [f - before, f + after], both ends inside the fold space."""
    if f - before < 0 or f + after > M64:
        return False
    return sum(f - before <= o <= f + after for o in folds) == 1


def _limit_scenario(orc):
    """The probe limit under the passes, k = 5, in a table so sparse that whole clusters of 97 fit (see the module's docstring).  A genome
    of 60 minimizers; 25 reads from its first 40; unitigs: [5, 25) with abundance 5, [40, 50) with abundance 2, [50, 60) with abundance 1.
    No read covers the last two, so their 4-windows were counted once: the record set has them with abundance 1, records that are not
    loaded.  Three real keys get 96 shadows each:
      A2, a window of the unitig with abundance 1 -- never in the table; a look-up of it walks the 96 occupied slots and says "missing, so 1";
      A1, a window of the unitig with abundance 2 -- the overlay inserts it behind its 96 shadows, at probe 96, the last a look-up makes;
      B,  a real key of abundance >= 2, one of a cluster of exactly 97, wherever the device's order puts it.
    Each of the three folds is alone -- among the folds of the rows and of every window the overlay may insert -- from 14 slots below
    to 99 slots above its home at 5120 slots, the least a record file's table has (table_slots_for(.) >= 1024, + 4096 for the overlay);
    at a larger capacity the same folds span fewer slots."""
    if "limit" in _SCENARIOS:
        return _SCENARIOS["limit"]
    k = 5
    rng = np.random.default_rng(77)
    S = Scenario()
    S.k = k
    genome, S.mins, S.offs = _inputs(rng, k, 60, 25, 30, None, read_span=40)
    S.umins, S.uoffs = _unitigs(genome, [(5, 25), (40, 50), (50, 60)])
    uab = np.array([5, 2, 1], dtype=np.uint32)
    S.allm = np.concatenate([S.mins, S.umins]); S.alloff = np.concatenate([S.offs, S.offs[-1] + S.uoffs[1:]])
    real = orc.table_abundance_records(orc.kminmer_count_first(S.allm, S.alloff, k - 1, 0))
    S.asked = _windows_asked(orc, S.allm, S.alloff, k)
    table = dict(zip(zip(real["lo"].tolist(), real["hi"].tolist()), real["abundance"].tolist()))
    of_unitig = [_window_keys(orc, S.umins, S.uoffs[u:u + 2], k - 1, k) for u in range(3)]
    # the windows only a unitig has were counted once; the first pass writes such a row only for a rescued read: add the others
    once = sorted(kk for kk in (of_unitig[1] | of_unitig[2]) if kk not in table)
    assert len(once) >= 12 and all(table.get(kk, 1) == 1 for kk in of_unitig[1] | of_unitig[2])
    real = np.concatenate([real, _records([kk[0] for kk in once], [kk[1] for kk in once], [1] * len(once))])
    table.update((kk, 1) for kk in once)
    universe = sorted(set(table) | of_unitig[0])
    folds = [lo ^ (hi >> 17) for lo, hi in universe]
    slot = (1 << 64) // 5120
    alone = [kk for kk, f in zip(universe, folds) if _alone(folds, f, 14 * slot, 99 * slot)]
    a1 = [kk for kk in alone if kk in of_unitig[1]]
    a2 = [kk for kk in alone if kk in of_unitig[2]]
    b = [kk for kk in alone if table.get(kk, 0) >= 2 and kk in S.asked]
    assert a1 and a2 and b, (len(real), len(alone), a1, a2, b)
    row = {kk: i for i, kk in enumerate(zip(real["lo"].tolist(), real["hi"].tolist()))}
    S.A1, S.A2, S.B = row[a1[0]], row[a2[0]], row[b[0]]
    S.shadowed = np.array([S.A1, S.A2, S.B])
    K = Keys(rng, table)
    fold_of = lambda r: np.uint64(real["lo"][r]) ^ (np.uint64(real["hi"][r]) >> np.uint64(17))
    blocks = [K.add(shadows(fold_of(S.A1), 96, rng, K.used))]                # side by side
    singles = [K.add(shadows(fold_of(S.A2), 96, rng, K.used)), K.add(shadows(fold_of(S.B), 96, rng, K.used)), real]
    _SCENARIOS["limit"] = _finish(S, orc, rng, real, K, singles, blocks, uab)
    return S


def _device_side(ctx, S, overlay=True):
    d_reads = ctx.minimizers_from_host(S.mins, S.offs)
    d_unitigs = ctx.minimizers_from_host(S.umins, S.uoffs)
    dprev = ctx.prev_from_records(S.raw)
    if overlay:
        ctx.prev_overlay_unitigs(dprev, d_unitigs, S.uab, S.k - 1)
    return d_reads, d_unitigs, dprev


def _check_prev(dprev, oprev, S):
    """The table against the oracle's map, key for key; the crafted keys keep their values; keys of abundance 1 that no overlay touched are absent."""
    ohi, olo, oab = oprev.arrays()
    assert np.array_equal(dprev.lookup(olo, ohi), oab)
    clo, chi, cab = S.crafted
    assert np.array_equal(dprev.lookup(clo, chi), cab)
    have = set(zip(olo.tolist(), ohi.tolist()))
    gone = np.array([(l, h) for l, h in zip(S.real["lo"].tolist(), S.real["hi"].tolist()) if (l, h) not in have], dtype=np.uint64).reshape(-1, 2)
    assert not dprev.lookup(gone[:, 0], gone[:, 1]).any()


def _check_passes(ctx, S, form):
    d_reads, d_unitigs, dprev = _device_side(ctx, S)
    with _table_form(ctx, form):
        rec, vec = ctx.kminmer_count_refined(d_reads, d_unitigs, S.k, dprev).to_host()
        _assert_tables_equal(rec, vec, S.exp["refined"], S.k)
        rec, vec = ctx.kminmer_index(d_reads, d_unitigs, S.k, dprev).to_host()
        _assert_tables_equal(rec, vec, S.exp["index"], S.k)
    assert np.array_equal(ctx.small_contigs(d_unitigs, S.k, S.k - 1, dprev), S.exp["small"])
    _check_prev(dprev, S.oprev, S)                                           # the passes read the table, and leave it as it was


@pytest.mark.parametrize("which", [5, 13, "limit"])
def test_shadows_are_absent_keys_to_the_reference_and_stand_where_the_passes_ask(orc, which):
    """The oracle's results with the crafted rows equal its results with the real rows alone; the shadowed real keys are (k-1)-windows
    the passes look up (250 of 300 at the least; all three at the limit); the results are not empty."""
    S = _limit_scenario(orc) if which == "limit" else _scenario(orc, which)
    for name in ("refined", "index"):
        a, b = S.exp[name], S.exp_real[name]
        assert a["n"] > 0 and a["n"] == b["n"]
        assert np.array_equal(formats.sorted_abundance_records(orc.table_abundance_records(a)), formats.sorted_abundance_records(orc.table_abundance_records(b)))
    assert np.array_equal(S.exp["small"], S.exp_real["small"])
    if which != "limit":
        assert S.exp["small"].any() and not S.exp["small"].all()
    n_asked = sum((int(S.real["lo"][r]), int(S.real["hi"][r])) in S.asked for r in S.shadowed)
    print("shadowed real keys the passes ask for:", n_asked, "of", len(S.shadowed))
    assert n_asked >= (3 if which == "limit" else 250)


@pytest.mark.parametrize("k", [5, 13])
def test_lookup_of_real_keys_among_shadows(ctx, orc, k):
    """mdbg_table_lookup over every real key equals the oracle's map, over every crafted key its own abundance -- before any overlay."""
    S = _scenario(orc, k)
    _, _, dprev = _device_side(ctx, S, overlay=False)
    _check_prev(dprev, S.oprev_plain, S)
    rng = np.random.default_rng(5)
    clo, chi, _ = S.crafted
    used = set(zip(S.raw["lo"].tolist(), S.raw["hi"].tolist()))
    absent = np.concatenate([twins(l, h, 1, rng, used) for l, h in zip(clo[::3], chi[::3])])
    assert not dprev.lookup(absent[:, 0], absent[:, 1]).any()


def test_overlay_finds_and_inserts_along_chains(ctx, orc):
    """mdbg_prev_overlay_unitigs with abundances 0, 1, 2, 5 and "none" over unitigs whose (k-1)-windows are shadowed keys: overlay_kernel's
    find (abundance 1: set to 0 if present) and find-or-insert along a chain; the crafted keys keep their values."""
    S = _scenario(orc, 5)
    # every abundance meets shadowed keys among its unitigs' windows
    shadowed = set((int(S.real["lo"][r]), int(S.real["hi"][r])) for r in S.shadowed)
    for a in (0, 1, 2, 5, 0xFFFFFFFF):
        n = sum(len(shadowed & _window_keys(orc, S.umins, S.uoffs[u:u + 2], S.k - 1, S.k - 1)) for u in np.flatnonzero(S.uab == a))
        assert n >= 5, (a, n)
    _, _, dprev = _device_side(ctx, S)
    _check_prev(dprev, S.oprev, S)
    ohi, olo, oab = S.oprev.arrays()
    phi, plo, pab = S.oprev_plain.arrays()
    shadowed_new = sum(kk in shadowed for kk in set(zip(olo.tolist(), ohi.tolist())) - set(zip(plo.tolist(), phi.tolist())))
    assert len(olo) > len(plo) + 200 and shadowed_new >= 20                  # the overlay inserted keys, a score of them behind shadows
    before = dict(zip(zip(plo.tolist(), phi.tolist()), pab.tolist()))
    assert sum(before.get(kk) not in (None, v) for kk, v in zip(zip(olo.tolist(), ohi.tolist()), oab.tolist())) > 100   # ... and changed values


def _passes_cases():
    return [(5, f) for f in FORMS] + [(13, f) for f in ("slots", "slots_round4", "buckets")]


@pytest.mark.parametrize("k,form", _passes_cases())
def test_passes_with_shadowed_previous_table(ctx, orc, k, form):
    """kminmer_count_refined, kminmer_index and small_contigs in every form against the oracle, the previous table full of clusters
    around the keys they ask for: k = 5 in every form, k = 13 (the generic window hash) in the default form, the narrow look-up and the
    bucket image."""
    _check_passes(ctx, _scenario(orc, k), form)


@pytest.mark.parametrize("form", FORMS)
def test_passes_at_the_probe_limit(ctx, orc, form):
    """The same over _limit_scenario: a key behind 96 shadows at the last probe, a key that is missing behind 96 shadows, a cluster of 97."""
    S = _limit_scenario(orc)
    _check_passes(ctx, S, form)


def test_lookups_at_the_probe_limit(ctx, orc):
    """Before the overlay A1 and A2 are missing behind their 96 shadows; after it A1 has the unitig's abundance at probe 96, A2 is
    still missing (abundance 1 sets a key to 0 only where it is present), B has its own value in its cluster of 97."""
    S = _limit_scenario(orc)
    lo, hi, ab = S.real["lo"][S.shadowed], S.real["hi"][S.shadowed], S.real["abundance"][S.shadowed]
    assert ab[0] == 1 and ab[1] == 1 and ab[2] >= 2
    _, _, dprev = _device_side(ctx, S, overlay=False)
    _check_prev(dprev, S.oprev_plain, S)
    assert list(dprev.lookup(lo, hi)) == [0, 0, ab[2]]
    _, _, dprev = _device_side(ctx, S)
    _check_prev(dprev, S.oprev, S)
    assert list(dprev.lookup(lo, hi)) == [2, 0, ab[2]]
