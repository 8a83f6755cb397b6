"""The candidate hash with the finalisers' upper half shared (murmur.hpp: kmer_hash32_hi_shared_x2) in the block kernel's position
loops (scan.hip, scan_fast_kernel): exact unless a position's guard word is below 68, and a lane that saw one walks its span again
with the exact test.  Two things can go wrong -- a guard value that is not caught, and the slow path itself -- so:

  * the 65 keys that fail the guard (tests/test_murmur_shared_hi_host.py lists them) are PLANTED as l-mers, forward and reverse
    complement, where the walks differ: a full block's first and second half span, a lane's first and last position, the tail's
    chain a and chain b, the last lane of a tail with odd P;
  * "scan_guard_slack" sends practically every span down the slow path, on reads whose lengths sit on the block borders.

Values, positions, directions and counts per read against the oracle.  Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import formats, synth

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
# the keys below 2^30 whose guard word is below 68, and the one key below 2^32 without equal adjacent digits that fails it
FAILING_BELOW_2_30 = [18684438, 62257441, 95494466, 172304494, 421419016, 498229044, 531466069, 550150507, 583387532, 626960535,
                      660197560, 737007588, 986122110, 1062932138]
FAILING_REPEAT_FREE_16 = 3871895021


def guard_word(v):
    """bl of kmer_hash32_hi_shared: lo((rotl64(v * c1, 31) * c2)) ^ 34, + 68 in 32 bits."""
    k = (v * 0x87c37b91114253d5) & M64
    k = ((k << 31) | (k >> 33)) & M64
    k = (k * 0x4cf5ad432745937f) & M64
    return (((k & M32) ^ 34) + 68) & M32


def revcomp_value(v, l):
    out = 0
    for i in range(l):
        out = (out << 2) | (((v >> (2 * i)) & 3) ^ 2)
    return out


def lmer_codes(v, l):
    """The l bases whose forward k-mer is v: the first base is the top digit."""
    return np.array([(v >> (2 * (l - 1 - i))) & 3 for i in range(l)], dtype=np.int64)


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


def _scan_lists(ctx, seqs, K, density, hpc):
    reads = ctx.reads_from_ascii(seqs)
    h = ctx.scan(reads, K=K, density=density, hpc=hpc, apply_read_filters=False).to_host()
    reads.free()
    assert len(h["offsets"]) == len(seqs) + 1
    out = []
    for i in range(len(seqs)):
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        out.append((h["minimizers"][a:b].tolist(), h["pos"][a:b].tolist(), h["dir"][a:b].tolist()))
    return out


_oracle_cache = {}


def _oracle_lists(orc, key, seqs, K, density, hpc):
    k = (key, K, density, hpc)
    if k not in _oracle_cache:
        _oracle_cache[k] = [tuple(list(x) for x in orc.minimizer_parse(s, K, density, hpc)) for s in seqs]
    return _oracle_cache[k]


def _assert_same(got, exp, what):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert len(g[0]) == len(e[0]), (what, i, len(g[0]), len(e[0]))
        assert g == e, (what, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# planted guard values
# ---------------------------------------------------------------------------------------------------------------------------------
CATEGORIES = ("block first half", "block second half", "lane first", "lane last", "tail chain a", "tail chain b", "odd P last lane")
_planted = {}


def _planted_reads(l, repeat_free, lengths=(2100, 9001), values=None):
    """64 random reads of 2.1 - 9 kb (uncompressed: a position is a base offset) with the failing keys of this l, forward and
    reverse complement, written at offsets that fall into every part of the walks.  Returns (reads, plants, categories hit):
    plants = per read a list of (offset, key).  repeat_free: no two equal adjacent bases anywhere, so that homopolymer
    compression leaves the reads -- and the offsets -- as they are.  (lengths, values: another range of lengths, some of the keys.)"""
    if (l, repeat_free, lengths) in _planted:
        return _planted[(l, repeat_free, lengths)]
    if values is None:
        values = [FAILING_REPEAT_FREE_16] if repeat_free else [v for v in FAILING_BELOW_2_30 if v < (1 << (2 * l))]
    assert values and all(guard_word(v) < 68 for v in values)
    forms = [w for v in values for w in (v, revcomp_value(v, l))]
    rng = np.random.default_rng(7000 + l + lengths[0])
    seqs, plants, hit, turn = [], [], {c: 0 for c in CATEGORIES}, 0
    for r in range(64):
        n = int(rng.integers(*lengths))
        if repeat_free:
            c = np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) & 3     # every base differs from the last
        else:
            c = rng.integers(0, 4, n)
        nblocks = (n - l - 1) // 2048            # blocks run while length - done >= 2048 + l + 1 (the end trim)
        tail0 = 2048 * nblocks
        npos = n - l - tail0                     # positions left to the tail
        P = (npos + 63) // 64
        Ph = (P + 1) // 2
        last_lane = (npos - 1) // P
        blk = 2048 * int(rng.integers(0, max(nblocks, 1)))
        lanes = rng.choice(np.arange(1, 63), 4, replace=False)
        # (in order of precedence: a later offset within l + 2 of an earlier one is left out)
        cand = [(blk + 32 * int(lanes[2]), "lane first"), (blk + 32 * int(lanes[3]) + 31, "lane last"),
                (blk + 32 * int(lanes[0]) + int(rng.integers(1, 15)), "block first half"),
                (blk + 32 * int(lanes[1]) + int(rng.integers(17, 31)), "block second half")] if nblocks else []
        tl = rng.choice(np.arange(0, max(last_lane, 1)), min(3, max(last_lane, 1)), replace=False)
        cand += [(tail0 + int(t) * P + j, cat) for t, (j, cat) in zip(tl, [(0, "tail chain a"), (Ph if Ph < P else 0, "tail chain b" if Ph < P else "tail chain a"),
                                                                       (P - 1, "tail chain b" if P > 1 else "tail chain a")])]
        if P % 2 == 1:                           # the last lane: its first position, and the read's last position
            cand = [(tail0 + last_lane * P, "odd P last lane"), (tail0 + npos - 1, "odd P last lane")] + cand
        taken, mine = [], []
        for off, cat in cand:
            if off < 1 or off > n - l - 1 or any(abs(off - t) < l + 2 for t in taken):
                continue
            v = forms[turn % len(forms)]; turn += 1
            c[off:off + l] = lmer_codes(v, l)
            taken.append(off); mine.append((off, min(v, revcomp_value(v, l)))); hit[cat] += 1
        if repeat_free:                          # mend the borders of the planted l-mers (they are repeat-free themselves)
            fixed = np.zeros(n, dtype=bool)
            for off in taken: fixed[off:off + l] = True
            for i in range(1, n):
                if c[i] == c[i - 1]:
                    j = i if not fixed[i] else i - 1
                    assert not fixed[j]
                    c[j] = next(x for x in range(4) if x != c[j - 1] and (j + 1 >= n or x != c[j + 1]))
            assert not np.any(c[1:] == c[:-1])
        seqs.append(bytes(synth.CODE2ASCII[c])); plants.append(mine)
    _planted[(l, repeat_free, lengths)] = (seqs, plants, hit)
    return _planted[(l, repeat_free, lengths)]


def _hashed_keys(l, repeat_free):
    """The keys the planted l-mers are hashed by: the failing keys that are their own canonical form (a key above its reverse
    complement is never hashed: 8 of the 14 at l = 15, 2 of the 4 at l = 14).  At l = 13 neither of the two failing keys is one, nor
    is the one repeat-free key at l = 16 -- planting them shows just that -- and there the canonical forms of the planted l-mers stand
    in for the density choice and the selected / rejected count."""
    values = [FAILING_REPEAT_FREE_16] if repeat_free else [v for v in FAILING_BELOW_2_30 if v < (1 << (2 * l))]
    canon = sorted({v for v in values if v <= revcomp_value(v, l)})
    assert canon or l in (13, 16), "no failing key of this l is a canonical form"
    return canon or sorted({min(v, revcomp_value(v, l)) for v in values})


def _high_densities(orc, l, repeat_free):
    """Densities near 0.5 at which at least one of the hashed planted keys is selected and one rejected: half way between the two
    hashes next to 2^63.  With a single key (l = 16) no one density can do both: two densities then, 0.02 of the hash range to
    either side of its hash."""
    canon = _hashed_keys(l, repeat_free)
    f = sorted(orc.kmer_hash(v) / 2.0 ** 64 for v in canon)
    if len(f) == 1:
        return [min(max(f[0] - 0.02, 0.01), 0.98), min(max(f[0] + 0.02, 0.02), 0.99)]
    i = min(range(len(f) - 1), key=lambda i: abs((f[i] + f[i + 1]) / 2 - 0.5))
    return [(f[i] + f[i + 1]) / 2]


@pytest.mark.parametrize("l,hpc", [(15, False), (14, False), (13, False), (16, True)])
def test_planted_guard_values_vs_oracle(ctx, orc, l, hpc):
    """At 0.005 a planted key is rejected and the guard shows in the span around it: the slow path must find that span's real
    minimizers.  A batch at a density of 0.2 or more is not given to the block kernel at all (mdbg_scan: its reads would outgrow
    the stage of 384 rows), so the density near 0.5 checks that routing, and test_planted_guard_values_within_the_stage is where a
    SELECTED planted key has to come out of the block kernel itself."""
    seqs, plants, hit = _planted_reads(l, hpc)
    assert all(hit[c] > 0 for c in CATEGORIES), hit
    counted = set(_hashed_keys(l, hpc))
    assert l in (13, 16) or all(guard_word(v) < 68 for v in counted)
    assert counted <= {v for p in plants for _, v in p}
    selected = rejected = 0
    high = _high_densities(orc, l, hpc)
    for density in [0.005] + high:
        exp = _oracle_lists(orc, ("planted", l, hpc), seqs, l, density, hpc)
        if density != 0.005:
            for e, p in zip(exp, plants):
                at = dict(zip(e[1], e[0]))
                for off, v in p:
                    if v not in counted: continue
                    if off in at:
                        assert at[off] == v          # the l-mer really is where it was written, and this is its key
                        selected += 1
                    else:
                        rejected += 1
        _assert_same(_scan_lists(ctx, seqs, l, density, hpc), exp, (l, hpc, density))
    print("planted l-mers, by the keys they are hashed by: selected %d, rejected %d at densities %s; categories %s" % (selected, rejected, high, hit))
    assert selected > 0 and rejected > 0


STAGE_ROWS = 384      # scan.hip, STAGE_CAP: a read with more minimizers is re-run by the general kernel


@pytest.mark.parametrize("lengths,fmax", [((2100, 3001), 0.1), ((300, 1301), 0.2)])
def test_planted_guard_values_within_the_stage(ctx, orc, lengths, fmax):
    """A wrong hash for a failing key shows only where the key is SELECTED (a false candidate is confirmed with the full hash and its
    read re-run) and the batch and its read stay on the block kernel: density below 0.2, mean length x density x 1.4 + 24 below the
    stage's 384 rows (mdbg_scan), at most 384 minimizers in the read.  Two of the canonical failing keys at l = 15 hash that low:
    421419016 (0.0875 of the hash range: reads of one block and a tail) and 583387532 (0.1844: both keys, short reads, tails only).
    At l = 14 the two canonical failing keys hash to 0.52 and 0.70: no batch that selects them runs on the block kernel."""
    l = 15
    f = {v: orc.kmer_hash(v) / 2.0 ** 64 for v in _hashed_keys(l, False)}
    keys = sorted(v for v in f if f[v] < fmax)
    assert keys and all(guard_word(v) < 68 for v in keys)
    density = max(f[v] for v in keys) + 0.003
    seqs, plants, _ = _planted_reads(l, False, lengths, keys)
    assert density < 0.2 and sum(len(s) for s in seqs) / len(seqs) * density * 1.4 + 24 < STAGE_ROWS        # the batch goes to the block kernel
    exp = _oracle_lists(orc, ("planted", l, lengths), seqs, l, density, False)
    staged = sum(1 for e, p in zip(exp, plants) if len(e[0]) <= STAGE_ROWS for off, _ in p if off in e[1])
    outgrowing = sum(1 for e in exp if len(e[0]) > STAGE_ROWS)
    print("lengths %s, density %.4f: %d selected planted l-mers in reads that stay in the stage; %d of %d reads outgrow it" % (lengths, density, staged, outgrowing, len(seqs)))
    assert staged >= 10 and outgrowing <= len(seqs) // 4
    _assert_same(_scan_lists(ctx, seqs, l, density, False), exp, (lengths, density))


def test_planted_reads_compressed_l15_control(ctx, orc):
    """The same reads under homopolymer compression at l = 15: the unguarded instantiation (no compressed window is a failing key)."""
    seqs, _, _ = _planted_reads(15, False)
    for density in (0.005, _high_densities(orc, 15, False)[0]):
        _assert_same(_scan_lists(ctx, seqs, 15, density, True), _oracle_lists(orc, ("planted", 15, False), seqs, 15, density, True),
                     ("control", density))


# ---------------------------------------------------------------------------------------------------------------------------------
# the slow path everywhere
# ---------------------------------------------------------------------------------------------------------------------------------
_border = {}


def _border_reads(l, hpc):
    """Reads of 2047 + l, 2048 + l, 2049 + l and 4096 + l compressed bases (six each), one shorter than l, one of exactly l bases and
    eight of any length; with compression the reads are repeat-free sequences of those lengths with every fourth run stretched."""
    if (l, hpc) not in _border:
        rng = np.random.default_rng(8100 + 2 * l + int(hpc))
        lens = [x + l for x in (2047, 2048, 2049, 4096) for _ in range(6)] + [l - 1, l] + [int(x) for x in rng.integers(40, 7000, 8)]
        out = []
        for n in lens:
            if hpc:
                c = np.cumsum(np.concatenate([rng.integers(0, 4, 1), rng.integers(1, 4, n - 1)])) & 3
                c = np.repeat(c, rng.choice([1, 1, 1, 3], n))
            else:
                c = rng.integers(0, 4, n)
            out.append(bytes(synth.CODE2ASCII[c]))
        _border[(l, hpc)] = out
    return _border[(l, hpc)]


_plain = {}


@pytest.mark.parametrize("slack", [1 << 26, 1 << 31])
@pytest.mark.parametrize("l", [15, 13])
@pytest.mark.parametrize("hpc", [False, True])
def test_slow_path_everywhere_vs_oracle(ctx, orc, hpc, l, slack):
    seqs = _border_reads(l, hpc)
    density = 0.05
    exp = _oracle_lists(orc, ("border",), seqs, l, density, hpc)
    if hpc:      # the compressed lengths are the ones asked for
        assert [orc.read_selection(s, None, K=l, density=density, hpc=True)["hpc_length"] for s in seqs[:24:6]] == [x + l for x in (2047, 2048, 2049, 4096)]
    if (l, hpc) not in _plain:
        _plain[(l, hpc)] = _scan_lists(ctx, seqs, l, density, hpc)
    ctx.set_option("scan_guard_slack", slack)
    try:
        got = _scan_lists(ctx, seqs, l, density, hpc)
    finally:
        ctx.set_option("scan_guard_slack", 0)
    _assert_same(got, exp, (hpc, l, slack))
    _assert_same(got, _plain[(l, hpc)], (hpc, l, slack, "against slack 0"))
    _assert_same(_plain[(l, hpc)], exp, (hpc, l, "slack 0"))


@pytest.mark.parametrize("slack", [1 << 26, 1 << 31])
def test_slow_path_fastq_vs_oracle(ctx, orc, slack):
    """The QUAL variant (compressed, l = 15): the records of readSelection with every span walked exactly."""
    seqs = _border_reads(15, True)
    rng = np.random.default_rng(8200)
    quals = [bytes((rng.integers(2, 60, len(s)) + 33).astype(np.uint8)) for s in seqs]
    reads = ctx.reads_from_ascii(seqs, quals)
    plain = formats.build_read_data_init(ctx.scan(reads, K=15, density=0.02, hpc=True).to_host())
    ctx.set_option("scan_guard_slack", slack)
    try:
        got = formats.build_read_data_init(ctx.scan(reads, K=15, density=0.02, hpc=True).to_host())
    finally:
        ctx.set_option("scan_guard_slack", 0)
    reads.free()
    exp = b"".join(orc.read_selection(s, quals[i], K=15, density=0.02, hpc=True)["record"] for i, s in enumerate(seqs))
    assert got == exp
    assert got == plain


def test_both_slacks_together(ctx, orc):
    """The candidate test widened AND every span on the slow path: the slow path lists the same false candidates, the reads that
    have one are still re-run by the general kernel, and no record changes."""
    rng = np.random.default_rng(8300)
    seqs = [bytes(synth.CODE2ASCII[rng.integers(0, 4, int(n))]) for n in rng.integers(3000, 9000, 300)]
    reads = ctx.reads_from_ascii(seqs)
    plain = formats.build_read_data_init(ctx.scan(reads, K=15, density=0.005, hpc=True).to_host())
    ctx.set_option("scan_candidate_slack", 1 << 15)
    ctx.set_option("scan_guard_slack", 1 << 26)
    try:
        ctx.timing(True); ctx.timing_reset()
        both = formats.build_read_data_init(ctx.scan(reads, K=15, density=0.005, hpc=True).to_host())
        launches = ctx.timing_get("scan")[1]
    finally:
        ctx.set_option("scan_candidate_slack", 0)
        ctx.set_option("scan_guard_slack", 0)
        ctx.timing(False)
    reads.free()
    assert launches == 2                                    # the block kernel, then the general kernel over the reads it lost
    assert both == plain
    exp = b"".join(orc.read_selection(s, None, K=15, density=0.005, hpc=True)["record"] for s in seqs[:60])
    assert plain[:len(exp)] == exp
