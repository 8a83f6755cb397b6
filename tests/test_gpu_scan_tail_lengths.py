"""The tail of a read in the block kernel (scan.hip, scan_fast_kernel): the up to 2048 positions the full blocks leave go to the
lanes in spans of P = ceil(npos / 64) positions, each walked as two half spans of Ph = ceil(P / 2) side by side.  It can go wrong at
span and chain borders only -- P = 1, odd and even P, P = 32 with Ph = 16, a last lane partly filled, one live lane, the order of the
two chains' verdict bits, the padding bit of an odd P -- so the reads are short and every border length is there.  Values, positions,
directions and counts per read against the oracle.  Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

from metamdbg_amd import formats, synth

pytestmark = pytest.mark.gpu

# positions left to the tail; lengths 2048 m + npos + K + 1 (+ K without the end trim) and, one base shorter, the lengths at which
# the kernel's own count of tail positions is npos itself
NPOS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1341, 1984, 1985, 2046, 2047]
BLOCKS = [0, 1, 3]


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


def _random_read(rng, n):
    return bytes(synth.CODE2ASCII[rng.integers(0, 4, int(n))])


_exact = {}


def _exact_length_reads(K, trim):
    """Without homopolymer compression the compressed length is the length: every (m, npos) of the issue, and one base less."""
    if (K, trim) not in _exact:
        rng = np.random.default_rng(1000 + 2 * K + int(trim))
        _exact[(K, trim)] = [_random_read(rng, 2048 * m + npos + K + (1 if trim else 0) - d)
                             for m in BLOCKS for npos in NPOS for d in (0, 1)]
    return _exact[(K, trim)]


_hpc_reads = None


def _compressed_reads():
    """Random reads of 50 - 6200 bases, runs stretched as a sequencer's would be: their compressed lengths sweep the same borders."""
    global _hpc_reads
    if _hpc_reads is None:
        rng = np.random.default_rng(4242)
        out = []
        for n in rng.integers(50, 6201, 320):
            c = rng.integers(0, 4, int(n))
            if len(out) % 2:                      # every other read with longer runs (the compressed length falls well below n)
                c = np.repeat(c, rng.choice([1, 1, 2, 3], len(c)))[:int(n)]
            out.append(bytes(synth.CODE2ASCII[c]))
        _hpc_reads = out
    return _hpc_reads


def _compare_with_parse(ctx, orc, seqs, K, density, hpc, trim):
    reads = ctx.reads_from_ascii(seqs)
    h = ctx.scan(reads, K=K, density=density, hpc=hpc, apply_read_filters=False, no_end_trim=not trim).to_host()
    assert len(h["offsets"]) == len(seqs) + 1
    n_total = 0
    for i, s in enumerate(seqs):
        e = orc.minimizer_parse(s, K, density, hpc, trim=1 if trim else 0)
        a, b = int(h["offsets"][i]), int(h["offsets"][i + 1])
        assert b - a == len(e[0]), (K, density, hpc, trim, i, len(s))
        assert (h["minimizers"][a:b].tolist(), h["pos"][a:b].tolist(), h["dir"][a:b].tolist()) == \
            (list(e[0]), list(e[1]), list(e[2])), (K, density, hpc, trim, i, len(s))
        n_total += b - a
    reads.free()
    return n_total


# 0.005: the headline's density, a tail lists 0 - 10 positions.  0.15: every span has bits set in both chains, and a read of up to
# 2047 positions still fits the stage (384 rows), so the order of the chains' bits is what places every one of them.  1.0f: the full
# verdict (the candidate limit would saturate), EVERY tail position selected -- the padding bit of an odd P would show as one
# minimizer too many, a dropped or swapped bit as a wrong position.  0.99999994f: the same through the candidate test.
@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("K,density", [(15, 0.005), (15, 0.15), (15, 1.0), (15, 0.99999994), (16, 0.02), (16, 1.0), (13, 0.15)])
def test_tail_exact_lengths_vs_oracle(ctx, orc, K, density, trim):
    seqs = _exact_length_reads(K, trim)
    n = _compare_with_parse(ctx, orc, seqs, K, density, False, trim)
    if density == 1.0:       # every position but the trimmed first (and, trimmed, the last l-mer) is a minimizer
        assert n == sum(len(s) - K + 1 - (2 if trim else 0) for s in seqs)


@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("K,density", [(15, 0.005), (15, 0.15), (13, 0.02), (16, 1.0)])
def test_tail_compressed_reads_vs_oracle(ctx, orc, K, density, trim):
    seqs = _compressed_reads()
    # the compressed lengths really sweep the spans: every P from 1 up to 32 with one exception at most, odd and even
    spans = {(max(orc.read_selection(s, None, K=K, density=density, hpc=True)["hpc_length"] - K, 1) % 2048 + 63) // 64 for s in seqs}
    assert len(spans & set(range(1, 33))) >= 31, sorted(spans)
    _compare_with_parse(ctx, orc, seqs, K, density, True, trim)


@pytest.mark.parametrize("hpc", [False, True])
def test_tail_with_widened_candidate_test(ctx, orc, hpc):
    """scan_candidate_slack widens the candidate test: the tails list false candidates at both chains' edges, the reads that have one
    are re-run by the general kernel, and no record changes (as test_scan_false_candidates_are_rerun does for whole reads)."""
    seqs = _compressed_reads() if hpc else _exact_length_reads(15, True)
    ctx.set_option("scan_candidate_slack", 1 << 24)
    try:
        _compare_with_parse(ctx, orc, seqs, 15, 0.005, hpc, True)
    finally:
        ctx.set_option("scan_candidate_slack", 0)


@pytest.mark.parametrize("hpc", [False, True])
def test_tail_fastq_min_quality_vs_oracle(ctx, orc, hpc):
    """The QUAL variants: the minimum quality of a minimizer the tail selected, with and without compression (records of readSelection)."""
    rng = np.random.default_rng(99 + int(hpc))
    seqs = (_compressed_reads()[:160] if hpc else _exact_length_reads(15, True))
    quals = [bytes((rng.integers(2, 60, len(s)) + 33).astype(np.uint8)) for s in seqs]
    reads = ctx.reads_from_ascii(seqs, quals)
    got = formats.build_read_data_init(ctx.scan(reads, K=15, density=0.02, hpc=hpc).to_host())
    exp = b"".join(orc.read_selection(s, quals[i], K=15, density=0.02, hpc=hpc)["record"] for i, s in enumerate(seqs))
    assert got == exp
    reads.free()
