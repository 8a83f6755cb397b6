"""mdbg_minimizers_to_record_bytes: a minimizer set serialised on the device (csrc/records_dev.hpp, records_write_kernel) into the exact
bytes of its record file -- `u32 n; u8 circular; u32 m[n]` (MDBG_RECORDS_PLAIN) and read_data_init.txt's records (MDBG_RECORDS_INIT) --
against formats.write_minimizer_reads / formats.build_read_data_init and the reference's own files under tests/golden.  Counts are
chosen so that every short count meets every alignment of a record's start, and the tests assert that they did.
Run on the GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import os

import numpy as np
import pytest

from metamdbg_amd import capi, formats, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

PLAIN, INIT = capi.RECORDS_PLAIN, capi.RECORDS_INIT


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def record_bytes(ctx, m, form) -> bytes:
    b = ctx.minimizers_to_record_bytes(m, form)
    raw = b.download(0, b.n)
    b.free()
    return raw


def random_reads(seed, lengths):
    rng = np.random.default_rng(seed)
    return [bytes(synth.CODE2ASCII[rng.integers(0, 4, int(n))]) for n in lengths]


def random_quals(seed, seqs):
    rng = np.random.default_rng(seed)
    return [bytes((rng.integers(2, 60, len(s)) + 33).astype(np.uint8)) for s in seqs]


def covered(offsets, per_read, per_min, counts) -> set:
    """(count, residue of the record's first byte mod 4) of every record with a count in `counts`."""
    offs = np.asarray(offsets, dtype=np.int64)
    cnt = np.diff(offs)
    start = per_read * np.arange(len(cnt), dtype=np.int64) + per_min * offs[:-1]
    return {(int(c), int(a)) for c, a in zip(cnt, start % 4) if int(c) in counts}


# ---- PLAIN ---------------------------------------------------------------------------------------------------------------------------
PLAIN_COUNTS = [c for c in range(41) for _ in range(5)] + [15, 16, 17, 31, 32, 33, 70001]


def test_plain_from_host_every_count_at_every_alignment(ctx):
    rng = np.random.default_rng(11)
    offs = np.concatenate([[0], np.cumsum(PLAIN_COUNTS)]).astype(np.uint64)
    mins = rng.integers(0, 1 << 32, int(offs[-1]), dtype=np.uint64).astype(np.uint32)
    mins[rng.integers(0, len(mins), 400)] = 0
    mins[rng.integers(0, len(mins), 400)] = 0xFFFFFFFF
    mins[:6] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    assert covered(offs, 5, 4, range(41)) == {(c, a) for c in range(41) for a in range(4)}
    m = ctx.minimizers_from_host(mins, offs)
    b = ctx.minimizers_to_record_bytes(m, PLAIN)
    assert b.n == 5 * len(PLAIN_COUNTS) + 4 * len(mins)
    raw = b.download(0, b.n)
    assert raw == formats.write_minimizer_reads(mins, offs)
    # ... and back through the gather, queued behind the serialisation on the same context
    back, circ = ctx.minimizers_from_record_bytes(b, offs, want_circular=True)
    h = back.to_host(full=False)
    assert np.array_equal(h["offsets"], offs) and np.array_equal(h["minimizers"], mins)
    assert not circ.any()
    for x in (back, b, m):
        x.free()


@pytest.fixture(scope="module")
def hifi_scan(ctx):
    spec = synth.hifi_spec(256, seed=3, read_len=6000, coverage=30.0)
    reads = ctx.reads_synthetic(spec)
    mins = ctx.scan(reads, K=15, density=0.005, hpc=True)
    reads.free()
    yield mins
    mins.free()


def test_plain_from_a_purge_output_and_a_slice(ctx, hifi_scan):
    pur = ctx.purge_palindromes(hifi_scan, 4, 100)
    h = pur.to_host(full=False)
    assert len(h["minimizers"]) > 256
    assert record_bytes(ctx, pur, PLAIN) == formats.write_minimizer_reads(h["minimizers"], h["offsets"])
    for first, n in ((0, 256), (7, 50), (255, 1), (100, 0)):
        sl = ctx.minimizers_slice(pur, first, n)
        a, b = int(h["offsets"][first]), int(h["offsets"][first + n])
        assert record_bytes(ctx, sl, PLAIN) == formats.write_minimizer_reads(h["minimizers"][a:b], h["offsets"][first:first + n + 1] - h["offsets"][first])
        sl.free()
    # a scan output in PLAIN form: its values alone
    hs = hifi_scan.to_host(full=False)
    assert record_bytes(ctx, hifi_scan, PLAIN) == formats.write_minimizer_reads(hs["minimizers"], hs["offsets"])
    pur.free()


# ---- INIT ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_qual", [True, False])
@pytest.mark.parametrize("hpc", [True, False])
def test_init_short_reads_fresh_and_canonical(ctx, hpc, with_qual):
    """1200 reads of 1 .. 59 bases at l = 15, density 0.3: records of 0 .. a dozen minimizers, where nothing has an interior word and every
    field straddles.  The scan output is serialised as it comes (scattered), then again after to_host has brought it into read order."""
    rng = np.random.default_rng(77)
    seqs = random_reads(77, rng.integers(1, 60, 1200))
    quals = random_quals(78, seqs) if with_qual else None
    reads = ctx.reads_from_ascii(seqs, quals)
    m = ctx.scan(reads, K=15, density=0.3, hpc=hpc)
    fresh = record_bytes(ctx, m, INIT)
    h = m.to_host()
    want = formats.build_read_data_init(h)
    assert fresh == want
    assert record_bytes(ctx, m, INIT) == want
    assert len(want) == 13 * 1200 + 10 * len(h["minimizers"])
    # the point of these reads: every count 0 .. 9 at every residue of the record's start
    assert covered(h["offsets"], 13, 10, range(10)) == {(c, a) for c in range(10) for a in range(4)}
    if with_qual:
        assert np.isfinite(h["mean_quality"]).all() and len(set(h["mean_quality"].tolist())) > 100
    else:
        assert np.isnan(h["mean_quality"]).all()                  # the NaN the reference writes, bit for bit (checked by the equality above)
    m.free()
    reads.free()


def test_init_one_long_read_at_high_density(ctx):
    seqs = random_reads(5, [3000])
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=15, density=0.9, hpc=False)
    raw = record_bytes(ctx, m, INIT)
    h = m.to_host()
    assert len(h["minimizers"]) > 2000
    assert raw == formats.build_read_data_init(h)
    m.free()
    reads.free()


def test_init_from_concat_and_density_threshold(ctx):
    parts, quals_on = [], [True, False, True]
    for i, q in enumerate(quals_on):
        seqs = random_reads(300 + i, np.random.default_rng(300 + i).integers(1, 400, 150))
        reads = ctx.reads_from_ascii(seqs, random_quals(400 + i, seqs) if q else None)
        parts.append(ctx.scan(reads, K=15, density=0.05, hpc=True))
        reads.free()
    cat = ctx.minimizers_concat(parts)
    h = cat.to_host()
    assert len(h["offsets"]) == 451 and np.isnan(h["mean_quality"][150:300]).all() and np.isfinite(h["mean_quality"][:150]).all()
    assert record_bytes(ctx, cat, INIT) == formats.build_read_data_init(h)
    thin = ctx.apply_density_threshold(cat, 0.01)
    ht = thin.to_host()
    assert 0 < len(ht["minimizers"]) < len(h["minimizers"])
    assert record_bytes(ctx, thin, INIT) == formats.build_read_data_init(ht)
    for x in parts + [cat, thin]:
        x.free()


def test_init_read_emptied_by_the_complexity_filter(ctx):
    seqs = random_reads(9, [500, 700]) + [b"AC" * 1500] + random_reads(10, [300])
    quals = random_quals(12, seqs)
    reads = ctx.reads_from_ascii(seqs, quals)
    m = ctx.scan(reads, K=15, density=0.3, hpc=False)
    raw = record_bytes(ctx, m, INIT)
    h = m.to_host()
    cnt = np.diff(h["offsets"].astype(np.int64))
    assert h["flags"][2] & capi.MDBG_READ_LOW_COMPLEXITY and cnt[2] == 0 and cnt[1] > 0 and cnt[3] > 0
    assert h["read_length"][2] == 3000 and np.isfinite(h["mean_quality"][2]) and h["mean_quality"][2] > 0
    assert raw == formats.build_read_data_init(h)
    rec = formats.parse_read_data_init(raw)
    assert len(rec) == 4
    m.free()
    reads.free()


# ---- the reference's own files ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,K,dens,hpc", [("hpc_k15", 15, 0.005, True), ("nohpc_k15", 15, 0.005, False),
                                            ("hpc_k16", 16, 0.005, True), ("nohpc_k13", 13, 0.02, False)])
def test_edge_reads_golden(ctx, tag, K, dens, hpc):
    seqs = [s.upper() for s in H.read_fasta(os.path.join(H.GOLDEN, "edge", "edge.fasta"))]
    rep = np.frombuffer(H.golden_bytes("edge", f"repetitiveMinimizers.{tag}.bin"), "<u4")
    reads = ctx.reads_from_ascii(seqs)
    m = ctx.scan(reads, K=K, density=dens, hpc=hpc, repetitive=rep)
    assert record_bytes(ctx, m, INIT) == H.golden_bytes("edge", f"read_data_init.{tag}.txt")
    m.free()
    reads.free()


def test_hifi_200_golden(ctx):
    from oracle import pyoracle as orc
    man = H.load_manifest("hifi_200")
    reads = ctx.reads_synthetic(H.spec_from_manifest(man))
    mins = ctx.scan(reads, K=man["K"], density=man["density"], hpc=man["hpc"])
    assert record_bytes(ctx, mins, INIT) == H.golden_bytes("hifi_200", "read_data_init.txt")
    st = formats.parse_read_stats(H.golden_bytes("hifi_200", "read_stats.txt"))
    corr = ctx.purge_palindromes(mins, 4, orc.lib().orc_compute_last_k(man["density"], st["n50"], 4, 0))
    got = formats.parse_minimizer_reads(record_bytes(ctx, corr, PLAIN))
    exp = formats.parse_minimizer_reads(H.golden_bytes("hifi_200", "read_data_corrected.txt"))
    assert len(exp[1]) == 201 and formats.minimizer_reads_equal_as_multisets(got[0], got[1], exp[0], exp[1])
    for x in (corr, mins, reads):
        x.free()


# ---- errors and the empty set ----------------------------------------------------------------------------------------------------------
def test_errors_and_zero_reads(ctx):
    import ctypes as C
    offs = np.array([0, 3, 3, 5], dtype=np.uint64)
    m = ctx.minimizers_from_host(np.arange(5, dtype=np.uint32), offs)
    with pytest.raises(capi.MdbgError) as ei:
        ctx.minimizers_to_record_bytes(m, INIT)
    assert ei.value.code == -1 and "mdbg_scan output" in str(ei.value)
    with pytest.raises(capi.MdbgError) as ei:
        ctx.minimizers_to_record_bytes(m, 7)
    assert ei.value.code == -1 and "form 7" in str(ei.value)
    rc = capi.lib().mdbg_minimizers_to_record_bytes(ctx.h, m.h, PLAIN, None, None)
    assert rc == -1 and b"null argument" in capi.lib().mdbg_last_error(ctx.h)
    h = C.c_void_p()
    assert capi.lib().mdbg_minimizers_to_record_bytes(ctx.h, None, PLAIN, C.byref(h), None) == -1 and not h.value
    # n_bytes is optional
    assert capi.lib().mdbg_minimizers_to_record_bytes(ctx.h, m.h, PLAIN, C.byref(h), None) == 0
    b = capi.DeviceBytes(ctx, h, 5 * 3 + 4 * 5)
    assert b.download(0, b.n) == formats.write_minimizer_reads(np.arange(5, dtype=np.uint32), offs)
    b.free()
    m.free()
    empty = ctx.minimizers_from_host(np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    b = ctx.minimizers_to_record_bytes(empty, PLAIN)
    assert b.n == 0 and b.download(0, 0) == b""
    b.free()
    empty.free()
    reads = ctx.reads_from_ascii([])
    none = ctx.scan(reads, K=15, density=0.005, hpc=True)
    b = ctx.minimizers_to_record_bytes(none, INIT)
    assert b.n == 0
    for x in (b, none, reads):
        x.free()


def test_the_timer_counts_the_launch(ctx, hifi_scan):
    ctx.timing(True); ctx.timing_reset()
    try:
        record_bytes(ctx, hifi_scan, INIT)
        ms, launches = ctx.timing_get("records_write")
        assert launches == 1 and ms > 0
    finally:
        ctx.timing(False)
