"""tests/extract_model.py -- the numpy restatement of mdbg_spans_extract that the GPU tests use on seeded inputs -- against the REFERENCE's
answers under tests/golden/kminmer_sequences (ToBasespaceGfa::extractKminmerSequence + DnaBitset2 over the windows of MDBG::getKminmers,
written by the generator committed there): the three-part rule with its exchange for reversed windows, the reverse complement, N and the
other characters with bit 3 as code 0, DnaBitset2's layout, and the layout of the output buffer.  Needs no GPU."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests import extract_model as EM
from tests import helpers as H

FIX = os.path.join(H.GOLDEN, "kminmer_sequences")
with open(os.path.join(FIX, "manifest.json")) as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def fixture_reads():
    with open(os.path.join(FIX, MANIFEST["reads"]), "rb") as f:
        reads = f.read().split(b"\n")[:-1]
    assert len(reads) == MANIFEST["n_reads"]
    return reads


def test_the_fixture_leaves_out_only_soft_and_iupac_reads(fixture_reads):
    with open(os.path.join(H.GOLDEN, "kminmer_spans", "manifest.json")) as f:
        spans = {c["name"]: c for c in json.load(f)["configs"]}
    assert [c["name"] for c in MANIFEST["configs"]] == list(spans)
    for cfg in MANIFEST["configs"]:
        theirs = spans[cfg["name"]]
        assert all(cfg[f] == theirs[f] for f in ("l", "density", "hpc", "trim", "k"))
        dropped = [i for i in theirs["reads"] if i not in cfg["reads"]]
        assert len(dropped) == cfg["left_out"] <= MANIFEST["soft_or_iupac_reads"]
        for i in dropped:                       # a lower-case letter, or an IUPAC letter without bit 3
            assert any(c not in b"ACGT" and not c & 8 for c in fixture_reads[i]), i
        for i in cfg["reads"]:
            assert all(c in b"ACGT" or c & 8 for c in fixture_reads[i]), i


@pytest.mark.parametrize("cfg", MANIFEST["configs"], ids=[c["name"] for c in MANIFEST["configs"]])
def test_model_against_the_reference(fixture_reads, cfg):
    want = np.load(os.path.join(FIX, cfg["name"] + ".npz"))
    seqs = [fixture_reads[i] for i in cfg["reads"]]
    spans = {f: want[f] for f in ("window_offsets", "reversed", "pos_start", "pos_end", "seq_length_start", "seq_length_end")}
    windows, parts = want["req_window"], want["req_part"]
    assert len(windows) == cfg["n_requests"] and int(spans["window_offsets"][-1]) == cfg["n_windows"]
    rev = spans["reversed"][windows.astype(np.int64)]
    for p in (EM.ENTIRE, EM.LEFT, EM.RIGHT):
        assert ((parts == p) & (rev == 0)).sum() >= 100 and ((parts == p) & (rev == 1)).sum() >= 100
    got = EM.expected_requests(seqs, spans, windows, parts, EM.BITSET)
    assert np.array_equal(got["lengths"], want["lengths"])
    assert np.array_equal(EM.unpadded(got, EM.BITSET), want["bitset"])
    # the characters: the same strings packed by DnaBitset2's rule give the reference's bytes, and N sits where the read has bit 3
    text = EM.expected_requests(seqs, spans, windows, parts, EM.ASCII)
    chars = EM.unpadded(text, EM.ASCII)
    assert set(np.unique(chars)) <= set(b"ACGTN") and int(text["lengths"].sum()) == len(chars) == cfg["n_bases"]
    at = np.concatenate([[0], np.cumsum(text["lengths"].astype(np.int64))])
    first = np.concatenate([[0], np.cumsum((want["lengths"].astype(np.int64) + 3) // 4)])
    for i in np.linspace(0, len(windows) - 1, 200).astype(np.int64):
        lo = int(first[i])
        s = bytes(chars[at[i]:at[i + 1]])
        assert np.array_equal(EM.bitset(s), want["bitset"][lo:lo + (len(s) + 3) // 4]), i
    if cfg["n_cover_bit3"]:
        assert (chars == ord("N")).any()


def test_the_example_of_the_header():
    """The read ACGTTNGCAaCGGTAC, a reversed window [2, 14) with seq_length_start 3 and seq_length_end 5: the reference returns
    ACCGtTGCNAAC / ACC / CNAAC (the packed read keeps no case: T for t)."""
    read = b"ACGTTNGCAaCGGTAC"
    want = [b"ACCGTTGCNAAC", b"ACC", b"CNAAC"]
    for part, w in zip((EM.ENTIRE, EM.LEFT, EM.RIGHT), want):
        start, length = EM.part_range([2], [14], [3], [5], [1], [part])
        assert EM.oriented(read, int(start[0]), int(length[0]), True) == w
    assert bytes(EM.bitset(b"ACCGTTGCNAAC")) == bytes([0b00010110, 0b11111001, 0b00000001])
