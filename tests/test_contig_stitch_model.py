"""tests/stitch_model.py -- the numpy restatement tests/test_gpu_contig_stitch.py compares the device with -- against the text the
REFERENCE wrote for the fixture under tests/golden/contig_stitch (ToBasespaceGfa::CreateBaseContigsFunctor over DnaBitset2 pieces, through
gzwrite; the generator committed there), byte for byte; the conditions the generator asserted on its selection, asserted again on the
committed data; the Python helper that builds pieces by the reference's rule; and that the library exports the entry points."""
from __future__ import annotations

import importlib.util
import json
import os

import numpy as np
import pytest

from tests import extract_model as EM
from tests import helpers as H
from tests import stitch_model as SM

FIX, SEQUENCES, MANIFEST, load = SM.FIX, SM.SEQUENCES, SM.MANIFEST, SM.load
SPANS = os.path.join(H.GOLDEN, "kminmer_spans")


@pytest.mark.parametrize("cfg", MANIFEST["configs"], ids=[c["name"] for c in MANIFEST["configs"]])
def test_model_writes_the_references_text(cfg):
    reads, spans, contigs, want = load(cfg)
    assert len(contigs) == cfg["n_contigs"] and sum(map(len, contigs)) == cfg["n_positions"]
    pieces, offsets = SM.pieces_by_the_rule(contigs, spans["window_offsets"])
    strings = SM.contig_strings(reads, spans, pieces, offsets, EM.BITSET)
    text = SM.fasta_text(strings, want["names"], want["flags"])
    assert len(text) == cfg["n_text_bytes"]
    assert text == want["text"].tobytes()
    # the layout of the two forms: offsets at multiples of 8, lengths = the contig's bases, the characters differ only where the bitset has no N
    for form in (EM.BITSET, EM.ASCII):
        lay = SM.layout(SM.contig_strings(reads, spans, pieces, offsets, form), form)
        assert np.array_equal(lay["lengths"], [len(s) for s in strings]) and not (lay["byte_offsets"] % 8).any()
        EM.unpadded(lay, form)
    ascii_strings = SM.contig_strings(reads, spans, pieces, offsets, EM.ASCII)
    assert any(b"N" in s for s in ascii_strings) and not any(b"N" in s for s in strings)
    for a, b in zip(ascii_strings, strings):
        assert len(a) == len(b) and all(x == y or (x == ord("N") and y in b"AT") for x, y in zip(a, b))


@pytest.mark.parametrize("cfg", MANIFEST["configs"], ids=[c["name"] for c in MANIFEST["configs"]])
def test_conditions_on_the_selection(cfg):
    """Each of the eight (position 0 / later) x (read window reversed) x (contig window reversed) at least 50 times, pieces beginning at
    every base offset mod 32, a flipped and an unflipped piece over a bit-3 character, a contig whose window 0 is missing, one with every
    window missing, one without windows, all three flags, names of 1, 2 and 10 digits with 0 and 4294967295 -- by the generator's own
    function, on the committed data."""
    spec = importlib.util.spec_from_file_location("contig_stitch_make_fixture", os.path.join(FIX, "make_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    reads, spans, contigs, want = load(cfg)
    found = gen.conditions(reads, spans, contigs, want["names"], want["flags"])
    assert found == {f: cfg[f] for f in found}
    # nothing but the reads tests/golden/kminmer_sequences leaves out is left out, and the count is recorded
    with open(os.path.join(SEQUENCES, "manifest.json")) as f:
        theirs = {c["name"]: c for c in json.load(f)["configs"]}[cfg["name"]]
    assert cfg["reads"] == theirs["reads"] and cfg["left_out"] == theirs["left_out"]
    # no committed file larger than the largest under tests/golden/kminmer_spans
    limit = max(os.path.getsize(os.path.join(SPANS, f)) for f in os.listdir(SPANS))
    assert all(os.path.getsize(os.path.join(FIX, f)) <= limit for f in os.listdir(FIX))


def test_the_invalid_rule_on_a_hand_made_piece():
    """GNT forward, kept as DnaBitset2: GAT; behind the flip ATC -- the invalid base is T, whatever the read window's orientation."""
    reads = [b"CCGNTCC"]
    spans = dict(window_offsets=np.array([0, 1], np.uint64), reversed=np.array([0], np.uint8), pos_start=np.array([2], np.uint32), pos_end=np.array([5], np.uint32),
                 seq_length_start=np.array([1], np.uint32), seq_length_end=np.array([2], np.uint32))
    piece = lambda part, flip: np.array([(0, part, flip)], SM.PIECE)[0]
    assert SM.piece_string(reads, spans, piece(EM.ENTIRE, 0), EM.BITSET) == b"GAT" and SM.piece_string(reads, spans, piece(EM.ENTIRE, 1), EM.BITSET) == b"ATC"
    assert SM.piece_string(reads, spans, piece(EM.ENTIRE, 0), EM.ASCII) == b"GNT" and SM.piece_string(reads, spans, piece(EM.ENTIRE, 1), EM.ASCII) == b"ANC"
    assert SM.piece_string(reads, spans, piece(EM.RIGHT, 0), EM.BITSET) == b"AT" and SM.piece_string(reads, spans, piece(EM.LEFT, 1), EM.BITSET) == b"C"
    spans["reversed"][0] = 1                      # the read's window reversed: stored ANC -> AAC; flipped GTT
    assert SM.piece_string(reads, spans, piece(EM.ENTIRE, 0), EM.BITSET) == b"AAC" and SM.piece_string(reads, spans, piece(EM.ENTIRE, 1), EM.BITSET) == b"GTT"
    assert SM.fasta_text([b"GAT", b"", b"ATC"], [7, 4294967295, 10], [1, 2, 2]) == b">ctg7c\nGAT\n>ctg4294967295l\nA\n>ctg10c\nATC\n"


def test_python_helper_builds_pieces_by_the_rule():
    from metamdbg_amd import capi
    assert capi.STITCH_PIECE == SM.PIECE and capi.STITCH_NONE == SM.NONE
    contigs = [[(0, 1, 0, 1), (1, 0, 1, 1), (1, 2, 0, 0), (0, 0, 0, 1)], [], [(1, 1, 1, 1)]]
    woff = np.array([0, 3, 6], np.uint64)
    want, want_off = SM.pieces_by_the_rule(contigs, woff)
    got, got_off = capi.stitch_pieces([[((r, w) if p else None, v) for r, w, v, p in c] for c in contigs], woff)
    assert np.array_equal(got, want) and np.array_equal(got_off, want_off) and list(got_off) == [0, 4, 4, 5]
    assert got.tolist() == [(1, 0, 0), (3, 1, 1), (SM.NONE, 0, 0), (0, 2, 0), (4, 0, 1)]
    flat, _ = capi.stitch_pieces([[(1, 0), (3, 1), (None, 0), (0, 0)], [], [(4, 1)]])
    assert np.array_equal(flat, want)


def test_library_exports_the_entry_points():
    import subprocess
    from metamdbg_amd import build, capi
    build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mdbg_spans_stitch", "mdbg_reads_stitch_ranges", "mdbg_sequences_to_fasta_bytes"):
        assert f" T {name}\n" in out and name in capi.SIGNATURES
