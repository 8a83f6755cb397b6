"""formats.bgzf_compress / formats.bgzf_blocks: the Python statement of BGZF that the GPU tests build their inputs and block tables
with.  bgzf_blocks applies BgzfReader::index's acceptance rule (metamdbg_amd/host/hostfeed.hpp)."""
import gzip
import random
import zlib

import pytest

from metamdbg_amd import formats


def _text(n, seed=5):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT\n") for _ in range(n)).encode()


@pytest.mark.parametrize("block", [1, 2, 3000, 0xFF00, 65536])
@pytest.mark.parametrize("level,strategy", [(6, 0), (1, zlib.Z_FIXED), (0, 0), (9, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)])
def test_blocks_round_trip(block, level, strategy):
    data = _text(7 if block < 3 else 150000)
    if level == 0 and block == 65536:                          # stored, 65536 bytes and their framing do not fit a 64 KB member
        with pytest.raises(ValueError):
            formats.bgzf_compress(data, block=block, level=level, strategy=strategy)
        return
    raw = formats.bgzf_compress(data, block=block, level=level, strategy=strategy)
    assert gzip.decompress(raw) == data                        # any gzip reader takes it
    blocks = formats.bgzf_blocks(raw)
    assert blocks is not None and len(blocks) == (len(data) + block - 1) // block + 1
    at = 0
    for src, csize, isize, crc in blocks:
        piece = zlib.decompress(raw[src:src + csize], -15)
        assert piece == data[at:at + isize] and isize == len(piece) <= block
        assert crc == zlib.crc32(piece) & 0xFFFFFFFF
        at += isize
    assert at == len(data)
    assert blocks[-1][2] == 0                                  # the EOF marker
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def test_without_eof_marker_and_empty():
    data = _text(5000)
    raw = formats.bgzf_compress(data, eof_marker=False)
    blocks = formats.bgzf_blocks(raw)
    assert len(blocks) == 1 and blocks[0][2] == 5000
    assert len(formats.bgzf_blocks(formats.bgzf_compress(b""))) == 1
    assert formats.bgzf_blocks(formats.bgzf_compress(b"", eof_marker=False)) is None      # no member at all
    assert formats.bgzf_blocks(b"") is None


def test_what_is_not_pure_bgzf_is_refused():
    data = _text(100000)
    raw = formats.bgzf_compress(data, block=3000)
    assert formats.bgzf_blocks(raw) is not None
    assert formats.bgzf_blocks(gzip.compress(data)) is None                               # plain gzip
    assert formats.bgzf_blocks(raw + gzip.compress(b"tail")) is None                      # BGZF, then a gzip member
    assert formats.bgzf_blocks(raw + b"\0") is None
    last = formats.bgzf_blocks(raw)[-2]
    for cut in (1, 8, 9, 28 + 1, 28 + last[1] // 2):
        assert formats.bgzf_blocks(raw[:-cut]) is None, cut                                # a truncated last block
    bad = bytearray(raw)
    bad[3] |= 8                                                                           # FNAME: no BGZF writer sets it
    assert formats.bgzf_blocks(bytes(bad)) is None
    bad = bytearray(raw)
    bad[12] = ord("X")                                                                    # no 'BC' subfield
    assert formats.bgzf_blocks(bytes(bad)) is None


def test_a_member_that_cannot_hold_its_text_is_an_error():
    import os
    with pytest.raises(ValueError):
        formats.bgzf_compress(os.urandom(65536), block=65536)                             # stored: 65536 + 5 + 26 bytes
