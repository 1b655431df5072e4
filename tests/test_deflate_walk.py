"""tests/deflate_walk.py against zlib (CPU only): the walker is what test_png_encode_edges.py trusts to say which matches and which
block types a device stream holds, so here it reads zlib's own output at levels 0, 1, 6 and 9 over the filtered streams of four small
pictures and one of more than 32 KB.  Replaying its symbols must give the input back, and every block it reports must be a block to zlib's inflate as well:
cut out of the stream at the walker's bit positions, marked final and inflated alone with the bytes before it as the dictionary,
it ends zlib's stream exactly at its last bit and yields exactly the bytes the walker's symbols stand for."""
import zlib

import numpy as np
import pytest

import deflate_walk as dw
import synth
from png_enc_model import filter_rows

LEVELS = (0, 1, 6, 9)


def _pictures():
    rng = np.random.default_rng(11)
    ramp = (np.arange(3 * 2, dtype=np.uint8) * 7).reshape(2, 3, 1)
    return {"photo": synth.photo(40, 56, 3, index=41), "flat": np.full((30, 30, 4), 77, np.uint8),
            "noise": rng.integers(0, 256, (24, 24, 1), dtype=np.uint8), "ramp": ramp,
            "sparse": (rng.integers(0, 50, (300, 120, 1)) == 0).astype(np.uint8) * 200}   # > 32 KB: zlib's window wraps


@pytest.fixture(scope="module")
def streams():
    return {name: filter_rows(px)[1] for name, px in _pictures().items()}


def _cut(data, a, b, final):
    """Bits [a, b) of data as a byte string of their own, bit a becoming bit 0 and BFINAL forced to `final`."""
    v = (int.from_bytes(data, "little") >> a) & ((1 << (b - a)) - 1)
    v = (v & ~1) | int(final)
    return v.to_bytes((b - a + 7) // 8, "little")


def _raw(stream, level):
    z = zlib.compress(stream, level)
    assert zlib.decompress(z) == stream
    return z[2:-4]


@pytest.mark.parametrize("level", LEVELS)
def test_replaying_the_symbols_gives_the_input_back(streams, level):
    for name, stream in streams.items():
        raw = _raw(stream, level)
        blocks, end = dw.walk(raw)
        assert dw.replay(blocks) == stream, name
        assert (end + 7) // 8 == len(raw), name           # nothing after the final block but the padding of its byte
        assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True], name
        assert blocks[0].start_bit == 0 and all(a.end_bit == b.start_bit for a, b in zip(blocks, blocks[1:]))
        for b in blocks:
            for length, dist in b.matches():
                assert 3 <= length <= 258 and 1 <= dist <= 32768 - 262, (name, length, dist)   # zlib's own limits
            if b.type == dw.DYNAMIC:
                assert len(b.cl_lens) == 19 and 257 <= len(b.lit_lens) <= 286 and 1 <= len(b.dist_lens) <= 30
                assert max(b.cl_lens) <= 7 and max(b.lit_lens) <= 15 and max(b.dist_lens) <= 15 and b.lit_lens[256] > 0
            else:
                assert b.cl_lens is None and b.lit_lens is None and b.dist_lens is None


def test_blocks_and_their_types_are_what_zlib_inflates(streams):
    seen = set()
    for level in LEVELS:
        for name, stream in streams.items():
            raw = _raw(stream, level)
            blocks, _ = dw.walk(raw)
            done = b""
            for k, b in enumerate(blocks):
                alone = _cut(raw, b.start_bit, b.end_bit, True)
                assert (alone[0] >> 1) & 3 == b.type
                d = zlib.decompressobj(-15, zdict=done[-32768:]) if done else zlib.decompressobj(-15)
                got = d.decompress(alone)
                assert d.eof and d.unused_data == b"", (name, level, k)    # one whole block, and no second one behind it
                assert got == dw.replay([b], history=done), (name, level, k)
                # one bit less is no block to zlib (a stored block of 0 bytes aside: its last bits are the NLEN field's)
                if b.end_bit - b.start_bit > 8:
                    short = zlib.decompressobj(-15, zdict=done[-32768:]) if done else zlib.decompressobj(-15)
                    short.decompress(alone[:-1])
                    assert not short.eof, (name, level, k)
                done += got
                seen.add(b.type)
            assert done == stream
            if level == 0:
                assert all(b.type == dw.STORED for b in blocks), name
                assert sum(len(b.symbols) for b in blocks) == len(stream)
            else:
                assert all(b.type != dw.STORED for b in blocks) or name == "noise", (name, level)
    assert seen == {dw.STORED, dw.FIXED, dw.DYNAMIC}


def test_damaged_streams_are_refused():
    stream = bytes(range(256)) * 4
    raw = _raw(stream, 6)
    with pytest.raises(dw.DeflateError):
        dw.walk(raw[:len(raw) // 2])
    with pytest.raises(dw.DeflateError):
        dw.walk(b"\x07")                                  # block type 3
    with pytest.raises(dw.DeflateError):
        dw.walk(b"\x00\x05\x00\x00\x00hello")             # LEN / NLEN
    far = dw.Block(dw.FIXED, True, 0)
    far.symbols = [65, (3, 2)]
    with pytest.raises(dw.DeflateError):
        dw.replay([far])                                  # a distance that reaches before the first byte
    assert dw.replay([far], history=b"x") == b"AxAx"


# ------------------------------------------------------------------- the segment-layout checker on files made with zlib --

def _segmented_png(px, level=6, break_it=None):
    """A PNG in the device encoder's layout, written with zlib: one IDAT per 32 KB of the filtered stream, each ended by a sync
    flush (the empty stored block), the Adler-32 in an IDAT of its own."""
    import struct
    from png_enc_model import SEG
    h, w, c = px.shape
    raw = filter_rows(px)[1]
    co = zlib.compressobj(level, zlib.DEFLATED, 15)
    parts = []
    for s in range(0, len(raw), SEG):
        last = s + SEG >= len(raw)
        parts.append(co.compress(raw[s:s + SEG]) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH))
    parts[-1], adler = parts[-1][:-4], parts[-1][-4:]
    if break_it == "merged_adler":
        parts[-1] += adler
    elif break_it == "no_flush":
        parts[0], parts[1] = parts[0][:-4], parts[0][-4:] + parts[1]
    parts.append(adler if break_it != "wrong_adler" else bytes([adler[0] ^ 1]) + adler[1:])
    if break_it == "merged_adler":
        parts.pop()

    def chunk(t, b):
        return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""), raw


def test_segment_chunks_accepts_the_layout_and_refuses_what_breaks_it():
    from png_enc_model import check_stream, segment_chunks
    px = _pictures()["sparse"]                       # 36,300 filtered bytes: two segments
    data, raw = _segmented_png(px)
    check_stream(data, px, 75)
    got, bodies = segment_chunks(data)
    assert got == raw and len(bodies) == 2
    blocks = [dw.walk(b)[0] for b in bodies]
    assert [b.type for b in blocks[0]][-1] == dw.STORED and blocks[0][-1].symbols == [] and blocks[1][-1].final
    assert dw.replay(blocks[1], history=raw[:32768]) == raw[32768:]
    for how in ("merged_adler", "no_flush", "wrong_adler"):
        with pytest.raises(AssertionError):
            segment_chunks(_segmented_png(px, break_it=how)[0])
