"""The checker tests/png_encode_ref.py itself: check_file accepts build_file's files (golden pages, gray, noise, tiny pages) and
rejects a flipped CRC, a flipped Adler-32, a Paeth row, an ancillary chunk and a plain Pillow file whose IDATs are not
independent: so a pass on the device encoder's files means something."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_page(name, gray=False):
    im = Image.open(os.path.join(GOLDEN, name))
    if gray:
        return np.ascontiguousarray(np.asarray(im.convert("L")))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


@pytest.fixture(scope="module")
def pages():
    rng = np.random.RandomState(0)
    return {"map": golden_page("sample_0717_023.jpg")[:500], "page": golden_page("sample_0717_023_orig.jpg")[300:800],
            "gray": golden_page("sample_0717_023_orig.jpg", gray=True)[:700],
            "noise": rng.randint(0, 256, (300, 400, 3)).astype(np.uint8), "one": np.array([[7]], np.uint8),
            "row": rng.randint(0, 256, (1, 50, 3)).astype(np.uint8), "col": rng.randint(0, 256, (50, 1)).astype(np.uint8)}


@pytest.mark.parametrize("policy", ["minsum", "changes", "up", "sub", "none"])
def test_accepts_built_files(pages, policy):
    for name, p in pages.items():
        f = R.build_file(p, policy)
        n = R.check_file(f, p)
        assert n == (p.shape[0] * (1 + p[0].size) + R.CHUNK - 1) // R.CHUNK, name
        assert len(f) <= R.encode_bound(p.shape[1], p.shape[0], 1 if p.ndim == 2 else 3), name


def test_accepts_stored_files_and_they_hit_the_bound(pages):
    for name, p in pages.items():
        f = R.build_file(p, "up", stored=True)
        R.check_file(f, p)
        assert len(f) == R.encode_bound(p.shape[1], p.shape[0], 1 if p.ndim == 2 else 3), name


def rechunk(chunks):
    return R.SIGNATURE + b"".join(R._chunk(k, b) for k, b in chunks)


def test_rejects_a_flipped_crc(pages):
    p = pages["page"]
    f = bytearray(R.build_file(p))
    f[8 + 25 + 8 + 100] ^= 1                                        # a byte inside IDAT 0: its CRC no longer matches
    with pytest.raises(AssertionError, match="CRC"):
        R.check_file(bytes(f), p)
    f = bytearray(R.build_file(p))
    f[-13] ^= 1                                                      # the last IDAT's stored CRC
    with pytest.raises(AssertionError, match="CRC"):
        R.check_file(bytes(f), p)


def test_rejects_a_flipped_adler(pages):
    p = pages["page"]
    chunks = R.parse_chunks(R.build_file(p))
    kind, body = chunks[-2]
    chunks[-2] = (kind, body[:-1] + bytes([body[-1] ^ 1]))
    with pytest.raises(AssertionError, match="Adler"):
        R.check_file(rechunk(chunks), p)


def test_rejects_a_paeth_row(pages):
    p = pages["gray"][:20, :100]
    h, w = p.shape
    stream = bytearray(R.filter_rows(p, "none"))
    y = 5                                                            # row 5 refiltered with Paeth (type 4), a valid PNG still
    cur, up = p[y].astype(np.int32), p[y - 1].astype(np.int32)
    left = np.concatenate([[0], cur[:-1]])
    ul = np.concatenate([[0], up[:-1]])
    pa, pb, pc = np.abs(up - ul), np.abs(left - ul), np.abs(left + up - 2 * ul)
    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    stream[y * (w + 1)] = 4
    stream[y * (w + 1) + 1:(y + 1) * (w + 1)] = ((cur - pred) & 255).astype(np.uint8).tobytes()
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    data = R.ZLIB_HEADER + co.compress(bytes(stream)) + co.flush(zlib.Z_SYNC_FLUSH) + R.FINAL + struct.pack(
        ">I", zlib.adler32(bytes(stream)) & 0xffffffff)
    f = rechunk([(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)), (b"IDAT", data), (b"IEND", b"")])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), p)   # Pillow reads it: only the filter rule is broken
    with pytest.raises(AssertionError, match="filter types"):
        R.check_file(f, p)


def test_rejects_an_ancillary_chunk(pages):
    p = pages["page"]
    chunks = R.parse_chunks(R.build_file(p))
    chunks.insert(1, (b"tEXt", b"Comment\x00x"))
    with pytest.raises(AssertionError, match="other than"):
        R.check_file(rechunk(chunks), p)


def test_rejects_a_plain_pillow_file(pages):
    p = pages["page"]
    assert p.shape[0] * (1 + p[0].size) > R.CHUNK
    b = io.BytesIO()
    Image.fromarray(R.rgb_of(p)).save(b, "PNG")
    with pytest.raises(AssertionError):
        R.check_file(b.getvalue(), p)


def test_rejects_other_pixels(pages):
    p = pages["gray"]
    q = p.copy()
    q[3, 3] ^= 1
    with pytest.raises(AssertionError, match="pixels"):
        R.check_file(R.build_file(p), q)
