"""Checker and host builder for the PNG layout csrc/rtn_png_enc.hip writes: signature, IHDR, one IDAT per
independently deflated chunk of CHUNK raw bytes, IEND; row filters None / Sub / Up only.  Uses zlib, struct, NumPy and Pillow
alone.  check_file takes any file apart and raises AssertionError at the first rule it breaks; build_file writes a file of this
layout with the host's zlib (Z_SYNC_FLUSH per chunk), or with stored blocks only (the worst case the size bound is derived for).
tests/test_png_encode_ref.py proves the checker can fail."""
import io
import struct
import zlib

import numpy as np

CHUNK = 32768                                            # RTN_PNG_CHUNK
SIGNATURE = b"\x89PNG\r\n\x1a\n"
SYNC = b"\x00\x00\x00\xff\xff"                            # empty stored block, not final: ends a chunk byte-aligned
FINAL = b"\x01\x00\x00\xff\xff"                           # empty stored block, final
ZLIB_HEADER = b"\x78\x01"


def encode_bound(w, h, c, chunk=CHUNK):
    """rtn_png_encode_bound restated: signature + IHDR + IEND + per chunk (raw bytes + one stored-block header + sync flush +
    IDAT framing) + zlib header + final block + Adler-32; 0 for an invalid page."""
    if w < 1 or h < 1 or c not in (1, 3) or h * (1 + w * c) >= 2 ** 31:
        return 0
    stream = h * (1 + w * c)
    nchunks = (stream + chunk - 1) // chunk
    return 8 + 25 + 12 + stream + nchunks * (5 + 5 + 12) + 2 + 5 + 4


def rgb_of(page_bgr):
    a = np.ascontiguousarray(page_bgr)
    return np.ascontiguousarray(a[:, :, ::-1]) if a.ndim == 3 else a


def filter_rows(page_bgr, policy="minsum"):
    """The filtered stream (bytes) of a page: policy 'none' / 'sub' / 'up' (that filter on every row), 'minsum' (libpng's
    minimum sum of absolute values among None, Sub, Up), 'changes' (the device's rule: the fewest bytes that differ from the byte
    before them, ties to the lower type), or a callable (row index, [none, sub, up] rows as uint8) -> 0..2."""
    a = rgb_of(page_bgr)
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else 3
    rows = a.reshape(h, w * c)
    left = np.zeros_like(rows)
    left[:, c:] = rows[:, :-c]
    up = np.zeros_like(rows)
    up[1:] = rows[:-1]
    cand = [rows, rows - left, rows - up]                # uint8 arithmetic wraps mod 256
    if policy in ("none", "sub", "up"):
        pick = np.full(h, ("none", "sub", "up").index(policy))
    elif policy == "minsum":
        cost = np.stack([np.minimum(f, 256 - f.astype(np.int32)).sum(1) for f in cand])
        pick = cost.argmin(0)                             # ties: the lower filter type
    elif policy == "changes":
        pick = np.stack([(f[:, 1:] != f[:, :-1]).sum(1) for f in cand]).argmin(0)
    else:
        pick = np.array([policy(y, [f[y] for f in cand]) for y in range(h)])
    out = np.empty((h, 1 + w * c), np.uint8)
    out[:, 0] = pick
    for t in range(3):
        out[pick == t, 1:] = cand[t][pick == t]
    return out.tobytes()


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def _stored(raw):
    out = b""
    for i in range(0, max(len(raw), 1), 65535):
        part = raw[i:i + 65535]
        out += b"\x00" + struct.pack("<HH", len(part), len(part) ^ 0xffff) + part
    return out


def build_file(page_bgr, policy="minsum", level=1, stored=False, chunk=CHUNK):
    """A file of the layout for the page.  stored=True writes every chunk as stored blocks (the size bound's case)."""
    a = np.ascontiguousarray(page_bgr)
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else 3
    stream = filter_rows(a, policy)
    out = SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0))
    n = (len(stream) + chunk - 1) // chunk
    for k in range(n):
        raw = stream[k * chunk:(k + 1) * chunk]
        if stored:
            data = _stored(raw) + SYNC
        else:
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            data = co.compress(raw) + co.flush(zlib.Z_SYNC_FLUSH)
            assert data.endswith(SYNC[1:])
            if len(data) > len(_stored(raw)) + len(SYNC):
                data = _stored(raw) + SYNC
        if k == 0:
            data = ZLIB_HEADER + data
        if k == n - 1:
            data += FINAL + struct.pack(">I", zlib.adler32(stream) & 0xffffffff)
        out += _chunk(b"IDAT", data)
    return out + _chunk(b"IEND", b"")


def parse_chunks(data):
    """[(type, payload)] of a PNG file; verifies the signature, every CRC and that nothing follows IEND."""
    assert data[:8] == SIGNATURE, "signature"
    pos, chunks = 8, []
    while pos < len(data):
        assert pos + 12 <= len(data), "truncated chunk at %d" % pos
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        assert pos + 12 + n <= len(data), "chunk %r at %d runs past the file" % (kind, pos)
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xffffffff), "CRC of chunk %d (%r)" % (len(chunks), kind)
        chunks.append((kind, body))
        pos += 12 + n
        if kind == b"IEND":
            break
    assert pos == len(data), "%d bytes after IEND" % (len(data) - pos)
    return chunks


def _inflate_alone(body, k):
    """Raw bytes of one chunk's deflate data, inflated with no history; the data must end byte-aligned on the sync flush."""
    assert body.endswith(SYNC[1:]), "IDAT %d does not end with an empty stored block" % k
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(body)
    except zlib.error as e:
        raise AssertionError("IDAT %d does not inflate on its own: %s" % (k, e))
    assert not d.eof, "IDAT %d holds a final block before its end" % k
    assert d.unused_data == b"", "IDAT %d: bytes after the deflate data" % k
    # the empty stored block is a block of its own, byte-aligned: the data before its 4 length bytes inflates to the same bytes
    d2 = zlib.decompressobj(-15)
    assert d2.decompress(body[:-4]) == raw, "IDAT %d: the sync flush is not a block of its own" % k
    return raw


def unfilter(stream, w, h, c):
    """Undo filters None / Sub / Up of the filtered stream -> (h, w*c) uint8; any other filter type is an error."""
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + w * c)
    types = rows[:, 0]
    assert set(np.unique(types)) <= {0, 1, 2}, "filter types %s (only 0, 1, 2 allowed)" % sorted(set(types.tolist()))
    x = rows[:, 1:].copy()
    sub = types == 1
    if sub.any():                                         # Sub: prefix sum along the row, per channel
        s = x[sub].reshape(-1, w, c).astype(np.uint32)
        x[sub] = (np.cumsum(s, axis=1) & 255).astype(np.uint8).reshape(-1, w * c)
    out = np.zeros((h, w * c), np.uint8)
    prev = np.zeros(w * c, np.uint8)
    for y in range(h):                                    # Up: plus the reconstructed row above
        out[y] = x[y] + prev if types[y] == 2 else x[y]
        prev = out[y]
    return out


def check_file(data, page_bgr, chunk=CHUNK):
    """AssertionError unless `data` is a file of the layout that holds exactly page_bgr.  Returns the number of IDATs."""
    from PIL import Image
    a = np.ascontiguousarray(page_bgr)
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else 3
    chunks = parse_chunks(data)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND", "chunk order %s" % kinds[:3]
    assert all(k == b"IDAT" for k in kinds[1:-1]), "chunks other than IHDR, IDAT, IEND: %s" % sorted(set(kinds))
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0), "IHDR fields"
    assert chunks[-1][1] == b"", "IEND payload"
    idat = [b for _, b in chunks[1:-1]]
    stream_len = h * (1 + w * c)
    n = (stream_len + chunk - 1) // chunk
    assert len(idat) == n, "%d IDATs for %d chunks" % (len(idat), n)
    assert idat[0][:2] == ZLIB_HEADER, "zlib header"
    idat[0] = idat[0][2:]
    assert idat[-1][-9:-4] == FINAL, "final empty stored block"
    (adler,) = struct.unpack(">I", idat[-1][-4:])
    idat[-1] = idat[-1][:-9]
    parts = []
    for k, body in enumerate(idat):
        raw = _inflate_alone(body, k)
        want = min(chunk, stream_len - k * chunk)
        assert len(raw) == want, "IDAT %d inflates to %d bytes, its slice has %d" % (k, len(raw), want)
        parts.append(raw)
    stream = b"".join(parts)
    assert adler == (zlib.adler32(stream) & 0xffffffff), "Adler-32"
    # the concatenation is one valid zlib stream too (what every PNG reader sees)
    whole = zlib.decompress(b"".join(b for _, b in chunks[1:-1]))
    assert whole == stream, "the concatenated IDATs inflate to something else"
    got = unfilter(stream, w, h, c)
    want_rows = rgb_of(a).reshape(h, w * c)
    assert np.array_equal(got, want_rows), "pixels differ after undoing the filters"
    im = Image.open(io.BytesIO(data))
    assert im.mode == ("RGB" if c == 3 else "L"), im.mode
    assert np.array_equal(np.asarray(im).reshape(h, w * c), want_rows), "Pillow reads other pixels"
    return n
