"""CPU tests of the host half of the device PNG decoder (csrc/rtn_png_dec.hip): what rtn_png_inspect accepts (files of the chunked
layout of DESIGN §3.4d, built here with zlib by tests/png_encode_ref.py) and what it sends to the host decoder with a reason, and
rtn_png_inflate_chunk_host, which runs the device's inflate functions (csrc/rtn_png_inflate.h) on a CPU, against zlib on valid,
mutated and truncated payloads.  No kernel is launched here."""
import ctypes as C
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inspect(pkg, data, with_blob=True, capacity=None):
    L = pkg._lib
    info = L.PngInfo()
    blob = np.zeros(L.png_blob_bound(len(data)), np.uint8)
    cap = blob.size if capacity is None else capacity
    rc = L.lib.rtn_png_inspect(None, data, len(data), C.byref(info), blob.ctypes.data if with_blob else None, cap)
    return rc, info, L.lib.rtn_last_error(None).decode()


def page(shape, seed=0):
    rng = np.random.RandomState(seed)
    h, w = shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    base = (xx * 3 + yy * 2) % 256
    if len(shape) == 3:
        base = np.stack([base, (yy * 5) % 256, ((xx + yy) // 2) % 256], -1)
    return np.clip(base + rng.randint(-3, 4, base.shape), 0, 255).astype(np.uint8)


def rebuild(chunks):
    return R.SIGNATURE + b"".join(R._chunk(k, b) for k, b in chunks)


@pytest.mark.parametrize("shape", [(1, 1), (1, 1, 3), (9, 7, 3), (97, 113, 3), (8, 1365, 3), (1, 32768)])
def test_accepts_the_layout(pkg, shape):
    data = R.build_file(page(shape))
    rc, info, why = inspect(pkg, data)
    assert rc == 0, why
    h, w = shape[:2]
    c = 3 if len(shape) == 3 else 1
    stream = h * (1 + w * c)
    assert (info.width, info.height, info.components) == (w, h, c)
    assert info.chunks == (stream + R.CHUNK - 1) // R.CHUNK
    assert info.blob_bytes % 16 == 0 and 0 < info.blob_bytes <= pkg._lib.png_blob_bound(len(data))
    assert info.workspace_bytes >= stream and info.payload_bytes > 0
    rc2, info2, _ = inspect(pkg, data, with_blob=False)
    assert rc2 == 0 and (info2.width, info2.height, info2.chunks, info2.blob_bytes) == (w, h, info.chunks, info.blob_bytes)
    rc3, _, why3 = inspect(pkg, data, capacity=info.blob_bytes - 1)
    assert rc3 == -1 and "capacity" in why3
    assert inspect(pkg, data, capacity=info.blob_bytes)[0] == 0


def test_chunk_counts_of_the_edge_shapes(pkg):
    counts = {}
    for shape in [(97, 113, 3), (8, 1365, 3), (1, 32768)]:
        counts[shape] = inspect(pkg, R.build_file(page(shape)))[1].chunks
    assert counts == {(97, 113, 3): 2, (8, 1365, 3): 1, (1, 32768): 2}
    for stored in (False, True):
        for level in (1, 9):
            assert inspect(pkg, R.build_file(page((40, 30, 3)), policy="sub", level=level, stored=stored))[0] == 0


def pillow_file(img, **kw):
    b = io.BytesIO()
    img.save(b, "PNG", **kw)
    return b.getvalue()


def test_rejects_other_pngs_with_a_reason(pkg):
    rgb = page((20, 30, 3))
    files = {
        "L": pillow_file(Image.fromarray(rgb[..., 0])),
        "RGB": pillow_file(Image.fromarray(rgb)),
        "RGBA": pillow_file(Image.fromarray(np.dstack([rgb, rgb[..., :1]]))),
        "P": pillow_file(Image.fromarray(rgb).convert("P")),
        "I;16": pillow_file(Image.fromarray((rgb[..., 0].astype(np.uint16) * 257))),
    }
    for name, data in files.items():
        rc, _, why = inspect(pkg, data)
        assert rc == -1 and why, name
    assert "colour type" in inspect(pkg, files["RGBA"])[2] and "colour type" in inspect(pkg, files["P"])[2]
    assert "bit depth" in inspect(pkg, files["I;16"])[2]
    # an interlaced file (Pillow does not write one): a layout file with the IHDR's interlace byte set
    chunks = R.parse_chunks(R.build_file(rgb))
    inter = rebuild([(b"IHDR", chunks[0][1][:12] + b"\x01")] + chunks[1:])
    rc, _, why = inspect(pkg, inter)
    assert rc == -1 and "interlace" in why
    Image.open(io.BytesIO(files["RGB"])).load()                        # what they all are: files Pillow reads


def test_rejects_broken_layouts_with_a_reason(pkg):
    img = page((97, 113, 3))
    good = R.build_file(img)
    chunks = R.parse_chunks(good)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IDAT", b"IEND"]
    assert inspect(pkg, rebuild(chunks))[0] == 0

    def refused(data, word):
        rc, _, why = inspect(pkg, data)
        assert rc == -1 and word in why, (word, why)

    refused(rebuild(chunks[:1] + [(b"tEXt", b"Comment\0hello")] + chunks[1:]), "chunk")
    refused(rebuild(chunks[:2] + [(b"tEXt", b"Comment\0hello")] + chunks[2:]), "chunk")
    refused(rebuild(chunks[:3] + [(b"tEXt", b"Comment\0hello")] + chunks[3:]), "chunk")
    refused(R.build_file(img, chunk=16384), "IDAT")
    refused(rebuild(chunks[:2] + chunks[3:]), "IDAT")                  # an IDAT removed
    refused(rebuild(chunks[:3] + chunks[2:]), "IDAT")                  # one too many
    body = chunks[1][1]
    refused(rebuild([chunks[0], (b"IDAT", body[:-1] + b"\xfe")] + chunks[2:]), "empty stored block")
    refused(rebuild([chunks[0], (b"IDAT", body[:-5])] + chunks[2:]), "empty stored block")
    for hdr in (b"\x78\x02", b"\x79\x01", b"\x78\x20", b"\x88\x1c"):   # check bits, method, preset dictionary, window too large
        refused(rebuild([chunks[0], (b"IDAT", hdr + body[2:])] + chunks[2:]), "zlib header")
    last = chunks[2][1]
    refused(rebuild(chunks[:2] + [(b"IDAT", last[:-9] + last[-4:]), chunks[3]]), "final")     # no final block
    refused(rebuild(chunks[:2] + [(b"IDAT", last[:-9] + b"\x00" + last[-8:]), chunks[3]]), "final")
    refused(good + b"\0", "after IEND")
    refused(good + good[-12:], "after IEND")
    refused(rebuild(chunks[:3] + [(b"IEND", b"x")]), "IEND")
    ihdr = bytearray(good)
    ihdr[30] ^= 1
    refused(bytes(ihdr), "CRC of IHDR")
    zero = rebuild([(b"IHDR", struct.pack(">IIBBBBB", 0, 5, 8, 2, 0, 0, 0))] + chunks[1:])
    refused(zero, "sides")
    huge = rebuild([(b"IHDR", struct.pack(">IIBBBBB", 40000, 40000, 8, 2, 0, 0, 0))] + chunks[1:])
    refused(huge, "2^31")


def test_every_proper_prefix_is_refused(pkg):
    data = R.build_file(page((9, 7, 3)))
    assert inspect(pkg, data)[0] == 0
    for n in range(len(data)):
        rc, _, why = inspect(pkg, data[:n])
        assert rc == -1 and why, n
    L = pkg._lib
    info = L.PngInfo()
    assert L.lib.rtn_png_inspect(None, None, 10, C.byref(info), None, 0) == -1
    assert L.lib.rtn_png_inspect(None, data, len(data), None, None, 0) == -1


def test_chunk_crcs_are_left_to_the_device(pkg):
    """rtn_png_inspect does not compute the IDAT CRCs (the device does, see tests/test_gpu_png_decode.py): the stored value
    travels in the blob's table."""
    data = bytearray(R.build_file(page((9, 7, 3))))
    at = data.index(b"IEND") - 8                                       # the IDAT's CRC
    data[at] ^= 0x55
    rc, info, why = inspect(pkg, bytes(data))
    assert rc == 0, why


# ---- rtn_png_inflate_chunk_host against zlib --------------------------------------------------------------------------------------------
def payloads_of(data):
    """The deflate payload of every IDAT of a layout file."""
    idat = [b for k, b in R.parse_chunks(data) if k == b"IDAT"]
    idat[0] = idat[0][2:]
    idat[-1] = idat[-1][:-9]
    return idat


def zlib_says(payload, want):
    """The bytes, if zlib inflates the payload as raw deflate on its own, through non-final blocks, exactly to the sync marker that
    ends it, to `want` bytes; else None."""
    if len(payload) < 5 or payload[-4:] != R.SYNC[1:]:
        return None
    try:
        d = zlib.decompressobj(-15)
        raw = d.decompress(payload)
        if d.eof or len(raw) != want:
            return None
        if zlib.decompressobj(-15).decompress(payload[:-4]) != raw:    # the sync marker is a block of its own
            return None
        d3 = zlib.decompressobj(-15)                                   # ... after which the next block starts
        if d3.decompress(payload + R.FINAL) != raw or not d3.eof or d3.unused_data:
            return None
    except zlib.error:
        return None
    return raw


def inflate_host(pkg, payload, want):
    L = pkg._lib
    guard = 64
    buf = np.full(want + 2 * guard, 0xA5, np.uint8)
    st = C.c_int32(-1)
    rc = L.lib.rtn_png_inflate_chunk_host(payload, len(payload), buf.ctypes.data + guard, want, C.byref(st))
    assert rc == 0
    assert (buf[:guard] == 0xA5).all() and (buf[guard + want:] == 0xA5).all(), "guard bytes"
    if st.value != 0:
        assert (buf == 0xA5).all(), "output written with status %d" % st.value
    return st.value, buf[guard:guard + want].tobytes()


def fuzz_cases():
    rng = np.random.RandomState(20260)
    noise = rng.randint(0, 256, (20, 30, 3)).astype(np.uint8)
    const = np.full((60, 70, 3), 200, np.uint8)
    sources = []
    for img, policy in [(page((40, 50, 3)), "minsum"), (noise, "none"), (const, "up"), (page((97, 113)), "sub"),
                        (page((97, 113, 3), 3), "changes"), (np.zeros((1, 1), np.uint8), "none")]:
        for level, stored in [(1, False), (6, False), (9, False), (1, True)]:
            data = R.build_file(img, policy=policy, level=level, stored=stored)
            h, w = img.shape[:2]
            stream = h * (1 + w * (3 if img.ndim == 3 else 1))
            for k, p in enumerate(payloads_of(data)):
                sources.append((p, min(R.CHUNK, stream - k * R.CHUNK)))
    cases = []
    for p, want in sources:
        cases.append((p, want))
        if want < R.CHUNK:
            cases.append((p, want + 1))
        if want > 1:
            cases.append((p, want - 1))
        for _ in range(70):
            q = bytearray(p)
            for _ in range(rng.randint(1, 4)):
                q[rng.randint(len(q))] = rng.randint(256)
            cases.append((bytes(q), want))
        for _ in range(12):
            cut = rng.randint(0, len(p))
            cases.append((p[:cut], want))
            cases.append((p[:cut] + R.SYNC[1:], want))                 # a truncation that still ends like a chunk
            cases.append((p[:cut] + R.SYNC, want))
    return sources, cases


def test_inflate_chunk_host_agrees_with_zlib(pkg):
    sources, cases = fuzz_cases()
    assert len(cases) >= 2000
    accepted = refused = 0
    for p, want in sources:
        st, got = inflate_host(pkg, p, want)
        assert st == 0 and got == zlib.decompressobj(-15).decompress(p)
    for n, (p, want) in enumerate(cases):
        ref = zlib_says(p, want)
        st, got = inflate_host(pkg, p, want)
        if ref is None:
            assert st != 0, "case %d: zlib refuses, status 0" % n
            refused += 1
        else:
            assert st == 0 and got == ref, "case %d: zlib accepts, status %d" % (n, st)
            accepted += 1
    assert accepted > len(sources) and refused > 1000, (accepted, refused)


def test_inflate_chunk_host_block_types_and_rules(pkg):
    """Hand-made payloads: fixed and multi-block chunks, a final block, a match before the chunk, a too long stored block."""
    raw = bytes(range(256)) * 8
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    fixed = co.compress(raw) + co.flush(zlib.Z_SYNC_FLUSH)
    assert (fixed[0] >> 1) & 3 == 1
    st, got = inflate_host(pkg, fixed, len(raw))
    assert st == 0 and got == raw
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    multi = co.compress(raw[:1000]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(raw[1000:1003]) + co.flush(zlib.Z_FULL_FLUSH) + \
        co.compress(raw[1003:]) + co.flush(zlib.Z_SYNC_FLUSH)
    st, got = inflate_host(pkg, multi, len(raw))
    assert st == 0 and got == raw
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    final = co.compress(raw) + co.flush(zlib.Z_FINISH)
    assert inflate_host(pkg, final + R.SYNC, len(raw))[0] != 0
    co = zlib.compressobj(6, zlib.DEFLATED, -15)                       # second half of a stream: its matches reach into the first
    co.compress(raw[:1024])
    co.flush(zlib.Z_SYNC_FLUSH)
    second = co.compress(raw[1024:]) + co.flush(zlib.Z_SYNC_FLUSH)
    assert zlib_says(second, len(raw) - 1024) is None
    assert inflate_host(pkg, second, len(raw) - 1024)[0] != 0
    stored = b"\x00" + struct.pack("<HH", 40, 40 ^ 0xffff) + raw[:40] + R.SYNC
    assert inflate_host(pkg, stored, 40) == (0, raw[:40])
    assert inflate_host(pkg, stored, 39)[0] != 0 and inflate_host(pkg, stored, 41)[0] != 0
    assert inflate_host(pkg, b"\x06" + R.SYNC[1:], 1)[0] != 0          # block type 3
    L = pkg._lib
    st = C.c_int32(0)
    out = np.zeros(8, np.uint8)
    assert L.lib.rtn_png_inflate_chunk_host(stored, len(stored), out.ctypes.data, 0, C.byref(st)) == -1
    assert L.lib.rtn_png_inflate_chunk_host(stored, len(stored), out.ctypes.data, R.CHUNK + 1, C.byref(st)) == -1


def test_png_info_layout_matches_header(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtn.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(rtn_png_info_t),offsetof(rtn_png_info_t,components),offsetof(rtn_png_info_t,chunks),'
                   'offsetof(rtn_png_info_t,blob_bytes),offsetof(rtn_png_info_t,workspace_bytes),offsetof(rtn_png_info_t,payload_bytes),'
                   '(size_t)RTN_PNG_BLOB_BOUND(1000));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    L = pkg._lib
    P = L.PngInfo
    assert got == [C.sizeof(P), P.components.offset, P.chunks.offset, P.blob_bytes.offset, P.workspace_bytes.offset,
                   P.payload_bytes.offset, L.png_blob_bound(1000)]
