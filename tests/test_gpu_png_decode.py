"""GPU tests of the device PNG decoder (csrc/rtn_png_dec.hip) behind read_images_bgr and decode_png_bgr.

The files are built on the host with zlib (tests/png_encode_ref.build_file and the builders below), so no test here but the round
trip depends on the device encoder.  The reference is read_image_bgr, Pillow's decode: the device's pages must have its bits, and
every file the device cannot vouch for (history carried across chunks, Paeth / Average rows, a mis-cut chunk, a wrong Adler-32 or
CRC, corrupted or truncated data) must come back through it, with a non-zero device status the tests can see."""
import importlib
import io
import os
import random
import struct
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POLICIES = ("none", "sub", "up", "minsum", "changes")
MODES = [(1, False), (6, False), (9, False), (1, True)]                # (level, stored)
COMBOS = [(p, l, s) for p in POLICIES for l, s in MODES]


@pytest.fixture(scope="module")
def U():
    return importlib.import_module("retinanet-for-table-detection_amd.model.utils")


@pytest.fixture(scope="module")
def CG():
    return importlib.import_module("retinanet-for-table-detection_amd.csv_generator")


@pytest.fixture(scope="module")
def P():
    return importlib.import_module("retinanet-for-table-detection_amd.model.preprocess")


@pytest.fixture(scope="module")
def PIO():
    return importlib.import_module("retinanet-for-table-detection_amd.model.page_io")


@pytest.fixture(scope="module")
def fixtures():
    """The three size fixtures, B,G,R (or gray): Pillow's decode of the golden JPEGs."""
    m = np.asarray(Image.open(os.path.join(GOLDEN, "sample_0717_023.jpg")).convert("RGB"))
    o = Image.open(os.path.join(GOLDEN, "sample_0717_023_orig.jpg"))
    return {"map": np.ascontiguousarray(m[:, :, ::-1]), "page": np.ascontiguousarray(np.asarray(o.convert("RGB"))[:, :, ::-1]),
            "gray": np.ascontiguousarray(np.asarray(o.convert("L")))}


def crops(fixtures):
    return [np.ascontiguousarray(fixtures["map"][300:397, 200:313]), np.ascontiguousarray(fixtures["gray"][1000:1300, 200:533]),
            np.ascontiguousarray(fixtures["page"][1000:1111, 3:1000])]


def host_pixels(data):
    """read_image_bgr of a file held in memory."""
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def bgr3(page):
    return page if page.ndim == 3 else np.repeat(page[:, :, None], 3, axis=2)


def payloads(data):
    idat = [b for k, b in R.parse_chunks(data) if k == b"IDAT"]
    idat[0] = idat[0][2:]
    idat[-1] = idat[-1][:-9]
    return idat


def assemble(w, h, c, datas, adler):
    """A file of the layout's shape from one deflate payload per IDAT (each ending on a sync flush) and the stream's Adler-32."""
    out = R.SIGNATURE + R._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0))
    for k, d in enumerate(datas):
        if k == 0:
            d = R.ZLIB_HEADER + d
        if k == len(datas) - 1:
            d = d + R.FINAL + struct.pack(">I", adler & 0xffffffff)
        out += R._chunk(b"IDAT", d)
    return out + R._chunk(b"IEND", b"")


def dims(page):
    return page.shape[1], page.shape[0], (3 if page.ndim == 3 else 1)


def multiblock_file(page, policy, level):
    """The layout, every chunk of more than 5,003 bytes in three runs of blocks: a sync flush after 5,000 bytes, a full flush three
    bytes later, the rest."""
    stream = R.filter_rows(page, policy)
    datas = []
    for k in range(0, len(stream), R.CHUNK):
        raw = stream[k:k + R.CHUNK]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        d = co.compress(raw[:5000]) + co.flush(zlib.Z_SYNC_FLUSH)
        if len(raw) > 5000:
            d += co.compress(raw[5000:5003]) + co.flush(zlib.Z_FULL_FLUSH)
        if len(raw) > 5003:
            d += co.compress(raw[5003:]) + co.flush(zlib.Z_SYNC_FLUSH)
        datas.append(d)
    return assemble(*dims(page), datas, zlib.adler32(stream))


def carried_history_file(page, level=6):
    """Layout-shaped, but written by ONE deflate stream flushed every CHUNK bytes: later chunks match into earlier ones."""
    stream = R.filter_rows(page, "minsum")
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    datas = [co.compress(stream[k:k + R.CHUNK]) + co.flush(zlib.Z_SYNC_FLUSH) for k in range(0, len(stream), R.CHUNK)]
    return assemble(*dims(page), datas, zlib.adler32(stream))


def chunked(stream, cuts=None):
    """One independently deflated payload per slice of the stream; cuts = the slice ends (default: every CHUNK bytes)."""
    cuts = cuts or list(range(R.CHUNK, len(stream), R.CHUNK)) + [len(stream)]
    datas, a = [], 0
    for b in cuts:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        datas.append(co.compress(stream[a:b]) + co.flush(zlib.Z_SYNC_FLUSH))
        a = b
    return datas


def filtered_with(page, ftype):
    """The filtered stream of an R,G,B page with filter type 3 (Average) or 4 (Paeth) on every row."""
    a = R.rgb_of(page).astype(np.int32)
    h, w = a.shape[:2]
    rows = a.reshape(h, w * 3)
    out = np.zeros((h, 1 + w * 3), np.uint8)
    out[:, 0] = ftype
    for y in range(h):
        up = rows[y - 1] if y else np.zeros(w * 3, np.int32)
        left = np.concatenate([np.zeros(3, np.int32), rows[y][:-3]])
        ul = np.concatenate([np.zeros(3, np.int32), up[:-3]])
        if ftype == 3:
            pred = (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out[y, 1:] = (rows[y] - pred) & 255
    return out.tobytes()


def write_all(tmp, files):
    paths = []
    for i, data in enumerate(files):
        p = tmp / ("f%04d.png" % i)
        p.write_bytes(data)
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def corpus(fixtures, tmp_path_factory):
    """(paths, files, pages): the layout over the encoder tests' shapes, contents, filter policies, levels and stored chunks."""
    rng = np.random.RandomState(2)
    smooth = lambda *s: (np.cumsum(rng.randint(0, 3, s), axis=1) & 255).astype(np.uint8)      # noqa: E731
    shapes = [(1, 1), (1, 1, 3), (1, 100), (1, 100, 3), (100, 1), (100, 1, 3), (1, 40000), (40000, 1, 3),
              (9, 5, 3), (9, 7, 3), (9, 6), (9, 7), (33, 47, 3), (13, 1001), (10, 100, 3),
              (8, 1365, 3), (16, 1365, 3), (64, 511), (32, 341, 3), (1, 32767), (1, 32768), (9, 1365, 3)]
    pages = [smooth(*s) for s in shapes] + [rng.randint(0, 256, s).astype(np.uint8) for s in shapes] + \
        [np.full(s, 37 + 5 * i, np.uint8) for i, s in enumerate(shapes)]
    files, owners = [], []
    for i, p in enumerate(pages):                                       # two of the twenty (policy, level / stored) settings per page
        for policy, level, stored in (COMBOS[i % 20], COMBOS[(7 * i + 3) % 20]):
            files.append(R.build_file(p, policy=policy, level=level, stored=stored))
            owners.append(p)
    for p in crops(fixtures):                                           # all twenty for the crops
        for policy, level, stored in COMBOS:
            files.append(R.build_file(p, policy=policy, level=level, stored=stored))
            owners.append(p)
    multi = (rng.randint(0, 16, (97, 113, 3)) * 16).astype(np.uint8)
    for p, policy, level in [(multi, "changes", 1), (crops(fixtures)[0], "sub", 6), (crops(fixtures)[1], "up", 9)]:
        files.append(multiblock_file(p, policy, level))
        owners.append(p)
    return write_all(tmp_path_factory.mktemp("png_corpus"), files), files, owners


def test_corpus_is_the_layout_with_every_block_type(CG, corpus):
    paths, files, pages = corpus
    types = set()
    for data, page in zip(files, pages):
        info, blob = CG.png_inspect(data)
        assert info is not None, blob
        assert (info.width, info.height, info.components) == dims(page)
        types |= {(p[0] >> 1) & 3 for p in payloads(data)}               # BTYPE of every IDAT's first block
    assert types == {0, 1, 2}
    for data, page in list(zip(files, pages))[-3:]:                      # the multi-block files: each IDAT still inflates alone
        R.check_file(data, page)


def test_device_decode_is_bit_identical(CG, corpus):
    paths, files, pages = corpus
    want = [CG.read_image_bgr(p) for p in paths]
    for w, page in zip(want, pages):
        assert np.array_equal(w, bgr3(page))
    got = CG.read_images_bgr(paths)                                      # one batch
    assert len(got) == len(paths)
    for p, w, g in zip(paths, want, got):
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == w.shape
        assert np.array_equal(g.cpu().numpy(), w), p
    for p, w in zip(paths, want):                                        # one file per call
        (g,) = CG.read_images_bgr([p])
        assert np.array_equal(g.cpu().numpy(), w), p


def test_device_path_is_taken(CG, U, PIO, corpus, monkeypatch):
    paths, files, pages = corpus

    def no_host(path):
        raise AssertionError("host decode of %s" % path)
    monkeypatch.setattr(PIO, "read_image_bgr", no_host)
    monkeypatch.setattr(Image, "open", no_host)
    out = CG.read_images_bgr(paths)
    assert len(out) == len(paths) and all(t.is_cuda for t in out)
    got, status = U.decode_png_bgr(files[:50], return_status=True)
    assert status == [0] * 50
    for g, page in zip(got, pages[:50]):
        assert np.array_equal(g.cpu().numpy(), bgr3(page))


def test_round_trip_with_the_device_encoder(U, fixtures):
    rng = np.random.RandomState(3)
    pages = crops(fixtures) + [np.zeros((300, 200, 3), np.uint8), np.full((500, 333), 128, np.uint8),
                               np.full((120, 90, 3), (23, 200, 141), np.uint8),
                               (np.cumsum(rng.randint(0, 3, (1, 40000)), axis=1) & 255).astype(np.uint8),
                               (np.cumsum(rng.randint(0, 3, (40000, 1, 3)), axis=0) & 255).astype(np.uint8), fixtures["map"]]
    for i in range(16):
        src = fixtures[("map", "page", "gray")[i % 3]]
        h, w = rng.randint(1, 600), rng.randint(1, 900)
        y, x = rng.randint(0, src.shape[0] - h), rng.randint(0, src.shape[1] - w)
        pages.append(np.ascontiguousarray(src[y:y + h, x:x + w]))
    files = U.encode_png_bgr(pages)
    got, status = U.decode_png_bgr(files, return_status=True)
    assert status == [0] * len(pages)
    for g, page in zip(got, pages):
        assert np.array_equal(g.cpu().numpy(), bgr3(page)), page.shape
    mixed = files[-16:]
    batch = U.decode_png_bgr(mixed)                                      # a batch of 16 mixed sizes; a page does not depend on its batch
    for f, b in zip(mixed, batch):
        (alone,) = U.decode_png_bgr([f])
        assert torch.equal(alone, b)
    assert U.decode_png_bgr([]) == []


def test_both_entry_points_share_one_reader(U, CG, PIO, tmp_path, monkeypatch):
    """read_images_bgr (files) and decode_png_bgr (bytes) take the same per-device handle of page_io._readers: whichever runs
    first creates it, the other finds it, and both give Pillow's pixels."""
    rng = np.random.RandomState(11)
    pages = [rng.randint(0, 256, (7, 5)).astype(np.uint8), rng.randint(0, 256, (33, 40, 3)).astype(np.uint8)]   # 5x7 gray, 40x33 colour
    paths = [str(tmp_path / ("p%d.png" % i)) for i in range(len(pages))]
    U.write_images_bgr(paths, pages, png="device")
    files = [open(p, "rb").read() for p in paths]
    want = [host_pixels(f) for f in files]
    for w, page in zip(want, pages):
        assert np.array_equal(w, bgr3(page))
    dev = torch.cuda.current_device()
    monkeypatch.setattr(PIO, "_readers", {})
    from_bytes, status = U.decode_png_bgr(files, return_status=True)
    assert status == [0, 0] and list(PIO._readers) == [dev]
    h = PIO._readers[dev]
    from_files = CG.read_images_bgr(paths)
    assert list(PIO._readers) == [dev] and PIO._readers[dev] is h
    for w, a, b in zip(want, from_bytes, from_files):
        assert a.is_cuda and b.is_cuda and np.array_equal(a.cpu().numpy(), w) and np.array_equal(b.cpu().numpy(), w)
    torch.cuda.synchronize()
    h.close()


def raw_decode(U, CG, handle, data):
    """(status word, page) of one inspected file through the C ABI alone."""
    import ctypes as C
    L = U.L
    info, blob = CG.png_inspect(data)
    assert info is not None, blob
    host = torch.empty(int(info.blob_bytes), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = blob
    dev = host.cuda()
    offs = np.zeros(1, np.int64)
    page = torch.zeros(info.height, info.width, 3, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    wsb = int(L.lib.rtn_png_decode_workspace_bytes(1, host.data_ptr(), offs.ctypes.data))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * 1)(page.data_ptr())
    handle.set_stream(torch.cuda.current_stream().cuda_stream)
    handle.check(L.lib.rtn_png_decode(handle.raw, 1, host.data_ptr(), dev.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(),
                                      ws.data_ptr(), wsb))
    torch.cuda.synchronize()
    return int(status[0]), page


def test_files_only_the_device_can_refuse(CG, U, fixtures, handle):
    """Layout-shaped files the inspector accepts and Pillow reads, whose chunks are not independent, not None / Sub / Up, not cut
    at the chunk edge, or not under the stored Adler-32: the device's status is non-zero and the pixels are Pillow's."""
    rng = np.random.RandomState(8)
    smooth = (np.cumsum(rng.randint(0, 3, (120, 200, 3)), axis=1) & 255).astype(np.uint8)
    files = []
    for page in (crops(fixtures)[0], smooth, np.full((120, 200, 3), (9, 80, 200), np.uint8)):
        data = carried_history_file(page)
        second = payloads(data)[1]
        with pytest.raises(zlib.error, match="distance too far back"):
            zlib.decompressobj(-15).decompress(second)
        files.append((data, page))
    small = np.ascontiguousarray(fixtures["page"][1000:1120, 300:420])    # 120 x 120 x 3: two chunks
    for ftype in (3, 4):
        stream = filtered_with(small, ftype)
        files.append((assemble(*dims(small), chunked(stream), zlib.adler32(stream)), small))
    stream = R.filter_rows(small, "sub")
    assert R.CHUNK < len(stream) < 2 * R.CHUNK
    files.append((assemble(*dims(small), chunked(stream, [R.CHUNK - 1, len(stream)]), zlib.adler32(stream)), small))
    good = R.build_file(small)
    files.append((good[:-20] + bytes([good[-20] ^ 1]) + good[-19:], small))     # the stored Adler-32 changed, the IDAT's CRC left stale
    bad_adler = assemble(*dims(small), chunked(R.filter_rows(small, "minsum")), zlib.adler32(R.filter_rows(small, "minsum")) ^ 0x10000)
    files.append((bad_adler, small))
    for data, page in files[:6]:
        info, why = CG.png_inspect(data)
        assert info is not None, why
        assert np.array_equal(host_pixels(data), page)
    outcomes = []
    for data, page in files:
        assert raw_decode(U, CG, handle, data)[0] > 0                    # the device's own word, whatever the host then does
        try:
            want = host_pixels(data)
        except Exception as e:                                           # Pillow may refuse a wrong Adler-32: then so must we
            with pytest.raises(type(e)):
                U.decode_png_bgr([data])
            outcomes.append(None)
            continue
        (got,), (status,) = U.decode_png_bgr([data], return_status=True)
        assert status not in (0, None), status
        assert np.array_equal(got.cpu().numpy(), want)
        outcomes.append(status)
    assert sum(s is not None for s in outcomes) >= 6
    # in one batch with good files: only the refused pages take the host path
    datas = [d for (d, _), s in zip(files, outcomes) if s is not None] + [good]
    pages, status = U.decode_png_bgr(datas, return_status=True)
    assert status[-1] == 0 and all(s for s in status[:-1])
    for d, g in zip(datas, pages):
        assert np.array_equal(g.cpu().numpy(), host_pixels(d))


def test_corrupted_and_truncated_files_behave_like_the_host(CG, tmp_path):
    rng = np.random.RandomState(11)
    page = (np.cumsum(rng.randint(0, 3, (97, 113, 3)), axis=1) & 255).astype(np.uint8)
    good = R.build_file(page, policy="sub", level=6)
    chunks = R.parse_chunks(good)
    assert len(chunks) == 4
    files = []
    for j in range(6):
        k = 1 + j % 2
        body = bytearray(chunks[k][1])
        lo, hi = (2, len(body) - 4) if k == 1 else (0, len(body) - 13)    # inside the deflate payload, before the sync marker
        for i in rng.randint(lo, hi, rng.randint(1, 4)):
            body[i] = (body[i] + 1 + rng.randint(0, 255)) % 256
        c = list(chunks)
        c[k] = (b"IDAT", bytes(body))
        data = R.SIGNATURE + b"".join(R._chunk(t, b) for t, b in c)       # the chunk CRC recomputed
        assert CG.png_inspect(data)[0] is not None
        files.append(data)
    files.append(good[: len(good) * 2 // 3])
    paths = write_all(tmp_path, files)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for p in paths:
            try:
                want = CG.read_image_bgr(p)
            except Exception as e:
                with pytest.raises(type(e)):
                    CG.read_images_bgr([p])
                continue
            (got,) = CG.read_images_bgr([p])
            assert np.array_equal(got.cpu().numpy(), want), p
    gp = tmp_path / "good.png"
    gp.write_bytes(good)
    (got,) = CG.read_images_bgr([str(gp)])                               # the process decodes a good file afterwards
    assert np.array_equal(got.cpu().numpy(), page)


def test_a_wrong_chunk_crc_goes_to_the_host(U):
    page = np.full((9, 7, 3), 77, np.uint8)
    data = bytearray(R.build_file(page))
    data[data.index(b"IEND") - 8] ^= 0x55
    try:
        want = host_pixels(bytes(data))
    except Exception as e:
        with pytest.raises(type(e)):
            U.decode_png_bgr([bytes(data)])
        return
    (got,), (status,) = U.decode_png_bgr([bytes(data)], return_status=True)
    assert status not in (0, None) and np.array_equal(got.cpu().numpy(), want)


def test_mixed_batch_keeps_order_dtype_and_device(CG, fixtures, tmp_path):
    img = np.ascontiguousarray(fixtures["page"][1000:1100, 300:480])
    rgb = img[:, :, ::-1]
    names = []
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=95)
    for name, data in [("a.jpg", b.getvalue()), ("b.png", R.build_file(img[:50])), ("c.png", None), ("d.bmp", None),
                       ("e.png", R.build_file(img[:, :, 0])), ("f.jpg", b.getvalue())]:
        p = tmp_path / name
        if data is None:
            Image.fromarray(rgb[10:]).save(p)
        else:
            p.write_bytes(data)
        names.append(str(p))
    want = [CG.read_image_bgr(p) for p in names]
    assert [w.shape[0] for w in want] == [100, 50, 90, 90, 100, 100]
    got = CG.read_images_bgr(names, device=0)
    for w, g in zip(want, got):
        assert g.dtype == torch.uint8 and g.device == torch.device("cuda", 0) and g.is_contiguous()
        assert np.array_equal(g.cpu().numpy(), w)


def make_png_dataset(tmp_path, n=5, seed=0):
    """The generator tests' dataset with its pages as layout PNGs under the CSV's .png names."""
    rng = np.random.RandomState(seed)
    d = tmp_path / "pages"
    d.mkdir()
    rows = ["image_id,xmin,ymin,xmax,ymax,label"]
    for i in range(n):
        h, w = int(rng.randint(300, 420)), int(rng.randint(240, 330))
        yy, xx = np.mgrid[0:h, 0:w]
        page = np.stack([(xx * 3 + yy) % 256, (yy * 2) % 256, ((xx + yy) // 2) % 256], -1)
        page = np.clip(page + rng.randint(-8, 9, page.shape), 0, 255).astype(np.uint8)
        name = "page_%02d.png" % i
        (d / name).write_bytes(R.build_file(page, policy=POLICIES[i % 5], level=(1, 6, 9)[i % 3]))
        for _ in range(int(rng.randint(1, 4))):
            bw, bh = rng.uniform(60, 200), rng.uniform(50, 200)
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
            rows.append("%s,%.2f,%.2f,%.2f,%.2f,table" % (name, x1, y1, x1 + bw, y1 + bh))
    csvf = tmp_path / "train.csv"
    csvf.write_text("\n".join(rows) + "\n")
    return str(csvf), str(d)


def generator_batches(CG, csvf, d, augment):
    T = importlib.import_module("retinanet-for-table-detection_amd.model.transform")
    random.seed(1)
    kw = dict(batch_size=2, group_method="none", shuffle_groups=False, image_min_side=224, image_max_side=288, dtype=torch.float32)
    if augment:
        kw.update(transform_generator=T.random_transform_generator(prng=np.random.RandomState(21), min_rotation=-0.1, max_rotation=0.1,
                                                                   flip_x_chance=0.5, min_scaling=(0.9, 0.9), max_scaling=(1.1, 1.1)),
                  transform_parameters=T.TransformParameters())
    gen = CG.CSVGenerator(csvf, d, {"table": 0}, **kw)
    out = []
    for gi in range(len(gen)):
        x, (reg, lab) = gen[gi]
        out.append((x.cpu().numpy(), reg.cpu().numpy(), lab.cpu().numpy()))
    gen.close()
    return out


@pytest.mark.parametrize("augment", [False, True])
def test_generator_over_layout_png_pages(CG, PIO, tmp_path, monkeypatch, augment):
    csvf, d = make_png_dataset(tmp_path)
    device = generator_batches(CG, csvf, d, augment)
    with monkeypatch.context() as m:                                     # the same dataset decoded by read_image_bgr, page by page
        m.setattr(CG.CSVGenerator, "load_image_group", CG.Generator.load_image_group)
        host = generator_batches(CG, csvf, d, augment)
    assert len(device) == len(host) == 3
    for a, b in zip(device, host):
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y)

    def no_host(path):
        raise AssertionError("host decode of %s" % path)
    monkeypatch.setattr(PIO, "read_image_bgr", no_host)
    monkeypatch.setattr(CG, "read_image_bgr", no_host)          # CSVGenerator.load_image looks the name up there
    again = generator_batches(CG, csvf, d, augment)
    for a, b in zip(again, host):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_preprocess_files_from_layout_png(PIO, P, fixtures, tmp_path, monkeypatch):
    pages = [np.ascontiguousarray(fixtures["page"][200:500, 100:340]), np.ascontiguousarray(fixtures["page"][900:1160, 600:1010]),
             np.ascontiguousarray(fixtures["map"][:260, :410])]
    src = []
    for i, p in enumerate(pages):
        f = tmp_path / ("src%d.png" % i)
        f.write_bytes(R.build_file(p, policy=POLICIES[1 + i], level=6))
        src.append(str(f))
    dst = [str(tmp_path / ("o%d.png" % i)) for i in range(len(pages))]
    want = [P.preprocess_pages(p) for p in pages]

    def no_host(*a, **k):
        raise AssertionError("host image reader or writer")
    monkeypatch.setattr(PIO, "read_image_bgr", no_host)
    monkeypatch.setattr(PIO, "write_image", no_host)
    P.preprocess_files(src, dst, png="device")
    for d, w in zip(dst, want):
        R.check_file(open(d, "rb").read(), w)


def test_c_abi_rejects_bad_arguments(U, CG, handle):
    import ctypes as C
    L = U.L
    info, blob = CG.png_inspect(R.build_file(np.zeros((4, 4, 3), np.uint8)))
    host = torch.empty(int(info.blob_bytes), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = blob
    dev = host.cuda()
    offs = np.zeros(1, np.int64)
    page = torch.empty(4, 4, 3, dtype=torch.uint8, device="cuda")
    status = torch.empty(1, dtype=torch.int32, device="cuda")
    wsb = int(L.lib.rtn_png_decode_workspace_bytes(1, host.data_ptr(), offs.ctypes.data))
    assert wsb == info.workspace_bytes > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * 1)(page.data_ptr())
    call = lambda *a: L.lib.rtn_png_decode(handle.raw, *a)               # noqa: E731
    assert call(1, host.data_ptr(), dev.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(), ws.data_ptr(), wsb) == 0
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(page.max()) == 0
    assert raw_decode(U, CG, handle, R.build_file(np.full((5, 6), 9, np.uint8)))[0] == 0
    assert call(0, None, None, None, None, None, None, 0) == 0
    assert call(1, None, dev.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(), ws.data_ptr(), wsb) == -1
    assert call(1, host.data_ptr(), dev.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(), ws.data_ptr(), wsb - 1) != 0
    assert call(1, host.data_ptr(), dev.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(), ws.data_ptr() + 16, wsb) == -1
    host.numpy()[0] ^= 1                                                 # not a blob any more
    assert L.lib.rtn_png_decode_workspace_bytes(1, host.data_ptr(), offs.ctypes.data) == 0
    assert call(1, host.data_ptr(), dev.data_ptr(), offs.ctypes.data, ptrs, status.data_ptr(), ws.data_ptr(), wsb) == -1
