"""NumPy restatement of the baseline JPEG encoder csrc/rtn_jpeg_enc.hip reproduces (libjpeg-turbo as Pillow runs it), written from
the libjpeg rules listed in DESIGN §3.4c.  A diagnostic, not part of the product: it splits a file into its stages, so a device
mismatch can be located to the coefficients (colour conversion, edges, downsampling, FDCT, quantisation, dummy blocks) or to the
bitstream (DC prediction, Huffman coding, stuffing).  tests/test_jpeg_encode_ref.py checks it against Pillow."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])                          # zig-zag index -> natural index
BASE_QUANT = [                                                       # Annex K.1, zig-zag order
    [16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92,
     101, 103, 99],
    [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66] + [99] * 50]
HUFF_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
             [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]]


def _ac_vals(first):
    """Annex K.3 AC symbol orders: the listed leading symbols, then every other run/size symbol in increasing order."""
    rest = [s for s in range(256) if (s & 15) in range(1, 11) and s not in first]
    return first + rest


HUFF_VALS = [list(range(12)),
             _ac_vals([0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
                       0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
                       0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
                       0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
                       0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
                       0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
                       0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
                       0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
                       0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1]),
             list(range(12)),
             _ac_vals([0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
                       0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
                       0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1])]


def quant_table(t, quality):
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): zig-zag order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(BASE_QUANT[t]) * scale + 50) // 100, 1, 255)


def _fdct_1d(d, pass1):
    """jfdctint.c jpeg_fdct_islow along the last axis (int64)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if pass1 else 15
    ds = lambda x: (x + (1 << (sh - 1))) >> sh                            # noqa: E731
    o = np.empty_like(d)
    o[..., 0], o[..., 4] = ((t10 + t11) * 4, (t10 - t11) * 4) if pass1 else ((t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2)
    z1 = (t12 + t13) * 4433
    o[..., 2], o[..., 6] = ds(z1 + t13 * 6270), ds(z1 - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7], o[..., 5] = ds(t4 * 2446 + z1 + z3), ds(t5 * 16819 + z2 + z4)
    o[..., 3], o[..., 1] = ds(t6 * 25172 + z2 + z3), ds(t7 * 12299 + z1 + z4)
    return o


def _blocks(plane):
    """(rows, cols) plane, multiples of 8 -> (rows/8, cols/8, 64) zig-zagged quantisation-ready FDCT input"""
    r, c = plane.shape
    return plane.reshape(r // 8, 8, c // 8, 8).transpose(0, 2, 1, 3).reshape(r // 8, c // 8, 8, 8)


def _quantised(plane, qt):
    d = _blocks(plane.astype(np.int64) - 128)
    d = _fdct_1d(_fdct_1d(d, True).swapaxes(-1, -2), False).swapaxes(-1, -2)
    x = d.reshape(d.shape[:2] + (64,))[..., ZIGZAG]
    qd = 8 * qt
    return np.where(x < 0, -((-x + qd // 2) // qd), (x + qd // 2) // qd)


def coefficients(page, quality, subsampling):
    """The quantised, zig-zagged coefficients of every block in scan order (dummy blocks included): int64 (nblocks, 64)."""
    a = np.asarray(page)
    H, W = a.shape[:2]
    if a.ndim == 2:
        mx, my = -(-W // 8), -(-H // 8)
        plane = np.pad(a, ((0, my * 8 - H), (0, mx * 8 - W)), mode="edge")
        return _quantised(plane, quant_table(0, quality)).reshape(-1, 64)
    hm, vm = (1, 1) if subsampling == 0 else ((2, 1) if subsampling == 1 else (2, 2))
    mx, my = -(-W // (8 * hm)), -(-H // (8 * vm))
    b, g, r = [a[..., i].astype(np.int64) for i in range(3)]
    ycc = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
           (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
           (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    hpad = -(-H // vm) * vm                                              # input rows replicated to a multiple of v_max only
    full = [np.pad(p, ((0, hpad - H), (0, mx * hm * 8 - W)), mode="edge") for p in ycc]
    luma = np.pad(full[0], ((0, my * vm * 8 - hpad), (0, 0)), mode="edge")
    chroma = []
    for p in full[1:]:
        if hm == 2 and vm == 2:
            s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
            s = (s + (1 + (np.arange(s.shape[1]) & 1))) >> 2             # bias 1, 2, 1, 2, ...
        elif hm == 2:
            s = (p[:, 0::2] + p[:, 1::2] + (np.arange(p.shape[1] // 2) & 1)) >> 1
        else:
            s = p
        chroma.append(np.pad(s, ((0, my * 8 - s.shape[0]), (0, 0)), mode="edge"))   # last downsampled row to the iMCU height
    Y = _quantised(luma, quant_table(0, quality))
    C = [_quantised(p, quant_table(1, quality)) for p in chroma]
    wib, hib = -(-W // 8), -(-H // 8)
    for by in range(Y.shape[0]):                                         # jccoefct.c compress_data dummy blocks
        for bx in range(Y.shape[1]):
            if by >= hib:
                src = Y[by - 1, min((bx // hm) * hm + hm - 1, wib - 1), 0]
            elif bx >= wib:
                src = Y[by, wib - 1, 0]
            else:
                continue
            Y[by, bx] = 0
            Y[by, bx, 0] = src
    out = []
    for j in range(my):
        for i in range(mx):
            out += [Y[j * vm + dy, i * hm + dx] for dy in range(vm) for dx in range(hm)]
            out += [C[0][j, i], C[1][j, i]]
    return np.array(out)


def _codes(t, huff=None):
    bits, vals = (HUFF_BITS[t], HUFF_VALS[t]) if huff is None else huff[t]
    codes, code, k = {}, 0, 0
    for length, count in enumerate(bits, 1):
        for _ in range(count):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def scan(coefs, components, subsampling, huff=None):
    """The entropy-coded segment of the blocks in scan order: DC prediction per component, Huffman coding with the standard
    tables (or huff: four (bits, vals) pairs in the order of HUFF_BITS), 1-bit padding, 0xFF stuffing."""
    hm, vm = (1, 1) if components == 1 or subsampling == 0 else ((2, 1) if subsampling == 1 else (2, 2))
    comp = [0] if components == 1 else [0] * (hm * vm) + [1, 2]
    tabs = [(_codes(0, huff), _codes(1, huff)), (_codes(2, huff), _codes(3, huff))]
    bits = []
    pred = [0, 0, 0]

    def put(v, n):
        bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def field(codes, sym, v, n):
        code, length = codes[sym]
        put(code, length)
        if n:
            put(v if v >= 0 else v - 1 + (1 << n), n)
    for j, blk in enumerate(coefs):
        c = comp[j % len(comp)]
        dc, ac = tabs[0 if c == 0 else 1]
        diff = int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
        field(dc, int(abs(diff)).bit_length(), diff, int(abs(diff)).bit_length())
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                field(ac, 0xF0, 0, 0)
                run -= 16
            n = abs(v).bit_length()
            field(ac, (run << 4) | n, v, n)
            run = 0
        if run:
            field(ac, 0x00, 0, 0)
    bits += [1] * (-len(bits) % 8)
    out = bytearray()
    for i in range(0, len(bits), 8):
        byte = int("".join(map(str, bits[i:i + 8])), 2)
        out.append(byte)
        if byte == 0xFF:
            out.append(0)
    return bytes(out)
