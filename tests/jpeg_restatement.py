"""NumPy restatement of the baseline JPEG encoder (footprints_amd/csrc/jpeg.hip), written for reading rather than speed: what Pillow's
`Image.fromarray(a).save(f, format="JPEG", quality=q)` writes for an RGB picture with default options on libjpeg-turbo (or libjpeg 6b) --
sequential DCT (SOF0), YCbCr 4:2:0 in one interleaved scan, no restart markers, the standard Huffman tables, optimize=False.

Nothing of a header is stated here: `parse_header` reads quantisation and Huffman tables out of any file of the library at the wanted
quality, and the file of an h x w picture is those header bytes with SOF0's size patched, the scan and FF D9.  `encode` also counts what
the tests want their cases to cover: 0xF0 run codes, stuffed FF bytes, dummy blocks beyond the right and below the bottom edge."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def parse_header(data):
    """bytes of a baseline file -> dict(header = the bytes up to and including SOS, size_at = index of SOF0's height, quant = {id: 64
    values in zigzag order}, huff = {class << 4 | id: {symbol: (code, length)}})"""
    assert data[:2] == b"\xff\xd8"
    quant, huff, size_at, i = {}, {}, None, 2
    while True:
        assert data[i] == 0xFF
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        body = data[i + 4:i + 2 + length]
        if marker == 0xDB:
            for p in range(0, len(body), 65):
                assert body[p] >> 4 == 0                                        # 8-bit entries
                quant[body[p] & 15] = [int(v) for v in body[p + 1:p + 65]]
        elif marker == 0xC4:
            p = 0
            while p < len(body):
                counts = list(body[p + 1:p + 17])
                values = list(body[p + 17:p + 17 + sum(counts)])
                code, k, table = 0, 0, {}
                for bits in range(1, 17):                                       # canonical codes: counting up, a zero appended per length
                    for _ in range(counts[bits - 1]):
                        table[values[k]] = (code, bits)
                        code += 1
                        k += 1
                    code <<= 1
                huff[body[p]] = table
                p += 17 + len(values)
        elif marker == 0xC0:
            size_at = i + 5
        elif marker == 0xDA:
            return dict(header=bytes(data[:i + 2 + length]), size_at=size_at, quant=quant, huff=huff)
        i += 2 + length


def file_header(tables, h, w):
    at = tables["size_at"]
    return tables["header"][:at] + bytes((h >> 8, h & 255, w >> 8, w & 255)) + tables["header"][at + 4:]


def fix(x):
    return int(x * 65536 + 0.5)


def colour(a):
    """libjpeg's 16-bit fixed point RGB -> YCbCr"""
    R, G, B = (a[..., k].astype(np.int64) for k in range(3))
    Y = (fix(.299) * R + fix(.587) * G + fix(.114) * B + 32768) >> 16
    Cb = (-fix(.16874) * R - fix(.33126) * G + fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (fix(.5) * R - fix(.41869) * G - fix(.08131) * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def pad_edge(x, h, w):
    return np.pad(x, ((0, max(0, h - x.shape[0])), (0, max(0, w - x.shape[1]))), mode="edge")


def downsample(x):
    s = x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)                      # 1 on even output columns, 2 on odd ones
    return (s + bias) >> 2


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_pass(d, first):
    """jfdctint's 8-point pass along the last axis"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t1, t2, t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4
    t4, t5, t6, t7 = d3 - d4, d2 - d5, d1 - d6, d0 - d7
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4], n = (t10 + t11) << 2, (t10 - t11) << 2, 11
    else:
        out[0], out[4], n = descale(t10 + t11, 2), descale(t10 - t11, 2), 15
    z1 = (t12 + t13) * 4433
    out[2] = descale(z1 + t13 * 6270, n)
    out[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069, z4 * -3196
    z3, z4 = z3 + z5, z4 + z5
    out[7], out[5], out[3], out[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def fdct(blocks):
    """[..., 8, 8] level-shifted samples: rows first, then columns"""
    rows = fdct_pass(blocks, True)
    return fdct_pass(rows.swapaxes(-1, -2), False).swapaxes(-1, -2)


def quantise(coef, quant_zigzag):
    natural = np.zeros(64, dtype=np.int64)
    natural[ZIGZAG] = quant_zigzag
    div = (natural << 3).reshape(8, 8)
    t = (np.abs(coef) + (div >> 1)) // div
    return np.where(coef < 0, -t, t)


def planes(a):
    """the three component planes as the DCT sees them, padded to whole blocks"""
    H, W, _ = a.shape
    Y, Cb, Cr = colour(a)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    cwib, chib = (cw + 7) // 8, (ch + 7) // 8

    def chroma(c):
        # replication comes before the downsample horizontally (16 columns per block column) and for the one row that completes a row
        # pair, after it for the rows that complete a block
        return pad_edge(downsample(pad_edge(c, 2 * ch, 16 * cwib)), 8 * chib, 8 * cwib)
    return pad_edge(Y, 8 * ((H + 7) // 8), 8 * ((W + 7) // 8)), chroma(Cb), chroma(Cr)


def bit_length(v):
    return int(abs(int(v))).bit_length()


def encode(a, tables):
    """uint8 [H, W, 3] and parse_header's result -> (the file's bytes, counters)"""
    H, W, _ = a.shape
    quantised = []
    for plane, tq in zip(planes(a), (0, 1, 1)):
        blocks = plane.reshape(plane.shape[0] // 8, 8, plane.shape[1] // 8, 8).transpose(0, 2, 1, 3) - 128
        quantised.append(quantise(fdct(blocks), tables["quant"][tq]))
    counters = dict(zrl=0, stuffed=0, dummy_right=0, dummy_bottom=0)
    codes = []                                                                  # (value, bits)
    prediction = [0, 0, 0]
    for my in range((H + 15) // 16):
        for mx in range((W + 15) // 16):
            last_dc = 0                                                         # DC of the block before this one inside the MCU
            for ci, (hs, vs) in enumerate(((2, 2), (1, 1), (1, 1))):
                dc_table, ac_table = tables["huff"][0x00 | min(ci, 1)], tables["huff"][0x10 | min(ci, 1)]
                hib, wib = quantised[ci].shape[:2]
                for by in range(vs):
                    before_row = last_dc
                    for bx in range(hs):
                        y, x = my * vs + by, mx * hs + bx
                        if y < hib and x < wib:
                            natural = quantised[ci][y, x].reshape(64)
                            z = [int(natural[ZIGZAG[k]]) for k in range(64)]
                        elif y < hib:                                           # beyond the right edge: the DC of the block just before it
                            z = [last_dc] + [0] * 63
                            counters["dummy_right"] += 1
                        else:                                                   # below the bottom edge: the DC before this row's first block
                            z = [before_row] + [0] * 63
                            counters["dummy_bottom"] += 1
                        last_dc = z[0]
                        diff = z[0] - prediction[ci]
                        prediction[ci] = z[0]
                        n = bit_length(diff)
                        codes.append(dc_table[n])
                        if n:
                            codes.append(((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
                        run = 0
                        for k in range(1, 64):
                            if z[k] == 0:
                                run += 1
                                continue
                            while run > 15:
                                codes.append(ac_table[0xF0])
                                counters["zrl"] += 1
                                run -= 16
                            n = bit_length(z[k])
                            codes.append(ac_table[(run << 4) | n])
                            codes.append(((z[k] if z[k] >= 0 else z[k] - 1) & ((1 << n) - 1), n))
                            run = 0
                        if run:
                            codes.append(ac_table[0x00])
    # bits MSB first, a zero byte behind every FF, the last byte filled with one-bits
    scan, acc, nbits = bytearray(), 0, 0

    def emit(byte):
        scan.append(byte)
        if byte == 0xFF:
            scan.append(0)
            counters["stuffed"] += 1
    for value, bits in codes:
        acc, nbits = (acc << bits) | value, nbits + bits
        while nbits >= 8:
            emit((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8
        acc &= (1 << nbits) - 1
    if nbits:
        emit(((acc << (8 - nbits)) | ((1 << (8 - nbits)) - 1)) & 0xFF)
    return file_header(tables, H, W) + bytes(scan) + b"\xff\xd9", counters
