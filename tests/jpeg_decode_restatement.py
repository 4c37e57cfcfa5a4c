"""NumPy restatement of the baseline JPEG decoder (csrc/jpeg_decode.hip, footprints_amd.ops.jpeg_parse): marker parser, serial Huffman
decode, dequantisation, libjpeg's jidctint, fancy upsampling and the integer YCbCr -> RGB conversion -- what
`PIL.Image.open(f).convert("RGB")` returns for the files the parser accepts, byte for byte -- and a model of the subsequence scheme that
says how many launches and hops a file needs to settle.  Written from the JPEG standard and libjpeg's documented arithmetic; shares no
code with the package."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
GROUP = 64              # subsequences per workgroup of the synchronisation kernel


class Host(Exception):
    """the file is not one the device decodes"""


def _parse(data):
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Host("no SOI")
    quant, huff, frame, jfif, i = {}, {}, None, False, 2
    while True:
        if i + 4 > len(data):
            raise Host("header cut")
        if data[i] != 0xFF:
            raise Host("marker expected")
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        n = (data[i + 2] << 8) | data[i + 3]
        if n < 2 or i + 2 + n > len(data):
            raise Host("bad segment length")
        body = data[i + 4:i + 2 + n]
        if m == 0xE0 and n >= 16 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe":
            raise Host("Adobe marker")
        elif m == 0xDB:
            p = 0
            while p < len(body):
                if body[p] >> 4 or (body[p] & 15) > 3 or p + 65 > len(body):
                    raise Host("quantisation table")
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = np.frombuffer(body[p + 1:p + 65], np.uint8)
                quant[body[p] & 15] = nat
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body) or (body[p] >> 4) > 1 or (body[p] & 15) > 1:
                    raise Host("Huffman table")
                counts = list(body[p + 1:p + 17])
                if sum(counts) > 256 or p + 17 + sum(counts) > len(body):
                    raise Host("Huffman table")
                values = list(body[p + 17:p + 17 + sum(counts)])
                code = 0
                for length in range(1, 17):
                    code = (code + counts[length - 1]) << 1
                    if code > (1 << (length + 1)):
                        raise Host("Huffman table")
                if (body[p] >> 4) == 0 and any(v > 15 for v in values):
                    raise Host("Huffman table")
                huff[(body[p] >> 4, body[p] & 15)] = (counts, values)
                p += 17 + len(values)
        elif m == 0xC0:
            if frame is not None or len(body) < 6 or body[0] != 8 or len(body) != 6 + 3 * body[5]:
                raise Host("frame header")
            frame = dict(h=(body[1] << 8) | body[2], w=(body[3] << 8) | body[4],
                         comps=[(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])])
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF, 0xDD, 0xDC):
            raise Host("not baseline without restarts")
        elif m == 0xDA:
            break
        elif m in (0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or m == 0x01:
            raise Host("marker out of place")
        i += 2 + n
    if frame is None or frame["h"] < 1 or frame["w"] < 1:
        raise Host("no frame")
    comps = frame["comps"]
    if len(comps) not in (1, 3) or len(body) != 4 + 2 * len(comps) or body[0] != len(comps):
        raise Host("components")
    if bytes(body[1 + 2 * len(comps):]) != b"\x00\x3f\x00":
        raise Host("scan parameters")
    td, ta = [], []
    for c, comp in enumerate(comps):
        if body[1 + 2 * c] != comp[0]:
            raise Host("scan order")
        td.append(body[2 + 2 * c] >> 4)
        ta.append(body[2 + 2 * c] & 15)
        if (0, td[-1]) not in huff or (1, ta[-1]) not in huff or comp[3] not in quant:
            raise Host("missing table")
    if len(comps) == 1:
        if comps[0][1:3] != (1, 1):
            raise Host("sampling")
        hs = vs = 1
    else:
        if not jfif and [c[0] for c in comps] != [1, 2, 3]:
            raise Host("colour space")
        hs, vs = comps[0][1:3]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
            raise Host("sampling")
    start = i + 2 + n
    a = np.frombuffer(data, np.uint8)[start:]
    marks = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0))
    if marks.size == 0 or a[marks[0] + 1] != 0xD9 or marks[0] == 0:
        raise Host("scan does not end in EOI")
    return dict(h=frame["h"], w=frame["w"], ncomp=len(comps), hs=hs, vs=vs, tq=[c[3] for c in comps], td=td, ta=ta, quant=quant, huff=huff,
                scan_offset=start, scan_bytes=int(marks[0]))


def parse(data):
    """-> dict(device=True, ...) or dict(device=False, reason=...)"""
    try:
        info = _parse(bytes(data))
    except Host as e:
        return dict(device=False, reason=str(e))
    info["device"] = True
    return info


def _look16(counts, values):
    """16-bit look-up of a canonical Huffman table: length << 8 | symbol, 0 where no code starts"""
    t = np.zeros(65536, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            t[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | values[k]
            code += 1
            k += 1
        code <<= 1
    return t


class Stream:
    """the scan with the stuffed zero bytes removed: win[p] = the 32 bits at bit p; one-bits beyond the end"""

    def __init__(self, info, data):
        raw = np.frombuffer(data, np.uint8)[info["scan_offset"]:info["scan_offset"] + info["scan_bytes"]]
        keep = np.ones(raw.size, bool)
        keep[1:] = ~((raw[1:] == 0) & (raw[:-1] == 0xFF))
        b = np.concatenate([raw[keep], np.full(8, 255, np.uint8)]).astype(np.uint64)
        n = b.size - 8
        u = np.zeros(n + 1, np.uint64)
        for j in range(8):
            u |= b[j:j + n + 1] << np.uint64(56 - 8 * j)
        self.total = 8 * n
        win = np.empty((n + 1, 8), np.uint64)
        for o in range(8):
            win[:, o] = (u >> np.uint64(32 - o)) & np.uint64(0xFFFFFFFF)
        self.win = win.reshape(-1)[:self.total + 1].astype(np.int64).tolist()
        self.nb = 1 if info["ncomp"] == 1 else info["hs"] * info["vs"] + 2
        nluma = self.nb - 2 if info["ncomp"] == 3 else 1
        self.comp = [0 if j < nluma else j - nluma + 1 for j in range(self.nb)]
        self.dc = [_look16(*info["huff"][(0, t)]).tolist() for t in info["td"]]
        self.ac = [_look16(*info["huff"][(1, t)]).tolist() for t in info["ta"]]

    def peek(self, pos):
        return self.win[pos] if pos <= self.total else 0xFFFFFFFF

    def run(self, state, end, coefs=None, first=0, strict=False, marks=None):
        """decode from `state` = (bit, block within the MCU, zigzag index) until the bit position reaches `end`
        -> (exit state, blocks completed); a symbol that would need bits beyond the scan ends the run"""
        pos, blk, k = state
        count = 0
        while pos < end:
            if marks is not None:
                marks.add((pos, blk, k))
            c = self.comp[blk]
            p = self.peek(pos)
            e = (self.dc[c] if k == 0 else self.ac[c])[p >> 16]
            if e == 0:
                if strict:
                    raise ValueError("code no table has")
                pos += 1
                continue
            length, sym = e >> 8, e & 255
            r, s = (0, sym & 15) if k == 0 else (sym >> 4, sym & 15)
            if pos + length + s > self.total:
                break
            v = 0
            if s:
                v = (p >> (32 - length - s)) & ((1 << s) - 1)
                if v < (1 << (s - 1)):
                    v -= (1 << s) - 1
            if k == 0:
                at, k = 0, 1
            elif s == 0:
                at, k = -1, (k + 16 if r == 15 else 64)
                if k > 64 and strict:
                    raise ValueError("zigzag index past 63")
            else:
                k += r
                if k > 63:
                    if strict:
                        raise ValueError("zigzag index past 63")
                    at, k = -1, 64
                else:
                    at, k = int(ZIGZAG[k]), k + 1
            if coefs is not None and at >= 0 and first + count < coefs.shape[0]:
                coefs[first + count, at] = v
            pos += length + s
            if k >= 64:
                k, blk, count = 0, (blk + 1) % self.nb, count + 1
        return (pos, blk, k), count


def geometry(info):
    hs, vs = info["hs"], info["vs"]
    if info["ncomp"] == 1:
        mx, my = (info["w"] + 7) // 8, (info["h"] + 7) // 8
    else:
        mx, my = -(-info["w"] // (8 * hs)), -(-info["h"] // (8 * vs))
    return mx, my, mx * my * (1 if info["ncomp"] == 1 else hs * vs + 2)


def serial_coefficients(info, data, marks=None):
    """[blocks][64] in natural order, scan order of the blocks, the DC term still a difference"""
    st = Stream(info, data)
    nblocks = geometry(info)[2]
    coefs = np.zeros((nblocks, 64), np.int64)
    state, total = (0, 0, 0), 0
    while total < nblocks:
        # one block at a time: the run stops at the first position at or past `end`
        before = state
        state, n = st.run(state, state[0] + 1, coefs, total, strict=True, marks=marks)
        if state == before:
            raise ValueError("scan too short")
        total += n
    return coefs


def _idct_pass(d, shift):
    """jidctint's 8-point pass over the first axis of d [8, ...]"""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(t10 + t3 + r) >> shift, (t11 + t2 + r) >> shift, (t12 + t1 + r) >> shift, (t13 + t0 + r) >> shift,
                     (t13 - t0 + r) >> shift, (t12 - t1 + r) >> shift, (t11 - t2 + r) >> shift, (t10 - t3 + r) >> shift])


def back_half(info, coefs):
    """DC prefix sums, dequantisation, IDCT, fancy upsampling, colour conversion -> uint8 [h, w, 3]"""
    h, w, hs, vs, ncomp = info["h"], info["w"], info["hs"], info["vs"], info["ncomp"]
    mx, my, nblocks = geometry(info)
    nb = nblocks // (mx * my)
    planes = []
    for c in range(ncomp):
        js = list(range(nb - 2)) if (c == 0 and ncomp == 3) else [nb - 3 + c if ncomp == 3 else 0]
        idx = (np.arange(mx * my)[:, None] * nb + np.array(js)[None, :]).reshape(-1)
        blk = coefs[idx].copy()
        blk[:, 0] = np.cumsum(blk[:, 0])
        blk = (blk * info["quant"][info["tq"][c]][None, :]).reshape(-1, 8, 8)
        cols = _idct_pass(blk.transpose(1, 2, 0), 11)                        # [row][col][block]
        rows = _idct_pass(cols.transpose(1, 0, 2), 18)                       # [col][row][block]
        pix = np.clip(rows.transpose(2, 1, 0) + 128, 0, 255)                # [block][row][col]
        ch, cv = (hs, vs) if (c == 0 and ncomp == 3) else (1, 1)
        plane = np.zeros((my * cv * 8, mx * ch * 8), np.int64)
        for n_, b in enumerate(idx):
            m, j = divmod(int(b), nb)
            bx = (m % mx) * ch + (j % ch if ch * cv > 1 else 0)
            by = (m // mx) * cv + (j // ch if ch * cv > 1 else 0)
            plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = pix[n_]
        planes.append(plane)
    if ncomp == 1:
        return np.repeat(planes[0][:h, :w, None], 3, axis=2).astype(np.uint8)
    Y = planes[0][:h, :w]
    ups = []
    for p in planes[1:]:
        cw, chh = -(-w // hs), -(-h // vs)
        p = p[:chh, :cw]
        if vs == 2:
            above, below = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
            rows = np.empty((2 * chh, cw), np.int64)
            rows[0::2], rows[1::2] = 3 * p + above, 3 * p + below
            left, right = np.hstack([rows[:, :1], rows[:, :-1]]), np.hstack([rows[:, 1:], rows[:, -1:]])
            out = np.empty((2 * chh, 2 * cw), np.int64)
            out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
            p = out
        elif hs == 2:
            left, right = np.hstack([p[:, :1], p[:, :-1]]), np.hstack([p[:, 1:], p[:, -1:]])
            out = np.empty((chh, 2 * cw), np.int64)
            out[:, 0::2], out[:, 1::2] = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
            p = out
        ups.append(p[:h, :w])
    cb, cr = ups[0] - 128, ups[1] - 128
    fix = lambda x: int(x * 65536 + 0.5)
    R = Y + ((fix(1.402) * cr + 32768) >> 16)
    B = Y + ((fix(1.772) * cb + 32768) >> 16)
    G = Y + ((-fix(0.34414) * cb - fix(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    """Image.open(data).convert("RGB") of an accepted file"""
    info = parse(data)
    if not info["device"]:
        raise Host(info["reason"])
    return back_half(info, serial_coefficients(info, data))


def model(data, subseq_bits, group=GROUP, max_launches=1 << 20):
    """the subsequence scheme of the device: -> dict(launches = launches until one changes nothing (the settling one included),
    hops = the largest number of hops a workgroup looped in one launch, entries = the settled entry states, nsub)"""
    info = parse(data)
    st = Stream(info, data)
    nsub = max(1, -(-st.total // subseq_bits))
    entry = [(g * subseq_bits, 0, 0) for g in range(nsub + 1)]
    done, exits = [None] * nsub, [None] * nsub
    launches, hops = 0, 0
    while launches < max_launches:
        launches += 1
        changed = False
        old = list(entry)
        for g0 in range(0, nsub, group):
            ids = range(g0, min(g0 + group, nsub))
            local = {g: old[g] for g in ids}
            local[ids[-1] + 1] = old[ids[-1] + 1]
            settled = False
            for it in range(group + 1):
                cur = dict(local)
                moved = False
                for g in ids:
                    if done[g] != cur[g]:
                        exits[g], _ = st.run(cur[g], min((g + 1) * subseq_bits, st.total))
                        done[g] = cur[g]
                    if local[g + 1] != exits[g]:
                        local[g + 1] = exits[g]
                        moved = True
                hops = max(hops, it + 1)
                if not moved:
                    settled = True
                    break
            for g in ids[1:]:
                entry[g] = local[g]
            if ids[-1] + 1 < nsub and local[ids[-1] + 1] != old[ids[-1] + 1]:
                entry[ids[-1] + 1] = local[ids[-1] + 1]
                changed = True
            if not settled:
                changed = True
        if not changed:
            break
    return dict(launches=launches, hops=hops, entries=entry[:nsub], nsub=nsub)
