"""Writes tests/golden/g19_jpeg_decode.npz: JPEG files Pillow wrote (`Image.fromarray(a).save(f, format="JPEG", quality=q, subsampling=s,
optimize=o)`, Pillow on libjpeg-turbo) for small seeded pictures, and the arrays the same Pillow decoded from them
(`Image.open(f).convert("RGB")`), as recorded where this was run.  `grid()` is the whole size x sampling x quality x content grid the
tests write afresh with the installed Pillow; the fixture holds a fixed subset of it (every size with every sampling and every content,
the qualities in turn), one file with optimised Huffman tables per size, and two grey files.

    python -m tests.golden.make_golden_jpeg_decode
"""
import io
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "g19_jpeg_decode.npz")

SIZES = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 17), (15, 33), (33, 15), (37, 53), (48, 64))      # (h, w)
MORE_SIZES = ((64, 48), (100, 75))          # written afresh only: above the fixture's size limit
SAMPLINGS = (0, 1, 2)                       # Pillow's `subsampling`: 4:4:4, 4:2:2, 4:2:0
QUALITIES = (30, 75, 95, 100)
CONTENTS = ("noise", "ramp", "sat")


def picture(size, content, grey=False):
    """uint8 [h, w, 3] ([h, w] when grey): noise; a smooth ramp with mild noise; saturated noise (every channel 0 or 255)"""
    h, w = size
    rng = np.random.default_rng(zlib.crc32(("jpeg decode %dx%d %s" % (h, w, content)).encode()))
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif content == "ramp":
        ramp = np.stack([(xx * 5 + yy) % 256, (yy * 3) % 256, 255 - (xx + yy * 2) % 256], -1)
        a = np.clip(ramp + rng.integers(-6, 6, ramp.shape), 0, 255).astype(np.uint8)
    elif content == "sat":
        a = (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    else:
        raise ValueError(content)
    return a[:, :, 0].copy() if grey else a


def photo(h, w, seed):
    """a picture-like frame: smooth shading, a few flat shapes, mild sensor noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([90 + 100 * yy / h + 20 * np.sin(xx / 37), 110 + 60 * yy / h + 25 * np.cos(xx / 21), 160 - 70 * yy / h + 15 * np.sin((xx + yy) / 15)], -1)
    for _ in range(8):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(5, 40)
        inside = (yy - cy) ** 2 + ((xx - cx) / 2) ** 2 < r * r
        img[inside] = img[inside] * 0.4 + rng.uniform(0, 255, 3) * 0.6
    return np.clip(img + rng.normal(0, 2.5, img.shape), 0, 255).astype(np.uint8)


def write(a, quality, subsampling=None, optimize=False):
    from PIL import Image
    buf = io.BytesIO()
    extra = {} if subsampling is None else {"subsampling": subsampling}
    Image.fromarray(a).save(buf, format="JPEG", quality=quality, optimize=optimize, **extra)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def grid(sizes=SIZES + MORE_SIZES):
    """(name, size, content, quality, subsampling) of the whole grid"""
    for size in sizes:
        for s in SAMPLINGS:
            for q in QUALITIES:
                for c in CONTENTS:
                    yield "%dx%d_s%d_q%d_%s" % (size[0], size[1], s, q, c), size, c, q, s


def cases():
    """(name, picture, quality, subsampling or None, optimize) of the fixture's cases"""
    n = 0
    for size in SIZES:
        for s in SAMPLINGS:
            for j, c in enumerate(CONTENTS):
                q = QUALITIES[(n + j) % 4]
                yield "%dx%d_s%d_q%d_%s" % (size[0], size[1], s, q, c), picture(size, c), q, s, False
            n += 1
    for i, size in enumerate(SIZES):
        yield "%dx%d_s%d_q75_noise_opt" % (size[0], size[1], i % 3), picture(size, "noise"), 75, i % 3, True
    yield "37x53_grey_q90_noise", picture((37, 53), "noise", grey=True), 90, None, False
    yield "8x8_grey_q75_ramp", picture((8, 8), "ramp", grey=True), 75, None, False


def load():
    """{name: (file bytes, uint8 [h, w, 3] Pillow decoded)}"""
    with np.load(PATH) as z:
        return {name[5:]: (z[name].tobytes(), z["rgb_" + name[5:]]) for name in z.files if name.startswith("file_")}


def main():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "record the fixture with a Pillow built on libjpeg-turbo"
    out = {}
    for name, a, q, s, opt in cases():
        data = write(a, q, s, opt)
        out["file_" + name] = np.frombuffer(data, dtype=np.uint8)
        out["rgb_" + name] = pillow_decode(data)
    np.savez_compressed(PATH, **out)
    print("wrote %s: %d cases, %d bytes on disk" % (PATH, len(out) // 2, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
