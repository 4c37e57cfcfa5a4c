"""Writes tests/golden/g18_jpeg.npz: Pillow's JPEG bytes (`Image.fromarray(a).save(f, format="JPEG", quality=q)`, Pillow on
libjpeg-turbo) of small seeded pictures -- every size x content x quality of the lists below -- as recorded where this was run.  The
pictures themselves are not stored: `picture(size, content)` rebuilds them from the case's seed.

    python -m tests.golden.make_golden_jpeg
"""
import io
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "g18_jpeg.npz")

QUALITIES = (30, 75, 95, 100)
CONTENTS = ("noise", "ramp", "flat", "bw")
SIZES = ((1, 1), (8, 8), (9, 25), (16, 17), (17, 16), (16, 24), (23, 1), (24, 40), (33, 47), (37, 50), (41, 57), (75, 122))      # (h, w)


def seed_of(size, content):
    return zlib.crc32(("jpeg %dx%d %s" % (size[0], size[1], content)).encode())


def picture(size, content):
    """uint8 [h, w, 3]: noise; a smooth ramp with noise on it; two flat colours split along a slanted line; black / white noise"""
    h, w = size
    rng = np.random.default_rng(seed_of(size, content))
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "ramp":
        ramp = np.stack([(xx * 2 + yy) % 256, (yy * 3) % 256, (xx + yy * 2) % 256], -1)
        return np.clip(ramp + rng.integers(-20, 20, ramp.shape), 0, 255).astype(np.uint8)
    if content == "flat":
        colours = rng.integers(0, 256, (2, 3), dtype=np.uint8)
        return colours[((xx + 2 * yy) * 3 > w + 2 * h).astype(np.int64)]
    if content == "bw":
        return np.repeat(rng.integers(0, 2, (h, w, 1), dtype=np.uint8) * 255, 3, axis=2)
    raise ValueError(content)


def cases():
    """(name, size, content, quality) of every case"""
    for size in SIZES:
        for content in CONTENTS:
            for quality in QUALITIES:
                yield "%dx%d_%s_q%d" % (size[0], size[1], content, quality), size, content, quality


def load():
    """{name: bytes}"""
    with np.load(PATH) as z:
        return {name: z[name].tobytes() for name in z.files}


def main():
    from PIL import Image, features
    assert features.check_feature("libjpeg_turbo"), "record the fixture with a Pillow built on libjpeg-turbo"
    out = {}
    for name, size, content, quality in cases():
        buf = io.BytesIO()
        Image.fromarray(picture(size, content)).save(buf, format="JPEG", quality=quality)
        out[name] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    np.savez_compressed(PATH, **out)
    print("wrote %s: %d cases, %d bytes of files" % (PATH, len(out), sum(len(v) for v in out.values())))


if __name__ == "__main__":
    main()
