"""Inputs of the reader fixture (tests/golden/g14_reader.npz) and of the reader tests, as pure functions of their arguments (an integer
hash, no random generator whose stream could change between library versions)."""
import numpy as np

# (name, source (h, w), target (H, W), channels): the small resize cases whose Pillow output the fixture holds whole
SMALL_CASES = [("down", (37, 53), (16, 24), 3), ("down_L", (37, 53), (16, 24), 1), ("up", (16, 24), (37, 53), 3), ("tiny", (7, 5), (3, 2), 3),
               ("ragged", (37, 53), (17, 23), 3)]
# one pass skipped each: the fixture holds a digest of the output
SKIP_CASES = [("skip_v", (192, 53), (192, 24), 3), ("skip_h", (37, 640), (16, 640), 3)]
HALF_CASE = ("half", (37, 53), (16, 24), 3)
KITTI_SIZES = [(375, 1242), (370, 1224), (376, 1241)]
KITTI_TARGET = (192, 640)
MASK_SIZES = [(20, 30), (24, 36)]


def image(h, w, c, seed):
    """uint8 [h, w, c] ([h, w] when c == 1 and squeeze): hashed noise over a smooth ramp, with saturated patches so that the filters overshoot"""
    y, x, ch = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(c, dtype=np.uint64), indexing="ij")
    v = (y * np.uint64(7919) + x * np.uint64(104729) + ch * np.uint64(1299709) + np.uint64(seed) * np.uint64(15485863)) * np.uint64(2654435761)
    noise = ((v >> np.uint64(13)) & np.uint64(255)).astype(np.int64)
    ramp = ((x * np.uint64(255)) // np.uint64(max(w - 1, 1)) + (y * np.uint64(255)) // np.uint64(max(h - 1, 1))).astype(np.int64) // 2
    img = (noise + ramp) // 2
    block = (((y // np.uint64(5)) + (x // np.uint64(7)) + np.uint64(seed)) % np.uint64(4)).astype(np.int64)
    img = np.where(block == 0, 0, np.where(block == 1, 255, img))
    return img.astype(np.uint8)


def random_mask(h, w, density_percent, seed):
    """float64 [h, w] of zeros and ones"""
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    v = (y * np.uint64(104729) + x * np.uint64(7919) + np.uint64(seed) * np.uint64(15485863) + np.uint64(12345)) * np.uint64(2654435761)
    v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519)
    return (((v >> np.uint64(16)) % np.uint64(100)) < np.uint64(density_percent)).astype(np.float64)


def kitti_masks():
    """name -> float64 [192, 640]: 10 % density (every component far below the limit of 1228.8 pixels), and the same with a solid 40 x 40
    block and a 1200-pixel bar laid over it (the block and what touches it go, the bar stays unless noise pushes it past the limit)"""
    H, W = KITTI_TARGET
    m = random_mask(H, W, 10, 7)
    b = m.copy()
    b[60:100, 300:340] = 1
    b[150:152, 10:610] = 1
    return {"random10": m, "random10_block": b}
