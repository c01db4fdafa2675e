"""NumPy restatement of MultiCUB.create_sample (spair/data.py:59-158 of the reference) given a layout and a sprite bank, for the
two backgrounds create_cub_tfrec selects (solid_fixed, ckb_rot_6 and their unseen forms).  Written from spair/data.py, not from
the kernel: the 192 x 192 board is painted, rotated with the transform of tfa.image.rotate 0.6 (angles_to_projective_transforms +
the bilinear rule of its projective-transform op, zero fill outside) in float64, cropped to its central quarter, and the sprites
are pasted in object order.  TensorFlow Addons cannot be run here, so the rotation is restated from its published source."""
import numpy as np

TRAIN_COLORS_TRIAD = [(195, 135, 255), (193, 255, 135), (255, 165, 135), (81, 197, 255), (255, 229, 81), (255, 81, 139)]   # :52
TEST_COLORS_TRIAD = [(255, 125, 227), (125, 255, 184), (255, 205, 125)]                                                       # :53
TRAIN_COLORS = [(100, 209, 72), (209, 72, 100), (209, 127, 72), (72, 129, 209), (84, 184, 209), (209, 109, 84), (184, 209, 84),
                (109, 84, 209)]                                                                                               # :56
TEST_COLORS = [(222, 222, 102), (100, 100, 219), (219, 100, 219), (100, 219, 100)]                                            # :57
TABLES = {"solid_fixed": TRAIN_COLORS, "unseen_solid_fixed": TEST_COLORS, "ckb_rot_6": TRAIN_COLORS_TRIAD,
          "unseen_ckb_rot_6": TEST_COLORS_TRIAD}


def calculate_intersection(a0, a1, b0, b1):
    """calculateIntersection, :18-29, literally."""
    if a0 >= b0 and a1 <= b1:
        return a1 - a0
    elif a0 < b0 and a1 > b1:
        return b1 - b0
    elif a0 < b0 and a1 > b0:
        return a1 - b0
    elif a1 > b1 and a0 < b1:
        return b1 - a0
    return 0


def calculate_overlap(rand_x, rand_y, drawn_boxes):
    """:31-37"""
    for x, y in drawn_boxes:
        if calculate_intersection(rand_x, rand_x + 14, x, x + 14) * calculate_intersection(rand_y, rand_y + 14, y, y + 14) / 14 ** 2 > 0.15:
            return True
    return False


def checkerboard(colors, size=192, cell=6):
    """:90-103: temp_canvas float32 [size,size,3], cell (i, j) takes colors[(i + j) % 2] / 255."""
    t = np.zeros((size, size, 3), np.float32)
    for i in range(size // cell):
        for j in range(size // cell):
            for ch in range(3):
                t[i * cell:(i + 1) * cell, j * cell:(j + 1) * cell, ch] = colors[(i + j) % 2][ch] / 255.
    return t


def rotate_bilinear(img, angle, region=None):
    """tfa.image.rotate(img, angle, 'BILINEAR'): output (y, x) reads the source point
    xs = cos x - sin y + xo, ys = sin x + cos y + yo, xo = ((W-1) - (cos (W-1) - sin (H-1))) / 2, yo = ((H-1) - (sin (W-1) + cos (H-1))) / 2,
    value = (y1 - ys) ((x1 - xs) v[y0,x0] + (xs - x0) v[y0,x1]) + (ys - y0) ((x1 - xs) v[y1,x0] + (xs - x0) v[y1,x1]), zeros outside.
    Returns (rotated float64 image, in_range bool image: all four taps inside the source).  region = (r0, r1): only output rows and
    columns r0..r1-1 are computed (what central_crop keeps; the rest of the rotated image is never looked at)."""
    H, W = img.shape[:2]
    a = np.float64(np.float32(angle))
    c, s = np.cos(a), np.sin(a)
    xo = ((W - 1) - (c * (W - 1) - s * (H - 1))) / 2.0
    yo = ((H - 1) - (s * (W - 1) + c * (H - 1))) / 2.0
    r0, r1 = region if region is not None else (0, H)
    y, x = np.mgrid[r0:r1, r0:r1].astype(np.float64) if region is not None else np.mgrid[0:H, 0:W].astype(np.float64)
    xs, ys = c * x - s * y + xo, s * x + c * y + yo
    x0, y0 = np.floor(xs), np.floor(ys)
    src = img.astype(np.float64)

    def read(yy, xx):
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        v = src[np.clip(yy, 0, H - 1).astype(np.int64), np.clip(xx, 0, W - 1).astype(np.int64)]
        return np.where(ok[..., None], v, 0.0), ok

    v00, k00 = read(y0, x0)
    v01, k01 = read(y0, x0 + 1)
    v10, k10 = read(y0 + 1, x0)
    v11, k11 = read(y0 + 1, x0 + 1)
    wx1, wy1 = (xs - x0)[..., None], (ys - y0)[..., None]
    out = (1 - wy1) * ((1 - wx1) * v00 + wx1 * v01) + wy1 * ((1 - wx1) * v10 + wx1 * v11)
    return out, k00 & k01 & k10 & k11


def central_crop_quarter(img):
    """tf.image.central_crop(img, 0.25) of a 192-pixel image: rows and columns 72..119."""
    n = img.shape[0]
    start = int((n - n * 0.25) / 2)
    size = n - 2 * start
    return img[start:start + size, start:start + size]


def background(bg, colour, angle):
    """canvas [48,48,3] float32 before the sprites (:70-79, :89-105); colour = indices into the table of bg."""
    table = TABLES[bg]
    if "rot" not in bg:
        canvas = np.zeros((48, 48, 3), np.float32)
        for ch in range(3):
            canvas[:, :, ch] = table[colour[0]][ch] / 255.
        return canvas
    board = checkerboard([table[colour[0]], table[colour[1]]])
    rot, ok = rotate_bilinear(board, angle, region=(72, 120))                    # = central_crop_quarter(rotate_bilinear(board, angle))
    assert ok.all(), "the crop reached the zero fill"                            # 24 sqrt(2) + 1 < 95.5
    return rot.astype(np.float32)


def create_sample(layout, bank, bg):
    """layout: a record with count, row, col, sprite, colour, angle; bank uint8 [N,14,14,3] -> float32 [48,48,3] (:124-158)."""
    canvas = background(bg, layout["colour"], layout["angle"])
    for k in range(int(layout["count"])):
        rand_x, rand_y = int(layout["row"][k]), int(layout["col"][k])
        rand_img = bank[int(layout["sprite"][k])]
        alpha_img = np.where(np.max(rand_img, axis=-1) > 0, 1.0, 0.0)
        rand_img = rand_img / 255.
        alpha_bg = 1.0 - alpha_img
        alpha_img, alpha_bg = alpha_img[:, :, np.newaxis], alpha_bg[:, :, np.newaxis]
        canvas[rand_x:rand_x + 14, rand_y:rand_y + 14] = alpha_img * rand_img + alpha_bg * canvas[rand_x:rand_x + 14, rand_y:rand_y + 14]
    return canvas


def create_dataset(layouts, bank, bg):
    x = np.stack([create_sample(L, bank, bg) for L in layouts]) if len(layouts) else np.zeros((0, 48, 48, 3), np.float32)
    return x, np.asarray([L["count"] for L in layouts], np.float32)
