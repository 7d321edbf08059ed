"""Shapes, images and parameter tables of the tiled augmentation's tests (csrc/spv_augment_tiled.hip), shared by tests/test_augment_tiled.py
(CPU: the restatement alone must stay inside the left-out caps on these very tables) and tests/test_gpu_augment_tiled.py (GPU: the kernels
against the restatement tests/augment_ref.py).  A plain helper module; every table is a pure function of its case name.

Shapes: the smallest at which tiling (16 x 64 output tiles, 4096-pixel chunks of the contrast mean) can go wrong, and the motivating one.
Batches: rotation cases draw at least 16 angles (a single image's rotation ties reach 1.9 % of its pixels, 17 % once a blur dilates
them; a batch's mean is 0.4 % / 3.3 %); at 224 x 224 the other cases keep to batch 4 (the restatement takes 0.1 s for it)."""
import numpy as np

import augment_ref as R

MEAN = (0.5071, 0.4867, 0.4408)
STD = (0.2675, 0.2565, 0.2761)

LARGE = [(3, 64, 64),     # first size the LDS kernel refuses; several full tiles
         (3, 70, 45),     # partial tiles both ways; H W % 4 != 0: scalar stores
         (1, 33, 97),     # one channel; a one-row last tile row, a second tile column of 33 (the LDS kernel takes it too)
         (3, 224, 224)]   # the motivating size
BOTH = [(3, 32, 32), (1, 28, 28)]   # the shapes both kernels take
SHAPES = LARGE + BOTH
ALLOWANCE_CAP = 1.4e-3   # a tenth of one 8-bit step of the normalised image, 1 / (255 * 0.2761) / 10
CAP_TIES, CAP_DILATED = 0.01, 0.05

ALL_OPS_ALONE = ["flip", "brightness", "contrast", "saturation", "hue", "gray", "rotate", "blur", "erase"]
ALL_OPS = ("flip", "brightness", "contrast", "saturation", "hue", "order", "gray", "rotate", "blur", "erase")


def sid(shape):
    return "x".join(map(str, shape))


def big(shape):
    return shape[1] * shape[2] > 128 * 128


def image_set(n, shape, seed):
    """uint8 NHWC; every other image smooth (low-saturation pixels, flat areas, black and white patches), the rest noise"""
    C, H, W = shape
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(0, n, 2):
        s = 96.0 / max(H, W)
        base = rng.uniform(0, 220, size=C) + rng.uniform(-s, s, size=C) * xx[..., None] + rng.uniform(-s, s) * yy[..., None]
        imgs[k] = np.clip(base + rng.uniform(0, 20) * rng.standard_normal((H, W, C)), 0, 255).astype(np.uint8)
    return imgs


def random_table(batch, shape, rng, ops):
    """identity table with the named ops switched on at random values inside the reference recipe's ranges"""
    C, H, W = shape
    p = R.identity_params(batch)
    u = lambda lo, hi: rng.uniform(lo, hi, size=batch).astype(np.float32)
    if "flip" in ops:
        p[:, R.FLIP] = rng.integers(0, 2, size=batch)
    if "brightness" in ops:
        p[:, R.BRIGHT] = u(0.6, 1.4)
    if "contrast" in ops:
        p[:, R.CONTRAST] = u(0.6, 1.4)
    if "saturation" in ops:
        p[:, R.SAT] = u(0.6, 1.4)
    if "hue" in ops:
        p[:, R.HUE] = u(-0.1, 0.1)
    if "order" in ops:
        p[:, R.ORDER] = (np.arange(batch) + rng.integers(0, 24)) % 24
    if "gray" in ops:
        p[:, R.GRAY] = rng.integers(0, 2, size=batch)
    if "rotate" in ops:
        p[:, R.ANGLE] = u(-30, 30)
    if "blur" in ops:
        p[:, R.BLUR] = 1
        p[:, R.SIGMA] = u(0.1, 2.0)
    if "erase" in ops:
        h, w = rng.integers(1, H, size=batch), rng.integers(1, W, size=batch)
        p[:, R.ERASE_H], p[:, R.ERASE_W] = h, w
        p[:, R.ERASE_I], p[:, R.ERASE_J] = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
    return p


def seed_of(*parts):
    import zlib
    return zlib.crc32(repr(parts).encode())


# ---------------------------------------------------------------- the cases: (images, index or None, params)
def case_identity(shape):
    batch = 4 if big(shape) else 8
    return image_set(batch, shape, 1), None, R.identity_params(batch)


def case_op(shape, op):
    rng = np.random.default_rng(seed_of("op", shape, op))
    batch = 16 if (op == "rotate" or not big(shape)) else 4
    n = 8
    imgs = image_set(n, shape, 2)
    if op == "blur":
        imgs = np.random.default_rng(3).integers(0, 256, size=imgs.shape, dtype=np.uint8)   # noise: every seam shows
    index = rng.integers(0, n, size=batch)
    params = random_table(batch, shape, rng, (op,))
    if op in ("flip", "gray"):
        params[:2, R.FLIP if op == "flip" else R.GRAY] = (0, 1)
    return imgs, index, params


def case_orders(shape):
    """each of the 24 orders on the same image with the same four factors"""
    rng = np.random.default_rng(24)
    imgs = image_set(2, shape, 3)
    params = random_table(24, shape, rng, ("brightness", "contrast", "saturation", "hue"))
    params[:, R.BRIGHT:R.HUE + 1] = params[0, R.BRIGHT:R.HUE + 1]
    params[:, R.ORDER] = np.arange(24)
    return imgs, np.zeros(24, np.int64), params


def chain_batches(shape):
    """1, 7 and 64; at 224 x 224 1, 4 (that shape's batch) and 16 (the fewest angles a rotation case draws)"""
    return (1, 4, 16) if big(shape) else (1, 7, 64)


FIXED_ANGLE = 17.0   # the batch-1 chain's rotation: tests/test_augment_tiled.py holds its dilated ties under the cap at every shape


def case_chain(shape, batch, with_index):
    rng = np.random.default_rng(seed_of("chain", shape, batch, with_index))
    n = max(batch, 8)
    imgs = image_set(n, shape, 4)
    index = rng.integers(0, n, size=batch) if with_index else None
    if with_index and batch > 1:
        index[-1] = index[0]   # a repeat, whatever the draw
    params = random_table(batch, shape, rng, ALL_OPS)
    params[:, R.BLUR] = np.arange(batch) % 2 if batch > 1 else 1   # half the images blur; the single one does
    if batch == 1:
        params[:, R.ANGLE] = FIXED_ANGLE
    params[rng.integers(0, 2, size=batch).astype(bool), R.ERASE_H] = 0   # no rectangle
    return imgs, index, params


def all_cases():
    """(name, shape, builder) of every table the GPU tests hold to the restatement"""
    for shape in SHAPES:
        yield f"identity-{sid(shape)}", shape, (lambda s=shape: case_identity(s))
        for op in ALL_OPS_ALONE:
            yield f"{op}-{sid(shape)}", shape, (lambda s=shape, o=op: case_op(s, o))
        yield f"orders-{sid(shape)}", shape, (lambda s=shape: case_orders(s))
        for batch in chain_batches(shape):
            for with_index in (False, True):
                yield (f"chain-{sid(shape)}-{batch}-{'index' if with_index else 'rows'}", shape,
                       (lambda s=shape, b=batch, w=with_index: case_chain(s, b, w)))


def left_out(params, shape):
    """(B, H, W) bool: what the restatement leaves out for this table -- rotation ties, dilated where the sample blurs -- without
    running the chain"""
    C, H, W = shape
    blank = np.zeros((1, H, W))
    masks = []
    for p in np.asarray(params):
        _, ties = R.rotate(blank, float(np.float64(p[R.ANGLE])))
        masks.append(R.dilate3(ties) if p[R.BLUR] != 0 else ties)
    return np.stack(masks)


def cap_of(params):
    """the share of pixels a comparison on this table may leave out"""
    if not (params[:, R.ANGLE] != 0).any():
        return 0.0
    return CAP_DILATED if (params[:, R.BLUR] != 0).any() else CAP_TIES
