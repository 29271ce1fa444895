"""Host restatement of the device RandAugment ops, of the Random Erasing draws and of the normal erase fill, plus a
Pillow reference builder.  A helper, not a test.

Every op of torchvision's RandAugment on PIL images is restated in numpy with the arithmetic Pillow runs in C (16.16
fixed point for the affine ops, fp32 for the blends and the 3x3 filter, integers and one fp64 LUT for the rest);
tests/test_augment_host.py checks the restatements against Pillow bit for bit, tests/test_gpu_augment.py checks
favit_randaugment against Pillow itself.  numpy and Pillow only; runs on the CPU."""
import math

import numpy as np

from _dropout_ref import rand_u32

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
       "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")


def magnitude(op, bin_, bins, S, sign=0):
    """The magnitude value torchvision's RandAugment gives `op` at bin `bin_` of `bins` for an S x S image (None for the
    ops without one); signed ops are negated when sign == 1."""
    if op in ("Identity", "AutoContrast", "Equalize"):
        return None
    if op in ("ShearX", "ShearY"):
        m = float(np.linspace(0.0, 0.3, bins)[bin_])
    elif op in ("TranslateX", "TranslateY"):
        m = float(np.linspace(0.0, 150.0 / 331.0 * S, bins)[bin_])
    elif op == "Rotate":
        m = float(np.linspace(0.0, 30.0, bins)[bin_])
    elif op in ("Brightness", "Color", "Contrast", "Sharpness"):
        m = float(np.linspace(0.0, 0.9, bins)[bin_])
    elif op == "Posterize":
        return int((8 - np.round(np.arange(bins) / ((bins - 1) / 4)))[bin_])
    elif op == "Solarize":
        return float(np.linspace(255.0, 0.0, bins)[bin_])
    else:
        raise ValueError(op)
    return -m if (sign and op in SIGNED) else m


# ---------------------------------------------------------------------------------------------------------------------
# Pillow reference
def pil_apply(im, op, m, fill=(0, 0, 0)):
    """`op` with magnitude value m on an RGB PIL.Image, exactly as the issue's table (torchvision on PIL images)."""
    from PIL import Image, ImageEnhance, ImageOps
    fill = tuple(int(v) for v in fill)
    A, N = Image.Transform.AFFINE, Image.Resampling.NEAREST
    if op == "Identity":
        return im
    if op == "ShearX":
        return im.transform(im.size, A, (1, m, 0, 0, 1, 0), N, fillcolor=fill)
    if op == "ShearY":
        return im.transform(im.size, A, (1, 0, 0, m, 1, 0), N, fillcolor=fill)
    if op == "TranslateX":
        return im.transform(im.size, A, (1, 0, -int(m), 0, 1, 0), N, fillcolor=fill)
    if op == "TranslateY":
        return im.transform(im.size, A, (1, 0, 0, 0, 1, -int(m)), N, fillcolor=fill)
    if op == "Rotate":
        return im.rotate(m, N, fillcolor=fill)
    if op in ("Brightness", "Color", "Contrast", "Sharpness"):
        return getattr(ImageEnhance, op)(im).enhance(1 + m)
    if op == "Posterize":
        return ImageOps.posterize(im, int(m))
    if op == "Solarize":
        return ImageOps.solarize(im, m)
    if op == "AutoContrast":
        return ImageOps.autocontrast(im)
    if op == "Equalize":
        return ImageOps.equalize(im)
    raise ValueError(op)


def pil_chain(img, chain, fill=(0, 0, 0)):
    """img uint8 [S,S,3] through the (op, m) pairs of `chain`, in order, by Pillow -> uint8 [S,S,3]."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    for op, m in chain:
        im = pil_apply(im, op, m, fill)
    return np.asarray(im).copy()


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements
def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_matrix(angle, w, h):
    """PIL.Image.rotate's matrix (centre of the image, no translation), with its round(..., 15)."""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    mt = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    mt[2] = mt[0] * -cx + mt[1] * -cy + mt[2]
    mt[5] = mt[3] * -cx + mt[4] * -cy + mt[5]
    mt[2] += cx
    mt[5] += cy
    return mt


def affine_fixed(mt):
    """The six 16.16 fixed-point coefficients of Pillow's nearest-neighbour affine transform (half-pixel centre folded
    into a2, a5)."""
    a0, a1, a2, a3, a4, a5 = (float(v) for v in mt)
    return (_fix(a0), _fix(a1), _fix(a2 + a0 * 0.5 + a1 * 0.5), _fix(a3), _fix(a4), _fix(a5 + a3 * 0.5 + a4 * 0.5))


def np_affine(img, mt, fill):
    H, W, _ = img.shape
    a0, a1, a2, a3, a4, a5 = affine_fixed(mt)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    sx = (a2 + a1 * y + a0 * x) >> 16
    sy = (a5 + a4 * y + a3 * x) >> 16
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    out = np.empty_like(img)
    out[:] = np.asarray(fill, dtype=np.uint8)
    out[ok] = img[sy[ok], sx[ok]]
    return out


def np_luma(img):
    i = img.astype(np.int64)
    return ((19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16).astype(np.uint8)


def np_smooth(img):
    """ImageFilter.SMOOTH: (1,1,1,1,5,1,1,1,1)/13 in fp32, accumulator 0.5, the three taps of a row summed left to
    right and each row's sum added to the accumulator (rows y+1, y, y-1), floored and clipped; the border is copied."""
    f = img.astype(np.float32)
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    H, W, _ = img.shape
    out = img.copy()
    if H < 3 or W < 3:
        return out

    def row(r, kc):
        l, c, rr = f[r, 0:W - 2], f[r, 1:W - 1], f[r, 2:W]
        return (l * k1 + c * kc) + rr * k1

    ss = np.full((H - 2, W - 2, img.shape[2]), np.float32(0.5), dtype=np.float32)
    ss = ss + row(slice(2, H), k1)
    ss = ss + row(slice(1, H - 1), k5)
    ss = ss + row(slice(0, H - 2), k1)
    out[1:H - 1, 1:W - 1] = np.where(ss <= 0.0, 0, np.where(ss >= 255.0, 255, np.floor(ss))).astype(np.uint8)
    return out


def np_blend(deg, src, f):
    """ImagingBlend(deg, src, f) in fp32: deg + f * (src - deg), truncated for 0 <= f <= 1, else clipped first."""
    f = np.float32(f)
    d = deg.astype(np.float32)
    v = d + f * (src.astype(np.float32) - d)
    assert v.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return v.astype(np.int32).astype(np.uint8)
    return np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int32))).astype(np.uint8)


def np_equalize(img):
    out = img.copy()
    for c in range(img.shape[2]):
        h = np.bincount(img[..., c].reshape(-1), minlength=256).astype(np.int64)
        nz = np.nonzero(h)[0]
        if len(nz) <= 1:
            continue
        step = (int(h.sum()) - int(h[nz[-1]])) // 255
        if step == 0:
            continue
        n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
        lut = np.minimum(255, n // step).astype(np.uint8)
        out[..., c] = lut[img[..., c]]
    return out


def np_autocontrast(img):
    out = img.copy()
    for c in range(img.shape[2]):
        lo, hi = int(img[..., c].min()), int(img[..., c].max())
        if hi <= lo:
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        lut = np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], dtype=np.uint8)
        out[..., c] = lut[img[..., c]]
    return out


def np_apply(img, op, m, fill=(0, 0, 0)):
    """`op` with magnitude value m on a uint8 [S,S,3] array: the arithmetic the device runs."""
    H, W, _ = img.shape
    if op == "Identity":
        return img.copy()
    if op == "ShearX":
        return np_affine(img, (1, m, 0, 0, 1, 0), fill)
    if op == "ShearY":
        return np_affine(img, (1, 0, 0, m, 1, 0), fill)
    if op == "TranslateX":
        return np_affine(img, (1, 0, -int(m), 0, 1, 0), fill)
    if op == "TranslateY":
        return np_affine(img, (1, 0, 0, 0, 1, -int(m)), fill)
    if op == "Rotate":
        return np_affine(img, rotate_matrix(m, W, H), fill)
    if op == "Brightness":
        return np_blend(np.zeros_like(img), img, 1 + m)
    if op == "Color":
        return np_blend(np.repeat(np_luma(img)[..., None], 3, axis=2), img, 1 + m)
    if op == "Contrast":
        L = np_luma(img).astype(np.int64)
        mean = int(int(L.sum()) / L.size + 0.5)
        return np_blend(np.full_like(img, mean), img, 1 + m)
    if op == "Sharpness":
        return np_blend(np_smooth(img), img, 1 + m)
    if op == "Posterize":
        return img & np.uint8(~(2 ** (8 - int(m)) - 1) & 0xFF)
    if op == "Solarize":
        return np.where(img < m, img, 255 - img).astype(np.uint8)
    if op == "AutoContrast":
        return np_autocontrast(img)
    if op == "Equalize":
        return np_equalize(img)
    raise ValueError(op)


def np_chain(img, chain, fill=(0, 0, 0)):
    for op, m in chain:
        img = np_apply(img, op, m, fill)
    return img


def normalize(u8, mean, std):
    """ToTensor + Normalize with the device transform's own expression: ((float)v / 255.0f - mean) / std in fp32.
    u8 [B,S,S,C] -> fp32 [B,C,S,S]."""
    t = u8.astype(np.float32) / np.float32(255.0)
    t = (t - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    assert t.dtype == np.float32
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# Random Erasing
def erase_draws(rng, B, H, W, p, scale, ratio):
    """torchvision RandomErasing.get_params per image from a numpy RandomState -> int32 [B,4] = (y0, y1, x0, x1); an
    all-zero row means no erase.  (The order of the draws is the one data.RandomErasing uses.)"""
    box = np.zeros((B, 4), dtype=np.int32)
    area = H * W
    lr = (math.log(ratio[0]), math.log(ratio[1]))
    for b in range(B):
        if not rng.rand() < p:
            continue
        for _ in range(10):
            a = area * rng.uniform(scale[0], scale[1])
            r = math.exp(rng.uniform(lr[0], lr[1]))
            h, w = int(round(math.sqrt(a * r))), int(round(math.sqrt(a / r)))
            if not (h < H and w < W):
                continue
            i, j = int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1))
            box[b] = (i, i + h, j, j + w)
            break
    return box


def normal_uniforms(seed, idx):
    """The two uniforms behind element idx of the normal fill, exactly (both are multiples of 2^-24):
    u1 in (0, 1] from draw 2 idx, u2 in [0, 1) from draw 2 idx + 1."""
    idx = np.asarray(idx).astype(np.uint64)
    r1 = rand_u32(seed, idx * np.uint64(2))
    r2 = rand_u32(seed, idx * np.uint64(2) + np.uint64(1))
    u1 = ((r1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (r2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal_fill(seed, idx, dtype=np.float32):
    """Box-Muller value of element idx = ((b*C + c)*H + y)*W + x: sqrt(-2 log u1) * cos(2 pi u2), evaluated in `dtype`
    (fp32: the device's expression with numpy's logf / cosf; fp64: the value both approximate)."""
    u1, u2 = normal_uniforms(seed, idx)
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    two_pi = dtype(6.283185307179586)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    z = r * np.cos(two_pi * u2)
    assert z.dtype == dtype
    return z


def element_index(b, C, H, W):
    """idx of every element of image b of a [B,C,H,W] batch -> uint64 [C,H,W]."""
    return (np.uint64(b) * np.uint64(C * H * W) + np.arange(C * H * W, dtype=np.uint64)).reshape(C, H, W)
