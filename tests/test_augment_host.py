"""Host side of the device RandAugment / Random Erasing: the numpy restatement of every op (tests/_augment_ref.py: the
arithmetic csrc/augment.hip runs) against Pillow bit for bit, the table rows data.RandAugment builds against the same
restatement, the draws and their checkpoint state, and the loader's state keys.  No GPU."""
import math

import numpy as np
import pytest

import _augment_ref as R

BINS = 31
CASE_BINS = (0, 15, 30)
FILLS = ((0, 0, 0), (128, 3, 250))


@pytest.fixture(scope="module")
def data(favit):
    return favit.data


def _images(S, seed=0, n_noise=5):
    """noise images, one with its levels in a 20-wide band, a constant one (the identity paths of Equalize and
    AutoContrast) and a smooth ramp."""
    rng = np.random.RandomState(seed + S)
    imgs = [rng.randint(0, 256, (S, S, 3)).astype(np.uint8) for _ in range(n_noise)]
    imgs.append((100 + rng.randint(0, 20, (S, S, 3))).astype(np.uint8))
    imgs.append(np.full((S, S, 3), 77, dtype=np.uint8))
    yy, xx = np.mgrid[0:S, 0:S]
    imgs.append(np.stack([(yy * 7) % 256, xx * 255 // S, ((xx + yy) * 4) % 256], axis=2).astype(np.uint8))
    return imgs


@pytest.mark.parametrize("S", [17, 32])
@pytest.mark.parametrize("op", R.OPS)
def test_restatement_matches_pillow(op, S):
    """Every op at bins 0, mid and max with both signs, on noise / low-contrast / constant / ramp images, two fills:
    bit-exact.  (Sharpness runs on all 8 images: its fp32 3x3 filter is the one order-sensitive sum.)"""
    for k, img in enumerate(_images(S)):
        fill = FILLS[k % 2]
        for bin_ in CASE_BINS:
            for sign in (0, 1):
                m = R.magnitude(op, bin_, BINS, S, sign)
                want = R.pil_chain(img, [(op, m)], fill)
                got = R.np_apply(img, op, m, fill)
                assert np.array_equal(got, want), f"{op} bin {bin_} sign {sign} image {k}: {(got != want).sum()} bytes differ"


def test_smooth_filter_matches_pillow_widely():
    """The SMOOTH filter alone (Sharpness's degenerate image) on 24 images of 5 sizes, odd and even."""
    from PIL import Image, ImageFilter
    for S in (3, 5, 17, 32, 41):
        for img in _images(S, seed=7, n_noise=3)[:4] + _images(S, seed=11, n_noise=2)[:2]:
            want = np.asarray(Image.fromarray(img, "RGB").filter(ImageFilter.SMOOTH))
            assert np.array_equal(R.np_smooth(img), want)


def test_chains_match_pillow():
    S = 32
    img = _images(S)[0]
    chains = [[("Rotate", 21.0), ("Equalize", None)], [("ShearX", -0.3), ("Contrast", 0.9)],
              [("Sharpness", 0.9), ("Rotate", -30.0)], [("TranslateY", 9.7), ("AutoContrast", None), ("Color", -0.45)]]
    for ch in chains:
        assert np.array_equal(R.np_chain(img, ch, (9, 200, 31)), R.pil_chain(img, ch, (9, 200, 31)))


# ---------------------------------------------------------------------------------------------------------------------
def _apply_row(img, row):
    """A table row of data.RandAugment, run by the restatement (what the kernel does with it)."""
    op = int(row[0])
    if op == 0:
        return img.copy()
    if op == 1:
        S = img.shape[0]
        a0, a1, a2, a3, a4, a5 = (int(v) for v in row[1:7])
        fill = (int(row[7]) & 255, (int(row[7]) >> 8) & 255, (int(row[7]) >> 16) & 255)
        y, x = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
        sx, sy = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
        ok = (sx >= 0) & (sx < S) & (sy >= 0) & (sy < S)
        out = np.empty_like(img)
        out[:] = np.asarray(fill, dtype=np.uint8)
        out[ok] = img[sy[ok], sx[ok]]
        return out
    if op == 2:
        f = float(np.array([row[2]], dtype=np.int32).view(np.float32)[0])
        kind = int(row[1])
        L = R.np_luma(img)
        deg = [np.zeros_like(img), np.repeat(L[..., None], 3, axis=2),
               np.full_like(img, (2 * int(L.astype(np.int64).sum()) + L.size) // (2 * L.size)), R.np_smooth(img)][kind]
        return R.np_blend(deg, img, f)
    if op == 3:
        return img & np.uint8(row[1])
    if op == 4:
        return np.where(img < int(row[1]), img, 255 - img).astype(np.uint8)
    return R.np_autocontrast(img) if op == 5 else R.np_equalize(img)


@pytest.mark.parametrize("S", [17, 32])
def test_table_rows_match_pillow(data, S):
    """The rows RandAugment builds on the host (matrices, fixed point, masks, thresholds, factor bits), interpreted
    as the kernel interprets them, give Pillow's bytes for every op, bin and sign."""
    img = _images(S)[1]
    low = _images(S)[5]
    for bin_ in CASE_BINS:
        ra = data.RandAugment(num_ops=1, magnitude=bin_, num_magnitude_bins=BINS, fill=(128, 3, 250))
        for name in ra.OPS:
            for sign in (0, 1):
                m = ra.magnitude_value(name, S, sign if name in ra.SIGNED else 0)
                assert m == R.magnitude(name, bin_, BINS, S, sign)
                row = ra.row(name, m, S)
                for im in (img, low):
                    assert np.array_equal(_apply_row(im, row), R.pil_chain(im, [(name, m)], (128, 3, 250))), (name, bin_, sign)


def test_randaugment_draws(data):
    a, b = data.RandAugment(seed=5), data.RandAugment(seed=5)
    t1, t2 = a.params(6, 32), b.params(6, 32)
    assert t1.shape == (6, 2, 8) and t1.dtype == np.int32 and np.array_equal(t1, t2)
    assert not np.array_equal(data.RandAugment(seed=6).params(6, 32), t1)
    # state round trip mid-stream reproduces the following draws
    state = a.state_dict()
    nxt = [a.params(4, 32) for _ in range(3)]
    c = data.RandAugment(seed=99)
    c.load_state_dict(state)
    assert all(np.array_equal(c.params(4, 32), t) for t in nxt)
    with pytest.raises(ValueError):
        data.RandAugment(num_ops=3).load_state_dict(state)
    # every op is reachable, and the draw order is op then sign, per image then per slot
    ra = data.RandAugment(num_ops=2, seed=1)
    d = ra.draw(400)
    assert set(d[:, :, 0].reshape(-1)) == set(range(len(ra.OPS))) and set(d[:, :, 1].reshape(-1)) == {0, 1}
    rs = np.random.RandomState(1)
    want = np.array([[(rs.randint(14), rs.randint(2)) for _ in range(2)] for _ in range(400)])
    assert np.array_equal(d, want)
    # a restricted list draws only from it; an unknown name is refused
    only = data.RandAugment(ops=("Rotate", "Equalize"), seed=0).params(50, 32)
    assert set(only[:, :, 0].reshape(-1)) <= {data.RandAugment.K_AFFINE, data.RandAugment.K_EQUALIZE}
    with pytest.raises(ValueError):
        data.RandAugment(ops=("Rotate", "Invert"))
    with pytest.raises(ValueError):
        data.RandAugment(num_ops=data.RandAugment.MAX_OPS + 1)


def test_randaugment_check_params(data, favit):
    RA = data.RandAugment
    assert favit._abi.lib().favit_randaugment_max_ops() == RA.MAX_OPS
    good = RA(seed=0).params(3, 32)
    RA.check_params(good, 3)
    bad = good.copy()
    bad[1, 0, 0] = 7
    with pytest.raises(ValueError, match="unknown op id"):
        RA.check_params(bad, 3)
    bad = good.copy()
    bad[0, 1] = (RA.K_BLEND, 1, int(np.array([np.nan], dtype=np.float32).view(np.int32)[0]), 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="non-finite"):
        RA.check_params(bad, 3)
    bad[0, 1] = (RA.K_BLEND, 4, 0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="degenerate"):
        RA.check_params(bad, 3)
    with pytest.raises(ValueError, match="exceed"):
        RA.check_params(np.zeros((3, RA.MAX_OPS + 1, 8), dtype=np.int32), 3)
    with pytest.raises(ValueError):
        RA.check_params(good.astype(np.int64), 3)
    with pytest.raises(ValueError):
        RA.check_params(good, 4)


def test_random_erasing_draws(data):
    H = W = 32
    scale, ratio = (0.02, 0.33), (0.3, 3.3)
    a, b = data.RandomErasing(p=1.0, seed=3), data.RandomErasing(p=1.0, seed=3)
    (box, seed), (box2, seed2) = a.params(200, H, W), b.params(200, H, W)
    assert box.dtype == np.int32 and box.shape == (200, 4) and np.array_equal(box, box2) and seed == seed2
    # the draws are those of the restatement, in its order
    rs = np.random.RandomState(3)
    assert np.array_equal(box, R.erase_draws(rs, 200, H, W, 1.0, scale, ratio))
    h, w = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
    drawn = (h > 0) & (w > 0)
    assert drawn.sum() > 150
    assert (box[:, 0] >= 0).all() and (box[:, 2] >= 0).all() and (box[:, 1] <= H).all() and (box[:, 3] <= W).all()
    assert (h < H).all() and (w < W).all()
    # area and aspect inside the bounds, up to the rounding of h and w to whole pixels (half a pixel each side)
    hd, wd = h[drawn].astype(np.float64), w[drawn].astype(np.float64)
    assert ((hd + 0.5) * (wd + 0.5) >= scale[0] * H * W).all() and ((hd - 0.5) * (wd - 0.5) <= scale[1] * H * W).all()
    assert ((hd + 0.5) / np.maximum(wd - 0.5, 1e-9) >= ratio[0]).all() and ((hd - 0.5) / (wd + 0.5) <= ratio[1]).all()
    # p = 0: no boxes; p in between: some of each
    assert not data.RandomErasing(p=0.0, seed=1).params(64, H, W)[0].any()
    mid = data.RandomErasing(p=0.25, seed=1).params(400, H, W)[0]
    frac = ((mid[:, 1] > mid[:, 0]) & (mid[:, 3] > mid[:, 2])).mean()
    assert abs(frac - 0.25) < 5 * math.sqrt(0.25 * 0.75 / 400)
    # state round trip mid-stream
    state = a.state_dict()
    nxt = [a.params(8, H, W) for _ in range(3)]
    c = data.RandomErasing(p=1.0, seed=77)
    c.load_state_dict(state)
    for want in nxt:
        got = c.params(8, H, W)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    # seeds of consecutive batches differ (the normal fill of two batches is not the same field)
    assert nxt[0][1] != nxt[1][1]
    for bad in (dict(p=1.5), dict(scale=(0.5, 0.1)), dict(ratio=(0.0, 1.0)), dict(value="gauss"), dict(value=(1.0, float("nan"), 0.0))):
        with pytest.raises(ValueError):
            data.RandomErasing(**bad)
    with pytest.raises(ValueError):
        data.RandomErasing.check_params(np.array([[0, 33, 0, 4]], dtype=np.int32), 1, H, W)


def test_normal_fill_restatement():
    """The uniforms are exact multiples of 2^-24 in (0, 1] / [0, 1), and the fp32 restatement follows fp64."""
    idx = np.arange(1 << 16, dtype=np.uint64) + np.uint64(123456789)
    u1, u2 = R.normal_uniforms(0x1234_5678_9ABC, idx)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.array_equal(u1 * 2.0 ** 24, np.round(u1 * 2.0 ** 24))
    z32, z64 = R.normal_fill(0x1234_5678_9ABC, idx), R.normal_fill(0x1234_5678_9ABC, idx, np.float64)
    assert z32.dtype == np.float32 and np.abs(z32 - z64).max() < 1e-5
    n = idx.size
    assert abs(z64.mean()) < 5 / math.sqrt(n) and abs(z64.var() - 1.0) < 5 * math.sqrt(2.0 / n)
    assert not np.array_equal(z32, R.normal_fill(0x1234_5678_9ABD, idx))


# ---------------------------------------------------------------------------------------------------------------------
def _loader(data, **kw):
    """A DeviceLoader without a device (its streams need a GPU): only its state handling is exercised."""
    L = data.DeviceLoader.__new__(data.DeviceLoader)
    L.src, L.tf = [], data.DeviceTransform("resize", 32, (0.5,) * 3, (0.5,) * 3)
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def test_loader_state_keys(data):
    plain = _loader(data)
    assert set(plain.state_dict()) == {"transform", "batches"}          # exactly the state of a loader without options
    full = _loader(data, augment=data.RandAugment(seed=1), erase=data.RandomErasing(seed=2), mix=data.BatchMix(seed=3))
    assert set(full.state_dict()) == {"transform", "batches", "mix", "augment", "erase"}
    only_aug = _loader(data, augment=data.RandAugment(seed=1))
    assert set(only_aug.state_dict()) == {"transform", "batches", "augment"}
    # round trip restores the generators
    state = full.state_dict()
    want = (full.augment.params(3, 32), full.erase.params(3, 32, 32))
    other = _loader(data, augment=data.RandAugment(seed=8), erase=data.RandomErasing(seed=9), mix=data.BatchMix(seed=10))
    other.load_state_dict(state)
    assert np.array_equal(other.augment.params(3, 32), want[0])
    got = other.erase.params(3, 32, 32)
    assert np.array_equal(got[0], want[1][0]) and got[1] == want[1][1]
    # with / without mismatches raise, naming the part
    with pytest.raises(ValueError, match="with a RandAugment and this loader is built without"):
        plain.check_state_dict(only_aug.state_dict())
    with pytest.raises(ValueError, match="without a RandAugment and this loader is built with"):
        only_aug.check_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="RandomErasing"):
        _loader(data, erase=data.RandomErasing()).check_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="with a RandomErasing"):
        only_aug.check_state_dict(_loader(data, augment=data.RandAugment(), erase=data.RandomErasing()).state_dict())


def test_experiment_tool_flags_default_to_off():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("favit_run_experiment_aug", os.path.join(root, "tools", "run_experiment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--experiment", "mhla"])
    assert a.ra_num_ops == 0 and a.ra_magnitude == 9 and a.erase_prob == 0.0 and a.erase_value == "zero"
    b = tool.parse_args(["--experiment", "mhla", "--ra_num_ops", "2", "--ra_magnitude", "7", "--erase_prob", "0.25",
                         "--erase_value", "normal"])
    assert (b.ra_num_ops, b.ra_magnitude, b.erase_prob, b.erase_value) == (2, 7, 0.25, "normal")
