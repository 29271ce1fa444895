"""Device RandAugment / Random Erasing on the GPU: favit_randaugment against Pillow bit for bit (single ops, chains,
full size), the identity table against the plain transform, the erase fills (constant and normal, fused and
stand-alone) and the loader."""
import math

import numpy as np
import pytest
import torch

import _augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BINS = 31
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)

# Largest |device - fp64| of the normal fill over the elements of test_erase_normal_fill, measured on an MI355X:
# 1.026e-6 (numpy's own fp32 evaluation of the same expression: 9.66e-7; the two are not bit-equal, logf / cosf differ
# in the last place); the bound is 4x the measured figure.
NORMAL_FILL_BOUND = 4 * 1.026e-6


@pytest.fixture(scope="module")
def D(favit):
    return favit.data


def _bits(t):
    return t.contiguous().view(torch.int32)


def _images(B, S, seed=0):
    """B images: noise, a 20-level band, a constant, a ramp, noise ..."""
    rng = np.random.RandomState(seed + S)
    yy, xx = np.mgrid[0:S, 0:S]
    kinds = [lambda: rng.randint(0, 256, (S, S, 3)), lambda: 100 + rng.randint(0, 20, (S, S, 3)),
             lambda: np.full((S, S, 3), 77), lambda: np.stack([(yy * 7) % 256, xx * 255 // S, ((xx + yy) * 4) % 256], 2)]
    return np.stack([kinds[b % 4]() for b in range(B)]).astype(np.uint8)


def _table(ra, chains, S, n_ops):
    t = np.zeros((len(chains), n_ops, 8), dtype=np.int32)
    for b, ch in enumerate(chains):
        for s, (name, m) in enumerate(ch):
            t[b, s] = ra.row(name, m, S)
    return t


def _own_normalize(D, u8, S):
    """ToTensor + Normalize of bytes [B,S,S,3] by the transform's own kernel (an S -> S resize is the identity)."""
    return D.DeviceTransform("resize", S, MEAN, STD)(u8)


def _run_and_check(D, imgs, chains, fill, n_ops):
    """favit_randaugment on imgs [B,S,S,3] with one chain per image: bytes against Pillow, fp32 against the
    transform's own expression on those bytes."""
    B, S = imgs.shape[0], imgs.shape[1]
    ra = D.RandAugment(num_ops=n_ops, fill=fill)
    tf = D.DeviceTransform("resize", S, MEAN, STD)
    out, u8 = ra(torch.from_numpy(imgs).to(DEV), tf.mean, tf.std, params=_table(ra, chains, S, n_ops), want_bytes=True)
    got = u8.cpu().numpy()
    for b, ch in enumerate(chains):
        want = R.pil_chain(imgs[b], ch, fill)
        assert np.array_equal(got[b], want), f"image {b} {ch}: {(got[b] != want).sum()} bytes differ from Pillow"
    assert torch.equal(_bits(out), _bits(_own_normalize(D, u8, S)))
    assert np.array_equal(out.cpu().numpy(), R.normalize(got, MEAN, STD))


@pytest.mark.parametrize("S", [32, 40])
def test_single_ops_match_pillow(D, S):
    """Every op of the table at bins 0, mid, max and both signs, five images per launch (each op meets noise, band,
    constant and ramp images over its six cases), fills (0,0,0) and a coloured one."""
    B = 5
    cases = [(op, bin_, sign) for op in R.OPS for bin_ in (0, 15, 30) for sign in (0, 1)]
    cases += cases[:(-len(cases)) % B]
    for k in range(0, len(cases), B):
        imgs = np.roll(_images(B, S, seed=k), k // B, axis=0)
        chains = [[(op, R.magnitude(op, bin_, BINS, S, sign))] for op, bin_, sign in cases[k:k + B]]
        _run_and_check(D, imgs, chains, (0, 0, 0) if (k // B) % 2 == 0 else (128, 3, 250), 1)


@pytest.mark.parametrize("fill", [(0, 0, 0), (9, 200, 31)])
def test_chains_match_pillow(D, fill):
    """Chains of 2 and 3 ops in one launch: geometric -> Equalize / Contrast / AutoContrast (the fill region enters the
    statistics), Sharpness -> Rotate (the filtered plane is gathered from), LUT ops back to back."""
    S = 32
    chains = [[("Rotate", 21.0), ("Equalize", None)],
              [("ShearX", -0.3), ("Contrast", 0.9)],
              [("Sharpness", 0.9), ("Rotate", -30.0)],
              [("TranslateX", 9.7), ("AutoContrast", None), ("Color", -0.45)],
              [("ShearY", 0.2), ("Equalize", None), ("Sharpness", -0.6)],
              [("Posterize", 4), ("Solarize", 110.5), ("Brightness", 0.33)],
              [("TranslateY", -14.2), ("Contrast", -0.9), ("Rotate", 7.0)]]
    imgs = _images(len(chains), S, seed=3)
    imgs[2], imgs[1] = imgs[0][::-1], imgs[3]          # Sharpness and Contrast on textured images
    _run_and_check(D, np.ascontiguousarray(imgs), chains, fill, 3)


def test_full_size_chain_matches_pillow(D):
    """S = 224: 150 KB per image, every stage strides the workgroup many times over the scratch planes."""
    S = 224
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:S, 0:S]
    smooth = np.stack([(yy + xx) // 2, 255 - yy, (xx * 3) % 256], 2)
    imgs = np.stack([np.clip(smooth + rng.randint(-20, 21, (S, S, 3)), 0, 255), rng.randint(0, 256, (S, S, 3))]).astype(np.uint8)
    # image 1: the 2-op chain; image 0 adds a third op, which writes the plane the first op's result was read from
    _run_and_check(D, imgs, [[("Rotate", 9.0), ("Equalize", None), ("Sharpness", 0.63)],
                             [("Sharpness", 0.27), ("ShearY", -0.09)]], (0, 0, 0), 3)


def test_identity_table_gives_the_plain_transform(D):
    """An all-Identity table (and num_ops = 0) returns the bits of DeviceTransform.__call__, uniform and ragged."""
    S, rs = 32, np.random.RandomState(0)
    x = torch.from_numpy(rs.randint(0, 256, (4, 40, 40, 3)).astype(np.uint8)).to(DEV)
    tf = D.DeviceTransform("resize_flip", S, MEAN, STD, seed=1)
    prm = tf.params(4, 40, 40)
    plain = tf(x, params=prm)
    both, u8 = tf(x, params=prm, want_bytes=True)
    assert torch.equal(_bits(plain), _bits(both))
    for ra in (D.RandAugment(num_ops=2, ops=("Identity",)), D.RandAugment(num_ops=0)):
        out, u8b = ra(u8, tf.mean, tf.std, want_bytes=True)
        assert torch.equal(_bits(out), _bits(plain)) and torch.equal(u8b, u8)
    sizes = [(45, 60), (33, 33), (64, 40)]
    rb = D.RaggedBatch.from_images([rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]).to(DEV)
    tfr = D.DeviceTransform("imagenet_train", S, MEAN, STD, seed=2)
    prm = tfr.params(3, rb.heights, rb.widths)
    plain = tfr(rb, params=prm)
    _, u8 = tfr(rb, params=prm, want_bytes=True)
    out = D.RandAugment(num_ops=3, ops=("Identity",))(u8, tfr.mean, tfr.std)
    assert torch.equal(_bits(out), _bits(plain))


# ---------------------------------------------------------------------------------------------------------------------
# (y0, y1, x0, x1): edges off the 4-element groups, group-aligned, one pixel, one column, reaching the last row and
# column, empty (twice: zero rows, and x0 == x1)
BOXES = [(3, 17, 5, 19), (0, 8, 4, 12), (7, 8, 9, 10), (2, 29, 13, 14), (20, 30, 22, 30), (0, 0, 0, 0), (4, 9, 6, 6)]


def _check_erased(before, after, box, fill_of):
    """Inside the box `after` is the fill, outside every bit of `before` is kept.  fill_of(b, region) -> expected
    values [C, h, w] of image b for the index region."""
    before, after = before.cpu(), after.cpu()
    for b, (y0, y1, x0, x1) in enumerate(box):
        want = before[b].clone()
        if y0 < y1 and x0 < x1:
            want[:, y0:y1, x0:x1] = fill_of(b, (slice(y0, y1), slice(x0, x1)))
        assert torch.equal(_bits(after[b]), _bits(want)), f"image {b} box {(y0, y1, x0, x1)}"


@pytest.mark.parametrize("S", [32, 30])
def test_erase_constant_fill(D, favit, S):
    """Fused (favit_randaugment's final write) and stand-alone (favit_random_erase, 16-byte groups at S = 32, single
    elements at S = 30), a number and a per-channel value."""
    K = favit.kernels
    box = np.array([tuple(min(v, S) for v in bx) for bx in BOXES], dtype=np.int32)
    B = len(box)
    imgs = torch.from_numpy(_images(B, S, seed=9)).to(DEV)
    tf = D.DeviceTransform("resize", S, MEAN, STD)
    ra = D.RandAugment(num_ops=1, ops=("Equalize",))
    tbl = ra.params(B, S)
    clean = ra(imgs, tf.mean, tf.std, params=tbl)
    d_box = torch.from_numpy(box).to(DEV)
    for value in (0, 1.5, (0.25, -1.0, 2.0)):
        v3 = torch.tensor([value] * 3 if np.ndim(value) == 0 else value, dtype=torch.float32)
        fill_of = lambda b, reg: v3[:, None, None].expand(3, S, S)[(slice(None),) + reg]       # noqa: E731
        fused = ra(imgs, tf.mean, tf.std, params=tbl, erase_box=d_box, erase_value=value)
        _check_erased(clean, fused, box, fill_of)
        alone = K.random_erase(clean.clone(), d_box, value)
        _check_erased(clean, alone, box, fill_of)
        assert torch.equal(_bits(alone), _bits(D.RandomErasing(value=value)(clean.clone(), params=(box, 0))))
    # a misaligned base pointer takes the single-element path, with the same result
    buf = torch.zeros(clean.numel() + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view_as(clean).copy_(clean)
    assert view.data_ptr() % 16 != 0
    _check_erased(clean, K.random_erase(view, d_box, 1.5), box, lambda b, reg: torch.full((3, S, S), 1.5)[(slice(None),) + reg])
    assert float(buf[0]) == 0.0


def test_erase_normal_fill(D, favit):
    """The normal fill against its numpy restatement, fused and stand-alone (two launch geometries: the same bits).

    Equality with numpy's fp32 evaluation holds only if logf / cosf agree in the last place, so the assertion is
    against the fp64 value of the same two uniforms: measured on an MI355X max |device - fp64| = 1.026e-6 over these
    elements (numpy's fp32 evaluation: 9.66e-7, not bit-equal to the device's), bound NORMAL_FILL_BOUND = 4x that =
    4.1e-6, against values of up to 5.8 in magnitude.  The figures are printed."""
    K = favit.kernels
    S, seed = 32, 0x5EED_1234_ABCD
    box = np.array([(3, 17, 5, 19), (0, 31, 1, 30), (0, 0, 0, 0)], dtype=np.int32)
    B = len(box)
    imgs = torch.from_numpy(_images(B, S, seed=2)).to(DEV)
    tf = D.DeviceTransform("resize", S, MEAN, STD)
    ra = D.RandAugment(num_ops=1, ops=("Identity",))
    clean = ra(imgs, tf.mean, tf.std)
    d_box = torch.from_numpy(box).to(DEV)
    fused = ra(imgs, tf.mean, tf.std, erase_box=d_box, erase_value="normal", erase_seed=seed)
    alone = K.random_erase(clean.clone(), d_box, "normal", seed)
    assert torch.equal(_bits(fused), _bits(alone))
    z32 = [torch.from_numpy(R.normal_fill(seed, R.element_index(b, 3, S, S))) for b in range(B)]
    z64 = [R.normal_fill(seed, R.element_index(b, 3, S, S), np.float64) for b in range(B)]
    # outside the boxes nothing moves; inside, the restatement's values up to the libm difference
    got = fused.cpu()
    probe = got.clone()
    worst = worst32 = 0.0
    exact = True
    for b, (y0, y1, x0, x1) in enumerate(box):
        if y0 < y1 and x0 < x1:
            g = got[b, :, y0:y1, x0:x1].numpy()
            worst = max(worst, float(np.abs(g - z64[b][:, y0:y1, x0:x1]).max()))
            worst32 = max(worst32, float(np.abs(z32[b][:, y0:y1, x0:x1].numpy() - z64[b][:, y0:y1, x0:x1]).max()))
            exact = exact and np.array_equal(g, z32[b][:, y0:y1, x0:x1].numpy())
            probe[b, :, y0:y1, x0:x1] = clean[b, :, y0:y1, x0:x1].cpu()
    print(f"normal fill: max |device - fp64| = {worst:.3e}, numpy fp32 - fp64 = {worst32:.3e}, bit-equal to numpy fp32: {exact}")
    assert torch.equal(_bits(probe), _bits(clean.cpu()))
    assert worst <= NORMAL_FILL_BOUND
    # the same seed gives the same bits, another seed others
    again = K.random_erase(clean.clone(), d_box, "normal", seed)
    other = K.random_erase(clean.clone(), d_box, "normal", seed + 1)
    assert torch.equal(_bits(again), _bits(alone)) and not torch.equal(_bits(other), _bits(alone))
    # moments over one box of 3 * 60 * 60 = 10800 elements
    x = torch.zeros((1, 3, 64, 64), dtype=torch.float32, device=DEV)
    K.random_erase(x, torch.tensor([[2, 62, 1, 61]], dtype=torch.int32, device=DEV), "normal", 77)
    z = x[0, :, 2:62, 1:61].double().cpu().numpy().reshape(-1)
    n = z.size
    assert n >= 10 ** 4 and abs(z.mean()) < 5 / math.sqrt(n) and abs(z.var() - 1.0) < 5 * math.sqrt(2.0 / n)
    x[0, :, 2:62, 1:61] = 0.0
    assert not bool(x.any())                               # nothing outside the box was written


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_device_loader_augments_erases_and_mixes(D, ragged):
    """DeviceLoader(augment=, erase=, mix=) over 3 batches of B = 4 equals the same steps done by hand from the same
    seeds (and the augmented bytes are Pillow's for the drawn ops); the state saved after batch 1, loaded into a fresh
    loader, reproduces batches 2-3 bit for bit."""
    B, S = 4, 32
    rs = np.random.RandomState(4)
    host = []
    for _ in range(3):
        if ragged:
            imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((45, 60), (33, 33), (64, 40), (50, 50))]
            host.append((D.RaggedBatch.from_images(imgs), rs.randint(0, 10, size=B)))
        else:
            host.append((rs.randint(0, 256, size=(B, 40, 40, 3)).astype(np.uint8), rs.randint(0, 10, size=B)))
    kind = "imagenet_train" if ragged else "resize_flip"

    def parts(s):
        return (D.DeviceTransform(kind, S, MEAN, STD, seed=s), D.RandAugment(2, 9, seed=s + 1),
                D.RandomErasing(p=0.75, value="normal", seed=s + 2), D.BatchMix(0.8, 1.0, mode="elem", seed=s + 3))

    tf, ra, er, mix = parts(10)
    loader = D.DeviceLoader(host, tf, augment=ra, erase=er, mix=mix)
    tf_r, ra_r, er_r, mix_r = parts(10)
    seen, state = [], None
    for k, (images, mixed) in enumerate(loader):
        src = host[k][0].to(DEV) if ragged else torch.from_numpy(host[k][0]).to(DEV)
        _, u8 = tf_r(src, want_bytes=True)
        draws = ra_r.draw(B)
        box, seed = er_r.params(B, S, S)
        x, u8a = ra_r(u8, tf_r.mean, tf_r.std, params=ra_r.table(draws, S), erase_box=torch.from_numpy(box).to(DEV),
                      erase_value="normal", erase_seed=seed, want_bytes=True)
        x, ml = mix_r(x, torch.from_numpy(host[k][1]).long().to(DEV))
        assert torch.equal(_bits(images), _bits(x)) and torch.equal(mixed.lam, ml.lam) and torch.equal(mixed.labels, ml.labels)
        for b in range(B):
            chain = []
            for op_i, sign in draws[b]:
                name = ra_r.ops[int(op_i)]
                chain.append((name, R.magnitude(name, 9, BINS, S, int(sign))))
            assert np.array_equal(u8a[b].cpu().numpy(), R.pil_chain(u8[b].cpu().numpy(), chain))
        seen.append(images.clone())
        if k == 0:
            state = loader.state_dict()
    assert len(seen) == 3 and set(state) == {"transform", "batches", "mix", "augment", "erase"}
    loader2 = D.DeviceLoader(host[1:], *parts(50)[:1], augment=parts(51)[1], erase=parts(52)[2], mix=parts(53)[3])
    loader2.load_state_dict(state)
    rest = [im for im, _ in loader2]
    assert len(rest) == 2 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(rest, seen[1:]))
    with pytest.raises(ValueError, match="RandAugment"):
        D.DeviceLoader(host[:1], parts(1)[0], mix=parts(1)[3]).load_state_dict(state)


def test_device_loader_erases_without_augment(D):
    """erase alone: the stand-alone kernel after the plain transform; labels stay plain tensors."""
    B, S = 4, 32
    rs = np.random.RandomState(6)
    host = [(rs.randint(0, 256, size=(B, 40, 40, 3)).astype(np.uint8), rs.randint(0, 10, size=B)) for _ in range(2)]
    loader = D.DeviceLoader(host, D.DeviceTransform("resize", S, MEAN, STD), erase=D.RandomErasing(p=1.0, value=(1.0, 2.0, 3.0), seed=3))
    tf_r, er_r = D.DeviceTransform("resize", S, MEAN, STD), D.RandomErasing(p=1.0, value=(1.0, 2.0, 3.0), seed=3)
    for k, (images, labels) in enumerate(loader):
        assert torch.is_tensor(labels)
        clean = tf_r(torch.from_numpy(host[k][0]).to(DEV))
        box, _ = er_r.params(B, S, S)
        v3 = torch.tensor([1.0, 2.0, 3.0])
        _check_erased(clean, images, box, lambda b, reg: v3[:, None, None].expand(3, S, S)[(slice(None),) + reg])
    assert set(loader.state_dict()) == {"transform", "batches", "erase"}
