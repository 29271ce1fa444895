"""Host side of the on-disk dataset readers (datasets.py) and of ragged batches (data.RaggedBatch, DeviceTransform.params
with per-image sizes): everything here runs without a GPU.  The reference's counterparts are load_cifar10 /
load_imagenet_subset (utils/data_utils.py:83-244) over torchvision's CIFAR10 / ImageFolder; torchvision is not
importable here, so the layout rules are restated from its documentation and Pillow is the decoder to compare with.
"""
import gc
import os
import threading

import numpy as np
import pytest
from PIL import Image


# ------------------------------------------------------------------ fixtures written by the tests themselves ----
def write_cifar(root, n_per_file=40, seed=0):
    """Five train files and a test file of random CIFAR-10 binary records; returns ({train|test: (x HWC, y)})."""
    rs = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    out = {}
    for split, names in (("train", [f"data_batch_{i}.bin" for i in range(1, 6)]), ("test", ["test_batch.bin"])):
        xs, ys = [], []
        for n in names:
            y = rs.randint(0, 10, size=n_per_file).astype(np.uint8)
            planes = rs.randint(0, 256, size=(n_per_file, 3, 32, 32), dtype=np.uint8)     # R, G, B planes, row-major
            rec = np.concatenate([y[:, None], planes.reshape(n_per_file, -1)], axis=1)
            assert rec.shape[1] == 3073
            rec.tofile(os.path.join(root, n))
            xs.append(planes.transpose(0, 2, 3, 1))
            ys.append(y.astype(np.int64))
        out[split] = (np.concatenate(xs), np.concatenate(ys))
    return out


# class directories created in an order that differs from the sorted one
FOLDER_SPEC = [
    ("zebra", [("a.png", (32, 32), "RGB"), ("c.png", (180, 240), "L"), ("b.png", (37, 53), "RGBA")]),
    ("apple", [("img2.png", (500, 333), "P"), ("img10.PNG", (40, 200), "RGB"), ("notes.txt", None, None)]),
    ("mango", [("x.png", (64, 48), "RGB"), ("sub/y.png", (33, 47), "L")]),
]


def write_image_tree(root, seed=0):
    """PNG files (lossless) of several sizes and modes; returns the expected (path, class index) list in torchvision's
    order: classes sorted, files of a class walked in sorted order."""
    rs = np.random.RandomState(seed)
    for cls, files in FOLDER_SPEC:
        for name, hw, mode in files:
            path = os.path.join(root, cls, name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if hw is None:
                with open(path, "w") as f:
                    f.write("not an image\n")
                continue
            h, w = hw
            if mode == "L":
                im = Image.fromarray(rs.randint(0, 256, size=(h, w), dtype=np.uint8), "L")
            elif mode == "RGBA":
                im = Image.fromarray(rs.randint(0, 256, size=(h, w, 4), dtype=np.uint8), "RGBA")
            elif mode == "P":
                im = Image.fromarray(rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB").convert("P")
            else:
                im = Image.fromarray(rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB")
            im.save(path, format="PNG")
    j = os.path.join
    return [(j(root, "apple", "img10.PNG"), 0), (j(root, "apple", "img2.png"), 0),
            (j(root, "mango", "x.png"), 1), (j(root, "mango", "sub", "y.png"), 1),
            (j(root, "zebra", "a.png"), 2), (j(root, "zebra", "b.png"), 2), (j(root, "zebra", "c.png"), 2)]


# ------------------------------------------------------------------ CIFAR-10 binary ----
@pytest.mark.parametrize("nested", [False, True])
def test_cifar10_binary_reads_records_in_file_order(favit, tmp_path, nested):
    DS = favit.datasets
    root = tmp_path / "cifar-10-batches-bin" if nested else tmp_path
    want = write_cifar(str(root))
    for train in (True, False):
        ds = DS.Cifar10Binary(str(tmp_path), train)
        x, y = want["train" if train else "test"]
        assert ds.x.dtype == np.uint8 and ds.x.shape == x.shape and ds.y.dtype == np.int64
        np.testing.assert_array_equal(ds.x, x)
        np.testing.assert_array_equal(ds.y, y)
        assert len(ds) == len(y)
        assert ds.classes == ["airplane", "automobile", "bird", "cat", "deer", "dog", "frog", "horse", "ship", "truck"]


def test_cifar10_binary_class_names_from_meta_file(favit, tmp_path):
    write_cifar(str(tmp_path), n_per_file=4)
    names = [f"c{i}" for i in range(10)]
    (tmp_path / "batches.meta.txt").write_text("\n".join(names) + "\n\n")
    assert favit.datasets.Cifar10Binary(str(tmp_path), False).classes == names


def test_cifar10_binary_refuses_bad_files(favit, tmp_path):
    DS = favit.datasets
    write_cifar(str(tmp_path / "ok"), n_per_file=8)
    # truncated file
    t = tmp_path / "trunc"
    write_cifar(str(t), n_per_file=8)
    raw = (t / "data_batch_3.bin").read_bytes()
    (t / "data_batch_3.bin").write_bytes(raw[:-5])
    with pytest.raises(ValueError, match="multiple of"):
        DS.Cifar10Binary(str(t), True)
    DS.Cifar10Binary(str(t), False)                       # the test file is intact
    # label 10
    l = tmp_path / "label"
    write_cifar(str(l), n_per_file=8)
    raw = bytearray((l / "test_batch.bin").read_bytes())
    raw[3073 * 2] = 10
    (l / "test_batch.bin").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="label 10"):
        DS.Cifar10Binary(str(l), False)
    # only the pickled distribution: refused by name, nothing is unpickled (the file is not a pickle at all)
    p = tmp_path / "py" / "cifar-10-batches-py"
    p.mkdir(parents=True)
    for n in [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch", "batches.meta"]:
        (p / n).write_bytes(b"\x00not a pickle")
    with pytest.raises(FileNotFoundError, match="binary distribution"):
        DS.Cifar10Binary(str(tmp_path / "py"), True)
    with pytest.raises(FileNotFoundError):
        DS.Cifar10Binary(str(tmp_path / "missing"), True)
    with pytest.raises(FileNotFoundError):
        DS.Cifar10Binary(str(tmp_path), True)             # a directory without any of the files


def test_cifar10_binary_subset_is_seeded(favit, tmp_path):
    DS = favit.datasets
    want = write_cifar(str(tmp_path))
    a, b = DS.Cifar10Binary(str(tmp_path), True, subset_size=50, seed=3), DS.Cifar10Binary(str(tmp_path), True, subset_size=50, seed=3)
    c = DS.Cifar10Binary(str(tmp_path), True, subset_size=50, seed=4)
    assert len(a) == 50 and a.x.shape == (50, 32, 32, 3)
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.y, b.y)
    assert not np.array_equal(a.x, c.x)
    # every kept record is one of the file's records, each at most once
    flat = {want["train"][0][i].tobytes(): i for i in range(len(want["train"][1]))}
    idx = [flat[a.x[i].tobytes()] for i in range(50)]
    assert len(set(idx)) == 50
    np.testing.assert_array_equal(a.y, want["train"][1][idx])


# ------------------------------------------------------------------ ImageFolder ----
def test_image_folder_layout_order_and_decoding(favit, tmp_path):
    DS = favit.datasets
    want = write_image_tree(str(tmp_path))
    ds = DS.ImageFolder(str(tmp_path))
    assert ds.classes == ["apple", "mango", "zebra"]
    assert ds.class_to_idx == {"apple": 0, "mango": 1, "zebra": 2}
    assert ds.samples == want                              # notes.txt skipped, img10.PNG kept (and sorted before img2.png)
    assert len(ds) == 7 and ds.targets.tolist() == [t for _, t in want]
    shapes = []
    for i, (path, _) in enumerate(want):
        got = ds.load(i)
        ref = np.asarray(Image.open(path).convert("RGB"))
        assert got.dtype == np.uint8 and got.ndim == 3 and got.shape[2] == 3
        np.testing.assert_array_equal(got, ref)
        shapes.append(got.shape[:2])
    assert shapes == [(40, 200), (500, 333), (64, 48), (33, 47), (32, 32), (37, 53), (180, 240)]


def test_image_folder_refuses_an_empty_class_and_a_missing_root(favit, tmp_path):
    DS = favit.datasets
    write_image_tree(str(tmp_path))
    (tmp_path / "berry").mkdir()
    (tmp_path / "berry" / "readme.txt").write_text("no image here")
    with pytest.raises(FileNotFoundError, match="berry"):
        DS.ImageFolder(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        DS.ImageFolder(str(tmp_path / "nowhere"))


def test_image_folder_subset_is_seeded(favit, tmp_path):
    DS = favit.datasets
    want = write_image_tree(str(tmp_path))
    a, b = DS.ImageFolder(str(tmp_path), subset_size=4, seed=1), DS.ImageFolder(str(tmp_path), subset_size=4, seed=1)
    assert len(a) == 4 and a.samples == b.samples and len(set(a.samples)) == 4 and set(a.samples) <= set(want)
    assert a.targets.tolist() == [t for _, t in a.samples]
    assert a.classes == ["apple", "mango", "zebra"]


# ------------------------------------------------------------------ RaggedBatch ----
def test_ragged_batch_from_images_round_trips(favit):
    D = favit.data
    rs = np.random.RandomState(0)
    sizes = [(32, 32), (37, 53), (5, 200), (64, 48)]
    imgs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    rb = D.RaggedBatch.from_images(imgs)
    assert len(rb) == 4 and rb.channels == 3 and not rb.is_cuda
    assert rb.offsets.dtype == np.int64 and rb.heights.dtype == np.int32 and rb.widths.dtype == np.int32
    run = np.cumsum([0] + [h * w * 3 for h, w in sizes])
    assert rb.offsets.tolist() == run[:-1].tolist() and rb.bytes.numel() == run[-1]
    assert rb.heights.tolist() == [h for h, _ in sizes] and rb.widths.tolist() == [w for _, w in sizes]
    raw = rb.bytes.numpy()
    for b, im in enumerate(imgs):
        np.testing.assert_array_equal(raw[run[b]:run[b + 1]].reshape(im.shape), im)
        np.testing.assert_array_equal(rb.image(b), im)
    d = rb.descriptors()
    assert d.dtype == np.int64 and d.shape == (4, 3) and d[:, 0].tolist() == rb.offsets.tolist()
    with pytest.raises(TypeError):
        D.RaggedBatch.from_images([imgs[0], imgs[1].astype(np.float32)])


def test_ragged_descriptors_are_checked_on_the_host(favit):
    """The kernel trusts the descriptor rows, so a row that leaves the buffer is refused from the host arrays."""
    D = favit.data
    rs = np.random.RandomState(1)
    mk = lambda: D.RaggedBatch.from_images([rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in [(8, 9), (10, 4)]])
    mk().descriptors()
    rb = mk(); rb.heights[1] += 1
    with pytest.raises(ValueError, match="image 1"):
        rb.descriptors()
    rb = mk(); rb.offsets[1] += 1
    with pytest.raises(ValueError, match="image 1"):
        rb.descriptors()
    rb = mk(); rb.offsets[0] = -3
    with pytest.raises(ValueError, match="image 0"):
        rb.descriptors()
    rb = mk(); rb.widths[0] = 0
    with pytest.raises(ValueError, match="image 0"):
        rb.descriptors()
    rb = mk(); rb.heights = rb.heights[:1]
    with pytest.raises(ValueError):
        rb.descriptors()


# ------------------------------------------------------------------ params with per-image sizes ----
SIZES = [(32, 32), (37, 53), (180, 240), (375, 500), (500, 333), (64, 48), (224, 224), (40, 200), (1200, 1600)]


@pytest.mark.parametrize("S", [224, 64])
def test_params_with_arrays_draw_each_row_from_its_own_image(favit, S):
    D = favit.data
    H, W = np.array([h for h, _ in SIZES]), np.array([w for _, w in SIZES])
    tf = D.DeviceTransform("imagenet_test", S, D.IMAGENET_MEAN, D.IMAGENET_STD)
    p = tf.params(len(SIZES), H, W)
    assert p.dtype == np.int32 and p.shape == (len(SIZES), 12)
    for b, (h, w) in enumerate(SIZES):
        np.testing.assert_array_equal(p[b], tf.params(1, h, w)[0])
    if S == 224:
        assert (p[3, 5], p[3, 6]) == (255, 340) and (p[3, 7], p[3, 8]) == (16, 58)      # (375, 500): Resize(255) -> CenterCrop(224)
    tf = D.DeviceTransform("imagenet_train", S, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=5)
    for _ in range(20):
        p = tf.params(len(SIZES), H, W)
        assert (p[:, 0] >= 0).all() and (p[:, 1] >= 0).all() and (p[:, 2] > 0).all() and (p[:, 3] > 0).all()
        assert (p[:, 0] + p[:, 2] <= H).all() and (p[:, 1] + p[:, 3] <= W).all()          # each box inside its own image
        assert (p[:, 5] == S).all() and (p[:, 6] == S).all() and (p[:, 4] == 0).all()
    # the boxes of the large image use its extent, those of the small one cannot
    assert p[8, 2] > 40 and p[0, 2] <= 32


def _old_imagenet_train_rows(r, B, H, W, S):
    """The scalar path's RandomResizedCrop draws, call for call (scale (0.08, 1), log-uniform ratio (3/4, 4/3), ten tries)."""
    import math
    p = np.zeros((B, 12), dtype=np.int32)
    for b in range(B):
        box = None
        for _ in range(10):
            ta = H * W * r.uniform(0.08, 1.0)
            ar = math.exp(r.uniform(math.log(3.0 / 4.0), math.log(4.0 / 3.0)))
            w, h = int(round(math.sqrt(ta * ar))), int(round(math.sqrt(ta / ar)))
            if 0 < w <= W and 0 < h <= H:
                box = (r.randint(0, H - h + 1), r.randint(0, W - w + 1), h, w)
                break
        assert box is not None                                # (the sizes used below never reach the fallback)
        p[b, 0:4] = box
    p[:, 5], p[:, 6] = S, S
    p[:, 10] = r.rand(B) < 0.5
    return p


@pytest.mark.parametrize("kind", ["cifar10_train", "imagenet_train", "resize", "resize_flip", "imagenet_test"])
def test_params_scalar_path_draws_as_before(favit, kind):
    """Scalars behave as before the array form existed: the same draws from the same seed, in the same order of
    generator calls (restated here from numpy's RandomState), and two transforms built alike agree call after call."""
    D = favit.data
    a = D.DeviceTransform(kind, 64, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=7)
    b = D.DeviceTransform(kind, 64, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=7)
    r = np.random.RandomState(7)
    for B in (6, 1, 16):
        p = a.params(B, 32, 32)
        np.testing.assert_array_equal(p, b.params(B, 32, 32))
        if kind == "cifar10_train":
            np.testing.assert_array_equal(p[:, 0], r.randint(0, 9, B))
            np.testing.assert_array_equal(p[:, 1], r.randint(0, 9, B))
            np.testing.assert_array_equal(p[:, 9], r.rand(B) < 0.5)
            assert (p[:, 2:7] == [32, 32, 4, 64, 64]).all()
        elif kind == "imagenet_train":
            np.testing.assert_array_equal(p, _old_imagenet_train_rows(r, B, 32, 32, 64))
        elif kind == "resize_flip":
            np.testing.assert_array_equal(p[:, 10], r.rand(B) < 0.5)
            assert (p[:, 2:7] == [32, 32, 0, 64, 64]).all()
        elif kind == "resize":
            assert (p == [0, 0, 32, 32, 0, 64, 64, 0, 0, 0, 0, 0]).all()
        else:                                                     # imagenet_test: Resize(72) -> CenterCrop(64)
            assert (p == [0, 0, 32, 32, 0, 72, 72, 4, 4, 0, 0, 0]).all()


def test_resize_refuses_non_square_sources_per_image(favit):
    D = favit.data
    for kind in ("resize", "resize_flip"):
        tf = D.DeviceTransform(kind, 64, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        tf.params(3, np.array([32, 48, 500]), np.array([32, 48, 500]))
        with pytest.raises(ValueError, match=r"image 2 \(37x53\).*non-square"):
            tf.params(4, np.array([32, 48, 37, 64]), np.array([32, 48, 53, 64]))
    tf = D.DeviceTransform("imagenet_test", 32, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="filter taps"):           # check_params applies per row, unchanged
        tf.params(2, np.array([64, 4000]), np.array([64, 4000]))


# ------------------------------------------------------------------ batches ----
def _key(img):
    return (img.shape, img.tobytes())


def test_batches_cifar_epochs(favit, tmp_path):
    DS = favit.datasets
    want = write_cifar(str(tmp_path), n_per_file=21)              # 105 train records
    ds = DS.Cifar10Binary(str(tmp_path), True)
    it = DS.batches(ds, 32, shuffle=True, seed=9)
    assert len(it) == 4 and len(DS.batches(ds, 32, True, 9, drop_last=True)) == 3
    epochs = []
    for _ in range(2):
        got = list(it)
        assert [len(y) for _, y in got] == [32, 32, 32, 9]
        assert all(x.dtype == np.uint8 and x.shape[1:] == (32, 32, 3) and y.dtype == np.int64 for x, y in got)
        x, y = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
        src = {want["train"][0][i].tobytes(): i for i in range(105)}
        idx = [src[x[i].tobytes()] for i in range(105)]
        assert sorted(idx) == list(range(105))                    # every sample once
        np.testing.assert_array_equal(y, want["train"][1][idx])
        epochs.append(idx)
    assert epochs[0] != epochs[1]                                 # a fresh shuffle per epoch
    again = DS.batches(ds, 32, shuffle=True, seed=9)
    for e in range(2):
        x = np.concatenate([g[0] for g in again])
        np.testing.assert_array_equal(x, want["train"][0][epochs[e]])       # same seed -> same epochs
    assert [len(y) for _, y in DS.batches(ds, 32, True, 9, drop_last=True)] == [32, 32, 32]
    plain = list(DS.batches(ds, 50, shuffle=False, seed=0))
    np.testing.assert_array_equal(np.concatenate([g[0] for g in plain]), want["train"][0])


def test_batches_image_folder_epochs(favit, tmp_path):
    DS, D = favit.datasets, favit.data
    want = write_image_tree(str(tmp_path))
    ds = DS.ImageFolder(str(tmp_path))
    ref = [np.asarray(Image.open(p).convert("RGB")) for p, _ in want]
    keys = {_key(r): i for i, r in enumerate(ref)}
    it = DS.batches(ds, 3, shuffle=True, seed=2, num_workers=3)
    assert len(it) == 3 and len(DS.batches(ds, 3, True, 2, drop_last=True)) == 2
    orders = []
    for _ in range(3):
        idx = []
        sizes = []
        for rb, y in it:
            assert isinstance(rb, D.RaggedBatch) and y.dtype == np.int64 and len(rb) == len(y)
            rb.descriptors()
            sizes.append(len(rb))
            for b in range(len(rb)):
                i = keys[_key(rb.image(b))]
                assert int(y[b]) == want[i][1]
                idx.append(i)
        assert sizes == [3, 3, 1] and sorted(idx) == list(range(7))
        orders.append(idx)
    assert len({tuple(o) for o in orders}) > 1
    again = DS.batches(ds, 3, shuffle=True, seed=2, num_workers=16)
    assert [keys[_key(rb.image(b))] for rb, _ in again for b in range(len(rb))] == orders[0]
    assert [len(rb) for rb, _ in DS.batches(ds, 3, True, 2, drop_last=True)] == [3, 3]
    plain = [keys[_key(rb.image(b))] for rb, _ in DS.batches(ds, 4, False, 0) for b in range(len(rb))]
    assert plain == list(range(7))                                # unshuffled: the sample order


def test_batches_worker_count_is_capped(favit, tmp_path):
    DS = favit.datasets
    write_image_tree(str(tmp_path))
    it = DS.batches(DS.ImageFolder(str(tmp_path)), 2, False, 0, num_workers=400)
    assert it.workers == 16 and DS.MAX_WORKERS == 16


def test_abandoned_epoch_leaves_no_blocking_thread(favit, tmp_path):
    DS = favit.datasets
    write_image_tree(str(tmp_path))
    ds = DS.ImageFolder(str(tmp_path))
    before = {t.ident for t in threading.enumerate()}
    ep = iter(DS.batches(ds, 1, shuffle=True, seed=0, num_workers=4))
    next(ep)                                                      # one batch, then walk away
    mine = [t for t in threading.enumerate() if t.ident not in before]
    assert mine and all(t.daemon for t in mine)                   # nothing that would hold the interpreter at exit
    del ep
    gc.collect()
    for t in mine:
        t.join(timeout=5.0)
    assert not any(t.is_alive() for t in mine)                    # and they end once the iterator is collected
    # a failing decode reaches the consumer as its exception
    bad = os.path.join(str(tmp_path), "apple", "broken.png")
    with open(bad, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\nthis is not a png")
    with pytest.raises(Exception):
        list(DS.batches(DS.ImageFolder(str(tmp_path)), 4, False, 0))


def test_loader_functions_refuse_missing_directories(favit, tmp_path):
    DS = favit.datasets
    with pytest.raises(FileNotFoundError):
        DS.load_cifar10(str(tmp_path / "nope"), 32, 8)
    with pytest.raises(FileNotFoundError):
        DS.load_imagenet_subset(str(tmp_path / "nope"), 32, 8)
    (tmp_path / "train").mkdir()
    with pytest.raises(FileNotFoundError, match="train or validation"):
        DS.load_imagenet_subset(str(tmp_path), 32, 8)


def test_new_symbol_is_declared_bound_and_poisoned(favit):
    """favit_image_transform_ragged: in the header, in the ctypes table, exported, and tools/poison.py treats it as a
    launching call (its LDS poison kernel runs in front of it)."""
    import importlib.util
    name = "favit_image_transform_ragged"
    assert name in favit._abi.declared_symbols() and name in favit._abi._SIGS
    assert hasattr(favit._abi.lib(), name)
    assert len(favit._abi._SIGS[name][0]) == 13
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("favit_poison_tool", os.path.join(root, "tools", "poison.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert name not in mod._NO_LAUNCH and name.startswith("favit_")
    assert favit._abi.lib().favit_abi_version() == 8
