"""Ragged device transform (favit_image_transform_ragged), ragged batches through DeviceTransform / DeviceLoader, the
on-disk readers end to end, and the experiment runner's --data_dir / *_pretrained branches, on the GPU.

The standard is the one of tests/test_data_pipeline.py: Pillow is the checker, the resized bytes are compared with
assert_array_equal and the fp32 output with torch.equal -- no tolerance anywhere in this file.
"""
import csv
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from test_datasets_host import write_cifar, write_image_tree

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(32, 32), (37, 53), (180, 240), (375, 500), (500, 333), (64, 48), (224, 224), (40, 200), (1200, 1600)]


def _pil_pipeline(img_u8, top, left, ch, cw, pad, rh, rw, oy, ox, S, flip_src, flip_out, mean, std):
    """crop (of the zero-padded image) -> flip -> PIL bilinear resize -> window -> flip -> ToTensor -> Normalize
    (the construction of tests/test_data_pipeline.py, restated)"""
    H, W, C = img_u8.shape
    padded = np.zeros((H + 2 * pad, W + 2 * pad, C), dtype=np.uint8)
    padded[pad:pad + H, pad:pad + W] = img_u8
    crop = padded[top:top + ch, left:left + cw]
    if flip_src:
        crop = crop[:, ::-1]
    res = np.asarray(Image.fromarray(np.ascontiguousarray(crop)).resize((rw, rh), Image.BILINEAR))
    win = res[oy:oy + S, ox:ox + S]
    if flip_out:
        win = win[:, ::-1]
    t = torch.from_numpy(np.ascontiguousarray(win)).permute(2, 0, 1).float().div(255)
    m, s = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)
    return np.ascontiguousarray(win), (t - m) / s


def _check_against_pillow(imgs, prm, S, out, u8, mean, std):
    out, u8 = out.cpu(), u8.cpu().numpy()
    assert tuple(out.shape) == (len(imgs), 3, S, S) and out.dtype == torch.float32 and u8.shape == (len(imgs), S, S, 3)
    for b, im in enumerate(imgs):
        top, left, ch, cw, pad, rh, rw, oy, ox, fs, fo, _ = [int(v) for v in prm[b]]
        ref_u8, ref_f = _pil_pipeline(im, top, left, ch, cw, pad, rh, rw, oy, ox, S, fs, fo, mean, std)
        np.testing.assert_array_equal(u8[b], ref_u8, err_msg=f"image {b} {im.shape}")      # byte work: bit-exact
        assert torch.equal(out[b], ref_f), (b, im.shape, (out[b] - ref_f).abs().max())     # same fp32 operations as torch


def _images(sizes, seed):
    rs = np.random.RandomState(seed)
    imgs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    h, w = sizes[0]
    imgs[0] = np.ascontiguousarray(np.broadcast_to((np.add.outer(np.arange(h), np.arange(w))[:, :, None] * 3 % 256), (h, w, 3)).astype(np.uint8))
    return imgs


@pytest.mark.gpu
@pytest.mark.parametrize("S", [224, 64])
@pytest.mark.parametrize("kind", ["imagenet_test", "imagenet_train"])
def test_ragged_transform_is_bit_identical_to_pillow(favit, kind, S):
    D = favit.data
    imgs = _images(SIZES, seed=S + len(kind))
    rb = D.RaggedBatch.from_images(imgs)
    tf = D.DeviceTransform(kind, S, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=3)
    prm = tf.params(len(imgs), rb.heights, rb.widths)
    out, u8 = tf(rb.to(DEV), params=prm, want_bytes=True)
    _check_against_pillow(imgs, prm, S, out, u8, D.IMAGENET_MEAN, D.IMAGENET_STD)
    # without explicit rows the transform draws them from each image's own size; the plain call returns the tensor only
    tf2 = D.DeviceTransform(kind, S, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=3)
    again = tf2(rb.to(DEV))
    assert torch.is_tensor(again) and torch.equal(again, out)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [0, 1])
def test_ragged_crop_beyond_an_image_reads_zero_padding_not_the_neighbour(favit, flip):
    """A cifar10_train-style padded crop that reaches past the image's edges: the packed buffer continues with an
    all-255 neighbour (and starts with one), the result must be Pillow's on the ZERO-padded image."""
    D = favit.data
    rs = np.random.RandomState(4)
    white = np.full((32, 32, 3), 255, dtype=np.uint8)
    img = rs.randint(1, 256, size=(32, 32, 3), dtype=np.uint8)
    imgs = [white, img, white, rs.randint(1, 256, size=(24, 40, 3), dtype=np.uint8), white]
    S = 64
    prm = np.zeros((5, 12), dtype=np.int32)
    prm[:, 2], prm[:, 3], prm[:, 4], prm[:, 5], prm[:, 6], prm[:, 9] = 32, 32, 4, S, S, flip
    # crop origins inside the padded image (the Pillow construction slices it): bottom/right overhang, top/left overhang,
    # and for the 24x40 image (padded 32x48) rows -4..27 and columns 12..43: above, below and right of it
    prm[:, 0], prm[:, 1] = [8, 8, 0, 0, 4], [8, 8, 0, 16, 4]
    tf = D.DeviceTransform("cifar10_train", S, D.CIFAR10_MEAN, D.CIFAR10_STD)
    out, u8 = tf(D.RaggedBatch.from_images(imgs).to(DEV), params=prm, want_bytes=True)
    _check_against_pillow(imgs, prm, S, out, u8, D.CIFAR10_MEAN, D.CIFAR10_STD)
    assert (u8[1, -4:, :, :] == 0).all().item() and (u8[1, :, (slice(0, 4) if flip else slice(-4, None)), :] == 0).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H,W,S", [("imagenet_train", 48, 64, 96), ("cifar10_train", 32, 32, 64), ("imagenet_test", 375, 500, 224)])
def test_ragged_and_uniform_entries_agree_on_a_uniform_batch(favit, kind, H, W, S):
    D = favit.data
    rs = np.random.RandomState(6)
    x = rs.randint(0, 256, size=(6, H, W, 3), dtype=np.uint8)
    tf = D.DeviceTransform(kind, S, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=2)
    prm = tf.params(6, H, W)
    a, a8 = tf(torch.from_numpy(x).to(DEV), params=prm, want_bytes=True)
    b, b8 = tf(D.RaggedBatch.from_images(list(x)).to(DEV), params=prm, want_bytes=True)
    assert torch.equal(a, b) and torch.equal(a8, b8)


@pytest.mark.gpu
def test_ragged_descriptor_beyond_the_buffer_is_refused_before_any_launch(favit):
    D = favit.data
    imgs = _images([(20, 30), (16, 16), (9, 50)], seed=8)
    tf = D.DeviceTransform("imagenet_test", 32, D.IMAGENET_MEAN, D.IMAGENET_STD)
    calls = []
    real = favit._abi.lib().favit_image_transform_ragged

    class Spy:                                          # stands in front of the library: any launch would be recorded
        def __getattr__(self, name):
            if name == "favit_image_transform_ragged":
                return lambda *a: (calls.append(a), real(*a))[1]
            return getattr(saved, name)
    saved = favit._abi._lib
    favit._abi._lib = Spy()
    try:
        for corrupt in ("heights", "widths", "offsets"):
            rb = D.RaggedBatch.from_images(imgs).to(DEV)
            getattr(rb, corrupt)[2] += 7
            with pytest.raises(ValueError, match="image 2"):
                tf(rb)
        rb = D.RaggedBatch.from_images(imgs).to(DEV)
        rb.offsets[0] = -1
        with pytest.raises(ValueError, match="image 0"):
            tf(rb)
        assert calls == []
        tf(D.RaggedBatch.from_images(imgs).to(DEV))
        assert len(calls) == 1
    finally:
        favit._abi._lib = saved
    with pytest.raises(RuntimeError):                   # bytes still on the host
        tf(D.RaggedBatch.from_images(imgs))


@pytest.mark.gpu
def test_device_loader_ragged_batches_staging_grows_and_short_batch_passes(favit):
    D = favit.data
    sizes = [[(40, 30)] * 4, [(64, 48), (375, 500), (33, 47), (90, 20)], [(500, 333), (224, 224), (37, 53), (180, 240)],
             [(32, 32)] * 4, [(120, 160), (48, 64)]]
    host = []
    for k, sz in enumerate(sizes):
        imgs = _images(sz, seed=20 + k)
        host.append((imgs, D.RaggedBatch.from_images(imgs), np.arange(len(sz)) + 10 * k))
    S = 64
    tf = D.DeviceTransform("imagenet_test", S, D.IMAGENET_MEAN, D.IMAGENET_STD)
    loader = D.DeviceLoader([(rb, y) for _, rb, y in host], tf)
    assert len(loader) == 5
    caps, n = [], 0
    for (x, y), (imgs, rb, hy) in zip(loader, host):
        assert x.is_cuda and tuple(x.shape) == (len(imgs), 3, S, S) and y.dtype == torch.int64
        assert torch.equal(y.cpu(), torch.from_numpy(hy))
        prm = tf.params(len(imgs), rb.heights, rb.widths)
        for b, im in enumerate(imgs):
            ref = _pil_pipeline(im, *[int(v) for v in prm[b][:9]], S, 0, 0, D.IMAGENET_MEAN, D.IMAGENET_STD)[1]
            assert torch.equal(x[b].cpu(), ref)
        caps.append(tuple(None if p is None else p[0].numel() for p in loader._pin_ragged))
        n += 1
    assert n == 5
    # one pinned staging buffer per slot, grown to the largest batch that slot has seen, never shrunk or re-made for a
    # smaller batch (slot 0 stages batches 0, 2, 4; slot 1 batches 1, 3)
    big0, big1 = host[2][1].bytes.numel(), host[1][1].bytes.numel()
    assert caps[-1] == (big0, big1)
    assert all(p[0].is_pinned() for p in loader._pin_ragged)
    ptrs = [p[0].data_ptr() for p in loader._pin_ragged]
    for _ in loader:                                     # a second epoch: nothing grows, so nothing is allocated
        pass
    assert [p[0].data_ptr() for p in loader._pin_ragged] == ptrs


@pytest.mark.gpu
def test_load_imagenet_subset_end_to_end(favit, tmp_path):
    D, DS = favit.data, favit.datasets
    want = write_image_tree(str(tmp_path / "val"), seed=1)
    write_image_tree(str(tmp_path / "train"), seed=2)
    S = 64
    d = DS.load_imagenet_subset(str(tmp_path), img_size=S, batch_size=3, num_workers=4)
    assert d["num_classes"] == 3 and d["idx_to_class"] == {0: "apple", 1: "mango", 2: "zebra"}
    assert isinstance(d["val_loader"], D.DeviceLoader) and isinstance(d["train_loader"], D.DeviceLoader)
    assert len(d["val_loader"]) == 3 and len(d["train_loader"]) == 3
    tf = D.DeviceTransform("imagenet_test", S, D.IMAGENET_MEAN, D.IMAGENET_STD)
    xs, ys = [], []
    for x, y in d["val_loader"]:
        xs.append(x.cpu())
        ys.append(y.cpu())
    assert [len(y) for y in ys] == [3, 3, 1]                      # the short last batch passes through
    x, y = torch.cat(xs), torch.cat(ys)
    assert y.tolist() == [t for _, t in want]
    for i, (path, _) in enumerate(want):
        im = np.asarray(Image.open(path).convert("RGB"))
        p = [int(v) for v in tf.params(1, im.shape[0], im.shape[1])[0]]
        ref = _pil_pipeline(im, *p[:9], S, p[9], p[10], D.IMAGENET_MEAN, D.IMAGENET_STD)[1]
        assert torch.equal(x[i], ref), path
    seen = 0
    for x, y in d["train_loader"]:                                # RandomResizedCrop on ragged input: shapes and labels
        assert tuple(x.shape[1:]) == (3, S, S) and bool(torch.isfinite(x).all()) and int(y.max()) <= 2
        seen += len(y)
    assert seen == 7
    sub = DS.load_imagenet_subset(str(tmp_path), img_size=S, batch_size=2, subset_size=5)
    assert len(sub["train_dataset"]) == 5 and len(sub["val_dataset"]) == 1 and sub["num_classes"] == 3


@pytest.mark.gpu
def test_load_cifar10_end_to_end(favit, tmp_path):
    D, DS = favit.data, favit.datasets
    want = write_cifar(str(tmp_path / "cifar-10-batches-bin"), n_per_file=40)
    S = 64
    d = DS.load_cifar10(str(tmp_path), img_size=S, batch_size=16)
    assert d["num_classes"] == 10 and d["class_names"][0] == "airplane" and len(d["test_loader"]) == 3
    tf = D.DeviceTransform("resize", S, D.CIFAR10_MEAN, D.CIFAR10_STD)
    x = torch.cat([xb for xb, _ in d["test_loader"]])
    y = torch.cat([yb for _, yb in d["test_loader"]])
    assert torch.equal(x, tf(torch.from_numpy(want["test"][0]).to(DEV)))
    assert torch.equal(y.cpu(), torch.from_numpy(want["test"][1]))
    n = sum(len(yb) for xb, yb in d["train_loader"] if tuple(xb.shape[1:]) == (3, S, S))
    assert n == 200
    sub = DS.load_cifar10(str(tmp_path), img_size=S, batch_size=16, subset_size=50)
    assert len(sub["train_dataset"]) == 50 and len(sub["test_dataset"]) == 10


@pytest.mark.gpu
def test_device_loader_prefetches_label_maps_for_ragged_batches(favit):
    """DeviceLoader(segmenter=...) with ragged input: the maps installed with each yielded batch are those of
    segmenting the yielded images directly (the uniform case is in tests/test_data_pipeline.py)."""
    D = favit.data
    rs = np.random.RandomState(3)
    host = []
    for k in range(4):
        imgs = [np.kron(rs.randint(0, 256, size=(7, 7, 3), dtype=np.uint8), np.ones((c, c, 1), dtype=np.uint8))
                for c in (8, 10, 6, 12, 8, 9)[: 6 if k < 3 else 3]]           # blocky squares of 56, 70, 42, 84, ... pixels
        host.append((D.RaggedBatch.from_images(imgs), rs.randint(0, 10, size=len(imgs))))
    tf = D.DeviceTransform("resize", 64, D.CIFAR10_MEAN, D.CIFAR10_STD)
    seg = favit.models.sppp.SuperpixelSegmentation(num_segments=16, compactness=10.0)
    loader = D.DeviceLoader(host, tf, segmenter=seg)
    n = 0
    torch.cuda.synchronize()
    with torch.cuda.stream(loader.compute_stream):
        for (x, y), (rb, hl) in zip(loader, host):
            ref_x = tf(rb.to(DEV))
            assert torch.equal(x, ref_x) and torch.equal(y.cpu(), torch.from_numpy(hl))
            got = seg.segment(x)
            _ = (x @ x.transpose(-1, -2)).sum()
            want = seg.segment_device(x)
            assert got.dtype == torch.int64 and tuple(got.shape) == (len(rb), 64, 64)
            assert torch.equal(got, want)
            n += 1
    torch.cuda.synchronize()
    assert n == 4
    seg.set_label_maps(None)


def _tool():
    spec = importlib.util.spec_from_file_location("favit_run_experiment", os.path.join(ROOT, "tools", "run_experiment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_run_experiment_trains_from_a_cifar10_directory(tmp_path):
    write_cifar(str(tmp_path / "data"), n_per_file=64)            # 320 train, 64 test records
    res = tmp_path / "results"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_experiment.py"), "--experiment", "mhla", "--dataset", "cifar10",
           "--data_dir", str(tmp_path / "data"), "--img_size", "32", "--patch_size", "4", "--embed_dim", "64", "--depth", "2",
           "--num_heads", "4", "--epochs", "1", "--batch_size", "64", "--results_dir", str(res)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    with open(res / "exp_mhla.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1 and rows[0]["model"] == "mhla" and np.isfinite(float(rows[0]["test_loss"]))
    assert 0.0 <= float(rows[0]["test_acc"]) <= 100.0


@pytest.mark.gpu
@pytest.mark.parametrize("experiment", ["mhla_pretrained", "sppp_mhla_pretrained"])
def test_pretrained_experiments_freeze_everything_but_head_and_latent_proj(favit, tmp_path, experiment):
    """Two optimizer steps with --freeze_layers: exactly the parameters named head* / *latent_proj* moved; the archive's
    tensors were loaded, keys it lacks stayed as initialised, every latent_proj started as the identity."""
    tool = _tool()
    favit.set_compute_dtype("fp32")
    try:
        sppp = experiment.startswith("sppp")
        argv = ["--experiment", experiment, "--img_size", "64", "--patch_size", "8", "--embed_dim", "64", "--depth", "2",
                "--num_heads", "4", "--window_size", "3", "--num_superpixels", "4", "--compactness", "10", "--dropout", "0",
                "--freeze_layers"]
        a = tool.parse_args(argv)
        torch.manual_seed(a.seed)
        fresh = {k: v.clone() for k, v in tool.build_model(favit, a, 10).state_dict().items()}
        torch.manual_seed(a.seed)
        model = tool.build_model(favit, a, 10)
        assert all(torch.equal(v, fresh[k]) for k, v in model.state_dict().items())        # built seeded
        rs = np.random.RandomState(0)
        arc = {"norm.weight": rs.rand(64).astype(np.float32) + 0.5,
               "blocks.0.attn.qkv.weight": (rs.randn(192, 64) * 0.05).astype(np.float32),
               "blocks.1.attn.latent_proj.weight": rs.randn(16, 16).astype(np.float32),   # overridden by the identity
               "not.in.the.model": np.zeros(3, dtype=np.float32)}
        path = str(tmp_path / "w.npz")
        np.savez(path, **arc)
        loaded = tool.prepare_pretrained(model, path, a.freeze_layers)
        assert sorted(loaded) == sorted(k for k in arc if k != "not.in.the.model")
        sd = model.state_dict()
        for k in sd:
            if "latent_proj.weight" in k:
                assert torch.equal(sd[k], torch.eye(16))
            elif "latent_proj.bias" in k:
                assert not sd[k].any()
            elif k in arc:
                assert torch.equal(sd[k], torch.from_numpy(arc[k]))
            else:
                assert torch.equal(sd[k], fresh[k]), k                                     # missing from the archive
        trainable = {n for n, p in model.named_parameters() if p.requires_grad}
        assert trainable == {n for n, _ in model.named_parameters() if "head" in n or "latent_proj" in n} and trainable
        model = model.to(DEV).train()
        if sppp:
            model.assume_num_tokens = 4
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        opt = favit.train.FusedAdamW(favit.train.param_groups(model, lr=1e-2, head_lr=1e-2), lr=1e-2, weight_decay=0.05,
                                     distributed=False)
        assert len(opt.groups) == 2                                                        # 5x latent_proj group, head group
        assert sorted(g["lr"] for g in opt.groups) == pytest.approx([1e-2, 5e-2])
        tf = favit.data.DeviceTransform("resize", 64, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        for _ in range(2):
            # 2 x 2 blocks of flat colour: SLIC finds exactly the four quadrants (4 superpixel tokens per image)
            q = rs.randint(30, 226, size=(8, 2, 2, 3)).astype(np.uint8)
            x = tf(torch.from_numpy(np.kron(q, np.ones((1, 32, 32, 1), dtype=np.uint8))).to(DEV))
            y = torch.from_numpy(rs.randint(0, 10, size=8)).to(DEV)
            loss = favit.train.train_step(model, x, y, opt)
        assert np.isfinite(loss.item())
        for n, p in model.named_parameters():
            if n in trainable:
                assert not torch.equal(p.detach(), before[n]), f"{n} did not train"
            else:
                assert torch.equal(p.detach(), before[n]), f"frozen parameter {n} changed"
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
