"""Host-side tests of the resumable training checkpoint (train.save_checkpoint / load_checkpoint) and of the state
dictionaries behind it: FusedAdamW (by parameter name), WarmupCosine, data.DeviceTransform, datasets.batches, the torch
CPU generator.  Nothing here launches a kernel: the optimizer's moments are filled by hand."""
import copy
import os

import numpy as np
import pytest
import torch


def _vit(favit, seed):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=4, use_mhla=True)


def _opt(favit, model, lr=1e-3, groups=None):
    T = favit.train
    return T.FusedAdamW(groups if groups is not None else T.param_groups(model, lr=lr, head_lr=4 * lr), lr=lr,
                        weight_decay=0.05, distributed=False)


def _fill(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for grp in opt.groups:
        grp["m"].copy_(torch.randn(grp["m"].shape, generator=g))
        grp["v"].copy_(torch.rand(grp["v"].shape, generator=g))


def _per_name(opt, model, key):
    """{parameter name: the slice of the group's flat `key` buffer}, read through the optimizer's own layout."""
    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    for grp in opt.groups:
        for p, o in zip(grp["flat"].params, grp["flat"].offsets):
            out[names[id(p)]] = grp[key][o:o + p.numel()].clone()
    return out


@pytest.fixture()
def saved(favit, tmp_path):
    """A tiny model, an optimizer with hand-filled moments at steps = 7, a stepped schedule, and their file."""
    T = favit.train
    model = _vit(favit, 11)
    opt = _opt(favit, model)
    _fill(opt, 1)
    opt.steps = 7
    sched = T.WarmupCosine(opt, 3, 20, min_ratio=0.1)
    for _ in range(7):
        sched.step()
    path = str(tmp_path / "state.pt")
    T.save_checkpoint(path, model, opt, sched, extra={"epoch": 2, "history": {"train_loss": [1.5, 1.25]}})
    return model, opt, sched, path


def test_format_and_round_trip(favit, saved):
    T = favit.train
    model, opt, sched, path = saved
    assert not os.path.exists(path + ".tmp")
    ck = torch.load(path, map_location="cpu", weights_only=True)          # no pickled class in the file
    assert ck["format"] == "favit-train-state" and ck["version"] == 1
    assert ck["compute_mode"] == favit.functional.get_compute_mode()
    assert list(ck["model"].keys()) == list(model.state_dict().keys())
    assert all(v.dtype == torch.float32 for v in ck["model"].values())
    assert set(ck["optimizer"]["state"].keys()) == {n for n, _ in model.named_parameters()}
    assert ck["rng"]["dropout_epoch"] is None or isinstance(ck["rng"]["dropout_epoch"], int)
    # state is keyed by name: a per-parameter tensor has the parameter's shape, whatever the flat layout pads
    for n, p in model.named_parameters():
        assert tuple(ck["optimizer"]["state"][n]["m"].shape) == tuple(p.shape)

    model2 = _vit(favit, 23)
    opt2 = _opt(favit, model2, lr=7e-2)
    _fill(opt2, 2)
    sched2 = T.WarmupCosine(opt2, 1, 5)
    assert not torch.equal(model2.head.weight, model.head.weight)
    extra = T.load_checkpoint(path, model2, opt2, sched2)
    assert extra == {"epoch": 2, "history": {"train_loss": [1.5, 1.25]}}
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    for key in ("m", "v"):
        a, b = _per_name(opt, model, key), _per_name(opt2, model2, key)
        assert a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a), key
    assert opt2.steps == 7 and opt2.ema_updates == 0
    assert [g["lr"] for g in opt2.groups] == [g["lr"] for g in opt.groups]
    assert sched2.t == sched.t and sched2.base_lrs == sched.base_lrs and sched2.last_lr == sched.last_lr
    # the parameters are still views of the optimizer's flat buffers (load_state_dict copies in place)
    for grp in opt2.groups:
        for p, o in zip(grp["flat"].params, grp["flat"].offsets):
            assert p.data_ptr() == grp["flat"].flat_p.data_ptr() + 4 * o


def _snapshot(model, opt):
    return ([v.clone() for v in model.state_dict().values()], [g["m"].clone() for g in opt.groups],
            [g["v"].clone() for g in opt.groups], opt.steps, [g["lr"] for g in opt.groups])


def _unchanged(model, opt, snap):
    now = _snapshot(model, opt)
    for a, b in zip(snap[:3], now[:3]):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert snap[3:] == now[3:]


def _rewrite(path, edit):
    ck = torch.load(path, map_location="cpu", weights_only=True)
    edit(ck)
    torch.save(ck, path)


def _rename(ck, old, new):
    ck["model"] = {(new if k == old else k): v for k, v in ck["model"].items()}
    ck["optimizer"]["state"] = {(new if k == old else k): v for k, v in ck["optimizer"]["state"].items()}
    for g in ck["optimizer"]["groups"]:
        g["names"] = [new if k == old else k for k in g["names"]]


def _reshape(ck, key):
    ck["model"][key] = ck["model"][key].reshape(-1)


def _reshape_moment(ck, key):
    ck["optimizer"]["state"][key]["v"] = ck["optimizer"]["state"][key]["v"].reshape(-1)[:-1].clone()


def _version(ck):
    ck["version"] = 2


@pytest.mark.parametrize("what", ["renamed_key", "wrong_shape", "wrong_moment_shape", "moved_group", "version",
                                  "ema_missing"])
def test_refusals_name_the_key_and_write_nothing(favit, saved, what):
    T = favit.train
    _, _, _, path = saved
    model2 = _vit(favit, 23)
    key = "head.weight"
    groups = None
    if what == "renamed_key":
        _rewrite(path, lambda ck: _rename(ck, key, "head.kernel"))
        needle = key
    elif what == "wrong_shape":
        _rewrite(path, lambda ck: _reshape(ck, key))
        needle = key
    elif what == "wrong_moment_shape":
        _rewrite(path, lambda ck: _reshape_moment(ck, key))
        needle = key
    elif what == "moved_group":
        # the optimizer that loads keeps head.bias with the body's parameters; the file has it in the head's group
        groups = T.param_groups(model2, lr=1e-3, head_lr=4e-3)
        moved = groups[-1]["params"].pop()
        assert moved is model2.head.bias
        groups[0]["params"].append(moved)
        needle = "head.bias"
    elif what == "version":
        _rewrite(path, _version)
        needle = "version"
    else:
        needle = "ema"
    opt2 = _opt(favit, model2, groups=groups)
    _fill(opt2, 2)
    if what == "ema_missing":
        # (an optimizer with an average lives on the GPU; its host-side bookkeeping is staged by hand, like m and v)
        opt2.ema_decay = 0.99
        for g in opt2.groups:
            g["ema"] = g["flat"].flat_p.clone()
    snap = _snapshot(model2, opt2)
    rng = torch.get_rng_state()
    with pytest.raises(ValueError) as e:
        T.load_checkpoint(path, model2, opt2)
    print(e.value)
    assert needle in str(e.value)
    _unchanged(model2, opt2, snap)
    assert torch.equal(rng, torch.get_rng_state())


def test_schedule_and_format_refusals(favit, saved, tmp_path):
    T = favit.train
    model, opt, sched, path = saved
    model2 = _vit(favit, 23)
    opt2 = _opt(favit, model2, groups=[{"params": list(model2.parameters())}])       # one group: the file has more
    snap = _snapshot(model2, opt2)
    with pytest.raises(ValueError, match="groups"):
        T.load_checkpoint(path, model2, opt2)
    _unchanged(model2, opt2, snap)
    other = str(tmp_path / "other.pt")
    torch.save({"format": "something-else", "version": 1}, other)
    with pytest.raises(ValueError, match="format"):
        T.load_checkpoint(other, model2)
    with pytest.raises(ValueError, match="use_ema"):
        T.load_checkpoint(path, model2, use_ema=True)                      # the file's optimizer kept no average
    with pytest.warns(UserWarning, match="compute mode"):
        _rewrite(path, lambda ck: ck.__setitem__("compute_mode", "fp8"))
        T.load_checkpoint(path, model2)
    assert torch.equal(model2.head.weight, model.head.weight)


def _write_cifar_test_batch(root, n, seed):
    rs = np.random.RandomState(seed)
    rec = rs.randint(0, 256, size=(n, 1 + 3 * 32 * 32)).astype(np.uint8)
    rec[:, 0] = np.arange(n) % 10
    rec.tofile(os.path.join(root, "test_batch.bin"))


def test_transform_and_batches_round_trip(favit, tmp_path):
    T, D, DS = favit.train, favit.data, favit.datasets
    _write_cifar_test_batch(str(tmp_path), 64, 0)
    ds = DS.Cifar10Binary(str(tmp_path), train=False)
    model = _vit(favit, 11)

    def order(b):
        return np.concatenate([y for _, y in b])

    tf = D.DeviceTransform("cifar10_train", 32, D.CIFAR10_MEAN, D.CIFAR10_STD, seed=3)
    bt = DS.batches(ds, 8, True, seed=5)
    tf.params(8, 32, 32)
    tf.rng.randn()                       # (leaves a cached gaussian in the generator: part of its state)
    first = order(bt)
    path = str(tmp_path / "loaders.pt")
    T.save_checkpoint(path, model, loaders=[tf, bt])
    torch.load(path, map_location="cpu", weights_only=True)
    want_p, want_g, want_o = tf.params(8, 32, 32), tf.rng.randn(), order(bt)
    assert not np.array_equal(want_o, first)

    tf2 = D.DeviceTransform("cifar10_train", 32, D.CIFAR10_MEAN, D.CIFAR10_STD, seed=77)
    bt2 = DS.batches(ds, 8, True, seed=5)
    T.load_checkpoint(path, model, loaders=[tf2, bt2])
    assert np.array_equal(tf2.params(8, 32, 32), want_p) and tf2.rng.randn() == want_g
    assert bt2.epoch == 1 and np.array_equal(order(bt2), want_o)
    # the wrong number of loaders, another transform kind and another shuffle seed are refused
    with pytest.raises(ValueError, match="loaders"):
        T.load_checkpoint(path, model, loaders=[tf2])
    with pytest.raises(ValueError, match="kind"):
        T.load_checkpoint(path, model, loaders=[D.DeviceTransform("resize", 32, D.CIFAR10_MEAN, D.CIFAR10_STD), bt2])
    with pytest.raises(ValueError, match="seed"):
        T.load_checkpoint(path, model, loaders=[tf2, DS.batches(ds, 8, True, seed=6)])


def test_torch_cpu_generator_is_restored(favit, tmp_path):
    T = favit.train
    model = _vit(favit, 11)
    torch.manual_seed(1234)
    torch.randint(0, 1 << 30, (5,))
    path = str(tmp_path / "rng.pt")
    T.save_checkpoint(path, model)
    want = torch.randint(0, 1 << 30, (5,))
    torch.manual_seed(99)
    T.load_checkpoint(path, _vit(favit, 23))              # (building a model draws from the generator as well)
    assert torch.equal(torch.randint(0, 1 << 30, (5,)), want)


def test_ema_decay_at(favit):
    f = favit.train.ema_decay_at
    for d in (0.0, 0.5, 0.9999):
        for n in (0, 1, 90, 10 ** 6):
            assert f(d, n, False) == d and f(d, n) == d
            assert f(d, n, True) == min(d, (1 + n) / (10 + n))
    assert f(0.9999, 0, True) == 0.1 and f(0.9999, 1, True) == 2 / 11 and f(0.9999, 90, True) == 0.91
    assert f(0.9999, 10 ** 6, True) == 0.9999


def test_failed_save_keeps_the_previous_file(favit, saved, monkeypatch):
    T = favit.train
    model, opt, sched, path = saved
    before = copy.deepcopy(torch.load(path, map_location="cpu", weights_only=True))
    real = torch.save

    def broken(obj, f, *a, **kw):
        with open(f, "wb") as fh:                          # a partial file, then the failure
            fh.write(b"partial")
        raise OSError("disk full")

    with torch.no_grad():
        model.head.weight.add_(1.0)
    monkeypatch.setattr(torch, "save", broken)
    with pytest.raises(OSError, match="disk full"):
        T.save_checkpoint(path, model, opt, sched)
    monkeypatch.setattr(torch, "save", real)
    assert not os.path.exists(path + ".tmp")
    after = torch.load(path, map_location="cpu", weights_only=True)
    assert all(torch.equal(after["model"][k], before["model"][k]) for k in before["model"])
    model2 = _vit(favit, 23)
    T.load_checkpoint(path, model2, _opt(favit, model2))
    assert not torch.equal(model2.head.weight, model.head.weight)


def test_optimizer_options_that_need_kernels_refuse_cpu_parameters(favit):
    model = _vit(favit, 11)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        favit.train.FusedAdamW(model, distributed=False, ema_decay=0.99)
    with pytest.raises(ValueError, match="ema_decay"):
        favit.train.FusedAdamW(_vit(favit, 11), distributed=False, ema_decay=1.0)
    opt = favit.train.FusedAdamW(_vit(favit, 11), distributed=False)
    with pytest.raises(RuntimeError, match="no average"):
        with opt.ema_weights():
            pass


def test_abi_additions_are_declared_and_the_version_stays(favit):
    sig, declared = favit._abi._SIGS, favit._abi.declared_symbols()
    for name in ("favit_adamw_ema", "favit_adamw_clip_ema", "favit_swap_params"):
        assert name in declared and name in sig
    # the EMA entry points take their twins' arguments plus the buffer (after p_bf16) and the decay (before the stream)
    for twin in ("favit_adamw", "favit_adamw_clip"):
        a, e = sig[twin][0], sig[twin + "_ema"][0]
        assert len(e) == len(a) + 2 and e[:5] == a[:5] and e[6:-2] == a[5:-1]
    with open(favit._abi.HEADER_PATH) as f:
        assert "#define FAVIT_ABI_VERSION 8" in f.read()
