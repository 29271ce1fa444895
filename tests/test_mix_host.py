"""Host-side checks (no GPU) of batch mixing: BatchMix's draws, their invariants and checkpoint state, argument
validation, the two C ABI additions (favit_batch_mix, favit_cross_entropy_mix) and the loader's unchanged state."""
import re

import numpy as np
import pytest
import torch

S = 32


def _is_cutmix(box):
    return (box[:, 1] > box[:, 0]) & (box[:, 3] > box[:, 2])


def test_params_are_reproducible_by_seed(favit):
    D = favit.data
    a, b, c = D.BatchMix(seed=5, mode="elem"), D.BatchMix(seed=5, mode="elem"), D.BatchMix(seed=6, mode="elem")
    differs = False
    for _ in range(4):
        la, ba = a.params(9, S)
        lb, bb = b.params(9, S)
        lc, bc = c.params(9, S)
        assert la.dtype == np.float32 and ba.dtype == np.int32 and la.shape == (9,) and ba.shape == (9, 4)
        assert np.array_equal(la, lb) and np.array_equal(ba, bb)
        differs |= not (np.array_equal(la, lc) and np.array_equal(ba, bc))
    assert differs, "another seed gives another stream"


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_state_dict_round_trip_continues_the_stream(favit, mode):
    D = favit.data
    a = D.BatchMix(seed=3, mode=mode)
    for _ in range(3):
        a.params(8, S)
    state = a.state_dict()
    want = [a.params(8, S) for _ in range(3)]
    b = D.BatchMix(seed=99, mode=mode)
    b.load_state_dict(state)
    for lw, bw in want:
        lg, bg = b.params(8, S)
        assert np.array_equal(lw, lg) and np.array_equal(bw, bg)


@pytest.mark.parametrize("mode", ["batch", "elem"])
@pytest.mark.parametrize("B", [8, 7, 1])
def test_parameter_invariants(favit, mode, B):
    mix = favit.data.BatchMix(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5, mode=mode, seed=B)
    seen_cut = seen_mix = seen_plain = 0
    for _ in range(60):
        lam, box = mix.params(B, S)
        assert np.all(lam >= 0.0) and np.all(lam <= 1.0)
        cut = _is_cutmix(box)
        # CutMix rows: a box inside the image and lam = 1 - area / S^2; every other row: a zero box
        assert np.all(box[cut] >= 0) and np.all(box[cut] <= S)
        area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
        assert np.array_equal(lam[cut], (1.0 - area[cut] / float(S * S)).astype(np.float32))
        assert np.all(box[~cut] == 0)
        if B % 2:                                    # the middle row of an odd batch is its own partner
            assert lam[B // 2] == 1.0 and np.all(box[B // 2] == 0)
        if mode == "batch":
            rows = [b for b in range(B) if not (B % 2 and b == B // 2)]
            assert all(lam[b] == lam[rows[0]] and np.array_equal(box[b], box[rows[0]]) for b in rows)
        seen_cut += int(cut.sum())
        seen_mix += int(((~cut) & (lam < 1.0)).sum())
        seen_plain += int(((~cut) & (lam == 1.0)).sum())
    if B > 1:
        assert seen_cut and seen_mix and seen_plain, "all three kinds of row occur at prob 0.8 / switch 0.5"
    else:
        assert seen_cut == 0 and seen_mix == 0


def test_single_alpha_selects_the_one_kind(favit):
    D = favit.data
    only_mixup, only_cutmix = D.BatchMix(0.8, 0.0, mode="elem", seed=1), D.BatchMix(0.0, 1.0, mode="elem", seed=1)
    for _ in range(10):
        lam, box = only_mixup.params(8, S)
        assert np.all(box == 0)
        lam, box = only_cutmix.params(8, S)
        assert np.all(_is_cutmix(box) | (lam == 1.0))            # (a box clipped to nothing leaves the row alone)


def test_prob_zero_leaves_every_row_unchanged(favit):
    for mode in ("batch", "elem"):
        mix = favit.data.BatchMix(prob=0.0, mode=mode, seed=2)
        for _ in range(5):
            lam, box = mix.params(6, S)
            assert np.all(lam == 1.0) and np.all(box == 0)


@pytest.mark.parametrize("kw", [dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=0.0, cutmix_alpha=0.0),
                                dict(prob=1.5), dict(prob=-0.1), dict(switch_prob=2.0), dict(mode="pair")])
def test_constructor_validation(favit, kw):
    with pytest.raises(ValueError):
        favit.data.BatchMix(**kw)


def test_state_validation(favit):
    D = favit.data
    mix = D.BatchMix(seed=0)
    good = mix.state_dict()
    mix.check_state_dict(good)
    for k in ("bit_generator", "keys", "pos", "has_gauss", "cached_gaussian"):
        bad = {q: v for q, v in good.items() if q != k}
        with pytest.raises(ValueError, match=k):
            mix.load_state_dict(bad)
    with pytest.raises(ValueError, match="keys"):
        mix.load_state_dict(dict(good, keys=good["keys"][:100]))
    with pytest.raises(ValueError, match="mode"):
        D.BatchMix(mode="elem").load_state_dict(good)


def test_kernel_wrappers_validate_on_the_host(favit):
    K = favit.kernels
    x, lam, box = torch.zeros(2, 3, 4, 4), torch.ones(2), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.batch_mix(x, lam, box)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), mix_lam=torch.ones(2))
    with pytest.raises(ValueError):
        K.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), label_smoothing=1.0, mix_lam=torch.ones(2))


def test_entry_points_are_declared_exported_and_bound(favit):
    lib, sig = favit._abi.lib(), favit._abi._SIGS
    declared = favit._abi.declared_symbols()
    with open(favit._abi.HEADER_PATH) as f:
        header = f.read()
    for name, arity in (("favit_batch_mix", 8), ("favit_cross_entropy_mix", 10)):
        assert name in declared, f"{name} is not declared in include/favit.h"
        assert hasattr(lib, name), f"libfavit.so does not export {name}"
        assert len(sig[name][0]) == arity
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl and len(decl.group(1).split(",")) == arity, f"{name}: the header declares another arity"
    assert lib.favit_abi_version() == 8, "the additions are additive: the ABI version stays"
    # the mixed loss takes favit_cross_entropy_ls's arguments with `lam` after the labels
    ls, mx = sig["favit_cross_entropy_ls"][0], sig["favit_cross_entropy_mix"][0]
    assert mx[:2] == ls[:2] and mx[3:] == ls[2:]


class _Src:
    def __iter__(self):
        return iter(())

    def __len__(self):
        return 0


class _Tf:
    def state_dict(self):
        return {"kind": "resize"}

    def check_state_dict(self, state):
        pass

    def load_state_dict(self, state):
        pass


def _loader(favit, mix):
    """A DeviceLoader without a device: only its state handling is exercised."""
    L = favit.data.DeviceLoader.__new__(favit.data.DeviceLoader)
    L.src, L.tf, L.mix = _Src(), _Tf(), mix
    return L


def test_loader_state_without_mix_is_unchanged_and_presence_must_match(favit):
    plain, mixed = _loader(favit, None), _loader(favit, favit.data.BatchMix(seed=4))
    assert set(plain.state_dict().keys()) == {"transform", "batches"}
    assert set(mixed.state_dict().keys()) == {"transform", "batches", "mix"}
    plain.load_state_dict(plain.state_dict())
    mixed.load_state_dict(mixed.state_dict())
    with pytest.raises(ValueError, match="mix"):
        plain.load_state_dict(mixed.state_dict())
    with pytest.raises(ValueError, match="mix"):
        mixed.load_state_dict(plain.state_dict())


def test_experiment_tool_flags_default_to_off(favit):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("favit_run_experiment", os.path.join(root, "tools", "run_experiment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--experiment", "mhla"])
    assert a.mixup_alpha == 0.0 and a.cutmix_alpha == 0.0 and a.mix_prob == 1.0 and a.mix_switch_prob == 0.5
    assert a.mix_mode == "batch"
    b = tool.parse_args(["--experiment", "mhla", "--mixup_alpha", "0.8", "--cutmix_alpha", "1.0", "--mix_prob", "0.5",
                         "--mix_switch_prob", "0.25", "--mix_mode", "elem"])
    assert (b.mixup_alpha, b.cutmix_alpha, b.mix_prob, b.mix_switch_prob, b.mix_mode) == (0.8, 1.0, 0.5, 0.25, "elem")
