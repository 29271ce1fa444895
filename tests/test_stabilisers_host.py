"""Host-side checks (no GPU) of the training stabilisers: the C ABI additions (favit_grad_norm, favit_adamw_clip,
favit_cross_entropy_ls), FusedAdamW's argument validation, the WarmupCosine schedule and the experiment tool's flags."""
import importlib.util
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("favit_grad_norm", "favit_grad_norm_workspace", "favit_adamw_clip", "favit_cross_entropy_ls")


def test_new_entry_points_are_declared_exported_and_bound(favit):
    lib = favit._abi.lib()
    declared = favit._abi.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/favit.h"
        assert hasattr(lib, s), f"libfavit.so does not export {s}"
        assert s in favit._abi._SIGS, f"{s} has no ctypes signature"
    assert lib.favit_abi_version() == 8, "the additions are additive: the ABI version stays"
    # plain favit_adamw / favit_cross_entropy keep their signatures; the new ones append their arguments to them
    sig = favit._abi._SIGS
    assert sig["favit_adamw_clip"][0][:14] == sig["favit_adamw"][0][:14] and len(sig["favit_adamw_clip"][0]) == 17
    assert sig["favit_cross_entropy_ls"][0][:7] == sig["favit_cross_entropy"][0][:7]
    ws = lib.favit_grad_norm_workspace()
    assert ws > 0 and ws % 8 == 0


def test_workspace_query_is_known_to_the_poison_tool():
    spec = importlib.util.spec_from_file_location("favit_poison_tool", os.path.join(ROOT, "tools", "poison.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "favit_grad_norm_workspace" in mod._NO_LAUNCH


def _groups(n):
    return [{"params": [torch.nn.Parameter(torch.zeros(3))]} for _ in range(n)]


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_fused_adamw_rejects_a_non_positive_max_grad_norm(favit, bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        favit.train.FusedAdamW(_groups(1), distributed=False, max_grad_norm=bad)


@pytest.mark.parametrize("kw", [{"max_grad_norm": 1.0}, {"skip_nonfinite": True}])
def test_fused_adamw_rejects_more_than_16_groups_with_either_option(favit, kw):
    with pytest.raises(ValueError, match="16"):
        favit.train.FusedAdamW(_groups(17), distributed=False, **kw)


def test_fused_adamw_defaults_keep_both_options_off(favit):
    opt = favit.train.FusedAdamW(_groups(17), distributed=False)             # (no limit on the groups without them)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    assert opt.grad_norm is None and opt.skipped_steps is None


def test_kernel_wrappers_validate_on_the_host(favit):
    K = favit.kernels
    with pytest.raises(ValueError):
        K.grad_norm([torch.zeros(1)] * 17)
    with pytest.raises(ValueError):
        K.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), label_smoothing=1.0)
    with pytest.raises(ValueError):
        K.adamw(*[torch.zeros(1)] * 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, skip_nonfinite=True)


class _Opt:
    def __init__(self, lrs):
        self.groups = [{"lr": lr} for lr in lrs]


def test_warmup_cosine_values_and_group_ratios(favit):
    base = [1e-4, 5e-4, 1e-3]                      # param_groups: body, latent_proj at 5x, head
    opt = _Opt(base)
    W, T = 10, 110
    sch = favit.train.WarmupCosine(opt, W, T, min_ratio=0.1)

    def lrs_at(t):
        while sch.t < t:
            sch.step()
        assert sch.t == t
        return [g["lr"] for g in opt.groups]

    def check(t, factor):
        got = lrs_at(t)
        for lr, b in zip(got, base):
            assert lr == pytest.approx(b * factor, rel=1e-12)
        assert got[1] / got[0] == pytest.approx(5.0, rel=1e-12) and got[2] / got[0] == pytest.approx(10.0, rel=1e-12)

    check(0, 1.0 / W)                               # step 0: the first rung of the linear warm-up
    check(4, 5.0 / W)
    check(W - 1, 1.0)                               # the last warm-up step runs at the full rate
    check(W, 1.0)                                   # the cosine starts from there
    check(W + (T - W) // 4, 0.1 + 0.9 * 0.5 * (1.0 + math.cos(math.pi / 4)))
    check(W + (T - W) // 2, 0.1 + 0.9 * 0.5)        # mid-point: halfway between 1 and min_ratio
    check(T, 0.1)                                   # the end ...
    check(T + 7, 0.1)                               # ... and it stays there
    assert sch.last_lr == [g["lr"] for g in opt.groups]


def test_warmup_cosine_without_warmup_and_argument_checks(favit):
    opt = _Opt([2e-3])
    sch = favit.train.WarmupCosine(opt, 0, 4)
    seen = [opt.groups[0]["lr"]]
    for _ in range(4):
        sch.step()
        seen.append(opt.groups[0]["lr"])
    want = [2e-3 * 0.5 * (1.0 + math.cos(math.pi * k / 4)) for k in range(5)]
    assert seen == pytest.approx(want, rel=1e-12, abs=1e-18)
    for args in [(-1, 10), (11, 10), (0, 0)]:
        with pytest.raises(ValueError):
            favit.train.WarmupCosine(_Opt([1.0]), *args)
    with pytest.raises(ValueError):
        favit.train.WarmupCosine(_Opt([1.0]), 1, 10, min_ratio=1.5)


def _tool():
    spec = importlib.util.spec_from_file_location("favit_run_experiment_cli", os.path.join(ROOT, "tools", "run_experiment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_defaults_are_todays_behaviour_and_the_flags_parse():
    tool = _tool()
    a = tool.parse_args(["--experiment", "mhla"])
    assert a.clip_grad_norm is None and a.skip_nonfinite is False and a.label_smoothing == 0.0
    assert a.lr_schedule == "constant" and a.warmup_epochs == 0.0
    assert a.learning_rate == 1e-4 and a.epochs == 100                  # (untouched neighbours)
    b = tool.parse_args(["--experiment", "mhla", "--clip_grad_norm", "1.0", "--skip_nonfinite", "--label_smoothing", "0.1",
                         "--lr_schedule", "cosine", "--warmup_epochs", "2.5"])
    assert b.clip_grad_norm == 1.0 and b.skip_nonfinite is True and b.label_smoothing == 0.1
    assert b.lr_schedule == "cosine" and b.warmup_epochs == 2.5
    with pytest.raises(SystemExit):
        tool.parse_args(["--experiment", "mhla", "--lr_schedule", "linear"])
