"""Host side of stochastic depth (DropPath): the linear rate rule and where a rate is in force, pruning stays on, the
entry points are declared / bound / exported under ABI 8 and refuse bad arguments before they launch anything, the
run_experiment flag, and the seed restatement the GPU tests rebuild their masks from."""
import ctypes
import importlib
import inspect
import os
import sys

import pytest
import torch

import _drop_path_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mhla_model(favit, depth, rate=None, **kw):
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=depth,
                                                    num_heads=2, window_size=7, use_mhla=True, **kw)
    return m if rate is None else m.set_drop_path_rate(rate)


@pytest.mark.parametrize("depth", [1, 2, 12])
def test_linear_rate_rule(favit, depth):
    m = _mhla_model(favit, depth, 0.3)
    got = [b.drop_path for b in m.blocks]
    assert got == [0.3 * i / max(1, depth - 1) for i in range(depth)] == R.linear_rates(0.3, depth)
    assert got[0] == 0.0 and (depth == 1 or got[-1] == 0.3)
    assert all(isinstance(p, float) for p in got)
    assert [b._spec().drop_path for b in m.blocks] == got
    assert m.drop_path_rate == 0.3


def test_every_model_with_a_block_stack_takes_a_rate(favit):
    M = favit.models
    kw = dict(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=3, num_heads=2)
    models = [M.vit.VisionTransformer(**kw), M.vit_mhla.VisionTransformerMHLA(use_mhla=True, **kw),
              M.vit_mhla.VisionTransformerMHLA(use_mhla=False, **kw), M.sppp_mhla.SPPPViTMHLA(use_mhla=True, **kw),
              M.mhla_models.PretrainedViTWithMHLA(window_size=7, **kw),
              M.mhla_models.PretrainedSPPPViTWithMHLA(window_size=7, **kw)]
    for m in models:
        keys = list(m.state_dict().keys())
        assert [b.drop_path for b in m.blocks] == [0.0, 0.0, 0.0], type(m).__name__
        assert m.set_drop_path_rate(0.2) is m
        assert [b._spec().drop_path for b in m.blocks] == [0.0, 0.1, 0.2], type(m).__name__
        assert list(m.state_dict().keys()) == keys, "a rate adds no parameter and no buffer"
        assert "drop_path" not in inspect.signature(type(m).__init__).parameters      # constructors mirror the reference
        with pytest.raises(ValueError):
            m.set_drop_path_rate(1.0)


def test_rate_zero_and_eval_leave_no_active_half(favit):
    F = favit.functional
    specs = [b._spec() for b in _mhla_model(favit, 4).blocks]
    assert all(F.EncoderOp(specs, None, True).drop_path_of(s) == 0.0 for s in specs)
    specs = [b._spec() for b in _mhla_model(favit, 4, 0.3).blocks]
    assert all(F.EncoderOp(specs, None, False).drop_path_of(s) == 0.0 for s in specs), "eval mode"
    assert [F.EncoderOp(specs, None, True).drop_path_of(s) > 0 for s in specs] == [False, True, True, True]
    with pytest.raises(ValueError):
        F.BlockSpec(specs[0].attn, specs[0].mlp, drop_path=1.0)
    assert F.BlockSpec(specs[0].attn, specs[0].mlp).drop_path == 0.0


def test_drop_path_keeps_the_pruned_path_and_element_dropout_does_not(favit, monkeypatch):
    F = favit.functional
    monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
    L = 65
    plain = [b._spec() for b in _mhla_model(favit, 4).blocks]
    dropped = [b._spec() for b in _mhla_model(favit, 4, 0.5).blocks]
    want = F.cls_only_cuts(plain, L, None, True)
    assert want is not None and all(c is not None for c in want)
    assert F.cls_only_cuts(dropped, L, None, True) == want
    assert F.mlp_narrow_plan(F.cls_only_cuts(dropped, L, None, True)) == F.mlp_narrow_plan(want)
    both = [b._spec() for b in _mhla_model(favit, 4, 0.5, dropout=0.1).blocks]
    assert F.cls_only_cuts(both, L, None, True) is None
    assert F.cls_only_cuts(both, L, None, False) == want


def test_entry_points_are_declared_bound_and_exported(favit):
    A = favit._abi
    lib, sig, declared = A.lib(), A._SIGS, A.declared_symbols()
    for name in ("favit_drop_path_add", "favit_drop_path_bwd"):
        assert name in declared, f"{name} is not declared in include/favit.h"
        assert name in sig, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"libfavit.so does not export {name}"
    assert lib.favit_abi_version() == 8, "the additions are additive: the ABI version stays"
    assert callable(favit.kernels.drop_path_add) and callable(favit.kernels.drop_path_bwd)
    with open(os.path.join(ROOT, "focused-attention-vit_amd", "csrc", "Makefile")) as f:
        assert "drop_path.hip" in f.read()


def test_refusals_come_before_any_launch(favit):
    """Bad arguments are answered on the host: no device is needed (or touched) to be refused."""
    A = favit._abi
    lib = A.lib()
    buf = (ctypes.c_float * 64)()                       # 256 bytes of host memory: never dereferenced
    p = ctypes.c_void_p(ctypes.addressof(buf))
    add = lambda x=p, y=p, dt=A.F32, out=p, B=2, n=1, D=8, rate=0.5: lib.favit_drop_path_add(x, y, dt, out, B, n, D, rate, 1, None)
    bwd = lambda g=p, lp=p, dt=A.BF16, B=2, n=1, D=8, rate=0.5, lpp=0.0: lib.favit_drop_path_bwd(g, lp, dt, B, n, D, rate, 1, lpp, 2, None)
    for fn in (add, bwd):
        for rate in (1.0, -0.1, 1.5, float("nan")):
            assert fn(rate=rate) == A.ERR_INVALID, rate
        for kw in (dict(B=0), dict(n=0), dict(D=0), dict(B=-1), dict(dt=A.FP8)):
            assert fn(**kw) == A.ERR_INVALID, kw
        for D in (4, 12, 100):
            assert fn(D=D) == A.ERR_UNSUPPORTED, D
    assert add(x=None) == add(y=None) == add(out=None) == A.ERR_INVALID
    assert bwd(g=None) == bwd(lp=None) == A.ERR_INVALID
    assert bwd(lpp=1.0) == bwd(lpp=-0.5) == A.ERR_INVALID


def test_kernel_wrappers_refuse_cpu_tensors(favit):
    K = favit.kernels
    t = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.drop_path_add(t, t.clone(), 2, 1, 8, 0.5, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.drop_path_bwd(t, torch.bfloat16, 2, 1, 8, 0.5, 1)


def test_run_experiment_flag_parses_and_reaches_the_blocks(favit):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        tool = importlib.import_module("run_experiment")
    finally:
        sys.path.pop(0)
    assert tool.parse_args(["--experiment", "mhla"]).drop_path == 0.0
    a = tool.parse_args(["--experiment", "mhla", "--drop_path", "0.2", "--img_size", "32", "--patch_size", "4",
                         "--embed_dim", "64", "--depth", "3", "--num_heads", "2"])
    assert a.drop_path == 0.2
    for exp in ("traditional", "mhla", "sppp_mhla"):
        a.experiment = exp
        m = tool.build_model(favit, a, 10)
        assert [b.drop_path for b in m.blocks] == [0.0, 0.1, 0.2], exp


def test_expected_seeds_restates_functional_seed(favit):
    F = favit.functional
    want = R.expected_seeds(77, 5)
    assert len(set(want)) == 5 and all(0 <= s < 2 ** 63 for s in want)
    torch.manual_seed(77)
    assert [F._seed() for _ in range(5)] == want
    assert R.expected_seeds(77, 3) == want[:3]
    assert R.expected_seeds(78, 3) != want[:3]


def test_sample_keep_is_the_dropout_draw_by_sample_number():
    import _dropout_ref as DR
    for seed in (1, 0x5DEECE66D, 2 ** 62 + 12345):
        for p in (0.1, 0.5):
            k = R.sample_keep(seed, 9, p)
            assert k.shape == (9,) and (k == DR.keep_mask(seed, 9, p)).all()
            assert (k[:5] == R.sample_keep(seed, 5, p)).all(), "the draw of sample b does not depend on B"
            s = R.sample_scale(seed, 9, p)
            assert torch.equal(s != 0, torch.from_numpy(k)) and set(s.tolist()) <= {0.0, DR.keep_scale(p)}
    assert torch.equal(R.sample_scale(3, 4, 0.0), torch.ones(4, dtype=torch.float64))
