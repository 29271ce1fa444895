"""fp32x3 compute mode, host side (no GPU): the mode switch, the ABI constant, and the numerical model of the
three-pass split product (include/favit.h, FAVIT_F32X3) that the GPU tolerances of tests/test_gpu_fp32x3.py rest on."""
import os
import re

import pytest
import torch

from conftest import ROOT, rel_l2

GEMM_TOL = 1e-5          # rel-L2 of one split GEMM against fp64: the model sits at 4.4e-6 for every K, fp32 accumulation
                         # adds ~4e-7; a truncating split (1.3e-5) or a dropped cross term (2e-3) lands above the line


def test_mode_switch_and_environment_hook(favit, monkeypatch):
    monkeypatch.delenv("FAVIT_FP32_GEMM", raising=False)
    try:
        favit.set_compute_dtype("fp32x3")
        assert favit.get_compute_mode() == "fp32x3"
        assert favit.get_compute_dtype() is torch.float32
        assert favit.kernels._F32_GEMM["in_dtype"] == favit._abi.F32X3
        favit.set_compute_dtype("fp32")
        assert favit.get_compute_mode() == "fp32" and favit.get_compute_dtype() is torch.float32
        assert favit.kernels._F32_GEMM["in_dtype"] == favit._abi.F32
        with pytest.raises((KeyError, ValueError)):
            favit.set_compute_dtype("fp32x4")
        assert favit.get_compute_mode() == "fp32"                     # a rejected string changes nothing
        # the benchmark's hook: read at each call, fp32 only
        monkeypatch.setenv("FAVIT_FP32_GEMM", "x3")
        favit.set_compute_dtype("fp32")
        assert favit.get_compute_mode() == "fp32x3" and favit.get_compute_dtype() is torch.float32
        favit.set_compute_dtype(torch.float32)
        assert favit.get_compute_mode() == "fp32x3"
        favit.set_compute_dtype("bf16")
        assert favit.get_compute_mode() == "bf16" and favit.kernels._F32_GEMM["in_dtype"] == favit._abi.F32
        favit.set_compute_dtype("fp8")
        assert favit.get_compute_mode() == "fp8"
        monkeypatch.delenv("FAVIT_FP32_GEMM")
        favit.set_compute_dtype("fp32")
        assert favit.get_compute_mode() == "fp32"
    finally:
        monkeypatch.delenv("FAVIT_FP32_GEMM", raising=False)
        favit.set_compute_dtype("fp32")


def test_abi_constant_matches_the_header(favit):
    assert favit._abi.F32X3 == 3
    assert (favit._abi.F32, favit._abi.BF16, favit._abi.FP8) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "favit.h")).read()
    assert re.search(r"\bFAVIT_F32X3\s*=\s*3\b", hdr)
    assert re.search(r"#define\s+FAVIT_ABI_VERSION\s+8\b", hdr)       # additive: the version does not move
    so = os.path.join(ROOT, "focused-attention-vit_amd", "lib", "libfavit.so")
    if os.path.exists(so):
        assert favit._abi.lib().favit_abi_version() == 8


def _split(x):
    """hi = bf16_rne(x), lo = bf16_rne(x - float(hi)) -- torch's float32 -> bfloat16 cast rounds to nearest even."""
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def _x3_product(a, b, drop_cross_term=False):
    """The definition in include/favit.h on exact bf16 parts (their pairwise products are exact in fp32; the sum runs in
    fp64 here, so what is measured is the split alone)."""
    ah, al = _split(a)
    bh, bl = _split(b)
    ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    acc = ah @ bh.t() + ah @ bl.t()
    if not drop_cross_term:
        acc = acc + al @ bh.t()
    return acc


@pytest.mark.parametrize("Kd", [384, 1536, 50432])
def test_split_product_model_against_fp64(Kd):
    g = torch.Generator().manual_seed(Kd)
    a = torch.randn((96, Kd), generator=g)
    b = torch.randn((64, Kd), generator=g)
    ref = a.double() @ b.double().t()
    err = rel_l2(_x3_product(a, b), ref)
    err_dropped = rel_l2(_x3_product(a, b, drop_cross_term=True), ref)
    print(f"K={Kd}: three-pass split {err:.2e}, lo_a*hi_b left out {err_dropped:.2e}")
    assert err < GEMM_TOL
    assert err_dropped > GEMM_TOL
    # the parts are what the header says: hi carries 8 significant bits, hi + lo 16
    hi, lo = _split(a)
    assert rel_l2(hi, a) < 2.0 ** -8 and rel_l2(hi + lo, a) < 2.0 ** -16
