"""Host side of the native block chains: the two layout queries, the descriptor mirror and the
symbol table.  No GPU: the layout queries are host arithmetic, and a declined geometry returns before any launch."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest


def _rows(L, W, depth):
    """Row counts the blocks of a CLS-only encoder run on (functional.cls_plan; None = all L rows)."""
    h = W // 2
    out = []
    for k in range(1, depth + 1):
        j = depth - k
        n = 2 + h * (2 * j + 1)
        out.append(min(n, L))
    return out


# (B, D, H, W, hidden, row counts)
SHAPES = [
    (3, 128, 2, 7, 512, _rows(17, 7, 3)),            # 17, 11, 5
    (2, 192, 3, 3, 768, _rows(30, 3, 5)),            # 11, 9, 7, 5, 3
    (3, 128, 2, 7, 512, _rows(50, 7, 4)),            # 23, 17, 11, 5
    (256, 384, 6, 7, 1536, _rows(197, 7, 12)),       # cfg2: 71, 65, ..., 5
    (64, 768, 12, 7, 3072, _rows(577, 7, 12)),       # cfg4: the same row counts at B = 64, D = 768
    (2, 384, 6, 7, 1536, [197]),                     # an encoder that is not cut
]
CASES = [(B, n, D, H, W, hid) for B, D, H, W, hid, rows in SHAPES for n in rows]


def _desc(favit, B, n, D, H, W, hidden, training):
    d = favit._abi.BlockDesc()
    d.B, d.n, d.D, d.H, d.W, d.hidden, d.training, d.eps = B, n, D, H, W, hidden, training, 1e-5
    return d


def _expected_sizes(B, n, D, H, hidden, training, want_lp):
    M = B * n
    nparts = min(2048, (M + 3) // 4)
    tape = dict(xn1=M * D * 2, mu1=M * 4, rs1=M * 4, qkv=M * 3 * D * 2, o=M * D * 2, lse=B * H * n * 4 if training else 0,
                x1=M * D * 4, xn2=M * D * 2, mu2=M * 4, rs2=M * 4, h=M * hidden * 2, pre=M * hidden * 2, x2=M * D * 4)
    bwd = dict(dpre=M * hidden * 2, dxn2=M * D * 2, g1_f32=M * D * 4, g1_lp=M * D * 2, do=M * D * 2, dqkv=M * 3 * D * 2,
               dxn1=M * D * 2, g_out_f32=M * D * 4, g_out_lp=M * D * 2 if want_lp else 0, part1=2 * nparts * D * 4,
               part2=2 * nparts * D * 4)
    return tape, bwd


def _check_layout(names, offsets, total, sizes):
    """Offsets are multiples of 256, ascend, every slot holds its buffer without reaching the next one, and the last
    slot ends at the returned size (rounded up to 256 like every other)."""
    assert len(offsets) == len(names)
    end = 0
    for k, off in zip(names, offsets):
        assert off % 256 == 0, k
        assert off >= end, f"{k} overlaps its predecessor"
        end = off + sizes[k]
    assert 0 <= total - end < 256 and total % 256 == 0


def test_row_counts_are_the_cls_plan(favit):
    F = favit.functional
    for L, W, depth in ((17, 7, 3), (30, 3, 5), (50, 7, 4), (197, 7, 12), (577, 7, 12)):
        want = [L if c is None else sum(c) for c in F.cls_plan(L, W, depth)]
        assert _rows(L, W, depth) == want
    assert _rows(197, 7, 12) == list(range(71, 4, -6))


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("B,n,D,H,W,hidden", CASES)
def test_layouts(favit, B, n, D, H, W, hidden, training):
    lib, A = favit._abi.lib(), favit._abi
    d = _desc(favit, B, n, D, H, W, hidden, training)
    to = (ctypes.c_int64 * len(A.BLOCK_TAPE_SLOTS))()
    total = lib.favit_mhla_block_tape_layout(ctypes.byref(d), to)
    supported = bool(lib.favit_mhla_attn_lse_supported(n, 64, W, A.BF16))
    if not supported:                                  # 5 rows under a 7-wide window, 3 under a 3-wide one
        assert n < W + 1
        assert total == A.ERR_UNSUPPORTED
        assert lib.favit_mhla_block_bwd_layout(ctypes.byref(d), 1, None) == A.ERR_UNSUPPORTED
        assert favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, training) is None
        return
    assert total == lib.favit_mhla_block_tape_layout(ctypes.byref(d), None)
    for want_lp in (0, 1):
        tape, bwd = _expected_sizes(B, n, D, H, hidden, training, want_lp)
        _check_layout(A.BLOCK_TAPE_SLOTS, list(to), total, tape)
        bo = (ctypes.c_int64 * len(A.BLOCK_BWD_SLOTS))()
        nb = lib.favit_mhla_block_bwd_layout(ctypes.byref(d), want_lp, bo)
        _check_layout(A.BLOCK_BWD_SLOTS, list(bo), nb, bwd)
        i = A.BLOCK_BWD_SLOTS.index("g_out_lp")
        assert (bo[i + 1] - bo[i] == 0) == (not want_lp), "g_out_lp is empty exactly when a row cut follows"
    i = A.BLOCK_TAPE_SLOTS.index("lse")
    assert (to[i + 1] - to[i] == 0) == (not training), "lse is empty exactly in eval mode"
    # the Python-side plan is the same table
    plan = favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, training)
    assert plan.tape_bytes == total and [plan.off[k][0] for k in A.BLOCK_TAPE_SLOTS] == list(to)
    assert plan.off["lse"][1] == (0 if not training else to[i + 1] - to[i])
    assert plan.nparts == min(2048, (B * n + 3) // 4)


@pytest.mark.parametrize("B,n,D,H,W,hidden,code", [
    (2, 17, 96, 2, 7, 384, "ERR_UNSUPPORTED"),       # D is no multiple of 64
    (2, 17, 128, 4, 7, 512, "ERR_UNSUPPORTED"),      # head size 32
    (2, 17, 128, 2, 7, 516, "ERR_UNSUPPORTED"),      # hidden is no multiple of 8
    (2, 17, 128, 2, 6, 512, "ERR_UNSUPPORTED"),      # even window
    (2, 17, 128, 2, 13, 512, "ERR_UNSUPPORTED"),     # a window the lse kernels do not take
    (0, 17, 128, 2, 7, 512, "ERR_INVALID"),
    (2, 17, 128, 0, 7, 512, "ERR_INVALID"),
])
def test_declined_geometry_returns_before_any_launch(favit, B, n, D, H, W, hidden, code):
    """fwd / bwd check the geometry first, so these calls return on a machine without a GPU."""
    lib, A = favit._abi.lib(), favit._abi
    d = _desc(favit, B, n, D, H, W, hidden, 1)
    want = getattr(A, code)
    assert lib.favit_mhla_block_tape_layout(ctypes.byref(d), None) == want
    assert lib.favit_mhla_block_bwd_layout(ctypes.byref(d), 0, None) == want
    d.x = d.tape = d.g1 = d.b1 = d.g2 = d.b2 = d.weff = d.beff = d.wproj = d.bproj = d.wfc1 = d.bfc1 = d.wfc2 = d.bfc2 = 0x10000
    d.tape_bytes = 1 << 40
    assert lib.favit_mhla_block_fwd(ctypes.byref(d), None) == want
    assert lib.favit_mhla_block_bwd(ctypes.byref(d), 0x10000, 0x10000, 0x10000, 1 << 40, 1, None) == want
    assert favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, True) is None


def test_bad_arguments_return_before_any_launch(favit):
    """Null pointers, a short or misaligned tape, a short arena, a backward after an eval-mode forward."""
    lib, A = favit._abi.lib(), favit._abi
    fields = ("x", "tape", "g1", "b1", "g2", "b2", "weff", "beff", "wproj", "bproj", "wfc1", "bfc1", "wfc2", "bfc2")

    def fresh(training=1):
        d = _desc(favit, 2, 17, 128, 2, 7, 512, training)
        for f in fields:
            setattr(d, f, 0x10000)
        d.tape_bytes = lib.favit_mhla_block_tape_layout(ctypes.byref(d), None)
        return d
    d = fresh()
    nb = lib.favit_mhla_block_bwd_layout(ctypes.byref(d), 1, None)
    bwd = lambda d, g=0x10000, glp=0x10000, ar=0x10000, n=nb: lib.favit_mhla_block_bwd(ctypes.byref(d), g, glp, ar, n, 1, None)
    for f in fields:
        d = fresh()
        setattr(d, f, None)
        assert lib.favit_mhla_block_fwd(ctypes.byref(d), None) == A.ERR_INVALID, f
        assert bwd(d) == A.ERR_INVALID, f
    d = fresh()
    d.tape_bytes -= 1
    assert lib.favit_mhla_block_fwd(ctypes.byref(d), None) == A.ERR_INVALID
    assert bwd(d) == A.ERR_INVALID
    d = fresh()
    d.tape = 0x10080
    assert lib.favit_mhla_block_fwd(ctypes.byref(d), None) == A.ERR_ALIGN
    d = fresh()
    assert bwd(d, n=nb - 1) == A.ERR_INVALID
    assert bwd(d, g=None) == A.ERR_INVALID and bwd(d, glp=None) == A.ERR_INVALID and bwd(d, ar=None) == A.ERR_INVALID
    assert bwd(d, ar=0x10010) == A.ERR_ALIGN
    assert bwd(fresh(training=0)) == A.ERR_INVALID
    assert lib.favit_mhla_block_fwd(None, None) == A.ERR_INVALID


def test_block_descriptor_layout_matches_header(favit):
    BD = favit._abi.BlockDesc
    assert ctypes.sizeof(BD) == 14 * 8 + 8 + 7 * 4 + 4
    if not shutil.which("gcc"):
        return
    fields = [f[0] for f in BD._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"favit.h\"\nint main(){printf(\"%zu\", sizeof(favit_mhla_block_t));" + \
          "".join(f'printf(" %zu", offsetof(favit_mhla_block_t, {f}));' for f in fields) + \
          'printf(" %d %d", FAVIT_BLOCK_TAPE_SLOTS, FAVIT_BLOCK_BWD_SLOTS);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as fh:
            fh.write(src)
        inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
        subprocess.check_call(["gcc", "-I", inc, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")], text=True).split()
    assert int(out[0]) == ctypes.sizeof(BD)
    for f, off in zip(fields, out[1:]):
        assert getattr(BD, f).offset == int(off), f
    assert int(out[-2]) == len(favit._abi.BLOCK_TAPE_SLOTS) and int(out[-1]) == len(favit._abi.BLOCK_BWD_SLOTS)


def test_symbols_and_abi_version(favit):
    A = favit._abi
    new = {"favit_mhla_block_tape_layout", "favit_mhla_block_bwd_layout", "favit_mhla_block_fwd", "favit_mhla_block_bwd"}
    assert new <= set(A._SIGS)
    assert sorted(A._SIGS) == A.declared_symbols()
    lib = A.lib()
    assert all(hasattr(lib, s) for s in new)
    assert lib.favit_abi_version() == 8


@pytest.mark.parametrize("training", [False, True])
def test_native_tape_builds_the_chains_records(favit, training):
    """What the Python backward reads from a native tape are the chains' own records, every tensor field a view of its
    plan.off slot, every dropout field zero (a block with an active dropout never runs the native chain)."""
    import torch
    F = favit.functional
    B, n, D, H, W, hidden = 3, 17, 128, 2, 7, 512
    plan = favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, training)
    buf = torch.zeros(plan.tape_bytes, dtype=torch.uint8)
    pa, pm, weff, wc = [object()] * 6, [object()] * 4, object(), (object(), object(), object())
    tp = F._NativeTape(plan, buf, None, (None, None), (None, None), pa, pm, weff, wc, None)
    M, f32, bf16 = B * n, torch.float32, torch.bfloat16

    def check(t, slot, shape, dtype):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), slot
        assert t.data_ptr() - buf.data_ptr() == plan.off[slot][0], slot
        assert t.numel() * t.element_size() <= plan.off[slot][1], slot
    sa, sm = tp.sa, tp.sm
    assert type(sa) is F.MHLASaved and type(sm) is F.MLPSaved
    check(sa.xn, "xn1", (M, D), bf16)
    check(sa.qkv, "qkv", (M, 3 * D), bf16)
    check(sa.o, "o", (M, D), bf16)
    check(tp.mu1, "mu1", (M,), f32)
    check(tp.rs1, "rs1", (M,), f32)
    if training:
        check(sa.lse, "lse", (B, H, n), f32)
    else:
        assert sa.lse is None
    assert sa.weff is weff and sa.wp_c is wc[0] and sa.prm is pa and sa.mask is None and (sa.B, sa.L) == (B, n)
    assert (sa.p_attn, sa.seed_attn, sa.p_proj, sa.seed_proj) == (0.0, 0, 0.0, 0)
    assert F.MHLAChain.out_dropout(sa) == (0.0, 0)
    check(sm.xn, "xn2", (M, D), bf16)
    check(sm.pre, "pre", (M, hidden), bf16)
    check(sm.h, "h", (M, hidden), bf16)
    check(tp.mu2, "mu2", (M,), f32)
    check(tp.rs2, "rs2", (M,), f32)
    check(tp.x1, "x1", (M, D), f32)
    assert sm.pre_is_grad is True and sm.w1_c is wc[1] and sm.w2_c is wc[2] and sm.prm is pm
    assert (sm.p, sm.seed_fc1, sm.seed_fc2) == (0.0, 0, 0)
    assert F.MLPChain.out_dropout(sm) == (0.0, 0)
    assert tp.sa is sa and tp.sm is sm, "made once"


def test_switches(favit, monkeypatch):
    F = favit.functional
    favit.set_compute_dtype("bf16")
    try:
        monkeypatch.delenv("FAVIT_NO_NATIVE_BLOCKS", raising=False)
        assert F._native_blocks_on()
        F.set_native_blocks(False)
        assert not F._native_blocks_on()
        F.set_native_blocks(True)
        monkeypatch.setenv("FAVIT_NO_NATIVE_BLOCKS", "1")
        assert not F._native_blocks_on()
        monkeypatch.delenv("FAVIT_NO_NATIVE_BLOCKS")
        monkeypatch.setattr(favit.kernels, "GEMM_TRACE", [])
        assert not F._native_blocks_on()
        monkeypatch.setattr(favit.kernels, "GEMM_TRACE", None)
        for mode in ("fp32", "fp32x3", "fp8"):
            favit.set_compute_dtype(mode)
            assert not F._native_blocks_on()
    finally:
        favit.set_compute_dtype("fp32")
        F.set_native_blocks(True)
