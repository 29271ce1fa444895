"""GPU tests of the batched ("many in one launch") and accumulating ("add into the gradient buffer") kernel forms the
fused training step runs: the row reductions, the MHLA latent_proj fold at all three head dims, the LayerNorm backward
in its accumulate / defer / frozen / dropout / strided forms, and the pos-less embedding prologue and the unfused
softmax with a key-keep mask and dropout.  Each is compared with a plain float64 PyTorch restatement of the operation
on the same seeded inputs.  Gates (the header of test_gpu_kernels.py): fp32 results 2e-5 rel-L2, bf16 outputs 1e-2
against a reference that starts from the bf16-rounded inputs.  Where a form only re-orders launches of the same code
(multi vs single, frozen vs ordinary, masked copy vs dropout kernel) the assertion is bit-equality.

Every sum that is compared is drawn with a non-zero mean (randn + 0.5), so no reference is a near-cancellation."""
import ctypes as C

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

_WORST = {}         # (group, gate) -> worst rel-L2 seen in this run (printed at module teardown; visible with -s)


@pytest.fixture(scope="module")
def K(favit):
    yield favit.kernels
    for (group, gate), e in sorted(_WORST.items()):
        print(f"\n[batched launches] {group}: worst rel-L2 {e:.3e} (gate {gate:g})", end="")
    print()


def _tol(dtype):
    return 2e-5 if dtype == F32 else 1e-2


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, shift=0.0, scale=1.0):
    return torch.randn(shape, generator=g, device=DEV) * scale + shift


def _close(group, got, ref, tol, what=""):
    e = rel_l2(got, ref)
    _WORST[(group, tol)] = max(_WORST.get((group, tol), 0.0), e)
    assert e < tol, f"{group} {what}: rel-L2 {e:.3e} >= {tol:g}"


def _raises_code(code, fn, *a, **kw):
    with pytest.raises(RuntimeError, match=rf"\(code {code}\)"):
        fn(*a, **kw)


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------------------
# 1. Row reductions
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(37, 1), (1, 5), (16, 64), (65, 65), (2048, 384), (113, 200)])
def test_reduce_rows(K, rows, cols):
    """out[c] = sum_r t[r, c]; (37, 1) is the loss of train.cross_entropy (one column, rows = batch)."""
    t = _randn((rows, cols), _gen(rows * 1000 + cols), shift=0.5)
    out = K.reduce_rows(t)
    assert out.shape == (cols,) and out.dtype == F32
    _close("reductions", out, t.double().sum(0), 2e-5, f"reduce_rows {rows}x{cols}")


def test_reduce_rows_row_strided_input(K):
    """ld > cols: a column slice of a wider tensor (the neighbouring columns must not leak into the sums)."""
    wide = _randn((113, 300), _gen(7), shift=0.5)
    t = wide[:, 50:250]
    assert t.stride(0) == 300 and not t.is_contiguous()
    _close("reductions", K.reduce_rows(t), t.double().sum(0), 2e-5, "reduce_rows strided")


@pytest.mark.parametrize("n", [1, 3, 32, 33])
@pytest.mark.parametrize("rows,cols", [(9, 68), (175, 192), (511, 64), (512, 64), (2048, 384)])
def test_reduce_rows_multi(K, rows, cols, n):
    """out0[e] += colsum(part[e][0]), out1[e] += colsum(part[e][1]): every entry has its own data and its own
    pre-filled destinations and is checked against its own entry (entry index, second stacked matrix, row split:
    rows >= 512 splits the rows eight ways; 33 entries are two launches of the wrapper)."""
    g = _gen(rows * 31 + cols * 7 + n)
    parts = [_randn((2, rows, cols), g, shift=0.5) for _ in range(n)]
    outs = [(_randn((cols,), g), _randn((cols,), g)) for _ in range(n)]
    refs = [[o.double() + part[s].double().sum(0) for s, o in enumerate(o01)] for part, o01 in zip(parts, outs)]
    K.reduce_rows_multi([(part, o0, o1) for part, (o0, o1) in zip(parts, outs)])
    for e in range(n):
        for s in range(2):
            _close("reductions", outs[e][s], refs[e][s], 2e-5, f"reduce_rows_multi entry {e} stack {s} of {n}")


def test_reduce_rows_multi_refuses_bad_arguments(K, favit):
    abi = favit._abi
    rows, cols = 9, 68
    g = _gen(11)
    parts = [_randn((2, rows, cols), g, shift=0.5) for _ in range(33)]
    o0 = [_randn((cols,), g) for _ in range(33)]
    o1 = [_randn((cols,), g) for _ in range(33)]
    before = [t.clone() for t in o0 + o1]
    fn = abi.lib().favit_reduce_rows_multi
    assert fn(0, _ptrs(parts), _ptrs(o0), _ptrs(o1), rows, cols, _st()) == abi.ERR_INVALID
    assert fn(33, _ptrs(parts), _ptrs(o0), _ptrs(o1), rows, cols, _st()) == abi.ERR_INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(o0 + o1, before)), "a refused call must not have launched"
    odd = _randn((2, rows, 64), g)
    with pytest.raises(ValueError):
        K.reduce_rows_multi([(parts[0], o0[0], o1[0]), (odd, o0[1][:64], o1[1][:64])])
    assert all(torch.equal(a, b) for a, b in zip(o0 + o1, before))


# --------------------------------------------------------------------------------------
# 2. MHLA fold: all three head dims, batched and accumulating
# --------------------------------------------------------------------------------------
# (D, H): hd = 16 with D + 1 < 64 (one partial tile), the shape of test_mhla_fold_matches_separate_latent_proj, hd = 32,
# hd = 64 at 3 / 4 tiles, and cfg2 (7 tiles over FOLD_L_SPLIT = 4 row groups)
FOLD_GEOMS = [(48, 3), (64, 4), (96, 3), (128, 2), (192, 3), (384, 6)]
_FOLD_CACHE = {}


def _fold_layer(D, H, i):
    """Layer i of geometry (D, H): parameters, an upstream gradient, pre-fill gradients and the float64 reference
    (Weff, beff, and autograd of (Weff*dWeff).sum() + (beff*dbeff).sum()); computed once and never written to."""
    key = (D, H, i)
    if key in _FOLD_CACHE:
        return _FOLD_CACHE[key]
    hd = D // H
    g = _gen(100003 * D + 1009 * H + i)
    L = {"wqkv": _randn((3 * D, D), g), "bqkv": _randn((3 * D,), g), "wl": _randn((hd, hd), g), "bl": _randn((hd,), g),
         "dweff": _randn((3 * D, D), g, shift=0.5), "dbeff": _randn((3 * D,), g, shift=0.5),
         "pre": (_randn((3 * D, D), g), _randn((3 * D,), g), _randn((hd, hd), g), _randn((hd,), g))}
    w, b, l, lb = [L[k].double().requires_grad_(True) for k in ("wqkv", "bqkv", "wl", "bl")]
    wk, bk = w.reshape(3, H, hd, D), b.reshape(3, H, hd)
    weff = torch.cat([wk[0].reshape(D, D), (l @ wk[1]).reshape(D, D), (l @ wk[2]).reshape(D, D)])
    beff = torch.cat([bk[0].reshape(D), (bk[1] @ l.t() + lb).reshape(D), (bk[2] @ l.t() + lb).reshape(D)])
    ((weff * L["dweff"].double()).sum() + (beff * L["dbeff"].double()).sum()).backward()
    L["weff_ref"], L["beff_ref"] = weff.detach(), beff.detach()
    L["grad_ref"] = (w.grad, b.grad, l.grad, lb.grad)
    _FOLD_CACHE[key] = L
    return L


def _fold_params(L):
    return L["wqkv"], L["bqkv"], L["wl"], L["bl"]


def _fold_bwd_single_acc(K, L, H):
    out = tuple(t.clone() for t in L["pre"])
    K.mhla_fold_bwd(L["dweff"], L["dbeff"], L["wqkv"], L["bqkv"], L["wl"], H, out=out)
    return out


@pytest.mark.parametrize("D,H", FOLD_GEOMS)
def test_fold_fwd_single(K, D, H):
    L = _fold_layer(D, H, 0)
    weff, beff = K.mhla_fold_fwd(*_fold_params(L), H, F32)
    _close("fold", weff, L["weff_ref"], 2e-5, f"weff D={D} H={H}")
    _close("fold", beff, L["beff_ref"], 2e-5, f"beff D={D} H={H}")
    weff_lp, beff_lp = K.mhla_fold_fwd(*_fold_params(L), H, BF16)
    assert weff_lp.dtype == BF16 and beff_lp.dtype == F32
    assert torch.equal(weff_lp, weff.to(BF16)), "the bf16 fold is the fp32 fold, rounded once on the way out"
    assert torch.equal(beff_lp, beff)


@pytest.mark.parametrize("n", [1, 2, 12, 32])
@pytest.mark.parametrize("D,H", FOLD_GEOMS)
def test_fold_fwd_multi_is_the_single_launch_per_layer(K, D, H, n):
    layers = [_fold_layer(D, H, i) for i in range(n)]
    for dtype in (F32, BF16):
        got = K.mhla_fold_fwd_multi([_fold_params(L) for L in layers], H, dtype)
        assert len(got) == n
        for i, (L, (weff, beff)) in enumerate(zip(layers, got)):
            w1, b1 = K.mhla_fold_fwd(*_fold_params(L), H, dtype)
            assert weff.dtype == dtype and torch.equal(weff, w1) and torch.equal(beff, b1), (i, dtype)
    # and the layers really differ, so an off-by-one layer index cannot pass the comparison above
    if n > 1:
        assert not torch.equal(got[0][0], got[1][0]) and not torch.equal(got[0][1], got[1][1])
    _close("fold", got[n - 1][0].float(), layers[n - 1]["weff_ref"], 1e-2, "last layer of the bf16 multi fold")


def test_fold_fwd_multi_refuses_33_layers(K, favit):
    abi = favit._abi
    D, H = 48, 3
    L = _fold_layer(D, H, 0)
    weff = torch.full((3 * D, D), 7.0, device=DEV)
    beff = torch.full((3 * D,), 7.0, device=DEV)
    cols = [_ptrs([t] * 33) for t in _fold_params(L)]
    fn = abi.lib().favit_mhla_fold_fwd_multi
    assert fn(33, *cols, _ptrs([weff] * 33), abi.F32, _ptrs([beff] * 33), D, H, _st()) == abi.ERR_INVALID
    assert fn(0, *cols, _ptrs([weff] * 33), abi.F32, _ptrs([beff] * 33), D, H, _st()) == abi.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((weff == 7.0).all()) and bool((beff == 7.0).all())


@pytest.mark.parametrize("D,H", FOLD_GEOMS)
def test_fold_bwd_single_fresh_and_accumulating(K, D, H):
    L = _fold_layer(D, H, 0)
    names = ("dwqkv", "dbqkv", "dwl", "dbl")
    fresh = K.mhla_fold_bwd(L["dweff"], L["dbeff"], L["wqkv"], L["bqkv"], L["wl"], H)
    for nm, got, ref in zip(names, fresh, L["grad_ref"]):
        _close("fold", got, ref, 2e-5, f"{nm} D={D} H={H}")
    acc = _fold_bwd_single_acc(K, L, H)
    for nm, got, pre, ref in zip(names, acc, L["pre"], L["grad_ref"]):
        _close("fold", got, pre.double() + ref, 2e-5, f"accumulated {nm} D={D} H={H}")
    # the q rows of dwqkv / dbqkv are a plain copy-add of the upstream gradient: exact
    assert torch.equal(acc[0][:D], L["pre"][0][:D] + L["dweff"][:D])
    assert torch.equal(acc[1][:D], L["pre"][1][:D] + L["dbeff"][:D])


@pytest.mark.parametrize("n", [1, 3, 16, 17])
@pytest.mark.parametrize("D,H", FOLD_GEOMS)
def test_fold_bwd_multi(K, D, H, n):
    """Every layer's fold backward in one launch (the wrapper chunks at 16), adding into pre-filled buffers."""
    layers = [_fold_layer(D, H, i) for i in range(n)]
    bufs = [tuple(t.clone() for t in L["pre"]) for L in layers]
    K.mhla_fold_bwd_multi([(L["dweff"], L["dbeff"], L["wqkv"], L["bqkv"], L["wl"], b) for L, b in zip(layers, bufs)], H)
    for i, (L, b) in enumerate(zip(layers, bufs)):
        one = _fold_bwd_single_acc(K, L, H)
        # each element of dwqkv / dbqkv has one owner and the same arithmetic in both launches
        assert torch.equal(b[0], one[0]) and torch.equal(b[1], one[1]), f"layer {i} of {n}"
        _close("fold", b[0], L["pre"][0].double() + L["grad_ref"][0], 2e-5, f"multi dwqkv layer {i} of {n}")
        # dwl / dbl are fp32 atomics over 2H x FOLD_L_SPLIT partial sums: not bitwise
        _close("fold", b[2], L["pre"][2].double() + L["grad_ref"][2], 2e-5, f"multi dwl layer {i} of {n}")
        _close("fold", b[3], L["pre"][3].double() + L["grad_ref"][3], 2e-5, f"multi dbl layer {i} of {n}")


@pytest.mark.parametrize("n", [3, 17])
@pytest.mark.parametrize("D,H", FOLD_GEOMS)
def test_fold_bwd_multi_frozen_qkv(K, D, H, n):
    """dwqkv = dbqkv = None for every layer (frozen qkv projection): only the latent_proj gradients, same values."""
    layers = [_fold_layer(D, H, i) for i in range(n)]
    bufs = [(None, None, L["pre"][2].clone(), L["pre"][3].clone()) for L in layers]
    K.mhla_fold_bwd_multi([(L["dweff"], L["dbeff"], L["wqkv"], L["bqkv"], L["wl"], b) for L, b in zip(layers, bufs)], H)
    for i, (L, b) in enumerate(zip(layers, bufs)):
        _close("fold", b[2], L["pre"][2].double() + L["grad_ref"][2], 2e-5, f"frozen dwl layer {i} of {n}")
        _close("fold", b[3], L["pre"][3].double() + L["grad_ref"][3], 2e-5, f"frozen dbl layer {i} of {n}")


@pytest.mark.parametrize("none_at", [0, 1])
def test_fold_bwd_multi_refuses_mixed_frozen_layers(K, none_at):
    D, H = 48, 3
    layers = [_fold_layer(D, H, i) for i in range(2)]
    bufs = [tuple(t.clone() for t in L["pre"]) for L in layers]
    bufs[none_at] = (None, None) + bufs[none_at][2:]
    before = [t.clone() for b in bufs for t in b if t is not None]
    _raises_code(-1, K.mhla_fold_bwd_multi,
                 [(L["dweff"], L["dbeff"], L["wqkv"], L["bqkv"], L["wl"], b) for L, b in zip(layers, bufs)], H)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip([t for b in bufs for t in b if t is not None], before))


def test_fold_refuses_unsupported_head_dim(K, favit):
    """hd = 8 has no instantiation: FAVIT_ERR_UNSUPPORTED from all four entry points and nothing launched (the
    non-accumulating single backward zero-fills dwl / dbl before its kernel: that fill must not run either)."""
    abi = favit._abi
    D, H, hd = 32, 4, 8
    g = _gen(5)
    wqkv, bqkv, wl, bl = _randn((3 * D, D), g), _randn((3 * D,), g), _randn((hd, hd), g), _randn((hd,), g)
    dweff, dbeff = _randn((3 * D, D), g), _randn((3 * D,), g)
    for dtype in (F32, BF16):
        _raises_code(-2, K.mhla_fold_fwd, wqkv, bqkv, wl, bl, H, dtype)
        _raises_code(-2, K.mhla_fold_fwd_multi, [(wqkv, bqkv, wl, bl)] * 2, H, dtype)
    _raises_code(-2, K.mhla_fold_bwd, dweff, dbeff, wqkv, bqkv, wl, H)
    out = [torch.full(s, 7.0, device=DEV) for s in ((3 * D, D), (3 * D,), (hd, hd), (hd,))]
    _raises_code(-2, K.mhla_fold_bwd, dweff, dbeff, wqkv, bqkv, wl, H, out=tuple(out))
    _raises_code(-2, K.mhla_fold_bwd_multi, [(dweff, dbeff, wqkv, bqkv, wl, tuple(out))] * 2, H)
    p = [C.c_void_p(t.data_ptr()) for t in (dweff, dbeff, wqkv, bqkv, wl, *out)]
    assert abi.lib().favit_mhla_fold_bwd(*p, D, H, 0, _st()) == abi.ERR_UNSUPPORTED      # accumulate = 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)


# --------------------------------------------------------------------------------------
# 3. LayerNorm backward: the forms the fused step uses
# --------------------------------------------------------------------------------------
# (8192 + 37, 64): nparts is capped at 2048, so the grid-stride row loop runs more than once, with a ragged last pass;
# (3, 2048): the widest supported row, one workgroup with an idle wave; (37, 68), the dropout case: D = 4 * 17, so the
# 4-element groups (two draws of the dropout counter each, element row*D + col) start at 0 and at 4 mod 8 in alternate rows
LN_SHAPES = [(37, 64), (700, 384), (8192 + 37, 64), (3, 2048)]
_LN_CACHE = {}


def _ln_case(K, rows, D, dtype, variant=0):
    """Inputs, saved statistics, the float64 layer_norm autograd reference and the ORDINARY backward call (fresh
    dgamma / dbeta, dres, low-precision copy) of one case; computed once and never written to."""
    key = (rows, D, dtype, variant)
    if key in _LN_CACHE:
        return _LN_CACHE[key]
    g = _gen(rows * 131 + D * 17 + variant * 7919 + (1 if dtype == BF16 else 0))
    c = {"x": _randn((rows, D), g, shift=0.5, scale=2.0), "gam": _randn((D,), g, shift=0.5), "bet": _randn((D,), g),
         "dy": _randn((rows, D), g, shift=0.5).to(dtype), "dres": _randn((rows, D), g),
         "pre_g": _randn((D,), g), "pre_b": _randn((D,), g)}
    _, c["mu"], c["rs"] = K.layernorm_fwd(c["x"], D, c["gam"], c["bet"], rows, D, F32)
    xr, gr, br = [c[k].double().requires_grad_(True) for k in ("x", "gam", "bet")]
    torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-5).backward(c["dy"].double())
    c["dx_ref"], c["dg_ref"], c["db_ref"] = xr.grad + c["dres"].double(), gr.grad, br.grad
    c["plain"] = K.layernorm_bwd(c["dy"], c["x"], D, c["gam"], c["mu"], c["rs"], rows, D, dres=c["dres"], want_lp=True)
    _LN_CACHE[key] = c
    return c


def _ln_bwd(K, c, rows, D, **kw):
    return K.layernorm_bwd(c["dy"], c["x"], D, c["gam"], c["mu"], c["rs"], rows, D, dres=c["dres"], want_lp=True, **kw)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,D", LN_SHAPES + [(37, 68)])
def test_ln_bwd_ordinary_call_at_the_new_shapes(K, rows, D, dtype):
    c = _ln_case(K, rows, D, dtype)
    dx, dx_lp, dg, db = c["plain"]
    _close("layernorm", dx, c["dx_ref"], 2e-5, "dx")
    _close("layernorm", dx_lp.float(), c["dx_ref"], _tol(dtype), "dx_lp")
    _close("layernorm", dg, c["dg_ref"], 2e-5, "dgamma")
    _close("layernorm", db, c["db_ref"], 2e-5, "dbeta")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_ln_bwd_accumulates_into_gradient_buffers(K, rows, D, dtype):
    """accumulate = 1: the fold runs with the partial rows split eight ways and fp32 atomics onto the buffers."""
    c = _ln_case(K, rows, D, dtype)
    bg, bb = c["pre_g"].clone(), c["pre_b"].clone()
    dx, dx_lp, dg, db = _ln_bwd(K, c, rows, D, dg_out=bg, db_out=bb)
    assert dg is None and db is None
    _close("layernorm", bg, c["pre_g"].double() + c["dg_ref"], 2e-5, "accumulated dgamma")
    _close("layernorm", bb, c["pre_b"].double() + c["db_ref"], 2e-5, "accumulated dbeta")
    assert torch.equal(dx, c["plain"][0]) and torch.equal(dx_lp, c["plain"][1])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_ln_bwd_deferred_fold(K, rows, D, dtype):
    """defer: no fold launch (dgamma = NULL); three deferred calls are folded by ONE reduce_rows_multi."""
    cases = [_ln_case(K, rows, D, dtype, v) for v in range(3)]
    bufs = [(c["pre_g"].clone(), c["pre_b"].clone()) for c in cases]
    lst = []
    for i, (c, (bg, bb)) in enumerate(zip(cases, bufs)):
        dx, dx_lp, dg, db = _ln_bwd(K, c, rows, D, dg_out=bg, db_out=bb, defer=lst)
        assert dg is None and db is None and len(lst) == i + 1
        part, o0, o1 = lst[-1]
        assert o0 is bg and o1 is bb and tuple(part.shape) == (2, min(2048, (rows + 3) // 4), D)
        assert torch.equal(bg, c["pre_g"]) and torch.equal(bb, c["pre_b"]), "a deferred call leaves the buffers alone"
        assert torch.equal(dx, c["plain"][0]) and torch.equal(dx_lp, c["plain"][1])
    K.reduce_rows_multi(lst)
    for i, (c, (bg, bb)) in enumerate(zip(cases, bufs)):
        _close("layernorm", bg, c["pre_g"].double() + c["dg_ref"], 2e-5, f"deferred dgamma of call {i}")
        _close("layernorm", bb, c["pre_b"].double() + c["db_ref"], 2e-5, f"deferred dbeta of call {i}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_ln_bwd_frozen_affine(K, rows, D, dtype):
    c = _ln_case(K, rows, D, dtype)
    dx, dx_lp, dg, db = _ln_bwd(K, c, rows, D, frozen=True)
    assert dg is None and db is None
    assert torch.equal(dx, c["plain"][0]) and torch.equal(dx_lp, c["plain"][1])
    # frozen wins over gradient buffers: they are not touched
    bg, bb = c["pre_g"].clone(), c["pre_b"].clone()
    _ln_bwd(K, c, rows, D, frozen=True, dg_out=bg, db_out=bb)
    assert torch.equal(bg, c["pre_g"]) and torch.equal(bb, c["pre_b"])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,D", LN_SHAPES + [(37, 68)])
def test_ln_bwd_dropout_mask_on_the_low_precision_copy(K, rows, D, dtype):
    """lp_drop: dx stays unmasked, dx_lp carries exactly the mask and scale of favit_dropout (element row*D + col).
    With test_gemm_dropout_epilogue_matches_dropout_kernel this ties the backward mask to the forward's."""
    c = _ln_case(K, rows, D, dtype)
    p, seed = 0.25, 0x5EED0000 + rows
    dx, dx_lp, dg, db = _ln_bwd(K, c, rows, D, lp_drop=(p, seed))
    assert torch.equal(dx, c["plain"][0]), "dx is not masked"
    assert torch.equal(dg, c["plain"][2]) and torch.equal(db, c["plain"][3])
    want = K.dropout(dx, p, seed)
    assert torch.equal(dx_lp, want if dtype == F32 else want.to(BF16))
    drop = (want == 0).float().mean().item()
    assert abs(drop - p) < 5 * (p * (1 - p) / (rows * D)) ** 0.5, "five sigma of the Bernoulli mean"
    assert not torch.equal(dx_lp, _ln_bwd(K, c, rows, D, lp_drop=(p, seed + 1))[1])


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("B,L,D", [(37, 5, 64), (6, 17, 384)])
def test_ln_bwd_strided_dx_of_the_cls_head(K, B, L, D, with_dres):
    """The CLS-head call: x and dx are [B, L, D] streams, rows = B, ldx = lddx = L*D; only rows [:, 0] are written.
    dres is read with the stride of dx (lddx): an equally strided [B, L, D] tensor whose rows [:, 0] are added."""
    g = _gen(B * 1000 + L * 10 + D + int(with_dres))
    x = _randn((B, L, D), g, shift=0.5, scale=2.0)
    gam, bet = _randn((D,), g, shift=0.5), _randn((D,), g)
    dy = _randn((B, D), g, shift=0.5)
    dres = _randn((B, L, D), g) if with_dres else None
    pre_g, pre_b = _randn((D,), g), _randn((D,), g)
    _, mu, rs = K.layernorm_fwd(x, L * D, gam, bet, B, D, F32)
    xr, gr, br = [t.double().requires_grad_(True) for t in (x, gam, bet)]
    torch.nn.functional.layer_norm(xr[:, 0], (D,), gr, br, 1e-5).backward(dy.double())
    dx_ref = xr.grad[:, 0] + (dres[:, 0].double() if with_dres else 0.0)
    sentinel = -12345.678
    dx = torch.full((B, L, D), sentinel, device=DEV)
    bg, bb = pre_g.clone(), pre_b.clone()
    got, lp, dg, db = K.layernorm_bwd(dy, x, L * D, gam, mu, rs, B, D, dres=dres, dx=dx, lddx=L * D, dg_out=bg, db_out=bb)
    assert got is dx and lp is None and dg is None and db is None
    _close("layernorm", dx[:, 0], dx_ref, 2e-5, "strided dx rows [:, 0]")
    assert bool((dx[:, 1:] == torch.tensor(sentinel, device=DEV)).all()), "rows other than [:, 0] were written"
    _close("layernorm", bg, pre_g.double() + gr.grad, 2e-5, "dgamma")
    _close("layernorm", bb, pre_b.double() + br.grad, 2e-5, "dbeta")


def test_ln_refuses_too_wide_rows(K):
    """D = 2052 (a multiple of 4 above the widest instantiation, 2048): FAVIT_ERR_UNSUPPORTED, nothing launched."""
    rows, D = 3, 2052
    g = _gen(2052)
    x, gam, bet = _randn((rows, D), g), _randn((D,), g), _randn((D,), g)
    for dtype in (F32, BF16):
        _raises_code(-2, K.layernorm_fwd, x, D, gam, bet, rows, D, dtype)
    mu, rs = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
    dx = torch.full((rows, D), 7.0, device=DEV)
    bg, bb = torch.full((D,), 7.0, device=DEV), torch.full((D,), 7.0, device=DEV)
    for dtype in (F32, BF16):
        _raises_code(-2, K.layernorm_bwd, _randn((rows, D), g).to(dtype), x, D, gam, mu, rs, rows, D, dx=dx, lddx=D,
                     want_lp=True, dg_out=bg, db_out=bb)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (dx, bg, bb))


# --------------------------------------------------------------------------------------
# 4. Smaller neighbours: pos-less embedding prologue, unfused softmax with key-keep mask and dropout
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(3, 16, 64), (33, 5, 8)])
def test_embed_prologue_fwd_without_pos(K, B, N, D):
    g = _gen(B + N + D)
    tok, cls = _randn((B, N, D), g), _randn((D,), g)
    x = K.embed_prologue_fwd(tok, cls, None, B, N, D)
    assert torch.equal(x, torch.cat([cls.expand(B, 1, D), tok], 1))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("want_pos", [False, True])
@pytest.mark.parametrize("B,N,D", [(33, 5, 8), (130, 3, 12), (31, 5, 8)])
def test_embed_prologue_bwd_ragged_chunks_and_no_dpos(K, B, N, D, want_pos, dtype):
    """B = 33 / 130: the chunked kernel with 4 / 16 batch chunks that do not divide B (130: the last chunk is empty);
    B = 31: the serial kernel just below the switch.  want_pos=False: dpos = NULL (the SPPP models)."""
    dx = _randn((B, N + 1, D), _gen(B * 100 + N * 10 + D), shift=0.5)
    dtok, dcls, dpos = K.embed_prologue_bwd(dx, B, N, D, dtype, want_pos=want_pos)
    assert dtok.dtype == dtype and torch.equal(dtok.reshape(B, N, D), dx[:, 1:].to(dtype))
    _close("rest", dcls, dx[:, 0].double().sum(0), 1e-6, "dcls")
    if want_pos:
        _close("rest", dpos, dx.double().sum(0), 1e-6, "dpos")
    else:
        assert dpos is None


SOFTMAX_SHAPES = [(6, 9, 70, 3), (4, 5, 64, 2), (2, 7, 3, 1)]      # Lk above / at / below one wave; 54 and 14 rows: a ragged last workgroup


def _softmax_case(Z, Lq, Lk, H):
    g = _gen(Z * 1000 + Lq * 100 + Lk)
    S = _randn((Z, Lq, Lk), g, scale=3.0)
    keep_keys = torch.rand((Z // H, Lk), generator=g, device=DEV) > 0.3          # [B, Lk]: m_sb = Lk, m_sq = 0
    keep_keys[:, 0] = True
    full = keep_keys.repeat_interleave(H, 0)[:, None, :].expand(Z, Lq, Lk)
    return S, keep_keys.to(torch.uint8).contiguous(), full, _randn((Z, Lq, Lk), g, shift=0.5)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Z,Lq,Lk,H", SOFTMAX_SHAPES)
def test_softmax_key_keep_mask(K, Z, Lq, Lk, H, dtype):
    S, mask, full, dP = _softmax_case(Z, Lq, Lk, H)
    P, Pd = K.softmax_fwd(S, dtype, H, Z, Lq, Lk, mask, Lk, 0)
    assert Pd is P
    Sr = S.double().requires_grad_(True)
    ref = torch.softmax(Sr.masked_fill(~full, float("-inf")), -1)
    _close("rest", P.float(), ref, _tol(dtype), "softmax with a key-keep mask")
    assert bool((P[~full] == 0).all())
    dS = K.softmax_bwd(P, dP, Z, Lq, Lk)
    if dtype == F32:
        (ref * dP.double()).sum().backward()
        want = Sr.grad
    else:       # the input of the backward is the bf16-rounded P: the reference starts from it
        Pr = P.double()
        want = Pr * (dP.double() - (Pr * dP.double()).sum(-1, keepdim=True))
    _close("rest", dS.float(), want, _tol(dtype), "softmax backward")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Z,Lq,Lk,H", SOFTMAX_SHAPES)
def test_softmax_dropout(K, Z, Lq, Lk, H, dtype):
    S, mask, full, dPd = _softmax_case(Z, Lq, Lk, H)
    p, seed = 0.3, 4242 + Lk
    P0, _ = K.softmax_fwd(S, dtype, H, Z, Lq, Lk, mask, Lk, 0)
    P, Pd = K.softmax_fwd(S, dtype, H, Z, Lq, Lk, mask, Lk, 0, p, seed)
    assert Pd is not P and torch.equal(P, P0), "P is the undropped softmax"
    keep = K.dropout(torch.ones((Z, Lq, Lk), device=DEV), p, seed) != 0          # element index row*Lk + k
    assert torch.equal(Pd == 0, ~keep | (P == 0)), "Pd is zero exactly where the dropout kernel drops (or P is masked)"
    # elsewhere Pd = P / (1 - p) to output rounding: fp32 stores P exactly, so only 1/(1-p) and the product round
    # (2 * 2^-24 < 1e-6); bf16 rounds P and Pd separately (the 1e-2 gate of bf16 outputs)
    _close("rest", Pd.float()[keep], P.double()[keep] / (1 - p), 1e-6 if dtype == F32 else 1e-2, "kept Pd")
    dS = K.softmax_bwd(P, dPd, Z, Lq, Lk, p, seed)
    scale = keep.double() / (1 - p)
    if dtype == F32:
        Sr = S.double().requires_grad_(True)
        (torch.softmax(Sr.masked_fill(~full, float("-inf")), -1) * scale * dPd.double()).sum().backward()
        want = Sr.grad
    else:
        Pr, dp = P.double(), dPd.double() * scale
        want = Pr * (dp - (Pr * dp).sum(-1, keepdim=True))
    _close("rest", dS.float(), want, _tol(dtype), "softmax backward through dropout")
    _, Pd2 = K.softmax_fwd(S, dtype, H, Z, Lq, Lk, mask, Lk, 0, p, seed + 1)
    assert not torch.equal(Pd2, Pd), "another seed, another mask"
