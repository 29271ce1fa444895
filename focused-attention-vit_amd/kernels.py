"""Tensor-level wrappers over the C ABI (include/favit.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
function below hands raw device pointers to libfavit.so.  All tensors must live on a
ROCm device; there is no CPU path (the oracle in ``oracle/`` is test infrastructure and
is never imported from the product).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _abi
from ._abi import ACT_DGELU, ACT_GELU, ACT_NONE, BF16, F32, GemmDesc, SdpaDesc

_DT = {torch.float32: F32, torch.bfloat16: BF16}

# in_dtype that gemm() gives a problem with fp32 operands: F32 (exact f32 MFMA) or F32X3 (the split-bf16 product of the
# 'fp32x3' compute mode).  functional.set_compute_dtype owns it; small_linear_* and the attention kernels never see it.
_F32_GEMM = {"in_dtype": F32}


def set_f32_gemm_split(on: bool) -> None:
    _F32_GEMM["in_dtype"] = _abi.F32X3 if on else F32

# bench.py sets this to a list to time every favit_gemm launch with HIP events recorded on the
# stream the kernel is launched on (torch's current stream): entries are
# (start_event, end_event, algorithmic_flops, kernel_key, shape, kernel family the library dispatched to).
GEMM_TRACE = None


def dt(t_or_dtype) -> int:
    d = t_or_dtype.dtype if torch.is_tensor(t_or_dtype) else t_or_dtype
    try:
        return _DT[d]
    except KeyError:
        raise TypeError(f"favit kernels support float32 / bfloat16 only, got {d}") from None


def require_gpu(*ts):
    """Every tensor must live on the CURRENT ROCm device: kernels are launched on the current device's
    current stream (_st), so a tensor of another device would be dereferenced on the wrong GPU."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "focused-attention-vit_amd runs its hot path in HIP kernels on an MI355X; got a CPU tensor. "
                "There is no CPU fallback (move the module and its inputs to the GPU).")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(
                f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: one process drives one GPU "
                "(torch.cuda.set_device(local_rank) before building the model), or wrap the call in "
                "`with torch.cuda.device(t.device):`")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _st():
    """The current stream's handle.  Every wrapper asks for it (about 80 times per cfg2 step), so where torch has the
    raw accessor it is used: no Stream object is built (1 us instead of 4)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------------------
def gemm(A, B, Cc, M, N, K, lda, ldb, ldc, *, a_kmajor=True, b_kmajor=True, bias=None, act=ACT_NONE,
         aux_in=None, ld_aux_in=0, aux_out=None, ld_aux_out=0, residual=None, ld_res=0, a_rowsum=None,
         accumulate=False, alpha=1.0, batch=1, batch_inner=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), split_k=0,
         a_off=0, b_off=0, c_off=0, dropout_p=0.0, dropout_seed=0, scale_a=None, scale_b=None, in_dtype=None):
    """C[m,n] = epilogue(alpha * sum_k A[m,k] B[n,k]).  Offsets/strides are in elements.
    in_dtype (fp32 operands only): _abi.F32 or _abi.F32X3 for this call, whatever the compute mode says.
    float8 operands (A e4m3 / e5m2, B e4m3; both k-major): scale_a / scale_b are the device scalars
    written by fp8_quantize."""
    require_gpu(A, B, Cc)
    fp8 = A.dtype in _FP8_DT
    if fp8:
        if B.dtype != torch.float8_e4m3fn:
            raise TypeError("fp8 gemm: B must be float8_e4m3fn")
    elif A.dtype != B.dtype:
        raise TypeError("gemm operands must share a dtype")
    d = GemmDesc()
    ea, ec = A.element_size(), Cc.element_size()
    d.A = A.data_ptr() + a_off * ea
    d.B = B.data_ptr() + b_off * ea
    d.C = Cc.data_ptr() + c_off * ec
    d.bias = bias.data_ptr() if bias is not None else None
    d.aux_in = aux_in.data_ptr() if aux_in is not None else None
    d.aux_out = aux_out.data_ptr() if aux_out is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.a_rowsum = a_rowsum.data_ptr() if a_rowsum is not None else None
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.ld_aux_in, d.ld_aux_out, d.ld_res = ld_aux_in, ld_aux_out, ld_res
    d.sAo, d.sAi = sA
    d.sBo, d.sBi = sB
    d.sCo, d.sCi = sC
    d.batch, d.batch_inner = batch, batch_inner
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.in_dtype, d.out_dtype = (_abi.FP8 if fp8 else dt(A)), dt(Cc)
    if d.in_dtype == F32:
        d.in_dtype = _F32_GEMM["in_dtype"] if in_dtype is None else in_dtype
    elif in_dtype is not None:
        raise TypeError("in_dtype selects the product of fp32 operands only")
    if fp8:
        d.fp8_fmt = 1 if A.dtype == torch.float8_e5m2 else 0
        d.scale_a = scale_a.data_ptr() if scale_a is not None else None
        d.scale_b = scale_b.data_ptr() if scale_b is not None else None
    d.act = act
    d.accumulate = int(accumulate)
    d.split_k = split_k
    d.alpha = alpha
    d.dropout_p = dropout_p
    d.dropout_seed = dropout_seed
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("bias must be fp32")
    if residual is not None and residual.dtype != torch.float32:
        raise TypeError("residual must be fp32")
    if GEMM_TRACE is None:
        _abi.check(_abi.lib().favit_gemm(C.byref(d), _st()), "favit_gemm")
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _abi.check(_abi.lib().favit_gemm(C.byref(d), _st()), "favit_gemm")
    e1.record()
    key = ("fp8" if fp8 else "bf16" if A.dtype == torch.bfloat16 else "f32x3" if d.in_dtype == _abi.F32X3 else "f32") + ("_K" if a_kmajor else "_M") + ("K" if b_kmajor else "M") + \
          ("_obf16" if Cc.dtype == torch.bfloat16 else "_of32")
    GEMM_TRACE.append((e0, e1, 2.0 * M * N * K * batch, key, (M, N, K, batch), _abi.lib().favit_gemm_last_kernel().decode()))


def ln_gemm(x, ldx, gamma, beta, w, out, M, N, D, *, bias=None, act=ACT_NONE, aux_in=None, ld_aux_in=0, aux_out=None,
            residual=None, dropout_p=0.0, dropout_seed=0, eps=1e-5):
    """out = epilogue(LayerNorm(x) @ w^T) in one launch (favit_ln_gemm); returns (xn bf16 [M, D], mean, rstd), or None
    when the library declines the shape (the caller then runs layernorm_fwd + gemm)."""
    require_gpu(x, gamma, beta, w, out)
    if w.dtype != torch.bfloat16 or x.dtype != torch.float32:
        return None
    d = GemmDesc()
    d.A = None
    d.B, d.C = w.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.aux_in = aux_in.data_ptr() if aux_in is not None else None
    d.aux_out = aux_out.data_ptr() if aux_out is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.M, d.N, d.K = M, N, D
    d.lda, d.ldb, d.ldc = D, w.stride(0), out.stride(0)
    d.ld_aux_in, d.ld_aux_out, d.ld_res = ld_aux_in, N, N
    d.batch, d.batch_inner = 1, 1
    d.a_kmajor, d.b_kmajor = 1, 1
    d.in_dtype, d.out_dtype = BF16, dt(out)
    d.act, d.alpha = act, 1.0
    d.dropout_p, d.dropout_seed = dropout_p, dropout_seed
    xn = torch.empty((M, D), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    if GEMM_TRACE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = _abi.lib().favit_ln_gemm(C.byref(d), _p(x), ldx, _p(gamma), _p(beta), eps, _p(xn), _p(mean), _p(rstd), _st())
    if rc == _abi.ERR_UNSUPPORTED:
        return None
    _abi.check(rc, "favit_ln_gemm")
    if GEMM_TRACE is not None:
        e1.record()
        GEMM_TRACE.append((e0, e1, 2.0 * M * N * D, "bf16_KK_" + ("obf16" if out.dtype == torch.bfloat16 else "of32"),
                           (M, N, D, 1), "s64ln"))
    return xn, mean, rstd


_GROUPED_WS = {}          # device index -> workspace tensor of the slab-mode split-K reduction
# Workspaces that were outgrown stay alive: a captured HIP graph holds their ADDRESS (train.GraphedStep: one graph per
# token-count bucket, the second bucket can need a larger workspace than the first), and torch.cuda.graph() empties the
# allocator cache when the next capture begins -- a freed workspace is then unmapped under the first graph's replays
# (memory access fault; found with the two-bucket cfg5 bench once its one-problem launches took the slab path).
_GROUPED_WS_RETIRED = []


GROUP_MAX = _abi.GEMM_GROUP_MAX            # problems per grouped launch (include/favit.h)


def gemm_grouped_tn(problems, use_workspace: bool = True) -> bool:
    """One launch for several weight-gradient GEMMs dW = dY^T X that share the token dim (more than GROUP_MAX problems:
    consecutive launches of GROUP_MAX).
    problems: list of (dy [T,N], a [T,K], dw [N,K] fp32, db [N] fp32 or None, accumulate: bool).
    Returns False if the library cannot group them (caller falls back to single launches).
    use_workspace: when the library splits the token dimension, the partial results of the K-splits go through a
    cached device workspace and are summed in a fixed order (deterministic, no fp32 atomics); False keeps the atomic
    path.  With enough tiles in the launch there is ONE split and the tiles write dW themselves (no workspace)."""
    if len(problems) > GROUP_MAX:
        T = problems[0][0].shape[0]
        if any(p[0].shape[0] != T or p[0].dtype != torch.bfloat16 or p[1].dtype != torch.bfloat16 for p in problems) or T % 32:
            return False                               # decline as a whole: never half a list
        for i in range(0, len(problems), GROUP_MAX):
            if not gemm_grouped_tn(problems[i:i + GROUP_MAX], use_workspace):
                raise RuntimeError("grouped weight-gradient launch declined a chunk after launching another")
        return True
    return _grouped_launch(problems, use_workspace, False)


def gemm_grouped_tn_ragged(problems, use_workspace: bool = True) -> bool:
    """gemm_grouped_tn for problems whose token counts differ (the blocks of a pruned encoder in one launch): the
    library plans K-splits per chunk of problems that share a token count, splits the long blocks into slabs of the
    workspace and lets the short ones write dW themselves.  Every token count must be a multiple of 32 and the list at
    most GROUP_MAX long; returns False (nothing launched) otherwise, and the caller falls back."""
    if len(problems) > GROUP_MAX:
        return False
    return _grouped_launch(problems, use_workspace, True)


def _grouped_launch(problems, use_workspace, ragged):
    n = len(problems)
    if n == 0:
        return True
    L = _abi.lib()
    f_query, f_ws, f_plain = ((L.favit_gemm_grouped_tn_ragged_workspace, L.favit_gemm_grouped_tn_ragged_ws,
                               L.favit_gemm_grouped_tn_ragged) if ragged else
                              (L.favit_gemm_grouped_tn_workspace, L.favit_gemm_grouped_tn_ws, L.favit_gemm_grouped_tn))
    arr = (GemmDesc * n)()
    T = problems[0][0].shape[0]
    for d, (dy, a, dw, db, acc) in zip(arr, problems):
        require_gpu(dy, a, dw)
        if dy.dtype != torch.bfloat16 or a.dtype != torch.bfloat16 or dw.dtype != torch.float32:
            return False
        if a.shape[0] != dy.shape[0] or (dy.shape[0] != T and not ragged):
            return False
        T_i = dy.shape[0]
        N, Kd = dy.shape[1], a.shape[1]
        d.A, d.B, d.C = dy.data_ptr(), a.data_ptr(), dw.data_ptr()
        d.a_rowsum = db.data_ptr() if db is not None else None
        d.M, d.N, d.K = N, Kd, T_i
        d.lda, d.ldb, d.ldc = dy.stride(0), a.stride(0), dw.stride(0)
        d.batch, d.batch_inner = 1, 1
        d.a_kmajor, d.b_kmajor = 0, 0
        d.in_dtype, d.out_dtype = BF16, F32
        d.act, d.accumulate, d.split_k = ACT_NONE, int(acc), 0
        d.alpha, d.dropout_p, d.dropout_seed = 1.0, 0.0, 0
    if GEMM_TRACE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    need = int(f_query(arr, n)) if use_workspace else 0
    if need > 0:
        dev = problems[0][0].device
        ws = _GROUPED_WS.get(dev.index)
        if ws is None or ws.numel() < need:
            if ws is not None:
                _GROUPED_WS_RETIRED.append(ws)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _GROUPED_WS[dev.index] = ws
        rc = f_ws(arr, n, _p(ws), ws.numel(), _st())
    else:
        rc = f_plain(arr, n, _st())
    if rc == _abi.ERR_UNSUPPORTED:
        return False
    _abi.check(rc, "favit_gemm_grouped_tn")
    if GEMM_TRACE is not None:
        e1.record()
        fl = sum(2.0 * p[0].shape[0] * p[0].shape[1] * p[1].shape[1] for p in problems)
        GEMM_TRACE.append((e0, e1, fl, "bf16_MM_of32_grouped", (len(problems), int(_abi.lib().favit_gemm_grouped_last_splits())),
                           "grouped_tn"))
    return True


_FP8_DT = (torch.float8_e4m3fn, torch.float8_e5m2)


class Fp8History:
    """Delayed per-tensor scaling state of one quantisation site: three rotating amax slots (this call's scale
    comes from the amax the previous call measured; this call measures into the next slot and clears the one
    after) and the scale_inv scalar the GEMM reads."""
    __slots__ = ("slots", "scale_inv", "calls")

    NSLOT = _abi.FP8_AMAX_SLOTS                   # partial maxima per array

    def __init__(self, device):
        self.slots = torch.zeros(3 * self.NSLOT, dtype=torch.float32, device=device)
        self.scale_inv = torch.ones(1, dtype=torch.float32, device=device)
        self.calls = 0


def fp8_quantize(src: torch.Tensor, fmt: torch.dtype, *, want=True, want_t=False, colsum: Optional[torch.Tensor] = None,
                 hist: Optional[Fp8History] = None):
    """Per-tensor scaled conversion of a [rows, cols] fp32 / bf16 matrix to OCP fp8 (`fmt` =
    torch.float8_e4m3fn | torch.float8_e5m2).  Returns (q [rows, cols] or None, q_t [cols, ld_t] or None
    with ld_t = rows rounded up to 64 and the pad zero-filled, scale_inv device scalar).  Without `hist` the amax is
    taken on the device in the same call sequence (a separate pass, no host sync).  With `hist` (delayed scaling) the
    scale comes from the amax the site's previous call measured and this call measures the next one while it
    quantises: one pass over the tensor; values beyond the previous amax saturate.  colsum [cols] fp32 (optional) gets
    the column sums of src ADDED (bias gradient)."""
    require_gpu(src)
    if src.dim() != 2 or src.stride(1) != 1:
        raise ValueError("fp8_quantize expects a row-major 2-D matrix")
    rows, cols = src.shape
    dev = src.device
    L = _abi.lib()
    q = torch.empty((rows, cols), dtype=fmt, device=dev) if want else None
    ld_t = (rows + 63) // 64 * 64
    q_t = torch.empty((cols, ld_t), dtype=fmt, device=dev) if want_t else None
    f8 = _abi.E5M2 if fmt == torch.float8_e5m2 else _abi.E4M3
    if hist is None:
        st = torch.zeros(2, dtype=torch.float32, device=dev)        # [amax, scale_inv]
        _abi.check(L.favit_fp8_amax(_p(src), dt(src), rows, cols, src.stride(0), _p(st), _st()), "favit_fp8_amax")
        _abi.check(L.favit_fp8_quantize(_p(src), dt(src), rows, cols, src.stride(0), _p(q), cols, _p(q_t), ld_t, f8,
                                        _p(st), C.c_void_p(st.data_ptr() + 4), _p(colsum), None, None, _st()),
                   "favit_fp8_quantize")
        return q, q_t, st[1:2]
    base = hist.slots.data_ptr()
    stride = 4 * hist.NSLOT
    cur, nxt, clr = hist.calls % 3, (hist.calls + 1) % 3, (hist.calls + 2) % 3
    if hist.calls == 0:                                             # no history yet: measure this tensor first
        _abi.check(L.favit_fp8_amax(_p(src), dt(src), rows, cols, src.stride(0), C.c_void_p(base + stride * cur), _st()),
                   "favit_fp8_amax")
    hist.calls += 1
    sinv = torch.empty(1, dtype=torch.float32, device=dev)          # per call: the GEMM reads it after later calls
    _abi.check(L.favit_fp8_quantize(_p(src), dt(src), rows, cols, src.stride(0), _p(q), cols, _p(q_t), ld_t, f8,
                                    C.c_void_p(base + stride * cur), _p(sinv), _p(colsum), C.c_void_p(base + stride * nxt),
                                    C.c_void_p(base + stride * clr), _st()), "favit_fp8_quantize")
    return q, q_t, sinv


def cast(src: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    require_gpu(src)
    src = src.contiguous()
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    _abi.check(_abi.lib().favit_cast(_p(src), dt(src), _p(out), dt(out), src.numel(), _st()), "favit_cast")
    return out


def _q8_slots(hist: "Fp8History"):
    """Rotate a delayed-scaling history by one call: (amax, amax_next, amax_clear) pointers of THIS call."""
    base, stride = hist.slots.data_ptr(), 4 * hist.NSLOT
    cur, nxt, clr = hist.calls % 3, (hist.calls + 1) % 3, (hist.calls + 2) % 3
    hist.calls += 1
    return C.c_void_p(base + stride * cur), C.c_void_p(base + stride * nxt), C.c_void_p(base + stride * clr)


def _q8_fused_ok(q8, out_dtype, D) -> bool:
    """A LayerNorm pass may quantise its bf16 output for the consumer site: the site has a measured amax (its first
    call takes the two-pass form, which measures before it scales) and the rows are whole 4-byte groups."""
    return q8 is not None and q8[1] is not None and q8[1].calls > 0 and out_dtype == torch.bfloat16 and D % 4 == 0


def layernorm_fwd(x, ldx, gamma, beta, rows, D, out_dtype, eps=1e-5, q8=None):
    """x: fp32 rows with stride ldx -> y [rows, D] (out_dtype), mean, rstd.
    q8 = (fp8 dtype, Fp8History of the consumer GEMM's operand site) in fp8 mode: y also leaves the pass quantised
    (favit_layernorm_fwd_q8) and the result is parked on the tensor where functional._q8 finds it."""
    require_gpu(x, gamma, beta)
    y = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    if _q8_fused_ok(q8, out_dtype, D):
        fmt, hist = q8
        q = torch.empty((rows, D), dtype=fmt, device=x.device)
        sinv = torch.empty(1, dtype=torch.float32, device=x.device)
        cur, nxt, clr = _q8_slots(hist)
        _abi.check(_abi.lib().favit_layernorm_fwd_q8(_p(x), ldx, _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D, eps,
                                                     _p(q), _abi.E5M2 if fmt == torch.float8_e5m2 else _abi.E4M3, cur,
                                                     _p(sinv), nxt, clr, _st()), "favit_layernorm_fwd_q8")
        y._favit_q8 = ((fmt, y._version), (q, None, sinv))
        return y, mean, rstd
    _abi.check(_abi.lib().favit_layernorm_fwd(_p(x), ldx, _p(gamma), _p(beta), _p(y), dt(y), _p(mean), _p(rstd),
                                              rows, D, eps, _st()), "favit_layernorm_fwd")
    return y, mean, rstd


SMALL_LINEAR_MAX_N = _abi.SMALL_LINEAR_MAX_N


def small_linear_fwd(x, w, bias):
    """y = x @ w.T + bias in exact fp32 (x [M, K] fp32 contiguous rows, w [N, K] fp32, N <= 64): the classification head."""
    require_gpu(x, w)
    M, Kd = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().favit_small_linear_fwd(_p(x), x.stride(0), _p(w), _p(bias), _p(y), M, N, Kd, _st()),
               "favit_small_linear_fwd")
    return y


def small_linear_bwd(dy, x, w, *, want_dx=True, dw_out=None, db_out=None, want_db=True):
    """(dx or None, dw or None, db or None) of small_linear_fwd.  dw_out / db_out: fp32 gradient buffers the results are
    ACCUMULATED into (then None is returned in their place)."""
    require_gpu(dy, x, w)
    M, Kd = x.shape
    N = w.shape[0]
    dev = x.device
    dx = torch.empty((M, Kd), dtype=torch.float32, device=dev) if want_dx else None
    acc = dw_out is not None and (db_out is not None or not want_db)
    dw = dw_out if acc else torch.empty((N, Kd), dtype=torch.float32, device=dev)
    db = (db_out if acc else torch.empty(N, dtype=torch.float32, device=dev)) if want_db else None
    _abi.check(_abi.lib().favit_small_linear_bwd(_p(dy), _p(x), x.stride(0), _p(w), _p(dx), _p(dw), _p(db), int(acc), M, N, Kd,
                                                 _st()), "favit_small_linear_bwd")
    return dx, (None if acc else dw), (None if (acc or not want_db) else db)


def layernorm_bwd(dy, x, ldx, gamma, mean, rstd, rows, D, *, dres=None, dx=None, lddx=None, want_lp=False,
                  dg_out=None, db_out=None, lp_drop=(0.0, 0), defer=None, frozen=False, q8=None):
    """Returns dx (fp32, row stride lddx), dx_lp (dy.dtype copy or None), dgamma, dbeta.
    dg_out / db_out: optional fp32 [D] gradient buffers the affine gradients are ACCUMULATED into
    (then None is returned in their place).  lp_drop = (p, seed): dx_lp carries that dropout mask (the branch it
    feeds had its output dropped in forward), saving a separate masking pass.
    defer (a list, with dg_out / db_out): the fold of the partial sums into dg_out / db_out is NOT launched; the
    entry (part, dg_out, db_out) is appended and the caller folds several of them in one launch (reduce_rows_multi).
    frozen: gamma and beta take no gradient (fine-tuning with frozen layers): no fold launch at all, (.., None, None).
    q8 = (fp8 dtype, Fp8History) in fp8 mode: dx_lp also leaves the pass quantised (see layernorm_fwd)."""
    require_gpu(dy, x)
    dev = x.device
    if dx is None:
        dx = torch.empty((rows, D), dtype=torch.float32, device=dev)
        lddx = D
    dx_lp = torch.empty((rows, D), dtype=dy.dtype, device=dev) if want_lp else None
    nparts = int(min(2048, (rows + 3) // 4))
    part = torch.empty((2, nparts, D), dtype=torch.float32, device=dev)
    acc = dg_out is not None and db_out is not None
    if frozen:
        acc, dg, db = True, None, None
    elif acc and defer is not None:
        defer.append((part, dg_out, db_out))
        dg = db = None
    elif acc:
        dg, db = dg_out, db_out
    else:
        dgb = torch.empty((2, D), dtype=torch.float32, device=dev)
        dg, db = dgb[0], dgb[1]
    if want_lp and _q8_fused_ok(q8, dy.dtype, D):
        fmt, hist = q8
        q = torch.empty((rows, D), dtype=fmt, device=dev)
        sinv = torch.empty(1, dtype=torch.float32, device=dev)
        cur, nxt, clr = _q8_slots(hist)
        _abi.check(_abi.lib().favit_layernorm_bwd_q8(_p(dy), _p(x), ldx, _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), lddx,
                                                     _p(dx_lp), _p(part[0]), _p(part[1]), nparts, _p(dg), _p(db), int(acc), rows, D,
                                                     float(lp_drop[0]), int(lp_drop[1]) & ((1 << 64) - 1), _p(q),
                                                     _abi.E5M2 if fmt == torch.float8_e5m2 else _abi.E4M3, cur, _p(sinv), nxt, clr,
                                                     _st()), "favit_layernorm_bwd_q8")
        dx_lp._favit_q8 = ((fmt, dx_lp._version), (q, None, sinv))
        return (dx, dx_lp, None, None) if acc else (dx, dx_lp, dg, db)
    _abi.check(_abi.lib().favit_layernorm_bwd(_p(dy), dt(dy), _p(x), ldx, _p(gamma), _p(mean), _p(rstd), _p(dres),
                                              _p(dx), lddx, _p(dx_lp), dt(dy), _p(part[0]), _p(part[1]), nparts,
                                              _p(dg), _p(db), int(acc), rows, D, float(lp_drop[0]), int(lp_drop[1]) & ((1 << 64) - 1),
                                              _st()), "favit_layernorm_bwd")
    return (dx, dx_lp, None, None) if acc else (dx, dx_lp, dg, db)


def _head_pool_args(who, x, first):
    """(B, L, D, workspace bytes) of a mean-pooled head call on x fp32 [B, L, D]; the library refuses the widths it has
    no kernel for before anything is allocated or launched."""
    require_gpu(x)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{who} expects a contiguous fp32 [B, L, D] tensor")
    B, L, D = x.shape
    if not 0 <= int(first) < L:
        raise ValueError(f"{who}: first = {first} leaves no row of {L} to pool")
    nbytes = _abi.lib().favit_head_pool_workspace(B, L, int(first), D)
    if nbytes < 0:
        _abi.check(int(nbytes), who)
    return B, L, D, nbytes


def _head_pool_row(who, name, t, B, D):
    require_gpu(t)
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, D):
        raise ValueError(f"{who}: {name} is a contiguous fp32 [B, D] = [{B}, {D}] tensor")


def ln_meanpool_fwd(x, gamma, beta, first=1, eps=1e-5):
    """x fp32 [B, L, D] -> (y, s, mean, rstd): y [B, D] = mean over the rows [first, L) of LayerNorm(x) (gamma, beta),
    s [B, D] the mean of the normalised rows before the affine map, mean / rstd [B, L - first] (favit_ln_meanpool_fwd)."""
    B, L, D, nbytes = _head_pool_args("favit_ln_meanpool_fwd", x, first)
    require_gpu(gamma, beta)
    dev, n = x.device, L - int(first)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    y = torch.empty((B, D), dtype=torch.float32, device=dev)
    s = torch.empty((B, D), dtype=torch.float32, device=dev)
    mean = torch.empty((B, n), dtype=torch.float32, device=dev)
    rstd = torch.empty((B, n), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().favit_ln_meanpool_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(s), _p(mean), _p(rstd), _p(ws), B, L,
                                                int(first), D, eps, _st()), "favit_ln_meanpool_fwd")
    return y, s, mean, rstd


def ln_meanpool_bwd(dy, x, gamma, s, mean, rstd, first=1, *, dg_out=None, db_out=None, frozen=False):
    """(dx [B, L, D] with zeros in the rows below first, dgamma, dbeta) of ln_meanpool_fwd.  dg_out / db_out: fp32 [D]
    gradient buffers the affine gradients are ACCUMULATED into (then None is returned in their place); frozen: gamma
    and beta take no gradient."""
    B, L, D, _ = _head_pool_args("favit_ln_meanpool_bwd", x, first)
    _head_pool_row("favit_ln_meanpool_bwd", "dy", dy, B, D)
    _head_pool_row("favit_ln_meanpool_bwd", "s", s, B, D)
    require_gpu(gamma, mean, rstd)
    dx = torch.empty((B, L, D), dtype=torch.float32, device=x.device)
    acc = dg_out is not None and db_out is not None
    if frozen:
        dg = db = None
    elif acc:
        dg, db = dg_out, db_out
    else:
        dgb = torch.empty((2, D), dtype=torch.float32, device=x.device)
        dg, db = dgb[0], dgb[1]
    _abi.check(_abi.lib().favit_ln_meanpool_bwd(_p(dy), _p(x), _p(gamma), _p(s), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db),
                                                int(acc), B, L, int(first), D, _st()), "favit_ln_meanpool_bwd")
    return (dx, None, None) if acc or frozen else (dx, dg, db)


def meanpool_fwd(x, first=1):
    """x fp32 [B, L, D] -> p [B, D], the mean over the rows [first, L) (favit_meanpool_fwd)."""
    B, L, D, nbytes = _head_pool_args("favit_meanpool_fwd", x, first)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    p = torch.empty((B, D), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().favit_meanpool_fwd(_p(x), _p(p), _p(ws), B, L, int(first), D, _st()), "favit_meanpool_fwd")
    return p


def meanpool_bwd(dp, L, first=1):
    """dp fp32 [B, D] -> dx [B, L, D]: dp / (L - first) in the rows [first, L), zeros below (favit_meanpool_bwd)."""
    require_gpu(dp)
    if dp.dim() != 2 or dp.dtype != torch.float32 or not dp.is_contiguous():
        raise ValueError("favit_meanpool_bwd expects a contiguous fp32 [B, D] tensor")
    B, D = dp.shape
    if not 0 <= int(first) < L:
        raise ValueError(f"favit_meanpool_bwd: first = {first} leaves no row of {L} to pool")
    nbytes = _abi.lib().favit_head_pool_workspace(B, L, int(first), D)       # refuses an unsupported D before dx exists
    if nbytes < 0:
        _abi.check(int(nbytes), "favit_meanpool_bwd")
    dx = torch.empty((B, L, D), dtype=torch.float32, device=dp.device)
    _abi.check(_abi.lib().favit_meanpool_bwd(_p(dp), _p(dx), B, L, int(first), D, _st()), "favit_meanpool_bwd")
    return dx


def reduce_rows_multi(entries):
    """entries: [(part [2, rows, cols] fp32 contiguous, out0 [cols], out1 [cols])] -> out0 += colsum(part[0]),
    out1 += colsum(part[1]) for every entry in ONE launch (at most 32 entries per launch).  Entries whose row counts
    differ (one cols) go through reduce_rows_multi_ragged, still one launch."""
    if entries and any(tuple(e[0].shape) != tuple(entries[0][0].shape) for e in entries):
        return reduce_rows_multi_ragged(entries)
    for i in range(0, len(entries), _abi.REDUCE_ROWS_MULTI_MAX):
        chunk = entries[i:i + _abi.REDUCE_ROWS_MULTI_MAX]
        n = len(chunk)
        rows, cols = chunk[0][0].shape[1], chunk[0][0].shape[2]
        arr = C.c_void_p * n
        for part, o0, o1 in chunk:
            require_gpu(part, o0, o1)
            if tuple(part.shape) != (2, rows, cols) or not part.is_contiguous() or part.dtype != torch.float32:
                raise ValueError("reduce_rows_multi: every entry must be a contiguous fp32 [2, rows, cols] stack of one shape")
        _abi.check(_abi.lib().favit_reduce_rows_multi(n, arr(*[e[0].data_ptr() for e in chunk]),
                                                      arr(*[e[1].data_ptr() for e in chunk]),
                                                      arr(*[e[2].data_ptr() for e in chunk]), rows, cols, _st()),
                   "favit_reduce_rows_multi")


def reduce_rows_multi_ragged(entries):
    """reduce_rows_multi for entries [(part [2, rows_e, cols], out0 [cols], out1 [cols])] whose row counts differ: one
    launch per 32 entries; every entry is summed as a reduce_rows_multi launch of its own would sum it."""
    if not entries:
        return
    cols = entries[0][0].shape[-1]
    for part, o0, o1 in entries:                        # validate everything before the first launch
        require_gpu(part, o0, o1)
        if part.dim() != 3 or part.shape[0] != 2 or part.shape[2] != cols or not part.is_contiguous() or part.dtype != torch.float32:
            raise ValueError("reduce_rows_multi: every entry must be a contiguous fp32 [2, rows, cols] stack of one cols")
    for i in range(0, len(entries), _abi.REDUCE_ROWS_MULTI_MAX):
        chunk = entries[i:i + _abi.REDUCE_ROWS_MULTI_MAX]
        n = len(chunk)
        arr = C.c_void_p * n
        rows = (C.c_int64 * n)(*[e[0].shape[1] for e in chunk])
        _abi.check(_abi.lib().favit_reduce_rows_multi_ragged(n, arr(*[e[0].data_ptr() for e in chunk]),
                                                             arr(*[e[1].data_ptr() for e in chunk]),
                                                             arr(*[e[2].data_ptr() for e in chunk]), rows, cols, _st()),
                   "favit_reduce_rows_multi_ragged")


def reduce_rows(t2d: torch.Tensor) -> torch.Tensor:
    require_gpu(t2d)
    rows, cols = t2d.shape
    out = torch.empty(cols, dtype=torch.float32, device=t2d.device)
    _abi.check(_abi.lib().favit_reduce_rows(_p(t2d), t2d.stride(0), _p(out), rows, cols, 0, _st()), "favit_reduce_rows")
    return out


def mhla_fold_fwd(wqkv, bqkv, wl, bl, H, dtype):
    require_gpu(wqkv, bqkv, wl, bl)
    D = wqkv.shape[1]
    weff = torch.empty((3 * D, D), dtype=dtype, device=wqkv.device)
    beff = torch.empty(3 * D, dtype=torch.float32, device=wqkv.device)
    _abi.check(_abi.lib().favit_mhla_fold_fwd(_p(wqkv), _p(bqkv), _p(wl), _p(bl), _p(weff), dt(weff), None, _p(beff),
                                              D, H, _st()), "favit_mhla_fold_fwd")
    return weff, beff


def mhla_fold_fwd_multi(params, H, dtype):
    """params: list of (wqkv, bqkv, wl, bl) per block -> list of (weff, beff); one launch for all blocks."""
    n = len(params)
    D = params[0][0].shape[1]
    dev = params[0][0].device
    for q in params:
        require_gpu(*q)
    weff = torch.empty((n, 3 * D, D), dtype=dtype, device=dev)
    beff = torch.empty((n, 3 * D), dtype=torch.float32, device=dev)
    arr = C.c_void_p * n
    cols = [arr(*[q[j].data_ptr() for q in params]) for j in range(4)]
    wp = arr(*[weff[i].data_ptr() for i in range(n)])
    bp = arr(*[beff[i].data_ptr() for i in range(n)])
    _abi.check(_abi.lib().favit_mhla_fold_fwd_multi(n, cols[0], cols[1], cols[2], cols[3], wp, dt(weff), bp, D, H, _st()),
               "favit_mhla_fold_fwd_multi")
    return [(weff[i], beff[i]) for i in range(n)]


def mhla_fold_bwd(dweff, dbeff, wqkv, bqkv, wl, H, out=None):
    """out = (dwqkv, dbqkv, dwl, dbl) gradient buffers to ACCUMULATE into, or None for fresh tensors."""
    D = wqkv.shape[1]
    hd = D // H
    dev = wqkv.device
    acc = out is not None
    if acc:
        dwqkv, dbqkv, dwl, dbl = out
    else:
        dwqkv = torch.empty((3 * D, D), dtype=torch.float32, device=dev)
        dbqkv = torch.empty(3 * D, dtype=torch.float32, device=dev)
        dwl = torch.empty((hd, hd), dtype=torch.float32, device=dev)
        dbl = torch.empty(hd, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().favit_mhla_fold_bwd(_p(dweff), _p(dbeff), _p(wqkv), _p(bqkv), _p(wl), _p(dwqkv), _p(dbqkv),
                                              _p(dwl), _p(dbl), D, H, int(acc), _st()), "favit_mhla_fold_bwd")
    return dwqkv, dbqkv, dwl, dbl


def mhla_fold_bwd_multi(entries, H):
    """entries: [(dweff, dbeff, wqkv, bqkv, wl, (dwqkv, dbqkv, dwl, dbl))] of equal geometry: every layer's fold
    backward in ONE launch (chunks of 16), ACCUMULATING into the gradient buffers."""
    for i in range(0, len(entries), _abi.FOLD_BWD_MAX):
        chunk = entries[i:i + _abi.FOLD_BWD_MAX]
        n = len(chunk)
        D = chunk[0][2].shape[1]
        arr = C.c_void_p * n
        cols = []
        for j in range(5):
            cols.append(arr(*[e[j].data_ptr() for e in chunk]))
        for j in range(4):     # (dwqkv, dbqkv may be None for every layer: frozen qkv projection, latent_proj gradients only)
            cols.append(arr(*[(e[5][j].data_ptr() if e[5][j] is not None else None) for e in chunk]))
        for e in chunk:
            require_gpu(*e[:5], *e[5])
        _abi.check(_abi.lib().favit_mhla_fold_bwd_multi(n, *cols, D, H, _st()), "favit_mhla_fold_bwd_multi")


def mhla_attn_lse_supported(L, hd, W, dtype) -> bool:
    """Do favit_mhla_attn_fwd_lse / _bwd_lse take this shape (bf16, hd = 64, odd W <= 7 or <= 11 with L > 16)?"""
    code = {torch.float32: _abi.F32, torch.bfloat16: _abi.BF16}.get(dtype)
    return code is not None and bool(_abi.lib().favit_mhla_attn_lse_supported(L, hd, W, code))


def _check_mhla_mask(mask, qkv, B, L):
    """The kernels index mask[(b*L + i)*L + j] as bytes: anything but a contiguous uint8 / bool [B, L, L] on the inputs'
    device would be read out of bounds, or as the bytes of another type."""
    if mask is None:
        return
    ok = (torch.is_tensor(mask) and mask.dtype in (torch.uint8, torch.bool) and tuple(mask.shape) == (B, L, L)
          and mask.is_contiguous() and mask.device == qkv.device)
    if not ok:
        got = (f"{mask.dtype} {tuple(mask.shape)} on {mask.device}, {'' if mask.is_contiguous() else 'not '}contiguous"
               if torch.is_tensor(mask) else type(mask).__name__)
        raise ValueError(f"MHLA attention mask: expected a contiguous uint8 or bool tensor of shape ({B}, {L}, {L}) on "
                         f"{qkv.device}, got {got}")


def _check_dense_mask(what, mask, m_sb, m_sq, B, Lq, Lk):
    """The dense kernels read mask[b*m_sb + q*m_sq + k] as bytes, for b < B, q < Lq, k < Lk."""
    if mask is None:
        return
    need = (B - 1) * m_sb + (Lq - 1) * m_sq + Lk
    ok = (torch.is_tensor(mask) and mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous() and m_sb >= 0
          and m_sq >= 0 and mask.numel() >= need)
    if not ok:
        got = (f"{mask.dtype} {tuple(mask.shape)} ({mask.numel()} elements), {'' if mask.is_contiguous() else 'not '}"
               f"contiguous" if torch.is_tensor(mask) else type(mask).__name__)
        raise ValueError(f"{what} mask: expected a contiguous uint8 or bool tensor of at least {need} elements "
                         f"(B = {B}, Lq = {Lq}, Lk = {Lk}, batch stride {m_sb}, query stride {m_sq}), got {got}")


def mhla_attn_fwd(qkv, B, L, H, hd, W, mask=None, p=0.0, seed=0, want_lse=False):
    """Attention core; with want_lse returns (out, lse fp32 [B, H, L]) -- lse is None where the saved-statistics
    backward does not apply (the caller then uses mhla_attn_bwd without it).  mask: contiguous uint8 / bool [B, L, L]
    (non-zero = keep) or None; a row with every window key masked gives out = 0 and lse = -inf (include/favit.h)."""
    _check_mhla_mask(mask, qkv, B, L)
    require_gpu(qkv, mask)
    out = torch.empty((B * L, H * hd), dtype=qkv.dtype, device=qkv.device)
    if want_lse and mhla_attn_lse_supported(L, hd, W, qkv.dtype):
        lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
        _abi.check(_abi.lib().favit_mhla_attn_fwd_lse(_p(qkv), _p(out), _p(lse), _p(mask), B, L, H, hd, W, dt(qkv), p,
                                                      seed, _st()), "favit_mhla_attn_fwd_lse")
        return out, lse
    _abi.check(_abi.lib().favit_mhla_attn_fwd(_p(qkv), _p(out), _p(mask), B, L, H, hd, W, dt(qkv), p, seed, _st()),
               "favit_mhla_attn_fwd")
    return (out, None) if want_lse else out


def mhla_attn_bwd(qkv, dout, B, L, H, hd, W, mask=None, p=0.0, seed=0, o=None, lse=None):
    """dqkv of the attention core; with the forward's output and lse the saved-statistics kernel runs."""
    _check_mhla_mask(mask, qkv, B, L)
    require_gpu(qkv, dout, mask, o, lse)
    dqkv = torch.empty_like(qkv)
    if o is not None and lse is not None:
        _abi.check(_abi.lib().favit_mhla_attn_bwd_lse(_p(qkv), _p(dout), _p(o), _p(lse), _p(dqkv), _p(mask), B, L, H, hd,
                                                      W, dt(qkv), p, seed, _st()), "favit_mhla_attn_bwd_lse")
        return dqkv
    _abi.check(_abi.lib().favit_mhla_attn_bwd(_p(qkv), _p(dout), _p(dqkv), _p(mask), B, L, H, hd, W, dt(qkv), p, seed,
                                              _st()), "favit_mhla_attn_bwd")
    return dqkv


class BlockPlan:
    """What favit_mhla_block_fwd / _bwd need for one block at one shape, kept from step to step: the descriptor with
    its geometry filled in and the two layouts (include/favit.h).  off / boff map slot names to (byte offset, bytes);
    boff and bwd_bytes are indexed by want_lp_out (0: a row cut follows the block's backward).
    Narrowed plans (n_mlp < n: the MLP half runs on fewer rows) also carry the companion struct
    (rows / rref); Mm = B * n_mlp and nparts2 belong to the MLP half's slots (equal to M and nparts otherwise); st is
    the stream of the first call of a pair of halves, which the second one reuses."""
    __slots__ = ("desc", "ref", "M", "D", "hidden", "B", "n", "H", "nparts", "tape_bytes", "off", "bwd_bytes", "boff",
                 "n_mlp", "Mm", "nparts2", "rows", "rref", "st")


def mhla_block_plan(B, n, D, H, W, hidden, training, eps=1e-5, n_mlp=None) -> Optional[BlockPlan]:
    """The layout queries for one block geometry (host arithmetic, once per shape), or None where the native chain
    does not take it (D / H != 64, hidden not a multiple of 8, a row count the lse attention kernels decline).
    n_mlp: rows per image of the MLP half where that is narrower than n (the two-row-count layouts)."""
    d = _abi.BlockDesc()
    d.B, d.n, d.D, d.H, d.W, d.hidden, d.training, d.eps = B, n, D, H, W, hidden, int(bool(training)), eps
    lib = _abi.lib()
    narrow = n_mlp is not None and n_mlp != n
    p = BlockPlan()
    p.rows = p.rref = p.st = None
    if narrow:
        p.rows = _abi.BlockMlp()
        p.rows.n_mlp = n_mlp
        p.rref = C.byref(p.rows)
    to = (C.c_int64 * len(_abi.BLOCK_TAPE_SLOTS))()
    tape_bytes = (lib.favit_mhla_block_tape_layout2(C.byref(d), p.rref, to) if narrow
                  else lib.favit_mhla_block_tape_layout(C.byref(d), to))
    if tape_bytes < 0:
        return None
    p.desc, p.ref, p.M, p.D, p.hidden, p.B, p.n, p.H = d, C.byref(d), B * n, D, hidden, B, n, H
    p.n_mlp = n_mlp if narrow else n
    p.Mm = B * p.n_mlp
    p.nparts = int(min(2048, (B * n + 3) // 4))
    p.nparts2 = int(min(2048, (p.Mm + 3) // 4))
    p.tape_bytes = d.tape_bytes = tape_bytes
    ends = list(to[1:]) + [tape_bytes]
    p.off = {k: (to[i], ends[i] - to[i]) for i, k in enumerate(_abi.BLOCK_TAPE_SLOTS)}
    p.bwd_bytes, p.boff = [], []
    for want_lp in (0, 1):
        bo = (C.c_int64 * len(_abi.BLOCK_BWD_SLOTS))()
        nb = (lib.favit_mhla_block_bwd_layout2(C.byref(d), p.rref, want_lp, bo) if narrow
              else lib.favit_mhla_block_bwd_layout(C.byref(d), want_lp, bo))
        ends = list(bo[1:]) + [nb]
        p.bwd_bytes.append(nb)
        p.boff.append({k: (bo[i], ends[i] - bo[i]) for i, k in enumerate(_abi.BLOCK_BWD_SLOTS)})
    return p


def _block_code(code: int, what: str) -> int:
    """0, or the negative code of a DECLINED call (nothing was launched: the caller issues the launches itself); a
    failed launch raises."""
    if code == _abi.ERR_LAUNCH:
        _abi.check(code, what)
    return code


def mhla_block_fwd(plan: BlockPlan, x, tape, g1, b1, g2, b2, weff, beff, wproj, bproj, wfc1, bfc1, wfc2, bfc2) -> int:
    """The forward chain of one block (favit_mhla_block_fwd) on the current stream -- of a narrowed plan its attention
    half (favit_mhla_block_attn_fwd: x1 is in the tape afterwards; mhla_block_mlp_fwd follows the row cut).  tape:
    uint8 device tensor of plan.tape_bytes.  All pointers of the descriptor are rewritten (they may change from step
    to step); the geometry and the layout stay.  Returns 0 or the code of a declined call."""
    d = plan.desc
    d.x, d.tape, d.tape_bytes = x.data_ptr(), tape.data_ptr(), tape.numel()
    d.g1, d.b1, d.g2, d.b2 = g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), b2.data_ptr()
    d.weff, d.beff, d.wproj, d.bproj = weff.data_ptr(), beff.data_ptr(), wproj.data_ptr(), bproj.data_ptr()
    d.wfc1, d.bfc1, d.wfc2, d.bfc2 = wfc1.data_ptr(), bfc1.data_ptr(), wfc2.data_ptr(), bfc2.data_ptr()
    if plan.rows is not None:
        plan.st = _st()
        return _block_code(_abi.lib().favit_mhla_block_attn_fwd(plan.ref, plan.rref, plan.st), "favit_mhla_block_attn_fwd")
    return _block_code(_abi.lib().favit_mhla_block_fwd(plan.ref, _st()), "favit_mhla_block_fwd")


def mhla_block_mlp_fwd(plan: BlockPlan, x1c) -> int:
    """The MLP half of a narrowed plan's forward (favit_mhla_block_mlp_fwd) on x1c fp32 [B * n_mlp, D], the cut copy of
    the x1 that mhla_block_fwd left in the tape.  The descriptor is the one that call filled: nothing is looked up or
    allocated here, and the stream is the one of that call (the two run in one frame of EncoderOp.fwd).  Returns 0 or
    the code of a declined call."""
    plan.rows.x1c = x1c.data_ptr()
    return _block_code(_abi.lib().favit_mhla_block_mlp_fwd(plan.ref, plan.rref, plan.st), "favit_mhla_block_mlp_fwd")


def _block_bwd_ptrs(plan, x, tape, g1, g2, weff, wproj, wfc1, wfc2):
    d = plan.desc
    d.x, d.tape, d.tape_bytes = x.data_ptr(), tape.data_ptr(), tape.numel()
    d.g1, d.g2 = g1.data_ptr(), g2.data_ptr()
    d.weff, d.wproj, d.wfc1, d.wfc2 = weff.data_ptr(), wproj.data_ptr(), wfc1.data_ptr(), wfc2.data_ptr()


def mhla_block_mlp_bwd(plan: BlockPlan, x, tape, g1, g2, weff, wproj, wfc1, wfc2, x1c, g, g_lp, arena,
                       want_lp_out: bool) -> int:
    """The MLP half of a narrowed plan's input-gradient chain (favit_mhla_block_mlp_bwd).  g / g_lp: gradient of the
    block's output, fp32 and bf16 [B * n_mlp, D].  Leaves g1_f32 [B * n_mlp, D] in the arena (plan.boff); the caller
    expands it (rows_cut_bwd) and hands the pair to mhla_block_bwd with the same arena and want_lp_out."""
    _block_bwd_ptrs(plan, x, tape, g1, g2, weff, wproj, wfc1, wfc2)
    plan.rows.x1c = x1c.data_ptr()
    plan.st = _st()
    return _block_code(_abi.lib().favit_mhla_block_mlp_bwd(plan.ref, plan.rref, g.data_ptr(), g_lp.data_ptr(),
                                                           arena.data_ptr(), arena.numel(), int(bool(want_lp_out)), plan.st),
                       "favit_mhla_block_mlp_bwd")


def mhla_block_bwd(plan: BlockPlan, x, tape, g1, g2, weff, wproj, wfc1, wfc2, g, g_lp, arena, want_lp_out: bool,
                   ptrs_set: bool = False) -> int:
    """The input-gradient chain of one block (favit_mhla_block_bwd).  g / g_lp: gradient of the block's output, fp32 and
    bf16 [M, D]; arena: uint8 device tensor of plan.bwd_bytes[want_lp_out].  Only the pointers the chain reads are
    rewritten (the biases are not read).  Returns 0 or the code of a declined call.
    A narrowed plan: the attention half (favit_mhla_block_attn_bwd); g / g_lp are then the gradient of x1, expanded to
    [M, D] by the row cut that follows mhla_block_mlp_bwd (ptrs_set: that call has just written the same pointers
    into the descriptor and taken the stream, and nothing has used the plan since)."""
    if not ptrs_set:
        _block_bwd_ptrs(plan, x, tape, g1, g2, weff, wproj, wfc1, wfc2)
    if plan.rows is not None:
        return _block_code(_abi.lib().favit_mhla_block_attn_bwd(plan.ref, plan.rref, g.data_ptr(), g_lp.data_ptr(),
                                                                arena.data_ptr(), arena.numel(), int(bool(want_lp_out)),
                                                                plan.st if ptrs_set else _st()), "favit_mhla_block_attn_bwd")
    return _block_code(_abi.lib().favit_mhla_block_bwd(plan.ref, g.data_ptr(), g_lp.data_ptr(), arena.data_ptr(),
                                                       arena.numel(), int(bool(want_lp_out)), _st()),
                       "favit_mhla_block_bwd")


def _sdpa_desc(q, k, v, o, lse, B, H, Lq, Lk, hd, scale, mask, m_sb, m_sq, p, seed):
    """q, k, v, o: (tensor, element offset, row stride, batch stride, head stride) views (functional._View)."""
    d = SdpaDesc()
    es = q.t.element_size()
    for name, vw in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(d, name, vw.t.data_ptr() + vw.off * es)
        getattr(d, name + "_str")[:] = [vw.ld, vw.sb, vw.sh]
    d.lse = lse.data_ptr()
    d.mask = mask.data_ptr() if mask is not None else None
    d.m_sb, d.m_sq = m_sb, m_sq
    d.B, d.H, d.Lq, d.Lk, d.hd, d.dtype = B, H, Lq, Lk, hd, dt(q.t)
    d.scale, d.dropout_p, d.seed = scale, p, seed
    return d


def sdpa_fwd(q, k, v, o, B, H, Lq, Lk, hd, scale, mask=None, m_sb=0, m_sq=0, p=0.0, seed=0):
    """Fused attention forward: writes o (view) and returns lse [B*H, Lq] fp32 (saved for backward)."""
    _check_dense_mask("favit_sdpa_fwd", mask, m_sb, m_sq, B, Lq, Lk)
    require_gpu(q.t, k.t, v.t, o.t, mask)
    lse = torch.empty((B * H, Lq), dtype=torch.float32, device=q.t.device)
    d = _sdpa_desc(q, k, v, o, lse, B, H, Lq, Lk, hd, scale, mask, m_sb, m_sq, p, seed)
    _abi.check(_abi.lib().favit_sdpa_fwd(C.byref(d), _st()), "favit_sdpa_fwd")
    return lse


def sdpa_bwd(q, k, v, o, do, dq, dk, dv, lse, B, H, Lq, Lk, hd, scale, mask=None, m_sb=0, m_sq=0, p=0.0, seed=0):
    """Fused attention backward: writes dq, dk, dv (views); probabilities are recomputed from lse."""
    _check_dense_mask("favit_sdpa_bwd", mask, m_sb, m_sq, B, Lq, Lk)
    require_gpu(q.t, k.t, v.t, o.t, do.t, dq.t, dk.t, dv.t, lse, mask)
    delta = torch.empty((B * H, Lq), dtype=torch.float32, device=q.t.device)
    d = _sdpa_desc(q, k, v, o, lse, B, H, Lq, Lk, hd, scale, mask, m_sb, m_sq, p, seed)
    es = q.t.element_size()
    for name, vw in (("dout", do), ("dq", dq), ("dk", dk), ("dv", dv)):
        setattr(d, name, vw.t.data_ptr() + vw.off * es)
        getattr(d, ("do" if name == "dout" else name) + "_str")[:] = [vw.ld, vw.sb, vw.sh]
    d.delta = delta.data_ptr()
    _abi.check(_abi.lib().favit_sdpa_bwd(C.byref(d), _st()), "favit_sdpa_bwd")


def softmax_fwd(S, p_dtype, H, Z, Lq, Lk, mask=None, m_sb=0, m_sq=0, p=0.0, seed=0):
    _check_dense_mask("favit_softmax_fwd", mask, m_sb, m_sq, (Z - 1) // H + 1, Lq, Lk)     # mask batch of row z: z / H
    require_gpu(S, mask)
    P = torch.empty((Z, Lq, Lk), dtype=p_dtype, device=S.device)
    Pd = torch.empty_like(P) if p > 0 else None
    _abi.check(_abi.lib().favit_softmax_fwd(_p(S), _p(P), _p(Pd), dt(P), _p(mask), m_sb, m_sq, H, Z, Lq, Lk, p, seed,
                                            _st()), "favit_softmax_fwd")
    return P, (Pd if Pd is not None else P)


def softmax_bwd(P, dPd, Z, Lq, Lk, p=0.0, seed=0):
    dS = torch.empty_like(P)
    _abi.check(_abi.lib().favit_softmax_bwd(_p(P), dt(P), _p(dPd), _p(dS), dt(dS), Z, Lq, Lk, p, seed, _st()),
               "favit_softmax_bwd")
    return dS


def patchify_fwd(img, P, dtype):
    require_gpu(img)
    B, Cc, HW, HW2 = img.shape
    if HW != HW2 or HW % P:
        raise ValueError("patchify needs square images with size divisible by patch_size")
    img = img.contiguous()
    g = HW // P
    out = torch.empty((B * g * g, P * P * Cc), dtype=dtype, device=img.device)
    _abi.check(_abi.lib().favit_patchify_fwd(_p(img), _p(out), dt(out), B, Cc, HW, P, _st()), "favit_patchify_fwd")
    return out


def patchify_bwd(dpatch, B, Cc, HW, P):
    dimg = torch.empty((B, Cc, HW, HW), dtype=torch.float32, device=dpatch.device)
    _abi.check(_abi.lib().favit_patchify_bwd(_p(dpatch), _p(dimg), B, Cc, HW, P, _st()), "favit_patchify_bwd")
    return dimg


def embed_prologue_fwd(tok, cls, pos, B, N, D):
    x = torch.empty((B, N + 1, D), dtype=torch.float32, device=tok.device)
    _abi.check(_abi.lib().favit_embed_prologue_fwd(_p(tok), _p(cls), _p(pos), _p(x), B, N, D, _st()),
               "favit_embed_prologue_fwd")
    return x


def embed_prologue_bwd(dx, B, N, D, tok_dtype, want_pos=True):
    dev = dx.device
    dtok = torch.empty((B * N, D), dtype=tok_dtype, device=dev)
    dcls = torch.empty(D, dtype=torch.float32, device=dev)
    dpos = torch.empty((N + 1, D), dtype=torch.float32, device=dev) if want_pos else None
    _abi.check(_abi.lib().favit_embed_prologue_bwd(_p(dx), _p(dtok), dt(dtok), _p(dcls), _p(dpos), B, N, D, _st()),
               "favit_embed_prologue_bwd")
    return dtok, dcls, dpos


def rows_cut_fwd(x, B, n_in, a, b, D):
    """x fp32 [B, n_in, D] (contiguous) -> [B, a + b, D]: the first a and the last b rows of every image."""
    require_gpu(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != B * n_in * D:
        raise ValueError("rows_cut_fwd expects a contiguous fp32 [B, n_in, D] tensor")
    y = torch.empty((B, a + b, D), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().favit_rows_cut_fwd(_p(x), _p(y), B, n_in, a, b, D, _st()), "favit_rows_cut_fwd")
    return y


def rows_cut_bwd(dy, B, n_in, a, b, D, lp_dtype=None):
    """dy fp32 [B, a + b, D] -> (dx fp32 [B, n_in, D] with zeros in the cut rows, its lp_dtype copy or None)."""
    require_gpu(dy)
    if dy.dtype != torch.float32 or not dy.is_contiguous() or dy.numel() != B * (a + b) * D:
        raise ValueError("rows_cut_bwd expects a contiguous fp32 [B, a + b, D] tensor")
    dx = torch.empty((B, n_in, D), dtype=torch.float32, device=dy.device)
    lp = torch.empty((B, n_in, D), dtype=lp_dtype, device=dy.device) if lp_dtype is not None else None
    _abi.check(_abi.lib().favit_rows_cut_bwd(_p(dy), _p(dx), _p(lp), dt(lp) if lp is not None else F32, B, n_in, a, b, D,
                                             _st()), "favit_rows_cut_bwd")
    return dx, lp


def dropout(x, p, seed):
    y = torch.empty_like(x)
    _abi.check(_abi.lib().favit_dropout(_p(x), _p(y), dt(x), x.numel(), p, seed, _st()), "favit_dropout")
    return y


_U64 = (1 << 64) - 1


def drop_path_add(x, y, B, n, D, p, seed, out=None):
    """x + (keep(b) ? y / (1 - p) : 0) per sample b (favit_drop_path_add): x fp32 [B*n, D], y [B*n, D] fp32 or bf16,
    both contiguous.  out: None (a new tensor), x or y (in place; y only in fp32)."""
    require_gpu(x, y, out)
    if x.dtype != torch.float32 or not x.is_contiguous() or not y.is_contiguous() or x.numel() != B * n * D \
            or y.numel() != x.numel():
        raise ValueError("drop_path_add expects contiguous [B*n, D] tensors, x in fp32")
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != x.numel():
        raise ValueError("drop_path_add: out is a contiguous fp32 [B*n, D] tensor")
    _abi.check(_abi.lib().favit_drop_path_add(_p(x), _p(y), dt(y), _p(out), B, n, D, float(p), int(seed) & _U64, _st()),
               "favit_drop_path_add")
    return out


def drop_path_bwd(g, lp_dtype, B, n, D, p, seed, lp_drop=(0.0, 0)):
    """The branch gradient of a drop-path residual add in the compute dtype lp_dtype (favit_drop_path_bwd):
    keep(b) ? g / (1 - p) : 0 per sample b, times the element mask lp_drop = (p, seed) of the branch's output dropout
    (as layernorm_bwd's lp copy carries it).  g fp32 [B*n, D] contiguous."""
    require_gpu(g)
    if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != B * n * D:
        raise ValueError("drop_path_bwd expects a contiguous fp32 [B*n, D] tensor")
    g_lp = torch.empty((B * n, D), dtype=lp_dtype, device=g.device)
    _abi.check(_abi.lib().favit_drop_path_bwd(_p(g), _p(g_lp), dt(lp_dtype), B, n, D, float(p), int(seed) & _U64,
                                              float(lp_drop[0]), int(lp_drop[1]) & _U64, _st()), "favit_drop_path_bwd")
    return g_lp


def sppp_map_patches(seg, P):
    require_gpu(seg)
    if seg.dtype != torch.int64:
        seg = seg.to(torch.int64)
    seg = seg.contiguous()
    B, HW, _ = seg.shape
    N = (HW // P) ** 2
    dev = seg.device
    rank = torch.empty((B, N), dtype=torch.int32, device=dev)
    ntok = torch.empty(B, dtype=torch.int32, device=dev)
    perm = torch.empty((B, N), dtype=torch.int32, device=dev)
    offs = torch.empty((B, N + 1), dtype=torch.int32, device=dev)
    dom = torch.empty((B, N), dtype=torch.int64, device=dev)
    _abi.check(_abi.lib().favit_sppp_map_patches(_p(seg), _p(rank), _p(ntok), _p(perm), _p(offs), _p(dom), B, HW, P,
                                                 _st()), "favit_sppp_map_patches")
    return rank, ntok, perm, offs, dom


def sppp_pool_fwd(emb, perm, offs, kind, R):
    B, N, D = emb.shape
    out = torch.empty((B, R, D), dtype=torch.float32, device=emb.device)
    argmax = torch.empty((B, R, D), dtype=torch.int32, device=emb.device) if kind == 1 else None
    _abi.check(_abi.lib().favit_sppp_pool_fwd(_p(emb), _p(perm), _p(offs), _p(out), _p(argmax), kind, B, N, R, D,
                                              _st()), "favit_sppp_pool_fwd")
    return out, argmax


def sppp_pool_bwd(dout, emb, perm, offs, argmax, kind, R):
    B, N, D = emb.shape
    demb = torch.zeros_like(emb)
    _abi.check(_abi.lib().favit_sppp_pool_bwd(_p(dout), _p(emb), None, _p(perm), _p(offs), _p(argmax), _p(demb), kind,
                                              B, N, R, D, _st()), "favit_sppp_pool_bwd")
    return demb


def sppp_centroids(seg, S):
    require_gpu(seg)
    seg = seg.to(torch.int64).contiguous()
    B, HW, _ = seg.shape
    cent = torch.empty((B, S, 2), dtype=torch.float32, device=seg.device)
    _abi.check(_abi.lib().favit_sppp_centroids(_p(seg), _p(cent), B, HW, S, _st()), "favit_sppp_centroids")
    return cent


def sppp_posenc_fwd(x, cent):
    B, L, D = x.shape
    y = torch.empty_like(x)
    _abi.check(_abi.lib().favit_sppp_posenc_fwd(_p(x), _p(cent), _p(y), B, L, D, 0 if cent is None else cent.shape[1], _st()),
               "favit_sppp_posenc_fwd")
    return y


def slic_grid(H, W, n_segments):
    """Seed grid of skimage.segmentation.slic for a 2-D image (skimage.util.regular_grid on (1, H, W)): returns
    (ys, xs, step) -- seeds at start + i*stride per axis, start = floor(s/2), stride = round(s), s = sqrt(H*W/n)."""
    import math
    if H * W <= n_segments:
        return list(range(H)), list(range(W)), 1
    s = math.sqrt(H * W / float(n_segments))
    sy = sx = s
    if min(H, W) < s:                      # regular_grid: a dimension shorter than the step gets step = its length
        if H <= W:
            sy, sx = float(H), (W / float(n_segments))
        else:
            sx, sy = float(W), (H / float(n_segments))
    ys = list(range(int(sy // 2), H, max(1, int(round(sy)))))
    xs = list(range(int(sx // 2), W, max(1, int(round(sx)))))
    return ys, xs, max(max(1, int(round(sy))), max(1, int(round(sx))))


def slic(images, n_segments=16, compactness=0.1, sigma=1.0, max_num_iter=10, min_size_factor=0.5, stages=False,
         rescale=True):
    """SLIC label maps [B,H,W] int64 of fp32 images [B,3,H,W] on the device (csrc/slic.hip; parity with
    scikit-image unpinned, see include/favit.h).  stages=True also returns (feat, cluster_labels, n_regions).
    rescale (default, scikit-image >= 0.19): every image is first rescaled to [0, 1] by its own min / max over all
    channels, so mean/std-normalised inputs (what the reference's models pass) segment like their [0, 1] originals;
    rescale=False restates scikit-image < 0.19, which takes the values as sRGB in [0, 1] as they are."""
    require_gpu(images)
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise TypeError("slic expects fp32 images [B, 3, H, W]")
    images = images.contiguous()
    B, _, H, W = images.shape
    ys, xs, step = slic_grid(H, W, n_segments)
    if len(ys) * len(xs) > 64:
        raise ValueError("slic: at most 64 seed centres are supported")
    dev = images.device
    init = torch.tensor([[y, x] for y in ys for x in xs], dtype=torch.int32, device=dev)
    Kc = init.shape[0]
    coef = int(round((step / float(compactness)) ** 2))
    min_size = int(min_size_factor * (H * W / float(Kc)))
    feat = torch.empty((B, H * W, 4), dtype=torch.int16, device=dev)
    lab = torch.empty((B, H * W), dtype=torch.uint8, device=dev)
    ws = torch.empty((2, B, H * W), dtype=torch.int32, device=dev)
    out = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    nreg = torch.empty(B, dtype=torch.int32, device=dev)
    L = _abi.lib()
    fws = torch.empty(int(L.favit_slic_features_workspace(B, H, W)) // 4, dtype=torch.float32, device=dev)
    _abi.check(L.favit_slic_features(_p(images), _p(feat), B, H, W, float(sigma), int(bool(rescale)), _p(fws), _st()),
               "favit_slic_features")
    cws = torch.empty(int(L.favit_slic_cluster_workspace(Kc, B)) // 8 + 1, dtype=torch.int64, device=dev)
    _abi.check(L.favit_slic_cluster(_p(feat), _p(lab), _p(init), Kc, B, H, W, step, coef, max_num_iter, _p(cws), _st()),
               "favit_slic_cluster")
    _abi.check(L.favit_slic_connect(_p(lab), _p(ws[0]), _p(ws[1]), _p(out), _p(nreg), B, H, W, min_size, _st()),
               "favit_slic_connect")
    return (out, feat, lab.view(B, H, W), nreg) if stages else out


def slic_stage_times(images, n_segments=16, compactness=0.1, sigma=1.0, max_num_iter=10, min_size_factor=0.5, reps=5):
    """[(stage, ms)] of the three SLIC launches (tools/slic_bench.py)."""
    out = []
    import functools
    B, _, H, W = images.shape
    ys, xs, step = slic_grid(H, W, n_segments)
    dev = images.device
    init = torch.tensor([[y, x] for y in ys for x in xs], dtype=torch.int32, device=dev)
    Kc = init.shape[0]
    coef = int(round((step / float(compactness)) ** 2))
    min_size = int(min_size_factor * (H * W / float(Kc)))
    feat = torch.empty((B, H * W, 4), dtype=torch.int16, device=dev)
    lab = torch.empty((B, H * W), dtype=torch.uint8, device=dev)
    ws = torch.empty((2, B, H * W), dtype=torch.int32, device=dev)
    o = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    nreg = torch.empty(B, dtype=torch.int32, device=dev)
    L = _abi.lib()
    cws = torch.empty(int(L.favit_slic_cluster_workspace(Kc, B)) // 8 + 1, dtype=torch.int64, device=dev)
    fws = torch.empty(int(L.favit_slic_features_workspace(B, H, W)) // 4, dtype=torch.float32, device=dev)
    stages = [
        ("features", lambda: L.favit_slic_features(_p(images), _p(feat), B, H, W, float(sigma), 1, _p(fws), _st())),
        ("cluster", lambda: L.favit_slic_cluster(_p(feat), _p(lab), _p(init), Kc, B, H, W, step, coef, max_num_iter, _p(cws), _st())),
        ("connect", lambda: L.favit_slic_connect(_p(lab), _p(ws[0]), _p(ws[1]), _p(o), _p(nreg), B, H, W, min_size, _st())),
    ]
    for name, fn in stages:
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append((name, e0.elapsed_time(e1) / reps))
    return out


def batch_mix(x, lam, box):
    """Mixup / CutMix of an fp32 [B, C, H, W] batch with its flip, in place (favit_batch_mix): row b is paired with
    row B-1-b; box[b] = (y0, y1, x0, x1) non-empty pastes the partner's pixels into the box, an empty box blends
    lam[b] * x[b] + (1 - lam[b]) * x[B-1-b], and lam[b] == 1 with an empty box leaves the row's bits alone.
    lam: fp32 [B], box: int32 [B, 4], both on the device (data.BatchMix draws them).  Returns x."""
    require_gpu(x, lam, box)
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("batch_mix: x must be a contiguous fp32 [B, C, H, W] tensor")
    B, Cn, H, W = x.shape
    if lam.dtype != torch.float32 or tuple(lam.shape) != (B,) or not lam.is_contiguous():
        raise TypeError("batch_mix: lam must be a contiguous fp32 [B] tensor")
    if box.dtype != torch.int32 or tuple(box.shape) != (B, 4) or not box.is_contiguous():
        raise TypeError("batch_mix: box must be a contiguous int32 [B, 4] tensor of (y0, y1, x0, x1)")
    _abi.check(_abi.lib().favit_batch_mix(_p(x), _p(lam), _p(box), B, Cn, H, W, _st()), "favit_batch_mix")
    return x


def _erase_fill(value, channels):
    """(host float array, normal flag) of an erase fill: a number, a per-channel sequence or "normal"."""
    n = max(int(channels), 3)
    if isinstance(value, str):
        if value != "normal":
            raise ValueError(f"erase value {value!r}: a number, a per-channel sequence or 'normal'")
        return (C.c_float * n)(), 1
    v = [float(value)] * n if np.ndim(value) == 0 else [float(t) for t in value]
    if len(v) < channels or not all(math.isfinite(t) for t in v):
        raise ValueError(f"erase value {value!r}: one finite number, or one per channel ({channels})")
    v = (v + [v[-1]] * n)[:n]
    return (C.c_float * n)(*v), 0


def randaugment(src_u8, ops, mean, std, erase_box=None, erase_value=0.0, erase_seed=0, want_bytes=False):
    """favit_randaugment: src_u8 uint8 [B,S,S,3] (the resized bytes of the image transform) through the op rows
    ops (int32 [B, n_ops, 8] on the device, include/favit.h; data.RandAugment builds them) in one launch -> fp32
    [B,3,S,S] normalized with mean / std (ctypes float[3]), the erase boxes (int32 [B,4] on the device, or None)
    filled with erase_value (a number, a per-channel sequence or "normal" under erase_seed) in the same write.
    Returns out, or (out, augmented bytes [B,S,S,3]) with want_bytes."""
    require_gpu(src_u8, ops)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[1] != src_u8.shape[2] or not src_u8.is_contiguous():
        raise TypeError("randaugment: src_u8 must be a contiguous uint8 [B, S, S, C] tensor")
    B, S, _, Cn = src_u8.shape
    if ops.dtype != torch.int32 or ops.dim() != 3 or ops.shape[0] != B or ops.shape[2] != 8 or not ops.is_contiguous():
        raise TypeError(f"randaugment: ops must be a contiguous int32 [{B}, n_ops, 8] tensor")
    fill, normal = (None, 0)
    if erase_box is not None:
        require_gpu(erase_box)
        if erase_box.dtype != torch.int32 or tuple(erase_box.shape) != (B, 4) or not erase_box.is_contiguous():
            raise TypeError(f"randaugment: erase_box must be a contiguous int32 [{B}, 4] tensor of (y0, y1, x0, x1)")
        fill, normal = _erase_fill(erase_value, Cn)
    dev = src_u8.device
    scratch = torch.empty((2, B, S, S, Cn), dtype=torch.uint8, device=dev)
    out = torch.empty((B, Cn, S, S), dtype=torch.float32, device=dev)
    u8 = torch.empty((B, S, S, Cn), dtype=torch.uint8, device=dev) if want_bytes else None
    _abi.check(_abi.lib().favit_randaugment(_p(src_u8), _p(scratch), _p(out), _p(u8), _p(ops), int(ops.shape[1]),
                                            _p(erase_box), fill, normal, int(erase_seed) & 0xFFFFFFFFFFFFFFFF, B, S, Cn,
                                            mean, std, _st()), "favit_randaugment")
    return (out, u8) if want_bytes else out


def random_erase(x, box, value=0.0, seed=0):
    """favit_random_erase, in place on x fp32 [B,C,H,W]: the box (y0, y1, x0, x1) of every row (int32 [B,4] on the
    device; empty = leave the row alone) is filled with `value` (a number, a per-channel sequence, or "normal": one
    standard-normal value per element under `seed`).  Only the 16-byte groups a box meets are touched.  Returns x."""
    require_gpu(x, box)
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("random_erase: x must be a contiguous fp32 [B, C, H, W] tensor")
    B, Cn, H, W = x.shape
    if box.dtype != torch.int32 or tuple(box.shape) != (B, 4) or not box.is_contiguous():
        raise TypeError(f"random_erase: box must be a contiguous int32 [{B}, 4] tensor of (y0, y1, x0, x1)")
    fill, normal = _erase_fill(value, Cn)
    _abi.check(_abi.lib().favit_random_erase(_p(x), _p(box), fill, normal, int(seed) & 0xFFFFFFFFFFFFFFFF, B, Cn, H, W,
                                             _st()), "favit_random_erase")
    return x


def _check_distill(logits, teacher, alpha, tau, hard):
    """Argument checks of the distilled loss, before the library is touched."""
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"cross_entropy: distill_alpha must be in [0, 1], got {alpha}")
    if not hard and not (math.isfinite(tau) and tau > 0.0):
        raise ValueError(f"cross_entropy: distill_tau must be a finite number > 0, got {tau}")
    if not isinstance(teacher, torch.Tensor):
        raise TypeError("cross_entropy: teacher must be a tensor of teacher logits")
    if teacher.dtype != torch.float32 or tuple(teacher.shape) != tuple(logits.shape) or not teacher.is_contiguous():
        raise TypeError(f"cross_entropy: teacher must be a contiguous fp32 tensor of the logits' shape "
                        f"{tuple(logits.shape)}, got {teacher.dtype} {tuple(teacher.shape)}")
    if teacher.device != logits.device:
        raise ValueError(f"cross_entropy: teacher is on {teacher.device}, the logits on {logits.device}")


def cross_entropy_distill(logits, teacher, labels, grad_scale=None, label_smoothing=0.0, mix_lam=None, alpha=0.5,
                          tau=1.0, hard=False):
    """favit_cross_entropy_distill: returns (loss_rows[B], dlogits or None, kd_rows[B]) with
    loss_rows = (1 - alpha) * base + alpha * kd, base the row kernels.cross_entropy gives for the same labels,
    label_smoothing and mix_lam, and kd the distance to the teacher's logits (fp32 [B, C], no gradient):
    soft, tau^2 * KL(softmax(teacher / tau) || softmax(logits / tau)); hard, the cross-entropy against the teacher's
    argmax (lowest index on ties; tau unused).  dlogits is the gradient of the weighted sum with respect to the
    logits alone.  alpha = 0 is the loss without a teacher, bit for bit; kd_rows is then zero."""
    alpha, tau, hard = float(alpha), float(tau), bool(hard)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"cross_entropy: label_smoothing must be in [0, 1), got {label_smoothing}")
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.dtype != torch.float32 \
            or not logits.is_contiguous():
        raise TypeError("cross_entropy: logits must be a contiguous fp32 [B, C] tensor")
    _check_distill(logits, teacher, alpha, tau, hard)
    require_gpu(logits, teacher, labels)
    B, Cn = logits.shape
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
        raise TypeError("cross_entropy: labels must be a contiguous int64 [B] tensor of class indices "
                        "(out-of-range labels, e.g. ignore_index = -100, give a NaN loss row)")
    if mix_lam is not None:
        require_gpu(mix_lam)
        if mix_lam.dtype != torch.float32 or tuple(mix_lam.shape) != (B,) or not mix_lam.is_contiguous():
            raise TypeError("cross_entropy: mix_lam must be a contiguous fp32 [B] tensor")
    loss_rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    kd_rows = (torch.zeros if alpha == 0.0 else torch.empty)(B, dtype=torch.float32, device=logits.device)
    dlog = torch.empty_like(logits) if grad_scale is not None else None
    gs = 0.0 if grad_scale is None else grad_scale
    _abi.check(_abi.lib().favit_cross_entropy_distill(_p(logits), _p(teacher), _p(labels), _p(mix_lam), _p(loss_rows),
                                                      _p(kd_rows), _p(dlog), B, Cn, gs, float(label_smoothing), alpha,
                                                      tau, int(hard), _st()), "favit_cross_entropy_distill")
    return loss_rows, dlog, kd_rows


def cross_entropy(logits, labels, grad_scale=None, label_smoothing=0.0, mix_lam=None, teacher=None,
                  distill_alpha=0.0, distill_tau=1.0, distill_hard=False):
    """Returns (loss_rows[B], dlogits or None).  label_smoothing = eps in [0, 1): the loss of
    nn.CrossEntropyLoss(label_smoothing=eps) (favit_cross_entropy_ls); 0 calls favit_cross_entropy.
    mix_lam (fp32 [B] on the device, read when the kernel runs): the target of row b is lam[b] * onehot(labels[b]) +
    (1 - lam[b]) * onehot(labels[B-1-b]), the labels of kernels.batch_mix's pairs (favit_cross_entropy_mix).
    teacher (fp32 [B, C] teacher logits): the distilled loss of cross_entropy_distill with distill_alpha / distill_tau /
    distill_hard, without its kd_rows.  Without a teacher the call is the one of before; a distill_alpha other than 0
    is then an error."""
    if teacher is not None:
        return cross_entropy_distill(logits, teacher, labels, grad_scale, label_smoothing, mix_lam, distill_alpha,
                                     distill_tau, distill_hard)[:2]
    if distill_alpha:
        if not 0.0 <= distill_alpha <= 1.0:
            raise ValueError(f"cross_entropy: distill_alpha must be in [0, 1], got {distill_alpha}")
        raise ValueError("cross_entropy: distill_alpha > 0 needs teacher logits")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"cross_entropy: label_smoothing must be in [0, 1), got {label_smoothing}")
    require_gpu(logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise TypeError("cross_entropy: logits must be a contiguous fp32 [B, C] tensor")
    B, Cn = logits.shape
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
        raise TypeError("cross_entropy: labels must be a contiguous int64 [B] tensor of class indices "
                        "(out-of-range labels, e.g. ignore_index = -100, give a NaN loss row)")
    loss_rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlog = torch.empty_like(logits) if grad_scale is not None else None
    gs = 0.0 if grad_scale is None else grad_scale
    if mix_lam is not None:
        require_gpu(mix_lam)
        if mix_lam.dtype != torch.float32 or tuple(mix_lam.shape) != (B,) or not mix_lam.is_contiguous():
            raise TypeError("cross_entropy: mix_lam must be a contiguous fp32 [B] tensor")
        _abi.check(_abi.lib().favit_cross_entropy_mix(_p(logits), _p(labels), _p(mix_lam), _p(loss_rows), _p(dlog), B,
                                                      Cn, gs, float(label_smoothing), _st()),
                   "favit_cross_entropy_mix")
    elif label_smoothing:
        _abi.check(_abi.lib().favit_cross_entropy_ls(_p(logits), _p(labels), _p(loss_rows), _p(dlog), B, Cn, gs,
                                                     float(label_smoothing), _st()), "favit_cross_entropy_ls")
    else:
        _abi.check(_abi.lib().favit_cross_entropy(_p(logits), _p(labels), _p(loss_rows), _p(dlog), B, Cn, gs, _st()),
                   "favit_cross_entropy")
    return loss_rows, dlog


EVAL_MAX_TOPK = _abi.EVAL_MAX_TOPK
EVAL_STATE_WORDS = _abi.EVAL_STATE_WORDS
EVAL_SLOTS = {name: i for i, name in enumerate(_abi.EVAL_SLOTS)}      # loss_sum, batch_mean_sum, rows, ..., hits


def check_topk(topk):
    """The k values of eval_metrics as a tuple: at most EVAL_MAX_TOPK integers, each >= 1 (checked without a GPU)."""
    ks = tuple(topk)
    if len(ks) > EVAL_MAX_TOPK:
        raise ValueError(f"eval_metrics: at most {EVAL_MAX_TOPK} top-k values per launch, got {len(ks)}")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"eval_metrics: every k must be an integer >= 1, got {k!r}")
    return tuple(min(k, 2 ** 31 - 1) for k in ks)


def eval_metrics(logits, labels, state, loss_rows, pred_rows, rank_rows, topk=(1,), class_total=None,
                 class_correct=None, confusion=None):
    """favit_eval_metrics: two launches, no sync.  logits fp32 [B, C] (rows may be strided, columns not), labels
    int64 [B].  Written: loss_rows fp32, pred_rows / rank_rows int32, [>= B] each (row b: the cross-entropy, the argmax
    with the lowest index on ties, the label's place in a stable descending sort; a label outside [0, C) is ignored: NaN,
    -1, -1).  ADDED to: state, int64 [EVAL_STATE_WORDS] (EVAL_SLOTS names the words; loss_sum and batch_mean_sum hold
    doubles: read them through state.view(torch.float64)), and the optional int64 class_total [C], class_correct [C],
    confusion [C, C] (row = label, column = prediction).  The caller zeroes what is added to."""
    ks = check_topk(topk)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.dtype != torch.float32 \
            or (logits.shape[1] > 1 and logits.stride(1) != 1) or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise TypeError("eval_metrics: logits must be an fp32 [B, C] tensor with contiguous rows")
    B, Cn = logits.shape
    if Cn < 1:
        raise ValueError("eval_metrics: no classes")
    require_gpu(logits, labels, state, loss_rows, pred_rows, rank_rows, class_total, class_correct, confusion)
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
        raise TypeError("eval_metrics: labels must be a contiguous int64 [B] tensor")
    if state.dtype != torch.int64 or state.numel() != EVAL_STATE_WORDS or not state.is_contiguous():
        raise TypeError(f"eval_metrics: state must be {EVAL_STATE_WORDS} contiguous int64")
    for name, t, dt in (("loss_rows", loss_rows, torch.float32), ("pred_rows", pred_rows, torch.int32),
                        ("rank_rows", rank_rows, torch.int32)):
        if t.dtype != dt or t.dim() != 1 or t.numel() < B or not t.is_contiguous():
            raise TypeError(f"eval_metrics: {name} must be a contiguous {dt} vector of at least {B} elements")
    for name, t, n in (("class_total", class_total, Cn), ("class_correct", class_correct, Cn),
                       ("confusion", confusion, Cn * Cn)):
        if t is not None and (t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous()):
            raise TypeError(f"eval_metrics: {name} must be {n} contiguous int64")
    ld = logits.stride(0) if B > 1 else Cn
    k4 = ks + (0,) * (EVAL_MAX_TOPK - len(ks))
    _abi.check(_abi.lib().favit_eval_metrics(_p(logits), ld, _p(labels), _p(loss_rows), _p(pred_rows), _p(rank_rows),
                                             _p(state), _p(class_total), _p(class_correct), _p(confusion), B, Cn,
                                             len(ks), k4[0], k4[1], k4[2], k4[3], _st()), "favit_eval_metrics")


MAPS_MAX_WINDOW = _abi.MAPS_MAX_WINDOW
ROLLOUT_MAX_LAYERS = _abi.ROLLOUT_MAX_LAYERS
ROLLOUT_MAX_L = _abi.ROLLOUT_MAX_L


def _check_qkv(who, qkv, B, L, H, hd):
    if not torch.is_tensor(qkv) or qkv.dim() != 2 or tuple(qkv.shape) != (B * L, 3 * H * hd) \
            or not qkv.is_contiguous() or qkv.dtype not in _DT:
        got = f"{qkv.dtype} {tuple(qkv.shape)}" if torch.is_tensor(qkv) else type(qkv).__name__
        raise ValueError(f"{who}: qkv must be a contiguous fp32 or bf16 [B*L, 3*H*hd] = ({B * L}, {3 * H * hd}) "
                         f"tensor, got {got}")


def mhla_attn_probs(qkv, B, L, H, hd, W, mask=None, head_mean=False):
    """favit_mhla_attn_probs: the window probabilities of mhla_attn_fwd's softmax, recomputed from the stored qkv
    [B*L, 3*H*hd].  fp32 [B, H, L, W], or [B, L, W] with head_mean (heads summed in ascending order, times 1 / H).
    Slot w of row i is key functional.window_indices(L, W)[i, w]; pad copies are slots of their own.  mask as in
    mhla_attn_fwd: masked slots are exactly 0 and a row without a live slot is all zeros."""
    _check_qkv("mhla_attn_probs", qkv, B, L, H, hd)
    if W < 1 or W % 2 == 0:
        raise ValueError(f"mhla_attn_probs: the window must be odd and positive, got W = {W}")
    _check_mhla_mask(mask, qkv, B, L)
    require_gpu(qkv, mask)
    probs = torch.empty((B, L, W) if head_mean else (B, H, L, W), dtype=torch.float32, device=qkv.device)
    _abi.check(_abi.lib().favit_mhla_attn_probs(_p(qkv), _p(probs), _p(mask), B, L, H, hd, W, dt(qkv),
                                                1 if head_mean else 0, _st()), "favit_mhla_attn_probs")
    return probs


def sdpa_probs(qkv, B, L, H, hd, key_keep=None, scale=None, head_mean=False):
    """favit_sdpa_probs: softmax(scale * q k^T) of the dense self-attention on qkv [B*L, 3*H*hd] (q, k = column blocks
    0 and D, DenseChain's layout).  fp32 [B, H, L, L], or [B, L, L] with head_mean.  key_keep: contiguous uint8 / bool
    [B, L] (0 masks the key) or None; scale defaults to hd ** -0.5."""
    _check_qkv("sdpa_probs", qkv, B, L, H, hd)
    if key_keep is not None and tuple(key_keep.shape) != (B, L):
        raise ValueError(f"sdpa_probs: key_keep must have shape ({B}, {L}), got {tuple(key_keep.shape)}")
    _check_dense_mask("sdpa_probs", key_keep, L, 0, B, L, L)
    require_gpu(qkv, key_keep)
    probs = torch.empty((B, L, L) if head_mean else (B, H, L, L), dtype=torch.float32, device=qkv.device)
    _abi.check(_abi.lib().favit_sdpa_probs(_p(qkv), _p(probs), _p(key_keep), B, L, H, hd, dt(qkv),
                                           float(hd ** -0.5 if scale is None else scale), 1 if head_mean else 0, _st()),
               "favit_sdpa_probs")
    return probs


def attn_rollout(probs, widths, cls_row=0, residual=0.5):
    """favit_attn_rollout: attention rollout of the row cls_row through a stack of head-mean maps, one launch.
    probs[k]: block k's map, contiguous fp32 [B, L, W_k] (widths[k] = W_k, odd) or [B, L, L] (widths[k] = 0, dense), in
    block order, at most ROLLOUT_MAX_LAYERS of them; L <= ROLLOUT_MAX_L.  Returns fp32 [B, L]: r = e_cls_row, and from
    the last block to the first r <- residual * r + (1 - residual) * r P_k.  Bitwise reproducible."""
    probs, widths = list(probs), [int(w) for w in widths]
    n = len(probs)
    if not 1 <= n <= ROLLOUT_MAX_LAYERS or len(widths) != n:
        raise ValueError(f"attn_rollout: 1..{ROLLOUT_MAX_LAYERS} maps with one width each, got {n} maps and "
                         f"{len(widths)} widths")
    if not torch.is_tensor(probs[0]) or probs[0].dim() != 3:
        raise ValueError("attn_rollout: every map must be a [B, L, W] or [B, L, L] tensor")
    B, L = probs[0].shape[:2]
    for k, (p, w) in enumerate(zip(probs, widths)):
        if w < 0 or (w > 0 and w % 2 == 0):
            raise ValueError(f"attn_rollout: widths[{k}] = {w} is neither 0 (dense) nor an odd window")
        want = (B, L, w if w > 0 else L)
        if not torch.is_tensor(p) or p.dtype != torch.float32 or tuple(p.shape) != want or not p.is_contiguous():
            got = f"{p.dtype} {tuple(p.shape)}" if torch.is_tensor(p) else type(p).__name__
            raise ValueError(f"attn_rollout: map {k} must be a contiguous fp32 tensor of shape {want}, got {got}")
    if not 0 <= cls_row < L:
        raise ValueError(f"attn_rollout: cls_row = {cls_row} outside [0, {L})")
    if not 0.0 <= residual <= 1.0:
        raise ValueError(f"attn_rollout: residual = {residual} outside [0, 1]")
    if L > ROLLOUT_MAX_L:
        raise ValueError(f"attn_rollout: L = {L} exceeds ROLLOUT_MAX_L = {ROLLOUT_MAX_L} (two rows of L floats in LDS)")
    require_gpu(*probs)
    out = torch.empty((B, L), dtype=torch.float32, device=probs[0].device)
    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in probs])
    ws = (C.c_int32 * n)(*widths)
    _abi.check(_abi.lib().favit_attn_rollout(n, ptrs, ws, _p(out), cls_row, B, L, float(residual), _st()),
               "favit_attn_rollout")
    return out


POS_RESAMPLE_MAX_L = _abi.POS_RESAMPLE_MAX_L


def _cubic(x, a):
    x = abs(x)
    if x <= 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return a * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


def pos_resample_matrix(g_in: int, g_out: int, antialias: bool = True) -> torch.Tensor:
    """The float64 matrix M [g_out, g_in] of one axis of the bicubic resampling of a grid side g_in to g_out
    (align_corners=False): resampling a g_in x g_in grid X is M X M^T.  antialias=False is torch's plain bicubic
    (a = -0.75, four taps at floor(src) - 1 .. + 2, indices clamped to the grid and accumulated); antialias=True is
    torch's and Pillow's antialiased bicubic (a = -0.5, support 2 * max(scale, 1), weights normalised to sum to 1),
    timm's default for position embeddings.  Equal sides give the identity exactly.  Built in Python floats."""
    g_in, g_out = int(g_in), int(g_out)
    if g_in < 1 or g_out < 1:
        raise ValueError(f"pos_resample_matrix: grid sides must be >= 1, got {g_in} -> {g_out}")
    M = np.zeros((g_out, g_in), dtype=np.float64)
    scale = g_in / g_out
    for d in range(g_out):
        if antialias:
            support, inv, center = 2.0 * max(scale, 1.0), 1.0 / max(scale, 1.0), scale * (d + 0.5)
            xmin, xmax = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), g_in)
            w = [_cubic((j + xmin - center + 0.5) * inv, -0.5) for j in range(xmax - xmin)]
            tot = sum(w)
            for j, v in enumerate(w):
                M[d, xmin + j] = v / tot
        else:
            src = (d + 0.5) * scale - 0.5
            f = math.floor(src)
            t = src - f
            for k in range(-1, 3):
                M[d, min(max(f + k, 0), g_in - 1)] += _cubic(k - t, -0.75)
    return torch.from_numpy(M)


def _csr(M32: np.ndarray):
    """(rowptr int32, cols int32, vals fp32) of the non-zero entries of a 2-D fp32 matrix, columns ascending."""
    rows, cols = np.nonzero(M32)                               # row-major order: rows ascending, then columns
    rowptr = np.zeros(M32.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=M32.shape[0]), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), np.ascontiguousarray(M32[rows, cols], dtype=np.float32)


_POS_TABLES = {}          # (device index, g_in, g_out, antialias) -> ((rowptr, cols, vals) of M, the same of M^T)


def pos_resample_tables(g_in: int, g_out: int, antialias: bool, device):
    """The device tables favit_pos_resample reads for (g_in -> g_out, antialias): the compressed rows of
    pos_resample_matrix rounded to fp32, and those of its transpose (the adjoint's table: the same fp32 values).  Built,
    checked and uploaded ONCE per device and kept, so that a later call -- inside a HIP graph capture too -- allocates
    and copies nothing; the eager warm-up steps of GraphedStep / GraphedEval fill the cache."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(g_in), int(g_out), bool(antialias))
    hit = _POS_TABLES.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"pos_resample: no table for {g_in} -> {g_out} on this device yet, and a HIP graph is being "
                               "captured (an upload cannot be captured): run one eager step at this resolution first")
        M32 = pos_resample_matrix(g_in, g_out, antialias).numpy().astype(np.float32)
        both = []
        for mat, n_cols in ((M32, g_in), (np.ascontiguousarray(M32.T), g_out)):
            rowptr, cols, vals = _csr(mat)
            if rowptr[0] != 0 or np.any(np.diff(rowptr) < 0) or rowptr[-1] != len(cols) or len(cols) != len(vals) \
                    or cols.min() < 0 or cols.max() >= n_cols:
                raise AssertionError(f"pos_resample: malformed table for {g_in} -> {g_out}")
            both.append(tuple(torch.from_numpy(t).to(dev) for t in (rowptr, cols, vals)))
        hit = _POS_TABLES[key] = tuple(both)
    return hit


def pos_resample(x, g_in: int, g_out: int, antialias: bool = True, n_prefix: int = 1, adjoint: bool = False):
    """favit_pos_resample.  x: contiguous fp32 [n_prefix + g_in^2, D] -> [n_prefix + g_out^2, D]: the n_prefix leading
    rows copied, the grid rows resampled with M = pos_resample_matrix(g_in, g_out, antialias) along both axes.
    adjoint=True applies the transpose instead (the backward): x is [n_prefix + g_out^2, D], the result
    [n_prefix + g_in^2, D].  One launch, no atomics, bitwise reproducible; D % 4 == 0."""
    g_in, g_out, n_prefix = int(g_in), int(g_out), int(n_prefix)
    g_src, g_dst = (g_out, g_in) if adjoint else (g_in, g_out)
    if n_prefix not in (0, 1):
        raise ValueError(f"pos_resample: n_prefix must be 0 or 1, got {n_prefix}")
    if g_in < 1 or g_out < 1 or max(g_in, g_out) ** 2 + n_prefix > POS_RESAMPLE_MAX_L:
        raise ValueError(f"pos_resample: grid sides {g_in} -> {g_out} outside 1 .. {POS_RESAMPLE_MAX_L} token rows")
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() \
            or x.shape[0] != n_prefix + g_src * g_src:
        got = f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else type(x).__name__
        raise ValueError(f"pos_resample: x must be a contiguous fp32 [{n_prefix + g_src * g_src}, D] tensor, got {got}")
    D = x.shape[1]
    if D < 4 or D % 4:
        raise ValueError(f"pos_resample: D = {D} must be a positive multiple of 4")
    require_gpu(x)
    rowptr, cols, vals = pos_resample_tables(g_in, g_out, antialias, x.device)[1 if adjoint else 0]
    y = torch.empty((n_prefix + g_dst * g_dst, D), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().favit_pos_resample(_p(x), _p(y), _p(rowptr), _p(cols), _p(vals), g_src, g_dst, n_prefix, D,
                                             _st()), "favit_pos_resample")
    return y


GRAD_NORM_MAX_BUFS = _abi.GRAD_NORM_MAX_BUFS


def grad_norm_workspace(device) -> torch.Tensor:
    """An (uninitialised) workspace for grad_norm; allocate once and pass it as `ws`."""
    return torch.empty(int(_abi.lib().favit_grad_norm_workspace()) // 8, dtype=torch.float64, device=device)


def grad_norm(bufs, scale=1.0, max_norm=0.0, out=None, skipped=None, ws=None):
    """Global L2 norm of up to 16 flat fp32 tensors (any 4-byte-aligned start, any length) on the device, bitwise
    reproducible (favit_grad_norm).  Returns `out`, two fp32: out[0] = scale * norm, out[1] = the coefficient of
    torch.nn.utils.clip_grad_norm_, min(1, max_norm / (out[0] + 1e-6)) -- 1 without max_norm, NaN when out[0] is not
    finite, in which case `skipped` (one int32 on the device, optional) is incremented.  No host sync."""
    bufs = list(bufs)
    n = len(bufs)
    if n > GRAD_NORM_MAX_BUFS:
        raise ValueError(f"grad_norm: at most {GRAD_NORM_MAX_BUFS} buffers per call, got {n}")
    if not n and out is None:
        raise ValueError("grad_norm: no buffer and no `out` to take the device from")
    require_gpu(*bufs, out, skipped, ws)
    for t in bufs:
        if t.dtype != torch.float32 or (t.numel() and not t.is_contiguous()):
            raise TypeError("grad_norm: every buffer must be a contiguous fp32 tensor")
    dev = bufs[0].device if n else out.device
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() != 2 or not out.is_contiguous():
        raise TypeError("grad_norm: out must be two contiguous fp32")
    if skipped is not None and (skipped.dtype != torch.int32 or skipped.numel() != 1):
        raise TypeError("grad_norm: skipped must be one int32")
    if ws is None:
        ws = grad_norm_workspace(dev)
    ptrs = (C.c_void_p * max(1, n))(*[t.data_ptr() if t.numel() else None for t in bufs])
    lens = (C.c_int64 * max(1, n))(*[t.numel() for t in bufs])
    _abi.check(_abi.lib().favit_grad_norm(n, ptrs, lens, float(scale), float(max_norm), _p(out), _p(skipped), _p(ws),
                                          ws.numel() * ws.element_size(), _st()), "favit_grad_norm")
    return out


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, p_lp=None, coef=None, skip_nonfinite=False,
          ema=None, ema_decay=0.0):
    """coef: one fp32 on the DEVICE (grad_norm's out[1:2]) the gradient is multiplied by when the kernel runs
    (favit_adamw_clip); with skip_nonfinite a non-finite coefficient leaves p, m, v and p_lp untouched.
    ema: a contiguous fp32 tensor of p's length that the same launch moves towards the updated parameters,
    ema = ema_decay * ema + (1 - ema_decay) * p_new (favit_adamw_ema / favit_adamw_clip_ema); a skipped launch
    leaves it untouched too.  None: the launches without the average."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    if ema is not None:
        require_gpu(ema)
        if ema.dtype != torch.float32 or ema.numel() != p.numel() or (ema.numel() and not ema.is_contiguous()):
            raise TypeError("adamw: ema must be a contiguous fp32 tensor of p's length")
        if not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"adamw: ema_decay must be in [0, 1], got {ema_decay}")
    if coef is None:
        if skip_nonfinite:
            raise ValueError("adamw: skip_nonfinite needs the device coefficient of grad_norm (coef)")
        if ema is not None:
            _abi.check(_abi.lib().favit_adamw_ema(_p(p), _p(g), _p(m), _p(v), _p(p_lp), _p(ema), p.numel(), lr, beta1,
                                                  beta2, eps, wd, bc1, bc2, grad_scale, float(ema_decay), _st()),
                       "favit_adamw_ema")
            return
        _abi.check(_abi.lib().favit_adamw(_p(p), _p(g), _p(m), _p(v), _p(p_lp), p.numel(), lr, beta1, beta2, eps, wd,
                                          bc1, bc2, grad_scale, _st()), "favit_adamw")
        return
    require_gpu(coef)
    if coef.dtype != torch.float32 or coef.numel() != 1:
        raise TypeError("adamw: coef must be one fp32 on the device")
    if ema is not None:
        _abi.check(_abi.lib().favit_adamw_clip_ema(_p(p), _p(g), _p(m), _p(v), _p(p_lp), _p(ema), p.numel(), lr, beta1,
                                                   beta2, eps, wd, bc1, bc2, grad_scale, _p(coef),
                                                   int(bool(skip_nonfinite)), float(ema_decay), _st()),
                   "favit_adamw_clip_ema")
        return
    _abi.check(_abi.lib().favit_adamw_clip(_p(p), _p(g), _p(m), _p(v), _p(p_lp), p.numel(), lr, beta1, beta2, eps, wd,
                                           bc1, bc2, grad_scale, _p(coef), int(bool(skip_nonfinite)), _st()),
               "favit_adamw_clip")


ADAMW_MAX_SEGMENTS, ADAMW_SEG_ALIGN = _abi.ADAMW_MAX_SEGMENTS, _abi.ADAMW_SEG_ALIGN


def _adamw_limits():
    """(FAVIT_ADAMW_MAX_SEGMENTS, FAVIT_ADAMW_SEG_ALIGN) as the loaded library reports them: a library built from
    another header than the one _abi read is refused."""
    got = (int(_abi.lib().favit_adamw_multi_max_segments()), int(_abi.lib().favit_adamw_multi_align()))
    if got != (ADAMW_MAX_SEGMENTS, ADAMW_SEG_ALIGN):
        raise _abi.FavitLibraryError("libfavit.so and _abi.AdamwMulti disagree on the segment table's size")
    return got


def adamw_multi(p, g, m, v, ends, lrs, wds, beta1, beta2, eps, step, grad_scale=1.0, p_lp=None, coef=None,
                skip_nonfinite=False, ema=None, ema_decay=0.0):
    """adamw() over ONE arena cut into len(ends) segments, in one launch (favit_adamw_multi): segment s covers
    [ends[s-1], ends[s]) (ends exclusive, strictly ascending multiples of ADAMW_SEG_ALIGN, the last one p.numel()) and
    is updated with lrs[s] and wds[s]; everything else is shared.  Per element the bits are adamw()'s on the segment's
    slice.  The table is a by-value argument of the launch: plain Python numbers, read at every call.  coef,
    skip_nonfinite, ema, ema_decay: as in adamw().  ValueError for a table the library would refuse."""
    _adamw_limits()
    ends, lrs, wds = [int(e) for e in ends], [float(x) for x in lrs], [float(x) for x in wds]
    require_gpu(p, g, m, v, p_lp, ema, coef)
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise TypeError(f"adamw_multi: {name} must be a contiguous fp32 tensor of p's length")
    n = p.numel()
    if p_lp is not None and (p_lp.dtype != torch.bfloat16 or p_lp.numel() != n or not p_lp.is_contiguous()):
        raise TypeError("adamw_multi: p_lp must be a contiguous bf16 tensor of p's length")
    if ema is not None:
        if ema.dtype != torch.float32 or ema.numel() != n or not ema.is_contiguous():
            raise TypeError("adamw_multi: ema must be a contiguous fp32 tensor of p's length")
        if not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"adamw_multi: ema_decay must be in [0, 1], got {ema_decay}")
    if coef is None:
        if skip_nonfinite:
            raise ValueError("adamw_multi: skip_nonfinite needs the device coefficient of grad_norm (coef)")
    elif coef.dtype != torch.float32 or coef.numel() != 1:
        raise TypeError("adamw_multi: coef must be one fp32 on the device")
    if not 1 <= len(ends) <= ADAMW_MAX_SEGMENTS:
        raise ValueError(f"adamw_multi: 1..{ADAMW_MAX_SEGMENTS} segments per launch, got {len(ends)}")
    if len(lrs) != len(ends) or len(wds) != len(ends):
        raise ValueError(f"adamw_multi: {len(ends)} ends, {len(lrs)} learning rates and {len(wds)} weight decays")
    prev = 0
    for s, e in enumerate(ends):
        if e <= prev or e % ADAMW_SEG_ALIGN:
            raise ValueError(f"adamw_multi: end {e} of segment {s} must be a multiple of {ADAMW_SEG_ALIGN} above the "
                             f"previous end {prev}")
        prev = e
    if prev != n:
        raise ValueError(f"adamw_multi: the last end is {prev}, the arena has {n} elements")
    for name, t, a in (("p", p, 16), ("g", g, 16), ("m", m, 16), ("v", v, 16), ("ema", ema, 16), ("p_lp", p_lp, 8)):
        if t is not None and t.data_ptr() % a:
            raise ValueError(f"adamw_multi: {name} must be {a}-byte aligned")
    d = _abi.AdamwMulti()
    d.p, d.g, d.m, d.v, d.p_bf16, d.ema, d.coef = _p(p), _p(g), _p(m), _p(v), _p(p_lp), _p(ema), _p(coef)
    d.n, d.count, d.skip_nonfinite = n, len(ends), int(bool(skip_nonfinite))
    for s in range(len(ends)):
        d.end[s], d.lr[s], d.weight_decay[s] = ends[s], lrs[s], wds[s]
    d.beta1, d.beta2, d.eps, d.bias_c1, d.bias_c2 = beta1, beta2, eps, 1.0 - beta1 ** step, 1.0 - beta2 ** step
    d.grad_scale, d.ema_decay = grad_scale, float(ema_decay)
    _abi.check(_abi.lib().favit_adamw_multi(C.byref(d), _st()), "favit_adamw_multi")


def swap_params(a, b, a_lp=None):
    """Exchange the contents of two flat fp32 tensors in place and, with a_lp, rewrite the bf16 mirror of `a` from
    its new contents, in one pass (favit_swap_params).  No address changes."""
    require_gpu(a, b, a_lp)
    for t in (a, b):
        if t.dtype != torch.float32 or (t.numel() and not t.is_contiguous()):
            raise TypeError("swap_params: a and b must be contiguous fp32 tensors")
    if a.numel() != b.numel() or (a_lp is not None and (a_lp.dtype != torch.bfloat16 or a_lp.numel() != a.numel()
                                                         or (a_lp.numel() and not a_lp.is_contiguous()))):
        raise TypeError("swap_params: b (fp32) and a_lp (bf16, optional) must have a's length")
    _abi.check(_abi.lib().favit_swap_params(_p(a), _p(b), _p(a_lp), a.numel(), _st()), "favit_swap_params")
