"""CPU checks of the mask validation that runs before any attention kernel is launched.

The kernels index their mask with the extents they are given (MHLA: mask[(b*L + i)*L + j], dense: mask[b*m_sb +
q*m_sq + k], one byte per element), so a mask of another shape, type or layout would be read past its end, or as the
bytes of another type, on the device.  kernels.mhla_attn_fwd / _bwd, kernels.sdpa_fwd / _bwd / softmax_fwd and the
attention chains of functional.py refuse such a mask with a ValueError before they look at the device of anything:
every call here uses CPU tensors, and a check placed after require_gpu would raise its RuntimeError instead.

These refusals have no GPU test on purpose: on code without the check the same call reads out of bounds."""
import pytest
import torch

B, L, H, HD, W = 2, 12, 2, 16, 7
D = H * HD


def _qkv(dtype=torch.float32):
    return torch.zeros(B * L, 3 * D, dtype=dtype), torch.zeros(B * L, D, dtype=dtype)


BAD_MHLA = {
    "key-keep [B, L]": lambda: torch.ones(B, L, dtype=torch.uint8),
    "[L, L]": lambda: torch.ones(L, L, dtype=torch.uint8),
    "[B, 1, L, L]": lambda: torch.ones(B, 1, L, L, dtype=torch.uint8),
    "[B, L, L + 1]": lambda: torch.ones(B, L, L + 1, dtype=torch.uint8),
    "one image short": lambda: torch.ones(B - 1, L, L, dtype=torch.uint8),
    "float32": lambda: torch.ones(B, L, L, dtype=torch.float32),
    "int64": lambda: torch.ones(B, L, L, dtype=torch.int64),
    "transposed view": lambda: torch.ones(B, L, L, dtype=torch.uint8).transpose(1, 2),
    "strided view": lambda: torch.ones(B, L, 2 * L, dtype=torch.uint8)[:, :, ::2],
    "a list": lambda: [[1] * L] * L,
}


@pytest.mark.parametrize("kind", sorted(BAD_MHLA))
def test_mhla_kernel_wrappers_refuse_a_bad_mask(favit, kind):
    K = favit.kernels
    qkv, dout = _qkv()
    mask = BAD_MHLA[kind]()
    with pytest.raises(ValueError, match=rf"\({B}, {L}, {L}\)") as e:
        K.mhla_attn_fwd(qkv, B, L, H, HD, W, mask)
    if torch.is_tensor(mask):
        assert str(tuple(mask.shape)) in str(e.value), "the message names the actual shape"
    with pytest.raises(ValueError, match=rf"\({B}, {L}, {L}\)"):
        K.mhla_attn_fwd(qkv, B, L, H, HD, W, mask, want_lse=True)
    with pytest.raises(ValueError, match=rf"\({B}, {L}, {L}\)"):
        K.mhla_attn_bwd(qkv, dout, B, L, H, HD, W, mask)
    with pytest.raises(ValueError, match=rf"\({B}, {L}, {L}\)"):
        K.mhla_attn_bwd(qkv, dout, B, L, H, HD, W, mask, o=dout, lse=torch.zeros(B, H, L))


def test_mhla_kernel_wrappers_refuse_a_mask_on_another_device(favit):
    qkv, _ = _qkv()
    with pytest.raises(ValueError, match="on cpu, got .* on meta"):
        favit.kernels.mhla_attn_fwd(qkv, B, L, H, HD, W, torch.ones(B, L, L, dtype=torch.uint8, device="meta"))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool])
def test_a_good_mhla_mask_passes_the_check_and_reaches_the_device_check(favit, dtype):
    """uint8 and bool [B, L, L], contiguous: no ValueError; with CPU tensors the call then ends in require_gpu."""
    qkv, dout = _qkv()
    mask = torch.ones(B, L, L, dtype=dtype)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        favit.kernels.mhla_attn_fwd(qkv, B, L, H, HD, W, mask)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        favit.kernels.mhla_attn_bwd(qkv, dout, B, L, H, HD, W, mask)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        favit.kernels.mhla_attn_fwd(qkv, B, L, H, HD, W, None)


def _views(favit, Lq, Lk):
    V = favit.functional._View
    q, k = torch.zeros(B * Lq, D), torch.zeros(B * Lk, D)
    return V(q, 0, D, Lq * D, HD), V(k, 0, D, Lk * D, HD)


@pytest.mark.parametrize("form", ["full", "keys"])
def test_dense_kernel_wrappers_refuse_a_short_mask(favit, form):
    """One element fewer than (B - 1) m_sb + (Lq - 1) m_sq + Lk is refused, exactly that many pass on to the device check."""
    K = favit.kernels
    Lq, Lk = 5, 9
    m_sb, m_sq = (Lq * Lk, Lk) if form == "full" else (Lk, 0)
    need = (B - 1) * m_sb + (Lq - 1) * m_sq + Lk
    qv, kv = _views(favit, Lq, Lk)
    lse = torch.zeros(B * H, Lq)
    S = torch.zeros(B * H, Lq, Lk)

    def calls(mask):
        yield lambda: K.sdpa_fwd(qv, kv, kv, qv, B, H, Lq, Lk, HD, 0.25, mask, m_sb, m_sq)
        yield lambda: K.sdpa_bwd(qv, kv, kv, qv, qv, qv, kv, kv, lse, B, H, Lq, Lk, HD, 0.25, mask, m_sb, m_sq)
        yield lambda: K.softmax_fwd(S, torch.float32, H, B * H, Lq, Lk, mask, m_sb, m_sq)

    for bad in (torch.ones(need - 1, dtype=torch.uint8), torch.ones(Lk, dtype=torch.uint8),
                torch.ones(need, dtype=torch.float32), torch.ones(2 * need, dtype=torch.uint8)[::2]):
        for call in calls(bad):
            with pytest.raises(ValueError, match=rf"at least {need} elements"):
                call()
    for good in (torch.ones(need, dtype=torch.uint8), torch.ones(need, dtype=torch.bool), None):
        for call in calls(good):
            with pytest.raises(RuntimeError, match="CPU tensor"):
                call()
    if form == "full":      # a [B, Lk] key-keep mask handed over with the strides of a full mask: the mistake the check is for
        for call in calls(torch.ones(B, Lk, dtype=torch.uint8)):
            with pytest.raises(ValueError, match="at least"):
                call()


def test_attention_chains_refuse_a_mask_of_another_form(favit):
    """MHLAChain takes [B, L, L], DenseChain the key-keep [B, L], CrossChain [B, Lq, Lk]; each names itself and both
    shapes, before it touches its parameters (None here) or any device."""
    F = favit.functional
    Lq, Lk = 5, 9
    xn = torch.zeros(B * L, D)
    u8 = lambda *s: torch.ones(*s, dtype=torch.uint8)
    for bad in (u8(B, L), u8(L, L), u8(B, L, L + 1), u8(B, 1, L, L), u8(1, L, L)):
        with pytest.raises(ValueError, match=rf"MHLAChain.*\[B, L, L\] = \({B}, {L}, {L}\), got \({', '.join(map(str, bad.shape))}\)"):
            F.MHLAChain(H, W).fwd(xn, None, B, L, None, bad, False)
    for bad in (u8(B, L, L), u8(L), u8(B, L + 1), u8(L, B)):
        with pytest.raises(ValueError, match=rf"DenseChain.*\[B, L\] = \({B}, {L}\), got \("):
            F.DenseChain(H, torch_mha=True).fwd(xn, None, B, L, None, bad, False)
    for bad in (u8(B, Lk), u8(Lq, Lk), u8(B, Lk, Lq), u8(B, 1, Lk)):
        with pytest.raises(ValueError, match=rf"CrossChain.*\[B, Lq, Lk\] = \({B}, {Lq}, {Lk}\), got \("):
            F.CrossChain(H).fwd(torch.zeros(B * Lq, D), torch.zeros(B * Lk, D), None, B, Lq, Lk, None, bad, False)
    # a mask of the right form passes the check: the chain goes on to unpack its parameters
    for chain, args in ((F.MHLAChain(H, W), (xn, None, B, L, None, u8(B, L, L), False)),
                        (F.DenseChain(H, torch_mha=True), (xn, None, B, L, None, u8(B, L), False)),
                        (F.CrossChain(H), (xn, xn, None, B, L, L, None, u8(B, L, L), False))):
        with pytest.raises(TypeError):
            chain.fwd(*args)


def test_modules_refuse_a_key_keep_mask_before_any_launch(favit):
    """The public path: MultiHeadLatentAttention(x, attention_mask) with the [B, L] mask that the dense blocks next door
    document.  On the CPU the module call ends at the device check of its input, so the chain is reached through the op
    the module builds, as models/mhla.py builds it."""
    F = favit.functional
    m = favit.models.mhla.MultiHeadLatentAttention(D, H, W)
    x = torch.zeros(B, L, D)
    op = F.AttnOp(F.MHLAChain(H, W), F._mask_u8(torch.ones(B, L, dtype=torch.bool)), False)
    prm = [p.detach() for p in m.parameters()]
    with pytest.raises(ValueError, match="MHLAChain"):
        op.chain.fwd(x.reshape(B * L, D), prm, B, L, None, op.mask, op.training)
