"""Host side of the narrowed MLP halves: the plan function that moves every row cut of a
CLS-only encoder from in front of a block up into the block below it, and the two-row-count layout queries of the
native block chains.  No GPU: both are host arithmetic."""
import ctypes

import pytest

ENCODERS = [(197, 7, 12), (577, 7, 12), (50, 7, 4), (30, 3, 5), (17, 7, 3), (12, 5, 3)]


def _rows(cuts, L):
    return [L if c is None else sum(c) for c in cuts]


def _cut_positions(cuts, mcuts, L):
    """What EncoderOp.fwd does with the two lists: (cuts in front of a block, cuts inside a block, rows behind)."""
    front = inside = 0
    for c, m in zip(cuts, mcuts):
        if c is not None and sum(c) < L:
            front, L = front + 1, sum(c)
        if m is not None and sum(m) < L:
            inside, L = inside + 1, sum(m)
    return front, inside, L


@pytest.mark.parametrize("L,W,depth", ENCODERS)
def test_mlp_rows_are_the_next_blocks_rows(favit, L, W, depth):
    F = favit.functional
    cuts = F.cls_plan(L, W, depth)
    m = F.mlp_narrow_plan(cuts)
    assert len(m) == depth and m[-1] is None, "the last block keeps its rows: the caller reads them"
    rows = _rows(cuts, L)
    for k in range(depth - 1):
        if rows[k + 1] < rows[k]:
            assert m[k] == cuts[k + 1]
        else:
            assert m[k] is None
    today = sum(1 for k, c in enumerate(cuts) if c is not None and sum(c) < ([L] + rows)[k])
    front, inside, behind = _cut_positions(cuts, m, L)
    assert front + inside == today, "the cuts move, their number stays"
    assert front == (1 if cuts[0] is not None else 0), "only the first block can still have a cut in front of it"
    assert behind == rows[-1]
    # every pair is a (head, tail) of the compact layout it is cut out of
    for k in range(depth):
        if m[k] is not None and cuts[k] is not None:
            assert m[k][0] <= cuts[k][0] and m[k][1] <= cuts[k][1]


def test_all_rows_then_cut_narrows(favit):
    F = favit.functional
    cuts = F.cls_plan(30, 7, 7)
    assert cuts[:2] == [None, None] and cuts[2] is not None
    m = F.mlp_narrow_plan(cuts)
    assert m[0] is None and m[1] == cuts[2], "block 2 runs on all rows, its MLP half on block 3's 29"
    assert _cut_positions(cuts, m, 30) == (0, 5, 5)
    assert F.mlp_narrow_plan([None, None]) == [None, None]
    assert F.mlp_narrow_plan([None], after=(4, 1)) == [(4, 1)]


@pytest.mark.parametrize("L,W,depth,per", [(50, 7, 4, 2), (197, 7, 12, 6), (197, 7, 12, 5), (30, 7, 7, 4)])
def test_segments_with_and_without_a_known_successor(favit, L, W, depth, per):
    F = favit.functional
    cuts = F.cls_plan(L, W, depth)
    whole = F.mlp_narrow_plan(cuts)
    today = sum(1 for k, c in enumerate(cuts) if c is not None and sum(c) < ([L] + _rows(cuts, L))[k])
    for known in (True, False):
        rows, n_cuts, joined = L, 0, []
        for i in range(0, depth, per):
            seg = cuts[i:i + per]
            after = cuts[i + per] if known and i + per < depth else None
            m = F.mlp_narrow_plan(seg, after=after)
            joined += m
            if not known:
                assert m[-1] is None, "nobody said what the next node reads: its first block cuts in front of itself"
            front, inside, rows = _cut_positions(seg, m, rows)
            n_cuts += front + inside
        assert rows == _rows(cuts, L)[-1] and n_cuts == today
        if known:
            assert joined == whole


def test_switch(favit, monkeypatch):
    F = favit.functional
    monkeypatch.delenv("FAVIT_NO_MLP_NARROW", raising=False)
    assert F.mlp_narrow_on()
    monkeypatch.setenv("FAVIT_NO_MLP_NARROW", "1")
    assert not F.mlp_narrow_on()


# ------------------------------------------------------------------ layout queries
def _desc(favit, B, n, D, H, W, hidden, training):
    d = favit._abi.BlockDesc()
    d.B, d.n, d.D, d.H, d.W, d.hidden, d.training, d.eps = B, n, D, H, W, hidden, training, 1e-5
    return d


def _mlp(favit, n_mlp):
    r = favit._abi.BlockMlp()
    r.n_mlp = n_mlp
    return r


# (B, n, n_mlp, D, H, W, hidden)
LAYOUTS = [(3, 17, 11, 128, 2, 7, 512), (3, 11, 5, 128, 2, 7, 512), (2, 11, 9, 192, 3, 3, 768), (2, 5, 3, 192, 3, 3, 768),
           (3, 23, 17, 128, 2, 7, 512), (256, 71, 65, 384, 6, 7, 1536), (256, 11, 5, 384, 6, 7, 1536),
           (64, 71, 65, 768, 12, 7, 3072), (3, 17, 1, 128, 2, 7, 512)]


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("B,n,n_mlp,D,H,W,hidden", LAYOUTS)
def test_two_row_count_layouts(favit, B, n, n_mlp, D, H, W, hidden, training):
    lib, A = favit._abi.lib(), favit._abi
    d, r = _desc(favit, B, n, D, H, W, hidden, training), _mlp(favit, n_mlp)
    M, Mm = B * n, B * n_mlp
    tape = dict(xn1=M * D * 2, mu1=M * 4, rs1=M * 4, qkv=M * 3 * D * 2, o=M * D * 2, lse=B * H * n * 4 if training else 0,
                x1=M * D * 4, xn2=Mm * D * 2, mu2=Mm * 4, rs2=Mm * 4, h=Mm * hidden * 2, pre=Mm * hidden * 2, x2=Mm * D * 4)
    to = (ctypes.c_int64 * len(A.BLOCK_TAPE_SLOTS))()
    total = lib.favit_mhla_block_tape_layout2(ctypes.byref(d), ctypes.byref(r), to)
    assert total == lib.favit_mhla_block_tape_layout2(ctypes.byref(d), ctypes.byref(r), None) > 0

    def check(names, offsets, total, sizes):
        end = 0
        for k, off in zip(names, offsets):
            assert off % 256 == 0 and off >= end, k
            end = off + sizes[k]
        assert 0 <= total - end < 256 and total % 256 == 0
        ends = list(offsets[1:]) + [total]
        for k, off, e in zip(names, offsets, ends):
            assert e - off == (sizes[k] + 255) // 256 * 256, k       # the slot is exactly its buffer, rounded up
    check(A.BLOCK_TAPE_SLOTS, list(to), total, tape)
    np1, np2 = min(2048, (M + 3) // 4), min(2048, (Mm + 3) // 4)
    for want_lp in (0, 1):
        bwd = dict(dpre=Mm * hidden * 2, dxn2=Mm * D * 2, g1_f32=Mm * D * 4, g1_lp=0, do=M * D * 2, dqkv=M * 3 * D * 2,
                   dxn1=M * D * 2, g_out_f32=M * D * 4, g_out_lp=M * D * 2 if want_lp else 0, part1=2 * np1 * D * 4,
                   part2=2 * np2 * D * 4)
        bo = (ctypes.c_int64 * len(A.BLOCK_BWD_SLOTS))()
        nb = lib.favit_mhla_block_bwd_layout2(ctypes.byref(d), ctypes.byref(r), want_lp, bo)
        check(A.BLOCK_BWD_SLOTS, list(bo), nb, bwd)
    # the Python-side plan is the same table
    plan = favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, training, n_mlp=n_mlp)
    assert plan.tape_bytes == total and [plan.off[k][0] for k in A.BLOCK_TAPE_SLOTS] == list(to)
    assert (plan.M, plan.Mm, plan.n_mlp, plan.nparts, plan.nparts2) == (M, Mm, n_mlp, np1, np2)
    assert plan.boff[1]["g1_lp"][1] == 0 and plan.boff[1]["part2"][1] >= 2 * np2 * D * 4


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("B,n,D,H,W,hidden", [(3, 17, 128, 2, 7, 512), (2, 11, 192, 3, 3, 768), (256, 71, 384, 6, 7, 1536)])
def test_equal_row_counts_reproduce_the_one_row_count_layouts(favit, B, n, D, H, W, hidden, training):
    lib, A = favit._abi.lib(), favit._abi
    d, r = _desc(favit, B, n, D, H, W, hidden, training), _mlp(favit, n)
    t1, t2 = (ctypes.c_int64 * 13)(), (ctypes.c_int64 * 13)()
    assert lib.favit_mhla_block_tape_layout(ctypes.byref(d), t1) == lib.favit_mhla_block_tape_layout2(ctypes.byref(d), ctypes.byref(r), t2)
    assert list(t1) == list(t2)
    for want_lp in (0, 1):
        b1, b2 = (ctypes.c_int64 * 11)(), (ctypes.c_int64 * 11)()
        assert (lib.favit_mhla_block_bwd_layout(ctypes.byref(d), want_lp, b1)
                == lib.favit_mhla_block_bwd_layout2(ctypes.byref(d), ctypes.byref(r), want_lp, b2))
        assert list(b1) == list(b2)
    plain, same = favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, training), favit.kernels.mhla_block_plan(B, n, D, H, W, hidden, training, n_mlp=n)
    assert same.rows is None and same.off == plain.off and same.boff == plain.boff


@pytest.mark.parametrize("n_mlp", [18, 0, -3])
def test_bad_mlp_rows_are_refused_before_any_launch(favit, n_mlp):
    lib, A = favit._abi.lib(), favit._abi
    d, r = _desc(favit, 3, 17, 128, 2, 7, 512, 1), _mlp(favit, n_mlp)
    assert lib.favit_mhla_block_tape_layout2(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_INVALID
    assert lib.favit_mhla_block_bwd_layout2(ctypes.byref(d), ctypes.byref(r), 1, None) == A.ERR_INVALID
    assert lib.favit_mhla_block_tape_layout2(ctypes.byref(d), None, None) == A.ERR_INVALID
    assert favit.kernels.mhla_block_plan(3, 17, 128, 2, 7, 512, True, n_mlp=n_mlp) is None
    # the chain calls check the rows (and the geometry) first, so these return on a machine without a GPU
    d.x = d.tape = d.g1 = d.b1 = d.g2 = d.b2 = d.weff = d.beff = d.wproj = d.bproj = d.wfc1 = d.bfc1 = d.wfc2 = d.bfc2 = 0x10000
    d.tape_bytes = 1 << 40
    r.x1c = 0x10000
    assert lib.favit_mhla_block_attn_fwd(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_INVALID
    assert lib.favit_mhla_block_mlp_fwd(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_INVALID
    assert lib.favit_mhla_block_mlp_bwd(ctypes.byref(d), ctypes.byref(r), 0x10000, 0x10000, 0x10000, 1 << 40, 1, None) == A.ERR_INVALID
    assert lib.favit_mhla_block_attn_bwd(ctypes.byref(d), ctypes.byref(r), 0x10000, 0x10000, 0x10000, 1 << 40, 1, None) == A.ERR_INVALID
    # valid rows: a misaligned or missing x1c and a short tape are refused just the same
    r.n_mlp, r.x1c = 11, 0x10004
    assert lib.favit_mhla_block_mlp_fwd(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_ALIGN
    r.x1c = None
    assert lib.favit_mhla_block_mlp_fwd(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_INVALID
    r.x1c = 0x10000
    d.tape_bytes = lib.favit_mhla_block_tape_layout2(ctypes.byref(d), ctypes.byref(r), None) - 1
    assert lib.favit_mhla_block_attn_fwd(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_INVALID
    assert lib.favit_mhla_block_mlp_fwd(ctypes.byref(d), ctypes.byref(r), None) == A.ERR_INVALID
