"""The host side of the ragged grouped weight-gradient launch (csrc/gemm.hip: grouped_plan_ragged), without a GPU:
favit_gemm_grouped_plan describes the plan a launch would get.  Over random ragged groups

* every (chunk, split) unit sits in exactly one XCD queue, at most 24 per queue and 255 in all;
* the k-ranges of a chunk tile [0, K_c) without overlap, in steps of 32 tokens, and none is empty;
* the workspace query equals what the plan uses: the slabs of the chunks that are split, nothing for the others;
* a group with one token count gets the plan of the uniform entry point."""
import ctypes as C
import random

import pytest

SHAPES = {384: [(384, 1536), (1536, 384), (384, 384), (1152, 384)], 128: [(384, 128), (128, 128), (512, 128), (128, 512)]}


def _descs(favit, blocks):
    """blocks: [(T, D)] -> the four (N, K) problems of every block."""
    arr = (favit._abi.GemmDesc * (4 * len(blocks)))()
    i = 0
    for T, D in blocks:
        for N, Kd in SHAPES[D]:
            d = arr[i]
            d.A = d.B = d.C = 0x10000
            d.M, d.N, d.K = N, Kd, T
            d.lda, d.ldb, d.ldc = N, Kd, Kd
            d.batch = d.batch_inner = 1
            d.in_dtype, d.out_dtype = favit._abi.BF16, favit._abi.F32
            d.alpha = 1.0
            i += 1
    return arr


def _plan(favit, arr, ragged=1):
    out = (C.c_int64 * 1024)()
    n = favit._abi.lib().favit_gemm_grouped_plan(arr, len(arr), ragged, out, 1024)
    assert n > 0, n
    v = list(out[:n])
    nchunks, nunits, max_tiles, ws = v[:4]
    chunks = [tuple(v[4 + 5 * c:9 + 5 * c]) for c in range(nchunks)]       # (first, tiles, K, splits, tokens per split)
    o, queues = 4 + 5 * nchunks, []
    for _ in range(8):
        queues.append(v[o + 1:o + 1 + v[o]])
        o += 1 + v[o]
    assert o == n
    return nunits, max_tiles, ws, chunks, queues


def _check(favit, arr, blocks):
    nunits, max_tiles, ws, chunks, queues = _plan(favit, arr)
    assert nunits == sum(c[3] for c in chunks) <= 255
    seen = sorted(u for q in queues for u in q)
    assert seen == list(range(nunits)), "every unit in exactly one queue"
    assert all(len(q) <= 24 for q in queues)
    first, tiles_of = 0, {}
    for (p0, tiles, Kc, s, kps) in chunks:
        assert Kc % 32 == 0 and kps % 32 == 0 and kps > 0
        assert (s - 1) * kps < Kc <= s * kps, "the splits tile [0, K) and the last one is not empty"
        for sp in range(s):
            tiles_of[first + sp] = tiles
        first += s
    assert max_tiles == max(sum(tiles_of[u] for u in q) for q in queues)
    need = 0
    for (p0, tiles, Kc, s, kps), nxt in zip(chunks, [c[0] for c in chunks[1:]] + [len(arr)]):
        assert len({arr[i].K for i in range(p0, nxt)}) == 1, "a chunk's problems share K"
        floats = sum(arr[i].M * arr[i].N + (arr[i].M + 3) // 4 * 4 for i in range(p0, nxt))
        if s > 1:
            need += s * ((floats + 63) // 64 * 64) * 4
    assert ws == need == int(favit._abi.lib().favit_gemm_grouped_tn_ragged_workspace(arr, len(arr)))
    return chunks, queues


def test_random_ragged_groups(favit):
    rng = random.Random(8)
    for _ in range(200):
        D = rng.choice([128, 384])
        blocks = [(32 * rng.randint(1, rng.choice([8, 60, 700])), D) for _ in range(rng.randint(1, 12))]
        _check(favit, _descs(favit, blocks), blocks)


def test_pruned_cfg2_launches(favit):
    """The launches of the pruned cfg2 step -- the whole encoder in one launch (the default) and
    the lists a 384 MB hold limit makes: the short blocks are one direct-writing unit each, the 71-row block is cut into
    several units, and no split is longer than 6,400 tokens."""
    chunks, queues = _check(favit, _descs(favit, [(256 * r, 384) for r in range(5, 72, 6)]), None)
    splits = {c[2] // 256: c[3] for c in chunks}
    assert splits[5] == splits[11] == splits[17] == 1 and splits[71] > 1, splits
    assert all(c[4] <= 6400 for c in chunks) and all(2 <= len(q) <= 4 for q in queues), (chunks, queues)
    rows = [5, 11, 17, 23, 29, 35]
    chunks, queues = _check(favit, _descs(favit, [(256 * r, 384) for r in rows]), None)
    splits = {c[2] // 256: c[3] for c in chunks}
    assert splits[5] == splits[11] == splits[17] == 1, splits
    assert splits[35] > 1, splits
    for group in ([41, 47], [53, 59], [65], [71]):
        chunks, _ = _check(favit, _descs(favit, [(256 * r, 384) for r in group]), None)
        assert all(c[3] > 1 and c[4] <= 6400 for c in chunks), chunks


@pytest.mark.parametrize("T,D,nblocks", [(256 * 197, 384, 4), (128 * 17, 384, 12), (2048, 128, 3)])
def test_uniform_group_gets_the_uniform_plan(favit, T, D, nblocks):
    arr = _descs(favit, [(T, D)] * nblocks)
    assert _plan(favit, arr, 1) == _plan(favit, arr, 0)
    lib = favit._abi.lib()
    assert int(lib.favit_gemm_grouped_tn_ragged_workspace(arr, len(arr))) == int(lib.favit_gemm_grouped_tn_workspace(arr, len(arr)))


def test_plan_refusals(favit):
    abi = favit._abi
    out = (C.c_int64 * 1024)()
    arr = _descs(favit, [(160, 128), (176, 128)])                       # 176 % 32 != 0
    assert abi.lib().favit_gemm_grouped_plan(arr, len(arr), 1, out, 1024) == abi.ERR_UNSUPPORTED
    assert int(abi.lib().favit_gemm_grouped_tn_ragged_workspace(arr, 49)) == 0
    arr = _descs(favit, [(160, 128), (352, 128)])
    assert abi.lib().favit_gemm_grouped_plan(arr, len(arr), 0, out, 1024) == abi.ERR_UNSUPPORTED, "the uniform plan takes one K"
