"""The ctypes binding against the header it is read from (CPU only): focused-attention-vit_amd/_abi.py derives every
constant, struct mirror and signature from include/favit.h.  Checked here: every struct layout against the C compiler's,
that the reader refuses what it does not understand, that no prototype is lost, the signatures against a table frozen
from the last hand-written binding, and the header's limits against the library's own answers."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# (name, arity, positions of the float arguments, positions of the 8-byte integer arguments) of every entry point, as
# the hand-written table of ABI 8 had them.  A new entry point adds a row; an existing row changes only with the ABI.
FROZEN = [
    ('favit_abi_version', 0, [], []),
    ('favit_strerror', 1, [], []),
    ('favit_set_dropout_epoch', 1, [], []),
    ('favit_set_health_word', 1, [], []),
    ('favit_gemm', 2, [], []),
    ('favit_gemm_last_kernel', 0, [], []),
    ('favit_ln_gemm', 10, [5], [2]),
    ('favit_gemm_grouped_tn', 3, [], []),
    ('favit_gemm_grouped_tn_workspace', 2, [], []),
    ('favit_gemm_grouped_tn_ws', 5, [], [3]),
    ('favit_gemm_grouped_tn_ragged', 3, [], []),
    ('favit_gemm_grouped_tn_ragged_workspace', 2, [], []),
    ('favit_gemm_grouped_tn_ragged_ws', 5, [], [3]),
    ('favit_gemm_grouped_last_splits', 0, [], []),
    ('favit_gemm_grouped_plan', 5, [], []),
    ('favit_cast', 6, [], [4]),
    ('favit_fp8_amax', 7, [], [2, 3, 4]),
    ('favit_fp8_quantize', 16, [], [2, 3, 4, 6, 8]),
    ('favit_layernorm_fwd', 12, [10], [1, 8]),
    ('favit_layernorm_bwd', 23, [20], [3, 9, 18, 21]),
    ('favit_layernorm_fwd_q8', 17, [9], [1, 7]),
    ('favit_layernorm_bwd_q8', 27, [18], [2, 8, 16, 19]),
    ('favit_small_linear_fwd', 9, [], [1]),
    ('favit_small_linear_bwd', 12, [], [2]),
    ('favit_reduce_rows', 7, [], [1, 3]),
    ('favit_reduce_rows_multi', 7, [], [4]),
    ('favit_reduce_rows_multi_ragged', 7, [], []),
    ('favit_mhla_fold_fwd', 11, [], []),
    ('favit_mhla_fold_fwd_multi', 11, [], []),
    ('favit_mhla_fold_bwd', 13, [], []),
    ('favit_mhla_fold_bwd_multi', 13, [], []),
    ('favit_mhla_attn_fwd', 12, [9], [10]),
    ('favit_mhla_attn_bwd', 13, [10], [11]),
    ('favit_mhla_attn_lse_supported', 4, [], []),
    ('favit_mhla_attn_fwd_lse', 13, [10], [11]),
    ('favit_mhla_attn_bwd_lse', 15, [12], [13]),
    ('favit_sdpa_fwd', 2, [], []),
    ('favit_sdpa_bwd', 2, [], []),
    ('favit_softmax_fwd', 14, [11], [5, 6, 8, 12]),
    ('favit_softmax_bwd', 11, [8], [5, 9]),
    ('favit_patchify_fwd', 8, [], []),
    ('favit_patchify_bwd', 7, [], []),
    ('favit_embed_prologue_fwd', 8, [], []),
    ('favit_embed_prologue_bwd', 9, [], []),
    ('favit_rows_cut_fwd', 8, [], []),
    ('favit_rows_cut_bwd', 10, [], []),
    ('favit_mhla_block_tape_layout', 2, [], []),
    ('favit_mhla_block_bwd_layout', 3, [], []),
    ('favit_mhla_block_fwd', 2, [], []),
    ('favit_mhla_block_bwd', 7, [], [4]),
    ('favit_mhla_block_tape_layout2', 3, [], []),
    ('favit_mhla_block_bwd_layout2', 4, [], []),
    ('favit_mhla_block_attn_fwd', 3, [], []),
    ('favit_mhla_block_mlp_fwd', 3, [], []),
    ('favit_mhla_block_mlp_bwd', 8, [], [5]),
    ('favit_mhla_block_attn_bwd', 8, [], [5]),
    ('favit_dropout', 7, [4], [3, 5]),
    ('favit_drop_path_add', 10, [7], [8]),
    ('favit_drop_path_bwd', 11, [6, 8], [7, 9]),
    ('favit_sppp_map_patches', 10, [], []),
    ('favit_sppp_pool_fwd', 11, [], []),
    ('favit_sppp_pool_bwd', 13, [], []),
    ('favit_sppp_centroids', 6, [], []),
    ('favit_sppp_posenc_fwd', 8, [], []),
    ('favit_image_transform', 14, [], []),
    ('favit_image_transform_ragged', 13, [], []),
    ('favit_slic_features_workspace', 3, [], []),
    ('favit_slic_features', 9, [5], []),
    ('favit_slic_cluster_workspace', 2, [], []),
    ('favit_slic_cluster', 12, [], [8]),
    ('favit_slic_connect', 10, [], []),
    ('favit_cross_entropy', 8, [6], []),
    ('favit_adamw', 15, [6, 7, 8, 9, 10, 11, 12, 13], [5]),
    ('favit_cross_entropy_ls', 9, [6, 7], []),
    ('favit_grad_norm_workspace', 0, [], []),
    ('favit_grad_norm', 10, [3, 4], [8]),
    ('favit_adamw_clip', 17, [6, 7, 8, 9, 10, 11, 12, 13], [5]),
    ('favit_adamw_ema', 17, [7, 8, 9, 10, 11, 12, 13, 14, 15], [6]),
    ('favit_adamw_clip_ema', 19, [7, 8, 9, 10, 11, 12, 13, 14, 17], [6]),
    ('favit_swap_params', 5, [], [3]),
    ('favit_adamw_multi', 2, [], []),
    ('favit_adamw_multi_max_segments', 0, [], []),
    ('favit_adamw_multi_align', 0, [], []),
    ('favit_batch_mix', 8, [], []),
    ('favit_cross_entropy_mix', 10, [7, 8], []),
    ('favit_randaugment_max_ops', 0, [], []),
    ('favit_randaugment', 16, [], [9]),
    ('favit_random_erase', 10, [], [4]),
    ('favit_cross_entropy_distill', 15, [9, 10, 11, 12], []),
]

# the entry points that do not return an int status
NOT_INT = dict.fromkeys(("favit_strerror", "favit_gemm_last_kernel"), ctypes.c_char_p)
NOT_INT.update(dict.fromkeys((
    "favit_gemm_grouped_tn_workspace", "favit_gemm_grouped_tn_ragged_workspace", "favit_mhla_block_tape_layout",
    "favit_mhla_block_bwd_layout", "favit_mhla_block_tape_layout2", "favit_mhla_block_bwd_layout2",
    "favit_slic_features_workspace", "favit_slic_cluster_workspace", "favit_grad_norm_workspace"), ctypes.c_int64))


def test_struct_layouts_match_the_compiler(favit):
    """sizeof and every offsetof / field size of every struct of the header, from a C probe generated from the parsed
    field names, against the ctypes classes."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = favit._abi.STRUCTS
    assert set(favit._abi._STRUCT_NAMES) <= set(structs) and len(structs) >= 5
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "favit.h"\nint main(){'
    for name, cls in structs.items():
        src += f'printf("%zu\\n", sizeof({name}));'
        for f, _ in cls._fields_:
            src += f'printf("%zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));'
    src += "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = iter(subprocess.check_output([os.path.join(d, "t")], text=True).splitlines())
    for name, cls in structs.items():
        assert int(next(out)) == ctypes.sizeof(cls), name
        for f, _ in cls._fields_:
            off, size = map(int, next(out).split())
            assert (getattr(cls, f).offset, getattr(cls, f).size) == (off, size), (name, f)
    A = favit._abi
    assert [ctypes.sizeof(c) for c in (A.GemmDesc, A.SdpaDesc, A.BlockDesc, A.BlockMlp, A.AdamwMulti)] == [
        256, 336, 152, 16, 1128]


@pytest.mark.parametrize("text,named", [
    ("int favit_scale(double factor, void* stream);", "favit_scale"),                 # unknown scalar type
    ("typedef struct favit_tab { int64_t end[FAVIT_NONE]; } favit_tab_t;", "favit_tab_t"),   # unknown array length
    ("int favit_visit(void (*fn)(int, int), void* stream);", "favit_visit"),          # a list that does not split
    ("int favit_a(void) int favit_b(void);", "favit_a"),                              # two prototypes run together
    ("enum { FAVIT_FIRST, FAVIT_SECOND };", "FAVIT_FIRST"),                           # enumerator without a value
    ("double favit_ratio(void);", "favit_ratio"),                                     # unknown return type
    ("struct favit_bare { int x; };", "favit_bare"),                                  # not the header's typedef form
    ("#define FAVIT_MASK (1 << 3)\n", "FAVIT_MASK"),                                  # no integer literal
])
def test_reader_refuses_what_it_does_not_understand(favit, text, named):
    with pytest.raises(ValueError, match=named):
        favit._abi.parse_header("#define FAVIT_LIMIT 4\n" + text)


def test_reader_takes_the_forms_the_header_uses(favit):
    consts, structs, sigs = favit._abi.parse_header(
        '#ifndef H_\n#define FAVIT_N 2 /* two */\nextern "C" {\nenum { FAVIT_A = 0, FAVIT_B = -3 };\n'
        "typedef struct favit_s { const float* p; void* q; int64_t a, b[3], c[FAVIT_N]; uint64_t u; } favit_s_t;\n"
        "const char* favit_name(void);\n"
        "int64_t favit_f(const favit_s_t* s, const float* const* in, void* const* out, int n, int32_t m,\n"
        "                float x /* a comment, with a comma */, uint64_t seed, int64_t* offsets /* [2] or NULL */);\n"
        "}\n#endif\n")
    assert consts == {"FAVIT_N": 2, "FAVIT_A": 0, "FAVIT_B": -3}
    S = structs["favit_s_t"]
    assert [(f, t) for f, t in S._fields_] == [
        ("p", ctypes.c_void_p), ("q", ctypes.c_void_p), ("a", ctypes.c_int64), ("b", ctypes.c_int64 * 3),
        ("c", ctypes.c_int64 * 2), ("u", ctypes.c_uint64)]
    assert sigs == {
        "favit_name": ([], ctypes.c_char_p),
        "favit_f": ([ctypes.POINTER(S), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_float,
                     ctypes.c_uint64, ctypes.c_void_p], ctypes.c_int64)}


def test_every_prototype_is_parsed_and_frozen(favit):
    A = favit._abi
    with open(A.HEADER_PATH) as fh:
        consts, _, sigs = A.parse_header(fh.read())
    assert sorted(sigs) == A.declared_symbols() == sorted(A._SIGS)
    assert consts == A.CONSTS and consts["FAVIT_ABI_VERSION"] == 8
    frozen = {row[0]: row[1:] for row in FROZEN}
    assert len(frozen) == len(FROZEN) == 89 and set(frozen) <= set(sigs)
    for name, (arity, floats, wide) in frozen.items():
        args, res = A._SIGS[name]
        assert len(args) == arity, name
        assert [i for i, t in enumerate(args) if t is ctypes.c_float] == floats, name
        assert [i for i, t in enumerate(args) if t in (ctypes.c_int64, ctypes.c_uint64)] == wide, name
        for i, t in enumerate(args):      # everything else is a 4-byte integer or a pointer
            assert i in floats + wide or t in (ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p) \
                or issubclass(t, ctypes._Pointer), (name, i, t)
        assert res is NOT_INT.get(name, ctypes.c_int), name


def test_names_the_package_imports_come_from_the_header(favit):
    A = favit._abi
    assert (A.F32, A.BF16, A.FP8, A.F32X3, A.E4M3, A.E5M2) == (0, 1, 2, 3, 0, 1)
    assert (A.ACT_NONE, A.ACT_GELU, A.ACT_DGELU, A.ACT_GELU_SAVEGRAD, A.ACT_MULAUX) == (0, 1, 2, 3, 4)
    assert (A.ERR_INVALID, A.ERR_UNSUPPORTED, A.ERR_ALIGN, A.ERR_LAUNCH) == (-1, -2, -3, -4)
    assert A.POOL == {"mean": 0, "max": 1, "attention": 2}
    assert A.BLOCK_TAPE_SLOTS == ("xn1", "mu1", "rs1", "qkv", "o", "lse", "x1", "xn2", "mu2", "rs2", "h", "pre", "x2")
    assert A.BLOCK_BWD_SLOTS == ("dpre", "dxn2", "g1_f32", "g1_lp", "do", "dqkv", "dxn1", "g_out_f32", "g_out_lp",
                                 "part1", "part2")
    K, R = favit.kernels, favit.data.RandAugment
    assert (K.GROUP_MAX, K.GRAD_NORM_MAX_BUFS, K.SMALL_LINEAR_MAX_N, K.Fp8History.NSLOT) == (48, 16, 64, 256)
    assert (K.ADAMW_MAX_SEGMENTS, K.ADAMW_SEG_ALIGN) == (64, 256)
    assert (A.REDUCE_ROWS_MULTI_MAX, A.FOLD_MAX, A.FOLD_BWD_MAX) == (32, 32, 16)
    assert R.MAX_OPS == 8
    assert (R.K_IDENTITY, R.K_AFFINE, R.K_BLEND, R.K_MASK, R.K_SOLARIZE, R.K_AUTOCONTRAST,
            R.K_EQUALIZE) == tuple(range(7))


def test_header_limits_equal_the_library(favit):
    A, lib = favit._abi, favit._abi.lib()
    assert lib.favit_abi_version() == A.ABI_VERSION
    assert lib.favit_adamw_multi_max_segments() == A.ADAMW_MAX_SEGMENTS
    assert lib.favit_adamw_multi_align() == A.ADAMW_SEG_ALIGN
    assert lib.favit_randaugment_max_ops() == A.RANDAUGMENT_MAX_OPS
