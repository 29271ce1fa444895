"""ctypes binding of libfavit.so, derived from the C ABI declared in include/favit.h.

The header is read at import (the library is not needed for that): every ``FAVIT_X`` constant becomes the module
attribute ``X`` (F32, BF16, ACT_GELU, ERR_INVALID, ADAMW_MAX_SEGMENTS, ...), every ``favit_*_t`` struct a
ctypes.Structure (STRUCTS; the five the package fills in also under the names of _STRUCT_NAMES) and every prototype
an entry of _SIGS.  A declaration the reader does not recognise is an error, never skipped.

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C focused-attention-vit_amd/csrc``.  There is NO fallback: if the library is
missing every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfavit.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "favit.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "float": C.c_float}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
_STRUCT_NAMES = {"favit_gemm_t": "GemmDesc", "favit_sdpa_t": "SdpaDesc", "favit_mhla_block_t": "BlockDesc",
                 "favit_mhla_block_mlp_t": "BlockMlp", "favit_adamw_multi_t": "AdamwMulti"}

_DECL = re.compile(r"\s*([^;{}]*(?:\{[^{}]*\}[^;{}]*)?);")           # one declaration, with at most one { } block
_TYPED = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(.*)", re.S)   # base type, stars, the rest


def _refuse(what, decl):
    raise ValueError(f"favit.h: {what} in `{' '.join(decl.split())}`")


def _ctype(base, stars, structs, decl):
    if not stars:
        if base not in _SCALARS:
            _refuse(f"unknown scalar type {base!r}", decl)
        return _SCALARS[base]
    return C.POINTER(structs[base]) if base in structs and stars.count("*") == 1 else C.c_void_p


def _struct(name, body, consts, structs, decl):
    fields = []
    for line in filter(None, (s.strip() for s in body.split(";"))):
        typed = _TYPED.fullmatch(line)
        for item in typed.group(3).split(",") if typed else [""]:
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", item)
            if not m:
                _refuse(f"field {line!r} not understood", decl)
            t = _ctype(typed.group(1), typed.group(2), structs, decl)
            if m.group(2) is not None:
                n = int(m.group(2)) if m.group(2).isdigit() else consts.get(m.group(2))
                if n is None:
                    _refuse(f"unknown array length {m.group(2)!r}", decl)
                t = t * n
            fields.append((m.group(1), t))
    return type(_STRUCT_NAMES.get(name, name), (C.Structure,),
                {"_fields_": fields, "__doc__": f"Mirror of {name} (include/favit.h)."})


def _prototype(ret, args, structs, decl):
    ret = re.sub(r"\s*\*", "*", ret)
    if ret not in _RETURNS:
        _refuse(f"unknown return type {ret!r}", decl)
    types = []
    for arg in ([] if args.strip() == "void" else args.split(",")):
        m = _TYPED.fullmatch(arg.strip())
        if not m or not re.fullmatch(r"\w*", m.group(3).strip()):
            _refuse(f"argument {arg.strip()!r} not understood", decl)
        types.append(_ctype(m.group(1), m.group(2), structs, decl))
    return types, _RETURNS[ret]


def parse_header(text):
    """(constants {FAVIT_X: int}, structs {favit_x_t: ctypes.Structure}, prototypes {favit_x: (argtypes, restype)})
    of the text of a header written like include/favit.h; ValueError names the first declaration that is not."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, structs, sigs = {}, {}, {}
    for line in re.findall(r"^[ \t]*#[^\n]*", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(FAVIT_\w+)(?:\s+(-?\d+))?\s*", line)
        if m and m.group(2) is not None:
            consts[m.group(1)] = int(m.group(2))
        elif not m and re.match(r"\s*#\s*define\b", line):
            _refuse("#define that is no integer constant", line)
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text)
    pos = 0
    while m := _DECL.match(text, pos):
        pos, decl = m.end(), m.group(1).strip()
        if e := re.fullmatch(r"enum\s*\{(.*)\}", decl, re.S):
            for item in filter(None, (s.strip() for s in e.group(1).split(","))):
                v = re.fullmatch(r"(FAVIT_\w+)\s*=\s*(-?\d+)", item)
                if not v:
                    _refuse(f"enumerator {item!r} without an integer value", decl)
                consts[v.group(1)] = int(v.group(2))
        elif s := re.fullmatch(r"typedef\s+struct\s+\w*\s*\{(.*)\}\s*(favit_\w+_t)", decl, re.S):
            structs[s.group(2)] = _struct(s.group(2), s.group(1), consts, structs, decl)
        elif p := re.fullmatch(r"(.*?)\b(favit_\w+)\s*\((.*)\)", decl, re.S):
            sigs[p.group(2)] = _prototype(p.group(1).strip(), p.group(3), structs, decl)
        else:
            _refuse("declaration not understood", decl)
    if text[pos:].strip() != "}" * wrapped:
        _refuse("declaration not understood", text[pos:][:200])
    return consts, structs, sigs


def _slot_names(prefix, count):
    """Lower-cased suffixes of the FAVIT_<prefix>* enumerators in value order, which must be 0 .. count - 1."""
    found = sorted((v, k[len(prefix):].lower()) for k, v in CONSTS.items() if k.startswith(prefix))
    if [v for v, _ in found] != list(range(count)):
        raise ValueError(f"favit.h: the {prefix}* enumerators are not 0..{count - 1}")
    return tuple(k for _, k in found)


with open(HEADER_PATH) as _f:
    CONSTS, STRUCTS, _SIGS = parse_header(_f.read())      # _SIGS: name -> (argtypes, restype), applied by lib()
globals().update({k[len("FAVIT_"):]: v for k, v in CONSTS.items()})
globals().update({_STRUCT_NAMES[k]: v for k, v in STRUCTS.items() if k in _STRUCT_NAMES})
POOL = {k[len("FAVIT_POOL_"):].lower(): v for k, v in CONSTS.items() if k.startswith("FAVIT_POOL_")}
# the slot NAMES of the two block layouts, in the order of their offsets (these replace the two counts of the header)
BLOCK_TAPE_SLOTS = _slot_names("FAVIT_TAPE_", CONSTS["FAVIT_BLOCK_TAPE_SLOTS"])
BLOCK_BWD_SLOTS = _slot_names("FAVIT_BWD_", CONSTS["FAVIT_BLOCK_BWD_SLOTS"])
# the slots of favit_eval_metrics' state; the last one, hits, is EVAL_MAX_TOPK words long
EVAL_SLOTS = _slot_names("FAVIT_EVAL_SLOT_", CONSTS["FAVIT_EVAL_STATE_WORDS"] - CONSTS["FAVIT_EVAL_MAX_TOPK"] + 1)

_lib = None


class FavitLibraryError(RuntimeError):
    pass


def declared_symbols():
    """Entry points declared in include/favit.h (used by the symbol-export test)."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(favit_[a-z0-9_]+)\s*\(", txt)))


def lib():
    """Load libfavit.so (once).  Raises FavitLibraryError if it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FavitLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C focused-attention-vit_amd/csrc`.  There is no CPU / PyTorch fallback.")
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise FavitLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (args, res) in _SIGS.items():
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        _lib = l
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = lib().favit_strerror(code).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")
