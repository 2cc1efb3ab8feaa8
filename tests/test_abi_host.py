"""The ctypes binding (iqlpref_amd/_lib.py: SYMBOLS and the Structure classes) against include/iqlhip.h, parsed
as text (tests/helpers.parse_c_header).  They are two hand-kept copies of one ABI: a wrong width or a wrong field
order makes the library read or write the wrong memory with status 0.  No GPU, no library load."""
import ctypes as C
import os

import pytest

from iqlpref_amd import _lib
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16,
           "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t}
STRUCTS = {"iqlhip_replay_view": _lib.ReplayView, "iqlhip_trainer_config": _lib.TrainerConfig,
           "iqlhip_arenas": _lib.Arenas, "iqlhip_mlp_desc": _lib.MlpDesc, "iqlhip_pt_weights": _lib.PtWeights,
           "iqlhip_pt_block": _lib.PtBlock, "iqlhip_pt_model": _lib.PtModel, "iqlhip_bb_sim": _lib.BbSim}


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "iqlhip.h")) as f:
        h = helpers.parse_c_header(f.read())
    # (a parser that silently skipped declarations would let everything below pass)
    assert len(h["functions"]) >= 60 and len(h["structs"]) >= 8, (len(h["functions"]), len(h["structs"]))
    return h


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def pointee_problem(bound, want, levels, array):
    """Why ``bound`` does not bind ``levels`` of ``*`` (or, levels = 0, an array of ``array`` elements, which a
    parameter passes as a pointer) to the header's base type ``want``; None when it does.  void* binds anything."""
    if not is_pointer(bound):
        return f"{bound} is no pointer type"
    if want == "char" and levels == 1:
        return None if bound is C.c_char_p else f"{bound} for char *"
    if not (isinstance(bound, type) and issubclass(bound, C._Pointer)):
        return None  # c_void_p
    to = bound._type_
    if levels >= 2:
        return pointee_problem(to, want, levels - 1, None)
    if array is not None:
        if not (issubclass(to, C.Array) and to._type_ is SCALARS.get(want) and to._length_ == array):
            return f"POINTER({to}) for {want}[{array}]"
        return None
    known = SCALARS.get(want) or STRUCTS.get(want)
    if known is None:  # an opaque handle, void
        return None if to is C.c_void_p or want == "void" else f"POINTER({to}) for {want} *"
    return None if to is known else f"POINTER({to}) for {want} *"


def value_problem(bound, t):
    """Why the ctypes type ``bound`` does not pass a value of the header's type ``t`` (a CType); None when it does."""
    if t.ptr == 0 and t.array is None:
        want = SCALARS.get(t.base)
        assert want is not None, f"scalar {t.base} unknown to the test"
        return None if bound is want else f"{bound} for {t.base}"
    return pointee_problem(bound, t.base, t.ptr, t.array)


def test_functions_match_the_header(header):
    funcs = header["functions"]
    assert set(funcs) == set(_lib.SYMBOLS), set(funcs) ^ set(_lib.SYMBOLS)
    bad = []
    for name, (ret, params) in sorted(funcs.items()):
        res, args = _lib.SYMBOLS[name]
        if len(args) != len(params):
            bad.append(f"{name}: {len(args)} bound arguments, {len(params)} declared")
            continue
        if (why := value_problem(res, ret)):
            bad.append(f"{name}: returns {why}")
        for i, ((pname, t), bound) in enumerate(zip(params, args)):
            if (why := value_problem(bound, t)):
                bad.append(f"{name}: argument {i} ({pname}): {why}")
    assert not bad, "\n".join(bad)


def test_structs_match_the_header(header):
    structs = header["structs"]
    assert set(structs) == set(STRUCTS), set(structs) ^ set(STRUCTS)
    bound_classes = {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert bound_classes == set(STRUCTS.values()), bound_classes ^ set(STRUCTS.values())
    bad = []
    for name, fields in structs.items():
        have = STRUCTS[name]._fields_
        if [f for f, _ in fields] != [f[0] for f in have]:
            bad.append(f"{name}: fields {[f[0] for f in have]}, the header has {[f for f, _ in fields]}")
            continue
        for (fname, t), (_, bound) in zip(fields, have):
            if t.array is None:
                why = value_problem(bound, t)
            elif not (issubclass(bound, C.Array) and bound._length_ == t.array):  # an array lies in the struct
                why = f"{bound} for {t}"
            elif t.ptr == 0:
                why = None if bound._type_ is SCALARS[t.base] else f"{bound} for {t}"
            else:
                why = pointee_problem(bound._type_, t.base, t.ptr, None)
            if why:
                bad.append(f"{name}.{fname}: {why}")
    assert not bad, "\n".join(bad)


def test_constants_match_the_header(header):
    m, e = header["macros"], header["enums"]
    assert e["IQLHIP_OK"] == 0
    pairs = (("PREC_FP32", "IQLHIP_PREC_FP32"), ("PREC_BF16", "IQLHIP_PREC_BF16"),
             ("MAX_CRITICS", "IQLHIP_MAX_CRITICS"), ("MAX_HIDDEN", "IQLHIP_MAX_HIDDEN"),
             ("N_TENSORS", "IQLHIP_N_TENSORS"), ("MAX_GROUP", "IQLHIP_MAX_GROUP"),
             ("MLP_MAX_LAYERS", "IQLHIP_MLP_MAX_LAYERS"), ("MLP_SET_MAX", "IQLHIP_MLP_SET_MAX"),
             ("CHOICE_MEAN", "IQLHIP_CHOICE_MEAN"), ("CHOICE_MEDIAN", "IQLHIP_CHOICE_MEDIAN"))
    assert set(m) == {c for _, c in pairs}  # every integer macro of the header is compared
    for py, c in pairs:
        assert getattr(_lib, py) == m[c], (py, c)
    for py in ("ERR_INVALID", "ERR_HIP", "ERR_UNSUPPORTED", "ERR_NOMEM"):
        assert getattr(_lib, py) == e["IQLHIP_" + py], py
