"""include/gsrast.h read as data: every prototype and every struct it declares, and which ctypes type may stand for a C type.
The one parser of the header the tests share (tests/test_capi_abi.py compares the binding's signature table and structs against it)."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")

# the header's struct -> the class of diff_gaussian_rasterization_ch3._C that declares it
STRUCTS = {"gsrast_options": "OptionsStruct", "gsrast_raw_inputs": "RawInputsStruct", "gsrast_raw_grads": "RawGradsStruct",
           "gsrast_forward_call": "ForwardCallStruct", "gsrast_backward_call": "BackwardCallStruct", "gsrast_adam_group": "AdamGroupStruct",
           "gsrast_densify_group": "DensifyGroupStruct", "gsrast_mlp3": "Mlp3Struct", "gsrast_bilagrid": "BilagridStruct",
           "gsrast_plane": "PlaneStruct", "gsrast_prealloc": "PreallocStruct"}
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "long long": C.c_longlong, "void": None}


def text():
    """The header without its comments (they cite the reference's C++ types and name functions in prose)."""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _norm(ctype):
    return re.sub(r"\s*\*\s*", "*", re.sub(r"\s+", " ", ctype.strip()))


def _declarator(piece):
    """('const float*', 'means3D') of 'const float* means3D'."""
    ctype, name = re.fullmatch(r"(.*[\s*])(\w+)", piece.strip(), flags=re.S).groups()
    return _norm(ctype), name


def prototypes():
    """{name: (return C type, [parameter C types])} of every function the header declares, parameters in order."""
    out = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+(?:\s*\*)?)\s+(gsrast_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text(), flags=re.M):
        assert name not in out, name
        out[name] = (_norm(ret), [] if params.strip() == "void" else [_declarator(p)[0] for p in params.split(",")])
    return out


def structs():
    """{name: [(field, C type)]} of every `typedef struct ... { ... } name;`, fields in order (`int P, D, M;` is three of them)."""
    out = {}
    for body, name in re.findall(r"typedef struct(?:\s+\w+)?\s*\{(.*?)\}\s*(\w+)\s*;", text(), flags=re.S):
        fields = out[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            ctype, field = _declarator(first)
            fields.append((field, ctype))
            for piece in more:          # `const float *src, *src_m`: the base type with each declarator's own stars
                stars, field = re.fullmatch(r"\s*(\**)\s*(\w+)\s*", piece).groups()
                fields.append((field, ctype.rstrip("*") + stars))
    return out


def _unconst(ctype):
    return re.sub(r"\bconst\b ?", "", ctype).strip()


def allowed(ctype, binding):
    """The ctypes types (compared by identity) that may stand for the C type `ctype` in `binding` (the _C module); the first is the one
    a struct's field has.  KeyError: a scalar the mapping does not know -- extend SCALARS knowingly."""
    if not ctype.endswith("*"):
        t = _unconst(ctype)
        return [binding._ALLOC_FN] if t == "gsrast_alloc_fn" else [SCALARS[t]]
    if ctype == "const char*":
        return [C.c_char_p, C.c_void_p]             # the only place c_char_p is allowed
    pointee = _unconst(ctype[:-1])
    if pointee == "gsrast_context":                 # an opaque handle
        return [C.c_void_p]
    if pointee in STRUCTS:
        return [C.POINTER(getattr(binding, STRUCTS[pointee]))]
    if pointee.endswith("*"):
        return [C.c_void_p, C.POINTER(C.c_void_p)]
    inner = SCALARS.get(pointee)
    return [C.c_void_p] if inner is None else [C.c_void_p, C.POINTER(inner)]
