"""CPU: the C-ABI shared library loads without a GPU, exports every symbol include/gsrast.h declares,
and rejects bad arguments before touching a device (no compute calls here)."""
import ctypes as C
import re

import pytest

import capi_header as hdr
import capi_records as cr

HEADER = hdr.HEADER


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_header_and_library_agree(rast, L):
    names = sorted(hdr.prototypes())      # (each of them exported and in EXPORTS: the next test)
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert re.search(r"#define GSRAST_ABI_VERSION 6\b", open(HEADER).read())
    render = [n for n in names if re.fullmatch(r"gsrast_(render_)?(forward|backward)\w*", n)]
    assert render == ["gsrast_backward", "gsrast_forward", "gsrast_render_backward", "gsrast_render_forward"]      # four render entry points, no more


def test_every_prototype_matches_its_row_of_the_signature_table(rast, L):
    """include/gsrast.h against _C.SIGNATURES, the one table lib() binds from: the same names, and for each the header's number of
    arguments, with every argument and the return type of the C type's width and kind (capi_header.allowed; ctypes types compared by
    identity).  A c_int where the header says long long, a c_float for a double or a defaulted restype for a size_t fails here."""
    _C = rast._C
    protos = hdr.prototypes()
    assert set(protos) == set(_C.SIGNATURES) and len(protos) >= 78
    raw = C.CDLL(_C.LIB_PATH)
    for name, (ret, params) in protos.items():
        restype, argtypes = _C.SIGNATURES[name]
        assert hasattr(raw, name), f"{name} is not exported"
        assert any(restype is t for t in hdr.allowed(ret, _C)) and (restype is not C.c_char_p or ret == "const char*"), (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert any(bound is t for t in hdr.allowed(ctype, _C)), (name, k, ctype, bound)
        fn = getattr(L, name)       # ... and lib() has bound exactly the row
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert _C.EXPORTS == tuple(_C.SIGNATURES)


def test_every_struct_matches_the_header(rast):
    """Every struct the binding declares against its `typedef struct` in include/gsrast.h: the same field names, in the same order, each of
    the one ctypes type a field of that C type has (capi_header.allowed's first: a typed pointer to a struct, c_void_p for any other)."""
    _C = rast._C
    declared = hdr.structs()
    assert set(declared) == set(hdr.STRUCTS)      # (gsrast_context is opaque: no body, no class)
    for struct, cls in hdr.STRUCTS.items():
        want, have = declared[struct], getattr(_C, cls)._fields_
        assert [n for n, _ in want] == [n for n, _ in have], struct
        for (name, ctype), (_, bound) in zip(want, have):
            assert bound is hdr.allowed(ctype, _C)[0] and bound is not C.c_char_p, (struct, name, ctype, bound)


def test_call_records_match_the_header(rast, L):
    """The two call records (include/gsrast.h: how the records grow) as the binding declares them: the same fields, in the same order, of
    the same C types; the prefixes a caller of an earlier header passes end where the header says; the flag bits and families have the
    header's values.  Every render feature is a field and a bit here -- the header declares no symbol for any of them."""
    _C = rast._C
    src = open(HEADER).read()
    for struct in ("gsrast_forward_call", "gsrast_backward_call"):      # (every field's name, order and type: test_every_struct_matches_the_header)
        assert hdr.structs()[struct][:3] == [("struct_size", "size_t"), ("flags", "unsigned"), ("family", "int")]
    B = _C.BackwardCallStruct
    names = [n for n, _ in B._fields_]
    # MIN: everything up to the aux gradients; then the absgrad sink; then the two pose fields, which end the record
    assert re.search(r"#define GSRAST_BACKWARD_CALL_MIN offsetof\(gsrast_backward_call, dL_dmean2D_abs\)", src)
    assert re.search(r"#define GSRAST_BACKWARD_CALL_ABS offsetof\(gsrast_backward_call, dL_dcamera\)", src)
    assert re.search(r"#define GSRAST_FORWARD_CALL_MIN  sizeof\(gsrast_forward_call\)", src)
    assert names[-5:] == ["dL_dacc_depth", "dL_dalpha", "dL_dmean2D_abs", "dL_dcamera", "pose_scratch"]
    assert cr.SIZES == dict(min=B.dL_dmean2D_abs.offset, abs=B.dL_dcamera.offset, full=C.sizeof(B))
    assert cr.SIZES["min"] + 8 == cr.SIZES["abs"] and cr.SIZES["abs"] + 16 == cr.SIZES["full"]
    assert [n for n, _ in _C.ForwardCallStruct._fields_][-2:] == ["out_acc_depth", "out_alpha"]
    for name, value in (("RENDER_AUX", 1), ("RENDER_ANTIALIAS", 2), ("RENDER_ABSGRAD", 4), ("RENDER_POSEGRAD", 8)):
        assert re.search(r"#define\s+GSRAST_" + name + r"\s+" + hex(value) + r"u\b", src) and getattr(_C, name) == value
    for name, value in (("FAMILY_DENSE", 0), ("FAMILY_RAW", 1)):
        assert re.search(r"#define\s+GSRAST_" + name + r"\s+" + str(value) + r"\b", src) and getattr(_C, name) == value
    for fn, args in ((L.gsrast_render_forward, [C.c_void_p, C.POINTER(_C.OptionsStruct), C.POINTER(_C.ForwardCallStruct)]),
                     (L.gsrast_render_backward, [C.POINTER(_C.OptionsStruct), C.POINTER(B)])):
        assert fn.argtypes == args and fn.restype is C.c_int


def test_call_records_are_refused_by_size_family_and_unknown_bits(L, rast):
    """The refusals of the record itself, all before any device work (every pointer in these records is 16)."""
    _C = rast._C
    AUX, AA, ABS, POSE = _C.RENDER_AUX, _C.RENDER_ANTIALIAS, _C.RENDER_ABSGRAD, _C.RENDER_POSEGRAD
    # a NULL record
    assert L.gsrast_render_forward(None, None, None) == -1 and b"call record: NULL" in L.gsrast_last_error()
    assert L.gsrast_render_backward(None, None) == -1 and b"call record: NULL" in L.gsrast_last_error()
    # struct_size 0, MIN - 1, sizeof + 8 (the record behind it is never read past what this library knows)
    F = C.sizeof(_C.ForwardCallStruct)
    for size in (0, F - 1, F + 8):
        rc, err = cr.call(cr.forward(size=size))
        assert rc == -1 and b"struct_size" in err, size
    for size in (0, cr.SIZES["min"] - 1, cr.SIZES["full"] + 8):
        for family in ("dense", "raw"):
            rc, err = cr.call(cr.backward(family=family, size=size))
            assert rc == -1 and b"struct_size" in err, size
    # every size in between is a record (here: refused for its P, not for its size)
    for size in ("min", cr.SIZES["min"] + 4, "abs", "full"):
        rc, err = cr.call(cr.backward(-1, size=size))
        assert rc == -1 and b"bad sizes" in err, size
    # an unknown family; a dense record with `raw` set, a raw record with a dense input set
    for make in (cr.forward, cr.backward):
        rec = make()
        rec.family = 2
        rc, err = cr.call(rec)
        assert rc == -1 and b"unknown family" in err
        rc, err = cr.call(make(raw=cr.RAW_INPUTS))
        assert rc == -1 and b"call record: dense family with raw" in err
        rc, err = cr.call(make(family="raw", means3D=cr.ONE))
        assert rc == -1 and b"raw family with a dense input" in err
    rc, err = cr.call(cr.backward(raw_grads=cr.RAW_GRADS))
    assert rc == -1 and b"call record: dense family with raw" in err
    rc, err = cr.call(cr.backward(family="raw", dL_dmean3D=cr.ONE))
    assert rc == -1 and b"raw family with a dense input" in err
    rc, err = cr.call(cr.forward(family="raw", prefiltered=1))
    assert rc == -1 and b"prefiltered" in err
    # a flag bit whose fields lie beyond struct_size is an unknown bit; P = -1 on each of those records is refused for its size, not its flags
    for family in ("dense", "raw"):
        for size, flags in (("min", ABS), ("min", POSE), ("min", ABS | AA), ("abs", POSE), ("abs", POSE | AUX), ("full", 0x10), ("full", POSE | 0x10)):
            rc, err = cr.call(cr.backward(10, flags, family, size=size))
            assert rc == -1 and b"unknown bits" in err, (family, size, flags)
            rc, err = cr.call(cr.backward(-1, 0, family, size=size))
            assert rc == -1 and b"bad sizes" in err and b"ABSGRAD" not in err and b"POSEGRAD" not in err and b"unknown bits" not in err
    for flags in (ABS, POSE, 0x10):
        for family in ("dense", "raw"):
            rc, err = cr.call(cr.forward(10, flags, family))
            assert rc == -1 and b"unknown bits" in err


def test_no_torch_or_cxx_types_in_the_boundary():
    text = open(HEADER).read()
    assert 'extern "C"' in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)          # comments cite the reference's C++ types
    for banned in ("torch", "at::", "std::", "Tensor", "#include <vector>", "#include <functional>"):
        assert banned not in text


def test_state_buffer_sizes(L):
    g = [L.gsrast_geometry_bytes(p) for p in (0, 1, 1000, 100000, 3000000)]
    assert all(b >= a for a, b in zip(g, g[1:])) and g[0] > 0 and g[2] > g[1]
    assert g[-1] / 3000000 < 345          # ~145 B per Gaussian of forward state + the backward's 64-byte gradient record and 36 B of
                                          # colour / view-direction derivatives + the bucket depth sort's slabs (32-64 B per Gaussian)
                                          # + the list cut's compact early set (2 x 4 B per bucket slot: 22 B per Gaussian at 3 M) and flag byte
    b = [L.gsrast_binning_bytes(r, 1920, 1080) for r in (0, 10, 10**6, 5 * 10**7)]
    assert all(y >= x for x, y in zip(b, b[1:])) and b[2] > b[1]
    assert b[-1] / (5 * 10**7) < 20       # 16 B per instance + histograms
    i = L.gsrast_image_bytes(1920, 1080)
    assert 8 * 1920 * 1080 <= i <= 12 * 1920 * 1080     # 8 B per pixel + per-tile arrays (ranges, work-bucket lists; round 5: the predicted cut's
                                                         # opacity-mass table, 8 copies x 16 depth bins x 4 B per tile = 2 B per pixel)
    assert all(x % 256 == 0 for x in g + b + [i])


def test_options_round_trip(L, rast):
    for mode in (0, 1, 2, 0):
        rast._C.set_option("exp_mode", mode)
        assert rast._C.get_option("exp_mode") == mode
    with pytest.raises(ValueError):
        rast._C.set_option("exp_mode", 7)
    with pytest.raises(ValueError):
        rast._C.set_option("no_such_option", 1)
    n = L.gsrast_profile_kernel_count()
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(n)]
    assert "blend_fwd" in names and "blend_bwd" in names and "preprocess_fwd" in names


def test_bad_arguments_fail_before_any_device_work(L, rast):
    ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
    cb = ALLOC(lambda ctx, n: None)
    # negative P / zero-size image / SH degree out of range / NULL allocators
    base = dict(P=10, D=3, M=16, W=64, H=64)
    for bad in (dict(P=-1), dict(W=0), dict(D=4)):
        a = dict(base, **bad)
        rc = L.gsrast_forward(cb, None, cb, None, cb, None, a["P"], a["D"], a["M"], None, a["W"], a["H"], None, None,
                              None, None, None, 1.0, None, None, None, None, None, 0.5, 0.5, 0, None, None, None, None)
        assert rc == -1 and L.gsrast_last_error()
    rc = L.gsrast_backward(-3, 3, 16, 0, None, 64, 64, None, None, None, None, 1.0, None, None, None, None, None, 0.5, 0.5,
                           None, None, None, None, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == -1
    assert L.gsrast_mark_visible(-1, None, None, None, None, None) == -1


def test_widened_rows_reject_bad_arguments_without_a_device(rast, L):
    """hexplane lookup / Linear weight gradient: argument checks run before any HIP call (no GPU here)."""
    PS = rast._C.PlaneStruct
    ok = (PS * 1)(PS(None, None, 64, 64, 0, 1, 7, 0))
    n = L.gsrast_hexplane_scratch_bytes(1, ok, 32, 1000)
    assert n > 2 * 1365 * 32 * 4                               # value + gradient stacks of levels >= 1 (1365 texels), + the sorted pairs
    assert L.gsrast_hexplane_scratch_bytes(1, ok, 32, 2000) > n
    odd = (PS * 1)(PS(None, None, 12, 10, 0, 1, 7, 0))         # 6 x 5 cannot be halved
    assert L.gsrast_hexplane_scratch_bytes(1, odd, 32, 1000) == 0
    assert L.gsrast_hexplane_scratch_bytes(1, ok, 12, 1000) == 0   # channels: power of two in [4, 64]
    assert L.gsrast_hexplane_scratch_bytes(0, ok, 32, 1000) == 0
    assert L.gsrast_hexplane_forward(10, 4, 32, 32, 1, odd, None, None, None, None, None) == -1
    assert b"odd extent" in L.gsrast_last_error()
    far = (PS * 1)(PS(None, None, 64, 64, 0, 5, 7, 0))         # coordinate column outside a 4-float point row
    assert L.gsrast_hexplane_forward(10, 4, 32, 32, 1, far, None, None, None, None, None) == -1
    off = (PS * 1)(PS(None, None, 64, 64, 0, 1, 7, 16))        # feature block [16, 48) outside a 32-float row
    assert L.gsrast_hexplane_backward(10, 4, 32, 32, 1, off, None, None, None, None, None, 0, None, None) == -1


def test_raw_entry_points_reject_bad_arguments_before_any_device_work(L, rast):
    """GSRAST_FAMILY_RAW records: the pointer sets are validated on the host (no GPU needed for the refusals)."""
    _C = rast._C
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    assert opts.forward_only == 0 and opts.tile_clip == 1
    rc, err = cr.call(cr.forward(family="raw", raw={}), opts)
    assert rc < 0 and b"raw" in err
    rc, err = cr.call(cr.forward(family="raw", M=9), opts)
    assert rc < 0 and b"M must be" in err
    rc, err = cr.call(cr.forward(family="raw", raw=dict(cr.RAW_INPUTS, features_rest=20)), opts)
    assert rc < 0 and b"aligned" in err
    rc, err = cr.call(cr.backward(family="raw", raw_grads={}), opts)
    assert rc < 0 and b"NULL required gradient" in err
    rc, err = cr.call(cr.backward(family="raw", raw_grads=dict(dL_dmean2D=16, d_xyz=16, d_rotation=16, d_scaling=16, d_opacity_logit=16, d_shs_res=16)), opts)
    assert rc < 0 and b"d_shs_res" in err


def test_prealloc_callback_hands_out_what_fits_and_nothing_else():
    """gsrast_alloc_prealloc (include/gsrast.h, round 6): the library's own allocation callback over memory the caller already holds --
    pure host code, callable without a GPU.  Returns the pointer when the request fits, NULL otherwise, and records the request."""
    import ctypes as C
    from diff_gaussian_rasterization_ch3 import _C
    L = _C.lib()
    p = _C.PreallocStruct()
    p.ptr, p.capacity = 0x1000, 4096
    assert L.gsrast_alloc_prealloc(C.addressof(p), 4096) == 0x1000 and p.requested == 4096
    assert L.gsrast_alloc_prealloc(C.addressof(p), 100) == 0x1000 and p.requested == 100
    assert L.gsrast_alloc_prealloc(C.addressof(p), 4097) is None and p.requested == 4097
    assert L.gsrast_alloc_prealloc(None, 16) is None
    assert _C._PREALLOC_CB is not None
    # the sizes a caller pre-allocates are the ones the forward will ask for: monotone, 256-byte aligned arrays inside
    gb, ib = _C._state_bytes(1000, 640, 480)
    assert gb == L.gsrast_geometry_bytes(1000) and ib == L.gsrast_image_bytes(640, 480) and gb > 0 and ib > 0


def test_launch_makes_the_device_current_once_passes_the_stream_last_and_raises_by_name(rast, monkeypatch):
    """_C.launch over a stand-in library: the device scope is entered exactly once around the call, the stream handle of that device is the
    last argument, zero returns normally and a non-zero code raises the RuntimeError of _err -- the symbol's name, the code and
    gsrast_last_error's text.  _C.scratch_bytes: the size, or that error for the 0 of a refusal.  No device is touched."""
    import torch
    _C = rast._C
    log = []

    class Lib:
        code = 0

        def gsrast_last_error(self):
            return b"the reason"

        def __getattr__(self, name):
            return lambda *args: log.append((name, args)) or self.code

    class Scope:
        def __init__(self, dev):
            log.append(("scope", dev))

        def __enter__(self):
            log.append("enter")

        def __exit__(self, *exc):
            log.append("exit")
            return False

    fake, dev = Lib(), torch.device("cuda", 1)
    monkeypatch.setattr(_C, "lib", lambda: fake)
    monkeypatch.setattr(_C, "_on_device", Scope)
    monkeypatch.setattr(_C, "_stream_of", lambda d: log.append(("stream", d)) or 0xABC0)
    assert _C.launch("gsrast_some_kernel", dev, 7, None, 2.5) is None
    assert log == [("scope", dev), "enter", ("stream", dev), ("gsrast_some_kernel", (7, None, 2.5, 0xABC0)), "exit"]
    del log[:]
    fake.code = -3
    with pytest.raises(RuntimeError) as e:
        _C.launch("gsrast_some_kernel", dev, 7)
    assert str(e.value) == "gsrast_some_kernel failed (-3): the reason"
    assert log == [("scope", dev), "enter", ("stream", dev), ("gsrast_some_kernel", (7, 0xABC0)), "exit"]
    fake.code = 4096
    assert _C.scratch_bytes("gsrast_some_scratch_bytes", 1, 2) == 4096 and log[-1] == ("gsrast_some_scratch_bytes", (1, 2))
    fake.code = 0
    with pytest.raises(RuntimeError, match=r"gsrast_some_scratch_bytes failed \(-1\): the reason"):
        _C.scratch_bytes("gsrast_some_scratch_bytes", 1, 2)
