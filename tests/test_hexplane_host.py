"""Hexplane lookup, host side (no GPU): every refusal of hex_check and of the entry points of gsrast_hexplane_* (GSRAST_E_ARG with its
text, before any device call), and what gsrast_hexplane_scratch_bytes -- which is not given the row width F -- accepts and refuses.

The reference ships 32 channels x multires [1, 2, 4, 8], concatenated (arguments/__init__.py:83-89, scene/hexplane.py:168): 24 planes,
F = 128, out_offset 0 / 32 / 64 / 96.  scratch_bytes used to judge those offsets against a row of 64 floats and returned 0 for three
and four scales: test_scratch_bytes_accepts_the_shipped_field is the regression test of that."""
import itertools

import pytest

PLANES = list(itertools.combinations(range(4), 2))
E_ARG = -1
ONE = 256      # any non-NULL, 16-byte aligned value: never dereferenced on the host


def _arr(rast, planes):
    a = (rast._C.PlaneStruct * max(len(planes), 1))()
    for i, p in enumerate(planes):
        d = dict(tex=ONE, grad_tex=ONE, W=8, H=8, cu=0, cv=1, max_mip_level=7, out_offset=0)
        d.update(p)
        a[i] = rast._C.PlaneStruct(d["tex"], d["grad_tex"], d["W"], d["H"], d["cu"], d["cv"], d["max_mip_level"], d["out_offset"])
    return a


def _field(reso, mults, C_):
    """The descriptors fused_hexplane.interpolate_ms_features builds for concatenated scales."""
    out = []
    for s, m in enumerate(mults):
        for (a, b) in PLANES:
            out.append(dict(W=reso[a] * m if a < 3 else reso[a], H=reso[b] * m if b < 3 else reso[b], cu=a, cv=b,
                            max_mip_level=7 if 3 not in (a, b) else 0, out_offset=s * C_))
    return out


class Calls:
    def __init__(self, rast):
        self.L = rast._C.lib()
        self.rast = rast

    def err(self):
        return self.L.gsrast_last_error().decode()

    def scratch(self, planes, C_=4, N=10, n=None):
        return self.L.gsrast_hexplane_scratch_bytes(len(planes) if n is None else n, _arr(self.rast, planes), C_, N)

    def fwd(self, planes, C_=4, N=10, D=4, F=None, n=None, pts=ONE, levels=ONE, features=ONE, scratch=ONE):
        return self.L.gsrast_hexplane_forward(N, D, C_, C_ if F is None else F, len(planes) if n is None else n, _arr(self.rast, planes),
                                              pts, levels, features, scratch, None)

    def bwd(self, planes, C_=4, N=10, D=4, F=None, n=None, pts=ONE, levels=ONE, dy=ONE, d_pts=ONE, d_levels=ONE, mips_built=1, scratch=ONE):
        return self.L.gsrast_hexplane_backward(N, D, C_, C_ if F is None else F, len(planes) if n is None else n, _arr(self.rast, planes),
                                               pts, levels, dy, d_pts, d_levels, mips_built, scratch, None)


@pytest.fixture
def calls(rast):
    return Calls(rast)


# (what is wrong, keyword arguments of the call, planes, the text, does the error need the row width F or the row length D to be seen?)
BAD = [
    ("0 planes", dict(n=0), [{}], "1..24 planes", False),
    ("25 planes", dict(), [{}] * 25, "1..24 planes", False),
    ("C = 2", dict(C_=2), [{}], "power of two in [4, 64]", False),
    ("C = 12", dict(C_=12), [{}], "power of two in [4, 64]", False),
    ("C = 128", dict(C_=128), [{}], "power of two in [4, 64]", False),
    ("D = 1", dict(D=1), [{}], "2..8 coordinates per point", True),
    ("D = 9", dict(D=9), [{}], "2..8 coordinates per point", True),
    ("F < C", dict(C_=8, F=4), [{}], "feature rows a multiple of 4 floats", True),
    ("F = 10", dict(C_=8, F=10), [{}], "feature rows a multiple of 4 floats", True),
    ("W = 0", dict(), [dict(W=0)], "bad plane extent", False),
    ("H = 0", dict(), [dict(H=0)], "bad plane extent", False),
    ("W < 0", dict(), [dict(W=-8)], "bad plane extent", False),
    ("2^26 + 2^13 texels", dict(), [dict(W=8192, H=8193, max_mip_level=0)], "bad plane extent", False),
    ("cu = -1", dict(), [dict(cu=-1)], "coordinate column outside the point row", False),
    ("cv = 8", dict(D=8), [dict(cv=8)], "coordinate column outside the point row", False),
    ("cv = 4 of D = 4", dict(), [dict(cv=4)], "coordinate column outside the point row", True),
    ("second plane's column", dict(), [{}, dict(cu=2, cv=9)], "coordinate column outside the point row", False),
    ("max_mip_level = -1", dict(), [dict(max_mip_level=-1)], "negative max_mip_level", False),
    ("offset 2", dict(F=8), [dict(out_offset=2)], "feature block outside the row", False),
    ("offset -4", dict(F=8), [dict(out_offset=-4)], "feature block outside the row", False),
    ("offset past the row", dict(F=8), [dict(out_offset=8)], "feature block outside the row", True),
    ("block over the row's end", dict(C_=8, F=12), [dict(out_offset=8)], "feature block outside the row", True),
    ("12 x 10 at limit 7", dict(), [dict(W=12, H=10)], "odd extent", False),
    ("8 x 6 at limit 2", dict(), [dict(W=8, H=6, max_mip_level=2)], "odd extent", False),
    ("16 levels", dict(), [dict(W=1 << 16, H=1 << 10, max_mip_level=16)], "too many mip levels", False),
    # planes sharing a feature block must be adjacent; blocks are equal or disjoint
    ("offsets 0, 32, 0", dict(C_=32, F=64), [dict(out_offset=0), dict(out_offset=32), dict(out_offset=0)], "must be adjacent", False),
    ("offsets 0, 0, 8, 0", dict(C_=8, F=16), [dict(out_offset=o) for o in (0, 0, 8, 0)], "must be adjacent", False),
    ("blocks 0..8 and 4..12", dict(C_=8, F=16), [dict(out_offset=0), dict(out_offset=4)], "equal or disjoint", False),
    ("blocks 8..24 and 0..16", dict(C_=16, F=32), [dict(out_offset=8), dict(out_offset=0)], "equal or disjoint", False),
]


@pytest.mark.parametrize("what,kw,planes,text,needs_row", BAD, ids=[b[0] for b in BAD])
def test_descriptor_refusals(calls, what, kw, planes, text, needs_row):
    """forward and backward refuse with GSRAST_E_ARG and the text; scratch_bytes, which is told neither F nor D, returns 0 (with the same
    text) exactly for the errors that can be seen without them."""
    assert calls.fwd(planes, **kw) == E_ARG and "hexplane" in calls.err() and text in calls.err(), calls.err()
    assert calls.bwd(planes, **kw) == E_ARG and text in calls.err(), calls.err()
    skw = {k: v for k, v in kw.items() if k in ("C_", "n")}
    calls.L.gsrast_hexplane_forward(-1, 4, 4, 4, 1, _arr(calls.rast, [{}]), ONE, ONE, ONE, ONE, None)      # another text in between
    nbytes = calls.scratch(planes, **skw)
    if needs_row:
        assert nbytes > 0
    else:
        assert nbytes == 0 and text in calls.err(), calls.err()


def test_pointer_and_size_refusals(calls):
    ok = [dict(W=16, H=16), dict(W=16, H=4, cu=1, cv=3, max_mip_level=0)]
    assert calls.scratch(ok) > 0
    assert calls.fwd(ok, N=-1) == E_ARG and "hexplane_forward: bad size" in calls.err()
    assert calls.bwd(ok, N=-1) == E_ARG and "hexplane_backward: bad size" in calls.err()
    assert calls.scratch(ok, N=-1) == 0 and "hexplane_scratch_bytes: bad size" in calls.err()
    assert calls.L.gsrast_hexplane_scratch_bytes(1, None, 4, 10) == 0 and "1..24 planes" in calls.err()
    assert calls.L.gsrast_hexplane_forward(10, 4, 4, 4, 1, None, ONE, ONE, ONE, ONE, None) == E_ARG and "1..24 planes" in calls.err()
    for i in (0, 1):
        bad = [dict(p) for p in ok]
        bad[i]["tex"] = None
        assert calls.fwd(bad) == E_ARG and "hexplane_forward: NULL plane" in calls.err()
        assert calls.bwd(bad) == E_ARG and "hexplane_backward: NULL plane or gradient" in calls.err()
        bad = [dict(p) for p in ok]
        bad[i]["grad_tex"] = None
        assert calls.bwd(bad) == E_ARG and "hexplane_backward: NULL plane or gradient" in calls.err()
        assert calls.fwd(bad, pts=None) == E_ARG and "NULL pointer" in calls.err()        # the forward does not look at grad_tex
        assert calls.scratch(bad) > 0                                                       # and scratch_bytes at no pointer
    for p in ("pts", "levels", "features", "scratch"):
        assert calls.fwd(ok, **{p: None}) == E_ARG and "hexplane_forward: NULL pointer" in calls.err(), p
    for p in ("pts", "levels", "dy", "scratch"):
        assert calls.bwd(ok, **{p: None}) == E_ARG and "hexplane_backward: NULL pointer" in calls.err(), p
    # N = 0 needs no tensor, but still its scratch
    assert calls.fwd(ok, N=0, pts=None, levels=None, features=None, scratch=None) == E_ARG and "NULL pointer" in calls.err()
    assert calls.bwd(ok, N=0, pts=None, levels=None, dy=None, scratch=None) == E_ARG and "NULL pointer" in calls.err()


@pytest.mark.parametrize("C_", [32, 4])
def test_scratch_bytes_accepts_the_shipped_field(calls, C_):
    """24 planes, multires (1, 2, 4, 8), F = 4 C: offsets 0, C, 2C, 3C.  (Refused for 3 and 4 scales before: 0 bytes.)"""
    sizes = {}
    for n_scales in (1, 2, 3, 4):
        planes = _field([64, 64, 64, 25], (1, 2, 4, 8)[:n_scales], C_)
        assert len(planes) == 6 * n_scales and planes[-1]["out_offset"] == (n_scales - 1) * C_
        got = [calls.scratch(planes, C_=C_, N=N) for N in (0, 1, 255, 256, 257, 1000, 100000)]
        assert all(g > 0 for g in got), (n_scales, got)
        assert all(a <= b for a, b in zip(got, got[1:])), (n_scales, got)
        sizes[n_scales] = got[5]
    assert sizes[1] < sizes[2] < sizes[3] < sizes[4]
    if C_ == 32:
        assert (sizes[1], sizes[2]) == (1341696, 5825792)       # what the call has always returned for one and two scales at N = 1000
    # the row width is for forward / backward to judge: the same descriptors in a row of 64 floats are refused there
    planes = _field([64, 64, 64, 25], (1, 2, 4, 8), C_)
    assert calls.fwd(planes, C_=C_, F=2 * C_) == E_ARG and "feature block outside the row" in calls.err()
    assert calls.bwd(planes, C_=C_, F=4 * C_ - 4) == E_ARG and "feature block outside the row" in calls.err()


def test_accepted_layouts_pass_the_descriptor_check(calls):
    """What must NOT be refused by the new adjacency rule: the layouts interpolate_ms_features builds (seen through scratch_bytes > 0,
    and through forward reaching its pointer check)."""
    layouts = {
        "concatenated": [0] * 6 + [8] * 6,
        "summed": [0] * 12,
        "concat_planes": [0, 0, 0, 8, 8, 8, 16, 16, 16, 24, 24, 24],
        "descending": [24] * 3 + [8] * 3 + [16] * 3 + [0] * 3,
        "gap": [0, 0, 24],
    }
    for name, offs in layouts.items():
        planes = [dict(out_offset=o) for o in offs]
        assert calls.scratch(planes, C_=8) > 0, name
        assert calls.fwd(planes, C_=8, F=32, pts=None) == E_ARG and "hexplane_forward: NULL pointer" in calls.err(), name


def test_python_refusals_need_no_device(rast):
    import torch
    import fused_hexplane
    g = torch.zeros((1, 4, 8, 8))
    uv = torch.rand((5, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        fused_hexplane.texture_planes(uv, uv, [g], [(0, 1)], [0], [0], 4)
    with pytest.raises(NotImplementedError):
        fused_hexplane.interpolate_ms_features(uv, [[g] * 6], 3, True, uv, None)
    with pytest.raises(NotImplementedError):
        fused_hexplane.grid_sample_wrapper(g, torch.rand((5, 3)), uv, True)
