"""Runs the REFERENCE's own kernels (oracle/_ref/libref_rasterizer.so, built by oracle/ref_build.py) on a file of cases -- a helper of
the tests, not a test, and a stand-alone script: numpy and ctypes only, no torch.

    python tests/ref_kernels.py CASES_IN.npz OUT.npz

It is meant to run as a CHILD process of its own (tests/test_gpu_reference_kernels.py, tests/golden/make_golden.py refkernels), so that
a fault in foreign code cannot take the caller's GPU context with it.  For every case: forward, backward and markVisible; everything
oracle/ref_capi.cpp exports is written out.  The first HIP error ends the run with a non-zero exit status: nothing further is started.

Input file: `names` (array of case names) and per case `<name>/<field>`:
    means3D [P,3]  opacities [P,1]  bg [3]  viewmatrix [4,4]  projmatrix [4,4]  campos [3]  dL_dpix [3,H,W]
    either shs [P,M,3] or rgb [P,3];  either scales [P,3] + rotations [P,4] or cov3D [P,6]
    meta = [W, H, sh_degree, tanfovx, tanfovy, scale_modifier]  (float64)
Output file: per case `<name>/<array>` (see FORWARD_OUT / BACKWARD_OUT below) and `<name>/present`."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "oracle", "_ref", "libref_rasterizer.so")

FORWARD_OUT = ("out_color", "out_depth", "radii", "num_rendered", "depths", "means2D", "cov3D", "conic_opacity", "rgb", "clamped",
               "tiles_touched", "keys_sorted", "point_list", "ranges", "n_contrib", "accum_alpha")
BACKWARD_OUT = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
INPUT_FIELDS = ("means3D", "opacities", "bg", "viewmatrix", "projmatrix", "campos", "dL_dpix", "shs", "rgb", "scales", "rotations", "cov3D")


def pack_case(name, sc, cam, sh_degree, dL_dpix):
    """The input entries of one case: sc / cam as the tests build them (float32 scene arrays, camera dict with scale_modifier)."""
    d = {}
    for k in ("means3D", "opacities", "bg"):
        d[f"{name}/{k}"] = np.ascontiguousarray(sc[k], np.float32)
    pre_colour, pre_cov = "rgb" in sc, "cov3D" in sc
    for k in (("rgb",) if pre_colour else ("shs",)) + (("cov3D",) if pre_cov else ("scales", "rotations")):
        d[f"{name}/{k}"] = np.ascontiguousarray(sc[k], np.float32)
    for k in ("viewmatrix", "projmatrix", "campos"):
        d[f"{name}/{k}"] = np.ascontiguousarray(cam[k], np.float32)
    d[f"{name}/dL_dpix"] = np.ascontiguousarray(dL_dpix, np.float32)
    d[f"{name}/meta"] = np.array([cam["image_width"], cam["image_height"], sh_degree, cam["tanfovx"], cam["tanfovy"],
                                  cam.get("scale_modifier", 1.0)], np.float64)
    return d


def unpack(npz, names):
    """{case name: {array name: array}} of an output (or input) file."""
    out = {n: {} for n in names}
    for key in npz.files:
        n, _, field = key.partition("/")
        if n in out:
            out[n][field] = npz[key]
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HipError(RuntimeError):
    pass


def run_case(L, c):
    W, H, D = int(c["meta"][0]), int(c["meta"][1]), int(c["meta"][2])
    tanx, tany, smod = (C.c_float(float(v)) for v in c["meta"][3:6])
    g = lambda k: np.ascontiguousarray(c[k], np.float32) if k in c else None      # noqa: E731
    means3D, opac, bg, view, proj, campos = (g(k) for k in ("means3D", "opacities", "bg", "viewmatrix", "projmatrix", "campos"))
    shs, rgb_in, scales, rots, cov_in = g("shs"), g("rgb"), g("scales"), g("rotations"), g("cov3D")
    P = means3D.shape[0]
    M = 0 if shs is None else shs.shape[1]
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    cap = max(P * tiles, 1)                      # no Gaussian touches more tiles than there are
    o = dict(out_color=np.zeros((3, H, W), np.float32), out_depth=np.zeros((1, H, W), np.float32), radii=np.zeros(P, np.int32),
             num_rendered=np.zeros(1, np.int32), depths=np.zeros(P, np.float32), means2D=np.zeros((P, 2), np.float32),
             cov3D=np.zeros((P, 6), np.float32), conic_opacity=np.zeros((P, 4), np.float32), rgb=np.zeros((P, 3), np.float32),
             clamped=np.zeros((P, 3), np.uint8), tiles_touched=np.zeros(P, np.uint32), keys_sorted=np.zeros(cap, np.uint64),
             point_list=np.zeros(cap, np.uint32), ranges=np.zeros((tiles, 2), np.uint32), n_contrib=np.zeros((H, W), np.uint32),
             accum_alpha=np.zeros((H, W), np.float32))
    handle = C.c_void_p()
    rc = L.ref_forward(C.c_int(P), C.c_int(D), C.c_int(M), _p(bg), C.c_int(W), C.c_int(H), _p(means3D), _p(shs), _p(rgb_in), _p(opac),
                       _p(scales), smod, _p(rots), _p(cov_in), _p(view), _p(proj), _p(campos), tanx, tany,
                       _p(o["out_color"]), _p(o["out_depth"]), _p(o["radii"]), _p(o["num_rendered"]), _p(o["depths"]), _p(o["means2D"]),
                       _p(o["cov3D"]), _p(o["conic_opacity"]), _p(o["rgb"]), _p(o["clamped"]), _p(o["tiles_touched"]), C.c_int64(cap),
                       _p(o["keys_sorted"]), _p(o["point_list"]), _p(o["ranges"]), _p(o["n_contrib"]), _p(o["accum_alpha"]), C.byref(handle))
    if rc != 0:
        raise HipError(f"ref_forward returned {rc}")
    R = int(o["num_rendered"][0])
    o["keys_sorted"], o["point_list"] = o["keys_sorted"][:R].copy(), o["point_list"][:R].copy()
    b = dict(dL_dmeans2D=np.zeros((P, 3), np.float32), dL_dconic=np.zeros((P, 4), np.float32), dL_dopacity=np.zeros((P, 1), np.float32),
             dL_dcolors=np.zeros((P, 3), np.float32), dL_dmeans3D=np.zeros((P, 3), np.float32), dL_dcov3D=np.zeros((P, 6), np.float32),
             dL_dsh=np.zeros((P, M, 3), np.float32), dL_dscales=np.zeros((P, 3), np.float32), dL_drotations=np.zeros((P, 4), np.float32))
    try:
        rc = L.ref_backward(handle, C.c_int(P), C.c_int(D), C.c_int(M), _p(bg), C.c_int(W), C.c_int(H), _p(means3D), _p(shs), _p(rgb_in),
                            _p(scales), smod, _p(rots), _p(cov_in), _p(view), _p(proj), _p(campos), tanx, tany, _p(o["radii"]),
                            _p(g("dL_dpix")), *[_p(b[k]) for k in BACKWARD_OUT])
    finally:
        L.ref_free(handle)
    if rc != 0:
        raise HipError(f"ref_backward returned {rc}")
    present = np.zeros(P, np.uint8)
    rc = L.ref_mark_visible(C.c_int(P), _p(means3D), _p(view), _p(proj), _p(present))
    if rc != 0:
        raise HipError(f"ref_mark_visible returned {rc}")
    o.update(b)
    o["present"] = present
    return o


def load_library():
    L = C.CDLL(LIB_PATH)
    for f in (L.ref_forward, L.ref_backward, L.ref_mark_visible):
        f.restype = C.c_int
    L.ref_free.restype = None
    L.ref_free.argtypes = [C.c_void_p]
    return L


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    src = np.load(argv[1])
    names = [str(n) for n in src["names"]]
    L = load_library()
    out = {"names": np.array(names)}
    for n, c in unpack(src, names).items():
        try:
            res = run_case(L, c)
        except HipError as e:               # nothing more is started on the GPU after an error
            print(f"ref_kernels: case {n}: {e}", file=sys.stderr)
            return 1
        out.update({f"{n}/{k}": v for k, v in res.items()})
        print(f"ref_kernels: {n}: P={c['means3D'].shape[0]} rendered={int(res['num_rendered'][0])}", flush=True)
    np.savez(argv[2], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
