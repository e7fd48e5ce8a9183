"""What the stand-alone projection (fused_project.project_gaussians) costs beside a vectorised torch restatement of the same projection, timed
in the same process: device-synchronised medians at BASELINE's cfg3 (1 M Gaussians @ 1352 x 1014) and cfg5 (3 M @ 1080p) scenes, with
antialiasing (all five outputs).  Per size:
    fwd_fused / fwd_torch          project_gaussians under no_grad  against  the restatement (EWA projection, frustum clamp, dilation, conic,
                                   radius, tile rectangle, the renderer's culling, compensation) under no_grad
    fwdbwd_fused / fwdbwd_torch    the same with autograd: forward + backward to means3D, scales and rotations from an upstream gradient on
                                   each of the four float outputs
and the two kernels alone, from device events around the C calls (GB/s over the bytes a row needs: forward 40 B read + 32 B written,
backward 68 B read + 40 B written), beside the profile time of preprocess_fwd in renders of the same scene in this run.  With --other-lib
the kernels' events are also taken on a second build of the library (tools/build_variant.sh), alternating with the default one: how the
per-lane stores of the 12- and 24-byte rows ("lane") were chosen over an LDS-staged float4 run ("staged", profiles/project_overhead_stores.json).
The two claims, each recorded as it came out: (a) fwdbwd_fused < fwdbwd_torch at both sizes -- "holds" / "does not hold"; (b) no claim
against preprocess_fwd, only the number.  One JSON line on stdout and in --out (kept as profiles/project_overhead.json).

usage: python tools/project_overhead.py [--steps 20] [--warmup 3] [--configs cfg3,cfg5] [--out profiles/project_overhead.json]
                                        [--label lane] [--other-lib PATH --other-label NAME]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {"cfg3": (1_000_000, 1352, 1014), "cfg5": (3_000_000, 1920, 1080)}
FWD_BYTES, BWD_BYTES = 40 + 32, 68 + 40


def torch_project(m, s, q, V, Pm, W, H, tanx, tany):
    """The projection restated with torch ops, fp32, vectorised over the rows: (means2D, depths, conics, radii, compensation), culled rows
    zero.  The backward's conventions are autograd's own (the frustum clamp is differentiated as written)."""
    P = m.shape[0]
    ph = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
    hom, t = ph @ Pm, (ph @ V)[:, :3]
    pw = 1.0 / (hom[:, 3] + 1e-7)
    pix = torch.stack([((hom[:, 0] * pw + 1.0) * W - 1.0) * 0.5, ((hom[:, 1] * pw + 1.0) * H - 1.0) * 0.5], dim=1)
    r, x, y, z = q.unbind(dim=1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(P, 3, 3)
    M = R * s[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    tz = t[:, 2]
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    txc = torch.clamp(t[:, 0] / tz, -1.3 * tanx, 1.3 * tanx) * tz
    tyc = torch.clamp(t[:, 1] / tz, -1.3 * tany, 1.3 * tany) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], dim=1).reshape(P, 2, 3)
    A = J @ V[:3, :3].T
    cov = A @ Sigma @ A.transpose(1, 2)
    c00, c01, c11 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    a, b, c = c00 + 0.3, c01, c11 + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], dim=1)
    comp = torch.sqrt(torch.clamp((c00 * c11 - b * b) / det, min=0.000025))
    with torch.no_grad():
        mid = 0.5 * (a + c)
        radius = torch.ceil(3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))))
        gx, gy = (W + 15) // 16, (H + 15) // 16
        x0 = torch.clamp(torch.trunc((pix[:, 0] - radius) / 16.0), 0, gx); x1 = torch.clamp(torch.trunc((pix[:, 0] + radius + 15.0) / 16.0), 0, gx)
        y0 = torch.clamp(torch.trunc((pix[:, 1] - radius) / 16.0), 0, gy); y1 = torch.clamp(torch.trunc((pix[:, 1] + radius + 15.0) / 16.0), 0, gy)
        vis = (tz > 0.2) & (det != 0.0) & ((x1 - x0) * (y1 - y0) > 0)
    keep = lambda v: torch.where(vis.reshape((P,) + (1,) * (v.dim() - 1)), v, torch.zeros_like(v))  # noqa: E731
    return keep(pix), keep(tz), keep(conic), keep(radius).to(torch.int32), keep(comp)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="cfg3,cfg5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_overhead.json"))
    ap.add_argument("--label", default="lane")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--other-label", default="other")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_project as fp
    import scenes
    _C = rast._C
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)  # noqa: E731
    libs = {a.label: _C.lib()}
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        for fn in ("gsrast_project_forward", "gsrast_project_backward"):
            getattr(other, fn).restype, getattr(other, fn).argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        libs[a.other_label] = other
    kid = {_C.lib().gsrast_profile_kernel_name(k).decode(): k for k in range(_C.lib().gsrast_profile_kernel_count())}
    result = {"steps": a.steps, "warmup": a.warmup, "antialiasing": True, "stores_of_the_library": a.label,
              "bytes_per_row": {"project_fwd": FWD_BYTES, "project_bwd": BWD_BYTES}, "configs": {}}

    def timed(run):
        ms = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]

    for name in a.configs.split(","):
        P, W, H = CONFIGS[name]
        sc, cam = scenes.synth(P, 0), scenes.camera(0, 1, W, H)
        rs = rast.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(sc["bg"]), scale_modifier=1.0,
            viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]), sh_degree=sc["sh_degree"], campos=t(cam["campos"]), prefiltered=False)
        m, s, q = (t(sc[k]).requires_grad_(True) for k in ("means3D", "scales", "rotations"))
        V, Pm = rs.viewmatrix, rs.projmatrix
        ups = [torch.randn((P, 2), device=dev), torch.randn((P,), device=dev), torch.randn((P, 3), device=dev), torch.randn((P,), device=dev)]
        fused = lambda: fp.project_gaussians(m, s, q, raster_settings=rs, antialiasing=True)  # noqa: E731
        plain = lambda: torch_project(m, s, q, V, Pm, W, H, float(cam["tanfovx"]), float(cam["tanfovy"]))  # noqa: E731

        def fwdbwd(project):
            m.grad = s.grad = q.grad = None
            o = project()
            torch.autograd.backward([o[0], o[1], o[2], o[4]], ups)

        def no_grad(project):
            with torch.no_grad():
                project()

        res = {"P": P, "W": W, "H": H}
        with torch.no_grad():
            pf, pt = fused(), plain()
            res["visible_rows"] = int((pf.radii > 0).sum())
            res["radii_differ_from_torch"] = int((pf.radii != pt[3]).sum())
        for leg, run in (("fwd_fused", lambda: no_grad(fused)), ("fwd_torch", lambda: no_grad(plain)),
                         ("fwdbwd_fused", lambda: fwdbwd(fused)), ("fwdbwd_torch", lambda: fwdbwd(plain))):
            res[f"{leg}_ms"], res[f"{leg}_spread_ms"] = timed(run)
        for leg in ("fwd", "fwdbwd"):
            res[f"{leg}_fused_over_torch"] = round(res[f"{leg}_fused_ms"] / res[f"{leg}_torch_ms"], 4)
        res["a_fwdbwd_fused_below_torch"] = "holds" if res["fwdbwd_fused_ms"] < res["fwdbwd_torch_ms"] else "does not hold"
        # the kernels alone: events around the C calls, the builds alternating
        d = _C.ProjectStruct()
        d.P, d.width, d.height, d.tanfovx, d.tanfovy, d.scale_modifier = P, W, H, float(cam["tanfovx"]), float(cam["tanfovy"]), 1.0
        d.viewmatrix, d.projmatrix, d.flags = V.data_ptr(), Pm.data_ptr(), _C.PROJECT_ANTIALIAS
        d.means3D, d.scales, d.rotations = m.data_ptr(), s.data_ptr(), q.data_ptr()
        o = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
        outs = [o(P, 2), o(P), o(P, 3), torch.empty(P, dtype=torch.int32, device=dev), o(P)]
        d.means2D, d.depths, d.conics, d.radii, d.compensation = [x.data_ptr() for x in outs]
        d.dL_dmeans2D, d.dL_ddepths, d.dL_dconics, d.dL_dcompensation = [x.data_ptr() for x in ups]
        grads = [o(P, 3), o(P, 3), o(P, 4)]
        d.dL_dmeans3D, d.dL_dscales, d.dL_drotations = [x.data_ptr() for x in grads]
        stream = torch.cuda.current_stream(dev).cuda_stream
        events = {label: {"project_fwd": [], "project_bwd": []} for label in libs}
        for it in range(a.warmup + a.steps):
            for label, lib in libs.items():
                for kernel, fn in (("project_fwd", lib.gsrast_project_forward), ("project_bwd", lib.gsrast_project_backward)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = fn(C.addressof(d), stream)
                    e1.record()
                    torch.cuda.synchronize()
                    assert rc == 0, (label, kernel, rc)
                    if it >= a.warmup:
                        events[label][kernel].append(e0.elapsed_time(e1))
        res["kernels_ms"] = {label: {k: round(statistics.median(v), 4) for k, v in ks.items()} for label, ks in events.items()}
        res["kernels_GBps"] = {label: {"project_fwd": round(P * FWD_BYTES / (ks["project_fwd"] * 1e-3) / 1e9, 1),
                                       "project_bwd": round(P * BWD_BYTES / (ks["project_bwd"] * 1e-3) / 1e9, 1)} for label, ks in res["kernels_ms"].items()}
        # (b) the render's own per-Gaussian forward kernel on the same scene, from the library's profile table
        opac, shs = t(sc["opacities"]), t(sc["shs"])
        ras = rast.GaussianRasterizer(rs)
        m2 = torch.zeros((P, 3), device=dev)
        render = lambda: ras(means3D=m.detach(), means2D=m2, opacities=opac, shs=shs, scales=s.detach(), rotations=q.detach(), antialiasing=True)  # noqa: E731
        with torch.no_grad():
            for _ in range(a.warmup):
                render()
            torch.cuda.synchronize()
            _C.profile_reset()
            _C.set_option("profile", 1 << kid["preprocess_fwd"])
            for _ in range(max(3, a.steps // 3)):
                render()
            torch.cuda.synchronize()
            pk = _C.profile_read()
            _C.set_option("profile", 0)
        res["b_preprocess_fwd_ms_per_launch"] = round(pk["preprocess_fwd"][0] / max(pk["preprocess_fwd"][1], 1), 4)
        result["configs"][name] = res
        del m, s, q, ups, outs, grads, opac, shs, ras, m2, pf, pt
        torch.cuda.empty_cache()
    result["a_fwdbwd_fused_below_torch_at_both_sizes"] = ("holds" if all(r["a_fwdbwd_fused_below_torch"] == "holds" for r in result["configs"].values())
                                                         else "does not hold")
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
