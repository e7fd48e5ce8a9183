"""What anti-aliased rendering costs: device-synchronised forward + backward of one training-shaped step (SH colours, scales / rotations,
a loss on the colour), the plain call against antialiasing=True, at BASELINE's cfg3 (1 M Gaussians @ 1352 x 1014) and cfg5 (3 M @ 1080p)
shapes -- and the per-Gaussian kernels' own time (option "profile": preprocess_fwd, preprocess_bwd) and the two blend kernels', which the
filter reaches through o_eff < o (pixels saturate later: more pairs).  The two variants alternate step by step on the same pose, so drift
and the list cut's state affect both alike.  One JSON object on stdout.

usage: python tools/aa_overhead.py [--steps 30] [--warmup 5] [--configs cfg3,cfg5]"""
import argparse
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
KERNELS = ("preprocess_fwd", "preprocess_bwd", "blend_fwd", "blend_bwd")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="cfg3,cfg5")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import scenes
    _C = rast._C
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)  # noqa: E731
    kid = {_C.lib().gsrast_profile_kernel_name(k).decode(): k for k in range(_C.lib().gsrast_profile_kernel_count())}
    result = {"steps": a.steps, "warmup": a.warmup, "configs": {}}
    for name in a.configs.split(","):
        P, W, H = CONFIGS[name]
        sc = scenes.synth(P, 0)
        cam = scenes.camera(0, 1, W, H)
        rs = rast.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(sc["bg"]), scale_modifier=1.0,
            viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]), sh_degree=sc["sh_degree"], campos=t(cam["campos"]),
            prefiltered=False)
        leaves = {k: t(sc[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        gC = t(scenes.upstream_grad(H, W, 1))
        ras = rast.GaussianRasterizer(rs)

        def step(aa: bool) -> float:
            for v in list(leaves.values()) + [m2]:
                v.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ras(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                      scales=leaves["scales"], rotations=leaves["rotations"], antialiasing=aa)
            (out[0] * gC).sum().backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(a.warmup):
            step(False); step(True)
        plain, aa = [], []
        for _ in range(a.steps):
            plain.append(step(False)); aa.append(step(True))
        mp, ma = statistics.median(plain), statistics.median(aa)
        # the kernels' own time: a few profiled steps of each variant (events around the launches: kept out of the timings above)
        kern = {}
        mask = sum(1 << kid[k] for k in KERNELS)
        for variant in (False, True):
            torch.cuda.synchronize()
            _C.profile_reset()
            _C.set_option("profile", mask)
            for _ in range(max(3, a.steps // 3)):
                step(variant)
            pk = _C.profile_read()
            _C.set_option("profile", 0)
            kern["aa" if variant else "plain"] = {k: round(pk[k][0] / max(pk[k][1], 1), 4) for k in KERNELS}
        result["configs"][name] = {"P": P, "W": W, "H": H, "plain_ms": round(mp, 4), "aa_ms": round(ma, 4), "ratio": round(ma / mp, 4),
                                   "plain_spread_ms": [round(min(plain), 4), round(max(plain), 4)],
                                   "aa_spread_ms": [round(min(aa), 4), round(max(aa), 4)],
                                   "kernel_ms_per_launch": kern, "last_late": _C.context_query("last_late")}
        del leaves, m2, ras
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
