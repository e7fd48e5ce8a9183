"""What rendering the depth-distortion map (distortion=True) costs: device-synchronised forward and forward + backward, at BASELINE's cfg3
(1 M Gaussians @ 1352 x 1014) and cfg5 (3 M @ 1080p) shapes, for three variants that alternate call by call on the same pose (drift and the
list cut's state affect all alike):
    plain        the colour render alone
    distortion   the same call with distortion=True (the L1 form: sum_ij w_i w_j |z_i - z_j|)
    moments      what the interface could compose before: features=[1, z, z^2] with z the view-space depth computed in torch, and the L2
                 cousin A M2 - M1^2 = sum_{i<j} w_i w_j (z_i - z_j)^2 formed from the three maps -- another quantity, at the price of fp32
                 cancellation, shown for its cost only
The loss of the backward is the sum of the colour and of the map.  A second pass, with the library's kernel timers on (option "profile"),
gives distort_fwd's and distort_bwd's own time beside blend_fwd's and blend_bwd's from the same calls.  One JSON object on stdout (kept as
profiles/distort_overhead.json).

usage: python tools/distort_overhead.py [--steps 20] [--warmup 3] [--configs cfg3,cfg5]"""
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

CONFIGS = {"cfg3": (1_000_000, 1352, 1014), "cfg5": (3_000_000, 1920, 1080), "tiny": (20_000, 256, 192)}
KERNELS = ("blend_fwd", "blend_bwd", "distort_fwd", "distort_bwd")
VARIANTS = ("plain", "distortion", "moments")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="cfg3,cfg5")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import scenes
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)  # noqa: E731
    result = {"steps": a.steps, "warmup": a.warmup, "configs": {}}
    for name in a.configs.split(","):
        P, W, H = CONFIGS[name]
        sc = scenes.synth(P, 0)
        cam = scenes.camera(0, 1, W, H)
        V = t(cam["viewmatrix"])
        ras = rast.GaussianRasterizer(rast.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(sc["bg"]), scale_modifier=1.0,
            viewmatrix=V, projmatrix=t(cam["projmatrix"]), sh_degree=sc["sh_degree"], campos=t(cam["campos"]), prefiltered=False))
        ten = {k: t(sc[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        geo = dict(means3D=ten["means3D"], means2D=m2, opacities=ten["opacities"], scales=ten["scales"], rotations=ten["rotations"])

        def step(variant: str, backward: bool) -> float:
            for x in list(ten.values()) + [m2]:
                x.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.enable_grad() if backward else torch.no_grad():
                if variant == "moments":
                    z = ten["means3D"] @ V[:3, 2] + V[3, 2]
                    out = ras(shs=ten["shs"], features=torch.stack([torch.ones_like(z), z, z * z], dim=1), **geo)
                    A, M1, M2 = out[3]
                    loss = out[0].sum() + (A * M2 - M1 * M1).sum()
                else:
                    out = ras(shs=ten["shs"], **geo, **({"distortion": True} if variant == "distortion" else {}))
                    loss = out[0].sum() + (out[3].sum() if variant == "distortion" else 0.0)
                if backward:
                    loss.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        res = {"P": P, "W": W, "H": H}
        for backward, tag in ((False, "fwd"), (True, "fwd_bwd")):
            for _ in range(a.warmup):
                for v in VARIANTS:
                    step(v, backward)
            ms = {v: [] for v in VARIANTS}
            for _ in range(a.steps):
                for v in VARIANTS:
                    ms[v].append(step(v, backward))
            med = {v: statistics.median(ms[v]) for v in VARIANTS}
            for v in VARIANTS:
                res[f"{v}_{tag}_ms"] = round(med[v], 4)
                res[f"{v}_{tag}_spread_ms"] = [round(min(ms[v]), 4), round(max(ms[v]), 4)]
            res[f"distortion_added_{tag}_ms"] = round(med["distortion"] - med["plain"], 4)
            res[f"moments_added_{tag}_ms"] = round(med["moments"] - med["plain"], 4)
        # the kernels alone, from the library's event timers around their launches (they serialise the call: a pass of its own)
        kernel = {k: [] for k in KERNELS}
        L = rast._C.lib()
        kid = {L.gsrast_profile_kernel_name(k).decode(): k for k in range(L.gsrast_profile_kernel_count())}
        rast._C.set_option("profile", sum(1 << kid[k] for k in KERNELS))      # (a mask of kernel ids: only these are timed)
        try:
            for _ in range(a.steps):
                rast._C.profile_reset()
                step("distortion", True)
                prof = rast._C.profile_read()
                for k in KERNELS:
                    kms, n = prof[k]
                    kernel[k].append(kms / max(n, 1))
        finally:
            rast._C.set_option("profile", 0)
        for k in KERNELS:
            res[f"{k}_ms"] = round(statistics.median(kernel[k]), 4)
        res["last_late"] = rast._C.context_query("last_late")
        result["configs"][name] = res
        del ten, m2, ras, geo
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
