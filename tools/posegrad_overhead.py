"""What camera-pose gradients (camera_grads=True: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos) cost: device-synchronised forward + backward
of one training-shaped step (SH colours, scales / rotations, a loss on the colour), the plain call against camera_grads=True with the three
camera tensors requiring grad, at BASELINE's cfg3 (1 M Gaussians @ 1352 x 1014) and cfg5 (3 M @ 1080p) shapes.  The two variants alternate
step by step on the same pose, so drift and the list cut's state affect both alike.  A second pass, with the library's kernel timers on
(option "profile"), gives the per-Gaussian backward's own time per step (preprocess_bwd: with the flag it includes pose_grad_reduce_kernel)
for both variants, again alternating.  One JSON object on stdout.

usage: python tools/posegrad_overhead.py [--steps 30] [--warmup 5] [--configs cfg3,cfg5]"""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
        rs = rast.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(sc["bg"]), scale_modifier=1.0,
            viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]), sh_degree=sc["sh_degree"], campos=t(cam["campos"]),
            prefiltered=False)
        leaves = {k: t(sc[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        gC = t(scenes.upstream_grad(H, W, 1))
        camera = [rs.viewmatrix.requires_grad_(True), rs.projmatrix.requires_grad_(True), rs.campos.requires_grad_(True)]
        ras = rast.GaussianRasterizer(rs)

        def step(pose: bool) -> float:
            for v in list(leaves.values()) + [m2] + camera:
                v.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ras(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                      scales=leaves["scales"], rotations=leaves["rotations"], **({"camera_grads": True} if pose else {}))
            (out[0] * gC).sum().backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(a.warmup):
            step(False); step(True)
        plain, ab = [], []
        for _ in range(a.steps):
            plain.append(step(False)); ab.append(step(True))
        mp, ma = statistics.median(plain), statistics.median(ab)
        cam_max = max(float(v.grad.abs().max()) for v in camera)      # (the last timed step was one with the flag)
        # the per-Gaussian backward alone, from the library's event timers around its launches (they serialise the call: a pass of its own)
        kernel = {False: [], True: []}
        L = rast._C.lib()
        kid = {L.gsrast_profile_kernel_name(k).decode(): k for k in range(L.gsrast_profile_kernel_count())}
        rast._C.set_option("profile", 1 << kid["preprocess_bwd"])      # (a mask of kernel ids: only this one is timed)
        try:
            for _ in range(a.steps):
                for v in (False, True):
                    rast._C.profile_reset()
                    step(v)
                    ms, n = rast._C.profile_read()["preprocess_bwd"]
                    kernel[v].append(ms / max(n, 1))
        finally:
            rast._C.set_option("profile", 0)
        kp, ka = statistics.median(kernel[False]), statistics.median(kernel[True])
        result["configs"][name] = {"P": P, "W": W, "H": H, "plain_ms": round(mp, 4), "camera_grads_ms": round(ma, 4), "ratio": round(ma / mp, 4),
                                   "plain_spread_ms": [round(min(plain), 4), round(max(plain), 4)],
                                   "camera_grads_spread_ms": [round(min(ab), 4), round(max(ab), 4)],
                                   "preprocess_bwd_plain_ms": round(kp, 4), "preprocess_bwd_camera_grads_ms": round(ka, 4),
                                   "preprocess_bwd_ratio": round(ka / kp, 4),
                                   "camera_grad_max": cam_max, "last_late": rast._C.context_query("last_late")}
        del leaves, m2, ras, camera
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
