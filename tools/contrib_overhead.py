"""What the per-Gaussian blend-weight statistics (contrib=sink, the input of importance pruning) cost: device-synchronised forward under
torch.no_grad() -- how a pruning sweep over the training cameras runs --, the plain call against contrib=sink, at BASELINE's cfg3
(1 M Gaussians @ 1352 x 1014) and cfg5 (3 M @ 1080p) shapes.  The two variants alternate call by call on the same pose, so drift and the
list cut's state affect both alike.  A second pass, with the library's kernel timers on (option "profile"), gives contrib_blend's and
contrib_finish's own time beside blend_fwd's from the same calls: the pass walks the same lists with a little more work per pair, so
blend_fwd is its yardstick.  One JSON object on stdout (kept as profiles/contrib_overhead.json).

usage: python tools/contrib_overhead.py [--steps 30] [--warmup 5] [--configs cfg3,cfg5]"""
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
KERNELS = ("blend_fwd", "contrib_blend", "contrib_finish")


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
        ten = {k: t(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        m2 = torch.zeros((P, 3), device=dev)
        sink = torch.zeros((P, 4), device=dev)
        ras = rast.GaussianRasterizer(rs)

        def step(contrib: bool) -> float:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                ras(means3D=ten["means3D"], means2D=m2, opacities=ten["opacities"], shs=ten["shs"], scales=ten["scales"], rotations=ten["rotations"],
                    **({"contrib": sink} if contrib else {}))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(a.warmup):
            step(False); step(True)
        plain, co = [], []
        for _ in range(a.steps):
            plain.append(step(False)); co.append(step(True))
        mp, mc = statistics.median(plain), statistics.median(co)
        # the kernels alone, from the library's event timers around their launches (they serialise the call: a pass of its own)
        kernel = {k: [] for k in KERNELS}
        L = rast._C.lib()
        kid = {L.gsrast_profile_kernel_name(k).decode(): k for k in range(L.gsrast_profile_kernel_count())}
        rast._C.set_option("profile", sum(1 << kid[k] for k in KERNELS))      # (a mask of kernel ids: only these are timed)
        try:
            for _ in range(a.steps):
                rast._C.profile_reset()
                step(True)
                prof = rast._C.profile_read()
                for k in KERNELS:
                    ms, n = prof[k]
                    kernel[k].append(ms / max(n, 1))
        finally:
            rast._C.set_option("profile", 0)
        km = {k: statistics.median(v) for k, v in kernel.items()}
        result["configs"][name] = {"P": P, "W": W, "H": H, "plain_ms": round(mp, 4), "contrib_ms": round(mc, 4), "ratio": round(mc / mp, 4),
                                   "plain_spread_ms": [round(min(plain), 4), round(max(plain), 4)],
                                   "contrib_spread_ms": [round(min(co), 4), round(max(co), 4)],
                                   "blend_fwd_ms": round(km["blend_fwd"], 4), "contrib_blend_ms": round(km["contrib_blend"], 4),
                                   "contrib_finish_ms": round(km["contrib_finish"], 4),
                                   "contrib_over_blend_fwd": round((km["contrib_blend"] + km["contrib_finish"]) / km["blend_fwd"], 4),
                                   "rows_nonzero": int((sink[:, 2] > 0).sum()), "weight_sum_total": float(sink[:, 0].double().sum()),
                                   "last_late": rast._C.context_query("last_late")}
        del ten, m2, ras, sink
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
