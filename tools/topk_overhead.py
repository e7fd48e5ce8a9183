"""What the per-pixel contributor query (pixel_contributors: each pixel's heaviest or first K Gaussians, their weights, its count) costs, at
BASELINE's cfg3 (1 M Gaussians @ 1352 x 1014) and cfg5 (3 M @ 1080p) shapes.  All legs in one run, taking turns call by call on the same
pose, so drift and the list cut's state affect them alike; medians of `--steps` device-synchronised calls after `--warmup` warm-ups:

    render_ms                 the forward-only render alone (_C.rasterize_gaussians(..., forward_only=True) under torch.no_grad())
    query_ms[order][K]        the public call -- that render plus the query -- at K = 1, 8, 16 in both orders
    contrib_stats_ms          gsrast_contrib_stats on one render's state: a replay of the same blend, the natural yardstick
    kernel_ms[order][K]       the query on that state by device events (the kernel and its output allocations, no render)
    contrib_stats_kernel_ms   contrib_stats on that state by device events

One JSON object on stdout (kept as profiles/topk_overhead.json).

usage: python tools/topk_overhead.py [--steps 20] [--warmup 3] [--configs cfg3,cfg5]"""
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
KS = (1, 8, 16)
ORDERS = ("weight", "depth")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="cfg3,cfg5")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import scenes
    _C = rast._C
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
        sink = torch.zeros((P, 4), device=dev)
        e = torch.empty(0)

        def render():
            with torch.no_grad():
                return _C.rasterize_gaussians(rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                              rs.tanfovx, rs.tanfovy, H, W, ten["shs"], sc["sh_degree"], rs.campos, False, forward_only=True)

        def wall(fn) -> float:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def events(fn) -> float:
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a_.record()
            fn()
            b_.record()
            torch.cuda.synchronize()
            return a_.elapsed_time(b_)

        R, _, _, gb, bb, ib, _ = render()          # the state the two replays are timed on (nothing renders between them and it)
        state_legs = {"contrib_stats": lambda: _C.contrib_stats(sink, None, R, W, H, gb, bb, ib)}
        for order in ORDERS:
            for K in KS:
                state_legs[f"{order}{K}"] = lambda K=K, order=order: _C.pixel_contributors(K, order, R, W, H, gb, bb, ib, P=P)
        kernel = {k: [] for k in state_legs}
        contrib_wall = []
        for step in range(a.warmup + a.steps):
            for k, fn in state_legs.items():
                ms = events(fn)
                if step >= a.warmup:
                    kernel[k].append(ms)
            ms = wall(state_legs["contrib_stats"])
            if step >= a.warmup:
                contrib_wall.append(ms)
        last = _C.pixel_contributors(16, "weight", R, W, H, gb, bb, ib, P=P)
        torch.cuda.synchronize()
        facts = {"instances": int(R), "count_mean": float(last[2].double().mean()), "count_max": int(last[2].max()),
                 "pixels_over_16": float((last[2] > 16).double().mean()), "pixels_empty": float((last[2] == 0).double().mean())}
        del gb, bb, ib, last
        # the render alone against the public call (render + query), taking turns
        legs = {"render": render}
        for order in ORDERS:
            for K in KS:
                legs[f"{order}{K}"] = lambda K=K, order=order: rast.pixel_contributors(ten["means3D"], ten["opacities"], ten["scales"], ten["rotations"],
                                                                                       raster_settings=rs, K=K, order=order, shs=ten["shs"])
        times = {k: [] for k in legs}
        for step in range(a.warmup + a.steps):
            for k, fn in legs.items():
                ms = wall(fn)
                if step >= a.warmup:
                    times[k].append(ms)
        med = lambda v: round(statistics.median(v), 4)  # noqa: E731
        render_ms = med(times["render"])
        result["configs"][name] = {
            "P": P, "W": W, "H": H, "render_ms": render_ms, "render_spread_ms": [round(min(times["render"]), 4), round(max(times["render"]), 4)],
            "query_ms": {order: {str(K): med(times[f"{order}{K}"]) for K in KS} for order in ORDERS},
            "query_over_render": {order: {str(K): round(med(times[f"{order}{K}"]) / render_ms, 4) for K in KS} for order in ORDERS},
            "contrib_stats_ms": med(contrib_wall), "contrib_stats_kernel_ms": med(kernel["contrib_stats"]),
            "kernel_ms": {order: {str(K): med(kernel[f"{order}{K}"]) for K in KS} for order in ORDERS},
            "k16_weight_query_costs_more_than_the_render": bool(med(times["weight16"]) - render_ms > render_ms),
            **facts, "last_late": _C.context_query("last_late")}
        del ten, sink
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
