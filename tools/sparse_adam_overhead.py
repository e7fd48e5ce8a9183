"""What GaussianAdam.step(visibility=mask) costs beside the dense step(): device-synchronised medians at P = 1 M and 3 M, the seven groups of
tests/test_adam.py (60 floats per Gaussian) with per-row rates as tools/bench_extras.py's adam_row sets them (every group but f_rest).
Measured in ONE run on one card, in this order:
    dense_A, dense_A2        the dense step(), twice: |A - A2| is the run's own noise
    visible_1.0 / 0.5 / 0.22 / 0.05      step(visibility=mask), a seeded random bool mask of that visible fraction
    visible_0.22_runs256     the same fraction with visibility in runs of 256 consecutive rows (whole waves of the kernel leave at once)
    visible_0.22_int32       the 0.22 random mask passed as int32 (> 0 = visible: a render's radii)
and, from a second pass with the library's kernel timers on (option "profile"), adam_step_visible's own time per variant.
The two conditions the README states: (a) masked at 0.22 random < dense at both sizes; (b) masked at 1.0 exceeds dense by no more than
2 |A - A2|.  One JSON object on stdout (kept as profiles/sparse_adam_overhead.json).

usage: python tools/sparse_adam_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import torch  # noqa: E402

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "temporal_pos": (1,)}
FRACTIONS = (1.0, 0.5, 0.22, 0.05)
RUN = 256


def masks(P: int, dev) -> dict:
    g = torch.Generator(device="cpu").manual_seed(1234)
    out = {}
    for f in FRACTIONS:
        out[f"visible_{f}"] = (torch.rand(P, generator=g) < f).to(dev)
    runs = torch.rand((P + RUN - 1) // RUN, generator=g) < 0.22
    out["visible_0.22_runs256"] = runs.repeat_interleave(RUN)[:P].contiguous().to(dev)
    out["visible_0.22_int32"] = out["visible_0.22"].to(torch.int32) * 7
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_adam
    dev = torch.device("cuda:0")
    result = {"steps": a.steps, "warmup": a.warmup, "floats_per_gaussian": 60, "sizes": {}}
    for P in (int(x) for x in a.sizes.split(",")):
        torch.manual_seed(0)
        ps = {k: torch.randn((P,) + s, device=dev).requires_grad_(True) for k, s in SHAPES.items()}
        inv = 1.0 + torch.rand(P, 1, device=dev)
        opt = fused_adam.GaussianAdam([{"params": [ps[k]], "lr": 1e-3 * inv if k != "f_rest" else 1e-4, "name": k} for k in SHAPES], eps=1e-15)
        for v in ps.values():
            v.grad = torch.randn_like(v) * 1e-2
        ms_of = masks(P, dev)

        def step(mask) -> float:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.step() if mask is None else opt.step(visibility=mask)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def timed(mask):
            for _ in range(a.warmup):
                step(mask)
            ms = [step(mask) for _ in range(a.steps)]
            return statistics.median(ms), [round(min(ms), 4), round(max(ms), 4)]

        res = {"P": P}
        for name, mask in [("dense_A", None), ("dense_A2", None)] + list(ms_of.items()):
            med, spread = timed(mask)
            res[f"{name}_ms"], res[f"{name}_spread_ms"] = round(med, 4), spread
            if mask is not None:
                res[f"{name}_fraction"] = round(float((mask > 0).float().mean()), 4)
        noise = abs(res["dense_A_ms"] - res["dense_A2_ms"])
        dense = min(res["dense_A_ms"], res["dense_A2_ms"])
        res["dense_noise_ms"] = round(noise, 4)
        for name in ms_of:
            res[f"{name}_over_dense"] = round(res[f"{name}_ms"] / dense, 4)
        res["a_visible_0.22_below_dense"] = bool(res["visible_0.22_ms"] < dense)
        res["b_all_visible_within_2x_noise"] = bool(res["visible_1.0_ms"] - dense <= 2.0 * noise)
        # the kernel alone, from the library's event timers around its launch (a pass of its own)
        L = rast._C.lib()
        kid = {L.gsrast_profile_kernel_name(k).decode(): k for k in range(L.gsrast_profile_kernel_count())}
        rast._C.set_option("profile", 1 << kid["adam_step_visible"])
        try:
            for name, mask in ms_of.items():
                ks = []
                for _ in range(a.steps):
                    rast._C.profile_reset()
                    step(mask)
                    kms, n = rast._C.profile_read()["adam_step_visible"]
                    ks.append(kms / max(n, 1))
                res[f"{name}_kernel_ms"] = round(statistics.median(ks), 4)
        finally:
            rast._C.set_option("profile", 0)
        nbytes = P * 60 * 28 + P * 4 * 6
        res["dense_GBps"] = round(nbytes / (dense * 1e-3) / 1e9, 1)
        result["sizes"][str(P)] = res
        del ps, opt, ms_of, inv
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
