"""What one densification costs: `fused_densify.densify_and_prune` (one classify, one scan, one row-moving launch, one read-back)
against the sequential torch restatement of the reference's clone -> split -> prune chain on a torch.optim.Adam (tests/densify_math.py
::sequential, run on the same device) -- what a user without the fused call has to run.  P = 1 M and 3 M Gaussians, M = 16 (60 floats
+ 120 of moments per Gaussian), about 10 % cloned, 5 % split, 5 % pruned.  Medians of device-synchronised runs after warm-up runs, the
peak of allocated bytes above the model itself, the bytes the fused call moves per second, and its kernels' own times (option "profile").
One JSON object on stdout.  One process; run it under a time limit of its own:

usage: timeout -k 10 900 python tools/densify_overhead.py [--sizes 1000000,3000000] [--runs 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

THR, TAU, MIN_OPACITY, N = 2e-4, 0.05, 0.005, 2
KERNELS = ("densify_classify", "densify_scan", "densify_apply")
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29          # MI355X: specification, and what a float4 copy reaches


def inputs(P, M, dev, seed=0):
    import densify_math as dm
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, device=dev)  # noqa: E731
    params = {k: torch.randn(P, *s, generator=g, device=dev) for k, s in dm.shapes(M).items()}
    sel, big = u(P) < 0.15, u(P) < 1.0 / 3.0                         # 15 % over the gradient threshold: two thirds small (clone), a third big (split)
    grad = torch.where(sel, THR * (1.05 + 2 * u(P)), THR * 0.95 * u(P))
    denom = torch.floor(1 + 6 * u(P))
    top = torch.where(big, TAU * (1.05 + 3 * u(P)), TAU * (0.2 + 0.75 * u(P)))
    params["scaling"] = torch.log(top[:, None] * (0.1 + 0.9 * u(P, 3)).clamp(max=1.0).index_fill_(1, torch.tensor([0], device=dev), 1.0))
    o = torch.where(u(P) < 0.05, MIN_OPACITY * (0.05 + 0.45 * u(P)), 2 * MIN_OPACITY + (0.99 - 2 * MIN_OPACITY) * u(P))
    params["opacity"] = torch.log(o / (1 - o)).reshape(P, 1)
    moments = {k: (torch.randn_like(v) * 1e-3, torch.rand_like(v) * 1e-5) for k, v in params.items()}
    return params, moments, (grad * denom).reshape(P, 1), denom.reshape(P, 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=16)
    a = ap.parse_args()
    import densify_math as dm
    import fused_adam
    import fused_densify
    from diff_gaussian_rasterization_ch3 import _C
    dev = torch.device("cuda:0")
    kid = {_C.lib().gsrast_profile_kernel_name(k).decode(): k for k in range(_C.lib().gsrast_profile_kernel_count())}
    result = {"runs": a.runs, "warmup": a.warmup, "M": a.M, "n_split": N, "sizes": {}}
    for P in (int(x) for x in a.sizes.split(",")):
        params, moments, accum, denom = inputs(P, a.M, dev)
        floats = sum(v[0].numel() for v in params.values())

        def fused():
            opt = fused_adam.GaussianAdam([{"params": [torch.nn.Parameter(v)], "lr": 0.0, "name": k} for k, v in params.items()], eps=1e-15)
            for g in opt.param_groups:
                opt.state[g["params"][0]] = {"exp_avg": moments[g["name"]][0], "exp_avg_sq": moments[g["name"]][1]}
            stats = fused_densify.DensifyStats(P, dev)
            stats.xyz_gradient_accum, stats.denom = accum, denom
            gen = torch.Generator(device=dev).manual_seed(1)
            return lambda: fused_densify.densify_and_prune(opt, stats, grad_threshold=THR, percent_dense=TAU, extent=1.0, min_opacity=MIN_OPACITY,
                                                           n_split=N, generator=gen)[0]

        def sequential():
            opt = dm.make_adam(params, moments)          # (copies the model: outside the timed part)
            n_all = int(dm.classify(params, accum, denom, thr=THR, tau=TAU, min_opacity=MIN_OPACITY)[1].sum())
            gen = torch.Generator(device=dev).manual_seed(1)

            def run():
                noise = torch.randn((N * n_all, 3), generator=gen, device=dev)
                left = dm.sequential(opt, accum, denom, noise, thr=THR, tau=TAU, N=N, min_opacity=MIN_OPACITY)
                return {"P": left}
            return run

        def measure(make):
            times, peak, last = [], 0, None
            for k in range(a.warmup + a.runs):
                run = make()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                t0 = time.perf_counter()
                last = run()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if k >= a.warmup:
                    times.append(dt)
                    peak = max(peak, torch.cuda.max_memory_allocated(dev) - base)
                del run
            return times, peak, last

        tf, pf, counts = measure(fused)
        ts, ps, left = measure(sequential)
        assert left["P"] == counts["P"], (left, counts)
        # the fused call's traffic: kept originals read parameter + two moments, split sources their parameter; every new row written with both moments
        moved = 4 * floats * (3 * counts["n_kept"] + counts["n_split"] + 3 * counts["P"]) + P * (4 * 7 + 2)
        mask = sum(1 << kid[k] for k in KERNELS)
        _C.profile_reset()
        _C.set_option("profile", mask)
        for _ in range(3):
            fused()()
        torch.cuda.synchronize()
        pk = _C.profile_read()
        _C.set_option("profile", 0)
        mf, ms = statistics.median(tf), statistics.median(ts)
        kern = {k: round(pk[k][0] / max(pk[k][1], 1), 4) for k in KERNELS}
        result["sizes"][str(P)] = {
            "counts": counts, "fused_ms": round(mf, 4), "sequential_torch_ms": round(ms, 4), "ratio": round(ms / mf, 3),
            "fused_spread_ms": [round(min(tf), 4), round(max(tf), 4)], "sequential_spread_ms": [round(min(ts), 4), round(max(ts), 4)],
            "fused_peak_bytes": pf, "sequential_peak_bytes": ps, "fused_bytes_moved": moved,
            "fused_gb_per_s_whole_call": round(moved / mf / 1e6, 1), "kernel_ms_per_launch": kern,
            "apply_gb_per_s": round(moved / max(kern["densify_apply"], 1e-9) / 1e6, 1),
            "apply_fraction_of_hbm_peak": round(moved / max(kern["densify_apply"], 1e-9) / 1e9 / HBM_PEAK_TBS, 3),
            "apply_fraction_of_measured_copy": round(moved / max(kern["densify_apply"], 1e-9) / 1e9 / HBM_COPY_TBS, 3)}
        del params, moments, accum, denom
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
