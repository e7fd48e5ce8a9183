"""What the MCMC densification calls cost beside a torch restatement of gsplat's ops, timed in the same process: device-synchronised
medians at P = 1 M and 3 M, the seven groups of tests/test_adam.py (60 floats per Gaussian) with Adam moments.  Per size, in this order:
    noise_fused / noise_torch        mcmc_inject_noise  against  quat_scale_to_covar + einsum + add_ over all P rows
    relocate_fused / relocate_torch  mcmc_relocate (its one read-back included)  against  the index-based relocate with torch.multinomial
                                     and bincount; 5 % of the rows dead, the state restored outside the timed window
    grow_fused / grow_torch          mcmc_grow  against  sample_add with torch.cat; 5 % growth, on a fresh optimizer each step
and, from a second pass with the library's kernel timers on (option "profile"), mcmc_plan / mcmc_sample / mcmc_apply / mcmc_noise on
their own.  The two conditions the README states: (a) noise_fused < noise_torch, (b) relocate_fused < relocate_torch, at both sizes.
One JSON object on stdout (kept as profiles/mcmc_overhead.json).

usage: python tools/mcmc_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import torch  # noqa: E402

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "temporal_pos": (1,)}
MIN_OPACITY, DEAD_FRACTION, N_MAX = 0.005, 0.05, 51


def binoms(dev):
    b = torch.zeros((N_MAX, N_MAX), dtype=torch.float32, device=dev)
    for n in range(N_MAX):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b


def torch_compute_relocation(opacities, scales, ratios, B):
    """gsplat/relocation.py compute_relocation as torch ops: its fp32 double loop, vectorised over the sampled rows."""
    ratios = ratios.clamp(1, N_MAX)
    new_o = 1.0 - torch.pow(1.0 - opacities, 1.0 / ratios)
    k = torch.arange(N_MAX, device=opacities.device, dtype=torch.float32)
    terms = torch.pow(-1.0, k) / torch.sqrt(k + 1) * torch.pow(new_o[:, None], k + 1)      # [n, 51]
    csum = torch.cumsum(B, 0)                                                               # sum_{i <= r} C(i-1, k)
    denom = (csum[ratios.long() - 1] * terms).sum(1)
    return new_o, (opacities / denom)[:, None] * scales


def torch_noise(xyz, rotation, scaling, opacity, noise, scale):
    q = torch.nn.functional.normalize(rotation, dim=1)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * torch.exp(scaling)[:, None, :]
    covars = torch.bmm(M, M.transpose(1, 2))
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - torch.sigmoid(opacity).reshape(-1)) - 0.995)))
    xyz.add_(torch.einsum("bij,bj->bi", covars, noise * gate[:, None] * scale))


def torch_relocate(params, state, B, gen):
    o = torch.sigmoid(params["opacity"]).reshape(-1)
    dead = o <= MIN_OPACITY
    dead_idx, alive_idx = dead.nonzero(as_tuple=True)[0], (~dead).nonzero(as_tuple=True)[0]
    if dead_idx.numel() == 0:
        return
    sampled = alive_idx[torch.multinomial(o[alive_idx], dead_idx.numel(), replacement=True, generator=gen)]
    ratios = torch.bincount(sampled, minlength=o.numel())[sampled] + 1
    new_o, new_s = torch_compute_relocation(o[sampled], torch.exp(params["scaling"][sampled]), ratios, B)
    new_o = new_o.clamp(MIN_OPACITY, 1.0 - torch.finfo(torch.float32).eps)
    params["opacity"][sampled] = torch.logit(new_o)[:, None]
    params["scaling"][sampled] = torch.log(new_s)
    for k, p in params.items():
        p[dead_idx] = p[sampled]
        for m in state[k]:
            m[sampled] = 0


def torch_grow(params, state, n, B, gen):
    o = torch.sigmoid(params["opacity"]).reshape(-1)
    sampled = torch.multinomial(o, n, replacement=True, generator=gen)
    ratios = torch.bincount(sampled, minlength=o.numel())[sampled] + 1
    new_o, new_s = torch_compute_relocation(o[sampled], torch.exp(params["scaling"][sampled]), ratios, B)
    new_o = new_o.clamp(MIN_OPACITY, 1.0 - torch.finfo(torch.float32).eps)
    params["opacity"][sampled] = torch.logit(new_o)[:, None]
    params["scaling"][sampled] = torch.log(new_s)
    out_p = {k: torch.cat((p, p[sampled])) for k, p in params.items()}
    out_s = {k: tuple(torch.cat((m, torch.zeros((n,) + tuple(m.shape[1:]), device=m.device))) for m in state[k]) for k in state}
    return out_p, out_s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_adam
    import fused_densify
    dev = torch.device("cuda:0")
    B = binoms(dev)
    result = {"steps": a.steps, "warmup": a.warmup, "floats_per_gaussian": 60, "dead_fraction": DEAD_FRACTION, "growth": 1.05, "sizes": {}}
    for P in (int(x) for x in a.sizes.split(",")):
        torch.manual_seed(0)
        base = {k: torch.randn((P,) + s, device=dev) for k, s in SHAPES.items()}
        o = 0.02 + 0.97 * torch.rand(P, 1, device=dev)
        o[torch.rand(P, 1, device=dev) < DEAD_FRACTION] = 0.001
        base["opacity"] = torch.logit(o)
        base["scaling"] = torch.log(0.01 + 0.05 * torch.rand(P, 3, device=dev))
        noise = torch.randn(P, 3, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        n_grow = int(1.05 * P) - P

        def fresh():
            """(optimizer over clones of `base` with moments, its parameter dict, its moment dict)"""
            ps = {k: v.clone().requires_grad_(True) for k, v in base.items()}
            opt = fused_adam.GaussianAdam([{"params": [ps[k]], "lr": 1e-3, "name": k} for k in SHAPES], eps=1e-15)
            for p in ps.values():
                opt.state[p] = {"exp_avg": torch.full_like(p, 1e-3), "exp_avg_sq": torch.full_like(p, 1e-6)}
            return opt, {k: p.detach() for k, p in ps.items()}, {k: (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for k, p in ps.items()}

        def timed(setup, run):
            ms = []
            for it in range(a.warmup + a.steps):
                ctx = setup()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(ctx)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
                del ctx
            return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]

        legs = {
            "noise_fused": (fresh, lambda c: fused_densify.mcmc_inject_noise(c[1]["xyz"], c[1]["rotation"], c[1]["scaling"], c[1]["opacity"], scale=1e-3, noise=noise)),
            "noise_torch": (fresh, lambda c: torch_noise(c[1]["xyz"], c[1]["rotation"], c[1]["scaling"], c[1]["opacity"], noise, 1e-3)),
            "relocate_fused": (fresh, lambda c: fused_densify.mcmc_relocate(c[0], min_opacity=MIN_OPACITY, generator=gen)),
            "relocate_torch": (fresh, lambda c: torch_relocate(c[1], c[2], B, gen)),
            "grow_fused": (fresh, lambda c: fused_densify.mcmc_grow(c[0], cap_max=10**9, min_opacity=MIN_OPACITY, generator=gen)),
            "grow_torch": (fresh, lambda c: torch_grow(c[1], c[2], n_grow, B, gen)),
        }
        res = {"P": P, "n_dead": int((torch.sigmoid(base["opacity"]) <= MIN_OPACITY).sum()), "n_grow": n_grow}
        with torch.no_grad():
            for name, (setup, run) in legs.items():
                res[f"{name}_ms"], res[f"{name}_spread_ms"] = timed(setup, run)
        for leg in ("noise", "relocate", "grow"):
            res[f"{leg}_fused_over_torch"] = round(res[f"{leg}_fused_ms"] / res[f"{leg}_torch_ms"], 4)
        res["a_noise_fused_below_torch"] = bool(res["noise_fused_ms"] < res["noise_torch_ms"])
        res["b_relocate_fused_below_torch"] = bool(res["relocate_fused_ms"] < res["relocate_torch_ms"])
        # the kernels alone, from the library's event timers around their launches (a pass of its own)
        L = rast._C.lib()
        kid = {L.gsrast_profile_kernel_name(k).decode(): k for k in range(L.gsrast_profile_kernel_count())}
        mine = ("mcmc_plan", "mcmc_sample", "mcmc_apply", "mcmc_noise")
        word = sum(1 << kid[n] for n in mine)
        rast._C.set_option("profile", word - (1 << 32) if word >= 1 << 31 else word)      # (the option's word is a signed int)
        try:
            with torch.no_grad():
                for leg in ("noise_fused", "relocate_fused", "grow_fused"):
                    setup, run = legs[leg]
                    per = {n: [] for n in mine}
                    for _ in range(a.steps):
                        ctx = setup()
                        rast._C.profile_reset()
                        run(ctx)
                        torch.cuda.synchronize()
                        got = rast._C.profile_read()
                        for n in mine:
                            if got[n][1]:
                                per[n].append(got[n][0] / got[n][1])
                        del ctx
                    res[f"{leg}_kernels_ms"] = {n: round(statistics.median(v), 4) for n, v in per.items() if v}
        finally:
            rast._C.set_option("profile", 0)
        res["noise_fused_GBps"] = round(P * 68 / (res["noise_fused_kernels_ms"]["mcmc_noise"] * 1e-3) / 1e9, 1)      # 56 B read + 12 B written per row
        result["sizes"][str(P)] = res
        del base, noise, legs
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
