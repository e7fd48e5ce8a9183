"""What the fused 3-layer heads cost beside the same nn.Sequential on the same device in the same process: device-synchronised medians
at N = 1 M and 3 M rows for the reference's four heads (scene/saro_gaussian.py:104-110):
    motion 32 + 9 -> 128 -> 128 -> 3     rot 32 + 9 -> 128 -> 128 -> 7     shs 32 + 9 -> 128 -> 128 -> 48     opacity 32 -> 128 -> 64 -> 1, sigmoid
Per head: forward (under no_grad) and forward + backward (gradients to x and all six parameters), fused and torch, and the peak memory
of one forward + backward above what is allocated before it.  torch's leg includes the cat((feature, time_emb), 1) the reference makes;
the fused leg reads the tail in place.  three_heads_* is the sum over motion, rot and shs.  From a second pass with the library's kernel
timers on (option "profile" = -1), mlp_fwd and mlp_bwd on their own, with the TFLOP/s they amount to (forward 2 N (D_in H1 + H1 H2 +
H2 D_out) flop; backward 3 x that: recomputation, data gradient, weight gradient).
The two conditions the README states: (a) fused forward + backward of the three 3-layer heads below torch's, (b) fused peak memory of a
forward + backward below torch's by about the hidden activations, N (H1 + H2) 4 B.  One JSON object on stdout (kept as
profiles/mlp_overhead.json).

usage: python tools/mlp_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import torch  # noqa: E402
from torch import nn  # noqa: E402

HEADS = {"motion": (32, 9, 128, 128, 3, False), "rot": (32, 9, 128, 128, 7, False), "shs": (32, 9, 128, 128, 48, False),
         "opacity": (32, 0, 128, 64, 1, True)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_mlp
    dev = torch.device("cuda:0")
    result = {"steps": a.steps, "warmup": a.warmup, "heads": {k: list(v) for k, v in HEADS.items()}, "sizes": {}}

    def timed(run):
        ms = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 4)

    def peak_of(run):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        run()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2**20

    for N in (int(x) for x in a.sizes.split(",")):
        res = {"N": N}
        torch.manual_seed(0)
        for name, (d_x, d_tail, h1, h2, d_out, sig) in HEADS.items():
            seq = nn.Sequential(*([nn.Linear(d_x + d_tail, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU(), nn.Linear(h2, d_out)]
                                  + ([nn.Sigmoid()] if sig else []))).to(dev)
            fused = fused_mlp.FusedMLP3.from_sequential(seq)
            x = torch.randn(N, d_x, device=dev, requires_grad=True)
            tail = torch.randn(N, d_tail, device=dev) if d_tail else None
            dy = torch.randn(N, d_out, device=dev)

            def fwd_torch():
                return seq(torch.cat((x, tail), 1) if tail is not None else x)

            def fwd_fused():
                return fused(x, tail)

            def both(fwd):
                def run():
                    x.grad = None
                    seq.zero_grad(set_to_none=True)
                    fwd().backward(dy)
                return run

            def no_grad(fwd):
                def run():
                    with torch.no_grad():
                        fwd()
                return run

            r = {}
            r["fwd_fused_ms"], r["fwd_torch_ms"] = timed(no_grad(fwd_fused)), timed(no_grad(fwd_torch))
            r["fwd_bwd_fused_ms"], r["fwd_bwd_torch_ms"] = timed(both(fwd_fused)), timed(both(fwd_torch))
            x.grad = None
            seq.zero_grad(set_to_none=True)
            r["peak_fused_MiB"], r["peak_torch_MiB"] = round(peak_of(both(fwd_fused)), 1), round(peak_of(both(fwd_torch)), 1)
            x.grad = None
            seq.zero_grad(set_to_none=True)
            r["hidden_activations_MiB"] = round(N * (h1 + h2) * 4 / 2**20, 1)
            # the two kernels alone: the library's event timers around their launches (a pass of its own)
            flop = 2.0 * N * ((d_x + d_tail) * h1 + h1 * h2 + h2 * d_out)
            rast._C.set_option("profile", -1)
            try:
                per = {"mlp_fwd": [], "mlp_bwd": []}
                run = both(fwd_fused)
                for _ in range(a.steps):
                    rast._C.profile_reset()
                    run()
                    torch.cuda.synchronize()
                    got = rast._C.profile_read()
                    for k in per:
                        if got[k][1]:
                            per[k].append(got[k][0] / got[k][1])
            finally:
                rast._C.set_option("profile", 0)
            r["kernels_ms"] = {k: round(statistics.median(v), 4) for k, v in per.items() if v}
            r["kernels_TFLOPs"] = {"mlp_fwd": round(flop / (r["kernels_ms"]["mlp_fwd"] * 1e-3) / 1e12, 1),
                                   "mlp_bwd": round(3 * flop / (r["kernels_ms"]["mlp_bwd"] * 1e-3) / 1e12, 1)}
            res[name] = r
            del seq, fused, x, tail, dy
            torch.cuda.empty_cache()
        three = ("motion", "rot", "shs")
        for leg in ("fwd_fused_ms", "fwd_torch_ms", "fwd_bwd_fused_ms", "fwd_bwd_torch_ms"):
            res["three_heads_" + leg] = round(sum(res[h][leg] for h in three), 4)
        res["three_heads_fwd_bwd_fused_over_torch"] = round(res["three_heads_fwd_bwd_fused_ms"] / res["three_heads_fwd_bwd_torch_ms"], 4)
        res["a_three_heads_fwd_bwd_fused_below_torch"] = bool(res["three_heads_fwd_bwd_fused_ms"] < res["three_heads_fwd_bwd_torch_ms"])
        # (b) "about": the saving is at least three quarters of the hidden activations, for every head
        res["b_peak_lower_by_about_the_hidden_activations"] = bool(all(
            res[h]["peak_torch_MiB"] - res[h]["peak_fused_MiB"] >= 0.75 * res[h]["hidden_activations_MiB"] for h in HEADS))
        result["sizes"][str(N)] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
