"""What the bf16 path of the fused 3-layer heads costs beside the fp32 path and beside torch, on the same device in the same process:
device-synchronised medians at N = 1 M and 3 M rows for the reference's four heads (scene/saro_gaussian.py:104-110), the protocol of
tools/mlp_overhead.py (medians of --steps synchronised calls after --warmup).  Four legs per head:
    fused_bf16      FusedMLP3(precision="bf16")          fused_fp32      FusedMLP3(precision="fp32")
    torch_fp32      the nn.Sequential                    torch_autocast  the nn.Sequential under torch.autocast("cuda", torch.bfloat16)
each as forward (under no_grad) and forward + backward (gradients to x and all six parameters); torch's legs include the
cat((feature, time_emb), 1) the reference makes, the fused legs read the tail in place.  From a second pass with the library's kernel
timers on (option "profile" = -1): mlp_fwd and mlp_bwd on their own for both fused legs, with the TFLOP/s they amount to (forward
2 N (D_in H1 + H1 H2 + H2 D_out) flop; backward 3 x that).  three_heads_* is the sum over motion, rot and shs.
The two claims the README records as holds / does not hold:
    (a) bf16 forward + backward of the three 3-layer heads is below the fused fp32's of the same run
    (b) bf16 forward of the three 3-layer heads is below torch's fp32 forward (the render path)
With --test-log PATH (the output of `pytest -s tests/test_gpu_mlp_bf16.py -k generic_floats` on the same device) the accuracy figures that
test printed are recorded too: per shape the worst r = |T_gpu - T_model|_2 / |T_model|_2 over its tensors and row counts, the tensor and row
count it occurred at, R and the bar 4 R + 2^-23.
One JSON object on stdout (kept as profiles/mlp_bf16_overhead.json).

usage: python tools/mlp_bf16_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000] [--test-log PATH]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import torch  # noqa: E402
from torch import nn  # noqa: E402

HEADS = {"motion": (32, 9, 128, 128, 3, False), "rot": (32, 9, 128, 128, 7, False), "shs": (32, 9, 128, 128, 48, False),
         "opacity": (32, 0, 128, 64, 1, True)}
LEGS = ("fused_bf16", "fused_fp32", "torch_fp32", "torch_autocast")


def accuracy_from_test_log(path: str) -> dict:
    """{shape: worst r, where, R, bar} from the lines "<shape> N=<n> <tensor>: r <r>  R <R>  bar <bar>" of the generic-floats test."""
    out = {}
    for m in re.finditer(r"([\d-]+) N=(\d+) (\w+): r (\S+)  R (\S+)  bar (\S+)", open(path).read()):
        shape, n, tensor, r, R, bar = m.group(1), int(m.group(2)), m.group(3), float(m.group(4)), float(m.group(5)), float(m.group(6))
        if shape not in out or r > out[shape]["worst_r"]:
            out[shape] = {"worst_r": r, "tensor": tensor, "N": n, "R": R, "bar": bar}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--test-log", default=None)
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

    for N in (int(x) for x in a.sizes.split(",")):
        res = {"N": N}
        torch.manual_seed(0)
        for name, (d_x, d_tail, h1, h2, d_out, sig) in HEADS.items():
            seq = nn.Sequential(*([nn.Linear(d_x + d_tail, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU(), nn.Linear(h2, d_out)]
                                  + ([nn.Sigmoid()] if sig else []))).to(dev)
            fused = {p: fused_mlp.FusedMLP3.from_sequential(seq, precision=p) for p in ("bf16", "fp32")}
            x = torch.randn(N, d_x, device=dev, requires_grad=True)
            tail = torch.randn(N, d_tail, device=dev) if d_tail else None
            dy = torch.randn(N, d_out, device=dev)

            def torch_fp32():
                return seq(torch.cat((x, tail), 1) if tail is not None else x)

            def torch_autocast():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return seq(torch.cat((x, tail), 1) if tail is not None else x).float()

            fwd = {"fused_bf16": lambda: fused["bf16"](x, tail), "fused_fp32": lambda: fused["fp32"](x, tail),
                   "torch_fp32": torch_fp32, "torch_autocast": torch_autocast}

            def both(f):
                def run():
                    x.grad = None
                    seq.zero_grad(set_to_none=True)
                    f().backward(dy)
                return run

            def no_grad(f):
                def run():
                    with torch.no_grad():
                        f()
                return run

            r = {}
            for leg in LEGS:
                r["fwd_" + leg + "_ms"] = timed(no_grad(fwd[leg]))
            for leg in LEGS:
                r["fwd_bwd_" + leg + "_ms"] = timed(both(fwd[leg]))
            x.grad = None
            seq.zero_grad(set_to_none=True)
            # the kernels alone: the library's event timers around their launches (a pass of its own)
            flop = 2.0 * N * ((d_x + d_tail) * h1 + h1 * h2 + h2 * d_out)
            rast._C.set_option("profile", -1)
            try:
                for leg in ("fused_bf16", "fused_fp32"):
                    per = {"mlp_fwd": [], "mlp_bwd": []}
                    run = both(fwd[leg])
                    for _ in range(a.steps):
                        rast._C.profile_reset()
                        run()
                        torch.cuda.synchronize()
                        got = rast._C.profile_read()
                        for k in per:
                            if got[k][1]:
                                per[k].append(got[k][0] / got[k][1])
                    ms = {k: round(statistics.median(v), 4) for k, v in per.items() if v}
                    r["kernels_" + leg + "_ms"] = ms
                    r["kernels_" + leg + "_TFLOPs"] = {"mlp_fwd": round(flop / (ms["mlp_fwd"] * 1e-3) / 1e12, 1),
                                                       "mlp_bwd": round(3 * flop / (ms["mlp_bwd"] * 1e-3) / 1e12, 1)}
            finally:
                rast._C.set_option("profile", 0)
            res[name] = r
            del seq, fused, x, tail, dy
            torch.cuda.empty_cache()
        three = ("motion", "rot", "shs")
        for mode in ("fwd_", "fwd_bwd_"):
            for leg in LEGS:
                res["three_heads_" + mode + leg + "_ms"] = round(sum(res[h][mode + leg + "_ms"] for h in three), 4)
        res["a_three_heads_fwd_bwd_bf16_below_fused_fp32"] = bool(res["three_heads_fwd_bwd_fused_bf16_ms"] < res["three_heads_fwd_bwd_fused_fp32_ms"])
        res["b_three_heads_fwd_bf16_below_torch_fp32"] = bool(res["three_heads_fwd_fused_bf16_ms"] < res["three_heads_fwd_torch_fp32_ms"])
        result["sizes"][str(N)] = res
    if a.test_log:
        result["generic_floats_r_and_R"] = accuracy_from_test_log(a.test_log)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
