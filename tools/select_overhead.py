"""What the differentiable row selection costs and what it saves, on the same device in the same process: device-synchronised medians (of
--steps synchronised calls after --warmup) at P = 1 M and 3 M rows for alive fractions 1.0, 0.7 and 0.3, the alive rows placed at random
and in runs of 256.  All legs in one run.

Primitives, forward + backward (every input requires a gradient):
    gather_fused     sel.gather(feature [P,32], time_emb [P,9])            gather_torch     x[rows] for each (rows: int64, made beforehand)
    scatter_fused    sel.scatter(residuals [n,3], [n,7], [n,48])           scatter_torch    zeros.index_copy_(0, rows, y) for each
    select_fused     fused_densify.select_rows (plan + the read-back)      select_torch     mask.nonzero()
Heads step, forward + backward, the three 3-layer heads at the reference's widths in fp32 and in bf16, upstream gradients on the three
residuals and on `state`, gradients to the feature, the opacity head's output, temporal_pos and the heads' parameters:
    full        temporal_gate + the heads on P rows
    selected    temporal_rows (the plan and its read-back included) + gather(feature, time_emb) + the heads on n rows + scatter(residuals)
The claims, each recorded as "holds" / "does NOT hold" with its numbers:
    (a) at 0.7 alive the selected heads step is below the full step of the same run, at both precisions, both sizes and both placements
    (b) each fused primitive (gather, scatter; forward + backward) is below torch's indexing, at every size, fraction and placement
and the ratio selected / full at 1.0 alive: the price of selecting when nothing is dead.
One JSON object on stdout (kept as profiles/select_overhead.json).

usage: python tools/select_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000]"""
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

HEADS = {"motion": 3, "rot": 7, "shs": 48}      # 41 -> 128 -> 128 -> d_out (scene/saro_gaussian.py:104-110)
CASES = (("all", 1.0), ("random", 0.7), ("runs256", 0.7), ("random", 0.3), ("runs256", 0.3))
T, MIN_SCALE = 0.5, 0.01


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    a = ap.parse_args()
    import fused_densify
    import fused_mlp
    import fused_temporal
    dev = torch.device("cuda:0")
    result = {"steps": a.steps, "warmup": a.warmup, "heads": HEADS, "sizes": {}}

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

    for P in (int(x) for x in a.sizes.split(",")):
        torch.manual_seed(0)
        res = {"P": P, "cases": {}}
        seqs = {k: nn.Sequential(nn.Linear(41, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, d)).to(dev) for k, d in HEADS.items()}
        heads = {p: {k: fused_mlp.FusedMLP3.from_sequential(s, precision=p) for k, s in seqs.items()} for p in ("fp32", "bf16")}
        feature = torch.randn(P, 32, device=dev, requires_grad=True)
        head = torch.rand(P, 1, device=dev, requires_grad=True)
        d_state = torch.randn(P, 1, device=dev)
        d_res = {k: torch.randn(P, d, device=dev) for k, d in HEADS.items()}
        leaves = [feature, head]

        def clear():
            for x in leaves:
                x.grad = None
            for s in seqs.values():
                s.zero_grad(set_to_none=True)

        def full_step(precision, pos):
            def run():
                clear()
                pos.grad = None
                _, state, emb = fused_temporal.temporal_gate(head, pos, T, min_scale=MIN_SCALE)
                out = [heads[precision][k](feature, emb) for k in HEADS]
                torch.autograd.backward(out + [state], [d_res[k] for k in HEADS] + [d_state])
            return run

        def selected_step(precision, pos):
            def run():
                clear()
                pos.grad = None
                sel, _, state, emb = fused_temporal.temporal_rows(head, pos, T, min_scale=MIN_SCALE)
                feat_n, emb_n = sel.gather(feature, emb)
                out = sel.scatter(*[heads[precision][k](feat_n, emb_n) for k in HEADS])
                torch.autograd.backward(list(out) + [state], [d_res[k] for k in HEADS] + [d_state])
            return run

        for layout, frac in CASES:
            if layout == "runs256":
                alive = (torch.rand((P + 255) // 256, device=dev) < frac).repeat_interleave(256)[:P]
            else:
                alive = torch.rand(P, device=dev) < frac if frac < 1.0 else torch.ones(P, dtype=torch.bool, device=dev)
            # alive rows sit on the timestamp (state 1), dead rows two lifespans or more away (state <= e^-16)
            pos = torch.where(alive, torch.full((P,), T, device=dev), torch.full((P,), T + 2.0, device=dev)).reshape(P, 1).requires_grad_(True)
            sel = fused_densify.select_rows(keep=alive)
            n, rows = sel.count, alive.nonzero().reshape(-1)
            r = {"layout": layout, "alive_fraction": frac, "n": n}
            # ---- primitives
            emb = torch.randn(P, 9, device=dev, requires_grad=True)
            g_feat, g_emb = torch.randn(n, 32, device=dev), torch.randn(n, 9, device=dev)
            ys = [torch.randn(n, d, device=dev, requires_grad=True) for d in HEADS.values()]

            def gather_fused():
                feature.grad = emb.grad = None
                torch.autograd.backward(sel.gather(feature, emb), (g_feat, g_emb))

            def gather_torch():
                feature.grad = emb.grad = None
                torch.autograd.backward((feature[rows], emb[rows]), (g_feat, g_emb))

            def scatter_fused():
                for y in ys:
                    y.grad = None
                torch.autograd.backward(sel.scatter(*ys), [d_res[k] for k in HEADS])

            def scatter_torch():
                for y in ys:
                    y.grad = None
                out = [torch.zeros(P, y.shape[1], device=dev).index_copy_(0, rows, y) for y in ys]
                torch.autograd.backward(out, [d_res[k] for k in HEADS])

            for name, fn in (("gather_fused", gather_fused), ("gather_torch", gather_torch), ("scatter_fused", scatter_fused), ("scatter_torch", scatter_torch),
                             ("select_fused", lambda: fused_densify.select_rows(keep=alive)), ("select_torch", lambda: alive.nonzero())):
                r[name + "_ms"] = timed(fn)
            r["primitives_fused_ms"] = round(r["gather_fused_ms"] + r["scatter_fused_ms"], 4)
            r["primitives_torch_ms"] = round(r["gather_torch_ms"] + r["scatter_torch_ms"], 4)
            del emb, g_feat, g_emb, ys
            # ---- the heads step
            for p in ("fp32", "bf16"):
                r[f"full_{p}_ms"] = timed(full_step(p, pos))
                r[f"selected_{p}_ms"] = timed(selected_step(p, pos))
                r[f"selected_over_full_{p}"] = round(r[f"selected_{p}_ms"] / r[f"full_{p}_ms"], 4)
            clear()
            res["cases"][f"{layout}_{frac}"] = r
            del pos, sel, rows, alive
            torch.cuda.empty_cache()
        result["sizes"][str(P)] = res
        del seqs, heads, feature, head, d_state, d_res, leaves
        torch.cuda.empty_cache()

    every = [(P, k, c) for P, s in result["sizes"].items() for k, c in s["cases"].items()]
    word = lambda ok: "holds" if ok else "does NOT hold"  # noqa: E731
    at07 = [(P, k, c) for P, k, c in every if c["alive_fraction"] == 0.7]
    a_ok = {p: all(c[f"selected_{p}_ms"] < c[f"full_{p}_ms"] for _, _, c in at07) for p in ("fp32", "bf16")}
    result["claims"] = {
        "a_selected_heads_step_below_full_at_0.7_alive": {
            "verdict": word(all(a_ok.values())), "fp32": word(a_ok["fp32"]), "bf16": word(a_ok["bf16"]),
            "numbers": {f"{P}_{k}": {p: [c[f"selected_{p}_ms"], c[f"full_{p}_ms"]] for p in ("fp32", "bf16")} for P, k, c in at07}},
        "b_fused_primitives_below_torch_indexing": {
            "verdict": word(all(c[f"{m}_fused_ms"] < c[f"{m}_torch_ms"] for _, _, c in every for m in ("gather", "scatter"))),
            "gather": word(all(c["gather_fused_ms"] < c["gather_torch_ms"] for _, _, c in every)),
            "scatter": word(all(c["scatter_fused_ms"] < c["scatter_torch_ms"] for _, _, c in every)),
            "numbers": {f"{P}_{k}": {m: [c[f"{m}_fused_ms"], c[f"{m}_torch_ms"]] for m in ("gather", "scatter")} for P, k, c in every}},
        "selected_over_full_at_1.0_alive": {f"{P}": {p: c[f"selected_over_full_{p}"] for p in ("fp32", "bf16")} for P, k, c in every if c["alive_fraction"] == 1.0},
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
