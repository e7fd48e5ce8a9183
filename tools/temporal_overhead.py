"""What the temporal-lifespan calls (fused_temporal.py) cost beside a torch restatement of the reference's ops, timed in the same process:
device-synchronised medians at P = 1 M and 3 M, multires 4, min_scale 0.01.  Per size, in this order:
    gate_fwd_fused / gate_fwd_torch          temporal_gate under no_grad  against  get_deformation's lifespan, distance, survival state,
                                             time_emb(distance) AND time_emb(0) (the reference embeds twice per view)
    gate_fwdbwd_fused / gate_fwdbwd_torch    the same with autograd: forward + backward to the head and temporal_pos
    integral_fused / integral_torch          temporal_integral  against  get_intergral, the valid mask, I[valid], 1 / I, / min
    select_fused / select_torch              temporal_select over feature [P,32], xyz, rotation, scaling, opacity, f_dc, f_rest (+ state and
                                             time_emb: 101 floats per row, about 70 % alive)  against  get_deformation_eval's ops: the gate, the
                                             cat, and its boolean indexings of deform_feature, state and the six parameter tensors
and the kernels alone, from device events around the C calls: gate forward (with the `dead` output: 8 B read + 45 B written per row, as
GB/s of those 53 B), gate backward, integral.  The two conditions the README states, each recorded as it came out:
(a) gate_fwdbwd_fused < gate_fwdbwd_torch, (b) select_fused < select_torch, at both sizes.
One JSON object on stdout (kept as profiles/temporal_overhead.json).

usage: python tools/temporal_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000]"""
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

MULTIRES, MIN_SCALE, T, MIN_INTEGRAL, ALIVE = 4, 0.01, 0.5, 0.0025, 0.7
A1, A2 = 0.070565902, 1.5976


def torch_embed(x):
    out = [x]
    for f in (2.0 ** k for k in range(MULTIRES)):
        out += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(out, -1)


def torch_gate(head, pos):
    """get_deformation :782-795 (the ops between the opacity head and the other heads)."""
    lifespan = 1 - head
    lifespan = (1 - MIN_SCALE) * lifespan + MIN_SCALE
    distance = T - pos
    state = torch.exp(-4 * (distance / lifespan) ** 2)
    emb = torch_embed(distance).detach()
    base = torch_embed(torch.zeros_like(distance)).detach()
    return lifespan, state, emb, base


def torch_integral(head, pos):
    """get_intergral :761-777 and update_learning_rate :350-356 (without the prune itself)."""
    lifespan = (1 - MIN_SCALE) * (1 - head) + MIN_SCALE
    q = lambda x: 1 - 1 / (1 + torch.exp(A1 * x ** 3 + A2 * x))  # noqa: E731
    integral = lifespan * math.sqrt(math.pi) / 2 * (q(2 * math.sqrt(2) * (1.0 - pos) / lifespan) - q(2 * math.sqrt(2) * (0.0 - pos) / lifespan))
    valid = (integral > MIN_INTEGRAL).squeeze()
    inv = 1 / integral[valid]
    return integral, ~valid, inv / inv.min()


def torch_select(lifespan, pos, feature, params):
    """get_deformation_eval :872-914 up to the heads."""
    distance = T - pos
    state = torch.exp(-4 * (distance / lifespan) ** 2)
    deform_feature = torch.cat((feature, torch_embed(distance)), 1)
    mask = state > 0.001
    out = [deform_feature[mask.squeeze()], state[mask.squeeze()]]
    return out + [p[mask.squeeze()] for p in params]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_temporal as ft
    _C = rast._C
    dev = torch.device("cuda:0")
    result = {"steps": a.steps, "warmup": a.warmup, "multires": MULTIRES, "min_scale": MIN_SCALE, "select_floats_per_row": 101, "sizes": {}}

    def timed(run):
        ms = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]

    def kernel_ms(call):
        """Median device time of one C call, from events on the current stream."""
        ms = []
        for it in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0, _C.lib().gsrast_last_error()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return round(statistics.median(ms), 4)

    for P in (int(x) for x in a.sizes.split(",")):
        torch.manual_seed(0)
        head = torch.rand(P, 1, device=dev)
        L = (1 - MIN_SCALE) * (1 - head) + MIN_SCALE
        alive = torch.rand(P, 1, device=dev) < ALIVE
        pos = torch.where(alive, T + 0.5 * L * (2 * torch.rand(P, 1, device=dev) - 1), torch.full_like(L, T + 2.0))      # state >= e^-1, or <= e^-16
        pos_train = torch.rand(P, 1, device=dev) * 1.4 - 0.2
        shapes = ((3,), (4,), (3,), (1,), (1, 3), (15, 3))
        params = [torch.randn((P,) + s, device=dev) for s in shapes]
        feature = torch.randn(P, 32, device=dev)
        d_l, d_s = torch.randn(P, 1, device=dev), torch.randn(P, 1, device=dev)
        hg, pg = head.clone().requires_grad_(True), pos_train.clone().requires_grad_(True)

        def fwdbwd(gate):
            hg.grad = pg.grad = None
            out = gate(hg, pg)
            torch.autograd.backward((out[0], out[1]), (d_l, d_s))

        fused_gate = lambda h, p: ft.temporal_gate(h, p, T, min_scale=MIN_SCALE, multires=MULTIRES)  # noqa: E731
        res = {"P": P}
        with torch.no_grad():
            res["alive_fraction"] = round(float((torch_gate(head, pos)[1] > 0.001).float().mean()), 4)
            legs = {
                "gate_fwd_fused": lambda: fused_gate(head, pos_train),
                "gate_fwd_torch": lambda: torch_gate(head, pos_train),
                "integral_fused": lambda: ft.temporal_integral(head, pos_train, min_scale=MIN_SCALE, min_integral=MIN_INTEGRAL),
                "integral_torch": lambda: torch_integral(head, pos_train),
                "select_fused": lambda: ft.temporal_select(head, pos, T, [feature] + params, min_scale=MIN_SCALE, multires=MULTIRES),
                "select_torch": lambda: torch_select(L, pos, feature, params),
            }
            for name, run in legs.items():
                res[f"{name}_ms"], res[f"{name}_spread_ms"] = timed(run)
        for name, gate in (("gate_fwdbwd_fused", fused_gate), ("gate_fwdbwd_torch", torch_gate)):
            res[f"{name}_ms"], res[f"{name}_spread_ms"] = timed(lambda g=gate: fwdbwd(g))
        for leg in ("gate_fwd", "gate_fwdbwd", "integral", "select"):
            res[f"{leg}_fused_over_torch"] = round(res[f"{leg}_fused_ms"] / res[f"{leg}_torch_ms"], 4)
        res["a_gate_fwdbwd_fused_below_torch"] = bool(res["gate_fwdbwd_fused_ms"] < res["gate_fwdbwd_torch_ms"])
        res["b_select_fused_below_torch"] = bool(res["select_fused_ms"] < res["select_torch_ms"])
        # the kernels alone
        lib, s = _C.lib(), torch.cuda.current_stream(dev).cuda_stream
        h, c = head.reshape(-1), pos_train.reshape(-1).contiguous()
        o = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
        life, state, emb, dead = o(P), o(P), o(P, 2 * MULTIRES + 1), torch.empty(P, dtype=torch.uint8, device=dev)
        g_h, g_c, integral, inv, stats = o(P), o(P), o(P), o(P), torch.empty(2, dtype=torch.int32, device=dev)
        res["kernels_ms"] = {
            "gate_fwd": kernel_ms(lambda: lib.gsrast_temporal_gate_forward(P, MULTIRES, 0, T, MIN_SCALE, 0.001, h.data_ptr(), c.data_ptr(), life.data_ptr(),
                                                                           state.data_ptr(), emb.data_ptr(), dead.data_ptr(), s)),
            "gate_bwd": kernel_ms(lambda: lib.gsrast_temporal_gate_backward(P, 0, T, MIN_SCALE, h.data_ptr(), c.data_ptr(), d_l.data_ptr(), d_s.data_ptr(),
                                                                            g_h.data_ptr(), g_c.data_ptr(), s)),
            "integral": kernel_ms(lambda: lib.gsrast_temporal_integral(P, 0, 0.0, 1.0, MIN_SCALE, MIN_INTEGRAL, h.data_ptr(), c.data_ptr(), integral.data_ptr(),
                                                                       dead.data_ptr(), inv.data_ptr(), stats.data_ptr(), s)),
        }
        res["gate_fwd_GBps"] = round(P * 53 / (res["kernels_ms"]["gate_fwd"] * 1e-3) / 1e9, 1)
        result["sizes"][str(P)] = res
        del head, L, alive, pos, pos_train, params, feature, d_l, d_s, hg, pg, legs, life, state, emb, dead, g_h, g_c, integral, inv, stats
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
