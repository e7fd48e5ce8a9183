"""What Mip-Splatting's 3-D smoothing filter (fused_filter3d.py) costs beside a torch restatement of upstream's code, timed in the same
process: device-synchronised medians at 1 M and 3 M rows.  Per size, in this order:
    sweep_fused_C / sweep_torch_C            compute_filter_3d  against  upstream's compute_3D_filter loop (camera tensors already on the
                                             device), at C = 20 and C = 300 cameras on a ring
    apply_fwdbwd_fused / apply_fwdbwd_torch  apply_filter_3d forward + backward (gradients to scales and opacities)  against  the torch
                                             composition of get_scaling_with_3D_filter / get_opacity_with_3D_filter and its autograd
and the kernels alone, from device events around the C calls: the sweep (its clear, sweep and finish launches) at both camera counts, the
apply forward, the apply backward.  The claims the README states, recorded as they came out:
    (a) sweep_fused < sweep_torch at both camera counts and both sizes;   (b) apply_fwdbwd_fused < apply_fwdbwd_torch at both sizes.
--accuracy-log: the -s output of tests/test_gpu_filter3d.py; its `worst error / bar` lines per tensor are copied into the result.
One JSON line, written to --out (kept as profiles/filter3d_overhead.json) and printed.

usage: python tools/filter3d_overhead.py [--steps 20] [--warmup 3] [--sizes 1000000,3000000] [--cameras 20,300] [--accuracy-log LOG] [--out PATH]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


@torch.no_grad()
def torch_compute_3D_filter(xyz, cameras):
    """upstream's loop; cameras: (R, T, focal_x, focal_y, W, H) with R, T already device tensors (upstream builds them per camera per call)"""
    distance = torch.ones((xyz.shape[0]), device=xyz.device) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    focal_length = 0.
    for R, T, fx, fy, W, H in cameras:
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * fx + W / 2.0
        y = y / z * fy + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * W, x <= W * 1.15), torch.logical_and(y >= -0.15 * H, y <= 1.15 * H))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        focal_length = max(focal_length, fx)
    distance[~valid_points] = distance[valid_points].max()
    return (distance / focal_length * (0.2 ** 0.5))[..., None]


def torch_apply(scales, opacity, filter_3D):
    sq = torch.square(scales)
    after = sq + torch.square(filter_3D)
    return torch.sqrt(after), opacity * torch.sqrt(sq.prod(dim=1) / after.prod(dim=1))[..., None]


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def accuracy_from(log_path):
    worst = {}
    for m in re.finditer(r"(\w+) worst error / bar = ([0-9.]+)", open(log_path).read()):
        worst[m.group(1)] = max(worst.get(m.group(1), 0.0), float(m.group(2)))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--cameras", default="20,300")
    ap.add_argument("--accuracy-log")
    ap.add_argument("--out")
    a = ap.parse_args()
    import fused_filter3d as ff
    import scenes
    from diff_gaussian_rasterization_ch3 import _C
    dev = torch.device("cuda:0")
    res = dict(tool="filter3d_overhead", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup, sizes={})
    a_holds = b_holds = True
    for P in (int(s) for s in a.sizes.split(",")):
        r = res["sizes"][str(P)] = {}
        rng = np.random.default_rng(3)
        xyz = torch.tensor(rng.uniform(-1.3, 1.3, size=(P, 3)).astype(np.float32), device=dev)
        for C in (int(c) for c in a.cameras.split(",")):
            cams = [scenes.camera(k, C, 1352 + 16 * (k % 3), 1014, radius=2.0) for k in range(C)]
            table = ff.camera_table(cams, dev)
            upstream = [(table[c, :9].reshape(3, 3).clone(), table[c, 9:12].clone(), *(float(v) for v in table[c, 12:].tolist())) for c in range(C)]
            flt = ff.compute_filter_3d(xyz, table)
            r[f"valid_fraction_{C}"] = float(flt.valid.float().mean())
            r[f"max_rel_diff_to_torch_{C}"] = float(((flt.filter_3D - torch_compute_3D_filter(xyz, upstream)).abs() / flt.filter_3D).max())
            r[f"sweep_fused_{C}"] = median_ms(lambda: ff.compute_filter_3d(xyz, table), a.steps, a.warmup)
            r[f"sweep_torch_{C}"] = median_ms(lambda: torch_compute_3D_filter(xyz, upstream), a.steps, a.warmup)
            out, valid = torch.empty((P, 1), device=dev), torch.empty(P, dtype=torch.bool, device=dev)
            scratch = torch.empty(_C.scratch_bytes("gsrast_filter3d_scratch_bytes", P, C), dtype=torch.uint8, device=dev)
            r[f"sweep_kernels_{C}"] = event_ms(lambda: _C.launch("gsrast_filter3d_compute", dev, P, C, xyz.data_ptr(), table.data_ptr(), 0.2, 0.15, 0.2, table.focal_max,
                                                                 out.data_ptr(), valid.data_ptr(), scratch.data_ptr()), a.steps, a.warmup)
            a_holds = a_holds and r[f"sweep_fused_{C}"] < r[f"sweep_torch_{C}"]
        f3 = flt.filter_3D
        s = torch.exp(torch.tensor(rng.uniform(np.log(1e-4), 0.0, size=(P, 3)).astype(np.float32), device=dev)).requires_grad_(True)
        o = torch.tensor(rng.uniform(0.01, 0.99, size=(P, 1)).astype(np.float32), device=dev).requires_grad_(True)
        g_s, g_o = torch.randn(P, 3, device=dev), torch.randn(P, 1, device=dev)

        def step(apply):
            s.grad = o.grad = None
            torch.autograd.backward(list(apply(s, o, f3)), [g_s, g_o])

        r["apply_fwdbwd_fused"] = median_ms(lambda: step(ff.apply_filter_3d), a.steps, a.warmup)
        r["apply_fwdbwd_torch"] = median_ms(lambda: step(torch_apply), a.steps, a.warmup)
        with torch.no_grad():
            r["apply_fwd_fused"] = median_ms(lambda: ff.apply_filter_3d(s, o, f3), a.steps, a.warmup)
            r["apply_fwd_torch"] = median_ms(lambda: torch_apply(s, o, f3), a.steps, a.warmup)
        sd, od, s_f, o_f, d_s, d_o = s.detach(), o.detach(), torch.empty_like(s), torch.empty_like(o), torch.empty_like(s), torch.empty_like(o)
        r["apply_fwd_kernel"] = event_ms(lambda: _C.launch("gsrast_filter3d_apply_forward", dev, P, sd.data_ptr(), od.data_ptr(), f3.data_ptr(), s_f.data_ptr(), o_f.data_ptr()), a.steps, a.warmup)
        r["apply_bwd_kernel"] = event_ms(lambda: _C.launch("gsrast_filter3d_apply_backward", dev, P, sd.data_ptr(), od.data_ptr(), f3.data_ptr(), g_s.data_ptr(), g_o.data_ptr(),
                                                           d_s.data_ptr(), d_o.data_ptr()), a.steps, a.warmup)
        r["apply_fwd_GBps"] = P * 36 / (r["apply_fwd_kernel"] * 1e-3) / 1e9      # 20 B read, 16 B written per row
        r["apply_bwd_GBps"] = P * 52 / (r["apply_bwd_kernel"] * 1e-3) / 1e9      # 36 B read, 16 B written per row
        b_holds = b_holds and r["apply_fwdbwd_fused"] < r["apply_fwdbwd_torch"]
    res["claim_a_sweep_below_torch"] = "holds" if a_holds else "does NOT hold"
    res["claim_b_apply_below_torch"] = "holds" if b_holds else "does NOT hold"
    if a.accuracy_log:
        res["worst_error_over_bar"] = accuracy_from(a.accuracy_log)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
