"""What the normal-consistency ops (fused_normal.py) cost beside a torch restatement of the same formulas and beside the fused photometric
loss, timed in the same process: device-synchronised medians at 1352 x 1014 and 1920 x 1080 on a smooth, render-like depth and normal map
with an alpha-like weight.  Per size, in this order:
    loss_fwd_fused / loss_fwd_torch          normal_consistency_loss under no_grad  against  the restatement under no_grad
    loss_fwdbwd_fused / loss_fwdbwd_torch    forward + backward to the normal map and the depth
    l1_dssim_fwdbwd                          fused_loss.l1_dssim_loss forward + backward of the same [3, H, W] image, for scale
and the kernels alone, from device events around the C calls: depth_normal forward and backward, the loss forward (its launch and the
reduction) and the loss backward (both gradients, dL/dN alone, dL/dd alone).  gaussian_normals forward + backward at 1 M and 3 M rows
against its restatement, and its two kernels alone.  The restatement is gsplat's form: points, two slice differences, cross, F.normalize,
zero padding, with this project's two validity masks, and the mean; the reference's rotation matrix.
The claim the README states, recorded as it came out: (a) loss_fwdbwd_fused < loss_fwdbwd_torch; a_holds: at both sizes.
Not measured here: a training step's share (the render with features= and return_aux=True is timed by tools/features_overhead.py and
tools/aux_overhead.py).
--accuracy-log: the -s output of tests/test_gpu_normal.py; its summary lines' worst e_hip / bar per tensor are copied into the result.
One JSON object, written to --out (kept as profiles/normal_overhead.json) and printed.

usage: python tools/normal_overhead.py [--steps 20] [--warmup 3] [--sizes 1352x1014,1920x1080] [--rows 1000000,3000000] [--accuracy-log LOG] [--out PATH]"""
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
import torch.nn.functional as F  # noqa: E402

TANFOV_Y = 0.36      # fovy 0.69, as scenes.camera


def torch_depth_to_normal(d, tx, ty):
    H, W = d.shape
    x, y = torch.arange(W, dtype=d.dtype, device=d.device), torch.arange(H, dtype=d.dtype, device=d.device)
    u, v = ((2.0 * x + 1.0) / W - 1.0) * tx, ((2.0 * y + 1.0) / H - 1.0) * ty
    dirs = torch.stack([u[None, :].expand(H, W), v[:, None].expand(H, W), torch.ones_like(d)], dim=-1)
    points = torch.where(d > 0, d, torch.ones_like(d))[..., None] * dirs
    dx = points[2:, 1:-1, :] - points[:-2, 1:-1, :]
    dy = points[1:-1, 2:, :] - points[1:-1, :-2, :]
    c = torch.cross(dx, dy, dim=-1)
    ok = (d[2:, 1:-1] > 0) & (d[:-2, 1:-1] > 0) & (d[1:-1, 2:] > 0) & (d[1:-1, :-2] > 0) & ((c * c).sum(-1) >= 1e-24)
    n = F.normalize(torch.where(ok[..., None], c, torch.tensor([0.0, 0.0, -1.0], dtype=d.dtype, device=d.device)), dim=-1)
    n = torch.where(ok[..., None], n, torch.zeros_like(n))
    return F.pad(n, (0, 0, 1, 1, 1, 1), value=0.0).permute(2, 0, 1)


def torch_normal_loss(N, d, tx, ty, w):
    return (1.0 - w * (N * torch_depth_to_normal(d, tx, ty)).sum(0)).mean()


def torch_gaussian_normals(means3D, scales, rotations, V):
    P = means3D.shape[0]
    length = torch.sqrt((rotations * rotations).sum(1))
    ok = torch.isfinite(rotations).all(1) & (length > 0)
    q = torch.where(ok[:, None], rotations, torch.tensor([1.0, 0.0, 0.0, 0.0], device=rotations.device))
    q = q / torch.sqrt((q * q).sum(1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    n = R[torch.arange(P, device=R.device), :, torch.argmin(scales, dim=1)] @ V[:3, :3]
    p = means3D @ V[:3, :3] + V[3, :3]
    n = torch.where(((n * p).sum(1) > 0)[:, None], -n, n)
    return torch.where(ok[:, None], n, torch.zeros_like(n))


def accuracy_from(log_path):
    """{tensor: worst e_hip / bar} over the summary lines `normal <case> <tensor>: worst e_hip / bar <ratio> ...` of a test log"""
    worst = {}
    for m in re.finditer(r"^\.*normal .*? (\w+): worst e_hip / bar ([0-9.]+)", open(log_path).read(), flags=re.M):
        worst[m.group(1)] = max(worst.get(m.group(1), 0.0), float(m.group(2)))
    return worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1352x1014,1920x1080")
    ap.add_argument("--rows", default="1000000,3000000")
    ap.add_argument("--accuracy-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_overhead.json"))
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_loss
    import fused_normal as fn
    import scenes
    _C = rast._C
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "sizes": {}, "gaussians": {}}

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

    class Settings:
        def __init__(self, W, H, viewmatrix=None):
            self.image_width, self.image_height, self.tanfovx, self.tanfovy, self.viewmatrix = W, H, TANFOV_Y * W / H, TANFOV_Y, viewmatrix

    lib, s = _C.lib(), torch.cuda.current_stream(dev).cuda_stream
    for W, H in (tuple(int(v) for v in size.split("x")) for size in a.sizes.split(",")):
        torch.manual_seed(0)
        rs = Settings(W, H)
        tx, ty = rs.tanfovx, rs.tanfovy
        # smooth and render-like: low-frequency relief with 0.1 % noise, a disc of full coverage fading to an uncovered rim, the normal map
        # the surface's own normals blended with a little noise
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, device=dev), torch.linspace(-1, 1, W, device=dev), indexing="ij")
        alpha = (1.25 - (xx * xx + yy * yy)).clamp(0, 1).contiguous()
        depth = (3.0 + 0.5 * torch.sin(5.0 * xx + 2.0 * yy) * torch.cos(4.0 * yy - xx) + 0.003 * torch.randn(H, W, device=dev)) * (alpha > 0)
        depth = depth.contiguous()
        with torch.no_grad():
            N = (alpha * fn.depth_to_normal(depth, raster_settings=rs) + 0.05 * torch.randn(3, H, W, device=dev)).contiguous()
        gt = torch.rand(3, H, W, device=dev)
        Ng, dg = N.clone().requires_grad_(True), depth.clone().requires_grad_(True)

        def fwdbwd(loss_of):
            Ng.grad = dg.grad = None
            loss_of(Ng, dg).backward()

        def l1_dssim():
            Ng.grad = None
            fused_loss.l1_dssim_loss(Ng, gt, 0.2).backward()

        fused = lambda NN, dd: fn.normal_consistency_loss(NN, dd, raster_settings=rs, weight=alpha)  # noqa: E731
        plain = lambda NN, dd: torch_normal_loss(NN, dd, tx, ty, alpha)  # noqa: E731
        res = {"W": W, "H": H, "pixels_with_a_normal": float((fn.depth_to_normal(depth, raster_settings=rs) != 0).any(0).float().mean())}
        with torch.no_grad():
            res["loss_fwd_fused_ms"], res["loss_fwd_fused_spread_ms"] = timed(lambda: fused(N, depth))
            res["loss_fwd_torch_ms"], res["loss_fwd_torch_spread_ms"] = timed(lambda: plain(N, depth))
            res["loss_fused"], res["loss_torch"] = float(fused(N, depth)), float(plain(N, depth))
        for name, run in (("loss_fwdbwd_fused", lambda: fwdbwd(fused)), ("loss_fwdbwd_torch", lambda: fwdbwd(plain)), ("l1_dssim_fwdbwd", l1_dssim)):
            res[f"{name}_ms"], res[f"{name}_spread_ms"] = timed(run)
        fwdbwd(fused)
        gN, gd = Ng.grad.clone(), dg.grad.clone()
        fwdbwd(plain)
        res["max_abs_dN_fused_minus_torch"], res["max_abs_dd_fused_minus_torch"] = float((gN - Ng.grad).abs().max()), float((gd - dg.grad).abs().max())
        res["max_abs_dN"], res["max_abs_dd"] = float(gN.abs().max()), float(gd.abs().max())
        for leg in ("loss_fwd", "loss_fwdbwd"):
            res[f"{leg}_fused_over_torch"] = round(res[f"{leg}_fused_ms"] / res[f"{leg}_torch_ms"], 4)
        res["a_fwdbwd_fused_below_torch"] = bool(res["loss_fwdbwd_fused_ms"] < res["loss_fwdbwd_torch_ms"])
        # the kernels alone
        n_out, d_out, dN_out = torch.empty(3, H, W, device=dev), torch.empty(H, W, device=dev), torch.empty(3, H, W, device=dev)
        up, value = torch.ones((), device=dev), torch.empty((), device=dev)
        scratch = torch.empty(lib.gsrast_normal_loss_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr()  # noqa: E731
        res["kernels_ms"] = {
            "depth_normal_fwd": kernel_ms(lambda: lib.gsrast_depth_normal_forward(W, H, tx, ty, p(depth), p(n_out), s)),
            "depth_normal_bwd": kernel_ms(lambda: lib.gsrast_depth_normal_backward(W, H, tx, ty, p(depth), p(N), p(d_out), s)),
            "loss_fwd": kernel_ms(lambda: lib.gsrast_normal_loss_forward(W, H, tx, ty, p(N), p(depth), p(alpha), p(value), p(scratch), s)),
            "loss_bwd": kernel_ms(lambda: lib.gsrast_normal_loss_backward(W, H, tx, ty, p(N), p(depth), p(alpha), p(up), p(dN_out), p(d_out), s)),
            "loss_bwd_dN_only": kernel_ms(lambda: lib.gsrast_normal_loss_backward(W, H, tx, ty, p(N), p(depth), p(alpha), p(up), p(dN_out), None, s)),
            "loss_bwd_dd_only": kernel_ms(lambda: lib.gsrast_normal_loss_backward(W, H, tx, ty, p(N), p(depth), p(alpha), p(up), None, p(d_out), s)),
        }
        # bytes the algorithm needs: forward N + d + w read; backward the same and dN + dd written
        res["loss_fwd_GBps"] = round(W * H * 20 / (res["kernels_ms"]["loss_fwd"] * 1e-3) / 1e9, 1)
        res["loss_bwd_GBps"] = round(W * H * 36 / (res["kernels_ms"]["loss_bwd"] * 1e-3) / 1e9, 1)
        result["sizes"][f"{W}x{H}"] = res
    cam = scenes.camera(1, 6, 1920, 1080)
    V = torch.tensor(cam["viewmatrix"], device=dev)
    for P in (int(v) for v in a.rows.split(",")):
        sc = scenes.synth(P, 7)
        m, sca, q = (torch.tensor(sc[k], device=dev) for k in ("means3D", "scales", "rotations"))
        qg, g = q.clone().requires_grad_(True), torch.randn(P, 3, device=dev)
        rs = Settings(1920, 1080, V)

        def fwdbwd_g(normals_of):
            qg.grad = None
            normals_of(m, sca, qg).backward(g)

        res = {"P": P}
        res["fwdbwd_fused_ms"], res["fwdbwd_fused_spread_ms"] = timed(lambda: fwdbwd_g(lambda mm, ss, qq: fn.gaussian_normals(mm, ss, qq, raster_settings=rs)))
        res["fwdbwd_torch_ms"], res["fwdbwd_torch_spread_ms"] = timed(lambda: fwdbwd_g(lambda mm, ss, qq: torch_gaussian_normals(mm, ss, qq, V)))
        res["fwdbwd_fused_over_torch"] = round(res["fwdbwd_fused_ms"] / res["fwdbwd_torch_ms"], 4)
        n_out, dq_out = torch.empty(P, 3, device=dev), torch.empty(P, 4, device=dev)
        p = lambda t: t.data_ptr()  # noqa: E731
        res["kernels_ms"] = {"fwd": kernel_ms(lambda: lib.gsrast_gaussian_normals_forward(P, p(m), p(sca), p(q), p(V), p(n_out), s)),
                             "bwd": kernel_ms(lambda: lib.gsrast_gaussian_normals_backward(P, p(m), p(sca), p(q), p(V), p(g), p(dq_out), s))}
        res["fwd_GBps"] = round(P * 52 / (res["kernels_ms"]["fwd"] * 1e-3) / 1e9, 1)      # 40 B read + 12 B written per row
        result["gaussians"][str(P)] = res
    result["a_holds"] = all(r["a_fwdbwd_fused_below_torch"] for r in result["sizes"].values())
    result["not_measured"] = "a training step's share (the render with features= and return_aux=True is not run here)"
    if a.accuracy_log:
        result["worst_e_hip_over_bar"] = accuracy_from(a.accuracy_log)
    text = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
