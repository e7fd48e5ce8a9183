"""What the bilateral-grid colour correction (fused_bilagrid.py) costs beside a torch restatement (F.grid_sample + einsum, and its autograd)
and beside the fused loss it feeds, timed in the same process: device-synchronised medians at 1352 x 1014 and 1920 x 1080 with the
16 x 16 x 8 grid, each on a smooth (render-like) image and on per-pixel noise (the gather's worst case).  Per size and image, in this order:
    fwd_fused / fwd_torch              bilagrid_apply under no_grad  against  the restatement under no_grad
    fwdbwd_fused / fwdbwd_torch        forward + backward to the grid and the image
    loss_fwdbwd                        fused_loss.l1_dssim_loss forward + backward of the same image
and the kernels alone, from device events around the C calls: forward, backward pixel pass (dL/dimage only), backward grid pass
(dL/dgrid only: the gather and, with more than one slab, its reduce) at the library's slab count and at forced ones, and the TV value and
gradient launches for 20 cameras.  The two claims the README states, each recorded as it came out:
(a) fwdbwd_fused < fwdbwd_torch, (b) fwdbwd_fused < loss_fwdbwd; a_holds / b_holds: at both sizes on both images.
--accuracy-log: the -s output of tests/test_gpu_bilagrid.py; its summary lines' worst e_hip / bar per tensor are copied into the result.
One JSON object, written to --out (kept as profiles/bilagrid_overhead.json) and printed.

usage: python tools/bilagrid_overhead.py [--steps 20] [--warmup 3] [--sizes 1352x1014,1920x1080] [--accuracy-log LOG] [--out PATH]"""
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

GRID = (16, 16, 8)      # GW, GH, L
TV_CAMERAS = 20
FORCED_SPLITS = (1, 2, 4, 8, 16, 32)


def torch_apply(grid, image):
    H, W = image.shape[1:]
    x = (torch.arange(W, dtype=image.dtype, device=image.device) + 0.5) / W
    y = (torch.arange(H, dtype=image.dtype, device=image.device) + 0.5) / H
    gray = 0.299 * image[0] + 0.587 * image[1] + 0.114 * image[2]
    coords = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), gray], -1)
    A = F.grid_sample(grid[None], (2.0 * coords - 1.0)[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(3, 4, H, W)
    return torch.einsum("ckhw,khw->chw", A[:, :3], image) + A[:, 3]


def accuracy_from(log_path):
    """{tensor: worst e_hip / bar} over the summary lines `bilagrid <case> <tensor>: worst e_hip / bar <ratio> ...` of a test log"""
    worst = {}
    for m in re.finditer(r"^\.*bilagrid .*? (\w+): worst e_hip / bar ([0-9.]+)", open(log_path).read(), flags=re.M):
        worst[m.group(1)] = max(worst.get(m.group(1), 0.0), float(m.group(2)))
    return worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1352x1014,1920x1080")
    ap.add_argument("--accuracy-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilagrid_overhead.json"))
    a = ap.parse_args()
    import diff_gaussian_rasterization_ch3 as rast
    import fused_bilagrid as fb
    import fused_loss
    _C = rast._C
    dev = torch.device("cuda:0")
    GW, GH, L = GRID
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "grid": {"GW": GW, "GH": GH, "L": L}, "sizes": {}}

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

    lib, s = _C.lib(), torch.cuda.current_stream(dev).cuda_stream

    def make_image(kind, W, H):
        """smooth: low-frequency waves + 2 % noise, as a render is (neighbouring pixels share their luminance slice); noise: every pixel
        its own uniform draw in [-0.1, 1.1] -- the worst case of the gather, whose lanes then take all L slice branches."""
        if kind == "noise":
            return torch.rand(3, H, W, device=dev) * 1.2 - 0.1
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
        base = torch.stack([0.5 + 0.45 * torch.sin(7.0 * xx + 3.0 * yy + c) * torch.cos(5.0 * yy - 2.0 * xx + 0.5 * c) for c in range(3)])
        return (base + 0.02 * torch.randn(3, H, W, device=dev)).contiguous()

    for W, H, kind in ((*(int(v) for v in size.split("x")), kind) for size in a.sizes.split(",") for kind in ("smooth", "noise")):
        torch.manual_seed(0)
        grid = (fb.identity_grids(1, GW, GH, L)[0] + 0.1 * torch.randn(12, L, GH, GW)).to(dev)
        image, gt, d_out = make_image(kind, W, H), torch.rand(3, H, W, device=dev), torch.randn(3, H, W, device=dev)
        gg, ig = grid.clone().requires_grad_(True), image.clone().requires_grad_(True)

        def fwdbwd(apply):
            gg.grad = ig.grad = None
            apply(gg, ig).backward(d_out)

        def loss_fwdbwd():
            ig.grad = None
            fused_loss.l1_dssim_loss(ig, gt, 0.2).backward()

        res = {"W": W, "H": H, "image": kind}
        with torch.no_grad():
            res["fwd_fused_ms"], res["fwd_fused_spread_ms"] = timed(lambda: fb.bilagrid_apply(grid, image))
            res["fwd_torch_ms"], res["fwd_torch_spread_ms"] = timed(lambda: torch_apply(grid, image))
            res["max_abs_fused_minus_torch"] = float((fb.bilagrid_apply(grid, image) - torch_apply(grid, image)).abs().max())
        for name, run in (("fwdbwd_fused", lambda: fwdbwd(fb.bilagrid_apply)), ("fwdbwd_torch", lambda: fwdbwd(torch_apply)), ("loss_fwdbwd", loss_fwdbwd)):
            res[f"{name}_ms"], res[f"{name}_spread_ms"] = timed(run)
        for leg in ("fwd", "fwdbwd"):
            res[f"{leg}_fused_over_torch"] = round(res[f"{leg}_fused_ms"] / res[f"{leg}_torch_ms"], 4)
        res["a_fwdbwd_fused_below_torch"] = bool(res["fwdbwd_fused_ms"] < res["fwdbwd_torch_ms"])
        res["b_fwdbwd_fused_below_loss_fwdbwd"] = bool(res["fwdbwd_fused_ms"] < res["loss_fwdbwd_ms"])
        # the kernels alone
        out, d_image, d_grid = torch.empty_like(image), torch.empty_like(image), torch.empty_like(grid)

        def grid_pass(splits):
            desc = _C.BilagridStruct(GW, GH, L, W, H, 0, 0, W, H, splits)
            nbytes = lib.gsrast_bilagrid_scratch_bytes(desc)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ms = kernel_ms(lambda: lib.gsrast_bilagrid_backward(desc, grid.data_ptr(), image.data_ptr(), d_out.data_ptr(), None, d_grid.data_ptr(), scratch.data_ptr(), s))
            return ms, (nbytes - 256) // (12 * L * GH * GW * 4)

        desc0 = _C.BilagridStruct(GW, GH, L, W, H, 0, 0, W, H, 0)
        auto_ms, auto_slabs = grid_pass(0)
        res["kernels_ms"] = {
            "fwd": kernel_ms(lambda: lib.gsrast_bilagrid_forward(desc0, grid.data_ptr(), image.data_ptr(), out.data_ptr(), s)),
            "bwd_pixel": kernel_ms(lambda: lib.gsrast_bilagrid_backward(desc0, grid.data_ptr(), image.data_ptr(), d_out.data_ptr(), d_image.data_ptr(), None, None, s)),
            "bwd_grid": auto_ms,
            "bwd_grid_by_splits": {str(k): grid_pass(k)[0] for k in FORCED_SPLITS},
        }
        res["bwd_grid_slabs_chosen"] = int(auto_slabs) if auto_slabs else 1
        res["fwd_GBps"] = round(W * H * 24 / (res["kernels_ms"]["fwd"] * 1e-3) / 1e9, 1)      # 12 B read + 12 B written per pixel
        result["sizes"][f"{W}x{H} {kind}"] = res
    # the regulariser over 20 cameras' grids
    grids = (fb.identity_grids(TV_CAMERAS, GW, GH, L) + 0.1 * torch.randn(TV_CAMERAS, 12, L, GH, GW)).to(dev)
    value, up, d_grids = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(grids)
    result["tv"] = {"cameras": TV_CAMERAS, "kernels_ms": {
        "value": kernel_ms(lambda: lib.gsrast_bilagrid_tv(TV_CAMERAS, GW, GH, L, grids.data_ptr(), value.data_ptr(), None, None, s)),
        "gradient": kernel_ms(lambda: lib.gsrast_bilagrid_tv(TV_CAMERAS, GW, GH, L, grids.data_ptr(), None, up.data_ptr(), d_grids.data_ptr(), s))}}
    result["a_holds"] = all(r["a_fwdbwd_fused_below_torch"] for r in result["sizes"].values())
    result["b_holds"] = all(r["b_fwdbwd_fused_below_loss_fwdbwd"] for r in result["sizes"].values())
    if a.accuracy_log:
        result["worst_e_hip_over_bar"] = accuracy_from(a.accuracy_log)
    text = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
