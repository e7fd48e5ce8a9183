"""Bilateral-grid colour correction, host side (no GPU): tests/bilagrid_math.py against torch.autograd of the fp64 F.grid_sample
composition it restates, the identity grid, the C ABI of gsrast_bilagrid_* (declared, exported, bound, every argument error refused
before any device call, the scratch size) and the Python module's bookkeeping and refusals.

There is no golden file: gsplat is not a dependency of the project, so the restatement is pinned to the definition in include/gsrast.h
and to torch's own grid_sample."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bilagrid_math as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = [(1, 1, None), (7, 5, None), (37, 53, None), (37, 53, (11, 20, 120, 90))]      # (W, H, window)
# the profile table as it stood before this feature (its last names are pinned by tests/test_mlp_bf16_host.py as well)
PROFILE_TAIL = ["mcmc_plan", "mcmc_sample", "mcmc_apply", "mcmc_noise", "mlp_fwd", "mlp_bwd"]


@pytest.mark.parametrize("W,H,window", IMAGES)
@pytest.mark.parametrize("GW,GH,L", bm.GRIDS)
def test_restatement_equals_autograd_in_fp64(GW, GH, L, W, H, window):
    c = bm.make_case(GW, GH, L, W, H, seed=GW + 10 * L + W)
    want = bm.torch_run(c["grid"], c["image"], c["d_out"], window, torch.float64)
    d_grid, d_image = bm.backward(c["grid"], c["image"], c["d_out"], window)
    got = dict(out=bm.forward(c["grid"], c["image"], window), d_grid=d_grid, d_image=d_image)
    for k, w in want.items():
        assert got[k].shape == w.shape and np.abs(got[k] - w).max() <= 1e-12, k
    # the clamped pixels take no guidance gradient: there d image is the matrix product alone
    gray = np.tensordot(bm.GRAY, c["image"].astype(np.float64), 1)
    if L > 1 and W * H >= 64:
        assert ((gray < 0) | (gray > 1)).any() and ((gray > 0) & (gray < 1)).any()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("GW,GH,L", bm.GRIDS)
def test_tv_restatement_equals_autograd_in_fp64(GW, GH, L, N):
    grids = bm.make_grids(N, GW, GH, L, seed=GW + L + N)
    want = bm.torch_tv_run(grids, torch.float64)
    assert abs(bm.tv(grids) - float(want["tv"])) <= 1e-12
    assert np.abs(bm.tv_grad(grids) - want["d_tv"]).max() <= 1e-12
    if (GW, GH, L) == (1, 1, 1):
        assert bm.tv(grids) == 0.0 and not bm.tv_grad(grids).any()      # every axis has one vertex


@pytest.mark.parametrize("GW,GH,L", bm.GRIDS)
def test_identity_grid_reproduces_the_image_and_has_no_variation(GW, GH, L):
    """to one fp64 epsilon (2.2e-16): the eight weights sum to 1 within a rounding, the image is below 2 in magnitude"""
    eps = float(np.finfo(np.float64).eps)
    ident = bm.identity_grid(GW, GH, L)
    for W, H, window in IMAGES:
        image = bm.make_case(GW, GH, L, W, H, seed=5)["image"]
        assert np.abs(bm.forward(ident, image, window) - image.astype(np.float64)).max() <= eps, (W, H, window)
        assert np.abs(bm.torch_apply(torch.tensor(ident).double(), torch.tensor(image).double(), window).numpy() - image).max() <= eps, (W, H, window)
    assert bm.tv(ident[None]) == 0.0 and not bm.tv_grad(ident[None]).any()


def test_symbols_are_declared_exported_and_bound(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    assert C.sizeof(rast._C.BilagridStruct) == 40
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert len(names) == 34 and names[-6:] == PROFILE_TAIL and not any("bilagrid" in n for n in names)      # the profile table is unchanged


def _desc(rast, **kw):
    d = dict(GW=16, GH=16, L=8, W=64, H=48, x0=0, y0=0, full_W=64, full_H=48, splits=0)
    d.update(kw)
    return rast._C.BilagridStruct(*(d[f] for f, _ in rast._C.BilagridStruct._fields_))


BAD_DESCRIPTORS = [
    (dict(GW=0), "GW and GH must be in [1, 64]"), (dict(GW=65), "GW and GH must be in [1, 64]"), (dict(GH=0), "GW and GH must be in [1, 64]"),
    (dict(GH=65), "GW and GH must be in [1, 64]"), (dict(GW=-3), "GW and GH must be in [1, 64]"),
    (dict(L=0), "L must be in [1, 16]"), (dict(L=17), "L must be in [1, 16]"),
    (dict(W=0), "W and H must be >= 1"), (dict(H=0), "W and H must be >= 1"), (dict(H=-1), "W and H must be >= 1"),
    (dict(full_W=0), "full_W and full_H must be in [1, 32768]"), (dict(full_H=40000, H=48), "full_W and full_H must be in [1, 32768]"),
    (dict(x0=-1), "the window must lie inside the frame"), (dict(y0=-1), "the window must lie inside the frame"),
    (dict(x0=1), "the window must lie inside the frame"), (dict(y0=1), "the window must lie inside the frame"),
    (dict(full_W=63), "the window must lie inside the frame"), (dict(x0=2**31 - 10, full_W=32768), "the window must lie inside the frame"),
    (dict(splits=-1), "splits must be in [0, 1024]"), (dict(splits=1025), "splits must be in [0, 1024]"),
]


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    L = rast._C.lib()
    one = 256      # any non-NULL value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731

    def fwd(d, grid=one, image=one, out=one):
        return L.gsrast_bilagrid_forward(d, grid, image, out, None)

    def bwd(d, grid=one, image=one, dout=one, dimage=one, dgrid=one, scratch=one):
        return L.gsrast_bilagrid_backward(d, grid, image, dout, dimage, dgrid, scratch, None)

    for who, call in (("bilagrid_forward", fwd), ("bilagrid_backward", bwd)):
        assert call(None) == -1 and who in err() and "NULL descriptor" in err()
        for bad, text in BAD_DESCRIPTORS:
            assert call(_desc(rast, **bad)) == -1 and who in err() and text in err(), (who, bad, err())
        for p in ("grid", "image"):
            assert call(_desc(rast), **{p: None}) == -1 and who in err() and "NULL required pointer" in err(), p
    assert fwd(_desc(rast), out=None) == -1 and "NULL required pointer" in err()
    assert bwd(_desc(rast), dout=None) == -1 and "NULL required pointer" in err()
    assert bwd(_desc(rast), dimage=None, dgrid=None) == -1 and "both NULL" in err()
    assert bwd(_desc(rast, splits=2), scratch=None) == -1 and "NULL scratch" in err()
    # scratch_bytes: 0 and the reason for a refused descriptor
    assert L.gsrast_bilagrid_scratch_bytes(None) == 0 and "bilagrid_scratch_bytes" in err() and "NULL descriptor" in err()
    for bad, text in BAD_DESCRIPTORS:
        assert L.gsrast_bilagrid_scratch_bytes(_desc(rast, **bad)) == 0 and text in err(), bad

    def tv(N=2, GW=16, GH=16, Lg=8, grids=one, loss=one, up=one, dg=one):
        return L.gsrast_bilagrid_tv(N, GW, GH, Lg, grids, loss, up, dg, None)

    for bad, text in ((dict(N=0), "N must be in [1, 2048]"), (dict(N=-1), "N must be in [1, 2048]"), (dict(N=2049), "N must be in [1, 2048]"),
                      (dict(GW=0), "GW and GH must be in [1, 64]"), (dict(GH=65), "GW and GH must be in [1, 64]"), (dict(Lg=0), "L must be in [1, 16]"),
                      (dict(Lg=17), "L must be in [1, 16]"), (dict(grids=None), "NULL required pointer"), (dict(loss=None, dg=None), "both NULL")):
        assert tv(**bad) == -1 and "bilagrid_tv" in err() and text in err(), bad


def test_scratch_bytes_is_monotone_in_splits_and_needs_none_for_one_slab(rast):
    L = rast._C.lib()
    sizes = [L.gsrast_bilagrid_scratch_bytes(_desc(rast, splits=s)) for s in (1, 2, 3, 7, 64, 1024)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    n = 12 * 8 * 16 * 16 * 4
    assert sizes[0] == 256 and sizes[1] == 2 * n + 256 and sizes[3] == 7 * n + 256
    # the library's choice is a function of the descriptor alone: the same answer twice, and one of the forced sizes
    auto = L.gsrast_bilagrid_scratch_bytes(_desc(rast, W=1920, H=1080, full_W=1920, full_H=1080))
    assert auto == L.gsrast_bilagrid_scratch_bytes(_desc(rast, W=1920, H=1080, full_W=1920, full_H=1080)) and (auto - 256) % n == 0
    assert L.gsrast_bilagrid_scratch_bytes(_desc(rast, GW=1, GH=1, L=1, W=1, H=1, full_W=1, full_H=1)) == 256


def test_module_bookkeeping():
    import fused_bilagrid as fb
    m = fb.BilateralGrids(3)
    assert [k for k, _ in m.named_parameters()] == ["grids"] and list(m.state_dict()) == ["grids"]
    assert tuple(m.grids.shape) == (3, 12, 8, 16, 16) and m.grids.dtype == torch.float32 and m.grids.requires_grad
    m = fb.BilateralGrids(2, grid_x=5, grid_y=3, grid_w=4)
    assert tuple(m.grids.shape) == (2, 12, 4, 3, 5)      # [num, 12, L, GH, GW]
    A = m.grids.detach().permute(0, 2, 3, 4, 1).reshape(-1, 3, 4)
    assert torch.equal(A, torch.eye(3, 4).expand_as(A))
    assert np.array_equal(m.grids.detach()[0].numpy(), bm.identity_grid(5, 3, 4))
    for bad in (dict(num=0), dict(num=1, grid_x=65), dict(num=1, grid_y=0), dict(num=1, grid_w=17)):
        with pytest.raises(ValueError):
            fb.BilateralGrids(**bad)


def test_python_refusals_need_no_device(monkeypatch):
    import fused_bilagrid as fb
    monkeypatch.setattr(fb._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    grid, image = torch.zeros(12, 8, 16, 16), torch.zeros(3, 48, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        fb.bilagrid_apply(grid, image)
    with pytest.raises(RuntimeError, match="GPU"):
        fb.tv(grid[None])
    m = fb.BilateralGrids(2)
    with pytest.raises(RuntimeError, match="GPU"):
        m(image, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        m.tv_loss()
    with pytest.raises(IndexError):
        m(image, 2)
    # what is checked once the tensors pass for device tensors: shapes, dtype, layout, the window (the device check stubbed out)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for g, im, text in ((grid[:11], image, "12, L, GH, GW"), (grid[None], image, "12, L, GH, GW"), (grid, image[:2], r"\[3, H, W\]"),
                        (grid, image[None], r"\[3, H, W\]"), (grid, image[:, :0], r"\[3, H, W\]"), (grid.double(), image, "float32"),
                        (grid, image.half(), "float32"), (grid, image.permute(0, 2, 1), "contiguous"), (grid.transpose(2, 3), image, "contiguous"),
                        (torch.zeros(12, 17, 4, 4), image, "L must be"), (torch.zeros(12, 4, 65, 4), image, "GW and GH")):
        with pytest.raises(ValueError, match=text):
            fb.bilagrid_apply(g, im)
    for window in ((-1, 0, 64, 48), (1, 0, 64, 48), (0, 0, 63, 48), (0, 1, 64, 48), (0, 0, 40000, 48)):
        with pytest.raises(ValueError, match="window|frame"):
            fb.bilagrid_apply(grid, image, window=window)
    with pytest.raises(ValueError, match="12, L, GH, GW"):
        fb.tv(grid)
