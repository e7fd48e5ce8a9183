"""MCMC densification, host side (no GPU): tests/mcmc_math.py held against literal transcriptions of the formulas (relocation, sampler,
noise), the sampler's statistics, and the C ABI of gsrast_mcmc_* (declared, exported, every argument error refused before any device call)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mcmc_math as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPACITIES = (0.006, 0.1, 0.5, 0.9, 0.99)


def test_relocation_equals_the_literal_triple_loop():
    o = np.array([o for o in OPACITIES for _ in range(7)])
    count = np.array([c for _ in OPACITIES for c in (1, 2, 3, 10, 49, 50, 300)])
    on, coeff = mm.relocation(o, count)
    for s in range(o.size):
        lo, lc = mm.relocation_literal(float(o[s]), int(count[s]))
        assert abs(on[s] - lo) <= 1e-15 and abs(coeff[s] - lc) <= 1e-12 * abs(lc), (o[s], count[s])


def test_ratio_one_changes_nothing():
    """r = 1 (count 0): o' = o and denom = o, so the scale factor is 1."""
    for o in OPACITIES:
        on, coeff = mm.relocation_literal(o, 0)
        assert abs(on - o) <= 1e-15 and abs(coeff - 1.0) <= 1e-14
    on, coeff = mm.relocation(np.array(OPACITIES), np.zeros(len(OPACITIES), np.int64))
    assert np.allclose(on, OPACITIES, rtol=0, atol=1e-15) and np.allclose(coeff, 1.0, rtol=0, atol=1e-14)


def test_ratio_clamps_at_51():
    for o in OPACITIES:
        assert mm.relocation_literal(o, 50) == mm.relocation_literal(o, 51) == mm.relocation_literal(o, 100000)
        assert mm.relocation_literal(o, 49) != mm.relocation_literal(o, 50)
    a = mm.relocation(np.array(OPACITIES), np.full(len(OPACITIES), 50))
    b = mm.relocation(np.array(OPACITIES), np.full(len(OPACITIES), 7777))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_relocation_is_finite_and_lowers_the_opacity():
    for o in OPACITIES:
        for r in range(2, 52):
            on, coeff = mm.relocation_literal(o, r - 1)
            assert math.isfinite(on) and math.isfinite(coeff) and coeff > 0.0 and 0.0 < on < o, (o, r, on, coeff)


def test_new_values_clamp_and_logit():
    logit = torch.log(torch.tensor([0.006, 0.5, 0.99]) / (1 - torch.tensor([0.006, 0.5, 0.99]))).reshape(3, 1)
    scaling = torch.log(torch.tensor([[0.1, 0.2, 0.3]] * 3))
    idx, lo, ls = mm.new_values(logit, scaling, [4, 0, 2], 0.005)
    assert idx.tolist() == [0, 2]
    assert abs(float(torch.sigmoid(lo[0])) - 0.005) < 1e-12           # 1 - (1 - 0.006)^(1/5) = 0.0012 is clamped up to min_opacity
    on, coeff = mm.relocation_literal(float(mm.sigmoid(logit)[2]), 2)
    assert abs(float(torch.sigmoid(lo[1])) - on) < 1e-12 and torch.allclose(ls[1], torch.log(coeff * torch.exp(scaling[2].double())), rtol=0, atol=1e-12)


def test_integer_sampler_equals_brute_force():
    q = [0, 3, 0, 0, 1, 5, 0, 2, 0]
    W = sum(q)
    cum = np.cumsum(q)
    for t in range(W):
        want = mm.sample_brute(q, t)
        assert q[want] > 0 and int(np.searchsorted(cum, t, side="right")) == want
        # a draw whose target is t: the smallest d with floor(d * W / 2^62) = t, and the largest
        lo, hi = -((-t << 62) // W), (((t + 1) << 62) - 1) // W
        for d in {lo, hi, (lo + hi) // 2}:
            assert mm.target(d, W) == t
            assert mm.sample(q, [d])[0] == [want]


def test_zero_weight_rows_are_never_returned_and_the_ends_land_on_the_ends():
    rng = np.random.default_rng(5)
    q = rng.integers(1, mm.Q_ONE + 1, size=1200)
    q[rng.random(1200) < 0.4] = 0
    q[:3] = 0
    q[-2:] = 0
    draws = [int(d) for d in rng.integers(0, mm.DRAW_RANGE, size=5000)] + [0, mm.DRAW_RANGE - 1]
    src, count = mm.sample(q, draws)
    assert all(q[i] > 0 for i in src) and sum(count) == len(draws) and all(c == 0 for c, v in zip(count, q) if v == 0)
    positive = np.nonzero(q)[0]
    assert src[-2] == positive[0] and src[-1] == positive[-1]
    assert sum(int(v) for v in q) > 1 << 32                          # (the 64-bit prefix is what these draws walked)


def test_sampler_statistics():
    """200 000 seeded draws over 64 weights: every bin within 5 sigma of its binomial expectation (seed 2024 checked on the CPU and kept)."""
    n, bins = 200000, 64
    gen = torch.Generator().manual_seed(2024)
    o = 0.01 + 0.98 * torch.rand(bins, generator=gen, dtype=torch.float64)
    q = torch.clamp(torch.floor(o * mm.Q_ONE).long(), min=1).tolist()
    draws = torch.randint(0, mm.DRAW_RANGE, (n,), generator=gen, dtype=torch.int64).tolist()
    _, count = mm.sample(q, draws)
    W = sum(q)
    worst = 0.0
    for c, v in zip(count, q):
        p = v / W
        worst = max(worst, abs(c - n * p) / math.sqrt(n * p * (1 - p)))
    print("worst bin: %.2f sigma" % worst)
    assert worst <= 5.0


def test_noise_equals_gsplats_formula():
    gen = torch.Generator().manual_seed(3)
    P = 200
    xyz, rot, eps = torch.randn(P, 3, generator=gen), torch.randn(P, 4, generator=gen) * 3.0, torch.randn(P, 3, generator=gen)
    scaling = torch.log(0.01 + 0.5 * torch.rand(P, 3, generator=gen))
    o = torch.cat((torch.full((P // 2,), 0.001), 0.002 + 0.99 * torch.rand(P - P // 2, generator=gen)))
    logit = torch.log(o / (1 - o)).reshape(P, 1)
    a = mm.noise(xyz, rot, scaling, logit, eps, 0.37)
    b = mm.noise_gsplat(xyz, rot, scaling, logit, eps, 0.37)
    assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    assert float((a - xyz.double()).abs().max()) > 1e-3             # the step is not nothing
    rs = 1.0 + torch.rand(P, generator=gen)
    c = mm.noise(xyz, rot, scaling, logit, eps, 0.37, row_scale=rs)
    assert torch.allclose(c - xyz.double(), (a - xyz.double()) * rs.double()[:, None], rtol=1e-12, atol=1e-15)


def test_symbols_are_declared_and_exported(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    for n in ("mcmc_plan", "mcmc_sample", "mcmc_apply", "mcmc_noise"):
        assert n in names and names.index(n) < 32, n              # a bit of the "profile" option's word
    assert (rast._C.MCMC_COPY, rast._C.MCMC_OPACITY, rast._C.MCMC_SCALING) == (0, 1, 2)
    for role in ("COPY 0", "OPACITY 1", "SCALING 2"):
        assert re.search(r"#define\s+GSRAST_MCMC_" + role.replace(" ", r"\s+"), text)


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    _C = rast._C
    L = _C.lib()
    one = 256      # any non-NULL, 16-byte aligned value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    GS = _C.DensifyGroupStruct
    assert L.gsrast_mcmc_scratch_bytes(1000, 50) > 1000 * (4 + 1 + 4 + 16) and L.gsrast_mcmc_scratch_bytes(1000, 50) % 256 == 0
    assert L.gsrast_mcmc_scratch_bytes(0, 0) > 0 and L.gsrast_mcmc_scratch_bytes(-5, -5) == L.gsrast_mcmc_scratch_bytes(0, 0)

    # plan
    assert L.gsrast_mcmc_plan(-1, one, None, 0.005, one, one, one, None) == -1 and "negative P" in err()
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        assert L.gsrast_mcmc_plan(10, one, None, bad, one, one, one, None) == -1 and "min_opacity must be in [0, 1)" in err()
    assert L.gsrast_mcmc_plan(10, one, None, 0.005, one, None, one, None) == -1 and "NULL scratch" in err()
    assert L.gsrast_mcmc_plan(10, one, None, 0.005, one, one, None, None) == -1 and "counts" in err()
    assert L.gsrast_mcmc_plan(10, None, None, 0.005, one, one, one, None) == -1 and "NULL opacity_logit" in err()
    assert L.gsrast_mcmc_plan(10, one, None, 0.005, None, one, one, None) == -1 and "weights_out" in err()

    # sample
    assert L.gsrast_mcmc_sample(-1, 5, one, one, one, None, None) == -1 and "negative" in err()
    assert L.gsrast_mcmc_sample(10, -5, one, one, one, None, None) == -1 and "negative" in err()
    assert L.gsrast_mcmc_sample(10, 5, one, None, one, None, None) == -1 and "NULL scratch" in err()
    assert L.gsrast_mcmc_sample(10, 5, None, one, one, None, None) == -1 and "NULL draws" in err()
    assert L.gsrast_mcmc_sample(10, 5, one, one, None, None, None) == -1 and "src_out" in err()
    assert L.gsrast_mcmc_sample(0, 0, None, one, None, None, None) == 0

    # relocate / grow
    def groups(*g):
        return (GS * max(len(g), 1))(*g), len(g)

    def grp(width=3, role=_C.MCMC_COPY, dst=one, src=None, moments=True):
        m = one if moments else None
        return GS(src, m if src else None, m if src else None, dst, m, m, width, role)

    ok_counts = (C.c_uint * 4)(4, 6, 6 << 20, 0)
    full = [grp(1, _C.MCMC_OPACITY), grp(3, _C.MCMC_SCALING), grp(4), grp(45)]
    for fn, name in ((L.gsrast_mcmc_relocate, "mcmc_relocate"), (L.gsrast_mcmc_grow, "mcmc_grow")):
        grow = name == "mcmc_grow"
        mk = (lambda *a, **k: grp(*a, src=one, **k)) if grow else grp
        base = [mk(1, _C.MCMC_OPACITY), mk(3, _C.MCMC_SCALING), mk(4), mk(45)]

        def call(gs=base, P=10, n=4, src=one, scratch=one, counts=ok_counts, mo=0.005, n_groups=None):
            arr, k = groups(*gs)
            return fn(P, n, src, scratch, counts, mo, k if n_groups is None else n_groups, arr, None)

        assert call(P=-1) == -1 and name in err() and "negative" in err()
        assert call(n=-1) == -1 and "negative" in err()
        assert call(P=2**31 - 2, n=4) == -1 and "2^31" in err()
        for bad in (-0.5, 1.0):
            assert call(mo=bad) == -1 and "min_opacity must be in [0, 1)" in err()
        assert call(gs=base + [mk()] * 13) == -1 and "at most 16 groups" in err()
        assert call(n_groups=-1) == -1 and "at most 16 groups" in err()
        for w in (0, 65, -3):
            assert call(gs=base + [mk(w)]) == -1 and "width must be in [1, 64]" in err()
        assert call(gs=base + [mk(3, 7)]) == -1 and "unknown group role" in err()
        assert call(gs=[mk(2, _C.MCMC_OPACITY)] + base[1:]) == -1 and "opacity role needs width 1" in err()
        assert call(gs=[base[0], mk(4, _C.MCMC_SCALING)] + base[2:]) == -1 and "scaling role needs width 3" in err()
        assert call(gs=base + [mk(1, _C.MCMC_OPACITY)]) == -1 and "more than one" in err()
        assert call(gs=base[2:]) == -1 and "one opacity and one scaling group are required" in err()
        assert call(scratch=None) == -1 and "NULL scratch" in err()
        assert call(src=None) == -1 and "NULL scratch / groups / src" in err()
        assert fn(10, 4, one, one, ok_counts, 0.005, 2, None, None) == -1 and "NULL" in err()
        assert call(gs=base + [mk(dst=None)]) == -1 and "NULL" in err()
        assert call(counts=(C.c_uint * 4)(4, 7, 1 << 20, 0)) == -1 and "not those of a plan" in err()      # n_dead + n_alive != P
        assert call(counts=(C.c_uint * 4)(4, 6, 0, 1)) == -1 and "not those of a plan" in err()            # W above n_alive * 2^24
        assert call(counts=(C.c_uint * 4)(10, 0, 0, 0)) == -1 and "total weight of 0" in err()
        assert call(P=0, n=4, counts=(C.c_uint * 4)(0, 0, 0, 0)) == -1
        if grow:
            assert call(P=0, n=4, counts=None) == -1 and "empty model" in err()
            assert call(gs=base + [GS(one, one, one, one, None, None, 3, 0)]) == -1 and "go together" in err()
            assert call(gs=base + [GS(None, None, None, one, None, None, 3, 0)]) == -1 and "NULL src / dst" in err()
        else:
            assert call(counts=None) == -1 and "NULL counts" in err()
            assert call(n=5) == -1 and "exceeds the number of dead rows" in err()
            assert call(gs=base + [GS(512, None, None, one, None, None, 3, 0)]) == -1 and "in place" in err()
        # nothing to launch: OK without a device
        assert call(P=0, n=0, counts=(C.c_uint * 4)(0, 0, 0, 0)) == 0
        assert call(gs=[], n=0) == 0
    assert L.gsrast_mcmc_relocate(10, 0, None, one, ok_counts, 0.005, *reversed(groups(*full)), None) == 0      # no draw: relocate has nothing to do

    # noise
    assert L.gsrast_mcmc_noise(-1, one, one, one, one, one, None, 1.0, 100.0, 0.995, None) == -1 and "negative P" in err()
    for k in range(5):
        a = [one] * 5
        a[k] = None
        assert L.gsrast_mcmc_noise(10, *a, None, 1.0, 100.0, 0.995, None) == -1 and "NULL pointer" in err()
    assert L.gsrast_mcmc_noise(10, one, 260, one, one, one, None, 1.0, 100.0, 0.995, None) == -1 and "16-byte aligned" in err()
    assert L.gsrast_mcmc_noise(0, None, None, None, None, None, None, 1.0, 100.0, 0.995, None) == 0


def _cpu_optimizer(P=4):
    import fused_adam
    shapes = {"xyz": (3,), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
    ps = {k: torch.zeros((P,) + s, requires_grad=True) for k, s in shapes.items()}
    return fused_adam.GaussianAdam([{"params": [ps[k]], "lr": 1e-3, "name": k} for k in shapes], eps=1e-15), ps


def test_python_refusals_need_no_device(monkeypatch):
    import fused_densify as fd
    monkeypatch.setattr(fd._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    opt, ps = _cpu_optimizer(4)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="min_opacity"):
            fd.mcmc_relocate(opt, min_opacity=bad)
        with pytest.raises(ValueError, match="min_opacity"):
            fd.mcmc_grow(opt, cap_max=100, min_opacity=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        fd.mcmc_relocate(opt)
    with pytest.raises(RuntimeError, match="GPU"):
        fd.mcmc_grow(opt, cap_max=100)
    with pytest.raises(RuntimeError, match="GPU"):
        fd.mcmc_inject_noise(ps["xyz"], ps["rotation"], ps["scaling"], ps["opacity"], scale=1.0)
    assert fd.DRAW_RANGE == mm.DRAW_RANGE == 1 << 62
