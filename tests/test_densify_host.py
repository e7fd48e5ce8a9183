"""Densification, host side (no GPU): the two CPU restatements of tests/densify_math.py agree exactly, the C ABI declares and exports
the new entry points without a version bump, and every argument error is refused before any device call."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import densify_math as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsrast_densify_scratch_bytes", "gsrast_densify_plan", "gsrast_densify_apply", "gsrast_densify_stats_update")


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("P", [0, 1, 300])
@pytest.mark.parametrize("mix", dm.MIXES)
def test_sequential_equals_closed_form(mix, P, N):
    d = dm.draw(P, 4, mix, seed=100 + P + N)
    assert dm.margins_ok(d)
    kw = dict(d["kw"], N=N, prune_mask=d["prune_mask"], grad_scale=d["grad_scale"])
    _, split_all, pruned = dm.classify(d["params"], d["accum"], d["denom"], **{k: v for k, v in kw.items() if k != "N"})
    n_all = int(split_all.sum())
    noise = torch.randn(N * n_all, 3, generator=torch.Generator().manual_seed(7))
    counts, rows, parts = dm.closed_form(d["params"], d["moments"], d["accum"], d["denom"], noise, **kw)
    opt = dm.make_adam(d["params"], d["moments"])
    left = dm.sequential(opt, d["accum"], d["denom"], noise, **kw)
    assert left == counts["P"] == counts["n_kept"] + counts["n_clone"] + N * counts["n_split"]
    seq = dm.optimizer_rows(opt)
    for k in dm.GROUPS:
        for a, b, what in zip(seq[k], rows[k], ("param", "exp_avg", "exp_avg_sq")):
            assert a.shape == b.shape and torch.equal(a, b), (k, what)
    if P == 300:        # the mixes are what they say
        expect = dict(none=lambda c: c["n_clone"] == 0 and c["n_split_all"] == 0 and c["n_kept"] > 0,
                      all_clone=lambda c: c["n_clone"] == c["n_kept"] > 0 and c["n_split_all"] == 0,
                      all_split=lambda c: c["n_kept"] == 0 and c["n_split_all"] == c["n_split"] == P and c["P"] == N * P,
                      all_pruned=lambda c: c["P"] == 0 and c["n_split_all"] > 0,
                      overlap=lambda c: 0 < c["n_split"] < c["n_split_all"] and c["n_clone"] > 0,     # pruned AND split-selected sources: rank_all != rank
                      mixed=lambda c: min(c["n_kept"], c["n_clone"], c["n_split"]) > 0 and c["n_split"] < c["n_split_all"])
        assert expect[mix](counts), counts


def test_prune_only_is_a_gather():
    d = dm.draw(300, 4, "mixed", seed=5)
    counts, rows, parts = dm.closed_form(d["params"], d["moments"], d["accum"], d["denom"], torch.zeros(0, 3), thr=math.inf, tau=0.0, N=1,
                                         prune_mask=d["prune_mask"])
    keep = ~d["prune_mask"]
    assert counts == dict(n_kept=int(keep.sum()), n_clone=0, n_split=0, n_split_all=0, P=int(keep.sum()))
    for k in dm.GROUPS:
        assert torch.equal(rows[k][0], d["params"][k][keep]) and torch.equal(rows[k][1], d["moments"][k][0][keep])


def test_new_symbols_are_declared_and_exported(rast):
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    raw = C.CDLL(rast._C.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in rast._C.EXPORTS and hasattr(raw, n), n
        assert getattr(L, n).argtypes is not None
    assert "gsrast_densify_group" in text
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert C.sizeof(rast._C.DensifyGroupStruct) == 6 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_int)
    b = [L.gsrast_densify_scratch_bytes(p) for p in (-1, 0, 1, 70001, 3_000_000)]
    assert b[0] == b[1] > 0 and all(y >= x for x, y in zip(b, b[1:])) and all(x % 256 == 0 for x in b)
    assert b[-1] / 3_000_000 < 1.1          # a class byte per Gaussian + 16 B per 256 of them


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    _C = rast._C
    L = _C.lib()
    one = 16      # any non-NULL value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731

    def plan(P=10, N=2, thr=1e-4, accum=one, denom=one, scaling=one, opacity=one, min_opacity=0.005, scratch=one, counts=one):
        return L.gsrast_densify_plan(P, N, accum, denom, None, scaling, opacity, None, thr, 0.01, min_opacity, scratch, counts, None)

    for thr in (0.0, -1.0, float("nan"), -math.inf):
        assert plan(thr=thr) == -1 and "grad_threshold must be > 0" in err()
    for N in (0, 5, -1):
        assert plan(N=N) == -1 and "[1, 4]" in err()
    assert plan(P=-1) == -1 and "negative P" in err()
    assert plan(scratch=None) == -1 and "NULL scratch" in err()
    assert plan(scaling=None) == -1 and "needs scaling" in err()
    assert plan(opacity=None) == -1 and "without opacity_logit" in err()

    GS = _C.DensifyGroupStruct

    def apply(groups, P=10, N=2, counts=(6, 2, 1, 3, 10), n_groups=None, rotation=one, scaling=one, noise=one, scratch=one):
        arr = (GS * max(len(groups), 1))(*groups)
        ch = (C.c_uint * 5)(*counts) if counts is not None else None
        return L.gsrast_densify_apply(P, N, scratch, ch, len(groups) if n_groups is None else n_groups, arr, rotation, scaling, noise, None)

    ok = GS(one, one, one, one, one, one, 3, _C.DENSIFY_COPY)
    assert apply([ok], P=-1) == -1 and "negative P" in err()
    assert apply([ok], N=5) == -1 and "[1, 4]" in err()
    assert apply([ok] * 17) == -1 and "at most 16 groups" in err()
    assert apply([ok], n_groups=-1) == -1
    for w in (0, 65, -3):
        assert apply([GS(one, None, None, one, None, None, w, _C.DENSIFY_COPY)]) == -1 and "width must be in [1, 64]" in err()
    assert apply([GS(one, one, None, one, None, None, 3, _C.DENSIFY_COPY)]) == -1 and "without dst_m" in err()
    assert apply([GS(one, None, one, one, None, None, 3, _C.DENSIFY_COPY)]) == -1 and "without dst_m" in err()
    assert apply([GS(one, None, None, one, None, None, 3, 7)]) == -1 and "role" in err()
    xyz = GS(one, None, None, one, None, None, 3, _C.DENSIFY_XYZ)
    for missing in ("rotation", "scaling", "noise"):
        assert apply([xyz], **{missing: None}) == -1 and "rotation, scaling and noise" in err()
    assert apply([GS(one, None, None, one, None, None, 4, _C.DENSIFY_XYZ)]) == -1 and "width 3" in err()
    assert apply([ok], counts=(6, 2, 1, 3, 11)) == -1 and "counts are not those of a plan" in err()      # P' != kept + clone + N * split
    assert apply([ok], counts=(9, 2, 1, 3, 13)) == -1                                                     # kept + split_all > P
    assert apply([ok], counts=None) == -1 and apply([ok], scratch=None) == -1
    # what is valid and needs no device: nothing to move
    assert apply([], P=0, counts=(0, 0, 0, 0, 0)) == 0
    assert apply([xyz], P=0, counts=(0, 0, 0, 0, 0), rotation=None, scaling=None, noise=None) == 0       # n_split == 0: no noise needed

    assert L.gsrast_densify_stats_update(-1, one, one, one, one, one, one, 0, None) == -1 and "negative P" in err()
    assert L.gsrast_densify_stats_update(10, None, one, one, one, one, one, 0, None) == -1 and "NULL" in err()
    assert L.gsrast_densify_stats_update(10, one, one, None, one, one, one, 0, None) == -1
    assert L.gsrast_densify_stats_update(0, None, None, None, None, None, None, 0, None) == 0


def test_python_surface_refuses_cpu_tensors():
    import fused_densify
    p = {k: torch.nn.Parameter(torch.zeros((4,) + s)) for k, s in dm.shapes(4).items()}
    opt = dm.make_adam({k: v.detach() for k, v in p.items()}, None)
    with pytest.raises(RuntimeError, match="GPU"):
        fused_densify.prune(opt, torch.zeros(4, dtype=torch.bool))
