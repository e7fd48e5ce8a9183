"""Each pixel's first or heaviest K contributors (include/gsrast.h: gsrast_pixel_contributors; `pixel_contributors` of the Python package) in
torch -- a helper of the tests, not a test.

The restatement on tests/contrib_math.py's pairs(): math_renderer.blend_pairs gives every pair's weight w = alpha T (`bl["w"]`, [N, G], N = H W
pixels row-major, G the visible Gaussians in depth order = blend order) and whether the forward blends it (`bl["live"]`); out["order"] names
the G Gaussians' rows.  Per pixel

    count            the number of live pairs
    order "weight"   slots 0 .. min(K, count) - 1: the live pairs by descending w -- a STABLE argsort of -w, so that on equal w the pair earlier
                     in blend order comes first (contrib's top_count rule: slot 0 is contrib_math's `best`)
    order "depth"    slots 0 .. min(K, count) - 1: the first live pairs in blend order
    unused slots     id -1, weight +0.0

`slots` does that for any weight matrix (the host test drives it with hand-made ones); `reference(name, antialiasing)` holds the float64 and
the float32 pair matrices of a contrib_math case, computed once per process and shared: do not modify them; `topk` is `slots` on one of them.

A pixel is AMBIGUOUS (`ambiguous`) where math_renderer's own mask is set (a blend decision within fp32 rounding of its threshold) and also, in
weight order, where two adjacent entries of its sorted top-(K + 1) weights differ by less than GAP = 1e-4 relative: there fp32 rounding may
swap two slots, or the last slot with the first pair left out.

`bar(ref)`: the tolerance of the GPU test's weights for a case, 4 x max |w32 - w64| + 2^-23 -- w32 the restatement run with dtype=float32, the
maximum over the case's non-ambiguous entries: the K = 16 slots of both orders on the pixels that are not ambiguous for that order."""
import functools

import numpy as np
import torch

import contrib_math as cm

GAP = 1e-4
K_MAX = 16
ORDERS = ("weight", "depth")


def slots(w, live, rows, K, order):
    """(ids [N,K] int64, weights [N,K] in w's dtype, count [N] int64) of a pair matrix: w [N,G] (any value where not live), live [N,G] bool,
    rows [G] the Gaussians' ids in blend order."""
    w, live, rows = torch.as_tensor(w), torch.as_tensor(live), torch.as_tensor(rows, dtype=torch.int64)
    N, G = w.shape
    count = live.sum(dim=1)
    wl = torch.where(live, w, torch.zeros_like(w))
    if order == "weight":
        key = torch.where(live, -wl, torch.ones_like(wl))                  # (dead pairs behind every live one: a live w is > 0)
    elif order == "depth":
        key = (~live).to(w.dtype)
    else:
        raise ValueError(order)
    perm = torch.argsort(key, dim=1, stable=True)[:, :K]                    # [N, min(K, G)]
    ids = torch.full((N, K), -1, dtype=torch.int64)
    weights = torch.zeros((N, K), dtype=w.dtype)
    if G > 0:
        k = perm.shape[1]
        used = torch.arange(k)[None, :] < count[:, None]
        ids[:, :k] = torch.where(used, rows[perm], torch.full_like(perm, -1))
        weights[:, :k] = torch.where(used, torch.gather(wl, 1, perm), torch.zeros((), dtype=w.dtype))
    return ids, weights, count


def gap_ambiguous(w, live, K):
    """[N] bool: two adjacent entries of the pixel's sorted top-(K + 1) live weights differ by less than GAP relative."""
    w, live = torch.as_tensor(w), torch.as_tensor(live)
    wl = torch.where(live, w, torch.zeros_like(w))
    if wl.shape[1] < 2:
        return torch.zeros((wl.shape[0],), dtype=torch.bool)
    top = torch.topk(wl, min(K + 1, wl.shape[1]), dim=1).values            # descending
    hi, lo = top[:, :-1], top[:, 1:]
    return ((lo > 0) & ((hi - lo) < GAP * hi)).any(dim=1)


@functools.lru_cache(maxsize=None)
def _reference(name, antialiasing):
    r = cm.reference(name, antialiasing)                                    # (the float64 render, shared with the contrib tests)
    sc, cam, out = r["sc"], r["cam"], r["out"]
    bl64, _ = cm.pairs(sc, cam, torch.float64, antialiasing, out)
    bl32, _ = cm.pairs(sc, cam, torch.float32, antialiasing, out)
    H, W = out["ambiguous"].shape
    ref = dict(name=name, antialiasing=antialiasing, sc=sc, cam=cam, out=out, H=H, W=W, P=sc["means3D"].shape[0],
               rows=torch.as_tensor(out["order"], dtype=torch.int64), w64=bl64["w"], live64=bl64["live"], w32=bl32["w"], live32=bl32["live"],
               amb_mr=torch.as_tensor(out["ambiguous"].reshape(-1).copy()))
    return ref


def reference(name, antialiasing=False):
    """The pair matrices of contrib_math.CASES[name] (float64 and float32 on the float64 render's lists), computed once per process."""
    return _reference(name, bool(antialiasing))


def ambiguous(ref, K, order):
    """[N] bool (torch): the pixels of `ref` whose K slots in `order` the GPU need not reproduce."""
    return ref["amb_mr"] | gap_ambiguous(ref["w64"], ref["live64"], K) if order == "weight" else ref["amb_mr"]


def topk(ref, K, order, dtype=torch.float64):
    """slots() on the case's float64 (or float32) pair matrix."""
    w, live = (ref["w64"], ref["live64"]) if dtype == torch.float64 else (ref["w32"], ref["live32"])
    return slots(w, live, ref["rows"], K, order)


@functools.lru_cache(maxsize=None)
def _bar(name, antialiasing):
    ref = reference(name, antialiasing)
    worst = 0.0
    for order in ORDERS:
        ok = ~ambiguous(ref, K_MAX, order)
        w64 = topk(ref, K_MAX, order)[1]
        w32 = topk(ref, K_MAX, order, torch.float32)[1].to(torch.float64)
        if bool(ok.any()):
            worst = max(worst, float((w32 - w64)[ok].abs().max()))
    return worst


def bar(ref):
    """(the tolerance 4 max|w32 - w64| + 2^-23 of the case's weights, max|w32 - w64| itself)."""
    worst = _bar(ref["name"], ref["antialiasing"])
    return 4.0 * worst + 2.0 ** -23, worst


def planar(t, H, W):
    """[N, K] -> numpy [K, H, W], the layout of the call's outputs."""
    return np.ascontiguousarray(torch.as_tensor(t).T.reshape(-1, H, W).numpy())
