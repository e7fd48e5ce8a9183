"""What the k-NN index query (fused_knn.knn_query, the mmcv.ops.knn drop-in) costs: medians of device-synchronised calls -- a self-query at
k = 2 (the reference's own call, helper_model.py:150) and k = 16, and a separate query set (a jittered third of the cloud, k = 8) -- on
100 k and 1 M uniform points and on one clustered cloud.  Yardsticks from the same run: distCUDA2 on the same cloud (the 3-NN search this
one grew out of; it gathers through order[j], returns one mean and no ids), and a chunked torch.cdist + topk, which is what a user without
mmcv would write; its ids are cross-checked against ours on the first chunk.  No time here is a pass / fail condition.  One JSON object
on stdout (kept as profiles/knn_query_overhead.json).

usage: python tools/knn_query_overhead.py [--steps 20] [--warmup 3] [--clouds uniform_100k,uniform_1m,clustered_400k]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CDIST_CHUNK = 2048          # queries per torch.cdist call (x 1 M references x 4 B = 8 GiB of distances at the largest cloud)


def cloud(name: str) -> np.ndarray:
    rng = np.random.default_rng(5)
    if name == "uniform_100k":
        return rng.uniform(-10, 10, size=(100_000, 3)).astype(np.float32)
    if name == "uniform_1m":
        return rng.uniform(-10, 10, size=(1_000_000, 3)).astype(np.float32)
    if name == "clustered_400k":      # 400 clusters of 1000, sigma 0.02, in a cube of 20: most of the grid is empty
        return np.concatenate([rng.normal(c, 0.02, size=(1000, 3)) for c in rng.uniform(-10, 10, size=(400, 3))]).astype(np.float32)
    raise KeyError(name)


def median_ms(fn, steps: int, warmup: int):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]


def cdist_topk(ref: torch.Tensor, query: torch.Tensor, k: int, chunks: int) -> torch.Tensor:
    """The ids [k, .] of the first `chunks` chunks of the queries (every chunk is the same work: the whole set's time is this one's, scaled)."""
    out = []
    for m0 in range(0, min(query.shape[0], chunks * CDIST_CHUNK), CDIST_CHUNK):
        d = torch.cdist(query[m0:m0 + CDIST_CHUNK], ref, compute_mode="donot_use_mm_for_euclid_dist")
        out.append(d.topk(k, dim=1, largest=False).indices.t())
    return torch.cat(out, dim=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", default="uniform_100k,uniform_1m,clustered_400k")
    ap.add_argument("--cdist-steps", type=int, default=3, help="the brute-force yardstick is slow: fewer timed calls, one warm-up call")
    ap.add_argument("--cdist-chunks", type=int, default=8, help="chunks of the query set the yardstick is timed on; its whole-set time is scaled from them")
    a = ap.parse_args()
    from fused_knn import knn_query
    from simple_knn._C import distCUDA2
    dev = torch.device("cuda:0")
    result = {"steps": a.steps, "warmup": a.warmup, "cdist_steps": a.cdist_steps, "cdist_chunk": CDIST_CHUNK, "cdist_chunks": a.cdist_chunks, "clouds": {}}
    for name in a.clouds.split(","):
        pts = cloud(name)
        ref = torch.from_numpy(pts).to(dev)
        jitter = np.random.default_rng(6).normal(0, 1e-3, size=pts[::3].shape).astype(np.float32)
        query = torch.from_numpy(pts[::3] + jitter).to(dev)
        row = {"n_ref": int(ref.shape[0]), "n_query_separate": int(query.shape[0])}
        row["distCUDA2_ms"], row["distCUDA2_spread_ms"] = median_ms(lambda: distCUDA2(ref), a.steps, a.warmup)
        for label, q, k in (("self_k2", None, 2), ("self_k16", None, 16), ("separate_k8", query, 8)):
            row[label + "_ms"], row[label + "_spread_ms"] = median_ms(lambda: knn_query(ref, q, k), a.steps, a.warmup)
            row[label + "_ids_only_ms"], _ = median_ms(lambda: knn_query(ref, q, k, return_dist2=False), a.steps, a.warmup)
            qq = ref if q is None else q
            n_chunks = (qq.shape[0] + CDIST_CHUNK - 1) // CDIST_CHUNK
            timed = min(n_chunks, a.cdist_chunks)
            part, _ = median_ms(lambda: cdist_topk(ref, qq, k, timed), a.cdist_steps, 1)
            row[label + "_cdist_topk_ms"] = round(part * n_chunks / timed, 2)      # (timed on `timed` of the n_chunks equal chunks, scaled)
            row[label + "_cdist_chunks_timed"] = [timed, n_chunks]
            ours = knn_query(ref, q, k)[0][:, :CDIST_CHUNK].long()
            theirs = cdist_topk(ref, qq, k, 1)
            row[label + "_ids_equal_to_cdist_first_chunk"] = round(float((ours == theirs).float().mean()), 6)      # (near-ties may rank either way: a share, not an assertion)
        result["clouds"][name] = row
        del ref, query
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
