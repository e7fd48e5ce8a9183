// gsrast_knn_query.h -- exact k-nearest-neighbour query: for every query point the k reference points with the smallest (d2, index), ids
// and squared distances (include/gsrast.h: gsrast_knn_query).  Replaces `mmcv.ops.knn`, the un-vendored dependency the reference imports at
// helper_model.py:27 and calls as knn(2, xyz, xyz, False) at :150, :207 and :354.  Only the call's signature and its (B, k, npoint) result
// layout are mirrored; the search is the box search of gsrast_knn.h with three differences: the reference set is read from a Morton-ordered
// COPY (16-byte records {x, y, z, original index}, so a box scan reads 16 KiB of contiguous memory through one wave-uniform address instead
// of gathering through order[j] per lane and candidate), the query set may be another set than the reference, and a lane keeps k (d2, index)
// pairs, not three distances.
//
// d2(q, r) = (a a + b b) + c c with a = q.x - r.x, b = q.y - r.y, c = q.z - r.z, each one fp32 operation (the library is built with
// -ffp-contract=off).  A pair is one 64-bit key, d2's bits in the high word and the index in the low one: d2 is a sum of squares, so it is
// +0 or positive (or NaN), the bits of such floats order as the floats do, and `key <` is the lexicographic (d2, index) order.  A NaN
// (non-finite coordinates: unsupported) has bits above +inf's with either sign, so it is never below a limit and is never inserted.
//
// Search, one lane per query, queries in Morton order on the REFERENCE's grid (knn_morton_kernel clamps to it: a query outside the
// reference's bounding box gets the code of the nearest face, edge or corner), so the 64 queries of a wave want the same boxes:
//   seed:   an upper bound of the query's true k-th distance -- the largest d2 among k DISTINCT reference points, the k consecutive
//           records around the query's own place in the reference's Morton order (self-query: its own record; else a binary search of
//           its code in the sorted codes).  Whatever those k points are, k points lie within `seed`, so the k-th nearest does.
//           n_ref < k: +inf.
//   boxes:  b = 0 .. nboxes - 1 (wave-uniform).  A lane WANTS box b unless lb(b) > min(seed, the d2 of its current k-th pair); the wave
//           scans the box if any lane wants it (a ballot), every lane reading the same record at a time.
//   insert: a candidate goes into the lane's list only if its key is below the lane's limit = min(k-th key, (seed, 0xFFFFFFFF)).
//
// Why this is exact.  Let d_k be the query's true k-th smallest d2 and T the set of its true k smallest (d2, index) keys.
//   (1) seed >= d_k (above), and the list's k-th d2 is >= d_k at any time (it is the k-th smallest of a SUBSET of the keys, +inf while
//       the list is not full).  So a lane's rejection radius is never below d_k.
//   (2) lb(b) <= d2(q, r) for every r in box b, IN FP32: lb is evaluated with d2's own expression on the point c = clamp(q, lo, hi) of the
//       box nearest to q.  Per axis |q - c| <= |q - r| in the reals; the rounded difference, its rounded square and the two rounded sums
//       (added in the same order) are each monotone, so the inequality survives every rounding.  It would not if lb were shaped otherwise.
//   (3) a box is skipped only if lb > radius, STRICTLY.  By (1) and (2) every r of a skipped box has d2 >= lb > radius >= d_k: it is
//       not in T, not even as an equal-distance point with a lower index (that one has d2 == d_k, and its box, lb <= d_k, is visited).
//   (4) a visited candidate is dropped only if its key is not below the limit: not below the current k-th key (then k keys of the list
//       are smaller or equal: it is not in T, or already is that key -- every record is visited once), or its d2 > seed >= d_k.
//   So every member of T is visited and inserted, nothing displaces it but a smaller key, and the list ends as T, ascending.
//
// Registers: the list is CAP keys named by compile-time indices only (every loop over them is fully unrolled: no runtime-indexed array,
// no scratch; cdna_hip_programming.md, guideline 20), CAP in {2, 4, 8, 16, 32}, the smallest >= k chosen on the host.  The k live pairs
// sit in the LAST k slots; the CAP - k slots in front hold key 0, which no candidate is below, so slot CAP - 1 is the k-th pair whatever
// k is and nothing is indexed by k before the stores.  Insertion is topk's chain (gsrast_topk.h): the key goes in front of the first slot
// it is below, the slots behind move down one, the last leaves; lanes whose candidate is not below their limit skip it, a wave in which
// none is branches over it.
//
// Every output element has one writer (the lane of its query), there are no atomics and no LDS: bit-identical from run to run.
//
// Resources (gfx950, tools/kernel_resources.sh knnq; scratch 0 and LDS 0 in every instantiation), CAP 2 | 4 | 8 | 16 | 32:
//   knnq_search_kernel:  VGPR 20 | 24 | 32 | 45 | 77  (SGPR 38 | 38 | 40 | 53 | 83: the four records in flight are scalar registers)
//   knnq_records_kernel: VGPR 6;  knnq_fill_kernel: VGPR 8
#pragma once
#include "gsrast_common.h"
#include "gsrast_knn.h"

namespace gsrast {

constexpr int KNNQ_MAX_K = 32;
constexpr uint32_t KNNQ_NO_ID = 0x7FFFFFFFu;                                    // the index of an empty slot (n_ref <= INT_MAX: never a row)
constexpr uint64_t KNNQ_EMPTY = ((uint64_t)0x7F800000u << 32) | KNNQ_NO_ID;     // (+inf, no id)

// Morton-permuted copy of the reference: rec[s] = {x, y, z, bits of order[s]}
__global__ void __launch_bounds__(256)
knnq_records_kernel(int n, const float* __restrict__ pts, const uint32_t* __restrict__ order, float4* __restrict__ rec)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t g = order[s];
    rec[s] = make_float4(pts[3 * (size_t)g], pts[3 * (size_t)g + 1], pts[3 * (size_t)g + 2], __uint_as_float(g));
}

// n_ref == 0: every slot is missing
__global__ void __launch_bounds__(256)
knnq_fill_kernel(size_t slots, int32_t* __restrict__ idx, float* __restrict__ dist2 /* or null */)
{
    const size_t stride = (size_t)gridDim.x * 256u;
    for (size_t e = (size_t)blockIdx.x * 256u + threadIdx.x; e < slots; e += stride) {
        idx[e] = -1;
        if (dist2) dist2[e] = __uint_as_float(0x7F800000u);
    }
}

__device__ __forceinline__ float knnq_d2(float qx, float qy, float qz, float rx, float ry, float rz)
{
    const float a = qx - rx, b = qy - ry, c = qz - rz;
    return a * a + b * b + c * c;
}
__device__ __forceinline__ uint64_t knnq_key(float d2, uint32_t id) { return ((uint64_t)__float_as_uint(d2) << 32) | id; }

template <int CAP>
__global__ void __launch_bounds__(256)
knnq_search_kernel(int n_ref, const float4* __restrict__ rec, const uint32_t* __restrict__ ref_codes /* sorted */, const float* __restrict__ boxes, int nboxes,
                   int n_query, const float* __restrict__ query /* null: the reference queries itself */, const uint32_t* __restrict__ qorder,
                   const uint32_t* __restrict__ qcodes /* sorted */, int k /* 1 .. CAP */, int32_t* __restrict__ idx /* [k][n_query] */,
                   float* __restrict__ dist2 /* [k][n_query] or null */)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if ((int)(blockIdx.x * 256 + (threadIdx.x & ~63u)) >= n_query) return;      // a whole wave past the end (uniform)
    const bool live = s < n_query;
    if (!live) s = n_query - 1;       // the idle lanes of the last wave shadow its last query: the same boxes, the same insertions, no stores
    float qx, qy, qz;
    uint32_t qi;
    int pos;                          // the query's place in the reference's Morton order
    if (query == nullptr) {
        const float4 me = rec[s];
        qx = me.x; qy = me.y; qz = me.z; qi = __float_as_uint(me.w); pos = s;
    } else {
        qi = qorder[s];
        qx = query[3 * (size_t)qi]; qy = query[3 * (size_t)qi + 1]; qz = query[3 * (size_t)qi + 2];
        const uint32_t code = qcodes[s];
        int lo = 0, hi = n_ref;       // first reference code that is not below the query's
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (ref_codes[mid] < code) lo = mid + 1; else hi = mid; }
        pos = lo;
    }
    float seed = __uint_as_float(0x7F800000u);
    if (n_ref >= k) {
        int w0 = pos - (k >> 1);
        w0 = w0 < 0 ? 0 : (w0 > n_ref - k ? n_ref - k : w0);
        seed = 0.0f;
        for (int j = 0; j < k; j++) {
            const float4 r = rec[w0 + j];
            const float d = knnq_d2(qx, qy, qz, r.x, r.y, r.z);
            seed = d > seed ? d : seed;
        }
    }
    const uint64_t seed_limit = ((uint64_t)__float_as_uint(seed) << 32) | 0xFFFFFFFFu;

    uint64_t best[CAP];
#pragma unroll
    for (int c = 0; c < CAP; c++) best[c] = c < CAP - k ? 0ull : KNNQ_EMPTY;
    uint64_t limit = seed_limit < KNNQ_EMPTY ? seed_limit : KNNQ_EMPTY;

    for (int b = 0; b < nboxes; b++) {
        const float* bx = boxes + 6 * (size_t)b;
        const float cx = fminf(fmaxf(qx, bx[0]), bx[3]), cy = fminf(fmaxf(qy, bx[1]), bx[4]), cz = fminf(fmaxf(qz, bx[2]), bx[5]);
        const float lb = knnq_d2(qx, qy, qz, cx, cy, cz);
        const float radius = __uint_as_float((uint32_t)(limit >> 32));          // min(seed, the k-th pair's d2)
        if (__ballot(!(lb > radius)) == 0ull) continue;                         // no lane of the wave wants this box (uniform)
        const int j0 = b * KNN_BOX, j1 = (j0 + KNN_BOX) < n_ref ? (j0 + KNN_BOX) : n_ref;
        const auto consider = [&](const float4& r) {
            const uint64_t key = knnq_key(knnq_d2(qx, qy, qz, r.x, r.y, r.z), __float_as_uint(r.w));
            if (key < limit) {
#pragma unroll
                for (int c = CAP - 1; c >= 1; c--) {                            // (from the back: slot c - 1 still holds its old pair)
                    const bool here = key < best[c], above = key < best[c - 1];
                    best[c] = here ? (above ? best[c - 1] : key) : best[c];
                }
                if (key < best[0]) best[0] = key;
                limit = best[CAP - 1] < seed_limit ? best[CAP - 1] : seed_limit;
            }
        };
        // every address is wave-uniform (scalar loads); four records are fetched in front of the four insertions, which branch
        int j = j0;
        for (; j + 4 <= j1; j += 4) {
            const float4 r0 = rec[j], r1 = rec[j + 1], r2 = rec[j + 2], r3 = rec[j + 3];
            consider(r0); consider(r1); consider(r2); consider(r3);
        }
        for (; j < j1; j++) consider(rec[j]);
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < CAP; c++) {
            const int j = c - (CAP - k);                                        // (uniform test)
            if (j >= 0) {
                const uint32_t id = (uint32_t)best[c];
                const bool missing = id == KNNQ_NO_ID;
                const size_t o = (size_t)j * (size_t)n_query + qi;
                idx[o] = missing ? -1 : (int32_t)id;
                if (dist2) dist2[o] = __uint_as_float(missing ? 0x7F800000u : (uint32_t)(best[c] >> 32));
            }
        }
    }
}

} // namespace gsrast
