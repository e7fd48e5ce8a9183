// C ABI over the REFERENCE's own CudaRasterizer::Rasterizer, built by oracle/ref_build.py into oracle/_ref/libref_rasterizer.so
// together with the reference's three kernel sources (compiled for gfx950 from a build-time copy; none of their text is in this
// repository).  TEST INFRASTRUCTURE ONLY: loaded by tests/ref_kernels.py in a child process of its own, never by the product.
//
// Every entry point takes plain HOST pointers: it uploads its inputs, calls the reference's static method, synchronises, downloads the
// outputs and frees what it allocated.  Return value: the HIP error code (0 = hipSuccess); -1 = the list capacity was too small, -2 = a C++
// exception from the reference or from an allocator.  After a non-zero return nothing in the output arrays is meaningful.
//
// ref_forward mirrors the reference binding's `if (P != 0)` guard (rasterize_points.cu:81) and keeps the three state buffers alive in an
// opaque handle for ref_backward; ref_free releases them.  The state buffers are zero-filled when allocated, so the rows of the
// intermediates that the preprocess kernel never writes (culled Gaussians) read as zero and not as whatever the allocation held.
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <vector>

#include <hip/hip_runtime.h>

#include "rasterizer.h"
#include "rasterizer_impl.h"

namespace {

struct Handle {
    char* geom = nullptr;
    char* binning = nullptr;
    char* img = nullptr;
    int P = 0, R = 0, W = 0, H = 0;
};

// every device allocation of one call, freed when the call returns
struct Arena {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~Arena() { for (void* p : ptrs) (void)hipFree(p); }

    void* raw(size_t bytes) {
        if (err != hipSuccess || bytes == 0) return nullptr;
        void* p = nullptr;
        err = hipMalloc(&p, bytes);
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
    template <typename T> T* zeros(size_t n) {
        T* p = static_cast<T*>(raw(n * sizeof(T)));
        if (p && err == hipSuccess) err = hipMemset(p, 0, n * sizeof(T));
        return p;
    }
    // a null host pointer stays a null device pointer: the reference tests `colors_precomp != nullptr`, `cov3D_precomp != nullptr`
    template <typename T> T* upload(const T* host, size_t n) {
        if (host == nullptr) return nullptr;
        T* p = static_cast<T*>(raw(n * sizeof(T)));
        if (p && err == hipSuccess) err = hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
        return p;
    }
};

template <typename T> hipError_t download(T* host, const void* dev, size_t n) {
    if (host == nullptr || dev == nullptr || n == 0) return hipSuccess;
    return hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
}

std::function<char*(size_t)> state_allocator(char** slot) {
    return [slot](size_t n) -> char* {
        void* p = nullptr;
        if (hipMalloc(&p, n) != hipSuccess || hipMemset(p, 0, n) != hipSuccess) throw std::runtime_error("state buffer allocation failed");
        *slot = static_cast<char*>(p);
        return *slot;
    };
}

void release(Handle* h) {
    if (h == nullptr) return;
    if (h->geom) (void)hipFree(h->geom);
    if (h->binning) (void)hipFree(h->binning);
    if (h->img) (void)hipFree(h->img);
    delete h;
}

hipError_t sync_and_last_error() {
    hipError_t e = hipDeviceSynchronize();
    hipError_t l = hipGetLastError();
    return e != hipSuccess ? e : l;
}

#define REF_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return static_cast<int>(e_); } while (0)

}  // namespace

extern "C" {

// shs [P, M, 3] or null; colors_precomp [P, 3] or null; scales [P, 3] + rotations [P, 4] or cov3D_precomp [P, 6].
// Outputs (any may be null): out_color [3, H, W], out_depth [H, W], radii [P], num_rendered [1]; the intermediates depths [P], means2D
// [P, 2], cov3D [P, 6], conic_opacity [P, 4], rgb [P, 3], clamped [P, 3] (bytes), tiles_touched [P], keys_sorted / point_list
// [list_capacity], ranges [tiles, 2], n_contrib [H, W], accum_alpha [H, W].  *handle receives the state (null when P == 0).
int ref_forward(int P, int D, int M, const float* background, int W, int H, const float* means3D, const float* shs,
                const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                float tan_fovy, float* out_color, float* out_depth, int* radii, int* num_rendered, float* depths, float* means2D,
                float* cov3D, float* conic_opacity, float* rgb, uint8_t* clamped, uint32_t* tiles_touched, int64_t list_capacity,
                uint64_t* keys_sorted, uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib, float* accum_alpha, void** handle)
{
    if (handle) *handle = nullptr;
    if (num_rendered) *num_rendered = 0;
    const size_t N = static_cast<size_t>(W) * static_cast<size_t>(H);
    Arena a;
    float* d_color = a.zeros<float>(3 * N);          // the binding's torch::full(..., 0.0)
    float* d_depth = a.zeros<float>(N);
    int* d_radii = a.zeros<int>(P);
    REF_TRY(a.err);
    int R = 0;
    Handle* h = nullptr;
    if (P != 0) {
        const size_t p = static_cast<size_t>(P);
        const float* d_bg = a.upload(background, 3);
        const float* d_means = a.upload(means3D, 3 * p);
        const float* d_shs = a.upload(shs, 3 * p * static_cast<size_t>(M));
        const float* d_pre = a.upload(colors_precomp, 3 * p);
        const float* d_opac = a.upload(opacities, p);
        const float* d_scales = a.upload(scales, 3 * p);
        const float* d_rot = a.upload(rotations, 4 * p);
        const float* d_cov = a.upload(cov3D_precomp, 6 * p);
        const float* d_view = a.upload(viewmatrix, 16);
        const float* d_proj = a.upload(projmatrix, 16);
        const float* d_cam = a.upload(campos, 3);
        REF_TRY(a.err);
        h = new Handle();
        h->P = P; h->W = W; h->H = H;
        try {
            R = CudaRasterizer::Rasterizer::forward(state_allocator(&h->geom), state_allocator(&h->binning), state_allocator(&h->img),
                                                    P, D, M, d_bg, W, H, d_means, d_shs, d_pre, d_opac, d_scales, scale_modifier, d_rot,
                                                    d_cov, d_view, d_proj, d_cam, tan_fovx, tan_fovy, /*prefiltered=*/false, d_color,
                                                    d_depth, d_radii);
        } catch (const std::exception&) {
            (void)hipDeviceSynchronize();
            release(h);
            return -2;
        }
        hipError_t e = sync_and_last_error();
        if (e != hipSuccess) { release(h); return static_cast<int>(e); }
        h->R = R;
    } else {
        REF_TRY(sync_and_last_error());
    }
    if (num_rendered) *num_rendered = R;
    hipError_t e = download(out_color, d_color, 3 * N);
    if (e == hipSuccess) e = download(out_depth, d_depth, N);
    if (e == hipSuccess) e = download(radii, d_radii, static_cast<size_t>(P));
    if (h != nullptr && e == hipSuccess) {
        const size_t p = static_cast<size_t>(P);
        char* c = h->geom;
        CudaRasterizer::GeometryState g = CudaRasterizer::GeometryState::fromChunk(c, p);
        c = h->img;
        CudaRasterizer::ImageState im = CudaRasterizer::ImageState::fromChunk(c, N);
        c = h->binning;
        CudaRasterizer::BinningState b = CudaRasterizer::BinningState::fromChunk(c, static_cast<size_t>(R));
        const size_t tiles = static_cast<size_t>((W + 15) / 16) * static_cast<size_t>((H + 15) / 16);
        e = download(depths, g.depths, p);
        if (e == hipSuccess) e = download(means2D, g.means2D, 2 * p);
        if (e == hipSuccess) e = download(cov3D, g.cov3D, 6 * p);
        if (e == hipSuccess) e = download(conic_opacity, g.conic_opacity, 4 * p);
        if (e == hipSuccess) e = download(rgb, g.rgb, 3 * p);
        if (e == hipSuccess) e = download(clamped, g.clamped, 3 * p);
        if (e == hipSuccess) e = download(tiles_touched, g.tiles_touched, p);
        if (e == hipSuccess) e = download(ranges, im.ranges, 2 * tiles);
        if (e == hipSuccess) e = download(n_contrib, im.n_contrib, N);
        if (e == hipSuccess) e = download(accum_alpha, im.accum_alpha, N);
        if (e == hipSuccess && (keys_sorted != nullptr || point_list != nullptr)) {
            if (static_cast<int64_t>(R) > list_capacity) { release(h); return -1; }
            e = download(keys_sorted, b.point_list_keys, static_cast<size_t>(R));
            if (e == hipSuccess) e = download(point_list, b.point_list, static_cast<size_t>(R));
        }
    }
    if (e != hipSuccess) { release(h); return static_cast<int>(e); }
    if (handle) *handle = h; else release(h);
    return 0;
}

// handle: ref_forward's (null when P == 0); radii: ref_forward's output.  Outputs, all zero-filled first as the binding's torch::zeros:
// dL_dmeans2D [P, 3], dL_dconic [P, 4], dL_dopacity [P], dL_dcolors [P, 3], dL_dmeans3D [P, 3], dL_dcov3D [P, 6], dL_dsh [P, M, 3],
// dL_dscales [P, 3], dL_drotations [P, 4].
int ref_backward(void* handle, int P, int D, int M, const float* background, int W, int H, const float* means3D, const float* shs,
                 const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                 float tan_fovy, const int* radii, const float* dL_dpix, float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity,
                 float* dL_dcolors, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations)
{
    Handle* h = static_cast<Handle*>(handle);
    const size_t p = static_cast<size_t>(P), N = static_cast<size_t>(W) * static_cast<size_t>(H), m = static_cast<size_t>(M);
    Arena a;
    float* g_m2 = a.zeros<float>(3 * p);
    float* g_con = a.zeros<float>(4 * p);
    float* g_op = a.zeros<float>(p);
    float* g_col = a.zeros<float>(3 * p);
    float* g_m3 = a.zeros<float>(3 * p);
    float* g_cov = a.zeros<float>(6 * p);
    float* g_sh = a.zeros<float>(3 * p * m);
    float* g_sc = a.zeros<float>(3 * p);
    float* g_rot = a.zeros<float>(4 * p);
    REF_TRY(a.err);
    if (P != 0) {
        if (h == nullptr || h->P != P || h->W != W || h->H != H) return -2;
        const float* d_bg = a.upload(background, 3);
        const float* d_means = a.upload(means3D, 3 * p);
        const float* d_shs = a.upload(shs, 3 * p * m);
        const float* d_pre = a.upload(colors_precomp, 3 * p);
        const float* d_scales = a.upload(scales, 3 * p);
        const float* d_rot = a.upload(rotations, 4 * p);
        const float* d_cov = a.upload(cov3D_precomp, 6 * p);
        const float* d_view = a.upload(viewmatrix, 16);
        const float* d_proj = a.upload(projmatrix, 16);
        const float* d_cam = a.upload(campos, 3);
        const int* d_radii = a.upload(radii, p);
        const float* d_pix = a.upload(dL_dpix, 3 * N);
        REF_TRY(a.err);
        try {
            CudaRasterizer::Rasterizer::backward(P, D, M, h->R, d_bg, W, H, d_means, d_shs, d_pre, d_scales, scale_modifier, d_rot, d_cov,
                                                 d_view, d_proj, d_cam, tan_fovx, tan_fovy, d_radii, h->geom, h->binning, h->img, d_pix,
                                                 g_m2, g_con, g_op, g_col, g_m3, g_cov, g_sh, g_sc, g_rot);
        } catch (const std::exception&) {
            (void)hipDeviceSynchronize();
            return -2;
        }
    }
    REF_TRY(sync_and_last_error());
    REF_TRY(download(dL_dmeans2D, g_m2, 3 * p));
    REF_TRY(download(dL_dconic, g_con, 4 * p));
    REF_TRY(download(dL_dopacity, g_op, p));
    REF_TRY(download(dL_dcolors, g_col, 3 * p));
    REF_TRY(download(dL_dmeans3D, g_m3, 3 * p));
    REF_TRY(download(dL_dcov3D, g_cov, 6 * p));
    REF_TRY(download(dL_dsh, g_sh, 3 * p * m));
    REF_TRY(download(dL_dscales, g_sc, 3 * p));
    REF_TRY(download(dL_drotations, g_rot, 4 * p));
    return 0;
}

// present [P] (bytes): the reference's coarse frustum test, false-filled first as the binding's torch::full.
int ref_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present)
{
    static_assert(sizeof(bool) == 1, "present is downloaded as bytes");
    const size_t p = static_cast<size_t>(P);
    Arena a;
    bool* d_present = a.zeros<bool>(p);
    REF_TRY(a.err);
    if (P != 0) {
        float* d_means = a.upload(const_cast<float*>(means3D), 3 * p);
        float* d_view = a.upload(const_cast<float*>(viewmatrix), 16);
        float* d_proj = a.upload(const_cast<float*>(projmatrix), 16);
        REF_TRY(a.err);
        CudaRasterizer::Rasterizer::markVisible(P, d_means, d_view, d_proj, d_present);
    }
    REF_TRY(sync_and_last_error());
    REF_TRY(download(present, d_present, p));
    return 0;
}

void ref_free(void* handle) { release(static_cast<Handle*>(handle)); }

}  // extern "C"
