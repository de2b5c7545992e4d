// nca_view.hip -- the inference side of the C ABI (include/nerfca_hip.h, "view rendering"): rays of any C-arm view generated on the
// device, the composition of two single-field renders into the three images the reference's display block logs, and the per-image
// min / max normalisation it applies before logging (train/run_composite.py:361, 405-413).  Forward only, no MLP here: the static
// field is rendered by nca_render_fwd in single-field mode, the dynamic field by nca_mlp_fwd on the query points made here and
// nca_composite_fwd.  This translation unit keeps its own thread-local error message (nca_view_last_error): it shares no state with
// nca_api.hip or the other sections; the message type and the launch epilogue are nca_view_common.hpp's.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_view_last_error(void) { return g_err.msg; }

constexpr int VIEW_BLOCK = 256;

// ---- rays of one view ------------------------------------------------------------------------------------------------------------
// train/proj_helpers.get_ray_values_tigre in its own order, every operation a rounded f32 one (the build has -ffp-contract=off;
// the explicit _rn intrinsics keep that true whatever the flags).  One thread per pixel p = w*H + h.
template <typename OUT>
__global__ void __launch_bounds__(VIEW_BLOCK) view_rays_kernel(NcaView v, int64_t p0, int64_t n, OUT* __restrict__ origins, OUT* __restrict__ dirs) {
    const int64_t i = (int64_t)blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t p = p0 + i;
    const int32_t w = (int32_t)(p / v.H), h = (int32_t)(p % v.H);
    const float half_w = __fmul_rn((float)v.W, 0.5f), half_h = __fmul_rn((float)v.H, 0.5f);
    const float u = __fadd_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)w, 0.5f), half_w), v.d_det[0]), v.off_det[0]);
    const float t = __fadd_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)h, 0.5f), half_h), v.d_det[1]), v.off_det[1]);
    const float lx = __fdiv_rn(u, v.dsd), ly = __fdiv_rn(t, v.dsd);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float* row = v.pose + 4 * r;
        const float d = __fadd_rn(__fadd_rn(__fmul_rn(row[0], lx), __fmul_rn(row[1], ly)), row[2]);
        dirs[3 * i + r] = (OUT)d;
        origins[3 * i + r] = (OUT)row[3];
    }
}

extern "C" int nca_view_rays(const NcaView* view, int64_t p0, int64_t n, int32_t out_f64, void* origins, void* dirs, void* stream) {
    if (!view) return g_err.fail(NCA_E_INVALID, "nca_view_rays: the view descriptor is NULL");
    if (view->W <= 0 || view->H <= 0) return g_err.fail(NCA_E_INVALID, "nca_view_rays: detector %d x %d is not positive", (int)view->W, (int)view->H);
    if (n <= 0) return g_err.fail(NCA_E_INVALID, "nca_view_rays: n = %lld is not positive", (long long)n);
    if (p0 < 0) return g_err.fail(NCA_E_INVALID, "nca_view_rays: p0 = %lld is negative", (long long)p0);
    const int64_t npix = (int64_t)view->W * view->H;
    if (p0 > npix || n > npix - p0)
        return g_err.fail(NCA_E_INVALID, "nca_view_rays: pixels [%lld, %lld + %lld) leave the %lld of the detector", (long long)p0, (long long)p0, (long long)n, (long long)npix);
    if (!origins || !dirs) return g_err.fail(NCA_E_INVALID, "nca_view_rays: an output pointer is NULL");
    const int64_t blocks = (n + VIEW_BLOCK - 1) / VIEW_BLOCK;
    if (blocks > 0x7fffffffLL) return g_err.fail(NCA_E_INVALID, "nca_view_rays: n = %lld is more than one launch covers", (long long)n);
    const dim3 grid((unsigned)blocks);
    if (out_f64)
        hipLaunchKernelGGL(view_rays_kernel<double>, grid, dim3(VIEW_BLOCK), 0, (hipStream_t)stream, *view, p0, n, (double*)origins, (double*)dirs);
    else
        hipLaunchKernelGGL(view_rays_kernel<float>, grid, dim3(VIEW_BLOCK), 0, (hipStream_t)stream, *view, p0, n, (float*)origins, (float*)dirs);
    return nca_launched(g_err, "nca_view_rays");
}

// ---- query points of a ray chunk ----------------------------------------------------------------------------------------------------
// pts[r][s] = f32(o[r] + d[r] z[s]) exactly as the fused render kernels form a sample's query point from f64 rays (the sum in f64, rounded
// once).  The dynamic net is evaluated on these through the point forward, once per phase: the render
// forward binds time latents to its second net only, so a dynamic net cannot run there in single-field mode.  One thread per coordinate.
__global__ void __launch_bounds__(VIEW_BLOCK) view_points_kernel(int64_t total, int32_t S, const double* __restrict__ origins, const double* __restrict__ dirs,
                                                                 const float* __restrict__ z, float* __restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int64_t smp = i / 3;
    const int c = (int)(i - smp * 3);
    const int64_t ray = smp / S;
    const float zz = z[smp - ray * S];
    pts[i] = (float)__dadd_rn(origins[ray * 3 + c], __dmul_rn(dirs[ray * 3 + c], (double)zz));
}

extern "C" int nca_view_points(int64_t R, int32_t S, const double* origins, const double* dirs, const float* z, float* pts, void* stream) {
    if (R <= 0 || S <= 0) return g_err.fail(NCA_E_INVALID, "nca_view_points: %lld rays x %d samples is not positive", (long long)R, (int)S);
    if (!origins || !dirs || !z) return g_err.fail(NCA_E_INVALID, "nca_view_points: an input pointer is NULL");
    if (!pts) return g_err.fail(NCA_E_INVALID, "nca_view_points: the output pointer is NULL");
    if (R > (INT64_MAX / 3) / S) return g_err.fail(NCA_E_INVALID, "nca_view_points: %lld rays x %d samples overflows", (long long)R, (int)S);
    const int64_t total = R * S * 3, blocks = (total + VIEW_BLOCK - 1) / VIEW_BLOCK;
    if (blocks > 0x7fffffffLL) return g_err.fail(NCA_E_INVALID, "nca_view_points: %lld rays x %d samples is more than one launch covers", (long long)R, (int)S);
    const dim3 grid((unsigned)blocks);
    hipLaunchKernelGGL(view_points_kernel, grid, dim3(VIEW_BLOCK), 0, (hipStream_t)stream, total, S, origins, dirs, z, pts);
    return nca_launched(g_err, "nca_view_points");
}

// ---- composite / static / dynamic image from two single-field renders ------------------------------------------------------------
// Each single-field pix is already I0 - sum(sigma dists scale); the composite of the reference is I0 - sum((s + d) dists), so the two
// add up to it once one I0 is taken off again.  f64 in exactly this order, rounded to f32 once.
template <typename IN>
__global__ void __launch_bounds__(VIEW_BLOCK) view_compose_kernel(int64_t n, double i0, const IN* __restrict__ pix_s, const IN* __restrict__ pix_d,
                                                                  float* __restrict__ pred, float* __restrict__ pred_s, float* __restrict__ pred_d) {
    const int64_t i = (int64_t)blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double s = (double)pix_s[i];
    const float fs = (float)s;
    pred_s[i] = fs;
    if (pix_d) {
        const double d = (double)pix_d[i];
        pred[i] = (float)(__dsub_rn(__dadd_rn(s, d), i0));
        pred_d[i] = (float)d;
    } else {
        pred[i] = fs;
        pred_d[i] = (float)i0;
    }
}

extern "C" int nca_view_compose(int64_t n, double i0, const void* pix_s, const void* pix_d, int32_t pix_is_f64, float* pred, float* pred_s,
                                float* pred_d, void* stream) {
    if (n <= 0) return g_err.fail(NCA_E_INVALID, "nca_view_compose: n = %lld is not positive", (long long)n);
    if (!pix_s) return g_err.fail(NCA_E_INVALID, "nca_view_compose: pix_s is NULL");
    if (!pred || !pred_s || !pred_d) return g_err.fail(NCA_E_INVALID, "nca_view_compose: an output pointer is NULL");
    const int64_t blocks = (n + VIEW_BLOCK - 1) / VIEW_BLOCK;
    if (blocks > 0x7fffffffLL) return g_err.fail(NCA_E_INVALID, "nca_view_compose: n = %lld is more than one launch covers", (long long)n);
    const dim3 grid((unsigned)blocks);
    if (pix_is_f64)
        hipLaunchKernelGGL(view_compose_kernel<double>, grid, dim3(VIEW_BLOCK), 0, (hipStream_t)stream, n, i0, (const double*)pix_s, (const double*)pix_d,
                           pred, pred_s, pred_d);
    else
        hipLaunchKernelGGL(view_compose_kernel<float>, grid, dim3(VIEW_BLOCK), 0, (hipStream_t)stream, n, i0, (const float*)pix_s, (const float*)pix_d,
                           pred, pred_s, pred_d);
    return nca_launched(g_err, "nca_view_compose");
}

// ---- per-image min / max and (x - min) / (max - min) -----------------------------------------------------------------------------
// Three launches, no atomics: (1) 256-thread blocks walk one image with a grid-stride loop, reduce in the wave by shuffles and across
// the four waves through LDS, and leave one (min, max) per block in the workspace; (2) one block per image folds those partials in a
// fixed order into minmax; (3) the scaling pass.  The order of every fold is a function of (n, n_img) alone, so two runs give the same
// bits.  min and max are exact whatever the order.  A NaN pixel makes both min and max of its image NaN, as torch.min / torch.max and
// trainer.normalize_image do (fminf / fmaxf alone would skip it); the scaled image is then NaN throughout, as there.
constexpr int NORM_ELEMS_PER_BLOCK = VIEW_BLOCK * 8;      // pixels one block of pass 1 is sized for
constexpr int NORM_MAX_BLOCKS = 1024;                      // per image: pass 2 folds at most 4 partials per thread

static int64_t norm_blocks(int64_t n) {
    const int64_t b = (n + NORM_ELEMS_PER_BLOCK - 1) / NORM_ELEMS_PER_BLOCK;
    return b < 1 ? 1 : (b > NORM_MAX_BLOCKS ? NORM_MAX_BLOCKS : b);
}

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : fminf(a, b)); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
    __shared__ float s_lo[VIEW_BLOCK / 64], s_hi[VIEW_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {          // wave 64: six steps
        lo = nan_min(lo, __shfl_down(lo, off, 64));
        hi = nan_max(hi, __shfl_down(hi, off, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < VIEW_BLOCK / 64; ++k) { lo = nan_min(lo, s_lo[k]); hi = nan_max(hi, s_hi[k]); }
    }
}

__global__ void __launch_bounds__(VIEW_BLOCK) norm_partial_kernel(int64_t n, int32_t blocks, const float* __restrict__ img, float2* __restrict__ part) {
    const float* x = img + (int64_t)blockIdx.y * n;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * VIEW_BLOCK + threadIdx.x; i < n; i += (int64_t)blocks * VIEW_BLOCK) {
        const float v = x[i];
        lo = nan_min(lo, v);
        hi = nan_max(hi, v);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * blocks + blockIdx.x] = make_float2(lo, hi);
}

__global__ void __launch_bounds__(VIEW_BLOCK) norm_finish_kernel(int32_t blocks, const float2* __restrict__ part, float* __restrict__ minmax) {
    const float2* p = part + (int64_t)blockIdx.x * blocks;
    float lo = INFINITY, hi = -INFINITY;
    for (int k = threadIdx.x; k < blocks; k += VIEW_BLOCK) {
        lo = nan_min(lo, p[k].x);
        hi = nan_max(hi, p[k].y);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) { minmax[2 * blockIdx.x] = lo; minmax[2 * blockIdx.x + 1] = hi; }
}

__global__ void __launch_bounds__(VIEW_BLOCK) norm_scale_kernel(int64_t n, const float* __restrict__ img, const float* __restrict__ minmax, float* __restrict__ out) {
    const float lo = minmax[2 * blockIdx.y], hi = minmax[2 * blockIdx.y + 1];
    const float span = __fsub_rn(hi, lo);
    const float* x = img + (int64_t)blockIdx.y * n;
    float* y = out + (int64_t)blockIdx.y * n;
    for (int64_t i = (int64_t)blockIdx.x * VIEW_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VIEW_BLOCK)
        y[i] = span == 0.0f ? 0.0f : __fdiv_rn(__fsub_rn(x[i], lo), span);       // a constant image: zeros (the reference's expression gives 0/0); a NaN span stays NaN
}

extern "C" int64_t nca_image_normalize_workspace(int64_t n) {
    if (n <= 0) return g_err.fail(NCA_E_INVALID, "nca_image_normalize_workspace: n = %lld is not positive", (long long)n);
    const int64_t bytes = norm_blocks(n) * (int64_t)sizeof(float2);
    return (bytes + 255) / 256 * 256;
}

extern "C" int nca_image_normalize(int32_t n_img, int64_t n, const float* img, float* out, float* minmax, void* work, int64_t work_bytes, void* stream) {
    if (n_img <= 0) return g_err.fail(NCA_E_INVALID, "nca_image_normalize: n_img = %d is not positive", (int)n_img);
    if (n_img > 65535) return g_err.fail(NCA_E_INVALID, "nca_image_normalize: n_img = %d is more than 65535 images a call", (int)n_img);
    if (n <= 0) return g_err.fail(NCA_E_INVALID, "nca_image_normalize: n = %lld is not positive", (long long)n);
    if (!img) return g_err.fail(NCA_E_INVALID, "nca_image_normalize: img is NULL");
    if (!minmax) return g_err.fail(NCA_E_INVALID, "nca_image_normalize: minmax is NULL");
    const int64_t need = (int64_t)n_img * nca_image_normalize_workspace(n);
    if (!work || work_bytes < need)
        return g_err.fail(NCA_E_WORKSPACE, "nca_image_normalize: workspace of %lld bytes, %lld needed (n_img x nca_image_normalize_workspace)", (long long)(work ? work_bytes : 0),
                     (long long)need);
    const int32_t blocks = (int32_t)norm_blocks(n);
    float2* part = (float2*)work;
    hipLaunchKernelGGL(norm_partial_kernel, dim3(blocks, n_img), dim3(VIEW_BLOCK), 0, (hipStream_t)stream, n, blocks, img, part);
    hipLaunchKernelGGL(norm_finish_kernel, dim3(n_img), dim3(VIEW_BLOCK), 0, (hipStream_t)stream, blocks, (const float2*)part, minmax);
    if (out) hipLaunchKernelGGL(norm_scale_kernel, dim3(blocks, n_img), dim3(VIEW_BLOCK), 0, (hipStream_t)stream, n, img, (const float*)minmax, out);
    return nca_launched(g_err, "nca_image_normalize");
}
