// nca_vess.hip -- the multi-scale Hessian vesselness of voxel stacks (include/nerfca_hip.h, "vess"): ccta.hessian_eigenvalues and
// ccta.vesselness.
//
// One kernel in three modes, one launch per call and scale.  A workgroup owns a tile of 4 x 8 x 64 nodes (nca_view_common.hpp) and stages
// the smoothed volume on the tile grown by one node in LDS; a staged node outside the grid holds the value of the nearest node inside
// (every index clamped on its own axis), so the stencil below needs no bounds.  Each thread then takes its four nodes in turn: the 19-point
// stencil from LDS, the Hessian in f64, five sweeps of cyclic Jacobi in registers, the sort, and what the mode asks for -- the three
// eigenvalues, the vesselness with its merge over scales, or the largest squared norm.  A node is written by the one thread that owns it.
// The maximum is taken per thread, per workgroup in an LDS tree, and across workgroups with one integer atomicMax per workgroup on the bit
// pattern of a non-negative double: exact in any order, the same bits on every run.
//
// Every f64 operation is spelled as the header spells it and the build has -ffp-contract=off: a transcription has the same bits up to exp.
//
// This translation unit keeps its own thread-local error message (nca_vess_last_error): it shares no state with the other sections.  The
// grid checks, the tile count and the launch epilogue are nca_view_common.hpp's.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_vess_last_error(void) { return g_err.msg; }

constexpr int VS_S0 = NCA_TILE0 + 2, VS_S1 = NCA_TILE1 + 2, VS_S2 = NCA_TILE2 + 2;          // the tile and a halo of one node
constexpr int VS_SWEEPS = 5;
constexpr int64_t VS_MAX_BLOCKS = 0x7fffffffLL;
static_assert((size_t)(VS_S0 * VS_S1 * VS_S2) * sizeof(float) + NCA_TILE_BLOCK * sizeof(double) <= 65536, "the tile and the tree fit the LDS of one workgroup");

enum { VS_EIG = 0, VS_NORM = 1, VS_VESS = 2 };

// one Jacobi rotation of the pair (p, q): app, aqq, apq its entries, arp and arq the third row's
__device__ __forceinline__ void vs_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double tp = t * apq;
    app = app - tp;
    aqq = aqq + tp;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
}

// x and y, x in the earlier position, change places iff |y| < |x|, or |y| == |x| and y < x
__device__ __forceinline__ void vs_order(double& x, double& y) {
    const double ax = fabs(x), ay = fabs(y);
    if (ay < ax || (ay == ax && y < x)) {
        const double z = x;
        x = y;
        y = z;
    }
}

// The sorted eigenvalues of the Hessian at the node whose staged value is t[0][0][0] (t points into the LDS tile); false, and nothing
// computed, when an entry of the Hessian is not finite.
__device__ __forceinline__ bool vs_eigen(const float (*t)[VS_S1][VS_S2], int j0, int j1, int j2, double scale, double l[3]) {
#define VS_AT(d0, d1, d2) ((double)t[j0 + (d0)][j1 + (d1)][j2 + (d2)])
    const double v = VS_AT(0, 0, 0);
    double a00 = scale * ((VS_AT(1, 0, 0) - v) - (v - VS_AT(-1, 0, 0)));
    double a11 = scale * ((VS_AT(0, 1, 0) - v) - (v - VS_AT(0, -1, 0)));
    double a22 = scale * ((VS_AT(0, 0, 1) - v) - (v - VS_AT(0, 0, -1)));
    double a01 = scale * (0.25 * ((VS_AT(1, 1, 0) - VS_AT(1, -1, 0)) - (VS_AT(-1, 1, 0) - VS_AT(-1, -1, 0))));
    double a02 = scale * (0.25 * ((VS_AT(1, 0, 1) - VS_AT(1, 0, -1)) - (VS_AT(-1, 0, 1) - VS_AT(-1, 0, -1))));
    double a12 = scale * (0.25 * ((VS_AT(0, 1, 1) - VS_AT(0, 1, -1)) - (VS_AT(0, -1, 1) - VS_AT(0, -1, -1))));
#undef VS_AT
    if (!(isfinite(a00) && isfinite(a01) && isfinite(a02) && isfinite(a11) && isfinite(a12) && isfinite(a22))) return false;
#pragma unroll 1
    for (int sweep = 0; sweep < VS_SWEEPS; ++sweep) {
        vs_rotate(a00, a11, a01, a02, a12);          // (0,1), r = 2
        vs_rotate(a00, a22, a02, a01, a12);          // (0,2), r = 1
        vs_rotate(a11, a22, a12, a01, a02);          // (1,2), r = 0
    }
    vs_order(a00, a11);
    vs_order(a11, a22);
    vs_order(a00, a11);
    l[0] = a00;
    l[1] = a11;
    l[2] = a22;
    return true;
}

// f32 of an eigenvalue; a NaN becomes the canonical quiet NaN
__device__ __forceinline__ float vs_f32(double x) { return (x != x) ? __int_as_float(0x7fc00000) : (float)x; }

// Block b owns tile b % tiles of volume b / tiles.  Wave w stages the rows w, w + 8, .. of the tile, its 64 lanes along the contiguous
// axis.  No thread returns before the last barrier.  MODE VS_EIG: out = eig.  VS_NORM: norm_max, zeroed before the launch.  VS_VESS: out,
// scale_out (or NULL), c, ta = 2 alpha^2, tb = 2 beta^2, bright, scale_index.
template <int MODE>
__global__ void __launch_bounds__(NCA_TILE_BLOCK) vess_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t tiles, int32_t nb1, int32_t nb2,
                                                              const float* __restrict__ in, double scale, float* __restrict__ out, int32_t* __restrict__ scale_out,
                                                              unsigned long long* __restrict__ norm_max, const double* __restrict__ c, double ta, double tb,
                                                              int32_t bright, int32_t scale_index) {
    __shared__ float s_t[VS_S0][VS_S1][VS_S2];          // s at clamp(base - 1 + l) per axis
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / tiles;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    const float* __restrict__ x = in + v * voxels;

    for (int r = wave; r < VS_S0 * VS_S1; r += NCA_TILE_WAVES) {
        const int l0 = r / VS_S1, l1 = r % VS_S1;
        const int32_t g0 = min(max(tile.base0 - 1 + l0, 0), n0 - 1), g1 = min(max(tile.base1 - 1 + l1, 0), n1 - 1);
        const int64_t row = ((int64_t)g0 * n1 + g1) * n2;
        for (int cc = lane; cc < VS_S2; cc += 64) {
            const int32_t g2 = min(max(tile.base2 - 1 + cc, 0), n2 - 1);          // every index inside the grid: no load out of bounds
            s_t[l0][l1][cc] = x[row + g2];
        }
    }
    __syncthreads();

    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    double tc = 0.0;
    if constexpr (MODE == VS_VESS) {
        const double cv = c[v];
        tc = 2.0 * (cv * cv);
    }
    double most = 0.0;
#pragma unroll 1
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        if (!nodes.live(k)) continue;
        double l[3];
        const bool finite = vs_eigen(s_t, k + 1, wave + 1, lane + 1, scale, l);
        const int64_t off = nodes.off(k);
        if constexpr (MODE == VS_EIG) {
            float* __restrict__ e = out + v * 3 * voxels + off;
            const float nan = __int_as_float(0x7fc00000);
            e[0] = finite ? vs_f32(l[0]) : nan;
            e[voxels] = finite ? vs_f32(l[1]) : nan;
            e[2 * voxels] = finite ? vs_f32(l[2]) : nan;
        } else if constexpr (MODE == VS_NORM) {
            if (finite) {
                const double x1 = (double)vs_f32(l[0]), x2 = (double)vs_f32(l[1]), x3 = (double)vs_f32(l[2]);
                const double s2 = (x1 * x1 + x2 * x2) + x3 * x3;
                most = (s2 > most) ? s2 : most;
            }
        } else {
            float V = 0.0f;
            if (finite && (bright ? (l[1] < 0.0 && l[2] < 0.0) : (l[1] > 0.0 && l[2] > 0.0))) {
                const double q1 = l[0] * l[0], q2 = l[1] * l[1], q3 = l[2] * l[2];
                const double ra2 = q2 / q3, rb2 = q1 / fabs(l[1] * l[2]), s2 = (q1 + q2) + q3;
                const double A = 1.0 - exp(-ra2 / ta), B = exp(-rb2 / tb);
                const double C = (tc == 0.0) ? 1.0 : 1.0 - exp(-s2 / tc);
                V = (float)((A * B) * C);
            }
            const int64_t o = v * voxels + off;
            if (scale_index == 0 || V > out[o]) {
                out[o] = V;
                if (scale_out) scale_out[o] = scale_index;
            }
        }
    }

    if constexpr (MODE == VS_NORM) {          // the workgroup's maximum in a binary tree, then one atomicMax on the bit pattern (most >= +0, never a NaN)
        __shared__ double s_m[NCA_TILE_BLOCK];
        s_m[tid] = most;
        __syncthreads();
        for (int h = NCA_TILE_BLOCK / 2; h > 0; h >>= 1) {
            if (tid < h) {
                const double b = s_m[tid + h], a = s_m[tid];
                s_m[tid] = (b > a) ? b : a;
            }
            __syncthreads();
        }
        if (tid == 0 && s_m[0] > 0.0) atomicMax(norm_max + v, (unsigned long long)__double_as_longlong(s_m[0]));
    }
}

// What the three entry points share, after their own NULL refusals: the stack checks, the scale, and the blocks of the launch.
static int vess_check(const char* who, const NcaGrid* grid, int32_t n_vol, double scale, NcaGrid* g, int64_t* nodes) {
    const int rc = nca_check_stack(g_err, who, grid, n_vol, "n_vol", 16, "volumes", 0, g, nodes);          // 4 bytes of s and up to 12 of the outputs per node
    if (rc != NCA_OK) return rc;
    if (!(isfinite(scale) && scale > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: scale = %g is not finite and positive", who, scale);
    return NCA_OK;
}

static int vess_blocks(const char* who, const NcaGrid& g, int32_t n_vol, int32_t nb[3], int64_t* tiles) {
    const int rct = nca_count_tiles(g_err, who, g, 0, nb, tiles);
    if (rct != NCA_OK) return rct;
    return nca_check_launch_blocks(g_err, who, n_vol, g, *tiles * n_vol, 0, 0, VS_MAX_BLOCKS);          // both factors below 2^31
}

#define VS_REFUSE_SAME(who, p, s)                                                                                      \
    do {                                                                                                               \
        if ((const void*)(p) == (const void*)(s)) return g_err.fail(NCA_E_INVALID, "%s: " #p " is s: nothing is formed in place", who); \
    } while (0)

extern "C" int nca_vol_hessian_eig(const NcaGrid* grid, const float* s, int32_t n_vol, double scale, float* eig, void* stream) {
    const char* who = "nca_vol_hessian_eig";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, s);
    NCA_REFUSE_NULL(g_err, who, eig);
    VS_REFUSE_SAME(who, eig, s);
    NcaGrid g;
    int64_t nodes, tiles;
    int32_t nb[3];
    int rc = vess_check(who, grid, n_vol, scale, &g, &nodes);
    if (rc != NCA_OK) return rc;
    rc = vess_blocks(who, g, n_vol, nb, &tiles);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((vess_kernel<VS_EIG>), dim3((unsigned)(tiles * n_vol)), dim3(NCA_TILE_BLOCK), 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], nodes / n_vol, tiles,
                       nb[1], nb[2], s, scale, eig, (int32_t*)nullptr, (unsigned long long*)nullptr, (const double*)nullptr, 0.0, 0.0, 0, 0);
    return nca_launched(g_err, who);
}

__global__ __launch_bounds__(256) void vess_zero_kernel(unsigned long long* __restrict__ p, int32_t n) {
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) p[i] = 0ull;
}

extern "C" int nca_vol_hessian_norm_max(const NcaGrid* grid, const float* s, int32_t n_vol, double scale, double* norm_max, void* stream) {
    const char* who = "nca_vol_hessian_norm_max";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, s);
    NCA_REFUSE_NULL(g_err, who, norm_max);
    VS_REFUSE_SAME(who, norm_max, s);
    NcaGrid g;
    int64_t nodes, tiles;
    int32_t nb[3];
    int rc = vess_check(who, grid, n_vol, scale, &g, &nodes);
    if (rc != NCA_OK) return rc;
    rc = vess_blocks(who, g, n_vol, nb, &tiles);
    if (rc != NCA_OK) return rc;
    // the clear is a KERNEL on the stream, not hipMemsetAsync: a memset node captured into a HIP graph does not replay to what the eager call does
    // (tests/test_graph_replay_gpu.py), and a stale maximum would survive into every later replay on a dimmer volume
    hipLaunchKernelGGL(vess_zero_kernel, dim3((unsigned)((n_vol + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)norm_max, n_vol);          // +0.0 is all zero bits
    rc = nca_launched(g_err, who);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((vess_kernel<VS_NORM>), dim3((unsigned)(tiles * n_vol)), dim3(NCA_TILE_BLOCK), 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], nodes / n_vol, tiles,
                       nb[1], nb[2], s, scale, (float*)nullptr, (int32_t*)nullptr, (unsigned long long*)norm_max, (const double*)nullptr, 0.0, 0.0, 0, 0);
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_vesselness(const NcaGrid* grid, const float* s, int32_t n_vol, double scale, double alpha, double beta, const double* c, int32_t bright,
                                  int32_t scale_index, float* out, int32_t* scale_out, void* stream) {
    const char* who = "nca_vol_vesselness";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, s);
    NCA_REFUSE_NULL(g_err, who, c);
    NCA_REFUSE_NULL(g_err, who, out);
    VS_REFUSE_SAME(who, out, s);
    VS_REFUSE_SAME(who, scale_out, s);
    NcaGrid g;
    int64_t nodes, tiles;
    int32_t nb[3];
    int rc = vess_check(who, grid, n_vol, scale, &g, &nodes);
    if (rc != NCA_OK) return rc;
    if (!(isfinite(alpha) && alpha > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: alpha = %g is not finite and positive", who, alpha);
    if (!(isfinite(beta) && beta > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: beta = %g is not finite and positive", who, beta);
    if (bright != 0 && bright != 1) return g_err.fail(NCA_E_INVALID, "%s: bright = %d is neither 0 nor 1", who, (int)bright);
    if (scale_index < 0) return g_err.fail(NCA_E_INVALID, "%s: scale_index = %d is negative", who, (int)scale_index);
    rc = vess_blocks(who, g, n_vol, nb, &tiles);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((vess_kernel<VS_VESS>), dim3((unsigned)(tiles * n_vol)), dim3(NCA_TILE_BLOCK), 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], nodes / n_vol, tiles,
                       nb[1], nb[2], s, scale, out, scale_out, (unsigned long long*)nullptr, c, 2.0 * (alpha * alpha), 2.0 * (beta * beta), bright, scale_index);
    return nca_launched(g_err, who);
}
