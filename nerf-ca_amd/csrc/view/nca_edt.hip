// nca_edt.hip -- the exact Euclidean distance transform of thresholded voxel stacks (include/nerfca_hip.h, "edt"): metrics.distance_transform
// and the vessel distances built on it.  Separable, three launches: the integer distance g to the nearest feature of a row (one wave per
// row, features as ballot masks), then the lower envelope min_j (w d^2 + f(j)) along axis 1 and along axis 0 by a pruned outward search over
// a line staged in LDS.  Every node of every stage is written once by one thread: no atomics, the same bits on every run.  This translation
// unit keeps its own thread-local error message (nca_edt_last_error): it shares no state with the other sections.  The grid checks and the
// workspace refusal are nca_view_common.hpp's; the limit on an axis is checked here, after them.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_edt_last_error(void) { return g_err.msg; }

constexpr int ED_BLOCK = 256, ED_WAVES = ED_BLOCK / 64;
constexpr int ED_CHUNKS = NCA_EDT_MAX_AXIS / 64;          // ballot masks of the longest row
constexpr int ED_TC = 16;                                 // columns of a line tile
constexpr int ED_TL = ED_BLOCK / ED_TC;                   // nodes along the line the block takes per step
constexpr int32_t ED_NONE = 0x7fffffff;                   // g of a row without a feature
constexpr int64_t ED_MAX_BLOCKS = (1LL << 32) / ED_BLOCK;          // a launch carries at most 2^32 threads
static_assert(NCA_EDT_MAX_AXIS % 64 == 0, "a row is whole chunks of 64 nodes");
static_assert((size_t)NCA_EDT_MAX_AXIS * ED_TC * sizeof(double) <= 65536, "the longest line tile fits the LDS of one workgroup");
static_assert(ED_TC == 16 && ED_TL == 16, "thread t owns column t & 15 and the nodes (t >> 4) + 16 k of the line");

// The row pass.  Wave w of a block owns row 4 blockIdx.x + w of the `rows` = n_vol n0 n1 rows of n2 nodes.  The features of chunk c of
// the row (nodes 64 c .. 64 c + 63) are one ballot mask, kept in LDS; the nearest feature at or before / at or after a node is the highest
// / lowest set bit of the masked word of its own chunk, else of the nearest chunk with any bit on that side (the carry).  A wave past the
// last row loads and stores nothing but takes every barrier.
__global__ void __launch_bounds__(ED_BLOCK) edt_row_kernel(int64_t rows, int32_t n2, const float* __restrict__ vol, double threshold, int32_t invert,
                                                           int32_t* __restrict__ gout) {
    __shared__ unsigned long long s_mask[ED_WAVES][ED_CHUNKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row = (int64_t)blockIdx.x * ED_WAVES + wave;
    const bool live = row < rows;
    const int nch = (n2 + 63) >> 6;
    const float* p = vol + (live ? row : 0) * n2;
    for (int c = 0; c < nch; ++c) {
        const int i2 = c * 64 + lane;
        bool feat = false;
        if (live && i2 < n2) feat = ((double)p[i2] > threshold) != (invert != 0);          // a NaN is not > threshold
        const unsigned long long m = __ballot(feat);
        if (lane == 0) s_mask[wave][c] = m;
    }
    __syncthreads();
    int32_t* q = gout + (live ? row : 0) * n2;
    for (int c = 0; c < nch; ++c) {
        const int i2 = c * 64 + lane;
        const unsigned long long m = s_mask[wave][c];
        const unsigned long long le = m & (~0ull >> (63 - lane)), ge = m & (~0ull << lane);
        int32_t left = ED_NONE, right = ED_NONE;
        if (le) {
            left = lane - (63 - __clzll((long long)le));
        } else {
            for (int cc = c - 1; cc >= 0; --cc) {
                const unsigned long long mm = s_mask[wave][cc];
                if (mm) {
                    left = i2 - (cc * 64 + 63 - __clzll((long long)mm));
                    break;
                }
            }
        }
        if (ge) {
            right = (__ffsll((unsigned long long)ge) - 1) - lane;
        } else {
            for (int cc = c + 1; cc < nch; ++cc) {
                const unsigned long long mm = s_mask[wave][cc];
                if (mm) {
                    right = cc * 64 + (__ffsll((unsigned long long)mm) - 1) - i2;
                    break;
                }
            }
        }
        if (live && i2 < n2) q[i2] = min(left, right);
    }
}

// One step of the separable minimum along an axis of `len` nodes: out(i, c) = min over j of (w (double)((i - j)^2) + f(j, c)) for the lines
// c = 0 .. cols - 1 of slab `o`, element (o, j, c) at (o len + j) cols + c.  A block owns 16 consecutive lines of one slab: f for all of them
// is staged in LDS as f64 [len][16] (+inf for a line past the end), then thread t takes line t & 15 and the nodes (t >> 4) + 16 k.
// FIRST: the input is the row pass's int32 g and f = wf (double)((int64)g g), +inf for a row without a feature; the output is f64.
// !FIRST: the input is that f64; the output is (float)sqrt(min).
// A line whose f is +inf throughout is written as +inf without a search (it would run to both ends and find nothing).
// The search runs outward from i, d = 1, 2, ..: t = w (double)(d d) grows with d and every candidate is t + f >= t (f >= 0, rounding is
// monotone), so it stops at the first t >= best without changing a bit.  No thread returns early: the barrier is safe.
template <bool FIRST>
__global__ void __launch_bounds__(ED_BLOCK) edt_line_kernel(int32_t len, int64_t cols, int64_t col_tiles, double w, double wf, const void* __restrict__ in,
                                                            void* __restrict__ out) {
    extern __shared__ double s_f[];          // [len][ED_TC]
    __shared__ int s_some[ED_TC];            // does line c hold any finite f?
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t o = bid / col_tiles, c0 = (bid % col_tiles) * ED_TC;
    const int64_t base = o * len * cols;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    if (tid < ED_TC) s_some[tid] = 0;
    __syncthreads();
    for (int idx = tid; idx < len * ED_TC; idx += ED_BLOCK) {
        const int j = idx / ED_TC;
        const int64_t c = c0 + (idx % ED_TC);
        double f = inf;
        if (c < cols) {
            const int64_t at = base + (int64_t)j * cols + c;
            if constexpr (FIRST) {
                const int32_t g = ((const int32_t*)in)[at];
                if (g != ED_NONE) f = __dmul_rn(wf, (double)((int64_t)g * (int64_t)g));
            } else {
                f = ((const double*)in)[at];
            }
        }
        s_f[idx] = f;
        if (f < inf) s_some[idx % ED_TC] = 1;          // every writer stores the same value
    }
    __syncthreads();

    const int tc = tid & (ED_TC - 1);
    const int64_t c = c0 + tc;
    if (c < cols) {
        const bool some = s_some[tc] != 0;          // a line without a feature is +inf at every node: there is nothing to search
        for (int i = tid / ED_TC; i < len; i += ED_TL) {
            double best = s_f[i * ED_TC + tc];
            const int reach = some ? max(i, len - 1 - i) : 0;
            for (int d = 1; d <= reach; ++d) {
                const double t = __dmul_rn(w, (double)((int64_t)d * (int64_t)d));
                if (t >= best) break;
                if (i - d >= 0) best = fmin(best, __dadd_rn(t, s_f[(i - d) * ED_TC + tc]));
                if (i + d < len) best = fmin(best, __dadd_rn(t, s_f[(i + d) * ED_TC + tc]));
            }
            const int64_t at = base + (int64_t)i * cols + c;
            if constexpr (FIRST)
                ((double*)out)[at] = best;
            else
                ((float*)out)[at] = (float)__dsqrt_rn(best);
        }
    }
}

// The checks the query and the entry point share: the 12 bytes per node of the workspace (and the 4 of the volumes) must fit int64.
static int edt_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    return nca_check_stack(g_err, who, grid, n_vol, "n_vol", 16, "volumes", NCA_EDT_MAX_AXIS, g, nodes);
}

extern "C" size_t nca_vol_edt_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes;
    if (edt_check("nca_vol_edt_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    return ((size_t)nodes * 12 + 255) / 256 * 256;
}

extern "C" int nca_vol_edt(const NcaGrid* grid, const float* vol, int32_t n_vol, double threshold, int32_t invert, float* out, void* work, size_t work_bytes,
                           void* stream) {
    const char* who = "nca_vol_edt";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, out);
    if (invert != 0 && invert != 1) return g_err.fail(NCA_E_INVALID, "%s: invert = %d is neither 0 nor 1", who, (int)invert);
    if (threshold != threshold) return g_err.fail(NCA_E_INVALID, "%s: threshold = %g is not a number", who, threshold);
    NcaGrid g;
    int64_t nodes;
    const int rc = edt_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const int64_t rows = (int64_t)n_vol * n0 * n1, plane = (int64_t)n1 * n2;
    const int64_t blocks_r = (rows + ED_WAVES - 1) / ED_WAVES;
    const int64_t tiles_1 = (n2 + ED_TC - 1) / ED_TC, blocks_1 = (int64_t)n_vol * n0 * tiles_1;
    const int64_t tiles_0 = (plane + ED_TC - 1) / ED_TC, blocks_0 = (int64_t)n_vol * tiles_0;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, blocks_r, blocks_1, blocks_0, ED_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_edt_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    double w[3];
    for (int a = 0; a < 3; ++a) {
        const double h = 1.0 / g.inv[a];
        w[a] = h * h;
    }
    double* b = (double*)work;                         // f64 [nodes], then int32 [nodes]
    int32_t* gd = (int32_t*)(b + nodes);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)blocks_r), dim3(ED_BLOCK), 0, s, rows, n2, vol, threshold, invert, gd);
    hipLaunchKernelGGL((edt_line_kernel<true>), dim3((unsigned)blocks_1), dim3(ED_BLOCK), (size_t)n1 * ED_TC * sizeof(double), s, n1, (int64_t)n2, tiles_1, w[1], w[2],
                       (const void*)gd, (void*)b);
    hipLaunchKernelGGL((edt_line_kernel<false>), dim3((unsigned)blocks_0), dim3(ED_BLOCK), (size_t)n0 * ED_TC * sizeof(double), s, n0, plane, tiles_0, w[0], 0.0,
                       (const void*)b, (void*)out);
    return nca_launched(g_err, who);
}
