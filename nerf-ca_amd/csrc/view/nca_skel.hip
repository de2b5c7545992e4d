// nca_skel.hip -- the soft skeleton of voxel stacks and the sums of clDice (include/nerfca_hip.h, "skel"): metrics.soft_skeleton and
// metrics.cldice.
//
// Soft skeleton: K + 1 launches of one kernel.  Launch j reads E_j (the volume itself at j = 0) and writes E_{j+1} = erode(E_j) and the
// skeleton S, which lives in `out` and is updated in place.  A workgroup owns a tile of 4 x 8 x 64 nodes (nca_view_common.hpp).  It
// stages E_j on the tile grown by two nodes in LDS, +inf outside the grid; forms E_{j+1} on the tile grown by one node in LDS, -inf outside
// the grid; and then every thread takes the box maximum of E_{j+1} around its own four nodes, d = relu(E_j - open(E_j)) and the update of
// S.  A node of E_{j+1} and of S is written by the one thread that owns it: no atomics, the same bits on every run.  The comparisons are
// spelled out in the order of the definition, so a NaN and the sign of a zero come out as the header says.
//
// Overlap sums: per-workgroup sums of 4096 consecutive nodes of one volume in a fixed order, then one workgroup per volume that adds them
// in a fixed order.
//
// This translation unit keeps its own thread-local error message (nca_skel_last_error): it shares no state with the other sections.  The
// grid checks, the tile count, the workspace refusal and the launch epilogue are nca_view_common.hpp's.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_skel_last_error(void) { return g_err.msg; }

// ------------------------------------------------------------------------------------------------------------------------- soft skeleton
constexpr int SK_S0 = NCA_TILE0 + 4, SK_S1 = NCA_TILE1 + 4, SK_S2 = NCA_TILE2 + 4;          // E_j staged: the tile and a halo of two nodes
constexpr int SK_G0 = NCA_TILE0 + 2, SK_G1 = NCA_TILE1 + 2, SK_G2 = NCA_TILE2 + 2;          // E_{j+1}: the tile and a halo of one node
constexpr int64_t SK_MAX_BLOCKS = 0x7fffffffLL;
static_assert((size_t)(SK_S0 * SK_S1 * SK_S2 + SK_G0 * SK_G1 * SK_G2) * sizeof(float) <= 65536, "both tiles fit the LDS of one workgroup");

__device__ __forceinline__ float sk_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float sk_max(float a, float b) { return (b > a) ? b : a; }
__device__ __forceinline__ float sk_relu(float x) { return (x > 0.0f) ? x : 0.0f; }

// One launch: block b owns tile b % tiles of volume b / tiles.  `in` is E_j, `next` gets E_{j+1} (NULL in the last launch: nobody reads
// it), `S` is the skeleton; FIRST: S = d, every node written, nothing read.  Wave w stages the rows w, w + 8, .. of a tile, its 64 lanes
// along the contiguous axis.  No thread returns before the second barrier.
template <bool FIRST>
__global__ void __launch_bounds__(NCA_TILE_BLOCK) softskel_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t tiles, int32_t nb1, int32_t nb2,
                                                                  const float* __restrict__ in, float* __restrict__ next, float* __restrict__ S) {
    __shared__ float s_e[SK_S0][SK_S1][SK_S2];          // E_j at (base - 2 + l); +inf outside the grid
    __shared__ float s_f[SK_G0][SK_G1][SK_G2];          // E_{j+1} at (base - 1 + l); -inf outside the grid
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t vol_off = (bid / tiles) * voxels;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    const float* __restrict__ x = in + vol_off;

    for (int r = wave; r < SK_S0 * SK_S1; r += NCA_TILE_WAVES) {
        const int l0 = r / SK_S1, l1 = r % SK_S1;
        const int32_t g0 = tile.base0 - 2 + l0, g1 = tile.base1 - 2 + l1;
        const bool ok01 = g0 >= 0 && g0 < n0 && g1 >= 0 && g1 < n1;
        const int64_t row = ((int64_t)g0 * n1 + g1) * n2;          // used only where ok01
        for (int c = lane; c < SK_S2; c += 64) {
            const int32_t g2 = tile.base2 - 2 + c;
            float v = INFINITY;
            if (ok01 && g2 >= 0 && g2 < n2) v = x[row + g2];
            s_e[l0][l1][c] = v;
        }
    }
    __syncthreads();

    for (int r = wave; r < SK_G0 * SK_G1; r += NCA_TILE_WAVES) {
        const int l0 = r / SK_G1, l1 = r % SK_G1;
        const int32_t g0 = tile.base0 - 1 + l0, g1 = tile.base1 - 1 + l1;
        const bool ok01 = g0 >= 0 && g0 < n0 && g1 >= 0 && g1 < n1;
        for (int c = lane; c < SK_G2; c += 64) {
            const int32_t g2 = tile.base2 - 1 + c;
            float a = -INFINITY;
            if (ok01 && g2 >= 0 && g2 < n2) {          // the centre, then the six neighbours in raster order of their offsets
                a = s_e[l0 + 1][l1 + 1][c + 1];
                a = sk_min(a, s_e[l0][l1 + 1][c + 1]);
                a = sk_min(a, s_e[l0 + 1][l1][c + 1]);
                a = sk_min(a, s_e[l0 + 1][l1 + 1][c]);
                a = sk_min(a, s_e[l0 + 1][l1 + 1][c + 2]);
                a = sk_min(a, s_e[l0 + 1][l1 + 2][c + 1]);
                a = sk_min(a, s_e[l0 + 2][l1 + 1][c + 1]);
            }
            s_f[l0][l1][c] = a;
        }
    }
    __syncthreads();

    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        if (!nodes.live(k)) continue;
        const float e1 = s_f[k + 1][wave + 1][lane + 1];
        float a = e1;          // the centre, then the 26 neighbours in raster order of their offsets
#pragma unroll
        for (int d0 = 0; d0 < 3; ++d0)
#pragma unroll
            for (int d1 = 0; d1 < 3; ++d1)
#pragma unroll
                for (int d2 = 0; d2 < 3; ++d2)
                    if (d0 != 1 || d1 != 1 || d2 != 1) a = sk_max(a, s_f[k + d0][wave + d1][lane + d2]);
        const float d = sk_relu(__fsub_rn(s_e[k + 2][wave + 2][lane + 2], a));
        const int64_t off = vol_off + nodes.off(k);
        if (next) next[off] = e1;
        if (FIRST) {
            S[off] = d;
        } else {
            const float s = S[off];
            S[off] = __fadd_rn(s, sk_relu(__fsub_rn(d, __fmul_rn(s, d))));
        }
    }
}

// The checks the query and the entry point share: the 8 bytes per node of the workspace and the 4 + 4 of the volumes must fit int64.
static int skel_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    return nca_check_stack(g_err, who, grid, n_vol, "n_vol", 16, "volumes", 0, g, nodes);
}

extern "C" size_t nca_vol_softskel_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes;
    if (skel_check("nca_vol_softskel_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    return ((size_t)nodes * 8 + 255) / 256 * 256;
}

extern "C" int nca_vol_softskel(const NcaGrid* grid, const float* vol, int32_t n_vol, int32_t iterations, float* out, void* work, size_t work_bytes, void* stream) {
    const char* who = "nca_vol_softskel";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, out);
    if ((const void*)out == (const void*)vol) return g_err.fail(NCA_E_INVALID, "%s: out is vol: the skeleton is not formed in place", who);
    NcaGrid g;
    int64_t nodes;
    const int rc = skel_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    if (iterations < 0) return g_err.fail(NCA_E_INVALID, "%s: iterations = %d is negative", who, (int)iterations);
    if (iterations > NCA_SKEL_MAX_ITER)
        return g_err.fail(NCA_E_UNSUPPORTED, "%s: iterations = %d is larger than NCA_SKEL_MAX_ITER = %d", who, (int)iterations, (int)NCA_SKEL_MAX_ITER);
    int32_t nb[3];
    int64_t tiles;
    const int rct = nca_count_tiles(g_err, who, g, 0, nb, &tiles);
    if (rct != NCA_OK) return rct;
    const int64_t blocks = tiles * n_vol;          // both below 2^31
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, blocks, 0, 0, SK_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_softskel_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    float* buf[2] = {(float*)work, (float*)work + nodes};          // E_{j+1} of launch j goes to buf[j & 1]
    const int64_t voxels = nodes / n_vol;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid_dim((unsigned)blocks), block_dim(NCA_TILE_BLOCK);
    for (int32_t j = 0; j <= iterations; ++j) {
        const float* in = j == 0 ? vol : buf[(j - 1) & 1];
        float* next = j == iterations ? nullptr : buf[j & 1];
        if (j == 0)
            hipLaunchKernelGGL((softskel_kernel<true>), grid_dim, block_dim, 0, s, g.n[0], g.n[1], g.n[2], voxels, tiles, nb[1], nb[2], in, next, out);
        else
            hipLaunchKernelGGL((softskel_kernel<false>), grid_dim, block_dim, 0, s, g.n[0], g.n[1], g.n[2], voxels, tiles, nb[1], nb[2], in, next, out);
    }
    return nca_launched(g_err, who);
}

// -------------------------------------------------------------------------------------------------------------------------- overlap sums
constexpr int OV_BLOCK = 256, OV_NPT = 16, OV_CHUNK = OV_BLOCK * OV_NPT;
constexpr int64_t OV_MAX_BLOCKS = (1LL << 32) / OV_BLOCK;          // a launch carries at most 2^32 threads

// the sum over the threads of a workgroup in a binary tree: s[t] += s[t + h] for h = 128, 64, .., 1; the result is in s[0][.]
__device__ __forceinline__ void ov_tree(double (*s)[OV_BLOCK], int tid, double p, double q) {
    s[0][tid] = p;
    s[1][tid] = q;
    __syncthreads();
    for (int h = OV_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s[0][tid] = __dadd_rn(s[0][tid], s[0][tid + h]);
            s[1][tid] = __dadd_rn(s[1][tid], s[1][tid + h]);
        }
        __syncthreads();
    }
}

// Block b owns the nodes OV_CHUNK c .. OV_CHUNK c + OV_CHUNK - 1 of volume v, (v, c) = (b / chunks, b % chunks); thread t adds the nodes
// t, t + 256, .. of them in this order.  part[b] = (sum a b, sum a).
__global__ void __launch_bounds__(OV_BLOCK) overlap_part_kernel(int64_t voxels, int64_t chunks, const float* __restrict__ a, const float* __restrict__ b,
                                                                double* __restrict__ part) {
    __shared__ double s[2][OV_BLOCK];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t base = (bid / chunks) * voxels, i0 = (bid % chunks) * OV_CHUNK;
    double p = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < OV_NPT; ++k) {
        const int64_t i = i0 + k * OV_BLOCK + tid;
        if (i < voxels) {
            const double x = (double)a[base + i], y = (double)b[base + i];
            p = __dadd_rn(p, __dmul_rn(x, y));
            q = __dadd_rn(q, x);
        }
    }
    ov_tree(s, tid, p, q);
    if (tid == 0) {
        part[2 * bid] = s[0][0];
        part[2 * bid + 1] = s[1][0];
    }
}

// Block v adds the `chunks` partial sums of volume v: thread t those of the chunks t, t + 256, .. in this order, then the tree.
__global__ void __launch_bounds__(OV_BLOCK) overlap_sum_kernel(int64_t chunks, const double* __restrict__ part, double* __restrict__ sums) {
    __shared__ double s[2][OV_BLOCK];
    const int tid = threadIdx.x;
    const int64_t v = blockIdx.x;
    double p = 0.0, q = 0.0;
    for (int64_t c = tid; c < chunks; c += OV_BLOCK) {
        p = __dadd_rn(p, part[2 * (v * chunks + c)]);
        q = __dadd_rn(q, part[2 * (v * chunks + c) + 1]);
    }
    ov_tree(s, tid, p, q);
    if (tid == 0) {
        sums[2 * v] = s[0][0];
        sums[2 * v + 1] = s[1][0];
    }
}

// The checks the query and the entry point share: the 4 + 4 bytes per node of the two stacks must fit int64 (the workspace is smaller).
static int overlap_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    return nca_check_stack(g_err, who, grid, n_vol, "n_vol", 8, "volumes", 0, g, nodes);
}

extern "C" size_t nca_vol_overlap_sums_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes;
    if (overlap_check("nca_vol_overlap_sums_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    const int64_t chunks = (nodes / n_vol + OV_CHUNK - 1) / OV_CHUNK;
    return ((size_t)chunks * n_vol * 16 + 255) / 256 * 256;
}

extern "C" int nca_vol_overlap_sums(const NcaGrid* grid, const float* a, const float* b, int32_t n_vol, double* sums, void* work, size_t work_bytes, void* stream) {
    const char* who = "nca_vol_overlap_sums";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, a);
    NCA_REFUSE_NULL(g_err, who, b);
    NCA_REFUSE_NULL(g_err, who, sums);
    NcaGrid g;
    int64_t nodes;
    const int rc = overlap_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    const int64_t voxels = nodes / n_vol, chunks = (voxels + OV_CHUNK - 1) / OV_CHUNK;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, chunks * n_vol, 0, 0, OV_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_overlap_sums_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(overlap_part_kernel, dim3((unsigned)(chunks * n_vol)), dim3(OV_BLOCK), 0, s, voxels, chunks, a, b, (double*)work);
    hipLaunchKernelGGL(overlap_sum_kernel, dim3((unsigned)n_vol), dim3(OV_BLOCK), 0, s, chunks, (const double*)work, sums);
    return nca_launched(g_err, who);
}
