// nca_path.hip -- minimal paths in voxel stacks (include/nerfca_hip.h, "path"): the geodesic distance transform under a cost, its
// predecessor field, path tracing and ball cover -- what centreline.geodesic_distance, predecessors, trace_paths, ball_cover and extract run.
//
// The geodesic transform is a sequence of SWEEPS.  A sweep reads state s - 1 from one buffer and writes state s to the other (`dist` and the
// workspace, ping-pong).  A workgroup owns a tile of 4 x 8 x 64 nodes (nca_view_common.hpp): it stages the tile with a halo of one node in
// LDS (6 x 10 x 66 f64 of D and as many f32 of the cost, 47.5 KB: three workgroups, 24 waves, per CU of 160 KB -- the rounds are latency-bound
// LDS gathers, so resident waves are what hides them), relaxes the tile's nodes in rounds until a round lowers nothing, and writes the tile.
// The halo is never written: tiles exchange values only between sweeps (Jacobi across tiles), so state s is a function of state s - 1 alone.
//
// TERMINATION: no workgroup ever waits for another one.  There is no flag wait, no spin and no cooperative launch in this file; the changed
// bytes of the previous sweep are read once at the start of a workgroup and were written by an earlier launch.  The loops:
//   rounds:   in a round every thread recomputes, for each of its four nodes, min(own, min over open neighbours u of fl(D[u] + w(u, v))) from
//             LDS and stores it if it is lower; a barrier ends the round.  A thread is the only writer of its nodes and the 8-byte LDS words
//             are read and written whole, so a value read during a round is the one from the end of the previous round or a lower one of this
//             round -- both at or above the node's final value, since values only ever decrease towards the tile's fixed point, which is
//             unique given the halo.  By induction a node whose minimal path (from the halo or from the tile's own input values) has r edges
//             inside the tile is final after round r: its predecessor on that path was final after round r - 1 and is read as such.  Such a
//             path visits no node twice, so r is below the tile's node count N = 2048: after at most N rounds nothing can be lowered, and
//             round N + 1 at the latest lowers nothing and ends the loop.  The loop is capped at N + 1 rounds whatever the loads return.
//   trace:    at most max_len steps for ANY contents of pred; a word outside [0, voxels) ends the walk.
//   cover:    the nodes of a box clipped to the grid, counted up front.
//
// DETERMINISM: within a tile the updates race, but only towards the unique fixed point; across tiles a sweep reads only state s - 1.  No atomics
// on D.  The same bits on every run, with or without skipping.
//
// SKIPPING: a tile whose own changed byte and those of its 26 neighbour tiles are all 0 for sweep s - 1 is not run in sweep s.  INVARIANT:
// after every sweep the destination buffer holds the whole of state s.  A tile that is skipped in sweep s did not change in sweep s - 1, so
// its two copies (state s - 2 in this sweep's destination, state s - 1 in its source) are equal; its halo did not change either, so the fixed
// point it reached in sweep s - 1 is still its fixed point: state s equals both copies and nothing needs writing.  The first sweep of a call
// runs every tile (the workspace holds nothing yet).
//
// This translation unit keeps its own thread-local error message (nca_path_last_error): it shares no state with the other sections.
#include <atomic>

#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_path_last_error(void) { return g_err.msg; }

static std::atomic<int> g_pt_skip{1};

extern "C" int nca_path_set_skip(int32_t on) {
    if (on != 0 && on != 1) return g_err.fail(NCA_E_INVALID, "nca_path_set_skip: on = %d is neither 0 nor 1", (int)on);
    g_pt_skip.store(on);
    return NCA_OK;
}

extern "C" int nca_path_get_skip(void) { return g_pt_skip.load(); }

constexpr int64_t PT_MAX_NODES = 0x7ffffffeLL;          // a node index in int32, and -1 besides
constexpr int64_t PT_MAX_BLOCKS = 0x7fffffffLL;
constexpr int PT_TILE_NODES = NCA_TILE0 * NCA_TILE1 * NCA_TILE2;
constexpr int PT_H0 = NCA_TILE0 + 2, PT_H1 = NCA_TILE1 + 2, PT_H2 = NCA_TILE2 + 2, PT_HALO_NODES = PT_H0 * PT_H1 * PT_H2;
constexpr int PT_BLOCK = 256;
static_assert(PT_TILE_NODES == 2048 && PT_HALO_NODES == 3960, "6 x 10 x 66 nodes of 8 + 4 bytes in LDS");

// The neighbourhood of a call: the offsets d with 1 .. conn non-zero components in ascending (d0, d1, d2) order, the edge lengths len(d) in
// f64, formed on the host, and the offsets as steps of the halo'd tile in LDS and of the volume.
struct PtNbrs {
    int32_t count;
    int8_t d[26][3];
    int32_t lds_step[26];
    double len[26];
};

static PtNbrs pt_neighbours(const NcaGrid& g, int32_t conn) {
    PtNbrs nb;
    nb.count = 0;
    double h[3];
    for (int a = 0; a < 3; ++a) h[a] = 1.0 / g.inv[a];
    for (int d0 = -1; d0 <= 1; ++d0)
        for (int d1 = -1; d1 <= 1; ++d1)
            for (int d2 = -1; d2 <= 1; ++d2) {
                const int nz = (d0 != 0) + (d1 != 0) + (d2 != 0);
                if (nz == 0 || nz > conn) continue;
                const int i = nb.count++;
                nb.d[i][0] = (int8_t)d0;
                nb.d[i][1] = (int8_t)d1;
                nb.d[i][2] = (int8_t)d2;
                nb.lds_step[i] = (d0 * PT_H1 + d1) * PT_H2 + d2;
                const double a0 = d0 * h[0], a1 = d1 * h[1], a2 = d2 * h[2];
                nb.len[i] = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
            }
    for (int i = nb.count; i < 26; ++i) {
        nb.d[i][0] = nb.d[i][1] = nb.d[i][2] = 0;
        nb.lds_step[i] = 0;
        nb.len[i] = 0.0;
    }
    return nb;
}

__device__ __forceinline__ bool pt_open(float c) { return c >= 0.0f && c < INFINITY; }          // finite and >= 0: a NaN fails both

// whole 8-byte LDS words, as nca_label.hip reads and writes its 4-byte ones
__device__ __forceinline__ double pt_lds_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
__device__ __forceinline__ void pt_lds_store(double* p, double v) {
    __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ------------------------------------------------------------------------------------------------------------------------------ a sweep
// Block b owns tile b % tiles of volume b / tiles.  chg_prev (NULL in the first sweep of a call and with skipping off) and chg_next are the
// changed bytes of sweeps s - 1 and s, one per tile of the stack.
__global__ void __launch_bounds__(NCA_TILE_BLOCK) path_sweep_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t tiles, int32_t nb0, int32_t nb1,
                                                                    int32_t nb2, const float* __restrict__ cost, const double* __restrict__ src,
                                                                    double* __restrict__ dst, const uint8_t* __restrict__ chg_prev,
                                                                    uint8_t* __restrict__ chg_next, PtNbrs nbrs) {
    __shared__ double s_d[PT_HALO_NODES];
    __shared__ float s_c[PT_HALO_NODES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / tiles, t = bid % tiles;
    const int64_t vol_off = v * voxels;
    const NcaTile tile = nca_tile(t, nb1, nb2);

    if (chg_prev) {          // uniform over the workgroup
        const int32_t t2 = (int32_t)(t % nb2), t1 = (int32_t)((t / nb2) % nb1), t0 = (int32_t)(t / ((int64_t)nb2 * nb1));
        bool any = false;
        for (int e0 = -1; e0 <= 1; ++e0)
            for (int e1 = -1; e1 <= 1; ++e1)
                for (int e2 = -1; e2 <= 1; ++e2) {
                    const int32_t u0 = t0 + e0, u1 = t1 + e1, u2 = t2 + e2;
                    if (u0 < 0 || u0 >= nb0 || u1 < 0 || u1 >= nb1 || u2 < 0 || u2 >= nb2) continue;
                    any = any || chg_prev[v * tiles + ((int64_t)u0 * nb1 + u1) * nb2 + u2] != 0;
                }
        if (!any) {          // both copies of the tile hold state s already (the invariant at the top of the file)
            if (tid == 0) chg_next[bid] = 0;
            return;
        }
    }

    for (int i = tid; i < PT_HALO_NODES; i += NCA_TILE_BLOCK) {
        const int32_t j2 = i % PT_H2, j1 = (i / PT_H2) % PT_H1, j0 = i / (PT_H2 * PT_H1);
        const int32_t i0 = tile.base0 - 1 + j0, i1 = tile.base1 - 1 + j1, i2 = tile.base2 - 1 + j2;
        float c = -1.0f;          // outside the grid: a wall
        double d = INFINITY;
        if (i0 >= 0 && i0 < n0 && i1 >= 0 && i1 < n1 && i2 >= 0 && i2 < n2) {
            const int64_t off = vol_off + ((int64_t)i0 * n1 + i1) * n2 + i2;
            c = cost[off];
            if (pt_open(c))
                d = src[off];
            else
                c = -1.0f;
        }
        s_c[i] = c;
        s_d[i] = d;
    }
    __syncthreads();

    const int own0 = (PT_H1 + wave + 1) * PT_H2 + lane + 1;          // node k = 0 of this thread in the halo'd tile
    for (int round = 0; round <= PT_TILE_NODES; ++round) {          // at most N + 1 rounds (TERMINATION)
        bool lowered = false;
#pragma unroll
        for (int k = 0; k < NCA_TILE_NPT; ++k) {
            const int x = own0 + k * PT_H1 * PT_H2;
            const float cv = s_c[x];
            if (!pt_open(cv)) continue;
            const double own = pt_lds_load(s_d + x);
            double best = own;
            for (int j = 0; j < nbrs.count; ++j) {
                const int y = x + nbrs.lds_step[j];
                const float cu = s_c[y];
                if (!pt_open(cu)) continue;
                const double w = nbrs.len[j] * (0.5 * ((double)cu + (double)cv));
                const double cand = pt_lds_load(s_d + y) + w;
                if (cand < best) best = cand;
            }
            if (best < own) {
                pt_lds_store(s_d + x, best);
                lowered = true;
            }
        }
        if (!__syncthreads_or(lowered)) break;
    }

    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    bool changed = false;
#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        if (!nodes.live(k)) continue;
        const int64_t off = vol_off + nodes.off(k);
        const double now = s_d[own0 + k * PT_H1 * PT_H2], was = src[off];
        changed = changed || now != was;
        dst[off] = now;
    }
    const int any_changed = __syncthreads_or(changed);
    if (tid == 0) chg_next[bid] = any_changed ? 1 : 0;
}

__global__ void __launch_bounds__(PT_BLOCK) path_copy_kernel(int64_t n, const double* __restrict__ src, double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// Block v counts the changed bytes of volume v: integer adds, exact in any order.
__global__ void __launch_bounds__(PT_BLOCK) path_count_kernel(int64_t tiles, const uint8_t* __restrict__ chg, int32_t* __restrict__ changed) {
    __shared__ int32_t s[PT_BLOCK / 64];
    const int tid = threadIdx.x;
    const uint8_t* __restrict__ p = chg + (int64_t)blockIdx.x * tiles;
    int32_t n = 0;
    for (int64_t i = tid; i < tiles; i += PT_BLOCK) n += p[i] != 0;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((tid & 63) == 0) s[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) changed[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// ------------------------------------------------------------------------------------------------------------------------- predecessors
// One thread per node: among the open neighbours u with D[u] < D[v] the one that minimises fl(D[u] + w(u, v)), the first in offset order on a tie.
__global__ void __launch_bounds__(PT_BLOCK) path_pred_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t nodes, const float* __restrict__ cost,
                                                             const double* __restrict__ dist, int32_t* __restrict__ pred, PtNbrs nbrs) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= nodes) return;
    const int64_t x = i % voxels, vol_off = i - x;
    const int32_t i2 = (int32_t)(x % n2), i1 = (int32_t)((x / n2) % n1), i0 = (int32_t)(x / ((int64_t)n2 * n1));
    const float cv = cost[i];
    int32_t out = -1;
    if (pt_open(cv)) {
        const double dv = dist[i];
        double best = INFINITY;
        for (int j = 0; j < nbrs.count; ++j) {
            const int32_t j0 = i0 + nbrs.d[j][0], j1 = i1 + nbrs.d[j][1], j2 = i2 + nbrs.d[j][2];
            if (j0 < 0 || j0 >= n0 || j1 < 0 || j1 >= n1 || j2 < 0 || j2 >= n2) continue;
            const int64_t y = ((int64_t)j0 * n1 + j1) * n2 + j2;
            const float cu = cost[vol_off + y];
            if (!pt_open(cu)) continue;
            const double du = dist[vol_off + y];
            if (!(du < dv)) continue;
            const double cand = du + nbrs.len[j] * (0.5 * ((double)cu + (double)cv));
            if (out < 0 || cand < best) {
                best = cand;
                out = (int32_t)y;
            }
        }
    }
    pred[i] = out;
}

// -------------------------------------------------------------------------------------------------------------------------------- trace
// One thread per path.  At most max_len steps whatever pred holds.
__global__ void __launch_bounds__(PT_BLOCK) path_trace_kernel(int64_t voxels, const int32_t* __restrict__ pred, const uint8_t* __restrict__ stop, int32_t n_paths,
                                                              const int32_t* __restrict__ starts, int32_t max_len, int32_t* __restrict__ paths,
                                                              int32_t* __restrict__ lengths, int32_t* __restrict__ status) {
    const int64_t p = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (p >= n_paths) return;
    int32_t* __restrict__ row = paths + p * max_len;
    int32_t x = starts[p], len = 0, st = 3;
    if (x >= 0 && (int64_t)x < voxels) {
        st = 2;
        while (len < max_len) {
            row[len++] = x;
            if (stop && stop[x]) {
                st = 1;
                break;
            }
            const int32_t nx = pred[x];
            if (nx < 0 || (int64_t)nx >= voxels) {
                st = 0;
                break;
            }
            x = nx;
        }
    }
    for (int32_t i = len; i < max_len; ++i) row[i] = -1;
    lengths[p] = len;
    status[p] = st;
}

// --------------------------------------------------------------------------------------------------------------------------- ball cover
// Block p covers the ball of point p: the nodes of the ball's box, clipped to the grid, are tested one by one.  Every writer writes 1.
__global__ void __launch_bounds__(PT_BLOCK) path_cover_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, double h0, double h1, double h2,
                                                              const int32_t* __restrict__ nodes, const float* __restrict__ radius,
                                                              uint8_t* __restrict__ covered) {
    const int32_t node = nodes[blockIdx.x];
    if (node < 0 || (int64_t)node >= voxels) return;
    const double r = (double)radius[blockIdx.x], rr = r * r;
    if (!(rr >= 0.0)) return;          // a NaN covers nothing
    const int32_t p2 = node % n2, p1 = (node / n2) % n1, p0 = (int32_t)(node / ((int64_t)n2 * n1));
    const int32_t n[3] = {n0, n1, n2}, p[3] = {p0, p1, p2};
    const double h[3] = {h0, h1, h2};
    int32_t lo[3], ext[3];
    for (int a = 0; a < 3; ++a) {
        const double reach = fabs(r) / h[a] + 1.0;          // one node more than the ball reaches: the test below decides
        const int32_t e = reach < (double)n[a] ? (int32_t)reach : n[a];
        lo[a] = p[a] - e > 0 ? p[a] - e : 0;
        const int32_t hi = p[a] + e < n[a] - 1 ? p[a] + e : n[a] - 1;
        ext[a] = hi - lo[a] + 1;
    }
    const int64_t box = (int64_t)ext[0] * ext[1] * ext[2];
    for (int64_t i = threadIdx.x; i < box; i += PT_BLOCK) {
        const int32_t x2 = lo[2] + (int32_t)(i % ext[2]), x1 = lo[1] + (int32_t)((i / ext[2]) % ext[1]), x0 = lo[0] + (int32_t)(i / ((int64_t)ext[2] * ext[1]));
        const double a0 = (double)(x0 - p0) * h0, a1 = (double)(x1 - p1) * h1, a2 = (double)(x2 - p2) * h2;
        if ((a0 * a0 + a1 * a1) + a2 * a2 <= rr) covered[((int64_t)x0 * n1 + x1) * n2 + x2] = 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- entry points
// What the query and the entry points share: 4 + 8 bytes per node of cost and dist and 8 of the workspace must fit int64.
static int path_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    return nca_check_stack(g_err, who, grid, n_vol, "n_vol", 32, "volumes", 0, g, nodes);
}

static int path_check_nodes(const char* who, const NcaGrid& g, int64_t voxels) {
    if (voxels > PT_MAX_NODES)
        return g_err.fail(NCA_E_UNSUPPORTED, "%s: a volume of %d x %d x %d = %lld nodes has more than 2^31 - 2: a predecessor is a node index in int32", who,
                          (int)g.n[0], (int)g.n[1], (int)g.n[2], (long long)voxels);
    return NCA_OK;
}

static int path_check_conn(const char* who, int32_t conn) {
    if (conn < 1 || conn > 3) return g_err.fail(NCA_E_UNSUPPORTED, "%s: conn = %d is not 1, 2 or 3 (6, 18 or 26 neighbours)", who, (int)conn);
    return NCA_OK;
}

static size_t path_round256(size_t b) { return (b + 255) / 256 * 256; }

extern "C" size_t nca_vol_geodesic_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes, tiles;
    if (path_check("nca_vol_geodesic_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    NcaViewErr unused;          // the count is what is wanted here; the entry point refuses one that a launch cannot carry, after the workspace
    int32_t nb[3];
    nca_count_tiles(unused, "nca_vol_geodesic_workspace", g, 0, nb, &tiles);
    return path_round256((size_t)nodes * 8) + 2 * path_round256((size_t)tiles * n_vol);
}

extern "C" int nca_vol_geodesic(const NcaGrid* grid, int32_t n_vol, const float* cost, double* dist, int32_t conn, int32_t sweeps, int32_t* changed, void* work,
                                size_t work_bytes, void* stream) {
    const char* who = "nca_vol_geodesic";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, cost);
    NCA_REFUSE_NULL(g_err, who, dist);
    NCA_REFUSE_NULL(g_err, who, changed);
    NcaGrid g;
    int64_t nodes;
    const int rc = path_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    const int rcc = path_check_conn(who, conn);
    if (rcc != NCA_OK) return rcc;
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "sweeps", sweeps);
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_geodesic_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    int32_t nb[3];
    int64_t tiles;
    const int rct = nca_count_tiles(g_err, who, g, 0, nb, &tiles);
    if (rct != NCA_OK) return rct;
    const int64_t voxels = nodes / n_vol, copy_blocks = (nodes + PT_BLOCK - 1) / PT_BLOCK;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, tiles * n_vol, (sweeps & 1) ? copy_blocks : 0, 0, PT_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcn = path_check_nodes(who, g, voxels);
    if (rcn != NCA_OK) return rcn;

    double* buf[2] = {dist, (double*)work};
    uint8_t* chg[2] = {(uint8_t*)work + path_round256((size_t)nodes * 8), (uint8_t*)work + path_round256((size_t)nodes * 8) + path_round256((size_t)tiles * n_vol)};
    const PtNbrs nbrs = pt_neighbours(g, conn);
    const bool skip = g_pt_skip.load() != 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 tile_grid((unsigned)(tiles * n_vol)), tile_block(NCA_TILE_BLOCK);
    for (int32_t i = 0; i < sweeps; ++i) {          // sweep i reads buf[i & 1] and the changed bytes chg[(i + 1) & 1] of sweep i - 1
        const uint8_t* prev = (skip && i > 0) ? chg[(i + 1) & 1] : nullptr;
        hipLaunchKernelGGL(path_sweep_kernel, tile_grid, tile_block, 0, s, g.n[0], g.n[1], g.n[2], voxels, tiles, nb[0], nb[1], nb[2], cost, (const double*)buf[i & 1],
                           buf[(i + 1) & 1], prev, chg[i & 1], nbrs);
    }
    if (sweeps & 1)          // the last state is in the workspace, whole (the invariant)
        hipLaunchKernelGGL(path_copy_kernel, dim3((unsigned)copy_blocks), dim3(PT_BLOCK), 0, s, nodes, (const double*)buf[1], buf[0]);
    hipLaunchKernelGGL(path_count_kernel, dim3((unsigned)n_vol), dim3(PT_BLOCK), 0, s, tiles, (const uint8_t*)chg[(sweeps - 1) & 1], changed);
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_geodesic_pred(const NcaGrid* grid, int32_t n_vol, const float* cost, const double* dist, int32_t conn, int32_t* pred, void* stream) {
    const char* who = "nca_vol_geodesic_pred";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, cost);
    NCA_REFUSE_NULL(g_err, who, dist);
    NCA_REFUSE_NULL(g_err, who, pred);
    NcaGrid g;
    int64_t nodes;
    const int rc = path_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    const int rcc = path_check_conn(who, conn);
    if (rcc != NCA_OK) return rcc;
    const int64_t voxels = nodes / n_vol, blocks = (nodes + PT_BLOCK - 1) / PT_BLOCK;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, blocks, 0, 0, PT_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcn = path_check_nodes(who, g, voxels);
    if (rcn != NCA_OK) return rcn;
    hipLaunchKernelGGL(path_pred_kernel, dim3((unsigned)blocks), dim3(PT_BLOCK), 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], voxels, nodes, cost, dist, pred,
                       pt_neighbours(g, conn));
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_trace_paths(int64_t voxels, const int32_t* pred, const uint8_t* stop, int32_t n_paths, const int32_t* starts, int32_t max_len, int32_t* paths,
                                   int32_t* lengths, int32_t* status, void* stream) {
    const char* who = "nca_vol_trace_paths";
    NCA_REFUSE_NULL(g_err, who, pred);
    NCA_REFUSE_NULL(g_err, who, starts);
    NCA_REFUSE_NULL(g_err, who, paths);
    NCA_REFUSE_NULL(g_err, who, lengths);
    NCA_REFUSE_NULL(g_err, who, status);
    if (voxels <= 0) return g_err.fail(NCA_E_INVALID, "%s: voxels = %lld is not positive", who, (long long)voxels);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_paths", n_paths);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "max_len", max_len);
    if (voxels > PT_MAX_NODES)
        return g_err.fail(NCA_E_UNSUPPORTED, "%s: a volume of %lld nodes has more than 2^31 - 2: a predecessor is a node index in int32", who, (long long)voxels);
    const int64_t blocks = ((int64_t)n_paths + PT_BLOCK - 1) / PT_BLOCK;
    hipLaunchKernelGGL(path_trace_kernel, dim3((unsigned)blocks), dim3(PT_BLOCK), 0, (hipStream_t)stream, voxels, pred, stop, n_paths, starts, max_len, paths, lengths,
                       status);
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_ball_cover(const NcaGrid* grid, int32_t n_points, const int32_t* nodes, const float* radius, uint8_t* covered, void* stream) {
    const char* who = "nca_vol_ball_cover";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, nodes);
    NCA_REFUSE_NULL(g_err, who, radius);
    NCA_REFUSE_NULL(g_err, who, covered);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_points", n_points);
    NcaGrid g;
    int64_t voxels;
    const int rc = nca_check_grid(g_err, who, grid, 1, 32, "volumes", &g, &voxels);
    if (rc != NCA_OK) return rc;
    const int rcn = path_check_nodes(who, g, voxels);
    if (rcn != NCA_OK) return rcn;
    hipLaunchKernelGGL(path_cover_kernel, dim3((unsigned)n_points), dim3(PT_BLOCK), 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], voxels, 1.0 / g.inv[0],
                       1.0 / g.inv[1], 1.0 / g.inv[2], nodes, radius, covered);
    return nca_launched(g_err, who);
}
