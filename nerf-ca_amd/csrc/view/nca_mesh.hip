// nca_mesh.hip -- iso-surfaces of voxel stacks as indexed triangle meshes (include/nerfca_hip.h, "mesh"): mesh.isosurface and
// export.density_surfaces.
//
// Marching tetrahedra on the Kuhn split of every grid cell.  The output size depends on the data, so the work is two entry points with a
// host read of the totals between them:
//   nca_vol_iso_count   1 count   a workgroup per tile of 4 x 8 x 64 nodes (nca_view_common.hpp) stages the tile and the next node on every
//                                 axis (5 x 9 x 65 f32) in LDS; every node writes one 16-bit word: the mask of its crossed edges (7 bits)
//                                 and the triangle count of the cell it is the base of (0 .. 12).
//                       2 reduce  a workgroup per MS_CHUNK = 1024 consecutive nodes of a volume sums the vertex and triangle counts.
//                       3 scan    one workgroup per volume turns those sums into exclusive offsets, MS_SCAN_BATCH = 256 pairs at a time (a pair
//                                 as one 64-bit word) with a running carry, and writes the volume's totals.
//                       4 bases   one workgroup turns the totals into every volume's first vertex and first triangle in the stack.
//                       5 add     the workgroups of launch 2 scan their own 1024 counts, add their offset and write every node's first vertex
//                                 and first triangle within its volume.
//   nca_vol_iso_emit    6 emit    the tiles of launch 1 again, with the words and the vertex offsets of the tile and its halo staged too: every
//                                 node writes the vertices of the edges it owns and the triangles of the cell it is the base of.  A tile whose
//                                 own words are all 0 ends after reading them.
// Every vertex and every triangle is written once, by the thread that owns it, at an offset that is a sum of integers: no atomics, no flags,
// no workgroup waits for another one, and the same bits on every run.  The scans are wave scans with __shfl_up (wave64) joined through LDS.
//
// BOUNDS: every load of vol and of the workspace is at an index formed from node indices clamped into the grid; every store into the
// workspace is at a node or chunk of the checked stack; every store into verts, normals and tris is guarded by the capacities as unsigned
// comparisons, so offsets from a workspace that nca_vol_iso_count did not fill (negative ones included) write nothing.
//
// Every f64 operation is spelled as the header spells it and the build has -ffp-contract=off: a transcription has the same bits.
//
// This translation unit keeps its own thread-local error message (nca_mesh_last_error): it shares no state with the other sections.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_mesh_last_error(void) { return g_err.msg; }

constexpr int MS_S0 = NCA_TILE0 + 1, MS_S1 = NCA_TILE1 + 1, MS_S2 = NCA_TILE2 + 1;          // the tile and the next node on every axis
constexpr int MS_BLOCK = 256, MS_NPT = 4, MS_CHUNK = MS_BLOCK * MS_NPT;                      // launches 2 and 5: 1024 consecutive nodes per workgroup
constexpr int MS_SCAN_BATCH = MS_BLOCK;                                                      // launches 3 and 4: sums per round
constexpr int64_t MS_MAX_BLOCKS = 0x7fffffffLL;
constexpr int64_t MS_MAX_OFFSET = 0x7fffffffLL;          // offsets are int32
static_assert((size_t)(MS_S0 * MS_S1 * MS_S2) * (sizeof(float) + sizeof(int32_t) + sizeof(uint16_t)) <= 65536, "the staged tile fits the LDS of one workgroup");
static_assert(MS_NPT == 4, "a thread of launches 2 and 5 owns four consecutive nodes: one 8-byte load, two 16-byte stores");

// The corners p1 and p2 of tetrahedron q as codes 4 d0 + 2 d1 + d2 of their offset from the base node (p0 = 0, p3 = 7), and its parity
__constant__ const uint8_t MS_P1[6] = {4, 4, 2, 2, 1, 1};
__constant__ const uint8_t MS_P2[6] = {6, 5, 6, 3, 5, 3};
__constant__ const uint8_t MS_ODD[6] = {0, 1, 1, 0, 0, 1};
// The edges 0 .. 5 of a tetrahedron as corner pairs (i, j), i < j
__constant__ const uint8_t MS_EI[6] = {0, 0, 0, 1, 1, 2};
__constant__ const uint8_t MS_EJ[6] = {1, 2, 3, 2, 3, 3};
// case (bit i: corner i is inside) -> the edges of its triangles, for even parity: the header's table
__constant__ const uint8_t MS_TRI[16][6] = {{0, 0, 0, 0, 0, 0}, {0, 1, 2, 0, 0, 0}, {0, 4, 3, 0, 0, 0}, {1, 2, 4, 1, 4, 3}, {1, 3, 5, 0, 0, 0}, {0, 3, 5, 0, 5, 2},
                                            {0, 4, 5, 0, 5, 1}, {2, 4, 5, 0, 0, 0}, {2, 5, 4, 0, 0, 0}, {0, 1, 5, 0, 5, 4}, {0, 2, 5, 0, 5, 3}, {1, 5, 3, 0, 0, 0},
                                            {1, 3, 4, 1, 4, 2}, {0, 3, 4, 0, 0, 0}, {0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};

// a row of verts, normals or tris: one 12-byte store
template <typename T>
struct MsRow {
    T a, b, c;
};

struct MsGeom {
    double lo[3], h[3], inv[3];          // h = 1 / inv, formed once on the host
};

// triangles of a tetrahedron with the corners of `m` inside: 0, 1, 2, 1, 0 for 0 .. 4 corners
__device__ __forceinline__ int ms_case_tris(uint32_t m) {
    const int pc = __popc(m);
    return pc == 2 ? 2 : (pc & 1);
}

__device__ __forceinline__ uint32_t ms_case(uint32_t inb, int q) {
    return (inb & 1u) | (((inb >> MS_P1[q]) & 1u) << 1) | (((inb >> MS_P2[q]) & 1u) << 2) | (((inb >> 7) & 1u) << 3);
}

// Wave w stages the rows w, w + 8, .. of the tile and its halo, its 64 lanes along the contiguous axis (lane 0 takes the 65th node too).  A
// staged node outside the grid holds the value of the nearest node inside: no load out of bounds; such a node is never looked at.
template <typename T>
__device__ __forceinline__ void ms_stage(T (*s)[MS_S1][MS_S2], const T* __restrict__ x, NcaTile tile, int32_t n0, int32_t n1, int32_t n2, int wave, int lane) {
    for (int r = wave; r < MS_S0 * MS_S1; r += NCA_TILE_WAVES) {
        const int l0 = r / MS_S1, l1 = r % MS_S1;
        const int32_t g0 = min(tile.base0 + l0, n0 - 1), g1 = min(tile.base1 + l1, n1 - 1);
        const int64_t row = ((int64_t)g0 * n1 + g1) * n2;
        for (int cc = lane; cc < MS_S2; cc += 64) s[l0][l1][cc] = x[row + min(tile.base2 + cc, n2 - 1)];
    }
}

// bit c = 4 d0 + 2 d1 + d2 of `exist`: node + d is inside the grid; of `inb`: it is, and its value is above the level
struct MsBits {
    uint32_t inb, exist;
};

__device__ __forceinline__ MsBits ms_bits(const float (*s_v)[MS_S1][MS_S2], int j0, int j1, int j2, int32_t i0, int32_t i1, int32_t i2, int32_t n0, int32_t n1, int32_t n2,
                                          float level) {
    uint32_t inb = 0, exist = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int d0 = (c >> 2) & 1, d1 = (c >> 1) & 1, d2 = c & 1;
        const bool ok = i0 + d0 < n0 && i1 + d1 < n1 && i2 + d2 < n2;
        exist |= (uint32_t)ok << c;
        inb |= (uint32_t)(ok && s_v[j0 + d0][j1 + d1][j2 + d2] > level) << c;
    }
    return {inb, exist};
}

// ---------------------------------------------------------------------------------------------------------------------------- 1: count
// Block b owns tile b % tiles of volume b / tiles.  word = the crossing mask (bit k - 1: edge k) | the cell's triangle count << 8.
__global__ void __launch_bounds__(NCA_TILE_BLOCK) iso_count_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t vstride, int64_t tiles, int32_t nb1, int32_t nb2,
                                                                   const float* __restrict__ vol, float level, uint16_t* __restrict__ cnt) {
    __shared__ float s_v[MS_S0][MS_S1][MS_S2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / tiles;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    ms_stage<float>(s_v, vol + v * voxels, tile, n0, n1, n2, wave, lane);
    __syncthreads();
    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        if (!nodes.live(k)) continue;
        const MsBits b = ms_bits(s_v, k, wave, lane, tile.base0 + k, nodes.i1, nodes.i2, n0, n1, n2, level);
        const uint32_t mask = ((((b.inb & 1u) ? ~b.inb : b.inb) & b.exist) >> 1) & 0x7fu;
        uint32_t nt = 0;
        if (b.exist == 0xffu) {
#pragma unroll
            for (int q = 0; q < 6; ++q) nt += ms_case_tris(ms_case(b.inb, q));
        }
        cnt[v * vstride + nodes.off(k)] = (uint16_t)(mask | (nt << 8));
    }
}

// --------------------------------------------------------------------------------------------------------------- 2 .. 5: the scan
// The exclusive prefix of `x` over the 256 threads of a workgroup in thread order, and the sum over all of them in *total: an inclusive
// scan per wave with __shfl_up, the four wave sums through s (4 words).  Ends with a barrier: s may be used again at once.
template <typename T>
__device__ __forceinline__ T ms_block_scan(T* s, int tid, T x, T* total) {
    const int lane = tid & 63, wave = tid >> 6;
    T inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T below = __shfl_up(inc, o);
        if (lane >= o) inc += below;
    }
    if (lane == 63) s[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MS_BLOCK / 64; ++w) {
        if (w < wave) before += s[w];
        all += s[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - x;
}

// the four words of the thread's nodes c .. c + 3 (c a multiple of 4, so all four lie below vstride or none does): the vertex and triangle
// counts of those below `voxels`, the rest 0
__device__ __forceinline__ void ms_load4(const uint16_t* __restrict__ cnt, int64_t c, int64_t voxels, int64_t vstride, int32_t nv[4], int32_t nt[4]) {
    uint2 w = {0u, 0u};
    if (c < vstride) w = *reinterpret_cast<const uint2*>(cnt + c);
    const uint32_t word[4] = {w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = c + j < voxels;
        nv[j] = ok ? __popc(word[j] & 0x7fu) : 0;
        nt[j] = ok ? (int32_t)((word[j] >> 8) & 15u) : 0;
    }
}

// Block b owns the nodes 1024 c .. 1024 c + 1023 of volume v, (v, c) = (b / chunks, b % chunks); thread t the nodes 4 t .. 4 t + 3 of them.
__global__ void __launch_bounds__(MS_BLOCK) iso_reduce_kernel(int64_t voxels, int64_t vstride, int64_t chunks, const uint16_t* __restrict__ cnt, int32_t* __restrict__ part) {
    __shared__ int32_t s[MS_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / chunks, c = (bid % chunks) * MS_CHUNK + (int64_t)tid * MS_NPT;
    int32_t nv[4], nt[4], sv, st;
    ms_load4(cnt + v * vstride, c, voxels, vstride, nv, nt);
    ms_block_scan<int32_t>(s, tid, (nv[0] + nv[1]) + (nv[2] + nv[3]), &sv);
    ms_block_scan<int32_t>(s, tid, (nt[0] + nt[1]) + (nt[2] + nt[3]), &st);
    if (tid == 0) {
        part[2 * bid] = sv;
        part[2 * bid + 1] = st;
    }
}

// Block v turns the `chunks` pairs of sums of volume v into exclusive offsets, in place, 256 at a time with a running carry; totals[v] = the
// carry after the last round, written twice.  A pair is scanned as one 64-bit word, the vertices above the triangles: the refusals keep every
// sum below 2^31, so the low half never carries into the high one.  The next round's pairs are loaded before this round's scan.
__global__ void __launch_bounds__(MS_BLOCK) iso_scan_kernel(int64_t chunks, int32_t* __restrict__ part, int64_t* __restrict__ kept, int64_t* __restrict__ totals) {
    __shared__ long long s[MS_BLOCK / 64];
    const int tid = threadIdx.x;
    int2* p = reinterpret_cast<int2*>(part) + (int64_t)blockIdx.x * chunks;
    long long carry = 0;
    int2 x = tid < chunks ? p[tid] : make_int2(0, 0);
    for (int64_t c0 = 0; c0 < chunks; c0 += MS_SCAN_BATCH) {
        const int64_t c = c0 + tid;
        const int2 next = c + MS_SCAN_BATCH < chunks ? p[c + MS_SCAN_BATCH] : make_int2(0, 0);          // not written in this round
        long long sum;
        const long long e = carry + ms_block_scan<long long>(s, tid, ((long long)x.x << 32) | (long long)(uint32_t)x.y, &sum);
        if (c < chunks) p[c] = make_int2((int32_t)(e >> 32), (int32_t)(e & 0xffffffffLL));
        carry += sum;
        x = next;
    }
    if (tid == 0) {          // once for launch 4, in the workspace, and once for the caller
        kept[2 * blockIdx.x] = totals[2 * blockIdx.x] = carry >> 32;
        kept[2 * blockIdx.x + 1] = totals[2 * blockIdx.x + 1] = carry & 0xffffffffLL;
    }
}

// One block: bases[v] = the sum of totals[0 .. v - 1], pair by pair in int64.
__global__ void __launch_bounds__(MS_BLOCK) iso_bases_kernel(int32_t n_vol, const int64_t* __restrict__ totals, int64_t* __restrict__ bases) {
    __shared__ long long s[MS_BLOCK / 64];
    const int tid = threadIdx.x;
    long long cv = 0, ct = 0;
    for (int64_t v0 = 0; v0 < n_vol; v0 += MS_SCAN_BATCH) {
        const int64_t v = v0 + tid;
        const bool ok = v < n_vol;
        const long long xv = ok ? (long long)totals[2 * v] : 0, xt = ok ? (long long)totals[2 * v + 1] : 0;
        long long sv, st;
        const long long ev = ms_block_scan<long long>(s, tid, xv, &sv), et = ms_block_scan<long long>(s, tid, xt, &st);
        if (ok) {
            bases[2 * v] = cv + ev;
            bases[2 * v + 1] = ct + et;
        }
        cv += sv;
        ct += st;
    }
}

// The blocks of launch 2: voff[i] = part + the vertices of the block's nodes before i, toff[i] likewise, for every node below vstride.
__global__ void __launch_bounds__(MS_BLOCK) iso_add_kernel(int64_t voxels, int64_t vstride, int64_t chunks, const uint16_t* __restrict__ cnt, const int32_t* __restrict__ part,
                                                           int32_t* __restrict__ voff, int32_t* __restrict__ toff) {
    __shared__ int32_t s[MS_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / chunks, c = (bid % chunks) * MS_CHUNK + (int64_t)tid * MS_NPT;
    int32_t nv[4], nt[4], unused;
    ms_load4(cnt + v * vstride, c, voxels, vstride, nv, nt);
    const int32_t ev = part[2 * bid] + ms_block_scan<int32_t>(s, tid, (nv[0] + nv[1]) + (nv[2] + nv[3]), &unused);
    const int32_t et = part[2 * bid + 1] + ms_block_scan<int32_t>(s, tid, (nt[0] + nt[1]) + (nt[2] + nt[3]), &unused);
    if (c < vstride) {
        *reinterpret_cast<int4*>(voff + v * vstride + c) = make_int4(ev, ev + nv[0], ev + nv[0] + nv[1], ev + nv[0] + nv[1] + nv[2]);
        *reinterpret_cast<int4*>(toff + v * vstride + c) = make_int4(et, et + nt[0], et + nt[0] + nt[1], et + nt[0] + nt[1] + nt[2]);
    }
}

// ----------------------------------------------------------------------------------------------------------------------------- 6: emit
// the central difference of `x` at node (i0, i1, i2) along axis a in nodes, indices clamped into the grid, times inv[a]
__device__ __forceinline__ void ms_gradient(const float* __restrict__ x, int32_t i0, int32_t i1, int32_t i2, int32_t n0, int32_t n1, int32_t n2, const MsGeom& geo, double g[3]) {
    const int64_t s1 = n2, s0 = (int64_t)n1 * n2;
    const int64_t at = ((int64_t)i0 * n1 + i1) * n2 + i2;
    const double p0 = (double)x[at + (i0 + 1 < n0 ? s0 : 0)], m0 = (double)x[at - (i0 > 0 ? s0 : 0)];
    const double p1 = (double)x[at + (i1 + 1 < n1 ? s1 : 0)], m1 = (double)x[at - (i1 > 0 ? s1 : 0)];
    const double p2 = (double)x[at + (i2 + 1 < n2 ? 1 : 0)], m2 = (double)x[at - (i2 > 0 ? 1 : 0)];
    g[0] = (0.5 * (p0 - m0)) * geo.inv[0];
    g[1] = (0.5 * (p1 - m1)) * geo.inv[1];
    g[2] = (0.5 * (p2 - m2)) * geo.inv[2];
}

// Block b owns tile b % tiles of volume b / tiles.  s_w and s_o are the words and the vertex offsets of the tile and its halo, as launches 1
// and 5 left them.  A node's vertices go to verts[vb + voff + r], r = the rank of the edge among the node's crossed edges; the triangles of
// its cell to tris[tb + toff + r], r counting through the tetrahedra in order.
template <bool NORMALS>
__global__ void __launch_bounds__(NCA_TILE_BLOCK) iso_emit_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t vstride, int64_t tiles, int32_t nb1, int32_t nb2,
                                                                  const float* __restrict__ vol, float level, MsGeom geo, const uint16_t* __restrict__ cnt,
                                                                  const int32_t* __restrict__ voff, const int32_t* __restrict__ toff, const int64_t* __restrict__ bases,
                                                                  int64_t vert_cap, int64_t tri_cap, float* __restrict__ verts, int32_t* __restrict__ tris,
                                                                  float* __restrict__ normals) {
    __shared__ float s_v[MS_S0][MS_S1][MS_S2];
    __shared__ int32_t s_o[MS_S0][MS_S1][MS_S2];
    __shared__ uint16_t s_w[MS_S0][MS_S1][MS_S2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / tiles;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    const float* __restrict__ x = vol + v * voxels;
    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    // a tile none of whose own nodes has a crossed edge or a triangle writes nothing: it costs its 2 bytes per node and ends here, all of it
    int any = 0;
#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k)
        if (nodes.live(k)) any |= cnt[v * vstride + nodes.off(k)];
    if (!__syncthreads_or(any)) return;
    ms_stage<float>(s_v, x, tile, n0, n1, n2, wave, lane);
    ms_stage<int32_t>(s_o, voff + v * vstride, tile, n0, n1, n2, wave, lane);
    ms_stage<uint16_t>(s_w, cnt + v * vstride, tile, n0, n1, n2, wave, lane);
    __syncthreads();
    const int64_t vb = bases[2 * v], tb = bases[2 * v + 1];
#pragma unroll 1
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        if (!nodes.live(k)) continue;
        const int32_t i0 = tile.base0 + k, i1 = nodes.i1, i2 = nodes.i2;
        const MsBits b = ms_bits(s_v, k, wave, lane, i0, i1, i2, n0, n1, n2, level);
        const uint32_t mask = ((((b.inb & 1u) ? ~b.inb : b.inb) & b.exist) >> 1) & 0x7fu;
        // the vertices of the edges this node owns
        if (mask) {
            const double va = (double)s_v[k][wave][lane], lv = (double)level;
            double ga[3];
            if constexpr (NORMALS) ms_gradient(x, i0, i1, i2, n0, n1, n2, geo, ga);
            int64_t at = vb + (int64_t)s_o[k][wave][lane];
#pragma unroll 1
            for (int e = 1; e < 8; ++e) {
                if (!((mask >> (e - 1)) & 1u)) continue;
                const int d0 = (e >> 2) & 1, d1 = (e >> 1) & 1, d2 = e & 1;
                const double t0 = (lv - va) / ((double)s_v[k + d0][wave + d1][lane + d2] - va);
                const double t = isfinite(t0) ? fmin(fmax(t0, 0.0), 1.0) : 0.5;
                if ((uint64_t)at < (uint64_t)vert_cap) {
                    const double q0 = (double)i0 + (d0 ? t : 0.0), q1 = (double)i1 + (d1 ? t : 0.0), q2 = (double)i2 + (d2 ? t : 0.0);
                    *reinterpret_cast<MsRow<float>*>(verts + 3 * at) = {(float)(geo.lo[0] + q0 * geo.h[0]), (float)(geo.lo[1] + q1 * geo.h[1]), (float)(geo.lo[2] + q2 * geo.h[2])};
                    if constexpr (NORMALS) {
                        double gb[3];
                        ms_gradient(x, i0 + d0, i1 + d1, i2 + d2, n0, n1, n2, geo, gb);
                        const double m0 = -(ga[0] + t * (gb[0] - ga[0])), m1 = -(ga[1] + t * (gb[1] - ga[1])), m2 = -(ga[2] + t * (gb[2] - ga[2]));
                        const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
                        const bool ok = isfinite(len) && len != 0.0;
                        *reinterpret_cast<MsRow<float>*>(normals + 3 * at) = {ok ? (float)(m0 / len) : 0.0f, ok ? (float)(m1 / len) : 0.0f, ok ? (float)(m2 / len) : 0.0f};
                    }
                }
                ++at;
            }
        }
        // the triangles of the cell this node is the base of
        if (b.exist != 0xffu || b.inb == 0u || b.inb == 0xffu) continue;
        int64_t at = tb + (int64_t)toff[v * vstride + nodes.off(k)];
#pragma unroll 1
        for (int q = 0; q < 6; ++q) {
            const uint32_t m = ms_case(b.inb, q);
            const int nt = ms_case_tris(m);
            const uint32_t code[4] = {0u, MS_P1[q], MS_P2[q], 7u};
            for (int s = 0; s < nt; ++s, ++at) {
                if ((uint64_t)at >= (uint64_t)tri_cap) continue;
                int32_t idx[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int e = MS_TRI[m][3 * s + r];
                    const uint32_t own = code[MS_EI[e]], kk = own ^ code[MS_EJ[e]];
                    const int j0 = k + (int)((own >> 2) & 1u), j1 = wave + (int)((own >> 1) & 1u), j2 = lane + (int)(own & 1u);
                    idx[r] = s_o[j0][j1][j2] + __popc((uint32_t)s_w[j0][j1][j2] & ((1u << (kk - 1)) - 1u));
                }
                const bool odd = MS_ODD[q] != 0;
                *reinterpret_cast<MsRow<int32_t>*>(tris + 3 * at) = {idx[0], odd ? idx[2] : idx[1], odd ? idx[1] : idx[2]};
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ the host side
static size_t ms_round256(size_t b) { return (b + 255) / 256 * 256; }

struct MsLayout {
    int64_t voxels, vstride, chunks;
    size_t cnt, voff, toff, part, totals, bases, bytes;          // offsets of the regions, and the size of all of them
};

// The checks the query and both entry points share: the stack, then that 7 vertices per node and 12 triangles per cell fit the int32 offsets.
static int mesh_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, MsLayout* y) {
    int64_t nodes;
    const int rc = nca_check_stack(g_err, who, grid, n_vol, "n_vol", 32, "volumes", 0, g, &nodes);          // 4 bytes of vol and 10 of the workspace per node, with room
    if (rc != NCA_OK) return rc;
    const int64_t voxels = nodes / n_vol, cells = (int64_t)(g->n[0] - 1) * (g->n[1] - 1) * (g->n[2] - 1);
    if (voxels > MS_MAX_OFFSET / 7 || cells > MS_MAX_OFFSET / 12)
        return g_err.fail(NCA_E_UNSUPPORTED, "%s: a volume of %d x %d x %d nodes may have more than 2^31 - 1 vertices (7 per node) or triangles (12 per cell): offsets are int32",
                          who, (int)g->n[0], (int)g->n[1], (int)g->n[2]);
    y->voxels = voxels;
    y->vstride = (voxels + 3) / 4 * 4;
    y->chunks = (voxels + MS_CHUNK - 1) / MS_CHUNK;
    const size_t per = (size_t)n_vol * (size_t)y->vstride;
    y->cnt = 0;
    y->voff = y->cnt + ms_round256(per * 2);
    y->toff = y->voff + ms_round256(per * 4);
    y->part = y->toff + ms_round256(per * 4);
    y->totals = y->part + ms_round256((size_t)n_vol * (size_t)y->chunks * 8);
    y->bases = y->totals + ms_round256((size_t)n_vol * 16);
    y->bytes = y->bases + ms_round256((size_t)n_vol * 16);
    return NCA_OK;
}

extern "C" size_t nca_vol_iso_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    MsLayout y;
    if (mesh_check("nca_vol_iso_workspace", grid, n_vol, &g, &y) != NCA_OK) return 0;
    return y.bytes;
}

// after the pointers: the stack, the level, the workspace, the launch limits
static int mesh_prepare(const char* who, const NcaGrid* grid, int32_t n_vol, float level, const void* work, size_t work_bytes, NcaGrid* g, MsLayout* y, int32_t nb[3],
                        int64_t* tiles) {
    int rc = mesh_check(who, grid, n_vol, g, y);
    if (rc != NCA_OK) return rc;
    if (!isfinite(level)) return g_err.fail(NCA_E_INVALID, "%s: level = %g is not finite", who, (double)level);
    rc = nca_check_workspace(g_err, who, work, work_bytes, y->bytes);
    if (rc != NCA_OK) return rc;
    rc = nca_count_tiles(g_err, who, *g, 0, nb, tiles);
    if (rc != NCA_OK) return rc;
    return nca_check_launch_blocks(g_err, who, n_vol, *g, *tiles * n_vol, y->chunks * n_vol, 0, MS_MAX_BLOCKS);          // each factor below 2^31
}

extern "C" int nca_vol_iso_count(const NcaGrid* grid, const float* vol, int32_t n_vol, float level, int64_t* totals, void* work, size_t work_bytes, void* stream) {
    const char* who = "nca_vol_iso_count";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, totals);
    NcaGrid g;
    MsLayout y;
    int32_t nb[3];
    int64_t tiles;
    const int rc = mesh_prepare(who, grid, n_vol, level, work, work_bytes, &g, &y, nb, &tiles);
    if (rc != NCA_OK) return rc;
    char* w = (char*)work;
    uint16_t* cnt = (uint16_t*)(w + y.cnt);
    int32_t *voff = (int32_t*)(w + y.voff), *toff = (int32_t*)(w + y.toff), *part = (int32_t*)(w + y.part);
    int64_t *tot = (int64_t*)(w + y.totals), *bases = (int64_t*)(w + y.bases);
    hipStream_t s = (hipStream_t)stream;
    const dim3 tile_grid((unsigned)(tiles * n_vol)), tile_block(NCA_TILE_BLOCK), lin_grid((unsigned)(y.chunks * n_vol)), lin_block(MS_BLOCK);
    hipLaunchKernelGGL(iso_count_kernel, tile_grid, tile_block, 0, s, g.n[0], g.n[1], g.n[2], y.voxels, y.vstride, tiles, nb[1], nb[2], vol, level, cnt);
    hipLaunchKernelGGL(iso_reduce_kernel, lin_grid, lin_block, 0, s, y.voxels, y.vstride, y.chunks, (const uint16_t*)cnt, part);
    hipLaunchKernelGGL(iso_scan_kernel, dim3((unsigned)n_vol), lin_block, 0, s, y.chunks, part, tot, totals);
    hipLaunchKernelGGL(iso_bases_kernel, dim3(1), lin_block, 0, s, n_vol, (const int64_t*)tot, bases);
    hipLaunchKernelGGL(iso_add_kernel, lin_grid, lin_block, 0, s, y.voxels, y.vstride, y.chunks, (const uint16_t*)cnt, (const int32_t*)part, voff, toff);
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_iso_emit(const NcaGrid* grid, const float* vol, int32_t n_vol, float level, const void* work, size_t work_bytes, int64_t vert_cap, int64_t tri_cap,
                                float* verts, int32_t* tris, float* normals, void* stream) {
    const char* who = "nca_vol_iso_emit";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    if (vert_cap < 0) return g_err.fail(NCA_E_INVALID, "%s: vert_cap = %lld is negative", who, (long long)vert_cap);
    if (tri_cap < 0) return g_err.fail(NCA_E_INVALID, "%s: tri_cap = %lld is negative", who, (long long)tri_cap);
    if (vert_cap > 0) NCA_REFUSE_NULL(g_err, who, verts);
    if (tri_cap > 0) NCA_REFUSE_NULL(g_err, who, tris);
    NcaGrid g;
    MsLayout y;
    int32_t nb[3];
    int64_t tiles;
    const int rc = mesh_prepare(who, grid, n_vol, level, work, work_bytes, &g, &y, nb, &tiles);
    if (rc != NCA_OK) return rc;
    if (vert_cap == 0 && tri_cap == 0) return NCA_OK;          // nothing to write: nothing is launched
    MsGeom geo;
    for (int a = 0; a < 3; ++a) {
        geo.lo[a] = g.lo[a];
        geo.inv[a] = g.inv[a];
        geo.h[a] = 1.0 / g.inv[a];
    }
    const char* w = (const char*)work;
    const uint16_t* cnt = (const uint16_t*)(w + y.cnt);
    const int32_t *voff = (const int32_t*)(w + y.voff), *toff = (const int32_t*)(w + y.toff);
    const int64_t* bases = (const int64_t*)(w + y.bases);
    const dim3 tile_grid((unsigned)(tiles * n_vol)), tile_block(NCA_TILE_BLOCK);
    if (normals && vert_cap > 0)
        hipLaunchKernelGGL((iso_emit_kernel<true>), tile_grid, tile_block, 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], y.voxels, y.vstride, tiles, nb[1], nb[2], vol, level, geo,
                           cnt, voff, toff, bases, vert_cap, tri_cap, verts, tris, normals);
    else
        hipLaunchKernelGGL((iso_emit_kernel<false>), tile_grid, tile_block, 0, (hipStream_t)stream, g.n[0], g.n[1], g.n[2], y.voxels, y.vstride, tiles, nb[1], nb[2], vol, level, geo,
                           cnt, voff, toff, bases, vert_cap, tri_cap, verts, tris, (float*)nullptr);
    return nca_launched(g_err, who);
}
