// tsdf.hip — fusing depth maps into a truncated signed distance volume and pulling a triangle mesh out of it (an extension, no
// reference counterpart; include/splat.h, "TSDF fusion and mesh extraction", states the contract).
//
// Integration, k_tsdf_integrate: one projection and one depth lookup per node per view.  A workgroup of 256 threads owns a brick
// of 32 x 4 x 4 nodes, lanes along i: every load and store of the planes is a full 128-byte line per 32 lanes.  Before it touches
// memory each wave projects the brick's eight corner nodes in float64 (brick_unseen) and leaves when all eight are behind the
// eye or, with all eight safely in front of it, beyond one side of the screen by more than a pixel: x / w < c is linear in the
// node where w > 0, so what holds at the corners of a box holds inside it.  The margins (a pixel; 2^-20 of the magnitude of w)
// are wider than the binary32 error of the per-node arithmetic wherever the test is applied, so a brick that returns holds no
// node the per-node rule would have written: the cull changes the time, never the bytes.  Every per-node quantity is formed from
// (i, j, k) alone, in fmaf chains written out below, so the result does not depend on the brick shape either.  The depth lookup
// is a gather from the map as it lies (neighbouring nodes see neighbouring pixels; the map of one view is L2-resident).
//
// Extraction is marching tetrahedra on the Kuhn split of every cube, indexed and ordered without atomics:
//   k_tsdf_classify  a workgroup stages its 8 x 8 x 8 brick and a one-node halo on every side as two bits per node (valid, inside)
//                    in LDS, from them the "meshed" flag of the 9 x 9 x 9 cubes that touch the brick's nodes, and writes per node
//                    its 7-bit mask of active edges, that mask's popcount, its own cube's inside pattern (0 unless the cube is
//                    meshed) and the cube's triangle count;
//   two scans        splat_scan_u32's kernels over the popcounts and the triangle counts, in place: vertex and triangle bases;
//   k_tsdf_emit_vertices / k_tsdf_emit_triangles  one thread per node / cube: positions and colours of the active edges (the only
//                    re-read of the tsdf plane), and the triangles of the six tetrahedra from the table below.
// The id of edge e at node n is base[n] + popcount(mask[n] & ((1 << e) - 1)), which is the order the contract asks for.
//
// The case table (which edges of a tetrahedron carry a triangle's corners, and in which order they run counter-clockwise seen
// from outside) is not typed in: make_tet_table() builds it at compile time from the geometry, in integers, with the edges'
// midpoints standing for the vertices.  tests/tsdf_ref.py generates its own from the same rules and the GPU tests hold every one
// of the 256 patterns of a cube to it.
//
// Roofline: the passes stream the planes once and are laid out for HBM; DESIGN.md section 4, "TSDF fusion and meshing", has the
// measured times beside the traffic floors and says what bounds each pass where it is not the traffic.
#include "common.h"

#include <math.h>

namespace {

constexpr uint32_t TSDF_MAX_DIM = 2048, TSDF_MAX_NODES = 1u << 30, TSDF_MAX_SIDE = 65535;
constexpr int IBX = 32, IBY = 4, IBZ = 4; // integration brick: 512 nodes, two per thread
constexpr int EB = 8, EH = EB + 2;        // extraction brick edge; with its halo

struct TsdfView {
    float vp[16]; // by columns: VP[r][c] = vp[4 c + r]
    float eye[3];
    int distance; // depth is |X - eye| (else clip w)
    int w, h;
    const float *depth, *obs, *image;
    uint32_t stride;
    float max_weight;
};

// ---- the case table -----------------------------------------------------------------------------------------------------------
// Cube corners are 3-bit masks (bit 0: +x, bit 1: +y, bit 2: +z).  Tetrahedron p of a cube has the corners 0, e_a, e_a + e_b, 7
// for the p-th permutation (a, b, c) of the axes in lexicographic order.  An edge between tetrahedron vertices lo < hi is owned by
// corner[lo] and runs in the direction corner[hi] ^ corner[lo], one of the seven edge numbers.
struct TetCase {
    uint8_t n;    // triangle corners: 0, 3 (one triangle) or 4 (a quad)
    uint8_t v[4]; // (owning corner << 3) | edge number, in counter-clockwise order seen from outside
};
struct TetTable {
    TetCase c[6][16];     // [tetrahedron][inside bits of its four vertices]
    uint8_t corner[6][4]; // the tetrahedron's vertices as cube corners
};
constexpr int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int EDGE_OF_DIR[8] = {-1, 0, 1, 3, 2, 4, 5, 6}; // direction mask -> edge number: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
constexpr int DIR_OF_EDGE[7] = {1, 2, 4, 3, 5, 6, 7};

constexpr TetTable make_tet_table() {
    TetTable t{};
    for (int p = 0; p < 6; ++p) {
        const int cm[4] = {0, 1 << PERM[p][0], (1 << PERM[p][0]) | (1 << PERM[p][1]), 7};
        for (int k = 0; k < 4; ++k) t.corner[p][k] = (uint8_t)cm[k];
        for (int m = 0; m < 16; ++m) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
            for (int k = 0; k < 4; ++k) {
                if ((m >> k) & 1) in[nin++] = k;
                else out[nout++] = k;
            }
            int cyc[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, n = 0;
            if (nin == 1) {
                for (int q = 0; q < 3; ++q) cyc[q][0] = in[0], cyc[q][1] = out[q];
                n = 3;
            } else if (nin == 3) {
                for (int q = 0; q < 3; ++q) cyc[q][0] = out[0], cyc[q][1] = in[q];
                n = 3;
            } else if (nin == 2) { // a-c, a-d, b-d, b-c: neighbours in the cycle share a tetrahedron vertex
                cyc[0][0] = in[0], cyc[0][1] = out[0];
                cyc[1][0] = in[0], cyc[1][1] = out[1];
                cyc[2][0] = in[1], cyc[2][1] = out[1];
                cyc[3][0] = in[1], cyc[3][1] = out[0];
                n = 4;
            }
            t.c[p][m].n = (uint8_t)n;
            if (n == 0) continue;
            // twice the edges' midpoints; the normal of the first three; the direction from the inside vertices' centroid to the
            // outside ones' (times nin nout)
            int P[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, D[3] = {0, 0, 0};
            for (int q = 0; q < n; ++q)
                for (int x = 0; x < 3; ++x) P[q][x] = ((cm[cyc[q][0]] >> x) & 1) + ((cm[cyc[q][1]] >> x) & 1);
            for (int x = 0; x < 3; ++x) {
                for (int k = 0; k < nout; ++k) D[x] += nin * ((cm[out[k]] >> x) & 1);
                for (int k = 0; k < nin; ++k) D[x] -= nout * ((cm[in[k]] >> x) & 1);
            }
            const int a[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
            const int b[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
            const int dot = (a[1] * b[2] - a[2] * b[1]) * D[0] + (a[2] * b[0] - a[0] * b[2]) * D[1] + (a[0] * b[1] - a[1] * b[0]) * D[2];
            if (dot < 0) { // run the cycle the other way round, from the same start
                const int last = n - 1;
                const int s0 = cyc[1][0], s1 = cyc[1][1];
                cyc[1][0] = cyc[last][0], cyc[1][1] = cyc[last][1];
                cyc[last][0] = s0, cyc[last][1] = s1;
            }
            for (int q = 0; q < n; ++q) {
                const int lo = cyc[q][0] < cyc[q][1] ? cyc[q][0] : cyc[q][1], hi = cyc[q][0] < cyc[q][1] ? cyc[q][1] : cyc[q][0];
                t.c[p][m].v[q] = (uint8_t)((cm[lo] << 3) | EDGE_OF_DIR[cm[hi] ^ cm[lo]]);
            }
        }
    }
    return t;
}
__constant__ TetTable c_tet = make_tet_table();

// ---- integration --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float node_coord(float origin, float voxel, uint32_t i) { return fmaf(voxel, (float)i, origin); }
__device__ __forceinline__ float clip_row(const float *vp, int r, float x, float y, float z) {
    return fmaf(vp[r], x, fmaf(vp[4 + r], y, fmaf(vp[8 + r], z, vp[12 + r])));
}

// Whether no node of the brick [i0, i1] x [j0, j1] x [k0, k1] (its corner NODES) can be written by this view.  Lane l evaluates
// corner l & 7 in float64; wave-uniform result; every lane of the wave must call it.
__device__ __forceinline__ bool brick_unseen(const splat_tsdf_grid &g, const TsdfView &v, uint32_t i0, uint32_t j0, uint32_t k0) {
    const uint32_t c = threadIdx.x & 7u;
    const uint32_t i1 = min(i0 + IBX, g.dims[0]) - 1u, j1 = min(j0 + IBY, g.dims[1]) - 1u, k1 = min(k0 + IBZ, g.dims[2]) - 1u;
    const double x = (double)g.origin[0] + (double)g.voxel * (double)((c & 1u) ? i1 : i0);
    const double y = (double)g.origin[1] + (double)g.voxel * (double)((c & 2u) ? j1 : j0);
    const double z = (double)g.origin[2] + (double)g.voxel * (double)((c & 4u) ? k1 : k0);
    double cl[3], ab[3]; // rows 0, 1, 3 of VP on the corner, and the sums of the absolute values of their terms
    const int rows[3] = {0, 1, 3};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int r = rows[q];
        const double tx = (double)v.vp[r] * x, ty = (double)v.vp[4 + r] * y, tz = (double)v.vp[8 + r] * z, tw = (double)v.vp[12 + r];
        cl[q] = ((tx + ty) + tz) + tw;
        ab[q] = ((fabs(tx) + fabs(ty)) + fabs(tz)) + fabs(tw);
    }
    const double W = (double)v.w, H = (double)v.h;
    const bool behind = cl[2] < -0x1p-20 * ab[2];
    const bool safe = cl[2] > (ab[0] + ab[2]) * W * 0x1p-19 && cl[2] > (ab[1] + ab[2]) * H * 0x1p-19;
    const double pu = (cl[0] / cl[2] * 0.5 + 0.5) * W, pv = (0.5 - 0.5 * cl[1] / cl[2]) * H;
    if (__all(behind)) return true;
    if (!__all(safe)) return false;
    return __all(pu < -1.0) || __all(pu > W + 1.0) || __all(pv < -1.0) || __all(pv > H + 1.0);
}

// The contract's ten steps for node (i, j, k), linear index n
template <bool COLOR>
__device__ __forceinline__ void integrate_node(const splat_tsdf_grid &g, const TsdfView &v, uint32_t i, uint32_t j, uint32_t k, size_t n,
                                               float *__restrict__ tsdf, float *__restrict__ weight, float *__restrict__ color) {
    const float x = node_coord(g.origin[0], g.voxel, i), y = node_coord(g.origin[1], g.voxel, j), z = node_coord(g.origin[2], g.voxel, k);
    const float cw = clip_row(v.vp, 3, x, y, z);
    if (!(cw > 0.0f)) return;
    const float cx = clip_row(v.vp, 0, x, y, z), cy = clip_row(v.vp, 1, x, y, z);
    const float fw = (float)v.w, fh = (float)v.h;
    const float pu = fmaf(cx / cw, 0.5f, 0.5f) * fw, pv = fmaf(cy / cw, -0.5f, 0.5f) * fh;
    if (!(pu >= 0.0f && pu < fw && pv >= 0.0f && pv < fh)) return; // (false for a NaN)
    const int ix = (int)floorf(pu), iy = (int)floorf(pv);
    if (ix >= v.w || iy >= v.h) return; // (pu < fw already: kept as the bound of the loads below)
    const size_t p = (size_t)iy * (size_t)v.w + (size_t)ix;
    const float D = v.depth[p];
    if (!(D > 0.0f && D <= 3.402823466e38f)) return;
    float a = 1.0f;
    if (v.obs) {
        a = v.obs[p];
        if (!(a > 0.0f)) return;
    }
    float r = cw;
    if (v.distance) {
        const float dx = x - v.eye[0], dy = y - v.eye[1], dz = z - v.eye[2];
        r = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    }
    const float s = D - r;
    if (s < -g.trunc) return;
    const float f = fminf(1.0f, s / g.trunc);
    const float w0 = weight[n];
    const bool seen = w0 > 0.0f; // (a node of weight 0 has no value yet: its tsdf and colour are not read)
    const float w1 = w0 + a;
    const float t0 = seen ? tsdf[n] : 0.0f;
    tsdf[n] = fmaf(t0, w0, f * a) / w1;
    if constexpr (COLOR) {
        const float *px = v.image + p * v.stride;
        float *c = color + 3 * n;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float c0 = seen ? c[q] : 0.0f;
            c[q] = fmaf(c0, w0, px[q] * a) / w1;
        }
    }
    weight[n] = v.max_weight > 0.0f ? fminf(w1, v.max_weight) : w1;
}

template <bool COLOR>
__global__ __launch_bounds__(256) void k_tsdf_integrate(splat_tsdf_grid g, TsdfView v, float *__restrict__ tsdf, float *__restrict__ weight,
                                                        float *__restrict__ color) {
    const uint32_t tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * IBX, j0 = blockIdx.y * IBY, k0 = blockIdx.z * IBZ;
    if (brick_unseen(g, v, i0, j0, k0)) return;
    const uint32_t i = i0 + (tid & (IBX - 1)), j = j0 + ((tid >> 5) & (IBY - 1));
    if (i >= g.dims[0] || j >= g.dims[1]) return;
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
        const uint32_t k = k0 + (tid >> 7) + 2u * half;
        if (k < g.dims[2]) integrate_node<COLOR>(g, v, i, j, k, (size_t)i + (size_t)g.dims[0] * ((size_t)j + (size_t)g.dims[1] * k), tsdf, weight, color);
    }
}

// ---- extraction ---------------------------------------------------------------------------------------------------------------
struct MeshWs {
    uint32_t *vbase, *tbase; // per node: popcount of its edge mask / its cube's triangle count; after the scans, the bases
    uint8_t *mask, *cfg;     // per node: active edges; inside bits of its cube's corners (0 unless the cube is meshed)
    uint32_t *totals;        // {vertices, triangles}
};
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
uint64_t mesh_ws_bytes(uint64_t nodes) { return 2 * align256(4 * nodes) + 2 * align256(nodes) + 256; }
MeshWs mesh_ws(void *workspace, uint64_t nodes) {
    char *p = (char *)workspace;
    MeshWs w;
    w.vbase = (uint32_t *)p, p += align256(4 * nodes);
    w.tbase = (uint32_t *)p, p += align256(4 * nodes);
    w.mask = (uint8_t *)p, p += align256(nodes);
    w.cfg = (uint8_t *)p, p += align256(nodes);
    w.totals = (uint32_t *)p;
    return w;
}

__global__ __launch_bounds__(256) void k_tsdf_classify(uint32_t nx, uint32_t ny, uint32_t nz, const float *__restrict__ tsdf,
                                                       const float *__restrict__ weight, float min_weight, MeshWs ws) {
    __shared__ uint8_t s_node[EH][EH][EH];             // bit 0: valid, bit 1: inside; the brick's nodes are at [1, EB] on each axis
    __shared__ uint8_t s_cube[EH - 1][EH - 1][EH - 1]; // the cube whose lower corner is s_node[z][y][x] is meshed
    const int tid = threadIdx.x;
    const int i0 = (int)(blockIdx.x * EB), j0 = (int)(blockIdx.y * EB), k0 = (int)(blockIdx.z * EB);
    for (int q = tid; q < EH * EH * EH; q += 256) {
        const int z = q / (EH * EH), y = (q / EH) % EH, x = q % EH;
        const int gi = i0 - 1 + x, gj = j0 - 1 + y, gk = k0 - 1 + z;
        uint8_t b = 0;
        if (gi >= 0 && gi < (int)nx && gj >= 0 && gj < (int)ny && gk >= 0 && gk < (int)nz) {
            const size_t n = (size_t)gi + (size_t)nx * ((size_t)gj + (size_t)ny * (size_t)gk);
            if (weight[n] > min_weight) b = tsdf[n] < 0.0f ? 3 : 1; // (an invalid node's tsdf is not read; exactly 0, -0 and NaN are outside)
        }
        s_node[z][y][x] = b;
    }
    __syncthreads();
    for (int q = tid; q < (EH - 1) * (EH - 1) * (EH - 1); q += 256) {
        const int z = q / ((EH - 1) * (EH - 1)), y = (q / (EH - 1)) % (EH - 1), x = q % (EH - 1);
        uint8_t all = 1; // (a node outside the grid was staged invalid: a cube that reaches past the grid is never meshed)
#pragma unroll
        for (int c = 0; c < 8; ++c) all &= s_node[z + (c >> 2)][y + ((c >> 1) & 1)][x + (c & 1)];
        s_cube[z][y][x] = all;
    }
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int q = tid + 256 * half;
        const int x = (q & 7) + 1, y = ((q >> 3) & 7) + 1, z = (q >> 6) + 1;
        const uint32_t gi = (uint32_t)(i0 + x - 1), gj = (uint32_t)(j0 + y - 1), gk = (uint32_t)(k0 + z - 1);
        if (gi >= nx || gj >= ny || gk >= nz) continue;
        const uint32_t own = s_node[z][y][x];
        uint32_t pattern = 0, mask = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) pattern |= (uint32_t)((s_node[z + (c >> 2)][y + ((c >> 1) & 1)][x + (c & 1)] >> 1) & 1) << c;
        const uint32_t cfg = s_cube[z][y][x] ? pattern : 0u;
        // edge e (direction d) of this node lies in the cubes whose lower corner is this node minus o, for every o disjoint from d
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            const int d = DIR_OF_EDGE[e];
            const uint32_t other = s_node[z + (d >> 2)][y + ((d >> 1) & 1)][x + (d & 1)];
            uint32_t meshed = 0;
#pragma unroll
            for (int o = 0; o < 7; ++o)
                if ((o & d) == 0) meshed |= s_cube[z - (o >> 2)][y - ((o >> 1) & 1)][x - (o & 1)];
            if (((own ^ other) & 2u) && meshed) mask |= 1u << e;
        }
        uint32_t tris = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const uint32_t in = ((cfg >> c_tet.corner[p][0]) & 1u) + ((cfg >> c_tet.corner[p][1]) & 1u) + ((cfg >> c_tet.corner[p][2]) & 1u) +
                                ((cfg >> c_tet.corner[p][3]) & 1u);
            tris += in == 2u ? 2u : (in == 1u || in == 3u) ? 1u : 0u;
        }
        const size_t n = (size_t)gi + (size_t)nx * ((size_t)gj + (size_t)ny * (size_t)gk);
        ws.mask[n] = (uint8_t)mask;
        ws.cfg[n] = (uint8_t)cfg;
        ws.vbase[n] = __popc(mask);
        ws.tbase[n] = tris;
    }
}

// One thread per node: the vertices of its active edges.  t = f0 / (f0 - f1) from the lower endpoint; position and colour are
// fmaf(t, end - start, start).
__global__ __launch_bounds__(256) void k_tsdf_emit_vertices(splat_tsdf_grid g, const float *__restrict__ tsdf, const float *__restrict__ color,
                                                            MeshWs ws, float *__restrict__ vertices, float *__restrict__ vcolors) {
    const uint32_t nodes = g.dims[0] * g.dims[1] * g.dims[2];
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nodes) return;
    const uint32_t mask = ws.mask[n];
    if (!mask) return;
    const uint32_t nx = g.dims[0], ny = g.dims[1];
    const uint32_t i = n % nx, j = (n / nx) % ny, k = n / (nx * ny);
    const float p0[3] = {node_coord(g.origin[0], g.voxel, i), node_coord(g.origin[1], g.voxel, j), node_coord(g.origin[2], g.voxel, k)};
    const float f0 = tsdf[n];
    uint32_t id = ws.vbase[n];
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        if (!((mask >> e) & 1u)) continue;
        const int d = DIR_OF_EDGE[e];
        const uint32_t di = d & 1, dj = (d >> 1) & 1, dk = d >> 2;
        const uint32_t n1 = n + di + nx * (dj + ny * dk);
        const float f1 = tsdf[n1];
        const float t = f0 / (f0 - f1);
        const float p1[3] = {node_coord(g.origin[0], g.voxel, i + di), node_coord(g.origin[1], g.voxel, j + dj),
                             node_coord(g.origin[2], g.voxel, k + dk)};
        float *o = vertices + 3 * (size_t)id;
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = fmaf(t, p1[q] - p0[q], p0[q]);
        if (vcolors) {
            const float *c0 = color + 3 * (size_t)n, *c1 = color + 3 * (size_t)n1;
            float *oc = vcolors + 3 * (size_t)id;
#pragma unroll
            for (int q = 0; q < 3; ++q) oc[q] = fmaf(t, c1[q] - c0[q], c0[q]);
        }
        ++id;
    }
}

// One thread per cube (named by its lower corner): the triangles of its six tetrahedra, in order
__global__ __launch_bounds__(256) void k_tsdf_emit_triangles(uint32_t nx, uint32_t ny, uint32_t nz, MeshWs ws, uint32_t *__restrict__ triangles) {
    const uint32_t nodes = nx * ny * nz;
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nodes) return;
    const uint32_t cfg = ws.cfg[n];
    if (cfg == 0u || cfg == 255u) return;
    uint32_t *out = triangles + 3 * (size_t)ws.tbase[n];
#pragma unroll 1
    for (int p = 0; p < 6; ++p) {
        const uint32_t m = ((cfg >> c_tet.corner[p][0]) & 1u) | (((cfg >> c_tet.corner[p][1]) & 1u) << 1) | (((cfg >> c_tet.corner[p][2]) & 1u) << 2) |
                           (((cfg >> c_tet.corner[p][3]) & 1u) << 3);
        const TetCase &tc = c_tet.c[p][m];
        if (tc.n == 0) continue;
        uint32_t id[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < tc.n) {
                const uint32_t corner = tc.v[q] >> 3, e = tc.v[q] & 7u;
                const uint32_t owner = n + (corner & 1u) + nx * (((corner >> 1) & 1u) + ny * (corner >> 2)); // (a meshed cube: inside the grid)
                id[q] = ws.vbase[owner] + __popc((uint32_t)ws.mask[owner] & ((1u << e) - 1u));
            }
        }
        uint32_t a = id[0], b = id[1], c = id[2], d = id[3];
        if (tc.n == 3) { // rotated so that the smallest id comes first
            if (b < a && b < c) { const uint32_t s = a; a = b; b = c; c = s; }
            else if (c < a && c < b) { const uint32_t s = c; c = b; b = a; a = s; }
            out[0] = a; out[1] = b; out[2] = c;
            out += 3;
        } else { // the cycle rotated to start at the smallest id, split along the diagonal from it
            if (b < a && b < c && b < d) { const uint32_t s = a; a = b; b = c; c = d; d = s; }
            else if (c < a && c < b && c < d) { uint32_t s = a; a = c; c = s; s = b; b = d; d = s; }
            else if (d < a && d < b && d < c) { const uint32_t s = d; d = c; c = b; b = a; a = s; }
            out[0] = a; out[1] = b; out[2] = c;
            out[3] = a; out[4] = c; out[5] = d;
            out += 6;
        }
    }
}

bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool positive_finite(float v) { return v > 0.0f && v <= 3.402823466e38f; }

int grid_check(splat_ctx *ctx, const splat_tsdf_grid *g) {
    ARG_CHECK(ctx, g != nullptr);
    ARG_CHECK(ctx, g->dims[0] >= 1 && g->dims[1] >= 1 && g->dims[2] >= 1);
    ARG_CHECK(ctx, g->dims[0] <= TSDF_MAX_DIM && g->dims[1] <= TSDF_MAX_DIM && g->dims[2] <= TSDF_MAX_DIM);
    ARG_CHECK(ctx, (uint64_t)g->dims[0] * g->dims[1] * g->dims[2] <= TSDF_MAX_NODES);
    ARG_CHECK(ctx, positive_finite(g->voxel) && positive_finite(g->trunc));
    ARG_CHECK(ctx, fabsf(g->origin[0]) <= 3.402823466e38f && fabsf(g->origin[1]) <= 3.402823466e38f && fabsf(g->origin[2]) <= 3.402823466e38f);
    return SPLAT_OK;
}

} // namespace

extern "C" int splat_tsdf_integrate(splat_ctx *ctx, const splat_tsdf_grid *grid, void *tsdf, void *weight, void *color, const float *uniforms,
                                    uint32_t depth_kind, const void *depth, const void *obs_weight, const void *image, uint32_t image_stride,
                                    uint32_t width, uint32_t height, float max_weight) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    const int rc = grid_check(ctx, grid);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, tsdf && weight && uniforms && depth);
    ARG_CHECK(ctx, depth_kind == SPLAT_DEPTH_DISTANCE || depth_kind == SPLAT_DEPTH_Z);
    ARG_CHECK(ctx, width >= 1 && height >= 1 && width <= TSDF_MAX_SIDE && height <= TSDF_MAX_SIDE);
    ARG_CHECK(ctx, !image || image_stride >= 3);
    ARG_CHECK(ctx, max_weight >= 0.0f && max_weight <= 3.402823466e38f);
    ARG_CHECK(ctx, aligned_to(tsdf, 4) && aligned_to(weight, 4) && aligned_to(color, 4) && aligned_to(depth, 4) && aligned_to(obs_weight, 4) &&
                       aligned_to(image, 4));
    TsdfView v;
    for (int q = 0; q < 16; ++q) v.vp[q] = uniforms[q];
    for (int q = 0; q < 3; ++q) v.eye[q] = uniforms[16 + q];
    v.distance = depth_kind == SPLAT_DEPTH_DISTANCE;
    v.w = (int)width, v.h = (int)height;
    v.depth = (const float *)depth, v.obs = (const float *)obs_weight, v.image = (const float *)image;
    v.stride = image_stride;
    v.max_weight = max_weight;
    const dim3 bricks(div_up(grid->dims[0], IBX), div_up(grid->dims[1], IBY), div_up(grid->dims[2], IBZ));
    if (color && image)
        hipLaunchKernelGGL(k_tsdf_integrate<true>, bricks, dim3(256), 0, ctx->stream, *grid, v, (float *)tsdf, (float *)weight, (float *)color);
    else
        hipLaunchKernelGGL(k_tsdf_integrate<false>, bricks, dim3(256), 0, ctx->stream, *grid, v, (float *)tsdf, (float *)weight, (float *)nullptr);
    LAUNCH_CHECK(ctx, "k_tsdf_integrate");
    return SPLAT_OK;
}

extern "C" uint64_t splat_tsdf_mesh_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > TSDF_MAX_DIM || ny > TSDF_MAX_DIM || nz > TSDF_MAX_DIM) return 0;
    const uint64_t nodes = (uint64_t)nx * ny * nz;
    return nodes <= TSDF_MAX_NODES ? mesh_ws_bytes(nodes) : 0;
}

extern "C" int splat_tsdf_mesh_count(splat_ctx *ctx, const splat_tsdf_grid *grid, const void *tsdf, const void *weight, float min_weight,
                                     void *workspace, uint64_t workspace_bytes, uint32_t *n_vertices_host, uint32_t *n_triangles_host) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    int rc = grid_check(ctx, grid);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, tsdf && weight && workspace && n_vertices_host && n_triangles_host);
    ARG_CHECK(ctx, aligned_to(tsdf, 4) && aligned_to(weight, 4) && aligned_to(workspace, 16));
    ARG_CHECK(ctx, min_weight >= 0.0f && min_weight <= 3.402823466e38f);
    const uint32_t nx = grid->dims[0], ny = grid->dims[1], nz = grid->dims[2], nodes = nx * ny * nz;
    ARG_CHECK(ctx, workspace_bytes >= mesh_ws_bytes(nodes));
    rc = ctx_ensure_pinned(ctx, 2 * sizeof(uint32_t));
    if (rc != SPLAT_OK) return rc;
    const MeshWs ws = mesh_ws(workspace, nodes);
    hipLaunchKernelGGL(k_tsdf_classify, dim3(div_up(nx, EB), div_up(ny, EB), div_up(nz, EB)), dim3(256), 0, ctx->stream, nx, ny, nz,
                       (const float *)tsdf, (const float *)weight, min_weight, ws);
    LAUNCH_CHECK(ctx, "k_tsdf_classify");
    rc = scan_exclusive_u32(ctx, ws.vbase, ws.vbase, nodes, ws.totals);
    if (rc != SPLAT_OK) return rc;
    rc = scan_exclusive_u32(ctx, ws.tbase, ws.tbase, nodes, ws.totals + 1);
    if (rc != SPLAT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, ws.totals, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_vertices_host = ((const uint32_t *)ctx->pinned)[0];
    *n_triangles_host = ((const uint32_t *)ctx->pinned)[1];
    return SPLAT_OK;
}

extern "C" int splat_tsdf_mesh_emit(splat_ctx *ctx, const splat_tsdf_grid *grid, const void *tsdf, const void *color, const void *workspace,
                                    uint64_t workspace_bytes, void *vertices, void *vertex_colors, void *triangles) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    const int rc = grid_check(ctx, grid);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, tsdf && workspace && vertices && triangles);
    ARG_CHECK(ctx, !vertex_colors || color);
    ARG_CHECK(ctx, aligned_to(tsdf, 4) && aligned_to(color, 4) && aligned_to(workspace, 16) && aligned_to(vertices, 4) && aligned_to(vertex_colors, 4) &&
                       aligned_to(triangles, 4));
    const uint32_t nx = grid->dims[0], ny = grid->dims[1], nz = grid->dims[2], nodes = nx * ny * nz;
    ARG_CHECK(ctx, workspace_bytes >= mesh_ws_bytes(nodes));
    const MeshWs ws = mesh_ws(const_cast<void *>(workspace), nodes);
    hipLaunchKernelGGL(k_tsdf_emit_vertices, dim3(div_up(nodes, 256)), dim3(256), 0, ctx->stream, *grid, (const float *)tsdf, (const float *)color, ws,
                       (float *)vertices, (float *)vertex_colors);
    LAUNCH_CHECK(ctx, "k_tsdf_emit_vertices");
    hipLaunchKernelGGL(k_tsdf_emit_triangles, dim3(div_up(nodes, 256)), dim3(256), 0, ctx->stream, nx, ny, nz, ws, (uint32_t *)triangles);
    LAUNCH_CHECK(ctx, "k_tsdf_emit_triangles");
    return SPLAT_OK;
}
