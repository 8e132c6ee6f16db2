// Isosurface extraction (include/ncnerf_mesh.h states the definition; this file follows its words):
//   ncn_mesh_points      lattice positions of a range of points, the input of the density pass; with a
//                        bitfield only the points that touch an active cell, compacted
//   ncn_mesh_count       per point the mask of owned edges that carry a vertex, per cell the face count:
//                        one workgroup per 32 x 8 x 8 tile, the tile's inside / active bits with their
//                        +1 halo staged once in LDS (every lattice value is read once per tile it
//                        touches, 1.31 times on average; the eight corners come from LDS, each z level
//                        read once per thread), the mask and the count from two 256-byte tables
//                        evaluated at compile time
//   ncn_mesh_scan        ordered exclusive scan of the masks' popcounts / the face counts: u16 offsets
//                        inside blocks of 4096, then the blocks' int64 bases and the total by one workgroup
//   ncn_mesh_emit_verts  the vertices, each at its number
//   ncn_mesh_emit_faces  the faces, each at its number, their vertex numbers looked up from the owners
// Nothing here is atomic but the compaction counter of ncn_mesh_points (whose order does not matter:
// the densities are scattered back by point index).  Positions and interpolation are plain fp32, one
// rounding per operation.
#pragma clang fp contract(off)

#include <cmath>
#include "workgroup.h"
#include "vren_march.h"
#include "../../include/ncnerf_mesh.h"

namespace ncn {

constexpr int MT_X = NCN_MESH_TILE_X, MT_Y = NCN_MESH_TILE_Y, MT_Z = NCN_MESH_TILE_Z;
constexpr int MESH_THREADS = 256;
constexpr int SCAN_PER_THREAD = NCN_MESH_SCAN_ELEMS / MESH_THREADS;  // 16 bytes: one dwordx4 per thread
static_assert(MT_X * MT_Y == MESH_THREADS && SCAN_PER_THREAD == 16, "tile rows / scan loads are sized to 256 threads");
static_assert(NCN_MESH_SCAN_ELEMS * 15 < 65536, "a block's offsets fit uint16");

struct Lattice {
    int64_t nx, ny, nz;
    float lo[3], h[3];
    const uint8_t* bitfield;  // NULL: every cell is active
    int G;
    float scale;
};

static Lattice make_lattice(int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z, float hi_x,
                            float hi_y, float hi_z, const uint8_t* bitfield, int G, float scale) {
    Lattice L;
    L.nx = nx, L.ny = ny, L.nz = nz;
    L.lo[0] = lo_x, L.lo[1] = lo_y, L.lo[2] = lo_z;
    L.h[0] = (hi_x - lo_x) / (float)nx, L.h[1] = (hi_y - lo_y) / (float)ny, L.h[2] = (hi_z - lo_z) / (float)nz;
    L.bitfield = bitfield, L.G = G, L.scale = scale;
    return L;
}

__device__ __forceinline__ float lattice_pos(const Lattice& L, int axis, int64_t i) {
    return L.lo[axis] + (float)i * L.h[axis];
}

// the cell exists and (no bitfield, or) the occupancy cell around its centre is set: the marcher's probe, cascade 0
// (coordinates are ints: check_lattice keeps every axis below 2^20)
__device__ __forceinline__ bool cell_active(const Lattice& L, int cx, int cy, int cz) {
    if (cx < 0 || cy < 0 || cz < 0 || cx >= (int)L.nx || cy >= (int)L.ny || cz >= (int)L.nz) return false;
    if (L.bitfield == nullptr) return true;
    const float x = L.lo[0] + ((float)cx + 0.5f) * L.h[0];
    const float y = L.lo[1] + ((float)cy + 0.5f) * L.h[1];
    const float z = L.lo[2] + ((float)cz + 0.5f) * L.h[2];
    const MarchConst m = make_march_const(1, L.scale, 0.0f, L.G, 1, L.scale);
    int a, b, c;
    float mip_bound;
    uint32_t cache_bi = ~0u, cache_b = 0;
    return probe<true>(m, L.bitfield, x, y, z, 0.0f, a, b, c, mip_bound, cache_bi, cache_b);
}

// the Kuhn split: corner v1 and v2 of the six tetrahedra (v0 = 0, v3 = 7) and their signs
__device__ constexpr int TET_V1[6] = {1, 1, 2, 2, 4, 4};
__device__ constexpr int TET_V2[6] = {3, 5, 3, 6, 5, 6};
__device__ constexpr int TET_SIGN[6] = {1, -1, -1, 1, 1, -1};

// ---- the two byte tables of ncn_mesh_count, evaluated at compile time ----
struct ByteTable {
    uint8_t v[256];
};
// by the inside bits of a cell's eight corners (bit d = corner d): the face count of its six tetrahedra
constexpr ByteTable make_cell_faces() {
    constexpr int v1[6] = {1, 1, 2, 2, 4, 4}, v2[6] = {3, 5, 3, 6, 5, 6};
    ByteTable t{};
    for (int in8 = 0; in8 < 256; in8++) {
        int nf = 0;
        for (int q = 0; q < 6; q++) {
            const int k = (in8 & 1) + ((in8 >> v1[q]) & 1) + ((in8 >> v2[q]) & 1) + ((in8 >> 7) & 1);
            nf += (k == 2) ? 2 : (k == 1 || k == 3) ? 1 : 0;
        }
        t.v[in8] = (uint8_t)nf;
    }
    return t;
}
// by the active bits of a point's eight incident cells (bit e set = the cell at the point's coordinate on the
// axes of e, one less on the others): bit d - 1 set when the edge of direction d lies in an active cell,
// i.e. in one of the cells e that contain d's axes
constexpr ByteTable make_edge_active() {
    constexpr int cells[8] = {0xFF, 0xAA, 0xCC, 0x88, 0xF0, 0xA0, 0xC0, 0x80};
    ByteTable t{};
    for (int act8 = 0; act8 < 256; act8++) {
        int m = 0;
        for (int d = 1; d < 8; d++)
            if (act8 & cells[d]) m |= 1 << (d - 1);
        t.v[act8] = (uint8_t)m;
    }
    return t;
}
__device__ constexpr ByteTable CELL_FACES = make_cell_faces();
__device__ constexpr ByteTable EDGE_ACTIVE = make_edge_active();

// ---- the triangles of one tetrahedron of sign +1, by its inside bits (corner i = bit i): the header's
//      rule evaluated at compile time.  Packed: bits 24.. the triangle count, 4 bits per vertex
//      (6 vertices), a vertex being the edge (a, b), a < b, as a * 4 + b. ----
constexpr uint32_t tet_edge(int a, int b) { return a < b ? (uint32_t)(a * 4 + b) : (uint32_t)(b * 4 + a); }
constexpr uint32_t tet_case(int bits) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int v = 0; v < 4; v++) {
        if ((bits >> v) & 1) in[ni++] = v;
        else out[no++] = v;
    }
    uint32_t e[6] = {0, 0, 0, 0, 0, 0};
    uint32_t n = 0;
    int i = 0, j = 0, k = 0, l = 0;
    bool flip = false;
    if (ni == 1 || ni == 3) {
        const int* rest = ni == 1 ? out : in;
        i = ni == 1 ? in[0] : out[0], j = rest[0], k = rest[1], l = rest[2];
        e[0] = tet_edge(i, j), e[1] = tet_edge(i, k), e[2] = tet_edge(i, l);
        n = 1;
        flip = ni == 3;
    } else if (ni == 2) {
        i = in[0], j = in[1], k = out[0], l = out[1];
        e[0] = tet_edge(i, k), e[1] = tet_edge(i, l), e[2] = tet_edge(j, l);
        e[3] = e[0], e[4] = e[2], e[5] = tet_edge(j, k);
        n = 2;
    }
    const int inversions = (i > j) + (i > k) + (i > l) + (j > k) + (j > l) + (k > l);
    if (((inversions & 1) != 0) != flip) {
        uint32_t t = e[1];
        e[1] = e[2], e[2] = t;
        t = e[4], e[4] = e[5], e[5] = t;
    }
    uint32_t w = n << 24;
    for (int q = 0; q < 6; q++) w |= e[q] << (4 * q);
    return w;
}
__device__ constexpr uint32_t TET_CASES[16] = {tet_case(0),  tet_case(1),  tet_case(2),  tet_case(3),
                                               tet_case(4),  tet_case(5),  tet_case(6),  tet_case(7),
                                               tet_case(8),  tet_case(9),  tet_case(10), tet_case(11),
                                               tet_case(12), tet_case(13), tet_case(14), tet_case(15)};

// ---- points ----
__global__ __launch_bounds__(MESH_THREADS) void mesh_points_kernel(Lattice L, int64_t p0, int64_t n,
                                                                   float* __restrict__ xyz, int64_t* __restrict__ idx,
                                                                   int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    const bool live = i < n;
    const int64_t p = p0 + (live ? i : 0);
    const int64_t ix = p % (L.nx + 1), iy = (p / (L.nx + 1)) % (L.ny + 1), iz = p / ((L.nx + 1) * (L.ny + 1));
    const float x = lattice_pos(L, 0, ix), y = lattice_pos(L, 1, iy), z = lattice_pos(L, 2, iz);
    if (L.bitfield == nullptr) {
        if (live) xyz[3 * i] = x, xyz[3 * i + 1] = y, xyz[3 * i + 2] = z;
        return;
    }
    bool act = false;
    if (live) {
#pragma unroll
        for (int e = 0; e < 8; e++) act = act || cell_active(L, (int)ix - 1 + (e & 1), (int)iy - 1 + ((e >> 1) & 1), (int)iz - 1 + (e >> 2));
    }
    // one atomic per wave: the first active lane reserves the wave's slots
    const unsigned long long b = __ballot(act);
    if (b == 0) return;  // wave-uniform
    const int lane = lane_id(), leader = __ffsll(b) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(count, __popcll(b));
    base = shfl_i(base, leader);
    if (act) {
        const int64_t o = (int64_t)base + __popcll(b & ((1ull << lane) - 1ull));
        if (o < n) {  // (always: at most n points are active)
            xyz[3 * o] = x, xyz[3 * o + 1] = y, xyz[3 * o + 2] = z;
            idx[o] = p;
        }
    }
}

// ---- count ----
__global__ __launch_bounds__(MESH_THREADS) void mesh_count_kernel(Lattice L, const float* __restrict__ sigma, float iso,
                                                                  uint8_t* __restrict__ mask, uint8_t* __restrict__ nfaces) {
    // bit 0: the point (x0 + lx, y0 + ly, z0 + lz) is inside; bit 4: the cell one lower on every axis,
    // (x0 - 1 + lx, ...), is active.  A thread's eight corners are then also its eight incident cells, and
    // the four bytes of one z level, shifted by their corner number and or-ed, are that level's four
    // inside bits (0..3) and four active bits (4..7).
    __shared__ uint8_t tile[MT_Z + 1][MT_Y + 1][MT_X + 4];
    __shared__ uint8_t cell_faces[256], edge_active[256];
    const int x0 = (int)blockIdx.x * MT_X, y0 = (int)blockIdx.y * MT_Y, z0 = (int)blockIdx.z * MT_Z;
    const int nx = (int)L.nx, ny = (int)L.ny, nz = (int)L.nz;
    const int64_t sx = L.nx + 1, sy = L.ny + 1;
    cell_faces[threadIdx.x] = CELL_FACES.v[threadIdx.x];
    edge_active[threadIdx.x] = EDGE_ACTIVE.v[threadIdx.x];
    for (int e = threadIdx.x; e < (MT_Z + 1) * (MT_Y + 1) * (MT_X + 1); e += MESH_THREADS) {
        const int lx = e % (MT_X + 1), ly = (e / (MT_X + 1)) % (MT_Y + 1), lz = e / ((MT_X + 1) * (MT_Y + 1));
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        int bits = 0;
        if (x <= nx && y <= ny && z <= nz) bits = sigma[((int64_t)z * sy + y) * sx + x] >= iso ? 1 : 0;
        if (cell_active(L, x - 1, y - 1, z - 1)) bits |= 16;
        tile[lz][ly][lx] = (uint8_t)bits;
    }
    __syncthreads();
    const int tx = threadIdx.x & (MT_X - 1), ty = threadIdx.x / MT_X;
    const int x = x0 + tx, y = y0 + ty;
    if (x > nx || y > ny) return;
    auto level = [&](int lz) {
        return (int)tile[lz][ty][tx] | ((int)tile[lz][ty][tx + 1] << 1) | ((int)tile[lz][ty + 1][tx] << 2) |
               ((int)tile[lz][ty + 1][tx + 1] << 3);
    };
    int64_t p = ((int64_t)z0 * sy + y) * sx + x, c = ((int64_t)z0 * ny + y) * nx + x;
    const bool owns_cell = x < nx && y < ny;
    int lo = level(0);
#pragma unroll
    for (int lz = 0; lz < MT_Z; lz++) {
        const int z = z0 + lz;
        if (z > nz) break;
        const int hi = level(lz + 1);
        const int in8 = (lo & 0xF) | ((hi & 0xF) << 4), act8 = (lo >> 4) | (hi & 0xF0);
        const int differs = in8 ^ ((in8 & 1) ? 0xFF : 0);  // bit d: corner d and the point differ in the inside test
        mask[p] = (uint8_t)((differs >> 1) & edge_active[act8]);
        if (owns_cell && z < nz) nfaces[c] = (act8 & 0x80) ? cell_faces[in8] : (uint8_t)0;
        lo = hi;
        p += sx * sy;
        c += (int64_t)nx * ny;
    }
}

// ---- scan ----
__device__ __forceinline__ uint32_t byte_popcounts(uint32_t w) {
    w = w - ((w >> 1) & 0x55555555u);
    w = (w & 0x33333333u) + ((w >> 2) & 0x33333333u);
    return (w + (w >> 4)) & 0x0F0F0F0Fu;
}

// offsets inside one block of NCN_MESH_SCAN_ELEMS elements and the block's sum (into block_base[b])
__global__ __launch_bounds__(MESH_THREADS) void mesh_scan_local_kernel(const uint8_t* __restrict__ in, int64_t n, int popcount,
                                                                       uint16_t* __restrict__ local,
                                                                       int64_t* __restrict__ block_base) {
    __shared__ int wave_total[MESH_THREADS / WAVE];
    const int64_t e0 = (int64_t)blockIdx.x * NCN_MESH_SCAN_ELEMS + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    const bool full = e0 + SCAN_PER_THREAD <= n;
    uint32_t w[4] = {0, 0, 0, 0};
    if (full) {
        const uint4 q = *reinterpret_cast<const uint4*>(in + e0);
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
        for (int q = 0; q < SCAN_PER_THREAD; q++)
            if (e0 + q < n) w[q >> 2] |= (uint32_t)in[e0 + q] << (8 * (q & 3));
    }
    int v[SCAN_PER_THREAD], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t c = popcount ? byte_popcounts(w[q]) : (w[q] & 0x0F0F0F0Fu);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            v[4 * q + r] = sum;  // exclusive inside the thread
            sum += (c >> (8 * r)) & 0xFF;
        }
    }
    int total;
    const int before = block_excl_scan<MESH_THREADS>(sum, total, wave_total);
    if (full) {
        uint32_t o[8];
#pragma unroll
        for (int q = 0; q < 8; q++) o[q] = (uint32_t)(v[2 * q] + before) | ((uint32_t)(v[2 * q + 1] + before) << 16);
        uint4* dst = reinterpret_cast<uint4*>(local + e0);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    } else {
        for (int q = 0; q < SCAN_PER_THREAD; q++)
            if (e0 + q < n) local[e0 + q] = (uint16_t)(v[q] + before);
    }
    if (threadIdx.x == 0) block_base[blockIdx.x] = total;
}

// block sums -> exclusive int64 bases in place, by ONE workgroup sweeping NCN_MESH_SCAN_SWEEP sums at a time
__global__ __launch_bounds__(NCN_MESH_SCAN_SWEEP) void mesh_scan_base_kernel(int64_t* __restrict__ block_base, int64_t nb,
                                                                             int64_t* __restrict__ total) {
    __shared__ long long wave_total[NCN_MESH_SCAN_SWEEP / WAVE];
    long long carry = 0;
    for (int64_t s0 = 0; s0 < nb; s0 += NCN_MESH_SCAN_SWEEP) {  // (uniform trip count: the barriers are safe)
        const int64_t i = s0 + threadIdx.x;
        const long long own = i < nb ? (long long)block_base[i] : 0;
        const long long before = block_excl_sweep<NCN_MESH_SCAN_SWEEP>(own, carry, wave_total);
        if (i < nb) block_base[i] = (int64_t)before;
    }
    if (threadIdx.x == 0) total[0] = (int64_t)carry;
}

// ---- emit ----
// number of the vertex on the edge of direction d owned by point p (the header's formula)
__device__ __forceinline__ int64_t vertex_number(const uint8_t* __restrict__ mask, const uint16_t* __restrict__ vlocal,
                                                 const int64_t* __restrict__ vbase, int64_t p, int d) {
    return vbase[p / NCN_MESH_SCAN_ELEMS] + (int64_t)vlocal[p] + __popc((unsigned)mask[p] & ((1u << (d - 1)) - 1u));
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_emit_verts_kernel(Lattice L, const float* __restrict__ sigma, float iso,
                                                                       const uint8_t* __restrict__ mask,
                                                                       const uint16_t* __restrict__ vlocal,
                                                                       const int64_t* __restrict__ vbase,
                                                                       float* __restrict__ verts, int64_t n_verts) {
    const int64_t sx = L.nx + 1, sy = L.ny + 1, P = sx * sy * (L.nz + 1);
    const int64_t p = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (p >= P) return;
    const int m = mask[p];
    if (m == 0) return;
    const int64_t ix = p % sx, iy = (p / sx) % sy, iz = p / (sx * sy);
    const float sa = sigma[p];
    const float pa[3] = {lattice_pos(L, 0, ix), lattice_pos(L, 1, iy), lattice_pos(L, 2, iz)};
    int64_t v = vbase[p / NCN_MESH_SCAN_ELEMS] + (int64_t)vlocal[p];
#pragma unroll
    for (int d = 1; d < 8; d++) {
        if (!((m >> (d - 1)) & 1)) continue;
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        if (ix + dx <= L.nx && iy + dy <= L.ny && iz + dz <= L.nz && v >= 0 && v < n_verts) {
            const float sb = sigma[p + dx + dy * sx + dz * sx * sy];
            const float t = (std::isfinite(sa) && std::isfinite(sb)) ? (iso - sa) / (sb - sa) : 0.5f;
            const float pb[3] = {lattice_pos(L, 0, ix + dx), lattice_pos(L, 1, iy + dy), lattice_pos(L, 2, iz + dz)};
#pragma unroll
            for (int a = 0; a < 3; a++) verts[3 * v + a] = pa[a] + t * (pb[a] - pa[a]);
        }
        v++;
    }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_emit_faces_kernel(
    int64_t nx, int64_t ny, int64_t nz, const float* __restrict__ sigma, float iso, const uint8_t* __restrict__ mask,
    const uint16_t* __restrict__ vlocal, const int64_t* __restrict__ vbase, const uint8_t* __restrict__ nfaces,
    const uint16_t* __restrict__ flocal, const int64_t* __restrict__ fbase, int64_t* __restrict__ faces, int64_t n_faces) {
    const int64_t C = nx * ny * nz, c = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (c >= C) return;
    if (nfaces[c] == 0) return;
    const int64_t ix = c % nx, iy = (c / nx) % ny, iz = c / (nx * ny);
    const int64_t sx = nx + 1, sy = ny + 1;
    const int64_t p000 = (iz * sy + iy) * sx + ix;
    int in8 = 0;
#pragma unroll
    for (int d = 0; d < 8; d++)
        in8 |= (sigma[p000 + (d & 1) + ((d >> 1) & 1) * sx + (d >> 2) * sx * sy] >= iso ? 1 : 0) << d;
    int64_t f = fbase[c / NCN_MESH_SCAN_ELEMS] + (int64_t)flocal[c];
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const int corner[4] = {0, TET_V1[t], TET_V2[t], 7};
        const int bits = (in8 & 1) | (((in8 >> corner[1]) & 1) << 1) | (((in8 >> corner[2]) & 1) << 2) | (((in8 >> 7) & 1) << 3);
        const uint32_t w = TET_CASES[bits];
        const int n = (int)(w >> 24);
        for (int q = 0; q < n; q++) {
            int64_t tri[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int e = (w >> (4 * (3 * q + r))) & 15, a = corner[e >> 2], b = corner[e & 3];
                tri[r] = vertex_number(mask, vlocal, vbase, p000 + (a & 1) + ((a >> 1) & 1) * sx + (a >> 2) * sx * sy, b - a);
            }
            if (TET_SIGN[t] < 0) {
                const int64_t s = tri[1];
                tri[1] = tri[2], tri[2] = s;
            }
            if (f >= 0 && f < n_faces) faces[3 * f] = tri[0], faces[3 * f + 1] = tri[1], faces[3 * f + 2] = tri[2];
            f++;
        }
    }
}

}  // namespace ncn

using namespace ncn;

// the checks every entry point shares; the products stay far inside int64 (and the grids inside 2^31 blocks)
static int check_lattice(const char* name, int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z,
                         float hi_x, float hi_y, float hi_z, const uint8_t* bitfield, int grid_size, float scale) {
    NCN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, hipErrorInvalidValue, "%s: res (%lld, %lld, %lld) must be >= 1 per axis",
                name, (long long)nx, (long long)ny, (long long)nz);
    NCN_REQUIRE(nx < (1 << 20) && ny < (1 << 20) && nz < (1 << 20) &&
                    (double)(nx + 1) * (double)(ny + 1) * (double)(nz + 1) < 2.0e11,
                hipErrorInvalidValue, "%s: res (%lld, %lld, %lld) is too large", name, (long long)nx, (long long)ny,
                (long long)nz);
    NCN_REQUIRE(lo_x < hi_x && lo_y < hi_y && lo_z < hi_z && std::isfinite(hi_x - lo_x) && std::isfinite(hi_y - lo_y) &&
                    std::isfinite(hi_z - lo_z),
                hipErrorInvalidValue, "%s: the box needs finite lo < hi on every axis", name);
    if (bitfield != nullptr) {
        NCN_REQUIRE(grid_size >= 2 && grid_size <= 1024 && (grid_size & (grid_size - 1)) == 0, hipErrorInvalidValue,
                    "%s: grid_size %d must be a power of two in [2, 1024]", name, grid_size);
        NCN_REQUIRE(scale > 0.0f && std::isfinite(scale), hipErrorInvalidValue, "%s: scale must be positive", name);
    }
    return 0;
}

extern "C" {

int ncn_mesh_points(int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y,
                    float hi_z, int64_t p0, int64_t n, const uint8_t* bitfield, int grid_size, float scale, float* xyz,
                    int64_t* idx, int32_t* count, void* stream) {
    if (int rc = check_lattice("ncn_mesh_points", nx, ny, nz, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, bitfield, grid_size, scale))
        return rc;
    const int64_t P = (nx + 1) * (ny + 1) * (nz + 1);
    NCN_REQUIRE(p0 >= 0 && n >= 0 && p0 + n <= P && n <= INT32_MAX, hipErrorInvalidValue,
                "ncn_mesh_points: [p0, p0 + n) = [%lld, %lld) must lie in [0, %lld) with n < 2^31", (long long)p0,
                (long long)(p0 + n), (long long)P);
    NCN_REQUIRE(xyz != nullptr && (bitfield == nullptr || (idx != nullptr && count != nullptr)), hipErrorInvalidValue,
                "ncn_mesh_points: xyz (and, with a bitfield, idx and count) must not be NULL");
    if (n == 0) return 0;
    const Lattice L = make_lattice(nx, ny, nz, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, bitfield, grid_size, scale);
    hipLaunchKernelGGL(mesh_points_kernel, dim3((unsigned)cdiv(n, MESH_THREADS)), dim3(MESH_THREADS), 0,
                       (hipStream_t)stream, L, p0, n, xyz, idx, count);
    NCN_LAUNCH_CHECK("ncn_mesh_points");
    return 0;
}

int ncn_mesh_count(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z,
                   float hi_x, float hi_y, float hi_z, float iso, const uint8_t* bitfield, int grid_size, float scale,
                   uint8_t* mask, uint8_t* nfaces, void* stream) {
    if (int rc = check_lattice("ncn_mesh_count", nx, ny, nz, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, bitfield, grid_size, scale))
        return rc;
    NCN_REQUIRE(sigma != nullptr && mask != nullptr && nfaces != nullptr, hipErrorInvalidValue,
                "ncn_mesh_count: sigma, mask and nfaces must not be NULL");
    NCN_REQUIRE(std::isfinite(iso), hipErrorInvalidValue, "ncn_mesh_count: iso must be finite");
    const int64_t gy = cdiv(ny + 1, MT_Y), gz = cdiv(nz + 1, MT_Z);
    NCN_REQUIRE(gy <= 65535 && gz <= 65535, hipErrorInvalidValue, "ncn_mesh_count: res (.., %lld, %lld) needs more than 65535 tiles",
                (long long)ny, (long long)nz);
    const Lattice L = make_lattice(nx, ny, nz, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, bitfield, grid_size, scale);
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)cdiv(nx + 1, MT_X), (unsigned)gy, (unsigned)gz), dim3(MESH_THREADS), 0,
                       (hipStream_t)stream, L, sigma, iso, mask, nfaces);
    NCN_LAUNCH_CHECK("ncn_mesh_count");
    return 0;
}

int ncn_mesh_scan(const uint8_t* in, int64_t n, int popcount, uint16_t* local, int64_t* block_base, int64_t* total,
                  void* stream) {
    NCN_REQUIRE(n >= 1 && n < ((int64_t)1 << 42), hipErrorInvalidValue, "ncn_mesh_scan: n = %lld out of range", (long long)n);
    NCN_REQUIRE(in != nullptr && local != nullptr && block_base != nullptr && total != nullptr, hipErrorInvalidValue,
                "ncn_mesh_scan: in, local, block_base and total must not be NULL");
    NCN_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)local & 15) == 0, hipErrorInvalidValue,
                "ncn_mesh_scan: in and local must be 16-byte aligned");
    const int64_t nb = cdiv(n, NCN_MESH_SCAN_ELEMS);
    hipLaunchKernelGGL(mesh_scan_local_kernel, dim3((unsigned)nb), dim3(MESH_THREADS), 0, (hipStream_t)stream, in, n,
                       popcount ? 1 : 0, local, block_base);
    NCN_LAUNCH_CHECK("ncn_mesh_scan");
    hipLaunchKernelGGL(mesh_scan_base_kernel, dim3(1), dim3(NCN_MESH_SCAN_SWEEP), 0, (hipStream_t)stream, block_base, nb, total);
    NCN_LAUNCH_CHECK("ncn_mesh_scan");
    return 0;
}

int ncn_mesh_emit_verts(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z,
                        float hi_x, float hi_y, float hi_z, float iso, const uint8_t* mask, const uint16_t* vlocal,
                        const int64_t* vbase, float* verts, int64_t n_verts, void* stream) {
    if (int rc = check_lattice("ncn_mesh_emit_verts", nx, ny, nz, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, nullptr, 0, 0.0f))
        return rc;
    NCN_REQUIRE(sigma != nullptr && mask != nullptr && vlocal != nullptr && vbase != nullptr && n_verts >= 0 &&
                    (verts != nullptr || n_verts == 0),
                hipErrorInvalidValue, "ncn_mesh_emit_verts: NULL argument or n_verts < 0");
    if (n_verts == 0) return 0;
    const Lattice L = make_lattice(nx, ny, nz, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, nullptr, 0, 0.0f);
    const int64_t P = (nx + 1) * (ny + 1) * (nz + 1);
    hipLaunchKernelGGL(mesh_emit_verts_kernel, dim3((unsigned)cdiv(P, MESH_THREADS)), dim3(MESH_THREADS), 0,
                       (hipStream_t)stream, L, sigma, iso, mask, vlocal, vbase, verts, n_verts);
    NCN_LAUNCH_CHECK("ncn_mesh_emit_verts");
    return 0;
}

int ncn_mesh_emit_faces(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float iso, const uint8_t* mask,
                        const uint16_t* vlocal, const int64_t* vbase, const uint8_t* nfaces, const uint16_t* flocal,
                        const int64_t* fbase, int64_t* faces, int64_t n_faces, void* stream) {
    if (int rc = check_lattice("ncn_mesh_emit_faces", nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, nullptr, 0, 0.0f))
        return rc;
    NCN_REQUIRE(sigma != nullptr && mask != nullptr && vlocal != nullptr && vbase != nullptr && nfaces != nullptr &&
                    flocal != nullptr && fbase != nullptr && n_faces >= 0 && (faces != nullptr || n_faces == 0),
                hipErrorInvalidValue, "ncn_mesh_emit_faces: NULL argument or n_faces < 0");
    if (n_faces == 0) return 0;
    const int64_t C = nx * ny * nz;
    hipLaunchKernelGGL(mesh_emit_faces_kernel, dim3((unsigned)cdiv(C, MESH_THREADS)), dim3(MESH_THREADS), 0,
                       (hipStream_t)stream, nx, ny, nz, sigma, iso, mask, vlocal, vbase, nfaces, flocal, fbase, faces, n_faces);
    NCN_LAUNCH_CHECK("ncn_mesh_emit_faces");
    return 0;
}

}  // extern "C"
