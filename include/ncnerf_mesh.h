/*
 * ncnerf_mesh.h — isosurface extraction of libncnerf.so: an indexed triangle mesh of {sigma = iso} from
 * a lattice of densities.  A fourth header beside ncnerf.h, ncnerf_metrics.h and ncnerf_geom.h, in the
 * same grammar and under the same rules (ncnerf.h, top): plain device pointers, `void* stream` last,
 * nothing allocated, nothing synchronised, 0 or a hipError_t returned.  THIS FILE IS PARSED by
 * ncnerf_amd/_lib.py exactly as ncnerf.h is, into a table of its own; every entry point returns int.
 * The reference has no counterpart: the definition below is the contract (tests/mesh_ref.py restates
 * it in NumPy, independently).
 *
 * LATTICE.  res = (nx, ny, nz) cells over the box [lo, hi]; (nx+1)(ny+1)(nz+1) points, linear index
 *   p = (iz (ny+1) + iy)(nx+1) + ix   (int64 throughout), sigma is the (nz+1, ny+1, nx+1) f32 array.
 *   Position per axis: lo + (float)i * h with h = (hi - lo) / (float)n, plain fp32, no contraction
 *   (one rounding per operation: NumPy float32 reproduces it bit for bit).
 *   Cells: c = (iz ny + iy) nx + ix.
 * INSIDE.  A point is inside when sigma >= iso: a NaN is outside, +Inf is inside.
 * CELLS.  Every cell is cut into the six tetrahedra of the Kuhn (Freudenthal) split, one per
 *   permutation (a, b, c) of the axes (x = 0, y = 1, z = 2), in lexicographic order of the permutation:
 *   xyz, xzy, yxz, yzx, zxy, zyx.  With corners named by their offset bits (dx + 2 dy + 4 dz) the
 *   tetrahedron's corners are, in path order, v0 = 0, v1 = 1<<a, v2 = v1 | 1<<b, v3 = 7: all six share
 *   the body diagonal.  Its sign s is the permutation's (+1 for xyz, yzx, zxy).  The split is the same
 *   in every cell, so neighbouring cells agree on every face diagonal and the surface is watertight.
 * EDGES.  The edges of the split have the seven directions d = dx + 2 dy + 4 dz in 1..7 (three axis
 *   edges, three face diagonals, the body diagonal); an edge is owned by its lower endpoint and has
 *   kind k = d - 1, bit k of the owner's mask.  An owned edge whose endpoints differ in the inside
 *   test (and, under occupancy culling, that lies in at least one active cell) carries exactly one
 *   vertex, pa + t (pb - pa) per axis with t = (iso - sa) / (sb - sa), a the owner; again no
 *   contraction.  If sa or sb is not finite, t = 0.5.
 * VERTICES are numbered by an exclusive scan over (owner point index, kind): the vertex array is a
 *   function of the input alone.  The number of edge (p, k) is
 *   vbase[p / NCN_MESH_SCAN_ELEMS] + vlocal[p] + popcount(mask[p] & ((1 << k) - 1)).
 * FACES are emitted per cell in cell order, per tetrahedron in the order above.  E(i, j) (i < j in
 *   path order) is the vertex on the edge v_i v_j: owner = the cell's origin + v_i, d = v_j - v_i.
 *     one corner i inside, (j, k, l) the others ascending:   T = (E(i,j), E(i,k), E(i,l))
 *     one corner i outside, (j, k, l) the others ascending:  the same T
 *     i < j inside, k < l outside:  Q = (E(i,k), E(i,l), E(j,l), E(j,k)), cut into
 *                                   (Q0, Q1, Q2) and (Q0, Q2, Q3)
 *   (E(i,j) with i > j means E(j,i)).  Let o = s * sign of the permutation (i, j, k, l) of (0, 1, 2, 3),
 *   negated in the one-corner-outside case.  If o < 0 the last two vertices of every triangle are
 *   swapped.  Every triangle then has its normal toward lower density.  Degenerate triangles (t = 0
 *   on several edges of one point) are kept.  Faces are numbered by an exclusive scan of the
 *   per-cell counts (0..12): face f of cell c is fbase[c / NCN_MESH_SCAN_ELEMS] + flocal[c] + f.
 * OCCUPANCY CULLING (bitfield != NULL).  A cell is active when the occupancy cell that contains its
 *   centre lo + ((float)i + 0.5f) * h is set in the bitfield, by the marcher's own lookup at cascade
 *   0: n = (int)clamp(0.5 * fma(x, 1 / b, 1) * G, 0, G - 1) per axis with b = min(0.5, scale), bit
 *   morton3D(nx, ny, nz).  Inactive cells emit no face, an edge that lies in no active cell carries
 *   no vertex, and a point with no active incident cell is not listed by ncn_mesh_points.  Without a
 *   bitfield every cell is active.
 *
 * Order of calls: ncn_mesh_count; ncn_mesh_scan twice (mask with popcount = 1, nfaces with popcount
 * = 0), which leave V and F in a device buffer; a host read of them; ncn_mesh_emit_verts and
 * ncn_mesh_emit_faces into buffers of exactly that size.  No sum is atomic: two calls on the same
 * inputs give the same bits.  Buffer sizes (P points, C cells, B(n) = ceil(n / NCN_MESH_SCAN_ELEMS)):
 *   mask (P) u8, nfaces (C) u8, vlocal (P) u16, flocal (C) u16, vbase (B(P)) i64, fbase (B(C)) i64.
 */
#ifndef NCNERF_MESH_H
#define NCNERF_MESH_H
#include <stdint.h>

/* points per workgroup of ncn_mesh_count: a tile of TILE_X x TILE_Y x TILE_Z plus its halo in LDS */
#define NCN_MESH_TILE_X 32
#define NCN_MESH_TILE_Y 8
#define NCN_MESH_TILE_Z 8
/* elements per workgroup of ncn_mesh_scan (the block of vbase / fbase) */
#define NCN_MESH_SCAN_ELEMS 4096
/* most block sums ncn_mesh_scan's second pass takes per sweep of its one workgroup */
#define NCN_MESH_SCAN_SWEEP 1024

#ifdef __cplusplus
extern "C" {
#endif

/* ---- positions of the lattice points [p0, p0 + n).  bitfield NULL: xyz (n, 3) = every position in
 *      order; idx and count are not touched (may be NULL).  With a bitfield (grid_size^3 / 8 bytes of
 *      cascade 0, `scale` the model's): only the points with at least one active incident cell,
 *      compacted in no particular order: xyz (<= n, 3), idx (<= n) their point indices, count (1)
 *      their number, which THE CALLER ZEROES before the launch. ---- */
int ncn_mesh_points(int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y,
                    float hi_z, int64_t p0, int64_t n, const uint8_t* bitfield, int grid_size, float scale, float* xyz,
                    int64_t* idx, int32_t* count, void* stream);

/* ---- per point the 7-bit mask of its owned edges that carry a vertex (mask, P bytes), per cell the
 *      number of faces (nfaces, C bytes, 0..12); every element of both is written. ---- */
int ncn_mesh_count(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z,
                   float hi_x, float hi_y, float hi_z, float iso, const uint8_t* bitfield, int grid_size, float scale,
                   uint8_t* mask, uint8_t* nfaces, void* stream);

/* ---- ordered exclusive scan of v[i] = in[i] (popcount = 0) or popcount(in[i]) (popcount = 1), v <= 15:
 *      local[i] = the sum of v over the elements of i's block before i, block_base[b] = the sum over
 *      all blocks before b (int64), total[0] = the sum of everything.  Two launches. ---- */
int ncn_mesh_scan(const uint8_t* in, int64_t n, int popcount, uint16_t* local, int64_t* block_base, int64_t* total,
                  void* stream);

/* ---- verts (n_verts, 3): every vertex, at its number.  n_verts is the scan's total; a number
 *      outside [0, n_verts) is never written. ---- */
int ncn_mesh_emit_verts(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float lo_x, float lo_y, float lo_z,
                        float hi_x, float hi_y, float hi_z, float iso, const uint8_t* mask, const uint16_t* vlocal,
                        const int64_t* vbase, float* verts, int64_t n_verts, void* stream);

/* ---- faces (n_faces, 3) int64 vertex numbers: every face, at its number.  n_faces is the scan's
 *      total; a number outside [0, n_faces) is never written. ---- */
int ncn_mesh_emit_faces(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float iso, const uint8_t* mask,
                        const uint16_t* vlocal, const int64_t* vbase, const uint8_t* nfaces, const uint16_t* flocal,
                        const int64_t* fbase, int64_t* faces, int64_t n_faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif
