/*
 * gsr_chunker.h -- C ABI of the scene partition: which cameras train a chunk, which sparse points seed
 * it, which 2-D observations each image keeps and which depth-only views belong to it, for every chunk
 * of the grid at once.  Exported by libgsr_hip.so.
 *
 * Replaces make_chunk and the grid set-up of the reference's chunker (preprocess/ss_make_chunk.py:441-643,
 * 671-747) from the decoded COLMAP model on.  The reference script cannot be run beside this project
 * (it imports laspy, open3d, trimesh, cv2 and joblib), so the rule below is this project's own
 * statement of what it does: parity with it is unpinned.
 *
 * Grid (host, gs_train/chunker.py chunk_grid, the reference's dtypes :675-736).  cam_centers (M, 3) fp32,
 * -R.astype(f32).T @ t.astype(f32); global_bbox stays fp32 through the padding and the % arithmetic;
 * n_w = round(extent_x / cs), n_h likewise; cell (i, j) has the linear index i n_h + j (the reference's
 * loop order).  Bounds are fp64, one rounded product and one rounded sum each:
 *   bx(i) = (double)x0 + (double)i * cs,  x0 = global_bbox[0, 0];  by(j) likewise with y0
 * The upper bound of cell i is bx(i + 1), not bx(i) + cs.
 *
 * Boxes (every test a strict < in fp64; NaN fails):
 *   box(i, j):   bx(i) < x < bx(i + 1), by(j) < y < by(j + 1), -1e12 < z < 1e12
 *   pbox(i, j):  the same, but the lower x bound is -1e12 when i == 0 and the upper one 1e12 when
 *                i == n_w - 1; y likewise (+-1e12, not +-infinity)
 *   ebox(i, j):  per axis, with lo / hi of box: c = (lo + hi) / 2, h = (hi - lo) / 2, bounds c - 2 h
 *                and c + 2 h in that operation order (z: +-2e12)
 * The grid must lie inside the extension: -1e12 < bx(0), bx(n_w) < 1e12, and the same on y.
 *
 * Points: point_id (N) int64, unique, >= 0; point_xyz (N, 3) fp64; point_error (N) fp32.
 *   C        = the rows with error < 10 (fp32, strict; NaN is out)
 *   cell32(r), r in C = the cell whose pbox holds (float)xyz widened back to fp64, or -1
 *   cell64(r), every r = the same with the fp64 xyz itself
 * The two differ for a point within fp32 rounding of a bound: the reference takes a chunk's points and
 * its cameras' counts from fp32 positions (:462, 483) and the observation filter from the file's
 * doubles (:539-542).
 *
 * Observations: obs_ptr (M + 1) int64, obs_point_id (O) int64, -1: none.  For observation o of camera m
 * with id q:
 *   inC(o)  = the row r of C with id == q, if there is one
 *   vis(o)  = inC(o) exists and the fp32 position of r is not exactly (0, 0, 0)    (:705-717; q < L,
 *             L = 1 + the largest id in C, follows from inC)
 *   total[m] = sum of vis;  n_pts[m][cell] = sum of vis with cell32(r) == cell
 *   blend[m][cell] = sum of "inC(o) exists" with cell32(r) == cell   (np.isin, :560: the origin counts)
 *   keep(o, cell) = q >= 0, some row r (in C or not) has id == q, and cell64(r) == cell
 * Duplicate observations of one point count each time.
 *
 * Cameras, per (m, cell): IN if the centre is in box(cell); else NEAR if it is in ebox(cell) and
 * n_pts > 20; else DRAW if n_pts > 10 and add_far_cams.  (A near camera with 11..20 points is a DRAW.)
 * The host resolves the DRAW states and the camera limits with Python's random (gs_train/chunker.py).
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, `stream` a hipStream_t, rows and
 * cells int32.  N, M, O, D, P = 0 are valid and launch nothing.
 */
#ifndef GSR_CHUNKER_H
#define GSR_CHUNKER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* x0, y0: global_bbox[0, :2] widened; cs: chunk_size.  1 <= n_w, n_h, n_w n_h < 2^31. */
typedef struct gsr_chunk_grid {
    double x0, y0, cs;
    int32_t n_w, n_h;
} gsr_chunk_grid;

#define GSR_CHUNK_NOT_IN_C (-2) /* cell32 of a row outside C */
#define GSR_CHUNK_IN 1
#define GSR_CHUNK_NEAR 2
#define GSR_CHUNK_DRAW 3

/* cell32[r] (GSR_CHUNK_NOT_IN_C for a row outside C, -1 for a row of C in no pbox) and cell64[r], one
 * streaming pass over xyz (N, 3) fp64 and error (N) fp32.  grid: host.  0 <= N < 2^31. */
int gsr_chunk_classify_points(int64_t N, const double *xyz, const float *error, const gsr_chunk_grid *grid,
                              int32_t *cell32, int32_t *cell64, void *stream);

/* cam_cell[m] / depth_cell[d]: the cell whose box (not pbox) holds the centre, or -1.  cam_centers (M, 3)
 * fp32 (widened), depth_centers (D, 3) fp64.  One launch over M + D. */
int gsr_chunk_classify_centers(int64_t M, const float *cam_centers, int64_t D, const double *depth_centers,
                               const gsr_chunk_grid *grid, int32_t *cam_cell, int32_t *depth_cell, void *stream);

/* min_max (host, 2 x int64): the smallest and the largest of ids (N); (0, -1) for N = 0.  Synchronises. */
int gsr_chunk_id_range(int64_t N, const int64_t *ids, int64_t *min_max, void *stream);

/* table[id] = the row with that id, -1 where there is none; T = the largest id + 1 entries.
 * GSR_ERR_INVALID_ARGUMENT: an id < 0 or >= T, T > 2^31 - 1, two rows with one id.  Synchronises. */
int gsr_chunk_id_table(int64_t N, const int64_t *ids, int64_t T, int32_t *table, void *stream);

/* n_pts, blend (M, cells) int32 and total (M) int32, zeroed here.  One wave per camera over
 * obs_point_id[obs_ptr[m] .. obs_ptr[m + 1]); the lanes that share a cell issue one add of their
 * popcount.  cell32 as gsr_chunk_classify_points wrote it.  M cells < 2^31.  obs_ptr must ascend from 0
 * to O (a range reaching outside [0, O) is cut to it). */
int gsr_chunk_camera_counts(int64_t M, const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T,
                            const int32_t *table, const int32_t *cell32, const double *xyz, int64_t cells,
                            int32_t *n_pts, int32_t *blend, int32_t *total, void *stream);

/* The (cell, m) pairs with a state, in ascending (cell, m) order.  _count writes *count (host) after
 * one ballot per wave and a scan, and synchronises; _write, given the same arguments and scratch,
 * writes out (count, 5) int32: cell, m, state, n_pts, total.  scratch: gsr_chunk_candidates_scratch_bytes(M cells). */
size_t gsr_chunk_candidates_scratch_bytes(int64_t n);
int gsr_chunk_candidates_count(int64_t M, const float *cam_centers, const int32_t *cam_cell, const int32_t *n_pts,
                               const gsr_chunk_grid *grid, int add_far_cams, void *scratch, int64_t *count, void *stream);
int gsr_chunk_candidates_write(int64_t M, const float *cam_centers, const int32_t *cam_cell, const int32_t *n_pts,
                               const int32_t *total, const gsr_chunk_grid *grid, int add_far_cams, const void *scratch,
                               int32_t *out, void *stream);

/* The observation filter for P (cell, camera) pairs: _count writes offsets (P + 1) int64, the exclusive
 * sum of the pairs' kept observations, and *n_kept (host), and synchronises; _write writes
 * out_index[offsets[p] .. offsets[p + 1]): the kept observations of pair p as indices into obs_point_id,
 * ascending.  One wave per pair.  scratch: gsr_chunk_obs_filter_scratch_bytes(P). */
size_t gsr_chunk_obs_filter_scratch_bytes(int64_t P);
int gsr_chunk_obs_filter_count(int64_t P, const int32_t *pair_cell, const int32_t *pair_cam, int64_t M,
                               const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T,
                               const int32_t *table, const int32_t *cell64, void *scratch, int64_t *offsets,
                               int64_t *n_kept, void *stream);
int gsr_chunk_obs_filter_write(int64_t P, const int32_t *pair_cell, const int32_t *pair_cam, int64_t M,
                               const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T,
                               const int32_t *table, const int32_t *cell64, const int64_t *offsets, int64_t *out_index,
                               void *stream);

/* The rows with cell32 >= 0 by cell, input order within a cell (a stable sort on the cell):
 * out_rows[out_offsets[c] .. out_offsets[c + 1]) are cell c's rows; out_rows (N) int32, out_offsets
 * (cells + 1) int64.  0 <= N < 2^31, 1 <= cells < 2^31. */
size_t gsr_chunk_points_by_cell_scratch_bytes(int64_t N, int64_t cells);
int gsr_chunk_points_by_cell(int64_t N, const int32_t *cell32, int64_t cells, void *scratch, int32_t *out_rows,
                             int64_t *out_offsets, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_CHUNKER_H */
