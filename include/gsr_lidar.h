/*
 * gsr_lidar.h -- C ABI of a chunk's LiDAR cloud preparation: the crop to the chunk's box, the filter
 * "within max_distance of the reconstructed mesh" and the voxel mean that makes the initial points.
 * Exported by libgsr_hip.so.
 *
 * Replaces process_lidar_points of the reference's chunker (preprocess/ss_make_chunk.py:36-305): the
 * crop (:105-114), filter_points_by_mesh_distance (:157-235, an Open3D raycasting scene on the host)
 * and downsample_for_max_density (:70-74, Open3D's voxel_down_sample).  LAZ decoding and the tile
 * selection (:237-270) stay with the caller.  Neither Open3D nor embree can be run beside this
 * project, so the rule below is this project's own statement of what they document.
 *
 * Crop (fp32, on the fp32 bounds x_lo, x_hi, y_lo, y_hi = c -+ e/2 the caller formed in fp32):
 *   in_box = x_lo < x && x < x_hi && y_lo < y && y < y_hi          strict; no z test; NaN fails
 *
 * Mesh filter.  A point p is kept when the Euclidean distance from p to the closest point of some
 * closed triangle (v0, v1, v2) is <= max_distance; a zero-area triangle is the segment or the point
 * it covers.  A point with a NaN or Inf coordinate is dropped.  The kernel decides it in fp32 on
 * differences formed first, a = v0 - p, b = v1 - p, c = v2 - p (p is the origin from here on), so
 * the arithmetic runs at the scale of the triangle, not of the map coordinates:
 *   sep   = on some axis k: min(a_k, b_k, c_k) >= reach or max(a_k, b_k, c_k) <= -reach
 *   seg(u, w)  = |u + t (w - u)|^2, t = clamp(-(u . e) / (e . e), 0, 1), e = w - u   (t = 0 if e . e = 0)
 *   n     = (b - a) x (c - a), each component x y - z w as fma(x, y, -rn(z w)) + fma(-z, w, rn(z w))
 *   inside = n.(b x c) >= 0 && n.(c x a) >= 0 && n.(a x b) >= 0
 *   d2    = min(seg(a, b), seg(b, c), seg(a, c), inside && n.n > 0 ? (n . a)^2 / (n . n) : +Inf)
 *   near  = !sep && d2 <= T
 * with T the largest fp32 <= max_distance^2 and reach an fp32 >= max_distance (1 + 2^-20), every
 * operation rounded to fp32, no contraction but the two fused operations of n (they keep a needle's
 * normal, a difference of products that cancels, to a few ulp).  sep never rejects a triangle within
 * max_distance (a separated triangle is farther than reach (1 - 2^-24) > max_distance); it is what
 * makes the grid exact.  fp32 and real arithmetic can differ only for points whose distance is
 * within rounding of max_distance.
 *
 * Voxel mean (Open3D's documented voxel_down_sample, in fp64).  With lo the per-axis minimum of the
 * kept points and s = voxel_size, a point p (widened to fp64) falls in voxel
 * floor((p - (lo - s/2)) / s) per axis.  The output is, per occupied voxel in ascending (iz, iy, ix)
 * order, the fp64 mean of its positions and colours rounded to fp32, and its count.  The sums run in
 * a fixed order (input order within a voxel; a fixed tree for long voxels): two runs on the same
 * input are bitwise equal.
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, fp32, `stream` a hipStream_t.
 */
#ifndef GSR_LIDAR_H
#define GSR_LIDAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_mesh_index gsr_mesh_index;

/* Build the index over a triangle mesh: vertices (V, 3) contiguous fp32, finite; faces (F, 3) int32
 * with 0 <= index < V; 1 <= V, 1 <= F < 2^31, for queries around max_distance (a finite double > 0 with
 * max_distance^2 an fp32 normal).  A uniform grid of the occupied cells only: every triangle is listed
 * (as its three vertices, 36 B) in each cell its bounding box grown by the reach touches; a triangle
 * whose grown box covers more than 512 cells goes to an oversize list every query tests.  Allocates
 * device memory of its own (build scratch is freed before it returns) and synchronises `stream`.
 * NULL on failure (gsr_last_error): a non-finite vertex, a face index out of range, more than
 * 2^31 - 1 references. */
gsr_mesh_index *gsr_mesh_index_create(int64_t V, const float *vertices, int64_t F, const int32_t *faces,
                                      double max_distance, void *stream);
void gsr_mesh_index_destroy(gsr_mesh_index *index);

/* info (host, up to n of 9 x int64): V, F, occupied cells, references stored (oversize ones not
 * counted), oversize triangles, device bytes held, cells along x, y, z. */
int gsr_mesh_index_info(const gsr_mesh_index *index, int64_t *info, int n);

/* out_mask[i] = in_box(p_i) && finite(p_i) && near(p_i, some triangle), one byte per point of xyz (P, 3).
 * box (host, 4 floats x_lo, x_hi, y_lo, y_hi) or NULL: no crop.  index NULL: no mesh filter
 * (out_mask[i] = in_box && finite).  max_distance may differ from the one the index was built for:
 * the result is exact for any (the searched cell range grows with it). */
int gsr_mesh_near_mask(int64_t P, const float *xyz, const gsr_mesh_index *index, double max_distance,
                       const float *box, uint8_t *out_mask, void *stream);

/* Scratch of gsr_voxel_mean for P points (0 for P < 1 or P >= 2^31). */
size_t gsr_voxel_mean_scratch_bytes(int64_t P);

/* The voxel mean of the points with keep_mask[i] != 0 (keep_mask: P bytes, or NULL: all).  colors
 * (P, 3) or NULL (out_colors is then not written).  out_xyz / out_colors (P, 3) and out_count (P) int32
 * have room for P voxels; *n_out (host) is the number written.  Kept points must be finite, and
 * voxel_size a finite double > 0 for which no axis needs more than 2^31 - 1 voxels and the three
 * axes' index bits fit a 63-bit key (GSR_ERR_INVALID_ARGUMENT otherwise).  Synchronises `stream`. */
int gsr_voxel_mean(int64_t P, const float *xyz, const float *colors, const uint8_t *keep_mask, double voxel_size,
                   void *scratch, float *out_xyz, float *out_colors, int32_t *out_count, int64_t *n_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_LIDAR_H */
