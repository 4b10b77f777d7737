/*
 * gsr_gtcloud.h -- C ABI of the ground-truth point cloud constraint of densification
 * (gt_point_cloud_constraints).  Exported by libgsr_hip.so.
 *
 * Replaces GaussianModel.load_gt_point_cloud (scene/gaussian_model.py:796-851: a FAISS flat L2 index
 * and the cloud's XY bounds) and compare_points_to_gt (:853-962: every Gaussian inside the XY bounds
 * whose nearest cloud point is farther than constraint_treshold is pruned), as
 * densify_and_prune(..., True) uses them (:757-758).
 *
 * For a row with position p and a cloud of G points g, all fp32:
 *
 *   inside  = p.x >= x_min && p.x <= x_max && p.y >= y_min && p.y <= y_max     (no z test; a NaN or
 *             Inf x or y fails it)
 *   d2(p,g) = (dx*dx + dy*dy) + dz*dz,  d = g - p, every operation rounded to fp32, no contraction
 *   D       = inside && for every g: (double)d2(p,g) > thr*thr                  (thr a double)
 *
 * x_min .. y_max are the fp32 minimum and maximum of the cloud's x and y.  The comparison is made
 * against the largest fp32 not above thr*thr, which decides the same.  D is "no cloud point within
 * thr": no distance is output.  A NaN z gives D = 0 (no comparison with NaN holds), an infinite z
 * gives D = 1 when inside (every d2 is +Inf).
 *
 * The index is a uniform grid over the cloud (cell edge >= the thr it was built for): the points as
 * float4 in cell order and a sorted table of the occupied cells, 16 B per point + 12 B per occupied
 * cell.  Queries with another thr are exact too (the searched cell range follows thr), only slower
 * when thr is much larger than the cell.
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, fp32, `stream` a hipStream_t.
 */
#ifndef GSR_GTCLOUD_H
#define GSR_GTCLOUD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_gt_index gsr_gt_index;

/* Build the index over points (G, 3) contiguous fp32, finite, 1 <= G < 2^31, for thresholds around
 * thr.  Allocates device memory of its own (build scratch is freed before it returns) and
 * synchronises `stream`.  NULL on failure (gsr_last_error). */
gsr_gt_index *gsr_gt_index_create(int64_t G, const float *points, double thr, void *stream);
void gsr_gt_index_destroy(gsr_gt_index *index);

/* bounds (host, 4 floats): x_min, x_max, y_min, y_max. */
int gsr_gt_index_bounds(const gsr_gt_index *index, float *bounds);

/* info (host, up to n of 6 x int64): G, occupied cells, device bytes held, cells along x, y, z. */
int gsr_gt_index_info(const gsr_gt_index *index, int64_t *info, int n);

/* compare_points_to_gt's distance mask: out_mask[i] = D_i of xyz (P, 3) for rows with skip[i] == 0
 * (skip: P bytes or NULL), 0 for the others. */
int gsr_gt_far_mask(int64_t P, const float *xyz, const gsr_gt_index *index, double thr, const uint8_t *skip,
                    uint8_t *out_mask, void *stream);

/* gsr_densify_plan (gsr_densify.h; same scratch, then gsr_densify_apply as usual) with the distance
 * prune: D_i is evaluated on the rows with !S_i && !Z_i, rows below first_row included, and the
 * output rows are
 *   [old rows i with !S_i && !Z_i && !D_i] [clones of C_i && !Z_i && !D_i] [children set 1] [set 2]
 * (children of S_i && !Z_i, never distance-tested; n_split still counts every S_i).
 * counts (device, 6 x int64): {old rows kept, clones kept, n_split, total output rows, rows removed
 * by D (old rows + clones), of those the old rows below first_row}. */
int gsr_densify_plan_gt(int64_t P0, int64_t first_row, const float *grad_accum, const float *max_radii2D,
                        const float *opacity_raw, const float *scaling_raw, const float *xyz, float max_grad,
                        float min_opacity, float max_scale, const gsr_gt_index *index, double thr, void *scratch,
                        int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_GTCLOUD_H */
