/*
 * gsr_model_init.h -- C ABI of the model construction from a point cloud and of the scaffold
 * selection in front of a chunk.  Exported by libgsr_hip.so.  New entry
 * points only: GSR_ABI_VERSION stays.
 *
 *   gsr_model_init_cloud     restates GaussianModel.create_from_pcd up to the parameters
 *                            (scene/gaussian_model.py:163-222): the cloud's bounding box, the skybox
 *                            rows, the kNN scales, the opacities and the SH DC term.
 *   gsr_scaffold_merge_*     restate :224-264: the scaffold rows inside the ring around the chunk
 *                            (and the scaffold's skybox), SH padded, in front of the chunk's rows.
 *
 * Output rows are [skybox | cloud] resp. [selected scaffold rows | chunk rows] in the joined layout
 * the train step uses: xyz (P,3), features (P,M,3), opacity_raw (P,1), scaling_raw (P,3),
 * rotation (P,4).
 *
 * gsr_model_init_cloud, all fp32 unless said otherwise, no contraction:
 *
 *   min, max   per-axis minimum and maximum of the N cloud points
 *   mean       0.5 * (min + max)
 *   radius     sqrt((dx*dx + dy*dy) + dz*dz), d = max - mean
 *   skybox row r < S (skybox mode):
 *     dir      (cos(2 pi u_theta[r]) sin(phi), sin(2 pi u_theta[r]) sin(phi), cos(phi)) with
 *              cos(phi) = 1 - 1.4 u_phi[r], sin(phi) = sqrt(1 - cos(phi)^2), evaluated in fp64 and
 *              rounded once to fp32 per component (u_phi = 0 gives (0, 0, 1) exactly)
 *     xyz      mean + (10 * radius) * dir           (two fp32 operations per component)
 *     rgb      (0.7, 0.8, 0.95)
 *   cloud row: xyz and rgb copied
 *   dist2      gsr_knn_mean_dist2 over all S + N rows (gsr_knn.h)
 *   d          max(dist2, 1e-7);  skybox mode: skybox rows d * 10, cloud rows min(d, 10)
 *   scaling    log(sqrt(d)) three times;  rotation (1, 0, 0, 0)
 *   opacity    skybox mode: cloud rows logit(0.02), skybox rows the raw value 0.7 (the reference
 *              assigns it in logit space, :217);  plain mode: logit(0.01).  The logits are
 *              evaluated in fp64 and rounded once.
 *   features   coefficient 0 = (rgb - 0.5) / 0.28209479177387814f (a division); the others 0
 *
 * A NaN or Inf cloud coordinate fails the call with GSR_ERR_INVALID_ARGUMENT naming the first such
 * point, before any output is written (torch would carry it into every skybox row).
 *
 * gsr_scaffold_merge_count, row r of the Ps scaffold rows is selected iff
 *
 *   r < S  ||  (m > 0.5f * extent[0]  &&  m < 1.5f * extent[0]),   m = max(|x - cx|, |y - cy|)
 *
 * every operation rounded to fp32 (1.5f * extent[0] rounded once), m NaN when either term is NaN
 * (torch.max): a row with a NaN x or y is selected only by r < S; z is not read.
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, fp32, contiguous, `stream` a
 * hipStream_t, gsr_last_error() on failure.
 */
#ifndef GSR_MODEL_INIT_H
#define GSR_MODEL_INIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GSR_MODEL_INIT_PLAIN = 0, GSR_MODEL_INIT_SKYBOX = 1 };

/* Bytes of device scratch gsr_model_init_cloud needs (the kNN's included); 0 for bad sizes. */
size_t gsr_model_init_scratch_bytes(int64_t N, int64_t S);

/* points, colors: (N, 3), N >= 1.  u_theta, u_phi: (S) uniform draws in [0, 1) (NULL when S == 0).
 * mode GSR_MODEL_INIT_SKYBOX needs S >= 1, GSR_MODEL_INIT_PLAIN needs S == 0.  M: SH coefficients per
 * row, 1 <= M <= 16.  Outputs for S + N < 2^31 rows.  bounds (host, 4 floats, or NULL): mean x, y, z
 * and radius.  Synchronises `stream` once (the bounding box and the non-finite flag). */
int gsr_model_init_cloud(int64_t N, const float *points, const float *colors, int64_t S, const float *u_theta,
                         const float *u_phi, int M, int mode, float *xyz, float *features, float *opacity_raw,
                         float *scaling_raw, float *rotation, float *bounds, void *scratch, void *stream);

/* Bytes of device scratch the two calls below share for a scaffold of Ps rows; 0 for bad sizes. */
size_t gsr_scaffold_merge_scratch_bytes(int64_t Ps);

/* xyz: the scaffold's positions (Ps, 3), 0 <= Ps < 2^31; 0 <= S.  center, extent: host, 3 floats each.
 * count (device, one int64): K, the number of selected rows.  The row list stays in `scratch` for
 * gsr_scaffold_merge_write. */
int gsr_scaffold_merge_count(int64_t Ps, int64_t S, const float *xyz, const float *center, const float *extent,
                             void *scratch, int64_t *count, void *stream);

/* The K selected rows (as counted into `scratch`, original order) then the Pc chunk rows, for all five
 * arrays in one launch.  s_*: the scaffold's rows, SH (Ps, 4, 3).  c_*: the chunk's rows, SH (Pc, M, 3),
 * 4 <= M <= 16.  Outputs (K + Pc) rows with M coefficients; coefficients 4..M-1 of the scaffold rows 0. */
int gsr_scaffold_merge_write(int64_t Ps, int64_t K, const float *s_xyz, const float *s_shs, const float *s_opacity,
                             const float *s_scaling, const float *s_rotation, int64_t Pc, int M, const float *c_xyz,
                             const float *c_features, const float *c_opacity, const float *c_scaling,
                             const float *c_rotation, float *xyz, float *features, float *opacity_raw,
                             float *scaling_raw, float *rotation, const void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_MODEL_INIT_H */
