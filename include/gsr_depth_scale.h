/*
 * gsr_depth_scale.h -- C ABI of the depth scale fit: per image the affine map (scale, offset) that takes a
 * 16-bit inverse depth map of unknown scale (a monocular depth network's, or any PNG a user brings) onto
 * the inverse depths of the calibrated sparse points the image observes.  Exported by libgsr_hip.so.
 *
 * Replaces get_scales of the reference's preprocess/make_depth_scale.py (:19-75), which
 * preprocess/make_chunks_depth_scale.py runs once per chunk.  The rule, for one image:
 *
 *   masked  = 0 <= pid < T, T = the largest point id + 1.  A masked id with no row in the point table
 *             takes the point (0, 0, 0) (missing = 0, "origin": the reference's zero rows) or leaves the
 *             observation out of masked (missing = 1, "skip").
 *   z       = ((R20 X + R21 Y) + R22 Z) + t2, fp64, every operation rounded once; inv = 1 / z.
 *             R is qvec2rotmat(q), made on the host in fp64.
 *   s       = Hd / height (fp64);  m = fl32(xy s) per component: an fp64 product, one rounding to fp32
 *   valid   = masked and m.x >= 0, m.y >= 0, m.x < fl32(width s), m.y < fl32(height s) in fp32, inv > 0
 *             (NaN fails, -0.0 passes)
 *   fitted  = (number of valid) > 10 and max(inv) - min(inv) > 1e-3 over the MASKED observations (points
 *             behind the camera count; a NaN among them makes it false).  Not fitted: scale = offset = 0.
 *   v       = the map's bilinear sample at m: src = u16 / 65536 (fp32); sx = rint(32 m.x) (ties to even,
 *             saturating at 2^30), ix = sx >> 5, fx = (sx & 31) / 32, likewise y; ix, ix + 1, iy, iy + 1
 *             clamped into the map; v = ((S00 w00 + S01 w01) + S10 w10) + S11 w11 in fp32 with
 *             w00 = (1 - fy)(1 - fx), w01 = (1 - fy) fx, w10 = fy (1 - fx), w11 = fy fx.
 *             (cv2.remap's INTER_LINEAR / BORDER_REPLICATE as this project states it: OpenCV cannot be
 *             run beside this project, so this step's parity is unpinned.)
 *   t_colmap = median of the valid inv (fp64; even count: fl64(a + b) / 2 of the two middle values)
 *   t_mono   = median of the valid v (fp32, the same form)
 *   s_colmap = mean of |inv - t_colmap|;  s_mono = mean of fl32(|v - t_mono|): fp64 sums in a fixed order,
 *              divided by the count in fp64 (numpy's float32 pairwise mean of s_mono is not reproduced)
 *   scale    = s_colmap / s_mono,  offset = t_colmap - t_mono scale  (fp64, IEEE: a flat map gives
 *              inf / -inf, 0 / 0 gives NaN, as in the reference)
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, `stream` a hipStream_t.
 */
#ifndef GSR_DEPTH_SCALE_H
#define GSR_DEPTH_SCALE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A camera is 15 doubles: R row-major (9), t (3), width, height, the index of its map or -1. */
#define GSR_DEPTH_SCALE_CAMERA_DOUBLES 15

#define GSR_DEPTH_SCALE_FITTED 1u   /* scale and offset are the fit's (else both 0) */
#define GSR_DEPTH_SCALE_NO_MAP 2u   /* the camera's map index is outside [0, K): the record is otherwise 0 */
#define GSR_DEPTH_SCALE_NAN_SEEN 4u /* a masked observation's inv is NaN */

/* The statistics are 0 where the image is not fitted; n_valid is set whenever the camera has a map. */
typedef struct gsr_depth_scale_record {
    double scale, offset, t_colmap, s_colmap, t_mono, s_mono;
    int32_t n_valid;
    uint32_t flags;
} gsr_depth_scale_record;

/* C: the longest observation range whose valid (inv, v) pairs stay in LDS; longer ranges go through
 * the scratch, by the same code. */
int gsr_depth_scale_lds_capacity(void);

/* Scratch of gsr_depth_scale_fit for ranges over L entries in all (0 for L < 1). */
size_t gsr_depth_scale_scratch_bytes(int64_t L);

/* records[k], k < M: the fit above of camera k = cams[15 k ..] over its observations.  Those are
 * obs_index[obs_offsets[k] .. obs_offsets[k + 1]) as indices into obs_xy (O, 2) fp64 and obs_point_id (O)
 * int64 (Chunk.obs_index / obs_offsets), or, with obs_index NULL, that range of the arrays itself.
 * L: the entries obs_offsets addresses (the length of obs_index, or O); obs_offsets (M + 1) int64 should
 * ascend from 0 to L: a range reaching outside [0, L) is cut to it, a descending one is empty, an
 * obs_index entry outside [0, O) is no observation.  table (T) int32: gsr_chunk_id_table's, over the N
 * rows of point_xyz (N, 3) fp64.  maps: (K, Hd, Wd) uint16.  missing: 0 origin, 1 skip.
 * 0 <= M < 2^31; Hd, Wd >= 1 when M > 0; T <= 2^31 - 1.  M = 0 launches nothing.
 * One launch for the whole batch (one workgroup per camera), no allocation and no synchronisation:
 * the records are on the device, in stream order.  Two calls on the same input write the same bits. */
int gsr_depth_scale_fit(int64_t M, const double *cams, const int64_t *obs_offsets, int64_t L, const int64_t *obs_index,
                        int64_t O, const double *obs_xy, const int64_t *obs_point_id, int64_t N, int64_t T,
                        const int32_t *table, const double *point_xyz, int64_t K, int Hd, int Wd, const uint16_t *maps,
                        int missing, void *scratch, gsr_depth_scale_record *records, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_DEPTH_SCALE_H */
