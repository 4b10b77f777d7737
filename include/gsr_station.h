/*
 * gsr_station.h -- C ABI of the station render: the F cube faces of one recording position drawn
 * from one hierarchy cut (csrc/station.hip).  Exported by libgsr_hip.so.
 *
 * A street recording is a set of stations: one camera centre with four to six faces around it.  The
 * cut, the interpolation weights, render_post's child / parent blend, the world-space covariance and
 * the SH colour (its direction is mean - campos) read the centre only, so they are the same for every
 * face.  gsr_rasterize_station_forward does that work once for the R rows of the cut
 * (station_rows), keeps for each face the rows that reach it, in cut order, and runs the existing
 * forward on each face's compact rows (cov3D_precomp + colors_precomp, GSR_FWD_NO_BACKWARD).
 * Inference only: no backward exists for these frames.
 *
 * Conventions as in gsr.h (device pointers, stream, resize callbacks, status codes,
 * gsr_last_error).  New entry points only: GSR_ABI_VERSION is unchanged.
 */
#ifndef GSR_STATION_H
#define GSR_STATION_H

#include <stddef.h>
#include <stdint.h>

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most faces one call takes (a row's faces are one byte of flags). */
#define GSR_STATION_MAX_FACES 8
/* A compact row: mean 3, covariance 6 (xx,xy,xz,yy,yz,zz), opacity 1, rgb 3. */
#define GSR_STATION_ROW_FLOATS 13
/* Arrays per face in the rows buffer: means (P,3), cov3D (P,6), opacity (P), rgb (P,3) float32,
 * src (P) int32 = the row's index in the cut, radii (P) int32 = the face frame's radii. */
#define GSR_STATION_FACE_ARRAYS 6

/* Bytes of `scratch` for a cut of R rows and F faces: the R staged rows (52 B each), one byte of
 * face flags per row, the per-face tile and group sums.  0 when F is out of range or R < 0. */
size_t gsr_station_rows_scratch_bytes(int64_t R, int F);

/* Host arithmetic only: the rows buffer for faces that keep kept[0..F) rows.  Returns its size in
 * bytes; offsets (optional, F * GSR_STATION_FACE_ARRAYS entries) receives each face's array offsets in
 * the order above.  Every array starts on a 256-byte boundary. */
size_t gsr_station_rows_layout(int F, const int64_t *kept, size_t *offsets);

/* The station forward.
 *   N hierarchy rows: means3D (N,3), shs (N,16,3), opacities (N), scales (N,3), rotations (N,4),
 *     activated, as render_post reads them; M must be 16, shs and rotations 16-byte aligned (the
 *     conditions of the fused single-view cut frame).  The scale modifier is 1.
 *   The cut: render_indices / parent_indices (int32) and interpolation_weights (float32), R entries
 *     each; parent -1 = the last row; R = 0 is valid (every face is the background).
 *   F faces (1 .. GSR_STATION_MAX_FACES) that share the centre cam_pos[3], the size and the field of
 *     view: viewmatrices / projmatrices (F,16), 16-byte aligned, in gsr.h's matrix convention.
 *   D = active SH degree (0..3).
 *   scratch: gsr_station_rows_scratch_bytes(R, F) bytes, 256-byte aligned.
 *   rows_buffer: asked once per call (when some face keeps a row) for gsr_station_rows_layout's
 *     bytes; it holds each face's compact rows, readable after the call until the caller reuses it.
 *     geom / binning / image_buffer: as gsr_rasterize_forward_ex, asked once per face (binning may be
 *     asked again when a face's capacity was short); a buffer need not outlive the next request for
 *     it: the faces run one after another on `stream`.
 * Outputs: out_color (F,3,H,W); out_invdepth (F,1,H,W) or NULL; radii (F,R) int32, a face's radii at
 *   the rows' places in the cut and zero elsewhere; num_rendered[F] (host) = each face's K;
 *   rows_kept[F] (host, optional) = each face's kept rows P_f.  A row the single-view frame of a face
 *   gives radii > 0 is always kept for that face; rows it culls (view depth <= 0.2, an empty tile
 *   rectangle) are dropped.  The host waits once for the F counts.
 * Returns GSR_ERR_INVALID_ARGUMENT for F < 1, F > GSR_STATION_MAX_FACES, M != 16, misaligned or NULL
 * pointers, a bad degree or size. */
int gsr_rasterize_station_forward(gsr_resize_fn geom_buffer, gsr_resize_fn binning_buffer,
                                  gsr_resize_fn image_buffer, gsr_resize_fn rows_buffer, void *resize_ctx,
                                  void *scratch, size_t scratch_bytes, int64_t N, int D, int M,
                                  const float *means3D, const float *shs, const float *opacities,
                                  const float *scales, const float *rotations, const int *render_indices,
                                  const int *parent_indices, const float *interpolation_weights, int R, int F,
                                  const float *viewmatrices, const float *projmatrices, const float *cam_pos,
                                  float tan_fovx, float tan_fovy, int width, int height, const float *background,
                                  float *out_color, float *out_invdepth, int *radii, int64_t *num_rendered,
                                  int64_t *rows_kept, int debug, void *stream);

/* Device time of the last station call's stages on this thread, filled only after
 * gsr_station_set_profiling(1) (HIP events): 0 station_rows + the group scan, 1 the host's read of
 * the counts and the compaction's write launch, 2 the F face frames, 3 the radii scatter.  Returns the
 * number of values written; gsr_station_set_profiling returns the previous setting. */
int gsr_station_set_profiling(int enable);
int gsr_station_stage_times_ms(float *out, int max_stages);

#ifdef __cplusplus
}
#endif
#endif /* GSR_STATION_H */
