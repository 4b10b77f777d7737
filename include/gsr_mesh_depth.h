/*
 * gsr_mesh_depth.h -- C ABI of the depth supervision maps of a chunk: the reconstructed mesh ray cast
 * from a batch of pinhole cameras, and the 16-bit normalised inverse depth maps with their per-image
 * scale / offset.  Exported by libgsr_hip.so.
 *
 * Replaces steps 7 and 8 of the reference's ss_utils/ss_generate_depths.py: the embree ray cast of
 * render_depth_gaussians (ss_utils/deprecatedAndOthers/gaussian_splatting/render_depth_gaussians/
 * src/render_depth_gaussians.cpp, src/render/render_meshes.cpp) with its 3-channel distance code
 * (DistanceToColor, render_depth_gaussians.cpp:162-195), and ss_utils/depth_scripts/
 * depth_map_to_distances.py (convert_depth_map_to_meters :21-56, convert_to_gaussian_splatting_format
 * :58-123).  embree cannot be run beside this project, so the ray cast rule below is this project's
 * own; the encode is the script's arithmetic, in fp64 where the script's is.
 *
 * Ray cast.  A camera is 11 doubles: the COLMAP qvec (w, x, y, z), tvec (x_cam = R x + t), fx, fy, cx,
 * cy.  In fp64: q is normalised, R is its rotation matrix, C = -R^T t the camera centre.  Then R, fx,
 * fy, cx, cy are rounded to fp32 and C is split into C_hi = fp32(C), C_lo = fp32(C - C_hi).  All
 * that follows is fp32, every operation rounded once, no contraction, in the order written:
 *   e   = (v - C_hi) - C_lo                      per vertex v and axis: differences formed first, so the
 *   a   = R e: a_x = ((R00 e_x + R01 e_y) + R02 e_z), likewise a_y, a_z; b and c from v1 and v2
 *                                                 arithmetic runs at the scale of the view
 *   d   = (((ix + 0.5) - cx) / fx, ((iy + 0.5) - cy) / fy, 1)          the ray of pixel (ix, iy)
 *   X(p, q) = (p_y q_z - p_z q_y, p_z q_x - p_x q_z, p_x q_y - p_y q_x)     two products, one subtraction
 *   E(p, q) = (d_x X_x + d_y X_y) + X_z          the edge function, with p, q put in ascending
 *                                                 lexicographic (x, y, z) order first and the sign
 *                                                 flipped when that swapped them
 *   U = E(b, c), V = E(c, a), W = E(a, b)
 *   inside = (U >= 0 && V >= 0 && W >= 0 || U <= 0 && V <= 0 && W <= 0) && !(U == 0 && V == 0 && W == 0)
 *   n   = X'(b - a, c - a), X' being X with each component x y - z w computed as
 *         fma(x, y, -rn(z w)) + fma(-z, w, rn(z w)): the only fused operations; they keep a needle's
 *         normal, a difference of products that cancels, to a few ulp
 *   na  = (n_x a_x + n_y a_y) + n_z a_z,  nd = (n_x d_x + n_y d_y) + n_z
 *   s   = na / nd                                 the hit's camera z
 *   t   = s sqrt((d_x d_x + d_y d_y) + 1)         its distance along the ray
 *   hit = inside && nd != 0 && s > 0 && tnear < t && t <= tfar
 * The test is two-sided (no back-face culling).  The two triangles that share an edge compute its
 * edge function from the same ordered pair, so their results are exact negatives and a ray through
 * the edge is inside at least one of them.  A triangle with two equal vertices has E = 0 on that
 * edge and exact negatives on the other two: it misses; so does one whose n is zero.
 * The pixel's value is the smallest t (mode 0), or the smallest s (mode 1: camera z, what the
 * rasterizer's inverse depth is the reciprocal of), over the triangles that hit; 0 when none does.
 * A minimum does not depend on the order it is taken in: reruns are bitwise equal.
 *
 * The reference renders 1536 x 1536 and keeps every third sample (INTER_NEAREST): its sample of output
 * pixel ix sits at ix + 1/6, not ix + 1/2.  A caller who wants that passes cx + 1/3, cy + 1/3.
 *
 * Encode (fp64).  depth and background of a distance d:
 *   quantize = 0:  depth = (double)d, background = (d == 0)
 *   quantize = 1:  mm = 1000.0 * (double)d; background when !(mm >= 1) or mm > 1048576; else
 *                  k = 1, 2, 3 for mm <= 65536, <= 262144, <= 1048576; units = (uint32)(mm / 4^k);
 *                  depth = (double)((units & 0x3FFF) << 2k) / 1000.0
 *                  (DistanceToColor, then the code's own decode.  At mm = 65536, 262144 and 1048576
 *                  exactly, units = 16384 carries out of the 14 unit bits into the precision bits the
 *                  code ORs it with: the decode returns depth 0 on a pixel that is not background.
 *                  That is the reference's; it is reproduced, not repaired.)
 *   valid  = !background && depth > min_depth && (max_depth <= 0 || depth < max_depth)
 *   inv    = 1.0 / depth;  lo, hi = min, max of inv over the image's valid pixels
 *   hi > lo:   scale = hi - lo, offset = lo, u16 = (uint16)(clip((inv - offset) / scale, 0, 1) * 65535)
 *              (truncated) on valid pixels, 0 elsewhere
 *   hi == lo:  scale = 0, offset = lo, u16 = 0;        no valid pixel: scale = offset = 0, u16 = 0
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, fp32, `stream` a hipStream_t.
 */
#ifndef GSR_MESH_DEPTH_H
#define GSR_MESH_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scratch of gsr_mesh_distance_maps for K cameras and F triangles (0 when K F is < 1 or >= 2^31). */
size_t gsr_mesh_distance_scratch_bytes(int64_t K, int64_t F);

/* out (K, H, W): the ray cast above of the mesh vertices (V, 3) fp32, faces (F, 3) int32 from the K
 * cameras cams (K, 11) fp64, all of W x H pixels.  mode 0: distance along the ray; 1: camera z.
 * 0 <= tnear < tfar, both finite; 1 <= W, H <= 32768; K F < 2^31; K tiles-per-camera < 2^31.
 * K, F, W or H of 0 is a no-op that returns GSR_OK (with F == 0 and the rest positive, out is zeroed).
 * A face with an index outside [0, V) or a non-finite vertex is skipped.
 * The (camera, tile, triangle) references are held in device memory the call allocates once their
 * number is known and frees before it returns: the call synchronises `stream` (twice).  More than
 * 2^31 - 1 references is GSR_ERR_INVALID_ARGUMENT: pass fewer cameras per call.
 * stats (host, 6 x int64, or NULL): references, of which oversize (per-camera list), the longest
 * run one tile walks (its own and its camera's oversize list), tiles with a run of their own, and
 * the microseconds between device events around the binning (cameras to sort, its one wait on the
 * host included) and around the ray cast kernel (0 where no frame held a triangle). */
int gsr_mesh_distance_maps(int64_t V, const float *vertices, int64_t F, const int32_t *faces, int64_t K,
                           const double *cams, int W, int H, double tnear, double tfar, int mode, void *scratch,
                           float *out, int64_t *stats, void *stream);

/* Scratch of gsr_depth_encode for K images (0 for K < 1). */
size_t gsr_depth_encode_scratch_bytes(int64_t K);

/* The encode above of distance (K, H, W) into out_u16 (K, H, W) uint16 and, on the host, scale[K] and
 * offset[K] (doubles).  K <= 65535; min_depth >= 0 and finite; max_depth <= 0: none.  Each launch covers
 * the whole batch: the per-image minimum and maximum (atomics on the doubles' bit patterns, which
 * order as the positive doubles do: the result does not depend on the order), then the
 * normalisation, which reads them on the device.  The call synchronises `stream` once, to hand scale
 * and offset to the host.
 * K, H or W of 0 is a no-op that returns GSR_OK. */
int gsr_depth_encode(int64_t K, int H, int W, const float *distance, int quantize, double min_depth, double max_depth,
                     void *scratch, uint16_t *out_u16, double *scale, double *offset, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_MESH_DEPTH_H */
