/*
 * gsr_hier_build.h -- C ABI of the LOD hierarchy builder (csrc/hier_build.hip): the step between a
 * trained chunk (train_single.py) and its post-optimisation (train_post.py) that the reference runs
 * as the GaussianHierarchyCreator tool (scripts/full_train.py:152,203-216).  Exported by
 * libgsr_hip.so.
 *
 * P Gaussians in, a binary hierarchy of N = 2P - 1 nodes out, one Gaussian per node (Gaussian row n
 * belongs to node n), in the layout gsr_expand_to_size / gsr_interpolation_weights read
 * (gsr_hier.h): nodes (N, 7) int32 {depth, parent, start, count_leafs, count_merged,
 * start_children, count_children}, boxes (N, 2, 4) float {minn.xyz, size | maxx.xyz, 0}.
 *
 * The rule (DESIGN.md "Hierarchy builder") is this project's definition: Kerbl et al. 2024 sec. 5
 * restated over an LBVH (63-bit Morton order, Karras 2012 topology with ties broken by sorted
 * position, breadth-first node ids, surface-weighted moment-matching merges).  The gaussianhierarchy
 * tool is not vendored in the reference, so parity against it is UNPINNED; the kernels are pinned to
 * the numpy restatement tests/hier_build_ref.py.
 *
 * Conventions as in gsr.h: device pointers, fp32, 0 = GSR_OK, the message of a failure in
 * gsr_last_error().
 */
#ifndef GSR_HIER_BUILD_H
#define GSR_HIER_BUILD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device scratch gsr_hier_build needs for P input rows (0 when P is out of range). */
size_t gsr_hier_build_scratch_bytes(int64_t P);

/* Inputs, P rows: xyz (P,3) finite; log_scales (P,3); rotations (P,4) raw quaternions (r, x, y, z);
 * opacities (P) activated; shs (P, M, 3), 1 <= M <= 16.  Outputs, N = 2P - 1 rows: the five
 * attribute arrays, nodes (N,7), boxes (N,2,4) and leaf_rows (N): the input row of a leaf, -1 for an
 * interior node.  *levels (a host int) receives the number of tree levels (root = level 0).
 * The call reads one word per level back to the host and returns with the stream idle.
 * GSR_ERR_INVALID_ARGUMENT before any device work: P < 1 or P > 2^30, M outside 1..16, a NULL
 * pointer, rotations / out_rotations / boxes not 16-byte aligned (they are read and written as
 * float4), scratch_bytes < gsr_hier_build_scratch_bytes(P). */
int gsr_hier_build(int64_t P, int M, const float *xyz, const float *log_scales, const float *rotations,
                   const float *opacities, const float *shs, float *out_xyz, float *out_log_scales,
                   float *out_rotations, float *out_opacities, float *out_shs, int *nodes, float *boxes,
                   int *leaf_rows, int *levels, void *scratch, size_t scratch_bytes, void *stream);

/* Device time of the calling thread's last gsr_hier_build, in ms (HIP events): out[0..3] = sort
 * (bounds, keys, radix sort), topology, numbering (breadth-first ids, node rows), merge (leaf rows
 * and the per-level merges).  Returns the number of values written (at most n, at most 4). */
int gsr_hier_build_stage_ms(float *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* GSR_HIER_BUILD_H */
