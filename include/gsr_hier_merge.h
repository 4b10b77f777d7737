/*
 * gsr_hier_merge.h -- C ABI of the hierarchy merger (csrc/hier_merge.hip): the last stage of the
 * reference's pipeline, which it runs as the GaussianHierarchyMerger tool over the post-optimised
 * chunk hierarchies (scripts/full_train.py:259-282) to write the merged.hier render_hierarchy.py
 * loads.  Exported by libgsr_hip.so.
 *
 * C chunk hierarchies in the builder's layout (gsr_hier_build.h: N_c = 2 P_c - 1 nodes, one Gaussian
 * per node, breadth-first ids) and one centre per chunk in; one hierarchy of N = 2K - 1 nodes out, in
 * the same layout.  Each chunk keeps the leaves nearer to its own centre than to any other chunk's
 * (ties to the lowest chunk), interior nodes left with one surviving child are spliced out, and the
 * chunks' trees are joined under a new upper tree built with the builder's rules A, B and E over the
 * chunk roots' rows.
 *
 * The rule (DESIGN.md "Hierarchy merger") is this project's definition: the published method's
 * consolidation restated.  The gaussianhierarchy tool is not vendored in the reference and no file it
 * wrote is available, so parity against it is UNPINNED; the kernels are pinned to the numpy
 * restatement tests/hier_merge_ref.py.
 *
 * The chunks are passed concatenated: chunk c's rows are [chunk_first[c], chunk_first[c + 1]) of every
 * input array, and the node indices inside `nodes` stay chunk-local.  Only the first N_c Gaussian
 * rows of a chunk are passed (a .hier_opt file may hold skybox rows after them).
 *
 * Conventions as in gsr.h: device pointers unless stated, fp32, 0 = GSR_OK, the message of a failure
 * in gsr_last_error().
 */
#ifndef GSR_HIER_MERGE_H
#define GSR_HIER_MERGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Leaves' owners are searched over the centres in batches of this many (staged through LDS). */
#define GSR_HIER_MERGE_CENTRE_BATCH 256

/* Device scratch of a merge of C chunks with `total_nodes` input nodes in all (0 when out of range:
 * C < 1, total_nodes < C or total_nodes > 2^31 - 1). */
size_t gsr_hier_merge_scratch_bytes(int64_t C, int64_t total_nodes);

/* Floats of the `top_rows` buffer of a merge of C chunks with M SH coefficients: (2C - 1) (19 + 3M). */
size_t gsr_hier_merge_top_floats(int64_t C, int M);

/* The plan: validation, ownership, survival, splicing, the top tree and the numbering.
 * Host inputs: chunk_first (C + 1, ascending from 0; T = chunk_first[C] <= 2^31 - 1).
 * Device inputs: centres (C,3) finite; the concatenated xyz (T,3), log_scales (T,3), rotations (T,4),
 * opacities (T), shs (T,M,3), nodes (T,7) int32, boxes (T,2,4).
 * Host outputs: leaves[c] = K_c, the chunk's surviving leaves; *out_nodes = N = 2 sum(K_c) - 1;
 * *levels = the merged tree's level count.
 * Device outputs, sized for the worst case of T + C - 1 nodes: nodes_out (T + C - 1, 7) and source
 * (T + C - 1, 2) int32, of which the first N rows are written (source[n] = {chunk, node id in the chunk}, {-1, -1} for a new top node);
 * top_rows (gsr_hier_merge_top_floats) and top_node (2C - 1) int32, which gsr_hier_merge_gather reads.
 * Every chunk's nodes are validated on the device before any kernel follows a parent or child index;
 * a violation is GSR_ERR_INVALID_ARGUMENT naming the chunk and its first offending node.  The call
 * reads the flag word, C counts and one word per level back and returns with the stream idle.
 * GSR_ERR_INVALID_ARGUMENT before any device work: C < 1, chunk_first not ascending from 0 or a chunk
 * with an even node count, T > 2^31 - 1, M outside 1..16, a NULL pointer, rotations / boxes /
 * top_rows not 16-byte aligned, scratch too small.  When no leaf survives: GSR_ERR_INVALID_ARGUMENT,
 * "no chunk has a surviving leaf". */
int gsr_hier_merge_plan(int64_t C, const int64_t *chunk_first, int M, const float *centres, const float *xyz,
                        const float *log_scales, const float *rotations, const float *opacities, const float *shs,
                        const int *nodes, const float *boxes, int64_t *leaves, int64_t *out_nodes, int *levels,
                        int *nodes_out, int *source, float *top_rows, int *top_node, void *scratch,
                        size_t scratch_bytes, void *stream);

/* The gather: the N rows of the merged hierarchy, after a plan with the same C, M, inputs and
 * scratch (unchanged since: it holds the chunk offsets).  A retained chunk node's attributes and box
 * are bit copies of the chunk's row; a new top node's come from top_rows.  out_rotations and
 * out_boxes 16-byte aligned.  Returns with the stream idle. */
int gsr_hier_merge_gather(int64_t C, int M, int64_t N, const float *xyz, const float *log_scales,
                          const float *rotations, const float *opacities, const float *shs, const float *boxes,
                          const int *source, const float *top_rows, const int *top_node, float *out_xyz,
                          float *out_log_scales, float *out_rotations, float *out_opacities, float *out_shs,
                          float *out_boxes, const void *scratch, size_t scratch_bytes, void *stream);

/* Device time of the calling thread's last plan and gather, in ms (HIP events): out[0..5] = ownership
 * (with the validation), survive, splice, numbering, top, gather.  Returns the number of values
 * written (at most n, at most 6). */
int gsr_hier_merge_stage_ms(float *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* GSR_HIER_MERGE_H */
