// station.hip -- the F cube faces of one recording position from one hierarchy cut
// (include/gsr_station.h).
//
// The reference draws every camera of a recording position on its own (render_hierarchy.py,
// render_position.py): each gets its own expand_to_size, get_interpolation_weights and render_post.
// The cut, the weights, the child / parent blend, the world-space covariance and the SH colour read
// the camera centre only, so for the faces of one station they are the same work.  Here:
//
//   station_rows     one pass over the R rows of the cut: the blend (gsr_device.h's cut_source /
//                    cut_lerp, the fused preprocess's expressions), the covariance
//                    (cov3d_from_scale_rot), the SH colour (sh_dir / sh_channel, + 0.5, clamp at 0),
//                    a 13-float row staged; per face the keep test and one ballot per wave, the
//                    tile's sums stored and added to its group's (one atomic per tile and face)
//   station_scan     one workgroup: the groups' exclusive sums and each face's total (the F counts
//                    the host reads to size the rows buffer)
//   station_compact  per tile: its offsets from the group prefix and the group's earlier tiles -- no
//                    workgroup waits for another -- then each kept row to its face's dense arrays, in
//                    cut order (depth ties resolve as in the single-view frame)
//   the F face frames  gsr_rasterize_forward_ex on the compact rows (cov3D_precomp +
//                    colors_precomp, GSR_FWD_NO_BACKWARD): no gather, no covariance, no SH pass
//   station_scatter  every face's radii back through src into (F, R)
//
// The keep test of a face is the preprocess's own cull: view_depth_culled on the view-space mean,
// then the tile rectangle of the projected splat from the same shared device functions in the same
// order (ewa_rows, quad_form, ndc2pix, get_rect); the library is compiled with -ffp-contract=off, so
// the same expressions give the same bits and a row is dropped exactly when the face's preprocess
// would leave its radii at 0.
#include <algorithm>
#include <atomic>
#include <string>

#include "../../include/gsr_station.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr int kStThreads = 256;           // one row per thread
constexpr int kStTile = kStThreads;       // rows per compaction tile
constexpr int kStWaves = kStThreads / kWave;
constexpr int kStGroup = 256;             // tiles per group sum
constexpr int kStMaxF = GSR_STATION_MAX_FACES;
constexpr int kStRow = GSR_STATION_ROW_FLOATS;
static_assert(kStMaxF <= 8, "a row's faces are one byte of flags");

struct StScratch {
    float *rows;         // R x 13: the staged rows
    uint8_t *mask;       // R: bit f = face f keeps the row
    uint32_t *tile_cnt;  // F x ntiles
    uint32_t *grp;       // F x ngroups: the groups' sums, then (station_scan) their exclusive prefix
    uint32_t *counts;    // kStMaxF: each face's total
};

struct StFaces {  // each face's dense arrays in the rows buffer
    float *means[kStMaxF], *cov[kStMaxF], *opac[kStMaxF], *rgb[kStMaxF];
    int *src[kStMaxF], *radii[kStMaxF];
    int64_t kept[kStMaxF];
};

struct StView {
    const float *views, *projs;  // (F,16) each
    int F, W, H, gx, gy;
    float tanx, tany, fx, fy;
};

inline int64_t st_tiles(int64_t R) { return (R + kStTile - 1) / kStTile; }
inline int64_t st_groups(int64_t ntiles) { return (ntiles + kStGroup - 1) / kStGroup; }

size_t st_carve(int64_t R, int F, StScratch *sc, char *base) {
    const int64_t ntiles = st_tiles(std::max<int64_t>(R, 1)), ngroups = st_groups(ntiles);
    size_t off = 0;
    const auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off = (off + bytes + 255) & ~(size_t)255;
        return p;
    };
    char *rows = take(sizeof(float) * kStRow * (size_t)std::max<int64_t>(R, 1));
    char *mask = take((size_t)std::max<int64_t>(R, 1));
    char *tc = take(sizeof(uint32_t) * (size_t)F * (size_t)ntiles);
    char *gr = take(sizeof(uint32_t) * (size_t)F * (size_t)ngroups);
    char *cn = take(sizeof(uint32_t) * kStMaxF);
    if (sc) {
        sc->rows = reinterpret_cast<float *>(rows);
        sc->mask = reinterpret_cast<uint8_t *>(mask);
        sc->tile_cnt = reinterpret_cast<uint32_t *>(tc);
        sc->grp = reinterpret_cast<uint32_t *>(gr);
        sc->counts = reinterpret_cast<uint32_t *>(cn);
    }
    return off;
}

// Whether face (V, Pm) may draw the row: the cull of preprocess_kernel up to `area == 0`.
__device__ __forceinline__ bool face_keeps(float3 p, const float c3[6], const Mat4 &V, const Mat4 &Pm,
                                           const StView &v) {
    const float3 pv = xf_point43(p, V);
    if (view_depth_culled(pv)) return false;
    const float4 ph = xf_point44(p, Pm);
    const float pw = 1.0f / (ph.w + 0.0000001f);
    const float ndcx = ph.x * pw, ndcy = ph.y * pw;
    const Ewa e = ewa_rows(p, V, v.fx, v.fy, v.tanx, v.tany);
    const float ca = quad_form(e.m0, c3, e.m0) + 0.3f;
    const float cb = quad_form(e.m0, c3, e.m1);
    const float cc = quad_form(e.m1, c3, e.m1) + 0.3f;
    const float det = ca * cc - cb * cb;
    if (det == 0.0f) return false;
    const float mid = 0.5f * (ca + cc);
    const float lambda1 = mid + sqrtf(fmax_(0.1f, mid * mid - det));
    const float radius = ceilf(3.f * sqrtf(lambda1));
    const float px = ndc2pix(ndcx, v.W), py = ndc2pix(ndcy, v.H);
    const Rect r = get_rect(px, py, (int)radius, v.gx, v.gy);
    return (r.x1 - r.x0) * (r.y1 - r.y0) != 0;
}

// One row per thread, one tile per workgroup.  M = 16; shs and rotations are 16-byte aligned.
__global__ __launch_bounds__(kStThreads) void station_rows_kernel(
    int R, int D, const float *__restrict__ means3D, const float *__restrict__ scales,
    const float *__restrict__ rotations, const float *__restrict__ opacities, const float *__restrict__ shs,
    const float *__restrict__ campos, CutRef cut, StView v, StScratch sc, int64_t ntiles, int64_t ngroups) {
    __shared__ uint32_t s_cnt[kStMaxF][kStWaves];
    const int64_t tile = blockIdx.x;
    const int64_t r = tile * kStTile + threadIdx.x;
    const int wv = threadIdx.x >> 6;
    const bool live = r < (int64_t)R;
    float3 p = make_float3(0.f, 0.f, 0.f);
    float c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        int64_t ci, pi;
        float ct;
        cut_source(cut, r, ci, pi, ct);
        // the blend as the fused preprocess forms it
        p = make_float3(cut_lerp(ct, means3D[3 * ci], means3D[3 * pi]),
                        cut_lerp(ct, means3D[3 * ci + 1], means3D[3 * pi + 1]),
                        cut_lerp(ct, means3D[3 * ci + 2], means3D[3 * pi + 2]));
        const float3 s =
            make_float3(cut_lerp(ct, scales[3 * ci], scales[3 * pi]), cut_lerp(ct, scales[3 * ci + 1], scales[3 * pi + 1]),
                        cut_lerp(ct, scales[3 * ci + 2], scales[3 * pi + 2]));
        const float4 qc = reinterpret_cast<const float4 *>(rotations)[ci];
        float4 qp = reinterpret_cast<const float4 *>(rotations)[pi];
        const float dot = qc.x * qp.x + qc.y * qp.y + qc.z * qp.z + qc.w * qp.w;  // torch.bmm, left to right
        if (dot < 0.f) qp = make_float4(-qp.x, -qp.y, -qp.z, -qp.w);
        const float4 q = make_float4(cut_lerp(ct, qc.x, qp.x), cut_lerp(ct, qc.y, qp.y), cut_lerp(ct, qc.z, qp.z),
                                     cut_lerp(ct, qc.w, qp.w));
        cov3d_from_scale_rot(s, 1.f, q, c3);
        const float op = cut_lerp(ct, opacities[ci], opacities[pi]);
        // the SH row blended float4 by float4 (the colour pass's expressions), coefficients above
        // the active degree not fetched
        const int nc = (D + 1) * (D + 1);
        const float4 *c4 = reinterpret_cast<const float4 *>(shs) + ci * 12;
        const float4 *p4 = reinterpret_cast<const float4 *>(shs) + pi * 12;
        float sh[48];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * k < nc * 3) {
                const float4 a = c4[k], b = p4[k];
                w = make_float4(cut_lerp(ct, a.x, b.x), cut_lerp(ct, a.y, b.y), cut_lerp(ct, a.z, b.z),
                                cut_lerp(ct, a.w, b.w));
            }
            sh[4 * k] = w.x; sh[4 * k + 1] = w.y; sh[4 * k + 2] = w.z; sh[4 * k + 3] = w.w;
        }
#pragma unroll
        for (int k = 0; k < 48; k++) sh[k] = k < nc * 3 ? sh[k] : 0.f;  // tail of a partial float4
        float dir[3], dor[3];
        sh_dir(p, make_float3(campos[0], campos[1], campos[2]), dir, dor);
        float rgb[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float val = sh_channel(D, sh + ch, dir[0], dir[1], dir[2]);
            rgb[ch] = val < 0.f ? 0.f : val;
        }
        float *o = sc.rows + (size_t)r * kStRow;
        o[0] = p.x; o[1] = p.y; o[2] = p.z;
#pragma unroll
        for (int k = 0; k < 6; k++) o[3 + k] = c3[k];
        o[9] = op;
        o[10] = rgb[0]; o[11] = rgb[1]; o[12] = rgb[2];
    }
    uint32_t m = 0;
    for (int f = 0; f < v.F; f++) {
        const Mat4 V = load_mat4(v.views + 16 * f);
        const Mat4 Pm = load_mat4(v.projs + 16 * f);
        const bool keep = live && face_keeps(p, c3, V, Pm, v);
        const uint64_t b = __ballot(keep);
        if ((threadIdx.x & 63) == 0) s_cnt[f][wv] = (uint32_t)__popcll(b);
        m |= keep ? 1u << f : 0u;
    }
    if (live) sc.mask[r] = (uint8_t)m;
    __syncthreads();
    if ((int)threadIdx.x < v.F) {
        const int f = threadIdx.x;
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < kStWaves; w++) n += s_cnt[f][w];
        sc.tile_cnt[(size_t)f * ntiles + tile] = n;
        if (n) atomicAdd(sc.grp + (size_t)f * ngroups + tile / kStGroup, n);
    }
}

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t x, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, kWave);
        if (lane >= d) x += y;
    }
    return x;
}

// One workgroup of F waves: wave f turns face f's group sums into their exclusive prefix and stores
// the face's total.
__global__ __launch_bounds__(kStMaxF *kWave) void station_scan_kernel(int F, int64_t ngroups, StScratch sc) {
    const int f = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (f >= F) return;
    uint32_t *g = sc.grp + (size_t)f * ngroups;
    uint32_t carry = 0;
    for (int64_t c0 = 0; c0 < ngroups; c0 += kWave) {
        const int64_t i = c0 + lane;
        const uint32_t x = i < ngroups ? g[i] : 0u;
        const uint32_t inc = wave_incl_scan_u32(x, lane);
        if (i < ngroups) g[i] = carry + inc - x;
        carry += __shfl(inc, kWave - 1, kWave);
    }
    if (lane == 0) sc.counts[f] = carry;
}

__global__ __launch_bounds__(kStThreads) void station_compact_kernel(int R, int F, StScratch sc, StFaces out,
                                                                     int64_t ntiles, int64_t ngroups) {
    __shared__ uint32_t s_part[kStMaxF][kStWaves];
    __shared__ uint32_t s_cnt[kStMaxF][kStWaves];
    const int64_t tile = blockIdx.x;
    const int64_t g = tile / kStGroup;
    const int in_group = (int)(tile - g * kStGroup);  // the group's earlier tiles: < kStGroup = kStThreads
    const int64_t r = tile * kStTile + threadIdx.x;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t m = r < (int64_t)R ? sc.mask[r] : 0u;
    uint64_t ranks = 0;  // the row's rank among its wave's kept rows, one byte per face
    for (int f = 0; f < F; f++) {
        uint32_t x = (int)threadIdx.x < in_group ? sc.tile_cnt[(size_t)f * ntiles + g * kStGroup + threadIdx.x] : 0u;
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_xor(x, d, kWave);
        const uint64_t b = __ballot((m >> f) & 1u);
        ranks |= (uint64_t)__popcll(b & ((1ull << lane) - 1ull)) << (8 * f);
        if (lane == 0) {
            s_part[f][wv] = x;
            s_cnt[f][wv] = (uint32_t)__popcll(b);
        }
    }
    __syncthreads();
    if (!m) return;
    float row[kStRow];
    const float *src = sc.rows + (size_t)r * kStRow;
#pragma unroll
    for (int k = 0; k < kStRow; k++) row[k] = src[k];
    for (int f = 0; f < F; f++) {
        if (!((m >> f) & 1u)) continue;
        uint32_t at = sc.grp[(size_t)f * ngroups + g] + (uint32_t)((ranks >> (8 * f)) & 0xFFu);
#pragma unroll
        for (int w = 0; w < kStWaves; w++) at += s_part[f][w] + (w < wv ? s_cnt[f][w] : 0u);
        if ((int64_t)at >= out.kept[f]) continue;  // never past the face's arrays
        float *mo = out.means[f] + 3 * (size_t)at, *co = out.cov[f] + 6 * (size_t)at, *go = out.rgb[f] + 3 * (size_t)at;
        mo[0] = row[0]; mo[1] = row[1]; mo[2] = row[2];
#pragma unroll
        for (int k = 0; k < 6; k++) co[k] = row[3 + k];
        out.opac[f][at] = row[9];
        go[0] = row[10]; go[1] = row[11]; go[2] = row[12];
        out.src[f][at] = (int)r;
    }
}

// radii (F, R), zeroed by the caller: every face's radii at its rows' places in the cut
__global__ __launch_bounds__(256) void station_scatter_kernel(int R, StFaces in, int *__restrict__ radii) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.kept[f]) return;
    const int r = in.src[f][i];
    if (r < 0 || r >= R) return;
    radii[(size_t)f * R + r] = in.radii[f][i];
}

int fail_st(int code, const std::string &m) {
    set_last_error("gsr_rasterize_station_forward: " + m);
    return code;
}

std::atomic<int> g_st_profile{0};
constexpr int kStStages = 4;
thread_local hipEvent_t t_ev[kStStages + 1];
thread_local bool t_ev_init = false, t_ev_valid = false;

bool st_profile() { return g_st_profile.load(std::memory_order_relaxed) != 0; }
void st_mark(int k, hipStream_t s) {
    if (!st_profile()) return;
    if (!t_ev_init) {
        for (auto &e : t_ev) (void)hipEventCreate(&e);
        t_ev_init = true;
    }
    (void)hipEventRecord(t_ev[k], s);
    if (k == kStStages) t_ev_valid = true;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_station_rows_scratch_bytes(int64_t R, int F) {
    if (F < 1 || F > kStMaxF || R < 0 || R > INT32_MAX) return 0;
    return st_carve(R, F, nullptr, nullptr) + 256;
}

size_t gsr_station_rows_layout(int F, const int64_t *kept, size_t *offsets) {
    if (F < 1 || F > kStMaxF || !kept) return 0;
    static const size_t width[GSR_STATION_FACE_ARRAYS] = {3, 6, 1, 3, 1, 1};  // 4-byte words per row
    size_t off = 0;
    for (int f = 0; f < F; f++) {
        const size_t P = kept[f] > 0 ? (size_t)kept[f] : 0;
        for (int a = 0; a < GSR_STATION_FACE_ARRAYS; a++) {
            if (offsets) offsets[(size_t)f * GSR_STATION_FACE_ARRAYS + a] = off;
            off = (off + 4 * width[a] * P + 255) & ~(size_t)255;
        }
    }
    return off;
}

int gsr_station_set_profiling(int enable) { return g_st_profile.exchange(enable ? 1 : 0); }

int gsr_station_stage_times_ms(float *out, int max_stages) {
    if (!out || max_stages <= 0 || !t_ev_valid) return 0;
    if (hipEventSynchronize(t_ev[kStStages]) != hipSuccess) return 0;
    const int n = std::min(max_stages, kStStages);
    for (int k = 0; k < n; k++)
        if (hipEventElapsedTime(out + k, t_ev[k], t_ev[k + 1]) != hipSuccess) out[k] = 0.f;
    return n;
}

int gsr_rasterize_station_forward(gsr_resize_fn geom_buffer, gsr_resize_fn binning_buffer,
                                  gsr_resize_fn image_buffer, gsr_resize_fn rows_buffer, void *resize_ctx,
                                  void *scratch, size_t scratch_bytes, int64_t N, int D, int M,
                                  const float *means3D, const float *shs, const float *opacities,
                                  const float *scales, const float *rotations, const int *render_indices,
                                  const int *parent_indices, const float *interpolation_weights, int R, int F,
                                  const float *viewmatrices, const float *projmatrices, const float *cam_pos,
                                  float tan_fovx, float tan_fovy, int width, int height, const float *background,
                                  float *out_color, float *out_invdepth, int *radii, int64_t *num_rendered,
                                  int64_t *rows_kept, int debug, void *stream) {
    const auto aligned16 = [](const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (F < 1) return fail_st(GSR_ERR_INVALID_ARGUMENT, "F must be >= 1");
    if (F > kStMaxF)
        return fail_st(GSR_ERR_INVALID_ARGUMENT, "F = " + std::to_string(F) + " exceeds GSR_STATION_MAX_FACES (" +
                                                     std::to_string(kStMaxF) + ")");
    if (!viewmatrices || !projmatrices || !cam_pos)
        return fail_st(GSR_ERR_INVALID_ARGUMENT, "NULL viewmatrices / projmatrices / cam_pos");
    if (!aligned16(viewmatrices) || !aligned16(projmatrices))
        return fail_st(GSR_ERR_INVALID_ARGUMENT, "viewmatrices / projmatrices must be 16-byte aligned");
    if (!num_rendered || !background || !out_color) return fail_st(GSR_ERR_INVALID_ARGUMENT, "NULL required pointer");
    if (!geom_buffer || !binning_buffer || !image_buffer || !rows_buffer)
        return fail_st(GSR_ERR_INVALID_ARGUMENT, "resize callbacks must be non-NULL");
    for (int f = 0; f < F; f++) {
        num_rendered[f] = 0;
        if (rows_kept) rows_kept[f] = 0;
    }
    if (R < 0) return fail_st(GSR_ERR_INVALID_ARGUMENT, "R must be >= 0");
    if (width <= 0 || height <= 0) return fail_st(GSR_ERR_INVALID_ARGUMENT, "image size must be positive");
    if (D < 0 || D > 3) return fail_st(GSR_ERR_INVALID_ARGUMENT, "sh degree out of range (0..3)");
    if (M != 16) return fail_st(GSR_ERR_INVALID_ARGUMENT, "needs M = 16 SH coefficients per row");
    if (R > 0) {
        if (N <= 0 || N > INT32_MAX) return fail_st(GSR_ERR_INVALID_ARGUMENT, "N out of range for a non-empty cut");
        if (!means3D || !shs || !opacities || !scales || !rotations)
            return fail_st(GSR_ERR_INVALID_ARGUMENT, "NULL hierarchy rows (means3D, shs, opacities, scales, rotations)");
        if (!aligned16(shs) || !aligned16(rotations))
            return fail_st(GSR_ERR_INVALID_ARGUMENT, "shs and rotations must be 16-byte aligned");
        if (!render_indices || !parent_indices || !interpolation_weights)
            return fail_st(GSR_ERR_INVALID_ARGUMENT, "NULL render_indices / parent_indices / interpolation_weights");
        if (!radii) return fail_st(GSR_ERR_INVALID_ARGUMENT, "NULL radii");
        if (!scratch || scratch_bytes < gsr_station_rows_scratch_bytes(R, F))
            return fail_st(GSR_ERR_INVALID_ARGUMENT, "scratch too small (gsr_station_rows_scratch_bytes)");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t npix = (size_t)width * (size_t)height;

    StView v{viewmatrices, projmatrices, F, width, height, (width + kTile - 1) / kTile, (height + kTile - 1) / kTile,
             tan_fovx, tan_fovy, (float)width / (2.0f * tan_fovx), (float)height / (2.0f * tan_fovy)};
    StScratch sc{};
    StFaces faces{};
    int64_t kept[kStMaxF] = {};
    const int64_t ntiles = st_tiles(std::max(R, 1)), ngroups = st_groups(ntiles);
    st_mark(0, s);
    if (R > 0) {
        (void)st_carve(R, F, &sc, reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255));
        hipError_t e = hipMemsetAsync(radii, 0, sizeof(int) * (size_t)F * (size_t)R, s);
        if (e == hipSuccess) e = hipMemsetAsync(sc.grp, 0, sizeof(uint32_t) * (size_t)F * (size_t)ngroups, s);
        if (e == hipSuccess) {
            const CutRef cut{render_indices, parent_indices, interpolation_weights, N};
            hipLaunchKernelGGL(station_rows_kernel, dim3((unsigned)ntiles), dim3(kStThreads), 0, s, R, D, means3D, scales,
                               rotations, opacities, shs, cam_pos, cut, v, sc, ntiles, ngroups);
            hipLaunchKernelGGL(station_scan_kernel, dim3(1), dim3(kStMaxF * kWave), 0, s, F, ngroups, sc);
            e = hipGetLastError();
        }
        st_mark(1, s);
        uint32_t counts[kStMaxF] = {};
        if (e == hipSuccess) e = hipMemcpyAsync(counts, sc.counts, sizeof(uint32_t) * (size_t)F, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail_st(GSR_ERR_DEVICE, std::string("station_rows: ") + hipGetErrorString(e));
        int64_t total = 0;
        for (int f = 0; f < F; f++) {
            kept[f] = (int64_t)counts[f];
            if (kept[f] > R) return fail_st(GSR_ERR_DEVICE, "station_rows: a face's count exceeds the cut");
            total += kept[f];
            if (rows_kept) rows_kept[f] = kept[f];
        }
        if (total > 0) {
            size_t offs[kStMaxF * GSR_STATION_FACE_ARRAYS];
            const size_t bytes = gsr_station_rows_layout(F, kept, offs);
            char *base = static_cast<char *>(rows_buffer(resize_ctx, bytes));
            if (!base) return fail_st(GSR_ERR_ALLOCATION, "rows buffer allocation failed");
            if (reinterpret_cast<uintptr_t>(base) % 16 != 0)
                return fail_st(GSR_ERR_INVALID_ARGUMENT, "the rows buffer must be 16-byte aligned");
            for (int f = 0; f < F; f++) {
                const size_t *o = offs + (size_t)f * GSR_STATION_FACE_ARRAYS;
                faces.means[f] = reinterpret_cast<float *>(base + o[0]);
                faces.cov[f] = reinterpret_cast<float *>(base + o[1]);
                faces.opac[f] = reinterpret_cast<float *>(base + o[2]);
                faces.rgb[f] = reinterpret_cast<float *>(base + o[3]);
                faces.src[f] = reinterpret_cast<int *>(base + o[4]);
                faces.radii[f] = reinterpret_cast<int *>(base + o[5]);
                faces.kept[f] = kept[f];
            }
            hipLaunchKernelGGL(station_compact_kernel, dim3((unsigned)ntiles), dim3(kStThreads), 0, s, R, F, sc, faces,
                               ntiles, ngroups);
            if (int rc = launched("gsr_rasterize_station_forward (station_compact)")) return rc;
        }
    } else {
        st_mark(1, s);
    }
    st_mark(2, s);
    for (int f = 0; f < F; f++) {
        const int P = (int)kept[f];
        const int rc = gsr_rasterize_forward_ex(
            geom_buffer, binning_buffer, image_buffer, resize_ctx, P, 0, 0, background, width, height, faces.means[f],
            nullptr, faces.rgb[f], faces.opac[f], nullptr, 1.0f, nullptr, faces.cov[f], viewmatrices + 16 * f,
            projmatrices + 16 * f, cam_pos, tan_fovx, tan_fovy, 0, out_color + (size_t)f * 3 * npix,
            out_invdepth ? out_invdepth + (size_t)f * npix : nullptr, faces.radii[f], nullptr, nullptr, nullptr, nullptr,
            0, debug, stream, num_rendered + f, GSR_FWD_NO_BACKWARD);
        if (rc) return rc;  // the forward's message stands
    }
    st_mark(3, s);
    int64_t most = 0;
    for (int f = 0; f < F; f++) most = std::max(most, kept[f]);
    if (most > 0)
        hipLaunchKernelGGL(station_scatter_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)F), dim3(256), 0, s, R,
                           faces, radii);
    st_mark(4, s);
    return launched("gsr_rasterize_station_forward");
}

}  // extern "C"
