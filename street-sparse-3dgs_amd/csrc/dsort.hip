// dsort.hip -- the depth order of the P Gaussians: a stable LSD radix sort
// of the 32-bit depth keys in 9-bit digits, with the tile-count scan and the depth-order gather
// fused in.  A frame whose visible depths fit a 27-bit window above the near plane is sorted in
// three passes; any other frame takes a fourth pass of the same kernel.
//
// Upstream sorts K (tile << 32 | depth bits) keys; this build sorts only the P depth keys
// (binning.hip derives every tile's (depth, id) list from this order) and does it with its own
// onesweep-style kernels instead of a library sort: at P ~ 1M the library's per-pass launches,
// memsets and lookback resets cost ~0.17 ms for ~8 MB of data movement per pass.
//
// Sort key.  gs.dkey and the key ping-pong array hold the raw fp32 depth bits (0xFFFFFFFF when
// culled), which binning.hip's local sort and the debug snapshot read; the subtraction below happens
// in registers, one VALU per key and pass.  The kernels sort by r = key - kKeyBase, kKeyBase = bits(0.2f), the preprocess's near plane -- no
// visible key is below it, positive fp32 bit patterns order like integers, so r keeps the order
// and the ties.  Digits 0-2 are r's bits [0, 27) (r taken modulo 2^32); digit 3 is
// (r >> 27) + (key >= kKeyBase ? 32 : 0), which orders any 32-bit key (one below the base wraps
// to a large r and is put in front by the missing 32), so the four digits sort arbitrary keys
// (tools/dsort_bench.hip feeds its own).  A frame is narrow when digit 3 is 32 for every visible
// key, i.e. every depth is below 0.2 * 2^16 = 13107.2; three passes then order it, and the same
// histograms serve the narrow and the wide frame.
//
//   dsort_upsweep   one read of the keys and tile counts by <= 128 workgroups: each one's four
//                   9-bit digit histograms (LDS, written out as one row -- no global atomics on a
//                   few hot lines) and tiles_touched sums; a key whose digit 3 is not 32 sets the
//                   control word `wide`.  The last workgroup to finish adds up K and stores `wide`
//                   and then K straight into pinned host memory, so the host sizes the binning
//                   buffer while the sort passes still run.
//   dsort_pass x4   per 8192-key tile (1024 threads, 8 keys each, wave-striped so that wave, item,
//                   lane order is the input order): the pass's global digit bases from the per-tile
//                   histograms, match-mask ranking (9 ballots per key) into per-wave LDS counters,
//                   block digit scan, decoupled lookback per digit over the preceding tiles (16
//                   predecessors per round trip), the tile reordered through LDS by digit,
//                   coalesced stores.  Pass 0 takes the Gaussian index as the value (no id array)
//                   and writes the Gaussian-major record offsets (exclusive scan of tiles_touched
//                   in index order, gs.offsets).  The last pass writes the order and each slot's
//                   tile rect and no keys: that is pass 2 of a narrow frame (pass 3 then returns at
//                   once) and pass 3 of a wide one; the kernels read `wide` from the device, the
//                   host enqueues the four launches before it knows anything about the frame.
//
// Stability: every pass ranks equal digits in input order, so equal depth bits keep Gaussian-id
// order -- upstream's key (depth bits, then the stable sort's index order).  Culled Gaussians
// carry key 0xFFFFFFFF and end up behind every visible one.
//
// Control words: [0, kCtlHead) tickets / counters, then the lookback status of every pass
// (count | flag << 30) -- zeroed by the preprocess kernel, which runs first on the same stream --
// then the upsweep's tile offsets, workgroup totals and histogram rows (fully written by it).
#include "gsr_launch.h"

namespace gsr {

namespace {

constexpr int kDsThreads = 1024;
constexpr int kDsWaves = kDsThreads / kWave;
constexpr int kDsItems = 8;
constexpr int kDsTile = kDsThreads * kDsItems;
constexpr int kDigitBits = 9;
constexpr int kRadix = 1 << kDigitBits;
constexpr int kPasses = 4;
constexpr int kLookWin = 16;
constexpr int kMaxResident = 240;  // tiles numbered by blockIdx.x up to this many (< CUs)
constexpr uint32_t kKeyBase = 0x3E4CCCCDu;  // bits(0.2f): the preprocess culls z <= 0.2f
constexpr uint32_t kTopNarrow = 32u;        // digit 3 of a key in [kKeyBase, kKeyBase + 2^27)

// control word offsets
constexpr int kCtlTicket = 0;  // [p] pass p
constexpr int kCtlDone = 4;    // upsweep tiles finished
constexpr int kCtlK = 5;       // sum of tiles_touched
constexpr int kCtlErr = 6;     // set when a bounded spin gave up (never expected)
constexpr int kCtlAux = 7;     // per-frame counter lent to the binning (sb_colscan's last-workgroup count)
constexpr int kCtlMaxSB = 8;   // local-sort frames: the longest SB list (sb_colscan)
constexpr int kCtlFwdReady = 9;  // the forward split's queue released by tile_order (workers launched ahead)
constexpr int kCtlSpare = 10;    // [2]: unused (the words after it keep their places)
constexpr int kCtlCulled = 12;   // culled Gaussians (key 0xFFFFFFFF): the depth order's last P - visible slots
constexpr int kCtlLive = 13;     // [2]: the backward's live-row list length and finished workgroups (backward.hip;
                                 // zeroed again by grad_live_kernel's last workgroup)
constexpr int kCtlWide = 15;     // a visible key lies outside [kKeyBase, kKeyBase + 2^27): four passes
constexpr int kCtlHead = 16;
// The upsweep runs at most kUpMax workgroups, each over tpb consecutive tiles, so that a pass
// reduces at most kUpMax histogram rows: a thread takes kRowVec digits (one 16-B load) of every
// kRowSets-th row, kRowLoads loads in groups of kRowGroup.
constexpr int kUpMax = 128;
constexpr int kRowVec = 4;
constexpr int kRowSets = kDsThreads / (kRadix / kRowVec);
constexpr int kRowLoads = kUpMax / kRowSets;
constexpr int kRowGroup = 8;
__host__ __device__ inline int up_tpb(int nb) { return (nb + kUpMax - 1) / kUpMax; }
__host__ __device__ inline int up_blocks(int nb) { return (nb + up_tpb(nb) - 1) / up_tpb(nb); }
__host__ __device__ inline size_t ctl_status(int nb, int p) { return kCtlHead + (size_t)p * nb * kRadix; }
__host__ __device__ inline size_t ctl_zero_words(int nb) { return ctl_status(nb, kPasses); }
__host__ __device__ inline size_t ctl_bex(int nb) { return ctl_zero_words(nb); }              // [nb]
__host__ __device__ inline size_t ctl_btot(int nb) { return ctl_bex(nb) + nb; }               // [kUpMax]
__host__ __device__ inline size_t ctl_blkhist(int nb) { return (ctl_btot(nb) + kUpMax + 63) / 64 * 64; }
__host__ __device__ inline size_t ctl_words(int nb) { return ctl_blkhist(nb) + (size_t)kUpMax * kPasses * kRadix; }
constexpr int kSpinLimit = 1 << 20;  // ~1 s of polling: a predecessor tile can never take that long

// Diagnostic build only (tools/dsort_bench.hip): per-workgroup phase stamps of s_memrealtime
// (100 MHz) into g_ds_trace[(kernel * 4096 + block) * 8 + slot].
#ifdef GSR_DS_TRACE
__device__ uint64_t *g_ds_trace;
#define DS_STAMP(kern, slot)                                                                          \
    do {                                                                                              \
        if (threadIdx.x == 0) {                                                                       \
            const uint64_t t_ = __builtin_amdgcn_s_memrealtime();                                     \
            __builtin_amdgcn_s_waitcnt(0xC07F);                                                       \
            if (blockIdx.x < 4096) g_ds_trace[((size_t)(kern) * 4096 + blockIdx.x) * 8 + (slot)] = t_; \
        }                                                                                             \
    } while (0)
#else
#define DS_STAMP(kern, slot) \
    do {                     \
    } while (0)
#endif
#ifdef GSR_DS_TRACE
#define DS_STAMP_AFTER(kern, slot, x)            \
    do {                                         \
        asm volatile("s_waitcnt vmcnt(0)" ::"v"(x)); \
        DS_STAMP(kern, slot);                    \
    } while (0)
#else
#define DS_STAMP_AFTER(kern, slot, x) DS_STAMP(kern, slot)
#endif

// Rect carry: with 4-B rects, the tile rect travels with the Gaussian id through the
// passes (read coalesced by pass 0 in index order, ping-ponged through the idle rect8 array), so
// the last pass stores it instead of gathering rect4[id] -- one random 64-B line per Gaussian.

constexpr uint32_t kFlagAgg = 1u << 30, kFlagInc = 2u << 30, kCountMask = (1u << 30) - 1u;

__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// digit p of a key (file header): the near-plane-relative bits, digit 3 made total over all keys
template <int p>
__device__ __forceinline__ uint32_t digit_of(uint32_t key) {
    const uint32_t r = key - kKeyBase;
    if (p < kPasses - 1) return (r >> (kDigitBits * p)) & (uint32_t)(kRadix - 1);
    return (r >> (kDigitBits * p)) + (key >= kKeyBase ? kTopNarrow : 0u);
}

// lanes of `valid` whose 9-bit digit equals this lane's
__device__ __forceinline__ uint64_t match_digit(uint32_t d, uint64_t valid) {
    uint64_t m = valid;
#pragma unroll
    for (int b = 0; b < kDigitBits; b++) {
        // bit b of d spread over the word: the lanes that agree with this one are ~(ballot ^ spread)
        const uint32_t spread = (uint32_t)((int32_t)(d << (31 - b)) >> 31);
        const uint64_t bb = __ballot(spread != 0u);
        m &= ~(bb ^ ((uint64_t)spread << 32 | spread));
    }
    return m;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Exclusive scan of the kRadix LDS counters in place by one wave (8 per lane); returns the total.
__device__ __forceinline__ uint32_t scan_radix_wave(uint32_t *a, int lane) {
    constexpr int kPer = kRadix / kWave;
    uint32_t x[kPer], s = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        x[k] = a[kPer * lane + k];
        s += x[k];
    }
    const uint32_t incl = wave_incl_scan(s, lane);
    uint32_t e = incl - s;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        a[kPer * lane + k] = e;
        e += x[k];
    }
    return (uint32_t)__shfl((int)incl, 63, 64);
}

// Per workgroup u: tiles [u tpb, (u + 1) tpb): the digit histograms of all passes over its tiles
// (one LDS add per key and digit 0-2; conflicts only where a wave's digits coincide) -> histogram
// row u; the tiles_touched sum of each tile -> its exclusive offset inside the workgroup (bex) and
// the workgroup total (btot); K = the sum of the totals, stored by the last workgroup to finish.
__global__ __launch_bounds__(kDsThreads) void dsort_upsweep_kernel(int P, int nb, const uint32_t *__restrict__ keys,
                                                                    const uint32_t *__restrict__ tiles,
                                                                    uint32_t *__restrict__ ctl,
                                                                    uint32_t *__restrict__ host_K,
                                                                    uint32_t *__restrict__ host_wide) {
    GSR_KS(kKsUpsweep);
    constexpr int kMidCopies = 16;
    __shared__ uint32_t s_hist[kPasses * kRadix];
    // digit 2 (r's bits 18-26: the exponent's low bits and the top of the mantissa) repeats inside a
    // wave when neighbouring rows have similar depths (rows in spatial order,
    // gs_train.chunk.reorder_rows: 64-way conflicts on an unreplicated counter, config-3 upsweep
    // 15.5 -> 25.0 us per call): its counters are replicated 16x (lane & 15 picks the copy).
    // Digit 3 is one value for every key of a narrow frame: those keys are counted by a ballot and
    // only the others (a wide frame's far rows) add into LDS.
    __shared__ uint32_t s_mid[kMidCopies][kRadix];
    __shared__ uint32_t s_wsum[kDsWaves];
    __shared__ uint32_t s_cull, s_far;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int u = blockIdx.x, tpb = up_tpb(nb);
    DS_STAMP(0, 0);
#pragma unroll
    for (int k = 0; k < kPasses * kRadix / kDsThreads; k++) s_hist[t + k * kDsThreads] = 0u;
    if (t == 0) s_cull = s_far = 0u;
#pragma unroll
    for (int k = 0; k < kMidCopies * kRadix / kDsThreads; k++) (&s_mid[0][0])[t + k * kDsThreads] = 0u;
    __syncthreads();
    uint32_t run = 0;  // thread 0: tiles_touched of the workgroup's earlier tiles
    uint32_t culled = 0;  // this wave's culled keys (wave-uniform)
    uint32_t near = 0;    // this wave's keys with digit 3 == kTopNarrow (wave-uniform)
    bool far = false;     // this wave met a visible key outside the window (wave-uniform)
    const int v1 = min(nb, (u + 1) * tpb);
    for (int v = u * tpb; v < v1; v++) {
        const size_t base = (size_t)v * kDsTile + (size_t)w * kDsItems * kWave;
        uint32_t key[kDsItems], tl[kDsItems];
#pragma unroll
        for (int k = 0; k < kDsItems; k++) {
            const size_t e = base + (size_t)k * kWave + lane;
            key[k] = e < (size_t)P ? keys[e] : 0u;
            tl[k] = e < (size_t)P ? tiles[e] : 0u;
        }
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kDsItems; k++) {
            const size_t e = base + (size_t)k * kWave + lane;
            // culled Gaussians (key 0xFFFFFFFF) are left out of the sort: counted by a ballot (LDS
            // atomics would all hit one word -- 70% of a street view's rows lie outside its 90-degree
            // frustum: config-3 upsweep 59 us per call at 3M rows, r05i), and dropped by pass 0
            const bool cull = e < (size_t)P && key[k] == 0xFFFFFFFFu;
            const bool vis = e < (size_t)P && !cull;
            const uint32_t top = digit_of<3>(key[k]);
            const uint64_t nearm = __ballot(vis && top == kTopNarrow);
            culled += (uint32_t)__popcll(__ballot(cull));
            near += (uint32_t)__popcll(nearm);
            if (vis) {
                atomicAdd(&s_hist[digit_of<0>(key[k])], 1u);
                atomicAdd(&s_hist[kRadix + digit_of<1>(key[k])], 1u);
                atomicAdd(&s_mid[lane & (kMidCopies - 1)][digit_of<2>(key[k])], 1u);
                if (top != kTopNarrow) atomicAdd(&s_hist[3 * kRadix + top], 1u);
            }
            far = far || __ballot(vis) != nearm;
            sum += tl[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o, 64);
        if (lane == 0) s_wsum[w] = sum;
        __syncthreads();
        if (t == 0) {
            ctl[ctl_bex(nb) + v] = run;
#pragma unroll
            for (int k = 0; k < kDsWaves; k++) run += s_wsum[k];
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (culled) atomicAdd(&s_cull, culled);
        if (near) atomicAdd(&s_hist[3 * kRadix + kTopNarrow], near);
        if (far) s_far = 1u;
    }
    __syncthreads();
    DS_STAMP(0, 1);
#pragma unroll
    for (int k = 0; k < kPasses * kRadix / kDsThreads; k++) {
        const int i = t + k * kDsThreads;
        uint32_t hv = s_hist[i];
        if (i >= 2 * kRadix && i < 3 * kRadix) {
#pragma unroll
            for (int c = 0; c < kMidCopies; c++) hv += s_mid[c][i - 2 * kRadix];
        }
        ctl[ctl_blkhist(nb) + (size_t)u * kPasses * kRadix + i] = hv;
    }
    if (t == 0) {
        ctl[ctl_btot(nb) + u] = run;
        __hip_atomic_fetch_add(&ctl[kCtlK], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s_cull) __hip_atomic_fetch_add(&ctl[kCtlCulled], s_cull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s_far) __hip_atomic_fetch_or(&ctl[kCtlWide], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t done = __hip_atomic_fetch_add(&ctl[kCtlDone], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (done == (uint32_t)gridDim.x - 1u && host_K) {
            const uint32_t K = ld_agent(&ctl[kCtlK]);
            // `wide` first: the host reads it once it has seen K
            if (host_wide) __hip_atomic_store(host_wide, ld_agent(&ctl[kCtlWide]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_K, K, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    DS_STAMP(0, 2);
}

// One pass over digit kPass.  Passes 0 and 1 write (kout, vout, rout).  Pass 2 is the last pass of a
// narrow frame (control word `wide` clear) and then writes (order, drect) and no keys; in a wide frame
// it writes (kout, vout, rout) like the passes before it.  Pass 3 returns at once in a narrow frame
// and is the last pass of a wide one.
template <int kPass>
__global__ __launch_bounds__(kDsThreads) void dsort_pass_kernel(int P, int nb, const uint32_t *__restrict__ kin,
                                                                 uint32_t *__restrict__ kout,
                                                                 const uint32_t *__restrict__ vin,
                                                                 uint32_t *__restrict__ vout,
                                                                 uint32_t *__restrict__ order, uint32_t *__restrict__ ctl,
                                                                 uint32_t *__restrict__ offsets,
                                                                 const uint32_t *__restrict__ tiles,
                                                                 const uint2 *__restrict__ rect8,
                                                                 const uint32_t *__restrict__ rect4,
                                                                 uint2 *__restrict__ drect,
                                                                 const uint32_t *__restrict__ rin,
                                                                 uint32_t *__restrict__ rout,
                                                                 uint32_t *__restrict__ host_err) {
    GSR_KS(kKsPass0 + kPass);
    constexpr bool kFirst = kPass == 0;
    const bool wide = kPass >= 2 && ctl[kCtlWide] != 0u;  // the upsweep's, complete before any pass starts
    if (kPass == kPasses - 1 && !wide) return;            // pass 2 was the last
    const bool last = kPass == kPasses - 1 || (kPass == kPasses - 2 && !wide);
    // rect carry: pass 0 reads rect4 itself, the others rin; the last pass stores into drect's 4-B
    // form, the others into rout
    const bool carry = rect4 != nullptr;
    __shared__ uint32_t s_key[kDsTile];
    __shared__ uint32_t s_val[kDsTile];
    __shared__ uint32_t s_rc[kDsTile];  // carried rects
    __shared__ uint32_t s_wh[kDsWaves][kRadix];  // per-wave digit counts -> exclusive prefix over waves
    __shared__ __attribute__((aligned(16))) uint32_t s_gb[kRowSets][kRadix];  // global digit base (partial sums, then [0] scanned)
    __shared__ uint32_t s_bex[kRadix];           // tile-local digit base
    __shared__ uint32_t s_dst[kRadix];           // global slot of tile-local position 0 of each digit
    __shared__ uint32_t s_wsum[kDsWaves];
    __shared__ uint32_t s_v, s_pre, s_nsort;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    DS_STAMP(1 + kPass, 0);
#pragma unroll
    for (int k = 0; k < kDsWaves * kRadix / kDsThreads; k++) (&s_wh[0][0])[t + k * kDsThreads] = 0u;
    // Tile numbering: up to kMaxResident tiles every workgroup can be resident at once (one per CU;
    // nothing else this build runs holds a CU indefinitely), so a tile waiting on lower-numbered
    // ones can always be overtaken and blockIdx.x is the tile; above that, tiles are numbered in
    // start order by a ticket, so a tile only ever waits on tiles that are already running.
    // The histogram-row loads (kRowLoads 16-B loads per thread: digits 4 (t & 127) .. + 3 of rows
    // (t >> 7) + 8 q) go out in groups of kRowGroup so the 128-VGPR budget holds: the first group is
    // issued here; in the middle of the ranking it is summed and its registers take the next group,
    // which is summed after the ranking.
    const int nbu = up_blocks(nb);
    const uint4 *bh = reinterpret_cast<const uint4 *>(ctl + ctl_blkhist(nb) + kPass * kRadix) + (t & (kRadix / kRowVec - 1));
    const auto row = [&](int q) {
        const int j = t / (kRadix / kRowVec) + kRowSets * q;
        return j < nbu ? bh[(size_t)j * (kPasses * kRadix / kRowVec)] : make_uint4(0u, 0u, 0u, 0u);
    };
    constexpr int kRowGroups = kRowLoads / kRowGroup, kRowEvery = kDsItems / kRowGroups;
    static_assert(kRowLoads % kRowGroup == 0 && kDsItems % kRowGroups == 0, "row groups spread over the ranked items");
    uint4 h[kRowGroup], gsum = make_uint4(0u, 0u, 0u, 0u);
    const auto sum_rows = [&]() {
#pragma unroll
        for (int q = 0; q < kRowGroup; q++) {
            gsum.x += h[q].x;
            gsum.y += h[q].y;
            gsum.z += h[q].z;
            gsum.w += h[q].w;
        }
    };
#pragma unroll
    for (int q = 0; q < kRowGroup; q++) h[q] = row(q);
    uint32_t v = blockIdx.x;
    if (nb > kMaxResident) {
        if (t == 0) s_v = atomicAdd(&ctl[kCtlTicket + kPass], 1u);
        __syncthreads();
        v = s_v;
    } else {
        __builtin_amdgcn_s_waitcnt(0xc07f);  // s_wh zeroed: LDS only (the row loads stay in flight)
        __builtin_amdgcn_s_barrier();
    }
    // Culled Gaussians (key 0xFFFFFFFF, no tiles) are not sorted: pass 0 reads every key in index
    // order and drops them, so the later passes run over the Pv = P - culled visible keys only and the
    // depth order's slots [Pv, P) are never written (nothing reads them: the binning stops at Pv).
    const size_t Pn = kFirst ? (size_t)P : (size_t)P - min((size_t)ctl[kCtlCulled], (size_t)P);
    const uint32_t nbv = (uint32_t)((Pn + kDsTile - 1) / kDsTile);
    if (v >= nbv) return;  // control words not zeroed past nb; tiles past the visible keys: nothing to do
    DS_STAMP(1 + kPass, 5);
    const int wbase = w * kDsItems * kWave;
    const size_t tile0 = (size_t)v * kDsTile;
    const int n = (int)min((size_t)kDsTile, Pn - tile0);
    uint32_t key[kDsItems], val[kDsItems], tl[kDsItems];
#pragma unroll
    for (int k = 0; k < kDsItems; k++) {
        const int i = wbase + k * kWave + lane;
        const bool valid = i < n;
        key[k] = valid ? kin[tile0 + i] : 0xFFFFFFFFu;
        val[k] = (!kFirst && valid) ? vin[tile0 + i] : 0u;  // pass 0: the index, formed where it is stored
        tl[k] = (kFirst && valid) ? tiles[tile0 + i] : 0u;
    }
    DS_STAMP_AFTER(1 + kPass, 6, key[kDsItems - 1] + val[kDsItems - 1]);
    if (kFirst) {
        // record offsets: the totals of the earlier upsweep workgroups + this tile's offset inside
        // its workgroup, then the in-tile order
        if (w == 0) {
            const int u = (int)v / up_tpb(nb);
            uint32_t c = 0;
#pragma unroll
            for (int q = 0; q < kUpMax / kWave; q++) c += lane + q * kWave < u ? ctl[ctl_btot(nb) + lane + q * kWave] : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
            if (lane == 0) s_pre = c + ctl[ctl_bex(nb) + v];
        }
        uint32_t run = 0;
#pragma unroll
        for (int k = 0; k < kDsItems; k++) {
            const uint32_t incl = wave_incl_scan(tl[k], lane);
            // exclusive offset inside the wave's 512 keys, parked in this thread's own slot of s_key
            // (idle until the tile is reordered, two barriers on) to keep it out of the ranking's registers
            s_key[wbase + k * kWave + lane] = run + incl - tl[k];
            run += (uint32_t)__shfl((int)incl, 63, 64);
        }
        if (lane == 0) s_wsum[w] = run;
    }
    // ranks: within the wave, equal digits in (item, lane) order (9 ballots per key)
    uint32_t rk[kDsItems];
#pragma unroll
    for (int k = 0; k < kDsItems; k++) {
        const bool valid = wbase + k * kWave + lane < n && key[k] != 0xFFFFFFFFu;
        const uint32_t d = digit_of<kPass>(key[k]) & (uint32_t)(kRadix - 1);
        const uint64_t m = match_digit(d, __ballot(valid));
        const uint32_t b = below(m);
        const uint32_t old = s_wh[w][d];
        if (valid && b == 0u) s_wh[w][d] = old + (uint32_t)__popcll(m);
        rk[k] = old + b;
        // global digit base: column kPass of the upsweep's histogram rows, kRowSets strided partial sums
        if ((k + 1) % kRowEvery == 0 && (k + 1) / kRowEvery < kRowGroups) {
            asm volatile("" ::: "memory");  // keeps the compiler from hoisting these loads to the first group
            sum_rows();
#pragma unroll
            for (int q = 0; q < kRowGroup; q++) h[q] = row((k + 1) / kRowEvery * kRowGroup + q);
        }
    }
    sum_rows();
    *reinterpret_cast<uint4 *>(&s_gb[t / (kRadix / kRowVec)][kRowVec * (t & (kRadix / kRowVec - 1))]) = gsum;
    // the carried rects are loaded once the histogram rows are summed (register pressure); they are
    // not needed before the tile goes through LDS, two barriers on
    uint32_t rc[kDsItems];
    if (carry) {
        const uint32_t *rsrc = kFirst ? rect4 : rin;
#pragma unroll
        for (int k = 0; k < kDsItems; k++) {
            const int i = wbase + k * kWave + lane;
            rc[k] = i < n ? rsrc[tile0 + i] : 0u;
        }
    }
    __syncthreads();
    DS_STAMP(1 + kPass, 1);
    if (kFirst) {
        uint32_t pre = s_pre;
        for (int k = 0; k < w; k++) pre += s_wsum[k];
#pragma unroll
        for (int k = 0; k < kDsItems; k++) {
            const int i = wbase + k * kWave + lane;
            if (i < n) offsets[tile0 + i] = pre + s_key[i];
        }
    }
    uint32_t cnt = 0;
    if (t < kRadix) {
#pragma unroll
        for (int ww = 0; ww < kDsWaves; ww++) {
            const uint32_t c = s_wh[ww][t];
            s_wh[ww][t] = cnt;
            cnt += c;
        }
        uint32_t *st = ctl + ctl_status(nb, kPass);
        st_agent(&st[(size_t)v * kRadix + t], (v == 0 ? kFlagInc : kFlagAgg) | cnt);
        s_bex[t] = cnt;
        uint32_t gb = s_gb[0][t];
#pragma unroll
        for (int q = 1; q < kRowSets; q++) gb += s_gb[q][t];
        s_gb[0][t] = gb;
    }
    __syncthreads();
    if (w == 0) {
        const uint32_t nv = scan_radix_wave(s_bex, lane);  // the tile's sorted (visible) keys
        if (lane == 0) s_nsort = nv;
    }
    if (w == 1) (void)scan_radix_wave(s_gb[0], lane);
    __syncthreads();
    const int nsort = (int)s_nsort;
    DS_STAMP(1 + kPass, 2);
    // the tile in digit order, through LDS (the item indices recomputed from an opaque copy of the
    // wave's base: kept live since the loads, they cost pass 0 eight registers and a spill)
    int wb = wbase + lane;
    asm volatile("" : "+v"(wb));
#pragma unroll
    for (int k = 0; k < kDsItems; k++) {
        const int i = wb + k * kWave;
        if (i < n && key[k] != 0xFFFFFFFFu) {
            const uint32_t d = digit_of<kPass>(key[k]) & (uint32_t)(kRadix - 1);
            const uint32_t lp = s_bex[d] + s_wh[w][d] + rk[k];
            s_key[lp] = key[k];
            s_val[lp] = kFirst ? (uint32_t)tile0 + (uint32_t)i : val[k];
            if (carry) s_rc[lp] = rc[k];
        }
    }
    DS_STAMP(1 + kPass, 7);
    if (t < kRadix) {
        // decoupled lookback for digit t over the preceding tiles, kLookWin status words per round
        // trip: add words from the nearest predecessor back until an inclusive one; a word not yet
        // published ends the round (re-polled next round)
        const uint32_t *st = ctl + ctl_status(nb, kPass);
        uint32_t excl = 0;
        int spins = 0;
        for (int j = (int)v - 1; j >= 0;) {
            uint32_t s[kLookWin];
#pragma unroll
            for (int q = 0; q < kLookWin; q++)
                s[q] = j - q >= 0 ? ld_agent(&st[(size_t)(j - q) * kRadix + t]) : kFlagInc;  // past tile 0: +0, stop
            int q = 0;
            bool inc = false;
#pragma unroll
            for (int qq = 0; qq < kLookWin; qq++) {
                const uint32_t f = s[qq] & ~kCountMask;
                if (q == qq && f != 0u && !inc) {
                    excl += s[qq] & kCountMask;
                    inc = f == kFlagInc;
                    q = qq + 1;
                }
            }
            if (inc) break;
            j -= q;
            if (q < kLookWin) {
                if (++spins > kSpinLimit) {
                    // never expected; made loud: render_fwd writes NaN pixels when this word is
                    // set, and the sticky host word fails the next library call on this thread
                    ctl[kCtlErr] = 1u;
                    if (host_err) __hip_atomic_store(host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (v > 0) st_agent(&ctl[ctl_status(nb, kPass) + (size_t)v * kRadix + t], kFlagInc | (excl + cnt));
        s_dst[t] = s_gb[0][t] + excl - s_bex[t];
    }
    __syncthreads();
    DS_STAMP(1 + kPass, 3);
    for (int i = t; i < nsort; i += kDsThreads) {
        const uint32_t k = s_key[i];
        const uint32_t j = s_dst[digit_of<kPass>(k) & (uint32_t)(kRadix - 1)] + (uint32_t)i;
        const uint32_t g = s_val[i];
        if (last) {
            order[j] = g;
            if (carry) reinterpret_cast<uint32_t *>(drect)[j] = s_rc[i];  // drect4_of(gs), carried
            else drect[j] = rect8[g];
        } else {
            kout[j] = k;
            vout[j] = g;
            if (carry) rout[j] = s_rc[i];
        }
    }
    DS_STAMP(1 + kPass, 4);
}

}  // namespace

int dsort_blocks(int P) { return (P + kDsTile - 1) / kDsTile; }

size_t dsort_ctrl_words(int P) { return ctl_words(dsort_blocks(P) > 0 ? dsort_blocks(P) : 1); }
size_t dsort_ctrl_zero_words(int P) { return ctl_zero_words(dsort_blocks(P) > 0 ? dsort_blocks(P) : 1); }

void launch_depth_sort(int P, const GeomState &gs, uint32_t *host_K, uint32_t *host_wide, uint32_t *host_err,
                       hipStream_t s, hipEvent_t k_ready) {
    if (P == 0) return;
    const int nb = dsort_blocks(P);
    hipLaunchKernelGGL(dsort_upsweep_kernel, dim3(up_blocks(nb)), dim3(kDsThreads), 0, s, P, nb, gs.dkey, gs.tiles,
                       gs.ctrl, host_K, host_wide);
    if (k_ready) (void)hipEventRecord(k_ready, s);
    // keys: dkey -> dkey_sorted -> dkey [-> dkey_sorted]; values: (index) -> ids -> ids2 -> order, in a
    // wide frame ids2 -> ids -> order; carried 4-B rects (rect4 set: rect8 is idle, two P-word
    // halves): rect4 -> A -> B -> drect, in a wide frame B -> A -> drect
    uint32_t *ra = reinterpret_cast<uint32_t *>(gs.rect8), *rb = ra + P;
    hipLaunchKernelGGL(dsort_pass_kernel<0>, dim3(nb), dim3(kDsThreads), 0, s, P, nb, gs.dkey, gs.dkey_sorted,
                       (const uint32_t *)nullptr, gs.ids, (uint32_t *)nullptr, gs.ctrl, gs.offsets, gs.tiles, gs.rect8,
                       gs.rect4, gs.drect, (const uint32_t *)nullptr, ra, host_err);
    hipLaunchKernelGGL(dsort_pass_kernel<1>, dim3(nb), dim3(kDsThreads), 0, s, P, nb, gs.dkey_sorted, gs.dkey, gs.ids,
                       gs.ids2, (uint32_t *)nullptr, gs.ctrl, gs.offsets, gs.tiles, gs.rect8, gs.rect4, gs.drect, ra,
                       rb, host_err);
    hipLaunchKernelGGL(dsort_pass_kernel<2>, dim3(nb), dim3(kDsThreads), 0, s, P, nb, gs.dkey, gs.dkey_sorted, gs.ids2,
                       gs.ids, gs.order, gs.ctrl, gs.offsets, gs.tiles, gs.rect8, gs.rect4, gs.drect, rb, ra, host_err);
    hipLaunchKernelGGL(dsort_pass_kernel<3>, dim3(nb), dim3(kDsThreads), 0, s, P, nb, gs.dkey_sorted,
                       (uint32_t *)nullptr, gs.ids, (uint32_t *)nullptr, gs.order, gs.ctrl, gs.offsets, gs.tiles,
                       gs.rect8, gs.rect4, gs.drect, ra, (uint32_t *)nullptr, host_err);
}

uint32_t *dsort_K_word(const GeomState &gs) { return gs.ctrl + kCtlK; }
uint32_t *dsort_err_word(const GeomState &gs) { return gs.ctrl + kCtlErr; }
uint32_t *dsort_aux_word(const GeomState &gs) { return gs.ctrl + kCtlAux; }
uint32_t *dsort_maxsb_word(const GeomState &gs) { return gs.ctrl + kCtlMaxSB; }
uint32_t *dsort_fwdready_word(const GeomState &gs) { return gs.ctrl + kCtlFwdReady; }
uint32_t *dsort_culled_word(const GeomState &gs) { return gs.ctrl + kCtlCulled; }
uint32_t *dsort_live_words(const GeomState &gs) { return gs.ctrl + kCtlLive; }
int dsort_head_words() { return kCtlHead; }

GSR_KSTAMP_READER(kstamp_read_dsort)

}  // namespace gsr
