// Full-reference PSNR / SSIM of two frame batches (spec PP-METRIC-1)
// on gfx950.
//
// New feature after p03 (the reference's image builds FFmpeg with libvmaf for
// this step; it has no code of its own).  Modelled on FFmpeg's vf_psnr and
// vf_ssim (x264's 4x4-block / 8x8-window SSIM at stride 4), parity unpinned.
//
//   SSE  = sum (a - b)^2 over every sample of a plane             (uint64)
//   SSIM = mean over the (bw-1)(bh-1) windows of 2x2 blocks of
//          (2 s1 s2 + c1)(2 covar + c2) / ((s1^2 + s2^2 + c1)(vars + c2))
//
// Layout: a workgroup (256 lanes, 4 waves) owns one unit = (frame, plane,
// column span, band of kBandBlocks block rows).  A lane takes 16 B of a row
// from each input (8 samples at 10 bits = 2 blocks, 16 at 8 bits = 4 blocks)
// through bounds-checked buffer loads and builds its 4x4 block sums
// (s1, s2, ss, s12) over four rows with v_dot2 / v_dot4.  The right-hand
// neighbour block comes from the next lane by a DPP wave shift; lane 63 of
// every wave is a halo lane that loads the 16 B right of the wave's span (a
// second read served by the caches) and owns nothing.  The horizontal block
// pairs of the previous block row stay in registers for the vertical half of
// the window, so a band reads every sample once plus one halo block row below.
// Samples outside the plane read as 0 in BOTH inputs (buffer range for rows
// and whole lanes, a mask for the lane straddling a ragged right edge), so
// the block identity ss - 2 s12 = sum (a - b)^2 gives the SSE of partial
// blocks too: the trailing pw & 3 columns and ph & 3 rows count in the SSE
// and never complete a window.
// Integers: block and window sums fit 32 bits (a window's ss <= 64 * 2 *
// 1023^2 < 2^28); vars and covar are formed in 64 bits (64 ss, s1^2 and
// 2 s1 s2 pass 2^31 at 10 bits) and every quotient is fp64.
// Reduction: lane -> wave (xor butterfly) -> workgroup (4 values through LDS
// in wave order) -> one partial per unit, no atomics; metrics_finalize adds a
// (frame, plane)'s partials in unit order: bit-reproducible.
// The piece loader, the plane descriptor, the edge mask and the butterfly are
// the analysis kernels' common ones (analysis_dev.hpp); the unaligned path
// reads uint16_t samples there, so 10-bit planes may sit on the 2-byte grid.
#include <algorithm>
#include <cstdlib>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kMetLaneBytes = 16;   // one load per lane and row
constexpr int kMetOwnLanes = 63;    // lanes of a wave that own blocks; lane 63 is the halo lane
constexpr int kMetWaves = 4;        // waves per workgroup
constexpr int kBandBlocks = 16;     // block rows per band (64 sample rows), plus one halo block row

struct MetPartial {
    uint64_t sse;
    double ssim;  // sum of the unit's window values
};

struct MetArgs {
    const uint8_t *ref[3], *dist[3];
    int64_t rls[3], rfs[3], dls[3], dfs[3];
    int pw[3], ph[3];
    int tiles_x[3], tile0[3];  // column spans of a plane; first tile of a plane within a frame
    int tiles;                 // tiles of one frame (all planes)
    int nk;                    // dist frames of this launch
    int identity;              // ref frame = dist frame (idx unused)
    int depth;
    MetPartial *part;          // [nk][tiles]
    int32_t idx[kFrameMap];
};

template <typename T>
__device__ inline uint32_t dot(uint32_t a, uint32_t b, uint32_t acc) {
    typedef uint16_t v2u16 __attribute__((ext_vector_type(2)));
    if constexpr (sizeof(T) == 2)
        return __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, a), __builtin_bit_cast(v2u16, b), acc, false);
    else
        return __builtin_amdgcn_udot4(a, b, acc, false);
}

// Four rows x 16 B of one input.
struct Quad {
    uint32_t w[4][4];
};

// Rows r0..r0+3 of a plane at the lane's byte column c (load_piece; rows >= ph
// read 0 through the descriptor's range or the clamp).
template <typename T, bool ALIGNED>
__device__ inline void load_quad(Quad &q, __amdgpu_buffer_rsrc_t rs, const uint8_t *base, int64_t ls, int r0, int ph,
                                 int c, int rb, bool in) {
#pragma unroll
    for (int j = 0; j < 4; ++j) load_piece<T, ALIGNED>(q.w[j], rs, base, ls, r0 + j, ph, c, rb, in);
}

// One window from its exact sums; widened before multiplying (PP-METRIC-1).
__device__ inline double ssim_window(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12, double c1, double c2) {
    const int64_t a = s1, b = s2;
    const int64_t sq = a * a + b * b;
    const int64_t vars = 64 * (int64_t)ss - sq;
    const int64_t covar = 64 * (int64_t)s12 - a * b;
    const double num = ((double)(2 * a * b) + c1) * ((double)(2 * covar) + c2);
    const double den = ((double)sq + c1) * ((double)vars + c2);
    return num / den;
}

template <typename T, bool ALIGNED, bool RAGGED>
__device__ __forceinline__ void metrics_unit(const MetArgs &a, int k, int tile, MetPartial *out) {
    constexpr int PX = kMetLaneBytes / sizeof(T);  // samples per lane and row
    constexpr int LB = PX / 4;                     // blocks per lane
    constexpr int DPB = 4 / LB;                    // dwords per block row of a block
    constexpr uint32_t kOnes = sizeof(T) == 2 ? 0x00010001u : 0x01010101u;
    __shared__ uint64_t s_sse[kMetWaves];
    __shared__ double s_ssim[kMetWaves];

    const int p = plane_of_tile(a.tile0, tile);
    const int t = tile - a.tile0[p];
    const int tx = t % a.tiles_x[p], band = t / a.tiles_x[p];
    const int pw = a.pw[p], ph = a.ph[p];
    const int bw = pw >> 2, bh = ph >> 2, bhc = (ph + 3) >> 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = ((tx * kMetWaves + wave) * kMetOwnLanes + lane) * PX;
    const bool own = lane < kMetOwnLanes;
    const int c0 = x >> 2;  // the lane's first block column
    const int b0 = band * kBandBlocks;

    const int rf = a.identity ? k : a.idx[k];
    const uint8_t *rbase = a.ref[p] + (int64_t)rf * a.rfs[p];
    const uint8_t *dbase = a.dist[p] + (int64_t)k * a.dfs[p];
    const int64_t rls = a.rls[p], dls = a.dls[p];
    const int rb = pw * (int)sizeof(T), xb = x * (int)sizeof(T);  // bytes of a row; the lane's byte column
    // ALIGNED: the column test is made once, here: a lane right of the plane has kOobOff as its
    // column (row * ls + kOobOff < 2^32 by the range check) and load_piece's per-row select folds
    const int c = ALIGNED && x >= pw ? kOobOff : xb;
    const bool in = ALIGNED || x < pw;
    const auto rrs = plane_rsrc<ALIGNED>(rbase, ph, rls, rb);
    const auto drs = plane_rsrc<ALIGNED>(dbase, ph, dls, rb);

    uint32_t mask[4] = {~0u, ~0u, ~0u, ~0u};  // RAGGED: the samples of the lane inside the plane
    mask_piece(mask, rb - xb);
    const double mx = (double)((1 << a.depth) - 1);
    const double c1 = .01 * .01 * mx * mx * 64.0, c2 = .03 * .03 * mx * mx * 64.0 * 63.0;

    uint32_t sse = 0;   // <= 16 block rows * 32 samples * 1023^2 < 2^32
    double acc = 0.0;
    uint32_t prev[LB][4];  // horizontal block pairs of the block row above
    Quad qa, qb;
    load_quad<T, ALIGNED>(qa, rrs, rbase, rls, 4 * b0, ph, c, rb, in);
    load_quad<T, ALIGNED>(qb, drs, dbase, dls, 4 * b0, ph, c, rb, in);
    // block row i of the band (kBandBlocks is the halo block row)
    auto step = [&](int i) {
        Quad ca = qa, cb = qb;
        if (i < kBandBlocks) {  // the next block row travels while this one is summed
            load_quad<T, ALIGNED>(qa, rrs, rbase, rls, 4 * (b0 + i + 1), ph, c, rb, in);
            load_quad<T, ALIGNED>(qb, drs, dbase, dls, 4 * (b0 + i + 1), ph, c, rb, in);
        }
        uint32_t blk[LB + 1][4];
#pragma unroll
        for (int b = 0; b < LB; ++b) {
            uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int d = b * DPB; d < (b + 1) * DPB; ++d) {
                    uint32_t va = ca.w[j][d], vb = cb.w[j][d];
                    if constexpr (RAGGED && ALIGNED) { va &= mask[d]; vb &= mask[d]; }
                    s1 = dot<T>(va, kOnes, s1);
                    s2 = dot<T>(vb, kOnes, s2);
                    ss = dot<T>(va, va, ss);
                    ss = dot<T>(vb, vb, ss);
                    s12 = dot<T>(va, vb, s12);
                }
            blk[b][0] = s1; blk[b][1] = s2; blk[b][2] = ss; blk[b][3] = s12;
            if (i < kBandBlocks) sse += ss - 2 * s12;  // sum (a - b)^2 of the block; the halo row belongs to the next band
        }
        // the next lane's first block (wave_shl:1; the halo lane's own result is unused)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            blk[LB][v] = (uint32_t)__builtin_amdgcn_mov_dpp((int)blk[0][v], 0x130, 0xf, 0xf, true);
        const bool rows_ok = b0 + i < bh;  // the lower block row of the window is a full one
#pragma unroll
        for (int b = 0; b < LB; ++b) {
            uint32_t h[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) h[v] = blk[b][v] + blk[b + 1][v];
            if (i > 0 && own && rows_ok && c0 + b + 1 < bw)
                acc += ssim_window(prev[b][0] + h[0], prev[b][1] + h[1], prev[b][2] + h[2], prev[b][3] + h[3], c1, c2);
#pragma unroll
            for (int v = 0; v < 4; ++v) prev[b][v] = h[v];
        }
    };
    // rows at and below bhc hold nothing but zeros (the test is uniform)
    if constexpr (ALIGNED) {
#pragma unroll
        for (int i = 0; i <= kBandBlocks; ++i) {
            if (b0 + i >= bhc) break;
            step(i);
        }
    } else {  // the sample-by-sample path stays rolled: unrolled it spills SGPRs
#pragma unroll 1
        for (int i = 0; i <= kBandBlocks && b0 + i < bhc; ++i) step(i);
    }

    const uint64_t s64 = wave_sum<uint64_t>(own ? sse : 0);
    acc = wave_sum(acc);
    __syncthreads();  // the previous unit's partial has been read
    if (lane == 0) { s_sse[wave] = s64; s_ssim[wave] = acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out->sse = s_sse[0] + s_sse[1] + s_sse[2] + s_sse[3];
        out->ssim = ((s_ssim[0] + s_ssim[1]) + s_ssim[2]) + s_ssim[3];
    }
}

// 1-D grid over the (frame, tile) units, frame-major and band-major within a
// plane, with the XCD-aware numbering: the workgroups running at any moment
// hold vertically adjacent bands of the same frames on one XCD, so a band's
// halo block row is read from HBM by one neighbour and hits that L2 for the other.
template <typename T, bool ALIGNED, bool RAGGED>
__global__ __launch_bounds__(256) void metrics_kernel(const MetArgs a) {
    const int64_t total = (int64_t)a.nk * a.tiles;
    for (int64_t u = xcd_remap(blockIdx.x, gridDim.x); u < total; u += gridDim.x) {
        const int k = (int)(u / a.tiles);
        metrics_unit<T, ALIGNED, RAGGED>(a, k, (int)(u - (int64_t)k * a.tiles), a.part + u);
    }
}

struct MetFinal {
    int tile0[3], ntile[3];
    int tiles;
    int64_t windows[3];  // 0: SSIM undefined (bw < 2 or bh < 2)
};

// One lane per (frame, plane): its partials in unit order.
__global__ __launch_bounds__(64) void metrics_finalize(const MetPartial *part, MetFinal f, int nframes, uint64_t *sse,
                                                       double *ssim) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= nframes * 3) return;
    const int k = o / 3, p = o - 3 * k;
    const MetPartial *q = part + (int64_t)k * f.tiles + f.tile0[p];
    uint64_t s = 0;
    double v = 0.0;
    for (int i = 0; i < f.ntile[p]; ++i) { s += q[i].sse; v += q[i].ssim; }
    sse[o] = s;
    ssim[o] = f.windows[p] ? v / (double)f.windows[p] : __builtin_nan("");
}

}  // namespace pp

using namespace pp;

extern "C" int pp_metrics(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *ref, const pp_frames *dist,
                          const int32_t *ref_index, int nframes, uint64_t *sse, double *ssim, void *stream) {
    if (!ctx || !ref || !dist || !sse || !ssim) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid || fi.packed) PP_FAIL(PP_ERR_INVALID, "metrics need a planar format (got %d)", fmt);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    if (nframes < 1) PP_FAIL(PP_ERR_INVALID, "nframes %d < 1", nframes);
    if (ref_index)
        for (int k = 0; k < nframes; ++k)
            if (ref_index[k] < 0) PP_FAIL(PP_ERR_INVALID, "ref_index[%d] = %d is negative", k, ref_index[k]);
    const int bytes = fi.depth > 8 ? 2 : 1;
    const int span = kMetWaves * kMetOwnLanes * (kMetLaneBytes / bytes);
    PairPlanes pl;
    // the band's halo rows stay inside the buffer range too
    if (int e = check_pair(pl, fmt, w, h, ref, dist, 4 * (kBandBlocks + 1), "", "", true)) return e;
    MetArgs a{};
    MetFinal f{};
    put_pair(a, pl);
    bool ragged = false;
    for (int p = 0; p < 3; ++p) {
        const int pw = pl.g[p].pw, ph = pl.g[p].ph;
        ragged |= (pl.g[p].rb & 15) != 0;
        a.pw[p] = pw; a.ph[p] = ph;
        a.tiles_x[p] = (pw + span - 1) / span;
        const int bands = (((ph + 3) >> 2) + kBandBlocks - 1) / kBandBlocks;
        a.tile0[p] = f.tile0[p] = a.tiles;
        f.ntile[p] = a.tiles_x[p] * bands;
        a.tiles += f.ntile[p];
        const int bw = pw >> 2, bh = ph >> 2;
        f.windows[p] = bw < 2 || bh < 2 ? 0 : (int64_t)(bw - 1) * (bh - 1);
    }
    f.tiles = a.tiles;
    a.depth = fi.depth;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    if (int e = grow(ctx->met, sizeof(MetPartial) * (size_t)a.tiles * nframes)) return e;
    MetPartial *part = static_cast<MetPartial *>(ctx->met.buf);

    const auto k = bytes == 2 ? PP_PICK_EDGE(metrics_kernel, uint16_t, pl.aligned, ragged)
                              : PP_PICK_EDGE(metrics_kernel, uint8_t, pl.aligned, ragged);
    // identity: one launch over all frames; a map travels in the kernel
    // arguments, kFrameMap dist frames per launch (as pp_stall_compose's)
    each_launch(nframes, ref_index ? kFrameMap : nframes, [&](int k0, int nk) {
        MetArgs b = a;
        b.nk = nk;
        b.identity = ref_index == nullptr;
        if (ref_index) fill_map(b.idx, ref_index, k0, nk);  // the identity's launch may pass kFrameMap frames
        for (int p = 0; p < 3; ++p) b.dist[p] += (int64_t)k0 * a.dfs[p];
        b.part = part + (int64_t)k0 * a.tiles;
        const int64_t units = (int64_t)b.nk * a.tiles;
        const int groups = (int)std::min<int64_t>(units, (int64_t)std::max(1, ctx->cus) * 8);
        hipLaunchKernelGGL(k, dim3(groups), dim3(256), 0, st, b);
    });
    hipLaunchKernelGGL(metrics_finalize, dim3((nframes * 3 + 63) / 64), dim3(64), 0, st, part, f, nframes, sse, ssim);
    PP_HIP(hipGetLastError());
    return PP_OK;
}
