// Multi-scale SSIM of two luma batches (spec PP-MSSSIM-1) on gfx950:
// per distorted frame and scale s = 0 .. 4 the mean of cs and of l * cs over the
// 11 x 11 Gaussian windows (sigma 1.5, valid, stride 1) of the 2^s x 2^s block
// means of both planes.  Pooling the ten values into MS-SSIM is host work
// (pixpath/msssim.py).
//
// The first analysis kernel here that is bound by arithmetic, not by the
// stream: about 200 fp64 instructions per window against 2 to 4 element loads.
//
// Pyramid: integers.  Scale s >= 1 of a plane is kept as the SUM of each
// 2^s x 2^s block (uint32, <= 65535 * 256 < 2^24), built level by level with
// the odd trailing row / column dropped (msssim_pyr1 from the samples,
// msssim_pyr_next from the level above), for the reference frame ref_index[k]
// and the distorted frame k of every k of the launch, in the context's
// workspace.  The window filter runs on those sums as they are: the mean is the
// sum over 4^s, a power of two, so every moment of the means is the moment of
// the sums scaled exactly, and C1, C2 are scaled by 16^s instead: the quotients
// are the same bits as on the means, and nothing is rounded before the window.
//
// Windows: a workgroup (256 lanes, 4 waves) owns one unit = (frame k, scale,
// tile of kMsTileCols window columns x kMsBandRows window rows); a lane owns one
// window column.  Per input row of the band (kMsBandRows + 10 of them):
//   - every lane loads one sample of each plane (lanes 0 .. 9 one more: the
//     halo right of the tile), the next row's while this one is worked on, and
//     puts both as doubles into one of two LDS rows (one barrier a row);
//   - H: the lane reads its 11 neighbours (a, b) from LDS and filters the five
//     quantities a, b, a^2, b^2, a b (the products are exact: 24 x 24 bits)
//     into slot row % 11 of a ring of 11 rows x 5 doubles held in registers
//     (the row loop is unrolled by 11, so every slot is a fixed register);
//   - V: from the tenth row on, the ring's 11 rows give the window's five
//     weighted sums, then l and cs, added to the lane's two sums.
// Every load is one element at a clamped position, whatever the pointer and
// the pitches are: there is no second path for sources off the 16-byte grid,
// and the layout of the same samples cannot change a bit of the result.
// a^2, b^2 and a b go through the same operations, so on identical planes
// 2 sigma_ab and sigma_a^2 + sigma_b^2 are the same bits, and l = cs = 1.0.
// Reduction: lane -> wave (xor butterfly) -> workgroup (4 values through LDS in
// wave order) -> one partial per unit; msssim_finalize adds a (frame, scale)'s
// partials in unit order and divides by the window count.  No atomics: two runs
// give the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kMsScales = 5;
constexpr int kMsTaps = 11;             // window side
constexpr int kMsHalo = kMsTaps - 1;    // input rows / columns a tile needs beyond its windows
constexpr int kMsWaves = 4;             // waves per workgroup
constexpr int kMsTileCols = 64 * kMsWaves;  // window columns of a tile: one per lane
constexpr int kMsBandRows = 64;         // window rows of a tile
constexpr int kMsIdx = 256;             // ref_index entries per launch (kernel arguments)
constexpr int64_t kMsWork = 1 << 30;    // bytes of pyramids a launch may hold (at least one frame's)

struct MsPartial {
    double cs, ssim;  // sums over the unit's windows
};

struct MsArgs {
    const uint8_t *ref, *dist;
    int64_t rls, rfs, dls, dfs;
    int nk;                       // distorted frames of this launch
    int ws[kMsScales], hs[kMsScales];
    int tx[kMsScales];            // tiles across a scale (0: no window)
    int unit0[kMsScales + 1];     // first unit of a scale within a frame; [5]: units of a frame
    int64_t off[kMsScales];       // first element of scale s (1 .. 4) within a plane's pyramid
    int64_t plane;                // elements of a plane's pyramid
    uint32_t *pyr;                // [nk][2: ref, dist][plane]
    MsPartial *part;              // [nk][units]
    double *out;                  // [nk][5][2]
    double g[kMsTaps];
    double c1, c2;                // of scale 0
    int32_t idx[kMsIdx];          // reference frame of distorted frame k
};

// Level 1 of both pyramids from the samples: one lane per block sum.
template <typename T>
__global__ __launch_bounds__(256) void msssim_pyr1(const MsArgs a) {
    const int w1 = a.ws[1];
    const int64_t per = (int64_t)w1 * a.hs[1], total = per * 2 * a.nk;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t pl = o / per, r = o - pl * per;  // pl = 2 k + (0: ref, 1: dist)
        const int i = (int)(r / w1), j = (int)(r - (int64_t)i * w1);
        const int k = (int)(pl >> 1);
        const uint8_t *base = (pl & 1) ? a.dist + (int64_t)k * a.dfs : a.ref + (int64_t)a.idx[k] * a.rfs;
        const int64_t ls = (pl & 1) ? a.dls : a.rls;
        const T *r0 = reinterpret_cast<const T *>(base + (int64_t)(2 * i) * ls);
        const T *r1 = reinterpret_cast<const T *>(base + (int64_t)(2 * i + 1) * ls);
        a.pyr[pl * a.plane + r] = (uint32_t)r0[2 * j] + r0[2 * j + 1] + r1[2 * j] + r1[2 * j + 1];
    }
}

// Level s >= 2 from level s - 1.
__global__ __launch_bounds__(256) void msssim_pyr_next(const MsArgs a, int s) {
    const int w = a.ws[s], wp = a.ws[s - 1];
    const int64_t per = (int64_t)w * a.hs[s], total = per * 2 * a.nk;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t pl = o / per, r = o - pl * per;
        const int i = (int)(r / w), j = (int)(r - (int64_t)i * w);
        const uint32_t *src = a.pyr + pl * a.plane + a.off[s - 1] + (int64_t)(2 * i) * wp + 2 * j;
        a.pyr[pl * a.plane + a.off[s] + r] = src[0] + src[1] + src[wp] + src[wp + 1];
    }
}

// One plane of one scale as the window kernel reads it: scale 0 the samples
// themselves (T), the others the pyramid's uint32 sums.
struct MsPlane {
    const uint8_t *base;
    int64_t ls;
};

template <typename T>
__device__ __forceinline__ uint32_t ms_sample(const MsPlane &p, bool samples, int y, int x) {
    const uint8_t *row = p.base + (int64_t)y * p.ls;
    return samples ? (uint32_t) reinterpret_cast<const T *>(row)[x] : reinterpret_cast<const uint32_t *>(row)[x];
}

template <typename T>
__device__ __forceinline__ void msssim_unit(const MsArgs &a, int k, int unit, double2 (*s_row)[kMsTileCols + kMsHalo],
                                            MsPartial *s_red) {
    int s = 0;
    while (unit >= a.unit0[s + 1]) ++s;  // uniform; a scale without windows has no unit
    const int t = unit - a.unit0[s];
    const int band = t / a.tx[s], tile = t - band * a.tx[s];
    const int ws = a.ws[s], hs = a.hs[s];
    const int x0 = tile * kMsTileCols, y0 = band * kMsBandRows;
    const int nin = min(kMsBandRows, hs - kMsHalo - y0) + kMsHalo;  // input rows of the band
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool own = x0 + tid < ws - kMsHalo;             // the lane's column has windows
    const bool busy = x0 + wave * 64 < ws - kMsHalo;      // some lane of the wave has (uniform)
    const bool samples = s == 0;
    MsPlane pa, pb;
    if (samples) {
        pa = {a.ref + (int64_t)a.idx[k] * a.rfs, a.rls};
        pb = {a.dist + (int64_t)k * a.dfs, a.dls};
    } else {
        const uint32_t *q = a.pyr + (int64_t)(2 * k) * a.plane + a.off[s];
        pa = {reinterpret_cast<const uint8_t *>(q), (int64_t)ws * 4};
        pb = {reinterpret_cast<const uint8_t *>(q + a.plane), (int64_t)ws * 4};
    }
    // every load goes to an element of the plane: columns and rows are clamped
    // (a clamped value only reaches windows that do not exist)
    const int cx = min(x0 + tid, ws - 1), hx = min(x0 + kMsTileCols + tid, ws - 1);
    const bool halo = tid < kMsHalo;
    uint32_t na, nb, nha = 0, nhb = 0;  // the next row's samples
    auto fetch = [&](int i) {
        const int y = min(y0 + i, hs - 1);
        na = ms_sample<T>(pa, samples, y, cx);
        nb = ms_sample<T>(pb, samples, y, cx);
        if (halo) {
            nha = ms_sample<T>(pa, samples, y, hx);
            nhb = ms_sample<T>(pb, samples, y, hx);
        }
    };
    // the sums are 4^s times the means: C1 and C2 follow by 16^s (exact)
    const double sc = (double)(1u << (4 * s));
    const double c1 = a.c1 * sc, c2 = a.c2 * sc;

    double ring[kMsTaps][5];
    double acs = 0.0, ass = 0.0;
    fetch(0);
    for (int i0 = 0; i0 < nin; i0 += kMsTaps) {
#pragma unroll
        for (int j = 0; j < kMsTaps; ++j) {
            const int i = i0 + j;  // input row of the band; its ring slot is j
            if (i >= nin) break;   // uniform
            double2 *row = s_row[i & 1];
            row[tid] = make_double2((double)na, (double)nb);
            if (halo) row[kMsTileCols + tid] = make_double2((double)nha, (double)nhb);
            // this row has landed; the row before it has been read by every wave, so the
            // next one may overwrite it
            __syncthreads();
            if (i + 1 < nin) fetch(i + 1);  // travels while this row is filtered
            if (!busy) continue;
            double h[5];
#pragma unroll
            for (int u = 0; u < kMsTaps; ++u) {
                const double2 v = row[tid + u];
                const double q[5] = {v.x, v.y, v.x * v.x, v.y * v.y, v.x * v.y};
#pragma unroll
                for (int m = 0; m < 5; ++m) h[m] = u ? __builtin_fma(a.g[u], q[m], h[m]) : a.g[0] * q[m];
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) ring[j][m] = h[m];
            if (i < kMsHalo) continue;  // uniform
            double v[5];
#pragma unroll
            for (int u = 0; u < kMsTaps; ++u)  // tap u is input row i - 10 + u
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    const double x = ring[(j + 1 + u) % kMsTaps][m];
                    v[m] = u ? __builtin_fma(a.g[u], x, v[m]) : a.g[0] * x;
                }
            const double maa = v[0] * v[0], mbb = v[1] * v[1], mab = v[0] * v[1];
            const double saa = v[2] - maa, sbb = v[3] - mbb, sab = v[4] - mab;
            const double l = (mab + mab + c1) / (maa + mbb + c1);
            const double cs = (sab + sab + c2) / (saa + sbb + c2);
            if (own) { acs += cs; ass += l * cs; }
        }
    }
    acs = wave_sum(acs);
    ass = wave_sum(ass);
    if (lane == 0) { s_red[wave].cs = acs; s_red[wave].ssim = ass; }
    __syncthreads();
    if (tid == 0) {
        MsPartial *out = a.part + (int64_t)k * a.unit0[kMsScales] + unit;
        out->cs = ((s_red[0].cs + s_red[1].cs) + s_red[2].cs) + s_red[3].cs;
        out->ssim = ((s_red[0].ssim + s_red[1].ssim) + s_red[2].ssim) + s_red[3].ssim;
    }
    __syncthreads();  // s_red and the rows have been read: the next unit may write them
}

// 1-D grid over the (frame, unit) pairs, frame-major.
template <typename T>
__global__ __launch_bounds__(256) void msssim_kernel(const MsArgs a) {
    __shared__ double2 s_row[2][kMsTileCols + kMsHalo];
    __shared__ MsPartial s_red[kMsWaves];
    const int upf = a.unit0[kMsScales];
    const int64_t total = (int64_t)a.nk * upf;
    for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const int k = (int)(u / upf);
        msssim_unit<T>(a, k, (int)(u - (int64_t)k * upf), s_row, s_red);
    }
}

// One lane per (frame, scale): its partials in unit order over the window
// count; NaN for a scale without windows.
__global__ __launch_bounds__(64) void msssim_finalize(const MsArgs a) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.nk * kMsScales) return;
    const int k = o / kMsScales, s = o - k * kMsScales;
    const MsPartial *q = a.part + (int64_t)k * a.unit0[kMsScales];
    double cs = __builtin_nan(""), ss = __builtin_nan("");
    if (a.unit0[s + 1] > a.unit0[s]) {
        cs = ss = 0.0;
        for (int u = a.unit0[s]; u < a.unit0[s + 1]; ++u) { cs += q[u].cs; ss += q[u].ssim; }
        const double n = (double)((int64_t)(a.ws[s] - kMsHalo) * (a.hs[s] - kMsHalo));
        cs /= n; ss /= n;
    }
    a.out[2 * o] = cs;
    a.out[2 * o + 1] = ss;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_ms_ssim(pp_ctx *ctx, int bitdepth, int w, int h, const void *ref, int64_t ref_linesize,
                          int64_t ref_frame_stride, int nref, const void *dist, int64_t dist_linesize,
                          int64_t dist_frame_stride, int ndist, const int32_t *ref_index, double *out, void *stream) {
    if (!ctx || !ref || !dist || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    if (bitdepth != 8 && bitdepth != 10) PP_FAIL(PP_ERR_INVALID, "bitdepth %d (8 or 10)", bitdepth);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    if (ndist < 0) PP_FAIL(PP_ERR_INVALID, "ndist %d < 0", ndist);
    if (nref < 0) PP_FAIL(PP_ERR_INVALID, "nref %d < 0", nref);
    const int es = bitdepth > 8 ? 2 : 1;
    PlaneGeom g{};
    g.pw = w; g.ph = h; g.rb = (int64_t)w * es;
    bool aligned = true;  // unused: one element-wise path
    pp_frames fr{}, fd{};
    fr.data[0] = const_cast<void *>(ref); fr.linesize[0] = ref_linesize; fr.frame_stride[0] = ref_frame_stride;
    fd.data[0] = const_cast<void *>(dist); fd.linesize[0] = dist_linesize; fd.frame_stride[0] = dist_frame_stride;
    if (int e = check_plane(&fr, 0, g, aligned, 0, "ref ")) return e;
    if (int e = check_plane(&fd, 0, g, aligned, 0, "dist ")) return e;
    if (((uintptr_t)dist | (uint64_t)dist_linesize | (uint64_t)dist_frame_stride | (uintptr_t)ref |
         (uint64_t)ref_linesize | (uint64_t)ref_frame_stride) & (es - 1))
        PP_FAIL(PP_ERR_INVALID, "16-bit samples off the 2-byte grid");
    if (ref_index) {
        for (int k = 0; k < ndist; ++k)
            if (ref_index[k] < 0 || ref_index[k] >= nref)
                PP_FAIL(PP_ERR_INVALID, "ref_index[%d] = %d outside the %d reference frames", k, ref_index[k], nref);
    } else if (ndist > nref) {
        PP_FAIL(PP_ERR_INVALID, "ndist %d > nref %d without ref_index", ndist, nref);
    }
    if (ndist == 0) return PP_OK;

    MsArgs a{};
    a.ref = static_cast<const uint8_t *>(ref);
    a.dist = static_cast<const uint8_t *>(dist);
    a.rls = ref_linesize; a.rfs = ref_frame_stride;
    a.dls = dist_linesize; a.dfs = dist_frame_stride;
    for (int s = 0; s < kMsScales; ++s) {
        a.ws[s] = w >> s; a.hs[s] = h >> s;
        const bool any = a.ws[s] >= kMsTaps && a.hs[s] >= kMsTaps;
        a.tx[s] = any ? (a.ws[s] - kMsHalo + kMsTileCols - 1) / kMsTileCols : 0;
        a.unit0[s + 1] = a.unit0[s] + (any ? a.tx[s] * ((a.hs[s] - kMsHalo + kMsBandRows - 1) / kMsBandRows) : 0);
        if (s) {
            a.off[s] = a.plane;
            a.plane += (int64_t)a.ws[s] * a.hs[s];
        }
    }
    // the window, normalised in fp64 (PP-MSSSIM-1)
    double sum = 0.0;
    for (int i = 0; i < kMsTaps; ++i) sum += a.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5);
    for (int i = 0; i < kMsTaps; ++i) a.g[i] /= sum;
    const double L = (double)((1 << bitdepth) - 1);
    a.c1 = (.01 * L) * (.01 * L);
    a.c2 = (.03 * L) * (.03 * L);

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    // frames per launch: the map's room in the kernel arguments, and a workspace of about kMsWork
    const int64_t pyr_bytes = (int64_t)sizeof(uint32_t) * 2 * a.plane;
    const int per = (int)std::min<int64_t>(std::min(ndist, kMsIdx), std::max<int64_t>(1, kMsWork / std::max<int64_t>(pyr_bytes, 1)));
    const int upf = a.unit0[kMsScales];
    const size_t part_bytes = sizeof(MsPartial) * (size_t)per * std::max(upf, 1);
    if (int e = grow(ctx->mss, part_bytes + (size_t)per * (size_t)pyr_bytes)) return e;
    a.part = static_cast<MsPartial *>(ctx->mss.buf);
    a.pyr = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ctx->mss.buf) + part_bytes);

    const int cus = std::max(1, ctx->cus);
    auto blocks = [&](int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)cus * 64)); };
    // the frame map travels in the kernel arguments, kMsIdx frames per launch (as
    // pp_metrics'); launches on one stream run in order, so they share the workspace
    for (int k0 = 0; k0 < ndist; k0 += per) {
        MsArgs b = a;
        b.nk = std::min(per, ndist - k0);
        for (int k = 0; k < b.nk; ++k) b.idx[k] = ref_index ? ref_index[k0 + k] : k0 + k;
        b.dist += (int64_t)k0 * a.dfs;
        b.out = out + (int64_t)k0 * kMsScales * 2;
        for (int s = 1; s < kMsScales; ++s) {
            const int64_t n = (int64_t)a.ws[s] * a.hs[s] * 2 * b.nk;
            if (n == 0) break;  // and no smaller scale has a sample either
            if (s > 1) hipLaunchKernelGGL(msssim_pyr_next, blocks(n), dim3(256), 0, st, b, s);
            else if (es == 2) hipLaunchKernelGGL(msssim_pyr1<uint16_t>, blocks(n), dim3(256), 0, st, b);
            else hipLaunchKernelGGL(msssim_pyr1<uint8_t>, blocks(n), dim3(256), 0, st, b);
        }
        const int64_t units = (int64_t)b.nk * upf;
        if (units > 0) {
            const dim3 grid((unsigned)std::min<int64_t>(units, (int64_t)1 << 30));
            if (es == 2) hipLaunchKernelGGL(msssim_kernel<uint16_t>, grid, dim3(256), 0, st, b);
            else hipLaunchKernelGGL(msssim_kernel<uint8_t>, grid, dim3(256), 0, st, b);
        }
        hipLaunchKernelGGL(msssim_finalize, dim3((b.nk * kMsScales + 63) / 64), dim3(64), 0, st, b);
    }
    PP_HIP(hipGetLastError());
    return PP_OK;
}
