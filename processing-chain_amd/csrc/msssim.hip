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
// window column.  The band's kMsBandRows + 10 input rows go through
// window_moments (analysis_dev.hpp) with N = 11: every lane loads one sample of
// each plane a row (lanes 0 .. 9 one more: the halo right of the tile), the
// products a^2, b^2, a b are exact (24 x 24 bits), and a window's five weighted
// sums give l and cs, added to the lane's two sums.
// Every load is one element at a clamped position, whatever the pointer and
// the pitches are: there is no second path for sources off the 16-byte grid,
// and the layout of the same samples cannot change a bit of the result.
// a^2, b^2 and a b go through the same operations, so on identical planes
// 2 sigma_ab and sigma_a^2 + sigma_b^2 are the same bits, and l = cs = 1.0.
// Reduction: block_sum -> one partial per unit; msssim_finalize adds a (frame, scale)'s
// partials in unit order and divides by the window count.  No atomics: two runs
// give the same bits.
#include <algorithm>
#include <cmath>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kMsScales = 5;
constexpr int kMsTaps = 11;             // window side
constexpr int kMsHalo = kMsTaps - 1;    // input rows / columns a tile needs beyond its windows
constexpr int kMsWaves = 4;             // waves per workgroup
constexpr int kMsTileCols = 64 * kMsWaves;  // window columns of a tile: one per lane
constexpr int kMsBandRows = 64;         // window rows of a tile

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
    int32_t idx[kFrameMap];       // reference frame of distorted frame k
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

// Element (y, x) of a level as the window kernel reads it: scale 0 the samples
// themselves (T), the others the pyramid's uint32 sums.
template <typename T>
__device__ __forceinline__ uint32_t ms_sample(const LevelPlane &p, bool samples, int y, int x) {
    const uint8_t *row = p.base + (int64_t)y * p.ls;
    return samples ? (uint32_t) reinterpret_cast<const T *>(row)[x] : reinterpret_cast<const uint32_t *>(row)[x];
}

template <typename T>
__device__ __forceinline__ void msssim_unit(const MsArgs &a, int k, int unit, double2 (*s_row)[kMsTileCols + kMsHalo],
                                            double (*s_red)[2]) {
    int s = 0;
    while (unit >= a.unit0[s + 1]) ++s;  // uniform; a scale without windows has no unit
    const int t = unit - a.unit0[s];
    const int band = t / a.tx[s], tile = t - band * a.tx[s];
    const int ws = a.ws[s], hs = a.hs[s];
    const int x0 = tile * kMsTileCols, y0 = band * kMsBandRows;
    const int nin = min(kMsBandRows, hs - kMsHalo - y0) + kMsHalo;  // input rows of the band
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool own = x0 + tid < ws - kMsHalo;             // the lane's column has windows
    const bool busy = x0 + wave * 64 < ws - kMsHalo;      // some lane of the wave has (uniform)
    const bool samples = s == 0;
    LevelPlane pa, pb;
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
    auto fetch = [&](int i, bool halo, uint2 &nx, uint2 &nh) {
        const int y = min(y0 + i, hs - 1);
        nx = make_uint2(ms_sample<T>(pa, samples, y, cx), ms_sample<T>(pb, samples, y, cx));
        if (halo) nh = make_uint2(ms_sample<T>(pa, samples, y, hx), ms_sample<T>(pb, samples, y, hx));
    };
    // the sums are 4^s times the means: C1 and C2 follow by 16^s (exact)
    const double sc = (double)(1u << (4 * s));
    const double c1 = a.c1 * sc, c2 = a.c2 * sc;
    double acc[2] = {0.0, 0.0};  // cs, l * cs
    window_moments<kMsTaps, kMsTileCols, uint2>(s_row, a.g, nin, busy, fetch, [&](const double v[5]) {
        const double maa = v[0] * v[0], mbb = v[1] * v[1], mab = v[0] * v[1];
        const double saa = v[2] - maa, sbb = v[3] - mbb, sab = v[4] - mab;
        const double l = (mab + mab + c1) / (maa + mbb + c1);
        const double cs = (sab + sab + c2) / (saa + sbb + c2);
        if (own) { acc[0] += cs; acc[1] += l * cs; }
    });
    block_sum(acc, s_red);
    if (tid == 0) {
        MsPartial *out = a.part + (int64_t)k * a.unit0[kMsScales] + unit;
        out->cs = acc[0];
        out->ssim = acc[1];
    }
    __syncthreads();  // s_red and the rows have been read: the next unit may write them
}

// 1-D grid over the (frame, unit) pairs, frame-major.
template <typename T>
__global__ __launch_bounds__(256) void msssim_kernel(const MsArgs a) {
    __shared__ double2 s_row[2][kMsTileCols + kMsHalo];
    __shared__ double s_red[kMsWaves][2];
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
    const LumaClip r{ref, ref_linesize, ref_frame_stride, nref}, d{dist, dist_linesize, dist_frame_stride, ndist};
    LumaPlanes lp;
    // one element-wise path: lp.aligned is not looked at
    if (int e = luma_checks(lp, bitdepth, w, h, r, d, false, ref_index, ndist, kRefIndexMap)) return e;
    const int es = lp.es;
    if (ndist == 0) return PP_OK;

    MsArgs a{};
    put_luma_pair(a, r, d);
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
    const int64_t pyr_bytes = (int64_t)sizeof(uint32_t) * 2 * a.plane;
    const int per = frames_per_launch(ndist, pyr_bytes);
    const int upf = a.unit0[kMsScales];
    const size_t part_bytes = sizeof(MsPartial) * (size_t)per * std::max(upf, 1);
    if (int e = grow(ctx->mss, part_bytes + (size_t)per * (size_t)pyr_bytes)) return e;
    a.part = static_cast<MsPartial *>(ctx->mss.buf);
    a.pyr = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ctx->mss.buf) + part_bytes);

    const int cus = std::max(1, ctx->cus);
    auto blocks = [&](int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)cus * 64)); };
    each_launch(ndist, per, [&](int k0, int nk) {
        MsArgs b = a;
        b.nk = nk;
        fill_map(b.idx, ref_index, k0, nk);
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
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
