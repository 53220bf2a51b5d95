// Pixel-domain Visual Information Fidelity of two luma batches (spec PP-VIF-1,
// DESIGN.md) on gfx950: per distorted frame and scale s = 0 .. 3 the pair
// (sum num, sum den) over every sample position of the scale, after Sheikh &
// Bovik 2006 in the four-scale form VMAF uses as vif_scale0..3.  Pooling into
// vif_scale_s and vif is host work (pixpath/vif.py).  Parity with libvmaf's
// float_vif is unpinned: no libvmaf exists to compare with.
//
// Samples are brought to the 8-bit scale (x = sample / 2^(bitdepth - 8), exact)
// and everything after that is fp64.  Borders are mirrored without repeating
// the edge sample (index -i reads i, n - 1 + i reads n - 1 - i) by index
// arithmetic at load time, never by a padded copy; a scale exists only where
// one reflection suffices (w_s, h_s >= N_s / 2 + 1).
//
// Pyramid: level s + 1 is level s filtered with the N_{s+1}-tap Gaussian and
// decimated to its even rows and columns (vif_decimate), for the reference frame
// ref_index[k] and the distorted frame k of every k of the launch, as doubles in
// the context's workspace.  A workgroup owns 256 output columns x 32 output rows
// of one plane; a lane owns one output column.  Per input row of the band
// (2 * 31 + N of them) the lanes put the row's 512 + N - 1 samples as doubles
// into one of two LDS rows, a lane filters along the row at its even column
// only (H at the kept columns), keeps the result in a ring of N registers, and
// on every second row filters the ring (V at the kept rows) and stores.
//
// Statistics (vif_stat<T, N>, N = 17, 9, 5, 3): a workgroup (256 lanes, 4
// waves) owns one unit = (frame k, tile of kVifTileCols positions x
// kVifBandRows rows) of one scale; a lane owns one column.  The band's
// kVifBandRows + N - 1 input rows (mirrored) go through window_moments
// (analysis_dev.hpp; its ring takes 170 VGPRs at N = 17): every lane loads one
// sample of each plane a row (lanes 0 .. N - 2 one more: the halo right of the
// tile), and a position's five means go through the spec's arithmetic (two
// IEEE divisions, two log2) into num and den, added to the lane's two sums.
// Every load is one element at a mirrored, clamped position, whatever the
// pointer and the pitches are: there is one path, and the layout of the same
// samples cannot change a bit of the result.
// Reduction: block_sum -> one partial per unit; vif_finalize adds a (frame, scale)'s
// partials in unit order, or writes NaN.  No atomics: two runs give the same
// bits.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kVifScales = 4;
constexpr int kVifMaxTaps = 17;
constexpr int kVifWaves = 4;             // waves per workgroup
constexpr int kVifTileCols = 64 * kVifWaves;  // columns of a tile: one per lane
constexpr int kVifBandRows = 64;         // rows of a statistics tile
constexpr int kVifDecRows = 32;          // output rows of a decimation tile
constexpr double kVifEps = 1e-10;
constexpr double kVifNoise = 2.0;        // sigma_n^2

constexpr int vif_taps(int s) { return s == 0 ? 17 : s == 1 ? 9 : s == 2 ? 5 : 3; }
constexpr int vif_scale_of(int n) { return n == 17 ? 0 : n == 9 ? 1 : n == 5 ? 2 : 3; }

struct VifPartial {
    double num, den;  // sums over the unit's positions
};

struct VifArgs {
    const uint8_t *ref, *dist;
    int64_t rls, rfs, dls, dfs;
    int nk;                        // distorted frames of this launch
    int nsc;                       // scales that exist (the first nsc)
    double mul;                    // sample -> 8-bit scale: 2^-(bitdepth - 8)
    int ws[kVifScales], hs[kVifScales];
    int tx[kVifScales];            // tiles across a scale
    int unit0[kVifScales + 1];     // first unit of a scale within a frame; [4]: units of a frame
    int64_t off[kVifScales];       // first element of level s (1 .. 3) within a plane's pyramid
    int64_t plane;                 // elements of a plane's pyramid
    double *pyr;                   // [nk][2: ref, dist][plane]
    VifPartial *part;              // [nk][units]
    double *out;                   // [nk][4][2]
    double g[kVifScales][kVifMaxTaps];
    int32_t idx[kFrameMap];        // reference frame of distorted frame k
};

// One plane of one scale: scale 0 the samples themselves (T), the others the
// pyramid's doubles.
template <typename T>
__device__ __forceinline__ LevelPlane vif_plane(const VifArgs &a, int k, int side, int s) {
    if constexpr (std::is_same<T, double>::value) {
        const double *q = a.pyr + (int64_t)(2 * k + side) * a.plane + a.off[s];
        return {reinterpret_cast<const uint8_t *>(q), (int64_t)a.ws[s] * 8};
    } else {
        if (side) return {a.dist + (int64_t)k * a.dfs, a.dls};
        return {a.ref + (int64_t)a.idx[k] * a.rfs, a.rls};
    }
}

// Level s + 1 of both pyramids from level s (T = the sample type for s = 0,
// double after that); N = the taps of scale s + 1.  One workgroup per (plane,
// tile) of the launch, plane-major.
template <typename T, int N>
__global__ __launch_bounds__(256) void vif_decimate(const VifArgs a) {
    constexpr int R = N / 2, s = vif_scale_of(N) - 1;
    __shared__ __align__(16) double s_row[2][2 * kVifTileCols + N - 1];
    const int wi = a.ws[s], hi = a.hs[s], wo = a.ws[s + 1], ho = a.hs[s + 1];
    const int tx = (wo + kVifTileCols - 1) / kVifTileCols, ty = (ho + kVifDecRows - 1) / kVifDecRows;
    const int per = tx * ty;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *g = a.g[s + 1];
    const bool halo = tid < N - 1;
    {
        const int pl = blockIdx.x / per;  // 2 k + (0: ref, 1: dist)
        const int t = blockIdx.x - pl * per;
        const int band = t / tx, tile = t - band * tx;
        const LevelPlane p = vif_plane<T>(a, pl >> 1, pl & 1, s);
        const int xo0 = tile * kVifTileCols, yo0 = band * kVifDecRows;
        const int nout = min(kVifDecRows, ho - yo0);
        const int nin = 2 * (nout - 1) + N;  // input rows of the band
        const bool own = xo0 + tid < wo;
        const bool busy = xo0 + wave * 64 < wo;  // some lane of the wave owns a column (uniform)
        // LDS entry j of a row is input column 2 xo0 - R + j
        const int c0 = mirror_index(2 * xo0 - R + 2 * tid, wi), c1 = mirror_index(2 * xo0 - R + 2 * tid + 1, wi);
        const int ch = mirror_index(2 * xo0 - R + 2 * kVifTileCols + tid, wi);
        double n0, n1, nh = 0.0;  // the next row's samples
        auto fetch = [&](int i) {
            const int y = mirror_index(2 * yo0 - R + i, hi);
            n0 = level_sample<T>(p, y, c0, a.mul);
            n1 = level_sample<T>(p, y, c1, a.mul);
            if (halo) nh = level_sample<T>(p, y, ch, a.mul);
        };
        double *dst = a.pyr + (int64_t)pl * a.plane + a.off[s + 1] + (int64_t)yo0 * wo + min(xo0 + tid, wo - 1);
        double ring[N];
        fetch(0);
        for (int i0 = 0; i0 < nin; i0 += N) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int i = i0 + j;  // input row of the band; its ring slot is j
                if (i >= nin) break;   // uniform
                double *row = s_row[i & 1];
                reinterpret_cast<double2 *>(row)[tid] = make_double2(n0, n1);
                if (halo) row[2 * kVifTileCols + tid] = nh;
                // this row has landed; the row before it has been read by every wave
                __syncthreads();
                if (i + 1 < nin) fetch(i + 1);  // travels while this row is filtered
                if (!busy) continue;
                double hsum;
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const double v = row[2 * tid + q];
                    hsum = q ? __builtin_fma(g[sym_tap(q, N)], v, hsum) : g[0] * v;
                }
                ring[j] = hsum;
                if (i < N - 1 || ((i - (N - 1)) & 1)) continue;  // uniform: V at the even rows only
                double v;
#pragma unroll
                for (int q = 0; q < N; ++q) {  // tap q is input row i - (N - 1) + q
                    const double x = ring[(j + 1 + q) % N];
                    v = q ? __builtin_fma(g[sym_tap(q, N)], x, v) : g[0] * x;
                }
                if (own) dst[(int64_t)((i - (N - 1)) >> 1) * wo] = v;
            }
        }
    }
}

// num and den of one position from its five filtered quantities (PP-VIF-1).
__device__ __forceinline__ void vif_position(const double v[5], double &num, double &den) {
    const double mu1 = v[0], mu2 = v[1];
    double s1 = fmax(v[2] - mu1 * mu1, 0.0);
    const double s2 = fmax(v[3] - mu2 * mu2, 0.0);
    const double s12 = v[4] - mu1 * mu2;
    double g = s12 / (s1 + kVifEps);
    double sv = s2 - g * s12;
    if (s1 < kVifEps) { g = 0.0; sv = s2; s1 = 0.0; }
    if (s2 < kVifEps) { g = 0.0; sv = 0.0; }
    if (g < 0.0) { sv = s2; g = 0.0; }
    sv = fmax(sv, kVifEps);
    g = fmin(g, 100.0);
    num = ::log2(1.0 + g * g * s1 / (sv + kVifNoise));
    den = ::log2(1.0 + s1 / kVifNoise);
    if (s12 < 0.0) num = 0.0;
    if (s1 < kVifNoise) { num = 1.0 - s2 * 4.0 / 65025.0; den = 1.0; }
}

// The scale of N taps of every frame of the launch: one workgroup per (frame,
// unit of the scale), frame-major.
template <typename T, int N>
__global__ __launch_bounds__(256) void vif_stat(const VifArgs a) {
    constexpr int R = N / 2, s = vif_scale_of(N);
    __shared__ __align__(16) double2 s_row[2][kVifTileCols + N - 1];
    __shared__ double s_red[kVifWaves][2];
    const int ws = a.ws[s], hs = a.hs[s], tx = a.tx[s];
    const int ups = a.unit0[s + 1] - a.unit0[s];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x / ups, t = blockIdx.x - k * ups;
    const int band = t / tx, tile = t - band * tx;
    const int x0 = tile * kVifTileCols, y0 = band * kVifBandRows;
    const int nin = min(kVifBandRows, hs - y0) + N - 1;  // input rows of the band
    const bool own = x0 + tid < ws;            // the lane's column is a position
    const bool busy = x0 + wave * 64 < ws;     // some lane of the wave has one (uniform)
    const LevelPlane pa = vif_plane<T>(a, k, 0, s), pb = vif_plane<T>(a, k, 1, s);
    // LDS entry j of a row is column x0 - R + j
    const int cx = mirror_index(x0 - R + tid, ws), hx = mirror_index(x0 - R + kVifTileCols + tid, ws);
    auto fetch = [&](int i, bool halo, double2 &nx, double2 &nh) {
        const int y = mirror_index(y0 - R + i, hs);
        nx = make_double2(level_sample<T>(pa, y, cx, a.mul), level_sample<T>(pb, y, cx, a.mul));
        if (halo) nh = make_double2(level_sample<T>(pa, y, hx, a.mul), level_sample<T>(pb, y, hx, a.mul));
    };
    double acc[2] = {0.0, 0.0};  // num, den
    window_moments<N, kVifTileCols, double2>(s_row, a.g[s], nin, busy, fetch, [&](const double v[5]) {
        double num, den;
        vif_position(v, num, den);
        if (own) { acc[0] += num; acc[1] += den; }
    });
    block_sum(acc, s_red);
    if (tid == 0) {
        VifPartial *out = a.part + (int64_t)k * a.unit0[kVifScales] + a.unit0[s] + t;
        out->num = acc[0];
        out->den = acc[1];
    }
}

// One lane per (frame, scale): its partials in unit order; NaN for a scale
// that does not exist.
__global__ __launch_bounds__(64) void vif_finalize(const VifArgs a) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.nk * kVifScales) return;
    const int k = o / kVifScales, s = o - k * kVifScales;
    double num = __builtin_nan(""), den = __builtin_nan("");
    if (s < a.nsc) {
        const VifPartial *q = a.part + (int64_t)k * a.unit0[kVifScales];
        num = den = 0.0;
        for (int u = a.unit0[s]; u < a.unit0[s + 1]; ++u) { num += q[u].num; den += q[u].den; }
    }
    a.out[2 * o] = num;
    a.out[2 * o + 1] = den;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_vif(pp_ctx *ctx, int bitdepth, int w, int h, const void *ref, int64_t ref_linesize,
                      int64_t ref_frame_stride, int nref, const void *dist, int64_t dist_linesize,
                      int64_t dist_frame_stride, int ndist, const int32_t *ref_index, double *out, void *stream) {
    if (!ctx || !ref || !dist || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    const LumaClip r{ref, ref_linesize, ref_frame_stride, nref}, d{dist, dist_linesize, dist_frame_stride, ndist};
    LumaPlanes lp;
    // one element-wise path: lp.aligned is not looked at
    if (int e = luma_checks(lp, bitdepth, w, h, r, d, false, ref_index, ndist, kRefIndexMap)) return e;
    const int es = lp.es;
    if (ndist == 0) return PP_OK;

    VifArgs a{};
    put_luma_pair(a, r, d);
    a.mul = 1.0 / (double)(1 << (bitdepth - 8));
    a.nsc = kVifScales;
    for (int s = 0; s < kVifScales; ++s) {
        const int n = vif_taps(s);
        a.ws[s] = w >> s; a.hs[s] = h >> s;
        // a scale exists where one reflection suffices; a missing one ends the pyramid
        if (s < a.nsc && (a.ws[s] < n / 2 + 1 || a.hs[s] < n / 2 + 1)) a.nsc = s;
        const bool any = s < a.nsc;
        a.tx[s] = any ? (a.ws[s] + kVifTileCols - 1) / kVifTileCols : 0;
        a.unit0[s + 1] = a.unit0[s] + (any ? a.tx[s] * ((a.hs[s] + kVifBandRows - 1) / kVifBandRows) : 0);
        if (s && any) {
            a.off[s] = a.plane;
            a.plane += (int64_t)a.ws[s] * a.hs[s];
        }
        // the window, normalised in fp64 (PP-VIF-1): sigma = N / 5
        const double sigma = (double)n / 5.0;
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += a.g[s][i] = std::exp(-(double)((i - n / 2) * (i - n / 2)) / (2.0 * sigma * sigma));
        for (int i = 0; i < n; ++i) a.g[s][i] /= sum;
    }

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    const int64_t pyr_bytes = (int64_t)sizeof(double) * 2 * a.plane;
    const int per = frames_per_launch(ndist, pyr_bytes);
    const int upf = a.unit0[kVifScales];
    const size_t part_bytes = sizeof(VifPartial) * (size_t)per * std::max(upf, 1);
    if (int e = grow(ctx->vif, part_bytes + (size_t)per * (size_t)pyr_bytes)) return e;
    a.part = static_cast<VifPartial *>(ctx->vif.buf);
    a.pyr = reinterpret_cast<double *>(static_cast<uint8_t *>(ctx->vif.buf) + part_bytes);

    // a workgroup per tile: far below 2^31 for planes inside the 2 GiB range and kFrameMap frames
    auto grid = [](int64_t n) { return dim3((unsigned)n); };
    each_launch(ndist, per, [&](int k0, int nk) {
        VifArgs b = a;
        b.nk = nk;
        fill_map(b.idx, ref_index, k0, nk);
        b.dist += (int64_t)k0 * a.dfs;
        b.out = out + (int64_t)k0 * kVifScales * 2;
        for (int s = 0; s + 1 < a.nsc; ++s) {  // level s + 1 from level s
            const int64_t tiles = (int64_t)((a.ws[s + 1] + kVifTileCols - 1) / kVifTileCols) *
                                  ((a.hs[s + 1] + kVifDecRows - 1) / kVifDecRows) * 2 * b.nk;
            if (s == 0 && es == 2) hipLaunchKernelGGL((vif_decimate<uint16_t, 9>), grid(tiles), dim3(256), 0, st, b);
            else if (s == 0) hipLaunchKernelGGL((vif_decimate<uint8_t, 9>), grid(tiles), dim3(256), 0, st, b);
            else if (s == 1) hipLaunchKernelGGL((vif_decimate<double, 5>), grid(tiles), dim3(256), 0, st, b);
            else hipLaunchKernelGGL((vif_decimate<double, 3>), grid(tiles), dim3(256), 0, st, b);
        }
        for (int s = 0; s < a.nsc; ++s) {
            const dim3 gr = grid((int64_t)b.nk * (a.unit0[s + 1] - a.unit0[s]));
            if (s == 0 && es == 2) hipLaunchKernelGGL((vif_stat<uint16_t, 17>), gr, dim3(256), 0, st, b);
            else if (s == 0) hipLaunchKernelGGL((vif_stat<uint8_t, 17>), gr, dim3(256), 0, st, b);
            else if (s == 1) hipLaunchKernelGGL((vif_stat<double, 9>), gr, dim3(256), 0, st, b);
            else if (s == 2) hipLaunchKernelGGL((vif_stat<double, 5>), gr, dim3(256), 0, st, b);
            else hipLaunchKernelGGL((vif_stat<double, 3>), gr, dim3(256), 0, st, b);
        }
        hipLaunchKernelGGL(vif_finalize, dim3((b.nk * kVifScales + 63) / 64), dim3(64), 0, st, b);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
