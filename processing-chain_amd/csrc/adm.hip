// Additive / Detail-loss Metric of two luma batches (spec PP-ADM-1)
// on gfx950: per distorted frame and scale s = 0 .. 3 the six sums
// {sum x_H^3, sum x_V^3, sum x_D^3, sum |rf o_H|^3, sum |rf o_V|^3, sum |rf o_D|^3}
// over the scale's region, after Li, Ngan et al. 2011 in the four-scale form
// VMAF uses as adm2 and adm_scale0..3.  Pooling is host work (pixpath/adm.py).
// Parity with libvmaf's float_adm is unpinned: no libvmaf exists to compare with.
//
// Samples are brought to the 8-bit scale (x = sample / 2^(bitdepth - 8), exact)
// and everything after that is fp64.  Level s of the Daubechies-2 transform has
// (w_{s-1} + 1) / 2 x (h_{s-1} + 1) / 2 coefficients; coefficient i of an axis
// reads inputs 2i - 1 .. 2i + 2, mirrored without repeating the edge sample
// (mirror_index) by index arithmetic at load time.  Rows are filtered first
// (along the row), then columns.
//
// One fused kernel per scale (adm_scale<T, S>): a workgroup (256 lanes, 4
// waves) owns one unit = (frame k, tile of kAdmTileCols coefficient columns x
// kAdmBandRows coefficient rows); lane t owns coefficient column x0 - 1 + t, so
// lanes 0 and 255 are the tile's one-coefficient halo, and the band has one
// halo row above and below.  Per coefficient row of the band:
//   - the lane loads the two new input rows of both planes at its four mirrored
//     columns (the next row's while this one is worked on) and filters them
//     along the row into a ring of 4 input rows x {lo, hi} x {ref, dist};
//   - the ring filtered down the column gives A, H, V, D of both planes; A goes
//     to the workspace for the next scale, H / V / D never leave registers;
//   - decoupling (three IEEE divisions, the angle test) gives rf r, rf o and
//     the position's masking term m = sum |rf a|;
//   - m goes through one of two LDS rows to the lane's neighbours (one barrier a
//     row); with the rows before, the row above gets its threshold M and adds
//     its six cubes to the lane's sums if it lies in the region.
// Every load is one element at a mirrored, clamped position, whatever the
// pointer and the pitches are: there is one path, and the layout of the same
// samples cannot change a bit of the result.
// Reduction: block_gather / block_total -> one partial per unit; adm_finalize adds a (frame, scale)'s
// partials in unit order, or writes NaN.  No atomics: two runs give the same
// bits.
#include <algorithm>
#include <cmath>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kAdmScales = 4;
constexpr int kAdmSums = 6;
constexpr int kAdmWaves = 4;                  // waves per workgroup
constexpr int kAdmLanes = 64 * kAdmWaves;
constexpr int kAdmTileCols = kAdmLanes - 2;   // coefficient columns of a tile: a lane each, less the halo
constexpr int kAdmBandRows = 32;              // coefficient rows of a tile

struct AdmPartial {
    double v[kAdmSums];  // sums over the unit's positions of the region
};

struct AdmArgs {
    const uint8_t *ref, *dist;
    int64_t rls, rfs, dls, dfs;
    int nk;                         // distorted frames of this launch
    int nsc;                        // scales that exist (the first nsc)
    double mul;                     // sample -> 8-bit scale: 2^-(bitdepth - 8)
    int w[kAdmScales + 1], h[kAdmScales + 1];  // [s + 1]: level s; [0]: the plane
    int mw[kAdmScales], mh[kAdmScales];        // margins of the region
    int tx[kAdmScales];             // tiles across a scale
    int unit0[kAdmScales + 1];      // first unit of a scale within a frame; [4]: units of a frame
    int64_t off[kAdmScales];        // first element of A of level s (0 .. 2) within a plane's bands
    int64_t plane;                  // elements of a plane's A bands
    double *pyr;                    // [nk][2: ref, dist][plane]
    AdmPartial *part;               // [nk][units]
    double *out;                    // [nk][4][6]
    double lo[4], hi[4];            // the analysis pair
    double rf[kAdmScales][3];       // 1 / Q(s, theta), theta = H, V, D
    double cos2;                    // cos^2 of one degree
    int32_t idx[kFrameMap];         // reference frame of distorted frame k
};

// One plane of the level a scale reads: the samples themselves (T) for scale
// 0, the A band of the level before (doubles) after that.
template <typename T, int S>
__device__ __forceinline__ LevelPlane adm_plane(const AdmArgs &a, int k, int side) {
    if constexpr (S > 0) {
        const double *q = a.pyr + (int64_t)(2 * k + side) * a.plane + a.off[S - 1];
        return {reinterpret_cast<const uint8_t *>(q), (int64_t)a.w[S] * 8};
    } else {
        if (side) return {a.dist + (int64_t)k * a.dfs, a.dls};
        return {a.ref + (int64_t)a.idx[k] * a.rfs, a.rls};
    }
}

__device__ __forceinline__ double adm_dot4(const double f[4], double v0, double v1, double v2, double v3) {
    return __builtin_fma(f[3], v3, __builtin_fma(f[2], v2, __builtin_fma(f[1], v1, f[0] * v0)));
}

// Decoupling of one position (PP-ADM-1): o, t = {H, V, D} of the reference and
// the distorted plane.  p = rf r, q = rf o, returns m = sum |rf a|.
__device__ __forceinline__ double adm_decouple(const double o[3], const double t[3], const double rf[3], double cos2,
                                               double p[3], double q[3]) {
    const double dp = o[0] * t[0] + o[1] * t[1];
    const double om = o[0] * o[0] + o[1] * o[1];
    const double tm = t[0] * t[0] + t[1] * t[1];
    const bool angle = dp >= 0.0 && dp * dp >= cos2 * om * tm;
    double m = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double k = o[c] == 0.0 ? 0.0 : fmin(fmax(t[c] / o[c], 0.0), 1.0);
        double r = k * o[c];
        double d = t[c] - r;
        if (angle) { r = t[c]; d = 0.0; }
        p[c] = rf[c] * r;
        q[c] = rf[c] * o[c];
        m += fabs(rf[c] * d);
    }
    return m;
}

// Scale S of every frame of the launch: one workgroup per (frame, unit of the
// scale), frame-major.
template <typename T, int S>
__global__ __launch_bounds__(kAdmLanes) void adm_scale(const AdmArgs a) {
    __shared__ double s_m[2][kAdmLanes];
    __shared__ double s_red[kAdmWaves][kAdmSums];
    const int wi = a.w[S], hi = a.h[S], wo = a.w[S + 1], ho = a.h[S + 1];
    const int tx = a.tx[S], ups = a.unit0[S + 1] - a.unit0[S];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x / ups, t = blockIdx.x - k * ups;
    const int band = t / tx, tile = t - band * tx;
    const int x0 = tile * kAdmTileCols, y0 = band * kAdmBandRows;
    const int nrow = min(kAdmBandRows, ho - y0);   // coefficient rows of the band; two more with the halo
    const int c = x0 - 1 + tid;                    // the lane's coefficient column
    const bool own = tid >= 1 && tid <= kAdmTileCols && c < wo;  // a column of the tile, not of its halo
    const bool reg_c = own && c >= a.mw[S] && c < wo - a.mw[S];
    const bool busy = x0 - 1 + wave * 64 < wo;     // some lane of the wave has a column that exists (uniform)
    const bool store = S + 1 < a.nsc;              // a later scale reads A (uniform)
    const LevelPlane pl[2] = {adm_plane<T, S>(a, k, 0), adm_plane<T, S>(a, k, 1)};
    int cx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cx[q] = mirror_index(2 * c - 1 + q, wi);
    double *dst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
        dst[p] = a.pyr + (int64_t)(2 * k + p) * a.plane + a.off[S < 3 ? S : 0] + min(max(c, 0), wo - 1);

    double nx[2][2][4];  // the next two input rows: [row][plane][column]
    auto fetch = [&](int y) {  // input rows y, y + 1
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int yy = mirror_index(y + i, hi);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) nx[i][p][q] = level_sample<T>(pl[p], yy, cx[q], a.mul);
        }
    };
    double ring[4][4];  // input rows 2r - 1 .. 2r + 2 filtered along the row: {ref lo, ref hi, dist lo, dist hi}
    auto rows = [&]() {  // nx into the ring's last two rows
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                ring[2 + i][2 * p] = adm_dot4(a.lo, nx[i][p][0], nx[i][p][1], nx[i][p][2], nx[i][p][3]);
                ring[2 + i][2 * p + 1] = adm_dot4(a.hi, nx[i][p][0], nx[i][p][1], nx[i][p][2], nx[i][p][3]);
            }
    };
    double acc[kAdmSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // the row above (r - 1): rf r, rf o, its m and its neighbours' m; the row above that: its three m
    double pp1[3] = {0.0, 0.0, 0.0}, pq1[3] = {0.0, 0.0, 0.0}, m1 = 0.0, side1 = 0.0, hs2 = 0.0, hs1 = 0.0;
    const int r0 = y0 - 1;
    if (busy) {
        fetch(2 * r0 - 1);
        rows();
        fetch(2 * r0 + 1);
    }
    for (int j = 0; j < nrow + 2; ++j) {
        const int r = r0 + j;  // the coefficient row
        double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, m = 0.0;
        if (busy) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { ring[0][i] = ring[2][i]; ring[1][i] = ring[3][i]; }
            rows();
            if (j + 1 < nrow + 2) fetch(2 * r + 3);  // travels while this row is worked on
            double o[3], d[3], A[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {  // ref, dist
                double *b = s ? d : o;
                A[s] = adm_dot4(a.lo, ring[0][2 * s], ring[1][2 * s], ring[2][2 * s], ring[3][2 * s]);
                b[0] = adm_dot4(a.hi, ring[0][2 * s], ring[1][2 * s], ring[2][2 * s], ring[3][2 * s]);
                b[1] = adm_dot4(a.lo, ring[0][2 * s + 1], ring[1][2 * s + 1], ring[2][2 * s + 1], ring[3][2 * s + 1]);
                b[2] = adm_dot4(a.hi, ring[0][2 * s + 1], ring[1][2 * s + 1], ring[2][2 * s + 1], ring[3][2 * s + 1]);
            }
            if (S < 3 && store && own && j >= 1 && j <= nrow) {
                dst[0][(int64_t)r * wo] = A[0];
                dst[1][(int64_t)r * wo] = A[1];
            }
            m = adm_decouple(o, d, a.rf[S], a.cos2, p, q);
        }
        s_m[j & 1][tid] = m;
        // this row's m has landed; the row before has been read by every wave, so the next may overwrite it
        __syncthreads();
        const double side = s_m[j & 1][max(tid - 1, 0)] + s_m[j & 1][min(tid + 1, kAdmLanes - 1)];
        const double hs = side + m;
        if (j >= 2 && reg_c && r - 1 >= a.mh[S] && r - 1 < ho - a.mh[S]) {
            const double M = ((hs2 + hs) + side1) * (1.0 / 30.0) + m1 * (1.0 / 15.0);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double x = fmax(fabs(pp1[i]) - M, 0.0), y = fabs(pq1[i]);
                acc[i] += x * x * x;
                acc[3 + i] += y * y * y;
            }
        }
        hs2 = hs1; hs1 = hs; m1 = m; side1 = side;
#pragma unroll
        for (int i = 0; i < 3; ++i) { pp1[i] = p[i]; pq1[i] = q[i]; }
    }
    block_gather(acc, s_red);
    if (tid < kAdmSums) {  // a lane per sum
        AdmPartial *out = a.part + (int64_t)k * a.unit0[kAdmScales] + a.unit0[S] + t;
        out->v[tid] = block_total(s_red, tid);
    }
}

// One lane per (frame, scale): its partials in unit order; NaN for a scale
// that does not exist.
__global__ __launch_bounds__(64) void adm_finalize(const AdmArgs a) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= a.nk * kAdmScales) return;
    const int k = o / kAdmScales, s = o - k * kAdmScales;
    double v[kAdmSums];
    for (int i = 0; i < kAdmSums; ++i) v[i] = __builtin_nan("");
    if (s < a.nsc) {
        const AdmPartial *q = a.part + (int64_t)k * a.unit0[kAdmScales];
        for (int i = 0; i < kAdmSums; ++i) v[i] = 0.0;
        for (int u = a.unit0[s]; u < a.unit0[s + 1]; ++u)
            for (int i = 0; i < kAdmSums; ++i) v[i] += q[u].v[i];
    }
    for (int i = 0; i < kAdmSums; ++i) a.out[(int64_t)kAdmSums * o + i] = v[i];
}

}  // namespace pp

using namespace pp;

extern "C" int pp_adm(pp_ctx *ctx, int bitdepth, int w, int h, const void *ref, int64_t ref_linesize,
                      int64_t ref_frame_stride, int nref, const void *dist, int64_t dist_linesize,
                      int64_t dist_frame_stride, int ndist, const int32_t *ref_index, double *out, void *stream) {
    if (!ctx || !ref || !dist || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    const LumaClip r{ref, ref_linesize, ref_frame_stride, nref}, d{dist, dist_linesize, dist_frame_stride, ndist};
    LumaPlanes lp;
    // one element-wise path: lp.aligned is not looked at
    if (int e = luma_checks(lp, bitdepth, w, h, r, d, false, ref_index, ndist, kRefIndexMap)) return e;
    const int es = lp.es;
    if (ndist == 0) return PP_OK;

    AdmArgs a{};
    put_luma_pair(a, r, d);
    a.mul = 1.0 / (double)(1 << (bitdepth - 8));
    // the Daubechies-2 analysis pair, in fp64 (PP-ADM-1)
    const double r3 = std::sqrt(3.0), nrm = 4.0 * std::sqrt(2.0);
    a.lo[0] = (1.0 + r3) / nrm; a.lo[1] = (3.0 + r3) / nrm; a.lo[2] = (3.0 - r3) / nrm; a.lo[3] = (1.0 - r3) / nrm;
    a.hi[0] = a.lo[3]; a.hi[1] = -a.lo[2]; a.hi[2] = a.lo[1]; a.hi[3] = -a.lo[0];
    const double pi = 3.14159265358979323846;
    const double c1 = std::cos(pi / 180.0);
    a.cos2 = c1 * c1;
    // rf[s][theta] = 1 / Q(s, theta): Watson's model with the 9/7 basis amplitudes
    static const double amp[kAdmScales][2] = {{0.67234, 0.72709}, {0.41317, 0.49428}, {0.22727, 0.28688}, {0.11792, 0.15214}};
    const double rr = 3.0 * 1080.0 * pi / 180.0;
    a.w[0] = w; a.h[0] = h;
    a.nsc = kAdmScales;
    for (int s = 0; s < kAdmScales; ++s) {
        for (int th = 0; th < 3; ++th) {
            const double gth = th == 2 ? 0.534 : 1.0;
            const double lg = std::log10(std::pow(2.0, s + 1) * 0.401 * gth / rr);
            a.rf[s][th] = 1.0 / (2.0 * 0.495 * std::pow(10.0, 0.466 * lg * lg) / amp[s][th == 2]);
        }
        const int wo = a.w[s + 1] = (a.w[s] + 1) / 2, ho = a.h[s + 1] = (a.h[s] + 1) / 2;
        // a scale exists where its input and its bands are at least 3 each way; a missing one ends the list
        if (s < a.nsc && (a.w[s] < 3 || a.h[s] < 3 || wo < 3 || ho < 3)) a.nsc = s;
        const bool any = s < a.nsc;
        a.mw[s] = std::max(1, (wo - 5) / 10);
        a.mh[s] = std::max(1, (ho - 5) / 10);
        a.tx[s] = any ? (wo + kAdmTileCols - 1) / kAdmTileCols : 0;
        a.unit0[s + 1] = a.unit0[s] + (any ? a.tx[s] * ((ho + kAdmBandRows - 1) / kAdmBandRows) : 0);
    }
    for (int s = 0; s + 1 < a.nsc; ++s) {  // A of level s, read by scale s + 1
        a.off[s] = a.plane;
        a.plane += (int64_t)a.w[s + 1] * a.h[s + 1];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    const int upf = a.unit0[kAdmScales];
    const int64_t pyr_bytes = (int64_t)sizeof(double) * 2 * a.plane;
    const int per = frames_per_launch(ndist, pyr_bytes);
    const size_t part_bytes = sizeof(AdmPartial) * (size_t)per * std::max(upf, 1);
    if (int e = grow(ctx->adm, part_bytes + (size_t)per * (size_t)pyr_bytes)) return e;
    a.part = static_cast<AdmPartial *>(ctx->adm.buf);
    a.pyr = reinterpret_cast<double *>(static_cast<uint8_t *>(ctx->adm.buf) + part_bytes);

    // a workgroup per tile: far below 2^31 for planes inside the 2 GiB range and kFrameMap frames
    auto grid = [](int64_t n) { return dim3((unsigned)n); };
    each_launch(ndist, per, [&](int k0, int nk) {
        AdmArgs b = a;
        b.nk = nk;
        fill_map(b.idx, ref_index, k0, nk);
        b.dist += (int64_t)k0 * a.dfs;
        b.out = out + (int64_t)k0 * kAdmScales * kAdmSums;
        for (int s = 0; s < a.nsc; ++s) {
            const dim3 gr = grid((int64_t)b.nk * (a.unit0[s + 1] - a.unit0[s]));
            if (s == 0 && es == 2) hipLaunchKernelGGL((adm_scale<uint16_t, 0>), gr, dim3(kAdmLanes), 0, st, b);
            else if (s == 0) hipLaunchKernelGGL((adm_scale<uint8_t, 0>), gr, dim3(kAdmLanes), 0, st, b);
            else if (s == 1) hipLaunchKernelGGL((adm_scale<double, 1>), gr, dim3(kAdmLanes), 0, st, b);
            else if (s == 2) hipLaunchKernelGGL((adm_scale<double, 2>), gr, dim3(kAdmLanes), 0, st, b);
            else hipLaunchKernelGGL((adm_scale<double, 3>), gr, dim3(kAdmLanes), 0, st, b);
        }
        hipLaunchKernelGGL(adm_finalize, dim3((b.nk * kAdmScales + 63) / 64), dim3(64), 0, st, b);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
