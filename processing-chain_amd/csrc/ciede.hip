// CIEDE2000 colour difference of two frame batches (spec PP-CIEDE-1)
// on gfx950: per distorted frame the sum and the largest of the dE00 of every
// luma position against the reference frame the map names.
//
// New feature after p03 (the reference has no code for it).  The conversion
// (limited-range BT.709 Y'CbCr -> sRGB-curve linear light -> XYZ D65 -> Lab)
// and the formula (Sharma, Wu, Dalal 2005) are the spec's text; the model is
// libvmaf's `ciede` feature as recalled, parity unpinned: no libvmaf exists to
// compare with.
//
// Layout: a lane owns one 16-B piece of a chroma row (16 samples at 8 bits, 8
// at 10 bits) and the 2^hsub x 2^vsub luma positions of each of its samples:
// 2^hsub luma pieces on each of 2^vsub luma rows.  A wave is 64 such lanes
// across and kCieWaveRows chroma rows down; the 4 waves of a workgroup lie
// below one another, so a unit = (frame, span of 64 chroma pieces, band of
// 4 kCieWaveRows chroma rows).  Per chroma row the lane loads U and V of both
// clips once (4 pieces) and keeps them in registers while it walks its luma
// pieces (2 loads each, both clips); the next luma piece and the next chroma
// row travel while the current piece is worked on.  Every plane sample is
// read once.  Pointers, pitches and frame strides on the 16-B grid: one
// bounds-checked buffer load a piece; elsewhere sample by sample with the same
// values in the same lanes (load_piece, analysis_dev.hpp), so the sums have
// the same bits.  Positions outside the plane are left out by their
// coordinates, never by what the loads return there.
// Arithmetic: fp64 throughout, in the spec's order of operations; the build
// has contraction off.  A pair with equal Y, U and V skips the maths: its dE00
// is exactly 0 either way (every difference is 0 and the square root of 0).
// Reduction: lane (step order, then sample order) -> wave (xor butterfly) ->
// workgroup (LDS, wave order) -> one partial per unit, no atomics;
// ciede_finalize adds a frame's partials in unit order: bit-reproducible and
// independent of the layout path.
#include <algorithm>
#include <cmath>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kCiePieceBytes = 16;  // a lane's piece of a chroma row
constexpr int kCieLanes = 64;       // lanes (chroma pieces) a workgroup is wide: one wave
constexpr int kCieWaves = 4;        // waves of a workgroup, one below the other
constexpr int kCieWaveRows = 4;     // chroma rows a wave walks

struct CiePartial {
    double sum, max;
};

struct CieArgs {
    const uint8_t *ref[3], *dist[3];
    int64_t rls[3], rfs[3], dls[3], dfs[3];
    int w, h, cw, ch;  // luma and chroma plane sizes
    int hsub, vsub;
    int tx, tiles;     // units across; units of a frame
    int nk;            // dist frames of this launch
    double y0, yr, c0, cr;  // 16 s, 219 s, 128 s, 224 s
    double kL, kC, kH;
    CiePartial *part;  // [nk][tiles]
    double *out;       // [nk][2]
    int32_t idx[kFrameMap];
};

constexpr double kCieRad = 0.017453292519943295;  // pi / 180
constexpr double kCieDeg = 57.29577951308232;     // 180 / pi
constexpr double kCie25p7 = 6103515625.0;         // 25^7

struct CieLab {
    double L, a, b;
};

__device__ __forceinline__ double cie_linear(double c) {
    c = fmin(fmax(c, 0.0), 1.0);
    return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
}

__device__ __forceinline__ double cie_f(double t) {
    return t > 216.0 / 24389.0 ? cbrt(t) : (24389.0 / 27.0 * t + 16.0) / 116.0;
}

// Steps 1 .. 5 of PP-CIEDE-1 for one position's code values.
__device__ __forceinline__ CieLab cie_lab(const CieArgs &a, uint32_t Y, uint32_t U, uint32_t V) {
    const double y = ((double)Y - a.y0) / a.yr, cb = ((double)U - a.c0) / a.cr, cr = ((double)V - a.c0) / a.cr;
    const double r = cie_linear(y + 1.5748 * cr);
    const double g = cie_linear((y - 0.1873 * cb) - 0.4681 * cr);
    const double b = cie_linear(y + 1.8556 * cb);
    const double X = ((0.4124564 * r + 0.3575761 * g) + 0.1804375 * b) / 0.95047;
    const double Yl = ((0.2126729 * r + 0.7151522 * g) + 0.0721750 * b) / 1.0;
    const double Z = ((0.0193339 * r + 0.1191920 * g) + 0.9503041 * b) / 1.08883;
    const double fx = cie_f(X), fy = cie_f(Yl), fz = cie_f(Z);
    return {116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)};
}

__device__ __forceinline__ double cie_pow7(double x) {
    const double x2 = x * x, x4 = x2 * x2;
    return (x4 * x2) * x;
}

// atan2(b, a) in degrees within [0, 360); 0 for a = b = 0.
__device__ __forceinline__ double cie_hue(double b, double a) {
    if (a == 0.0 && b == 0.0) return 0.0;
    const double h = atan2(b, a) * kCieDeg;
    return h < 0.0 ? h + 360.0 : h;
}

// Step 6: dE00 of two Lab colours.
__device__ __forceinline__ double cie_de00(const CieLab &p, const CieLab &q, double kL, double kC, double kH) {
    const double C1 = sqrt(p.a * p.a + p.b * p.b), C2 = sqrt(q.a * q.a + q.b * q.b);
    const double Cb7 = cie_pow7((C1 + C2) / 2.0);
    const double G = 0.5 * (1.0 - sqrt(Cb7 / (Cb7 + kCie25p7)));
    const double a1 = (1.0 + G) * p.a, a2 = (1.0 + G) * q.a;
    const double Cp1 = sqrt(a1 * a1 + p.b * p.b), Cp2 = sqrt(a2 * a2 + q.b * q.b);
    const double h1 = cie_hue(p.b, a1), h2 = cie_hue(q.b, a2);
    const double dL = q.L - p.L, dC = Cp2 - Cp1;
    const double CC = Cp1 * Cp2, hs = h1 + h2, hd = h2 - h1;
    double dh, hb;
    if (CC == 0.0) {
        dh = 0.0;
        hb = hs;
    } else {
        dh = hd > 180.0 ? hd - 360.0 : hd < -180.0 ? hd + 360.0 : hd;
        hb = fabs(h1 - h2) <= 180.0 ? hs / 2.0 : hs < 360.0 ? (hs + 360.0) / 2.0 : (hs - 360.0) / 2.0;
    }
    const double dH = 2.0 * sqrt(CC) * sin(dh / 2.0 * kCieRad);
    const double Lb = (p.L + q.L) / 2.0, Cb = (Cp1 + Cp2) / 2.0;
    const double T = (((1.0 - 0.17 * cos((hb - 30.0) * kCieRad)) + 0.24 * cos(2.0 * hb * kCieRad)) +
                      0.32 * cos((3.0 * hb + 6.0) * kCieRad)) -
                     0.20 * cos((4.0 * hb - 63.0) * kCieRad);
    const double e = (hb - 275.0) / 25.0;
    const double dth = 30.0 * exp(-(e * e));
    const double Cq7 = cie_pow7(Cb);
    const double RC = 2.0 * sqrt(Cq7 / (Cq7 + kCie25p7));
    const double l50 = (Lb - 50.0) * (Lb - 50.0);
    const double SL = 1.0 + 0.015 * l50 / sqrt(20.0 + l50);
    const double SC = 1.0 + 0.045 * Cb;
    const double SH = 1.0 + 0.015 * Cb * T;
    const double RT = -sin(2.0 * dth * kCieRad) * RC;
    const double tl = dL / (kL * SL), tc = dC / (kC * SC), th = dH / (kH * SH);
    return sqrt(((tl * tl + tc * tc) + th * th) + RT * tc * th);
}

// Dword d (0 .. 3, lane-varying) of a piece held in registers.
__device__ __forceinline__ uint32_t cie_dword(const uint32_t q[4], int d) {
    return d == 0 ? q[0] : d == 1 ? q[1] : d == 2 ? q[2] : q[3];
}

// Sample i of a piece.
template <typename T>
__device__ __forceinline__ uint32_t cie_sample(const uint32_t q[4], int i) {
    constexpr int EPD = 4 / sizeof(T), BITS = 8 * sizeof(T);
    return (cie_dword(q, i / EPD) >> (BITS * (i % EPD))) & ((1u << BITS) - 1u);
}

// Largest over the 64 lanes of a wave, in every lane.
__device__ __forceinline__ double cie_wave_max(double x) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// One workgroup per unit of the launch, frame-major.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kCieLanes * kCieWaves) void ciede_kernel(const CieArgs a) {
    constexpr int CP = kCiePieceBytes / sizeof(T);  // samples of a piece
    __shared__ double s_red[kCieWaves][1];
    __shared__ double s_max[kCieWaves];

    const int k = blockIdx.x / a.tiles, tile = blockIdx.x - k * a.tiles;
    const int tx = tile % a.tx, band = tile / a.tx;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hs = a.hsub, vs = a.vsub;
    const int piece = tx * kCieLanes + lane;  // of the chroma row; < 2^27 for a plane inside the buffer range
    const int cbyte = piece * kCiePieceBytes;
    const int x0 = (piece * CP) << hs;        // the lane's first luma column
    const int crow0 = (band * kCieWaves + wave) * kCieWaveRows;
    const int nsub = 1 << (hs + vs);          // luma pieces under a chroma piece
    const int nsteps = max(min(kCieWaveRows, a.ch - crow0), 0) * nsub;

    const int rf = a.idx[k];
    const uint8_t *base[2][3];
    int64_t ls[2][3];
    __amdgpu_buffer_rsrc_t rs[2][3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        base[0][p] = a.ref[p] + (int64_t)rf * a.rfs[p];
        base[1][p] = a.dist[p] + (int64_t)k * a.dfs[p];
        ls[0][p] = a.rls[p]; ls[1][p] = a.dls[p];
        const int ph = p ? a.ch : a.h;
        const int64_t rb = (int64_t)(p ? a.cw : a.w) * (int)sizeof(T);
#pragma unroll
        for (int c = 0; c < 2; ++c) rs[c][p] = plane_rsrc<ALIGNED>(base[c][p], ph, ls[c][p], rb);
    }
    const int yrb = a.w * (int)sizeof(T), crb = a.cw * (int)sizeof(T);
    const bool cin = piece * CP < a.cw;

    // U and V of chroma row `row` of both clips: q[clip][U, V]
    auto fetch_chroma = [&](uint32_t (&q)[2][2][4], int row) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int p = 1; p < 3; ++p)
                load_piece<T, ALIGNED>(q[c][p - 1], rs[c][p], base[c][p], ls[c][p], row, a.ch, cbyte, crb, cin);
    };
    // the luma piece of step t of both clips
    auto fetch_luma = [&](uint32_t (&q)[2][4], int t) {
        const int sub = t & (nsub - 1);
        const int row = (((crow0 + (t >> (hs + vs))) << vs) + (sub >> hs));
        const int hp = sub & ((1 << hs) - 1);
        const bool in = x0 + hp * CP < a.w && row < a.h;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            load_piece<T, ALIGNED>(q[c], rs[c][0], base[c][0], ls[c][0], row, a.h, (cbyte << hs) + hp * kCiePieceBytes,
                                   yrb, in);
    };

    double acc[1] = {0.0}, top = 0.0;
    uint32_t nc[2][2][4], cc[2][2][4], ny[2][4], cy[2][4];
    if (nsteps > 0) {
        fetch_chroma(nc, crow0);
        fetch_luma(ny, 0);
    }
#pragma unroll 1
    for (int t = 0; t < nsteps; ++t) {  // uniform
        const int sub = t & (nsub - 1);
        if (sub == 0) {  // a new chroma row: it serves every luma piece below from registers
            __builtin_memcpy(cc, nc, sizeof(cc));
            if (t + nsub < nsteps) fetch_chroma(nc, crow0 + (t >> (hs + vs)) + 1);
        }
        __builtin_memcpy(cy, ny, sizeof(cy));
        if (t + 1 < nsteps) fetch_luma(ny, t + 1);  // travels while this piece is worked on
        const int row = ((crow0 + (t >> (hs + vs))) << vs) + (sub >> hs);
        if (row >= a.h) continue;  // uniform: the odd last luma row's missing partner
        const int hp = sub & ((1 << hs) - 1);
#pragma unroll 1
        for (int i = 0; i < CP; ++i) {
            if (x0 + hp * CP + i >= a.w) break;  // right of the plane (pitch padding is never looked at)
            const int ci = (hp * CP + i) >> hs;  // the chroma sample above this position
            const uint32_t Y1 = cie_sample<T>(cy[0], i), Y2 = cie_sample<T>(cy[1], i);
            const uint32_t U1 = cie_sample<T>(cc[0][0], ci), U2 = cie_sample<T>(cc[1][0], ci);
            const uint32_t V1 = cie_sample<T>(cc[0][1], ci), V2 = cie_sample<T>(cc[1][1], ci);
            if (Y1 == Y2 && U1 == U2 && V1 == V2) continue;  // dE00 = 0: adds +0, leaves the maximum
            const double de = cie_de00(cie_lab(a, Y1, U1, V1), cie_lab(a, Y2, U2, V2), a.kL, a.kC, a.kH);
            acc[0] += de;
            top = fmax(top, de);
        }
    }
    top = cie_wave_max(top);
    if (lane == 0) s_max[wave] = top;
    block_gather(acc, s_red);  // its barrier covers s_max
    if (threadIdx.x == 0) {
        CiePartial *out = a.part + (int64_t)k * a.tiles + tile;
        out->sum = block_total(s_red, 0);
        out->max = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
    }
}

// One lane per frame: its partials in unit order.
__global__ __launch_bounds__(64) void ciede_finalize(const CieArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.nk) return;
    const CiePartial *q = a.part + (int64_t)k * a.tiles;
    double s = 0.0, m = 0.0;
    for (int i = 0; i < a.tiles; ++i) { s += q[i].sum; m = fmax(m, q[i].max); }
    a.out[2 * (int64_t)k] = s;
    a.out[2 * (int64_t)k + 1] = m;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_ciede(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *ref, const pp_frames *dist,
                        const int32_t *ref_index, int nref, int ndist, double kL, double kC, double kH, double *out,
                        void *stream) {
    if (!ctx || !ref || !dist || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid || fi.packed) PP_FAIL(PP_ERR_INVALID, "ciede needs a planar format (got %d)", fmt);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    if (ndist < 0) PP_FAIL(PP_ERR_INVALID, "ndist %d < 0", ndist);
    if (nref < 0) PP_FAIL(PP_ERR_INVALID, "nref %d < 0", nref);
    for (double kw : {kL, kC, kH})
        if (!(kw > 0.0) || !std::isfinite(kw)) PP_FAIL(PP_ERR_INVALID, "weights %g, %g, %g (positive and finite)", kL, kC, kH);
    const int bytes = fi.depth > 8 ? 2 : 1;
    PairPlanes pl;
    if (int e = check_pair(pl, fmt, w, h, ref, dist)) return e;
    if (int e = check_frame_map(ref_index, ndist, nref, kRefIndexMap)) return e;
    if (ndist == 0) return PP_OK;

    CieArgs a{};
    put_pair(a, pl);
    a.w = pl.g[0].pw; a.h = pl.g[0].ph;
    a.cw = pl.g[2].pw; a.ch = pl.g[2].ph;
    a.hsub = fi.hsub; a.vsub = fi.vsub;
    const double s = (double)(1 << (fi.depth - 8));
    a.y0 = 16.0 * s; a.yr = 219.0 * s; a.c0 = 128.0 * s; a.cr = 224.0 * s;
    a.kL = kL; a.kC = kC; a.kH = kH;
    const int span = kCieLanes * (kCiePieceBytes / bytes);  // chroma samples a unit is wide
    const int band = kCieWaves * kCieWaveRows;               // chroma rows it is high
    a.tx = (a.cw + span - 1) / span;
    a.tiles = a.tx * ((a.ch + band - 1) / band);

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    // the partials of a launch within the workspace budget: its units (the grid) stay below 2^26
    const int per = frames_per_launch(ndist, (int64_t)sizeof(CiePartial) * a.tiles);
    if (int e = grow(ctx->cie, sizeof(CiePartial) * (size_t)per * a.tiles)) return e;
    a.part = static_cast<CiePartial *>(ctx->cie.buf);

    const auto kern = bytes == 2 ? PP_PICK(ciede_kernel, uint16_t, pl.aligned) : PP_PICK(ciede_kernel, uint8_t, pl.aligned);
    each_launch(ndist, per, [&](int k0, int nk) {
        CieArgs b = a;
        b.nk = nk;
        fill_map(b.idx, ref_index, k0, nk);
        for (int p = 0; p < 3; ++p) b.dist[p] += (int64_t)k0 * a.dfs[p];
        b.out = out + 2 * (int64_t)k0;
        hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)b.nk * a.tiles)), dim3(kCieLanes * kCieWaves), 0, st, b);
        hipLaunchKernelGGL(ciede_finalize, dim3((b.nk + 63) / 64), dim3(64), 0, st, b);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
