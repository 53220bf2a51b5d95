// PSNR-HVS and PSNR-HVS-M sums of two frame batches (spec PP-HVS-1)
// on gfx950: per distorted frame and plane the contrast-sensitivity-weighted
// squared DCT differences of every 8 x 8 block against the reference frame the
// map names, without (S_hvs) and with (S_hvsm) between-coefficient masking.
//
// New feature after p03 (the reference has no code for it).  The model is the
// published psnrhvsm definition (Ponomarenko et al. 2007) and libvmaf's
// `psnr_hvs` feature as recalled; parity with both is unpinned: neither exists
// to compare with.  The same tables serve all three planes (build-defined: the
// published measure is for grey pictures).
//
// Layout: 8 lanes own a block, a wave 8 blocks, a workgroup (4 waves) the
// kHvsGroupBlocks = 32 consecutive blocks of one block row of one plane of one
// frame: a unit.  32 blocks start 32 step samples apart, 256 or 224: a multiple
// of 16 bytes at either sample width, so a unit's first byte lies on the plane's
// 16-B grid whatever the step.
//   tile:    the unit's 8 rows x 32 pieces of 16 B of both clips go to LDS, one
//            piece of each clip a lane, through load_piece (analysis_dev.hpp:
//            one bounds-checked buffer load on the 16-B grid, sample by sample
//            with the same values elsewhere).  Blocks lie wholly inside the
//            plane; what a piece holds past the row's end is never read by a
//            block that counts.
//   rows:    lane r of a block's 8 reads row r of A and of B from the tile (16
//            doubles), adds the integer sums of the variance ratio from the
//            same samples, and transforms both rows in registers against the
//            cosine matrix as constants, folded by C[k][7 - n] = (-1)^k C[k][n].
//   columns: the 8 x 8 of a block crosses through LDS (a wave's own region);
//            lane l then holds column l and transforms it the same way: it owns
//            the coefficients (k, l), k = 0 .. 7, of both clips.
//   block:   m and the integer sums meet over the 8 lanes by xor 1, 2, 4; every
//            lane then has T and adds its 8 coefficients' terms in k order.
// Reduction: lane -> wave (wave_sum: xor 1, 2, 4 is the block, 8, 16, 32 the
// wave's blocks) -> workgroup (block_gather / block_total, wave order) -> one
// partial (S_hvs, S_hvsm) per unit, no atomics; hvs_finalize adds a plane's
// partials (a wave per frame and plane: lane i the units i, i + 64, .. in that
// order, then wave_sum): bit-reproducible and independent of the layout path.
// Arithmetic: fp64 throughout in the spec's order, contraction off; the fused
// multiply-adds of the transform are the spec's.
#include <algorithm>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kHvsN = 8;              // a block's rows and columns; lanes of a block
constexpr int kHvsWaves = 4;          // waves of a workgroup
constexpr int kHvsGroupBlocks = 32;   // blocks of a unit: 8 a wave
constexpr int kHvsPieces = 32;        // 16-B pieces of a tile row: (31 * 8 + 8) * 2 bytes at most
constexpr int kHvsTilePitch = 528;    // bytes between tile rows in LDS (512 + one piece)
constexpr int kHvsBlockPitch = 72;    // doubles between the blocks of a wave's transpose region (64 + 8)

// C[k][n] = c(k) cos((2n + 1) k pi / 16), n < 4, c(0) = sqrt(1/8), else 1/2: the
// orthonormal 8-point DCT-II; C[k][7 - n] = (-1)^k C[k][n].
constexpr double kHvsC[kHvsN][kHvsN / 2] = {
    {0.3535533905932738, 0.3535533905932738, 0.3535533905932738, 0.3535533905932738},
    {0.4903926402016152, 0.4157348061512726, 0.27778511650980114, 0.09754516100806417},
    {0.46193976625564337, 0.19134171618254492, -0.19134171618254486, -0.46193976625564337},
    {0.4157348061512726, -0.0975451610080641, -0.4903926402016152, -0.2777851165098011},
    {0.3535533905932738, -0.35355339059327373, -0.35355339059327384, 0.3535533905932737},
    {0.27778511650980114, -0.4903926402016152, 0.09754516100806415, 0.41573480615127273},
    {0.19134171618254492, -0.4619397662556434, 0.46193976625564326, -0.19134171618254495},
    {0.09754516100806417, -0.2777851165098011, 0.41573480615127273, -0.4903926402016153},
};

// JPEG Annex K luminance quantisation table.
constexpr int kHvsQ[kHvsN][kHvsN] = {
    {16, 11, 10, 16, 24, 40, 51, 61},     {12, 12, 14, 19, 26, 58, 60, 55},
    {14, 13, 16, 24, 40, 57, 69, 56},     {14, 17, 22, 29, 51, 87, 80, 62},
    {18, 22, 37, 56, 68, 109, 103, 77},   {24, 35, 55, 64, 81, 104, 113, 92},
    {49, 64, 78, 87, 103, 121, 120, 101}, {72, 92, 95, 98, 112, 100, 103, 99},
};

// The published six-decimal contrast-sensitivity table: 25.735088 / Q[k][l]
// rounded to six decimals everywhere but at [0][1], where the publication has
// 2.339554 and the quotient 2.3395535.
constexpr double kHvsCsf[kHvsN][kHvsN] = {
    {1.608443, 2.339554, 2.573509, 1.608443, 1.072295, 0.643377, 0.504610, 0.421887},
    {2.144591, 2.144591, 1.838221, 1.354478, 0.989811, 0.443708, 0.428918, 0.467911},
    {1.838221, 1.979622, 1.608443, 1.072295, 0.643377, 0.451493, 0.372972, 0.459555},
    {1.838221, 1.513829, 1.169777, 0.887417, 0.504610, 0.295806, 0.321689, 0.415082},
    {1.429727, 1.169777, 0.695543, 0.459555, 0.378457, 0.236102, 0.249855, 0.334222},
    {1.072295, 0.735288, 0.467911, 0.402111, 0.317717, 0.247453, 0.227744, 0.279729},
    {0.525206, 0.402111, 0.329937, 0.295806, 0.249855, 0.212687, 0.214459, 0.254803},
    {0.357432, 0.279729, 0.270896, 0.262603, 0.229778, 0.257351, 0.249855, 0.259950},
};

// CSF[k][l] = kHvsCsf[k][l], M[k][l] = (10 / Q[k][l])^2, as the lanes read
// them: [l][k], the 8 coefficients of column l side by side.
struct HvsTables {
    double csf[kHvsN][kHvsN], m[kHvsN][kHvsN];
};
constexpr HvsTables hvs_tables() {
    HvsTables t{};
    for (int k = 0; k < kHvsN; ++k)
        for (int l = 0; l < kHvsN; ++l) {
            const double q = (double)kHvsQ[k][l], r = 10.0 / q;
            t.csf[l][k] = kHvsCsf[k][l];
            t.m[l][k] = r * r;
        }
    return t;
}
__constant__ HvsTables c_hvs = hvs_tables();

struct HvsArgs {
    const uint8_t *ref[3], *dist[3];
    int64_t rls[3], rfs[3], dls[3], dfs[3];
    int ph[3], rb[3];  // rows; bytes of a row that count
    int nbx[3];        // blocks across
    int gx[3];         // units across
    int tile0[3];      // first unit of a plane within a frame
    int tiles;         // units of a frame
    int step;          // 7 or 8
    int nk;            // dist frames of this launch
    double2 *part;     // [nk][tiles]: S_hvs, S_hvsm
    double *out;       // [nk][3][2]
    int32_t idx[kFrameMap];
};

// The 8-point transform of a line: the sums x[n] + x[7 - n] serve the even k,
// the differences the odd ones; term 0 a product, every later one an fma, in n
// order.
__device__ __forceinline__ void hvs_dct8(const double (&x)[kHvsN], double (&y)[kHvsN]) {
    double f[2][kHvsN / 2];
#pragma unroll
    for (int n = 0; n < kHvsN / 2; ++n) {
        f[0][n] = x[n] + x[kHvsN - 1 - n];
        f[1][n] = x[n] - x[kHvsN - 1 - n];
    }
#pragma unroll
    for (int k = 0; k < kHvsN; ++k) {
        double acc = kHvsC[k][0] * f[k & 1][0];
#pragma unroll
        for (int n = 1; n < kHvsN / 2; ++n) acc = __builtin_fma(kHvsC[k][n], f[k & 1][n], acc);
        y[k] = acc;
    }
}

// Sum over the 8 lanes of a block, in every one of them: xor 1, 2, 4 in that order.
template <typename V>
__device__ __forceinline__ V hvs_block_sum(V x) {
#pragma unroll
    for (int o = 1; o < kHvsN; o <<= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// One workgroup per unit of the launch, frame-major.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(64 * kHvsWaves) void hvs_kernel(const HvsArgs a) {
    constexpr int ES = sizeof(T);
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[2][kHvsN][kHvsTilePitch];
    __shared__ double s_tr[kHvsWaves][2][kHvsN * kHvsBlockPitch];
    __shared__ double s_red[kHvsWaves][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x / a.tiles, tile = blockIdx.x - k * a.tiles;
    const int p = plane_of_tile(a.tile0, tile);
    const int u = tile - a.tile0[p];
    const int gy = u / a.gx[p], bx0 = (u - gy * a.gx[p]) * kHvsGroupBlocks;
    const int nblk = min(kHvsGroupBlocks, a.nbx[p] - bx0);  // blocks of this unit
    const int row0 = gy * a.step;
    const int byte0 = bx0 * a.step * ES;  // on the 16-B grid: 32 step ES is 224, 256, 448 or 512
    const int ph = a.ph[p], rb = a.rb[p];

    // the tile: lane (row, piece) loads that piece of both clips
    {
        const uint8_t *base[2] = {a.ref[p] + (int64_t)a.idx[k] * a.rfs[p], a.dist[p] + (int64_t)k * a.dfs[p]};
        const int64_t ls[2] = {a.rls[p], a.dls[p]};
        const int row = tid / kHvsPieces, pc = tid % kHvsPieces;
        const int c = byte0 + pc * 16;
#pragma unroll
        for (int cl = 0; cl < 2; ++cl) {
            const auto rs = plane_rsrc<ALIGNED>(base[cl], ph, ls[cl], rb);
            uint32_t q[4];
            load_piece<T, ALIGNED>(q, rs, base[cl], ls[cl], row0 + row, ph, c, rb, c < rb);
            *reinterpret_cast<uint4 *>(&s_tile[cl][row][pc * 16]) = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
    __syncthreads();

    const int g = lane >> 3, r = lane & 7;  // block of the wave; row, then column, of the block
    const int bi = wave * kHvsN + g;
    const bool valid = bi < nblk;           // the other lanes work on samples that do not count

    double D[2][kHvsN];  // coefficients (k, r) of A and B
    double mask[2];
#pragma unroll
    for (int cl = 0; cl < 2; ++cl) {
        // row r of the block, its sums by half (columns 0 .. 3, 4 .. 7)
        const T *src = reinterpret_cast<const T *>(&s_tile[cl][r][0]) + bi * a.step;
        double x[kHvsN], y[kHvsN];
        uint32_t s[2] = {0, 0};
        uint64_t q[2] = {0, 0};
#pragma unroll
        for (int n = 0; n < kHvsN; ++n) {
            const uint32_t v = src[n];
            x[n] = (double)v;
            s[n >> 2] += v;
            q[n >> 2] += (uint64_t)v * v;
        }
        hvs_dct8(x, y);
        double *tr = s_tr[wave][cl] + g * kHvsBlockPitch;
#pragma unroll
        for (int kk = 0; kk < kHvsN; ++kk) tr[kk * kHvsN + r] = y[kk];
        // variance ratio in integers: xor 1, 2 gives the 4 x 4 quadrants of the lane's half, xor 4 the block
#pragma unroll
        for (int o = 1; o < 4; o <<= 1)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                s[e] += __shfl_xor(s[e], o, 64);
                q[e] += __shfl_xor(q[e], o, 64);
            }
        int64_t vq = 0, S = 0, Q = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            vq += 16 * (int64_t)q[e] - (int64_t)s[e] * (int64_t)s[e];
            S += s[e];
            Q += (int64_t)q[e];
        }
        vq += __shfl_xor(vq, 4, 64);
        S += __shfl_xor(S, 4, 64);
        Q += __shfl_xor(Q, 4, 64);
        const int64_t V = 64 * Q - S * S;
        const double pop = V != 0 ? (double)(21 * vq) / (double)(5 * V) : 0.0;

        __syncthreads();  // the wave's rows have landed (every wave reads its own region)
        double z[kHvsN];
#pragma unroll
        for (int i = 0; i < kHvsN; ++i) z[i] = tr[r * kHvsN + i];
        hvs_dct8(z, D[cl]);

        double m = 0.0;
#pragma unroll
        for (int kk = 0; kk < kHvsN; ++kk) {
            const double t = (D[cl][kk] * D[cl][kk]) * c_hvs.m[r][kk];
            m += (kk == 0 && r == 0) ? 0.0 : t;  // DC does not mask
        }
        m = hvs_block_sum(m);
        mask[cl] = sqrt(m * pop) / 32.0;
    }
    const double thr = fmax(mask[0], mask[1]);

    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < kHvsN; ++kk) {
        const double csf = c_hvs.csf[r][kk];
        const double d = fabs(D[0][kk] - D[1][kk]);
        const double dm = (kk == 0 && r == 0) ? d : fmax(d - thr / c_hvs.m[r][kk], 0.0);
        const double t0 = d * csf, t1 = dm * csf;
        acc[0] += t0 * t0;
        acc[1] += t1 * t1;
    }
    if (!valid) acc[0] = acc[1] = 0.0;
    block_gather(acc, s_red);
    if (tid < 2) {
        double *out = reinterpret_cast<double *>(a.part + (int64_t)k * a.tiles + tile);
        out[tid] = block_total(s_red, tid);
    }
}

// One wave per frame and plane: lane i adds the plane's partials i, i + 64, ..
// in that order, wave_sum adds the lanes'.  A plane without a block gives 0, 0.
__global__ __launch_bounds__(64) void hvs_finalize(const HvsArgs a) {
    const int k = blockIdx.x / 3, p = blockIdx.x - 3 * k;
    const int t0 = a.tile0[p], t1 = p == 2 ? a.tiles : a.tile0[p + 1];
    const double2 *q = a.part + (int64_t)k * a.tiles;
    double s0 = 0.0, s1 = 0.0;
    for (int i = t0 + (int)threadIdx.x; i < t1; i += 64) {
        s0 += q[i].x;
        s1 += q[i].y;
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (threadIdx.x == 0) {
        double *out = a.out + ((int64_t)k * 3 + p) * 2;
        out[0] = s0;
        out[1] = s1;
    }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_psnr_hvs(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *ref, const pp_frames *dist,
                           const int32_t *ref_index, int nref, int ndist, int step, double *out, void *stream) {
    if (!ctx || !ref || !dist || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid || fi.packed) PP_FAIL(PP_ERR_INVALID, "psnr_hvs needs a planar format (got %d)", fmt);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    if (ndist < 0) PP_FAIL(PP_ERR_INVALID, "ndist %d < 0", ndist);
    if (nref < 0) PP_FAIL(PP_ERR_INVALID, "nref %d < 0", nref);
    if (step != 7 && step != 8) PP_FAIL(PP_ERR_INVALID, "step %d (7 or 8)", step);
    const int bytes = fi.depth > 8 ? 2 : 1;
    PairPlanes pl;
    if (int e = check_pair(pl, fmt, w, h, ref, dist)) return e;
    if (int e = check_frame_map(ref_index, ndist, nref, kRefIndexMap)) return e;
    if (ndist == 0) return PP_OK;

    HvsArgs a{};
    put_pair(a, pl);
    for (int p = 0; p < 3; ++p) {
        const PlaneGeom &g = pl.g[p];
        a.ph[p] = g.ph; a.rb[p] = (int)g.rb;
        // blocks of an axis of n samples: origins i step with i step + 8 <= n
        const int nbx = g.pw < kHvsN ? 0 : (g.pw - kHvsN) / step + 1;
        const int nby = g.ph < kHvsN ? 0 : (g.ph - kHvsN) / step + 1;
        a.nbx[p] = nbx;
        a.gx[p] = std::max((nbx + kHvsGroupBlocks - 1) / kHvsGroupBlocks, 1);  // a divisor in the kernel: never 0
        a.tile0[p] = a.tiles;
        a.tiles += nbx ? a.gx[p] * nby : 0;
    }
    a.step = step;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    // the partials of a launch within the workspace budget: its units (the grid) stay below 2^26
    const int per = frames_per_launch(ndist, (int64_t)sizeof(double2) * a.tiles);
    if (int e = grow(ctx->hvs, sizeof(double2) * (size_t)per * a.tiles)) return e;
    a.part = static_cast<double2 *>(ctx->hvs.buf);

    const auto kern = bytes == 2 ? PP_PICK(hvs_kernel, uint16_t, pl.aligned) : PP_PICK(hvs_kernel, uint8_t, pl.aligned);
    each_launch(ndist, per, [&](int k0, int nk) {
        HvsArgs b = a;
        b.nk = nk;
        fill_map(b.idx, ref_index, k0, nk);
        for (int p = 0; p < 3; ++p) b.dist[p] += (int64_t)k0 * a.dfs[p];
        b.out = out + 6 * (int64_t)k0;
        if (a.tiles)  // a frame under 8 samples in a direction has no unit
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)b.nk * a.tiles)), dim3(64 * kHvsWaves), 0, st, b);
        hipLaunchKernelGGL(hvs_finalize, dim3(3 * b.nk), dim3(64), 0, st, b);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
