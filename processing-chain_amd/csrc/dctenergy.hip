// DCT-energy complexity of a luma sequence (spec PP-DCTE-1) on
// gfx950.  Modelled on the texture energy of the Video Complexity Analyzer
// (Menon et al., 2022); parity with VCA is unpinned: no VCA exists to compare
// with.  The weight formula is VCA's as recalled; the integer transform, its two
// roundings and the brightness are this library's own.  This comment is the
// normative text of the spec.
//
// Input: as pp_motion's: `bitdepth` d of 8 (bytes) or 10 (uint16 LE), w x h,
// pointer / pitch / frame stride, nsrc, an optional index map of n shown
// frames, an optional prev plane with a pitch of its own.  x = min(stored,
// 2^d - 1).  Blocks are the non-overlapping 32 x 32 squares at multiples of 32
// that lie wholly inside the plane: bx = w / 32 across, by = h / 32 down
// (floor), nb = bx by; the ragged right and bottom remainder is not analysed.
// With w < 32 or h < 32 every output is absent (2^64 - 1).
//
// Tables (csrc/dct32_tables.hpp; the committed integers are the spec):
//   C[k][n] = round(4096 s_k cos((2n + 1) k pi / 64)), s_0 = 1 / sqrt 2, else 1:
//             2^14 times the orthonormal 32-point DCT-II
//   W[l][k] = round(256 exp(|((l k) / 1024)^2 - 1|)) <= 696
// Transform of block x[i][n] (signed 32-bit, >> arithmetic):
//   rows:    T[i][k] = (sum_n C[k][n] x[i][n] + 2^(d+3)) >> (d + 4)
//   columns: Y[l][k] = (sum_i C[l][i] T[i][k] + 2^13) >> 14
// so both depths land on one scale, four times the orthonormal transform of
// the 8-bit picture.  The two roundings are fixed points of the spec; between
// them the sums are exact integers and any factorisation gives the same bits.
// Per block b of shown frame k:
//   e_b  = sum over (l, k) != (0, 0) of W[l][k] |Y[l][k]|        dc_b = Y[0][0]
// Per shown frame, out[k][0..2] (uint64):
//   energy = sum_b e_b        dc = sum_b dc_b
//   tdiff  = sum_b |e_b(k) - e_b(k - 1)| against the frame shown before
//            (index[k - 1], or prev for k = 0); absent for k = 0 without prev;
//            a repeated frame gives exactly 0
// and optionally blocks[k][by bx] = e_b, row-major: the spatial complexity map.
// Pooling is host arithmetic (pixpath/dctenergy.py): E = energy / (nb 2^20),
// h = tdiff / (nb 2^20), L = dc / (128 nb) = the mean luma of the covered area
// on the 8-bit scale (VCA's L is a square root of the DC: a stated departure).
//
// Layout: a workgroup (256 lanes, 4 waves) owns kDeBlocks = 8 consecutive
// blocks (row-major) of one frame, a half-wave (32 lanes) one block.
//   rows:    lane i of the half-wave loads row i of its block (two or four
//            16-B pieces through analysis_dev.hpp: bounds-checked buffer loads,
//            element-wise off the 16-B grid with the same results; a block lies
//            wholly inside the plane, so no pitch padding is ever loaded) and
//            folds it by the symmetry C[k][31 - n] = (-1)^k C[k][n]:
//            s[n] = x[n] + x[31 - n] serves the even k, d[n] = x[n] - x[31 - n]
//            the odd ones, 16 multiply-adds each.  The coefficient does not
//            depend on the lane: it comes through scalar loads of a 2 KB
//            constant table (32 x 16 dwords).  T goes to LDS as 16-bit values,
//            two to a dword, a row 17 dwords apart (odd: no bank conflicts).
//   columns: lane k reads column k of T back, folds it the same way, and gives
//            Y[l][k] for l = 0 .. 31, adding W[l][k] |Y[l][k]| as it goes (one
//            dword load a pair of l from the transposed, packed weights).
//            Either pass is a loop of 16 turns, a pair of outputs a turn, kept
//            rolled so that a turn's 32 coefficients are loaded next to their use.
//   e_b:     a butterfly over the half-wave's 32 lanes in 64 bits; lane 0
//            stores e_b and dc_b into the workspace slot of its frame.
// dct_finalize: a workgroup per shown frame adds the blocks' e_b, dc_b and
// |e_b - e_b of the slot before| and copies the e_b to `blocks`.  Slot 0 of a
// launch is the frame shown before its first (prev, or across a launch seam
// index[k0 - 1], analysed again).
//
// Exactness (the sums of |C| are over the committed table, tests/test_dctenergy_host.py):
//   x:       <= 1023 (255): 10 bits
//   fold:    |s|, |d| <= 2046: 12 bits signed
//   rows:    |acc| <= max_k sum_n |C[k][n]| * 1023 = 92672 * 1023 (k = 0) < 2^27;
//            |T| <= (92672 * 1023 + 2^13) >> 14 = 5786 (5769 at 8 bits): 14 bits, LDS holds 16
//   fold:    |s|, |d| <= 11572: 15 bits signed
//   columns: |acc| <= 92672 * 5786 + 2^13 < 2^29; |Y| <= 32727: 17 bits signed
//   (the spec's crude bounds: < 2^27, 8184, < 2^31, 65472).  Every product has
//   both operands in 24 signed bits: v_mad_i32_i24.
//   e:       a term <= 696 * 32727 < 2^25; a lane's 32 terms < 2^30 (32 bits);
//            a block's 1024 < 2^35, a frame's in 64 bits: a plane of < 2^31
//            samples has < 2^21 blocks: < 2^56
// No atomics; integer sums in a fixed order: two runs give the same bits.
#include <algorithm>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"
#include "dct32_tables.hpp"

namespace pp {

constexpr int kDeN = 32;          // a block's rows and columns
constexpr int kDeWaves = 4;       // waves per workgroup
constexpr int kDeBlocks = 8;      // blocks per workgroup: two per wave
constexpr int kDeRowD = 17;       // dwords between rows of T in LDS

// The halves of the tables the symmetry leaves, as the dwords the scalar loads take.
struct DeCoef {
    int32_t c[kDeN][kDeN / 2];    // C[k][n], n < 16
};
struct DeWeight {
    uint32_t w[kDeN / 2][kDeN];   // W[2j][k] | W[2j + 1][k] << 16
};
constexpr DeCoef de_coef() {
    DeCoef t{};
    for (int k = 0; k < kDeN; ++k)
        for (int n = 0; n < kDeN / 2; ++n) t.c[k][n] = kDct32C[k][n];
    return t;
}
constexpr DeWeight de_weight() {
    DeWeight t{};
    for (int j = 0; j < kDeN / 2; ++j)
        for (int k = 0; k < kDeN; ++k) t.w[j][k] = (uint32_t)kDct32W[2 * j][k] | ((uint32_t)kDct32W[2 * j + 1][k] << 16);
    return t;
}
__constant__ DeCoef c_de_coef = de_coef();
__constant__ DeWeight c_de_weight = de_weight();

struct DeArgs {
    const uint8_t *src, *prev;  // prev: the frame shown before frame 0 of the launch (any valid frame if none)
    int64_t ls, fs, pls;
    int h, rb;                  // rows; bytes of a row
    int bx, nb;                 // blocks across; blocks of a plane
    int groups;                 // workgroups of a frame
    int nk;                     // shown frames of this launch
    uint64_t *e;                // [nk + 1][nb]: slot 0 the frame shown before
    int64_t *dc;                // [nk + 1][nb]
    int32_t idx[kFrameMap];     // source frame of shown frame k
};

// sum_{n < 16} C[k][n] f[n]: f the sums (k even) or the differences (k odd) of a folded line.
// One v_mad_i32_i24 a term, the coefficient a scalar operand: left to itself the compiler
// reassociates the chain into two multiplies and a three-way add, half as many again.
__device__ __forceinline__ int de_dot(const int (&f)[kDeN / 2], int k) {
    int acc = __mul24(c_de_coef.c[k][0], f[0]);
#pragma unroll
    for (int n = 1; n < kDeN / 2; ++n)
        asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "s"(c_de_coef.c[k][n]), "v"(f[n]));
    return acc;
}

// One workgroup per (slot, group of kDeBlocks blocks) of the launch, slot-major.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void dct_kernel(const DeArgs a) {
    constexpr int ES = sizeof(T), NPC = kDeN * ES / 16;  // pieces of a block's row
    constexpr int D = ES == 2 ? 10 : 8;
    __shared__ uint32_t s_t[kDeWaves][2][kDeN * kDeRowD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, li = lane & 31;
    const int slot = blockIdx.x / a.groups, group = blockIdx.x - slot * a.groups;
    const int blk = group * kDeBlocks + wave * 2 + half;
    const bool valid = blk < a.nb;
    const int byi = valid ? blk / a.bx : 0, bxi = valid ? blk - byi * a.bx : 0;
    const bool outer = slot == 0;  // the launch's prev, with a pitch of its own
    const uint8_t *base = outer ? a.prev : a.src + (int64_t)a.idx[max(slot - 1, 0)] * a.fs;
    const int64_t ls = outer ? a.pls : a.ls;
    const auto rs = plane_rsrc<ALIGNED>(base, a.h, ls, a.rb);
    uint32_t *const tt = s_t[wave][half];

    // rows: the lane's row of its block, folded
    int f[2][kDeN / 2];
    {
        uint32_t q[NPC][4];
#pragma unroll
        for (int p = 0; p < NPC; ++p)
            load_piece<T, ALIGNED>(q[p], rs, base, ls, byi * kDeN + li, a.h, (bxi * kDeN * ES) + p * 16, a.rb, valid);
        int x[kDeN];
#pragma unroll
        for (int n = 0; n < kDeN; ++n) {
            const uint32_t dw = q[n * ES / 16][(n * ES / 4) & 3];
            if constexpr (ES == 2) x[n] = (int)min((n & 1) ? dw >> 16 : dw & 0xffffu, 1023u);
            else x[n] = (int)((dw >> (8 * (n & 3))) & 0xffu);
        }
#pragma unroll
        for (int n = 0; n < kDeN / 2; ++n) {
            f[0][n] = x[n] + x[kDeN - 1 - n];
            f[1][n] = x[n] - x[kDeN - 1 - n];
        }
    }
    // a pair of outputs a turn, not unrolled: the turn's 32 coefficients are scalar loads that
    // stay next to their use (unrolled, all 512 are hoisted and spilled)
#pragma nounroll
    for (int j = 0; j < kDeN / 2; ++j) {
        const int t0 = (de_dot(f[0], 2 * j) + (1 << (D + 3))) >> (D + 4);
        const int t1 = (de_dot(f[1], 2 * j + 1) + (1 << (D + 3))) >> (D + 4);
        tt[li * kDeRowD + j] = ((uint32_t)t0 & 0xffffu) | ((uint32_t)t1 << 16);
    }
    __syncthreads();  // the block's T has landed

    // columns: column li of T, folded
    {
        int t[kDeN];
#pragma unroll
        for (int i = 0; i < kDeN; ++i) {
            const uint32_t dw = tt[i * kDeRowD + (li >> 1)];
            t[i] = (li & 1) ? (int)dw >> 16 : (int)(dw << 16) >> 16;
        }
#pragma unroll
        for (int i = 0; i < kDeN / 2; ++i) {
            f[0][i] = t[i] + t[kDeN - 1 - i];
            f[1][i] = t[i] - t[kDeN - 1 - i];
        }
    }
    uint32_t sum = 0;
    int y0 = 0;
#pragma nounroll
    for (int j = 0; j < kDeN / 2; ++j) {
        const uint32_t wp = c_de_weight.w[j][li];
        const int ye = (de_dot(f[0], 2 * j) + (1 << 13)) >> 14;
        const int yo = (de_dot(f[1], 2 * j + 1) + (1 << 13)) >> 14;
        uint32_t te = __umul24(wp & 0xffffu, (uint32_t)(ye < 0 ? -ye : ye));
        if (j == 0) {  // uniform
            y0 = ye;
            if (li == 0) te = 0;  // (0, 0) is the DC: it does not count
        }
        sum += te + __umul24(wp >> 16, (uint32_t)(yo < 0 ? -yo : yo));
    }
    unsigned long long e = sum;
#pragma unroll
    for (int o = 1; o < kDeN; o <<= 1) e += __shfl_xor(e, o, 64);  // stays inside the half-wave
    if (valid && li == 0) {
        a.e[(int64_t)slot * a.nb + blk] = e;
        a.dc[(int64_t)slot * a.nb + blk] = y0;
    }
}

// One workgroup per shown frame of the launch: its blocks' sums, the lanes'
// through block_sum; UINT64_MAX for tdiff of a frame without a previous one and
// for everything of a plane without a block.
__global__ __launch_bounds__(256) void dct_finalize(const uint64_t *e, const int64_t *dc, int nb, int first_absent,
                                                    uint64_t *out, uint64_t *blocks) {
    __shared__ unsigned long long s_red[kDeWaves][3];
    const int k = blockIdx.x;
    if (nb == 0) {
        if (threadIdx.x < 3) out[(int64_t)k * 3 + threadIdx.x] = ~uint64_t(0);
        return;
    }
    const uint64_t *cur = e + (int64_t)(k + 1) * nb, *last = e + (int64_t)k * nb;
    const int64_t *cdc = dc + (int64_t)(k + 1) * nb;
    unsigned long long s[3] = {0, 0, 0};
    for (int b = threadIdx.x; b < nb; b += 256) {
        const uint64_t v = cur[b], p = last[b];
        s[0] += v;
        s[1] += (unsigned long long)cdc[b];
        s[2] += v > p ? v - p : p - v;
        if (blocks) blocks[(int64_t)k * nb + b] = v;
    }
    block_sum(s, s_red);
    if (threadIdx.x == 0) {
        out[(int64_t)k * 3 + 0] = s[0];
        out[(int64_t)k * 3 + 1] = s[1];
        out[(int64_t)k * 3 + 2] = (k == 0 && first_absent) ? ~uint64_t(0) : s[2];
    }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_dct_energy(pp_ctx *ctx, int bitdepth, int w, int h, const void *src, int64_t src_linesize,
                             int64_t src_frame_stride, int nsrc, const int32_t *index, int n, const void *prev,
                             int64_t prev_linesize, uint64_t *out, uint64_t *blocks, void *stream) {
    if (!ctx || !src || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    LumaPlanes lp;
    const LumaClip pool{src, src_linesize, src_frame_stride, nsrc}, before{prev, prev_linesize, 0, 1};
    if (int e = luma_checks(lp, bitdepth, w, h, pool, before, true, index, n, kIndexMap)) return e;
    const int es = lp.es;
    if (n == 0) return PP_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    DeArgs a{};
    a.src = static_cast<const uint8_t *>(src);
    a.ls = src_linesize; a.fs = src_frame_stride;
    a.h = h; a.rb = (int)lp.g.rb;
    a.bx = w / kDeN;
    a.nb = a.bx * (h / kDeN);  // 0: no block, every output absent
    a.groups = (a.nb + kDeBlocks - 1) / kDeBlocks;
    const int64_t slot_bytes = (int64_t)a.nb * (sizeof(uint64_t) + sizeof(int64_t));
    // a launch holds its frames' slots and the one before them
    const int per = frames_per_launch(n, slot_bytes, kLaunchWork - slot_bytes);
    if (a.nb) {
        if (int e = grow(ctx->dct, (size_t)slot_bytes * (per + 1))) return e;
        a.e = static_cast<uint64_t *>(ctx->dct.buf);
        a.dc = reinterpret_cast<int64_t *>(a.e + (size_t)(per + 1) * a.nb);
    }
    const auto kern = es == 2 ? PP_PICK(dct_kernel, uint16_t, lp.aligned) : PP_PICK(dct_kernel, uint8_t, lp.aligned);
    each_launch(n, per, [&](int k0, int nk) {
        DeArgs b = a;
        b.nk = nk;
        fill_map(b.idx, index, k0, nk);
        const int first_absent = put_shown_before(b, index, k0, prev, prev_linesize);
        if (a.nb)  // a workgroup per (slot, group): far below 2^31 for planes inside the 2 GiB range and kFrameMap frames
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)(b.nk + 1) * a.groups)), dim3(256), 0, st, b);
        hipLaunchKernelGGL(dct_finalize, dim3(b.nk), dim3(256), 0, st, b.e, b.dc, a.nb, first_absent,
                           out + (int64_t)k0 * 3, blocks ? blocks + (int64_t)k0 * a.nb : nullptr);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
