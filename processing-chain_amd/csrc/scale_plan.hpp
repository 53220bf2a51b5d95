// Scaler planner: pure host arithmetic, no HIP.  Turns FFmpeg's four filter
// banks into the strip / segment / chunk geometry and the index and
// coefficient tables that scale_kernel (scale.hip) and strip_kernel
// (strip.hpp) read without any bounds check.  Built into the library by hipcc
// and into the sanitizer fuzzer (fuzz_host.cpp, `make sanitize`) by plain g++
// -DPIXPATH_HOST_ONLY, which walks the tables on the CPU as the kernels do.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "common.hpp"
#include "filters.hpp"

namespace pp {

constexpr int kTileW = 256;      // widest output tile (columns); narrower for large downscales
constexpr int kThreads = 256;    // 4 waves
constexpr int kLdsBudget = 40 * 1024;
#ifndef PIXPATH_CHO_MAX
#define PIXPATH_CHO_MAX 32
#endif
#ifndef PIXPATH_SEG_ROWS
#define PIXPATH_SEG_ROWS 540
#endif
constexpr int kChoMax = PIXPATH_CHO_MAX;    // output rows per chunk (upper bound)
constexpr int kSegRows = PIXPATH_SEG_ROWS;  // output rows per segment (target; profiles/r2: 540 beats 256 by ~1.5 %)
#ifndef PIXPATH_DIRECT_CHO
#define PIXPATH_DIRECT_CHO 24
#endif
constexpr int kDirectCho = PIXPATH_DIRECT_CHO;  // strip_kernel DIRECT: tallest chunk (output rows)
#ifndef PIXPATH_CHAIN_CHO
#define PIXPATH_CHAIN_CHO 16
#endif
// chain plans: 16-row chunks, so the LDS ring of the second stage still leaves
// 6 workgroups per CU (32-row chunks: 2.73 vs 2.30 ms per 600-frame config-4
// canvas launch, profiles/r2/chain_ab.log)
constexpr int kChainCho = PIXPATH_CHAIN_CHO;
#ifndef PIXPATH_CHAIN_SEG2
#define PIXPATH_CHAIN_SEG2 4
#endif
constexpr int kChainSeg2 = PIXPATH_CHAIN_SEG2;  // second-stage segments of a chain plan's chroma planes
constexpr size_t kChainLdsMax = 64 * 1024;      // a fused chain launch's LDS limit

struct PlaneJob {
    int sw, sh, dw, dh;
    int tiles_x, tiles_y, tile_base;  // strips x vertical segments, first block index
    int tw, twl, seg_h, cho; // strip width (= 1 << twl), output rows per segment, output rows per chunk
    int vtp, ring, maxnew, S; // V tap pairs, window rows (even), staged rows per chunk, staged cols
    int dither_off;       // 0 (Y, U) or 3 (V)
    const int32_t *hpos;  // [dw]   window start (absolute source column)
    const int16_t *hcoef; // [dw * HT]
    const int32_t *vbase; // [dh]   first ring row of the window, rounded down to even
    const int32_t *vcoef2; // [dh * vtp] tap pairs (rows base+2j, base+2j+1) packed lo|hi
    const int32_t *tile_c0, *tile_cn; // [tiles_x] staged column window per strip
    const int32_t *chunk_lo, *chunk_hi; // [ceil(dh/cho)] source rows needed by each chunk
    // strip_kernel only
    const int32_t *hbase4;  // [tiles_x * 64] 8-B aligned window base (staged-row sample) per 4-column lane
    const int32_t *hcoefw;  // [tiles_x * 64][4][HW] taps re-laid over the lane's HW dwords (int16 pairs)
    const int32_t *vrow16;  // [dh][16] per output row: window base row (even), then 8 tap pairs (zero padded)
    // chain plans (strip_kernel FUSE != 0, see strip.hpp)
    int fuse;               // 0 as is, 1 identity second stage, 2 second-stage vertical filter through ring2
    int vtp2;               // second-stage V tap pairs (fuse 2)
    int r2mask;             // fuse 2: rows of the circular byte ring2 - 1 (a power of two)
    const int32_t *vrow2;   // [dh2][16] second-stage row records (base row, tap pairs)
    const int32_t *chunk2;  // [nch][4] per chunk: second-stage rows [lo2, hi2), ring2 base row, kept pairs
    const int32_t *seg2;    // fuse 2: [tiles_y][4] per segment: first-stage rows [y0, y1) (chunk aligned,
                            // overlapping by the second stage's halo), second-stage rows [r0, r1) it stores
    int pk_off, pk_step;    // strip_kernel FUSE == 1: byte offset / step of this plane in the uyvy422 row
};

struct ScaleArgs {
    PlaneJob pl[3];
    const uint8_t *src[3];
    int64_t sls[3], sfs[3];
    uint8_t *dst[3];
    int64_t dls[3], dfs[3];
    int nplanes;
    int tiles;    // workgroups per frame (all planes)
    int hshift;   // 7 for 8-bit sources, depth-1 otherwise
    int dither;   // ordered dither (>8-bit source narrowed to 8 bit)
    int vec_src;  // all source rows 16-B aligned
    int vec_dst;  // all destination rows 8-B aligned (4 outputs per lane)
    int debug;    // ablation (measurement only, PIXPATH_SCALE_DEBUG): 1 no V stores, 2 no staging loads, 4 no H pass
};

// One table of a layout: byte offset into ScaleLayout::blob and its length.
struct Table {
    static constexpr size_t kNone = ~size_t(0);
    size_t off = kNone, bytes = 0;
};

// The table pointers of one PlaneJob, as blob offsets (same names).
struct JobTables {
    Table hpos, hcoef, vbase, vcoef2, tile_c0, tile_cn, chunk_lo, chunk_hi, hbase4, hcoefw, vrow16, vrow2, chunk2, seg2;
};

// Everything the planner decides for one plan.  The jobs' table pointers are
// null until bind() points them at a copy of `blob`: the device allocation
// (what the kernels read) or the blob itself (host code walking the tables).
struct ScaleLayout {
    enum Kind { GENERIC, COPY, INTERLEAVE, GENERIC_UYVY, CHAIN } kind = GENERIC;
    int src_fmt = 0, dst_fmt = 0, sw = 0, sh = 0, dw = 0, dh = 0;
    FmtInfo si{}, di{};
    int csw = 0, csh = 0, cdw = 0, cdh = 0;
    FilterBank f[4];        // hl, hc, vl, vc (FFmpeg layout)
    int ht = 1;             // compiled H-tap bucket
    PlaneJob job[3]{};      // scale_kernel jobs
    size_t lds_bytes = 0;
    PlaneJob fjob[3]{};     // strip_kernel jobs (fast_hw > 0)
    int fast_hw = 0;        // H window dwords of strip_kernel, 0 = generic kernel only
    size_t fast_lds = 0;
    int fast_tw = 256;      // strip_kernel strip width = threads per workgroup (256 or 512)
    int fast_tiles = 0;     // strip_kernel workgroups per frame (all planes)
    size_t fast_lds_plane[2] = {0, 0};  // strip_kernel LDS of the luma / chroma jobs alone
    bool direct = false;    // strip_kernel DIRECT tiling (8-bit source, HW 8): fast_lds = the V ring only
    // CHAIN (plan_chain_layout): this layout is the first stage (-> yuv420p)
    std::unique_ptr<ScaleLayout> stage2;  // yuv420p -> target at the same size (two-launch path)
    int chain_out = 0;                    // target bit depth
    Kind first_kind = GENERIC;            // the first stage's own kind (two-launch path)
    bool chain_fused = false;             // one strip_kernel launch does both stages
    size_t chain_lds = 0;                 // the fused launch's LDS (with `luma`: the chroma launch's)
    // CHAIN, fused, 4:2:0 -> 4:2:2 target: luma's second stage is an identity
    // bank, so luma runs as its own launch of this first-stage plan (config-2
    // tiling: 32-row chunks, no second-stage ring) and the chain launch keeps
    // the chroma planes only -- LDS is sized per launch, so luma no longer
    // takes the 16-row chunks and ring2 LDS the chroma planes need
    std::unique_ptr<ScaleLayout> luma;
    // every table, each padded to 256 B; jtab / ftab locate the tables of job / fjob
    std::vector<uint8_t> blob;
    JobTables jtab[3], ftab[3];
};

// The layout of pp_scale_plan_create / pp_scale_chain_plan_create (same
// arguments and return codes; PP_PLAN_GENERIC in `flags` as there).
int plan_layout(int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh, int flags, double p0, double p1,
                std::unique_ptr<ScaleLayout> *out);
int plan_chain_layout(int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh, int flags, double p0, double p1,
                      std::unique_ptr<ScaleLayout> *out);

// Point every table pointer of L.job / L.fjob at `base` + its offset, `base`
// being a copy of L.blob (256-B aligned on the device).  Nested layouts
// (stage2, luma) have their own blobs and are bound on their own.
void bind(ScaleLayout &L, const void *base);

}  // namespace pp
