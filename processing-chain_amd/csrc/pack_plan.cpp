// Host side of pack_plan.hpp: the checked geometry the pad / CPVS / stall
// entry points launch with, and pp_pack_arms, which walks a launch's rows,
// chunks and groups with the kernels' own predicates and reports the arms
// taken.  No HIP call in this file.
#include "pack_plan.hpp"

#include <algorithm>

#include "filters.hpp"

namespace pp {

void row_planes(RowPlane *pl, const FmtInfo &fi, const pp_frames *src, const pp_frames *dst, int sframes, int dframes,
                int sw, int sh, int dw, int dh, int x, int y) {
    const int es = fi.depth > 8 ? 2 : 1;
    for (int p = 0; p < 3; ++p) {
        const int hs = p ? fi.hsub : 0, vs = p ? fi.vsub : 0;
        RowPlane &g = pl[p];
        g.src = (const uint8_t *)src->data[p];
        g.sls = src->linesize[p];
        g.sfs = src->frame_stride[p];
        g.dst = (uint8_t *)dst->data[p];
        g.dls = dst->linesize[p];
        g.dfs = dst->frame_stride[p];
        g.W = ceil_rshift(dw, hs);
        g.rows = ceil_rshift(dh, vs);
        g.iw = ceil_rshift(sw, hs);
        g.ih = ceil_rshift(sh, vs);
        g.ox = x >> hs;
        g.oy = y >> vs;
        g.black = (p ? 128 : 16) << (fi.depth - 8);
        g.vec = row_src_vec((uintptr_t)g.src, g.sls, g.sfs, sframes, g.ox, es);
        g.dvec = row_dst_vec((uintptr_t)g.dst, g.dls, g.dfs, dframes);
    }
}

int pad_geometry(int fmt, int sw, int sh, const pp_frames *src, int dw, int dh, int x, int y, const pp_frames *dst,
                 int nframes, PadGeom *g) {
    if (!src || !dst || nframes < 0) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid || fi.packed) PP_FAIL(PP_ERR_INVALID, "pad needs a planar format");
    x = pad_offset(x, dw, sw, fi.hsub);  // (ow-iw)/2, truncated like the expression's int conversion
    y = pad_offset(y, dh, sh, fi.vsub);
    if (pad_exceeds(x, sw, dw) || pad_exceeds(y, sh, dh))
        PP_FAIL(PP_ERR_INVALID, "input %dx%d at (%d,%d) exceeds %dx%d", sw, sh, x, y, dw, dh);
    g->fi = fi;
    g->nframes = nframes;
    g->empty = nframes == 0;
    if (g->empty) return PP_OK;
    row_planes(g->pl, fi, src, dst, nframes, nframes, sw, sh, dw, dh, x, y);
    const int64_t units = (int64_t)nframes * (g->pl[0].rows + g->pl[1].rows + g->pl[2].rows);
    if (units >= ((int64_t)1 << 31)) PP_FAIL(PP_ERR_UNSUPPORTED, "pad: too many rows in one call");
    return PP_OK;
}

int cpvs_geometry(int src_fmt, int w, int h, const pp_frames *src, int W, int H, int x, int y, int out_fmt,
                  const pp_frames *dst, int nframes, CpvsGeom *g) {
    if (!src || !dst || nframes < 0) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(src_fmt);
    if (!fi.valid || fi.packed || fi.hsub != 1) PP_FAIL(PP_ERR_INVALID, "cpvs source must be 4:2:0 or 4:2:2 planar");
    if (out_fmt == PP_FMT_UYVY422 ? fi.depth != 8 : out_fmt == PP_FMT_V210 ? fi.depth != 10 : true)
        PP_FAIL(PP_ERR_INVALID, "cpvs: uyvy422 needs an 8-bit AVPVS, v210 a 10-bit one");
    if (W < w || H < h || (out_fmt == PP_FMT_UYVY422 && (W & 1))) PP_FAIL(PP_ERR_INVALID, "bad canvas %dx%d", W, H);
    // v210enc: "v210 needs even width"; the tail arm has no class for W % 6 in {3, 5}
    if (out_fmt == PP_FMT_V210 && (W & 1)) PP_FAIL(PP_ERR_INVALID, "v210 needs an even width, not %d", W);
    x = pad_offset(x, W, w, fi.hsub);
    y = pad_offset(y, H, h, fi.vsub);
    if (pad_exceeds(x, w, W) || pad_exceeds(y, h, H)) PP_FAIL(PP_ERR_INVALID, "input exceeds the canvas");
    g->v210 = out_fmt == PP_FMT_V210;
    const int64_t line = g->v210 ? v210_linesize(W) : 2LL * W;
    if (dst->linesize[0] < line || !plane_aligned((uintptr_t)dst->data[0], dst->linesize[0], dst->frame_stride[0], nframes))
        PP_FAIL(PP_ERR_INVALID, "cpvs destination must be 16-B aligned with linesize >= %lld", (long long)line);
    g->fi = fi;
    g->nframes = nframes;
    g->empty = nframes == 0;
    if (g->empty) return PP_OK;
    g->w = w; g->h = h; g->cw = ceil_rshift(w, 1); g->ch = ceil_rshift(h, fi.vsub);
    g->W = W; g->H = H; g->ox = x; g->oy = y;
    g->v420 = fi.vsub != 0;
    g->chunks = cpvs_chunks(W, g->v210);
    g->es = fi.depth > 8 ? 2 : 1;
    g->ys = cpvs_lds_stride(w, g->es);
    g->cs = cpvs_lds_stride(g->cw, g->es);
    g->aligned = 1;
    for (int p = 0; p < 3; ++p)
        if (!plane_aligned((uintptr_t)src->data[p], src->linesize[p], src->frame_stride[p], nframes)) g->aligned = 0;
    g->lds = cpvs_lds_bytes(g->ys, g->cs, g->es);
    if (g->lds > kCpvsLdsMax) PP_FAIL(PP_ERR_UNSUPPORTED, "cpvs: AVPVS width %d exceeds the LDS row stage", w);
    if ((int64_t)H * nframes >= (int64_t)1 << 31) PP_FAIL(PP_ERR_UNSUPPORTED, "cpvs: too many rows in one call");
    return PP_OK;
}

int cpvs_vfilter(int H, int *vt, std::vector<int32_t> *pos, std::vector<int16_t> *coef) {
    const int csh = ceil_rshift(H, 1);
    const int inc = (int)((((int64_t)csh << 16) + (H >> 1)) / H);
    FilterBank fb;
    FilterBank::Compact c;
    std::string err;
    if (fb.build(inc, csh, H, 2, 1 << 12, PP_SWS_BICUBIC, PP_SWS_PARAM_DEFAULT, PP_SWS_PARAM_DEFAULT, local_pos(1),
                 local_pos(0), &err) ||
        fb.compact(csh, 1, &c, &err))
        PP_FAIL(PP_ERR_UNSUPPORTED, "cpvs chroma filter: %s", err.c_str());
    if (c.taps > kCpvsTaps) PP_FAIL(PP_ERR_UNSUPPORTED, "cpvs chroma filter of %d taps", c.taps);
    *vt = c.taps;
    pos->assign(c.pos.begin(), c.pos.begin() + H);
    coef->assign(c.coef.begin(), c.coef.end());
    return PP_OK;
}

int stall_geometry(int fmt, int w, int h, const pp_frames *src, const int32_t *src_index, const int32_t *spinner_index,
                   const pp_frames *dst, int nframes, int spin_fmt, int spin_n, int spin_w, int spin_h, StallGeom *g) {
    if (!src || !dst || !src_index || !spinner_index || nframes < 0) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid || fi.packed) PP_FAIL(PP_ERR_INVALID, "stall compose needs a planar format");
    if ((w & ((1 << fi.hsub) - 1)) || (h & ((1 << fi.vsub) - 1))) PP_FAIL(PP_ERR_INVALID, "odd frame size");
    bool need_spin = false;
    for (int k = 0; k < nframes; ++k) need_spin |= spinner_index[k] >= 0;
    if (need_spin && (spin_fmt != fmt || spin_n < 1)) PP_FAIL(PP_ERR_INVALID, "no spinner uploaded for format %d", fmt);
    for (int k = 0; k < nframes; ++k)
        if (spinner_index[k] >= spin_n) PP_FAIL(PP_ERR_INVALID, "spinner index %d out of range", spinner_index[k]);
    g->fi = fi;
    g->nframes = nframes;
    g->empty = nframes == 0;
    if (g->empty) return PP_OK;
    // the kernel indexes source frame si at si * frame stride: the source
    // extent it can reach decides on vector loads, not the output frame count
    int sframes = 0;
    for (int k = 0; k < nframes; ++k) sframes = std::max(sframes, src_index[k] + 1);
    row_planes(g->pl, fi, src, dst, sframes, nframes, w, h, w, h, 0, 0);
    g->sw = need_spin ? spin_w : 0;
    g->sh = need_spin ? spin_h : 0;
    g->ox = pad_offset(-1, w, g->sw, fi.hsub);
    g->oy = pad_offset(-1, h, g->sh, fi.vsub);
    // frames per wave (one source load, G stores of the row).  Round 2,
    // one wave per (row, frame) in tiles of G: G = 1 1.34 ms, 2
    // 1.09-1.12, 3 1.07-1.10, 4 1.12, 6 1.03-1.05, 8 1.33, 16 1.42, 64 1.55
    // (power-of-two tiles alias the frames' rows onto the same HBM channels)
    g->G = PIXPATH_STALL_G;
    return PP_OK;
}

namespace {

inline void arm(uint64_t &m, int a) { m |= (uint64_t)1 << a; }

// source and destination arms of one row of a row kernel, as shifted_chunk / put_chunk take them
void row_arms(uint64_t &m, const RowPlane &g, int n, bool has_row, int ox, int iw, bool load) {
    const int chunks = row_chunks(g.W, n);
    if (chunks > kRowPass) arm(m, PP_ARM_ROW_CHUNKS_GT256);
    for (int q = 0; q < chunks; ++q) {
        const int x = q * n, sx = x - ox;
        if (load) {
            if (!has_row) arm(m, PP_ARM_ROW_SRC_NULL);
            else if (chunk_src_vec(has_row, g.vec, sx, n, iw)) arm(m, PP_ARM_ROW_SRC_VEC);
            else if (!g.vec) arm(m, PP_ARM_ROW_SRC_SCALAR);
            else arm(m, chunk_src_outside(sx, n, iw) ? PP_ARM_ROW_SRC_OUTSIDE : PP_ARM_ROW_SRC_EDGE);
        }
        if (chunk_dst_vec(g.dvec, x, n, g.W)) arm(m, PP_ARM_ROW_DST_VEC);
        else arm(m, g.dvec ? PP_ARM_ROW_DST_TAIL : PP_ARM_ROW_DST_SCALAR);
    }
}

void layout_arm(uint64_t &m, const FmtInfo &fi) {
    arm(m, fi.vsub ? PP_ARM_ROW_420 : fi.hsub ? PP_ARM_ROW_422 : PP_ARM_ROW_444);
}

uint64_t pad_arms(const PadGeom &g) {
    uint64_t m = 0;
    layout_arm(m, g.fi);
    const int n = g.fi.depth > 8 ? 8 : 16;
    for (int p = 0; p < 3; ++p) {
        const RowPlane &pl = g.pl[p];
        for (int y = 0; y < pl.rows; ++y) row_arms(m, pl, n, row_live(y - pl.oy, pl.ih), pl.ox, pl.iw, true);
    }
    return m;
}

uint64_t stall_arms(const StallGeom &g, const int32_t *src_index, const int32_t *spinner_index) {
    uint64_t m = 0;
    layout_arm(m, g.fi);
    const int n = g.fi.depth > 8 ? 8 : 16;
    if (g.nframes > kStallLaunchFrames) arm(m, PP_ARM_STALL_LAUNCH_SPLIT);
    for (int k0 = 0; k0 < g.nframes; k0 += kStallLaunchFrames) {
        const int nk = std::min(kStallLaunchFrames, g.nframes - k0);
        for (int f0 = 0; f0 < nk; f0 += g.G) {
            const int f1 = std::min(nk, f0 + g.G);
            arm(m, f1 - f0 == g.G ? PP_ARM_STALL_TILE_FULL : PP_ARM_STALL_TILE_SHORT);
            for (int p = 0; p < 3; ++p) {
                const RowPlane &pl = g.pl[p];
                const int pw = p ? (g.sw >> g.fi.hsub) : g.sw, ph = p ? (g.sh >> g.fi.vsub) : g.sh;
                const int px0 = p ? (g.ox >> g.fi.hsub) : g.ox, py0 = p ? (g.oy >> g.fi.vsub) : g.oy;
                for (int y = 0; y < pl.rows; ++y) {
                    const bool spin_row = y >= py0 && y < py0 + ph;
                    int cur = -2;
                    for (int f = f0; f < f1; ++f) {
                        const int si = src_index[k0 + f], sp = spinner_index[k0 + f];
                        const bool load = si != cur;
                        if (load && cur != -2) arm(m, PP_ARM_STALL_SRC_CHANGE);
                        cur = si;
                        if (si < 0) arm(m, PP_ARM_STALL_BLACK);
                        row_arms(m, pl, n, si >= 0, 0, pl.W, load);
                        if (sp < 0) {
                            arm(m, PP_ARM_STALL_NO_SPINNER);
                            continue;
                        }
                        if (px0 < 0 || py0 < 0 || px0 + pw > pl.W || py0 + ph > pl.rows) arm(m, PP_ARM_STALL_SPIN_CLIPPED);
                        for (int q = 0; q < row_chunks(pl.W, n); ++q) {
                            const int x = q * n;
                            if (!stall_chunk_blends(spin_row, x, n, px0, pw)) continue;
                            const bool left = !stall_sample_blends(x - px0, pw);
                            const bool right = !stall_sample_blends(x + n - 1 - px0, pw);
                            if (left) arm(m, PP_ARM_STALL_SPIN_LEFT);
                            if (right) arm(m, PP_ARM_STALL_SPIN_RIGHT);
                            if (!left && !right) arm(m, PP_ARM_STALL_SPIN_INSIDE);
                        }
                    }
                }
            }
        }
    }
    return m;
}

int cpvs_arms(const CpvsGeom &g, uint64_t *out) {
    uint64_t m = 0;
    int vt = 1;
    std::vector<int32_t> vpos;
    std::vector<int16_t> vcoef;
    if (g.v420) {
        const int rc = cpvs_vfilter(g.H, &vt, &vpos, &vcoef);
        if (rc) return rc;
    }
    const int depth = g.fi.depth, px = cpvs_px(depth);
    const bool fast8 = cpvs_fast8(depth, g.ox);
    if (g.chunks > kCpvsLanes) arm(m, PP_ARM_CPVS_CHUNKS_GT64);
    for (int y = 0; y < g.H; ++y) {
        const bool live = row_live(y - g.oy, g.h);
        arm(m, live ? PP_ARM_CPVS_ROW_LIVE : PP_ARM_CPVS_ROW_PAD);
        if (live) {
            if (g.aligned) {
                const int total = cpvs_stage_luma(g.ys, g.es) + 2 * cpvs_stage_chroma(g.cs, g.es, g.v420);
                arm(m, total > kCpvsStagePass ? PP_ARM_CPVS_STAGE_VEC_MULTI : PP_ARM_CPVS_STAGE_VEC_ONE);
            } else {
                arm(m, PP_ARM_CPVS_STAGE_SAMPLES);
            }
        }
        if (g.v420) {
            const int coy = g.oy >> 1, ngroups = cpvs_groups(g.cw);
            if (ngroups > kCpvsLanes) arm(m, PP_ARM_CPVS_GROUPS_GT64);
            for (int k = 0; k < kCpvsTaps; ++k) {
                const int r = vpos[y] + k - coy;
                if (!cpvs_tap_in(k, vt, r, g.ch)) {
                    if (k < vt) arm(m, r < 0 ? PP_ARM_CPVS_TAP_ABOVE : PP_ARM_CPVS_TAP_BELOW);
                    continue;
                }
                for (int gr = 0; gr < ngroups; ++gr) {
                    if (cpvs_group_vec(g.aligned)) {
                        arm(m, gr < g.cs / 8 ? PP_ARM_CPVS_GROUP_VEC : PP_ARM_CPVS_GROUP_VEC_RAGGED);
                    } else {
                        arm(m, PP_ARM_CPVS_GROUP_SAMPLES);
                        if (cpvs_group_clamped(gr, g.cw)) arm(m, PP_ARM_CPVS_GROUP_CLAMPED);
                    }
                }
            }
        }
        for (int q = 0; q < g.chunks; ++q) {
            const int x0 = q * px;
            if (depth == 8) {
                if (cpvs_fast8_chunk(fast8, live, x0, g.ox, g.w, g.cw, g.W)) arm(m, PP_ARM_CPVS_C8_FAST);
                else if (cpvs_fast8_chunk(true, live, x0, g.ox, g.w, g.cw, g.W)) arm(m, PP_ARM_CPVS_C8_OFFGRID);
                else arm(m, uyvy_chunk_full(x0, g.W) ? PP_ARM_CPVS_C8_SLOW_FULL : PP_ARM_CPVS_C8_SLOW_TAIL);
            } else {
                static const int cls[] = {PP_ARM_CPVS_V210_FULL, PP_ARM_CPVS_V210_TAIL2, PP_ARM_CPVS_V210_TAIL4,
                                          PP_ARM_CPVS_V210_ZERO};
                arm(m, cls[v210_chunk(q, g.W)]);
            }
        }
    }
    *out = m;
    return PP_OK;
}

}  // namespace
}  // namespace pp

using namespace pp;

extern "C" int pp_pack_arms(const pp_pack_query *q, uint64_t *arms) {
    if (!q || !arms) PP_FAIL(PP_ERR_INVALID, "null argument");
    *arms = 0;
    switch (q->op) {
    case PP_PACK_OP_PAD: {
        PadGeom g;
        const int rc = pad_geometry(q->fmt, q->w, q->h, &q->src, q->W, q->H, q->x, q->y, &q->dst, q->nframes, &g);
        if (rc) return rc;
        if (!g.empty) *arms = pad_arms(g);
        return g.fi.depth > 8 ? PP_PACK_INST_PAD16 : PP_PACK_INST_PAD8;
    }
    case PP_PACK_OP_CPVS:
    case PP_PACK_OP_V210: {
        CpvsGeom g;
        int rc;
        if (q->op == PP_PACK_OP_V210) {
            // pp_v210_pack's own checks, then the fused pass with the canvas = the frame
            if (q->w < 1 || q->h < 1 || q->nframes < 0) PP_FAIL(PP_ERR_INVALID, "bad argument");
            if (q->dst.linesize[0] < v210_linesize(q->w) ||
                !plane_aligned((uintptr_t)q->dst.data[0], q->dst.linesize[0], q->dst.frame_stride[0], q->nframes))
                PP_FAIL(PP_ERR_INVALID, "v210 destination must be 16-B aligned with linesize >= %lld",
                        (long long)v210_linesize(q->w));
            rc = cpvs_geometry(PP_FMT_YUV422P10LE, q->w, q->h, &q->src, q->w, q->h, 0, 0, PP_FMT_V210, &q->dst,
                               q->nframes, &g);
        } else {
            const FmtInfo fi = fmt_info(q->fmt);
            rc = cpvs_geometry(q->fmt, q->w, q->h, &q->src, q->W, q->H, q->x, q->y,
                               fi.depth > 8 ? PP_FMT_V210 : PP_FMT_UYVY422, &q->dst, q->nframes, &g);
        }
        if (rc) return rc;
        if (!g.empty && (rc = cpvs_arms(g, arms))) return rc;
        return g.fi.depth > 8 ? (g.fi.vsub ? PP_PACK_INST_CPVS10_420 : PP_PACK_INST_CPVS10_422)
                              : (g.fi.vsub ? PP_PACK_INST_CPVS8_420 : PP_PACK_INST_CPVS8_422);
    }
    case PP_PACK_OP_STALL: {
        StallGeom g;
        const int rc = stall_geometry(q->fmt, q->w, q->h, &q->src, q->src_index, q->spinner_index, &q->dst, q->nframes,
                                      q->spin_n > 0 ? q->fmt : -1, q->spin_n, q->spin_w, q->spin_h, &g);
        if (rc) return rc;
        if (!g.empty) *arms = stall_arms(g, q->src_index, q->spinner_index);
        return g.fi.depth > 8 ? PP_PACK_INST_STALL16 : PP_PACK_INST_STALL8;
    }
    default: PP_FAIL(PP_ERR_INVALID, "unknown pack operation %d", q->op);
    }
}
