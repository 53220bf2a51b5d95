// Scaler planner (host only): see scale_plan.hpp.  scale.hip has the reference
// semantics and the strip-streaming design these tables serve.
#include "scale_plan.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace pp {
namespace {

struct HostPlane {
    FilterBank::Compact h, v;
    std::vector<int32_t> c0, cn, lo, hi;
    std::vector<int32_t> vbase, vcoef2;  // V window as even-aligned row pairs
    int vtp = 1;
    int tiles_x = 0, nseg = 0, tw = 0, seg_h = 0, cho = 0, ring = 0, maxnew = 0, S = 0;
    // strip_kernel layout (its own strip width f_tw: column windows f_c0 / f_cn)
    std::vector<int32_t> hbase4, hcoefw, vrow16, f_c0, f_cn;
    int hw_need = 0, max_base = 0, S_fast = 0, f_tw = 256, f_tiles_x = 0, f_S = 0;
};

// Vertical taps regrouped as row pairs starting at an even row (the ring keeps
// row pairs interleaved, so one 32-bit LDS word is a v_dot2 operand).  An odd
// window start gets a leading zero tap; trailing zeros are dropped.
void pair_rows(HostPlane &hp) {
    const auto &v = hp.v;
    const int n = (int)v.pos.size();
    int vtp = 1;
    for (int i = 0; i < n; ++i) {
        int last = 0;
        for (int k = 0; k < v.taps; ++k)
            if (v.coef[(size_t)i * v.taps + k]) last = k;
        vtp = std::max(vtp, ((v.pos[i] & 1) + last + 2) / 2);
    }
    hp.vtp = vtp;
    hp.vbase.assign(n, 0);
    hp.vcoef2.assign((size_t)n * vtp, 0);
    for (int i = 0; i < n; ++i) {
        const int odd = v.pos[i] & 1;
        hp.vbase[i] = v.pos[i] - odd;
        auto tap = [&](int k) -> uint16_t {
            return (k >= 0 && k < v.taps) ? (uint16_t)v.coef[(size_t)i * v.taps + k] : 0;
        };
        for (int j = 0; j < vtp; ++j)
            hp.vcoef2[(size_t)i * vtp + j] =
                (int32_t)((uint32_t)tap(2 * j - odd) | ((uint32_t)tap(2 * j + 1 - odd) << 16));
    }
}

// Column window of every strip for a strip width.
int col_windows(HostPlane &hp, int sw, int dw, int tw) {
    const int tiles_x = (dw + tw - 1) / tw;
    hp.c0.assign(tiles_x, 0);
    hp.cn.assign(tiles_x, 0);
    int S = 0;
    for (int tx = 0; tx < tiles_x; ++tx) {
        int lo = sw, hi = 0;
        for (int x = tx * tw; x < std::min(dw, (tx + 1) * tw); ++x) {
            lo = std::min(lo, hp.h.pos[x]);
            hi = std::max(hi, hp.h.pos[x] + hp.h.taps);
        }
        lo &= ~15;
        const int n = (hi - lo + 15) & ~15;
        hp.c0[tx] = lo;
        hp.cn[tx] = n;
        S = std::max(S, n);
    }
    return S;
}

// Row windows per chunk of `cho` output rows; returns (max new rows per chunk, ring rows).
void row_chunks(HostPlane &hp, int sh, int dh, int cho, int seg_h, int *maxnew, int *ring) {
    const int nch = (dh + cho - 1) / cho;
    hp.lo.assign(nch, 0);
    hp.hi.assign(nch, 0);
    for (int ci = 0; ci < nch; ++ci) {
        int lo = sh, hi = 0;
        for (int y = ci * cho; y < std::min(dh, (ci + 1) * cho); ++y) {
            lo = std::min(lo, hp.v.pos[y]);
            hi = std::max(hi, hp.v.pos[y] + hp.v.taps);
        }
        hp.lo[ci] = lo;
        hp.hi[ci] = hi;
    }
    // simulate the kernel's walk to size the staging buffer
    int mn = 0;
    for (int y0 = 0; y0 < dh; y0 += seg_h) {
        int next = hp.lo[y0 / cho];
        for (int y = y0; y < std::min(dh, y0 + seg_h); y += cho) {
            const int ci = y / cho;
            if (next < hp.lo[ci]) next = hp.lo[ci];
            mn = std::max(mn, hp.hi[ci] - next);
            next = std::max(next, hp.hi[ci]);
        }
    }
    // window rows: from the chunk's even base to its last staged row or the
    // last row pair its vertical taps read (zero-weight taps included)
    int wr = 2;
    for (int ci = 0; ci < nch; ++ci) {
        const int b = hp.lo[ci] & ~1;
        int top = hp.hi[ci];
        for (int y = ci * cho; y < std::min(dh, (ci + 1) * cho); ++y) top = std::max(top, hp.vbase[y] + 2 * hp.vtp);
        wr = std::max(wr, top - b);
    }
    *maxnew = std::max(mn, 1);
    *ring = (wr + 1) & ~1;
}

// LDS budget per workgroup in bytes (PIXPATH_SCALE_LDS_KB overrides, measurement only)
size_t lds_budget() {
    const char *e = PP_KNOB("PIXPATH_SCALE_LDS_KB");
    return e ? (size_t)std::max(8, std::min(160, atoi(e))) * 1024 : (size_t)kLdsBudget;
}

// Strip width / chunk height / segments for one plane: the widest strip and
// tallest chunk whose LDS (staging + ring) fits the budget; ~256-row segments.
int plan_tiles(HostPlane &hp, int sw, int sh, int dw, int dh, size_t *lds, std::string *err, int seg_force = 0,
               int cho_force = 0, bool ring_only = false) {
    static const int tws[] = {256, 128, 64, 32};
    static const int chos[] = {64, 48, 32, 24, 16, 8, 4, 2, 1};
    // tuning overrides (measurement only): tallest chunk, rows per segment
    const char *e_cho = PP_KNOB("PIXPATH_SCALE_CHO_MAX"), *e_seg = PP_KNOB("PIXPATH_SCALE_SEG_ROWS");
    const int cho_max = e_cho ? std::max(1, atoi(e_cho)) : cho_force > 0 ? cho_force : kChoMax;
    const int seg_rows = seg_force > 0 ? seg_force : e_seg ? std::max(1, atoi(e_seg)) : kSegRows;
    for (int tw : tws) {
        if (tw > 32 && tw / 2 >= dw) continue;  // narrower strips suffice for this plane
        const int S = col_windows(hp, sw, dw, tw);
        for (int cho : chos) {
            if (cho > cho_max) continue;
            int nseg = std::max(1, (dh + seg_rows / 2) / seg_rows);
            int seg_h = (dh + nseg - 1) / nseg;
            seg_h = (seg_h + cho - 1) / cho * cho;
            nseg = (dh + seg_h - 1) / seg_h;
            int maxnew, ring;
            row_chunks(hp, sh, dh, cho, seg_h, &maxnew, &ring);
            // ring_only: strip_kernel DIRECT, whose LDS is the V window ring alone
            const size_t bytes = ring_only ? (size_t)ring * tw * 2
                                           : (size_t)maxnew * S * 2 + (size_t)ring * tw * 2 + (size_t)cho * hp.vtp * 4 +
                                                 (size_t)cho * 4;
            if (bytes > lds_budget()) continue;
            hp.tiles_x = (dw + tw - 1) / tw;
            hp.nseg = nseg; hp.tw = tw; hp.seg_h = seg_h; hp.cho = cho;
            hp.ring = ring; hp.maxnew = maxnew; hp.S = S;
            *lds = std::max(*lds, bytes);
            return 0;
        }
    }
    *err = "scale ratio too large for the LDS budget";
    return -1;
}

// strip_kernel column windows for its strip width tw (256 or 512)
void fast_tiling(HostPlane &hp, int sw, int dw, int tw) {
    std::vector<int32_t> c0 = hp.c0, cn = hp.cn;  // the generic tiling's, kept
    hp.f_S = col_windows(hp, sw, dw, tw);
    hp.f_c0.swap(hp.c0);
    hp.f_cn.swap(hp.cn);
    hp.c0.swap(c0);
    hp.cn.swap(cn);
    hp.f_tw = tw;
    hp.f_tiles_x = (dw + tw - 1) / tw;
}

// strip_kernel windows: per 4-column lane group, an 8-B aligned base in the
// staged row and the dwords that hold every non-zero tap of its 4 outputs.
void fast_windows(HostPlane &hp, int dw) {
    const int taps = hp.h.taps, gpt = hp.f_tw / 4;
    hp.hbase4.assign((size_t)hp.f_tiles_x * gpt, 0);
    hp.hw_need = 1;
    hp.max_base = 0;
    for (int tx = 0; tx < hp.f_tiles_x; ++tx)
        for (int g = 0; g < gpt; ++g) {
            int lo = INT32_MAX, end = 0;
            for (int j = 0; j < 4; ++j) {
                const int x = tx * hp.f_tw + 4 * g + j;
                if (x >= dw) break;
                const int16_t *c = &hp.h.coef[(size_t)x * taps];
                for (int k = 0; k < taps; ++k)
                    if (c[k]) {
                        lo = std::min(lo, hp.h.pos[x] + k);
                        end = std::max(end, hp.h.pos[x] + k + 1);
                    }
            }
            if (lo == INT32_MAX) continue;
            const int base = (lo - hp.f_c0[tx]) & ~3;
            hp.hbase4[(size_t)tx * gpt + g] = base;
            hp.hw_need = std::max(hp.hw_need, (end - hp.f_c0[tx] - base + 1) / 2);
            hp.max_base = std::max(hp.max_base, base);
        }
}

// Taps of every output re-laid over its lane group's HW dwords (zero elsewhere).
void fast_coefs(HostPlane &hp, int dw, int HW) {
    const int taps = hp.h.taps, gpt = hp.f_tw / 4;
    hp.hcoefw.assign((size_t)hp.f_tiles_x * gpt * 4 * HW, 0);
    uint16_t *h16 = reinterpret_cast<uint16_t *>(hp.hcoefw.data());
    for (int tx = 0; tx < hp.f_tiles_x; ++tx)
        for (int g = 0; g < gpt; ++g)
            for (int j = 0; j < 4; ++j) {
                const int x = tx * hp.f_tw + 4 * g + j;
                if (x >= dw) break;
                const int base = hp.hbase4[(size_t)tx * gpt + g];
                for (int k = 0; k < taps; ++k) {
                    const int16_t c = hp.h.coef[(size_t)x * taps + k];
                    if (!c) continue;
                    // in [0, 2*HW): fast_windows sized hw_need <= HW for it (fuzz_host.cpp checks)
                    const int s = hp.h.pos[x] + k - hp.f_c0[tx] - base;
                    h16[(((size_t)tx * gpt + g) * 4 + j) * HW * 2 + s] = (uint16_t)c;
                }
            }
    // per output row: window base row, then the V tap pairs padded to 8
    const int n = (int)hp.vbase.size();
    hp.vrow16.assign((size_t)n * 16, 0);
    for (int i = 0; i < n; ++i) {
        hp.vrow16[(size_t)i * 16] = hp.vbase[i];
        for (int j = 0; j < hp.vtp; ++j) hp.vrow16[(size_t)i * 16 + 1 + j] = hp.vcoef2[(size_t)i * hp.vtp + j];
    }
}

// strip_kernel packs an H row pair with v_cvt_pk_i16_i32, whose saturation
// stands in for hScale*To15's FFMIN(val >> sh, 32767): exact only if no output
// can fall below -32768 (the most negative sum: every negative tap on a
// full-scale sample).  Plans that could are left to scale_kernel.
bool strip_h_sat_ok(const HostPlane &hp, int depth) {
    const int64_t maxs = (1 << depth) - 1;
    const int sh = depth == 8 ? 7 : depth - 1;
    const int taps = hp.h.taps, n = (int)hp.h.pos.size();
    for (int x = 0; x < n; ++x) {
        int64_t neg = 0;
        for (int k = 0; k < taps; ++k) neg += std::min<int64_t>(0, hp.h.coef[(size_t)x * taps + k]);
        if ((neg * maxs) >> sh < -32768) return false;
    }
    return true;
}

int hw_bucket(int need) {
    static const int b[] = {3, 4, 5, 6, 8, 10, 12, 16};
    for (int v : b)
        if (need <= v) return v;
    return -1;
}

int ht_bucket(int t) {
    static const int b[] = {1, 2, 4, 6, 8, 12, 16, 24, 32};
    for (int v : b)
        if (t <= v) return v;
    return -1;
}

// An FFmpeg "unscaled" filter bank (initFilter's |xInc - 0x10000| < 10 case):
// output i takes input i with the single tap `one`.
bool identity_bank(const FilterBank &f, int one) {
    for (int i = 0; i < f.n; ++i)
        for (int j = 0; j < f.size; ++j) {
            const int16_t c = f.coef[(size_t)i * f.size + j];
            if (f.pos[i] + j == i ? c != one : c != 0) return false;
        }
    return true;
}

// Append a table to the blob (entries padded to 256 B, the alignment the
// kernels' vector and scalar table loads assume).
template <typename T>
Table put(ScaleLayout &L, const std::vector<T> &v) {
    Table t;
    t.off = L.blob.size();
    t.bytes = v.size() * sizeof(T);
    L.blob.resize(t.off + ((t.bytes + 255) & ~size_t(255)), 0);
    if (t.bytes) std::memcpy(L.blob.data() + t.off, v.data(), t.bytes);
    return t;
}

// strip_kernel eligibility: the generic tiling fits 256-column strips,
// <= 8 V tap pairs, one H window bucket for both planes, single-pass
// staging, LDS within the budget.  Strip width 256; PIXPATH_STRIP_TW=512
// (plain plans only, measurement) runs 512-column strips with 8 waves and
// twice the LDS budget -- measured slower on every config (config 2
// 1.554 vs 1.501 ms, config 3 10-bit 5.17 vs 4.87 ms, 8-bit 3.57 vs
// 3.25 ms per 600-frame launch; profiles/r3/strip_tw_ab.txt).
void plan_strip(ScaleLayout &L, HostPlane hp[2], bool force_generic, bool one_seg_chroma) {
    const char *etw = PP_KNOB("PIXPATH_STRIP_TW");
    bool ok0 = !force_generic;
    const int CH = L.si.depth > 8 ? 8 : 16;
    for (int c = 0; c < 2 && ok0; ++c) ok0 = hp[c].tw == kTileW && hp[c].vtp <= 8 && strip_h_sat_ok(hp[c], L.si.depth);
    const int tw_first = (etw && atoi(etw) == 512 && !one_seg_chroma && !L.di.packed) ? 512 : 256;
    for (int ftw = tw_first; ok0 && ftw >= 256; ftw /= 2) {
        bool ok = true;
        int need = 1;
        for (int c = 0; c < 2 && ok; ++c) {
            fast_tiling(hp[c], c ? L.csw : L.sw, c ? L.cdw : L.dw, ftw);
            for (int v : hp[c].f_cn) ok = ok && (v + CH - 1) / CH <= ftw;
            if (!ok) break;
            fast_windows(hp[c], c ? L.cdw : L.dw);
            need = std::max(need, hp[c].hw_need);
        }
        const int HW = ok ? hw_bucket(need) : -1;
        size_t lds = 0;
        for (int c = 0; c < 2 && HW > 0; ++c) {
            fast_coefs(hp[c], c ? L.cdw : L.dw, HW);
            hp[c].S_fast = std::max(hp[c].f_S, (hp[c].max_base + 2 * HW + 15) & ~15);
            L.fast_lds_plane[c] = (size_t)hp[c].maxnew * hp[c].S_fast * 2 + (size_t)hp[c].ring * ftw * 2;
            lds = std::max(lds, L.fast_lds_plane[c]);
        }
        if (HW > 0 && lds <= lds_budget() * (size_t)(ftw / 256)) {
            L.fast_hw = HW;
            L.fast_lds = lds;
            L.fast_tw = ftw;
            break;
        }
    }
}

// strip_kernel DIRECT (8-bit sources, 8-dword windows, plain plans: the
// 2:1 downscales of config 3): no staged rows, so the chunks are chosen
// for the V window ring alone -- its own row tiling and chunk tables
// (24-row chunks: 2.73 ms per 600-frame config-3 8-bit launch, against
// 3.04 at the staged plan's 8 rows and 2.76 at 32, profiles/r5/)
void plan_direct(ScaleLayout &L, const HostPlane hp[2], HostPlane hpd[2], bool allowed) {
    if (L.fast_hw != 8 || L.si.depth != 8) return;
    bool okd = allowed && !L.di.packed && L.fast_tw == 256;
    size_t dl = 0;
    std::string err;
    for (int c = 0; c < 2 && okd; ++c) {
        hpd[c] = hp[c];
        size_t tmp = 0;
        okd = plan_tiles(hpd[c], c ? L.csw : L.sw, c ? L.csh : L.sh, c ? L.cdw : L.dw, c ? L.cdh : L.dh, &tmp, &err, 0,
                         kDirectCho, true) == 0 && hpd[c].tw == 256;
        dl = std::max(dl, (size_t)hpd[c].ring * 256 * 2);
    }
    if (okd) {
        L.direct = true;
        L.fast_lds = dl;
    }
}

// launch geometry of every plane: scale_kernel jobs, then strip_kernel's with
// its own strip width (and the DIRECT row tiling)
void fill_jobs(ScaleLayout &L, const HostPlane hp[2], const HostPlane hpd[2]) {
    int base = 0;
    for (int p = 0; p < 3; ++p) {
        const int c = p ? 1 : 0;
        PlaneJob &J = L.job[p];
        J.sw = c ? L.csw : L.sw; J.sh = c ? L.csh : L.sh;
        J.dw = c ? L.cdw : L.dw; J.dh = c ? L.cdh : L.dh;
        J.tiles_x = hp[c].tiles_x; J.tiles_y = hp[c].nseg; J.tw = hp[c].tw;
        J.twl = 0;
        while ((1 << J.twl) < J.tw) ++J.twl;
        J.seg_h = hp[c].seg_h; J.cho = hp[c].cho;
        J.tile_base = base;
        base += J.tiles_x * J.tiles_y;
        J.vtp = hp[c].vtp; J.ring = hp[c].ring; J.maxnew = hp[c].maxnew; J.S = hp[c].S;
        J.dither_off = p == 2 ? 3 : 0;
    }
    int fbase = 0;
    for (int p = 0; p < 3; ++p) {
        const int c = p ? 1 : 0;
        PlaneJob &F = L.fjob[p];
        F = L.job[p];
        F.S = hp[c].S_fast;
        if (L.fast_hw) {
            F.tiles_x = hp[c].f_tiles_x;
            F.tw = L.fast_tw;
            F.twl = L.fast_tw == 512 ? 9 : 8;
        }
        if (L.direct) {
            F.tiles_y = hpd[c].nseg; F.seg_h = hpd[c].seg_h; F.cho = hpd[c].cho;
            F.ring = hpd[c].ring; F.maxnew = 0;
        }
        F.tile_base = fbase;
        fbase += F.tiles_x * F.tiles_y;
    }
    L.fast_tiles = fbase;
}

// every table into the blob; the strip jobs share the generic jobs' tables but
// for their own column windows and (DIRECT) chunk rows
void pack_tables(ScaleLayout &L, const HostPlane hp[2], const HostPlane hpd[2]) {
    JobTables t[2], f[2];
    for (int c = 0; c < 2; ++c) {
        t[c].hpos = put(L, hp[c].h.pos);
        t[c].hcoef = put(L, hp[c].h.coef);
        t[c].vbase = put(L, hp[c].vbase);
        t[c].vcoef2 = put(L, hp[c].vcoef2);
        t[c].tile_c0 = put(L, hp[c].c0);
        t[c].tile_cn = put(L, hp[c].cn);
        t[c].chunk_lo = put(L, hp[c].lo);
        t[c].chunk_hi = put(L, hp[c].hi);
        if (L.fast_hw) {
            t[c].hbase4 = put(L, hp[c].hbase4);
            t[c].hcoefw = put(L, hp[c].hcoefw);
            t[c].vrow16 = put(L, hp[c].vrow16);
        }
        f[c] = t[c];
        if (L.fast_hw) {
            f[c].tile_c0 = put(L, hp[c].f_c0);
            f[c].tile_cn = put(L, hp[c].f_cn);
        }
        if (L.direct) {
            f[c].chunk_lo = put(L, hpd[c].lo);
            f[c].chunk_hi = put(L, hpd[c].hi);
        }
    }
    for (int p = 0; p < 3; ++p) {
        L.jtab[p] = t[p ? 1 : 0];
        L.ftab[p] = f[p ? 1 : 0];
    }
}

// one_seg_chroma: chroma planes walk their whole height in one segment (the
// chain plan's second-stage vertical filter follows the first stage's rows)
int plan_one(int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh, int flags, double p0, double p1,
             bool one_seg_chroma, std::unique_ptr<ScaleLayout> *out, int cho_max = 0, bool allow_direct = true) {
    if (!out) PP_FAIL(PP_ERR_INVALID, "null argument");
    out->reset();
    const bool force_generic = (flags & PP_PLAN_GENERIC) != 0;
    flags &= ~PP_PLAN_GENERIC;
    FmtInfo si = fmt_info(src_fmt), di = fmt_info(dst_fmt);
    if (!si.valid || si.packed) PP_FAIL(PP_ERR_INVALID, "source format %d must be planar YUV", src_fmt);
    if (!di.valid || dst_fmt == PP_FMT_V210) PP_FAIL(PP_ERR_INVALID, "destination format %d unsupported", dst_fmt);
    if (sw < 4 || sh < 4 || dw < 1 || dh < 1 || sw > 16384 || sh > 16384 || dw > 16384 || dh > 16384)
        PP_FAIL(PP_ERR_INVALID, "bad dimensions %dx%d -> %dx%d", sw, sh, dw, dh);
    if (!(flags & (PP_SWS_BICUBIC | PP_SWS_LANCZOS | PP_SWS_BILINEAR)))
        PP_FAIL(PP_ERR_UNSUPPORTED, "flags 0x%x: only bicubic, lanczos, bilinear", flags);

    std::unique_ptr<ScaleLayout> P(new ScaleLayout());
    ScaleLayout &L = *P;
    L.src_fmt = src_fmt; L.dst_fmt = dst_fmt;
    L.sw = sw; L.sh = sh; L.dw = dw; L.dh = dh;
    L.si = si; L.di = di;
    L.csw = ceil_rshift(sw, si.hsub); L.csh = ceil_rshift(sh, si.vsub);
    L.cdw = ceil_rshift(dw, di.hsub); L.cdh = ceil_rshift(dh, di.vsub);

    // ff_get_unscaled_swscale(): converters tried before the generic path.
    if (sw == dw && sh == dh) {
        if (src_fmt == PP_FMT_YUV422P && dst_fmt == PP_FMT_UYVY422) {
            L.kind = ScaleLayout::INTERLEAVE;
            *out = std::move(P);
            return PP_OK;
        }
        if (!di.packed && si.hsub == di.hsub && si.vsub == di.vsub && si.depth <= di.depth) {
            L.kind = ScaleLayout::COPY;
            *out = std::move(P);
            return PP_OK;
        }
    }
    L.kind = di.packed ? ScaleLayout::GENERIC_UYVY : ScaleLayout::GENERIC;

    // sws_init_context(): increments and siting (get_local_pos, default -513)
    std::string err;
    const int lumXInc = (int)((((int64_t)sw << 16) + (dw >> 1)) / dw);
    const int lumYInc = (int)((((int64_t)sh << 16) + (dh >> 1)) / dh);
    const int chrXInc = (int)((((int64_t)L.csw << 16) + (L.cdw >> 1)) / L.cdw);
    const int chrYInc = (int)((((int64_t)L.csh << 16) + (L.cdh >> 1)) / L.cdh);
    if (L.f[0].build(lumXInc, sw, dw, 4, 1 << 14, flags, p0, p1, local_pos(0), local_pos(0), &err) ||
        L.f[1].build(chrXInc, L.csw, L.cdw, 4, 1 << 14, flags, p0, p1, local_pos(si.hsub), local_pos(di.hsub), &err) ||
        L.f[2].build(lumYInc, sh, dh, 2, 1 << 12, flags, p0, p1, local_pos(0), local_pos(0), &err) ||
        L.f[3].build(chrYInc, L.csh, L.cdh, 2, 1 << 12, flags, p0, p1, local_pos(si.vsub), local_pos(di.vsub), &err))
        PP_FAIL(PP_ERR_UNSUPPORTED, "filter construction: %s", err.c_str());

    // GPU layout: compact windows, one H-tap bucket for the launch
    HostPlane hp[2], hpd[2];
    for (int c = 0; c < 2; ++c) {
        const int src_w = c ? L.csw : sw, src_h = c ? L.csh : sh;
        if (L.f[c].compact(src_w, 1, &hp[c].h, &err) || L.f[2 + c].compact(src_h, 1, &hp[c].v, &err))
            PP_FAIL(PP_ERR_UNSUPPORTED, "%s", err.c_str());
    }
    const int ht = ht_bucket(std::max(hp[0].h.taps, hp[1].h.taps));
    if (ht < 0) PP_FAIL(PP_ERR_UNSUPPORTED, "horizontal filter of %d taps", std::max(hp[0].h.taps, hp[1].h.taps));
    L.ht = ht;
    for (int c = 0; c < 2; ++c) {
        const int src_w = c ? L.csw : sw, src_h = c ? L.csh : sh;
        const int dst_w = c ? L.cdw : dw, dst_h = c ? L.cdh : dh;
        if (hp[c].h.taps != ht && L.f[c].compact(src_w, ht, &hp[c].h, &err))
            PP_FAIL(PP_ERR_UNSUPPORTED, "%s", err.c_str());
        pair_rows(hp[c]);
        // chain plans (one_seg_chroma): the chroma ring of the fused second stage
        // needs the short chunks; PIXPATH_CHAIN_LUMA_CHO (measurement) sets luma's
        int cho_c = cho_max;
        if (!c && one_seg_chroma)
            if (const char *e = PP_KNOB("PIXPATH_CHAIN_LUMA_CHO")) cho_c = std::max(1, atoi(e));
        if (plan_tiles(hp[c], src_w, src_h, dst_w, dst_h, &L.lds_bytes, &err, c && one_seg_chroma ? 1 << 20 : 0, cho_c))
            PP_FAIL(PP_ERR_UNSUPPORTED, "%s", err.c_str());
    }
    plan_strip(L, hp, force_generic, one_seg_chroma);
    plan_direct(L, hp, hpd, allow_direct && !one_seg_chroma);
    fill_jobs(L, hp, hpd);
    pack_tables(L, hp, hpd);
    *out = std::move(P);
    return PP_OK;
}

const int32_t *table_i32(const ScaleLayout &L, const Table &t) {
    return reinterpret_cast<const int32_t *>(L.blob.data() + t.off);
}

// The fuse-2 second stage of a chain layout (4:2:2 targets): the chroma rows
// of the first stage (cdh1 rows, in L's chunks of `cho`) pass through an LDS
// byte ring into the second stage's vertical filter `fv` (dh2 output rows).
struct Stage2 {
    std::vector<int32_t> vrow2, chunk2, seg2;
    int vtp2 = 0, ring2 = 0, maxnew2 = 0;
    bool ok = true;  // the kernel has an instance for vtp2
};

int plan_stage2(const ScaleLayout &L, const FilterBank &fv, int dh2, Stage2 *s2) {
    // second-stage chroma rows: compact window, tap pairs, record per row
    const int cdh1 = L.cdh;
    FilterBank::Compact v;
    std::string err;
    if (fv.compact(cdh1, 1, &v, &err)) PP_FAIL(PP_ERR_UNSUPPORTED, "%s", err.c_str());
    std::vector<int> need(dh2, 0);
    for (int r = 0; r < dh2; ++r) {
        int last = 0;
        for (int k = 0; k < v.taps; ++k)
            if (v.coef[(size_t)r * v.taps + k]) last = k;
        need[r] = v.pos[r] + last;
    }
    // rows in pairs (2m, 2m + 1) over one shared window (strip.hpp pass2):
    // base = the even row at or below the pair's first non-zero tap, each
    // row's non-zero taps placed at their rows within the window
    const int npair = (dh2 + 1) / 2, T2 = v.taps;
    auto tap_rows = [&](int r, int *lo, int *hi) {
        *lo = INT32_MAX;
        *hi = -1;
        for (int k = 0; k < T2; ++k)
            if (v.coef[(size_t)r * T2 + k]) {
                *lo = std::min(*lo, v.pos[r] + k);
                *hi = std::max(*hi, v.pos[r] + k);
            }
        if (*hi < 0) *lo = *hi = v.pos[r];  // an all-zero row (none in practice)
    };
    std::vector<int> pbase(npair);
    int vtp2 = 1;
    for (int m = 0; m < npair; ++m) {
        int la, ha, lb, hb;
        tap_rows(2 * m, &la, &ha);
        tap_rows(std::min(2 * m + 1, dh2 - 1), &lb, &hb);
        pbase[m] = std::min(la, lb) & ~1;
        vtp2 = std::max(vtp2, (std::max(ha, hb) - pbase[m]) / 2 + 1);
    }
    s2->vtp2 = vtp2;
    s2->ok = vtp2 <= 3;  // strip.hpp pass2 instances (registers: spill-free at 6 waves)
    s2->vrow2.assign((size_t)npair * 16, 0);
    for (int m = 0; s2->ok && m < npair; ++m) {
        s2->vrow2[(size_t)m * 16] = pbase[m];
        uint16_t *t16 = reinterpret_cast<uint16_t *>(&s2->vrow2[(size_t)m * 16 + 1]);
        for (int h = 0; h < 2 && 2 * m + h < dh2; ++h)
            for (int k = 0; k < T2; ++k) {
                const int16_t c = v.coef[(size_t)(2 * m + h) * T2 + k];
                if (!c) continue;
                // in [0, 2 * vtp2): vtp2 covers every pair's last tap (fuzz_host.cpp checks)
                const int y = v.pos[2 * m + h] + k - pbase[m];
                t16[2 * (h * vtp2 + y / 2) + (y & 1)] = (uint16_t)c;
            }
    }
    // per first-stage chunk: the second-stage rows it completes and the ring2 rows kept
    const int cho = L.fjob[1].cho, nch = (cdh1 + cho - 1) / cho;
    s2->chunk2.assign((size_t)nch * 4, 0);
    int done = 0, ring2 = 0;
    for (int ci = 0; ci < nch; ++ci) {
        const int y0 = ci * cho, end = std::min(cdh1, y0 + cho);
        const int lo2 = done;
        // pairs complete together (a pair's rows are computed at once)
        while (done < dh2 && need[done] < end && (done + 1 >= dh2 || need[done + 1] < end))
            done = std::min(dh2, done + 2);
        if (ci == nch - 1) done = dh2;
        const int b2 = (std::min(lo2 < dh2 ? pbase[lo2 / 2] : y0, y0)) & ~1;
        s2->chunk2[4 * ci] = lo2;
        s2->chunk2[4 * ci + 1] = done;
        s2->chunk2[4 * ci + 2] = b2;
        s2->chunk2[4 * ci + 3] = (y0 - b2 + 1) >> 1;
        int top = end;
        for (int m = lo2 / 2; m < (done + 1) / 2; ++m) top = std::max(top, pbase[m] + 2 * vtp2);
        ring2 = std::max(ring2, top - b2);
    }
    s2->ring2 = (ring2 + 1) & ~1;
    // segments of the second-stage rows (the first stage's chroma walk is
    // one segment so that the second stage's taps are always in ring2):
    // each segment's walk starts at the chunk of its first row's window
    // and ends at the chunk that completes its last row, recomputing the
    // few first-stage rows of the halo instead of one 1080-row workgroup
    // per strip (4,800 long workgroups per 600-frame launch: a tail)
    int nseg2 = kChainSeg2;
    if (const char *e = PP_KNOB("PIXPATH_CHAIN_SEG2")) nseg2 = std::max(1, atoi(e));
    nseg2 = std::min(nseg2, std::max(1, dh2 / 16));
    s2->seg2.assign((size_t)nseg2 * 4, 0);
    const int32_t *chroma_lo = table_i32(L, L.jtab[1].chunk_lo), *chroma_hi = table_i32(L, L.jtab[1].chunk_hi);
    for (int sg = 0; sg < nseg2; ++sg) {
        // segments start on a row pair
        const int r0 = (int)((int64_t)sg * dh2 / nseg2) & ~1;
        const int r1 = sg + 1 == nseg2 ? dh2 : (int)((int64_t)(sg + 1) * dh2 / nseg2) & ~1;
        s2->seg2[4 * sg] = pbase[r0 / 2] / cho * cho;
        s2->seg2[4 * sg + 1] = std::min(cdh1, (need[r1 - 1] / cho + 1) * cho);
        s2->seg2[4 * sg + 2] = r0;
        s2->seg2[4 * sg + 3] = r1;
        // a segment's first chunk stages its whole source window, not only
        // the rows new to a walk from the top: the staging buffer grows to it
        const int c0 = s2->seg2[4 * sg] / cho;
        s2->maxnew2 = std::max(s2->maxnew2, chroma_hi[c0] - chroma_lo[c0]);
    }
    return PP_OK;
}

}  // namespace

int plan_layout(int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh, int flags, double p0, double p1,
                std::unique_ptr<ScaleLayout> *out) {
    return plan_one(src_fmt, sw, sh, dst_fmt, dw, dh, flags, p0, p1, false, out);
}

// create_avpvs_segment's two stages (lib/ffmpeg.py:1037-1048): the scale
// filter writes the overlay's yuv420p (overlay's default format=yuv420), then
// libavfilter converts yuv420p -> dst_fmt at the same size with a second
// swscale context (bicubic).  Both stages in one strip_kernel launch when the
// first stage is a strip plan and the second stage's luma / horizontal chroma
// filters are FFmpeg's identity banks (always, for the AVPVS formats).
int plan_chain_layout(int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh, int flags, double p0, double p1,
                      std::unique_ptr<ScaleLayout> *out) {
    if (!out) PP_FAIL(PP_ERR_INVALID, "null argument");
    out->reset();
    if (dst_fmt != PP_FMT_YUV420P && dst_fmt != PP_FMT_YUV422P && dst_fmt != PP_FMT_YUV420P10LE &&
        dst_fmt != PP_FMT_YUV422P10LE)
        PP_FAIL(PP_ERR_INVALID, "chain target %d: yuv420p, yuv422p, yuv420p10le or yuv422p10le", dst_fmt);
    if (dst_fmt == PP_FMT_YUV420P)  // no conversion after the overlay
        return plan_one(src_fmt, sw, sh, dst_fmt, dw, dh, flags, p0, p1, false, out);
    std::unique_ptr<ScaleLayout> P, p2;
    int rc = plan_one(src_fmt, sw, sh, PP_FMT_YUV420P, dw, dh, flags, p0, p1, true, &P, kChainCho, false);
    if (rc) return rc;
    rc = plan_one(PP_FMT_YUV420P, dw, dh, dst_fmt, dw, dh, PP_SWS_BICUBIC, PP_SWS_PARAM_DEFAULT, PP_SWS_PARAM_DEFAULT,
                  false, &p2);
    if (rc) return rc;
    ScaleLayout &L = *P;
    L.first_kind = L.kind;
    L.kind = ScaleLayout::CHAIN;
    const FmtInfo di = fmt_info(dst_fmt);
    L.chain_out = di.depth;
    L.dst_fmt = dst_fmt;
    L.stage2 = std::move(p2);
    const ScaleLayout &L2 = *L.stage2;
    *out = std::move(P);  // from here on a plan exists: fused below, or two launches
    if ((L2.kind != ScaleLayout::GENERIC && L2.kind != ScaleLayout::COPY) || !L.fast_hw) return PP_OK;
    const bool v422 = di.vsub == 0;
    // COPY (yuv420p -> yuv420p10le, planarCopyWrapper) is x << 2 as well
    bool ok = L2.kind == ScaleLayout::COPY ||
              (identity_bank(L2.f[0], 1 << 14) && identity_bank(L2.f[1], 1 << 14) &&
               identity_bank(L2.f[2], 1 << 12) && (v422 || identity_bank(L2.f[3], 1 << 12)));
    Stage2 s2;
    if (ok && v422) {
        if (int rc2 = plan_stage2(L, L2.f[3], L2.cdh, &s2)) {
            out->reset();
            return rc2;
        }
        ok = s2.ok;
    }
    if (s2.maxnew2 > L.fjob[1].maxnew) {
        for (int p = 1; p < 3; ++p) L.fjob[p].maxnew = s2.maxnew2;
        L.fast_lds_plane[1] = (size_t)s2.maxnew2 * L.fjob[1].S * 2 + (size_t)L.fjob[1].ring * L.fast_tw * 2;
        L.fast_lds = std::max(L.fast_lds, L.fast_lds_plane[1]);
    }
    // the byte ring is circular: a power of two of rows >= every chunk's live span
    int r2rows = 2;
    while (r2rows < s2.ring2) r2rows <<= 1;
    const size_t lds = L.fast_lds + (s2.ring2 ? (size_t)r2rows * L.fast_tw : 0);
    if (!ok || lds > kChainLdsMax) return PP_OK;
    // luma as its own launch (4:2:2 targets: the chroma launch then carries
    // only the ring2 planes): its plan is the plain first stage, same filters
    std::unique_ptr<ScaleLayout> lp;
    // PIXPATH_CHAIN_ONE_LAUNCH (measurement build): keep luma in the chroma launch
    const char *e_cho = PP_KNOB("PIXPATH_CHAIN_LUMA_CHO");
    if (v422 && !PP_KNOB("PIXPATH_CHAIN_ONE_LAUNCH") &&
        plan_one(src_fmt, sw, sh, PP_FMT_YUV420P, dw, dh, flags, p0, p1, false, &lp, e_cho ? std::atoi(e_cho) : 0,
                 false) == PP_OK &&
        lp->kind == ScaleLayout::GENERIC && lp->fast_hw > 0 && lp->fast_tw == 256) {
        lp->fjob[0].fuse = L.chain_out > 8 ? 1 : 0;
        L.luma = std::move(lp);
    }
    L.chain_lds = L.luma ? L.fast_lds_plane[1] + (size_t)r2rows * L.fast_tw : lds;
    L.chain_fused = true;
    const Table vrow2 = put(L, s2.vrow2), chunk2 = put(L, s2.chunk2), seg2 = put(L, s2.seg2);
    const int widen = L.chain_out > 8 ? 1 : 0;
    for (int p = 0; p < 3; ++p) {
        PlaneJob &J = L.fjob[p];
        J.fuse = (p && v422) ? 2 : widen;
        if (J.fuse == 2) {
            J.vtp2 = s2.vtp2;
            J.r2mask = r2rows - 1;
            L.ftab[p].vrow2 = vrow2;
            L.ftab[p].chunk2 = chunk2;
            L.ftab[p].seg2 = seg2;
            J.tiles_y = (int)s2.seg2.size() / 4;
        }
    }
    return PP_OK;
}

void bind(ScaleLayout &L, const void *base) {
    auto set = [base](auto *&ptr, const Table &t) {
        using P = std::remove_reference_t<decltype(ptr)>;
        ptr = t.off == Table::kNone ? nullptr : reinterpret_cast<P>(static_cast<const uint8_t *>(base) + t.off);
    };
    for (int p = 0; p < 3; ++p)
        for (int k = 0; k < 2; ++k) {
            PlaneJob &J = k ? L.fjob[p] : L.job[p];
            const JobTables &T = k ? L.ftab[p] : L.jtab[p];
            set(J.hpos, T.hpos); set(J.hcoef, T.hcoef); set(J.vbase, T.vbase); set(J.vcoef2, T.vcoef2);
            set(J.tile_c0, T.tile_c0); set(J.tile_cn, T.tile_cn);
            set(J.chunk_lo, T.chunk_lo); set(J.chunk_hi, T.chunk_hi);
            set(J.hbase4, T.hbase4); set(J.hcoefw, T.hcoefw); set(J.vrow16, T.vrow16);
            set(J.vrow2, T.vrow2); set(J.chunk2, T.chunk2); set(J.seg2, T.seg2);
        }
}

}  // namespace pp
