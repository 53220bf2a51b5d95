// Host-side fuzzer of libpixpath's parsers of untrusted bytes (SURVEY.md
// section 5: sanitizer builds of the host code).  Built by `make sanitize`
// with g++ -fsanitize=address,undefined and no GPU code; run by
// tests/test_host_sanitize.py.  Every input comes from a seeded generator:
//
//   * FFV1 configuration records (ffv1host.cpp ffv1_parse_record): pixpath's
//     own records for every format / slice grid, then bit flips, byte
//     overwrites, truncations, extensions and random buffers -- a valid record
//     must parse back to what was written, a corrupt one may fail but must
//     never read outside its buffer;
//   * FFV1 frame packets (ffv1_slice_table, the footer walk the decoder's host
//     side does on every packet of an AVPVS file): frames with valid 24-bit
//     slice-size footers, then corrupt footers, sizes (negative, zero, larger
//     than the buffer) -- on success every slice lies inside its frame and the
//     slices tile it;
//   * the p02 bitstream scanners (scan.cpp pp_annexb_frame_sizes,
//     pp_ivf_frame_sizes) on random and start-code-laden buffers;
//   * the swscale filter construction (filters.cpp FilterBank::build /
//     compact) for random sizes, flags and parameters;
//   * the scaler planner (scale_plan.cpp): plain and chain layouts of the
//     tested shapes and of seeded random ones, bound to their own table blob
//     and walked the way scale_kernel / strip_kernel index them -- every
//     window, ring row, staged row and LDS byte inside what the layout sizes;
//   * the group decode planner (ffv1host.cpp ffv1_plan_group): groups of 1-6
//     streams of 0-40 frames with random slice counts, keyframes and carried
//     GOPs, half of them valid, half with mutated packets or frame sizes --
//     an accepted plan is read as decode_group's uploads and
//     ffv1_decode_kernel read it: every slice inside its stream's 64-byte
//     aligned window of the packet buffer, the GOP triples tiling the frames
//     stream by stream, a continued GOP only where states were carried; a
//     refused one names its stream and says why;
//   * the SI/TI launch planner (siti_plan.hpp siti_plan): random widths,
//     heights, frame and slot counts, small and huge -- the chunks cover the
//     frames with only the last one short, the grid is min(slots, units) >= 1,
//     and the interior band count is that of the band condition.
//
//   * general FFV1 records given as seeds (file of u32-LE-length-prefixed
//     records: the oracle's FFmpeg-like records with transmitted state
//     tables, 5-input table sets and initial states) -- each must parse, then
//     its mutations must never read outside the buffer.
//
// usage: fuzz_host [iterations (default 20000)] [seed] [seed-record file]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "ffv1host.hpp"
#include "filters.hpp"
#include "scale_plan.hpp"
#include "siti_plan.hpp"

namespace pp {
// the library's error sink (api.cpp in the product build)
void set_error(const char *fmt, ...) { (void)fmt; }
}  // namespace pp

extern "C" int64_t pp_annexb_frame_sizes(const uint8_t *buf, int64_t n, int codec, int64_t *sizes, int64_t cap);
extern "C" int64_t pp_ivf_frame_sizes(const uint8_t *buf, int64_t n, int64_t *sizes, int64_t cap,
                                      int64_t *misdetected);

namespace {

using namespace pp;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    int below(int n) { return n > 0 ? (int)(next() % (uint64_t)n) : 0; }
};

int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            std::fprintf(stderr, "CHECK failed: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                         \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

// a heap copy of exactly n bytes, so ASan flags any read past the end
std::vector<uint8_t> exact(const std::vector<uint8_t> &v) { return std::vector<uint8_t>(v.begin(), v.end()); }

void mutate(Rng &r, std::vector<uint8_t> &b) {
    const int kind = r.below(6);
    if (b.empty() || kind == 5) {
        b.resize(r.below(64));
        for (auto &x : b) x = (uint8_t)r.next();
        return;
    }
    switch (kind) {
    case 0: b[r.below((int)b.size())] ^= (uint8_t)(1u << r.below(8)); break;  // bit flip
    case 1: b[r.below((int)b.size())] = (uint8_t)r.next(); break;              // byte overwrite
    case 2: b.resize(r.below((int)b.size())); break;                            // truncation
    case 3:                                                                     // extension
        for (int k = r.below(16) + 1; k; --k) b.push_back((uint8_t)r.next());
        break;
    default:                                                                    // several flips
        for (int k = r.below(8) + 2; k; --k) b[r.below((int)b.size())] ^= (uint8_t)r.next();
    }
}

long fuzz_records(Rng &r, int iters) {
    static const int fmts[][3] = {{8, 1, 1}, {8, 1, 0}, {10, 1, 1}, {10, 1, 0}};
    long n = 0;
    for (int it = 0; it < iters; ++it) {
        const int *f = fmts[r.below(4)];
        const int nh = 1 + r.below(16), nv = 1 + r.below(16);
        const int w = 64 * (1 + r.below(30)), h = 64 * (1 + r.below(17));
        std::vector<uint8_t> rec = ffv1_write_record(f[0], f[1], f[2], nh, nv, ffv1_default_quant(f[0]));
        pp::Ffv1Record out;
        std::string err;
        if (it % 8 == 0) {  // the valid record round trips
            std::vector<uint8_t> b = exact(rec);
            const int rc = ffv1_parse_record(b.data(), (int)b.size(), w, h, &out, &err);
            CHECK(rc == 0 && out.bits == f[0] && out.hsub == f[1] && out.vsub == f[2] && out.nh == nh &&
                      out.nv == nv && out.ec == 1 && out.ntables == 1 && out.ctx_count[0] == ffv1_default_quant(f[0]).contexts() && out.intra == 1 &&
                      out.coder == 1,
                  "record %d/%d/%d %dx%d did not round trip: %d %s", f[0], f[1], f[2], nh, nv, rc, err.c_str());
        }
        std::vector<uint8_t> m = rec;
        for (int k = 1 + r.below(3); k; --k) mutate(r, m);
        std::vector<uint8_t> b = exact(m);
        (void)ffv1_parse_record(b.empty() ? nullptr : b.data(), (int)b.size(), w, h, &out, &err);
        ++n;
    }
    return n;
}

long fuzz_seed_records(Rng &r, int iters, const char *path) {
    std::vector<std::vector<uint8_t>> seeds;
    if (FILE *f = std::fopen(path, "rb")) {
        uint8_t hdr[4];
        while (std::fread(hdr, 1, 4, f) == 4) {
            const uint32_t n = hdr[0] | hdr[1] << 8 | hdr[2] << 16 | (uint32_t)hdr[3] << 24;
            std::vector<uint8_t> b(n);
            if (std::fread(b.data(), 1, n, f) != n) break;
            seeds.push_back(std::move(b));
        }
        std::fclose(f);
    }
    CHECK(!seeds.empty(), "no seed records in %s", path);
    long n = 0;
    for (size_t k = 0; k < seeds.size(); ++k) {
        pp::Ffv1Record out;
        std::string err;
        std::vector<uint8_t> b = exact(seeds[k]);
        const int rc = ffv1_parse_record(b.data(), (int)b.size(), 1920, 1080, &out, &err);
        CHECK(rc == 0, "seed record %zu refused: %s", k, err.c_str());
    }
    for (int it = 0; it < iters && !seeds.empty(); ++it) {
        std::vector<uint8_t> m = seeds[r.below((int)seeds.size())];
        for (int k = 1 + r.below(3); k; --k) mutate(r, m);
        std::vector<uint8_t> b = exact(m);
        pp::Ffv1Record out;
        std::string err;
        (void)ffv1_parse_record(b.empty() ? nullptr : b.data(), (int)b.size(), 1920, 1080, &out, &err);
        ++n;
    }
    return n;
}

long fuzz_packets(Rng &r, int iters) {
    long n = 0;
    for (int it = 0; it < iters; ++it) {
        const int per = 1 + r.below(16), nframes = 1 + r.below(4), ec = r.below(2);
        const int trailer = 3 + 5 * ec;
        std::vector<uint8_t> pk;
        std::vector<int64_t> sizes;
        for (int f = 0; f < nframes; ++f) {
            const size_t base = pk.size();
            for (int s = 0; s < per; ++s) {
                const int len = r.below(200);
                for (int k = 0; k < len; ++k) pk.push_back((uint8_t)r.next());
                for (int k = 0; k < trailer - 3; ++k) pk.push_back((uint8_t)r.next());
                pk.push_back((uint8_t)(len >> 16));
                pk.push_back((uint8_t)(len >> 8));
                pk.push_back((uint8_t)len);
            }
            sizes.push_back((int64_t)(pk.size() - base));
        }
        // mutate footers, payload bytes or the frame sizes
        const int kind = r.below(5);
        if (kind == 1 && !pk.empty()) {
            for (int k = 1 + r.below(4); k; --k) pk[r.below((int)pk.size())] = (uint8_t)r.next();
        } else if (kind == 2) {
            sizes[r.below(nframes)] += r.below(41) - 20;
        } else if (kind == 3) {
            sizes[r.below(nframes)] = -(int64_t)r.below(1000) - 1;
        } else if (kind == 4 && !pk.empty()) {
            pk.resize(r.below((int)pk.size()));
            int64_t tot = 0;
            for (auto &s : sizes) {  // frame sizes past the truncation are cut to what is left
                s = std::max<int64_t>(0, std::min<int64_t>(s, (int64_t)pk.size() - tot));
                tot += s;
            }
        }
        int64_t total_sz = 0;
        bool sizes_ok = true;
        for (int64_t s : sizes) {
            sizes_ok = sizes_ok && s >= 0;
            total_sz += s;
        }
        if (!sizes_ok || total_sz > (int64_t)pk.size()) {
            // a caller hands over its own buffer of the sizes it claims: skip
            // lies about the buffer length, keep negative sizes (must be refused)
            if (sizes_ok) continue;
        }
        std::vector<uint8_t> b = exact(pk);
        std::vector<int64_t> soff((size_t)nframes * per, -1), slen((size_t)nframes * per, -1);
        int64_t total = -1;
        std::string err;
        const int rc = ffv1_slice_table(b.empty() ? nullptr : b.data(), sizes.data(), nframes, per, ec,
                                        soff.data(), slen.data(), &total, &err);
        ++n;
        if (rc == 0) {
            int64_t base = 0;
            for (int f = 0; f < nframes; ++f) {
                int64_t at = base;
                for (int s = 0; s < per; ++s) {
                    const int64_t o = soff[(size_t)f * per + s], l = slen[(size_t)f * per + s];
                    CHECK(o == at && l >= trailer && o + l <= base + sizes[f], "slice %d of frame %d outside", s, f);
                    at = o + l;
                }
                CHECK(at == base + sizes[f], "frame %d slices do not tile it", f);
                base += sizes[f];
            }
            CHECK(total == base, "total %lld != %lld", (long long)total, (long long)base);
        } else {
            CHECK(!err.empty(), "failure without a message");
        }
    }
    return n;
}

long fuzz_scanners(Rng &r, int iters) {
    long n = 0;
    for (int it = 0; it < iters; ++it) {
        std::vector<uint8_t> buf(r.below(4096));
        for (auto &x : buf) x = (uint8_t)(r.below(4) ? r.below(3) : r.next());  // many 0x00 / 0x01 bytes
        if (it % 3 == 0 && buf.size() > 32) {  // an IVF-like header
            std::memcpy(buf.data(), "DKIF", 4);
            buf[6] = 32;
        }
        std::vector<uint8_t> b = exact(buf);
        std::vector<int64_t> sizes(r.below(64));
        int64_t mis = 0;
        const uint8_t *p = b.empty() ? nullptr : b.data();
        (void)pp_annexb_frame_sizes(p, (int64_t)b.size(), 1 + r.below(2), sizes.empty() ? nullptr : sizes.data(),
                                    (int64_t)sizes.size());
        (void)pp_ivf_frame_sizes(p, (int64_t)b.size(), sizes.empty() ? nullptr : sizes.data(), (int64_t)sizes.size(),
                                 &mis);
        n += 2;
    }
    return n;
}

long fuzz_filters(Rng &r, int iters) {
    static const int flags[] = {PP_SWS_BICUBIC, PP_SWS_LANCZOS, PP_SWS_BILINEAR};
    long n = 0;
    for (int it = 0; it < iters; ++it) {
        const int src = 4 + r.below(r.below(2) ? 64 : 4096), dst = 1 + r.below(r.below(2) ? 64 : 4096);
        const int xinc = (int)((((int64_t)src << 16) + (dst >> 1)) / dst);
        pp::FilterBank fb;
        std::string err;
        const double p0 = r.below(4) ? PP_SWS_PARAM_DEFAULT : (double)r.below(10);
        if (fb.build(xinc, src, dst, r.below(2) ? 4 : 2, r.below(2) ? 1 << 14 : 1 << 12, flags[r.below(3)], p0,
                     PP_SWS_PARAM_DEFAULT, pp::local_pos(r.below(2)), pp::local_pos(r.below(2)), &err) == 0) {
            pp::FilterBank::Compact c;
            if (fb.compact(src, 1 + r.below(8), &c, &err) == 0) {
                // a window wider than the plane starts at 0 (the kernel zero-fills
                // past the edge); every non-zero tap reads inside the plane
                for (int i = 0; i < dst; ++i) {
                    CHECK(c.pos[i] >= 0 && (c.pos[i] + c.taps <= src || c.pos[i] == 0), "window %d at %d", i,
                          c.pos[i]);
                    for (int k = 0; k < c.taps; ++k)
                        if (c.coef[(size_t)i * c.taps + k])
                            CHECK(c.pos[i] + k < src, "tap %d of output %d outside [0, %d)", k, i, src);
                }
            }
        }
        ++n;
    }
    return n;
}

// ---- scaler plans (scale_plan.cpp) ------------------------------------------
// A layout bound to its own blob is walked as scale_kernel (scale.hip) and
// strip_kernel (strip.hpp) walk it; every bound below is one of their unchecked
// indexings.  `tag` names the plan in a failure message.
#define PCHECK(cond, fmt, ...) CHECK(cond, "%s: " fmt, tag, ##__VA_ARGS__)

using Taps = std::vector<std::pair<int, int>>;  // (source position, coefficient) of the non-zero taps

size_t count32(const Table &t) { return t.off == Table::kNone ? 0 : t.bytes / 4; }

Taps compact_taps(const FilterBank::Compact &c, int i) {
    Taps t;
    for (int k = 0; k < c.taps; ++k)
        if (c.coef[(size_t)i * c.taps + k]) t.push_back({c.pos[i] + k, c.coef[(size_t)i * c.taps + k]});
    return t;
}

// strip geometry and column windows (both kernels): the staged window of a
// strip is 16-sample aligned, fits the staged row, and holds every H window
void check_columns(const char *tag, const PlaneJob &J, const JobTables &T, int ht) {
    PCHECK((1 << J.twl) == J.tw && J.tiles_x == (J.dw + J.tw - 1) / J.tw, "strips %d x %d for %d columns", J.tiles_x,
           J.tw, J.dw);
    PCHECK(count32(T.tile_c0) == (size_t)J.tiles_x && count32(T.tile_cn) == (size_t)J.tiles_x &&
               count32(T.hpos) == (size_t)J.dw && T.hcoef.bytes == (size_t)J.dw * ht * 2,
           "column table sizes");
    PCHECK(J.S % 8 == 0, "staged row stride %d not 16-B", J.S);
    for (int tx = 0; tx < J.tiles_x; ++tx) {
        const int c0 = J.tile_c0[tx], cn = J.tile_cn[tx];
        PCHECK(c0 >= 0 && c0 % 16 == 0 && cn % 16 == 0 && cn <= J.S, "strip %d window [%d, +%d) S %d", tx, c0, cn, J.S);
        for (int x = tx * J.tw; x < std::min(J.dw, (tx + 1) * J.tw); ++x) {
            const int pos = J.hpos[x];
            PCHECK(pos >= c0 && pos + ht <= c0 + cn, "column %d window at %d outside [%d, +%d)", x, pos, c0, cn);
            for (int k = 0; k < ht; ++k)
                if (J.hcoef[(size_t)x * ht + k]) PCHECK(pos + k < J.sw, "column %d tap %d past the row", x, k);
        }
    }
}

// strip_kernel H tables: a lane reads HW dwords at hbase4 of the staged row and
// its outputs' taps re-laid over them (hcoefw)
void check_strip_h(const char *tag, const PlaneJob &F, const JobTables &T, int ht, int HW) {
    const size_t ng = (size_t)F.tiles_x * (F.tw / 4);
    PCHECK(count32(T.hbase4) == ng && count32(T.hcoefw) == ng * 4 * HW, "strip H table sizes");
    for (size_t g = 0; g < ng; ++g) {
        const int hb = F.hbase4[g];
        PCHECK(hb >= 0 && hb % 4 == 0 && hb + 2 * HW <= F.S, "lane group %zu base %d + %d > S %d", g, hb, 2 * HW, F.S);
    }
    const int16_t *h16 = reinterpret_cast<const int16_t *>(F.hcoefw);
    for (int x = 0; x < F.dw; ++x) {
        const int c0 = F.tile_c0[x / F.tw], hb = F.hbase4[x / 4];
        Taps got, want;
        for (int s = 0; s < 2 * HW; ++s)
            if (const int c = h16[(size_t)x * HW * 2 + s]) got.push_back({c0 + hb + s, c});
        for (int k = 0; k < ht; ++k)
            if (const int c = F.hcoef[(size_t)x * ht + k]) want.push_back({F.hpos[x] + k, c});
        PCHECK(got == want, "column %d: re-laid taps differ from the compact filter", x);
    }
}

// V tables and chunk rows: every row's window [base, base + 2 vtp) lies in the
// ring of its chunk (window row 0 = the chunk's first source row, rounded to
// even) and carries the compact V filter; strip_kernel reads vrow16 records
void check_rows(const char *tag, const PlaneJob &J, const JobTables &T, const FilterBank::Compact &v, bool strip) {
    const int nch = (J.dh + J.cho - 1) / J.cho;
    PCHECK(J.cho > 0 && J.seg_h > 0 && J.seg_h % J.cho == 0, "segment %d rows, chunk %d", J.seg_h, J.cho);
    PCHECK(count32(T.chunk_lo) == (size_t)nch && count32(T.chunk_hi) == (size_t)nch &&
               count32(T.vbase) == (size_t)J.dh && count32(T.vcoef2) == (size_t)J.dh * J.vtp,
           "row table sizes");
    if (strip) PCHECK(J.vtp <= 8 && count32(T.vrow16) == (size_t)J.dh * 16, "strip row records, %d tap pairs", J.vtp);
    PCHECK(J.ring % 2 == 0, "ring %d", J.ring);
    for (int ci = 0; ci < nch; ++ci) {
        const int lo = J.chunk_lo[ci], hi = J.chunk_hi[ci], b = lo & ~1;
        PCHECK(0 <= lo && lo < hi && hi <= J.sh, "chunk %d rows [%d, %d) of %d", ci, lo, hi, J.sh);
        PCHECK(hi - b <= J.ring, "chunk %d rows [%d, %d) past ring %d", ci, lo, hi, J.ring);
        for (int y = ci * J.cho; y < std::min(J.dh, (ci + 1) * J.cho); ++y) {
            const int32_t *rec = strip ? J.vrow16 + (size_t)y * 16 : nullptr;
            const int base = strip ? rec[0] : J.vbase[y];
            PCHECK(base % 2 == 0 && base >= b && base + 2 * J.vtp - b <= J.ring,
                   "row %d window [%d, +%d) outside ring [%d, +%d)", y, base, 2 * J.vtp, b, J.ring);
            Taps got;
            for (int j = 0; j < J.vtp; ++j) {
                const uint32_t w = (uint32_t)(strip ? rec[1 + j] : J.vcoef2[(size_t)y * J.vtp + j]);
                if (const int c = (int16_t)(w & 0xffff)) got.push_back({base + 2 * j, c});
                if (const int c = (int16_t)(w >> 16)) got.push_back({base + 2 * j + 1, c});
            }
            PCHECK(got == compact_taps(v, y), "row %d: tap pairs differ from the compact filter", y);
            for (const auto &t : got) PCHECK(t.first >= lo && t.first < hi, "row %d reads unstaged row %d", y, t.first);
        }
    }
}

// the kernels' walk over the chunks of output rows [y_begin, y_end): the rows
// new to each chunk fit the staging buffer (DIRECT stages none)
void check_walk(const char *tag, const PlaneJob &J, int y_begin, int y_end, bool direct) {
    const int nch = (J.dh + J.cho - 1) / J.cho;
    PCHECK(y_begin >= 0 && y_begin % J.cho == 0 && y_begin < y_end && y_end <= J.dh, "walk [%d, %d) of %d rows", y_begin,
           y_end, J.dh);
    if (y_begin < 0 || y_begin >= J.dh) return;
    int next = J.chunk_lo[y_begin / J.cho];
    for (int y0 = y_begin; y0 < y_end; y0 += J.cho) {
        const int ci = y0 / J.cho;
        if (ci >= nch) break;  // (reported above: y_end > dh)
        if (next < J.chunk_lo[ci]) next = J.chunk_lo[ci];
        const int nnew = J.chunk_hi[ci] - next;
        if (!direct) PCHECK(nnew <= J.maxnew, "chunk %d stages %d rows, buffer %d", ci, nnew, J.maxnew);
        if (nnew > 0) next = J.chunk_hi[ci];
    }
}

void check_segments(const char *tag, const PlaneJob &J, bool direct) {
    PCHECK(J.tiles_y >= 1 && (J.tiles_y - 1) * J.seg_h < J.dh && J.tiles_y * J.seg_h >= J.dh, "%d segments of %d rows",
           J.tiles_y, J.seg_h);
    if (direct) PCHECK(J.maxnew == 0, "DIRECT with %d staged rows", J.maxnew);
    for (int sg = 0; sg < J.tiles_y; ++sg) check_walk(tag, J, sg * J.seg_h, std::min(J.dh, (sg + 1) * J.seg_h), direct);
}

// fuse 2: the chroma planes of a fused chain layout.  Segments come from seg2;
// after each first-stage chunk the second stage emits the rows chunk2 lists,
// reading row pairs' windows from the circular byte ring2 (row & r2mask).
void check_chain(const char *tag, const ScaleLayout &L, const PlaneJob &F, const JobTables &T) {
    const int cdh1 = F.dh, dh2 = L.stage2->cdh, cho = F.cho, nch = (cdh1 + cho - 1) / cho, R = F.r2mask + 1;
    const int npair = (dh2 + 1) / 2, VT2 = F.vtp2;
    PCHECK(VT2 >= 1 && VT2 <= 3, "vtp2 %d", VT2);
    PCHECK(R >= 2 && (R & (R - 1)) == 0, "ring2 of %d rows", R);
    PCHECK(count32(T.vrow2) == (size_t)npair * 16 && count32(T.chunk2) == (size_t)nch * 4 &&
               count32(T.seg2) == (size_t)F.tiles_y * 4 && F.tiles_y >= 1,
           "second-stage table sizes");
    FilterBank::Compact v2;
    std::string err;
    PCHECK(L.stage2->f[3].compact(cdh1, 1, &v2, &err) == 0, "second-stage filter: %s", err.c_str());
    for (int m = 0; m < npair; ++m) {  // vrow2 records: base row, VT2 pairs of row 2m, VT2 of row 2m + 1
        const int32_t *rec = F.vrow2 + (size_t)m * 16;
        PCHECK(rec[0] >= 0 && rec[0] % 2 == 0, "pair %d base %d", m, rec[0]);
        for (int h = 0; h < 2 && 2 * m + h < dh2; ++h) {
            Taps got;
            for (int j = 0; j < VT2; ++j) {
                const uint32_t w = (uint32_t)rec[1 + h * VT2 + j];
                if (const int c = (int16_t)(w & 0xffff)) got.push_back({rec[0] + 2 * j, c});
                if (const int c = (int16_t)(w >> 16)) got.push_back({rec[0] + 2 * j + 1, c});
            }
            PCHECK(got == compact_taps(v2, 2 * m + h), "second-stage row %d: taps differ from the filter", 2 * m + h);
        }
    }
    int done = 0;
    for (int ci = 0; ci < nch; ++ci) {  // chunk2: monotone cover of [0, dh2)
        const int32_t *c2 = F.chunk2 + 4 * ci;
        PCHECK(c2[0] == done && c2[1] >= c2[0] && c2[1] <= dh2 && (c2[0] % 2 == 0 || c2[0] == dh2),
               "chunk %d second-stage rows [%d, %d) after %d", ci, c2[0], c2[1], done);
        done = c2[1];
    }
    PCHECK(done == dh2, "second-stage rows end at %d of %d", done, dh2);
    int r_next = 0;
    for (int sg = 0; sg < F.tiles_y; ++sg) {
        const int32_t *s = F.seg2 + 4 * sg;
        const int y_begin = s[0], y_end = s[1], r0 = s[2], r1 = s[3];
        PCHECK(r0 == r_next && r0 < r1 && r0 % 2 == 0, "segment %d rows [%d, %d) after %d", sg, r0, r1, r_next);
        r_next = r1;
        PCHECK(y_begin >= 0 && y_begin % cho == 0 && (y_end % cho == 0 || y_end == cdh1) && y_end <= cdh1,
               "segment %d first-stage rows [%d, %d) of %d", sg, y_begin, y_end, cdh1);
        check_walk(tag, F, y_begin, y_end, false);
        // the segment's walk: every row of [r0, r1) is emitted once, by a chunk
        // that has every ring2 row its taps read (computed since y_begin, not
        // yet overwritten: the ring holds rows (end - R, end))
        int r = r0;
        for (int y0 = y_begin; y0 < y_end && y0 / cho < nch; y0 += cho) {
            const int32_t *c2 = F.chunk2 + 4 * (y0 / cho);
            const int end = std::min(y_end, y0 + cho), b2 = c2[2];
            const int lo2 = std::max(c2[0], r0), hi2 = std::min(c2[1], r1);
            PCHECK(b2 % 2 == 0 && b2 <= y0 && end - b2 <= R, "chunk %d ring2 base %d, rows to %d, ring %d", y0 / cho, b2,
                   end, R);
            for (int q = lo2; q < hi2; ++q, ++r) {
                PCHECK(q == r, "segment %d: row %d emitted at %d", sg, q, r);
                const int pbase = F.vrow2[(size_t)(q / 2) * 16];
                PCHECK(pbase >= b2 && pbase + 2 * VT2 <= b2 + R, "row %d window [%d, +%d) outside ring2 [%d, +%d)", q,
                       pbase, 2 * VT2, b2, R);
                for (const auto &t : compact_taps(v2, q))
                    PCHECK(t.first >= y_begin && t.first < end && t.first >= end - R, "row %d tap row %d not in ring2 at %d",
                           q, t.first, end);
            }
        }
        PCHECK(r == r1, "segment %d emits rows to %d of %d", sg, r, r1);
    }
    PCHECK(r_next == dh2, "segments end at %d of %d", r_next, dh2);
}

// the LDS a strip_kernel launch of job F needs (strip.hpp: staged rows, window ring, ring2)
size_t strip_lds(const PlaneJob &F) {
    return (size_t)F.maxnew * F.S * 2 + (size_t)F.ring * F.tw * 2 + (F.fuse == 2 ? (size_t)(F.r2mask + 1) * F.tw : 0);
}

void check_layout(const char *tag, ScaleLayout &L) {
    if (L.stage2) check_layout(tag, *L.stage2);
    if (L.luma) {
        check_layout(tag, *L.luma);
        PCHECK(L.luma->fast_hw > 0 && strip_lds(L.luma->fjob[0]) == L.luma->fast_lds_plane[0], "luma launch LDS");
    }
    const ScaleLayout::Kind kind = L.kind == ScaleLayout::CHAIN ? L.first_kind : L.kind;
    if (kind == ScaleLayout::COPY || kind == ScaleLayout::INTERLEAVE) {
        PCHECK(L.blob.empty() && !L.chain_fused, "tables of an unscaled plan");
        return;
    }
    bind(L, L.blob.data());
    FilterBank::Compact v[2];
    std::string err;
    for (int c = 0; c < 2; ++c)
        PCHECK(L.f[2 + c].compact(c ? L.csh : L.sh, 1, &v[c], &err) == 0, "vertical filter: %s", err.c_str());
    // scale_kernel jobs (the fallback of every plan)
    size_t lds = 0;
    int base = 0;
    for (int p = 0; p < 3; ++p) {
        const PlaneJob &J = L.job[p];
        check_columns(tag, J, L.jtab[p], L.ht);
        check_rows(tag, J, L.jtab[p], v[p ? 1 : 0], false);
        check_segments(tag, J, false);
        PCHECK(J.tile_base == base, "plane %d tile base %d, running sum %d", p, J.tile_base, base);
        base += J.tiles_x * J.tiles_y;
        lds = std::max(lds, (size_t)J.maxnew * J.S * 2 + (size_t)J.ring * J.tw * 2 + (size_t)J.cho * J.vtp * 4 +
                                (size_t)J.cho * 4);
    }
    PCHECK(lds == L.lds_bytes && lds <= (size_t)kLdsBudget, "scale_kernel LDS %zu, layout %zu", lds, L.lds_bytes);
    if (!L.fast_hw) {
        PCHECK(!L.direct && !L.chain_fused, "strip decisions without a strip plan");
        return;
    }
    // strip_kernel jobs
    lds = 0;
    base = 0;
    for (int p = 0; p < 3; ++p) {
        const PlaneJob &F = L.fjob[p];
        check_columns(tag, F, L.ftab[p], L.ht);
        check_strip_h(tag, F, L.ftab[p], L.ht, L.fast_hw);
        check_rows(tag, F, L.ftab[p], v[p ? 1 : 0], true);
        if (F.fuse == 2) {
            PCHECK(L.chain_fused && p > 0, "fuse 2 on plane %d", p);
            if (L.chain_fused) check_chain(tag, L, F, L.ftab[p]);
        } else {
            check_segments(tag, F, L.direct);
        }
        // (a fused chain launch numbers its planes' tiles itself: fuse 2 changes tiles_y)
        if (!L.chain_fused) PCHECK(F.tile_base == base, "strip plane %d tile base %d, running sum %d", p, F.tile_base, base);
        base += F.tiles_x * F.tiles_y;
        if (!(L.luma && p == 0)) lds = std::max(lds, strip_lds(F));  // (with `luma`, plane 0 runs from that layout)
    }
    if (L.chain_fused) {
        PCHECK(lds <= L.chain_lds && L.chain_lds <= kChainLdsMax, "chain LDS %zu, needs %zu", L.chain_lds, lds);
        if (L.luma) PCHECK(lds == L.chain_lds, "chroma launch LDS %zu, needs %zu", L.chain_lds, lds);
    } else {
        PCHECK(base == L.fast_tiles, "strip tiles %d, sum %d", L.fast_tiles, base);
        PCHECK(lds == L.fast_lds && lds <= (size_t)kLdsBudget * (L.fast_tw / 256), "strip LDS %zu, layout %zu", lds,
               L.fast_lds);
    }
}

struct PlanCase {
    bool chain;
    int sf, sw, sh, df, dw, dh, flags;
};

void plan_case(const PlanCase &c) {
    char tag[96];
    std::snprintf(tag, sizeof tag, "%s %d %dx%d -> %d %dx%d flags 0x%x", c.chain ? "chain" : "plan", c.sf, c.sw, c.sh,
                  c.df, c.dw, c.dh, c.flags);
    std::unique_ptr<ScaleLayout> L;
    const int rc = c.chain ? plan_chain_layout(c.sf, c.sw, c.sh, c.df, c.dw, c.dh, c.flags, PP_SWS_PARAM_DEFAULT,
                                               PP_SWS_PARAM_DEFAULT, &L)
                           : plan_layout(c.sf, c.sw, c.sh, c.df, c.dw, c.dh, c.flags, PP_SWS_PARAM_DEFAULT,
                                         PP_SWS_PARAM_DEFAULT, &L);
    PCHECK((rc == 0) == (L != nullptr) && rc <= 0, "return code %d %s a layout", rc, L ? "with" : "without");
    if (L) check_layout(tag, *L);
}

long fuzz_plans(Rng &r, int iters) {
    static const PlanCase fixed[] = {
        // tests/test_native_abi.py CONFIGS and chain cases, the 6x shapes of tests/test_gpu_scale.py
        {false, PP_FMT_YUV420P, 1280, 720, PP_FMT_YUV420P, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV422P10LE, 1280, 720, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV422P10LE, 1280, 720, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_LANCZOS},
        {false, PP_FMT_YUV420P10LE, 960, 540, PP_FMT_YUV420P, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 1920, 1080, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 1920, 1080, PP_FMT_YUV420P, 1280, 720, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV422P10LE, 3840, 2160, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 3840, 2160, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 3840, 2160, PP_FMT_YUV420P, 640, 360, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 3840, 1600, PP_FMT_YUV420P, 1920, 800, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 4096, 2160, PP_FMT_YUV420P, 1920, 1012, PP_SWS_LANCZOS},
        {false, PP_FMT_YUV420P, 640, 360, PP_FMT_YUV420P, 3840, 2160, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV422P, 250, 99, PP_FMT_YUV420P10LE, 77, 61, PP_SWS_LANCZOS},
        {false, PP_FMT_YUV444P10LE, 64, 48, PP_FMT_YUV422P, 130, 90, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 333, 197, PP_FMT_YUV420P, 500, 301, PP_SWS_BILINEAR},
        {false, PP_FMT_YUV420P, 1920, 1080, PP_FMT_UYVY422, 1920, 1080, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 8, 8, PP_FMT_YUV420P, 3, 3, PP_SWS_BICUBIC},
        {true, PP_FMT_YUV420P10LE, 1280, 720, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {true, PP_FMT_YUV422P10LE, 1280, 720, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {true, PP_FMT_YUV420P, 1280, 720, PP_FMT_YUV422P, 1920, 1080, PP_SWS_BICUBIC},
        {true, PP_FMT_YUV420P, 1280, 720, PP_FMT_YUV420P10LE, 1920, 1080, PP_SWS_BICUBIC},
        {true, PP_FMT_YUV420P, 1920, 1080, PP_FMT_YUV422P10LE, 1920, 1080, PP_SWS_BICUBIC},
        // refused: packed source, packed chain target, too small, no filter
        {false, PP_FMT_UYVY422, 64, 64, PP_FMT_YUV420P, 32, 32, PP_SWS_BICUBIC},
        {true, PP_FMT_YUV420P, 64, 64, PP_FMT_UYVY422, 64, 64, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 3, 64, PP_FMT_YUV420P, 32, 32, PP_SWS_BICUBIC},
        {false, PP_FMT_YUV420P, 64, 64, PP_FMT_YUV420P, 32, 32, 0},
    };
    long n = 0;
    for (const PlanCase &c : fixed) {
        plan_case(c);
        ++n;
    }
    // seeded plans: a third chain plans, every filter, every planar format
    // pair; ragged sizes in 4..700, now and then one very small side
    static const int flags[] = {PP_SWS_BICUBIC, PP_SWS_LANCZOS, PP_SWS_BILINEAR};
    static const int targets[] = {PP_FMT_YUV422P, PP_FMT_YUV420P10LE, PP_FMT_YUV422P10LE, PP_FMT_YUV420P};
    auto side = [&r] { return r.below(8) ? 4 + r.below(697) : 4 + r.below(5); };
    for (int it = 0; it < iters; ++it) {
        PlanCase c;
        c.chain = it % 3 == 2;
        c.sf = (it / 3) % 6;  // the six planar formats (PP_FMT_YUV420P .. PP_FMT_YUV444P10LE)
        c.df = c.chain ? targets[(it / 18) % 4] : (it / 18) % 6;
        c.flags = flags[r.below(3)];
        c.sw = side(); c.sh = side(); c.dw = side(); c.dh = side();
        plan_case(c);
        ++n;
    }
    return n;
}

// ---- group decode plans (ffv1host.cpp ffv1_plan_group) ------------------------
struct GroupCase {
    int n, per, ec;
    std::vector<std::vector<uint8_t>> pk;     // per stream: its packets back to back
    std::vector<std::vector<int64_t>> sizes;  // per stream: frame sizes
    std::vector<int> nframes;
    std::vector<char> carry;
    long gops = 0;  // GOPs the frames were built with
};

// a group of valid streams: slices with 24-bit size footers, keyframes placed
// at random (a frame 0 that continues a GOP only where carry is set)
GroupCase make_group(Rng &r) {
    static const int pers[] = {1, 4, 6, 16, 64};
    GroupCase g;
    g.n = 1 + r.below(6);
    g.per = pers[r.below(5)];
    g.ec = r.below(2);
    g.pk.resize(g.n);
    g.sizes.resize(g.n);
    for (int k = 0; k < g.n; ++k) {
        const int nf = r.below(41);
        g.nframes.push_back(nf);
        g.carry.push_back((char)r.below(2));
        for (int f = 0; f < nf; ++f) {
            const bool key = f == 0 && !g.carry[k] ? true : r.below(4) == 0;
            g.gops += f == 0 || key;
            const size_t base = g.pk[k].size();
            for (int s = 0; s < g.per; ++s) {
                const int len = 2 + r.below(12);
                for (int i = 0; i < len; ++i) g.pk[k].push_back((uint8_t)r.next());
                if (s == 0) {  // the keyframe bit: the first two bytes against 0x7F80 (ffv1_keyframe_bit)
                    uint8_t *b = g.pk[k].data() + g.pk[k].size() - len;
                    if (r.below(4) == 0) {
                        b[0] = 0x7F;
                        b[1] = (uint8_t)((key ? 0x80 : 0) | (b[1] & 0x7F));
                    } else {
                        b[0] = (uint8_t)(key ? 0x80 | b[0] : b[0] % 0x7F);
                    }
                }
                g.pk[k].push_back((uint8_t)(len >> 16));
                g.pk[k].push_back((uint8_t)(len >> 8));
                g.pk[k].push_back((uint8_t)len);
                for (int i = 0; i < 5 * g.ec; ++i) g.pk[k].push_back((uint8_t)r.next());
            }
            g.sizes[k].push_back((int64_t)(g.pk[k].size() - base));
        }
    }
    return g;
}

// an accepted plan, checked the way decode_group's uploads and
// ffv1_decode_kernel read it
void check_group(const GroupCase &g, const std::vector<const uint8_t *> &pk, const Ffv1GroupPlan &P, long id) {
    char tag[48];
    std::snprintf(tag, sizeof tag, "group %ld", id);
    const int n = g.n, per = g.per;
    int64_t ftot = 0;
    for (int nf : g.nframes) ftot += nf;
    const int fail0 = g_fail;  // a table that failed a check is not indexed further
    PCHECK(P.ftot == ftot && P.soff.size() == (size_t)(ftot * per) && P.slen.size() == P.soff.size() &&
               P.gop.size() % 3 == 0 && P.first_gop.size() == (size_t)n && P.ngop.size() == (size_t)n &&
               P.bytes.size() == (size_t)n && P.base.size() == (size_t)n,
           "table sizes for %lld frames", (long long)ftot);
    if (g_fail != fail0) return;
    const int ngops = (int)P.gop.size() / 3;
    int64_t at = 0, f0 = 0;  // packet-buffer bytes and frames of the streams so far
    int g0 = 0;              // their GOPs
    for (int k = 0; k < n; ++k) {
        const int nf = g.nframes[k];
        int64_t sum = 0;
        for (int64_t s : g.sizes[k]) sum += s;
        PCHECK(P.base[k] == at && at % 64 == 0 && P.bytes[k] == sum, "stream %d window [%lld, +%lld), expected [%lld, +%lld)",
               k, (long long)P.base[k], (long long)P.bytes[k], (long long)at, (long long)sum);
        for (int64_t i = f0 * per; i < (f0 + nf) * per; ++i)
            PCHECK(P.base[k] <= P.soff[i] && P.slen[i] >= 0 && P.soff[i] + P.slen[i] <= P.base[k] + P.bytes[k],
                   "stream %d slice %lld [%lld, +%lld) outside its window", k, (long long)i, (long long)P.soff[i],
                   (long long)P.slen[i]);
        PCHECK(P.first_gop[k] == g0 && P.ngop[k] >= 0 && g0 + P.ngop[k] <= ngops && (nf > 0) == (P.ngop[k] > 0),
               "stream %d GOPs [%d, +%d) after %d of %d", k, P.first_gop[k], P.ngop[k], g0, ngops);
        if (g_fail != fail0) return;
        int64_t f = f0;
        for (int q = g0; q < g0 + P.ngop[k]; ++q) {  // the stream's GOPs tile its frames
            const int first = P.gop[3 * q], cnt = P.gop[3 * q + 1], flag = P.gop[3 * q + 2];
            PCHECK(first == f && cnt >= 1 && f + cnt <= f0 + nf, "GOP %d frames [%d, +%d) at %lld of stream %d to %lld", q,
                   first, cnt, (long long)f, k, (long long)(f0 + nf));
            PCHECK(flag == 1 || (flag == 0 && q == g0 && g.carry[k]), "GOP %d flag %d (stream %d, carry %d)", q, flag, k,
                   g.carry[k]);
            if (g_fail != fail0) return;
            for (int j = 0; j < cnt; ++j) {  // the flag is the first frame's keyframe bit; no keyframe inside a GOP
                const int64_t s0 = (f + j) * per;
                const int key = ffv1_keyframe_bit(pk[k] + (P.soff[s0] - P.base[k]), P.slen[s0]);
                PCHECK(key == (j == 0 ? flag : 0), "GOP %d frame %d keyframe bit %d", q, j, key);
            }
            f += cnt;
        }
        PCHECK(f == f0 + nf, "stream %d GOPs end at frame %lld of %lld", k, (long long)f, (long long)(f0 + nf));
        at += (sum + 63) & ~int64_t(63);
        f0 += nf;
        g0 += P.ngop[k];
    }
    PCHECK(g0 == ngops && P.total == at, "%d GOPs of %d, buffer %lld of %lld", g0, ngops, (long long)P.total, (long long)at);
}

// The first half of the groups are valid and must plan, to the GOPs they were
// built with; the second half have a stream's packets or frame sizes mutated,
// or a frame 0 turned into an inter frame.
long fuzz_groups(Rng &r, int iters, long *ok) {
    long n = 0;
    for (int it = 0; it < iters; ++it) {
        GroupCase g = make_group(r);
        const bool valid = it < (iters + 1) / 2;
        if (!valid) {
            const int k = r.below(g.n), kind = r.below(3);
            std::vector<uint8_t> &b = g.pk[k];
            std::vector<int64_t> &sz = g.sizes[k];
            if (kind == 0) {
                mutate(r, b);
            } else if (kind == 1 && !sz.empty()) {
                std::vector<uint8_t> raw(sz.size() * 8);
                std::memcpy(raw.data(), sz.data(), raw.size());
                mutate(r, raw);
                std::memcpy(sz.data(), raw.data(), std::min(raw.size(), sz.size() * 8));
            } else if (b.size() >= 2) {
                b[0] = 0;
            }
            // a caller hands over a buffer of the sizes it claims: sizes past the
            // bytes that are left are cut to them, up to the first negative one
            // (which must be refused before anything behind it is read)
            int64_t tot = 0;
            for (auto &s : sz) {
                if (s < 0) break;
                s = std::min<int64_t>(s, (int64_t)b.size() - tot);
                tot += s;
            }
        }
        std::vector<std::vector<uint8_t>> held;
        std::vector<const uint8_t *> pk;
        std::vector<const int64_t *> sz;
        for (int k = 0; k < g.n; ++k) {
            held.push_back(exact(g.pk[k]));
            pk.push_back(held.back().data());
            sz.push_back(g.sizes[k].data());
        }
        Ffv1GroupPlan P;
        std::string err;
        int failed = -1;
        const int rc = ffv1_plan_group(g.n, pk.data(), sz.data(), g.nframes.data(), g.carry.data(), g.per, g.ec, &P,
                                       &failed, &err);
        ++n;
        if (rc == 0) {
            ++*ok;
            check_group(g, pk, P, n);
            if (valid) CHECK((long)P.gop.size() / 3 == g.gops, "group %ld: %zu GOPs planned, %ld built", n, P.gop.size() / 3, g.gops);
        } else {
            CHECK(!valid, "group %ld: a valid group was refused: %s", n, err.c_str());
            CHECK(rc < 0 && failed >= 0 && failed < g.n && !err.empty(), "group %ld: failure %d at stream %d, message '%s'", n,
                  rc, failed, err.c_str());
        }
    }
    return n;
}

// ---- SI/TI launch plans (siti_plan.hpp) ---------------------------------------
long fuzz_siti_plans(Rng &r, int iters) {
    long n = 0;
    for (int it = 0; it < iters; ++it) {
        // sizes and counts small (every value near the tile, band and lane edges) and up to the ABI's int range
        // (heights to 100000 rows: the planner counts the bands one by one)
        auto pick = [&r](int small, int big) { return r.below(4) ? 1 + r.below(small) : 1 + r.below(big); };
        const int w = 2 + pick(4100, 0x7ffffff0), h = 2 + pick(70, 100000), nf = pick(40, 0x7ffffff0);
        const int64_t slots = r.below(8) ? pick(70, 4096) : pick(0x7ffffff0, 0x7ffffff0);
        if ((int64_t)((w + kSpan - 1) / kSpan) * ((h + kBand - 1) / kBand) > 0x7fffffff) continue;  // ntiles is an int
        const SitiPlan p = siti_plan(1 + r.below(2), w, h, nf, slots);
        ++n;
        char tag[96];
        std::snprintf(tag, sizeof tag, "siti plan %dx%d x%d on %lld", w, h, nf, (long long)slots);
        PCHECK(p.tiles_x == (w + kSpan - 1) / kSpan && p.bands == (h + kBand - 1) / kBand &&
                   p.ntiles == p.tiles_x * p.bands && p.ragged == (w % kLanePx != 0),
               "geometry %d x %d = %d, ragged %d", p.tiles_x, p.bands, p.ntiles, p.ragged);
        // every band but the first and the last has a row above and a row below its 16
        const int interior = std::max(0, p.bands - 2);
        PCHECK(p.interior_bands == interior && !siti_band_interior(0, h), "%d interior bands, expected %d",
               p.interior_bands, interior);
        PCHECK(p.fchunk >= 1 && p.fchunk <= nf, "fchunk %d", p.fchunk);
        if (p.fchunk < 1) continue;
        PCHECK((int64_t)(p.chunks - 1) * p.fchunk < nf && (int64_t)p.chunks * p.fchunk >= nf, "%d chunks of %d", p.chunks,
               p.fchunk);
        PCHECK(p.groups >= 1 && p.groups == std::min<int64_t>(slots, (int64_t)p.ntiles * p.chunks), "%d groups", p.groups);
    }
    // no frames, no slots: the geometry alone / one slot
    const SitiPlan e = siti_plan(2, 1985, 34, 0, 4), o = siti_plan(2, 1985, 34, 9, 0), o1 = siti_plan(2, 1985, 34, 9, 1);
    CHECK(e.ntiles == 6 && e.fchunk == 0 && e.chunks == 0 && e.groups == 0, "plan of no frames");
    CHECK(o.fchunk == o1.fchunk && o.chunks == o1.chunks && o.groups == 1, "plan on no slots");
    return n;
}

}  // namespace

int main(int argc, char **argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 20000;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    Rng r(seed);
    const long a = fuzz_records(r, iters);
    const long b = fuzz_packets(r, iters);
    const long c = fuzz_scanners(r, iters / 4);
    const long d = fuzz_filters(r, iters / 20);
    const long e = argc > 3 ? fuzz_seed_records(r, iters, argv[3]) : 0;
    const long f = fuzz_plans(r, iters / 60);
    long groups_ok = 0;
    const long g = fuzz_groups(r, iters / 10, &groups_ok);
    const long h = fuzz_siti_plans(r, iters);
    std::printf("records %ld packets %ld scans %ld filters %ld seeded %ld plans %ld groups %ld groups_ok %ld "
                "siti_plans %ld failures %d\n",
                a, b, c, d, e, f, g, groups_ok, h, g_fail);
    return g_fail ? 1 : 0;
}
