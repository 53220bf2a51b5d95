// Launch plan of the SI/TI kernel (siti.hip): how a clip of `nframes` frames
// of w x h is cut into (chunk, tile) units and how many workgroups walk them.
// Host arithmetic only -- shared by pp_siti_slots (which launches the plan),
// pp_siti_plan (which reports it, no GPU needed) and the host fuzzer
// (fuzz_host.cpp).
#pragma once

#include <algorithm>
#include <cstdint>

namespace pp {

constexpr int kBand = 16;                // rows of a workgroup's band
constexpr int kLanePx = 8;               // pixels a lane holds of a row
constexpr int kWaveSpan = 62 * kLanePx;  // 496 px per wave: lanes 0 and 63 are halo lanes
constexpr int kSpan = 4 * kWaveSpan;     // 1984 px per workgroup

// A band whose 18 window rows (y0 - 1 .. y0 + kBand) all lie in the frame runs
// the INTERIOR body of siti_range; the first band, the last band and every
// short band run the other.  siti_kernel spells this condition out instead of
// calling it: through the call the compiler allocates the frame loop's
// registers differently (the same kernel otherwise, to the instruction), and
// tests/test_siti_plan_host.py holds the two spellings together.
constexpr bool siti_band_interior(int y0, int H) { return y0 >= 1 && y0 + kBand + 1 <= H; }

// The fields pp_siti_plan reports, in this order.
struct SitiPlan {
    int tiles_x;         // kSpan-px tile columns
    int bands;           // kBand-row bands
    int ntiles;          // tiles_x * bands
    int ragged;          // w % kLanePx != 0: the RAGGED kernel instances
    int interior_bands;  // bands with siti_band_interior
    int fchunk;          // frames a unit walks
    int chunks;          // ceil(nframes / fchunk); the last one may be shorter
    int groups;          // workgroups launched: min(slots, ntiles * chunks)
};

// `slots`: the workgroups resident at once (CUs x occupancy on the device, or
// what the caller of pp_siti_slots gives); values below 1 count as 1.  One wave
// of resident workgroups (a partial second wave would idle most of the chip),
// each walking an equal share of the (tile, frame) units.  Frames per chunk:
// for R = 1..8 rounds of units over the slots, the longest chunk that still
// fits R rounds; keep the R with the shortest makespan (R * fchunk frames, plus
// ~1 frame of pipeline fill per round).  `bytes` (1 or 2 a sample) selects the
// instance, not the plan.  nframes < 1: the geometry alone, nothing to launch.
inline SitiPlan siti_plan(int bytes, int w, int h, int nframes, int64_t slots) {
    (void)bytes;
    SitiPlan p{};
    p.tiles_x = (w + kSpan - 1) / kSpan;
    p.bands = (h + kBand - 1) / kBand;
    p.ntiles = p.tiles_x * p.bands;
    p.ragged = (w % kLanePx) != 0;
    for (int b = 0; b < p.bands; ++b) p.interior_bands += siti_band_interior(b * kBand, h);
    if (nframes < 1 || p.ntiles < 1) return p;
    slots = std::max<int64_t>(1, slots);
    // (64-bit throughout: nframes + fchunk and ntiles * chunks pass 2^31 for counts an int holds)
    const int64_t ntiles = p.ntiles, nf = nframes;
    int64_t fchunk = nf;
    double best = 1e300;
    for (int R = 1; R <= 8; ++R) {
        const int64_t K = std::max<int64_t>(1, std::min<int64_t>(nf, R * slots / ntiles));
        const int64_t fc = (nf + K - 1) / K;
        const int64_t units = ntiles * ((nf + fc - 1) / fc);
        const int64_t rounds = (units + std::min(slots, units) - 1) / std::min(slots, units);
        const double cost = (double)rounds * (double)(fc + 1);
        if (cost < best) { best = cost; fchunk = fc; }
    }
    p.fchunk = (int)fchunk;
    p.chunks = (int)((nf + fchunk - 1) / fchunk);
    p.groups = (int)std::min<int64_t>(slots, ntiles * p.chunks);
    return p;
}

}  // namespace pp
