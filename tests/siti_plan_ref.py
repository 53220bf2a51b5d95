"""Python re-statement of the SI/TI launch planner (csrc/siti_plan.hpp),
written from the planner's description, for tests/test_siti_plan_host.py.

A workgroup owns a tile: 1984 columns (4 waves x 62 lanes x 8 px) by 16 rows.
The frames are cut into chunks of `fchunk`; a (chunk, tile) pair is a unit and
`slots` workgroups are resident at once.  For R = 1..8 rounds of units over the
slots the planner allows as many chunks as R rounds of slots hold per tile
(at least one, at most one a frame), takes the shortest chunk length that needs
no more chunks than that, and prices the candidate at
(rounds it really takes) x (fchunk + 1 frame of pipeline fill).  The cheapest
candidate wins, the smaller R on a tie."""
import collections

SPAN, BAND, LANE_PX = 1984, 16, 8

Plan = collections.namedtuple("Plan", "tiles_x bands ntiles ragged interior_bands fchunk chunks groups")


def ceil_div(a, b):
    return -(-a // b)


def band_rows(h):
    """(y0, rows) of every band of a frame of h rows."""
    return [(y0, min(BAND, h - y0)) for y0 in range(0, h, BAND)]


def interior(y0, h):
    """The band's window, rows y0 - 1 .. y0 + 16, lies wholly in the frame."""
    return y0 - 1 >= 0 and y0 + BAND <= h - 1


def plan(w, h, n, slots):
    tiles_x, bands = ceil_div(w, SPAN), ceil_div(h, BAND)
    ntiles = tiles_x * bands
    candidates = []
    for rounds_wanted in range(1, 9):
        max_chunks = min(max(rounds_wanted * slots // ntiles, 1), n)
        fchunk = ceil_div(n, max_chunks)
        units = ntiles * ceil_div(n, fchunk)
        rounds = ceil_div(units, min(slots, units))
        candidates.append((rounds * (fchunk + 1), rounds_wanted, fchunk))
    fchunk = min(candidates)[2]
    chunks = ceil_div(n, fchunk)
    return Plan(tiles_x, bands, ntiles, w % LANE_PX != 0, sum(interior(y0, h) for y0, _ in band_rows(h)), fchunk,
                chunks, min(slots, ntiles * chunks))
