#!/usr/bin/env python3
"""Time pp_dct_energy (PP-DCTE-1) on one MI355X with HIP events, next to
pp_motion, pp_siti and pp_ms_ssim on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080 luma, 8 and 10 bits, three contents:
noise over the legal range, a smooth moving gradient, a constant plane (the
kernel does the same work for all three: the check that it does).
  dct_energy  one ops.dct_energy call over the clip's luma (dct_kernel and
              dct_finalize of every launch of 256 frames)
  motion      one ops.motion call over the same luma
  siti        one ops.siti call over the same luma
  ms_ssim     one ops.ms_ssim call of the luma against itself
The box-to-box spread cancels in the ratios.  Before timing, the GPU sums of
the first frames are compared with the numpy restatement
(tests/dctenergy_ref.py) for equality.  Next to the time the json records the
bytes the algorithm must move (every luma sample read once) and their rate
against the HBM peaks (8.0 TB/s spec, 6.29 TB/s measured copy), and the
multiply-adds the folded transform takes (2 passes x 32 lines x 32 outputs x
16 = 32768 a block, one v_mad_i32_i24 each) against the integer multiply-add
issue rate of the device (CUs x 4 SIMDs x 16 lanes x clock): a count of
instructions, not a counter reading.
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/dctenergy_bench.py [--frames 600] [--out profiles/dctenergy/NAME.json]
"""
import sys

import callbench

CHECKED = 3  # frames compared with the CPU
MADS_PER_BLOCK = 2 * 32 * 32 * 16
W, H = callbench.W, callbench.H


def fill(luma, content, depth, dev):
    """The clip's content, frame by frame: no batch-sized temporaries."""
    import torch
    lo, hi = (64, 941) if depth > 8 else (16, 236)
    sp = luma.view(torch.int16) if depth > 8 else luma
    ramp = (torch.arange(W, device=dev)[None, :] + 2 * torch.arange(H, device=dev)[:, None])
    for k in range(luma.shape[0]):
        if content == "noise":
            f = torch.randint(lo, hi, sp[k].shape, dtype=torch.int16, device=dev)
        elif content == "smooth":
            f = lo + ((ramp + 3 * k) // 8) % (hi - lo)
        else:
            f = torch.full(sp[k].shape, (lo + hi) // 2, device=dev)
        sp[k].copy_(f)
    torch.cuda.synchronize()


def one_case(depth, content, luma, a, dev, peak_mads):
    import torch

    import dctenergy_ref as R
    from pixpath import dctenergy, ops
    n = luma.shape[0]
    fill(luma, content, depth, dev)
    keep = {}

    def dct_pass():
        keep["dct"] = ops.dct_energy(luma, depth)

    def motion_pass():
        keep["motion"] = ops.motion(luma, depth)

    def siti_pass():
        keep["siti"] = ops.siti(luma, depth)

    def msssim_pass():
        keep["msssim"] = ops.ms_ssim(luma, luma)

    dct_pass()
    torch.cuda.synchronize()
    got = [[int(v) for v in r] for r in keep["dct"][:CHECKED].cpu().numpy()]
    want = R.sums(luma[:CHECKED].cpu().numpy(), depth)
    if got != want:
        raise SystemExit("dctenergy_bench: %d-bit %s differs from the restatement: %r against %r" % (depth, content, got, want))
    E, T, L = dctenergy.pool(keep["dct"].cpu().numpy(), W, H)
    de = callbench.timed(dct_pass, a.warmup, a.iters)
    res = {"bitdepth": depth, "content": content, "dct_energy": de,
           "clip": {"dct_energy_y": float(E.mean()), "dct_temporal_y": float(T.mean()), "brightness_y": float(L.mean())}}
    if content == "noise":  # the neighbours' times do not depend on the content either: once per depth
        mo, si, ms = (callbench.timed(f, a.warmup, a.iters) for f in (motion_pass, siti_pass, msssim_pass))
        res.update({"motion": mo, "siti": si, "ms_ssim": ms,
                    "dct_energy_over_motion": round(de["avg_ms"] / mo["avg_ms"], 3),
                    "dct_energy_over_siti": round(de["avg_ms"] / si["avg_ms"], 3),
                    "dct_energy_over_ms_ssim": round(de["avg_ms"] / ms["avg_ms"], 3)})
    traffic = n * W * H * (2 if depth > 8 else 1)  # every luma sample once (the 24 ragged rows are not read)
    rate = traffic / (de["avg_ms"] * 1e-3)
    bx, by = dctenergy.geometry(W, H)
    mads = n * bx * by * MADS_PER_BLOCK  # lane operations
    res.update({"algorithmic_bytes": traffic, "tb_per_s": round(rate / 1e12, 3),
                "share_of_hbm_spec": round(rate / callbench.HBM_PEAK, 3), "share_of_hbm_copy": round(rate / callbench.HBM_COPY, 3),
                "multiply_adds": mads, "share_of_int_mad_issue_rate": round(mads / (de["avg_ms"] * 1e-3) / peak_mads, 3),
                "cpu_check_frames": CHECKED, "cpu_check": "equal"})
    return res


def main(argv=None):
    ap = callbench.parser(600, 3, 10)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("dctenergy_bench", seed=910)
    import torch
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 2400000)) * 1e3
    peak = prop.multi_processor_count * 4 * 16 * clock_hz
    cases = []
    for depth in (8, 10):
        luma = torch.empty((a.frames, H, W), dtype=torch.uint16 if depth > 8 else torch.uint8, device=dev)
        for content in ("noise", "smooth", "constant"):
            cases.append(one_case(depth, content, luma, a, dev, peak))
        del luma
    res = callbench.header(
        "dctenergy_bench", a, compute_units=prop.multi_processor_count, clock_hz=clock_hz, int_mad_lane_ops_per_s=peak,
        timer="HIP events around one call over the clip: every launch of pp_dct_energy (dct_kernel, "
              "dct_finalize) / of pp_motion / of pp_siti / of pp_ms_ssim (the luma against itself)",
        hbm_spec_bytes_per_s=callbench.HBM_PEAK, hbm_copy_bytes_per_s=callbench.HBM_COPY, cases=cases)
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
