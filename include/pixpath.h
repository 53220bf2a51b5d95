/*
 * pixpath.h -- C ABI of libpixpath.so, the MI355X (gfx950) raw-frame pixel path
 * behind pnats2avhd/processing-chain's command builders (lib/ffmpeg.py) and SRC
 * analysis hooks (util/SRC_analysis.py, util/complexity_classification.py).
 *
 * Plain C types only: device pointers, byte strides, sizes, an opaque context.
 * Every entry point returns PP_OK (0) or a negative PP_ERR_* code; the message
 * of the last failure is available from pp_last_error() (thread-local).
 * Kernels are enqueued on the caller's HIP stream (`stream`, a hipStream_t
 * passed as void*; NULL = the null stream) and never synchronise it.
 * A context is bound to one device and is not thread-safe (one per process,
 * matching the one-process-per-GPU model of SURVEY.md section 8e).
 *
 * Which reference interface each entry point replaces is given per function as
 * reference file:line.  The reference reaches all of these through ffmpeg
 * command strings; the strings are reproduced by the Python host
 * (processing-chain_amd/pixpath/ffmpeg.py), which calls this library.
 */
#ifndef PIXPATH_H
#define PIXPATH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ABI_VERSION 7

/* return codes */
#define PP_OK 0
#define PP_ERR_INVALID -1     /* bad argument / unsupported combination */
#define PP_ERR_HIP -2         /* HIP runtime failure */
#define PP_ERR_NOMEM -3
#define PP_ERR_UNSUPPORTED -4

/* pixel formats (ffmpeg -pix_fmt names in comments) */
enum pp_pix_fmt {
    PP_FMT_YUV420P = 0,      /* yuv420p */
    PP_FMT_YUV422P = 1,      /* yuv422p */
    PP_FMT_YUV444P = 2,      /* yuv444p */
    PP_FMT_YUV420P10LE = 3,  /* yuv420p10le */
    PP_FMT_YUV422P10LE = 4,  /* yuv422p10le */
    PP_FMT_YUV444P10LE = 5,  /* yuv444p10le */
    PP_FMT_UYVY422 = 6,      /* uyvy422 (packed, 1 plane) */
    PP_FMT_V210 = 7          /* -c:v v210 payload (packed, 1 plane) */
};

/* swscale flag values (same bits as FFmpeg's SWS_*) */
#define PP_SWS_BILINEAR 0x2
#define PP_SWS_BICUBIC 0x4
#define PP_SWS_LANCZOS 0x200
#define PP_SWS_PARAM_DEFAULT 123456.0
/* ABI v5: plan flag selecting the general scale_kernel even where the strip
 * kernel applies (both are bit-exact; tests run every plan through both). */
#define PP_PLAN_GENERIC 0x10000000

/*
 * A batch of `nframes` frames.  Plane p of frame f starts at
 * data[p] + f * frame_stride[p]; rows are linesize[p] bytes apart.
 * Packed formats use plane 0 only.  Every row of a plane, the last one
 * included, must be readable for min(linesize, width rounded up to 16 bytes)
 * bytes: with 16-byte aligned pointers and linesizes the kernels read whole
 * 16-byte granules (a plane allocated as height x linesize always qualifies).
 */
typedef struct pp_frames {
    void *data[3];
    int64_t linesize[3];
    int64_t frame_stride[3];
} pp_frames;

typedef struct pp_ctx pp_ctx;
typedef struct pp_scale_plan pp_scale_plan;

/* ---- library / context ------------------------------------------------- */
int pp_abi_version(void);
const char *pp_last_error(void);
/* Select `device` and create a context.  Replaces nothing in the reference
 * (the reference runs CPU processes, lib/cmd_utils.py:93-101). */
int pp_ctx_create(int device, pp_ctx **out);
int pp_ctx_destroy(pp_ctx *ctx);

/* Byte size of one plane of one frame and the v210 line size (v210enc.c:
 * ceil(w/48)*48*8/3). */
int64_t pp_plane_bytes(int fmt, int w, int h, int plane, int64_t linesize);
int64_t pp_v210_linesize(int w);

/* ---- scaling / format conversion (libswscale restatement) --------------
 * Replaces `scale=W:H:flags=bicubic` at lib/ffmpeg.py:992 (create_avpvs_short),
 * :1038 (create_avpvs_segment), :1213 (create_cpvs mobile), `scale=W:-2` at
 * :800 (encode_segment) and the implicit `-pix_fmt` conversions at :994, :1048,
 * :1198.  flags: PP_SWS_BICUBIC | PP_SWS_LANCZOS | PP_SWS_BILINEAR; param0/1 as
 * FFmpeg's sws param[0]/[1] (PP_SWS_PARAM_DEFAULT = FFmpeg default).
 * dst_fmt may be planar YUV or PP_FMT_UYVY422 (packed output path).
 * Coefficient tables are built on the host once per plan and kept in HBM.
 * ctx == NULL builds a host-only plan (filter introspection, no execution). */
int pp_scale_plan_create(pp_ctx *ctx, int src_fmt, int src_w, int src_h,
                         int dst_fmt, int dst_w, int dst_h, int flags,
                         double param0, double param1, pp_scale_plan **out);
int pp_scale_plan_destroy(pp_scale_plan *plan);
/* Introspection for parity tests: which = 0 luma-H, 1 chroma-H, 2 luma-V,
 * 3 chroma-V.  Copies the FFmpeg-layout filter (before device compaction):
 * coef[n * size] int16, pos[n] int32 on the host.  Returns size (>0),
 * 0 when the plan uses an unscaled converter, or <0. */
int pp_scale_plan_filter(const pp_scale_plan *plan, int which, int16_t *coef,
                         int32_t *pos, int capacity);
/* Kernel the plan runs for 16-B aligned sources: > 0 = the strip kernel's
 * horizontal window in dwords (the common case), 0 = the general kernel
 * (narrow strips / long vertical filters / unscaled converters).  The
 * environment variable PIXPATH_SCALE_KERNEL=generic at plan creation forces 0
 * (parity tests run both kernels on the same cases). */
int pp_scale_plan_path(const pp_scale_plan *plan);
/* Launch geometry of the plan for measurement and documentation: fills up to
 * n of {LDS bytes per workgroup, threads per workgroup, workgroups per frame,
 * luma chunk rows, luma segment rows, luma V tap pairs, chroma V tap pairs,
 * luma staged columns, luma window rows, luma max new rows per chunk}.
 * Returns the number of values written. */
int pp_scale_plan_stats(const pp_scale_plan *plan, int64_t *out, int n);
/* Which compiled kernel instances pp_scale_execute launches for this plan.
 * The strip, packed, chain and general-kernel launchers pick their kernel
 * through the code that fills the key, so for those the report is the choice;
 * the list of launches itself (unscaled converters, the two-launch chain)
 * restates the executor.
 * Works on host-only plans.  vec_src: every source plane pointer, linesize and
 * frame stride is 16-B aligned; vec_dst: every destination plane's is 8-B
 * aligned (4-B for 8-bit planar output).  One key of PP_SCALE_KEY_FIELDS
 * int32 per launch, in launch order:
 *   [0] family (PP_SCALE_FAM_*)
 *   [1] source sample bytes (1, 2)      [2] output bits (8, 10)
 *   [3] strip families: H window dwords (HW); general kernel: H-tap bucket (HT)
 *   [4] strip families: V tap-pair bucket (VTM), else 0
 *   [5] 1 = the DIRECT instance (8-bit source, HW 8, plain)
 *   [6] 1 = 256-column strips (general kernel: the TW-256 variant)
 *   [7] second-stage V tap pairs of a chain launch's fuse-2 planes, else 0
 *   [8] 1 = every strip of the launch runs the clamped V pass (vector stores,
 *       every plane width a multiple of 4), 0 = a per-lane strip exists
 *   [9] 1 = the instance compiles the clamped V-pass copy at all
 *   [10] output rows per chunk of the launch's first plane (0: no chunks)
 *   [11] fewest chunks any plane of the launch walks in one segment (a chain
 *        launch's second-stage planes: over their whole height); >= 2 means
 *        every plane carries window rows from one chunk to the next
 * A fused 4:2:2 chain with its own luma plan reports two keys (luma launch,
 * chroma launch); a two-launch chain reports PP_SCALE_FAM_TWO_LAUNCH followed
 * by the keys of its first and second stage; a packed plan off the strip path
 * reports the general kernel and PP_SCALE_FAM_INTERLEAVE.
 * Returns the number of keys (<= 8), or < 0 (PP_ERR_INVALID when `capacity`,
 * in keys, is too small).  Added without raising PP_ABI_VERSION. */
#define PP_SCALE_KEY_FIELDS 12
#define PP_SCALE_FAM_PLAIN 0
#define PP_SCALE_FAM_PACKED 1
#define PP_SCALE_FAM_CHAIN 2
#define PP_SCALE_FAM_CHAIN_LUMA 3
#define PP_SCALE_FAM_CHAIN_CHROMA 4
#define PP_SCALE_FAM_GENERAL 5
#define PP_SCALE_FAM_COPY 6
#define PP_SCALE_FAM_INTERLEAVE 7
#define PP_SCALE_FAM_TWO_LAUNCH 8
int pp_scale_plan_instances(const pp_scale_plan *plan, int vec_src, int vec_dst,
                            int32_t *out, int capacity);
/* The two-stage chain of create_avpvs_segment (lib/ffmpeg.py:1037-1048):
 * `scale=W:H:flags=...` into the overlay's yuv420p, then libavfilter's
 * auto-inserted yuv420p -> dst_fmt conversion at the same size (bicubic).
 * Executed with pp_scale_execute; bit-exact with running the two plans one
 * after the other.  When the first stage is a strip plan
 * (pp_scale_plan_path > 0) both stages run in ONE kernel launch with no
 * intermediate in HBM; otherwise two launches through a plan-owned yuv420p
 * scratch batch (so such a plan serves one stream at a time).
 * dst_fmt: yuv420p (one stage), yuv422p, yuv420p10le, yuv422p10le. */
int pp_scale_chain_plan_create(pp_ctx *ctx, int src_fmt, int src_w, int src_h,
                               int dst_fmt, int dst_w, int dst_h, int flags,
                               double param0, double param1, pp_scale_plan **out);
/* Run the plan on `nframes` device frames. */
int pp_scale_execute(pp_scale_plan *plan, const pp_frames *src,
                     const pp_frames *dst, int nframes, void *stream);

/* ---- padding -----------------------------------------------------------
 * Replaces `pad=width=DW:height=DH:x=(ow-iw)/2:y=(oh-ih)/2` at
 * lib/ffmpeg.py:1183 (create_cpvs PC) and :1209 (tablet).  Black is
 * Y 16 / C 128 scaled to the bit depth; x/y are rounded down to the chroma
 * grid.  Pass x = y = -1 for the reference's centring expression. */
int pp_pad_execute(pp_ctx *ctx, int fmt, int src_w, int src_h,
                   const pp_frames *src, int dst_w, int dst_h, int x, int y,
                   const pp_frames *dst, int nframes, void *stream);

/* ---- CPVS packers ------------------------------------------------------
 * `-c:v v210 -pix_fmt yuv422p10le` (lib/test_config.py:208-215 via
 * lib/ffmpeg.py:1198): pack yuv422p10le into v210 (libavcodec/v210enc.c);
 * dst plane 0 with linesize >= pp_v210_linesize(w).  An odd w is
 * PP_ERR_INVALID, as in FFmpeg ("v210 needs even width"). */
int pp_v210_pack(pp_ctx *ctx, int w, int h, const pp_frames *src,
                 const pp_frames *dst, int nframes, void *stream);

/* Fused PC CPVS: `fps,pad=W:H:(ow-iw)/2:(oh-ih)/2` + `-pix_fmt` conversion +
 * packing in one pass (lib/ffmpeg.py:1177-1201).  src: AVPVS frames (w x h,
 * yuv420p/yuv422p for out_fmt PP_FMT_UYVY422, yuv420p10le/yuv422p10le for
 * PP_FMT_V210); canvas W x H with the input at (x, y) (-1 = centred, rounded
 * to the chroma grid); dst plane 0, 16-B aligned.  Bit-identical to pad ->
 * swscale (bicubic) -> packer.  An odd W is PP_ERR_INVALID for both packings
 * (uyvy422 pairs pixels; FFmpeg's v210 encoder refuses odd widths). */
int pp_cpvs_execute(pp_ctx *ctx, int src_fmt, int w, int h, const pp_frames *src,
                    int W, int H, int x, int y, int out_fmt,
                    const pp_frames *dst, int nframes, void *stream);

/* ---- CPVS unpackers ----------------------------------------------------
 * Reads the payloads above back: a v210 or uyvy422 CPVS (to score it against
 * its AVPVS with pp_metrics) or an uncompressed SRC (pp_siti on its luma).
 * Inverse of the CPVS packers.  src: plane 0 of nframes W x H frames of
 * in_fmt (PP_FMT_V210 or PP_FMT_UYVY422).  dst: the w x h window at (x, y)
 * of each frame as planar 4:2:2 (yuv422p10le for v210, yuv422p for uyvy422).
 * dst->data[1] == dst->data[2] == NULL: luma only.
 * v210 (libavcodec/v210dec.c): little-endian 32-bit words of three 10-bit
 * fields (bits 30-31 ignored), U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5 per
 * 16 bytes; the tails of W % 6 in {2, 4} are the same layout cut short.  W
 * even; src linesize a multiple of 4 and >= ceil(W/6)*16 (it need not be
 * pp_v210_linesize(W) nor 16-byte aligned).  uyvy422: bytes U Y0 V Y1; W
 * even; linesize >= 2 W.  Window: 0 <= x, x even, x + w <= W, 0 <= y,
 * y + h <= H, w >= 1 (may be odd: chroma width (w+1)/2), h >= 1; there is no
 * -1 = centred shorthand: pass the offsets the pad put the picture at.
 * Sources and destinations on the 16-byte grid (pointers, linesizes, frame
 * strides) move as 16-byte loads and stores; anything else goes sample by
 * sample with identical output.  Arguments are checked before any HIP call;
 * nframes == 0 is PP_OK.  Parity with FFmpeg's v210dec / rawdec is unpinned.
 * Added without raising PP_ABI_VERSION (still 7). */
int pp_unpack_execute(pp_ctx *ctx, int in_fmt, int W, int H, const pp_frames *src,
                      int x, int y, int w, int h, const pp_frames *dst,
                      int nframes, void *stream);

/* ---- stall compositing (spec PP-STALL-1) -----------------
 * Replaces the external `bufferer -s spinner.png` call at
 * p03_generateAvPvs.py:236-243.  Uploads one spinner animation (n RGBA8
 * frames of sw x sh, host memory) converted for `fmt`. */
int pp_spinner_upload(pp_ctx *ctx, int fmt, const uint8_t *rgba, int n,
                      int sw, int sh);
/* For each output frame k: dst[k] = src[src_index[k]] (or black when
 * src_index[k] < 0) with spinner frame spinner_index[k] composited centred
 * (no overlay when spinner_index[k] < 0).  Index arrays are host memory. */
int pp_stall_compose(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *src,
                     const int32_t *src_index, const int32_t *spinner_index,
                     const pp_frames *dst, int nframes, void *stream);

/* ---- which code paths a pad / CPVS / v210 / stall launch takes ------------
 * Host only: no GPU, no context, nothing is read through the data pointers.
 * The pad and stall row kernels and the fused CPVS kernel choose a path per
 * launch, row, 16-B chunk and chroma group (vector or sample-by-sample loads
 * and stores, image edges, pad rows, v210 tails, spinner overlap, frame
 * tiles ...).  The walker below runs the kernels' own predicates
 * (csrc/pack_plan.hpp) over every row, chunk and group of the launch the
 * query describes and reports the arms taken, so a test table can show that
 * it reaches every one.  Bit numbers of the mask: */
enum pp_pack_arm {
    /* fused CPVS kernel, per instance (8 / 10 bit x 4:2:0 / 4:2:2) */
    PP_ARM_CPVS_ROW_LIVE = 0,       /* canvas row inside the AVPVS */
    PP_ARM_CPVS_ROW_PAD,            /* canvas row above / below it */
    PP_ARM_CPVS_STAGE_VEC_ONE,      /* 16-B staging, one pass of 512 pieces */
    PP_ARM_CPVS_STAGE_VEC_MULTI,    /* 16-B staging, two or more passes */
    PP_ARM_CPVS_STAGE_SAMPLES,      /* unaligned rows: sample by sample */
    PP_ARM_CPVS_GROUP_VEC,          /* 4:2:0 chroma group: vector loads */
    PP_ARM_CPVS_GROUP_SAMPLES,      /* 4:2:0 chroma group: by samples */
    PP_ARM_CPVS_GROUP_CLAMPED,      /* ragged last group: min(x, cw - 1) */
    PP_ARM_CPVS_GROUP_VEC_RAGGED,   /* aligned rows, group past the padded row: unreachable (pack_plan.hpp) */
    PP_ARM_CPVS_TAP_ABOVE,          /* vertical tap row above the image: black */
    PP_ARM_CPVS_TAP_BELOW,          /* ... below it */
    PP_ARM_CPVS_GROUPS_GT64,        /* more chroma groups than lanes */
    PP_ARM_CPVS_C8_FAST,            /* uyvy422 chunk: 3 LDS words + v_perm */
    PP_ARM_CPVS_C8_OFFGRID,         /* chunk inside the AVPVS, pad offset off the 8-px grid: by samples */
    PP_ARM_CPVS_C8_SLOW_FULL,       /* other uyvy422 chunk by samples, 16-B store */
    PP_ARM_CPVS_C8_SLOW_TAIL,       /* uyvy422 last chunk, byte stores */
    PP_ARM_CPVS_V210_FULL,          /* v210 chunk of 6 pixels */
    PP_ARM_CPVS_V210_TAIL2,         /* v210 tail, W % 6 == 2 */
    PP_ARM_CPVS_V210_TAIL4,         /* v210 tail, W % 6 == 4 */
    PP_ARM_CPVS_V210_ZERO,          /* zero fill up to the line size */
    PP_ARM_CPVS_CHUNKS_GT64,        /* more output chunks than lanes */
    /* pad and stall row kernels, per sample size */
    PP_ARM_ROW_SRC_VEC,             /* source chunk: one 16-B load */
    PP_ARM_ROW_SRC_EDGE,            /* vector mode, chunk across an image edge: by samples */
    PP_ARM_ROW_SRC_OUTSIDE,         /* live row, chunk wholly in the pad columns (pad only) */
    PP_ARM_ROW_SRC_SCALAR,          /* unaligned source or shift: by samples throughout */
    PP_ARM_ROW_SRC_NULL,            /* no source row: black */
    PP_ARM_ROW_DST_VEC,             /* 16-B store */
    PP_ARM_ROW_DST_TAIL,            /* aligned destination, ragged last chunk */
    PP_ARM_ROW_DST_SCALAR,          /* unaligned destination: by samples throughout */
    PP_ARM_ROW_CHUNKS_GT256,        /* second trip of the chunk loop */
    PP_ARM_ROW_420,
    PP_ARM_ROW_422,
    PP_ARM_ROW_444,
    /* stall only */
    PP_ARM_STALL_TILE_FULL,         /* tile of G frames */
    PP_ARM_STALL_TILE_SHORT,        /* shorter last tile */
    PP_ARM_STALL_SRC_CHANGE,        /* source index changes inside a tile */
    PP_ARM_STALL_BLACK,             /* black source frame */
    PP_ARM_STALL_NO_SPINNER,        /* frame without a spinner */
    PP_ARM_STALL_SPIN_LEFT,         /* chunk across the spinner's left edge */
    PP_ARM_STALL_SPIN_RIGHT,        /* ... its right edge */
    PP_ARM_STALL_SPIN_INSIDE,       /* chunk wholly inside the spinner */
    PP_ARM_STALL_SPIN_CLIPPED,      /* spinner larger than the frame */
    PP_ARM_STALL_LAUNCH_SPLIT,      /* more than 256 frames: several launches */
    PP_ARM_COUNT
};
#define PP_PACK_OP_PAD 0
#define PP_PACK_OP_CPVS 1
#define PP_PACK_OP_V210 2
#define PP_PACK_OP_STALL 3
/* kernel instances, the return value of the walker */
#define PP_PACK_INST_CPVS8_420 0
#define PP_PACK_INST_CPVS8_422 1
#define PP_PACK_INST_CPVS10_420 2
#define PP_PACK_INST_CPVS10_422 3
#define PP_PACK_INST_PAD8 4
#define PP_PACK_INST_PAD16 5
#define PP_PACK_INST_STALL8 6
#define PP_PACK_INST_STALL16 7
/* One launch as the execute call would receive it.  src / dst carry only the
 * alignment facts (addresses, line sizes, frame strides); for PP_PACK_OP_V210
 * W, H, x, y are ignored; the stall fields are read for PP_PACK_OP_STALL only
 * (spin_n frames of spin_w x spin_h uploaded for `fmt`, spin_n = 0: none). */
typedef struct pp_pack_query {
    int op, fmt, w, h, W, H, x, y, nframes;
    pp_frames src, dst;
    const int32_t *src_index, *spinner_index;
    int spin_n, spin_w, spin_h;
} pp_pack_query;
/* Returns the kernel instance (PP_PACK_INST_*) and sets *arms, or returns the
 * error the execute call returns for this launch (same code, same message).
 * Added without raising PP_ABI_VERSION (still 7). */
int pp_pack_arms(const pp_pack_query *q, uint64_t *arms);

/* ---- P.910 SI/TI (spec PP-SITI-1) ------------------------
 * New feature behind util/SRC_analysis.py:120-147 (analyse_src) and
 * util/complexity_classification.py:50-69 (get_difficulty).
 * luma: nframes frames of w x h, 8- or 10-bit (uint16 LE), linesize and
 * frame_stride in bytes.  prev: the frame before luma[0] (1-frame halo) or
 * NULL.  si/ti: DEVICE arrays of nframes doubles; ti[0] is NaN without prev. */
int pp_siti(pp_ctx *ctx, int bitdepth, int w, int h, const void *luma,
            int64_t linesize, int64_t frame_stride, int nframes,
            const void *prev, double *si, double *ti, void *stream);
/* pp_siti with flags: PP_SITI_NORMALIZE divides SI_n and TI_n by
 * 2^(bitdepth-8) (SURVEY.md 8a-13's optional normalisation), so 8- and 10-bit
 * SRCs report on the 8-bit scale; an exact power-of-two scaling of the raw
 * values.  pp_siti(...) == pp_siti_ex(..., 0, stream). */
#define PP_SITI_NORMALIZE 1
int pp_siti_ex(pp_ctx *ctx, int bitdepth, int w, int h, const void *luma,
               int64_t linesize, int64_t frame_stride, int nframes,
               const void *prev, double *si, double *ti, int flags, void *stream);
/* The launch plan of the SI/TI kernel for `nframes` frames of w x h on `slots`
 * resident workgroups (csrc/siti_plan.hpp): host only, no context, no GPU.
 * Writes the first min(n, PP_SITI_PLAN_FIELDS) of
 *   tiles_x, bands, ntiles, ragged, interior_bands, fchunk, chunks, groups
 * to out: 1984-px tile columns, 16-row bands, their product, w % 8 != 0 (the
 * ragged kernel instances), bands whose 18 window rows all lie in the frame,
 * frames a (chunk, tile) unit walks, chunks (the last may be shorter), and
 * workgroups launched = min(slots, ntiles * chunks); nframes == 0 plans
 * fchunk = chunks = groups = 0.  Bad depth or size: the code and message of
 * pp_siti_ex; slots < 1, nframes < 0, out == NULL or n < 1: PP_ERR_INVALID.
 * Added without raising PP_ABI_VERSION (still 7). */
#define PP_SITI_PLAN_FIELDS 8
int pp_siti_plan(int bitdepth, int w, int h, int nframes, int slots,
                 int32_t *out, int n);
/* pp_siti_ex planned for `slots` resident workgroups instead of the device's
 * own count (CUs x occupancy): slots == 0 asks the device, so
 * pp_siti_ex(...) == pp_siti_slots(..., flags, 0, stream); slots < 0 is
 * PP_ERR_INVALID.  Any positive count is a legal launch (the grid never exceeds
 * the units) and the results do not depend on it, bit for bit: the plan decides
 * which workgroup computes a partial, never its arithmetic.  For tests, which
 * force small clips onto every arm of the kernel with it.  Added without
 * raising PP_ABI_VERSION (still 7). */
int pp_siti_slots(pp_ctx *ctx, int bitdepth, int w, int h, const void *luma,
                  int64_t linesize, int64_t frame_stride, int nframes,
                  const void *prev, double *si, double *ti, int flags, int slots,
                  void *stream);

/* ---- full-reference PSNR / SSIM (spec PP-METRIC-1) --------
 * New feature after p03_generateAvPvs.py: how far an AVPVS is from its SRC,
 * per frame and plane (the reference's image builds FFmpeg with libvmaf for
 * this step).  Modelled on vf_psnr / vf_ssim; parity with FFmpeg is unpinned.
 * ref, dist: batches of w x h frames of the planar format `fmt` (packed
 * formats: PP_ERR_INVALID); pitches and frame strides may differ.  dist frame
 * k is compared with ref frame ref_index[k] (HOST array of nframes entries,
 * NULL = identity; a negative entry is PP_ERR_INVALID).  sse / ssim: DEVICE
 * arrays of nframes x 3, frame-major: the exact sum of squared differences of
 * every sample of the plane, and the mean SSIM over its 8x8 windows at stride
 * 4 (NaN for a plane under 8 samples wide or high).  Arguments are checked
 * before any HIP call.  The partials workspace belongs to the context.
 * Added without raising PP_ABI_VERSION (still 7): the addition is backward
 * compatible, no existing entry point or structure changed. */
int pp_metrics(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *ref,
               const pp_frames *dist, const int32_t *ref_index, int nframes,
               uint64_t *sse, double *ssim, void *stream);

/* ---- per-frame Adler-32 (spec PP-HASH-1) -------------------
 * The checksum FFmpeg's framecrc muxer prints for a frame, computed where the
 * frame lies: 4 bytes a frame leave the device.  src: nframes w x h frames of
 * any of the eight formats.  The byte string of a frame: planar formats plane
 * 0, 1, 2, each row by row, the first width * bytes_per_sample bytes of every
 * row exactly as stored (10-bit samples as their two little-endian bytes,
 * nothing masked); uyvy422 the 2 w bytes of every row of plane 0; v210 the
 * pp_v210_linesize(w) bytes of every row of plane 0 (the packet v210enc
 * writes, zero fill included).  Bytes between a row's extent and its linesize
 * never count.  out: DEVICE array of nframes uint32: Adler-32 of the string
 * continued from `init` (low half a0, high half b0; 1 is zlib's default, 0
 * framecrc's), i.e. zlib's adler32(init, bytes, N).  Exact for every size
 * the call accepts.  An odd w of a packed format, a linesize below the row's
 * bytes (v210: below pp_v210_linesize(w)), nframes < 0, w or h < 1 and NULL
 * ctx, src, out or plane pointers are PP_ERR_INVALID; rows of 2^24 bytes or
 * more and planes past the 2 GiB buffer range are PP_ERR_UNSUPPORTED.
 * Arguments are checked before any HIP call; nframes == 0 is PP_OK.  Sources
 * on the 16-byte grid (pointers, linesizes, frame strides) are read as 16-byte
 * loads, anything else byte by byte with identical results.  The partials
 * workspace belongs to the context.  Parity with FFmpeg's framecrc is
 * unpinned.  Added without raising PP_ABI_VERSION (still 7). */
int pp_frame_adler32(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *src,
                     int nframes, uint32_t init, uint32_t *out, void *stream);

/* ---- per-frame signal statistics (spec PP-STATS-1) ----------
 * What is inside a clip: per frame and plane the histogram of the samples and
 * the sum of absolute differences to the previous frame, in one pass over the
 * frames where they lie.  src: nframes w x h frames of one of the six planar
 * formats (a packed format is PP_ERR_INVALID: unpack it first with
 * pp_unpack_execute).  Plane sizes follow pp_plane_bytes' rule (a chroma plane
 * is (w+1)>>hsub by (h+1)>>vsub); only the first width samples of a row count,
 * pitch padding never does.  Three DEVICE arrays, frame-major, each written in
 * full (the caller need not clear them):
 *   hist [nframes][3][bins] uint32, bins = 1 << depth (256 or 1024):
 *        hist[k][p][v] = samples of plane p of frame k equal to v; a stored
 *        16-bit sample >= 1024 of a 10-bit format is in no bin;
 *   over [nframes][3] uint32: the 10-bit samples >= 1024 (0 for 8-bit
 *        formats); sum(hist[k][p]) + over[k][p] == samples of the plane;
 *   sad  [nframes][3] uint64: sum over the plane of |src[k] - src[k-1]| on the
 *        samples as stored (the raw 16-bit value, nothing masked).  Frame 0 is
 *        compared with `prev`, a one-frame batch of the same fmt, w and h with
 *        pitches of its own; without prev (NULL) sad[0][p] = UINT64_MAX:
 *        absent, as pp_siti's NaN ti[0].  sad == NULL skips the differences
 *        (prev is then ignored).
 * All three are exact integers and identical from run to run.  NULL ctx, src,
 * hist, over or plane pointers, w or h < 1, nframes < 0 and a linesize below
 * the row's bytes are PP_ERR_INVALID; a plane of 2^31 samples or more (a bin
 * is 32 bits) or past the 2 GiB buffer range is PP_ERR_UNSUPPORTED.  Arguments
 * are checked before any HIP call; nframes == 0 is PP_OK and writes nothing.
 * Sources on the 16-byte grid (pointers, linesizes, frame strides, prev's too)
 * are read as 16-byte loads, anything else byte by byte with identical
 * results.  The workspace (one histogram per frame and 64-row x 1024-byte
 * tile) belongs to the context.  Parity of the derived values with FFmpeg's
 * signalstats / blackdetect / freezedetect is unpinned.  Added without raising
 * PP_ABI_VERSION (still 7). */
int pp_frame_stats(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *src,
                   int nframes, const pp_frames *prev,
                   uint32_t *hist, uint64_t *sad, uint32_t *over, void *stream);

/* ---- luma SSE of every distorted frame against a band of reference frames
 * (spec PP-ALIGN-1) -------------------------------------------
 * The sums a temporal alignment searches: dist holds ndist luma planes of
 * w x h samples, ref holds nref of them, each with a pitch and frame stride of
 * its own.  bitdepth 8: bytes; 10: uint16 LE taken as stored, nothing masked
 * (as pp_metrics and pp_frame_stats).  first: HOST array of ndist entries.
 *   sse [ndist][ncand] uint64, DEVICE, every element written:
 *        sse[k][c] = sum over the w x h samples of
 *        (dist[k] - ref[first[k] + c])^2, exact; UINT64_MAX (absent, as
 *        pp_frame_stats' sad) where first[k] + c lies outside [0, nref).
 *        A negative first[k] only makes the leading candidates absent.
 * Pitch padding never counts.  The results are exact integers and identical
 * from run to run for every stored 16-bit value.  NULL ctx, dist, ref, first
 * or sse, w or h < 1, ndist or nref < 0, ncand < 1, a linesize below the row's
 * bytes, 16-bit samples off the 2-byte grid and a bitdepth other than 8 or 10
 * are PP_ERR_INVALID; a plane past the 2 GiB buffer range is
 * PP_ERR_UNSUPPORTED.  Arguments are checked before any HIP call; ndist == 0
 * is PP_OK and writes nothing.  Sources on the 16-byte grid (both pointers,
 * linesizes and frame strides) are read with 16-byte loads, dist once and ref
 * once per candidate; if either is off the grid both are read element by
 * element, with identical results.  The workspace (one partial per
 * frame, candidate and 64-row x 1024-byte tile) belongs to the context.  No
 * reference implementation exists: parity is unpinned.  Added without raising
 * PP_ABI_VERSION (still 7). */
int pp_frame_sse_band(pp_ctx *ctx, int bitdepth, int w, int h,
                      const void *dist, int64_t dist_linesize, int64_t dist_frame_stride, int ndist,
                      const void *ref, int64_t ref_linesize, int64_t ref_frame_stride, int nref,
                      const int32_t *first, int ncand, uint64_t *sse, void *stream);

/* ---- multi-scale SSIM of a distorted luma batch against its reference
 * (spec PP-MSSSIM-1) ------------------------------------------
 * MS-SSIM after Wang, Simoncelli & Bovik 2003, the metric between pp_metrics'
 * block SSIM and VMAF: five dyadic scales (scale s = the means of the 2^s x 2^s
 * blocks, trailing w mod 2^s columns and h mod 2^s rows dropped), an 11 x 11
 * Gaussian window (sigma 1.5) at every position where all 121 samples exist,
 * K1 = .01, K2 = .03, L = 2^bitdepth - 1.  ref holds nref luma planes of
 * w x h samples, dist holds ndist of them, each with a pitch and frame stride
 * of its own.  bitdepth 8: bytes; 10: uint16 LE taken as stored, nothing masked
 * (as pp_frame_sse_band).  dist frame k is compared with ref frame
 * ref_index[k] (HOST array of ndist entries, NULL = identity, which needs
 * ndist <= nref; an entry outside [0, nref) is PP_ERR_INVALID).
 *   out [ndist][5][2] double, DEVICE, every element written and nothing else:
 *        out[k][s][0] = mean of cs = (2 sigma_ab + C2) / (sigma_a^2 +
 *        sigma_b^2 + C2) over the (w_s - 10)(h_s - 10) windows of scale s,
 *        out[k][s][1] = mean of l * cs (the scale's SSIM; s = 0 is the
 *        Gaussian-window SSIM of the 2004 paper); both NaN for a scale under
 *        11 samples wide or high.  Scale 4 has a window from 176 x 176 on.
 * The five exponents and the product (clamping negative means to 0) are host
 * arithmetic: pixpath/msssim.py `pool`.  The number of scales is fixed by the
 * paper's exponents, so the call has no scale-count argument.  Everything is
 * fp64 on exact integer pyramids; identical planes give exactly 1.0, and two
 * runs give the same bits (no atomics, partials added in a fixed order).
 * Pitch padding never counts.  NULL ctx, ref, dist or out, w or h < 1, ndist or
 * nref < 0, a linesize below the row's bytes, 16-bit samples off the 2-byte
 * grid and a bitdepth other than 8 or 10 are PP_ERR_INVALID; a plane past the
 * 2 GiB buffer range is PP_ERR_UNSUPPORTED.  Arguments are checked before any
 * HIP call; ndist == 0 is PP_OK and writes nothing.  Every sample is loaded as
 * one element, whatever grid the pointers, linesizes and frame strides lie on:
 * the kernel is bound by its arithmetic, and the layout of the same samples
 * cannot change a bit of the result.  The workspace (both integer pyramids of
 * up to 256 frames or 1 GiB a launch, one partial per frame, scale and tile of
 * 256 x 64 windows) belongs to the context.  Parity with libvmaf's
 * float_ms_ssim, which downsamples with another low-pass filter, is unpinned.
 * Added without raising PP_ABI_VERSION (still 7). */
int pp_ms_ssim(pp_ctx *ctx, int bitdepth, int w, int h,
               const void *ref, int64_t ref_linesize, int64_t ref_frame_stride, int nref,
               const void *dist, int64_t dist_linesize, int64_t dist_frame_stride, int ndist,
               const int32_t *ref_index, double *out, void *stream);

/* ---- pixel-domain VIF of a distorted luma batch against its reference
 * (spec PP-VIF-1) ---------------------------------------------
 * Visual Information Fidelity after Sheikh & Bovik 2006 in the four-scale
 * pixel-domain form VMAF uses as vif_scale0..3.  Samples are brought to the
 * 8-bit scale (sample / 2^(bitdepth - 8), exact); scale s = 0 .. 3 has
 * w >> s x h >> s samples and a Gaussian window of 17, 9, 5, 3 taps (sigma =
 * taps / 5, normalised in fp64); scale s + 1 is scale s under the window of
 * scale s + 1, even rows and columns kept.  Borders are mirrored without
 * repeating the edge sample on all four sides, so every sample position of a
 * scale has a window.  A scale exists if it is at least taps / 2 + 1 samples
 * wide and high (9, 5, 3, 2; all four from 16 x 16 on).  ref, dist, bitdepth,
 * ref_index and their rules are pp_ms_ssim's: bitdepth 8 is bytes, 10 is
 * uint16 LE taken as stored, nothing masked; dist frame k is compared with ref
 * frame ref_index[k] (HOST array of ndist entries, NULL = identity, which needs
 * ndist <= nref; an entry outside [0, nref) is PP_ERR_INVALID).
 *   out [ndist][4][2] double, DEVICE, every element written and nothing else:
 *        out[k][s][0] = sum of num, out[k][s][1] = sum of den over the
 *        (w >> s)(h >> s) positions of scale s (sigma_n^2 = 2, eps = 1e-10, the
 *        steps of DESIGN.md in order); both NaN for a scale that does not exist
 *        and for every later one.
 * vif_scale_s = num_s / den_s and vif = sum num / sum den are host arithmetic:
 * pixpath/vif.py `pool`.  Everything is fp64.  Identical planes give values
 * within 1e-9 of 1 where sigma_1^2 >= 2 everywhere, not exactly 1: eps keeps
 * the gain just under 1.  Two runs give the same bits (no atomics, partials
 * added in a fixed order).  Pitch padding never counts.  NULL ctx, ref, dist or
 * out, w or h < 1, ndist or nref < 0, a linesize below the row's bytes, 16-bit
 * samples off the 2-byte grid and a bitdepth other than 8 or 10 are
 * PP_ERR_INVALID; a plane past the 2 GiB buffer range is PP_ERR_UNSUPPORTED.
 * Arguments are checked before any HIP call; ndist == 0 is PP_OK and writes
 * nothing.  Every sample is loaded as one element at a mirrored position,
 * whatever grid the pointers, linesizes and frame strides lie on: the layout of
 * the same samples cannot change a bit of the result.  The workspace (fp64
 * pyramid levels 1 .. 3 of both planes of up to 256 frames or 1 GiB a launch,
 * about 11 MB a frame at 1080p, and one partial per frame, scale and tile of
 * 256 x 64 positions) belongs to the context.  The constants are those
 * published for VMAF's VIF feature; parity with libvmaf's float_vif is
 * unpinned: no libvmaf exists to compare with, and its border and decimation
 * details could not be read.  Added without raising PP_ABI_VERSION (still 7). */
int pp_vif(pp_ctx *ctx, int bitdepth, int w, int h,
           const void *ref, int64_t ref_linesize, int64_t ref_frame_stride, int nref,
           const void *dist, int64_t dist_linesize, int64_t dist_frame_stride, int ndist,
           const int32_t *ref_index, double *out, void *stream);

/* ---- Additive / Detail-loss Metric of a distorted luma batch against its
 * reference (spec PP-ADM-1) -----------------------------------
 * ADM after Li, Ngan et al. 2011 in the four-scale form VMAF uses as adm2 and
 * adm_scale0..3.  Samples are brought to the 8-bit scale (sample /
 * 2^(bitdepth - 8), exact).  Level s = 0 .. 3 of the Daubechies-2 transform has
 * (w_{s-1} + 1) / 2 x (h_{s-1} + 1) / 2 coefficients (level -1: the plane);
 * coefficient i of an axis reads inputs 2i - 1 .. 2i + 2 under the low-pass or
 * high-pass taps, borders mirrored without repeating the edge sample; rows are
 * filtered first, then columns; level s + 1 is taken from the approximation
 * band of level s.  Per position the distorted H, V, D coefficients are
 * decoupled into a restored and an additive part (gain clipped to [0, 1]; both
 * directions within one degree: all restored), weighted by the contrast
 * sensitivity rf[s][theta], and the restored part is lowered by the masking
 * threshold M taken from the additive part's 3 x 3 neighbourhood.  A scale
 * exists if its input and its bands are at least 3 samples wide and high (all
 * four from 33 x 33 on).  ref, dist, bitdepth, ref_index and their rules are
 * pp_vif's: bitdepth 8 is bytes, 10 is uint16 LE taken as stored, nothing
 * masked; dist frame k is compared with ref frame ref_index[k] (HOST array of
 * ndist entries, NULL = identity, which needs ndist <= nref; an entry outside
 * [0, nref) is PP_ERR_INVALID).
 *   out [ndist][4][6] double, DEVICE, every element written and nothing else:
 *        out[k][s][0..2] = sum of max(|rf r| - M, 0)^3 for H, V, D and
 *        out[k][s][3..5] = sum of |rf o|^3 for H, V, D over the region of scale
 *        s (the band less a margin of max(1, (n - 5) / 10) on every side); all
 *        six NaN for a scale that does not exist and for every later one.
 * adm_scale_s and adm2 are host arithmetic: pixpath/adm.py `pool`.  Everything
 * is fp64.  Identical planes give the same bits in out[k][s][i] and
 * out[k][s][3 + i], so every pooled value is exactly 1.0.  Two runs give the
 * same bits (no atomics, partials added in a fixed order).  Pitch padding never
 * counts.  NULL ctx, ref, dist or out, w or h < 1, ndist or nref < 0, a
 * linesize below the row's bytes, 16-bit samples off the 2-byte grid and a
 * bitdepth other than 8 or 10 are PP_ERR_INVALID; a plane past the 2 GiB
 * buffer range is PP_ERR_UNSUPPORTED.  Arguments are checked before any HIP
 * call; ndist == 0 is PP_OK and writes nothing.  Every sample is loaded as one
 * element at a mirrored position, whatever grid the pointers, linesizes and
 * frame strides lie on: the layout of the same samples cannot change a bit of
 * the result.  The workspace (fp64 approximation bands of levels 0 .. 2 of
 * both planes of up to 256 frames or 1 GiB a launch, about 11 MB a frame at
 * 1080p, and one partial per frame, scale and tile of 254 x 32 coefficients)
 * belongs to the context; the H, V and D bands are never stored.  The
 * constants are those published for VMAF's ADM feature; parity with libvmaf's
 * float_adm is unpinned: no libvmaf exists to compare with.  Added without
 * raising PP_ABI_VERSION (still 7). */
int pp_adm(pp_ctx *ctx, int bitdepth, int w, int h,
           const void *ref, int64_t ref_linesize, int64_t ref_frame_stride, int nref,
           const void *dist, int64_t dist_linesize, int64_t dist_frame_stride, int ndist,
           const int32_t *ref_index, double *out, void *stream);

/* ---- CIEDE2000 colour difference of a distorted batch against its reference
 * (spec PP-CIEDE-1) --------------------------------------------
 * The one measure that reads chroma on a perceptual scale: the CIE's dE00
 * (Sharma, Wu, Dalal 2005) of every luma position of a frame pair.  ref, dist:
 * batches of w x h frames of the planar format `fmt` (packed formats:
 * PP_ERR_INVALID; unpack them first with pp_unpack_execute); pitches and frame
 * strides may differ.  dist frame k is compared with ref frame ref_index[k]
 * (HOST array of ndist entries, NULL = identity, which needs ndist <= nref; an
 * entry outside [0, nref) is PP_ERR_INVALID).  Position (x, y) takes luma[y][x]
 * and the chroma samples at [y >> vsub][x >> hsub] (nearest, no interpolation;
 * odd sizes: the ceil-sized chroma planes of pp_plane_bytes), as stored, nothing
 * masked.  With s = 2^(depth - 8): y' = (Y - 16 s) / (219 s), cb, cr = (U, V -
 * 128 s) / (224 s) (limited range, samples outside it used as they are); the
 * BT.709 matrix, each of R, G, B clipped to [0, 1]; the sRGB curve to linear
 * light; XYZ (D65) over its white; Lab; dE00 with the weights kL, kC, kH (the
 * CIE's: 1, 1, 1).  Everything is IEEE double in the order DESIGN.md writes.
 *   out [ndist][2] double, DEVICE, every element written and nothing else:
 *        out[k][0] = the sum of dE00 over the w h positions of frame k,
 *        out[k][1] = the largest dE00 of frame k.
 * delta_e = sum / (w h) and the score min(45 - 20 log10(delta_e), 100) are
 * host arithmetic: pixpath/ciede.py `pool`.  A pair of equal Y, U and V skips
 * the maths; its dE00 is exactly 0 either way, so identical frames give 0.0
 * and 0.0.  Two runs give the same bits (no atomics, partials added in a fixed
 * order), and the layout of the same samples (pitches, pointers or strides on
 * or off the 16-byte grid) cannot change a bit of the result.  Pitch padding
 * never counts.  NULL ctx, ref, dist or out, a packed or unknown format, w or
 * h < 1, ndist or nref < 0, a null plane, a linesize below the row's bytes,
 * 16-bit samples off the 2-byte grid and a weight that is not positive and
 * finite are PP_ERR_INVALID; a plane past the 2 GiB buffer range is
 * PP_ERR_UNSUPPORTED.  Arguments are checked before any HIP call; ndist == 0
 * is PP_OK and writes nothing.  The partials workspace (16 bytes per unit of
 * 64 chroma pieces x 16 chroma rows) belongs to the context.  Modelled on
 * libvmaf's `ciede` feature as recalled (which is recalled to use other
 * weights, hence the parameters); parity with it is unpinned: no libvmaf
 * exists to compare with.  Added without raising PP_ABI_VERSION (still 7). */
int pp_ciede(pp_ctx *ctx, int fmt, int w, int h,
             const pp_frames *ref, const pp_frames *dist,
             const int32_t *ref_index, int nref, int ndist,
             double kL, double kC, double kH,
             double *out /* DEVICE, ndist x 2: sum, max */,
             void *stream);

/* ---- PSNR-HVS and PSNR-HVS-M of a distorted batch against its reference
 * (spec PP-HVS-1) ------------------------------------------------
 * The contrast-sensitivity-weighted PSNR over 8 x 8 DCT blocks, without and
 * with between-coefficient contrast masking, of each of the three planes.
 * ref, dist: batches of w x h frames of the planar format `fmt` (packed
 * formats: PP_ERR_INVALID; unpack them first with pp_unpack_execute); pitches
 * and frame strides may differ.  dist frame k is compared with ref frame
 * ref_index[k] (HOST array of ndist entries, NULL = identity, which needs
 * ndist <= nref; an entry outside [0, nref) is PP_ERR_INVALID).  Samples are
 * used as stored, nothing masked or clipped.  Per plane of pw x ph samples the
 * blocks have their origins at (i step, j step) for every i, j with origin + 8
 * <= the plane's size; `step` is 8 (the published definition) or 7 (blocks
 * overlap by a sample, so that an 8-grid codec's block edges fall inside
 * blocks); per axis nb(n) = n < 8 ? 0 : (n - 8) / step + 1, and samples right
 * of or below the last block do not count.  Per block of A (ref) and B (dist):
 * D(X) the orthonormal 2-D DCT-II, rows first; with Q the JPEG Annex K
 * luminance table, CSF the published six-decimal contrast-sensitivity table
 * (25.735088 / Q to 5.5e-7; DESIGN.md prints it) and M = (10 / Q)^2 (the same
 * tables for all three planes: build-defined, the published measure is for
 * grey pictures); m = the sum over (k, l) != (0, 0) of D(X)[k][l]^2 M[k][l]; pop =
 * 21 (sum of V_q of the four 4 x 4 quadrants) / (5 V) in exact 64-bit integers,
 * V = 64 sum x^2 - (sum x)^2, V_q = 16 sum_q x^2 - (sum_q x)^2, 0 for V = 0;
 * mask(X) = sqrt(m pop) / 32; T = max(mask(A), mask(B)); u = |D(A) - D(B)|;
 * S_hvs adds (u CSF)^2 over the 64 coefficients; S_hvsm the same after u =
 * max(u - T / M, 0) at every coefficient but DC.  Everything floating is IEEE
 * double in the order DESIGN.md writes.
 *   out [ndist][3][2] double, DEVICE, every element written and nothing else:
 *        out[k][p][0] = S_hvs, out[k][p][1] = S_hvsm of plane p (Y, U, V) of
 *        frame k, summed over its blocks; 0.0, 0.0 for a plane with no block
 *        (under 8 samples in a direction).
 * mse = S / (64 blocks), psnr = 10 log10(peak^2 / mse) and the `all` value
 * from 0.8 mse_y + 0.1 (mse_u + mse_v) are host arithmetic: pixpath/psnrhvs.py
 * `pool`.  Identical blocks give exactly 0 and 0; S_hvsm <= S_hvs.  Two runs
 * give the same bits (no atomics, partials added in a fixed order), and the
 * layout of the same samples (pitches, pointers or strides on or off the
 * 16-byte grid) cannot change a bit of the result.  Pitch padding never
 * counts.  NULL ctx, ref, dist or out, a packed or unknown format, w or h < 1,
 * ndist or nref < 0, a step other than 7 or 8, a null plane, a linesize below
 * the row's bytes and 16-bit samples off the 2-byte grid are PP_ERR_INVALID; a
 * plane past the 2 GiB buffer range is PP_ERR_UNSUPPORTED.  Arguments are
 * checked before any HIP call; ndist == 0 is PP_OK and writes nothing.  The
 * partials workspace (16 bytes per unit of 32 blocks of a block row) belongs
 * to the context.  Modelled on Ponomarenko et al. (2007), the published
 * psnrhvsm definition, and on libvmaf's `psnr_hvs` feature as recalled (step
 * 7, the 0.8 / 0.1 / 0.1 weighting); parity with both is unpinned: neither
 * exists to compare with.  Added without raising PP_ABI_VERSION (still 7). */
int pp_psnr_hvs(pp_ctx *ctx, int fmt, int w, int h,
                const pp_frames *ref, const pp_frames *dist,
                const int32_t *ref_index, int nref, int ndist, int step,
                double *out /* DEVICE, ndist x 3 x 2: per plane S_hvs, S_hvsm */,
                void *stream);

/* ---- VMAF-style motion of a luma sequence (spec PP-MOTION-1) --
 * The temporal feature VMAF calls motion / motion2: every shown frame's luma
 * is blurred with the separable integer filter f = {3571, 16004, 26386, 16004,
 * 3571} (sum 65536), columns first, a rounding after each pass:
 *   t(i, j) = (sum_k f[k] x(m(i + k - 2, h), j) + 2^(d-1)) >> d
 *   B(i, j) = (sum_k f[k] t(i, m(j + k - 2, w)) + 32768) >> 16
 * with d = bitdepth and m mirroring without repeating the edge sample
 * (PP-VIF-1's rule).  bitdepth 8 is bytes, 10 is uint16 LE; unlike the
 * comparison metrics a stored sample above 2^d - 1 counts as 2^d - 1 (x =
 * min(stored, 2^d - 1)): that keeps every intermediate below 2^32 and B in 16
 * bits (B <= 65472).  A constant plane c gives B = c 2^(16-d) exactly.  The
 * shown sequence is src[index[0]], .., src[index[n-1]] (index: HOST array of n
 * entries, NULL = identity, which needs n <= nsrc; an entry outside [0, nsrc)
 * is PP_ERR_INVALID; repeats and backward steps are allowed, a repeat gives
 * exactly 0).
 *   sad [n] uint64, DEVICE, every element written and nothing else:
 *        sad[k] = sum over the plane of |B(src[index[k]]) - B(src[index[k-1]])|,
 *        exact, < 2^47; sad[0] is taken against `prev` (one luma plane of the
 *        same w, h and bitdepth, pitch prev_linesize), or is UINT64_MAX =
 *        absent when prev is NULL (as pp_frame_stats' sad); with w < 3 or
 *        h < 3 one reflection does not suffice and every entry is absent.
 * motion = sad / 256 / (w h) (the 8-bit scale at both depths) and motion2 are
 * host arithmetic: pixpath/motion.py `pool`.  Everything is 32-bit unsigned
 * integer arithmetic, 64-bit from the tile's sum up: no float, no atomics,
 * partials added in a fixed order, two runs give the same bits.  Pitch padding
 * never counts.  NULL ctx, src or sad, w or h < 1, n or nsrc < 0, a linesize
 * below the row's bytes, 16-bit samples off the 2-byte grid and a bitdepth
 * other than 8 or 10 are PP_ERR_INVALID; a plane past the 2 GiB buffer range
 * is PP_ERR_UNSUPPORTED.  Arguments are checked before any HIP call; n == 0 is
 * PP_OK and writes nothing.  Pointers, linesizes and the frame stride on the
 * 16-B grid take 16-B loads, anything else element loads with the same
 * results.  A workgroup walks a segment of 4 shown frames over its tile with
 * the previous frame's blurred tile in registers: no blurred sample is ever
 * stored, and the workspace (one 64-bit partial per frame and tile of 64 rows
 * x 62 16-B pieces, up to 256 frames a launch) belongs to the context.  The
 * taps, the two roundings and the / 256 are libvmaf's integer motion as
 * recalled, the mirror rule is this library's; parity with libvmaf is
 * unpinned: no libvmaf exists to compare with.  Added without raising
 * PP_ABI_VERSION (still 7). */
int pp_motion(pp_ctx *ctx, int bitdepth, int w, int h,
              const void *src, int64_t src_linesize, int64_t src_frame_stride, int nsrc,
              const int32_t *index, int n,
              const void *prev, int64_t prev_linesize,
              uint64_t *sad, void *stream);

/* ---- Banding detection of a luma sequence (spec PP-BAND-1) ----
 * A no-reference measure of banding (staircase gradients) modelled on CAMBI
 * (Tandon et al., PCS 2021) as recalled and defined by DESIGN.md's text alone:
 * no display-luminance model, a mask threshold, a tie rule of the mode filter
 * and integer contrast values of its own.  Per shown frame: the luma is brought
 * to the ten-bit scale (bitdepth 8: bytes, x << 2; 10: uint16 LE, min(x, 1023),
 * PP-MOTION-1's rule), averaged over 2 x 2 against dither, masked to its flat
 * areas (a 7 x 7 count of samples equal to their right and lower neighbour, at
 * least 25), and reduced four times by a 3 x 3 mode filter and decimation by 2:
 * scale s + 1 has (w_s + 1) / 2 x (h_s + 1) / 2 positions, and all five scales
 * exist for every w, h >= 1.  At every masked position of every scale the
 * masked samples of the values v - 4 .. v + 4 inside the window x window
 * neighbourhood are counted (v the position's value; the same number of samples
 * at every scale), and the contrast value is
 *   Q = max over k = 1 .. 4 with v <= tvi[k-1] and both signs of
 *       floor(1024 k n_0 n_k / ((n_0 + n_k) window^2))  <= 1023,
 * 0 at an unmasked position.  The shown sequence is src[index[0]], ..,
 * src[index[n-1]] (index: HOST array of n entries, NULL = identity, which
 * needs n <= nsrc; an entry outside [0, nsrc) is PP_ERR_INVALID; repeats and
 * backward steps are allowed and give identical rows).
 *   window  odd, 3 .. 63; anything else is PP_ERR_INVALID
 *   tvi     HOST array of four entries, the largest v at which a step of
 *           k = 1 .. 4 codes counts; NULL = 1023 for all four.  The hook for a
 *           display model; none ships.
 *   hist    [n][5][1024] uint32, DEVICE, every element written and nothing
 *           else: hist[k][s][q] = positions of scale s of frame k with Q = q;
 *           the sum over q is w_s h_s.
 * The banding index is host arithmetic on the histograms: pixpath/banding.py
 * `pool`.  Everything is exact integer arithmetic (the quotient: two exact
 * integers divided in fp64 and floored, which is the integer quotient here);
 * the bins are added with integer atomics, so two runs give the same bits.
 * Pitch padding never counts.  NULL ctx, src or hist, w or h < 1, n or nsrc
 * < 0, a linesize below the row's bytes, 16-bit samples off the 2-byte grid
 * and a bitdepth other than 8 or 10 are PP_ERR_INVALID; a plane past the 2 GiB
 * buffer range is PP_ERR_UNSUPPORTED.  Arguments are checked before any HIP
 * call; n == 0 is PP_OK and writes nothing.  Every sample is loaded as one
 * element, whatever grid the pointer, linesize and frame stride lie on: the
 * layout of the same samples cannot change a bit of the result.  The workspace
 * (the five levels, 16 bits a position, of up to 256 frames or 1 GiB a launch:
 * about 5.5 MB a frame at 1080p) belongs to the context.  Parity with libvmaf's
 * CAMBI is unpinned: no libvmaf exists to compare with.  Added without raising
 * PP_ABI_VERSION (still 7). */
int pp_banding(pp_ctx *ctx, int bitdepth, int w, int h,
               const void *src, int64_t src_linesize, int64_t src_frame_stride, int nsrc,
               const int32_t *index, int n,
               int window, const uint16_t *tvi,
               uint32_t *hist, void *stream);

/* ---- DCT-energy complexity of a luma sequence (spec PP-DCTE-1)
 * A no-reference content descriptor of a clip, modelled on the texture energy
 * of the Video Complexity Analyzer (Menon et al., 2022): the weight formula is
 * VCA's as recalled, the integer transform, its two roundings and the
 * brightness are this library's own; parity with VCA is unpinned: no VCA exists
 * to compare with.  The normative text is the header comment of
 * csrc/dctenergy.hip; in short: bitdepth d of 8 (bytes) or 10 (uint16 LE),
 * x = min(stored, 2^d - 1) (PP-MOTION-1's rule).  Blocks are the
 * non-overlapping 32 x 32 squares at multiples of 32 wholly inside the plane:
 * bx = w / 32, by = h / 32 (floor); the ragged right and bottom remainder is not
 * analysed.  With the integer tables C (2^14 times the orthonormal 32-point
 * DCT-II, |C| <= 4096) and W (<= 696) of csrc/dct32_tables.hpp, in signed
 * 32-bit arithmetic with arithmetic shifts:
 *   T[i][k] = (sum_n C[k][n] x[i][n] + 2^(d+3)) >> (d + 4)
 *   Y[l][k] = (sum_i C[l][i] T[i][k] + 2^13) >> 14
 *   e_b = sum over (l, k) != (0, 0) of W[l][k] |Y[l][k]|,   dc_b = Y[0][0]
 * (both depths on one scale: four times the orthonormal transform of the 8-bit
 * picture).  The shown sequence is src[index[0]], .., src[index[n-1]] (index:
 * HOST array of n entries, NULL = identity, which needs n <= nsrc; an entry
 * outside [0, nsrc) is PP_ERR_INVALID; repeats and backward steps are allowed).
 *   out    [n][3] uint64, DEVICE, every element written:
 *          out[k][0] energy = sum_b e_b, out[k][1] dc = sum_b dc_b,
 *          out[k][2] tdiff = sum_b |e_b(k) - e_b(k-1)| against the frame shown
 *          before; tdiff of frame 0 is taken against `prev` (one luma plane of
 *          the same w, h and bitdepth, pitch prev_linesize), or is UINT64_MAX
 *          = absent when prev is NULL; a repeated frame gives exactly 0.  With
 *          w < 32 or h < 32 no block exists and all three are absent.
 *   blocks [n][by bx] uint64, DEVICE, row-major, may be NULL: the e_b, the
 *          spatial complexity map; its sum over b is energy.
 * E = energy / (nb 2^20), h = tdiff / (nb 2^20) and L = dc / (128 nb) (the mean
 * luma of the covered area on the 8-bit scale; VCA's L is a square root of the
 * DC) are host arithmetic: pixpath/dctenergy.py `pool`.  Exact integer
 * arithmetic, no float, no atomics, sums in a fixed order: two runs give the
 * same bits.  Pitch padding and the ragged remainder never count.  NULL ctx,
 * src or out, w or h < 1, n or nsrc < 0, a linesize below the row's bytes,
 * 16-bit samples off the 2-byte grid and a bitdepth other than 8 or 10 are
 * PP_ERR_INVALID; a plane past the 2 GiB buffer range is PP_ERR_UNSUPPORTED.
 * Arguments are checked before any HIP call; n == 0 is PP_OK and writes
 * nothing.  Pointers, linesizes and the frame stride on the 16-B grid take 16-B
 * loads, anything else element loads with the same results.  The workspace
 * (16 bytes per block and frame, one frame more than a launch's up to 256)
 * belongs to the context.  Added without raising PP_ABI_VERSION (still 7). */
int pp_dct_energy(pp_ctx *ctx, int bitdepth, int w, int h,
                  const void *src, int64_t src_linesize, int64_t src_frame_stride, int nsrc,
                  const int32_t *index, int n,
                  const void *prev, int64_t prev_linesize,
                  uint64_t *out, uint64_t *blocks, void *stream);

/* ---- host helpers --------------------------------------------------------
 * vf_fps output->input frame map (lib/ffmpeg.py:832-834, :959-961, :1038,
 * :1179): map[k] = input frame shown at output frame k.  Returns the number of
 * output frames (<= capacity) or <0. */
int pp_fps_map(int n_in, int64_t in_num, int64_t in_den, int64_t out_num,
               int64_t out_den, int32_t *map, int capacity);

/* ---- host transfer: device / pinned host memory, streams, events, copies --
 * SURVEY.md 8(b) "pinned host alloc + async H2D/D2H on caller-supplied
 * streams": everything a host without torch needs between ffmpeg's decode
 * pipe and its encode pipe (the reference hands frames between decoder,
 * filter graph and encoder inside one ffmpeg process, lib/ffmpeg.py:992-998).
 * Streams and events are hipStream_t / hipEvent_t passed as void*.  The
 * caller owns every buffer it allocates here and frees it with the matching
 * call. */
#define PP_COPY_H2D 1
#define PP_COPY_D2H 2
#define PP_COPY_D2D 3
int pp_device_alloc(pp_ctx *ctx, int64_t bytes, void **out);
int pp_device_free(pp_ctx *ctx, void *ptr);
int pp_host_alloc(int64_t bytes, void **out);   /* page-locked (pinned) */
int pp_host_free(void *ptr);
int pp_stream_create(pp_ctx *ctx, void **out);  /* non-blocking stream */
int pp_stream_destroy(pp_ctx *ctx, void *stream);
int pp_stream_synchronize(void *stream);
int pp_event_create(pp_ctx *ctx, void **out);
int pp_event_destroy(void *event);
int pp_event_record(void *event, void *stream);
int pp_stream_wait_event(void *stream, void *event);
int pp_event_synchronize(void *event);
int pp_event_elapsed_ms(void *start, void *end, float *ms);
/* `bytes` contiguous bytes; kind PP_COPY_*. */
int pp_copy_async(void *dst, const void *src, int64_t bytes, int kind, void *stream);
/* `rows` rows of `width_bytes`, pitches in bytes. */
int pp_copy2d_async(void *dst, int64_t dpitch, const void *src, int64_t spitch,
                    int64_t width_bytes, int64_t rows, int kind, void *stream);
/* All planes of `nframes` w x h frames of `fmt` between two pp_frames layouts
 * (e.g. a dense pinned host batch and a pitched device batch). */
int pp_frames_copy_async(int fmt, int w, int h, const pp_frames *dst,
                         const pp_frames *src, int nframes, int kind, void *stream);

/* ---- p02 byte scanners (host only, no device work) -----------------------
 * Per-frame sizes of a bitstream held in host memory, exactly as
 * lib/get_framesize.py computes them, quirks included (see csrc/scan.cpp).
 * Return the number of frames (sizes[] receives the first `cap` of them) or
 * a negative PP_ERR_*.  pp_annexb_frame_sizes replaces the byte loops of
 * get_framesize_h264 (lib/get_framesize.py:144-201, PP_NAL_H264) and
 * get_framesize_h265 (:204-263, PP_NAL_H265) over the *_tmp.h264/.h265 file;
 * an H.264 NAL header on which the reference raises ValueError (hex digit
 * a..f, :180) returns PP_ERR_INVALID.  pp_ivf_frame_sizes replaces
 * get_framesize_vp9's IVF walk (:87-141); *misdetected counts the frames whose
 * header fails the "10" frame-marker test (the reference prints a line each). */
#define PP_NAL_H264 1
#define PP_NAL_H265 2
int64_t pp_annexb_frame_sizes(const uint8_t *buf, int64_t n, int codec, int64_t *sizes, int64_t cap);
int64_t pp_ivf_frame_sizes(const uint8_t *buf, int64_t n, int64_t *sizes, int64_t cap, int64_t *misdetected);

/* ---- FFV1 AVPVS encoder -----------------------
 * Replaces the `-c:v ffv1 -level 3 -coder 1 -context 1 -slicecrc 1` encode of
 * the AVPVS (lib/ffmpeg.py:993, :1047): FFV1 version 3 (RFC 9043), range
 * coder, slice CRCs, every frame a keyframe, one 3-input quantisation set
 * (63 contexts at 10 bits, 172 at 8), slices_h x slices_v slices per
 * frame (<= 256), one GPU lane per slice.  Bitstream choices and the parity
 * status (unpinned: no FFV1 decoder exists here) are in DESIGN.md.
 * pp_ffv1_encoder_create with ctx == NULL builds the configuration record only.
 * pp_ffv1_extradata copies the configuration record (AVI/MKV codec private
 * data) and returns its size (cap 0: size only).
 * pp_ffv1_encode encodes nframes <= max_frames device frames into frame
 * packets laid out back to back in the device buffer dst (frame_sizes[f] on
 * the host); it synchronises `stream` and returns the total bytes or < 0. */
typedef struct pp_ffv1_enc pp_ffv1_enc;
int pp_ffv1_encoder_create(pp_ctx *ctx, int fmt, int w, int h, int slices_h, int slices_v,
                           int max_frames, pp_ffv1_enc **out);
int pp_ffv1_encoder_destroy(pp_ffv1_enc *enc);
int pp_ffv1_extradata(const pp_ffv1_enc *enc, uint8_t *out, int cap);
int64_t pp_ffv1_encode(pp_ffv1_enc *enc, const pp_frames *src, int nframes, uint8_t *dst,
                       int64_t dst_cap, int64_t *frame_sizes, void *stream);
/* ABI v5.  pp_ffv1_encode_packets: the same encode into the encoder's own
 * device packet buffer (grown as needed, kept across calls); *packets points
 * at the packets back to back, valid until the next encode; returns the total
 * bytes.  The encoder sizes its per-slice renorm records for content coding at
 * 2:1 or better and re-codes a batch in halves when a slice needs more, so
 * the packets never depend on that sizing (pp_ffv1_encode_stats: launches of
 * the last encode, 1 unless it was split).  pp_ffv1_encoder_memory: device
 * bytes the encoder holds. */
int64_t pp_ffv1_encode_packets(pp_ffv1_enc *enc, const pp_frames *src, int nframes, int64_t *frame_sizes,
                               const uint8_t **packets, void *stream);
int pp_ffv1_encode_stats(const pp_ffv1_enc *enc, int *launches);
/* Grow the encoder's packet buffer to `packet_bytes` now (a writer process
 * sizes it once, before its first PVS, instead of inside the first encode). */
int pp_ffv1_encoder_reserve(pp_ffv1_enc *enc, int64_t packet_bytes);
int pp_ffv1_encoder_memory(const pp_ffv1_enc *enc, int64_t *bytes);
/* FFV1 decoder (the CPVS stage reads the AVPVS back, lib/ffmpeg.py:1149):
 * version 3 streams with the range coder (default or transmitted state
 * table), up to 8 quantisation table sets of up to 5 inputs, initial context
 * states, intra or inter frames (a GOP's context states carry from frame to
 * frame), with or without slice CRCs, <= 256 slices, 8/10-bit 4:2:0 / 4:2:2 /
 * 4:4:4 YCbCr -- what pp_ffv1_encode writes and what `ffmpeg -c:v ffv1 -level 3
 * -coder 1 -context 1 -slicecrc 1` writes (RFC 9043).  pp_ffv1_decoder_create
 * parses and checks the configuration record (ctx == NULL: record check
 * only); pp_ffv1_decoder_format gives the PP_FMT_* of the decoded frames;
 * pp_ffv1_decode decodes nframes consecutive packets of the stream held back
 * to back in HOST memory (frame_sizes[f] bytes each) into dst (device),
 * checking every slice's CRC, header and end position; synchronises
 * `stream`.  ABI v6: a decode whose first frame is not a keyframe continues
 * the GOP of the previous successful decode's last frame (its context states
 * are kept); pp_ffv1_decoder_reset forgets them (after a seek), and such a
 * decode then fails. */
typedef struct pp_ffv1_dec pp_ffv1_dec;
int pp_ffv1_decoder_create(pp_ctx *ctx, const uint8_t *extradata, int extradata_size, int w, int h,
                           int max_frames, pp_ffv1_dec **out);
int pp_ffv1_decoder_destroy(pp_ffv1_dec *dec);
int pp_ffv1_decoder_format(const pp_ffv1_dec *dec);
/* The slice grid of the stream (configuration record num_h/v_slices). */
int pp_ffv1_decoder_slices(const pp_ffv1_dec *dec, int *slices_h, int *slices_v);
int pp_ffv1_decode(pp_ffv1_dec *dec, const uint8_t *packets, const int64_t *frame_sizes, int nframes,
                   const pp_frames *dst, void *stream);
/* ABI v6.  The record as parsed: up to n of micro_version, coder_type,
 * quantisation table sets, largest context count, intra, ec, bit mask of the
 * sets with transmitted initial states, 1 if the tables are of pixpath's
 * form (one 3-input set: one threshold quantiser at scales 1, L, L^2 -- what
 * pp_ffv1_encode writes: 63 contexts at 10 bits, 172 at 8; round-4 files: 666),
 * decoded by the one-line-row path; returns the count written. */
int pp_ffv1_decoder_info(const pp_ffv1_dec *dec, int *info, int n);
int pp_ffv1_decoder_reset(pp_ffv1_dec *dec);
int pp_ffv1_decoder_geometry(const pp_ffv1_dec *dec, int *slices_per_workgroup, int *row_cap);
/* ABI v7.  One launch over n streams of ONE configuration record (equal
 * extradata, size and context): decs[k] decodes stream k -- nframes[k]
 * packets back to back in host memory at packets[k], sizes frame_sizes[k] --
 * into dst frames [nframes[0] + ... + nframes[k-1], ...) of the one device
 * batch dst, each stream continuing / keeping its own carried GOP states as
 * pp_ffv1_decode does.  The slice chains of an FFmpeg-made AVPVS are few
 * (GOP 12 at 2x2 slices: 200 per 600 frames, one lane each); several
 * streams' chains side by side are what fill the SIMDs -- the reference's
 * ParallelRunner feeds the CPVS stage several PVSes at once
 * (lib/cmd_utils.py:93-101).  decs[0] holds the launch workspace; the
 * decoders' workspaces grow on demand to what a call needs.  Synchronises
 * `stream`; on a slice error the message names the stream. */
int pp_ffv1_decode_group(pp_ffv1_dec *const *decs, int n, const uint8_t *const *packets,
                         const int64_t *const *frame_sizes, const int *nframes, const pp_frames *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIXPATH_H */
