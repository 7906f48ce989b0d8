/*
 * eae_hip.h -- C ABI of the gfx950 (MI355X / CDNA4) device path (libeae_hip.so).
 *
 * The reference has no native code for the transforms: its hot loops are the TensorFlow kernels that
 * `sess.run(entropy_ae.node_y)` (kodak_tensorflow/eae/batching.py:96-99) and
 * `sess.run(isolated_decoder.node_reconstruction)` (batching.py:49-52) dispatch, plus numpy helpers
 * (kodak_tensorflow/tools/tools.py). Each entry point below replaces one TF op / numpy helper (or a fused run of
 * them) and cites it. All pointers are DEVICE pointers unless named host_*; `stream` is a hipStream_t passed as
 * void* (NULL = default stream). Layout is the reference's: NHWC, C-contiguous, float32 activations.
 * Every function returns 0 on success, a negative EAE_HIP_* code for bad arguments, or a positive hipError_t.
 * Launches are asynchronous on `stream`.
 *
 * NUMERICS CONTRACT (mirrored by oracle/transforms_oracle.c, checked bit-for-bit in tests):
 *  - every dot product is ONE f32 fused-multiply-add chain in a fixed order (conv / transposed conv: input channels in
 *    blocks of 32 (outer), then the taps row-major, then the channel inside the block; GDN: channel ascending),
 *    started from +0, bias/beta added afterwards -- this is what v_mfma_f32_32x32x2_f32 / 16x16x4_f32 compute
 *    (exact f32 FMA chain, k ascending);
 *  - division, sqrt are correctly rounded; rounding to integer is round-half-to-even (numpy.round).
 */
#ifndef EAE_HIP_H
#define EAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    EAE_HIP_OK = 0,
    EAE_HIP_BAD_ARGUMENT = -1,  /* NULL pointer, non-positive size */
    EAE_HIP_BAD_SHAPE = -2      /* spatial size not accepted by the op (see each op) */
};

enum { EAE_NORM_NONE = 0, EAE_NORM_GDN = 1, EAE_NORM_IGDN = 2 };

#define EAE_NB_MAPS 128 /* eae/graph/constants.py:42-44 (NB_MAPS_1/2/3) */

const char* eae_hip_version(void);
/* Fills name (e.g. "gfx950:sramecc+:xnack-"), CU count; returns 0, or a hipError_t when no device is usable. */
int eae_hip_device_info(char* name, int name_cap, int* compute_units, int* clock_mhz, int64_t* hbm_bytes);
/* The compute partition the current logical device is, as far as it matters here: its compute units, the XCDs that makes on
 * gfx950 (32 CUs each; 0 on another architecture), and whether it is one whole MI355X (256 CUs, mode SPX) -- the shape the
 * conv launches' XCD-aware tile order and the sizing of their cut tiles are built on. On a partition (DPX / QPX / CPX) every
 * result is the same, the launches keep whole tiles, and a note goes to stderr once. */
int eae_hip_partition_info(int* compute_units, int* xcds, int* whole_device);

/* Small results for the host (bit counts, statuses, histograms): a kernel copies `bytes` (multiple of 4) from device
 * memory into PINNED, device-mapped host memory (hipHostMalloc / torch pin_memory) in stream order; the host reads them
 * after synchronising an event recorded behind it. Unlike hipMemcpyAsync this never blocks the calling thread. */
int eae_hip_publish_to_host(const void* src_device, void* dst_host_mapped, uint64_t bytes, void* stream);
/* A step counter for a host thread: in stream order, *counter_device (uint32, device memory) is incremented and the new value is
 * left in *word_host_mapped (uint32, pinned host memory), behind everything the stream did before -- in particular behind an
 * eae_hip_publish_to_host in front of it. The host, which knows how many times it submitted the step, waits for that value with
 * plain loads: no event to record, query or wait on (capturable into a hipGraph: every replay bumps the counter). */
int eae_hip_publish_sequence(void* counter_device, void* word_host_mapped, void* stream);
/* The end of one side of a step in ONE launch (what codec.BatchCodec enqueues behind a batch's coder and behind its synthesis
 * transform; each launch costs the submitting thread ~10 us): in stream order, (1) when `conv_workspace` is given, what
 * eae_hip_conv_workspace_collect does with it and `error_word` (which must lie inside the source block: it is copied in (2); the block
 * is then at most 256 KB); (2) eae_hip_publish_to_host of `bytes` from `src_device`; (3) the source's bytes from `clear_from_byte` on are
 * zeroed -- the accumulators of the next step that uses the block (pass `bytes` to clear nothing); (4) eae_hip_publish_sequence on
 * `counter_device` / `word_host_mapped`, behind the copy. `tickets_device`: a zeroed uint32 in device memory, left zeroed (the copying
 * blocks count themselves in; steps that may run concurrently need their own). */
int eae_hip_publish_step(void* src_device, void* dst_host_mapped, uint64_t bytes, uint64_t clear_from_byte, void* conv_workspace,
                         uint32_t* error_word, void* tickets_device, void* counter_device, void* word_host_mapped, void* stream);

/* ---- whole-path entry points (csrc/hip/model.hip) --------------------------------------------------------------------
 * What `sess.run(entropy_ae.node_y, feed_dict={node_visible_units: batch})` (eae/batching.py:96-99) and
 * `sess.run(isolated_decoder.node_reconstruction, feed_dict={node_quantized_y: batch})` followed by `tls.cast_bt601`
 * (batching.py:49-53) are to the reference: one model object per trained entropy autoencoder, one call per mini-batch.
 * The numpy steps the reference runs between the two (centring, quantiser, statistics: reconstructing_eae_kodak.py:170-192)
 * are eae_hip_latent_stage / eae_hip_quantize_maps below; the per-layer ops that encode / decode chain follow further down.
 *
 * eae_hip_variables: HOST pointers to the variables of `EntropyAutoencoder` / `IsolatedDecoder` in TensorFlow's layouts, as a
 * checkpoint holds them (float32, C-contiguous): weights_1 [9][9][1][128], weights_2/3 [5][5][128 in][128 out],
 * weights_4/5 [5][5][128 out][128 in], weights_6 [9][9][1][128], gamma_i [128][128], biases_i / beta_i [128].
 * gamma_3, beta_3, gamma_4, beta_4 exist only in the fixed-bin-width model (components.py:137-142, 53-58): NULL when
 * are_bin_widths_learned != 0. Either side may be left out entirely (all its pointers NULL): an encoder-only model for
 * eae_hip_encode, a decoder-only one (the reference's IsolatedDecoder, IsolatedDecoder.py:21-129) for eae_hip_decode; a side
 * that is given must be complete, else EAE_HIP_BAD_ARGUMENT.
 * eae_hip_model_create uploads and re-lays them out on the current device (7 MB resident) and returns when that is done.
 * eae_hip_encode:  images uint8 [n][h][w] (device, 4-byte aligned) -> latents f32 [n][h/16][w/16][128] (device). h, w
 *                  multiples of 16.
 * eae_hip_decode:  quantised latents f32 [n][h_latent][w_latent][128] (after the de-centring of
 *   reconstructing_eae_kodak.py:192) -> out_f32 [n][16 h_latent][16 w_latent] (nullable: the float reconstruction),
 *   out_u8 (nullable: its BT.601 cast), and with ref_u8 + sse the squared error per image as in eae_hip_tconv9x9s4_luma.
 * scratch: device memory of eae_hip_{encode,decode}_scratch_bytes(...) bytes for the activations between the layers;
 * contents need not survive between calls, calls that may overlap (different streams) need different blocks. Everything is
 * asynchronous on `stream`; results are bit-identical to the per-layer entry points and to oracle/transforms_oracle.c. */
typedef struct eae_hip_model eae_hip_model;
typedef struct eae_hip_variables {
    const float *weights_1, *biases_1, *gamma_1, *beta_1;
    const float *weights_2, *biases_2, *gamma_2, *beta_2;
    const float *weights_3, *biases_3, *gamma_3, *beta_3;
    const float *gamma_4, *beta_4;
    const float *weights_4, *biases_4, *gamma_5, *beta_5;
    const float *weights_5, *biases_5, *gamma_6, *beta_6;
    const float *weights_6;
} eae_hip_variables;
int eae_hip_model_create(const eae_hip_variables* host_variables, int are_bin_widths_learned, eae_hip_model** model);
void eae_hip_model_destroy(eae_hip_model* model);
int eae_hip_model_are_bin_widths_learned(const eae_hip_model* model);
uint64_t eae_hip_encode_scratch_bytes(int n, int h, int w);                 /* 0 for sizes eae_hip_encode rejects */
uint64_t eae_hip_decode_scratch_bytes(int n, int h_latent, int w_latent);
/* eae_hip_transform_status: the failure word of the MOST RECENT encode / decode call issued on `stream` with this scratch
 * block (the hand-off timeout of a cut launch, see eae_hip_conv_workspace_collect). Waits for `stream`, writes the count to
 * *host_count (0 = the results are valid) and returns 0, or a hipError_t. Not calling it forgoes the check; it never
 * affects later calls (encode / decode zero their workspace and the word on entry). */
int eae_hip_transform_status(void* scratch, uint32_t* host_count, void* stream);
int eae_hip_encode(const eae_hip_model* model, const uint8_t* images, int n, int h, int w, float* latents, void* scratch,
                   uint64_t scratch_bytes, void* stream);
int eae_hip_decode(const eae_hip_model* model, const float* quantized_latents, int n, int h_latent, int w_latent,
                   float* out_f32, uint8_t* out_u8, const uint8_t* ref_u8, uint64_t* sse, void* scratch,
                   uint64_t scratch_bytes, void* stream);

/* ---- tiled encode / decode (csrc/hip/tile.hip) -------------------------------------------------
 * An image of any size goes through eae_hip_encode / eae_hip_decode as a batch of equally shaped windows; each window keeps only
 * its interior, the part whose receptive field it holds, so the stitched result is bit-identical to the untiled one. The plan
 * (pipeline.tile_plan) is int32 [n_windows][EAE_TILE_PLAN_COLS], all coordinates in latents: image, window origin (row, col),
 * interior origin in the window (row, col), interior origin in the image (row, col), interior extent (rows, cols). `plan` is the
 * device copy the kernel reads, `host_plan` the same rows in host memory, which the argument checks read before any launch.
 * Both functions: NULL pointer or a non-positive size -> EAE_HIP_BAD_ARGUMENT; a window larger than the plane, a row of a latent
 * (unit * elem_bytes) that is not a multiple of 16 bytes, a base pointer not aligned to 16 bytes, or a plan row outside the plane
 * or its window (or whose two interior origins disagree) -> EAE_HIP_BAD_SHAPE; nothing is launched then. The full plane is
 * addressed with 64-bit offsets (no size limit); a window's bytes / 16 stay below 2^31, n_windows <= 65535. One launch per call.
 * tile_copy: plane [n][h * unit][w * unit][elem_bytes] and windows [n_windows][window_h * unit][window_w * unit][elem_bytes];
 *   to_windows != 0 copies every whole window out of the plane (gather), to_windows == 0 copies every interior into it (stitch).
 *   uint8 images: unit 16, elem 1; latents: unit 1, elem 512; float reconstruction: unit 16, elem 4.
 * tile_stitch_u8: uint8 reconstruction windows (unit 16) -> their interiors into image [n][16 h][16 w] (nullable) and, with ref_u8
 *   (same shape as image), sse[i] += the exact squared error over the interior pixels of image i (caller zeroes; eae_hip_decode's
 *   own sse would count the halos). At least one of image and ref_u8. */
#define EAE_TILE_PLAN_COLS 9
int eae_hip_tile_copy(void* plane, int n, int h, int w, void* windows, int window_h, int window_w, int unit, int elem_bytes,
                      const int32_t* plan, const int32_t* host_plan, int n_windows, int to_windows, void* stream);
int eae_hip_tile_stitch_u8(const uint8_t* windows, int window_h, int window_w, uint8_t* image, const uint8_t* ref_u8, uint64_t* sse,
                           int n, int h, int w, const int32_t* plan, const int32_t* host_plan, int n_windows, void* stream);

/* ---- coding tiles of the tile-indexed container EAT1 (csrc/hip/tile_symbols.hip; container.py) -----------
 * The coder reads each map as one contiguous run. These two move the symbols of a group of coding tiles between the planar layout
 * and the tile-major layout of the coder. The plan is int64 [n_tiles][EAE_TILE_SYMBOLS_PLAN_COLS]: image, tile origin (row, col),
 * tile extent (rows, cols), element offset of the tile's map 0 in `tiles`; map m of the tile is the run of rows * cols symbols at
 * offset + m * rows * cols, in raster order. One plan may mix tiles of several shapes. `plan` is the device copy the kernel reads,
 * `host_plan` the same rows in host memory, which the argument checks read before any launch. NULL pointer or a non-positive size
 * -> EAE_HIP_BAD_ARGUMENT; a malformed row, a run outside `tiles` (tile_elems int16), a tile of 2^31 pixels or more, or more than
 * 65535 tiles -> EAE_HIP_BAD_SHAPE; nothing is launched then. Planes are addressed with 64-bit offsets. One launch per call.
 * tile_symbols_gather: symbols_planar [n][128][h * w] int16 (eae_hip_quantize_maps) -> `tiles`. Every tile lies inside the h x w plane.
 * tile_symbols_dequantize: `tiles` -> shifted_out f32 [n][hs][ws][128] = bin_widths[c] * symbol + map_mean[c] (map_mean nullable),
 *   the arithmetic of eae_hip_dequantize_maps, bit for bit. Image and origin are in the hs x ws output; the origin may be negative
 *   and a tile may reach past the output: only its pixels inside are written. shifted_out aligned to 16 bytes.
 * tile_symbols_dequantize_rows: tile_symbols_dequantize with one row of bin widths and one row of means (nullable) per image of the
 *   output, f32 [n][128] each: a tile is dequantised with the rows of its plan row's image, bin_widths_rows[image][c] * symbol +
 *   map_mean_rows[image][c]. Same plan, same checks, same limits, same arithmetic: the output equals, bit for bit, that of
 *   tile_symbols_dequantize called image by image with that image's rows (codec.BatchDecoder(coding_tile=...), whose step holds
 *   images of several blobs).
 * tile_symbols_dequantize_placed: tile_symbols_dequantize_rows for a step whose SHAPE is static and whose PLACEMENT changes with
 *   every step (codec.RegionDecoder). The static half of a plan row lives in `slots`, int64
 *   [n_slots][EAE_TILE_SYMBOLS_SLOT_COLS]: extent (rows, cols) and element offset of the slot's map 0 in `tiles`; `host_slots` is
 *   its host copy, checked before the launch as a plan row's extent and offset are (a run outside `tiles`, a tile of 2^31 pixels
 *   or more, more than 65535 slots -> EAE_HIP_BAD_SHAPE). The per-step half lives in `placement`, int32 [n_slots][4] in DEVICE
 *   memory, read by the kernel only: image, origin row, origin col in the hs x ws output, one unused word. Whatever those words
 *   hold, nothing outside the buffers is touched: a slot whose image is outside [0, n) is skipped, origins are arbitrary and only
 *   the pixels inside hs x ws are written. Same arithmetic: the output equals, bit for bit, tile_symbols_dequantize_rows with the
 *   plan rows (image, origin, extent, offset) put together. shifted_out aligned to 16 bytes, placement to 4. */
#define EAE_TILE_SYMBOLS_PLAN_COLS 6
#define EAE_TILE_SYMBOLS_SLOT_COLS 3
int eae_hip_tile_symbols_gather(const int16_t* symbols_planar, int n, int h, int w, int16_t* tiles, int64_t tile_elems,
                                const int64_t* plan, const int64_t* host_plan, int n_tiles, void* stream);
int eae_hip_tile_symbols_dequantize(const int16_t* tiles, int64_t tile_elems, const int64_t* plan, const int64_t* host_plan, int n_tiles,
                                    const float* bin_widths, const float* map_mean, float* shifted_out, int n, int hs, int ws,
                                    void* stream);
int eae_hip_tile_symbols_dequantize_rows(const int16_t* tiles, int64_t tile_elems, const int64_t* plan, const int64_t* host_plan,
                                         int n_tiles, const float* bin_widths_rows, const float* map_mean_rows, float* shifted_out, int n,
                                         int hs, int ws, void* stream);
int eae_hip_tile_symbols_dequantize_placed(const int16_t* tiles, int64_t tile_elems, const int64_t* slots, const int64_t* host_slots,
                                           int n_slots, const int32_t* placement, const float* bin_widths_rows,
                                           const float* map_mean_rows, float* shifted_out, int n, int hs, int ws, void* stream);

/* ---- analysis transform (eae/graph/components.py:86-142) ---------------------------------------------------------*/

/* conv_1 + bias_add + gdn_1  (components.py:119-125; tf.nn.conv2d 9x9, 1->128, stride 4, 'SAME' = pad 2/3;
 * tfutils.py:393-397). x: uint8 [N][H][W] (the uint8->float32 cast of batching.py:95 is done in-kernel, no offset,
 * no scale); w_packed: [82][128] from eae_hip_pack_conv9x9s4_weights; out: f32 [N][H/4][W/4][128]. H, W multiples
 * of 4, x aligned to 4 bytes (the kernel reads whole 32-bit words; EAE_HIP_BAD_ARGUMENT otherwise). gamma_packed: from
 * eae_hip_pack_gamma; NULL skips the normalisation (plain conv + bias). */
int eae_hip_conv9x9s4_u8(const uint8_t* x, const float* w_packed, const float* bias, const float* gamma_packed,
                         const float* beta, float* out, int n, int h, int w_in, void* stream);

/* conv_2 / conv_3 + bias_add (+ gdn_2 / gdn_3)  (components.py:126-142; tf.nn.conv2d 5x5, 128->128, stride 2,
 * 'SAME' = pad 1/2). x: f32 [N][H][W][128]; w_packed: from eae_hip_pack_conv_weights (HWIO [5][5][128][128] with the
 * output channels in packed order); out: [N][H/2][W/2][128]. H, W even, and H * W * 512 bytes (one image's input plane; the
 * kernels address inside an image with 32-bit byte offsets) below 2 GB: EAE_HIP_BAD_SHAPE otherwise. For the untiled whole path
 * that is an image of at most 67 megapixels (conv_2's input is the 1/16-size plane: 8192 x 8176 passes, 8192 x 8192 does not);
 * the tiled path (eae_hip_tile_copy above) is bounded by the window, not the image.
 * norm: EAE_NORM_NONE (learned-bin-width model, components.py:137-138) or EAE_NORM_GDN (gamma_packed, beta). */
int eae_hip_conv5x5s2(const float* x, const float* w_packed, const float* bias, int norm, const float* gamma_packed,
                      const float* beta, float* out, int n, int h, int w_in, void* stream);

/* GDN / IGDN on its own (tfutils.py:363-397 / 480-509): out[r][c] = x[r][c] (/ or *) sqrt(beta[c] + sum_k x[r][k]^2
 * gamma[k][c]); x, out: [rows][128]; gamma_packed from eae_hip_pack_gamma. Used for inverse_gdn #4
 * (components.py:53-58) and as a standalone op. */
int eae_hip_gdn(const float* x, const float* gamma_packed, const float* beta, int inverse, float* out, int64_t rows,
                void* stream);

/* ---- synthesis transform (components.py:11-84) --------------------------------------------------------------------*/

/* transpose_conv_1 / _2 + bias_add + inverse_gdn of the next layer (components.py:63-78; tf.nn.conv2d_transpose 5x5,
 * 128->128, stride 2, 'SAME'). x: [N][h][w][128]; w_packed: from eae_hip_pack_tconv_weights (the TF filter
 * [5][5][out][in] as [25][in][packed out]); out: [N][2h][2w][128] (one image's output plane below 2 GB, as above). */
int eae_hip_tconv5x5s2(const float* x, const float* w_packed, const float* bias, int norm, const float* gamma_packed,
                       const float* beta, float* out, int n, int h, int w_in, void* stream);

/* The same two ops with a workspace that lets the launch cut its last tiles (csrc/hip/conv_gemm_split.hip): identical
 * results, no partly empty last round. A batch gives every SIMD a non-integer number of 32-position tiles (4.5 for conv_2
 * and 1.1 for conv_3 on 24 Kodak images); with the workspace the last tiles of the launch are interrupted at a K-step
 * boundary -- the accumulators parked in the tile's own output pixels -- and finished by a wave dispatched at the very end,
 * so that every SIMD runs dry at the same time. The per-element f32 FMA chain, hence every bit of the result, is the one
 * documented above. workspace: eae_hip_conv_workspace_bytes() bytes of device memory, ALL ZERO on entry and all zero again
 * when the launch has completed (zero it once); launches that may run concurrently need their own. Whether a launch is cut
 * is decided from its shape (only the convolutions, only when the last round would be less than ~97 % full). */
uint64_t eae_hip_conv_workspace_bytes(void);
/* Failure mode of a cut launch, and how it surfaces. The second half of a cut tile waits for the first half's accumulators;
 * the first half is always dispatched earlier (workgroups start in grid order on gfx950, the only device on which launches
 * are cut), so the wait is finite. Should it ever exceed ~1 s, the waiting wave writes NO result for its tile and counts
 * itself in the workspace's error word. eae_hip_conv_workspace_collect, enqueued behind the launch(es), adds that count to
 * *error_word (device memory or device-mapped pinned host memory; non-zero = the outputs of the launches since the last
 * collect are INVALID) and restores the all-zero workspace, so later launches are unaffected. A caller that cuts launches
 * must collect before trusting their outputs (codec.BatchCodec does per batch and raises from Ticket.result()). */
int eae_hip_conv_workspace_collect(void* workspace, uint32_t* error_word, void* stream);
int eae_hip_conv5x5s2_ws(const float* x, const float* w_packed, const float* bias, int norm, const float* gamma_packed,
                         const float* beta, float* out, int n, int h, int w_in, void* workspace, void* stream);
int eae_hip_tconv5x5s2_ws(const float* x, const float* w_packed, const float* bias, int norm, const float* gamma_packed,
                          const float* beta, float* out, int n, int h, int w_in, void* workspace, void* stream);

/* transpose_conv_3 (components.py:79-83; 9x9, 128->1, stride 4, 'SAME', no bias) fused with what follows it on the
 * path: tls.cast_bt601 (tools.py:93: uint8(round_half_even(clip(x,16,235)))) and the squared error of tls.psnr_2d
 * (tools.py:873-875). x: [N][h][w][128]; w_phase: 18432 floats from eae_hip_pack_tconv9x9s4_weights;
 * out_f32 (nullable): [N][4h][4w] float reconstruction; out_u8 (nullable): [N][4h][4w] BT.601 cast;
 * ref_u8 + sse (both nullable): sse[i] += sum over image i of (ref - out_u8)^2, exact uint64 (caller zeroes). */
int eae_hip_tconv9x9s4_luma(const float* x, const float* w_phase, float* out_f32, uint8_t* out_u8,
                            const uint8_t* ref_u8, uint64_t* sse, int n, int h, int w_in, void* stream);

/* The same launch with the squared error over the REAL pixels of padded planes: the contraction, the tiling,
 * the persistent grid and the BT.601 cast are eae_hip_tconv9x9s4_luma's, and out_f32 / out_u8, where requested, are written over the
 * whole coded plane [N][4h][4w]. ref_u8 is the CODED frame, rows of 4 w_in bytes (what eae_hip_frame_pad_u8 writes);
 * sse[i] += the sum over y < real_h and x < real_w only, exact uint64, masked per pixel: real_w is any value in [1, 4 w_in]. Bytes
 * of ref_u8 outside the rectangle may be loaded -- they lie inside the buffer -- and never reach the sum. At real_h = 4 h,
 * real_w = 4 w_in it adds what eae_hip_tconv9x9s4_luma adds. Refused (EAE_HIP_BAD_ARGUMENT) beyond what that entry point
 * refuses: real_h or real_w below 1 or outside the coded plane. */
int eae_hip_tconv9x9s4_luma_frame(const float* x, const float* w_phase, float* out_f32, uint8_t* out_u8,
                                  const uint8_t* ref_u8, uint64_t* sse, int n, int h, int w_in, int real_h, int real_w,
                                  void* stream);

/* TF filter [9][9][1][128] -> per-lane MFMA fragments [4 channel blocks][9 neighbours][64 lanes][8] (zeros where an
 * output phase has no tap). */
int eae_hip_pack_tconv9x9s4_weights(const float* w_tf, float* w_phase, void* stream);

/* Kernel-side layouts, packed once per model on the device. "Packed" channel order: out channel c sits at position
 * (c % 32) * 4 + c / 32 of its row, so that the 4 values one lane needs for its 4 column tiles are one 16-byte load.
 *   eae_hip_pack_conv_weights : HWIO [taps][128 in][128 out]            -> [taps][128 in][packed out]   (conv_2, conv_3)
 *   eae_hip_pack_tconv_weights: TF conv2d_transpose [taps][128 out][128 in] -> [taps][128 in][packed out] (tconv_1, _2)
 *   eae_hip_pack_gamma        : gamma [128 k][128 c]                     -> [128 k][packed c]            (every GDN / IGDN) */
int eae_hip_pack_conv_weights(const float* w_hwio, float* w_packed, int taps, void* stream);
/* conv_1 filter [9][9][1][128] -> [82 taps (81 + one zero row)][packed out] */
int eae_hip_pack_conv9x9s4_weights(const float* w_tf, float* w_packed, void* stream);
int eae_hip_pack_tconv_weights(const float* w_tf, float* w_packed, int taps, void* stream);
int eae_hip_pack_gamma(const float* gamma, float* gamma_packed, void* stream);

/* ---- quantiser, symbols, per-map statistics ------------------------------------------------------------------------
 * One pass over the latents y: [N][h*w][C] f32, C = 128. For every element, with m = map_mean[c] (NULL = 0) and
 * bw = bin_widths[c]:
 *   centered  = y - m                                   (reconstructing_eae_kodak.py:178)
 *   r         = round_half_even(centered / bw)          (tools.py:929)
 *   cq        = bw * r                                  (tools.py:929, `quantize_per_map`)
 *   symbol    = int16(round_half_even(cq / bw))         (lossless/compression.py:142, tools.py:126-133)
 *   shifted   = cq + m                                  (reconstructing_eae_kodak.py:192)
 * Outputs (each nullable):
 *   cq_out, shifted_out : f32 [N][h*w][C]
 *   symbols_planar      : int16 [N][C][h*w]  -- map-major: map (i, c) is `ref_int16[:, :, c].flatten()` of
 *                         compression.py:77 for image i; this is the buffer the single device->host copy moves
 *   nonzero_flags       : uint32 [N][C], set to 1 when some cq of the map is != 0 (so `count_nb_deads`,
 *                         tools.py:318-320, is the number of zero flags); caller zeroes
 *   checks              : uint32 [3], caller zeroes; each += a count of offending elements:
 *       [0] |round(cq/bw)| >= 32768                      -> AssertionError of tools.py:130-132
 *       [1] |bw*round(x/bw) - x| >= 1.5e-10, x = y - m   -> AssertionError "The quantization was omitted."
 *                                                           (tools.py:372-375) when y is passed as already quantised
 *       [2] float(symbol)*bw != x                        -> AssertionError of lossless/compression.py:149-153
 * c = number of maps (last axis). c == 128 takes the tiled kernel; any other c a generic one (same arithmetic). */
int eae_hip_quantize_maps(const float* y, const float* map_mean, const float* bin_widths,
                          float* cq_out, float* shifted_out, int16_t* symbols_planar,
                          uint32_t* nonzero_flags, uint32_t* checks, int n, int hw, int c, void* stream);

/* The whole latent stage of the fixed-bin-width model in one pass (csrc/hip/latent.hip): x = conv_3 + bias (NORM_NONE)
 *   -> gdn_3 (gamma_in_packed/beta_in; both NULL = no normalisation, the learned-bin-width model, components.py:137-138)
 *   -> the quantiser exactly as eae_hip_quantize_maps (symbols_planar, nonzero_flags, checks: same meaning, caller zeroes
 *      flags and checks; map_mean nullable)
 *   -> + map_mean -> inverse_gdn_4 (gamma_out_packed/beta_out; both NULL = none) into t_out, the input of transpose_conv_1.
 * y_out (the latents after gdn_3), shifted_out (quantised + mean) are optional f32 [N][hw][128] outputs.
 * Same arithmetic as eae_hip_gdn + eae_hip_quantize_maps + eae_hip_gdn: identical bits (tests/test_gpu_latent.py). */
int eae_hip_latent_stage(const float* x, const float* gamma_in_packed, const float* beta_in, const float* map_mean,
                         const float* bin_widths, const float* gamma_out_packed, const float* beta_out, float* y_out,
                         float* shifted_out, float* t_out, int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks,
                         int n, int hw, void* stream);

/* conv_3 + bias_add with the latent stage behind it in one launch: the convolution's register tile goes straight through
 * gdn_3 -> quantiser -> inverse_gdn_4 (eae_hip_latent_stage's arithmetic, same bits) instead of through HBM and a second
 * kernel -- what `codec.BatchCodec` launches between conv_2 and transpose_conv_1. x: gdn_2 output [N][h][w][128]; w_packed /
 * bias: conv_3; gamma_in/beta_in (gdn_3) and gamma_out/beta_out (inverse_gdn_4): both pairs (fixed-bin-width model) or
 * neither (learned: the quantiser only); outputs as eae_hip_latent_stage ([N][h/2 * w/2][128] f32, planar int16 symbols,
 * flags and checks zeroed by the caller); t_out (fixed) / shifted_out (learned) is required: it is the synthesis transform's
 * input. workspace: as eae_hip_conv5x5s2_ws (nullable: then the launch is never cut). Layers too small for the fused kernel
 * run as the convolution followed by eae_hip_latent_stage in place. */
int eae_hip_conv5x5s2_latent(const float* x, const float* w_packed, const float* bias, const float* gamma_in_packed,
                             const float* beta_in, const float* map_mean, const float* bin_widths, const float* gamma_out_packed,
                             const float* beta_out, float* y_out, float* shifted_out, float* t_out, int16_t* symbols_planar,
                             uint32_t* nonzero_flags, uint32_t* checks, int n, int h, int w_in, void* workspace, void* stream);

/* The map means of lossless/stats.py:306, `numpy.mean(y_float32, axis=(0, 1, 2))`, bit for bit: means[c] = (the float32
 * sum of y[row][c] accumulated row by row, rows ascending) / float32(rows) -- the order numpy reduces the leading axes of a
 * C-contiguous float32 array in (tests/test_host_logic.py pins that order against numpy itself). y: [rows][c] f32. */
int eae_hip_map_means(const float* y, float* means, int64_t rows, int c, void* stream);

/* The two device passes of lossless/stats.py:197-241 (find_index_map_exception), whose per-map loop calls
 * compute_probabilities_intervals(map, 1.) (stats.py:70-134): numpy.amin / amax per map, then a histogram over the
 * unit-width intervals [floor(min), ceil(max)].
 *   map_minmax: minmax[0][c] = min, minmax[1][c] = max over rows of y[row][c] (both NaN when the map holds a NaN, like
 *   numpy); scratch_keys: 2*c uint32 of scratch.
 *   floor_histograms: hist[c][floor(y) + radius] += 1 for |floor(y)| <= radius, else overflow[c] += 1 (caller zeroes both;
 *   hist is [c][2*radius+1]). The closed last interval of numpy.histogram (values equal to the right edge) is folded in
 *   by the host, which also forms the probabilities and the Jensen-Shannon divergences in float64 like the reference. */
int eae_hip_map_minmax(const float* y, float* minmax, uint32_t* scratch_keys, int64_t rows, int c, void* stream);
int eae_hip_floor_histograms(const float* y, uint32_t* hist, int radius, uint32_t* overflow, int64_t rows, int c, void* stream);

/* tls.count_nb_deads (tools.py:294-320) for an arbitrary stack x [N][hw][C]: nonzero_flags[n][c] = 1 when some
 * element of map (n, c) is != 0 (caller zeroes); the number of dead maps of image n is the number of zero flags. */
int eae_hip_nonzero_flags(const float* x, uint32_t* nonzero_flags, int n, int hw, int c, void* stream);

/* tls.cast_float_to_int16 (tools.py:95-133): out = int16(round_half_even(x)); *range_error += number of elements
 * with |round(x)| >= 32768 (the reference raises AssertionError); caller zeroes. */
int eae_hip_cast_int16(const float* x, int16_t* out, int64_t count, uint32_t* range_error, void* stream);

/* Per-map symbol histograms (tls.count_symbols, tools.py:376-388, is this histogram restricted to [min, max]; it feeds
 * discrete_entropy :523-537, rate_3d :977-989 and stats.count_binary_decisions, lossless/stats.py:179-195).
 * symbols_planar: int16 [n_maps][map_size]; hist: uint32 [n_maps][2*hist_radius+1], bin = symbol + hist_radius;
 * symbols outside the radius are counted in overflow[n_maps] instead (re-run with a larger radius; 32768 covers
 * int16). hist and overflow are ACCUMULATED into: the caller zeroes them. */
int eae_hip_symbol_histograms(const int16_t* symbols_planar, uint32_t* hist, int hist_radius, uint32_t* overflow,
                              int n_maps, int map_size, void* stream);
/* Same over every map_step-th map starting at first_map (row i of hist = map first_map + i * map_step): the exception
 * map of every image of a batch (first_map = idx_map_exception, map_step = 128) without gathering it first. */
int eae_hip_symbol_histograms_strided(const int16_t* symbols_planar, uint32_t* hist, int hist_radius, uint32_t* overflow,
                                      int n_maps, int map_size, int64_t first_map, int64_t map_step, void* stream);

/* ---- rate ladder (csrc/hip/ladder.hip; ratecontrol.py) ------------------------------------------------
 * One pass over the latents y [N][hw][128] for the K rate points of a ladder (the reference walks nine, `multipliers`, and
 * quantises, counts and codes once per point: lossless/stats.py:314-320, reconstructing_eae_kodak.py). For every element and every
 * point k the symbol is eae_hip_quantize_maps' with bw = bin_widths_points[k][c] and m = map_mean[c] (NULL = 0), the same float32
 * expressions in the same order:  rs = round_half_even(bw * round_half_even((y - m) / bw) / bw).  Then
 *   hist[i][k][c][min(|rs|, L)] += 1                      uint32 [N][K][128][L + 1]: the clipped histogram the binary decisions of
 *                                                         stats.py:181-195 are counted from
 *   bypass_bits[i][k][c] += (rs != 0) + (|rs| >= L ? 2 * floor(log2(|rs| - L + 1)) + 1 : 0)       uint64 [N][K][128], nullable:
 *                                                         the exact length of the map's bypass stream (LosslessCoder.cpp:22-37,
 *                                                         58-111, 232-252: sign bits and Exp-Golomb suffixes)
 *   an element with !(|rs| < 32768) (NaN included) goes into no bin and no bit count: range_errors[k] += 1 (uint32 [K], nullable),
 *                                                         the AssertionError of tools.py:130-132 at that point
 * All three are ACCUMULATED into: the caller zeroes them. L = length, 1..255; k_points 1..eae_hip_ladder_max_points(length), the most
 * rate points one launch takes at this L (its block keeps (L + 3) * 512 bytes of LDS per point: 9 at L = 10) and 0 when not even
 * one fits or L is out of range. Those, NULL y / bin_widths_points / hist and non-positive n / hw -> EAE_HIP_BAD_ARGUMENT (a grid
 * of 2^31 blocks or more, n * hw / 64 at the most: EAE_HIP_BAD_SHAPE). One launch; bin widths are not checked (a zero or negative width gives the symbols the quantiser would give). */
int eae_hip_ladder_histograms(const float* y, const float* map_mean, const float* bin_widths_points, int k_points, int length,
                              uint32_t* hist, uint64_t* bypass_bits, uint32_t* range_errors, int n, int hw, void* stream);
int eae_hip_ladder_max_points(int length);
/* The same counts per coding tile: y [N][h * w][128] is a plane of h x w latents per image, the tile th x tw
 * latents, clamped to the plane; T = ceil(h / th) * ceil(w / tw) tiles, row-major, edge tiles smaller (container.coding_tile_grid).
 *   hist uint32 [N][K][T][128][L + 1], bypass_bits uint64 [N][K][T][128] (nullable), range_errors uint32 [K] (nullable)
 * Symbols, bins, bits and range errors are eae_hip_ladder_histograms'; all three are ACCUMULATED into, and summed over T they are that
 * function's outputs on the same input. k_points and length as there. NULL y / bin_widths_points / hist, non-positive n, h, w, th or
 * tw -> EAE_HIP_BAD_ARGUMENT; h * w >= 2^30, or n * T times the chunks a tile is cut into (tile pixels / 64 at the most) >= 2^31 ->
 * EAE_HIP_BAD_SHAPE. One launch, at most two blocks per compute unit. */
int eae_hip_ladder_histograms_tiles(const float* y, const float* map_mean, const float* bin_widths_points, int k_points, int length,
                                    uint32_t* hist, uint64_t* bypass_bits, uint32_t* range_errors, int n, int h, int w, int th, int tw,
                                    void* stream);

/* ---- a rate point per image, on the device (csrc/hip/budget.hip, latent_rows.hip; ratecontrol.py) -------
 * eae_hip_ladder_select: the point of every image of a batch for its byte budget, from what eae_hip_ladder_histograms left. Integer
 * arithmetic only; equal, element for element, to ratecontrol.upper_bounds_fixed + valid_points + select_by_upper_bound.
 *   hist uint32 [N][K][128][L + 1], bypass_bits uint64 [N][K][128]           as eae_hip_ladder_histograms leaves them
 *   fixed_costs uint32 [K][128][L][2]   ratecontrol.fixed_costs: ceil(-log2(p) 2^20), ceil(-log2(1 - p) 2^20)
 *   log2_tables uint32 [2][map_size + 1]  ratecontrol.log2_tables: ceil / floor of log2(n) 2^20; NULL without an exception map
 *   idx_map_exception: the map costed with the row of its own counts (negative: none); header_bytes: ratecontrol.header_bytes;
 *   map_size: symbols per map (point k of image i is VALID when its histograms hold all 128 * map_size of them);
 *   budgets int64 [N], in device memory; exception_row_base: the coder's table row of image 0's exception map.
 * Per (image, point, map): fp = sum_i zeros[i] c0[i] + ones[i] c1[i] in 64 bits (exception map: t Lceil[t] - z Lfloor[z] -
 * o Lfloor[o], o C99 / z C99 when z / o is 0, 0 when t is 0; counts beyond map_size are clamped as table indices);
 * bytes = (((fp + 2^20 - 1) >> 20) + 3 + 7) / 8 + (bypass + 7) / 8. Every element of every output is written by every call:
 *   upper int64 [N][K]     header_bytes + the bytes of the 128 maps
 *   point int32 [N]        the first valid point with upper <= budget; else the last valid point; else K - 1
 *   flags uint32 [N]       bit 0: promised (a valid point fitted); bit 1: no valid point
 *   prob_row int32 [N][128]  point * 128 + m; exception_row_base + i for the exception map
 * L 1..255, k_points 1..eae_hip_ladder_max_points(L), map_size 1..2^24 (beyond: EAE_HIP_BAD_SHAPE). A NULL among the required
 * pointers, idx_map_exception >= 128 or >= 0 without log2_tables, a negative header_bytes / exception_row_base, n <= 0, 64-bit
 * arrays or fixed_costs not 8-byte aligned -> EAE_HIP_BAD_ARGUMENT, before any launch. One launch, one block per image.
 *
 * eae_hip_latent_quantize_rows (latent_rows.hip): the quantiser half of eae_hip_latent_stage (no gdn_3: y [N][hw][128] are the
 * latents the quantiser sees) with one row of bin widths per image: image i takes bin_widths_points[clamp(point[i], 0, K - 1)] (float32 [K][128]; point
 * int32 [N] in device memory, e.g. eae_hip_ladder_select's). Outputs as eae_hip_latent_stage: planar int16 symbols, dead-map
 * flags, the three checks (summed over the images; flags and checks are set / added to: the caller zeroes them), shifted_out
 * (nullable) and, with gamma_out_packed / beta_out, t_out = inverse_gdn_4(shifted). Image i's results are bit for bit
 * eae_hip_latent_stage's on y[i] with that row, whichever images share a 32-position tile with it. hw <= 2^21 (beyond:
 * EAE_HIP_BAD_SHAPE); NULL y / bin_widths_points / point, k_points < 1, gamma without beta or without t_out, n or hw <= 0,
 * float arrays not 16-byte aligned -> EAE_HIP_BAD_ARGUMENT. One launch. */
int eae_hip_ladder_select(const uint32_t* hist, const uint64_t* bypass_bits, const uint32_t* fixed_costs, const uint32_t* log2_tables,
                          int k_points, int length, int idx_map_exception, int64_t header_bytes, int map_size, const int64_t* budgets,
                          int exception_row_base, int32_t* point, int32_t* prob_row, int64_t* upper, uint32_t* flags, int n, void* stream);
int eae_hip_latent_quantize_rows(const float* y, const float* map_mean, const float* bin_widths_points, const int32_t* point, int k_points,
                                 const float* gamma_out_packed, const float* beta_out, float* shifted_out, float* t_out,
                                 int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks, int n, int hw, void* stream);
/* eae_hip_ladder_select for single-image EAT1 blobs, from what eae_hip_ladder_histograms_tiles left: hist
 * uint32 [N][K][T][128][L + 1], bypass_bits uint64 [N][K][T][128], T = nb_tiles. Equal, element for element, to
 * ratecontrol.upper_bounds_fixed_tiles + valid_points (on the counts summed over T) + select_by_upper_bound. Every (tile, map) is a
 * pair of streams of its own: bytes = (((fp + 2^20 - 1) >> 20) + 3 + 7) / 8 + (bypass + 7) / 8 per tile, fp from the tile's counts.
 * The exception map keeps ONE row per image, measured on the whole map: with Z, O its whole-map counts of a decision (summed over
 * the tiles inside, before any tile is priced), a tile's z zeros and o ones cost z (Lceil[Z + O] - Lfloor[Z]) + o (Lceil[Z + O] -
 * Lfloor[O]); o C99 when Z is 0, z C99 when O is 0. map_size: symbols of a WHOLE map (sizes log2_tables and the validity of a
 * point); header_bytes: ratecontrol.header_bytes(..., coding_tile); fixed_costs, log2_tables, budgets, exception_row_base, upper,
 * point, flags as eae_hip_ladder_select.
 *   entry_image int32 [n_entries], device memory: the image of every entry (image, tile) in the order the coder takes them (the
 *                          run order of codec.coding_tile_layout); a value outside [0, N) is clamped
 *   prob_row int32 [n_entries][128]: point[image] * 128 + m; exception_row_base + image for the exception map
 * Every element of every output is written by every call. Argument checks as eae_hip_ladder_select, and NULL entry_image, nb_tiles or
 * n_entries < 1 -> EAE_HIP_BAD_ARGUMENT; nb_tiles > map_size, K T 128 (L + 1) or n_entries 128 >= 2^31 -> EAE_HIP_BAD_SHAPE. Two
 * launches: one block per image, then prob_row. */
int eae_hip_ladder_select_tiles(const uint32_t* hist, const uint64_t* bypass_bits, const uint32_t* fixed_costs, const uint32_t* log2_tables,
                                int k_points, int length, int idx_map_exception, int64_t header_bytes, int map_size, int nb_tiles,
                                const int64_t* budgets, const int32_t* entry_image, int n_entries, int exception_row_base, int32_t* point,
                                int32_t* prob_row, int64_t* upper, uint32_t* flags, int n, void* stream);

/* ---- a PSNR floor per image, searched on the device (csrc/hip/quality.hip; ratecontrol.py) ---------------
 * eae_hip_quality_search: ONE round of the bisection that finds, per image, the coarsest rate point >= first whose squared error
 * against the input is at most max_sse. Integer arithmetic only; after round nb_rounds it equals, element for element,
 * ratecontrol.select_by_quality. A step calls it nb_rounds + 1 times, round = 0, 1, .., nb_rounds, and between round r - 1 and
 * round r quantises every image at point[i] (eae_hip_latent_quantize_rows), synthesises it and adds its squared error into
 * probe_acc[i] (eae_hip_tconv9x9s4_luma's sse). Every argument but `round` is the same in every call and none depends on the data.
 *   first int32 [N]          the finest point the search may take (eae_hip_ladder_select's point); clamped to [0, K)
 *   max_sse int64 [N]        the threshold: ratecontrol.max_sse_for_psnr
 *   state int32 [N][2]       (L, R) of the bisection: points <= L met the threshold, points >= R did not
 *   probe_acc uint64 [N]     the squared error of the point the previous round left in `point`; zeroed by every round
 *   point int32 [N]          the point to quantise next: the next probe, after the last round the chosen point
 *   prob_row int32 [N][128]  point * 128 + m; exception_row_base + i for the exception map (as eae_hip_ladder_select)
 *   trace_point int32 [N][nb_rounds], trace_sse int64 [N][nb_rounds]   what round r probed and found, in column r - 1
 *   flags uint32 [N]         bit 0: met (the chosen point's squared error was within max_sse); 0 before the last round
 * Round 0: (L, R) = (first - 1, K); every element of the trace = -1. Round r >= 1: with mid the point round r - 1 left, column
 * r - 1 of the trace = (mid, probe_acc); when R - L > 1 (a LIVE round), L = mid if probe_acc <= max_sse, else R = mid. Every round
 * then leaves the next point -- (L + R) >> 1 when R - L > 1, else max(L, first), which moves nothing -- and after round nb_rounds
 * point = L and met = 1 if L >= first, else point = first and met = 0. Round 0 writes every element of every output; a later
 * round writes state, probe_acc, point, prob_row, flags and its column of the trace.
 * nb_rounds must be ceil(log2(k_points + 1)) (ratecontrol.quality_rounds): the interval is then one point wide whatever the data.
 * A NULL pointer, k_points < 1, another nb_rounds, round outside [0, nb_rounds], idx_map_exception >= 128, a negative
 * exception_row_base, n <= 0, a 64-bit array not 8-byte aligned -> EAE_HIP_BAD_ARGUMENT; n > 65535 -> EAE_HIP_BAD_SHAPE; both
 * before any launch. One launch, one block per image: 11 to 12 us at 24 images (profiles/quality_codec.md). */
int eae_hip_quality_search(const int32_t* first, const int64_t* max_sse, int32_t* state, uint64_t* probe_acc, int32_t* point,
                           int32_t* prob_row, int32_t* trace_point, int64_t* trace_sse, uint32_t* flags, int k_points, int nb_rounds,
                           int round, int idx_map_exception, int exception_row_base, int n, void* stream);
/* eae_hip_quality_search for a step in coding tiles (codec.TiledQualityCodec): the same round, state, trace and
 * arguments, with the coder's rows written per stream of the step, where the coder takes them from.
 *   run_entry int32 [N * nb_tiles], device memory: the run-order index (codec.coding_tile_layout) of every entry (image, tile), in
 *                          payload order (image, then tile); an entry whose value lies outside [0, N * nb_tiles) is skipped
 *   prob_row int32 [N * nb_tiles][128]: for run-order entry e of image i, prob_row[e][m] = point[i] * 128 + m; exception_row_base + i
 *                          for the exception map (as eae_hip_ladder_select_tiles)
 * With nb_tiles == 1 and run_entry the identity every word equals eae_hip_quality_search's. Argument checks as
 * eae_hip_quality_search, and NULL run_entry or nb_tiles < 1 -> EAE_HIP_BAD_ARGUMENT; n * nb_tiles > 65535 -> EAE_HIP_BAD_SHAPE;
 * before any launch. One launch, one block per image, which walks the image's own tiles: no block reads what another block of the
 * same launch writes. */
int eae_hip_quality_search_tiles(const int32_t* first, const int64_t* max_sse, int32_t* state, uint64_t* probe_acc, int32_t* point,
                                 int32_t* prob_row, int32_t* trace_point, int64_t* trace_sse, uint32_t* flags, const int32_t* run_entry,
                                 int nb_tiles, int k_points, int nb_rounds, int round, int idx_map_exception, int exception_row_base,
                                 int n, void* stream);

/* ---- rate-distortion optimised quantiser (csrc/hip/latent_rows.hip; ratecontrol.py) ----------------------
 * eae_hip_latent_quantize_rdo: eae_hip_latent_quantize_rows with one more input, thresholds_points float32 [K][128][16]
 * (ratecontrol.rdo_thresholds; image i takes row clamp(point[i], 0, K - 1) of it as of bin_widths_points), and `length`, the
 * truncated unary length L. Per latent, in IEEE float32: centered = y - mean; x = centered / bw; r = round_half_even(x); a = |r|;
 * u = |x| - a; if a >= 1 && a <= min(L, 16) (tested in float: a NaN, an infinity or a huge a never indexes the table) and
 * 2 u + 1 < thresholds[k][c][(int)a - 1], then r = r - copysign(1, r): the symbol one step nearer zero. From that r on every
 * statement, output, check and flag is eae_hip_latent_quantize_rows': cq = bw r, the symbol round_half_even(cq / bw), shifted_out,
 * t_out = inverse_gdn_4(shifted). Equal to ratecontrol.rdo_quantize_numpy element for element; with a table of zeros (the
 * comparison is strict) equal to eae_hip_latent_quantize_rows bit for bit. The decoder is unchanged: the symbols are ordinary ones.
 * Refusals as eae_hip_latent_quantize_rows, and a NULL or not 16-byte aligned thresholds_points or length outside [1, 255] ->
 * EAE_HIP_BAD_ARGUMENT, before any launch. One launch. */
int eae_hip_latent_quantize_rdo(const float* y, const float* map_mean, const float* bin_widths_points, const float* thresholds_points,
                                const int32_t* point, int k_points, int length, const float* gamma_out_packed, const float* beta_out,
                                float* shifted_out, float* t_out, int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks,
                                int n, int hw, void* stream);

/* ---- the ladder's counts of the rate-distortion optimised symbols (csrc/hip/ladder.hip; ratecontrol.py) --
 * eae_hip_ladder_histograms_rdo: eae_hip_ladder_histograms with one more input, the thresholds of the K points, and with `length`
 * deciding which magnitudes may be lowered. The table arrives BY MAGNITUDE, not in eae_hip_latent_quantize_rdo's layout:
 *   thresholds_by_magnitude float32 [K][16][128]:  [k][a - 1][c] = ratecontrol.rdo_thresholds(...)[k][c][a - 1], the transposed copy
 *                                                  of a ladder's (K, 128, 16) table (a lane of the kernel owns a channel: the lanes
 *                                                  of a wave that hold the same magnitude read 256 contiguous bytes)
 * Per latent and point k, in IEEE float32 with no contraction, statement for statement eae_hip_latent_quantize_rdo's rule
 * (ratecontrol.rdo_quantize_numpy): centered = y - mean; x = centered / bw; r = round_half_even(x); a = |r|; u = |x| - a; if
 * a >= 1 && a <= min(L, 16) (tested in float: a NaN, an infinity or a huge a never indexes the table) and
 * 2 u + 1 < thresholds_by_magnitude[k][(int)a - 1][c], then r = r - copysign(1, r). From that r on every statement is
 * eae_hip_ladder_histograms': cq = bw r; rs = round_half_even(cq / bw); the range check, the bin min(|rs|, L), the bypass bits.
 *   - With thresholds all zero (the comparison is strict) every output word equals eae_hip_ladder_histograms' on the same input.
 *   - For every k, hist[i][k] is the clipped histogram, and bypass_bits[i][k] the bypass length, of the symbols
 *     eae_hip_latent_quantize_rdo writes for image i when point[i] == k (given the same table in its own layout).
 * Outputs, accumulation, the limits on k_points and length and every refusal are eae_hip_ladder_histograms'; a NULL or not 16-byte
 * aligned thresholds_by_magnitude -> EAE_HIP_BAD_ARGUMENT, before any launch. One launch, the LDS of eae_hip_ladder_histograms (the
 * table stays in memory): eae_hip_ladder_max_points holds for both. */
int eae_hip_ladder_histograms_rdo(const float* y, const float* map_mean, const float* bin_widths_points,
                                  const float* thresholds_by_magnitude, int k_points, int length, uint32_t* hist, uint64_t* bypass_bits,
                                  uint32_t* range_errors, int n, int hw, void* stream);
/* The same per coding tile: eae_hip_ladder_histograms_tiles with thresholds_by_magnitude as above. hist uint32
 * [N][K][T][128][L + 1], bypass_bits uint64 [N][K][T][128] (nullable), range_errors uint32 [K] (nullable), all ACCUMULATED into;
 * summed over T they are eae_hip_ladder_histograms_rdo's outputs on the same input, and with thresholds all zero every word equals
 * eae_hip_ladder_histograms_tiles'. Refusals as eae_hip_ladder_histograms_tiles, and a NULL or not 16-byte aligned
 * thresholds_by_magnitude -> EAE_HIP_BAD_ARGUMENT, before any launch. One launch, at most two blocks per compute unit. */
int eae_hip_ladder_histograms_rdo_tiles(const float* y, const float* map_mean, const float* bin_widths_points,
                                        const float* thresholds_by_magnitude, int k_points, int length, uint32_t* hist,
                                        uint64_t* bypass_bits, uint32_t* range_errors, int n, int h, int w, int th, int tw, void* stream);

/* ---- lossless coder on the device: one feature map per lane --------------------------------------------------------
 * Replaces the per-map compress_lossless loop of lossless/compression.py:76-81 (and, underneath it,
 * lossless/c++/source/compression.cpp:3-65) for a whole batch of images whose symbols are already in HBM
 * (symbols_planar of eae_hip_quantize_maps). Same arguments and stream layout as the HOST entry points
 * eae_coder_compress_maps / eae_coder_encode_maps / eae_coder_decode_maps of include/eae_coder.h, every pointer a
 * DEVICE pointer; same source for the arithmetic (csrc/coder/coder_core.h), so bits, bytes, bit counts and error codes
 * are identical to the host library's and therefore to the reference's.
 *   symbols [n_maps][map_size] int16; probs [rows][L] float64; prob_row[m] = row for map m, < 0 skips the map
 *   (exception map: 0 bits, verbatim copy when `reconstruction` is given), NULL = row m;
 *   streams: n_maps regions of `stride` bytes, BAC bytes at +0, bypass bytes at +stride/2 (stride from
 *   eae_hip_coder_stream_stride_bytes; 8-byte aligned base); bac_bits/bypass_bits/status/stage: per map.
 *   mode: 0 encode + decode into `reconstruction`; 1 encode only; 2 encode + decode + compare in registers
 *   (status 6 = EAE_ROUNDTRIP_MISMATCH). lanes_per_wave: 1..64 = that many maps per 64-thread block, one per lane
 *   (fewer lanes = more blocks over more CUs and less divergence per wave, but more wave-instructions in total);
 *   <= 0 = one wavefront per map with wave-uniform state (scalar registers, ~20 VGPRs: shortest latency per map).
 * Returns 0, -1 (NULL argument / bad mode), 1 (stride too small: EAE_CAPACITY_ERROR) or a hipError_t. Per-map failures
 * are reported in status[] (the launch is asynchronous). */
uint64_t eae_hip_coder_stream_stride_bytes(uint32_t map_size, uint8_t truncated_unary_length);
int eae_hip_coder_compress_maps(uint32_t n_maps, uint32_t map_size, const int16_t* symbols, int16_t* reconstruction,
                                uint8_t truncated_unary_length, const double* probabilities, const int32_t* prob_row,
                                uint8_t* streams, uint64_t stream_stride_bytes, uint32_t* bac_bits, uint32_t* bypass_bits,
                                int32_t* status, int32_t* stage, int mode, int lanes_per_wave, void* stream);
int eae_hip_coder_decode_maps(uint32_t n_maps, uint32_t map_size, int16_t* symbols_out, uint8_t truncated_unary_length,
                              const double* probabilities, const int32_t* prob_row, const uint8_t* streams,
                              uint64_t stream_stride_bytes, const uint32_t* bac_bits, const uint32_t* bypass_bits,
                              int32_t* status, int32_t* stage, int lanes_per_wave, void* stream);
/* The second half of compress_lossless as its own launch (so that it can run on another stream, concurrently with the
 * next batch's encode): decodes every map from its streams and compares with `expected` (the symbols that were
 * encoded) in registers. status[m] = 6 (EAE_ROUNDTRIP_MISMATCH) or a decoder error; maps whose status is already
 * non-zero (failed encode) and skipped maps are left alone. */
int eae_hip_coder_verify_maps(uint32_t n_maps, uint32_t map_size, const int16_t* expected, uint8_t truncated_unary_length,
                              const double* probabilities, const int32_t* prob_row, const uint8_t* streams,
                              uint64_t stream_stride_bytes, const uint32_t* bac_bits, const uint32_t* bypass_bits,
                              int32_t* status, int32_t* stage, int lanes_per_wave, void* stream);

/* ---- the same coder, 64 maps per wavefront in step (csrc/hip/coder_simd.hip) -----------------------------------------
 * Same arguments, stream layout and results as the entry points above, organised for the machine. Only the interval
 * arithmetic of the binary arithmetic coder is serial (one map per lane, csrc/coder/lean_step.h); everything around it is
 * data-parallel over the symbols:
 *   encode_batch: binarise (decisions, the bypass stream of signs / Exp-Golomb suffixes) -> the serial core, which leaves
 *     one 32-bit record per decision (the bits that may leave, E1/E2 and E3 counts) -> emit (prefix sums over the records
 *     place the bits and the pending-E3 runs in the stream);
 *   decode_batch: the serial core reads the stream through a small ring in LDS and leaves one byte per symbol (its
 *     truncated-unary prefix) -> debinarise (signs, suffixes from the bypass stream) -> compare with `expected`.
 * Every map the fast kernels cannot finish (any error, streams that outgrow their region, exotic lengths) is recoded by
 * the general kernel above, so statuses, stages, bit counts and bytes are identical in every case. These are the launches
 * bench.py times.
 *   streams / stream_stride_bytes: as above, with every map's two streams on 16-byte boundaries and 16 spare bytes per
 *   stream (the stride of eae_hip_coder_stream_stride_bytes on a 16-byte aligned base does that): encode_batch returns
 *   1 (hipErrorInvalidValue) for any other layout, decode_batch hands such streams to the general kernel, map by map.
 *   L == 0 and L > 32 go to the general kernel too. Same results in every case.
 *   workspace: device scratch of eae_hip_coder_workspace_bytes(n_maps, map_size, L) bytes, private to the call chain
 *   (encode_batch followed by decode_batch of the same maps may share it; concurrent batches need their own). It holds the
 *   decisions and records of the batch: about 4 * (L + 1) + 12 bytes per symbol for the records alone.
 *   encode_batch: symbols -> streams + bac_bits/bypass_bits/status/stage (all written for every map).
 *   decode_batch: streams -> symbols_out (expected == NULL; status/stage written for every map; skipped maps are left
 *   untouched), or, with expected != NULL, decode into the workspace (symbols_out may be NULL) and compare: maps whose
 *   status is already non-zero are left alone, a difference gives status 6 (EAE_ROUNDTRIP_MISMATCH). */
uint64_t eae_hip_coder_workspace_bytes(uint32_t n_maps, uint32_t map_size, uint8_t truncated_unary_length);
int eae_hip_coder_encode_batch(uint32_t n_maps, uint32_t map_size, const int16_t* symbols, uint8_t truncated_unary_length,
                               const double* probabilities, const int32_t* prob_row, uint8_t* streams,
                               uint64_t stream_stride_bytes, uint32_t* bac_bits, uint32_t* bypass_bits, int32_t* status,
                               int32_t* stage, void* workspace, uint64_t workspace_bytes, void* stream);
int eae_hip_coder_decode_batch(uint32_t n_maps, uint32_t map_size, int16_t* symbols_out, const int16_t* expected,
                               uint8_t truncated_unary_length, const double* probabilities, const int32_t* prob_row,
                               const uint8_t* streams, uint64_t stream_stride_bytes, const uint32_t* bac_bits,
                               const uint32_t* bypass_bits, int32_t* status, int32_t* stage, void* workspace,
                               uint64_t workspace_bytes, void* stream);

/* ==== EXPERIMENTAL (-DEAE_EXPERIMENTAL_CODER): NOT exported by the product library lib/libeae_hip.so ==========================
 * Two byte-exact alternatives for the coder's round trip on small batches, both measured slower than the encode_batch +
 * decode_batch pair on this runtime. They are compiled into lib/libeae_hip_test.so only
 * (csrc/Makefile: `make hip-test`), where their parity tests run (tests/test_coder_device.py). */
#ifdef EAE_EXPERIMENTAL_CODER
/* The round trip of lossless/c++/source/compression.cpp:27-64 (encode every map, decode it back, compare) for SMALL batches -- one or
 * two images, two to four wavefronts of maps -- where what it costs is the length of its serial chains one after the other. The
 * chains are cut into `chunks` launches (2..16; 4 is a good value): while the encoder core runs chunk c + 1 the emit pass assembles
 * the stream words of chunk c and the decoder works through those of chunk c - 1, on two side streams of the library's own joined
 * to `stream` by events (nothing is polled: capturable into a hipGraph). Results as eae_hip_coder_encode_batch followed by
 * eae_hip_coder_decode_batch(expected = symbols): same stream bytes, bit counts, statuses (6 on a difference) and stages, same
 * fall-back to the general kernel per map. workspace: eae_hip_coder_trailing_workspace_bytes. chunks < 2: the two calls one after
 * the other. For large batches the transforms of the batches in flight hide the coder anyway and the extra launches only cost. */
uint64_t eae_hip_coder_trailing_workspace_bytes(uint32_t n_maps, uint32_t map_size, uint8_t truncated_unary_length);
int eae_hip_coder_roundtrip_trailing(uint32_t n_maps, uint32_t map_size, const int16_t* symbols, uint8_t truncated_unary_length,
                                     const double* probabilities, const int32_t* prob_row, uint8_t* streams,
                                     uint64_t stream_stride_bytes, uint32_t* bac_bits, uint32_t* bypass_bits, int32_t* status,
                                     int32_t* stage, void* workspace, uint64_t workspace_bytes, uint32_t chunks, void* stream);

/* The same round trip with the three serial stages of every group of 64 maps in ONE workgroup: the encoder core, a bit writer
 * (the emit pass, one map per lane) and the decoder core are three wavefronts that hand records and stream words to each other
 * through rings in LDS, so the decoder runs a few hundred bits behind the encoder instead of after it, and the records never go
 * to memory. One stream, five launches (binarise, the pipeline, the general kernel for what the pipeline hands over, debinarise,
 * compare). Same stream bytes, bit counts, statuses and stages as encode_batch + decode_batch(expected = symbols).
 * workspace: eae_hip_coder_trailing_workspace_bytes. */
int eae_hip_coder_roundtrip_fused(uint32_t n_maps, uint32_t map_size, const int16_t* symbols, uint8_t truncated_unary_length,
                                  const double* probabilities, const int32_t* prob_row, uint8_t* streams,
                                  uint64_t stream_stride_bytes, uint32_t* bac_bits, uint32_t* bypass_bits, int32_t* status,
                                  int32_t* stage, void* workspace, uint64_t workspace_bytes, void* stream);

#endif /* EAE_EXPERIMENTAL_CODER */

/* ---- container support (the reference never serialises, compression.cpp:27-64) ------------------
 * pack_streams: gathers the valid bytes of every map's two streams (layout above) into `payload`: the arithmetic-coded
 * bytes of map m at offsets[2m], its bypass bytes at offsets[2m+1] (uint64 byte offsets, device memory, chosen by the
 * caller from the bit counts); unpack_streams is the inverse, into a stream region a decoder can read.
 * dequantize_maps: the inverse of the symbol conversion of lossless/compression.py:142 followed by the de-centring of
 * reconstructing_eae_kodak.py:192: symbols_planar [N][128][hw] int16 -> cq_out = bin_widths[c] * symbol (the exact value
 * tools.py:929 produced) and shifted_out = cq + map_mean[c], both f32 [N][hw][128], each nullable. */
int eae_hip_coder_pack_streams(uint32_t n_maps, const uint8_t* streams, uint64_t stream_stride_bytes, const uint32_t* bac_bits,
                               const uint32_t* bypass_bits, const uint64_t* offsets, uint8_t* payload, void* stream);
int eae_hip_coder_unpack_streams(uint32_t n_maps, const uint8_t* payload, const uint64_t* offsets, const uint32_t* bac_bits,
                                 const uint32_t* bypass_bits, uint8_t* streams, uint64_t stream_stride_bytes, void* stream);
int eae_hip_dequantize_maps(const int16_t* symbols_planar, const float* bin_widths, const float* map_mean, float* cq_out,
                            float* shifted_out, int n, int hw, int c, void* stream);

/* ---- containers from the pipelined codec (csrc/hip/codec_container.hip) --------------------------
 * What container.encode_images does between the coder and the blob, with device-resident arguments only: every call is
 * asynchronous on `stream`, none has an argument the host has to compute from a result of the step, so all five can be captured
 * into a hipGraph behind the coder's launches.
 * index_streams: the piece e = 2 m + piece of map m (arithmetic-coded bytes, bypass bytes) is min((bits + 7) >> 3, stride / 2)
 *   bytes long, as pack_streams copies it. offsets_out[2 n_maps]: the exclusive prefix sum of those lengths in payload order
 *   (image -> map -> piece), 64-bit; index_out[0] their total, index_out[1] = 1 when the total exceeds capacity_bytes (else 0),
 *   index_out[2 + i] the bytes of image i (n_maps / maps_per_image images). n_maps >= 1; n_maps not a multiple of
 *   maps_per_image -> EAE_HIP_BAD_SHAPE.
 * pack_indexed: pack_streams, except that nothing is copied when index[1] != 0 (the payload buffer holds capacity_bytes).
 * publish_prefix: the first ceil(min(*nbytes_device, capacity_bytes) / 16) 16-byte words of src_device into pinned,
 *   device-mapped host memory, visible to the host as eae_hip_publish_to_host's copy is; no byte at or beyond that length is
 *   written. Both buffers hold capacity_bytes (a multiple of 16) and are 16-byte aligned, else EAE_HIP_BAD_ARGUMENT.
 * exception_rows: the probability row of an image's exception map from that map's histogram (stats.py:181-195, :56-66 on
 *   eae_hip_symbol_histograms' output: hist uint32 [n][2 radius + 1], overflow uint32 [n]): with zeros[j] = the symbols of
 *   magnitude j and ones[j] = map_size - the symbols of magnitude <= j, rows_out[i][j] = zeros / (zeros + ones) in float64, 0 / 0
 *   -> 0.5, 0 -> 0.01, 1 -> 0.99, j < length. Needs radius >= length (EAE_HIP_BAD_ARGUMENT otherwise): then a symbol beyond the
 *   radius is a one of every position, which map_size already accounts for, so the rows are exact whatever `overflow` counts
 *   (it is not read).
 * index_tiles: index_streams for a step coded in coding tiles (codec.BatchCodec(coding_tile=...)). An entry
 *   is one (image, tile): maps_per_entry maps. bac_bits / bypass_bits [n_streams] and offsets_out [2 n_streams] are in RUN order
 *   (the entries of one shape class side by side, as the coder batches them); the payload is in PAYLOAD order (image -> tile,
 *   row-major -> map -> piece). entry_table uint64 [n_streams / maps_per_entry][2], device memory, one row per payload-order
 *   entry: its run-order entry index, and half the stream stride of its class, to which its pieces are clamped as pack_indexed
 *   clamps them. offsets_out of a piece: the exclusive prefix sum, taken in payload order, of the clamped lengths, so that a
 *   class's pack_indexed takes a plain slice of it. index_out as index_streams', image i = the payload-order entries
 *   [i entries_per_image, (i + 1) entries_per_image). With one entry per image, the identity table and one stride it writes
 *   what index_streams writes, word for word. Three launches (per entry, over the entries, per entry), no scratch: plain loads
 *   and stores. A table row that names no entry is skipped. NULL pointers, n_streams == 0, maps_per_entry == 0 or
 *   entries_per_image == 0 -> EAE_HIP_BAD_ARGUMENT; n_streams not a multiple of maps_per_entry * entries_per_image ->
 *   EAE_HIP_BAD_SHAPE; both before any launch. */
int eae_hip_coder_index_tiles(uint32_t n_streams, uint32_t maps_per_entry, uint32_t entries_per_image, const uint32_t* bac_bits,
                              const uint32_t* bypass_bits, const uint64_t* entry_table, uint64_t capacity_bytes,
                              uint64_t* offsets_out, uint64_t* index_out, void* stream);
int eae_hip_coder_index_streams(uint32_t n_maps, uint32_t maps_per_image, const uint32_t* bac_bits, const uint32_t* bypass_bits,
                                uint64_t stream_stride_bytes, uint64_t capacity_bytes, uint64_t* offsets_out, uint64_t* index_out,
                                void* stream);
int eae_hip_coder_pack_indexed(uint32_t n_maps, const uint8_t* streams, uint64_t stream_stride_bytes, const uint32_t* bac_bits,
                               const uint32_t* bypass_bits, const uint64_t* offsets, const uint64_t* index, uint8_t* payload,
                               void* stream);
int eae_hip_publish_prefix(const void* src_device, void* dst_host_mapped, uint64_t capacity_bytes, const uint64_t* nbytes_device,
                           void* stream);
int eae_hip_exception_rows(int n, const uint32_t* hist, const uint32_t* overflow, int radius, int map_size, int length,
                           double* rows_out, void* stream);

/* ---- the pipelined decoders' own launches (csrc/hip/codec_decode.hip; DESIGN.md sections 14 and 17) ---------------------
 * The rest of a codec.BatchDecoder step is index_streams, unpack_streams, coder_decode_batch, eae_hip_decode and the publish
 * launches above. All three are asynchronous on `stream` and have no argument the host computes from the step's contents, so a step
 * can be captured into one hipGraph.
 * fetch_prefix: the mirror of publish_prefix: the first ceil(min(*nbytes_device, capacity_bytes) / 16) 16-byte words of pinned,
 *   device-mapped host memory into dst_device; no byte at or beyond that length is written. *nbytes_device is read on the device
 *   (a word an earlier launch of the stream left there). Both buffers hold capacity_bytes (a multiple of 16) and are 16-byte
 *   aligned, nbytes_device 8-byte aligned, else EAE_HIP_BAD_ARGUMENT.
 * dequantize_maps_rows: eae_hip_dequantize_maps with one row of bin widths and means per image: bin_widths_rows and
 *   map_mean_rows (nullable) are f32 [n][128]. Image i's outputs are bit-identical to eae_hip_dequantize_maps of that image with
 *   row i. The outputs leave as 16-byte stores: cq_out / shifted_out (each nullable, not both) 16-byte aligned and n <= 65535,
 *   else EAE_HIP_BAD_SHAPE. */
int eae_hip_fetch_prefix(const void* src_host_mapped, void* dst_device, uint64_t capacity_bytes, const uint64_t* nbytes_device,
                         void* stream);
int eae_hip_dequantize_maps_rows(const int16_t* symbols_planar, const float* bin_widths_rows, const float* map_mean_rows,
                                 float* cq_out, float* shifted_out, int n, int hw, int c, void* stream);
/* publish_crops (codec.RegionDecoder): the ch x cw rectangle at origins[i] = (row, col) -- int32 [n][2] in
 *   DEVICE memory, read by the kernel -- of every plane of planes u8 [n][H][W] into dst = u8 [n][ch][cw], flat: pinned,
 *   device-mapped host memory (visible to the host as eae_hip_publish_to_host's copy is) or device memory. Every store is one
 *   16-byte word of dst; the bytes of the last word behind n * ch * cw are zero, and nothing behind that word is written. The
 *   origins are clamped on the device to [0, H - ch] x [0, W - cw]: no load leaves the planes whatever the words hold. NULL
 *   pointer, a non-positive size, dst not 16-byte aligned, dst_capacity_bytes no multiple of 16, planes or origins not 4-byte
 *   aligned -> EAE_HIP_BAD_ARGUMENT; ch > H, cw > W, a crop of 2^31 bytes or more, or a capacity below n * ch * cw rounded up to
 *   16 -> EAE_HIP_BAD_SHAPE; nothing is launched then. */
int eae_hip_publish_crops(const uint8_t* planes, int n, int H, int W, const int32_t* origins, int ch, int cw, void* dst,
                          uint64_t dst_capacity_bytes, void* stream);

/* ---- images of any height and width (csrc/hip/frame.hip) --------------------------------------------
 * An h x w image is coded as H x W = (h, w) rounded up to multiples of 16, extended by edge replication; a decoder crops
 * (eae_hip_publish_crops at origin (0, 0)). Both entry points are one launch, asynchronous on `stream`, with no argument the host
 * computes from the data: a step can be captured into a hipGraph. Planes are addressed with 64-bit offsets. NULL pointer or a
 * non-positive size -> EAE_HIP_BAD_ARGUMENT; H x W not the coded size of h x w, or a misaligned dst / sse -> EAE_HIP_BAD_SHAPE;
 * nothing is launched then.
 * frame_pad_u8: src u8 [n][h][w] in device or pinned, device-mapped host memory, at ANY byte address (w odd, h * w odd: image 1
 *   then starts misaligned) -> dst u8 [n][H][W] in device memory, 16-byte aligned:
 *   dst[i][y][x] = src[i][min(y, h - 1)][min(x, w - 1)], the rows of numpy.pad(..., mode='edge'). Every store is one 16-byte word of
 *   a destination row. Every load lies inside the n * h * w bytes of src: no aligned word that begins in front of them or ends
 *   behind them is touched. With h == H and w == W it is a copy.
 * frame_sse_u8: rec u8 [n][H][W], ref u8 [n][h][w] (device memory, any byte address), sse u64 [n], 8-byte aligned:
 *   sse[i] += sum over y < h, x < w of (ref[i][y][x] - rec[i][y][x])^2, exact; the caller zeroes sse (as for eae_hip_sse_u8 and
 *   eae_hip_tconv9x9s4_luma). The pixels of rec outside h x w are not read. */
int eae_hip_frame_pad_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int H, int W, void* stream);
int eae_hip_frame_sse_u8(const uint8_t* rec, const uint8_t* ref, uint64_t* sse, int n, int h, int w, int H, int W, void* stream);

/* ---- colour images, 4:2:0 (csrc/hip/colour.hip) -------------------------------------------------------------
 * An RGB picture of h x w is coded as three planes through the luminance model: Y at h x w, Cb and Cr at hc x wc = ceil(h / 2) x
 * ceil(w / 2). The two entry points stand in front of and behind the codecs of the planes; autoencoder_based_image_compression_amd/
 * colour.py states both in numpy and the kernels are held to it bit for bit. Each is one launch, asynchronous on `stream`, with no
 * argument the host computes from the data (a hipGraph can capture it); images are addressed with 64-bit offsets, the bytes inside
 * one image with 32 bits: h * w * 3 and H * W must stay below 2^32. Every refusal returns EAE_HIP_BAD_ARGUMENT in front of the launch.
 *
 * colour_split_420: rgb u8 [n][h][w][3] dense, in device or pinned, device-mapped host memory, at ANY byte address ->
 *   y u8 [n][h][w], cb and cr u8 [n][hc][wc], dense, in device memory. Per pixel (Y, Cb, Cr) is tls.rgb_to_ycbcr (float64 BT.601,
 *   eae_hip_rgb_to_ycbcr's expressions); the Cb and Cr of a picture are extended to even sides by edge replication and every chroma
 *   sample is (a + b + c + d + 2) >> 2 over its 2 x 2 block. Chroma is not clamped: up to 240 goes in, and the model's cast
 *   (eae_hip_cast_bt601) returns 235 at most. A lane owns one chroma sample. Every load lies inside the n * h * w * 3 bytes of rgb (no
 *   aligned word that begins in front of them or ends behind them is touched), every store inside the three outputs.
 *   Refused: a NULL pointer, a non-positive size, an image of 2^32 bytes or more, more than 2^31 - 1 blocks.
 * colour_merge_420: y u8 [n][H][W], cb and cr u8 [n][Hc][Wc] in device memory -- the coded planes a codec keeps, of which the
 *   top-left h x w and hc x wc are read and NOTHING else (H = h, W = w, Hc = hc, Wc = wc: dense planes) -> rgb_out u8 [n][h][w][3]
 *   dense, in device or pinned host memory, nullable. Chroma is upsampled centre-sited with weights 3:1 both ways, the neighbour
 *   clamped at the REAL chroma size: for pixel (r, c), i = r >> 1, i2 = clip(i + (r & 1 ? 1 : -1), 0, hc - 1), j and j2 alike,
 *   C = (9 P[i][j] + 3 P[i][j2] + 3 P[i2][j] + P[i2][j2] + 8) >> 4; then in int32, with Y' = 298 (Y - 16), U = Cb - 128, V = Cr - 128:
 *   R = clip((Y' + 409 V + 128) >> 8), G = clip((Y' - 100 U - 208 V + 128) >> 8), B = clip((Y' + 516 U + 128) >> 8), clip to [0, 255],
 *   `>>` an arithmetic shift (a floor). ref_rgb u8 [n][h][w][3] dense in device memory with sse u64 [n], 8-byte aligned, both or
 *   neither: sse[i] += the exact squared error of image i over its 3 h w samples (the caller zeroes sse); one 64-bit atomic per block,
 *   and with sse at most 64 blocks per image, which then loop over the image (without it: one chroma sample per lane, no cap).
 *   Refused: y, cb or cr NULL, neither rgb_out nor ref_rgb, ref_rgb without sse or sse without ref_rgb, a misaligned sse, a
 *   non-positive size, H < h, W < w, Hc < hc, Wc < wc, a plane or image of 2^32 bytes or more, more than 2^31 - 1 blocks. */
int eae_hip_colour_split_420(const uint8_t* rgb, uint8_t* y, uint8_t* cb, uint8_t* cr, int n, int h, int w, void* stream);
int eae_hip_colour_merge_420(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* rgb_out, const uint8_t* ref_rgb,
                             uint64_t* sse, int n, int h, int w, int H, int W, int Hc, int Wc, void* stream);

/* colour_merge_420_words: the planes, the top-left rule and the picture of colour_merge_420, written as the
 *   dense [n][h][w][3] batch, flat, into dst in WHOLE aligned 16-byte words -- what a resident decoder publishes, into device or
 *   pinned, device-mapped host memory. With B = n * h * w * 3 and K = ceil(B / 16): exactly the words 0 .. K - 1 of dst are written,
 *   each by one 16-byte store (no narrower store reaches dst); bytes B .. 16 K - 1, the pad of the last word, are zero; nothing
 *   behind word K - 1 is touched, so a longer dst keeps its tail. A lane owns 16 consecutive flat pixels (three words) across row and
 *   picture ends, a block of 256 lanes 768 consecutive words, staged in LDS so that a wave's store instruction writes 1 KB of
 *   consecutive words; ceil(K / 768) blocks, whatever the size (no cap, no loop). Every load lies inside the top-left h x w of y and
 *   hc x wc of cb and cr. One launch, asynchronous on `stream`, no argument computed from data. Picture offsets are 64 bits wide,
 *   everything inside a picture 32.
 *   Refused (EAE_HIP_BAD_ARGUMENT, in front of the launch): y, cb, cr or dst NULL, everything colour_merge_420 refuses of the sizes,
 *   a dst that is not 16-byte aligned, a dst_bytes that is not a multiple of 16 or is less than 16 K, more than 2^31 - 1 blocks. */
int eae_hip_colour_merge_420_words(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* dst, uint64_t dst_bytes,
                                   int n, int h, int w, int H, int W, int Hc, int Wc, void* stream);

/* colour_merge_420_crops: colour_merge_420_words for CROPS of pictures. y u8 [n][rh][rw] dense, crop k the
 *   pixels [y0, y0 + rh) x [x0, x0 + rw) of an h x w picture, (y0, x0) = origins[k]; cb and cr u8 [n][rch][rcw] dense, the chroma
 *   rectangle of colour.py's chroma_region: rch = min(hc, rh / 2 + 3), rcw = min(wc, rw / 2 + 3), its origin
 *   cy0 = min(max((y0 >> 1) - 1, 0), hc - rch), cx0 alike, derived by the kernel. origins i32 [n][2] (row, column) in device or
 *   pinned, device-mapped host memory: the kernel reads it, so no argument of the launch depends on where the crops lie. Pixel
 *   (r, c) of crop k is colour_merge_420's pixel (y0 + r, x0 + c) of the picture: i, i2, j, j2 and the parity of the weights from that
 *   position, the clamp at hc - 1 / wc - 1 of the REAL chroma planes, every chroma index then less (cy0, cx0) -- bit for bit
 *   colour.merge_420_region_numpy. dst as colour_merge_420_words': with B = n * rh * rw * 3 and K = ceil(B / 16) exactly the words
 *   0 .. K - 1 are written, each by one 16-byte store, the pad of the last one zero, nothing behind it; a lane owns 16 consecutive flat
 *   pixels across row and crop ends, a block 768 words staged in LDS, ceil(K / 768) blocks. Every load lies inside the three dense
 *   inputs and origins. 0 <= y0 <= h - rh and 0 <= x0 <= w - rw are the caller's to ensure (an origin outside is clamped into that
 *   range, so that no load leaves the inputs; the pixels are then those of the clamped crop). One launch, asynchronous on `stream`.
 *   Refused (EAE_HIP_BAD_ARGUMENT, in front of the launch): a NULL pointer, a non-positive size, rh > h or rw > w, rch or rcw other
 *   than chroma_region's, a picture of 2^32 bytes or more, origins not 4-byte aligned, a dst that is not 16-byte aligned, a
 *   dst_bytes that is not a multiple of 16 or is less than 16 K, more than 2^31 - 1 blocks. */
int eae_hip_colour_merge_420_crops(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, const int32_t* origins, uint8_t* dst,
                                   uint64_t dst_bytes, int n, int h, int w, int rh, int rw, int rch, int rcw, void* stream);

/* colour_budget_rest: the byte budget of the luminance plane of n colour pictures, from what their chroma planes
 *   took -- ratecontrol.colour_luma_budgets, integers only, so that the number never visits the host between the chroma steps and the
 *   luminance step of a colour codec. budgets i64 [n]: B, the budget of each picture's single-picture EAC1 blob; header_bytes: the
 *   bytes of the EAC1 header in front of the three plane blobs (container.py's colour header struct, 48); upper_cb, upper_cr i64
 *   [n][k_points]: the upper bounds of the chroma planes at every point (eae_hip_ladder_select's `upper`, byte counts, never
 *   negative); point_cb, point_cr i32 [n]: the points they took. With P = max(B - header_bytes, 0):
 *     out[i] = max(max(P - upper_cb[i][point_cb[i]], 0) - upper_cr[i][point_cr[i]], 0)
 *   which for bounds that are not negative is max(P - ub_cb - ub_cr, 0), and in which no difference leaves int64 for any B in
 *   [-2^63 + header_bytes, 2^63). A picture with a point outside [0, k_points) gets out[i] = 0 and nothing of its rows is loaded.
 *   All six in device or pinned, device-mapped host memory. One lane per picture, ceil(n / 256) blocks of 256, any n; one launch,
 *   asynchronous on `stream`, no argument computed from data.
 *   Refused (EAE_HIP_BAD_ARGUMENT, in front of the launch): a NULL pointer, n or k_points not positive, header_bytes negative, a 64-bit
 *   array that is not 8-byte aligned, a point array that is not 4-byte aligned. */
int eae_hip_colour_budget_rest(const int64_t* budgets, const int64_t* upper_cb, const int32_t* point_cb, const int64_t* upper_cr,
                               const int32_t* point_cr, int64_t* out, int n, int k_points, int64_t header_bytes, void* stream);

/* colour_quality_rest: the squared-error threshold of the luminance plane of n colour pictures, from what their
 *   chroma planes spent -- ratecontrol.colour_luma_max_sse, integers only, so that the number never visits the host between the
 *   chroma steps and the luminance step of a colour codec. max_sse i64 [n]: M, the threshold of each picture over all samples of
 *   its 4:2:0 form, in [0, 2^62]; sse_cb, sse_cr i64 [n]: the squared errors of the points the chroma planes took, over their real
 *   samples, never negative.
 *     out[i] = max(max(M - sse_cb[i], 0) - sse_cr[i], 0)
 *   which for errors that are not negative is max(M - sse_cb - sse_cr, 0); no difference leaves int64. All four in device or
 *   pinned, device-mapped host memory. One lane per picture, ceil(n / 256) blocks of 256, any n; one launch, asynchronous on
 *   `stream`, no argument computed from data.
 *   Refused (EAE_HIP_BAD_ARGUMENT, in front of the launch): a NULL pointer, n not positive, an array that is not 8-byte aligned. */
int eae_hip_colour_quality_rest(const int64_t* max_sse, const int64_t* sse_cb, const int64_t* sse_cr, int64_t* out, int n, void* stream);

/* ==== TEST HOOKS (-DEAE_TEST_HOOKS): NOT exported by the product library lib/libeae_hip.so ====================================
 * Five entry points the test-suite needs and a deployment must not have (they change what later launches do, or only
 * exist to prove something about the kernels). Compiled into lib/libeae_hip_test.so only; tests/test_abi.py checks that
 * the product library exports no symbol of this section (nor any other `debug` symbol). */
#ifdef EAE_TEST_HOOKS
/* Diagnostic hook (not part of the path): when given a device buffer of grid * waves * 8 uint64, the conv GEMM kernel
 * records s_memtime stamps per wave (start, loop start, loop end, GDN end, end, K-steps, XCC id, HW id). NULL disables. */
int eae_hip_debug_set_stamp_buffer(uint64_t* device_buffer);

/* Kernel-form overrides (EAE_HIP_GEMM, EAE_HIP_SPLIT_WAVES, EAE_HIP_FORCE_TILE, EAE_HIP_FORCE_NT, EAE_HIP_LATENT: README.md) are
 * read from the environment ONCE, when the library is loaded -- no launch reads the environment, and a hipGraph captures what
 * every later launch would have done anyway. The parity tests of every kernel form change the environment inside one process and
 * then call this to have it read again. Not part of the path. */
int eae_hip_debug_reload_launch_options(void);
/* Fault injection for the cut-tile hand-off of the conv launches (tests/test_gpu_conv_split.py, tests/test_gpu_codec.py): with
 * on != 0 the heads of cut tiles never publish and the tails give up after ~1 ms, so the launch reports the hand-off failure
 * (eae_hip_conv_workspace_collect, eae_hip_transform_status). Reachable through this entry point only -- no environment variable
 * can make a deployment drop tiles. */
int eae_hip_debug_set_split_mute(int on);
/* Proof harness of the normalisations' mid-range forms (csrc/hip/common.h: sqrt_mid, div_mid -- hipcc's correctly rounded sqrtf and
 * `/` without the scaling and fix-up steps that only extreme operands need). mode 0: every float with bits in [first, first + count)
 * through sqrt_mid and sqrtf; mode 1: `count` pseudo-random operand pairs of the guarded range (all exponents, random and extreme
 * mantissas) through div_mid and `/`; mode 2: the one pair (x, s) in `first` (bits of x in the high word, of s in the low word; count = 1),
 * any operands at all, through div_mid and `/`. out2_device[0] += results whose bits differ, out2_device[1] = one such operand (pair). */
int eae_hip_debug_check_mid_forms(int mode, uint64_t first, uint64_t count, uint64_t seed, uint64_t* out2_device, void* stream);
/* What the last conv GEMM launch of the CALLING THREAD (eae_hip_conv5x5s2 / _tconv5x5s2, their _ws forms, eae_hip_conv5x5s2_latent)
 * launched, as the launcher wrote it down beside the launch itself -- not a second evaluation of its rules (tests/
 * test_gpu_launch_decisions.py holds every leaf of the decision at the size that reaches it). Up to `count` of these 11 words go to
 * `out` (host memory), in this order:
 *   [0] kernel family: 0 = no launch on this thread yet, 1 = block-cooperative LDS, 2 = wave kernel, 3 = split kernel
 *   [1] waves per block            [2] 32-channel tiles per wave (nt): 4 = whole position tiles with the fused epilogue, 2 / 1 = half
 *   / quarter tiles                [3] 1 = packed (four-wave blocks of channel parts)      [4] 1 = the last tiles are cut
 *   [5] resident waves per SIMD the cut was sized for (k), 0 when nothing is cut           [6] grid (blocks)   [7] threads per block
 *   [8] 1 = the normalisation follows as a pass of its own
 *   [9] eae_hip_conv5x5s2_latent: 1 = the latent stage ran as this launch's epilogue, 0 = as a launch of its own behind the
 *       convolution; -1 for every other entry point
 *   [10] tiles x phases as the launcher counted them, in the launched kernel's tile shape.
 * Returns the number of words written, or EAE_HIP_BAD_ARGUMENT (out NULL, count < 0). */
int eae_hip_debug_last_gemm_plan(int32_t* out, int count);
#endif /* EAE_TEST_HOOKS */

/* tls.cast_bt601 (tools.py:61-93) on its own: u8 = uint8(round_half_even(clip(x, 16, 235))). */
int eae_hip_cast_bt601(const float* x, uint8_t* out, int64_t count, void* stream);

/* tls.rgb_to_ycbcr (tools.py:1019-1083; how the dataset builders turn RGB photographs into the luminance images of the
 * path, datasets/kodak/kodak.py:70): rgb uint8 [count][3] -> ycbcr uint8 [count][3] and / or luma uint8 [count] (each
 * nullable), ITU-R BT.601 in float64, round half to even. Exact for all 2^24 inputs (tests/test_gpu_kernels.py). */
int eae_hip_rgb_to_ycbcr(const uint8_t* rgb, uint8_t* ycbcr, uint8_t* luma, int64_t count, void* stream);

/* Squared error per image for tls.psnr_2d (tools.py:873-875): sse[i] += sum (a - b)^2 over pixels_per_image. */
int eae_hip_sse_u8(const uint8_t* a, const uint8_t* b, uint64_t* sse, int n, int64_t pixels_per_image, void* stream);

/* ---- SVHN path, BASELINE.json configs[0] (svhn/eae/EntropyAutoencoder.py, svhn/eae/utils.py) ------------------------
 * The reference's pure-numpy FLOAT64 fully connected autoencoder 3072 -> 300 -> 200 -> 300 -> 3072, LeakyReLU(0.1).
 * All tensors row-major float64 on the device. Every dot product is one float64 FMA chain, k ascending from +0, bias
 * added afterwards (oracle/svhn_oracle.c runs the same chain; numpy.dot's BLAS order is unspecified). */

/* out[n][m] = act(x[n][:] . w[:][m] + b[m]); act = LeakyReLU(0.1) when leaky_relu != 0 (svhn/tools/tools.py:676-694).
 * One call per layer of `encoder` (EntropyAutoencoder.py:239-246) / `decoder` (:270-277). x: [n][k], w: [k][m]. */
int eae_hip_svhn_dense_f64(const double* x, const double* w, const double* b, double* out, int n, int k, int m,
                           int leaky_relu, void* stream);
/* preprocess_svhn (svhn/svhn/svhn.py:210): (uint8 - mean[j]) / std. images: [n][d] uint8, mean: [d]. */
int eae_hip_svhn_preprocess(const uint8_t* images, const double* mean, double std_training, double* out, int n, int d,
                            void* stream);
/* tls.quantization (svhn/tools/tools.py:1095): q = bw * round_half_even(y / bw) with ONE scalar bin width, plus the
 * int32 symbols round(q / bw) behind tls.count_symbols / discrete_entropy (:214-231, :289-). q and symbols nullable.
 * checks[2] (caller zeroes): [0] symbols outside int32 (NaN and +-inf included), [1] |q - y| >= 1.5e-10 ("The quantization
 * was omitted.", tools.py:214-217, when y is passed as already quantised; NaN and +-inf pass that numpy assertion and are not
 * counted). */
int eae_hip_svhn_quantize_f64(const double* y, double bin_width, double* q, int32_t* symbols, uint32_t* checks,
                              int64_t count, void* stream);
/* minmax[0] = min(minmax[0], min symbols), minmax[1] = max(...): caller initialises to (INT32_MAX, INT32_MIN). */
int eae_hip_svhn_symbol_range(const int32_t* symbols, int64_t count, int32_t* minmax, void* stream);
/* hist[s - lowest] += 1 for lowest <= s < lowest + nb_bins, *overflow += 1 otherwise (caller zeroes both). */
int eae_hip_svhn_symbol_histogram(const int32_t* symbols, int64_t count, int32_t lowest, int32_t nb_bins, uint32_t* hist,
                                  uint32_t* overflow, void* stream);
/* utils.py:71-74: uint8(round_half_even(clip(rec*std + mean[j], 0, 255))) (tools.py:166) and, with ref_u8 + sse, the
 * squared error per image behind tls.mean_psnr (tools.py:857-859). sse[i] is overwritten. */
int eae_hip_svhn_postprocess(const double* reconstruction, double std_training, const double* mean, uint8_t* out_u8,
                             const uint8_t* ref_u8, uint64_t* sse, int n, int d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EAE_HIP_H */
