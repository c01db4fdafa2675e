/*
 * splitvae.h -- C ABI of libsplitvae_hip.so: the MI355X (gfx950) SPLIT-VAE training path.
 *
 * The reference (51616/split-vae) has no FFI/plugin layer: its hot path is Python calling
 * TensorFlow-2.0 library kernels.  Every entry point below therefore cites the reference *call
 * site(s)* whose TF op sequence it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain C, raw DEVICE pointers + explicit sizes, `stream` is a hipStream_t passed as void*;
 *   - the caller owns every buffer including the workspace; no entry point allocates device
 *     memory, synchronises the host, or keeps global mutable state (plans are caller-owned);
 *   - return 0 on success, <0 = sv_status error, >0 = a hipError_t from a launch;
 *   - activations are NHWC; conv kernels HWIO fp32; dense kernels [in,out] fp32 (Keras layouts);
 *   - `dtype` selects the arithmetic type of the MFMA contractions (SV_BF16: bf16 operands,
 *     fp32 accumulate; SV_F32: exact fp32 MFMA).  Master weights, ELBO terms, KL, Adam are fp32.
 */
#ifndef SPLITVAE_H
#define SPLITVAE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { SV_OK = 0, SV_E_BADARG = -1, SV_E_UNSUPPORTED = -2, SV_E_WORKSPACE = -3, SV_E_STATE = -4 } sv_status;
typedef enum { SV_F32 = 0, SV_BF16 = 1 } sv_dtype;
typedef enum { SV_ACT_NONE = 0, SV_ACT_RELU = 1, SV_ACT_ELU = 2 /* pointwise kernels of the GMVAE encoder only */ } sv_act;

const char* sv_version(void);

/* Fixed-order reductions for every launch that FOLLOWS: 1 = on (no split-K / m-split fp32 atomics anywhere: same inputs twice ->
 * identical bits; SURVEY section 5's determinism test), 0 = off (the faster atomics-ordered dense layers), -1 = what the environment
 * variable SV_DETERMINISTIC said at load time (the default).  Host-side, per launch: plans, workspaces and prepared weights do not
 * depend on it.  The reference has no such switch (TF-2.0 GPU kernels are nondeterministic, no seed is set anywhere: SURVEY 0);
 * the parity tests use it to compare against the oracle at the bounds of SURVEY 8c without a summation-order allowance. */
int sv_set_deterministic(int32_t mode);
int sv_get_deterministic(void);

/* ---------------------------------------------------------------- A1: patch scramble
 * Replaces Augmentator.scramble (augmentation.py:43-57) as wired at vae/main.py:54-61:
 * extract_patches -> reshape -> shuffle -> split/unstack/concat -> concat([x, x_aug], axis=2).
 * x[B,H,W,3] fp32, perm[B,(H/patch)*(W/patch)] int32 (destination patch n takes source patch
 * perm[n]); images6[B,H,W,6] fp32 = [x | x_aug].  Pure index bookkeeping: bit-exact. */
int sv_scramble_gather(const float* x, const int32_t* perm, float* images6,
                       int32_t B, int32_t H, int32_t W, int32_t patch, void* stream);
/* The same, also writing the two zero-padded 8-channel NHWC tensors (x | x_aug, sv_dtype `dtype`) the first encoder layers of
 * sv_lgvae_step read -- pass the plan's in8_x / in8_xh buffers (sv_lgvae_buffer) and SV_PHASE_INPUTS_STAGED to the step: images6 is
 * read once less and the step's split / pad pass drops out (vae/main.py:57-61 + vae/model.py:190 in one kernel).  x8 and xh8 are
 * stored 16 bytes at a time: SV_E_BADARG for either not 16-byte aligned. */
int sv_scramble_gather_staged(const float* x, const int32_t* perm, float* images6, void* x8, void* xh8, int32_t dtype, int32_t B,
                              int32_t H, int32_t W, int32_t patch, void* stream);
/* tf.random.shuffle (augmentation.py:49) stand-in: one uniform permutation per image from a
 * counter-based Philox stream keyed by (seed, step, global sample index = sample_offset + b),
 * so 1-GPU and N-GPU runs draw identical permutations.  n_patch <= 4096. */
int sv_random_perm(int32_t* perm, int32_t B, int32_t n_patch, uint64_t seed, uint64_t step,
                   int64_t sample_offset, void* stream);

/* ---------------------------------------------------------------- A1b: blur, high/low pass, mixed-size scramble
 * The other augmentations of Augmentator (augmentation.py:12-30), per image in fp32 NHWC, batched on the device.
 * Gaussian filter (augmentation.py:33-38, :83-101): low = depthwise cross-correlation of pad(x, r, SYMMETRIC) with
 * K = outer(v, v) / sum(outer(v, v)), v = Normal(mean, std).prob(-r..r), VALID -- run separably (row pass, column pass) in
 * fp32 with the taps formed in fp32, every sum in one fixed order (bit-reproducible).  SYMMETRIC mirrors including the edge
 * pixel (-1 -> 0, H -> H-1).  All filter entries: SV_E_BADARG for a null pointer or B, H, W <= 0 or a radius < 0;
 * SV_E_UNSUPPORTED for H != W, a radius > H or > 64, (2r+1)*W*24 bytes above the 64 KiB of LDS a workgroup stages, or
 * B > 65535 (the image index is the grid's y dimension).
 * The _staged forms also write the plan's in8_x / in8_xh (channels 0-2 and 3-5, zero padded to 8, sv_dtype `dtype`):
 * the contract of sv_scramble_gather_staged, passed to the step as SV_PHASE_INPUTS_STAGED.  x8 and xh8 are stored 16 bytes at
 * a time: a pointer that is not 16-byte aligned is SV_E_BADARG (this holds for sv_scramble_gather_mixed_staged too). */
/* gaussian_blur (augmentation.py:83-94): images6[B,H,W,6] = [x | blur(x)], radius[B] int32 and std[B] fp32 device arrays
 * (sv_blur_params draws them); a radius outside [0, max_radius] is clamped to it. */
int sv_gauss_blur(const float* x, const int32_t* radius, const float* std, float* images6, int32_t B, int32_t H, int32_t W,
                  int32_t max_radius, void* stream);
int sv_gauss_blur_staged(const float* x, const int32_t* radius, const float* std, float* images6, void* x8, void* xh8, int32_t dtype,
                         int32_t B, int32_t H, int32_t W, int32_t max_radius, void* stream);
/* high_low_pass (augmentation.py:23-28, :97-101): one fixed kernel of radius `size` (--patch_size), Normal(mean, std);
 * images9[B,H,W,9] = [x | x - low | low].  std <= 0: SV_E_BADARG. */
int sv_high_low_pass(const float* x, float* images9, int32_t B, int32_t H, int32_t W, int32_t size, float mean, float std,
                     void* stream);
int sv_high_low_pass_staged(const float* x, float* images9, void* x8, void* xh8, int32_t dtype, int32_t B, int32_t H, int32_t W,
                            int32_t size, float mean, float std, void* stream);
/* augmentation.py:86-87: radius[b] ~ U{3,4,5,6}, std[b] ~ U[5,10), from the Philox stream keyed by (seed, step, global sample
 * index = sample_offset + b) like sv_random_perm: a shard at sample_offset draws the rows of the single-process batch. */
int sv_blur_params(int32_t* radius, float* std, int32_t B, uint64_t seed, uint64_t step, int64_t sample_offset, void* stream);
/* augmentation.py:40-41,65 (np.random.choice([1, 2, 4, 8])): sizes[b] for the per-image mixed scramble, keyed as above. */
int sv_mix_sizes(int32_t* sizes, int32_t B, uint64_t seed, uint64_t step, int64_t sample_offset, void* stream);
/* The same draw on the host, for (seed, step, sample): the one patch size of a whole pipeline (the reference draws it once,
 * when Dataset.map traces mix_scramble).  Needs no device. */
int32_t sv_mix_size_host(uint64_t seed, uint64_t step, int64_t sample);
/* mix_scramble's tf.random.shuffle (augmentation.py:74) with a size per image: row b of perm (row stride ld) is the
 * sv_random_perm permutation of (H/sizes[b])^2 patches, same keys.  sizes[b] must divide H with (H/sizes[b])^2 <= min(ld, 4096);
 * a row whose size does not is left unwritten.  SV_E_BADARG for a null pointer or B, H, ld <= 0. */
int sv_random_perm_mixed(int32_t* perm, const int32_t* sizes, int32_t B, int32_t H, int32_t ld, uint64_t seed, uint64_t step,
                         int64_t sample_offset, void* stream);
/* mix_scramble's gather (augmentation.py:70-81) with a size per image: images6[B,H,W,6] = [x | x_aug], the patches of image b
 * sizes[b] square, perm as sv_random_perm_mixed writes it.  An image whose size is invalid (see above) or whose permutation
 * entry is out of range copies x through.  SV_E_BADARG for a null pointer or sizes <= 0; SV_E_UNSUPPORTED for H != W. */
int sv_scramble_gather_mixed(const float* x, const int32_t* perm, const int32_t* sizes, int32_t ld, float* images6, int32_t B,
                             int32_t H, int32_t W, void* stream);
int sv_scramble_gather_mixed_staged(const float* x, const int32_t* perm, const int32_t* sizes, int32_t ld, float* images6, void* x8,
                                    void* xh8, int32_t dtype, int32_t B, int32_t H, int32_t W, void* stream);

/* ---------------------------------------------------------------- A1c: Multi-Bird canvas synthesis
 * Replaces MultiCUB.create_dataset / create_sample (spair/data.py:39-174) for the two datasets create_cub_tfrec builds
 * (:229-255): 48 x 48 x 3 canvases in [0,1] with 0..5 hard-masked 14 x 14 sprites on a solid colour or on a rotated
 * 6-pixel checkerboard.  Canvas `sample` of `split` is a pure function of (seed, split, sample): every draw is one
 * Philox4x32-10 block with counter (sample, split, kind | object | try), so nothing is stored and shards agree.
 * `bg` names the background AND its colour table (spair/data.py:52-57). */
typedef enum { SV_MB_SOLID_FIXED = 0, SV_MB_UNSEEN_SOLID_FIXED = 1, SV_MB_CKB_ROT_6 = 2, SV_MB_UNSEEN_CKB_ROT_6 = 3 } sv_multibird_bg;
/* Everything random about one canvas.  count: objects placed, 0..5 (uniform; :166).  row[k], col[k] in 0..33 (np.random.randint(0, 34),
 * :127-131; rand_x indexes axis 0 = rows), redrawn until no earlier box is overlapped by more than 15 % -- for 14-wide boxes:
 * ix = max(0, 14 - |row_a - row_b|), iy likewise, reject iff ix * iy >= 30.  sprite[k] in 0..n_sprites-1.  colour[0..1]: indices
 * into the table of `bg` (solid: colour[1] == colour[0]; checkerboard: an ordered pair of distinct colours).  angle: fp32 in
 * [-pi/2, pi/2), 0 on the solid backgrounds.  Entries k >= count are -1.
 * The rejection loop is capped at 4096 tries per object: on reaching the cap that object and all later ones are dropped, count
 * is the number actually placed and max_tries is 4096; otherwise max_tries is the largest (0-based) try number accepted. */
typedef struct { int32_t count, row[5], col[5], sprite[5], colour[2], max_tries; float angle; } sv_multibird_layout;
/* The plain sequential loop on the host; needs no device.  SV_E_BADARG: out NULL or n_sprites <= 0; SV_E_UNSUPPORTED: a bg
 * outside sv_multibird_bg or n_sprites > 2^20.  (The same two rules hold for the device entries below.) */
int sv_multibird_layout_host(sv_multibird_layout* out, int32_t bg, int32_t n_sprites, uint64_t seed, int32_t split, int64_t sample);
/* out[B] on the device, one wave per canvas: lane l tests try 64 r + l and the ballot's lowest bit picks the first accepted try,
 * the one the host loop accepts -- bit for bit the host's layouts.  index[B] int64 device sample numbers, or NULL: sample_offset + b.
 * SV_E_BADARG: out NULL or B <= 0. */
int sv_multibird_layouts(sv_multibird_layout* out, const int64_t* index, int32_t bg, int32_t n_sprites, int32_t B, uint64_t seed,
                         int32_t split, int64_t sample_offset, void* stream);
/* x[B,48,48,3] fp32 canvases (16-byte aligned) and, unless NULL, count[B] fp32 = the layouts' counts (the label test_step takes).
 * sprites[n_sprites,14,14,3] uint8 on the device (4-byte aligned), zero outside the object.  layouts NULL: drawn in the same
 * launch as sv_multibird_layouts draws them; a pointer pins them (counts are clamped to 0..5, a sprite id outside the bank pastes
 * nothing).  Background: colour / 255, or the 192 x 192 board of 6-pixel cells rotated by `angle` about its centre with bilinear
 * interpolation (tfa.image.rotate's transform) and cropped to its central quarter (:89-105), sampled analytically.  Sprites in
 * object order, later ones on top; a sprite pixel replaces the canvas iff max(r,g,b) > 0, value v / 255 in correctly rounded
 * fp32 (= np.float32(v / 255.0)).  Every output element is written exactly once; no workspace.
 * SV_E_BADARG: x or sprites NULL or misaligned, B <= 0. */
int sv_multibird_canvases(float* x, float* count, const uint8_t* sprites, int32_t n_sprites, const int64_t* index,
                          const sv_multibird_layout* layouts, int32_t bg, int32_t B, uint64_t seed, int32_t split,
                          int64_t sample_offset, void* stream);

/* ---------------------------------------------------------------- A1d: device-resident datasets
 * The batch fetch of vae/main.py:56-61 (shuffle -> batch) over a training set that stays in device memory: src[N,H,W,3] is
 * the whole set, uint8 (SVHN's pixel levels) or fp32 (the CelebA files' images), index[B] int32 the batch's rows on the
 * device.  A uint8 level v becomes lut[v]: lut[256] fp32 on the device, filled by the host with vae/data.py:52's
 * (v / 255.0 * 2 - 1) in float64 rounded once, so the fetch is bit for bit the host's normalisation; fp32 sources are
 * copied (lut may be NULL).  An index outside [0, N) is clamped to it: nothing is read outside src (the host layer refuses
 * such an index before upload).  No atomics, no workspace, every output element written exactly once.
 * All three image entries: SV_E_BADARG for a null pointer (lut only for uint8), N, B, H or W <= 0, a src_dtype outside
 * sv_src_dtype, or a src / output pointer that is not 16-byte aligned; SV_E_UNSUPPORTED for B > 65535 or H * W * 3 >= 2^30. */
typedef enum { SV_SRC_U8 = 0, SV_SRC_F32 = 1 } sv_src_dtype;
/* x[B,H,W,3] fp32, x[b] = value(src[index[b]]). */
int sv_dataset_gather(const void* src, int32_t src_dtype, const float* lut, const int32_t* index, float* x, int32_t N, int32_t B,
                      int32_t H, int32_t W, void* stream);
/* The same fetch fused with the patch scramble and the step's input staging: bit for bit sv_dataset_gather followed by
 * sv_scramble_gather_staged (perm, patch, images6, x8, xh8, dtype as there) without the intermediate x.  x8 = xh8 = NULL:
 * images6 only (sv_scramble_gather).  A perm entry outside [0, (H/patch)^2) is clamped.  Also SV_E_BADARG: patch <= 0, one of
 * x8 / xh8 NULL and the other not, a dtype outside sv_dtype when they are given; SV_E_UNSUPPORTED: H != W, H % patch != 0, or
 * a uint8 image above 57 KiB (it is staged in LDS; 128 x 128 is 48 KiB). */
int sv_dataset_gather_scramble(const void* src, int32_t src_dtype, const float* lut, const int32_t* index, const int32_t* perm,
                               float* images6, void* x8, void* xh8, int32_t dtype, int32_t N, int32_t B, int32_t H, int32_t W,
                               int32_t patch, void* stream);
/* labels[N] uint8 on the device -> out[B,depth] fp32 = one_hot(labels[index[b]] - 1, depth) (vae/data.py:55-57: SVHN's
 * label 10, the digit 0, lands on the last index); a label outside 1..depth gives an all-zero row (tf.one_hot).
 * SV_E_BADARG: a null pointer, N, B or depth <= 0. */
int sv_dataset_onehot(const uint8_t* labels, const int32_t* index, float* out, int32_t N, int32_t B, int32_t depth, void* stream);

/* ---------------------------------------------------------------- A6: discretised logistic NLL
 * Replaces discretised_logistic_loss (vae/trainer.py:21-38) + reduce_sum[1,2,3] (:127-128) and,
 * when grad != NULL, its adjoint under tape.gradient (:137).
 * images6[B,H,W,6] fp32; channels [ch_off, ch_off+3) are the targets (0: x, 3: x_hat).
 * out6[B,H,W,6] fp32 decoder head: ch 0-2 mean, 3-5 log_scale (vae/model.py:169).
 * nll[B] fp32 per-image sums.  grad[B,H,W,8] (dtype) = d(mean_b nll)/d(out6) * grad_scale in
 * ch 0-5, zeros in ch 6-7 (the padded layout the conv dgrad/wgrad kernels consume). */
int sv_dlogistic_nll(const float* images6, int32_t ch_off, const float* out6, float* nll,
                     void* grad, int32_t grad_dtype, float grad_scale,
                     int32_t B, int32_t H, int32_t W, float* partial_ws, void* stream);
int64_t sv_dlogistic_nll_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* The x and the x-hat reconstruction in one launch, as the plan calls it (for tests and host bindings): network e reads channels [3e, 3e+3)
 * of images6 and its buffers lie e strides behind the given pointers -- out6 + e*zs_out, nll + e*zs_nll, grad + e*zs_grad, partial_ws +
 * e*zs_part, strides in ELEMENTS of the buffer's type.  grad NULL: no gradients.  partial_ws holds 2 * sv_dlogistic_nll_workspace_bytes.
 * The same bits as two sv_dlogistic_nll calls.  SV_E_BADARG: a null images6 / out6 / nll / partial_ws, B, H or W <= 0, a stride shorter than
 * one network's buffer, an odd zs_out, images6 / out6 not 8-byte aligned; with grad: a dtype outside sv_dtype, grad not 16-byte aligned or
 * zs_grad no multiple of the elements of 16 bytes. */
int sv_dlogistic_nll_twin(const float* images6, const float* out6, int64_t zs_out, float* nll, int64_t zs_nll, void* grad, int64_t zs_grad,
                          int32_t grad_dtype, float grad_scale, int32_t B, int32_t H, int32_t W, float* partial_ws, int64_t zs_part,
                          void* stream);
/* The step's loss finaliser (vae/trainer.py:127-135, :140-144), as the plan calls it (for tests and host bindings).  Per-image terms nll_x,
 * nll_xh, kl_x, kl_xh [B] -> losses[6] = batch means {x_recon, x_kl, x_hat_recon, x_hat_kl, beta (x_kl + x_hat_kl), x_recon + x_hat_recon +
 * total_kl}; a NULL nll_xh / kl_x / kl_xh counts as zeros (a one-branch model).  part_x [B][P] (and part_xh) given: nll_x (nll_xh) is first
 * WRITTEN as the index-order sum of its P partials.  accumulate != 0: metric_acc[0..4] += losses[0..4], metric_acc[5] += 1.
 * SV_E_BADARG: a null nll_x / losses, B <= 0, accumulate without metric_acc, part_xh without part_x, with part_x: P <= 0, or part_xh given
 * and nll_xh not (or the reverse). */
int sv_finalize_losses(float* nll_x, float* nll_xh, const float* kl_x, const float* kl_xh, const float* part_x, const float* part_xh,
                       int32_t P, int32_t B, float beta, float* losses, float* metric_acc, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------- A4+A7: reparameterise + KL
 * Replaces Sampling.call (vae/model.py:9-13), the Dense bias/softplus epilogues of e4_mean/e4_sd
 * (:41-42,:111-112) and kl_divergence (vae/trainer.py:11-15).
 * pre[B,2L] fp32 = [f@W_mean | f@W_sd] WITHOUT bias; bias[2L]; eps[B,L] (NULL: drawn from Philox
 * keyed by (seed, step, stream_id, sample_offset+b, j) and written to eps_out).
 * Outputs: z_mean,z_sig,z [B,L] fp32; z_lp (dtype) [B, ldz] at column z_col (decoder input,
 * the tf.concat of vae/model.py:197 is this write); kl[B] = -1/2 sum_j(1+log sig^2-mu^2-sig^2). */
int sv_reparam_kl_fwd(const float* pre, const float* bias, const float* eps, float* eps_out,
                      float* z_mean, float* z_sig, float* z, void* z_lp, int32_t z_dtype,
                      int32_t ldz, int32_t z_col, float* kl, int32_t B, int32_t L,
                      uint64_t seed, uint64_t step, int32_t stream_id, int64_t sample_offset,
                      void* stream);
/* Adjoint: dz[B,L] fp32 (ld_dz, optional second addend dz2) -> g_pre[B,2L] (dtype) =
 * [dz + kl_scale*mu | (dz*eps + kl_scale*(sig-1/sig)) * (1-exp(-sig))]; kl_scale = beta/B. */
int sv_reparam_kl_bwd(const float* dz, int32_t ld_dz, const float* dz2, int32_t ld_dz2,
                      const float* z_mean, const float* z_sig, const float* eps, float kl_scale,
                      void* g_pre, int32_t g_dtype, int32_t B, int32_t L, void* stream);

/* ---------------------------------------------------------------- K14: Keras Adam
 * Replaces tf.keras.optimizers.Adam(lr).apply_gradients (vae/main.py:65, vae/trainer.py:138):
 * alpha=lr*sqrt(1-b2^t)/(1-b1^t); m+=(g-m)(1-b1); v+=(g*g-v)(1-b2); p-=alpha*m/(sqrt(v)+eps).
 * One launch over the flat parameter buffer; g is multiplied by grad_scale first (1/world). */
int sv_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                 float beta2, float eps, int64_t t, float grad_scale, void* stream);

/* The same with Keras `clipnorm` (SPLIT-SPAIR: Adam(..., clipnorm=1.0), spair/main.py:109): every gradient tensor is scaled by
 * clipnorm / max(||g * grad_scale||_2, clipnorm) first (tf.clip_by_norm).  tensor_off: DEVICE array of n_tensors+1 element
 * offsets into the flat buffers; norm_ws: DEVICE scratch of 256*n_tensors floats.  Deterministic (fixed-order norms). */
int sv_adam_step_clipnorm(float* p, const float* g, float* m, float* v, const int64_t* tensor_off, int32_t n_tensors,
                          float* norm_ws, float clipnorm, float lr, float beta1, float beta2, float eps, int64_t t,
                          float grad_scale, void* stream);

/* hipGraph-replay form: the step size alpha = lr*sqrt(1-b2^t)/(1-b1^t) is read from DEVICE memory (alpha_dev, one float the
 * caller refreshes before each replay with sv_adam_alpha(lr, beta1, beta2, t)); alpha_dev == NULL = the call above. */
int sv_adam_step_clipnorm_dyn(float* p, const float* g, float* m, float* v, const int64_t* tensor_off, int32_t n_tensors,
                              float* norm_ws, float clipnorm, float lr, float beta1, float beta2, float eps, int64_t t,
                              const float* alpha_dev, float grad_scale, void* stream);
float sv_adam_alpha(float lr, float beta1, float beta2, int64_t t);
/* The same over SEPARATE gradient tensors: grads = HOST array of n_tensors (<= 128) DEVICE pointers, 16-byte aligned, tensor i
 * holding tensor_off[i+1] - tensor_off[i] floats.  The addresses are passed to the kernels by value: no flat copy of the
 * gradients, and a captured hipGraph stays valid while the tensors keep their addresses.  alpha_dev may be NULL. */
int sv_adam_step_clipnorm_ptrs(float* p, const float* const* grads, float* m, float* v, const int64_t* tensor_off, int32_t n_tensors,
                               float* norm_ws, float clipnorm, float lr, float beta1, float beta2, float eps, int64_t t,
                               const float* alpha_dev, float grad_scale, void* stream);

/* ---------------------------------------------------------------- K10a: bilinear 2x
 * Replaces tf.image.resize(x,[2H,2W]) (vae/model.py:163,:165,:167; bilinear, half-pixel centres,
 * edge clamp) and its adjoint (ResizeBilinearGrad) fused with the ReLU mask of the producer. */
int sv_upsample2x_fwd(const void* in, void* out, int32_t dtype, int32_t B, int32_t H, int32_t W,
                      int32_t C, void* stream);
int sv_upsample2x_bwd(const void* g_hi, const void* y_lo_mask, void* g_lo, int32_t dtype,
                      int32_t B, int32_t H, int32_t W, int32_t C, void* stream);

/* ---------------------------------------------------------------- SPLIT-SPAIR: spatial transformer (fp32)
 * Replaces spair.utils.STN.call + bilinear_sampler + get_pixel_value (spair/utils.py:119-200, :202-272, :274-330) and the
 * gradient tape.gradient takes through them.  z_where [B,Hc,Wc,4] pre-activations; inverse = 0: img [B,H,W,C] -> one
 * [Ho,Wo,C] glimpse per cell, out [B,Hc*Wc,Ho,Wo,C]; inverse = 1 (the renderer's STN): img [B,Hc*Wc,H,W,C] -> each object
 * pasted on its own [Ho,Wo,C] canvas.  bbox (may be NULL) = obj_bbox_mask [B,Hc*Wc,4].  Backward: g_z_where [B,Hc,Wc,4] and
 * g_img (same shape as img; may be NULL when the image takes no gradient).  g_img is scatter-ADDED with atomics -- zero it
 * first -- unless sv_stn_bwd_overwrites(H, W, C, inverse) is 1 (inverse form, small objects: each cell's gradient is
 * accumulated in LDS and stored whole). */
int sv_stn_sample_fwd(const float* img, const float* z_where, float* out, float* bbox, int32_t B, int32_t Hc, int32_t Wc,
                      int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t inverse, void* stream);
int sv_stn_bwd_overwrites(int32_t H, int32_t W, int32_t C, int32_t inverse);
int sv_stn_sample_bwd(const float* img, const float* z_where, const float* g_out, float* g_img, float* g_z_where, int32_t B,
                      int32_t Hc, int32_t Wc, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t inverse,
                      void* stream);

/* SPLIT-SPAIR: Renderer.call (spair/spair.py:534-579), fp32.  obj [B,B',H,W,C+1] = every object's rgb + alpha on its own
 * canvas (sv_stn_sample_fwd, inverse = 1), bg [B,H,W,C], z_depth / z_pres / z_pres_logits [B,B'] -> out [B,H,W,C]; B' <= 16,
 * C <= 4.  training != 0: z_pres as given and `noise` [B,B',H,W,C] (the GaussianNoise(0.01) draw, may be NULL) added to the
 * object images before their clip; training == 0: z_pres = max(round(sigmoid(z_pres_logits)), 1e-8), noise must be NULL.
 * Backward (training form): g_obj like obj, g_bg like bg, g_z_pres / g_z_depth [B,B'] (all written, none accumulated). */
int sv_spair_render_fwd(const float* obj, const float* bg, const float* z_depth, const float* z_pres,
                        const float* z_pres_logits, const float* noise, float* out, int32_t B, int32_t Bp, int32_t H,
                        int32_t W, int32_t C, int32_t training, void* stream);
int sv_spair_render_bwd(const float* obj, const float* bg, const float* z_depth, const float* z_pres, const float* noise,
                        const float* g_out, float* g_obj, float* g_bg, float* g_z_pres, float* g_z_depth, int32_t B,
                        int32_t Bp, int32_t H, int32_t W, int32_t C, void* stream);

/* The same with a workspace of sv_spair_render_bwd_workspace_floats(B, H, W) floats: a workgroup per 256-pixel chunk instead of
 * one per image (288 instead of 32 workgroups at batch 32); the chunks' partial g_z sums are added in chunk order (deterministic). */
int64_t sv_spair_render_bwd_workspace_floats(int32_t B, int32_t H, int32_t W);
int sv_spair_render_bwd_ws(const float* obj, const float* bg, const float* z_depth, const float* z_pres, const float* noise,
                           const float* g_out, float* g_obj, float* g_bg, float* g_z_pres, float* g_z_depth, int32_t B,
                           int32_t Bp, int32_t H, int32_t W, int32_t C, float* ws, int64_t ws_floats, void* stream);

/* SPLIT-SPAIR: compute_z_pres_kl_yolo_air + concrete_binary_sample_kl (spair/trainer.py:28-42, :45-94), fp32: the sequential
 * count-prior KL of the n_cells <= 16 presence variables, cells in raster order.  z_pres / z_pres_logits / z_pres_pre_sigmoid
 * [B,n_cells] -> kl [B] (per-image sums: tf_mean_sum = their batch mean); g_pre_sigmoid / g_logits (may be NULL) =
 * grad_scale * d kl_b / d input (the prior depends on the thresholded samples only: no gradient to z_pres). */
int sv_spair_zpres_kl(const float* z_pres, const float* z_pres_logits, const float* z_pres_pre_sigmoid, float* kl,
                      float* g_pre_sigmoid, float* g_logits, int32_t B, int32_t n_cells, float prior_prob, float temperature,
                      float grad_scale, void* stream);

/* hipGraph-replay form: prior_prob_dev (may be NULL) = one DEVICE float that overrides prior_prob (the prior anneals with the
 * step, spair/trainer.py:153). */
int sv_spair_zpres_kl_dyn(const float* z_pres, const float* z_pres_logits, const float* z_pres_pre_sigmoid, float* kl,
                          float* g_pre_sigmoid, float* g_logits, int32_t B, int32_t n_cells, float prior_prob,
                          const float* prior_prob_dev, float temperature, float grad_scale, void* stream);

/* SPLIT-SPAIR: the per-image loss sums of spair/trainer.py with their gradients, fp32, one launch each (spair_loss.hip):
 *   mode 0: xent_loss :103-104, a = label, b = prediction;  mode 1: kl_divergence :13-21, a = z_mean, b = z_sig;
 *   mode 2: kl_divergence_two_gauss :23-24 against the constant prior N(prior_mean, prior_sig) (:156-157), a = mean, b = sig.
 * a, b [B,n] -> sums [B] (tf_mean_sum :107-109 = their batch mean); ga / gb [B,n] (may be NULL) = the per-element derivatives
 * (mode 0: ga is ignored).  tf_safe_log :97-101 semantics (log(v + 1e-8); NaN / inf -> -100, no gradient). */
int sv_spair_loss(int32_t mode, const float* a, const float* b, float* sums, float* ga, float* gb, int32_t B, int32_t n,
                  float prior_mean, float prior_sig, void* stream);
/* hipGraph-replay form: prior_mean_dev (may be NULL) = one DEVICE float that overrides prior_mean (mode 2: the zoom prior
 * anneals with the step, spair/trainer.py:156). */
int sv_spair_loss_dyn(int32_t mode, const float* a, const float* b, float* sums, float* ga, float* gb, int32_t B, int32_t n,
                      float prior_mean, const float* prior_mean_dev, float prior_sig, void* stream);

/* SPLIT-SPAIR evaluation (spair_eval.hip), fp32, plain loads and stores, no atomics (same inputs -> same bits).  Every argument is
 * checked before anything is enqueued: SV_E_BADARG leaves all outputs untouched.
 *
 * tf.image.draw_bounding_boxes as spair/visualizer.py:107-111 calls it (boxes = obj_bbox_mask * z_pres, one white colour).
 * images / out [B,H,W,C], C in {1,3,4}; out may alias images.  boxes [B,NB,4] = (ymin, xmin, ymax, xmax) in [0,1] coordinates
 * (obj_bbox_mask's layout); gate [B,NB] (may be NULL) multiplies each box first.  colors [NC,ldc], ldc >= C: box bb takes row
 * bb % NC and its first C components are written as they are (no blending).  TF's rules: in fp32, r0 = (int64)(ymin * (H-1)),
 * r1 = (int64)(ymax * (H-1)), c0 / c1 the same with xmin / xmax and W (truncation toward zero; NaN or beyond the int64 range ->
 * INT64_MIN, as on x86); a box with r0 > r1 or c0 > c1 (inverted) or r0 >= H, r1 < 0, c0 >= W or c1 < 0 (outside) is skipped;
 * the top edge (row r0) is drawn if r0 >= 0, the bottom (row r1) if r1 < H, both over the columns [c0, c1] clamped to the image;
 * the left (column c0) if c0 >= 0, the right (column c1) if c1 < W, both over the clamped rows.  Boxes are drawn in index order:
 * where outlines overlap, the highest-index box wins.  As in TF, a gated-off box becomes (0,0,0,0) and colours pixel (0,0).
 * Every other pixel of out is a copy of images.  SV_E_BADARG: a null images / boxes / colors / out, B, H, W, NB or NC <= 0, C not in
 * {1,3,4}, ldc < C; SV_E_UNSUPPORTED: H * W >= 2^31 - 256 or B > 65535. */
int sv_draw_bounding_boxes(const float* images, const float* boxes, const float* gate, const float* colors, float* out, int32_t B,
                           int32_t H, int32_t W, int32_t C, int32_t NB, int32_t NC, int32_t ldc, void* stream);

/* The object-count metrics of test_step (spair/trainer.py:292-301), one launch, no host synchronisation.  z_pres_logits [B,ncell]
 * with row pitch ld >= ncell, labels [B] -> pred[b] = sum over the cells, in cell order, of rint(sigmoid(logit)) (fp32 sigmoid, round
 * half to even as tf.round: a logit of exactly 0 is not counted), written when pred != NULL; metrics[2] = (MAE, MAPE) of the batch:
 * mean |label - pred| (tf.metrics.mean_absolute_error) and 100 * mean(|label - pred| / max(|label|, 1e-7))
 * (mean_absolute_percentage_error, Keras epsilon); acc (may be NULL) int32[2] += (number of images with pred == label, B): the
 * state of tf.keras.metrics.Accuracy (count_acc_test, :132, :301), result = acc[0] / acc[1] (0 when acc[1] == 0).  Zero acc once per
 * test set.  SV_E_BADARG: a null z_pres_logits / labels / metrics, B or ncell <= 0, ld < ncell. */
int sv_spair_count_metrics(const float* z_pres_logits, int32_t ld, const float* labels, float* pred, float* metrics, int32_t* acc,
                           int32_t B, int32_t ncell, void* stream);

/* Detection average precision on Multi-Bird canvases (detect_ap.hip; DESIGN.md 4.20 pins the definitions; no reference
 * counterpart: spair/data.py drops the positions).  Plain loads and stores, no atomics, one fixed order for every sum: the same
 * inputs give the same bits.  Every argument is checked before anything is enqueued.  Boxes are (ymin, xmin, ymax, xmax),
 * normalised to the canvas (obj_bbox_mask's convention).
 *
 * Sprite extents: out[s] = (r0, c0, r1, c1), the inclusive tight bounds of the pixels of sprite s of bank [n,14,14,3] uint8 with
 * max(r,g,b) > 0 (the renderer's mask rule); four -1 for an all-zero sprite.  SV_E_BADARG: a null pointer, n <= 0;
 * SV_E_UNSUPPORTED: n > 2^20.  The _host entry is the same arithmetic in a plain loop; it needs no device. */
int sv_sprite_extents_host(const uint8_t* bank, int32_t n, int32_t* out /* [n][4] */);
int sv_sprite_extents(const uint8_t* bank, int32_t n, int32_t* out /* [n][4] */, void* stream);
/* Ground truth of B canvases: for each k < count (clamped to 0..5) whose sprite[k] is inside the bank and has extents, the box
 * ((row + r0) / 48, (col + c0) / 48, (row + r1 + 1) / 48, (col + c1 + 1) / 48) in correctly rounded fp32 -- the sprite's full
 * extent, occluded or not -- packed in object order into boxes[b][0 .. n_gt[b] - 1]; the remaining slots are zero.
 * SV_E_BADARG: a null or misaligned pointer, n_sprites or B <= 0; SV_E_UNSUPPORTED: n_sprites > 2^20. */
int sv_multibird_gt_boxes_host(const sv_multibird_layout* layouts, const int32_t* extents, int32_t n_sprites, float* boxes /* [B][5][4] */,
                               int32_t* n_gt /* [B] */, int32_t B);
int sv_multibird_gt_boxes(const sv_multibird_layout* layouts, const int32_t* extents, int32_t n_sprites, float* boxes /* [B][5][4] */,
                          int32_t* n_gt /* [B] */, int32_t B, void* stream);
/* Matching of B images of `cells` cells (1..64) against their ground truth.  bbox: image b's cells at bbox + b * ld_bbox, four
 * floats a cell (ld_bbox >= 4 * cells, in floats); logits: image b's at logits + b * ld_logits (ld_logits >= cells); gt_boxes
 * [B][5][4], n_gt [B] (clamped to 0..5).  Cell j of image b is record id = (image_offset + b) * cells + j.
 *   A detection is a cell with logit > 0 (NaN, +-0 and negatives are none).  rec_key[id] = (K << 32) | id with, for a detection,
 *   K = ~(u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000)), u the logit's bits -- ascending keys are descending logits, ties to the lower
 *   id -- and K = 0xFFFFFFFF for a non-detection, which sorts behind every detection.
 *   A box is an area iff its coordinates are finite and ymax > ymin, xmax > xmin.  For two areas, in fp32 with every operation
 *   rounded on its own: ih = min(ymax) - max(ymin), iw likewise; if both > 0, inter = ih * iw, a and b the two areas,
 *   union = (a + b) - inter, iou = inter / union, and threshold t = 1..9 passes iff inter > 0 and 10 * inter >= t * union.
 *   Anything else: iou 0, no threshold passes.
 *   Per threshold the image's detections are walked in key order; each takes the unmatched box of highest iou among those that
 *   pass (ties to the lower box index) and is a true positive, or takes none and is a false positive.
 *   rec_tp[id]: bit t - 1 set iff the record is a true positive at threshold t / 10; 0 for a non-detection.
 * Exactly the B * cells record slots from image_offset * cells are written.  SV_E_BADARG: a null or misaligned pointer (4 bytes;
 * rec_key 8; rec_tp 2), B or cells <= 0, image_offset < 0, a pitch below its row; SV_E_UNSUPPORTED: cells > 64 or
 * image_offset + B > (2^31 - 1) / 64. */
int sv_detect_match_host(const float* bbox, int64_t ld_bbox, const float* logits, int64_t ld_logits, int32_t cells, const float* gt_boxes,
                         const int32_t* n_gt, int32_t B, int64_t image_offset, uint64_t* rec_key, uint16_t* rec_tp);
int sv_detect_match(const float* bbox, int64_t ld_bbox, const float* logits, int64_t ld_logits, int32_t cells, const float* gt_boxes,
                    const int32_t* n_gt, int32_t B, int64_t image_offset, uint64_t* rec_key, uint16_t* rec_tp, void* stream);
/* The curve over n_records records (1 .. 2^20) in any order.  M = the detections, G = sum of n_gt[0 .. n_images - 1] (each clamped
 * to 0..5).  In ascending key order, TP_t(i) = the true positives among the first i detections and p_i = TP_t(i) / i in fp64:
 *   out[0..8]   AP_t  = (1/G) sum_i [tp_i] max_{j >= i} p_j     (all-point interpolation)
 *   out[9..17]  AP'_t = (1/G) sum_i [tp_i] p_i
 *   out[18..26] TP_t(M), out[27] M, out[28] G                    (int64 in the same 8-byte slots)
 * AP_t and AP'_t are 0 when G == 0 or M == 0.  rec_key / rec_tp are not modified; the workspace (16-byte aligned, at least
 * sv_detect_ap_workspace_bytes, any contents) holds the sorted copy and the block partials.  sv_detect_ap_chunk_records: the
 * records of one LDS sort chunk and scan block.  SV_E_BADARG: a null or misaligned pointer, n_images < 1; SV_E_UNSUPPORTED:
 * n_records outside 1 .. 2^20, n_images > 2^20; SV_E_WORKSPACE: workspace_bytes too small. */
int sv_detect_ap_chunk_records(void);
int sv_detect_ap_workspace_bytes(int64_t n_records, int64_t* bytes);
int sv_detect_ap_finish(const uint64_t* rec_key, const uint16_t* rec_tp, int64_t n_records, const int32_t* n_gt, int64_t n_images,
                        void* workspace, int64_t workspace_bytes, double* out /* [29] */, void* stream);

/* ---------------------------------------------------------------- K3-K10: NHWC conv (implicit GEMM on MFMA)
 * Replaces tf.keras.layers.Conv2D(padding='same') forward (vae/model.py:36-38,:153-156) and the
 * Conv2DBackpropInput / Conv2DBackpropFilter / BiasAddGrad / ReluGrad nodes of tape.gradient
 * (vae/trainer.py:137).  Dense layers (vae/model.py:41-42,:152) are the H=W=KH=KW=1 case.
 * Channel counts are padded to a multiple of 8 in the low-precision activation tensors.
 *
 * Accepted domain (anything else: SV_E_BADARG for malformed values, SV_E_UNSUPPORTED for valid layers without kernels):
 *   B, H, W, Cin, Cout, KH, KW > 0; dtype SV_BF16 or SV_F32 (else SV_E_BADARG); stride 1, 2 or 3 and KH * KW <= 81 (else SV_E_UNSUPPORTED);
 *   stride > 1: the stride divides H and W (SV_E_UNSUPPORTED); ldx >= Cin, ldx % 8 == 0 (SV_E_BADARG); r8(Cin) = Cin rounded up to 8 is a
 *   power of two, i.e. Cin in 1..8, 9..16, 17..32, 33..64, ... (SV_E_UNSUPPORTED); ldy >= Cout, and ldy % 8 == 0 unless y_f32 (SV_E_BADARG);
 *   ups_in: stride 1, H and W even (SV_E_UNSUPPORTED); B * H * W * ldx and B * OH * OW * r8(Cout) below 2^31 (SV_E_UNSUPPORTED).
 *   Any extents and kernel shapes in that domain, KH != KW included: power-of-two grids run on the LDS-tile / row-ring kernels, other
 *   extents on the im2col kernels.  The input gradients also need r8(Cout) to be a power of two (else they return SV_E_UNSUPPORTED).
 *   ups_in forwards exist on the LDS-tile / row-ring kernels only (the im2col kernels read a materialised input): they also need
 *   power-of-two H and W with H * W >= 16, Cout <= 16 or a multiple of 32, an 8-byte multiple of stored output bytes per pixel (y_f32 or
 *   SV_F32 with Cout % 8 != 0: min(ldy, r8(Cout)) even) and a tile that fits the LDS; otherwise SV_E_UNSUPPORTED with nothing written --
 *   upsample with sv_upsample2x_fwd and run the layer without ups_in.
 * Input precondition: the pad channels [C, pitch) of every activation and gradient input (x, dy, relu masks) are zero.
 * Output postcondition of the write-only outputs (y, the non-atomic dx, dx_lo): channels [C, min(pitch, r8(C))) are written as zeros
 *   whatever the dtype; channels from r8(C) to the pitch are left untouched or zeroed (the split-K forwards zero the whole pitch first).
 * Accumulators (dw, dbias, the fp32-atomic dx) are ADDED to, never assigned; the fp32-atomic dx leaves channels [Cin, ldx) untouched.
 * A refused call (any return other than SV_OK, checked before anything is enqueued) leaves every output buffer untouched.
 * Reproducibility under sv_set_deterministic(1): same inputs -> same bits, for the calls WITH their workspaces; without one, the polyphase
 *   head's border terms (sv_conv2d_nhwc_fwd) and the tile weight gradients (sv_conv2d_nhwc_wgrad) are added with fp32 atomics; the weight
 *   gradient of an x-packed thin head (stride 1, Cout <= 8, y_f32, W >= 32) folds its columns onto dw with atomics even with a workspace.
 * SV_TRACE_DISPATCH=1 (read once per process): every successful call prints "sv_dispatch <op> <form>" to stderr, the form it launched --
 *   fwd: row, tile, tile_packx, tile_s2d3, im2col, im2col_small, dense_splitk, conv_splitk, poly_ws, poly_atomic, polyc, polyc_direct;
 *   dgrad: merged, multi_class, per_class, atomic_splitk; dgrad_lowres: lowres_row, lowres_polyd, lowres_unsupported (the refusal);
 *   wgrad: wgrad_tile, wgrad_tile_f32, wgrad_roll, wgrad_e1, wgrad_e2, polyc_wgrad, poly_wgrad, wgrad_im2col; wgrad_poly: wgrad_tile, wgrad_p5. */
typedef struct {
  int32_t B, H, W;          /* input spatial size (see the accepted domain above) */
  int32_t Cin, Cout;        /* real channel counts (HWIO weight shape = [KH,KW,Cin,Cout]) */
  int32_t KH, KW, stride;   /* TF 'SAME' padding is implied: out=ceil(in/stride) */
  int32_t act;              /* sv_act fused into the forward epilogue */
  int32_t dtype;            /* sv_dtype of activations / prepared weights */
  int32_t ldx;              /* channels per input pixel in memory  (>= Cin, multiple of 8) */
  int32_t ldy;              /* channels per output pixel in memory (>= Cout; multiple of 8 unless y_f32) */
  int32_t y_f32;            /* forward output written as fp32 (decoder head) */
  int32_t ups_in;           /* x is the LOW-RES tensor [B,H/2,W/2,ldx] and the layer input is its 2x bilinear
                               upsample (tf.image.resize, vae/model.py:163-167), produced on the fly while the
                               tile is staged: forward and wgrad only, stride 1, tile kernels (else SV_E_UNSUPPORTED) */
} sv_conv_desc;

/* element counts (of `dtype`) of the prepared forward / dgrad weight images */
int64_t sv_conv2d_wprep_elems(const sv_conv_desc* d, int32_t for_dgrad);
/* fp32 HWIO master -> MFMA-ready [Cout_pad][taps][Cin_pad] (fwd) and per-parity-class
 * [Cin_pad][taps'][Cout_pad] (dgrad) images in `dtype`. */
int sv_conv2d_prep_weights(const sv_conv_desc* d, const float* w_hwio, void* w_fwd, void* w_dgrad,
                           void* stream);
int sv_conv2d_nhwc_fwd(const sv_conv_desc* d, const void* x, const void* w_fwd, const float* bias,
                       void* y, void* stream);
/* Same with a caller-owned workspace (sv_conv2d_fwd_workspace_bytes; 0 for most layers).  The bf16 decoder head
 * (UpSampling2D(bilinear) -> Conv2D(6, 6x6, 'same'), vae/model.py:163-167 + d5) runs in POLYPHASE form: one 5x5 conv over
 * the low-res tensor whose four output parities are four column classes, plus 1-D border terms for the taps that leave the
 * zero-padded hi-res image; with a workspace those terms are computed first and added by the conv's epilogue, without one
 * they are added to y with atomics afterwards (same result, slower).  The fp32 upsample -> 6 x 6 conv layers with 32 output channels (d4) run per output-parity
 * class over the low-res tensor and need the workspace for their border terms; WITHOUT one the call runs the direct fused-resize form on a second
 * weight image that sv_conv2d_prep_weights keeps behind the class images (sv_conv2d_wprep_elems counts it) -- same result to fp32 rounding, 1.4x the time.
 * A workspace smaller than sv_conv2d_fwd_workspace_bytes counts as none (never read or written): the same fallbacks.
 * Form selection is a pure function of the descriptor (and of the SV_POLYC_K switch, which must not change between
 * sv_conv2d_prep_weights and the calls that consume its images). */
int64_t sv_conv2d_fwd_workspace_bytes(const sv_conv_desc* d);
int sv_conv2d_nhwc_fwd_ws(const sv_conv_desc* d, const void* x, const void* w_fwd, const float* bias, void* y,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* dx = conv-transpose(dy, w) * (mask>0 if mask!=NULL); dy[B,OH,OW,ldy], dx[B,H,W,ldx] (dtype).
 * dx_f32_atomic!=0: K is split over workgroups and dx (fp32, pre-zeroed) is accumulated atomically. */
int sv_conv2d_nhwc_dgrad(const sv_conv_desc* d, const void* dy, const void* w_dgrad,
                         const void* relu_mask, void* dx, int32_t dx_f32_atomic, void* stream);
/* The same for a layer with ups_in (its input is the 2x bilinear upsample of a low-res tensor, vae/model.py:163-167),
 * delivered AT THE LOW-RES TENSOR: dx_lo[B,H/2,W/2,ldx] = (relu_mask_lo > 0) * resize_adjoint(conv-transpose(dy, w)) in
 * one launch -- ResizeBilinearGrad + ReluGrad of tape.gradient (vae/trainer.py:137) fused into the Conv2DBackpropInput
 * kernel; the hi-res gradient never reaches HBM.  SV_E_UNSUPPORTED when the geometry has no fused kernel: call
 * sv_conv2d_nhwc_dgrad followed by sv_upsample2x_bwd instead (bitwise the same result). */
int sv_conv2d_nhwc_dgrad_lowres(const sv_conv_desc* d, const void* dy, const void* w_dgrad,
                                const void* relu_mask_lo, void* dx_lo, void* stream);
/* The same with a caller-owned workspace (sv_conv2d_dgrad_lowres_workspace_bytes; 0: the layer needs none).  At the reference's precision (SV_F32) the
 * 6 x 6 upsample -> conv layers (vae/model.py:155-156 behind :165 / :167: d4, d5) take the POLYPHASE form: the transposed conv and the resize adjoint collapse
 * into one stride-2 conv with 9 x 9 taps over the hi-res dy (81 tap products per low-res pixel instead of 4 x 36), the zero-padding / edge-clamp terms of the
 * first and last low-res row and column travel through the workspace (csrc/polyd_dgrad.hip).  Without a (large enough) workspace: sv_conv2d_nhwc_dgrad_lowres. */
int64_t sv_conv2d_dgrad_lowres_workspace_bytes(const sv_conv_desc* d);
int sv_conv2d_nhwc_dgrad_lowres_ws(const sv_conv_desc* d, const void* dy, const void* w_dgrad, const void* relu_mask_lo, void* dx_lo,
                                   void* workspace, int64_t workspace_bytes, void* stream);
/* dw[KH,KW,Cin,Cout] += x^T*dy, dbias[Cout] += colsum(dy) (fp32 HWIO, atomically accumulated:
 * zero them first).  ups_in layers off the model's decoder geometries may return SV_E_UNSUPPORTED (nothing written): upsample
 * x with sv_upsample2x_fwd and call the plain layer instead. */
int sv_conv2d_nhwc_wgrad(const sv_conv_desc* d, const void* x, const void* dy, float* dw,
                         float* dbias, void* stream);
/* Same with a caller-owned partial-sum workspace (sv_conv2d_wgrad_workspace_bytes): the tile kernel
 * then writes per-split slabs and reduces them in a fixed order -- faster than atomics and
 * bitwise reproducible.  dw is still accumulated into (zero it first). */
int64_t sv_conv2d_wgrad_workspace_bytes(const sv_conv_desc* d);
int sv_conv2d_nhwc_wgrad_ws(const sv_conv_desc* d, const void* x, const void* dy, float* dw,
                            float* dbias, void* workspace, int64_t workspace_bytes, void* stream);

/* Weight gradient of the bf16 decoder head (UpSampling2D(bilinear) -> Conv2D(6x6), vae/model.py:163-169) in POLYPHASE form: the
 * weight gradient of the 5x5 low-res conv (no blend arithmetic, a quarter of the pixels staged), projected back onto the 6x6
 * kernel, minus the out-of-image taps of the five border rows / columns (tests/test_polyphase_math.py).  Same result
 * as sv_conv2d_nhwc_wgrad on the same layer to bf16 accuracy (closer to the fp64 gradient: the upsampled activations are never
 * rounded).  Workspace: sv_conv2d_wgrad_poly_workspace_bytes (0 = the layer has no polyphase form), ZEROED before its first use.
 * H and W must be multiples of 32 (the frame kernel takes border lines in 32-pixel chunks); otherwise SV_E_UNSUPPORTED and a workspace
 * size of 0: use sv_conv2d_nhwc_wgrad_ws. */
int64_t sv_conv2d_wgrad_poly_workspace_bytes(const sv_conv_desc* d);
int sv_conv2d_nhwc_wgrad_poly(const sv_conv_desc* d, const void* x_lo, const void* dy, float* dw, float* dbias, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- F3: input files (host side, no device work)
 * CRC-32C of the TFRecord framing the reference's CelebA files use (tf.io.TFRecordWriter at vae/data.py:93-100,
 * TFRecordDataset at :123-131): record = uint64 length | masked_crc32c(length) | data | masked_crc32c(data),
 * masked(c) = rotr(c, 15) + 0xa282ead8.  sv_crc32c("123456789") == 0xE3069283. */
uint32_t sv_crc32c(const void* data, int64_t n);
uint32_t sv_masked_crc32c(const void* data, int64_t n);

/* ---------------------------------------------------------------- A9: SPLIT-GMVAE global encoder glue
 * The contractions of Encoder(type='gmvae') (vae/model.py:48-79, call_gmvae :116-135) run on the
 * sv_conv2d_* kernels (dense layers = 1x1 convs on a 1x1 grid); these are the pointwise pieces between
 * them.  `dtype` arguments are sv_dtype; "lp" tensors are in the contraction dtype with the row pitch
 * the next MFMA layer reads (padding columns are written as zeros).
 *
 * sv_act_fwd: x[r,c] = dropout(act(a[r,c])), c < C  (Conv2D/Dense activation='elu' :50-52,:55,:57,:64,:73;
 *   Dropout(rate) in training = x * keep / (1-rate) :56,:72 as called at :118,:129).  y_act (optional) receives
 *   the pre-dropout activation (act' is recovered from it in the backward).  keep_in (optional, [rows*C] 0/1)
 *   pins the mask; otherwise it is drawn from Philox keyed by (seed, step, stream_id, sample_offset + r /
 *   rows_per_sample, column) and written to keep_out.
 * sv_act_bwd: ga = (gx * keep/(1-rate) + gx2) * act'(y_act)   (gx2, y_act optional). */
int sv_act_fwd(const void* a, int32_t a_dtype, int32_t lda, void* y_act, void* x, int32_t x_dtype, int32_t ldx,
               int64_t rows, int32_t C, int32_t act, float drop_rate, const float* keep_in, float* keep_out,
               uint64_t seed, uint64_t step, int32_t stream_id, int64_t sample_offset, int32_t rows_per_sample,
               void* stream);
int sv_act_bwd(const void* gx, int32_t gx_dtype, int32_t ldg, const void* gx2, int32_t gx2_dtype, int32_t ldg2,
               const void* y_act, int32_t y_dtype, int32_t ldy, int32_t act, float drop_rate, const float* keep,
               void* ga, int32_t ga_dtype, int32_t ldga, int64_t rows, int32_t C, void* stream);
/* out = a + b (vae/model.py:130: h = h + h_top) */
int sv_add(const void* a, const void* b, void* out, int32_t dtype, int64_t n, void* stream);
/* The five Mean metrics of train_step_lg_gm_vae / test_step_lg_gm_vae (vae/trainer.py:157-173) and the total loss from the per-image terms
 * [B] fp32: out6 = {mean nll_x, mean kl_x, mean nll_xh, mean kl_xh, mean y_kl, out[0] + out[2] + beta (out[1] + out[3]) + alpha out[4]}.
 * One launch, fixed-order sums. */
int sv_gm_metrics(const float* nll_x, const float* kl_x, const float* nll_xh, const float* kl_xh, const float* y_kl, int32_t B,
                  float beta, float alpha, float* out6, void* stream);
/* Unsupervised cluster accuracy (vae/trainer.py:40-68 linear_assignment, :315-349): for each of the B rows, cluster k = argmax of
 * logits[b, :K] and class c = argmax of labels_onehot[b, :C] (first index on ties, as tf.argmax); counts[k * C + c] += 1 (int32,
 * integer atomics: deterministic).  counts [K][C] is accumulated into -- zero it once, call once per batch.  The accuracy of the
 * majority-class assignment is sum_k max_c counts[k][c] / N. */
int sv_cluster_confusion(const float* logits, int32_t ld, const float* labels_onehot, int32_t ld_lab, int32_t B, int32_t K, int32_t C,
                         int32_t* counts, void* stream);
/* Gumbel-softmax (vae/model.py:121-122): y = softmax((logits - log(-log u)) / tau, axis=1); u[B,K] (NULL: Philox,
 * written to u_out).  y[B,K] fp32 and y_lp[B,ld_lp] (zero padded).  K, ld_lp <= 128. */
int sv_gumbel_softmax_fwd(const float* logits, int32_t ld_logits, const float* u, float* u_out, float tau, float* y,
                          void* y_lp, int32_t lp_dtype, int32_t ld_lp, int32_t B, int32_t K, uint64_t seed,
                          uint64_t step, int64_t sample_offset, void* stream);
/* its adjoint plus the categorical term of train_step_lg_gm_vae (vae/trainer.py:161-165):
 * g_logits = (1/tau) y (gy - <y,gy>) + alpha_over_B * d/dlogits sum_k p_k (log(p_k + 1e-8) - log(1/K)), p = softmax(logits);
 * y_kl[b] = that sum for image b.  g_logits NULL: only y_kl (evaluation). */
int sv_gumbel_softmax_bwd(const float* gy, int32_t ldg, const float* y, const float* logits, int32_t ld_logits,
                          float tau, float alpha_over_B, void* g_logits, int32_t g_dtype, int32_t ld_out,
                          float* y_kl, int32_t B, int32_t K, void* stream);
/* posterior and prior heads (vae/model.py:124-125,:131-133; Sampling :9-13) from the four fp32 pre-activations
 * (bias included): z_mean = a_mean, z_sig = softplus(a_sig), z = z_mean + z_sig*eps, prior likewise; z_lp is the
 * decoder input (columns [z_col, z_col+L) of `zcat`); kl2[b] = kl_divergence_two_gauss row sum (vae/trainer.py:17-18). */
int sv_gm_head_fwd(const float* a_mean, const float* a_sig, const float* a_prior_mean, const float* a_prior_sig,
                   const float* eps, float* eps_out, float* z_mean, float* z_sig, float* z, float* prior_mean,
                   float* prior_sig, void* z_lp, int32_t lp_dtype, int32_t ldz, int32_t z_col, float* kl2,
                   int32_t B, int32_t L, uint64_t seed, uint64_t step, int64_t sample_offset, void* stream);
/* adjoint: dL/dz (decoder) + kl_scale * d kl2, through the two softplus heads, as the dY of the four Dense layers */
int sv_gm_head_bwd(const float* dz, int32_t ld_dz, const float* z_mean, const float* z_sig, const float* prior_mean,
                   const float* prior_sig, const float* eps, float kl_scale, void* g_a_mean, void* g_a_sig,
                   void* g_a_prior_mean, void* g_a_prior_sig, int32_t g_dtype, int32_t B, int32_t L, void* stream);

/* ---------------------------------------------------------------- A9: the SPLIT-GMVAE global encoder as one object
 * Replaces Encoder(type='gmvae').call_gmvae (vae/model.py:48-79, :116-135) and its adjoint in train_step_lg_gm_vae
 * (vae/trainer.py:146-173) with native launch sequences over one caller-owned workspace.  It plugs into an LGVae plan
 * created with external_global_encoder = 1: FWD_ENCODERS phase -> sv_gm_encoder_forward (writes z_x into zcat[:, :L])
 * -> FWD_DECODERS/LOSS/BWD_DECODERS phases -> sv_gm_encoder_backward (reads dL/dz_x from the plan's gz_x) -> ... */
typedef struct {
  int32_t B, H, W;          /* H == W, power of two >= 8 */
  int32_t latent;           /* global latent size L (power of two) */
  int32_t y_size;           /* categorical size K (2..128) */
  float tau;                /* Gumbel-softmax temperature */
  int32_t dtype;            /* sv_dtype of the contractions */
} sv_gm_desc;
typedef struct {
  const float* params;      /* flat fp32 [sv_gm_param_count]: the 24 arrays in the reference's variable order */
  float* grads;             /* backward: same layout, ACCUMULATED into (zero it first) */
  const void* in8_x;        /* [B,H,W,8] network input in `dtype` (the plan's buffer "in8_x") */
  void* zcat; int32_t ldz;  /* forward: decoder input rows (the plan's "zcat"), row pitch in elements */
  const float* gz; int32_t ld_gz;   /* backward: dL/dz_x rows (the plan's "gz_x"), columns [0, L) */
  const float* eps;         /* [B,L]     or NULL -> Philox        (pins for parity tests) */
  const float* u;           /* [B,K]     Gumbel uniforms or NULL */
  const float* keep1;       /* [B,1024]  y_block dropout mask (0/1) or NULL */
  const float* keep5;       /* [B,F]     do5 dropout mask or NULL */
  int32_t training;         /* 1: y_block's Dropout and do5 act (vae/model.py:56,:72,:129).  train_step_lg_gm_vae passes
                             training=True (vae/trainer.py:149) but LGGMVae.call drops it before encoder_x (:241): under the
                             pinned tensorflow 2.0.0 the dropouts never fire (pass 0), under >= 2.1 they do (pass 1) */
  float beta, alpha;        /* backward: weights of the two-Gaussian KL and of the categorical KL */
  uint64_t seed, step;
  int64_t sample_offset;
} sv_gm_args;
typedef struct sv_gm_encoder sv_gm_encoder;
int64_t sv_gm_param_count(const sv_gm_desc* d);
int sv_gm_param_info(const sv_gm_desc* d, int32_t index, int64_t* offset, int32_t* ndim, int64_t shape[4], char name[96]);
int sv_gm_encoder_create(const sv_gm_desc* d, sv_gm_encoder** enc);
void sv_gm_encoder_destroy(sv_gm_encoder* enc);
int64_t sv_gm_encoder_workspace_bytes(const sv_gm_encoder* enc);
int sv_gm_encoder_bind(sv_gm_encoder* enc, void* workspace, int64_t bytes, void* stream);   /* zero-fills the workspace, uploads the job table (as sv_lgvae_plan_bind) */
/* named activation / gradient buffers inside the workspace (z, zm, zs, pm, ps, y, logits, kl2, ykl, keep1, ...) */
int sv_gm_encoder_buffer(const sv_gm_encoder* enc, const char* name, int64_t* offset, int64_t* bytes);
/* fp32 masters -> MFMA-ready weight images of the twelve layers (after every parameter update) */
int sv_gm_encoder_prep(sv_gm_encoder* enc, const float* params, void* stream);
int sv_gm_encoder_forward(sv_gm_encoder* enc, const sv_gm_args* a, void* stream);
int sv_gm_encoder_backward(sv_gm_encoder* enc, const sv_gm_args* a, void* stream);
/* evaluation: the per-image categorical KL term "ykl" of the last forward, no gradients */
int sv_gm_encoder_y_kl(sv_gm_encoder* enc, void* stream);

/* ---------------------------------------------------------------- A2/A3/A5/A8: the whole LGVae step
 * Replaces LGVae.call (vae/model.py:189-200) and train_step_lg_vae (vae/trainer.py:120-144)
 * with one native launch sequence on `stream` (captured into a hipGraph by the caller if wanted). */
typedef struct {
  int32_t B, H, W;                       /* per-device batch; H==W power of two, multiple of 8 */
  int32_t global_latent, local_latent;   /* vae/main.py:16-17 (multiples of 8) */
  int32_t dtype;                         /* sv_dtype of the contractions */
  float beta;                            /* vae/main.py:19 */
  int32_t external_global_encoder;       /* 1: SPLIT-GMVAE (LGGMVae, vae/model.py:221-246): encoder_x is the caller's
                                            (type 'gmvae', :48-79).  The plan then skips encoder_x in every phase: the
                                            caller stores z_x into columns [0, global_latent) of the `zcat` buffer between
                                            FWD_ENCODERS and FWD_DECODERS and reads dL/dz_x from columns [0, global_latent)
                                            of `gz_x` after BWD_DECODERS.  The encoder_x slots of the parameter table stay
                                            (unused, zero gradient) so the flat layout is the same in both modes. */
  int32_t global_only;                   /* 1: GMVae (vae/model.py:277-298): ONE branch -- the caller's encoder_x (requires
                                            external_global_encoder = 1, else SV_E_BADARG) and decoder_x over z_x alone.  The
                                            parameter table then holds only the 10 decoder_x arrays (d1 kernel [global_latent,
                                            (H/8)(W/8)128]); local_latent is ignored.  Every phase skips encoder_x_hat,
                                            decoder_x_hat and the x-hat loss; FWD_ENCODERS only zeroes gz_x and fills in8_x
                                            (in8_xh stays, so the staged augmentation writes the same buffers); the BWD_ENC
                                            phases do nothing.  `zcat` and `gz_x` have row pitch global_latent; the caller
                                            reads dL/dz_x from gz_x.  The loss phase writes nll_x (per image) and losses[0]
                                            (mean) -- the KL terms are the caller's.  Graph replay is refused
                                            (sv_lgvae_graph_enable: SV_E_UNSUPPORTED).  0: the two-branch plan above. */
} sv_lgvae_desc;

typedef struct sv_lgvae_plan sv_lgvae_plan;

/* the 40 trainable variables (10 with global_only), Keras creation order, flat fp32 buffer */
int64_t sv_lgvae_param_count(const sv_lgvae_desc* d);
int sv_lgvae_param_info(const sv_lgvae_desc* d, int32_t index, int64_t* offset, int32_t* ndim,
                        int64_t shape[4], char name[96]);

int sv_lgvae_plan_create(const sv_lgvae_desc* d, sv_lgvae_plan** plan);
void sv_lgvae_plan_destroy(sv_lgvae_plan* plan);
int64_t sv_lgvae_workspace_bytes(const sv_lgvae_plan* plan);
/* carve the caller-owned workspace: ZERO-FILLS it (pad channels / rows that no kernel writes are read as zeros; a few accumulators count up from zero) and uploads the
 * (tiny) weight-prep job table, both on `stream`; returns after the upload has finished.  The workspace must not be written by anything else while the plan is bound. */
int sv_lgvae_plan_bind(sv_lgvae_plan* plan, void* workspace, int64_t bytes, void* stream);
/* byte offset/size of a named workspace buffer (for zero-copy views of outputs); <0 if unknown */
int sv_lgvae_buffer(const sv_lgvae_plan* plan, const char* name, int64_t* offset, int64_t* bytes);

enum { SV_PHASE_PREP = 1,           /* fp32 master weights -> MFMA-ready images */
       SV_PHASE_FWD_ENCODERS = 2,   /* split/pad, e1-e3, heads, reparameterisation + KL */
       SV_PHASE_FWD_DECODERS = 4,   /* d1-d5 of both decoders from the latents in `zcat` */
       SV_PHASE_LOSS = 8,           /* ELBO terms (+ their gradients and grad zeroing when grads != NULL) */
       SV_PHASE_BWD_DECODERS = 16,  /* fills the decoder_x / decoder_x_hat gradient ranges */
       SV_PHASE_BWD_ENC_HEADS = 32, /* reparam adjoint, e4_mean/e4_sd gradients, dgrad into a3 */
       SV_PHASE_BWD_ENC_CONVS = 64, /* e3, e2, e1 gradients */
       SV_PHASE_ADAM = 128,
       SV_PHASE_NO_RECON = 256,     /* modifier: a call that runs the decoders, the loss and its gradients together evaluates the loss in
                                       the head conv's epilogue; the reconstruction tensors out6_x / out6_xh (x_mean | x_log_scale) are
                                       then dead -- train_step_lg_vae (vae/trainer.py:121-144) returns nothing -- and with this bit they
                                       are not stored (100 MB of HBM writes per 512-image step).  Losses and gradients are unchanged. */
       SV_PHASE_INPUTS_STAGED = 512, /* modifier: the plan buffers in8_x / in8_xh already hold this call's images6 as padded 8-channel
                                       tensors in the plan's dtype (written by sv_scramble_gather_staged): the split / pad pass is skipped */
       SV_PHASE_BUCKET_EVENTS = 1024, /* modifier (data parallelism): the plan records an event set when each gradient bucket is complete -- 0: both decoders
                                       (after SV_PHASE_BWD_DECODERS), 1: the encoder heads (e4_mean / e4_sd, after SV_PHASE_BWD_ENC_HEADS), 2: the encoder convs --
                                       on the compute stream AND on its weight-gradient side streams, so ONE call can run the whole backward with the
                                       single-GPU stream overlap while the caller's communication stream picks every bucket up as it completes
                                       (sv_lgvae_bucket_wait); no phase-split host round trips */
       SV_PHASE_FORWARD = 6, SV_PHASE_BACKWARD = 112, SV_PHASE_ALL = 255 };

typedef struct {
  float* params;            /* flat fp32 [param_count] */
  float* grads;             /* flat fp32 [param_count] (zeroed by PHASE_LOSS) */
  float* adam_m;            /* flat fp32 */
  float* adam_v;            /* flat fp32 */
  const float* images6;     /* [B,H,W,6] fp32, output of sv_scramble_gather */
  const float* eps_x;       /* [B,global_latent] or NULL -> Philox */
  const float* eps_x_hat;   /* [B,local_latent]  or NULL -> Philox */
  uint64_t seed, step;
  int64_t sample_offset;    /* global index of this rank's first sample */
  float lr, beta1, beta2, adam_eps;
  int64_t t;                /* Adam iteration (iterations+1) */
  float grad_scale;         /* applied in Adam (1/world_size for DP) */
  int32_t phases;           /* SV_PHASE_* mask */
  int32_t accumulate_metrics; /* add the 5 scalars into the running-mean accumulators (K15) */
} sv_lgvae_step_args;

int sv_lgvae_step(sv_lgvae_plan* plan, const sv_lgvae_step_args* a, void* stream);

/* hipGraph replay of sv_lgvae_step (no reference counterpart: the reference's tf.function traces its step once,
 * vae/trainer.py:117 / :146; this is the HIP equivalent for the launch-bound small-batch configurations).  With it on,
 * the first step of each distinct (phase mask, buffer set, Adam constants) runs eagerly, the second is captured on
 * `stream`, later ones are ONE hipGraphLaunch; seed / step / sample_offset / lr / t stay per-step values (they reach
 * the kernels through a small device record).  Steps issued on the legacy default stream (stream == NULL) are never
 * captured; at most 16 distinct graphs are kept (callers that rotate buffers beyond that stay eager).  Disabling destroys
 * the captured graphs.  Profiling turns replay off.  Measured (scripts/bench_graph.py, SVHN-32 B=64 .. CelebA-64
 * B=512): replay == eager to 1 %: the kernels already run back to back, the small configurations are bound by the
 * ~10 us dependent-kernel latency of an in-order stream, which a graph of the same chain keeps. */
int sv_lgvae_graph_enable(sv_lgvae_plan* plan, int32_t enable);
/* Make `stream` wait (hipStreamWaitEvent, no host sync) until gradient bucket `bucket` of the most recent sv_lgvae_step call that carried
 * SV_PHASE_BUCKET_EVENTS is complete: 0 decoders, 1 encoder heads, 2 encoder convs, 3 = 1 and 2 (the whole encoders' range).  The gradient
 * all-reduce of that bucket (RCCL over xGMI) is then enqueued on `stream`.  SV_E_STATE: no such events were recorded.
 * Every call that runs a backward phase invalidates the events of the steps before it; a captured (hipGraph) step records none -- callers then order the
 * collective behind the compute stream instead (split_vae_amd/trainer.py falls back to one all-reduce after the backward).  Every layer's weight-gradient slab reduce
 * runs on the layer's own stream right behind its main kernel, so it is in front of the events. */
int sv_lgvae_bucket_wait(sv_lgvae_plan* plan, int32_t bucket, void* stream);
/* Test hooks of ONE plan (tests/test_gpu_dist.py); an explicit call, never an environment variable, so nothing a training job inherits can switch them on:
 *   "side_delay_us" = n    the first weight-gradient side-stream launch of every step is held back n microseconds (a consumer that misses the side
 *                          stream's part of a bucket then reads gradients that do not exist yet);
 *   "bucket_skip_side" = 1 sv_lgvae_bucket_wait drops the side streams' events (the negative control of the dependency test).
 * SV_E_BADARG: unknown key / value out of range. */
int sv_lgvae_plan_debug(sv_lgvae_plan* plan, const char* key, int64_t value);
/* Test hook, no plan and no device call (tests/test_plan_state_host.py): the host state machine that tracks where dL/dz of the decoders lives between the phases
 * of a step (csrc/plan_latent.h).  state: 0 zeroed, 1 stale (the encoders' forward skipped the zero fill: nothing accumulates), 2 summed in gz_*, 3 unsummed
 * K-slice slabs in lat_ws_*.  event: 0 encoders' forward (slab_path: both split-K launches of the plan run on latent_gemm.hip), 1 decoders' backward that leaves
 * the slabs, 2 decoders' backward with dL/dz in gz_* (slab_path: summed from slabs; 0: accumulated), 3 encoder heads' backward.  *next: the state after the event;
 * *zero_range: what the phase zeroes first -- 0 nothing, 1 gz_x .., 2 pre_x .. gz_xh.  SV_E_BADARG: state / event outside 0 .. 3 or a null result. */
int sv_lgvae_dz_transition(int32_t state, int32_t event, int32_t slab_path, int32_t* next, int32_t* zero_range);
/* The library's side streams: hipStream_t `index` (0 .. 2) of the CURRENT device, created once per process and shared by every plan (weight-gradient
 * streams), tape (lanes) and by the SPLIT-GMVAE step's second encoder stream -- a stream per object put a later object's stream on the hardware queue of the
 * compute stream it should run beside (csrc/streams.hip).  A host binding that wants a library-compatible side stream of its own takes it from here.
 * On failure *stream is NULL and the status is non-zero: SV_E_BADARG for an index outside 0 .. 2, SV_E_STATE when the stream cannot be created. */
int sv_side_stream(int32_t index, void** stream);
/* number of captured (instantiated) step graphs, or a negative SV_E_* */
int sv_lgvae_graph_count(const sv_lgvae_plan* plan);

/* per-kernel hipEvent timing (bench roofline): enable, run steps, read average ms per launch */
int sv_lgvae_profile_enable(sv_lgvae_plan* plan, int32_t enable);
/* restrict the event brackets to launches whose label equals `name` (NULL or "" = all launches) */
int sv_lgvae_profile_filter(sv_lgvae_plan* plan, const char* name);
int sv_lgvae_profile_read(sv_lgvae_plan* plan, int32_t max_entries, char names[][64],
                          double* total_ms, int32_t* launches, double* flops_per_launch,
                          double* bytes_per_launch);
/* FLOPs per launch the scope's algorithm really multiplies on the matrix pipe, entry i = entry i of sv_lgvae_profile_read.  flops_per_launch above is the DIRECT
 * form's count (2 B OH OW Cout KH KW Cin: SURVEY 8d); the polyphase forms of the upsample -> conv layers multiply 81 (per-class forms, the
 * stride-2 input gradient) or 100 (the head's merged 25-tap form) of the direct form's 144 tap products per low-res pixel, plus their border terms: a scope's
 * rate against the MFMA peak is a utilisation figure only at THIS count.  Equal to flops_per_launch for every direct-form scope. */
int sv_lgvae_profile_read_issued(sv_lgvae_plan* plan, int32_t max_entries, double* issued_flops_per_launch);

/* ---------------------------------------------------------------- IW: importance-weighted test log-likelihood of LGVae
 * No reference counterpart: test_step_lg_vae (vae/trainer.py:199-233) reports the single-sample ELBO pieces only.  This is the
 * K-sample importance-weighted bound (Burda et al.), log (1/K) sum_k p(x, z_k) / q(z_k | x), the estimator of log p(x) VAE papers
 * are compared by.  The expensive parts are the plan's: SV_PHASE_FWD_ENCODERS once per batch, then per sample
 * SV_PHASE_FWD_DECODERS | SV_PHASE_LOSS over the latents in `zcat`; the two entries below are the code between those passes
 * (csrc/iw.hip).  K samples cost K decoder passes and K + 1 launches of sv_iw_advance, all on one stream, no host round trip.
 *
 * The estimator.  Image i has encoder outputs mu_g, sig_g [Lg] (from x) and mu_l, sig_l [Ll] (from x_hat): the plan buffers
 * z_mean_x, z_sig_x, z_mean_xh, z_sig_xh.  Sample k:
 *   z = mu + sig * eps per dimension -- the fp32 expression of sv_reparam_kl_fwd -- stored to zcat in the plan's dtype, columns
 *     [0, Lg) global, [Lg, Lg + Ll) local;
 *   r(i,k) = sum_j [log N(z_j; 0, 1) - log N(z_j; mu_j, sig_j)] = sum_j [(eps_j^2 - z_j^2) / 2 + log sig_j] over all Lg + Ll
 *     dimensions, fp32;
 *   after the decoder + loss pass over that zcat the plan holds nll_x[i], nll_xh[i] (fp32);
 *   lw_joint = -nll_x - nll_xh + r   estimates log p(x, x_hat) under p(z_g) p(z_l) p(x | z_g, z_l) p(x_hat | z_l);
 *   lw_x     = -nll_x + r            the same proposal as an importance sampler for the marginal p(x): the literature's figure;
 *   per image L_K = logsumexp_k lw(i,k) - log K for both weights, elbo = mean_k lw_joint;
 *   bits per dimension of x = -mean_i L_K^x / (H W 3 ln 2), no offset: the discretised logistic is a probability MASS over the
 *     256 levels.
 * SV_BF16 plans: the stored value enters -- z~ = bf16(z) in the prior term, eps~ = (z~ - mu) / sig in the q term -- so the weight
 * is evaluated at the latent the decoder consumed.  SV_F32: z and eps as drawn.
 * Device state [B,5] fp64 per image: (m, s) of the streamed log-sum-exp of lw_joint, (m, s) of lw_x, sum_k lw_joint;
 * m' = max(m, lw), s' = s exp(m - m') + exp(lw - m').  (Log-weights are ~1e4 nats and K may be thousands: fp32 sums lose the
 * third decimal.)
 * Random numbers: eps [B, Lg + Ll] pins the draw; NULL: the library's Philox4x32-10 with a key constant of its own (seed ^
 * 0x1a7e17a11eed) and counter (dimension j, global image index sample_offset + b, 'iw' tag | 0 global / 1 local, sample k), the
 * Box-Muller of sv_reparam_kl_fwd: sample k of image i is a pure function of (seed, i, k), whatever batch it sits in and
 * whatever K is, and never coincides with a training step's draws.
 *
 * sv_iw_advance: `k` = the number of samples drawn before this call.  SV_IW_ACCUMULATE folds sample k - 1 -- nll_x, nll_xh and
 * the r its draw left in r[B] -- into state (k == 1 starts the state: it need not be initialised); SV_IW_DRAW then draws sample
 * k: writes zcat (row pitch ldz elements) and r.  The first call of a batch is draw-only (k = 0), the last accumulate-only
 * (k = K).  One wave per image; no atomics; bit-reproducible.  SV_E_BADARG: B, Lg or Ll <= 0, k < 0, flags 0 or with an unknown
 * bit, a z_dtype outside sv_dtype, r NULL; with ACCUMULATE: nll_x / nll_xh / state NULL or k < 1; with DRAW: a null mean / sig /
 * zcat or ldz < Lg + Ll. */
enum { SV_IW_ACCUMULATE = 1, SV_IW_DRAW = 2 };
int sv_iw_advance(const float* z_mean_x, const float* z_sig_x, const float* z_mean_xh, const float* z_sig_xh, const float* eps,
                  void* zcat, int32_t z_dtype, int32_t ldz, float* r, const float* nll_x, const float* nll_xh, double* state,
                  int32_t B, int32_t Lg, int32_t Ll, int32_t k, uint64_t seed, int64_t sample_offset, int32_t flags, void* stream);
/* out3 [B,3] fp32 = per image (L_K^joint, L_K^x, elbo) from the state after K accumulated samples; acc (may be NULL) [4] fp64 +=
 * (sum_i L_K^joint, sum_i L_K^x, sum_i elbo, B), the fp64 values added in image index order by one workgroup (deterministic):
 * zero it once per test set, read it back once.  SV_E_BADARG: state or out3 NULL, K or B <= 0. */
int sv_iw_finish(const double* state, int32_t K, float* out3, double* acc, int32_t B, void* stream);

/* ---------------------------------------------------------------- IW for the mixture models: LGGMVae (SPLIT-GMVAE) and GMVae
 * No reference counterpart.  The same K-sample bound for the two models whose global latent has the y-conditional mixture prior,
 * with y marginalised on both sides (Rao-Blackwellised) instead of weighting (y, z) pairs (csrc/iw_gm.hip).  `n` below is the number
 * of mixture components (y_size, 1 .. 128); K stays the number of importance samples.
 *
 * Generative model (the discrete-y model visualizer.generate samples from):
 *   y ~ Uniform{0 .. n-1}                                   (the y-KL of vae/trainer.py:161 is against 1/n)
 *   z_g | y ~ N(pm[y], ps[y]),  pm[y] = W_pm[y,:] + b_pm,  ps[y] = softplus(W_ps[y,:] + b_ps)       (encode_y of a one-hot)
 *   z_l ~ N(0, I)                                           (LGGMVae only)
 * Proposal per image b: the encoder of vae/model.py:116-135 evaluated at one-hot y:
 *   pi_b = softmax(logits[b]);  h_top[c] = elu(W_ht[c,:] + b_ht)  (does not depend on the image);
 *   zm[b,c,:] = (he[b] + h_top[c]) . W_zm + b_zm,   zs[b,c,:] = softplus((he[b] + h_top[c]) . W_zs + b_zs),
 *   he = the GM encoder's buffer of that name (elu of e1) in test mode (no dropout); q(z_l | x_hat) = N(mu_l, sig_l) as in LGVae.
 * Sample k:  c ~ Cat(pi_b);  z_g = zm[b,c] + zs[b,c] * eps_g;  z_l = mu_l + sig_l * eps_l   (the fp32 expression of sv_iw_advance),
 * stored to zcat in the plan's dtype.  With z the STORED latent (SV_F32: z as drawn; SV_BF16: z~ = bf16(z), the existing rule) and
 *   g(z; m, s) = sum_d [ -((z_d - m_d) / s_d)^2 / 2 - log s_d ]     (log N without the -Lg/2 log 2 pi both mixtures share)
 *   r = logsumexp_c [ -log n + g(z_g; pm[c], ps[c]) ] - logsumexp_c [ log pi_b,c + g(z_g; zm[b,c], zs[b,c]) ]
 *       + sum_j [ (t_j^2 - z_l,j^2) / 2 + log sig_l,j ],   t_j = (z_l,j - mu_l,j) / sig_l,j,
 * all in fp32, both log-sum-exps with their maximum subtracted (components hundreds of sigmas away underflow to 0, never to -inf or
 * NaN), log pi_b,c = (logits[b,c] - max) - log sum_c' exp(logits[b,c'] - max) with the sum cumulated in index order.
 *   lw_joint = -nll_x - nll_xh + r,  lw_x = -nll_x + r;  per-image L_K, elbo and bits/dim exactly as sv_iw_advance / sv_iw_finish define
 * them: the state is the same [B,5] fp64 layout and sv_iw_finish is the finish of both.  GMVae is the one-branch mode: Ll = 0, no
 * nll_xh, joint == x.  `elbo` here is the MEAN LOG-WEIGHT OF THIS MARGINAL ESTIMATOR, mean_k lw_joint -- not the training loss, whose
 * y is relaxed (Gumbel-softmax) and whose KL terms are taken per y sample.
 * The component pick when `comp` is NULL: a Philox uniform u in (0, 1] with the key constant of sv_iw_advance and counter (0, global
 * image index sample_offset + b, 'iw' tag | 2, sample k) -- a pure function of (seed, image, sample); inverse CDF over the fp32
 * e_c = exp(logits[b,c] - max), cumulated in index order: the first c whose cumulated mass is >= u * total, the last component
 * catching rounding.  sv_iw_gm_uniform_host is the host mirror of u.  eps_g / eps_l: `eps` [B, Lg + Ll] pins them, NULL draws them
 * as sv_iw_advance does (tags 0 / 1).  comp [B] int32 pins the component (clamped to 0 .. n-1); comp_out [B] always receives it.
 *
 * sv_iw_gm_advance has the contract of sv_iw_advance (k, SV_IW_ACCUMULATE, SV_IW_DRAW, a draw-only first and an accumulate-only last
 * call, no atomics, no host round trip, bit-reproducible).  logits [B,n], zm_all / zs_all [B,n,Lg], pm / ps [n,Lg], all fp32.
 * One 256-thread workgroup per image: wave 0 takes the softmax and the pick; all threads draw z (z_g kept in LDS); for the densities
 * thread (c, s) owns component c and the dimensions d = s, s + S, ... with S = min(64, 256 / pow2ceil(n)) adjacent lanes per
 * component, so ONE log2(S)-step shuffle reduction finishes all 2 n sums at once, and wave 0 takes both log-sum-exps over n together.
 * Lg and Ll may be any positive size (Ll = 0: one branch).  SV_E_BADARG: B or Lg <= 0, Ll < 0, n outside 1 .. 128, k < 0, flags 0 or
 * with an unknown bit, a z_dtype outside sv_dtype, r NULL; with ACCUMULATE: nll_x / state NULL, nll_xh NULL while Ll > 0, k < 1; with
 * DRAW: a null logits / zm_all / zs_all / pm / ps / zcat / comp_out, a null z_mean_xh / z_sig_xh while Ll > 0, ldz < Lg + Ll. */
int sv_iw_gm_advance(const float* logits, const float* zm_all, const float* zs_all, const float* pm, const float* ps,
                     const float* z_mean_xh, const float* z_sig_xh, const float* eps, const int32_t* comp, int32_t* comp_out,
                     void* zcat, int32_t z_dtype, int32_t ldz, float* r, const float* nll_x, const float* nll_xh, double* state,
                     int32_t B, int32_t n, int32_t Lg, int32_t Ll, int32_t k, uint64_t seed, int64_t sample_offset, int32_t flags,
                     void* stream);
/* the uniform of the component pick of (seed, global image index, sample k): no device needed */
float sv_iw_gm_uniform_host(uint64_t seed, int64_t image, int32_t sample);
/* The component tables of one batch, once per batch, in exact fp32 (sequential fma-free multiply-adds over the hidden index in
 * ascending order): h_top[c] = elu(w_ht[c,:] + b_ht); zm_all[b,c,:] = (he[b] + h_top[c]) . w_zm + b_zm; zs_all = softplus(the same
 * with w_zs, b_zs); pm[c,:] = w_pm[c,:] + b_pm; ps[c,:] = softplus(w_ps[c,:] + b_ps).  he [B, hidden] in he_dtype (the GM encoder's
 * buffer, row pitch hidden); w_ht [n, hidden], w_zm / w_zs [hidden, L], w_pm / w_ps [n, L]: the Keras kernels as they lie in the
 * flat parameter buffer.  SV_E_BADARG: a null pointer, B, L or hidden <= 0, n outside 1 .. 128, hidden > 1024, a he_dtype outside
 * sv_dtype. */
int sv_iw_gm_tables(const void* he, int32_t he_dtype, const float* w_ht, const float* b_ht, const float* w_zm, const float* b_zm,
                    const float* w_zs, const float* b_zs, const float* w_pm, const float* b_pm, const float* w_ps, const float* b_ps,
                    float* zm_all, float* zs_all, float* pm, float* ps, int32_t B, int32_t n, int32_t hidden, int32_t L, void* stream);

/* ---------------------------------------------------------------- k-NN label probe of the latents (csrc/knn.hip)
 * No reference counterpart: the probe classifier of vae/trainer.py:81-97 needs a weights blob that is missing upstream.  This is
 * the parameter-free representation metric instead: classify each query latent q [Nq, L] (row pitch ldq) by the majority label of
 * its k nearest reference latents r [Nr, L] (row pitch ldr, classes r_class [Nr] uint8).  fp32 only; ALL INPUTS ARE FINITE --
 * a NaN or Inf in q or r is the caller's error (the order below is not total then).
 *   norm         n(v) = sum_j v_j^2 in fp32, per row, computed once per row in a pre-pass in one fixed order (lane l of a wave
 *                sums j = l, l + 64, ... in ascending j, then the 64-lane xor butterfly 32, 16, ..., 1): it does not depend on
 *                where the row lies;
 *   distance     d(q, r) = max(0, (n(q) + n(r)) - 2 (q . r)), fp32 operations in that order; the dot product runs over the whole
 *                of L in ascending order on v_mfma_f32_16x16x4_f32 (exact fp32 fma chain, L zero-padded to a multiple of 32): no
 *                split over L, no atomics.  d(q, r) is therefore bit-identical whatever Nq, Nr, the rows' positions or the
 *                chunking;
 *   neighbours   the k references smallest under the total order (d, reference index): equal fp32 distances go to the lower
 *                index; reported in ascending order: nn_index [Nq, k] int32, nn_dist [Nq, k] fp32 (either may be NULL);
 *   prediction   pred [Nq] int32 = the class with the most votes among the k neighbours' r_class; vote ties go to the lowest
 *                class id: a function of the neighbour SET only.  Classes >= n_class get no votes.
 *   acc          (may be NULL) int64 [2] += (number of queries with pred == q_class, Nq); q_class NULL: only the count is added.
 *                Integer atomics: the sums do not depend on the order.  Zero it once per test set, read it back once.
 * The references are cut into chunks of sv_knn_chunk_rows() rows; a tile kernel leaves one sorted k-list per (query, chunk) in
 * the workspace and a second kernel merges them per query in chunk order.  The workspace (sv_knn_workspace_bytes; 16-byte aligned)
 * may hold anything on entry.  Everything is enqueued on `stream`; no host synchronisation.
 * Accepted domain: Nq >= 1, 1 <= k <= 32, k <= Nr <= 65535 chunks, 1 <= L <= 512, ldq, ldr >= L, 2 <= n_class <= 64: anything
 * else SV_E_UNSUPPORTED; a null q / r / r_class / pred / workspace or a misaligned pointer (4 bytes; acc 8; workspace 16):
 * SV_E_BADARG; workspace_bytes below sv_knn_workspace_bytes: SV_E_WORKSPACE.  All checked before anything is enqueued. */
int sv_knn_chunk_rows(void);     /* reference rows per chunk of the tile kernel: lets callers and tests size Nr */
int sv_knn_workspace_bytes(int32_t Nq, int32_t Nr, int32_t k, int64_t* bytes);
int sv_knn_classify(const float* q, int32_t ldq, const float* r, int32_t ldr, const uint8_t* r_class, int32_t Nq, int32_t Nr,
                    int32_t L, int32_t k, int32_t n_class, int32_t* nn_index /* [Nq,k] or NULL */,
                    float* nn_dist /* [Nq,k] or NULL */, int32_t* pred /* [Nq] */, const uint8_t* q_class /* or NULL */,
                    int64_t* acc /* [2]: hits, count; ADDED to; or NULL */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- aggregate-posterior information report (csrc/latent_info.hip)
 * No reference counterpart.  Hoffman & Johnson's decomposition ("ELBO surgery") of the average KL term into the index-code mutual
 * information and the marginal KL, per latent block, plus the mutual information of the two blocks under the aggregate posterior.
 * Needs no labels.  A block of width L has posterior means mu_j and standard deviations sig_j for the images j = 0 .. N-1; the two
 * blocks are concatenated: columns 0 .. Lg-1 are z_g, columns Lg .. Lg+Ll-1 are z_l (Ll = 0: one block).  fp32 inputs, ALL FINITE,
 * sig > 0.
 *   sample       z_i = mu_i + sig_i * eps_i (fp32, that expression).  eps [N, Lg+Ll] (row pitch lde) pins it; NULL: the library's
 *                Philox4x32-10 with a key constant of its own (seed ^ 0x1a7e27140f0) and counter (dimension j within its block,
 *                global image index sample_offset + b, 'li' tag | 0 global / 1 local, 0) and the Box-Muller of sv_iw_advance: a
 *                pure function of (seed, image, block, dimension), whatever batch the image sits in;
 *   row constant c_j = -sum_d log sig_jd - L/2 log(2 pi), the sum in fp64 over fp32 logf; cst [N,2] fp32 = (c^g_j, c^l_j);
 *   pair score   e_ij = c_j - 1/2 sum_d ((z_id - mu_jd) * rsig_jd)^2 with rsig = 1 / sig (fp32, correctly rounded), computed in this
 *                DIRECT form in fp32 -- subtract, multiply, fused multiply-add onto the running sum, d ascending within the block
 *                (zero-padded to a multiple of 32), then c_j - 0.5 * sum.  Only non-negative terms: the error is relative to the
 *                score.  (The expanded z^2.a - 2 z.b + c cancels ~1e5 against ~1e5 at sig ~ 1e-2.)  e^gl_ij = e^g_ij + e^l_ij (fp32);
 *   own term     own_i = c_i - 1/2 sum_d eps_id^2, in closed form from eps (fp64 sums): never taken from the pair loop;
 *   prior term   prior_i = -L/2 log(2 pi) - 1/2 sum_d z_id^2 (fp64 sums) = log N(z_i; 0, I);
 *   aggregate    lse_g[i] = logsumexp_j e^g_ij - log Nr, lse_l[i] likewise, lse_gl[i] = logsumexp_j (e^g_ij + e^l_ij) - log Nr;
 *   reported     per block KL = mean_i (own_i - prior_i), MI = mean_i (own_i - lse_i), marginal KL = mean_i (lse_i - prior_i), so
 *                KL = MI + marginal KL by construction; overlap I(z_g; z_l) = mean_i (lse_gl[i] - lse_g[i] - lse_l[i]); log N.
 *                Every MI-type figure saturates at log N: the known upward bias of this estimator.
 * sv_latent_info_draw: mu, sig [N, Lg+Ll] (row pitches ldm, lds) -> z (ldz), rsig (ldr), cst [N,2] fp32, own [N,2] and prior [N,2]
 *   fp64 (column 1 is 0 when Ll = 0).  One wave per image.
 * sv_latent_info_lse: queries z [Nq, Lg+Ll] against the references mu, rsig [Nr, Lg+Ll] and cst [Nr,2] -> lse [3, Nq] fp64: rows
 *   lse_g, lse_l, lse_gl (rows 1 and 2 are not written when Ll = 0).  Nq and Nr are independent.  The references are cut into chunks
 *   of sv_latent_info_chunk_rows() rows; a tile kernel leaves one fp32 (max, sum) per (query, chunk, sum) in the workspace
 *   (sv_latent_info_workspace_bytes; 16-byte aligned; may hold anything on entry) and a merge kernel folds them per query in chunk
 *   order in fp64.  No atomics: the same inputs give the same bits, wherever a query row sits.
 * sv_latent_info_finish: own, prior [N,2], lse [3,N] of Nq = Nr = N -> out [8] fp64 = (KL_g, MI_g, marginal KL_g, KL_l, MI_l,
 *   marginal KL_l, overlap, log N), the means summed in one fixed order by one workgroup (thread t takes the images t, t + 256, ... in
 *   ascending order, then the 256 partial sums are added in thread order: deterministic); entries 3 .. 6 are 0 when Ll = 0.  One
 *   read-back per evaluation.
 * Everything is enqueued on `stream`; no host synchronisation.  Accepted domain: 1 <= Lg <= 512, 0 <= Ll <= 512, N, Nq, Nr >= 1 (Nr
 * at most 65535 chunks), row pitches >= Lg + Ll, sample_offset >= 0: anything else SV_E_UNSUPPORTED; a null pointer (eps may be
 * NULL) or a misaligned one (4 bytes; fp64 arrays 8; workspace 16): SV_E_BADARG; workspace_bytes below
 * sv_latent_info_workspace_bytes: SV_E_WORKSPACE.  All checked before anything is enqueued. */
int sv_latent_info_chunk_rows(void);
int sv_latent_info_workspace_bytes(int32_t Nq, int32_t Nr, int64_t* bytes);
int sv_latent_info_draw(const float* mu, int32_t ldm, const float* sig, int32_t lds, const float* eps /* or NULL */, int32_t lde,
                        float* z, int32_t ldz, float* rsig, int32_t ldr, float* cst /* [N,2] */, double* own /* [N,2] */,
                        double* prior /* [N,2] */, int32_t N, int32_t Lg, int32_t Ll, uint64_t seed, int64_t sample_offset,
                        void* stream);
int sv_latent_info_lse(const float* z, int32_t ldz, const float* mu, int32_t ldm, const float* rsig, int32_t ldr, const float* cst,
                       int32_t Nq, int32_t Nr, int32_t Lg, int32_t Ll, double* lse /* [3,Nq] */, void* workspace,
                       int64_t workspace_bytes, void* stream);
int sv_latent_info_finish(const double* own, const double* prior, const double* lse, int32_t N, int32_t Ll, double* out /* [8] */,
                          void* stream);

/* ---------------------------------------------------------------- per-dimension latent report (csrc/latent_dims.hip)
 * No reference counterpart.  Which dimensions of a latent block carry anything (Burda et al. 2016: active units) and Chen et al.
 * 2018's decomposition of the block's KL term into index-code MI, total correlation and dimension-wise KL, from scores under the
 * per-dimension aggregate posterior q_j(z_j) = 1/N sum_n q(z_j | x_n).  One block of width L per call (a column range of the
 * arrays of sv_latent_info_draw, addressed by base pointer and row pitch), N images, one sample z_i per image: the bits
 * sv_latent_info_draw writes.  fp32 inputs, ALL FINITE, sig > 0, taken exactly.
 *   lc_nj    = -log sig_nj - 1/2 log(2 pi): fp32, (float)(-(double)logf(sig) - 1/2 log 2 pi); an INPUT of sv_latent_dims_lse;
 *   e_inj    = lc_nj - 1/2 ((z_ij - mu_nj) * rsig_nj)^2 in this DIRECT form in fp32: subtract, multiply, square, then one rounding
 *              of lc - 0.5 * square.  Only non-negative terms, as in sv_latent_info_lse;
 *   lse_ij   = logsumexp_n e_inj - log Nr;
 *   own_ij   = lc_ij - 1/2 eps_ij^2 (fp64, from the fp32 lc: the rounding of lc cancels in own - lse);
 *   prior_ij = -1/2 log(2 pi) - 1/2 z_ij^2 (fp64);
 *   per dimension  mean_j, var_j: the mean and the POPULATION variance of mu_.j over the images (fp64, two passes); a dimension
 *              is active when var_j > 0.01 (Burda et al.'s threshold: the caller's comparison);
 *              KL_j = mean_i [1/2 (mu_ij^2 + sig_ij^2 - 1) - log sig_ij]: the closed form, fp64 throughout;
 *              MI_j = mean_i (own_ij - lse_ij), dwKL_j = mean_i (lse_ij - prior_ij), mlse_j = mean_i lse_ij;
 *   per block  TC = mean_i lse_block_i - sum_j mlse_j (= mean_i (lse_block_i - sum_j lse_ij)), lse_block: row 0 (z_g) or 1 (z_l) of
 *              sv_latent_info_lse on the same z; dwKL = sum_j dwKL_j.  With KL and MI of sv_latent_info_finish on the same draws
 *              KL = MI + TC + dwKL holds term by term (the sums telescope).  Every MI-type figure saturates at log N.
 * sv_latent_dims_prepare: mu, sig [N, L] (pitches ldm, lds) -> lc [N, L] fp32 (ldc), own [N, L] fp64 (dense) and cols [3, L] fp64 =
 *   (mean_j, var_j, KL_j).  eps [N, L] (lde) pins the draw; NULL: the Philox stream of sv_latent_info_draw at (seed, sample_offset + i,
 *   block: 0 global / 1 local, j), the same numbers that call drew.  Column sums: one workgroup per dimension, thread t takes the
 *   images t, t + 256, ... in ascending order, then the 256 partial sums are added in thread order.  No atomics.
 * sv_latent_dims_lse: queries z [Nq, L] (ldz) against the references mu, rsig, lc [Nr, L] (ldm, ldr, ldc) -> lse [Nq, L] fp64 (row
 *   pitch ldl).  Nq and Nr are independent.  The references are cut into chunks of sv_latent_dims_chunk_rows() rows; within a chunk
 *   they are pushed onto a per-(query, dimension) running (max, sum) in groups of 8 consecutive rows (the group's maximum, one
 *   rescale of the sum, then one exponential per element, added in row order); one fp32 (max, sum) per (query, chunk, dimension)
 *   is left in the workspace (sv_latent_dims_workspace_bytes; 16-byte aligned; may hold anything on entry) and a merge kernel folds
 *   them in chunk order in fp64.  The Nq x Nr x L scores never exist in memory.  No atomics.  lse_ij depends on row i of z and
 *   column j of the references only: the same inputs give the same bits wherever the query row or the column sits.
 * sv_latent_dims_finish: lse [N, L] (ldl), own [N, L] (dense), z [N, L] (ldz), lse_block [N] -> out [3 L + 2] fp64 = (MI_j [L],
 *   dwKL_j [L], mlse_j [L], TC, dwKL).  The means in the fixed order of sv_latent_dims_prepare's column sums; TC and dwKL add
 *   the dimensions in ascending order.
 * Everything is enqueued on `stream`; no host synchronisation.  Accepted domain: 1 <= L <= 512, N, Nq, Nr >= 1 (Nr at most 65535
 * chunks), row pitches >= L, block 0 or 1, sample_offset >= 0: anything else SV_E_UNSUPPORTED; a null pointer (eps may be NULL) or
 * a misaligned one (4 bytes; fp64 arrays 8; workspace 16): SV_E_BADARG; workspace_bytes below sv_latent_dims_workspace_bytes:
 * SV_E_WORKSPACE.  All checked before anything is enqueued. */
int sv_latent_dims_chunk_rows(void);
int sv_latent_dims_workspace_bytes(int32_t Nq, int32_t Nr, int32_t L, int64_t* bytes);
int sv_latent_dims_prepare(const float* mu, int32_t ldm, const float* sig, int32_t lds, const float* eps /* or NULL */, int32_t lde,
                           float* lc, int32_t ldc, double* own /* [N,L] */, double* cols /* [3,L] */, int32_t N, int32_t L,
                           int32_t block, uint64_t seed, int64_t sample_offset, void* stream);
int sv_latent_dims_lse(const float* z, int32_t ldz, const float* mu, int32_t ldm, const float* rsig, int32_t ldr, const float* lc,
                       int32_t ldc, int32_t Nq, int32_t Nr, int32_t L, double* lse, int32_t ldl, void* workspace,
                       int64_t workspace_bytes, void* stream);
int sv_latent_dims_finish(const double* lse, int32_t ldl, const double* own, const float* z, int32_t ldz, const double* lse_block,
                          int32_t N, int32_t L, double* out /* [3 L + 2] */, void* stream);

/* ---------------------------------------------------------------- label-free reconstruction quality (csrc/recon_quality.hip)
 * The three decodes of the reference's labelled test step (vae/trainer.py:213-226: the reconstruction, decode(z_x, random z_l) and
 * decode(random z_g, z_x_hat)) scored in image space instead of by the classifier whose weights are missing upstream: mean PSNR and
 * mean SSIM against the original image.  The project's own stand-in for Table 1, as the k-NN probe is; needs no labels.
 *   images       reference a = (x + 1) * 0.5 from channels 0..2 of the six-channel batch; decode b = clip((x_mean + 1) * 0.5, 0, 1),
 *                which is decode(rescale=True) (vae/model.py:215), from channels 0..2 of the plan's out6_x; max_val = 1.  Both are
 *                NHWC fp32 and read IN PLACE: base pointer, pixel pitch in floats, channel offset (three channels from there).
 *   PSNR         per image 10 log10(1 / max(MSE_i, 1e-10)), MSE_i over H*W*3 (the tf.image.psnr convention; the floor only keeps an
 *                exact copy finite: 100 dB); reported: the mean over images.
 *   SSIM         the defaults of tf.image.ssim (Wang et al. 2004): 11 x 11 Gaussian window of sigma 1.5 normalised to sum 1
 *                (separable: the outer product of sv_recon_window's 11 fp64 taps), population moments mu_a, mu_b, var_a = E[a^2] -
 *                mu_a^2, var_b, cov = E[a b] - mu_a mu_b, C1 = 0.01^2, C2 = 0.03^2,
 *                ((2 mu_a mu_b + C1)(2 cov + C2)) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2)) over the VALID region only,
 *                (H-10) x (W-10) windows, per channel; per image the mean over windows and the three channels; reported: the mean
 *                over images.
 *   arithmetic   every pixel is converted to fp64 when it is loaded and everything after that is fp64 (the rescale and the clip are
 *                then exact): the moments' cancellation leaves ~1e-15 against C2 = 9e-4.
 *   kept blocks  are the posterior MEANS (the reference keeps a posterior sample z_x / z_x_hat): the figures are a function of the
 *                weights and the seed alone.
 *   drawn blocks eps [B, Lg+Ll] (row pitch lde) pins the normals; NULL: Philox4x32-10 with a key constant of this report's own
 *                (seed ^ 0x1a7e2c0a11f7) and counter (dimension j within its block, global image index sample_offset + b, 'rq' tag |
 *                mode << 4 | 0 global / 1 local, 0) and the Box-Muller of sv_iw_advance: image i draws the same numbers whatever batch
 *                it sits in.  The global block's prior is N(0, I) when pm, ps are NULL; otherwise the uniform mixture over the n rows
 *                of pm, ps [n, Lg] (encode_y of the identity, vae/model.py:263-265): z_g = pm[c] + ps[c] * eps (fp32: one multiply,
 *                one add), c = comp[b] clamped to 0..n-1, or with comp NULL floor(u32 * n / 2^32) of the first word of counter
 *                (0, image, tag | 2, 0).
 * sv_recon_draw: zcat [B, Lg+Ll] (row pitch ldz, dtype SV_F32 or SV_BF16: fp32 rounded to nearest even) = [z_g | z_l].
 *   SV_RECON_MEANS: both blocks are z_mean_x [B,Lg] (ldg), z_mean_xh [B,Ll] (ldl); SV_RECON_KEEP_G: z_l is drawn from N(0, I);
 *   SV_RECON_KEEP_L: z_g is drawn from its prior.  Ll = 0 is the one-branch model (z_mean_xh may be NULL).  One wave per image.
 * sv_recon_quality: per_image [B,2] fp64 = (MSE_i, SSIM_i) of a against b (clip_b != 0: b is clipped to [0,1] after the rescale; a
 *   never is).  Work is split over (image, band of 8 output rows, tile of up to 75 output columns); each tile leaves one fp64 pair in
 *   the workspace (sv_recon_quality_workspace_bytes; 8-byte aligned; may hold anything on entry) and one thread per image adds them in
 *   tile order.  Outputs are overwritten.  No atomics: the same inputs give the same bits.
 * sv_recon_finish: acc [3] fp64 += (sum_i PSNR_i, sum_i SSIM_i, B) over per_image [B,2], added onto the accumulator in image order
 *   by one thread (the caller zeroes acc once; one accumulator per variant, read back once per evaluation).
 * Everything is enqueued on `stream`; no host synchronisation.  Accepted domain: B >= 1, 11 <= H, W <= 16384, B * tiles < 2^31,
 * 0 <= offset, offset + 3 <= pitch <= 4096, 1 <= Lg <= 512, 0 <= Ll <= 512, 1 <= n <= 4096, row pitches >= their widths,
 * sample_offset >= 0, a known mode and dtype: anything else SV_E_UNSUPPORTED; a null pointer (eps, comp, pm and ps may be NULL, pm and
 * ps only together; z_mean_xh when Ll = 0) or a misaligned one: SV_E_BADARG; workspace_bytes too small: SV_E_WORKSPACE.  All checked
 * before anything is enqueued. */
enum { SV_RECON_MEANS = 0, SV_RECON_KEEP_G = 1, SV_RECON_KEEP_L = 2 };
void sv_recon_window(double* w /* [11] */);
int sv_recon_quality_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes);
int sv_recon_draw(const float* z_mean_x, int32_t ldg, const float* z_mean_xh /* or NULL */, int32_t ldl, int32_t mode,
                  const float* eps /* or NULL */, int32_t lde, const int32_t* comp /* [B] or NULL */, const float* pm /* or NULL */,
                  const float* ps /* or NULL */, int32_t n, void* zcat, int32_t ldz, int32_t dtype, int32_t B, int32_t Lg, int32_t Ll,
                  uint64_t seed, int64_t sample_offset, void* stream);
int sv_recon_quality(const float* a, int32_t pitch_a, int32_t off_a, const float* b, int32_t pitch_b, int32_t off_b, int32_t clip_b,
                     int32_t B, int32_t H, int32_t W, double* per_image /* [B,2] */, void* workspace, int64_t workspace_bytes,
                     void* stream);
int sv_recon_finish(const double* per_image /* [B,2] */, int32_t B, double* acc /* [3] */, void* stream);

/* ---------------------------------------------------------------- SPLIT-SPAIR: Dense layers, exact fp32 on the matrix cores
 * tf.keras.layers.Dense (spair/spair.py:135-154, :185-202, :246-273, :341-366, :424-467) for ANY fan-in / fan-out, reading the Keras
 * [in, out] kernel as it lies in the variable buffer (dense_f32.hip).  x [M, ldx], y / dy [M, ldy], w [K, N] row-major.
 *   fwd:   y = act(x . w + bias)                       act: SV_ACT_NONE | SV_ACT_RELU
 *   dgrad: dx = dy . w^T (accumulate != 0: added to dx with atomics, K may be split over workgroups)
 *   wgrad: dw += x^T . dy, dbias += column sums of dy (atomics onto the zeroed gradients; dbias may be NULL) */
int sv_dense_f32_fwd(const float* x, int32_t ldx, const float* w, const float* bias, float* y, int32_t ldy, int32_t M, int32_t K,
                     int32_t N, int32_t act, void* stream);
int sv_dense_f32_dgrad(const float* dy, int32_t ldy, const float* w, float* dx, int32_t ldx, int32_t M, int32_t K, int32_t N,
                       int32_t accumulate, void* stream);
int sv_dense_f32_wgrad(const float* x, int32_t ldx, const float* dy, int32_t ldy, float* dw, float* dbias, int32_t M, int32_t K,
                       int32_t N, void* stream);

/* ---------------------------------------------------------------- the latent block's kernels, one by one (csrc/latent_gemm.hip)
 * Direct access for tests and host bindings to the kernels sv_lgvae_step runs between the encoder convs and the decoder convs: the Dense
 * layers e4_mean | e4_sd (vae/model.py:41-42) and d1 (:152), their input and weight gradients, and the twin Sampling + KL kernels that read
 * the GEMMs' K-slice slabs.  Thin wrappers: they add no kernel and no launch of the step goes through them.  Every argument is checked before
 * anything is enqueued; a refused call leaves every buffer untouched.  `dtype` is the sv_dtype of the operands (SV_BF16: bf16 operands, fp32
 * accumulate; SV_F32: exact fp32 products and sums).  All of a launch's problems share it.
 *
 * sv_latent_nt_gemm: out [M, N] = A [M, K] . W^T for n = 1 or 2 problems in one launch.  A [M][lda] and the weight image W [N][ldw] are
 *   K-contiguous, in `dtype`.
 *   out_f32 = 0 (needs splitk = 1): out [M][ldo] in `dtype` = gate(act(product + bias)); bias [N] fp32 or NULL, act SV_ACT_NONE | SV_ACT_RELU,
 *     mask [M][ldo] in `dtype` or NULL: elements whose mask is not > 0 are stored as zero (ReluGrad of the tensor the gradient lands on).
 *   out_f32 = 1: out = fp32 slabs [splitk][M][ldo], slab s at out + s * slab_stride floats = the product over K slice s alone; bias, act and
 *     mask are ignored (they belong to the consumer of the summed slabs).
 *   splitk = 0 on entry: replaced by sv_latent_nt_pick_splitk(M, N, K, n), the plan's choice; on return p[i].splitk is what ran.
 *   bm = 64 | 128 rows per tile (the plan: 128 from B >= 256 for typed outputs, 64 for slabs).  *form (may be NULL) = the kernel that was
 *     launched: 0 = nt_gemm_kernel (one LDS slot), 1 = nt_gemm_ring_kernel (three slots; bm = 64, every problem out_f32 with slices of two
 *     or more phases, a phase being 128 (bf16) or 64 (fp32) of K).
 *   Rows >= M, columns [N, ldo) and everything behind the last slab are not written.
 *   SV_E_BADARG: p NULL, n outside 1..2, bm not 64 | 128, a dtype outside sv_dtype, a null A / W / out, M < 1, lda or ldw < K, ldo < N,
 *     splitk < 0, an act outside NONE | RELU.  SV_E_UNSUPPORTED: N or the K of a slice no multiple of 128 (N) / a phase (K), K % splitk != 0,
 *     lda / ldw no multiple of the elements of 16 bytes, ldo % 4 != 0, A / W / out / bias / mask not 16-byte aligned, splitk > 1 without
 *     out_f32 (every slice would store its own partial product over the others'), out_f32 with a slab_stride that is no multiple of 4 floats
 *     or below M * ldo (slabs would overlap). */
typedef struct {
  const void* A; int32_t lda;
  const void* W; int32_t ldw;
  void* out; int32_t ldo;
  const float* bias;
  const void* mask;
  int32_t M, N, K, act, splitk, out_f32;
  int64_t slab_stride;
} sv_latent_nt_prob;
int sv_latent_nt_gemm(sv_latent_nt_prob* p, int32_t n, int32_t dtype, int32_t bm, int32_t* form, void* stream);
/* K slices the plan gives a big-K layer of `nprob` problems per launch (host logic, no device): 1 <= s <= K / 128, K % s == 0,
 * (K / s) % 128 == 0; 1 for a shape the kernels do not take. */
int32_t sv_latent_nt_pick_splitk(int32_t M, int32_t N, int32_t K, int32_t nprob);
/* out [M][ldo] = 0.f + slab 0 + slab 1 + ... + slab S-1 in fp32, in that order, for n = 1 or 2 problems in one launch (all M * ldo floats
 * of a slab are read).  SV_E_BADARG: a null pointer, n outside 1..2, S < 1, M < 1, ldo < 1; SV_E_UNSUPPORTED: ldo or slab_stride no
 * multiple of 4 floats, a pointer not 16-byte aligned. */
typedef struct { const float* slabs; float* out; int32_t S, M, ldo; int64_t slab_stride; } sv_latent_reduce_prob;
int sv_latent_nt_slab_reduce(const sv_latent_reduce_prob* p, int32_t n, void* stream);
/* Weight gradients dW [Kw, N] = X^T . dY (rows [0, Kw_real) stored, row pitch N; ASSIGNED) and, unless dbias is NULL, dbias [N] = column sums
 * of dY, for n = 1 .. 4 problems in one launch.  X [M][ldx] (columns [0, Kw) read) and dY [M][ldy] (columns [0, N) from the pointer) in
 * `dtype`; the contraction runs over the M rows.  SV_E_BADARG: p NULL, n outside 1..4, a dtype outside sv_dtype, a null X / dY / dW,
 * ldx < Kw, ldy < N; SV_E_UNSUPPORTED: M no positive multiple of 32, Kw or N no positive multiple of 128, Kw_real outside 1..Kw, ldx / ldy
 * no multiple of the elements of 16 bytes, X / dY not 16-byte aligned. */
typedef struct { const void* X; int32_t ldx; const void* dY; int32_t ldy; float* dW; float* dbias; int32_t M, Kw, Kw_real, N; } sv_latent_tn_prob;
int sv_latent_tn_wgrad(const sv_latent_tn_prob* p, int32_t n, int32_t dtype, void* stream);
/* Both networks' Sampling + KL in one launch (a[0] = x, a[1] = x-hat; sv_reparam_kl_fwd each, Philox stream id = the index), as the plan calls
 * it.  S > 0: `pre` is the first of S K-slice slabs [B][2L] fp32, slab_stride floats apart, summed in the kernel as sv_latent_nt_slab_reduce
 * sums them (the same bits as reduce + sv_reparam_kl_fwd); S = 0: `pre` [B][2L] itself.  z_lp [B][ldz] in z_dtype is shared: network e writes
 * columns [z_col, z_col + L).  SV_E_BADARG: a NULL, B <= 0, a z_dtype outside sv_dtype, per network a null pre / bias_mean / bias_sd / z_mean /
 * z_sig / z / kl, L <= 0, S < 0, z_col < 0 or z_col + L > ldz; z_lp NULL. */
typedef struct {
  const float *pre, *bias_mean, *bias_sd, *eps;   /* eps NULL: Philox, written to eps_out */
  float *eps_out, *z_mean, *z_sig, *z, *kl;       /* eps_out may be NULL */
  int32_t L, z_col, S;
  int64_t slab_stride;
} sv_reparam_twin_fwd;
int sv_reparam_kl_fwd_twin(const sv_reparam_twin_fwd* a, void* z_lp, int32_t z_dtype, int32_t ldz, int32_t B, uint64_t seed, uint64_t step,
                           int64_t sample_offset, void* stream);
/* The adjoints of both networks in one launch (sv_reparam_kl_bwd each).  S > 0: dz is the first of S slabs (row pitch ld_dz, `stride` floats
 * apart) and dz2, unless NULL, the first of S2 slabs (ld_dz2, stride2); each set is summed from 0.f in slice order and the two sums are then
 * added.  S = 0: plain tensors.  g_pre [B][2L] in g_dtype.  SV_E_BADARG: a NULL, B <= 0, a g_dtype outside sv_dtype, per network a null dz /
 * z_mean / z_sig / eps / g_pre, L <= 0, S < 0, ld_dz < L, with dz2: ld_dz2 < L, and with dz2 and S > 0: S2 < 1. */
typedef struct {
  const float *dz, *dz2, *z_mean, *z_sig, *eps;
  void* g_pre;
  int32_t ld_dz, ld_dz2, L, S, S2;
  int64_t stride, stride2;
} sv_reparam_twin_bwd;
int sv_reparam_kl_bwd_twin(const sv_reparam_twin_bwd* a, float kl_scale, int32_t g_dtype, int32_t B, void* stream);

/* ---------------------------------------------------------------- SPLIT-SPAIR: the train step as one native launch sequence
 * Replaces, for spair/: SPAIR.call / LGSPAIR.call (spair/spair.py:35-49, :84-106), the loss assembly and tape.gradient of train_step
 * (spair/trainer.py:136-228) and optimizer.apply_gradients (:226-227, spair/main.py:109).  The host records the model ONCE as a list
 * of nodes over fp32 2-D tensors [rows, cols | row pitch ld floats] (split_vae_amd/spair_native.py mirrors the reference's classes);
 * sv_tape_run walks it forwards and backwards natively: no Python, autograd engine or library GEMM between the launches (tape.hip).
 * Tensor ids index the tape's tensors; *_off are float offsets into the flat variable / gradient buffers (-1: none). */
typedef struct sv_tape sv_tape;
enum { SV_TAPE_DENSE = 0, SV_TAPE_CONV, SV_TAPE_UNARY, SV_TAPE_SAMPLE, SV_TAPE_LOGITNOISE, SV_TAPE_UPSAMPLE, SV_TAPE_STN, SV_TAPE_RENDER,
       SV_TAPE_ZPRES, SV_TAPE_LOSS, SV_TAPE_NOISE };
enum { SV_TAPE_COPY = 0, SV_TAPE_RELU, SV_TAPE_SIGMOID, SV_TAPE_SOFTPLUS /* softplus(x + p0) */, SV_TAPE_CLAMP /* [p0, p1] */,
       SV_TAPE_SCALE /* p0 * x */ };
enum { SV_TAPE_PHASE_FORWARD = 1, SV_TAPE_PHASE_BACKWARD = 2, SV_TAPE_PHASE_ADAM = 4 };
typedef struct {
  int32_t kind;                 /* SV_TAPE_* node kind */
  int32_t x, y, t2, t3, t4, t5, t6;   /* tensors: main input, output, extra inputs (-1: none); per kind:
      DENSE       y[M,N] = act(x[M,K] . W + b)                         (Dense; also the backbone's 1x1 convolutions)
      CONV        y = act(conv2d_same(x, W) + b); B,H,W,C = input extent, Cout, k, stride       (spair/spair.py Conv2D layers)
      UNARY       y[:, yo:yo+n] = op(x[:, xo:xo+n]), `rep` output rows per input row (tf.tile / concat / slice / activations)
      SAMPLE      y[:, yo:] = x[:, xo:] + t2[:, o2:] * t3[:, o3:]      (Sampling, spair/utils.py:19-24: mean, sig, eps)
      LOGITNOISE  y = (x + log(t2 + 1e-8) - log(1 - t2 + 1e-8)) / p0   (concrete_binary_pre_sigmoid_sample, spair/utils.py:14-17)
      UPSAMPLE    y = tf.image.resize(x, 2x) on [B,H,W,C=ld]           (spair/spair.py:175-180, :360-364)
      STN         y (, t3 = obj_bbox_mask) = STN(x = images, t2 = z_where [B*Hc*Wc,4]); B,H,W,C input, Ho,Wo output, Hc,Wc cells, inverse
      RENDER      y = Renderer(x = objects, t2 = bg, t3 = z_depth, t4 = z_pres, t5 = z_pres_logits, t6 = GaussianNoise draw (-1)); R cells
      ZPRES       loss[loss_idx] = compute_z_pres_kl_yolo_air(x = z_pres, t2 = logits, t3 = pre_sigmoid); prior_prob = dyn[dyn_idx], p0 = tau
      LOSS        loss[loss_idx] = per-image sums of mode 0 xent(x = label, t2 = pred) | 1 kl(x = mean, t2 = sig) | 2 kl vs N(dyn[dyn_idx] | p0, p1)
                  over rows [b*R, (b+1)*R) x columns [xo | o2, +n)
      NOISE       y <- Philox draws, op 0: normal * p0, 1: uniform (skipped when the run pins the noise tensors) */
  int32_t xo, yo, o2, o3;       /* column offsets */
  int32_t n, rep, op, act;
  float p0, p1;
  int64_t w_off, b_off;
  int32_t B, H, W, C, Cout, k, stride, Ho, Wo, Hc, Wc, inverse, training;
  int32_t loss_idx, dyn_idx, mode, R, stream_id;
  int32_t group;                /* UNARY: consecutive nodes with the same non-zero group are independent of each other and run as ONE launch (at most 8 per launch).
                                   Parts may READ the same source columns (a tile of z into two places): their adjoints then run one launch per part, in tape
                                   order reversed, because they add into the same gradient */
  int32_t lane;                 /* 0: the caller's stream; 1..3: a HIP stream of the tape's own.  Independent branches of the model (LG-SPAIR's x-hat / background
                                   networks beside the object pipeline, spair/spair.py:84-104) recorded on another lane run concurrently with lane 0; sv_tape_finalize
                                   derives every cross-lane dependency from the nodes' tensors and sv_tape_run orders conflicting accesses in tape order with events,
                                   so any lane assignment computes the single-stream step bit for bit (SV_TAPE_LANES=0: everything on the caller's stream) */
} sv_tape_node;
typedef struct {
  float* params;                /* flat fp32 variables (updated by the ADAM phase) */
  float* grads;                 /* flat fp32 gradients, same layout (zeroed and filled by the BACKWARD phase) */
  const float* loss_weights;    /* HOST array [n_weights]: total = sum_i loss_weights[i] * mean_b loss_i (spair/trainer.py:165-207) */
  int32_t n_weights;
  float dyn[8];                 /* step-dependent scalars the nodes reference (prior_z_pres_prob, the zoom prior's mean: :153, :156) */
  uint64_t seed, step;          /* Philox key of the NOISE nodes */
  int32_t pinned_noise;         /* != 0: the caller filled the noise tensors (tests) */
  int32_t phases;               /* SV_TAPE_PHASE_* */
  int32_t accumulate_metrics;
  float* adam_m; float* adam_v; int64_t n_params;
  float lr, beta1, beta2, adam_eps; int64_t t;
  float clipnorm;               /* > 0: tf.clip_by_norm per variable before the update (TF >= 2.4 apply_gradients); 0: plain Keras Adam */
  const int64_t* tensor_off; int32_t n_tensors; float* norm_ws;   /* clipnorm only: device [n_tensors + 1] offsets, [n_tensors * 256] floats */
} sv_tape_run_args;
int sv_tape_create(sv_tape** out, int32_t batch, int32_t conv_dtype);
void sv_tape_destroy(sv_tape* t);
int32_t sv_tape_tensor(sv_tape* t, int64_t rows, int32_t cols, int32_t ld, int32_t need_grad);       /* -> tensor id (>= 0) or SV_E_* */
int32_t sv_tape_view(sv_tape* t, int32_t src, int64_t rows, int32_t cols, int32_t ld);               /* same storage, other 2-D shape */
int sv_tape_add(sv_tape* t, const sv_tape_node* node);
/* What a finalized tape launches: one step list per pass (0 forward, 1 backward) in issue order; sv_tape_run walks exactly these lists (wait, launch, record).
 *   Forward: the nodes in tape order, each one SV_TAPE_PART_ALL step on its node's lane (lanes above the SV_TAPE_LANES cap fold onto the cap); consecutive UNARY
 *     nodes of one non-zero group and one lane, at most 8, are ONE step over nodes first..last.
 *   Backward: the same units in reverse order, each one SV_TAPE_PART_ALL step, except the hand-off: on a tape with more than one lane, a lane-0 node whose input x
 *     has a gradient and which is a DENSE node, or a CONV node of a bf16 tape, runs its adjoint as up to three steps, in this order --
 *       PRE   on lane 0: the CONV's in-place ReLU gate of dY and the bf16 cast of dY (a DENSE node launches nothing here: no PRE step),
 *       WGRAD on lane 1: the weight and bias gradients, which feed only Adam,
 *       DGRAD on lane 0: the input gradient, the critical path of the adjoint.
 * A step's stream first waits for the events of the steps waits[0 .. n_waits) -- indices into the same pass's list, all < k -- and, when `records` is 1, records
 * its own event behind its launches for a later step of another lane.  sv_tape_finalize derives the waits from what every step reads and writes (activations,
 * gradients, variable gradients, a CONV's bf16 copy of dY, a lane's weight-gradient slab region), so every pair of conflicting steps on different lanes keeps the
 * tape's order.  A single-lane tape has step lists too: SV_TAPE_PART_ALL only, no waits, no records.  Host logic only -- no GPU needed.
 * sv_tape_steps: the number of steps, or SV_E_BADARG (not finalized, pass outside 0..1).  sv_tape_step_info: step k into *out and its first max_waits wait indices
 * into waits (may be NULL); SV_E_BADARG: not finalized, pass outside 0..1, k outside the list, out NULL. */
enum { SV_TAPE_PART_ALL = 0, SV_TAPE_PART_PRE, SV_TAPE_PART_WGRAD, SV_TAPE_PART_DGRAD };
typedef struct { int32_t first, last, part, lane, records, n_waits; } sv_tape_step;
int sv_tape_steps(const sv_tape* t, int32_t pass);
int sv_tape_step_info(const sv_tape* t, int32_t pass, int32_t k, sv_tape_step* out, int32_t* waits, int32_t max_waits);
/* reported[j] = sum_i matrix[j * 16 + i] * mean_b loss_i: the `losses` list of train_step (spair/trainer.py:158-160, :208-216) */
int sv_tape_set_report(sv_tape* t, const float* matrix, int32_t n_report);
/* SV_E_UNSUPPORTED: two DENSE / CONV nodes name the same w_off, or the same b_off >= 0 (a layer's adjoint ASSIGNS its variables' gradients: one writer each) */
int sv_tape_finalize(sv_tape* t);
int64_t sv_tape_workspace_bytes(const sv_tape* t);
int sv_tape_bind(sv_tape* t, void* workspace, int64_t bytes, void* stream);                           /* zero-fills the workspace */
int sv_tape_tensor_info(const sv_tape* t, int32_t id, int64_t* offset, int64_t* grad_offset);        /* byte offsets (-1: no gradient) */
/* out block (floats): [total, reported x 16, mean loss_i x 16]; metric block: running sums of [total, reported x 16], then the count */
int sv_tape_loss_info(const sv_tape* t, int64_t* out_offset, int64_t* metric_offset, int32_t* n_loss);
int sv_tape_run(sv_tape* t, const sv_tape_run_args* args, void* stream);

/* ---------------------------------------------------------------- k-means cluster report of the latents (csrc/kmeans.hip)
 * No reference counterpart: the unsupervised companion of the k-NN probe.  Lloyd's k-means on x [N, L] fp32 (row pitch ldx), R
 * independent restarts in one pass, k-means++ seeding.  ALL INPUTS ARE FINITE.
 *   norm, distance  exactly sv_knn_classify's: n(v) per row in that fixed order; d(x, c) = max(0, (n(x) + n(c)) - 2 (x . c)), fp32
 *                operations in that order, the dot product over the whole of L in ascending order on v_mfma_f32_16x16x4_f32 (L
 *                zero-padded, no split over L, no atomics): d is bit-identical wherever the row or the centroid sits;
 *   assignment   a_i = the centroid smallest under the total order (d, centroid index): equal fp32 distances go to the lower index;
 *                the padded columns of a tile never win;
 *   seeding      k-means++ as an exponential race, per restart r.  Philox4x32-10 with the key seed ^ 0x1a7e3c105fe5 and the tag
 *                'km' << 16: the first centre is the row (uint64(w) * N) >> 32, w the first word at counter (0, r, 0, tag).  With m_i
 *                the fp32 distance of row i to the nearest centre chosen so far, centre k >= 1 is the row smallest under (key_i, i),
 *                key_i = -logf(u_i) / m_i in fp32, u_i in (0, 1] from the first word at counter (i, r, k, tag) (((w >> 8) + 1) 2^-24),
 *                key_i = +inf where m_i = 0; all keys +inf: row 0.  P(i) is proportional to m_i (the D^2 rule); the pick is an argmin
 *                under a total order and does not depend on the grid.  A centre is a copy of its row;
 *   update       per cluster count_k (int32) and sum_k in fp64 in one fixed order that depends on N and sv_kmeans_chunk_rows() alone:
 *                a chunk is 8 runs of sv_kmeans_chunk_rows() / 8 rows; the rows of a run in ascending order, the runs of a chunk in
 *                ascending order, then the chunks in ascending order.  c_k = (float)(sum_k / count_k); an
 *                empty cluster keeps its centroid.  No floating-point atomics;
 *   fit          from centroids C_0, for t = 0, 1, ...: assign against C_t; stop if t > 0 and no assignment changed, or if t == T;
 *                otherwise update to C_{t+1}.  assign, counts and inertia are those of the last assign pass and the centroids are the
 *                ones that pass was made against.  inertia = sum_i d(x_i, c_{a_i}), the fp32 distances summed in fp64 in a fixed order
 *                (the rows of a 64-row tile ascending, then the tiles: lane l of a wave takes the tiles l, l + 64, ..., then the lanes
 *                in lane order).  n_iter = the t at which the restart stopped.  Past a fixed point an iteration reproduces the same
 *                bits, so a converged restart rides along until every restart has converged: only its n_iter is frozen.  From then on
 *                the launches of the fit return at once;
 *   best         the restart with the lowest inertia, ties to the lower r.
 * sv_kmeans_seed: centroids [R, K, L] fp32 <- the K centres of every restart; picks [R, K] int32 (may be NULL) <- their rows.
 * sv_kmeans_iterate: resume = 0 starts a fit at the given centroids: one assign pass (t = 0), then `iters` times update + assign, so
 *   T = iters; resume = 1 continues the fit whose centroids / assign / counts / n_iter / state the previous call left, with `iters`
 *   more update + assign steps: calls in groups give the bits of one call with the total.  iters = 0, resume = 0: one assign pass.
 *   centroids [R, K, L] in-out; assign [R, N] int32; counts [R, K] int32; inertia [R] fp64; n_iter [R] int32; state [2 R + 1]
 *   int32 (per restart: passes made, converged; then the number of converged restarts), written by resume = 0.
 * sv_kmeans_best: best [1] int32.  sv_contingency: counts [Ka, Kb] int32 += the pairs (a_i, b_i) of two int32 label vectors [N]
 *   (integer atomics; a label outside its range is skipped).
 * The workspace (sv_kmeans_workspace_bytes; 16-byte aligned) may hold anything on entry.  Everything is enqueued on `stream`; no host
 * synchronisation.  Accepted domain: 1 <= L <= 512, 2 <= K <= 64, 1 <= R <= 16, K <= N < 2^24, ldx >= L, iters >= 0, resume 0 / 1;
 * sv_contingency: N >= 1, 1 <= Ka, Kb <= 64: anything else SV_E_UNSUPPORTED; a null pointer (picks may be NULL) or a misaligned one
 * (4 bytes; fp64 8; workspace 16): SV_E_BADARG; workspace_bytes below sv_kmeans_workspace_bytes: SV_E_WORKSPACE.  All checked before
 * anything is enqueued. */
int sv_kmeans_chunk_rows(void);     /* rows per chunk of the segmented sum */
int sv_kmeans_workspace_bytes(int32_t N, int32_t L, int32_t K, int32_t R, int64_t* bytes);
int sv_kmeans_seed(const float* x, int32_t ldx, int32_t N, int32_t L, int32_t K, int32_t R, uint64_t seed, float* centroids,
                   int32_t* picks /* [R,K] or NULL */, void* workspace, int64_t workspace_bytes, void* stream);
int sv_kmeans_iterate(const float* x, int32_t ldx, int32_t N, int32_t L, int32_t K, int32_t R, int32_t iters, int32_t resume,
                      float* centroids, int32_t* assign, int32_t* counts, double* inertia, int32_t* n_iter, int32_t* state,
                      void* workspace, int64_t workspace_bytes, void* stream);
int sv_kmeans_best(const double* inertia, int32_t R, int32_t* best, void* stream);
int sv_contingency(const int32_t* a, const int32_t* b, int32_t N, int32_t Ka, int32_t Kb, int32_t* counts /* ADDED to */, void* stream);

/* ---------------------------------------------------------------- linear label probe of the latents (csrc/linprobe.hip)
 * No reference counterpart: the linear companion of the k-NN probe.  Softmax regression of the classes y [N] uint8 on the rows of
 * x [N, L] fp32 (row pitch ldx), fitted by Boehning's fixed-Hessian majorise-minimise step.  ALL INPUTS ARE FINITE.  With A = [x 1]
 * (N x (L + 1)), W [(L + 1), C] fp64 (row L is the bias) and W32 its fp32 rounding, a row whose class is >= C takes no part (its
 * residual and its loss are 0; the divisor stays N):
 *   logits       z_i = x_i . W32[:L] + W32[L]: the dot product over the whole of L in ascending order on v_mfma_f32_16x16x4_f32 (L
 *                zero-padded, no split over L, no atomics -- sv_knn_classify's rule), then one fp32 addition of the bias;
 *   softmax      in fp32: m = max_c z_c; e_c = expf(z_c - m); s = sum_c e_c in ascending c; p_c = e_c / s; r_c = p_c - [c == y_i];
 *                loss_i = logf(s) - (z_y - m);
 *   chunk sums   a chunk is sv_linprobe_chunk_rows() consecutive rows.  A^T M of a chunk (M = the residuals R, or A itself) is summed in
 *                fp32 on the same MFMA, the reduction dimension being the chunk's rows in ascending order; the chunks are folded in fp64
 *                in ascending chunk order.  The order depends on N and sv_linprobe_chunk_rows() alone.  No floating-point atomics;
 *   loss         loss_t = (sum_i loss_i) / N + (l2 / 2) sum W[:L]^2, both sums in fp64: the fp32 loss_i of a 64-row tile in ascending
 *                row order, then thread u of 256 takes the tiles u, u + 256, ... in ascending order, then the threads in ascending order;
 *                the squares W_e^2 (e the flat index over [L, C]) likewise: thread u takes e = u, u + 256, ..., then the threads in order;
 *   gradient     G = (A^T R) / N + l2 W on the rows < L, (A^T R) / N on the bias row: fp64 after the chunk fold; gmax_t = max |G|;
 *   step         W <- W - P G in fp64: per element sum_j P[i][j] G[j][c] from 0 in ascending j (a product, then an addition), then
 *                one subtraction.  P is the caller's: (A^T A / (2 N) + diag(l2 .. l2, 0))^-1 makes the step Boehning's, which never
 *                increases the objective;
 *   fit          from W_0, for t = 0 .. T: logits, softmax, loss_t, G, gmax_t against W_t; stop if t == T; otherwise step to W_{t+1}.
 * sv_linprobe_gram: S [(L + 1), (L + 1)] fp64 <- A^T A (not divided by N) by the chunk sums above; the upper triangle is computed
 *   and mirrored, so S is symmetric bit for bit.
 * sv_linprobe_fit: resume = 0 starts at the given W and the trajectory index 0 and makes `iters` steps (T = iters; iters = 0: one
 *   evaluation pass).  resume = 1 continues the fit whose W / state the previous call left with `iters` more steps: it makes the last
 *   pass again (the same bits at the same index), then goes on; calls in groups give the bits of one call with the total.  W in-out;
 *   loss, gmax [T_total + 1] fp64: the trajectories; grad [(L + 1), C] fp64 (may be NULL) <- the G of the last pass; state [1] int32:
 *   the index of the next trajectory element, written by resume = 0.
 * sv_linprobe_predict: pred [Nq] int32 <- the first maximum of the same logits of q [Nq, L] (ties to the lower class); acc [2] int64
 *   (may be NULL) += (hits, Nq), the hits only with q_class (integer atomics); loss [1] fp64 (may be NULL; needs q_class) <- the mean
 *   of loss_i by the same formulas and fold.
 * The workspace (sv_linprobe_workspace_bytes; 16-byte aligned) may hold anything on entry.  Everything is enqueued on `stream`; no
 * host synchronisation.  Accepted domain: 1 <= L <= 512, 2 <= C <= 64, 1 <= N < 2^24, ldx >= L, iters >= 0, resume 0 / 1, l2 >= 0 and
 * finite: anything else SV_E_UNSUPPORTED; a null pointer (grad, q_class, acc and loss of predict may be NULL; loss without q_class may
 * not) or a misaligned one (4 bytes; fp64 and acc 8; workspace 16): SV_E_BADARG; workspace_bytes below sv_linprobe_workspace_bytes:
 * SV_E_WORKSPACE.  All checked before anything is enqueued. */
int sv_linprobe_chunk_rows(void);     /* rows per fp32 partial of A^T M */
int sv_linprobe_workspace_bytes(int32_t N, int32_t L, int32_t C, int64_t* bytes);   /* covers gram, fit and predict of these sizes */
int sv_linprobe_gram(const float* x, int32_t ldx, int32_t N, int32_t L, double* S, void* workspace, int64_t workspace_bytes, void* stream);
int sv_linprobe_fit(const float* x, int32_t ldx, const uint8_t* y, int32_t N, int32_t L, int32_t C, const double* P, double l2,
                    int32_t iters, int32_t resume, double* W, double* loss, double* gmax, double* grad /* or NULL */, int32_t* state,
                    void* workspace, int64_t workspace_bytes, void* stream);
int sv_linprobe_predict(const float* q, int32_t ldq, int32_t Nq, int32_t L, int32_t C, const double* W, int32_t* pred,
                        const uint8_t* q_class /* or NULL */, int64_t* acc /* ADDED to, or NULL */, double* loss /* or NULL */,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- exact t-SNE map of the latents (csrc/tsne.hip)
 * No reference counterpart: the 2-D map of the latent means (van der Maaten & Hinton 2008, the exact O(N^2) form) of x [N, L] fp32
 * (row pitch ldx).  ALL INPUTS ARE FINITE.
 *   distance     d(i, j) = sv_knn_classify's distance of rows i and j, bit for bit: the same norms, the same fp32 MFMA chain over the
 *                whole of L, max(0, .).  In the row search a d that is NaN or +inf (an overflowed norm) counts as FLT_MAX;
 *   conditional  per row i, in fp64 over the fp32 distances: dmin_i = min_{k != i} d_ik, dd_j = d_ij - dmin_i (exact),
 *                e_j = exp(-beta_i dd_j), S = sum_{j != i} e_j, T = sum_{j != i} e_j dd_j, H(beta) = log S + beta T / S (the Shannon
 *                entropy in nats), p(j|i) = (float)(e_j / S), p(i|i) = 0.  The sums: thread u of 256 takes j = u, u + 256, ... in
 *                ascending order, then the threads in thread order;
 *   search       beta_i by bisection on H(beta) = log(perplexity), H being decreasing in beta: beta = 1, both sides unbounded; then
 *                exactly 100 steps, no early exit: if H(beta) > log(perplexity) then lo = beta and beta <- (lo + hi) / 2, or 2 beta
 *                while hi is unbounded; else hi = beta and beta <- (lo + hi) / 2, or beta / 2 while lo is unbounded; after each step
 *                beta is clamped to [2^-60, 2^60].  beta_i is the value after step 100, row_entropy_i = H(beta_i), and the row is
 *                the formula above at beta_i.  A row without a root -- H(inf) = log(the number of minimisers of d_i.) >= log
 *                (perplexity): all distances equal, or more exact duplicates of point i than the perplexity -- ends at beta = 2^60,
 *                where the formula gives 1 / m on the m minimisers (and what exp(-2^60 dd) leaves elsewhere: 0 for dd > 2^-50).  S >= 1
 *                always (a minimiser contributes 1), so no row holds a NaN or an inf;
 *   joint        P_ij = P_ji = (float)(((double)p(j|i) + (double)p(i|j)) / (2 N)), P_ii = 0: dense fp32 [N, N], symmetric bit for
 *                bit, in the buffer that held the distances and the conditional rows.  p_const [2] fp64 = (sum P, sum_{P > 0} P log P):
 *                per row lane l of 64 takes j = l, l + 64, ... ascending in fp64, then the lanes in lane order; then thread u of 256
 *                takes the rows u, u + 256, ..., then the threads in thread order;
 *   initial map  Y0 [N, 2] = 1e-4f * n(i, c): Philox4x32-10 with the key seed ^ 0x1a7e475e3a9, the standard normal of the counter
 *                (c, i, 'ts' << 16, 0) by the library's Box-Muller (cosine branch of the first two words); inc = 0, gain = 1,
 *                state[0] = 0 (the iteration counter; state is int32 [4]);
 *   pair sums    with w_ij = rcp(q_ij), q_ij = (1 + dx^2) + dy^2, dx = y_i0 - y_j0, dy = y_i1 - y_j1 in fp32 (v_rcp_f32), and w_ii = 0:
 *                A_ic = sum_j (P_ij w_ij) d_c, R_ic = sum_j (w_ij w_ij) d_c, z_i = sum_j w_ij, l_i = sum_{P_ij > 0} P_ij log2 q_ij
 *                (v_log_f32).  fp32 partials per (row, chunk of sv_tsne_chunk_rows() columns): lane l of 64 takes the columns
 *                l, l + 64, ... of the chunk ascending, then the xor butterfly 32, 16, ..., 1; the chunks of a row are folded in
 *                chunk order in fp64 (l_i then times ln 2).  Z = sum_i z_i and Lw = sum_i l_i in fp64: thread u of a 256-row group
 *                in thread order, then the groups in order.  The order depends on N and sv_tsne_chunk_rows() alone.  No
 *                floating-point atomics;
 *   objective    KL_t = p_const[1] + Lw + log(Z) p_const[0] = sum_{P > 0} P log(P / (w / Z)) of the unexaggerated P, fp64;
 *   gradient     g_ic = (float)(4 (e A_ic - R_ic / Z)) from the fp64 folds; e = exaggeration while t < exag_iters, else 1;
 *   update       the original delta-bar-delta rule, fp32 per component: gain <- gain + 0.2 if (g > 0) != (inc > 0) else gain * 0.8;
 *                gain <- max(gain, 0.01); inc <- m inc - (eta gain) g; y <- y + inc; m = 0.5 while t < exag_iters, else 0.8; then
 *                y <- y - (float)(column sum / N), the column sums in fp64 in the order of Z; then t <- t + 1.
 * sv_tsne_affinities: stages = 3 runs all of it; 1 stops behind the distances (P holds d), 2 behind the conditional rows (P holds
 *   p(j|i) in row i; beta, row_entropy written): for tests.  beta, row_entropy [N] fp64; p_const written by stage 3 only.
 * sv_tsne_init: Y, inc, gain [N, 2] fp32 and state [4] int32 as above.
 * sv_tsne_iterate: `iters` iterations from the caller's (Y, inc, gain, state[0] = t) -- sv_tsne_init's, a previous call's, or the
 *   caller's own -- enqueued without a host round trip.  Exaggeration and momentum switch on state[0], so calls in groups give the bits
 *   of one call with the total.  kl_trace [trace_len] fp64: iteration t writes kl_trace[t] = KL of the map it STARTED from, when
 *   t < trace_len; z_last [1] fp64 (may be NULL) <- that iteration's Z.
 * sv_tsne_neighbour_scores: nn_latent, nn_map [N, k + 1] int32: the neighbour lists sv_knn_classify returns for the latent rows and
 *   the map rows with queries = references.  Per row "self" is the first entry with index i if the list has it, else the last entry;
 *   the other k entries are the row's neighbours.  counts [3] int64 += (the number of latent neighbours that are map neighbours too,
 *   summed over rows; rows whose label equals the majority label of its map neighbours; the same for the latent neighbours); vote ties
 *   go to the lowest class id; labels NULL: only counts[0].  Integer atomics.  Entries outside [0, N) are no neighbours.
 * The workspace (sv_tsne_workspace_bytes; 16-byte aligned) may hold anything on entry.  Everything is enqueued on `stream`; no host
 * synchronisation.  Accepted domain: 4 <= N <= 32768, 1 <= L <= 512, ldx >= L, 1 < perplexity < N - 1, stages 1 .. 3, iters >= 0,
 * trace_len >= 0, exag_iters >= 0, 1 <= exaggeration <= 1e6, 0 < eta <= 1e9, 1 <= k, k + 1 <= min(32, N), 2 <= n_class <= 64 with
 * labels: anything else SV_E_UNSUPPORTED; a null pointer (z_last and labels may be NULL) or a misaligned one (4 bytes; fp64 and counts
 * 8; workspace 16): SV_E_BADARG; workspace_bytes below sv_tsne_workspace_bytes: SV_E_WORKSPACE.  All checked before anything is
 * enqueued. */
int sv_tsne_chunk_rows(void);     /* columns per fp32 partial of the pair sums */
int sv_tsne_workspace_bytes(int32_t N, int64_t* bytes);   /* covers affinities and iterate */
int sv_tsne_affinities(const float* x, int32_t ldx, int32_t N, int32_t L, double perplexity, int32_t stages, float* P /* [N,N] */,
                       double* beta /* [N] */, double* row_entropy /* [N] */, double* p_const /* [2] */, void* workspace,
                       int64_t workspace_bytes, void* stream);
int sv_tsne_init(int32_t N, uint64_t seed, float* Y, float* inc, float* gain, int32_t* state /* [4] */, void* stream);
int sv_tsne_iterate(const float* P, const double* p_const, int32_t N, int32_t iters, float exaggeration, int32_t exag_iters, float eta,
                    float* Y, float* inc, float* gain, int32_t* state, double* kl_trace, int32_t trace_len, double* z_last /* or NULL */,
                    void* workspace, int64_t workspace_bytes, void* stream);
int sv_tsne_neighbour_scores(const int32_t* nn_latent, const int32_t* nn_map, const uint8_t* labels /* [N] or NULL */, int32_t N, int32_t k,
                             int32_t n_class, int64_t* counts /* [3]: ADDED to */, void* stream);

/* ---------------------------------------------------------------- swap-consistency report of the latents (csrc/swap.hip)
 * No reference counterpart.  decode(z_g of image A, z_l of image B) is re-encoded as the image it is, and the originals are ranked by
 * their distance from the re-encoded latents: does each block come back from its own source?  (split_vae_amd/swap.py)
 * sv_swap_pair: zcat [B, Lg + Ll] (contiguous, `dtype` of sv_dtype) <- [ mu[ig[b], 0:Lg] | mu[il[b], Lg:Lg+Ll] ], one rounding to the
 *   dtype.  mu [N, Lg + Ll] fp32 with row pitch ldmu >= Lg + Ll; ig, il [B] int32 on the device.  An index outside [0, N) is clamped
 *   (nothing is read outside mu; the host layer refuses such an index).  SV_E_BADARG: a null or misaligned pointer, N, B, Lg or Ll <= 0,
 *   ldmu below the width, a dtype outside sv_dtype.
 * sv_swap_requantise: a decode as the image it is, and the encoders' six-channel batch of it, in one pass.  out6 [B,H,W,6] fp32 (the
 *   plan's out6_x, read in place): channels 0..2 are the mean m; channels 3..5 are NEVER READ.  Per value, in fp32:
 *   v = fminf(fmaxf(m, -1), 1); level = (int) rintf(fmaf(v, 127.5, 127.5)) (one rounding, ties to even), clamped to 0 .. 255; the
 *   pixel is lut[level], lut [256] fp32 = data.ResidentDataset.make_lut(): the data's own values x / 255 * 2 - 1.  A NaN MEAN MAPS TO
 *   LEVEL 0.  images6 [B,H,W,6] fp32: channels 0..2 the requantised image, channels 3..5 its patch scramble by perm [B, (H/patch)^2]
 *   int32 with sv_scramble_gather's index rule (x_aug[r s + i, c s + j] = x[pr s + i, pc s + j], (pr, pc) = divmod(perm[r G + c], G));
 *   a perm entry outside [0, G^2) is clamped.  Every output element is written exactly once; no workspace; out6 and images6 must not
 *   be the same buffer.  SV_E_BADARG: a null or misaligned (4 bytes) pointer, out6 == images6, B, H, W or patch <= 0;
 *   SV_E_UNSUPPORTED: H != W or patch does not divide H.
 * sv_swap_rank: queries q [Nq, L] and references r [Nr, L] fp32 (row pitches ldq, ldr >= L), two target lists t0, t1 [Nq] int32 in
 *   [0, Nr) on the device (clamped; the host layer refuses others).  rank [Nq, 2] int32:
 *     rank[q][s] = #{ j != t_s[q] : d(q, j) < d(q, t_s[q])  or  (d(q, j) == d(q, t_s[q]) and j < t_s[q]) }
 *   with d sv_knn_classify's squared distance, bit for bit (the same norms, the same fp32 MFMA chain over the whole of L, d = max(0,
 *   (n(q) + n(r)) - 2 dot)); ALL INPUTS ARE FINITE.  The thresholds d(q, t_s[q]) come from the same tile code on the gathered target
 *   rows, so they are the bits the count sees in column t_s[q]; that column is excluded by index.  The references are cut into chunks
 *   of sv_swap_chunk_rows() rows; integer partial counts per (chunk, query) are folded in chunk order: no atomics, no floating-point
 *   sums, the same bits on a repeat.  The Nq x Nr matrix never exists.  Nothing outside rank [Nq, 2] and the workspace is written; the
 *   workspace (sv_swap_rank_workspace_bytes; 16-byte aligned) may hold anything on entry.  Everything is enqueued on `stream`; no host
 *   synchronisation.  SV_E_BADARG: a null or misaligned pointer (4 bytes; workspace 16), Nq, Nr or L <= 0, a pitch below L;
 *   SV_E_UNSUPPORTED: Nq > 8 * 65536, Nr > 2^24 or L > 512; SV_E_WORKSPACE: workspace_bytes below sv_swap_rank_workspace_bytes.  All
 *   checked before anything is enqueued.
 * sv_swap_shift_word_host: the 32-bit Philox word the report draws its partner shifts from, keyed by (seed, a tag of this report's own,
 *   partner p, attempt); host only. */
int sv_swap_pair(const float* mu, int32_t ldmu, const int32_t* ig, const int32_t* il, void* zcat, int32_t dtype, int32_t N, int32_t B,
                 int32_t Lg, int32_t Ll, void* stream);
int sv_swap_requantise(const float* out6, const float* lut /* [256] */, const int32_t* perm, float* images6, int32_t B, int32_t H,
                       int32_t W, int32_t patch, void* stream);
int sv_swap_chunk_rows(void);     /* reference rows per chunk of the count pass: lets callers and tests size Nr */
int sv_swap_rank_workspace_bytes(int32_t Nq, int32_t Nr, int32_t L, int64_t* bytes);
int sv_swap_rank(const float* q, int32_t ldq, const float* r, int32_t ldr, const int32_t* t0, const int32_t* t1, int32_t Nq, int32_t Nr,
                 int32_t L, int32_t* rank /* [Nq,2] */, void* workspace, int64_t workspace_bytes, void* stream);
uint32_t sv_swap_shift_word_host(uint64_t seed, int32_t p, int32_t attempt);

/* ---------------------------------------------------------------- sample-quality report of prior draws (csrc/prdc.hip)
 * No reference counterpart.  Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) ask "is
 * query q inside reference j's k-NN ball": a compare against a per-COLUMN radius, a count and a row minimum behind the distance tile,
 * and the k-NN radius of a set against itself.  (split_vae_amd/sample_quality.py)
 *   distance  d(q, r) = sv_knn_classify's squared distance, bit for bit (the same norms, the same fp32 MFMA chain over the whole of L in
 *             ascending order, d = max(0, (n(q) + n(r)) - 2 q . r)); ALL INPUTS ARE FINITE.
 * sv_prdc_radius: x [N, L] fp32 (row pitch ldx >= L).  rad [N] fp32: rad[i] = the k-th smallest element of { d(i, j) : j != i } under the
 *   total order (d, j).  SELF IS EXCLUDED BY INDEX, NOT BY A ZERO DISTANCE: a duplicate of row i at another index is a neighbour at
 *   distance 0.  Computed from sv_knn_classify's (k + 1)-list of x against itself: index i is dropped from the list if it is there, the
 *   k-th of what remains is the radius (self is missing from the list only when k + 1 other rows precede it under (d, j), and then the
 *   k-th entry is the answer as well).  Domain: 1 <= k <= 31, k + 1 <= N <= 8 * 65536, 1 <= L <= 512.
 * sv_prdc_count: queries q [Nq, L] and references r [Nr, L] fp32 (row pitches ldq, ldr >= L), rad [Nr] fp32, the radius of each
 *   REFERENCE.    cnt[q]  = #{ j : d(q, j) <= rad[j] }          (note <=)                         int32 [Nq]
 *                 dmin[q] = min_j d(q, j)                                                          fp32 [Nq] or NULL
 *                 imin[q] = the lowest j that attains the minimum                                  int32 [Nq] or NULL
 *   The references are cut into chunks of sv_prdc_chunk_rows() rows; one (cnt, dmin, imin) partial per (chunk, query) is folded in
 *   ascending chunk order, a strict < keeping the lower index: integer counts and minima, no atomics, no floating-point sums, the same
 *   bits on a repeat.  The Nq x Nr matrix never exists.
 * Both: nothing outside the outputs and the workspace is written; the workspace (sv_prdc_workspace_bytes; 16-byte aligned) may hold
 *   anything on entry.  sv_prdc_workspace_bytes(Nq, Nr, L, k) covers sv_prdc_count at (Nq, Nr, L) and, where Nq == Nr >= k + 1,
 *   sv_prdc_radius at (N = Nr, L, k) too; it wants 1 <= k <= 31 either way.  Everything is enqueued on `stream`; no host
 *   synchronisation.  SV_E_BADARG: a null or misaligned pointer (4 bytes; workspace 16), N, Nq, Nr or L <= 0, a pitch below L;
 *   SV_E_UNSUPPORTED: Nq > 8 * 65536, Nr > 2^24, L > 512, k outside 1 .. 31, N < k + 1 or N > 8 * 65536; SV_E_WORKSPACE:
 *   workspace_bytes below what the call needs.  All checked before anything is enqueued. */
int sv_prdc_chunk_rows(void);     /* reference rows per chunk of the count pass: lets callers and tests size Nr */
int sv_prdc_workspace_bytes(int32_t Nq, int32_t Nr, int32_t L, int32_t k, int64_t* bytes);
int sv_prdc_radius(const float* x, int32_t ldx, int32_t N, int32_t L, int32_t k, float* rad /* [N] */, void* workspace,
                   int64_t workspace_bytes, void* stream);
int sv_prdc_count(const float* q, int32_t ldq, const float* r, int32_t ldr, const float* rad /* [Nr] */, int32_t Nq, int32_t Nr, int32_t L,
                  int32_t* cnt /* [Nq] */, float* dmin /* [Nq] or NULL */, int32_t* imin /* [Nq] or NULL */, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* ---- K16 data-parallel gradient exchange: absent in the reference (single device) -----------
 * One process per GPU; gradients of the batch-mean loss (vae/trainer.py:13,:127-128,:137) are averaged over equal
 * shards by an in-place all-reduce(sum) of the flat fp32 gradient buffer; 1/world is sv_adam_step's grad_scale.
 * RCCL is loaded at run time (the process's own copy if it has one, e.g. PyTorch's): SV_E_UNSUPPORTED without it.
 *   sv_comm_unique_id   rank 0 draws the 128-byte rendezvous id and ships it to the others out of band
 *   sv_comm_init        collective over all ranks; binds the calling thread's current HIP device
 *   sv_comm_allreduce   enqueue on `stream` (asynchronous): buf[0..count) <- sum over ranks
 *   sv_comm_allreduce_ranges   n disjoint element ranges [begin[i], end[i]) of one buffer as one RCCL group
 *                       (a bucket = the contiguous runs of the parameters whose gradients one backward phase completes) */
typedef struct sv_comm sv_comm;
int sv_comm_unique_id(void* id128);
int sv_comm_init(const void* id128, int32_t rank, int32_t world, sv_comm** out);
int sv_comm_allreduce(sv_comm* comm, float* buf, int64_t count, void* stream);
int sv_comm_allreduce_ranges(sv_comm* comm, float* base, const int64_t* begin, const int64_t* end, int32_t n, void* stream);
int sv_comm_destroy(sv_comm* comm);

#ifdef __cplusplus
}
#endif
#endif
