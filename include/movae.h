/*
 * movae.h -- C ABI of libmovae_hip.so: the MI355X (gfx950) kernels under MO-VAE's per-step
 * training hot path.  The reference has no native boundary of its own
 * (it is pure Python on ATen + torchjd); each entry point below names the reference call whose
 * device arithmetic it replaces (paths relative to the reference root).  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer (fp32 unless stated); nothing is allocated,
 *     freed or synchronised inside; work is enqueued on `stream` (a hipStream_t, may be NULL);
 *   - activations are NHWC ("channels_last"): x[n][h][w][c]; conv weights are [Co][KH][KW][Ci]
 *     and transposed-conv weights [Ci][KH][KW][Co] in memory (the channels_last image of the
 *     reference's OIHW / IOHW parameter shapes), Linear weights [out][in];
 *   - `ws`/`ws_bytes`: scratch for split-K partials / reduction partials; may be NULL/0 where stated (then no
 *     split-K).  The FIRST 4096 BYTES of the workspace are the library's header: they must be zero before the
 *     first call (hipMemset once), are left zero by every call, and one workspace must only be used by one stream
 *     at a time.  The header is reserved: no kernel uses it at present.  Everything after the header is plain
 *     scratch with no state between calls;
 *   - return 0 on success, <0 on invalid argument (-1), unsupported shape (-2) or launch
 *     failure (-3); movae_last_error() gives the text for the calling thread.
 */
#ifndef MOVAE_H
#define MOVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* movae_stream_t; /* hipStream_t */

enum movae_act { MOVAE_ACT_NONE = 0, MOVAE_ACT_LRELU = 1, MOVAE_ACT_RELU = 2, MOVAE_ACT_TANH = 3, MOVAE_ACT_SIGMOID = 4 };
enum movae_recon { MOVAE_RECON_MSE = 0, MOVAE_RECON_BCE = 1, MOVAE_RECON_L1 = 2, MOVAE_RECON_SMOOTH_L1 = 3 };
enum movae_mgda_norm { MOVAE_MGDA_NONE = 0, MOVAE_MGDA_L2 = 1, MOVAE_MGDA_LOSS = 2, MOVAE_MGDA_LOSS_PLUS = 3 };
enum movae_upgrad_norm { MOVAE_UPGRAD_TRACE = 0, MOVAE_UPGRAD_MIN_L2 = 1, MOVAE_UPGRAD_COSINE = 2 };
enum movae_amtl_scale { MOVAE_AMTL_MIN = 0, MOVAE_AMTL_MEDIAN = 1, MOVAE_AMTL_RMSE = 2 };

int movae_version(void);
const char* movae_last_error(void);

/* ---- layout ------------------------------------------------------------------------------
 * NCHW <-> NHWC transposes at the model boundary (main.py:155 hands NCHW images; nn.Flatten /
 * nn.Unflatten in models/vae.py:128,143 order features NCHW). */
int movae_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, movae_stream_t stream);
int movae_nhwc_to_nchw(const float* src, float* dst, int n, int c, int h, int w, movae_stream_t stream);

/* ---- convolutions (implicit GEMM on v_mfma_f32_32x32x2_f32) -----------------------------------
 * conv2d      : nn.Conv2d forward/backward      models/vae.py:121,170; vq_vae.py:232-257; vq_vae2.py:36-47; betatc_vae.py:104-110
 * convT2d     : nn.ConvTranspose2d              models/vae.py:151-156,163-168; vq_vae.py:287-300; vq_vae2.py:75-88
 * linear      : nn.Linear == conv2d with h=w=kh=kw=1   models/vae.py:133-137; betatc_vae.py:124-131
 * `act`/`slope` fuse the following nn.LeakyReLU/ReLU/Tanh/Sigmoid into the epilogue.
 * y[n][ho][wo][co] with ho = (hi + 2*pad - kh)/stride + 1 (conv) or (hi-1)*stride - 2*pad + kh + out_pad (convT). */
int movae_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                     int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                     int act, float slope, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_conv2d_dgrad(const float* dy, const float* w, float* dx,
                       int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                       void* ws, size_t ws_bytes, movae_stream_t stream);
/* dw[co][kh][kw][ci] (+)= sum dy * x ; dbias[co] (+)= sum dy (dbias may be NULL). accumulate!=0 adds to dw/dbias. */
int movae_conv2d_wgrad(const float* dy, const float* x, float* dw, float* dbias,
                       int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                       int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);
/* wgrad for `groups` (<= 8) cotangents of one forward in ONE launch (batched pull-back of mtl_backward's K losses):
 * dy is stacked [groups][n][ho][wo][co], x is shared; dw / dbias are HOST arrays of `groups` device pointers (rows of
 * the Jacobian); dbias or any dbias[i] may be NULL. */
int movae_conv2d_wgrad_grouped(int groups, const float* dy, const float* x, float* const* dw, float* const* dbias,
                               int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                               int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_convT2d_fwd(const float* x, const float* w, const float* bias, float* y,
                      int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                      int act, float slope, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_convT2d_dgrad(const float* dy, const float* w, float* dx,
                        int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                        void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_convT2d_wgrad(const float* dy, const float* x, float* dw, float* dbias,
                        int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                        int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);
/* The backward of one layer in one call: movae_conv[T]2d_dgrad over groups * n images (dy stacked [groups][n][ho][wo][co],
 * dx likewise) followed by movae_conv[T]2d_wgrad_grouped.  When both land on the small-tile MFMA kernels they share ONE
 * launch (igemm2_pair: the two problems only share read-only operands and neither fills the chip alone); results are
 * bit-identical to the two separate calls.  MOVAE_NO_PAIR=1 forces the separate launches. */
int movae_conv2d_dgrad_wgrad_grouped(int groups, const float* dy, const float* w, const float* x, float* dx, float* const* dw,
                                     float* const* dbias, int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw,
                                     int stride, int pad, int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_convT2d_dgrad_wgrad_grouped(int groups, const float* dy, const float* w, const float* x, float* dx, float* const* dw,
                                      float* const* dbias, int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw,
                                      int stride, int pad, int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_convT2d_wgrad_grouped(int groups, const float* dy, const float* x, float* const* dw, float* const* dbias,
                                int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                                int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);
/* Two nn.Linear layers applied to the same input -- fc_mu || fc_var (models/vae.py:128-129,187-192, betatc_vae.py:100-101,181-182):
 *   y1 = x w1^T + b1, y2 = x w2^T + b2      x [m][k], w [n][k], y [m][n]                          (one launch)
 *   dx[g] = dy1[g] w1 + dy2[g] w2;  dw_i[g] = dy_i[g]^T x;  db_i[g] = column sums of dy_i[g]       (two launches, all groups)
 * dy_i stacked [groups][m][n], dx [groups][m][k] (NULL: not wanted), dw_i / db_i HOST arrays of device pointers (db_i or its entries
 * may be NULL; dw1 == dw2 == NULL: no weight gradients).  Results equal the four ordinary calls up to the summation order of dx.
 * Returns MOVAE_EUNSUPPORTED, with nothing launched, outside the one-launch GEMM kernels' range (groups <= 4, n, k multiples of 4, m * n,
 * m * k, n * k <= 2^20, reductions <= 2048, 16-byte aligned operands): make the ordinary calls then. */
int movae_linear_pair_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y1, float* y2,
                          int m, int n, int k, movae_stream_t stream);
int movae_linear_pair_bwd(int groups, const float* dy1, const float* dy2, const float* w1, const float* w2, const float* x, float* dx,
                          float* const* dw1, float* const* dw2, float* const* db1, float* const* db2, int m, int n, int k,
                          movae_stream_t stream);

/* ---- BatchNorm2d (training statistics) + activation ------------------------------------------
 * nn.BatchNorm2d + nn.LeakyReLU   models/vae.py:123-125,157-158,169-170   (eps 1e-5, momentum 0.1)
 * y is the conv output [rows][c]; stats are accumulated in fp64.  `ws` must hold
 * movae_bn_ws_bytes(rows, c) bytes.  num_batches_tracked (device int64, may be NULL) is incremented by the
 * statistics kernel in training mode (torch's BatchNorm2d does it with a launch of its own). */
size_t movae_bn_ws_bytes(int rows, int c);
int movae_bn_act_fwd(const float* y, const float* gamma, const float* beta, float* out,
                     float* save_mean, float* save_rstd, float* running_mean, float* running_var,
                     long long* num_batches_tracked,
                     int rows, int c, float eps, float momentum, int training, int act, float slope,
                     void* ws, size_t ws_bytes, movae_stream_t stream);
/* dy = d(loss)/d(conv output); dgamma/dbeta written (or accumulated when accumulate!=0). */
int movae_bn_act_bwd(const float* dout, const float* y, const float* gamma, const float* beta,
                     const float* save_mean, const float* save_rstd, float* dy, float* dgamma, float* dbeta,
                     int rows, int c, int act, float slope, int accumulate,
                     void* ws, size_t ws_bytes, movae_stream_t stream);

/* the same backward for `groups` (<= 8) cotangents of ONE forward at once (the K loss cotangents of
 * mtl_backward, main.py:188-190): dout / dy are stacked [groups][rows][c]; y and the saved statistics are shared; the
 * batch means of the cotangent are taken per group; dgamma / dbeta are HOST arrays of `groups` device pointers
 * (rows of the Jacobian).  ws must hold 4096 + groups * (movae_bn_ws_bytes(rows, c) - 4096) bytes. */
int movae_bn_act_bwd_grouped(int groups, const float* dout, const float* y, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_rstd, float* dy,
                             float* const* dgamma, float* const* dbeta,
                             int rows, int c, int act, float slope, int accumulate,
                             void* ws, size_t ws_bytes, movae_stream_t stream);

/* ---- element-wise ---------------------------------------------------------------------------- */
int movae_act_fwd(const float* x, float* y, size_t n, int act, float slope, movae_stream_t stream);
/* dx = dy * act'(.) evaluated from the activation OUTPUT `out` (valid for all five kinds) */
int movae_act_bwd(const float* dy, const float* out, float* dx, size_t n, int act, float slope, movae_stream_t stream);
/* dpre = dy * act'(out) for `groups` (<= 8) stacked cotangents [groups][rows][c] of one forward (out is shared) AND, in the
 * same pass, dbias[g][c] (+)= sum_rows dpre -- the bias gradient of the conv whose epilogue applied the activation
 * (models/betatc_vae.py:104-110, vq_vae2.py:36-47: Conv2d(bias) -> LeakyReLU / ReLU).  c %% 4 == 0; dbias: HOST array
 * of device pointers, or NULL: only dpre (one launch for all groups; the conv weight-gradient entry points form the column
 * sums of dpre themselves while they stage it). */
int movae_act_bwd_bias_grouped(int groups, const float* dy, const float* out, float* dpre, float* const* dbias,
                               int rows, int c, int act, float slope, int accumulate,
                               void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_add(const float* a, const float* b, float* y, size_t n, movae_stream_t stream);
int movae_axpby(float alpha, const float* a, float beta, const float* b, float* y, size_t n, movae_stream_t stream);
/* channel concat / split of NHWC tensors: dst[rows][c_dst], src[rows][c_src] placed at channel offset */
int movae_copy_channels(const float* src, float* dst, int rows, int c_src, int c_dst, int src_off, int dst_off, int c_copy, movae_stream_t stream);
/* column sums: out[c] (+)= sum_rows x[rows][c]   (bias gradients) */
int movae_colsum(const float* x, float* out, int rows, int c, int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream);

/* reparameterize  z = mu + eps * exp(0.5 * log_var)      models/vae.py:187-192, betatc_vae.py:206-216 */
int movae_reparam_fwd(const float* mu, const float* log_var, const float* eps, float* z, size_t n, movae_stream_t stream);
/* z = mu + exp(0.5 * log_var) * eps with eps ~ N(0, 1) drawn inside the launch (Philox4x32-10 keyed by state[0], counter block =
 * (output quad, state[1]); Box-Muller) and written to `eps` for the backward.  state: device uint64[2] = {seed, draws made so far};
 * advance != 0: state[1] += 1 by the block that finishes last, so a replayed hipGraph draws fresh noise each time (one launch
 * where torch.randn_like + movae_reparam_fwd are four).  One such call at a time per process (the arrival count is a device global). */
int movae_reparam_rng_fwd(const float* mu, const float* log_var, float* eps, float* z, size_t n, unsigned long long* state, int advance,
                          movae_stream_t stream);
/* movae_reparam_rng_fwd that also fills prior[0 .. n_prior) with N(0, 1) draws from the same generator state and draw number (the
 * counter blocks that follow eps's): the cycle branch's z_prior of the cycle / recursive-cyclic VAEs, one launch and one advance for both. */
int movae_reparam_prior_rng_fwd(const float* mu, const float* log_var, float* eps, float* z, size_t n, float* prior, size_t n_prior,
                                unsigned long long* state, int advance, movae_stream_t stream);
int movae_reparam_bwd(const float* dz, const float* log_var, const float* eps, float* dmu, float* dlog_var, size_t n, movae_stream_t stream);

/* ---- losses -------------------------------------------------------------------------------------
 * recon: utils/objectives.py:95-97 (mse), 108-110 (bce), 129-131 (l1), 134-136 (smooth_l1): mean over all
 * elements; out[0] = scale * loss.  ws >= movae_reduce_ws_bytes(n). */
size_t movae_reduce_ws_bytes(size_t n);
int movae_recon_loss_fwd(const float* recons, const float* inputs, float* out, size_t n, int kind, float scale,
                         void* ws, size_t ws_bytes, movae_stream_t stream);
/* drecons = (*gscale_dev) * scale * d(mean loss)/d(recons) ; gscale_dev may be NULL (=1) */
int movae_recon_loss_bwd(const float* recons, const float* inputs, const float* gscale_dev, float* drecons,
                         size_t n, int kind, float scale, movae_stream_t stream);
/* The same, times act'(pre) for recons = act(pre) -- the decoder's output activation, whose derivative is a function of its output
 * (MOVAE_ACT_*): dpre is the gradient w.r.t. the PRE-activation values, so the producing convolution's backward needs no
 * activation-backward pass (ops.ActLink). */
int movae_recon_loss_bwd_act(const float* recons, const float* inputs, const float* gscale_dev, float* dpre, size_t n, int kind,
                             float scale, int act, float slope, movae_stream_t stream);
/* kl: utils/objectives.py:141-144, out[0] = scale * mean_b(-0.5 sum_d(1 + lv - mu^2 - e^lv)) */
int movae_kl_fwd(const float* mu, const float* log_var, float* out, int b, int d, float scale,
                 void* ws, size_t ws_bytes, movae_stream_t stream);
/* The scalar arithmetic of a loss_function (models/vq_vae.py:381-391, vq_vae2.py:313-334, betatc_vae.py:298-324) in ONE launch:
 * `nterms` device scalars, out[k] = f_k * w_k * (sum of the terms whose coef[k][t] != 0 -- a row's non-zero coefficients must all
 * equal w_k), k < nout <= 7, and out[nout] = out[0] + ... in order.  f_k = 1 except for k == anneal_row (>= 0) with iter_dev
 * given: BetaTC's annealing factor min(iter / anneal_steps, 1), the device counter iter_dev being advanced first when training
 * (models/betatc_vae.py:13,298-302); anneal_out (nullable) keeps the factor for the backward.  terms / g: HOST arrays of device
 * pointers (g has nout + 1 entries, NULL = absent cotangent); gterms: device [nterms]. */
int movae_combine_losses_fwd(int nterms, const float* const* terms, int nout, const float* coef, float* iter_dev, float anneal_steps,
                             int anneal_row, int training, float* out, float* anneal_out, movae_stream_t stream);
int movae_combine_losses_bwd(int nterms, int nout, const float* const* g, const float* coef, const float* anneal_dev, int anneal_row,
                             float* gterms, movae_stream_t stream);
/* VAE.loss_function (models/vae.py:211-228) in three launches: out[3] = (reconstruction_loss, kld_loss, total_loss = their fp32 sum);
 * the same arithmetic as movae_recon_loss_fwd + movae_kl_fwd + a tensor add.  ws >= the two reductions' workspaces together. */
int movae_vae_losses_fwd(const float* recons, const float* inputs, size_t n, int kind, float rec_scale,
                         const float* mu, const float* log_var, int b, int d, float kl_scale, float* out,
                         void* ws, size_t ws_bytes, movae_stream_t stream);
/* loss_function of the recursive-KL / cycle / recursive-cyclic VAEs (models/recursive_kl_vae.py, cycle_vae.py,
 * recursive_cyclic_vae.py) in two launches.  out = [w_rec * recon, (anneal * w_kl * kl(mu_hat, log_var_hat)),
 * (w_cyc * mean_b sum_d (z_prior - mu_gen)^2), total]: a term is present when its operands are (mu_hat / log_var_hat, z_prior / mu_gen
 * nullable in pairs).  anneal: 1 when !training; else anneal_host, or with iter_dev min(++iter_dev / anneal_steps, 1) on the device.
 * anneal_out (nullable) keeps the factor for the backward.  ws >= movae_reduce_ws_bytes(n) + 2 * movae_reduce_ws_bytes(b * d).
 * The backward writes the cotangents of recons / mu_hat / log_var_hat / mu_gen (each output nullable) for the present cotangents
 * g_* of the outputs (device scalars, nullable; g_tot reaches every term). */
int movae_recursive_losses_fwd(const float* recons, const float* inputs, size_t n, int kind, const float* mu_hat, const float* log_var_hat,
                               const float* z_prior, const float* mu_gen, int b, int d, float w_rec, float w_kl, float w_cyc,
                               float* iter_dev, float anneal_host, float anneal_steps, int training, float* out, float* anneal_out,
                               void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_recursive_losses_bwd(const float* recons, const float* inputs, size_t n, int kind, const float* mu_hat, const float* log_var_hat,
                               const float* z_prior, const float* mu_gen, int b, int d, float w_rec, float w_kl, float w_cyc,
                               const float* anneal_dev, const float* g_rec, const float* g_kl, const float* g_cyc, const float* g_tot,
                               float* drecons, float* dmu_hat, float* dlog_var_hat, float* dmu_gen, movae_stream_t stream);
/* ---- the conv Sphere Encoder (models/sphere_encoder.py) -------------------------------------------------------------------------
 * movae_sphere_latents_fwd: everything between encoder_proj and the two decoder calls in one launch.  With n(x) = radius * x /
 * sqrt(mean(x^2) + eps) per row of z[b][l]:
 *     v = n(z);   deg = u0 * angle_max, or mix_min + u2 * (mix_max - mix_min) where mix_prob > 0 and u1 < mix_prob;
 *     sigma = tan(deg * pi / 180);  sigma_sub = (0.5 * u3) * sigma;   v_noisy = n(v + sigma * e);   v_noisy_small = n(v + sigma_sub * e)
 * u[b][4] = (angle, mix mask, mix angle, s) uniforms and e[b][l] the noise direction.  Modes:
 *   schedule     e and u given (state null, fixed_sigma 0);
 *   in-kernel    state = device uint64[2] {seed, draws}: e and u are DRAWN in the launch (Philox4x32-10 keyed by the seed; per row
 *                ceil(l / 4) counter blocks of e through Box-Muller, then one of u) and written out for the backward; advance != 0:
 *                state[1] += 1 by the block that finishes last.  One such call at a time per process (the arrival count is a device
 *                global), as for movae_reparam_rng_fwd;
 *   given sigma  fixed_sigma != 0: sigma_in[b] (sigma_rows != 0), sigma_in[0], or sigma_val when sigma_in is null; e given; produces
 *                v_noisy (and v when asked), no v_noisy_small;
 *   clean        e null: v only.
 * Outputs are nullable; inv_rms[3][b] keeps 1 / rms of z, w, w' for the backward.  l <= 16384.
 * movae_sphere_latents_bwd: dz = nT(g_v + nT(g_noisy; w) + nT(g_small; w'); z) with nT(g; x) = radius * (g / rms - x * (g . x) /
 * (l * rms^3)), w and w' recomputed from v, e and sigma; the cotangents are nullable (e / sigma only needed with theirs); the
 * noise terms carry no gradient. */
int movae_sphere_latents_fwd(const float* z, float* e, float* u, const float* sigma_in, int sigma_rows, float sigma_val, int fixed_sigma,
                             unsigned long long* state, int advance, int b, int l, float angle_max_deg, float mix_prob, float mix_min_deg,
                             float mix_max_deg, float radius, float eps, float* v, float* v_noisy, float* v_noisy_small, float* sigma,
                             float* sigma_sub, float* inv_rms, movae_stream_t stream);
int movae_sphere_latents_bwd(const float* v, const float* e, const float* sigma, const float* sigma_sub, const float* inv_rms,
                             const float* g_v, const float* g_noisy, const float* g_small, float* dz, int b, int l, float radius,
                             movae_stream_t stream);
/* SphereEncoder.loss_function in two launches: out[4] = (lam_rec * (w_rec_sl1 * mean smooth_l1(recons - inputs)), lam_con * (w_con_sl1 *
 * mean smooth_l1(x_noisy - sg)), lam_lat * mean_b(1 - cos(v, v_enc_dec)), their fp32 sum in that order); sg = recons_sg, or recons
 * itself when recons_sg is null (recons is then read once for both pixel terms); smooth-L1 with beta = 1; the cosine with
 * F.cosine_similarity's clamp of each norm at 1e-8.  n image elements in one memory order, v / v_enc_dec [b][l].
 * ws >= movae_sphere_losses_ws_bytes(n, b).  The backward serves the present cotangents g_* (device scalars, nullable; g_tot reaches
 * every term) and writes the outputs given (nullable): drecons from pix_recon alone (pix_con's target is a constant), dx_noisy,
 * dv, dv_enc_dec. */
size_t movae_sphere_losses_ws_bytes(size_t n, int b);
int movae_sphere_losses_fwd(const float* recons, const float* inputs, const float* x_noisy, const float* recons_sg, size_t n, const float* v,
                            const float* v_enc_dec, int b, int l, float lam_rec, float w_rec_sl1, float lam_con, float w_con_sl1,
                            float lam_lat, float* out, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_sphere_losses_bwd(const float* recons, const float* inputs, const float* x_noisy, const float* recons_sg, size_t n, const float* v,
                            const float* v_enc_dec, int b, int l, float lam_rec, float w_rec_sl1, float lam_con, float w_con_sl1,
                            float lam_lat, const float* g_rec, const float* g_con, const float* g_lat, const float* g_tot, float* drecons,
                            float* dx_noisy, float* dv, float* dv_enc_dec, movae_stream_t stream);
int movae_kl_bwd(const float* mu, const float* log_var, const float* gscale_dev, float* dmu, float* dlog_var,
                 int b, int d, float scale, movae_stream_t stream);
/* Beta-TC decomposition: models/betatc_vae.py:262-296.  out[0..2] = mi, tc, kld (unweighted means).
 * log_iw is the [b][b] fp32 log-importance-weight matrix of betatc_vae.py:275-289. */
int movae_tc_decomp_fwd(const float* z, const float* mu, const float* log_var, const float* log_iw, float* out,
                        float* lse_joint, float* lse_marg, int b, int d, void* ws, size_t ws_bytes, movae_stream_t stream);
/* g[0..2] = upstream gradients of (mi, tc, kld) on device */
int movae_tc_decomp_bwd(const float* z, const float* mu, const float* log_var, const float* log_iw,
                        const float* lse_joint, const float* lse_marg, const float* g,
                        float* dz, float* dmu, float* dlog_var, int b, int d, movae_stream_t stream);

/* ---- Sobel edge losses of the gradient-guided VAE --------------------------------------------
 * models/gg_vae.py:42-53 (depthwise Sobel x / y, zero padding 1), EPS = 1e-8 (gg_vae.py:8); images NHWC [n][h][w][c].
 * edge weights (gg_vae.py:125-132): w_raw[n*h*w] = max_c sqrt(gx^2 + gy^2 + EPS) of `inputs`, wmax[0] = global max;
 * edge-weighted pixel loss (gg_vae.py:134-137): out = scale * mean( w_raw / (wmax + EPS) * (recons - inputs)^2 );
 * edge matching losses: out = scale * mean f(sobel recons, sobel inputs), one point-wise variant per `mode`
 * (enum movae_edge_match; gp / gt = |sobel recons| / |sobel inputs|, sl1 = smooth-L1 with beta 1):
 *   MAG         sl1(gp - gt)                                  gg_vae.py:139-156, gg_vq_vae.py:184-199, gg_vq_vae2.py:118-129
 *   SIGNED_MSE  (rx - tx)^2 + (ry - ty)^2                     gg_vq_vae.py:172-182
 *   MAXNORM     sl1(gp / (max gp + EPS) - gt / (max gt + EPS)), gradient through the max   gg_vae.py:158-173, gg_vq_vae.py:201-216
 *   ANGLE       sl1(atan2(ry, rx) - atan2(ty, tx))            gg_vae.py:176-190, gg_vq_vae.py:219-232
 *   MASKED      sl1(m * gp - m * gt), m = gt > mean gt        gg_vq_vae.py:234-247
 *   COSINE      1 - cos(normalize(rx, ry), normalize(tx, ty)) gg_vae.py:192-208, gg_vq_vae.py:249-264
 * `stats`: device float[8] written by the forward and read by the backward of MAXNORM / MASKED (may be NULL otherwise).
 * The backward passes take the upstream gradient as a device scalar (gscale_dev, may be NULL = 1). */
enum movae_edge_match {
    MOVAE_EDGE_MAG = 0, MOVAE_EDGE_SIGNED_MSE = 1, MOVAE_EDGE_MAXNORM = 2, MOVAE_EDGE_ANGLE = 3, MOVAE_EDGE_MASKED = 4,
    MOVAE_EDGE_COSINE = 5
};
int movae_edge_weights(const float* inputs, float* w_raw, float* wmax, int n, int h, int w, int c,
                       void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_edge_weighted_mse_fwd(const float* recons, const float* inputs, const float* w_raw, const float* wmax, float* out,
                                int n, int h, int w, int c, float scale, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_edge_weighted_mse_bwd(const float* recons, const float* inputs, const float* w_raw, const float* wmax,
                                const float* gscale_dev, float* drecons, int n, int h, int w, int c, float scale,
                                movae_stream_t stream);
int movae_edge_match_fwd(const float* recons, const float* inputs, float* out, int n, int h, int w, int c, float scale,
                         int mode, float* stats, void* ws, size_t ws_bytes, movae_stream_t stream);
/* tmp_a / tmp_b: two scratch tensors of the images' size (d loss / d Sobel-x and -y responses) */
int movae_edge_match_bwd(const float* recons, const float* inputs, const float* gscale_dev, float* drecons, float* tmp_a,
                         float* tmp_b, int n, int h, int w, int c, float scale, int mode, const float* stats,
                         movae_stream_t stream);

/* ---- vector quantiser ------------------------------------------------------------------------------
 * models/vq_vae.py:27-64: nearest code under ||x||^2 + ||e||^2 - 2 x.e (first index on ties), gather, and
 * sse[0] = sum (q - x)^2 (commitment and embedding losses are both sse/numel).  x,q: [rows][d], e: [k][d]. */
int movae_vq_nearest_fwd(const float* x, const float* e, float* q, int64_t* idx, float* sse, int32_t* used_count,
                         int rows, int k, int d, void* ws, size_t ws_bytes, movae_stream_t stream);
/* the same, and the two loss terms of models/vq_vae.py:51-52 written by the finalize kernel: mse2[0] = mse2[1] = sse / (rows * d) */
int movae_vq_nearest_fwd_mse(const float* x, const float* e, float* q, int64_t* idx, float* sse, int32_t* used_count, float* mse2,
                             int rows, int k, int d, void* ws, size_t ws_bytes, movae_stream_t stream);
/* dx = dq + gc * 2 (x - q)/numel ; de[k] = ge * 2/numel * sum_{idx[r]==k} (q[r] - x[r])   (gc, ge: device scalars, may be
 * NULL = 0; dx / de may be NULL).  The codebook gradient is a sorted segmented sum (no float atomics, bit-reproducible);
 * `ws` must hold movae_vq_bwd_ws_bytes(rows, k, d) bytes when de and ge are given. */
size_t movae_vq_bwd_ws_bytes(int rows, int k, int d);
int movae_vq_bwd(const float* x, const float* q, const int64_t* idx, const float* dq, const float* gc, const float* ge,
                 float* dx, float* de, int rows, int k, int d, void* ws, size_t ws_bytes, movae_stream_t stream);

/* ---- K-loss gradient aggregation ---------------------------------------------------------------------
 * torchjd GramianWeightedAggregator (base of utils/torchmoo/mgda.py:12, aligned_mtl.py:39): G = J J^T,
 * w = weighting(G), g = w @ J.   J is [k][m] row-major with leading dimension ldj, k <= MOVAE_MAX_K. */
#define MOVAE_MAX_K 8
size_t movae_gram_ws_bytes(int k, size_t m);
int movae_gram(const float* J, size_t ldj, int k, size_t m, float* G, void* ws, size_t ws_bytes, movae_stream_t stream);
/* UPGrad (torchjd; constructed main.py:1195): G/tr(G) (0 if tr<norm_eps) + reg_eps I; for each i solve
 * min 1/2 w'Gw s.t. w >= u_i e_i; sum rows.  pref may be NULL (u = 1/k).  Solved in fp64 on device. */
int movae_weights_upgrad(const float* G, int k, float norm_eps, float reg_eps, const float* pref, float* w, movae_stream_t stream);
/* the same projection on a differently normalised Gramian: MOVAE_UPGRAD_MIN_L2 = NUPGrad
 * (utils/torchmoo/nupgrad.py:115-158, main.py:1226), MOVAE_UPGRAD_COSINE = the other branch of PNUPGrad's coin flip
 * (utils/torchmoo/pnupgrad.py:13-24,127-134, main.py:1228); MOVAE_UPGRAD_TRACE is movae_weights_upgrad. */
int movae_weights_upgrad_norm(const float* G, int k, int norm_mode, float norm_eps, float reg_eps, const float* pref, float* w,
                              movae_stream_t stream);
/* movae_gram followed by movae_weights_upgrad_norm (dual == 0) or movae_weights_dualproj (dual != 0; norm_mode 0) in two launches
 * instead of three: the solver kernel folds the Gramian's block partials itself -- the arithmetic of movae_gram's final kernel, so
 * G [k][k] and w [k] are bit-identical to the two separate calls. */
int movae_gram_upgrad(const float* J, size_t ldj, int k, size_t m, float* G, int norm_mode, float norm_eps, float reg_eps,
                      const float* pref, float* w, int dual, void* ws, size_t ws_bytes, movae_stream_t stream);
/* MGDA Frank-Wolfe (utils/torchmoo/mgda.py:221-367); losses may be NULL for norm NONE/L2. info[0]=iterations */
int movae_weights_mgda(const float* G, int k, int norm, const float* losses, float epsilon, int max_iters,
                       float* w, int32_t* info, movae_stream_t stream);
/* StableMGDA (utils/torchmoo/mgda.py:139-153,286-317; COMFORT's --comfort_mgda_stable): the (normalised) Gramian's
 * eigenvalues are clamped to >= min_eigenvalue and the matrix reconstructed before the Frank-Wolfe iteration. */
int movae_weights_mgda_stable(const float* G, int k, int norm, const float* losses, float epsilon, int max_iters,
                              float min_eigenvalue, float* w, int32_t* info, movae_stream_t stream);
/* Aligned-MTL (utils/torchmoo/aligned_mtl.py:97-133) */
int movae_weights_amtl(const float* G, int k, int scale_mode, const float* pref, float* w, movae_stream_t stream);
/* torchjd aggregators that main.py:1196-1222 also offers (third-party torchjd @ main, absent from the reference tree:
 * restated from the published algorithms, parity unpinned):
 *   DualProj  one dual-cone projection of the preference vector (default mean weights) on the trace-normalised,
 *             regularised Gramian -- movae_weights_upgrad's QP solved once;
 *   PCGrad    gradient surgery on the Gramian; perm = K rows of a permutation of 0..K-1 (int32, device), row i is the
 *             order in which task i is de-conflicted against the others (the reference: torch.randperm per task);
 *   IMTL-G    w = pinv(G) d / sum(pinv(G) d), d_i = sqrt(G_ii); zeros when the sum vanishes;
 *   CAGrad    w = 1/K + c g0 / sqrt(w*'G w*) w*, w* = argmin over the simplex of (G 1/K)'w + c g0 sqrt(w'Gw), g0 = sqrt(1/K' G 1/K)
 *             (main.py:1216-1217: c = 1.0); the mean weights when c g0 or sqrt(w*'G w*) is <= norm_eps. */
int movae_weights_dualproj(const float* G, int k, float norm_eps, float reg_eps, const float* pref, float* w, movae_stream_t stream);
int movae_weights_pcgrad(const float* G, int k, const int32_t* perm, float* w, movae_stream_t stream);
int movae_weights_imtlg(const float* G, int k, float* w, movae_stream_t stream);
int movae_weights_cagrad(const float* G, int k, float c, float norm_eps, float* w, movae_stream_t stream);
/* constant weightings (torchjd Sum / Mean) */
int movae_weights_const(int k, float value, float* w, movae_stream_t stream);
/* g[m] (+)= sum_i w[i] J[i][:]  ; also usable as the hook's J.T @ w (main.py:112-118) */
int movae_combine(const float* J, size_t ldj, int k, size_t m, const float* w, float* g, int accumulate, movae_stream_t stream);
/* cos(J.T @ w, mean_rows(J)) -> out[0] (main.py:108-119) */
int movae_gd_similarity(const float* J, size_t ldj, int k, size_t m, const float* w, float* out,
                        void* ws, size_t ws_bytes, movae_stream_t stream);

/* ---- optimizer tail (torch.optim.Adam semantics, main.py:1169-1178,214) ------------------
 * flat multi-tensor Adam over one contiguous fp32 arena; step_dev holds the step count as float. */
int movae_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int decoupled_wd, int step, movae_stream_t stream);
/* the same update for a LIST of tensors in one launch per 64 tensors (torch.optim.Adam(foreach) semantics:
 * main.py:1169-1178 builds it, main.py:214 steps it).  p/g/m/v/numel are HOST arrays of n_tensors device
 * pointers / element counts.  hyper_dev == NULL: `step` (>= 1) is the step count and lr the learning rate.
 * hyper_dev != NULL: device float[2] = {steps made so far, lr}; the update is made for step counter + 1 with the device lr
 * (`step` and `lr` arguments are ignored) and the counter is advanced inside the same launch, by the block that finishes last
 * -- the form a captured hipGraph replays.  (One such call at a time per process: the kernel keeps its arrival count in a
 * device global.) */
int movae_adam_multi(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                     const size_t* numel, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int decoupled_wd, int step, float* hyper_dev, movae_stream_t stream);
/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) (main.py:211-212) over a LIST of gradient tensors in three
 * launches per 64 tensors: total_sumsq_dev[0] receives the squared total L2 norm (its sqrt is the value torch
 * returns), every gradient is scaled in place by min(max_norm / (norm + 1e-6), 1).  g / numel are HOST arrays. */
int movae_clip_grad_norm_multi(int n_tensors, float* const* g, const size_t* numel, float max_norm, float* total_sumsq_dev,
                               void* ws, size_t ws_bytes, movae_stream_t stream);
/* sumsq of a flat arena into out[0] (clip_grad_norm_, main.py:211-212) */
int movae_sumsq(const float* x, size_t n, float* out, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_scale_by_clip(float* g, size_t n, const float* sumsq_dev, float max_norm, movae_stream_t stream);

/* ---- opt-in reduced-precision operands (BASELINE.json configs[1] names bf16; the reference itself is fp32 end to end) ----------
 * MOVAE_DTYPE_BF16: the 128x128 implicit-GEMM convolution kernels (forward, input gradient, weight gradient -- the layers that
 * are MFMA-bound at the C3-C5 shapes) round their two operands to bf16 on the way into LDS and multiply on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; tensors in memory, master weights, BatchNorm, losses, aggregation and the
 * optimizer stay fp32.  The attention entry points (movae_attn_*, movae_causal_attn_*) take their bf16-operand instances in this
 * mode too: q and k after RoPE, v, dO, the dropout-scaled probabilities and dS are rounded, everything else stays fp32; a backward
 * must run under the dtype of its forward (the saved lse carries the forward's rounding).  Process-wide, returns the previous setting.  The default, MOVAE_DTYPE_F32, is the parity path: results
 * under bf16 are held to their own, looser tolerance (tests/test_hip_bf16.py, tests/test_hip_bf16_attention.py), never to the fp32 oracle's. */
#define MOVAE_DTYPE_F32 0
#define MOVAE_DTYPE_BF16 1
int movae_set_compute_dtype(int dtype);

/* A weight gradient's split-K reduce need not be a launch of its own on the backward's dependency chain: nobody reads the weight
 * gradient before the aggregation / the optimizer.  movae_reduce_defer(1) arms the NEXT movae_conv*_wgrad* / *_dgrad_wgrad* call
 * (one call): its reduce is parked instead of launched, and the next implicit-GEMM launch on the same stream carries it as extra
 * blocks behind its own (same arithmetic, same order).  The caller guarantees (mo-vae_amd/ops.py does) that until then (a) nothing
 * reads the call's dw / dbias destinations and (b) nothing writes the scratch arena `ws` the call was given.  A second armed call,
 * a following call's bias column sums, or movae_reduce_flush() launch a still-parked reduce stand-alone.  Returns the previous
 * arming.  movae_reduce_defer_stats: out3 = {parked, carried by a later launch, launched stand-alone after all}; returns 1 while a
 * reduce is parked. */
int movae_reduce_defer(int on);
int movae_reduce_flush(void);
int movae_reduce_defer_stats(long long* out3, int reset);
/* Only reduces whose slabs hold at most this many bytes are parked (a parked reduce runs with its carrier's occupancy: right for a
 * launch-bound reduce, wrong for a bandwidth-bound one).  Default 12 MiB (MOVAE_DEFER_MAX_BYTES; measured: C2 0.841 -> 0.816 ms, C4 4.49 -> 4.44, larger slabs cost their carrier more than the launch saves); bytes < 0 only reads.  Returns the
 * previous value. */
long long movae_reduce_defer_max_bytes(long long bytes);

/* ---- measurement hook (bench.py's roofline leg only; no reference counterpart) ------------------------
 * on != 0: the conv family launches ONLY its main MFMA kernel (split-K reduce / bias column-sum launches are
 * skipped, so outputs are incomplete) so that one kernel can be timed between HIP events.  Process-wide;
 * returns the previous setting.  Never enabled by the product path. */
int movae_bench_main_kernel_only(int on);
/* name (as rocprofv3 prints it, without the argument list) of the main kernel the most recent conv-family call
 * on this process dispatched to, e.g. "igemm2_bwd<64,64>" -- lets bench.py group its HIP-event timings per kernel */
const char* movae_bench_last_kernel(void);
/* names of the split-K reduce kernels the conv family chose since the previous read (a parked reduce is named when it is
 * parked), joined with " + " in launch order, e.g. "splitk_reduce_cls + splitk_reduce_flat"; "" if there was none.  Reading
 * clears the list.  The main kernel's name does not change with the split factor: this is what tells a test which of
 * splitk_reduce / _wide / _vec / _flat / _cls / _stats a call went through. */
const char* movae_bench_last_reduce(void);
/* s > 0 pins the conv family's split-K factor (tools/conv_microbench.py tuning sweeps); 0 restores the heuristic.
 * Returns the previous value. */
int movae_bench_force_split(int s);
/* mode > 0: every conv-family call whose shape the block-internal split-K kernels (csrc/kgemm.h) can serve takes them, whatever
 * the size heuristic says; mode < 0: none does; 0: the heuristic (small, latency-bound problems only).  Lets the parity tests run
 * the whole conv test matrix through either family.  Returns the previous mode. */
int movae_bench_force_kgemm(int mode);
/* n > 0 pins the fewest 128x128 work items from which the conv dispatcher prefers its big tiles (igemm2_*<128,128>,
 * igemm2_wgrad<64,128>), whatever MOVAE_BIG_TILE_MIN says: n = 1 lets a test reach them at shapes of a few tiles.  0 restores
 * the environment's value or the default (256).  Returns the previous pin (0: none).  Never set by the product path. */
int movae_bench_big_tile_min(int n);

/* ---- BatchNorm fused into its neighbouring convolutions -----------------------------------------
 * models/vae.py:119-126,149-158: Conv2d / ConvTranspose2d -> BatchNorm2d (training statistics) -> LeakyReLU chains.  Instead of
 * a statistics pass and an apply pass per BatchNorm, (1) the conv that PRODUCES y emits the per-channel partial sums of y from
 * its epilogue (or from its split-K reduction), (2) movae_bn_finalize turns them into the saved statistics, the running
 * statistics and the folded map scale = gamma * rstd, shift = beta - mean * scale, and (3) the conv that CONSUMES the
 * normalised activation applies act(scale[c] * y + shift[c]) between its global load and its LDS store (forward and weight
 * gradient alike): the normalised tensor is never written.
 * movae_fuse_t asks one *_f call for (1) and / or (3).  in_scale == NULL: plain input.  stats == NULL: no statistics.  On return
 * stats_parts is the number of partial pairs written per channel, stats[(p * 2 + {0: sum, 1: sum of squares}) * co + c]; 0 when
 * the dispatched kernel cannot emit them (use movae_bn_stats).  A requested input transform that the dispatched kernel cannot
 * apply returns -2 (unsupported) BEFORE anything is launched: materialise with movae_scale_shift_act and call the plain entry.
 * in_slope: leaky-ReLU slope of the fused activation (1 = none, 0 = ReLU).  The *_f entry points are otherwise identical to
 * their plain namesakes (which call them with fuse == NULL). */
typedef struct movae_fuse {
    const float* in_scale; /* [ci] device pointers, 16-byte aligned, ci % 4 == 0 */
    const float* in_shift;
    float in_slope;
    float* stats;          /* device buffer for the partial sums (fwd entry points, act == none, no fused activation) */
    size_t stats_cap;      /* floats available at stats */
    int stats_parts;       /* OUT */
    /* input-gradient passes (dgrad / dgrad_wgrad entry points): dx is the gradient `dout` w.r.t. the never-materialised output
     * act(bn_scale[c] * bn_y + bn_shift[c]) of a fused BatchNorm over the raw conv output bn_y [n][hi][wi][ci] (shared by the
     * `groups` cotangents).  The epilogue / split-K reduce then also emits that BatchNorm's backward sums per cotangent group,
     * bn_part[((g * bn_ppg + p) * 2 + {0,1}) * ci + c] = partial (sum d, sum d * bn_y), d = dout * act'(...), for
     * movae_bn_bwd_finalize.  bn_ppg == 0 on return: not produced (shape / kernel without the epilogue). */
    const float* bn_y;
    const float* bn_scale;
    const float* bn_shift;
    float bn_slope;
    float* bn_part;
    size_t bn_cap;         /* floats available at bn_part */
    int bn_ppg;            /* OUT: partial pairs per group and channel */
    /* input-gradient passes, alternatively: dx is the gradient w.r.t. the OUTPUT of the epilogue activation of the layer before
     * (Conv2d(bias) -> LeakyReLU / ReLU -> this layer, models/betatc_vae.py:104-110, vq_vae.py:36-47), whose stored output is
     * ep_act_y [n][hi][wi][ci] (shared by the `groups` cotangents).  The epilogue / split-K reduce then stores
     * dx * act'(ep_act_y) -- the gradient w.r.t. that layer's PRE-activation -- and sets ep_act_done = 1; 0 on return: not applied
     * (kernel without the epilogue), dx is the plain input gradient and the caller runs movae_act_bwd. */
    const float* ep_act_y;
    int ep_act;            /* MOVAE_ACT_* of that layer */
    float ep_slope;
    int ep_act_done;       /* OUT: everything asked of the epilogue (ep_act_y and / or ep_res) was applied */
    /* ... and / or the layer is the first of a residual block's branch (out = branch(x) + x, models/vq_vae.py:127-145,
     * vq_vae2.py:13-28): ep_res [groups][n][hi][wi][ci] -- the gradient w.r.t. the block's output, i.e. the identity branch's
     * share -- is added to dx, which then is the block's complete input gradient. */
    const float* ep_res;
} movae_fuse_t;
int movae_conv2d_fwd_f(const float* x, const float* w, const float* bias, float* y,
                       int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                       int act, float slope, void* ws, size_t ws_bytes, movae_stream_t stream, movae_fuse_t* fuse);
int movae_convT2d_fwd_f(const float* x, const float* w, const float* bias, float* y,
                        int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                        int act, float slope, void* ws, size_t ws_bytes, movae_stream_t stream, movae_fuse_t* fuse);
/* backward passes: `fuse` describes the activation operand x (only in_scale / in_shift / in_slope are read) */
int movae_conv2d_wgrad_grouped_f(int groups, const float* dy, const float* x, float* const* dw, float* const* dbias,
                                 int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                                 int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream, const movae_fuse_t* fuse);
int movae_convT2d_wgrad_grouped_f(int groups, const float* dy, const float* x, float* const* dw, float* const* dbias,
                                  int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                                  int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream, const movae_fuse_t* fuse);
int movae_conv2d_dgrad_wgrad_grouped_f(int groups, const float* dy, const float* w, const float* x, float* dx,
                                       float* const* dw, float* const* dbias,
                                       int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                                       int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream, const movae_fuse_t* fuse);
int movae_convT2d_dgrad_wgrad_grouped_f(int groups, const float* dy, const float* w, const float* x, float* dx,
                                        float* const* dw, float* const* dbias,
                                        int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                                        int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream, const movae_fuse_t* fuse);
int movae_conv2d_dgrad_f(const float* dy, const float* w, float* dx,
                         int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                         void* ws, size_t ws_bytes, movae_stream_t stream, movae_fuse_t* fuse, int groups);
int movae_convT2d_dgrad_f(const float* dy, const float* w, float* dx,
                          int n, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int pad,
                          void* ws, size_t ws_bytes, movae_stream_t stream, movae_fuse_t* fuse, int groups);
/* BatchNorm backward from the sums above (models/vae.py:119-126 through autograd): per cotangent group g
 *   dbeta[g] = S1, dgamma[g] = rstd * (S2 - mean * S1)            (dgamma / dbeta: HOST arrays of device pointers, NULLs allowed)
 *   coef[g][0..2][c] such that dy = coef0 * d + coef1 * y + coef2, d = dout * act'(scale * y + shift)
 * and the one pass that forms dy [groups][rows][c] from dout [groups][rows][c] and y [rows][c].  accumulate != 0 adds to
 * dgamma / dbeta. */
int movae_bn_bwd_finalize(const float* bn_part, size_t bn_cap, int ppg, int groups, int rows, int c, const float* gamma,
                          const float* save_mean, const float* save_rstd, float* const* dgamma, float* const* dbeta, float* coef,
                          int accumulate, movae_stream_t stream);
int movae_bn_bwd_apply(const float* dout, const float* y, const float* scale, const float* shift, float slope, const float* coef,
                       float* dy, int groups, size_t rows, int c, movae_stream_t stream);
/* The two calls above as one: with few partials per group (the deep layers) a single launch folds them per 32-channel slice and forms
 * dy; otherwise the two launches.  coef is scratch of [groups][3][c] floats either way. */
int movae_bn_bwd_finalize_apply(const float* bn_part, size_t bn_cap, int ppg, int groups, size_t rows, int c, const float* gamma,
                                const float* save_mean, const float* save_rstd, float* const* dgamma, float* const* dbeta, float* coef,
                                int accumulate, const float* dout, const float* y, const float* scale, const float* shift, float slope,
                                float* dy, movae_stream_t stream);
/* partial sums -> mean / rstd (saved for movae_bn_act_bwd), scale / shift (for the consumers), running statistics with
 * nn.BatchNorm2d's momentum rule and unbiased variance, num_batches_tracked += 1 (each may be NULL).  rows = n * h * w.
 * stats_cap / bn_cap: floats available at the partials buffer -- with more than 256 partials and room behind them, a first
 * stage folds them to 64 rows there (the buffer is scratch: its contents are not preserved). */
int movae_bn_finalize(const float* stats, size_t stats_cap, int parts, int rows, int c, const float* gamma, const float* beta, float eps,
                      float momentum, float* save_mean, float* save_rstd, float* scale, float* shift, float* running_mean,
                      float* running_var, long long* num_batches_tracked, movae_stream_t stream);
/* the same partial sums from one read of y, for producers whose kernel cannot emit them; *parts_out is a HOST int */
int movae_bn_stats(const float* y, int rows, int c, float* stats, size_t stats_cap, int* parts_out, movae_stream_t stream);
/* out = leaky_relu(scale[c] * y + shift[c], slope): materialises a fused BatchNorm output */
int movae_scale_shift_act(const float* y, const float* scale, const float* shift, float* out, size_t rows, int c, float slope,
                          movae_stream_t stream);
/* name of the host dispatch branch the most recent successful BatchNorm call on this process took (the sibling of
 * movae_bench_last_kernel for this family; "" before the first one; a refused call leaves it as it was):
 *   movae_bn_act_fwd             fwd_small | fwd_stats4+apply_vec | fwd_stats4+apply_scalar | fwd_stats+apply_scalar |
 *                                fwd_eval+apply_vec | fwd_eval+apply_scalar
 *   movae_bn_act_bwd[_grouped]   bwd_small | bwd_vec4 | bwd_scalar
 *   movae_bn_finalize            finalize | fold+finalize
 *   movae_bn_bwd_finalize        bwd_finalize | bwd_fold+finalize
 *   movae_bn_bwd_apply           bwd_apply
 *   movae_bn_bwd_finalize_apply  bwd_fused | bwd_finalize+apply | bwd_fold+finalize+apply
 *   movae_scale_shift_act        scale_shift_act
 * Tests assert it so that a moved dispatch threshold fails them instead of changing what they cover. */
const char* movae_bn_last_path(void);

/* ---- PixelCNN prior over the VQ code grids (models/pixelcnn_prior.py, trained by main.py:890-1085) -------
 * The prior's convolutions are movae_conv2d_* calls; MaskedConv2d (pixelcnn_prior.py:25-54) multiplies its weight by the
 * mask IN PLACE before every forward (movae_mul with y == a).
 *   movae_embedding_fwd    nn.Embedding forward of the code grid     pixelcnn_prior.py:306 (x = self.embedding(x)), :371
 *                          y[r][:] = weight[idx[r]][:]; idx int64 [rows] (a [B,H,W] grid gives NHWC activations directly)
 *   movae_embedding_bwd    its gradient: dweight[k][:] = sum_{r: idx[r]==k} dy[r][:] -- rows sorted by (code, row) and summed in
 *                          fixed order (no float atomics, bit-reproducible); ws >= movae_vq_bwd_ws_bytes(rows, k, d)
 *   movae_gated_residual_* GatedResBlock's combine: out = res + gate * feat with gate = sigmoid(conv_gate), feat = tanh(conv_feature)
 *                          already activated by the conv epilogues            pixelcnn_prior.py:85-90; n %% 4 == 0
 *   movae_cross_entropy_*  F.cross_entropy(logits.permute(0,2,3,1).reshape(-1,K), z.reshape(-1)) (mean reduction)
 *                          main.py:1003-1006,1026-1029; pixelcnn_prior.py:392-395.  logits [rows][k] (NHWC logits are that
 *                          matrix as they lie), lse [rows] is kept for the backward; gscale_dev: device scalar upstream gradient
 *                          or NULL (= 1). */
int movae_embedding_fwd(const float* weight, const int64_t* idx, float* y, size_t rows, int k, int d, movae_stream_t stream);
int movae_embedding_bwd(const float* dy, const int64_t* idx, float* dweight, int rows, int k, int d,
                        void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_gated_residual_fwd(const float* res, const float* gate, const float* feat, float* out, size_t n, movae_stream_t stream);
int movae_gated_residual_bwd(const float* dout, const float* gate, const float* feat, float* dgate, float* dfeat, size_t n,
                             movae_stream_t stream);
int movae_mul(const float* a, const float* b, float* y, size_t n, movae_stream_t stream);
size_t movae_cross_entropy_ws_bytes(size_t rows);
int movae_cross_entropy_fwd(const float* logits, const int64_t* target, float* loss, float* lse, size_t rows, int k,
                            void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_cross_entropy_bwd(const float* logits, const int64_t* target, const float* lse, const float* gscale_dev, float* dlogits,
                            size_t rows, int k, movae_stream_t stream);

/* ---- Cached ancestral sampling for the PixelCNN prior (pixelcnn_prior.py:323-349 PixelCNN.sample) ---------------------------
 * The reference runs a full-grid forward for each of the H*W positions and keeps one pixel's logits.  The network is causal,
 * so movae_prior_sample_step computes raster position (i, j) alone, for every sample of the batch, in one launch:
 *   conv_in (mask A) over the causal taps of h0 [B,H,W,D0] = embedding(code) ++ condition (zero outside the grid)  -> x [C]
 *   per GatedResBlock l: a = relu(conv1 x + b), stored to acache[l][B,H,W,C/2] at (i, j); m = relu(masked-B 3x3 over acache[l],
 *     the centre tap being that a); x += sigmoid(conv_gate m) * tanh(conv_feature m)
 *   logits = conv(relu(conv(relu(x))))  [K], stored raw to logits_out [B,H,W,K] where that is not NULL
 *   code = forced[b,i,j] where forced is not NULL, else the smallest k with u < cdf_k of softmax(logits * inv_temperature),
 *     clamped to K - 1; u = uniforms[b,i,j] where uniforms is not NULL, else 24 bits of Philox4x32-10 under key `seed` at
 *     counter (sample_base + b, i*W + j, draw) -- a sample's draws do not depend on the batch it sits in
 *   codes[b,i,j] = code (int64);  h0[b,i,j,0..E-1] = embedding row `code`
 * Call it for (i, j) in raster order on one stream; h0's channels E..D0-1 hold the condition beforehand.  No workgroup talks to
 * another and nothing is atomic: results are bit-identical from run to run and independent of B.
 *   wpack: one 16-byte-aligned fp32 buffer of movae_prior_sample_pack_floats(...) floats (0 for an unsupported shape), every
 *     matrix stored [row][cout padded to a multiple of 4, zero filled] with row = tap * cin + ci over the CAUSAL taps in raster
 *     order, followed by its bias [cout padded]:  conv_in | per block: conv1, conv2 (taps (-1,-1) (-1,0) (-1,1) (0,-1) (0,0)),
 *     gate ++ feature side by side ([C/2][2 * pad4(C)], bias alike) | head conv 1 | head conv 2 | embedding [K][E].
 *   Supported: C even <= 256, 1 <= E <= D0 <= 256, K <= 2048, ks odd <= 7, any B, H, W >= 1, L >= 0 (3x3 block convs). */
size_t movae_prior_sample_pack_floats(int D0, int E, int C, int L, int K, int ks);
int movae_prior_sample_step(const float* wpack, size_t wpack_floats, float* h0, float* acache, int64_t* codes, const int64_t* forced,
                            const float* uniforms, float* logits_out, int B, int H, int W, int D0, int E, int C, int L, int K, int ks, int i,
                            int j, float inv_temperature, unsigned long long seed, unsigned long long draw, unsigned long long sample_base,
                            movae_stream_t stream);

/* ---- Cached ancestral sampling for the PixelSNAIL prior (pixelcnn_prior.py:159-259 PixelSNAIL; :95-156 its blocks) -------------
 * The same step as movae_prior_sample_step, with NB PixelSNAILBlocks of NR GatedResBlocks each between conv_in and the head, and
 * the attention's K and V rows of every earlier position kept in a cache.  Raster position (i, j) of every sample, one launch:
 *   x = conv_in (mask A) over the causal taps of h0 [B,H,W,D0] = embedding(code) ++ the 2 position channels ++ condition
 *   per PixelSNAILBlock nb:  r = its NR gated blocks applied to x, over acache[nb * NR + g][B,H,W,C/2] as above
 *     q ++ k ++ v = r [Wq ++ Wk ++ Wv] + b (one product);  k, v stored to kvcache[nb][B][H*W][2P] at raster index i*W + j
 *       (k in columns 0 .. P-1, v in P .. 2P-1, P = heads * hd; head h = channels h*hd .. h*hd+hd-1)
 *     per head: o = softmax(q . k_t / sqrt(hd), t = 0 .. i*W + j, the position itself included) V, written in the reference's
 *       channel order d * heads + h;  a = out_proj(o);  x = x + (out_conv([r ++ a]) + r)
 *   head, draw, codes and h0's embedding channels exactly as movae_prior_sample_step (same Philox keying); no dropout.
 * The keys of a (sample, head) are split over the lanes of one wave in a fixed pattern and the online-softmax partials merged in a
 * fixed butterfly order; no atomics: results are bit-identical from run to run and independent of B and of the sample's slot.
 *   wpack: as above, of movae_prior_snail_sample_pack_floats(...) floats:  conv_in | per PixelSNAILBlock: its NR gated blocks (conv1,
 *     conv2, gate ++ feature), q ++ k ++ v side by side ([C][3 * pad4(P)], bias alike), out_proj [P][pad4(C)] (rows in the order
 *     d * heads + h), out_conv [2C][pad4(C)] (rows r, then attention) | head conv 1 | head conv 2 | embedding [K][E].
 *   Supported: what movae_prior_sample_step supports with E + 2 <= D0 <= 256, 1 <= hd <= 64, P <= 256, NB >= 0, NR >= 0; the LDS
 *     need (at most 140 KiB at these limits) is checked against the 160 KiB of a workgroup.  kvcache 16-byte aligned. */
size_t movae_prior_snail_sample_pack_floats(int D0, int E, int C, int NB, int NR, int heads, int hd, int K, int ks);
int movae_prior_snail_sample_step(const float* wpack, size_t wpack_floats, float* h0, float* acache, float* kvcache, int64_t* codes,
                                  const int64_t* forced, const float* uniforms, float* logits_out, int B, int H, int W, int D0, int E, int C,
                                  int NB, int NR, int heads, int hd, int K, int ks, int i, int j, float inv_temperature,
                                  unsigned long long seed, unsigned long long draw, unsigned long long sample_base, movae_stream_t stream);

/* ---- PixelSNAIL's causal self-attention (models/pixelcnn_prior.py:95-135 CausalAttention2d.forward; :16-22 the mask) ------
 * Replaces  attn = matmul(q, k^T) / sqrt(hd); masked_fill(tril == 0, -inf); softmax(-1); dropout; out = matmul(attn, v) and the
 * permute(0, 2, 3, 1).reshape of `out` (:118-131) -- fused, FlashAttention-2 style: no [L, L] matrix is ever stored.
 *   q, k, v     [B, L, ld] row-major (the NHWC 1x1-conv outputs); head h reads channels h*hd .. h*hd+hd-1 in place
 *   out, dout   [B, L, heads*hd], element (h, d) at channel d*heads + h: the reference's channel order after its permute
 *   lse         [B*heads, L] natural log-sum-exp of the scaled, masked scores (written by the forward, read by the backward)
 *   dq, dk, dv  written in the q / k / v layout (same ld)
 *   1 <= hd <= 64 (larger is refused), any L >= 1.  Key j is visible from query i iff j <= i.
 *   p in [0, 1): dropout on the probabilities, P' = P * Z / (1 - p); p == 0 takes the no-dropout kernels.  Z(bh, i, j) is a pure
 *   function of (seed, draw, bh, i, j) -- Philox4x32-10 -- so the backward regenerates it; movae_causal_attn_dropout_mask writes
 *   it out (keep [BH][L][L] uint8, 1 = kept) as a test and measurement hook.
 *   ws >= movae_causal_attn_ws_bytes(B, heads, L) (the 4096-byte header included).  No float atomics: the gradients are
 *   bit-identical from run to run. */
int movae_causal_attn_fwd(const float* q, const float* k, const float* v, long ld, float* out, float* lse, int B, int heads, int L,
                          int hd, float p, unsigned long long seed, unsigned long long draw, movae_stream_t stream);
size_t movae_causal_attn_ws_bytes(int B, int heads, int L);
int movae_causal_attn_bwd(const float* q, const float* k, const float* v, long ld, const float* out, const float* dout, const float* lse,
                          float* dq, float* dk, float* dv, int B, int heads, int L, int hd, float p, unsigned long long seed,
                          unsigned long long draw, void* ws, size_t ws_bytes, movae_stream_t stream);
int movae_causal_attn_dropout_mask(uint8_t* keep, int BH, int L, float p, unsigned long long seed, unsigned long long draw,
                                   movae_stream_t stream);

/* ---- the ViT Sphere Encoder's bidirectional self-attention with RoPE (models/sphere_encoder_vit.py:143-167 AttentionWithRoPE.forward;
 * :71-89 apply_rotary_pos_emb) -- the kernels above with the causal mask off: every query sees every key j < L.
 *   q, k, v     [B, L, ld] row-major, head h at channels h*hd .. h*hd+hd-1, read in place.  With the packed qkv projection [B, L, 3C]
 *               pass q = qkv, k = qkv + C, v = qkv + 2C and ld = 3C; dq / dk / dv likewise into one [B, L, 3C] buffer.
 *   out, dout   [B, L, heads*hd], element (h, d) at channel h*hd + d: the reference's (attn @ v).transpose(1, 2).reshape(B, N, C)
 *   rope_cos, rope_sin   [L, hd/2] tables of the rotation angles (both or neither; null: no rotation), built by the host as the
 *               reference does: outer(arange(L), 1 / base^(arange(0, hd, 2) / hd)), then cos / sin in fp32.  The rotation is
 *               interleaved, (u[2t], u[2t+1]) -> (u[2t] c - u[2t+1] s, u[2t] s + u[2t+1] c), applied to q and k as they are loaded; dq
 *               and dk are rotated back before the store; no rotated copy of q or k is written.  RoPE needs an even hd.
 *   lse         [B*heads, L] as above.  1 <= hd <= 64, any L >= 1.  p must be 0: attention dropout is refused.
 *   ws >= movae_attn_ws_bytes(B, heads, L).  No float atomics: the gradients are bit-identical from run to run. */
int movae_attn_fwd(const float* q, const float* k, const float* v, long ld, const float* rope_cos, const float* rope_sin, float* out,
                   float* lse, int B, int heads, int L, int hd, float p, movae_stream_t stream);
size_t movae_attn_ws_bytes(int B, int heads, int L);
int movae_attn_bwd(const float* q, const float* k, const float* v, long ld, const float* rope_cos, const float* rope_sin, const float* out,
                   const float* dout, const float* lse, float* dq, float* dk, float* dv, int B, int heads, int L, int hd, float p, void* ws,
                   size_t ws_bytes, movae_stream_t stream);

/* ---- row operators of the ViT Sphere Encoder (csrc/vit.hip): fp32, row-major [rows][d], fixed-order reductions, no float atomics ----
 * Row norm over the last dimension.  mode 0: LayerNorm (nn.LayerNorm: biased variance; the caller passes eps 1e-5), weight and bias
 * nullable; mode 1: RMSNorm  x / sqrt(mean(x^2) + eps) * weight  (the reference's models/sphere_encoder.py rms_norm and models/sphere_encoder_vit.py:34-50 RMSNorm; eps
 * 1e-6), weight nullable, no bias.  pos (nullable) [pos_rows][d] is added after the affine: out = norm(x) * w + b + pos[row % pos_rows].
 * The forward saves rstd[rows] (and mean[rows] in mode 0) for the backward, which writes whichever of dx, dweight, dbias are given:
 * dweight / dbias through per-block partial rows in ws (>= movae_rownorm_ws_bytes(rows, d)) folded in order. */
int movae_rownorm_fwd(const float* x, const float* weight, const float* bias, const float* pos, int pos_rows, float* out, float* mean,
                      float* rstd, long rows, int d, int mode, float eps, movae_stream_t stream);
size_t movae_rownorm_ws_bytes(long rows, int d);
int movae_rownorm_bwd(const float* dy, const float* x, const float* weight, const float* mean, const float* rstd, float* dx, float* dweight,
                      float* dbias, long rows, int d, int mode, void* ws, size_t ws_bytes, movae_stream_t stream);
/* y = gelu(x + bias[col]) with the exact erf form (nn.GELU() default) on x[rows][c]; bias nullable.  The backward takes the saved x
 * WITHOUT the bias (the bias-free output of the linear in front) and the bias, and writes dx = dy * gelu'(x + bias); the bias gradient
 * is the column sum of dx (movae_colsum). */
int movae_bias_gelu_fwd(const float* x, const float* bias, float* y, long rows, int c, movae_stream_t stream);
int movae_bias_gelu_bwd(const float* dy, const float* x, const float* bias, float* dx, long rows, int c, movae_stream_t stream);
/* Unpatchify + tanh (models/sphere_encoder_vit.py:125-140, :388): x [b][(h/patch)*(w/patch)][patch*patch*c] -> out NHWC [b][h][w][c];
 * token (i, j), channel (pi*patch + pj)*c + ch goes to pixel (i*patch + pi, j*patch + pj), channel ch.  The backward takes dout and
 * the saved out: dx = dout * (1 - out^2) at the source position. */
int movae_unpatchify_act_fwd(const float* x, float* out, int b, int h, int w, int c, int patch, movae_stream_t stream);
int movae_unpatchify_act_bwd(const float* dout, const float* out, float* dx, int b, int h, int w, int c, int patch, movae_stream_t stream);
/* y[row][:] = x[row][:] + pos[row % pos_rows][:]  (SinusoidalPosEmbedding.forward, :53-68); rows is a multiple of pos_rows */
int movae_add_rows_bcast(const float* x, const float* pos, float* y, long rows, int pos_rows, int d, movae_stream_t stream);

/* ---- reconstruction metrics of the final evaluation (main.py:335-373 over utils/metrics.py ssim :14-80, ssnr :108-154,
 * psnr :157-203) ----------------------------------------------------------------------------------------------------------
 * One chunk of n (real, recon) image pairs of c x h x w, each operand given by its element strides (n, c, h, w) -- e.g. NCHW
 * images and the decoder's NHWC buffer seen as NCHW, with no copy.  Like the reference, each operand is mapped to
 * clamp((x + 1) / 2, 0, 1) if its minimum over the chunk is negative, else clamp(x, 0, 1); that decision is made on the device.
 * SSIM uses the separable form of the reference's Gaussian window (sigma 1.5, window_size odd in 3..15) with zero padding.
 * out (device float[3 + 3 n]): [0] ssim (mean of the SSIM map over n c h w), [1] psnr (mean over the images of
 * 20 log10(max_val) - 10 log10(max(mse, 1e-10))), [2] ssnr (mean over the images of 10 log10(max(var(real), 1e-10) /
 * max(mse, 1e-10)), unbiased variance), then per image: [3 + i] SSIM, [3 + n + i] MSE, [3 + 2 n + i] SSNR in dB.
 * ws >= movae_recon_metrics_ws_bytes(n, c, h, w) bytes (the 4096-byte header included; this call uses only the scratch behind
 * it); three launches, fixed summation order (fp64 partials, no float atomics): bit-identical results from run to run. */
size_t movae_recon_metrics_ws_bytes(int n, int c, int h, int w);
int movae_recon_metrics(const float* real, long long rs_n, long long rs_c, long long rs_h, long long rs_w,
                        const float* recon, long long ps_n, long long ps_c, long long ps_h, long long ps_w,
                        int n, int c, int h, int w, int window_size, float max_val, float* out, void* ws, size_t ws_bytes,
                        movae_stream_t stream);

/* ---- the perceptual (VGG16 feature) loss around its convolutions (csrc/perceptual.hip; utils/objectives.py:53-79 PerceptualLoss) ----
 * PerceptualLoss._norm_input (:66-72) on g (1..8) same-shape fp32 NHWC tensors of n elements each with C = 3 (channel = index % 3):
 * per tensor, x -> (x + 1) / 2 if ANY of its elements is negative, then clamp to [0, 1], then (x - mean_c) / std_c with the ImageNet
 * mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225).  The decision stays on the device: two launches for the whole group (block
 * partials in ws, folded by the normalise launch), no atomics.  x, y, dy, dx are HOST arrays of g device pointers; flags is a device
 * int[g], written by the forward (1 = rescaled) and read by the backward.  ws >= movae_vgg_prep_ws_bytes(g).
 * Backward: dx = dy * (flag ? 0.5 : 1) / std_c where 0 <= x' <= 1 (x' the value before the clamp, recomputed from x; the interval is
 * inclusive, like torch.clamp's backward), else 0.  A null dy[i] skips member i (its dx[i] is not written); one launch. */
size_t movae_vgg_prep_ws_bytes(int g);
int movae_vgg_prep_fwd(int g, const float* const* x, float* const* y, int* flags, size_t n, void* ws, size_t ws_bytes,
                       movae_stream_t stream);
int movae_vgg_prep_bwd(int g, const float* const* dy, const float* const* x, const int* flags, float* const* dx, size_t n,
                       movae_stream_t stream);
/* 2x2 / stride-2 / floor-mode max-pool, NHWC fp32, c % 4 == 0, 16-byte aligned tensors: x [n][h][w][c] -> y [n][h/2][w/2][c]; an odd h
 * or w drops the last row / column.  The backward writes EVERY element of dx (zeros in a dropped row / column; no memset, no
 * atomics): dy goes to the first element of the window in the order (0,0), (0,1), (1,0), (1,1) that equals y, the others get 0. */
int movae_maxpool2x2_fwd(const float* x, float* y, int n, int h, int w, int c, movae_stream_t stream);
int movae_maxpool2x2_bwd(const float* dy, const float* x, const float* y, float* dx, int n, int h, int w, int c, movae_stream_t stream);

/* ---- the feature distance of LPIPS (csrc/lpips.hip; utils/metrics.py:290-357 lpips) -------------------------------------------------
 * movae_lpips_layer: f1, f2 contiguous fp32 NHWC [n][h][w][c], c % 4 == 0 (at most 1024), 16-byte aligned.  Per pixel
 * sum_c (f1 / max(||f1||_2, 1e-12) - f2 / max(||f2||_2, 1e-12))^2 (F.normalize's rule: an all-zero pixel normalises to zeros), formed
 * directly from the two normalised values -- identical operands give exactly 0.  Every element is read once; the arithmetic is fp64.
 * partials (device, movae_lpips_ws_bytes(n, h, w, c) bytes, 8-byte aligned, plain scratch: carve it from a workspace BEHIND its
 * 4096-byte header) receives, per image, the blocks' sums over their pixels times `scale` (a weight on the layer; 1 for the
 * reference's plain mean).  A block never straddles two images.  One launch, no atomics, no memset.
 * movae_lpips_finalize: one launch over the partials of `layers` (1..8) such calls with the same n (h, w, c: HOST arrays of the layers'
 * geometry; partials: HOST array of the device pointers): per image the mean over the layers of (sum of the layer's partials) / (h w),
 * out (device float[1 + n]) = [mean over the images, image 0, ..., image n - 1].  Fixed summation order: bit-identical between runs. */
size_t movae_lpips_ws_bytes(int n, int h, int w, int c);
int movae_lpips_layer(const float* f1, const float* f2, int n, int h, int w, int c, float scale, double* partials,
                      size_t partials_bytes, movae_stream_t stream);
int movae_lpips_finalize(int layers, const double* const* partials, const int* h, const int* w, const int* c, int n, float* out,
                         movae_stream_t stream);

/* ---- batches from a device-resident uint8 image set (csrc/data.hip; the reference's RandomHorizontalFlip -> ToTensor -> Normalize) ----
 * store: device uint8 [n][h][w][c], c in {1, 3}.  idx: device int[b], row numbers into store (the caller has range-checked them).
 * lut: device float[c][256], the per-channel value of every byte.  out: device fp32 NHWC [b][h][w][c], 16-byte aligned.
 * out[j][y][x][ch] = lut[ch][store[idx[j]][y][x'][ch]] with x' = x, or w - 1 - x where row idx[j] is flipped (channel order unchanged).
 * With flip != 0, row i = idx[j] is flipped iff bit 31 of word 0 of Philox4x32-10 with counter (i low word, i high word, epoch low word,
 * epoch high word) and key (seed low word, seed high word) is set: a function of (seed, epoch, i) alone.  Offsets into store are 64-bit.
 * One launch, no atomics, no workspace; capturable.  Refused (MOVAE_EINVAL, nothing launched): a null pointer, b, h or w <= 0, c not in
 * {1, 3}, a misaligned out. */
int movae_batch_u8(const uint8_t* store, const int* idx, int b, int h, int w, int c, const float* lut, int flip,
                   unsigned long long seed, unsigned long long epoch, float* out, movae_stream_t stream);

/* The device step of a STREAMED batch (data.StreamedBatchLoader: a set that stays in host memory).  stage: device uint8 [b][h][w][c],
 * the batch's images already in batch order (gathered on the host, copied up).  ids: device int[b], the dataset index of every row.
 * out[j][y][x][ch] = lut[ch][stage[j][y][x'][ch]], x' mirrored iff row ids[j] is flipped under (seed, epoch) by the rule above:
 * movae_batch_u8 with the source row (j) and the flip key (ids[j]) separated, so stage = store[ids] gives movae_batch_u8's bits.
 * The same kernel body, paths (w % 4 == 0 and a 4-byte-aligned stage: 4 pixels per thread), checks and refusals. */
int movae_batch_u8_staged(const uint8_t* stage, const int* ids, int b, int h, int w, int c, const float* lut, int flip,
                          unsigned long long seed, unsigned long long epoch, float* out, movae_stream_t stream);

/* ---- batches from a device-resident RAGGED uint8 image set (csrc/data.hip; the reference's RandomResizedCrop(BICUBIC) ->
 * RandomHorizontalFlip -> ToTensor -> Normalize on PIL images) ----
 * blob: device uint8, the images back to back in HWC order, each starting at ANY byte.  offsets: device int64[n], the byte offset of
 * every image (64-bit).  dims: device int[n][2] = (h, w).  boxes: device int[n][4] = (top, left, bh, bw), the crop of every image,
 * inside it.  idx: device int[b], row numbers (the caller has range-checked rows and boxes).  lut: device float[c][256].
 * out: device fp32 NHWC [b][s][s][c], 16-byte aligned.  out[j] = lut[ch][R], R = PIL's crop(box).resize((s, s), BICUBIC) of image
 * idx[j] bit for bit: per axis a table of 22-bit fixed-point weights computed in fp64 (Keys' cubic a = -0.5 at
 * (tap - center + 0.5) * (1 / filterscale), filterscale = max(1, crop side / s), taps clamped at the edges of the CROP), the
 * horizontal pass rounded to uint8 before the vertical one, int32 accumulation.  With flip != 0 the output columns of image i are
 * mirrored iff the Philox bit of movae_batch_u8 for (seed, epoch, i) is set.  kmax: the caller's bound on taps per output sample,
 * 2 * ceil(2 * max(1, largest crop side / s)) + 1; a crop side may be at most 8 s (kmax 33).  The kernel cannot see a broken
 * promise: a crop side over 8 s, or a kmax below that bound, stays inside its buffers but gives UNDEFINED pixels, not an error.
 * One launch, a block per 32 x 32 output tile, 46.6 KB static LDS, no atomics, no workspace; capturable.
 * Refused (MOVAE_EINVAL, nothing launched): a null pointer, b or s <= 0, c not in {1, 3}, kmax even or outside 5 .. 33, a misaligned
 * out. */
int movae_batch_rrc_u8(const uint8_t* blob, const long long* offsets, const int* dims, const int* boxes, const int* idx, int b, int s, int c,
                       int kmax, const float* lut, int flip, unsigned long long seed, unsigned long long epoch, float* out,
                       movae_stream_t stream);

/* The table routine of movae_batch_rrc_u8 alone (a test entry): for each of n input sizes (device int[n]) and each of out_size output
 * samples, k (device int[n][out_size][kmax]) = the fixed-point weights, zero past the last tap, and bounds (device
 * int[n][out_size][2]) = (first tap, taps); taps are cut at kmax (odd, >= 5; no upper limit here: nothing is staged in LDS). */
int movae_resample_coeffs(const int* in_sizes, int n, int out_size, int kmax, int* k, int* bounds, movae_stream_t stream);

/* ---- batches of VQ code grids from device-resident stores (csrc/prior.hip; prior.DeviceCodeLoader) -----------------------------------
 * store_top: device [n][len_top], store_bottom: device [n][len_bottom] or NULL (one level only); both int16 (wide == 0) or both int32
 * (wide == 1).  idx: device int[b], row numbers into the stores.  out_top: device int64 [b][len_top]; out_bottom: int64 [b][len_bottom],
 * NULL exactly when store_bottom is.  out_x[j][:] = (int64) store_x[idx[j]][:], both levels in ONE launch.  A level whose row length
 * is a multiple of 4 and whose bases are aligned (store: 4 elements, out: 16 bytes) moves 4 codes per load and two 16-byte stores; any
 * other length goes code by code (lengths such as 15 work).  The caller range-checks idx; the kernel clamps a row number into
 * [0, n - 1] all the same, so it never reads outside a store.  Offsets are 64-bit.  No atomics, no workspace; capturable.  Refused
 * (MOVAE_EINVAL, nothing launched): a null store_top / idx / out_top, a second store without its output or the reverse, wide not in
 * {0, 1}, n, b or a row length <= 0, a pointer not aligned to its element. */
int movae_codes_batch(const void* store_top, const void* store_bottom, int wide, int n, int len_top, int len_bottom, const int* idx, int b,
                      int64_t* out_top, int64_t* out_bottom, movae_stream_t stream);

/* ---- forward-only inference kernels of the Inception-v3 feature stack behind rFID (csrc/inception.hip; the reference's
 * utils/metrics.py:360-450 InceptionV3, :513-615 calculate_fid) ------------------------------------------------------------------------
 * All tensors fp32; activations NHWC; no workspace, no atomics, one launch each, bit-identical from run to run; capturable.
 *
 * movae_infer_conv2d: y[n][ho][wo][coff + o] = max(0, scale[o] * sum_{kh,kw,c} x[n][ho*stride - pad_h + kh][wo*stride - pad_w + kw][c]
 * * w[o][kh][kw][c] + shift[o]) with ho = (h + 2 pad_h - kh) / stride + 1 (likewise wo), zero padding.  x [n][h][w][ci] contiguous,
 * w [co][kh][kw][ci] contiguous, scale / shift [co] (an eval-mode BatchNorm folded by the caller; the ReLU is always applied).  y is a
 * buffer of `ldy` channels per pixel ([n][ho][wo][ldy]); the result goes to channels coff .. coff + co - 1 and no other element of y
 * is written (a branch writes its slice of a concat buffer).  An implicit GEMM (M = n ho wo, N = co, K = kh kw ci) on the exact-fp32
 * MFMA: every product is rounded once and summed in k order.  Any ci, co >= 1; 16-byte loads where ci % 4 == 0 and x, w are 16-byte
 * aligned.  Refused (MOVAE_EINVAL, nothing launched): a null pointer, a dimension <= 0, kh or kw above 7, a pad >= its kernel side,
 * an empty output, ldy < coff + co or coff < 0, n ho wo or an operand's element count at or above 2^31.
 *
 * movae_infer_pool3x3: a 3x3 window over x [n][h][w][c] into channels coff .. coff + c - 1 of y [n][ho][wo][ldy].  mode 0: maximum,
 * stride 2, no padding (ho = (h - 3) / 2 + 1; h, w >= 3).  mode 1: average, stride 1, padding 1, the sum of the in-bounds taps divided
 * by 9 everywhere (count_include_pad), summed in fp64 and rounded once (ho = h).
 * movae_infer_global_mean: y[n][c] = mean over the hw pixels of x [n][hw][c], summed in fp64 in pixel order, rounded once.
 *
 * movae_inception_prep: x [n][3][h][w] contiguous NCHW (h, w <= 299) -> y [n][299][299][3] NHWC: v = clamp(0.5 x + 0.5, 0, 1) ALWAYS
 * (calculate_fid's `denormalize`, applied to [0, 1] data too); the shorter side resized to 299 (the other to floor(299 * long / short))
 * with the antialiased bicubic of F.interpolate -- for an enlargement the separable Keys kernel, a = -0.5, at (tap - scale * (i + 0.5)
 * + 0.5), taps cut at the border and the weights renormalised, no clamp afterwards; the 299 x 299 centre crop (offset round-half-even
 * of (side - 299) / 2); then (v - mean_c) / std_c with the ImageNet mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225).  Weights
 * and sums are fp64, the result is rounded once.  Refused: a null pointer, n, h or w <= 0, a side above 299 (that needs a true
 * antialiasing filter). */
int movae_infer_conv2d(const float* x, const float* w, const float* scale, const float* shift, float* y, int n, int h, int wd, int ci,
                       int co, int kh, int kw, int stride, int pad_h, int pad_w, int ldy, int coff, movae_stream_t stream);
int movae_infer_pool3x3(const float* x, float* y, int n, int h, int w, int c, int mode, int ldy, int coff, movae_stream_t stream);
int movae_infer_global_mean(const float* x, float* y, int n, int hw, int c, movae_stream_t stream);
int movae_inception_prep(const float* x, float* y, int n, int h, int w, movae_stream_t stream);

/* ---- the generative evaluation: gFID / Inception Score / KID / precision and recall (csrc/gen_metrics.hip, and the second filter of
 * the input pipeline in csrc/inception.hip; the reference's main.py:695-887, utils/metrics.py:682-736, :835-914) ------------------------
 * Forward only, fp32 operands, no atomics, bit-identical from run to run; capturable.
 *
 * movae_inception_prep_filter: movae_inception_prep with the resize filter named.  MOVAE_RESIZE_BICUBIC is movae_inception_prep itself,
 * bit for bit.  MOVAE_RESIZE_BILINEAR is calculate_inception_score's TF.resize(batch, 299, antialias=True) -- the default filter: the
 * antialiased bilinear of F.interpolate, for an enlargement the triangle 1 - |t| of support 1 at (tap - scale * (i + 0.5) + 0.5), at
 * most 3 taps per axis, cut at the border and renormalised; everything else (0.5 x + 0.5, clamp, centre crop, ImageNet normalisation,
 * NHWC output, fp64 weights and sums) as in movae_inception_prep.  Refused as there, and any other filter value.
 *
 * movae_linear_softmax: probs[i][c] = softmax_c(sum_k feat[i][k] * weight[c][k] + bias[c]), feat [n][D], weight [C][D], bias [C],
 * probs [n][C], all contiguous; fp32 throughout, the row maximum subtracted before expf.  Four rows per block are staged in LDS once;
 * weight rows are read with 16-byte loads where D % 4 == 0 and weight is 16-byte aligned.  Refused: a null pointer, a dimension <= 0,
 * 4 * (D + C) floats above 64 KB (D = 2048 with C = 1000 takes 48 KB).
 *
 * movae_inception_score: utils/metrics.py:895-914 on probs [n][C]: split i is rows i * (n / splits) .. (i + 1) * (n / splits) - 1
 * (integer division: the remainder rows belong to no split); with p = clip(probs, 1e-16, 1) and p_y = clip(mean over the split's rows
 * of p, 1e-16, 1), scores[i] = exp(mean over the rows of sum_c p (log p - log p_y)).  One block per split; every sum, logarithm and
 * the exponential in fp64.  scores [splits] fp64 on the device; mean and standard deviation over the splits are the caller's.
 * Refused: n / splits == 0 (every split empty -- the caller reports NaN), C above 7000, a misaligned scores.
 *
 * movae_kid_subsets: utils/metrics.py:682-709 for S subsets at once.  real [nr][D], fake [nf][D]; idx_real / idx_fake [S][m] int32 row
 * numbers (the caller draws them).  Per subset, with r / f the gathered rows: K(x, y) = (gamma x.y + 1)^degree, mmd2[s] =
 * max(0, sum_{i != j} K(r_i, r_j) / (m (m - 1)) + sum_{i != j} K(f_i, f_j) / (m (m - 1)) - 2 sum_{i, j} K(r_i, f_j) / m^2).  Dots,
 * powers and sums in fp64 (operands widened before the product).  One block per subset.  An index outside its set contributes a
 * zero row (the caller validates the indices).  Refused: m < 2, m above 240 or above a set's size, degree outside 1 .. 16.
 *
 * movae_knn_rows: for every row i of a [na][D] its k smallest squared Euclidean distances to the rows of b [nb][D], ascending, into
 * dist2 [na][k], clamped below at 0, and the row number of the nearest into idx [na]; exclude_diag = 1 leaves j == i out (a against
 * itself: the reference's fill_diagonal(inf)).  Gram form |a_i|^2 + |b_j|^2 - 2 a_i.b_j: the norms are summed in fp64 and rounded
 * once into norms [na + nb] (scratch of the caller), the dots run on the exact-fp32 MFMA, k ascending.  No na x nb matrix is formed:
 * a block owns `tile` rows (64 or 128; 0: chosen here) for all of b and keeps the candidates in registers.  Equal distances: the
 * smaller row number of b is reported.  Refused: k outside 1 .. 8, fewer than k candidates per row, any other tile. */
#define MOVAE_RESIZE_BICUBIC 0
#define MOVAE_RESIZE_BILINEAR 1
int movae_inception_prep_filter(const float* x, float* y, int n, int h, int w, int filter, movae_stream_t stream);
int movae_linear_softmax(const float* feat, const float* weight, const float* bias, float* probs, int n, int C, int D, movae_stream_t stream);
int movae_inception_score(const float* probs, int n, int C, int splits, double* scores, movae_stream_t stream);
int movae_kid_subsets(const float* real, const float* fake, const int* idx_real, const int* idx_fake, int nr, int nf, int S, int m, int D,
                      double gamma, int degree, double* mmd2, movae_stream_t stream);
int movae_knn_rows(const float* a, const float* b, int na, int nb, int D, int k, int exclude_diag, int tile, float* norms, float* dist2,
                   int* idx, movae_stream_t stream);

/* ---- image grids as bytes (csrc/visual.hip; the figures of main.py:511-656) -------------------------------------------------------
 * A float image batch x, logical [n][c][h][w] given by pointer and four element strides (NCHW, channels_last and sliced views alike, no
 * copy), becomes the finished picture out [H][W][3] uint8: torchvision's make_grid followed by save_image's quantisation.
 *   xmaps = min(nrow, n), ymaps = ceil(n / xmaps); H = ymaps * (h + padding) + padding, W = xmaps * (w + padding) + padding; image k has
 *   its top-left corner at ((k / xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding); every byte outside an image,
 *   whole cells beyond n included, is pad_value, quantised and never normalised; n == 1 gives the image itself (H = h, W = w, no
 *   border); c == 1 is written to all three channels.
 * Per pixel, in fp32 and in this order: mode RAW: v = x; mode RANGE: v = (min(max(x, lo), hi) - lo) / max(hi - lo, 1e-5f) with the
 * given lo, hi; mode MINMAX: the same with lo, hi the minimum and maximum over the whole batch, found on the device (lo, hi ignored);
 * then byte = (uint8) min(max(v * 255 + 0.5f, 0), 255), truncating; a NaN pixel gives 0.  The division is an IEEE division.
 * Mode MINMAX is two launches (per-block partials into ws, folded by every block of the second launch) and needs
 * ws >= movae_image_grid_ws_bytes bytes (the 4096-byte header included; only the scratch behind it is used); the other modes are one
 * launch and ignore ws.  No atomics, no host read; capturable.  Refused (MOVAE_EINVAL, nothing launched): a null x or out; n, h, w or
 * nrow <= 0; padding < 0; c not in {1, 3}; a mode outside 0 .. 2; hi < lo in mode RANGE; in mode MINMAX a null or too small workspace. */
#define MOVAE_GRID_RAW 0
#define MOVAE_GRID_RANGE 1
#define MOVAE_GRID_MINMAX 2
size_t movae_image_grid_ws_bytes(int n, int c, int h, int w);
int movae_image_grid_u8(const float* x, long long sn, long long sc, long long sh, long long sw, int n, int c, int h, int w, int nrow,
                        int padding, float pad_value, int mode, float lo, float hi, uint8_t* out, void* ws, size_t ws_bytes,
                        movae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOVAE_H */
