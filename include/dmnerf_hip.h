/*
 * dmnerf_hip.h -- C ABI of libdmnerf_hip.so: the MI355X (gfx950) implementation of the
 * DM-NeRF ray-rendering hot path.
 *
 * The reference (vLAR-group/DM-NeRF) has no FFI/plugin layer: its boundary is a set of Python
 * callables.  Each entry point below replaces the ATen op sequence of
 * one of them and cites it (paths relative to the reference checkout).  The Python mirror of
 * those callables (dm_nerf_amd/networks/) binds these symbols with ctypes; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer marked d_ is a DEVICE pointer to contiguous row-major float32 (int64 where
 *     stated); h_ pointers are HOST pointers.  No torch / ATen types cross this boundary.
 *   - the caller owns all memory; the library never allocates, frees or synchronises on the hot
 *     path, and launches only on the `stream` it is given (hipStream_t passed as void*),
 *     so every call is graph-capturable.
 *   - return 0 on success; negative on error (DMNERF_E_*), message via dmnerf_last_error().
 *   - sizes are validated first; an EMPTY batch (N == 0 rays / M == 0 rows) is legal, returns 0 without launching
 *     and without looking at the data pointers (an empty tensor's pointer is null).
 *   - N rays, S samples per ray, C = ins_num + 1 object logits, raw row = [r g b sigma | C logits].
 */
#ifndef DMNERF_HIP_H
#define DMNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMNERF_ABI_VERSION 8

#define DMNERF_OK 0
#define DMNERF_E_ARG (-1)     /* bad size / null pointer / unsupported shape */
#define DMNERF_E_LAUNCH (-2)  /* hipGetLastError() after launch */
#define DMNERF_E_NODEV (-3)   /* no HIP device visible */

#define DMNERF_POS_CH 63   /* 3 + 2*10*3, get_embedder(multires=10)  networks/dm_nerf.py:41-55 */
#define DMNERF_DIR_CH 27   /* 3 + 2*4*3,  get_embedder(multires_views=4) */
#define DMNERF_W 256       /* netwidth  (config.py:33 default; every shipped config) */
#define DMNERF_D 8         /* netdepth  (config.py:31 default), skips=[4] (config.py:133) */
#define DMNERF_MAX_LOGITS 128 /* C = ins_num+1 <= 128 (Replica room_0: 94) */
#define DMNERF_MAX_TRAIN_SAMPLES 1048576LL /* samples per training launch: 32-bit byte offsets into a 256-row tensor */

int dmnerf_abi_version(void);
const char* dmnerf_last_error(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int dmnerf_device_count(void);

/* ---- weights: reference state_dict -> kernel layout -------------------------------------
 * Flat parameter order = DM_NeRF.__init__ / state_dict order (networks/dm_nerf.py:59-78):
 *   mlps.0..7, rgb_feature_linear, ins_feature_linear, rgb_feature_linears.0,
 *   ins_feature_linears.0, density_linear, ins_linear, rgb_linear; each as weight[out,in]
 *   row-major followed by bias[out].
 * The kernel "blob" holds the same numbers permuted into MFMA A-operand order (DESIGN.md
 * section 3), zero padded.  blob[i] = idx[i] >= 0 ? flat[idx[i]] : 0.
 */
int64_t dmnerf_param_count(int ins_num);                    /* 696338 for ins_num=13 */
int64_t dmnerf_blob_floats(int ins_num);
int dmnerf_build_pack_index(int ins_num, int32_t* h_idx, int64_t n_idx);   /* host only, no GPU */
int dmnerf_pack_weights(const float* d_flat, const int32_t* d_idx, float* d_blob,
                        int64_t n_blob, void* stream);

/* ---- helpers.py --------------------------------------------------------------------------
 * get_rays_k (networks/helpers.py:50-61) for image rows [row0, row0+nrows):
 *   dirs = [(i-K02)/K00, (j-K12)/K11, K22]; rays_d = R dirs; rays_o = c2w[:3,3].
 *   h_intr = {K00, K11, K02, K12, K22} already rounded to float32 (what ATen does with the
 *   numpy float64 scalars); h_c2w = first 3 rows of c2w, row-major [3][4].
 *   d_rays_o / d_rays_d: [nrows*W, 3].                                                     */
int dmnerf_raygen(int H, int W, const float* h_intr, const float* h_c2w, int row0, int nrows,
                  float* d_rays_o, float* d_rays_d, void* stream);

/* Rays of selected pixels only: what get_select_full (networks/helpers.py:99-111) gathers out of a
 * full-frame get_rays_k.  d_idx: int64 flat pixel indices k = row*W + col; outputs [n,3].           */
int dmnerf_raygen_select(int H, int W, const float* h_intr, const float* h_c2w, const int64_t* d_idx,
                         int64_t n, float* d_rays_o, float* d_rays_d, void* stream);

/* z_val_sample (networks/helpers.py:114-119): z[n,s] = near + t[s]*(far-near); d_t = linspace(0,1,S). */
int dmnerf_z_val_sample(const float* d_t, float near_, float far_, int64_t N, int S, float* d_z,
                        void* stream);

/* stratified jitter (networks/render.py:42-47): mids/upper/lower, lower + (upper-lower)*t_rand. */
int dmnerf_stratify(const float* d_z_in, const float* d_t_rand, int64_t N, int S, float* d_z_out,
                    void* stream);

/* sample_pdf (networks/helpers.py:123-155).  bins [N,nb], weights [N,nb-1], u [N,n_samples]
 * (u_row_stride = n_samples) or one shared row (u_row_stride = 0, the det=True linspace).
 * Optional outputs (may be NULL): d_cdf [N,nb] float32, d_inds [N,n_samples] int64.          */
int dmnerf_sample_pdf(const float* d_bins, const float* d_weights, const float* d_u,
                      int64_t u_row_stride, int64_t N, int nb, int n_samples, float* d_samples,
                      float* d_cdf, int64_t* d_inds, void* stream);

/* stage-isolated inverse-CDF step (helpers.py:139-153): same (cdf,u) => same inds, samples. */
int dmnerf_sample_from_cdf(const float* d_bins, const float* d_cdf, const float* d_u,
                           int64_t u_row_stride, int64_t N, int nb, int n_samples,
                           float* d_samples, int64_t* d_inds, void* stream);

/* hierarchical resample + merge (networks/render.py:66-70):
 *   z_mid, sample_pdf(z_mid, weights[...,1:-1], n_imp, u), sort(cat(z_coarse, z_samples)).
 * d_z_samples may be NULL.  d_z_fine [N, S + n_imp].                                         */
int dmnerf_importance_resample(const float* d_z_coarse, const float* d_weights_coarse,
                               const float* d_u, int64_t u_row_stride, int64_t N, int S, int n_imp,
                               float* d_z_fine, float* d_z_samples, void* stream);

/* ---- dm_nerf.py ---------------------------------------------------------------------------
 * Embedder.embed (networks/dm_nerf.py:37-38): x [M,3] -> [M, 3+6L], L frequencies 2^0..2^(L-1). */
int dmnerf_embed(const float* d_x, int64_t M, int L, float* d_out, void* stream);

/* DM_NeRF.forward (networks/dm_nerf.py:80-106) on pre-embedded rows x [M, 63+27] -> raw [M, 4+C]. */
int dmnerf_mlp_fwd_embedded(const float* d_blob, int ins_num, const float* d_x, int64_t M,
                            float* d_raw, void* stream);

/* Fused points + positional encoding + DM_NeRF.forward (networks/render.py:49-61 / :71-83):
 *   pts = o + d*z; embed(pts) | embed(d/|d|); MLP.  rays_o/rays_d [N,3], z [N,S] -> raw [N,S,4+C]. */
int dmnerf_mlp_fwd_rays(const float* d_blob, int ins_num, const float* d_rays_o,
                        const float* d_rays_d, const float* d_z, int64_t N, int S, float* d_raw,
                        void* stream);

/* ---- render.py ----------------------------------------------------------------------------
 * render_train (networks/render.py:6-28): raw [N,S,4+C], z [N,S], rays_d [N,3] ->
 *   rgb_map [N,3], weights [N,S], depth_map [N], ins_map [N,C-1] (sigmoid after the sum, last
 *   channel dropped).                                                                       */
int dmnerf_composite_fwd(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t N,
                         int S, int C, float* d_rgb_map, float* d_weights, float* d_depth_map,
                         float* d_ins_map, void* stream);

/* ---- training (autograd of the two entry points above) ------------------------------------
 * Backward of render_train: given dL/d{rgb_map [N,3], ins_map [N,C-1], depth_map [N] (nullable),
 * weights [N,S] (nullable)} -> dL/draw [N,S,4+C] (every element written).  d_ins_map = the forward's
 * ins_map.  Honours weights.detach() on the ins path (render.py:22-23).                        */
int dmnerf_composite_bwd(const float* d_raw, const float* d_z, const float* d_rays_d,
                         const float* d_ins_map, const float* d_g_rgb, const float* d_g_ins,
                         const float* d_g_depth, const float* d_g_weights, int64_t N, int S, int C,
                         float* d_grad_raw, void* stream);

/* Training forward of dmnerf_mlp_fwd_rays: additionally saves every layer input / relu output into
 * d_save (dmnerf_train_save_floats(M) floats, M = N*S, Mp = M rounded up to 32).  Each tensor with R
 * rows is stored block-major: addr(sample m, row) = ((m/32 * R + row) * 32 + m%32); tensors in order:
 *   embed(pts) R=63 | embed(dirs) R=27 | h_0..h_7 8 x R=256 | rgb hidden 128 | ins hidden 128,
 *   each R*Mp floats, then the 1-bit ReLU masks.  (rgb_feature / ins_feature are not saved: they have no
 *   activation, dm_nerf.py:89,96, and the backward re-associates around them -- see dmnerf_head_product.)
 * In the 256- and 128-row tensors (not the two encodings) memory row rho holds feature
 * (rho & ~7) | ((rho & 7) >> 1) | ((rho & 1) << 2), i.e. inside each group of 8 features the rows are
 * 0,4,1,5,2,6,3,7 (the kernels' TID-addressed stores; only dmnerf_mlp_bwd_* read these buffers, and the
 * gradients they return are in the reference's parameter order).   M <= DMNERF_MAX_TRAIN_SAMPLES.       */
int64_t dmnerf_train_save_floats(int64_t M);
int dmnerf_mlp_fwd_rays_train(const float* d_blob, int ins_num, const float* d_rays_o,
                              const float* d_rays_d, const float* d_z, int64_t N, int S,
                              float* d_raw, float* d_save, void* stream);
/* OPT-IN: the training forward on the fused-heads blob (dmnerf_fuse_heads + dmnerf_build_pack_index_fused): same outputs
 * and the same d_save contents as dmnerf_mlp_fwd_rays_train up to f32 re-association of the two feature linears. */
int dmnerf_mlp_fwd_rays_train_fused(const float* d_blob_fused, int ins_num, const float* d_rays_o,
                                    const float* d_rays_d, const float* d_z, int64_t N, int S,
                                    float* d_raw, float* d_save, void* stream);
/* OPT-IN: the training forward on the split-bf16 MFMA path (blob of dmnerf_pack_split): f32-class values (not the bitwise
 * f32 chain), the same f32 d_save contents for the same backward. */
int dmnerf_mlp_fwd_rays_train_split(const float* d_blob_split, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                    const float* d_z, int64_t N, int S, float* d_raw, float* d_save, void* stream);
/* DM_NeRF.forward on pre-embedded rows (networks/dm_nerf.py:80-106 called directly, as mesh / third-party code does) in
 * training mode: d_raw as dmnerf_mlp_fwd_embedded, plus the activation workspace d_save (dmnerf_train_save_floats(M))
 * that dmnerf_mlp_bwd_data / dmnerf_mlp_bwd_weights consume.  Parameter gradients only: the kernels produce no
 * gradient for the embedded rows themselves. */
int dmnerf_mlp_fwd_embedded_train(const float* d_blob, int ins_num, const float* d_x, int64_t M, float* d_raw,
                                  float* d_save, void* stream);

/* Backward blob (W^T as MFMA A operand) and the data-gradient pass: dL/draw [M,4+C] + d_save ->
 * d_dsave (same layout as d_save): dy of mlps.0..7 in the h rows, d(rgb hidden pre-act), d(ins hidden pre-act).
 * Weight gradients are dW = dy . x^T over M.
 * d_graw_t (nullable): receives dL/draw in block-major form [block][4+C][32] (zero padding columns),
 * the third operand of dmnerf_mlp_bwd_weights.
 * Gradient barriers: h.detach() on the ins branch (dm_nerf.py:95); none to the encodings.
 * The two feature linears carry no activation, so their gradients are never materialised: with
 * A = rgb_feature_linears.0.weight[:, :256] and F = A . rgb_feature_linear.weight [128,256], d h_7 = F^T dg1 is ONE
 * GEMM (instead of 128 -> 256 -> 256).  dmnerf_head_product forms F (f32 fmaf chain, k ascending) from the flat
 * parameter vector; the W^T blob gathers from [flat parameters | F]: the index of dmnerf_build_pack_index_t addresses
 * dmnerf_param_count(ins_num) + 32768 source floats.                                             */
int64_t dmnerf_blob_t_floats(int ins_num);
int dmnerf_build_pack_index_t(int ins_num, int32_t* h_idx, int64_t n_idx);
int dmnerf_head_product(const float* d_params_flat, int ins_num, float* d_F, void* stream);
/* Inference-only head fusion (the blobs of dmnerf_mlp_fwd_rays_fused / _split): d_flat_fused = the flat parameter vector
 * with the two hidden layers replaced by hidden . feature (products accumulated in float64, rounded once); it must not
 * alias d_params_flat.  Pack it with the index of dmnerf_build_pack_index_fused.                                    */
int dmnerf_fuse_heads(const float* d_params_flat, int ins_num, float* d_flat_fused, void* stream);
int dmnerf_mlp_bwd_data(const float* d_blob, const float* d_blob_t, int ins_num, const float* d_save,
                        const float* d_graw, int64_t M, float* d_dsave, float* d_graw_t, void* stream);

/* Weight / bias gradients dW = dy . x^T over the batch (split-K f32 MFMA, deterministic 2-stage sum).
 * The plan (which workgroup does which job slices) depends only on (ins_num, M, max_wgs): build it once
 * on the host, upload the two tables, reuse every step.  n_jobs = the number of WORKGROUPS (<= max_wgs; the grid of the launch,
 * all filled to the same modelled time); the job table (n_job_bytes) holds one leader item per workgroup followed by the further
 * items some of them continue with (a job's last slice and the next job's first), each item with its own partial tile.  d_graw_t = dL/draw in the same block-major
 * form, R = 4+C rows, zero in the padding columns.  d_grad_flat: dmnerf_param_count(ins_num) floats in the
 * flat parameter order above.  d_part: workspace of `part_floats` floats.
 * The gradients of rgb_feature_linear, ins_feature_linear and of the two hidden layers that consume them are formed from
 * G = dg1 . h_7^T, Q = dg2 . h_7^T and the weights themselves (d_params_flat: the flat parameter vector the forward
 * used), e.g. d rgb_feature_linear.weight = A^T G: exact algebra, f32 re-association (csrc/heads.hip).        */
int dmnerf_wgrad_plan_sizes(int ins_num, int64_t M, int max_wgs, int64_t* n_job_bytes,
                            int64_t* n_out_bytes, int64_t* part_floats, int* n_jobs, int* n_outs);
int dmnerf_wgrad_plan(int ins_num, int64_t M, int max_wgs, void* h_jobs, int64_t job_bytes,
                      void* h_outs, int64_t out_bytes);
int dmnerf_mlp_bwd_weights(const float* d_save, const float* d_dsave, const float* d_graw_t, int64_t M,
                           const void* d_jobs, int n_jobs, const void* d_outs, int n_outs,
                           const float* d_params_flat, int ins_num, float* d_part, float* d_grad_flat, void* stream);
/* OPT-IN split-bf16 weight gradients (training with args.mfma_split; csrc/wgrad_split.hip) -- the parameter gradients of
 * networks/dm_nerf.py:80-106 that torch autograd forms in the reference's train loops (train_dmsr.py:62-64): the same tables, workspace and
 * second stage; both f32 operands are split on the fly into three bf16 planes and a product is six bf16 MFMAs accumulated
 * in f32 (f32-class, not the bitwise chain of dmnerf_mlp_bwd_weights).  The _split plan balances the slices for this
 * kernel's chunk times (its 256 x 256 jobs are HBM-bound); either plan is valid for either kernel.                  */
int dmnerf_wgrad_plan_sizes_split(int ins_num, int64_t M, int max_wgs, int64_t* n_job_bytes,
                                  int64_t* n_out_bytes, int64_t* part_floats, int* n_jobs, int* n_outs);
int dmnerf_wgrad_plan_split(int ins_num, int64_t M, int max_wgs, void* h_jobs, int64_t job_bytes,
                            void* h_outs, int64_t out_bytes);
int dmnerf_mlp_bwd_weights_split(const float* d_save, const float* d_dsave, const float* d_graw_t, int64_t M,
                                 const void* d_jobs, int n_jobs, const void* d_outs, int n_outs,
                                 const float* d_params_flat, int ins_num, float* d_part, float* d_grad_flat, void* stream);
/* Diagnostic: when d_ticks != NULL every workgroup of the following dmnerf_mlp_bwd_weights launches writes its
 * {start, end} 100 MHz wall-clock ticks to d_ticks[2*wg], d_ticks[2*wg+1] (n_jobs pairs); NULL turns it off.
 * Used by scripts/diag_wgrad.py to fit the split-K cost model. */
int dmnerf_wgrad_set_trace(int64_t* d_ticks);

/* ---- inference-only algebraic fusion (opt-in) -------------------------------------------
 * rgb_feature_linear and ins_feature_linear have no activation (dm_nerf.py:89,96), so for inference they can be
 * folded into the hidden layers that consume them: W' = W_hidden[:, :256] . W_feature, b' = W_hidden[:, :256] .
 * b_feature + b_hidden (the caller forms them, e.g. in float64, and writes them over the rgb_feature_linears.0 /
 * ins_feature_linears.0 slots of a copy of the flat parameter vector).  The fused blob has the same table and the
 * same stream without the two 256x256 stages (36 quarters instead of 44: -18.9 % MACs at ins_num 13).  Results
 * differ from the layer-by-layer evaluation by f32 re-association only (|d raw| ~ 1e-6), hence opt-in.           */
int64_t dmnerf_blob_fused_floats(int ins_num);
int dmnerf_build_pack_index_fused(int ins_num, int32_t* h_idx, int64_t n_idx);
int dmnerf_mlp_fwd_rays_fused(const float* d_blob_fused, int ins_num, const float* d_rays_o,
                              const float* d_rays_d, const float* d_z, int64_t N, int S,
                              float* d_raw, void* stream);

/* ---- opt-in split-bf16 ("bf16x3") inference (docs/EXPERIMENTS.md section 8) -----------------------------------------
 * The MLP on v_mfma_f32_32x32x16_bf16 with every f32 operand split by truncation into three bf16 planes
 * (x = hi + mid + lo exactly) and the six leading products accumulated in f32: the rounding class of an f32 GEMM
 * at 2.7x fewer MFMA cycles; not the bitwise fmaf chain of dmnerf_mlp_fwd_rays, hence opt-in.  The blob is
 * [the fused blob's 4096-float table | split stream]: dmnerf_build_pack_index_split gives one int32 per bf16
 * element of the stream (source parameter | plane << 28, -1 = zero) over the FUSED flat parameter vector
 * (see above), dmnerf_pack_split writes the stream words (n_words = dmnerf_blob_split_words - 4096).          */
int64_t dmnerf_blob_split_words(int ins_num);
int dmnerf_build_pack_index_split(int ins_num, int32_t* h_idx, int64_t n_idx);
int dmnerf_pack_split(const float* d_flat, const int32_t* d_idx, float* d_stream_words, int64_t n_words, void* stream);
/* OPT-IN split-bf16 data-gradient kernel (training with args.mfma_split): the blob is [the first 1024 floats of the W^T
 * blob (dmnerf_build_pack_index_t: the two VALU heads' table) | W^T split stream]; the index (two int32 per stream word,
 * as above) addresses [flat parameters | F] like dmnerf_build_pack_index_t.  Reads and writes exactly what
 * dmnerf_mlp_bwd_data reads and writes (networks/dm_nerf.py:80-106 backward), f32-class, not its bitwise chain. */
int64_t dmnerf_blob_t_split_words(int ins_num);
int dmnerf_build_pack_index_t_split(int ins_num, int32_t* h_idx, int64_t n_idx);
int dmnerf_mlp_bwd_data_split(const float* d_blob_t_split, int ins_num, const float* d_save, const float* d_graw, int64_t M,
                              float* d_dsave, float* d_graw_t, void* stream);
int dmnerf_mlp_fwd_rays_split(const float* d_blob_split, int ins_num, const float* d_rays_o, const float* d_rays_d,
                              const float* d_z, int64_t N, int S, float* d_raw, void* stream);

/* OPT-IN split-f16 ("f16x2") inference (args.mfma_split = "f16x2"): the same function as dmnerf_mlp_fwd_rays_fused
 * (networks/dm_nerf.py:80-106 with the two activation-free feature linears folded in) on v_mfma_f32_32x32x16_f16 with every f32
 * operand split into two f16 planes and THREE products per f32 product (csrc/mlp_f16_impl.h, split_f16.h): f32-class values
 * (|d raw| <= 1e-5 (1 + |raw|), like the f32 kernels; not their bitwise chain), half the MFMAs of the bf16x3 mode; activations
 * saturate at 65 504 (f16 range).  Blob: dmnerf_blob_f16_words 32-bit words = [4096-float bias table | stream of 16 KiB groups];
 * dmnerf_build_pack_index_f16 fills the table's float gather index (h_idx_tab[4096], for dmnerf_pack_weights) and the stream's
 * element index (h_idx_stream[(words - 4096) * 2]: source parameter | plane << 28, or -1), both addressing the FUSED flat
 * parameter vector (dmnerf_fuse_heads); dmnerf_pack_f16 writes the stream words (n_words = dmnerf_blob_f16_words - 4096). */
int64_t dmnerf_blob_f16_words(int ins_num);
int dmnerf_build_pack_index_f16(int ins_num, int32_t* h_idx_tab, int64_t n_tab, int32_t* h_idx_stream, int64_t n_stream);
int dmnerf_pack_f16(const float* d_flat, const int32_t* d_idx, float* d_stream_words, int64_t n_words, void* stream);
int dmnerf_mlp_fwd_rays_f16(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d,
                            const float* d_z, int64_t N, int S, float* d_raw, void* stream);

/* OPT-IN training forward on the split-f16 path (args.mfma_split = "f16x2" with grad enabled): dmnerf_mlp_fwd_rays_f16 plus
 * the f32 workspace d_save of dmnerf_mlp_fwd_rays_train (dmnerf_train_save_floats(N S) floats: pe, de, h_0..h_7, g1, g2 as
 * block-major rows + 1-bit ReLU masks), which every backward kernel of this library consumes. */
int dmnerf_mlp_fwd_rays_train_f16(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                  const float* d_z, int64_t N, int S, float* d_raw, float* d_save, void* stream);

/* OPT-IN split-f16 data-gradient kernel (training with args.mfma_split = "f16x2"): the blob is [the first 1024 floats of the
 * W^T blob (dmnerf_build_pack_index_t: the two VALU heads' table) | W^T stream of 16 KiB groups, two f16 planes]; the index (two
 * int32 per stream word: source | plane << 28) addresses [flat parameters | F] like dmnerf_build_pack_index_t; dmnerf_pack_f16
 * writes the stream.  Reads and writes exactly what dmnerf_mlp_bwd_data reads and writes (networks/dm_nerf.py:80-106 backward),
 * f32-class, not its bitwise chain.
 */
int64_t dmnerf_blob_t_f16_words(int ins_num);
int dmnerf_build_pack_index_t_f16(int ins_num, int32_t* h_idx, int64_t n_idx);
/* Gradient scaling.  f16 has 5 exponent bits and the data gradients of a real training step sit far below its normal range, so
 * the split-f16 backward runs on 2^s dL/draw (the whole backward is linear in it; s = 6 - ceil(log2 max|dL/draw|), exact) and
 * the weight-gradient reduction multiplies by 2^-s: dmnerf_grad_scale reduces max|d_graw[0..n)| and writes d_scale4 = {2^s,
 * 2^-s, scratch, scratch} (4 floats the caller zeroes ONCE; the kernel leaves the scratch words zero); d_scale = that buffer,
 * or null for s = 0.  With a scale, every row the kernel writes (d_dsave, d_graw_t) carries the factor 2^s. */
int dmnerf_grad_scale(const float* d_graw, int64_t n, float* d_scale4, void* stream);
int dmnerf_mlp_bwd_data_f16(const float* d_blob_t_f16, int ins_num, const float* d_save, const float* d_graw, int64_t M,
                            float* d_dsave, float* d_graw_t, const float* d_scale, void* stream);
/* OPT-IN split-f16 weight-gradient kernel: dmnerf_mlp_bwd_weights on the f16 MFMA (both operands split on the fly into two f16
 * planes, three products per f32 product).  The _f16 plan balances the slices for this kernel's chunk times (every job class is
 * HBM-bound); any of the three plans is valid for any of the three kernels.  The dy-side operands
 * (d_dsave, d_graw_t) carry the factor 2^s of dmnerf_grad_scale; the second stage multiplies every gradient by d_scale[1] = 2^-s
 * (d_scale null: 1). */
int dmnerf_wgrad_plan_sizes_f16(int ins_num, int64_t M, int max_wgs, int64_t* n_job_bytes,
                                int64_t* n_out_bytes, int64_t* part_floats, int* n_jobs, int* n_outs);
int dmnerf_wgrad_plan_f16(int ins_num, int64_t M, int max_wgs, void* h_jobs, int64_t job_bytes,
                          void* h_outs, int64_t out_bytes);
/* Run-time honesty of the f16x2 mode (opt-in diagnostic: DMNERF_CHECK_F16=1 / args.check_f16 in the Python mirror).  The
 * conversions saturate silently at 65 504; every converted operand is also a row of the f32 workspace the training forward saves
 * (gradients = 0) or the data-gradient kernel writes (gradients = 1, values carry the factor 2^s of dmnerf_grad_scale), so one
 * pass over the workspace of M samples finds them: ORs DMNERF_F16_ACT_SATURATED / DMNERF_F16_GRAD_SATURATED into the int32 at
 * d_flags (sticky: the caller zeroes it when it has read it) if any |x| >= 65 504 or non-finite.  No sync. */
#define DMNERF_F16_ACT_SATURATED 1
#define DMNERF_F16_GRAD_SATURATED 2
int dmnerf_f16x2_range_flags(const float* d_workspace, int64_t M, int gradients, int32_t* d_flags, void* stream);
int dmnerf_mlp_bwd_weights_f16(const float* d_save, const float* d_dsave, const float* d_graw_t, int64_t M,
                               const void* d_jobs, int n_jobs, const void* d_outs, int n_outs,
                               const float* d_params_flat, int ins_num, float* d_part, float* d_grad_flat,
                               const float* d_scale, void* stream);

/* ---- evaluator.py (the object-code loss, no host round trip) ---------------------------
 * ins_criterion (networks/evaluator.py:19-74): pred [N, ins_num] (rendered object codes in (0,1)), labels [N]
 * (int32, values 0..ins_num; other values are ignored) -> out4 = {ins_loss_sum, valid_ce, invalid_ce,
 * valid_siou}.  The cost matrices (:57-69), the label -> channel assignment that the reference delegates to
 * scipy.optimize.linear_sum_assignment (:43-54; same optimum, solved on the device by shortest augmenting
 * paths) and the three means (:28-37) run on `stream`; d_work (dmnerf_ins_criterion_work_bytes) carries the
 * assignment to _bwd, which writes d loss / d pred [N, ins_num] for upstream gradients gout4 of the four outputs.
 * ins_num <= 128; at most ins_num distinct labels may occur (the reference's own limit, :21-26).
 * Where the reference RAISES, the stream cannot: more distinct labels than channels (its one-hot column assignment
 * fails, :24) keeps the first ins_num of them, and a label outside [0, ins_num] (its F.one_hot / indexing fails, :23)
 * joins no row.  Both conditions are recorded in an int32 flags word inside d_work, at byte offset
 * dmnerf_ins_criterion_flags_offset(N, ins_num), valid once _fwd has run on the stream: a caller that wants the
 * reference's behaviour reads it back and raises (the Python mirror does under check=True / DMNERF_CHECK_LABELS=1). */
#define DMNERF_CRIT_TOO_MANY_LABELS 1
#define DMNERF_CRIT_LABEL_RANGE 2
int64_t dmnerf_ins_criterion_work_bytes(int64_t N, int ins_num);
int64_t dmnerf_ins_criterion_flags_offset(int64_t N, int ins_num);
int dmnerf_ins_criterion_fwd(const float* d_pred, const int32_t* d_labels, int64_t N, int ins_num, void* d_work,
                             int64_t work_bytes, float* d_out4, void* stream);
int dmnerf_ins_criterion_bwd(const float* d_pred, const int32_t* d_labels, int64_t N, int ins_num, const void* d_work,
                             const float* d_gout4, float* d_grad_pred, void* stream);
/* The same two calls for TWO predictions against the same labels -- the fine and the coarse level of a training step
 * (train_dmsr.py:38-47) -- in one launch per kernel; each with its own work buffer (work_bytes each) and outputs. */
int dmnerf_ins_criterion_fwd2(const float* d_pred_a, const float* d_pred_b, const int32_t* d_labels, int64_t N, int ins_num,
                              void* d_work_a, void* d_work_b, int64_t work_bytes, float* d_out4_a, float* d_out4_b, void* stream);
int dmnerf_ins_criterion_bwd2(const float* d_pred_a, const float* d_pred_b, const int32_t* d_labels, int64_t N, int ins_num,
                              const void* d_work_a, const void* d_work_b, const float* d_gout4_a, const float* d_gout4_b,
                              float* d_grad_a, float* d_grad_b, void* stream);

/* ---- the scalar tail of the training step (train_dmsr.py:33-61; extension: the reference forms it from tensor operations) ----
 * loss = sum over the levels a (fine), b (coarse) of img2mse(rgb, target) (evaluator.py:11) + ins_criterion (out4[0] of the
 * calls above; nullable) + emptiness penalizer (penalizer.py:43-55 from the four batch sums of dmnerf_penalizer_sums / _sums2;
 * nullable), added in f32 in the training loop's order.  _fwd: d_terms8 = {mse_a, crit_a, pen_a, mse_b, crit_b, pen_b, total, 0},
 * d_pen_inv4 = the penalizer's two normalisers per level.  _bwd, for the upstream scalar d_g_total: d loss / d rgb of both
 * levels ((g / 3N) * (2 (rgb - target)), the products autograd forms), d_gout8 = {g, 0, 0, 0} x 2 for dmnerf_ins_criterion_bwd2
 * and d_pen_scales4 = d_pen_inv4 * g for dmnerf_penalizer_bwd; d_g_partials8 (nullable) = the same factors as the 4-double rows
 * {scale_b, 0, scale_m, 0} per level that dmnerf_composite_pen_bwd reads.  One launch each. */
int dmnerf_loss_tail_fwd(const float* d_rgb_a, const float* d_rgb_b, const float* d_target, int64_t N,
                         const float* d_crit_out4_a, const float* d_crit_out4_b, const double* d_pen_sums4_a,
                         const double* d_pen_sums4_b, int C, float* d_terms8, float* d_pen_inv4, void* stream);
int dmnerf_loss_tail_bwd(const float* d_rgb_a, const float* d_rgb_b, const float* d_target, int64_t N,
                         const float* d_g_total, const float* d_pen_inv4, float* d_grad_rgb_a, float* d_grad_rgb_b,
                         float* d_gout8, float* d_pen_scales4, double* d_g_partials8, void* stream);

/* ---- manipulator.py (scene editing at render time) -----------------------------------
 * manipulator_render (networks/manipulator.py:86-105): render_train whose object map keeps all C channels
 * (d_ins_map [N,C]).  z_val_lerp: the grid of manipulator_nerf (:117-119), near (1-t) + far t.
 * sort_rows: torch.sort(x, -1).values per row (K <= 2048), exact permutation (:191,:195).
 * exchanger (:18-83): per-sample / per-ray argmax labels and the masked swaps of raw rows, d_ori_raw modified in
 * place; h_tar_raws / h_tar_accs: HOST arrays of T device pointers ([N,S,4+C] / [N,C]); h_labels: T moved labels;
 * outputs (nullable): int64 labels [N,S] of the original rays and of the last target.                 */
int dmnerf_manipulator_render(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t N, int S,
                              int C, float* d_rgb_map, float* d_weights, float* d_depth_map,
                              float* d_ins_map, void* stream);
int dmnerf_z_val_lerp(const float* d_t, float near_, float far_, int64_t N, int S, float* d_z, void* stream);
int dmnerf_sort_rows(const float* d_in, int64_t N, int K, float* d_out, void* stream);
int dmnerf_exchanger(float* d_ori_raw, const float* const* h_tar_raws, const float* d_ori_acc,
                     const float* const* h_tar_accs, const int* h_labels, int T, int64_t N, int S, int C,
                     int64_t* d_ori_label, int64_t* d_tar_label, void* stream);
/* dmnerf_edit_exchange: the exchanger (networks/manipulator.py:18-83) generalised to E edits of three kinds plus a keep mask;
 *   d_ori_raw [N,S,4+C] is edited in place.  Per (ray, sample): l0 = the sample's own label (argmax of the sigmoid over C
 *   channels, first maximum), the ray's label from d_ori_acc [N,C] over C - 1 channels; then the edits in order, each first
 *   applying the occlusion correction of :32-33 to the running original label for its label L = h_labels[e]:
 *     h_kinds[e] = 0 MOVE    the loop body of dmnerf_exchanger (:30-81): fill, exchange, eliminate;
 *                  1 COPY    the target's label corrected as for a MOVE; the row is overwritten by the target's only where the
 *                            target sample is L and the original is not; no fill, no eliminate;
 *                  2 REMOVE  row = row * 0.f where the original's label is L (the form of :81, so -0 and NaN arise as there);
 *                            h_tar_raws[e] and h_tar_accs[e] must be NULL (both arrays may be NULL when every edit is a REMOVE).
 *   h_keep (nullable): 128 label bits in two words; after the edits the row becomes row * 0.f when bit l0 is clear.
 *   1 <= E <= 8, or E == 0 with h_keep; 2 <= C <= 128; labels in [0, C).  d_ori_label (nullable): int64 [N,S], the original's
 *   label after the corrections.  Arguments are validated before anything touches a device; no allocation, no sync.          */
int dmnerf_edit_exchange(float* d_ori_raw, const float* const* h_tar_raws, const float* d_ori_acc,
                         const float* const* h_tar_accs, const int* h_labels, const int* h_kinds, int E,
                         const uint64_t* h_keep, int64_t N, int S, int C, int64_t* d_ori_label, void* stream);

/* ---- manipulator.py, the drivers around manipulator(): manipulator_eval / manipulator_demo (csrc/edit_frame.hip) --------------
 * dmnerf_edit_rays: the target rays of T edited objects (1 .. DMNERF_EDIT_MAX_OBJECTS, the exchanger's limit) for image rows
 *   [row0, row0 + nrows), one launch, written as d_rays [T, 2, n, 3] (n = nrows W; [t][0] origins, [t][1] directions) -- the
 *   tensor manipulator() takes as f_tar_rays, replacing the per-object get_rays_k / clone / stack / reshape of networks/
 *   manipulator.py:392-441.  h_intr as for dmnerf_raygen; h_poses [T][12] = the first 3 rows of each object's c2w; h_kind [T]:
 *     0 rigid  -- exactly what dmnerf_raygen writes for that pose and band (the same device function: bit-identical rows;
 *                 :431-433, the pose being trans @ ori_pose formed by the caller);
 *     1 deform -- origin and direction of the pose given (the driver passes the ORIGINAL pose), origin x replaced by
 *                 (float)((double)x + d_off[t][row]) with row the ABSOLUTE image row: tar_rays_o[:, 0] + v_1 of :428, an f32 column
 *                 plus an f64 tensor, summed in f64 and rounded once.  y, z and the direction are unchanged (:427, :429).
 *   d_off: device double [T, H], read only in the rows of deform objects (may be null when there is none).
 * dmnerf_edit_products: what the drivers write out for n pixels (:472-488, :310-323), from STRIDED rows -- pixel p's colour at
 *   d_rgb + p rgb_stride (3 floats), its object channels at d_ins + p ins_stride (C floats; strides in floats, >= 3 / >= C) -- so
 *   the packed band of the frame driver or a channel slice of the gathered frame is read without a copy.  Outputs, each nullable:
 *     d_rgb8 [n,3] uint8    (uint8)(255.f * min(max(x, 0), 1)), the product in f32, truncated: to8b (networks/evaluator.py:13);
 *     d_label [n] int64     argmax over ALL C channels, first maximum (the tie rule of dmnerf_ins_label_conf): the drivers take
 *                           torch.argmax(ins) with the last channel included (:321, :477);
 *     d_mask [n] uint8      (uint8)label (:488);
 *     d_ins_img [n,3] uint8 d_lut[label], d_lut = uint8 [C,3] (render_label2img, tools/visualizer.py:73-86, as a table).
 *   d_ins null: only d_rgb8 is written; d_lut null: d_ins_img is not written.  C <= DMNERF_EDIT_MAX_CHANNELS.  Non-finite
 *   inputs are outside the contract (a NaN colour or object channel gives an unspecified byte / label, never an access outside
 *   the buffers).
 * Both validate their arguments before touching a device (DMNERF_E_ARG), allocate nothing, do not synchronise, run on the
 * caller's stream and are capturable.                                                                                        */
#define DMNERF_EDIT_MAX_OBJECTS 8
#define DMNERF_EDIT_MAX_CHANNELS 129
int dmnerf_edit_rays(int H, int W, const float* h_intr, const float* h_poses, const int* h_kind, int T,
                     const double* d_off, int row0, int nrows, float* d_rays, void* stream);
int dmnerf_edit_products(const float* d_rgb, int64_t rgb_stride, const float* d_ins, int64_t ins_stride, int C,
                         const uint8_t* d_lut, int64_t n, uint8_t* d_rgb8, int64_t* d_label, uint8_t* d_mask,
                         uint8_t* d_ins_img, void* stream);

/* ---- evaluator.py ins_eval, the part every frame needs (networks/evaluator.py:127-137) ----------------
 * d_label [N] int64 = argmax over the C object channels of d_ins [N,C] (first maximum, like torch.argmax on CPU);
 * d_conf [N] (nullable) = that maximum (np.max(pred_ins, -1)).                                                    */
int dmnerf_ins_label_conf(const float* d_ins, int64_t N, int C, int64_t* d_label, float* d_conf, void* stream);

/* ---- evaluator.py ins_eval + calculate_ap, the rest of it (networks/evaluator.py:77-175): instance AP of one frame ---------
 * Replaces the host-side one-hot broadcast [ins_num, ins_num, H W] of hungarian (:55-70), the per-label np.median (:141-145),
 * scipy's match (:43-47) and the AP integral (:77-122) with count-based kernels on the stream (csrc/ins_eval.hip).  ins_num
 * <= 128, 0 <= gt_num <= ins_num.  No host synchronisation, no allocation; capturable.  The caller owns d_work
 * (dmnerf_ins_eval_work_bytes; -1 for unsupported sizes); _prep clears what it needs, so one buffer serves any number of frames.
 *
 * _prep, one pass over the N pixels:
 *   prediction: d_pred_ins (rows of pred_row_stride >= ins_num floats, first ins_num used: a view such as ins[..., :-1] needs no
 *     copy) -> label = argmax (first maximum), conf = max (:127-137); or, with d_pred_ins NULL, d_label_in [N] int64 (in
 *     [0, ins_num); others are flagged DMNERF_IE_LABEL_RANGE and join no count) with d_conf [N];
 *   d_mask [N] (nullable, f32): label = ins_num where mask == 0 (:130-133);
 *   d_label_out [N] int64 = the labels with the mask rule applied (may equal d_label_in: modified in place);
 *   ground truth: d_gt_ins (rows of gt_row_stride >= gt_num floats, columns < gt_num one-hot; a row with another value or more
 *     than one 1 sets DMNERF_IE_GT_NOT_ONEHOT) or, with d_gt_ins NULL, d_gt_label [N] int64 and d_gt_rows [gt_num] int64
 *     ascending: a pixel whose label is d_gt_rows[g] belongs to row g, other pixels to no row.
 * dmnerf_ins_eval then writes d_ap6 [6] f32 = calculate_ap(..., 'integral') at the thresholds 0.5 0.75 0.8 0.85 0.9 0.95, and
 *   d_matched [ins_num] int64 = the returned labels (:169-173) of rows 0..gt_num-1, -1 for an unmatched row and beyond gt_num.
 *   masked != 0: the call of _prep had a mask, and the largest label present is no channel (unique(pred_label)[:-1], :133).
 * Cost entries: cost_siou from the exact counts in the reference's f32 order (bit-equal); cost_ce = 18.420681 x (pixels where
 * the two one-hot maps differ) / N from the counts in f64, rounded once (the reference's last bit depends on ATen's summation
 * order).  Ties of the confidences sort in index order.  No valid label (the reference raises at :172): every row unmatched.
 * dmnerf_ins_eval_flags_offset: byte offset in d_work of the int32 DMNERF_IE_* word written by _prep;
 * dmnerf_ins_eval_median_offset: of the f32 [ins_num] per-label median confidences written by dmnerf_ins_eval (0: no pixel). */
#define DMNERF_IE_LABEL_RANGE 1
#define DMNERF_IE_GT_NOT_ONEHOT 2
int64_t dmnerf_ins_eval_work_bytes(int64_t N, int ins_num);
int64_t dmnerf_ins_eval_flags_offset(int64_t N, int ins_num);
int64_t dmnerf_ins_eval_median_offset(int64_t N, int ins_num);
int dmnerf_ins_eval_prep(const float* d_pred_ins, int64_t pred_row_stride, const int64_t* d_label_in, const float* d_conf,
                         int64_t* d_label_out, const float* d_mask, const float* d_gt_ins, int64_t gt_row_stride,
                         const int64_t* d_gt_label, const int64_t* d_gt_rows, int gt_num, int64_t N, int ins_num,
                         void* d_work, int64_t work_bytes, void* stream);
int dmnerf_ins_eval(int64_t N, int ins_num, int gt_num, int masked, void* d_work, int64_t work_bytes, float* d_ap6,
                    int64_t* d_matched, void* stream);

/* ---- the image scores of render_test / manipulator_eval (networks/tester.py:89-90, networks/manipulator.py:277-278) ----------
 * Replaces skimage.metrics.peak_signal_noise_ratio(rgb.cpu().numpy(), gt, data_range=1) and
 * skimage.metrics.structural_similarity(rgb.cpu().numpy(), gt, multichannel=True, data_range=1): a device-to-host copy of the
 * frame, a synchronisation and ~0.2 s of host filtering per 480x640 pose.  csrc/img_metrics.hip scores P frame pairs on the
 * stream: d_pred, d_gt [P,H,W,C] f32 contiguous, C in 1..4, H, W >= 7 (and <= 32768).
 * SSIM as scikit-image 0.18 documents it for these arguments -- written down without the library at hand, see the kernel file's
 * header -- in float64 throughout: per channel the 7x7 box means ux, uy, uxx, uyy, uxy of x, y, x x, y y, x y; vx = 49/48 (uxx -
 * ux ux), vy, vxy likewise (sample covariance); C1 = 1e-4, C2 = 9e-4;
 *     S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2));
 * the map is cropped by 3 on every side, so only the (H-6)(W-6) windows wholly inside the image count and there is no border
 * rule; d_ssim_ch [P,C] (nullable) = the per-channel means of S, d_ssim [P] = their mean over the channels (summed in channel
 * order, divided by C).  d_mse [P] = mean of (x - y)^2 with the difference and the square in f32 and the sum in f64, d_psnr [P] =
 * 10 log10(1 / mse) in f64, +inf for mse == 0.  A NaN in a frame makes that frame's outputs NaN and touches no other frame.
 * Every 7-tap sum is formed directly; the per-workgroup partials in d_work (dmnerf_img_metrics_work_bytes; -1 for unsupported
 * sizes) are added in index order by a second launch, with no floating-point atomic: results are bit-identical from run to run
 * and independent of P.  No host synchronisation, no allocation; capturable.  P == 0 is a successful no-op.               */
int64_t dmnerf_img_metrics_work_bytes(int P, int H, int W, int C);
int dmnerf_img_metrics(const float* d_pred, const float* d_gt, int P, int H, int W, int C, void* d_work, int64_t work_bytes,
                       double* d_ssim, double* d_ssim_ch, double* d_mse, double* d_psnr, void* stream);

/* ---- LPIPS (VGG16) of rendered frames: lpips.LPIPS(net="vgg")(rgb, gt) of render_test / manipulator_eval (networks/tester.py:43,91,
 * networks/manipulator.py:216,280) -- csrc/conv3x3.hip, csrc/lpips.hip; the definition (lpips 0.1.4, net='vgg', version='0.1',
 * spatial=False) is written down in lpips.hip's header.  All activations are NHWC f32 in the PADDED-FLAT layout: per image
 * (H+2)(W+2) rows of C floats with a zero border, the N images of a batch stacked, W+3 zeroed guard rows before the first and after
 * the last image: N (H+2)(W+2) + 2 (W+3) rows in all; *_floats = floats the buffer holds (checked).  Pointers 16-byte aligned.
 *   dmnerf_conv3x3_pack: torch's [Cout][Cin][3][3] weights as d_out [Cout][ldb], column (3 dy + dx) Cin + c, ldb = 9 Cin rounded up
 *     to 32 (only Cin = 3 rounds: columns 27 .. 31 zero); Cin = 3 or a multiple of 32.
 *   dmnerf_conv3x3: out = relu?(conv3x3(in) + bias), stride 1, zero padding 1, exact f32 (an fmaf chain per output, taps in (dy, dx,
 *     c) order from the bias), padded-flat in, padded-flat out (P images of H x W): the border rows and the guard rows of the output
 *     are written as exact zeros whatever was accumulated there.  Cin, Cout multiples of 32 (32 .. 4096).  taps = 9: the 3x3
 *     convolution; taps = 1 (Cin = 32): d_in is [P (H+2)(W+2)][32] rows WITHOUT guard rows, each holding a whole K range
 *     (dmnerf_lpips_prologue's), and the product is per row -- the first VGG layer.  ReLU keeps a NaN.
 *   dmnerf_maxpool2: 2x2 / stride 2 maximum (floor: an odd last row / column is dropped) of N images H x W x C, padded-flat to
 *     padded-flat (H/2 x W/2), borders and guards written zero; a NaN wins.  C a multiple of 4.
 *   dmnerf_lpips_prologue: frames d_pred, d_gt [P,H,W,3] f32 -> d_taps [2P (H+2)(W+2)][32]: per pixel the 27 taps (3 dy + dx) 3 + c
 *     of the scaled image (x - shift) / scale (normalize != 0: of 2 x - 1), zero outside the image, columns 27 .. 31 and border
 *     rows zero; images 0 .. P-1 = pred, P .. 2P-1 = gt.
 *   dmnerf_lpips_tail: one tapped layer d_feat (padded-flat, 2P images of H x W x C, pred then gt) and its lin weights d_lin [C]:
 *     per pixel sum_c w_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2 in f32, n = sqrt(sum_c f_c^2); the mean over the pixels in
 *     f64 through per-workgroup partials (d_partials: P ceil(H W / 256) doubles) added in index order by a second launch;
 *     d_out [P] (f64) = that mean (first != 0) or d_out + that mean.  No floating-point atomics: bit-identical from run to run,
 *     independent of P; a NaN stays in its frame.
 *   dmnerf_lpips_work_bytes: bytes of the whole metric's workspace for P frame pairs of H x W: [tap rows | activations A |
 *     activations B | partials], each rounded up to 256 bytes (tap rows 2P (H+2)(W+2) x 32 floats; an activation buffer (2P (H+2)(W+2)
 *     + 2 (W+3)) x 64 floats; partials P ceil(H W / 256) doubles); -1 for unsupported sizes (H, W in 16 .. 4096).
 * None allocates or synchronises; all are capturable; P (N) == 0 is a successful no-op; bad sizes return DMNERF_E_ARG.           */
int dmnerf_conv3x3_pack(const float* d_w, int Cout, int Cin, float* d_out, int ldb, void* stream);
int dmnerf_conv3x3(const float* d_in, int64_t in_floats, const float* d_wp, int64_t w_floats, const float* d_bias, float* d_out,
                   int64_t out_floats, int P, int H, int W, int Cin, int Cout, int taps, int relu, void* stream);
int dmnerf_maxpool2(const float* d_in, int64_t in_floats, float* d_out, int64_t out_floats, int N, int H, int W, int C, void* stream);
int dmnerf_lpips_prologue(const float* d_pred, const float* d_gt, int P, int H, int W, int normalize, float* d_taps, int64_t taps_floats,
                          void* stream);
int dmnerf_lpips_tail(const float* d_feat, int64_t feat_floats, const float* d_lin, int P, int H, int W, int C, int first, double* d_partials,
                      int64_t partials_count, double* d_out, void* stream);
int64_t dmnerf_lpips_work_bytes(int P, int H, int W);

/* ---- penalizer.py (the consumer of raw / z_vals / depth) ---------------------------
 * emptiness_penalizer (networks/penalizer.py:5-55) fused: _fwd writes per-ray partial sums
 * d_partials [N,4] (double): {sum BCE*w_before, sum m_before, sum loss_middle*w_middle, sum m_middle};
 *   loss = S0 / (C max(S1,1e-8)) + S2 / max(S3,1e-8) with Sk = sum over rays.
 * _bwd writes dL/draw [N,S,4+C] (zero in channels 0..3) given d_scales = {up/(C max(S1,1e-8)), up/max(S3,1e-8)}.
 * two_deta_w_sq = 2*deta_w^2 and gauss_norm = 0.4*sqrt(2 pi), both rounded to float32 as the reference forms them.
 * depth is a constant (the reference detaches it, penalizer.py:59).                                   */
int dmnerf_penalizer_fwd(const float* d_raw, const float* d_z, const float* d_depth, const float* d_rays_d,
                         int64_t N, int S, int C, float tolerance, float two_deta_w_sq, float gauss_norm,
                         double* d_partials, void* stream);
int dmnerf_penalizer_bwd(const float* d_raw, const float* d_z, const float* d_depth, const float* d_rays_d,
                         int64_t N, int S, int C, float tolerance, float two_deta_w_sq, float gauss_norm,
                         const float* d_scales, float* d_grad_raw, void* stream);
/* The scalar tail of the same function (penalizer.py:44-55) without a chain of scalar tensor operations: _sums reduces the per-ray
 * partials to d_sums4 = {S0, S1, S2, S3} (doubles; one block, fixed order; a ray-sharded caller all-reduces them here), _finish
 * writes d_loss1 = (float)(S0 / (C max(S1,1e-8)) + S2 / max(S3,1e-8)) and d_inv2 = {1 / (C max(S1,1e-8)), 1 / max(S3,1e-8)}
 * (float; d_scales of _bwd = d_inv2 * upstream gradient). */
int dmnerf_penalizer_sums(const double* d_partials, int64_t N, double* d_sums4, void* stream);
/* render_train AND the penalizer's per-ray partial sums in one pass over the ray (extension, SURVEY 8(f)-1: the penalizer's only
 * other input is the ray's own depth, which the compositing pass has just produced): the outputs of dmnerf_composite_fwd plus
 * d_partials [N,4] of dmnerf_penalizer_fwd called with that depth map -- bit-equal to the two calls.  _bwd: dmnerf_composite_bwd
 * plus the penalizer's gradient (dmnerf_penalizer_bwd's values) ADDED in the same pass; d_g_partials = d loss / d partials of ONE
 * ray, 4 doubles, the same for every ray ({up / (C max(sum m_b, 1e-8)), -, up / max(sum m_m, 1e-8), -}: the normalisers are
 * batch sums).  One kernel and one write of d raw instead of two kernels, two writes and an elementwise add. */
int dmnerf_composite_pen_fwd(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t N, int S, int C,
                             float tolerance, float two_deta_w_sq, float gauss_norm, float* d_rgb_map, float* d_weights,
                             float* d_depth_map, float* d_ins_map, double* d_partials, void* stream);
int dmnerf_composite_pen_bwd(const float* d_raw, const float* d_z, const float* d_rays_d, const float* d_ins_map,
                             const float* d_depth_map, const float* d_g_rgb, const float* d_g_ins, const float* d_g_depth,
                             const float* d_g_weights, const double* d_g_partials, int64_t N, int S, int C, float tolerance,
                             float two_deta_w_sq, float gauss_norm, float* d_grad_raw, void* stream);
/* ... of two levels in one launch: d_sums8 = the four sums of a, then of b. */
int dmnerf_penalizer_sums2(const double* d_partials_a, int64_t N_a, const double* d_partials_b, int64_t N_b, double* d_sums8,
                           void* stream);
int dmnerf_penalizer_finish(const double* d_sums4, int C, float* d_loss1, float* d_inv2, void* stream);

/* dm_nerf inference (networks/render.py:31-96, perturb handled by the caller passing t_rand/u):
 * all stages on `stream`, outputs = the 10 tensors of the reference dict (ins_* are [N, C-1]).
 *   d_t_rand: [N,S] or NULL (no jitter); d_u / u_row_stride as in dmnerf_sample_pdf.
 * Scratch: d_weights_ws [N, S+n_imp] floats.                                                  */
typedef struct {
    const float* d_blob_coarse;
    const float* d_blob_fine;
    int ins_num;
    const float* d_rays_o;
    const float* d_rays_d;
    const float* d_z_in;        /* [N,S] coarse depths before jitter */
    const float* d_t_rand;      /* nullable */
    const float* d_u;
    int64_t u_row_stride;
    int64_t N;
    int S;
    int n_imp;
    /* outputs */
    float* d_z_coarse;          /* [N,S]        'z_vals_coarse' (jittered) */
    float* d_raw_coarse;        /* [N,S,4+C]    'raw_coarse'   */
    float* d_rgb_coarse;        /* [N,3]        'rgb_coarse'   */
    float* d_depth_coarse;      /* [N]          'depth_coarse' */
    float* d_ins_coarse;        /* [N,C-1]      'ins_coarse'   */
    float* d_z_fine;            /* [N,S+n_imp]  'z_vals_fine'  */
    float* d_raw_fine;          /* [N,S+n_imp,4+C] 'raw_fine'  */
    float* d_rgb_fine;          /* [N,3]        'rgb_fine'     */
    float* d_depth_fine;        /* [N]          'depth_fine'   */
    float* d_ins_fine;          /* [N,C-1]      'ins_fine'     */
    float* d_weights_ws;        /* scratch [N, S+n_imp] */
    /* optional hipEvent_t pair recorded on `stream` around the fine-network MLP launch (the dominant
     * kernel), so a caller can time it live without splitting the call; NULL = not recorded */
    void* ev_fine_mlp_begin;
    void* ev_fine_mlp_end;
    /* 1: d_blob_coarse / d_blob_fine are fused-heads blobs (dmnerf_build_pack_index_fused); 2: split-bf16 blobs; 3: split-f16 blobs */
    int fused_heads;
} dmnerf_render_args;
int dmnerf_render_rays_fwd(const dmnerf_render_args* args, void* stream);

/* The same render for a caller that keeps only the fine outputs -- render_test (networks/tester.py:71-77) takes rgb_fine, ins_fine
 * and depth_fine from the dict and drops the rest.  Of the coarse level only the compositing weights reach the fine one
 * (networks/render.py:66-70), and they depend on the density channel alone (:6-20), so the coarse network runs as far as
 * density_linear and no further; every fine output is bit-identical to dmnerf_render_rays_fwd's.  Additive: the struct above and
 * dmnerf_render_rays_fwd are unchanged.
 *   dmnerf_mlp_fwd_rays_density: render.py:49-61 + DM_NeRF.forward up to density_linear (networks/dm_nerf.py:80-88,101):
 *     sigma [N,S] = raw[..., 3] of dmnerf_mlp_fwd_rays, bit for bit; d_blob: the forward blob (dmnerf_build_pack_index) or the
 *     fused-heads blob (dmnerf_build_pack_index_fused) -- the trunk and the table entries used are the same in both.
 *   dmnerf_weights_from_sigma: the weights of render_train (render.py:6-20) from that row: weights [N,S] = what
 *     dmnerf_composite_fwd writes for raw[..., 3] = sigma.
 *   dmnerf_render_rays_fwd_fine: jitter / z copy, density-only coarse, weights, resample + merge (render.py:66-70), the full fine
 *     network and its compositing (render.py:71-86).  fused_heads: 0 or 1 (the f32 blobs), or 3 (f16x2, see below; bf16x3 is refused).
 *     d_z_coarse may alias d_z_in when d_t_rand is NULL.  Scratch: d_sigma_ws [N,S], d_weights_ws [N,S+n_imp].              */
int dmnerf_mlp_fwd_rays_density(const float* d_blob, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                const float* d_z, int64_t N, int S, float* d_sigma, void* stream);
int dmnerf_weights_from_sigma(const float* d_sigma, const float* d_z, const float* d_rays_d, int64_t N, int S,
                              float* d_weights, void* stream);
typedef struct {
    const float* d_blob_coarse;
    const float* d_blob_fine;
    int ins_num;
    const float* d_rays_o;
    const float* d_rays_d;
    const float* d_z_in;        /* [N,S] coarse depths before jitter */
    const float* d_t_rand;      /* nullable */
    const float* d_u;
    int64_t u_row_stride;
    int64_t N;
    int S;
    int n_imp;
    float* d_z_coarse;          /* [N,S]        jittered coarse depths (workspace) */
    float* d_sigma_ws;          /* scratch [N,S] */
    float* d_weights_ws;        /* scratch [N,S+n_imp] */
    /* outputs */
    float* d_z_fine;            /* [N,S+n_imp]  'z_vals_fine'  */
    float* d_raw_fine;          /* [N,S+n_imp,4+C] 'raw_fine'  */
    float* d_rgb_fine;          /* [N,3]        'rgb_fine'     */
    float* d_depth_fine;        /* [N]          'depth_fine'   */
    float* d_ins_fine;          /* [N,C-1]      'ins_fine'     */
    void* ev_fine_mlp_begin;    /* as in dmnerf_render_args */
    void* ev_fine_mlp_end;
    int fused_heads;            /* 0 / 1; 3 = f16x2: d_blob_coarse is the f16 density blob */
} dmnerf_render_fine_args;
int dmnerf_render_rays_fwd_fine(const dmnerf_render_fine_args* args, void* stream);

/* A render that does not march through empty space (opt-in; csrc/skip.hip, csrc/mlp_fwd_sparse.hip).  An occupancy bit grid marks
 * the cells of an axis-aligned world box that hold density; a sample whose cell is clear is not evaluated and its row of raw /
 * sigma is zero, which is exactly neutral to the compositing: alpha = 1 - exp(-0) = 0, so its weight is exactly 0, and its rgb,
 * depth and object terms are 0 * x ("Skipping empty space").  Replaces the dense pts -> embed -> network evaluation of
 * networks/render.py:49-61 (coarse) and :71-83 (fine) by one over the marked samples only.  Additive (the ABI version stays).
 *   dmnerf_skip_grid: lo / inv_cell / dims of the box, one bit per cell: cell g = (i * dims[1] + j) * dims[2] + k is bit g & 31 of
 *     word g >> 5 of d_bits [ceil(cells / 32)].  outside: the flag of a sample outside the box.
 *   dmnerf_skip_grid_build: bit(g) = any d_sigma [dx,dy,dz] in the (2 dilate + 1)^3 neighbourhood of g, clipped at the faces, is
 *     > threshold; NaN counts as occupied.  0 <= dilate <= 4; the unused bits of the last word are written 0.
 *   dmnerf_skip_select: for sample m = n * S + s: p = o + d * z (separate multiply and add, as networks/render.py:49),
 *     c_a = floorf((p_a - lo_a) * inv_cell_a) with each operation rounded to f32 on its own; inside iff 0 <= c_a < dims_a on the float
 *     for all three axes (a NaN point is outside).  d_flag [N,S] = the cell's bit, or the outside policy; d_sel = the flagged m in
 *     ascending order (prefix sums: the same list every run); d_count [1] = their number, on the device.  d_work: scratch of
 *     dmnerf_skip_select_work_ints(N * S) int32.  N * S < 2^31.
 *   dmnerf_skip_select_fill: dmnerf_skip_select (same cell arithmetic, flags, ascending d_sel, device-side d_count, same argument
 *     checks) that in the same pass over the samples writes d_fill_row [width] into row m of d_rows [N*S, width] for every sample
 *     whose flag is 0; flagged rows are left untouched (the sparse network writes them afterwards), so no separate fill of the
 *     buffer is needed.  Rows need no alignment (width = 4 + C is rarely a multiple of 4): the stores are one float per lane over
 *     the block's contiguous run of rows.  No atomics.  d_rows == NULL: exactly dmnerf_skip_select (which launches the kernels it
 *     always launched).  d_totals (may be NULL): [2] int64 running sums on the device, += (*d_count, N * S), by a one-thread kernel
 *     behind the select: a plain read-modify-write, so every call that shares one d_totals must be on the same stream; with
 *     N * S == 0 nothing is added.
 *     The manipulation render (networks/manipulator.py) fills with the EMPTY ROW E = (0, 0, 0, 0 | 0, .., 0, 1): sigma 0 makes the
 *     sample's weight exactly 0 in manipulator_render, and the argmax over its C logits is C - 1 -- the label the field gives empty
 *     space, which is never a move label -- where an all-zero row would read as object 0 to the exchanger.
 *   dmnerf_mlp_fwd_rays_sel / dmnerf_mlp_fwd_rays_density_sel: dmnerf_mlp_fwd_rays (fused_heads = 1: dmnerf_mlp_fwd_rays_fused) /
 *     dmnerf_mlp_fwd_rays_density on the samples d_sel [0, *d_count) only: those rows of d_raw [N*S, 4+C] / entries of d_sigma [N*S]
 *     are written, bit-identical to the dense call's; every other row is left untouched (the caller zero-fills).  The batch size is
 *     read on the device; d_sel is read below *d_count only; nothing synchronises, so the chain can be captured in a graph and
 *     replayed with another grid.  N * S < 2^31.
 *   dmnerf_render_rays_fwd_fine_skip: dmnerf_render_rays_fwd_fine with the levels in `levels` (bit 0 coarse, bit 1 fine) evaluated
 *     through the grid: jitter, select on z_coarse, zero-fill of sigma_ws, sparse density network, weights, resample + merge, select
 *     on z_fine, zero-fill of raw_fine, sparse full network, compositing.  A level whose bit is clear runs dense.
 *     d_n_eval [2] = samples evaluated per level.  d_flag, d_sel: [N, S+n_imp]; d_select_ws: dmnerf_skip_select_work_ints(N * (S+n_imp)). */
#define DMNERF_SKIP_OUTSIDE_EVALUATE 0
#define DMNERF_SKIP_OUTSIDE_EMPTY 1
#define DMNERF_SKIP_LEVEL_COARSE 1
#define DMNERF_SKIP_LEVEL_FINE 2
typedef struct {
    float lo[3];
    float inv_cell[3];
    int dims[3];
    int outside;                /* DMNERF_SKIP_OUTSIDE_* */
    const uint32_t* d_bits;
} dmnerf_skip_grid;
int dmnerf_skip_grid_build(const float* d_sigma, int dx, int dy, int dz, float threshold, int dilate, uint32_t* d_bits, void* stream);
int64_t dmnerf_skip_select_work_ints(int64_t M);
int dmnerf_skip_select(const dmnerf_skip_grid* grid, const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S,
                       uint8_t* d_flag, int* d_sel, int* d_count, int* d_work, void* stream);
int dmnerf_skip_select_fill(const dmnerf_skip_grid* grid, const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S,
                            uint8_t* d_flag, int* d_sel, int* d_count, int* d_work, float* d_rows, const float* d_fill_row, int width,
                            int64_t* d_totals, void* stream);
int dmnerf_mlp_fwd_rays_sel(const float* d_blob, int ins_num, int fused_heads, const float* d_rays_o, const float* d_rays_d,
                            const float* d_z, int64_t N, int S, const int* d_sel, const int* d_count, float* d_raw, void* stream);
int dmnerf_mlp_fwd_rays_density_sel(const float* d_blob, int ins_num, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                                    int64_t N, int S, const int* d_sel, const int* d_count, float* d_sigma, void* stream);
typedef struct {
    dmnerf_render_fine_args fine;
    dmnerf_skip_grid grid;
    int* d_sel;                 /* scratch [N, S+n_imp] */
    int* d_n_eval;              /* out [2]: samples evaluated at the coarse / the fine level */
    uint8_t* d_flag;            /* scratch [N, S+n_imp] */
    int* d_select_ws;           /* scratch, dmnerf_skip_select_work_ints(N * (S+n_imp)) */
    int levels;                 /* DMNERF_SKIP_LEVEL_* mask */
} dmnerf_render_fine_skip_args;
int dmnerf_render_rays_fwd_fine_skip(const dmnerf_render_fine_skip_args* args, void* stream);

/* The grid from rendered views instead of from the density at the cell centres (csrc/skip.hip): a cell is worth evaluating if, in
 * some view of interest, a sample in it received a compositing weight (networks/render.py:6-20) above a threshold.  A dense render
 * leaves what this needs on the device: the fine weights in d_weights_ws, the coarse sigma in d_sigma_ws (-> dmnerf_weights_from_sigma).
 * Additive (the ABI version stays).
 *   dmnerf_skip_grid_mark: sample m = n * S + s takes the cell of p = o + d * z (networks/render.py:49) with dmnerf_skip_select's
 *     arithmetic, operation for operation; if p is inside the box and !(d_weights[m] <= threshold) the cell's bit is OR-ed into
 *     d_bits (so a NaN weight marks, as NaN sigma does in the build).  Samples outside the box mark nothing.  Only lo / inv_cell /
 *     dims of `grid` are read -- not grid->outside, not grid->d_bits; d_bits is the writable pointer to the same
 *     ceil(cells / 32) words.  Bits are only ever set: what was set stays, the unused bits of the last word stay 0.  The one
 *     atomic of the file (atomicOr, issued only where the bit still reads clear); OR commutes, so the words are the same every run.
 *     d_z, d_weights [N,S].  N * S < 2^31, S >= 1, threshold >= 0 (NaN refused); N == 0 returns 0 without a launch.  Nothing is
 *     allocated and nothing synchronises: the call can be captured in a graph.
 *   dmnerf_skip_grid_dilate: out(g) = OR of in over the (2 dilate + 1)^3 neighbourhood of g, clipped at the faces -- the dilation
 *     of dmnerf_skip_grid_build with a set bit as the predicate instead of sigma > threshold.  0 <= dilate <= 4; the unused bits
 *     of the last word are written 0; d_bits_in == d_bits_out is refused. */
int dmnerf_skip_grid_mark(const dmnerf_skip_grid* grid, uint32_t* d_bits, const float* d_rays_o, const float* d_rays_d,
                          const float* d_z, const float* d_weights, int64_t N, int S, float threshold, void* stream);
int dmnerf_skip_grid_dilate(const uint32_t* d_bits_in, int dx, int dy, int dz, int dilate, uint32_t* d_bits_out, void* stream);

/* A TRAINING step that does not evaluate empty space (opt-in; csrc/train_skip.hip, autograd.run_network_train_skip).  The select
 * pass above flags the samples and fills the clear rows of raw with zeros; these three entries move data between the dense
 * [N*S, ..] tensors and the compact batch of n_pad >= n_sel one-sample rays that the unchanged training kernels
 * (dmnerf_mlp_fwd_rays_train*, dmnerf_mlp_bwd_data*, dmnerf_mlp_bwd_weights*) run on with N = n_pad, S = 1.  n_sel is the HOST copy
 * of the select's *d_count (the one host read of the path); d_sel is the select's ascending list.  No atomics (the list is strictly
 * ascending: one writer per row), no allocation, no synchronisation.  Additive (the ABI version stays).
 *   dmnerf_skip_gather_samples: d_o, d_d [n_pad,3], d_zc [n_pad]: row i < n_sel is the ray (row d_sel[i] / S of d_rays_o, d_rays_d)
 *     and the depth d_z[d_sel[i]] of sample d_sel[i], copied bit for bit; rows n_sel <= i < n_pad repeat row n_sel - 1, so the padded
 *     launch reads finite, in-range data.  n_pad == 0 returns 0 without a launch; n_pad > 0 with n_sel == 0 is refused.
 *   dmnerf_rows_scatter: row i of d_src [n_pad, width] goes to row d_sel[i] of d_dst [n_rows, width] for i < n_sel; no other row of
 *     d_dst is touched.  n_sel == 0 returns 0 without a launch.
 *   dmnerf_rows_gather: the transpose.  d_dst [n_pad, width]: row i = row d_sel[i] of d_src [n_rows, width] for i < n_sel, exact
 *     zeros for n_sel <= i < n_pad (a padded row's cotangent: it adds exact zeros to every gradient sum).
 *   Rows need no alignment: as in dmnerf_skip_select_fill a block owns the contiguous run of its 256 compact rows, one float per lane
 *   per step.  1 <= width <= 65536.  Refused with DMNERF_E_ARG: negative sizes, n_sel > n_pad, n_sel > n_rows, n_rows (= N * S) or
 *   n_pad >= 2^31, a null pointer with non-zero sizes.  An entry of d_sel outside [0, n_rows) is the caller's bug: that row is
 *   not scattered and gathers as zeros (gather_samples: the last sample), so nothing is read or written out of bounds. */
int dmnerf_skip_gather_samples(const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S, const int* d_sel,
                               int64_t n_sel, int64_t n_pad, float* d_o, float* d_d, float* d_zc, void* stream);
int dmnerf_rows_scatter(const float* d_src, int64_t n_pad, const int* d_sel, int64_t n_sel, float* d_dst, int64_t n_rows, int width,
                        void* stream);
int dmnerf_rows_gather(const float* d_src, int64_t n_rows, const int* d_sel, int64_t n_sel, float* d_dst, int64_t n_pad, int width,
                       void* stream);

/* The occupancy volume labelled by object (csrc/label_grid.hip): which object owns a cell of the box, what every object covers, and
 * the bit grid of a set of objects.  The network runs in front of these (networks/render.py run_network_skip at one point per cell:
 * field.label_grid); none of the three allocates or synchronises, so the chain can be captured in a graph.  Additive (the ABI
 * version stays).
 *   dmnerf_label_cells: one sample per lane.  d_labels[m] = the first index of the maximum of d_raw[m, 4 : 4 + C] if
 *     d_raw[m, 3] > sigma_threshold, else 255 (unlabelled).  The comparison is exactly that: a NaN sigma is unlabelled, and so is
 *     the empty row (sigma 0).  The argmax is dmnerf_ins_label_conf's: best = 0, and channel c > 0 replaces it iff x[c] > x[best];
 *     ties go to the first channel, a NaN logit in a channel c > 0 is never chosen and a NaN in channel 0 is never replaced
 *     (label 0).  The exchanger takes the same first-maximum argmax over ALL C logits, behind a sigmoid (networks/manipulator.py:18-20;
 *     monotone, so the two agree unless two unequal logits round to one f32 sigmoid -- both above ~17, where the exchanger keeps
 *     the first): a cell labelled k is a cell whose centre sample the manipulation render treats as object k.  1 <= C <= 128,
 *     sigma_threshold >= 0 (NaN refused), M == 0 returns 0 without a launch.
 *   dmnerf_label_stats: over d_labels [dx,dy,dz] (cell (i,j,k) at (i * dy + j) * dz + k), per label l < C: d_count [C] = number of
 *     cells, d_index_sum [C,3] = sums of their i, j, k, d_lo [C,3] = smallest index per axis, d_hi [C,3] = largest index + 1.  The
 *     call initialises the outputs itself (count 0, sums 0, lo = dims, hi = 0: what a label without a cell keeps).  Labels >= C,
 *     255 included, are ignored.  Integer atomics only (LDS table per workgroup, then atomicAdd / atomicMin / atomicMax): the same
 *     result every run.  1 <= C <= 128, dx dy dz < 2^31.
 *   dmnerf_skip_grid_from_labels: bit g of d_bits [ceil(n_cells / 32)] (the packing of dmnerf_skip_grid) is set iff
 *     d_labels[g] < 128 and bit d_labels[g] of the 128-bit `mask` is set: label l is bit l & 31 of mask[l >> 5], a HOST array --
 *     the two 64-bit words of networks/manipulator.py keep_words, little end first.  Every word is written, the unused bits of the
 *     last one 0; no atomics.  1 <= n_cells < 2^31. */
int dmnerf_label_cells(const float* d_raw, int64_t M, int C, float sigma_threshold, uint8_t* d_labels, void* stream);
int dmnerf_label_stats(const uint8_t* d_labels, int dx, int dy, int dz, int C, int64_t* d_count, int64_t* d_index_sum, int32_t* d_lo,
                       int32_t* d_hi, void* stream);
int dmnerf_skip_grid_from_labels(const uint8_t* d_labels, int64_t n_cells, const uint32_t mask[4], uint32_t* d_bits, void* stream);

/* What is connected in a label volume (csrc/components.hip): 3-D connected-component labelling and the filters built on it, so stray
 * cells can be dropped from the volume itself.  tests/_components_restate.py states all of it in numpy.  Additive (the ABI version
 * stays).
 *   Contract (canonical: independent of the algorithm and of the execution order).  d_labels [dx,dy,dz] uint8, cell (i,j,k) at
 *     g = (i * dy + j) * dz + k.  A cell is labelled iff d_labels[g] < C.  Two labelled cells are adjacent iff they carry the same
 *     label and differ by exactly one in one axis (connectivity 6) or by at most one in every axis without being the same cell (26);
 *     nothing wraps round the box.  Components are the equivalence classes of adjacency.
 *   dmnerf_label_components: d_root [dx,dy,dz] int32 = the smallest index g of the cell's component, -1 for an unlabelled cell;
 *     d_size [dx,dy,dz] int32 = the number of cells of the cell's component, 0 for an unlabelled cell.  Both are written whole and
 *     are the call's only workspace.  A tile pass (union-find on LDS parents inside 8 x 8 x 32 cells), a seam pass (cells with a
 *     neighbour of smaller index in another tile join it in d_root: find with path halving, the larger root hooked under the smaller
 *     by atomicMin, a failed hook retried from the returned, strictly smaller index), a flatten and a size pass.  parent[x] <= x
 *     always, so every walk descends and ends; no loop waits for another lane or workgroup, no grid-wide synchronisation.  Integer
 *     atomics only: the same arrays every run.
 *   dmnerf_label_components_largest: d_best [C] int64, written whole: for a label with a cell, size << 32 | (0x7fffffff - root) of its
 *     largest component, the smallest root on equal sizes (atomicMax over the root cells); 0 for a label without a cell.
 *   dmnerf_label_components_filter: d_root / d_size as dmnerf_label_components wrote them for the same d_labels and C; mask = four HOST
 *     words (dmnerf_skip_grid_from_labels' packing).  A cell whose label is < C and in the mask keeps its label iff its component has
 *     size >= min_cells and, with mode DMNERF_COMPONENTS_KEEP_LARGEST, is the largest component of its label (d_best, which the call
 *     computes first in that mode, as dmnerf_label_components_largest does; mode DMNERF_COMPONENTS_KEEP_ALL neither writes nor
 *     reads it); otherwise d_out_labels[g] = 255.  Every other cell passes through
 *     unchanged.  With d_cells [dx,dy,dz,4] f32 (else null, with d_out_cells; both 16-byte aligned) a cell that loses its label gets
 *     four zeros, every other cell its 16 bytes copied bit for bit.  d_removed / d_kept [C] int64, written whole: per label < C the
 *     cells that lost it and the cells that carry it in d_out_labels (labels outside the mask count as kept): removed + kept =
 *     dmnerf_label_stats' count.  Ballots and popcounts per wave into an LDS table, then integer atomics.  The outputs must not
 *     overlap the inputs.
 *   Refused with DMNERF_E_ARG before anything touches a device: a dim < 1, dx dy dz >= 2^31, C outside 1..128, a connectivity other
 *     than 6 or 26, min_cells < 1, a mode other than the two, a null pointer, cells given on one side only or misaligned.  No
 *     allocation, no synchronisation, no host read: each can be captured in a graph and reads d_labels anew on every replay.  All three
 *     return the status as int32_t, as dmnerf_volume_edit does. */
#define DMNERF_COMPONENTS_KEEP_ALL 0
#define DMNERF_COMPONENTS_KEEP_LARGEST 1
int32_t dmnerf_label_components(const uint8_t* d_labels, int dx, int dy, int dz, int C, int connectivity, int32_t* d_root, int32_t* d_size,
                            void* stream);
int32_t dmnerf_label_components_largest(const uint8_t* d_labels, int dx, int dy, int dz, int C, const int32_t* d_root, const int32_t* d_size,
                                    int64_t* d_best, void* stream);
int32_t dmnerf_label_components_filter(const uint8_t* d_labels, const float* d_cells, int dx, int dy, int dz, int C, const uint32_t mask[4],
                                   const int32_t* d_root, const int32_t* d_size, int min_cells, int mode, int64_t* d_best,
                                   uint8_t* d_out_labels, float* d_out_cells, int64_t* d_removed, int64_t* d_kept, void* stream);

/* Rays through the label volume (csrc/label_trace.hip): the first cell along a ray whose label belongs to a set -- an object from
 * a pixel, an edit previewed without the networks.  Additive (the ABI version stays).
 *   dmnerf_label_trace: d_labels [dx,dy,dz] uint8 over the box whose lower corner, cell size, 1 / cell size and dims are the HOST
 *     arrays lo, cell, inv_cell, dims (the values field.SkipGrid / field.LabelGrid compute); d_rays [R,2,N,3] = R ray sets of N
 *     (origin, direction) pairs; masks = R x 4 HOST words, set r accepting label l iff l < C and bit l & 31 of masks[4 r + (l >> 5)]
 *     is set (dmnerf_skip_grid_from_labels' words).  Label 255 and every label >= C are never accepted.  Per set and pixel, one
 *     lane: exact cell-by-cell traversal, every f32 operation rounded on its own (tests/_label_trace_restate.py states it in numpy).
 *     The planes of axis a are lo_a + float(b) * cell_a, b = 0 .. dims_a; the ray is clipped against the box and [t_near, t_far]
 *     (an axis with d_a == 0 bounds nothing if lo_a <= o_a < plane_a(dims_a), else the ray misses) and misses unless
 *     t_enter < t_exit, so a NaN anywhere is a miss; the walk starts in the (clamped) cell of o + d t_enter, visits at most
 *     dx + dy + dz + 1 cells, accepts the first cell of the set at the current t, and otherwise crosses the nearest next plane
 *     (tmax_a recomputed from the integer index, the lowest axis on ties), missing once that plane is not in front of t_exit.
 *     Per pixel the hit with the smallest t over the sets wins, the lowest set on equal t: d_label [N] uint8 (255 on a miss),
 *     d_t [N] f32 (+inf), d_cell [N] int32 = (i * dy + j) * dz + k (-1), d_source [N] uint8 = the set (255).
 *     1 <= R <= 16, 1 <= C <= 128, dims >= 1 with dx dy dz < 2^31, N >= 0; N == 0 returns 0 without a launch.  No allocation, no
 *     synchronisation, no atomics: it can be captured in a graph and reads d_labels anew on every replay. */
int dmnerf_label_trace(const uint8_t* d_labels, const float lo[3], const float cell[3], const float inv_cell[3], const int dims[3], int C,
                       const float* d_rays, int R, int64_t N, const uint32_t* masks, float t_near, float t_far, uint8_t* d_label,
                       float* d_t, int32_t* d_cell, uint8_t* d_source, void* stream);

/* The baked field volume (csrc/label_grid.hip, csrc/baked.hip): colour logits and density kept per cell next to the label, and
 * volume-rendered along rays -- an edit previewed with colour, soft edges and a weighted depth, still without the networks.
 * Additive (the ABI version stays).
 *   dmnerf_bake_cells: one sample per lane over d_raw [M, 4 + C].  d_labels[m] follows exactly the rule of dmnerf_label_cells: the
 *     first maximum over all C logits where d_raw[m, 3] > sigma_threshold, else 255.  d_cells [M, 4] holds, for a labelled row, the
 *     four floats d_raw[m, 0:4] (three colour logits and sigma) copied bit for bit, and four exact zeros for an unlabelled row; each
 *     row is one 16-byte store, so d_cells must be 16-byte aligned (else DMNERF_E_ARG).  1 <= C <= 128, sigma_threshold >= 0 (NaN
 *     refused), M == 0 returns 0 without a launch.  No atomics, no allocation, no synchronisation.
 *   dmnerf_baked_render: dmnerf_label_trace's arguments (d_labels, the box arrays, C, d_rays [R,2,N,3], R x 4 HOST mask words,
 *     t_near, t_far) plus d_cells [dx,dy,dz,4] (16-byte aligned) and `stop`; 1 <= R <= 4 (every set's walk state lives in registers).
 *     One lane per pixel, every f32 operation rounded on its own (tests/_baked_restate.py states it in numpy).
 *     Walk: each set's clip, start cell, cell sequence and t values are dmnerf_label_trace's, but the walk goes on behind a counted
 *       cell (at most dx + dy + dz + 1 cells per set).  A cell of set r counts if its label is < C and in the set's mask; the
 *       16-byte d_cells entry is read for a counted cell only.
 *     Segment: for a counted cell t_in is the walk's current t, t_out the next plane crossing tmax_a if tmax_a < t_exit, else
 *       t_exit; len = (t_out - t_in) * |d_r|, |d| = sqrtf(d0 d0 + d1 d1 + d2 d2) summed in that order.
 *     Merge: the pending segments of the R sets are composited in ascending t_in, the lowest set first on equal t_in (a pixel's rays
 *       share the ray parameter); within a set the walk's order stands; a set without a further counted cell drops out.
 *     Composite: alpha = 1 - expf(-max(sigma, 0) * len), w = T * alpha, T <- T * (1 - alpha) from T = 1;
 *       rgb += w * 1 / (1 + expf(-logit)); depth += w * t_in; acc += w.  The label and source of the pixel are those of the segment
 *       with the largest w so far (a strict > from best_w = 0: the first wins ties; without a positive weight 255 / 255).  After a
 *       segment the pixel stops if T < stop; stop = 0 never stops early.  max(sigma, 0) is sigma > 0 ? sigma : 0: a NaN sigma
 *       contributes nothing.  (A ray of direction 0 inside the box has segments of length 0 * (t_out - t_in): nothing for a finite
 *       t_far, NaN for an infinite one.)
 *     Outputs [N]: d_rgb [N,3], d_depth, d_acc f32; d_label, d_source uint8; d_nseg int32, the number of composited segments.  A
 *     pixel whose sets all miss gets zeros, 255 / 255 and 0.
 *     Refused: what dmnerf_label_trace refuses, R > 4, a stop that is negative or NaN, a misaligned d_cells.  N == 0 returns 0
 *     without a launch.  No allocation, synchronisation, atomics or float reductions across lanes: it can be captured in a graph and
 *     reads d_labels and d_cells anew on every replay. */
int dmnerf_bake_cells(const float* d_raw, int64_t M, int C, float sigma_threshold, uint8_t* d_labels, float* d_cells, void* stream);
int dmnerf_baked_render(const uint8_t* d_labels, const float* d_cells, const float lo[3], const float cell[3], const float inv_cell[3],
                        const int dims[3], int C, const float* d_rays, int R, int64_t N, const uint32_t* masks, float t_near, float t_far,
                        float stop, float* d_rgb, float* d_depth, float* d_acc, uint8_t* d_label, uint8_t* d_source, int32_t* d_nseg,
                        void* stream);

/* An edit applied to the volume itself (csrc/volume_edit.hip): the label / baked volume resampled under a list of moves, copies and
 * removals into a volume of the same kind, with what the edit covers and what it collides with.  Additive (the ABI version stays).
 *   dmnerf_volume_edit: d_labels [dx,dy,dz] uint8 and, for a baked volume, d_cells [dx,dy,dz,4] f32 (else null, with d_out_cells)
 *     over the box of the HOST arrays lo, cell, inv_cell, dims (dmnerf_label_trace's); keep = the four HOST words of the labels that
 *     exist at all (dmnerf_skip_grid_from_labels' mask); entries = E <= 32 HOST entries {kind, label, m[12]}: kind 0 MOVE / 1 COPY /
 *     2 REMOVE (networks/manipulator.py), label in [0, C), m = rows 0..2 of the entry's 4 x 4 matrix in f32.  The target pose of an
 *     entry is trans @ pose, so the edited volume at x is the source volume at trans x: m maps the centre of a DESTINATION cell to its
 *     source point, no inverse is taken.  One lane per destination cell g = (i * dy + j) * dz + k, every f32 operation rounded on its
 *     own (tests/_volume_edit_restate.py states it in numpy):
 *     Centre: p_a = (float(idx_a) + 0.5) * cell_a + lo_a.
 *     Candidate 0, the cell's own content: its label l0 < C, in keep, and not the label of a MOVE or REMOVE entry.
 *     Candidate 1 + e, for a MOVE or COPY entry e: q_a = ((m_a0 p_x + m_a1 p_y) + m_a2 p_z) + m_a3, c_a = floor((q_a - lo_a) *
 *       inv_cell_a); it exists iff 0 <= c_a < dims_a on all axes (false for NaN), the source label there equals the entry's label and
 *       that label is in keep.  Nearest-cell resampling: no interpolation.
 *     Winner: rule 0 ("first") the lowest candidate; rule 1 ("densest", baked only) the candidate with the largest source sigma
 *       (d_cells[..., 3]), the lowest on equal sigma; a NaN sigma never beats a number and loses to any number.
 *     Outputs per cell: d_out_labels = the winner's label or 255; d_out_source = the winner's candidate number or 255 (1 + e counts
 *       REMOVE entries: it is the index into the list); d_out_cells = the winner's 16 bytes (one load, one store), zeros without one.
 *     Counts, written whole by the call: d_won [1 + E] cells per winner; d_claimed [E] cells where candidate 1 + e exists; d_hits
 *       [E, C]: for every cell with two or more candidates, every entry e among them and every OTHER candidate b there,
 *       hits[e, label(b)] += 1, label(0) being the cell's own label.  Integer atomics only (per-wave popcounts into an LDS table, one
 *       flush): the same numbers every run.
 *     Returns the status as int32_t: 0 or a DMNERF_E_* code, with dmnerf_last_error() set, like every other entry.
 *     E == 0 is legal (the volume filtered by keep; d_claimed and d_hits are empty and may be null).
 *     Refused: bad dims / C / E / kind / label / rule, rule 1 without d_cells, d_cells without d_out_cells or the reverse, cells not
 *     16-byte aligned, a destination (volume, source or count buffer) that overlaps a source or another destination.  No allocation,
 *     no synchronisation, no host read: it can be captured in a graph and reads d_labels / d_cells anew on every replay. */
#define DMNERF_VOLUME_EDIT_MAX 32
typedef struct {
    int kind;
    int label;
    float m[12];
} dmnerf_volume_edit_entry;
int32_t dmnerf_volume_edit(const uint8_t* d_labels, const float* d_cells, const float lo[3], const float cell[3], const float inv_cell[3],
                           const int dims[3], int C, const uint32_t keep[4], const dmnerf_volume_edit_entry* entries, int E, int rule,
                           uint8_t* d_out_labels, float* d_out_cells, uint8_t* d_out_source, int64_t* d_won, int64_t* d_claimed,
                           int64_t* d_hits, void* stream);

/* The trained field rendered through an edited volume (csrc/field_edit.hip; networks/render.py run_network_edited): the `source`
 * volume of dmnerf_volume_edit says whose content stands in every cell of the edited scene, so every sample needs ONE network
 * evaluation at a known place.  The network between the two entries is dmnerf_mlp_fwd_rays_sel / .._f16_sel called with
 * (d_o_w, d_d_w, d_z, N = N * S, S = 1, d_sel, d_count).  Additive (the ABI version stays).
 *   dmnerf_field_edit_select: dmnerf_skip_select_fill over the byte volume d_source [dx,dy,dz] instead of a bit grid.  lo, inv_cell,
 *     dims: HOST arrays of the box (dmnerf_skip_grid's values); entries: E <= 32 HOST dmnerf_volume_edit_entry, the list the volume
 *     was edited with.  Sample m = n * S + s: p = o + d * z and c_a = floorf((p_a - lo_a) * inv_cell_a) with dmnerf_skip_select's
 *     arithmetic, operation for operation (a NaN point is outside).  Its owner: inside the box the byte b = d_source[cell], read as 255
 *     if b > E or entry b - 1 is a REMOVE; b == 255 gives the `unowned` policy, a point outside the box the `outside` policy
 *     (DMNERF_SKIP_OUTSIDE_EVALUATE: owner 0, DMNERF_SKIP_OUTSIDE_EMPTY: owner 255).
 *       owner 255: not evaluated; row m of d_rows [N*S, 4 + C] becomes d_fill_row [4 + C] (d_rows may be NULL: no fill).
 *       owner 0: evaluated on its own ray: d_o_w[m] = o, d_d_w[m] = d, copied bit for bit.
 *       owner 1 + e: evaluated on the ray carried back into the trained scene, every f32 operation rounded on its own:
 *         d_o_w[m]_a = ((m_a0 o_x + m_a1 o_y) + m_a2 o_z) + m_a3,  d_d_w[m]_a = (m_a0 d_x + m_a1 d_y) + m_a2 d_z (no translation).
 *     Outputs: d_owner [N*S] uint8; d_o_w, d_d_w [N*S,3], written for evaluated samples only; d_sel = the evaluated m in ascending
 *     order (prefix sums: the same list every run), d_count [1] their number, on the device; d_work: scratch of
 *     dmnerf_skip_select_work_ints(N * S) int32; d_totals (may be NULL): [2] int64, += (*d_count, N * S), as in
 *     dmnerf_skip_select_fill.  tests/_field_edit_restate.py states it in numpy.
 *   dmnerf_field_edit_filter: one lane per row of d_raw [M, 4 + C].  A row whose d_owner[m] is 255 is left alone.  Otherwise its label
 *     is the first maximum over its C logits (dmnerf_label_cells' argmax with its tie and NaN rules, no sigma threshold); if bit
 *     label & 31 of masks[4 * owner + (label >> 5)] is clear the row is overwritten with d_fill_row [4 + C].  masks: (1 + E) x 4 HOST
 *     words (dmnerf_skip_grid_from_labels' packing).  d_kept (may be NULL): [1 + E] int64, written whole by the call: the rows kept per
 *     owner (ballots and popcounts into an LDS table, integer atomics: the same numbers every run).  Rows need no alignment.
 *   Refused with DMNERF_E_ARG before anything is launched: a null pointer, N < 0, S < 1, N * S (M) >= 2^31, dims < 1 or dx dy dz >= 2^31,
 *   C outside 1..128, E outside 0..32, an unknown policy, an entry whose kind is not 0..2 or whose label is outside [0, C).  N * S == 0
 *   (M == 0) returns 0 without a launch (nothing is written, *d_count included).  No float atomics, no allocation, no synchronisation: the chain can be
 *   captured in a graph and reads d_source anew on every replay.  Both return the status as int32_t, as dmnerf_volume_edit does. */
int32_t dmnerf_field_edit_select(const uint8_t* d_source, const float lo[3], const float inv_cell[3], const int dims[3], int outside,
                                 int unowned, const dmnerf_volume_edit_entry* entries, int E, int C, const float* d_rays_o,
                                 const float* d_rays_d, const float* d_z, int64_t N, int S, uint8_t* d_owner, float* d_o_w,
                                 float* d_d_w, int* d_sel, int* d_count, int* d_work, float* d_rows, const float* d_fill_row,
                                 int64_t* d_totals, void* stream);
int32_t dmnerf_field_edit_filter(float* d_raw, const uint8_t* d_owner, int64_t M, int C, const uint32_t* masks, int E,
                                 const float* d_fill_row, int64_t* d_kept, void* stream);

/* The two renders above on the OPT-IN split-f16 ("f16x2") kernels (csrc/mlp_f16_density.hip, csrc/mlp_f16_sparse.hip; the body of
 * csrc/mlp_f16_impl.h with template flags).  Additive (the ABI version stays).
 *   f16 density blob: dmnerf_blob_f16_density_words 32-bit words = [the f16 blob's 4096-float bias table | its 120 trunk groups
 *     (mlps.0 .. mlps.7) | its 2 density_linear groups | 6 landing groups]; dmnerf_blob_f16_density_from_f16 copies them out of
 *     a packed f16 blob (dmnerf_pack_f16) on `stream`, device to device.  Re-make it whenever the f16 blob is re-packed.
 *   dmnerf_mlp_fwd_rays_density_f16: render.py:49-61 + DM_NeRF.forward up to density_linear (networks/dm_nerf.py:80-88,101):
 *     sigma [N,S] = raw[..., 3] of dmnerf_mlp_fwd_rays_f16, bit for bit (the same MFMAs on the same tiles in the same order).
 *   dmnerf_mlp_fwd_rays_f16_sel / dmnerf_mlp_fwd_rays_density_f16_sel: dmnerf_mlp_fwd_rays_f16 (render.py:71-83) /
 *     dmnerf_mlp_fwd_rays_density_f16 on the samples d_sel [0, *d_count) only, with the contract of dmnerf_mlp_fwd_rays_sel: those
 *     rows of d_raw [N*S, 4+C] / entries of d_sigma [N*S] are written, bit-identical to the dense call's, every other row is left
 *     untouched; the batch size is read on the device, d_sel below *d_count only; *d_count == 0 is legal.  N * S < 2^31.
 *   dmnerf_render_rays_fwd_fine / .._fine_skip with fused_heads = 3: d_blob_coarse is the f16 DENSITY blob of the coarse model,
 *     d_blob_fine the f16 blob of the fine model (two formats: d_blob_coarse == d_blob_fine is refused); the chains are otherwise
 *     unchanged.  fused_heads = 2 (bf16x3) is refused. */
int64_t dmnerf_blob_f16_density_words(int ins_num);
int dmnerf_blob_f16_density_from_f16(const float* d_blob_f16, int ins_num, float* d_blob_f16_density, void* stream);
int dmnerf_mlp_fwd_rays_density_f16(const float* d_blob_f16_density, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                    const float* d_z, int64_t N, int S, float* d_sigma, void* stream);
int dmnerf_mlp_fwd_rays_f16_sel(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                                int64_t N, int S, const int* d_sel, const int* d_count, float* d_raw, void* stream);
int dmnerf_mlp_fwd_rays_density_f16_sel(const float* d_blob_f16_density, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                        const float* d_z, int64_t N, int S, const int* d_sel, const int* d_count, float* d_sigma,
                                        void* stream);

/* The density of the field off the rays: what mesh_main (tools/mesh_generator.py:12-143) asks the fine network for (csrc/mlp_fwd_points.hip).
 * Both entries run dmnerf_mlp_fwd_rays_density's body -- encoding, trunk, density_linear; no direction, no heads -- so sigma is
 * raw[..., 3] of the full network bit for bit, and both take the forward blob or the fused-heads blob.  Neither allocates nor
 * synchronises.  voxel < 0: d_out [M] = sigma.  voxel >= 0: d_out [M] = 1 - exp(-relu(sigma) * voxel), occupancy_activation of
 * mesh_generator.py:54-60 with distances = voxel, full-precision exp.  Additive (the ABI version stays).
 *   dmnerf_mlp_fwd_points_density: d_pts [M,3] contiguous.  Replaces mesh_generator.py:36-51 for one chunk: embed(in_pcd) |
 *     embed(zeros) -> model_fine(embedded)[..., 3], without the [n, 90] tensor.
 *   dmnerf_occupancy_slab: samples [m0, m0 + M) of a dim^3 grid, flattened as reshape(-1, 3) flattens it (g = (i * dim + j) * dim + k);
 *     sample g computes its own point and no point tensor exists.  Replaces mesh_generator.py:27-31 (grid_within_bound,
 *     tools/visualizer.py:111-155, then the axis swap) and :36-63 for the slab.  d_t [dim] = torch.linspace(lo, hi, dim) as the host
 *     evaluates it; scale [3] = float32(extents / (hi - lo)) and transform [12] = rows 0..2 of the 4 x 4 scene transform, row-major
 *     (R_r0 R_r1 R_r2 T_r) -- HOST pointers, copied into the kernel arguments.  x = t[i] s0, y = t[j] s1, z = t[k] s2,
 *     q_r = ((R_r0 x + R_r1 y) + R_r2 z) + T_r with every product and sum rounded to f32 on its own (the reference's unfused torch
 *     ops), point = (q_0, -q_2, q_1).  1 <= dim <= 1024; 0 <= m0, m0 + M <= dim^3.                                              */
int dmnerf_mlp_fwd_points_density(const float* d_blob, int ins_num, const float* d_pts, int64_t M, float* d_out, float voxel,
                                  void* stream);
int dmnerf_occupancy_slab(const float* d_blob, int ins_num, const float* d_t, int dim, const float* scale, const float* transform,
                          int64_t m0, int64_t M, float* d_out, float voxel, void* stream);

/* ---- network shapes other than D = 8, W = 256, multires 10 / 4 (config.py:126-138 passes args.netdepth / netwidth /
 * multires* through; no shipped config changes them): the layer-by-layer path of csrc/generic.hip.  One strided f32-MFMA
 * GEMM serves the three products of a linear layer; the Python mirror (dm_nerf_amd/generic.py) chains them as
 * DM_NeRF.forward does (networks/dm_nerf.py:80-106) and as its autograd would.
 *   dmnerf_gemm:   C[i*ldc + j] (+)= sum_k A[i*sai + k*sak] * B[k*sbk + j*sbj]   (+ bias[j], ReLU, * [mask[i*ldm + j] > 0]);
 *                  splits > 1: split-K over k with a workspace of splits*I*J floats, partials added in slice order
 *                  (then no bias / relu / mask).
 *   dmnerf_colsum: out[j] = sum_m X[m*ldx + j] (bias gradient), workspace slices*J floats.
 *   dmnerf_ray_points: pts [N*S,3] = o + d z, dirs [N*S,3] = d / |d| per sample (render.py:37,49-57).
 *   dmnerf_copy_cols:  dst[m*ld_dst + c] = src[m*ld_src + c], c < n (the cat of dm_nerf.py:87,90 into a column slice). */
int dmnerf_gemm(const float* d_A, int64_t sai, int64_t sak, const float* d_B, int64_t sbk, int64_t sbj, float* d_C, int64_t ldc,
                int64_t I, int J, int64_t K, const float* d_bias, int relu, const float* d_mask, int64_t ldm, int accumulate,
                float* d_ws, int splits, void* stream);
int dmnerf_colsum(const float* d_X, int64_t ldx, int64_t M, int J, float* d_out, float* d_ws, int slices, void* stream);
int dmnerf_ray_points(const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S, float* d_pts,
                      float* d_dirs, void* stream);
int dmnerf_copy_cols(const float* d_src, int64_t ld_src, float* d_dst, int64_t ld_dst, int64_t M, int n, void* stream);

/* The same path's forward and data-gradient products on the machine's own terms (csrc/gemm_nt.hip, ABI 7): both operands k-fast,
 * global -> LDS by LDS-DMA into a swizzled ring, ds_read_b128 operand reads, one workgroup = 128 samples x all outputs of the layer.
 *   dmnerf_pack_nt: the layer's weight matrix in the kernel's form -- d_out [rows_pad][ldb], rows_pad = 32 x dmnerf_gemm_nt_blocks(n)
 *     x tiles, ldb = 32 (ceil(k0 / 32) + ceil(k1 / 32)), zero-filled padding: row n = source row n, columns [c0, c0 + k0) then (from
 *     column 32 ceil(k0 / 32)) [c1, c1 + k1) -- the two K ranges of a layer whose input is a cat (dm_nerf.py:87 [h, pts], :90
 *     [rgb_feature, dirs]); transposed != 0: the source is read as W^T (row n = source COLUMN n, column k = source ROW c + k): the
 *     data-gradient form.  d_bias_out [rows_pad] (nullable) = the bias, zero beyond n_rows.
 *   dmnerf_gemm_nt: C[m*ldc + n] = act(sum_k A(m, k) Wp[n][k] + bias[n]) for m < M, n < n_store, zeros in columns [n_store, n_zero)
 *     (the pad columns that keep the NEXT layer's operand rows 16-byte aligned); A(m, k) = A0[m*lda0 + k] for k < k0, then
 *     A1[m*lda1 + (k - k0)] (k1 = 0: one range); lda0 / lda1 multiples of 4, base pointers 16-byte aligned, a*_floats = floats from the
 *     pointer to the end of its allocation (the kernel's descriptor bound).  A-operand contract: the kernel reads columns
 *     [0, 32 ceil(k0 / 32)) of every A0 row (likewise A1 with k1), so lda0 >= 32 ceil(k0 / 32) and lda1 >= 32 ceil(k1 / 32) -- a shorter
 *     row is refused with DMNERF_E_ARG, as its last chunk would read the next row -- and the columns read past k0 / k1 must be finite:
 *     they meet zero weights, but 0 * NaN = NaN.  relu; d_mask (nullable): C = mask[m*ldm + n] > 0 ? v : 0 (the
 *     ReLU derivative of the data gradient); accumulate: C += before relu / mask.  Bias is the accumulator's initial value.
 *   dmnerf_ray_embed: pts = o + d z, viewdirs = d / |d| per sample (render.py:37,49-57) and Embedder.embed of both (dm_nerf.py:37-38)
 *     into row-padded buffers x_pos [N*S][ldp], x_dir [N*S][ldv], pad columns zeroed.
 *   dmnerf_copy_cols_pad: dst[m*ld_dst + c] = c < n ? src[m*ld_src + c] : 0 for c < n_pad -- a column slice as such an operand.      */
int dmnerf_gemm_nt_blocks(int n_out);
int dmnerf_pack_nt(const float* d_W, int64_t ldw, int n_rows, int c0, int k0, int c1, int k1, int transposed, const float* d_bias,
                   float* d_out, int rows_pad, int ldb, float* d_bias_out, void* stream);
int dmnerf_gemm_nt(const float* d_A0, int64_t lda0, int64_t a0_floats, int k0, const float* d_A1, int64_t lda1, int64_t a1_floats, int k1,
                   const float* d_B, int64_t b_floats, int ldb, const float* d_bias, float* d_C, int64_t ldc, int n_store, int n_zero,
                   int64_t M, int relu, const float* d_mask, int64_t ldm, int accumulate, void* stream);
/* The same path's WEIGHT gradient (csrc/gemm_tn.hip, ABI 8): dW[i*ldw + j] = sum_m dy[m*ldy + i] x[m*ldx + j] for i < n_out, j < n_in
 * and (d_db non-null) db[i] = sum_m dy[m*ldy + i] -- both operands sample-major rows as gemm_nt reads and writes them (ldy / ldx multiples
 * of 4, base pointers 16-byte aligned, *_floats = floats from the pointer to the end of its allocation), 32-sample chunks through an
 * LDS-DMA ring, split over the samples with a workspace of dmnerf_gemm_tn_ws_floats(n_out, n_in, M) floats whose partials are added in
 * slice order (deterministic).  Replaces dmnerf_gemm's splits > 1 form + dmnerf_colsum on this path (those remain for operands whose
 * rows are not 16-byte aligned).  torch.autograd of nn.Linear in the reference: dm_nerf.py:66-83 layers under train_dmsr.py:62-64.   */
int64_t dmnerf_gemm_tn_ws_floats(int n_out, int n_in, int64_t M);
int dmnerf_gemm_tn(const float* d_dy, int64_t ldy, int64_t dy_floats, int n_out, const float* d_x, int64_t ldx, int64_t x_floats, int n_in,
                   int64_t M, float* d_dW, int64_t ldw, float* d_db, float* d_ws, int64_t ws_floats, void* stream);
/* The TRUNK of a narrow network (width 32 .. 160, a multiple of 32) as ONE launch in inference (csrc/gemm_chain.hip): the activations
 * of a 128-sample tile stay in LDS from layer to layer, the weights of all layers stream through an LDS ring.  Layer l: h_l = relu?(
 * [h_{l-1} if from_act | x if from_x] W_l^T + b_l) with d_B packed by dmnerf_pack_nt (range 0 = the `width` columns of h, range 1 = the
 * x_cols columns of the encoding; layer 0: from_x only), d_bias [width]; d_x = the row-padded encoding [M][ldx] of dmnerf_ray_embed,
 * d_out = the last layer's output [M][ldo].  d_x follows dmnerf_gemm_nt's A-operand contract: columns [0, 32 ceil(x_cols / 32)) of every
 * row are read, so ldx >= 32 ceil(x_cols / 32) (else DMNERF_E_ARG) and the columns past x_cols must be finite.  Sizes are checked before
 * the M = 0 return: n_layers in 1 .. DMNERF_CHAIN_MAX_LAYERS and n_layers x (width / 32) x 128 <= 8192 bytes of bias table.
 * dmnerf_mlp_chain_supported: whether (width, x_cols) fits the CU's LDS (the layer-count bounds are the caller's to check).          */
#define DMNERF_CHAIN_MAX_LAYERS 16
typedef struct dmnerf_chain_layer {
    const float* d_B;
    const float* d_bias;
    int ldb;          /* 32 x (width / 32 if from_act) + 32 x ceil(x_cols / 32) if from_x) */
    int from_act, from_x, relu;
} dmnerf_chain_layer;
int dmnerf_mlp_chain_supported(int width, int x_cols);
int dmnerf_mlp_chain(const float* d_x, int64_t ldx, int64_t x_floats, int x_cols, const dmnerf_chain_layer* layers, int n_layers,
                     int width, float* d_out, int64_t ldo, int64_t M, void* stream);
int dmnerf_copy_cols_pad(const float* d_src, int64_t ld_src, float* d_dst, int64_t ld_dst, int64_t M, int n, int n_pad, void* stream);
int dmnerf_ray_embed(const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S, int Lp, int Lv,
                     float* d_x_pos, int ldp, float* d_x_dir, int ldv, void* stream);

/* ---- EXTENSION: the optimizer update and the weight re-packing of a training step as two launches (csrc/optim.hip).
 * The reference steps torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr, betas=(0.9, 0.999))
 * (train_dmsr.py:124-125) after total_loss.backward() (:62-64); the drop-in path keeps exactly that.  These two entries are what
 * dm_nerf_amd.optim.FlatAdam runs instead when a caller opts in: at small per-rank batches the ~9 multi-tensor launches of the
 * torch optimizer and the 8 pack / cat launches after it are a measurable part of the step.
 *   dmnerf_adam_step: ONE pass over flat f32 vectors of n elements -- parameters, gradients (the gradient arena the
 *     weight-gradient kernels wrote), first and second moments -- applying torch.optim.Adam's update (amsgrad off, no weight
 *     decay) operation for operation, each rounded to f32 on its own, scalar factors formed in double:
 *       m <- m + (1-b1)(g - m);  v <- v b2;  v <- v + (1-b2)(g g);  p <- p + (-(lr / (1 - b1^t))) (m / (sqrt(v) / sqrt(1 - b2^t) + eps))
 *     The second-moment product is g * g FIRST, then scaled by (1-b2) (torch's multi-tensor form, _foreach_addcmul_): g * g is inf
 *     in f32 for |g| beyond about 1.8e19, v becomes inf and stays inf, m / inf = 0 -- that element's parameter stops moving from
 *     that step on, exactly as under torch.optim.Adam(foreach=True); single-tensor Adam forms (value * g) * g and stays finite.
 *     t = d_state2[0] + 1 is read on the device and stored back by the last workgroup to finish (d_state2[1] is its ticket
 *     counter; both start at 0): no host synchronisation, HIP-graph capturable.  d_lr (nullable): a device f32 scalar that
 *     overrides lr (a captured graph changes the learning rate by writing it).
 *   dmnerf_repack_train: for up to DMNERF_REPACK_MAX_MODELS models in one launch, from each model's (updated) flat parameter
 *     vector: d_flat_copy (nullable; dmnerf_param_count floats, must not alias the source), the forward blob (what
 *     dmnerf_pack_weights gathers with dmnerf_build_pack_index) and the W^T blob (dmnerf_build_pack_index_t over
 *     [parameters | F], F = A . rgb_feature_linear.weight formed inline with dmnerf_head_product's fmaf chain): bit-identical to
 *     dmnerf_head_product + two dmnerf_pack_weights calls.                                                                  */
#define DMNERF_REPACK_MAX_MODELS 4
typedef struct dmnerf_repack_model {
    const float* d_params_flat;
    int ins_num;
    float* d_flat_copy;
    const int32_t* d_idx;
    float* d_blob;
    const int32_t* d_idx_t;
    float* d_blob_t;
    const int32_t* d_f_pos;   /* nullable; 32768 entries: position in d_blob_t of F[i][j] (i * 256 + j), i.e. the inverse of d_idx_t on
                               * its entries >= dmnerf_param_count (each occurs once).  Given, F is formed in its natural order
                               * (coalesced) and scattered; NULL: every blob slot that holds an F element computes it itself. */
} dmnerf_repack_model;
int dmnerf_adam_step(float* d_params, const float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, int64_t n,
                     double lr, const float* d_lr, double beta1, double beta2, double eps, int64_t* d_state2, void* stream);
int dmnerf_repack_train(const dmnerf_repack_model* models, int n_models, void* stream);

/* ---- the iso-surface of the occupancy grid (tools/mesh_generator.py:68-104; csrc/surface.hip) -----------------------
 * d_occ [dx, dy, dz] f32 row-major, linear index p = (i dy + j) dz + k; every dimension >= 2 and dx dy dz < 2^31, checked with
 * the pointers before anything is launched (-1 and a message otherwise).  A point is inside iff v > level (NaN: outside).  The
 * classic 256-case Lorensen-Cline triangulation, degenerate triangles kept; winding of skimage's gradient_direction='ascent'.
 * dmnerf_surface_count: d_vcount [p] = crossing edges among the (up to) three that run from p along +i, +j, +k (0..3); d_tcount [p]
 *   = triangles of the cell whose lowest corner is p (0..5; 0 where p is on an upper border).  The caller forms the INCLUSIVE prefix
 *   sums d_vscan / d_tscan [p] int64 of the two (their last entries are V and F, the only values a host needs).
 * dmnerf_surface_emit: d_vertices [V, 3] f32 in index units, ordered by (owning point, axis): on the edge between a = occ[p] and b at
 *   the next point, i + t along that axis with t = (level - a) / (b - a) in f32.  d_faces [F, 3] int32, ordered by (cell, position
 *   in the case's table row); a vertex id is the owner's scan - count + the rank of the axis among the owner's crossing edges,
 *   recomputed from the grid.
 * dmnerf_surface_normals: d_normals [V, 3] = normalise(sum over the triangles at the vertex, in ascending triangle index, of
 *   (p1 - p0) x (p2 - p0)), every operation in f32, length sqrt((x x + y y) + z z); a zero sum stays 0.  d_inc_vertex [3 F] int32 is
 *   d_faces flattened and STABLY sorted, d_inc_slot [3 F] int64 the position in flattened d_faces of each sorted entry.
 * dmnerf_surface_clusters: two triangles are connected iff they share an unordered vertex pair.  d_edge_key [3 F] int64 sorted
 *   (min << 32 | max of the two ends of each triangle side), d_edge_slot [3 F] the side 3 f + s of each sorted entry; d_parent [F]
 *   int32 must hold 0..F-1 and d_count [F] zeros on entry.  d_rep [f] = the smallest triangle of f's cluster, d_count [r] = the
 *   size of the cluster that r represents (0 for a non-representative).  Integer atomics only; the result is order-independent.
 * dmnerf_surface_clean_mark: d_keep [f] = d_count[d_rep[f]] >= min_triangles, or with d_single (device int64, nullable) d_rep[f] ==
 *   *d_single; d_used [v] = 1 for every vertex of a kept triangle (d_used must be zero on entry).
 * dmnerf_surface_clean_compact: with the inclusive int32 prefix sums d_fscan / d_vscan of d_keep / d_used (Fk, Vk their totals),
 *   the kept triangles re-indexed and the used vertices with their normals, both in their original order; d_out_kept [Vk] int64 =
 *   the original index of every kept vertex.                                                                              */
int dmnerf_surface_count(const float* d_occ, int dx, int dy, int dz, float level, uint8_t* d_vcount, uint8_t* d_tcount, void* stream);
int dmnerf_surface_emit(const float* d_occ, int dx, int dy, int dz, float level, const uint8_t* d_vcount, const uint8_t* d_tcount,
                        const int64_t* d_vscan, const int64_t* d_tscan, int64_t V, int64_t F, float* d_vertices, int32_t* d_faces,
                        void* stream);
int dmnerf_surface_normals(const float* d_vertices, int64_t V, const int32_t* d_faces, int64_t F, const int32_t* d_inc_vertex,
                           const int64_t* d_inc_slot, float* d_normals, void* stream);
int dmnerf_surface_clusters(const int64_t* d_edge_key, const int64_t* d_edge_slot, int64_t F, int32_t* d_parent, int32_t* d_rep,
                            int32_t* d_count, void* stream);
int dmnerf_surface_clean_mark(const int32_t* d_faces, int64_t F, int64_t V, const int32_t* d_rep, const int32_t* d_count,
                              int min_triangles, const int64_t* d_single, uint8_t* d_keep, uint8_t* d_used, void* stream);
int dmnerf_surface_clean_compact(const float* d_vertices, const float* d_normals, const int32_t* d_faces, int64_t V, int64_t F,
                                 const uint8_t* d_keep, const uint8_t* d_used, const int32_t* d_fscan, const int32_t* d_vscan, int64_t Vk,
                                 int64_t Fk, float* d_out_vertices, float* d_out_normals, int32_t* d_out_faces, int64_t* d_out_kept,
                                 void* stream);

/* ---- one closed iso-surface per object of a label volume, in one pass (tools/mesh_generator.py:68 per object; csrc/object_surface.hip)
 * d_value [dx, dy, dz] f32 and d_labels [dx, dy, dz] uint8, row-major; every dimension >= 1.  label_mask: four host words, bit l set
 * = object l is meshed; a label >= C (1 .. DMNERF_MAX_LOGITS), 255 included, or one whose bit is clear owns nothing.  level must be
 * > 0 and finite (-1 otherwise).  The surface of object k is what dmnerf_surface_count / _emit give on the masked field M_k = value
 * where labels == k, else 0: the same inside rule, vertex formula, table, winding and order.  closed = 1: M_k is surrounded by one
 * layer of 0 points, so every mesh is watertight and coordinates lie in [-1, d]; the kernels then walk the EXTENDED grid of
 * (dx + 2) (dy + 2) (dz + 2) points, which (like dx dy dz with closed = 0) must stay below 2^31.  All per-point arrays below are over
 * that grid, p = (i Dy + j) Dz + k.
 * dmnerf_object_surface_count: d_vcount [p] = vertices on the (up to) three edges that run from p along +i, +j, +k over all objects
 *   (0..6: an edge between two inside points of different labels carries one per object); d_tcount [p] = triangles of the cell whose
 *   lowest corner is p over all objects (0..40).  The caller forms the INCLUSIVE int64 prefix sums d_vscan / d_tscan.
 * dmnerf_object_surface_emit: in grid order, per vertex d_vkey [V] int64 = (label << 40) | (3 p + axis), d_vpos [V, 3] f32 = the
 *   position in index units of the real grid (i + t, t = (level - a) / (b - a) on the masked operands, then - 1 with closed), d_vcell
 *   [V] int32 = the linear index in the real grid of the edge's end that is inside the object; per triangle d_tkey [F] int64 =
 *   (label << 40) | (5 p + position in the table row) and d_ckey [F, 3] int64 = the d_vkey of its three corners.  The keys are
 *   unique: sorting them gives the order (object, owning point, axis) / (object, cell, table position), and a corner's vertex id is
 *   the rank of its key among the sorted d_vkey.
 * dmnerf_object_surface_measures: per object k < C the area d_area [k] and the signed volume d_volume [k] in float64 of the
 *   triangles d_face_offset [k] .. d_face_offset [k + 1] (device int64 [C + 1]) of d_faces [F, 3] over d_vertices [V, 3], every
 *   coordinate first multiplied by the host doubles cell [3]: sum |(p1 - p0) x (p2 - p0)| / 2 and sum p0 . (p1 x p2) / 6.  One
 *   workgroup per object, a fixed summation order, no atomics: the same bits every run.
 * All three return the status as int32_t, as dmnerf_volume_edit does.                                                      */
int32_t dmnerf_object_surface_count(const float* d_value, const uint8_t* d_labels, int dx, int dy, int dz, int C, const uint32_t* label_mask,
                                float level, int closed, uint8_t* d_vcount, uint8_t* d_tcount, void* stream);
int32_t dmnerf_object_surface_emit(const float* d_value, const uint8_t* d_labels, int dx, int dy, int dz, int C, const uint32_t* label_mask,
                               float level, int closed, const uint8_t* d_vcount, const uint8_t* d_tcount, const int64_t* d_vscan,
                               const int64_t* d_tscan, int64_t V, int64_t F, int64_t* d_vkey, float* d_vpos, int32_t* d_vcell,
                               int64_t* d_tkey, int64_t* d_ckey, void* stream);
int32_t dmnerf_object_surface_measures(const float* d_vertices, int64_t V, const int32_t* d_faces, int64_t F, const int64_t* d_face_offset,
                                   int C, const double* cell, double* d_area, double* d_volume, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMNERF_HIP_H */
