/* libmvd_hip.so -- C ABI of the MI355X-native multi-view denoiser (Morphable Diffusion hot path).
 *
 * The reference has no FFI: its plug-in surface is Python (YAML ``target:`` classes + method signatures,
 * SURVEY.md section 8(b)).  This header is the boundary a binding for that surface talks to; each entry
 * point names the reference interface it replaces.  Plain pointers and sizes only, no torch types.
 * Device pointers are HIP device memory on the context's device; ``stream`` is a hipStream_t (NULL = the
 * default stream).  Tensors at the boundary use the reference's own layouts (NCHW / NCDHW, fp32).
 * All work of a call is ordered on ``stream``: mvd_denoise_views / mvd_unet_forward overlap part of it on one internal side
 * stream per context, forked from and joined back into ``stream`` with events inside the call (MVD_NO_SIDE_STREAM=1 in the
 * environment disables that).
 * Every function returns 0 on success, non-zero on failure; mvd_last_error() gives the text.
 * A context is thread-compatible (one thread at a time per context).  No allocation happens on the step
 * path: weights and the workspace are allocated at create / finalize / set_mesh time.
 */
#ifndef MVD_H
#define MVD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvd_ctx mvd_ctx;

/* kwargs of ldm.models.diffusion.attention.DepthWiseAttention (reference configs/facescape.yaml:28-42,
 * ctor ldm/modules/diffusionmodules/openaimodel.py:444-727, ldm/models/diffusion/attention.py:87-115) */
typedef struct {
  int image_size;       /* latent resolution (32) */
  int in_channels;      /* 8 */
  int out_channels;     /* 4 */
  int model_channels;   /* 320 */
  int num_res_blocks;   /* 2 */
  int channel_mult[4];  /* 1,2,4,4 */
  int num_heads;        /* 8 */
  int context_dim;      /* 768 */
  int volume_dims[4];   /* 64,128,256,512 */
  int attention_levels; /* bit i set: attention at downsample rate 2^i (attention_resolutions [4,2,1] -> 0x7) */
} mvd_unet_config;

/* SpatialVolumeNet ctor (ldm/models/diffusion/morphable_diffusion.py:152-180) */
typedef struct {
  int time_dim;             /* 256 */
  int view_dim;             /* 4 */
  int num_views;            /* N: SMPLFeatureExtractor.num_views (hard-coded 16 in the reference) */
  int input_image_size;     /* 256 */
  int frustum_volume_depth; /* 48 */
  int spatial_volume_size;  /* 32 */
  float spatial_volume_length; /* 0.5 */
  float frustum_volume_length; /* 0.86603 */
  int projection;           /* 0 perspective, 1 orthographic */
  int frustum_dims[4];      /* 64,128,256,512 */
  float voxel_size;         /* 0.005 */
} mvd_volume_config;

int mvd_create(const mvd_unet_config* ucfg, const mvd_volume_config* vcfg, int device, size_t workspace_bytes,
               mvd_ctx** out);
void mvd_destroy(mvd_ctx* ctx);
const char* mvd_last_error(void);
/* "f16" (libmvd_hip.so) or "bf16" (libmvd_hip_bf16.so: the same sources built with bfloat16 MFMA operands and storage, the
 * training dtype BASELINE configs[3] names; the reference trainer's `precision` key, configs/facescape.yaml:65). */
const char* mvd_compute_dtype(void);

/* Replaces load_state_dict (reference generate_face.py:75-76): one call per state_dict entry, keyed by the
 * reference's own names.  data is fp32, contiguous, reference layout; on_device
 * selects device or host memory.  Unknown keys (VAE, CLIP, schedule buffers) are ignored and return 0. */
int mvd_upload_weight(mvd_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim, int on_device);
/* Numerical policy, to be set before mvd_finalize_weights.  MFMA operands are fp16 (11 significand bits: ~4e-4 relative
 * error per GEMM output); the layers whose error reaches the UNet output almost undamped run in EXTENDED precision: both
 * operands split into fp16 hi + lo parts, three products accumulated in fp32 (a_hi w_hi + a_lo w_hi + a_hi w_lo).
 * level 0: none.  1: output conv + conv_in.  2: + the cheap layers (skip conv, transformer proj_in / proj_out, DepthTransformer)
 * of the last output block.  3 (default since round 6): + the same layers of the block before it.  4: + the last block's ResBlock
 * 3x3 convs.  5: all such layers of every full-resolution output block.  6: + of the full-resolution input blocks.  The ladder is
 * ordered by error removed per unit of time (until round 5 levels 3 and 4 added these two steps in the other order and the
 * default was 2).  Measured guided-eps error of the full step against the fp32 reference and step time (DESIGN.md section 2,
 * profiles/r06_k_xp_levels.txt): level 2 7.3-8.4e-4, level 4 6.0-7.1e-4 at +3.6 %; level 3 sits between at +1.2 %. */
int mvd_set_precision_level(mvd_ctx* ctx, int level);
/* First-stage model (mvd_vae_decode / mvd_vae_encode), to be set before mvd_finalize_weights.  0 (default): fp16 MFMA operands
 * like the UNet -- ~30 convolutions in series leave 1.8-2.0e-3 relative L2 in the decoded image (at most 0.8 of an 8-bit step).
 * 1 ("exact"): every convolution, the attention projections and both attention products run in extended precision (fp16 hi + lo
 * operand split, three products accumulated in fp32): the reference's fp32 result to ~1e-5, at about three times the cost. */
int mvd_set_vae_precision(mvd_ctx* ctx, int exact);
/* Packs/folds the uploaded tensors into their MFMA layouts; fails (listing the key) if one is missing. */
int mvd_finalize_weights(mvd_ctx* ctx);

/* DepthWiseAttention.forward(x, timesteps, context, source_dict) -- ldm/models/diffusion/attention.py:117-138.
 * x [Bv,in_channels,s,s]; timesteps [Bv] int64; context [Bv,1,context_dim]; src{32,16,8,4}: the source_dict
 * volumes [n_ctx,C_l,D_l,s_l,s_l] fp32 for the FIRST n_ctx samples, the remaining Bv-n_ctx samples are
 * treated as all-zero volumes (the classifier-free-guidance half, morphable_diffusion.py:137-139);
 * depth0 = D of the finest level (48); out [Bv,out_channels,s,s]. */
int mvd_unet_forward(mvd_ctx* ctx, const float* x, const int64_t* timesteps, const float* context, int Bv, int n_ctx,
                     const float* src0, const float* src1, const float* src2, const float* src3, int depth0, float* out,
                     void* stream);
/* ONE block of DepthWiseAttention on its own input, through the production block code (same plans and kernels as
 * mvd_unet_forward): `path` is the reference module path below model.diffusion_model --
 *   "input_blocks.I.J" / "middle_block.J" / "output_blocks.I.J": ResBlock._forward (openaimodel.py:256-276; needs timesteps [B]),
 *      SpatialTransformer.forward (modules/attention.py:325-336; needs context [B,1,context_dim]), Downsample / Upsample /
 *      the input convolution (openaimodel.py:100-157);
 *   "middle_conditions" / "output_conditions.K": DepthTransformer.forward (ldm/models/diffusion/attention.py:78-84; needs
 *      volume [n_ctx,C_l,D,H,W] for the FIRST n_ctx samples; the remaining B - n_ctx samples are context-free (all-zero volumes,
 *      the classifier-free-guidance half, as in mvd_unet_forward) and take the production forms of that case: x + K, or with
 *      MVD_NO_COND_CONST=1 the relu(beta) fill rows.  n_ctx == 0: volume may be NULL).  Other blocks ignore n_ctx.
 * x [B,C,H,W] at a UNet resolution (image_size >> level); out receives [B,Cout,Ho,Wo] (at most out_capacity floats) and
 * out_shape[4] its shape.  Used by the block-level parity tests. */
int mvd_unet_block(mvd_ctx* ctx, const char* path, const float* x, int B, int C, int H, int W, const int64_t* timesteps,
                   const float* context, const float* volume, int D, int n_ctx, float* out, int out_capacity, int* out_shape,
                   void* stream);


/* SyncMultiviewDiffusion.embed_time -- morphable_diffusion.py:491-494. t [B] int64 -> out [B,time_dim] */
int mvd_embed_time(mvd_ctx* ctx, const int64_t* t, int B, float* out, void* stream);

/* Step-invariant per-sample metadata (batch dict, generate_face.py:227-241), HOST pointers:
 * vertices [Nv,3] fp32 (+-0.5 cube frame), coord [Nv,3] int32 (z,y,x), out_sh [3] int32, bounds [2,3] fp32.
 * Builds the sparse-convolution neighbour tables (replaces spconv's indice generation, morphable_diffusion.py:245-254).
 * Transactional: on failure the previously set mesh stays active and intact. */
int mvd_set_mesh(mvd_ctx* ctx, const float* vertices, const int32_t* coord, const int32_t* out_sh, const float* bounds,
                 int Nv);
/* A context keeps up to 64 independent sets of per-sample tables (mesh + cameras): mvd_select_sample makes set `slot` the
 * active one -- mvd_set_mesh / mvd_set_cameras write it, the stage calls read it.  A batch of B samples (the reference's
 * ``for bi in range(B)`` loop, morphable_diffusion.py:245) uploads each sample's tables once and switches between them at
 * every step instead of rebuilding them.  Slot 0 is active after mvd_create. */
int mvd_select_sample(mvd_ctx* ctx, int slot);
/* target_K [N,4,4], target_RT [N,3,4] fp32 HOST pointers (batch['target_K'], batch['target_RT']) */
int mvd_set_cameras(mvd_ctx* ctx, const float* K, const float* RT, int N);
/* The same two uploads in the order of `stream`, for callers whose mesh changes at every step (a training step sees a new
 * batch, generate_face.py one mesh per trajectory): the host pointers are read before the call returns, the tables go to the
 * device as ONE copy enqueued on `stream` -- launches enqueued on `stream` earlier keep reading the previous tables, later
 * ones read the new tables; nothing is allocated and nothing synchronises once the slot's pools have grown to the mesh size.
 * All launches of this context that read the slot must be on `stream` (or ordered after it by the caller). */
int mvd_set_mesh_async(mvd_ctx* ctx, const float* vertices, const int32_t* coord, const int32_t* out_sh, const float* bounds,
                       int Nv, void* stream);
int mvd_set_cameras_async(mvd_ctx* ctx, const float* K, const float* RT, int N, void* stream);
/* A whole batch at once (the reference's ``for bi in range(B)`` loop over a NEW batch, morphable_diffusion.py:245-254: spconv
 * regenerates its indices for every sample at every call): sample i's mesh and cameras go to slot slots[i] (distinct). The B
 * rule books are built on B host threads, every sample is validated before the first table is replaced, the uploads are
 * enqueued on `stream` as in the two calls above.  The active slot is unchanged on return. */
int mvd_set_samples_async(mvd_ctx* ctx, int B, const int* slots, const float* const* vertices, const int32_t* const* coord,
                          const int32_t* const* out_sh, const float* const* bounds, const int* Nv, const float* const* K,
                          const float* const* RT, int N, void* stream);
/* Host-only view of the rule book (no context, no GPU: used by the CPU tests): builds the tables of one mesh on the calling
 * thread -- n_sites[3] active sites per level, lens[6] = ints in nbr_subm[0..2] ([n_sites][27], -1 = inactive), nbr_down[0..1]
 * ([n_sites of the next level][27]) and the coarse index grid -- and mvd_rulebook_table copies table `which` (0..5) of that
 * build.  force_hash != 0 takes the open-addressing path that grids of more than 2^25 cells use. */
int mvd_rulebook_build(const int32_t* coord, const int32_t* out_sh, int Nv, int force_hash, int32_t* n_sites, int64_t* lens);
int mvd_rulebook_table(int which, int32_t* out);

/* First half of SpatialVolumeNet.construct_spatial_volume (morphable_diffusion.py:203-231) for the views
 * view_idx[0..n_local): x_noisy [n_local,4,s,s], t_embed [time_dim], v_embed [n_local,view_dim];
 * fused_out [Nv,16] = this rank's share of conv0(mean over ALL num_views views); with add_bias != 0 the
 * conv bias is included (exactly one rank adds it).  Summing fused_out over ranks gives the full tensor. */
int mvd_vertex_features(mvd_ctx* ctx, const float* x_noisy, const float* t_embed, const float* v_embed,
                        const int32_t* view_idx, int n_local, int add_bias, float* fused_out, void* stream);
/* The same stage split for the exact view exchange ("equivalently an all-gather of [N,16,Nv] if bit-exact
 * view-order summation is wanted"): mvd_vertex_view_features writes the per-view features vf_out [n_local,Nv,16]
 * (morphable_diffusion.py:203-229) without reducing them; after the ranks' slices are gathered in view order,
 * mvd_fuse_vertex_features applies SMPLFeatureExtractor (network.py:41-72) to vf_all [num_views,Nv,16] -> fused_out
 * [Nv,16].  Summation runs over the views in index order, so a sharded step is bit-identical to the single-GPU one. */
int mvd_vertex_view_features(mvd_ctx* ctx, const float* x_noisy, const float* t_embed, const float* v_embed,
                             const int32_t* view_idx, int n_local, float* vf_out, void* stream);
int mvd_fuse_vertex_features(mvd_ctx* ctx, const float* vf_all, int n_views, float* fused_out, void* stream);
/* 1 when mvd_vertex_view_features touches no memory of the context's shared workspace (the 2-D encoder runs as its one-launch
 * form out of a scratch of its own): the call may then be enqueued on the caller's communication stream WHILE mvd_denoise_views of
 * the same context runs on another stream -- the sampler moves the step's head (encoder, vertex gather, exchange, sparse CNN) off
 * the UNet's stream entirely.  0: keep it on the stream the UNet is launched on (64 x 64 latents, MVD_NO_FUSED_ENC). */
int mvd_vertex_features_stream_safe(mvd_ctx* ctx);
/* Stage probes for the parity tests (each stage of the conditioner on its own, in the reference's layouts):
 *   mvd_stage_target_encoder   NoisyTargetViewEncoder.forward (ldm/models/diffusion/network.py:181-207) for n_local views of one
 *                              sample: x_noisy [n_local,4,s,s], t_embed [time_dim], v_embed [n_local,view_dim] -> feats [n_local,16,s,s];
 *   mvd_stage_sparse_dense     SparseConvNet.forward(...) (network.py:74-96, the xyzc_net call of morphable_diffusion.py:253-254):
 *                              fused [Nv,16] -> dense [C,d,h,w] of the coarsest level (spconv's .dense(), batch 1); train_mode != 0
 *                              uses batch statistics in the BatchNorm1d layers.  shape_out (may be NULL) receives {C,d,h,w};
 *                              dense_out == NULL only queries the shape. */
int mvd_stage_target_encoder(mvd_ctx* ctx, const float* x_noisy, const float* t_embed, const float* v_embed, int n_local,
                             float* feats, void* stream);
int mvd_stage_sparse_dense(mvd_ctx* ctx, const float* fused, int train_mode, float* dense_out, int32_t* shape_out, void* stream);
/* use_spatial_volume=True (morphable_diffusion.py:197-225,259-261; SpatialTime3DNet network.py:235-283).
 *   mvd_spatial_time_volume  NoisyTargetViewEncoder of ALL num_views views of the active sample slot -> dense unprojection onto
 *                            the V^3 lattice -> SpatialTime3DNet; the result is ADDED into the slot's volume (call it after
 *                            mvd_volume_from_fused of the same slot, on the same stream) and, when volume_out is not NULL, the
 *                            network's own output [64,V,V,V] (before the add, reference layout) is written there.
 *                            x_noisy [n_views,4,s,s], t_embed [time_dim], v_embed [n_views,view_dim]; n_views must equal
 *                            num_views.  The stage runs out of an arena of its own (sized at mvd_finalize_weights): no
 *                            allocation, and no use of the shared workspace.  Errors: switch off, weights not finalized,
 *                            mvd_set_mesh / mvd_set_cameras not called, wrong view count.
 *   mvd_stage_unproject      parity probe of the unprojection alone: feats [n_views,16,s,s] -> out [n_views*16,V,V,V] (view-major,
 *                            the reference's layout; values as the fp16 operand holds them). */
/* The switch itself: mvd_volume_config keeps its layout (existing callers pass it unchanged), the two new settings arrive
 * through a setter, like the precision level -- after mvd_create, before the first mvd_upload_weight.  use != 0 turns the stage
 * on; spatial_dims (NULL: 64,128,256,512) are SpatialTime3DNet's widths.  Checked: spatial_dims[0] == 64 (the volume's channel
 * count), every dim a positive multiple of 8, spatial_volume_size % 8 == 0 (three stride-2 levels). */
int mvd_set_spatial_volume(mvd_ctx* ctx, int use, const int* spatial_dims);
int mvd_spatial_time_volume(mvd_ctx* ctx, const float* x_noisy, const float* t_embed, const float* v_embed, int n_views,
                            float* volume_out, void* stream);
int mvd_stage_unproject(mvd_ctx* ctx, const float* feats, int n_views, float* out, void* stream);
/* The view-sharded step's ONE collective behind the C ABI (replaces nothing in the reference, whose sampler
 * is single-GPU: ldm/models/diffusion/morphable_diffusion.py:701-739).  Rank g owns views [g N/G, (g+1) N/G); every step each
 * rank computes the per-view vertex features of its views (mvd_vertex_view_features) and ALL-GATHERS them, so that every rank
 * sums the N views in index order (mvd_fuse_vertex_features): bit-identical to the single-GPU step.
 *   mvd_comm_unique_id : one rank creates the RCCL id (128 bytes) and hands it to the others over any side channel
 *   mvd_comm_init      : collective; creates the communicator this context owns (librccl.so is opened on first use)
 *   mvd_exchange_view_features : ncclAllGather of [n_local][Nv][16] fp32 from `local` into `all` ([N][Nv][16], rank r's slice
 *                        at views [r n_local, (r+1) n_local)) on `stream` -- no Python and no torch.distributed on the step path
 *   mvd_comm_destroy   : also done by mvd_destroy */
typedef struct { char internal[128]; } mvd_rccl_id;
int mvd_comm_unique_id(mvd_rccl_id* id_out);
int mvd_comm_init(mvd_ctx* ctx, const mvd_rccl_id* id, int rank, int world);
int mvd_comm_destroy(mvd_ctx* ctx);
int mvd_exchange_view_features(mvd_ctx* ctx, const float* local, float* all, int n_local, void* stream);
/* In-place sum all-reduce of `count` device floats over the context's communicator on `stream` (ncclAllReduce): the
 * "all_reduce" form of the step's exchange (321 KB of per-vertex sums) and the building block of the gradient
 * averaging below. */
int mvd_comm_all_reduce(mvd_ctx* ctx, float* buf, size_t count, void* stream);
/* Cross-stream hand-over of the volume.  The exchange + mvd_fuse_vertex_features + mvd_volume_from_fused may run on a
 * communication stream of the caller while `stream` of mvd_denoise_views already executes the UNet's input blocks (which
 * need none of it): record a hipEvent_t after mvd_volume_from_fused on that stream and register it here; every later reader
 * of the volume inside the library (the frustum stage of mvd_denoise_views / mvd_frustum_volumes) makes ITS stream wait for
 * the event before the first read.  The event is caller-owned and must stay alive while registered; NULL unregisters. */
int mvd_set_volume_ready_event(mvd_ctx* ctx, void* event);
/* Second half (morphable_diffusion.py:232-257): sparse voxel CNN + lattice gather. fused [Nv,16] ->
 * volume_out [64,V,V,V] (reference layout, may be NULL); the result is also kept in the context for
 * mvd_frustum_volumes / mvd_denoise_views. */
int mvd_volume_from_fused(mvd_ctx* ctx, const float* fused, float* volume_out, void* stream);

/* Training-step variants (reference training_step morphable_diffusion.py:520-549).  The Lightning module
 * is in train mode there, so the sparse CNN's BatchNorm1d layers (network.py:105) normalise with the statistics of the
 * sample's active rows instead of their running buffers: mvd_volume_from_fused_train is mvd_volume_from_fused with that
 * behaviour.  mvd_mse_loss: out[0] = mean((a - b)^2) over n device floats (the "loss_simple" of :541-542). */
int mvd_volume_from_fused_train(mvd_ctx* ctx, const float* fused, float* volume_out, void* stream);
int mvd_mse_loss(mvd_ctx* ctx, const float* a, const float* b, size_t n, float* out, void* stream);
/* Training step of the UNet (reference training_step morphable_diffusion.py:520-549 from `self.model(...)`
 * on, loss.backward(), configure_optimizers :627-646).
 *   mvd_train_enable(ctx, 1)        BEFORE mvd_finalize_weights: the uploaded fp32 tensors of model.diffusion_model.* /
 *                                   spatial_volume.* / time_embed.* are kept as master parameters in ONE flat arena (sorted by
 *                                   key, each tensor aligned to 64 floats); gradients and Adam moments use the same layout.
 *   mvd_train_param_count / _info   enumerate the parameters: name (state_dict key), offset and numel in the arena (floats),
 *                                   shape (up to 8 dims) -- what nn.Module.named_parameters() is to the reference.
 *   mvd_train_arena_size            floats per arena.
 *   mvd_train_adopt_arena(which, ptr, numel)   moves arena `which` (0 parameters, 1 gradients, 2 / 3 Adam moments, 4 EMA) into
 *                                   caller-owned device memory of the same size (its content is copied over, a not yet
 *                                   existing arena is zeroed): the caller's tensor framework then sees parameters / gradients
 *                                   as views of ONE buffer (one RCCL all-reduce for the DDP gradient averaging of
 *                                   train_morphable_diffusion.py:302-303).  The memory must outlive the context.
 *   mvd_train_zero_grad             optimizer.zero_grad().
 *   mvd_train_unet_step             x [B,in_channels,s,s], timesteps [B], context [B,1,context_dim], src{0..3} the
 *                                   source_dict volumes [B,C_l,D_l,s_l,s_l] (after the condition dropout), target [B,out,s,s]:
 *                                   pred = UNet(x, ...), loss = mean((target - pred)^2) (morphable_diffusion.py:541-542), then
 *                                   dL/dpred * loss_scale is back-propagated through every block; parameter gradients are
 *                                   ACCUMULATED (x loss_scale) into the gradient arena.  dsrc{0..3} (each may be NULL) receive
 *                                   the gradient w.r.t. the volumes (x loss_scale).  recompute != 0: activation checkpointing
 *                                   per block (ldm/modules/diffusionmodules/util.py:102-148 -- only block inputs are kept, a
 *                                   block is re-run before its backward); 0 keeps every intermediate of the forward pass.
 *                                   fp16 MFMA operands, fp32 accumulation / master weights; pick loss_scale so that the scaled
 *                                   gradients stay inside the fp16 range (mvd_train_adamw_step reports overflow).
 *   mvd_train_get_grad              copy of one parameter's gradient (PyTorch layout), still multiplied by the loss scale(s).
 *   mvd_train_adamw_step            torch.optim.AdamW on the arena: the UNet group (all of model.diffusion_model.* when
 *                                   finetune_unet != 0, else the DepthTransformers of attention.py:140-142) at `lr`,
 *                                   time_embed.* and spatial_volume.* at `lr_aux` (the reference: 10 lr); gradients are
 *                                   multiplied by inv_scale first.  `step` counts from 1.  If any gradient is inf / nan the
 *                                   whole update is skipped (*skipped_out = 1; reading it back synchronises the stream; NULL
 *                                   = no read-back).  A group no backward call has written to since the last
 *                                   mvd_train_zero_grad is left alone -- parameters AND moments -- as torch.optim.AdamW skips
 *                                   parameters whose .grad is None (e.g. spatial_volume.* when only mvd_train_unet_step ran).
 *                                   With inv_scale == 1 (no loss scaling: the bfloat16 build) the overflow
 *                                   check is not run -- torch.optim.AdamW's own behaviour -- and *skipped_out stays 0.
 *   mvd_train_repack                after the parameters changed: re-derive every packed fp16 weight in place.
 * Gradient clipping by global norm (Lightning's gradient_clip_val / clip_grad_norm_) and EMA weights (LDM's LitEma), fused into
 * the optimiser step:
 *   mvd_train_adopt_arena(4, ...)   the EMA arena; one that does not exist yet starts as a COPY of the parameter arena (LitEma's
 *                                   initial shadow), not zeroed.
 *   mvd_train_grad_norm             norm_out (device, 1 float) = || inv_scale * g || over exactly the ranges mvd_train_adamw_step
 *                                   would update (same groups, same untouched-group rule; clip_grad_norm_ likewise ignores
 *                                   parameters without a gradient).  Two-stage sum without atomics on a grid that depends only
 *                                   on the range lengths: bit-reproducible.
 *   mvd_train_adamw_step_ex         mvd_train_adamw_step plus: max_grad_norm > 0 multiplies the un-scaled gradients by
 *                                   min(1, max_grad_norm / (norm + 1e-6)) (<= 0: no clipping); ema_decay >= 0 applies
 *                                   e -= (1 - ema_decay) (e - p_new) on the EMA arena (created on first use; < 0: no EMA; the
 *                                   caller computes LitEma's warm-up, ema_decay is THIS step's decay); grad_norm_out (HOST, may
 *                                   be NULL) receives the norm.  Reading skipped_out or grad_norm_out back synchronises the
 *                                   stream; with both NULL the call does not.  With inv_scale != 1 the norm pass doubles as the
 *                                   overflow check: a non-finite norm skips the step -- parameters, moments and EMA untouched,
 *                                   *skipped_out = 1.  With inv_scale == 1 nothing is special-cased, as in torch.  The norm pass
 *                                   runs only when clipping, loss scaling or grad_norm_out asks for it.
 *   mvd_train_last_grad_norm        norm_out (device, 1 float) = the norm of the last mvd_train_adamw_step_ex /
 *                                   mvd_train_grad_norm pass, copied in stream order: no synchronisation.
 *   mvd_train_ema_swap              exchanges the parameter arena and the EMA arena in place (sampling / validating from the
 *                                   averaged weights); the caller re-packs afterwards, and swaps back the same way. */
int mvd_train_enable(mvd_ctx* ctx, int on);
int mvd_train_param_count(mvd_ctx* ctx);
int mvd_train_param_info(mvd_ctx* ctx, int index, char* name, size_t name_cap, int64_t* offset, int64_t* numel, int64_t* shape,
                         int* ndim);
int64_t mvd_train_arena_size(mvd_ctx* ctx);
int mvd_train_adopt_arena(mvd_ctx* ctx, int which, float* ptr, int64_t numel);
int mvd_train_zero_grad(mvd_ctx* ctx, void* stream);
int mvd_train_unet_step(mvd_ctx* ctx, const float* x, const int64_t* timesteps, const float* context, int B, const float* src0,
                        const float* src1, const float* src2, const float* src3, int depth0, const float* target, float loss_scale,
                        int recompute, float* pred_out, float* loss_out, float* dsrc0, float* dsrc1, float* dsrc2, float* dsrc3,
                        void* stream);
/* Loss options of the training step (not in the reference, whose objective is the plain mean above): sample weights (Min-SNR),
 * a pixel weight (foreground mask), a Huber branch, and per-sample read-outs.  With d = pred - target in fp32:
 *     rho(d) = d^2,  rho'(d) = 2 d                                        loss_type 0 (l2), and 1 (huber) where |d| <= huber_delta
 *     rho(d) = 2 delta |d| - delta^2,  rho'(d) = 2 delta sign(d)          loss_type 1 where |d| > huber_delta
 *   (twice torch's huber_loss, so that it IS l2 inside the threshold; |d| == delta takes the quadratic branch)
 *     a_b   = sum_hw m[b,h,w]                                             m = pixel_w >= 0, NULL = 1
 *     l_b   = sum_{c,h,w} m[b,h,w] rho(d[b,c,h,w]) / (C a_b)              a_b == 0: l_b = 0 and the sample's gradient is exactly 0
 *     L     = (1/B) sum_b w_b l_b                                         w = sample_w, NULL = 1; all NULL and l2: mean(d^2)
 *     dpred = c_b m[b,h,w] rho'(d)/2,  c_b = ((2 loss_scale) w_b) / ((float)(B C) a_b)   in fp32, in this order: a power-of-two
 *                                                                         change of w or loss_scale changes dpred exactly
 *     mse_b = mean_{c,h,w} d^2                                            unweighted, unmasked: what is logged / validated on
 * One fused kernel between an area pass (only with pixel_w) and a finalise launch (csrc/k_loss.hip): pred and target are read
 * once, sums are double partials combined in an order that depends on (B, HW, C) alone, no atomics -- two calls agree bit for bit.
 * Negative or non-finite weights are NOT checked (the weights live on the device): they give what the formulas give.
 *   mvd_train_unet_step_ex   mvd_train_unet_step with that loss stage.  sample_w [B], pixel_w [B,1,s,s] (device, either may be
 *                            NULL); loss_out receives L; loss_per_sample / mse_per_sample (device, B floats, either may be NULL)
 *                            receive l_b / mse_b.  loss_type outside {0, 1}, or huber_delta <= 0 with huber, is an error and
 *                            launches nothing.  mvd_train_unet_step itself is unchanged and keeps its own two loss kernels.
 *   mvd_op_train_loss        the loss stage alone on raw channels-last device buffers, no context: pred / target [B,HW,C],
 *                            pixel_w [B,HW], dpred [B,HW,C] (NULL: forward only -- the held-out loss), loss_out (1 float, may be
 *                            NULL).  The parity hook of the stage.  Synchronises the stream (its scratch lives for the call). */
int mvd_train_unet_step_ex(mvd_ctx* ctx, const float* x, const int64_t* timesteps, const float* context, int B, const float* src0,
                           const float* src1, const float* src2, const float* src3, int depth0, const float* target, float loss_scale,
                           int recompute, const float* sample_w, const float* pixel_w, int loss_type, float huber_delta,
                           float* pred_out, float* loss_out, float* loss_per_sample, float* mse_per_sample, float* dsrc0, float* dsrc1,
                           float* dsrc2, float* dsrc3, void* stream);
int mvd_op_train_loss(const float* pred, const float* target, int B, int HW, int C, const float* sample_w, const float* pixel_w,
                      int loss_type, float huber_delta, float loss_scale, float* dpred, float* loss_out, float* loss_per_sample,
                      float* mse_per_sample, void* stream);
/* 2-D image metrics of generated views against captured views (SSIM, squared / absolute error) under the reference's evaluation
 * protocol: 8-bit images, skimage's structural_similarity at its uint8 defaults.  No context; one fused kernel and a finalise
 * launch (csrc/k_metrics.hip), no atomics, every order of summation a function of (V, H, W) alone: two calls agree bit for bit.
 *   pixel values  a float image in [-1, 1] is quantised q = trunc(((clamp(x, -1, 1) + 1) * 0.5) * 255), every step in fp32 in
 *                 that order (batch.views_to_uint8's bytes); a uint8 image is taken as it is.
 *   background    where a pixel is background the PREDICTED pixel becomes 255 in all three channels, the target stays (the
 *                 ground truth was composited on white).  mask_mode 0: none; 1: mask [V,H,W] uint8, nonzero = background;
 *                 2: derived from the target -- background iff all three quantised target channels are >= 254.
 *   ssim          per channel, 7 x 7 uniform window, K1 = 0.01, K2 = 0.03, L = 255, C1 = (K1 L)^2, C2 = (K2 L)^2, sample
 *                 (co)variances (normalised by 49/48):  S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),
 *                 averaged over the window centres whose window lies inside the image (rows 3..H-4, columns 3..W-4), then over
 *                 the three channels.  The five window sums are exact integers; only S is evaluated, in fp64.
 *   sse, sae      sums of (p - t)^2 and |p - t| over all 3 H W quantised values after the background rule: exact integers.
 *   non-finite    NaNs and infinities of a float image are counted per view; a view with any reports NaN for ssim, sse, sae and the
 *                 background count, so that nothing derived from them is a plausible number.
 * pred / target: device pointers; dtype 0 = float32, 1 = uint8; layout 0 = [V,3,H,W], 1 = [V,H,W,3] (the two may differ in
 * both).  out: device, [V][5] doubles = ssim, sse, sae, background pixels, non-finite values.  Null pred / target / out,
 * H < 7, W < 7, V < 1, V > 65535, V H W 3 >= 2^31, an unknown dtype / layout / mode, or mode 1 without a mask are errors and
 * launch nothing.  Synchronises the stream (its scratch lives for the call). */
int mvd_op_image_metrics(const void* pred, int pred_dtype, int pred_layout, const void* target, int target_dtype, int target_layout,
                         const unsigned char* mask, int mask_mode, int V, int H, int W, double* out, void* stream);
/* Mesh texturing from generated views (csrc/k_mesh.hip): an exact visibility rasteriser of the conditioning mesh into the N target
 * cameras and a per-vertex fusion of the view colours under that visibility.  No context; device pointers; each call
 * synchronises the stream (the rasteriser's scratch lives for the call).  Everything downstream of the projection is integer
 * arithmetic, defined here so that it can be reproduced exactly.
 *   constants     SUB = 4: screen coordinates are int32 in 1/16 pixel; KMAX = 2^24 - 1; guard band |u|, |v| <= 4096 px.  These
 *                 keep every edge function within 2^35 and every key interpolation within 2^59 in int64.
 *   mvd_op_mesh_project   one thread per (view, vertex), fp32: cam = R x + t (RT [N,3,4], world -> camera),
 *                 u = (K00 X + K01 Y) / Z + K02, v = K11 Y / Z + K12 (K [N,3,3]); pixel (i, j) has its centre at (u, v) = (j, i),
 *                 the conditioner's convention.  xy [N,Nv,2] = rint(16 u), rint(16 v); key [N,Nv] = clamp(rint(z_near / Z KMAX),
 *                 1, KMAX): a larger key is nearer, and z_near / Z is linear in screen space, so that integer interpolation of
 *                 keys orders depth correctly.  key = 0 (and xy = 0) marks an invalid vertex: Z < z_near, a non-finite value, or
 *                 a point outside the guard band.
 *   mvd_op_mesh_raster    faces [Nf,3] int32.  A face is skipped in a view if one of its vertices is invalid there (key outside
 *                 1..KMAX or a coordinate beyond the guard band, whoever produced them), if one of its indices is outside
 *                 [0, Nv) -- never dereferenced, and counted once per face into *bad_faces (one device int) -- or if
 *                 A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) is zero.  A < 0: vertices 1 and 2 are swapped (both windings are
 *                 drawn).  Edge functions: for k = 0, 1, 2 with a = v[(k+1)%3], b = v[(k+2)%3], dx = bx - ax, dy = by - ay,
 *                 e_k(p) = dx (py - ay) - dy (px - ax) at p = (16 j, 16 i).  Pixel (i, j) is covered iff for every k: e_k > 0, or
 *                 e_k == 0 and the edge is owned (dy < 0, or dy == 0 and dx > 0) -- a shared edge belongs to exactly one of
 *                 its two faces.  Pixel key = (e_0 key_0 + e_1 key_1 + e_2 key_2) / A, int64, truncating.  Winner per pixel: the
 *                 largest key, ties to the smallest face index, independent of arrival order (a 64-bit atomic maximum of
 *                 (key << 32) | (0xFFFFFFFF - f), then a resolve launch).  face_id [N,H,W]: -1 background; pix_key [N,H,W]:
 *                 0 background.  Bounding boxes are clamped to the image before any loop.
 *   mvd_op_mesh_vertex_colors   one thread per vertex, views in index order.  Nearest pixel pj = (xs + 8) >> 4,
 *                 pi = (ys + 8) >> 4.  The vertex is visible in view n iff it is valid there, that pixel is inside the image and
 *                 covered, and the winning face there has the vertex as a corner or key_v + bias >= pix_key.  Weight
 *                 w_n = max(0, cos)^power (two_sided: |cos|^power), cos between the vertex normal (normals [Nv,3], any length)
 *                 and the direction from the vertex (verts [Nv,3]) to the camera centre (centres [N,3]); a zero normal weighs 0.
 *                 Colour of a view: bilinear, clamp to edge, sampled at the SNAPPED position (xs / 16, ys / 16); images are
 *                 dtype 0 float32 in [-1, 1] mapped (clamp + 1) / 2, or 1 uint8 / 255; layout 0 [N,3,H,W], 1 [N,H,W,3].
 *                 color [Nv,3] = sum w c / sum w; weight_sum [Nv]; n_seen [Nv] = views passing the integer visibility test,
 *                 whatever their weight; spread [Nv] = sqrt(sum_n w_n mean_c (c_n - color)^2 / sum w) from a second pass over
 *                 the views; visible [N,Nv] bytes (may be NULL): the visibility test per view.  sum w == 0: the fill colour and
 *                 a NaN spread.  fp32 in a fixed order, no floating-point atomics: two calls agree bit for bit.
 * Errors, which launch nothing: a null pointer (but visible); N < 1, Nv < 1, Nf < 1; H or W < 1 or > 4096; N H W >= 2^31;
 * z_near <= 0 or non-finite; power < 1; an unknown dtype or layout; N > 65535, N Nv >= 2^30.
 * UV texture atlases and perspective-correct rendering: the next block. */
int mvd_op_mesh_project(const float* verts, const float* K, const float* RT, int N, int Nv, float z_near, int32_t* xy, int32_t* key,
                        void* stream);
int mvd_op_mesh_raster(const int32_t* xy, const int32_t* key, const int32_t* faces, int N, int Nv, int Nf, int H, int W, int32_t* face_id,
                       int32_t* pix_key, int32_t* bad_faces, void* stream);
int mvd_op_mesh_vertex_colors(const void* images, int dtype, int layout, const int32_t* xy, const int32_t* key, const int32_t* faces,
                              const int32_t* face_id, const int32_t* pix_key, const float* verts, const float* normals,
                              const float* centres, int N, int Nv, int Nf, int H, int W, float power, int bias, int two_sided,
                              float fill_r, float fill_g, float fill_b, float* color, float* weight_sum, int32_t* n_seen, float* spread,
                              unsigned char* visible, void* stream);
/* UV texture atlases out of the same views (csrc/k_mesh_uv.hip; shared device helpers in csrc/mesh.h): vertex normals on the device, a
 * per-texel bake with the visibility and the weights of mvd_op_mesh_vertex_colors, a dilation of the atlas into its gutters, and a
 * render of the textured mesh with perspective-correct UVs.  No context; device pointers; each call synchronises the stream.
 *   conventions   uv [Nt,2] float; face_uv [Nf,3] int32, indices into uv, parallel to faces [Nf,3].  OBJ convention: u to the right,
 *                 v up, (0, 0) at the bottom-left.  The atlas is [Ht,Wt,3] with row 0 at the top (a PNG written as is): texel (i, j)
 *                 has its centre at u = (j + 0.5) / Wt, v = 1 - (i + 0.5) / Ht.  Chart coordinates in 1/16 texel:
 *                 xs = rint(16 (u Wt - 0.5)), ys = rint(16 ((1 - v) Ht - 0.5)), computed on the host in float64 (mesh.uv_to_atlas) and
 *                 passed as int32 uv_xy [Nt,2].  mvd_op_mesh_raster on them (N = 1, Nv = Nt, faces = face_uv, key = 1 everywhere) IS
 *                 the UV-space rasteriser: its face_id [1,Ht,Wt] is the texel -> face map tex_face (-1: no chart; a texel on a
 *                 shared chart edge belongs to one face by the top-left rule, overlapping charts go to the smallest face index).  A
 *                 chart vertex beyond the guard band is invalid here as it is there.
 *   mvd_op_mesh_vertex_normals   verts [F,Nv,3]; the vertex -> face incidence of the topology in CSR form, built once on the host:
 *                 inc_ptr [Nv+1], inc_face [3 Nf], the faces of a vertex in ascending order.  One thread per (frame, vertex):
 *                 the sum of cross(v1 - v0, v2 - v0) over its incident faces in table order, fp32, then divided by its length; a
 *                 vertex with no face or a zero sum gets the zero vector.  A row of inc_ptr outside 0 <= lo <= hi <= 3 Nf, a face
 *                 index outside [0, Nf) or a corner outside [0, Nv) is never dereferenced and is counted (by frame 0) into
 *                 *bad_faces (one device int).  No floating-point atomics: frame f of a batch equals the frame computed alone.
 *   mvd_op_mesh_texel_bake   images / dtype / layout / N / H / W, face_id and pix_key [N,H,W] as mvd_op_mesh_vertex_colors takes them;
 *                 K [N,3,3], RT [N,3,4], centres [N,3], z_near as mvd_op_mesh_project; verts, normals [Nv,3]; faces, face_uv [Nf,3];
 *                 uv_xy [Nt,2]; tex_face [Ht,Wt].  A workgroup owns a 16 x 16 tile of texels.  Texel (i, j) with f = tex_face in
 *                 [0, Nf), valid indices and valid chart vertices of non-zero area A: the three int64 edge functions e_k of chart
 *                 triangle f at (16 j, 16 i), exactly as the rasteriser computes them (orientation swap included);
 *                 b_k = (float)e_k / (float)A belongs to corner k of the face AS STORED, whichever orientation the chart has;
 *                 p = sum b_k verts[faces[f][k]], n = sum b_k normals[...] (not normalised: the cosine normalises it).  For every
 *                 view in index order the fp32 chain of mvd_op_mesh_project on p gives xs, ys, key; the texel is visible in the view
 *                 iff they are valid, the nearest pixel ((xs + 8) >> 4, (ys + 8) >> 4) is inside the image and covered, and the
 *                 winning face there IS f or key + bias >= pix_key.  Weight and colour as for the vertices (cosine between n and
 *                 centre - p; bilinear at the snapped position).  texture [Ht,Wt,3] = sum w c / sum w; weight_sum, n_seen, spread
 *                 [Ht,Wt] as for the vertices (spread from a second pass).  A texel without a face or with a zero weight sum: the
 *                 fill colour, n_seen as counted, a NaN spread.  Nullable taps: visible [N,Ht,Wt] bytes, pos [Ht,Wt,3] (p; NaN
 *                 without a face), txy [N,Ht,Wt,2] and tkey [N,Ht,Wt] (the per-view integers; 0 without a face).  fp32 in a fixed
 *                 order, no floating-point atomics: two calls agree bit for bit.
 *   mvd_op_mesh_texture_dilate   texture [Ht,Wt,3] fp32, valid [Ht,Wt] bytes, passes in 0..64 -> texture_out, valid_out.  In a round an
 *                 invalid texel with at least one valid 8-neighbour (validity BEFORE the round) becomes valid and takes the mean of
 *                 the valid neighbours: summed in fp32 in the order N, NE, E, SE, S, SW, W, NW, divided by their count.  One launch
 *                 per round between two buffers; passes = 0 copies.  The outputs must not alias the inputs.
 *   mvd_op_mesh_render_uv   xy [N,Nv,2], key [N,Nv], face_id [N,H,W] as the projection and the rasteriser return them; faces, face_uv,
 *                 uv [Nt,2] fp32, texture [Ht,Wt,3] fp32 in [0, 1].  Per covered pixel: the int64 edge functions e_k of the winning
 *                 face and g_k = e_k key_k (exact, within the 2^59 above); perspective-correct barycentrics
 *                 b_k = (float)((double)g_k / (double)(g_0 + g_1 + g_2)) -- keys are proportional to 1 / Z, so this is the textbook
 *                 division done on integers; (u, v) = sum b_k uv[face_uv[f][k]]; bilinear, clamp to edge, at (u Wt - 0.5,
 *                 (1 - v) Ht - 0.5).  images: float32 in [-1, 1] (2 c - 1), layout 0 [N,3,H,W] or 1 [N,H,W,3]; uncovered pixels, and
 *                 pixels whose face has an index out of range, take the background.
 * Errors, which launch nothing: a null pointer (but the taps); F, N, Nv, Nf or Nt < 1; N > 65535; F Nv or N Nv >= 2^30; 3 Nf >= 2^31;
 * H, W, Ht or Wt outside 1..4096; N H W or N Ht Wt >= 2^31; z_near <= 0 or non-finite; power < 1; passes outside 0..64; an unknown
 * dtype or layout.  Not computed: UV unwrapping beyond mesh.triangle_atlas, mip-maps, seam-aware blending across charts. */
int mvd_op_mesh_vertex_normals(const float* verts, const int32_t* faces, const int32_t* inc_ptr, const int32_t* inc_face, int F, int Nv,
                               int Nf, float* normals, int32_t* bad_faces, void* stream);
int mvd_op_mesh_texel_bake(const void* images, int dtype, int layout, const int32_t* face_id, const int32_t* pix_key, const float* K,
                           const float* RT, const float* centres, float z_near, const float* verts, const float* normals,
                           const int32_t* faces, const int32_t* uv_xy, const int32_t* face_uv, const int32_t* tex_face, int N, int Nv,
                           int Nf, int Nt, int H, int W, int Ht, int Wt, float power, int bias, int two_sided, float fill_r, float fill_g,
                           float fill_b, float* texture, float* weight_sum, int32_t* n_seen, float* spread, unsigned char* visible,
                           float* pos, int32_t* txy, int32_t* tkey, void* stream);
int mvd_op_mesh_texture_dilate(const float* texture, const unsigned char* valid, int Ht, int Wt, int passes, float* texture_out,
                               unsigned char* valid_out, void* stream);
int mvd_op_mesh_render_uv(const int32_t* xy, const int32_t* key, const int32_t* face_id, const int32_t* faces, const int32_t* face_uv,
                          const float* uv, const float* texture, int N, int Nv, int Nf, int Nt, int H, int W, int Ht, int Wt, int layout,
                          float bg_r, float bg_g, float bg_b, float* images, void* stream);
/* Closest point on a triangle mesh (csrc/k_closest.hip; the per-triangle function in csrc/mesh.h): for each of Q query points the
 * closest point of the mesh by exhaustive search over its faces -- exact, no spatial structure is built.  No context; device
 * pointers; the call synchronises the stream.  fp32 on the vector ALU, every sum written out below, no floating-point atomics:
 * two calls agree bit for bit and the result does not depend on how the faces are spread over workgroups.
 *   one triangle  dot(x, y) = fma(x_2, y_2, fma(x_1, y_1, x_0 y_0)).  ab = b - a, ac = c - a; d1 = dot(ab, q - a), d2 = dot(ac, q - a),
 *                 d3 = dot(ab, q - b), d4 = dot(ac, q - b), d5 = dot(ab, q - c), d6 = dot(ac, q - c); vc = fma(d1, d4, -(d3 d2)),
 *                 vb = fma(d5, d2, -(d1 d6)), va = fma(d3, d6, -(d5 d4)); e1 = d4 - d3, e2 = d5 - d6.  The first region that holds, in
 *                 this order, gives the barycentrics w (all >= 0):
 *                   corner a   d1 <= 0 and d2 <= 0                    w = (1, 0, 0)
 *                   corner b   d3 >= 0 and d4 <= d3                   w = (0, 1, 0)
 *                   edge ab    vc <= 0 and d1 >= 0 and d3 <= 0        t = d1 / (d1 - d3),  w = (1 - t, t, 0)
 *                   corner c   d6 >= 0 and d5 <= d6                   w = (0, 0, 1)
 *                   edge ac    vb <= 0 and d2 >= 0 and d6 <= 0        t = d2 / (d2 - d6),  w = (1 - t, 0, t)
 *                   edge bc    va <= 0 and e1 >= 0 and e2 >= 0        t = e1 / (e1 + e2),  w = (0, 1 - t, t)
 *                   interior   s = (va + vb) + vc, v = max(vb / s, 0), u = max(vc / s, 0),  w = (max((1 - v) - u, 0), v, u)
 *                 A division whose denominator is zero gives parameter 0, so a zero-area face returns a point of itself and never
 *                 a NaN; a point cloud is passed as faces (i, i, i), which always answer with corner a.  point_k = fma(w_2, c_k,
 *                 fma(w_1, b_k, w_0 a_k)); dist2 = dot(q - point, q - point).  The regions are selected by predication.
 *   selection     key [Q] = (bits(dist2) << 32) | face; the smallest key wins: the smallest distance (dist2 >= 0, so its bits order
 *                 as the floats do), ties to the smallest face index.  A candidate needs dist2 < +inf: a face whose arithmetic
 *                 overflows, or gives a NaN, is no candidate.  The search keeps only dist2 (a 64-bit integer atomicMin on key);
 *                 a finalize pass recomputes bary / point / dist2 of the winner with the same function, so that the dist2 written
 *                 equals the key's high word bit for bit and key's low word equals face.
 *   skipped       a face with an index outside [0, Nv) or a non-finite corner is skipped and never dereferenced.
 *   normal gate   only when query_normals [Q,3] (any length) is given: face f is a candidate for query q iff dot(n_q, N_f) >=
 *                 cos_min (|n_q| |N_f|) with N_f = (b - a) x (c - a), N_0 = fma(ab_1, ac_2, -(ab_2 ac_1)) and cyclic, |x| =
 *                 sqrt(dot(x, x)).  A zero-area face, and a zero query normal, therefore always pass; a NaN normal never does.
 *   distance gate after the search: dist2 > max_dist2 is no match (+inf: no gate).
 *   no match      face = -1, dist2 = +inf, bary and point zero, key = (bits(+inf) << 32) | 0xFFFFFFFF.  A non-finite query gives
 *                 no match.
 *   launch        a workgroup owns a tile of 256 queries and one slab of faces: the grid is tiles x slabs.  slabs = 0 takes
 *                 mvd_mesh_closest_slabs(Q, Nf), a host function of Q and Nf alone that fills the chip when the query tiles do
 *                 not (1 when they do); any other count gives the same bits.
 * Errors, which return before the first HIP call: a null pointer (but query_normals); Q, Nv or Nf < 1; 3 Q, 3 Nv or 3 Nf >= 2^31;
 * max_dist2 not positive or NaN; cos_min outside [-1, 1] or NaN; slabs < 0.  Not computed: point-to-plane distances, spatial
 * acceleration structures. */
int mvd_mesh_closest_slabs(int Q, int Nf);
int mvd_op_mesh_closest_point(const float* queries, const float* query_normals, const float* verts, const int32_t* faces, int Q, int Nv,
                              int Nf, float cos_min, float max_dist2, int slabs, uint64_t* key, int32_t* face, float* bary, float* point,
                              float* dist2, void* stream);
/* The morphable-model forward (csrc/k_morph.hip): FLAME / SMPL-X parameters to vertices by linear blend skinning, the formulas of
 * the reference's third_party/MICA/models/lbs.py.  No context; device pointers but `parents`; each call synchronises the stream.
 * Everything is fp32 on the vector ALU with fused multiply-adds in an order fixed by indices alone, no atomics: two calls agree
 * bit for bit, frame f of a batch equals the same frame computed alone, and both library builds give the same bits.
 *   mvd_op_morph_pose     one wave per frame.  betas [F,NB], pose [F,J,3] (axis-angle), j_template [J,3], j_dirs [NB,J*3]:
 *                 the joint regressor folded into the template and the shape directions at load (J_reg (t + S b) = J_reg t +
 *                 (J_reg S) b), so j_rest [F,J,3] = j_template + sum_n betas[f,n] j_dirs[n], n ascending.  Rodrigues as the
 *                 reference writes it: q = r + 1e-8 per component, angle = |q|, k = r / angle, D = sin(angle) K + (1 - cos(angle))
 *                 K^2 with K the cross-product matrix of k, R = I + D: a zero vector gives D = 0 and R = I exactly.
 *                 rot [F,J,9] = R; pose_feature [F,9 (J-1)] = R_j - I for j >= 1, taken as D_j (may be NULL when J == 1).
 *                 Chain, joints in index order with p = parents[j]: G_j = G_p R_j (G_0 = R_0) and the translation of the
 *                 relative transform directly, a_j = a_p - G_p (D_j j_rest_j) (a_0 = -D_0 j_rest_0), which is the reference's
 *                 t_j - G_j j_rest_j with the rest offsets cancelled analytically: a zero pose gives A = [I|0] exactly.
 *                 A [F,J,12] = [G_j | a_j] (3x4 row-major; the reference's fourth row is constant); joints [F,J,3], the posed
 *                 joints, as the reference chains them: t_j = G_p (j_rest_j - j_rest_p) + t_p, t_0 = j_rest_0.
 *                 parents: HOST array of J <= 64 entries, parents[0] == -1 and
 *                 0 <= parents[j] < j, checked here and passed to the kernel by value.
 *   mvd_op_morph_skin     basis [L,3V]: the shape directions re-packed to [NB,3V] with the pose directions [9 (J-1),3V] appended,
 *                 coef [F,L] = betas with the pose feature appended, L = NB + 9 (J-1); v_template [V,3], weights [V,J],
 *                 A [F,J,12], post [12] (3x4, may be NULL).  b_k = fma chain over l ascending starting from v_template[v,k];
 *                 T = sum_j weights[v,j] A[f,j], j ascending; out_i = fma(T_i0, b_0, fma(T_i1, b_1, fma(T_i2, b_2, T_i3))); then
 *                 the same form with post if given.  verts [F,V,3].  A workgroup owns 16 vertices and a tile of 32 frames: the
 *                 basis is read once per 32 frames, and the order over l does not depend on the tiling.
 *   mvd_op_morph_landmarks   verts [F,V,3], faces [Nf,3] int32, lmk_face [M] int32, lmk_bary [M,3]: out [F,M,3] =
 *                 fma(w_2, x_2, fma(w_1, x_1, w_0 x_0)) over the corners of face lmk_face[m] (a static embedding).  A face or
 *                 vertex index out of range is never dereferenced: that landmark is NaN.
 * Errors, which return before the first HIP call: a null pointer (but post, and pose_feature when J == 1); F, V, L, NB, M or
 * Nf < 1; J < 1 or J > 64; L != NB + 9 (J-1); a bad parents; F V 3 >= 2^31 (and F M 3, F J 12, NB J 3 likewise).
 * Not computed here: vertex normals (mvd_op_mesh_vertex_normals); the pose-dependent contour landmarks are mvd_op_morph_contour_*
 * further down. */
int mvd_op_morph_pose(const float* betas, const float* pose, const float* j_template, const float* j_dirs, const int32_t* parents, int F,
                      int NB, int J, float* j_rest, float* rot, float* pose_feature, float* joints, float* A, void* stream);
int mvd_op_morph_skin(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                      const float* post, int F, int V, int L, int NB, int J, float* verts, void* stream);
int mvd_op_morph_landmarks(const float* verts, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary, int F, int V, int Nf,
                           int M, float* out, void* stream);
/* The morphable-model backward and the fitter (csrc/k_morph_bwd.hip, entries in csrc/c_api_morph.hip): the vector-Jacobian product
 * of the forward above, a data term and an Adam step, all fp32 with every sum in an order fixed by indices alone and no atomics:
 * two calls agree bit for bit and frame f of a batch equals the frame computed alone.  With b = t + B^T c, T = sum_j w_vj A_j,
 * o = T[:, :3] b + T[:, 3] (+ transl_f), y = P[:, :3] o + P[:, 3]:
 *   mvd_op_morph_skin_ex    mvd_op_morph_skin with an optional transl [F,3] added to o (NULL is a branch, not "+ 0": the bits of
 *                 mvd_op_morph_skin, which calls the same kernel with both NULL) and an optional output blend [F,V,3] = b.
 *   mvd_op_morph_skin_bwd   g_y [F,V,3], post [12] or NULL, weights, A, blend, basis as above.  Vertex phase, a thread per (vertex,
 *                 frame): g_o_k = fma(P_2k, g_y2, fma(P_1k, g_y1, P_0k g_y0)) (g_y without post); T as the forward chains it;
 *                 g_b [F,V,3]: g_b_k = fma(T_2k, g_o2, fma(T_1k, g_o1, T_0k g_o0)); g_T_ik = g_o_i b_k, g_T_i3 = g_o_i; the
 *                 products w_vj g_T are summed over a chunk of 256 consecutive vertices: a butterfly over each wave's 64 lanes
 *                 (partners at distance 32, 16, ... 1), then ((s0 + s1) + s2) + s3 over the chunk's 4 waves.  part_a
 *                 [mvd_morph_bwd_chunks(V), F, J 12 + 3]: g_A of the chunk, then the chunk's sum of g_o (the adjoint of transl).
 *                 Basis phase: the 3V basis columns in slabs of 256; part_c [mvd_morph_bwd_slabs(V), F, L], part_c[s,f,l] = fma
 *                 chain of basis[l,k] g_b[f,k] over the slab's columns k ascending, starting from 0.  Both counts depend on V
 *                 alone.  The consumer sums part_a over chunks and part_c over slabs, ascending, starting from chunk / slab 0.
 *   mvd_op_morph_pose_bwd   one workgroup per frame.  pose [F,J,3], j_rest [F,J,3] and A [F,J,12] as mvd_op_morph_pose wrote them,
 *                 j_dirs, parents (HOST), the two partial buffers with their counts, g_joints [F,J,3] or NULL (the adjoint of the
 *                 posed joints).  Sums the partials as above (g_pose_feature = the summed part_c[:, NB:]), then goes back through
 *                 the chain in the forward's own form, joints descending with p = parents[j]: g_R_j = G_p^T g_G_j, g_G_p +=
 *                 g_G_j R_j^T - g_a_j u_j^T + g_t_j (j_rest_j - j_rest_p)^T, g_a_p += g_a_j, g_t_p += g_t_j, g_u_j = -G_p^T g_a_j,
 *                 g_D_j = g_pose_feature_j + g_R_j + g_u_j j_rest_j^T, g_j_rest_j += D_j^T g_u_j + G_p^T g_t_j, g_j_rest_p -=
 *                 G_p^T g_t_j (root: g_R_0 = g_G_0, g_u_0 = -g_a_0, g_j_rest_0 += g_t_0); then through Rodrigues as the forward
 *                 writes it, q = r + 1e-8, angle = |q|, k = r / angle differentiated as written: the reference's autograd, finite
 *                 at a zero pose (the rotation generators).  g_pose [F,J,3]; g_betas [F,NB] = summed part_c[:, n] + (an fma
 *                 chain of j_dirs[n,c] g_j_rest[c] from 0, c ascending); g_transl [F,3] = the summed last three columns of part_a.
 *   mvd_op_morph_landmarks_bwd   g_lmk [F,M,3], g_in [F,V,3] or NULL, the vertex -> (landmark, corner) table csr_ptr [V+1], csr_ent
 *                 [n_ent] (entry = landmark * 3 + corner, ascending within a vertex), lmk_bary [M,3]: g_verts [F,V,3] = fma chain
 *                 of lmk_bary[entry] g_lmk[f, entry / 3] over the vertex's entries in table order, starting from g_in or 0.  A gather:
 *                 landmarks that share a vertex are summed in a fixed order.  Entries and offsets out of range are skipped.
 *   mvd_op_morph_fit_data   E_f = inv_vw_sum sum_v w_v |y - t|^2 + lmk_scale sum_m w'_m |l - l'|^2 (inv_vw_sum = 1 / sum_v w_v,
 *                 lmk_scale = lambda / sum_m w'_m, computed by the caller; weights NULL = ones).  verts [F,V,3]; target
 *                 [target_frames,V,3] with target_frames 1 or F, or NULL; lmk / target_lmk likewise with M, or NULL (not both
 *                 targets NULL).  g_y [F,V,3] = 2 w_v inv_vw_sum (y - t), then per table entry fma(lmk_bary[entry] (2 lmk_scale
 *                 w'_m), l - l', g_y).  E [F]: squares summed per block of 256 vertices in the vertex phase's shape into e_part
 *                 [mvd_morph_bwd_chunks(V), F], then per frame a lane-strided ascending sum over blocks (and over landmarks) and one
 *                 butterfly.  Each frame's loss is its own: no mean over F.
 *   mvd_op_morph_fit_update   p, g, m, v [F,P]; lr, lam, p0 [P].  g' = fma(2 lam, p - p0, g); torch.optim.Adam's step `step` (>= 1):
 *                 m = fma(1 - beta1, g' - m, m), v = fma((1 - beta2) g', g', v beta2), p = fma(-(lr / bias1), m / (sqrt(v) /
 *                 sqrt(bias2) + eps), p) with bias_i = 1 - beta_i^step in double on the host.  lr[c] == 0: p, m and v of that
 *                 column keep their bits.
 *   mvd_morph_fit_run   `iters` iterations of pose, skin_ex, landmarks, fit_data, skin_bwd, pose_bwd, fit_update enqueued on the
 *                 stream as plain launches with no host synchronisation between them and one at the end.  p [F,P] = betas |
 *                 pose | transl, P = NB + 3 J + 3, is read and written in place by the stages through row strides; m, v
 *                 likewise; Adam steps step0 + 1 .. step0 + iters.  workspace: as many floats of the caller as
 *                 mvd_morph_fit_workspace(F, V, NB, J, M, &floats) stores in the HOST integer (M = 0 without a landmark target).  loss_history [iters,F]: E before each update.  Each
 *                 iteration's bits are those of the seven per-op entries called in turn.
 *   mvd_op_morph_fit_data_corr   the data term against correspondences, for a target of another topology: corr_point [F,V,3] and
 *                 corr_face [F,V] as mvd_op_mesh_closest_point returns point and face for queries = verts; m_fv = (corr_face >= 0).
 *                 The normaliser is computed per frame on the device: W_f = sum_v w_v m_fv.  E_f = sum_v w_v m_fv |y - c|^2 / W_f +
 *                 the landmark term of mvd_op_morph_fit_data, unchanged; g_y = (2 w_v m_fv (1 / W_f)) (y - c), then the same landmark
 *                 gather; n_matched [F] = sum_v m_fv.  Summation shape as mvd_op_morph_fit_data: the squares and the weights per block
 *                 of 256 vertices into e_part and w_part [mvd_morph_bwd_chunks(V) + 1, F] (its last row takes 1 / W_f), then per
 *                 frame a lane-strided ascending sum over blocks and one butterfly.  W_f = 0 (nothing matched): the vertex term
 *                 and its gradient are exactly zero.  An unmatched vertex's corr_point is never read: a NaN there does not leak.
 *   mvd_morph_fit_scan_run   the loop of mvd_morph_fit_run with the target replaced by correspondences to a scan.  Iteration `it`:
 *                 pose, skin_ex, landmarks (with a landmark target); if it % refresh == 0: mvd_op_mesh_vertex_normals of the
 *                 current vertices (only with normal_gate != 0; inc_ptr / inc_face: the model's face incidence) and
 *                 mvd_op_mesh_closest_point with queries = the current vertices (their normals as query_normals with the gate),
 *                 cos_min, max_dist2 and the planned slab count; then fit_data_corr, skin_bwd, pose_bwd, fit_update.  Plain
 *                 launches on the stream, one synchronisation at the end.  Scans: Fs = 1 (shared: one query launch with Q = F V)
 *                 or Fs = F (one launch per frame), concatenated in scan_verts / scan_faces with HOST offset arrays scan_vptr
 *                 [Fs+1] and scan_fptr [Fs+1] (vertices and faces, starting at 0); face indices are local to their scan.
 *                 workspace: mvd_morph_fit_scan_workspace(F, V, NB, J, M, &floats) floats.  Outputs beyond mvd_morph_fit_run's:
 *                 matched_history [iters,F] (n_matched of every iteration) and corr_face [F,V] (the last correspondences).  Each
 *                 iteration's bits are those of the per-op entries called in turn.  Further errors: refresh < 1; Fs neither 1 nor
 *                 F; offsets that do not start at 0 or leave a scan without a vertex or a face; the normal gate without faces and
 *                 incidence; those of mvd_op_mesh_closest_point.  Not computed: point-to-plane and robust kernels, the
 *                 scan-to-model direction as a gradient term (a scatter), non-rigid per-vertex offsets.
 * Errors, which return before the first HIP call: those of the forward's list for the same arguments; a null pointer (but post,
 * transl, blend, g_joints, g_in, the weights, and one of the two targets); counts < 1; a target with neither 1 nor F frames; more
 * than 65535 frames in fit_data / fit_run; step < 1, beta outside [0, 1), eps <= 0; a workspace that is too small. */
int mvd_morph_bwd_chunks(int V);
int mvd_morph_bwd_slabs(int V);
int mvd_morph_fit_workspace(int F, int V, int NB, int J, int M, int64_t* floats);
int mvd_op_morph_skin_ex(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                         const float* post, const float* transl, int F, int V, int L, int NB, int J, float* verts, float* blend,
                         void* stream);
int mvd_op_morph_skin_bwd(const float* g_y, const float* post, const float* weights, const float* A, const float* blend,
                          const float* basis, int F, int V, int L, int NB, int J, float* g_b, float* part_a, float* part_c, void* stream);
int mvd_op_morph_pose_bwd(const float* pose, const float* j_rest, const float* A, const float* j_dirs, const int32_t* parents,
                          const float* part_a, int nchunk, const float* part_c, int nslab, const float* g_joints, int F, int NB, int J,
                          float* g_betas, float* g_pose, float* g_transl, void* stream);
int mvd_op_morph_landmarks_bwd(const float* g_lmk, const float* g_in, const int32_t* csr_ptr, const int32_t* csr_ent, const float* lmk_bary,
                               int F, int V, int M, int n_ent, float* g_verts, void* stream);
int mvd_op_morph_fit_data(const float* verts, const float* target, int target_frames, const float* vertex_weight, float inv_vw_sum,
                          const float* lmk, const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale,
                          const int32_t* csr_ptr, const int32_t* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent,
                          float* g_y, float* e_part, float* E, void* stream);
int mvd_op_morph_fit_update(float* p, const float* g, float* m, float* v, const float* lr, const float* lam, const float* p0, int F, int P,
                            int step, float beta1, float beta2, float eps, void* stream);
int mvd_morph_fit_run(const float* basis, const float* v_template, const float* weights, const float* j_template, const float* j_dirs,
                      const int32_t* parents, const float* post, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary,
                      const int32_t* csr_ptr, const int32_t* csr_ent, int F, int V, int NB, int J, int Nf, int M, int n_ent,
                      const float* target, int target_frames, const float* vertex_weight, float inv_vw_sum, const float* target_lmk,
                      int target_lmk_frames, const float* lmk_weight, float lmk_scale, float* p, float* m, float* v, const float* lr,
                      const float* lam, const float* p0, int iters, int step0, float beta1, float beta2, float eps, float* workspace,
                      size_t workspace_floats, float* loss_history, void* stream);
int mvd_op_morph_fit_data_corr(const float* verts, const float* corr_point, const int32_t* corr_face, const float* vertex_weight,
                               const float* lmk, const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale,
                               const int32_t* csr_ptr, const int32_t* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent,
                               float* g_y, float* e_part, float* w_part, float* E, int32_t* n_matched, void* stream);
int mvd_morph_fit_scan_workspace(int F, int V, int NB, int J, int M, int64_t* floats);
int mvd_morph_fit_scan_run(const float* basis, const float* v_template, const float* weights, const float* j_template, const float* j_dirs,
                           const int32_t* parents, const float* post, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary,
                           const int32_t* csr_ptr, const int32_t* csr_ent, const int32_t* inc_ptr, const int32_t* inc_face, int F, int V,
                           int NB, int J, int Nf, int M, int n_ent, const float* scan_verts, const int32_t* scan_faces,
                           const int32_t* scan_vptr, const int32_t* scan_fptr, int Fs, int normal_gate, float cos_min, float max_dist2,
                           int refresh, const float* vertex_weight, const float* target_lmk, int target_lmk_frames,
                           const float* lmk_weight, float lmk_scale, float* p, float* m, float* v, const float* lr, const float* lam,
                           const float* p0, int iters, int step0, float beta1, float beta2, float eps, float* workspace,
                           size_t workspace_floats, float* loss_history, int32_t* matched_history, int32_t* corr_face, void* stream);
/* The 2-D multi-view landmark term, the per-view contour landmarks and their loop (csrc/k_morph_2d.hip, entries in
 * csrc/c_api_morph.hip): landmarks projected into C calibrated views against detected key points in pixels, the reprojection term
 * of the reference's third_party/metrical-tracker (tracker.py:405-412, 495-508), and its per-view sliding contour (flame/FLAME.py:
 * 126-163).  The rules of the block above: fp32, every sum in an order fixed by indices alone, no atomics, two calls agree bit for
 * bit, frame f of a batch equals the frame alone.  Cameras: K [Fc,C,3,3], RT [Fc,C,3,4] (world -> camera) with Fc = cam_frames, 1
 * (shared by the frames) or F.
 *   projection    exactly mvd_op_mesh_project's fp32 chain (one device function serves both): cam = R l + t, u = (K00 X + K01 Y) / Z
 *                 + K02, v = K11 Y / Z + K12, pixel (i, j) centred at (u, v) = (j, i).  Its adjoint for a cotangent (du, dv), the chain
 *                 differentiated as written with iz = 1 / Z: gX = (du K00) iz, gY = fma(du, K01, dv K11) iz, gZ = -fma(du, fma(K01, Y,
 *                 K00 X), dv (K11 Y)) (iz iz), g_l_j = fma(R_2j, gZ, fma(R_1j, gY, R_0j gX)).
 *   mvd_op_morph_project      points [F,M,3] -> uv [F,C,M,2] (as computed, whatever the validity) and valid [F,C,M] int32 = (Z >=
 *                 z_near and X, Y, Z, u, v finite).  A thread per (frame, view, point).
 *   mvd_op_morph_project_bwd  g_uv [F,C,M,2] -> g_points [F,M,3] = the adjoint above summed over the valid views, c ascending,
 *                 starting from 0, by plain additions; a thread per (frame, point).  An invalid view adds nothing and its g_uv is
 *                 never read.
 *   mvd_op_morph_fit_data_2d  lmk [F,M,3] as mvd_op_morph_landmarks writes it; target_uv [Ft,C,M,2] in pixels and weight [Ft,C,M]
 *                 or NULL (ones), Ft = target_frames, 1 or F.  Optionally the contour set: dyn_lmk [F,C,Md,3] (one point per view),
 *                 dyn_target_uv [Ft,C,Md,2], dyn_weight [Ft,C,Md] or NULL; without it dyn_lmk, dyn_target_uv, dyn_weight, dyn_uv and
 *                 g_dyn are all NULL.  An observation (f, c, point) counts iff weight > 0, Z >= z_near and X, Y, Z, u, v are finite;
 *                 the target of an observation that does not count is never read.  With r = px_scale (uv - target): W_f = sum of w
 *                 over the counted observations of both sets, E2_f = lambda2 (sum w |r|^2) (1 / W_f) (+ E_add[f] if E_add is given:
 *                 the loop's 3-D term, one rounded addition); W_f = 0: E2_f = 0 and a zero gradient, exactly.  Outputs: uv
 *                 [F,C,M,2] and dyn_uv [F,C,Md,2] (every observation, as computed), E2 [F], n_valid [F] int32 (the counted
 *                 observations), g_lmk [F,M,3] = sum over the counted views c ascending, from 0, of the adjoint above at (du, dv) =
 *                 cf (uv - target), cf = (((2 lambda2) (px_scale px_scale)) w) (1 / W_f); g_dyn [F,C,Md,3] the same per view (0 where
 *                 the observation does not count).  Summation shape, as mvd_op_morph_fit_data_corr: the points are the M static
 *                 landmarks followed by the Md contour landmarks, a thread per (frame, point) walking the views in index order
 *                 (e = fma(w, fma(rv, rv, ru ru), e), W += w); per block of 256 points a butterfly over each wave's 64 lanes and
 *                 ((s0 + s1) + s2) + s3 over the 4 waves into part [3 mvd_morph_2d_blocks(M, Md) + 1, F] (the blocks' sums of
 *                 w |r|^2, of w, their counts as int32 bits, and a last row that takes 1 / W_f); then one wave per frame: a
 *                 lane-strided ascending sum over the blocks and one butterfly.
 *   mvd_op_morph_contour_select   A [F,J,12] as mvd_op_morph_pose wrote it.  Per (frame, view): g = the first column of the 3x3 of
 *                 A[f, neck_joint] (the chained global-times-neck rotation), Mx = S R_c G with S = diag(1, -1, -1) taking the
 *                 camera's axes (x right, y down, z forward) to the model's: Mx00 = fma chain of R_c row 0 with g, Mx10 and Mx20 the
 *                 negated chains of rows 1 and 2; yaw_deg = -atan2(-Mx20, sqrt(fma(Mx10, Mx10, Mx00 Mx00))) 180 / pi: 0 for a
 *                 frontal camera on an unposed head.  Row of a table of R = 2 h + 1 rows (R odd): y = rint(min(yaw_deg, h)) (half
 *                 to even); y >= 0: y; -h <= y < 0: h - y; y < -h: 2 h; a non-finite yaw: 0.  row [F,C] int32; yaw_deg [F,C] or NULL.
 *                 Piecewise constant: no gradient, as in the reference.
 *   mvd_op_morph_contour_landmarks   dyn_lmk_face [R,Md] int32, dyn_lmk_bary [R,Md,3]: dyn_lmk [F,C,Md,3] by mvd_op_morph_landmarks'
 *                 fma form on row[f,c] of the table.  A row, face or vertex index out of range is never dereferenced: NaN.
 *   mvd_op_morph_contour_bwd   a gather.  ct_vert [n_list]: the vertices that appear in the table, ascending; ct_ptr [n_list+1], ct_ent
 *                 [n_ent]: vertex ct_vert[i] has the entries ct_ent[ct_ptr[i] .. ct_ptr[i+1]), entry = (row Md + landmark) 3 + corner,
 *                 ascending.  g_verts [F,V,3] = g_in (NULL: zeros; g_in == g_verts: in place, what the loop does), and at every listed
 *                 vertex, over its entries in table order and inside an entry over the views c ascending with row[f,c] == the
 *                 entry's row, acc = fma(dyn_lmk_bary[entry], g_dyn[f,c,landmark], acc).  Entries and offsets out of range are skipped.
 *   mvd_morph_fit_2d_run   mvd_morph_fit_run's loop with the 2-D term.  Iteration: pose, skin_ex, landmarks; contour_select and
 *                 contour_landmarks (only with dyn_target_uv); fit_data on the vertices alone (only with a 3-D `target`: g_y0 and
 *                 E3; without one nothing reads a target and the adjoint starts from zero); fit_data_2d (E_add = E3); landmarks_bwd
 *                 with g_in = g_y0; contour_bwd in place; skin_bwd, pose_bwd, fit_update.  Plain launches on the stream, one
 *                 synchronisation at the end.  loss_history [iters,F]: the sum of the terms before each update; n_valid_history
 *                 [iters,F].  workspace: mvd_morph_fit_2d_workspace(F, V, NB, J, M, Md, C, &floats) floats (Md = 0 without a contour
 *                 target).  Each iteration's bits are those of the per-op entries called in turn.
 * Errors, which return before the first HIP call: those of the block above for the same arguments; a null pointer (but the weights,
 * E_add, yaw_deg, g_in and the contour set as a whole); Fc or Ft neither 1 nor F; C < 1, M < 1, F C M 2 >= 2^31 (F C Md 3 likewise);
 * z_near <= 0 or not finite; px_scale or lambda2 negative or not finite; part of the contour set without the rest; a contour
 * target without the model's tables; neck_joint outside [0, J); an even R; more than 65535 frames.
 * Not computed: focal length and camera refinement, photometric and silhouette terms, robust kernels, the landmark detector; the
 * tracker's eyelid / iris / mouth sub-losses are weights on this term and the caller's to set. */
int mvd_morph_2d_blocks(int M, int Md);
int mvd_op_morph_project(const float* points, const float* K, const float* RT, int cam_frames, int F, int C, int M, float z_near, float* uv,
                         int32_t* valid, void* stream);
int mvd_op_morph_project_bwd(const float* points, const float* K, const float* RT, int cam_frames, const float* g_uv, int F, int C, int M,
                             float z_near, float* g_points, void* stream);
int mvd_op_morph_fit_data_2d(const float* lmk, const float* dyn_lmk, const float* K, const float* RT, int cam_frames, const float* target_uv,
                             const float* weight, const float* dyn_target_uv, const float* dyn_weight, int target_frames, int F, int C, int M,
                             int Md, float z_near, float px_scale, float lambda2, const float* E_add, float* uv, float* dyn_uv, float* part,
                             float* E2, int32_t* n_valid, float* g_lmk, float* g_dyn, void* stream);
int mvd_op_morph_contour_select(const float* A, const float* RT, int cam_frames, int F, int C, int J, int neck_joint, int R, int32_t* row,
                                float* yaw_deg, void* stream);
int mvd_op_morph_contour_landmarks(const float* verts, const int32_t* faces, const int32_t* dyn_lmk_face, const float* dyn_lmk_bary,
                                   const int32_t* row, int F, int C, int V, int Nf, int R, int Md, float* dyn_lmk, void* stream);
int mvd_op_morph_contour_bwd(const float* g_dyn, const float* g_in, const int32_t* row, const int32_t* ct_vert, const int32_t* ct_ptr,
                             const int32_t* ct_ent, const float* dyn_lmk_bary, int F, int C, int V, int R, int Md, int n_list, int n_ent,
                             float* g_verts, void* stream);
int mvd_morph_fit_2d_workspace(int F, int V, int NB, int J, int M, int Md, int C, int64_t* floats);
int mvd_morph_fit_2d_run(const float* basis, const float* v_template, const float* weights, const float* j_template, const float* j_dirs,
                         const int32_t* parents, const float* post, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary,
                         const int32_t* csr_ptr, const int32_t* csr_ent, const int32_t* dyn_lmk_face, const float* dyn_lmk_bary,
                         const int32_t* ct_vert, const int32_t* ct_ptr, const int32_t* ct_ent, int F, int V, int NB, int J, int Nf, int M,
                         int n_ent, int R, int Md, int n_list, int ct_n_ent, int neck_joint, const float* K, const float* RT, int cam_frames,
                         int C, const float* target_uv, const float* weight, const float* dyn_target_uv, const float* dyn_weight,
                         int target_frames, float z_near, float px_scale, float lambda2, const float* target, int target3_frames,
                         const float* vertex_weight, float inv_vw_sum, float* p, float* m, float* v, const float* lr, const float* lam,
                         const float* p0, int iters, int step0, float beta1, float beta2, float eps, float* workspace,
                         size_t workspace_floats, float* loss_history, int32_t* n_valid_history, void* stream);
/* The conditioner's backward for ONE sample (its mesh / cameras active: mvd_select_sample): re-runs construct_spatial_volume and
 * construct_view_frustum_volume (morphable_diffusion.py:203-320: step embedding, 2-D encoder on the N noisy views, vertex gather,
 * view fusion, sparse voxel CNN in train mode, lattice gather, frustum gather and FrustumTV3DNet for the target view) with every
 * intermediate kept, then back-propagates dsrc{0..3} = dL/d(frustum volume l) [1,C_l,D_l,s_l,s_l] (what mvd_train_unet_step
 * returns for that sample, after the condition-dropout mask) into the gradients of spatial_volume.* and time_embed.*
 * (accumulated into the arena).  x_noisy [N,4,s,s], v_embed [N,view_dim] device pointers; timestep / target_index host values.
 * dbg_* (each may be NULL): dL/d(32^3 volume) [64,V,V,V], dL/d(fused vertex features) [Nv,16], dL/d(2-D encoder output)
 * [N,16,s,s], dL/d(step embedding) [time_dim] -- for the parity tests.  The three gather adjoints use fp32 atomic adds unless
 * mvd_train_set_deterministic turned the deterministic mode on. */
int mvd_train_conditioner_backward(mvd_ctx* ctx, const float* x_noisy, int64_t timestep, const float* v_embed, int n_views,
                                   int target_index, const float* dsrc0, const float* dsrc1, const float* dsrc2, const float* dsrc3,
                                   float* dbg_dvolume, float* dbg_dfused, float* dbg_dfeats, float* dbg_dtembed, void* stream);
/* The same for the B samples whose tables sit in slots[0..B) (distinct; uploaded by mvd_set_samples_async): the per-sample
 * stages run sample by sample, FrustumTV3DNet -- shared weights, same-shaped volumes -- runs once with the samples as its batch.
 * x_noisy [B,N,4,s,s], v_embed [B,N,view_dim], dsrc{l} [B,C_l,D_l,s_l,s_l] device pointers; timesteps [B] / target_index [B] HOST
 * arrays; dbg_* only with B = 1.  The active slot is unchanged on return. */
int mvd_train_conditioner_backward_batch(mvd_ctx* ctx, int B, const int* slots, const float* x_noisy, const int64_t* timesteps,
                                         const float* v_embed, int n_views, const int* target_index, const float* dsrc0,
                                         const float* dsrc1, const float* dsrc2, const float* dsrc3, float* dbg_dvolume,
                                         float* dbg_dfused, float* dbg_dfeats, float* dbg_dtembed, void* stream);
/* Deterministic training mode (opt-in, default off; the reference has none: grid_sample's CUDA backward raises under
 * torch.use_deterministic_algorithms).  The conditioner's backward is the one part of the training step that does not repeat bit
 * for bit: the adjoints of its three gathers -- frustum gather (morphable_diffusion.py:265-320), lattice gather of the sparse
 * CNN's rows (:232-257) and vertex gather (:203-231) -- and the fold of duplicate vertices' rows add with fp32 atomics in arrival
 * order.  With the mode on they run as gathers: no floating-point atomic, every sum in an order fixed by indices alone (view,
 * depth, row, column of the frustum points; z, y, x of the lattice points; vertex index, then voxel index), so that two backward
 * calls on the same inputs leave bit-identical gradients.  Values agree with the atomic forms to fp32 summation order.
 *   mvd_train_set_deterministic  any time on a training context (mvd_train_enable), takes effect from the next backward call; an
 *                                error on any other context, and when the sparse CNN runs in its site form (MVD_SPARSE_VALU).
 *   mvd_op_frustum_adjoint       parity hooks: ONE of the three adjoints on device buffers of the caller, deterministic != 0 the
 *   mvd_op_latent_adjoint        gather form, 0 the atomic form (which accumulates: the hook zeroes the output first); cameras and
 *   mvd_op_vertex_adjoint        mesh of the active slot, any finalized context with a mesh / cameras set.  Channels-last fp32:
 *                                frustum  d_out [TN,D,S,S,64] = dL/d(gathered frustum), view_idx [TN] HOST -> d_vol [V,V,V,64];
 *                                latent   d_vol [V,V,V,64] -> d_rows [n_rows,64], the rows of the coarsest sparse level in the
 *                                         order of mvd_rulebook_table(5); *n_rows_out (may be NULL) = n_rows, d_rows == NULL
 *                                         only queries it;
 *                                vertex   d_vf [n_views,Nv,16] = dL/d(per-view vertex features), view_idx [n_views] HOST ->
 *                                         d_feats [n_views,s,s,16] = dL/d(2-D encoder maps).
 *   mvd_probe_adjoint_calls      out[6] = launches so far of the frustum / latent / vertex adjoint in the atomic form (0..2) and
 *                                in the gather form (3..5), hooks included. */
int mvd_train_set_deterministic(mvd_ctx* ctx, int on);
int mvd_op_frustum_adjoint(mvd_ctx* ctx, const float* d_out, const int32_t* view_idx, int TN, int D, int S, int deterministic,
                           float* d_vol, void* stream);
int mvd_op_latent_adjoint(mvd_ctx* ctx, const float* d_vol, int deterministic, float* d_rows, int32_t* n_rows_out, void* stream);
int mvd_op_vertex_adjoint(mvd_ctx* ctx, const float* d_vf, const int32_t* view_idx, int n_views, int deterministic, float* d_feats,
                          void* stream);
int mvd_probe_adjoint_calls(mvd_ctx* ctx, int64_t* out);
/* Parity hooks for the forward gathers those adjoints belong to: ONE production launch of the vertex / lattice / frustum gather on
 * device buffers of the caller, with the cameras and the mesh of the active slot (any finalized context).  Channels-last fp32:
 *   mvd_op_vertex_gather    feats [n_views,s,s,16] (the layout mvd_op_vertex_adjoint writes), view_idx [n_views] HOST ->
 *                           vf_out [n_views,Nv,16];
 *   mvd_op_latent_gather    rows [n_rows,64] in the order of mvd_rulebook_table(5) -> vol_out [V,V,V,64];
 *   mvd_op_frustum_gather   vol [V,V,V,64], view_idx [TN] HOST -> out [TN,D,S,S,64]: the values exactly as the kernel stored them
 *                           in the operand type (mvd_compute_dtype), widened to fp32. */
int mvd_op_vertex_gather(mvd_ctx* ctx, const float* feats, const int32_t* view_idx, int n_views, float* vf_out, void* stream);
int mvd_op_latent_gather(mvd_ctx* ctx, const float* rows, float* vol_out, void* stream);
int mvd_op_frustum_gather(mvd_ctx* ctx, const float* vol, const int32_t* view_idx, int TN, int D, int S, float* out, void* stream);
/* Parity hook: the backward pass of ONE DepthTransformer (attention.py:49-84; cond_index 0 = middle_conditions, 1 + k =
 * output_conditions.k) given its input x [B,dim,H,W], its context volume [B,C_l,D_l,H,W] and dL/d(output) [B,dim,H,W]:
 * dx, dcontext (may be NULL) are written, parameter gradients accumulated into the arena.  depth0 = D of the finest level. */
int mvd_train_cond_backward(mvd_ctx* ctx, int cond_index, const float* x, const float* context, const float* d_out, int B, int H,
                            int W, int depth0, float* dx, float* dcontext, void* stream);
int mvd_train_get_grad(mvd_ctx* ctx, const char* name, float* out, size_t numel, void* stream);
/* Checkpoint export of a training context (what Lightning's ModelCheckpoint gets from ``state_dict()``): the current value of a
 * resident tensor by its state_dict key -- a master parameter, or a BatchNorm running_mean / running_var buffer of the sparse
 * CNN, which train-mode forwards (mvd_volume_from_fused_train) update with momentum 0.01 like nn.BatchNorm1d (network.py:105).
 * out: device pointer, numel floats.  mvd_train_bn_calls: the number of such forwards since the weights were loaded (what
 * ``num_batches_tracked`` advanced by). */
int mvd_train_get_tensor(mvd_ctx* ctx, const char* name, float* out, size_t numel, void* stream);
int64_t mvd_train_bn_calls(mvd_ctx* ctx);
int mvd_train_adamw_step(mvd_ctx* ctx, float lr, float lr_aux, float beta1, float beta2, float eps, float weight_decay, int step,
                         float inv_scale, int finetune_unet, int* skipped_out, void* stream);
int mvd_train_grad_norm(mvd_ctx* ctx, float inv_scale, int finetune_unet, float* norm_out, void* stream);
int mvd_train_adamw_step_ex(mvd_ctx* ctx, float lr, float lr_aux, float beta1, float beta2, float eps, float weight_decay, int step,
                            float inv_scale, int finetune_unet, int* skipped_out, float max_grad_norm, float ema_decay,
                            float* grad_norm_out, void* stream);
int mvd_train_last_grad_norm(mvd_ctx* ctx, float* norm_out, void* stream);
int mvd_train_ema_swap(mvd_ctx* ctx, void* stream);
int mvd_train_repack(mvd_ctx* ctx);
/* The same in the order of `stream` (the stream the optimiser update was enqueued on and the next forward will be): no device
 * synchronisation -- the pack launches wait for an event on `stream`, later work on `stream` waits for them. */
int mvd_train_repack_async(mvd_ctx* ctx, void* stream);
/* LoRA fine-tuning of a training context: low-rank adapters on chosen weight matrices, W_eff = W0 + s B A with A [rank][in],
 * B [out][rank], s = alpha / rank.  The forward and the backward pass are unchanged: the backward writes the dense gradient dW of
 * every UNet weight into the gradient arena as before, and the optimiser step projects it onto the adapters (dA = s B^T dW,
 * dB = s dW A^T), updates them with the fused AdamW kernel and writes W0 + s B A back into the master arena; the caller then
 * re-packs (mvd_train_repack*).  The projection is linear in dW, so it runs after the gradient averaging of a multi-GPU run.
 *   mvd_lora_attach        keys: n parameter names, each of shape (out, in) followed only by 1s (Linear, 1x1 and 1x1x1 convolution
 *                          weights); 1 <= rank <= 64, one rank per attach.  Snapshots W0 (a compact fp32 copy of the targets) and
 *                          allocates the adapter arenas -- parameters, gradients, two Adam moments, all zero: per target A then B,
 *                          each padded to 64 floats.  The masters are not changed (B = 0).  An attached context detaches first.
 *   mvd_lora_arena_size / _target_count / _info   floats per adapter arena; the targets in attach order: name, offsets of A and B
 *                          in the adapter arenas, out, in (each pointer may be NULL).
 *   mvd_lora_adopt_arena   as mvd_train_adopt_arena, for adapter arena `which` (0 parameters, 1 gradients, 2 / 3 moments).
 *   mvd_lora_project       the projection alone: the adapter gradient arena is OVERWRITTEN with s B^T dW / s dW A^T of the gradient
 *                          arena as it is (inspection, timing; mvd_lora_step does it itself).
 *   mvd_lora_step          projection (overwrites the adapter gradients, which keep dW's loss scale) -> the gradient-norm pass over
 *                          the adapter gradients when clipping, loss scaling or grad_norm_out asks for it (as in
 *                          mvd_train_adamw_step_ex; mvd_train_last_grad_norm reports it too) -> AdamW on the adapter arenas -> merge.
 *                          An overflowed step (*skipped_out = 1) leaves adapters, moments and masters as they were.
 *   mvd_lora_set_scale     merges at another strength s (0: the masters are W0 again) without touching the adapters; later steps
 *                          use that s.  Also the call that merges adapters written into the parameter arena by the caller.
 *   mvd_lora_detach        keep_merged == 0 restores W0 first; frees the LoRA state.  The caller re-packs. */
int mvd_lora_attach(mvd_ctx* ctx, const char* const* keys, int n, int rank, float alpha);
int mvd_lora_arena_size(mvd_ctx* ctx, int64_t* numel);
int mvd_lora_target_count(mvd_ctx* ctx);
int mvd_lora_info(mvd_ctx* ctx, int i, char* name, size_t cap, int64_t* a_off, int64_t* b_off, int64_t* out, int64_t* in);
int mvd_lora_adopt_arena(mvd_ctx* ctx, int which, float* ptr, int64_t numel);
int mvd_lora_project(mvd_ctx* ctx, void* stream);
int mvd_lora_step(mvd_ctx* ctx, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float inv_scale,
                  float max_grad_norm, int* skipped_out, float* grad_norm_out, void* stream);
int mvd_lora_set_scale(mvd_ctx* ctx, float scale, void* stream);
int mvd_lora_detach(mvd_ctx* ctx, int keep_merged);
/* DDP's bucketed, overlapped gradient averaging (train_morphable_diffusion.py:302-303: Lightning wraps the module in
 * DistributedDataParallel, whose reducer all-reduces a bucket as soon as its gradients are ready).  mvd_train_unet_step leaves
 * its UNet gradients as buckets in the order they become final during the backward pass -- one per chain of blocks (output
 * blocks 11..0, middle block, input blocks 11..0), then one for what completes at the end (the stacked emb_layers / attn2
 * projections, the head, time_embed) -- each a list of gradient-arena ranges (floats) plus an event recorded behind the last
 * kernel that writes them; together they cover model.diffusion_model.* exactly once.
 *   mvd_train_grad_bucket_count   buckets of the last step (0 before the first).
 *   mvd_train_grad_bucket         ranges of bucket k (offs / lens NULL: only *n_ranges).
 *   mvd_train_grad_bucket_wait    makes `stream` (the caller's communication stream) wait for bucket k's event.
 *   mvd_train_set_bucket_snapshot test hook: while set, every bucket's ranges are copied into `arena` (gradient-arena layout,
 *                                 device memory) right behind its event -- equal to the final gradients iff the ranges were final. */
int mvd_train_grad_bucket_count(mvd_ctx* ctx);
int mvd_train_grad_bucket(mvd_ctx* ctx, int k, int max_ranges, int64_t* offs, int64_t* lens, int* n_ranges);
int mvd_train_grad_bucket_wait(mvd_ctx* ctx, int k, void* stream);
int mvd_train_set_bucket_snapshot(mvd_ctx* ctx, float* arena);
/* The whole reducer behind the C ABI, on the communicator of mvd_comm_init (replaces DistributedDataParallel's reducer,
 * train_morphable_diffusion.py:302-303; no Python and no torch.distributed per bucket).  phase 0, called once right after
 * mvd_train_unet_step: every bucket's ranges are all-reduced (sum, in place in the gradient arena) on `comm_stream`, each bucket
 * behind its event.  phase 1, after the conditioner's backward was enqueued on `stream`: `comm_stream` waits for `stream`,
 * every arena range outside the buckets is reduced, `stream` waits for `comm_stream` and the arena is scaled by 1 / world on
 * `stream`.  phase 1 without a phase 0 reduces the whole arena (the flat all-reduce). */
int mvd_train_sync_gradients(mvd_ctx* ctx, int phase, void* comm_stream, void* stream);
/* Puts a volume [64,V,V,V] (reference layout, e.g. one sample of construct_spatial_volume's [B,64,V,V,V] result) back into
 * the context for mvd_frustum_volumes / mvd_denoise_views: with B > 1 samples per step (training_step) the per-sample
 * volumes are built first and the frustum stage runs afterwards (morphable_diffusion.py:531-533). */
int mvd_set_volume(mvd_ctx* ctx, const float* volume, void* stream);

/* SpatialVolumeNet.construct_view_frustum_volume (morphable_diffusion.py:265-320) for TN views of the
 * volume held in the context.  out_l: [TN,C_l,D_l,s_l,s_l] fp32 (reference layout), any may be NULL. */
int mvd_frustum_volumes(mvd_ctx* ctx, const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN,
                        float* out0, float* out1, float* out2, float* out3, void* stream);
/* The same for ONE target view of each of B samples (the training step, morphable_diffusion.py:496-518 with TN = 1): sample b's
 * frustum is gathered from volumes[b] [64,V,V,V] with the cameras of slot slots[b], then FrustumTV3DNet runs once with the B
 * volumes as its batch.  t_embed [B,time_dim], v_rows [B,view_dim] (the target view's embedding), view_idx [B] int32 -- device
 * pointers; out_l [B,C_l,D_l,s_l,s_l].  The active slot is unchanged on return. */
int mvd_frustum_volumes_batch(mvd_ctx* ctx, int B, const int* slots, const float* volumes, const float* t_embed, const float* v_rows,
                              const int32_t* view_idx, float* out0, float* out1, float* out2, float* out3, void* stream);

/* The per-view part of SyncDDIMSampler.denoise_apply (morphable_diffusion.py:721-738) for TN views, fully on
 * the device without leaving the library's layouts: frustum volumes -> CFG-batched UNet
 * (predict_with_unconditional_scale :132-149) -> DDIM update (:675-698).
 * x_noisy [TN,4,s,s], x_input [4,s,s], clip [context_dim], noise [TN,4,s,s] or NULL (is_step0),
 * coefficients from the DDIM tables; eps_out / x_prev [TN,4,s,s] (either may be NULL). */
int mvd_denoise_views(mvd_ctx* ctx, const float* x_noisy, const float* x_input, const float* clip, int64_t timestep,
                      const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN, float cfg_scale,
                      const float* noise, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float dir_coef,
                      float sigma, float* eps_out, float* x_prev, void* stream);
/* The same step for B samples in ONE UNet pass (batch 2 * B * TN with guidance): the reference's own batching of
 * eval/generate_all_facescape.py:106-108,128-129,184-187, where denoise_apply (morphable_diffusion.py:701-739) receives B > 1.
 * slots[b]: the sample slot (mvd_select_sample) that holds sample b's mesh tables, cameras AND 32^3 volume (the volume built
 * by mvd_volume_from_fused while that slot was active); x_noisy / noise / eps_out / x_prev [B,TN,4,h,w]; x_input [B,4,h,w];
 * clip [B,context_dim]; timesteps [B] (host); t_embed [B,time_dim]; v_embed [B,TN,view_dim]; view_idx [TN] (the same views
 * of every sample).  B == 1 with slots == NULL is mvd_denoise_views.  Per sample the result equals the single-sample call to
 * fp16 operand rounding (the larger batch changes tile plans, i.e. fp32 summation orders), not bit for bit. */
int mvd_denoise_views_batch(mvd_ctx* ctx, int B, const int* slots, const float* x_noisy, const float* x_input, const float* clip,
                            const int64_t* timesteps, const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN,
                            float cfg_scale, const float* noise, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                            float dir_coef, float sigma, float* eps_out, float* x_prev, void* stream);

/* The same step with a DPM-Solver++ multistep update in place of DDIM's (SyncDPMSolverSampler, morphablediffusion_amd/schedule.py
 * DPMSolverSchedule): the arguments of mvd_denoise_views_batch up to `noise`, then one step's coefficient row.  With the guided
 * eps and x0 = (x_noisy - s1m eps) / sqrt_at (DDIM's x0 prediction):
 *     x_next = c_x x_noisy + c_d x0 + c_c (x0 - x0_hist) + c_n noise,   then x0_hist <- x0.
 * x0_hist [B,TN,4,h,w]: the previous step's x0, read and overwritten in place (required).  first != 0: the first step of a
 * trajectory -- x0_hist is written but NOT read (its contents may be anything, NaN included).  noise may be NULL (no noise
 * term); eps_out may be NULL; x_next is required.  B == 1 with slots == NULL is the single-sample step. */
int mvd_denoise_views_ms(mvd_ctx* ctx, int B, const int* slots, const float* x_noisy, const float* x_input, const float* clip,
                         const int64_t* timesteps, const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN,
                         float cfg_scale, const float* noise, float s1m, float sqrt_at, float c_x, float c_d, float c_c, float c_n,
                         float* x0_hist, int first, float* eps_out, float* x_next, void* stream);

/* ---- per-op hooks: one kernel, or one layer's launch sequence, on the caller's data ----
 * The stateless product ops (mvd_op_cfg_ms, mvd_op_adamw_ex, mvd_op_lora_*, and above mvd_op_train_loss, mvd_op_image_metrics,
 * mvd_op_mesh_*, mvd_op_morph_*) are defined with the product API in csrc/c_api.hip (the morphable-model backward and fitter
 * in csrc/c_api_morph.hip).  Everything else from here to the end of
 * the section is a test or bench hook: csrc/c_api_hooks.hip, and for the backward, adjoint and gather hooks (which call the
 * training step's file-local functions) the end of csrc/engine_train.hip, both on the scaffold of csrc/hooks.h.  Every hook
 * that takes a context refuses a NULL one ("null context") before it touches anything.  The hooks come in two kinds:
 *   asynchronous   mvd_op_conv, mvd_op_conv3d, mvd_op_linear, mvd_op_group_norm, mvd_op_depth_attn, mvd_op_conv_bwd,
 *                  mvd_op_linear_bwd, mvd_op_conv3d_bwd, mvd_op_tgemm and the adjoint / gather hooks (mvd_op_*_adjoint,
 *                  mvd_op_*_gather): they enqueue on `stream` and return without synchronising it, so they can run beside work
 *                  on another stream (tests/test_gpu_determinism.py, tools/race_micro.py); their scratch is the context's
 *                  workspace, which the stream's order protects.
 *   synchronous    every *_ex hook (and mvd_op_group_norm_bwd / mvd_op_layer_norm_bwd, which are calls of theirs),
 *                  mvd_op_group_norm_fwd32, mvd_op_layer_norm_slabs, mvd_op_folded_group_norm, mvd_op_softmax_rows,
 *                  mvd_op_rows_split, the context-free sparse-CNN hooks, the mvd_op_train_* hooks (context-free but for
 *                  mvd_op_train_colsum / _sum_rows / _outer_add), the small-op hooks (mvd_op_target_encoder ... mvd_op_small_mix,
 *                  below, which check their arguments and write into guarded caller buffers like the *_ex kind), and the timing
 *                  hooks (mvd_bench_*, mvd_op_st_tail / mvd_op_st_head with iters > 0): the stream is synchronised before the call returns.  The *_ex kind also checks
 *                  its arguments before anything is launched and writes into caller buffers that carry guard rows. */
/* The update kernel of mvd_denoise_views_ms on its own, over n device floats: eps = eps_u + scale (eps_c - eps_u) (eps_u NULL:
 * eps = eps_c), then the update above.  No context: runs on the current device. */
int mvd_op_cfg_ms(const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise, float s1m, float sqrt_at,
                  float c_x, float c_d, float c_c, float c_n, float* x0_hist, int first, float* eps_out, float* x_next, size_t n,
                  void* stream);
/* The kernels of mvd_train_adamw_step_ex on raw device buffers of n floats (n % 4 == 0, 16-byte aligned), no context: the
 * gradient norm (norm_out: device, 1 float, may be NULL), then the fused AdamW (+ clipping for max_grad_norm > 0, + EMA for
 * e != NULL and ema_decay >= 0) step.  Synchronises the stream when a norm was computed (its scratch lives for the call). */
int mvd_op_adamw_ex(float* p, const float* g, float* m, float* v, float* e, size_t n, float lr, float beta1, float beta2, float eps,
                    float wd, int step, float inv_scale, float max_grad_norm, float ema_decay, float* norm_out, void* stream);
/* The LoRA kernels (below: mvd_lora_*) on raw device buffers, one target, no context: dW / W0 / W [out][in], A [r][in],
 * B [out][r], gA / gB shaped like A / B, all fp32; 1 <= r <= 64.  mvd_op_lora_project OVERWRITES gA = scale B^T dW and
 * gB = scale dW A^T; mvd_op_lora_merge writes W = W0 + scale B A.  A bad argument returns an error and launches nothing.  Both
 * synchronise the stream (their table and scratch live for the call). */
int mvd_op_lora_project(const float* dW, const float* A, const float* B, int out, int in, int r, float scale, float* gA, float* gB,
                        void* stream);
int mvd_op_lora_merge(const float* W0, const float* A, const float* B, int out, int in, int r, float scale, float* W, void* stream);
/* The same for n targets in one launch, as mvd_lora_step runs them: per target the offsets (floats) of dW / W from `dW` / `W`, of
 * its compact W0 from `W0`, of A from `A` (gA from `gA`) and of B from `B` (gB from `gB`), and out / in. */
int mvd_op_lora_project_grouped(const float* dW, const float* A, const float* B, int n, const int64_t* w_off, const int64_t* out,
                                const int64_t* in, const int64_t* a_off, const int64_t* b_off, int r, float scale, float* gA, float* gB,
                                void* stream);
int mvd_op_lora_merge_grouped(const float* W0, const float* A, const float* B, int n, const int64_t* w_off, const int64_t* w0_off,
                              const int64_t* out, const int64_t* in, const int64_t* a_off, const int64_t* b_off, int r, float scale,
                              float* W, void* stream);
/* The sparse voxel CNN's kernels (csrc/k_cond.hip, k_cond_bwd.hip) one at a time on raw device buffers, no context: the parity hooks
 * of tests/test_gpu_sparse_cnn_ops.py.  Rows are channels-last fp32; nbr [n_out][27] is a rule-book table (mvd_rulebook_table: row
 * index of the input at tap k = (kd*3 + kh)*3 + kw, or -1).  w is the 3x3x3 kernel in one of the checkpoint layouts -- layout 0
 * [Cout][Cin][27], 1 [Cout][27][Cin], 2 [27][Cin][Cout] -- packed here by the functions that pack a loaded checkpoint.  form 0 is the
 * one-site-per-workgroup kernel, form 1 the matrix-core kernel; form 1 with channel counts that kernel does not take is an
 * error, never a fall-back.  A bad argument returns an error and launches nothing.  Every hook synchronises the stream (its
 * scratch lives for the call).
 *   mvd_op_sparse_conv        ONE production launch of the layer: in [n_in][Cin] -> out [n_out][Cout].  scale / shift (both or
 *                             neither) [Cout]: out = relu(conv * scale + shift), the eval path's folded BatchNorm; NULL: the raw
 *                             conv output of the train path.
 *   mvd_op_bn_rows_relu       train-mode BatchNorm1d (batch statistics, biased variance) + ReLU over x [n][C] -> y (may be x);
 *                             stats_out [2][C] = [mean | rstd] (may be NULL); rmean / rvar [C] (both or neither): the running
 *                             statistics, updated with `momentum` as nn.BatchNorm1d does.  MVD_BN_LOOP selects the looped form.
 *   mvd_op_bn_rows_relu_bwd   its backward: xraw [n][C] the forward's input, stats what the forward wrote, dy [n][C] =
 *                             dL/d(output) on entry and dL/d(xraw) on return; dgamma / dbeta [C] are ADDED to.  C must divide 256.
 *   mvd_op_sparse_conv_bwd    the backward of ONE layer as the conditioner's backward runs it per layer: in [n_in][Cin] the
 *                             layer's input, d_out [n_out][Cout] (form 1 with level0_subm: the duplicate fold rewrites it in
 *                             place) -> d_in [n_in][Cin] written, the weight gradient ADDED to gw, laid out like w.  strided: the
 *                             stride-2 layer (data gradient through the inverse table), else submanifold (n_in == n_out; tap
 *                             flip).  level0_subm (form 1): nbr may hold duplicate rows (centre tap != own row), whose
 *                             gradients are folded into their representatives first -- with atomics, or for deterministic != 0
 *                             in row order.  form 0 zero-fills d_in and scatters with atomics (deterministic != 0: an error).
 * poison != 0: the hook's scratch (partial sums, inverse table, flags) is filled with 0xFF bytes before use. */
int mvd_op_sparse_conv(const float* in, const int32_t* nbr, int n_out, int Cin, int Cout, const float* w, int layout, const float* scale,
                       const float* shift, int form, float* out, void* stream);
int mvd_op_bn_rows_relu(const float* x, int n, int C, const float* gamma, const float* beta, float eps, float momentum, float* y,
                        float* stats_out, float* rmean, float* rvar, void* stream);
int mvd_op_bn_rows_relu_bwd(const float* xraw, float* dy, int n, int C, const float* gamma, const float* beta, const float* stats,
                            int poison, float* dgamma, float* dbeta, void* stream);
int mvd_op_sparse_conv_bwd(const float* in, const int32_t* nbr, float* d_out, int n_in, int n_out, int Cin, int Cout, int strided,
                           int level0_subm, int deterministic, int form, const float* w, int layout, int poison, float* d_in, float* gw,
                           void* stream);
int mvd_op_conv(mvd_ctx* ctx, const float* x_nchw, int B, int Cin, int H, int W, const float* w, const float* bias,
                int Cout, int ksize, int stride, int upsample, const float* resid_nchw, float* out_nchw, int force_splitk,
                void* stream);
/* (mvd_op_conv: force_splitk == -2 with Cin <= 8 runs the UNet's inference form of its first layer, -3 with Cout <= 4 that of its
 * last layer: exact fp32 on the vector ALU) */
/* a_half != 0: A is rounded to fp16 in HBM first (the layout of operand-only activations) and, for M >= 512,
 * the dense LDS-DMA GEMM runs; resid [M][N] (or null) is added in the epilogue; force_splitk > 0 fixes the
 * split-K factor */
int mvd_op_linear(mvd_ctx* ctx, const float* a, int M, int K, const float* w, const float* bias, int N, int geglu,
                  const float* resid, int a_half, int force_splitk, float* out, void* stream);
int mvd_op_group_norm(mvd_ctx* ctx, const float* x_nchw, int B, int C, int HW, int groups, const float* gamma,
                      const float* beta, float eps, int act, float* out_nchw, void* stream);
/* depth_attn_kernel (csrc/k_depth.hip) on its own, in the kernel's layouts: qk [n_cond*HW][4][Cc] fp32 (the folded query),
 * context [n_cond][D][HW][Cc] fp32 (rounded to fp16 here into rows of ldx >= Cc halfs, ldx % 8 == 0, 0 = Cc; the pad columns hold NaN
 * bit patterns, so a read past Cc shows in the result), fill_row [4*Cc] fp32 (nfill > 0; rounded to fp16, with split != 0 to the
 * [hi | lo | hi] row relu_beta_tile_kernel writes).  out [n_cond*HW + nfill + 1][4*Cc] fp32: z, then the nfill fill rows, then ONE
 * guard row behind what the launch may write, preset to NaN bit patterns (it must come back NaN).  split != 0: the kernel writes
 * [hi | lo | hi] rows, out receives hi + lo (NaN where the third block differs from the first) and hi_out (may be NULL) hi alone.
 * check_only != 0: nothing is allocated or launched, the call returns what the launcher's argument check returns (0, or non-zero
 * with its text in mvd_last_error). */
int mvd_op_depth_attn(mvd_ctx* ctx, const float* qk, const float* context, const float* fill_row, int n_cond, int HW, int D, int Cc,
                      int heads, int ldx, int split, int nfill, int check_only, float* out, float* hi_out, void* stream);
int mvd_op_conv3d(mvd_ctx* ctx, const float* x_ncdhw, int B, int Cin, int D, int H, int W, const float* w,
                  const float* bias, int Cout, int stride, int transposed, const float* resid, float* out, void* stream);
/* backward-kernel hooks used by tests/test_gpu_train_ops.py (each is compared with torch.autograd of the same op): GroupNorm
 * (+ SiLU / ReLU) backward and LayerNorm backward on channels-last fp32 ([B,rows,C] / [rows,C]): mvd_op_group_norm_bwd_ex /
 * mvd_op_layer_norm_bwd_ex below with dense rows, eps 1e-5 (LayerNorm), no pre-add, and dx / dgamma / dbeta WRITTEN.
 * MVD_GN_BWD_ONE_BLOCK picks form 1.  (The self-attention backward is mvd_op_attention_bwd_ex below.) */
int mvd_op_group_norm_bwd(mvd_ctx* ctx, const float* x, const float* dy, int B, int rows, int C, int groups, const float* gamma,
                          const float* beta, float eps, int act, float* dx, float* dgamma, float* dbeta, void* stream);
int mvd_op_layer_norm_bwd(mvd_ctx* ctx, const float* x, const float* dy, int rows, int C, const float* gamma, float* dx,
                          float* dgamma, float* dbeta, void* stream);
/* The training backward's norms and row reductions (csrc/k_bwd.hip) in every form the training step launches them in
 * (tests/test_gpu_norm_bwd_ops.py), through the step's own gn_backward / ln_backward / gn_forward32 (csrc/engine_train.hip).  All
 * operands are fp32 device buffers; a bad argument, or a shape the launcher refuses, returns non-zero before anything is
 * launched.  The caller presets every result buffer to 0xFF bytes with one guard row behind it (and pad columns where a stride
 * exceeds the width) -- or, where the result is added to, its body to the values to start from; the production launch writes into
 * them directly.  poison != 0 fills the free workspace (slab partials, per-slab channel sums) with 0xFF bytes first.
 *
 * mvd_op_group_norm_bwd_ex: x [B][rows][ld] the norm's input, pre [B][pld] (may be NULL) the per-sample pre-add of the forward
 * (FiLM), dy [B][rows][ldy] the gradient of act(gamma xhat + beta), act 0 none / 1 SiLU / 2 ReLU.  form 0: the slabbed kernels with
 * S_force (1..64) row slabs per (sample, group), 0 = the plan of bwd_gn_slabs; form 1: one workgroup per (sample, group).
 * dx [B][rows][lddx] is written, or added to with accum != 0; dgamma / dbeta [C] are always ADDED to, as the gradient arena is
 * (two-job bwd_sum_rows_multi over the B * S partial rows); dpre [B][ldp] (may be NULL) receives the per-sample column sums of dx
 * (bwd_colsum_samples over the S slab rows), columns C .. ldp - 1 are not touched.  *S_used (may be NULL): the slab count.
 * mvd_op_group_norm_fwd32: the fp32 forward of the DepthTransformer's re-computation, y [B][rows][ldy] = act(GroupNorm(x)).
 * mvd_op_layer_norm_bwd_ex: x [rows][ld], dy [rows][ldy], C <= 1280; dx [rows][lddx] written or added to, dgamma / dbeta ADDED to
 * (partials of [nblk][2][C], two-job sum with a row stride of 2 C); *nblk_used (may be NULL): the partial rows. */
int mvd_op_group_norm_bwd_ex(mvd_ctx* ctx, const float* x, int ld, const float* pre, int pld, const float* dy, int ldy, int B, int rows,
                             int C, int groups, const float* gamma, const float* beta, float eps, int act, int form, int S_force,
                             float* dx, int lddx, int accum, float* dgamma, float* dbeta, float* dpre, int ldp, int poison,
                             int* S_used, void* stream);
int mvd_op_group_norm_fwd32(mvd_ctx* ctx, const float* x, int ld, int B, int rows, int C, int groups, const float* gamma,
                            const float* beta, float eps, int act, int S_force, float* y, int ldy, int poison, int* S_used,
                            void* stream);
int mvd_op_layer_norm_bwd_ex(mvd_ctx* ctx, const float* x, int ld, const float* dy, int ldy, int rows, int C, const float* gamma,
                             float eps, float* dx, int lddx, int accum, float* dgamma, float* dbeta, int poison, int* nblk_used,
                             void* stream);
/* The reductions, one launch each.  mvd_op_train_colsum (bwd_colsum_samples): out[b][c] = sum over the rows of sample b of
 * v [B][rows][ld], c < C, out rows ldo apart; src_f16: v is rounded to the library's 16-bit type first and the 16-bit kernel runs.
 * mvd_op_train_sum_rows (bwd_sum_rows_multi): n = 1..4 jobs in one launch, out[k][c] (+)= sum_{r < R[k]} part[k][r * ldp[k] + c]
 * for c < C[k]; the arrays are host arrays, their pointers device pointers.  mvd_op_train_outer_add (bwd_outer_add):
 * out [M][N] += sum_{k < K} a[k][m] b[k][n], a [K][lda], b [K][ldb]. */
int mvd_op_train_colsum(mvd_ctx* ctx, const float* v, int src_f16, int ld, int B, int rows, int C, float* out, int ldo, void* stream);
int mvd_op_train_sum_rows(mvd_ctx* ctx, int n, const float* const* part, const int* R, const int* C, const long* ldp, float* const* out,
                          const int* accum, void* stream);
int mvd_op_train_outer_add(mvd_ctx* ctx, const float* a, int lda, const float* b, int ldb, float* out, int M, int N, int K,
                           void* stream);
/* Adjoints of the training step's convolutions, Linears and GEMMs (csrc/engine_train.hip), one layer at a time on the production
 * code: the engine's forward pack of w (xp != 0: the extended-precision [w_hi | w_hi | w_lo] layout), the adjoint pack built as at
 * finalize, then the backward functions the training step calls.  Activations are channels-last fp32 device buffers; an input
 * width C is stored with a row stride of up8(C) (pad columns zero); x_f16 != 0: the production path reads x as fp16 (rounded
 * here).  dx is written, or added to with accum != 0; dw / db (reference layouts; either may be NULL) are always ADDED to, as
 * the gradient arena is.  poison != 0: the free workspace is filled with 0xFF bytes before the op runs.
 * mvd_op_conv_bwd: kind 0 plain 3x3 / 1x1 (ksize), 1 Downsample (3x3 stride 2), 2 Upsample (nearest x2, then 3x3); x / dx
 * [B,H,W,up8(Cin)], dy [B,Ho,Wo,Cout], w [Cout][Cin][k][k]; need_din == 0 skips dx (the first layer). */
int mvd_op_conv_bwd(mvd_ctx* ctx, int kind, int ksize, int B, int Cin, int H, int W, int Cout, const float* x, int x_f16,
                    const float* w, const float* dy, int xp, int accum, int need_din, int poison, float* dx, float* dw, float* db,
                    void* stream);
/* mvd_op_linear_bwd: x / dx [rows][up8(K)] (rows % B == 0, B = samples), w [N][K], dy [rows][N].  dx_f16: dx produced in fp16
 * (as the attention output projection's), returned as fp32.  staged: dy's fp16 row image and transposed image come from one
 * read (the SpatialTransformer's staging).  geglu: the FF1 GEGLU backward (bias [N] needed, N % 64 == 0): dy is dL/d(value *
 * gelu(gate)) [rows][N/2], the pre-activations are re-computed from fp16 x. */
int mvd_op_linear_bwd(mvd_ctx* ctx, int B, int rows, int K, int N, const float* x, int x_f16, const float* w, const float* bias,
                      const float* dy, int geglu, int dx_f16, int staged, int xp, int accum, int poison, float* dx, float* dw,
                      float* db, void* stream);
/* mvd_op_conv3d_bwd: kind 0 Conv3d(k3, s1, p1), 1 Conv3d(k3, s2, p1) (even D, H, W), 2 ConvTranspose3d(k3, s2, p1, op1);
 * x / dx [B,D,H,W,Cin] (Cin % 8 == 0), dy on the output grid [B,Do,Ho,Wo,Cout], w [Cout][Cin][27] (kind 2: [Cin][Cout][27]). */
int mvd_op_conv3d_bwd(mvd_ctx* ctx, int kind, int B, int Cin, int D, int H, int W, int Cout, const float* x, int x_f16,
                      const float* w, const float* dy, int accum, int poison, float* dx, float* dw, float* db, void* stream);
/* mvd_op_tgemm: out[M][N] (ldc) (+)= op(A) op(B) through the training step's tgemm.  a_trans: A stored [K][M], else [M][K];
 * b_trans: B stored [N][K], else [K][N]; lda / ldb the stored row strides; a_f16 / b_f16: the operand is passed to tgemm as
 * fp16 (rounded here); xp: extended precision (fp32 operands only). */
int mvd_op_tgemm(mvd_ctx* ctx, int M, int N, int K, const float* a, int a_f16, int a_trans, long lda, const float* b, int b_f16,
                 int b_trans, long ldb, float* out, int ldc, int accum, int xp, int poison, void* stream);
/* Row-chain kernel test / timing hook (csrc/k_rowchain.hip): the row-local tail of a SpatialTransformer block in ONE launch,
 *   t2 = ao @ w_ao^T + b_ao + rowbias[sample] + xin   (flags & 1; otherwise t2 = xin)     ldm/modules/attention.py:196-200, 266-267
 *   t3 = t2 + FF2(GEGLU(FF1(LayerNorm(t2))))                                              ldm/modules/attention.py:37-73, 268
 *   out = t3 @ w_po^T + b_po + resid                  (flags & 2; otherwise out = fp16(t3)) ldm/modules/attention.py:333-336
 * on fp32 operands in the reference's layouts (w1 [8C][C] value rows then gate rows, w2 [C][4C]); rows % 128 == 0, T (rows per
 * sample) % 32 == 0, C in {64, 128, 256, 320}.  flags & 4 (without 2): the fp16 result is written as [hi | lo | hi] rows and
 * returned as hi + lo; flags & 8 (with 2): proj_out in extended precision.  iters > 0: the launch is repeated and *ms_out receives the mean milliseconds per launch. */
int mvd_op_st_tail(mvd_ctx* ctx, int C, int rows, int T, const float* ao, const float* xin, const float* rowbias,
                   const float* w_ao, const float* b_ao, const float* ln_g, const float* ln_b, const float* w1, const float* b1,
                   const float* w2, const float* b2, const float* w_po, const float* b_po, const float* resid, float* out,
                   int flags, int iters, float* ms_out, void* stream);
/* Row-head kernel test / timing hook (csrc/k_rowchain.hip: rowhead_kernel), the row-local front of a SpatialTransformer block in ONE
 * launch, C = 320:  t0 = n0 @ w_pi^T + b_pi (fp32 out; n0 = the GroupNorm output, rounded to fp16 as in the engine);
 * qkv = LayerNorm(t0; ln_g, ln_b) @ [w_q; w_k; w_v]^T (fp16 in the engine, returned as fp32 [rows][3C]).
 * ldm/modules/attention.py:325-332, 266, 186-190.  rows % 128 == 0.  xp != 0: proj_in in extended precision (fp16 hi + lo parts of
 * both operands, three products) -- n0 is then NOT rounded to fp16 first. */
int mvd_op_st_head(mvd_ctx* ctx, int rows, int xp, const float* n0, const float* w_pi, const float* b_pi, const float* ln_g,
                   const float* ln_b, const float* w_q, const float* w_k, const float* w_v, float* t0_out, float* qkv_out,
                   int iters, float* ms_out, void* stream);
/* Forward-form hooks (tests/test_gpu_epilogue_forms.py): the forward kernels in the forms the inference path and the first-stage
 * model launch them in.  Common rules: operands are fp32 in the reference's layouts (activations channels-last, weights [N][K] /
 * [Cout][Cin][k][k]); result buffers are the caller's, written by the production launch itself, as fp32 or as the library's
 * 16-bit type (mvd_compute_dtype) -- the caller sizes them with one guard row behind the last row (and pad columns where ld > width)
 * and presets them to 0xFF bytes, so a write outside the result shows; a bad argument returns non-zero before anything is
 * launched; poison != 0 fills the free workspace (the launch's own scratch: split-K slabs, operand copies) with 0xFF bytes once
 * the operands are staged; the stream is synchronised before the call returns.
 *
 * mvd_op_linear_ex (run_linear) / mvd_op_conv_ex (run_conv2d, or run_upconv2d with up_fold): every GemmArgs field.  B samples of
 * rows / B rows; rowbias [B][rb_ld] (conv: rb_ld % 4 == 0); out = act(alpha * acc + bias + rowbias[sample] + resid) with act 0 / 1 (SiLU); use_bias = 0
 * ignores the bias; out_f16: 16-bit result, with out_split as [hi | lo | hi] blocks of N columns (ldc >= 3 N); resid [rows][ldr]
 * fp32, rounded to 16 bits first when resid_f16; a_half: the activation is rounded to 16 bits in memory first (else the kernels
 * read fp32); xp: extended precision -- the activation is split into [a_hi | a_lo | a_hi] (launch_rows_f32_to_f16_split) and the
 * weight packed as [w_hi | w_hi | w_lo]; force_splitk > 0 fixes the split.  slabs (may be NULL): a buffer of slabs_cap floats offered
 * for a deferred split-K reduction (GemmArgs::slabs, defer_epilogue); *sk_used is the split left in it (1: `out` is finished).
 * conv only: x [B][H][W][Cin] (Cin % 8 == 0), stride 1 / 2, upsample 0 / 1 (fused nearest x2), tap_shift = 1: zero padding on the right
 * and bottom only (the first-stage encoder's Downsample: 3x3, stride 2, even H and W only); conv3x_stream != 0 also packs the
 * weights as a conv3x fragment stream where the shape has one. */
int mvd_op_linear_ex(mvd_ctx* ctx, const float* a, int B, int rows, int K, const float* w, const float* bias, int N,
                     const float* rowbias, int rb_ld, float alpha, int act, int use_bias, int out_f16, int out_split, int ldc,
                     const float* resid, int resid_f16, int ldr, int a_half, int force_splitk, int xp, float* slabs,
                     size_t slabs_cap, int defer_epilogue, int* sk_used, int poison, void* out, void* stream);
int mvd_op_conv_ex(mvd_ctx* ctx, const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout, int ksize,
                   int stride, int upsample, int up_fold, int tap_shift, const float* rowbias, int rb_ld, float alpha, int act,
                   int use_bias, int out_f16, int out_split, int ldc, const float* resid, int resid_f16, int ldr, int a_half,
                   int force_splitk, int xp, int conv3x_stream, float* slabs, size_t slabs_cap, int defer_epilogue, int* sk_used,
                   int poison, void* out, void* stream);
/* mvd_op_conv3d_ex (run_conv3d / run_convT3d; tests/test_gpu_conv3d_forms.py): the GemmArgs fields the two 3-D U-nets set.
 * x [B][D][H][W][Cin] (Cin % 8 == 0); w [Cout][Cin][27], or [Cin][Cout][27] with transposed (ConvTranspose3d k3 s2 p1 op1, stride
 * must be 1 then); stride 1 / 2; out = acc + bias + resid on [B][Do][Ho][Wo] rows of ldc columns, fp32 or 16-bit (out_f16);
 * resid [rows][ldr] fp32; in_place: the residual image is first copied into the result buffer (rounded to 16 bits with out_f16)
 * and read from there by the launch, as the networks' up path does.  a_half, force_splitk, poison: as above. */
int mvd_op_conv3d_ex(mvd_ctx* ctx, const float* x, int B, int D, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                     int stride, int transposed, int use_bias, const float* resid, int ldr, int in_place, int out_f16, int ldc,
                     int a_half, int force_splitk, int poison, void* out, void* stream);
/* mvd_op_conv3d_form (tests/test_gpu_conv3d_halo.py): mvd_op_conv3d_ex with the kernel form chosen by the caller.  form 0: the
 * engine's own routing; form 1: conv3z, the plane-halo kernel of the 3x3x3 stride-1 layers (k_conv3x.hip), whatever the row count --
 * an error, never another kernel, where the layer is outside its limits (fp16 source, Cin % 64 == 0, Cout 64 or 128, H and W
 * multiples of 16; force_splitk is not used: the kernel does not split). */
int mvd_op_conv3d_form(mvd_ctx* ctx, const float* x, int B, int D, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                       int stride, int transposed, int use_bias, const float* resid, int ldr, int in_place, int out_f16, int ldc,
                       int a_half, int force_splitk, int form, int poison, void* out, void* stream);
/* The form the engine's routing gives a 3x3x3 layer of this shape (0: the kernels mvd_op_conv3d_ex documents, 1: conv3z), assuming
 * the weights carry every stream the engine packs for them and a context with its default switches: the gate igemm_go puts in front
 * of the predicate (MVD_NO_CONV3X / MVD_NO_HALO unset, inference context) is not evaluated here -- with either switch set, or in a
 * training context, no layer has a stream and every layer keeps form 0.  Needs no context and no device; -1 = bad arguments. */
int mvd_conv3d_routed_form(int B, int D, int H, int W, int Cin, int Cout, int stride, int transposed, int a_half, int out_f16, int ldc,
                           int has_resid, int resid_f16, int ldr, int force_splitk);
/* GroupNorm(+act) of sum(slabs) + bias2 + preadd[sample] + resid.  x: nslab slabs of [B][rows][ld] fp32, slab_stride floats apart.
 * form 0: run_group_norm's own choice of kernel; form 1: the two-pass pair called directly (one slab, no bias2 / resid / mat).
 * split 0: out [B*rows + 1][ldo] 16-bit; 1: [hi | lo | hi] blocks of C columns; 2: fp32 rows of ldo / 2 floats.  mat (may be NULL):
 * the summed tensor in fp32, [B*rows + 1][ldm]. */
int mvd_op_group_norm_ex(mvd_ctx* ctx, const float* x, int B, int rows, int C, int ld, int groups, const float* gamma,
                         const float* beta, float eps, int act, int form, const float* preadd, int pld, int split, int nslab,
                         size_t slab_stride, const float* bias2, const float* resid, int ldr, float* mat, int ldm, int ldo,
                         int poison, void* out, void* stream);
/* LayerNorm of sum(slabs) + bias + rowbias[row / T] + resid (launch_layernorm_slabs; mat [rows + 1][C] receives that row in fp32,
 * raw -- may be NULL -- its 16-bit copy, rows ld_raw apart).  plain != 0: launch_layernorm on one slab, raw optional, no mat. */
int mvd_op_layer_norm_slabs(mvd_ctx* ctx, const float* slabs, int nslab, size_t slab_stride, int rows, int C, const float* bias,
                            const float* rowbias, int rb_ld, int T, const float* resid, int ldr, const float* gamma,
                            const float* beta, float eps, int plain, int ld_raw, int poison, float* mat, void* raw, void* out,
                            void* stream);
/* GroupNorm folded into two GEMM passes (the UNet's context fold): statistics-only GEMM -> partials [B * rps / 256 + 1][N / cpg][2]
 * (sum, sum of squares per 256-row tile and group), launch_gn_finalize -> scale, shift [B + 1][N], apply GEMM -> out
 * [B * rps + 1][N] 16-bit = relu(group_norm(x @ w^T)).  Refuses what the engine does not fold: rps % 256 != 0, cpg not 8 / 16 / 32. */
int mvd_op_folded_group_norm(mvd_ctx* ctx, const float* x, int B, int rps, int K, const float* w, int N, int cpg,
                             const float* gamma, const float* beta, float eps, int poison, float* partials, float* scale,
                             float* shift, void* out, void* stream);
/* row softmax of [rows][cols] fp32 scores, cols <= 4096: 16-bit (out_f32 == 0) or fp32 probabilities, out [rows + 1][cols] */
int mvd_op_softmax_rows(mvd_ctx* ctx, const float* scores, int rows, int cols, int out_f32, void* out, void* stream);
/* launch_rows_f32_to_f16_split: fp32 rows lda floats apart -> out [rows + 1][3 C] 16-bit, [hi | lo | hi] */
int mvd_op_rows_split(mvd_ctx* ctx, const float* x, int lda, int rows, int C, void* out, void* stream);
/* Attention hooks (tests/test_gpu_attention.py).  q, k, v (and d_out) are fp32 [B][T][heads*d]; a bad argument (T < 1, Tstride
 * non-zero and < T, ld_pad % 8 != 0, a head width without a kernel, a null pointer) returns non-zero before anything is launched;
 * the stream is synchronised before the call returns.
 *
 * mvd_op_attention_ex: attn_kernel on the engine's fused 16-bit image [token][q | k | v] with rows of 3 C + ld_pad elements
 * (C = heads * d) and samples Tstride rows apart (0 = T; CLIP runs 257 tokens in 264 rows).  The whole image -- pad rows
 * T .. Tstride - 1 of every sample, pad columns, and one guard row behind the last sample -- is filled with 0xFF bytes (NaN in
 * fp16 and in bfloat16) before q, k, v are packed into it, and so is the kernel's result [B * Tstride + 1][C]; out receives
 * those result rows as fp32, pad and guard rows included: they must come back NaN.  xcd: -1 = the workgroup order
 * MVD_ATTN_NO_XCD asks for, 0 = without the XCD remap, 1 = with it.
 *
 * mvd_op_attention_bwd_ex: the training step's sequence (attn_kernel forward, cast of d_out to 16 bits, bwd_attention; the kernels
 * themselves work on the 16-bit images) with one guard row behind the
 * last sample of the qkv, o, dO and dqkv images; dqkv, lse and delta start as 0xFF bytes.  dq, dk, dv, o: [B * T + 1][C] fp32
 * (the last row is the guard); lse (log2 units, as the kernels keep it), delta: [B * heads * T + 1] fp32, the last element the
 * guard. */
int mvd_op_attention_ex(mvd_ctx* ctx, const float* q, const float* k, const float* v, int B, int T, int heads, int d, int Tstride,
                        int ld_pad, int xcd, float* out, void* stream);
int mvd_op_attention_bwd_ex(mvd_ctx* ctx, const float* q, const float* k, const float* v, const float* d_out, int B, int T,
                            int heads, int d, float* dq, float* dk, float* dv, float* lse, float* delta, float* o, void* stream);
/* The fp32 kernels of the DepthTransformer's training form (csrc/k_train.hip) one at a time on raw device buffers, no context.
 * The caller presets every result buffer to NaN (with a guard row behind it); what a launcher refuses comes back as its error,
 * nothing is launched and the results stay as they were; the stream is synchronised.
 *   mvd_op_train_depth_attn      q [R][I], k / v [(R / HW) * D * HW][I] (row = (b * D + depth) * HW + pixel), I = hn * hd, scale
 *                                hd^-0.5 -> attn [R][hn][D], z [R][I]
 *   mvd_op_train_depth_attn_bwd  its backward from attn and dz [R][I] -> dq [R][I], dk / dv shaped like k
 *   mvd_op_train_im2col3         x [B][H][W][C] -> col [B*H*W][9*C], tap = (dy + 1) * 3 + (dx + 1), zero outside
 *   mvd_op_train_col2im3         the transpose: dcol [B*H*W][9*C] -> dx [B][H][W][C]
 *   mvd_op_train_perm_w3         to_mat != 0: conv weight [N][C][3][3] -> GEMM matrix [N][9][C]; 0: the reverse */
int mvd_op_train_depth_attn(const float* q, const float* k, const float* v, int R, int HW, int D, int hn, int hd, float* attn,
                            float* z, void* stream);
int mvd_op_train_depth_attn_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dz, int R, int HW,
                                int D, int hn, int hd, float* dq, float* dk, float* dv, void* stream);
int mvd_op_train_im2col3(const float* x, int B, int H, int W, int C, float* col, void* stream);
int mvd_op_train_col2im3(const float* dcol, int B, int H, int W, int C, float* dx, void* stream);
int mvd_op_train_perm_w3(const float* src, int N, int C, int to_mat, float* dst, void* stream);
/* The small-op layer one production launcher at a time (tests/test_gpu_small_ops.py; csrc/c_api_hooks.hip describes every operand):
 * synchronous, arguments checked before anything is allocated or launched, results written by the launcher straight into the
 * caller's buffers (0xFF presets, one guard row, pad columns where a stride exceeds the width).  16-bit operands are given in
 * fp32 and rounded by the hook; 16-bit results are returned as written.  *form_used (may be NULL): the kernel form the launcher
 * chose -- mvd_op_small_linear 1 vector / 0 scalar, mvd_op_layout 1 LDS-tiled / 0 element, mvd_op_pack_weight 0 element / 1 per-tap /
 * 2 per-tap with 16-byte stores.
 *   mvd_op_target_encoder     launch_target_encoder on w[8] ([16][4][3][3], then [16][16][3][3]), bias[8], gamma[7], beta[7]
 *   mvd_op_small_linear       launch_small_linear; rows < 0 broadcasts the one input row to -rows result rows
 *   mvd_op_timestep_embedding launch_timestep_embedding, t on the device
 *   mvd_op_layout             op 0 launch_nchw_to_nhwc, 1 launch_nhwc_to_nchw
 *   mvd_op_pack_weight        launch_pack_weight at out + dst_off halfs; Cin is the packed width
 *   mvd_op_move               op 0 pack_upconv_weight, 1 permute_geglu_bias, 2 relu_beta_tile, 3 fill_rows_f16, 4 rows_f32_to_f16,
 *                             5 upsample2_f16, 6 add_image_rows, 7 rows_f16_to_nchw, 8 sparse_densify
 *   mvd_op_fold               op 0 launch_fold_qk, 1 launch_fold_ov, 2 launch_fold_mm; out fp32 (out_f32) or 16-bit
 *   mvd_op_cfg_assemble       the samplers' UNet batch assembly (timesteps: host), mvd_op_cfg_ddim: launch_cfg_ddim
 *   mvd_op_small_mix          op 0 launch_fuse_views, 1 launch_mse, 2 launch_accumulate_f32, 3 launch_add_rows */
int mvd_op_target_encoder(mvd_ctx* ctx, const float* x, const float* pre, int n_views, const float* const* w, const float* const* bias,
                          const float* const* gamma, const float* const* beta, float* feats, void* stream);
int mvd_op_small_linear(mvd_ctx* ctx, const float* a, int lda, int rows, int K, const float* w, const float* bias, int N, int act_in,
                        float* out, int ldo, int accumulate, int* form_used, void* stream);
int mvd_op_timestep_embedding(mvd_ctx* ctx, const int64_t* t, int B, int dim, float* out, void* stream);
int mvd_op_layout(mvd_ctx* ctx, int op, const float* in, int B, int C, int HW, int ld, int cpad, float* out, int* form_used,
                  void* stream);
int mvd_op_pack_weight(mvd_ctx* ctx, const float* src, int N, int Cin, int taps, int transposed, int geglu, int cin_src, int xp,
                       int dst_off, void* out, int* form_used, void* stream);
int mvd_op_move(mvd_ctx* ctx, int op, const float* a, const void* b, int i0, int i1, int i2, int i3, int i4, void* out, void* stream);
int mvd_op_fold(mvd_ctx* ctx, int op, const float* a, const float* b, int heads, int hd, int Cc, int I, float scale, int M, int N,
                int K, int lda, int ldb, int ldc, int out_f32, void* out, void* stream);
int mvd_op_cfg_assemble(mvd_ctx* ctx, const float* x_noisy, const float* x_input, const float* clip, const int64_t* timesteps, int B,
                        int TN, int HW, int dim, int copies, float* xin, float* ctx_out, int64_t* tt, void* stream);
int mvd_op_cfg_ddim(mvd_ctx* ctx, const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise, float s1m,
                    float sqrt_at, float sqrt_aprev, float dir_coef, float sigma, float* eps_out, float* x_prev, size_t n,
                    void* stream);
int mvd_op_small_mix(mvd_ctx* ctx, int op, const float* a, const float* b, const float* w, int i0, int i1, int i2, int i3, size_t n,
                     float* out, void* stream);
/* time of the dominant kernel, for bench.py: runs the 3x3 conv implicit GEMM `iters` times on stream and
 * returns the mean kernel time in ms measured with HIP events on that stream */
int mvd_bench_conv(mvd_ctx* ctx, int B, int C, int H, int W, int Cout, int iters, float* ms_out, void* stream);
/* First-stage decoder.  Replaces AutoencoderKL.decode (ldm/models/autoencoder.py:330-333 =
 * post_quant_conv + Decoder.forward, ldm/modules/diffusionmodules/model.py:535-568) for a batch of latents:
 * z [B, embed_dim, h, w] fp32 NCHW on the device (already divided by the 0.18215 scale factor, as
 * decode_first_stage does, morphable_diffusion.py:468-471) -> out [B, out_ch, 8h, 8w] fp32 NCHW.  Needs the
 * first_stage_model.decoder.* and first_stage_model.post_quant_conv.* tensors uploaded before finalize. */
int mvd_vae_decode(mvd_ctx* ctx, const float* z, int B, int h, int w, float* out, void* stream);
/* AutoencoderKL.encode(x).parameters (autoencoder.py:324-328 = Encoder.forward model.py:434-459 + quant_conv):
 * x [B, 3, H, W] fp32 NCHW in [-1,1] -> moments [B, 2*embed_dim, H/8, W/8] = (mean | logvar).  Sampling from the
 * posterior (DiagonalGaussianDistribution.sample / .mode) stays host code so the RNG stream is torch's.  Needs the
 * first_stage_model.encoder.* and first_stage_model.quant_conv.* tensors. */
int mvd_vae_encode(mvd_ctx* ctx, const float* x, int B, int H, int W, float* moments, void* stream);
/* CLIP image embedding.  Replaces FrozenCLIPImageEmbedder.forward
 * (ldm/modules/encoders/modules.py:373-379 = preprocess :363-371 + clip's VisionTransformer.forward) as
 * SyncMultiviewDiffusion.prepare calls it (morphable_diffusion.py:487-488): x [B, 3, H, W] fp32 NCHW in [-1,1] on the
 * device -> out [B, embed] fp32 (the caller adds FrozenCLIPImageEmbedder.encode's unsqueeze(1)).  Needs the
 * clip_image_encoder.model.visual.* tensors (openai/CLIP key names; geometry is read off their shapes,
 * heads = width / 64 as clip's build_model does) uploaded before finalize. */
int mvd_clip_encode(mvd_ctx* ctx, const float* x, int B, int H, int W, float* out, void* stream);
/* embedding width of the uploaded CLIP vision tower (768 for ViT-L/14), 0 when none was uploaded */
int mvd_clip_embed_dim(mvd_ctx* ctx);
/* In-situ per-kernel-family timing for the roofline report (bench.py).  While enabled, launches are bracketed by HIP events
 * on their launch stream and booked under the kernel's template instance ("gemm_dma_kernel<128,0>",
 * "conv3_dma_kernel<160,16,16>", "igemm_kernel<1,128>", "splitk_reduce_kernel", "group_norm", "layernorm", "attn_kernel",
 * "depth_attn_kernel") together with their ALGORITHMIC flops and bytes (each operand and the result once).
 * mode 0: off.  mode 1: every launch of every family (a survey pass: it perturbs the step, use it outside the timed region).
 * mode 2: only `family`, a deterministic pseudo-random 1-in-`stride` sample of its launches (for the timed region).
 * A non-zero mode resets the counters.  mvd_probe_report synchronises on the recorded events and writes a JSON array
 * [{"family", "launches", "sampled", "ms", "flops", "bytes", "all_flops", "all_bytes"}, ...] (ms / flops / bytes: the bracketed
 * launches; all_*: every launch seen) into buf.  In mode 1 the report also carries the pseudo-family "(empty bracket)": event
 * pairs with NOTHING between them, recorded after every 8th launch -- ms / sampled of that row is what a bracket adds to a
 * launch's own duration (the second event's barrier packet), for the caller to subtract. */
int mvd_probe_config(mvd_ctx* ctx, int mode, const char* family, int stride);
int mvd_probe_report(mvd_ctx* ctx, char* buf, size_t cap);
/* same for a Linear layer [M,K] x [N,K]^T (fp16 operands in HBM); flags: 1 = fp32 residual add, 2 = fp16 output,
 * 4 = GEGLU epilogue, 8 = bias, 16 = per-sample bias (32 samples), 32 = cold operands (a 768 MiB memset evicts the caches
 * before every launch and each launch is timed on its own), 64 = fp32 activations */
int mvd_bench_linear(mvd_ctx* ctx, int M, int K, int N, int flags, int iters, float* ms_out, void* stream);
/* same for GroupNorm(groups) + SiLU of a channels-last fp32 [B, HW, C] tensor -> fp16 (split: the [hi | lo | hi] operand
 * of an extended-precision consumer); flags: 1 = split output */
int mvd_bench_group_norm(mvd_ctx* ctx, int B, int C, int HW, int groups, int flags, int iters, float* ms_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
