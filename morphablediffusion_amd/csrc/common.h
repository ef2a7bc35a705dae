// Shared declarations for the gfx950 kernels and the host engine.  HIP only, wave64, no CUDA shims.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "env.h"

// The 16-bit MFMA operand type of the whole library.  Default build: IEEE fp16 (11-bit significand: what the inference parity
// bounds are stated for).  -DMVD_BF16 (make bf16 -> libmvd_hip_bf16.so, selected with MVD_DTYPE=bf16): bfloat16 operands and
// storage, fp32 accumulation and master weights -- BASELINE configs[3]'s training dtype (fp32 range: no loss scaling needed;
// same MFMA rate on gfx950).  Every kernel is written against `half_t` and the two MFMA macros only.
#ifdef MVD_BF16
typedef __bf16 half_t;
#define MVD_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#define MVD_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define MVD_DTYPE_NAME "bf16"
#else
typedef _Float16 half_t;
#define MVD_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#define MVD_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_f16
#define MVD_DTYPE_NAME "f16"
#endif
typedef half_t h8 __attribute__((ext_vector_type(8)));
typedef half_t h4 __attribute__((ext_vector_type(4)));
typedef half_t h2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// one element of an fp32 or a 16-bit source as fp32 (kernels templated on their source type: k_bwd.hip, k_cond_bwd.hip)
__device__ __forceinline__ float ldf(const float* p) { return *p; }
__device__ __forceinline__ float ldf(const half_t* p) { return (float)*p; }

#define MVD_MAX_TAPS 27

enum { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2 };

// ------------------------------------------------------------------------------------------------
// Implicit-GEMM descriptor:  out[row(m)][n] = epilogue( sum_{tap,c} A[in(m,tap)][c] * W[tap][n][c] )
// A is a channels-last activation tensor [B, PZ, PY, PX, lda] (fp16 or fp32) gathered through a
// tap table; W is fp16 [ntaps][N][Cin] (k-contiguous per output channel).
// ------------------------------------------------------------------------------------------------
// Which operand the workgroups of one XCD (one L2) should share.  Workgroup ids are dealt round-robin to the 8 XCDs and the kernels
// remap them so that an XCD owns a CONTIGUOUS range of tiles; walking that range row-tile-major makes an XCD re-use the activations
// of a few row tiles against every column group (all 8 L2s fill with all the weights), column-major the other way round.  Returns
// true when the column-major walk fills the L2s with clearly fewer bytes (deep levels: weights >> activations).
inline bool xcd_prefers_cols(int tiles_m, int groups_n, double a_bytes, double w_bytes) {
  const int nwg = tiles_m * groups_n, q = (nwg + 7) / 8;
  if (nwg < 16) return false;
  auto span = [](int q_, int inner, int outer) {  // distinct outer indices under q_ consecutive ids (inner index fastest), on average
    const double n = q_ % inner == 0 ? q_ / inner : (q_ - 1) / (double)inner + 1.0;
    return n < outer ? n : (double)outer;
  };
  const double at = a_bytes / tiles_m, wt = w_bytes / groups_n;
  const double row = at * span(q, groups_n, tiles_m) + wt * (q < groups_n ? q : groups_n);
  const double col = wt * span(q, tiles_m, groups_n) + at * (q < tiles_m ? q : tiles_m);
  return col < 0.8 * row;
}

struct IGemm {
  const void* a;        // activation base (channel offset already applied)
  int a_f32;            // 1: fp32 source (converted to fp16 while staging), 0: fp16 source
  int lda;              // elements between consecutive pixels
  int Cin;              // channels per tap (multiple of 8)
  int cin_alg;          // the layer's own channel count (Cin / 3 for extended-precision layers): algorithmic FLOP bookkeeping
  // logical output grid; M = B*Z*Y*X
  int B, Z, Y, X;
  // virtual input extent (after nearest upsample), strides, physical extent = virtual >> ups
  int IZ, IY, IX;
  int sz, sy, sx;
  int ups;
  int PZ, PY, PX;
  int ntaps;
  // per loop tap: (dz+1) | (dy+1)<<2 | (dx+1)<<4 | weight_slab<<8.  The weight slab is the tap's index in
  // the packed weights (identity except for the transposed-conv parity classes).
  int tap[MVD_MAX_TAPS];
  // weights
  const half_t* w;
  int N;                // GEMM N (before GEGLU halving)
  // output
  void* out;
  int out_f32;
  int ldc;
  int out_linear;       // 1: row offset = m*ldc ; 0: use the (OZ..oxo) mapping below
  int OZ, OY, OX, ozm, ozo, oym, oyo, oxm, oxo;
  // epilogue
  const float* bias;    // [N] or null
  const float* rowbias; // [B][rb_ld] or null (per-sample bias, e.g. timestep embedding)
  int rb_ld;
  const float* rowscale; // [B][rs_ld] or null: per-sample, per-column scale applied to the accumulator before the
  int rs_ld;             // biases (a GroupNorm folded into the GEMM that produces its input)
  // statistics-only pass (LDS-DMA kernel): nothing is stored; every 256-row tile writes (sum, sumsq) of the
  // accumulators per GroupNorm group to gn_partial[(m0/256) * (N/gn_cpg) + group][2].  Needs N % gn_cpg == 0,
  // gn_cpg in {8,16,32} and rows-per-sample % 256 == 0.
  float* gn_partial;
  int gn_cpg;
  const void* resid;    // same row mapping / ld as out, or null
  int resid_f32;
  int ldr;
  int out_split;        // fp16 output only, 0 or the logical width C: column n is written three times, as
                        // hi = fp16(v) at n and n + 2C and lo = fp16(v - hi) at n + C (ldc >= 3C): the [hi | lo | hi] operand
                        // of an extended-precision consumer (see ConvW::xp)
  int geglu;            // pairs 32-column blocks (x | gate): out cols = N/2
  float alpha;          // scale on the accumulator before bias
  int act;              // ACT_SILU applied last (non-GEGLU path)
  // split-K
  int nch;              // dense GEMM kernel: column tiles walked by one workgroup
  int xcd_cols;         // set by the launchers (xcd_prefers_cols): an XCD's workgroups share COLUMN tiles (weights) instead of row tiles
  // parity-batched launch (LDS-DMA kernel only): blockIdx.z picks one of npar tap tables / output offsets, so the
  // 8 parity classes of a transposed conv (or the 4 of a folded upsample conv) are ONE launch
  int npar;
  int par_ntaps[8];
  int par_tap[8][8];
  int par_oz[8], par_oy[8], par_ox[8];
  int par_walk;         // LDS-DMA kernel: one workgroup walks the npar classes of its tile (grid.z = 1) instead of one per class
  const half_t* wx;     // the same weights as a conv3x fragment stream (k_conv3x.hip) packed for column tiles of wx_bn, or null
                        // (27 taps: the conv3z stream, wx_bn 64 or 128)
  int wx_bn;
  int bn;               // column-tile width (64 / 96 / 128 / 160); 0 = pick from N
  int bm;               // LDS-DMA GEMM only: row-tile height, 256 (0 = 256: eight waves) or 128 (four waves; plain GEMMs)
  int splitk;
  float* partial;       // [splitk][M][N] fp32 when splitk > 1
};

struct MvdStream {
  hipStream_t s;
};

#define HIP_CHECK_RET(expr)                                        \
  do {                                                             \
    hipError_t _e = (expr);                                        \
    if (_e != hipSuccess) return mvd_fail(hipGetErrorString(_e));  \
  } while (0)

int mvd_fail(const char* msg);  // records thread-local error text, returns -1
const char* mvd_error_text();

#define MVD_MAX_DEVICES 64
static inline int mvd_current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MVD_MAX_DEVICES) d = 0;
  return d;
}
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int igemm_tap(int dz, int dy, int dx, int slab) { return (dz + 1) | ((dy + 1) << 2) | ((dx + 1) << 4) | (slab << 8); }

// ---- kernel launchers (defined in the .hip files) -------------------------------------------------
int launch_igemm(const IGemm& g, hipStream_t s);
int igemm_pick_bn(int N, int geglu);
int launch_splitk_reduce(const IGemm& g, hipStream_t s);
bool conv3_halo_eligible(const IGemm& g);
int conv3_halo_tiles(const IGemm& g, int bn);
int launch_conv3_halo(const IGemm& g, hipStream_t s);
int igemm_pick_splitk(int M, int N, int ksteps, int bn);
bool conv3x_eligible(const IGemm& g, int bn);
size_t conv3x_stream_halfs(int N, int Cin, int bn);
int conv3x_pack(const half_t* w, int N, int Cin, int bn, half_t* stream, hipStream_t s);
int launch_conv3x(const IGemm& g, const half_t* stream, int bn, hipStream_t s);
// the 3 x 3 x 3 stride-1 form of the same kernel (k_conv3x.hip, conv3z): hard limits, stream size / pack (bn 64 or 128), launch
constexpr int CONV3D_DMA_MAX_M = 16384;  // rows up to which igemm_go sends a 27-tap layer to the LDS-DMA tap gather
int conv3z_stream_bn(int taps, int N, int Cin);  // the column tile a layer's conv3z stream is packed for, 0: the layer gets none
bool conv3z_eligible(const IGemm& g, int bn);
size_t conv3z_stream_halfs(int N, int Cin, int bn);
int conv3z_pack(const half_t* w, int N, int Cin, int bn, half_t* stream, hipStream_t s);
int launch_conv3z(const IGemm& g, const half_t* stream, int bn, hipStream_t s);
bool gemm_dma_eligible(const IGemm& g);
bool gemm_dma_is_plain(const IGemm& g);
void gemm_dma_plan(int M, int N, int ksteps, int bn, int geglu, int* nch_out, int* splitk_out);
int launch_target_encoder(const float* x, const float* pre, int n_views, const half_t* const* w, const float* const* bias,
                          const int* cin, const float* const* gamma, const float* const* beta, float* feats, hipStream_t s);
void gemm_dma_plan_us(int M, int N, int ksteps, int geglu, int out_b, int res_b, int* bn_io, int* nch_out, int* splitk_out,
                      int* bm_out = nullptr);
int launch_gemm_dma(const IGemm& g, hipStream_t s);

int launch_gn_stats(const float* x, int ld, int B, int rows_per_sample, int C, int G, const float* preadd, int pld,
                    float* partial, int* nslabs_out, hipStream_t s);
int launch_gn_apply(const float* x, int ld, int B, int rows_per_sample, int C, int G, const float* preadd, int pld,
                    const float* partial, int nslabs, const float* gamma, const float* beta, float eps, int act,
                    half_t* out, int ldo, hipStream_t s, int split = 0);
int gn_max_slabs();
// slab / tile partials [B][nslabs][G][2] -> per-sample scale[c] = rstd*gamma, shift[c] = beta - mean*rstd*gamma
int launch_gn_finalize(const float* partial, int B, int nslabs, int rows_per_sample, int C, int G, const float* gamma,
                       const float* beta, float eps, float* scale, float* shift, int ld, hipStream_t s);
bool gn_group_eligible(int ld, int rows, int C, int G, int pld, int ldo);
// split != 0: out rows hold [hi | lo | hi] (3C halfs, ldo >= 3C), see IGemm::out_split
int launch_gn_group(const float* x, int ld, int B, int rows, int C, int G, const float* preadd, int pld, const float* gamma,
                    const float* beta, float eps, int act, half_t* out, int ldo, hipStream_t s, int split = 0,
                    int nslab = 1, size_t slab_stride = 0, const float* bias2 = nullptr, const float* resid = nullptr, int ldr = 0,
                    float* mat = nullptr, int ldm = 0);
// raw (optional): x itself as fp16, rows ld_raw halfs apart (widths 320 / 640 / 1280 / 2560, 16-byte aligned)
int launch_layernorm(const float* x, int rows, int C, const float* gamma, const float* beta, float eps,
                     half_t* out, hipStream_t s, half_t* raw = nullptr, int ld_raw = 0);
bool layernorm_slabs_takes(int C);
// x = nslab split-K slabs [rows][C] (slab_stride floats apart): their sum + bias + rowbias[row / T] + resid is written to mat (fp32)
// and normalised into out (fp16): the producing GEMM's reduce pass and the LayerNorm in one launch
int launch_layernorm_slabs(const float* slabs, int nslab, size_t slab_stride, int rows, int C, const float* bias, const float* rowbias,
                           int rb_ld, int T, const float* resid, int ldr, float* mat, const float* gamma, const float* beta, float eps,
                           half_t* out, hipStream_t s, half_t* raw = nullptr, int ld_raw = 0);
int launch_layernorm_f32(const float* x, long ldx, int rows, int C, const float* gamma, const float* beta, float eps,
                         float* out, hipStream_t s);
// q | k rows at `qk` (k at column offset heads*d), V row-major at `v` (row strides ldqk / ldv: all three normally live
// in one fused projection buffer).  Tstride (0 = T): rows between consecutive samples when the token axis is padded
// (CLIP: 257 tokens in 264 rows).  xcd: the XCD remap of the workgroup index, -1 = as MVD_ATTN_NO_XCD says, 0 / 1 = off / on (the
// parity hook's A/B: the results are bit-identical)
int launch_attention(const half_t* qk, int ldqk, const half_t* v, int ldv, half_t* out, int ldo, int B, int T, int heads,
                     int d, hipStream_t s, int Tstride = 0, int xcd = -1);
int launch_clip_patches(const float* img, int B, int H, int W, int S, int P, int Kp, half_t* out, hipStream_t s);
int launch_clip_tokens(const float* pe, const float* cls, const float* pos, int B, int T, int Tp, int C, float* x,
                       hipStream_t s);
int launch_scale_copy(const float* src, size_t n, float k, float* dst, hipStream_t s);
int launch_softmax_rows(const float* s, long rows, int cols, half_t* p, hipStream_t st);
int launch_softmax_rows_f32(const float* s, long rows, int cols, float* p, hipStream_t st);
// ldx (0 = Cc): halfs between consecutive rows of ctxn (the block's column slice of a context fold shared by one level)
int launch_depth_attn(const float* qk, const half_t* ctxn, half_t* z, int n_cond, int HW, int D, int Cc, int heads,
                      hipStream_t s, int split = 0, int nfill = 0, const half_t* fill_row = nullptr, int ldx = 0);
int depth_attn_check(int D, int Cc, int heads, int ldx, int nfill);  // the launcher's shape check alone: 0, or mvd_fail
int launch_small_linear(const float* a, int lda, int rows, int K, const half_t* w, const float* bias, int N,
                        int act_in, float* out, int ldo, int accumulate, hipStream_t s);
int small_linear_form(const float* a, int lda, int K, const half_t* w);  // the path launch_small_linear takes: 1 vector, 0 scalar
int launch_timestep_embedding(const int64_t* t, int B, int dim, float* out, hipStream_t s);
int launch_nchw_to_nhwc(const float* in, int B, int C, int HW, float* out, int ldo, int cpad, hipStream_t s);
int launch_nhwc_to_nchw(const float* in, int ld, int B, int C, int HW, float* out, hipStream_t s);
int layout_form(int B, int C, int HW, int cols);  // the two launchers above: 1 LDS-tiled kernel, 0 element kernel (cols: cpad / C)
int pack_weight_form(int N, int Cin, int taps, int transposed, const half_t* dst, int xp);  // 0 element, 1 per-tap, 2 per-tap vector
// xp != 0: Cin is the packed width 3 * Cl and each row holds [w_hi | w_hi | w_lo] (w_hi = fp16(w), w_lo = fp16(w - w_hi))
int launch_pack_weight(const float* src, int N, int Cin, int taps, int transposed, int geglu, half_t* dst,
                       hipStream_t s, int cin_src = -1, int xp = 0);
// fp32 rows -> fp16 [hi | lo | hi] rows of 3C halfs
int launch_rows_f32_to_f16_split(const float* in, int lda, long rows, int C, half_t* out, hipStream_t s);
int launch_permute_geglu_bias(const float* src, int N, float* dst, hipStream_t s);
int launch_f32_to_f16(const float* in, half_t* out, size_t n, hipStream_t s);
int launch_rows_f32_to_f16(const float* in, int lda, long rows, int C, half_t* out, hipStream_t s);
int launch_pack_upconv_weight(const float* src, int N, int Cin, half_t* dst, hipStream_t s);
int launch_fill_rows_f16(half_t* out, int ld, int rows, const half_t* vec, int n, hipStream_t s);
int launch_fold_qk(const float* wq, const float* wk, int heads, int hd, int Cc, int I, float scale, half_t* out,
                   hipStream_t s, float* out32 = nullptr);
int launch_fold_ov(const float* wo, const float* wv, int heads, int hd, int Cc, int I, half_t* out, hipStream_t s,
                   float* out32 = nullptr);
// C[m][n] = sum_k A[m][k] B[k][n] in fp64 (row-major fp32 operands, row strides lda / ldb), written as fp16 (out16, row stride ldc)
// or fp32 (out32, row stride ldc): weight folds at finalize time
int launch_fold_mm(const float* a, int lda, const float* b, int ldb, int M, int N, int K, half_t* out16, int ldc, float* out32,
                   hipStream_t s);
int launch_relu_beta_tile(const float* beta, int Cc, int heads, half_t* out, hipStream_t s, int split = 0);
int launch_cfg_ddim(const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise,
                    float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float dir_coef, float sigma,
                    float* eps_out, float* x_prev, size_t n, hipStream_t s);
// the samplers' UNet batch assembly (c_api.hip: build_cfg_input_kernel + build_cfg_context_kernel per sample); timesteps: host
int launch_build_cfg_batch(const float* x_noisy, const float* x_input, const float* clip, const int64_t* timesteps, int B, int TN, int HW,
                           int dim, int copies, float* xin, float* ctx, int64_t* tt, hipStream_t s);
// DPM-Solver++ multistep update coefficients of one step (schedule.py DPMSolverSchedule.rows)
struct DpmCoef {
  float s1m, sqrt_at, c_x, c_d, c_c, c_n;
};
// CFG combine + x0 prediction + x_next = c_x x + c_d x0 + c_c (x0 - x0_hist) + c_n noise, x0 -> x0_hist (in place);
// x0_hist is not read when use_hist == 0; eps_u / noise / eps_out may be null
int launch_cfg_dpm(const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise, DpmCoef k,
                   float* x0_hist, int use_hist, float* eps_out, float* x_next, size_t n, hipStream_t s);
// conditioner
struct ViewCam {
  float P[12];     // 3x4 projection into the size x size feature map (rows of the 4x4 minus the last)
  float Pinv[12];  // 3x4 inverse mapping (perspective: inv(P); orthographic: see engine)
  float Kinv[9];   // orthographic only
  float near_, far_;
};
int launch_vertex_gather(const float* feats, const ViewCam* cams, const int* view_idx, int n_views, const float* verts, int Nv, int V,
                         float vol_len, int fsize, int persp, float* out, hipStream_t s);
int launch_unproject_views(const float* feats, const ViewCam* cams, int N, int V, float vol_len, int S, int persp, half_t* out,
                           hipStream_t s);
int launch_rows_f16_to_nchw(const half_t* in, long rows, int C, float* out, hipStream_t s);
int launch_accumulate_f32(float* dst, const float* src, size_t n, hipStream_t s);
int launch_fuse_views(const float* vf, int n_views, int Nv, int total_views, const float* w, const float* b,
                      float* out, int accumulate, hipStream_t s);
// w: [27][Cin][Cout]; wp: the same weights as matrix-core B fragments (launch_sparse_w_frag) or null -> one-site-per-workgroup kernel
int launch_sparse_conv(const float* in, const int* nbr, int n_out, int Cin, int Cout, const float* w, const float* wp,
                       const float* scale, const float* shift, float* out, hipStream_t s, int mask_nonrep = 0);
bool sparse_mfma_takes(int Cin, int Cout);
int launch_sparse_w_frag(const float* w, int Cl_in, int Cl_out, int transposed, int flip, float* dst, hipStream_t s);
// BatchNorm1d in train mode over n rows of C <= 256 channels + ReLU, in place: x = relu((x - mean) / sqrt(var + eps) * g + b),
// biased variance (what F.batch_norm normalises with)
int launch_sparse_w_pack(const float* src, int Cin, int Cout, int layout, float* dst, hipStream_t s);
int launch_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C, float* scale,
                   float* shift, hipStream_t s);
int launch_bn_rows_relu(const float* x, float* y, int n, int C, const float* gamma, const float* beta, float eps, float* stats_out,
                        hipStream_t s, float* rmean = nullptr, float* rvar = nullptr, float momentum = 0.f);
int launch_mse(const float* a, const float* b, size_t n, float* out, hipStream_t s);
// k_loss.hip: the weighted / masked / Huber training objective on channels-last [B][HW][C] (include/mvd.h: mvd_op_train_loss).
// train_loss_check: the argument errors (0 = fine); scratch: train_loss_scratch_bytes(B, HW) bytes, 8-byte aligned, alive until the
// launches have run.  w [B], m [B][HW], dpred and the three outputs may be null.
size_t train_loss_scratch_bytes(int B, int HW);
int train_loss_check(const char* who, int B, int HW, int C, int loss_type, float huber_delta);
int launch_train_loss(const float* pred, const float* target, int B, int HW, int C, const float* w, const float* m, int loss_type,
                      float huber_delta, float loss_scale, float* dpred, float* loss_out, float* loss_ps, float* mse_ps, void* scratch,
                      hipStream_t s);
// k_metrics.hip: SSIM / squared / absolute error of 8-bit views (include/mvd.h: mvd_op_image_metrics).  dtype 0 float32, 1 uint8;
// layout 0 [V][3][H][W], 1 [V][H][W][3]; mask [V][H][W] (mode 1).  image_metrics_check: the argument errors (0 = fine); scratch:
// image_metrics_scratch_bytes(V, H, W) bytes, 8-byte aligned, alive until the launches have run; out [V][5] doubles.
size_t image_metrics_scratch_bytes(int V, int H, int W);
int image_metrics_check(const char* who, const void* pred, int pred_dtype, int pred_layout, const void* target, int target_dtype,
                        int target_layout, const unsigned char* mask, int mask_mode, int V, int H, int W, const double* out);
int launch_image_metrics(const void* pred, int pred_dtype, int pred_layout, const void* target, int target_dtype, int target_layout,
                         const unsigned char* mask, int mask_mode, int V, int H, int W, double* out, void* scratch, hipStream_t s);
// k_mesh.hip: mesh texturing from views (include/mvd.h: mvd_op_mesh_project / _raster / _vertex_colors).  The *_check functions
// are the argument errors (0 = fine).  xy [N][Nv][2] / key [N][Nv]: 1/16-pixel screen coordinates and depth keys (0 = invalid);
// face_id / pix_key [N][H][W]; raster scratch: mesh_raster_scratch_bytes(N, H, W) bytes, 8-byte aligned, alive until the launches
// have run; bad_faces: one device int, the faces with an index outside [0, Nv); visible [N][Nv] bytes may be null.
int mesh_project_check(const char* who, const float* verts, const float* K, const float* RT, int N, int Nv, float z_near, const int* xy,
                       const int* key);
int launch_mesh_project(const float* verts, const float* K, const float* RT, int N, int Nv, float z_near, int* xy, int* key, hipStream_t s);
int mesh_raster_check(const char* who, const int* xy, const int* key, const int* faces, int N, int Nv, int Nf, int H, int W,
                      const int* face_id, const int* pix_key, const int* bad_faces);
size_t mesh_raster_scratch_bytes(int N, int H, int W);
int launch_mesh_raster(const int* xy, const int* key, const int* faces, int N, int Nv, int Nf, int H, int W, int* face_id, int* pix_key,
                       int* bad_faces, void* scratch, hipStream_t s);
int mesh_vertex_colors_check(const char* who, const void* images, int dtype, int layout, const int* xy, const int* key, const int* faces,
                             const int* face_id, const int* pix_key, const float* verts, const float* normals, const float* centres, int N,
                             int Nv, int Nf, int H, int W, float power, const float* color, const float* weight_sum, const int* n_seen,
                             const float* spread);
int launch_mesh_vertex_colors(const void* images, int dtype, int layout, const int* xy, const int* key, const int* faces, const int* face_id,
                              const int* pix_key, const float* verts, const float* normals, const float* centres, int N, int Nv, int Nf,
                              int H, int W, float power, int bias, int two_sided, float fill_r, float fill_g, float fill_b, float* color,
                              float* weight_sum, int* n_seen, float* spread, unsigned char* visible, hipStream_t s);
// k_mesh_uv.hip: UV texture atlases (include/mvd.h: mvd_op_mesh_vertex_normals / _texel_bake / _texture_dilate / _render_uv).  The
// *_check functions are the argument errors (0 = fine) and touch no device.  MeshBakeArgs holds the arguments of
// mvd_op_mesh_texel_bake as the header names them; visible / pos / txy / tkey may be null.
struct MeshBakeArgs {
  const void* images;
  const int *face_id, *pix_key, *faces, *uv_xy, *face_uv, *tex_face;
  const float *K, *RT, *centres, *verts, *normals;
  int dtype, layout, N, Nv, Nf, Nt, H, W, Ht, Wt, bias, two_sided;
  float z_near, power, fill[3];
  float *texture, *weight_sum, *spread, *pos;
  int *n_seen, *txy, *tkey;
  unsigned char* visible;
};
int mesh_vertex_normals_check(const char* who, const float* verts, const int* faces, const int* inc_ptr, const int* inc_face, int F, int Nv,
                              int Nf, const float* normals, const int* bad_faces);
int launch_mesh_vertex_normals(const float* verts, const int* faces, const int* inc_ptr, const int* inc_face, int F, int Nv, int Nf,
                               float* normals, int* bad_faces, hipStream_t s);
int mesh_texel_bake_check(const char* who, const MeshBakeArgs& a);
int launch_mesh_texel_bake(const MeshBakeArgs& a, hipStream_t s);
int mesh_texture_dilate_check(const char* who, const float* texture, const unsigned char* valid, int Ht, int Wt, int passes,
                              const float* texture_out, const unsigned char* valid_out);
size_t mesh_texture_dilate_scratch_bytes(int Ht, int Wt);
int launch_mesh_texture_dilate(const float* texture, const unsigned char* valid, int Ht, int Wt, int passes, float* texture_out,
                               unsigned char* valid_out, void* scratch, hipStream_t s);
int mesh_render_uv_check(const char* who, const int* xy, const int* key, const int* face_id, const int* faces, const int* face_uv,
                         const float* uv, const float* texture, int N, int Nv, int Nf, int Nt, int H, int W, int Ht, int Wt, int layout,
                         const float* images);
int launch_mesh_render_uv(const int* xy, const int* key, const int* face_id, const int* faces, const int* face_uv, const float* uv,
                          const float* texture, int N, int Nv, int Nf, int Nt, int H, int W, int Ht, int Wt, int layout, float bg_r, float bg_g,
                          float bg_b, float* images, hipStream_t s);
// k_morph.hip: the morphable-model forward (include/mvd.h: mvd_op_morph_pose / _skin / _landmarks).  The *_check functions are the
// argument errors (0 = fine) and touch no device; parents [J] is a HOST array, copied into the pose kernel's argument struct.
// pose_feature [F][9 (J - 1)] may be null when J == 1, post [12] may be null; everything else is a device buffer of the caller.
constexpr int MORPH_MAX_JOINTS = 64;
int morph_pose_check(const char* who, const float* betas, const float* pose, const float* j_template, const float* j_dirs,
                     const int* parents, int F, int NB, int J, const float* j_rest, const float* rot, const float* pose_feature,
                     const float* joints, const float* A);
int launch_morph_pose(const float* betas, const float* pose, const float* j_template, const float* j_dirs, const int* parents, int F,
                      int NB, int J, float* j_rest, float* rot, float* pose_feature, float* joints, float* A, hipStream_t s);
int morph_skin_check(const char* who, const float* basis, const float* v_template, const float* coef, const float* weights,
                     const float* A, int F, int V, int L, int NB, int J, const float* verts);
int launch_morph_skin(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                      const float* post, int F, int V, int L, int J, float* verts, hipStream_t s);
int morph_landmarks_check(const char* who, const float* verts, const int* faces, const int* lmk_face, const float* lmk_bary, int F, int V,
                          int Nf, int M, const float* out);
int launch_morph_landmarks(const float* verts, const int* faces, const int* lmk_face, const float* lmk_bary, int F, int V, int Nf, int M,
                           float* out, hipStream_t s);
int launch_latent_gather(const float* feats, const int* grid, int gd, int gh, int gw, const float* min_xyz,
                         const int* out_sh, float voxel, int V, float vol_len, float* out, hipStream_t s);
int launch_sparse_densify(const float* feats, const int* grid, long nvox, int C, float* out, hipStream_t s);
int launch_frustum_gather(const float* vol, const ViewCam* cams, const int* view_idx, int TN, int D, int S, int V,
                          float vol_len, int persp, half_t* out, hipStream_t s);
int launch_bits_checksum(const void* p, size_t bytes, unsigned long long* out, hipStream_t s);
int launch_add_rows(float* dst, const float* a, const float* b, size_t n, hipStream_t s);
// out[(b * HW + p) * ldo + c] = in[(b * HW + p) * ldi + c] + img[p * C + c] for b < nb (C, ldi, ldo multiples of 4)
int launch_add_image_rows(const float* in, int ldi, const float* img, int C, int nb, int HW, float* out, int ldo, hipStream_t s);
// nearest x2 upsample + fp16 cast: in fp32 [B][H][W][ldi] -> out fp16 [B][2H][2W][C]
int launch_upsample2_f16(const float* in, int ldi, int B, int H, int W, int C, half_t* out, hipStream_t s);
// 3 x 3, pad 1, stride 1 convolution of a channels-last fp32 image batch with 4 or 8 input channels, in exact fp32 on the vector ALU:
// x [B][H][W][ldx], w [N][cin_src][3][3] (the checkpoint's layout), out [B][H][W][ldo] (+ bias)
int launch_conv_in_f32(const float* x, int ldx, const float* w, int cin_src, const float* bias, int N, int B, int H, int W, float* out,
                       int ldo, hipStream_t s);
// 3 x 3, pad 1, stride 1 convolution C -> N <= 4 of a channels-last fp32 image batch in exact fp32 on the vector ALU (the UNet's
// output head): a [B][H][W][C], w [N][C][3][3] (the checkpoint's layout), out [B][H][W][ldo] (+ bias).  C % 32 == 0, W % 16 == 0.
int launch_out_conv_f32(const float* a, int C, const float* w, const float* bias, int N, int B, int H, int W, float* out, int ldo,
                        hipStream_t s);
int launch_probe_null(hipStream_t s);  // one wave that does nothing: the launch path's own cost (ProbeScope calibration)
// ---- training: backward / adjoint launchers -----------------------------------------------------
// k_bwd.hip
int bwd_tcast(const void* src, int src_f32, long ld, int R, int C, half_t* dst, int Rp, hipStream_t s, int split = 0, half_t* rows16 = nullptr,
              int Cp = 0);
int bwd_im2colT(const void* src, int src_f32, long ld, int B, int H, int W, int C, int stride, int ups, half_t* dst, int Rp, hipStream_t s);
int bwd_cast_rows(const float* src, long ld, long rows, int C, int Cp, half_t* dst, hipStream_t s, int split = 0);
int bwd_pack_dgrad(const half_t* w, int taps, int N, int ldw, int Cl, int Np, half_t* wT, hipStream_t s, int flip = 1);
int bwd_group_norm(const float* x, long ld, const float* pre, int pld, const float* dy, long ldy, int B, int rows, int C, int G,
                   const float* gamma, const float* beta, float eps, int act, float* dx, long lddx, int accum, float* dg_part,
                   float* db_part, float* dpre_part, hipStream_t s);
int bwd_sum_rows_add(const float* part, int R, int C, long ldp, float* out, int accum, hipStream_t s);
int bwd_sum_rows_multi(int n, const float* const* part, const int* R, const int* C, const long* ldp, float* const* out, const int* accum,
                       hipStream_t s);
int bwd_gn_slabs(int B, int G, int rows);
int bwd_group_norm_fwd(const float* x, long ld, int B, int rows, int C, int G, const float* gamma, const float* beta, float eps, int act,
                       float* y, long ldy, float* part, int S, hipStream_t s);
int bwd_group_norm_slab(const float* x, long ld, const float* pre, int pld, const float* dy, long ldy, int B, int rows, int C, int G,
                        const float* gamma, const float* beta, float eps, int act, float* dx, long lddx, int accum, float* part,
                        float* part2, float* dg_part, float* db_part, float* dpre_part, int S, hipStream_t s);
int bwd_outer_add(const float* a, long lda, const float* b, long ldb, float* C, int M, int N, int K, hipStream_t s);
int bwd_colsum_samples(const void* v, int v_f32, long ld, int B, int rows, int C, float* out, long ldo, hipStream_t s);
int bwd_ln_max_blocks();
int bwd_layer_norm(const float* x, long ld, const float* dy, long ldy, int rows, int C, const float* gamma, float eps, float* dx,
                   long lddx, int accum, float* part, int* nblk, hipStream_t s);
int bwd_geglu(const half_t* pre, const float* dgg, long ldg, long rows, int N, half_t* dpre, hipStream_t s);
int bwd_geglu_unpermute_add(const float* src, int N, int C, float* dst, hipStream_t s);
int bwd_add_views(float* out, long ldo, const float* a, long lda, const float* b, long ldb, long rows, int C, int accum, hipStream_t s);
int bwd_upsample2(const float* dup, int B, int H, int W, int C, float* dx, long lddx, int accum, hipStream_t s);
int bwd_col2im3(const float* dcol, int B, int H, int W, int C, int stride, float* dx, long lddx, int accum, hipStream_t s);
int bwd_silu_inplace(float* g, const float* u, size_t n, hipStream_t s);
int bwd_attention(const half_t* qkv, int ld3, const half_t* o, const half_t* dO, int ldo, half_t* dqkv, int ldd, float* lse, float* delta,
                  int B, int T, int heads, int d, hipStream_t s);
int bwd_silu_fwd(const float* u, float* out, size_t n, hipStream_t s);
int bwd_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, float wd, int step,
              float inv_scale, const int* skip, hipStream_t s);
int bwd_finite_check(const float* g, size_t n, int* flag, hipStream_t s);
// global-norm clipping + EMA (k_bwd.hip): deterministic two-stage sum of squares, the fused step, the arena exchange
int bwd_grad_sumsq_blocks(size_t n);
int bwd_grad_sumsq(const float* g, size_t n, float inv_scale, float* partial, hipStream_t s);
int bwd_grad_norm_final(const float* partial, int count, float max_norm, float* out, int* flag, hipStream_t s);
int bwd_adamw_ex(float* p, const float* g, float* m, float* v, float* e, size_t n, float lr, float beta1, float beta2, float eps, float wd,
                 int step, float inv_scale, const float* clip, float ema_decay, const int* skip, hipStream_t s);
int bwd_swap_f32(float* a, float* b, size_t n, hipStream_t s);
// k_lora.hip: low-rank adapters W0 + s B A (A [r][in], B [out][r]) on fp32 arenas.  One table entry per adapted tensor; offsets in
// floats: w_off into the arena of dW / W, w0_off into the compact copy of the adapted tensors, a_off / b_off into the adapter
// arenas, pa_off / pb_off into the projection's partial-sum workspace.  tile0 / red0: the target's first workgroup in the tile
// launches (LORA_TILE_O x LORA_TILE_I tiles, row-tile major) and in the projection's reduce launch (lora_plan fills the last four).
#define LORA_MAX_RANK 64
#define LORA_TILE_O 32
#define LORA_TILE_I 128
struct LoraTarget {
  long long w_off, w0_off, a_off, b_off, pa_off, pb_off;
  int out, in, tile0, red0;
};
void lora_plan(LoraTarget* tab, int n, int r, int* tiles, int* red_blocks, size_t* part_floats);
// gA = scale B^T dW, gB = scale dW A^T for every target (overwritten; two launches, no atomic, bit-reproducible)
int lora_project(const LoraTarget* tab, int n, int tiles, int red_blocks, const float* dW, const float* A, const float* B, int r,
                 float scale, float* part, float* gA, float* gB, hipStream_t s);
// W = W0 + scale B A for every target: exactly out x in elements each
int lora_merge(const LoraTarget* tab, int n, int tiles, const float* W0, const float* A, const float* B, int r, float scale, float* W,
               hipStream_t s);
// k_cond_bwd.hip
int cbwd_frustum_scatter(const float* d_out, const ViewCam* cams, const int* view_idx, int TN, int D, int S, int V, float vol_len, int persp,
                         float* d_vol, hipStream_t s);
int cbwd_latent_scatter(const float* d_vol, const int* grid, int gd, int gh, int gw, const float* min_xyz, const int* out_sh, float voxel,
                        int V, float vol_len, float* d_rows, hipStream_t s);
int cbwd_vertex_scatter(const float* d_out, const ViewCam* cams, const int* view_idx, int n_views, const float* verts, int Nv, int V,
                        float vol_len, int S, int persp, float* d_feats, hipStream_t s);
// the same adjoints as gathers (deterministic mode): no floating-point atomics, outputs written, not accumulated into
int cbwd_frustum_gather_adj(const float* d_out, const ViewCam* cams, const int* view_idx, int TN, int D, int S, int V, float vol_len,
                            int persp, float* pos, float* d_vol, hipStream_t s);
int cbwd_latent_gather_adj(const float* d_vol, const int* grid, int gd, int gh, int gw, const float* min_xyz, const int* out_sh, float voxel,
                           int V, float vol_len, float* d_rows, hipStream_t s);
size_t cbwd_vertex_adj_scratch_bytes(int n_views, int Nv, int V);
int cbwd_vertex_gather_adj(const float* d_out, const ViewCam* cams, const int* view_idx, int n_views, const float* verts, int Nv, int V,
                           float vol_len, int S, int persp, void* scratch, float* d_feats, hipStream_t s);
int cbwd_lattice_to_views_adj(const float* d_lat, const ViewCam* cams, const int* view_idx, int n_views, const int* vox_list,
                              const int* n_ptr, int n_max, int V, float vol_len, int S, int persp, float4* rec, float* d_feats,
                              hipStream_t s);
int cbwd_sparse_fold_dups_det(float* d, const int* nbr, int n, int C, int* flag, hipStream_t s);
int cbwd_fuse_scratch_floats(int Nv);
int cbwd_fuse(const float* d_fused, const float* vf, const float* w, int n_views, int Nv, int total_views, float* d_vf, float* dw, float* db,
              float* part, hipStream_t s);
int cbwd_bn_scratch_floats(int n, int C);
int cbwd_bn_rows_relu(const float* xraw, float* dy, int n, int C, const float* gamma, const float* beta, const float* stats,
                      float* scratch, float* dgamma, float* dbeta, hipStream_t s);
int cbwd_sparse_wgrad_chunks(int n_out);
int cbwd_sparse_conv(const float* in, const int* nbr, const float* d_out, int n_out, int Cin, int Cout, const float* w, float* d_in,
                     float* dw_packed, float* dw_part, hipStream_t s);
int cbwd_sparse_w_unpack_add(const float* pk, int Cin, int Cout, int layout, float* dst, hipStream_t s);
int cbwd_sparse_wgrad_mfma(const float* in, const int* nbr, const float* d_out, int n_out, int Cin, int Cout, float* dw_packed,
                           float* dw_part, hipStream_t s);
int cbwd_sparse_inverse_table(const int* nbr_down, int n_out, int n_in, int* inv, hipStream_t s);
int cbwd_sparse_fold_dups(float* d, const int* nbr, int n, int C, hipStream_t s);
// one sparse layer's conv backward (k_cond_bwd.hip): its scratch in elements (dwp / dw_part floats, flag / inv ints; 0 = not used)
struct SparseLayerScratch {
  size_t dwp, dw_part, flag, inv;
};
SparseLayerScratch cbwd_sparse_layer_scratch(int n_in, int n_out, int Cin, int Cout, bool strided, bool lvl0_subm, bool det, bool mfma);
int cbwd_sparse_layer(const float* in, const int* nbr, float* d_out, int n_in, int n_out, int Cin, int Cout, bool strided, bool lvl0_subm,
                      bool det, const float* w, const float* wd, int layout, float* dwp, float* dw_part, int* flag, int* inv, float* d_in,
                      float* gw, hipStream_t s);
int cbwd_im2colT3d(const void* src, int src_f32, long ld, int B, int D, int H, int W, int C, int stride, half_t* dst, int Rp, hipStream_t s);
int cbwd_small_linear_bwd(const float* g, long ldg, int rows, int N, const half_t* w, int K, float* out, long ldo, int accum, hipStream_t s);
// k_train.hip
int train_im2col3(const float* X, int B, int H, int W, int C, float* col, hipStream_t s);
int train_col2im3(const float* dcol, int B, int H, int W, int C, float* dX, hipStream_t s);
int train_perm_w3(const float* src, int N, int C, int to_mat, float* dst, hipStream_t s);
int train_depth_fwd(const float* q, const float* k, const float* v, int R, int HW, int D, int hn, int hd, float scale, float* attn,
                    float* z, hipStream_t s);
int train_depth_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dz, int R, int HW, int D, int hn,
                    int hd, float scale, float* dq, float* dk, float* dv, hipStream_t s);
int train_add_inplace(float* a, const float* b, size_t n, hipStream_t s);
int train_copy_rows(const float* src, int ld, long rows, int C, float* dst, hipStream_t s);
int train_add_bias_rows(float* x, long rows, int C, const float* bias, hipStream_t s);
