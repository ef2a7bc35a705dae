// Every environment variable libmvd_hip.so reads, once.  None is needed in normal use: they select equivalent forms of a
// computation for A/B runs and bisection, sweep tile plans, or turn on host-side timing and debugging.  DESIGN.md section 5
// lists them for readers; tests/test_host_cpu.py holds that list, and every MVD_* name that tests/, tools/ and the Python
// package set, against this table -- and checks that no other file under csrc calls getenv.
//
//   LIFETIME(kind, field, "NAME", default, "what it selects")
//
// kind      on:  set (to anything, "0" and "" included) => field true          off: set => field false (the field names the default form)
//           one: a value that begins with '1' => field true                    num: atoi of the value, `default` when unset
// LIFETIME  PROCESS: parsed with all other process rows at the first mvd_env() of the process; setting it later does nothing
//           ENGINE:  parsed by mvd_create() into the context (mvd_env_engine()): one process can hold engines of both forms
//           CALL:    re-read at every use (mvd_env_call::field()): tests flip these inside one process -- do not cache them
//           PROCESS_CALL: a PROCESS row that the stand-alone op hooks of c_api.hip re-read per call
// A field is named for what it turns on; `default` is the field's value with the variable unset; the description says what
// SETTING the variable selects.
#pragma once

#define MVD_ENV_TABLE(PROCESS, ENGINE, CALL, PROCESS_CALL) \
  /* ---- convolution / GEMM routing and plans (engine_unet.hip: igemm_go) ---- */ \
  ENGINE(off, halo, "MVD_NO_HALO", true, "3x3 convs on the gather kernel instead of the LDS-halo / conv3x kernels") \
  PROCESS_CALL(off, conv3x, "MVD_NO_CONV3X", true, "no conv3x fragment streams: 3x3 ResBlock convs on the LDS-halo kernel") \
  PROCESS(off, up_conv3x, "MVD_NO_UP_CONV3X", true, "the 4x4 -> 8x8 upsample conv as the 9-tap GEMM on the fp32 source, not upsample + conv3x") \
  PROCESS(off, gemm_dma, "MVD_NO_GEMM_DMA", true, "GEMMs / 1x1 convs on the older register-staged igemm kernel, not the LDS-DMA kernel") \
  PROCESS(num, dense_min_m, "MVD_DENSE_MIN_M", 64, "fewest rows routed to the LDS-DMA kernel (2 views per rank: 7.08 ms at 512, 6.97 ms at 64)") \
  PROCESS(off, plain, "MVD_NO_PLAIN", true, "general row mapping for plain GEMMs instead of the PLAIN instantiations") \
  PROCESS(on, old_plan, "MVD_OLD_PLAN", false, "k-step cost model (gemm_dma_plan) instead of gemm_dma_plan_us for plain GEMMs") \
  PROCESS(on, igemm_f32_bn128, "MVD_IGEMM_F32_BN128", false, "fp32 sources on 128-column tiles where 160 is picked (32768 x 960 x 320: 48 vs 37 us)") \
  PROCESS(on, bm128, "MVD_BM128", false, "offer the planner the four-wave 128-row tiles: measured, lost (profiles/r06_b_bm_sweep.txt)") \
  PROCESS(on, bm128_off, "MVD_NO_BM128", false, "overrides MVD_BM128: the 128-row tiles stay off") \
  PROCESS(num, dense_bn, "MVD_DENSE_BN", 0, "sweep (tools/gemm_plan_sweep.py): column-tile width of the dense launches, 0 = planner's") \
  PROCESS(num, dense_sk, "MVD_DENSE_SK", 0, "sweep: split-K of the dense launches, 0 = planner's") \
  PROCESS(num, dense_bm, "MVD_DENSE_BM", 0, "sweep: 128 = four-wave row tiles with MVD_DENSE_BN, else 256") \
  PROCESS(num, halo_bn, "MVD_HALO_BN", 0, "sweep (tools/conv_bench3.py): column width of the LDS-halo kernel, 0 = planner's") \
  PROCESS(num, halo_sk, "MVD_HALO_SK", 0, "sweep: split over 64-channel chunks of the LDS-halo kernel, 0 = planner's") \
  PROCESS(off, parity_batch, "MVD_NO_PARITY_BATCH", true, "one launch per output-parity class of the transposed / upsample convs, not one for all") \
  PROCESS(num, par_walk_min, "MVD_PAR_WALK_MIN", 0, "tiles from which a workgroup walks the parity classes, 0 = never (profiles/r06_y_ab_pwalk.txt: nothing)") \
  PROCESS(off, xcd_cols, "MVD_NO_XCD_COLS", true, "row-tile-major XCD walk always, never the column-major one (common.h: xcd_prefers_cols)") \
  PROCESS(off, attn_xcd, "MVD_ATTN_NO_XCD", true, "attention with the pre-remap workgroup order") \
  /* ---- split-K slabs left to the consumer ---- */ \
  PROCESS(num, defer_max, "MVD_DEFER_MAX", 16, "largest split a consumer takes as slabs (4 = the round-3 limit)") \
  PROCESS(off, defer_reduce, "MVD_NO_DEFER_REDUCE", true, "ResBlock conv1 with its own reduce pass; also turns off ln_defer and cond_defer") \
  PROCESS(off, cond_defer, "MVD_NO_COND_DEFER", true, "the DepthTransformer's GEMMs in front of a GroupNorm with their reduce passes") \
  PROCESS(on, ln_defer, "MVD_LN_DEFER", false, "LayerNorm sums the split-K slabs of proj_in / to_out (profiles/r06_g_ab_ln_defer.txt: no time gained)") \
  PROCESS(off, carry, "MVD_NO_CARRY", true, "a block's last GEMM reduces its own slabs instead of leaving them to the next block's GroupNorm") \
  /* ---- UNet blocks (engine_unet.hip) ---- */ \
  PROCESS(on, gn_two_pass, "MVD_GN_TWO_PASS", false, "two-pass GroupNorm everywhere; also turns off defer_reduce, cond_defer and out_conv_f32") \
  PROCESS(on, skip_side, "MVD_SKIP_SIDE", false, "the ResBlock's 1x1 skip conv on a helper stream (profiles/r06_z_ab_skip_side.txt: nothing)") \
  PROCESS(off, rowchain, "MVD_NO_ROWCHAIN", true, "the transformer block behind the attention as layered GEMMs, not the row-chain kernel") \
  PROCESS(num, rowchain_min_rows, "MVD_ROWCHAIN_MIN_ROWS", 16384, "fewest rows that take the row-chain kernel") \
  PROCESS(off, rowhead, "MVD_NO_ROWHEAD", true, "proj_in, LayerNorm1 and q | k | v as separate launches, not the row-head kernel") \
  PROCESS(off, xp_fuse, "MVD_NO_XP_FUSE", true, "extended-precision proj_in / proj_out as separate GEMMs beside the row kernels") \
  PROCESS(off, ffp, "MVD_NO_FFP", true, "FF2 and proj_out as two GEMMs, not one over [gg | t2]") \
  PROCESS(on, ln_scalar, "MVD_LN_SCALAR", false, "element-per-thread LayerNorm (also keeps FF2 and proj_out apart)") \
  PROCESS(off, ctx_fold, "MVD_NO_CTX_FOLD", true, "GroupNorm(proj_context(volume)) materialised, not folded into two GEMM passes") \
  PROCESS(off, ctx_group, "MVD_NO_CTX_GROUP", true, "context fold block by block, not once per level") \
  PROCESS(off, cond_const, "MVD_NO_COND_CONST", true, "DepthTransformer over all samples, context-free ones included (profiles/r06_i_ab_cond_const.txt)") \
  PROCESS(off, conv_in_f32, "MVD_NO_CONV_IN_F32", true, "the input conv on the MFMA forms, not in exact fp32 on the vector ALU") \
  PROCESS(off, out_conv_f32, "MVD_NO_OUT_CONV_F32", true, "the output head on the MFMA forms, not GroupNorm + conv in exact fp32") \
  PROCESS(off, side_stream, "MVD_NO_SIDE_STREAM", true, "context volumes and folds on the caller's stream") \
  PROCESS(off, side_emb, "MVD_NO_SIDE_EMB", true, "the timestep-embedding GEMMs on the caller's stream") \
  PROCESS(on, one_way_fork, "MVD_ONE_WAY_FORK", false, "side-stream fork without the acknowledgement: the round-1 race on demand (DESIGN.md section 4, tools/det_fork.sh)") \
  /* ---- conditioner and training ---- */ \
  PROCESS(off, fused_enc, "MVD_NO_FUSED_ENC", true, "the 2-D target encoder layer by layer, not as one launch") \
  CALL(one, bn_loop, "MVD_BN_LOOP", false, "the looped BatchNorm + ReLU kernel; tests/test_gpu_train.py flips it for its bit-identity check") \
  CALL(one, sparse_valu, "MVD_SPARSE_VALU", false, "read when sparse-conv weights are built: one-site-per-workgroup kernels and the scatter-form data gradient") \
  CALL(num, xp, "MVD_XP", precision_level, "overrides the engine's extended-precision level when the policy is applied") \
  PROCESS(on, stage_scalar, "MVD_STAGE_SCALAR", false, "element-per-thread staging kernels of the backward pass (profiles/r04_m_*)") \
  PROCESS(on, gn_bwd_one_block, "MVD_GN_BWD_ONE_BLOCK", false, "mvd_op_group_norm_bwd: one workgroup per (sample, group), not the slabbed form") \
  PROCESS(one, repack_one_stream, "MVD_REPACK_STREAMS", false, "=1: the training re-pack on one stream, not four") \
  /* ---- host-side timing and debugging (stderr) ---- */ \
  PROCESS(on, plan_debug, "MVD_PLAN_DEBUG", false, "print every dense plan as a [plan] line") \
  PROCESS(on, layer_timing, "MVD_LAYER_TIMING", false, "per-GEMM event time (tools/layer_step.py); synchronises every launch") \
  PROCESS(on, debug_sum, "MVD_DEBUG_SUM", false, "bit checksums of the step's buffers: which differ between repeats?") \
  PROCESS(on, mesh_timing, "MVD_MESH_TIMING", false, "host phases of set_mesh / set_samples") \
  PROCESS(on, cond_bwd_timing, "MVD_COND_BWD_TIMING", false, "host-side enqueue time of each conditioner-backward phase")

#include <stdlib.h>

// the value readers: the library's only getenv calls; `unset` is what an unset variable gives
inline bool mvd_env_on(const char* name, bool) { return getenv(name) != nullptr; }
inline bool mvd_env_off(const char* name, bool) { return getenv(name) == nullptr; }
inline bool mvd_env_one(const char* name, bool) { const char* v = getenv(name); return v && v[0] == '1'; }
inline int mvd_env_num(const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; }

#define MVD_ENV_SKIP(...)
#define MVD_ENV_FIELD(kind, field, name, def, doc) decltype(mvd_env_##kind(name, 0)) field = def;
#define MVD_ENV_PARSE(kind, field, name, def, doc) e.field = mvd_env_##kind(name, def);

struct MvdEnv {  // the PROCESS rows
  MVD_ENV_TABLE(MVD_ENV_FIELD, MVD_ENV_SKIP, MVD_ENV_SKIP, MVD_ENV_FIELD)
};
inline const MvdEnv& mvd_env() {  // parsed once, at the first call
  static const MvdEnv env = [] {
    MvdEnv e;
    MVD_ENV_TABLE(MVD_ENV_PARSE, MVD_ENV_SKIP, MVD_ENV_SKIP, MVD_ENV_PARSE)
    // One switch implies others: folded in here, once, so that a use site reads one field.  (In this order: ln_defer follows
    // MVD_NO_DEFER_REDUCE alone, cond_defer follows MVD_GN_TWO_PASS as well.)
    e.ln_defer = e.ln_defer && e.defer_reduce;
    e.defer_reduce = e.defer_reduce && !e.gn_two_pass;  // the single-pass GroupNorm is what adds the slabs
    e.cond_defer = e.cond_defer && e.defer_reduce;
    e.out_conv_f32 = e.out_conv_f32 && !e.gn_two_pass;  // the fp32 head takes the single-pass GroupNorm's fp32 output
    e.bm128 = e.bm128 && !e.bm128_off;
    return e;
  }();
  return env;
}

struct MvdEnvEngine {  // the ENGINE rows
  MVD_ENV_TABLE(MVD_ENV_SKIP, MVD_ENV_FIELD, MVD_ENV_SKIP, MVD_ENV_SKIP)
};
inline MvdEnvEngine mvd_env_engine() {  // parsed at every call: mvd_create keeps the result in the context
  MvdEnvEngine e;
  MVD_ENV_TABLE(MVD_ENV_SKIP, MVD_ENV_PARSE, MVD_ENV_SKIP, MVD_ENV_SKIP)
  return e;
}

namespace mvd_env_call {  // the CALL rows, one function each: a getenv per use, on purpose.  A num row takes its unset value from the caller
#define MVD_ENV_CALL_BOOL(kind, field, name, def) inline bool field() { return mvd_env_##kind(name, def); }
#define MVD_ENV_CALL_on MVD_ENV_CALL_BOOL
#define MVD_ENV_CALL_off MVD_ENV_CALL_BOOL
#define MVD_ENV_CALL_one MVD_ENV_CALL_BOOL
#define MVD_ENV_CALL_num(kind, field, name, def) inline int field(int unset) { return mvd_env_num(name, unset); }
#define MVD_ENV_CALL_FN(kind, field, name, def, doc) MVD_ENV_CALL_##kind(kind, field, name, def)
MVD_ENV_TABLE(MVD_ENV_SKIP, MVD_ENV_SKIP, MVD_ENV_CALL_FN, MVD_ENV_CALL_FN)
}  // namespace mvd_env_call
