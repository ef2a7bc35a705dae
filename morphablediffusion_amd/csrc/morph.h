// The morphable-model launchers beyond the three of common.h: the extended forward (k_morph.hip) and the backward, data term and
// optimiser of the fitter (k_morph_bwd.hip; include/mvd.h: mvd_op_morph_*_bwd, mvd_op_morph_fit_*, mvd_morph_fit_run).  The *_check
// functions are the argument errors (0 = fine) and touch no device; the launchers enqueue on `s` and never synchronise.
#pragma once
#include "common.h"

int morph_fail(const char* who, const char* what);
bool morph_too_big(long long a, long long b, long long c);  // a b c >= 2^31

// the forward with row strides (ldb, ldp, ldt: floats between two frames' betas, poses and translations), an optional coef
// [F][NB + 9 (J-1)] = betas | pose feature written by the pose kernel, an optional translation and the blended template as output
int launch_morph_pose_ex(const float* betas, int ldb, const float* pose, int ldp, const float* j_template, const float* j_dirs,
                         const int* parents, int F, int NB, int J, float* j_rest, float* rot, float* pose_feature, float* joints, float* A,
                         float* coef, hipStream_t s);
int launch_morph_skin_ex(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                         const float* post, const float* transl, int ldt, int F, int V, int L, int J, float* verts, float* blend,
                         hipStream_t s);

// vertices of a chunk of the vertex phase (and of a block of the data term), basis columns of a slab of the basis phase: the
// partial buffers are [chunks][F][J 12 + 3] and [slabs][F][L], and both counts follow from V alone
constexpr int MORPH_BWD_CHUNK = 256, MORPH_BWD_SLAB = 256;
inline int morph_bwd_chunks(int V) { return (V + MORPH_BWD_CHUNK - 1) / MORPH_BWD_CHUNK; }
inline int morph_bwd_slabs(int V) { return (int)((3LL * V + MORPH_BWD_SLAB - 1) / MORPH_BWD_SLAB); }

int morph_skin_bwd_check(const char* who, const float* g_y, const float* weights, const float* A, const float* blend, const float* basis,
                         int F, int V, int L, int NB, int J, const float* g_b, const float* part_a, const float* part_c);
int launch_morph_skin_bwd(const float* g_y, const float* post, const float* weights, const float* A, const float* blend,
                          const float* basis, int F, int V, int L, int J, float* g_b, float* part_a, float* part_c, hipStream_t s);
// g_betas / g_pose / g_transl with their row strides; g_joints may be null
int morph_pose_bwd_check(const char* who, const float* pose, const float* j_rest, const float* A, const float* j_dirs, const int* parents,
                         const float* part_a, int nchunk, const float* part_c, int nslab, int F, int NB, int J, const float* g_betas,
                         const float* g_pose, const float* g_transl);
int launch_morph_pose_bwd(const float* pose, int ldp, const float* j_rest, const float* A, const float* j_dirs, const int* parents,
                          const float* part_a, int nchunk, const float* part_c, int nslab, const float* g_joints, int F, int NB, int J,
                          float* g_betas, int ldgb, float* g_pose, int ldgp, float* g_transl, int ldgt, hipStream_t s);
int morph_landmarks_bwd_check(const char* who, const float* g_lmk, const int* csr_ptr, const int* csr_ent, const float* lmk_bary, int F,
                              int V, int M, int n_ent, const float* g_verts);
int launch_morph_landmarks_bwd(const float* g_lmk, const float* g_in, const int* csr_ptr, const int* csr_ent, const float* lmk_bary, int F,
                               int V, int M, int n_ent, float* g_verts, hipStream_t s);
int morph_fit_data_check(const char* who, const float* verts, const float* target, int target_frames, const float* lmk,
                         const float* target_lmk, int target_lmk_frames, const int* csr_ptr, const int* csr_ent, const float* lmk_bary,
                         int F, int V, int M, int n_ent, const float* g_y, const float* e_part, const float* E);
int launch_morph_fit_data(const float* verts, const float* target, int target_frames, const float* vertex_weight, float inv_vw_sum,
                          const float* lmk, const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale,
                          const int* csr_ptr, const int* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent, float* g_y,
                          float* e_part, float* E, hipStream_t s);
// the data term against correspondences: corr_point [F][V][3] is read only where corr_face [F][V] >= 0; w_part is [chunks + 1][F]
// (the block sums of the weights, then 1 / W_f)
int morph_fit_data_corr_check(const char* who, const float* verts, const float* corr_point, const int* corr_face, const float* lmk,
                              const float* target_lmk, int target_lmk_frames, const int* csr_ptr, const int* csr_ent, const float* lmk_bary,
                              int F, int V, int M, int n_ent, const float* g_y, const float* e_part, const float* w_part, const float* E,
                              const int* n_matched);
int launch_morph_fit_data_corr(const float* verts, const float* corr_point, const int* corr_face, const float* vertex_weight, const float* lmk,
                               const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale, const int* csr_ptr,
                               const int* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent, float* g_y, float* e_part,
                               float* w_part, float* E, int* n_matched, hipStream_t s);
int morph_fit_update_check(const char* who, const float* p, const float* g, const float* m, const float* v, const float* lr,
                           const float* lam, const float* p0, int F, int P, int step, float beta1, float beta2, float eps);
int launch_morph_fit_update(float* p, const float* g, float* m, float* v, const float* lr, const float* lam, const float* p0, int F, int P,
                            int step, float beta1, float beta2, float eps, hipStream_t s);

// k_morph_2d.hip: the 2-D multi-view landmark term and the per-view contour landmarks (include/mvd.h: mvd_op_morph_project,
// mvd_op_morph_fit_data_2d, mvd_op_morph_contour_*, mvd_morph_fit_2d_run).  Points of a block of the 2-D term's reduction:
constexpr int MORPH_2D_BLOCK = 256;
inline int morph_2d_blocks(int M, int Md) { return (int)(((long long)M + Md + MORPH_2D_BLOCK - 1) / MORPH_2D_BLOCK); }
// what the 2-D term reads besides the landmarks: cameras K [cam_frames][C][9], RT [cam_frames][C][12], targets in pixels
// [target_frames][C][M][2] (and [..][Md][2] for the contour landmarks) with optional weights (null = ones)
struct Morph2dTerm {
  const float *K, *RT, *target_uv, *weight, *dyn_target_uv, *dyn_weight;
  int cam_frames, target_frames, C;
  float z_near, px_scale, lambda2;
};
int morph_project_check(const char* who, const float* points, const float* K, const float* RT, int cam_frames, int F, int C, int M,
                        float z_near, const void* out_a, const void* out_b);
int launch_morph_project(const float* points, const float* K, const float* RT, int cam_frames, int F, int C, int M, float z_near, float* uv,
                         int* valid, hipStream_t s);
int launch_morph_project_bwd(const float* points, const float* K, const float* RT, int cam_frames, const float* g_uv, int F, int C, int M,
                             float z_near, float* g_points, hipStream_t s);
// part is [3 blocks + 1][F]: the block sums of w |r|^2, of w, the block counts (int32 bits), then 1 / W_f; E_add [F] or null is
// added to E2 (the loop's 3-D term); dyn_lmk null = no contour landmarks (dyn_uv, g_dyn and the term's dyn_* then null too)
int morph_fit_data_2d_check(const char* who, const Morph2dTerm& t, int F, int M, int Md, const float* lmk, const float* dyn_lmk,
                            const float* uv, const float* dyn_uv, const float* part, const float* E2, const int* n_valid, const float* g_lmk,
                            const float* g_dyn);
int launch_morph_fit_data_2d(const Morph2dTerm& t, int F, int M, int Md, const float* lmk, const float* dyn_lmk, const float* E_add,
                             float* uv, float* dyn_uv, float* part, float* E2, int* n_valid, float* g_lmk, float* g_dyn, hipStream_t s);
int morph_contour_select_check(const char* who, const float* A, const float* RT, int cam_frames, int F, int C, int J, int neck_joint, int R,
                               const int* row);
int launch_morph_contour_select(const float* A, const float* RT, int cam_frames, int F, int C, int J, int neck_joint, int R, int* row,
                                float* yaw, hipStream_t s);
int morph_contour_landmarks_check(const char* who, const float* verts, const int* faces, const int* dyn_face, const float* dyn_bary,
                                  const int* row, int F, int C, int V, int Nf, int R, int Md, const float* out);
int launch_morph_contour_landmarks(const float* verts, const int* faces, const int* dyn_face, const float* dyn_bary, const int* row, int F,
                                   int C, int V, int Nf, int R, int Md, float* out, hipStream_t s);
// g_verts is read and written in place at the listed vertices
int morph_contour_bwd_check(const char* who, const float* g_dyn, const int* row, const int* ct_vert, const int* ct_ptr, const int* ct_ent,
                            const float* dyn_bary, int F, int C, int V, int R, int Md, int n_list, int n_ent, const float* g_verts);
int launch_morph_contour_bwd(const float* g_dyn, const int* row, const int* ct_vert, const int* ct_ptr, const int* ct_ent,
                             const float* dyn_bary, int F, int C, int V, int R, int Md, int n_list, int n_ent, float* g_verts, hipStream_t s);
