// The morphable-model backward and the fitter's kernels -- include/mvd.h: mvd_op_morph_skin_bwd, _pose_bwd, _landmarks_bwd,
// mvd_op_morph_fit_data, _fit_update, and the loop mvd_morph_fit_run enqueues.  The vector-Jacobian product of k_morph.hip's forward,
// fp32 on the vector ALU, every sum in an order fixed by indices alone, no atomics: two calls agree bit for bit, and frame f of a
// batch equals the same frame computed alone.
// Launches:
//   morph_skin_bwd_vert_kernel   a workgroup of 4 waves owns a chunk of 256 vertices of one frame, a thread per vertex.  g_o = P^T g_y,
//                           T = sum_j w_j A_j as the forward chains it, g_b = T^T g_o; then, per joint and entry, w_vj g_T is summed
//                           over the chunk in a fixed shape: a butterfly over the 64 lanes of a wave (xor 32, 16, ... 1: every lane
//                           ends with the same bits), the 4 wave sums through LDS as ((s0 + s1) + s2) + s3.  One partial row
//                           [J 12 + 3] per (chunk, frame), the last three being the chunk's sum of g_o (the translation's adjoint).
//   morph_skin_bwd_basis_kernel  the bandwidth-bound stage, the forward's skin kernel turned round.  A workgroup owns a slab of 256
//                           basis columns, 64 basis rows and a tile of 32 frames, 8 per wave.  The slab of g_b of the 32 frames sits
//                           in LDS as [column][frame] for the whole workgroup's life; the basis streams through two LDS tiles of
//                           64 rows x 32 columns (8 loads per thread in flight under the previous tile's arithmetic).  Lane r of every
//                           wave owns row r: it reads its row's element of column c out of the tile (row stride 33: no bank
//                           conflict) and the 8 frames' g_b as two broadcast 16-byte reads, one chain of fused multiply-adds per frame
//                           over the slab's columns in ascending order.  The basis is read once per 32 frames and the chain of a frame
//                           is the same whatever the tiling.  Partials [slab][F][L]; ceil(3V / 256) slabs x ceil(L / 64) row groups:
//                           413 workgroups at FLAME's 5023 vertices and L = 436.
//   morph_pose_bwd_kernel   one workgroup of 4 waves per frame, the stages of morph_pose_kernel backwards: a thread per column sums the
//                           chunk and slab partials in ascending order; a thread per joint recomputes D_j = R_j - I; one thread
//                           walks the tree backwards (joints descending) out of LDS; a thread per joint goes back through Rodrigues
//                           as the forward writes it (q = r + 1e-8, angle = |q|, k = r / angle: finite at a zero pose, where it
//                           gives the rotation generators); a thread per beta adds j_dirs . g_j_rest to the summed g_coef.
//   morph_landmarks_bwd_kernel   a thread per (frame, vertex) gathers its (landmark, corner) entries of the CSR table in ascending order.
//   morph_fit_data_kernel   a thread per (vertex, frame): the residual, its weighted square and g_y with the landmark adjoint gathered
//                           through the same table; the squares are summed per block of 256 vertices in the vertex phase's shape.
//   morph_fit_energy_kernel one wave per frame: block partials and landmark squares, a lane-strided ascending sum and a butterfly.
//   morph_fit_corr_*_kernel the same data term against correspondences (a target point per frame and vertex, or none): block sums of
//                           the weighted squares and of the weights, one wave per frame for W_f, E_f and the matched count, then g_y.
//   morph_fit_update_kernel a thread per (frame, parameter): Adam as torch.optim.Adam steps it; lr == 0 leaves p, m and v alone.
#include "morph.h"

namespace {

constexpr int BWD_T = 256;
constexpr int BB_ROWS = 64, BB_TC = 32, BB_TLD = BB_TC + 1;   // rows and columns of a basis tile, its row stride in LDS
constexpr int BB_FW = 8, BB_FT = BB_FW * (BWD_T / 64);        // frames of a wave, of a workgroup
constexpr int BB_GLD = BB_FT + 4;                             // frame stride of the g_b slab [column][frame]: rows stay 16-byte aligned
constexpr int BB_NLD = BB_ROWS * BB_TC / BWD_T;               // basis tile elements per thread
static_assert(MORPH_BWD_CHUNK == BWD_T && MORPH_BWD_SLAB == BWD_T && MORPH_BWD_SLAB % BB_TC == 0 && BB_ROWS == 64 && BB_FW == 8,
              "backward geometry");

// the sum over a wave's 64 lanes, the same bits in every lane
__device__ inline float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__global__ __launch_bounds__(BWD_T) void morph_skin_bwd_vert_kernel(const float* __restrict__ g_y, const float* __restrict__ post,
                                                                    const float* __restrict__ weights, const float* __restrict__ A,
                                                                    const float* __restrict__ blend, int F, int V, int J,
                                                                    float* __restrict__ g_b, float* __restrict__ part_a) {
  __shared__ float s_A[MORPH_MAX_JOINTS * 12];
  __shared__ float s_red[BWD_T / 64][MORPH_MAX_JOINTS * 12 + 3];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int chunk = blockIdx.x, f = blockIdx.y;
  const int v = chunk * MORPH_BWD_CHUNK + t;
  const bool live = v < V;
  const int NPC = J * 12 + 3;
  for (int i = t; i < J * 12; i += BWD_T) s_A[i] = A[(size_t)f * J * 12 + i];
  __syncthreads();

  float go[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};  // a thread past V adds zeros to every sum
  if (live) {
    const size_t o = ((size_t)f * V + v) * 3;
    const float y0 = g_y[o], y1 = g_y[o + 1], y2 = g_y[o + 2];
    if (post) {
#pragma unroll
      for (int k = 0; k < 3; ++k) go[k] = fmaf(post[8 + k], y2, fmaf(post[4 + k], y1, post[k] * y0));
    } else {
      go[0] = y0, go[1] = y1, go[2] = y2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = blend[o + k];
  }
  const float* wr = weights + (size_t)(live ? v : 0) * J;
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = 0.0f;
  for (int j = 0; j < J; ++j) {
    const float wj = wr[j];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = fmaf(wj, s_A[j * 12 + e], T[e]);
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; ++k) g_b[((size_t)f * V + v) * 3 + k] = fmaf(T[8 + k], go[2], fmaf(T[4 + k], go[1], T[k] * go[0]));
  }
  float gT[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) gT[i * 4 + k] = go[i] * b[k];
    gT[i * 4 + 3] = go[i];
  }
  for (int j = 0; j < J; ++j) {
    const float wj = live ? wr[j] : 0.0f;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const float x = wave_sum(wj * gT[e]);
      if (lane == 0) s_red[w][j * 12 + e] = x;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float x = wave_sum(go[i]);
    if (lane == 0) s_red[w][J * 12 + i] = x;
  }
  __syncthreads();
  float* dst = part_a + ((size_t)chunk * F + f) * NPC;
  for (int i = t; i < NPC; i += BWD_T) dst[i] = ((s_red[0][i] + s_red[1][i]) + s_red[2][i]) + s_red[3][i];
}

__global__ __launch_bounds__(BWD_T) void morph_skin_bwd_basis_kernel(const float* __restrict__ basis, const float* __restrict__ g_b, int F,
                                                                     int V, int L, float* __restrict__ part_c) {
  __shared__ __align__(16) float s_gb[MORPH_BWD_SLAB * BB_GLD];
  __shared__ float s_tile[2][BB_ROWS * BB_TLD];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int slab = blockIdx.x, l0 = blockIdx.y * BB_ROWS, f0 = blockIdx.z * BB_FT;
  const int C = 3 * V, c0 = slab * MORPH_BWD_SLAB;
  const int ncol = min(MORPH_BWD_SLAB, C - c0);  // >= 1
  const int ntile = (ncol + BB_TC - 1) / BB_TC;

  // the slab of g_b: thread t is column t, a wave reads 256 consecutive bytes of a frame; 0 past F or the last column
  for (int fr = 0; fr < BB_FT; ++fr)
    s_gb[t * BB_GLD + fr] = (f0 + fr < F && t < ncol) ? g_b[(size_t)(f0 + fr) * C + c0 + t] : 0.0f;

  float stage[BB_NLD];
  // tile element e = t + 256 i is (row e / 32, column e % 32): a wave reads two 128-byte row segments; 0 past L or the last column
  auto load_tile = [&](int tc) {
#pragma unroll
    for (int i = 0; i < BB_NLD; ++i) {
      const int e = t + i * BWD_T, row = e / BB_TC, col = tc * BB_TC + (e % BB_TC);
      stage[i] = (l0 + row < L && col < ncol) ? basis[(size_t)(l0 + row) * C + c0 + col] : 0.0f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < BB_NLD; ++i) {
      const int e = t + i * BWD_T;
      s_tile[buf][(e / BB_TC) * BB_TLD + (e % BB_TC)] = stage[i];
    }
  };

  float acc[BB_FW];
#pragma unroll
  for (int i = 0; i < BB_FW; ++i) acc[i] = 0.0f;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int tc = 0; tc < ntile; ++tc) {
    const int buf = tc & 1;
    if (tc + 1 < ntile) load_tile(tc + 1);  // in flight under this tile's arithmetic
    const float* trow = s_tile[buf] + lane * BB_TLD;
    const float* grow = s_gb + (size_t)tc * BB_TC * BB_GLD + w * BB_FW;
#pragma unroll 4
    for (int c = 0; c < BB_TC; ++c) {
      const float bv = trow[c];
      const float4 ga = *reinterpret_cast<const float4*>(grow + c * BB_GLD), gb = *reinterpret_cast<const float4*>(grow + c * BB_GLD + 4);
      acc[0] = fmaf(ga.x, bv, acc[0]), acc[1] = fmaf(ga.y, bv, acc[1]), acc[2] = fmaf(ga.z, bv, acc[2]), acc[3] = fmaf(ga.w, bv, acc[3]);
      acc[4] = fmaf(gb.x, bv, acc[4]), acc[5] = fmaf(gb.y, bv, acc[5]), acc[6] = fmaf(gb.z, bv, acc[6]), acc[7] = fmaf(gb.w, bv, acc[7]);
    }
    if (tc + 1 < ntile) store_tile(buf ^ 1);  // the tile read at step tc - 1: every wave is past it
    __syncthreads();
  }
  if (l0 + lane >= L) return;
#pragma unroll
  for (int i = 0; i < BB_FW; ++i) {
    const int f = f0 + w * BB_FW + i;
    if (f < F) part_c[((size_t)slab * F + f) * L + l0 + lane] = acc[i];
  }
}

struct MorphPoseBwdArgs {
  const float *pose, *j_rest, *A, *j_dirs, *part_a, *part_c, *g_joints;
  float *g_betas, *g_pose, *g_transl;
  int F, NB, J, nchunk, nslab, ldp, ldgb, ldgp, ldgt;
  signed char parents[MORPH_MAX_JOINTS];
};

__global__ __launch_bounds__(BWD_T) void morph_pose_bwd_kernel(MorphPoseBwdArgs a) {
  __shared__ float s_gA[MORPH_MAX_JOINTS * 12 + 3], s_gD[MORPH_MAX_JOINTS * 9], s_D[MORPH_MAX_JOINTS * 9], s_G[MORPH_MAX_JOINTS * 12];
  __shared__ float s_jr[MORPH_MAX_JOINTS * 3], s_gjr[MORPH_MAX_JOINTS * 3], s_gt[MORPH_MAX_JOINTS * 3];
  const int f = blockIdx.x, lane = threadIdx.x;  // "lane": the thread of the workgroup's 256
  const int J = a.J, NB = a.NB, F = a.F;
  const int NPC = J * 12 + 3, L = NB + 9 * (J - 1);
  // chunk partials of g_A and g_transl, slab partials of the pose feature's adjoint: ascending.  Unrolled: the loads of 8 partials
  // are in flight under one chain of additions (one dependent load per step held this kernel to 117 us at FLAME size, F = 16)
  for (int c = lane; c < NPC; c += BWD_T) {
    float s = a.part_a[(size_t)f * NPC + c];
#pragma unroll 8
    for (int ch = 1; ch < a.nchunk; ++ch) s += a.part_a[((size_t)ch * F + f) * NPC + c];
    s_gA[c] = s;
  }
  for (int l = NB + lane; l < L; l += BWD_T) {
    float s = a.part_c[(size_t)f * L + l];
#pragma unroll 8
    for (int sl = 1; sl < a.nslab; ++sl) s += a.part_c[((size_t)sl * F + f) * L + l];
    s_gD[9 + l - NB] = s;
  }
  if (lane < 9) s_gD[lane] = 0.0f;
  for (int c = lane; c < J * 12; c += BWD_T) s_G[c] = a.A[(size_t)f * J * 12 + c];
  for (int c = lane; c < J * 3; c += BWD_T) {
    s_jr[c] = a.j_rest[(size_t)f * J * 3 + c];
    s_gt[c] = a.g_joints ? a.g_joints[(size_t)f * J * 3 + c] : 0.0f;
    s_gjr[c] = 0.0f;
  }
  // Rodrigues as the forward writes it; the same values serve the way back below
  float rx = 0.0f, ry = 0.0f, rz = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f, angle = 1.0f, x = 0.0f, y = 0.0f, z = 0.0f, sn = 0.0f, cs = 1.0f,
        oc = 0.0f;
  if (lane < J) {
    const float* pr = a.pose + (size_t)f * a.ldp + lane * 3;
    rx = pr[0], ry = pr[1], rz = pr[2];
    qx = rx + 1e-8f, qy = ry + 1e-8f, qz = rz + 1e-8f;
    angle = sqrtf(fmaf(qz, qz, fmaf(qy, qy, qx * qx)));
    x = rx / angle, y = ry / angle, z = rz / angle;
    sn = sinf(angle), cs = cosf(angle), oc = 1.0f - cs;
    float* D = s_D + lane * 9;
    D[0] = 0.0f - oc * fmaf(y, y, z * z);
    D[1] = fmaf(oc, x * y, 0.0f - sn * z);
    D[2] = fmaf(oc, x * z, sn * y);
    D[3] = fmaf(oc, x * y, sn * z);
    D[4] = 0.0f - oc * fmaf(x, x, z * z);
    D[5] = fmaf(oc, y * z, 0.0f - sn * x);
    D[6] = fmaf(oc, x * z, 0.0f - sn * y);
    D[7] = fmaf(oc, y * z, sn * x);
    D[8] = 0.0f - oc * fmaf(x, x, y * y);
  }
  __syncthreads();

  // the chain backwards, joints descending: with p = parents[j], G_j = G_p R_j, a_j = a_p - G_p u_j (u_j = D_j j_rest_j),
  // t_j = G_p (j_rest_j - j_rest_p) + t_p; every child of j has a larger index, so g_G_j, g_a_j and g_t_j are complete at step j
  if (lane == 0) {
    for (int j = J - 1; j >= 0; --j) {
      float D[9], R[9], jr[3], u[3], gG[9], ga[3], gt[3], gR[9], gu[3];
#pragma unroll
      for (int e = 0; e < 9; ++e) D[e] = s_D[j * 9 + e], R[e] = (e % 4 == 0 ? 1.0f : 0.0f) + D[e];
#pragma unroll
      for (int k = 0; k < 3; ++k) jr[k] = s_jr[j * 3 + k], gt[k] = s_gt[j * 3 + k];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        u[i] = fmaf(D[i * 3 + 2], jr[2], fmaf(D[i * 3 + 1], jr[1], D[i * 3] * jr[0]));
        ga[i] = s_gA[j * 12 + i * 4 + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) gG[i * 3 + k] = s_gA[j * 12 + i * 4 + k];
      }
      if (j == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) gR[e] = gG[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) gu[k] = 0.0f - ga[k], s_gjr[k] += gt[k];
      } else {
        const int p = a.parents[j];
        float Gp[9], rel[3], grel[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int k = 0; k < 3; ++k) Gp[i * 3 + k] = s_G[p * 12 + i * 4 + k];
          rel[i] = jr[i] - s_jr[p * 3 + i];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
          for (int l = 0; l < 3; ++l) gR[k * 3 + l] = fmaf(Gp[6 + k], gG[6 + l], fmaf(Gp[3 + k], gG[3 + l], Gp[k] * gG[l]));
          gu[k] = 0.0f - fmaf(Gp[6 + k], ga[2], fmaf(Gp[3 + k], ga[1], Gp[k] * ga[0]));
          grel[k] = fmaf(Gp[6 + k], gt[2], fmaf(Gp[3 + k], gt[1], Gp[k] * gt[0]));
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            // g_G_p += g_G_j R_j^T - g_a_j u_j^T + g_t_j rel^T
            float d = fmaf(gG[i * 3 + 2], R[k * 3 + 2], fmaf(gG[i * 3 + 1], R[k * 3 + 1], gG[i * 3] * R[k * 3]));
            d = fmaf(gt[i], rel[k], fmaf(0.0f - ga[i], u[k], d));
            s_gA[p * 12 + i * 4 + k] += d;
          }
          s_gA[p * 12 + i * 4 + 3] += ga[i];
          s_gt[p * 3 + i] += gt[i];
          s_gjr[j * 3 + i] += grel[i];
          s_gjr[p * 3 + i] -= grel[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_gD[j * 9 + i * 3 + k] += fmaf(gu[i], jr[k], gR[i * 3 + k]);
        s_gjr[j * 3 + i] += fmaf(D[6 + i], gu[2], fmaf(D[3 + i], gu[1], D[i] * gu[0]));
      }
    }
  }
  __syncthreads();

  if (lane < J) {
    const float* g = s_gD + lane * 9;
    const float g13 = g[1] + g[3], g26 = g[2] + g[6], g57 = g[5] + g[7];
    const float g_sn = fmaf(x, g[7] - g[5], fmaf(y, g[2] - g[6], z * (g[3] - g[1])));
    float g_oc = 0.0f - fmaf(fmaf(x, x, y * y), g[8], fmaf(fmaf(x, x, z * z), g[4], fmaf(y, y, z * z) * g[0]));
    g_oc = fmaf(y * z, g57, fmaf(x * z, g26, fmaf(x * y, g13, g_oc)));
    const float gx = fmaf(sn, g[7] - g[5], oc * fmaf(-2.0f * x, g[4] + g[8], fmaf(z, g26, y * g13)));
    const float gy = fmaf(sn, g[2] - g[6], oc * fmaf(-2.0f * y, g[0] + g[8], fmaf(z, g57, x * g13)));
    const float gz = fmaf(sn, g[3] - g[1], oc * fmaf(-2.0f * z, g[0] + g[4], fmaf(y, g57, x * g26)));
    // k = r / angle: g_r = g_k / angle, g_angle -= (g_k . k) / angle; angle = |q|: g_q = g_angle q / angle; q = r + 1e-8
    const float g_angle = fmaf(g_sn, cs, g_oc * sn) - fmaf(gz, z, fmaf(gy, y, gx * x)) / angle;
    float* dst = a.g_pose + (size_t)f * a.ldgp + lane * 3;
    dst[0] = fmaf(g_angle, qx / angle, gx / angle);
    dst[1] = fmaf(g_angle, qy / angle, gy / angle);
    dst[2] = fmaf(g_angle, qz / angle, gz / angle);
  }
  for (int n = lane; n < NB; n += BWD_T) {
    float s = a.part_c[(size_t)f * L + n];
#pragma unroll 8
    for (int sl = 1; sl < a.nslab; ++sl) s += a.part_c[((size_t)sl * F + f) * L + n];
    const float* jd = a.j_dirs + (size_t)n * J * 3;
    float d = 0.0f;  // the joints' share on its own, then one addition: it is small beside g_coef, which would round it 3 J times
    for (int c = 0; c < J * 3; ++c) d = fmaf(jd[c], s_gjr[c], d);
    a.g_betas[(size_t)f * a.ldgb + n] = s + d;
  }
  if (lane < 3) a.g_transl[(size_t)f * a.ldgt + lane] = s_gA[J * 12 + lane];
}

// the entries csr_ent[begin .. end) of vertex v, clamped to the table: a bad table reads nothing out of range
__device__ inline void csr_range(const int* __restrict__ csr_ptr, int v, int n_ent, int* begin, int* end) {
  *begin = min(max(csr_ptr[v], 0), n_ent);
  *end = min(max(csr_ptr[v + 1], *begin), n_ent);
}

__global__ __launch_bounds__(BWD_T) void morph_landmarks_bwd_kernel(const float* __restrict__ g_lmk, const float* __restrict__ g_in,
                                                                    const int* __restrict__ csr_ptr, const int* __restrict__ csr_ent,
                                                                    const float* __restrict__ lmk_bary, int F, int V, int M, int n_ent,
                                                                    float* __restrict__ g_verts) {
  const int i = blockIdx.x * BWD_T + threadIdx.x;  // F V 3 < 2^31
  if (i >= F * V) return;
  const int f = i / V, v = i - f * V;
  float acc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = g_in ? g_in[(size_t)i * 3 + k] : 0.0f;
  int q0, q1;
  csr_range(csr_ptr, v, n_ent, &q0, &q1);
  for (int q = q0; q < q1; ++q) {
    const int ent = csr_ent[q];  // landmark * 3 + corner
    if ((unsigned)ent >= (unsigned)(3 * M)) continue;
    const float wt = lmk_bary[ent];
    const float* g = g_lmk + ((size_t)f * M + ent / 3) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = fmaf(wt, g[k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) g_verts[(size_t)i * 3 + k] = acc[k];
}

__global__ __launch_bounds__(BWD_T) void morph_fit_data_kernel(const float* __restrict__ verts, const float* __restrict__ target,
                                                               int target_frames, const float* __restrict__ vertex_weight,
                                                               float inv_vw_sum, const float* __restrict__ lmk,
                                                               const float* __restrict__ target_lmk, int target_lmk_frames,
                                                               const float* __restrict__ lmk_weight, float lmk_scale,
                                                               const int* __restrict__ csr_ptr, const int* __restrict__ csr_ent,
                                                               const float* __restrict__ lmk_bary, int F, int V, int M, int n_ent,
                                                               float* __restrict__ g_y, float* __restrict__ e_part) {
  __shared__ float s_red[BWD_T / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int blk = blockIdx.x, f = blockIdx.y;
  const int v = blk * MORPH_BWD_CHUNK + t;
  float e = 0.0f;
  if (v < V) {
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (target) {
      const float* yp = verts + ((size_t)f * V + v) * 3;
      const float* tp = target + ((size_t)(target_frames == 1 ? 0 : f) * V + v) * 3;
      const float wt = vertex_weight ? vertex_weight[v] : 1.0f;
      const float r0 = yp[0] - tp[0], r1 = yp[1] - tp[1], r2 = yp[2] - tp[2];
      e = wt * fmaf(r2, r2, fmaf(r1, r1, r0 * r0));
      const float sc = 2.0f * wt * inv_vw_sum;
      g[0] = sc * r0, g[1] = sc * r1, g[2] = sc * r2;
    }
    if (target_lmk) {
      int q0, q1;
      csr_range(csr_ptr, v, n_ent, &q0, &q1);
      for (int q = q0; q < q1; ++q) {
        const int ent = csr_ent[q];
        if ((unsigned)ent >= (unsigned)(3 * M)) continue;
        const int m = ent / 3;
        const float sc = lmk_bary[ent] * (2.0f * lmk_scale * (lmk_weight ? lmk_weight[m] : 1.0f));
        const float* lp = lmk + ((size_t)f * M + m) * 3;
        const float* tp = target_lmk + ((size_t)(target_lmk_frames == 1 ? 0 : f) * M + m) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = fmaf(sc, lp[k] - tp[k], g[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g_y[((size_t)f * V + v) * 3 + k] = g[k];
  }
  e = wave_sum(e);
  if (lane == 0) s_red[w] = e;
  __syncthreads();
  if (t == 0) e_part[(size_t)blk * F + f] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(64) void morph_fit_energy_kernel(const float* __restrict__ e_part, int nblk, float inv_vw_sum,
                                                              const float* __restrict__ lmk, const float* __restrict__ target_lmk,
                                                              int target_lmk_frames, const float* __restrict__ lmk_weight,
                                                              float lmk_scale, int F, int M, float* __restrict__ E) {
  const int f = blockIdx.x, lane = threadIdx.x;
  float ev = 0.0f, el = 0.0f;
  for (int b = lane; b < nblk; b += 64) ev += e_part[(size_t)b * F + f];
  if (target_lmk) {
    for (int m = lane; m < M; m += 64) {
      const float* lp = lmk + ((size_t)f * M + m) * 3;
      const float* tp = target_lmk + ((size_t)(target_lmk_frames == 1 ? 0 : f) * M + m) * 3;
      const float r0 = lp[0] - tp[0], r1 = lp[1] - tp[1], r2 = lp[2] - tp[2];
      el = fmaf(lmk_weight ? lmk_weight[m] : 1.0f, fmaf(r2, r2, fmaf(r1, r1, r0 * r0)), el);
    }
  }
  ev = wave_sum(ev), el = wave_sum(el);
  if (lane == 0) E[f] = fmaf(el, lmk_scale, ev * inv_vw_sum);
}

// The data term against correspondences (include/mvd.h: mvd_op_morph_fit_data_corr): a vertex counts iff corr_face >= 0, and only
// then is its corr_point read.  Three launches, in morph_fit_data's summation shape.  Stats: per block of 256 vertices the sums of
// w m |y - c|^2 and of w m.
__global__ __launch_bounds__(BWD_T) void morph_fit_corr_stats_kernel(const float* __restrict__ verts, const float* __restrict__ corr_point,
                                                                     const int* __restrict__ corr_face,
                                                                     const float* __restrict__ vertex_weight, int F, int V,
                                                                     float* __restrict__ e_part, float* __restrict__ w_part) {
  __shared__ float s_red[2][BWD_T / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int blk = blockIdx.x, f = blockIdx.y;
  const int v = blk * MORPH_BWD_CHUNK + t;
  float e = 0.0f, ws = 0.0f;
  if (v < V && corr_face[(size_t)f * V + v] >= 0) {
    const float* yp = verts + ((size_t)f * V + v) * 3;
    const float* cp = corr_point + ((size_t)f * V + v) * 3;
    const float r0 = yp[0] - cp[0], r1 = yp[1] - cp[1], r2 = yp[2] - cp[2];
    ws = vertex_weight ? vertex_weight[v] : 1.0f;
    e = ws * fmaf(r2, r2, fmaf(r1, r1, r0 * r0));
  }
  e = wave_sum(e), ws = wave_sum(ws);
  if (lane == 0) s_red[0][w] = e, s_red[1][w] = ws;
  __syncthreads();
  if (t == 0) {
    e_part[(size_t)blk * F + f] = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
    w_part[(size_t)blk * F + f] = ((s_red[1][0] + s_red[1][1]) + s_red[1][2]) + s_red[1][3];
  }
}

// one wave per frame: W_f and the squares out of the block partials, the matched count straight from corr_face, the landmark
// squares; row nblk of w_part takes 1 / W_f (0 when W_f is not positive), which the gradient launch reads
__global__ __launch_bounds__(64) void morph_fit_corr_energy_kernel(const float* __restrict__ e_part, float* __restrict__ w_part, int nblk,
                                                                   const int* __restrict__ corr_face, const float* __restrict__ lmk,
                                                                   const float* __restrict__ target_lmk, int target_lmk_frames,
                                                                   const float* __restrict__ lmk_weight, float lmk_scale, int F, int V, int M,
                                                                   float* __restrict__ E, int* __restrict__ n_matched) {
  const int f = blockIdx.x, lane = threadIdx.x;
  float ev = 0.0f, wv = 0.0f, el = 0.0f;
  int cnt = 0;
  for (int b = lane; b < nblk; b += 64) ev += e_part[(size_t)b * F + f], wv += w_part[(size_t)b * F + f];
  for (int v = lane; v < V; v += 64) cnt += corr_face[(size_t)f * V + v] >= 0;
  if (target_lmk) {
    for (int m = lane; m < M; m += 64) {
      const float* lp = lmk + ((size_t)f * M + m) * 3;
      const float* tp = target_lmk + ((size_t)(target_lmk_frames == 1 ? 0 : f) * M + m) * 3;
      const float r0 = lp[0] - tp[0], r1 = lp[1] - tp[1], r2 = lp[2] - tp[2];
      el = fmaf(lmk_weight ? lmk_weight[m] : 1.0f, fmaf(r2, r2, fmaf(r1, r1, r0 * r0)), el);
    }
  }
  ev = wave_sum(ev), wv = wave_sum(wv), el = wave_sum(el);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane == 0) {
    const float inv = wv > 0.0f ? 1.0f / wv : 0.0f;
    w_part[(size_t)nblk * F + f] = inv;
    E[f] = fmaf(el, lmk_scale, ev * inv);
    n_matched[f] = cnt;
  }
}

__global__ __launch_bounds__(BWD_T) void morph_fit_corr_grad_kernel(const float* __restrict__ verts, const float* __restrict__ corr_point,
                                                                    const int* __restrict__ corr_face,
                                                                    const float* __restrict__ vertex_weight, const float* __restrict__ inv_w,
                                                                    const float* __restrict__ lmk, const float* __restrict__ target_lmk,
                                                                    int target_lmk_frames, const float* __restrict__ lmk_weight,
                                                                    float lmk_scale, const int* __restrict__ csr_ptr,
                                                                    const int* __restrict__ csr_ent, const float* __restrict__ lmk_bary, int F,
                                                                    int V, int M, int n_ent, float* __restrict__ g_y) {
  const int f = blockIdx.y, v = blockIdx.x * MORPH_BWD_CHUNK + threadIdx.x;
  if (v >= V) return;
  float g[3] = {0.0f, 0.0f, 0.0f};
  const float inv = inv_w[f];
  if (corr_face[(size_t)f * V + v] >= 0 && inv != 0.0f) {
    const float* yp = verts + ((size_t)f * V + v) * 3;
    const float* cp = corr_point + ((size_t)f * V + v) * 3;
    const float sc = 2.0f * (vertex_weight ? vertex_weight[v] : 1.0f) * inv;
    g[0] = sc * (yp[0] - cp[0]), g[1] = sc * (yp[1] - cp[1]), g[2] = sc * (yp[2] - cp[2]);
  }
  if (target_lmk) {
    int q0, q1;
    csr_range(csr_ptr, v, n_ent, &q0, &q1);
    for (int q = q0; q < q1; ++q) {
      const int ent = csr_ent[q];
      if ((unsigned)ent >= (unsigned)(3 * M)) continue;
      const int m = ent / 3;
      const float sc = lmk_bary[ent] * (2.0f * lmk_scale * (lmk_weight ? lmk_weight[m] : 1.0f));
      const float* lp = lmk + ((size_t)f * M + m) * 3;
      const float* tp = target_lmk + ((size_t)(target_lmk_frames == 1 ? 0 : f) * M + m) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = fmaf(sc, lp[k] - tp[k], g[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) g_y[((size_t)f * V + v) * 3 + k] = g[k];
}

// torch.optim.Adam's single-tensor step on g' = g + 2 lam (p - p0): m = lerp(m, g', 1 - beta1), v = v beta2 + (1 - beta2) g'^2,
// p -= (lr / bias1) m / (sqrt(v) / sqrt(bias2) + eps), the two bias corrections in double as torch computes them on the host
__global__ __launch_bounds__(BWD_T) void morph_fit_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, const float* __restrict__ lr,
                                                                 const float* __restrict__ lam, const float* __restrict__ p0, int n, int P,
                                                                 float beta1, float beta2, float eps, double bias1, float sqrt_bias2) {
  const int i = blockIdx.x * BWD_T + threadIdx.x;
  if (i >= n) return;
  const int c = i % P;
  const float lrc = lr[c];
  if (lrc == 0.0f) return;  // frozen: p, m and v keep their bits
  const float pi = p[i];
  const float gg = fmaf(2.0f * lam[c], pi - p0[c], g[i]);
  const float mi = fmaf(1.0f - beta1, gg - m[i], m[i]);
  const float vi = fmaf((1.0f - beta2) * gg, gg, v[i] * beta2);
  const float denom = sqrtf(vi) / sqrt_bias2 + eps;
  const float step = (float)((double)lrc / bias1);
  m[i] = mi, v[i] = vi;
  p[i] = fmaf(0.0f - step, mi / denom, pi);
}

}  // namespace

int morph_skin_bwd_check(const char* who, const float* g_y, const float* weights, const float* A, const float* blend, const float* basis,
                         int F, int V, int L, int NB, int J, const float* g_b, const float* part_a, const float* part_c) {
  if (!g_y || !weights || !A || !blend || !basis || !g_b || !part_a || !part_c) return morph_fail(who, ": null argument");
  if (F < 1 || V < 1 || L < 1 || NB < 1) return morph_fail(who, ": F, V, L and NB must be at least 1");
  if (J < 1 || J > MORPH_MAX_JOINTS) return morph_fail(who, ": J must be in 1..64");
  if ((long long)L != (long long)NB + 9LL * (J - 1)) return morph_fail(who, ": L must be NB + 9 (J - 1)");
  if (morph_too_big(F, V, 3) || morph_too_big(morph_bwd_slabs(V), F, L) || morph_too_big(morph_bwd_chunks(V), F, J * 12 + 3) || F > 65535 * 32)
    return morph_fail(who, ": F V 3 and the partial buffers must be below 2^31 elements, F at most 65535 x 32");
  return 0;
}

int launch_morph_skin_bwd(const float* g_y, const float* post, const float* weights, const float* A, const float* blend,
                          const float* basis, int F, int V, int L, int J, float* g_b, float* part_a, float* part_c, hipStream_t s) {
  // the frame axis of a grid holds 65535 blocks: the vertex phase goes over the frames in runs of that many
  for (int f0 = 0; f0 < F; f0 += 65535) {
    const int nf = min(65535, F - f0);
    hipLaunchKernelGGL(morph_skin_bwd_vert_kernel, dim3(morph_bwd_chunks(V), nf), dim3(BWD_T), 0, s, g_y + (size_t)f0 * V * 3, post, weights,
                       A + (size_t)f0 * J * 12, blend + (size_t)f0 * V * 3, F, V, J, g_b + (size_t)f0 * V * 3,
                       part_a + (size_t)f0 * (J * 12 + 3));
    HIP_CHECK_RET(hipGetLastError());
  }
  hipLaunchKernelGGL(morph_skin_bwd_basis_kernel, dim3(morph_bwd_slabs(V), (L + BB_ROWS - 1) / BB_ROWS, (F + BB_FT - 1) / BB_FT),
                     dim3(BWD_T), 0, s, basis, g_b, F, V, L, part_c);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_pose_bwd_check(const char* who, const float* pose, const float* j_rest, const float* A, const float* j_dirs, const int* parents,
                         const float* part_a, int nchunk, const float* part_c, int nslab, int F, int NB, int J, const float* g_betas,
                         const float* g_pose, const float* g_transl) {
  if (!pose || !j_rest || !A || !j_dirs || !parents || !part_a || !part_c || !g_betas || !g_pose || !g_transl)
    return morph_fail(who, ": null argument");
  if (F < 1 || NB < 1 || nchunk < 1 || nslab < 1) return morph_fail(who, ": F, NB and the partial counts must be at least 1");
  if (J < 1 || J > MORPH_MAX_JOINTS) return morph_fail(who, ": J must be in 1..64");
  if (morph_too_big(F, J, 12) || morph_too_big(NB, J, 3) || morph_too_big(nchunk, F, J * 12 + 3) ||
      morph_too_big(nslab, F, NB + 9 * (J - 1)))
    return morph_fail(who, ": F J 12, NB J 3 and the partial buffers must be below 2^31 elements");
  if (parents[0] != -1) return morph_fail(who, ": parents[0] must be -1");
  for (int j = 1; j < J; ++j)
    if (parents[j] < 0 || parents[j] >= j) return morph_fail(who, ": parents[j] must be in 0..j-1 for j >= 1");
  return 0;
}

int launch_morph_pose_bwd(const float* pose, int ldp, const float* j_rest, const float* A, const float* j_dirs, const int* parents,
                          const float* part_a, int nchunk, const float* part_c, int nslab, const float* g_joints, int F, int NB, int J,
                          float* g_betas, int ldgb, float* g_pose, int ldgp, float* g_transl, int ldgt, hipStream_t s) {
  MorphPoseBwdArgs a;
  a.pose = pose, a.j_rest = j_rest, a.A = A, a.j_dirs = j_dirs, a.part_a = part_a, a.part_c = part_c, a.g_joints = g_joints;
  a.g_betas = g_betas, a.g_pose = g_pose, a.g_transl = g_transl;
  a.F = F, a.NB = NB, a.J = J, a.nchunk = nchunk, a.nslab = nslab, a.ldp = ldp, a.ldgb = ldgb, a.ldgp = ldgp, a.ldgt = ldgt;
  for (int j = 0; j < MORPH_MAX_JOINTS; ++j) a.parents[j] = (signed char)(j < J ? parents[j] : -1);
  hipLaunchKernelGGL(morph_pose_bwd_kernel, dim3(F), dim3(BWD_T), 0, s, a);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_landmarks_bwd_check(const char* who, const float* g_lmk, const int* csr_ptr, const int* csr_ent, const float* lmk_bary, int F,
                              int V, int M, int n_ent, const float* g_verts) {
  if (!g_lmk || !csr_ptr || !csr_ent || !lmk_bary || !g_verts) return morph_fail(who, ": null argument");
  if (F < 1 || V < 1 || M < 1 || n_ent < 1) return morph_fail(who, ": F, V, M and the entry count must be at least 1");
  if (morph_too_big(F, V, 3) || morph_too_big(F, M, 3)) return morph_fail(who, ": F V 3 and F M 3 must be below 2^31");
  return 0;
}

int launch_morph_landmarks_bwd(const float* g_lmk, const float* g_in, const int* csr_ptr, const int* csr_ent, const float* lmk_bary, int F,
                               int V, int M, int n_ent, float* g_verts, hipStream_t s) {
  hipLaunchKernelGGL(morph_landmarks_bwd_kernel, dim3((F * V + BWD_T - 1) / BWD_T), dim3(BWD_T), 0, s, g_lmk, g_in, csr_ptr, csr_ent,
                     lmk_bary, F, V, M, n_ent, g_verts);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_fit_data_check(const char* who, const float* verts, const float* target, int target_frames, const float* lmk,
                         const float* target_lmk, int target_lmk_frames, const int* csr_ptr, const int* csr_ent, const float* lmk_bary,
                         int F, int V, int M, int n_ent, const float* g_y, const float* e_part, const float* E) {
  if (!verts || !g_y || !e_part || !E) return morph_fail(who, ": null argument");
  if (!target && !target_lmk) return morph_fail(who, ": neither a vertex nor a landmark target");
  if (F < 1 || V < 1) return morph_fail(who, ": F and V must be at least 1");
  if (F > 65535) return morph_fail(who, ": at most 65535 frames");
  if (target && target_frames != 1 && target_frames != F) return morph_fail(who, ": the vertex target must have 1 or F frames");
  if (target_lmk) {
    if (!lmk || !csr_ptr || !csr_ent || !lmk_bary) return morph_fail(who, ": a landmark target needs landmarks, their table and weights");
    if (M < 1 || n_ent < 1) return morph_fail(who, ": M and the entry count must be at least 1 with a landmark target");
    if (target_lmk_frames != 1 && target_lmk_frames != F) return morph_fail(who, ": the landmark target must have 1 or F frames");
    if (morph_too_big(F, M, 3)) return morph_fail(who, ": F M 3 must be below 2^31");
  }
  if (morph_too_big(F, V, 3)) return morph_fail(who, ": F V 3 must be below 2^31");
  return 0;
}

int launch_morph_fit_data(const float* verts, const float* target, int target_frames, const float* vertex_weight, float inv_vw_sum,
                          const float* lmk, const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale,
                          const int* csr_ptr, const int* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent, float* g_y,
                          float* e_part, float* E, hipStream_t s) {
  const int nblk = morph_bwd_chunks(V);
  hipLaunchKernelGGL(morph_fit_data_kernel, dim3(nblk, F), dim3(BWD_T), 0, s, verts, target, target_frames, vertex_weight, inv_vw_sum, lmk,
                     target_lmk, target_lmk_frames, lmk_weight, lmk_scale, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y, e_part);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(morph_fit_energy_kernel, dim3(F), dim3(64), 0, s, e_part, nblk, target ? inv_vw_sum : 0.0f, lmk, target_lmk,
                     target_lmk_frames, lmk_weight, lmk_scale, F, M, E);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_fit_data_corr_check(const char* who, const float* verts, const float* corr_point, const int* corr_face, const float* lmk,
                              const float* target_lmk, int target_lmk_frames, const int* csr_ptr, const int* csr_ent, const float* lmk_bary,
                              int F, int V, int M, int n_ent, const float* g_y, const float* e_part, const float* w_part, const float* E,
                              const int* n_matched) {
  if (!verts || !corr_point || !corr_face || !g_y || !e_part || !w_part || !E || !n_matched) return morph_fail(who, ": null argument");
  if (F < 1 || V < 1) return morph_fail(who, ": F and V must be at least 1");
  if (F > 65535) return morph_fail(who, ": at most 65535 frames");
  if (target_lmk) {
    if (!lmk || !csr_ptr || !csr_ent || !lmk_bary) return morph_fail(who, ": a landmark target needs landmarks, their table and weights");
    if (M < 1 || n_ent < 1) return morph_fail(who, ": M and the entry count must be at least 1 with a landmark target");
    if (target_lmk_frames != 1 && target_lmk_frames != F) return morph_fail(who, ": the landmark target must have 1 or F frames");
    if (morph_too_big(F, M, 3)) return morph_fail(who, ": F M 3 must be below 2^31");
  }
  if (morph_too_big(F, V, 3)) return morph_fail(who, ": F V 3 must be below 2^31");
  return 0;
}

int launch_morph_fit_data_corr(const float* verts, const float* corr_point, const int* corr_face, const float* vertex_weight, const float* lmk,
                               const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale, const int* csr_ptr,
                               const int* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent, float* g_y, float* e_part,
                               float* w_part, float* E, int* n_matched, hipStream_t s) {
  const int nblk = morph_bwd_chunks(V);
  hipLaunchKernelGGL(morph_fit_corr_stats_kernel, dim3(nblk, F), dim3(BWD_T), 0, s, verts, corr_point, corr_face, vertex_weight, F, V, e_part,
                     w_part);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(morph_fit_corr_energy_kernel, dim3(F), dim3(64), 0, s, e_part, w_part, nblk, corr_face, lmk, target_lmk,
                     target_lmk_frames, lmk_weight, lmk_scale, F, V, M, E, n_matched);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(morph_fit_corr_grad_kernel, dim3(nblk, F), dim3(BWD_T), 0, s, verts, corr_point, corr_face, vertex_weight,
                     w_part + (size_t)nblk * F, lmk, target_lmk, target_lmk_frames, lmk_weight, lmk_scale, csr_ptr, csr_ent, lmk_bary, F, V, M,
                     n_ent, g_y);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_fit_update_check(const char* who, const float* p, const float* g, const float* m, const float* v, const float* lr,
                           const float* lam, const float* p0, int F, int P, int step, float beta1, float beta2, float eps) {
  if (!p || !g || !m || !v || !lr || !lam || !p0) return morph_fail(who, ": null argument");
  if (F < 1 || P < 1 || step < 1) return morph_fail(who, ": F, P and step must be at least 1");
  if (morph_too_big(F, P, 1)) return morph_fail(who, ": F P must be below 2^31");
  if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps > 0.0f))
    return morph_fail(who, ": beta1 and beta2 must be in [0, 1) and eps positive");
  return 0;
}

int launch_morph_fit_update(float* p, const float* g, float* m, float* v, const float* lr, const float* lam, const float* p0, int F, int P,
                            int step, float beta1, float beta2, float eps, hipStream_t s) {
  const double bias1 = 1.0 - pow((double)beta1, (double)step), bias2 = 1.0 - pow((double)beta2, (double)step);
  const int n = F * P;
  hipLaunchKernelGGL(morph_fit_update_kernel, dim3((n + BWD_T - 1) / BWD_T), dim3(BWD_T), 0, s, p, g, m, v, lr, lam, p0, n, P, beta1, beta2,
                     eps, bias1, (float)sqrt(bias2));
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
