// UV texture atlases from generated views -- include/mvd.h: mvd_op_mesh_vertex_normals, mvd_op_mesh_texel_bake,
// mvd_op_mesh_texture_dilate, mvd_op_mesh_render_uv.  The texel -> face map comes from mvd_op_mesh_raster run on the chart
// coordinates (k_mesh.hip); the projection chain, the visibility integers, the weight and the bilinear sample are csrc/mesh.h,
// the same code the per-vertex fusion runs.
// Launches:
//   mesh_vertex_normals_kernel  one thread per (frame, vertex): walks the vertex's row of the CSR incidence table in order, sums
//                        the face cross products in fp32, normalises.  No atomics but the integer count of bad table entries.
//   mesh_texel_bake_kernel  grid (ceil(Wt / 16), ceil(Ht / 16)), 256 threads = one 16 x 16 tile of texels, so that neighbouring
//                        threads gather neighbouring view pixels.  A texel without a face writes its fill values and returns,
//                        so a tile without a covered texel ends before the view loop.  The camera rows (RT, K, centres) are
//                        __restrict__ kernel parameters indexed by the view alone: scalar loads in both passes (s_load_dwordx8 +
//                        x4 for a row of RT, checked in the code object).  Views in index order; the visibility of views 0..63 is kept in a bit mask,
//                        so that the second pass (the spread) samples only the views the first one saw.
//   mesh_texture_dilate_kernel  one thread per texel, one launch per round, ping-pong between two buffers.
//   mesh_render_uv_kernel  grid (ceil(H W / 256), N), one thread per pixel: int64 edge functions times keys, one fp64 division per
//                        corner, the UV sum and the bilinear fetch in fp32.
#include "mesh.h"

namespace {

constexpr int UV_T = 256, UV_TILE = 16;

int uv_fail(const char* who, const char* what) { return mvd_fail((std::string(who) + what).c_str()); }

__global__ __launch_bounds__(UV_T) void mesh_vertex_normals_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                   const int* __restrict__ inc_ptr, const int* __restrict__ inc_face,
                                                                   int Nv, int Nf, float* __restrict__ normals, int* __restrict__ bad_faces) {
  const int v = blockIdx.x * UV_T + threadIdx.x, fr = blockIdx.y;
  if (v >= Nv) return;
  const float* x = verts + (size_t)fr * Nv * 3;
  int lo = inc_ptr[v], hi = inc_ptr[v + 1], bad = 0;
  if (lo < 0 || hi < lo || (long long)hi > 3LL * Nf) {  // a broken row is not walked
    bad = 1;
    hi = lo = 0;
  }
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int e = lo; e < hi; ++e) {
    const int f = inc_face[e];
    if ((unsigned)f >= (unsigned)Nf) {
      ++bad;
      continue;
    }
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)Nv || (unsigned)i1 >= (unsigned)Nv || (unsigned)i2 >= (unsigned)Nv) {
      ++bad;
      continue;
    }
    const float ax = x[(size_t)i1 * 3] - x[(size_t)i0 * 3], ay = x[(size_t)i1 * 3 + 1] - x[(size_t)i0 * 3 + 1],
                az = x[(size_t)i1 * 3 + 2] - x[(size_t)i0 * 3 + 2];
    const float bx = x[(size_t)i2 * 3] - x[(size_t)i0 * 3], by = x[(size_t)i2 * 3 + 1] - x[(size_t)i0 * 3 + 1],
                bz = x[(size_t)i2 * 3 + 2] - x[(size_t)i0 * 3 + 2];
    {
      // no fused multiply-add here: rnd(rnd(p) - rnd(q)) is the exact negative of rnd(rnd(q) - rnd(p)), so a face and its flipped
      // twin cancel to an exact zero, which rnd(p - rnd(q)) would not give
#pragma clang fp contract(off)
      const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      sx += cx;
      sy += cy;
      sz += cz;
    }
  }
  if (bad && fr == 0) atomicAdd(bad_faces, bad);
  const float len = sqrtf(sx * sx + sy * sy + sz * sz);
  float* o = normals + ((size_t)fr * Nv + v) * 3;
  const bool ok = len > 0.0f && len <= 3.402823466e+38f;
  o[0] = ok ? sx / len : 0.0f;
  o[1] = ok ? sy / len : 0.0f;
  o[2] = ok ? sz / len : 0.0f;
}

// the chart triangle of face f at texel (i, j): barycentrics b (corner k of the face as stored) and the mesh corners id; false
// when the texel has no usable face (an index out of range, an invalid chart vertex, zero area)
__device__ inline bool bake_setup(const MeshBakeArgs& a, int f, int i, int j, int id[3], float b[3]) {
  if ((unsigned)f >= (unsigned)a.Nf) return false;
  int x[3], y[3];
  for (int c = 0; c < 3; ++c) {
    id[c] = a.faces[(size_t)f * 3 + c];
    const int t = a.face_uv[(size_t)f * 3 + c];
    if ((unsigned)id[c] >= (unsigned)a.Nv || (unsigned)t >= (unsigned)a.Nt) return false;
    x[c] = a.uv_xy[(size_t)t * 2];
    y[c] = a.uv_xy[(size_t)t * 2 + 1];
    if (!mesh_vertex_ok(x[c], y[c], 1)) return false;
  }
  long long A = (long long)(x[1] - x[0]) * (y[2] - y[0]) - (long long)(y[1] - y[0]) * (x[2] - x[0]);
  if (A == 0) return false;
  const bool swapped = A < 0;
  if (swapped) {
    int s;
    s = x[1], x[1] = x[2], x[2] = s;
    s = y[1], y[1] = y[2], y[2] = s;
    A = -A;
  }
  long long e[3];
  mesh_edge_functions(x, y, (long long)j << MESH_SUB, (long long)i << MESH_SUB, e);
  const float fa = (float)A;
  b[0] = (float)e[0] / fa;
  b[swapped ? 2 : 1] = (float)e[1] / fa;
  b[swapped ? 1 : 2] = (float)e[2] / fa;
  return true;
}

// view n at the surface point p with normal nrm of face f: the integers of the projection, the visibility test, and where
// visible the weight and the colour
// RT, K, centres: the kernel's own __restrict__ parameters (see mesh_texel_bake_kernel), uniform over the workgroup
__device__ inline bool bake_view(const MeshBakeArgs& a, const float* __restrict__ RT, const float* __restrict__ K,
                                 const float* __restrict__ centres, int n, int f, const float p[3], const float nrm[3], int& xs, int& ys,
                                 int& kk, float& wgt, float c[3]) {
  mesh_project_point(RT + (size_t)n * 12, K + (size_t)n * 9, p[0], p[1], p[2], a.z_near, xs, ys, kk);
  wgt = 0.0f;
  if (!mesh_vertex_ok(xs, ys, kk)) return false;
  const int pj = (xs + MESH_ONE / 2) >> MESH_SUB, pi = (ys + MESH_ONE / 2) >> MESH_SUB;
  if (pj < 0 || pj >= a.W || pi < 0 || pi >= a.H) return false;
  const size_t pix = ((size_t)n * a.H + pi) * a.W + pj;
  const int fid = a.face_id[pix];
  if (fid < 0) return false;
  if (fid != f && (long long)kk + a.bias < (long long)a.pix_key[pix]) return false;
  wgt = mesh_view_weight(nrm[0], nrm[1], nrm[2], centres[n * 3] - p[0], centres[n * 3 + 1] - p[1], centres[n * 3 + 2] - p[2], a.power,
                         a.two_sided);
  mesh_view_bilinear(a.images, a.dtype, a.layout, a.H, a.W, n, xs, ys, c);
  return true;
}

__device__ inline void bake_fill(const MeshBakeArgs& a, size_t t, int seen, float wsum) {
  a.texture[t * 3] = a.fill[0];
  a.texture[t * 3 + 1] = a.fill[1];
  a.texture[t * 3 + 2] = a.fill[2];
  a.weight_sum[t] = wsum;
  a.n_seen[t] = seen;
  a.spread[t] = __int_as_float(0x7fc00000);
}

// The camera rows come in as __restrict__ parameters of their own, not through the argument struct: the view loop stores through
// the struct's tap pointers, and only a no-alias pointer lets the compiler prove the rows unclobbered and load them with scalar
// loads (s_load_dwordx4 / x8 at an address uniform over the wave) instead of one vector load per lane.
__global__ __launch_bounds__(UV_T) void mesh_texel_bake_kernel(MeshBakeArgs a, const float* __restrict__ RT, const float* __restrict__ K,
                                                               const float* __restrict__ centres) {
  const int j = blockIdx.x * UV_TILE + (threadIdx.x & (UV_TILE - 1)), i = blockIdx.y * UV_TILE + (threadIdx.x / UV_TILE);
  if (i >= a.Ht || j >= a.Wt) return;
  const size_t t = (size_t)i * a.Wt + j, nt = (size_t)a.Ht * a.Wt;
  int f, id[3] = {0, 0, 0};
  float b[3] = {0.0f, 0.0f, 0.0f};
  f = a.tex_face[t];
  if (f >= 0 && !bake_setup(a, f, i, j, id, b)) f = -1;
  if (f < 0) {  // a tile without a covered texel ends here in all its threads, before the view loop
    bake_fill(a, t, 0, 0.0f);
    const float nan = __int_as_float(0x7fc00000);
    if (a.pos) a.pos[t * 3] = nan, a.pos[t * 3 + 1] = nan, a.pos[t * 3 + 2] = nan;
    if (a.visible || a.txy || a.tkey)
      for (int n = 0; n < a.N; ++n) {
        if (a.visible) a.visible[n * nt + t] = 0;
        if (a.txy) a.txy[(n * nt + t) * 2] = 0, a.txy[(n * nt + t) * 2 + 1] = 0;
        if (a.tkey) a.tkey[n * nt + t] = 0;
      }
    return;
  }
  float p[3], nrm[3];
  for (int c = 0; c < 3; ++c) {
    p[c] = b[0] * a.verts[(size_t)id[0] * 3 + c] + b[1] * a.verts[(size_t)id[1] * 3 + c] + b[2] * a.verts[(size_t)id[2] * 3 + c];
    nrm[c] = b[0] * a.normals[(size_t)id[0] * 3 + c] + b[1] * a.normals[(size_t)id[1] * 3 + c] + b[2] * a.normals[(size_t)id[2] * 3 + c];
  }
  if (a.pos) a.pos[t * 3] = p[0], a.pos[t * 3 + 1] = p[1], a.pos[t * 3 + 2] = p[2];
  float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f};
  int seen = 0;
  unsigned long long mask = 0;
  for (int n = 0; n < a.N; ++n) {
    int xs, ys, kk;
    float w, c[3];
    const bool vis = bake_view(a, RT, K, centres, n, f, p, nrm, xs, ys, kk, w, c);
    if (a.visible) a.visible[n * nt + t] = vis ? 1 : 0;
    if (a.txy) a.txy[(n * nt + t) * 2] = xs, a.txy[(n * nt + t) * 2 + 1] = ys;
    if (a.tkey) a.tkey[n * nt + t] = kk;
    if (!vis) continue;
    if (n < 64) mask |= 1ull << n;
    ++seen;
    sw += w;
    for (int ch = 0; ch < 3; ++ch) sc[ch] += w * c[ch];
  }
  if (!(sw > 0.0f)) {
    bake_fill(a, t, seen, sw);
    return;
  }
  const float m[3] = {sc[0] / sw, sc[1] / sw, sc[2] / sw};
  float acc = 0.0f;
  for (int n = 0; n < a.N; ++n) {
    if (n < 64 && !((mask >> n) & 1ull)) continue;
    int xs, ys, kk;
    float w, c[3];
    if (!bake_view(a, RT, K, centres, n, f, p, nrm, xs, ys, kk, w, c)) continue;
    const float d0 = c[0] - m[0], d1 = c[1] - m[1], d2 = c[2] - m[2];
    acc += w * ((d0 * d0 + d1 * d1 + d2 * d2) * (1.0f / 3.0f));
  }
  for (int ch = 0; ch < 3; ++ch) a.texture[t * 3 + ch] = m[ch];
  a.weight_sum[t] = sw;
  a.n_seen[t] = seen;
  a.spread[t] = sqrtf(acc / sw);
}

__global__ __launch_bounds__(UV_T) void mesh_texture_dilate_kernel(const float* __restrict__ src, const unsigned char* __restrict__ vsrc,
                                                                   int Ht, int Wt, float* __restrict__ dst, unsigned char* __restrict__ vdst) {
  const int p = blockIdx.x * UV_T + threadIdx.x;
  if (p >= Ht * Wt) return;
  const int i = p / Wt, j = p % Wt;
  float c0 = src[(size_t)p * 3], c1 = src[(size_t)p * 3 + 1], c2 = src[(size_t)p * 3 + 2];
  unsigned char ok = vsrc[p] ? 1 : 0;
  if (!ok) {
    const int di[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dj[8] = {0, 1, 1, 1, 0, -1, -1, -1};  // N, NE, E, SE, S, SW, W, NW; row 0 is the top
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ii = i + di[k], jj = j + dj[k];
      if (ii < 0 || ii >= Ht || jj < 0 || jj >= Wt) continue;
      const int q = ii * Wt + jj;
      if (!vsrc[q]) continue;
      s0 += src[(size_t)q * 3];
      s1 += src[(size_t)q * 3 + 1];
      s2 += src[(size_t)q * 3 + 2];
      ++cnt;
    }
    if (cnt) {
      const float d = (float)cnt;
      c0 = s0 / d, c1 = s1 / d, c2 = s2 / d;
      ok = 1;
    }
  }
  dst[(size_t)p * 3] = c0;
  dst[(size_t)p * 3 + 1] = c1;
  dst[(size_t)p * 3 + 2] = c2;
  vdst[p] = ok;
}

__global__ __launch_bounds__(UV_T) void mesh_render_uv_kernel(const int* __restrict__ xy, const int* __restrict__ key,
                                                              const int* __restrict__ face_id, const int* __restrict__ faces,
                                                              const int* __restrict__ face_uv, const float* __restrict__ uv,
                                                              const float* __restrict__ texture, int Nv, int Nf, int Nt, int H, int W, int Ht,
                                                              int Wt, int layout, float bg_r, float bg_g, float bg_b,
                                                              float* __restrict__ images) {
  const int p = blockIdx.x * UV_T + threadIdx.x, n = blockIdx.y;
  if (p >= H * W) return;
  const int i = p / W, j = p % W;
  float c[3] = {bg_r, bg_g, bg_b};
  const int f = face_id[(size_t)n * H * W + p];
  if ((unsigned)f < (unsigned)Nf) {
    int id[3], tid[3], x[3], y[3], k[3];
    bool ok = true;
    for (int q = 0; q < 3; ++q) {
      id[q] = faces[(size_t)f * 3 + q];
      tid[q] = face_uv[(size_t)f * 3 + q];
      ok &= (unsigned)id[q] < (unsigned)Nv && (unsigned)tid[q] < (unsigned)Nt;
    }
    if (ok) {
      for (int q = 0; q < 3; ++q) {
        const size_t o = (size_t)n * Nv + id[q];
        x[q] = xy[o * 2], y[q] = xy[o * 2 + 1], k[q] = key[o];
        ok &= mesh_vertex_ok(x[q], y[q], k[q]);
      }
    }
    long long A = 0;
    if (ok) A = (long long)(x[1] - x[0]) * (y[2] - y[0]) - (long long)(y[1] - y[0]) * (x[2] - x[0]);
    if (A != 0) {
      const bool swapped = A < 0;
      if (swapped) {
        int s;
        s = x[1], x[1] = x[2], x[2] = s;
        s = y[1], y[1] = y[2], y[2] = s;
        s = k[1], k[1] = k[2], k[2] = s;
      }
      long long e[3];
      mesh_edge_functions(x, y, (long long)j << MESH_SUB, (long long)i << MESH_SUB, e);
      const long long g0 = e[0] * k[0], g1 = e[1] * k[1], g2 = e[2] * k[2], G = g0 + g1 + g2;
      if (G > 0) {
        float b[3];
        b[0] = (float)((double)g0 / (double)G);
        b[swapped ? 2 : 1] = (float)((double)g1 / (double)G);
        b[swapped ? 1 : 2] = (float)((double)g2 / (double)G);
        const float u = b[0] * uv[(size_t)tid[0] * 2] + b[1] * uv[(size_t)tid[1] * 2] + b[2] * uv[(size_t)tid[2] * 2];
        const float v = b[0] * uv[(size_t)tid[0] * 2 + 1] + b[1] * uv[(size_t)tid[1] * 2 + 1] + b[2] * uv[(size_t)tid[2] * 2 + 1];
        const float tx = u * (float)Wt - 0.5f, ty = (1.0f - v) * (float)Ht - 0.5f;
        if (fabsf(tx) <= 16384.0f && fabsf(ty) <= 16384.0f) {  // false for a NaN: the conversions below stay in range
          const float x0 = floorf(tx), y0 = floorf(ty);
          const float fx = tx - x0, fy = ty - y0;
          const int ja = min(max((int)x0, 0), Wt - 1), jb = min(max((int)x0 + 1, 0), Wt - 1);
          const int ia = min(max((int)y0, 0), Ht - 1), ib = min(max((int)y0 + 1, 0), Ht - 1);
          for (int ch = 0; ch < 3; ++ch) {
            const float c00 = texture[((size_t)ia * Wt + ja) * 3 + ch], c01 = texture[((size_t)ia * Wt + jb) * 3 + ch];
            const float c10 = texture[((size_t)ib * Wt + ja) * 3 + ch], c11 = texture[((size_t)ib * Wt + jb) * 3 + ch];
            const float top = c00 + fx * (c01 - c00), bot = c10 + fx * (c11 - c10);
            c[ch] = top + fy * (bot - top);
          }
        }
      }
    }
  }
  for (int ch = 0; ch < 3; ++ch) {
    const size_t o = layout == 0 ? (((size_t)n * 3 + ch) * H + i) * W + j : (((size_t)n * H + i) * W + j) * 3 + ch;
    images[o] = 2.0f * c[ch] - 1.0f;
  }
}

bool uv_bad_counts(int N, int Nv, int Nf) { return N < 1 || N > 65535 || Nv < 1 || Nf < 1 || (long long)N * Nv > 0x3fffffffLL || Nf > 0x2aaaaaaa; }

}  // namespace

int mesh_vertex_normals_check(const char* who, const float* verts, const int* faces, const int* inc_ptr, const int* inc_face, int F, int Nv,
                              int Nf, const float* normals, const int* bad_faces) {
  if (!verts || !faces || !inc_ptr || !inc_face || !normals || !bad_faces) return uv_fail(who, ": null argument");
  if (uv_bad_counts(F, Nv, Nf)) return uv_fail(who, ": F must be in 1..65535, Nv and Nf at least 1, F Nv below 2^30 and 3 Nf below 2^31");
  return 0;
}

int launch_mesh_vertex_normals(const float* verts, const int* faces, const int* inc_ptr, const int* inc_face, int F, int Nv, int Nf,
                               float* normals, int* bad_faces, hipStream_t s) {
  HIP_CHECK_RET(hipMemsetAsync(bad_faces, 0, sizeof(int), s));
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3((Nv + UV_T - 1) / UV_T, F), dim3(UV_T), 0, s, verts, faces, inc_ptr, inc_face, Nv, Nf,
                     normals, bad_faces);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int mesh_texel_bake_check(const char* who, const MeshBakeArgs& a) {
  if (!a.images || !a.face_id || !a.pix_key || !a.K || !a.RT || !a.centres || !a.verts || !a.normals || !a.faces || !a.uv_xy || !a.face_uv ||
      !a.tex_face || !a.texture || !a.weight_sum || !a.n_seen || !a.spread)
    return uv_fail(who, ": null argument");
  if (uv_bad_counts(a.N, a.Nv, a.Nf) || a.Nt < 1)
    return uv_fail(who, ": N must be in 1..65535, Nv, Nf and Nt at least 1, N Nv below 2^30 and 3 Nf below 2^31");
  if (mesh_bad_image(a.N, a.H, a.W)) return uv_fail(who, ": H and W must be in 1..4096 and N H W below 2^31");
  if (mesh_bad_image(a.N, a.Ht, a.Wt)) return uv_fail(who, ": Ht and Wt must be in 1..4096 and N Ht Wt below 2^31");
  if (a.dtype != 0 && a.dtype != 1) return uv_fail(who, ": dtype must be 0 (float32) or 1 (uint8)");
  if (a.layout != 0 && a.layout != 1) return uv_fail(who, ": layout must be 0 ([N,3,H,W]) or 1 ([N,H,W,3])");
  if (!(a.z_near > 0.0f) || !(a.z_near <= 3.402823466e+38f)) return uv_fail(who, ": z_near must be positive and finite");
  if (!(a.power >= 1.0f) || !(a.power <= 3.402823466e+38f)) return uv_fail(who, ": power must be at least 1 and finite");
  return 0;
}

int launch_mesh_texel_bake(const MeshBakeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mesh_texel_bake_kernel, dim3((a.Wt + UV_TILE - 1) / UV_TILE, (a.Ht + UV_TILE - 1) / UV_TILE), dim3(UV_T), 0, s, a, a.RT, a.K, a.centres);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int mesh_texture_dilate_check(const char* who, const float* texture, const unsigned char* valid, int Ht, int Wt, int passes,
                              const float* texture_out, const unsigned char* valid_out) {
  if (!texture || !valid || !texture_out || !valid_out) return uv_fail(who, ": null argument");
  if (mesh_bad_image(1, Ht, Wt)) return uv_fail(who, ": Ht and Wt must be in 1..4096");
  if (passes < 0 || passes > 64) return uv_fail(who, ": passes must be in 0..64");
  if (texture == texture_out || valid == valid_out) return uv_fail(who, ": the outputs must not alias the inputs");
  return 0;
}

// 16-byte aligned halves: a texture and a validity plane
size_t mesh_texture_dilate_scratch_bytes(int Ht, int Wt) { return (size_t)Ht * Wt * 3 * sizeof(float) + (((size_t)Ht * Wt + 15) & ~(size_t)15); }

// scratch: mesh_texture_dilate_scratch_bytes(Ht, Wt) bytes, alive until the launches have run (unused when passes < 2)
int launch_mesh_texture_dilate(const float* texture, const unsigned char* valid, int Ht, int Wt, int passes, float* texture_out,
                               unsigned char* valid_out, void* scratch, hipStream_t s) {
  const size_t nt = (size_t)Ht * Wt;
  if (passes == 0) {
    HIP_CHECK_RET(hipMemcpyAsync(texture_out, texture, nt * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(valid_out, valid, nt, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  float* tbuf = (float*)scratch;
  unsigned char* vbuf = (unsigned char*)scratch + nt * 3 * sizeof(float);
  const float* src = texture;
  const unsigned char* vsrc = valid;
  for (int r = 0; r < passes; ++r) {
    const bool to_out = ((passes - 1 - r) & 1) == 0;  // the last round writes the outputs
    float* dst = to_out ? texture_out : tbuf;
    unsigned char* vdst = to_out ? valid_out : vbuf;
    hipLaunchKernelGGL(mesh_texture_dilate_kernel, dim3((unsigned)((nt + UV_T - 1) / UV_T)), dim3(UV_T), 0, s, src, vsrc, Ht, Wt, dst, vdst);
    HIP_CHECK_RET(hipGetLastError());
    src = dst, vsrc = vdst;
  }
  return 0;
}

int mesh_render_uv_check(const char* who, const int* xy, const int* key, const int* face_id, const int* faces, const int* face_uv,
                         const float* uv, const float* texture, int N, int Nv, int Nf, int Nt, int H, int W, int Ht, int Wt, int layout,
                         const float* images) {
  if (!xy || !key || !face_id || !faces || !face_uv || !uv || !texture || !images) return uv_fail(who, ": null argument");
  if (uv_bad_counts(N, Nv, Nf) || Nt < 1)
    return uv_fail(who, ": N must be in 1..65535, Nv, Nf and Nt at least 1, N Nv below 2^30 and 3 Nf below 2^31");
  if (mesh_bad_image(N, H, W) || (long long)N * H * W * 3 > 0x7fffffffLL) return uv_fail(who, ": H and W must be in 1..4096 and 3 N H W below 2^31");
  if (mesh_bad_image(1, Ht, Wt)) return uv_fail(who, ": Ht and Wt must be in 1..4096");
  if (layout != 0 && layout != 1) return uv_fail(who, ": layout must be 0 ([N,3,H,W]) or 1 ([N,H,W,3])");
  return 0;
}

int launch_mesh_render_uv(const int* xy, const int* key, const int* face_id, const int* faces, const int* face_uv, const float* uv,
                          const float* texture, int N, int Nv, int Nf, int Nt, int H, int W, int Ht, int Wt, int layout, float bg_r, float bg_g,
                          float bg_b, float* images, hipStream_t s) {
  hipLaunchKernelGGL(mesh_render_uv_kernel, dim3((H * W + UV_T - 1) / UV_T, N), dim3(UV_T), 0, s, xy, key, face_id, faces, face_uv, uv, texture,
                     Nv, Nf, Nt, H, W, Ht, Wt, layout, bg_r, bg_g, bg_b, images);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
