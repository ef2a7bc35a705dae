// Mesh texturing from generated views -- include/mvd.h: mvd_op_mesh_project, mvd_op_mesh_raster, mvd_op_mesh_vertex_colors.
// Everything downstream of the projection is integer arithmetic, so that it can be tested for equality.
//   screen coordinates  int32 in 1/16 pixel (MESH_SUB = 4 fractional bits); pixel (i, j) has its centre at (u, v) = (j, i), the
//                       conditioner's convention.  Guard band |u|, |v| <= 4096 px, so |xs|, |ys| <= 2^16.
//   depth keys          int32 in 1..MESH_KMAX = 2^24 - 1, key = rint(z_near / Z * KMAX): larger is nearer, and z_near / Z is linear
//                       in screen space, so integer interpolation of keys orders depth correctly.  key 0 = invalid vertex.
//   bounds              a coordinate difference is below 2^17 and a pixel centre minus a vertex below 2^17, so an edge function
//                       dx (py - ay) - dy (px - ax) stays within 2^35 in int64; e_0 + e_1 + e_2 = A (twice the area, <= 2^35) with every
//                       e_k >= 0 inside, so the key interpolation sum e_k key_k <= A KMAX stays within 2^59 in int64.  The raster
//                       kernel enforces the preconditions itself: a vertex with a key outside 1..KMAX or a coordinate beyond the
//                       guard band is invalid there, whoever produced it.
// Launches:
//   mesh_project_kernel  one thread per (view, vertex), fp32.
//   mesh_raster_kernel   grid (ceil(Nf / 256), N): thread t sets up face 256 b + t of its view (validity, orientation, bounding box
//                        clamped to the image BEFORE any loop) and walks a box of at most MESH_SMALL pixels itself -- the common
//                        case, triangles of 2-4 pixels.  A larger box goes on a list in LDS, and after a barrier the 256 threads
//                        walk each listed box together, pixel p of it in thread p % 256: a screen-filling triangle at 2048^2 is
//                        16 384 pixels per thread.  No trip count depends on unclamped data.  The winner of a pixel is the 64-bit
//                        atomicMax of (key << 32) | (0xFFFFFFFF - face) in a cleared buffer: the largest key, ties to the smallest
//                        face index, whatever the arrival order.  Faces with an index outside [0, Nv) are never dereferenced and
//                        are counted (once, by view 0) into a device counter.
//   mesh_resolve_kernel  one thread per pixel: face_id (-1 background) and pix_key (0 background) out of the packed winner.
//   mesh_vertex_colors_kernel  one thread per vertex, views in index order, two passes (weighted mean, then the weighted spread
//                        about it), fp32 in a fixed order and no floating-point atomics: two calls agree bit for bit.
// The projection chain, the vertex test, the weight and the bilinear sample are csrc/mesh.h, shared with k_mesh_uv.hip.
#include "mesh.h"

namespace {

constexpr int MESH_T = 256, MESH_SMALL = 32;

__global__ __launch_bounds__(MESH_T) void mesh_project_kernel(const float* __restrict__ verts, const float* __restrict__ K,
                                                              const float* __restrict__ RT, int N, int Nv, float z_near,
                                                              int* __restrict__ xy, int* __restrict__ key) {
  const int v = blockIdx.x * MESH_T + threadIdx.x, n = blockIdx.y;
  if (v >= Nv) return;
  const float* r = RT + (size_t)n * 12;
  const float* k = K + (size_t)n * 9;
  const float x = verts[(size_t)v * 3], y = verts[(size_t)v * 3 + 1], z = verts[(size_t)v * 3 + 2];
  int xs, ys, kk;
  mesh_project_point(r, k, x, y, z, z_near, xs, ys, kk);
  const size_t o = (size_t)n * Nv + v;
  xy[o * 2] = xs;
  xy[o * 2 + 1] = ys;
  key[o] = kk;
}

struct MeshTri {
  int x[3], y[3], k[3];
  int j0, j1, i0, i1;  // bounding box in pixels, inclusive, inside the image
  int f;
};

// twice the signed area after the orientation swap (> 0), or 0 when the face draws nothing in this view; bad: an index outside [0, Nv)
__device__ inline long long mesh_setup(const int* __restrict__ xy, const int* __restrict__ key, const int* __restrict__ faces, int n,
                                       int f, int Nv, int H, int W, MeshTri& t, bool& bad) {
  int id[3];
  bad = false;
  for (int c = 0; c < 3; ++c) {
    id[c] = faces[(size_t)f * 3 + c];
    bad |= (unsigned)id[c] >= (unsigned)Nv;
  }
  if (bad) return 0;
  bool ok = true;
  for (int c = 0; c < 3; ++c) {
    const size_t o = (size_t)n * Nv + id[c];
    t.x[c] = xy[o * 2];
    t.y[c] = xy[o * 2 + 1];
    t.k[c] = key[o];
    ok &= mesh_vertex_ok(t.x[c], t.y[c], t.k[c]);
  }
  if (!ok) return 0;
  long long A = (long long)(t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (long long)(t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
  if (A == 0) return 0;
  if (A < 0) {
    int s;
    s = t.x[1], t.x[1] = t.x[2], t.x[2] = s;
    s = t.y[1], t.y[1] = t.y[2], t.y[2] = s;
    s = t.k[1], t.k[1] = t.k[2], t.k[2] = s;
    A = -A;
  }
  const int xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
  const int ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
  // pixel centres 16 j inside [xmin, xmax]: ceil and floor by arithmetic shifts, then the clamp to the image
  t.j0 = max((xmin + MESH_ONE - 1) >> MESH_SUB, 0);
  t.j1 = min(xmax >> MESH_SUB, W - 1);
  t.i0 = max((ymin + MESH_ONE - 1) >> MESH_SUB, 0);
  t.i1 = min(ymax >> MESH_SUB, H - 1);
  t.f = f;
  if (t.j0 > t.j1 || t.i0 > t.i1) return 0;
  return A;
}

__device__ inline void mesh_pixel(const MeshTri& t, long long A, int i, int j, unsigned long long* __restrict__ win, int W) {
  const long long px = (long long)j << MESH_SUB, py = (long long)i << MESH_SUB;
  long long e[3];
  mesh_edge_functions(t.x, t.y, px, py, e);  // csrc/mesh.h: the one definition, shared with the texel bake and the UV render
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const long long dx = t.x[b] - t.x[a], dy = t.y[b] - t.y[a];
    in &= e[k] > 0 || (e[k] == 0 && (dy < 0 || (dy == 0 && dx > 0)));
  }
  if (!in) return;
  const long long kk = (e[0] * t.k[0] + e[1] * t.k[1] + e[2] * t.k[2]) / A;
  atomicMax(win + (size_t)i * W + j, ((unsigned long long)kk << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t.f));
}

__global__ __launch_bounds__(MESH_T) void mesh_raster_kernel(const int* __restrict__ xy, const int* __restrict__ key,
                                                             const int* __restrict__ faces, int Nv, int Nf, int H, int W,
                                                             unsigned long long* __restrict__ win, int* __restrict__ bad_faces) {
  __shared__ MeshTri s_tri[MESH_T];
  __shared__ long long s_area[MESH_T];
  __shared__ int s_n;
  const int t = threadIdx.x, n = blockIdx.y, f = blockIdx.x * MESH_T + t;
  unsigned long long* w = win + (size_t)n * H * W;
  if (t == 0) s_n = 0;
  __syncthreads();
  if (f < Nf) {
    MeshTri tri;
    bool bad;
    const long long A = mesh_setup(xy, key, faces, n, f, Nv, H, W, tri, bad);
    if (bad && n == 0) atomicAdd(bad_faces, 1);
    if (A > 0) {
      const int bw = tri.j1 - tri.j0 + 1, bh = tri.i1 - tri.i0 + 1;  // both in 1..4096
      if (bw * bh <= MESH_SMALL) {
        for (int p = 0; p < bw * bh; ++p) mesh_pixel(tri, A, tri.i0 + p / bw, tri.j0 + p % bw, w, W);
      } else {
        const int slot = atomicAdd(&s_n, 1);  // the order of the list does not reach the result: the winner is a maximum
        s_tri[slot] = tri;
        s_area[slot] = A;
      }
    }
  }
  __syncthreads();
  const int nl = s_n;  // <= MESH_T, the same in every thread
  for (int l = 0; l < nl; ++l) {
    const MeshTri tri = s_tri[l];
    const long long A = s_area[l];
    const int bw = tri.j1 - tri.j0 + 1, np = bw * (tri.i1 - tri.i0 + 1);  // <= 2^24
    for (int p = t; p < np; p += MESH_T) mesh_pixel(tri, A, tri.i0 + p / bw, tri.j0 + p % bw, w, W);
  }
}

__global__ __launch_bounds__(MESH_T) void mesh_resolve_kernel(const unsigned long long* __restrict__ win, size_t npix,
                                                              int* __restrict__ face_id, int* __restrict__ pix_key) {
  const size_t p = (size_t)blockIdx.x * MESH_T + threadIdx.x;
  if (p >= npix) return;
  const unsigned long long v = win[p];
  face_id[p] = v ? (int)(0xFFFFFFFFu - (unsigned)(v & 0xFFFFFFFFull)) : -1;
  pix_key[p] = (int)(v >> 32);
}

struct MeshColorArgs {
  const void* img;
  const int *xy, *key, *faces, *face_id, *pix_key;
  const float *normals, *centres, *verts;
  int dtype, layout, N, Nv, Nf, H, W, bias, two_sided;
  float power;
};

// the integer visibility test of vertex v in view n, its weight and, where visible, its bilinear colour at the snapped position
__device__ inline bool mesh_view_sample(const MeshColorArgs& a, int n, int v, float nx, float ny, float nz, float& wgt, float c[3]) {
  const size_t o = (size_t)n * a.Nv + v;
  const int xs = a.xy[o * 2], ys = a.xy[o * 2 + 1], kv = a.key[o];
  wgt = 0.0f;
  if (!mesh_vertex_ok(xs, ys, kv)) return false;
  const int pj = (xs + MESH_ONE / 2) >> MESH_SUB, pi = (ys + MESH_ONE / 2) >> MESH_SUB;
  if (pj < 0 || pj >= a.W || pi < 0 || pi >= a.H) return false;
  const size_t pix = ((size_t)n * a.H + pi) * a.W + pj;
  const int fid = a.face_id[pix];
  if (fid < 0) return false;
  bool corner = false;
  if (fid < a.Nf) corner = a.faces[(size_t)fid * 3] == v || a.faces[(size_t)fid * 3 + 1] == v || a.faces[(size_t)fid * 3 + 2] == v;
  if (!corner && (long long)kv + a.bias < (long long)a.pix_key[pix]) return false;
  // weight: cos of the angle between the normal and the direction to the camera centre
  const float dx = a.centres[n * 3] - a.verts[(size_t)v * 3], dy = a.centres[n * 3 + 1] - a.verts[(size_t)v * 3 + 1],
              dz = a.centres[n * 3 + 2] - a.verts[(size_t)v * 3 + 2];
  wgt = mesh_view_weight(nx, ny, nz, dx, dy, dz, a.power, a.two_sided);
  mesh_view_bilinear(a.img, a.dtype, a.layout, a.H, a.W, n, xs, ys, c);
  return true;
}

__global__ __launch_bounds__(MESH_T) void mesh_vertex_colors_kernel(MeshColorArgs a, float fill_r, float fill_g, float fill_b,
                                                                    float* __restrict__ color, float* __restrict__ weight_sum,
                                                                    int* __restrict__ n_seen, float* __restrict__ spread,
                                                                    unsigned char* __restrict__ visible) {
  const int v = blockIdx.x * MESH_T + threadIdx.x;
  if (v >= a.Nv) return;
  const float nx = a.normals[(size_t)v * 3], ny = a.normals[(size_t)v * 3 + 1], nz = a.normals[(size_t)v * 3 + 2];
  float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f};
  int seen = 0;
  for (int n = 0; n < a.N; ++n) {
    float w, c[3];
    const bool vis = mesh_view_sample(a, n, v, nx, ny, nz, w, c);
    if (visible) visible[(size_t)n * a.Nv + v] = vis ? 1 : 0;
    if (!vis) continue;
    ++seen;
    sw += w;
    for (int ch = 0; ch < 3; ++ch) sc[ch] += w * c[ch];
  }
  n_seen[v] = seen;
  weight_sum[v] = sw;
  if (!(sw > 0.0f)) {
    color[(size_t)v * 3] = fill_r;
    color[(size_t)v * 3 + 1] = fill_g;
    color[(size_t)v * 3 + 2] = fill_b;
    spread[v] = __int_as_float(0x7fc00000);
    return;
  }
  const float m[3] = {sc[0] / sw, sc[1] / sw, sc[2] / sw};
  float acc = 0.0f;
  for (int n = 0; n < a.N; ++n) {
    float w, c[3];
    if (!mesh_view_sample(a, n, v, nx, ny, nz, w, c)) continue;
    const float d0 = c[0] - m[0], d1 = c[1] - m[1], d2 = c[2] - m[2];
    acc += w * ((d0 * d0 + d1 * d1 + d2 * d2) * (1.0f / 3.0f));
  }
  for (int ch = 0; ch < 3; ++ch) color[(size_t)v * 3 + ch] = m[ch];
  spread[v] = sqrtf(acc / sw);
}

int mesh_fail(const char* who, const char* what) { return mvd_fail((std::string(who) + what).c_str()); }

}  // namespace

int mesh_project_check(const char* who, const float* verts, const float* K, const float* RT, int N, int Nv, float z_near, const int* xy,
                       const int* key) {
  if (!verts || !K || !RT || !xy || !key) return mesh_fail(who, ": null argument");
  if (N < 1 || N > 65535 || Nv < 1) return mesh_fail(who, ": N must be in 1..65535 and Nv at least 1");
  if ((long long)N * Nv > 0x3fffffffLL) return mesh_fail(who, ": N Nv must be below 2^30");
  if (!(z_near > 0.0f) || !(z_near <= 3.402823466e+38f)) return mesh_fail(who, ": z_near must be positive and finite");
  return 0;
}

int launch_mesh_project(const float* verts, const float* K, const float* RT, int N, int Nv, float z_near, int* xy, int* key, hipStream_t s) {
  hipLaunchKernelGGL(mesh_project_kernel, dim3((Nv + MESH_T - 1) / MESH_T, N), dim3(MESH_T), 0, s, verts, K, RT, N, Nv, z_near, xy, key);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int mesh_raster_check(const char* who, const int* xy, const int* key, const int* faces, int N, int Nv, int Nf, int H, int W,
                      const int* face_id, const int* pix_key, const int* bad_faces) {
  if (!xy || !key || !faces || !face_id || !pix_key || !bad_faces) return mesh_fail(who, ": null argument");
  if (N < 1 || N > 65535 || Nv < 1 || Nf < 1) return mesh_fail(who, ": N must be in 1..65535, Nv and Nf at least 1");
  if ((long long)N * Nv > 0x3fffffffLL || Nf > 0x2aaaaaaa) return mesh_fail(who, ": N Nv must be below 2^30 and 3 Nf below 2^31");
  if (mesh_bad_image(N, H, W)) return mesh_fail(who, ": H and W must be in 1..4096 and N H W below 2^31");
  return 0;
}

size_t mesh_raster_scratch_bytes(int N, int H, int W) { return (size_t)N * H * W * sizeof(unsigned long long); }

// scratch: mesh_raster_scratch_bytes(N, H, W) bytes, 8-byte aligned, alive until the launches have run
int launch_mesh_raster(const int* xy, const int* key, const int* faces, int N, int Nv, int Nf, int H, int W, int* face_id, int* pix_key,
                       int* bad_faces, void* scratch, hipStream_t s) {
  const size_t npix = (size_t)N * H * W;
  unsigned long long* win = (unsigned long long*)scratch;
  HIP_CHECK_RET(hipMemsetAsync(win, 0, npix * sizeof(unsigned long long), s));
  HIP_CHECK_RET(hipMemsetAsync(bad_faces, 0, sizeof(int), s));
  hipLaunchKernelGGL(mesh_raster_kernel, dim3((Nf + MESH_T - 1) / MESH_T, N), dim3(MESH_T), 0, s, xy, key, faces, Nv, Nf, H, W, win,
                     bad_faces);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((npix + MESH_T - 1) / MESH_T)), dim3(MESH_T), 0, s,
                     (const unsigned long long*)win, npix, face_id, pix_key);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int mesh_vertex_colors_check(const char* who, const void* images, int dtype, int layout, const int* xy, const int* key, const int* faces,
                             const int* face_id, const int* pix_key, const float* verts, const float* normals, const float* centres, int N,
                             int Nv, int Nf, int H, int W, float power, const float* color, const float* weight_sum, const int* n_seen,
                             const float* spread) {
  if (!images || !xy || !key || !faces || !face_id || !pix_key || !verts || !normals || !centres || !color || !weight_sum || !n_seen || !spread)
    return mesh_fail(who, ": null argument");
  if (N < 1 || N > 65535 || Nv < 1 || Nf < 1) return mesh_fail(who, ": N must be in 1..65535, Nv and Nf at least 1");
  if ((long long)N * Nv > 0x3fffffffLL || Nf > 0x2aaaaaaa) return mesh_fail(who, ": N Nv must be below 2^30 and 3 Nf below 2^31");
  if (mesh_bad_image(N, H, W)) return mesh_fail(who, ": H and W must be in 1..4096 and N H W below 2^31");
  if (dtype != 0 && dtype != 1) return mesh_fail(who, ": dtype must be 0 (float32) or 1 (uint8)");
  if (layout != 0 && layout != 1) return mesh_fail(who, ": layout must be 0 ([N,3,H,W]) or 1 ([N,H,W,3])");
  if (!(power >= 1.0f) || !(power <= 3.402823466e+38f)) return mesh_fail(who, ": power must be at least 1 and finite");
  return 0;
}

int launch_mesh_vertex_colors(const void* images, int dtype, int layout, const int* xy, const int* key, const int* faces, const int* face_id,
                              const int* pix_key, const float* verts, const float* normals, const float* centres, int N, int Nv, int Nf,
                              int H, int W, float power, int bias, int two_sided, float fill_r, float fill_g, float fill_b, float* color,
                              float* weight_sum, int* n_seen, float* spread, unsigned char* visible, hipStream_t s) {
  MeshColorArgs a;
  a.img = images, a.xy = xy, a.key = key, a.faces = faces, a.face_id = face_id, a.pix_key = pix_key;
  a.normals = normals, a.centres = centres, a.verts = verts;
  a.dtype = dtype, a.layout = layout, a.N = N, a.Nv = Nv, a.Nf = Nf, a.H = H, a.W = W, a.bias = bias, a.two_sided = two_sided;
  a.power = power;
  hipLaunchKernelGGL(mesh_vertex_colors_kernel, dim3((Nv + MESH_T - 1) / MESH_T), dim3(MESH_T), 0, s, a, fill_r, fill_g, fill_b, color,
                     weight_sum, n_seen, spread, visible);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
