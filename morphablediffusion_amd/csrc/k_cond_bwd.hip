// Backward kernels of the mesh conditioner (SpatialVolumeNet, morphable_diffusion.py:151-320; networks network.py): the
// adjoints of the gathers of k_cond.hip (the same coordinate maps, cond.h; scatter instead of gather), the sparse voxel CNN's layers in
// train mode (conv dgrad / wgrad through the neighbour tables, BatchNorm1d with batch statistics + ReLU), the view fusion, and
// the transposing im2col for the frustum network's 3-D convolutions.
// The three scatters use hardware fp32 atomic adds (unsafeAtomicAdd: the returning CAS loop of plain atomicAdd is 30x slower here) (unordered: the conditioner's gradients are reproducible to rounding, not bit
// for bit -- the UNet's are); everything else has fixed summation orders.
// Those atomic forms are the DEFAULT.  The deterministic mode (mvd_train_set_deterministic) runs the three adjoints, and the fold
// of duplicate vertices' rows, as gathers instead (cbwd_*_gather_adj, cbwd_lattice_to_views_adj, cbwd_sparse_fold_dups_det below):
// no floating-point atomic to HBM or LDS, every sum in an order fixed by indices alone, every output element written.
#include "cond.h"

namespace {

inline int gridn(size_t n, int cap = 8192) {
  size_t g = (n + 255) / 256;
  return (int)(g > (size_t)cap ? (size_t)cap : (g < 1 ? 1 : g));
}

// adjoint of frustum_gather_kernel: d_vol[corner][c] += w * d_out[point][c]   (d_out fp32 [TN*D*S*S][64])
__global__ __launch_bounds__(256) void frustum_scatter_kernel(const float* __restrict__ d_out, const ViewCam* __restrict__ cams,
                                                              const int* __restrict__ view_idx, int TN, int D, int S, int V, float vol_len,
                                                              int persp, float* __restrict__ d_vol) {
  constexpr int C = 64;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long pt = gid >> 4;
  const int cq = (int)(gid & 15) * 4;
  const long npts = (long)TN * D * S * S;
  if (pt >= npts) return;
  const int x = (int)(pt % S), y = (int)((pt / S) % S), d = (int)((pt / ((long)S * S)) % D), tv = (int)(pt / ((long)S * S * D));
  const ViewCam cam = cams[view_idx[tv]];
  float px, py, pz;
  frustum_to_lattice(cam, x, y, d, D, S, V, vol_len, persp, px, py, pz);
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
  const float tx = px - fx, ty = py - fy, tz = pz - fz;
  const float4 g = *(const float4*)(d_out + pt * C + cq);
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {
    const int bx = corner & 1, by = (corner >> 1) & 1, bz = corner >> 2;
    const int xx = x0 + bx, yy = y0 + by, zz = z0 + bz;
    if (xx < 0 || xx > V - 1 || yy < 0 || yy > V - 1 || zz < 0 || zz > V - 1) continue;
    const float wgt = trilinear_weight(bx, by, bz, tx, ty, tz);
    float* o = d_vol + (((long)zz * V + yy) * V + xx) * C + cq;
    unsafeAtomicAdd(o + 0, wgt * g.x);
    unsafeAtomicAdd(o + 1, wgt * g.y);
    unsafeAtomicAdd(o + 2, wgt * g.z);
    unsafeAtomicAdd(o + 3, wgt * g.w);
  }
}

// adjoint of latent_gather_kernel: d_rows[row][c] += w * d_vol[point][c]
__global__ void latent_scatter_kernel(const float* __restrict__ d_vol, const int* __restrict__ grid, int gd, int gh, int gw, float minx,
                                      float miny, float minz, float shx, float shy, float shz, float voxel, int V, float vol_len, int C,
                                      float* __restrict__ d_rows) {
  const long total = (long)V * V * V * C;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const int pt = (int)(idx / C);
    const int ix = pt % V, iy = (pt / V) % V, iz = pt / (V * V);
    const float px = latent_axis_pos(minx, shx, gw, voxel, V, vol_len, ix), py = latent_axis_pos(miny, shy, gh, voxel, V, vol_len, iy),
                pz = latent_axis_pos(minz, shz, gd, voxel, V, vol_len, iz);
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float tx = px - fx, ty = py - fy, tz = pz - fz;
    const float g = d_vol[idx];
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const int bx = corner & 1, by = (corner >> 1) & 1, bz = corner >> 2;
      const int xx = x0 + bx, yy = y0 + by, zz = z0 + bz;
      if (xx < 0 || xx > gw - 1 || yy < 0 || yy > gh - 1 || zz < 0 || zz > gd - 1) continue;
      const int row = grid[((long)zz * gh + yy) * gw + xx];
      if (row < 0) continue;
      const float wgt = trilinear_weight(bx, by, bz, tx, ty, tz);
      unsafeAtomicAdd(d_rows + (long)row * C + c, wgt * g);
    }
  }
}

// adjoint of vertex_gather_kernel: d_feats[view][pixel][c] += w2 * d_out[view][vertex][c].  One workgroup per view accumulates the
// whole S x S x 16 image in LDS (ds_add_f32: thousands of vertices land on the same few hundred pixels) and writes it once.
// gridDim.y workgroups share a view (each takes a slice of the vertices, its own LDS image, and adds it to HBM with fp32 atomics).
__global__ __launch_bounds__(1024) void vertex_scatter_kernel(const float* __restrict__ d_out, const ViewCam* __restrict__ cams,
                                                              const int* __restrict__ view_idx, const float* __restrict__ verts, int Nv, int V,
                                                              float vol_len, int S, int persp, float* __restrict__ d_feats) {
  extern __shared__ float s_img[];  // [16][S*S] channel-major: the lanes of a wave hit different pixels, i.e. different banks
  const int SS = S * S;
  const int view = blockIdx.x;
  const ViewCam cam = cams[view_idx[view]];
  for (int i = threadIdx.x; i < S * S * 16; i += blockDim.x) s_img[i] = 0.f;
  __syncthreads();
  // thread = (vertex, corner): 8 threads share a vertex
  const int per = (Nv + gridDim.y - 1) / gridDim.y, v_beg = blockIdx.y * per, v_end = min(Nv, v_beg + per);
  for (int job = v_beg * 8 + threadIdx.x; job < v_end * 8; job += blockDim.x) {
    const int vi = job >> 3, corner = job & 7;
    float fr[3];
    int lo[3];
    vertex_cell(verts, vi, V, vol_len, lo, fr);
    const int bx = corner & 1, by = (corner >> 1) & 1, bz = corner >> 2;
    const int ix = lo[0] + bx, iy = lo[1] + by, iz = lo[2] + bz;
    if (ix < 0 || ix > V - 1 || iy < 0 || iy > V - 1 || iz < 0 || iz > V - 1) continue;
    const float w3 = trilinear_weight(bx, by, bz, fr[0], fr[1], fr[2]);
    float px, py;
    lattice_to_map(cam.P, ix, iy, iz, V, vol_len, S, persp, px, py);
    const float fx0 = floorf(px), fy0 = floorf(py);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float tx = px - fx0, ty = py - fy0;
    const float* gsrc = d_out + ((long)view * Nv + vi) * 16;
    float g16[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) g16[c] = gsrc[c];
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int xx = x0 + (tap & 1), yy = y0 + (tap >> 1);
      if (xx < 0 || xx > S - 1 || yy < 0 || yy > S - 1) continue;
      const float w2 = bilinear_weight(tap, tx, ty) * w3;
      float* o = s_img + yy * S + xx;
#pragma unroll
      for (int c = 0; c < 16; ++c) unsafeAtomicAdd(o + c * SS, w2 * g16[c]);
    }
  }
  __syncthreads();
  float* fv = d_feats + (long)view * S * S * 16;
  for (int i = threadIdx.x; i < S * S * 16; i += blockDim.x) {
    const float v = s_img[(i & 15) * SS + (i >> 4)];
    if (v != 0.f) unsafeAtomicAdd(fv + i, v);
  }
}

// ---- deterministic mode: the same three adjoints as GATHERS -- one thread owns an output element, finds its contributions and
// adds them in an order that is a function of indices only; no floating-point atomic, every output element written (no zero
// fill).  Candidates come from a conservative index box, membership is decided by the forward's own position arithmetic, so
// every (point, corner) pair is counted exactly once whatever the box's rounding.
constexpr float BOX_FINITE = 1e9f;  // a box bound beyond this (or NaN) means: scan everything

// Lattice positions pos[point][3] of all frustum points, one thread per point, by frustum_scatter_kernel's map (cond.h).  The
// gather below reads them instead of recomputing them per candidate: once per point, not once per (candidate, channel quad),
// and -- a straight-line kernel of the map gets the same fused multiply-adds, whereas the same code inside the gather's loops
// is fused differently after hoisting -- the same fp32 positions as the atomic form's.  (With positions recomputed in the loops
// the two forms' dL/d(volume) differed by 1.07e-5 relative L2 at V = 32, with positions in double by 0.99e-5: fp32 rounding of
// x * depth against Pinv's small entries, not summation order.)
__global__ __launch_bounds__(256) void frustum_positions_kernel(const ViewCam* __restrict__ cams, const int* __restrict__ view_idx, int TN,
                                                                int D, int S, int V, float vol_len, int persp, float* __restrict__ pos) {
  const long pt = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long npts = (long)TN * D * S * S;
  if (pt >= npts) return;
  const int x = (int)(pt % S), y = (int)((pt / S) % S), d = (int)((pt / ((long)S * S)) % D), tv = (int)(pt / ((long)S * S * D));
  const ViewCam cam = cams[view_idx[tv]];
  float px, py, pz;
  frustum_to_lattice(cam, x, y, d, D, S, V, vol_len, persp, px, py, pz);
  pos[pt * 3 + 0] = px;
  pos[pt * 3 + 1] = py;
  pos[pt * 3 + 2] = pz;
}

// [lo, hi] := the indices 0..n-1 inside [mn - 1, mx + 1]; false when a bound is not a usable number
__device__ __forceinline__ bool index_window(float mn, float mx, int n, int& lo, int& hi) {
  if (!(fabsf(mn) < BOX_FINITE) || !(fabsf(mx) < BOX_FINITE)) return false;
  lo = max(0, (int)floorf(mn) - 1);
  hi = min(n - 1, (int)ceilf(mx) + 1);
  return true;
}

// Index box (d, y, x) of the frustum points that can have lattice voxel (xx, yy, zz) among their eight corners: they lie in the
// voxel's +-1 cube, whose image under the inverse of the forward's map (the affine Pinv inverted here, then the perspective
// divide or the inverse of Kinv's 2x2 block) is inside the bounding box of its eight corners' images -- as long as the
// projective map keeps its orientation on the cube, i.e. every corner's depth is at least the forward's clamp.  Otherwise, and
// whenever a bound is not a finite number, the box is the whole frustum.
__device__ void frustum_box(const ViewCam& cam, int xx, int yy, int zz, int D, int S, int V, float vol_len, int persp, int lo[3],
                            int hi[3]) {
  lo[0] = lo[1] = lo[2] = 0;
  hi[0] = D - 1;
  hi[1] = hi[2] = S - 1;
  const float* m = cam.Pinv;
  const float c00 = m[5] * m[10] - m[6] * m[9], c01 = m[2] * m[9] - m[1] * m[10], c02 = m[1] * m[6] - m[2] * m[5];
  const float c10 = m[6] * m[8] - m[4] * m[10], c11 = m[0] * m[10] - m[2] * m[8], c12 = m[2] * m[4] - m[0] * m[6];
  const float c20 = m[4] * m[9] - m[5] * m[8], c21 = m[1] * m[8] - m[0] * m[9], c22 = m[0] * m[5] - m[1] * m[4];
  const float inv_det = 1.f / (m[0] * c00 + m[1] * c10 + m[2] * c20);
  const float k_det = cam.Kinv[0] * cam.Kinv[4] - cam.Kinv[1] * cam.Kinv[3];
  const float hs = 0.5f * (float)(S - 1), d_scale = (float)(D - 1) / (cam.far_ - cam.near_);
  float mn[3] = {3e38f, 3e38f, 3e38f}, mx[3] = {-3e38f, -3e38f, -3e38f};
  bool ok = true;
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {
    const float lx = (float)(xx + ((corner & 1) ? 1 : -1)), ly = (float)(yy + ((corner & 2) ? 1 : -1)),
                lz = (float)(zz + ((corner & 4) ? 1 : -1));
    const float wx = (lx / (float)(V - 1) * 2.f - 1.f) * vol_len - m[3], wy = (ly / (float)(V - 1) * 2.f - 1.f) * vol_len - m[7],
                wz = (lz / (float)(V - 1) * 2.f - 1.f) * vol_len - m[11];
    const float a = (c00 * wx + c01 * wy + c02 * wz) * inv_det, b = (c10 * wx + c11 * wy + c12 * wz) * inv_det,
                c = (c20 * wx + c21 * wy + c22 * wz) * inv_det;
    float fx, fy;
    if (persp) {
      if (!(c >= 1e-4f)) ok = false;
      fx = a / c;
      fy = b / c;
    } else {
      const float ra = a - cam.Kinv[2], rb = b - cam.Kinv[5];
      fx = ((cam.Kinv[4] * ra - cam.Kinv[1] * rb) / k_det + 1.f) * hs;
      fy = ((cam.Kinv[0] * rb - cam.Kinv[3] * ra) / k_det + 1.f) * hs;
    }
    const float f[3] = {(c - cam.near_) * d_scale, fy, fx};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!(fabsf(f[k]) < BOX_FINITE)) ok = false;
      mn[k] = fminf(mn[k], f[k]);
      mx[k] = fmaxf(mx[k], f[k]);
    }
  }
  if (!ok) return;
  int l[3], h[3];
  const int n[3] = {D, S, S};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (!index_window(mn[k], mx[k], n[k], l[k], h[k])) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = l[k];
    hi[k] = h[k];
  }
}

// is lattice index `i` one of floor(p), floor(p) + 1?  -> its linear weight; compared as floats (p may be far outside int range)
__device__ __forceinline__ bool corner_weight(float p, int i, float& w) {
  const float f = floorf(p), e = (float)i - f, t = p - f;
  w = e == 0.f ? 1.f - t : t;
  return e == 0.f || e == 1.f;
}

// d_vol[voxel][c] = sum over (view, d, y, x) ascending of w * d_out[point][c]: one thread per (voxel, channel quad)
__global__ __launch_bounds__(256) void frustum_gather_adj_kernel(const float* __restrict__ d_out, const ViewCam* __restrict__ cams,
                                                                 const int* __restrict__ view_idx, const float* __restrict__ pos, int TN,
                                                                 int D, int S, int V, float vol_len, int persp,
                                                                 float* __restrict__ d_vol) {
  constexpr int C = 64;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long vox = gid >> 4;
  const int cq = (int)(gid & 15) * 4;
  if (vox >= (long)V * V * V) return;
  const int xx = (int)(vox % V), yy = (int)((vox / V) % V), zz = (int)(vox / ((long)V * V));
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int tv = 0; tv < TN; ++tv) {
    const ViewCam cam = cams[view_idx[tv]];
    int lo[3], hi[3];
    frustum_box(cam, xx, yy, zz, D, S, V, vol_len, persp, lo, hi);
    for (int d = lo[0]; d <= hi[0]; ++d)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[2]; x <= hi[2]; ++x) {
          const long pt = (((long)tv * D + d) * S + y) * S + x;
          float wx, wy, wz;
          if (!corner_weight(pos[pt * 3], xx, wx) || !corner_weight(pos[pt * 3 + 1], yy, wy) || !corner_weight(pos[pt * 3 + 2], zz, wz))
            continue;
          const float wgt = wx * wy * wz;
          const float4 g = *(const float4*)(d_out + pt * C + cq);
          acc.x += wgt * g.x;
          acc.y += wgt * g.y;
          acc.z += wgt * g.z;
          acc.w += wgt * g.w;
        }
  }
  *(float4*)(d_vol + vox * C + cq) = acc;
}

// Lattice indices whose grid coordinate p(i) = k (X(i) - mn), X(i) = -L + i 2L / (V - 1), can fall into (cell - 1, cell + 1),
// padded by one; the whole axis when the map is degenerate (a one-cell axis: k = 0)
__device__ __forceinline__ void latent_axis_window(float mn, float sh, int g, int cell, float voxel, int V, float vol_len, int& lo,
                                                   int& hi) {
  lo = 0;
  hi = V - 1;
  const float k = (float)(g - 1) / (voxel * sh), istep = (float)(V - 1) / (2.f * vol_len);
  if (!(k > 0.f)) return;
  const float a = (((float)(cell - 1)) / k + mn + vol_len) * istep, b = (((float)(cell + 1)) / k + mn + vol_len) * istep;
  int l, h;
  if (index_window(fminf(a, b), fmaxf(a, b), V, l, h)) {
    lo = l;
    hi = h;
  }
}
// d_rows[grid[cell]][c] = sum over lattice points (iz, iy, ix) ascending of w * d_vol[point][c]: one thread per (cell, channel);
// cells without a row are skipped, every row belongs to exactly one cell, so every row is written
__global__ __launch_bounds__(256) void latent_gather_adj_kernel(const float* __restrict__ d_vol, const int* __restrict__ grid, int gd,
                                                                int gh, int gw, float minx, float miny, float minz, float shx, float shy,
                                                                float shz, float voxel, int V, float vol_len, float* __restrict__ d_rows) {
  constexpr int C = 64;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long cell = gid >> 6;
  const int c = (int)(gid & 63);
  if (cell >= (long)gd * gh * gw) return;
  const int row = grid[cell];
  if (row < 0) return;
  const int xx = (int)(cell % gw), yy = (int)((cell / gw) % gh), zz = (int)(cell / ((long)gw * gh));
  int x0, x1, y0, y1, z0, z1;
  latent_axis_window(minx, shx, gw, xx, voxel, V, vol_len, x0, x1);
  latent_axis_window(miny, shy, gh, yy, voxel, V, vol_len, y0, y1);
  latent_axis_window(minz, shz, gd, zz, voxel, V, vol_len, z0, z1);
  float acc = 0.f;
  for (int iz = z0; iz <= z1; ++iz) {
    float wz;
    if (!corner_weight(latent_axis_pos(minz, shz, gd, voxel, V, vol_len, iz), zz, wz)) continue;
    for (int iy = y0; iy <= y1; ++iy) {
      float wy;
      if (!corner_weight(latent_axis_pos(miny, shy, gh, voxel, V, vol_len, iy), yy, wy)) continue;
      for (int ix = x0; ix <= x1; ++ix) {
        float wx;
        if (!corner_weight(latent_axis_pos(minx, shx, gw, voxel, V, vol_len, ix), xx, wx)) continue;
        acc += wx * wy * wz * d_vol[(((long)iz * V + iy) * V + ix) * C + c];
      }
    }
  }
  d_rows[(long)row * C + c] = acc;
}

// ---- vertex adjoint in two stages through the lattice: d_feats = B^T (A^T d_vf), weight = w3(vertex, corner) * w2(voxel, view, tap)
// The voxel -> (vertex, corner) lists are built inside the call without atomics: every voxel's thread walks the vertices in
// index order twice (count, then fill behind an exclusive scan of the counts), so a list is in ascending vertex order by
// construction (a vertex has at most one corner on a voxel).  The walk reads one packed int per vertex.
constexpr int VKEY_BITS = 10, VKEY_MASK = (1 << VKEY_BITS) - 1;  // per axis: floor(position) + 2, clamped to [0, V + 2]
__global__ void vertex_key_kernel(const float* __restrict__ verts, int Nv, int V, float vol_len, int* __restrict__ key) {
  const int vi = blockIdx.x * blockDim.x + threadIdx.x;
  if (vi >= Nv) return;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float pos = vertex_axis_pos(verts, vi, a, V, vol_len);
    const float f = fminf(fmaxf(floorf(pos), -2.f), (float)V);  // (outside [-1, V - 1] no corner is on the lattice)
    k |= ((int)f + 2) << (VKEY_BITS * a);
  }
  key[vi] = k;
}
// corner (0..7) of vertex key k that sits on voxel (xx, yy, zz), or -1
__device__ __forceinline__ int vertex_corner_on(int k, int xx, int yy, int zz) {
  const int dx = xx + 2 - (k & VKEY_MASK), dy = yy + 2 - ((k >> VKEY_BITS) & VKEY_MASK), dz = zz + 2 - ((k >> (2 * VKEY_BITS)) & VKEY_MASK);
  return ((unsigned)dx <= 1u && (unsigned)dy <= 1u && (unsigned)dz <= 1u) ? (dx | (dy << 1) | (dz << 2)) : -1;
}
// FILL = false: cnt[voxel] = its (vertex, corner) pairs.  FILL = true: the pairs (vertex, w3) behind off[voxel], and the
// compact list of occupied voxels (ascending: occ_rank is a prefix sum over voxel order).
template <bool FILL>
__global__ __launch_bounds__(256) void vertex_bins_kernel(const int* __restrict__ key, const float* __restrict__ verts, int Nv, int V,
                                                          float vol_len, int* __restrict__ cnt, const int* __restrict__ off,
                                                          const int* __restrict__ occ_rank, int* __restrict__ list_v,
                                                          float* __restrict__ list_w, int* __restrict__ occ_list) {
  const int vox = blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= V * V * V) return;
  const int xx = vox % V, yy = (vox / V) % V, zz = vox / (V * V);
  int n = FILL ? off[vox] : 0;
  const int first = n;
  for (int vi = 0; vi < Nv; ++vi) {
    const int corner = vertex_corner_on(key[vi], xx, yy, zz);
    if (corner < 0) continue;
    if (FILL) {
      float fr[3];
      int lo[3];
      vertex_cell(verts, vi, V, vol_len, lo, fr);
      list_v[n] = vi;
      list_w[n] = trilinear_weight(corner & 1, (corner >> 1) & 1, corner >> 2, fr[0], fr[1], fr[2]);
    }
    ++n;
  }
  if (!FILL) cnt[vox] = n;
  else if (n > first) occ_list[occ_rank[vox]] = vox;
}
// One workgroup: off[0..n] = exclusive prefix sum of cnt, occ_rank[0..n) = exclusive prefix count of non-empty entries,
// *n_occ = their number.  Integers only.
__global__ __launch_bounds__(1024) void vertex_scan_kernel(const int* __restrict__ cnt, int n, int* __restrict__ off,
                                                           int* __restrict__ occ_rank, int* __restrict__ n_occ) {
  __shared__ int s_a[1024], s_b[1024];
  const int t = threadIdx.x, per = (n + 1023) / 1024, b = min(n, t * per), e = min(n, b + per);
  int a = 0, q = 0;
  for (int i = b; i < e; ++i) {
    a += cnt[i];
    q += cnt[i] > 0;
  }
  s_a[t] = a;
  s_b[t] = q;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int va = t >= d ? s_a[t - d] : 0, vb = t >= d ? s_b[t - d] : 0;
    __syncthreads();
    s_a[t] += va;
    s_b[t] += vb;
    __syncthreads();
  }
  a = s_a[t] - a;  // exclusive
  q = s_b[t] - q;
  for (int i = b; i < e; ++i) {
    off[i] = a;
    occ_rank[i] = q;
    a += cnt[i];
    q += cnt[i] > 0;
  }
  if (t == 1023) {
    off[n] = s_a[1023];
    *n_occ = s_b[1023];
  }
}
// stage A: d_lat[view][j][c] = sum over the list of occupied voxel j (ascending vertex) of w3 * d_vf[view][vertex][c]
__global__ __launch_bounds__(256) void vertex_to_lattice_adj_kernel(const float* __restrict__ d_vf, const int* __restrict__ off,
                                                                    const int* __restrict__ occ_list, const int* __restrict__ n_occ,
                                                                    const int* __restrict__ list_v, const float* __restrict__ list_w,
                                                                    int Nv, int stride, float* __restrict__ d_lat) {
  const int view = blockIdx.y, gid = blockIdx.x * blockDim.x + threadIdx.x, j = gid >> 4, c = gid & 15;
  if (j >= min(*n_occ, stride)) return;
  const int vox = occ_list[j], b = off[vox], e = off[vox + 1];
  const float* src = d_vf + (long)view * Nv * 16 + c;
  float acc = 0.f;
  for (int i = b; i < e; ++i) acc += list_w[i] * src[(long)list_v[i] * 16];
  d_lat[((long)view * stride + j) * 16 + c] = acc;
}
// stage B, step 1: where lattice voxel vox_list[j] (NULL: voxel j) lands in every view's map, as (x0, y0, tx, ty), once per
// (view, voxel).  Positions far outside the map are pulled to its rim + 1, where no tap is inside either.
__global__ void lattice_project_kernel(const ViewCam* __restrict__ cams, const int* __restrict__ view_idx, const int* __restrict__ vox_list,
                                       const int* __restrict__ n_ptr, int n_max, int V, float vol_len, int S, int persp,
                                       float4* __restrict__ rec) {
  const int view = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (n_ptr ? min(*n_ptr, n_max) : n_max)) return;
  const ViewCam cam = cams[view_idx[view]];
  const int vox = vox_list ? vox_list[j] : j;
  const int ix = vox % V, iy = (vox / V) % V, iz = vox / (V * V);
  float px, py;
  lattice_to_map(cam.P, ix, iy, iz, V, vol_len, S, persp, px, py);
  px = fminf(fmaxf(px, -2.f), (float)(S + 1));
  py = fminf(fmaxf(py, -2.f), (float)(S + 1));
  const float fx0 = floorf(px), fy0 = floorf(py);
  rec[(long)view * n_max + j] = make_float4(__int_as_float((int)fx0), __int_as_float((int)fy0), px - fx0, py - fy0);
}
// stage B, step 2: d_feats[view][pixel][c] = sum over voxels j ascending of w2 * d_lat[view][j][c] (a pixel is at most one of a
// voxel's four taps): one thread per (pixel, channel quad); the voxels' records stream past every pixel of the view through LDS
__global__ __launch_bounds__(256) void lattice_to_views_adj_kernel(const float* __restrict__ d_lat, const float4* __restrict__ rec,
                                                                   const int* __restrict__ n_ptr, int n_max, int S,
                                                                   float* __restrict__ d_feats) {
  __shared__ float4 s_rec[256];
  const int view = blockIdx.y, t = threadIdx.x, pix = blockIdx.x * 64 + (t >> 2), q = (t & 3) * 4;
  const int n = n_ptr ? min(*n_ptr, n_max) : n_max;
  const bool valid = pix < S * S;
  const int xp = pix % S, yp = pix / S;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int base = 0; base < n; base += 256) {
    __syncthreads();
    if (base + t < n) s_rec[t] = rec[(long)view * n_max + base + t];
    __syncthreads();
    const int m = min(256, n - base);
    if (!valid) continue;
    for (int i = 0; i < m; ++i) {
      const float4 r = s_rec[i];
      const int dx = xp - __float_as_int(r.x), dy = yp - __float_as_int(r.y);
      if ((unsigned)dx > 1u || (unsigned)dy > 1u) continue;
      const float w = (dx ? r.z : 1.f - r.z) * (dy ? r.w : 1.f - r.w);
      const float4 g = *(const float4*)(d_lat + ((long)view * n_max + base + i) * 16 + q);
      acc.x += w * g.x;
      acc.y += w * g.y;
      acc.z += w * g.z;
      acc.w += w * g.w;
    }
  }
  if (valid) *(float4*)(d_feats + ((long)view * S * S + pix) * 16 + q) = acc;
}

// sparse_fold_dups_kernel without atomics: a representative that has duplicates (flagged by them) adds their rows in row order
__global__ void fold_dups_flag_kernel(const int* __restrict__ nbr, int n, int* __restrict__ flag) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int r = nbr[(long)s * 27 + 13];
  if (r != s && r >= 0) flag[r] = 1;
}
__global__ void fold_dups_sum_kernel(float* __restrict__ d, const int* __restrict__ nbr, const int* __restrict__ flag, int n, int C) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)n * C; e += (long)gridDim.x * blockDim.x) {
    const int r = (int)(e / C);
    if (!flag[r]) continue;
    float acc = d[e];  // (only duplicates' rows are read below, only representatives' rows written: disjoint)
    for (int s = r + 1; s < n; ++s)  // the representative is the voxel's FIRST row
      if (nbr[(long)s * 27 + 13] == r) acc += d[(long)s * C + (e - (long)r * C)];
    d[e] = acc;
  }
}
__global__ void fold_dups_clear_kernel(float* __restrict__ d, const int* __restrict__ nbr, int n, int C) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)n * C; e += (long)gridDim.x * blockDim.x) {
    const int s = (int)(e / C), r = nbr[(long)s * 27 + 13];
    if (r != s && r >= 0) d[e] = 0.f;
  }
}

// ---- view fusion (SMPLFeatureExtractor, network.py:41-72): fused[v][co] = sum_ci w[co][ci] mean_view vf[view][v][ci] + b[co] ----
// d_vf[view][v][ci] = (1 / total_views) sum_co w[co][ci] d_fused[v][co]  (the same for every view)
__global__ void fuse_bwd_dvf_kernel(const float* __restrict__ d_fused, const float* __restrict__ w, int n_views, int Nv, int total_views,
                                    float* __restrict__ d_vf) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Nv * 16) return;
  const int v = idx >> 4, ci = idx & 15;
  float acc = 0.f;
#pragma unroll
  for (int co = 0; co < 16; ++co) acc += w[co * 16 + ci] * d_fused[(long)v * 16 + co];
  acc /= (float)total_views;
  for (int view = 0; view < n_views; ++view) d_vf[((long)view * Nv + v) * 16 + ci] = acc;
}
// dw[co][ci] += sum_v d_fused[v][co] mean_view vf[.][v][ci];  db[co] += sum_v d_fused[v][co].
// A workgroup takes FW_CH vertices: their view mean m[v][16] and gradient rows g[v][16] go to LDS with row-contiguous 16-byte
// loads (the one-workgroup-per-(co, ci) form walked the vertices with a 64-byte stride, 16 views each: 148 us per sample), then
// thread (co, ci) sums its 256-vertex partial from LDS; partials per chunk, added in chunk order by fuse_bwd_w_reduce_kernel.
constexpr int FW_CH = 256;
__global__ __launch_bounds__(256) void fuse_bwd_w_kernel(const float* __restrict__ d_fused, const float* __restrict__ vf, int n_views, int Nv,
                                                         int total_views, float* __restrict__ part) {
  __shared__ float s_m[FW_CH][17], s_g[FW_CH][17];  // (+1: the (co, ci) readers of a row do not share a bank)
  const int t = threadIdx.x, v0 = blockIdx.x * FW_CH;
  for (int e = t; e < FW_CH * 4; e += 256) {
    const int vl = e >> 2, q = e & 3, v = v0 + vl;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f), g = m;
    if (v < Nv) {
      for (int view = 0; view < n_views; ++view) {
        const float4 x = *(const float4*)(vf + ((long)view * Nv + v) * 16 + 4 * q);
        m.x += x.x; m.y += x.y; m.z += x.z; m.w += x.w;
      }
      g = *(const float4*)(d_fused + (long)v * 16 + 4 * q);
    }
    const float inv = 1.0f / (float)total_views;
    s_m[vl][4 * q] = m.x * inv; s_m[vl][4 * q + 1] = m.y * inv; s_m[vl][4 * q + 2] = m.z * inv; s_m[vl][4 * q + 3] = m.w * inv;
    s_g[vl][4 * q] = g.x; s_g[vl][4 * q + 1] = g.y; s_g[vl][4 * q + 2] = g.z; s_g[vl][4 * q + 3] = g.w;
  }
  __syncthreads();
  const int co = t >> 4, ci = t & 15;
  float a = 0.f, b = 0.f;
#pragma unroll 8
  for (int vl = 0; vl < FW_CH; ++vl) {
    const float g = s_g[vl][co];
    a += g * s_m[vl][ci];
    b += g;
  }
  part[(long)blockIdx.x * 272 + t] = a;
  if (ci == 0) part[(long)blockIdx.x * 272 + 256 + co] = b;
}
__global__ __launch_bounds__(256) void fuse_bwd_w_reduce_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ dw,
                                                                float* __restrict__ db) {
  const int t = threadIdx.x;
  float a = 0.f, b = 0.f;
  for (int c = 0; c < nchunk; ++c) {
    a += part[(long)c * 272 + t];
    if (t < 16) b += part[(long)c * 272 + 256 + t];
  }
  dw[t] += a;
  if (t < 16) db[t] += b;
}

// ---- sparse voxel CNN, train mode -------------------------------------------------------------------------------------
// BatchNorm1d (batch statistics over the n active rows, biased variance) + ReLU backward, rows [n][C] with C dividing 256.
// xraw = the conv output, stats = [mean | rstd] of the forward pass, dy = gradient w.r.t. relu(bn(xraw)); writes d xraw over dy
// (in place), dgamma / dbeta accumulated.  Two launches over chunks of 128 rows, every access a full row segment (the
// one-workgroup-per-channel form walked columns with a stride of C floats: 44 -> 12 us): per-chunk sums of du and du * xhat, then every workgroup adds the partials in chunk order
// and applies; workgroup 0 accumulates the parameter gradients.
constexpr int BNB_CH = 128;
__global__ __launch_bounds__(256) void bn_rows_bwd_sums_kernel(const float* __restrict__ xraw, const float* __restrict__ dy, int n, int C,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ stats, float* __restrict__ part) {
  __shared__ float s_a[256], s_b[256];
  const int RL = 256 / C, t = threadIdx.x, c = t % C, rl = t / C;
  const int r0 = blockIdx.x * BNB_CH, r1 = min(n, r0 + BNB_CH);
  float s1 = 0.f, s2 = 0.f;
  if (rl < RL) {
    const float mean = stats[c], rstd = stats[C + c], g = gamma[c], b = beta[c];
#pragma unroll 8
    for (int r = r0 + rl; r < r1; r += RL) {
      const float xh = (xraw[(long)r * C + c] - mean) * rstd;
      const float du = (g * xh + b) > 0.f ? dy[(long)r * C + c] : 0.f;
      s1 += du;
      s2 += du * xh;
    }
  }
  s_a[t] = s1;
  s_b[t] = s2;
  __syncthreads();
  if (rl == 0) {
    for (int i = 1; i < RL; ++i) {
      s1 += s_a[i * C + c];
      s2 += s_b[i * C + c];
    }
    part[((long)blockIdx.x * 2) * C + c] = s1;
    part[((long)blockIdx.x * 2 + 1) * C + c] = s2;
  }
}
__global__ __launch_bounds__(256) void bn_rows_bwd_apply_kernel(const float* __restrict__ xraw, float* __restrict__ dy, int n, int C,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ stats, const float* __restrict__ part, int nchunk,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float s_1[256], s_2[256];
  const int t = threadIdx.x;
  if (t < C) {
    float a = 0.f, q = 0.f;
    for (int k = 0; k < nchunk; ++k) {
      a += part[((long)k * 2) * C + t];
      q += part[((long)k * 2 + 1) * C + t];
    }
    if (blockIdx.x == 0) {
      dgamma[t] += q;
      dbeta[t] += a;
    }
    s_1[t] = a / (float)n;
    s_2[t] = q / (float)n;
  }
  __syncthreads();
  const long e0 = (long)blockIdx.x * BNB_CH * C, e1 = min((long)n * C, e0 + (long)BNB_CH * C);
#pragma unroll 8
  for (long e = e0 + t; e < e1; e += 256) {
    const int c = (int)(e % C);
    const float rstd = stats[C + c], g = gamma[c];
    const float xh = (xraw[e] - stats[c]) * rstd;
    const float du = (g * xh + beta[c]) > 0.f ? dy[e] : 0.f;
    dy[e] = g * rstd * (du - s_1[c] - xh * s_2[c]);
  }
}

// d_in[nbr[site][k]][ci] += sum_co w[k][ci][co] d_out[site][co]: one workgroup per output site
__global__ __launch_bounds__(256) void sparse_conv_dgrad_kernel(const float* __restrict__ d_out, const int* __restrict__ nbr, int Cin,
                                                                int Cout, const float* __restrict__ w, float* __restrict__ d_in) {
  __shared__ int s_nb[27];
  __shared__ float s_g[256];
  const int site = blockIdx.x, t = threadIdx.x;
  if (t < 27) s_nb[t] = nbr[(long)site * 27 + t];
  if (t < Cout) s_g[t] = d_out[(long)site * Cout + t];
  __syncthreads();
  const int ci = t % Cin, p = t / Cin, P = 256 / Cin;
  if (p >= P) return;
  for (int k = p; k < 27; k += P) {
    const int nb = s_nb[k];
    if (nb < 0) continue;
    const float* wk = w + ((long)k * Cin + ci) * Cout;
    float acc = 0.f;
    for (int co = 0; co < Cout; ++co) acc += wk[co] * s_g[co];
    unsafeAtomicAdd(d_in + (long)nb * Cin + ci, acc);
  }
}

// dw[k][ci][co] = sum_site in[nbr[site][k]][ci] d_out[site][co]: grid (27, ceil(Cin*Cout / 256), site chunks); every chunk of
// SP_CHUNK sites writes its partial product to part[chunk][27][Cin][Cout], summed in chunk order by sparse_wgrad_reduce_kernel.
// Only ~30 % of a surface mesh's (site, tap) pairs are active: each wave first compacts the active pairs of its quarter of the
// chunk into LDS (ballot + prefix popcount: site order is kept, so the sum order is fixed), then every thread walks the four
// lists -- a third of the iterations, none of them a skipped one, four independent loads in flight.
constexpr int SP_CHUNK = 256;
__global__ __launch_bounds__(256) void sparse_conv_wgrad_kernel(const float* __restrict__ in, const int* __restrict__ nbr,
                                                                const float* __restrict__ d_out, int n_out, int Cin, int Cout,
                                                                float* __restrict__ part) {
  __shared__ int s_nb[4][SP_CHUNK / 4], s_site[4][SP_CHUNK / 4], s_cnt[4];
  const int k = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x, chunk = blockIdx.z;
  const int s0 = chunk * SP_CHUNK, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < SP_CHUNK / 256; ++j) {
    const int site = s0 + wave * (SP_CHUNK / 4) + j * 64 + lane;
    const int nb = site < n_out ? nbr[(long)site * 27 + k] : -1;
    const unsigned long long m = __ballot(nb >= 0);
    if (nb >= 0) {
      const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
      s_nb[wave][pos] = nb;
      s_site[wave][pos] = site;
    }
    cnt += __popcll(m);
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (e >= Cin * Cout) return;
  const int ci = e / Cout, co = e - ci * Cout;
  const float* pin = in + ci;
  const float* pd = d_out + co;
  float acc = 0.f;
  for (int w = 0; w < 4; ++w) {
    const int n = s_cnt[w];
    int i = 0;
    for (; i + 4 <= n; i += 4) {
      const float a0 = pin[(long)s_nb[w][i] * Cin], a1 = pin[(long)s_nb[w][i + 1] * Cin], a2 = pin[(long)s_nb[w][i + 2] * Cin],
                  a3 = pin[(long)s_nb[w][i + 3] * Cin];
      const float b0 = pd[(long)s_site[w][i] * Cout], b1 = pd[(long)s_site[w][i + 1] * Cout], b2 = pd[(long)s_site[w][i + 2] * Cout],
                  b3 = pd[(long)s_site[w][i + 3] * Cout];
      acc += a0 * b0;
      acc += a1 * b1;
      acc += a2 * b2;
      acc += a3 * b3;
    }
    for (; i < n; ++i) acc += pin[(long)s_nb[w][i] * Cin] * pd[(long)s_site[w][i] * Cout];
  }
  part[(((long)chunk * 27 + k) * Cin + ci) * Cout + co] = acc;
}
// The same weight gradient on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32): a wave owns one tap of one chunk of
// SP_CHUNK output sites and the whole Cin x Cout tile; the K dimension of the MFMA is the list of ACTIVE (site, neighbour) pairs of
// that tap (compacted with ballot + prefix popcount: site order is kept, so the summation order is fixed), four pairs per
// instruction: lane (m = lane & 15, q = lane >> 4) supplies in[nbr of pair q][16 a + m] as A and d_out[site of pair q][16 b + m] as
// B -- both are 64-byte row segments, no transposes.  Partials per chunk as before, summed in chunk order by the reduce kernel.
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void sparse_wgrad_mfma_kernel(const float* __restrict__ in, const int* __restrict__ nbr,
                                                                const float* __restrict__ d_out, int n_out, float* __restrict__ part) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int CA = CIN / 16, CB = COUT / 16, G = 4;  // G groups of four pairs in flight
  __shared__ int s_i[4][SP_CHUNK], s_o[4][SP_CHUNK];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = blockIdx.x * 4 + wave, chunk = blockIdx.y, s0 = chunk * SP_CHUNK;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < SP_CHUNK / 64; ++j) {
    const int site = s0 + j * 64 + lane;
    const int nb = (k < 27 && site < n_out) ? nbr[(long)site * 27 + k] : -1;
    const unsigned long long mk = __ballot(nb >= 0);
    if (nb >= 0) {
      const int pos = cnt + __popcll(mk & ((1ull << lane) - 1ull));
      s_i[wave][pos] = nb;
      s_o[wave][pos] = site;
    }
    cnt += __popcll(mk);
  }
  __syncthreads();
  if (k >= 27) return;
  const int m = lane & 15, q = lane >> 4;
  f32x4 acc[CA][CB];
#pragma unroll
  for (int a = 0; a < CA; ++a)
#pragma unroll
    for (int b = 0; b < CB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = 0; base < cnt; base += 4 * G) {
    float av[G][CA], bv[G][CB];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int p = base + 4 * g + q;
      const bool ok = p < cnt;
      const int i = ok ? s_i[wave][p] : 0, o = ok ? s_o[wave][p] : 0;
#pragma unroll
      for (int a = 0; a < CA; ++a) av[g][a] = ok ? in[(long)i * CIN + a * 16 + m] : 0.f;
#pragma unroll
      for (int b = 0; b < CB; ++b) bv[g][b] = ok ? d_out[(long)o * COUT + b * 16 + m] : 0.f;
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int a = 0; a < CA; ++a)
#pragma unroll
        for (int b = 0; b < CB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][a], bv[g][b], acc[a][b], 0, 0, 0);
  }
  float* dst = part + ((long)chunk * 27 + k) * CIN * COUT;
#pragma unroll
  for (int a = 0; a < CA; ++a)
#pragma unroll
    for (int b = 0; b < CB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(long)(a * 16 + 4 * q + r) * COUT + b * 16 + m] = acc[a][b][r];
#endif
}

// inverse of a strided layer's table: inv[i][k] = the output site that reads input row i at tap k (at most one), else -1
__global__ void sparse_inverse_table_kernel(const int* __restrict__ nbr_down, int n_out, int* __restrict__ inv) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)n_out * 27; e += (long)gridDim.x * blockDim.x) {
    const int i = nbr_down[e];
    if (i >= 0) inv[(long)i * 27 + (int)(e % 27)] = (int)(e / 27);
  }
}
// Several vertices in one voxel: the later ones' rows equal the representative's (the one every neighbour lookup returns, the
// centre tap included), so their output gradients belong to the representative's row.  After this the level's table is symmetric
// over the rows that carry gradient, which is what the gather-form data-gradient needs.
__global__ void sparse_fold_dups_kernel(float* __restrict__ d, const int* __restrict__ nbr, int n, int C) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)n * C; e += (long)gridDim.x * blockDim.x) {
    const int s = (int)(e / C), c = (int)(e - (long)s * C);
    const int r = nbr[(long)s * 27 + 13];
    if (r != s && r >= 0) {
      unsafeAtomicAdd(d + (long)r * C + c, d[e]);
      d[e] = 0.f;
    }
  }
}

__global__ void sparse_wgrad_reduce_kernel(const float* __restrict__ part, int nchunk, long n, float* __restrict__ dw) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float a = 0.f;
    for (int c = 0; c < nchunk; ++c) a += part[(long)c * n + i];
    dw[i] = a;
  }
}

// packed [27][Cin][Cout] gradient -> added to the parameter's own layout (engine_weights.hip: build_sparse_layer)
__global__ void sparse_w_unpack_add_kernel(const float* __restrict__ pk, int Cin, int Cout, int layout, float* __restrict__ dst) {
  const long total = (long)27 * Cin * Cout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout), ci = (int)((i / Cout) % Cin), k = (int)(i / ((long)Cout * Cin));
    const long d = layout == 0 ? ((long)co * Cin + ci) * 27 + k : layout == 1 ? ((long)co * 27 + k) * Cin + ci : i;
    dst[d] += pk[i];
  }
}

// ---- transposing im2col of a 3-D conv (k3, pad 1, stride s): dst[(ci*27 + tap)][r] = X[b, zo*s+kz-1, yo*s+ky-1, xo*s+kx-1, ci] ----
template <typename T>
__global__ __launch_bounds__(256) void im2colT3d_kernel(const T* __restrict__ src, long ld, int B, int D, int H, int W, int C, int stride,
                                                        int Do, int Ho, int Wo, half_t* __restrict__ dst, int Rp) {
  __shared__ half_t tile[64][66];
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tap = blockIdx.z;
  const int kz = tap / 9 - 1, ky = (tap / 3) % 3 - 1, kx = tap % 3 - 1;
  const int R = B * Do * Ho * Wo;
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int rr = i >> 6, cc = i & 63;
    const int r = r0 + rr, c = c0 + cc;
    half_t v = (half_t)0;
    if (r < R && c < C) {
      const int xo = r % Wo, yo = (r / Wo) % Ho, zo = (r / (Wo * Ho)) % Do, b = r / (Wo * Ho * Do);
      const int z = zo * stride + kz, y = yo * stride + ky, x = xo * stride + kx;
      if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) v = (half_t)ldf(src + ((((long)b * D + z) * H + y) * W + x) * ld + c);
    }
    tile[rr][cc] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int cc = i >> 6, rr = i & 63;
    const int r = r0 + rr, c = c0 + cc;
    if (c < C && r < Rp) dst[((long)c * 27 + tap) * Rp + r] = tile[rr][cc];
  }
}

// with 8- / 16-byte accesses (see im2colT_vec_kernel, k_bwd.hip): four channels per gather, eight rows per store; same values
template <typename T>
__global__ __launch_bounds__(256) void im2colT3d_vec_kernel(const T* __restrict__ src, long ld, int B, int D, int H, int W, int C, int stride,
                                                            int Do, int Ho, int Wo, half_t* __restrict__ dst, int Rp) {
  __shared__ half_t tile[64][66];
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tap = blockIdx.z;
  const int kz = tap / 9 - 1, ky = (tap / 3) % 3 - 1, kx = tap % 3 - 1;
  const int R = B * Do * Ho * Wo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = threadIdx.x + 256 * j;
    const int rr = i >> 4, cc = (i & 15) * 4;
    const int r = r0 + rr, c = c0 + cc;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < R && c < C) {
      const int xo = r % Wo, yo = (r / Wo) % Ho, zo = (r / (Wo * Ho)) % Do, b = r / (Wo * Ho * Do);
      const int z = zo * stride + kz, y = yo * stride + ky, x = xo * stride + kx;
      if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) {
        const T* p = src + ((((long)b * D + z) * H + y) * W + x) * ld + c;
        if constexpr (sizeof(T) == 4) {
          const float4 q = *(const float4*)p;
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
          const h4 q = *(const h4*)p;
          v[0] = (float)q[0]; v[1] = (float)q[1]; v[2] = (float)q[2]; v[3] = (float)q[3];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[rr][cc + e] = (half_t)v[e];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = threadIdx.x + 256 * j;
    const int cc = i >> 3, g = i & 7;
    const int c = c0 + cc;
    if (c >= C) continue;
    h8 hv;
#pragma unroll
    for (int k = 0; k < 8; ++k) hv[k] = tile[g * 8 + k][cc];
    *(h8*)(dst + ((long)c * 27 + tap) * Rp + r0 + g * 8) = hv;
  }
}

// out[r][k] (+)= sum_n g[r][n] w[n][k]  (w fp16 [N][K], the LinW pack) for a handful of rows (FiLM / step-MLP adjoints).
// One workgroup = 16 consecutive k x 16 lanes over n, combined through LDS in lane order.
__global__ __launch_bounds__(256) void small_linear_bwd_kernel(const float* __restrict__ g, long ldg, int N, const half_t* __restrict__ w,
                                                               int K, float* __restrict__ out, long ldo, int accum) {
  __shared__ float s_p[16][17];
  const int r = blockIdx.y, kk = threadIdx.x & 15, nl = threadIdx.x >> 4, k = blockIdx.x * 16 + kk;
  float acc = 0.f;
  if (k < K)
    for (int n = nl; n < N; n += 16) acc += g[r * ldg + n] * (float)w[(long)n * K + k];
  s_p[nl][kk] = acc;
  __syncthreads();
  if (nl == 0 && k < K) {
    float a = 0.f;
    for (int i = 0; i < 16; ++i) a += s_p[i][kk];
    out[r * ldo + k] = accum ? out[r * ldo + k] + a : a;
  }
}

}  // namespace

int cbwd_frustum_scatter(const float* d_out, const ViewCam* cams, const int* view_idx, int TN, int D, int S, int V, float vol_len, int persp,
                         float* d_vol, hipStream_t s) {
  const long threads = (long)TN * D * S * S * 16;
  hipLaunchKernelGGL(frustum_scatter_kernel, dim3((int)((threads + 255) / 256)), dim3(256), 0, s, d_out, cams, view_idx, TN, D, S, V,
                     vol_len, persp, d_vol);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_latent_scatter(const float* d_vol, const int* grid, int gd, int gh, int gw, const float* min_xyz, const int* out_sh, float voxel,
                        int V, float vol_len, float* d_rows, hipStream_t s) {
  const int C = 64;
  const size_t total = (size_t)V * V * V * C;
  hipLaunchKernelGGL(latent_scatter_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, s, d_vol, grid, gd, gh, gw, min_xyz[0],
                     min_xyz[1], min_xyz[2], (float)out_sh[2], (float)out_sh[1], (float)out_sh[0], voxel, V, vol_len, C, d_rows);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_vertex_scatter(const float* d_out, const ViewCam* cams, const int* view_idx, int n_views, const float* verts, int Nv, int V,
                        float vol_len, int S, int persp, float* d_feats, hipStream_t s) {
  const int lds = S * S * 16 * (int)sizeof(float);
  if (lds > 160 * 1024) return mvd_fail("vertex scatter: feature map too large for the LDS accumulation");
  static bool attr_done[MVD_MAX_DEVICES] = {false};
  bool& attr_set = attr_done[mvd_current_device()];
  if (!attr_set) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)vertex_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL(vertex_scatter_kernel, dim3(n_views, 16), dim3(1024), lds, s, d_out, cams, view_idx, verts, Nv, V, vol_len, S, persp,
                     d_feats);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
// ---- deterministic mode (gather forms: every output element is written, nothing is accumulated into) ----
// pos: scratch of TN * D * S * S * 3 floats
int cbwd_frustum_gather_adj(const float* d_out, const ViewCam* cams, const int* view_idx, int TN, int D, int S, int V, float vol_len,
                            int persp, float* pos, float* d_vol, hipStream_t s) {
  const long npts = (long)TN * D * S * S, threads = (long)V * V * V * 16;
  hipLaunchKernelGGL(frustum_positions_kernel, dim3((int)((npts + 255) / 256)), dim3(256), 0, s, cams, view_idx, TN, D, S, V, vol_len,
                     persp, pos);
  hipLaunchKernelGGL(frustum_gather_adj_kernel, dim3((int)((threads + 255) / 256)), dim3(256), 0, s, d_out, cams, view_idx, pos, TN, D, S, V,
                     vol_len, persp, d_vol);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_latent_gather_adj(const float* d_vol, const int* grid, int gd, int gh, int gw, const float* min_xyz, const int* out_sh, float voxel,
                           int V, float vol_len, float* d_rows, hipStream_t s) {
  const long threads = (long)gd * gh * gw * 64;
  hipLaunchKernelGGL(latent_gather_adj_kernel, dim3((int)((threads + 255) / 256)), dim3(256), 0, s, d_vol, grid, gd, gh, gw, min_xyz[0],
                     min_xyz[1], min_xyz[2], (float)out_sh[2], (float)out_sh[1], (float)out_sh[0], voxel, V, vol_len, d_rows);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
// Adjoint of the bilinear sampling of a lattice's voxels in every view's map (vertex gather stage B; unproject_views_kernel):
// d_lat [n_views][n_max][16] holds dL/d(sample) of voxel vox_list[j] (vox_list NULL: the dense lattice, n_max = V^3) for the
// first *n_ptr (NULL: n_max) entries j, in ascending voxel order; d_feats [n_views][S*S][16] is written.
// rec: scratch of n_views * n_max float4.
// Only the compact form (vox_list / n_ptr given) has a caller and tests today; the dense form is written for the backward of
// use_spatial_volume=True and has not run yet.
int cbwd_lattice_to_views_adj(const float* d_lat, const ViewCam* cams, const int* view_idx, int n_views, const int* vox_list,
                              const int* n_ptr, int n_max, int V, float vol_len, int S, int persp, float4* rec, float* d_feats,
                              hipStream_t s) {
  if (n_views <= 0 || n_max <= 0) return mvd_fail("lattice adjoint: bad shape");
  hipLaunchKernelGGL(lattice_project_kernel, dim3(cdiv(n_max, 256), n_views), dim3(256), 0, s, cams, view_idx, vox_list, n_ptr, n_max, V,
                     vol_len, S, persp, rec);
  hipLaunchKernelGGL(lattice_to_views_adj_kernel, dim3(cdiv(S * S, 64), n_views), dim3(256), 0, s, d_lat, rec, n_ptr, n_max, S, d_feats);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
namespace {
struct VertexAdjScratch {  // the pieces of cbwd_vertex_gather_adj's scratch, each 256-byte aligned
  size_t key, cnt, off, rank, n_occ, occ, list_v, list_w, rec, lat, total;
  int cap;
  VertexAdjScratch(int n_views, int Nv, int V) {
    const size_t vox = (size_t)V * V * V, pairs = (size_t)Nv * 8;
    cap = (int)std::min(vox, pairs);
    size_t o = 0;
    auto take = [&](size_t bytes) {
      const size_t at = o;
      o += (bytes + 255) & ~(size_t)255;
      return at;
    };
    key = take((size_t)Nv * 4);
    cnt = take(vox * 4);
    off = take((vox + 1) * 4);
    rank = take(vox * 4);
    n_occ = take(4);
    occ = take((size_t)cap * 4);
    list_v = take(pairs * 4);
    list_w = take(pairs * 4);
    rec = take((size_t)n_views * cap * 16);
    lat = take((size_t)n_views * cap * 64);
    total = o;
  }
};
}  // namespace
size_t cbwd_vertex_adj_scratch_bytes(int n_views, int Nv, int V) { return VertexAdjScratch(n_views, Nv, V).total; }
// scratch: cbwd_vertex_adj_scratch_bytes(n_views, Nv, V) bytes, 256-byte aligned
int cbwd_vertex_gather_adj(const float* d_out, const ViewCam* cams, const int* view_idx, int n_views, const float* verts, int Nv, int V,
                           float vol_len, int S, int persp, void* scratch, float* d_feats, hipStream_t s) {
  if (Nv <= 0 || V <= 0 || V + 2 > VKEY_MASK || (long)V * V * V > (1l << 30)) return mvd_fail("vertex adjoint: bad lattice size");
  const VertexAdjScratch L(n_views, Nv, V);
  char* b = (char*)scratch;
  int *key = (int*)(b + L.key), *cnt = (int*)(b + L.cnt), *off = (int*)(b + L.off), *rank = (int*)(b + L.rank),
      *n_occ = (int*)(b + L.n_occ), *occ = (int*)(b + L.occ), *list_v = (int*)(b + L.list_v);
  float *list_w = (float*)(b + L.list_w), *lat = (float*)(b + L.lat);
  const int vox = V * V * V;
  hipLaunchKernelGGL(vertex_key_kernel, dim3(cdiv(Nv, 256)), dim3(256), 0, s, verts, Nv, V, vol_len, key);
  hipLaunchKernelGGL(vertex_bins_kernel<false>, dim3(cdiv(vox, 256)), dim3(256), 0, s, key, verts, Nv, V, vol_len, cnt, (const int*)nullptr,
                     (const int*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(vertex_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, vox, off, rank, n_occ);
  hipLaunchKernelGGL(vertex_bins_kernel<true>, dim3(cdiv(vox, 256)), dim3(256), 0, s, key, verts, Nv, V, vol_len, (int*)nullptr, off, rank,
                     list_v, list_w, occ);
  hipLaunchKernelGGL(vertex_to_lattice_adj_kernel, dim3(cdiv(L.cap * 16, 256), n_views), dim3(256), 0, s, d_out, off, occ, n_occ, list_v,
                     list_w, Nv, L.cap, lat);
  HIP_CHECK_RET(hipGetLastError());
  return cbwd_lattice_to_views_adj(lat, cams, view_idx, n_views, occ, n_occ, L.cap, V, vol_len, S, persp, (float4*)(b + L.rec), d_feats, s);
}
// flag: scratch of n ints
int cbwd_sparse_fold_dups_det(float* d, const int* nbr, int n, int C, int* flag, hipStream_t s) {
  if (n <= 0) return 0;
  HIP_CHECK_RET(hipMemsetAsync(flag, 0, (size_t)n * sizeof(int), s));
  hipLaunchKernelGGL(fold_dups_flag_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, nbr, n, flag);
  hipLaunchKernelGGL(fold_dups_sum_kernel, dim3(gridn((size_t)n * C)), dim3(256), 0, s, d, nbr, flag, n, C);
  hipLaunchKernelGGL(fold_dups_clear_kernel, dim3(gridn((size_t)n * C)), dim3(256), 0, s, d, nbr, n, C);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
// part: scratch of cbwd_fuse_scratch_floats(Nv) floats (only read when dw / db are given)
int cbwd_fuse(const float* d_fused, const float* vf, const float* w, int n_views, int Nv, int total_views, float* d_vf, float* dw, float* db,
              float* part, hipStream_t s) {
  hipLaunchKernelGGL(fuse_bwd_dvf_kernel, dim3(cdiv(Nv * 16, 256)), dim3(256), 0, s, d_fused, w, n_views, Nv, total_views, d_vf);
  if (dw && db) {
    if (!part) return mvd_fail("fuse backward: scratch for the weight-gradient partials missing");
    const int nchunk = cdiv(Nv, FW_CH);
    hipLaunchKernelGGL(fuse_bwd_w_kernel, dim3(nchunk), dim3(256), 0, s, d_fused, vf, n_views, Nv, total_views, part);
    hipLaunchKernelGGL(fuse_bwd_w_reduce_kernel, dim3(1), dim3(256), 0, s, part, nchunk, dw, db);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_fuse_scratch_floats(int Nv) { return cdiv(Nv, FW_CH) * 272; }
int cbwd_bn_scratch_floats(int n, int C) { return cdiv(n, BNB_CH) * 2 * C; }
// stats: [mean | rstd] from launch_bn_rows_relu; scratch: cbwd_bn_scratch_floats(n, C) floats
int cbwd_bn_rows_relu(const float* xraw, float* dy, int n, int C, const float* gamma, const float* beta, const float* stats,
                      float* scratch, float* dgamma, float* dbeta, hipStream_t s) {
  if (n <= 0 || C <= 0) return 0;
  if (C > 256 || 256 % C) return mvd_fail("bn_rows_relu backward: the channel count must divide 256");
  const int nchunk = cdiv(n, BNB_CH);
  hipLaunchKernelGGL(bn_rows_bwd_sums_kernel, dim3(nchunk), dim3(256), 0, s, xraw, dy, n, C, gamma, beta, stats, scratch);
  hipLaunchKernelGGL(bn_rows_bwd_apply_kernel, dim3(nchunk), dim3(256), 0, s, xraw, dy, n, C, gamma, beta, stats, scratch, nchunk, dgamma, dbeta);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_sparse_wgrad_chunks(int n_out) { return cdiv(n_out, SP_CHUNK); }
// dw_part: scratch of cbwd_sparse_wgrad_chunks(n_out) * 27 * Cin * Cout floats
int cbwd_sparse_conv(const float* in, const int* nbr, const float* d_out, int n_out, int Cin, int Cout, const float* w, float* d_in,
                     float* dw_packed, float* dw_part, hipStream_t s) {
  if (n_out <= 0) return 0;
  if (Cin > 256 || Cout > 256) return mvd_fail("sparse conv backward: channel count > 256");
  if (d_in) hipLaunchKernelGGL(sparse_conv_dgrad_kernel, dim3(n_out), dim3(256), 0, s, d_out, nbr, Cin, Cout, w, d_in);
  if (dw_packed) {
    const int nchunk = cdiv(n_out, SP_CHUNK);
    const long n = (long)27 * Cin * Cout;
    hipLaunchKernelGGL(sparse_conv_wgrad_kernel, dim3(27, cdiv(Cin * Cout, 256), nchunk), dim3(256), 0, s, in, nbr, d_out, n_out, Cin, Cout,
                       dw_part);
    hipLaunchKernelGGL(sparse_wgrad_reduce_kernel, dim3(gridn((size_t)n)), dim3(256), 0, s, dw_part, nchunk, n, dw_packed);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
// Matrix-core form (channel counts sparse_mfma_takes): weight gradient only; the data gradient is launch_sparse_conv on the
// layer's transposed fragments (SparseLayerW::wd) -- no atomics, no zero fill.
int cbwd_sparse_wgrad_mfma(const float* in, const int* nbr, const float* d_out, int n_out, int Cin, int Cout, float* dw_packed,
                           float* dw_part, hipStream_t s) {
  if (n_out <= 0) return 0;
  const int nchunk = cdiv(n_out, SP_CHUNK);
  const long n = (long)27 * Cin * Cout;
  const dim3 grid(7, nchunk), blk(256);
#define MVD_SPW(CI, CO)                                                                                                    \
  if (Cin == CI && Cout == CO)                                                                                             \
    hipLaunchKernelGGL((sparse_wgrad_mfma_kernel<CI, CO>), grid, blk, 0, s, in, nbr, d_out, n_out, dw_part);               \
  else
  MVD_SPW(16, 16) MVD_SPW(16, 32) MVD_SPW(32, 32) MVD_SPW(32, 64) MVD_SPW(64, 64)
  return mvd_fail("sparse wgrad: no matrix-core kernel for these channel counts");
#undef MVD_SPW
  hipLaunchKernelGGL(sparse_wgrad_reduce_kernel, dim3(gridn((size_t)n)), dim3(256), 0, s, dw_part, nchunk, n, dw_packed);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_sparse_inverse_table(const int* nbr_down, int n_out, int n_in, int* inv, hipStream_t s) {
  HIP_CHECK_RET(hipMemsetAsync(inv, 0xFF, (size_t)n_in * 27 * sizeof(int), s));
  if (n_out > 0) hipLaunchKernelGGL(sparse_inverse_table_kernel, dim3(gridn((size_t)n_out * 27)), dim3(256), 0, s, nbr_down, n_out, inv);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_sparse_fold_dups(float* d, const int* nbr, int n, int C, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(sparse_fold_dups_kernel, dim3(gridn((size_t)n * C)), dim3(256), 0, s, d, nbr, n, C);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_sparse_w_unpack_add(const float* pk, int Cin, int Cout, int layout, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(sparse_w_unpack_add_kernel, dim3(gridn((size_t)27 * Cin * Cout)), dim3(256), 0, s, pk, Cin, Cout, layout, dst);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
// The backward of ONE sparse conv layer behind its BatchNorm backward, as the conditioner's backward runs it per layer and as the
// parity hook mvd_op_sparse_conv_bwd runs it on the caller's buffers: d_out [n_out][Cout] (level 0 of the matrix-core form: folded in
// place) -> d_in [n_in][Cin] written, the weight gradient added to gw in the parameter's own `layout`.
// wd != null: matrix-core form (k_cond.hip / here): gather-form data gradient through the layer's own table with the tap flipped
// (submanifold) or through the inverse table (strided) -- no atomics, no zero fill.  At level 0 (lvl0_subm) the gradients of
// duplicate vertices' rows are folded into their representatives' first (the table is symmetric over those only), with atomics or,
// det, in row order.  wd == null: site form on w ([27][Cin][Cout]): zero fill, scatter-form data gradient with fp32 atomics.
SparseLayerScratch cbwd_sparse_layer_scratch(int n_in, int n_out, int Cin, int Cout, bool strided, bool lvl0_subm, bool det, bool mfma) {
  SparseLayerScratch z;
  z.dwp = (size_t)27 * Cin * Cout;
  z.dw_part = (size_t)cbwd_sparse_wgrad_chunks(n_out) * 27 * Cin * Cout;
  z.flag = mfma && lvl0_subm && det ? (size_t)n_out : 0;
  z.inv = mfma && strided ? (size_t)n_in * 27 : 0;
  return z;
}
int cbwd_sparse_layer(const float* in, const int* nbr, float* d_out, int n_in, int n_out, int Cin, int Cout, bool strided, bool lvl0_subm,
                      bool det, const float* w, const float* wd, int layout, float* dwp, float* dw_part, int* flag, int* inv, float* d_in,
                      float* gw, hipStream_t s) {
  int rc = 0;
  if (wd) {
    if (lvl0_subm && !det) rc = cbwd_sparse_fold_dups(d_out, nbr, n_out, Cout, s);
    if (lvl0_subm && det) rc = cbwd_sparse_fold_dups_det(d_out, nbr, n_out, Cout, flag, s);  // the same fold, rows added in row order
    if (!rc) rc = cbwd_sparse_wgrad_mfma(in, nbr, d_out, n_out, Cin, Cout, dwp, dw_part, s);
    const int* table = nbr;
    if (!rc && strided) {
      rc = cbwd_sparse_inverse_table(nbr, n_out, n_in, inv, s);
      table = inv;
    }
    if (!rc) rc = launch_sparse_conv(d_out, table, n_in, Cout, Cin, nullptr, wd, nullptr, nullptr, d_in, s, lvl0_subm ? 1 : 0);
  } else {
    if (det) return mvd_fail("deterministic mode: this sparse layer has no matrix-core form (its site-form data gradient adds with "
                             "fp32 atomics); unset MVD_SPARSE_VALU");
    HIP_CHECK_RET(hipMemsetAsync(d_in, 0, (size_t)n_in * Cin * sizeof(float), s));
    rc = cbwd_sparse_conv(in, nbr, d_out, n_out, Cin, Cout, w, d_in, dwp, dw_part, s);
  }
  return rc ? rc : cbwd_sparse_w_unpack_add(dwp, Cin, Cout, layout, gw, s);
}
int cbwd_im2colT3d(const void* src, int src_f32, long ld, int B, int D, int H, int W, int C, int stride, half_t* dst, int Rp, hipStream_t s) {
  const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (Rp < B * Do * Ho * Wo) return mvd_fail("im2colT3d: bad shape");
  dim3 grid(cdiv(Rp, 64), cdiv(C, 64), 27);
  if (!mvd_env().stage_scalar && !(C & 3) && !(ld & 3) && !(Rp & 63) && !((uintptr_t)src & 15) && !((uintptr_t)dst & 15)) {
    if (src_f32) hipLaunchKernelGGL(im2colT3d_vec_kernel<float>, grid, dim3(256), 0, s, (const float*)src, ld, B, D, H, W, C, stride, Do, Ho, Wo, dst, Rp);
    else hipLaunchKernelGGL(im2colT3d_vec_kernel<half_t>, grid, dim3(256), 0, s, (const half_t*)src, ld, B, D, H, W, C, stride, Do, Ho, Wo, dst, Rp);
    HIP_CHECK_RET(hipGetLastError());
    return 0;
  }
  if (src_f32) hipLaunchKernelGGL(im2colT3d_kernel<float>, grid, dim3(256), 0, s, (const float*)src, ld, B, D, H, W, C, stride, Do, Ho, Wo, dst, Rp);
  else hipLaunchKernelGGL(im2colT3d_kernel<half_t>, grid, dim3(256), 0, s, (const half_t*)src, ld, B, D, H, W, C, stride, Do, Ho, Wo, dst, Rp);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int cbwd_small_linear_bwd(const float* g, long ldg, int rows, int N, const half_t* w, int K, float* out, long ldo, int accum, hipStream_t s) {
  hipLaunchKernelGGL(small_linear_bwd_kernel, dim3(cdiv(K, 16), rows), dim3(256), 0, s, g, ldg, N, w, K, out, ldo, accum);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
