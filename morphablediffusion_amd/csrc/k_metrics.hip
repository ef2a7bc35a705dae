// 2-D image metrics of generated views against captured views -- include/mvd.h: mvd_op_image_metrics.
// Both images are 8-bit: a float image is quantised q = trunc(((clamp(x, -1, 1) + 1) * 0.5) * 255) in fp32 (batch.views_to_uint8's
// bytes), a uint8 image is taken as it is; where a pixel is background the PREDICTED pixel becomes 255 in all three channels.
//     ssim  per channel, 7 x 7 uniform window, sample (co)variances: with the window sums X = sum x, Y = sum y, XX, YY, XY (integers)
//           S = (2 X Y / 49^2 + C1)(2 (49 XY - X Y) / (49 48) + C2) / (((X^2 + Y^2) / 49^2 + C1)((49 XX - X^2 + 49 YY - Y^2) / (49 48) + C2))
//           averaged over the centres whose window lies inside the image (rows 3..H-4, columns 3..W-4) and over the channels.
//           Every integer above stays below 2^31 (49^2 255^2 = 156 125 025); only the rational function S is evaluated, in fp64.
//     sse, sae, background pixels, non-finite values: exact integers, carried in doubles below 2^53.
// Two launches, no atomics, every order of summation a function of (V, H, W) alone:
//   1. metrics_tile_kernel   grid (tiles, V), tiles = ceil((W - 6) / 32) * ceil((H - 6) / 32), x fastest: a workgroup owns a tile of
//                            32 x 32 window centres.  It loads the 38 x 38 pixels under them (3-pixel halo) of both images, quantised
//                            and whitened, as bytes into LDS; thread t sums S over the centres (t % 32, t / 32 + 8 j), j = 0..3, channel by
//                            channel, a 49-tap loop from LDS each.  sse / sae / the counts are taken while loading, over the pixels
//                            the workgroup OWNS: the pixels under its centres, widened to the image's edge in the first and last
//                            tile of each axis -- every pixel has one owner.  Five trees over the 256 threads, five double partials.
//   2. metrics_final_kernel  one workgroup per view: thread t adds the partials of tiles t, t + 256, ... in that order, then a tree;
//                            thread 0 writes ssim = sum S / (3 centres), sse, sae and the counts (NaN where the view had a non-finite).
// LDS: rows of 40 bytes.  A ds_read_u8 is served per 32-lane half; a half reads 32 consecutive bytes of one row -- at most 9 dwords
// on 9 different banks, lanes on the same dword broadcast -- so the tap reads are conflict-free at any pitch
// (tools/lds_bank_model.py: metrics_tap_read_cycles).
#include "common.h"

namespace {

constexpr int MET_T = 256, MET_TILE = 32, MET_HALO = MET_TILE + 6, MET_PITCH = 40, MET_NOUT = 5;
constexpr double MET_C1 = (0.01 * 255.0) * (0.01 * 255.0), MET_C2 = (0.03 * 255.0) * (0.03 * 255.0);

// sum of v over the workgroup's MET_T threads, valid in thread 0; s_red is reusable after the call
__device__ inline double met_block_sum(double v, double* s_red) {
  const int t = threadIdx.x;
  __syncthreads();
  s_red[t] = v;
  __syncthreads();
  for (int o = MET_T / 2; o > 0; o >>= 1) {
    if (t < o) s_red[t] += s_red[t + o];
    __syncthreads();
  }
  return s_red[0];
}

// the 8-bit value of element (v, c, y, x); a float that is NaN or infinite adds one to nonfinite when count is set
__device__ inline int met_load(const void* __restrict__ base, int dtype, int layout, int H, int W, int v, int c, int y, int x, bool count,
                               int& nonfinite) {
  const size_t i = layout == 0 ? (((size_t)v * 3 + c) * H + y) * W + x : (((size_t)v * H + y) * W + x) * 3 + c;
  if (dtype == 1) return (int)((const unsigned char*)base)[i];
  const float f = ((const float*)base)[i];
  if (count && !(fabsf(f) <= 3.402823466e+38f)) ++nonfinite;
  const float cl = fminf(fmaxf(f, -1.0f), 1.0f);  // a NaN becomes -1: its view reports NaN anyway
  return (int)(((cl + 1.0f) * 0.5f) * 255.0f);
}

__global__ __launch_bounds__(MET_T) void metrics_tile_kernel(const void* __restrict__ pred, int pd, int pl, const void* __restrict__ target,
                                                             int td, int tl, const unsigned char* __restrict__ mask, int mode, int H, int W,
                                                             int nx, int ny, double* __restrict__ part) {
  __shared__ unsigned char sP[3][MET_HALO][MET_PITCH], sT[3][MET_HALO][MET_PITCH];
  __shared__ double s_red[MET_T];
  const int t = threadIdx.x, v = blockIdx.y;
  const int tx = blockIdx.x % nx, ty = blockIdx.x / nx;
  const int x0 = tx * MET_TILE, y0 = ty * MET_TILE;  // first centre of the tile = first pixel of its halo
  // owned pixels: [x0 + 3, x0 + 35) x [y0 + 3, y0 + 35), widened to the image's edge in the first / last tile of an axis
  const int ox0 = tx == 0 ? 0 : x0 + 3, ox1 = tx == nx - 1 ? W : x0 + MET_TILE + 3;
  const int oy0 = ty == 0 ? 0 : y0 + 3, oy1 = ty == ny - 1 ? H : y0 + MET_TILE + 3;
  long long sse = 0, sae = 0;
  int nbg = 0, nonfinite = 0;
  for (int i = t; i < MET_HALO * MET_HALO; i += MET_T) {
    const int ly = i / MET_HALO, lx = i % MET_HALO, gy = y0 + ly, gx = x0 + lx;
    int p[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    if (gy < H && gx < W) {
      const bool own = gx >= ox0 && gx < ox1 && gy >= oy0 && gy < oy1;
      for (int c = 0; c < 3; ++c) {
        p[c] = met_load(pred, pd, pl, H, W, v, c, gy, gx, own, nonfinite);
        q[c] = met_load(target, td, tl, H, W, v, c, gy, gx, own, nonfinite);
      }
      bool bg = false;
      if (mode == 1) bg = mask[((size_t)v * H + gy) * W + gx] != 0;
      else if (mode == 2) bg = q[0] >= 254 && q[1] >= 254 && q[2] >= 254;
      if (bg) p[0] = p[1] = p[2] = 255;
      if (own) {
        for (int c = 0; c < 3; ++c) {
          const int d = p[c] - q[c];
          sse += d * d;
          sae += d < 0 ? -d : d;
        }
        nbg += bg ? 1 : 0;
      }
    }
    for (int c = 0; c < 3; ++c) {
      sP[c][ly][lx] = (unsigned char)p[c];
      sT[c][ly][lx] = (unsigned char)q[c];
    }
  }
  __syncthreads();
  const int ncx = W - 6, ncy = H - 6, cx = t % MET_TILE;
  double ssum = 0.0;
  if (x0 + cx < ncx) {
    for (int j = 0; j < MET_TILE / (MET_T / MET_TILE); ++j) {
      const int cy = t / MET_TILE + j * (MET_T / MET_TILE);
      if (y0 + cy >= ncy) break;
      for (int c = 0; c < 3; ++c) {
        int X = 0, Y = 0, XX = 0, YY = 0, XY = 0;
        for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
          for (int dx = 0; dx < 7; ++dx) {
            const int a = sP[c][cy + dy][cx + dx], b = sT[c][cy + dy][cx + dx];
            X += a;
            Y += b;
            XX += a * a;
            YY += b * b;
            XY += a * b;
          }
        }
        const double a1 = (double)(2 * X * Y) / 2401.0 + MET_C1;
        const double a2 = (double)(2 * (49 * XY - X * Y)) / 2352.0 + MET_C2;
        const double b1 = (double)(X * X + Y * Y) / 2401.0 + MET_C1;
        const double b2 = (double)((49 * XX - X * X) + (49 * YY - Y * Y)) / 2352.0 + MET_C2;
        ssum += (a1 * a2) / (b1 * b2);
      }
    }
  }
  const double vals[MET_NOUT] = {ssum, (double)sse, (double)sae, (double)nbg, (double)nonfinite};
  double* dst = part + ((size_t)v * nx * ny + blockIdx.x) * MET_NOUT;
  for (int k = 0; k < MET_NOUT; ++k) {
    const double r = met_block_sum(vals[k], s_red);
    if (t == 0) dst[k] = r;
  }
}

__global__ __launch_bounds__(MET_T) void metrics_final_kernel(const double* __restrict__ part, int ntiles, int H, int W,
                                                              double* __restrict__ out) {
  __shared__ double s_red[MET_T];
  const int t = threadIdx.x, v = blockIdx.x;
  const double* src = part + (size_t)v * ntiles * MET_NOUT;
  double r[MET_NOUT];
  for (int k = 0; k < MET_NOUT; ++k) {
    double acc = 0.0;
    for (int i = t; i < ntiles; i += MET_T) acc += src[(size_t)i * MET_NOUT + k];
    r[k] = met_block_sum(acc, s_red);
  }
  if (t == 0) {
    const bool bad = r[4] != 0.0;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    out[v * MET_NOUT + 0] = bad ? nan : r[0] / (3.0 * (double)(W - 6) * (double)(H - 6));
    out[v * MET_NOUT + 1] = bad ? nan : r[1];
    out[v * MET_NOUT + 2] = bad ? nan : r[2];
    out[v * MET_NOUT + 3] = bad ? nan : r[3];
    out[v * MET_NOUT + 4] = r[4];
  }
}

inline int met_tiles(int n) { return (n - 6 + MET_TILE - 1) / MET_TILE; }

}  // namespace

size_t image_metrics_scratch_bytes(int V, int H, int W) {
  return (size_t)V * met_tiles(W) * met_tiles(H) * MET_NOUT * sizeof(double);
}

int image_metrics_check(const char* who, const void* pred, int pred_dtype, int pred_layout, const void* target, int target_dtype,
                        int target_layout, const unsigned char* mask, int mask_mode, int V, int H, int W, const double* out) {
  const char* what = nullptr;
  if (!pred || !target || !out) what = ": null argument";
  else if (H < 7 || W < 7) what = ": H and W must be at least 7 (one 7 x 7 window)";
  else if (V < 1 || V > 65535) what = ": V must be in 1..65535";
  else if ((long long)V * H * W * 3 > 0x7fffffffLL) what = ": V H W 3 must be below 2^31";
  else if ((pred_dtype != 0 && pred_dtype != 1) || (target_dtype != 0 && target_dtype != 1)) what = ": dtype must be 0 (float32) or 1 (uint8)";
  else if ((pred_layout != 0 && pred_layout != 1) || (target_layout != 0 && target_layout != 1))
    what = ": layout must be 0 ([V,3,H,W]) or 1 ([V,H,W,3])";
  else if (mask_mode < 0 || mask_mode > 2) what = ": mask_mode must be 0 (none), 1 (explicit) or 2 (derived from the target)";
  else if (mask_mode == 1 && !mask) what = ": mask_mode 1 needs a mask";
  if (!what) return 0;
  return mvd_fail((std::string(who) + what).c_str());
}

// scratch: image_metrics_scratch_bytes(V, H, W) bytes, 8-byte aligned, alive until the launches have run
int launch_image_metrics(const void* pred, int pred_dtype, int pred_layout, const void* target, int target_dtype, int target_layout,
                         const unsigned char* mask, int mask_mode, int V, int H, int W, double* out, void* scratch, hipStream_t s) {
  const int nx = met_tiles(W), ny = met_tiles(H);
  double* part = (double*)scratch;
  hipLaunchKernelGGL(metrics_tile_kernel, dim3(nx * ny, V), dim3(MET_T), 0, s, pred, pred_dtype, pred_layout, target, target_dtype,
                     target_layout, mask, mask_mode, H, W, nx, ny, part);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(metrics_final_kernel, dim3(V), dim3(MET_T), 0, s, (const double*)part, nx * ny, H, W, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
