// The training objective with sample weights, a pixel weight and a robust (Huber) branch -- include/mvd.h: mvd_op_train_loss.
// pred / target channels-last [B][HW][C], m [B][HW] (null = 1), w [B] (null = 1), d = pred - target in fp32:
//     rho(d) = d^2                      rho'/2 = d                  l2, and huber for |d| <= delta
//     rho(d) = 2 delta |d| - delta^2    rho'/2 = delta sign(d)      huber, |d| > delta
//     a_b = sum_p m[b,p]      l_b = sum m rho / (C a_b)      mse_b = sum d^2 / (HW C)      L = (1/B) sum_b w_b l_b
//     dpred[b,p,c] = c_b m[b,p] rho'(d)/2,   c_b = ((2 loss_scale) w_b) / ((float)(B C) a_b);   a_b == 0: l_b = 0, dpred = 0
// Three launches, no atomics, every order of summation a function of (B, HW, C) alone:
//   1. loss_area_kernel   (only with m) one workgroup per sample: a_b in double, thread t sums pixels t, t + 256, ..., then a tree.
//   2. loss_fused_kernel  grid (nblk, B), nblk = min(ceil(HW / 256), 256): workgroup k of sample b owns the pixels
//                         k * 256 + t + j * nblk * 256 (thread t, j = 0, 1, ...), reads pred / target once, writes dpred and one pair of
//                         double partial sums (sum m rho, sum d^2) after a tree over its 256 threads.
//   3. loss_final_kernel  one workgroup: per sample a tree over the nblk partials, then l_b, mse_b; thread 0 adds w_b l_b over b in
//                         index order.
#include "common.h"

namespace {

constexpr int LOSS_T = 256, LOSS_MAX_BLK = 256;

// sum of v over the workgroup's LOSS_T threads, valid in thread 0; s_red is reusable after the call
__device__ inline double block_sum(double v, double* s_red) {
  const int t = threadIdx.x;
  __syncthreads();
  s_red[t] = v;
  __syncthreads();
  for (int o = LOSS_T / 2; o > 0; o >>= 1) {
    if (t < o) s_red[t] += s_red[t + o];
    __syncthreads();
  }
  return s_red[0];
}

__global__ __launch_bounds__(LOSS_T) void loss_area_kernel(const float* __restrict__ m, int HW, double* __restrict__ area) {
  __shared__ double s_red[LOSS_T];
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int p = threadIdx.x; p < HW; p += LOSS_T) acc += (double)m[(size_t)b * HW + p];
  const double a = block_sum(acc, s_red);
  if (threadIdx.x == 0) area[b] = a;
}

__global__ __launch_bounds__(LOSS_T) void loss_fused_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                            const float* __restrict__ w, const float* __restrict__ m,
                                                            const double* __restrict__ area, int B, int HW, int C, int huber,
                                                            float delta, float loss_scale, float* __restrict__ dpred,
                                                            double* __restrict__ part) {
  __shared__ double s_red[LOSS_T];
  const int b = blockIdx.y, nblk = gridDim.x;
  const float a_b = m ? (float)area[b] : (float)HW;
  const float c_b = a_b == 0.f ? 0.f : ((2.0f * loss_scale) * (w ? w[b] : 1.0f)) / ((float)(B * C) * a_b);
  double s_l = 0.0, s_d = 0.0;
  for (int p = blockIdx.x * LOSS_T + threadIdx.x; p < HW; p += nblk * LOSS_T) {
    const size_t row = (size_t)b * HW + p;
    const float mp = m ? m[row] : 1.0f;
    const float cm = c_b * mp;
    double r_l = 0.0, r_d = 0.0;
    for (int c = 0; c < C; ++c) {
      const float d = pred[row * C + c] - target[row * C + c];
      const double dd = (double)d * (double)d;
      double rho = dd;
      float g = d;
      if (huber && fabsf(d) > delta) {
        rho = 2.0 * (double)delta * (double)fabsf(d) - (double)delta * (double)delta;
        g = copysignf(delta, d);
      }
      r_l += rho;
      r_d += dd;
      if (dpred) dpred[row * C + c] = a_b == 0.f ? 0.f : cm * g;
    }
    s_l += (double)mp * r_l;
    s_d += r_d;
  }
  const double t_l = block_sum(s_l, s_red);
  const double t_d = block_sum(s_d, s_red);
  if (threadIdx.x == 0) {
    part[((size_t)b * nblk + blockIdx.x) * 2 + 0] = t_l;
    part[((size_t)b * nblk + blockIdx.x) * 2 + 1] = t_d;
  }
}

__global__ __launch_bounds__(LOSS_T) void loss_final_kernel(const double* __restrict__ part, const double* __restrict__ area,
                                                            const float* __restrict__ w, int has_m, int B, int HW, int C, int nblk,
                                                            float* __restrict__ loss_out, float* __restrict__ loss_ps,
                                                            float* __restrict__ mse_ps) {
  __shared__ double s_red[LOSS_T];
  const int t = threadIdx.x;
  double L = 0.0;  // thread 0 only
  for (int b = 0; b < B; ++b) {
    const double s_l = block_sum(t < nblk ? part[((size_t)b * nblk + t) * 2 + 0] : 0.0, s_red);
    const double s_d = block_sum(t < nblk ? part[((size_t)b * nblk + t) * 2 + 1] : 0.0, s_red);
    if (t == 0) {
      const double a = has_m ? area[b] : (double)HW;
      const double l = (float)a == 0.f ? 0.0 : s_l / ((double)C * a);  // the same test the fused pass makes for c_b
      if (loss_ps) loss_ps[b] = (float)l;
      if (mse_ps) mse_ps[b] = (float)(s_d / ((double)HW * (double)C));
      L += (double)(w ? w[b] : 1.0f) * l;
    }
  }
  if (t == 0 && loss_out) loss_out[0] = (float)(L / (double)B);
}

inline int loss_blocks(int HW) {
  const int n = (HW + LOSS_T - 1) / LOSS_T;
  return n > LOSS_MAX_BLK ? LOSS_MAX_BLK : n;
}

}  // namespace

size_t train_loss_scratch_bytes(int B, int HW) { return ((size_t)B + (size_t)B * loss_blocks(HW) * 2) * sizeof(double); }

int train_loss_check(const char* who, int B, int HW, int C, int loss_type, float huber_delta) {
  const char* what = nullptr;
  if (B <= 0 || B > 65535 || HW <= 0 || C <= 0 || (long)B * HW * C > 0x7fffffffL) what = ": B, HW, C must be positive, B <= 65535, B HW C < 2^31";
  else if (loss_type != 0 && loss_type != 1) what = ": loss_type must be 0 (l2) or 1 (huber)";
  else if (loss_type == 1 && !(huber_delta > 0.f)) what = ": huber_delta must be > 0";  // (a NaN fails too)
  if (!what) return 0;
  return mvd_fail((std::string(who) + what).c_str());
}

// scratch: train_loss_scratch_bytes(B, HW) bytes, 8-byte aligned, alive until the launches have run
int launch_train_loss(const float* pred, const float* target, int B, int HW, int C, const float* w, const float* m, int loss_type,
                      float huber_delta, float loss_scale, float* dpred, float* loss_out, float* loss_ps, float* mse_ps, void* scratch,
                      hipStream_t s) {
  double* area = (double*)scratch;
  double* part = area + B;
  const int nblk = loss_blocks(HW);
  if (m) {
    hipLaunchKernelGGL(loss_area_kernel, dim3(B), dim3(LOSS_T), 0, s, m, HW, area);
    HIP_CHECK_RET(hipGetLastError());
  }
  hipLaunchKernelGGL(loss_fused_kernel, dim3(nblk, B), dim3(LOSS_T), 0, s, pred, target, w, m, area, B, HW, C, loss_type == 1 ? 1 : 0,
                     huber_delta, loss_scale, dpred, part);
  HIP_CHECK_RET(hipGetLastError());
  if (loss_out || loss_ps || mse_ps) {
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(LOSS_T), 0, s, part, area, w, m ? 1 : 0, B, HW, C, nblk, loss_out, loss_ps,
                       mse_ps);
    HIP_CHECK_RET(hipGetLastError());
  }
  return 0;
}
