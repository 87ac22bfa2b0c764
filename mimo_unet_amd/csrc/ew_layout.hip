// Input / output layout conversion: NCHW images <-> NHWC padded-channel tensors, image gradients folded off the reflect-padded domain.
#include "ew_device.h"

namespace mimo {

// ---------------------------------------------------------------------------------------
// layout conversion
// ---------------------------------------------------------------------------------------
__global__ void pack_input_kernel(const float* __restrict__ x, int64_t stride_n, int64_t stride_s,
                                  const int64_t* __restrict__ perm, int s, int N, int C, int HW,
                                  float* __restrict__ out, int cp) {
  const int64_t total = (int64_t)N * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / HW);
    const int yx = (int)(i - (int64_t)n * HW);
    const int64_t src_n = perm ? perm[(int64_t)s * N + n] : n;
    const float* src = x + src_n * stride_n + (int64_t)s * stride_s + yx;
    float* dst = out + i * cp;
    for (int c = 0; c < cp; ++c) dst[c] = c < C ? src[(int64_t)c * HW] : 0.f;
  }
}

int pack_input_launch(const float* x, int64_t stride_n, int64_t stride_s, const int64_t* perm, int s, int N, int C,
                      int H, int W, float* out, int cp, hipStream_t st) {
  const int64_t total = (int64_t)N * H * W;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  hipLaunchKernelGGL(pack_input_kernel, dim3(blocks), dim3(256), 0, st, x, stride_n, stride_s, perm, s, N, C, H * W, out, cp);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

template <typename T>
__global__ void unpack_dx_kernel(const T* __restrict__ dxpad, int ldp, int N, int S, int s, int C, int H, int W,
                                 float* __restrict__ dx) {
  const int64_t total = (int64_t)N * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / (H * W));
    const int yx = (int)(i - (int64_t)n * H * W);
    const int y = yx / W, x = yx - y * W;
    for (int c0 = 0; c0 < C; c0 += 4) {
      const float4 v = fold_read(dxpad, ldp, n, y, x, H, W, c0);
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int j = 0; j < 4 && c0 + j < C; ++j) dx[(((int64_t)n * S + s) * C + c0 + j) * H * W + yx] = vv[j];
    }
  }
}

int unpack_dx_launch(const void* dxpad, int dt, int ldp, int N, int S, int s, int C, int H, int W, float* dx, hipStream_t st) {
  const int64_t total = (int64_t)N * H * W;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  MIMO_ST_DISPATCH(dt, T, hipLaunchKernelGGL(unpack_dx_kernel<T>, dim3(blocks), dim3(256), 0, st, (const T*)dxpad, ldp, N, S, s,
                                             C, H, W, dx));
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// One thread per pixel: one folded float4 read of the padded-domain gradient (the image has at most 4 padded channels per
// quad), C coalesced plane accesses of the NCHW image gradient.  ldp is a multiple of 4 (padded channels).
__global__ void fold_image_grad_kernel(const float* __restrict__ dxpad, int ldp, int N, int C, int H, int W,
                                       float* __restrict__ dimage, int accumulate) {
  const int64_t HW = (int64_t)H * W, total = (int64_t)N * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / HW);
    const int yx = (int)(i - (int64_t)n * HW);
    const int y = yx / W, x = yx - y * W;
    for (int c0 = 0; c0 < C; c0 += 4) {
      const float4 v = fold_read(dxpad, ldp, n, y, x, H, W, c0);
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int j = 0; j < 4 && c0 + j < C; ++j) {
        float* d = dimage + ((int64_t)n * C + c0 + j) * HW + yx;
        *d = accumulate ? *d + vv[j] : vv[j];
      }
    }
  }
}

int fold_image_grad_launch(const float* dxpad, int ldp, int N, int C, int H, int W, float* dimage, int accumulate, hipStream_t st) {
  const int64_t total = (int64_t)N * H * W;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  hipLaunchKernelGGL(fold_image_grad_kernel, dim3(blocks), dim3(256), 0, st, dxpad, ldp, N, C, H, W, dimage, accumulate);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

// The same fold for R Monte-Carlo passes stacked pass-major on the batch axis (pass m, image b at row m * B + b of dxpad):
// one thread per pixel of the B images, the R folded float4 reads (each coalesced along x like the one above) added in the
// fixed order m = 0 ... R-1 in fp32 registers, one store per channel.  Pass 0 assigns (or adds to the stored value), so R = 1
// gives the bits of fold_image_grad_kernel, -0 included.
__global__ void fold_image_grad_mc_kernel(const float* __restrict__ dxpad, int ldp, int B, int R, int C, int H, int W,
                                          float* __restrict__ dimage, int accumulate) {
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const int yx = (int)(i - (int64_t)b * HW);
    const int y = yx / W, x = yx - y * W;
    for (int c0 = 0; c0 < C; c0 += 4) {
      float4 s = fold_read(dxpad, ldp, b, y, x, H, W, c0);
      float* d = dimage + ((int64_t)b * C + c0) * HW + yx;
      if (accumulate) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < 4 && c0 + j < C; ++j) o[j] = d[j * HW];
        s = f4add(make_float4(o[0], o[1], o[2], o[3]), s);
      }
      for (int m = 1; m < R; ++m) s = f4add(s, fold_read(dxpad, ldp, m * B + b, y, x, H, W, c0));
      const float vv[4] = {s.x, s.y, s.z, s.w};
      for (int j = 0; j < 4 && c0 + j < C; ++j) d[j * HW] = vv[j];
    }
  }
}

int fold_image_grad_mc_launch(const float* dxpad, int ldp, int B, int R, int C, int H, int W, float* dimage, int accumulate,
                              hipStream_t st) {
  const int64_t total = (int64_t)B * H * W;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  hipLaunchKernelGGL(fold_image_grad_mc_kernel, dim3(blocks), dim3(256), 0, st, dxpad, ldp, B, R, C, H, W, dimage, accumulate);
  MIMO_KERNEL_CHECK();
  return MIMO_OK;
}

}  // namespace mimo
