// Device-side augmentation over a device-resident uint8 dataset (survey K16).
// CIFAR style (mda_crop_flip_norm): gather the batch rows, RandomCrop(32, padding=4) with zero
// padding, RandomHorizontalFlip, ToTensor (/255) and Normalize, written as
// channels-last (NHWC) fp32 or bf16 -- the layout the conv kernels read.
// The whole CIFAR-100 train set is 150 MB of HBM; with this kernel the data
// pipeline never touches the host (the reference decodes PIL images in
// CPU workers, and its NUM_WORKERS //= world_size drops to 0 workers at
// world >= 3).  Tiny-ImageNet style (mda_rotate_flip_norm): the
// same with RandomRotation (nearest neighbour, fill 0) in place of the crop.
#include "common.h"

namespace {

template <typename TO>
__global__ void __launch_bounds__(256)
crop_flip_norm_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ idx,
                      const int32_t* __restrict__ offs, const uint8_t* __restrict__ flip,
                      const float* __restrict__ mean, const float* __restrict__ inv_std,
                      TO* __restrict__ out, int B, int H, int W, int C, int pad) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(p / (H * W));
    const int r = (int)(p - (int64_t)b * H * W);
    const int y = r / W, x = r - (r / W) * W;
    const int xs = flip[b] ? (W - 1 - x) : x;
    const int sy = y + offs[2 * b] - pad, sx = xs + offs[2 * b + 1] - pad;
    const bool ok = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
    const uint8_t* src = data + ((idx[b] * H + (ok ? sy : 0)) * W + (ok ? sx : 0)) * C;
    TO* dst = out + p * C;
    for (int c = 0; c < C; ++c) {
      float v = ok ? src[c] * (1.f / 255.f) : 0.f;
      io<TO>::st(dst, c, (v - mean[c]) * inv_std[c]);
    }
  }
}

// Source pixel of output (xs, y) under the 16.16 fixed-point affine map
// a[0..5] (sx = a0 (xs+1/2) + a1 (y+1/2) + a2, sy likewise with a3..a5),
// evaluated at half-pixel centres entirely in integers so the selection is
// exact and comparable with the torch reference: linear offset sy*W + sx, or
// -1 when the source falls outside the image.  64-bit intermediates: the
// coefficients are caller data, so no 32-bit range is assumed.
__device__ __forceinline__ int rot_src(const int32_t* __restrict__ a, int xs, int y, int H, int W) {
  const int64_t u = 2 * xs + 1, v = 2 * y + 1;
  const int64_t sx = (a[0] * u + a[1] * v + 2 * (int64_t)a[2]) >> 17;
  const int64_t sy = (a[3] * u + a[4] * v + 2 * (int64_t)a[5]) >> 17;
  const bool ok = (uint64_t)sx < (uint64_t)W && (uint64_t)sy < (uint64_t)H;
  return ok ? (int)(sy * W + sx) : -1;
}

template <typename TO>
__global__ void __launch_bounds__(256)
rotate_flip_norm_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ idx,
                        const int32_t* __restrict__ coef, const uint8_t* __restrict__ flip,
                        const float* __restrict__ mean, const float* __restrict__ inv_std,
                        TO* __restrict__ out, int B, int H, int W, int C) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(p / (H * W));
    const int r = (int)(p - (int64_t)b * H * W);
    const int y = r / W, x = r - (r / W) * W;
    const int xs = flip[b] ? (W - 1 - x) : x;
    const int s = rot_src(coef + 6 * b, xs, y, H, W);
    const bool ok = s >= 0;
    const uint8_t* src = data + (idx[b] * H * W + (ok ? s : 0)) * C;
    TO* dst = out + p * C;
    for (int c = 0; c < C; ++c) {
      float v = ok ? src[c] * (1.f / 255.f) : 0.f;
      io<TO>::st(dst, c, (v - mean[c]) * inv_std[c]);
    }
  }
}

struct alignas(4) u32x3 { uint32_t a, b, c; };

// bf16, C == 3, even W: one thread per pair of x-adjacent output pixels, so a
// lane owns 12 contiguous bytes (three packed bf16 pairs) and a wave writes
// 768 contiguous bytes, instead of 2-byte stores 6 bytes apart.
__global__ void __launch_bounds__(256)
rotate_flip_norm_bf16c3_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ idx,
                               const int32_t* __restrict__ coef, const uint8_t* __restrict__ flip,
                               const float* __restrict__ mean, const float* __restrict__ inv_std,
                               bf16_t* __restrict__ out, int B, int H, int W) {
  const int W2 = W >> 1;
  const int64_t total = (int64_t)B * H * W2;
  const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
  const float i0 = inv_std[0], i1 = inv_std[1], i2 = inv_std[2];
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(q / (H * W2));
    const int r = (int)(q - (int64_t)b * H * W2);
    const int y = r / W2, x = 2 * (r - (r / W2) * W2);
    const bool f = flip[b] != 0;
    const uint8_t* img = data + idx[b] * H * W * 3;
    float v[6];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int xs = f ? (W - 1 - (x + k)) : (x + k);
      const int s = rot_src(coef + 6 * b, xs, y, H, W);
      const bool ok = s >= 0;
      const uint8_t* src = img + (ok ? s : 0) * 3;
      v[3 * k + 0] = ((ok ? src[0] * (1.f / 255.f) : 0.f) - m0) * i0;
      v[3 * k + 1] = ((ok ? src[1] * (1.f / 255.f) : 0.f) - m1) * i1;
      v[3 * k + 2] = ((ok ? src[2] * (1.f / 255.f) : 0.f) - m2) * i2;
    }
    u32x3 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5])};
    *reinterpret_cast<u32x3*>(out + q * 6) = o;
  }
}

}  // namespace

// data [N, H, W, C] uint8; idx [B]; offs [B, 2] int32 in [0, 2*pad]; flip [B] uint8;
// out [B, H, W, C] (NHWC) fp32 (dt 0) or bf16 (dt 1).
MDA_API int mda_crop_flip_norm(const uint8_t* data, const int64_t* idx, const int32_t* offs,
                               const uint8_t* flip, const float* mean, const float* inv_std,
                               void* out, int64_t dt, int64_t B, int64_t H, int64_t W, int64_t C,
                               int64_t pad, hipStream_t st) {
  int64_t total = B * H * W;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  if (dt == DT_F32)
    hipLaunchKernelGGL(crop_flip_norm_kernel<float>, dim3(blocks), dim3(256), 0, st, data, idx,
                       offs, flip, mean, inv_std, (float*)out, (int)B, (int)H, (int)W, (int)C, (int)pad);
  else
    hipLaunchKernelGGL(crop_flip_norm_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, data, idx,
                       offs, flip, mean, inv_std, (bf16_t*)out, (int)B, (int)H, (int)W, (int)C, (int)pad);
  MDA_CHECK_LAUNCH();
}

// Tiny-ImageNet-style augmentation: RandomRotation (nearest neighbour, fill 0)
// then RandomHorizontalFlip of the rotated image, ToTensor and Normalize.
// data [N, H, W, C] uint8; idx [B]; coef [B, 6] int32, the 16.16 fixed-point
// output->source affine map (see rot_src); flip [B] uint8;
// out [B, H, W, C] (NHWC) fp32 (dt 0) or bf16 (dt 1).
MDA_API int mda_rotate_flip_norm(const uint8_t* data, const int64_t* idx, const int32_t* coef,
                                 const uint8_t* flip, const float* mean, const float* inv_std,
                                 void* out, int64_t dt, int64_t B, int64_t H, int64_t W, int64_t C,
                                 hipStream_t st) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || H * W > (1 << 24)) return (int)hipErrorInvalidValue;
  if (dt == DT_BF16 && C == 3 && (W & 1) == 0) {
    int64_t total = B * H * (W / 2);
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(rotate_flip_norm_bf16c3_kernel, dim3(blocks), dim3(256), 0, st, data, idx,
                       coef, flip, mean, inv_std, (bf16_t*)out, (int)B, (int)H, (int)W);
    MDA_CHECK_LAUNCH();
  }
  int64_t total = B * H * W;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  if (dt == DT_F32)
    hipLaunchKernelGGL(rotate_flip_norm_kernel<float>, dim3(blocks), dim3(256), 0, st, data, idx,
                       coef, flip, mean, inv_std, (float*)out, (int)B, (int)H, (int)W, (int)C);
  else
    hipLaunchKernelGGL(rotate_flip_norm_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, data, idx,
                       coef, flip, mean, inv_std, (bf16_t*)out, (int)B, (int)H, (int)W, (int)C);
  MDA_CHECK_LAUNCH();
}
