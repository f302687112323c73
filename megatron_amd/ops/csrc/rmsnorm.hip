// RMSNorm forward + backward (K3 in SURVEY.md §2.3).
// bf16 activations, bf16 weight, fp32 accumulation. One workgroup per row
// (fwd); grid-strided rows with LDS-accumulated dw (bwd).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

// Every multiply-add below names its roundings (mul_rn, add_rn, fma_rn)
// instead of leaving the fusing to the compiler's contraction, which depends
// on the loop around the expression.  The kernels here come in variants that
// must agree to the bit (with and without the residual add, row in registers
// or read twice), and the choices are the ones these kernels have always
// computed: row sums add a rounded product; dx fuses the dy term and rounds
// the x term; dw fuses the accumulation.
__device__ __forceinline__ float sumsq_acc(float acc, float f) { return add_rn(acc, mul_rn(f, f)); }
__device__ __forceinline__ float dywx_acc(float acc, float dy, float w, float x) {
  return add_rn(acc, mul_rn(mul_rn(dy, w), x));
}

// ---------------------------------------------------------------------------
// forward: out[r, :] = x[r, :] * rsqrt(mean(x^2) + eps) * w ; saves rstd[r]
// ---------------------------------------------------------------------------

template <int BLOCK>
__global__ void rmsnorm_fwd_kernel(
    const short8* __restrict__ x, const short8* __restrict__ w,
    short8* __restrict__ out, float* __restrict__ rstd,
    int rows, int h8 /* hidden/8 */, float eps) {
  __shared__ float lds[BLOCK / WAVE];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const short8* xr = x + (long)row * h8;
    short8* or_ = out + (long)row * h8;
    float sumsq = 0.f;
    for (int i = threadIdx.x; i < h8; i += BLOCK) {
      short8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = sbf2f(v[j]);
        sumsq = sumsq_acc(sumsq, f);
      }
    }
    float total = block_reduce_sum<BLOCK>(sumsq, lds);
    float rs = rsqrtf(total / (float)(h8 * 8) + eps);
    if (threadIdx.x == 0) rstd[row] = rs;
    for (int i = threadIdx.x; i < h8; i += BLOCK) {
      short8 v = xr[i];
      short8 wv = w[i];
      short8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2sbf(sbf2f(v[j]) * rs * sbf2f(wv[j]));
      or_[i] = o;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// backward:
//   dx = rstd * dy*w - x * rstd^3 / H * sum(dy*w*x)
//   dw = sum_rows dy * (x * rstd)
// Each block owns a row range; dw accumulated in LDS fp32, then written as
// that block's row of a [n_blocks, H] partial buffer which the host wrapper
// sums in a fixed order (float atomics would make dw depend on block
// scheduling from run to run).
//
// Rows of up to ROW_VECS * BLOCK vectors (h <= 8192) are loaded once: dy, x
// and w stay in registers across the row reduction (w across all rows).
// Longer rows read dy, x and w a second time.  Both bodies add in the same
// order, so they give the same bits.
//
// dres (optional): a gradient that reaches the norm's input by another path
// (the residual branch).  dx_out = bf16(bf16(dx) + dres), the two roundings of
// a separate bf16 add.
// ---------------------------------------------------------------------------

constexpr int ROW_VECS = 4;

// one vector of dx and of the dw accumulation; shared by both bodies
__device__ __forceinline__ short8 rmsnorm_bwd_vec(short8 dyv, short8 xv, short8 wv, float rs, float k,
                                                  float* __restrict__ dw_acc8,
                                                  const short8* __restrict__ dres) {
  short8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float dyf = sbf2f(dyv[j]), xf = sbf2f(xv[j]), wf = sbf2f(wv[j]);
    o[j] = f2sbf(fma_rn(mul_rn(rs, dyf), wf, -mul_rn(xf, k)));
    dw_acc8[j] = fma_rn(mul_rn(dyf, xf), rs, dw_acc8[j]);
  }
  if (dres) {
    short8 r = *dres;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2sbf(sbf2f(o[j]) + sbf2f(r[j]));
  }
  return o;
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) rmsnorm_bwd_kernel(
    const short8* __restrict__ dy, const short8* __restrict__ x,
    const short8* __restrict__ w, const float* __restrict__ rstd,
    const short8* __restrict__ dres /* may be null */,
    short8* __restrict__ dx, float* __restrict__ dw_part,
    int rows, int h8) {
  extern __shared__ float smem[];           // [h8*8] fp32 dw accum
  __shared__ float lds[BLOCK / WAVE];
  float* dw_acc = smem;
  const int H = h8 * 8;
  for (int i = threadIdx.x; i < H; i += BLOCK) dw_acc[i] = 0.f;
  __syncthreads();

  if (h8 <= ROW_VECS * BLOCK) {
    short8 wv[ROW_VECS];
#pragma unroll
    for (int u = 0; u < ROW_VECS; ++u) {
      int i = threadIdx.x + u * BLOCK;
      if (i < h8) wv[u] = w[i];
    }
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
      const short8* dyr = dy + (long)row * h8;
      const short8* xr = x + (long)row * h8;
      const short8* drr = dres ? dres + (long)row * h8 : nullptr;
      short8* dxr = dx + (long)row * h8;
      short8 dyv[ROW_VECS], xv[ROW_VECS];
#pragma unroll
      for (int u = 0; u < ROW_VECS; ++u) {
        int i = threadIdx.x + u * BLOCK;
        if (i < h8) {
          dyv[u] = dyr[i];
          xv[u] = xr[i];
        }
      }
      float rs = rstd[row];
      float c = 0.f;
#pragma unroll
      for (int u = 0; u < ROW_VECS; ++u) {
        if (threadIdx.x + u * BLOCK < h8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) c = dywx_acc(c, sbf2f(dyv[u][j]), sbf2f(wv[u][j]), sbf2f(xv[u][j]));
        }
      }
      c = block_reduce_sum<BLOCK>(c, lds);
      float k = rs * rs * rs * c / (float)H;
#pragma unroll
      for (int u = 0; u < ROW_VECS; ++u) {
        int i = threadIdx.x + u * BLOCK;
        if (i < h8)
          dxr[i] = rmsnorm_bwd_vec(dyv[u], xv[u], wv[u], rs, k, dw_acc + i * 8, drr ? drr + i : nullptr);
      }
      __syncthreads();
    }
  } else {
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
      const short8* dyr = dy + (long)row * h8;
      const short8* xr = x + (long)row * h8;
      const short8* drr = dres ? dres + (long)row * h8 : nullptr;
      short8* dxr = dx + (long)row * h8;
      float rs = rstd[row];
      // pass 1: c = sum(dy*w*x)
      float c = 0.f;
      for (int i = threadIdx.x; i < h8; i += BLOCK) {
        short8 dyv = dyr[i], xv = xr[i], wv = w[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) c = dywx_acc(c, sbf2f(dyv[j]), sbf2f(wv[j]), sbf2f(xv[j]));
      }
      c = block_reduce_sum<BLOCK>(c, lds);
      float k = rs * rs * rs * c / (float)H;
      for (int i = threadIdx.x; i < h8; i += BLOCK)
        dxr[i] = rmsnorm_bwd_vec(dyr[i], xr[i], w[i], rs, k, dw_acc + i * 8, drr ? drr + i : nullptr);
      __syncthreads();
    }
  }
  float* dw_row = dw_part + (long)blockIdx.x * H;
  for (int i = threadIdx.x; i < H; i += BLOCK) dw_row[i] = dw_acc[i];
}

// ---------------------------------------------------------------------------
// residual add + forward: sum = bf16(x + residual), then the forward above on
// the rounded sum (same expressions, same reduction order), in one pass.
// Rows of up to ROW_VECS * BLOCK vectors keep the sum in registers; longer
// rows read back what the same thread wrote to `sum`.
// ---------------------------------------------------------------------------

__device__ __forceinline__ short8 add_bf16x8(short8 a, short8 b) {
  short8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2sbf(sbf2f(a[j]) + sbf2f(b[j]));
  return o;
}

template <int BLOCK>
__global__ void add_rmsnorm_fwd_kernel(
    const short8* __restrict__ x, const short8* __restrict__ res, const short8* __restrict__ w,
    short8* sum, short8* __restrict__ out, float* __restrict__ rstd,
    int rows, int h8, float eps) {
  __shared__ float lds[BLOCK / WAVE];
  const bool in_regs = h8 <= ROW_VECS * BLOCK;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const short8* xr = x + (long)row * h8;
    const short8* rr = res + (long)row * h8;
    short8* sr = sum + (long)row * h8;
    short8* or_ = out + (long)row * h8;
    short8 sv[ROW_VECS];
    float sumsq = 0.f;
    if (in_regs) {
#pragma unroll
      for (int u = 0; u < ROW_VECS; ++u) {
        int i = threadIdx.x + u * BLOCK;
        if (i < h8) {
          sv[u] = add_bf16x8(xr[i], rr[i]);
          sr[i] = sv[u];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float f = sbf2f(sv[u][j]);
            sumsq = sumsq_acc(sumsq, f);
          }
        }
      }
    } else {
      for (int i = threadIdx.x; i < h8; i += BLOCK) {
        short8 v = add_bf16x8(xr[i], rr[i]);
        sr[i] = v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = sbf2f(v[j]);
          sumsq = sumsq_acc(sumsq, f);
        }
      }
    }
    float total = block_reduce_sum<BLOCK>(sumsq, lds);
    float rs = rsqrtf(total / (float)(h8 * 8) + eps);
    if (threadIdx.x == 0) rstd[row] = rs;
    if (in_regs) {
#pragma unroll
      for (int u = 0; u < ROW_VECS; ++u) {
        int i = threadIdx.x + u * BLOCK;
        if (i < h8) {
          short8 wv = w[i];
          short8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = f2sbf(sbf2f(sv[u][j]) * rs * sbf2f(wv[j]));
          or_[i] = o;
        }
      }
    } else {
      for (int i = threadIdx.x; i < h8; i += BLOCK) {
        short8 v = sr[i];  // this thread's own store
        short8 wv = w[i];
        short8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2sbf(sbf2f(v[j]) * rs * sbf2f(wv[j]));
        or_[i] = o;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 2);
  TORCH_CHECK(w.dtype() == torch::kBFloat16);
  TORCH_CHECK(x.size(1) % 8 == 0, "hidden must be a multiple of 8");
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  auto out = torch::empty_like(xc);
  auto rstd = torch::empty({x.size(0)}, x.options().dtype(torch::kFloat32));
  int rows = x.size(0), h8 = x.size(1) / 8;
  constexpr int BLOCK = 256;
  int grid = std::min(rows, 2048);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((rmsnorm_fwd_kernel<BLOCK>), dim3(grid), dim3(BLOCK), 0, stream,
                     (const short8*)xc.data_ptr(), (const short8*)wc.data_ptr(),
                     (short8*)out.data_ptr(), rstd.data_ptr<float>(), rows, h8, (float)eps);
  return {out, rstd};
}

std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor x, torch::Tensor residual, torch::Tensor w,
                                           double eps) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 2);
  TORCH_CHECK(residual.is_cuda() && residual.dtype() == torch::kBFloat16 && residual.sizes() == x.sizes());
  TORCH_CHECK(w.is_cuda() && w.dtype() == torch::kBFloat16 && w.numel() == x.size(1));
  TORCH_CHECK(x.size(1) % 8 == 0, "hidden must be a multiple of 8");
  auto xc = x.contiguous();
  auto rc = residual.contiguous();
  auto wc = w.contiguous();
  auto sum = torch::empty_like(xc);
  auto out = torch::empty_like(xc);
  auto rstd = torch::empty({x.size(0)}, x.options().dtype(torch::kFloat32));
  int rows = x.size(0), h8 = x.size(1) / 8;
  if (rows == 0) return {sum, out, rstd};
  constexpr int BLOCK = 256;
  int grid = std::min(rows, 2048);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((add_rmsnorm_fwd_kernel<BLOCK>), dim3(grid), dim3(BLOCK), 0, stream,
                     (const short8*)xc.data_ptr(), (const short8*)rc.data_ptr(),
                     (const short8*)wc.data_ptr(), (short8*)sum.data_ptr(), (short8*)out.data_ptr(),
                     rstd.data_ptr<float>(), rows, h8, (float)eps);
  return {sum, out, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w, torch::Tensor rstd,
                                       c10::optional<torch::Tensor> dres) {
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  int rows = x.size(0), h8 = x.size(1) / 8;
  auto dx = torch::empty_like(xc);
  torch::Tensor drc;
  if (dres.has_value()) {
    TORCH_CHECK(dres->is_cuda() && dres->dtype() == torch::kBFloat16 && dres->sizes() == x.sizes());
    drc = dres->contiguous();
  }
  constexpr int BLOCK = 256;
  int grid = std::min(rows, 512);
  auto dw_part = torch::empty({grid, x.size(1)}, x.options().dtype(torch::kFloat32));
  size_t smem = (size_t)h8 * 8 * sizeof(float);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<BLOCK>), dim3(grid), dim3(BLOCK), smem, stream,
                     (const short8*)dyc.data_ptr(), (const short8*)xc.data_ptr(),
                     (const short8*)wc.data_ptr(), rstd.data_ptr<float>(),
                     drc.defined() ? (const short8*)drc.data_ptr() : (const short8*)nullptr,
                     (short8*)dx.data_ptr(), dw_part.data_ptr<float>(), rows, h8);
  return {dx, dw_part.sum(0).to(torch::kBFloat16)};
}
