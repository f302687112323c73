// Fused QKV split + RoPE (K7b): one pass from the packed projection output
// qkv [s, b, ng, (rep+2)*d] (per query group: rep q heads | k | v) to
// contiguous q [s, b, ng*rep, d], k [s, b, ng, d], v [s, b, ng, d] with the
// rotate-half RoPE applied to q and k; the backward runs the same pass the
// other way round with the inverse rotation and writes the packed gradient.
//
// A head is d/8 16-byte vectors, the first 2*half8 of them rotated.  Each head
// gets P = d/8 - half8 lanes (blockDim.x): lane j < half8 owns vectors j and
// j + half8 (elements i..i+7 and their partners at +half), the other lanes own
// one vector of the passthrough tail.  A v head uses the same lanes as plain
// copies.  blockDim.y heads share a block; heads are grid-strided.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "rope_math.h"

__device__ __forceinline__ short bf16_bits(float f) { return __builtin_bit_cast(short, f2bf(f)); }

template <bool BWD>
__global__ void qkv_split_rope_kernel(short8* __restrict__ packed, short8* __restrict__ q,
                                      short8* __restrict__ k, short8* __restrict__ v,
                                      const float* __restrict__ cost, const float* __restrict__ sint,
                                      int heads /* s*b*ng*(rep+2) */, int rep, int bng /* b*ng */,
                                      int d8, int half8) {
  const int j = threadIdx.x;
  const int per_group = rep + 2;
  for (int r = blockIdx.x * blockDim.y + threadIdx.y; r < heads; r += gridDim.x * blockDim.y) {
    int tg = r / per_group;        // (s, b, group)
    int hh = r - tg * per_group;   // head inside the group: q heads, then k, then v
    short8* prow = packed + (long)r * d8;
    short8* srow = hh < rep    ? q + ((long)tg * rep + hh) * d8
                   : hh == rep ? k + (long)tg * d8
                               : v + (long)tg * d8;
    const short8* src = BWD ? srow : prow;
    short8* dst = BWD ? prow : srow;
    if (j >= half8) {
      dst[j + half8] = src[j + half8];
      continue;
    }
    short8 a = src[j], b = src[j + half8];
    if (hh <= rep) {
      long t = ((long)(tg / bng) * half8 + j) * 2;  // in float4v units
      const float4v* c4 = (const float4v*)cost + t;
      const float4v* s4 = (const float4v*)sint + t;
      float4v c0 = c4[0], c1 = c4[1], s0 = s4[0], s1 = s4[1];
      short8 oa, ob;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float cv = e < 4 ? c0[e & 3] : c1[e & 3];
        float sv = e < 4 ? s0[e & 3] : s1[e & 3];
        float o1, o2;
        rope_rotate<BWD>(sbf2f(a[e]), sbf2f(b[e]), cv, sv, o1, o2);
        oa[e] = bf16_bits(o1);
        ob[e] = bf16_bits(o2);
      }
      a = oa;
      b = ob;
    }
    dst[j] = a;
    dst[j + half8] = b;
  }
}

static void qkv_rope_launch(bool bwd, torch::Tensor packed, torch::Tensor q, torch::Tensor k,
                            torch::Tensor v, torch::Tensor cost, torch::Tensor sint, int rep) {
  long s = packed.size(0), b = packed.size(1), ng = packed.size(2);
  int d = packed.size(3) / (rep + 2);
  int half = cost.size(1);
  TORCH_CHECK(cost.is_cuda() && sint.is_cuda() && cost.dtype() == torch::kFloat32 &&
              sint.dtype() == torch::kFloat32 && cost.is_contiguous() && sint.is_contiguous() &&
              cost.dim() == 2 && sint.sizes() == cost.sizes());
  TORCH_CHECK(cost.size(0) >= s, "rope table is shorter than the sequence");
  TORCH_CHECK(d % 8 == 0 && half % 8 == 0 && 2 * half <= d,
              "qkv_split_rope needs d and d_rot/2 to be multiples of 8");
  long heads = s * b * ng * (rep + 2);
  TORCH_CHECK(heads < (1L << 31), "qkv_split_rope: too many heads for 32-bit indexing");
  if (heads == 0) return;
  int d8 = d / 8, half8 = half / 8;
  int px = d8 - half8;            // lanes per head
  TORCH_CHECK(px <= 256);
  int py = 256 / px;              // heads per block
  int grid = (int)std::min<long>((heads + py - 1) / py, 4096);
  auto stream = at::cuda::getCurrentHIPStream();
  auto kern = bwd ? qkv_split_rope_kernel<true> : qkv_split_rope_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(px, py), 0, stream,
                     (short8*)packed.data_ptr(), (short8*)q.data_ptr(), (short8*)k.data_ptr(),
                     (short8*)v.data_ptr(), cost.data_ptr<float>(), sint.data_ptr<float>(),
                     (int)heads, rep, (int)(b * ng), d8, half8);
}

std::vector<torch::Tensor> qkv_split_rope_fwd(torch::Tensor qkv, torch::Tensor cost,
                                              torch::Tensor sint, long rep) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dtype() == torch::kBFloat16 && qkv.dim() == 4);
  TORCH_CHECK(rep >= 1 && qkv.size(3) % (rep + 2) == 0);
  auto pc = qkv.contiguous();
  long s = pc.size(0), b = pc.size(1), ng = pc.size(2), d = pc.size(3) / (rep + 2);
  auto q = torch::empty({s, b, ng * rep, d}, pc.options());
  auto k = torch::empty({s, b, ng, d}, pc.options());
  auto v = torch::empty({s, b, ng, d}, pc.options());
  qkv_rope_launch(false, pc, q, k, v, cost, sint, (int)rep);
  return {q, k, v};
}

torch::Tensor qkv_split_rope_bwd(torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                                 torch::Tensor cost, torch::Tensor sint) {
  TORCH_CHECK(dq.is_cuda() && dk.is_cuda() && dv.is_cuda());
  TORCH_CHECK(dq.dtype() == torch::kBFloat16 && dk.dtype() == torch::kBFloat16 &&
              dv.dtype() == torch::kBFloat16);
  TORCH_CHECK(dq.dim() == 4 && dk.dim() == 4 && dv.sizes() == dk.sizes());
  long s = dk.size(0), b = dk.size(1), ng = dk.size(2), d = dk.size(3);
  TORCH_CHECK(ng > 0 && dq.size(0) == s && dq.size(1) == b && dq.size(3) == d && dq.size(2) % ng == 0 &&
              dq.size(2) >= ng);
  long rep = dq.size(2) / ng;
  auto dqc = dq.contiguous(), dkc = dk.contiguous(), dvc = dv.contiguous();
  auto dqkv = torch::empty({s, b, ng, (rep + 2) * d}, dqc.options());
  qkv_rope_launch(true, dqkv, dqc, dkc, dvc, cost, sint, (int)rep);
  return dqkv;
}
