// MXFP8 quantisation on CDNA4: bf16 [R, K] -> e4m3 elements and one e8m0
// scale byte (E + 127) per 32 elements along the contiguous dimension.
//
// Scale rule, amax = max|x| over the block: E is the smallest integer with
// amax * 2^-E <= 448.  With the fp32 bits of amax, exponent field ef and
// mantissa man, that is byte = ef - 8 when man <= 0x600000 (amax <= 1.75 *
// 2^(ef-127)) and ef - 7 otherwise, clamped at 0: integer arithmetic only.
// amax == 0 and fp32 subnormals have ef == 0 and give byte 0 (E = -127).
// Elements are x * 2^-E in fp32 (exact: a power of two with exponent field
// 254 - byte >= 6) rounded to e4m3 by the packed conversion; the rule keeps
// them within 448, so the conversion never saturates.
//
// mx_quant_row_kernel: the tensor is flat - K % 32 == 0 makes every aligned
// run of 32 elements one block of one row.  A lane loads 16 bytes (8
// elements), the 4 lanes of a block share the amax by two xor shuffles, each
// converts its 8 values and stores 8 bytes; lane 0 of the four stores the
// scale byte.  Input read once, nothing in between.
//
// mx_quant_dual_kernel (weights): a 256-thread block owns a 64 x 64 tile.
// Phase 1 is the rowwise quantisation from registers, and the same registers
// go into a swizzled bf16 LDS tile.  Phase 2 reads the tile by columns: lane
// (kq, jj) of a wave takes column 16w + 8it + kq, rows 8jj .. 8jj+7, the four
// lanes jj of a 32-row block share the amax, and the lane stores 8 bytes of
// qT [K, R] - eight lanes write 64 contiguous bytes.
// LDS tile: row pitch 128 B = 8 chunks of 16 B, chunk c of row r is stored at
// chunk c ^ ((r >> 3) & 7).  Bank group (16 B) of a chunk = 8 (r & 1) + pos.
//   writes (b128, 16 lanes = rows r, r+1 x 8 chunks): the 8 chunks of a row
//     are a permutation of the 8 positions, and the two rows differ in
//     parity: 16 distinct bank groups;
//   reads (u16, 64 lanes at one step i): rows 8jj + i have one parity and
//     (r >> 3) & 7 = jj, the 8 columns of the instruction lie in one chunk c,
//     so lane (kq, jj) reads dword 4 (c ^ jj) + (kq >> 1) of its half of the
//     banks: 32 distinct dwords, each read by the two lanes kq, kq ^ 1
//     (a broadcast), in 32 distinct banks.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

// e8m0 byte of a block from the fp32 bits of its amax (>= 0)
__device__ __forceinline__ int mx_scale_byte(float amax) {
  const unsigned u = __builtin_bit_cast(unsigned, amax);
  const int ef = (int)(u >> 23), man = (int)(u & 0x7fffffu);
  return max(ef - (man <= 0x600000 ? 8 : 7), 0);
}
// 2^-E as fp32
__device__ __forceinline__ float mx_inv_scale(int byte) {
  return __builtin_bit_cast(float, (unsigned)(254 - byte) << 23);
}
__device__ __forceinline__ float amax8(const short8& v) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(sbf2f(v[i])));
  return m;
}
// 8 bf16 times `inv` -> 8 e4m3 bytes
__device__ __forceinline__ int2 quant8(const short8& v, float inv) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(sbf2f(v[0]) * inv, sbf2f(v[1]) * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(sbf2f(v[2]) * inv, sbf2f(v[3]) * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(sbf2f(v[4]) * inv, sbf2f(v[5]) * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(sbf2f(v[6]) * inv, sbf2f(v[7]) * inv, hi, true);
  return make_int2(lo, hi);
}
// amax over the 4 consecutive lanes that share a block
__device__ __forceinline__ float quad_max(float m) {
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  return fmaxf(m, __shfl_xor(m, 2, 64));
}

constexpr int MXQ_UNR = 4;  // 16-byte chunks in flight per lane

__global__ __launch_bounds__(256) void mx_quant_row_kernel(const short8* __restrict__ x, int2* __restrict__ q,
                                                           unsigned char* __restrict__ s, long nchunk) {
  const long stride = (long)gridDim.x * 256;
  // nchunk % 4 == 0 and every index below is congruent to the lane number
  // mod 4, so the four lanes of a block are live together
  for (long base = (long)blockIdx.x * 256 + threadIdx.x; base < nchunk; base += stride * MXQ_UNR) {
    short8 v[MXQ_UNR];
#pragma unroll
    for (int u = 0; u < MXQ_UNR; ++u) {
      const long i = base + u * stride;
      v[u] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (i < nchunk) v[u] = x[i];
    }
#pragma unroll
    for (int u = 0; u < MXQ_UNR; ++u) {
      const long i = base + u * stride;
      const int byte = mx_scale_byte(quad_max(amax8(v[u])));
      if (i < nchunk) {
        q[i] = quant8(v[u], mx_inv_scale(byte));
        if ((i & 3) == 0) s[i >> 2] = (unsigned char)byte;
      }
    }
  }
}

__global__ __launch_bounds__(256) void mx_quant_dual_kernel(const bf16* __restrict__ x, unsigned char* __restrict__ q,
                                                            unsigned char* __restrict__ s,
                                                            unsigned char* __restrict__ qT,
                                                            unsigned char* __restrict__ sT, int R, int K) {
  __shared__ __align__(16) short tile[64][64];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * 64, k0 = blockIdx.x * 64;

  // phase 1: rows of the tile, 8 lanes per row; validity is uniform over the
  // 4 lanes of a block because R and K are multiples of 32
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int id = tid + it * 256, rr = id >> 3, ch = id & 7;
    const int row = r0 + rr, col = k0 + ch * 8;
    const bool live = row < R && col < K;
    short8 v = short8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live) v = *reinterpret_cast<const short8*>(x + (long)row * K + col);
    *reinterpret_cast<short8*>(&tile[rr][(ch ^ ((rr >> 3) & 7)) * 8]) = v;
    const int byte = mx_scale_byte(quad_max(amax8(v)));
    if (live) {
      *reinterpret_cast<int2*>(q + (long)row * K + col) = quant8(v, mx_inv_scale(byte));
      if ((ch & 3) == 0) s[(long)row * (K >> 5) + (col >> 5)] = (unsigned char)byte;
    }
  }
  __syncthreads();

  // phase 2: columns of the tile, 8 lanes (64 rows, two blocks) per column
  const int lane = tid & 63, w = tid >> 6, jj = lane & 7, kq = lane >> 3;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int kk = 16 * w + 8 * it + kq;
    const int pos = (((kk >> 3) ^ jj) << 3) | (kk & 7);
    short8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = tile[8 * jj + i][pos];
    const int byte = mx_scale_byte(quad_max(amax8(v)));
    const int row = r0 + 8 * jj, col = k0 + kk;
    if (row < R && col < K) {
      *reinterpret_cast<int2*>(qT + (long)col * R + row) = quant8(v, mx_inv_scale(byte));
      if ((jj & 3) == 0) sT[(long)col * (R >> 5) + (row >> 5)] = (unsigned char)byte;
    }
  }
}

}  // namespace

// t bf16 [R, K] -> {q [R, K] e4m3, s [R, K/32] u8}, and with dual also
// {qT [K, R], sT [K, R/32]}: the quantisation of t^T, blocks along R
std::vector<torch::Tensor> mx_quantize(torch::Tensor t, bool dual) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.is_contiguous() && t.dim() == 2,
              "mx_quantize: t must be a contiguous 2-D bf16 device tensor");
  const long R = t.size(0), K = t.size(1);
  TORCH_CHECK(K % 32 == 0 && K > 0, "mx_quantize: K must be a multiple of 32");
  TORCH_CHECK(!dual || (R % 32 == 0 && R > 0), "mx_quantize: dual needs R to be a multiple of 32");
  TORCH_CHECK(R < (1L << 31) && K < (1L << 31), "mx_quantize: dimension too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "mx_quantize: t must be 16-byte aligned");
  auto q = torch::empty({R, K}, t.options().dtype(torch::kFloat8_e4m3fn));
  auto s = torch::empty({R, K / 32}, t.options().dtype(torch::kUInt8));
  hipStream_t stream = at::hip::getCurrentHIPStream();
  if (!dual) {
    if (R == 0) return {q, s};
    const long nchunk = R * K / 8;
    const long blocks = (nchunk + 256L * MXQ_UNR - 1) / (256L * MXQ_UNR);
    hipLaunchKernelGGL(mx_quant_row_kernel, dim3((unsigned)std::min(blocks, 8192L)), dim3(256), 0, stream,
                       reinterpret_cast<const short8*>(t.data_ptr()), reinterpret_cast<int2*>(q.data_ptr()),
                       s.data_ptr<unsigned char>(), nchunk);
    return {q, s};
  }
  auto qT = torch::empty({K, R}, q.options());
  auto sT = torch::empty({K, R / 32}, s.options());
  TORCH_CHECK((R + 63) / 64 < 65536, "mx_quantize: too many rows for the dual grid");
  hipLaunchKernelGGL(mx_quant_dual_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)((R + 63) / 64)), dim3(256), 0,
                     stream, reinterpret_cast<const bf16*>(t.data_ptr()),
                     reinterpret_cast<unsigned char*>(q.data_ptr()), s.data_ptr<unsigned char>(),
                     reinterpret_cast<unsigned char*>(qT.data_ptr()), sT.data_ptr<unsigned char>(), (int)R, (int)K);
  return {q, s, qT, sT};
}
