// MXFP8 NT GEMM on CDNA4: C[M, N] bf16 = dequant(A[M, K]) . dequant(B[N, K])^T
// with e4m3 elements, one e8m0 scale byte per 32 elements along K ([R, K/32]
// uint8, byte = E + 127) and fp32 accumulation in
// v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 0).
//
// Operand layout of the instruction, as measured on the MI355X with
// per-block scales against an fp8 identity: lane l = 16 g + c supplies row c
// of its operand; its first four VGPRs hold k = 16 g .. 16 g + 15 of the
// 128-wide slab and its last four k = 64 + 16 g .. + 15, and the scale byte
// it supplies (byte of the scale VGPR chosen by opsel) applies to the
// 32 consecutive k values 32 g .. 32 g + 31, held by the lanes 2 (g & 1) and
// 2 (g & 1) + 1.  So a lane reads the 16-byte chunks g and 4 + g of its row
// and the scale of MX block g of the slab.
//
// One 512-thread block computes a 256 x 256 output tile; wave (wp, wq) of the
// 2 x 4 waves owns 128 output columns x 64 output rows as 8 x 4 MFMA tiles
// (128 accumulator registers).  B (indexed by the output column) is the MFMA
// A operand and A (indexed by the output row) the MFMA B operand, so the four
// accumulator elements of a lane are consecutive along the output row, and
// with the row permutation tile_row_a a sub-tile pair gives a lane 8
// consecutive columns: 16-byte stores.
//
// The reduction runs in 128-wide slabs (128 bytes per row) through two LDS
// stages per operand (4 x 32 KB): global loads of slab s+1 into registers
// before the MFMAs of slab s, swizzled LDS writes after them, one barrier per
// slab.  The tile is [256][128 B], 16-byte chunk c of row r stored at chunk
// c ^ swzf<64>(r) - the swizzle of the bf16 [.][64] tiles, same row pitch.
// Bank group (16 B) of a chunk = 8 (r & 1) + position.
//   writes: 16 lanes = rows r, r+1 x 8 chunks: a permutation of the 8
//     positions per row, two parities: 16 distinct bank groups;
//   fragment reads (two b128 per lane, chunks g and 4 + g): the 16 lanes of a
//     read pass share g and read the rows base + 8 (c >> 2) + (c & 3), whose
//     parity is c & 1 and whose swizzle term runs over all 8 values for the 8
//     rows of one parity: 16 distinct bank groups.
// Scales do not go through LDS: each lane loads the byte of its own row and
// block (s[row][4 slab + g]) straight from global memory one slab ahead, the
// bytes of four sub-tiles are packed into one VGPR and picked by opsel.
// Rows at or past M / N are staged as zeros with scale byte 127 and never
// stored.  No atomics, no split-K: the same inputs give the same bits.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <utility>
#include "attention_tile.h"
#include "gemm_block_order.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef unsigned char u8;

constexpr int MX_T = 256;    // output tile edge
constexpr int MX_SLAB = 128; // reduction elements (= bytes per row) of a slab

// Reg-staged copy of one [256 rows][128 B] slab into swizzled LDS by a
// 512-thread block; rows at or past rows_valid are read as zero.  `base` is
// uniform and the lane's part of the address a 32-bit offset (255 K + 128 <
// 2^32), so the loads address with a scalar base and one VGPR.
struct MxStager {
  int4 reg[4];
  __device__ __forceinline__ void loads(const u8* base, unsigned stride, int rows_valid) {
    const int r = (int)threadIdx.x >> 3, ch = (int)threadIdx.x & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      reg[i] = make_int4(0, 0, 0, 0);
      if (r + i * 64 < rows_valid)
        reg[i] = *reinterpret_cast<const int4*>(base + ((unsigned)(r + i * 64) * stride + (unsigned)ch * 16u));
    }
  }
  __device__ __forceinline__ void writes(char* tile) const {
    const int r = (int)threadIdx.x >> 3, ch = (int)threadIdx.x & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<int4*>(tile + (r + i * 64) * MX_SLAB + (swz<64>(r, ch) << 4)) = reg[i];
  }
};

// 2 x 16 fp8 of one lane: the chunks at byte offsets lo and hi of `row_base`
__device__ __forceinline__ v8i mx_frag(const char* row_base, int lo, int hi) {
  const int4 a = *reinterpret_cast<const int4*>(row_base + lo);
  const int4 b = *reinterpret_cast<const int4*>(row_base + hi);
  return v8i{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// sub-tile row PS of the wave: one B fragment against the four A fragments
template <int PS>
__device__ __forceinline__ void mx_ps(f32x4 (&acc)[8][4], const char* ptile, int lo, int hi, const v8i (&qf)[4],
                                      const int (&psc)[2], int qsc) {
  const v8i pf = mx_frag(ptile + (32 * (PS >> 1) + 4 * (PS & 1)) * MX_SLAB, lo, hi);
  acc[PS][0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pf, qf[0], acc[PS][0], 0, 0, PS & 3, psc[PS >> 2], 0, qsc);
  acc[PS][1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pf, qf[1], acc[PS][1], 0, 0, PS & 3, psc[PS >> 2], 1, qsc);
  acc[PS][2] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pf, qf[2], acc[PS][2], 0, 0, PS & 3, psc[PS >> 2], 2, qsc);
  acc[PS][3] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pf, qf[3], acc[PS][3], 0, 0, PS & 3, psc[PS >> 2], 3, qsc);
}
template <int... PS>
__device__ __forceinline__ void mx_slab(std::integer_sequence<int, PS...>, f32x4 (&acc)[8][4], const char* ptile,
                                        int lo, int hi, const v8i (&qf)[4], const int (&psc)[2], int qsc) {
  (mx_ps<PS>(acc, ptile, lo, hi, qf, psc, qsc), ...);
}

struct MxArgs {
  const u8 *a, *as, *b, *bs;  // A [M, K], its scales [M, K/32], B [N, K], its scales [N, K/32]
  bf16* out;                  // [M, N]
  int M, N, K;
  int T, nct;                 // row tiles and column tiles of the grid
};

__global__ __launch_bounds__(512) void mx_gemm_nt_kernel(MxArgs a) {
  int rt, ct;
  if (!gg_block(blockIdx.x, a.T, a.nct, rt, ct)) return;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int wp = wid & 1, wq = wid >> 1;
  const int row0 = rt * MX_T, col0 = ct * MX_T;
  const int prows = a.N - col0, qrows = a.M - row0;  // valid rows of the B and A tiles
  const int ns = a.K / MX_SLAB, kb = a.K / 32;
  // a wave whose outputs all lie past M or N only stages
  const bool wave_live = wq * 64 < qrows && wp * 128 < prows;

  __shared__ __align__(16) char lds[2][2][MX_T * MX_SLAB];

  const u8* pbase = a.b + (long)col0 * a.K;
  const u8* qbase = a.a + (long)row0 * a.K;

  // lane-constant part of a fragment's tile row (tile_row_a(n, c) minus its
  // sub-tile term), the two swizzled chunk offsets, and the scale addresses
  const int lrow = 8 * (c >> 2) + (c & 3);
  const int f = swzf<64>(lrow);
  const int lo = lrow * MX_SLAB + ((g ^ f) << 4), hi = lrow * MX_SLAB + (((4 + g) ^ f) << 4);
  const int prow = wp * 128 + lrow, qrow = wq * 64 + lrow;
  // scales: uniform base of the wave's rows plus a 32-bit lane offset
  const u8* ps_ptr = a.bs + (long)(col0 + wp * 128) * kb;
  const u8* qs_ptr = a.as + (long)(row0 + wq * 64) * kb;
  const unsigned sc_off = (unsigned)lrow * (unsigned)kb + (unsigned)g;

  f32x4 acc[8][4];
#pragma unroll
  for (int ps = 0; ps < 8; ++ps)
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) acc[ps][qs] = f32x4{0.f, 0.f, 0.f, 0.f};

  // scale bytes of slab s for the lane's 8 + 4 fragments, 127 past the edge
  int praw[8], qraw[4];
  auto scale_loads = [&](int s) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int d = 32 * (n >> 1) + 4 * (n & 1);
      praw[n] = (prow + d < prows) ? (int)(ps_ptr + ((long)d * kb + 4 * s))[sc_off] : 127;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int d = 32 * (n >> 1) + 4 * (n & 1);
      qraw[n] = (qrow + d < qrows) ? (int)(qs_ptr + ((long)d * kb + 4 * s))[sc_off] : 127;
    }
  };
  int psc[2], qsc;
  auto scale_pack = [&]() {
    psc[0] = praw[0] | (praw[1] << 8) | (praw[2] << 16) | (praw[3] << 24);
    psc[1] = praw[4] | (praw[5] << 8) | (praw[6] << 16) | (praw[7] << 24);
    qsc = qraw[0] | (qraw[1] << 8) | (qraw[2] << 16) | (qraw[3] << 24);
  };

  MxStager sp, sq;
  if (wave_live) scale_loads(0);
  sp.loads(pbase, a.K, prows);
  sq.loads(qbase, a.K, qrows);
  sp.writes(lds[0][0]);
  sq.writes(lds[0][1]);
  if (wave_live) scale_pack();
  __syncthreads();

  for (int s = 0; s < ns; ++s) {
    const int st = s & 1;
    if (s + 1 < ns) {
      if (wave_live) scale_loads(s + 1);
      sp.loads(pbase + (s + 1) * MX_SLAB, a.K, prows);
      sq.loads(qbase + (s + 1) * MX_SLAB, a.K, qrows);
    }
    if (wave_live) {
      v8i qf[4];
#pragma unroll
      for (int qs = 0; qs < 4; ++qs)
        qf[qs] = mx_frag(lds[st][1] + (wq * 64 + 32 * (qs >> 1) + 4 * (qs & 1)) * MX_SLAB, lo, hi);
      mx_slab(std::make_integer_sequence<int, 8>{}, acc, lds[st][0] + wp * 128 * MX_SLAB, lo, hi, qf, psc, qsc);
    }
    if (s + 1 < ns) {
      sp.writes(lds[st ^ 1][0]);
      sq.writes(lds[st ^ 1][1]);
      if (wave_live) scale_pack();
    }
    __syncthreads();
  }
  if (!wave_live) return;

  // epilogue: lane (g, c) holds output row tile_row_a(qs, c) of each q
  // sub-tile and, over the sub-tile pair (2pq, 2pq+1), the 8 output columns
  // 32pq + 8g .. +7 (MFMA D layout: element r of acc is MFMA row 4g + r)
#pragma unroll
  for (int qs = 0; qs < 4; ++qs) {
    const int m = row0 + wq * 64 + tile_row_a(qs, c);
    if (m >= a.M) continue;
    bf16* o = a.out + (long)m * a.N;
#pragma unroll
    for (int pq = 0; pq < 4; ++pq) {
      const int col = col0 + wp * 128 + 32 * pq + 8 * g;
      if (col >= a.N) continue;
      const f32x4 l = acc[2 * pq][qs], h = acc[2 * pq + 1][qs];
      *reinterpret_cast<int4*>(o + col) = make_int4(pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3]),
                                                    pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3]));
    }
  }
}

void mx_check(const torch::Tensor& t, torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() && t.dim() == 2,
              "mx_gemm_nt: ", name, " must be a contiguous 2-D device tensor of its dtype");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "mx_gemm_nt: ", name, " must start at a 16-byte aligned address");
}

}  // namespace

// out [M, N] bf16 = dequant(aq [M, K], a_s [M, K/32]) . dequant(bq [N, K], b_s [N, K/32])^T
torch::Tensor mx_gemm_nt(torch::Tensor aq, torch::Tensor a_s, torch::Tensor bq, torch::Tensor b_s) {
  mx_check(aq, torch::kFloat8_e4m3fn, "aq");
  mx_check(bq, torch::kFloat8_e4m3fn, "bq");
  mx_check(a_s, torch::kUInt8, "a_s");
  mx_check(b_s, torch::kUInt8, "b_s");
  const long M = aq.size(0), K = aq.size(1), N = bq.size(0);
  TORCH_CHECK(bq.size(1) == K, "mx_gemm_nt: inner dimensions differ");
  TORCH_CHECK(K % MX_SLAB == 0 && K > 0 && N % 16 == 0 && N > 0 && M >= 1,
              "mx_gemm_nt: K must be a multiple of 128, N of 16, M >= 1");
  TORCH_CHECK(a_s.size(0) == M && a_s.size(1) == K / 32 && b_s.size(0) == N && b_s.size(1) == K / 32,
              "mx_gemm_nt: scales must be [rows, K / 32]");
  TORCH_CHECK(M < (1L << 31) - 2 * MX_T && N < (1L << 31) - 2 * MX_T && K < (1L << 24), "mx_gemm_nt: too large");
  auto out = torch::empty({M, N}, aq.options().dtype(torch::kBFloat16));
  MxArgs g;
  g.a = reinterpret_cast<const u8*>(aq.data_ptr()); g.as = a_s.data_ptr<u8>();
  g.b = reinterpret_cast<const u8*>(bq.data_ptr()); g.bs = b_s.data_ptr<u8>();
  g.out = reinterpret_cast<bf16*>(out.data_ptr());
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.T = (int)((M + MX_T - 1) / MX_T); g.nct = (int)((N + MX_T - 1) / MX_T);
  TORCH_CHECK((long)g.T * g.nct < (1L << 30), "mx_gemm_nt: grid too large");
  hipLaunchKernelGGL(mx_gemm_nt_kernel, dim3(gg_grid(g.T, g.nct)), dim3(512), 0, at::hip::getCurrentHIPStream(), g);
  return out;
}
