// Grouped GEMM for MoE experts on CDNA4: bf16 operands, 16x16x32 MFMA, fp32
// accumulation, expert sizes read on the device only.
//
//   fwd   "NT"  Y[M, n]   rows of expert e = X_e[m_e, k] @ W[e][n, k]^T
//   dgrad "NN"  dX[M, k]  rows of expert e = dY_e[m_e, n] @ W[e][n, k]
//   wgrad "TN"  dW[e][n, k] (+)= dY_e^T @ X_e
//
// sizes [E] (int32 or int64, E <= 256) lives on the device.  Expert e owns the
// rows [min(off_e, M), min(off_{e+1}, M)) with off the prefix sums of
// max(sizes, 0); rows at or past the last offset are written as zeros in Y and
// dX and add nothing to dW.  gg_tile_map_kernel (one block) turns sizes into
// the clamped offsets and a row-tile map; every grid depends on shapes only,
// so a captured launch replays with new sizes.
//
// One 512-thread block computes a 256 x 256 output tile; wave (wp, wq) of the
// 2 x 4 waves owns 128 output columns x 64 output rows as 8 x 4 MFMA tiles
// (128 accumulator registers).  The operand indexed by the output COLUMN (P)
// is the MFMA A operand and the one indexed by the output ROW (Q) the B
// operand, so the four accumulator elements of a lane are consecutive along
// the output row.  The reduction runs in 64-wide slabs through two LDS stages
// per operand (128 KB): global loads of slab s+1 into registers before the
// MFMAs of slab s, swizzled LDS writes after them, one barrier per slab.
//   k-contiguous operand (X, W in NT; dY in NN): [256][64] tile, swz<64>,
//     read_a<64> on the rows tile_row_a(sub, lane) - a lane then holds 8
//     consecutive output columns over a sub-tile pair;
//   operand whose reduction index is its row (W in NN; X, dY in TN): the
//     [64][256] slab as two [64][128] tiles, swz<128>, read_b_tr<128>.
// No operand is ever stored transposed, nothing is atomic, wgrad has no
// split-K: the same inputs give the same bits.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "attention_tile.h"
#include "gemm_block_order.h"

namespace {

constexpr int GG_T = 256;      // output tile edge
constexpr int GG_MAXE = 256;   // local experts
constexpr int GG_NT = 0, GG_NN = 1, GG_TN = 2;

// ---------------------------------------------------------------------------
// sizes -> offs[0..E] (clamped prefix sums) and tiles[0..T): (expert, row0,
// row_end) of a live row tile, expert == E for a tile of the zero tail,
// expert == -1 for an unused slot.  sum_e ceil(m_e / 256) + ceil(tail / 256)
// <= floor(M / 256) + E + 1 = T.
// ---------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(256) void gg_tile_map_kernel(const I* __restrict__ sizes, int E, int M, int T,
                                                          int4* __restrict__ tiles, int* __restrict__ offs) {
  __shared__ int off_s[GG_MAXE + 1];
  __shared__ int ts_s[GG_MAXE + 2];
  const int tid = threadIdx.x;
  if (tid < E) {
    const long s = (long)sizes[tid];
    off_s[tid + 1] = (int)(s < 0 ? 0 : (s > M ? (long)M : s));
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0, t = 0;
    off_s[0] = 0;
    ts_s[0] = 0;
    for (int e = 0; e < E; ++e) {
      const int m = min(off_s[e + 1], M - o);
      o += m;
      off_s[e + 1] = o;
      t += (m + GG_T - 1) / GG_T;
      ts_s[e + 1] = t;
    }
    ts_s[E + 1] = t + (M - o + GG_T - 1) / GG_T;
  }
  __syncthreads();
  for (int e = tid; e <= E; e += 256) offs[e] = off_s[e];
  for (int t = tid; t < T; t += 256) {
    int4 v = make_int4(-1, 0, 0, 0);
    if (t < ts_s[E]) {
      int lo = 0, hi = E;  // largest e with ts_s[e] <= t
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ts_s[mid] <= t) lo = mid;
        else hi = mid;
      }
      v = make_int4(lo, off_s[lo] + (t - ts_s[lo]) * GG_T, off_s[lo + 1], 0);
    } else if (t < ts_s[E + 1]) {
      v = make_int4(E, off_s[E] + (t - ts_s[E]) * GG_T, M, 0);
    }
    tiles[t] = v;
  }
}

// Reg-staged copies of one reduction slab into swizzled LDS by a 512-thread
// block (the TileStager pattern: loads() early, writes() late).  Elements at
// or past rows_valid / cols_valid are read as zero.
struct KStager {  // [256 rows][64 reduction columns], k-contiguous
  short8 reg[4];
  __device__ __forceinline__ void loads(const bf16* base, long stride, int rows_valid, int) {
    const int r = (int)threadIdx.x >> 3, c8 = (int)threadIdx.x & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      reg[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r + i * 64 < rows_valid)
        reg[i] = *reinterpret_cast<const short8*>(base + (long)(r + i * 64) * stride + c8 * 8);
    }
  }
  __device__ __forceinline__ void writes(short* tile) const {
    const int r = (int)threadIdx.x >> 3, c8 = (int)threadIdx.x & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<short8*>(tile + (r + i * 64) * 64 + swz<64>(r + i * 64, c8) * 8) = reg[i];
  }
};
struct TStager {  // [64 reduction rows][256 columns] as two [64][128] tiles
  short8 reg[4];
  __device__ __forceinline__ void loads(const bf16* base, long stride, int rows_valid, int cols_valid) {
    const int r = (int)threadIdx.x >> 5, c32 = (int)threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      reg[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r + i * 16 < rows_valid && c32 * 8 < cols_valid)
        reg[i] = *reinterpret_cast<const short8*>(base + (long)(r + i * 16) * stride + c32 * 8);
    }
  }
  __device__ __forceinline__ void writes(short* tile) const {
    const int r = (int)threadIdx.x >> 5, c32 = (int)threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<short8*>(tile + (c32 >> 4) * (64 * 128) + (r + i * 16) * 128 +
                                 swz<128>(r + i * 16, c32 & 15) * 8) = reg[i];
  }
};

struct GGArgs {
  const bf16* q;  // operand indexed by the output row:    X (NT), dY (NN, TN)
  const bf16* p;  // operand indexed by the output column: W (NT, NN), X (TN)
  void* out;      // Y [M, n] (NT), dX [M, k] (NN), dW [E, n, k] (TN)
  const int4* tiles;
  const int* offs;
  int n, k, E;
  int T, nct;     // row tiles and column tiles of the grid
};

template <int MODE, bool OUT32>
__global__ __launch_bounds__(512) void gg_kernel(GGArgs a) {
  constexpr bool P_TR = MODE != GG_NT, Q_TR = MODE == GG_TN;
  using PStager = std::conditional_t<P_TR, TStager, KStager>;
  using QStager = std::conditional_t<Q_TR, TStager, KStager>;

  int rt, ct;
  if (!gg_block(blockIdx.x, a.T, a.nct, rt, ct)) return;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int wp = wid & 1, wq = wid >> 1;

  // rows [row0, row_end) of the token dimension: the output rows of this tile
  // (NT, NN) or the reduction range of this expert (TN)
  int expert, row0, row_end, qt = 0;
  if constexpr (MODE != GG_TN) {
    const int4 t = a.tiles[rt];
    expert = __builtin_amdgcn_readfirstlane(t.x);
    row0 = __builtin_amdgcn_readfirstlane(t.y);
    row_end = __builtin_amdgcn_readfirstlane(t.z);
    if (expert < 0) return;
  } else {
    const int nnt = (a.n + GG_T - 1) / GG_T;
    expert = rt / nnt;
    qt = rt % nnt;
    row0 = __builtin_amdgcn_readfirstlane(a.offs[expert]);
    row_end = __builtin_amdgcn_readfirstlane(a.offs[expert + 1]);
    if (OUT32 && row0 >= row_end) return;  // main_grad slice stays untouched
  }
  const int ocols = (MODE == GG_NT) ? a.n : a.k;  // row length of the output
  const int col0 = ct * GG_T;

  if constexpr (MODE != GG_TN) {
    if (expert == a.E) {  // tail past the last expert: zeros
      bf16* o = reinterpret_cast<bf16*>(a.out);
      for (int idx = tid; idx < GG_T * 32; idx += 512) {
        const int r = row0 + (idx >> 5), cc = col0 + (idx & 31) * 8;
        if (r < row_end && r < row0 + GG_T && cc < ocols)
          *reinterpret_cast<int4*>(o + (long)r * ocols + cc) = make_int4(0, 0, 0, 0);
      }
      return;
    }
  }

  __shared__ __align__(16) short lds[2][2][GG_T * 64];

  // slab s of each operand: base pointer, row stride, step per slab, bounds
  const bf16 *pbase, *qbase;
  long pstride, qstride, pstep, qstep;
  int ns, prows, pcols, qrows, qcols;
  if constexpr (MODE == GG_NT) {
    ns = a.k / 64;
    pbase = a.p + ((long)expert * a.n + col0) * a.k; pstride = a.k; pstep = 64;
    prows = a.n - col0; pcols = 64;
    qbase = a.q + (long)row0 * a.k; qstride = a.k; qstep = 64;
    qrows = row_end - row0; qcols = 64;
  } else if constexpr (MODE == GG_NN) {
    ns = a.n / 64;
    pbase = a.p + (long)expert * a.n * a.k + col0; pstride = a.k; pstep = 64L * a.k;
    prows = 64; pcols = a.k - col0;
    qbase = a.q + (long)row0 * a.n; qstride = a.n; qstep = 64;
    qrows = row_end - row0; qcols = 64;
  } else {
    ns = (row_end - row0 + 63) / 64;
    pbase = a.p + (long)row0 * a.k + col0; pstride = a.k; pstep = 64L * a.k;
    prows = row_end - row0; pcols = a.k - col0;
    qbase = a.q + (long)row0 * a.n + qt * GG_T; qstride = a.n; qstep = 64L * a.n;
    qrows = row_end - row0; qcols = a.n - qt * GG_T;
  }
  // a wave whose 64 output rows all lie past the expert's end only stages
  const bool wave_live = Q_TR || wq * 64 < row_end - row0;

  f32x4 acc[8][4];
#pragma unroll
  for (int ps = 0; ps < 8; ++ps)
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) acc[ps][qs] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int trb = tr_lane_base<128>(g, c);
  PStager sp;
  QStager sq;
  if (ns > 0) {
    sp.loads(pbase, pstride, prows, pcols);
    sq.loads(qbase, qstride, qrows, qcols);
    sp.writes(lds[0][0]);
    sq.writes(lds[0][1]);
  }
  __syncthreads();

  for (int s = 0; s < ns; ++s) {
    const int st = s & 1;
    if (s + 1 < ns) {
      sp.loads(pbase + (s + 1) * pstep, pstride, MODE == GG_TN ? prows - (s + 1) * 64 : prows, pcols);
      sq.loads(qbase + (s + 1) * qstep, qstride, MODE == GG_TN ? qrows - (s + 1) * 64 : qrows, qcols);
    }
    if (wave_live) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 qf[4];
#pragma unroll
        for (int qs = 0; qs < 4; ++qs) {
          if constexpr (Q_TR)
            qf[qs] = read_b_tr<128>(lds[st][1] + (wq >> 1) * (64 * 128), trb, ks * 32, (wq & 1) * 4 + qs);
          else
            qf[qs] = read_a<64>(reinterpret_cast<const short(*)[64]>(lds[st][1]),
                                wq * 64 + tile_row_a(qs, c), ks * 4 + g);
        }
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) {
          bf16x8 pf;
          if constexpr (P_TR)
            pf = read_b_tr<128>(lds[st][0] + wp * (64 * 128), trb, ks * 32, ps);
          else
            pf = read_a<64>(reinterpret_cast<const short(*)[64]>(lds[st][0]),
                            wp * 128 + tile_row_a(ps, c), ks * 4 + g);
#pragma unroll
          for (int qs = 0; qs < 4; ++qs)
            acc[ps][qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, qf[qs], acc[ps][qs], 0, 0, 0);
        }
      }
    }
    if (s + 1 < ns) {
      sp.writes(lds[st ^ 1][0]);
      sq.writes(lds[st ^ 1][1]);
    }
    __syncthreads();
  }
  if (!wave_live) return;

  // epilogue: lane (g, c) holds output row `c` of each q sub-tile and the
  // output columns 4g..4g+3 of each p sub-tile (MFMA D layout)
#pragma unroll
  for (int qs = 0; qs < 4; ++qs) {
    long orow;  // row of the output matrix
    bool live;
    if constexpr (MODE == GG_TN) {
      const int nn = qt * GG_T + wq * 64 + qs * 16 + c;
      live = nn < a.n;
      orow = (long)expert * a.n + nn;
    } else {
      const int m = row0 + wq * 64 + tile_row_a(qs, c);
      live = m < row_end;
      orow = m;
    }
    if (!live) continue;
    if constexpr (!P_TR) {
      bf16* o = reinterpret_cast<bf16*>(a.out) + orow * ocols;
#pragma unroll
      for (int pq = 0; pq < 4; ++pq) {
        const int col = col0 + wp * 128 + 32 * pq + 8 * g;
        if (col >= ocols) continue;
        const f32x4 lo = acc[2 * pq][qs], hi = acc[2 * pq + 1][qs];
        *reinterpret_cast<int4*>(o + col) = make_int4(pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]),
                                                      pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3]));
      }
    } else {
#pragma unroll
      for (int ps = 0; ps < 8; ++ps) {
        const int col = col0 + wp * 128 + ps * 16 + 4 * g;
        if (col >= ocols) continue;
        const f32x4 v = acc[ps][qs];
        if constexpr (OUT32) {
          float4v* o = reinterpret_cast<float4v*>(reinterpret_cast<float*>(a.out) + orow * ocols + col);
          float4v cur = *o;
          cur[0] += v[0]; cur[1] += v[1]; cur[2] += v[2]; cur[3] += v[3];
          *o = cur;
        } else {
          *reinterpret_cast<int2*>(reinterpret_cast<bf16*>(a.out) + orow * ocols + col) =
              make_int2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
        }
      }
    }
  }
}

// tile map of `sizes` for M rows: int32 [4 * T + E + 1], tiles then offsets
torch::Tensor gg_tile_map(const torch::Tensor& sizes, long M, int& T, hipStream_t stream) {
  TORCH_CHECK(sizes.is_cuda() && sizes.dim() == 1 && sizes.is_contiguous(), "grouped_gemm_hip: sizes must be a 1-D device tensor");
  TORCH_CHECK(sizes.scalar_type() == torch::kInt32 || sizes.scalar_type() == torch::kInt64,
              "grouped_gemm_hip: sizes must be int32 or int64");
  const int E = (int)sizes.numel();
  TORCH_CHECK(E >= 1 && E <= GG_MAXE, "grouped_gemm_hip: 1 <= E <= 256");
  TORCH_CHECK(M < (1L << 31) - 2 * GG_T, "grouped_gemm_hip: too many rows");
  T = (int)(M / GG_T) + E + 1;
  auto map = torch::empty({4L * T + E + 1}, sizes.options().dtype(torch::kInt32));
  int* p = map.data_ptr<int>();
  if (sizes.scalar_type() == torch::kInt32)
    hipLaunchKernelGGL(gg_tile_map_kernel<int>, dim3(1), dim3(256), 0, stream, sizes.data_ptr<int>(), E, (int)M, T,
                       reinterpret_cast<int4*>(p), p + 4L * T);
  else
    hipLaunchKernelGGL(gg_tile_map_kernel<int64_t>, dim3(1), dim3(256), 0, stream, sizes.data_ptr<int64_t>(), E,
                       (int)M, T, reinterpret_cast<int4*>(p), p + 4L * T);
  return map;
}

// every global access is a 16-byte (8-byte for bf16 dgrad / wgrad results) vector access
void gg_check_aligned(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "grouped_gemm_hip: ", name, " must start at a 16-byte aligned address");
}

void gg_check_operand(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.is_contiguous(),
              "grouped_gemm_hip: ", name, " must be a contiguous bf16 device tensor");
  gg_check_aligned(t, name);
}

}  // namespace

// trans_b: out[M, n] = a[M, k] @ b[e][n, k]^T (fwd); else out[M, k] = a[M, n] @ b[e][n, k] (dgrad)
torch::Tensor grouped_gemm_hip(torch::Tensor a, torch::Tensor b, torch::Tensor sizes, bool trans_b) {
  gg_check_operand(a, "a");
  gg_check_operand(b, "b");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 3 && b.size(0) == sizes.numel(), "grouped_gemm_hip: a [M, r], b [E, n, k]");
  const long M = a.size(0), n = b.size(1), k = b.size(2);
  TORCH_CHECK(n % 64 == 0 && k % 64 == 0 && n > 0 && k > 0, "grouped_gemm_hip: n and k must be multiples of 64");
  TORCH_CHECK(a.size(1) == (trans_b ? k : n), "grouped_gemm_hip: inner dimensions differ");
  const long ocols = trans_b ? n : k;
  auto out = torch::empty({M, ocols}, a.options());
  if (M == 0) return out;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  int T;
  auto map = gg_tile_map(sizes, M, T, stream);
  GGArgs g;
  g.q = (const bf16*)a.data_ptr(); g.p = (const bf16*)b.data_ptr(); g.out = out.data_ptr();
  g.tiles = reinterpret_cast<const int4*>(map.data_ptr<int>()); g.offs = map.data_ptr<int>() + 4L * T;
  g.n = (int)n; g.k = (int)k; g.E = (int)sizes.numel();
  g.T = T; g.nct = (int)((ocols + GG_T - 1) / GG_T);
  TORCH_CHECK((long)g.T * g.nct < (1L << 30), "grouped_gemm_hip: grid too large");
  const int grid = gg_grid(g.T, g.nct);
  if (trans_b)
    hipLaunchKernelGGL((gg_kernel<GG_NT, false>), dim3(grid), dim3(512), 0, stream, g);
  else
    hipLaunchKernelGGL((gg_kernel<GG_NN, false>), dim3(grid), dim3(512), 0, stream, g);
  return out;
}

// dw [E, n, k]: fp32 and accumulate (dw += dy_e^T x_e, empty experts untouched) or bf16 and
// overwrite (rounded once from fp32, empty experts zero)
void grouped_gemm_hip_wgrad(torch::Tensor dy, torch::Tensor x, torch::Tensor sizes, torch::Tensor dw,
                            bool accumulate) {
  gg_check_operand(dy, "dy");
  gg_check_operand(x, "x");
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && dw.dim() == 3 && dy.size(0) == x.size(0) &&
              dw.size(0) == sizes.numel() && dw.size(1) == dy.size(1) && dw.size(2) == x.size(1),
              "grouped_gemm_hip_wgrad: dy [M, n], x [M, k], dw [E, n, k]");
  TORCH_CHECK(dw.is_cuda() && dw.is_contiguous() &&
              dw.scalar_type() == (accumulate ? torch::kFloat32 : torch::kBFloat16),
              "grouped_gemm_hip_wgrad: dw must be contiguous fp32 (accumulate) or bf16 (overwrite)");
  gg_check_aligned(dw, "dw");
  const long M = dy.size(0), n = dy.size(1), k = x.size(1);
  TORCH_CHECK(n % 64 == 0 && k % 64 == 0 && n > 0 && k > 0, "grouped_gemm_hip: n and k must be multiples of 64");
  hipStream_t stream = at::hip::getCurrentHIPStream();
  int T;
  auto map = gg_tile_map(sizes, M, T, stream);
  GGArgs g;
  g.q = (const bf16*)dy.data_ptr(); g.p = (const bf16*)x.data_ptr(); g.out = dw.data_ptr();
  g.tiles = reinterpret_cast<const int4*>(map.data_ptr<int>()); g.offs = map.data_ptr<int>() + 4L * T;
  g.n = (int)n; g.k = (int)k; g.E = (int)sizes.numel();
  g.T = g.E * (int)((n + GG_T - 1) / GG_T);  // (expert, n tile) pairs
  g.nct = (int)((k + GG_T - 1) / GG_T);
  TORCH_CHECK((long)g.T * g.nct < (1L << 30), "grouped_gemm_hip: grid too large");
  const int grid = gg_grid(g.T, g.nct);
  if (accumulate)
    hipLaunchKernelGGL((gg_kernel<GG_TN, true>), dim3(grid), dim3(512), 0, stream, g);
  else
    hipLaunchKernelGGL((gg_kernel<GG_TN, false>), dim3(grid), dim3(512), 0, stream, g);
}
