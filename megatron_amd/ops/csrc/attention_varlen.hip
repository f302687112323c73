// Packed-sequence (varlen / THD) flash attention for CDNA4, forward and
// backward.
//
// Layout: q [t, 1, hq, d], k/v [t, 1, hkv, d] bf16, d in {64, 128}; documents
// are the token ranges [cu_seqlens[j], cu_seqlens[j+1]); every token attends
// inside its own document only, causally or in full.  GQA (hq multiple of
// hkv).  Outputs: o [t, 1, hq, d] bf16, lse [hq, t] f32; dq/dk/dv bf16.
//
// Structure:
//   * A prep kernel turns cu_seqlens into per-token bounds row_lo / row_hi
//     (document start, exclusive end).  The whole mask is then
//         row_lo[r] <= col < (causal ? r + 1 : row_hi[r]).
//     Nothing reads cu_seqlens on the host; every grid depends on t only.
//   * Blocks cover fixed token ranges, whatever the document boundaries are:
//     there is no work list.  Every kernel runs on a 1-D grid through
//     attn_block_map (attention_sched.h): whole kv groups per XCD, blocks in
//     the order that starts the heaviest causal block of a head first (a
//     heuristic once documents cut the ramp; the split by head stays exact).
//     Both bounds are non-decreasing in the row, so
//     the kv tiles a wave needs are [lo(first row)/64, (hi(last row)-1)/64]
//     and a block's range is the union over its waves.  A wave skips the MFMA
//     and softmax work of tiles outside its own range but still stages and
//     takes the barriers.
//   * A tile is interior for a wave when lo(last row) <= k0 and
//     hi(first row) >= k0 + 64: two wave-uniform compares, no mask arithmetic.
//     Only tiles that cross a document edge, the diagonal or the ragged tail
//     evaluate the per-element mask.
//   * All three MFMA kernels use row-major swizzled LDS tiles, double-buffered
//     with reg-staged issue-early/write-late prefetch and one barrier per
//     tile.  First-phase MFMAs take the operands swapped (tile as A, the
//     register-resident side as B) with the tile_row_a row permutation, so
//     softmax reductions are two shuffles and the packed P / dS D-fragments
//     are the second-phase A-fragments without a relayout; second-phase
//     B-fragments come from the same tile with the transposing LDS read.  In
//     the forward that removes both the transposed V tile and the permlane
//     relayout the dense forward uses.
//   * Backward = rowsum preprocess + dq (iterates like the forward) + dkv over
//     token-aligned kv blocks x hkv with the q heads of the GQA group looped
//     inside: no atomics, bit-reproducible.  In dkv rows and columns exchange
//     roles: kv column j is seen by q rows [causal ? j : row_lo[j], row_hi[j]).
//   * In the forward the defer-max decision is per row (a row only takes a new
//     max when its own max grew past the threshold), so a row's result never
//     depends on the data of other documents sharing its wave.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "attention_tile.h"
#include "attention_sched.h"

#define RESCALE_THR 8.0f

namespace {

// ---------------------------------------------------------------------------
// row_lo / row_hi from cu_seqlens, one thread per token.  Token r belongs to
// document j = #{i in [1, n_docs) : cu[i] <= r}: tokens before cu[0] fall into
// the first document and tokens at or past cu[n_docs] into the last, like the
// torch reference.  The clamps keep lo <= r < hi <= t for any cu contents, so
// no tile index derived from the bounds can leave [0, t).
// ---------------------------------------------------------------------------
__global__ void attn_varlen_bounds_kernel(const int* __restrict__ cu, int n_docs, int t,
                                          int* __restrict__ row_lo, int* __restrict__ row_hi) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= t) return;
  int lo = 1, hi = n_docs;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (cu[mid] <= r) lo = mid + 1;
    else hi = mid;
  }
  const int j = lo - 1;
  const int start = (j > 0) ? cu[j] : 0;
  const int end = (j + 1 < n_docs) ? cu[j + 1] : t;
  row_lo[r] = max(0, min(start, r));
  row_hi[r] = min(t, max(end, r + 1));
}

// drow[h, r] = sum_d dO[r, h, :] * O[r, h, :]; one wave per (r, h) row.
__global__ void attn_varlen_rowsum_kernel(const short8* __restrict__ dout, const short8* __restrict__ out,
                                          float* __restrict__ drow, long rows, int hq, int t, int d8) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x / 64;
  for (long row = (long)blockIdx.x * wpb + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * wpb) {
    float acc = 0.f;
    if (lane < d8) {
      short8 x = dout[row * d8 + lane], y = out[row * d8 + lane];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += sbf2f(x[j]) * sbf2f(y[j]);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) drow[(row % hq) * t + row / hq] = acc;
  }
}

// Bounds of the 16*NT consecutive rows a wave owns (q rows in fwd/dq, kv rows
// in dkv), starting at row0 < t.  lo/hi: this lane's rows row0 + 16*i + c
// (clamped to t - 1; clamped rows repeat the last row and are never stored).
// The *_first / *_last members are wave-uniform.  `diag` is the causal bound:
// in fwd/dq it replaces hi (col < r + 1), in dkv it replaces lo (row >= j).
template <int NT>
struct WaveBounds {
  int lo[NT], hi[NT];
  int lo_first, lo_last, hi_first, hi_last;

  __device__ __forceinline__ void load(const int* __restrict__ row_lo, const int* __restrict__ row_hi,
                                       int row0, int c, int t, bool diag_hi, bool diag_lo) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int r = min(row0 + 16 * i + c, t - 1);
      lo[i] = diag_lo ? r : row_lo[r];
      hi[i] = diag_hi ? r + 1 : row_hi[r];
    }
    const int rl = min(row0 + 16 * NT - 1, t - 1);
    lo_first = __builtin_amdgcn_readfirstlane(diag_lo ? row0 : row_lo[row0]);
    lo_last = __builtin_amdgcn_readfirstlane(diag_lo ? rl : row_lo[rl]);
    hi_first = __builtin_amdgcn_readfirstlane(diag_hi ? row0 + 1 : row_hi[row0]);
    hi_last = __builtin_amdgcn_readfirstlane(diag_hi ? rl + 1 : row_hi[rl]);
  }
  // first and last streamed tile this wave has any work in
  __device__ __forceinline__ int tile_first() const { return lo_first / KVBLK; }
  __device__ __forceinline__ int tile_last() const { return (hi_last - 1) / KVBLK; }
  // no element of (this wave's rows) x [x0, x0 + KVBLK) is masked
  __device__ __forceinline__ bool interior(int x0) const { return lo_last <= x0 && hi_first >= x0 + KVBLK; }
  __device__ __forceinline__ bool ok(int i, int x) const { return x >= lo[i] && x < hi[i]; }
};

// ---------------------------------------------------------------------------
// forward: 8 waves x 32 q rows (256-token blocks), kv tiles of 64.
//   S^T = mfma(A=K_lds, B=Q_regs)                 D[kv][q]
//   O  += mfma(A=P (own D-fragments), B=V_lds via transposing read)
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void attn_varlen_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const int* __restrict__ row_lo, const int* __restrict__ row_hi,
    bf16* __restrict__ o, float* __restrict__ lse,
    int t, int hq, int hkv, float scale, int causal, int nqc) {
  constexpr int QT = 2, QROWS = 16 * QT, QBLK = 8 * QROWS;
  constexpr int ND = D / 16, NKD = D / 32;

  __shared__ __align__(16) short K_lds[2][KVBLK][D];
  __shared__ __align__(16) short V_lds[2][KVBLK][D];

  const AttnBlock ab = attn_block_map(blockIdx.x, nqc, hkv, hq / hkv, true);
  if (ab.blk < 0) return;  // padding slot of the grid
  const int head = ab.head;
  const int q0 = ab.blk * QBLK;
  const int kv_head = head / (hq / hkv);

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const long q_srow = (long)hq * D, k_srow = (long)hkv * D;
  const bf16* qbase = q + (long)head * D;
  const bf16* kbase = k + (long)kv_head * D;
  const bf16* vbase = v + (long)kv_head * D;
  bf16* obase = o + (long)head * D;

  const int row0 = q0 + wid * QROWS;
  const bool wave_live = row0 < t;
  const int trb = tr_lane_base<D>(g, c);

  WaveBounds<QT> wb;
  wb.load(row_lo, row_hi, min(row0, t - 1), c, t, causal != 0, false);

  bf16x8 qb[QT][NKD];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const bf16* qr = qbase + (long)min(row0 + qt * 16 + c, t - 1) * q_srow;
#pragma unroll
    for (int ks = 0; ks < NKD; ++ks) qb[qt][ks] = load_frag(qr + ks * 32 + g * 8);
  }

  f32x4 oacc[QT][ND];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int n = 0; n < ND; ++n) oacc[qt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -1e30f; l_run[qt] = 0.f; }

  // block tile range: union over the waves (bounds are monotone in the row)
  const int rl_blk = min(q0 + QBLK - 1, t - 1);
  const int t_start = row_lo[q0] / KVBLK;
  const int t_end = ((causal ? rl_blk + 1 : row_hi[rl_blk]) - 1) / KVBLK;

  const float c1 = scale * LOG2E;
  const float thr_raw = RESCALE_THR / scale;

  TileStager<D> stg;
  stg.loads(kbase, vbase, k_srow, t_start * KVBLK, t);
  stg.writes(K_lds[0], V_lds[0]);
  __syncthreads();

  for (int tile = t_start; tile <= t_end; ++tile) {
    const int k0 = tile * KVBLK;
    const int cur = (tile - t_start) & 1;
    const bool have_next = (tile + 1 <= t_end);
    if (have_next) stg.loads(kbase, vbase, k_srow, k0 + KVBLK, t);

    if (wave_live && tile >= wb.tile_first() && tile <= wb.tile_last()) {
      // ---- S^T = K Q^T (raw scores; scale is folded into the exp fma) ----
      f32x4 st[KVBLK / 16][QT];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int n = 0; n < KVBLK / 16; ++n) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) st[n][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int krow = tile_row_a(n, c);
#pragma unroll
        for (int ks = 0; ks < NKD; ++ks) {
          bf16x8 ak = read_a<D>(K_lds[cur], krow, ks * 4 + g);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            st[n][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, qb[qt][ks], st[n][qt], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- mask (edge tiles only) + row max; lane (g,c): q = row0+16qt+c,
      //      kv = k0 + tile_row_d(n, g, r) ----
      float pmax[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) pmax[qt] = -1e30f;
      if (!wb.interior(k0)) {
#pragma unroll
        for (int n = 0; n < KVBLK / 16; ++n)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (!wb.ok(qt, k0 + tile_row_d(n, g, r))) st[n][qt][r] = -1e30f;
      }
#pragma unroll
      for (int n = 0; n < KVBLK / 16; ++n)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r) pmax[qt] = fmaxf(pmax[qt], st[n][qt][r]);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        pmax[qt] = fmaxf(pmax[qt], __shfl_xor(pmax[qt], 16, 64));
        pmax[qt] = fmaxf(pmax[qt], __shfl_xor(pmax[qt], 32, 64));
      }

      // ---- defer-max: a row takes a new max only when its own max grew by
      //      more than THR; the rescale pass runs if any row of the wave does ----
      bool need[QT], any_need = false;
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        need[qt] = (pmax[qt] > m_run[qt] + thr_raw) || (m_run[qt] == -1e30f);
        any_need |= need[qt];
      }
      if (__any(any_need)) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          const float m_new = need[qt] ? fmaxf(m_run[qt], pmax[qt]) : m_run[qt];
          const float alpha = __expf((m_run[qt] - m_new) * scale);
          m_run[qt] = m_new;
          l_run[qt] *= alpha;
          // alpha lives in the q = c layout, O in the q = 4g + r layout
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float a = __shfl(alpha, (lane & 48) + g * 4 + r, 64);
#pragma unroll
            for (int n = 0; n < ND; ++n) oacc[qt][n][r] *= a;
          }
        }
      }

      // ---- p = exp2(s*c1 - m*c1), row sums, pack pairs along kv ----
      int pk[KVBLK / 16][QT][2];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float ps = 0.f;
        const float mc = m_run[qt] * c1;
#pragma unroll
        for (int n = 0; n < KVBLK / 16; ++n) {
          float p[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sv = st[n][qt][r];
            p[r] = (sv <= -1e29f) ? 0.f : exp2f(__builtin_fmaf(sv, c1, -mc));
            ps += p[r];
          }
          pk[n][qt][0] = pack_bf16x2(p[0], p[1]);
          pk[n][qt][1] = pack_bf16x2(p[2], p[3]);
        }
        l_run[qt] += ps;
      }

      // ---- O += P V : one transposed V read feeds both q sub-tiles ----
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks2 = 0; ks2 < KVBLK / 32; ++ks2) {
        bf16x8 a[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) a[qt] = own_a_frag(pk[2 * ks2][qt], pk[2 * ks2 + 1][qt]);
#pragma unroll
        for (int n = 0; n < ND; ++n) {
          bf16x8 bV = read_b_tr<D>(&V_lds[cur][0][0], trb, ks2 * 32, n);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            oacc[qt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[qt], bV, oacc[qt][n], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (have_next) {
      // the other buffer was last read in iteration tile-1, before that
      // iteration's barrier
      __builtin_amdgcn_s_waitcnt(WAIT_VM0);
      __builtin_amdgcn_sched_barrier(0);
      stg.writes(K_lds[cur ^ 1], V_lds[cur ^ 1]);
      __syncthreads();
    }
  }

  // ---- epilogue: finish l over the 4 lanes per q column, normalise ----
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    l_run[qt] += __shfl_xor(l_run[qt], 16, 64);
    l_run[qt] += __shfl_xor(l_run[qt], 32, 64);
    const float linv = (l_run[qt] > 0.f) ? 1.f / l_run[qt] : 0.f;
    const int qrow = row0 + qt * 16 + c;
    if (g == 0 && qrow < t)
      lse[(long)head * t + qrow] = m_run[qt] * scale + __logf(fmaxf(l_run[qt], 1e-30f));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float inv = __shfl(linv, (lane & 48) + g * 4 + r, 64);
      const int orow_i = row0 + qt * 16 + g * 4 + r;
      if (orow_i >= t) continue;
      bf16* orow = obase + (long)orow_i * q_srow;
#pragma unroll
      for (int n = 0; n < ND; ++n) orow[n * 16 + c] = f2bf(oacc[qt][n][r] * inv);
    }
  }
}

// ---------------------------------------------------------------------------
// dq: 8 waves x 16 q rows (128-token blocks), kv tiles of 64.
//   S^T  = mfma(A=K_lds, B=Q_regs)    D[kv][q]
//   dP^T = mfma(A=V_lds, B=dO_regs)   D[kv][q]
//   dq  += mfma(A=dS (own D-fragments), B=K_lds via transposing read)
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void attn_varlen_dq_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ drow,
    const int* __restrict__ row_lo, const int* __restrict__ row_hi,
    bf16* __restrict__ dq, int t, int hq, int hkv, float scale, int causal) {
  constexpr int QBLK = 128;
  constexpr int ND = D / 16, NKD = D / 32;

  __shared__ __align__(16) short K_lds[2][KVBLK][D];
  __shared__ __align__(16) short V_lds[2][KVBLK][D];

  const AttnBlock ab = attn_block_map(blockIdx.x, (t + QBLK - 1) / QBLK, hkv, hq / hkv, true);
  if (ab.blk < 0) return;  // padding slot of the grid
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int q0 = ab.blk * QBLK;
  const int head = ab.head;
  const int kv_head = head / (hq / hkv);
  const long q_srow = (long)hq * D, k_srow = (long)hkv * D;
  const bf16* kbase = k + (long)kv_head * D;
  const bf16* vbase = v + (long)kv_head * D;

  const int row0 = q0 + wid * 16;
  const bool wave_live = row0 < t;
  const int trb = tr_lane_base<D>(g, c);

  WaveBounds<1> wb;
  wb.load(row_lo, row_hi, min(row0, t - 1), c, t, causal != 0, false);

  bf16x8 qa[NKD], doa[NKD];
  const int qrow = min(row0 + c, t - 1);
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd) {
    qa[kd] = load_frag(q + (long)qrow * q_srow + (long)head * D + kd * 32 + g * 8);
    doa[kd] = load_frag(dout + (long)qrow * q_srow + (long)head * D + kd * 32 + g * 8);
  }
  const float my_lse_l2 = lse[(long)head * t + qrow] * LOG2E;
  const float my_dr_s = drow[(long)head * t + qrow] * scale;
  const float c1 = scale * LOG2E;

  f32x4 dq_acc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) dq_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int rl_blk = min(q0 + QBLK - 1, t - 1);
  const int t_start = row_lo[q0] / KVBLK;
  const int t_end = ((causal ? rl_blk + 1 : row_hi[rl_blk]) - 1) / KVBLK;

  TileStager<D> stg;
  stg.loads(kbase, vbase, k_srow, t_start * KVBLK, t);
  stg.writes(K_lds[0], V_lds[0]);
  __syncthreads();

  for (int tile = t_start; tile <= t_end; ++tile) {
    const int k0 = tile * KVBLK;
    const int cur = (tile - t_start) & 1;
    const bool have_next = (tile + 1 <= t_end);
    if (have_next) stg.loads(kbase, vbase, k_srow, k0 + KVBLK, t);

    if (wave_live && tile >= wb.tile_first() && tile <= wb.tile_last()) {
      int pk[KVBLK / 16][2];
      auto phase1 = [&](auto masked_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int n = 0; n < KVBLK / 16; ++n) {
          f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f}, dpt = f32x4{0.f, 0.f, 0.f, 0.f};
          const int krow = tile_row_a(n, c);
#pragma unroll
          for (int kd = 0; kd < NKD; ++kd) {
            st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_a<D>(K_lds[cur], krow, kd * 4 + g), qa[kd], st, 0, 0, 0);
            dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_a<D>(V_lds[cur], krow, kd * 4 + g), doa[kd], dpt, 0, 0, 0);
          }
          // P, dS in D-layout [kv = tile_row_d(n, g, r)][q = c]; pack dS pairs along kv
          float ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pt = exp2f(__builtin_fmaf(st[r], c1, -my_lse_l2));
            if constexpr (MASKED) pt = wb.ok(0, k0 + tile_row_d(n, g, r)) ? pt : 0.f;
            ds[r] = pt * __builtin_fmaf(dpt[r], scale, -my_dr_s);
          }
          pk[n][0] = pack_bf16x2(ds[0], ds[1]);
          pk[n][1] = pack_bf16x2(ds[2], ds[3]);
        }
      };
      if (wb.interior(k0)) phase1(std::false_type{});
      else phase1(std::true_type{});
      __builtin_amdgcn_sched_barrier(0);

#pragma unroll
      for (int ks2 = 0; ks2 < KVBLK / 32; ++ks2) {
        bf16x8 a = own_a_frag(pk[2 * ks2], pk[2 * ks2 + 1]);
#pragma unroll
        for (int n = 0; n < ND; ++n)
          dq_acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, read_b_tr<D>(&K_lds[cur][0][0], trb, ks2 * 32, n), dq_acc[n], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (have_next) {
      __builtin_amdgcn_s_waitcnt(WAIT_VM0);
      __builtin_amdgcn_sched_barrier(0);
      stg.writes(K_lds[cur ^ 1], V_lds[cur ^ 1]);
      __syncthreads();
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + g * 4 + r;
    if (row >= t) continue;
    bf16* dqr = dq + (long)row * q_srow + (long)head * D;
#pragma unroll
    for (int n = 0; n < ND; ++n) dqr[n * 16 + c] = f2bf(dq_acc[n][r]);
  }
}

// ---------------------------------------------------------------------------
// dk/dv: 8 waves x 16 kv rows (128-token kv blocks) x hkv, q tiles of 64, the
// q heads of the GQA group looped inside.
//   S  = mfma(A=Q_lds,  B=K_regs)   D[q][kv]
//   dP = mfma(A=dO_lds, B=V_regs)   D[q][kv]
//   dV += mfma(A=P^T  (own D-fragments), B=dO_lds via transposing read)
//   dK += mfma(A=dS^T (own D-fragments), B=Q_lds  via transposing read)
// lse/drow of the q tile: lane (g,c) loads tile row tile_row_d(c>>2, g, c&3),
// so the 16 rows a lane group needs sit in its own row of 16 lanes (DPP row
// broadcasts, no LDS).
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void attn_varlen_dkv_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ drow,
    const int* __restrict__ row_lo, const int* __restrict__ row_hi,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int t, int hq, int hkv, float scale, int causal) {
  constexpr int KBLK = 128, QTILE = KVBLK;
  constexpr int ND = D / 16, NKD = D / 32;

  __shared__ __align__(16) short Q_lds[2][QTILE][D];
  __shared__ __align__(16) short dO_lds[2][QTILE][D];

  const AttnBlock ab = attn_block_map(blockIdx.x, (t + KBLK - 1) / KBLK, hkv, 1, false);
  if (ab.blk < 0) return;  // padding slot of the grid
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int k0 = ab.blk * KBLK;
  const int kv_head = ab.head;
  const int rep = hq / hkv;
  const long q_srow = (long)hq * D, k_srow = (long)hkv * D;

  const int krow0 = k0 + wid * 16;
  const bool wave_live = krow0 < t;
  const float c1 = scale * LOG2E;
  const int trb = tr_lane_base<D>(g, c);
  const int stat_row = tile_row_d(c >> 2, g, c & 3);

  // q rows that see kv column j: [causal ? j : row_lo[j], row_hi[j])
  WaveBounds<1> wb;
  wb.load(row_lo, row_hi, min(krow0, t - 1), c, t, false, causal != 0);

  bf16x8 ka[NKD], va[NKD];
  {
    const long krow = min(krow0 + c, t - 1);
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) {
      ka[kd] = load_frag(k + krow * k_srow + (long)kv_head * D + kd * 32 + g * 8);
      va[kd] = load_frag(v + krow * k_srow + (long)kv_head * D + kd * 32 + g * 8);
    }
  }

  f32x4 dk_acc[ND], dv_acc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) {
    dk_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int tq_start = (causal ? k0 : row_lo[k0]) / QTILE;
  const int tq_end = (row_hi[min(k0 + KBLK - 1, t - 1)] - 1) / QTILE;

  TileStager<D> stg;
  for (int hg = 0; hg < rep; ++hg) {
    const int head = kv_head * rep + hg;
    const bf16* qbase = q + (long)head * D;
    const bf16* dobase = dout + (long)head * D;
    const float* lse_row = lse + (long)head * t;
    const float* dr_row = drow + (long)head * t;

    float lse_nx, dr_nx;              // staged for the next tile
    float lse_cu = 0.f, dr_cu = 0.f;  // lse * LOG2E, drow * scale of the current tile
    auto stage_loads = [&](int qt0) {
      stg.loads(qbase, dobase, q_srow, qt0, t);
      const int qi = min(qt0 + stat_row, t - 1);
      lse_nx = lse_row[qi];
      dr_nx = dr_row[qi];
    };
    auto stage_writes = [&](int buf) {
      stg.writes(Q_lds[buf], dO_lds[buf]);
      lse_cu = lse_nx * LOG2E;
      dr_cu = dr_nx * scale;
    };

    stage_loads(tq_start * QTILE);
    stage_writes(0);
    __syncthreads();

    for (int tile = tq_start; tile <= tq_end; ++tile) {
      const int qt0 = tile * QTILE;
      const int cur = (tile - tq_start) & 1;
      const bool have_next = (tile + 1 <= tq_end);
      if (have_next) stage_loads(qt0 + QTILE);

      if (wave_live && tile >= wb.tile_first() && tile <= wb.tile_last()) {
        f32x4 st[QTILE / 16], dpt[QTILE / 16];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int n = 0; n < QTILE / 16; ++n) {
          st[n] = f32x4{0.f, 0.f, 0.f, 0.f};
          dpt[n] = f32x4{0.f, 0.f, 0.f, 0.f};
          const int qrow = tile_row_a(n, c);
#pragma unroll
          for (int kd = 0; kd < NKD; ++kd) {
            st[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_a<D>(Q_lds[cur], qrow, kd * 4 + g), ka[kd], st[n], 0, 0, 0);
            dpt[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_a<D>(dO_lds[cur], qrow, kd * 4 + g), va[kd], dpt[n], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);

        // P, dS in D-layout [q = qt0 + tile_row_d(n, g, r)][kv = krow0 + c]
        int pkP[QTILE / 16][2], pkD[QTILE / 16][2];
        auto softmax_tile = [&](auto masked_c) {
          constexpr bool MASKED = decltype(masked_c)::value;
#pragma unroll
          for (int n = 0; n < QTILE / 16; ++n) {
            float pv[4], dsv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float lse_q = row_bcast(lse_cu, 4 * n + r);
              const float dr_q = row_bcast(dr_cu, 4 * n + r);
              float pt = exp2f(__builtin_fmaf(st[n][r], c1, -lse_q));
              if constexpr (MASKED) pt = wb.ok(0, qt0 + tile_row_d(n, g, r)) ? pt : 0.f;
              pv[r] = pt;
              dsv[r] = pt * __builtin_fmaf(dpt[n][r], scale, -dr_q);
            }
            pkP[n][0] = pack_bf16x2(pv[0], pv[1]);
            pkP[n][1] = pack_bf16x2(pv[2], pv[3]);
            pkD[n][0] = pack_bf16x2(dsv[0], dsv[1]);
            pkD[n][1] = pack_bf16x2(dsv[2], dsv[3]);
          }
        };
        if (wb.interior(qt0)) softmax_tile(std::false_type{});
        else softmax_tile(std::true_type{});

        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks2 = 0; ks2 < QTILE / 32; ++ks2) {
          bf16x8 aP = own_a_frag(pkP[2 * ks2], pkP[2 * ks2 + 1]);
          bf16x8 aD = own_a_frag(pkD[2 * ks2], pkD[2 * ks2 + 1]);
#pragma unroll
          for (int n = 0; n < ND; ++n) {
            bf16x8 bdo = read_b_tr<D>(&dO_lds[cur][0][0], trb, ks2 * 32, n);
            bf16x8 bq = read_b_tr<D>(&Q_lds[cur][0][0], trb, ks2 * 32, n);
            dv_acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aP, bdo, dv_acc[n], 0, 0, 0);
            dk_acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aD, bq, dk_acc[n], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }

      if (have_next) {
        __builtin_amdgcn_s_waitcnt(WAIT_VM0);
        __builtin_amdgcn_sched_barrier(0);
        stage_writes(cur ^ 1);
      }
      __syncthreads();  // also the hg boundary: the next head restages buffer 0
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = krow0 + g * 4 + r;
    if (row >= t) continue;
    bf16* dkr = dk + (long)row * k_srow + (long)kv_head * D;
    bf16* dvr = dv + (long)row * k_srow + (long)kv_head * D;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      dkr[n * 16 + c] = f2bf(dk_acc[n][r]);
      dvr[n * 16 + c] = f2bf(dv_acc[n][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct Shape { int t, hq, hkv, d; };

Shape check_inputs(const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
                   const torch::Tensor& cu) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() && cu.is_cuda(), "attn_varlen: device tensors only");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4 && q.size(1) == 1 && k.size(1) == 1 && v.size(1) == 1,
              "attn_varlen: q/k/v are [t, 1, h, d]");
  TORCH_CHECK(q.dtype() == torch::kBFloat16 && k.dtype() == torch::kBFloat16 && v.dtype() == torch::kBFloat16,
              "attn_varlen: bf16 only");
  Shape s{(int)q.size(0), (int)q.size(2), (int)k.size(2), (int)q.size(3)};
  TORCH_CHECK(s.d == 64 || s.d == 128, "attn_varlen: head dim must be 64 or 128");
  TORCH_CHECK(k.size(3) == s.d && v.size(3) == s.d, "attn_varlen: q, k and v share one head dim");
  TORCH_CHECK(s.t > 0 && k.size(0) == s.t && v.size(0) == s.t && v.size(2) == s.hkv, "attn_varlen: q/k/v token counts differ");
  TORCH_CHECK(s.hkv > 0 && s.hq % s.hkv == 0, "attn_varlen: hq must be a multiple of hkv");
  TORCH_CHECK(cu.dim() == 1 && cu.dtype() == torch::kInt32 && cu.is_contiguous() && cu.numel() >= 2,
              "attn_varlen: cu_seqlens is a contiguous int32 [n_docs + 1]");
  return s;
}

// bounds[0] = row_lo, bounds[1] = row_hi
torch::Tensor row_bounds(const torch::Tensor& cu, int t, hipStream_t stream) {
  auto bounds = torch::empty({2, t}, cu.options());
  int* p = bounds.data_ptr<int>();
  hipLaunchKernelGGL(attn_varlen_bounds_kernel, dim3((t + 255) / 256), dim3(256), 0, stream,
                     cu.data_ptr<int>(), (int)cu.numel() - 1, t, p, p + t);
  return bounds;
}

template <int D>
void launch_fwd(hipStream_t stream, const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
                const int* lo, torch::Tensor& out, torch::Tensor& lse, Shape s, float scale, int causal) {
  const int nqc = (s.t + 255) / 256;
  hipLaunchKernelGGL((attn_varlen_fwd_kernel<D>), dim3(attn_sched_grid(nqc, s.hkv, s.hq / s.hkv)), dim3(512), 0, stream,
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     lo, lo + s.t, (bf16*)out.data_ptr(), lse.data_ptr<float>(),
                     s.t, s.hq, s.hkv, scale, causal, nqc);
}

template <int D>
void launch_bwd(hipStream_t stream, const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
                const torch::Tensor& dout, const torch::Tensor& lse, const torch::Tensor& drow, const int* lo,
                torch::Tensor& dq, torch::Tensor& dk, torch::Tensor& dv, Shape s, float scale, int causal) {
  const int nblk = (s.t + 127) / 128;
  hipLaunchKernelGGL((attn_varlen_dq_kernel<D>), dim3(attn_sched_grid(nblk, s.hkv, s.hq / s.hkv)), dim3(512), 0, stream,
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     (const bf16*)dout.data_ptr(), lse.data_ptr<float>(), drow.data_ptr<float>(),
                     lo, lo + s.t, (bf16*)dq.data_ptr(), s.t, s.hq, s.hkv, scale, causal);
  hipLaunchKernelGGL((attn_varlen_dkv_kernel<D>), dim3(attn_sched_grid(nblk, s.hkv, 1)), dim3(512), 0, stream,
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     (const bf16*)dout.data_ptr(), lse.data_ptr<float>(), drow.data_ptr<float>(),
                     lo, lo + s.t, (bf16*)dk.data_ptr(), (bf16*)dv.data_ptr(), s.t, s.hq, s.hkv, scale, causal);
}

}  // namespace

std::vector<torch::Tensor> attn_varlen_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                           torch::Tensor cu_seqlens, bool causal, double scale) {
  const Shape s = check_inputs(q, k, v, cu_seqlens);
  auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
  auto out = torch::empty_like(qc);
  auto lse = torch::empty({s.hq, s.t}, q.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentHIPStream();
  auto bounds = row_bounds(cu_seqlens, s.t, stream);
  const int* lo = bounds.data_ptr<int>();
  if (s.d == 128) launch_fwd<128>(stream, qc, kc, vc, lo, out, lse, s, (float)scale, causal ? 1 : 0);
  else launch_fwd<64>(stream, qc, kc, vc, lo, out, lse, s, (float)scale, causal ? 1 : 0);
  return {out, lse};
}

std::vector<torch::Tensor> attn_varlen_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, torch::Tensor out, torch::Tensor lse,
                                           torch::Tensor cu_seqlens, bool causal, double scale) {
  const Shape s = check_inputs(q, k, v, cu_seqlens);
  TORCH_CHECK(dout.is_cuda() && out.is_cuda() && dout.dtype() == torch::kBFloat16 && out.dtype() == torch::kBFloat16 &&
              dout.sizes() == q.sizes() && out.sizes() == q.sizes(), "attn_varlen_bwd: dout/out must match q");
  TORCH_CHECK(lse.is_cuda() && lse.dtype() == torch::kFloat32 && lse.is_contiguous() && lse.dim() == 2 &&
              lse.size(0) == s.hq && lse.size(1) == s.t, "attn_varlen_bwd: lse is f32 [hq, t]");
  auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
  auto doc = dout.contiguous(), oc = out.contiguous();
  auto dq = torch::empty_like(qc);
  auto dk = torch::empty_like(kc);
  auto dv = torch::empty_like(vc);
  auto drow = torch::empty({s.hq, s.t}, q.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentHIPStream();
  auto bounds = row_bounds(cu_seqlens, s.t, stream);
  const int* lo = bounds.data_ptr<int>();

  const long rows = (long)s.t * s.hq;
  hipLaunchKernelGGL(attn_varlen_rowsum_kernel, dim3(grid_for(rows * 64, 256)), dim3(256), 0, stream,
                     (const short8*)doc.data_ptr(), (const short8*)oc.data_ptr(),
                     drow.data_ptr<float>(), rows, s.hq, s.t, s.d / 8);
  if (s.d == 128) launch_bwd<128>(stream, qc, kc, vc, doc, lse, drow, lo, dq, dk, dv, s, (float)scale, causal ? 1 : 0);
  else launch_bwd<64>(stream, qc, kc, vc, doc, lse, drow, lo, dq, dk, dv, s, (float)scale, causal ? 1 : 0);
  return {dq, dk, dv};
}
