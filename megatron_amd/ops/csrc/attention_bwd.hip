// Fused attention BACKWARD for CDNA4 (K1).  Atomic-free two-kernel split
// (the FA2-style trade: P/dS recomputed in both kernels, no dq atomics):
//   bwd_dq :  block per (128 or 256 q rows, b*hq)  — dq = dS K
//   bwd_dkv:  block per (128 kv rows, b*hkv), q-heads of the GQA group looped
//             inside — dv = P^T dO ; dk = dS^T Q
// plus a rowsum preprocess  Drow = sum_d(dO * O).
//
// Structure (v4):
//   * swapped-operand phase-1 MFMAs: every LDS tile is consumed as an
//     A-fragment of a row-major tile.  Which tile row feeds which MFMA row
//     is free, so sub-tile n feeds MFMA row i with tile row
//     32(n>>1) + 8(i>>2) + 4(n&1) + (i&3)  (tile_row_a).  The D-fragment of
//     lane (g,c) then holds column c at tile rows 32(n>>1)+8g+4(n&1)+r
//     (tile_row_d): over the sub-tile pair (2ks, 2ks+1) exactly the rows
//     32ks+8g..+7, in order - the A-fragment of the phase-2 MFMA with the
//     natural k order, without any cross-lane relayout.  The matching
//     B-fragment is read from the SAME row-major tile with the transposing
//     LDS read (ds_read_b64_tr_b16), so no transposed copy of any tile
//     exists, in LDS or in registers.  Every MFMA sees the same operands in
//     the same k slots as with transposed tiles and a permlane relayout, so
//     results are bit-identical to that formulation.
//   * double-buffered swizzled LDS tiles, reg-staged issue-early/write-late
//     prefetch (T14), ONE barrier per tile.  Each block is alone on its CU
//     (512 threads at 2 waves/SIMD), so the barrier count is what it hides
//     least well.
//   * wave-uniform interior-tile path with no mask arithmetic; only tiles on
//     the diagonal, the window edge or the ragged tail evaluate the mask.
//   * per-wave causal/window tile skip; scale folded into one fma per exp.
//   * 1-D grids through attn_block_map (attention_sched.h): whole kv groups
//     per XCD, the heaviest causal block of every head first.
// Tile height (KVBLK, also the q tile of dkv), fragment reads and the tile
// row permutation come from attention_tile.h, shared with the packed kernels
// (attention_varlen.hip), whose dq/dkv are this file's with another mask.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "attention_tile.h"
#include "attention_sched.h"

// ---------------------------------------------------------------------------
// Drow[b, h, s] = sum_d dO[s,b,h,:] * O[s,b,h,:]
// ---------------------------------------------------------------------------
__global__ void attn_bwd_rowsum_kernel(const short8* __restrict__ dout, const short8* __restrict__ out,
                                       float* __restrict__ drow, long rows, int bh, int sq, int d8) {
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  int wpb = blockDim.x / 64;
  for (long row = (long)blockIdx.x * wpb + wid; row < rows; row += (long)gridDim.x * wpb) {
    const short8* a = dout + row * d8;
    const short8* b = out + row * d8;
    float acc = 0.f;
    for (int i = lane; i < d8; i += 64) {
      short8 x = a[i], y = b[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += sbf2f(x[j]) * sbf2f(y[j]);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) {
      long s = row / bh, rem = row % bh;
      drow[rem * sq + s] = acc;
    }
  }
}

// ---------------------------------------------------------------------------
// dq kernel: 8 waves x 16*QT q rows (QT = 2: 256-row blocks, every K/V
// A-fragment read feeds two MFMAs; QT = 1: 128-row blocks for short
// sequences and D = 64), kv tiles of 64.
//   ST  = mfma(A=K_lds,  B=Q_regs)   D[kv][q]
//   dPT = mfma(A=V_lds,  B=dO_regs)  D[kv][q]
//   dq += mfma(A=dS (own D-fragments),  B=K_lds via transposing read)
// ---------------------------------------------------------------------------
template <int D, int QT>
__global__ __launch_bounds__(512) void attn_bwd_dq_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ drow,
    bf16* __restrict__ dq,
    int sq, int skv, int b, int hq, int hkv, float scale, int causal, int window) {
  constexpr int QROWS = 16 * QT;  // q rows per wave
  constexpr int ND = D / 16, NKD = D / 32;
  constexpr int KCH = D / 8;
  constexpr int SREG = KVBLK * D / 8 / 512;

  __shared__ __align__(16) short K_lds[2][KVBLK][D];  // row-major, swizzled, double-buffered
  __shared__ __align__(16) short V_lds[2][KVBLK][D];

  const AttnBlock ab = attn_block_map(blockIdx.x, (sq + 8 * QROWS - 1) / (8 * QROWS), b * hkv, hq / hkv, true);
  if (ab.blk < 0) return;  // padding slot of the grid
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int q0 = ab.blk * (8 * QROWS);
  const int batch = ab.head / hq, head = ab.head % hq;
  const int kv_head = head / (hq / hkv);
  const long q_srow = (long)b * hq * D, k_srow = (long)b * hkv * D;
  const bf16* qbase = q + ((long)batch * hq + head) * D;
  const bf16* dobase = dout + ((long)batch * hq + head) * D;
  const bf16* kbase = k + ((long)batch * hkv + kv_head) * D;
  const bf16* vbase = v + ((long)batch * hkv + kv_head) * D;
  bf16* dqbase = dq + ((long)batch * hq + head) * D;
  const float* lse_row = lse + ((long)batch * hq + head) * sq;
  const float* dr_row = drow + ((long)batch * hq + head) * sq;

  const int row0 = q0 + wid * QROWS;
  const int off = skv - sq;
  const int trb = tr_lane_base<D>(g, c);

  bf16x8 qa[QT][NKD], doa[QT][NKD];
  float my_lse_l2[QT], my_dr_s[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    int qrow = min(row0 + qt * 16 + c, sq - 1);
    const bf16* qr = qbase + (long)qrow * q_srow;
    const bf16* dor = dobase + (long)qrow * q_srow;
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) {
      qa[qt][kd] = load_frag(qr + kd * 32 + g * 8);
      doa[qt][kd] = load_frag(dor + kd * 32 + g * 8);
    }
    my_lse_l2[qt] = lse_row[qrow] * LOG2E;
    my_dr_s[qt] = dr_row[qrow] * scale;
  }
  const float c1 = scale * LOG2E;

  f32x4 dq_acc[QT][ND];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int n = 0; n < ND; ++n) dq_acc[qt][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  int t_end = causal ? min((q0 + 8 * QROWS - 1 + off) / KVBLK, (skv - 1) / KVBLK) : (skv - 1) / KVBLK;
  int t_start = (window > 0) ? max(0, (q0 + off - window + 1) / KVBLK) : 0;

  int st_row[SREG], st_c8[SREG];
#pragma unroll
  for (int i = 0; i < SREG; ++i) {
    int idx = (int)threadIdx.x + i * 512;
    st_row[i] = idx / KCH;
    st_c8[i] = idx % KCH;
  }

  short8 kreg[SREG], vreg[SREG];
  auto stage_loads = [&](int k0) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      int krow = k0 + st_row[i];
      kreg[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      vreg[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (krow < skv) {
        kreg[i] = *reinterpret_cast<const short8*>(kbase + (long)krow * k_srow + st_c8[i] * 8);
        vreg[i] = *reinterpret_cast<const short8*>(vbase + (long)krow * k_srow + st_c8[i] * 8);
      }
    }
  };
  auto stage_writes = [&](int buf) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      *reinterpret_cast<short8*>(&K_lds[buf][st_row[i]][swz<D>(st_row[i], st_c8[i]) * 8]) = kreg[i];
      *reinterpret_cast<short8*>(&V_lds[buf][st_row[i]][swz<D>(st_row[i], st_c8[i]) * 8]) = vreg[i];
    }
  };

  stage_loads(t_start * KVBLK);
  stage_writes(0);
  __syncthreads();

  for (int t = t_start; t <= t_end; ++t) {
    const int k0 = t * KVBLK;
    const int cur = (t - t_start) & 1;
    const bool have_next = (t + 1 <= t_end);
    if (have_next) stage_loads(k0 + KVBLK);

    bool wave_skip = (causal && k0 > row0 + QROWS - 1 + off) ||
                     (window > 0 && k0 + KVBLK - 1 < row0 + off - window + 1);
    if (!wave_skip) {
      // no element of this wave's (q rows) x (kv tile) needs the mask
      const bool interior = (k0 + KVBLK <= skv) && (row0 + QROWS <= sq) &&
                            (!causal || k0 + KVBLK - 1 <= row0 + off) &&
                            (window <= 0 || k0 > row0 + QROWS - 1 + off - window);
      // per 16-row kv sub-tile: S^T/dP^T MFMAs -> dS -> packed pairs
      int pk[KVBLK / 16][QT][2];  // [n][qt][pair]
      auto phase1 = [&](auto masked_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int n = 0; n < KVBLK / 16; ++n) {
          f32x4 st[QT], dpt[QT];
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {
            st[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
            dpt[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          int krow = tile_row_a(n, c);
#pragma unroll
          for (int kd = 0; kd < NKD; ++kd) {
            bf16x8 ak = read_a<D>(K_lds[cur], krow, kd * 4 + g);
            bf16x8 av = read_a<D>(V_lds[cur], krow, kd * 4 + g);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
              st[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, qa[qt][kd], st[qt], 0, 0, 0);
              dpt[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, doa[qt][kd], dpt[qt], 0, 0, 0);
            }
          }
          // P, dS in D-layout [kv = tile_row_d(n, g, r)][q = c]; pack dS pairs along kv
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {
            const int qrow = row0 + qt * 16 + c;
            float ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float pt = exp2f(__builtin_fmaf(st[qt][r], c1, -my_lse_l2[qt]));
              if constexpr (MASKED) {
                int kvrow = k0 + tile_row_d(n, g, r);
                bool ok = (kvrow < skv) && (qrow < sq);
                if (causal) ok &= (kvrow <= qrow + off);
                if (window > 0) ok &= (kvrow > qrow + off - window);
                pt = ok ? pt : 0.f;
              }
              ds[r] = pt * __builtin_fmaf(dpt[qt][r], scale, -my_dr_s[qt]);
            }
            pk[n][qt][0] = pack_bf16x2(ds[0], ds[1]);
            pk[n][qt][1] = pack_bf16x2(ds[2], ds[3]);
          }
        }
      };
      if (interior) phase1(std::false_type{});
      else phase1(std::true_type{});
      __builtin_amdgcn_sched_barrier(0);

      // dq += dS K : one transposed K read feeds all QT MFMAs
#pragma unroll
      for (int ks2 = 0; ks2 < KVBLK / 32; ++ks2) {
        bf16x8 a[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) a[qt] = own_a_frag(pk[2 * ks2][qt], pk[2 * ks2 + 1][qt]);
#pragma unroll
        for (int n = 0; n < ND; ++n) {
          bf16x8 bK = read_b_tr<D>(&K_lds[cur][0][0], trb, ks2 * 32, n);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            dq_acc[qt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[qt], bK, dq_acc[qt][n], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (have_next) {
      // the other buffer was last read in iteration t-1, before that
      // iteration's barrier
      __builtin_amdgcn_s_waitcnt(WAIT_VM0);
      __builtin_amdgcn_sched_barrier(0);
      stage_writes(cur ^ 1);
      __syncthreads();
    }
  }

#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int row = row0 + qt * 16 + g * 4 + r;
      if (row >= sq) continue;
      bf16* dqr = dqbase + (long)row * q_srow;
#pragma unroll
      for (int n = 0; n < ND; ++n) dqr[n * 16 + c] = f2bf(dq_acc[qt][n][r]);
    }
}

// ---------------------------------------------------------------------------
// dk/dv kernel: 8 waves, 128 kv rows per block (16 per wave), q tiles of 64.
//   S  = mfma(A=Q_lds,  B=K_regs)   D[q][kv]
//   dP = mfma(A=dO_lds, B=V_regs)   D[q][kv]
//   dV += mfma(A=P^T  (own D-fragments), B=dO_lds via transposing read)
//   dK += mfma(A=dS^T (own D-fragments), B=Q_lds  via transposing read)
// lse/drow of the q tile never touch LDS: lane (g,c) loads the tile row
// tile_row_d(c>>2, g, c&3), so the 16 rows a lane group needs sit in its own
// row of 16 lanes and are fetched with DPP row broadcasts.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void attn_bwd_dkv_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ drow,
    bf16* __restrict__ dk, bf16* __restrict__ dv,
    int sq, int skv, int b, int hq, int hkv, float scale, int causal, int window) {
  constexpr int ND = D / 16, NKD = D / 32;
  constexpr int KCH = D / 8;
  constexpr int SREG = KVBLK * D / 8 / 512;

  __shared__ __align__(16) short Q_lds[2][KVBLK][D];   // row-major, swizzled, double-buffered
  __shared__ __align__(16) short dO_lds[2][KVBLK][D];

  const AttnBlock ab = attn_block_map(blockIdx.x, (skv + 127) / 128, b * hkv, 1, false);
  if (ab.blk < 0) return;  // padding slot of the grid
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int k0 = ab.blk * 128;  // 8 waves x 16 kv rows
  const int batch = ab.head / hkv, kv_head = ab.head % hkv;
  const int rep = hq / hkv;
  const long q_srow = (long)b * hq * D, k_srow = (long)b * hkv * D;
  const bf16* kbase = k + ((long)batch * hkv + kv_head) * D;
  const bf16* vbase = v + ((long)batch * hkv + kv_head) * D;
  bf16* dkbase = dk + ((long)batch * hkv + kv_head) * D;
  bf16* dvbase = dv + ((long)batch * hkv + kv_head) * D;

  const int krow0 = k0 + wid * 16;
  const int off = skv - sq;
  const float c1 = scale * LOG2E;
  const int trb = tr_lane_base<D>(g, c);
  const int stat_row = tile_row_d(c >> 2, g, c & 3);  // q-tile row whose lse/drow this lane loads

  // K/V B-fragments: lane (g,c) holds row krow0 + c (= B col c)
  bf16x8 ka[NKD], va[NKD];
  {
    int krow = min(krow0 + c, skv - 1);
    const bf16* kr = kbase + (long)krow * k_srow;
    const bf16* vr = vbase + (long)krow * k_srow;
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) {
      ka[kd] = load_frag(kr + kd * 32 + g * 8);
      va[kd] = load_frag(vr + kd * 32 + g * 8);
    }
  }

  f32x4 dk_acc[ND], dv_acc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) {
    dk_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  int tq_start = causal ? max(0, (k0 - off) / KVBLK) : 0;
  int tq_end = (sq - 1) / KVBLK;
  if (window > 0) tq_end = min(tq_end, (k0 + 127 - off + window - 1) / KVBLK);

  int st_row[SREG], st_c8[SREG];
#pragma unroll
  for (int i = 0; i < SREG; ++i) {
    int idx = (int)threadIdx.x + i * 512;
    st_row[i] = idx / KCH;
    st_c8[i] = idx % KCH;
  }

  for (int hg = 0; hg < rep; ++hg) {
    const int head = kv_head * rep + hg;
    const bf16* qbase = q + ((long)batch * hq + head) * D;
    const bf16* dobase = dout + ((long)batch * hq + head) * D;
    const float* lse_row = lse + ((long)batch * hq + head) * sq;
    const float* dr_row = drow + ((long)batch * hq + head) * sq;

    short8 qrm[SREG], dorm[SREG];
    float lse_nx, dr_nx;        // staged for the next tile
    float lse_cu = 0.f, dr_cu = 0.f;  // lse * LOG2E, drow * scale of the current tile
    auto stage_loads = [&](int qt0) {
#pragma unroll
      for (int i = 0; i < SREG; ++i) {
        int r1 = qt0 + st_row[i];
        qrm[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        dorm[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if (r1 < sq) {
          qrm[i] = *reinterpret_cast<const short8*>(qbase + (long)r1 * q_srow + st_c8[i] * 8);
          dorm[i] = *reinterpret_cast<const short8*>(dobase + (long)r1 * q_srow + st_c8[i] * 8);
        }
      }
      int qi = min(qt0 + stat_row, sq - 1);
      lse_nx = lse_row[qi];
      dr_nx = dr_row[qi];
    };
    auto stage_writes = [&](int buf) {
#pragma unroll
      for (int i = 0; i < SREG; ++i) {
        *reinterpret_cast<short8*>(&Q_lds[buf][st_row[i]][swz<D>(st_row[i], st_c8[i]) * 8]) = qrm[i];
        *reinterpret_cast<short8*>(&dO_lds[buf][st_row[i]][swz<D>(st_row[i], st_c8[i]) * 8]) = dorm[i];
      }
      lse_cu = lse_nx * LOG2E;
      dr_cu = dr_nx * scale;
    };

    stage_loads(tq_start * KVBLK);
    stage_writes(0);
    __syncthreads();

    for (int t = tq_start; t <= tq_end; ++t) {
      const int qt0 = t * KVBLK;
      const int cur = (t - tq_start) & 1;
      const bool have_next = (t + 1 <= tq_end);
      if (have_next) stage_loads(qt0 + KVBLK);

      // this wave's kv rows are krow0..+15; skip fully-masked q tiles
      bool wave_skip = (causal && qt0 + KVBLK - 1 < krow0 - off) ||
                       (window > 0 && qt0 >= krow0 + 15 - off + window);
      if (!wave_skip) {
        // no element of this wave's (q tile) x (kv rows) needs the mask
        const bool interior = (qt0 + KVBLK <= sq) && (krow0 + 16 <= skv) &&
                              (!causal || krow0 + 15 <= qt0 + off) &&
                              (window <= 0 || krow0 > qt0 + KVBLK - 1 + off - window);
        f32x4 st[KVBLK / 16], dpt[KVBLK / 16];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int n = 0; n < KVBLK / 16; ++n) {
          st[n] = f32x4{0.f, 0.f, 0.f, 0.f};
          dpt[n] = f32x4{0.f, 0.f, 0.f, 0.f};
          int qrow = tile_row_a(n, c);
#pragma unroll
          for (int kd = 0; kd < NKD; ++kd) {
            bf16x8 aq = read_a<D>(Q_lds[cur], qrow, kd * 4 + g);
            bf16x8 ado = read_a<D>(dO_lds[cur], qrow, kd * 4 + g);
            st[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, ka[kd], st[n], 0, 0, 0);
            dpt[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado, va[kd], dpt[n], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);

        // P, dS in D-layout [q = tile_row_d(n, g, r)][kv = c]; kv col = krow0 + c
        int pkP[KVBLK / 16][2], pkD[KVBLK / 16][2];
        auto softmax_tile = [&](auto masked_c) {
          constexpr bool MASKED = decltype(masked_c)::value;
          const int kvcol = krow0 + c;
#pragma unroll
          for (int n = 0; n < KVBLK / 16; ++n) {
            float pv[4], dsv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float lse_q = row_bcast(lse_cu, 4 * n + r);
              const float dr_q = row_bcast(dr_cu, 4 * n + r);
              float pt = exp2f(__builtin_fmaf(st[n][r], c1, -lse_q));
              if constexpr (MASKED) {
                int qrow = qt0 + tile_row_d(n, g, r);
                bool ok = (kvcol < skv) && (qrow < sq);
                if (causal) ok &= (kvcol <= qrow + off);
                if (window > 0) ok &= (kvcol > qrow + off - window);
                pt = ok ? pt : 0.f;
              }
              pv[r] = pt;
              dsv[r] = pt * __builtin_fmaf(dpt[n][r], scale, -dr_q);
            }
            pkP[n][0] = pack_bf16x2(pv[0], pv[1]);
            pkP[n][1] = pack_bf16x2(pv[2], pv[3]);
            pkD[n][0] = pack_bf16x2(dsv[0], dsv[1]);
            pkD[n][1] = pack_bf16x2(dsv[2], dsv[3]);
          }
        };
        if (interior) softmax_tile(std::false_type{});
        else softmax_tile(std::true_type{});

        // dV += P^T dO ; dK += dS^T Q
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks2 = 0; ks2 < KVBLK / 32; ++ks2) {
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
        // the other buffer was last read in iteration t-1, before that
        // iteration's barrier
        __builtin_amdgcn_s_waitcnt(WAIT_VM0);
        __builtin_amdgcn_sched_barrier(0);
        stage_writes(cur ^ 1);
      }
      __syncthreads();  // also the hg boundary: the next head restages buffer 0
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = krow0 + g * 4 + r;
    if (row >= skv) continue;
    bf16* dkr = dkbase + (long)row * k_srow;
    bf16* dvr = dvbase + (long)row * k_srow;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      dkr[n * 16 + c] = f2bf(dk_acc[n][r]);
      dvr[n * 16 + c] = f2bf(dv_acc[n][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// host wrapper
// ---------------------------------------------------------------------------
template <int D, int QT>
static void launch_dq(dim3 grid, hipStream_t stream, const torch::Tensor& q, const torch::Tensor& k,
                      const torch::Tensor& v, const torch::Tensor& dout, const torch::Tensor& lse,
                      const torch::Tensor& drow, torch::Tensor& dq, int sq, int skv, int b, int hq, int hkv,
                      float scale, int causal, int window) {
  hipLaunchKernelGGL((attn_bwd_dq_kernel<D, QT>), grid, dim3(512), 0, stream,
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     (const bf16*)dout.data_ptr(), lse.data_ptr<float>(), drow.data_ptr<float>(),
                     (bf16*)dq.data_ptr(), sq, skv, b, hq, hkv, scale, causal, window);
}

template <int D>
static void launch_dkv(dim3 grid, hipStream_t stream, const torch::Tensor& q, const torch::Tensor& k,
                       const torch::Tensor& v, const torch::Tensor& dout, const torch::Tensor& lse,
                       const torch::Tensor& drow, torch::Tensor& dk, torch::Tensor& dv, int sq, int skv, int b,
                       int hq, int hkv, float scale, int causal, int window) {
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<D>), grid, dim3(512), 0, stream,
                     (const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),
                     (const bf16*)dout.data_ptr(), lse.data_ptr<float>(), drow.data_ptr<float>(),
                     (bf16*)dk.data_ptr(), (bf16*)dv.data_ptr(), sq, skv, b, hq, hkv, scale, causal, window);
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor out, torch::Tensor lse,
                                    bool causal, double scale, long window) {
  int sq = q.size(0), b = q.size(1), hq = q.size(2), d = q.size(3);
  int skv = k.size(0), hkv = k.size(2);
  TORCH_CHECK(d == 64 || d == 128, "attn_bwd: head dim must be 64 or 128");
  auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
  auto doc = dout.contiguous(), oc = out.contiguous();
  auto dq = torch::empty_like(qc);
  auto dk = torch::empty_like(kc);
  auto dv = torch::empty_like(vc);
  auto drow = torch::empty({b, hq, sq}, q.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentHIPStream();

  long rows = (long)sq * b * hq;
  int d8 = d / 8;
  hipLaunchKernelGGL(attn_bwd_rowsum_kernel, dim3(2048), dim3(256), 0, stream,
                     (const short8*)doc.data_ptr(), (const short8*)oc.data_ptr(),
                     drow.data_ptr<float>(), rows, b * hq, sq, d8);

  // 256-row dq blocks (32 q rows per wave) for long sequences; 128-row blocks
  // via env, for D = 64, or when the sequence is too short to fill 256 rows.
  static const bool force_128 = getenv("MEGATRON_AMD_ATTN_BWD_V2") != nullptr;
  const bool dq_256 = !force_128 && sq >= 256 && d == 128;
  dim3 grid_dq(attn_sched_grid((sq + (dq_256 ? 255 : 127)) / (dq_256 ? 256 : 128), b * hkv, hq / hkv));
  dim3 grid_dkv(attn_sched_grid((skv + 127) / 128, b * hkv, 1));
  const float fs = (float)scale;
  const int ic = causal ? 1 : 0, iw = (int)window;
  if (d == 128) {
    if (dq_256)
      launch_dq<128, 2>(grid_dq, stream, qc, kc, vc, doc, lse, drow, dq, sq, skv, b, hq, hkv, fs, ic, iw);
    else
      launch_dq<128, 1>(grid_dq, stream, qc, kc, vc, doc, lse, drow, dq, sq, skv, b, hq, hkv, fs, ic, iw);
    launch_dkv<128>(grid_dkv, stream, qc, kc, vc, doc, lse, drow, dk, dv, sq, skv, b, hq, hkv, fs, ic, iw);
  } else {
    launch_dq<64, 1>(grid_dq, stream, qc, kc, vc, doc, lse, drow, dq, sq, skv, b, hq, hkv, fs, ic, iw);
    launch_dkv<64>(grid_dkv, stream, qc, kc, vc, doc, lse, drow, dk, dv, sq, skv, b, hq, hkv, fs, ic, iw);
  }
  return {dq, dk, dv};
}
