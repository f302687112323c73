// Mamba2 SSD scan for CDNA4, forward only: the chunked scan for prefill and
// evaluation and the single-token step for decode.
//
//   h_t = exp(dt_t A) h_{t-1} + dt_t x_t (x) B_t        h: [p, n] per (batch, head)
//   y_t = C_t . h_t + D x_t
//
// Layout: x [b, l, h, p] bf16, dt [b, l, h] bf16 or f32, A [h] f32, B/C
// [b, l, g, n] bf16 (h % g == 0), D [h] f32 or none, initial state
// [b, h, p, n] f32 or none; p and n in {64, 128}, any l >= 1.  Outputs
// y [b, l, h, p] bf16 and the final state [b, h, p, n] f32.  x, B and C may
// be row-strided views (the mixer passes slices of one conv output).
//
// The sequence is cut into chunks of Q = 128 rows (8 waves x 16 rows, two
// KVBLK tiles).  With cs_i the inclusive in-chunk cumulative sum of dt A:
//   ssd_chunk_state_kernel    cs, and S_c = sum_j exp(cs_last - cs_j) dt_j x_j (x) B_j
//   ssd_state_passing_kernel  prev_c = state entering chunk c (bf16), final state
//   ssd_chunk_scan_kernel     y_i = exp(cs_i) C_i . prev_c
//                                 + sum_{j <= i} (C_i . B_j) exp(cs_i - cs_j) dt_j x_j + D x_i
// Rows at or past l are read as zero (dt = 0: decay 1, contribution 0) and
// never stored.  No atomics, no host reads, grids depend on shapes only.
//
// Both MFMA kernels run one 512-thread block per (batch, chunk, head) on a 1-D
// grid through attn_block_map with the (batch, chunk, group) triples as its
// groups, so the heads that share one B/C tile run back to back on one XCD.
// Tiles are row-major swizzled LDS tiles read with the helpers of
// attention_tile.h; nothing is ever stored transposed.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "attention_tile.h"
#include "attention_sched.h"

namespace {

constexpr int SSD_Q = 128;  // chunk length of the kernels

struct SsdBlock { int batch, chunk, head, grp; };

// (batch, chunk, head) of workgroup `id`; false for a padding slot of the grid
__device__ __forceinline__ bool ssd_block(int id, int b, int nc, int g, int rep, SsdBlock& o) {
  const AttnBlock ab = attn_block_map(id, 1, b * nc * g, rep, false);
  if (ab.blk < 0) return false;
  const int grp_lin = ab.head / rep;
  o.grp = grp_lin % g;
  o.head = o.grp * rep + ab.head % rep;
  o.chunk = (grp_lin / g) % nc;
  o.batch = grp_lin / g / nc;
  return true;
}

__device__ __forceinline__ float load_dt(const void* dt, long idx, int dt_bf16) {
  return dt_bf16 ? sbf2f(reinterpret_cast<const short*>(dt)[idx]) : reinterpret_cast<const float*>(dt)[idx];
}

// Reg-staged copy of one [KVBLK][D] row-major tile (rows r0.. of `base`, row
// stride `srow` elements, rows >= rend read as zero) into swizzled LDS by a
// 512-thread block: loads() early, writes() late.  writes_scaled multiplies
// tile row r by w[r] in fp32 on the way.
template <int D>
struct RowStager {
  static constexpr int KCH = D / 8;
  static constexpr int SREG = KVBLK * D / 8 / 512;
  int row[SREG], c8[SREG];
  short8 reg[SREG];

  __device__ __forceinline__ RowStager() {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int idx = (int)threadIdx.x + i * 512;
      row[i] = idx / KCH;
      c8[i] = idx % KCH;
    }
  }
  __device__ __forceinline__ void loads(const bf16* base, long srow, int r0, int rend) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int r = r0 + row[i];
      reg[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < rend) reg[i] = *reinterpret_cast<const short8*>(base + (long)r * srow + c8[i] * 8);
    }
  }
  __device__ __forceinline__ void writes(short (*T)[D]) const {
#pragma unroll
    for (int i = 0; i < SREG; ++i)
      *reinterpret_cast<short8*>(&T[row[i]][swz<D>(row[i], c8[i]) * 8]) = reg[i];
  }
  __device__ __forceinline__ void writes_scaled(short (*T)[D], const float* w) const {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const float s = w[row[i]];
      int4 v;
      v.x = pack_bf16x2(sbf2f(reg[i][0]) * s, sbf2f(reg[i][1]) * s);
      v.y = pack_bf16x2(sbf2f(reg[i][2]) * s, sbf2f(reg[i][3]) * s);
      v.z = pack_bf16x2(sbf2f(reg[i][4]) * s, sbf2f(reg[i][5]) * s);
      v.w = pack_bf16x2(sbf2f(reg[i][6]) * s, sbf2f(reg[i][7]) * s);
      *reinterpret_cast<int4*>(&T[row[i]][swz<D>(row[i], c8[i]) * 8]) = v;
    }
  }
};

struct SsdArgs {
  const bf16 *x, *B, *C;
  const void* dt;
  const float *A, *D;
  long x_sb, x_sl, B_sb, B_sl, C_sb, C_sl, dt_sb, dt_sl;  // batch / row strides in elements
  int b, l, h, g, nc, dt_bf16;
};

// ---------------------------------------------------------------------------
// chunk states.  S_c[p][n] = sum_j (w_j x_j[p]) B_j[n], w_j = exp(cs_last - cs_j) dt_j.
// The reduction runs over tile rows for both operands: A-fragments (rows p)
// and B-fragments (columns n) are both transposing reads, of the scaled X tile
// and of the B tile.  Wave w owns the 16 p rows of block w % (P/16) and
// N*P/2048 of the 16-column n blocks.
// ---------------------------------------------------------------------------
template <int P, int N>
__global__ __launch_bounds__(512) void ssd_chunk_state_kernel(SsdArgs a, float* __restrict__ cs_ws,
                                                              float* __restrict__ states) {
  constexpr int PB = P / 16, NB = N * P / 2048;

  __shared__ __align__(16) short X_lds[KVBLK][P];
  __shared__ __align__(16) short B_lds[KVBLK][N];
  __shared__ float w_lds[SSD_Q];
  __shared__ float tot_lds[2];

  SsdBlock sb;
  if (!ssd_block(blockIdx.x, a.b, a.nc, a.g, a.h / a.g, sb)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int c0 = sb.chunk * SSD_Q;

  // inclusive cumulative sum of dt A over the chunk: waves 0 and 1 scan 64
  // rows each, wave 1 adds wave 0's total
  float dtv = 0.f, v = 0.f;
  if (tid < SSD_Q && c0 + tid < a.l) {
    dtv = load_dt(a.dt, sb.batch * a.dt_sb + (long)(c0 + tid) * a.dt_sl + sb.head, a.dt_bf16);
    v = dtv * a.A[sb.head];
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  if (tid == 63) tot_lds[0] = v;
  if (tid == 127) tot_lds[1] = v;
  __syncthreads();
  if (tid < SSD_Q) {
    if (tid >= 64) v += tot_lds[0];
    const float cs_last = tot_lds[1] + tot_lds[0];
    w_lds[tid] = __expf(cs_last - v) * dtv;
    cs_ws[(((long)sb.batch * a.h + sb.head) * a.nc + sb.chunk) * SSD_Q + tid] = v;
  }

  const bf16* xbase = a.x + sb.batch * a.x_sb + (long)sb.head * P;
  const bf16* bbase = a.B + sb.batch * a.B_sb + (long)sb.grp * N;
  const int pb = wid % PB, nb0 = (wid / PB) * NB;
  const int trbP = tr_lane_base<P>(g, c), trbN = tr_lane_base<N>(g, c);

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  RowStager<P> sx;
  RowStager<N> sbt;
  const int ntile = (min(SSD_Q, a.l - c0) + KVBLK - 1) / KVBLK;
  for (int tile = 0; tile < ntile; ++tile) {
    sx.loads(xbase, a.x_sl, c0 + tile * KVBLK, a.l);
    sbt.loads(bbase, a.B_sl, c0 + tile * KVBLK, a.l);
    __syncthreads();  // w_lds written (tile 0); previous tile's reads done (tile 1)
    sx.writes_scaled(X_lds, w_lds + tile * KVBLK);
    sbt.writes(B_lds);
    __syncthreads();
#pragma unroll
    for (int ks2 = 0; ks2 < KVBLK / 32; ++ks2) {
      const bf16x8 xa = read_b_tr<P>(&X_lds[0][0], trbP, ks2 * 32, pb);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            xa, read_b_tr<N>(&B_lds[0][0], trbN, ks2 * 32, nb0 + nb), acc[nb], 0, 0, 0);
    }
  }

  float* out = states + (((long)sb.batch * a.nc + sb.chunk) * a.h + sb.head) * (P * N);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      out[(pb * 16 + g * 4 + r) * N + (nb0 + nb) * 16 + c] = acc[nb][r];
}

// ---------------------------------------------------------------------------
// state passing: carry = carry * exp(cs_last of chunk) + S_c, sequential over
// the chunks, 8 state elements per thread.  prev[c] is the state entering
// chunk c, in bf16 as the scan kernel's MFMA consumes it.
// ---------------------------------------------------------------------------
__global__ void ssd_state_passing_kernel(const float* __restrict__ states, const float* __restrict__ cs_ws,
                                         const float* __restrict__ init, short* __restrict__ prev,
                                         float* __restrict__ final_state, int h, int nc, long pn, long total8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total8; i += (long)gridDim.x * blockDim.x) {
    const long e = i * 8, bh = e / pn, off = e % pn;
    const long bi = bh / h, hi = bh % h;
    float4v lo = float4v{0.f, 0.f, 0.f, 0.f}, hi4 = lo;
    if (init != nullptr) {
      lo = *reinterpret_cast<const float4v*>(init + e);
      hi4 = *reinterpret_cast<const float4v*>(init + e + 4);
    }
    for (int cidx = 0; cidx < nc; ++cidx) {
      const long base = ((bi * nc + cidx) * h + hi) * pn + off;
      int4 pk;
      pk.x = pack_bf16x2(lo[0], lo[1]);
      pk.y = pack_bf16x2(lo[2], lo[3]);
      pk.z = pack_bf16x2(hi4[0], hi4[1]);
      pk.w = pack_bf16x2(hi4[2], hi4[3]);
      *reinterpret_cast<int4*>(prev + base) = pk;
      const float d = __expf(cs_ws[(bh * nc + cidx) * SSD_Q + SSD_Q - 1]);
      lo = lo * d + *reinterpret_cast<const float4v*>(states + base);
      hi4 = hi4 * d + *reinterpret_cast<const float4v*>(states + base + 4);
    }
    *reinterpret_cast<float4v*>(final_state + e) = lo;
    *reinterpret_cast<float4v*>(final_state + e + 4) = hi4;
  }
}

// ---------------------------------------------------------------------------
// chunk scan: wave w owns output rows 16w..16w+15 of the chunk.
//   acc  = mfma(A=C_regs, B=prev tile [p][n], direct b128 reads)   D[i][p], then * exp(cs_i)
//   S^T  = mfma(A=B_lds (tile_row_a rows), B=C_regs)               D[j][i]
//   acc += mfma(A=P (own D-fragments), B=X_lds via transposing read)
// The C rows of a wave are the A-fragments of the first product and the
// B-fragments of the second in the same registers, so C never goes to LDS.
// ---------------------------------------------------------------------------
template <int P, int N>
__global__ __launch_bounds__(512) void ssd_chunk_scan_kernel(SsdArgs a, const float* __restrict__ cs_ws,
                                                             const short* __restrict__ prev,
                                                             bf16* __restrict__ y) {
  constexpr int ND = P / 16, NKN = N / 32;

  __shared__ __align__(16) short B_lds[2][KVBLK][N];
  __shared__ __align__(16) short X_lds[2][KVBLK][P];
  __shared__ __align__(16) short S_lds[P][N];
  __shared__ float cs_lds[SSD_Q], dt_lds[SSD_Q];

  SsdBlock sb;
  if (!ssd_block(blockIdx.x, a.b, a.nc, a.g, a.h / a.g, sb)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int c0 = sb.chunk * SSD_Q;
  const int rows = min(SSD_Q, a.l - c0);  // valid rows of this chunk, >= 1
  const int ntile = (rows + KVBLK - 1) / KVBLK;
  const int i0 = wid * 16;                // first in-chunk row of this wave
  const bool wave_live = i0 < rows;
  const int diag_tile = i0 / KVBLK;

  const bf16* xbase = a.x + sb.batch * a.x_sb + (long)sb.head * P;
  const bf16* bbase = a.B + sb.batch * a.B_sb + (long)sb.grp * N;
  const bf16* cbase = a.C + sb.batch * a.C_sb + (long)sb.grp * N;
  const int trbP = tr_lane_base<P>(g, c);

  RowStager<N> sbt;
  RowStager<P> sx;
  sbt.loads(bbase, a.B_sl, c0, a.l);
  sx.loads(xbase, a.x_sl, c0, a.l);

  // this wave's C rows: lane (g, c) holds row i0 + c, columns 32 ks + 8 g ..+7
  bf16x8 cfr[NKN];
  {
    const int row = c0 + i0 + c;
#pragma unroll
    for (int ks = 0; ks < NKN; ++ks) {
      short8 z = short8{0, 0, 0, 0, 0, 0, 0, 0};
      cfr[ks] = *reinterpret_cast<bf16x8*>(&z);
      if (row < a.l) cfr[ks] = load_frag(cbase + (long)row * a.C_sl + ks * 32 + g * 8);
    }
  }

  if (tid < SSD_Q) {
    cs_lds[tid] = cs_ws[(((long)sb.batch * a.h + sb.head) * a.nc + sb.chunk) * SSD_Q + tid];
    dt_lds[tid] = (c0 + tid < a.l)
        ? load_dt(a.dt, sb.batch * a.dt_sb + (long)(c0 + tid) * a.dt_sl + sb.head, a.dt_bf16) : 0.f;
  }
  {
    // state entering the chunk: contiguous [P][N] bf16 -> swizzled tile
    const short* src = prev + (((long)sb.batch * a.nc + sb.chunk) * a.h + sb.head) * (P * N);
#pragma unroll
    for (int i = 0; i < P * N / 8 / 512; ++i) {
      const int idx = tid + i * 512, row = idx / (N / 8), c8 = idx % (N / 8);
      *reinterpret_cast<short8*>(&S_lds[row][swz<N>(row, c8) * 8]) =
          *reinterpret_cast<const short8*>(src + (long)idx * 8);
    }
  }
  sbt.writes(B_lds[0]);
  sx.writes(X_lds[0]);
  __syncthreads();

  const float cs_i = cs_lds[i0 + c];  // row of the S^T column this lane holds

  // ---- off-diagonal term: exp(cs_i) C_i . prev ----
  f32x4 acc[ND];
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) {
    acc[nd] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKN; ++ks)
      acc[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          cfr[ks], read_a<N>(S_lds, nd * 16 + c, ks * 4 + g), acc[nd], 0, 0, 0);
  }
  __builtin_amdgcn_s_setprio(0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float e = __expf(cs_lds[i0 + g * 4 + r]);
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) acc[nd][r] *= e;
  }

  // ---- diagonal term over the B/X tiles at or below this wave's rows ----
  for (int tile = 0; tile < ntile; ++tile) {
    const int cur = tile & 1;
    const bool have_next = tile + 1 < ntile;
    if (have_next) {
      sbt.loads(bbase, a.B_sl, c0 + (tile + 1) * KVBLK, a.l);
      sx.loads(xbase, a.x_sl, c0 + (tile + 1) * KVBLK, a.l);
    }

    if (wave_live && tile <= diag_tile) {
      const bool masked = tile == diag_tile;
      int pk[KVBLK / 16][2];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int n = 0; n < KVBLK / 16; ++n) {
        f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
        const int jrow = tile_row_a(n, c);
#pragma unroll
        for (int ks = 0; ks < NKN; ++ks)
          st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_a<N>(B_lds[cur], jrow, ks * 4 + g), cfr[ks], st, 0, 0, 0);
        // D-layout [j = tile_row_d(n, g, r)][i = c].  Above the diagonal the
        // exponent is positive and may overflow: select, never multiply by 0.
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = tile * KVBLK + tile_row_d(n, g, r);
          const float pv = st[r] * (__expf(cs_i - cs_lds[j]) * dt_lds[j]);
          p[r] = (masked && j > i0 + c) ? 0.f : pv;
        }
        pk[n][0] = pack_bf16x2(p[0], p[1]);
        pk[n][1] = pack_bf16x2(p[2], p[3]);
      }
#pragma unroll
      for (int ks2 = 0; ks2 < KVBLK / 32; ++ks2) {
        const bf16x8 pa = own_a_frag(pk[2 * ks2], pk[2 * ks2 + 1]);
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
          acc[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pa, read_b_tr<P>(&X_lds[cur][0][0], trbP, ks2 * 32, nd), acc[nd], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (have_next) {
      // the other buffer has not been read yet: a chunk has two tiles
      __builtin_amdgcn_s_waitcnt(WAIT_VM0);
      __builtin_amdgcn_sched_barrier(0);
      sbt.writes(B_lds[cur ^ 1]);
      sx.writes(X_lds[cur ^ 1]);
      __syncthreads();
    }
  }

  // ---- epilogue: + D x (bf16 widened), one rounding to bf16 ----
  const float dskip = (a.D != nullptr) ? a.D[sb.head] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = c0 + i0 + g * 4 + r;
    if (row >= a.l) continue;
    const bf16* xr = xbase + (long)row * a.x_sl;
    bf16* yr = y + (((long)sb.batch * a.l + row) * a.h + sb.head) * P;
#pragma unroll
    for (int nd = 0; nd < ND; ++nd)
      yr[nd * 16 + c] = f2bf(acc[nd][r] + dskip * bf2f(xr[nd * 16 + c]));
  }
}

// ---------------------------------------------------------------------------
// decode step: state = state * exp(dt A) + dt x (x) B in place, y = state . C
// + D x.  A lane holds 4 consecutive n of one p row (16-byte state accesses),
// N/4 lanes span a row, a wave takes 64/(N/4) rows per pass and 16 rows in
// all; one 256-thread block covers 64 p rows of one (batch, head).
// ---------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void ssd_step_kernel(
    const bf16* __restrict__ x, const void* __restrict__ dt, const float* __restrict__ A,
    const bf16* __restrict__ B, const bf16* __restrict__ C, const float* __restrict__ D,
    float* __restrict__ state, bf16* __restrict__ y,
    long x_sb, long B_sb, long C_sb, long dt_sb, int h, int g, int p, int dt_bf16) {
  constexpr int LPR = N / 4, RPP = 64 / LPR;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int pblk = p / 64;
  const int bh = blockIdx.x / pblk;
  const int bi = bh / h, hi = bh % h, gi = hi / (h / g);
  const int n0 = (lane % LPR) * 4, rsub = lane / LPR;
  const int p0 = (blockIdx.x % pblk) * 64 + wid * 16;

  const float dtv = load_dt(dt, bi * dt_sb + hi, dt_bf16);
  const float dA = __expf(dtv * A[hi]);
  const float dskip = (D != nullptr) ? D[hi] : 0.f;
  const short4v bv = *reinterpret_cast<const short4v*>(B + bi * B_sb + (long)gi * N + n0);
  const short4v cv = *reinterpret_cast<const short4v*>(C + bi * C_sb + (long)gi * N + n0);
  float bf[4], cf[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { bf[k] = sbf2f(bv[k]); cf[k] = sbf2f(cv[k]); }

  const bf16* xr = x + bi * x_sb + (long)hi * p;
  float* srow = state + ((long)bh * p) * N + n0;
#pragma unroll
  for (int pass = 0; pass < 16 / RPP; ++pass) {
    const int pi = p0 + pass * RPP + rsub;
    const float xv = bf2f(xr[pi]);
    const float dx = dtv * xv;
    float4v s = *reinterpret_cast<float4v*>(srow + (long)pi * N);
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] = s[k] * dA + dx * bf[k];
      part += s[k] * cf[k];
    }
    *reinterpret_cast<float4v*>(srow + (long)pi * N) = s;
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane % LPR == 0) y[(long)bh * p + pi] = f2bf(part + dskip * xv);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// rows of 16-byte-aligned contiguous [.., inner] data behind arbitrary outer
// strides, as the kernels' 16-byte loads need; anything else is copied
torch::Tensor rows16(const torch::Tensor& t, int inner_dims) {
  bool ok = reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  int64_t expect = 1;
  for (int d = t.dim() - 1; d >= 0; --d) {
    if (d >= t.dim() - inner_dims) ok = ok && (t.size(d) == 1 || t.stride(d) == expect);
    else ok = ok && t.stride(d) % 8 == 0;
    expect *= t.size(d);
  }
  return ok ? t : t.contiguous();
}

template <int P, int N>
void launch_scan(hipStream_t stream, const SsdArgs& a, float* cs, float* states, short* prev,
                 const float* init, float* final_state, bf16* y) {
  const int grid = attn_sched_grid(1, a.b * a.nc * a.g, a.h / a.g);
  hipLaunchKernelGGL((ssd_chunk_state_kernel<P, N>), dim3(grid), dim3(512), 0, stream, a, cs, states);
  const long total8 = (long)a.b * a.h * P * N / 8;
  hipLaunchKernelGGL(ssd_state_passing_kernel, dim3(grid_for(total8, 256)), dim3(256), 0, stream,
                     (const float*)states, (const float*)cs, init, prev, final_state, a.h, a.nc,
                     (long)P * N, total8);
  hipLaunchKernelGGL((ssd_chunk_scan_kernel<P, N>), dim3(grid), dim3(512), 0, stream, a,
                     (const float*)cs, (const short*)prev, y);
}

void check_common(const torch::Tensor& x, const torch::Tensor& dt, const torch::Tensor& A,
                  const torch::Tensor& B, const torch::Tensor& C, const c10::optional<torch::Tensor>& D,
                  int h, int p, int g, int n, const char* who) {
  TORCH_CHECK(x.is_cuda() && dt.is_cuda() && A.is_cuda() && B.is_cuda() && C.is_cuda(), who, ": device tensors only");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && B.dtype() == torch::kBFloat16 && C.dtype() == torch::kBFloat16,
              who, ": x, B and C are bf16");
  TORCH_CHECK(dt.dtype() == torch::kBFloat16 || dt.dtype() == torch::kFloat32, who, ": dt is bf16 or f32");
  TORCH_CHECK((p == 64 || p == 128) && (n == 64 || n == 128), who, ": head dim and state dim must be 64 or 128");
  TORCH_CHECK(g > 0 && h % g == 0, who, ": heads must be a multiple of the B/C groups");
  TORCH_CHECK(B.sizes() == C.sizes(), who, ": B and C differ in shape");
  TORCH_CHECK(A.dtype() == torch::kFloat32 && A.dim() == 1 && A.size(0) == h, who, ": A is f32 [h]");
  if (D.has_value())
    TORCH_CHECK(D->is_cuda() && D->dtype() == torch::kFloat32 && D->dim() == 1 && D->size(0) == h, who, ": D is f32 [h]");
}

}  // namespace

std::vector<torch::Tensor> ssd_scan_fwd(torch::Tensor x, torch::Tensor dt, torch::Tensor A, torch::Tensor B,
                                        torch::Tensor C, c10::optional<torch::Tensor> D,
                                        c10::optional<torch::Tensor> initial_state) {
  TORCH_CHECK(x.dim() == 4 && dt.dim() == 3 && B.dim() == 4 && C.dim() == 4, "ssd_scan: x [b,l,h,p], dt [b,l,h], B/C [b,l,g,n]");
  const int b = x.size(0), l = x.size(1), h = x.size(2), p = x.size(3), g = B.size(2), n = B.size(3);
  check_common(x, dt, A, B, C, D, h, p, g, n, "ssd_scan");
  TORCH_CHECK(b > 0 && l > 0 && B.size(0) == b && B.size(1) == l && dt.size(0) == b && dt.size(1) == l && dt.size(2) == h,
              "ssd_scan: batch, length or head counts differ");
  auto xc = rows16(x, 2), Bc = rows16(B, 2), Cc = rows16(C, 2);
  auto dtc = dt.stride(2) == 1 ? dt : dt.contiguous();
  auto Ac = A.contiguous();
  torch::Tensor Dc, init;
  if (D.has_value()) Dc = D->contiguous();
  if (initial_state.has_value()) {
    TORCH_CHECK(initial_state->is_cuda() && initial_state->dtype() == torch::kFloat32 &&
                initial_state->sizes() == torch::IntArrayRef({b, h, p, n}), "ssd_scan: initial_state is f32 [b,h,p,n]");
    init = initial_state->contiguous();
  }

  const int nc = (l + SSD_Q - 1) / SSD_Q;
  auto f32 = x.options().dtype(torch::kFloat32);
  auto y = torch::empty({b, l, h, p}, x.options());
  auto final_state = torch::empty({b, h, p, n}, f32);
  auto cs = torch::empty({b, h, nc, SSD_Q}, f32);
  auto states = torch::empty({b, nc, h, p, n}, f32);
  auto prev = torch::empty({b, nc, h, p, n}, x.options());

  SsdArgs a;
  a.x = (const bf16*)xc.data_ptr(); a.B = (const bf16*)Bc.data_ptr(); a.C = (const bf16*)Cc.data_ptr();
  a.dt = dtc.data_ptr(); a.A = Ac.data_ptr<float>(); a.D = D.has_value() ? Dc.data_ptr<float>() : nullptr;
  a.x_sb = xc.stride(0); a.x_sl = xc.stride(1); a.B_sb = Bc.stride(0); a.B_sl = Bc.stride(1);
  a.C_sb = Cc.stride(0); a.C_sl = Cc.stride(1); a.dt_sb = dtc.stride(0); a.dt_sl = dtc.stride(1);
  a.b = b; a.l = l; a.h = h; a.g = g; a.nc = nc; a.dt_bf16 = dt.dtype() == torch::kBFloat16;

  auto stream = at::cuda::getCurrentHIPStream();
  const float* ip = initial_state.has_value() ? init.data_ptr<float>() : nullptr;
  float* csp = cs.data_ptr<float>();
  float* sp = states.data_ptr<float>();
  short* pp = (short*)prev.data_ptr();
  float* fp = final_state.data_ptr<float>();
  bf16* yp = (bf16*)y.data_ptr();
  if (p == 64 && n == 64) launch_scan<64, 64>(stream, a, csp, sp, pp, ip, fp, yp);
  else if (p == 64) launch_scan<64, 128>(stream, a, csp, sp, pp, ip, fp, yp);
  else if (n == 64) launch_scan<128, 64>(stream, a, csp, sp, pp, ip, fp, yp);
  else launch_scan<128, 128>(stream, a, csp, sp, pp, ip, fp, yp);
  return {y, final_state};
}

torch::Tensor ssd_step_fwd(torch::Tensor x, torch::Tensor dt, torch::Tensor A, torch::Tensor B, torch::Tensor C,
                           torch::Tensor state, c10::optional<torch::Tensor> D) {
  TORCH_CHECK(x.dim() == 3 && dt.dim() == 2 && B.dim() == 3 && C.dim() == 3, "ssd_step: x [b,h,p], dt [b,h], B/C [b,g,n]");
  const int b = x.size(0), h = x.size(1), p = x.size(2), g = B.size(1), n = B.size(2);
  check_common(x, dt, A, B, C, D, h, p, g, n, "ssd_step");
  TORCH_CHECK(b > 0 && B.size(0) == b && dt.size(0) == b && dt.size(1) == h, "ssd_step: batch or head counts differ");
  TORCH_CHECK(state.is_cuda() && state.dtype() == torch::kFloat32 && state.is_contiguous() &&
              state.sizes() == torch::IntArrayRef({b, h, p, n}), "ssd_step: state is contiguous f32 [b,h,p,n]");
  auto xc = rows16(x, 2), Bc = rows16(B, 2), Cc = rows16(C, 2);
  auto dtc = dt.stride(1) == 1 ? dt : dt.contiguous();
  auto Ac = A.contiguous();
  torch::Tensor Dc;
  if (D.has_value()) Dc = D->contiguous();
  auto y = torch::empty({b, h, p}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  const dim3 grid(b * h * (p / 64));
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream,
                       (const bf16*)xc.data_ptr(), (const void*)dtc.data_ptr(), (const float*)Ac.data_ptr<float>(),
                       (const bf16*)Bc.data_ptr(), (const bf16*)Cc.data_ptr(),
                       D.has_value() ? (const float*)Dc.data_ptr<float>() : (const float*)nullptr,
                       state.data_ptr<float>(), (bf16*)y.data_ptr(),
                       (long)xc.stride(0), (long)Bc.stride(0), (long)Cc.stride(0), (long)dtc.stride(0),
                       h, g, p, (int)(dt.dtype() == torch::kBFloat16));
  };
  if (n == 64) launch(ssd_step_kernel<64>);
  else launch(ssd_step_kernel<128>);
  return y;
}
