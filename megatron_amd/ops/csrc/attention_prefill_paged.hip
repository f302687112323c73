// Paged prefill attention for CDNA4: one request's chunk of s new query rows
// at absolute positions prior_len .. prior_len + s - 1 against keys and values
// 0 .. prior_len + s - 1 read in place from the paged KV cache through the
// request's block table (chunked prefill, prefix-cache hits, fp8 cache).
//
// Layout: q [s, hq, d] bf16; k/v cache [num_blocks, block_size, hkv, d] bf16
// or e4m3 (then with one f32 scale per (slot, head)); block_table [width]
// int64; out [s, hq, d] bf16.  d in {64, 128}, hq a multiple of hkv,
// block_size a multiple of 16, prior_len + s <= width * block_size.  The mask
// of q row i is  max(0, prior_len + i - window + 1) <= col <= prior_len + i.
//
// Structure (the packed forward of attention_varlen.hip, fed from pages):
//   * A 512-thread block handles PF_QBLK = 256 q rows of one q head; each of
//     the 8 waves owns 32 rows.  1-D grid through attn_block_map with
//     nblk = ceil(s / 256), ngrp = hkv, rep = hq / hkv, heavy_last: a block's
//     kv range ends at prior_len + q0 + 256, so work grows with the block
//     index; the heads of a kv group share an XCD and its L2.  prior_len is a
//     host int (prefill is not graph-captured), so the grid and every tile
//     range depend on it.
//   * PagedStager: tile row j of a 64-row tile is token k0 + j at cache slot
//     table[(k0 + j) / block_size] * block_size + (k0 + j) % block_size; the
//     table entry is looked up once per thread and tile row and ids outside
//     the cache are clamped.  16-byte (e4m3: 8-byte) global loads into
//     registers early, swizzled row-major LDS writes late, two buffers, one
//     barrier per tile.  Tokens at or past prior_len + s are never loaded:
//     their rows are written as zeros.
//   * e4m3 cache: the 8 values of a load widen to f32, are multiplied by the
//     row's scale and rounded to bf16 (nearest even) on the way to LDS - the
//     bits the gather path's dequantisation produces, so the MFMA operands are
//     the same and no scale is applied after the MFMA.
//   * S^T = mfma(A = K tile rows in tile_row_a order, B = Q regs)  D[kv][q];
//     the packed P D-fragments are the A-fragment of O += P V (own_a_frag), V
//     comes through the transposing read.  Online softmax in exp2 form with
//     the per-row defer-max of the packed forward.
//   * A block visits only the tiles its rows can see; a wave skips MFMA and
//     softmax work outside its own rows' range but still stages and takes the
//     barriers.  A tile is interior for a wave when its last column is at or
//     below the first row's diagonal and its first column is inside the last
//     row's window; only other tiles evaluate the mask (-1e30 before the max).
//     Every live row sees its own column, so no row is empty.
//   * No atomics, no workspace: the same inputs give the same bits.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <climits>
#include <type_traits>
#include "attention_tile.h"
#include "attention_sched.h"

#define RESCALE_THR 8.0f

namespace {

constexpr int PF_QT = 2;                // 16-row q sub-tiles per wave
constexpr int PF_QROWS = 16 * PF_QT;    // q rows per wave
constexpr int PF_QBLK = 8 * PF_QROWS;   // q rows per block

typedef float cvt_f2 __attribute__((ext_vector_type(2)));

// 8 cache elements as loaded (16 B of bf16 or 8 B of e4m3).
template <bool FP8> struct CacheVec { using type = short8; };
template <> struct CacheVec<true> { using type = int2; };

// what goes to LDS: bf16 as is; e4m3 as bf16(f32(x) * scale), nearest even
__device__ __forceinline__ short8 to_tile(short8 v, float) { return v; }
__device__ __forceinline__ short8 to_tile(int2 v, float s) {
  const cvt_f2 a = __builtin_amdgcn_cvt_pk_f32_fp8(v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(v.x, true);
  const cvt_f2 c = __builtin_amdgcn_cvt_pk_f32_fp8(v.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(v.y, true);
  int4 r = make_int4(pack_bf16x2(mul_rn(a[0], s), mul_rn(a[1], s)), pack_bf16x2(mul_rn(b[0], s), mul_rn(b[1], s)),
                     pack_bf16x2(mul_rn(c[0], s), mul_rn(c[1], s)), pack_bf16x2(mul_rn(d[0], s), mul_rn(d[1], s)));
  return *reinterpret_cast<short8*>(&r);
}

// Reg-staged copy of the [KVBLK][D] K and V tiles of tokens k0.. of one kv
// head out of the paged cache into swizzled LDS by a 512-thread block, shaped
// like TileStager: loads() early, writes() late.
template <int D, bool FP8>
struct PagedStager {
  static constexpr int KCH = D / 8;
  static constexpr int SREG = KVBLK * D / 8 / 512;
  using Vec = typename CacheVec<FP8>::type;
  using Elem = typename std::conditional<FP8, unsigned char, short>::type;

  const Elem *kc, *vc;
  const float *kscale, *vscale;
  const long* table;
  int block_size, num_blocks, hkv, head, kv_end;
  int row[SREG], c8[SREG];
  Vec rk[SREG], rv[SREG];
  float sk[SREG], sv[SREG];

  __device__ __forceinline__ PagedStager(const void* k, const void* v, const float* ks, const float* vs,
                                         const long* tbl, int bs, int nb, int hkv_, int head_, int kv_end_)
      : kc(reinterpret_cast<const Elem*>(k)), vc(reinterpret_cast<const Elem*>(v)), kscale(ks), vscale(vs),
        table(tbl), block_size(bs), num_blocks(nb), hkv(hkv_), head(head_), kv_end(kv_end_) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      int idx = (int)threadIdx.x + i * 512;
      row[i] = idx / KCH;
      c8[i] = idx % KCH;
    }
  }
  __device__ __forceinline__ void loads(int k0) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int tok = k0 + row[i];
      rk[i] = Vec{};
      rv[i] = Vec{};
      sk[i] = sv[i] = 0.f;
      if (tok < kv_end) {  // tok / block_size < width follows from the host check
        const int bi = tok / block_size;
        const long e = table[bi];
        // an id outside the cache (a corrupt table) is clamped, never followed
        const long blk = e < 0 ? 0 : (e >= num_blocks ? num_blocks - 1 : e);
        const long si = (blk * block_size + (tok - bi * block_size)) * hkv + head;
        rk[i] = *reinterpret_cast<const Vec*>(kc + si * D + c8[i] * 8);
        rv[i] = *reinterpret_cast<const Vec*>(vc + si * D + c8[i] * 8);
        if constexpr (FP8) {
          sk[i] = kscale[si];
          sv[i] = vscale[si];
        }
      }
    }
  }
  __device__ __forceinline__ void writes(short (*K)[D], short (*V)[D]) const {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      *reinterpret_cast<short8*>(&K[row[i]][swz<D>(row[i], c8[i]) * 8]) = to_tile(rk[i], sk[i]);
      *reinterpret_cast<short8*>(&V[row[i]][swz<D>(row[i], c8[i]) * 8]) = to_tile(rv[i], sv[i]);
    }
  }
};

// ---------------------------------------------------------------------------
// 8 waves x 32 q rows, kv tiles of 64 tokens.
//   S^T = mfma(A=K_lds, B=Q_regs)                 D[kv][q]
//   O  += mfma(A=P (own D-fragments), B=V_lds via transposing read)
// ---------------------------------------------------------------------------
template <int D, bool FP8>
__global__ __launch_bounds__(512) void attn_paged_prefill_kernel(
    const bf16* __restrict__ q, const void* __restrict__ kcache, const void* __restrict__ vcache,
    const float* __restrict__ kscale, const float* __restrict__ vscale, const long* __restrict__ table,
    bf16* __restrict__ o, int s, int prior, int hq, int hkv, int block_size, int num_blocks,
    int window, float scale, int nqc) {
  constexpr int QT = PF_QT, QROWS = PF_QROWS, QBLK = PF_QBLK;
  constexpr int ND = D / 16, NKD = D / 32;

  __shared__ __align__(16) short K_lds[2][KVBLK][D];
  __shared__ __align__(16) short V_lds[2][KVBLK][D];

  const int rep = hq / hkv;
  const AttnBlock ab = attn_block_map(blockIdx.x, nqc, hkv, rep, true);
  if (ab.blk < 0) return;  // padding slot of the grid
  const int head = ab.head;
  const int q0 = ab.blk * QBLK;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const long q_srow = (long)hq * D;
  const bf16* qbase = q + (long)head * D;
  bf16* obase = o + (long)head * D;

  const int row0 = q0 + wid * QROWS;
  const bool wave_live = row0 < s;
  const int trb = tr_lane_base<D>(g, c);

  // absolute column bounds (both inclusive) of this lane's rows row0 + 16*qt + c;
  // rows at or past s repeat the last row, load q as zero and are never stored
  int lo[QT], hi[QT];
  bf16x8 qb[QT][NKD];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int r = row0 + qt * 16 + c;
    hi[qt] = prior + min(r, s - 1);
    lo[qt] = hi[qt] - window + 1;
#pragma unroll
    for (int ks = 0; ks < NKD; ++ks) {
      short8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      qb[qt][ks] = *reinterpret_cast<bf16x8*>(&z);
      if (r < s) qb[qt][ks] = load_frag(qbase + (long)r * q_srow + ks * 32 + g * 8);
    }
  }
  // wave-uniform: diagonal of the first row, window start of the last row,
  // and the tiles the wave has any work in
  const int w_first = min(row0, s - 1), w_last = min(row0 + QROWS - 1, s - 1);
  const int hi_first = prior + w_first, lo_last = prior + w_last - window + 1;
  const int wt_first = max(0, hi_first - window + 1) / KVBLK, wt_last = (prior + w_last) / KVBLK;

  f32x4 oacc[QT][ND];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int n = 0; n < ND; ++n) oacc[qt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -1e30f; l_run[qt] = 0.f; }

  // block tile range: union over the waves (both bounds grow with the row)
  const int t_start = max(0, prior + q0 - window + 1) / KVBLK;
  const int t_end = (prior + min(q0 + QBLK, s) - 1) / KVBLK;

  const float c1 = scale * LOG2E;
  const float thr_raw = RESCALE_THR / scale;

  PagedStager<D, FP8> stg(kcache, vcache, kscale, vscale, table, block_size, num_blocks, hkv, head / rep, prior + s);
  stg.loads(t_start * KVBLK);
  stg.writes(K_lds[0], V_lds[0]);
  __syncthreads();

  for (int tile = t_start; tile <= t_end; ++tile) {
    const int k0 = tile * KVBLK;
    const int cur = (tile - t_start) & 1;
    const bool have_next = (tile + 1 <= t_end);
    if (have_next) stg.loads(k0 + KVBLK);

    if (wave_live && tile >= wt_first && tile <= wt_last) {
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
      if (!(k0 + KVBLK - 1 <= hi_first && k0 >= lo_last)) {
#pragma unroll
        for (int n = 0; n < KVBLK / 16; ++n)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int col = k0 + tile_row_d(n, g, r);
              if (col < lo[qt] || col > hi[qt]) st[n][qt][r] = -1e30f;
            }
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
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float inv = __shfl(linv, (lane & 48) + g * 4 + r, 64);
      const int orow_i = row0 + qt * 16 + g * 4 + r;
      if (orow_i >= s) continue;
      bf16* orow = obase + (long)orow_i * q_srow;
#pragma unroll
      for (int n = 0; n < ND; ++n) orow[n * 16 + c] = f2bf(oacc[qt][n][r] * inv);
    }
  }
}

template <int D, bool FP8>
void launch_prefill(hipStream_t stream, const torch::Tensor& q, const torch::Tensor& kc, const torch::Tensor& vc,
                    const float* ks, const float* vs, const torch::Tensor& table, torch::Tensor& out,
                    int s, int prior, int hq, int hkv, int window, float scale) {
  const int nqc = (s + PF_QBLK - 1) / PF_QBLK;
  hipLaunchKernelGGL((attn_paged_prefill_kernel<D, FP8>), dim3(attn_sched_grid(nqc, hkv, hq / hkv)), dim3(512), 0,
                     stream, (const bf16*)q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks, vs,
                     (const long*)table.data_ptr<int64_t>(), (bf16*)out.data_ptr(), s, prior, hq, hkv,
                     (int)kc.size(1), (int)kc.size(0), window, scale, nqc);
}

}  // namespace

// window <= 0: no sliding window.
torch::Tensor attn_paged_prefill(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                 torch::Tensor block_table, long prior_len, double scale, long window,
                                 c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale) {
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() && block_table.is_cuda(),
              "attn_paged_prefill: device tensors only");
  TORCH_CHECK(q.dim() == 3 && q.dtype() == torch::kBFloat16 && q.is_contiguous(), "attn_paged_prefill: q is contiguous bf16 [s, hq, d]");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes() && k_cache.dtype() == v_cache.dtype() &&
              k_cache.is_contiguous() && v_cache.is_contiguous(),
              "attn_paged_prefill: k/v cache are contiguous [num_blocks, block_size, hkv, d] of one dtype");
  const bool fp8 = k_cache.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || k_cache.dtype() == torch::kBFloat16, "attn_paged_prefill: cache is bf16 or float8_e4m3fn");
  const long s = q.size(0);
  const int hq = (int)q.size(1), d = (int)q.size(2);
  const long num_blocks = k_cache.size(0), block_size = k_cache.size(1);
  const int hkv = (int)k_cache.size(2);
  TORCH_CHECK(d == 64 || d == 128, "attn_paged_prefill: head dim must be 64 or 128");
  TORCH_CHECK(k_cache.size(3) == d && hkv > 0 && hq % hkv == 0, "attn_paged_prefill: hq must be a multiple of hkv");
  TORCH_CHECK(block_size > 0 && block_size % 16 == 0 && num_blocks > 0, "attn_paged_prefill: block_size must be a multiple of 16");
  TORCH_CHECK(block_table.dim() == 1 && block_table.dtype() == torch::kInt64 && block_table.size(0) > 0 &&
              block_table.is_contiguous(), "attn_paged_prefill: block_table is contiguous int64 [width]");
  const long width = block_table.size(0);
  TORCH_CHECK(s > 0 && prior_len >= 0 && prior_len + s <= width * block_size,
              "attn_paged_prefill: need s > 0, prior_len >= 0 and prior_len + s <= width * block_size");
  TORCH_CHECK(width * block_size < (1L << 31) && num_blocks * block_size < (1L << 31) && s * hq * d < (1L << 40) &&
              (long)attn_sched_grid((int)((s + PF_QBLK - 1) / PF_QBLK), hkv, hq / hkv) < (1L << 31),
              "attn_paged_prefill: shape out of range");
  TORCH_CHECK(scale > 0.0, "attn_paged_prefill: scale must be positive");
  const float *ks = nullptr, *vs = nullptr;
  if (fp8) {
    TORCH_CHECK(k_scale.has_value() && v_scale.has_value(), "attn_paged_prefill: an fp8 cache needs k_scale and v_scale");
    for (const auto& sc : {*k_scale, *v_scale})
      TORCH_CHECK(sc.is_cuda() && sc.dtype() == torch::kFloat32 && sc.is_contiguous() && sc.dim() == 2 &&
                  sc.size(0) == num_blocks * block_size && sc.size(1) == hkv,
                  "attn_paged_prefill: scales are contiguous f32 [num_blocks * block_size, hkv]");
    ks = k_scale->data_ptr<float>();
    vs = v_scale->data_ptr<float>();
  }

  // a window that reaches past position 0 for every row is no window
  const int win = (window <= 0 || window > prior_len + s) ? INT_MAX : (int)window;
  auto out = torch::empty_like(q);
  auto stream = at::cuda::getCurrentHIPStream();
  const float sc = (float)scale;
  const int si = (int)s, pi = (int)prior_len;
  if (d == 128 && fp8) launch_prefill<128, true>(stream, q, k_cache, v_cache, ks, vs, block_table, out, si, pi, hq, hkv, win, sc);
  else if (d == 128) launch_prefill<128, false>(stream, q, k_cache, v_cache, ks, vs, block_table, out, si, pi, hq, hkv, win, sc);
  else if (fp8) launch_prefill<64, true>(stream, q, k_cache, v_cache, ks, vs, block_table, out, si, pi, hq, hkv, win, sc);
  else launch_prefill<64, false>(stream, q, k_cache, v_cache, ks, vs, block_table, out, si, pi, hq, hkv, win, sc);
  return out;
}
