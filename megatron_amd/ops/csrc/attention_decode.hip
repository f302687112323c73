// Paged split-KV decode attention for CDNA4: one query token per request,
// read straight off the paged KV cache (flash-decoding).
//
// Layout: q [b, hq, d] bf16; k/v cache [num_blocks, block_size, hkv, d] bf16
// or e4m3 (then with one f32 scale per (slot, head)); block_tables [b, width]
// int64; lens [b] int64 (kv length including the token just written);
// out [b, hq, d] bf16.  d in {64, 128}, rep = hq / hkv <= 16, block_size a
// multiple of 16.
//
// Structure:
//   * One workgroup of 4 waves per (split, kv head, request).  The rep query
//     heads of the kv group are the columns of one MFMA 16x16x32 operand
//     (padded with zero rows up to 16, never stored), so every K/V byte is
//     fetched once per group.
//   * lens and block_tables are read on the device only; the grid and the
//     split length come from shapes (decode_splits), so a captured launch
//     replays with new table and length contents.  A split past lens[i]
//     returns at once.
//   * A wave streams the 32-token slices wid, wid + 4, .. of the split and
//     keeps its own (m, l, O) in the exp2 form of the other kernels; the four
//     waves merge once through LDS at the end.  The streaming loop has no
//     block barrier.
//   * S^T = mfma(A = K rows from 16-byte global loads, B = Q regs)  D[kv][q]
//     with the tile_row_a row permutation of attention_tile.h, so the packed
//     P D-fragments are the A-fragment of O += P V without a relayout.  V is
//     staged row-major swizzled into a wave-private LDS tile and read back
//     with the transposing read (read_b_tr).  The next slice's K and V are in
//     flight in registers while the current slice computes.
//   * Tokens at or past lens[i] are never loaded (zero registers) and their
//     scores are masked, so stale cache contents cannot reach the result.
//     Only slices with a live token are visited, so (m, l, O) never see an
//     all-masked slice; m starts at -1e30, not -inf.
//   * e4m3 cache: same body; elements widen to bf16 in registers (exact),
//     k_scale multiplies the score column after the MFMA, v_scale is folded
//     into the probability before it is packed (l sums the unscaled p).
//   * nsplit > 1: unnormalised (m, l, O) per split go to an f32 workspace and
//     attn_decode_combine_kernel merges the live splits in split order.  No
//     atomics anywhere: two runs give the same bits.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "attention_tile.h"

namespace {

constexpr int DEC_WAVES = 4;   // waves per workgroup
constexpr int DEC_SLICE = 32;  // tokens per wave step (one PV MFMA reduction)

typedef float cvt_f2 __attribute__((ext_vector_type(2)));

// 8 cache elements as loaded (16 B of bf16 or 8 B of e4m3) -> 8 bf16.
template <bool FP8> struct CacheVec { using type = short8; };
template <> struct CacheVec<true> { using type = int2; };

__device__ __forceinline__ bf16x8 widen(short8 v) { return *reinterpret_cast<bf16x8*>(&v); }
__device__ __forceinline__ bf16x8 widen(int2 v) {
  const cvt_f2 a = __builtin_amdgcn_cvt_pk_f32_fp8(v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(v.x, true);
  const cvt_f2 c = __builtin_amdgcn_cvt_pk_f32_fp8(v.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(v.y, true);
  int4 r = make_int4(pack_bf16x2(a[0], a[1]), pack_bf16x2(b[0], b[1]),
                     pack_bf16x2(c[0], c[1]), pack_bf16x2(d[0], d[1]));
  return *reinterpret_cast<bf16x8*>(&r);
}

__device__ __forceinline__ int clamped_len(const long* __restrict__ lens, int req, long cap) {
  const long l = lens[req];
  return (int)(l < 0 ? 0 : (l > cap ? cap : l));
}

template <int D, bool FP8>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_paged_decode_kernel(
    const bf16* __restrict__ q, const void* __restrict__ kcache, const void* __restrict__ vcache,
    const float* __restrict__ kscale, const float* __restrict__ vscale,
    const long* __restrict__ tables, long table_stride, const long* __restrict__ lens,
    bf16* __restrict__ out, float* __restrict__ part_o, float* __restrict__ part_ml,
    int hq, int hkv, int width, int block_size, int num_blocks, int split_tokens, int nsplit, float scale) {
  constexpr int ND = D / 16, NKD = D / 32, KCH = D / 8, VREG = DEC_SLICE * KCH / 64;
  using Vec = typename CacheVec<FP8>::type;
  using Elem = typename std::conditional<FP8, unsigned char, short>::type;

  // a wave's V tile; at the end the same bytes hold its O [16][D] f32
  __shared__ __align__(16) short V_lds[DEC_WAVES][DEC_SLICE][D];
  __shared__ float ml_lds[DEC_WAVES][16][2];
  static_assert(DEC_SLICE * D * 2 == 16 * D * 4, "O merge reuses the V tile");

  const int split = blockIdx.x, kvh = blockIdx.y, req = blockIdx.z;
  const int rep = hq / hkv;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;

  const int len = clamped_len(lens, req, (long)width * block_size);
  const int s_begin = split * split_tokens;
  const int s_end = min(len, s_begin + split_tokens);
  if (s_begin >= len) {
    // nothing to attend to; a single-split launch still owns the output
    if (nsplit == 1)
      for (int idx = threadIdx.x; idx < rep * D; idx += DEC_WAVES * 64)
        out[((long)req * hq + kvh * rep) * D + idx] = f2bf(0.f);
    return;
  }

  const Elem* kc = reinterpret_cast<const Elem*>(kcache);
  const Elem* vc = reinterpret_cast<const Elem*>(vcache);
  const long* tbl = tables + (long)req * table_stride;

  // Q as the B operand: column c = query head c of the group, zero past rep
  bf16x8 qb[NKD];
#pragma unroll
  for (int ks = 0; ks < NKD; ++ks) {
    short8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    qb[ks] = widen(z);
    if (c < rep) qb[ks] = load_frag(q + ((long)req * hq + kvh * rep + c) * D + ks * 32 + g * 8);
  }

  f32x4 oacc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) oacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;
  const float c1 = scale * LOG2E;

  // physical block of table entry bi, looked up once per block: the wave
  // keeps the last entry it read
  int last_bi = -1, last_blk = 0;
  auto block_of = [&](int bi) {
    if (bi != last_bi) {
      last_bi = bi;
      const long e = (bi < width) ? tbl[bi] : 0;
      // an id outside the cache (a corrupt table) is clamped, never followed
      last_blk = __builtin_amdgcn_readfirstlane((int)(e < 0 ? 0 : (e >= num_blocks ? num_blocks - 1 : e)));
    }
    return last_blk;
  };

  Vec kr[2][NKD], vr[VREG];
  float ksr[8], vsr[8];
  // one slice into registers: K rows in MFMA row order, V rows in tile order,
  // scales of tokens 8g..8g+7; tokens >= s_end stay zero
  auto load_slice = [&](int s0) {
    long slot_half[2];  // slot of the first token of each 16-token half
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t0 = s0 + 16 * h;
      const int bi = t0 / block_size;
      slot_half[h] = (t0 < s_end) ? (long)block_of(bi) * block_size + (t0 - bi * block_size) : 0;
    }
    const Vec zero = {};
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int tok = tile_row_a(n, c);
      const Elem* p = kc + ((slot_half[tok >> 4] + (tok & 15)) * hkv + kvh) * D + g * 8;
#pragma unroll
      for (int ks = 0; ks < NKD; ++ks)
        kr[n][ks] = (s0 + tok < s_end) ? *reinterpret_cast<const Vec*>(p + ks * 32) : zero;
    }
#pragma unroll
    for (int i = 0; i < VREG; ++i) {
      const int idx = lane + i * 64, row = idx / KCH, c8 = idx % KCH;
      const Elem* p = vc + ((slot_half[row >> 4] + (row & 15)) * hkv + kvh) * D + c8 * 8;
      vr[i] = (s0 + row < s_end) ? *reinterpret_cast<const Vec*>(p) : zero;
    }
    if constexpr (FP8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int tok = 8 * g + j;
        const long si = (slot_half[tok >> 4] + (tok & 15)) * hkv + kvh;
        const bool live = s0 + tok < s_end;
        ksr[j] = live ? kscale[si] : 0.f;
        vsr[j] = live ? vscale[si] : 0.f;
      }
    }
  };

  short (*Vw)[D] = V_lds[wid];
  const int trb = tr_lane_base<D>(g, c);
  const int step = DEC_WAVES * DEC_SLICE;
  int s0 = s_begin + wid * DEC_SLICE;
  if (s0 < s_end) load_slice(s0);

  for (; s0 < s_end; s0 += step) {
    // ---- current slice out of the staging registers: V to LDS, K widened ----
#pragma unroll
    for (int i = 0; i < VREG; ++i) {
      const int idx = lane + i * 64, row = idx / KCH, c8 = idx % KCH;
      bf16x8 w = widen(vr[i]);
      *reinterpret_cast<short8*>(&Vw[row][swz<D>(row, c8) * 8]) = *reinterpret_cast<short8*>(&w);
    }
    bf16x8 ka[2][NKD];
    float ks_cur[8], vs_cur[8];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int ks = 0; ks < NKD; ++ks) ka[n][ks] = widen(kr[n][ks]);
    if constexpr (FP8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { ks_cur[j] = ksr[j]; vs_cur[j] = vsr[j]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    // ---- next slice in flight while this one computes ----
    if (s0 + step < s_end) load_slice(s0 + step);

    // ---- S^T = K Q^T (raw scores); lane (g,c): q = c, kv = s0 + 8g + 4n + r ----
    f32x4 st[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      st[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKD; ++ks)
        st[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[n][ks], qb[ks], st[n], 0, 0, 0);
    }
    float pmax = -1e30f;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (FP8) st[n][r] *= ks_cur[4 * n + r];
        if (s0 + tile_row_d(n, g, r) >= s_end) st[n][r] = -1e30f;
        pmax = fmaxf(pmax, st[n][r]);
      }
    pmax = fmaxf(pmax, __shfl_xor(pmax, 16, 64));
    pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));

    // ---- online softmax; the slice has a live token, so pmax is a score ----
    const float m_new = fmaxf(m_run, pmax);
    const float alpha = exp2f((m_run - m_new) * c1);
    m_run = m_new;
    l_run *= alpha;
    // alpha lives in the q = c layout, O in the q = 4g + r layout
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = __shfl(alpha, (lane & 48) + g * 4 + r, 64);
#pragma unroll
      for (int n = 0; n < ND; ++n) oacc[n][r] *= a;
    }
    const float mc = m_run * c1;
    int pk[2][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sv = st[n][r];
        p[r] = (sv <= -1e29f) ? 0.f : exp2f(__builtin_fmaf(sv, c1, -mc));
        l_run += p[r];
        if constexpr (FP8) p[r] *= vs_cur[4 * n + r];
      }
      pk[n][0] = pack_bf16x2(p[0], p[1]);
      pk[n][1] = pack_bf16x2(p[2], p[3]);
    }

    // ---- O += P V ----
    const bf16x8 a = own_a_frag(pk[0], pk[1]);
#pragma unroll
    for (int n = 0; n < ND; ++n)
      oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, read_b_tr<D>(&Vw[0][0], trb, 0, n), oacc[n], 0, 0, 0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }

  // ---- merge the waves: O and (m, l) through LDS, one barrier ----
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  float* Ow = reinterpret_cast<float*>(&Vw[0][0]);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int n = 0; n < ND; ++n) Ow[(4 * g + r) * D + n * 16 + c] = oacc[n][r];
  if (g == 0) {
    ml_lds[wid][c][0] = m_run;
    ml_lds[wid][c][1] = l_run;
  }
  __syncthreads();

  for (int idx = threadIdx.x; idx < rep * D; idx += DEC_WAVES * 64) {
    const int row = idx / D, col = idx % D;
    float m_tot = -1e30f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) m_tot = fmaxf(m_tot, ml_lds[w][row][0]);
    float acc = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float wgt = exp2f((ml_lds[w][row][0] - m_tot) * c1);
      acc += reinterpret_cast<const float*>(&V_lds[w][0][0])[row * D + col] * wgt;
      l += ml_lds[w][row][1] * wgt;
    }
    const long oh = (long)req * hq + kvh * rep + row;
    if (nsplit == 1) {
      out[oh * D + col] = f2bf(l > 0.f ? acc / l : 0.f);
    } else {
      part_o[(oh * nsplit + split) * D + col] = acc;
      if (col == 0) {
        part_ml[(oh * nsplit + split) * 2] = m_tot;
        part_ml[(oh * nsplit + split) * 2 + 1] = l;
      }
    }
  }
}

// Merge the live splits of one (request, head) in split order; D threads.
__global__ void attn_decode_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                           const long* __restrict__ lens, bf16* __restrict__ out,
                                           int hq, int d, long cap, int split_tokens, int nsplit, float scale) {
  const int head = blockIdx.x, req = blockIdx.y, col = threadIdx.x;
  const int len = clamped_len(lens, req, cap);
  const int live = min(nsplit, (len + split_tokens - 1) / split_tokens);
  const long oh = (long)req * hq + head;
  const float* ml = part_ml + oh * nsplit * 2;
  const float c1 = scale * LOG2E;
  float m_tot = -1e30f;
  for (int s = 0; s < live; ++s) m_tot = fmaxf(m_tot, ml[2 * s]);
  float acc = 0.f, l = 0.f;
  for (int s = 0; s < live; ++s) {
    const float wgt = exp2f((ml[2 * s] - m_tot) * c1);
    acc += part_o[(oh * nsplit + s) * d + col] * wgt;
    l += ml[2 * s + 1] * wgt;
  }
  out[oh * d + col] = f2bf(l > 0.f ? acc / l : 0.f);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Tokens per KV split, from shapes only (nothing here may depend on lens: the
// launch is captured into graphs).  Aim at about two workgroups on each of
// the 256 CUs: b*hkv groups want 512 / (b*hkv) splits each, and one split
// once the groups alone fill the chip.  A split is a whole number of table
// blocks, a multiple of the 32-token slice, and at least one slice per wave.
int decode_split_tokens(int b, int hkv, int width, int block_size) {
  const long groups = (long)b * hkv;
  const int want = groups >= 256 ? 1 : (int)(512 / groups);
  int blocks = (width + want - 1) / want;
  const int min_blocks = (DEC_WAVES * DEC_SLICE + block_size - 1) / block_size;
  if (blocks < min_blocks) blocks = min_blocks;
  if ((blocks * block_size) % DEC_SLICE) ++blocks;
  return blocks * block_size;
}

template <int D, bool FP8>
void launch_decode(hipStream_t stream, const torch::Tensor& q, const torch::Tensor& kc, const torch::Tensor& vc,
                   const float* ks, const float* vs, const torch::Tensor& tables, const torch::Tensor& lens,
                   torch::Tensor& out, float* part_o, float* part_ml, int b, int hq, int hkv, int split_tokens,
                   int nsplit, float scale) {
  hipLaunchKernelGGL((attn_paged_decode_kernel<D, FP8>), dim3(nsplit, hkv, b), dim3(DEC_WAVES * 64), 0, stream,
                     (const bf16*)q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks, vs,
                     (const long*)tables.data_ptr<int64_t>(), (long)tables.stride(0),
                     (const long*)lens.data_ptr<int64_t>(), (bf16*)out.data_ptr(), part_o, part_ml,
                     hq, hkv, (int)tables.size(1), (int)kc.size(1), (int)kc.size(0), split_tokens, nsplit, scale);
}

}  // namespace

torch::Tensor attn_paged_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_tables, torch::Tensor lens, double scale,
                                c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale) {
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() && block_tables.is_cuda() && lens.is_cuda(),
              "attn_paged_decode: device tensors only");
  TORCH_CHECK(q.dim() == 3 && q.dtype() == torch::kBFloat16 && q.is_contiguous(), "attn_paged_decode: q is contiguous bf16 [b, hq, d]");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes() && k_cache.dtype() == v_cache.dtype() &&
              k_cache.is_contiguous() && v_cache.is_contiguous(),
              "attn_paged_decode: k/v cache are contiguous [num_blocks, block_size, hkv, d] of one dtype");
  const bool fp8 = k_cache.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || k_cache.dtype() == torch::kBFloat16, "attn_paged_decode: cache is bf16 or float8_e4m3fn");
  const int b = (int)q.size(0), hq = (int)q.size(1), d = (int)q.size(2);
  const long num_blocks = k_cache.size(0), block_size = k_cache.size(1);
  const int hkv = (int)k_cache.size(2);
  TORCH_CHECK(d == 64 || d == 128, "attn_paged_decode: head dim must be 64 or 128");
  TORCH_CHECK(k_cache.size(3) == d && hkv > 0 && hq % hkv == 0 && hq / hkv <= 16,
              "attn_paged_decode: hq must be a multiple of hkv, at most 16 query heads per kv head");
  TORCH_CHECK(block_size > 0 && block_size % 16 == 0 && num_blocks > 0, "attn_paged_decode: block_size must be a multiple of 16");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.dtype() == torch::kInt64 && block_tables.size(0) == b &&
              block_tables.size(1) > 0 && block_tables.stride(1) == 1, "attn_paged_decode: block_tables is int64 [b, width]");
  TORCH_CHECK(lens.dim() == 1 && lens.dtype() == torch::kInt64 && lens.size(0) == b && lens.is_contiguous(),
              "attn_paged_decode: lens is contiguous int64 [b]");
  const long width = block_tables.size(1);
  TORCH_CHECK(b > 0 && b < 65536 && hkv < 65536 && width * block_size < (1L << 31) && num_blocks * block_size < (1L << 31),
              "attn_paged_decode: shape out of range");
  TORCH_CHECK(scale > 0.0, "attn_paged_decode: scale must be positive");
  const float *ks = nullptr, *vs = nullptr;
  if (fp8) {
    TORCH_CHECK(k_scale.has_value() && v_scale.has_value(), "attn_paged_decode: an fp8 cache needs k_scale and v_scale");
    for (const auto& s : {*k_scale, *v_scale})
      TORCH_CHECK(s.is_cuda() && s.dtype() == torch::kFloat32 && s.is_contiguous() && s.dim() == 2 &&
                  s.size(0) == num_blocks * block_size && s.size(1) == hkv,
                  "attn_paged_decode: scales are contiguous f32 [num_blocks * block_size, hkv]");
    ks = k_scale->data_ptr<float>();
    vs = v_scale->data_ptr<float>();
  }

  const int split_tokens = decode_split_tokens(b, hkv, (int)width, (int)block_size);
  const int nsplit = (int)((width * block_size + split_tokens - 1) / split_tokens);
  auto out = torch::empty_like(q);
  torch::Tensor part_o, part_ml;
  float *po = nullptr, *pml = nullptr;
  if (nsplit > 1) {
    part_o = torch::empty({b, hq, nsplit, d}, q.options().dtype(torch::kFloat32));
    part_ml = torch::empty({b, hq, nsplit, 2}, q.options().dtype(torch::kFloat32));
    po = part_o.data_ptr<float>();
    pml = part_ml.data_ptr<float>();
  }
  auto stream = at::cuda::getCurrentHIPStream();
  const float sc = (float)scale;
  if (d == 128 && fp8) launch_decode<128, true>(stream, q, k_cache, v_cache, ks, vs, block_tables, lens, out, po, pml, b, hq, hkv, split_tokens, nsplit, sc);
  else if (d == 128) launch_decode<128, false>(stream, q, k_cache, v_cache, ks, vs, block_tables, lens, out, po, pml, b, hq, hkv, split_tokens, nsplit, sc);
  else if (fp8) launch_decode<64, true>(stream, q, k_cache, v_cache, ks, vs, block_tables, lens, out, po, pml, b, hq, hkv, split_tokens, nsplit, sc);
  else launch_decode<64, false>(stream, q, k_cache, v_cache, ks, vs, block_tables, lens, out, po, pml, b, hq, hkv, split_tokens, nsplit, sc);
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(hq, b), dim3(d), 0, stream, po, pml,
                       (const long*)lens.data_ptr<int64_t>(), (bf16*)out.data_ptr(), hq, d,
                       width * block_size, split_tokens, nsplit, sc);
  return out;
}
