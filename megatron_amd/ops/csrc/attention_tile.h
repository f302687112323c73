// LDS tile helpers shared by the attention kernels that consume row-major
// swizzled tiles through A-fragment b128 reads and transposing B-fragment
// reads (attention_bwd.hip, attention_varlen.hip): the tile height KVBLK,
// fragment reads (load_frag, read_a, read_b_tr, own_a_frag), the row
// permutation of the first phase, the DPP row broadcast, and the reg-staged
// tile copy TileStager.  attention_decode.hip uses the swizzle, the row
// permutation and read_b_tr on wave-private 32-row tiles.  The dense backward still stages with its own
// lambdas over separate arrays: moving it onto TileStager changes its
// register allocation (see profiles/README.md).
#pragma once

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));

#define LOG2E 1.44269504088896340736f
#define WAIT_VM0 0x0F70

constexpr int KVBLK = 64;  // rows of a streamed tile (kv rows in fwd/dq, q rows in dkv)

// 16-byte chunk swizzle of a row-major [rows][D] bf16 tile: chunk ^ swzf(row).
// LDS has 64 four-byte banks, so 256 B (one D=128 row, two D=64 rows) is one
// pass over the banks.  The term is chosen so that both read patterns of a
// tile touch every bank once per pass.  Write a row as 16A + 8a + 4h + e
// (e = row & 3, h = bit 2, a = bit 3, A = bit 4; h is the same for all
// lanes of either read):
//   * phase 1, b128: 16 lanes read the same logical chunk of the rows
//     (A, a, e) = all 16 combinations -> the term (D = 128) resp. the term
//     together with the row parity (D = 64) must differ for all of them;
//   * phase 2, transposing b64: 32 lanes read one 32-byte chunk pair of the
//     rows (a, e) = all 8 combinations at fixed A -> bits 1.. of the term
//     (with the row parity for D = 64) must differ for all of them.
template <int D>
__device__ __forceinline__ int swzf(int row) {
  const int lo = (D == 128) ? (row & 3) : ((row >> 1) & 1);
  return (lo << 2) | (((row >> 3) & 1) << 1) | ((row >> 4) & 1);
}
template <int D>
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ swzf<D>(row); }

// Reg-staged copy of two [KVBLK][D] row-major tiles (rows x0.. of a and b,
// row stride `srow` elements, rows >= t read as zero) into swizzled LDS by a
// 512-thread block: loads() early, writes() late.
template <int D>
struct TileStager {
  static constexpr int KCH = D / 8;
  static constexpr int SREG = KVBLK * D / 8 / 512;
  int row[SREG], c8[SREG];
  short8 ra[SREG], rb[SREG];

  __device__ __forceinline__ TileStager() {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      int idx = (int)threadIdx.x + i * 512;
      row[i] = idx / KCH;
      c8[i] = idx % KCH;
    }
  }
  __device__ __forceinline__ void loads(const bf16* a, const bf16* b, long srow, int x0, int t) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int r = x0 + row[i];
      ra[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      rb[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < t) {
        ra[i] = *reinterpret_cast<const short8*>(a + (long)r * srow + c8[i] * 8);
        rb[i] = *reinterpret_cast<const short8*>(b + (long)r * srow + c8[i] * 8);
      }
    }
  }
  __device__ __forceinline__ void writes(short (*A)[D], short (*B)[D]) const {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      *reinterpret_cast<short8*>(&A[row[i]][swz<D>(row[i], c8[i]) * 8]) = ra[i];
      *reinterpret_cast<short8*>(&B[row[i]][swz<D>(row[i], c8[i]) * 8]) = rb[i];
    }
  }
};

// A-fragment (8 bf16) of a first-phase MFMA: 16-byte chunk `chunk` of tile row
// `row`, and the same from global memory for the register-resident operand.
template <int D>
__device__ __forceinline__ bf16x8 read_a(const short (*tile)[D], int row, int chunk) {
  short8 tmp = *reinterpret_cast<const short8*>(&tile[row][swz<D>(row, chunk) * 8]);
  return *reinterpret_cast<bf16x8*>(&tmp);
}
__device__ __forceinline__ bf16x8 load_frag(const bf16* p) {
  short8 tmp = *reinterpret_cast<const short8*>(p);
  return *reinterpret_cast<bf16x8*>(&tmp);
}

// Transposing LDS read.  Within each group of 16 lanes, lane i supplies the
// address of 4 consecutive bf16: row i>>2, columns 4(i&3)..+3 of a 4x16
// block; lane c receives column c of that block (4 rows).
__device__ __forceinline__ short4v lds_read_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4v*)(p));
}

// Tile row that sub-tile n feeds into MFMA row i in phase 1, and tile row of
// element r of lane group g's D-fragment of sub-tile n: sub-tile n feeds MFMA
// row i with tile row 32(n>>1) + 8(i>>2) + 4(n&1) + (i&3), so the D-fragment
// of lane (g,c) holds column c at tile rows 32(n>>1)+8g+4(n&1)+r - over the
// sub-tile pair (2ks, 2ks+1) exactly the rows 32ks+8g..+7, in order, which is
// the A-fragment of the phase-2 MFMA in the natural k order.
__device__ __forceinline__ int tile_row_a(int n, int i) {
  return 32 * (n >> 1) + 8 * (i >> 2) + 4 * (n & 1) + (i & 3);
}
__device__ __forceinline__ int tile_row_d(int n, int g, int r) {
  return 32 * (n >> 1) + 8 * g + 4 * (n & 1) + r;
}

// Lane-constant byte offset of this lane's share of a transposed read of rows
// 8g..8g+3 (relative to a 32-row-aligned base) and the 16 columns of d-block 0.
template <int D>
__device__ __forceinline__ int tr_lane_base(int g, int c) {
  const int row = 8 * g + (c >> 2), sub = c & 3;
  return row * (2 * D) + ((((sub >> 1) ^ swzf<D>(row)) << 4) | ((sub & 1) << 3));
}

// B-fragment of a phase-2 MFMA for d-block nd, reduction rows r32..r32+31 of
// a swizzled row-major tile in the natural k order: lane group g gets rows
// r32+8g..+7 as two 4-row transposed reads.  swzf ignores row bits 2 and 5
// and d-block nd moves the chunk index by 2nd, which commutes with the
// swizzle xor: one v_xor per fragment, the rest is an immediate offset.
template <int D>
__device__ __forceinline__ bf16x8 read_b_tr(const short* tile, int lane_base, int r32, int nd) {
  const char* p = reinterpret_cast<const char*>(tile) + (lane_base ^ (nd * 32));
  short4v lo = lds_read_tr(p + r32 * (2 * D));
  short4v hi = lds_read_tr(p + (r32 + 4) * (2 * D));
  short8 t = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return *reinterpret_cast<bf16x8*>(&t);
}

// A-fragment made of the lane's own packed D-fragments (no relayout).
__device__ __forceinline__ bf16x8 own_a_frag(const int lo[2], const int hi[2]) {
  int4 a = make_int4(lo[0], lo[1], hi[0], hi[1]);
  return *reinterpret_cast<bf16x8*>(&a);
}

// Broadcast lane I of each row of 16 lanes to the whole row (DPP, no LDS).
template <int I>
__device__ __forceinline__ float row_bcast_i(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x150 + I, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_bcast(float v, int i) {
  switch (i) {
    case 0: return row_bcast_i<0>(v);
    case 1: return row_bcast_i<1>(v);
    case 2: return row_bcast_i<2>(v);
    case 3: return row_bcast_i<3>(v);
    case 4: return row_bcast_i<4>(v);
    case 5: return row_bcast_i<5>(v);
    case 6: return row_bcast_i<6>(v);
    case 7: return row_bcast_i<7>(v);
    case 8: return row_bcast_i<8>(v);
    case 9: return row_bcast_i<9>(v);
    case 10: return row_bcast_i<10>(v);
    case 11: return row_bcast_i<11>(v);
    case 12: return row_bcast_i<12>(v);
    case 13: return row_bcast_i<13>(v);
    case 14: return row_bcast_i<14>(v);
    default: return row_bcast_i<15>(v);
  }
}
