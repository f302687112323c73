// XCD-aware block order shared by the 256 x 256-tile GEMM kernels
// (grouped_gemm_hip.hip, mx_gemm.hip).
#pragma once

constexpr int GG_GR = 4;       // row tiles of a super-group
constexpr int GG_CHUNK = 32;   // consecutive blocks of the logical order that one XCD runs

// Block order.  Workgroup id lands on XCD id % 8.  The logical order walks
// super-groups of GG_GR row tiles, inside one column tile by column tile with
// the row tiles innermost; XCD x runs the chunks x, x + 8, ... of GG_CHUNK
// consecutive logical blocks, so the 32 blocks in flight on an XCD are 4 row
// tiles x 8 column tiles that share their operand tiles in its L2, and the
// unused row tiles at the end of the map spread over all XCDs.
__device__ __forceinline__ bool gg_block(int id, int T, int nct, int& rt, int& ct) {
  const int x = id & 7, j = id >> 3;
  const long L = ((long)(j / GG_CHUNK) * 8 + x) * GG_CHUNK + j % GG_CHUNK;
  if (L >= (long)T * nct) return false;
  const int per = GG_GR * nct;
  const int sg = (int)(L / per), rem = (int)(L % per);
  const int gr = min(GG_GR, T - sg * GG_GR);
  ct = rem / gr;
  rt = sg * GG_GR + rem % gr;
  return true;
}

static inline int gg_grid(long T, long nct) {
  const long per = 8 * GG_CHUNK;
  return (int)((T * nct + per - 1) / per * per);
}
