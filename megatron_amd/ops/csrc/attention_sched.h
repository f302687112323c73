// Block placement for the attention kernels: which (sequence block, head) a
// workgroup of a 1-D grid computes.  Plain C++ as well as HIP, so the map can
// be checked exhaustively on the host (tests/test_attention_block_map.py).
//
// Every attention kernel runs one 512-thread block per CU, and the hardware
// hands linear workgroup id i to XCD i % 8, in order inside each XCD.  Causal
// work per block is a ramp over the sequence block index, so a plain 2-D grid
// gives the XCDs unequal work and starts the heaviest blocks last.  The map:
//   * xcd = id & 7, idx = id >> 3.
//   * The ngrp = b * hkv kv groups are cut into 8 contiguous ranges whose sizes
//     differ by at most one; XCD x owns range x.  All `rep` heads of a group
//     that get blocks of their own stay on that XCD (one L2 holds the group's
//     K/V), and with ngrp % 8 == 0 every XCD gets the same work.
//   * Inside an XCD with H = groups * rep heads: rank = idx / H,
//     head = first + idx % H, blk = heavy_last ? nblk - 1 - rank : rank.  The
//     heaviest block of every head starts first, the lightest ones fill the
//     tail.
//   * Every XCD gets the same number of ids, so the grid is sized for the
//     largest range; ids beyond an XCD's own H * nblk are empty (blk < 0) and
//     the kernel returns at once.
// Scalar arithmetic on the workgroup id only: it costs no vector register.
#pragma once

#if defined(__HIPCC__)
#define ATTN_SCHED_HD __host__ __device__ __forceinline__
#else
#define ATTN_SCHED_HD inline
#endif

constexpr int ATTN_NXCD = 8;

struct AttnBlock {
  int blk;   // block along the sequence, -1: empty slot
  int head;  // group * rep + head-in-group (the group index itself when rep == 1)
};

// id: workgroup id of the 1-D grid; nblk: blocks along the sequence; ngrp: kv
// groups; rep: heads per group with blocks of their own (hq / hkv for fwd and
// dq, 1 for dkv); heavy_last: work grows with the block index (fwd, dq) or
// falls with it (dkv).
ATTN_SCHED_HD AttnBlock attn_block_map(int id, int nblk, int ngrp, int rep, bool heavy_last) {
  const int xcd = id & (ATTN_NXCD - 1), idx = id / ATTN_NXCD;
  const int gq = ngrp / ATTN_NXCD, gr = ngrp % ATTN_NXCD;
  const int first = xcd * gq + (xcd < gr ? xcd : gr);  // first group of this XCD
  const int heads = (gq + (xcd < gr ? 1 : 0)) * rep;
  if (idx >= heads * nblk) return AttnBlock{-1, -1};
  const int rank = idx / heads;
  return AttnBlock{heavy_last ? nblk - 1 - rank : rank, first * rep + idx % heads};
}

// Grid size: 8 XCDs x the slots of the largest group range.
inline int attn_sched_grid(int nblk, int ngrp, int rep) {
  return ATTN_NXCD * ((ngrp + ATTN_NXCD - 1) / ATTN_NXCD) * rep * nblk;
}
