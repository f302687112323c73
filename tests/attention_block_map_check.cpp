// Host check of attn_block_map (megatron_amd/ops/csrc/attention_sched.h),
// compiled and run by test_attention_block_map.py.  Walks every id of the grid
// for nblk 1..20, ngrp 1..40, rep in {1, 2, 4} and both orders, and checks that
//   * every (blk, head) is produced exactly once,
//   * the empty slots are exactly grid - nblk * ngrp * rep, and inside an XCD
//     they come after all of its blocks,
//   * all heads of a kv group land on one XCD,
//   * group counts per XCD differ by at most one,
//   * inside an XCD the causal work (blk + 1 when heavy_last, nblk - blk
//     otherwise) never increases with idx.
// Prints "OK <combinations>" and exits 0, or the first failure and exits 1.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "attention_sched.h"

static int fail(const char* what, int nblk, int ngrp, int rep, int heavy_last, int id) {
  std::printf("FAIL %s: nblk=%d ngrp=%d rep=%d heavy_last=%d id=%d\n", what, nblk, ngrp, rep, heavy_last, id);
  return 1;
}

int main() {
  long combos = 0;
  const int reps[] = {1, 2, 4};
  for (int nblk = 1; nblk <= 20; ++nblk)
    for (int ngrp = 1; ngrp <= 40; ++ngrp)
      for (int rep : reps)
        for (int hl = 0; hl < 2; ++hl) {
          const int heads = ngrp * rep;
          const int grid = attn_sched_grid(nblk, ngrp, rep);
          if (grid % ATTN_NXCD != 0 || grid < nblk * heads) return fail("grid size", nblk, ngrp, rep, hl, -1);
          std::vector<int> seen(nblk * heads, 0);
          std::vector<int> group_xcd(ngrp, -1);
          int groups_on[ATTN_NXCD] = {0};
          int last_work[ATTN_NXCD];
          bool ended[ATTN_NXCD] = {false};
          std::fill(last_work, last_work + ATTN_NXCD, nblk + 1);
          int empty = 0;
          // ids in increasing order visit every XCD's idx in increasing order
          for (int id = 0; id < grid; ++id) {
            const AttnBlock m = attn_block_map(id, nblk, ngrp, rep, hl != 0);
            const int xcd = id % ATTN_NXCD;
            if (m.blk < 0) {
              ++empty;
              ended[xcd] = true;
              continue;
            }
            if (ended[xcd]) return fail("block after an empty slot", nblk, ngrp, rep, hl, id);
            if (m.blk >= nblk || m.head < 0 || m.head >= heads) return fail("out of range", nblk, ngrp, rep, hl, id);
            if (seen[m.head * nblk + m.blk]++) return fail("produced twice", nblk, ngrp, rep, hl, id);
            const int grp = m.head / rep;
            if (group_xcd[grp] < 0) {
              group_xcd[grp] = xcd;
              ++groups_on[xcd];
            } else if (group_xcd[grp] != xcd) {
              return fail("group on two XCDs", nblk, ngrp, rep, hl, id);
            }
            const int work = hl ? m.blk + 1 : nblk - m.blk;
            if (work > last_work[xcd]) return fail("work increases with idx", nblk, ngrp, rep, hl, id);
            last_work[xcd] = work;
          }
          for (int i = 0; i < nblk * heads; ++i)
            if (seen[i] != 1) return fail("never produced", nblk, ngrp, rep, hl, i);
          if (empty != grid - nblk * heads) return fail("empty slot count", nblk, ngrp, rep, hl, empty);
          const int lo = *std::min_element(groups_on, groups_on + ATTN_NXCD);
          const int hi = *std::max_element(groups_on, groups_on + ATTN_NXCD);
          if (hi - lo > 1) return fail("group counts differ by more than one", nblk, ngrp, rep, hl, hi - lo);
          ++combos;
        }
  std::printf("OK %ld\n", combos);
  return 0;
}
