// block_layout.hpp -- where the owned reference blocks of a species lie in its packed arrays: the valid markers of all
// blocks first, in block order, their tail slots behind, in block order.  THE statement of that layout: particle_load,
// the optimisation events' OptBlocks, their re-pack and both directions of the pass on host copies take their offsets
// from here (tests/test_block_layout_host.py).  No context, no HIP call.
#pragma once
#include <cstdint>
#include <vector>

namespace pic1dp {

struct BlockSpan {
  int64_t voff, np, toff, ntail;  // valid markers [voff, voff + np), tail slots [toff, toff + ntail)
};
struct BlockLayout {
  std::vector<BlockSpan> blk;
  int64_t np = 0;  // the species' valid markers: where the tails begin
};
// blk_alloc[nblk]: slots of each block; blk_np[nblk]: its valid markers of one species
inline BlockLayout block_layout(const std::vector<int64_t> &blk_alloc, const std::vector<int64_t> &blk_np) {
  BlockLayout L;
  for (int64_t np : blk_np) L.np += np;
  int64_t voff = 0, toff = L.np;
  for (size_t b = 0; b < blk_alloc.size(); ++b) {
    L.blk.push_back(BlockSpan{voff, blk_np[b], toff, blk_alloc[b] - blk_np[b]});
    voff += blk_np[b];
    toff += blk_alloc[b] - blk_np[b];
  }
  return L;
}

}  // namespace pic1dp
