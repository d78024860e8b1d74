// rtx_f4node.h — the fast tree's node: plain data the host builds (build_fast4,
// rtx_scene_plan.cc) and the kernels walk and refit.  No HIP header.
#ifndef RTX_F4NODE_H_
#define RTX_F4NODE_H_

#include <stdint.h>

namespace rtxd {

// 4-wide fast node (RTX_PREC_FAST): a binary SAH tree collapsed so every node holds up to four
// children's outward-rounded f32 boxes (SoA for the four slab tests; build_fast4).  Every leaf
// slot holds exactly one primitive: child >= 0: node index; child < 0: leaf, ~child = the
// primitive; counts[]: 1 for a leaf slot (read by no kernel: the lean walk relies on the
// one-primitive layout); an empty slot is an inverted box (lo = +inf, hi = -inf, child -1) that
// no ray enters.  128 bytes = two cache lines.
struct F4Node {
  float lox[4], hix[4], loy[4], hiy[4], loz[4], hiz[4];  // axis a: lo at 32a, hi at 32a + 16 bytes
  int32_t child[4];
  uint32_t counts[2];
  uint32_t pad_[2];
};
static_assert(sizeof(F4Node) == 128, "F4Node must be two 64-byte lines");

}  // namespace rtxd

#endif  // RTX_F4NODE_H_
