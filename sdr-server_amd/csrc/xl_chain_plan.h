/* xl_chain_plan.h -- how the chain wave of xl_nco_chain_kernel (xl_kernels.hip) covers a region of table entries: HIP-free,
 * shared by the kernel and by tests/c/chain_plan_sweep.cpp.
 *
 * A region is the entries [e, e_stop) between two block ends: plain recurrence steps for every lane.  The chain wave has two
 * bodies for it.  The 32-entry block addresses its ring slots with immediate offsets, so it starts only where the ring slot
 * (entry & (ring - 1)) is a multiple of the block, and it is the fast one (13.9 cycles per step).  The any-slot entry carries its
 * own ring address, count and exit test and starts anywhere (about 17 cycles per step).  The cover of a region is therefore
 *   head   any-slot entries up to the next slot that is a multiple of the block (fewer than one block),
 *   blocks whole blocks, back to back,
 *   tail   any-slot entries (fewer than one block),
 * each of the three one asm block in the kernel.  A region too short to hold an aligned block is head and tail only.
 *
 * Head and tail need not be any-slot entries throughout (xl_chain_plan8): a run of 8 entries that starts at a slot that is a multiple of
 * 8 never runs over the ring's end either, and addresses its slots with immediates off one base, with one count post, one address
 * update and one exit test per 8 entries -- the block's cost per step.  So the head is any-slot entries up to the next multiple of 8
 * slots (fewer than 8) and then 8-entry runs up to the next multiple of the block (at most block / 8 - 1), and the tail is 8-entry runs
 * and then fewer than 8 any-slot entries; head and tail stay one asm block each. */
#ifndef XL_CHAIN_PLAN_H_
#define XL_CHAIN_PLAN_H_
#include <stdint.h>

#ifndef XL_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define XL_HD __host__ __device__ static inline
#else
#define XL_HD static inline
#endif
#endif

typedef struct XlChainPlan {
  uint32_t head;   /* any-slot entries e .. e + head - 1 */
  uint32_t blocks; /* aligned blocks from entry e + head on */
  uint32_t tail;   /* any-slot entries after the blocks, up to e_stop - 1 */
} XlChainPlan;

/* ring and block are powers of two, block <= ring (a block that starts at a multiple of itself never runs over the ring's end) */
XL_HD XlChainPlan xl_chain_plan(uint32_t e, uint32_t e_stop, uint32_t ring, uint32_t block) {
  XlChainPlan pl = {0u, 0u, 0u};
  uint32_t left, to_align;
  if (e_stop <= e) return pl;
  left = e_stop - e;
  to_align = (block - ((e & (ring - 1u)) & (block - 1u))) & (block - 1u);
  pl.head = to_align < left ? to_align : left;
  left -= pl.head;
  pl.blocks = left / block;
  pl.tail = left - pl.blocks * block;
  return pl;
}

typedef struct XlChainPlan8 {
  uint32_t head1;  /* any-slot entries e .. e + head1 - 1 (fewer than run) */
  uint32_t head8;  /* aligned runs of `run` entries after them (fewer than block / run) */
  uint32_t blocks; /* aligned blocks after those: as many as xl_chain_plan's */
  uint32_t tail8;  /* aligned runs after the blocks (fewer than block / run) */
  uint32_t tail1;  /* any-slot entries up to e_stop - 1 (fewer than run) */
} XlChainPlan8;

/* ring, block and run are powers of two, run <= block <= ring.  A region that ends before the next block boundary is head1, head8 and
 * tail1 only. */
XL_HD XlChainPlan8 xl_chain_plan8(uint32_t e, uint32_t e_stop, uint32_t ring, uint32_t block, uint32_t run) {
  XlChainPlan8 pl = {0u, 0u, 0u, 0u, 0u};
  uint32_t left, slot, to_run, to_block;
  if (e_stop <= e) return pl;
  left = e_stop - e;
  slot = e & (ring - 1u);
  to_run = (run - (slot & (run - 1u))) & (run - 1u);
  pl.head1 = to_run < left ? to_run : left;
  left -= pl.head1;
  slot += pl.head1;
  to_block = (block - (slot & (block - 1u))) & (block - 1u); /* (a multiple of run wherever left != 0) */
  if (left < to_block) {
    pl.head8 = left / run;
    pl.tail1 = left - pl.head8 * run;
    return pl;
  }
  pl.head8 = to_block / run;
  left -= to_block;
  pl.blocks = left / block;
  left -= pl.blocks * block;
  pl.tail8 = left / run;
  pl.tail1 = left - pl.tail8 * run;
  return pl;
}

#endif /* XL_CHAIN_PLAN_H_ */
