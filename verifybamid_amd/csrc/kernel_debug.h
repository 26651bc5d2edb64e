// kernel_debug.h -- every compile-time switch of the kernels (eval_body.h, llk_kernels.hip, llk_passes.hip, resident_kernel.inc).  A shipping build
// defines none of them; the profiling builds are made by csrc/Makefile (libvb2_stamps.so, `make stamps_round`) and
// tools/build_variant.sh.
//
//   VB2_WITH_STAMPS     in-kernel wall-clock stamps per workgroup (tools/stamps.py, tools/stamps_resident.py): the tests they
//                       leave behind in every kernel cost 0.6 % of a 48-point launch and 4 % of a small sample's search
//   VB2_STAMP_ROUND=n   the per-workgroup stamps are those of round n of a resident search (a round that took the short way)
//                       instead of the last evaluation's
//   VB2_STAMP_CTRL      stamp slot 3 of workgroup 0 = the control wave is back from its tile-phase work
//   VB2_ITEM_PROF       with VB2_WITH_STAMPS: where a wave's time per work item goes (tools/item_prof.py)
//   VB2_FLAG_RELEASE=0  the host hand-off's flag as a RELAXED system-scope store behind acknowledged write-through result stores (rounds
//                       4-5; the shipping build stores it with RELEASE semantics, and the host still sets the result words to NaN
//                       before every step and re-reads a NaN)
//   VB2_ABLATE=mask     ablation builds -- parts of a launch compiled out, to price what is left:
//                         1 kAblNoMap     nothing is read from mapped host memory (rows are made up, counts assumed full)
//                         2 kAblNoTable   the per-alpha table is not built
//                         4 kAblNoItems   no work items at all: a launch's fixed cost
//                         8 kAblNoReads   the run words are consumed, the table is not read
//                        16 kAblNoEpi     the sums and constants are consumed, nothing is computed from them
//                        32 kAblNoSignal  no hand-off to the host
//                        64 kAblNoMul     probability domain: the table rows are read, the products not multiplied
//                       128 kAblNoRowLoads  probability domain: the steps are made up in registers, no loads of the lists
//   VB2_SPLIT_FAST=mask the short head and tail of a split launch (eval_body, SPLIT), each part on its own for A/B builds (default: all):
//                         1 the tables are built from records and alphas requested at kernel entry, not from the staged copies
//                         2 one arrival ticket per share of the point groups: each share's last workgroup adds up that share's points
//   VB2_SIMD_DEAL=0     wave w of a search round takes item w instead of the SIMD-balanced first deal (eval_body)
//   VB2_READS_AHEAD=0xRNPS how a row word of the probability-domain walk (eval_body, walk_pd) orders its table reads and its multiplies, one
//                       hex digit per kernel family -- S llk_eval_split_kernel, P the plain 8-point launch llk_eval_kernel<2, ...>, N the
//                       4-point and narrower launches llk_eval_kernel<3..5, ...>, R the resident search kernel (default 0x0111):
//                         0 as the scheduler likes it: four landing quads, a step's six reads in three dependent round trips
//                         1 a row at a time: both steps' twelve reads, then their multiplies (a drain per two rows of the loop)
//                         2 a step at a time: a step's six reads, then its multiplies (a drain per step)
//                         3 as 1, and a tile's last row also requests the epilogue's 2 k projection coefficients before it multiplies (KSEL 2, 4)
//                         4 as 3 with the coefficients of the first two components only (four quads)
//                       (the cohort kernels and the pass-per-group kernel keep 0: with 1 some of them spill; R: see HISTORY.md)
//   VB2_ITEM_AHEAD=0xPS where a wave of the 8-point probability-domain shape on the work queue gets its NEXT item from (eval_body, AHEAD),
//                       one hex digit per kernel family -- S llk_eval_split_kernel, P the plain 8-point launch llk_eval_kernel<2, 1, *, true>:
//                         0 at the item's head: the draw, the tile's record, its first rows -- three dependent trips before the first table read
//                         1 the draw and the record's request behind the present item's last row, the list's rows 0, 1, 2 behind its
//                           epilogue; the first row's refill is row 2, so its three kinds meet without a copy of a loading register
//                         2 as 1, and the ring of row words has fixed registers: a row's two table addresses are taken from its word
//                           before the refill is loaded into the same register -- no copy of a ring word in any loop of the walk
//                       (default 0x02: -2.6 % on the 48-point launch; P measured faster, but not by three times the spread: HISTORY.md)
//   VB2_EPI_TRIPS=0xPS  the three dependent LDS round trips of an item's epilogue in the 8-point probability-domain shape on the work queue
//                       (eval_body, EPI), one hex digit per kernel family as for VB2_ITEM_AHEAD; each digit a MASK of three parts (bit 8: another
//                       place for part 1):
//                         1 the draw rides the last row's reads: the queue's ds_add_rtn goes out behind that row's twelve table reads and
//                           before its multiplies, its result is taken behind them (needs VB2_ITEM_AHEAD != 0 in that family; a tile of
//                           one row or none draws where it did)
//                         2 the 2 k projection coefficients are requested directly behind the last row's multiplies -- its landing registers
//                           are dead --, ahead of the next item's bookkeeping and the record's request (KSEL 2, 4)
//                         4 the tile butterfly's exchange over marker bit 3 without the LDS crossbar: two row-masked DPP moves and a
//                           v_permlane16_swap per dword instead of a ds_bpermute
//                         8 part 1 with the draw in FRONT of the last row's reads: the lane-0 branch around the atomic then does not cut
//                           the row's block between its reads and its multiplies (takes precedence over bit 1)
//                       (default 0x04: -1.2 % on the 48-point launch.  Parts 1 and 8 measured SLOWER by 0.4 us -- the tile's last row on its own
//                       costs more than the draw's trip --, part 2 without effect, digit P = 4 without effect: HISTORY.md)
#ifndef VB2_KERNEL_DEBUG_H_
#define VB2_KERNEL_DEBUG_H_

#ifndef VB2_ABLATE
#define VB2_ABLATE 0
#endif
#ifndef VB2_FLAG_RELEASE
#define VB2_FLAG_RELEASE 1      // the flag the host spins on is stored with system-scope RELEASE semantics (0: relaxed; A/B: profiles/r06/ab_flag_release.txt -- no measurable cost)
#endif
#ifndef VB2_SOFT_PROLOGUE
#define VB2_SOFT_PROLOGUE 1     // the resident kernel's control wave starts its round's work at once instead of behind the table build (eval_body; 0: A/B)
#endif
#ifndef VB2_CTRL_PRIO
#define VB2_CTRL_PRIO 3         // the control wave's priority during its tile-phase work
#endif
#ifndef VB2_SPLIT_FAST
#define VB2_SPLIT_FAST 3
#endif
#ifndef VB2_READS_AHEAD
#define VB2_READS_AHEAD 0x0111
#endif
#ifndef VB2_ITEM_AHEAD
#define VB2_ITEM_AHEAD 0x02     // (profiles/r10/ab_item_head.txt)
#endif
#ifndef VB2_EPI_TRIPS
#define VB2_EPI_TRIPS 0x04      // (profiles/r11/ab_epi_trips.txt)
#endif
#ifndef VB2_SIMD_DEAL
#define VB2_SIMD_DEAL 1    // (0: wave w takes item w -- the A/B of the SIMD-balanced first deal, see eval_body)
#endif
#ifndef VB2_STAMP_ROUND
#define VB2_STAMP_ROUND 0
#endif

namespace vb2 {
constexpr int kAblNoMap = 1, kAblNoTable = 2, kAblNoItems = 4, kAblNoReads = 8, kAblNoEpi = 16, kAblNoSignal = 32, kAblNoMul = 64, kAblNoRowLoads = 128;
constexpr int kAblate = VB2_ABLATE;
constexpr int kSplitFast = VB2_SPLIT_FAST;
constexpr int kReadsAheadMask = VB2_READS_AHEAD;
constexpr int reads_ahead(int family) { return (kReadsAheadMask >> (4 * family)) & 0xf; }      // family: 0 S, 1 P, 2 N, 3 R
constexpr int kItemAheadMask = VB2_ITEM_AHEAD;
constexpr int item_ahead(int family) { return (kItemAheadMask >> (4 * family)) & 0xf; }        // family: 0 S, 1 P
constexpr int kEpiTripsMask = VB2_EPI_TRIPS;
constexpr int epi_trips(int family) { return (kEpiTripsMask >> (4 * family)) & 0xf; }          // family: 0 S, 1 P
}  // namespace vb2

#ifdef VB2_WITH_STAMPS
#define VB2_STAMPS_OF(L) ((L).stamps)
#else
#define VB2_STAMPS_OF(L) (static_cast<unsigned long long*>(nullptr))
#endif

#ifdef VB2_ITEM_PROF
#define VB2_IP_T(var) const unsigned long long var = __builtin_readcyclecounter()
#define VB2_IP_USE(x) asm volatile("" ::"v"(x))
#else
#define VB2_IP_T(var)
#define VB2_IP_USE(x)
#endif

#endif
