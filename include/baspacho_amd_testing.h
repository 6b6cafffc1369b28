/* TESTING entry points of libbaspacho_amd.so -- NOT part of the drop-in boundary.  Kept out of
 * include/baspacho_amd.h (the header a caller installs) so that no product code links against a hook
 * that deliberately breaks factor(); tests/ and baspacho_amd/__init__.py (Solver._testSetFault) are
 * the only users. */
#ifndef BASPACHO_AMD_TESTING_H
#define BASPACHO_AMD_TESTING_H

#include "baspacho_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fault injection: kind 1 = factor() skips the sparse-elimination update (Solver.cpp:190-196,
 * doElimination's update half), so the factor is WRONG -- tests/test_full_size_gpu.py checks that the
 * full-size parity checks then fail; 0 = off.  Per solver, not reachable through the environment;
 * the library prints a warning to stderr the first time an injected fault takes effect. */
int bsp_test_set_fault(bsp_solver* s, int32_t kind);
/* kind 2 = the spine workgroup of block 1 of every persistent solve sweep (csrc/hip_sweep_kernels.h)
 * never publishes its x, and the sweeps' watchdog is set to 50 ms: the launch must end by itself and
 * the next solve must report the failed call (tests/test_sweep_gpu.py). */

/* The selected-inversion plan of the solver's skeleton (buildSelInvPlan, csrc/hip_plan.cpp: the plan
 * selectedInverse() runs), built on the host with no device involved.  Layout (int64):
 *   nLevels, nSmall, nNodes, linvElems, uElems, pElems, wElems,
 *   nSmall records {lump, level, n, r, k},
 *   nNodes records {lump, level, c0, w, r, nRest, kChunk, nk, nTiles, tileBase},
 * both in launch order.  *needed = total length; at most `capacity` values are written (buf may be
 * NULL to query the length). */
int bsp_test_selinv_plan(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed);
/* ... of the lumps before the cut at `span` alone (buildSelInvPlan(skel, upToLump): the plan
 * bsp_factor_adjoint_up_to_* runs), same record layout.  span == bsp_num_spans gives the plan above; a
 * span that bsp_factor_up_to_* refuses gives a non-zero return. */
int bsp_test_selinv_plan_up_to(const bsp_solver* s, int64_t span, int64_t* buf, int64_t capacity, int64_t* needed);

/* The reach plan (buildReachPlan, csrc/reach.cpp: the plan bsp_reach_solve_l_* / bsp_inverse_blocks_* run)
 * of `params` (caller's ids, HOST array) with one Gram item per pair (i, j), i >= j, of their positions,
 * built on the host with no device involved.  Layout (int64):
 *   cutLump, cutSpan, numCols, nQueries, nGroups, nItems, nUnits,
 *   nQueries records {span, lump, col0, width, len, len lumps of the reach (truncated at the cut)},
 *   nGroups records {query, col0, k, row0, len of its list, first lump of its list or -1},
 *   nItems records {i, j, colP, nP, colQ, nQ, outOff, rows, nRanges, nRanges pairs [begin, end) of
 *     internal scalars},
 *   nUnits pairs {column, row}: the unit entries of the queries at or beyond the cut.
 * buf / capacity / needed as bsp_test_selinv_plan. */
int bsp_test_reach_plan(const bsp_solver* s, int64_t num_params, const int64_t* params, int64_t* buf,
                        int64_t capacity, int64_t* needed);

/* The plan of the products with the factor (buildFactorProductPlan, csrc/factor_product_plan.cpp: the
 * plan bsp_factor_product_* run), built on the host with no device involved.  Layout (int64):
 *   nSpans, nChains, nLongRows, nTasks, nFolds, nSmallCols, partElems, nHugeSpans, nHugeWide,
 *   spanChainPtr (nSpans + 1), spanChain (nChains: the chains sorted by row span), spanChainLump (nChains:
 *   the column lump of each), spanLong (nSpans: 0 = rows one per lane, 1 = one per wave, 2 = the span per
 *   workgroup), longRows (nLongRows: the rows of the spans of kind 1),
 *   nTasks records {dataOff, lump, w, c0, nc, rBeg, rEnd, chain, part},
 *   nFolds records {col0, nc, part0, numChunks},
 *   smallColLump (nSmallCols), smallCol (nSmallCols),
 *   hugeSpans (nHugeSpans: the spans of kind 2), hugeWidePtr (nHugeSpans + 1), hugeWide (nHugeWide: positions
 *   in spanChain of the chains of lumps of more than 16 columns, per huge span).
 * buf / capacity / needed as bsp_test_selinv_plan. */
int bsp_test_factor_product_plan(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed);

/* The launch tables of the factor plan over every lump (buildLaunchTables, csrc/hip_plan.cpp: what the
 * launch code uploads beside the plan), built on the host with no device involved.  Layout (int64):
 *   nLevels, nMainLevels, nLevelPanels, nTrsmTasks, nUpdTasks (of the plan), then the lengths of
 *   levelPanelDescs, trsmTasksFat, updTasksFat, updTasksWide, slowPrefix, updTasksSplit, splitRange,
 *   foldRank, foldTiles, foldPanelEnd, foldDescs;
 *   nLevels records {elimination range or -1, tail, directPanel, panelBegin, panelEnd, trsmBegin, trsmEnd,
 *     updBegin, updEnd}: the bigLevels of every elimination range, then the plan's own (main) levels;
 *   levelPanelDescs {diagOff, lda, nb, rowsBelow, nRest, lumpRowBase, lump, vecOff};
 *   trsmTasksFat {diagOff, lda, nb, rowsBelow, rowTile};
 *   updTasksFat {srcOff, tgtBase, lda, K, rowsBelow, segEnd, rowTile, colTile, tgtStride, rowMin, atomic, fast};
 *   updTasksWide {srcOff, tgtBase, chainTabPtr, lda, K, rowsBelow, nRest, lumpRowBase, kind, segEnd, tgtStride,
 *     firstChainOrd, rowMin, rowTile, colTile, atomic};
 *   slowPrefix; updTasksSplit (as updTasksWide); splitRange {updBegin, begin, end}; foldRank; foldTiles;
 *   foldPanelEnd; foldDescs (as levelPanelDescs).
 * buf / capacity / needed as bsp_test_selinv_plan. */
int bsp_test_launch_tables(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed);
/* The solve schedule of the same plan's main levels (buildSolveSchedule) under the given switches.
 * Layout (int64):
 *   nLevels, nItems, nInvPanels, numSweeps, sweepInstStride, maxSweepWgs, maxSweepWgsM, maxSweepW, maxSweepBelow;
 *   nLevels records {panels, lump, column inside the lump, nb, rowsBelow} (the last four of the level's
 *     one panel, -1 for a level of several);
 *   nItems records {kind (0 level, 1 block group, 2 sweep), slot, l, e, sweep w, nBlocks, rowsBelow, invSlot,
 *     xchgOff, forward workgroups, backward workgroups};
 *   nInvPanels records {lump, column inside the lump, nb, rowsBelow}. */
int bsp_test_solve_schedule(const bsp_solver* s, int32_t with_sweeps, int32_t block_solve, int32_t inverses,
                            int32_t sweep_min_width, int64_t* buf, int64_t capacity, int64_t* needed);

/* Caps the chunk of a batched selected inversion (bsp_selected_inverse_batched_*) at `max_matrices`
 * matrices, so that tests can force several chunks on small batches; 0 = the product's rule. */
int bsp_test_set_selinv_batch_chunk(bsp_solver* s, int32_t max_matrices);

/* Read-only: *out = bytes of one slot of the ring that carries the pointer arrays of batched calls to the
 * device (PtrRing, csrc/hip_context.h): 0 before the first batched call, 512 up to 64 pointers, then the
 * largest array seen rounded up to 256.  A change between two calls shows that the ring's growth path
 * (wait for the device, free every slot, allocate anew) ran in between (tests/test_history_gpu.py). */
int bsp_test_ptr_ring_slot_bytes(bsp_solver* s, int64_t* out);

/* The tables of an ordered-fill plan (csrc/bal_fill_plan.h), copied out for the CPU tests.  Layout (int64):
 *   numPts, numCams, camSize, kept, skipped, nPairs, nChunks, C, W, scratchLen;
 *   ptPtr[numPts + 1], ptObs[kept], pairPtr[nPairs + 1], pairCam, pairPt, pairOff, pairStride,
 *   pairFlip [nPairs each], camPtr[numCams + 1], camObs[kept], camChunkPtr[numCams + 1], chunkCam,
 *   chunkBegin, chunkEnd [nChunks each], ptDiagOff, ptDiagStride, ptStart [numPts each], camDiagOff,
 *   camDiagStride, camStart [numCams each].
 * buf / capacity / needed as bsp_test_selinv_plan. */
int bsp_test_bal_fill_plan(const bsp_bal_fill_plan* p, int64_t* buf, int64_t capacity, int64_t* needed);

/* Developer aid: with BSP_SWEEP_TRACE=1 in the environment when the solver is created, every spine
 * workgroup of a persistent solve sweep stamps {start, operands on chip, inputs arrived, x published}
 * (wall clock, 100 MHz); this reads the stamps of the LAST sweep, 4 values per block. */
int bsp_test_read_sweep_trace(bsp_solver* s, long long* out, int32_t max_blocks, int32_t* n_blocks);

#ifdef __cplusplus
}
#endif

#endif
