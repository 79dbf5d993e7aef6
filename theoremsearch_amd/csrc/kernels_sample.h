// The threshold sample of the batched search: scores of every query against a sparse sample of the corpus (every
// `tile_stride`-th tile of 32 rows, at most 8192 rows), written as a dense [query][sample position] fp32 matrix that
// sample_select_fast_kernel (kernels_level.h) turns into the pass thresholds of the full-corpus pass.
//
// Round 2 ran the full-pass kernel itself over the sample (SPARSE instantiation: 393 KB of query fragments per workgroup
// for ONE tile of work, every score appended to lane-private lists that the select then gathered from 1,024 writers):
// 30-36 us + 21-24 us per search, whatever the corpus size - a tenth of the step of an eighth-of-the-corpus shard.  This
// kernel is shaped for the sample instead, and for latency: the whole launch is two memory round trips deep.
//   * a workgroup takes RB = 2 blocks of 16 sample rows and brings them into LDS by LDS-DMA
//     (global_load_lds_dwordx4), all pieces in flight at once: every 128-byte line of a row is fetched once, in ONE round trip to HBM
//     (a first version read operand fragments straight from global memory, 64 bytes of each row per k-step: a chain of
//     six dependent HBM round trips, 22 us at 4,096 rows and 44 us at 8,192);
//   * the queries come from L2 (every workgroup reads the same 393 KB) as MFMA B fragments, one 16-byte load per k-step
//     and lane, all of a 64-query chunk in flight at once; wave w holds queries 16 w .. 16 w + 15 of the chunk;
//   * one workgroup per (32 rows, 64-query chunk): 4,096 rows x 256 queries = 128 row groups x 4 chunks = 512 workgroups,
//     two to a CU (a first cut with every chunk looped inside 64 workgroups of 64 rows took 36 us against 15 for this
//     shape: the chunks are independent work); the chunk's query fragments are requested before the rows (round 4).
//
// Arithmetic: v_mfma_f32_16x16x32_bf16 (bf16 rows) or v_mfma_f32_16x16x4_f32 (fp32 rows: float i of a 16-byte chunk times
// float i of the matching query chunk, as the full pass does).  The sums may differ from the full pass's in the order of
// the additions only; the thresholds they produce are estimates that the full pass verifies (a query with fewer than k
// candidates back is re-run exactly), so nothing downstream depends on bit-equal sample scores.
#pragma once
#include "kernels_screen8_tile.h"

namespace ts {

struct SampleArgs {
    const void* corpus;       // [n_pad x ld] storage dtype
    int64_t n;                // real rows
    int ld;                   // elements per row (multiple of 64, a row of at most 4,096 bytes: mfma_sample checks the LDS)
    int64_t ntiles;           // sample tiles; sample position p = 32 * tile + row
    int64_t tile_stride;      // sample tile j is global tile (j / run) * run * tile_stride + j % run
    int run;
    const void* q;            // queries in the storage dtype, row stride ld, at least 64 * ceil(nq / 64) rows
    int nq;
    const u32* row_mask;      // optional filter: disallowed rows score -inf (the sample sees the allowed rows only)
    float* scores;            // [64 * ceil(nq / 64)][row_stride]
    int row_stride;           // sample positions per query row of `scores` (multiple of 64, >= 32 * ntiles)
    int* fb_count;            // per-search counters, reset here (this is the first launch of a search)
    // optional: tile boundaries of the previous search's full pass to rebalance (grid.y = chunks + 1 then)
    int64_t* part;
    const unsigned* wg_ticks;
    int part_g;
    float part_gain;
    // optional: the int8 screen's image of this launch's queries (screen_quantize_query, kernels_screen8_tile.h; bf16 at d = 768 or 1024),
    // made by the workgroups of the extra row (grid.y = chunks + 1 then) - it needs only `q`, and the screen runs behind the
    // select that follows this launch
    signed char* scr_qimg;
    float4* scr_qmeta;
    u32* scr_count;
    int scr_nrows;            // rows of q that are queries of the launch (the image has kMfmaQ rows, zero past them)
};

constexpr int kSampleRowPad = 16;                                   // bytes: rows land 4 banks apart, the 16-row reads spread out
constexpr int sample_lds_bytes(int rows, int row_bytes) { return rows * (row_bytes + kSampleRowPad); }

// RB = row blocks of 16 per workgroup (2: 32 rows).  grid = (row_stride / (16 RB), query chunks of 64 [+ 1]), 256 threads,
// dynamic LDS = sample_lds_bytes(16 RB, ld * elem).  Row y = chunks of the grid exists when `part` or `scr_qimg` is set: its
// first workgroup moves the tile boundaries of the PREVIOUS search's full pass (rebalance_tiles, common.h) while the others
// score - the job used to ride on the empty re-run launch behind the pass, where it was that launch's whole duration - and
// all of its workgroups share out the queries of the int8 screen's image, a wave per query (a launch of its own before).
template <bool F32, int RB>
__global__ void __launch_bounds__(256) sample_scores_kernel(SampleArgs a) {
#include "kernels_sample_scores.inc"
}

}  // namespace ts
