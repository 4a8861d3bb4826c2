/*
 * Voltrix-SpMM for MI355X (gfx950) -- C-ABI of libvoltrix_hip.so (the drop-in boundary).
 *
 * The reference (YaqiXia/Voltrix-SpMM) has exactly one process-internal FFI: each kernel module is
 * JIT-compiled into its own kernel.so exporting
 *
 *     extern "C" void launch(<args...>, int& __return_code);
 *
 * (voltrix/jit/template.py:104-123) which voltrix/jit/runtime.py:38-52 calls through ctypes with tensors
 * as data_ptr() -> void*, Python int -> C int, bool -> bool, torch.cuda.Stream -> void* (stream handle)
 * and `int&` passed as ctypes.byref(c_int), i.e. a pointer at ABI level.
 *
 * This header declares the same four argument lists as named symbols of ONE ahead-of-time library
 * (voltrix_launch_*), plus the gfx950 extensions (fp16 operand, tile selection, fused GPU preprocess).
 * The JIT layer of the Python package (voltrix/jit) still generates per-kernel `launch` wrappers with
 * these exact argument lists; both routes call the same voltrix:: host launchers
 * (the .hpp headers under voltrix-spmm_amd/voltrix/include/voltrix).
 *
 * Contract shared by every entry point
 *   - plain C types only; every buffer is owned by the caller (the reference allocates everything in
 *     Python, voltrix/spmm/spmm.py:28-57,101); the library never allocates or frees device memory and keeps
 *     no state between calls;
 *   - device work is enqueued asynchronously on `stream` (a hipStream_t; NULL = the null stream, which is
 *     where the reference runs its preprocess kernels, bmat_kernels.cuh:204,234); no host synchronisation;
 *   - *return_code is ALWAYS written: 0 on success, a voltrix_rc value otherwise (the reference plumbs
 *     __return_code but never sets it; on errors it throws through ctypes or exit(1)s,
 *     spmm_kernels.cuh:28-45);
 *   - nothing is printed (the reference's preprocess printf's, bmat_kernels.cuh:309-310);
 *   - memory the caller did not define (DESIGN.md section 3.21 has a row per buffer): no `workspace`, `fill_workspace`, `partials`,
 *     header, status, table or output argument NEED BE INITIALISED.  The library writes -- by a kernel or by a hipMemsetAsync on
 *     `stream` -- every byte of a scratch buffer before it reads it and every element of every output it documents as written, and
 *     nothing in a scratch buffer survives a call, except that a phase-2 call reads what its own phase 1 left in the SAME workspace,
 *     untouched in between.  A buffer last used by another call, another graph or another operator serves as well as a fresh one.
 *     The exceptions, each stated again where it applies, are inputs by nature: `output` of the atomic forms (atomic_out = 1,
 *     accumulate = 2: the CALLER ZERO-FILLS it) and of accumulate = 1 / combine passes with accumulate != 0 (it holds the other
 *     addend), and `level` / `rank` of the breadth-first search (the caller sets them to -1 before the first component).
 *   - Pointers.  Every argument is checked on the host, before any launch and before any other runtime call; the first bad one is
 *     answered with VOLTRIX_ERR_BAD_SHAPE (VOLTRIX_ERR_BAD_CONFIG / VOLTRIX_ERR_OVERFLOW where an entry point says so) and nothing is
 *     enqueued.  A pointer is one of three kinds:
 *       required      every valid call with non-zero sizes gives it an element -- blk_offsets, output, the plan arrays of the panel
 *                     and fused kernels (the builders pad them), units / runs of the stream kernel, records, tickets of the ticket
 *                     forms, every header / status / table output a builder writes, `input` of the entry points that take no
 *                     input_rows (the operand has num_nodes rows at least).  NULL: VOLTRIX_ERR_BAD_SHAPE.
 *       optional      NULL has the meaning its entry point documents: window_order, out_scale, units (with unit_ptr), row_map,
 *                     xcd_ptr / panel_xcd_ptr / window_xcd_ptr, panel_order, parts of the ticket form, partials of a table without
 *                     cut windows or cut panels, the workspace of voltrix_launch_cm_rank without a level above 1024 nodes.
 *       may be empty  an array that has no element for some valid input, where the launcher cannot tell on the host: hspa_packed and
 *                     hind of a graph without edges (the number of TC blocks is blk_offsets[W], on the device), edge_list / indices /
 *                     t_indices / resid_edge_list of a CSR without entries, cuts / runs of a table without any, `input` of the entry
 *                     points with an input_rows argument (an operator without columns), the workspace of the fused preprocess (its
 *                     size is a function of the sizes and the path).  NULL is accepted -- hosts that pass an empty tensor's address
 *                     pass NULL -- and nothing is read through it.
 *     Alignment: where an entry point states one (16 bytes: input, hspa_packed, units, cuts of the unit table, runs, records,
 *     tickets, the workspaces of the builders, of the transpose and of voltrix_launch_spmm_f32_as_f16, output of the ticket forms and of the combine pass of the unit table; 8: scale; 4: indptr / indices /
 *     values of the CSR row-gather kernel, scale of voltrix_launch_scale_rows) an address off by less is VOLTRIX_ERR_BAD_SHAPE, for an
 *     optional or possibly empty pointer as well.  Sizes that are "nothing to do" (num_nodes == 0, embedding_dim == 0, num_cuts == 0,
 *     count == 0, max_runs_per_xcd == 0) answer VOLTRIX_OK without a launch and without looking at a pointer, except where an entry
 *     point writes an output even then (the headers of the count phases, unit_ptr, run_ptr, wave_ptr[0], the padding record, the
 *     scale of the scaled cast, pointer1[0]: those outputs stay required).  tests/core_abi_cases.py has the role of every parameter.
 */
#ifndef VOLTRIX_CAPI_H_
#define VOLTRIX_CAPI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOLTRIX_ABI_VERSION 2 /* 2 (round 4): explicit path / slab_policy / input_rows arguments instead of environment reads */

#define VOLTRIX_CSR_AUTO (-1)  /* `path` of the fused preprocess entry points: the library's rule (0 sort, 1 bitmap, 2 mixed) */
#define VOLTRIX_SLAB_AUTO (-1) /* `slab_policy` of the panel kernel (0 one grid over all column slabs, 1 one launch per group) */
#define VOLTRIX_BLK_H 16 /* rows per row window           (voltrix/spmm/spmm.py:12) */
#define VOLTRIX_BLK_W 8  /* condensed columns per TC block (voltrix/spmm/spmm.py:13) */

enum voltrix_rc {
  VOLTRIX_OK = 0,
  VOLTRIX_ERR_BAD_SHAPE = 1,  /* negative sizes, embedding_dim % 8 != 0 (fp16) / % 4 (fp32), a misaligned pointer, a NULL pointer
                                 that has to point at something (see "Pointers" above), an enum or a range argument outside its range */
  VOLTRIX_ERR_LAUNCH = 2,     /* hipGetLastError() after the launch */
  VOLTRIX_ERR_BAD_CONFIG = 3, /* tile (fs, depth, waves) not instantiated */
  VOLTRIX_ERR_OVERFLOW = 4,   /* total TC blocks exceed int32 (the handle stores int32 offsets) */
  VOLTRIX_ERR_DUPLICATE = 5
};

int voltrix_abi_version(void);

/* ---- the reference's four launch() argument lists ------------------------------------------------------- */

/* Replaces launch() of kernel.preprocess_kernel.* -- voltrix/jit_kernels/preprocess.py:57-65 ->
 * voltrix::preprocess, bmat_kernels.cuh:264-320.  ALL pointers are HOST int32 arrays:
 * edge_list[E], node_pointer[num_nodes+1], block_partition[W], edge_to_column[E], edge_to_row[E],
 * pointer1[W+1], W = ceil(num_nodes/16). */
void voltrix_launch_preprocess(void* edge_list, void* node_pointer, int num_nodes, void* block_partition,
                               void* edge_to_column, void* edge_to_row, void* pointer1, int* return_code);

/* Replaces launch() of kernel.hmat_gen_kernel.* -- voltrix/jit_kernels/hmat_gem.py:56-68 -> voltrix::hmat_cuda,
 * bmat_kernels.cuh:195-212 (kernel :21-111).  DEVICE pointers; hspa float[T*128] and hind int[T*8] are fully
 * written (zero-filled then scattered), T = pointer1[num_row_windows].  Runs on the null stream like the
 * reference (:204). */
void voltrix_launch_hmat_gen(void* node_pointer, void* edge_list, void* block_partition, void* edge_to_column,
                             void* edge_to_row, void* pointer1, int num_row_windows, int num_nodes, int num_edges,
                             void* hspa, void* hind, int* return_code);

/* Replaces launch() of kernel.hmat_packed_swizzle_kernel.* -- voltrix/jit_kernels/bmat_swizzle.py:38-43 ->
 * voltrix::hmat_packed_swizzle_cuda, bmat_kernels.cuh:228-242 (kernel :151-193).  hspa_packed uint32[T*4]. */
void voltrix_launch_hmat_packed_swizzle(int num_row_windows, void* pointer1, void* hspa, void* hspa_packed,
                                        int* return_code);

/* Replaces launch() of kernel.spmm_kernel.* -- voltrix/jit_kernels/spmm.py:78-88 ->
 * voltrix::voltrix_spmm_forward_cuda, spmm_kernels.cuh:2003-2113.  input float32 [*, embedding_dim], output
 * float32 [num_nodes, embedding_dim], both row-major contiguous DEVICE buffers; every row of output
 * (including the num_nodes % 16 tail the reference leaves unwritten) is stored.  Exact fp32 products on
 * v_mfma_f32_16x16x4_f32 (the reference rounds `input` to TF32).  embedding_dim % 4 == 0.  num_edges is unused,
 * as in the reference.  The tile is chosen by voltrix_spmm_default_tile(). */
void voltrix_launch_spmm(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                         int embedding_dim, void* input, void* output, void* stream, int* return_code);

/* ---- gfx950 extensions ------------------------------------------------------------------------------------ */

/* Same as voltrix_launch_spmm with an explicit tile: fs = feature slab per wave (32/64/128), depth = LDS ring
 * depth (2..4), waves = waves per workgroup (1/2/4/8); VOLTRIX_ERR_BAD_CONFIG if not instantiated.
 * window_order: NULL, or the int32[W] schedule written by voltrix_launch_window_order (changes speed only). */
void voltrix_launch_spmm_f32_tile(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                  int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                  void* window_order, void* out_scale, void* stream, int* return_code);

/* fp16 dense operand (BASELINE.json's headline configuration): input _Float16 [*, embedding_dim], output float32.
 * v_mfma_f32_16x16x32_f16, fp32 accumulate.  embedding_dim % 8 == 0, input 16-byte aligned. */
void voltrix_launch_spmm_f16(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                             int embedding_dim, void* input, void* output, void* stream, int* return_code);
void voltrix_launch_spmm_f16_tile(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                  int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                  void* window_order, void* out_scale, void* stream, int* return_code);

/* fp32 features on the 16-bit matrix-core path -- the fast replacement of voltrix_launch_spmm for hosts that keep the
 * reference's fp32 contract (jit_kernels/spmm.py:53: input float32): `input` float32 [input_rows, embedding_dim] is rounded
 * to fp16 after ONE power-of-two rescale per call (voltrix_launch_cast_f32_f16_scaled below: the reference's TF32 rounding
 * keeps the same 10 mantissa bits; fp32's exponent range is preserved) into `workspace`, the product runs on
 * v_mfma_f32_16x16x32_f16 with the default tile and the epilogue undoes the scale (exact).  What voltrix.spmm does for a
 * float32 `feat`.  workspace: voltrix_spmm_f32_workspace_bytes(input_rows, embedding_dim) bytes, device, 16-byte aligned,
 * owned by the caller (input_rows = rows of `input`: num_nodes for a square adjacency), need not be initialised and holds nothing
 * a later call depends on.  embedding_dim % 8 == 0.
 * voltrix_launch_spmm itself keeps exact fp32 products (3.6x slower on the reddit-like headline graph). */
int64_t voltrix_spmm_f32_workspace_bytes(int64_t input_rows, int embedding_dim);
void voltrix_launch_spmm_f32_as_f16(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                    int embedding_dim, void* input, int64_t input_rows, void* output, void* workspace,
                                    void* stream, int* return_code);

/* bfloat16 dense operand (extension; 8-bit mantissa, fp32's exponent range): input bfloat16 [*, embedding_dim], output
 * float32, v_mfma_f32_16x16x32_bf16.  Same tiles, shapes and arguments as the fp16 entry points. */
void voltrix_launch_spmm_bf16(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                              int embedding_dim, void* input, void* output, void* stream, int* return_code);
void voltrix_launch_spmm_bf16_tile(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                   int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                   void* window_order, void* out_scale, void* stream, int* return_code);

/* Schedule / output extensions of the 16-bit-operand launches (no reference counterpart; the math is that of
 * voltrix_launch_spmm_f16_tile):
 *   atomic_out  0: every element of output is stored.  1: the result is ADDED to output with float atomics
 *               (global_atomic_add_f32): the caller zero-fills output and lets the panel kernel (accumulate = 2) add its
 *               part in any order -- two addends per element, so the sum does not depend on the order.
 *   units       NULL, or a unit table int32[U][4] = {window, phase, stride, slot} (16-byte aligned) that replaces
 *               window_order: a unit runs the stages phase, phase + stride, ... (a stage = 4 TC blocks) of its window.
 *               A long window is cut into `stride` interleaved units of bounded length that each sweep the window's whole
 *               (sorted) column range: no wave runs a window several times the usual length (the tail of the launch), and
 *               units listed by length run in step and share gathered rows through L2.  slot < 0: the unit is the
 *               whole window (stride 1) and its result goes to output; slot >= 0: the unit's [16][embedding_dim] float32
 *               tile goes to partials + slot * 16 * embedding_dim, and voltrix_launch_combine_partials sums the tiles
 *               of each cut window in unit order (deterministic) into output (partials need not be initialised: every unit with a
 *               slot stores its whole tile, and only the slots of cut windows are read).  unit_ptr int32[9]: XCD x owns units
 *               [unit_ptr[x], unit_ptr[x+1]); max_units_per_xcd = the largest of those eight counts.  Every stage of
 *               every window must belong to exactly one unit.
 *   units_per_wave  1, or 2 with a unit table and fs <= 128 (several column slabs: fs = 128, slab-major order): every wave runs two consecutive units of the
 *               table, their stages alternating through one ring into two accumulator sets (same bits as 1): twice the
 *               windows sweep their sorted columns in step per CU at the same LDS and bytes in flight.  Measured beside the
 *               panel kernel on the reddit-like graph with units cut at 1.25 x the median: 1.365 -> 1.293 ms.  Ignored
 *               (= 1) where it does not apply.
 *   row_map     NULL, or int32[16 W]: row i of the handle is row row_map[i] of output (-1: a padding row, never
 *               written).  For handles built from a row-permuted CSR (locality reorder: rows that share columns grouped
 *               into the same 16-row windows -- the reference takes externally reordered graphs, bench/graph_gen.py:42-45):
 *               the product is written through the permutation, there is no un-permute pass, and because column ids are
 *               not relabelled `input` is the caller's B as it is.
 * Pointers of every block-format launch (voltrix_launch_spmm, _f16, _bf16, their _tile, _sched and _sched_ticket forms and
 * voltrix_launch_spmm_f32_as_f16): blk_offsets, input and output are required when num_nodes > 0 and embedding_dim > 0; hspa_packed and
 * hind may be empty (a graph without edges); window_order, out_scale, units, partials and row_map are optional; unit_ptr is required
 * with units.  A NULL required pointer, a misaligned input / hspa_packed / units (and, in the ticket form, output / tickets):
 * VOLTRIX_ERR_BAD_SHAPE on the host, before any launch -- voltrix_launch_spmm_f32_as_f16 answers so before it enqueues the cast. */
void voltrix_launch_spmm_f16_sched(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                   int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                   void* window_order, void* out_scale, int atomic_out, void* units, void* unit_ptr,
                                   int max_units_per_xcd, void* partials, void* row_map, int units_per_wave, void* stream,
                                   int* return_code);
void voltrix_launch_spmm_bf16_sched(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                    int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                    void* window_order, void* out_scale, int atomic_out, void* units, void* unit_ptr,
                                    int max_units_per_xcd, void* partials, void* row_map, int units_per_wave, void* stream,
                                    int* return_code);
/* cuts int32[num_cuts][4] = {window, first slot, units, 0} (16-byte aligned): output rows of `window` = (accumulate ?
 * output : 0) + partials[first slot] + partials[first slot + 1] + ... in that order.  Run it on the stream of the
 * launch that wrote the partials, after the join with the panel kernel when accumulate != 0.  embedding_dim % 4 == 0.
 * row_map as for the launch that wrote the partials (NULL: identity). */
void voltrix_launch_combine_partials(void* cuts, int num_cuts, void* partials, void* output, int num_nodes,
                                     int embedding_dim, int accumulate, void* row_map, void* stream, int* return_code);

/* Unit table of a handle (the `units` / `unit_ptr` / `cuts` arguments above), built on the device from blk_offsets alone,
 * in two phases around the one host read that sizes the outputs (no reference counterpart -- its equal-work scheduler,
 * spmm_kernels.cuh:499-540, is dead code; layout and rules: voltrix/unit_table.hpp, profiles/HISTORY.md section 3.2):
 *   phase 1  voltrix_launch_unit_table_count: header int32[8] (device) = {num_units U, num_cuts C, num_slots, max units per
 *            XCD, max_stages L, top (longest unit), 0, 0}.  max_stages <= 0: L = max(8, floor(1.5 x median stages per window)),
 *            on handles of fewer than 1024 windows at most max(8, ceil(all stages / 1024)) (unit_table.hpp).
 *            workspace: voltrix_unit_table_workspace_bytes(num_nodes) bytes, device, 16-byte aligned; it and the header need not be
 *            initialised (the launch clears the histogram and the statistics itself and writes every other array before reading it).
 *   (caller reads the header; allocates units int32[U][4], unit_ptr int32[9], cuts int32[C][4], partials
 *    float[num_slots * 16 * embedding_dim] and voltrix_unit_table_fill_workspace_bytes(U) bytes of fill workspace)
 *   phase 2  voltrix_launch_unit_table_fill: writes units, unit_ptr, cuts (every element); same workspace, untouched since
 *            phase 1; num_units / num_cuts / top as read from the header.  The fill workspace need not be initialised.
 * xcd_ptr: NULL, or device int32[9] = first window of every XCD's range (xcd_ptr[0] = 0, xcd_ptr[8] = ceil(num_nodes / 16),
 * non-decreasing; the same array in both phases): ranges of equal WORK instead of equal window counts, for graphs whose
 * stages per row vary along the rows (communities); a two-level host passes 32 x the panel kernel's xcd_ptr so that both
 * kernels keep a panel's rows on one XCD.  Speed only: the SpMM gives the same bits with any ranges.
 * The table depends on blk_offsets (and xcd_ptr) only (ties between units of equal length are broken by window, then unit
 * index), so a handle always gets the same table and the SpMM the same bits. */
int64_t voltrix_unit_table_workspace_bytes(int num_nodes);
int64_t voltrix_unit_table_fill_workspace_bytes(int64_t num_units);
void voltrix_launch_unit_table_count(void* blk_offsets, int num_nodes, int max_stages, void* xcd_ptr, void* workspace,
                                     void* header, void* stream, int* return_code);
void voltrix_launch_unit_table_fill(void* blk_offsets, int num_nodes, void* xcd_ptr, void* workspace, void* fill_workspace,
                                    int num_units, int num_cuts, int top, void* units, void* unit_ptr, void* cuts,
                                    void* stream, int* return_code);

/* Stream kernel (round 5; spmm_stream_kernels.hpp): the window format walked as a STREAM OF STAGES -- the kernel for graphs of
 * short windows (the reference's low-degree evaluation graphs, bench/plot.py:8).  Replaces the reference's one-CTA-per-window
 * dispatch (voltrix_spmm_forward_cuda, spmm_kernels.cuh:2003-2113, grids :2028,2058,2089) for them: a wave owns a RUN of
 * consecutive units (whole windows; a long window's interleaved pieces), one LDS ring that never drains at a window boundary,
 * every finished window stored from the loop with 16-byte stores.  16-bit binary operand, plain stores (every row of the output
 * is written; cut windows go through `partials` and voltrix_launch_combine_partials with accumulate = 0, row_map = NULL).
 *   tables      built by the library from the handle's three tensors, two phases around the host reads that size the outputs:
 *     voltrix_launch_stream_table_count: header int32[8] (device) = {num_units U, cut windows C, partial-tile slots, bound on
 *       the number of runs, run_cost, cut_stages, 0, 0}.  run_cost <= 0: clamp((stages + windows) / 9216, 6, 48) (six runs per
 *       wave slot of the chip); cut_stages <= 0: max(run_cost, the unit table's default L).  run_cost <= 128.
 *       workspace: voltrix_stream_table_workspace_bytes(num_nodes) bytes, device, 16-byte aligned; it, the header and the fill
 *       workspace of phase 2 need not be initialised.
 *     (caller reads the header; allocates units int32[U][8], cuts int32[C][4], runs int32[bound][4], run_ptr int32[9],
 *      header2 int32[4], partials float[slots * 16 * embedding_dim], voltrix_stream_table_fill_workspace_bytes(U) bytes)
 *     voltrix_launch_stream_table_fill: writes them all (every record of runs up to `bound`: the ones past R are zero);
 *       header2 = {runs R, max runs per XCD, oversized, 0} (the launch's
 *       max_runs_per_xcd); same workspace, untouched since phase 1; run_cost as read from the header: 2 .. 128, anything else is
 *       refused (kErrBadShape) -- a larger value would make runs of more than 64 units, which the kernel (one lane per unit of a
 *       run) cannot walk; `oversized` != 0 reports such a run should one ever be built: do not launch with that table.
 *     units[u] = {first TC block, end TC block of the window, 4 x stride, window, partial-tile slot or -1, stages, columns of the
 *     window's last TC block that carry an edge (0: a window without edges), 0}; runs[r] = {first unit, units (<= 64), stages,
 *     0}; run_ptr[x] .. run_ptr[x + 1] = the runs of XCD x (contiguous windows, equal cost).  The tables depend on the handle
 *     only: a handle always gets the same tables and the product the same bits.
 *   tile        (fs, depth, waves): fs 32 | 64 | 128 (the slab: embedding_dim <= 32 | <= 64 | wider), depth 2..4, waves 1 | 2;
 *               fs = 0 selects the default (fs by width, depth 2, waves 1).
 *   input_rows  rows of the dense operand (0: num_nodes); decides 32- or 64-bit row addressing and the slab launches. */
int64_t voltrix_stream_table_workspace_bytes(int num_nodes);
int64_t voltrix_stream_table_fill_workspace_bytes(int64_t num_units);
void voltrix_launch_stream_table_count(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int run_cost,
                                       int cut_stages, void* workspace, void* header, void* stream, int* return_code);
void voltrix_launch_stream_table_fill(void* blk_offsets, int num_nodes, void* workspace, void* fill_workspace, int num_units,
                                      int num_cuts, int run_bound, int run_cost, void* units, void* cuts, void* runs,
                                      void* run_ptr, void* header2, void* stream, int* return_code);
void voltrix_launch_spmm_stream_f16(void* hspa_packed, void* hind, int num_nodes, int embedding_dim, void* input,
                                    int64_t input_rows, void* output, void* units, void* runs, void* run_ptr,
                                    int max_runs_per_xcd, void* partials, void* out_scale, int fs, int depth, int waves,
                                    int slab_policy, void* stream, int* return_code);
void voltrix_launch_spmm_stream_bf16(void* hspa_packed, void* hind, int num_nodes, int embedding_dim, void* input,
                                     int64_t input_rows, void* output, void* units, void* runs, void* run_ptr,
                                     int max_runs_per_xcd, void* partials, void* out_scale, int fs, int depth, int waves,
                                     int slab_policy, void* stream, int* return_code);

/* "Balance" schedule for a handle: order_out int32[W] (device) lists the windows of every XCD range, inside chunks of
 * `chunk` (1..4096) consecutive windows, by descending TC-block count, so that co-resident waves sweep their sorted
 * columns at a similar pace and share gathered rows through L2.  Depends on blk_offsets only; results of the SpMM are
 * bit-identical with or without it.  Every element of order_out is written. */
void voltrix_launch_window_order(void* blk_offsets, int num_nodes, int chunk, void* order_out, void* stream,
                                 int* return_code);

/* Panel kernel: the shared-column half of the two-level condensed format (spmm_panel_kernels.hpp; no reference
 * counterpart).  A panel = waves * row_blocks * 16 consecutive rows; per panel the plan lists the columns referenced by
 * several of its rows, cut into k-steps of 32:
 *   panel_ptr  int32 [NP+1]                  first k-step of every panel, S = panel_ptr[NP]
 *   panel_cols int32 [32 * (S + 2)]          row of `input` per (k-step, k); unused slots repeat a real column; 2 k-steps
 *                                            of padding (valid row ids) at the end
 *   panel_bits uint32 [(S + 1) * waves * 64] word (k-step, wave v, lane 16 g + R), bit 16 (c & 1) + 4 j + (c >> 1) <=>
 *                                            edge (row 16 (row_blocks v + j) + R of the panel, column 8 g + c of the
 *                                            k-step), j < row_blocks, c < 8
 *   panel_order int32 [NP] or NULL           launch position -> panel
 * output [num_nodes, embedding_dim] float32: accumulate == 0 overwrites every row; 1 adds onto it (read-add-store: output
 * already holds the window kernel's result for the remaining edges); 2 adds with float atomics onto a pre-zeroed output that
 * the window kernel (atomic_out = 1) adds to as well, in any order.  input _Float16 (bfloat16 for _bf16) [*, embedding_dim], 16-byte
 * aligned, embedding_dim % 8 == 0.  Tile: fs in {32,64,128}, depth = ring slots, ksteps per ring slot in {1,2}, or
 * VOLTRIX_PANEL_KSTEPS_PIPELINED (17): one k-step per slot walked by the software-pipelined loop (fragment reads of one half of
 * the column slots under the MFMAs of the other half; same bits as ksteps = 1; what the library uses for 8 x 2 workgroups =
 * 256-row panels, the shape it picks when the panel kernel is the critical path -- voltrix/hybrid.py PANEL_DOMINATED_RATIO);
 * VOLTRIX_ERR_BAD_CONFIG if the combination is not instantiated; VOLTRIX_ERR_BAD_SHAPE for accumulate outside 0..2.
 * out_scale as for voltrix_launch_spmm_f16_tile.
 * input_rows = rows of `input` (0: num_nodes, a square adjacency); slab_policy: how an operand wider than the tile's fs is
 * launched -- -1 (VOLTRIX_SLAB_AUTO) one launch per 256-byte group of column slabs when such a group of `input`
 * (input_rows x 256 bytes) fits the 256 MiB Infinity Cache, else one grid over all slabs; 0 always one grid; 1 always the
 * launches.  Same bits either way.
 * xcd_ptr / max_panels_per_xcd: NULL / 0, or device int32[9] = first launch POSITION of every XCD's range (xcd_ptr[8] =
 * NP) and the length of the longest range (sizes the grid): ranges of equal work instead of ceil(NP / 8) positions each
 * (graphs with community structure: the k-steps per panel vary by community); panel_order must have been built with the same
 * xcd_ptr.  Speed only.
 * MEMORY REQUIREMENT of the atomic forms (accumulate == 2 here, atomic_out != 0 in voltrix_launch_spmm_*_sched): they use the
 * hardware's no-return global_atomic_add_f32, which is only defined on ordinary (coarse-grained) device memory -- hipMalloc,
 * torch's allocator.  On fine-grained or host-mapped output (hipHostMalloc, hipMallocManaged with fine-grained coherence) the
 * adds can be lost silently: give such outputs a device-memory staging buffer, or use accumulate 0 / 1. */
#define VOLTRIX_PANEL_KSTEPS_PIPELINED 17
void voltrix_launch_spmm_panel_f16(void* panel_ptr, void* panel_cols, void* panel_bits, void* panel_order, void* xcd_ptr,
                                   int max_panels_per_xcd, int num_nodes, int embedding_dim, void* input, int64_t input_rows, void* output,
                                   int accumulate, int fs, int depth, int waves, int row_blocks, int ksteps,
                                   int slab_policy, void* out_scale, void* stream, int* return_code);
void voltrix_launch_spmm_panel_bf16(void* panel_ptr, void* panel_cols, void* panel_bits, void* panel_order, void* xcd_ptr,
                                    int max_panels_per_xcd, int num_nodes, int embedding_dim, void* input, int64_t input_rows, void* output,
                                    int accumulate, int fs, int depth, int waves, int row_blocks, int ksteps,
                                    int slab_policy, void* out_scale, void* stream, int* return_code);

/* The same kernel over PARTS of panels (round 4; voltrix/hybrid.py::panel_parts builds the table, no reference counterpart).
 * A panel's k-step list is walked by ONE workgroup, so the longest panel is a critical path (a panel inside a dense
 * community carries 5-20 x the k-steps of the median panel).  parts int32 [num_parts][4] = {panel, first k-step inside the
 * panel, k-steps, slot} replaces panel_order: launch position -> a piece of at most a bounded number of k-steps.  slot < 0:
 * the panel is whole and its tile goes to `output` per `accumulate`, exactly as above.  slot >= 0: the panel is cut; every
 * piece STORES its tile to partials[slot] (float32 [slots][16 waves row_blocks][embedding_dim], per-call scratch that need not be
 * initialised) and
 * voltrix_launch_combine_panel_partials -- on the same stream, after this launch (and, for accumulate == 2, after the window
 * kernel has been joined) -- adds the pieces to `output` in slot order: a fixed order, whatever the pieces' timing.
 * xcd_ptr / max_parts_per_xcd as above, over part positions (NULL / 0: ranges of ceil(num_parts / 8)).
 *   cuts int32 [num_cuts][4] = {panel, first slot, pieces, 0};  panel_rows = 16 waves row_blocks;  accumulate 0: output rows
 *   of the cut panels = the sum; != 0: added onto output (plain read-add-store). */
void voltrix_launch_spmm_panel_parts_f16(void* panel_ptr, void* panel_cols, void* panel_bits, void* parts, int num_parts,
                                         void* xcd_ptr, int max_parts_per_xcd, void* partials, int num_nodes, int embedding_dim,
                                         void* input, int64_t input_rows, void* output, int accumulate, int fs, int depth,
                                         int waves, int row_blocks, int ksteps, int slab_policy, void* out_scale, void* stream,
                                         int* return_code);
void voltrix_launch_spmm_panel_parts_bf16(void* panel_ptr, void* panel_cols, void* panel_bits, void* parts, int num_parts,
                                          void* xcd_ptr, int max_parts_per_xcd, void* partials, int num_nodes, int embedding_dim,
                                          void* input, int64_t input_rows, void* output, int accumulate, int fs, int depth,
                                          int waves, int row_blocks, int ksteps, int slab_policy, void* out_scale, void* stream,
                                          int* return_code);
void voltrix_launch_combine_panel_partials(void* cuts, int num_cuts, void* partials, void* output, int num_nodes,
                                           int embedding_dim, int panel_rows, int accumulate, void* stream, int* return_code);

/* TICKET JOIN of the two-level step (no reference counterpart; protocol: voltrix/spmm_kernels.hpp "Ticket join"): the window
 * kernel and the panel kernel meet in `output` WITHOUT a zero fill.  tickets int32 [4 + ceil(num_nodes / 16)] (device memory,
 * 16-byte aligned) is zeroed by the caller at the start of every call (hipMemsetAsync of the whole buffer, before either
 * launch); word 0 is a sticky error word (nonzero after the call: a bounded wait ran out and the result is not to be
 * trusted), word 4 + b the ticket of rows [16 b, 16 b + 16).  Per 16-row block the FIRST of the two kernels stores its tile
 * (write-through 16-byte stores) and the second adds its own with float atomics -- half the atomics of the atomic join, the
 * same bits but for the sign of an exact zero.  The four launches of a call, all with the same `tickets`:
 *   voltrix_launch_spmm_*_sched_ticket          the window kernel (arguments of _sched; no window_order, no row_map)
 *   voltrix_launch_spmm_panel_ticket_*          the panel kernel, on the same or on another stream: panels whole
 *                                               (panel_order or NULL, parts NULL) or in pieces (parts; panel_order ignored)
 *   voltrix_launch_combine_partials_ticket      after BOTH kernels (join the streams first), when the unit table has cuts
 *   voltrix_launch_combine_panel_partials_ticket   after that, when the part table has cuts
 * The combine passes store a block whose ticket is still 0 (no kernel wrote it) and add otherwise.  Only for embedding_dim <= fs
 * of BOTH tiles (one column slab), embedding_dim % 8 == 0, a binary 16-bit operand and `output` on ordinary device memory (see
 * MEMORY REQUIREMENT above); VOLTRIX_ERR_BAD_SHAPE otherwise. */
void voltrix_launch_spmm_f16_sched_ticket(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                          int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                          void* out_scale, void* units, void* unit_ptr, int max_units_per_xcd, void* partials,
                                          int units_per_wave, void* tickets, void* stream, int* return_code);
void voltrix_launch_spmm_bf16_sched_ticket(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, int num_edges,
                                           int embedding_dim, void* input, void* output, int fs, int depth, int waves,
                                           void* out_scale, void* units, void* unit_ptr, int max_units_per_xcd, void* partials,
                                           int units_per_wave, void* tickets, void* stream, int* return_code);
void voltrix_launch_combine_partials_ticket(void* cuts, int num_cuts, void* partials, void* output, int num_nodes,
                                            int embedding_dim, void* tickets, void* stream, int* return_code);
void voltrix_launch_spmm_panel_ticket_f16(void* panel_ptr, void* panel_cols, void* panel_bits, void* panel_order, void* parts,
                                          int num_parts, void* xcd_ptr, int max_per_xcd, void* partials, void* tickets,
                                          int num_nodes, int embedding_dim, void* input, int64_t input_rows, void* output, int fs,
                                          int depth, int waves, int row_blocks, int ksteps, int slab_policy, void* out_scale,
                                          void* stream, int* return_code);
void voltrix_launch_spmm_panel_ticket_bf16(void* panel_ptr, void* panel_cols, void* panel_bits, void* panel_order, void* parts,
                                           int num_parts, void* xcd_ptr, int max_per_xcd, void* partials, void* tickets,
                                           int num_nodes, int embedding_dim, void* input, int64_t input_rows, void* output, int fs,
                                           int depth, int waves, int row_blocks, int ksteps, int slab_policy, void* out_scale,
                                           void* stream, int* return_code);
void voltrix_launch_combine_panel_partials_ticket(void* cuts, int num_cuts, void* partials, void* output, int num_nodes,
                                                  int embedding_dim, int panel_rows, void* tickets, void* stream,
                                                  int* return_code);

/* Builders of the two schedules above, on the device (round 4; voltrix/schedule_tables.hpp; the Python host's
 * voltrix/schedule.py::split_equal_work and voltrix/hybrid.py::panel_parts are their torch-tensor restatements).
 * XCD ranges: xcd_ptr int32[9] <- b[0] = 0 <= ... <= b[8] = n such that the eight ranges of the items' work have about equal
 * sums (boundary = the index whose prefix sum is nearest to ceil(total x / 8), rounded up to `align`; total 0: ceil(n / 8)
 * items each).  _of_work: work int32[num_items]; _of_windows: the stages of a handle's windows (work of window w =
 * ceil(TC blocks / 4)), n = ceil(num_nodes / 16); _of_panels: work of panel p = round(kstep_cost_x10 / 10 x its k-steps) +
 * the stages of its panel_rows / 16 windows in resid_blk_offsets (the Python host passes 66: a k-step costs a CU about 6.6
 * residual stages), and window_xcd_ptr int32[9] (or NULL) <- the same ranges in windows, for the residual's unit table.
 * One workgroup each; stream-ordered, no host read.  All nine elements of xcd_ptr (and of window_xcd_ptr) are written, nothing of
 * them is read. */
void voltrix_launch_xcd_ranges_of_work(void* work, int num_items, int align, void* xcd_ptr, void* stream, int* return_code);
void voltrix_launch_xcd_ranges_of_windows(void* blk_offsets, int num_nodes, int align, void* xcd_ptr, void* stream,
                                          int* return_code);
void voltrix_launch_xcd_ranges_of_panels(void* panel_ptr, void* resid_blk_offsets, int num_nodes, int panel_rows,
                                         int kstep_cost_x10, void* xcd_ptr, void* window_xcd_ptr, void* stream,
                                         int* return_code);
/* Piece table, two phases around the host read that sizes it.  count: header int32[8] <- {pieces, cut panels, partial-tile
 * slots, pieces in the longest XCD range, cap, 0, 0, 0}; fill (same panel_ptr / cap / panel_xcd_ptr / workspace, untouched in
 * between): parts int32[pieces][4], part_xcd_ptr int32[9], cuts int32[max(1, cut panels)][4] as described above -- panels
 * of more than `cap` k-steps in ceil(k-steps / cap) contiguous pieces of nearly equal length; per XCD range (panel_xcd_ptr in
 * panel units, or NULL = ceil(num_panels / 8) panels each) longest first, ties by (panel, piece).  workspace: 16-byte aligned,
 * voltrix_panel_parts_workspace_bytes(num_panels) bytes; it and the header need not be initialised (the count call writes all of both).
 * Every element of parts and part_xcd_ptr and one row of cuts per cut panel are written; without a cut panel the one row of cuts is
 * neither written nor read. */
int64_t voltrix_panel_parts_workspace_bytes(int num_panels);
void voltrix_launch_panel_parts_count(void* panel_ptr, int num_panels, int cap, void* panel_xcd_ptr, void* workspace,
                                      void* header, void* stream, int* return_code);
void voltrix_launch_panel_parts_fill(void* panel_ptr, int num_panels, int cap, void* panel_xcd_ptr, void* workspace,
                                     void* parts, void* part_xcd_ptr, void* cuts, void* stream, int* return_code);

/* The two-level format in ONE launch (spmm_fused_kernels.hpp; round 3, rebuilt in round 4).  One 256-thread workgroup per
 * 512-row panel -- four waves, one per SIMD, eight 16-row blocks each; the plan keeps its waves = 8 x row_blocks = 4 layout --
 * computes the whole product for its rows: the shared columns from the panel plan (arrays as for
 * voltrix_launch_spmm_panel_f16) and the residual edges from per-wave streams of stage records, into the same accumulators;
 * output [num_nodes, embedding_dim] float32 is written once with plain stores (every row; no zero fill, no atomics, no
 * second stream, no combine pass; the summation order is fixed, so results are run-to-run identical).
 *   wave_ptr int32 [4 NP + 1]    first record of (panel p, wave v) at index 4 p + v; wave v owns windows 32 p + 8 v + j, j < 8
 *   records  uint32 [R + 1][64]  16-byte aligned; one record = one stage (4 TC blocks = 32 condensed columns) of ONE of the
 *                                wave's windows: words 0..31 rows of `input` (unused columns repeat a real one), 32..47 the
 *                                stage's 16 bitmap words (hspa_packed order), word 48 = j; a wave's records are sorted by
 *                                their first column; one record of padding at the end.  Built from the block-format handle of
 *                                the residual matrix by voltrix_launch_fused_records_* below.
 * Tile: fs in {32,64,128}, depth = slots of the shared panel ring (3, or 4 below fs 128); VOLTRIX_ERR_BAD_CONFIG otherwise.
 * pace_blocks: 0 / 1 = none; n > 1 (one column slab only) = the workgroups that share an XCD and a dispatch generation wait
 * for each other at n points of their column sweep (bounded polls on counters the library keeps: advisory, the result never
 * depends on it) so that an XCD's resident rows sweep the sorted columns together and share gathered rows through its L2.
 * input / out_scale / xcd_ptr / max_panels_per_xcd as for voltrix_launch_spmm_panel_f16. */
void voltrix_launch_spmm_fused_f16(void* panel_ptr, void* panel_cols, void* panel_bits, void* panel_order, void* xcd_ptr,
                                   int max_panels_per_xcd, void* wave_ptr, void* records, int num_nodes, int embedding_dim, void* input,
                                   void* output, int fs, int depth, int pace_blocks, void* out_scale, void* stream,
                                   int* return_code);
void voltrix_launch_spmm_fused_bf16(void* panel_ptr, void* panel_cols, void* panel_bits, void* panel_order, void* xcd_ptr,
                                    int max_panels_per_xcd, void* wave_ptr, void* records, int num_nodes, int embedding_dim, void* input,
                                    void* output, int fs, int depth, int pace_blocks, void* out_scale, void* stream,
                                   int* return_code);

/* Builder of the stage records above (fused_plan.hpp): block-format handle of the RESIDUAL matrix (the handle of
 * resid_node_pointer / resid_edge_list from the plan builder below, through voltrix_launch_csr_window_count / _fill) ->
 * (wave_ptr, records), in two phases because the caller owns every buffer:
 *   phase 1  voltrix_launch_fused_records_count: wave_ptr int32 [4 NP + 1] (NP = ceil(num_nodes / 512)), every element written;
 *            workspace: voltrix_fused_records_workspace_bytes(num_nodes) bytes, device, 16-byte aligned, need not be initialised
 *   (caller reads R = wave_ptr[4 NP] and allocates records uint32 [(R + 1) * 64], 16-byte aligned)
 *   phase 2  voltrix_launch_fused_records_fill: every word of records is written (the padding record is zero).
 * Once the records exist the residual handle is no longer needed by voltrix_launch_spmm_fused_*. */
/* How the one-launch kernel splits a 512-row panel: waves per workgroup (4) x 16-row blocks per wave (8).  wave_ptr has
 * waves * NP + 1 entries; hosts size it from THIS call, not from a constant of their own. */
void voltrix_fused_panel_geometry(int* waves, int* row_blocks);
int64_t voltrix_fused_records_workspace_bytes(int num_nodes);
void voltrix_launch_fused_records_count(void* blk_offsets, void* hspa_packed, int num_nodes, void* workspace, void* wave_ptr,
                                        void* stream, int* return_code);
void voltrix_launch_fused_records_fill(void* blk_offsets, void* hspa_packed, void* hind, int num_nodes, void* wave_ptr,
                                       int64_t num_records, void* records, void* stream, int* return_code);

/* Builder of the panel plan (panel_plan.hpp): CSR on the DEVICE (rows sorted, duplicate-free, ids in [0, num_cols),
 * num_cols <= 2^22) -> residual CSR + plan, in two phases because the caller owns every buffer:
 *   phase 1  voltrix_launch_panel_plan_count: panel_ptr int32[NP+1], resid_node_pointer int32[num_nodes+1], status[1];
 *            workspace: voltrix_panel_plan_workspace_bytes(...) bytes, device, 16-byte aligned, need not be initialised (the launch
 *            clears all of it); every element of the three outputs is written
 *   (caller reads S = panel_ptr[NP], E_r = resid_node_pointer[num_nodes] and status[0] -- the number of input
 *    violations, must be 0 -- and allocates resid_edge_list int32[E_r], panel_cols int32[32 (S + 2)],
 *    panel_bits uint32[(S + 1) * waves * 64])
 *   phase 2  voltrix_launch_panel_plan_fill: same arguments and workspace; every output element is written.
 * A column is shared in a panel when >= tau (1..65535) of the panel's rows reference it; waves in {4, 8}, row_blocks in
 * {2, 4}.  VOLTRIX_ERR_BAD_CONFIG: column universe above 2^22 (the two-level format is not built for it). */
int64_t voltrix_panel_plan_workspace_bytes(int num_nodes, int waves, int row_blocks);
void voltrix_launch_panel_plan_count(void* node_pointer, void* edge_list, int num_nodes, int num_cols, int64_t num_edges,
                                     int waves, int row_blocks, int tau, void* workspace, void* panel_ptr,
                                     void* resid_node_pointer, void* status, void* stream, int* return_code);
void voltrix_launch_panel_plan_fill(void* node_pointer, void* edge_list, int num_nodes, int num_cols, int64_t num_edges,
                                    int waves, int row_blocks, int tau, void* workspace, void* panel_ptr,
                                    void* resid_node_pointer, int64_t total_ksteps, void* resid_edge_list,
                                    void* panel_cols, void* panel_bits, void* stream, int* return_code);

/* `panel_order` of the panel launches: order_out int32[num_panels] (device), position -> panel; inside every XCD's range of
 * positions (xcd_ptr int32[9] on the device, or NULL: ceil(num_panels / 8) each), groups of `group` consecutive panels (neighbours share their band columns: side by side
 * they share gathered rows through L2), the groups with the most k-steps first (ties by index), natural order inside a
 * group; group = 1: plain longest-first (what the Python host uses: groups of 4 gained 3 % on the bare kernel pair, nothing
 * through the operator).  Speed only.  Every element of order_out is written (a permutation inside every range). */
void voltrix_launch_panel_order(void* panel_ptr, int num_panels, int group, void* xcd_ptr, void* order_out, void* stream,
                                int* return_code);

/* Default tile for a feature width; is_f16 selects the operand type.  Always succeeds. */
void voltrix_spmm_default_tile(int embedding_dim, int is_f16, int* fs, int* depth, int* waves);

/* Number of instantiated tiles and the i-th one (for autotuners that enumerate the ahead-of-time space). */
int voltrix_spmm_num_tiles(int is_f16);
void voltrix_spmm_tile_at(int is_f16, int index, int* fs, int* depth, int* waves);

/* fp32 -> fp16 cast of the dense operand into a caller-provided buffer (count % 8 == 0).  src and dst: 16-byte aligned, required when
 * count > 0 (VOLTRIX_ERR_BAD_SHAPE on the host, before any launch, otherwise); count == 0: VOLTRIX_OK, nothing is launched. */
void voltrix_launch_cast_f32_f16(void* src, void* dst, int64_t count, void* stream, int* return_code);

/* Range-safe variant (what voltrix.spmm uses for fp32 features): dst = fp16(src * 2^-e) with one power-of-two scale
 * per call, e = exponent(max |src|) - 14, so fp32 magnitudes beyond fp16's range neither overflow nor flush while the
 * 10-bit mantissa (= the reference's TF32 rounding, spmm_kernels.cuh:1671) is kept.  scale: device float[2], 8-byte
 * aligned; scale[0] <- 2^e, to be passed as `out_scale` of voltrix_launch_spmm_f16_tile (multiplied into every output
 * element in the epilogue; exact).  No host sync.  Inf / NaN in src: scale 1, they propagate as in fp32.  Neither dst nor scale
 * need be initialised: scale[1] is scratch (the bits of max |src|), the head of dst briefly holds one word per workgroup of the
 * reduction -- both are written before they are read -- and the conversion then writes every element of dst.  src and dst: 16-byte
 * aligned, required when count > 0; scale: always required (count == 0 still writes scale[0] = 1); anything else is
 * VOLTRIX_ERR_BAD_SHAPE on the host, before any launch. */
void voltrix_launch_cast_f32_f16_scaled(void* src, void* dst, int64_t count, void* scale, void* stream,
                                        int* return_code);

/* CSR row-gather kernel (round 6; spmm_csr_kernels.hpp): output[i, :] = sum over the entries of row i of input[indices[e], :],
 * straight from a DEVICE CSR (int32 indptr[num_rows + 1], indices[nnz]; binary A: entries count as 1, a duplicate (row, col) entry
 * counts TWICE here -- callers with duplicates keep to the block format, which counts it once like the reference's bitmaps,
 * bmat_kernels.cuh:100-103).  dtype 0 fp32 / 1 fp16 / 2 bfloat16 rows of `input` (embedding_dim a multiple of 16 bytes), fp32
 * `output` [num_rows, embedding_dim], every row written; exact products, fp32 sum in entry order.  No workspace, no tables.
 * xcd_ranges: 0 = consecutive row groups go round the XCDs (default), 1 = every XCD owns a contiguous eighth of the rows.  The
 * operator takes it for handles of short windows where it measured faster than the block-format kernels (fp32 features; wide
 * operands): voltrix/spmm/spmm.py.  No reference counterpart (the reference has the block format only).
 * Alignment: input and output 16 bytes -- rows are read and written 16 bytes per lane, anything else is VOLTRIX_ERR_BAD_SHAPE on the
 * host, before any launch; indptr, indices (and values below) 4 bytes suffice: 4-byte loads. */
void voltrix_launch_spmm_csr_rows(void* indptr, void* indices, int num_rows, int embedding_dim, void* input, int dtype, void* output,
                                  int xcd_ranges, void* stream, int* return_code);

/* The same kernel with edge values: output = csr(values) * input, values = device float[nnz] in CSR order (duplicate entries ADD, as in
 * torch.sparse.mm).  One fused multiply-add per element in fp32: with fp32 rows the weighted product is exact up to the rounding of
 * the sum (deg * 2^-23 (|A| |B|)) -- the block format's value planes are 16-bit.  Values can change between calls at no cost (nothing is
 * preprocessed).  voltrix/weighted.py takes it for general values on handles of short windows where it measured faster, and for
 * VOLTRIX_FP32_MODE=exact.  No reference counterpart (the reference has no edge values: spmm_kernels.cuh:1632-1644). */
void voltrix_launch_spmm_csr_rows_weighted(void* indptr, void* indices, void* values, int num_rows, int embedding_dim, void* input, int dtype,
                                           void* output, int xcd_ranges, void* stream, int* return_code);

/* New edge values on a fixed pattern: plane[slots[e]] = T(values[e]) for e < count; values device float[count], slots device int64[count]
 * (the element of the flat value plane [T * 128] every CSR entry lands on: voltrix/weighted.py::edge_slots; the entries of a
 * duplicate-free pattern own their elements), plane of dtype 0 fp32 / 1 fp16 / 2 bfloat16 (round to nearest even).  One pass instead
 * of rebuilding the plane (sorts and searches over all edges).  No reference counterpart. */
void voltrix_launch_scatter_values(void* values, void* slots, void* plane, int64_t count, int dtype, void* stream, int* return_code);

/* Sampled dense-dense product (sddmm_kernels.hpp): out[e] = sum_k x[row_e, k] * y[indices[e], k] for every entry e < nnz of a DEVICE CSR
 * (int32 indptr[num_rows + 1], indices[nnz]), row_e = the row whose indptr range holds e; out = device float[nnz] in CSR order, every
 * element written (duplicate entries each get the same value).  x [num_rows, embedding_dim] and y [*, embedding_dim] row-major, 16-byte
 * aligned; dtype pairs (x_dtype, y_dtype), codes 0 fp32 / 1 fp16 / 2 bfloat16: (0, 1), (0, 2), (1, 1), (2, 2), (0, 0); embedding_dim a
 * multiple of 8 when either is 16-bit, else of 4.  fp32 products and sum, one fused multiply-add per element, in an order fixed by
 * embedding_dim alone: |out - ref| <= embedding_dim * 2^-23 (|x| |y|)[e], the same bits on every launch.  The gradient of a weighted
 * SpMM with respect to its edge values (dv = sddmm(dC, B)) and attention scores.  VOLTRIX_ERR_BAD_SHAPE: negative sizes, a bad width, an
 * unsupported pair, a null or misaligned pointer; VOLTRIX_OK without a launch for nnz == 0 or embedding_dim == 0.  No reference
 * counterpart (the reference is forward-only and has no edge values).
 * Alignment: x and y 16 bytes, anything else is VOLTRIX_ERR_BAD_SHAPE on the host, before any launch; indptr, indices and out 4 bytes
 * suffice: 4-byte loads, and out is stored one float at a time, so nothing beyond out[nnz - 1] is written. */
void voltrix_launch_sddmm_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int embedding_dim, void* x, int x_dtype, void* y,
                              int y_dtype, void* out, void* stream, int* return_code);

/* Edge softmax (edge_softmax_kernels.hpp): alpha[e] = exp(z_e - m_r) / sum_{e' in row r} exp(z_e' - m_r), z = scale * scores, m_r the
 * row maximum, for every entry e < nnz of a DEVICE CSR (int32 indptr[num_rows + 1]); scores and out = device float[nnz] in CSR order,
 * every element written.  The step between attention scores (voltrix_launch_sddmm_csr) and the aggregation with them
 * (voltrix_launch_spmm_csr_rows_weighted).  Special values: z = -inf gives 0; a row whose entries are all -inf gets zeros, not NaN
 * (unlike torch.softmax); a NaN makes its own row NaN and no other; scale = 0 gives
 * 1 / (the row's entries that are not -inf) to each of them.  Accuracy, with deg_r the row's entries and ref the exact softmax:
 * |alpha - ref| <= ref * 2 (deg_r + |z_e - m_r| + 2) 2^-23 + 2^-126.  Deterministic: no float atomics, sums in an order fixed by
 * the pattern, the same bits on every launch.  Three kernel launches on `stream`, no host synchronisation; workspace: device, 16-byte
 * aligned, voltrix_edge_softmax_workspace_bytes(num_rows, nnz) bytes (a function of nnz alone), reused by the backward; it need not
 * be initialised and carries nothing from one call to the next (every call writes the chunk rows and partials it reads).
 * VOLTRIX_ERR_BAD_SHAPE: negative sizes, nnz > INT_MAX, a non-finite scale, a null or misaligned pointer; VOLTRIX_OK without a launch
 * for nnz == 0.  No reference counterpart (the reference is forward-only and has no edge values).
 * Alignment: indptr, scores and out 4 bytes suffice (the backward's alpha, grad_alpha and grad_scores likewise): a thread moves its 8
 * edges with 16-byte loads / stores when the tensor's base allows and with 4-byte ones when it does not -- the same values, the same
 * bits -- and never writes past out[nnz - 1]; workspace 16 bytes.  Anything less is VOLTRIX_ERR_BAD_SHAPE on the host, before any launch. */
int64_t voltrix_edge_softmax_workspace_bytes(int num_rows, int64_t nnz);
void voltrix_launch_edge_softmax_csr(void* indptr, int num_rows, int64_t nnz, void* scores, float scale, void* out, void* workspace,
                                     void* stream, int* return_code);

/* Its backward: grad_scores[e] = scale * alpha[e] * (grad_alpha[e] - sum_{e' in row r} alpha[e'] * grad_alpha[e']), alpha from the
 * forward, all device float[nnz] in CSR order; rows of zeros (all -inf) get zero gradients.  With D_r = sum alpha g and
 * A_r = sum alpha |g|: |grad - ref| <= |scale| alpha_e (2 |g_e - D_r| + (deg_r + 2) A_r) 2^-23 + 2^-126.  Same workspace, checks and
 * determinism as the forward. */
void voltrix_launch_edge_softmax_backward_csr(void* indptr, int num_rows, int64_t nnz, void* alpha, void* grad_alpha, float scale,
                                              void* grad_scores, void* workspace, void* stream, int* return_code);

/* Multi-head forms of the three attention operators (sddmm_heads_kernels.hpp, edge_softmax_heads_kernels.hpp,
 * spmm_csr_heads_kernels.hpp).  Layouts: node tensors [n, heads, head_dim] row-major (rows of heads * head_dim, 16-byte aligned), edge
 * tensors device float[nnz, heads] in CSR order with the head index fastest.  Per head each computes what its single-head entry point
 * computes on the head's contiguous slice, to the bit, within the same bounds (head_dim in place of embedding_dim); one index read and
 * one gathered row per edge serve all heads.  Element offsets are 64-bit; nnz <= INT_MAX, heads * head_dim <= INT_MAX.
 * VOLTRIX_ERR_BAD_SHAPE from each, on the host and before any launch: heads < 1, negative sizes, head_dim not a multiple of 16 bytes of
 * the gathered operand (8 for 16-bit, 4 for fp32), a dtype or pair outside the single-head set, a null or misaligned pointer;
 * VOLTRIX_OK without a launch when there is nothing to do.  No reference counterpart.
 * Alignment: the gathered node tensors (x, y; input) and the node-shaped output of voltrix_launch_spmm_csr_heads 16 bytes, required and
 * rejected otherwise; every edge tensor (out of the product, scores / alpha / grad_alpha / out of the softmax, values), indptr and indices
 * 4 bytes suffice: they are read and written one float at a time; the softmax's workspace 16 bytes.
 *
 * out[e, h] = sum_d x[row_e, h, d] * y[indices[e], h, d]; dtype pairs of voltrix_launch_sddmm_csr. */
void voltrix_launch_sddmm_heads_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, int head_dim, void* x, int x_dtype,
                                    void* y, int y_dtype, void* out, void* stream, int* return_code);

/* out[:, h] = edge softmax of scale * scores[:, h] for every head, special values per head (a NaN or a row of -inf stays in its own
 * row and its own head); three launches, deterministic, no host synchronisation.  Workspace: device, 16-byte aligned,
 * voltrix_edge_softmax_heads_workspace_bytes(num_rows, nnz, heads) bytes -- a function of (nnz, heads) alone; heads == 1: the single-head
 * size -- shared with the backward: grad_scores = scale * alpha * (grad_alpha - rowsum(alpha * grad_alpha)) per head. */
int64_t voltrix_edge_softmax_heads_workspace_bytes(int num_rows, int64_t nnz, int heads);
void voltrix_launch_edge_softmax_heads_csr(void* indptr, int num_rows, int64_t nnz, int heads, void* scores, float scale, void* out,
                                           void* workspace, void* stream, int* return_code);
void voltrix_launch_edge_softmax_heads_backward_csr(void* indptr, int num_rows, int64_t nnz, int heads, void* alpha, void* grad_alpha,
                                                    float scale, void* grad_scores, void* workspace, void* stream, int* return_code);

/* output[r, h, :] = sum_{e in row r} values[e, h] * input[indices[e], h, :]: fp32 / fp16 / bf16 input (dtype 0 / 1 / 2), fp32 values
 * [nnz, heads] and output [num_rows, heads, head_dim]; fp32 products, one fused multiply-add per element, summed in CSR order; every
 * row written, empty rows zero.  No value planes and no block-format handle.  VOLTRIX_OK without a launch for num_rows == 0 or
 * head_dim == 0. */
void voltrix_launch_spmm_csr_heads(void* indptr, void* indices, void* values, int num_rows, int heads, int head_dim, void* input,
                                   int dtype, void* output, void* stream, int* return_code);

/* GAT edge scores (gat_score_kernels.hpp): out[e, h] = leaky_relu(el[row_e, h] + er[indices[e], h], slope) for every entry e < nnz of a
 * DEVICE CSR (int32 indptr[num_rows + 1], indices[nnz]); el = device float[num_rows, heads], er = device float[*, heads] (gathered by
 * indices), out = device float[nnz, heads] in CSR order with the head index fastest, every element written (duplicate entries are
 * edges of their own).  z = el + er is one fp32 add; z > 0 gives z, anything else (z == 0 and NaN included, as torch's leaky_relu)
 * float(slope) * z.  slope: any finite float (1: the plain sum; 0: ReLU; negative allowed).  Against float64 from the fp32 inputs:
 * |out - ref| <= 1.5 * 2^-23 |ref| + 2^-149, and 2^-24 |ref| + 2^-149 when slope is 1 or a power of two; the sign of z is the sign of
 * the exact sum.  A NaN or +-inf in el[r, h] reaches only row r's entries of head h.  One launch split by edges (`indices` is read once
 * per edge), no workspace, no host synchronisation, 64-bit element offsets.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: heads < 1 or > 65535, negative sizes, nnz > INT_MAX, nnz > 0 with
 * num_rows == 0, heads * num_rows > INT_MAX, a non-finite slope, a null or misaligned (4 bytes) pointer; VOLTRIX_OK without a launch
 * for nnz == 0.  No reference counterpart (the reference is forward-only and has no edge values).
 * Alignment: 4 bytes suffice for every pointer.  heads == 4 / 8 move 16 bytes per lane when el, er and out all sit on 16 bytes and take
 * the any-heads kernel (4-byte accesses, the same two rounded operations per element: the same bits) when one does not; a thread reads
 * its 8 column ids (and the row sum its 8 `order` entries) with two 16-byte loads when the array's base allows, else one by one. */
void voltrix_launch_gat_score_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, void* el, void* er, float slope,
                                  void* out, void* stream, int* return_code);

/* The segment sum of its backward: out[r, h] = sum_{e in row r} gz, gz = z > 0 ? g : float(slope) * g with
 * z = a[r, h] + b[indices[e], h] and g = grad[order ? order[e] : e, h]; out = device float[num_rows, heads], every element written,
 * empty rows 0.  d_el is this on the CSR with (a, b) = (el, er) and order = NULL; d_er is this on the transposed CSR
 * (voltrix_launch_csr_transpose) with (a, b) = (er, el) and order = device int32[nnz], the entry of the CSR that entry e of the
 * transpose is: fp32 addition commutes, so the gate is the forward's decision to the bit.  Every term is g or one rounded product and a
 * row of deg entries has deg - 1 additions in an order fixed by the pattern alone:
 * |out - ref| <= deg * 2^-23 * sum |gz| + 2^-149 per row and head.  Deterministic: no float atomics, the same bits on every launch, and
 * out[:, h] of a call with `heads` heads has the bits of the single-head call on the contiguous slices a[:, h], b[:, h], grad[:, h].  A
 * NaN in grad[e, h] reaches only the one sum that holds it.  Three launches (zero fill, chunk sums, merge of the rows that cross a chunk
 * of 2048 edges), split by edges so a hub row costs what its edges cost; no host synchronisation.  workspace: device, 16-byte aligned,
 * voltrix_gat_score_workspace_bytes(num_rows, nnz, heads) bytes -- a function of (nnz, heads) alone, a multiple of 16, 0 for nnz == 0;
 * it need not be initialised (partials are read only for rows that cross a chunk boundary, and those are written by the same call).
 * The checks of voltrix_launch_gat_score_csr -- 4 bytes suffice for indptr, indices, order, a, b, grad and out (one float at a time);
 * workspace 16 bytes, required --; nnz == 0 zero-fills out (num_rows > 0 then needs a valid out) and is VOLTRIX_OK. */
int64_t voltrix_gat_score_workspace_bytes(int num_rows, int64_t nnz, int heads);
void voltrix_launch_gat_score_rowsum_csr(void* indptr, void* indices, void* order, int num_rows, int64_t nnz, int heads, void* a, void* b,
                                         void* grad, float slope, void* out, void* workspace, void* stream, int* return_code);

/* GATv2 edge scores (gatv2_score_kernels.hpp): out[e, h] = sum_d a[h, d] * leaky(xl[row_e, h, d] + xr[indices[e], h, d]) for every
 * entry e < nnz of a DEVICE CSR, leaky(z) = z > 0 ? z : float(slope) * z (z == 0 and NaN take the slope branch).  xl = device
 * [num_rows, heads, head_dim], xr = device [*, heads, head_dim] (gathered by indices), one type for both: dtype 0 fp32 / 1 fp16 /
 * 2 bfloat16, rows 16-byte aligned; a = device float[heads, head_dim], 16-byte aligned; out = device float[nnz, heads] in CSR order with
 * the head index fastest, every element written (duplicate entries are edges of their own).  Per element one fp32 add, one product with
 * slope on the slope branch and one fused multiply-add into the sum, in an order fixed by head_dim alone:
 * |out - ref| <= (head_dim + 2) * 2^-23 * sum_d |a_d| |leaky(z_d)| + 2^-149 against float64 from the inputs as stored, and out[:, h]
 * has the bits of the single-head call on the contiguous slices.  Nothing of size [nnz, heads, head_dim] exists.  One launch split by
 * edges, no workspace, no host synchronisation, 64-bit element offsets.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: heads < 1, negative sizes, nnz > INT_MAX, heads * head_dim > INT_MAX, nnz > 0
 * with num_rows == 0, head_dim not a multiple of 16 bytes of xr (8 for 16-bit, 4 for fp32), an unknown dtype, a non-finite slope, a
 * null or misaligned pointer (4 bytes for indptr, indices, out; 16 for xl, xr, a); VOLTRIX_OK without a launch for nnz == 0 or
 * head_dim == 0.  No reference counterpart (the reference is forward-only and has no edge values). */
void voltrix_launch_gatv2_score_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, int head_dim, void* xl, void* xr,
                                    int dtype, void* a, float slope, void* out, void* stream, int* return_code);

/* The gated row sum of its backward: out[r, h, d] = sum_{e in row r} (p[r, h, d] + q[indices[e], h, d] > 0 ? g : float(slope) * g) with
 * g = grad[order ? order[e] : e, h]; p, q as xl, xr above, grad = device float[nnz, heads], out = device float[num_rows, heads,
 * head_dim], 16-byte aligned, every row written, empty rows 0.  G_l is this on the CSR with (p, q) = (xl, xr) and order = NULL; G_r is
 * this on the transposed CSR (voltrix_launch_csr_transpose) with (p, q) = (xr, xl) and order = device int32[nnz], the entry of the CSR
 * that entry e of the transpose is: fp32 addition commutes, so the gate is the forward's decision to the bit.  Then d_xl = a * G_l,
 * d_xr = a * G_r and d_a = sum_r xl * G_l + sum_c xr * G_r are dense.  Every term is g or one rounded product, summed in CSR edge order:
 * |out - ref| <= deg * 2^-23 * sum_e |term_e| + 2^-149 per element; a NaN in grad[e, h] reaches only out[row_e, h, :].  One launch, a
 * row per lane group (a hub row serialises its wave, as in voltrix_launch_spmm_csr_heads), no workspace, no float atomics, no host
 * synchronisation.  The checks above, and grad 4-byte, out 16-byte aligned; VOLTRIX_OK without a launch for num_rows == 0 or
 * head_dim == 0; with nnz == 0 every row is zero-filled and indices, q, grad are not read. */
void voltrix_launch_gatv2_rowsum_csr(void* indptr, void* indices, void* order, int num_rows, int64_t nnz, int heads, int head_dim, void* p,
                                     void* q, int dtype, void* grad, float slope, void* out, void* stream, int* return_code);

/* Edge softmax and multi-head aggregation in one launch (attn_aggregate_kernels.hpp):
 * out[r, h, :] = sum_{e in row r} alpha[e, h] * feat[indices[e], h, :] with alpha the softmax of scale * scores[:, h] over every row of a
 * DEVICE CSR, never stored.  scores = device float[nnz, heads] in CSR order with the head index fastest; feat = device
 * [*, heads, head_dim], dtype 0 fp32 / 1 fp16 / 2 bfloat16; out = device float[num_rows, heads, head_dim]; m, l = device
 * float[num_rows, heads]: m = the row maximum of sign(scale) * scores (-inf for a row without entries), l = sum exp(|scale| *
 * (sign(scale) * scores - m)).  Every element of out, m and l is written; rows without entries and rows or heads whose scores are all
 * -inf give zeros and l = 0; a NaN or +inf score stays in its own row and head; scale = 0 is the mean over the entries that are not
 * -inf; the special values of voltrix_launch_spmm_csr_heads on voltrix_launch_edge_softmax_heads_csr.  Per row two passes (the maximum,
 * then fused multiply-adds of exp(.) * feat and the sum l in CSR edge order) and one reciprocal:
 * |out - ref| <= 2 (deg + 3) 2^-23 sum_e alpha_e |feat_e| + 2^-23 sum_e |feat_e| / l + 2^-126; out[:, h], m[:, h], l[:, h] have the bits
 * of the heads == 1 call on the contiguous slices.  One launch, a row per lane group (a hub row serialises its wave, twice), no
 * workspace, no float atomics, no host synchronisation.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: heads < 1, negative sizes, nnz > INT_MAX, heads * head_dim > INT_MAX, nnz > 0
 * with num_rows == 0, head_dim not a multiple of 16 bytes of feat (8 for 16-bit, 4 for fp32), an unknown dtype, a non-finite scale, a
 * null or misaligned pointer; VOLTRIX_OK without a launch for num_rows == 0 or head_dim == 0; with nnz == 0 out and l are zero-filled
 * (m: -inf) and indices, scores, feat are not read.
 * Alignment: indptr, indices, scores, m, l 4 bytes; feat and out 16 bytes (16 bytes per lane). */
void voltrix_launch_attn_aggregate_csr(void* indptr, void* indices, void* scores, int num_rows, int64_t nnz, int heads, int head_dim,
                                       void* feat, int dtype, float scale, void* out, void* m, void* l, void* stream, int* return_code);

/* Its gradient for the scores: grad_scores[e, h] = scale * alpha[e, h] * (<grad_out[row_e, h], feat[indices[e], h]> - delta[row_e, h]),
 * alpha recomputed from scores, m and l of the forward; delta[r, h] = <grad_out[r, h], out[r, h]> is the caller's dense product (device
 * float[num_rows, heads]).  grad_out = device float[num_rows, heads, head_dim]; feat, dtype as above; grad_scores = device
 * float[nnz, heads], every element written; a row or head with l == 0 gives 0.  One launch split by edges (a hub row costs what its
 * edges cost), fp32 fused multiply-adds in column order and a fixed butterfly, grad_scores[:, h] has the bits of the heads == 1 call.  The
 * checks above; VOLTRIX_OK without a launch for nnz == 0 or head_dim == 0.
 * Alignment: indptr, indices, scores, m, l, delta, grad_scores 4 bytes; grad_out and feat 16 bytes. */
void voltrix_launch_attn_aggregate_grad_scores_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads, int head_dim,
                                                   void* grad_out, void* feat, int dtype, void* scores, void* m, void* l, void* delta,
                                                   float scale, void* grad_scores, void* stream, int* return_code);

/* Its gradient for feat, on the TRANSPOSED CSR (voltrix_launch_csr_transpose; num_cols rows):
 * grad_feat[c, h, :] = sum_{e in row c} alpha[order[e], h] * grad_out[t_indices[e], h, :], order = device int32[nnz], the entry of the CSR
 * that entry e of the transpose is; scores stays in CSR order and grad_out is never permuted; m, l = the forward's, indexed by
 * t_indices.  grad_out = device [*, heads, head_dim] of dtype 0 fp32 / 1 fp16 / 2 bfloat16 (head_dim a multiple of 16 bytes of it);
 * grad_feat = device float[num_cols, heads, head_dim], every row written, rows without entries zero.  One fused multiply-add per element
 * in the transposed CSR's edge order; a row per lane group (a hub column serialises its wave).  The checks above; VOLTRIX_OK without a
 * launch for num_cols == 0 or head_dim == 0; with nnz == 0 grad_feat is zero-filled and nothing but t_indptr is read.
 * Alignment: t_indptr, t_indices, order, scores, m, l 4 bytes; grad_out and grad_feat 16 bytes. */
void voltrix_launch_attn_aggregate_grad_feat_csr(void* t_indptr, void* t_indices, void* order, int num_cols, int64_t nnz, int heads,
                                                 int head_dim, void* grad_out, int dtype, void* scores, void* m, void* l, float scale,
                                                 void* grad_feat, void* stream, int* return_code);

/* Attention dropout (dropout_mask_kernels.hpp; attn_aggregate_kernels.hpp with a mask).
 * The keep mask is device int32[nnz, W], W = ceil(heads / 32), in CSR edge order: bit (h & 31) of word (h >> 5) of edge e set means
 * (e, h) is kept; bits past heads are zero and never read.  voltrix_launch_dropout_mask writes every word: (e, h) is kept iff
 * x >= threshold with x = word (h & 3) of Philox4x32-10(counter = (e, h >> 2, offset & 0xffffffff, offset >> 32), key = (seed &
 * 0xffffffff, seed >> 32)), multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds.  threshold =
 * min(2^32 - 1, floor(p * 2^32)) for a drop probability p: the kept probability is 1 - threshold / 2^32 and threshold 0 keeps all.  A
 * bit depends on (seed, offset, e, h) only -- not on nnz, heads or the launch.  One thread per word (at most 2^24 - 1 workgroups: past
 * 2^32 - 256 words a thread writes more than one), one 4-byte store each, no LDS, no workspace, no atomics, no host synchronisation.
 * Every nnz <= INT_MAX works with every heads (nnz = 2^31 - 1 with 33 heads is tested on the device).
 * VOLTRIX_ERR_BAD_SHAPE on the host before any HIP call: heads < 1, nnz < 0, nnz > INT_MAX, mask null or not 4-byte aligned with
 * nnz > 0; VOLTRIX_OK without a launch for nnz == 0. */
void voltrix_launch_dropout_mask(int64_t nnz, int heads, uint32_t threshold, uint64_t seed, uint64_t offset, void* mask, void* stream,
                                 int* return_code);

/* voltrix_launch_attn_aggregate_csr and its two gradients with a keep mask: k[e, h] = keep_scale where the bit is set, 0 elsewhere.
 *   out[r, h, :]        = sum_{e in row r} alpha[e, h] * k[e, h] * feat[indices[e], h, :]
 *   grad_scores[e, h]   = scale * alpha[e, h] * (k[e, h] * <grad_out[row_e, h], feat[indices[e], h]> - delta[row_e, h])
 *   grad_feat[c, h, :]  = sum_{e in row c of the transpose} alpha[order[e], h] * k[order[e], h] * grad_out[t_indices[e], h, :]
 * alpha, m and l are those of the call without a mask (same bits): dropout acts after the normalisation, and delta is the dense product
 * with the dropped out.  A dropped entry is a predicate, not a product with 0: its 16-byte pieces of feat (grad_out for grad_feat) are
 * not loaded, so a NaN or inf there reaches nothing, and its dot in grad_scores is +0.  A row or head without a kept entry gives zeros.
 * With every bit set and keep_scale = 1 all five results have the bits of the calls without a mask.  |out - ref| <= (2 (deg + 3) + 1)
 * 2^-23 sum_e alpha_e k_e |feat_e| + 2^-23 sum_e k_e |feat_e| / l + 2^-126 with deg the row's full degree.  Lane maps, grids and the
 * order of the sums are those of the calls without a mask; one more broadcast 4-byte load per entry; no LDS, no workspace, no atomics.
 * The arguments, checks and alignments of the calls without a mask, and: keep_scale non-finite or negative is VOLTRIX_ERR_BAD_SHAPE
 * (checked with scale, before "nothing to do"); mask null or not 4-byte aligned is VOLTRIX_ERR_BAD_SHAPE when nnz > 0 and the call has
 * something to do.  mask = device int32[nnz, ceil(heads / 32)] in CSR order for all three (grad_feat reads it at order[e]). */
void voltrix_launch_attn_aggregate_dropout_csr(void* indptr, void* indices, void* scores, int num_rows, int64_t nnz, int heads,
                                               int head_dim, void* feat, int dtype, float scale, void* out, void* m, void* l, void* mask,
                                               float keep_scale, void* stream, int* return_code);
void voltrix_launch_attn_aggregate_dropout_grad_scores_csr(void* indptr, void* indices, int num_rows, int64_t nnz, int heads,
                                                           int head_dim, void* grad_out, void* feat, int dtype, void* scores, void* m,
                                                           void* l, void* delta, float scale, void* grad_scores, void* mask,
                                                           float keep_scale, void* stream, int* return_code);
void voltrix_launch_attn_aggregate_dropout_grad_feat_csr(void* t_indptr, void* t_indices, void* order, int num_cols, int64_t nnz,
                                                         int heads, int head_dim, void* grad_out, int dtype, void* scores, void* m,
                                                         void* l, float scale, void* grad_feat, void* mask, float keep_scale,
                                                         void* stream, int* return_code);

/* Max / min / mean neighbour aggregation on a DEVICE CSR (spmm_csr_reduce_kernels.hpp): op 0 max, 1 min, 2 mean.
 *   output[r, f] = max | min | mean over the entries e of row r of input[indices[e], f]
 *   arg[r, f]    = the CSR ENTRY id e of the winner (max / min; not its column: with duplicate (row, col) entries a column id would match
 *                  twice in the backward)
 * input = device [*, embedding_dim] of dtype 0 fp32 / 1 fp16 / 2 bfloat16, read as it is; output = device float[num_rows, embedding_dim];
 * arg = device int32[num_rows, embedding_dim] or NULL (then it is neither computed nor stored; it must be NULL for mean).  Every element
 * of output and arg is written.  Selection: entry e with value v replaces the winner when v > best (min: v < best) or v is the row's
 * first NaN -- strict, so the first entry in CSR order wins ties, +0 and -0 tie, a NaN among a row's entries gives NaN with arg at the
 * first NaN (torch.amax), a row whose entries are all -inf gives -inf with arg at its first entry.  A selection does not round: output
 * is the winning element converted to fp32, whatever the dtype.  A row without entries gives 0 and arg = -1.  mean: fp32 additions in
 * CSR order and one fp32 division by the row's entry count, |output - ref| <= (deg + 1) 2^-23 sum_e |input_e| / deg; duplicate entries
 * count twice; a row without entries gives 0.  One launch, a row per lane group (a hub row serialises its wave, as in
 * voltrix_launch_spmm_csr_heads), 16 bytes of every gathered row per lane, no workspace, no float atomics, no host synchronisation,
 * the same bits on every call; element offsets are 64-bit (num_rows * embedding_dim may pass 2^31).
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, an unknown dtype or op, a non-NULL arg with mean,
 * embedding_dim not a multiple of 16 bytes of input (8 for 16-bit, 4 for fp32), a null or misaligned pointer; VOLTRIX_OK without a
 * launch for num_rows == 0 or embedding_dim == 0.  On a pattern without entries every row is filled (0, arg = -1) and indices and input
 * are not read (they must still be valid pointers: the entry count is the device's indptr[num_rows]).  Nothing is checked on the device.
 * Alignment: indptr, indices 4 bytes; input, output, arg 16 bytes (16 bytes per lane).  No reference counterpart. */
void voltrix_launch_spmm_csr_reduce(void* indptr, void* indices, int num_rows, int embedding_dim, void* input, int dtype, int op,
                                    void* output, void* arg, void* stream, int* return_code);

/* The backward of max / min, on the TRANSPOSED CSR (voltrix_launch_csr_transpose; num_cols rows):
 *   output[c, f] = sum over the entries e of row c of the transpose with arg[t_indices[e], f] == t_order[e] of grad_out[t_indices[e], f]
 * num_entries = the pattern's entry count nnz; t_order = device int32[nnz], the entry of the CSR that entry e of the transpose is; grad_out
 * = device float[*, embedding_dim]; arg =
 * the forward's device int32[*, embedding_dim] (only compared, never used as an index); output = device float[num_cols, embedding_dim],
 * every row written, columns without entries zero.  A gather: the gradient of an element goes to its one winner, fp32 additions in the
 * transposed CSR's order (|output - ref| <= k 2^-23 sum |terms| for k terms), no float atomics, the same bits on every call; a row of
 * grad_out is loaded only where one of a lane's four components matched.  One launch, a column per lane group and 4 features per lane (a
 * hub column serialises its wave), no workspace, no host synchronisation, 64-bit element offsets.  The backward of mean needs no entry
 * point: voltrix_launch_spmm_csr_rows on the transposed CSR applied to grad_out / deg.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, nnz > INT_MAX, embedding_dim not a multiple of 4, a null or
 * misaligned pointer; VOLTRIX_OK without a launch for num_cols == 0 or embedding_dim == 0; with nnz == 0 output is zero-filled and
 * nothing but t_indptr is read.  Alignment: t_indptr, t_indices, t_order 4 bytes; grad_out, arg, output 16 bytes. */
void voltrix_launch_spmm_csr_reduce_backward(void* t_indptr, void* t_indices, void* t_order, int num_cols, int64_t num_entries, int embedding_dim,
                                             void* grad_out, void* arg, void* output, void* stream, int* return_code);

/* Aggregation with a feature VECTOR per edge on a DEVICE CSR (spmm_edge_kernels.hpp): op 0 mul, 1 add, 2 add_relu, 3 copy, 4 gate.
 *   output[r, f] = sum over the entries e of row r of m(input[indices[e], f], efeat[id_e, f]),  id_e = order ? order[e] : e
 *   m(x, w) = x * w (mul) | x + w (add) | max(x + w, 0) (add_relu) | w (copy: input is not read) |
 *             (self[r, f] + w) > 0 ? x : 0 (gate: the gradient of add_relu for the gathered operand, run on the transposed CSR with
 *             input = grad_out, self = the forward's gathered operand, order = t_order)
 * num_entries = the pattern's entry count nnz; order = device int32[nnz] or NULL; input = device [*, embedding_dim] of input_dtype;
 * efeat = device [nnz, embedding_dim] of efeat_dtype; self = device [num_rows, embedding_dim] of efeat_dtype (gate only, else NULL);
 * output = device float[num_rows, embedding_dim], every element written, a row without entries 0.  dtypes: 0 fp32 / 1 fp16 / 2
 * bfloat16, read as they are; the pairs (input_dtype, efeat_dtype) are (T, T) and (fp32, fp16 | bf16); gate takes input_dtype fp32
 * only; copy ignores input_dtype.  fp32 additions in CSR order: |output - ref| <= (k + 1) 2^-23 sum |terms| for the k terms of an
 * element.  max(x + w, 0) is a compare and a select: a NaN or inf propagates as the arithmetic does (max(NaN + w, 0) is NaN).  The gate
 * is one fp32 addition of the exactly converted operands, so its sign is that of the exact sum; it is closed at 0 and a closed gate
 * passes nothing.  One launch, a row per lane group (a hub row serialises its wave, as in voltrix_launch_spmm_csr_heads), 16 bytes of
 * efeat per lane and entry, no LDS, no workspace, no float atomics, no host synchronisation, the same bits on every call; element
 * offsets are 64-bit (nnz * embedding_dim may pass 2^31).
 * RETURNS the status code (no return_code slot).  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative
 * sizes, num_entries > INT_MAX, an unknown op or dtype, a pair that is not instantiated, embedding_dim not a multiple of 16 bytes of
 * efeat (8 for 16-bit, 4 for fp32), a null indptr / indices / efeat / output, a null input unless op is copy, a null self with gate, a
 * misaligned pointer; VOLTRIX_OK without a launch for num_rows == 0 or embedding_dim == 0.  On a pattern without entries output is
 * zero-filled and indices, input, efeat and order are not read (they must still be valid pointers).  Nothing is checked on the device.
 * Alignment: indptr, indices, order 4 bytes; input, efeat, self, output 16 bytes.  No reference counterpart. */
int voltrix_spmm_edge_csr(void* indptr, void* indices, void* order, int num_rows, int64_t num_entries, int embedding_dim,
                          void* input, int input_dtype, void* efeat, int efeat_dtype, void* self, int op,
                          void* output, void* stream);

/* The gradient of voltrix_spmm_edge_csr for efeat, row-parallel on the same CSR: op 0 mul, 1 add, 2 add_relu, 3 copy.
 *   output[e, f] = grad_out[row_e, f] * feat[indices[e], f] (mul) | grad_out[row_e, f] (add, copy) |
 *                  (feat[indices[e], f] + efeat[e, f]) > 0 ? grad_out[row_e, f] : 0 (add_relu)
 * grad_out = device float[num_rows, embedding_dim]; feat = device [*, embedding_dim] and efeat = device [nnz, embedding_dim], both of
 * dtype (0 fp32 / 1 fp16 / 2 bfloat16); output = device float[nnz, embedding_dim], every element written.  feat is read by mul and
 * add_relu, efeat by add_relu alone; what an op does not read may be NULL.  mul rounds once (|output - ref| <= 2^-23 |ref|), the others
 * are exact.  One launch, a row per lane group (a hub row serialises its wave), 16-byte stores, no atomics, the same bits on every call,
 * 64-bit element offsets.
 * RETURNS the status code.  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_entries > INT_MAX, an unknown
 * op (gate included) or dtype, embedding_dim not a multiple of 16 bytes of dtype, a null indptr / grad_out / output, a null operand the
 * op reads (indices and feat: mul, add_relu; efeat: add_relu), a misaligned pointer; VOLTRIX_OK without a launch for num_rows == 0,
 * embedding_dim == 0 or num_entries == 0.  Nothing is checked on the device.  Alignment: indptr, indices 4 bytes; the others 16. */
int voltrix_spmm_edge_grad_efeat_csr(void* indptr, void* indices, int num_rows, int64_t num_entries, int embedding_dim,
                                     void* grad_out, void* feat, void* efeat, int dtype, int op, void* output, void* stream);

/* Relational (R-GCN) aggregation over TYPED edges on a DEVICE CSR, with basis decomposition (spmm_rel_kernels.hpp):
 *   output[i, b, f] = sum over the entries e of row i of c(e, b) * input[indices[e], f],   c(e, b) = w_e * coef[etype[e], b]
 * num_entries = the pattern's entry count nnz; etype = device int32[nnz] in CSR entry order, 0 <= etype < num_types; weight = device
 * float[nnz] or NULL (w_e = 1: c(e, b) is coef itself); input = device [*, embedding_dim] of dtype (0 fp32 / 1 fp16 / 2 bfloat16, read
 * as stored); coef = device float[num_types, B_pad] with B_pad = num_bases rounded up to a multiple of 4 (rows of whole 16-byte pieces;
 * the padding is read and ignored); output = device float[num_rows, num_bases, embedding_dim], every element written, a row without
 * entries 0.  LIMITS: 1 <= num_types <= 65 536, 0 <= num_bases <= 1 024.  fp32 throughout, sums in CSR order per row: |output - ref|
 * <= (k + 2) 2^-23 sum |terms| for the k entries of a row (c(e, b) rounds once, a term once more).  NaN and inf propagate as the
 * arithmetic does.  One launch: a row per lane group (a hub row serialises its wave, as in voltrix_launch_spmm_csr_heads), 16 bytes of
 * the gathered row per lane and entry, tiles of 8 bases (4 where num_bases <= 4) in registers and over grid.z beyond -- the gathered
 * row is read again per tile --, coef by plain loads, no LDS, no workspace, no float atomics, no host synchronisation, the same bits on
 * every call; element offsets are 64-bit (num_rows * num_bases * embedding_dim may pass 2^31).
 * RETURNS the status code (no return_code slot).  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative
 * sizes, num_entries > INT_MAX, num_types or num_bases outside the limits, an unknown dtype, embedding_dim not a multiple of 16 bytes
 * of dtype (8 for 16-bit, 4 for fp32); then VOLTRIX_OK without a launch for num_rows == 0, embedding_dim == 0 or num_bases == 0; then
 * VOLTRIX_ERR_BAD_SHAPE for a null indptr / indices / etype / input / coef / output or a misaligned pointer.  On a pattern without
 * entries output is zero-filled and indices, etype, weight, input and coef are not read (they must still be valid pointers).  Nothing
 * is checked on the device.  Alignment: indptr, indices, etype, weight 4 bytes; input, coef, output 16 bytes.  No reference counterpart. */
int voltrix_spmm_rel_csr(void* indptr, void* indices, void* etype, void* weight, int num_rows, int64_t num_entries, int embedding_dim,
                         int num_types, int num_bases, void* input, int dtype, void* coef, void* output, void* stream);

/* The gradient of voltrix_spmm_rel_csr for its gathered operand, on the TRANSPOSED CSR (t_indptr has num_cols + 1 elements):
 *   output[c, f] = sum over the entries e of row c of the transpose, over b, of c(id_e, b) * grad_out[t_indices[e], b, f]
 *   id_e = order ? order[e] : e,   c(id, b) = w_id * coef[etype[id], b]
 * order = device int32[nnz] or NULL: the entry of the CSR that entry e of the transpose is (t_order); etype, weight (or NULL) and coef
 * as in voltrix_spmm_rel_csr, indexed by CSR entry; grad_out = device float[*, num_bases, embedding_dim]; output = device
 * float[num_cols, embedding_dim], every element written, a column without entries 0.  A gather: fp32 additions in a fixed order (the
 * transposed CSR's entries in batches of 4; inside a batch tiles of 4 bases, inside a tile entry by entry and basis by basis):
 * |output - ref| <= (k num_bases + 2) 2^-23 sum |terms| for the k entries of a column.  One launch, a column per lane group and 4
 * features per lane, no workspace, no float atomics, the same bits on every call, 64-bit element offsets.
 * RETURNS the status code.  VOLTRIX_ERR_BAD_SHAPE as for voltrix_spmm_rel_csr with embedding_dim a multiple of 4 and grad_out in the
 * place of input; VOLTRIX_OK without a launch for num_cols == 0, embedding_dim == 0 or num_bases == 0 (the caller zero-fills where
 * num_bases == 0).  Alignment: t_indptr, t_indices, order, etype, weight 4 bytes; grad_out, coef, output 16 bytes. */
int voltrix_spmm_rel_contract_csr(void* t_indptr, void* t_indices, void* order, void* etype, void* weight, int num_cols,
                                  int64_t num_entries, int embedding_dim, int num_types, int num_bases, void* grad_out, void* coef,
                                  void* output, void* stream);

/* The dots behind the gradient of voltrix_spmm_rel_csr for coef, row-parallel on the same CSR:
 *   output[e, b] = w_e * <grad_out[row_e, b, :], feat[indices[e], :]>     (b < num_bases;  0 for num_bases <= b < B_pad)
 * grad_out = device float[num_rows, num_bases, embedding_dim]; feat = device [*, embedding_dim] of dtype; weight = device float[nnz] or
 * NULL; output = device float[num_entries, B_pad], every element written.  The gradient is the sum of output's rows per type:
 * voltrix_launch_spmm_csr_rows on a table of the entries sorted by type (in chunks, then per type; voltrix/spmm_rel.py).  A dot of F
 * terms in fp32: |output - ref| <= (F + 1) 2^-23 |w_e| sum_f |g x|.  One launch, a row per lane group, embedding_dim beyond one slab
 * of 64 pieces walked inside the kernel, a butterfly of shuffles per dot, 16-byte stores, no atomics, the same bits on every call,
 * 64-bit element offsets.
 * RETURNS the status code.  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_entries > INT_MAX, num_bases
 * > 1 024, an unknown dtype, embedding_dim not a multiple of 16 bytes of dtype; then VOLTRIX_OK without a launch for num_rows == 0,
 * embedding_dim == 0, num_bases == 0 or num_entries == 0 (the caller zero-fills where embedding_dim == 0); then VOLTRIX_ERR_BAD_SHAPE
 * for a null indptr / indices / grad_out / feat / output or a misaligned pointer.  Alignment: indptr, indices, weight 4 bytes; grad_out,
 * feat, output 16 bytes. */
int voltrix_spmm_rel_dots_csr(void* indptr, void* indices, void* weight, int num_rows, int64_t num_entries, int embedding_dim,
                              int num_bases, void* grad_out, void* feat, int dtype, void* output, void* stream);

/* FP8 feature rows (OCP e4m3fn = torch.float8_e4m3fn: bias 7, subnormals m 2^-9, largest finite 448, 0x7f / 0xff NaN, no infinities;
 * NOT the MI300 e4m3fnuz encoding), spmm_fp8_kernels.hpp.  The quantiser, row-major, one launch that reads input once:
 *   output[i, f] = rne_e4m3(clamp(fp32(input[i, f]) * inv_scale[f], -448, 448))   for f < embedding_dim;  0x00 for the padding up to F16
 * F16 = embedding_dim rounded up to 16.  input = device [num_rows, embedding_dim] of dtype (0 fp32 / 1 fp16 / 2 bfloat16, read as
 * stored) whose rows are input_ld ELEMENTS apart (input_ld >= embedding_dim: a column slice of a wider matrix goes in as it is; rows on
 * 16-byte boundaries are read 16 bytes at a time, others element by element); inv_scale = device float[F16]; output = device
 * uint8[num_rows, F16] whose rows are output_ld BYTES apart (>= F16, a multiple of 16).  One fp32 multiply, then the clamp, then one
 * rounding to nearest even with e4m3 subnormals: torch's (x.float() * inv_scale).clamp(-448, 448).to(torch.float8_e4m3fn) bit for
 * bit.  +-inf saturates to +-448, a NaN gives an e4m3 NaN code, -0 keeps its sign.  A grid-stride loop over the rows, 64-bit offsets,
 * no LDS, no atomics, no host synchronisation.
 * RETURNS the status code (no return_code slot).  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative
 * sizes, an unknown dtype, input_ld < embedding_dim, output_ld < F16 or not a multiple of 16; then VOLTRIX_OK without a launch for
 * num_rows == 0 or embedding_dim == 0; then VOLTRIX_ERR_BAD_SHAPE for a null or misaligned pointer.  Alignment: input, inv_scale,
 * output 16 bytes.  No reference counterpart. */
int voltrix_quantize_fp8_rows(void* input, int dtype, int num_rows, int embedding_dim, int64_t input_ld, void* inv_scale, void* output,
                              int64_t output_ld, void* stream);

/* Aggregation of FP8 feature rows on a DEVICE CSR:
 *   output[i, f] = scale[f] * sum over the entries e of row i of v_e * dec(input[indices[e], f])        v_e = values ? values[e] : 1
 * input = device uint8[*, embedding_dim16] of e4m3fn codes (embedding_dim16 a multiple of 16; padding columns hold 0x00); scale =
 * device float[embedding_dim16], the dequantisation multiplier per COLUMN (a per-row scale would be a second gathered line per entry);
 * values = device float[nnz] in CSR order or NULL; output = device [num_rows, embedding_dim16] of out_dtype (0 fp32 / 1 fp16 / 2
 * bfloat16; a 16-bit output is the fp32 result rounded to nearest even), every element written, a row without entries 0; num_entries =
 * the pattern's entry count nnz; xcd_ranges as in voltrix_launch_spmm_csr_rows.  Decoded values are exact in fp32; the sum is fp32 in
 * CSR entry order (with values: one fused multiply-add per element) and starts from -0, so a lone -0 keeps its sign; then one multiply
 * by scale[f]: |output - ref| <= (k + 2) 2^-23 |scale[f]| sum_e |v_e dec_e| for the k entries of a row; integer-valued codes and
 * values with power-of-two scales give equality.  NaN propagates as the arithmetic does.  One launch, a row per lane group (a hub row
 * serialises its wave), 16 bytes = 16 features of the gathered row per lane and entry, no LDS, no workspace, no atomics, no host
 * synchronisation, the same bits on every call; element offsets are 64-bit (rows * embedding_dim16 may pass 2^31).
 * RETURNS the status code.  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_entries > INT_MAX,
 * embedding_dim16 not a multiple of 16, an unknown out_dtype; then VOLTRIX_OK without a launch for num_rows == 0 or embedding_dim16
 * == 0; then VOLTRIX_ERR_BAD_SHAPE for a null indptr / indices / input / scale / output or a misaligned pointer.  On a pattern without
 * entries indices, values and input are not read (they must still be valid pointers).  Nothing is checked on the device.  Alignment:
 * indptr, indices, values 4 bytes; input, scale, output 16 bytes.  No reference counterpart. */
int voltrix_spmm_fp8_csr(void* indptr, void* indices, void* values, int num_rows, int embedding_dim16, void* input, void* scale,
                         void* output, int out_dtype, int xcd_ranges, int64_t num_entries, void* stream);

/* Several aggregates of every row's neighbours from ONE gather of a DEVICE CSR (spmm_multi_kernels.hpp): per row r with d entries
 * (duplicates count twice) and per element f, over x_e = input[indices[e], f] in CSR order:
 *   sum   fp32 additions from 0 (the bits of voltrix_launch_spmm_csr_rows)       mean  sum / d (the bits of voltrix_launch_spmm_csr_reduce)
 *   max, min   strict selection: the first entry wins ties, the first NaN wins and stays (the bits of voltrix_launch_spmm_csr_reduce);
 *              argmax / argmin = the CSR ENTRY id of the winner
 *   var   max(S2 / d - (S1 / d)^2, 0) from moments SHIFTED by the row's first entry: y_e = x_e - x_first, S1 = sum y_e, S2 = sum y_e^2;
 *         |var - ref| <= (d + 4) 2^-23 (2 / d) sum_e (x_e - x_first)^2; one entry gives 0 exactly; a NaN or +-inf entry gives NaN
 *   std   sqrt(var + eps)
 * output = device float[num_rows, num_slots, embedding_dim]; slot_sum .. slot_std = the slot of each aggregate in a row of output, -1
 * for one that is not stored; the stored ones fill the slots 0 .. num_slots - 1, each exactly once.  argmax / argmin = device
 * int32[num_rows, embedding_dim] or NULL; one that is given needs its max / min stored.  input = device [*, embedding_dim] of dtype
 * (0 fp32 / 1 fp16 / 2 bfloat16), read as it is; num_entries = the pattern's entry count nnz.  Every element of output and of the
 * args is written; a row without entries gives 0 in every aggregate (std too) and -1 in the args.  An aggregate's bits do not depend
 * on which others are stored.  One launch, a row per lane group (a hub row serialises its wave, as in voltrix_launch_spmm_csr_heads),
 * 16 bytes of the gathered row per lane and entry, no LDS, no workspace, no atomics, no host synchronisation, the same bits on every
 * call; element offsets are 64-bit (num_rows * num_slots * embedding_dim may pass 2^31).
 * RETURNS the status code.  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_entries > INT_MAX, an unknown
 * dtype, num_slots outside 1 .. 6, a slot outside -1 .. num_slots - 1, two aggregates in one slot, a slot nobody fills, argmax / argmin
 * without max / min, eps not finite or <= 0 when std is stored, embedding_dim not a multiple of 16 bytes (8 for 16-bit, 4 for fp32);
 * then VOLTRIX_OK without a launch for num_rows == 0 or embedding_dim == 0; then VOLTRIX_ERR_BAD_SHAPE for a null indptr / indices /
 * input / output or a misaligned pointer.  On a pattern without entries indices and input are not read (they must still be valid
 * pointers).  Nothing is checked on the device.  Alignment: indptr, indices 4 bytes; input, output, argmax, argmin 16 bytes.  No
 * reference counterpart. */
int voltrix_spmm_multi_csr(void* indptr, void* indices, int num_rows, int64_t num_entries, int embedding_dim, void* input, int dtype,
                           int slot_sum, int slot_mean, int slot_max, int slot_min, int slot_var, int slot_std, int num_slots,
                           float eps, void* output, void* argmax, void* argmin, void* stream);

/* The joint backward of voltrix_spmm_multi_csr for its input, a gather on the TRANSPOSED CSR (t_indptr / t_indices; t_order[e] = the
 * entry of the CSR that entry e of the transpose is):
 *   output[c, f] = sum over the entries e of column c, r = t_indices[e], id = t_order[e], of
 *                  u[r, f] + w[r, f] (x[c, f] - mean[r, f]) + [argmax[r, f] == id] g_max[r, f] + [argmin[r, f] == id] g_min[r, f]
 * in the transposed CSR's order, the terms of an entry in this order, the centred term one fused multiply-add.  The caller forms
 * u = g_sum + g_mean / d and w = 2 g_var / d + g_std / (d std).  All operands are device float (the args int32) [*, embedding_dim];
 * x = the forward's input as fp32 [num_cols, embedding_dim], read once per column; mean has rows of mean_ld floats (a slot of the
 * forward's output).  u may be NULL; w, x and mean are NULL together; g_max with argmax and g_min with argmin are NULL in pairs; at
 * least one group is given.  A g_max / g_min row is loaded only where a component matched.  output = device float[num_cols,
 * embedding_dim], every row written, columns without entries zeros.  One launch, a column per lane group (a hub column serialises its
 * wave), 4 features per lane, no atomics, the same bits on every call; element offsets are 64-bit.
 * RETURNS the status code.  VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_entries > INT_MAX,
 * embedding_dim not a multiple of 4, a group given in part or none at all, mean_ld < embedding_dim or not a multiple of 4 (with w);
 * then VOLTRIX_OK without a launch for num_cols == 0 or embedding_dim == 0; then VOLTRIX_ERR_BAD_SHAPE for a null t_indptr / output,
 * a misaligned pointer, or with num_entries > 0 a null t_indices, or a null t_order beside g_max / g_min.  Nothing is checked on the
 * device; the args are only compared, never used as an index.  Alignment: t_indptr, t_indices, t_order 4 bytes; the rest 16 bytes.
 * No reference counterpart. */
int voltrix_spmm_multi_backward_csr(void* t_indptr, void* t_indices, void* t_order, int num_cols, int64_t num_entries, int embedding_dim,
                                    void* x, void* u, void* w, void* mean, int64_t mean_ld, void* g_max, void* argmax, void* g_min,
                                    void* argmin, void* output, void* stream);

/* Neighbour sampling on a device int32 CSR and the relabelling of a sampled block (voltrix/neighbor_sample_kernels.hpp): what produces
 * the rectangular [num_dst, num_src] patterns the CSR operators above take (GraphSAGE-style mini-batches).  No reference counterpart.
 * THE SAMPLING RULE.  For a seed row r (its global row id), fan-out k = fanout, degree d = indptr[r + 1] - indptr[r]:
 *   draw(r, i) = word i & 3 of Philox4x32-10(counter = (r, (i >> 2) | 0x80000000, offset & 0xffffffff, offset >> 32),
 *                key = (seed & 0xffffffff, seed >> 32)); bit 31 of counter word 1 separates these draws from
 *                voltrix_launch_dropout_mask's (edge, h >> 2, ...) counters: one seed for both gives unrelated streams.
 *   replace = 0, d <= k: every entry of the row, in CSR order, no draw used.  fanout = -1 (VOLTRIX_SAMPLE_ALL) means this for every
 *                row, whatever replace is.
 *   replace = 0, d > k:  Floyd's algorithm on entry positions: for i = 0 .. k - 1, j = d - k + i, t = (uint64(draw(r, i)) * (j + 1)) >> 32;
 *                take t unless it is taken already, then take j.  The k positions are output in ascending order (a sampled row keeps CSR
 *                order).  A function of (seed, offset, r, d, k) only: not of the other seeds, their order or the launch geometry.  The
 *                multiply-shift has a relative bias of at most d / 2^32 per position.
 *   replace = 1, d > 0:  exactly k entries, entry i at position (uint64(draw(r, i)) * d) >> 32, in draw order; d == 0: none.
 * seeds = device int32[num_seeds] global row ids; a seed outside [0, num_rows) has degree 0 inside the kernel (never an out-of-bounds
 * read; callers reject it earlier).  s_indptr = device int32[num_seeds + 1], the caller's prefix sum of the per-seed counts the rule
 * gives (min(d, k); d > 0 ? k : 0 with replace; d for fanout = -1); num_sampled = s_indptr[num_seeds].  Outputs, every element written
 * when s_indptr is the rule's, neither needs initialising: s_indices = device int32[num_sampled], the global column ids; s_entries =
 * device int32[num_sampled], the CSR entry id of every sampled entry (edge features, edge values, arg-style bookkeeping).  A row never
 * writes past its own segment of s_indptr.  One lane per seed, 256 per workgroup, O(k^2) compares and k gathers per row whatever its
 * degree (fanout = -1 copies a row with one lane: O(d)); the sorted positions live in 256 k 4 bytes of dynamic LDS (k <= 64); no
 * atomics, no workspace, no host synchronisation, the same bits on every call.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_sampled > INT_MAX, fanout outside 1 .. 64 and not -1,
 * replace outside {0, 1}, a null or misaligned pointer (indices, s_indices, s_entries only where num_sampled > 0); VOLTRIX_OK without a
 * launch for num_seeds == 0 or num_sampled == 0.  Alignment: 4 bytes everywhere. */
#define VOLTRIX_SAMPLE_ALL (-1)
void voltrix_launch_sample_neighbors(void* indptr, void* indices, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                     int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* s_indices,
                                     void* s_entries, void* stream, int* return_code);

/* Relabelling a sampled block: global column ids -> positions in src_ids, the seeds first.  table = device int32[num_cols], ZERO ON
 * ENTRY (the one buffer here that must be initialised); three launches on one stream:
 *   voltrix_launch_block_mark:        table[cols[e]] = 1 for e < num_sampled (plain stores of one value);
 *   voltrix_launch_block_mark_seeds:  table[seeds[i]] = -(i + 1) -- the seeds win over the marks.  Duplicate seeds are the caller's to
 *                                     exclude (one of the stores wins: which is not defined);
 *   (the caller takes rank = the inclusive count of table > 0 over the columns, device int32[num_cols], and num_src = num_seeds +
 *   rank[num_cols - 1])
 *   voltrix_launch_block_relabel:     local[e] = t < 0 ? -t - 1 : num_seeds + rank[c] - 1 with c = cols[e], t = table[c]; src_ids[num_seeds +
 *                                     rank[c] - 1] = c for marked c; src_ids[i] = seeds[i].
 * So src_ids[0 .. num_seeds) is the seeds in the given order and the rest the other sampled columns in ascending id: deterministic, and
 * a gather feat[src_ids] reads ascending addresses.  Every element of local (device int32[num_sampled]) and src_ids (device
 * int32[num_src]) is written; neither needs initialising.  A column or seed outside [0, num_cols) is skipped by the mark launches and
 * gives local = -1: never an out-of-bounds access.  No atomics, no host synchronisation inside.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: negative sizes, num_sampled > INT_MAX, num_src < num_seeds, a null or
 * misaligned pointer among those the sizes make the launch touch; VOLTRIX_OK without a launch where there is nothing to do
 * (num_sampled == 0 or num_cols == 0 for block_mark, num_seeds == 0 or num_cols == 0 for block_mark_seeds, both counts 0 for
 * block_relabel).  Alignment: 4 bytes everywhere. */
void voltrix_launch_block_mark(void* cols, int64_t num_sampled, int num_cols, void* table, void* stream, int* return_code);
void voltrix_launch_block_mark_seeds(void* seeds, int num_seeds, int num_cols, void* table, void* stream, int* return_code);
void voltrix_launch_block_relabel(void* cols, int64_t num_sampled, void* seeds, int num_seeds, void* table, void* rank, int num_cols,
                                  int num_src, void* local, void* src_ids, void* stream, int* return_code);

/* Induced subgraphs and random walks on a device int32 CSR (voltrix/induced_subgraph_kernels.hpp): what subgraph mini-batch training
 * needs (Cluster-GCN, GraphSAINT-RW).  No reference counterpart.
 * THE SUBGRAPH CONTRACT.  rows = device int32[num_sub_rows] global row ids, any order, duplicates allowed (a duplicate row is emitted
 * twice); cols = device int32[C] global column ids in [0, num_cols), no duplicates, known to these calls only through table = device
 * int32[num_cols] with table[cols[j]] = -(j + 1) and 0 elsewhere (ZERO it, then voltrix_launch_block_mark_seeds(cols, C, num_cols,
 * table)).  Row i of the result is row rows[i] of the CSR with exactly those entries whose column is in cols, IN CSR ORDER: a stable
 * compaction, so a sorted row stays sorted only if cols is ascending; a column that appears twice in a row is kept twice.  s_local[e]
 * is the position in cols of the entry's column (the local id of cols[j] is j: feat[cols] is the subgraph's feature matrix);
 * s_entries[e] is the entry's index in indices (edge values, edge features, arg-style bookkeeping, as in
 * voltrix_launch_sample_neighbors).  Columns in indices outside [0, num_cols) are never selected and never read through; a row id
 * outside [0, num_rows) has degree 0 inside the kernels (never an out-of-bounds read; callers reject it earlier).
 *   voltrix_launch_subgraph_count: counts[i] = the number of kept entries of row rows[i]; every element of counts (device
 *                                  int32[num_sub_rows]) is written;
 *   (the caller takes s_indptr = the exclusive prefix sum of counts, device int32[num_sub_rows + 1], and num_selected =
 *   s_indptr[num_sub_rows])
 *   voltrix_launch_subgraph_fill:  s_local, s_entries = device int32[num_selected]; every element of both is written, neither needs
 *                                  initialising; a row never writes more than s_indptr[i + 1] - s_indptr[i].
 * group = 4, 8, 16, 32 or 64: the lanes that own one row and walk it `group` entries at a time (coalesced loads of indices, a gather
 * of table, the group's slice of a 64-bit ballot: a stable compaction without LDS); every width gives the same bits.  A hub row is
 * walked by one group.  No atomics, no workspace, no host synchronisation inside.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any HIP call: negative sizes, num_selected > INT_MAX, a group outside the five widths,
 * a null or misaligned pointer (s_local and s_entries only where num_selected > 0); VOLTRIX_OK without a launch for num_sub_rows == 0
 * (and, for the fill, num_selected == 0).  Alignment: 4 bytes everywhere. */
void voltrix_launch_subgraph_count(void* indptr, void* indices, int num_rows, void* rows, int num_sub_rows, void* table, int num_cols,
                                   int group, void* counts, void* stream, int* return_code);
void voltrix_launch_subgraph_fill(void* indptr, void* indices, int num_rows, void* rows, int num_sub_rows, void* table, int num_cols,
                                  int group, void* s_indptr, int64_t num_selected, void* s_local, void* s_entries, void* stream,
                                  int* return_code);

/* THE WALK RULE.  nodes[w, 0] = starts[w].  At step t (0-based) walker w stands on node v of degree d = indptr[v + 1] - indptr[v]:
 *   d == 0:     the walk is over; this and every later step write -1 in nodes and in entries;
 *   otherwise:  the walker takes the entry at position (uint64(draw(w, t)) * d) >> 32 of row v: entries[w, t] is its CSR entry id,
 *               nodes[w, t + 1] its column;
 *   draw(w, t) = word t & 3 of Philox4x32-10(counter = (w, (t >> 2) | 0xC0000000, offset & 0xffffffff, offset >> 32),
 *               key = (seed & 0xffffffff, seed >> 32)); bits 31 and 30 of counter word 1 separate these draws from
 *               voltrix_launch_sample_neighbors' ((i >> 2) | 0x80000000, i < 64) and voltrix_launch_dropout_mask's (h >> 2 < 2^29):
 *               one seed for all three gives unrelated streams.
 * A node id outside [0, num_rows) -- a column of a rectangular CSR, a start the caller did not reject -- is recorded as it is and ends
 * the walk like a dead end (degree 0: indptr is never read out of bounds).  w is the walker's index in starts = device
 * int32[num_walkers]: duplicate starts are different walks; the result is a function of (seed, offset, w, starts[w], the graph) only.
 * Outputs, every element written, the -1 padding included: step_major = 0: nodes = device int32[num_walkers, length + 1], entries =
 * device int32[num_walkers, length]; step_major = 1: [length + 1, num_walkers] and [length, num_walkers] (coalesced stores).  One lane
 * per walker, one Philox evaluation per four steps; no atomics, no workspace, no host synchronisation.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any HIP call: negative sizes, length > 2^20, num_walkers * (length + 1) > INT_MAX,
 * step_major outside {0, 1}, a null or misaligned pointer (indices and entries only where length > 0); VOLTRIX_OK without a launch for
 * num_walkers == 0.  Alignment: 4 bytes everywhere. */
void voltrix_launch_random_walk(void* indptr, void* indices, int num_rows, void* starts, int num_walkers, int length, uint64_t seed,
                                uint64_t offset, void* nodes, void* entries, int step_major, void* stream, int* return_code);

/* Negative sampling on a device int32 CSR [num_rows, num_cols] and the endpoints of CSR entries (voltrix/negative_sample_kernels.hpp):
 * what link-prediction mini-batches need next to voltrix_launch_sample_neighbors (the layers) and voltrix_launch_sddmm_csr (the
 * scores).  No reference counterpart.
 * THE NEGATIVE RULE.  src = device int32[num_src] GLOBAL row ids, duplicates allowed; k slots per position, T = max_tries tries per slot:
 *   draw(p, q) = word q & 3 of Philox4x32-10(counter = (p, (q >> 2) | 0x40000000, offset & 0xffffffff, offset >> 32),
 *                key = (seed & 0xffffffff, seed >> 32)); p is the POSITION in src, not the row id, so duplicate sources get different
 *                negatives.  Bit 30 set with bit 31 clear is the last free domain of counter word 1: voltrix_launch_dropout_mask uses
 *                00, voltrix_launch_sample_neighbors 10, voltrix_launch_random_walk 11: one seed for all four gives unrelated streams.
 *   slot (p, j): the draws q = j T + t for the tries t = 0 .. T - 1 (j T need not be a multiple of 4).  Try t proposes
 *                c = (uint64(draw(p, q)) * num_cols) >> 32; it is rejected if c occurs in row src[p] and, with exclude_self = 1, if
 *                c == src[p].  neg[p, j] = the first accepted c, or -1 if all T tries are rejected.
 * Slots are independent: one column may appear twice in a row of neg.  neg[p, j] is a function of (seed, offset, p, j, src[p], T, the
 * graph) only: not of the launch geometry, of k or of the other sources.  A row id outside [0, num_rows) has degree 0 inside the kernel
 * (never an out-of-bounds read; callers reject it).  Entries of indices outside [0, num_cols) never match and are never read through.
 * num_cols == 0: every slot is -1.  assume_sorted = 1 is the PRECONDITION that every row's columns ascend (duplicates allowed): a binary
 * search, O(T log d) per slot, so a hub row costs log d; assume_sorted = 0: a linear scan by the slot's one lane, O(T d), the slow
 * path; on sorted input both give the same bits.  Output: neg = device int32[num_src, k], every element written, the -1 included;
 * nothing needs initialising.  One lane per slot, 256 per workgroup; no LDS, no atomics, no workspace, no host synchronisation.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any HIP call: negative sizes, num_entries > INT_MAX, k outside 1 .. 1024, max_tries
 * outside 1 .. 256, num_src * k > INT_MAX, exclude_self or assume_sorted outside {0, 1}, a null or misaligned pointer (indices may be
 * null where num_entries == 0); VOLTRIX_OK without a launch for num_src == 0.  Alignment: 4 bytes everywhere. */
void voltrix_launch_negative_sample(void* indptr, void* indices, int num_rows, int num_cols, int64_t num_entries, void* src, int num_src,
                                    int k, int max_tries, int exclude_self, int assume_sorted, uint64_t seed, uint64_t offset, void* neg,
                                    void* stream, int* return_code);

/* ENTRY -> ENDPOINTS.  entries = device int32[num_ids] CSR entry ids.  rows[i] = the one r with indptr[r] <= e < indptr[r + 1], found
 * as the upper bound of e in indptr minus one, so runs of empty rows before and after are stepped over (no [nnz] row-id array is
 * kept); cols[i] = indices[e].  An id outside [0, num_entries) writes (-1, -1): never an out-of-bounds read.  rows, cols = device
 * int32[num_ids], every element written.  One lane per id, O(log num_rows) reads of indptr; no atomics, no workspace, no host
 * synchronisation.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any HIP call: negative sizes, num_entries > INT_MAX, a null or misaligned pointer
 * (indices may be null where num_entries == 0); VOLTRIX_OK without a launch for num_ids == 0.  Alignment: 4 bytes everywhere. */
void voltrix_launch_edge_endpoints(void* indptr, void* indices, int num_rows, int64_t num_entries, void* entries, int num_ids, void* rows,
                                   void* cols, void* stream, int* return_code);

/* Neighbour sampling that leaves a set of CSR entries out (voltrix/neighbor_sample_kernels.hpp): what keeps a link-prediction
 * batch's positive edges and their reverses out of the sampled blocks (DGL's exclude="reverse_id").  No reference counterpart.
 * THE EXCLUSION RULE.  exclude = device int32[num_exclude] CSR entry ids, STRICTLY ASCENDING (sorted, distinct), each in [0, nnz): the
 * caller's to guarantee, not checked on the device.  For a seed row r with begin = indptr[r], end = indptr[r + 1], d = end - begin:
 *   lo = lower_bound(exclude, begin), hi = lower_bound(exclude, end), x = hi - lo;
 *   the excluded positions of the row are q_i = exclude[lo + i] - begin, i = 0 .. x - 1, ascending;
 *   the candidates are the d' = d - x positions of the row not among the q_i, in CSR order;
 *   candidate number t is position cand(t) = t + #{ i : q_i - i <= t } (q_i - i does not decrease: one binary search, O(log x)).
 * THE SAMPLING RULE of voltrix_launch_sample_neighbors then applies unchanged with d' in place of d, every position it yields mapped
 * through cand: replace = 0, d' <= k (and fanout = -1): every candidate in CSR order; replace = 0, d' > k: Floyd's algorithm on
 * 0 .. d' - 1 with the same draw(r, i) and the same counter domain, output ascending; replace = 1, d' > 0: k entries at
 * cand((uint64(draw(r, i)) * d') >> 32); d' = 0: nothing.  A row none of whose entries is excluded gets exactly the bits
 * voltrix_launch_sample_neighbors gives it, and num_exclude == 0 (exclude may be NULL then) gives that call's bits for every row.  The
 * result is a function of (seed, offset, r, d', k) and the row's excluded positions only; sorted rows stay sorted; s_entries holds ids
 * into the original indices.  s_indptr = the caller's prefix sum of the per-seed counts the rule gives with d' (min(d', k); d' > 0 ? k
 * : 0 with replace; d' for fanout = -1).  Every element of s_indices and s_entries is written then; a row never writes past its
 * segment, and no list, however malformed, makes the kernel read outside the row.  One lane per seed, 256 per workgroup, two binary
 * searches in exclude per row and one per output entry on top of voltrix_launch_sample_neighbors: the cost does not follow the degree
 * (fanout = -1 and d' <= k merge the row against its slice of exclude with one lane: O(d)).  No atomics, no workspace, no host
 * synchronisation.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any launch: what voltrix_launch_sample_neighbors refuses, num_exclude < 0, a misaligned
 * exclude, a null exclude with num_exclude > 0; VOLTRIX_OK without a launch for num_seeds == 0 or num_sampled == 0.  Alignment: 4 bytes
 * everywhere. */
void voltrix_launch_sample_neighbors_excluding(void* indptr, void* indices, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                               int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* exclude,
                                               int num_exclude, void* s_indices, void* s_entries, void* stream, int* return_code);

/* Weighted neighbour sampling on integer cumulative weights (voltrix/weighted_sample_kernels.hpp): DGL's sample_neighbors(prob=) --
 * importance sampling, edge-weight-biased GraphSAGE, masking entries with zero weights.  No reference counterpart.  (Not a
 * voltrix_launch_ name: it joins the launchers' host-contract table when that table is next opened.)
 * THE WEIGHT TABLE.  For an entry e of row r with weight w_e >= 0 (finite) and m_r = the largest weight of the row, in float64:
 *   q_e = 0 where w_e == 0 or m_r == 0, otherwise q_e = max(1, floor((w_e / m_r) * 2^30))
 * (one correctly rounded division, an exact multiplication, an exact floor): 0 <= q_e <= 2^30, a positive weight stays positive, a zero
 * weight is never sampled, q_e / 2^30 is within 2^-30 of w_e / m_r.  cum = device int64[nnz], the inclusive prefix sum of q over the
 * whole entry array (at most nnz 2^30 < 2^61), 8 bytes per entry: the caller builds it (voltrix.sampling_weights does).
 * THE SAMPLING RULE.  Row r with begin = indptr[r], d = indptr[r + 1] - begin, fan-out k = fanout:
 *   base = begin > 0 ? cum[begin - 1] : 0 (cum[-1] is never read); c(j) = cum[begin + j] - base; T = c(d - 1); p = the number of
 *   entries of the row with q > 0;
 *   draw(r, n) = word n & 3 of Philox4x32-10(counter = (r, (n >> 2) | 0xA0000000, offset & 0xffffffff, offset >> 32),
 *                key = (seed & 0xffffffff, seed >> 32)), n < 128: bits 31 and 29 of counter word 1, a part of
 *                voltrix_launch_sample_neighbors' domain that its own draws (0x80000000 | (i >> 2), i < 64) never enter;
 *   x_i = (uint64(draw(r, 2 i)) << 32) | draw(r, 2 i + 1); a uniform integer below R is umulhi64(x_i, R) = (x_i R) >> 64: an entry's
 *                probability differs from q_e / R by less than 2^-63;
 *   replace = 0, p <= k: every entry with q > 0, in CSR order, no draw used.  fanout = -1 (VOLTRIX_SAMPLE_ALL) means this for every row,
 *                whatever replace is.
 *   replace = 0, p > k:  successive sampling: for i = 0 .. k - 1, R_i = T - (the sum of q over the entries chosen so far),
 *                t = umulhi64(x_i, R_i); choose the smallest position j with g(j) > t, g(j) = c(j) - (the sum of q_s over chosen
 *                s <= j).  g does not decrease and is flat at chosen positions and zero weights, so j is new and has q > 0.  The k
 *                positions are output in ascending order (sorted rows stay sorted).
 *   replace = 1, T > 0:  exactly k entries, entry i at the smallest j with c(j) > umulhi64(x_i, T), in draw order; T == 0: none.
 * A function of (seed, offset, r, k) and the row's q values only; equal weights do NOT give voltrix_launch_sample_neighbors' bits.
 * seeds, s_indices, s_entries as for voltrix_launch_sample_neighbors; a seed outside [0, num_rows) has degree 0 inside the kernel.
 * s_indptr = device int32[num_seeds + 1], the caller's prefix sum of the per-seed counts the rule gives (min(p, k); T > 0 ? k : 0 with
 * replace; p for fanout = -1); num_sampled = s_indptr[num_seeds].  It is how the kernel learns p: a segment shorter than k gets every
 * positive entry, a segment of k is drawn.  Every element of s_indices and s_entries is written when s_indptr is the rule's; a row never
 * writes past its segment, and every read of cum and indices stays inside the row whatever cum and s_indptr hold.  One lane per seed,
 * 256 per workgroup; the chosen positions live sorted in 256 k 4 bytes of dynamic LDS (replace = 0 only); per row O(k (k + log d))
 * loads of cum whatever the degree, no loop whose trip count depends on a draw (fanout = -1 is O(d) at worst); no atomics, no
 * workspace, no host synchronisation, the same bits on every call.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any HIP call: negative sizes, num_sampled > INT_MAX, fanout outside 1 .. 64 and not -1,
 * replace outside {0, 1}, a null or misaligned pointer (indices, cum, s_indices, s_entries only where num_sampled > 0); VOLTRIX_OK
 * without a launch for num_seeds == 0 or num_sampled == 0.  Alignment: cum 8 bytes, 4 bytes everywhere else. */
void voltrix_sample_neighbors_weighted(void* indptr, void* indices, void* cum, int num_rows, void* seeds, int num_seeds, void* s_indptr,
                                       int64_t num_sampled, int fanout, int replace, uint64_t seed, uint64_t offset, void* s_indices,
                                       void* s_entries, void* stream, int* return_code);

/* (ROW, COLUMN) -> ENTRY (DGL's edge_ids / has_edges_between).  rows, cols = device int32[num_queries].  out[i] = the id of the FIRST
 * entry of row rows[i] whose column is cols[i]; -1 if there is none or rows[i] is outside [0, num_rows).  No [nnz] key array is kept,
 * so this is a search: assume_sorted = 1 is the PRECONDITION that every row's columns ascend (duplicates allowed): a lower bound,
 * O(log d); assume_sorted = 0: a linear scan by the query's one lane, O(d), the slow path; on sorted input both give the same bits.
 * out = device int32[num_queries], every element written.  One lane per query; no atomics, no workspace, no host synchronisation.
 * VOLTRIX_ERR_BAD_SHAPE, on the host and before any HIP call: negative sizes, num_entries > INT_MAX, assume_sorted outside {0, 1}, a
 * null or misaligned pointer (indices may be null where num_entries == 0); VOLTRIX_OK without a launch for num_queries == 0.
 * Alignment: 4 bytes everywhere. */
void voltrix_launch_find_edges(void* indptr, void* indices, int num_rows, int64_t num_entries, void* rows, void* cols, int num_queries,
                               int assume_sorted, void* out, void* stream, int* return_code);

/* Rows of a dense row-major matrix times a per-row factor: dst[i, :] = T(float(src[i, :]) * scale[i]); dst may be src.
 * dtype 0 fp32 / 1 fp16 / 2 bfloat16; a row (num_feats elements) must be a multiple of 16 bytes; scale: device float[rows].
 * What edge values of the form v_ij = r_i * c_j cost on top of the binary product (voltrix/weighted.py: B's rows times c before,
 * C's rows times r after -- the normalised adjacencies of GCN / mean aggregation); the reference has no edge values at all
 * (spmm_kernels.cuh:1632-1644: bits -> 1.0).  Every element of dst is written.
 * Alignment: src and dst 16 bytes (16 bytes per lane; anything else is
 * VOLTRIX_ERR_BAD_SHAPE on the host, before any launch), scale 4 bytes. */
void voltrix_launch_scale_rows(void* src, void* scale, void* dst, int64_t rows, int num_feats, int dtype, void* stream,
                               int* return_code);

/* Fused GPU preprocess: CSR on the DEVICE -> (pointer1, hspa_packed, hind) without the reference's host
 * preprocess, the O(TCb*E) rescan or the 512-byte/TC-block fp32 `hspa` intermediate.  Two phases because the
 * caller owns every buffer and T is data dependent:
 *   phase 1  voltrix_launch_csr_window_count: block_partition[W], pointer1[W+1], status[1] (device int32)
 *            workspace: voltrix_csr_preprocess_workspace_bytes(num_nodes, num_cols, num_edges, path) bytes, device, 16-B aligned,
 *            need not be initialised (the launch clears the four queue counters on the paths that queue windows; keys, queues and
 *            range groups are written for exactly the windows they are later read for); every element of all three outputs is written
 *   (caller reads T = pointer1[W] and status[0], allocates hspa_packed uint32[4T] and hind int32[8T])
 *   phase 2  voltrix_launch_csr_fill: writes hspa_packed and hind (every word), same workspace, same num_cols.
 * num_cols = the column universe: every id in edge_list lies in [0, num_cols) (square adjacency: num_nodes; a row shard
 * whose ids index a gathered B: the rows of that buffer).  num_cols <= 0 = unknown.  The condensed-column ranks come
 * from an LDS bitmap + popcounts when the universe fits LDS (num_cols <= 2^19) and is small next to a window's edge
 * list, otherwise from a per-window sort (needs the 4-byte-per-edge key workspace); universes of 2 .. 16 bitmap ranges
 * (up to 2^23 columns) sort the windows up to 8192 edges and send only the bigger ones through the bitmap kernels, one
 * sweep per range ("mixed").  path = -1 (VOLTRIX_CSR_AUTO): that rule; 0 sort / 1 bitmap / 2 mixed force a path where it is
 * applicable (the same value in all three calls; how the tests reach every path on one graph).  status[0] = number of edges with an id outside [0, num_cols) (outside
 * [0, 2^28) when num_cols <= 0): the handle is valid only if it is 0 (callers retry with num_cols = 0 or reject).
 * Output is bit-identical to preprocess + hmat_gen + hmat_packed_swizzle on every path. */
int64_t voltrix_csr_preprocess_workspace_bytes(int num_nodes, int num_cols, int64_t num_edges, int path);
void voltrix_launch_csr_window_count(void* node_pointer, void* edge_list, int num_nodes, int num_cols, int64_t num_edges,
                                     int path, void* workspace, void* block_partition, void* pointer1, void* status,
                                     void* stream, int* return_code);
void voltrix_launch_csr_fill(void* node_pointer, void* edge_list, int num_nodes, int num_cols, int64_t num_edges,
                             int path, void* workspace, void* pointer1, void* hspa_packed, void* hind, void* stream,
                             int* return_code);

/* Cuthill-McKee row order on the device (locality reorder; no reference counterpart -- the
 * reference reads externally reordered <name>.reorder.npz files, bench/graph_gen.py:42-45, bench/bench_all.py:120-129).
 * Specification (voltrix/reorder_kernels.hpp; oracle/oracle_np.py::cm_order restates it): nodes = rows u < num_nodes;
 * u, v are neighbours when A[u, v] or A[v, u] is stored (columns >= num_nodes are not nodes); deg(u) = entries of row u of
 * A + entries of row u of A^T; tie(u) = position of u in the stable sort by deg.  A component is searched breadth first
 * from `start`; inside level d the nodes are ordered by (rank of the earliest-ranked neighbour of level d - 1, tie).
 * The result is a function of the CSR alone -- no race decides anything -- whatever the order inside A^T's rows.
 *   voltrix_launch_csr_transpose: CSR of A^T (t_indptr int32[num_cols + 1], t_indices int32[num_edges]; rows sorted,
 *       duplicates kept; entries with a column id outside [0, num_cols) left out) -- the search walks row u of A and row u of
 *       A^T, and the backward pass of the SpMM multiplies with it (voltrix/autograd.py).  Row ids expanded per entry, one
 *       stable radix sort by column, row pointers by binary search: no atomics.  workspace:
 *       voltrix_csr_transpose_workspace_bytes(num_edges) bytes, device, 16-byte aligned, need not be initialised; every element of
 *       t_indptr and t_indices is written.
 *   voltrix_launch_bfs_seed: level[start] = 0 (level int32[num_nodes], -1 = unvisited: THE CALLER SETS IT, and rank, to -1 before
 *       the first component and keeps them across components; queue, ctrl and level_off need not be initialised: the seed
 *       writes what the level launches read), queue[0] = start (queue int32[num_nodes]),
 *       ctrl int32[8] = {head, tail, appended, depth, done, ...},
 *       level_off int32[num_nodes + 2] (level_off[d] = queue position of level d's first node).
 *   voltrix_launch_bfs_levels: one single-workgroup launch that walks every level while the frontier stays <= 2048 nodes,
 *       then `wide_levels` whole-chip levels.  The caller reads ctrl (its sync) and calls again until ctrl[4] != 0; then
 *       levels = ctrl[3] + 1, nodes of the component = ctrl[1] = level_off[levels], queue[0 .. nodes) = the component level
 *       by level (order inside a level: arbitrary so far).
 *   voltrix_launch_cm_rank: orders every level's queue segment (levels <= 1024 nodes: one workgroup walks runs of them,
 *       LDS bitonic; larger: keys + radix sort, workspace voltrix_cm_rank_workspace_bytes(largest level above 1024) bytes)
 *       and writes rank[v] = base + position (rank int32[num_nodes]).  level_off_host: HOST copy of level_off[0 .. levels].
 *       tie int32[num_nodes].  Afterwards queue[0 .. nodes) is the component's order.
 * Pointers: indices / t_indices may be empty (no entries); the transpose needs indptr, indices, t_indices and its workspace only when
 * num_edges > 0, t_indptr always; everything else is required, level_off_host (read on the HOST) included; the workspace of
 * voltrix_launch_cm_rank is optional (no level above 1024 nodes).  A NULL required pointer, a misaligned transpose workspace, start
 * outside [0, num_nodes), num_nodes <= 0 in the search: VOLTRIX_ERR_BAD_SHAPE on the host, before any launch. */
int64_t voltrix_csr_transpose_workspace_bytes(int64_t num_edges);
void voltrix_launch_csr_transpose(void* indptr, void* indices, int num_rows, int num_cols, int64_t num_edges, void* workspace,
                                  void* t_indptr, void* t_indices, void* stream, int* return_code);
void voltrix_launch_bfs_seed(int start, int num_nodes, void* level, void* queue, void* ctrl, void* level_off, void* stream,
                             int* return_code);
void voltrix_launch_bfs_levels(void* indptr, void* indices, void* t_indptr, void* t_indices, int num_nodes, int t_rows,
                               void* level, void* queue, void* ctrl, void* level_off, int wide_levels, void* stream,
                               int* return_code);
int64_t voltrix_cm_rank_workspace_bytes(int64_t max_level);
void voltrix_launch_cm_rank(void* indptr, void* indices, void* t_indptr, void* t_indices, int num_nodes, int t_rows,
                            void* level, void* rank, void* tie, void* queue, void* level_off, const int* level_off_host,
                            int num_levels, int base, void* workspace, void* stream, int* return_code);

/* out = inv(chol(gram + eps trace(gram) I))^T for a k x k symmetric positive semi-definite gram (float32, row-major,
 * k <= 64), float32 [k][k]: the small factor of a Cholesky QR (X <- X out has orthonormal columns), on the device so that
 * the spectral row order's subspace iteration (voltrix/reorder.py) has no host sync per step.  One workgroup, double
 * arithmetic.  VOLTRIX_ERR_BAD_SHAPE for k outside 1..64 or a NULL gram / out, on the host, before any launch.  Every element of out is
 * written (the elements below the diagonal as 0).  gram need not be exactly symmetric: 0.5 (gram + gram^T) is what is factored.  A
 * pivot that is not positive (a rank-deficient subspace) is replaced by eps trace(gram), or by 1e-300 when that is not positive. */
void voltrix_launch_chol_inv_transposed(void* gram, int k, double eps, void* out, void* stream, int* return_code);

#ifdef __cplusplus
}
#endif
#endif /* VOLTRIX_CAPI_H_ */
