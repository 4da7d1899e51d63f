/* hipstr_hmm_debug.h — diagnostics entry points of libhipstr_hmm.so (round 6: split from hipstr_hmm.h).
 *
 * NOT part of the drop-in boundary: nothing on the reference side binds these.  They exist for the test suite (tests/), the fuzzers
 * (tools/fuzz_*.py) and the measurement harness (bench.py) — host-only views of the preparation, the block caches' counters, the
 * device's copies of tables, a correctly-rounded-math probe.  A deployment build compiles the library with -DHIPSTR_NO_DEBUG_ABI and
 * none of them is defined or exported (tests/test_prep.py::test_library_exports_every_declared_symbol checks the default build, which
 * has them). */
#ifndef HIPSTR_HMM_DEBUG_H
#define HIPSTR_HMM_DEBUG_H
#include "hipstr_hmm.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Diagnostics (host only, no device): the haplotype rows of allele k of a ONE-locus batch as the
 * device sweep consumes them — side 0 = forward/left problem, 1 = reversed/right problem; which 0 =
 * leading flank block, 1 = trailing flank block.  Row encoding: bits 0-7 base, 8-11 homopolymer index
 * min(15, ..) of HapAligner.cpp:119-120, 12-23 compact row index, bit 31 valid.  Returns the row
 * count (0 if the allele is not realigned, -1 on error).  Used by tests/test_prep.py. */
int hipstr_debug_rows(const hipstr_batch_t* batch, int k, int side, int which, uint32_t* rows, int cap);

/* Diagnostics (host only): the host preparation of a batch (flatten, reuse replay, visiting lists, closed-form tables, launch plan
 * — what hipstr_hmm_upload does before any byte moves) run with `threads` host threads (0 = the library default,
 * HIPSTR_HOST_THREADS or min(hardware threads, 32)); *seconds = its wall time, *digest = a hash of everything it produced, which
 * must not depend on the thread count.  Used by tests/test_prep.py and bench.py. */
int hipstr_debug_prepare(const hipstr_batch_t* batch, int threads, double* seconds, uint64_t* digest);

/* Diagnostics (host only): the STR-block groups of the launch plan — reads of one locus and side whose columns are laid end to end over
 * one workgroup's lanes (hs_str_group_kernel).  Group g: side[g], reads[read_off[g] .. read_off[g+1]) (read indices of the batch),
 * columns[g] = the sum of their side lengths.  Returns the number of groups (-1 on error or if a capacity is too small); *max_columns =
 * lanes of a workgroup.  Used by tests/test_prep.py. */
int hipstr_debug_str_groups(const hipstr_batch_t* batch, int32_t* side, int32_t* columns, int32_t* read_off, int cap_groups,
                            int32_t* reads, int cap_reads, int32_t* max_columns);

/* Diagnostics (host only): the launch plan hipstr_hmm_align would run for a batch, with a workspace budget of ws_gib GiB per workspace
 * (<= 0: the upload's own, HIPSTR_WS_GIB or its default), from the same decisions the launches take — the flank shapes (and the
 * HIPSTR_FLANK_SYSTOLIC mode in force), the coop sweeps' bands per item, the STR-block kernels, the combine forms — as one JSON object:
 * "thresholds" (the limits compiled into the library, "shapes": [rows per band, bands per round] per flank shape), "routes" (every route
 * name there is) and per chunk "lead" / "trail" (route, items, per item in launch order [rows, rounds, bands of the last round, band
 * heights] or, systolic, [rows, bands of 64 rows]), "str" (kernels launched, (read side, allele) pairs per kernel, side stream, long
 * sides), "combine" ((read, allele) pairs per form: per-allele, 1..4 rounds of 64) and "routes" (the ones the chunk takes).  Writes up to
 * cap - 1 bytes and a NUL; returns the full length (-1 on error).  Used by tests/test_routes.py. */
int hipstr_debug_launch_plan(const hipstr_batch_t* batch, double ws_gib, char* json, int cap);

/* Diagnostics (host only): what hipstr_hmm_trace_seeded would launch for a request list (req_seed may be NULL), with a budget of ws_mib MiB
 * of decision matrices per chunk (<= 0: the call's own default or HIPSTR_TRACE_WS_MIB; where the call would ask the device for its free
 * memory the plan keeps that budget), from the same decisions the call takes, as one JSON object: "thresholds" (the compiled limits;
 * "fill_cols": template argument of the fill kernel per column class 1..HS_MAX_COLS), "routes" (every route name there is),
 * "compact_reads" (only the requested reads' bases are uploaded), and per chunk "q0" / "q1" (request range), "bytes", "classes" (sides per
 * column class), "mixed" (hs_trace_fill_mixed takes the static classes), "launch" ([kernel, workgroups]), "requests" ([left columns, right
 * columns, flank rows + 1, left walk, right walk]: walk 1 = decision bytes copied to LDS, 0 = read in the workspace) and "routes" (the ones
 * the chunk takes; "mixed<C>": class C inside the mixed launch).  Writes up to cap - 1 bytes and a NUL; returns the full length (-1 on
 * error).  Used by tests/test_stage_routes.py. */
int hipstr_debug_trace_plan(const hipstr_batch_t* batch, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                            const int32_t* req_seed, double ws_mib, char* json, int cap);
/* Diagnostics (host only): the slots hipstr_hmm_trace_ex(HIPSTR_TRACE_ASSEMBLE_DEVICE) gives every request of a list (req_seed and hap_to_ref
 * may be NULL) and the route its staging takes, from the functions the call and hs_trace_assemble use: "thresholds" ("HS_ASM_LDS": bytes of
 * staging a wavefront keeps in LDS), "routes" (every route name), "fields" (the columns of "requests"), "requests" (per request: entries of
 * the hap_aln slot, of each sequence piece, of the indel and SNP pair lists, of the stitched string / CIGAR / alignment string, the bytes it
 * would stage, 1 = staged in LDS / 0 = read in HBM) and "routes_hit".  Refusals as in the call.  Same conventions as hipstr_debug_trace_plan.
 * Used by tests/test_trace_assemble_host.py. */
int hipstr_debug_trace_assemble_plan(const hipstr_batch_t* batch, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                     const int32_t* req_seed, const char* const* hap_to_ref, char* json, int cap);
/* Diagnostics: a resident traceback result (hipstr_trace_dev_t) built from host arrays, so that fabricated edge cases run through
 * hipstr_post_census_dev and hipstr_assign_trace_stats_dev.  tr: arrays for n_req requests; one that is NULL is absent — its group cannot
 * be fetched, and a consumer that needs it refuses.  Nothing about the values is checked here (the consumers do that, on the device).
 * *td = NULL on failure.  Freed with hipstr_trace_dev_free.  Used by tests/test_trace_resident_gpu.py. */
int hipstr_debug_trace_dev_from_host(const hipstr_trace_out_t* tr, int32_t n_req, hipstr_trace_dev_t** td);
/* Diagnostics (host only): the chunks hipstr_nw_align would cut a batch into under a budget of ws_mib MiB of traceback bytes (<= 0: the
 * call's own default or HIPSTR_NW_WS_MIB) and, per chunk, "p0" / "p1" (pair range), "bytes", "over_budget" (one pair larger than the
 * budget, alone), "rungs" (pairs per rows-per-lane rung of "thresholds"."rows") and "launch" ([kernel, workgroups]).  Refused sizes fail
 * as in the call.  Same conventions as hipstr_debug_trace_plan. */
int hipstr_debug_nw_plan(const hipstr_nw_batch_t* batch, double ws_mib, char* json, int cap);
/* Diagnostics (host only): the launch hipstr_post_launch would make for a posterior batch — "n_units", "max_nd" (diplotypes of the largest
 * unit), "split" (workgroups per unit of the accumulation; > 1: hs_posterior_accumulate_kernel + hs_posterior_finish_kernel), "launch" and per
 * unit [alleles, reads, path (0 = registers, 1 = chunked), reads per LDS tile, tiles, chunks of HS_POST_ECHUNK exponentials, workgroups of
 * a split launch with an empty share], "routes_hit".  (HIPSTR_DEBUG_HOST_LIBM, which sends every unit down the chunked path, is not
 * modelled.)  Same conventions as hipstr_debug_trace_plan. */
int hipstr_debug_post_plan(const hipstr_post_batch_t* batch, char* json, int cap);
/* Diagnostics (host only): the launch decisions hipstr_em_train takes for a batch, after the same per-locus preparation and validation (a
 * batch the call refuses fails the plan with the same hipstr_last_error()): "thresholds" (hipstr_amd/csrc/em_layout.h's limits, "int_log_len"
 * = entries of the table of integer logarithms, "last_round" = last value of the host's round counter for the batch's max_iter), "routes"
 * (every route name), per locus "A", "S", "R", "gmax" ("wave" / "thread"), "row_tile" (posterior rows per LDS tile, or "direct"), "row_tiles",
 * "last_row_tile", "sweeps" and "last_sweep" (alleles of the last one), "scan_chunks" and "scan_last" (positions of the last chunk of a chain
 * of S + S A), "slice_rows" ([fewest, most] rows of the HS_EM_PARTS slices of the R A rows), "empty_slices", "slice_tiles" (tiles of
 * HS_EM_TILE rows of the fullest slice), "post" ([path of the posterior kernel, reads of the locus' largest unit, reads per LDS tile, tiles],
 * post_layout.h); for the batch "init_blocks", "compact_chunks", "compact_last_chunk", "max_S", "units_passes" and "routes_hit".  Same
 * conventions as hipstr_debug_trace_plan.  Used by tests/test_em_routes.py. */
int hipstr_debug_em_plan(const hipstr_em_batch_t* batch, char* json, int cap);
/* Diagnostics (host only): the launch decisions of hipstr_post_assign (post_layout.h) for a batch whose largest (locus, sample) unit has
 * max_unit_reads reads and n_units units, and for a locus of n_keys = pools x haplotypes keys and n_reads reads: out[0] wavefronts per unit
 * (1: four units share a workgroup; 4: a unit has the workgroup), out[1] workgroups, out[2] slots of the locus' first-occurrence table,
 * out[3] 1 = hashed, 0 = direct. */
int hipstr_debug_assign_plan(int32_t max_unit_reads, int64_t n_units, int64_t n_keys, int64_t n_reads, int64_t out[4]);

/* Diagnostics (host only): the route hipstr_rm_scatter / hipstr_rm_remap give a locus of n_alleles haplotypes with n_items work items (mate groups
 * of a scatter, rows of a remap; hipstr_amd/csrc/readmat_layout.h): out[0] 0 = narrow (n_alleles <= 32: several items packed into a wavefront),
 * 1 = wide (an item has the wavefront), out[1] lanes per item, out[2] items per wavefront, out[3] wavefronts of the locus, out[4] column
 * steps per lane (wide: ceil(n_alleles / 64)). */
int hipstr_debug_rm_plan(int32_t n_alleles, int64_t n_items, int64_t out[5]);

/* Diagnostics (host only): the route hipstr_post_census gives a locus of n_req requests and n_reads un-pooled reads
 * (hipstr_amd/csrc/census_layout.h): out[0] 0 = a wavefront per locus (four loci per workgroup, workspace in LDS), 1 = a workgroup per locus
 * with the workspace in LDS, 2 = a workgroup per locus with the workspace in a global block; out[1] dwords of the locus' workspace, out[2]
 * lanes of the locus, out[3] loci per workgroup, out[4] dwords the locus takes of the global block (route 2, else 0); then the compiled
 * limits: out[5] HS_CENSUS_WAVE_REQS, out[6] HS_CENSUS_WAVE_READS, out[7] HS_CENSUS_LDS_INTS, out[8] HS_CENSUS_THREADS, out[9]
 * HS_CENSUS_REQ_INTS.  Used by tests/test_census_plan.py. */
int hipstr_debug_census_plan(int64_t n_req, int64_t n_reads, int64_t out[10]);

/* Diagnostics (host only): what hipstr_pool_reads would do with a batch under a budget of ws_mib MiB of workspace per chunk (<= 0: the
 * call's own default or HIPSTR_POOL_WS_MIB), from the functions of hipstr_amd/csrc/pool_layout.h the call and its kernels use, as one JSON
 * object: "thresholds" (the compiled limits), "routes" (every route name: a locus is pooled on the "device" or, for its size, on the
 * "host"; a pool's medians are a "copy", come from the "net" or from the "radix" select), per chunk "l0" / "l1" (locus range), "reads" and
 * "bytes" (uploaded reads and the workspace they take), "device_loci", "host_loci", "lds_bytes" (of the grouping launch), "hash_steps"
 * (most steps of a hash wavefront), "pools" ([copy, net, radix]: pools by median route, from the host's pooling) and "routes_hit".  Same
 * conventions as hipstr_debug_trace_plan.  Used by tests/test_pool_host.py. */
int hipstr_debug_pool_plan(const hipstr_batch_t* unpooled, double ws_mib, char* json, int cap);
/* Diagnostics (host only): what hipstr_flank_assemble_dev would do with a request on the strings of `tr` (flank_seq_off / flank_seq), from the
 * functions of hipstr_amd/csrc/flank_layout.h the call and its kernel use, as one JSON object: "thresholds" (the compiled limits, "lds_bytes"
 * of a workgroup), "caps" (the limits of this call: the compiled ones, or smaller ones from HIPSTR_DEBUG_FLANK_CAPS =
 * "edges,nodes,recs,reads,len,path_len", read per call; 0 or missing = the compiled limit), "peel_rounds", "routes" (every route name), "fields"
 * (the columns of "tasks"), per task, in task order, [accepted k, most distinct edges, most nodes, path records, reads of the run, longest
 * string that entered (the reference flank included), longest path, strings that entered at the last k, HS_FLK_F_* flags, route index],
 * "routes_hit", "pool_bytes" and "workgroups".  The sizes come from the host twin.  Refusals as in hipstr_flank_assemble.  Same conventions as
 * hipstr_debug_trace_plan.  Used by tests/test_flank_plan.py. */
int hipstr_debug_flank_plan(const hipstr_post_batch_t* pb, const hipstr_flank_request_t* rq, const hipstr_trace_out_t* tr, char* json, int cap);
/* Diagnostics: the calling thread's last hipstr_flank_assemble_dev: out[0] tasks, out[1] tasks skipped, out[2] tasks the host twin assembled
 * for a limit, out[3] 1 when the flank strings were fetched, out[4] bytes sent to the device, out[5] bytes copied back; flags (HS_FLK_F_* per
 * task as the kernel set them) and sizes (per task: most edges, most nodes, path records, strings that entered, as the kernel counted
 * them up to where it stopped) are filled for up to cap_tasks tasks and may be NULL.  A refused call leaves the numbers of the call before. */
int hipstr_debug_flank_last(int64_t out[8], int32_t* flags, int32_t* sizes, int64_t cap_tasks);
/* Diagnostics: the calling thread's last hipstr_bias_pvalues or hipstr_record_fields: out[0] lanes (quadruples or samples), out[1] those the
 * host twin computed inside the call because their counts exceed the device's table, out[2] bytes sent to the device, out[3] bytes copied
 * back.  A call that was refused, or that had nothing to do, leaves zeros.  Used by tests/test_record_gpu.py and
 * tools/record_fields_timing.py. */
int hipstr_debug_record_last(int64_t out[4]);
/* Diagnostics: the calling thread's last hipstr_cigar_bp_diffs or hipstr_sample_histograms: out[0] reads or samples, out[1] those the host
 * twin did inside the call because they exceed HIPSTR_CIGAR_DEVICE_RUNS or HIPSTR_HISTOGRAM_DEVICE_READS, out[2] bytes sent to the device,
 * out[3] bytes copied back.  A call that was refused, or that had nothing to do, leaves zeros.  Used by tests/test_record_reads_gpu.py
 * and tools/record_alleles_timing.py. */
int hipstr_debug_record_reads_last(int64_t out[4]);
/* Diagnostics: the calling thread's last hipstr_record_alleles: out[0] loci, out[1] those the host twin did inside the call (more than
 * HIPSTR_ALLELES_DEVICE_OPTIONS options), out[2] bytes sent to the device, out[3] bytes copied back.  Used by tests/test_record_alleles_gpu.py. */
int hipstr_debug_record_alleles_last(int64_t out[4]);
/* Diagnostics: the calling thread's last hipstr_pool_reads (or hipstr_pool_batch on the device): out[0] loci pooled on the device, out[1]
 * loci the host pooled for their size, out[2] loci the host redid after a hash collision, out[3..5] pools of the device's loci by median
 * route (copy, net, radix), out[6] chunks, out[7] reads uploaded.  hipstr_debug_pool_last_timing: out[0] milliseconds between HIP events
 * around the call's kernels (0 unless HIPSTR_POOL_TIMING is set), out[1] bytes sent to the device, out[2] bytes copied back, out[3] seconds
 * the host spent staging the reads.  A call that was refused leaves the numbers of the call before it; one that failed on the way leaves
 * zeros.  Used by tests/test_pool_gpu.py and tools/pool_timing.py. */
int hipstr_debug_pool_last(int64_t out[8]);
int hipstr_debug_pool_last_timing(double out[4]);
/* Diagnostics (host only): what hipstr_hapgen would do with a request under a budget of ws_mib MiB of workspace per chunk (<= 0: the
 * call's own default or HIPSTR_HAPGEN_WS_MIB), from the functions of hipstr_amd/csrc/hapgen_layout.h the call and its kernels use, as one
 * JSON object: "thresholds" (the compiled limits), "budget_bytes", "max_lds_bytes" (the grouping workgroup's LDS at the caps), "routes"
 * (a locus is done on the "device" or, for its reads or samples, on the "host"), per chunk "l0" / "l1", "reads" and "bytes" (uploaded reads
 * and the workspace they take), "device_loci", "host_loci", "lds_bytes", and "routes_hit".  A locus with more distinct strings than
 * HS_HAPGEN_MAX_DISTINCT is found on the device only and is not in the plan.  Refusals as hipstr_hapgen (-1).  Same conventions as
 * hipstr_debug_trace_plan.  Used by tests/test_hapgen_host.py. */
int hipstr_debug_hapgen_plan(const hipstr_batch_t* reads, const hipstr_hapgen_request_t* rq, double ws_mib, char* json, int cap);
/* Diagnostics: the calling thread's last hipstr_hapgen (or hipstr_hapgen_batch on the device): out[0] loci done on the device, out[1] loci
 * the host did for their size (reads, samples, or distinct strings found on the device), out[2] loci the host redid after a hash
 * collision, out[3] chunks, out[4] reads uploaded, out[5..7] 0.  hipstr_debug_hapgen_last_timing: out[0] milliseconds between HIP events
 * around the call's kernels (0 unless HIPSTR_HAPGEN_TIMING is set), out[1] bytes sent to the device, out[2] bytes copied back, out[3]
 * seconds the host spent staging.  HIPSTR_DEBUG_HAPGEN_HASH_BITS (read by every call) keeps that many low bits of the hash: collisions at
 * test sizes.  A refused call leaves the numbers of the call before it; one that failed on the way leaves zeros.  Used by
 * tests/test_hapgen_gpu.py and tools/hapgen_timing.py. */
int hipstr_debug_hapgen_last(int64_t out[8]);
int hipstr_debug_hapgen_last_timing(double out[4]);
/* Diagnostics of hipstr_alleles_apply / _apply_host / _step.  hipstr_debug_alleles_hash_bits(bits): both forms keep that many low bits of
 * a haplotype's hash from now on (process-wide; 0 = all 64): unequal strings share hashes at test sizes, which the byte comparison must
 * tell apart.  hipstr_debug_alleles_last: the calling thread's last call: out[0] loci done on the device, out[1] loci done by the host code
 * (all of them for the host form; for the device form the loci beyond a limit of hipstr_amd/csrc/alleles_layout.h), out[2] table probes,
 * out[3] byte comparisons of two haplotypes, out[4] loci that took the identity, out[5] chunks, out[6..7] 0.  _last_timing: out[0]
 * milliseconds between HIP events around the call's kernels (0 unless HIPSTR_ALLELES_TIMING is set), out[1] bytes sent to the device,
 * out[2] bytes copied back, out[3] 0.  _limits: out[0] threads of the workgroup, out[1] most haplotypes and out[2] most options of a locus
 * the device takes, out[3] table slots.  A refused call leaves the numbers of the call before it; one that failed on the way leaves zeros.
 * Used by tests/test_alleles_*.py and tools/alleles_timing.py. */
int hipstr_debug_alleles_hash_bits(int bits);
int hipstr_debug_alleles_last(int64_t out[8]);
int hipstr_debug_alleles_last_timing(double out[4]);
int hipstr_debug_alleles_limits(int64_t out[4]);

/* Diagnostics (host only): the decisions hipstr_em_train_dev takes (hipstr_amd/csrc/em_input_layout.h) for a batch of n_runs (locus, sample)
 * runs whose run in question has run_reads reads, and for a locus whose sizes (ref_allele included) lie in [lo, hi] and are n_sizes many:
 * out[0] steps of a wavefront over the run, out[1] reads of its last step, out[2] workgroups of the select / scatter launches, out[3] chunks
 * of the scan, out[4] runs of its last chunk, out[5] 1 = the locus is prepared on the device (presence bitmap), 0 = the call takes the host's
 * preparation, out[6] words of the bitmap (0 on the host path), out[7] 1 = the initial allele frequencies are evaluated on the device (0:
 * "too many distinct allele sizes" awaits on the host); then the compiled limits: out[8] HS_EMI_THREADS, out[9] HS_EMI_WAVE, out[10]
 * HS_EMI_SCAN_CHUNK, out[11] HS_EMI_SPAN_LIMIT.  Used by tests/test_em_input_plan.py. */
int hipstr_debug_em_input_plan(int64_t n_runs, int64_t run_reads, int64_t lo, int64_t hi, int64_t n_sizes, int64_t out[12]);
/* Diagnostics: what hipstr_em_train_dev prepares before the EM loop, for the same arguments (the same refusals): the compact arrays, the
 * alleles' sizes per locus (size_off: [n_loci+1]), the reads' allele indices and the initial log allele frequencies; *route = 0 when the
 * device prepared them, 1 when the call took the host's preparation.  Per-read arrays: room for every read of the run; sizes / log_freq:
 * room for reads + loci.  Used by tests/test_em_from_traces_gpu.py. */
typedef struct hipstr_debug_em_input {
  int32_t* em_read_off; int32_t* num_bps; int32_t* sample_label; int32_t* obs; double* log_p1; double* log_p2;
  int32_t* size_off; int32_t* sizes; double* log_freq; int32_t* route;
} hipstr_debug_em_input_t;
int hipstr_debug_em_input_fetch(hipstr_post_dev_t* pd, const hipstr_em_trace_request_t* rq, const hipstr_trace_dev_t* td, hipstr_debug_em_input_t* out);

/* Diagnostics (host only): one entry {A, G, Bnd} of the tabulated closed form the STR kernel uses for a "simple" visiting
 * list (StutterAlignerClass.cpp:59-150 for a periodic block): with `bound` columns of the block in reach, a run of U0 equal
 * configurations at the block's right end and `tail` configurations in total, fast_log_sum_exp over the pushed values is
 * (lp0 + A) + G bit for bit whenever |lp0| < Bnd.  Used by tests/test_prep.py to check exactly that against the oracle. */
int hipstr_debug_simple_table(int bound, int U0, int tail, double entry[3]);

/* Diagnostics: where the calling process' host time inside the library goes.  mode 1 = reset and start, 0 = stop, anything else =
 * read only.  Fills up to `cap` entries of names / seconds (wall clock, summed over threads) / calls and returns the number of
 * buckets; names indented by two spaces are parts of the entry point above them.  Used by integration/genotype_flow.cpp --profile. */
int hipstr_debug_api_profile(int mode, int cap, const char** names, double* seconds, int64_t* calls);
/* Diagnostics: how many blocks the library has taken from the driver so far (hipMalloc / hipHostMalloc: misses of its block caches, 0.1 ms to
 * 1 s each).  A stream is in its steady state once this stops growing from pass to pass. */
int64_t hipstr_debug_driver_allocs(void);
/* Diagnostics (tests): the calling thread's device context's block caches — out[0..3] device: bytes held from the driver, bytes in free
 * blocks, blocks in use, the cap on idle bytes (HIPSTR_DEV_CACHE_GIB, default 70 % of the device's memory); out[4..7] the same for pinned
 * host memory (HIPSTR_PIN_CACHE_GIB, default 24).  A release that leaves more idle bytes than the cap gives the chunks without a block in
 * use back to the driver; when the driver refuses a new chunk a request is served from any free block that is large enough, then after
 * trimming idle chunks; only then does it fail.  out[8], out[9]: driver refusals the device cache survived by the first / the second way;
 * out[10], out[11]: the pinned cache's. */
int hipstr_debug_cache_stats(int64_t out[12]);
/* Diagnostics (tests): one block from / back to the calling thread's device block cache — what every upload does dozens of times. */
void* hipstr_debug_cache_get(int64_t bytes);
void hipstr_debug_cache_put(void* block);
/* Diagnostics (tests): the memory the calling thread's device context's block caches may hand out next — every FREE block and every chunk's not
 * yet carved tail, device (hipMemset) and pinned (memset) — filled with `byte`, after the device has gone idle; a block that is out is never
 * touched.  The caches never clear a block, so a kernel that reads a word of its workspace it did not write gets whatever the block held
 * before: after this call that is `byte` repeated, and results that change with `byte` show the read.  Returns the bytes filled (-1 on
 * error, hipstr_last_error()).  Used by tests/test_poison_gpu.py. */
int64_t hipstr_debug_cache_poison(int byte);
/* Diagnostics (tests): the correctly rounded exp (which = 0) / log (1) of hipstr_amd/csrc/cr_math.h evaluated ON THE DEVICE, element by
 * element — the functions the posterior, genotype and EM kernels use in place of the device's own exp / log so that they reproduce
 * the host libm's bits. */
int hipstr_debug_cr_math(int which, const double* x, double* y, int64_t n);
/* Diagnostics (tests): the float log-sum-exp primitives of hipstr_amd/csrc/float_lse.h — the reference's bit-trick fasterexp / fasterlog
 * (vector log-sum-exp) and fastexp / fastlog (pair log-sum-exp) — evaluated ON THE DEVICE at the `count` consecutive float bit patterns
 * from bits_lo (bits_lo + count <= 2^32, count <= 2^28): the arguments are generated on the device and only the results' bits come back.
 * which: 0 fasterexp, 1 fasterlog, 2 fastexp, 3 fastlog, 4 the pair term fastlog(1 + fastexp(p)), 5 the hand-made division
 * 27.7280233f / d (fastpow2's), 6 1.72587999f / d (fastlog's); 7 and 8 are the CONTROLS of 5 and 6: n * rcp(d) without Newton step or
 * correction, which differs from the IEEE quotient at some denominators (a sweep that never sees a difference there proves nothing).
 * hipstr_debug_fast_lse2: the double wrapper fast_log_sum_exp(a[i], b[i]) (threshold test, ordering, cast, final addition);
 * hipstr_debug_fast_lse_vec: the streaming Lse over the rows v[row_off[r] .. row_off[r+1]) (row_off[0] = 0, no empty row), both with
 * the library's LOG_THRESH.  The _host forms run the same header's host side without a device — what em.hip's host path and prep.cpp
 * run (which = 0..6).  Used by tests/test_float_lse.py and tests/test_float_lse_gpu.py. */
int hipstr_debug_float_fn(int which, uint32_t bits_lo, int64_t count, uint32_t* out_bits);
int hipstr_debug_fast_lse2(const double* a, const double* b, double* out, int64_t n);
int hipstr_debug_fast_lse_vec(const double* v, const int64_t* row_off, double* out, int64_t n_rows);
int hipstr_debug_float_fn_host(int which, uint32_t bits_lo, int64_t count, uint32_t* out_bits);
int hipstr_debug_fast_lse2_host(const double* a, const double* b, double* out, int64_t n);
int hipstr_debug_fast_lse_vec_host(const double* v, const int64_t* row_off, double* out, int64_t n_rows);
/* Diagnostics: (realigned allele, side) pairs of a batch by the STR kernel that takes them: counts[1] periodic blocks (tabulated closed form),
 * counts[2] blocks with one or two interruptions (piecewise closed form), counts[3] more interruptions (lists replayed in the grouped layout),
 * counts[0] the rest (per-read kernel). */
int hipstr_debug_allele_kinds(hipstr_dev_batch_t* dev, int64_t counts[4]);
/* Diagnostics (tests): a non-blocking HIP stream made by the library's own HIP runtime — what a caller passes as `hip_stream` — and its release. */
void* hipstr_debug_stream_create(void);
void hipstr_debug_stream_destroy(void* hip_stream);
/* Diagnostics: the device's copy of a batch's STR-option records (what = 0: hs_stropt_t of hipstr_amd/csrc/layout.h), its f64 pool incl. the
 * part the device generated (1) or the per-allele records the device assembled (2).  Returns the table's size in bytes (-1 on failure). */
int64_t hipstr_debug_fetch_table(hipstr_dev_batch_t* dev, int what, void* buf, int64_t cap_bytes);
/* Diagnostics (host only): the decisions of hipstr_amd/csrc/trace_cache_layout.h for a gather of n_out records and a cache of n_live keys,
 * n_dead dead records and n_segments segments.  out[0] workgroups of the lengths kernel, out[1] steps of 64 pieces the scan makes over a
 * one-piece pool, out[2] over the flank pool (two pieces a record), out[3] workgroups of the copy kernel, out[4] pieces of all pools,
 * out[5] 1 = hipstr_trace_cache_round compacts this cache by itself; then the compiled limits: out[6] HS_TC_COMPACT_MIN_DEAD, out[7]
 * HS_TC_MAX_SEGMENTS, out[8] HS_TC_LEN_THREADS, out[9] HS_TC_WAVE, out[10] HS_TC_TOTALS_BYTES; out[11] 1 = a pool of n_out elements fits
 * the 32-bit offsets.  Used by tests/test_trace_cache_host.py. */
int hipstr_debug_trace_cache_plan(int64_t n_out, int64_t n_live, int64_t n_dead, int64_t n_segments, int64_t out[12]);
/* Diagnostics: the calling thread's last gather (hipstr_trace_dev_gather, or the one inside hipstr_trace_cache_round / _view / _compact):
 * out[0] milliseconds of its three kernels (measured with events when HIPSTR_TRACE_GATHER_TIMING is set, else 0), out[1] bytes sent up,
 * out[2] bytes that came home, out[3] its records. */
int hipstr_debug_trace_gather_last(double out[4]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
