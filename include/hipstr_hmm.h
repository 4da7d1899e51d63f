/*
 * hipstr_hmm.h — C-ABI of the MI355X-native read-to-haplotype HMM alignment and
 * diplotype-posterior core (drop-in boundary for tfwillems/HipSTR's hot path).
 *
 * Every entry point below names the reference interface it replaces
 * (paths relative to the HipSTR v0.7 tree).  Plain pointers and sizes only; no
 * C++ or torch types cross this boundary.  The library never falls back to a
 * CPU path: if no gfx950 device can be opened every call returns non-zero and
 * hipstr_last_error() says why.
 *
 * Conventions
 *   - all log-likelihoods are natural logs, IEEE double (the reference computes
 *     in double; only its log-sum-exp approximations drop to float, and those
 *     are bit-replicated on the device)
 *   - a "locus" is one STR region = one Haplotype of exactly three HapBlocks
 *     [left flank, STR block, right flank] (the reference asserts this shape,
 *     src/SeqAlignment/Haplotype.cpp:12)
 *   - a "read" on this boundary is a pooled read (ReadPooler pool,
 *     src/read_pooler.h:13-53) — the unit HapAligner::process_reads sees
 *   - candidate haplotypes ("alleles") of a locus are indexed in the visit
 *     order of Haplotype::next() (reflected mixed-radix Gray code, block 0
 *     fastest; src/SeqAlignment/Haplotype.cpp:157-196)
 *   - return value 0 = ok; non-zero = error (the C++ adapter turns it into
 *     printErrorAndDie, src/error.cpp:5-9, to keep the reference convention)
 */
#ifndef HIPSTR_HMM_H_
#define HIPSTR_HMM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The functions declared here — and nothing else — are the library's ABI: libhipstr_hmm.so is built with -fvisibility=hidden. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define HIPSTR_NUM_BLOCKS        3   /* Haplotype.cpp:12 */
#define HIPSTR_MAX_STUTTER_REPS  6   /* RepeatStutterInfo.h:10-11 (MAX_STUTTER_REPEAT_INS / _DEL) */
#define HIPSTR_NUM_ARTIFACTS     (2 * HIPSTR_MAX_STUTTER_REPS + 1)
#define HIPSTR_MAX_HOMOP_LEN     15  /* AlignmentModel.h:6 */

/*
 * A batch of independent loci, flattened structure-of-arrays.  Host memory,
 * read-only, owned by the caller; the library copies what it needs.
 *
 * It carries exactly what the reference hands to
 *   HapAligner::HapAligner(Haplotype*, std::vector<bool>& realign_to_haplotype)   (HapAligner.h:56)
 *   HapAligner::process_reads(alignments, init_read_index, base_quality,
 *                             realign_read, aln_probs, seed_positions)           (HapAligner.h:86)
 * i.e. the HapBlock/RepeatBlock contents of the Haplotype (HapBlock.h:18-148,
 * RepeatBlock.h:26-43), the StutterModel parameters of the STR block
 * (stutter_model.h:31-60) and, per pooled read, the fields of `Alignment` the
 * path touches: sequence, base qualities, start and CIGAR (AlignmentData.h:28-137).
 *
 * Every entry point that takes a batch first checks that its tables agree with each other — counts in range, offsets non-negative
 * and never decreasing, no option longer than 65536 bases, no read longer than 1 Mi bases, CIGAR runs of positive length — and fails
 * the call with a message otherwise (where the reference would assert or index out of its vectors); what the pointers point AT cannot
 * be checked: the arrays must be as long as their offset tables say.
 */
typedef struct hipstr_batch {
  int32_t        n_loci;

  /* ---- haplotype structure ---- */
  const int32_t* blk_start;    /* [3*n_loci] HapBlock::start(), inclusive reference coordinate        */
  const int32_t* blk_end;      /* [3*n_loci] HapBlock::end(), exclusive                                */
  const int32_t* blk_nopts;    /* [3*n_loci] HapBlock::num_options() (option 0 = reference sequence)   */
  const int32_t* period;       /* [n_loci]   RepeatStutterInfo::get_period() of block 1                */
  const double*  stutter;      /* [6*n_loci] StutterModel ctor order: inframe_geom, inframe_up,
                                  inframe_down, outframe_geom, outframe_up, outframe_down
                                  (stutter_model.h:31-32); motif_len = period                         */
  const int32_t* opt_off;      /* [n_opts+1] byte offsets into seq; options are enumerated
                                  locus-major, block-major, option-minor                               */
  const char*    seq;          /* concatenated option sequences, ACGTN                                 */
  const int32_t* hap_off;      /* [n_loci+1] prefix sums of Haplotype::num_combs()                     */
  const uint8_t* realign_hap;  /* [hap_off[n_loci]] realign_to_haplotype flags, or NULL = all true     */

  /* ---- pooled reads ---- */
  const int32_t* read_off;     /* [n_loci+1] prefix sums of reads per locus                            */
  const int32_t* base_off;     /* [n_reads+1] offsets into bases/quals                                 */
  const char*    bases;        /* Alignment::get_sequence()                                            */
  const char*    quals;        /* Alignment::get_base_qualities(), Phred+33                            */
  const int32_t* read_start;   /* [n_reads] Alignment::get_start()                                     */
  const int32_t* cigar_off;    /* [n_reads+1] offsets into cigar_op/cigar_len                          */
  const char*    cigar_op;     /* CigarElement::get_type(): '=', 'X', 'I', 'D' only (HapAligner.cpp:309) */
  const int32_t* cigar_len;    /* CigarElement::get_num()                                              */
  const uint8_t* realign_read; /* [n_reads] realign_read flags, or NULL = all true                     */
} hipstr_batch_t;

/* Output layout shared by every align entry point:
 *   aln_probs[out_off[l] + i*A_l + k], i = read within locus l, k = allele, A_l = num_combs,
 *   out_off[l] = sum_{l'<l} P_l' * A_l'   — the row-major layout process_reads writes
 *   (HapAligner.cpp:324); seeds[read] = HapAligner::calc_seed_base (HapAligner.cpp:270-318). */
int hipstr_batch_out_offsets(const hipstr_batch_t* batch, int64_t* out_off /* [n_loci+1] */);

/*
 * Flat on-disk / wire form of a batch (host only): what a CPU worker that decoded and filtered the reads of a region shard
 * (the reference's read_and_filter_reads, bam_processor.cpp:173-473) hands to the process that owns a GPU.  One header, a
 * section table and the arrays of hipstr_batch_t back to back, checksummed; the reader points a hipstr_batch_t into one
 * allocation.  hipstr_batch_serialized_size returns -1 on an inconsistent batch.
 */
typedef struct hipstr_batch_file hipstr_batch_file_t;
int64_t hipstr_batch_serialized_size(const hipstr_batch_t* batch);
int  hipstr_batch_serialize(const hipstr_batch_t* batch, void* out, int64_t cap);
hipstr_batch_file_t* hipstr_batch_deserialize(const void* data, int64_t size);      /* NULL + hipstr_last_error() on a bad image */
int  hipstr_batch_write(const char* path, const hipstr_batch_t* batch);
hipstr_batch_file_t* hipstr_batch_read(const char* path);
const hipstr_batch_t* hipstr_batch_file_batch(const hipstr_batch_file_t* f);
void hipstr_batch_file_free(hipstr_batch_file_t* f);

/* Opaque device-resident batch (prepared tables + reads + output buffers in HBM). */
typedef struct hipstr_dev_batch hipstr_dev_batch_t;

/* Selects the device and builds the constant tables the reference keeps in
 * globals: INT_LOGS (mathops.cpp:13-21, precompute_integer_logs), the
 * LOG_MATCH_TO_* transition tables (AlignmentModel.cpp:20-32,
 * init_alignment_model) and BaseQuality's log tables (base_quality.h:29-38). */
int hipstr_hmm_init(int device_ordinal);
void hipstr_hmm_shutdown(void);
/* Device and pinned memory the library holds in its block caches but no object of the caller uses goes back to the driver (whole
 * chunks only: a chunk with one block still out stays).  The caches exist because a hipMalloc / hipFree next to running kernels stalls
 * for 0.1-0.9 s; a process that is done with a large stream and stays alive next to other users of the device calls this.  Returns the
 * bytes released.  (No counterpart in the reference: its matrices are new[]/delete[] per read, HapAligner.cpp:593-602.) */
int64_t hipstr_hmm_trim(void);

/* Flattens and uploads a batch.  Replaces HapAligner's constructor work
 * (reversed haplotype, StutterAlignerClass tables; HapAligner.h:56-69,
 * RepeatBlock.h:29-43) and calc_seed_base for every read. */
hipstr_dev_batch_t* hipstr_hmm_upload(const hipstr_batch_t* batch);
void hipstr_hmm_free(hipstr_dev_batch_t* dev);

/* Runs the forward HMM for every (realign_read, realign_hap) pair of the batch:
 * HapAligner::process_reads → process_read → align_seq_to_hap +
 * compute_aln_logprob (HapAligner.cpp:320-343, 573-709, 26-161, 163-231) with
 * StutterAlignerClass (StutterAlignerClass.cpp:12-162).  Asynchronous on
 * `hip_stream` (a hipStream_t, or NULL for the library's own stream). */
int hipstr_hmm_align(hipstr_dev_batch_t* dev, void* hip_stream);

/* Same, repeated `reps` times between two HIP events recorded on the stream the
 * kernels are launched on; *ms_total = elapsed milliseconds for all reps.
 * *ms_kernel (may be NULL) = time of the dominant DP kernel only. */
int hipstr_hmm_align_timed(hipstr_dev_batch_t* dev, int reps, float* ms_total, float* ms_kernel);

/* Per-pass, per-phase timing with HIP events recorded on the launch stream: after hipstr_hmm_profile(dev, 1)
 * every hipstr_hmm_align call records events at its phase boundaries; hipstr_hmm_profile_read synchronises and
 * writes, for up to `cap` passes (oldest first), four durations in ms: ms[4*i+0] leading-flank kernels,
 * [4*i+1] STR-block kernel, [4*i+2] trailing-flank kernels, [4*i+3] combine kernel; then clears the log.
 * Returns the number of passes written, or -1. */
int hipstr_hmm_profile(hipstr_dev_batch_t* dev, int enable);
int hipstr_hmm_profile_read(hipstr_dev_batch_t* dev, float* ms, int cap);

/* Number of (read x allele) HMM alignments one hipstr_hmm_align pass computes (realigned reads with a
 * seed x realigned alleles) and the ALGORITHMIC bytes of that pass (read bases+quals+len+seed,
 * per-allele haplotype bytes + homopolymer bytes + stutter pmf + run tables + block table, 8 B per output
 * log-likelihood, 4 B per seed). */
int hipstr_hmm_workload(hipstr_dev_batch_t* dev, int64_t* n_alignments, int64_t* algorithmic_bytes, int64_t* dp_cells);

/* Copies results back.  Entries whose read or allele was not realigned are left
 * untouched in the caller's buffers, as process_reads does (HapAligner.cpp:326-329,
 * 615-619); a realigned read without a seed (-1) gets 0 for EVERY allele of its row, realigned or
 * not, as in the reference (HapAligner.cpp:333-337). */
int hipstr_hmm_fetch(hipstr_dev_batch_t* dev, double* aln_probs, int32_t* seeds);

/* Device pointer to the batch's aln_probs buffer (same layout), for chaining
 * into hipstr_post_run without a host round trip.  The device buffer holds 0 where the host contract
 * says "untouched" (reads or alleles that were not realigned): chain it only for batches that realign
 * everything and whose reads are their own pools; hipstr_rm_scatter (below) expands a pooled batch's rows to its reads and merges
 * them into what earlier rounds left, on the device. */
double* hipstr_hmm_dev_aln_probs(hipstr_dev_batch_t* dev);

/* One-shot convenience = upload + align + fetch + free: the drop-in for
 * HapAligner::process_reads (HapAligner.h:86-87). */
int hipstr_hmm_process_reads(const hipstr_batch_t* batch, double* aln_probs, int32_t* seeds);
/* The same, locus by locus as far as failures go: a locus the library cannot take (an input HapAligner::process_reads would die on —
 * an invalid seed or CIGAR, HapAligner.cpp:309,316 — or one beyond the library's limits) is left out, its part of aln_probs / seeds
 * stays untouched and locus_status[l] = 1; every other locus is processed as if it had been submitted alone (status 0).  Returns 0
 * unless the call itself failed (device, memory); hipstr_last_error() holds the message of the first refused locus. */
int hipstr_hmm_process_reads_each(const hipstr_batch_t* batch, double* aln_probs, int32_t* seeds, int32_t* locus_status /* [n_loci] */);

/* The same with seeds chosen by the caller: HapAligner::process_read takes the seed base as an argument (HapAligner.h:83,
 * HapAligner.cpp:573-575) and so does trace_optimal_aln (HapAligner.h:93); process_reads is the one caller that derives it
 * with calc_seed_base.  seed_base[r] >= 1 is used as given (it must leave a base on either side, HapAligner.cpp:316),
 * -1 marks a read without a seed (row of zeros), HIPSTR_SEED_AUTO asks for calc_seed_base; seed_base == NULL = all auto. */
#define HIPSTR_SEED_AUTO (-2)
hipstr_dev_batch_t* hipstr_hmm_upload_seeded(const hipstr_batch_t* batch, const int32_t* seed_base /* [n_reads] or NULL */);
int hipstr_hmm_process_reads_seeded(const hipstr_batch_t* batch, const int32_t* seed_base, double* aln_probs, int32_t* seeds);

/*
 * Streaming form of hipstr_hmm_process_reads: the host pipeline between a caller that produces loci one region at a time — as
 * the reference's does (BamProcessor::process_regions, bam_processor.cpp:550-617 -> GenotyperBamProcessor::analyze_reads_and_phasing,
 * genotyper_bam_processor.cpp:229-243) — and kernels that want ~10^6-10^7 alignments per launch.  Submitted loci are copied, collected
 * into batches of about `batch_alignments` (reads x haplotypes), prepared on the host threads and sent while the previous batch
 * still runs on the device (`slots` batches may be in flight), and results are handed back STRICTLY IN SUBMISSION ORDER: with
 * loci submitted in region order that is the order the VCF writer needs (vcf_writer.cpp:7-36), i.e. the per-GPU ordered gather.
 * One stream per device; a stream may be fed from one thread and drained from another.
 */
typedef struct hipstr_stream hipstr_stream_t;
typedef struct hipstr_stream_opts {
  int32_t device;             /* ordinal; hipstr_stream_open initialises it like hipstr_hmm_init                              */
  int32_t slots;              /* batches in flight (prepared / running / waiting to be collected); 0 = 6                      */
  int64_t batch_alignments;   /* a pending batch is sent once it holds this many (read x haplotype) pairs; 0 = 2 Mi           */
                              /* (the pairs in flight stay within slots x min(batch_alignments, 2 Mi), two batches at least:  */
                              /*  a larger batch size does not multiply the device memory the stream holds)                   */
} hipstr_stream_opts_t;
typedef struct hipstr_stream_stats {
  int64_t batches, tickets, alignment_slots;  /* batches launched, tickets delivered, (read x haplotype) pairs submitted       */
  double  host_seconds;       /* worker thread: prepare + staging + launches, summed over batches                              */
  double  wait_seconds;       /* hipstr_stream_next: time spent waiting for a batch to land                                    */
  double  open_seconds;       /* since hipstr_stream_open                                                                      */
  /* CPU seconds (thread CPU clocks, not wall time) by role: what the stream costs the host */
  double  cpu_submit_seconds;   /* inside hipstr_stream_submit / _submit_each on the callers' threads (checks, seeds, the copy in)  */
  double  cpu_prepare_seconds;  /* workers: prepare_batch (a worker with a budget of one host thread does all of it itself)         */
  double  cpu_upload_seconds;   /* workers: packing the staging block, copies and launches queued                                   */
  double  cpu_collect_seconds;  /* inside hipstr_stream_take / _next / _collect on the callers' threads (wait + copy out)           */
} hipstr_stream_stats_t;
hipstr_stream_t* hipstr_stream_open(const hipstr_stream_opts_t* opts /* NULL = defaults on device 0 */);
/* Queues the loci of `loci` (1..n loci; arrays are copied).  Returns the submission's ticket (0, 1, 2, ...) or -1. */
int64_t hipstr_stream_submit(hipstr_stream_t* s, const hipstr_batch_t* loci);
/* Every locus of `loci` as its own submission, in order; *first_ticket = the ticket of locus 0 (the others follow consecutively). */
int hipstr_stream_submit_each(hipstr_stream_t* s, const hipstr_batch_t* loci, int64_t* first_ticket);
/* The next n_tickets submissions, in order, into back-to-back buffers; *n_out / *n_reads = doubles / seeds written. */
int hipstr_stream_collect(hipstr_stream_t* s, int64_t n_tickets, double* aln_probs, int64_t cap_probs, int32_t* seeds, int64_t cap_seeds,
                          int64_t* n_out, int64_t* n_reads);
/* Sends the pending batch now, whatever its size. */
int hipstr_stream_flush(hipstr_stream_t* s);
/* Sizes of the next submission to be delivered: n_out doubles of aln_probs, n_reads seeds.  Returns 2 when nothing is outstanding. */
int hipstr_stream_next_size(hipstr_stream_t* s, int64_t* ticket, int64_t* n_out, int64_t* n_reads);
/* Blocks until the next submission (in submission order) is done and writes its results exactly as hipstr_hmm_process_reads
 * would have for that submission alone: aln_probs / seeds laid out as hipstr_batch_out_offsets of the submitted batch, entries of
 * reads / haplotypes that were not realigned left untouched.  Returns 0, 1 on error (the submission is consumed: its batch failed),
 * 2 when nothing is outstanding, 3 when the buffers are too small for it (hipstr_stream_next_size) — the submission stays
 * outstanding and the call can be repeated with larger ones. */
int hipstr_stream_next(hipstr_stream_t* s, int64_t* ticket, double* aln_probs, int64_t cap_probs, int32_t* seeds, int64_t cap_seeds);
/* Collects ONE submission by its ticket, in any order (each ticket once): blocks until its batch has run.  For callers that keep
 * many loci in flight, one host thread per locus: SeqStutterGenotyper::genotype is a per-locus state machine (align, posteriors,
 * tracebacks, new alleles, align only those ... seq_stutter_genotyper.cpp:603-671), and the rounds of different loci share batches.
 * hipstr_stream_next(s, ...) == hipstr_stream_take(s, lowest ticket not collected yet, ...), same return codes.  A ticket whose batch
 * has not been launched yet is sent out even when all `slots` are held by batches with uncollected earlier tickets; two collectors
 * asking for the same ticket: the second is refused; hipstr_stream_close makes blocked collectors return with an error. */
int hipstr_stream_take(hipstr_stream_t* s, int64_t ticket, double* aln_probs, int64_t cap_probs, int32_t* seeds, int64_t cap_seeds);
int hipstr_stream_stats(hipstr_stream_t* s, hipstr_stream_stats_t* out);
/* Drops whatever has not been delivered and releases the stream. */
int hipstr_stream_close(hipstr_stream_t* s);

/*
 * Several GPUs from one process (STR loci are independent, the region list shards across the GPUs of a node with no
 * collective on the data path).  One hipstr_stream_t per device; submissions fill contiguous blocks of about `block_alignments`
 * (read x haplotype) pairs; a new block goes to the device that has been dealt the least estimated WORK so far (hipstr_locus_costs:
 * loci with interrupted repeats cost several times a periodic locus' pairs), ties to the lowest slot; hipstr_multi_next hands results
 * back in GLOBAL submission order.
 * devices == NULL: ordinals 0..n_devices-1.  (One process per GPU — torch.distributed / MPI launchers — needs nothing of this:
 * every process opens its own stream on its own device.)
 */
typedef struct hipstr_multi hipstr_multi_t;
hipstr_multi_t* hipstr_multi_open(int32_t n_devices, const int32_t* devices, int64_t block_alignments /* 0 = 16 Mi */, const hipstr_stream_opts_t* per_stream);
int64_t hipstr_multi_submit(hipstr_multi_t* m, const hipstr_batch_t* loci);
int hipstr_multi_flush(hipstr_multi_t* m);
int hipstr_multi_next_size(hipstr_multi_t* m, int64_t* ticket, int64_t* n_out, int64_t* n_reads);
int hipstr_multi_next(hipstr_multi_t* m, int64_t* ticket, double* aln_probs, int64_t cap_probs, int32_t* seeds, int64_t cap_seeds);
int hipstr_multi_close(hipstr_multi_t* m);
/* Estimated work dealt to every device so far (units of hipstr_locus_costs); returns the number of devices, fills at most `cap` entries. */
int hipstr_multi_dealt(hipstr_multi_t* m, double* cost_per_device, int32_t cap);
/* Work estimate per locus, in units of one (150-base read, allele) pair of a periodic repeat with 60 flank bases: reads x realigned alleles
 * x mean read length / 150 x [1.4 x flank bases / 60 + 1 + 2.4 x interruptions of the repeat per allele] — SURVEY 8(e)'s "sum of P A L H"
 * with the STR block priced by what it costs on the device.  What the region list is split by across ranks (hipstr_amd/shard.py) and
 * what hipstr_multi_submit deals blocks by.  Host-only (no device needed). */
int hipstr_locus_costs(const hipstr_batch_t* batch, double* costs /* [n_loci] */);

/*
 * Host-side ordered gather of per-worker record streams: the reference's VCF writer accepts out-of-order positions
 * only within MAX_RECORD_PAD = 50 bp (vcf_writer.h:53, vcf_writer.cpp:7-36), so the records produced by the workers of a sharded
 * region list are merged back by (chromosome index, position).  Every stream pushes its records in order and ends; a record is
 * released once it is the smallest pending one and no unfinished stream is empty.  Host only.
 * hipstr_gather_pop: 0 = record released; 2 = not yet (an unfinished stream has nothing pending); 3 = all streams ended and
 * drained; 1 = error (*bytes holds the size needed when the buffer was too small; the record stays queued).
 */
typedef struct hipstr_gather hipstr_gather_t;
hipstr_gather_t* hipstr_gather_open(int32_t n_streams);
int hipstr_gather_push(hipstr_gather_t* g, int32_t stream, int32_t chrom_index, int32_t pos, const void* record, int64_t bytes);
int hipstr_gather_end(hipstr_gather_t* g, int32_t stream);
int hipstr_gather_pop(hipstr_gather_t* g, int32_t* stream, int32_t* chrom_index, int32_t* pos, void* out, int64_t cap, int64_t* bytes);
void hipstr_gather_close(hipstr_gather_t* g);

/* HapAligner::calc_seed_base (HapAligner.cpp:270-318) for every read of a batch,
 * host only (no device needed): seeds[r] = read offset of the seed base or -1.
 * Returns non-zero on the inputs the reference dies on ("Invalid alignment
 * seed", "Unrecognized CIGAR char"). */
int hipstr_calc_seed_bases(const hipstr_batch_t* batch, int32_t* seeds);

/*
 * Diplotype posteriors: Genotyper::calc_log_sample_posteriors (genotyper.cpp:44-80)
 * with the default priors of Genotyper::init_log_sample_priors (genotyper.cpp:20-42)
 * and the MAP scan of Genotyper::get_optimal_haplotypes (genotyper.cpp:82-97),
 * batched over loci.  All arrays are host pointers unless stated.
 */
typedef struct hipstr_post_batch {
  int32_t        n_loci;
  const int32_t* n_alleles;     /* [n_loci] num_alleles_                                               */
  const int32_t* n_samples;     /* [n_loci] num_samples_                                               */
  const int32_t* read_off;      /* [n_loci+1] prefix sums of num_reads_ (un-pooled reads)              */
  const int32_t* sample_label;  /* [n_reads] sample index within the locus (genotyper.h:26)            */
  const double*  log_p1;        /* [n_reads] SNP phasing log-likelihoods (genotyper.h:25)              */
  const double*  log_p2;        /* [n_reads]                                                           */
  const int32_t* read_weight;   /* [n_reads] read_weights_ (0 for second mates; genotyper.h:44-46)     */
  const double*  log_aln_probs; /* [sum R_l*A_l] log_aln_probs_, read-major (genotyper.h:33); may be
                                   NULL when a device buffer is given to hipstr_post_run              */
  const uint8_t* haploid;       /* [n_loci] haploid_ flag, or NULL = diploid                           */
  const double*  log_prior;     /* [sum S_l*A_l^2] optional: the array a derived class's virtual
                                   init_log_sample_priors fills (genotyper.h:69; EMStutterGenotyper
                                   overrides it, em_stutter_genotyper.cpp:129-144); NULL = the default
                                   hom/het priors of genotyper.cpp:20-42                               */
} hipstr_post_batch_t;

/* log_post[post_off[l] + (s*A + a1)*A + a2]; post_off[l] = sum_{l'<l} S_l'*A_l'^2
 * sample_total_ll[samp_off[l] + s];           samp_off[l] = sum_{l'<l} S_l'
 * map_gt[2*(samp_off[l]+s) + {0,1}]                                                                     */
int hipstr_post_offsets(const hipstr_post_batch_t* pb, int64_t* post_off, int64_t* samp_off);

/* dev_log_aln_probs: optional device pointer overriding pb->log_aln_probs.
 * locus_total_ll[l] = the return value of calc_log_sample_posteriors (sum of sample totals). */
int hipstr_post_run(const hipstr_post_batch_t* pb, const double* dev_log_aln_probs,
                    double* log_post, double* sample_total_ll, int32_t* map_gt, double* locus_total_ll);

/* Resident form of the same computation (inputs uploaded once, kernel launched asynchronously on the
 * library stream or `hip_stream`, results fetched on demand) — what bench.py times. */
typedef struct hipstr_post_dev hipstr_post_dev_t;
hipstr_post_dev_t* hipstr_post_upload(const hipstr_post_batch_t* pb, const double* dev_log_aln_probs);
int  hipstr_post_launch(hipstr_post_dev_t* pd, void* hip_stream);
int  hipstr_post_fetch(hipstr_post_dev_t* pd, double* log_post, double* sample_total_ll, int32_t* map_gt, double* locus_total_ll);
void hipstr_post_free(hipstr_post_dev_t* pd);

/*
 * Genotype calls: Genotyper::extract_genotypes_and_likelihoods (genotyper.cpp:129-251) with calc_PLs (99-104) and calc_gl_diff
 * (106-127) on the resident posteriors of a hipstr_post_dev_t (after hipstr_post_launch): MAP haplotype pair -> genotype of
 * the STR block, haplotype posteriors marginalised to genotype posteriors (streaming log-sum-exp in the reference's order),
 * Q / PQ values, GL (log10, priors removed), GLDIFF, PL, PHASEDGL.  hap_to_allele maps every haplotype of a locus to its
 * variant (option of the STR block, SeqStutterGenotyper::haps_to_alleles); every variant must be hit by a haplotype.
 * Per sample the GL / PL arrays hold V(V+1)/2 values (diploid, VCF order) or V (haploid); PHASEDGL V*V or V.
 */
typedef struct hipstr_gt_request {
  const int32_t* n_variants;      /* [n_loci] V                                                                      */
  const int32_t* hap_to_allele;   /* [sum A_l]                                                                       */
  int32_t calc_gls, calc_pls, calc_phased_gls;
} hipstr_gt_request_t;
typedef struct hipstr_gt_out {
  int32_t* best_hap;              /* [2*n_samp] best_haplotypes                                                      */
  int32_t* best_gt;               /* [2*n_samp] best_gts                                                             */
  double*  log_phased_post;       /* [n_samp]                                                                        */
  double*  log_unphased_post;     /* [n_samp]                                                                        */
  double*  hap_log_phased_post;   /* [n_samp]                                                                        */
  double*  hap_log_unphased_post; /* [n_samp]                                                                        */
  double*  gl_diff;               /* [n_samp]; written when any calc_* flag is set                                    */
  double*  gls;                   /* [gl_off[n_samp]]  when calc_gls                                                  */
  int32_t* pls;                   /* [gl_off[n_samp]]  when calc_pls                                                  */
  double*  phased_gls;            /* [pgl_off[n_samp]] when calc_phased_gls                                           */
} hipstr_gt_out_t;
/* gl_off / pgl_off: [n_samp+1] starts of every sample's piece (samples in locus order, as sample_total_ll). */
int hipstr_gt_offsets(const hipstr_post_batch_t* pb, const hipstr_gt_request_t* rq, int64_t* gl_off, int64_t* pgl_off);
int hipstr_post_extract(hipstr_post_dev_t* pd, const hipstr_gt_request_t* rq, hipstr_gt_out_t* out);

/*
 * hipstr_post_extract with its outputs in the allele order of the VCF record: SeqStutterGenotyper::write_vcf_record renumbers the
 * genotypes and gathers every sample's GL / PL / PHASEDGL through reorder_alleles' maps (seq_stutter_genotyper.cpp:673-689, :1436-1481).
 * The extraction kernel runs unchanged; a permutation kernel behind it on the same stream writes the requested arrays in the new order
 * before they are fetched, so no host gather is left.  Per locus new_to_old is a permutation of [0, V) with new_to_old[0] == 0 (the
 * reference allele stays first) and old_to_new its inverse.  Against hipstr_post_extract's outputs (same request):
 *   best_gt            old_to_new[best_gt]; -1 stays
 *   gls, pls diploid   entry i(i+1)/2 + j, j <= i, = the old entry b(b+1)/2 + a with a = min(new_to_old[i], new_to_old[j]), b = their max (:1450-1470)
 *   gls, pls haploid   entry i = the old entry new_to_old[i]                                                                (:1436-1447)
 *   phased_gls         entry i*V + j = the old entry new_to_old[i]*V + new_to_old[j]; haploid: entry i = old new_to_old[i]   (:1472-1481)
 * Every double is a copy: its bits are hipstr_post_extract's.  best_hap and the per-sample posteriors and gl_diff do not depend on the
 * order.  With allele_bp_diff / allele_count (block-option order; hipstr_record_fields' allele_count) the same call returns them in the new
 * order: bp_diffs[i] = allele_bp_diff[new_to_old[i]] (BPDIFFS: the entries i >= 1, :1047-1050) and ac[i] = allele_count[new_to_old[i]]
 * (AC: i >= 1; REFAC = ac[0] = allele_count[0], :1261-1266).  An identity order reproduces hipstr_post_extract byte for byte.
 * Refused, nothing written: what hipstr_post_extract refuses, a null order, new_to_old[0] != 0, a new_to_old that is no permutation or
 * an old_to_new that is not its inverse, allele_bp_diff without bp_diffs, allele_count without ac.
 */
typedef struct hipstr_gt_vcf_order {
  const int32_t* new_to_old;      /* [sum V_l]                                                                        */
  const int32_t* old_to_new;      /* [sum V_l]                                                                        */
  const int32_t* allele_bp_diff;  /* [sum V_l] block-option order, or NULL                                            */
  const int32_t* allele_count;    /* [sum V_l] block-option order, or NULL                                            */
  int32_t*       bp_diffs;        /* [sum V_l] out, with allele_bp_diff                                               */
  int32_t*       ac;              /* [sum V_l] out, with allele_count                                                 */
} hipstr_gt_vcf_order_t;
int hipstr_post_extract_vcf(hipstr_post_dev_t* pd, const hipstr_gt_request_t* rq, const hipstr_gt_vcf_order_t* order, hipstr_gt_out_t* out);

/*
 * De novo stutter model: EMStutterGenotyper::train (em_stutter_genotyper.cpp:146-226) with its E-step
 * (calc_hap_aln_probs :146-150, Genotyper::calc_log_sample_posteriors under the allele-frequency priors of :129-144,
 * recalc_log_read_phase_posteriors :152-169) and M-step (recalc_log_gt_priors :22-57, recalc_stutter_model :64-127), batched
 * over loci.  A read is its observed STR size (bp difference from the reference); the alleles of a locus are the distinct
 * sizes, the reference size first and the rest ascending (em_stutter_genotyper.h:55-78).  Reads of a locus are grouped by
 * ascending sample, as in hipstr_post_batch_t.
 */
typedef struct hipstr_em_batch {
  int32_t        n_loci;
  const int32_t* period;        /* [n_loci] motif length                                                          */
  const uint8_t* haploid;       /* [n_loci] or NULL = diploid                                                     */
  const int32_t* n_samples;     /* [n_loci]                                                                       */
  const int32_t* read_off;      /* [n_loci+1]                                                                     */
  const int32_t* sample_label;  /* [n_reads]                                                                      */
  const int32_t* num_bps;       /* [n_reads] observed STR size of the read                                        */
  const double*  log_p1;        /* [n_reads]                                                                      */
  const double*  log_p2;        /* [n_reads]                                                                      */
  int32_t        ref_allele;    /* size of the reference allele (0 at both call sites of the reference)           */
  int32_t        max_iter;      /* MAX_EM_ITER = 100 (genotyper_bam_processor.h:106)                              */
  double         min_ll_abs_change;   /* ABS_LL_CONVERGE = 0.01                                                   */
  double         min_ll_frac_change;  /* FRAC_LL_CONVERGE = 0.001                                                 */
} hipstr_em_batch_t;
/* trained[l]   = the return value of train();
 * stutter[6*l] = inframe geom, up, down, outframe geom, up, down of get_stutter_model() after train();
 * n_iter[l]    = E-steps performed;  final_ll[l] = the last E-step's total log-likelihood.
 * Refused (non-zero return, hipstr_last_error(); nothing is launched): a period outside 1..9, a locus without samples, reads not grouped by
 * ascending sample label, 9998 or more distinct sizes at a locus, and a locus two of whose allele sizes (the observed sizes and ref_allele,
 * observed or not) lie so far apart that their effective difference — d / period for a difference d in frame, d - d / period (truncating)
 * out of frame — reaches the 10 000 entries of the table of integer logarithms: the reference indexes INT_LOGS[10000] with it
 * (mathops.cpp:13-21) and has no answer there either. */
int hipstr_em_train(const hipstr_em_batch_t* eb, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll);

/*
 * Needleman-Wunsch with affine gaps: NeedlemanWunsch::Align (NeedlemanWunsch.cpp:370-420: initMatrices 326-367, nw_helper 195-245,
 * findOptimalStop 142-171 / findOptimalStopEndPenalty 173-193, traceAlignment 247-324) for a batch of (reference, read) pairs —
 * the step before the HMM: realign() aligns every unique read to its reference window (AlignmentOps.cpp:14-26,
 * genotyper_bam_processor.cpp:68) and Haplotype::aln_haps_to_ref aligns every haplotype to the reference haplotype with the
 * end penalty (Haplotype.cpp:58-86).  Scores are float sums of 2, -2, -5 and -0.125, exact in any order; ties are broken as
 * bestIndex does (NeedlemanWunsch.cpp:120-140).  Limits: second sequence <= 1536 bases, reference <= 4095.
 */
typedef struct hipstr_nw_batch {
  int32_t        n_pairs;
  const int32_t* ref_off;        /* [n_pairs+1] into ref_seqs                                                        */
  const char*    ref_seqs;
  const int32_t* read_off;       /* [n_pairs+1] into read_seqs                                                       */
  const char*    read_seqs;
  int32_t        use_ref_end_penalty;
} hipstr_nw_batch_t;
typedef struct hipstr_nw_out {
  float*   score;                /* [n_pairs]                                                                         */
  uint8_t* ok;                   /* [n_pairs] the return value of Align                                               */
  int64_t* aln_off;              /* [n_pairs+1]: ref_seq_al / read_seq_al of pair i occupy [aln_off[i], aln_off[i+1])  */
  char*    ref_al;
  char*    read_al;
  int64_t* cigar_off;            /* [n_pairs+1]                                                                       */
  char*    cigar_op;             /* '=', 'X', 'I', 'D'                                                                */
  int32_t* cigar_len;
  int64_t  cap_aln, cap_cigar;   /* capacities of the pools                                                           */
} hipstr_nw_out_t;
int hipstr_nw_align(const hipstr_nw_batch_t* nb, hipstr_nw_out_t* out);

/* Haplotype::get_aln_info() of every haplotype of every locus (Haplotype::aln_haps_to_ref, Haplotype.cpp:58-86): Needleman-Wunsch
 * of the haplotype against the reference haplotype (all-first-options) with the end penalty, indels in the leading flank pushed
 * into the repeat (adjust_indels, Haplotype.cpp:8-56), then one of 'M','I','D' per alignment column.  The NUL-terminated string
 * of haplotype k of locus l starts at out + offs[hap_off[l] + k]; offs has hap_off[n_loci] + 1 entries.  This is the hap_to_ref
 * input of hipstr_hmm_trace.  Limits: hipstr_nw_align's — a haplotype of at most 1536 bases, a reference haplotype of at most 4095 (a locus beyond
 * them makes the call fail with that message: 1 + hipstr_last_error()). */
int hipstr_hap_aln_info(const hipstr_batch_t* batch, char* out, int64_t out_cap, int64_t* offs);

/*
 * Viterbi traceback: HapAligner::trace_optimal_aln (HapAligner.cpp:711-722) = process_read(..., retrace_aln=true) on one
 * fixed haplotype: full M/I/D matrices of both sides, arg-max seed position (compute_aln_logprob's max_index,
 * HapAligner.cpp:184-222), HapAligner::retrace (HapAligner.cpp:363-571) with its 0.001-nat tie tolerances, and — when the
 * caller supplies the haplotype-to-reference alignment strings (Haplotype::get_aln_info) — stitch_alignment_trace
 * (AlignmentTraceback.cpp:55-144).  One request = (read, allele): req_read indexes the reads of the whole batch (which fixes
 * the locus), req_allele the haplotypes of that locus; the read must have a seed.  Requests of many loci go in one call —
 * that is what fills the device (one locus alone offers only ~2 wavefronts per request).
 * Everything an AlignmentTrace holds (AlignmentTraceback.h:10-108) comes back flattened; all arrays are caller-allocated,
 * string pools are filled back to back with *_off[] giving the start of each request's piece ([n_req+1] entries).
 */
#define HIPSTR_NO_STR_DATA (-100000)     /* str_data_[block] == NULL: the alignment never entered the STR block */
typedef struct hipstr_trace_out {
  double*  ll;             /* [n_req] log-likelihood of the traced alignment (== the forward score)                  */
  int32_t* max_index;      /* [n_req] haplotype position aligned with the seed base                                   */
  int32_t* hap_aln_off;    /* [n_req+1] */
  char*    hap_aln;        /* AlignmentTrace::hap_aln(): read-vs-haplotype operations 'M','I','D','S'                 */
  int32_t* stutter_size;   /* [n_req] AlignmentTrace::stutter_size(1) or HIPSTR_NO_STR_DATA                            */
  int32_t* str_seq_off;    /* [n_req+1] */
  char*    str_seq;        /* AlignmentTrace::str_seq(1)                                                              */
  int32_t* flank_seq_off;  /* [2*n_req+1]: left flank (block 0) then right flank (block 2) of each request            */
  char*    flank_seq;      /* AlignmentTrace::flank_seq(block)                                                        */
  int32_t* flank_ins;      /* [n_req] flank_ins_size()                                                                */
  int32_t* flank_del;      /* [n_req] flank_del_size()                                                                */
  int32_t* indel_off;      /* [n_req+1] */
  int32_t* indel_pos;      /* flank_indel_data(): (position, size) pairs in the order retrace records them             */
  int32_t* indel_size;
  int32_t* snp_off;        /* [n_req+1] */
  int32_t* snp_pos;        /* flank_snp_data(): (position, base)                                                       */
  char*    snp_base;
  /* stitched alignment against the reference (only when hap_to_ref is given) */
  int32_t* aln_start;      /* [n_req] traced_aln().get_start()                                                        */
  int32_t* aln_stop;       /* [n_req] traced_aln().get_stop()                                                         */
  int32_t* cigar_off;      /* [n_req+1] */
  char*    cigar_op;       /* traced_aln().get_cigar_list()                                                           */
  int32_t* cigar_len;
  int32_t* aln_str_off;    /* [n_req+1] */
  char*    aln_str;        /* traced_aln().get_alignment()                                                            */
  int32_t  cap_chars;      /* capacity of every char pool / pair pool above (per pool)                                */
} hipstr_trace_out_t;

/* hap_to_ref: NULL, or for every haplotype of every locus the NUL-terminated Haplotype::get_aln_info() string ('M','I','D' of
 * the haplotype against the reference haplotype): hap_to_ref[hap_off[locus] + k], [hap_off[n_loci]] pointers. */
int hipstr_hmm_trace(const hipstr_batch_t* batch, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                     const char* const* hap_to_ref, hipstr_trace_out_t* out);
/* req_seed: the seed_base argument of trace_optimal_aln per request (HapAligner.h:93), or NULL / HIPSTR_SEED_AUTO entries to
 * have it computed with calc_seed_base as process_reads does. */
int hipstr_hmm_trace_seeded(const hipstr_batch_t* batch, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                            const int32_t* req_seed, const char* const* hap_to_ref, hipstr_trace_out_t* out);
/* hipstr_hmm_trace_seeded with a choice of where the records are assembled.  flags == 0: exactly hipstr_hmm_trace_seeded — the device
 * decides every move, host threads replay the operation strings into the fields above.  HIPSTR_TRACE_ASSEMBLE_DEVICE: the bookkeeping half
 * of HapAligner::retrace (HapAligner.cpp:363-571, 642-707: flank and STR sequences, SNPs, indel records, flank_ins / flank_del, hap_aln) and
 * stitch_alignment_trace (AlignmentTraceback.cpp:7-52, 55-144: seed position, the two stitch passes, leading 'I' -> 'S', start / stop, the
 * run-length CIGAR, the alignment string) run on the device as well, one wavefront per request; per chunk the host reads the pools' totals,
 * checks them against cap_chars and copies every pool and every offset / scalar array once into the caller's buffers.  Output, return
 * values and messages are those of flags == 0, byte for byte.  Any other flag bit is refused. */
#define HIPSTR_TRACE_ASSEMBLE_DEVICE 1u
int hipstr_hmm_trace_ex(const hipstr_batch_t* batch, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                        const int32_t* req_seed /* or NULL */, const char* const* hap_to_ref /* or NULL */,
                        uint32_t flags, hipstr_trace_out_t* out);

/*
 * The resident form of a device-assembled traceback call: the records stay on the device, and the two consumers that need a few of their
 * fields between the rounds of SeqStutterGenotyper::genotype() — the allele census and the read counts of a record — read them where they
 * lie (hipstr_post_census_dev, hipstr_assign_trace_stats_dev below).  What a caller still wants on the host it fetches by group.
 * A handle holds the arrays of hipstr_trace_out_t in ONE block of its context's device cache (no allocation in steady state): ll,
 * max_index, the five scalars, the seven offset arrays with their leading 0 and the ten pool arrays, dense.  It belongs to the device
 * (context) of the thread that created it, is read-only once created — several consumer calls may use it, also at once — and must not be
 * freed while one runs.
 */
typedef struct hipstr_trace_dev hipstr_trace_dev_t;

/* hipstr_hmm_trace_ex(..., HIPSTR_TRACE_ASSEMBLE_DEVICE, ...) whose records stay on the device.  flags: 0 (any bit is refused).
 * On success *td holds n_req records (n_req == 0: a valid empty handle); it is complete when the call returns.  On any failure *td = NULL,
 * nothing stays allocated, return value and hipstr_last_error() are those hipstr_hmm_trace_ex gives the same request list (cap_chars does
 * not exist here: the offsets are 32-bit, a pool of more than INT32_MAX elements is "too many requests for one call").  Per chunk of
 * requests only the 64-byte block of pool totals comes to the host; a call of one chunk keeps that chunk's arrays as they are, a call of
 * several joins them device-to-device after the last one. */
int  hipstr_hmm_trace_resident(const hipstr_batch_t* batch, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                               const int32_t* req_seed /* or NULL */, const char* const* hap_to_ref /* or NULL */,
                               uint32_t flags, hipstr_trace_dev_t** td);
/* n_req and the elements of the seven pools, in hipstr_trace_out_t's order: hap_aln, str_seq, flank_seq, indel, snp, cigar, aln_str.
 * Host only once the handle exists: what a caller sizes its buffers with. */
int  hipstr_trace_dev_sizes(const hipstr_trace_dev_t* td, int32_t* n_req, int64_t totals[7]);
/* Copies the chosen groups into out (one device-to-host copy per array through a pinned block); arrays of groups not chosen are neither
 * read nor written and may be NULL.  A chosen pool larger than out->cap_chars: non-zero, "hipstr_trace_out_t pools are too small
 * (cap_chars)", nothing written.  All groups chosen == the bytes hipstr_hmm_trace_ex writes for the same requests.  Refused: an unknown
 * bit, a chosen array that is NULL, a group the handle does not hold (hipstr_debug_trace_dev_from_host). */
#define HIPSTR_TRACE_F_SCALARS 0x01u   /* ll, max_index, stutter_size, flank_ins, flank_del, aln_start, aln_stop */
#define HIPSTR_TRACE_F_HAP_ALN 0x02u
#define HIPSTR_TRACE_F_STR_SEQ 0x04u
#define HIPSTR_TRACE_F_FLANKS  0x08u   /* flank_seq: what assemble_flanks reads */
#define HIPSTR_TRACE_F_INDELS  0x10u
#define HIPSTR_TRACE_F_SNPS    0x20u
#define HIPSTR_TRACE_F_STITCH  0x40u   /* cigar_*, aln_str (+ their offsets) */
#define HIPSTR_TRACE_F_ALL     0x7fu
int  hipstr_trace_dev_fetch(hipstr_trace_dev_t* td, uint32_t fields, hipstr_trace_out_t* out);
void hipstr_trace_dev_free(hipstr_trace_dev_t* td);

/* A ragged gather of resident records: a NEW handle whose record q is record out_idx[q] of src[out_src[q]] — any selection, any order,
 * repeats allowed.  The result has the layout of every hipstr_trace_dev_t and every consumer reads it unchanged (hipstr_trace_dev_fetch /
 * _sizes, hipstr_post_census_dev, hipstr_assign_trace_stats_dev, hipstr_em_train_dev, hipstr_flank_assemble_dev); its offsets ascend by
 * construction.  Three kernels on the calling thread's stream (lengths from the sources' offsets, a scan per pool, a wavefront per record
 * that copies its pieces); out_src / out_idx and a pointer table of the sources go up, the 64-byte block of pool totals comes down.  No
 * source is modified; the result is complete when the call returns, the caller frees it.  n_out == 0: a valid empty handle.
 * Refused (non-zero, hipstr_last_error(), *td = NULL, nothing written): a negative count, a NULL source, sources of different devices
 * (contexts), a source that lacks a group or was made by hipstr_debug_trace_dev_from_host, out_src / out_idx out of range, a pool of more
 * than INT32_MAX elements ("too many requests for one call; split the request list"). */
int  hipstr_trace_dev_gather(int32_t n_src, const hipstr_trace_dev_t* const* src, int32_t n_out, const int32_t* out_src, const int32_t* out_idx,
                             hipstr_trace_dev_t** td);

/*
 * The trace cache of a batch of loci: trace_cache_ of SeqStutterGenotyper (seq_stutter_genotyper.cpp:805-841), which outlives the rounds
 * of genotype() — a (pool, haplotype) pair is traced once, the first time a round asks for it, and add_and_remove_alleles re-keys the
 * cache through allele_mapping (:401-409).  The keys — (locus, pool within the locus, haplotype) — live in a host table; the records
 * stay on the device, in the segment the round that traced them left (one hipstr_hmm_trace_resident handle per round that missed).
 * A cache belongs to the device (context) of the thread that creates it and makes its first round (creation itself is host only) and is
 * used by one thread at a time; different caches on different threads are independent.
 */
typedef struct hipstr_trace_cache hipstr_trace_cache_t;
typedef struct hipstr_trace_cache_stats {
  int64_t n_hits;        /* requests of the round whose key the cache (or an earlier request of the same round) held */
  int64_t n_misses;      /* requests the round traced: its distinct new keys                                         */
  int64_t n_inserted;    /* of those, the keys the cache took (locus_takes)                                          */
  int64_t n_segments;    /* segments the cache holds after the call                                                  */
  int64_t n_live;        /* keys                                                                                     */
  int64_t n_dead;        /* records of the segments no key names (any more)                                          */
} hipstr_trace_cache_stats_t;
/* pool_off: [n_loci+1] prefix sums of the POOLED reads (== the pooled batch's read_off); n_alleles: [n_loci] haplotypes per locus.
 * Host only.  Refused (NULL + hipstr_last_error()): a negative count, pool_off that does not ascend from 0, an allele count below 1. */
hipstr_trace_cache_t* hipstr_trace_cache_create(int32_t n_loci, const int32_t* pool_off, const int32_t* n_alleles);
/* retrace_alignments for the batch: the requests (hipstr_post_assign(HIPSTR_ASSIGN_RETRACE)'s list: req_read a pooled read, req_allele a
 * haplotype of its locus) are split into hits and misses by key; the misses — if any — are traced with ONE hipstr_hmm_trace_resident call
 * on the compacted list (same pooled batch, same hap_to_ref, the misses' req_seed entries); *td receives one handle with a record for every
 * request in request order (hipstr_trace_dev_gather; the caller frees it).  A hit is the record of the round that first asked for the key,
 * as in the reference.  The cache keeps the new records of the loci with locus_takes[l] != 0 (NULL: all) — a locus that is done in
 * genotype() still gets its records for the round, but its cache does not take them.  stats (or NULL): the counts above.  The call
 * compacts the cache by itself when trace_cache_layout.h's rule says so (more than half of at least 4096 records dead, or more than 16
 * segments).
 * When the trace of the misses fails the cache is unchanged, *td = NULL, and return value and message are hipstr_hmm_trace_resident's for
 * the full list (a hit cannot be refused, so the first refused miss is the first refused request).  Refused before anything is traced:
 * NULL arguments, pooled->n_loci or pooled->read_off that differ from the cache's pool_off, a req_read outside the pooled reads, requests
 * not grouped by locus in locus order, a req_allele outside the locus' current haplotype count. */
int  hipstr_trace_cache_round(hipstr_trace_cache_t* tc, const hipstr_batch_t* pooled, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                              const int32_t* req_seed /* or NULL */, const char* const* hap_to_ref /* or NULL */,
                              const uint8_t* locus_takes /* [n_loci] or NULL = all */, hipstr_trace_dev_t** td, hipstr_trace_cache_stats_t* stats /* or NULL */);
/* seq_stutter_genotyper.cpp:401-409 with hipstr_rm_remap's arguments: every key's haplotype goes through allele_mapping ([sum of the OLD
 * A_l]); a key mapped to -1 is dropped and its record becomes dead.  Host only.  Refused (nothing changes): what hipstr_rm_remap refuses —
 * a count below 1, a mapping entry outside [-1, new A_l), two old haplotypes mapped to one new one. */
int  hipstr_trace_cache_remap(hipstr_trace_cache_t* tc, const int32_t* new_n_alleles, const int32_t* allele_mapping);
/* trace_cache_.clear() (:1579) for the loci with locus[l] != 0 (NULL: all).  The segments go back once no key is left. */
int  hipstr_trace_cache_clear(hipstr_trace_cache_t* tc, const uint8_t* locus /* [n_loci] or NULL = all */);
/* One gather of the live records, in the order of hipstr_trace_cache_entries, into a single segment: n_dead = 0, n_segments = 1 (0 for
 * an empty cache).  Changes no record and no later round's result. */
int  hipstr_trace_cache_compact(hipstr_trace_cache_t* tc);
/* The keys, sorted by (locus, pool, haplotype): ent_read[i] the pooled read (pool_off[locus] + pool), ent_allele[i] the haplotype; *n
 * their number.  Returns 3 (and *n) when cap is too small.  Host only. */
int  hipstr_trace_cache_entries(const hipstr_trace_cache_t* tc, int32_t cap, int32_t* n, int32_t* ent_read, int32_t* ent_allele);
/* The entries' records in that order as a new handle (the caller frees it): what the reference's final trace_cache_ holds. */
int  hipstr_trace_cache_view(hipstr_trace_cache_t* tc, hipstr_trace_dev_t** td);
/* n_segments, n_live and n_dead as they are now (the round's counts are 0).  Host only. */
int  hipstr_trace_cache_stats(const hipstr_trace_cache_t* tc, hipstr_trace_cache_stats_t* stats);
void hipstr_trace_cache_free(hipstr_trace_cache_t* tc);

/*
 * Reads assigned to the MAP haplotypes and the per-sample read counts of a VCF record: the loop over the reads of
 * SeqStutterGenotyper::write_vcf_record (seq_stutter_genotyper.cpp:1079-1157) with the phase totals of :1355-1356, and the pick of
 * retrace_alignments (:805-841), on a resident hipstr_post_dev_t after hipstr_post_launch — the likelihood matrix is read where it
 * lies (host array or device pointer given at upload), never fetched.  Per read, against its sample's MAP pair (hap_a, hap_b) = map_gt
 * (== best_hap of hipstr_post_extract) and its row LL of log_aln_probs, every quantity in the reference's operation order:
 *   log_phase_one = (LOG_ONE_HALF + log_p1) + LL[hap_a] - log_sum_exp((LOG_ONE_HALF + log_p1) + LL[hap_a], (LOG_ONE_HALF + log_p2) + LL[hap_b])
 *                   (:1090-1091; the exact pair log-sum-exp of mathops.cpp:52-57 with correctly rounded exp / log)
 *   read_strand   = 1 only if the locus is not haploid, hap_a != hap_b or |log_p1 - log_p2| > 1e-10, and with v1 = log_p1 + LL[hap_a],
 *                   v2 = log_p2 + LL[hap_b]: |v1 - v2| > strand_tolerance and !(v1 > v2)   (:1095-1099); uniq_* / rv_uniq_* count the
 *                   reads inside that tolerance branch by strand (:1100-1107)
 *   best_hap      = HIPSTR_ASSIGN_VCF: read_strand == 0 ? hap_a : hap_b (:1113); HIPSTR_ASSIGN_RETRACE: the first argument of the pair
 *                   log-sum-exp greater than the second ? hap_a : hap_b (:825).  The rule changes nothing else.
 *   phase1_reads  = exp(log_sum_exp(log_phase_one of the sample's reads that were not skipped)) — mathops.cpp:64-70: the maximum, then the
 *                   exponentials added IN READ ORDER — or 0 without such reads; phase2_reads = n_aligned - phase1_reads   (:1355-1356)
 * A read with seed < 0 is skipped (:1080) and counts nowhere; so are the reads of a sample without a MAP pair (map_gt -1).
 * Request list (with pool_index): request k is the k-th distinct (locus, pool_index, best_hap) met when the reads are walked in index
 * order — the order trace_cache_ fills in (:1115-1122, :828-835) — as (req_read, req_allele) for hipstr_hmm_trace on the pooled batch;
 * read_req[r] names the request of read r.  Returns 3 with *n_req set (nothing else promised) when n_req > cap_req, as hipstr_stream_next
 * does for buffers that are too small.  Without pool_index the request outputs are left untouched.
 * Device and pinned blocks come from the context's caches: no allocation in steady state.  The AB and FS p-values (cephes bdtr, htslib's
 * kt_fisher_exact), the sample filters and the INFO totals are computed from the counts returned here by hipstr_record_fields (below).
 */
#define HIPSTR_ASSIGN_VCF     0   /* write_vcf_record's rule, seq_stutter_genotyper.cpp:1094-1113 */
#define HIPSTR_ASSIGN_RETRACE 1   /* retrace_alignments' rule, :823-825 */
typedef struct hipstr_assign_request {
  const int32_t* seed;        /* [n_reads] seed_positions_ of the un-pooled reads; < 0 = read skipped (:1080) */
  const uint8_t* reverse;     /* [n_reads] Alignment::is_from_reverse_strand(), or NULL = none */
  const int32_t* pool_index;  /* [n_reads] pool of the read within its locus (pool_index_), or NULL = no request list */
  const int32_t* pool_off;    /* [n_loci+1] = hipstr_batch_t::read_off of the pooled batch; needed with pool_index */
  int32_t rule;
  double  strand_tolerance;   /* STRAND_TOLERANCE; 0 = the reference's 0.1 (seq_stutter_genotyper.h:157) */
} hipstr_assign_request_t;
typedef struct hipstr_assign_out {
  /* per read */
  int32_t* best_hap;          /* [n_reads] haplotype to trace on, -1 for a skipped read */
  int32_t* read_strand;       /* [n_reads] 0 / 1 (:1095-1099), -1 for a skipped read */
  double*  log_phase_one;     /* [n_reads] :1090-1091; untouched for skipped reads */
  /* per sample, sample_total_ll's order */
  int32_t* n_aligned, *n_snp, *n_strand_one, *n_strand_two;          /* :1135-1144 */
  int32_t* uniq_one, *uniq_two, *rv_uniq_one, *rv_uniq_two;          /* :1100-1107 */
  double*  phase1_reads, *phase2_reads;                              /* :1355-1356 */
  /* trace requests: distinct (locus, pool, best_hap) in order of first occurrence by read index */
  int32_t* n_req;             /* [1] */
  int32_t* req_read;          /* [cap_req] pool_off[locus] + pool: hipstr_hmm_trace's req_read */
  int32_t* req_allele;        /* [cap_req] */
  int32_t* read_req;          /* [n_reads] request of the read, -1 for a skipped read */
  int32_t  cap_req;
} hipstr_assign_out_t;
int hipstr_post_assign(hipstr_post_dev_t* pd, const hipstr_assign_request_t* rq, hipstr_assign_out_t* out);

/* Host only (no device needed; works on a library that never opened one): the counts of the record that need the tracebacks, from
 * hipstr_hmm_trace's output for the requests of hipstr_post_assign.  Per sample (sample_total_ll's order): n_stutter = reads whose request has
 * a stutter_size that is neither HIPSTR_NO_STR_DATA nor 0 (has_stutter(), AlignmentTraceback.h:79-85; seq_stutter_genotyper.cpp:1124-1125),
 * n_flank_indel = reads whose request has flank_ins != 0 || flank_del != 0 (:1126-1127).  Per read: ml_bp[r] =
 * allele_bp_diff[hap_to_allele[best_hap[r]]] + total_stutter_size (0 without STR data, AlignmentTraceback.h:87-93) when the traced alignment
 * spans the region by 5 bp — aln_start < (region_start > 4 ? region_start - 4 : 0) and aln_stop > region_stop + 4 (:1152-1154) — else
 * HIPSTR_NO_ML_BP.  Reads without a request (read_req < 0) count nowhere.  hap_to_allele: [sum A_l] as in hipstr_gt_request_t;
 * allele_bp_diff: [sum V_l], by variant; n_variants, region_start, region_stop: [n_loci].  Only n_loci, n_alleles, n_samples, read_off and
 * sample_label of `pb` are read. */
#define HIPSTR_NO_ML_BP INT32_MIN
int hipstr_assign_trace_stats(const hipstr_post_batch_t* pb, const int32_t* read_req /* [n_reads] */, const hipstr_trace_out_t* tr,
                              const int32_t* best_hap, const int32_t* hap_to_allele /* [sum A_l] */, const int32_t* allele_bp_diff /* [sum V_l], by variant */,
                              const int32_t* n_variants, const int32_t* region_start, const int32_t* region_stop /* [n_loci] */,
                              int32_t* n_stutter, int32_t* n_flank_indel /* [n_samp] */, int32_t* ml_bp /* [n_reads] */);

/*
 * The numeric fields of a VCF record that follow from those counts: SeqStutterGenotyper::write_vcf_record's three loops over the samples
 * (seq_stutter_genotyper.cpp:1159-1187, :1238-1254, :1326-1375) with compute_allele_bias (:965-982).
 *
 * hipstr_bias_pvalues: the raw pair for n count quadruples.
 *   ab[i] = compute_allele_bias(uniq_one[i], uniq_two[i]): 1 for an empty total, 0.0 for equal counts, else
 *           log10(min(1.0, 2*bdtr(min, total, 0.5))) with cephes' bdtr (incbet: incbcf / incbd / pseries, gamma, lgam)
 *   fs[i] = log10(min(1.0, two)) of htslib's kt_fisher_exact(u1 - rv1, rv1, u2 - rv2, rv2) (:1371-1374)
 * _host (no device needed) restates both routines in the reference's operation order over the host's libm and equals the compiled reference
 * bit for bit (tests/golden/record_pvalues.npz).  The device form runs one lane per quadruple with correctly rounded exp / log / log10
 * (cr_math.h) and gamma / lgam / lgamma read from a table the host form filled; it differs from the host form only where the host's libm is
 * not correctly rounded.  A quadruple whose counts exceed the table (uniq_one + uniq_two > HIPSTR_RECORD_TABLE_READS) is computed by the host
 * form inside the same call.  Refused, nothing written: null arguments, n < 0, a negative count, rv_uniq > uniq.
 *
 * hipstr_record_fields (on a hipstr_post_dev_t after hipstr_post_launch; the MAP pairs are read where they lie) and
 * hipstr_record_fields_host (map_gt: hipstr_post_fetch's, [2*n_samp]).  gt = hap_to_allele[map_gt].  Per sample (sample_total_ll's order):
 *   status  the output loop's tests in its order (:1326-1352): HIPSTR_RECORD_NOT_REPORTED (not in sample_names: the record has no column
 *           for it), else _NO_READS (n_aligned == 0), else _MASKED (sample_masked), else _FLANK_INDEL_FRAC
 *           ((float)n_flank_indel > max_flank_indel_frac*(float)n_aligned in FLOAT arithmetic: MAX_FLANK_INDEL_FRAC is a float), else _PASS
 *   gt[2]   the genotype of the MAP pair, -1 -1 for a sample without one; written for every sample
 *   ab, dab (uniq_one + uniq_two), fs: for PASS samples of a diploid locus whose MAP HAPLOTYPES differ (:1363, :1369) as
 *           hipstr_bias_pvalues gives them (an empty total gives ab = 1); everywhere else HIPSTR_RECORD_NOT_APPLICABLE (1.01) and dab 0
 * Per locus:
 *   n_skip, n_filt, an, allele_count[V] (block-option order): :1159-1187 — not reported and n_aligned == 0 pass by, then the flank fraction
 *           counts into n_filt BEFORE the mask is looked at (a sample that is masked and over the fraction counts in NFILT), then a masked
 *           sample counts into n_skip, and what is left adds its genotype's alleles (one for a haploid locus)
 *   dp, dsnp, dstutter, dflankindel: :1238-1254 — reported samples, masked ones skipped FIRST, then those over the flank fraction; samples
 *           without reads stay in
 * Refused, nothing written: null arguments, a negative count or rv_uniq > uniq on ANY sample (not reported and masked ones included: the
 * counts are checked before the filters are looked at), a negative max_flank_indel_frac, n_variants < 1,
 * a hap_to_allele outside [0, V), map_gt outside [-1, A), a sample with reads that passes the filters and has no MAP pair, a haploid locus with a sample that adds to the allele counts and has gt[0] !=
 * gt[1] (the reference asserts), a run that was not launched.  Uploads and results go through the context's caches.
 */
#define HIPSTR_RECORD_PASS             0
#define HIPSTR_RECORD_NO_READS         1
#define HIPSTR_RECORD_MASKED           2
#define HIPSTR_RECORD_FLANK_INDEL_FRAC 3
#define HIPSTR_RECORD_NOT_REPORTED     (-1)
#define HIPSTR_RECORD_NOT_APPLICABLE   1.01
#define HIPSTR_RECORD_TABLE_READS      5000    /* the reference's MAX_TOTAL_READS default per locus (hipstr_main.cpp) */
int hipstr_bias_pvalues(int64_t n, const int32_t* uniq_one, const int32_t* uniq_two, const int32_t* rv_uniq_one, const int32_t* rv_uniq_two,
                        double* ab, double* fs);
int hipstr_bias_pvalues_host(int64_t n, const int32_t* uniq_one, const int32_t* uniq_two, const int32_t* rv_uniq_one, const int32_t* rv_uniq_two,
                             double* ab, double* fs);
typedef struct hipstr_record_request {
  const int32_t* n_variants;      /* [n_loci] V                                                              */
  const int32_t* hap_to_allele;   /* [sum A_l] as in hipstr_gt_request_t                                     */
  const uint8_t* sample_reported; /* [n_samp] the sample is in sample_names, or NULL = all                   */
  const uint8_t* sample_masked;   /* [n_samp] !call_sample_[s].empty(), or NULL = none                       */
  const int32_t* n_aligned, *n_snp, *n_stutter, *n_flank_indel;             /* [n_samp] hipstr_post_assign(HIPSTR_ASSIGN_VCF),    */
  const int32_t* uniq_one, *uniq_two, *rv_uniq_one, *rv_uniq_two;           /*          hipstr_assign_trace_stats(_dev)            */
  float max_flank_indel_frac;     /* MAX_FLANK_INDEL_FRAC; 0 = the reference's 0.15f (genotyper.cpp:343)     */
} hipstr_record_request_t;
typedef struct hipstr_record_out {
  int32_t* status;                /* [n_samp] HIPSTR_RECORD_*                                                */
  int32_t* gt;                    /* [2*n_samp]                                                              */
  double*  ab;                    /* [n_samp]                                                                */
  int32_t* dab;                   /* [n_samp]                                                                */
  double*  fs;                    /* [n_samp]                                                                */
  int32_t* n_skip, *n_filt, *an;  /* [n_loci]                                                                */
  int32_t* dp, *dsnp, *dstutter, *dflankindel;    /* [n_loci]                                                */
  int32_t* allele_count;          /* [sum V_l], block-option order                                           */
} hipstr_record_out_t;
int hipstr_record_fields(hipstr_post_dev_t* pd, const hipstr_record_request_t* rq, hipstr_record_out_t* out);
int hipstr_record_fields_host(const hipstr_post_batch_t* pb, const int32_t* map_gt, const hipstr_record_request_t* rq, hipstr_record_out_t* out);

/*
 * The alleles of a VCF record: SeqStutterGenotyper::get_alleles (seq_stutter_genotyper.cpp:691-769) and reorder_alleles (:673-689) on the
 * options of block 1 of every locus of a batch (only n_loci, blk_start, blk_end, blk_nopts, opt_off and seq are read), with the base pair
 * differences of :1047-1050 and, on request, the LFLANKS / RFLANKS option strings of :1018-1040.  chrom_seq is given as
 * hipstr_hapgen_request_t gives it: window[win_off[l] + i] = chrom_seq[region_start - 40 + i], any case, win_off[l+1] - win_off[l] bytes
 * (region_stop + 40 - (region_start - 40) in the middle of a chromosome); a position below 0 or not among those bytes is outside.  Per locus:
 *   left trim    while start + left_trim < region_start: stop at the first option with left_trim + 1 >= size or a byte other than option
 *                0's at left_trim (:703-713); right trim mirrored, every option indexed from its own end (:721-733)
 *   flanks       left_flank = upper(chrom_seq[region_start, start)) only when the trimmed start >= region_start, right_flank =
 *                upper(chrom_seq[end, region_stop)) only when the trimmed end <= region_stop (:738-739); pos = min(region_start, start)
 *   pad          only with an empty left flank, when an option i >= 1 is empty or begins with another byte than option 0 (an empty
 *                option 0 begins with 0): pos - 1, and upper(chrom_seq[pos]) in front of every allele (:745-758)
 *   outputs      pos (1-based, :766); left_trim / right_trim = the returned pair (flank lengths and the pad subtracted, :741-742, :755);
 *                the V strings left_flank + option + right_flank in block-option order at alleles[allele_off[..]]; allele_bp_diff =
 *                size - size of allele 0; new_to_old / old_to_new: allele 0 first, the rest by (length, then bytes as unsigned char)
 *                (stringops.cpp:35-39)
 * status[l]: 0; HIPSTR_ALLELES_DUPLICATE: two equal allele strings (the reference's map loses an index there: no guess is made);
 * HIPSTR_ALLELES_OUTSIDE_WINDOW: the rule would read chrom_seq outside the window or before base 0.  A failed locus has zero-length
 * outputs (its V entries of allele_off repeat, its maps and bp_diffs hold -1 / 0, pos and trims 0).  With lflank_off / rflank_off given,
 * the options of block 0 cut by, or extended with, the first left_trim bases of the reference STR option (:1020-1028), and those of block
 * 2 likewise from the other end (:1032-1040); where an assert of :1015-1016, :1023, :1035 would fire, or right_trim < 0 (the reference's
 * substr(trim) throws there), HIPSTR_ALLELES_FLANK_ASSERT is or-ed into status and the locus' flank strings are empty.
 * Room: alleles needs sum over loci of V_l * (longest option of block 1 + window length + 1) bytes at most (cap_alleles is checked against
 * what is written); lflanks / rflanks the options' bytes plus, per option, the reference STR option's length.
 * The device form (hipstr_record_alleles) runs one wavefront per locus: lanes over the options for every position's test with a
 * wave-wide AND, every option's rank by counting the options that sort before it; a locus of more than HIPSTR_ALLELES_DEVICE_OPTIONS
 * options takes the host form inside the same call, and the flank strings are cut on the host in both forms.  Equal to
 * hipstr_record_alleles_host (no device needed) byte for byte, which equals the compiled reference (tests/golden/record_alleles_*.npz).
 * Refused, nothing written: null arguments, region_stop < region_start, a block 1 without options, offsets that do not ascend, a
 * capacity that is too small.
 */
#define HIPSTR_ALLELES_DUPLICATE        1
#define HIPSTR_ALLELES_OUTSIDE_WINDOW   2
#define HIPSTR_ALLELES_FLANK_ASSERT     4
#define HIPSTR_ALLELES_DEVICE_OPTIONS 256
typedef struct hipstr_record_alleles_request {
  const int32_t* region_start;    /* [n_loci]                                                                 */
  const int32_t* region_stop;     /* [n_loci]                                                                 */
  const int32_t* win_off;         /* [n_loci+1]                                                               */
  const char*    window;
} hipstr_record_alleles_request_t;
typedef struct hipstr_record_alleles_out {
  int32_t* status;                /* [n_loci]                                                                 */
  int32_t* pos, *left_trim, *right_trim;          /* [n_loci]                                                 */
  int32_t* allele_off;            /* [sum V + 1]                                                              */
  char*    alleles;
  int64_t  cap_alleles;
  int32_t* allele_bp_diff, *old_to_new, *new_to_old;      /* [sum V]                                          */
  int32_t* lflank_off;            /* [options of the blocks 0 + 1] or NULL                                    */
  char*    lflanks;
  int64_t  cap_lflanks;
  int32_t* rflank_off;            /* [options of the blocks 2 + 1] or NULL                                    */
  char*    rflanks;
  int64_t  cap_rflanks;
} hipstr_record_alleles_out_t;
int hipstr_record_alleles(const hipstr_batch_t* batch, const hipstr_record_alleles_request_t* rq, hipstr_record_alleles_out_t* out);
int hipstr_record_alleles_host(const hipstr_batch_t* batch, const hipstr_record_alleles_request_t* rq, hipstr_record_alleles_out_t* out);

/*
 * The per-read sizes of a VCF record and their per-sample histograms: ExtractCigar (extract_indels.cpp:18-90) for every read of a batch,
 * and Genotyper::condense_read_counts (genotyper.h:50-63) for every sample — the ALLREADS and MALLREADS fields of
 * SeqStutterGenotyper::write_vcf_record (seq_stutter_genotyper.cpp:1147-1154) without their text.  ExtractCigar is also all that lies
 * between the reads and hipstr_em_train in GenotyperBamProcessor::learn_stutter_model (genotyper_bam_processor.cpp:104-139):
 * hipstr_em_batch_from_bp_diffs is that loop.  Each device form equals its _host form (no device needed) byte for byte, and the host forms
 * equal the compiled reference (tests/golden/record_reads_*.npz).
 *
 * hipstr_cigar_bp_diffs: per read r of locus l, with region_start' = region_start[l] - pad[l] and region_end' = region_stop[l] + pad[l]
 * (both call sites pad with the period), span = the summed lengths of the runs that advance the reference (M = X D):
 *   got[r] = 0 when region_start' < read_start[r] or region_end' >= read_start[r] + span                     (:39-40)
 *   first  = the last M = X run among the runs that begin before region_start', 0 when there is none (last_match_index stays 0, :43-53);
 *            got[r] = 0 when first == 0 and run 0 is not M = X                                                (:54-58)
 *   last   = the lowest M = X run among the runs that end behind region_end' (the walk from the back stops at run 0, :64-75), the last run
 *            when there is none; got[r] = 0 when last is the last run and that run is not M = X               (:76-80)
 *   bp_diff[r] = sum of the I lengths minus the D lengths of the runs first..last (0 when first > last); 0 when got[r] == 0.
 * Any SAM op letter (MIDNSHP=X) is accepted: learn_stutter_model runs on raw BAM CIGARs.  One lane per read; a read of more than
 * HIPSTR_CIGAR_DEVICE_RUNS runs is done by the host form inside the same call.
 * Refused, nothing written (the reference asserts or indexes out of a vector there): null arguments, offsets that do not ascend from 0,
 * read_start < 0, a read without CIGAR runs, a run of non-positive length, another op byte, region_end' < region_start', and a read or
 * region whose positions leave int32 (read_start plus ALL its run lengths, region_start - pad, region_stop + pad).
 *
 * hipstr_sample_histograms: for the sample layout of a posterior batch (only n_loci, n_samples, read_off and sample_label of `pb` are
 * read; reads grouped by ascending sample as hipstr_post_upload requires) and one value per read, per sample (sample_total_ll's order)
 * the distinct values other than `skip`, ascending as signed integers, with the number of reads that hold each:
 *   sample s has the pairs [pair_off[s], pair_off[s+1]) of hist_value / hist_count; a sample without values has none (the reference
 *   prints "."); pair_off[n_samp] pairs in all, never more than n_reads: hist_value and hist_count have room for n_reads.
 * ALLREADS: value = bp_diff of hipstr_cigar_bp_diffs with the reads that have !got or seed < 0 (:1080) set to a skip value no read can
 * hold (e.g. HIPSTR_NO_ML_BP); MALLREADS: value = ml_bp of hipstr_assign_trace_stats(_dev), skip = HIPSTR_NO_ML_BP.
 * One wavefront per sample sorts the sample's values in LDS and counts the run heads, one scan over the samples gives pair_off, a third
 * kernel writes the pairs; a sample of more than HIPSTR_HISTOGRAM_DEVICE_READS reads is condensed by the host form inside the same call.
 * Refused, nothing written: null arguments, a negative sample count, read_off that does not ascend from 0, a label outside the locus'
 * samples, reads not grouped by ascending label.
 *
 * hipstr_em_batch_from_bp_diffs (host only): learn_stutter_model's loop (:113-139) on hipstr_cigar_bp_diffs' output.  Per locus the reads
 * with got[r] and bp_diff[r] >= -(region_stop - region_start + 1) enter, in order, with their label and log_p1 / log_p2 (0 and 0 when
 * pb->log_p1 is NULL: no SNP information, :123-125); the walk over a locus' samples ends behind the sample during which the entered count
 * passed 10000 (MAX_INF_READS, :131-132).  too_few[l] = the entered
 * count is below min_total_reads (:135-139: the reference trains no model there; the reads stay in the batch and the caller passes by).
 * em_read_off: [n_loci+1]; the four per-read arrays have room for every read of pb.  With period, haploid, n_samples = the caller's,
 * read_off = em_read_off and ref_allele 0 they are a hipstr_em_batch_t for hipstr_em_train.  Refused as hipstr_sample_histograms refuses,
 * and: region_stop < region_start, min_total_reads < 0, pb->log_p1 without pb->log_p2.
 */
#define HIPSTR_CIGAR_DEVICE_RUNS      4096
#define HIPSTR_HISTOGRAM_DEVICE_READS 1024
typedef struct hipstr_cigar_request {
  int32_t        n_loci;
  const int32_t* read_off;        /* [n_loci+1] reads of every locus                                          */
  const int32_t* read_start;      /* [n_reads] 0-based position of the alignment (BamAlignment::Position())   */
  const int32_t* cigar_off;       /* [n_reads+1] runs of every read                                           */
  const uint8_t* cigar_op;        /* [cigar_off[n_reads]] SAM op letters                                      */
  const int32_t* cigar_len;       /* [cigar_off[n_reads]]                                                     */
  const int32_t* region_start, *region_stop, *pad;      /* [n_loci]                                           */
} hipstr_cigar_request_t;
int hipstr_cigar_bp_diffs(const hipstr_cigar_request_t* rq, uint8_t* got /*[n_reads]*/, int32_t* bp_diff /*[n_reads]*/);
int hipstr_cigar_bp_diffs_host(const hipstr_cigar_request_t* rq, uint8_t* got, int32_t* bp_diff);
int hipstr_sample_histograms(const hipstr_post_batch_t* pb, const int32_t* value /*[n_reads]*/, int32_t skip,
                             int32_t* pair_off /*[n_samp+1]*/, int32_t* hist_value, int32_t* hist_count /* each [n_reads] capacity */);
int hipstr_sample_histograms_host(const hipstr_post_batch_t* pb, const int32_t* value, int32_t skip,
                                  int32_t* pair_off, int32_t* hist_value, int32_t* hist_count);
int hipstr_em_batch_from_bp_diffs(const hipstr_post_batch_t* pb, const uint8_t* got, const int32_t* bp_diff /* [n_reads] */,
                                  const int32_t* region_start, const int32_t* region_stop /* [n_loci] */, int32_t min_total_reads,
                                  int32_t* em_read_off /*[n_loci+1]*/, int32_t* sample_label, int32_t* num_bps,
                                  double* log_p1, double* log_p2 /* each [n_reads] capacity */, uint8_t* too_few /*[n_loci]*/);

/*
 * The allele census between two rounds of SeqStutterGenotyper::genotype (seq_stutter_genotyper.cpp:603-671): what decides the next round's
 * allele set, on a resident hipstr_post_dev_t after hipstr_post_launch — the likelihood matrix is read where it lies (host array or device
 * pointer given at upload, e.g. hipstr_rm_dev_log_aln_probs), never fetched.  Two functions of the reference in one call:
 *   get_stutter_candidate_alleles (:843-879, driven by id_and_align_to_stutter_alleles :570-601) -> cand_*, new_n_haps, n_spanning, n_span_stutter
 *   get_unused_alleles (:229-315; called at :649, :658 and :207)                                 -> called, spanned
 * A read HAS A TRACE iff seed >= 0 and read_req >= 0 (traced_alns[r] != NULL); its trace SPANS block 1 iff aln_start < blk_start and
 * aln_stop > blk_end of its request, both strict (:856-857, :274-275).
 * Candidates: over the reads with a spanning trace n_spanning[s]++ for the read's sample s (:860) and, if the request's stutter_size != 0,
 *   the count of the pair (s, CONTENT of the request's str_seq) goes up by one (:858-859) — the key is the string, not the request: requests
 *   of different pools or haplotypes with equal str_seq feed one count, the same string in two samples is two counts.  A pair qualifies iff
 *   count >= min_reads and 1.0*count/n_spanning[s] >= min_frac (:869: one double division, compared as written) and block 1 does not hold the
 *   string among its options (HapBlock::contains, :870).  A locus' candidates are the qualifying strings, each once, in
 *   orderByLengthAndSequence order (stringops.cpp:35-39: by length, then bytewise; :582); the empty string is a legal key.
 * Called: for every sample that has a read with seed >= 0, is not sample_uncallable and has a MAP pair (map_gt not -1), the options of hap_a
 *   and of hap_b are marked (:293-301), for every block with a hap_to_allele.  UNLIKE THE REFERENCE (:255-256) blocks with one option are
 *   written too: their option 0 simply ends up 0 or 1.
 * Spanned (block 1 only): per read with a spanning trace whose request has stutter_size == 0: best = hap_a; if the locus is not haploid and
 *   hap_a != hap_b, with v1 = log_p1 + LL[hap_a], v2 = log_p2 + LL[hap_b] (no LOG_ONE_HALF): if fabs(v1 - v2) > 1e-10 (TOLERANCE,
 *   mathops.cpp:10) best = v1 > v2 ? hap_a : hap_b (:280-284 — a third tie rule, neither HIPSTR_ASSIGN_VCF's nor HIPSTR_ASSIGN_RETRACE's);
 *   spanned[hap_to_allele[1][best]] = 1.  Reads of a sample without a MAP pair mark nothing.
 * called / spanned are zeroed by the call for the blocks it writes and left untouched for blocks whose hap_to_allele is NULL; the caller applies
 * allele_index >= 1 and the check_* choice of :305-311, or hands the census to hipstr_alleles_step, which builds the new Haplotype and allele_mapping;
 * copy_read and the re-keying of the trace cache through allele_mapping (:401-409) stay with the caller.
 * Refused (non-zero, hipstr_last_error(); checked on the host before any launch, nothing is written): a run that was not launched, pooled->n_loci
 * that differs from the run's, hap_off that disagrees with the run's allele counts, read_req outside [-1, n_req), a read whose request belongs to
 * another locus, requests not grouped by locus in locus order (hipstr_post_assign emits them so), str_seq_off that decreases, a hap_to_allele
 * entry outside its block's options, a spanning request with stutter_size == HIPSTR_NO_STR_DATA used by a read with a seed
 * (AlignmentTrace::stutter_size asserts there).
 * Returns 3 when cap_cand or cap_chars is too small: cand_off is filled (cand_off[n_loci] = candidates needed; cap_chars = str_seq_off[n_req]
 * always suffices), nothing else is promised — hipstr_post_assign's convention.
 * Only the five trace fields, the per-read and per-request indices, hap_to_allele and block 1's option strings are uploaded; the candidates'
 * bytes are copied on the host from trace->str_seq in the order the device fixed.  Device and pinned blocks come from the context's caches: no
 * allocation in steady state.
 */
typedef struct hipstr_census_request {
  const hipstr_batch_t* pooled;     /* the round's pooled batch: only n_loci, blk_start, blk_end, blk_nopts, opt_off, seq, hap_off, read_off are read */
  const int32_t* seed;              /* [n_reads] seed_positions_ of the un-pooled reads; < 0 = traced_alns[r] == NULL */
  const int32_t* read_req;          /* [n_reads] request of the read: hipstr_post_assign(HIPSTR_ASSIGN_RETRACE)'s read_req; -1 for a skipped read */
  int32_t        n_req;
  const int32_t* req_read;          /* [n_req] as given to hipstr_hmm_trace: fixes every request's locus */
  const hipstr_trace_out_t* trace;  /* only aln_start, aln_stop, stutter_size, str_seq_off, str_seq are read (host arrays) */
  const int32_t* hap_to_allele[3];  /* per block: [sum A_l] haps_to_alleles(block) (:219-227), or NULL = this block's flags are not wanted */
  const uint8_t* sample_uncallable; /* [n_samp] !call_sample_[s].empty(), or NULL = every sample callable */
  int32_t  min_reads;               /* 0 = the reference's 2     (:869) */
  double   min_frac;                /* 0 = the reference's 0.15  (:869) */
} hipstr_census_request_t;
typedef struct hipstr_census_out {
  /* stutter candidates of block 1, per locus, unique, in orderByLengthAndSequence order */
  int32_t* cand_off;       /* [n_loci+1] */
  int32_t* cand_req;       /* [cap_cand] the lowest-numbered request of the locus whose str_seq is this candidate */
  int32_t* cand_seq_off;   /* [cap_cand+1] */
  char*    cand_seq;       /* [cap_chars] */
  int64_t* new_n_haps;     /* [n_loci] num_combs / nopts(1) * (nopts(1) + candidates)  (:583-584, integer division as written) */
  /* per sample, sample_total_ll's order */
  int32_t* n_spanning;     /* [n_samp] sample_counts (:860) */
  int32_t* n_span_stutter; /* [n_samp] spanning reads with stutter_size != 0 */
  /* per option, opt_off's enumeration (locus-major, block-major, option-minor); untouched for blocks whose hap_to_allele is NULL */
  uint8_t* called;         /* [n_opts] :293-301 */
  uint8_t* spanned;        /* [n_opts] :265-291; written for block 1 only */
  int32_t  cap_cand, cap_chars;
} hipstr_census_out_t;
int hipstr_post_census(hipstr_post_dev_t* pd, const hipstr_census_request_t* rq, hipstr_census_out_t* out);

/* hipstr_post_census with the five trace fields read from td: rq->trace must be NULL, rq->n_req must equal td's, td must live on pd's
 * device.  Same outputs, same return codes (3 included), same refusals and messages as hipstr_post_census given
 * hipstr_trace_dev_fetch(td, ALL).  The checks that need the trace's values run on the device — str_seq_off that is negative or decreases
 * (before any census kernel runs; skipped for a handle of hipstr_hmm_trace_resident, whose offsets ascend by construction) and the spanning
 * request without STR data — after every check of the host's tables; a refusal still writes nothing into out.  The candidates' bytes are
 * gathered on the device (hs_census_gather_kernel) and come home with the counts and the marks. */
int  hipstr_post_census_dev(hipstr_post_dev_t* pd, const hipstr_census_request_t* rq, const hipstr_trace_dev_t* td, hipstr_census_out_t* out);
/* hipstr_assign_trace_stats with the five scalars read from td, on td's device (one kernel: a run of reads of one sample per wavefront).
 * Same arguments otherwise, same outputs, same refusals; read_req must stay below td's n_req. */
int  hipstr_assign_trace_stats_dev(const hipstr_post_batch_t* pb, const int32_t* read_req, const hipstr_trace_dev_t* td,
                                   const int32_t* best_hap, const int32_t* hap_to_allele, const int32_t* allele_bp_diff,
                                   const int32_t* n_variants, const int32_t* region_start, const int32_t* region_stop,
                                   int32_t* n_stutter, int32_t* n_flank_indel, int32_t* ml_bp);

/*
 * The stutter model retrained from the round's tracebacks: SeqStutterGenotyper::recompute_stutter_models (seq_stutter_genotyper.cpp:1542-1581,
 * reached from genotyper_bam_processor.cpp:237-239) — the traced alignments are walked, every read whose trace spans the STR block hands
 * its observed size, log_p1 and log_p2 to its sample (:1555-1566), and EMStutterGenotyper::train runs on them (hipstr_em_train above).
 * Read r of locus l ENTERS the EM iff seed[r] >= 0, q = read_req[r] >= 0, and aln_start[q] < blk_start[3l+1] and aln_stop[q] > blk_end[3l+1],
 * both strict (:1558-1559).  An entering read has num_bps = (str_seq_off[q+1] - str_seq_off[q]) + stutter_size[q], the read's log_p1 and
 * log_p2 and its sample label; reads keep their order (grouped by ascending sample), samples and loci without an entering read stay in the
 * batch (the reference constructs str_num_bps(num_samples_)).  period comes from pooled->period, haploid and n_samples from the posterior
 * batch or run.
 * Refused (non-zero, hipstr_last_error(), no output written): null arguments, pooled->n_loci that differs from the posterior batch's,
 * req_read outside the pooled reads or not grouped by locus in locus order, read_req outside [-1, n_req), a read whose request belongs to
 * another locus, an entering read whose request has stutter_size == HIPSTR_NO_STR_DATA (AlignmentTrace::stutter_size asserts,
 * AlignmentTraceback.h:95-98; the message names the lowest such read).
 */
typedef struct hipstr_em_trace_request {
  const hipstr_batch_t* pooled;   /* the round's pooled batch: only n_loci, blk_start, blk_end, period and read_off (the locus of a request) are read */
  const int32_t* seed;            /* [n_reads] seed_positions_ of the un-pooled reads; < 0 = traced_alns[r] == NULL */
  const int32_t* read_req;        /* [n_reads] hipstr_post_assign(HIPSTR_ASSIGN_RETRACE)'s read_req; -1 = no trace */
  int32_t        n_req;
  const int32_t* req_read;        /* [n_req] as given to the traceback call: fixes every request's locus */
  int32_t        ref_allele, max_iter;              /* as hipstr_em_batch_t (0 and 100 at the reference's call site) */
  double         min_ll_abs_change, min_ll_frac_change;
} hipstr_em_trace_request_t;

typedef struct hipstr_em_trace_out {
  uint8_t* trained; double* stutter; int32_t* n_iter; double* final_ll;   /* as hipstr_em_train, [n_loci] / [6*n_loci] */
  int32_t* em_read_off;   /* [n_loci+1] reads that entered the EM, or NULL */
  int32_t* n_sizes;       /* [n_loci] allele sizes of the EM (reference size included), or NULL */
} hipstr_em_trace_out_t;

/* Host only (no device needed; works on a library that never opened one): the batch recompute_stutter_models builds, from host traces —
 * only aln_start, aln_stop, stutter_size and str_seq_off of `tr` and n_loci, n_samples, read_off, sample_label, log_p1, log_p2 of `pb` are
 * read.  em_read_off: [n_loci+1]; the four per-read arrays have room for every read of pb.  With period = pooled->period, haploid and
 * n_samples = pb's and read_off = em_read_off they are a hipstr_em_batch_t. */
int hipstr_em_batch_from_traces(const hipstr_post_batch_t* pb, const hipstr_em_trace_request_t* rq, const hipstr_trace_out_t* tr,
                                int32_t* em_read_off /*[n_loci+1]*/, int32_t* sample_label, int32_t* num_bps,
                                double* log_p1, double* log_p2 /* each [n_reads] capacity */);

/* The same reads selected, compacted and prepared where the records lie, and hipstr_em_train's loop on them: stutter_size, aln_start,
 * aln_stop and str_seq_off are read from td, log_p1, log_p2 and the (locus, sample) runs of reads from what hipstr_post_upload left on the
 * device (the run need not have been launched); only seed, read_req and per-locus tables are uploaded, and per locus and per (locus, sample)
 * a few counts come home.  Outputs, return codes and hipstr_last_error() are those of hipstr_em_train on the batch
 * hipstr_em_batch_from_traces builds from hipstr_trace_dev_fetch(td, SCALARS | STR_SEQ), bit for bit; em_read_off and n_sizes (either may
 * be NULL) are that batch's read offsets and the EM's allele counts.  Refused as hipstr_em_batch_from_traces refuses, and: rq->n_req that
 * differs from td's, td on another device than pd, a handle without the scalars or the str_seq offsets.  Every refusal but the read without
 * STR data is decided before any kernel runs; none writes into out.  A locus whose sizes span the table of integer logarithms (10 000
 * values) or more, and every batch hipstr_em_train refuses, takes the host's preparation on the fetched compact arrays.  Device and pinned
 * blocks come from the context's caches: no allocation in steady state. */
int hipstr_em_train_dev(hipstr_post_dev_t* pd, const hipstr_em_trace_request_t* rq, const hipstr_trace_dev_t* td,
                        hipstr_em_trace_out_t* out);

/*
 * The read x haplotype matrix of a batch of loci, resident on the device between the rounds of SeqStutterGenotyper::genotype
 * (seq_stutter_genotyper.cpp:603-671): log_aln_probs_ (R x A per locus, un-pooled reads; genotyper.h:33) and seed_positions_, in the layout
 * of hipstr_post_batch_t::log_aln_probs.  The forward pass writes one row per POOLED read (hipstr_hmm_align, P x A); the posteriors, the
 * genotype calls and hipstr_post_assign read one row per read.  The calls below keep the matrix where it lies: one batch can go
 *   align -> hipstr_rm_scatter -> hipstr_post_upload(pb with log_aln_probs = NULL, hipstr_rm_dev_log_aln_probs(rm)) -> launch / assign -> traces
 *   -> new alleles: hipstr_rm_remap -> align only those -> hipstr_rm_scatter -> posteriors ...
 * without the matrix leaving the device.  The layout — reads per locus, each read's pool (pool_index_, read_pooler.cpp:3-20), the second
 * mates (second_mate_, seq_stutter_genotyper.cpp:499-507) — is fixed at creation and copied; the haplotype counts change with hipstr_rm_remap.
 * Device and pinned blocks come from the context's caches: no allocation in steady state.
 */
typedef struct hipstr_read_matrix hipstr_read_matrix_t;
typedef struct hipstr_read_layout {
  int32_t        n_loci;
  const int32_t* n_alleles;    /* [n_loci]   A_l                                                              */
  const int32_t* read_off;     /* [n_loci+1] prefix sums of the un-pooled reads (== hipstr_post_batch_t)      */
  const int32_t* pool_index;   /* [n_reads]  pool of the read within its locus (pool_index_)                  */
  const uint8_t* second_mate;  /* [n_reads]  second_mate_, or NULL = none                                     */
} hipstr_read_layout_t;
/* init_ll: [sum R_l*A_l] or NULL = every entry -100000, the value the reference gives columns it has not aligned yet
 * (seq_stutter_genotyper.cpp:374); init_seeds: [n_reads] or NULL = every seed -1.  Refused (NULL + hipstr_last_error()): negative counts,
 * read_off that does not ascend from 0, a negative pool_index, second_mate set on the first read of a locus (its first mate, read i-1 of
 * :555, would belong to another locus) or on two consecutive reads — the reference produces neither. */
hipstr_read_matrix_t* hipstr_rm_create(const hipstr_read_layout_t* layout, const double* init_ll, const int32_t* init_seeds);
/* The second half of SeqStutterGenotyper::calc_hap_aln_probs (seq_stutter_genotyper.cpp:530-564) on a batch hipstr_hmm_align has run on
 * (the first half, :522-528, is upload + align).  For every read i with copy_read[i] (NULL = all): seeds[i] = the seed of its pool, and
 * M[i][j] = the pool's row for every haplotype j the batch realigned (its realign_hap; :532-543); then for every second mate i with
 * copy_read[i], rows i-1 and i both become M[i-1][j] + M[i][j] for the realigned j (:551-564) — row i-1 as it then lies: freshly copied if
 * copy_read[i-1], the resident value otherwise.  Everything else keeps its value.  A pool without a seed contributes its row of zeros
 * (HapAligner.cpp:333-337).  Asynchronous, ordered behind the batch's last pass; hipstr_post_launch / hipstr_post_assign on a run that was
 * given the matrix' pointer are ordered behind the scatter without the caller synchronising, as long as everything runs on the library's
 * own streams (a pass launched on a stream of the caller's makes this call wait for the device instead).  The caller keeps a posterior run
 * on the matrix from being launched while a scatter of ANOTHER thread is being queued.
 * Refused (non-zero + hipstr_last_error(), nothing launched): a batch that was never aligned, n_loci or a locus' n_alleles that disagrees
 * with the batch, a pool_index outside the batch's pooled reads of that locus, copy_read[i] set for a read whose pool was not realigned
 * (the reference would copy memory process_reads never wrote, :526-542). */
int  hipstr_rm_scatter(hipstr_read_matrix_t* rm, hipstr_dev_batch_t* dev, const uint8_t* copy_read /* [n_reads] or NULL = all */);
/* The column re-layout of SeqStutterGenotyper::add_and_remove_alleles (seq_stutter_genotyper.cpp:371-386), per locus: a new matrix of
 * new_n_alleles[l] columns filled with -100000, old column j copied to column allele_mapping[j] where that is >= 0 (allele_mapping:
 * [sum of the OLD A_l], locus after locus; -1 = the haplotype is gone).  Seeds are unchanged.  THE DEVICE POINTER CHANGES: a
 * hipstr_post_dev_t built on the old pointer must be freed before this call, and hipstr_rm_dev_log_aln_probs asked again after it.
 * Returns when the new matrix is complete.  Refused: a count below 1, a mapping entry outside [-1, new A_l), two old columns mapped to
 * one new column. */
int  hipstr_rm_remap(hipstr_read_matrix_t* rm, const int32_t* new_n_alleles, const int32_t* allele_mapping);
/* Device pointer of the matrix, for hipstr_post_upload / hipstr_post_run (layout of hipstr_post_batch_t::log_aln_probs). */
const double* hipstr_rm_dev_log_aln_probs(hipstr_read_matrix_t* rm);
/* Copies the matrix and / or the seeds back (either may be NULL), after everything queued on the matrix has run. */
int  hipstr_rm_fetch(hipstr_read_matrix_t* rm, double* ll /* [sum R_l*A_l] */, int32_t* seeds /* [n_reads] */);
/* Every hipstr_post_dev_t built on the matrix' pointer must have been freed. */
void hipstr_rm_free(hipstr_read_matrix_t* rm);

/*
 * ReadPooler (read_pooler.h:13-53, read_pooler.cpp:3-20) and BaseQuality::median_base_qualities (base_quality.cpp:11-28) for a batch of
 * UN-POOLED reads: what stands in front of hipstr_hmm_upload.  Only n_loci, read_off, base_off, bases and quals of the batch are read.
 * Two reads of a locus share a pool iff their sequences are equal byte for byte (length included, case not folded; reads of length 0 form
 * one pool with empty qualities); pools are numbered in order of first appearance by read index; pool_rep is that first read; the quality
 * at position i of a pool is sorted(member bytes at i)[n / 2] with bytes ordered as signed char (the upper median: n = 2 gives the larger).
 * Loci are independent; a locus without reads has 0 pools.  The arrays are sized by the input, so they always suffice; entries past
 * pool_off[n_loci] of the per-pool arrays and past pool_qual_off[pool_off[n_loci]] are left untouched.
 * hipstr_pool_reads works on the device, in chunks of whole loci under a workspace budget (HIPSTR_POOL_WS_MIB, default 512): reads are
 * grouped by a 64-bit hash and every member is then compared with its pool's first read byte for byte — a locus in which two different
 * reads share a hash, and a locus of more reads than the grouping kernel holds in LDS (4096), is pooled by the host code inside the same
 * call.  hipstr_pool_reads_host is that host code for the whole batch; it needs no device.  Both give identical bytes in every output.
 * Refused (non-zero + hipstr_last_error(), nothing written, nothing launched): NULL arguments, a NULL output array, offset tables the other
 * entry points refuse.  hipstr_pool_reads without a device fails as every device entry point does; it does not fall back to the host.
 * A HIP error while the call runs (an allocation, a copy, a launch) is non-zero + hipstr_last_error() as well, but "nothing written" holds
 * for the first chunk only: the outputs of the loci of the chunks before the failing one are written already (discard them).
 * read_off[0] is normally 0.  Where it is not, reads 0 .. read_off[0] belong to no locus: their pool_index entries are left untouched,
 * and pool_rep counts from the batch's read 0 all the same.
 */
typedef struct hipstr_pool_out {
  int32_t* pool_index;     /* [n_reads]   pool of the read within its locus: ReadPooler::add_alignment's return value            */
  int32_t* n_pools;        /* [n_loci]                                                                                           */
  int32_t* pool_off;       /* [n_loci+1]  prefix sums of n_pools                                                                  */
  int32_t* pool_rep;       /* [n_reads]   per pool (pool_off order): the read that opened it, as an index into the batch's reads  */
  int32_t* pool_size;      /* [n_reads]   per pool: members                                                                       */
  int32_t* pool_qual_off;  /* [n_reads+1] per pool: start of its qualities                                                        */
  char*    pool_quals;     /* [base_off[n_reads]] median qualities, pools back to back                                            */
} hipstr_pool_out_t;
int hipstr_pool_reads(const hipstr_batch_t* unpooled, hipstr_pool_out_t* out);        /* on the device */
int hipstr_pool_reads_host(const hipstr_batch_t* unpooled, hipstr_pool_out_t* out);   /* host only, no device needed */

/* The batch ReadPooler leaves behind, in one allocation: the haplotype arrays copied, per pool its first read's bases, start and CIGAR and
 * the pool's median qualities, realign_read = NULL — ready for hipstr_hmm_upload — and the reads' pool indices for
 * hipstr_read_layout_t::pool_index.  flags: HIPSTR_POOL_ON_HOST pools with hipstr_pool_reads_host, 0 on the device.  NULL +
 * hipstr_last_error() on a refusal or a failure.  hipstr_pooled_batch_pool_index is indexed by the un-pooled batch's read number, read 0
 * first: with read_off[0] > 0 the entries of the reads in front of the first locus are 0 and mean nothing. */
#define HIPSTR_POOL_ON_HOST 1u
typedef struct hipstr_pooled_batch hipstr_pooled_batch_t;
hipstr_pooled_batch_t* hipstr_pool_batch(const hipstr_batch_t* unpooled, uint32_t flags);
const hipstr_batch_t*  hipstr_pooled_batch_batch(const hipstr_pooled_batch_t* p);
const int32_t*         hipstr_pooled_batch_pool_index(const hipstr_pooled_batch_t* p);      /* [n_reads of the un-pooled batch] */
void hipstr_pooled_batch_free(hipstr_pooled_batch_t* p);

/*
 * The flank reassembly that closes SeqStutterGenotyper::genotype(): assemble_flanks (seq_stutter_genotyper.cpp:40-217, reached from :666-668)
 * with DebruijnGraph (debruijn_graph.cpp) and the pre-check of :618-629, batched over loci.  Per flank (0 = block 0, 1 = block 2; ref_seq =
 * option 0 of the block) and per sample, one TASK: for k from calc_kmer_length(ref_seq, min_kmer, max_k) to max_k = min(max_kmer, len - 1) the
 * graph of ref_seq (weight 2, its edges never pruned) takes the flank_seq(block) of every read of the sample that has a trace (seed >= 0 and
 * read_req >= 0, as in the census) and a non-empty string (strings of length <= k do not count), is pruned with
 * max(2, ceil(0.02 * strings)), and the first k whose graph is acyclic with a proper source and sink gives at most max_paths sink paths
 * (weight >= min_path_weight), in the reference's pop order (libstdc++'s heap order among equal weights).  The aggregation (:99-201) runs as
 * written on those records: the 0.25 depth share, FLANK_ASSEMBLY_INDEL for an alternative of another length (a later path of the same sample
 * may still set realign_sample), FLANK_ASSEMBLY_CYCLIC, the LOW_FREQUENCY_ALT_FLANK pruning, flank 1 skipping what flank 0 masked, the three
 * ways a locus fails, new options in bytewise order, and the two masks add_and_remove_alleles takes.
 *
 * Tasks are numbered 2*samp_off[l] + flank*S_l + s (samp_off: hipstr_post_offsets).  A sample with sample_masked set is skipped (its status
 * stays 0); so is every task of a flank without a k-mer length.
 * Per locus: status 0 = ok, 1 = no k-mer length for a flank (:58-59), 2 = more than max_flank_haplotypes alternatives (:158-162), 3 = more than
 * max_total_haplotypes haplotypes (:176-180); new_n_haps as :48-55, :169 compute it (integer division as written).  For a locus with
 * status != 0 only status is promised (both entry points still write the same bytes).
 * Capacities: hipstr_post_census' convention — when cap_opts, cap_opt_chars, cap_paths or cap_path_chars is too small the call returns 3,
 * opt_off is filled (opt_off[2*n_loci] = options needed) and the four cap_* fields of `out` are overwritten with what is needed; nothing else
 * is promised.  The path arrays are optional: all of task_k, task_n_paths, path_weight, path_seq_off, path_seq may be NULL (each on its own).
 * Refused (non-zero, hipstr_last_error(), decided before any launch, nothing written): null arguments, pooled->n_loci that differs from the
 * posterior batch's, read_req outside [-1, n_req), a read whose request belongs to another locus, requests not grouped by locus in locus
 * order, a pool_index outside the locus' pooled reads, a block without options, a handle without the FLANKS group, td on another device
 * than pd, rq->n_req that differs from td's.
 */
typedef struct hipstr_flank_request {
  const hipstr_batch_t* pooled;     /* the round's pooled batch: only n_loci, blk_nopts, opt_off, seq, hap_off, read_off are read */
  const int32_t* seed;              /* [n_reads] seed_positions_ of the un-pooled reads; < 0 = traced_alns[r] == NULL */
  const int32_t* read_req;          /* [n_reads] hipstr_post_assign(HIPSTR_ASSIGN_RETRACE)'s read_req; -1 = no trace */
  int32_t        n_req;
  const int32_t* req_read;          /* [n_req] as given to the traceback call: fixes every request's locus */
  const int32_t* pool_index;        /* [n_reads] pool of the read within its locus (pool_index_) */
  const uint8_t* sample_masked;     /* [n_samp] !call_sample_[s].empty() before the stage, or NULL = none */
  int32_t  min_kmer, max_kmer, min_path_weight, max_paths;       /* 0 = the reference's 10 / 15 / 2 / 10 */
  int32_t  max_total_haplotypes, max_flank_haplotypes;           /* as given (no default) */
  double   min_flank_freq;
} hipstr_flank_request_t;

#define HIPSTR_FLANK_OK 0
#define HIPSTR_FLANK_ASSEMBLY_INDEL 1
#define HIPSTR_FLANK_ASSEMBLY_CYCLIC 2
#define HIPSTR_FLANK_LOW_FREQUENCY_ALT 3
#define HIPSTR_FLANK_TASK_CYCLIC (-1)
#define HIPSTR_FLANK_TASK_SKIPPED (-2)
typedef struct hipstr_flank_out {
  int32_t* status;          /* [n_loci] */
  int64_t* new_n_haps;      /* [n_loci] */
  int32_t* opt_off;         /* [2*n_loci+1] the new options of (locus, flank), std::map order */
  int32_t* opt_seq_off;     /* [cap_opts+1] */
  char*    opt_seq;         /* [cap_opt_chars] */
  int32_t* opt_n_samples;   /* [cap_opts] samples supporting the option (haplotype_to_sample[..].size()) */
  uint8_t* sample_status;   /* [n_samp] HIPSTR_FLANK_* the stage set, 0 = unchanged */
  uint8_t* realign_sample;  /* [n_samp] */
  uint8_t* realign_pool;    /* [pooled reads] realign_pools (:185-191), pooled->read_off's numbering */
  uint8_t* copy_read;       /* [n_reads] copy_reads */
  int32_t* task_k;          /* [2*n_samp] accepted k, HIPSTR_FLANK_TASK_CYCLIC or _SKIPPED; or NULL */
  int32_t* task_n_paths;    /* [2*n_samp] or NULL */
  int32_t* path_weight;     /* [cap_paths] min_weight of every path, task after task, pop order; or NULL */
  int32_t* path_seq_off;    /* [cap_paths+1] or NULL */
  char*    path_seq;        /* [cap_path_chars] or NULL */
  int32_t  cap_opts, cap_opt_chars, cap_paths, cap_path_chars;
} hipstr_flank_out_t;

/* calc_kmer_length for both flanks of every locus (host only): kmer[2*l + flank], -1 = too repetitive (:623) — a ref_seq of length <=
 * min_kmer included.  Only n_loci, blk_nopts, opt_off and seq of the batch are read.  0 = 10 / 15. */
int hipstr_flank_kmer_lengths(const hipstr_batch_t* batch, int32_t min_kmer, int32_t max_kmer, int32_t* kmer /* [2*n_loci] */);
/* Host only (works on a library that never opened a device).  Only flank_seq_off / flank_seq of `tr` and n_loci, n_samples, read_off,
 * sample_label of `pb` are read. */
int hipstr_flank_assemble(const hipstr_post_batch_t* pb, const hipstr_flank_request_t* rq, const hipstr_trace_out_t* tr, hipstr_flank_out_t* out);
/* The same stage where the records lie: the strings are read from td, the (locus, sample) runs of reads from what hipstr_post_upload left on
 * the device (the run need not have been launched); of the per-read arrays only seed and read_req are uploaded.  One wavefront assembles one
 * task (hipstr_amd/csrc/flank_task.h); only the per-task records and the paths' bytes come home, and the aggregation is the host entry
 * point's own function on them.  A task beyond a limit of hipstr_amd/csrc/flank_layout.h (distinct edges, nodes, path records, reads, string
 * length, a byte other than ACGTN, k above 15) is assembled by the host code inside the same call, on flank strings fetched once.  Outputs,
 * return codes and hipstr_last_error() equal hipstr_flank_assemble on hipstr_trace_dev_fetch(td, HIPSTR_TRACE_F_FLANKS), byte for byte.
 * Device and pinned blocks come from the context's caches. */
int hipstr_flank_assemble_dev(hipstr_post_dev_t* pd, const hipstr_flank_request_t* rq, const hipstr_trace_dev_t* td, hipstr_flank_out_t* out);

/*
 * HaplotypeGenerator for a batch of single-region loci: what SeqStutterGenotyper::init -> build_haplotype (seq_stutter_genotyper.cpp:422-488)
 * leaves behind, from UN-POOLED reads, a region and a reference window — add_haplotype_block (HaplotypeGenerator.cpp:286-337) with
 * gen_candidate_seqs (:157-241), extract_sequence (:82-155), trim (:12-80), get_aln_bounds (:243-254), fuse_haplotype_blocks (:339-366) and
 * the bounds loop of build_haplotype (:428-432).  The reference-VCF path (add_vcf_haplotype_block) and loci of several regions are not here.
 * The reads come as a hipstr_batch_t of which only n_loci, read_off, base_off, bases, read_start and cigar_* are read.
 *
 * Per locus: status 1 when region_start < 40 or region_stop + 40 > chrom_len (:292); else, with the padded region [region_start - 5,
 * region_stop + 5] and the smallest start / largest stop of the FLAGGED reads (use_read), status 2 when min + 5 >= region_start - 5 or
 * max - 5 <= region_stop + 5 (:305); else status 0 and the three blocks.  A flagged read is COUNTED when start < region_start - 5 and
 * stop > region_stop + 5 (stop as given: the reference only compares it, so either end convention of the caller works); its extracted
 * string is the run of its bases the walk of :86-152 collects — an insertion is kept when the walk stands in [region_start - 5, region_stop
 * + 5], either edge included, skipped before it; deleted bases are skipped; an empty extraction is the allele "" — folded to upper case
 * (a-z only).  Per sample s (ascending), with n_s counted reads, a string with c of them is strong when c >= 2 and c >= 0.2 * n_s, and adds
 * c * 1.0 / n_s to the string's sample fraction (IEEE double, summed in ascending sample index); a sample without counted reads adds nothing
 * and is not among the spanning samples.  A string is selected when it is strong in a sample, or its fraction > 0.05 * spanning samples, or
 * its reads > 0.05 * counted reads.  The options of block 1 are the padded region's reference string first, then the other selected strings
 * by (length, bytes as unsigned char); trim (ideal_min_length = 3 * period) then takes a common prefix / suffix of at most 5 bases off all of
 * them and moves the block's bounds.  Blocks 0 and 2 are the reference from max(blk1_start - 35, min start of ALL the locus' reads) — at most
 * blk1_start - 10 — to block 1, and from block 1 to min(blk1_end + 35, max stop of ALL reads), at least blk1_end + 10.
 * Deviation from the reference: a locus without a flagged read makes :305 compute INT_MAX + 5 and INT_MIN - 5, signed overflow; here that
 * arithmetic is done in 64 bits, so such a locus has status 2.
 *
 * Sizes: every output array is sized by the input.  Options (entries of opt_off, less one) <= 3*n_loci + n_reads; sequence bytes <=
 * win_off[n_loci] + base_off[n_reads]; the dist_* arrays hold at most n_reads entries.  A locus with status != 0 has 0 options in every
 * block, blk_start = blk_end = 0, its counts and trims are 0 and its reads' ext_off / ext_len are -1; min_aln_start / max_aln_stop are
 * written for every locus (INT32_MAX / INT32_MIN for one without reads).
 * hipstr_hapgen works on the device, in chunks of whole loci under a workspace budget (HIPSTR_HAPGEN_WS_MIB, default 256): counted reads are
 * grouped by a 64-bit hash of their extracted bytes and every member is then compared with its group's first read byte for byte — a locus in
 * which two different strings share a hash, and a locus beyond a cap of hipstr_amd/csrc/hapgen_layout.h (reads, samples, distinct strings),
 * is done by the host code inside the same call.  hipstr_hapgen_host is that host code for the whole batch; it needs no device.  Both give
 * identical bytes in every output, dist_frac included.
 * Refused (non-zero + hipstr_last_error(), nothing written, nothing launched): NULL arguments, a NULL required array, offset tables the
 * other entry points refuse, a CIGAR op other than = X I D, a period < 1, region_stop < region_start, n_samples < 0, a sample_label outside
 * [0, n_samples), a window shorter than region_stop - region_start + 80 for a locus that passes the chromosome-end check, a read whose
 * given read_stop exceeds start + the sum of its =, X and D runs (the one input on which the reference's walk runs off the CIGAR, :153).
 * hipstr_hapgen without a device fails as every device entry point does; it does not fall back to the host.  A HIP error in a later chunk
 * leaves the loci of the chunks before it written, as with hipstr_pool_reads.  Reads in front of read_off[0] belong to no locus: their
 * ext_off / ext_len are left untouched.
 */
typedef struct hipstr_hapgen_request {
  const int32_t* region_start;  /* [n_loci] Region::start()                                              */
  const int32_t* region_stop;   /* [n_loci] Region::stop(), exclusive                                    */
  const int32_t* period;        /* [n_loci]                                                              */
  const int64_t* chrom_len;     /* [n_loci] chrom_seq.size(): the end checks of :292                     */
  const int32_t* win_off;       /* [n_loci+1] offsets into window                                        */
  const char*    window;        /* per locus chrom_seq[region_start-40, region_stop+40), any case        */
  const int32_t* n_samples;     /* [n_loci]                                                              */
  const int32_t* sample_label;  /* [n_reads] sample within the locus; NO order of the reads is assumed   */
  const int32_t* read_stop;     /* [n_reads] Alignment::get_stop(), or NULL = start + sum of =,X,D runs  */
  const uint8_t* use_read;      /* [n_reads] use_for_hap_generation(0), or NULL = all                    */
  const double*  stutter;       /* [6*n_loci] only copied into the batch hipstr_hapgen_batch returns     */
} hipstr_hapgen_request_t;
typedef struct hipstr_hapgen_out {
  int32_t* status;              /* [n_loci]   0 ok, 1 too near to the chromosome ends, 2 no spanning alignments */
  int32_t* blk_start;           /* [3*n_loci] as in hipstr_batch_t                                              */
  int32_t* blk_end;             /* [3*n_loci]                                                                   */
  int32_t* blk_nopts;           /* [3*n_loci] 0 for every block of a failed locus                               */
  int32_t* opt_off;             /* [n_opts+1] locus-major, block-major, option-minor                            */
  char*    seq;                 /* upper case                                                                   */
  int32_t* n_spanning;          /* [n_loci] tot_reads: counted reads                                            */
  int32_t* n_samples_spanning;  /* [n_loci] tot_samples                                                         */
  int32_t* n_distinct;          /* [n_loci] distinct extracted strings                                          */
  int32_t* left_trim;           /* [n_loci] what trim took off                                                  */
  int32_t* right_trim;          /* [n_loci]                                                                     */
  int32_t* min_aln_start;       /* [n_loci] over ALL reads of the locus (:428-432)                              */
  int32_t* max_aln_stop;        /* [n_loci]                                                                     */
  int32_t* ext_off;             /* [n_reads] or NULL: first base of the read's extracted run, within the read; -1 = not counted */
  int32_t* ext_len;             /* [n_reads] or NULL: its length; -1 = not counted                              */
  int32_t* dist_len;            /* [n_reads] or NULL: per distinct string, locus after locus (n_distinct each), in (length, bytes) order */
  int32_t* dist_rep;            /* [n_reads] or NULL: the first read (batch index) that carries it              */
  int32_t* dist_reads;          /* [n_reads] or NULL: read_counts                                               */
  int32_t* dist_strong;         /* [n_reads] or NULL: must_inc — samples in which it is strong                  */
  double*  dist_frac;           /* [n_reads] or NULL: sample_counts                                             */
} hipstr_hapgen_out_t;
int hipstr_hapgen(const hipstr_batch_t* reads, const hipstr_hapgen_request_t* rq, hipstr_hapgen_out_t* out);        /* on the device */
int hipstr_hapgen_host(const hipstr_batch_t* reads, const hipstr_hapgen_request_t* rq, hipstr_hapgen_out_t* out);   /* host only, no device needed */
/* failure_msg_ of the reference for a status: "" for 0, NULL for a code that is none */
const char* hipstr_hapgen_status_message(int32_t status);

/* The un-pooled batch build_haplotype leaves behind, in one allocation, over the loci whose status is 0 (in locus order): the haplotype
 * arrays from the stage, hap_off from the option counts, period and stutter from the request, the kept loci's reads copied (quals too:
 * reads->quals must be given), realign_hap = realign_read = NULL — ready for hipstr_pool_batch and hipstr_post_*.  flags:
 * HIPSTR_HAPGEN_ON_HOST uses hipstr_hapgen_host, 0 the device.  NULL + hipstr_last_error() on a refusal or a failure.  _locus: the original
 * index of every kept locus ([_batch()->n_loci]); _status: the status of all loci ([reads->n_loci]). */
#define HIPSTR_HAPGEN_ON_HOST 1u
typedef struct hipstr_hapgen_batch hipstr_hapgen_batch_t;
hipstr_hapgen_batch_t* hipstr_hapgen_batch(const hipstr_batch_t* reads, const hipstr_hapgen_request_t* rq, uint32_t flags);
const hipstr_batch_t*  hipstr_hapgen_batch_batch(const hipstr_hapgen_batch_t* h);
const int32_t*         hipstr_hapgen_batch_locus(const hipstr_hapgen_batch_t* h);
const int32_t*         hipstr_hapgen_batch_status(const hipstr_hapgen_batch_t* h);
void hipstr_hapgen_batch_free(hipstr_hapgen_batch_t* h);

/*
 * The allele-set update between two rounds of SeqStutterGenotyper::genotype for a batch of loci: the body of add_and_remove_alleles
 * (seq_stutter_genotyper.cpp:330-369) — the new blocks, the new Haplotype's strings, allele_mapping and realign_to_haplotype — without the
 * matrix, the alignment or the trace cache.  What comes out feeds hipstr_rm_remap (allele_mapping, new_n_alleles), hipstr_hmm_upload
 * (_batch), hipstr_hmm_trace_* / hipstr_post_census* / the next update (_batch_all, hap_to_allele).
 * Per locus that is on: every block keeps its options whose keep flag is set, in their order (HapBlock::remove_alleles, HapBlock.h:138-147),
 *   for the blocks keep_blocks names (bit b = block b); the strings of add_off's (locus, block) run go behind them in the order given
 *   (add_alternate, :345-350) — a string the block already holds is added again, the empty string is a legal option.
 * Haplotypes are enumerated as Haplotype::next visits them (Haplotype.cpp:157-196: a reflected mixed-radix Gray code, block 0 fastest);
 *   a haplotype IS the bytes of its three options concatenated: two different option triples with equal bytes are one key (:331-336).
 * allele_mapping[old k] = the LAST new haplotype with old k's bytes, where old k is the LAST old haplotype with those bytes; -1 for every
 *   other old haplotype (:335, :365).  realign_hap[new j] = 0 iff some old haplotype has j's bytes — also when j's options are new (an
 *   added string equal to a removed or a present one) — else 1 (:361-364).  hap_to_allele(b)[new j] = j's option in block b (:219-227).
 * added[l] = 1 iff a string was added to locus l (:344-350, the condition of :397-398).
 * A locus that is off (locus_on[l] == 0) takes the identity whatever its strings: blocks copied, allele_mapping[k] = k, realign_hap 0,
 *   added 0; keep and add_off are not read for it (its add_off runs must still be there, and may be empty).
 * :369 (the first haplotype keeps its bytes) holds by construction: option 0 of every block is kept.
 * hipstr_alleles_apply works on the device, one workgroup per locus (alleles.hip): the host computes counts and offsets only, the device
 *   gathers the new strings, hashes every option once (64-bit polynomial; a haplotype's hash follows from its three options'), puts the old
 *   haplotypes into an LDS table and looks the new ones up; the hash only filters — equality is always decided on the bytes.  A locus of more
 *   than 1024 haplotypes or 1024 options (before or after) takes the host code inside the same call.  hipstr_alleles_apply_host is that host
 *   code for the whole batch; it needs no device.  Both give identical bytes in every output.  Device and pinned blocks come from the
 *   context's caches: no allocation in steady state.
 * Refused (NULL + hipstr_last_error(); checked on the host before any launch): NULL arguments, a block without options, opt_off / hap_off /
 *   add_off / add_seq_off that decrease or do not start at 0, hap_off that is not the prefix sum of num_combs, a keep that drops option 0 of a
 *   block it applies to in a locus that is on, a new num_combs (or the batch's sum) above INT32_MAX, more than INT32_MAX new sequence bytes.
 * The result owns its arrays; the read-side pointers of its batches are borrowed from rq->pooled, which must outlive it.
 */
typedef struct hipstr_alleles_request {
  const hipstr_batch_t* pooled;   /* the round's pooled batch: the haplotype side is read, the read side passed on */
  const uint8_t* locus_on;        /* [n_loci], or NULL = every locus */
  const uint8_t* keep;            /* [n_opts] opt_off's enumeration (hipstr_census_out_t::called / spanned), or NULL = keep everything */
  uint32_t       keep_blocks;     /* bit b: keep applies to block b */
  const int32_t* add_off;         /* [3*n_loci+1] strings to add per (locus, block), or NULL = none */
  const int32_t* add_seq_off;     /* [add_off[3*n_loci]+1] */
  const char*    add_seq;
} hipstr_alleles_request_t;
typedef struct hipstr_alleles hipstr_alleles_t;
hipstr_alleles_t* hipstr_alleles_apply(const hipstr_alleles_request_t* rq);        /* on the device */
hipstr_alleles_t* hipstr_alleles_apply_host(const hipstr_alleles_request_t* rq);   /* host only, no device needed */
const hipstr_batch_t* hipstr_alleles_batch(const hipstr_alleles_t* a);             /* blk_nopts, opt_off, seq, hap_off rebuilt; realign_hap the new mask */
const hipstr_batch_t* hipstr_alleles_batch_all(const hipstr_alleles_t* a);         /* the same with realign_hap = NULL */
const int32_t* hipstr_alleles_mapping(const hipstr_alleles_t* a);                  /* [sum old A] allele_mapping */
const int32_t* hipstr_alleles_new_n_alleles(const hipstr_alleles_t* a);            /* [n_loci] */
const int32_t* hipstr_alleles_hap_to_allele(const hipstr_alleles_t* a, int block); /* [sum new A]; NULL for a block outside 0..2 */
const uint8_t* hipstr_alleles_added(const hipstr_alleles_t* a);                    /* [n_loci] */
void hipstr_alleles_free(hipstr_alleles_t* a);

/*
 * What genotype() does with one census (seq_stutter_genotyper.cpp:570-601, :647-663), driving the update above: per locus, by phase[l],
 *   ADD with candidates (census->cand_off): new_n_haps > max_total_haplotypes -> phase ABORTED, the identity, status 1 (:591-595: the locus
 *     genotype() returns false for); else the candidates — already in orderByLengthAndSequence order — are added to block 1, the phase stays.
 *   ADD without candidates falls through to UNCALLED: in every block of more than one option the options >= 1 whose census->called is 0 are
 *     dropped (:255, :305-311); if any was, the phase becomes UNSPANNED and the locus is done for this call; else it falls through to
 *   UNSPANNED: block 1's options >= 1 whose census->spanned is 0 are dropped, the phase becomes DONE.
 *   DONE / ABORTED: the identity.  A locus nothing is added to or dropped from takes the identity too.
 * phase is read and written; max_total_haplotypes 0 = the reference's 1000; flags: HIPSTR_ALLELES_ON_HOST uses hipstr_alleles_apply_host,
 * 0 the device.  out (caller's arrays, [n_loci] each): status (0, or 1 for a locus that aborted in this call), n_added, n_removed and
 * n_affected_blocks (the numbers of the log lines :592 ff., :651, :660), any_added (whether to upload, align and scatter this round).
 * Refused (NULL + hipstr_last_error(), phase and out untouched): what hipstr_alleles_apply refuses, a phase outside 0..4, cand_off that
 * decreases, and a locus that reaches UNSPANNED with a flank block of more than one option (the census writes `spanned` for block 1 only).
 * copy_read and the re-keying of the trace cache through allele_mapping (:401-409) stay with the caller.
 */
#define HIPSTR_PHASE_ADD       0
#define HIPSTR_PHASE_UNCALLED  1
#define HIPSTR_PHASE_UNSPANNED 2
#define HIPSTR_PHASE_DONE      3
#define HIPSTR_PHASE_ABORTED   4
#define HIPSTR_ALLELES_ON_HOST 1u
typedef struct hipstr_alleles_step_out {
  int32_t* status;             /* [n_loci] */
  int32_t* n_added;            /* [n_loci] */
  int32_t* n_removed;          /* [n_loci] */
  int32_t* n_affected_blocks;  /* [n_loci] */
  int32_t  any_added;
} hipstr_alleles_step_out_t;
hipstr_alleles_t* hipstr_alleles_step(const hipstr_batch_t* pooled, const hipstr_census_out_t* census, int32_t* phase /* [n_loci] */,
                                      int32_t max_total_haplotypes, uint32_t flags, hipstr_alleles_step_out_t* out);

/* The diagnostics entry points (hipstr_debug_*: what the tests, the fuzzers and bench.py look inside the library with) are declared in
 * hipstr_hmm_debug.h — not part of the drop-in ABI; a build with -DHIPSTR_NO_DEBUG_ABI leaves them out of the library. */

const char* hipstr_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HIPSTR_HMM_H_ */
