/*
 * pgx.h -- C ABI of libpgx.so, the MI355X (gfx950) hot path of pangenomix.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * It replaces two things in the reference (AnnaLew/pangenomix, a pure-Python
 * package that has no native layer of its own):
 *
 *   pangenome.py:425-450 + :2061-2068   cluster_with_cdhit(): the shell pipe to the
 *                                       external `cd-hit` / `cd-hit-est` programs
 *                                       -> pgx_cluster_greedy*
 *   pangenome_analysis.py:72-98         estimate_pan_core_size(): the Python double loop
 *                                       over scipy CSR rows -> pgx_presence_bitmap* +
 *                                       pgx_pan_core*
 *   pangenome_analysis.py:101-166       compute_bernoulli_grid_core_genome(): the dense
 *                                       numpy likelihood and gradient -> pgx_bernoulli_*
 *   pangenome_analysis.py:169-242       compute_bernoulli_grid_core_genome_cd(): one scipy
 *                                       brentq call per gene and genome and sweep
 *                                       -> pgx_bernoulli_cd*
 *   pangenome_analysis.py:457-492       ks_montecarlo_bbn() / draw_bbn(): np.random.choice
 *                                       and the per-iteration eCDF loop -> pgx_bbn_*
 *   fcd.py:15-138, :199-219             formal_concept_decomposition() / compute_concept_coverage(): the dense
 *                                       np.ix_ block sums -> pgx_fcd*
 *   fcd.py:168-196                      compute_concept_list_similarity(): the Python double loop over pairs of
 *                                       sets -> pgx_fcd_match*
 *   sparse_utils.py:73-109, ml_pipelines.py:349-388   compress_rows_spmatrix() / contingency_tables_from_sparse(): the
 *                                       per-phenotype association screen -> pgx_assoc*
 *   pangenome.py:1246-1330, :1812-1889  validate_gene_table[_dense]() / extract_dominant_alleles(): the Python loops
 *                                       over allele rows or genome columns -> pgx_allele_runs*
 *   core_genome.py:7-26, allele_identification.py:7-20   create_core_genes_fasta() / create_alleles_fasta(): the
 *                                       iterrows() loops that pick one allele per gene -> pgx_core_select*
 *
 * The reference-side binding is a ctypes stub. Conventions:
 *   - every function returns 0 on success and a negative pgx_status on error;
 *     pgx_last_error() gives the thread-local message; no exception crosses the ABI;
 *   - the caller owns every buffer; the library keeps no caller pointer after return;
 *   - pgx_ctx owns device state (stream, scratch); one context per thread, calls on
 *     one context are not re-entrant;
 *   - *_dev variants take DEVICE pointers and a hipStream_t (as void*); they only
 *     enqueue work on that stream (graph-capturable: no allocation, no sync) and are
 *     what bench.py times with inputs resident in HBM. The plain variants take HOST
 *     pointers and do the copies themselves. (One exception: pgx_bernoulli_cd_dev
 *     synchronises its stream once, at its end; see there.)
 *   - there is no CPU fallback: without a usable GPU every compute entry point fails
 *     with PGX_ERR_NO_DEVICE.
 */
#ifndef PGX_H
#define PGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_VERSION 300 /* 0.3.0 */
#define PGX_EXCHANGE_KEYS 65536u /* keys per process and exchange = the largest window */
#define PGX_EXCHANGE_WORDS (PGX_EXCHANGE_KEYS + 8u) /* uint64 per process and exchange: the keys + the error word (+ padding) */
#define PGX_EXCHANGE_SLOTS 2u    /* windows in flight, each with its own send / receive buffers */

typedef enum pgx_status {
    PGX_OK = 0,
    PGX_ERR_INVALID = -1,   /* bad argument */
    PGX_ERR_NO_DEVICE = -2, /* no usable HIP device */
    PGX_ERR_HIP = -3,       /* a HIP runtime call failed */
    PGX_ERR_NOMEM = -4,
    PGX_ERR_CAPACITY = -5,  /* an internal fixed-capacity buffer overflowed */
    PGX_ERR_INTERNAL = -6
} pgx_status;

typedef struct pgx_ctx pgx_ctx;

typedef struct pgx_device_info_t {
    char name[64];
    char arch[32];          /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    int32_t device_id;
    int32_t compute_units;
    int32_t wavefront_size;
    int32_t lds_bytes_per_block;
    uint64_t hbm_bytes;
    int32_t clock_khz;
    int32_t reserved;
} pgx_device_info_t;

int pgx_version(void);
const char *pgx_last_error(void);
/* One context = ONE device. SURVEY 8b sketched `pgx_ctx_create(const int *device_ids, int n_devices, ...)`; the
 * build deliberately deviates: the multi-GPU mode is one PROCESS per GPU (torch.distributed / RCCL, see
 * pgx_cluster_params.shard_*), each process with its own single-device context, so a context never spans
 * devices. pgx_ctx_create_on() takes the surveyed argument shape and accepts exactly one device id. */
int pgx_ctx_create(int device_id, pgx_ctx **out);
int pgx_ctx_create_on(const int *device_ids, int n_devices, pgx_ctx **out);
void pgx_ctx_destroy(pgx_ctx *ctx);
int pgx_device_info(pgx_ctx *ctx, pgx_device_info_t *out);

/* Optional per-kernel timing for bench.py's roofline line: when enabled, every kernel the
 * library launches is bracketed by HIP events on the stream it is launched on; slots
 * accumulate by kernel name. Reading a slot waits for its pending events. */
int pgx_profile_enable(pgx_ctx *ctx, int on);
int pgx_profile_reset(pgx_ctx *ctx);
int pgx_profile_count(pgx_ctx *ctx);
int pgx_profile_read(pgx_ctx *ctx, int slot, char *name, size_t name_bytes, double *total_ms,
                     uint64_t *launches);

/* ------------------------------------------------------------------------------------
 * K3: presence/absence bitmap and pan/core rarefaction curves
 * (pangenome_analysis.py:72-98).
 *
 * Bitmap layout: genome-major; genome s owns `stride_words` 64-bit words, gene g is
 * bit (g & 63) of word (g >> 6). stride_words = pgx_bitmap_stride_words(n_genes)
 * (rows padded to a multiple of 16 words = 128 B so that every lane's 16-byte load is
 * aligned and in bounds; pad bits are zero).
 * ---------------------------------------------------------------------------------- */
uint32_t pgx_bitmap_stride_words(uint32_t n_genes);

/* bits[genome][word] |= 1 for every (row_of_record[k], genome_of_record[k]).
 * out_bits must hold n_genomes * stride_words words; it is zeroed first.
 * Duplicates: the number of records whose bit was already set, i.e. repeated (row, genome)
 * coordinates (counted on the device while the bitmap is built: the read-modify-write returns the
 * word before the update). The reference's loop (pangenome_analysis.py:88-90) equals the OR/AND
 * form only for a 0/1 table without duplicates, so the Python layer refuses a table with any.
 * Host variant: out_duplicates may be NULL; a record out of range fails with PGX_ERR_INVALID.
 * Device variant: d_counters = 2 x uint64 in device memory {duplicates, records out of range
 * (skipped)}, zeroed first; may be NULL. */
int pgx_presence_bitmap(pgx_ctx *ctx, const int32_t *row_of_record, const int32_t *genome_of_record,
                        uint64_t n_records, uint32_t n_rows, uint32_t n_genomes, uint64_t *out_bits,
                        uint64_t *out_duplicates);
int pgx_presence_bitmap_dev(pgx_ctx *ctx, const int32_t *d_row_of_record,
                            const int32_t *d_genome_of_record, uint64_t n_records, uint32_t n_rows,
                            uint32_t n_genomes, uint64_t *d_out_bits, uint64_t *d_counters, void *stream);

/* For each iteration i and step j (genomes taken in the order perms[i][0..j]):
 *   out_pan[i][j]  = number of genes present in at least one of the first j+1 genomes
 *   out_core[i][j] = number of genes present in all of the first j+1 genomes
 * perms: [n_iter][n_genomes] int32, each row a permutation of 0..n_genomes-1 (generated by
 * the caller with the legacy numpy RNG, pangenome_analysis.py:84-85). Outputs [n_iter][n_genomes]. */
int pgx_pan_core(pgx_ctx *ctx, const uint64_t *bits, uint32_t n_genes, uint32_t n_genomes,
                 const int32_t *perms, uint32_t n_iter, int32_t *out_pan, int32_t *out_core);
/* The whole of estimate_pan_core_size()'s device work in one call (pangenome_analysis.py:72-98):
 * COO coordinates of the binary gene x genome table and the permutations go up once, the bitmap
 * is built and consumed on the device (no bitmap round trip), the two curves come back. Device
 * buffers live in the context's workspace: repeated calls do not allocate. */
int pgx_pan_core_coo(pgx_ctx *ctx, const int32_t *row_of_record, const int32_t *genome_of_record,
                     uint64_t n_records, uint32_t n_genes, uint32_t n_genomes, const int32_t *perms,
                     uint32_t n_iter, int32_t *out_pan, int32_t *out_core, uint64_t *out_duplicates);
/* Row occupancy: out_counts[r] = number of genomes that hold row r (gene or allele) = the popcount of
 * the row across the bitmap. What core_genome.py:127-155 (count_gene_occurence) and
 * allele_identification.py:129-157 (count_allele_occurence) obtain from the .npz triples with a pandas
 * groupby; equal to their counts for a table without duplicate coordinates (duplicates reported). */
int pgx_row_counts(pgx_ctx *ctx, const int32_t *row_of_record, const int32_t *genome_of_record,
                   uint64_t n_records, uint32_t n_rows, uint32_t n_genomes, int32_t *out_counts,
                   uint64_t *out_duplicates);
int pgx_row_counts_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes,
                       int32_t *d_counts, void *stream);
size_t pgx_pan_core_workspace_bytes(uint32_t n_genes, uint32_t n_genomes, uint32_t n_iter);
int pgx_pan_core_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_genomes,
                     const int32_t *d_perms, uint32_t n_iter, int32_t *d_out_pan,
                     int32_t *d_out_core, void *d_workspace, size_t workspace_bytes, void *stream);

/* Heaps-law fits of the pan curves (pangenome_analysis.py:24-48, fit_heaps_by_iteration): per
 * iteration i the least-squares (alpha, kappa) of  pan[i][j-1] = kappa * j^alpha,  j = 1..n_genomes, from
 * the reference's start point (0.5, min of the row). Floating point: equal to scipy's curve_fit to a
 * tolerance (tests: rtol 1e-5; scipy's default stopping rule leaves it ~3e-6 off the minimum), and to the exact
 * least-squares minimiser (60-digit arithmetic, tests/golden/next/exact_heaps.npz) within rtol 6.4e-14 on alpha and kappa
 * (= 64 x 9.93e-16, the farthest a float64 restatement of the same fit ends from it on that file's curves: a floor
 * measured on the CPU restatement, not on the device, so a device pow / log that rounds differently can move the
 * fit against it; alpha of a flat curve absolutely). The device variant reads pgx_pan_core_dev's int32 output in place. */
int pgx_heaps_fit(pgx_ctx *ctx, const double *pan, uint32_t n_iter, uint32_t n_genomes, double *out_alpha,
                  double *out_kappa);
int pgx_heaps_fit_dev(pgx_ctx *ctx, const int32_t *d_pan, uint32_t n_iter, uint32_t n_genomes,
                      double *d_alpha, double *d_kappa, void *stream);

/* ------------------------------------------------------------------------------------
 * K1/K2: greedy incremental clustering with cd-hit's rules.
 * ---------------------------------------------------------------------------------- */
typedef struct pgx_cluster_params {
    int32_t alphabet;       /* 0 = protein (cd-hit), 1 = nucleotide (cd-hit-est) */
    int32_t word_len;       /* -n, 2..5 protein; nucleotide words use the same value */
    int32_t band_width;     /* -b, default 20 */
    int32_t min_length;     /* -l, default 10: sequences with length <= this are discarded */
    int32_t both_strands;   /* -r, nucleotide only, default 1 */
    int32_t batch_size;     /* queries per window (greedy sweep), at most PGX_EXCHANGE_KEYS; 0 = library default
                             * (pgx_cluster_window_cap). Any value gives the same clusters. */
    double identity;        /* -c, global identity threshold (double, as cd-hit parses it) */
    /* short-word filter cut-offs as fractions of the query length. cd-hit takes
     * max(analytic bound, naa_stat[tolerance-1][100c-40][...]/100); its table is not
     * available offline, so the caller passes the final values (see
     * pangenomix_amd/cluster.py:filter_cutoffs and DESIGN.md "filter table"). */
    double aan_cutoff;      /* shared word_len-mers   */
    double aas_cutoff;      /* shared 2-mers (4-mers for nucleotides) on the best band */
    /* Record-sharded multi-GPU mode, one process per GPU, every process called with the same
     * sequences (all 0 / NULL = single GPU). The sorted list is cut into windows; member i of a
     * window belongs to process i % shard_count, which runs the short-word filter and the
     * alignments of its members against its replica of the representative index. After every
     * evaluation the window's best keys (one uint64 per member; the minimum over the accepted
     * representatives) are ALL-GATHERED: the library keeps them in exchange_send, calls
     * `exchange`, and folds the rows of exchange_recv. New representatives follow from the
     * gathered keys by a deterministic rule every process repeats, so all replicas of the index
     * stay identical and all processes return the same clusters. Work counters and identities are
     * partial per process: sum the counters / take the maximum of out_identity over the processes
     * (pangenomix_amd/cluster.py does). */
    int32_t shard_index, shard_count;
    /* All-gather of PGX_EXCHANGE_WORDS uint64 per process: slot `slot` of exchange_send of every process p into
     * exchange_recv[slot][p][...] of all. Two consecutive windows are in flight on two streams, each with its own
     * slot (send: [PGX_EXCHANGE_SLOTS][PGX_EXCHANGE_WORDS], recv: [PGX_EXCHANGE_SLOTS][shard_count][PGX_EXCHANGE_WORDS]).
     * The callback ENQUEUES the collective on `stream` (the stream that window works on) and returns without
     * waiting: e.g. torch.distributed.all_gather_into_tensor under torch.cuda.ExternalStream(stream) = RCCL over
     * xGMI with the nccl backend. Every process issues its calls in the same order. 0 = success. A few calls per
     * window. The word behind the keys carries the process's error state: a capacity failure on one process makes
     * every process return PGX_ERR_CAPACITY at the same point (nobody is left waiting in a collective). */
    /* (exchange == NULL with shard_count >= 1: the context's own communicator, pgx_rccl_comm_create below; the
     * exchange_* fields are then unused) */
    int (*exchange)(void *user, void *stream, int slot);
    void *exchange_user;
    void *exchange_send;    /* device (the caller's allocation, so that its collective library can address it) */
    void *exchange_recv;    /* device */
    /* cd-hit's MEMORY-CHUNKED rule, optional emulation. cd-hit bounds its word table by what is left
     * of `-M` (default 800 MB; the reference's call passes no -M, pangenome.py:444-447): when the table is full,
     * every sequence not yet clustered is compared with the current table at once (and joins the first
     * representative that accepts it), the table is emptied, and clustering goes on with what is left. A
     * sequence therefore joins a representative of the EARLIEST chunk that accepts it, which can differ from the
     * unchunked winner. Where cd-hit places the boundaries depends on its memory accounting, which cannot be
     * reproduced offline, so they are an input: positions in the length-sorted list of the clustered sequences
     * (those longer than min_length), strictly increasing, each in (0, n_clustered); position b means "the table
     * is flushed before the b-th sequence of that list is processed". NULL / 0 = the unchunked rule (-M 0). */
    const uint32_t *chunk_boundaries;
    uint32_t n_chunk_boundaries;
    uint32_t reserved0;
} pgx_cluster_params;

/* Instrumentation that defines the roofline denominator. All are
 * properties of the sequential algorithm (what a one-by-one greedy pass visits), so the
 * oracle and the GPU path must agree on every field except `sweeps`. */
typedef struct pgx_cluster_stats {
    uint64_t n_input;          /* sequences handed in */
    uint64_t n_clustered;      /* N: sequences longer than min_length */
    uint64_t n_clusters;
    uint64_t sum_len_queries;  /* sum of L over clustered sequences */
    uint64_t sum_len_reps;     /* R */
    uint64_t rep_words;        /* R_words: distinct-word list entries written for representatives */
    uint64_t posting_visits;   /* P: posting entries a query's distinct words meet in the table */
    uint64_t filter_pairs;     /* (query, rep) pairs examined whose word count reached required_aan */
    uint64_t aligned_pairs;    /* of those, pairs that passed the diagonal test and were aligned */
    uint64_t aligned_rep_len;  /* A: sum of L_rep over aligned_pairs */
    uint64_t dp_cells;         /* sum over aligned_pairs of L_query * (band_right-band_left+1) */
    uint64_t sweeps;           /* windows (GPU path; 0 in the oracle) */
    /* GPU path only, actual device work incl. speculative pairs (0 in the oracle):
     * [0] candidate pairs through the diagonal test, [1] pairs aligned, [2] residue bytes of the
     * aligned pairs (len_query + len_rep, 1 byte per residue), [3] query words walked by the filter
     * passes (an upper bound: residues of the window per pass; each costs one bit-map probe and, for
     * the pass over the whole index, one 64-byte line read) */
    uint64_t reserved[4];
} pgx_cluster_stats;

/* residues: concatenated ASCII letters (already validated / upper-cased by the caller),
 * offsets: n+1 entries. Sequences are processed in stable descending-length order.
 *   out_cluster[i]  cluster number in order of representative creation, -1 = discarded
 *   out_member[i]   index inside the cluster = .clstr member number (0 = representative)
 *   out_identity[i] matches / query length as float (0 for representatives)
 *   out_strand[i]   0 '+', 1 '-' (nucleotide, both_strands; may be NULL)
 *   stats           may be NULL. The counters are those of the SEQUENTIAL rule, which looks up every word of every
 *                   sequence in the whole table; with stats the library does all of those look-ups so that its
 *                   counters equal that rule's. Without, the passes over a window's new representatives leave out the
 *                   members that cannot gain from them (final ones; those whose best candidate no new representative
 *                   can precede). The clusters, member numbers, identities and strands are the same either way. */
int pgx_cluster_greedy(pgx_ctx *ctx, const uint8_t *residues, const uint64_t *offsets, uint32_t n,
                       const pgx_cluster_params *params, int32_t *out_cluster, int32_t *out_member,
                       float *out_identity, uint8_t *out_strand, uint32_t *out_n_clusters,
                       pgx_cluster_stats *stats);
/* Same, with the sequences already resident in HBM: d_residues / d_offsets are DEVICE
 * pointers (total_bytes = offsets[n]); the out_* arrays and stats are HOST memory. The inputs are
 * read on `stream` (work already enqueued there is waited for); consecutive windows then alternate
 * between `stream` and a second, lower-priority stream of the context, ordered by events. The call
 * returns after the last window has been resolved and both streams have drained. */
/* queries per window the library will use for these parameters (env PGX_WINDOW overrides) */
uint32_t pgx_cluster_window_cap(const pgx_cluster_params *params);
int pgx_cluster_greedy_dev(pgx_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_offsets, uint32_t n,
                           uint64_t total_bytes, const pgx_cluster_params *params, int32_t *out_cluster,
                           int32_t *out_member, float *out_identity, uint8_t *out_strand,
                           uint32_t *out_n_clusters, pgx_cluster_stats *stats, void *stream);

/* The record-sharded mode without a callback: the library's own RCCL communicator (optional). With shard_count >= 1,
 * exchange == NULL and a communicator on the context, pgx_cluster_greedy[_dev] keeps the exchange buffers itself and
 * enqueues ncclAllGather on the window's stream (RCCL over xGMI; nothing of the host language in the loop).
 *   pgx_rccl_load         dlopen of librccl.so (path NULL = the loader's search path; a PyTorch-ROCm process passes
 *                         torch/lib/librccl.so so that the copy PyTorch uses is shared). libpgx does not link RCCL.
 *   pgx_rccl_unique_id    128 bytes made by ONE process and handed to the others by the caller's own means
 *                         (a file, MPI, torch.distributed.broadcast_object_list ...)
 *   pgx_rccl_comm_create  collective: every process calls it with the same id, its rank and the world size
 *   pgx_rccl_comm_destroy (pgx_ctx_destroy does it too)
 * The reference has no counterpart (its clustering is one cd-hit process, pangenome.py:444-447). */
int pgx_rccl_load(const char *librccl_path);
int pgx_rccl_unique_id(uint8_t *out_id128);
int pgx_rccl_comm_create(pgx_ctx *ctx, const uint8_t *id128, int rank, int world);
int pgx_rccl_comm_destroy(pgx_ctx *ctx);

/* ------------------------------------------------------------------------------------
 * Host side of the pipeline around the clustering call: multi-threaded FASTA
 * ingest, first-seen exact de-duplication and the text outputs. No GPU involved.
 *
 *   pangenome.py:336-405   consolidate_seqs()             -> pgx_fasta_open + pgx_fasta_write_consolidated
 *   pangenome.py:425-450   FASTA -> sequences, .clstr out -> pgx_fasta_residues/offsets, pgx_fasta_write_clustered
 *   pangenome.py:453-560   rename_genes_and_alleles()     -> pgx_fasta_write_clustered
 *
 * Reading rules are the reference's (record = line starting with '>'; header = first whitespace
 * token minus '>'; sequence = stripped lines joined; no sequence = "missing"). Inputs its
 * line-by-line Python semantics treat specially (carriage returns, non-ASCII or control bytes,
 * one header naming two different sequences) are reported through info.simple = 0 with the reason in info.why: the array
 * accessors then return NULL and the Python layer takes its own statement-by-statement path.
 * Pointers returned by the accessors stay valid until pgx_fasta_close.
 * ---------------------------------------------------------------------------------- */
typedef struct pgx_fasta_set pgx_fasta_set;
typedef struct pgx_fasta_info_t {
    uint64_t n_records;        /* records, all files, in the order given */
    uint64_t n_missing;        /* of those, without sequence */
    uint64_t n_groups;         /* distinct sequences, first-seen order (the non-redundant set) */
    uint64_t n_residue_bytes;  /* sequence bytes of the non-redundant set */
    uint64_t n_header_bytes;
    uint32_t simple;           /* 1: everything below is available */
    uint32_t reserved;
    char why[256];             /* simple == 0: what was found */
} pgx_fasta_info_t;

int pgx_fasta_open(const char *const *paths, uint32_t n_paths, int n_threads /* 0 = all cores (<= 32) */,
                   pgx_fasta_set **out);
void pgx_fasta_close(pgx_fasta_set *fs);
int pgx_fasta_info(const pgx_fasta_set *fs, pgx_fasta_info_t *out);
const int32_t *pgx_fasta_group_of_record(const pgx_fasta_set *fs);   /* [n_records], -1 = no sequence, -2 = a
                                                                      * sequence without a header (nameless) */
const uint32_t *pgx_fasta_file_of_record(const pgx_fasta_set *fs);   /* [n_records] index into paths */
const uint64_t *pgx_fasta_rep_of_group(const pgx_fasta_set *fs);     /* [n_groups] first-seen record */
const uint8_t *pgx_fasta_residues(const pgx_fasta_set *fs);          /* the groups' sequences, concatenated: */
const uint64_t *pgx_fasta_offsets(const pgx_fasta_set *fs);          /* [n_groups + 1]; pgx_cluster_greedy's input */
const uint32_t *pgx_fasta_letters(const pgx_fasta_set *fs);          /* [n_groups] letters per sequence (.clstr length) */
const uint8_t *pgx_fasta_digests(const pgx_fasta_set *fs);           /* [n_groups][32] sha256 of the sequence */
const char *pgx_fasta_header_blob(const pgx_fasta_set *fs);          /* the records' headers, concatenated: */
const uint64_t *pgx_fasta_header_offsets(const pgx_fasta_set *fs);   /* [n_records + 1] */
/* consolidate_seqs()'s files: non-redundant FASTA, groups with several headers, headers without sequence */
int pgx_fasta_write_consolidated(const pgx_fasta_set *fs, const char *nr_path /* may be NULL */,
                                 const char *shared_path, const char *missing_path /* may be NULL */);
/* after pgx_cluster_greedy on (residues, offsets): cd-hit's .clstr, the allele name table
 * (<prefix><cluster><variant><member> TAB header TAB synonyms) and the non-redundant FASTA with the
 * allele names as headers (unclustered records dropped). NULL paths are skipped. */
int pgx_fasta_write_clustered(const pgx_fasta_set *fs, const int32_t *cluster, const int32_t *member,
                              const float *identity, const uint8_t *strand /* may be NULL */, int nucleotide,
                              const char *prefix, const char *variant, const char *clstr_path,
                              const char *names_path, const char *nr_out_path);

/* n_iter permutations of 0..n-1 drawn exactly as `p = np.arange(n); np.random.shuffle(p)` draws them from
 * numpy's legacy global generator (pangenome_analysis.py:84-85): MT19937 state key[624] / pos in, advanced
 * state out (np.random.get_state() / set_state()). out_perms: [n_iter][n] int32. */
int pgx_legacy_shuffles(uint32_t *key, int32_t *pos, uint32_t n, uint32_t n_iter, int32_t *out_perms);
/* the next n_words raw 32-bit outputs of numpy's legacy generator (MT19937 tempered words, in stream order; one
 * random_sample() double is ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 of two of them), advancing key / pos as numpy does:
 * a stream that ends on a block boundary leaves pos = 624 and the key un-twisted. Host only. */
int pgx_legacy_uniform_words(uint32_t *key, int32_t *pos, uint64_t n_words, uint32_t *out);

/* The whole of estimate_pan_core_size() (pangenome_analysis.py:51-98) from the gene x genome table's COO arrays:
 * `values` (the table's stored values, int64; may be NULL) are checked to be all 1 (out_not_one = how many are
 * not; the curves are then NOT computed), the permutations are drawn from the generator state (as pgx_legacy_shuffles
 * draws them, on a host thread while the coordinates are uploaded and the bitmap is built), and the result is
 * written as the reference returns it: out_table float64 [n_iter][2 * n_genomes], pan curves in columns
 * 0..n_genomes-1, core curves behind them. out_perms [n_iter][n_genomes] receives the permutations used. */
int pgx_pan_core_table(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, const int64_t *values,
                       uint64_t n_records, uint32_t n_genes, uint32_t n_genomes, uint32_t *mt_key, int32_t *mt_pos,
                       uint32_t n_iter, int32_t *out_perms, double *out_table, uint64_t *out_duplicates,
                       uint64_t *out_not_one);

/* Device-resident hand-off (SURVEY build plan step 5; north_star "emitting the gene x genome presence/absence bitmap"):
 * the bitmap of a pangenome is built ON THE DEVICE straight from the clustering result -- record r of the genome files is
 * an instance of gene cluster_of_group[group_of_record[r]] in genome genome_of_file[file_of_record[r]] (negative group or
 * cluster: nothing), rows = cluster numbers -- and stays in the context until the next pgx_bitmap_from_clusters on it.
 * out_token names it; pgx_pan_core_table_resident computes estimate_pan_core_size()'s table from it with no upload of
 * the table at all (the curves do not depend on the order of the rows); pgx_bitmap_resident_read copies it out
 * (n_genomes x pgx_bitmap_stride_words(n_genes) words). A stale token fails with PGX_ERR_INVALID. */
int pgx_bitmap_from_clusters(pgx_ctx *ctx, const int32_t *cluster_of_group, uint64_t n_groups,
                             const int32_t *group_of_record, const uint32_t *file_of_record, uint64_t n_records,
                             const int32_t *genome_of_file, uint32_t n_files, uint32_t n_genes, uint32_t n_genomes,
                             uint64_t *out_token);
int pgx_bitmap_resident_read(pgx_ctx *ctx, uint64_t token, uint64_t *out_bits);
int pgx_pan_core_table_resident(pgx_ctx *ctx, uint64_t token, uint32_t n_genes, uint32_t n_genomes, uint32_t *mt_key,
                                int32_t *mt_pos, uint32_t n_iter, int32_t *out_perms, double *out_table);

/* Bernoulli grid likelihood (compute_bernoulli_grid_core_genome, reference pangenome_analysis.py:101-166): gene i occurs in
 * genome j with probability p_i q_j. One evaluation at (P, Q) gives, for the binary table X,
 *   LL      = sum_ij X_ij log(p_i q_j) + (1 - X_ij) log(1 - p_i q_j)
 *   dL/dp_i = rowsum_i / p_i - sum_j (1 - X_ij) q_j / (1 - p_i q_j)
 *   dL/dq_j = colsum_j / q_j - sum_i (1 - X_ij) p_i / (1 - p_i q_j)
 * in fp64, with every cell's terms as these per-cell expressions give them (so nan / inf appear where they put them:
 * p_i q_j = 1 on a present cell gives nan in LL and in that row's and column's gradient). Deterministic: the same
 * inputs give the same bits on every call (no atomics; partials summed in an order fixed by the table's shape).
 * When every fl(p_i q_j) is a normal number below 1 the present cells' log terms are summed as
 * rowsum_i log p_i + colsum_j log q_j; flags = PGX_BERNOULLI_EXACT evaluates every cell's own log instead.
 * Accuracy: LL within 1e-12 x (the sum of its absolute terms) + 2^-52 x (present cells) of the per-cell sum, each
 * gradient entry within 1e-12 x the sum of its absolute terms. The second LL term is log(fl(p q))'s own: up to 2^-53
 * absolute per present cell, which the log p + log q form does not carry; it decides on tables with few absent cells
 * near p q = 1, where |log(p q)| is about 1e-8 per cell.
 * pq = [P (n_genes); Q (n_genomes)], out = [LL; dL/dp (n_genes); dL/dq (n_genomes)].
 *   pgx_bernoulli_eval_dev      d_bits: the table in the bitmap layout above (pad bits zero; they are not cells);
 *                               DEVICE pointers and a caller workspace of pgx_bernoulli_workspace_bytes(); enqueues
 *                               on `stream` only (no allocation, no sync)
 *   pgx_bernoulli_load          uploads the table's COO coordinates once and keeps its bitmap in the context for the
 *                               evaluations that follow; out_duplicates as pgx_presence_bitmap (may be NULL); a record
 *                               out of range fails with PGX_ERR_INVALID
 *   pgx_bernoulli_load_resident the same from the bitmap a pipeline left resident (pgx_bitmap_from_clusters), whose rows
 *                               are cluster numbers: row i of the table is row row_map[i] of the resident bitmap
 *                               (0 <= row_map[i] < its n_genes; n_genomes must equal its n_genomes). No upload of the
 *                               table. A stale token fails with PGX_ERR_INVALID and leaves no table loaded.
 *   pgx_bernoulli_eval          one evaluation of the loaded table from HOST pq into HOST out (n_genes + n_genomes
 *                               and 1 + n_genes + n_genomes doubles) */
#define PGX_BERNOULLI_EXACT 1u
size_t pgx_bernoulli_workspace_bytes(uint32_t n_genes, uint32_t n_genomes);
int pgx_bernoulli_eval_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_genomes, const double *d_pq,
                           uint32_t flags, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
int pgx_bernoulli_load(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_genes,
                       uint32_t n_genomes, uint64_t *out_duplicates);
int pgx_bernoulli_load_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, uint32_t n_genes,
                                uint32_t n_genomes);
int pgx_bernoulli_eval(pgx_ctx *ctx, const double *pq, uint32_t flags, double *out);

/* Coordinate descent on that likelihood (compute_bernoulli_grid_core_genome_cd, reference pangenome_analysis.py:169-242 and
 * :251-292), the whole loop on the device. From P = init_p (n_genes values inside [lo, hi]) and Q = init_q everywhere, each
 * of the n_iterations iterations solves, for every gene i with Q fixed,
 *   f(p) = rowsum_i / p - sum_{j absent} q_j / (1 - p q_j) = 0        in [lo, hi]
 * then the same for every genome j with the new P, then takes LL. Inside a sweep no solve depends on another. The rule
 * around a solve: f is taken at lo and at hi; when f(lo) f(hi) >= 0 the result is lo if |last - lo| < |last - hi| and hi
 * otherwise (last: the coordinate's previous value) -- which is also where a row present everywhere or nowhere goes --
 * else the root by Brent's method, stopped when half the bracket is below (2e-12 + 4 x 2^-52 |x|) / 2 or f(x) == 0: the
 * result lies within 2e-12 + 4 x 2^-52 |x| of a sign change of the computed f. A solve that has not stopped after 100
 * steps fails the call with PGX_ERR_INTERNAL (the outputs are then unspecified).
 * flags = PGX_BERNOULLI_CD_LOGS: the solver's variables are lp = log p and lq = log q between log lo and log hi,
 *   f(lp) = rowsum_i exp(-lp) - sum_{j absent} exp(lq_j) / (-expm1(lp + lq_j)),
 *   LL    = sum X (lp + lq) + (1 - X) log(-expm1(lp + lq)).
 * fp64 without contraction or fast division; p q, 1 - p q and each quotient are rounded once each. Deterministic: the
 * same inputs give the same bits on every call. LL as pgx_bernoulli_eval gives it (its accuracy rule; the log flavour's own
 * sum under the same rule).
 * out_table: float64 [1 + n_genes + n_genomes][n_iterations + 1], row-major: row 0 = LL, rows 1.. = P then Q, column 0 =
 * the start point, column k = after iteration k; in the log flavour exp of the solver's variables. out_solver_table (may
 * be NULL): the same shape with the solver's own variables (lp, lq in the log flavour, otherwise equal to out_table).
 * Refused with PGX_ERR_INVALID before anything is launched: n_genes = 0 or n_genomes = 0, unknown flags, not 0 < lo < hi,
 * init_q <= 0, hi x max(hi, init_q) >= 1, a bound or init_q that is not finite, more than 2^20 iterations, and (host
 * entry) an init_p outside [lo, hi] -- so that every 1 - p q the call forms is a positive normal number. n_iterations = 0
 * is valid: one column.
 *   pgx_bernoulli_cd        on the table loaded by pgx_bernoulli_load / pgx_bernoulli_load_resident; HOST pointers
 *   pgx_bernoulli_cd_dev    d_bits: the table in the bitmap layout (pad bits beyond n_genes are ignored); d_init_p (the
 *                           caller keeps it inside [lo, hi]), the result tables and a workspace of
 *                           pgx_bernoulli_cd_workspace_bytes() are DEVICE pointers; plain launches on `stream`, no
 *                           allocation, ONE synchronisation of `stream` at the end (the count of failed solves is read);
 *                           nothing but the results and the workspace is written
 *   pgx_bernoulli_cd_stats  of the context's last call: {evaluations of f, most evaluations in one solve, solves not
 *                           converged, solves} (the two evaluations at the bounds included) */
#define PGX_BERNOULLI_CD_LOGS 1u
size_t pgx_bernoulli_cd_workspace_bytes(uint32_t n_genes, uint32_t n_genomes);
int pgx_bernoulli_cd_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_genomes, const double *d_init_p,
                         double init_q, double lo, double hi, uint32_t n_iterations, uint32_t flags, double *d_out_table,
                         double *d_out_solver_table, void *d_workspace, size_t workspace_bytes, void *stream);
int pgx_bernoulli_cd(pgx_ctx *ctx, const double *init_p, double init_q, double lo, double hi, uint32_t n_iterations,
                     uint32_t flags, double *out_table, double *out_solver_table);
int pgx_bernoulli_cd_stats(pgx_ctx *ctx, uint64_t *out_stats);

/* Monte-Carlo Kolmogorov-Smirnov test of a beta-binomial fit (ks_montecarlo_bbn / draw_bbn, reference
 * pangenome_analysis.py:457-492). A draw is np.random.choice(arange(L), p=probs) of the legacy generator:
 * u = random_sample() from two words (pgx_legacy_uniform_words), value = searchsorted(draw_cdf, u, side='right'), where
 * draw_cdf = probs.cumsum() / its last element (L = sim_limit values, non-decreasing, last = 1). Iteration i takes draws
 * [i n_samples, (i + 1) n_samples) of the stream; its statistic is
 *   ks_sim[i] = max_j | cumsum(hist_i)[j] / n_samples - model_cdf[j] |      (j < L; fp64; nan propagates)
 * with hist_i the histogram of its draws: every step exact or rounded once, so the result is the reference's bits.
 *   pgx_bbn_ks_sim      HOST arrays; the words are generated on the host from key / pos (advanced as numpy would,
 *                       2 n_samples iterations words) and streamed to the device in chunks of about chunk_draws draws
 *                       (whole iterations, at least one; 0 = the library's default; results do not depend on it)
 *   pgx_bbn_ks_sim_dev  d_words: the iterations' 2 n_samples words each, DEVICE pointers, a caller workspace of
 *                       pgx_bbn_workspace_bytes() (zero bytes up to PGX_BBN_LDS_LIMIT values); enqueues on `stream` only
 *   pgx_bbn_draws       the `size` values themselves (int64, as choice returns them), in chunks as above
 * n_samples >= 1 and sim_limit >= 1. */
#define PGX_BBN_LDS_LIMIT 4096u
size_t pgx_bbn_workspace_bytes(uint32_t sim_limit, uint32_t iterations);
int pgx_bbn_ks_sim_dev(pgx_ctx *ctx, const uint32_t *d_words, const double *d_draw_cdf, const double *d_model_cdf,
                       uint32_t sim_limit, uint32_t n_samples, uint32_t iterations, double *d_ks_sim, void *d_workspace,
                       size_t workspace_bytes, void *stream);
int pgx_bbn_ks_sim(pgx_ctx *ctx, const double *draw_cdf, const double *model_cdf, uint32_t sim_limit, uint32_t n_samples,
                   uint32_t iterations, uint32_t *mt_key, int32_t *mt_pos, uint64_t chunk_draws, double *out_ks_sim);
int pgx_bbn_draws(pgx_ctx *ctx, const double *draw_cdf, uint32_t sim_limit, uint64_t size, uint32_t *mt_key,
                  int32_t *mt_pos, uint64_t chunk_draws, int64_t *out_idx);

/* Formal concept decomposition (formal_concept_decomposition / compute_concept_coverage, reference fcd.py:15-138,
 * :199-219): the binary table is covered greedily with all-ones blocks ("concepts": a set of rows x a set of genomes).
 * U = the ones not covered yet (a working copy on the device; the table itself is never written). While ones are left
 * and fewer than `limit` concepts exist: acc = the rows with a one in U, live = the columns with a one in U, then, as long
 * as it raises the score, the live column with the largest score (the lowest index among equals) joins the concept and
 * acc &= that column of U (of the table under PGX_FCD_OVERLAP). With k columns merged and cnt[c] = popcount(U[:, c] & acc):
 *   default               score[c] = (k + 1) * cnt[c]                                        (int64)
 *   PGX_FCD_DIM_BALANCE   score[c] = dim_factors[k] * (double)cnt[c]   (one float64 multiply; dim_factors: HOST array of
 *                         n_genomes doubles, the caller's ((k + 1) ** (log(n_rows) / log(n_genomes))); ignored under overlap)
 *   PGX_FCD_OVERLAP       score[c] = cnt[c] + sum over the rows r of table[:, c] & acc of w[r],  w[r] = the ones U has
 *                         in row r among the merged columns                                   (int64)
 * The concept is (rows of acc ascending, columns in the order they joined); its block is cleared in U.
 * Two calls: one of pgx_fcd / pgx_fcd_resident / pgx_fcd_dev runs the decomposition and keeps the concepts in the
 * context; out_info says how many there are; pgx_fcd_fetch copies them out -- out_rows [n_row_entries] and out_cols
 * [n_col_entries] hold the concepts' rows / columns end to end, concept i owns [offsets[i], offsets[i + 1]) of each
 * (n_concepts + 1 offsets), out_left[i] = the ones still uncovered after concept i -- until the next run on the context.
 *   pgx_fcd            HOST COO coordinates of the table; out_duplicates as pgx_presence_bitmap (may be NULL): with
 *                      duplicate coordinates nothing is decomposed (out_info all zero)
 *   pgx_fcd_resident   the table is read from the bitmap a pipeline left resident (pgx_bitmap_from_clusters), which is not
 *                      modified: row i / column j of the table = row row_map[i] / column col_map[j] of it (col_map NULL:
 *                      column j). A stale token fails with PGX_ERR_INVALID.
 *   pgx_fcd_dev        d_bits: the table in the bitmap layout above (DEVICE, 16-byte aligned, pad bits zero, not written),
 *                      a caller workspace of pgx_fcd_workspace_bytes(). Unlike the other *_dev entry points it is not
 *                      graph-capturable: every step reads 16 bytes back, so it synchronises `stream` (plain launches on
 *                      that stream only; at most n_genomes steps per concept and `limit` concepts).
 * A concept that clears nothing (the reference would loop for ever) fails with PGX_ERR_INTERNAL.
 *   pgx_fcd_coverage   out_cleared[i] = the ones concept i clears when the given concepts (layout as pgx_fcd_fetch's; no
 *                      column twice in one concept) are cleared from the table one after the other with the same kernel;
 *                      out_ones = the ones of the table.
 *
 * Comparing two concept lists (compute_concept_list_similarity, reference fcd.py:168-196). A concept is a SET of rows and
 * a set of columns (an index listed twice counts once); O[i][j] = |rows1[i] & rows2[j]| * |cols1[i] & cols2[j]| are the
 * cells concept i of F1 and concept j of F2 share. For i = 0 .. k, k = min(n1, n2): concept i takes the unmatched j with
 * the largest O[i][j], the lowest j among equals (an overlap of 0 still takes one); match[i] = j, overlap[i] = O[i][j],
 * total = their sum. The matrix is formed 256 concepts of F1 at a time and never as a whole, unless the caller asks for
 * it: out_matrix / d_matrix (n1 x n2, row-major, rows beyond k included) may be NULL.
 *   pgx_fcd_match      HOST lists in the layout of pgx_fcd_fetch (n + 1 offsets, the first 0); an offset out of order or an
 *                      index outside the table fails with PGX_ERR_INVALID before anything runs. Synchronises the
 *                      context's stream.
 *   pgx_fcd_match_dev  DEVICE bit masks, concept-major: the row mask of concept i is the pgx_bitmap_stride_words(n_rows)
 *                      words at i * stride (bit r & 63 of word r >> 6 = row r), column masks likewise with n_cols; 16-byte
 *                      aligned, pad bits zero, not written. d_match int64[k], d_overlap uint64[k], d_total uint64, a
 *                      workspace of pgx_fcd_match_workspace_bytes() (16-byte aligned). No allocation, no synchronisation,
 *                      plain launches on `stream` only: graph-capturable. Nothing the caller passes is used as an index.
 * Both refuse (PGX_ERR_INVALID) n_rows, n_cols, n1 or n2 >= 2^31 and n_rows * n_cols * k >= 2^63 (total could overflow);
 * pgx_fcd_match_workspace_bytes returns 0 for those. n1 == 0 or n2 == 0: total = 0 and no kernel runs. The workspace is
 * (each part rounded up to 256 bytes; stride_r/c = pgx_bitmap_stride_words(n_rows / n_cols)):
 *   masks of F2  n2 * stride_r * 8 + n2 * stride_c * 8     masks of a block of F1  256 * stride_r * 8 + 256 * stride_c * 8
 *   a block of O  256 * n2 * 8                             unmatched flags  n2           (the result record is d_total) */
#define PGX_FCD_OVERLAP 1u
#define PGX_FCD_DIM_BALANCE 2u
typedef struct pgx_fcd_info_t {
    uint64_t n_concepts;
    uint64_t n_row_entries;    /* sum of the concepts' row counts */
    uint64_t n_col_entries;    /* sum of the concepts' column counts */
    uint64_t steps;            /* score evaluations (one masked popcount of every live column each) */
    uint64_t ones_total;       /* ones of the table */
    uint64_t ones_left;        /* of those, not covered (0 unless `limit` stopped the decomposition) */
} pgx_fcd_info_t;
size_t pgx_fcd_workspace_bytes(uint32_t n_rows, uint32_t n_genomes);
int pgx_fcd(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
            uint32_t n_genomes, uint64_t limit, uint32_t flags, const double *dim_factors, pgx_fcd_info_t *out_info,
            uint64_t *out_duplicates);
int pgx_fcd_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, const int32_t *col_map, uint32_t n_rows,
                     uint32_t n_genomes, uint64_t limit, uint32_t flags, const double *dim_factors, pgx_fcd_info_t *out_info);
int pgx_fcd_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, uint64_t limit, uint32_t flags,
                const double *dim_factors, void *d_workspace, size_t workspace_bytes, void *stream, pgx_fcd_info_t *out_info);
int pgx_fcd_fetch(pgx_ctx *ctx, int32_t *out_rows, uint64_t *out_row_offsets, int32_t *out_cols, uint64_t *out_col_offsets,
                  uint64_t *out_left);
int pgx_fcd_coverage(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
                     uint32_t n_genomes, const int32_t *concept_rows, const uint64_t *row_offsets, const int32_t *concept_cols,
                     const uint64_t *col_offsets, uint64_t n_concepts, uint64_t *out_cleared, uint64_t *out_ones,
                     uint64_t *out_duplicates);
size_t pgx_fcd_match_workspace_bytes(uint32_t n_rows, uint32_t n_cols, uint64_t n1, uint64_t n2);
int pgx_fcd_match(pgx_ctx *ctx, uint32_t n_rows, uint32_t n_cols, const int32_t *rows1, const uint64_t *row_off1,
                  const int32_t *cols1, const uint64_t *col_off1, uint64_t n1, const int32_t *rows2, const uint64_t *row_off2,
                  const int32_t *cols2, const uint64_t *col_off2, uint64_t n2, int64_t *out_match, uint64_t *out_overlap,
                  uint64_t *out_total, uint64_t *out_matrix);
int pgx_fcd_match_dev(pgx_ctx *ctx, const uint64_t *d_row_masks1, const uint64_t *d_col_masks1, uint64_t n1,
                      const uint64_t *d_row_masks2, const uint64_t *d_col_masks2, uint64_t n2, uint32_t n_rows,
                      uint32_t n_cols, int64_t *d_match, uint64_t *d_overlap, uint64_t *d_total, uint64_t *d_matrix,
                      void *d_workspace, size_t workspace_bytes, void *stream);

/* The association screen (reference sparse_utils.py:73-109 compress_rows_spmatrix, ml_pipelines.py:349-388
 * contingency_tables_from_sparse, :233-284 prepare_amr_case_data) on the table restricted to n_selected genomes
 * (col_map[j] = the genome that is column j of the selection; NULL = all of them in order, n_selected = n_genomes):
 *   incidence[r]      genomes of the selection row r is present in
 *   tp[t][r]          of those, the genomes whose bit is set in mask t: masks holds n_targets x ceil(n_selected / 64)
 *                     (at least 1) words, bit j % 64 of word j / 64 = column j of the selection; pad bits are ignored
 *   PGX_ASSOC_BLOCKS  rows present in the same genomes of the selection form a block; blocks are numbered by their first
 *                     row ascending: block_of_row[r] (n_rows entries), rep_row[b] = the first row of block b (room for
 *                     n_rows entries, *out_n_blocks used). All rows without a genome form one block, unless
 *   PGX_ASSOC_DROP_EMPTY  those rows take no part (block_of_row = -1): the blocks of the table without its empty rows.
 * The result does not depend on the order in which the device's waves run. The bitmap is never written. n_selected = 0
 * (col_map may then be NULL) is the table without a column: incidence and tp are 0 and all rows are empty.
 * PGX_ASSOC_NARROW_HASH (a test seam) keeps only the low 3 bits of every hash: same results, every probe collides.
 *   pgx_assoc            HOST COO coordinates of the table; out_duplicates as pgx_presence_bitmap (may be NULL): with
 *                        duplicate coordinates nothing is computed
 *   pgx_assoc_resident   the table is read from the bitmap a pipeline left resident (pgx_bitmap_from_clusters): row i of
 *                        the table = row row_map[i] of it. A stale token fails with PGX_ERR_INVALID.
 *   pgx_assoc_dev        d_bits: the table in the bitmap layout above; d_col_map, d_masks and the four result arrays are
 *                        DEVICE pointers, the workspace is the caller's (pgx_assoc_workspace_bytes(), 16-byte aligned).
 *                        Plain launches on `stream`, which is synchronised once at the end (status and block count back).
 * out_tp / masks may be NULL with n_targets = 0; the block arrays may be NULL without PGX_ASSOC_BLOCKS. n_rows < 2^30. */
#define PGX_ASSOC_BLOCKS 1u
#define PGX_ASSOC_DROP_EMPTY 2u
#define PGX_ASSOC_NARROW_HASH 4u   /* keep only the low 3 bits of every hash: same results, every probe collides */
size_t pgx_assoc_workspace_bytes(uint32_t n_rows, uint32_t n_selected);
int pgx_assoc(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
              uint32_t n_genomes, const int32_t *col_map, uint32_t n_selected, const uint64_t *masks, uint32_t n_targets,
              uint32_t flags, uint32_t *out_tp, uint32_t *out_incidence, int32_t *out_block_of_row, int32_t *out_rep_row,
              uint32_t *out_n_blocks, uint64_t *out_duplicates);
int pgx_assoc_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, uint32_t n_rows, uint32_t n_genomes,
                       const int32_t *col_map, uint32_t n_selected, const uint64_t *masks, uint32_t n_targets, uint32_t flags,
                       uint32_t *out_tp, uint32_t *out_incidence, int32_t *out_block_of_row, int32_t *out_rep_row,
                       uint32_t *out_n_blocks);
int pgx_assoc_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, const int32_t *d_col_map,
                  uint32_t n_selected, const uint64_t *d_masks, uint32_t n_targets, uint32_t flags, uint32_t *d_tp,
                  uint32_t *d_incidence, int32_t *d_block_of_row, int32_t *d_rep_row, void *d_workspace,
                  size_t workspace_bytes, void *stream, uint32_t *out_n_blocks);

/* A bagged ensemble of linear SVMs on the table's genomes (reference ml_pipelines.py:21-98 evaluate_model with sklearn's
 * BaggingClassifier(LinearSVC)): the samples are the n_genomes genomes, the features the n_rows rows of the bitmap above.
 *   masks              n_masks feature masks, each pgx_bitmap_stride_words(n_rows) words in the layout of one genome's bits
 *                      (bit r & 63 of word r >> 6 = row r takes part); bits at or behind n_rows are ignored
 *   sub-problem p      mask_of_problem[p] (0 .. n_masks - 1), C[p], multiplicity[p * n_genomes + i] = how often genome i
 *                      was drawn into p's training set (bootstrap draws folded; 0 = not in it); sub-problems that name the
 *                      same mask share its Gram matrix
 *   labels[i]          0 or 1, read as y_i = -1 / +1; one vector for all sub-problems
 * Sub-problem p is LinearSVC(penalty = l2, loss = squared_hinge, dual, fit_intercept, intercept_scaling = 1) on the drawn
 * genomes, solved in its dual with the copies of a genome summed into one variable b_i >= 0 (genomes with m_i > 0):
 *   min 1/2 b'Qb - sum b_i,   Q_ij = y_i y_j (K_ij + 1) + [i == j] / (2 C m_i),   K_ij = popcount(bits_i & bits_j & mask)
 * Q is positive definite (smallest eigenvalue >= 1 / (2 C max m)), the optimum unique. The solver is pinned: greedy dual
 * coordinate descent in double precision. g = Qb - 1 is kept; PG_i = g_i where b_i > 0, else min(g_i, 0); the i of largest
 * |PG_i| (ties: the smallest i) takes the step d = max(-b_i, -g_i / Q_ii), b_i += d, g += d Q[:, i]; when max |PG_i| <= tol,
 * g is recomputed from b in one product in ascending order of i and the test repeated, the descent going on if it fails.
 * More than max_steps steps (0 = 1,000,000 + 2,000 n_genomes) fail the call with PGX_ERR_INTERNAL, the outputs then
 * being unspecified. Gram entries are exact integers, every sum runs in a fixed order, there is no floating-point atomic:
 * the same inputs give the same bits on every call. At the end |PG_i| <= tol for the recomputed g, hence
 * every b_i, coef and the intercept lie within 2 C max(m) n tol of the optimum's.
 *   beta       [n_problems x n_genomes]  b_i, 0 where m_i = 0
 *   coef       [n_problems x n_rows]     sum_i b_i y_i bit(i, r) for the rows r of the mask, 0 outside it
 *   intercept  [n_problems]              sum_i b_i y_i
 *   decision   [n_problems x n_genomes]  sum_i b_i y_i (K_si + 1) for EVERY genome s of the table, drawn or not
 *   steps      [n_problems]              coordinate steps taken
 * Refused with PGX_ERR_INVALID: n_rows, n_genomes, n_masks or n_problems = 0, tol not finite and positive, a mask index
 * out of range, a mask without a bit below n_rows, a C that is not finite and positive, a label other than 0 or 1, a
 * sub-problem whose drawn genomes carry one class only. n_genomes above PGX_SVM_MAX_GENOMES: PGX_ERR_CAPACITY (there is
 * no slower path). n_rows < 2^30, n_masks and n_problems <= 65535.
 *   pgx_svm_bag        HOST COO coordinates of the table and host arrays; everything above is checked before anything
 *                      is launched; then a coordinate out of range or given twice is PGX_ERR_INVALID as well.
 *   pgx_svm_bag_dev    d_bits: the table in the bitmap layout above (never written); masks, sub-problems, labels and the
 *                      five results are DEVICE pointers, the workspace the caller's (pgx_svm_bag_workspace_bytes(),
 *                      16-byte aligned: the Gram matrices, n_masks x n_genomes^2 x 4 bytes, and a status word). The
 *                      scalars are checked before anything is launched; the arrays are checked on the device (a broken
 *                      sub-problem is skipped, the outputs are then unspecified). Plain launches on `stream`, which is
 *                      synchronised once at the end (the status back). Nothing is allocated. */
#define PGX_SVM_MAX_GENOMES 4096u
size_t pgx_svm_bag_workspace_bytes(uint32_t n_rows, uint32_t n_genomes, uint32_t n_masks);
int pgx_svm_bag(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
                uint32_t n_genomes, const uint64_t *masks, uint32_t n_masks, const int32_t *mask_of_problem, const double *C,
                const uint16_t *multiplicity, uint32_t n_problems, const uint8_t *labels, double tol, uint32_t max_steps,
                double *out_beta, double *out_coef, double *out_intercept, double *out_decision, uint32_t *out_steps);
int pgx_svm_bag_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, const uint64_t *d_masks,
                    uint32_t n_masks, const int32_t *d_mask_of_problem, const double *d_C, const uint16_t *d_multiplicity,
                    uint32_t n_problems, const uint8_t *d_labels, double tol, uint32_t max_steps, double *d_beta,
                    double *d_coef, double *d_intercept, double *d_decision, uint32_t *d_steps, void *d_workspace,
                    size_t workspace_bytes, void *stream);

/* Runs of allele rows (reference pangenome.py:1246-1330 validate_gene_table / validate_gene_table_dense, :1812-1889
 * extract_dominant_alleles): run r is the allele rows [run_start[r], run_start[r + 1]) of the allele table -- run_start holds
 * n_runs + 1 entries, starts at 0, never decreases and ends at or below n_alleles; a run may be empty, rows behind the last
 * run belong to none. gene_of_run[r] is the row of the gene table run r is compared with, -1 = none (its gene bits are 0);
 * gene_of_run NULL (or, for the device entry, no gene bitmap) = -1 everywhere. All three tables have n_genomes genomes.
 *   derived          bitmap of n_runs rows in the layout above (n_genomes x pgx_bitmap_stride_words(n_runs) words): bit
 *                    (r, j) is set iff genome j has a bit in any allele row of run r; pad bits are 0
 *   diff             the same shape: derived XOR (bit gene_of_run[r] of the gene table, for every genome)
 *   diff_per_genome  [n_genomes] set bits of the genome's words of diff;   diff_per_run [n_runs] set bits of row r of diff
 *   total            [n_runs] uint64: the sum over the run's rows of the genomes that hold the row
 *   best_allele      [n_runs] the first row of the run with the largest such count (a later row replaces an earlier one
 *                    only with a strictly greater count), -1 for an empty run;   best_count [n_runs] that count (0 if empty)
 * Every output pointer may be NULL; what is not asked for is not computed. The result does not depend on the order in which
 * the device's waves run (no atomics on a result). Bits of the allele bitmap at or beyond n_alleles are masked, not trusted.
 *   pgx_allele_runs      HOST COO coordinates of the allele table and (used only with gene_of_run) of the gene table;
 *                        out_duplicates (2 x uint64: allele table, gene table; may be NULL) as pgx_presence_bitmap: with
 *                        duplicate coordinates in either nothing is computed. run_start / gene_of_run that break the rules
 *                        above, or n_runs = 0 with an output requested, fail with PGX_ERR_INVALID before anything is launched.
 *   pgx_allele_runs_dev  d_allele_bits, d_gene_bits (may be NULL), d_run_start, d_gene_of_run (may be NULL), the result
 *                        arrays and the workspace (pgx_allele_runs_workspace_bytes(), 16-byte aligned) are the caller's
 *                        DEVICE pointers. Plain launches on `stream`, which is synchronised once at the end. The run arrays
 *                        are checked on the device: the kernels clamp what they read (no access out of bounds), and arrays
 *                        that break the rules fail with PGX_ERR_INVALID after the launches, the outputs then being unspecified.
 * n_alleles, n_runs, n_genes, n_genomes < 2^31. */
size_t pgx_allele_runs_workspace_bytes(uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes);
int pgx_allele_runs(pgx_ctx *ctx, const int32_t *allele_rows, const int32_t *allele_genomes, uint64_t n_allele_records,
                    uint32_t n_alleles, const int32_t *gene_rows, const int32_t *gene_genomes, uint64_t n_gene_records,
                    uint32_t n_genes, uint32_t n_genomes, const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run,
                    uint64_t *out_derived, uint64_t *out_diff, uint32_t *out_diff_per_genome, uint32_t *out_diff_per_run,
                    uint64_t *out_total, int32_t *out_best_allele, uint32_t *out_best_count, uint64_t *out_duplicates);
int pgx_allele_runs_dev(pgx_ctx *ctx, const uint64_t *d_allele_bits, uint32_t n_alleles, const uint64_t *d_gene_bits,
                        uint32_t n_genes, uint32_t n_genomes, const uint32_t *d_run_start, uint32_t n_runs,
                        const int32_t *d_gene_of_run, uint64_t *d_derived, uint64_t *d_diff, uint32_t *d_diff_per_genome,
                        uint32_t *d_diff_per_run, uint64_t *d_total, int32_t *d_best_allele, uint32_t *d_best_count,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/* Core / dominant allele selection (reference core_genome.py:7-26 create_core_genes_fasta, allele_identification.py:7-20
 * create_alleles_fasta): the runs, tables and rules of "Runs of allele rows" above, and thresholds[n_thresholds] (uint32,
 * 1 <= n_thresholds <= 32, in any order, repeats allowed).
 *   gene_count   [n_runs] uint32: set bits of row gene_of_run[r] of the gene table; 0 for -1, and 0 everywhere without
 *                gene_of_run or (device entry) without a gene bitmap
 *   best_allele  [n_runs] int32 / best_count [n_runs] uint32: as pgx_allele_runs gives them (the same code)
 *   mask         [n_runs] uint32: bit t is set iff the run is eligible and gene_count[r] >= thresholds[t]; a run is eligible
 *                iff best_allele[r] >= 0 and gene_of_run[r] >= 0 -- with gene_of_run NULL, iff best_allele[r] >= 0
 *   selected     [n_thresholds x n_runs] int32, n_selected [n_thresholds] uint32: row t of selected holds best_allele[r] of
 *                the runs with bit t, in ascending r; entries at and beyond n_selected[t] are NOT written
 * Every output pointer may be NULL; what is not asked for is not computed. No atomics on a result: the same inputs give
 * the same bytes whatever order the device's waves run in.
 *   pgx_core_select      HOST COO coordinates of both tables (the gene table is used only with gene_of_run), host run
 *                        arrays, thresholds and results; out_duplicates as pgx_allele_runs (2 x uint64, may be NULL): with
 *                        duplicate coordinates in either table nothing is computed. Run arrays that break the rules,
 *                        n_thresholds outside 1..32, or n_runs = 0 with an output requested fail with PGX_ERR_INVALID
 *                        before anything is launched.
 *   pgx_core_select_dev  the bitmaps, run arrays, thresholds, results and the workspace
 *                        (pgx_core_select_workspace_bytes(), 16-byte aligned) are the caller's DEVICE pointers. Plain
 *                        launches on `stream`, which is synchronised once at the end. The run arrays are checked on the
 *                        device: the kernels clamp what they read (a gene row out of range counts as none), and arrays that
 *                        break the rules fail with PGX_ERR_INVALID after the launches, the outputs then being unspecified.
 * pgx_core_select_block(): the runs one workgroup takes. n_alleles, n_runs, n_genes, n_genomes < 2^31. */
uint32_t pgx_core_select_block(void);
size_t pgx_core_select_workspace_bytes(uint32_t n_alleles, uint32_t n_genes, uint32_t n_runs);
int pgx_core_select(pgx_ctx *ctx, const int32_t *allele_rows, const int32_t *allele_genomes, uint64_t n_allele_records,
                    uint32_t n_alleles, const int32_t *gene_rows, const int32_t *gene_genomes, uint64_t n_gene_records,
                    uint32_t n_genes, uint32_t n_genomes, const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run,
                    const uint32_t *thresholds, uint32_t n_thresholds, uint32_t *out_gene_count, int32_t *out_best_allele,
                    uint32_t *out_best_count, uint32_t *out_mask, int32_t *out_selected, uint32_t *out_n_selected,
                    uint64_t *out_duplicates);
int pgx_core_select_dev(pgx_ctx *ctx, const uint64_t *d_allele_bits, uint32_t n_alleles, const uint64_t *d_gene_bits,
                        uint32_t n_genes, uint32_t n_genomes, const uint32_t *d_run_start, uint32_t n_runs,
                        const int32_t *d_gene_of_run, const uint32_t *d_thresholds, uint32_t n_thresholds,
                        uint32_t *d_gene_count, int32_t *d_best_allele, uint32_t *d_best_count, uint32_t *d_mask,
                        int32_t *d_selected, uint32_t *d_n_selected, void *d_workspace, size_t workspace_bytes, void *stream);

/* Exact search for fixed-length keys in a text (reference pangenome.py:1573-1647 validate_proximal_table_direct, which slides a
 * window over every contig): text is text_bytes raw bytes, keys n_keys x window raw bytes, found [n_keys] uint8:
 *   found[k] = 1 iff the window bytes of key k equal text[i .. i + window) for some 0 <= i <= text_bytes - window, else 0.
 * Bytes are compared as bytes (no case folding, no alphabet, values >= 0x80 allowed); equal keys given twice are both
 * flagged. Hashes only decide where to look -- a key is flagged after its bytes have been compared -- so the result is exact;
 * PGX_SCAN_NARROW_HASH (a test seam) keeps only the low 3 bits of every hash: same results, every probe collides.
 * window outside 1..1024, text_bytes >= 2^32, n_keys >= 2^24 or unknown flags fail with PGX_ERR_INVALID before anything is
 * launched or written. n_keys = 0 does nothing; a text shorter than window (text_bytes = 0 included) zeroes found.
 *   pgx_window_scan      HOST pointers; the device buffers stay in the context between calls
 *   pgx_window_scan_dev  d_text, d_keys, d_found and the workspace (pgx_window_scan_workspace_bytes(), 16-byte aligned; 0 for
 *                        sizes that are refused) are the caller's DEVICE pointers. Plain launches on `stream`, which is
 *                        synchronised once at the end; text and keys are not written, nothing outside found and the
 *                        workspace is.
 * pgx_window_scan_tile(): the text positions one workgroup takes at a time. */
#define PGX_SCAN_NARROW_HASH 1u   /* keep only the low 3 bits of every hash: same results, every probe collides */
uint32_t pgx_window_scan_tile(void);
size_t pgx_window_scan_workspace_bytes(uint64_t text_bytes, uint32_t n_keys, uint32_t window);
int pgx_window_scan(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint8_t *keys, uint32_t n_keys,
                    uint32_t window, uint32_t flags, uint8_t *out_found);
int pgx_window_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_keys, uint32_t n_keys,
                        uint32_t window, uint32_t flags, uint8_t *d_found, void *d_workspace, size_t workspace_bytes,
                        void *stream);

/* Exact look-up of whole byte strings in a set of byte strings (reference pangenome.py:1418-1546 validate_table_against_fasta,
 * which does one SHA-256 and one dict look-up per FASTA record). String i of a blob is the bytes [offsets[i], offsets[i + 1]):
 * offsets holds n + 1 entries that never decrease, offsets[0] may be non-zero, the blob is the bytes [0, offsets[n]) and may
 * start at any address; nothing outside it is read. The empty string is a legal key and a legal query. Bytes are compared
 * as bytes (values >= 0x80 allowed); two strings are equal iff they have the same length and the same bytes.
 *   first[k] = the smallest index of a key equal to key k (k itself for the first of its kind)
 *   last[q]  = the largest index of a key equal to query q, -1 for none
 * Both are a minimum / maximum over a set: the same input gives the same output on every call. Hashes only decide where to
 * look -- an index is reported after lengths and bytes have been compared -- so the result is exact (the reference compares
 * SHA-256 digests; the two agree unless SHA-256 collides). PGX_DICT_NARROW_HASH (a test seam) keeps only the low 3 bits of
 * every hash: same results, every probe collides, the look-up is then quadratic in the number of keys.
 * n_keys >= 2^24, n_queries >= 2^31, a blob of 2^32 bytes or more or decreasing offsets (host entries), unknown flags and
 * too small a workspace fail with PGX_ERR_INVALID before anything is launched or written. n_keys = 0 gives every query -1; n_queries = 0 does nothing.
 *   pgx_dict_load       HOST pointers: keeps the keys and their table in the context, replacing an earlier set; out_first
 *                       [n_keys] may be NULL
 *   pgx_dict_query      HOST pointers: searches the set loaded last (PGX_ERR_INVALID without one), with the flags it was
 *                       loaded with; any number of calls per load
 *   pgx_dict_match_dev  keys, queries, offsets (8-byte aligned), outputs (d_out_first may be NULL) and the workspace
 *                       (pgx_dict_workspace_bytes(), 16-byte aligned; 0 for sizes that are refused) are the caller's DEVICE
 *                       pointers. Plain launches on `stream`, which is synchronised once at the end; inputs are not written,
 *                       nothing outside the outputs and the workspace is. Device offsets are not checked, and the LAST offset is taken
 *                       as the blob's size: d_keys must hold d_key_offsets[n_keys] bytes and d_queries
 *                       d_query_offsets[n_queries] bytes. The kernels clamp every string into [0, last offset), so with a
 *                       last offset inside the caller's allocation nothing outside it is read whatever the other offsets
 *                       hold (the result for broken offsets is unspecified); a last offset beyond the allocation is the
 *                       caller's error and is not caught.
 * pgx_dict_group_bytes(): the bytes of a string the lanes that share it take per step. */
#define PGX_DICT_NARROW_HASH 1u   /* keep only the low 3 bits of every hash: same results, every probe collides */
uint32_t pgx_dict_group_bytes(void);
size_t pgx_dict_workspace_bytes(uint64_t key_bytes, uint32_t n_keys);
int pgx_dict_load(pgx_ctx *ctx, const uint8_t *keys, const uint64_t *key_offsets, uint32_t n_keys, uint32_t flags,
                  int32_t *out_first);
int pgx_dict_query(pgx_ctx *ctx, const uint8_t *queries, const uint64_t *query_offsets, uint32_t n_queries,
                   int32_t *out_last);
int pgx_dict_match_dev(pgx_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_key_offsets, uint32_t n_keys,
                       const uint8_t *d_queries, const uint64_t *d_query_offsets, uint32_t n_queries, uint32_t flags,
                       int32_t *d_out_first, int32_t *d_out_last, void *d_workspace, size_t workspace_bytes, void *stream);

/* Two sets of rows per genome, compared: A and B are bitmaps in the layout of pgx_presence_bitmap (n_genomes x
 * pgx_bitmap_stride_words(n_rows) words, row r = bit r & 63 of word r >> 6 of the genome's words);
 *   a_only[g] = rows of genome g set in A and not in B,   b_only[g] = rows set in B and not in A.
 * Bits at or beyond n_rows are masked, not trusted. n_rows, n_genomes < 2^31; n_genomes = 0 does nothing.
 *   pgx_genome_sets_diff      HOST COO coordinates of both sets; a coordinate given twice counts once, one out of range
 *                             fails with PGX_ERR_INVALID
 *   pgx_genome_sets_diff_dev  the caller's DEVICE bitmaps and outputs; one launch on `stream`, which is then synchronised */
int pgx_genome_sets_diff(pgx_ctx *ctx, const int32_t *a_rows, const int32_t *a_genomes, uint64_t n_a, const int32_t *b_rows,
                         const int32_t *b_genomes, uint64_t n_b, uint32_t n_rows, uint32_t n_genomes, uint32_t *out_a_only,
                         uint32_t *out_b_only);
int pgx_genome_sets_diff_dev(pgx_ctx *ctx, const uint64_t *d_a_bits, const uint64_t *d_b_bits, uint32_t n_rows,
                             uint32_t n_genomes, uint32_t *d_a_only, uint32_t *d_b_only, void *stream);

/* The two device steps of the proximal (5'/3' UTR) pangenome builders (reference pangenome.py:900-1184).
 *
 * cut: text is text_bytes raw bytes; window i is the length[i] bytes at start[i], and its piece of the output is
 * out[out_offsets[i] .. out_offsets[i] + length[i]), out_offsets being the exclusive prefix sum of the lengths (n + 1 entries).
 *   reverse[i] == 0:  out[out_offsets[i] + k] = text[start[i] + k]; any byte is allowed, bad[i] = 0
 *   reverse[i] != 0:  out[out_offsets[i] + k] = comp(text[start[i] + length[i] - 1 - k]), comp mapping
 *                     ACGTWSRYMKNacgtwsrymkn to TGCAWSYRKMNtgcawsyrkmn; any other byte gives the output byte 0 and bad[i] = 1
 * Zero-length windows are legal, windows may overlap or repeat, n = 0 does nothing. text_bytes >= 2^32 and n >= 2^24 fail
 * with PGX_ERR_INVALID before anything is launched or written.
 *   pgx_prox_cut      HOST pointers; computes the offsets itself (out holds the sum of the lengths, out_bad n bytes). A
 *                     window that leaves [0, text_bytes) or an output of 2^32 bytes or more is refused the same way.
 *   pgx_prox_cut_dev  the caller's DEVICE pointers (d_start and d_out_offsets 8-byte aligned, d_length 4-byte aligned; text
 *                     and output may start at any address). One launch on `stream`, which is then synchronised; no
 *                     workspace. The windows are not checked: every read is clamped into the text (a window is cut short at
 *                     its end), and d_out must hold d_out_offsets[i] + length[i] bytes for every window.
 * pgx_prox_cut_group_bytes(): the output bytes the lanes that share a window write per step.
 *
 * group: record i is the string i of a blob with n + 1 offsets (the conventions of pgx_dict_load) and a gene id
 * 0 <= gene[i] < 2^24. Two records are equal iff they have the same gene, the same length and the same bytes.
 *   first[i]    = the smallest j with record j equal to record i
 *   variant[i]  = the number of j with first[j] == j, gene[j] == gene[i] and j < first[i]: the number a dictionary per gene
 *                 gives a string when the records are entered in index order
 *   *n_distinct = the number of i with first[i] == i
 * All three are functions of the input alone: the same input gives the same bytes on every call. Hashes only decide where to
 * look -- a j is reported after gene, length and bytes have been compared. PGX_PROX_NARROW_HASH (a test seam) keeps only the
 * low 3 bits of every hash: same results, every probe collides. n >= 2^24, a blob of 2^32 bytes or more, decreasing offsets
 * or a gene outside [0, 2^24) (host entry), unknown flags and too small a workspace fail with PGX_ERR_INVALID before anything
 * is launched or written. n = 0 sets *n_distinct to 0.
 *   pgx_prox_group      HOST pointers; the device buffers stay in the context between calls
 *   pgx_prox_group_dev  the caller's DEVICE pointers (offsets 8-byte aligned, the int32 arrays 4-byte aligned) and workspace
 *                       (pgx_prox_group_workspace_bytes(), 16-byte aligned; 0 for an n that is refused). Plain launches on
 *                       `stream`, which is synchronised once at the end; inputs are not written, nothing outside the outputs
 *                       and the workspace is. Offsets and genes are not checked: strings are clamped into [0, last offset)
 *                       and only the low 24 bits of a gene order the records, so nothing outside the caller's buffers is
 *                       touched, the result for broken input being unspecified.
 * pgx_prox_group_tile(): the records one wave takes per pass of the sort by gene. */
#define PGX_PROX_NARROW_HASH 1u   /* keep only the low 3 bits of every hash: same results, every probe collides */
uint32_t pgx_prox_cut_group_bytes(void);
uint32_t pgx_prox_group_tile(void);
size_t pgx_prox_group_workspace_bytes(uint32_t n);
int pgx_prox_cut(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint64_t *start, const uint32_t *length,
                 const uint8_t *reverse, uint32_t n, uint8_t *out, uint8_t *out_bad);
int pgx_prox_cut_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_start,
                     const uint32_t *d_length, const uint8_t *d_reverse, const uint64_t *d_out_offsets, uint32_t n,
                     uint8_t *d_out, uint8_t *d_bad, void *stream);
int pgx_prox_group(pgx_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, const int32_t *gene, uint32_t n,
                   uint32_t flags, int32_t *out_first, int32_t *out_variant, uint32_t *out_n_distinct);
int pgx_prox_group_dev(pgx_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, const int32_t *d_gene, uint32_t n,
                       uint32_t flags, int32_t *d_first, int32_t *d_variant, uint32_t *d_n_distinct, void *d_workspace,
                       size_t workspace_bytes, void *stream);

/* Ordered de-duplication of rows of ids and the plurality vote of runs of rows: the device step of extract_annotations
 * (reference pangenome.py:1702-1810, one OrderedDict.fromkeys per names line and one collections.Counter per gene).
 * Row r holds the ids tok[row_off[r] .. row_off[r + 1]) (n_rows + 1 offsets, row_off[0] = 0, n_tokens = row_off[n_rows]); ids
 * are at least 0 and equal ids stand for equal strings. Run u is the rows [run_off[u], run_off[u + 1]) (n_runs + 1 offsets,
 * run_off[0] = 0, run_off[n_runs] = n_rows, strictly increasing).
 *   keep[p]    = 1 iff no earlier position of p's row holds the id at p, else 0 (n_tokens bytes)
 *   L(r)       = the kept ids of row r in order: the empty list for an empty row, and two empty lists are equal
 *   count(r)   = the rows r' of r's run with L(r') == L(r), element by element
 *   winner[u]  = the smallest row of run u with the largest count; votes[u] = that count (n_runs entries each)
 *   differs[r] = 1 iff L(r) != L(winner[run of r]), else 0 (n_rows bytes)
 * All four are functions of the input alone: the same input gives the same bytes on every call. Hashes only decide where to
 * look -- two lists are called equal after their lengths and every element have been compared. PGX_ANNOT_NARROW_HASH (a test
 * seam) keeps only the low 3 bits of every hash: same results, every probe collides. n_rows >= 2^24, n_tokens >= 2^31,
 * offsets that decrease or do not start at 0, an empty run or runs that do not cover exactly the rows, a negative id (host
 * entry), unknown flags and too small a workspace fail with PGX_ERR_INVALID before anything is launched or written.
 * n_rows = 0 (with n_runs = 0) does nothing.
 *   pgx_annot_vote      HOST pointers; the device buffers stay in the context between calls
 *   pgx_annot_vote_dev  the caller's DEVICE pointers (row_off 8-byte aligned, tok, run_off, winner and votes 4-byte aligned),
 *                       n_tokens given by the caller, and workspace (pgx_annot_vote_workspace_bytes(), 16-byte aligned; 0 for
 *                       sizes that are refused). Plain launches on `stream`, which is synchronised once at the end; inputs are
 *                       not written, nothing outside the outputs and the workspace is. Offsets and ids are not checked: rows
 *                       are clamped into [0, n_tokens) and runs into [0, n_rows), so nothing outside the caller's buffers is
 *                       touched, the result for broken input being unspecified.
 * pgx_annot_row_tile(): the ids of a row a lane group handles; a longer row goes to the long-row kernel.
 * pgx_annot_run_tile(): the rows of a run one wave handles; a longer run goes to the workgroup kernel. */
#define PGX_ANNOT_NARROW_HASH 1u  /* keep only the low 3 bits of every hash: same results, every probe collides */
uint32_t pgx_annot_row_tile(void);
uint32_t pgx_annot_run_tile(void);
size_t pgx_annot_vote_workspace_bytes(uint32_t n_rows, uint64_t n_tokens, uint32_t n_runs);
int pgx_annot_vote(pgx_ctx *ctx, const int32_t *tok, const uint64_t *row_off, uint32_t n_rows, const uint32_t *run_off,
                   uint32_t n_runs, uint32_t flags, uint8_t *out_keep, int32_t *out_winner, uint32_t *out_votes,
                   uint8_t *out_differs);
int pgx_annot_vote_dev(pgx_ctx *ctx, const int32_t *d_tok, const uint64_t *d_row_off, uint32_t n_rows, uint64_t n_tokens,
                       const uint32_t *d_run_off, uint32_t n_runs, uint32_t flags, uint8_t *d_keep, int32_t *d_winner,
                       uint32_t *d_votes, uint8_t *d_differs, void *d_workspace, size_t workspace_bytes, void *stream);

/* Shortest-path lengths from many sources to many targets of a directed graph: the device step of build_resistome and of
 * the drug-class terms of generate_probable_hits_from_annotations (reference amr.py:289-349 and :150-165, one nx.has_path or
 * nx.shortest_path per pair). The successors of node v are succ[succ_off[v] .. succ_off[v + 1]) (n_nodes + 1 offsets,
 * succ_off[0] = 0); self-loops, parallel edges and cycles are legal; sources and targets are node ids and may repeat, which
 * gives repeated rows or columns.
 *   len[s * n_targets + t] = the number of NODES on a shortest directed path from sources[s] to targets[t]: 1 when they are
 *                            the same node, 0 when there is no path (what len(nx.shortest_path(...)) returns, 0 for no path)
 *   rounds                 = 1 + the largest number of edges on a shortest path from ANY node to a target it reaches: the
 *                            rounds the device ran, the last one being the one that changed nothing
 * Every node holds a bit mask of the targets it reaches; a round pulls the successors' masks of the previous round into a
 * second buffer, so a bit that appears in round k stands for a path of k + 1 nodes. No atomics: both are functions of the
 * input alone and the same input gives the same bytes on every call.
 * n_nodes >= 2^24, 2^31 edges or more, n_nodes x ceil(n_targets / 64) >= 2^28, n_sources x n_targets >= 2^31, offsets that
 * decrease or do not start at 0, a successor, source or target outside [0, n_nodes) (host entry) and too small a workspace
 * fail with PGX_ERR_INVALID before anything is launched or written. n_sources = 0 or n_targets = 0 does nothing: no output
 * is written, out_rounds included.
 *   pgx_graph_reach      HOST pointers; out_rounds may be NULL; the device buffers stay in the context between calls
 *   pgx_graph_reach_dev  the caller's DEVICE pointers (4-byte aligned), n_edges given by the caller, d_out_rounds (one
 *                        uint32, may be NULL) and workspace (pgx_graph_reach_workspace_bytes(), 16-byte aligned; 0 for sizes
 *                        that are refused). Plain launches on `stream`, which is synchronised once per round -- the host
 *                        reads one word to learn whether anything changed -- and at the end; inputs are not written, nothing
 *                        outside the outputs and the workspace is. Offsets and ids are not checked: successor lists are
 *                        clamped into [0, n_edges) and an id that is not a node is skipped (as a successor it leads nowhere,
 *                        as a target nothing reaches it, as a source it reaches nothing), so nothing outside the caller's
 *                        buffers is touched, the result for broken offsets being unspecified. */
size_t pgx_graph_reach_workspace_bytes(uint32_t n_nodes, uint32_t n_targets, uint32_t n_sources);
int pgx_graph_reach(pgx_ctx *ctx, const uint32_t *succ_off, const uint32_t *succ, uint32_t n_nodes, const uint32_t *targets,
                    uint32_t n_targets, const uint32_t *sources, uint32_t n_sources, uint32_t *out_len, uint32_t *out_rounds);
int pgx_graph_reach_dev(pgx_ctx *ctx, const uint32_t *d_succ_off, const uint32_t *d_succ, uint32_t n_nodes, uint64_t n_edges,
                        const uint32_t *d_targets, uint32_t n_targets, const uint32_t *d_sources, uint32_t n_sources,
                        uint32_t *d_out_len, uint32_t *d_out_rounds, void *d_workspace, size_t workspace_bytes, void *stream);

/* Which of n_terms short patterns occur in each of n short strings: the device step of
 * generate_probable_hits_from_annotations (reference amr.py:196-230, Python's `in` for every annotation, drug and term).
 * String i is the length[i] bytes of `text` at start[i] (the windows of pgx_prox_cut: zero-length windows are legal, windows
 * may overlap or repeat); term t is the bytes terms[term_off[t] .. term_off[t + 1]) (n_terms + 1 offsets, term_off[0] = 0).
 *   bit (t & 63) of out_mask[i * W + (t >> 6)], W = ceil(n_terms / 64), is set iff term t occurs as a contiguous substring
 *   of string i; bits at or beyond n_terms are zero. The empty term occurs in every string, the empty one included.
 * With PGX_TERM_FOLD_ASCII the bytes 'A'-'Z' (0x41-0x5A) of strings and terms are compared as 'a'-'z'; no other byte is
 * changed: '@', '[', '`', '{' and bytes >= 0x80 are compared as they are. Every match is decided by a byte compare and no
 * atomics are used: the same input gives the same bytes on every call.
 * At most PGX_TERM_MAX_TERMS terms of PGX_TERM_MAX_BYTES bytes in all (they are kept in LDS). More than that, n >= 2^24,
 * text_bytes >= 2^32, unknown flags, offsets that decrease or do not start at 0 and a window that leaves [0, text_bytes)
 * (host entry) fail with PGX_ERR_INVALID before anything is launched or written. n = 0 or n_terms = 0 does nothing (there
 * are no words to write).
 *   pgx_term_scan      HOST pointers; the device buffers stay in the context between calls
 *   pgx_term_scan_dev  the caller's DEVICE pointers (d_start and d_out_mask 8-byte aligned, d_length and d_term_off 4-byte
 *                      aligned; text and terms may start at any address), term_bytes given by the caller. One launch on
 *                      `stream`, which is then synchronised; no workspace; inputs are not written, nothing outside
 *                      d_out_mask is. Windows and offsets are not checked: a window is clamped into [0, text_bytes) (cut
 *                      short at its end), term offsets into [0, term_bytes], and a term that ends before it starts is taken
 *                      as empty, so nothing outside the caller's buffers is read.
 * pgx_term_scan_group_bytes(): the bytes of a string the lanes that share it take per step (as start positions of matches;
 * a match may run over the end of its step). */
#define PGX_TERM_FOLD_ASCII 1u
#define PGX_TERM_MAX_TERMS 512u
#define PGX_TERM_MAX_BYTES 32768u
uint32_t pgx_term_scan_group_bytes(void);
int pgx_term_scan(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint64_t *start, const uint32_t *length,
                  uint32_t n, const uint8_t *terms, const uint32_t *term_off, uint32_t n_terms, uint32_t flags,
                  uint64_t *out_mask);
int pgx_term_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_start,
                      const uint32_t *d_length, uint32_t n, const uint8_t *d_terms, const uint32_t *d_term_off,
                      uint32_t n_terms, uint64_t term_bytes, uint32_t flags, uint64_t *d_out_mask, void *stream);

/* Exact grouping of fixed-width integer tuples: the device step of extract_primary_stnds and extract_mic_calls (reference
 * amr_inference.py:222-347, one value_counts per organism and drug and one collections.Counter per organism).
 * Record i is the k values cols[c * n + i], c = 0 .. k - 1 (column-major, n values per column); any int32 value is allowed.
 * Two records are equal iff they agree in all k columns.
 *   first[i]    = the smallest j with record j equal to record i
 *   count[i]    = the number of records equal to record i when first[i] == i, and 0 otherwise
 *   *n_distinct = the number of i with first[i] == i
 * All three are functions of the input alone: the same input gives the same bytes on every call. first is a minimum over a
 * set and count an integer sum; no atomic decides an order. Hashes only decide where to look -- a j is reported after all k
 * columns have been compared. PGX_TUPLE_NARROW_HASH (a test seam) keeps only the low 3 bits of every hash: same results,
 * every probe collides. k outside 1 .. PGX_TUPLE_MAX_COLUMNS, n >= 2^24, unknown flags and too small a workspace fail with
 * PGX_ERR_INVALID before anything is launched or written. n = 0 sets *n_distinct to 0.
 *   pgx_tuple_group      HOST pointers; the device buffers stay in the context between calls
 *   pgx_tuple_group_dev  the caller's DEVICE pointers (4-byte aligned) and workspace (pgx_tuple_group_workspace_bytes(),
 *                        16-byte aligned; 0 for sizes that are refused). Plain launches on `stream`, which is synchronised
 *                        once at the end; inputs are not written, nothing outside the outputs and the workspace is. */
#define PGX_TUPLE_NARROW_HASH 1u  /* keep only the low 3 bits of every hash: same results, every probe collides */
#define PGX_TUPLE_MAX_COLUMNS 8u
size_t pgx_tuple_group_workspace_bytes(uint32_t n, uint32_t k);
int pgx_tuple_group(pgx_ctx *ctx, const int32_t *cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *out_first,
                    uint32_t *out_count, uint32_t *out_n_distinct);
int pgx_tuple_group_dev(pgx_ctx *ctx, const int32_t *d_cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *d_first,
                        uint32_t *d_count, uint32_t *d_n_distinct, void *d_workspace, size_t workspace_bytes, void *stream);

/* SIR inference: the body of infer_sir (reference amr_inference.py:27-100) for n rows at once.
 * Case c (an organism x drug pair with reference MICs) has the class entries class_begin[c] .. class_begin[c + 1] (n_cases + 1
 * offsets, class_begin[0] = 0, class_begin[n_cases] = n_entries), in the order mic_ranges[entry] iterates. Class entry e:
 *   sir[e]   the code that is returned (>= 0);  role[e]  0 for 'susceptible', 1 for 'resistant', 2 for any other name
 *   fvals[fl_begin[e] .. fl_begin[e + 1])  its numeric MICs, sorted, no NaN (n_entries + 1 offsets, from 0 to n_fvals)
 *   tvals[tk_begin[e] .. tk_begin[e + 1])  the int32 codes of its string MICs, sorted (n_entries + 1 offsets, from 0 to n_tvals)
 * Row i:
 *   case[i]   its case, -1 for no case or no ranges
 *   sign[i]   0 equality, 1 '<' or '<=', 2 '>' or '>=', 3 neither
 *   combo[i]  the reference's is_likely_combo (0 or 1)
 *   kind[i]   0: a string measurement whose code is token[i], -1 for a string that is in no list; 1: a float measurement
 *             whose key is value[i], compared with ==, so that a NaN is never a member
 *   value[i]  float(measurement_value); read only when combo[i] == 0 or kind[i] == 1
 * A class entry TAKES a row when the row's key is a member of the entry's list (tvals for kind 0, fvals for kind 1) or, if
 * combo[i] == 0, when (role == 0 or value >= min) and (role == 1 or value <= max), min the first and max the last of the
 * entry's fvals, with IEEE comparisons (a NaN fails both).
 *   sign 0:  out[i] = sir[e] of the first entry of the case, in case order, that takes the row: a range hit of an earlier
 *            class beats a membership hit of a later one
 *   sign 1:  only the case's first entry of role 0 is tried; sign 2: only its first entry of role 1
 *   out[i] = -1 when no entry takes the row, the case is -1 or the sign is 3
 *   out[i] = -2 ("needs the host") when the range test would be evaluated on an entry that has a string MIC or no fvals:
 *            the reference raises TypeError or ValueError there
 * One launch, no atomics: the same input gives the same bytes on every call. n >= 2^31, and 2^24 or more cases, class
 * entries, fvals or tvals fail with PGX_ERR_INVALID before anything is launched or written, as do (host entry) offsets that
 * decrease or do not run from 0 to the stated totals, a role above 2, a negative sir code and a run that is not sorted or
 * holds a NaN. n = 0 does nothing.
 *   pgx_mic_infer      HOST pointers; the device buffers stay in the context between calls
 *   pgx_mic_infer_dev  the caller's DEVICE pointers (the doubles 8-byte aligned, the 32-bit arrays 4-byte aligned). One launch
 *                      on `stream`, which is then synchronised; no workspace; inputs are not written, nothing outside d_out
 *                      is. Offsets are not checked: every one is clamped to the array it points into and a case outside
 *                      [0, n_cases) is taken as -1, so nothing outside the caller's buffers is read, the result for broken
 *                      tables being unspecified. */
int pgx_mic_infer(pgx_ctx *ctx, const uint32_t *class_begin, uint32_t n_cases, const int32_t *sir, const uint8_t *role,
                  const uint32_t *fl_begin, const uint32_t *tk_begin, uint32_t n_entries, const double *fvals, uint32_t n_fvals,
                  const int32_t *tvals, uint32_t n_tvals, const int32_t *row_case, const uint8_t *sign, const uint8_t *combo,
                  const uint8_t *kind, const int32_t *token, const double *value, uint64_t n, int32_t *out);
int pgx_mic_infer_dev(pgx_ctx *ctx, const uint32_t *d_class_begin, uint32_t n_cases, const int32_t *d_sir, const uint8_t *d_role,
                      const uint32_t *d_fl_begin, const uint32_t *d_tk_begin, uint32_t n_entries, const double *d_fvals,
                      uint32_t n_fvals, const int32_t *d_tvals, uint32_t n_tvals, const int32_t *d_case, const uint8_t *d_sign,
                      const uint8_t *d_combo, const uint8_t *d_kind, const int32_t *d_token, const double *d_value, uint64_t n,
                      int32_t *d_out, void *stream);

/* Gene content of tree nodes: the device step of get_node_gene_content (reference weboflife.py:16-35, one gene per call) for
 * every gene of a table at once. The table is the presence bitmap of "K3" above with a species where it says genome: species
 * s owns pgx_bitmap_stride_words(n_genes) words, gene g is bit g & 63 of word g >> 6.
 *   leaf_species[n_nodes]   a species index >= 0: the node is MAPPED, and a leaf even where it has children, which are not
 *                           consulted; -1: unmapped. Two nodes may map to one species; a species may be mapped by none.
 *   child_off[n_nodes + 1], child[]   the children of node v are child[child_off[v] .. child_off[v + 1])
 *   order[n_nodes], level_off[n_levels + 1]   every node once, grouped by height: order[level_off[h] .. level_off[h + 1]) are
 *                           the nodes of height h. Height 0 holds the mapped nodes and the childless unmapped ones; any other
 *                           node has height 1 + the largest height among its children.
 *   out_counts[n_nodes][pgx_tree_content_stride(n_genes)]   (the stride is n_genes rounded up to a multiple of 4, so that rows
 *                           are 16-byte aligned; pad entries are zero.) For a mapped node v, out_counts[v][g] is the bit
 *                           (leaf_species[v], g); for a childless unmapped node 0; for any other node the sum of its
 *                           children's entries.
 *   out_totals[n_nodes]     may be NULL. 1 for a mapped node, 0 for a childless unmapped one, else the sum over the children.
 * out_counts[v][g] / out_totals[v] is the reference's value for node v and gene g (0 / 0 where it gives nan).
 * One launch per height on one stream, no atomics, integer sums in the children's order: the same input gives the same bytes
 * on every call. n_nodes x stride past 2^31 entries and more than 2^31 edges fail with PGX_ERR_INVALID, as do level offsets
 * that decrease or do not run from 0 to n_nodes; n_nodes = 0 does nothing.
 *   pgx_tree_content      HOST pointers; the table as COO records (row_of_record = the gene, species_of_record), built on the
 *                         device as for pgx_row_counts, duplicates reported through out_duplicates (may be NULL; the bitmap
 *                         holds a bit once, so a table with duplicates is not the 0/1 table the caller meant). The device
 *                         buffers stay in the context between calls. The tree is checked before anything is launched or
 *                         written, PGX_ERR_INVALID otherwise: offsets that decrease or do not start at 0; a child that is no
 *                         node; a node missing from or twice in `order`; a leaf_species below -1 or not below n_species; a
 *                         mapped node above height 0, or an unmapped node with children at height 0; a child of an unmapped
 *                         node that does not lie at a strictly lower height; a node that is a child of two nodes.
 *   pgx_tree_content_dev  the caller's DEVICE pointers (d_bits 8-byte, d_out_counts 16-byte, the others 4-byte aligned) and
 *                         workspace (pgx_tree_content_workspace_bytes(), 16-byte aligned; 0 for sizes that are refused; the
 *                         kernels keep nothing there today). level_off alone is HOST memory: it sizes the launches. Plain
 *                         launches on `stream`, which is not synchronised; inputs are not written, nothing outside the two
 *                         outputs is. The tree is not checked: an id that is no node or no species is skipped and offsets
 *                         are clamped to n_edges, so nothing outside the caller's buffers is read, the result for a broken
 *                         tree being unspecified. */
uint32_t pgx_tree_content_stride(uint32_t n_genes);
size_t pgx_tree_content_workspace_bytes(uint32_t n_nodes, uint32_t n_genes, uint64_t n_edges);
int pgx_tree_content(pgx_ctx *ctx, const int32_t *row_of_record, const int32_t *species_of_record, uint64_t n_records,
                     uint32_t n_genes, uint32_t n_species, const int32_t *leaf_species, const uint32_t *child_off,
                     const uint32_t *child, uint32_t n_nodes, const uint32_t *order, const uint32_t *level_off, uint32_t n_levels,
                     uint32_t *out_counts, uint32_t *out_totals, uint64_t *out_duplicates);
int pgx_tree_content_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_species,
                         const int32_t *d_leaf_species, const uint32_t *d_child_off, const uint32_t *d_child, uint32_t n_nodes,
                         uint64_t n_edges, const uint32_t *d_order, const uint32_t *level_off, uint32_t n_levels,
                         uint32_t *d_out_counts, uint32_t *d_out_totals, void *d_workspace, size_t workspace_bytes, void *stream);

/* Exact search for variable-length patterns in a text, with positions and counts (the primitive under pangenomix_amd.mlst; the
 * reference's pangenome_analysis.py:402-453 run_mlst shells out to an external program). Pattern k is the bytes
 * [pattern_offsets[k], pattern_offsets[k + 1]) of a blob (the conventions of pgx_dict_load: n + 1 offsets that never decrease,
 * the blob is the bytes [0, offsets[n])), L_k of them; text is text_bytes raw bytes;
 *   first[k] = the smallest i with text[i .. i + L_k) == pattern k, 0xFFFFFFFF for none
 *   count[k] = the number of such i; overlapping occurrences are each counted
 * Bytes are compared as bytes (no case folding, no alphabet, values >= 0x80 allowed); equal patterns given twice both get the
 * full answer. A pattern never matches past text_bytes and nothing at or beyond text_bytes is read. Both outputs are a minimum /
 * an integer sum over a set (atomicMin, atomicAdd, one lane per verified occurrence): the same input gives the same bytes on
 * every call. Only the first `seed` (1..64) bytes of a pattern are hashed, and hashes only decide where to look -- an
 * occurrence is counted after all L_k bytes have been compared -- so the result is exact; PGX_PATTERN_NARROW_HASH (a test
 * seam) keeps only the low 3 bits of every hash: same results, every position is verified against every pattern.
 * seed outside 1..64, text_bytes >= 2^32, n_patterns >= 2^24, unknown flags, too small or misaligned a workspace, and in the
 * host entries a blob of 2^32 bytes or more, decreasing offsets or a pattern shorter than seed fail with PGX_ERR_INVALID before
 * anything is launched or written. n_patterns = 0 does nothing; a text shorter than seed (text_bytes = 0 included) gives
 * first = 0xFFFFFFFF and count = 0 everywhere.
 *   pgx_pattern_load      HOST pointers: keeps the patterns, their offsets and their table in the context, replacing an
 *                         earlier set (a refused load leaves the earlier set loaded)
 *   pgx_pattern_query     HOST pointers: searches `text` for the set loaded last (PGX_ERR_INVALID without one), with the seed
 *                         and flags it was loaded with; any number of calls per load. out_first, out_count: [n_patterns]
 *   pgx_pattern_scan_dev  text, patterns, offsets (8-byte aligned), first and count (4-byte aligned) and the workspace
 *                         (pgx_pattern_workspace_bytes(), 16-byte aligned; 0 for sizes that are refused) are the caller's
 *                         DEVICE pointers; the text may start at any address. Plain launches on `stream`, which is
 *                         synchronised once at the end; inputs are not written, nothing outside first, count and the
 *                         workspace is. Device offsets are not checked, and the LAST offset is taken as the blob's size: the
 *                         kernels clamp every pattern into [0, last offset), so with a last offset inside the caller's
 *                         allocation nothing outside it is read whatever the other offsets hold. A pattern that is shorter
 *                         than seed after clamping matches nowhere; the result for broken offsets is otherwise unspecified.
 * pgx_pattern_scan_tile(): the text positions one workgroup takes at a time. */
#define PGX_PATTERN_NARROW_HASH 1u   /* keep only the low 3 bits of every hash: same results, every probe collides */
uint32_t pgx_pattern_scan_tile(void);
size_t pgx_pattern_workspace_bytes(uint64_t pattern_bytes, uint32_t n_patterns);
int pgx_pattern_load(pgx_ctx *ctx, const uint8_t *patterns, const uint64_t *pattern_offsets, uint32_t n_patterns, uint32_t seed,
                     uint32_t flags);
int pgx_pattern_query(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, uint32_t *out_first, uint32_t *out_count);
int pgx_pattern_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_patterns,
                         const uint64_t *d_pattern_offsets, uint32_t n_patterns, uint32_t seed, uint32_t flags,
                         uint32_t *d_first, uint32_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream);

/* Bounded-mismatch search for variable-length patterns in a text (the primitive under the novel-allele calls of
 * pangenomix_amd.mlst). Pattern k is the bytes [pattern_offsets[k], pattern_offsets[k + 1]) of a blob (the conventions of
 * pgx_pattern_load), L_k of them; max_mismatch[k] (uint8) is m_k; text is text_bytes raw bytes; separator is a byte value
 * 0..255 or PGX_NEAR_NO_SEPARATOR; active is one uint8 per pattern, or NULL for all patterns. A WINDOW of pattern k is a
 * position i with i + L_k <= text_bytes whose L_k text bytes do not hold `separator`, and
 *   d_k(i)  = #{ j : text[i + j] != pattern_k[j] }
 *   best[k] = min over windows i with d_k(i) <= m_k of (d_k(i) << 32 | i)
 *           = 0xFFFFFFFFFFFFFFFF when there is none, or when active[k] == 0
 * Bytes are compared as bytes (no case folding, no alphabet, values >= 0x80 allowed). A window never reaches past text_bytes
 * and nothing at or beyond text_bytes is read. best is a minimum over a set (a 64-bit atomicMin), so the same input gives the
 * same bytes on every call. Exact occurrences are included: d = 0, and the low word is then pgx_pattern_query's first. There
 * is NO occurrence count: a window is reached once for every indexed block that survived in it, and a sum would count it
 * that often.
 * The index: pattern k contributes its first m_k + 1 non-overlapping blocks of `block` (1..64) bytes, at offsets 0, block,
 * 2 * block, ... At most m_k mismatches cannot touch all m_k + 1 disjoint blocks, so every qualifying window holds at least
 * one of them exactly at its place and is found. Hashes only decide where to look -- a distance is counted over all L_k
 * bytes -- so the result is exact; PGX_NEAR_NARROW_HASH (a test seam) keeps only the low 3 bits of every hash: same results.
 * block outside 1..64, text_bytes >= 2^32, n_patterns >= 2^24, separator > 0x100, unknown flags, 2^30 blocks or more, too small
 * or misaligned a workspace, and in the host entries a blob of 2^32 bytes or more, decreasing offsets or a pattern with
 * (m_k + 1) * block > L_k fail with PGX_ERR_INVALID before anything is launched or written. n_patterns = 0 does nothing; a
 * text shorter than block (text_bytes = 0 included) gives all-ones everywhere.
 *   pgx_near_load      HOST pointers: keeps the patterns, their offsets, max_mismatch and the table in the context, replacing
 *                      an earlier set (a refused load leaves the earlier set loaded)
 *   pgx_near_query     HOST pointers: searches `text` for the set loaded last (PGX_ERR_INVALID without one), with the block
 *                      and flags it was loaded with; any number of calls per load. out_best: [n_patterns]
 *   pgx_near_scan_dev  text, patterns, offsets and best (8-byte aligned), max_mismatch, active (or NULL) and the workspace
 *                      (pgx_near_workspace_bytes(), 16-byte aligned; 0 for sizes that are refused) are the caller's DEVICE
 *                      pointers; the text may start at any address. n_blocks is the number of table entries the workspace was
 *                      sized for: the caller's sum of m_k + 1; blocks beyond it are not inserted. Plain launches on `stream`,
 *                      which is synchronised once at the end; no allocation; inputs are not written, nothing outside best and
 *                      the workspace is. Device offsets are not checked, and the LAST offset is taken as the blob's size: the
 *                      kernels clamp every pattern into [0, last offset) as pgx_pattern_scan_dev's do. A block that does not
 *                      fit its clamped pattern is not inserted; the result for such patterns is otherwise unspecified.
 * pgx_near_scan_tile(): the text positions one workgroup takes at a time. */
#define PGX_NEAR_NARROW_HASH 1u      /* keep only the low 3 bits of every hash: same results, every probe collides */
#define PGX_NEAR_NO_SEPARATOR 0x100u /* no byte value ends a window */
uint32_t pgx_near_scan_tile(void);
size_t pgx_near_workspace_bytes(uint64_t pattern_bytes, uint32_t n_patterns, uint64_t n_blocks);
int pgx_near_load(pgx_ctx *ctx, const uint8_t *patterns, const uint64_t *pattern_offsets, uint32_t n_patterns,
                  const uint8_t *max_mismatch, uint32_t block, uint32_t flags);
int pgx_near_query(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, uint32_t separator, const uint8_t *active,
                   uint64_t *out_best);
int pgx_near_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, uint32_t separator, const uint8_t *d_patterns,
                      const uint64_t *d_pattern_offsets, uint32_t n_patterns, const uint8_t *d_max_mismatch, uint32_t block,
                      uint64_t n_blocks, uint32_t flags, const uint8_t *d_active, uint64_t *d_best, void *d_workspace,
                      size_t workspace_bytes, void *stream);

/* Local alignment of pairs: Smith-Waterman with affine gaps on BLOSUM62, one best alignment per pair with its statistics
 * and no traceback (the primitive under pangenomix_amd.ncbi.bidirectional_blast; the rules are DESIGN.md 6t). Sequence k of a
 * set is the bytes [offsets[k], offsets[k + 1]) of its residues (offsets: n + 1 uint64, beginning with 0, not decreasing).
 * A byte is a LETTER: A-Z and a-z are the same 26 letters, every other byte is one 27th letter; a letter's class is
 * cluster_tables.h's (the 27th and J, O, U, X are class 20) and sub() is BLOSUM62 over the classes. Pair p aligns
 * q = sequence pair_a[p] of set 1 (m residues) with s = sequence pair_b[p] of set 2 (n residues); a gap of k costs 11 + k:
 *   E[i][j] = max(E[i][j-1] - 1, H[i][j-1] - 12)        F[i][j] = max(F[i-1][j] - 1, H[i-1][j] - 12)
 *   H[i][j] = max(0, H[i-1][j-1] + sub(q[i], s[j]), E[i][j], F[i][j])       borders: H = 0, E = F = minus infinity
 * On equal values the alternative written first wins (extension before opening; 0, diagonal, E, F). Every value carries the
 * statistics of the path it was chosen from: a diagonal step from a cell with H = 0 starts a path at (i, j); a diagonal step
 * adds a column and, for the same LETTER, an identity; an opening adds a column and a gap opening; an extension a column.
 * The result is the cell of maximum H, ties to the smallest i, then the smallest j:
 *   out[p] = { score, q_start, q_end, s_start, s_end, n_ident, n_cols, n_gapopen }    int32, positions 0-based inclusive
 * score, q_end and s_end are always written; the other five only where score >= min_score[p] and score > 0, and are 0
 * elsewhere (a score-only pass runs over every pair, the pass with statistics over those pairs alone). A pair with an empty
 * sequence gives eight zeros. No atomics: the same input gives the same bytes on every call.
 * A sequence of a pair longer than pgx_sw_max_length() (4,096), a pair index outside its set and decreasing offsets are
 * PGX_ERR_INVALID: the host entry finds them before anything is launched or written; the device entry's kernels skip such
 * a pair (eight zeros), never read outside what the offsets name, and the call then fails.
 *   pgx_sw_pairs      HOST pointers. Orders the pairs by the kernel's steps (longest first) before it launches.
 *   pgx_sw_pairs_dev  the caller's DEVICE pointers (offsets 8-byte, the other arrays 4-byte aligned) and stream; pairs run in
 *                     the caller's order. max_len: no sequence of a pair is longer (1..pgx_sw_max_length(); a longer one
 *                     is refused as above). Workspace: pgx_sw_workspace_bytes(ctx, n_pairs, max_len) bytes, 16-byte aligned
 *                     (0 for sizes that are refused). Plain launches on `stream`, which is synchronised once at the end; no
 *                     allocation; inputs are not written, nothing outside out and the workspace is.
 * pgx_sw_strip_width(): the query positions one lane group holds at a time (the kernel's strip).
 * pgx_sw_round_pairs(ctx, with_stats): the pairs that one round of the score pass (with_stats == 0) or of the pass with
 * statistics can hold on the context's device, for the tests: a longer list makes every lane group take a further pair per
 * round. 0 for a NULL ctx.
 * pgx_sw_last_stats_pairs(): how many pairs of the context's last call took the pass with statistics. */
uint32_t pgx_sw_max_length(void);
uint32_t pgx_sw_strip_width(void);
uint32_t pgx_sw_round_pairs(pgx_ctx *ctx, int with_stats);
size_t pgx_sw_workspace_bytes(pgx_ctx *ctx, uint32_t n_pairs, uint32_t max_len);
uint32_t pgx_sw_last_stats_pairs(pgx_ctx *ctx);
int pgx_sw_pairs(pgx_ctx *ctx, const uint8_t *residues1, const uint64_t *offsets1, uint32_t n1, const uint8_t *residues2,
                 const uint64_t *offsets2, uint32_t n2, const uint32_t *pair_a, const uint32_t *pair_b, uint32_t n_pairs,
                 const int32_t *min_score, int32_t *out);
int pgx_sw_pairs_dev(pgx_ctx *ctx, const uint8_t *d_residues1, const uint64_t *d_offsets1, uint32_t n1, const uint8_t *d_residues2,
                     const uint64_t *d_offsets2, uint32_t n2, const uint32_t *d_pair_a, const uint32_t *d_pair_b, uint32_t n_pairs,
                     const int32_t *d_min_score, uint32_t max_len, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                     void *stream);

/* feature names (pangenome.py:1944-1969) as fixed-width zero-padded ASCII records (numpy 'S<width>'):
 * <prefix><cluster>[<variant><member>]; variant NULL = gene names */
int pgx_format_labels(const char *prefix, const char *variant, const int32_t *cluster, const int32_t *member,
                      uint64_t n, uint32_t width, char *out);
/* the same names as numpy 'U<width>' records (UCS-4 code points, zero padded; prefix and variant ASCII, numbers >= 0,
 * width <= 64), written by several threads */
int pgx_format_labels_ucs4(const char *prefix, const char *variant, const int32_t *cluster, const int32_t *member,
                           uint64_t n, uint32_t width, uint32_t *out);

/* The two orderings of the feature tables (build_genetic_feature_tables, pangenome.py:563-680), host code:
 *   pgx_allele_order      out_order[i] = position of the i-th allele when the names <prefix><cluster><letter><member>
 *                         are sorted as strings (:615 sorts the names; here two stable radix passes over keys that
 *                         order integers like their decimal strings). cluster, member >= 0, n < 2^32.
 *   pgx_first_insertions  the triples a dictionary-of-keys matrix keeps when (rows[i], cols[i]) are set one after the
 *                         other (:649-650): out_first[0..*out_count) = ascending positions whose pair occurs there for
 *                         the first time (room for n entries). 0 <= cols[i] < n_cols, rows[i] >= 0. */
int pgx_allele_order(const int32_t *cluster, const int32_t *member, uint64_t n, int64_t *out_order);
/* Both tables' coordinates in one pass over a parsed set (the loops of pangenome.py:598-650 for inputs where every file is
 * one genome): cluster / member per non-redundant sequence as for pgx_fasta_write_clustered; file_order = the files in
 * the order their records are inserted (the reference walks sorted(paths)), genome_of_file = each file's column, both
 * permutations of 0..n_files-1. Out: allele_groups[i] = the sequence of allele row i (rows in pgx_allele_order's order),
 * gene_of_allele[i] = its gene row (room for n_groups each), *n_alleles, *n_genes; the COO triples of the allele and the
 * gene table in first-insertion order (a_row/a_col, g_row/g_col: room for n_records each; all values are 1);
 * lost_records = records that have no row (a sequence without a name, or one the clustering discarded), in
 * insertion order (room for n_records). */
int pgx_fasta_feature_coo(const pgx_fasta_set *fs, const int32_t *cluster, const int32_t *member, const int32_t *file_order,
                          const int32_t *genome_of_file, int64_t *allele_groups, int32_t *gene_of_allele, uint64_t *n_alleles,
                          uint64_t *n_genes, int32_t *a_row, int32_t *a_col, uint64_t *a_nnz, int32_t *g_row, int32_t *g_col,
                          uint64_t *g_nnz, int64_t *lost_records, uint64_t *n_lost);
int pgx_first_insertions(const int64_t *rows, const int64_t *cols, uint64_t n, uint64_t n_cols, int64_t *out_first,
                         uint64_t *out_count);

#ifdef __cplusplus
}
#endif
#endif /* PGX_H */
